"""LM sentence scoring (dsmi_lm_score) beside the host loop it stands in for and beside the calls it is used with: whole calls with
upload and copy back, all in one run.

  python tools/exp/lm_score_time.py [--reps 30] [--warmup 5] [--out profiles/lm_score_time.txt]

The workload: the 2048 hypotheses of 32 clips x 64-best x about 25 words over the order-3 synthetic ARPA model
(synthetic.make_arpa's defaults: 5000 words, 20000 n-grams per order), also as a KenLM probing binary; one sentence alone, and 32.
For each: dsmi_lm_score on prepared arrays with and without the terms (host clock around it: it synchronises), and a loop over
dsmi_lm_sentence_ln on prepared word ids -- what beam_score_out pays per hypothesis today, less its string work; the loop runs
through ctypes, whose cost per call is shown by the same loop over empty sentences; and dsmi_lm_score_plan, the segmentation alone
on the host, as a measure of the host's share of the call.  Beside them, on probabilities that spell the
32 base sentences: dsmi_score and dsmi_edit_distance (each hypothesis against its clip's base) of the same lists, dsmi_beam at
width 64 with the model, BeamCTCDecoder.rescore of the lists, and tune_lm_weights on a 9 x 9 grid against 81 beam searches (one
decode timed, times 81: a user would also reload the model at each grid point).  Medians with min / max over --reps.  One JSON
line per figure."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _spread(xs):
    xs = sorted(xs)
    return dict(median=round(xs[len(xs) // 2], 4), min=round(xs[0], 4), max=round(xs[-1], 4))


def _host_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        h0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - h0) * 1e3)
    return _spread(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lm_score_time.txt"))
    a = ap.parse_args()
    import torch
    from danspeech_amd import _native, synthetic as syn
    from danspeech_amd.deepspeech.decoder import BeamCTCDecoder
    from oracle import klm, lm as olm
    import _lm_score_ref as ref
    assert torch.cuda.is_available(), "needs the GPU"
    L = _native.lib()
    tmp = tempfile.mkdtemp()
    arpa = os.path.join(tmp, "lm3.arpa")
    syn.make_arpa(arpa, order=3)
    probing = os.path.join(tmp, "lm3.klm")
    klm.write_klm(arpa, probing, klm.PROBING)
    scorer = olm.Scorer(0.0, 0.0, arpa, ref.LABELS)
    rng = np.random.default_rng(7)
    vocab = [w for w in scorer.lm.vocab if w not in ref.SPECIAL]
    bases = []
    while len(bases) < 32:
        s = ref.sample_sentences(scorer, rng, 1, max_words=40, oov_every=25)[0]
        if len(s) >= 25:
            bases.append(s[:25])
    hyps = [[[vocab[int(rng.integers(0, len(vocab)))] if rng.random() < 0.08 else w for w in base] for _ in range(64)] for base in bases]
    ids = [[ref.label_ids(" ".join(h)) for h in row] for row in hyps]
    flat = [t for row in ids for t in row]
    lines = []
    d = BeamCTCDecoder(ref.LABELS, lm_path=arpa, alpha=0.8, beta=0.4, beam_width=64, blank_index=0)
    dec = d._dec(0)

    for kind, path in (("arpa (own table)", arpa), ("klm probing (looked up in place)", probing)):
        dec.set_lm(path, 0.8, 0.4)
        host = _native.NativeLM(path)
        word_ids = [np.array([host.word_index(w) for w in h], dtype=np.int32) for row in hyps for h in row]
        buf = np.zeros(64, dtype=np.float64)
        empty = np.zeros(1, dtype=np.int32)

        def host_loop(rows):
            return [L.dsmi_lm_sentence_ln(host._h, _native._np_ptr(w), len(w), _native._np_ptr(buf), 64) for w in rows]

        for name, rows, wids in (("one sentence", flat[:1], word_ids[:1]), ("32 sentences", flat[::64], word_ids[::64]), ("2048 sentences", flat, word_ids)):
            pool, lens = _native._padded_ids(rows, None, None, 0, None)
            got = dec.lm_score(pool, lens)
            assert got[0].tolist() == host_loop(wids), "the device and the host disagree"
            for terms in (False, True):
                lines.append(dict(figure="%s, dsmi_lm_score%s" % (name, " with terms" if terms else ""), model=kind, words=int(got[1].sum()), reps=a.reps,
                                  host_clock_ms=_host_ms(lambda: dec.lm_score(pool, lens, want_terms=terms), a.reps, a.warmup)))
            lines.append(dict(figure="%s, dsmi_lm_score_plan (host only: two passes over the tokens and its two output arrays; the call makes three passes)" % name, model=kind, reps=a.reps,
                              host_clock_ms=_host_ms(lambda: _native.lm_score_plan(pool, lens, space=ref.SPACE), a.reps, a.warmup)))
            lines.append(dict(figure="%s, the host loop over dsmi_lm_sentence_ln (ctypes)" % name, model=kind, reps=a.reps,
                              host_clock_ms=_host_ms(lambda: host_loop(wids), a.reps, a.warmup)))
            lines.append(dict(figure="%s, the same loop over EMPTY sentences (the cost of the calls themselves)" % name, model=kind, reps=a.reps,
                              host_clock_ms=_host_ms(lambda: [L.dsmi_lm_sentence_ln(host._h, _native._np_ptr(empty), 0, _native._np_ptr(buf), 64) for _ in wids], a.reps, a.warmup)))
        host.close()
    dec.set_lm(arpa, 0.8, 0.4)

    # ---- the neighbours, on probabilities that spell the base sentences under noise
    def spell(text, T):
        path = []
        for k, c in enumerate(text):
            path += ([0] if k and text[k - 1] == c else []) + [ref.LABELS.index(c)] * 2
        path += [0] * (T - len(path))
        z = rng.normal(size=(T, len(ref.LABELS)))
        z[np.arange(T), path] += 4.5
        p = np.exp(z - z.max(1, keepdims=True))
        return (p / p.sum(1, keepdims=True)).astype(np.float32)

    texts = [" ".join(b) for b in bases]
    frames = np.array([3 * len(t) + 8 for t in texts], dtype=np.int32)
    T = int(frames.max())
    probs = torch.from_numpy(np.stack([spell(t, T) for t in texts])).cuda()
    clip_of = [b for b in range(32) for _ in range(64)]
    table = {}
    word_pool = [d._risk_tokens(ref.label_ids(t), "word", table) for t in texts] + [d._risk_tokens(t, "word", table) for t in flat]
    pairs = np.stack([np.array(clip_of), 32 + np.arange(2048)], axis=1)
    logps = [[-50.0 - k for k in range(64)] for _ in range(32)]
    for name, fn in (("dsmi_score of the 2048 hypotheses", lambda: dec.score(probs, frames, clip_of, flat)),
                     ("dsmi_edit_distance, the 2048 hypotheses against their clip's base (words)", lambda: dec.edit_distance(word_pool, pairs)),
                     ("dsmi_beam width 64 with the model", lambda: dec.beam(probs, frames, beam_width=64)),
                     ("BeamCTCDecoder.decode (the search and its strings)", lambda: d.decode(probs, frames)),
                     ("BeamCTCDecoder.rescore of the 32 lists (ids in, one dsmi_lm_score, the order)", lambda: d.rescore(ids, logps))):
        lines.append(dict(figure=name, batch=32, frames=T, reps=a.reps, host_clock_ms=_host_ms(fn, a.reps, a.warmup)))
    grid = np.linspace(0.0, 2.0, 9)
    one = _host_ms(lambda: d.decode(probs, frames), a.reps, a.warmup)
    for n_best in (8, 64):
        r = max(3, a.reps // 5)
        lines.append(dict(figure="tune_lm_weights, 9 x 9 grid, 32 clips x %d-best (one search, one dsmi_score, one dsmi_lm_score, one dsmi_edit_distance, the grid)" % n_best,
                          reps=r, host_clock_ms=_host_ms(lambda: d.tune_lm_weights(probs, frames, texts, grid, grid, n_best=n_best), r, 1)))
    lines.append(dict(figure="81 beam searches (one BeamCTCDecoder.decode timed, times 81; reloading the model per grid point not counted)",
                      extrapolated_ms=round(81 * one["median"], 1)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for row in lines:
            print(json.dumps(row), flush=True)
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
