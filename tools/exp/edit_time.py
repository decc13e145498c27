"""Batched edit distance (dsmi_edit_distance) beside the Python loop it stands in for (Decoder.cer / Decoder.wer) and beside the
kernels whose output it compares: whole calls with upload and copy back, all in one run.

  python tools/exp/edit_time.py [--reps 30] [--warmup 5] [--out profiles/edit_time.txt]

The cases:
 (a) 32 CER pairs of 150 characters;
 (b) 32 WER pairs of 25 words;
 (c) the 64 512 pairs i < j of 32 clips x 64-best of about 150 characters (one pool of 2048 sequences, one call);
 (d) one pair of 4096 x 4096 tokens.
For each: the native call on prepared arrays (host clock around it: it synchronises), for (a) and (b) also Decoder.cer_batch /
wer_batch with strings in (tokenising included), and the Python loop on the same pairs -- for (c) on a stated sample of the
pairs, extrapolated; for (d) once.  Then dsmi_score of the same 2048 hypotheses, dsmi_beam at width 64 and the forward of the 32
clips behind them (a synthetic cfgA model), as tools/exp/score_time.py times them.  With the experiments library
(DSMI_LIBRARY=.../libdsmi_exp.so) every native case is also timed with the step's three lane moves through ds_bpermute
(DSMI_DEBUG_EDIT_MOVE=bpermute) in place of the DPP shifts.  Medians with min / max over --reps.  One JSON line per figure."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LETTERS = "abcdefghijklmnopqrstuvwxyzæøå"


def _text(rng, n_chars):
    words = []
    while len(" ".join(words)) < n_chars:
        words.append("".join(rng.choice(list(LETTERS), size=int(rng.integers(2, 9)))))
    return " ".join(words)[:n_chars].strip()


def _noisy(rng, text, rate):
    """``text`` with about ``rate`` of its characters replaced, dropped or doubled."""
    out = []
    for c in text:
        u = rng.random()
        if u < rate / 3:
            continue
        out.append(rng.choice(list(LETTERS)) if u < 2 * rate / 3 else c)
        if u > 1 - rate / 3:
            out.append(c)
    return "".join(out)


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
    ap.add_argument("--sample", type=int, default=64, help="pairs of case (c) that the Python loop is timed on")
    ap.add_argument("--cases", default="abcdn", help="which of the cases ab (together), c, d and n (the neighbours: score, beam, forward) to run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit_time.txt"))
    a = ap.parse_args()
    import torch
    from danspeech_amd import Recognizer, _native, synthetic as syn
    from danspeech_amd.deepspeech.model import DeepSpeech
    import _edit_ref as ref
    assert torch.cuda.is_available(), "needs the GPU"
    sd = syn.make_state_dict(2, "gru", 800, 5, seed=0, fc_gain=8.0)
    model = DeepSpeech("cfgA", rnn_type="gru", rnn_hidden_size=800, rnn_layers=5, conv_layers=2).load_state_dict(sd)
    rec = Recognizer(model=model)
    eng = rec.danspeech_recognizer
    d = eng.decoder
    dec = d._dec(eng._device_index())
    rng = np.random.default_rng(7)
    forms = ["dpp"] + (["bpermute"] if "exp" in os.path.basename(os.environ.get("DSMI_LIBRARY", "")) else [])
    lines = []

    def native_case(name, pool, pairs, lens=None, reps=a.reps):
        """The call's host clock (it synchronises), the forms alternating within each repetition."""
        if lens is None:                 # (prepared arrays: the padding of a list of sequences is not the call)
            pool, lens = _native._padded_ids(pool, None, None, 0, None)
        times = {form: [] for form in forms}
        for rep in range(a.warmup + reps):
            for form in forms:
                os.environ["DSMI_DEBUG_EDIT_MOVE"] = form
                h0 = time.perf_counter()
                got = dec.edit_distance(pool, pairs, lens)
                if rep >= a.warmup:
                    times[form].append((time.perf_counter() - h0) * 1e3)
        os.environ["DSMI_DEBUG_EDIT_MOVE"] = "dpp"
        for form in forms:
            lines.append(dict(figure="%s, dsmi_edit_distance" % name, lane_moves=form, pairs=len(pairs), reps=reps, host_clock_ms=_spread(times[form])))
        return got

    def chars(s):
        return np.array([ord(c) for c in s.replace(" ", "")], dtype=np.int32)

    # ---- (a) 32 CER pairs of 150 characters, (b) 32 WER pairs of 25 words
    if "a" in a.cases or "b" in a.cases:
        refs_a = [_text(rng, 150) for _ in range(32)]
        hyps_a = [_noisy(rng, t, 0.15) for t in refs_a]
        pairs32 = np.stack([np.arange(32), np.arange(32) + 32], axis=1)
        got = native_case("(a) 32 CER pairs of 150 characters", [chars(s) for s in refs_a + hyps_a], pairs32)
        loop = [d.cer(r, h) for r, h in zip(refs_a, hyps_a)]
        assert got[:, 0].tolist() == loop == d.cer_batch(refs_a, hyps_a)
        lines.append(dict(figure="(a), Decoder.cer_batch (strings in)", reps=a.reps, host_clock_ms=_host_ms(lambda: d.cer_batch(refs_a, hyps_a), a.reps, a.warmup)))
        lines.append(dict(figure="(a), the Python loop Decoder.cer", reps=5, host_clock_ms=_host_ms(lambda: [d.cer(r, h) for r, h in zip(refs_a, hyps_a)], 5, 1)))
        vocab = [_text(rng, 6).replace(" ", "") for _ in range(400)]
        refs_b = [" ".join(rng.choice(vocab, size=25)) for _ in range(32)]
        hyps_b = [" ".join(w if rng.random() > 0.2 else str(rng.choice(vocab)) for w in t.split()) for t in refs_b]
        table = {}
        pool_b = d._edit_tokens(refs_b, "word", table) + d._edit_tokens(hyps_b, "word", table)
        got = native_case("(b) 32 WER pairs of 25 words", pool_b, pairs32)
        assert got[:, 0].tolist() == [d.wer(r, h) for r, h in zip(refs_b, hyps_b)] == d.wer_batch(refs_b, hyps_b)
        lines.append(dict(figure="(b), Decoder.wer_batch (strings in)", reps=a.reps, host_clock_ms=_host_ms(lambda: d.wer_batch(refs_b, hyps_b), a.reps, a.warmup)))
        lines.append(dict(figure="(b), the Python loop Decoder.wer", reps=a.reps, host_clock_ms=_host_ms(lambda: [d.wer(r, h) for r, h in zip(refs_b, hyps_b)], a.reps, 1)))

    # ---- (c) 32 clips x 64-best of about 150 characters: every pair i < j of a clip's list, one pool, one call
    hyps_c = [[_noisy(rng, base, 0.08) for _ in range(64)] for base in (_text(rng, 150) for _ in range(32))]
    ids_c = [[d.transcript_ids(" ".join(t.split())) for t in row] for row in hyps_c]
    flat = [t for row in ids_c for t in row]
    iu = np.triu_indices(64, 1)
    pairs_c = np.concatenate([np.stack([iu[0] + 64 * b, iu[1] + 64 * b], axis=1) for b in range(32)])
    if "c" in a.cases:
        got = native_case("(c) 64512 pairs: 32 clips x 64-best x ~150 characters", flat, pairs_c, reps=max(5, a.reps // 3))
        pick = rng.choice(len(pairs_c), size=a.sample, replace=False)
        strs = [d._to_string(t) for t in flat]
        h0 = time.perf_counter()
        loop = [d.cer(strs[i], strs[j]) for i, j in pairs_c[pick]]
        sample_ms = (time.perf_counter() - h0) * 1e3
        assert (np.array(loop) == ref.counts_of([t[t != d.space_index] for t in flat], pairs_c[pick])[:, 0]).all()
        char_pool = [t[t != d.space_index] for t in flat]
        assert dec.edit_distance(char_pool, pairs_c[pick])[:, 0].tolist() == loop
        lines.append(dict(figure="(c), the Python loop Decoder.cer, EXTRAPOLATED from a sample", sample_pairs=a.sample, sample_ms=round(sample_ms, 2),
                          extrapolated_ms=round(sample_ms * len(pairs_c) / a.sample, 0), mean_tokens=round(float(np.mean([len(t) for t in flat])), 1)))
        lines.append(dict(figure="(c), Decoder.min_risk of the 32 lists (tokenising, the call, the risks)", unit="char", reps=5,
                          host_clock_ms=_host_ms(lambda: d.min_risk(ids_c, [[-1.0] * 64] * 32, unit="char"), 5, 1)))

    # ---- (d) one pair of 4096 x 4096
    if "d" in a.cases:
        big_a = rng.integers(0, 30, 4096)
        big_b = np.where(rng.random(4096) < 0.1, rng.integers(0, 30, 4096), big_a)
        got = native_case("(d) one pair of 4096 x 4096", [big_a, big_b], [(0, 1)], reps=max(5, a.reps // 3))
        h0 = time.perf_counter()
        from danspeech_amd.deepspeech.decoder import _edit_distance
        want = _edit_distance(big_a.tolist(), big_b.tolist())
        lines.append(dict(figure="(d), the Python loop _edit_distance, once", host_clock_ms=round((time.perf_counter() - h0) * 1e3, 0)))
        assert int(got[0, 0]) == want

    # ---- the neighbours: dsmi_score of the same 2048 hypotheses, dsmi_beam at width 64, the forward
    if "n" in a.cases:
        clips = [syn.make_clip(i, 160000) for i in range(32)]
        feats, frames = eng.audio_parser.parse_batch(clips)
        lens = torch.from_numpy(frames.astype(np.int32))
        probs, sizes = eng.model.forward(feats, lens)
        torch.cuda.synchronize()
        sz = sizes.numpy().astype(np.int32)
        clip_of = [b for b in range(32) for _ in range(64)]
        for name, fn in (("dsmi_score of the 2048 hypotheses", lambda: dec.score(probs, sz, clip_of, flat)),
                         ("dsmi_beam width 64 no LM", lambda: dec.beam(probs, sz, beam_width=64)),
                         ("forward", lambda: (eng.model.forward(feats, lens), torch.cuda.synchronize()))):
            lines.append(dict(figure=name, batch=32, frames=int(sz.max()), reps=a.reps, host_clock_ms=_host_ms(fn, a.reps, a.warmup)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for row in lines:
            print(json.dumps(row), flush=True)
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
