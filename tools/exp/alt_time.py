"""CTC token confidence (dsmi_alternatives) beside the only other way to the same numbers, dsmi_score over every variant
transcript, and beside the forward that made the probabilities: B = 32 clips of 10 s (501 frames) through a synthetic cfgA model
(2 conv, 5 x BiGRU 800, 33 labels), each with the transcript the model recognises in it -- the synthetic model's random weights
recognise only a token or two per clip -- and, the shape a subtitle line has, each with a random transcript of 150 characters.

  python tools/exp/alt_time.py [--reps 10] [--warmup 2] [--out profiles/alt_time.txt]

In every repetition, one after the other (so that all figures see the same clock and the same neighbours on the host):
For each of the two sets of transcripts:
1. dsmi_alternatives of the 32 transcripts in one call, and of ONE transcript alone (the chains of 500 frames with nothing beside
   them): device events on the call's stream around the whole call (upload, kernels, result copy) and the host clock around it
   (the call synchronises).
2. dsmi_score of all L * C variants of every transcript (token k replaced by each label, or deleted), in as few calls as its
   N * L_stride <= 2^24 allows; the candidate arrays are built before the clock starts.
and then the synchronous forward of the same batch.
Then, once per set, the largest distance between the two ways' numbers as a share of the sum of their bounds (8 T ... + 24 T ...), and the
number of variants that fit no more.  Medians with min / max over --reps.  One JSON line per figure, printed and written."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _spread(xs):
    xs = sorted(xs)
    return dict(median=round(xs[len(xs) // 2], 4), min=round(xs[0], 4), max=round(xs[-1], 4))


def _transcript(rng, n_chars, letters="abcdefghijklmnopqrstuvwxyzæøå"):
    words = []
    while len(" ".join(words)) < n_chars:
        words.append("".join(rng.choice(list(letters), size=int(rng.integers(2, 9)))))
    return " ".join(words)[:n_chars].strip()


def _variants(ids, C, blank):
    """Every (k, c) variant of every transcript as dsmi_score takes them: (clip [N], targets [N, L_max], lens [N])."""
    L_max = max(len(t) for t in ids)
    clip, rows, lens = [], [], []
    for b, t in enumerate(ids):
        t = np.asarray(t, dtype=np.int32)
        for k in range(len(t)):
            for c in range(C):
                row = np.zeros(L_max, dtype=np.int32)
                v = np.delete(t, k) if c == blank else np.concatenate((t[:k], [c], t[k + 1:]))
                row[:len(v)] = v
                clip.append(b)
                rows.append(row)
                lens.append(len(v))
    return np.array(clip, dtype=np.int32), np.array(rows, dtype=np.int32).reshape(len(clip), L_max), np.array(lens, dtype=np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--chars", type=int, default=150)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "alt_time.txt"))
    a = ap.parse_args()
    import torch
    from danspeech_amd import Recognizer, synthetic as syn
    from danspeech_amd.deepspeech.model import DeepSpeech
    import _alt_ref as alt_ref
    import _score_ref as ref
    assert torch.cuda.is_available(), "needs the GPU"
    sd = syn.make_state_dict(2, "gru", 800, 5, seed=0, fc_gain=8.0)
    model = DeepSpeech("cfgA", rnn_type="gru", rnn_hidden_size=800, rnn_layers=5, conv_layers=2).load_state_dict(sd)
    rec = Recognizer(model=model)
    eng = rec.danspeech_recognizer
    n = int(16000 * a.seconds)
    clips = [syn.make_clip(i, n) for i in range(a.batch)]
    feats, frames = eng.audio_parser.parse_batch(clips)
    lens = torch.from_numpy(frames.astype(np.int32))
    probs, sizes = eng.model.forward(feats, lens)
    torch.cuda.synchronize()
    dec = eng.decoder._dec(eng._device_index())
    sz = sizes.numpy().astype(np.int32)
    stream = torch.cuda.current_stream()
    C, blank = probs.shape[2], eng.decoder.blank_index
    rng = np.random.default_rng(7)
    sets = [("recognised transcripts", [np.asarray(t, dtype=np.int32) for t, _ in dec.greedy(probs, sz)]),
            ("%d-character transcripts" % a.chars,
             [eng.decoder.transcript_ids(eng.decoder.normalise_transcript(_transcript(rng, a.chars))) for _ in range(a.batch)])]
    calls, brutes, shapes = [], {}, {}
    for label, ids in sets:
        clip_v, rows_v, lens_v = _variants(ids, C, blank)
        N, L_max = rows_v.shape
        per_call = max(1, (1 << 24) // max(L_max, 1))
        cuts = list(range(0, N, per_call)) + [N]

        def brute(clip_v=clip_v, rows_v=rows_v, lens_v=lens_v, cuts=cuts):
            return np.concatenate([dec.score(probs, sz, clip_v[i:j], rows_v[i:j], lens_v[i:j])[0] for i, j in zip(cuts, cuts[1:])])

        brutes[label] = brute
        shapes[label] = dict(tokens=[int(min(len(t) for t in ids)), int(max(len(t) for t in ids))], variants=int(N), score_calls=len(cuts) - 1)
        calls.append(("dsmi_alternatives, the batch, " + label, lambda ids=ids: dec.alternatives(probs, sz, np.arange(a.batch), ids), label))
        calls.append(("dsmi_alternatives, one transcript alone, " + label, lambda ids=ids: dec.alternatives(probs, sz, [0], [ids[0]]), label))
        calls.append(("dsmi_score over every variant, the batch, " + label, brute, label))
    calls.append(("forward", lambda: eng.model.forward(feats, lens), None))
    for _ in range(a.warmup):
        for _, fn, _ in calls:
            fn()
    torch.cuda.synchronize()
    dev = {name: [] for name, _, _ in calls}
    host = {name: [] for name, _, _ in calls}
    for _ in range(a.reps):
        for name, fn, _ in calls:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            h0 = time.perf_counter()
            fn()
            e1.record(stream)
            e1.synchronize()
            host[name].append((time.perf_counter() - h0) * 1e3)
            dev[name].append(e0.elapsed_time(e1))
    lines = [dict(figure=name, device_events_ms=_spread(dev[name]), host_clock_ms=_spread(host[name]), batch=a.batch, frames=int(sz.max()),
                  labels=int(C), reps=a.reps, **(shapes[label] if label else {})) for name, _, label in calls]
    for label, ids in sets:
        fast = _spread(host["dsmi_alternatives, the batch, " + label])["median"]
        slow = _spread(host["dsmi_score over every variant, the batch, " + label])["median"]
        lines.append(dict(figure="dsmi_score over every variant / dsmi_alternatives, host clock medians, " + label, ratio=round(slow / fast, 2)))
        # ---- the two ways agree
        lp, alt, status = dec.alternatives(probs, sz, np.arange(a.batch), ids)
        direct = brutes[label]()
        worst, gone, i = 0.0, 0, 0
        for b, t in enumerate(ids):
            for k in range(len(t)):
                for c in range(C):
                    got, want = float(alt[b, k, c]), float(direct[i])
                    i += 1
                    if want == -np.inf or got == -np.inf:
                        assert got == want, (b, k, c, got, want)
                        gone += 1
                        continue
                    worst = max(worst, abs(got - want) / (ref.bound(int(sz[b]), want) + alt_ref.bound(int(sz[b]), want)))
        lines.append(dict(figure="agreement of the two ways, " + label, variants=i, fit_no_more=gone, feasible=int((status == 0).sum()),
                          worst_share_of_the_two_bounds=round(worst, 5)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for d in lines:
            print(json.dumps(d), flush=True)
            f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
