"""CTC transcript scoring (dsmi_score) beside the kernels whose output it rescores: B = 32 clips of 10 s (501 frames) through a
synthetic cfgA model (2 conv, 5 x BiGRU 800, 33 labels), 1, 8 and 64 candidates of 150 characters per clip.

  python tools/exp/score_time.py [--reps 30] [--warmup 5] [--out profiles/score_time.txt]

In every repetition, one after the other (so that all figures see the same clock and the same neighbours on the host):
1. dsmi_score of 32, 256 and 2048 candidates, and of ONE candidate alone (one workgroup: the chain of 500 frames with nothing
   beside it -- the per-frame look): device events on the call's stream around the whole call (upload, kernel, result copy) and
   the host clock around it (the call synchronises).
2. dsmi_align of the batch (one transcript per clip) and dsmi_beam (width 64, no language model): device events.
3. The synchronous forward of the same batch: device events around DeepSpeech.forward.
Then, once, the float64 numpy reference (tests/_score_ref.py) over the 32 first candidates on the host, and the kernel's largest
share of the contract's bound against it.  Medians with min / max over --reps.  One JSON line per figure, printed and written."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _transcript(rng, n_chars, letters="abcdefghijklmnopqrstuvwxyzæøå"):
    words = []
    while len(" ".join(words)) < n_chars:
        words.append("".join(rng.choice(list(letters), size=int(rng.integers(2, 9)))))
    return " ".join(words)[:n_chars].strip()


def _spread(xs):
    xs = sorted(xs)
    return dict(median=round(xs[len(xs) // 2], 4), min=round(xs[0], 4), max=round(xs[-1], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--chars", type=int, default=150)
    ap.add_argument("--per-clip", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_time.txt"))
    a = ap.parse_args()
    import torch
    from danspeech_amd import Recognizer, synthetic as syn
    from danspeech_amd.deepspeech.model import DeepSpeech
    import _score_ref as ref
    assert torch.cuda.is_available(), "needs the GPU"
    sd = syn.make_state_dict(2, "gru", 800, 5, seed=0, fc_gain=8.0)
    model = DeepSpeech("cfgA", rnn_type="gru", rnn_hidden_size=800, rnn_layers=5, conv_layers=2).load_state_dict(sd)
    rec = Recognizer(model=model)
    eng = rec.danspeech_recognizer
    n = int(16000 * a.seconds)
    clips = [syn.make_clip(i, n) for i in range(a.batch)]
    rng = np.random.default_rng(7)
    most = max(a.per_clip)
    ids = [[eng.decoder.transcript_ids(eng.decoder.normalise_transcript(_transcript(rng, a.chars))) for _ in range(most)] for _ in range(a.batch)]
    feats, frames = eng.audio_parser.parse_batch(clips)
    lens = torch.from_numpy(frames.astype(np.int32))
    probs, sizes = eng.model.forward(feats, lens)
    torch.cuda.synchronize()
    dec = eng.decoder._dec(eng._device_index())
    sz = sizes.numpy().astype(np.int32)
    stream = torch.cuda.current_stream()

    def score_call(k):
        clip = [b for b in range(a.batch) for _ in range(k)]
        flat = [t for b in range(a.batch) for t in ids[b][:k]]
        return lambda: dec.score(probs, sz, clip, flat)

    calls = [("dsmi_score %d per clip" % k, score_call(k)) for k in a.per_clip]
    calls.append(("dsmi_score one candidate alone", lambda: dec.score(probs, sz, [0], [ids[0][0]])))
    calls.append(("dsmi_align", lambda: dec.align(probs, sz, [c[0] for c in ids])))
    calls.append(("dsmi_beam width 64 no LM", lambda: dec.beam(probs, sz, beam_width=64)))
    calls.append(("forward", lambda: eng.model.forward(feats, lens)))
    for _ in range(a.warmup):
        for _, fn in calls:
            fn()
    torch.cuda.synchronize()
    dev = {name: [] for name, _ in calls}
    host = {name: [] for name, _ in calls}
    for _ in range(a.reps):
        for name, fn in calls:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            h0 = time.perf_counter()
            fn()
            e1.record(stream)
            e1.synchronize()
            host[name].append((time.perf_counter() - h0) * 1e3)
            dev[name].append(e0.elapsed_time(e1))
    lines = [dict(figure=name, batch=a.batch, frames=int(sz.max()), chars=a.chars, reps=a.reps, device_events_ms=_spread(dev[name]),
                  host_clock_ms=_spread(host[name])) for name, _ in calls]
    one = _spread(dev["dsmi_score one candidate alone"])["median"]
    lines.append(dict(figure="per frame, one candidate alone", us_per_frame=round(one * 1e3 / int(sz[0]), 3), states=2 * len(ids[0][0]) + 1,
                      note="whole call over frames: an upper bound of the chain from barrier to barrier"))

    # ---- the numpy reference on the host, and agreement with the kernel
    lp, status = dec.score(probs, sz, np.arange(a.batch), [c[0] for c in ids])
    p_host = probs.cpu().numpy()
    h0 = time.perf_counter()
    want = [ref.forward(p_host[b, :sz[b]], list(ids[b][0])) for b in range(a.batch)]
    ref_ms = (time.perf_counter() - h0) * 1e3
    share = max(abs(float(lp[b]) - float(want[b])) / ref.bound(int(sz[b]), want[b]) for b in range(a.batch))
    lines.append(dict(figure="numpy_reference float64", candidates=a.batch, host_ms=round(ref_ms, 1), feasible=int((status == 0).sum()),
                      gpu_worst_share_of_bound=round(share, 5)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for d in lines:
            print(json.dumps(d), flush=True)
            f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
