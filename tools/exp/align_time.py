"""CTC forced alignment (dsmi_align) against the forward that produced its probabilities: B = 32 clips of 10 s through a
synthetic cfgA model (2 conv, 5 x BiGRU 800, 33 labels), each aligned to a seeded random transcript of about 150 characters.

  python tools/exp/align_time.py [--reps 50] [--warmup 5] [--out DIR]

1. dsmi_align of the batch: device events on the call's stream around the whole call (target upload, kernel, result copies)
   and the host clock around it (the call synchronises).
2. The forward of the same batch (spectrograms already on the device): device events around DeepSpeech.forward.
3. The float32 numpy reference (tests/_align_ref.py) over the same batch on the host.
Medians with min / max over --reps (the reference: 3 runs).  Prints one JSON line per figure."""
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
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--chars", type=int, default=150)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from danspeech_amd import Recognizer, synthetic as syn
    from danspeech_amd.deepspeech.model import DeepSpeech
    import _align_ref as ref
    assert torch.cuda.is_available(), "needs the GPU"
    sd = syn.make_state_dict(2, "gru", 800, 5, seed=0, fc_gain=8.0)
    model = DeepSpeech("cfgA", rnn_type="gru", rnn_hidden_size=800, rnn_layers=5, conv_layers=2).load_state_dict(sd)
    rec = Recognizer(model=model)
    eng = rec.danspeech_recognizer
    n = int(16000 * a.seconds)
    clips = [syn.make_clip(i, n) for i in range(a.batch)]
    rng = np.random.default_rng(7)
    texts = [_transcript(rng, a.chars) for _ in range(a.batch)]
    ids = [eng.decoder.transcript_ids(eng.decoder.normalise_transcript(t)) for t in texts]
    feats, frames = eng.audio_parser.parse_batch(clips)
    lens = torch.from_numpy(frames.astype(np.int32))
    probs, sizes = eng.model.forward(feats, lens)
    torch.cuda.synchronize()
    dec = eng.decoder._dec(eng._device_index())
    sz = sizes.numpy().astype(np.int32)
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)

    # ---- 1. alignment
    for _ in range(a.warmup):
        spans, tp, lp, status = dec.align(probs, sz, ids)
    assert not status.any()
    dev_ms, host_ms = [], []
    stream = torch.cuda.current_stream()
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        h0 = time.perf_counter()
        dec.align(probs, sz, ids)
        h1 = time.perf_counter()
        e1.record(stream)
        e1.synchronize()
        dev_ms.append(e0.elapsed_time(e1))
        host_ms.append((h1 - h0) * 1e3)
    emit(dict(figure="dsmi_align", batch=a.batch, seconds=a.seconds, frames=int(sz.max()), chars=int(max(len(t) for t in ids)),
              device_events_ms=_spread(dev_ms), host_clock_ms=_spread(host_ms)))

    # ---- 2. the forward of the same batch
    for _ in range(a.warmup):
        eng.model.forward(feats, lens)
    torch.cuda.synchronize()
    fw = []
    for _ in range(max(10, a.reps // 5)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        eng.model.forward(feats, lens)
        e1.record(stream)
        e1.synchronize()
        fw.append(e0.elapsed_time(e1))
    emit(dict(figure="forward", batch=a.batch, seconds=a.seconds, model="cfgA 2 conv + 5 x BiGRU 800", device_events_ms=_spread(fw)))

    # ---- 3. the numpy reference on the host, and agreement with the kernel
    p_host = probs.cpu().numpy()
    runs = []
    for _ in range(3):
        h0 = time.perf_counter()
        res = [ref.viterbi(p_host[b, :sz[b]], list(ids[b])) for b in range(a.batch)]
        runs.append((time.perf_counter() - h0) * 1e3)
    same_spans = all(np.array_equal(spans[b, :len(ids[b])], res[b]["spans"]) for b in range(a.batch))
    max_dlogp = max(abs(float(lp[b]) - float(res[b]["path_logp"])) for b in range(a.batch))
    emit(dict(figure="numpy_reference", batch=a.batch, host_ms=_spread(runs), spans_equal=same_spans, max_abs_dlogp=max_dlogp))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "align_time.jsonl"), "w") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
