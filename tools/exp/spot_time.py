"""CTC phrase search (dsmi_spot) against the alignment and the forward of the same batch: B = 32 clips of 10 s through a
synthetic cfgA model (2 conv, 5 x BiGRU 800, 33 labels), searched for 1, 8 and 64 seeded random phrases of 10 characters.

  python tools/exp/spot_time.py [--reps 50] [--warmup 5] [--out DIR]

1. dsmi_spot of the batch for each phrase count: device events on the call's stream around the whole call (upload of the packed
   phrases, both kernels, the copy of the hits) and the host clock around it (the call synchronises).
2. dsmi_align of the same batch (seeded random transcripts of 150 characters, as tools/exp/align_time.py) and the forward of
   the same batch, measured again in this run: the yardsticks.
3. The float32 numpy reference (tests/_spot_ref.py) over the first 4 clips x 8 phrases on the host, and agreement with the
   kernel's tracks and hits.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _spread(xs):
    xs = sorted(xs)
    return dict(median=round(xs[len(xs) // 2], 4), min=round(xs[0], 4), max=round(xs[-1], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--chars", type=int, default=10)
    ap.add_argument("--max-hits", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from danspeech_amd import Recognizer, _native, synthetic as syn
    from danspeech_amd.deepspeech.model import DeepSpeech
    from align_time import _transcript
    import _spot_ref as ref
    assert torch.cuda.is_available(), "needs the GPU"
    sd = syn.make_state_dict(2, "gru", 800, 5, seed=0, fc_gain=8.0)
    model = DeepSpeech("cfgA", rnn_type="gru", rnn_hidden_size=800, rnn_layers=5, conv_layers=2).load_state_dict(sd)
    rec = Recognizer(model=model)
    eng = rec.danspeech_recognizer
    n = int(16000 * a.seconds)
    clips = [syn.make_clip(i, n) for i in range(a.batch)]
    rng = np.random.default_rng(7)
    letters = [i for i, c in enumerate(eng.decoder.labels) if i != eng.decoder.blank_index and c != " "]
    phrases = [[int(x) for x in rng.choice(letters, size=a.chars)] for _ in range(64)]
    feats, frames = eng.audio_parser.parse_batch(clips)
    lens = torch.from_numpy(frames.astype(np.int32))
    probs, sizes = eng.model.forward(feats, lens)
    torch.cuda.synchronize()
    dec = eng.decoder._dec(eng._device_index())
    sz = sizes.numpy().astype(np.int32)
    stream = torch.cuda.current_stream()
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)

    def timed(fn, reps):
        dev_ms, host_ms = [], []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            h0 = time.perf_counter()
            fn()
            h1 = time.perf_counter()
            e1.record(stream)
            e1.synchronize()
            dev_ms.append(e0.elapsed_time(e1))
            host_ms.append((h1 - h0) * 1e3)
        return _spread(dev_ms), _spread(host_ms)

    # ---- 1. the search, for 1, 8 and 64 phrases
    for K in (1, 8, 64):
        groups = _native.spot_plan([a.chars] * K)[0]
        for _ in range(a.warmup):
            dec.spot(probs, sz, phrases[:K], a.max_hits, -np.inf)
        dev, host = timed(lambda: dec.spot(probs, sz, phrases[:K], a.max_hits, -np.inf), a.reps)
        emit(dict(figure="dsmi_spot", batch=a.batch, seconds=a.seconds, frames=int(sz.max()), phrases=K, chars=a.chars, groups=groups,
                  max_hits=a.max_hits, device_events_ms=dev, host_clock_ms=host))

    # ---- 2. the yardsticks, again in this run: the alignment and the forward of the same batch
    texts = [_transcript(rng, 150) for _ in range(a.batch)]
    ids = [eng.decoder.transcript_ids(eng.decoder.normalise_transcript(t)) for t in texts]
    for _ in range(a.warmup):
        dec.align(probs, sz, ids)
    dev, host = timed(lambda: dec.align(probs, sz, ids), a.reps)
    emit(dict(figure="dsmi_align", batch=a.batch, seconds=a.seconds, frames=int(sz.max()), chars=150, device_events_ms=dev, host_clock_ms=host))
    for _ in range(a.warmup):
        eng.model.forward(feats, lens)
    torch.cuda.synchronize()
    dev, _ = timed(lambda: eng.model.forward(feats, lens), max(10, a.reps // 5))
    emit(dict(figure="forward", batch=a.batch, seconds=a.seconds, model="cfgA 2 conv + 5 x BiGRU 800", device_events_ms=dev))

    # ---- 3. the numpy reference on the host, and agreement with the kernel
    nb, nk = min(4, a.batch), 8
    hits, scores, counts, E, ST = dec.spot(probs[:nb].contiguous(), sz[:nb], phrases[:nk], a.max_hits, -np.inf, tracks=True)
    p_host = probs[:nb].cpu().numpy()
    runs = []
    for _ in range(3):
        h0 = time.perf_counter()
        res = [[ref.tracks(p_host[b, :sz[b]], phrases[k]) for k in range(nk)] for b in range(nb)]
        runs.append((time.perf_counter() - h0) * 1e3)
    finite = [np.isfinite(res[b][k][0]) for b in range(nb) for k in range(nk)]
    dE = max(float(np.abs(E[b, k, :sz[b]][finite[b * nk + k]] - res[b][k][0][finite[b * nk + k]]).max()) for b in range(nb) for k in range(nk))
    same_starts = all(np.array_equal(ST[b, k, :sz[b]], res[b][k][1]) for b in range(nb) for k in range(nk))
    same_hits = all([(s, e) for s, e, _ in ref.pick(E[b, k, :sz[b]], ST[b, k, :sz[b]], a.max_hits)] ==
                    [tuple(int(x) for x in hits[b, k, i]) for i in range(counts[b, k])] for b in range(nb) for k in range(nk))
    emit(dict(figure="numpy_reference", clips=nb, phrases=nk, host_ms=_spread(runs), starts_equal=same_starts, max_abs_dE=dE,
              hits_equal_pick_of_tracks=same_hits))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "spot_time.jsonl"), "w") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
