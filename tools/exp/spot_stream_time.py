"""The streaming phrase watch (dsmi_spot_stream_advance_many) on the streaming shape: 33 labels, 39-frame chunks of seeded peaky
probabilities, K random phrases of 3 to 12 labels, sessions 10 s (500 output frames) into their utterances.

  python tools/exp/spot_stream_time.py [--ns 1,64,256] [--ks 1,8,64] [--reps 20] [--trace-n N]

Per (N, K), in the same run:
  watch_ms      one round: N sessions advance by one 39-frame chunk in ONE dsmi_spot_stream_advance_many (events copied back);
  respot_ms     what it replaces: dsmi_spot over each session's utterance-so-far (500 frames, max_hits 4), one call per session
                as a caller without the watch would make them (two launches each);
  respot_batch_ms  the same work as ONE dsmi_spot call over the N utterances-so-far held as a batch [N, 500, 33];
and per N:
  forward_ms    the round it rides beside: dsmi_stream_forward_many of the N sessions' 39-frame chunks (CPUStreamingRNN shape:
                2 conv, 5 x GRU 800 unidirectional, context 20, synthetic weights).
Host clock around calls that end in a device synchronisation; medians over --reps.  Prints one JSON line per figure.
--trace-n N: only N's watch rounds at K = 8 (for rocprofv3 --kernel-trace --stats: launches per round)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def _probs(T, seed, C=33):
    rng = np.random.default_rng(seed)
    logits = rng.standard_normal((T, C)) * 3.0
    logits[:, 0] += 1.5
    e = np.exp(logits - logits.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", default="1,64,256")
    ap.add_argument("--ks", default="1,8,64")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trace-n", type=int, default=0)
    a = ap.parse_args()
    import torch
    from danspeech_amd import _native, synthetic as syn
    assert torch.cuda.is_available(), "needs the GPU"
    dec = _native.NativeDecoder(syn.DANSPEECH_LABELS, blank_index=0)
    CH, SOFAR = 39, 500
    floor, settle = float(np.log(0.5)), 25
    rng = np.random.default_rng(3)

    def timed(fn, reps):
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return round(float(np.median(ts)), 4)

    ns = [a.trace_n] if a.trace_n else [int(v) for v in a.ns.split(",")]
    ks = [8] if a.trace_n else [int(v) for v in a.ks.split(",")]
    base = [torch.from_numpy(_probs(SOFAR + CH * (a.reps + 2), 100 + i)).cuda() for i in range(16)]
    model = x0 = x = None
    for n in ns:
        p = [base[i % 16] for i in range(n)]
        for K in ks:
            phrases = [[int(v) for v in rng.integers(1, 33, size=int(rng.integers(3, 13)))] for _ in range(K)]
            watch = _native.NativeSpotWatch(dec, phrases, floor, settle)
            sts = [_native.NativeSpotStream(watch) for _ in range(n)]
            _native.NativeSpotStream.advance_many_counts(sts, [q[:SOFAR] for q in p], [False] * n, 4)      # 10 s in
            pos = [SOFAR]

            def round_():
                _native.NativeSpotStream.advance_many_counts(sts, [q[pos[0]:pos[0] + CH] for q in p], [False] * n, 4)
                pos[0] += CH
            round_()
            watch_ms = timed(round_, a.reps)
            row = dict(figure="round", sessions=n, phrases=K, groups=watch.n_groups, frames_per_chunk=CH, watch_ms=watch_ms)
            if not a.trace_n:
                sofar = torch.stack([q[:SOFAR] for q in p]).contiguous()
                few = max(2, a.reps // max(1, n // 8))
                row["respot_ms"] = timed(lambda: [dec.spot(sofar[i:i + 1], None, phrases, 4, floor) for i in range(n)], few)
                row["respot_batch_ms"] = timed(lambda: dec.spot(sofar, None, phrases, 4, floor), few)
            print(json.dumps(row), flush=True)
            for s in sts:
                s.close()
            watch.close()
        if a.trace_n:
            continue
        if model is None:
            cfg = dict(conv_layers=2, rnn_type="gru", rnn_hidden_size=800, rnn_layers=5, bidirectional=False, context=20)
            model = _native.NativeModel(cfg, syn.make_state_dict(2, "gru", 800, 5, bidirectional=False, context=20, seed=5, fc_gain=4.0))
            x0 = torch.from_numpy(syn.make_features(1, 54, seed=1)).cuda()
            x = torch.from_numpy(syn.make_features(1, 39, seed=2)).cuda()
        fw = [_native.NativeStream(model) for _ in range(n)]
        _native.NativeStream.forward_many(fw, [x0] * n, [True] * n, [False] * n)
        _native.NativeStream.forward_many(fw, [x] * n, [False] * n, [False] * n)
        print(json.dumps(dict(figure="forward", sessions=n, frames_per_chunk=CH,
                              forward_ms=timed(lambda: _native.NativeStream.forward_many(fw, [x] * n, [False] * n, [False] * n), a.reps))), flush=True)
        for s in fw:
            s.close()


if __name__ == "__main__":
    main()
