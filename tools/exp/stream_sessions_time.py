"""Batched streaming passes (dsmi_stream_forward_many) against sequential single-session passes, CPUStreamingRNN shape
(2 conv, 5 x GRU 800 unidirectional, context 20) with seeded synthetic weights and 39-frame chunks.

  python tools/exp/stream_sessions_time.py [--ns 1,8,32,64,128,256] [--reps 20] [--trace-n N]

Per N: ms per batched pass (all N sessions advance by one 39-frame chunk = 0.39 s of audio each), ms for the same N
sessions advanced one after the other through dsmi_stream_forward, the speedup per session, and the sessions one GPU
sustains in real time (N * 390 ms / pass time at the largest N that stays under 390 ms).  Then stream_recordings end to end.
--trace-n N: only N's batched passes (for rocprofv3 --kernel-trace --stats: launches per pass)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", default="1,8,32,64,128,256")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trace-n", type=int, default=0)
    a = ap.parse_args()
    import torch
    from danspeech_amd import _native, synthetic as syn
    cfg = dict(conv_layers=2, rnn_type="gru", rnn_hidden_size=800, rnn_layers=5, bidirectional=False, context=20)
    sd = syn.make_state_dict(2, "gru", 800, 5, bidirectional=False, context=20, seed=5, fc_gain=4.0)
    m = _native.NativeModel(cfg, sd)
    x0 = torch.from_numpy(syn.make_features(1, 54, seed=1)).cuda()
    x = torch.from_numpy(syn.make_features(1, 39, seed=2)).cuda()

    def primed(n):
        sts = [_native.NativeStream(m) for _ in range(n)]
        _native.NativeStream.forward_many(sts, [x0] * n, [True] * n, [False] * n)
        _native.NativeStream.forward_many(sts, [x] * n, [False] * n, [False] * n)
        return sts

    ns = [a.trace_n] if a.trace_n else [int(v) for v in a.ns.split(",")]
    res = []
    for n in ns:
        sts = primed(n)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            _native.NativeStream.forward_many(sts, [x] * n, [False] * n, [False] * n)
        torch.cuda.synchronize()
        many = (time.perf_counter() - t0) / a.reps * 1e3
        row = dict(N=n, batched_ms=round(many, 3))
        if not a.trace_n:
            seq_reps = max(2, a.reps // max(1, n // 8))
            t0 = time.perf_counter()
            for _ in range(seq_reps):
                for st in sts:
                    st.forward(x, False, False)
            torch.cuda.synchronize()
            seq = (time.perf_counter() - t0) / seq_reps * 1e3
            row.update(sequential_ms=round(seq, 3), per_session_speedup=round(seq / many, 2),
                       pass_share_of_audio=round(many / 390.0, 4))
        res.append(row)
        print(json.dumps(row), flush=True)
        for st in sts:
            st.close()
    if a.trace_n:
        return
    fit = [r for r in res if r["batched_ms"] < 390.0]
    best = max(fit, key=lambda r: r["N"]) if fit else None
    if best:
        print(json.dumps(dict(sustained_realtime_sessions=int(best["N"] * 390.0 / best["batched_ms"]), at_N=best["N"],
                              note="N * 390 ms of audio per pass / pass time, at the largest N measured")))
    # stream_recordings end to end: 64 recordings of 10 s, 1024-sample parts
    from danspeech_amd import Recognizer
    from danspeech_amd.deepspeech.model import DeepSpeech
    dm = DeepSpeech("t", rnn_type="gru", rnn_hidden_size=800, rnn_layers=5, conv_layers=2, context=20, bidirectional=False,
                    streaming_inference_model=True).load_state_dict(sd)
    rec = Recognizer()
    rec.enable_real_time_streaming(streaming_model=dm)
    for nrec in (1, 64):
        audio = [syn.make_clip(i, 160000) for i in range(nrec)]
        list(rec.stream_recordings(audio[:1], chunk_samples=1024))
        t0 = time.perf_counter()
        out = list(rec.stream_recordings(audio, chunk_samples=1024))
        dt = time.perf_counter() - t0
        print(json.dumps(dict(stream_recordings=nrec, seconds_of_audio=10 * nrec, wall_s=round(dt, 3),
                              audio_s_per_s=round(10 * nrec / dt, 1), outputs=len(out))))


if __name__ == "__main__":
    main()
