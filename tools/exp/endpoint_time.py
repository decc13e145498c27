"""One round of live sessions through the energy gate (dsmi_endpointer_push_many) beside the passes it feeds.

  python tools/exp/endpoint_time.py [--reps 100] [--warmup 10] [--out FILE]
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/exp/endpoint_time.py --trace        (a run of its own)
  python tools/exp/endpoint_time.py --trace-report DIR/.../*_results.db

A round: N = 1 / 8 / 32 / 64 / 128 / 256 sessions (chunk 1024, the reference's thresholds), each with 6 x 1024 new int16 samples
already on the device.  The audio is loud throughout, so every session is inside a phrase and every buffer is emitted: the gather
moves all the samples, the most a round can cost.  Per N, in the same run:

  push_many       the round through _native.NativeEndpointer.push_many (wall time: the call synchronises the stream once)
  native call     dsmi_endpointer_push_many alone, its arguments built beforehand (what a C host pays)
  (a) singles     the same round as N single-session pushes
  (b) the passes  dsmi_features_stream_many of N chunks of 6240 float64 samples (39 frames) and dsmi_stream_forward_many of the
                  N x 39 frames through 5 x GRU 800, context 20: the round the gate's samples feed

Medians with min / max over --reps rounds after --warmup.  --trace runs 50 rounds at N = 8 and at N = 256 and nothing else, for the
profiler to count the dispatches per push; --trace-report prints those counts from the database rocprofv3 wrote, one JSON line per
kernel and grid height.  profiles/endpoint.txt is the output of the three runs, one after the other."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

CHUNK, NEW = 1024, 6 * 1024


def _spread(xs):
    xs = sorted(xs)
    return dict(median=round(xs[len(xs) // 2], 4), min=round(xs[0], 4), max=round(xs[-1], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--ns", default="1,8,32,64,128,256")
    ap.add_argument("--out", default="")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--trace-report", default="", metavar="DB")
    a = ap.parse_args()
    if a.trace_report:
        import sqlite3
        db = sqlite3.connect(a.trace_report)
        q = ("select name, grid_y / workgroup_y, count(*), avg(duration) / 1000.0, min(duration) / 1000.0, max(duration) / 1000.0 "
             "from kernels group by name, grid_y order by name, grid_y")
        for name, rows, calls, avg, lo, hi in db.execute(q):
            print(json.dumps(dict(figure="kernel trace", kernel=name, grid_y=rows, dispatches=calls,
                                  us=dict(avg=round(avg, 2), min=round(lo, 2), max=round(hi, 2)))))
        return
    import torch
    from danspeech_amd import _native, synthetic as syn
    assert torch.cuda.is_available(), "needs the GPU"
    fe = _native.NativeFrontend()
    rng = np.random.default_rng(4)
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)

    def setup(n):
        pcm = torch.from_numpy(rng.integers(-3000, 3001, size=(n, NEW), dtype=np.int16)).cuda()
        eps = [_native.NativeEndpointer(fe, CHUNK, 16000) for _ in range(n)]
        return pcm, eps

    if a.trace:
        for n in (8, 256):
            pcm, eps = setup(n)
            for _ in range(50):
                _native.NativeEndpointer.push_many(eps, [pcm[i] for i in range(n)], [False] * n)
            torch.cuda.synchronize()
            print("traced 50 pushes of N = %d" % n)
            for e in eps:
                e.close()
        return

    def timed(fn):
        """wall ms per call, the device idle before and after"""
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return _spread(ms)

    cfg = dict(conv_layers=2, rnn_type="gru", rnn_hidden_size=800, rnn_layers=5, bidirectional=False, context=20)
    model = _native.NativeModel(cfg, syn.make_state_dict(2, "gru", 800, 5, bidirectional=False, context=20, seed=5, fc_gain=4.0))
    x0 = torch.from_numpy(syn.make_features(1, 54, seed=1)).cuda()
    x = torch.from_numpy(syn.make_features(1, 39, seed=2)).cuda()
    L = _native.lib()
    for n in [int(v) for v in a.ns.split(",")]:
        pcm, eps = setup(n)
        chunks = [pcm[i] for i in range(n)]
        flags = [False] * n
        gate = timed(lambda: _native.NativeEndpointer.push_many(eps, chunks, flags))
        emit(dict(figure="push_many", sessions=n, ms=gate))
        # the library call alone: every session holds at most one kept run and is given NEW samples
        hs = (C.c_void_p * n)(*[e._h for e in eps])
        pp = (C.c_void_p * n)(*[c.data_ptr() for c in chunks])
        ns = np.full(n, NEW, dtype=np.int64); eos = np.zeros(n, dtype=np.int32)
        cap_out, cap_seg = n * (NEW + 8 * CHUNK), n * (NEW // CHUNK + 2)
        out = torch.empty(cap_out, dtype=torch.float64, device="cuda")
        ss = np.zeros(cap_seg, dtype=np.int32); sl = np.zeros(cap_seg, dtype=np.int64); sla = np.zeros(cap_seg, dtype=np.int32)
        found = C.c_int(0)

        def native_call():
            rc = L.dsmi_endpointer_push_many(hs, n, pp, ns.ctypes.data, eos.ctypes.data, out.data_ptr(), cap_out, ss.ctypes.data, sl.ctypes.data,
                                             sla.ctypes.data, cap_seg, C.byref(found), None, None)
            assert rc == 0, L.dsmi_endpointer_last_error(None)
        raw = timed(native_call)
        emit(dict(figure="native call", sessions=n, ms=raw, segments=found.value, samples_out=int(sl[:found.value].sum())))
        single = timed(lambda: [e.push(c) for e, c in zip(eps, chunks)])
        emit(dict(figure="(a) single pushes", sessions=n, ms=single))
        for e in eps:
            e.close()
        feats_in = [torch.from_numpy(np.rint(3000.0 * rng.standard_normal(6240))).cuda() for _ in range(n)]
        states = [np.zeros(3) for _ in range(n)]
        feat = timed(lambda: fe.features_stream_many(feats_in, states))
        sts = [_native.NativeStream(model) for _ in range(n)]
        _native.NativeStream.forward_many(sts, [x0] * n, [True] * n, [False] * n)
        fwd = timed(lambda: _native.NativeStream.forward_many(sts, [x] * n, [False] * n, [False] * n))
        for st in sts:
            st.close()
        both = feat["median"] + fwd["median"]
        emit(dict(figure="(b) the passes", sessions=n, features_stream_many_ms=feat, stream_forward_many_ms=fwd,
                  gate_share_of_passes=dict(push_many=round(gate["median"] / both, 4), native_call=round(raw["median"] / both, 4))))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
