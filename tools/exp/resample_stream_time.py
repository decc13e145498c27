"""One round of live sessions through the chunked resampler (dsmi_resampler_push_many) beside what it stands next to.

  python tools/exp/resample_stream_time.py [--reps 200] [--warmup 20] [--out FILE]
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/exp/resample_stream_time.py --trace        (a run of its own)

A round: N = 1 / 8 / 64 / 256 sessions, each with a chunk worth 39 spectrogram frames at 16 kHz (6240 samples), arriving as
8 kHz int16 (3120 samples) or as 44.1 kHz stereo int16 (17199 frames), already on the device.  Per source and N, in the same run:

  push_many      the round in one call: host time of the call (it returns without synchronising) and device time between events
  (a) singles    the same round as N single-session pushes
  (b) features   dsmi_features_stream_many of the round's converted chunks (the stage behind it; it synchronises once)
  (c) one-shot   dsmi_resample over the same N chunks as N whole clips (no state, one launch)

Medians with min / max.  --trace runs a fixed number of rounds at N = 8 and N = 256 and nothing else, for the profiler to count the
dispatches per round; --trace-report DB prints those counts from the database rocprofv3 wrote (its `kernels` view), one JSON line
per kernel and grid height (= sessions).  profiles/resample_stream_time.txt is the output of the three runs, one after the other."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SOURCES = {"8k int16": dict(rate=8000, frames=3120, wav=None), "44.1k stereo int16": dict(rate=44100, frames=17199, wav=(2, 2))}


def _spread(xs):
    xs = sorted(xs)
    return dict(median=round(xs[len(xs) // 2], 4), min=round(xs[0], 4), max=round(xs[-1], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
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
    from danspeech_amd import _native
    assert torch.cuda.is_available(), "needs the GPU"
    fe = _native.NativeFrontend()
    stream = torch.cuda.current_stream()
    rng = np.random.default_rng(3)
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)

    def setup(src, n):
        per = 2 if src["wav"] else 1
        pcm = torch.from_numpy(rng.integers(-12000, 12000, size=(n, src["frames"] * per), dtype=np.int16)).cuda()
        kw = dict(wav_format=src["wav"]) if src["wav"] else dict(dtype=np.int16)
        rs = [_native.NativeResampler(fe, src["rate"], "polyphase", **kw) for _ in range(n)]
        return pcm, rs

    if a.trace:
        for n in (8, 256):
            pcm, rs = setup(SOURCES["8k int16"], n)
            for _ in range(50):
                _native.NativeResampler.push_many(rs, [pcm[i] for i in range(n)], [False] * n)
            torch.cuda.synchronize()
            print("traced 50 rounds of N = %d" % n)
        return

    def timed(fn):
        """(host ms per call, device ms between events)"""
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        host, dev = [], []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            t0 = time.perf_counter()
            fn()
            host.append((time.perf_counter() - t0) * 1e3)
            e1.record(stream)
            e1.synchronize()
            dev.append(e0.elapsed_time(e1))
        return _spread(host), _spread(dev)

    for name, src in SOURCES.items():
        for n in (1, 8, 64, 256):
            pcm, rs = setup(src, n)
            chunks = [pcm[i] for i in range(n)]
            flags = [False] * n
            h, d = timed(lambda: _native.NativeResampler.push_many(rs, chunks, flags))
            emit(dict(figure="push_many", source=name, sessions=n, host_call_ms=h, device_events_ms=d))
            h, d = timed(lambda: [r.push(c) for r, c in zip(rs, chunks)])
            emit(dict(figure="(a) single pushes", source=name, sessions=n, host_call_ms=h, device_events_ms=d))
            outs = _native.NativeResampler.push_many(rs, chunks, flags)
            states = [np.zeros(3) for _ in range(n)]
            h, d = timed(lambda: fe.features_stream_many(outs, states))
            emit(dict(figure="(b) features_stream_many", source=name, sessions=n, samples=int(outs[0].numel()), host_call_ms=h, device_events_ms=d))
            flat = pcm.reshape(-1).view(torch.uint8) if src["wav"] else pcm.reshape(-1)
            counts = np.full(n, src["frames"], dtype=np.int64)
            h, d = timed(lambda: fe.resample(flat, counts, src["rate"], "polyphase", wav_format=src["wav"]))
            emit(dict(figure="(c) one-shot dsmi_resample", source=name, sessions=n, host_call_ms=h, device_events_ms=d))
            for r in rs:
                r.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
