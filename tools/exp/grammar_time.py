"""CTC grammar decoding (dsmi_grammar) beside dsmi_align and the forward on the same probabilities.  B = 32 clips of 10 s (501
frames) through a synthetic cfgA model (2 conv, 5 x BiGRU 800, 33 labels).

  python tools/exp/grammar_time.py [--reps 10] [--warmup 2] [--out profiles/grammar_time.txt]
  DSMI_LIBRARY=danspeech_amd/lib/libdsmi_exp.so python tools/exp/grammar_time.py --serial     (also the backtrace that was not adopted)
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/exp/grammar_time.py --trace-n 10    (a run of its own)
  python tools/exp/grammar_time.py --trace-report DIR [--out profiles/grammar_time.txt]       (appends the kernels' times)

In every repetition, one after the other (the same clock, the same neighbours on the host):
- dsmi_align of a random 150-character transcript per clip, and dsmi_grammar of the same clips on the chain graphs of the same
  transcripts (each clip its own graph): the one comparison that means something, reported as a ratio;
- dsmi_grammar on a loop over ten digit words, on a loop over 300 words of synthetic.make_vocabulary, and on a graph at both
  limits (2048 nodes in a ring, four predecessors each: 8192 arcs), one graph for all clips;
- one node with a fan-in of 300 (walked by one thread per frame);
- the synchronous forward of the same batch.
Device events on the call's stream around the whole call (upload, kernel, result copy) and the host clock around it.  Medians with
min / max over --reps.  One JSON line per figure, printed and written.

--serial (the experiments library): every dsmi_grammar figure again with DSMI_DEBUG_GRAMMAR_TRACE=serial, the backtrace by one
lane with one dependent load per frame, and with =none, no backtrace at all (what the forward pass costs alone).
--trace-n N: only N dsmi_grammar calls of each graph and N dsmi_align calls, for the profiler.
--trace-report DIR: per kernel of the trace under DIR, by grid size, the dispatches and their median / min / max ns."""
import argparse
import csv
import glob
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

DIGITS = "$d = nul | en | to | tre | fire | fem | seks | syv | otte | ni ; $d+"


def _spread(xs):
    xs = sorted(xs)
    return dict(median=round(xs[len(xs) // 2], 4), min=round(xs[0], 4), max=round(xs[-1], 4))


def _graph(labels, flags, preds, empty_ok=False):
    g = SimpleNamespace(labels=np.asarray(labels, dtype=np.int32), flags=np.asarray(flags, dtype=np.int32), weights=None, empty_ok=empty_ok)
    g.arc_off = np.zeros(len(g.labels) + 1, dtype=np.int32)
    g.arc_off[1:] = np.cumsum([len(p) for p in preds])
    g.arc_pred = np.array([q for p in preds for q in p], dtype=np.int32)
    return g


def _chain(ids):
    L = len(ids)
    return _graph(ids, [(1 if k == 0 else 0) | (2 if k == L - 1 else 0) for k in range(L)], [[k - 1] if k else [] for k in range(L)], L == 0)


def trace_report(directory, out):
    paths = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    assert paths, "no *kernel_trace.csv under " + directory
    groups = {}
    for path in paths:
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row["Kernel_Name"]
                if "grammar_kernel" not in name and "align_kernel" not in name:
                    continue
                short = name.split("(")[0].split("::")[-1]
                threads, per = row.get("Grid_Size", row.get("Grid_Size_X")), row.get("Workgroup_Size", row.get("Workgroup_Size_X"))
                grid = int(threads) // max(int(per), 1) if threads and per else -1
                groups.setdefault((short, grid), []).append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
    lines = [dict(figure="kernel trace", kernel=k, workgroups=g, dispatches=len(v), ns=_spread(v)) for (k, g), v in sorted(groups.items())]
    with open(out, "a") as f:
        for d in lines:
            print(json.dumps(d), flush=True)
            f.write(json.dumps(d) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--chars", type=int, default=150)
    ap.add_argument("--serial", action="store_true")
    ap.add_argument("--trace-n", type=int, default=0)
    ap.add_argument("--trace-report", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grammar_time.txt"))
    a = ap.parse_args()
    if a.trace_report:
        return trace_report(a.trace_report, a.out)
    import torch
    from danspeech_amd import Recognizer, _native, synthetic as syn
    from danspeech_amd.deepspeech.model import DeepSpeech
    from danspeech_amd.grammar import Grammar
    assert torch.cuda.is_available(), "needs the GPU"
    sd = syn.make_state_dict(2, "gru", 800, 5, seed=0, fc_gain=8.0)
    model = DeepSpeech("cfgA", rnn_type="gru", rnn_hidden_size=800, rnn_layers=5, conv_layers=2).load_state_dict(sd)
    rec = Recognizer(model=model)
    eng = rec.danspeech_recognizer
    clips = [syn.make_clip(i, int(16000 * a.seconds)) for i in range(a.batch)]
    feats, frames = eng.audio_parser.parse_batch(clips)
    lens = torch.from_numpy(frames.astype(np.int32))
    probs, sizes = eng.model.forward(feats, lens)
    torch.cuda.synchronize()
    dec = eng.decoder._dec(eng._device_index())
    sz = sizes.numpy().astype(np.int32)
    stream = torch.cuda.current_stream()
    labels = syn.DANSPEECH_LABELS
    C = len(labels)
    rng = np.random.default_rng(7)
    ids = [rng.integers(1, C, size=a.chars).astype(np.int32) for _ in range(a.batch)]
    chains = [_chain(t) for t in ids]
    every = np.arange(a.batch, dtype=np.int32)
    graphs = {
        "chain graphs of the %d-character transcripts" % a.chars: (chains, every),
        "a loop over ten digit words": (Grammar(DIGITS, labels), None),
        "a loop over 300 words": (Grammar("(" + " | ".join(syn.make_vocabulary(300)) + ")+", labels), None),
        "2048 nodes, 8192 arcs": (_graph(rng.integers(1, C, size=2048), [3] * 2048, [[(n - j) % 2048 for j in range(1, 5)] for n in range(2048)]), None),
        "one node with a fan-in of 300": (_graph(rng.integers(1, C, size=301), [1] * 300 + [2], [[] for _ in range(300)] + [list(range(300))]), None),
    }
    if a.trace_n:
        for _ in range(a.trace_n):
            dec.align(probs, sz, ids)
            for g, cg in graphs.values():
                dec.grammar(probs, sz, g, cg)
        torch.cuda.synchronize()
        return

    def with_trace(form, fn):
        def run():
            os.environ["DSMI_DEBUG_GRAMMAR_TRACE"] = form
            fn()
        return run

    calls = [("dsmi_align, the %d-character transcripts" % a.chars, lambda: dec.align(probs, sz, ids))]
    for name, (g, cg) in graphs.items():
        fn = lambda g=g, cg=cg: dec.grammar(probs, sz, g, cg)
        calls.append(("dsmi_grammar, " + name, with_trace("wave", fn)))
        if a.serial:
            calls.append(("dsmi_grammar, serial backtrace, " + name, with_trace("serial", fn)))
            calls.append(("dsmi_grammar, no backtrace, " + name, with_trace("none", fn)))
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
    lines = [dict(figure=name, device_events_ms=_spread(dev[name]), host_clock_ms=_spread(host[name]), batch=a.batch, frames=int(sz.max()),
                  labels=C, reps=a.reps) for name, _ in calls]
    os.environ["DSMI_DEBUG_GRAMMAR_TRACE"] = "wave"
    for name, (g, cg) in graphs.items():
        one = g if cg is None else g[0]
        lens_, _, _, _, lp, st = dec.grammar(probs, sz, g, cg)
        lines.append(dict(figure="shape, " + name, nodes=int(len(one.labels)), arcs=int(len(one.arc_pred)), decoded=int((st == 0).sum()),
                          visits=[int(lens_.min()), int(lens_.max())], plan=_native.grammar_plan(a.batch, int(probs.shape[1]), len(one.labels), len(one.arc_pred))))
    al = _spread(dev[calls[0][0]])["median"]
    gr = _spread(dev[calls[1][0]])["median"]
    lines.append(dict(figure="dsmi_grammar on chain graphs / dsmi_align, device-event medians", ratio=round(gr / al, 3)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for d in lines:
            print(json.dumps(d), flush=True)
            f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
