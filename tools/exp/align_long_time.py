"""Long-form CTC alignment (dsmi_align_long) of one synthetic hour: T = 180 000 frames (20 ms each) of 33 labels and a transcript
of about 50 000 characters planted in them, beside the forward of the same amount of audio through a synthetic cfgA model (2 conv,
5 x BiGRU 800: 360 clips of 10 s in batches of 30) and beside dsmi_align over the same frames cut into pieces of 4096 characters
at the planted boundaries, which is what a caller who knew them could do today.

  python tools/exp/align_long_time.py [--reps 3] [--out profiles/align_long_time.txt]
  DSMI_LIBRARY=danspeech_amd/lib/libdsmi_exp.so python tools/exp/align_long_time.py --forms [--out ...]      (appends)
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/exp/align_long_time.py --trace-n 2      (a run of its own)
  python tools/exp/align_long_time.py --trace-report DIR --trace-n 2 [--out ...]                            (appends)

The hour: each character takes one or two frames with 6 added to its label's logit, a blank frame lies between equal neighbours,
the other frames are blank; unit normal noise on every logit, then the softmax.  Every call is timed by the host clock around it
(it ends in a synchronise) and by device events on its stream; medians with min / max over --reps, one JSON line per figure.
--forms, with the experiments build: the same call under DSMI_DEBUG_ALONG_FORM = w1792f128, w896f64 and w128f64 (W states per
forward workgroup, F frames per launch), the geometries that were measured and not adopted, each checked to return the adopted
geometry's result.
--trace-report: per kernel of the trace the dispatches and the sum of their times per call: the split between the forward
launches and the backtrace."""
import argparse
import csv
import glob
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def _spread(xs):
    xs = sorted(xs)
    return dict(median=round(xs[len(xs) // 2], 3), min=round(xs[0], 3), max=round(xs[-1], 3))


def planted_hour(T, n_chars, C, space, seed=1):
    """(probs float32 [T, C], ids int32 [L], starts int64 [L]): a transcript and the frames it was planted in."""
    rng = np.random.default_rng(seed)
    letters = [c for c in range(1, C) if c != space]
    ids = []
    while len(ids) < n_chars:
        ids += [int(x) for x in rng.choice(letters, size=int(rng.integers(2, 9)))] + [space]
    ids = np.array(ids[:n_chars - 1] + [letters[0]], dtype=np.int32)
    L = len(ids)
    dur = rng.integers(1, 3, size=L)
    gap = np.concatenate(([0], (ids[1:] == ids[:-1]).astype(np.int64)))      # blank frames in front of each token
    spare = T - int(dur.sum() + gap.sum())
    assert spare >= 0, "the transcript does not fit the frames"
    gap = gap + rng.multinomial(spare, np.ones(L + 1) / (L + 1))[:L]           # (the last share: blanks behind the last token)
    starts = np.cumsum(gap + np.concatenate(([0], dur[:-1])))
    lab = np.zeros(T, dtype=np.int64)
    for d in (0, 1):
        m = dur > d
        lab[starts[m] + d] = ids[m]
    z = rng.standard_normal((T, C)).astype(np.float32)
    z[np.arange(T), lab] += 6.0
    z -= z.max(1, keepdims=True)
    p = np.exp(z)
    return (p / p.sum(1, keepdims=True)).astype(np.float32), ids, starts


def trace_report(directory, calls, out):
    paths = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    assert paths, "no *kernel_trace.csv under " + directory
    groups = {}
    for path in paths:
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row["Kernel_Name"]
                found = re.search(r"along_[a-z]+", name)
                if not found:
                    continue
                short = found.group(0)
                groups.setdefault(short, []).append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
    lines = [dict(figure="kernel trace", kernel=k, dispatches_per_call=len(v) // calls, ms_per_call=round(sum(v) / calls / 1e6, 3),
                  us_per_dispatch=_spread([x / 1e3 for x in v])) for k, v in sorted(groups.items())]
    with open(out, "a") as f:
        for d in lines:
            print(json.dumps(d), flush=True)
            f.write(json.dumps(d) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=180000)
    ap.add_argument("--chars", type=int, default=50000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--forms", action="store_true")
    ap.add_argument("--trace-n", type=int, default=0)
    ap.add_argument("--trace-report", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_long_time.txt"))
    a = ap.parse_args()
    if a.trace_report:
        return trace_report(a.trace_report, max(a.trace_n, 1), a.out)
    import torch
    from danspeech_amd import _native, synthetic as syn
    assert torch.cuda.is_available(), "needs the GPU"
    labels = syn.DANSPEECH_LABELS
    C, T = len(labels), a.frames
    probs_h, ids, starts = planted_hour(T, a.chars, C, labels.index(" "))
    L = len(ids)
    probs = torch.from_numpy(probs_h).cuda()
    dec = _native.NativeDecoder(labels, blank_index=0)
    stream = torch.cuda.current_stream()
    plan = _native.align_long_plan(T, L)

    def timed(fn, reps):
        dev, host, last = [], [], None
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            h0 = time.perf_counter()
            last = fn()
            e1.record(stream)
            e1.synchronize()
            host.append((time.perf_counter() - h0) * 1e3)
            dev.append(e0.elapsed_time(e1))
        return _spread(dev), _spread(host), last

    whole = lambda: dec.align_long(probs, ids, True, True)
    whole()                                  # (the workspace grows here)
    if a.trace_n:
        for _ in range(a.trace_n):
            whole()
        torch.cuda.synchronize()
        return
    lines = []
    if a.forms:
        want = whole()
        for form in ("w1792f128", "w896f64", "w128f64"):
            os.environ["DSMI_DEBUG_ALONG_FORM"] = form
            whole()
            dev, host, got = timed(whole, a.reps)
            same = bool(np.array_equal(got[0], want[0]) and got[1].tobytes() == want[1].tobytes() and got[2] == want[2])
            lines.append(dict(figure="dsmi_align_long, the hour, form " + form,
                              device_events_ms=dev, host_clock_ms=host, same_result_as_adopted=same, reps=a.reps))
        del os.environ["DSMI_DEBUG_ALONG_FORM"]
        dev, host, _ = timed(whole, a.reps)
        lines.append(dict(figure="dsmi_align_long, the hour, adopted form, same process", device_events_ms=dev, host_clock_ms=host, plan=plan, reps=a.reps))
    else:
        dev, host, got = timed(whole, a.reps)
        hour_ms = host["median"]
        found = float(np.mean(got[0][:, 0] == starts))
        lines.append(dict(figure="dsmi_align_long, the hour, both ends free", device_events_ms=dev, host_clock_ms=host, frames=T, tokens=L, labels=C,
                          plan=plan, status=got[3], path_logp=round(got[2], 2), share_of_tokens_at_their_planted_start=round(found, 4), reps=a.reps))
        dev, host, got = timed(lambda: dec.align_long(probs, ids, False, False), a.reps)
        lines.append(dict(figure="dsmi_align_long, the hour, both ends costly", device_events_ms=dev, host_clock_ms=host, reps=a.reps))
        # ---- dsmi_align over the same frames cut into pieces of 4096 characters at the planted boundaries
        piece = _native.ALIGN_MAX_TOKENS
        cuts = list(range(0, L, piece)) + [L]
        edges = [0] + [int(starts[k]) for k in cuts[1:-1]] + [T]
        sizes = np.diff(edges).astype(np.int32)
        batch = torch.full((len(sizes), int(sizes.max()), C), 1.0 / C, device="cuda")
        for b in range(len(sizes)):
            batch[b, :sizes[b]] = probs[edges[b]:edges[b + 1]]
        rows = [list(ids[cuts[b]:cuts[b + 1]]) for b in range(len(sizes))]
        pieces = lambda: dec.align(batch, sizes, rows)
        pieces()
        dev, host, got = timed(pieces, a.reps)
        lines.append(dict(figure="dsmi_align, the same frames in %d pieces of at most %d characters, one call" % (len(sizes), piece),
                          device_events_ms=dev, host_clock_ms=host, frames_per_piece=[int(sizes.min()), int(sizes.max())],
                          infeasible=int(got[3].sum()), backpointer_bytes=int(len(sizes)) * int(sizes.max()) * (2 * piece + 4), reps=a.reps))
        del batch
        # ---- the forward of the same amount of audio: 360 clips of 10 s, 30 at a time
        from danspeech_amd import Recognizer
        from danspeech_amd.deepspeech.model import DeepSpeech
        sd = syn.make_state_dict(2, "gru", 800, 5, seed=0, fc_gain=8.0)
        rec = Recognizer(model=DeepSpeech("cfgA", rnn_type="gru", rnn_hidden_size=800, rnn_layers=5, conv_layers=2).load_state_dict(sd))
        eng = rec.danspeech_recognizer
        seconds = T * 0.02
        n_batches = int(np.ceil(seconds / 300.0))
        feats, frames = eng.audio_parser.parse_batch([syn.make_clip(i, 160000) for i in range(30)])
        lens = torch.from_numpy(frames.astype(np.int32))

        def forward():
            for _ in range(n_batches):
                eng.model.forward(feats, lens)
            torch.cuda.synchronize()

        forward()
        dev, host, _ = timed(forward, a.reps)
        lines.append(dict(figure="forward of %d s of audio: %d batches of 30 clips of 10 s (features not included)" % (int(n_batches * 300), n_batches),
                          device_events_ms=dev, host_clock_ms=host, reps=a.reps))
        lines.append(dict(figure="dsmi_align_long per hour of audio", seconds=round(hour_ms / 1e3 * 3600.0 / seconds, 4),
                          share_of_the_forward=round(hour_ms / host["median"], 3)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.forms else "w") as f:
        for d in lines:
            print(json.dumps(d), flush=True)
            f.write(json.dumps(d) + "\n")
    dec.close()


if __name__ == "__main__":
    main()
