"""CTC occupancy (dsmi_occupancy) beside its neighbours on the same probabilities -- dsmi_score, dsmi_alternatives, the forward
that made them -- and beside torch's own CTC loss, forward and backward in float64 on the same device and inputs, which is the
other way to the per-frame label posteriors (occ = P - the gradient torch returns).  B = 32 clips of 10 s (501 frames) through a
synthetic cfgA model (2 conv, 5 x BiGRU 800, 33 labels), each with the transcript the model recognises in it -- the synthetic
model's random weights recognise only a token or two per clip -- and, the shape a subtitle line has, each with a random
transcript of 150 characters.

  python tools/exp/occ_time.py [--reps 10] [--warmup 2] [--out profiles/occ_time.txt]
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/exp/occ_time.py --trace-n 10      (a run of its own)
  python tools/exp/occ_time.py --trace-report DIR [--out profiles/occ_time.txt]               (appends the kernels' times)

In every repetition, one after the other (so that all figures see the same clock and the same neighbours on the host), for each
of the two sets of transcripts: dsmi_occupancy of the 32 transcripts in one call (occ and tok; occ alone; logp alone), of ONE
transcript alone (the two chains of 501 frames with nothing beside them), dsmi_score and dsmi_alternatives of the same
candidates, torch.nn.functional.ctc_loss forward + backward in float64; and the synchronous forward of the same batch.  Device
events on the call's stream around the whole call (upload, kernels, result copy) and the host clock around it (every call ends in
a synchronise).  Medians with min / max over --reps.  Then, once per set, the largest distance between dsmi_occupancy's occ and
P - torch's gradient.  One JSON line per figure, printed and written.

--trace-n N: only N dsmi_occupancy calls of the 150-character batch and N of one transcript alone, for the profiler.
--trace-report DIR: per kernel of the trace under DIR, by grid size, the dispatches and their median / min / max ns."""
import argparse
import csv
import glob
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


def trace_report(directory, out):
    """The kernel trace's rows of the occupancy kernels, grouped by kernel and grid size."""
    paths = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    assert paths, "no *kernel_trace.csv under " + directory
    groups = {}
    for path in paths:
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row["Kernel_Name"]
                if "occ_" not in name:
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
    ap.add_argument("--trace-n", type=int, default=0)
    ap.add_argument("--trace-report", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "occ_time.txt"))
    a = ap.parse_args()
    if a.trace_report:
        return trace_report(a.trace_report, a.out)
    import torch
    from danspeech_amd import Recognizer, synthetic as syn
    from danspeech_amd.deepspeech.model import DeepSpeech
    import _occ_ref as occ_ref
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
    C = probs.shape[2]
    rng = np.random.default_rng(7)
    every = np.arange(a.batch)
    sets = [("recognised transcripts", [np.asarray(t, dtype=np.int32) for t, _ in dec.greedy(probs, sz)]),
            ("%d-character transcripts" % a.chars,
             [eng.decoder.transcript_ids(eng.decoder.normalise_transcript(_transcript(rng, a.chars))) for _ in range(a.batch)])]
    if a.trace_n:
        ids = sets[1][1]
        for _ in range(a.trace_n):
            dec.occupancy(probs, sz, every, ids)
            dec.occupancy(probs, sz, [0], [ids[0]])
        torch.cuda.synchronize()
        return
    # torch's loss takes [T, B, C] log probabilities; the same float32 probabilities, widened, floored as the library floors them
    lp_t = torch.log(probs.double().clamp_min(float(np.finfo(np.float32).tiny))).transpose(0, 1).contiguous()
    in_lens = torch.from_numpy(sz.astype(np.int64))
    calls, shapes, torch_grad = [], {}, {}
    for label, ids in sets:
        flat = torch.from_numpy(np.concatenate([np.asarray(t, dtype=np.int64) for t in ids] + [np.zeros(0, dtype=np.int64)])).cuda()
        tg_lens = torch.tensor([len(t) for t in ids], dtype=torch.int64)

        def torch_loss(label=label, flat=flat, tg_lens=tg_lens):
            x = lp_t.detach().requires_grad_(True)
            loss = torch.nn.functional.ctc_loss(x, flat, in_lens, tg_lens, blank=eng.decoder.blank_index, reduction="sum")
            loss.backward()
            torch.cuda.synchronize()
            torch_grad[label] = x.grad

        shapes[label] = dict(tokens=[int(min(len(t) for t in ids)), int(max(len(t) for t in ids))])
        calls.append(("dsmi_occupancy occ + tok, the batch, " + label, lambda ids=ids: dec.occupancy(probs, sz, every, ids), label))
        calls.append(("dsmi_occupancy occ alone, the batch, " + label, lambda ids=ids: dec.occupancy(probs, sz, every, ids, want_tok=False), label))
        calls.append(("dsmi_occupancy logp alone, the batch, " + label,
                      lambda ids=ids: dec.occupancy(probs, sz, every, ids, want_occ=False, want_tok=False), label))
        calls.append(("dsmi_occupancy occ + tok, one transcript alone, " + label, lambda ids=ids: dec.occupancy(probs, sz, [0], [ids[0]]), label))
        calls.append(("dsmi_score, the batch, " + label, lambda ids=ids: dec.score(probs, sz, every, ids), label))
        calls.append(("dsmi_alternatives, the batch, " + label, lambda ids=ids: dec.alternatives(probs, sz, every, ids), label))
        calls.append(("torch ctc_loss float64 forward + backward, the batch, " + label, torch_loss, label))
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
        ours = _spread(host["dsmi_occupancy occ alone, the batch, " + label])["median"]
        theirs = _spread(host["torch ctc_loss float64 forward + backward, the batch, " + label])["median"]
        lines.append(dict(figure="torch ctc_loss / dsmi_occupancy occ alone, host clock medians, " + label, ratio=round(theirs / ours, 2)))
        one = _spread(host["dsmi_occupancy occ + tok, one transcript alone, " + label])["median"]
        lines.append(dict(figure="per frame, one transcript alone, " + label, us_per_frame=round(one * 1e3 / int(sz[0]), 3),
                          note="whole call over frames: an upper bound of the two chains, one behind the other"))
        # ---- the two ways agree: occ against P - torch's gradient, as a share of the bound
        lp, occ, _, status = dec.occupancy(probs, sz, every, ids, want_tok=False)
        want = (probs.double() - torch_grad[label].transpose(0, 1)).cpu().numpy()
        got = occ.cpu().numpy()
        worst = max(float(np.abs(got[b, :sz[b]] - want[b, :sz[b]]).max()) / occ_ref.bound(int(sz[b]), lp[b]) for b in range(a.batch))
        lines.append(dict(figure="agreement with P - torch's gradient, " + label, feasible=int((status == 0).sum()),
                          worst_share_of_the_bound=round(worst, 5)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for d in lines:
            print(json.dumps(d), flush=True)
            f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
