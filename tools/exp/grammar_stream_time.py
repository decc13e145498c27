"""Streaming grammar decoding (dsmi_grammar_stream_advance_many) beside what a live caller does without it and beside the model
round it follows.  Synthetic probabilities on the device (33 labels).

  python tools/exp/grammar_stream_time.py [--ns 1,64,256] [--reps 10] [--out profiles/grammar_stream_time.txt]

Per graph (a loop over ten digit words, over 120 words, over 300 words, 2048 nodes in a ring with four predecessors each), per N
sessions and per utterance position P (the frames consumed after the round: 39, 501, 1500), one round = every session advances by
39 frames in ONE call:
  mode0_ms / mode1_ms / mode2_ms   the round with no result, with the partial result, with the final result;
  regrammar_ms   what a live caller does today: dsmi_grammar over the N utterances so far as one batch [N, P, 33] (one workgroup
                 per clip, the graph packed and uploaded again);
and per N:
  forward_ms     the round it follows: dsmi_stream_forward_many of the N sessions' 39-frame chunks (CPUStreamingRNN shape: 2 conv,
                 5 x GRU 800 unidirectional, context 20, synthetic weights);
and for the 300-word loop (one node with 300 predecessors), N = 1:
  per_frame_us   a 501-frame utterance in one call through the stream (mode 0) and through dsmi_grammar, divided by the frames:
                 the heavy-node pass against one thread walking the list.
A stream is reset and advanced to P - 39 in one call outside the clock before each timed round.  Host clock around calls that end
in a device synchronisation; medians over --reps.  One JSON line per figure, printed and written."""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

DIGITS = "$d = nul | en | to | tre | fire | fem | seks | syv | otte | ni ; $d+"


def _probs(T, seed, C=33):
    rng = np.random.default_rng(seed)
    logits = rng.standard_normal((T, C)) * 3.0
    logits[:, 0] += 1.5
    e = np.exp(logits - logits.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", default="1,64,256")
    ap.add_argument("--positions", default="39,501,1500")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grammar_stream_time.txt"))
    a = ap.parse_args()
    import torch
    from danspeech_amd import _native, synthetic as syn
    from danspeech_amd.grammar import Grammar
    assert torch.cuda.is_available(), "needs the GPU"
    labels = syn.DANSPEECH_LABELS
    C = len(labels)
    dec = _native.NativeDecoder(labels, blank_index=0)
    CH, TOP = 39, 1500
    rng = np.random.default_rng(3)
    ring = SimpleNamespace(labels=rng.integers(1, C, size=2048).astype(np.int32), flags=np.full(2048, 3, dtype=np.int32), weights=None, empty_ok=False,
                           arc_off=np.arange(0, 4 * 2048 + 1, 4, dtype=np.int32),
                           arc_pred=np.array([(n - j) % 2048 for n in range(2048) for j in range(1, 5)], dtype=np.int32))
    graphs = [("ten digit words", Grammar(DIGITS, labels)),
              ("120 words", Grammar("(" + " | ".join(syn.make_vocabulary(120)) + ")+", labels)),
              ("300 words", Grammar("(" + " | ".join(syn.make_vocabulary(300)) + ")+", labels)),
              ("2048 nodes, 8192 arcs", ring)]
    lines = []

    def say(**row):
        lines.append(row)
        print(json.dumps(row), flush=True)

    def timed(fn, reps, before=None):
        ts = []
        for _ in range(reps):
            if before:
                before()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return round(float(np.median(ts)), 4)

    ns = [int(v) for v in a.ns.split(",")]
    positions = [int(v) for v in a.positions.split(",")]
    base = [torch.from_numpy(_probs(TOP, 100 + i, C)).cuda() for i in range(16)]
    for name, g in graphs:
        net = _native.NativeGrammarNet(dec, g)
        fan = int(np.max(np.diff(g.arc_off))) if len(g.labels) else 0
        say(figure="shape", graph=name, nodes=int(len(g.labels)), arcs=int(len(g.arc_pred)), largest_fan_in=fan,
            plan=_native.grammar_stream_plan(len(g.labels), len(g.arc_pred), C, TOP))
        for n in ns:
            p = [base[i % 16] for i in range(n)]
            sts = [_native.NativeGrammarStream(net, 0, TOP) for _ in range(n)]
            for P in positions:
                def rewind():
                    for s in sts:
                        s.reset()
                    if P > CH:
                        _native.NativeGrammarStream.advance_many(sts, [q[:P - CH] for q in p], [0] * n)
                rows = [q[P - CH:P] for q in p]
                row = dict(figure="round", graph=name, sessions=n, position=P, frames_per_chunk=CH)
                for mode in (0, 1, 2):
                    fn = lambda mode=mode: _native.NativeGrammarStream.advance_many(sts, rows, [mode] * n)
                    rewind(); fn()
                    row["mode%d_ms" % mode] = timed(fn, a.reps, rewind)
                sofar = torch.stack([q[:P] for q in p]).contiguous()
                dec.grammar(sofar, None, g)
                row["regrammar_ms"] = timed(lambda: dec.grammar(sofar, None, g), max(2, a.reps // 2))
                say(**row)
            for s in sts:
                s.close()
        if name == "300 words":
            s = _native.NativeGrammarStream(net, 0, TOP)
            x = base[0][:501]
            one = lambda: s.advance(x, 0)
            s.reset(); one()
            stream_ms = timed(one, a.reps, s.reset)
            shot = x[None].contiguous()
            dec.grammar(shot, None, g)
            shot_ms = timed(lambda: dec.grammar(shot, None, g), a.reps)
            say(figure="per frame, 300 words, one session, 501 frames in one call", stream_ms=stream_ms, grammar_ms=shot_ms,
                stream_per_frame_us=round(stream_ms * 1e3 / 501, 3), grammar_per_frame_us=round(shot_ms * 1e3 / 501, 3))
            s.close()
        net.close()
    cfg = dict(conv_layers=2, rnn_type="gru", rnn_hidden_size=800, rnn_layers=5, bidirectional=False, context=20)
    model = _native.NativeModel(cfg, syn.make_state_dict(2, "gru", 800, 5, bidirectional=False, context=20, seed=5, fc_gain=4.0))
    x0 = torch.from_numpy(syn.make_features(1, 54, seed=1)).cuda()
    x = torch.from_numpy(syn.make_features(1, 39, seed=2)).cuda()
    for n in ns:
        fw = [_native.NativeStream(model) for _ in range(n)]
        _native.NativeStream.forward_many(fw, [x0] * n, [True] * n, [False] * n)
        _native.NativeStream.forward_many(fw, [x] * n, [False] * n, [False] * n)
        say(figure="forward", sessions=n, frames_per_chunk=CH,
            forward_ms=timed(lambda: _native.NativeStream.forward_many(fw, [x] * n, [False] * n, [False] * n), a.reps))
        for s in fw:
            s.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for d in lines:
            f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
