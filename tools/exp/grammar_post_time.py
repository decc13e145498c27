"""The CTC grammar posterior (dsmi_grammar_posterior) beside dsmi_occupancy, dsmi_grammar and the forward on the same
probabilities.  B = 32 clips of 10 s (501 frames) through a synthetic cfgA model (2 conv, 5 x BiGRU 800, 33 labels).

  python tools/exp/grammar_post_time.py [--reps 10] [--warmup 2] [--out profiles/grammar_post_time.txt]

In every repetition, one after the other (the same clock, the same neighbours on the host):
- dsmi_occupancy (occ alone) of a random 150-character transcript per clip, and dsmi_grammar_posterior of the same clips on the
  chain graphs of the same transcripts (each clip its own graph), in full and for logp alone (the forward pass only);
- dsmi_grammar and dsmi_grammar_posterior on a loop over ten digit words and on a loop over 300 words of
  synthetic.make_vocabulary, one graph for all clips; the posterior in full, without visits, and for logp alone;
- the synchronous forward of the same batch.
Device events on the call's stream around the whole call (upload, kernels, result copy) and the host clock around it.  Medians
with min / max over --reps.  One JSON line per figure, printed and written."""
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


def _spread(xs):
    xs = sorted(xs)
    return dict(median=round(xs[len(xs) // 2], 4), min=round(xs[0], 4), max=round(xs[-1], 4))


def _chain(ids):
    L = len(ids)
    g = SimpleNamespace(labels=np.asarray(ids, dtype=np.int32), weights=None, empty_ok=L == 0,
                        flags=np.array([(1 if k == 0 else 0) | (2 if k == L - 1 else 0) for k in range(L)], dtype=np.int32))
    g.arc_off = np.arange(L + 1, dtype=np.int32) - 1
    g.arc_off[0] = 0
    g.arc_pred = np.arange(L - 1, dtype=np.int32)
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--chars", type=int, default=150)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grammar_post_time.txt"))
    a = ap.parse_args()
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
    }
    calls = [("dsmi_occupancy (occ), the %d-character transcripts" % a.chars, lambda: dec.occupancy(probs, sz, every, ids, want_tok=False))]
    for name, (g, cg) in graphs.items():
        if cg is None:
            calls.append(("dsmi_grammar, " + name, lambda g=g, cg=cg: dec.grammar(probs, sz, g, cg)))
        calls.append(("dsmi_grammar_posterior, " + name, lambda g=g, cg=cg: dec.grammar_posterior(probs, sz, g, cg)))
        calls.append(("dsmi_grammar_posterior, occ alone, " + name, lambda g=g, cg=cg: dec.grammar_posterior(probs, sz, g, cg, want_visits=False)))
        calls.append(("dsmi_grammar_posterior, logp alone, " + name, lambda g=g, cg=cg: dec.grammar_posterior(probs, sz, g, cg, want_visits=False, want_occ=False)))
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
    for name, (g, cg) in graphs.items():
        one = g if cg is None else g[0]
        off = np.asarray(one.arc_off)
        lp, _, _, st = dec.grammar_posterior(probs, sz, g, cg, want_visits=False, want_occ=False)
        lines.append(dict(figure="shape, " + name, nodes=int(len(one.labels)), arcs=int(len(one.arc_pred)), fan_in=int((off[1:] - off[:-1]).max()),
                          decoded=int((st == 0).sum()), logp=[float(lp[st == 0].min()), float(lp[st == 0].max())] if (st == 0).any() else None,
                          plan=_native.grammar_posterior_plan(a.batch, int(probs.shape[1]), len(one.labels), len(one.arc_pred))))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for d in lines:
            print(json.dumps(d), flush=True)
            f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
