"""The resumable beam search (dsmi_beam_stream_advance_many) on the streaming shape: 33 labels, beam 64, a synthetic 3-gram
ARPA (synthetic.make_arpa), 39-frame chunks of seeded peaky probabilities.

  python tools/exp/beam_stream_time.py [--ns 1,64,256] [--reps 20] [--out DIR]

1. One round: N sessions, each 8 chunks (312 frames) into its utterance, advance by one 39-frame chunk in ONE launch --
   ms per round with n_best = 0 (advance only) and with n_best = 1 (plus every session's best hypothesis so far).
2. The is_last text of one utterance of 10 s and 30 s (500 and 1500 output frames at 20 ms): today's full search over the
   whole utterance (dsmi_beam, beam 64) against the carried search's last 39-frame chunk with n_best = 1.
Host clock around calls that end in a device synchronisation (both entry points synchronise); medians over --reps.
Prints one JSON line per figure."""
import argparse
import json
import os
import sys
import tempfile
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from danspeech_amd import _native, synthetic as syn
    assert torch.cuda.is_available(), "needs the GPU"
    labels = syn.DANSPEECH_LABELS
    arpa = os.path.join(tempfile.mkdtemp(), "s3.arpa")
    syn.make_arpa(arpa, order=3, n_words=5000, seed=11, ngrams_per_order=20000)
    dec = _native.NativeDecoder(labels, blank_index=0)
    dec.set_lm(arpa, 1.3, 0.2)
    BS, CH, WARM = 64, 39, 8
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)

    # ---- 1. rounds of N sessions
    for n in [int(v) for v in a.ns.split(",")]:
        p = [torch.from_numpy(_probs(CH * (WARM + 2 * a.reps + 2), 100 + i % 16)).cuda() for i in range(n)]
        sts = [_native.NativeBeamStream(dec, BS, 40, 1.0) for _ in range(n)]
        pos = 0
        for _ in range(WARM):
            _native.NativeBeamStream.advance_many(sts, [q[pos:pos + CH] for q in p], 0)
            pos += CH
        res = {}
        for n_best in (0, 1):
            ts = []
            for _ in range(a.reps):
                chunks = [q[pos:pos + CH] for q in p]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _native.NativeBeamStream.advance_many(sts, chunks, n_best)
                ts.append((time.perf_counter() - t0) * 1e3)
                pos += CH
            res[n_best] = float(np.median(ts))
        emit(dict(figure="round", sessions=n, frames_per_chunk=CH, beam=BS, lm="3-gram ARPA",
                  ms_advance=round(res[0], 4), ms_advance_and_best=round(res[1], 4),
                  us_per_frame_per_session=round(res[0] * 1e3 / CH / n, 3)))
        for s in sts:
            s.close()

    # ---- 2. is_last latency: full search against the carried search's last chunk
    for secs in (10, 30):
        T = secs * 50
        p = torch.from_numpy(_probs(T, 7 + secs)).cuda()
        full = []
        for _ in range(max(3, a.reps // 4) + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dec.beam(p.unsqueeze(0), None, beam_width=BS)
            full.append((time.perf_counter() - t0) * 1e3)
        last = []
        for _ in range(max(3, a.reps // 4) + 1):
            st = _native.NativeBeamStream(dec, BS, 40, 1.0)
            st.advance(p[:T - CH], 0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = st.advance(p[T - CH:], 1)
            last.append((time.perf_counter() - t0) * 1e3)
            st.close()
        want = dec.beam(p.unsqueeze(0), None, beam_width=BS)
        same = bool(np.array_equal(r[0][0, :r[2][0]], want[0][0, 0, :want[2][0, 0]]))
        emit(dict(figure="is_last", seconds=secs, frames=T, beam=BS, lm="3-gram ARPA", ms_full_search=round(float(np.median(full[1:])), 3),
                  ms_last_chunk=round(float(np.median(last[1:])), 3), best_text_equal=same))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "beam_stream_time.jsonl"), "w") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
