"""Every output array of dsmi_align, dsmi_spot and dsmi_score on fixed seeded inputs, written to one .npz -- to compare two builds
of the library byte for byte (a change of the kernels' shared feeder, csrc/ctc_trellis.h, must not move a bit).

  DSMI_LIBRARY=/path/to/one/libdsmi.so python tools/exp/ctc_ab.py --out a.npz
  python tools/exp/ctc_ab.py --out b.npz
  python tools/exp/ctc_ab.py --compare a.npz b.npz

The inputs: every shape of tests/_ctc_edge_cases.py (chunk boundaries, the image wrap, 3 / 33 / 128 labels, a shorter second clip,
127 and 128 tokens on 300 frames) and one batch of B = 32 clips of 501 frames with 150-token transcripts, three candidates and
four phrases per clip.  --compare prints the arrays that differ and exits 1 if any does."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _device(torch, probs):
    T = max(1, max(len(p) for p in probs))
    x = np.full((len(probs), T, probs[0].shape[1]), 1.0 / probs[0].shape[1], dtype=np.float32)
    for b, p in enumerate(probs):
        x[b, :len(p)] = p
    return torch.from_numpy(x).cuda(), np.array([len(p) for p in probs], dtype=np.int32)


def _run(torch, native, out, tag, C, probs, targets, clip, cands, phrases):
    import _ctc_edge_cases as edge
    dec = native.NativeDecoder(edge.labels(C), blank_index=0)
    p_dev, sizes = _device(torch, probs)
    for key, arr in zip(("spans", "token_probs", "path_logp", "status"), dec.align(p_dev, sizes, targets)):
        out["%s.align.%s" % (tag, key)] = arr
    for key, arr in zip(("logp", "status"), dec.score(p_dev, sizes, clip, cands)):
        out["%s.score.%s" % (tag, key)] = arr
    if phrases:
        for key, arr in zip(("hits", "scores", "counts", "E", "ST"), dec.spot(p_dev, sizes, phrases, 5, -np.inf, tracks=True)):
            out["%s.spot.%s" % (tag, key)] = arr
    dec.close()


def dump(path):
    import torch
    from danspeech_amd import _native as native
    import _ctc_edge_cases as edge
    from _spot_ref import peaky
    assert torch.cuda.is_available(), "needs the GPU"
    out = {}
    for shape in edge.SHAPES + edge.LONG:
        T, C, L = shape
        probs, rows = edge.case(T, C, L)
        _run(torch, native, out, edge.name(shape), C, probs, [r[0] for r in rows], [b for b, rs in enumerate(rows) for _ in rs],
             [r for rs in rows for r in rs], edge.phrases(T, C) if L is None else None)
    rng = np.random.default_rng(7)
    B, T, C, L = 32, 501, 33, 150
    probs = [peaky(rng, T - (b % 5) * 37, C, 3.0) for b in range(B)]
    tok = lambda n: [int(x) for x in rng.integers(1, C, size=n)]
    targets = [tok(L) for _ in range(B)]
    cands = [targets[b] if k == 0 else tok(L - 10 * k) for b in range(B) for k in range(3)]
    _run(torch, native, out, "B32-T501-L150", C, probs, targets, [b for b in range(B) for _ in range(3)], cands, [tok(n) for n in (1, 4, 12, 128)])
    np.savez(path, **out)
    print("%s: %d arrays, %d bytes, library %s" % (path, len(out), sum(a.nbytes for a in out.values()), native.LIB_PATH))


def compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    bad = sorted(set(a.files) ^ set(b.files))
    for k in sorted(set(a.files) & set(b.files)):
        if a[k].dtype != b[k].dtype or a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes():
            bad.append(k)
    print("%d arrays, %d bytes compared: %s" % (len(a.files), sum(a[k].nbytes for k in a.files), "DIFFERENT " + " ".join(bad) if bad else "equal byte for byte"))
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    a = ap.parse_args()
    if a.compare:
        raise SystemExit(compare(*a.compare))
    dump(a.out or "ctc_ab.npz")
