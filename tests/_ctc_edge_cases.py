"""The shapes at which the probability feeder that dsmi_align, dsmi_spot and dsmi_score share (csrc/ctc_trellis.h) can go wrong,
for one parametrised test in each of tests/test_gpu_align.py, test_gpu_spot.py and test_gpu_score.py.

The feeder moves 16 frames of C probabilities at a time through two LDS images, 2048 values per image and 8 per thread:
- frames T in 1, 15, 16, 17, 31, 32, 33, 48: one frame, either side of the first and the second chunk boundary, and a third chunk,
  which is the first to go into image 0 again;
- labels C in 3, 33, 128: 16 C far below the image (most threads move nothing), no multiple of the 256 threads, and all of it;
- two clips, the second shorter than T_out by a quarter and one frame (no frames at all where T = 1), so the last chunk of each
  ends at another frame and the frames past a clip must not be read for a value;
- for align and score, 127 and 128 tokens on 300 frames (33 labels): 255 and 257 states, either side of the 256 threads'
  stride -- in the first clip only; the second has 224 frames and so at most 112 tokens, 225 states.

Nothing is infeasible: a token row of a clip with n frames has at most n // 2 tokens (one more frame than the worst case, all
tokens equal, needs less one), and a phrase (at least one token) fits the first clip.  tests/test_ctc_edge_cases_host.py holds
the table to that on the CPU, with the numpy references each GPU test compares with."""
import numpy as np

import _align_ref as aref
from _spot_ref import peaky

FRAMES = (1, 15, 16, 17, 31, 32, 33, 48)
LABELS = (3, 33, 128)
SHAPES = [(T, C, None) for C in LABELS for T in FRAMES]
LONG = [(300, 33, 127), (300, 33, 128)]


def name(shape):
    T, C, L = shape
    return "T%d-C%d" % (T, C) + ("-L%d" % L if L else "")


def labels(C):
    return ["_"] + ["<%d>" % i for i in range(1, C)]


def _tokens(rng, L, C):
    return [int(x) for x in rng.integers(1, C, size=L)]


def case(T, C, L=None):
    """(probs, rows): two clips [T, C] and [T - 1 - T // 4, C] of float32 probabilities, and per clip its token rows, longest
    first: n // 2, at most one and no token for a clip of n frames (with L: one row of min(L, n // 2) tokens)."""
    rng = np.random.default_rng(1000 * C + T + (L or 0))
    probs = [peaky(rng, n, C) for n in (T, T - 1 - T // 4)]
    rows = []
    for p in probs:
        n = len(p)
        rows.append([_tokens(rng, k, C) for k in ([n // 2, min(1, n // 2), 0] if L is None else [min(L, n // 2)])])
        assert all(len(r) <= n // 2 and aref.min_frames(r) <= n for r in rows[-1])
    return probs, rows


def phrases(T, C):
    """Three phrases that fit T frames: max(1, T // 2), max(1, T // 4) and one token."""
    rng = np.random.default_rng(2000 * C + T)
    out = [_tokens(rng, max(1, k), C) for k in (T // 2, T // 4, 1)]
    assert all(aref.min_frames(ph) <= T for ph in out)
    return out
