"""Reference of CTC phrase search (dsmi_spot, csrc/spot.hip) in numpy: the recurrence and the picking rule of include/dsmi.h
with the same lp = log(max(p, FLT_MIN)), the same order of additions and the same tie rule, in float32 (the kernel's results
up to the last bits of log) or float64, and a brute force over every window and every frame labelling for tiny cases.  A
helper module of the tests (not collected)."""
import itertools

import numpy as np

from _align_ref import collapse, log_probs

FLT_MIN = np.finfo(np.float32).tiny


def peaky(rng, T, C, sharp=4.0, blank_boost=1.5):
    """The test probabilities of tests/test_gpu_align.py (``_peaky``): sharpened random softmax rows that favour the blank."""
    z = rng.normal(size=(T, C)) * sharp
    z[:, 0] += blank_boost * sharp
    z -= z.max(1, keepdims=True)
    p = np.exp(z)
    return (p / p.sum(1, keepdims=True)).astype(np.float32)


def state_labels(phrase, blank=0):
    """S = 2L - 1 states: token, blank, token, ..., token."""
    return np.array([int(phrase[s // 2]) if s % 2 == 0 else blank for s in range(2 * len(phrase) - 1)], dtype=np.int64)


def _shift(x, k, fill):
    return np.concatenate((np.full(k, fill, dtype=x.dtype), x[:len(x) - k]))[:len(x)]


def tracks(probs, phrase, blank=0, dtype=np.float32, margins=False):
    """probs [T, C] (the clip's frames only), phrase: label ids, at least one.  Returns (E [T] in ``dtype``, ST [T] int32): the
    score of the best path that emits exactly the phrase and ends in its last token at frame f, and the frame it began at
    (-inf / -1 where there is none).  With ``margins`` also MG [T]: the smallest gap between the best and the second best
    predecessor at any decision on that path (inf where nothing competed)."""
    probs = np.asarray(probs, dtype=np.float32)
    T, L = probs.shape[0], len(phrase)
    assert L >= 1
    S = 2 * L - 1
    lab = state_labels(phrase, blank)
    skip = np.array([s % 2 == 0 and s >= 2 and lab[s] != lab[s - 2] for s in range(S)])
    lp = log_probs(probs, dtype) if T else np.zeros((0, probs.shape[1]), dtype=dtype)
    ninf = dtype(-np.inf)
    a = np.full(S, ninf, dtype=dtype)
    b = np.full(S, -1, dtype=np.int32)
    g = np.full(S, np.inf)
    E = np.full(T, ninf, dtype=dtype)
    ST = np.full(T, -1, dtype=np.int32)
    MG = np.full(T, np.inf)
    for f in range(T):
        a1, b1, g1 = _shift(a, 1, ninf), _shift(b, 1, -1), _shift(g, 1, np.inf)
        a2, b2, g2 = _shift(a, 2, ninf), _shift(b, 2, -1), _shift(g, 2, np.inf)
        a2[~skip] = ninf
        best, start, gap = a.copy(), b.copy(), g.copy()
        m = a1 > best                      # strict: on equal scores s wins, then s - 1, then s - 2
        best[m], start[m], gap[m] = a1[m], b1[m], g1[m]
        m = a2 > best
        best[m], start[m], gap[m] = a2[m], b2[m], g2[m]
        if margins:
            with np.errstate(invalid="ignore"):
                second = np.sort(np.stack((a, a1, a2)).astype(np.float64), axis=0)[1]
                here = np.where(np.isfinite(second), best.astype(np.float64) - second, np.inf)
            gap = np.minimum(gap, here)
        best[0], start[0], gap[0] = 0, f, np.inf          # state 0 always restarts: nothing competes
        a = (best + lp[f, lab]).astype(dtype)
        b, g = start, gap
        E[f], ST[f], MG[f] = a[S - 1], b[S - 1], g[S - 1]
    return (E, ST, MG) if margins else (E, ST)


def pick(E, ST, max_hits, min_mean_logp=-np.inf):
    """The picking rule: [(start, end, score), ...] with frames [start, end), best first, pairwise disjoint."""
    E = np.asarray(E, dtype=np.float32)
    ST = np.asarray(ST, dtype=np.int64)
    f = np.arange(len(E), dtype=np.int64)
    with np.errstate(invalid="ignore"):
        floor = np.float32(min_mean_logp) * (f - ST + 1).astype(np.float32)         # a float32 multiply, as the kernel's
        alive = (E > -np.inf) & (E >= floor)
    hits = []
    while len(hits) < max_hits and alive.any():
        e = int(np.argmax(np.where(alive, E, -np.inf)))       # the first of equal maxima: the lowest frame
        s = int(ST[e])
        hits.append((s, e + 1, E[e]))
        alive &= ~((ST <= e) & (s <= f))
    return hits


_LABELLINGS = {}


def _labellings(n, C, blank):
    """Every labelling of n frames over C labels that begins and ends in a token: (rows [N, n], {collapse: row indices})."""
    key = (n, C, blank)
    if key not in _LABELLINGS:
        rows = np.array([r for r in itertools.product(range(C), repeat=n) if r[0] != blank and r[-1] != blank], dtype=np.int64)
        groups = {}
        for i, r in enumerate(rows.reshape(-1, n)):
            groups.setdefault(tuple(collapse(r, blank)), []).append(i)
        _LABELLINGS[key] = (rows.reshape(-1, n), {k: np.array(v) for k, v in groups.items()})
    return _LABELLINGS[key]


def brute_force(probs, phrases, blank=0):
    """Tiny cases.  W[k][s, e] = the best float64 score over every labelling of frames s..e that begins and ends in a token and
    collapses to phrases[k] (-inf where there is none).  max over s of W[k][:, f] is the end score of frame f."""
    probs = np.asarray(probs, dtype=np.float32)
    T, C = probs.shape
    lp = np.log(np.maximum(probs, FLT_MIN).astype(np.float64))
    W = [np.full((T, T), -np.inf) for _ in phrases]
    for s in range(T):
        for e in range(s, T):
            rows, groups = _labellings(e - s + 1, C, blank)
            scores = lp[np.arange(s, e + 1)[None, :], rows].sum(1)
            for k, ph in enumerate(phrases):
                idx = groups.get(tuple(int(x) for x in ph))
                if idx is not None:
                    W[k][s, e] = scores[idx].max()
    return W
