"""Reference of CTC occupancy (dsmi_occupancy, csrc/occ.hip) in numpy: the forward-backward pass of include/dsmi.h with the data
type as a parameter (float64 is the contract's; np.longdouble measures float64's own rounding), its bound, and a brute force
over every frame labelling that gives occ and tok by their definition: the share of the transcript's probability that passes
through label c, or through token k, at frame t.  A helper module of the tests (not collected)."""
import itertools

import numpy as np

import _align_ref as aref
from _alt_ref import _trellises

FLT_MIN = aref.FLT_MIN


def bound(T, logp):
    """The contract's bound on |occ or tok element - the recurrences evaluated exactly|: 32 T 2^-52 max(1, |logp| + 88)."""
    return 32.0 * max(T, 1) * 2.0 ** -52 * max(1.0, abs(float(logp)) + 88.0)


def occupancy(probs, targets, blank=0, dtype=np.float64):
    """probs [T, C] (the clip's frames only), targets: label ids.  None when infeasible, else (logp, occ [T, C], tok [T, L])
    in ``dtype``; the per-label sum runs over the states in ascending order, as the library's does."""
    probs = np.asarray(probs, dtype=np.float32)
    T, C = probs.shape
    y = np.array([int(x) for x in targets], dtype=np.int64)
    L = len(y)
    if aref.min_frames(y) > T:
        return None
    if T == 0:
        return dtype(0), np.zeros((0, C), dtype=dtype), np.zeros((0, L), dtype=dtype)
    lp = aref.log_probs(probs, dtype)
    lab = np.asarray(aref.state_labels(y, blank))
    alpha, beta = _trellises(lp, lab, dtype)
    logp = np.logaddexp(alpha[T - 1, -1], alpha[T - 1, -2]) if L else alpha[T - 1, 0]
    dead = np.isinf(alpha) | np.isinf(beta)
    with np.errstate(invalid="ignore"):
        x = alpha + beta - lp[:, lab] - logp
    gamma = np.where(dead, dtype(0), np.exp(np.where(dead, dtype(0), x))).astype(dtype)
    occ = np.zeros((T, C), dtype=dtype)
    for s in range(len(lab)):
        occ[:, lab[s]] += gamma[:, s]
    return dtype(logp), occ, gamma[:, 1::2].copy()


def _token_of_frames(labelling, blank):
    """For a frame labelling: per frame the index of the token it emits in the collapsed transcript, -1 on a blank frame."""
    out, k, prev = [], -1, blank
    for c in labelling:
        if c == blank:
            out.append(-1)
        else:
            if c != prev:
                k += 1
            out.append(k)
        prev = c
    return out


def brute_force(probs, blank=0):
    """Every frame labelling of T frames over C labels, grouped by its collapse: {transcript tuple: (sum, occ [T, C], tok [T, L])}
    with sum the probability of the transcript (prod max(p, FLT_MIN) over every labelling that collapses to it) and occ, tok
    the shares of it that carry label c, or are emitted by token k, at frame t -- in float64, by definition."""
    probs = np.asarray(probs, dtype=np.float32)
    T, C = probs.shape
    p = np.maximum(probs, FLT_MIN).astype(np.float64)
    acc = {}
    for labelling in itertools.product(range(C), repeat=T):
        w = 1.0
        for t, c in enumerate(labelling):
            w *= p[t, c]
        key = tuple(aref.collapse(labelling, blank))
        if key not in acc:
            acc[key] = [0.0, np.zeros((T, C)), np.zeros((T, len(key)))]
        e = acc[key]
        e[0] += w
        for t, (c, k) in enumerate(zip(labelling, _token_of_frames(labelling, blank))):
            e[1][t, c] += w
            if k >= 0:
                e[2][t, k] += w
    return {key: (s, occ / s, tok / s) for key, (s, occ, tok) in acc.items()}
