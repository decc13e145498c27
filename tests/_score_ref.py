"""Reference of CTC transcript scoring (dsmi_score, csrc/score.hip) in numpy: the forward recurrence of include/dsmi.h with the
data type as a parameter (float64 is the contract's; np.longdouble measures float64's own rounding), and a brute force that sums
the probability of every frame labelling whose collapse is the transcript.  A helper module of the tests (not collected)."""
import itertools

import numpy as np

import _align_ref as aref

FLT_MIN = aref.FLT_MIN


def bound(T, ref):
    """The contract's bound on |logp - the exact recurrence|: 8 T 2^-52 max(1, |ref|)."""
    return 8.0 * max(T, 1) * 2.0 ** -52 * max(1.0, abs(float(ref)))


def _lse3(a0, a1, a2):
    """Elementwise log(exp(a0) + exp(a1) + exp(a2)) in the arrays' type; all -inf gives -inf."""
    m = np.maximum(a0, np.maximum(a1, a2))
    safe = np.where(np.isinf(m), 0, m).astype(a0.dtype)
    with np.errstate(divide="ignore"):
        out = safe + np.log(np.exp(a0 - safe) + np.exp(a1 - safe) + np.exp(a2 - safe))
    return np.where(np.isinf(m), m, out).astype(a0.dtype)


def forward(probs, targets, blank=0, dtype=np.float64):
    """probs [T, C] (the clip's frames only), targets: label ids.  None when infeasible, else logp in ``dtype``."""
    probs = np.asarray(probs, dtype=np.float32)
    T, L = probs.shape[0], len(targets)
    if aref.min_frames(targets) > T:
        return None
    if T == 0:
        return dtype(0)
    S = 2 * L + 1
    lab = aref.state_labels(targets, blank)
    skip = np.array([s % 2 == 1 and s >= 3 and lab[s] != lab[s - 2] for s in range(S)])
    lp = aref.log_probs(probs, dtype)
    ninf = dtype(-np.inf)
    alpha = np.full(S, ninf, dtype=dtype)
    alpha[0] = lp[0, blank]
    if L:
        alpha[1] = lp[0, lab[1]]
    for t in range(1, T):
        a1 = np.concatenate(([ninf], alpha[:-1])).astype(dtype)
        a2 = np.concatenate(([ninf, ninf], alpha[:-2]))[:S].astype(dtype)
        a2[~skip] = ninf
        alpha = (_lse3(alpha, a1, a2) + lp[t, lab]).astype(dtype)
    last = alpha[S - 2:S - 1] if L else np.full(1, ninf, dtype=dtype)
    return _lse3(alpha[S - 1:], last, np.full(1, ninf, dtype=dtype))[0]


def brute_force(probs, blank=0):
    """Every frame labelling of T frames over C labels, grouped by its collapse: {transcript tuple: sum of prod max(p, FLT_MIN)}
    in float64 (the enumeration of _align_ref.brute_force, summed and not maximised)."""
    probs = np.asarray(probs, dtype=np.float32)
    T, C = probs.shape
    p = np.maximum(probs, FLT_MIN).astype(np.float64)
    out = {}
    for labelling in itertools.product(range(C), repeat=T):
        w = 1.0
        for t, c in enumerate(labelling):
            w *= p[t, c]
        key = tuple(aref.collapse(labelling, blank))
        out[key] = out.get(key, 0.0) + w
    return out


def all_sequences(T, C, blank=0):
    """Every label sequence of length 0 .. T over the non-blank labels."""
    labels = [c for c in range(C) if c != blank]
    for n in range(T + 1):
        for seq in itertools.product(labels, repeat=n):
            yield list(seq)


def peaky(rng, T, C, sharp=4.0, blank_boost=1.5):
    """Softmax rows with a favoured blank, as the alignment tests use."""
    z = rng.normal(size=(T, C)) * sharp
    z[:, 0] += blank_boost * sharp
    z -= z.max(1, keepdims=True)
    p = np.exp(z)
    return (p / p.sum(1, keepdims=True)).astype(np.float32)
