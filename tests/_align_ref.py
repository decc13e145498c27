"""Reference of CTC forced alignment (dsmi_align: csrc/ctc_tools.hip, the kernel csrc/align.hip) in numpy: the same lp = log(max(p, FLT_MIN)) in float32, the
same order of additions and the same tie rule (include/dsmi.h), so that its float32 results are the kernel's up to the last
bits of log.  Also a float64 re-scorer of a given path and a brute-force enumeration of every CTC path for tiny cases.  A
helper module of the tests (not collected)."""
import itertools

import numpy as np

FLT_MIN = np.finfo(np.float32).tiny


def log_probs(probs, dtype=np.float32):
    p = np.asarray(probs, dtype=np.float32)
    return np.log(np.maximum(p, FLT_MIN).astype(dtype)).astype(dtype)


def min_frames(targets):
    """Frames a transcript needs: one per token and one blank between two equal neighbours."""
    t = list(targets)
    return len(t) + sum(1 for a, b in zip(t, t[1:]) if a == b)


def state_labels(targets, blank=0):
    S = 2 * len(targets) + 1
    return np.array([blank if s % 2 == 0 else int(targets[s // 2]) for s in range(S)], dtype=np.int64)


def viterbi(probs, targets, blank=0, dtype=np.float32):
    """probs [T, C] (the clip's frames only), targets: label ids.  None when infeasible, else a dict with the state path
    [T], spans [L, 2] (frames [start, end) in state 2k + 1), token_probs [L] (float32 mean of p, frames in order) and
    path_logp (the final alpha, in ``dtype``)."""
    probs = np.asarray(probs, dtype=np.float32)
    T, L = probs.shape[0], len(targets)
    if min_frames(targets) > T:
        return None
    S = 2 * L + 1
    lab = state_labels(targets, blank)
    skip = np.array([s % 2 == 1 and s >= 3 and lab[s] != lab[s - 2] for s in range(S)])
    spans = np.zeros((L, 2), dtype=np.int32)
    tp = np.zeros(L, dtype=np.float32)
    if T == 0:
        return dict(path=np.zeros(0, dtype=np.int64), spans=spans, token_probs=tp, path_logp=dtype(0))
    lp = log_probs(probs, dtype)
    ninf = dtype(-np.inf)
    alpha = np.full(S, ninf, dtype=dtype)
    alpha[0] = lp[0, blank]
    if L:
        alpha[1] = lp[0, lab[1]]
    bp = np.zeros((T, S), dtype=np.int8)
    for t in range(1, T):
        a1 = np.concatenate(([ninf], alpha[:-1]))
        a2 = np.concatenate(([ninf, ninf], alpha[:-2]))[:S]
        a2[~skip] = ninf
        best = alpha.copy()
        k = np.zeros(S, dtype=np.int8)
        m = a1 > best                      # strict: on equal alpha s wins, then s - 1, then s - 2
        best[m] = a1[m]
        k[m] = 1
        m = a2 > best
        best[m] = a2[m]
        k[m] = 2
        alpha = (best + lp[t, lab]).astype(dtype)
        bp[t] = k
    s = S - 1
    if L and alpha[S - 2] > alpha[S - 1]:   # the trailing blank unless the last token is strictly better
        s = S - 2
    logp = alpha[s]
    path = np.zeros(T, dtype=np.int64)
    path[T - 1] = s
    for t in range(T - 1, 0, -1):
        s -= int(bp[t, s])
        path[t - 1] = s
    for k in range(L):
        fr = np.nonzero(path == 2 * k + 1)[0]
        spans[k] = (fr[0], fr[-1] + 1)
        acc = np.float32(0)
        for t in range(fr[0], fr[-1] + 1):
            acc = np.float32(acc + probs[t, targets[k]])
        tp[k] = np.float32(acc / np.float32(len(fr)))
    return dict(path=path, spans=spans, token_probs=tp, path_logp=logp)


def path_from_spans(spans, targets, T, blank=0):
    """The frame labels of a path given by its token spans (blank outside them); asserts that they form a CTC path of
    `targets`: spans in order, non-empty, inside [0, T), a blank between two equal neighbours."""
    lab = np.full(T, blank, dtype=np.int64)
    prev_end = 0
    for k, (a, b) in enumerate(np.asarray(spans).reshape(-1, 2)):
        assert prev_end <= a < b <= T, (k, a, b, prev_end, T)
        if k and targets[k] == targets[k - 1]:
            assert a > prev_end, ("no blank between equal tokens", k)
        lab[a:b] = targets[k]
        prev_end = b
    return lab


def collapse(frame_labels, blank=0):
    out, prev = [], None
    for c in frame_labels:
        if c != prev and c != blank:
            out.append(int(c))
        prev = c
    return out


def rescore64(probs, frame_labels):
    """Sum over frames of log(max(p(t, label_t), FLT_MIN)) in float64."""
    p = np.asarray(probs, dtype=np.float32)
    return float(np.sum(np.log(np.maximum(p[np.arange(len(frame_labels)), frame_labels], FLT_MIN).astype(np.float64))))


def brute_force(probs, targets, blank=0):
    """Every frame labelling of T frames over C labels whose collapse is `targets`: (best float64 score, count) or None."""
    probs = np.asarray(probs, dtype=np.float32)
    T, C = probs.shape
    allp = np.array(list(itertools.product(range(C), repeat=T)), dtype=np.int64).reshape(-1, T)
    keep = allp != blank
    keep[:, 1:] &= allp[:, 1:] != allp[:, :-1]
    L = len(targets)
    rows = allp[keep.sum(1) == L]
    kr = keep[keep.sum(1) == L]
    if L:
        seqs = rows[kr].reshape(-1, L)
        rows = rows[np.all(seqs == np.asarray(targets, dtype=np.int64)[None, :], axis=1)]
    if len(rows) == 0:
        return None
    lp = np.log(np.maximum(probs, FLT_MIN).astype(np.float64))
    scores = lp[np.arange(T)[None, :], rows].sum(1)
    return float(scores.max()), len(rows)
