"""Reference of long-form CTC forced alignment (dsmi_align_long: csrc/ctc_tools.hip, the kernels csrc/align_long.hip) in numpy.
``viterbi`` is tests/_align_ref.viterbi with the two flags: a free blank state costs 0 at every frame it holds, frame 0
included; with both flags off it is that function bit for bit.  ``tiled`` computes the same thing the way the kernels do --
forward tiles of W states with a halo of 2F recomputed states, one checkpoint row per F frames, no stored backpointers, a
backtrace that recomputes a window of 2n + 1 states per frame tile -- and ``brute_force`` enumerates every path of a tiny
case.  A helper module of the tests (not collected)."""
import numpy as np

import _align_ref as ar


def _setup(probs, targets, blank, lead_free, tail_free, dtype):
    """lab [S], skip [S] and lp [T, S]: the log probability of each state's label, 0 for a free state."""
    L = len(targets)
    S = 2 * L + 1
    lab = ar.state_labels(targets, blank)
    skip = np.array([s % 2 == 1 and s >= 3 and lab[s] != lab[s - 2] for s in range(S)])
    lps = ar.log_probs(probs, dtype)[:, lab]
    if lead_free:
        lps[:, 0] = 0
    if tail_free:
        lps[:, S - 1] = 0
    return lab, skip, lps


def _step(alpha, skip, lp_row, dtype):
    """One frame of the recurrence on a row (whole, or a window with -inf assumed to its left): the new row and the
    backpointers (0, 1, 2).  Strict comparisons: on equal alpha s wins, then s - 1, then s - 2."""
    ninf = dtype(-np.inf)
    n = len(alpha)
    pad = np.full(n + 2, ninf, dtype=dtype)
    pad[2:] = alpha
    a1 = pad[1:n + 1]
    a2 = np.where(skip, pad[:n], ninf)
    m1 = a1 > alpha
    best = np.where(m1, a1, alpha)
    m2 = a2 > best
    best = np.where(m2, a2, best)
    k = np.where(m2, 2, m1).astype(np.int8)
    return (best + lp_row).astype(dtype), k


def _first_row(lps, S, dtype):
    alpha = np.full(S, dtype(-np.inf), dtype=dtype)
    alpha[:2] = lps[0, :2]
    return alpha


def _finish(probs, targets, path, logp):
    L = len(targets)
    spans = np.zeros((L, 2), dtype=np.int32)
    tp = np.zeros(L, dtype=np.float32)
    for k in range(L):
        fr = np.nonzero(path == 2 * k + 1)[0]
        spans[k] = (fr[0], fr[-1] + 1)
        acc = np.float32(0)
        for t in range(fr[0], fr[-1] + 1):
            acc = np.float32(acc + probs[t, targets[k]])
        tp[k] = np.float32(acc / np.float32(len(fr)))
    return dict(path=path, spans=spans, token_probs=tp, path_logp=logp)


def viterbi(probs, targets, lead_free=False, tail_free=False, blank=0, dtype=np.float32):
    """probs [T, C] with T >= 1, targets: label ids.  None when infeasible, else _align_ref.viterbi's dict."""
    probs = np.asarray(probs, dtype=np.float32)
    T, L = probs.shape[0], len(targets)
    if ar.min_frames(targets) > T:
        return None
    S = 2 * L + 1
    lab, skip, lps = _setup(probs, targets, blank, lead_free, tail_free, dtype)
    alpha = _first_row(lps, S, dtype)
    bp = np.zeros((T, S), dtype=np.int8)
    for t in range(1, T):
        alpha, bp[t] = _step(alpha, skip, lps[t], dtype)
    s = S - 1
    if L and alpha[S - 2] > alpha[S - 1]:
        s = S - 2
    logp = alpha[s]
    path = np.zeros(T, dtype=np.int64)
    path[T - 1] = s
    for t in range(T - 1, 0, -1):
        s -= int(bp[t, s])
        path[t - 1] = s
    return _finish(probs, targets, path, logp)


def tiled(probs, targets, W, F, lead_free=False, tail_free=False, blank=0, dtype=np.float32, skip_unreached=True):
    """The same result by the kernels' scheme.  Also returns ``rows``, the checkpoint rows [frame tiles + 1, S]."""
    probs = np.asarray(probs, dtype=np.float32)
    T, L = probs.shape[0], len(targets)
    if ar.min_frames(targets) > T:
        return None
    S = 2 * L + 1
    ninf = dtype(-np.inf)
    lab, skip, lps = _setup(probs, targets, blank, lead_free, tail_free, dtype)
    n_ft = (T - 1 + F - 1) // F
    rows = np.full((n_ft + 1, S), dtype(np.nan), dtype=dtype)       # (a cell that is never stored would show)
    rows[0] = _first_row(lps, S, dtype)

    def window(row, lo, hi):        # row[lo:hi] with -inf below state 0
        out = np.full(hi - lo, ninf, dtype=dtype)
        out[max(0, -lo):] = row[max(lo, 0):hi]
        return out

    def run(j, lo, hi, keep_bp):
        """frames j F + 1 .. of the states lo .. hi - 1 from checkpoint j; states below 0 stay -inf"""
        t0 = j * F
        n = min(F, T - 1 - t0)
        x0 = max(0, -lo)
        al = window(rows[j], lo, hi)
        bps = np.zeros((n, hi - lo), dtype=np.int8)
        for r in range(n):
            new, k = _step(al[x0:], skip[lo + x0:hi], lps[t0 + 1 + r, lo + x0:hi], dtype)
            al = np.concatenate((al[:x0], new))
            bps[r, x0:] = k
        return al, bps, n

    for j in range(n_ft):
        for s0 in range(0, S, W):
            s1 = min(s0 + W, S)
            lo = s0 - 2 * F
            if skip_unreached and lo > 2 * j * F + 1:
                rows[j + 1, s0:s1] = ninf
                continue
            al, _, _ = run(j, lo, s1, False)
            rows[j + 1, s0:s1] = al[s0 - lo:]
    fin = rows[n_ft]
    s = S - 1
    if L and fin[S - 2] > fin[S - 1]:
        s = S - 2
    logp = fin[s]
    path = np.zeros(T, dtype=np.int64)
    path[T - 1] = s
    for j in range(n_ft - 1, -1, -1):
        t0 = j * F
        n = min(F, T - 1 - t0)
        lo = s - 2 * n
        _, bps, _ = run(j, lo, s + 1, True)
        for r in range(n - 1, -1, -1):
            s -= int(bps[r, s - lo])
            path[t0 + r] = s
    out = _finish(probs, targets, path, logp)
    out["rows"] = rows
    return out


def brute_force(probs, targets, lead_free=False, tail_free=False, blank=0):
    """The float64 optimum over every path, for tiny cases: a free end is the best over the clips with that end trimmed (lp <= 0:
    a blank that costs something is dominated by a longer free stretch).  None when infeasible."""
    probs = np.asarray(probs, dtype=np.float32)
    T = probs.shape[0]
    best = None
    for a in (range(T + 1) if lead_free else (0,)):
        for b in (range(a, T + 1) if tail_free else (T,)):
            if b < a:
                continue
            if b == a:
                got = (0.0, 1) if len(targets) == 0 else None
            else:
                got = ar.brute_force(probs[a:b], targets, blank)
            if got is not None and (best is None or got[0] > best):
                best = got[0]
    return best
