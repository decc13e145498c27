"""Reference of CTC token confidence (dsmi_alternatives, csrc/alt.hip) in numpy: for every token k of a transcript and every
label c the log likelihood of the transcript with token k replaced by c (c = blank: deleted), out of one forward-backward pass,
with the data type as a parameter (float64 is the contract's; np.longdouble measures float64's own rounding).  Whole trellises
alpha and beta [T, S] first, then every slot at once as [L, C] arrays that step through the frames together; the deletions have
no recursion and are one reduction over the frames.  tests/test_alt_host.py holds it to _score_ref.forward on the variants
themselves.  A helper module of the tests (not collected)."""
import numpy as np

import _align_ref as aref
import _score_ref as sref


def bound(T, ref):
    """The contract's bound on |value - the exact recurrence of the variant|: 24 T 2^-52 max(1, |ref|), three times dsmi_score's."""
    return 3.0 * sref.bound(T, ref)


def variant(targets, k, c, blank=0):
    """The transcript with token k replaced by c, or deleted where c is the blank."""
    t = [int(x) for x in targets]
    return t[:k] + t[k + 1:] if c == blank else t[:k] + [int(c)] + t[k + 1:]


def _trellises(lp, lab, dtype):
    """alpha [T, S] as in _score_ref.forward and beta [T, S]: the log probability of finishing from state s at frame t, frame
    t's emission included."""
    T, S = lp.shape[0], len(lab)
    ninf = dtype(-np.inf)
    hop = np.zeros(S, dtype=bool)                        # s takes from s - 2: a token that differs from the token before
    hop[3::2] = lab[3::2] != lab[1:-2:2]
    alpha = np.full((T, S), ninf, dtype=dtype)
    beta = np.full((T, S), ninf, dtype=dtype)
    alpha[0, :2] = lp[0, lab[:2]]
    beta[T - 1, max(S - 2, 0):] = lp[T - 1, lab[max(S - 2, 0):]]
    for t in range(1, T):
        a = alpha[t - 1].copy()
        a[1:] = np.logaddexp(a[1:], alpha[t - 1, :-1])
        a[hop] = np.logaddexp(a[hop], alpha[t - 1, np.flatnonzero(hop) - 2])
        alpha[t] = a + lp[t, lab]
    for t in range(T - 2, -1, -1):
        b = beta[t + 1].copy()
        b[:-1] = np.logaddexp(b[:-1], beta[t + 1, 1:])
        src = np.flatnonzero(hop) - 2                    # s - 2 hands over to s
        b[src] = np.logaddexp(b[src], beta[t + 1, src + 2])
        beta[t] = b + lp[t, lab]
    return alpha, beta


def alternatives(probs, targets, blank=0, dtype=np.float64):
    """probs [T, C] (the clip's frames only), targets: label ids.  None when infeasible, else (logp, alt [L, C]) in ``dtype``;
    alt[k, c] = -inf where the variant cannot fit the frames."""
    probs = np.asarray(probs, dtype=np.float32)
    T, C = probs.shape
    y = np.array([int(x) for x in targets], dtype=np.int64)
    L = len(y)
    if aref.min_frames(y) > T:
        return None
    if T == 0:
        return dtype(0), np.zeros((0, C), dtype=dtype)
    ninf = dtype(-np.inf)
    lp = aref.log_probs(probs, dtype)
    alpha, beta = _trellises(lp, aref.state_labels(y, blank), dtype)
    logp = np.logaddexp(alpha[T - 1, -1], alpha[T - 1, -2]) if L else alpha[T - 1, 0]
    if L == 0:
        return dtype(logp), np.zeros((0, C), dtype=dtype)
    col = np.full((T, 1), ninf, dtype=dtype)
    before = np.concatenate(([-1], y[:-1]))              # y_{k-1}, y_{k+1}; -1: none
    after = np.concatenate((y[1:], [-1]))
    labels = np.arange(C)[None, :]
    # into slot k: from the blank in front of it, and from the token before it where that is another label than the slot's
    blank_in = alpha[:, 0:2 * L:2]                       # [T, L]  alpha_t(2k)
    both_in = np.logaddexp(blank_in, np.concatenate((col, alpha[:, 1:2 * L - 1:2]), axis=1))
    # out of slot k: into the blank behind it, and into the token behind it where that is another label
    blank_out = beta[:, 2:2 * L + 1:2]                   # [T, L]  beta_t(2k+2)
    token_out = np.concatenate((beta[:, 3:2 * L:2], col), axis=1)
    both_out = np.logaddexp(blank_out, token_out)
    wide_in = (before[:, None] >= 0) & (before[:, None] != labels)          # [L, C]
    wide_out = (after[:, None] >= 0) & (after[:, None] != labels)
    u = np.where(np.arange(L)[:, None] == 0, lp[0][None, :], ninf).astype(dtype)
    alt = np.full((L, C), ninf, dtype=dtype)
    for t in range(T):
        if t:
            u = (np.logaddexp(u, np.where(wide_in, both_in[t - 1][:, None], blank_in[t - 1][:, None])) + lp[t][None, :]).astype(dtype)
        if t < T - 1:
            alt = np.logaddexp(alt, u + np.where(wide_out, both_out[t + 1][:, None], blank_out[t + 1][:, None]))
        else:
            alt[L - 1] = np.logaddexp(alt[L - 1], u[L - 1])
    # deletions: the two blanks around token k are one state; the token before hands over to the token behind where they differ
    gone = np.full(L, ninf, dtype=dtype)
    if L > 1:
        differ = (before[:L - 1] >= 0) & (before[:L - 1] != after[:L - 1])
        entry = np.where(differ[None, :], both_in[:T - 1, :L - 1], blank_in[:T - 1, :L - 1])
        gone[:L - 1] = np.logaddexp.reduce(entry + token_out[1:, :L - 1], axis=0)
        gone[0] = np.logaddexp(gone[0], beta[0, 3])
    gone[L - 1] = both_in[T - 1, L - 1]
    alt[:, blank] = gone
    return dtype(logp), alt.astype(dtype)


def posterior(alt):
    """post[k] = exp(alt[k] - logsumexp(alt[k])): the posterior over slot k's labels given the rest of the transcript."""
    alt = np.asarray(alt)
    with np.errstate(invalid="ignore"):
        return np.exp(alt - np.logaddexp.reduce(alt, axis=1, keepdims=True))
