"""Three independent references for the batched edit distance (dsmi_edit_distance): each returns (distance, substitutions,
deletions, insertions) of the minimum-distance alignment with the fewest substitutions.  A deletion is a token of a with no
partner in b, an insertion a token of b with no partner in a."""
import functools

import numpy as np


def _counts(d, s, la, lb):
    dele = (d - s - (lb - la)) // 2
    return (d, s, dele, dele + lb - la)


def all_optimal(a, b):
    """Every alignment of a and b by recursion (lengths <= 6 or so): the set of (d, s, deletions, insertions) vectors of the
    alignments with the least distance."""
    a, b = tuple(a), tuple(b)

    @functools.lru_cache(maxsize=None)
    def go(i, j):
        # the set of (s, d, i) count vectors of every alignment of a[i:] with b[j:]
        if i == len(a) and j == len(b):
            return frozenset([(0, 0, 0)])
        out = set()
        if i < len(a):
            out.update((s, d + 1, n) for s, d, n in go(i + 1, j))
        if j < len(b):
            out.update((s, d, n + 1) for s, d, n in go(i, j + 1))
        if i < len(a) and j < len(b):
            sub = int(a[i] != b[j])
            out.update((s + sub, d, n) for s, d, n in go(i + 1, j + 1))
        return frozenset(out)

    vecs = go(0, 0)
    best = min(s + d + n for s, d, n in vecs)
    return sorted((s + d + n, s, d, n) for s, d, n in vecs if s + d + n == best)


def brute(a, b):
    """The brute force: the lexicographic minimum of (distance, substitutions) over every alignment, counted directly."""
    return all_optimal(a, b)[0]


def tuple_dp(a, b):
    """Plain dynamic programme over (d, s) tuples with Python's lexicographic min; no packed integers."""
    la, lb = len(a), len(b)
    prev = [(j, 0) for j in range(lb + 1)]
    for i in range(1, la + 1):
        cur = [(i, 0)]
        for j in range(1, lb + 1):
            up, left, dg = prev[j], cur[j - 1], prev[j - 1]
            sub = dg if a[i - 1] == b[j - 1] else (dg[0] + 1, dg[1] + 1)
            cur.append(min((up[0] + 1, up[1]), (left[0] + 1, left[1]), sub))
        prev = cur
    d, s = prev[lb]
    return _counts(d, s, la, lb)


_BIG = 1 << 20      # the weight of the distance over the substitutions in the row form's int64 costs


def row_dp(a, b):
    """Vectorised numpy row form for the large cases, about len(a) numpy operations: with costs d * 2^20 + s in int64,
    t[j] = min(prev[j] + DEL, prev[j-1] + sub_j), then the insertions along the row as a running minimum,
    cur = minimum.accumulate(t - j * INS) + j * INS, which is valid because the insertion cost is constant."""
    a = np.asarray(a, dtype=np.int64).reshape(-1)
    b = np.asarray(b, dtype=np.int64).reshape(-1)
    la, lb = len(a), len(b)
    ramp = np.arange(lb + 1, dtype=np.int64) * _BIG
    prev = ramp.copy()
    for i in range(1, la + 1):
        t = np.empty(lb + 1, dtype=np.int64)
        t[0] = i * _BIG
        t[1:] = np.minimum(prev[1:] + _BIG, prev[:-1] + np.where(b == a[i - 1], 0, _BIG + 1))
        prev = np.minimum.accumulate(t - ramp) + ramp
    d, s = int(prev[lb]) >> 20, int(prev[lb]) & (_BIG - 1)
    return _counts(d, s, la, lb)


def row_dp_batch(A, B):
    """``row_dp`` for P pairs of equal shapes at once: A int [P, la], B int [P, lb] -> int32 [P, 4]."""
    A, B = np.asarray(A, dtype=np.int64), np.asarray(B, dtype=np.int64)
    (P, la), lb = A.shape, B.shape[1]
    ramp = np.arange(lb + 1, dtype=np.int64)[None, :] * _BIG
    prev = np.repeat(ramp, P, axis=0)
    for i in range(1, la + 1):
        t = np.empty((P, lb + 1), dtype=np.int64)
        t[:, 0] = i * _BIG
        t[:, 1:] = np.minimum(prev[:, 1:] + _BIG, prev[:, :-1] + np.where(B == A[:, i - 1:i], 0, _BIG + 1))
        prev = np.minimum.accumulate(t - ramp, axis=1) + ramp
    d, s = prev[:, lb] >> 20, prev[:, lb] & (_BIG - 1)
    dele = (d - s - (lb - la)) // 2
    return np.stack([d, s, dele, dele + lb - la], axis=1).astype(np.int32)


def counts_of(pool, pairs, ref=row_dp):
    """int32 [N, 4] of the pairs (a, b) of pool sequences, by ``ref``."""
    return np.array([ref(pool[a], pool[b]) for a, b in pairs], dtype=np.int32).reshape(-1, 4)
