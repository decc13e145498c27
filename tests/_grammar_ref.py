"""Reference of CTC grammar decoding (dsmi_grammar: csrc/ctc_tools.hip, the kernel csrc/grammar.hip) in numpy: the recurrence of
include/dsmi.h over a token graph, with the same lp = log(max(p, FLT_MIN)), the same order of additions and the same tie rule, so
that its float32 results are the kernel's up to the last bits of log.  Also a float64 re-scorer of a returned path (weights
included), an acceptor (a weighted NFA walk over label sentences) and a brute force over all C^T frame labellings for tiny
cases.  A helper module of the tests (not collected)."""
import itertools
from types import SimpleNamespace

import numpy as np

from _align_ref import FLT_MIN, collapse, log_probs

START, FINAL = 1, 2


def graph(labels, flags, preds, weights=None, empty_ok=False):
    """A graph from per-node lists: labels, flags (START | FINAL), preds (a list of predecessor ids per node, in order)."""
    g = SimpleNamespace()
    g.labels = np.asarray(labels, dtype=np.int32).reshape(-1)
    g.flags = np.asarray(flags, dtype=np.int32).reshape(-1)
    g.weights = None if weights is None else np.asarray(weights, dtype=np.float32).reshape(-1)
    g.arc_off = np.zeros(len(g.labels) + 1, dtype=np.int32)
    g.arc_off[1:] = np.cumsum([len(p) for p in preds])
    g.arc_pred = np.array([q for p in preds for q in p], dtype=np.int32)
    g.empty_ok = bool(empty_ok)
    return g


def chain(targets):
    """The chain graph of a transcript: dsmi_align's trellis."""
    L = len(targets)
    flags = [(START if k == 0 else 0) | (FINAL if k == L - 1 else 0) for k in range(L)]
    return graph(targets, flags, [[k - 1] if k else [] for k in range(L)], None, L == 0)


def _weights(g, dtype):
    N = len(g.labels)
    return np.zeros(N, dtype=dtype) if g.weights is None else np.asarray(g.weights, dtype=np.float32).astype(dtype)


def viterbi(probs, g, blank=0, dtype=np.float32):
    """probs [T, C] (the clip's frames only).  None when no accepted sentence fits, else a dict with nodes [M], spans [M, 2],
    token_probs [M] (float32 mean of p, frames in order), path_logp (in ``dtype``) and frame_labels [T]."""
    probs = np.asarray(probs, dtype=np.float32)
    T, N = probs.shape[0], len(g.labels)
    lab = np.asarray(g.labels, dtype=np.int64)
    if T == 0:
        if not g.empty_ok:
            return None
        return dict(nodes=np.zeros(0, np.int32), spans=np.zeros((0, 2), np.int32), token_probs=np.zeros(0, np.float32),
                    path_logp=dtype(0), frame_labels=np.zeros(0, np.int64))
    w = _weights(g, dtype)
    start = (np.asarray(g.flags) & START) != 0
    final = (np.asarray(g.flags) & FINAL) != 0
    off = np.asarray(g.arc_off, dtype=np.int64)
    fan = off[1:] - off[:-1]
    lp = log_probs(probs, dtype)
    ninf = dtype(-np.inf)
    lead = lp[0, blank]
    tok = np.where(start, (lp[0, lab] + w).astype(dtype), ninf).astype(dtype)
    blk = np.full(N, ninf, dtype=dtype)
    STAY, LEAD, BLK, TOK = 0, 1, 2, 3
    kind = np.zeros((T, N), dtype=np.int8)
    frm = np.zeros((T, N), dtype=np.int64)
    bfrom = np.zeros((T, N), dtype=bool)
    # a node's entry candidates in the contract's order, as indices into [lead, blk (N), tok (N), -inf]: lead (start nodes), then per
    # predecessor blk and tok (where the labels differ).  np.argmax takes the first of the greatest: a later candidate replaces
    # an earlier one only when strictly greater.
    NONE = 2 * N + 1
    cols = np.full((N, 1 + 2 * (int(fan.max()) if N else 0)), NONE, dtype=np.int64)
    cols[start, 0] = 0
    ap = np.asarray(g.arc_pred, dtype=np.int64)
    for n in range(N):
        p = ap[off[n]:off[n + 1]]
        cols[n, 1:1 + 2 * len(p):2] = 1 + p
        cols[n, 2:2 + 2 * len(p):2] = np.where(lab[p] != lab[n], 1 + N + p, NONE)
    rows = np.arange(N)
    for t in range(1, T):
        cand = np.concatenate(([lead], blk, tok, [ninf])).astype(dtype)[cols]
        col = cand.argmax(1)
        ent = cand[rows, col]
        src = cols[rows, col]
        ek = np.where(col == 0, LEAD, np.where(col % 2 == 1, BLK, TOK)).astype(np.int8)
        ep = np.where(col % 2 == 1, src - 1, src - 1 - N)
        cand = (ent + w).astype(dtype)
        m = cand > tok                   # strict: stay wins on equal
        best = np.where(m, cand, tok)
        kind[t], frm[t] = np.where(m, ek, STAY), ep
        bm = tok > blk
        bfrom[t] = bm
        nblk = (np.where(bm, tok, blk) + lp[t, blank]).astype(dtype)
        tok = (best + lp[t, lab]).astype(dtype)
        blk = nblk
        lead = dtype(lead + lp[t, blank])
    # ---- the end: lead (empty_ok), then the final nodes ascending, blk before tok; strictly greater replaces
    best, state = ninf, None
    if g.empty_ok:
        best, state = lead, ("lead", 0)
    for n in np.nonzero(final)[0]:
        if blk[n] > best:
            best, state = blk[n], ("blk", int(n))
        if tok[n] > best:
            best, state = tok[n], ("tok", int(n))
    if state is None:
        return None
    frame_labels = np.full(T, blank, dtype=np.int64)
    visits = []
    k, n = state
    end = None
    for t in range(T - 1, -1, -1):
        if k == "lead":
            break
        if k == "blk":
            if bfrom[t, n]:
                k = "tok"
            continue
        frame_labels[t] = lab[n]
        if end is None:
            end = t + 1
        if t == 0 or kind[t, n] != STAY:
            visits.append((n, t, end))
            end = None
            if t == 0:
                break
            kd, p = kind[t, n], int(frm[t, n])
            k, n = ("lead", 0) if kd == LEAD else ("blk", p) if kd == BLK else ("tok", p)
    visits.reverse()
    nodes = np.array([v[0] for v in visits], dtype=np.int32)
    spans = np.array([[v[1], v[2]] for v in visits], dtype=np.int32).reshape(-1, 2)
    tp = np.zeros(len(visits), dtype=np.float32)
    for i, (n, a, b) in enumerate(visits):
        acc = np.float32(0)
        for t in range(a, b):
            acc = np.float32(acc + probs[t, lab[n]])
        tp[i] = np.float32(acc / np.float32(b - a))
    return dict(nodes=nodes, spans=spans, token_probs=tp, path_logp=best, frame_labels=frame_labels)


def path_labels(g, nodes, spans, T, blank=0):
    """The frame labels of a returned path; asserts that it is a path of the graph: the first node a start node, the last a
    final one, every step an arc, spans in order and non-empty inside [0, T), a gap (a blank) between two nodes of one label,
    and no gap inside what would then be one visit."""
    lab = np.full(T, blank, dtype=np.int64)
    nodes = [int(n) for n in nodes]
    spans = np.asarray(spans).reshape(-1, 2)
    if not nodes:
        assert g.empty_ok
        return lab
    assert g.flags[nodes[0]] & START and g.flags[nodes[-1]] & FINAL, (nodes[0], nodes[-1])
    prev_end = 0
    for i, (n, (a, b)) in enumerate(zip(nodes, spans)):
        assert prev_end <= a < b <= T, (i, a, b, prev_end, T)
        if i:
            p = nodes[i - 1]
            assert p in list(g.arc_pred[g.arc_off[n]:g.arc_off[n + 1]]), ("no such arc", p, n)
            if g.labels[p] == g.labels[n]:
                assert a > prev_end, ("no blank between equal labels", i)
        lab[a:b] = g.labels[n]
        prev_end = b
    return lab


def rescore64(probs, frame_labels, g=None, nodes=()):
    """Sum over frames of log(max(p(t, label_t), FLT_MIN)) in float64, plus the weights of the path's nodes."""
    p = np.asarray(probs, dtype=np.float32)
    s = float(np.sum(np.log(np.maximum(p[np.arange(len(frame_labels)), frame_labels], FLT_MIN).astype(np.float64))))
    if g is not None and g.weights is not None:
        s += float(np.sum(np.asarray(g.weights, dtype=np.float32).astype(np.float64)[list(nodes)]))
    return s


def accept(g, sentence):
    """A weighted NFA walk: the greatest sum of node weights (float64) over the node paths that spell the label sentence, or
    None when the graph does not accept it."""
    sentence = [int(c) for c in sentence]
    if not sentence:
        return 0.0 if g.empty_ok else None
    w = _weights(g, np.float64)
    cur = None
    for c in sentence:
        nxt = {}
        for n in np.nonzero(np.asarray(g.labels) == c)[0]:
            n = int(n)
            if cur is None:
                if g.flags[n] & START:
                    nxt[n] = w[n]
            else:
                inn = [cur[int(p)] for p in g.arc_pred[g.arc_off[n]:g.arc_off[n + 1]] if int(p) in cur]
                if inn:
                    nxt[n] = max(inn) + w[n]
        if not nxt:
            return None
        cur = nxt
    ends = [v for n, v in cur.items() if g.flags[n] & FINAL]
    return float(max(ends)) if ends else None


def brute_force(probs, g, blank=0):
    """Every frame labelling of T frames over C labels whose collapse the graph accepts: the best float64 score, weights
    included, or None when there is none."""
    probs = np.asarray(probs, dtype=np.float32)
    T, C = probs.shape
    lp = np.log(np.maximum(probs, FLT_MIN).astype(np.float64))
    known, best = {}, None
    for frames in itertools.product(range(C), repeat=T):
        s = tuple(collapse(frames, blank))
        if s not in known:
            known[s] = accept(g, s)
        if known[s] is None:
            continue
        v = float(lp[np.arange(T), list(frames)].sum()) + known[s]
        if best is None or v > best:
            best = v
    return best
