"""Reference of the CTC grammar posterior (dsmi_grammar_posterior: csrc/ctc_tools.hip, the kernels csrc/grammar_post.hip) in
numpy: the recurrences of include/dsmi.h over a token graph in a chosen dtype (float64 or np.longdouble) -- logp, occ, visits,
status -- with the same lp = log(max(p, FLT_MIN)).  visits is formed by its definition, from the stored entries, and not by the
kernel's difference.  Also the weighted count of the node paths that spell a sentence, a brute force over all C^T frame
labellings for tiny cases, the contract's bound (the tests take their tolerance from nowhere else), deliberately wrong variants
of the recurrence and the inputs the GPU test and the host test share.  A helper module of the tests (not collected)."""
import itertools

import numpy as np

import _grammar_ref as gref
from _align_ref import FLT_MIN, collapse, log_probs

START, FINAL = gref.START, gref.FINAL
VARIANTS = ("equal_labels_enter", "weight_every_frame", "duplicate_arc_ignored")


def fan_in(g):
    """F: the most predecessors of one node."""
    off = np.asarray(g.arc_off, dtype=np.int64)
    return int((off[1:] - off[:-1]).max()) if len(off) > 1 else 0


def bound(T, F, logp):
    """The contract's bound on |occ element - the recurrences evaluated exactly|: k(F) T 2^-52 max(1, |logp| + 88) with
    k(F) = 32 + (F + 1) / 8.  A visits element holds T times it."""
    return (32.0 + (F + 1) / 8.0) * max(T, 1) * 2.0 ** -52 * max(1.0, abs(float(logp)) + 88.0)


def bound_logp(T, F, logp):
    """The contract's bound on |logp - the recurrence evaluated exactly|: dsmi_score's form and the fan-in's term."""
    return 8.0 * max(T, 1) * 2.0 ** -52 * max(1.0, abs(float(logp))) + (F + 1) * max(T, 1) * 2.0 ** -52


def _arcs(g, variant):
    """(src, dst, the two labels differ) of every arc, a predecessor listed twice twice."""
    N = len(g.labels)
    lab = np.asarray(g.labels, dtype=np.int64)
    off = np.asarray(g.arc_off, dtype=np.int64)
    src = np.asarray(g.arc_pred, dtype=np.int64)
    dst = np.repeat(np.arange(N, dtype=np.int64), off[1:] - off[:-1])
    if variant == "duplicate_arc_ignored" and len(src):
        pairs = np.unique(np.stack([dst, src], 1), axis=0)
        dst, src = pairs[:, 0], pairs[:, 1]
    dif = lab[src] != lab[dst] if variant != "equal_labels_enter" else np.ones(len(src), dtype=bool)
    return src, dst, dif


def _lse_into(out, idx, vals):
    if len(idx):
        np.logaddexp.at(out, idx, vals)
    return out


def posterior(probs, g, blank=0, dtype=np.float64, variant=None, lp=None, weights=None):
    """probs [T, C] (the clip's frames only).  A dict: status (1 = no accepted sentence fits; then logp = -inf and zeros),
    logp, occ [T, C], visits [N], in ``dtype``.  ``variant``: one of VARIANTS, a deliberately wrong recurrence.  ``lp`` [T, C] and
    ``weights`` [N] replace the clip's log probabilities and the graph's weights (the finite-difference checks)."""
    probs = np.asarray(probs, dtype=np.float32)
    T, C = probs.shape
    N = len(g.labels)
    lab = np.asarray(g.labels, dtype=np.int64)
    ninf = dtype(-np.inf)
    zeros = dict(status=1, logp=ninf, occ=np.zeros((T, C), dtype=dtype), visits=np.zeros(N, dtype=dtype))
    if T == 0:
        return dict(zeros, status=0, logp=dtype(0)) if g.empty_ok else zeros
    w = gref._weights(g, dtype) if weights is None else np.asarray(weights, dtype=dtype)
    start = (np.asarray(g.flags) & START) != 0
    final = (np.asarray(g.flags) & FINAL) != 0
    lp = log_probs(probs, dtype) if lp is None else np.asarray(lp, dtype=dtype)
    src, dst, dif = _arcs(g, variant)
    every = variant == "weight_every_frame"
    with np.errstate(invalid="ignore", over="ignore"):
        # ---- forward: alpha of tok, blk, lead, and the entries ent + w of every frame
        a_tok = np.full((T, N), ninf, dtype=dtype)
        a_blk = np.full((T, N), ninf, dtype=dtype)
        a_lead = np.zeros(T, dtype=dtype)
        enter = np.full((T, N), ninf, dtype=dtype)
        a_lead[0] = lp[0, blank]
        a_tok[0] = np.where(start, lp[0, lab] + w, ninf)
        enter[0] = np.where(start, w, ninf)
        for t in range(1, T):
            ent = np.where(start, a_lead[t - 1], ninf).astype(dtype)
            _lse_into(ent, dst, a_blk[t - 1][src])
            _lse_into(ent, dst[dif], a_tok[t - 1][src[dif]])
            enter[t] = ent + w
            stay = a_tok[t - 1] + w if every else a_tok[t - 1]
            a_tok[t] = np.logaddexp(stay, enter[t]) + lp[t, lab]
            a_blk[t] = np.logaddexp(a_blk[t - 1], a_tok[t - 1]) + lp[t, blank]
            a_lead[t] = a_lead[t - 1] + lp[t, blank]
        ends = [a_lead[T - 1]] if g.empty_ok else []
        for n in np.nonzero(final)[0]:
            ends += [a_blk[T - 1, n], a_tok[T - 1, n]]
        logp = np.logaddexp.reduce(np.array(ends, dtype=dtype)) if ends else ninf
        if not np.isfinite(logp):
            return zeros
        # ---- backward: beta with the frame's own emission, the mirror image over the successors
        b_tok = np.full((T, N), ninf, dtype=dtype)
        b_blk = np.full((T, N), ninf, dtype=dtype)
        b_lead = np.full(T, ninf, dtype=dtype)
        b_tok[T - 1] = np.where(final, lp[T - 1, lab], ninf)
        b_blk[T - 1] = np.where(final, lp[T - 1, blank], ninf)
        if g.empty_ok:
            b_lead[T - 1] = lp[T - 1, blank]
        for t in range(T - 2, -1, -1):
            into = w + b_tok[t + 1]
            out_all = _lse_into(np.full(N, ninf, dtype=dtype), src, into[dst])
            out_dif = _lse_into(np.full(N, ninf, dtype=dtype), src[dif], into[dst[dif]])
            stay = b_tok[t + 1] + w if every else b_tok[t + 1]
            b_tok[t] = np.logaddexp(np.logaddexp(stay, b_blk[t + 1]), out_dif) + lp[t, lab]
            b_blk[t] = np.logaddexp(b_blk[t + 1], out_all) + lp[t, blank]
            first = np.logaddexp.reduce(into[start]) if start.any() else ninf
            b_lead[t] = np.logaddexp(b_lead[t + 1], first) + lp[t, blank]
        g_tok = np.exp(a_tok + b_tok - lp[:, lab] - logp)
        g_blk = np.exp(a_blk + b_blk - lp[:, [blank]] - logp)
        g_lead = np.exp(a_lead + b_lead - lp[:, blank] - logp)
        occ = np.zeros((T, C), dtype=dtype)
        for n in range(N):               # ascending, as the library's sums are
            occ[:, lab[n]] += g_tok[:, n]
        occ[:, blank] += g_lead
        for n in range(N):
            occ[:, blank] += g_blk[:, n]
        visits = np.exp(enter + b_tok - logp).sum(0).astype(dtype)
    return dict(status=0, logp=dtype(logp), occ=occ, visits=visits)


def accept_logsum(g, sentence):
    """The weighted count of the node paths that spell the label sentence: the log-sum-exp over them of their weights
    (float64), a predecessor listed twice counting twice; None when the graph does not accept it."""
    sentence = [int(c) for c in sentence]
    if not sentence:
        return 0.0 if g.empty_ok else None
    w = gref._weights(g, np.float64)
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
                    nxt[n] = np.logaddexp.reduce(inn) + w[n]
        if not nxt:
            return None
        cur = nxt
    ends = [v for n, v in cur.items() if g.flags[n] & FINAL]
    return float(np.logaddexp.reduce(ends)) if ends else None


def brute_force_sum(probs, g, blank=0):
    """Every frame labelling of T frames over C labels whose collapse the graph accepts: the float64 log of the sum of their
    probabilities times the weighted count of node paths of the collapse, or None when there is none."""
    probs = np.asarray(probs, dtype=np.float32)
    T, C = probs.shape
    lp = np.log(np.maximum(probs, FLT_MIN).astype(np.float64))
    known, terms = {}, []
    for frames in itertools.product(range(C), repeat=T):
        s = tuple(collapse(frames, blank))
        if s not in known:
            known[s] = accept_logsum(g, s)
        if known[s] is not None:
            terms.append(float(lp[np.arange(T), list(frames)].sum()) + known[s])
    return float(np.logaddexp.reduce(terms)) if terms else None


# ---- the inputs that tests/test_gpu_grammar_post.py checks against this reference and tests/test_grammar_post_host.py measures
# the reference on: (name, graph, probs [T, C]) with T <= 60
def dirichlet(rng, T, C, conc=0.3):
    p = rng.dirichlet(np.full(C, conc), size=T).astype(np.float32)
    return np.maximum(p, np.float32(1e-30))


def hand_graph_300(C, rng):
    """301 nodes (no multiple of 4; a thread owns more than one): three start nodes, every later node one to three earlier
    predecessors, weights of both signs, a few self-loops, the last 20 nodes final."""
    N = 301
    labels = rng.integers(1, C, size=N)
    flags = np.zeros(N, dtype=np.int64)
    flags[:3] |= START
    flags[-20:] |= FINAL
    preds = [[]] * 3 + [[int(p) for p in rng.integers(max(0, n - 12), n, size=int(rng.integers(1, 4)))] for n in range(3, N)]
    for n in range(5, N, 37):
        preds[n] = preds[n] + [n]
    weights = rng.normal(size=N).astype(np.float32)
    return gref.graph(labels, flags, preds, weights, False)


def fan_graph_40(C, rng):
    """One start node with 40 successors that all lead into one node with 40 predecessors (both passes reduce such a node by a
    wave), then a tail with a way round its middle node, whose weight is -80."""
    labels = [4] + list(rng.integers(1, C, size=40)) + [1, 2, 3]
    flags = [START] + [0] * 40 + [0, 0, FINAL]
    preds = [[]] + [[0] for _ in range(40)] + [list(range(1, 41)), [41], [42, 41]]
    weights = [0.25] + list(rng.normal(size=40).astype(np.float32)) + [0.5, -80.0, -0.25]
    return gref.graph(labels, flags, preds, weights, False)


def path_cases(C):
    """Paths, not sentences: (name, graph, the chain it is to be set against, the factor by which its paths outnumber the
    chain's, probs).  Two parallel identical nodes in the middle of a chain; a predecessor listed twice."""
    rng = np.random.default_rng(77)
    chain = [3, 5, 5, 2]
    twin = gref.graph([3, 5, 5, 5, 2], [START, 0, 0, 0, FINAL], [[], [0], [0], [1, 2], [3]], None, False)
    twice = gref.graph(chain, [START, 0, 0, FINAL], [[], [0], [1, 1], [2]], None, False)
    return [("twin nodes", twin, gref.chain(chain), 2.0, dirichlet(rng, 12, C, 1.0)),
            ("arc listed twice", twice, gref.chain(chain), 2.0, dirichlet(rng, 12, C, 1.0))]


def reference_cases(labels_text):
    """The compiled grammars and hand-built graphs of the GPU test, each with its clip."""
    from danspeech_amd.grammar import Grammar
    rng = np.random.default_rng(2024)
    C = len(labels_text)
    cases = []
    for name, g, T in [
        ("docstring", Grammar("$digit = nul | en | to | tre ; (tænd | sluk) lyset [i (stuen | køkkenet:-0.5)] $digit*", labels_text), 60),
        ("digit loop", Grammar("(nul | en:0.25 | to:-0.5 | tre | fire | fem)+", labels_text), 50),
        ("five sentences", Grammar.from_sentences(["tænd lyset", "sluk lyset", "tænd for radioen", "hvad er klokken", "stop"], labels_text), 47),
        ("hand 301", hand_graph_300(C, rng), 60),
        ("fan-in 40", fan_graph_40(C, rng), 33),
    ]:
        cases.append((name, g, dirichlet(rng, T, C)))
    return cases
