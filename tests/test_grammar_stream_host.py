"""Streaming grammar decoding without a GPU: dsmi_grammar_stream_plan's numbers and refusals against the rules written out
plainly, and the definition of a partial result -- the numpy reference on the graph with every node final and empty_ok equals a
brute force over "the best path into any state"."""
import itertools

import numpy as np
import pytest

import _grammar_ref as gref
from _align_ref import FLT_MIN, collapse
from test_grammar_host import random_graph


@pytest.fixture(scope="module")
def native():
    from danspeech_amd import _native
    return _native


def test_plan_numbers_against_the_rules(native):
    rng = np.random.default_rng(3)
    cases = [(28, 60, 29, 1500), (native.GRAMMAR_MAX_NODES, native.GRAMMAR_MAX_ARCS, 128, 1500), (0, 0, 1, 1), (1, 0, 2, 1), (301, 300, 29, 39),
             (5, 7, 33, native.GRAMMAR_STREAM_MAX_FRAMES)]
    cases += [(int(rng.integers(0, 2049)), int(rng.integers(0, 8193)), int(rng.integers(1, 129)), int(rng.integers(1, 5000))) for _ in range(40)]
    for N, A, C, F in cases:
        p = native.grammar_stream_plan(N, A, C, F)
        stride = max(4, (N + 3) // 4 * 4)
        # LDS: the pairs double-buffered (8 bytes), node words and weights (4 each), arc offsets and arcs (2 each, the arcs rounded
        # up to 4), the feeder's two images of 16 frames x 128 labels and 256 16-bit words of heavy nodes
        lds = 16 * stride + 8 * stride + 2 * (stride + 4) + 2 * ((A + 3) // 4 * 4) + 2 * 4 * 16 * 128 + 2 * 256
        # the block: a 16-byte header, a pair per node, the rows and the backpointers of max_frames frames
        block = 16 + 8 * stride + 4 * F * C + 2 * F * stride
        assert p == dict(node_stride=stride, lds_bytes=lds, block_bytes=block), (N, A, C, F)
    assert native.grammar_stream_plan(28, 0, 29, 1500)["block_bytes"] - (16 + 8 * 28 + 4 * 1500 * 29) == 84000       # 84 KB of backpointers
    assert 2 * 1500 * 2048 == 6144000                                                                                  # 6.1 MB at the node limit
    assert native.grammar_stream_plan(native.GRAMMAR_MAX_NODES, native.GRAMMAR_MAX_ARCS, 128, 1)["lds_bytes"] <= 160 * 1024


def test_plan_refusals(native):
    INV, CAP = native.DSMI_ERR_INVALID, native.DSMI_ERR_CAPACITY
    top = native.GRAMMAR_STREAM_MAX_FRAMES
    for args, code in (((5, 5, 29, 0), INV), ((5, 5, 29, -4), INV), ((5, 5, 29, top + 1), CAP), ((native.GRAMMAR_MAX_NODES + 1, 0, 29, 10), CAP),
                       ((5, native.GRAMMAR_MAX_ARCS + 1, 29, 10), CAP), ((-1, 0, 29, 10), INV), ((5, -1, 29, 10), INV), ((5, 5, 0, 10), INV),
                       ((5, 5, 129, 10), INV), ((native.GRAMMAR_MAX_NODES, 0, 128, top), CAP)):      # (the last: 4.8 GB of block)
        with pytest.raises(native.DsmiError) as e:
            native.grammar_stream_plan(*args)
        assert e.value.code == code, args
    assert native.lib().dsmi_grammar_stream_plan(5, 5, 29, 10, None) == INV
    native.grammar_stream_plan(native.GRAMMAR_MAX_NODES, native.GRAMMAR_MAX_ARCS, 128, 100000)      # 0.46 GB: within the cap


def _any_state_brute_force(probs, g, blank=0):
    """The best float64 score of a frame labelling that follows the graph from a start node (or stays in the leading blank) and
    may stop in any state: every labelling whose collapse is a sentence PREFIX the graph can walk."""
    T, C = probs.shape
    lp = np.log(np.maximum(probs, FLT_MIN).astype(np.float64))
    w = np.zeros(len(g.labels)) if g.weights is None else np.asarray(g.weights, dtype=np.float32).astype(np.float64)

    def walk(sentence):                  # the greatest weight of a node path from a start node that spells it, any last node
        cur = None
        for c in sentence:
            nxt = {}
            for n in np.nonzero(np.asarray(g.labels) == c)[0]:
                n = int(n)
                if cur is None:
                    if g.flags[n] & gref.START:
                        nxt[n] = w[n]
                else:
                    inn = [cur[int(p)] for p in g.arc_pred[g.arc_off[n]:g.arc_off[n + 1]] if int(p) in cur]
                    if inn:
                        nxt[n] = max(inn) + w[n]
            if not nxt:
                return None
            cur = nxt
        return 0.0 if cur is None else max(cur.values())

    known, best = {}, None
    for frames in itertools.product(range(C), repeat=T):
        s = tuple(collapse(frames, blank))
        if s not in known:
            known[s] = walk(s)
        if known[s] is None:
            continue
        v = float(lp[np.arange(T), list(frames)].sum()) + known[s]
        if best is None or v > best:
            best = v
    return best


def test_the_partial_is_the_best_path_into_any_state():
    rng = np.random.default_rng(19)
    differs = 0
    for case in range(36):
        T, C = 1 + case % 6, 4
        g = random_graph(rng, C)
        probs = np.full((T, C), 0.25, dtype=np.float32) if case % 5 == 0 else rng.dirichlet(np.ones(C) * 0.5, size=T).astype(np.float32)
        every = gref.graph(g.labels, np.asarray(g.flags) | gref.FINAL, [list(g.arc_pred[g.arc_off[n]:g.arc_off[n + 1]]) for n in range(len(g.labels))],
                           g.weights, True)
        got = gref.viterbi(probs, every)
        best = _any_state_brute_force(probs, g)
        assert got is not None and best is not None              # the leading blank is always a state to stop in
        assert abs(float(got["path_logp"]) - best) < 1e-5, (case, float(got["path_logp"]), best)
        frames = got["frame_labels"]
        assert abs(gref.rescore64(probs, frames, every, got["nodes"]) - best) < 1e-5
        own = gref.viterbi(probs, g)
        assert own is None or float(own["path_logp"]) <= float(got["path_logp"]) + 1e-6      # (the accepted ends are among all the states)
        differs += own is None or float(own["path_logp"]) < float(got["path_logp"]) - 1e-6
    assert differs >= 3                  # (the partial is not the graph's own result)
