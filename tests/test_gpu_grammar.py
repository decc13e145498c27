"""CTC grammar decoding on the GPU (dsmi_grammar: csrc/ctc_tools.hip, the kernel csrc/grammar.hip) against a brute force over every
frame labelling, against dsmi_align bit for bit on chain graphs, against the numpy reference of tests/_grammar_ref.py on graphs
compiled by danspeech_amd/grammar.py, its edges and its refusals, and the recogniser surface end to end on a synthetic model."""
import ctypes

import numpy as np
import pytest

from danspeech_amd import synthetic as syn
from danspeech_amd.grammar import Grammar

import _align_ref as aref
import _ctc_edge_cases as edge
import _grammar_ref as gref
from test_grammar_host import random_graph

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
LABELS = syn.DANSPEECH_LABELS


@pytest.fixture(scope="module")
def native():
    from danspeech_amd import _native
    return _native


@pytest.fixture(scope="module")
def dec(native):
    d = native.NativeDecoder(LABELS, blank_index=0)
    yield d
    d.close()


def _padded(probs_list, T=None):
    T = T or max(1, max(len(p) for p in probs_list))
    C = probs_list[0].shape[1]
    x = np.full((len(probs_list), T, C), 1.0 / C, dtype=np.float32)
    for b, p in enumerate(probs_list):
        x[b, :len(p)] = p
    return torch.from_numpy(x).cuda(), np.array([len(p) for p in probs_list], dtype=np.int32)


def _peaky(rng, T, C, sharp=4.0, blank_boost=1.5):
    z = rng.normal(size=(T, C)) * sharp
    z[:, 0] += blank_boost * sharp
    z -= z.max(1, keepdims=True)
    p = np.exp(z)
    return (p / p.sum(1, keepdims=True)).astype(np.float32)


def _rows_past_the_path_are_zero(out, b):
    lens, nodes, spans, tp, lp, st = out
    M = lens[b]
    assert not nodes[b, M:].any() and not spans[b, M:].any() and not tp[b, M:].any()


def _valid(g, out, b, probs):
    """The returned path of clip b is a path of the graph; its frame labels and its float64 score, weights included."""
    lens, nodes, spans, tp, lp, st = out
    M = lens[b]
    _rows_past_the_path_are_zero(out, b)
    frames = gref.path_labels(g, nodes[b, :M], spans[b, :M], len(probs))
    assert gref.accept(g, aref.collapse(frames)) is not None
    for k in range(M):                   # the float32 mean of p(label) over the span, frames in order
        a, e = spans[b, k]
        acc = np.float32(0)
        for t in range(a, e):
            acc = np.float32(acc + probs[t, g.labels[nodes[b, k]]])
        assert tp[b, k] == np.float32(acc / np.float32(e - a))
    return frames, gref.rescore64(probs, frames, g, nodes[b, :M])


# ---- 1. brute force
def test_brute_force_small_cases(native):
    d = native.NativeDecoder(["_", "a", "b", "c"], blank_index=0)
    rng = np.random.default_rng(21)
    graphs, probs = [], []
    for case in range(48):
        T = int(rng.integers(1, 7))
        graphs.append(random_graph(rng, 4))
        probs.append(np.full((T, 4), 0.25, dtype=np.float32) if case % 6 == 0 else rng.dirichlet(np.ones(4) * 0.5, size=T).astype(np.float32))
    p_dev, sizes = _padded(probs)
    out = d.grammar(p_dev, sizes, graphs, np.arange(48))
    lens, nodes, spans, tp, lp, st = out
    decoded = 0
    for b, g in enumerate(graphs):
        best = gref.brute_force(probs[b], g)
        assert st[b] == (1 if best is None else 0), b
        if best is None:
            assert lp[b] == -np.inf and lens[b] == 0
            _rows_past_the_path_are_zero(out, b)
            continue
        decoded += 1
        _, score = _valid(g, out, b, probs[b])
        assert abs(score - best) < 1e-5, (b, score, best)
        assert abs(float(lp[b]) - best) < 1e-5, (b, float(lp[b]), best)
    assert 20 <= decoded < 48            # both outcomes are there
    d.close()


# ---- 2. a chain graph is dsmi_align, bit for bit
def _same_as_align(dec, probs, targets):
    p_dev, sz = _padded(probs)
    spans, tp, lp, status = dec.align(p_dev, sz, targets)
    out = dec.grammar(p_dev, sz, [gref.chain(t) for t in targets], np.arange(len(targets)))
    lens, nodes, gspans, gtp, glp, gst = out
    np.testing.assert_array_equal(gst, status)
    assert glp.tobytes() == lp.tobytes()
    for b, t in enumerate(targets):
        L = 0 if status[b] else len(t)
        assert lens[b] == L
        np.testing.assert_array_equal(nodes[b, :L], np.arange(L))
        np.testing.assert_array_equal(gspans[b, :L], spans[b, :L])
        assert gtp[b, :L].tobytes() == tp[b, :L].tobytes()
        _rows_past_the_path_are_zero(out, b)
    return status


@pytest.mark.parametrize("sharp", [3.0, 6.0])
def test_chain_graph_equals_align_on_the_ragged_batch(dec, sharp):
    rng = np.random.default_rng(int(sharp))
    sizes = [501, 480, 377, 260, 501, 133, 64, 9]
    probs = [_peaky(rng, T, len(LABELS), sharp=sharp) for T in sizes]
    p_dev, sz = _padded(probs)
    greedy = [list(ids) for ids, _ in dec.greedy(p_dev, sz)]
    randoms = []
    for T in sizes:
        L = int(rng.integers(0, T // 6 + 1))
        randoms.append([int(x) for x in rng.integers(1, len(LABELS), size=L)])
    for targets in (greedy, randoms):
        assert not _same_as_align(dec, probs, targets).any()


def test_chain_graph_equals_align_on_ties_and_an_infeasible_clip(dec):
    C = len(LABELS)
    ids = [LABELS.index(c) for c in "alle"]
    cases = [(5, [1, 2]), (5, [1, 1]), (40, ids), (7, ids + ids[:1]), (6, []), (300, ids * 20), (5, ids), (4, ids)]
    probs = [np.full((T, C), 1.0 / C, dtype=np.float32) for T, _ in cases]
    status = _same_as_align(dec, probs, [t for _, t in cases])
    assert status.tolist() == [0] * 7 + [1]                   # "alle" needs five frames


# ---- 3. general graphs against the numpy reference
def _render(rng, g, sentence, C):
    """A clip that says `sentence`: each character 2 to 4 frames of probability 0.9 on its label, one or two blank frames between
    the characters.  Returns (probs, the first frame of each character)."""
    rows, starts = [], []

    def frames(label, n):
        for _ in range(n):
            p = np.full(C, 0.1 / (C - 1), dtype=np.float32)
            p[label] = 0.9
            rows.append(p)
    frames(0, int(rng.integers(0, 3)))
    for c in sentence:
        starts.append(len(rows))
        frames(LABELS.index(c), int(rng.integers(2, 5)))
        frames(0, int(rng.integers(1, 3)))
    return np.array(rows, dtype=np.float32), starts


GRAMMARS = {
    "digits": "$d = nul | en | to | tre | fire | fem | seks | syv | otte | ni ; $d+",
    "sentence": "tænd [venligst] lyset i (stuen | køkkenet | gangen) [nu]",
    "words": None,      # a loop over 120 words of synthetic.make_vocabulary
}


@pytest.fixture(scope="module")
def compiled():
    out = {k: Grammar(v, LABELS) for k, v in GRAMMARS.items() if v}
    out["words"] = Grammar("(" + " | ".join(syn.make_vocabulary(120)) + ")+", LABELS)
    return out


@pytest.mark.parametrize("name", list(GRAMMARS))
def test_general_graphs_against_the_reference(dec, compiled, name):
    g = compiled[name]
    C = len(LABELS)
    rng = np.random.default_rng(len(name))
    # peaky clips of 9 to 501 frames; uniform clips (ties only); clips rendered from sentences of the grammar
    peaky = [_peaky(rng, T, C, sharp=3.0) for T in (501, 333, 120, 40, 9)]
    uniform = [np.full((T, C), 1.0 / C, dtype=np.float32) for T in (60, 17)]
    if name == "words":
        w = syn.make_vocabulary(120)
        said = [" ".join(w[i] for i in (5, 77, 5, 119, 0)), w[60]]
    else:
        some = g.sentences(40)
        said = [some[i] for i in (0, len(some) // 2, len(some) - 1)]
    rendered = [_render(rng, g, s, C) for s in said]
    probs = peaky + uniform + [r[0] for r in rendered]
    p_dev, sz = _padded(probs)
    out = dec.grammar(p_dev, sz, g)
    lens, nodes, spans, tp, lp, st = out
    for b, p in enumerate(probs):
        r32, r64 = gref.viterbi(p, g), gref.viterbi(p, g, dtype=np.float64)
        assert st[b] == (1 if r32 is None else 0), b
        if r32 is None:
            assert lp[b] == -np.inf and lens[b] == 0
            continue
        frames, score = _valid(g, out, b, p)
        assert g.accepts(g.text_of(nodes[b, :lens[b]]))
        assert abs(float(lp[b]) - float(r32["path_logp"])) < 1e-3, (b, float(lp[b]), float(r32["path_logp"]))
        assert abs(score - float(r64["path_logp"])) < 1e-3, (b, score, float(r64["path_logp"]))
        if b >= len(peaky):              # rounding cannot decide: the reference's path, node for node
            np.testing.assert_array_equal(nodes[b, :lens[b]], r32["nodes"])
            np.testing.assert_array_equal(spans[b, :lens[b]], r32["spans"])
    for (p, starts), s, b in zip(rendered, said, range(len(peaky) + len(uniform), len(probs))):
        assert st[b] == 0 and g.text_of(nodes[b, :lens[b]]) == s
        assert spans[b, :lens[b], 0].tolist() == starts


# ---- 4. edges
def _ring(N, rng, C, fan=1):
    """N nodes in a ring (node n's predecessors: n-1 .. n-fan, modulo N), every node a start and a final node."""
    labels = rng.integers(1, C, size=N)
    return gref.graph(labels, [gref.START | gref.FINAL] * N, [[(n - j) % N for j in range(1, fan + 1)] for n in range(N)],
                      -rng.random(N).astype(np.float32))


def _against_reference(dec, graphs, probs, clip_graph, T_out=None, exact=False):
    p_dev, sz = _padded(probs, T_out)
    out = dec.grammar(p_dev, sz, graphs, clip_graph)
    lens, nodes, spans, tp, lp, st = out
    for b, p in enumerate(probs):
        g = graphs[clip_graph[b]]
        r32, r64 = gref.viterbi(p, g), gref.viterbi(p, g, dtype=np.float64)
        assert st[b] == (1 if r32 is None else 0), b
        if r32 is None:
            assert lp[b] == -np.inf and lens[b] == 0
            _rows_past_the_path_are_zero(out, b)
            continue
        if len(p) == 0:
            assert lp[b] == 0 and lens[b] == 0
            continue
        _, score = _valid(g, out, b, p)
        assert abs(float(lp[b]) - float(r32["path_logp"])) < 1e-3, (b, float(lp[b]), float(r32["path_logp"]))
        assert abs(score - float(r64["path_logp"])) < 1e-3, (b, score, float(r64["path_logp"]))
        if exact:
            np.testing.assert_array_equal(nodes[b, :lens[b]], r32["nodes"])
            np.testing.assert_array_equal(spans[b, :lens[b]], r32["spans"])
    return out


@pytest.mark.parametrize("shape", [s for s in edge.SHAPES if s[0] in (1, 15, 16, 17, 32, 33)], ids=edge.name)
def test_feeder_edges(native, shape):
    """The feeder's chunk boundaries and widths (tests/_ctc_edge_cases.py: two clips, the second shorter under the same T_out),
    each clip on a chain of its longest token row and on a ring of 7 nodes."""
    T, C, _ = shape
    probs, rows = edge.case(T, C)
    rng = np.random.default_rng(T * C)
    d = native.NativeDecoder(edge.labels(C), blank_index=0)
    graphs = [gref.chain(rows[0][0]), gref.chain(rows[1][0]), _ring(7, rng, C, fan=2)]
    _against_reference(d, graphs, probs + probs, [0, 1, 2, 2], T_out=T)
    d.close()


@pytest.mark.parametrize("N", [1, 255, 256, 257, 600])
def test_node_counts_either_side_of_the_thread_stride(dec, N):
    rng = np.random.default_rng(N)
    C = len(LABELS)
    g = _ring(N, rng, C, fan=2)
    _against_reference(dec, [g], [_peaky(rng, 48, C, sharp=3.0), _peaky(rng, 21, C, sharp=3.0)], [0, 0])


def test_graphs_at_the_limits(native, dec):
    rng = np.random.default_rng(2048)
    C = len(LABELS)
    nodes = _ring(native.GRAMMAR_MAX_NODES, rng, C, fan=1)
    arcs = _ring(native.GRAMMAR_MAX_NODES, rng, C, fan=4)
    assert len(nodes.labels) == native.GRAMMAR_MAX_NODES and len(nodes.arc_pred) == native.GRAMMAR_MAX_NODES
    assert len(arcs.arc_pred) == native.GRAMMAR_MAX_ARCS and len(arcs.labels) == native.GRAMMAR_MAX_NODES
    _against_reference(dec, [nodes, arcs], [_peaky(rng, 64, C, sharp=3.0), _peaky(rng, 64, C, sharp=3.0)], [0, 1])


def test_one_node_with_a_fan_in_of_300(dec):
    rng = np.random.default_rng(300)
    C = len(LABELS)
    labels = rng.integers(1, C, size=301)
    preds = [[] for _ in range(300)] + [[int(p) for p in rng.permutation(300)]]
    g = gref.graph(labels, [gref.START] * 300 + [gref.FINAL], preds, -rng.random(301).astype(np.float32))
    _against_reference(dec, [g], [_peaky(rng, 40, C, sharp=3.0), np.full((12, C), 1.0 / C, dtype=np.float32)], [0, 0])
    # without weights and on uniform probabilities everything ties: the first predecessor of the list wins
    g = gref.graph(labels, [gref.START] * 300 + [gref.FINAL], preds)
    _against_reference(dec, [g], [np.full((12, C), 1.0 / C, dtype=np.float32)], [0], exact=True)


def test_empty_graphs_and_clips_without_frames(dec):
    rng = np.random.default_rng(0)
    C = len(LABELS)
    yes, no = gref.graph([], [], [], None, True), gref.graph([], [], [], None, False)
    a = gref.chain([LABELS.index(c) for c in "ja"])
    opt = gref.graph(a.labels, a.flags, [[], [0]], None, True)
    probs = [_peaky(rng, 20, C), _peaky(rng, 20, C), np.zeros((0, C), np.float32), np.zeros((0, C), np.float32), np.zeros((0, C), np.float32),
             _peaky(rng, 1, C), _peaky(rng, 1, C)]
    graphs, clip_graph = [yes, no, a, opt], [0, 1, 0, 1, 2, 2, 3]
    out = _against_reference(dec, graphs, probs, clip_graph)
    lens, nodes, spans, tp, lp, st = out
    assert st.tolist() == [0, 1, 0, 1, 1, 1, 0] and not lens[:6].any()
    acc = np.float32(0)
    for v in aref.log_probs(probs[0])[:, 0]:
        acc = np.float32(acc + v)
    assert abs(float(lp[0]) - float(acc)) < 1e-4 and lp[2] == 0 and lp[3] == -np.inf


# ---- 5. a clip's result does not depend on its neighbours
def test_batch_equals_single_calls(dec, compiled):
    rng = np.random.default_rng(8)
    C = len(LABELS)
    graphs = [compiled["digits"], compiled["sentence"], _ring(300, rng, C, fan=3)]
    clip_graph = [2, 0, 1, 1, 0, 2, 0, 1]
    probs = [_peaky(rng, T, C, sharp=3.0) for T in (200, 9, 77, 160, 33, 120, 64, 16)]
    p_dev, sz = _padded(probs)
    batch = dec.grammar(p_dev, sz, graphs, clip_graph)
    assert batch[5].tolist() == [0] * 7 + [1]                 # (no sentence of the second grammar fits 16 frames)
    for b, p in enumerate(probs):
        p1, s1 = _padded([p])
        one = dec.grammar(p1, s1, graphs[clip_graph[b]])
        M = one[0][0]
        assert M == batch[0][b] and one[5][0] == batch[5][b] and one[4].tobytes() == batch[4][b:b + 1].tobytes()
        np.testing.assert_array_equal(one[1][0, :M], batch[1][b, :M])
        np.testing.assert_array_equal(one[2][0, :M], batch[2][b, :M])
        assert one[3][0, :M].tobytes() == batch[3][b, :M].tobytes()


# ---- 6. refusals
def test_refusals_write_nothing(native, dec):
    L = native.lib()
    B, T, C = 2, 10, len(LABELS)
    probs = torch.full((B, T, C), 1.0 / C, device="cuda")
    i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)
    ok = dict(B=B, T=T, K=2, sizes=[10, 8], clip_graph=[0, 1], node_off=[0, 3, 5], labels=[1, 2, 3, 4, 4], weights=[0, -1, 0, -0.5, 0],
              flags=[1, 0, 2, 1, 3], arc_off=[0, 0, 1, 3, 3, 5], arc_pred=[0, 1, 0, 0, 1], empty_ok=[0, 1])

    def call(**kw):
        a = dict(ok, **kw)
        arrays = {k: i32(a[k]) for k in ("sizes", "clip_graph", "node_off", "labels", "flags", "arc_off", "arc_pred", "empty_ok")}
        w = np.ascontiguousarray(a["weights"], dtype=np.float32)
        ptr = lambda x: x.ctypes.data
        pool = native.GrammarPool(a["K"], ptr(arrays["node_off"]), ptr(arrays["labels"]), ptr(w), ptr(arrays["flags"]), ptr(arrays["arc_off"]),
                                  ptr(arrays["arc_pred"]), ptr(arrays["empty_ok"]))
        lens, st = np.full(2, 7, dtype=np.int32), np.full(2, 7, dtype=np.int32)
        nodes, spans = np.full((2, 10), 7, dtype=np.int32), np.full((2, 10, 2), 7, dtype=np.int32)
        tp, lp = np.full((2, 10), 7.5, dtype=np.float32), np.full(2, 7.5, dtype=np.float32)
        rc = L.dsmi_grammar(dec._h, probs.data_ptr(), native._np_ptr(arrays["sizes"]), a["B"], a["T"], ctypes.byref(pool), native._np_ptr(arrays["clip_graph"]),
                            native._np_ptr(lens), native._np_ptr(nodes), native._np_ptr(spans), native._np_ptr(tp), native._np_ptr(lp), native._np_ptr(st), None)
        untouched = all((x == 7).all() for x in (lens, st, nodes, spans)) and (tp == 7.5).all() and (lp == 7.5).all()
        return rc, untouched, L.dsmi_decoder_last_error(dec._h).decode()

    rc, untouched, _ = call()
    assert rc == 0 and not untouched
    faults = [
        (dict(B=0), "must be positive"), (dict(T=0), "must be positive"), (dict(T=-3), "must be positive"), (dict(K=0), "must be positive"),
        (dict(sizes=[11, 8]), "size outside 0 .. T_out"), (dict(sizes=[10, -1]), "size outside 0 .. T_out"),
        (dict(clip_graph=[0, 2]), "graph outside 0 .. K-1"), (dict(clip_graph=[-1, 1]), "graph outside 0 .. K-1"),
        (dict(node_off=[1, 3, 5]), "node_off[0] must be 0"), (dict(node_off=[0, 3, 2]), "node offsets not ascending"),
        (dict(arc_off=[1, 1, 1, 3, 3, 5]), "arc_off[0] must be 0"), (dict(arc_off=[0, 0, 1, 3, 2, 5]), "arc offsets not ascending"),
        (dict(labels=[1, 0, 3, 4, 4]), "is the blank or not a label"), (dict(labels=[1, 2, 3, C, 4]), "is the blank or not a label"),
        (dict(labels=[1, 2, -2, 4, 4]), "is the blank or not a label"),
        (dict(arc_pred=[0, 1, 3, 0, 1]), "outside the graph"), (dict(arc_pred=[0, 1, 0, 0, 2]), "outside the graph"), (dict(arc_pred=[-1, 1, 0, 0, 1]), "outside the graph"),
        (dict(weights=[0, np.nan, 0, 0, 0]), "weight is not finite"), (dict(weights=[0, 0, 0, 0, -np.inf]), "weight is not finite"),
        (dict(flags=[0, 0, 2, 1, 3]), "no start node"), (dict(flags=[1, 0, 2, 1, 1]), "no final node"),
    ]
    for kw, text in faults:
        rc, untouched, msg = call(**kw)
        assert rc == native.DSMI_ERR_INVALID and untouched and msg.startswith("grammar: ") and text in msg, (kw, rc, msg)
    assert len({text for _, text in faults}) == 12           # each fault its own message
    # one node, one arc over the limits: from the call and from the plan
    N, A = native.GRAMMAR_MAX_NODES + 1, native.GRAMMAR_MAX_ARCS + 1
    big = dict(K=1, clip_graph=[0, 0], node_off=[0, N], labels=np.ones(N), weights=np.zeros(N), flags=np.full(N, 3), empty_ok=[0],
               arc_off=np.zeros(N + 1), arc_pred=[0])
    rc, untouched, msg = call(**big)
    assert rc == native.DSMI_ERR_CAPACITY and untouched and "DSMI_GRAMMAR_MAX_NODES" in msg and str(N) in msg
    off = np.minimum(np.arange(N) * 5, A)
    rc, untouched, msg = call(**dict(big, node_off=[0, N - 1], arc_off=off, arc_pred=np.zeros(A)))
    assert rc == native.DSMI_ERR_CAPACITY and untouched and "DSMI_GRAMMAR_MAX_ARCS" in msg and str(A) in msg
    for n, a in ((N, 0), (1, A)):
        with pytest.raises(native.DsmiError) as e:
            native.grammar_plan(2, 10, n, a)
        assert e.value.code == native.DSMI_ERR_CAPACITY
    rc, untouched, _ = call()
    assert rc == 0 and not untouched


# ---- 7., 8. through the model: a small synthetic TALKATIVE model (2 conv, 2 x BiGRU 256) whose greedy texts have several words
@pytest.fixture(scope="module")
def talkative():
    from danspeech_amd import Recognizer
    from danspeech_amd.deepspeech.model import DeepSpeech
    sd = syn.make_state_dict(2, "gru", 256, 2, seed=3, **syn.TALKATIVE)
    model = DeepSpeech("talkative", rnn_type="gru", rnn_hidden_size=256, rnn_layers=2, conv_layers=2).load_state_dict(sd)
    rec = Recognizer(model=model)
    clips = [syn.make_clip(i, n) for i, n in enumerate([48000, 80000, 32000, 64000])]
    return rec, clips


def test_the_greedy_text_is_the_best_sentence_of_a_grammar_that_holds_it(talkative):
    """The unconstrained argmax path is a path of its own collapse, so where the grammar accepts the greedy text it is the best
    sentence, on the greedy path: character starts are the greedy offsets, and path_logp is dsmi_align's of that text."""
    rec, clips = talkative
    eng = rec.danspeech_recognizer
    job = eng._enqueue_batch(clips)
    job.collect_forward()
    dec = eng.decoder._dec(eng._device_index())
    sizes = job.sizes.numpy().astype(np.int32)
    greedy = dec.greedy(job.probs, sizes)
    texts = [eng.decoder.normalise_transcript(eng.decoder._to_string(np.asarray(g[0]))) for g in greedy]
    assert all(texts) and len(set(texts)) == len(texts)
    assert texts == [eng.decoder._to_string(np.asarray(g[0])) for g in greedy]      # (as a grammar writes them: single spaces inside only)
    distractors = ["ja tak", "nej", texts[0] + " og", texts[1][:-1] or "a"]
    g = Grammar.from_sentences(texts + distractors, LABELS)
    decoded = eng.decoder.decode_grammar(job.probs, g, job.sizes)
    aligned = eng.decoder.align_ids(job.probs, [np.asarray(x[0]) for x in greedy], job.sizes)
    for b, (ids, off) in enumerate(greedy):
        text, chars, path_logp = decoded[b]
        assert text == texts[b]
        np.testing.assert_array_equal([a for _, a, _, _ in chars], off)
        assert np.float32(path_logp) == np.float32(aligned[b][2])
        np.testing.assert_array_equal([[a, e] for _, a, e, _ in chars], aligned[b][0])
    # the batch in the caller's order equals the single calls; the fourth field is Recognizer.score's
    batch = rec.recognize_grammar(clips, g)
    scores = rec.score_batch(clips, [[r[0]] for r in batch])
    for i, clip in enumerate(clips):
        assert batch[i] is not None and batch[i][0] == texts[tuple(job.order).index(i)]
        single = rec.align_flexible(clip, g)
        assert single[0] == batch[i][0] and [w for w, *_ in single[1]] == batch[i][0].split()
        assert [(w, round(a * 50), round(e * 50)) for w, a, e, _ in single[1]] == [(w, round(a * 50), round(e * 50)) for w, a, e, _ in batch[i][1]]
        # (a clip's probabilities alone and in the batch agree to float32 rounding through the network, not bit for bit)
        assert single[2] == pytest.approx(batch[i][2], rel=1e-4)
        assert batch[i][3] == scores[i][0][1]                    # dsmi_score's of the same batch
        assert batch[i][3] >= batch[i][2] - 1e-3                 # every alignment against the best one


def test_align_flexible_picks_the_spoken_variant(talkative):
    rec, clips = talkative
    clip = clips[3]                      # (its greedy text has three words)
    text = rec.recognize(clip)
    words = text.split()
    assert len(words) >= 3, text
    k = len(words) // 2
    wrong = words[k][::-1] + "q" if words[k][::-1] + "q" != words[k] else "x"
    flexible = " ".join(words[:k] + ["(%s | %s)" % (words[k], wrong)] + ["[øh]"] + words[k + 1:])
    got = rec.align_flexible(clip, flexible)
    assert got is not None and got[0] == text
    exact = rec.align(clip, text)
    assert [(w, round(a * 50), round(e * 50)) for w, a, e, _ in got[1]] == [(w, round(a * 50), round(e * 50)) for w, a, e, _ in exact]
    np.testing.assert_allclose([c for *_, c in got[1]], [c for *_, c in exact], rtol=1e-5)
    # a grammar that does not hold the greedy text still decodes, to one of its own sentences
    other = rec.align_flexible(clip, "(ja | nej) tak")
    assert other is not None and other[0] in ("ja tak", "nej tak") and other[2] < got[2]
