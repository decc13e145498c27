"""The CTC grammar posterior on the GPU (dsmi_grammar_posterior: csrc/ctc_tools.hip, the kernels csrc/grammar_post.hip) against a
brute force over every frame labelling, against closed forms on a graph that accepts everything, against dsmi_score and
dsmi_occupancy on chain graphs, against the float64 numpy reference of tests/_grammar_post_ref.py on compiled and hand-built
graphs, its invariances and refusals, and the recogniser surface end to end on a synthetic model.

The tolerance against the reference is twice the contract's bound (tests/_grammar_post_ref.py: bound, bound_logp; T * bound for
visits), since each side is within the bound of the recurrences evaluated exactly."""
import ctypes

import numpy as np
import pytest

from danspeech_amd import synthetic as syn
from danspeech_amd.grammar import Grammar

import _align_ref as aref
import _ctc_edge_cases as edge
import _grammar_post_ref as pref
import _grammar_ref as gref
import _occ_ref as oref
import _score_ref as sref
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


def _padded(probs_list, T=None, fill=None):
    T = T or max(1, max(len(p) for p in probs_list))
    C = probs_list[0].shape[1]
    x = np.full((len(probs_list), T, C), 1.0 / C if fill is None else fill, dtype=np.float32)
    for b, p in enumerate(probs_list):
        x[b, :len(p)] = p
    return torch.from_numpy(x).cuda(), np.array([len(p) for p in probs_list], dtype=np.int32)


def _against_reference(out, b, g, probs, ref, what):
    """Clip b of a call against the reference's dict, within twice the bound; what lies past the clip and the graph is zero."""
    logp, visits, occ, status = out
    T, N, F = len(probs), len(g.labels), pref.fan_in(g)
    assert status[b] == ref["status"], what
    row = occ[b].cpu().numpy()
    assert not row[T:].any() and not visits[b, N:].any(), what
    if ref["status"]:
        assert logp[b] == -np.inf and not row.any() and not visits[b].any(), what
        return
    bound = pref.bound(T, F, ref["logp"])
    e_logp, e_occ = abs(logp[b] - float(ref["logp"])), np.abs(row[:T] - ref["occ"]).max() if T else 0.0
    e_vis = np.abs(visits[b, :N] - ref["visits"]).max() if N else 0.0
    print(what, "logp err %.3g (2 x %.3g)  occ err %.3g (2 x %.3g)  visits err %.3g (2 x %.3g)"
          % (e_logp, pref.bound_logp(T, F, ref["logp"]), e_occ, bound, e_vis, T * bound))
    assert e_logp <= 2 * pref.bound_logp(T, F, ref["logp"]), what
    assert e_occ <= 2 * bound, what
    assert e_vis <= 2 * T * bound, what
    if T:
        assert np.abs(row[:T].sum(1) - 1).max() <= 2 * bound + len(LABELS) * 2.0 ** -52, what


# ---- 1. brute force: the 48 cases of test_gpu_grammar.py::test_brute_force_small_cases
def test_brute_force_small_cases(native):
    d = native.NativeDecoder(["_", "a", "b", "c"], blank_index=0)
    rng = np.random.default_rng(21)
    graphs, probs = [], []
    for case in range(48):
        T = int(rng.integers(1, 7))
        graphs.append(random_graph(rng, 4))
        probs.append(np.full((T, 4), 0.25, dtype=np.float32) if case % 6 == 0 else rng.dirichlet(np.ones(4) * 0.5, size=T).astype(np.float32))
    p_dev, sizes = _padded(probs)
    logp, visits, occ, st = d.grammar_posterior(p_dev, sizes, graphs, np.arange(48))
    occ = occ.cpu().numpy()
    decoded = 0
    for b, g in enumerate(graphs):
        want = pref.brute_force_sum(probs[b], g)
        assert st[b] == (1 if want is None else 0), b
        if want is None:
            assert logp[b] == -np.inf and not occ[b].any() and not visits[b].any()
            continue
        decoded += 1
        T = len(probs[b])
        # (the brute force sums up to 4^6 terms in float64: 4096 * 2^-53 relative, beside the bound)
        assert abs(logp[b] - want) <= 2 * pref.bound_logp(T, pref.fan_in(g), want) + 4096 * 2.0 ** -53, (b, logp[b], want)
        assert not occ[b, T:].any() and not visits[b, len(g.labels):].any()
    assert 20 <= decoded < 48            # both outcomes are there
    d.close()


# ---- 2. a graph that accepts everything: no reference at all
def test_everything_is_accepted(dec):
    C = len(LABELS)
    N = C - 1
    g = gref.graph(np.arange(1, C), np.full(N, gref.START | gref.FINAL), [list(range(N))] * N, None, True)
    rng = np.random.default_rng(40)
    raw = rng.dirichlet(np.full(C, 0.3), size=40)
    probs = np.maximum(raw * rng.uniform(0.5, 1.0, size=(40, 1)), 1e-30).astype(np.float32)      # rows that do not sum to 1
    p_dev, sz = _padded([probs])
    logp, visits, occ, st = dec.grammar_posterior(p_dev, sz, g)
    rowsum = probs.astype(np.float64).sum(1)
    want = float(np.log(rowsum).sum())
    bound = pref.bound(40, N, want)
    assert st[0] == 0 and abs(logp[0] - want) <= pref.bound_logp(40, N, want) + 40 * C * 2.0 ** -52
    got = occ[0].cpu().numpy()
    assert np.abs(got - probs.astype(np.float64) / rowsum[:, None]).max() <= bound + C * 2.0 ** -52


# ---- 3. a chain graph is dsmi_score and dsmi_occupancy
def test_chain_graphs_equal_score_and_occupancy(native):
    C = 33
    d = native.NativeDecoder(edge.labels(C), blank_index=0)
    probs, targets = [], []
    for shape in [(T, C, None) for T in edge.FRAMES]:
        ps, rows = edge.case(*shape)
        for p, rws in zip(ps, rows):
            for r in rws:
                probs.append(p)
                targets.append(list(r))
    rng = np.random.default_rng(9)
    uni = lambda T: np.full((T, C), 1.0 / C, dtype=np.float32)
    for T, tg in [(5, [1, 1]), (3, [1, 1]), (2, [1, 1]), (9, [2, 2, 2, 3]), (0, []), (0, [4]), (6, []), (4, [1, 2, 3, 4, 5]), (48, [7] * 24), (47, [7] * 24)]:
        probs.append(uni(T) if T % 2 else sref.peaky(rng, T, C) if T else np.zeros((0, C), np.float32))
        targets.append(tg)
    p_dev, sz = _padded(probs)
    B = len(probs)
    graphs = [gref.chain(t) for t in targets]
    logp, visits, occ, st = d.grammar_posterior(p_dev, sz, graphs, np.arange(B))
    s_logp, s_occ, _, s_st = d.occupancy(p_dev, sz, np.arange(B), targets, want_tok=False)
    q_logp, q_st = d.score(p_dev, sz, np.arange(B), targets)
    np.testing.assert_array_equal(st, s_st)
    np.testing.assert_array_equal(st, q_st)
    assert st.any() and not st.all()
    occ, s_occ = occ.cpu().numpy(), s_occ.cpu().numpy()
    for b, t in enumerate(targets):
        T, L = len(probs[b]), len(t)
        if st[b]:
            assert logp[b] == -np.inf and not occ[b].any() and not visits[b].any()
            continue
        assert abs(logp[b] - q_logp[b]) <= sref.bound(T, q_logp[b]) + pref.bound_logp(T, 1, logp[b]), (b, logp[b], q_logp[b])
        assert abs(logp[b] - s_logp[b]) <= sref.bound(T, s_logp[b]) + pref.bound_logp(T, 1, logp[b])
        assert np.abs(occ[b] - s_occ[b]).max() <= oref.bound(T, s_logp[b]) + pref.bound(T, 1, logp[b]), b
        assert (np.abs(visits[b, :L] - 1).max() <= T * pref.bound(T, 1, logp[b])) if L else True, (b, visits[b, :L])
        assert not visits[b, L:].any()
    d.close()


# ---- 4., 5. compiled grammars and hand-built graphs against the reference; paths, not sentences
@pytest.fixture(scope="module")
def reference():
    """The shared inputs with their float64 reference, computed once: [(name, graph, probs, reference dict)]."""
    return [(name, g, probs, pref.posterior(probs, g)) for name, g, probs in pref.reference_cases(LABELS)]


def test_graphs_against_the_reference(dec, reference):
    assert any(len(g.labels) > 256 and len(g.labels) % 4 for _, g, _, _ in reference) and max(pref.fan_in(g) for _, g, _, _ in reference) == 40
    p_dev, sz = _padded([p for _, _, p, _ in reference])
    out = dec.grammar_posterior(p_dev, sz, [g for _, g, _, _ in reference], np.arange(len(reference)))
    for b, (name, g, probs, ref) in enumerate(reference):
        assert ref["status"] == 0
        _against_reference(out, b, g, probs, ref, name)
    # the weight of -80 is an entry of about e^-80 into its node, not 0 and not lost
    name, g, probs, ref = reference[-1]
    n = int(np.argmin(g.weights))
    assert g.weights[n] == -80 and 0 < out[1][len(reference) - 1, n] < 1e-30


def test_paths_not_sentences(dec):
    cases = pref.path_cases(len(LABELS))
    p_dev, sz = _padded([c[4] for c in cases] * 2)
    graphs = [c[1] for c in cases] + [c[2] for c in cases]
    out = dec.grammar_posterior(p_dev, sz, graphs, np.arange(len(graphs)))
    for b, (name, g, chain, factor, probs) in enumerate(cases):
        ref = pref.posterior(probs, g)
        _against_reference(out, b, g, probs, ref, name)
        T = len(probs)
        assert abs(out[0][b] - (out[0][len(cases) + b] + np.log(factor))) <= 2 * pref.bound_logp(T, pref.fan_in(g), out[0][b]), name


# ---- 6. invariance
def test_a_clip_does_not_depend_on_its_neighbours_or_on_rows_past_its_frames(dec, reference):
    rng = np.random.default_rng(8)
    C = len(LABELS)
    graphs = [g for _, g, _, _ in reference]
    clip_graph = [3, 0, 1, 4, 2, 3, 0]
    probs = [pref.dirichlet(rng, T, C) for T in (60, 33, 9, 21, 40, 16, 0)]
    p_dev, sz = _padded(probs)
    batch = dec.grammar_posterior(p_dev, sz, graphs, clip_graph)
    again = dec.grammar_posterior(p_dev, sz, graphs, clip_graph)
    p_nan, _ = _padded(probs, fill=np.nan)
    nan = dec.grammar_posterior(p_nan, sz, graphs, clip_graph)
    for other in (again, nan):
        assert batch[0].tobytes() == other[0].tobytes() and batch[1].tobytes() == other[1].tobytes() and torch.equal(batch[2], other[2])
        np.testing.assert_array_equal(batch[3], other[3])
    assert batch[3].tolist().count(0) >= 4 and batch[3][-1] == 1
    for b, p in enumerate(probs):
        g = graphs[clip_graph[b]]
        p1, s1 = _padded([p])
        one = dec.grammar_posterior(p1, s1, g)
        T, N = len(p), len(g.labels)
        assert one[3][0] == batch[3][b] and one[0].tobytes() == batch[0][b:b + 1].tobytes()
        assert one[1][0, :N].tobytes() == batch[1][b, :N].tobytes()
        assert torch.equal(one[2][0, :T], batch[2][b, :T]) and not batch[2][b, T:].any()
        if not batch[3][b]:
            rows = batch[2][b, :T].sum(1).cpu().numpy()
            assert np.abs(rows - 1).max() <= 2 * pref.bound(T, pref.fan_in(g), batch[0][b]) + C * 2.0 ** -52


# ---- 7. refusals
def test_refusals_write_nothing(native, dec):
    L = native.lib()
    B, T, C = 2, 10, len(LABELS)
    probs = torch.full((B, T, C), 1.0 / C, device="cuda")
    i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)
    ok = dict(B=B, T=T, K=2, sizes=[10, 8], clip_graph=[0, 1], node_off=[0, 3, 5], labels=[1, 2, 3, 4, 4], weights=[0, -1, 0, -0.5, 0],
              flags=[1, 0, 2, 1, 3], arc_off=[0, 0, 1, 3, 3, 5], arc_pred=[0, 1, 0, 0, 1], empty_ok=[0, 1], N_stride=3, logp=True, status=True,
              probs=probs)

    def call(**kw):
        a = dict(ok, **kw)
        arrays = {k: i32(a[k]) for k in ("sizes", "clip_graph", "node_off", "labels", "flags", "arc_off", "arc_pred", "empty_ok")}
        w = np.ascontiguousarray(a["weights"], dtype=np.float32)
        ptr = lambda x: x.ctypes.data
        pool = native.GrammarPool(a["K"], ptr(arrays["node_off"]), ptr(arrays["labels"]), ptr(w), ptr(arrays["flags"]), ptr(arrays["arc_off"]),
                                  ptr(arrays["arc_pred"]), ptr(arrays["empty_ok"]))
        lp, vis, st = np.full(2, 7.5), np.full((2, 3), 7.5), np.full(2, 7, dtype=np.int32)
        occ = torch.full((2, 10, C), 7.5, dtype=torch.float64, device="cuda")
        rc = L.dsmi_grammar_posterior(dec._h, a["probs"].data_ptr(), native._np_ptr(arrays["sizes"]), a["B"], a["T"], ctypes.byref(pool),
                                      native._np_ptr(arrays["clip_graph"]), a["N_stride"], native._np_ptr(lp) if a["logp"] else None, native._np_ptr(vis),
                                      occ.data_ptr(), native._np_ptr(st) if a["status"] else None, None)
        untouched = (st == 7).all() and (lp == 7.5).all() and (vis == 7.5).all() and bool((occ == 7.5).all())
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
        assert rc == native.DSMI_ERR_INVALID and untouched and msg.startswith("grammar") and text in msg, (kw, rc, msg)
    assert len({text for _, text in faults}) == 12           # each fault its own message
    for kw in (dict(logp=False), dict(status=False)):
        rc, untouched, msg = call(**kw)
        assert rc == native.DSMI_ERR_INVALID and untouched and "bad grammar posterior arguments" in msg
    rc, untouched, msg = call(N_stride=2)
    assert rc == native.DSMI_ERR_INVALID and untouched and "N_stride 2 is below the pool's largest graph (3 nodes)" in msg
    # the cap, reached by the numbers alone: nothing is read, so nothing needs to be there
    rc, untouched, msg = call(B=1 << 12, T=1 << 12)
    assert rc == native.DSMI_ERR_CAPACITY and untouched and "exceed 2^30" in msg and "stored trellises" in msg
    # one node, one arc over the limits
    N, A = native.GRAMMAR_MAX_NODES + 1, native.GRAMMAR_MAX_ARCS + 1
    big = dict(K=1, clip_graph=[0, 0], node_off=[0, N], labels=np.ones(N), weights=np.zeros(N), flags=np.full(N, 3), empty_ok=[0],
               arc_off=np.zeros(N + 1), arc_pred=[0])
    rc, untouched, msg = call(**big)
    assert rc == native.DSMI_ERR_CAPACITY and untouched and "DSMI_GRAMMAR_MAX_NODES" in msg and str(N) in msg
    off = np.minimum(np.arange(N) * 5, A)
    rc, untouched, msg = call(**dict(big, node_off=[0, N - 1], arc_off=off, arc_pred=np.zeros(A)))
    assert rc == native.DSMI_ERR_CAPACITY and untouched and "DSMI_GRAMMAR_MAX_ARCS" in msg and str(A) in msg
    rc, untouched, _ = call()
    assert rc == 0 and not untouched


# ---- 8. the surface, on a small synthetic model (2 conv, 2 x BiGRU 256)
def test_grammar_confidence_on_the_synthetic_model():
    from danspeech_amd import Recognizer
    from danspeech_amd.deepspeech.model import DeepSpeech
    sd = syn.make_state_dict(2, "gru", 256, 2, seed=3, **syn.TALKATIVE)
    model = DeepSpeech("talkative", rnn_type="gru", rnn_hidden_size=256, rnn_layers=2, conv_layers=2).load_state_dict(sd)
    rec = Recognizer(model=model)
    clips = [syn.make_clip(i, n) for i, n in enumerate([48000, 32000, 40000])]
    sentences = ["ja tak", "nej", rec.recognize(clips[0]), "sluk lyset"]
    assert len(set(sentences)) == 4 and all(sentences)
    g = Grammar.from_sentences(sentences, LABELS)
    got = rec.grammar_confidence_batch(clips, g)
    best = rec.recognize_grammar(clips, g)
    eng = rec.danspeech_recognizer
    job = eng._enqueue_batch(clips)
    job.collect_forward()
    full = eng.decoder.grammar_posterior(job.probs, g, job.sizes, candidates=sentences)
    for i, clip in enumerate(clips):
        pos = tuple(job.order).index(i)
        r, f = got[i], full[pos]
        assert r is not None and f is not None and set(r) == {"text", "chars", "path_logp", "grammar_logp", "sentence_posterior"}
        assert r["text"] == best[i][0] and r["path_logp"] == pytest.approx(best[i][2], rel=1e-4)
        T = int(job.sizes[pos])
        bound = pref.bound(T, pref.fan_in(g), f["logp"])
        # four sentences, each exp(three values within the bound): the unambiguous grammar's posteriors sum to 1
        assert abs(f["posteriors"].sum() - 1) <= 4 * 3 * bound
        assert r["grammar_logp"] == pytest.approx(f["logp"], rel=1e-4) and r["grammar_logp"] <= 0
        assert r["sentence_posterior"] == pytest.approx(f["posteriors"][sentences.index(r["text"])], rel=1e-3, abs=1e-6)
        assert f["occ"].shape == (job.probs.shape[1], len(LABELS)) and f["visits"].shape == (g.n_nodes,)
        single = rec.grammar_confidence(clip, g)
        assert single["text"] == r["text"]
