"""CTC forced alignment on the GPU (dsmi_align: csrc/ctc_tools.hip, the kernel csrc/align.hip) against the numpy reference of tests/_align_ref.py and a
brute-force enumeration of every path, its refusals, and the recogniser surface end to end on a synthetic cfgA-shaped model."""
import numpy as np
import pytest

from danspeech_amd import synthetic as syn

import _align_ref as ref
import _ctc_edge_cases as edge

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
LABELS = syn.DANSPEECH_LABELS


@pytest.fixture(scope="module")
def native():
    from danspeech_amd import _native
    return _native


def _padded(probs_list):
    T = max(len(p) for p in probs_list)
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


def test_brute_force_small_cases(native):
    dec = native.NativeDecoder(["_", "a", "b", "c", "d"], blank_index=0)
    rng = np.random.default_rng(5)
    probs, targets = [], []
    while len(probs) < 48:
        T = int(rng.integers(1, 8))
        t = [int(x) for x in rng.integers(1, 5, size=int(rng.integers(0, 4)))]
        if ref.min_frames(t) <= T:
            probs.append(rng.dirichlet(np.ones(5) * 0.5, size=T).astype(np.float32))
            targets.append(t)
    p_dev, sizes = _padded(probs)
    spans, tp, lp, status = dec.align(p_dev, sizes, targets)
    assert not status.any()
    for b, t in enumerate(targets):
        best, _ = ref.brute_force(probs[b], t)
        lab = ref.path_from_spans(spans[b, :len(t)], t, len(probs[b]))
        assert ref.collapse(lab) == t
        assert abs(float(lp[b]) - best) < 1e-5, (b, float(lp[b]), best)
        assert abs(ref.rescore64(probs[b], lab) - best) < 1e-5
    dec.close()


def _compare_with_reference(spans, tp, lp, status, probs, targets, exact):
    for b, t in enumerate(targets):
        r = ref.viterbi(probs[b], t)
        assert status[b] == 0
        assert abs(float(lp[b]) - float(r["path_logp"])) < 1e-3, (b, float(lp[b]), float(r["path_logp"]))
        lab = ref.path_from_spans(spans[b, :len(t)], t, len(probs[b]))
        assert ref.collapse(lab) == list(t)
        r64 = ref.viterbi(probs[b], t, dtype=np.float64)
        assert abs(ref.rescore64(probs[b], lab) - float(r64["path_logp"])) < 1e-3
        if exact:
            np.testing.assert_array_equal(spans[b, :len(t)], r["spans"])
            np.testing.assert_array_equal(tp[b, :len(t)], r["token_probs"])


@pytest.mark.parametrize("sharp, exact", [(3.0, False), (6.0, True)])
def test_reference_parity_ragged_batch(native, sharp, exact):
    dec = native.NativeDecoder(LABELS, blank_index=0)
    rng = np.random.default_rng(int(sharp))
    sizes = [501, 480, 377, 260, 501, 133, 64, 9]
    probs = [_peaky(rng, T, len(LABELS), sharp=sharp) for T in sizes]
    p_dev, sz = _padded(probs)
    greedy = [ids for ids, _ in dec.greedy(p_dev, sz)]
    for b, g in enumerate(greedy):
        assert ref.min_frames(g) <= sizes[b]
    randoms = []
    for T in sizes:
        L = int(rng.integers(0, T // 6 + 1))
        randoms.append([int(x) for x in rng.integers(1, len(LABELS), size=L)])
    # spans and token probabilities bit for bit where the margins are far above float32 rounding: the greedy transcripts of
    # sharpened probabilities; scores everywhere
    for targets, same in ((greedy, exact), (randoms, False)):
        spans, tp, lp, status = dec.align(p_dev, sz, targets)
        _compare_with_reference(spans, tp, lp, status, probs, targets, same)
    dec.close()


@pytest.mark.parametrize("shape", edge.SHAPES + edge.LONG, ids=edge.name)
def test_feeder_edges(native, shape):
    """The shared feeder's chunk boundaries, image wrap and widths (tests/_ctc_edge_cases.py), under the tolerances of
    _compare_with_reference.  No point is left out: the tests above have 33 labels only, and no batch of theirs pairs a clip of
    these frame counts with a shorter one under the same T_out."""
    T, C, L = shape
    probs, rows = edge.case(T, C, L)
    targets = [r[0] for r in rows]
    dec = native.NativeDecoder(edge.labels(C), blank_index=0)
    p_dev, sz = _padded(probs)
    assert p_dev.shape[1] == T and sz[1] < T
    spans, tp, lp, status = dec.align(p_dev, sz, targets)
    assert status.tolist() == [0, 0]
    _compare_with_reference(spans, tp, lp, status, probs, targets, False)
    dec.close()


def test_ties_follow_the_documented_rule(native):
    dec = native.NativeDecoder(LABELS, blank_index=0)
    C = len(LABELS)
    ids = [LABELS.index(c) for c in "alle"]
    cases = [(5, [1, 2]), (5, [1, 1]), (40, ids), (7, ids + ids[:1]), (6, []), (300, ids * 20), (5, ids)]
    probs = [np.full((T, C), 1.0 / C, dtype=np.float32) for T, _ in cases]
    targets = [t for _, t in cases]
    p_dev, sz = _padded(probs)
    spans, tp, lp, status = dec.align(p_dev, sz, targets)
    for b, t in enumerate(targets):
        r = ref.viterbi(probs[b], t)
        np.testing.assert_array_equal(spans[b, :len(t)], r["spans"])
        assert abs(float(lp[b]) - float(r["path_logp"])) < 1e-3
    assert spans[0, :2].tolist() == [[0, 1], [1, 2]]          # the hand-worked case: path 1, 3, 4, 4, 4
    assert spans[1, :2].tolist() == [[0, 1], [2, 3]]          # path 1, 2, 3, 4, 4
    dec.close()


def test_edge_cases_empty_and_infeasible(native):
    dec = native.NativeDecoder(LABELS, blank_index=0)
    rng = np.random.default_rng(9)
    alle = [LABELS.index(c) for c in "alle"]
    probs = [_peaky(rng, T, len(LABELS)) for T in (50, 4, 30, 20, 5)]
    targets = [alle, alle, [], alle * 2, alle]                 # clip 1: 4 frames < 5 needed; clip 4: exactly 5
    p_dev, sz = _padded(probs)
    spans, tp, lp, status = dec.align(p_dev, sz, targets)
    assert status.tolist() == [0, 1, 0, 0, 0]
    assert lp[1] == -np.inf and not spans[1].any() and not tp[1].any()
    lpb = ref.log_probs(probs[2])[:, 0]
    acc = np.float32(0)
    for v in lpb:
        acc = np.float32(acc + v)
    assert abs(float(lp[2]) - float(acc)) < 1e-4
    # every neighbour as if aligned alone
    for b in (0, 2, 3, 4):
        p1, s1 = _padded([probs[b]])
        sp1, tp1, lp1, st1 = dec.align(p1, s1, [targets[b]])
        L = len(targets[b])
        assert st1[0] == 0 and lp1[0] == lp[b]
        np.testing.assert_array_equal(sp1[0, :L], spans[b, :L])
        np.testing.assert_array_equal(tp1[0, :L], tp[b, :L])
    assert spans[4, :4].tolist() == [[0, 1], [1, 2], [3, 4], [4, 5]]
    dec.close()


def test_longest_transcript(native):
    """DSMI_ALIGN_MAX_TOKENS tokens: the largest LDS carve."""
    dec = native.NativeDecoder(LABELS, blank_index=0)
    rng = np.random.default_rng(13)
    t = [int(x) for x in rng.integers(1, len(LABELS), size=native.ALIGN_MAX_TOKENS)]
    T = ref.min_frames(t) + 200
    probs = [_peaky(rng, T, len(LABELS), sharp=2.0)]
    p_dev, sz = _padded(probs)
    spans, tp, lp, status = dec.align(p_dev, sz, [t])
    assert status[0] == 0
    lab = ref.path_from_spans(spans[0], t, T)
    assert ref.collapse(lab) == t
    r = ref.viterbi(probs[0], t)
    assert abs(float(lp[0]) - float(r["path_logp"])) <= 1e-5 * abs(float(r["path_logp"]))
    assert abs(ref.rescore64(probs[0], lab) - float(lp[0])) <= 1e-5 * abs(float(lp[0]))
    dec.close()


def test_refusals_write_nothing(native):
    dec = native.NativeDecoder(LABELS, blank_index=0)
    L = native.lib()
    B, T, Ls = 2, 10, 3
    probs = torch.full((B, T, len(LABELS)), 1.0 / len(LABELS), device="cuda")
    ok_sizes = np.array([10, 8], dtype=np.int32)
    ok_tg = np.array([[1, 2, 3], [4, 5, 0]], dtype=np.int32)
    ok_lens = np.array([3, 2], dtype=np.int32)

    def call(B=B, T=T, sizes=ok_sizes, tg=ok_tg, lens=ok_lens, Ls=Ls):
        spans = np.full((2, max(Ls, 1), 2), 7, dtype=np.int32)
        tp = np.full((2, max(Ls, 1)), 7.5, dtype=np.float32)
        lp = np.full(2, 7.5, dtype=np.float32)
        st = np.full(2, 7, dtype=np.int32)
        tgc = np.ascontiguousarray(tg, dtype=np.int32)
        rc = L.dsmi_align(dec._h, probs.data_ptr(), native._np_ptr(np.ascontiguousarray(sizes, dtype=np.int32)), B, T,
                          native._np_ptr(tgc), native._np_ptr(np.ascontiguousarray(lens, dtype=np.int32)), Ls,
                          native._np_ptr(spans), native._np_ptr(tp), native._np_ptr(lp), native._np_ptr(st), None)
        untouched = (spans == 7).all() and (tp == 7.5).all() and (lp == 7.5).all() and (st == 7).all()
        return rc, untouched, L.dsmi_decoder_last_error(dec._h).decode()

    rc, _, _ = call()
    assert rc == 0
    big = np.zeros((2, native.ALIGN_MAX_TOKENS + 1), dtype=np.int32)
    for kw in (dict(B=0), dict(T=0), dict(T=-3), dict(sizes=[11, 8]), dict(sizes=[-1, 8]), dict(lens=[-1, 2]), dict(lens=[4, 2]),
               dict(tg=[[1, 0, 3], [4, 5, 0]]), dict(tg=[[1, 2, 3], [4, len(LABELS), 0]]), dict(tg=[[1, 2, -2], [4, 5, 0]]),
               dict(tg=big, Ls=native.ALIGN_MAX_TOKENS + 1)):
        rc, untouched, msg = call(**kw)
        assert rc < 0 and untouched and msg, (kw, rc, msg)
    rc, _, _ = call()
    assert rc == 0
    dec.close()


# ---- end to end: a synthetic cfgA-shaped model (2 conv, 5 x BiGRU 800) with sharpened FC weights
@pytest.fixture(scope="module")
def cfga():
    from danspeech_amd import Recognizer
    from danspeech_amd.deepspeech.model import DeepSpeech
    sd = syn.make_state_dict(2, "gru", 800, 5, seed=0, fc_gain=8.0)
    model = DeepSpeech("cfgA", rnn_type="gru", rnn_hidden_size=800, rnn_layers=5, conv_layers=2).load_state_dict(sd)
    rec = Recognizer(model=model)
    clips = [syn.make_clip(i, n) for i, n in enumerate([48000, 160000, 32000, 96000, 71234])]
    return rec, clips


def test_greedy_transcript_aligns_to_the_greedy_offsets(native, cfga):
    """The unconstrained argmax path is a path of its own collapse, so it is the constrained optimum too: every token's
    start is the greedy offset of that token."""
    rec, clips = cfga
    eng = rec.danspeech_recognizer
    job = eng._enqueue_batch(clips)
    job.collect_forward()
    dec = eng.decoder._dec(eng._device_index())
    sizes = job.sizes.numpy().astype(np.int32)
    greedy = dec.greedy(job.probs, sizes)
    ids = [g[0] for g in greedy]
    assert all(len(g) for g in ids)
    spans, tp, lp, status = dec.align(job.probs, sizes, ids)
    assert not status.any()
    for b, (g, off) in enumerate(greedy):
        np.testing.assert_array_equal(spans[b, :len(g), 0], off)
    res = eng.decoder.align_ids(job.probs, ids, job.sizes)
    for b, (g, off) in enumerate(greedy):
        np.testing.assert_array_equal(res[b][0][:, 0], off)


def test_align_batch_equals_single_align_in_callers_order(cfga):
    rec, clips = cfga
    texts = rec.recognize_batch(clips)
    batch = rec.align_batch(clips, texts)
    frame_s = rec.danspeech_recognizer.frame_seconds()
    assert frame_s == pytest.approx(0.02)
    for clip, text, words in zip(clips, texts, batch):
        assert words is not None
        assert [w for w, _, _, _ in words] == text.split()
        single = rec.align(clip, text)
        assert [(w, round(a / frame_s), round(e / frame_s)) for w, a, e, _ in single] == \
               [(w, round(a / frame_s), round(e / frame_s)) for w, a, e, _ in words]
        np.testing.assert_allclose([c for *_, c in single], [c for *_, c in words], rtol=1e-5)
        for w, a, e, c in words:
            assert 0 <= a < e <= (len(clip) / 320 + 1) * frame_s and 0 < c <= 1      # (output frames: samples / 160 / 2)
    # an impossible transcript: far more letters than frames
    out = rec.align_batch(clips[:2], [texts[0], "a" * 3000])
    assert out[1] is None and out[0] is not None
