"""CTC phrase search on the GPU (dsmi_spot, csrc/spot.hip) against the numpy reference of tests/_spot_ref.py and a brute force
over every window and labelling, the packing of phrases into workgroups, ties, planted occurrences, its refusals, and the
recogniser surface end to end on a synthetic cfgA-shaped model."""
import numpy as np
import pytest

from danspeech_amd import synthetic as syn

import _align_ref as aref
import _ctc_edge_cases as edge
import _spot_ref as ref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
LABELS = syn.DANSPEECH_LABELS
ALLE = [LABELS.index(c) for c in "alle"]


@pytest.fixture(scope="module")
def native():
    from danspeech_amd import _native
    return _native


def _padded(probs_list, T=None):
    T = T or max(1, max(len(p) for p in probs_list))
    C = probs_list[0].shape[1]
    x = np.full((len(probs_list), T, C), 1.0 / C, dtype=np.float32)
    for b, p in enumerate(probs_list):
        x[b, :len(p)] = p
    return torch.from_numpy(x).cuda(), np.array([len(p) for p in probs_list], dtype=np.int32)


def _hits(hits, scores, counts, b, k):
    return [(int(hits[b, k, n, 0]), int(hits[b, k, n, 1]), scores[b, k, n]) for n in range(counts[b, k])]


def _check_rows_past_the_count(hits, scores, counts):
    for b in range(counts.shape[0]):
        for k in range(counts.shape[1]):
            assert not hits[b, k, counts[b, k]:].any() and not scores[b, k, counts[b, k]:].any()


def _check_picking(hits, scores, counts, E, ST, sizes, max_hits, floor):
    """The hits are exactly the documented picking applied to the kernel's own tracks."""
    for b in range(E.shape[0]):
        for k in range(E.shape[1]):
            want = ref.pick(E[b, k, :sizes[b]], ST[b, k, :sizes[b]], max_hits, floor)
            got = _hits(hits, scores, counts, b, k)
            assert [(s, e) for s, e, _ in got] == [(s, e) for s, e, _ in want], (b, k)
            assert [v for *_, v in got] == [v for *_, v in want], (b, k)
            assert (E[b, k, sizes[b]:] == -np.inf).all() and (ST[b, k, sizes[b]:] == -1).all()
    _check_rows_past_the_count(hits, scores, counts)


def test_brute_force_small_cases(native):
    dec = native.NativeDecoder(["_", "a", "b", "c", "d"], blank_index=0)
    rng = np.random.default_rng(5)
    probs = [rng.dirichlet(np.ones(5) * 0.5, size=int(rng.integers(1, 7))).astype(np.float32) for _ in range(48)]
    phrases = [[1], [2, 2], [1, 2], [3, 1, 3], [4, 4, 1], [2, 3, 4], [3]]
    p_dev, sizes = _padded(probs)
    hits, scores, counts, E, ST = dec.spot(p_dev, sizes, phrases, 3, -np.inf, tracks=True)
    n = 0
    for b, p in enumerate(probs):
        W = ref.brute_force(p, phrases)
        for k in range(len(phrases)):
            for f in range(len(p)):
                best = W[k][:, f].max()
                if best == -np.inf:
                    assert E[b, k, f] == -np.inf and ST[b, k, f] == -1
                    continue
                assert abs(float(E[b, k, f]) - best) < 1e-5, (b, k, f, float(E[b, k, f]), best)
                assert 0 <= ST[b, k, f] <= f and abs(W[k][ST[b, k, f], f] - best) < 1e-5
                n += 1
    assert n > 500
    _check_picking(hits, scores, counts, E, ST, sizes, 3, -np.inf)
    dec.close()


RAGGED = [501, 377, 133, 64, 33, 32, 31, 17, 16, 15, 9, 0]      # straddle the edges of the 16-frame chunks


@pytest.mark.parametrize("sharp", [3.0, 6.0])
def test_reference_parity_ragged_batch(native, sharp):
    dec = native.NativeDecoder(LABELS, blank_index=0)
    rng = np.random.default_rng(int(sharp))
    C = len(LABELS)
    probs = [ref.peaky(rng, T, C, sharp) for T in RAGGED]
    phrases = [[int(x) for x in rng.integers(1, C, size=L)] for L in (1, 2, 5, 12, 128)] + [ALLE]
    p_dev, sizes = _padded(probs)
    hits, scores, counts, E, ST = dec.spot(p_dev, sizes, phrases, 5, -np.inf, tracks=True)
    finite = exempt = 0
    worst = 0.0
    for b, p in enumerate(probs):
        for k, ph in enumerate(phrases):
            T = len(p)
            E32, S32 = ref.tracks(p, ph)
            ok = E32 > -np.inf
            assert ((E[b, k, :T] > -np.inf) == ok).all(), (b, k)
            finite += int(ok.sum())
            if ok.any():
                worst = max(worst, float(np.abs(E[b, k, :T][ok] - E32[ok]).max()))
            differ = np.nonzero(ST[b, k, :T] != S32)[0]
            if len(differ):
                E64, S64, MG = ref.tracks(p, ph, dtype=np.float64, margins=True)
                for f in differ:
                    # a near tie in float64 somewhere on the path, and the reported window is as good as the best
                    assert ok[f] and MG[f] < 1e-4, (b, k, f, MG[f])
                    r = aref.viterbi(p[ST[b, k, f]:f + 1], ph, dtype=np.float64)
                    assert r is not None and abs(float(r["path_logp"]) - E64[f]) < 1e-3, (b, k, f)
                    exempt += 1
    print("finite frames %d, exempt %d, max |E - E32| %.3g" % (finite, exempt, worst))
    assert worst < 1e-3
    assert finite > 4000 and exempt <= 0.01 * finite
    assert not counts[-1].any() and (E[-1] == -np.inf).all()              # the clip without frames
    assert counts[0, 4] >= 1 and not counts[3:, 4].any()                  # 128 tokens need at least 128 frames
    _check_picking(hits, scores, counts, E, ST, sizes, 5, -np.inf)
    floor = float(np.log(0.05))
    h2, s2, c2, E2, ST2 = dec.spot(p_dev, sizes, phrases, native.SPOT_MAX_HITS, floor, tracks=True)
    assert np.array_equal(E2, E) and np.array_equal(ST2, ST)
    _check_picking(h2, s2, c2, E, ST, sizes, native.SPOT_MAX_HITS, floor)
    assert c2.max() > 5
    # without the tracks: the same hits
    h3, s3, c3 = dec.spot(p_dev, sizes, phrases, 5, -np.inf)
    assert np.array_equal(h3, hits) and np.array_equal(s3, scores) and np.array_equal(c3, counts)
    dec.close()


@pytest.mark.parametrize("shape", edge.SHAPES, ids=edge.name)
def test_feeder_edges(native, shape):
    """The shared feeder's chunk boundaries, image wrap and widths (tests/_ctc_edge_cases.py), held as
    test_reference_parity_ragged_batch holds its clips: the same frames finite, scores within 1e-3 of the float32 reference, a
    start that differs only behind a float64 near tie, and the hits the documented picking of the kernel's own tracks.  No point
    is left out: RAGGED has these frame counts at 33 labels, each under a T_out of 501, never 3 or 128 labels."""
    T, C, _ = shape
    probs, _ = edge.case(T, C)
    phrases = edge.phrases(T, C)
    assert all(aref.min_frames(ph) <= T for ph in phrases)
    dec = native.NativeDecoder(edge.labels(C), blank_index=0)
    p_dev, sizes = _padded(probs)
    assert p_dev.shape[1] == T and sizes[1] < T
    hits, scores, counts, E, ST = dec.spot(p_dev, sizes, phrases, 5, -np.inf, tracks=True)
    assert counts[0].all()                                            # every phrase fits the first clip
    for b, p in enumerate(probs):
        for k, ph in enumerate(phrases):
            n = len(p)
            E32, S32 = ref.tracks(p, ph)
            ok = E32 > -np.inf
            assert ((E[b, k, :n] > -np.inf) == ok).all(), (b, k)
            assert not ok.any() or float(np.abs(E[b, k, :n][ok] - E32[ok]).max()) < 1e-3, (b, k)
            differ = np.nonzero(ST[b, k, :n] != S32)[0]
            if len(differ):
                E64, S64, MG = ref.tracks(p, ph, dtype=np.float64, margins=True)
                for f in differ:
                    assert ok[f] and MG[f] < 1e-4, (b, k, f, MG[f])
                    r = aref.viterbi(p[ST[b, k, f]:f + 1], ph, dtype=np.float64)
                    assert r is not None and abs(float(r["path_logp"]) - E64[f]) < 1e-3, (b, k, f)
    _check_picking(hits, scores, counts, E, ST, sizes, 5, -np.inf)
    dec.close()


def test_packed_phrases_equal_the_phrase_alone(native):
    """255 + 1 states fill group 0 exactly and more phrases follow: no phrase sees its neighbours' states."""
    dec = native.NativeDecoder(LABELS, blank_index=0)
    rng = np.random.default_rng(21)
    C = len(LABELS)
    probs = [ref.peaky(rng, T, C, 2.0) for T in (300, 133, 40)]
    lens = [128, 1, 1, 5, 12, 2, 1, 110, 8, 1]
    phrases = [[int(x) for x in rng.integers(1, C, size=L)] for L in lens]
    phrases[3] = ALLE + ALLE[:1]
    n_groups, group_of, first = native.spot_plan(lens)
    assert n_groups == 3 and group_of.tolist() == [0, 0, 1, 1, 1, 1, 1, 1, 2, 2]
    assert first[1] == 255 and first[7] + 2 * 110 - 1 == 256          # groups 0 and 1 are full to the last state
    p_dev, sizes = _padded(probs)
    hits, scores, counts, E, ST = dec.spot(p_dev, sizes, phrases, 4, -np.inf, tracks=True)
    assert counts[0].all()
    for k, ph in enumerate(phrases):
        h1, s1, c1, E1, ST1 = dec.spot(p_dev, sizes, [ph], 4, -np.inf, tracks=True)
        assert np.array_equal(E1[:, 0].view(np.int32), E[:, k].view(np.int32)), k
        assert np.array_equal(ST1[:, 0], ST[:, k]), k
        assert np.array_equal(h1[:, 0], hits[:, k]) and np.array_equal(c1[:, 0], counts[:, k]), k
        assert np.array_equal(s1[:, 0].view(np.int32), scores[:, k].view(np.int32)), k
    dec.close()


def test_ties_follow_the_documented_rule(native):
    dec = native.NativeDecoder(LABELS, blank_index=0)
    C = len(LABELS)
    sizes_in = [6, 40, 5, 2, 300]
    probs = [np.full((T, C), 1.0 / C, dtype=np.float32) for T in sizes_in]
    phrases = [[1, 2], [1, 1], [3], ALLE, ALLE * 3]
    p_dev, sizes = _padded(probs)
    hits, scores, counts, E, ST = dec.spot(p_dev, sizes, phrases, 8, -np.inf, tracks=True)
    for b, p in enumerate(probs):
        for k, ph in enumerate(phrases):
            E32, S32 = ref.tracks(p, ph)
            T = len(p)
            np.testing.assert_array_equal(ST[b, k, :T], S32)
            np.testing.assert_array_equal(E[b, k, :T], E32)
            want = ref.pick(E32, S32, 8)
            assert _hits(hits, scores, counts, b, k) == want, (b, k)
    _check_picking(hits, scores, counts, E, ST, sizes, 8, -np.inf)
    # the hand-worked cases (tests/test_spot_host.py has them against the reference): clip 0 has 6 frames
    assert ST[0, 0, :6].tolist() == [-1, 0, 1, 2, 3, 4]              # token, blank, token: a fresh start and the skip win
    assert [h[:2] for h in _hits(hits, scores, counts, 0, 0)] == [(0, 2), (2, 4), (4, 6)]
    assert ST[0, 1, :6].tolist() == [-1, -1, 0, 1, 2, 3]             # equal tokens: the blank between them, three frames
    assert [h[:2] for h in _hits(hits, scores, counts, 0, 1)] == [(0, 3), (3, 6)]
    assert [h[:2] for h in _hits(hits, scores, counts, 0, 2)] == [(f, f + 1) for f in range(6)]
    assert counts[3].tolist() == [1, 0, 2, 0, 0]                     # two frames
    dec.close()


def _plant(p, at, ids, peak, blank=0):
    """Two frames per token, a blank pair between equal neighbours, each at probability ``peak``; returns the run's end."""
    run = []
    for j, t in enumerate(ids):
        if j and ids[j - 1] == t:
            run += [blank, blank]
        run += [t, t]
    for i, c in enumerate(run):
        row = p[at + i].astype(np.float64)
        row[c] = 0
        row *= (1 - peak) / row.sum()
        row[c] = peak
        p[at + i] = row.astype(np.float32)
    return at + len(run)


@pytest.fixture(scope="module")
def planted():
    rng = np.random.default_rng(3)
    p = ref.peaky(rng, 300, len(LABELS), 3.0)
    runs = []
    for at, peak in ((40, 0.95), (130, 0.8), (220, 0.9)):
        runs.append((at, _plant(p, at, ALLE, peak), peak))
    return p, runs


def test_planted_occurrences(native, planted):
    dec = native.NativeDecoder(LABELS, blank_index=0)
    p, runs = planted
    p_dev, sizes = _padded([p])

    def inside(hit, run):
        (s, e, _), (r0, r1, _) = hit, run
        return r0 <= s <= r0 + 2 and r1 - 2 <= e <= r1

    hits, scores, counts = dec.spot(p_dev, sizes, [ALLE], 2, -np.inf)
    got = _hits(hits, scores, counts, 0, 0)
    assert len(got) == 2 and inside(got[0], runs[0]) and inside(got[1], runs[2]), (got, runs)
    assert got[0][2] > got[1][2]
    hits, scores, counts = dec.spot(p_dev, sizes, [ALLE], 3, -np.inf)
    got = _hits(hits, scores, counts, 0, 0)
    assert len(got) == 3 and inside(got[2], runs[1]), (got, runs)
    hits, scores, counts = dec.spot(p_dev, sizes, [ALLE], 8, float(np.log(0.85)))
    got = _hits(hits, scores, counts, 0, 0)
    assert len(got) == 2 and inside(got[0], runs[0]) and inside(got[1], runs[2]), (got, runs)
    hits, scores, counts = dec.spot(p_dev, sizes, [ALLE], 16, -np.inf)
    spans = sorted((s, e) for s, e, _ in _hits(hits, scores, counts, 0, 0))
    assert len(spans) == 16 and all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))       # disjoint
    assert list(scores[0, 0, :16]) == sorted(scores[0, 0, :16], reverse=True)             # best first
    dec.close()


def test_top_hit_equals_the_alignment_of_its_window(native, planted):
    dec = native.NativeDecoder(LABELS, blank_index=0)
    rng = np.random.default_rng(17)
    C = len(LABELS)
    probs = [planted[0], ref.peaky(rng, 200, C, 3.0), ref.peaky(rng, 77, C, 6.0)]
    phrases = [ALLE, [int(x) for x in rng.integers(1, C, size=7)], [5], [int(x) for x in rng.integers(1, C, size=20)]]
    p_dev, sizes = _padded(probs)
    hits, scores, counts = dec.spot(p_dev, sizes, phrases, 1, -np.inf)
    assert counts.all()
    windows, targets, want = [], [], []
    for b in range(len(probs)):
        for k, ph in enumerate(phrases):
            s, e = hits[b, k, 0]
            windows.append(probs[b][s:e])
            targets.append(ph)
            want.append(float(scores[b, k, 0]))
    w_dev, w_sizes = _padded(windows)
    spans, tp, lp, status = dec.align(w_dev, w_sizes, targets)
    assert not status.any()
    for i, v in enumerate(want):
        assert abs(float(lp[i]) - v) < 1e-3, (i, float(lp[i]), v)
        assert spans[i, 0, 0] == 0 and spans[i, len(targets[i]) - 1, 1] == len(windows[i])      # tight: no blank at either end
    dec.close()


def test_refusals_write_nothing(native):
    dec = native.NativeDecoder(LABELS, blank_index=0)
    L = native.lib()
    B, T, K, Ls, M = 2, 10, 2, 3, 4
    probs = torch.full((B, T, len(LABELS)), 1.0 / len(LABELS), device="cuda")
    ok_sizes = np.array([10, 8], dtype=np.int32)
    ok_ph = np.array([[1, 2, 3], [4, 5, 0]], dtype=np.int32)
    ok_lens = np.array([3, 2], dtype=np.int32)

    def call(B=B, T=T, K=K, sizes=ok_sizes, ph=ok_ph, lens=ok_lens, Ls=Ls, M=M, floor=-np.inf):
        rows = min(max(M, 1), 80)
        hits = np.full((2, 2, rows, 2), 7, dtype=np.int32)
        sc = np.full((2, 2, rows), 7.5, dtype=np.float32)
        cn = np.full((2, 2), 7, dtype=np.int32)
        E = np.full((2, 2, 10), 7.5, dtype=np.float32)
        ST = np.full((2, 2, 10), 7, dtype=np.int32)
        phc = np.ascontiguousarray(ph, dtype=np.int32)
        rc = L.dsmi_spot(dec._h, probs.data_ptr(), native._np_ptr(np.ascontiguousarray(sizes, dtype=np.int32)), B, T,
                         native._np_ptr(phc), native._np_ptr(np.ascontiguousarray(lens, dtype=np.int32)), K, Ls, M, floor,
                         native._np_ptr(hits), native._np_ptr(sc), native._np_ptr(cn), native._np_ptr(E), native._np_ptr(ST), None)
        untouched = (hits == 7).all() and (sc == 7.5).all() and (cn == 7).all() and (E == 7.5).all() and (ST == 7).all()
        return rc, untouched, L.dsmi_decoder_last_error(dec._h).decode(), cn

    rc, untouched, _, cn = call()
    assert rc == 0 and not untouched and cn.tolist() == [[3, 4], [2, 4]]       # windows of 3 and of 2 frames, at most 4 hits
    big = np.ones((2, native.SPOT_MAX_TOKENS + 1), dtype=np.int32)
    invalid = (dict(B=0), dict(B=-1), dict(T=0), dict(T=-3), dict(K=0), dict(K=-1), dict(sizes=[11, 8]), dict(sizes=[-1, 8]),
               dict(lens=[0, 2]), dict(lens=[-1, 2]), dict(lens=[4, 2]), dict(ph=[[1, 0, 3], [4, 5, 0]]),
               dict(ph=[[1, 2, 3], [4, len(LABELS), 0]]), dict(ph=[[1, 2, -2], [4, 5, 0]]), dict(M=0), dict(M=-1),
               dict(M=native.SPOT_MAX_HITS + 1), dict(floor=float("nan")), dict(Ls=0))
    capacity = (dict(ph=big, Ls=native.SPOT_MAX_TOKENS + 1), dict(K=native.SPOT_MAX_PHRASES + 1), dict(B=2 ** 14, K=2 ** 12, T=4),
                dict(T=2 ** 26))
    for code, cases in ((native.DSMI_ERR_INVALID, invalid), (native.DSMI_ERR_CAPACITY, capacity)):
        for kw in cases:
            rc, untouched, msg, _ = call(**kw)
            assert rc == code and untouched and msg, (kw, rc, msg)
    rc, untouched, _, cn = call()
    assert rc == 0 and not untouched and cn.tolist() == [[3, 4], [2, 4]]
    dec.close()


# ---- end to end: the synthetic cfgA-shaped model of tests/test_gpu_align.py (2 conv, 5 x BiGRU 800, sharpened FC weights)
@pytest.fixture(scope="module")
def cfga():
    from danspeech_amd import Recognizer
    from danspeech_amd.deepspeech.model import DeepSpeech
    sd = syn.make_state_dict(2, "gru", 800, 5, seed=0, fc_gain=8.0)
    model = DeepSpeech("cfgA", rnn_type="gru", rnn_hidden_size=800, rnn_layers=5, conv_layers=2).load_state_dict(sd)
    rec = Recognizer(model=model)
    clips = [syn.make_clip(i, n) for i, n in enumerate([48000, 160000, 32000, 96000, 71234])]
    return rec, clips


def test_find_phrases_finds_the_recognised_words(cfga):
    rec, clips = cfga
    texts = rec.recognize_batch(clips)
    timed = rec.align_batch(clips, texts)
    words = sorted(set(w for t in texts for w in t.split() if 3 <= len(w) <= 128))      # (a phrase has at most 128 labels)
    assert words
    found = rec.find_phrases_batch(clips, words)
    assert len(found) == len(clips) and all(len(f) == len(words) for f in found)
    n = 0
    for i, (text, spans) in enumerate(zip(texts, timed)):
        for w, a, e, _ in spans:
            if not 3 <= len(w) <= 128:
                continue
            hits = found[i][words.index(w)]
            assert hits, (i, w)
            assert any(hs < e and a < he for hs, he, _, _ in hits), (i, w, (a, e), hits)
            n += 1
        for hits in found[i]:
            for hs, he, conf, logp in hits:
                assert 0 <= hs < he and 0 < conf <= 1 and logp <= 0
    assert n >= 1
    # the batch is every clip on its own, in the caller's order
    frame_s = rec.danspeech_recognizer.frame_seconds()
    for clip, batch in zip(clips, found):
        single = rec.find_phrases(clip, words)
        assert [[(round(a / frame_s), round(e / frame_s)) for a, e, _, _ in h] for h in single] == \
               [[(round(a / frame_s), round(e / frame_s)) for a, e, _, _ in h] for h in batch]
        for h1, h2 in zip(single, batch):
            np.testing.assert_allclose([x[3] for x in h1], [x[3] for x in h2], rtol=1e-4, atol=1e-4)
    # a floor on the confidence keeps only hits at or above it
    for hits in rec.find_phrases(clips[0], words, max_hits=10, min_confidence=0.5):
        assert all(conf >= 0.5 * (1 - 1e-6) for _, _, conf, _ in hits)


def test_bad_phrases_raise_before_any_gpu_work(cfga, monkeypatch):
    rec, clips = cfga
    eng = rec.danspeech_recognizer
    monkeypatch.setattr(eng, "_enqueue_batch", lambda *a, **k: pytest.fail("GPU work before the phrase check"))
    for bad in ("nr #1", "  \t ", "a" * 129):
        with pytest.raises(ValueError):
            rec.find_phrases_batch(clips[:2], ["ok", bad])
        with pytest.raises(ValueError):
            rec.find_phrases(clips[0], [bad])
    assert rec.find_phrases_batch([], ["ok"]) == []
