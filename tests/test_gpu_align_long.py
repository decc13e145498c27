"""Long-form CTC forced alignment on the GPU (dsmi_align_long: csrc/ctc_tools.hip, the kernels csrc/align_long.hip): bit for bit
dsmi_align where dsmi_align can go, the numpy reference of tests/_align_long_ref.py beyond it and with free ends, the paths that
strain the tiling (two states per frame; one state for whole frame tiles), one handle across calls of different sizes, the
refusals, and the recogniser surface on a synthetic cfgA-shaped model.  W and F come from dsmi_align_long_plan.

Tolerances.  Spans and token means are compared exactly.  A score is compared with the float64 optimum under (T + 2) 2^-24
|logp|: the running float32 sum is rounded once per frame, each rounding at most 2^-24 of a partial sum that is at most |logp| in
size, and every term is a float32 logarithm, at most 2^-23 of itself from the float64 one.  The test beyond dsmi_align's limit
holds T 2^-24 |logp|."""
import itertools

import numpy as np
import pytest

from danspeech_amd import synthetic as syn

import _align_long_ref as lr
import _align_ref as ar

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
LABELS = syn.DANSPEECH_LABELS
C = len(LABELS)
FLAGS = list(itertools.product((False, True), repeat=2))


@pytest.fixture(scope="module")
def native():
    from danspeech_amd import _native
    return _native


@pytest.fixture(scope="module")
def dec(native):
    d = native.NativeDecoder(LABELS, blank_index=0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def geometry(native):
    g = native.align_long_plan(1000, 100)
    return g["W"], g["F"]


def _peaky(rng, T, sharp, blank_boost=1.5):
    z = rng.normal(size=(T, C)) * sharp
    z[:, 0] += blank_boost * sharp
    z -= z.max(1, keepdims=True)
    p = np.exp(z)
    return (p / p.sum(1, keepdims=True)).astype(np.float32)


def _greedy(p):
    return np.array(ar.collapse(p.argmax(1)), dtype=np.int32)


def _dev(p):
    return torch.from_numpy(np.ascontiguousarray(p)).cuda()


def _bound(T, logp):
    return (T + 2) * 2.0 ** -24 * abs(logp)


def _long(dec, p, tg, lead=False, tail=False):
    return dec.align_long(_dev(p), tg, lead, tail)


def _assert_equals_align(dec, p, tg):
    """dsmi_align_long with both ends costly against dsmi_align of the same clip: every output, bit for bit."""
    pd = _dev(p)
    sp, tp, lp, st = dec.align_long(pd, tg, False, False)
    sp1, tp1, lp1, st1 = dec.align(pd[None], None, [list(tg)])
    L = len(tg)
    assert st == int(st1[0]), (len(p), L)
    assert np.float32(lp).tobytes() == lp1[:1].tobytes(), (len(p), L, lp, lp1[0])
    assert np.array_equal(sp, sp1[0, :L]), (len(p), L)
    assert tp.tobytes() == tp1[0, :L].tobytes(), (len(p), L)
    return st


@pytest.mark.parametrize("kind", ["uniform", "peaky"])
def test_equal_to_align_bit_for_bit(dec, geometry, kind):
    """Frames below, at and above the frame tile, states below, at and above the state tile (S is odd: W itself when W is), and
    enough frames for the long transcripts to fit; with uniform probabilities every comparison is a tie."""
    W, F = geometry
    rng = np.random.default_rng(3)
    frames = [1, 2, F, F + 1, F + 2, 2 * F + 1, 3 * F - 1, W // 2 + 3, W // 2 + F + 1, W + 2 * F + 1, 2 * W, W + 7 * F]
    states = sorted(set(S for S in (1, 3, W - 1, W, W + 1, 2 * W + 1) if S % 2 == 1))
    assert max(states) // 2 <= 4096
    aligned = infeasible = long_aligned = 0
    for T in frames:
        p = np.full((T, C), 1.0 / C, dtype=np.float32) if kind == "uniform" else _peaky(rng, T, 3.0)
        for S in states:
            L = S // 2
            tg = rng.integers(1, 4, size=L) if kind == "uniform" else rng.integers(1, C, size=L)
            if _assert_equals_align(dec, p, tg.astype(np.int32)):
                infeasible += 1
            else:
                aligned += 1
                long_aligned += S >= W - 1
    assert aligned >= 2 * len(frames) and long_aligned >= 5 and infeasible > 0
    # the longest transcripts of the list fit the last frame counts: without equal neighbours at exactly T = L, too
    tg = (1 + np.arange(W) % 3).astype(np.int32)
    for T in (W, W + 1, W + F):
        p = np.full((T, C), 1.0 / C, dtype=np.float32) if kind == "uniform" else _peaky(rng, T, 3.0)
        assert _assert_equals_align(dec, p, tg) == 0


def test_infeasible_clip(dec):
    rng = np.random.default_rng(4)
    p = _peaky(rng, 5, 3.0)
    for tg in ([1, 2, 3, 4, 5, 6], [1, 1, 2, 2]):           # 6 tokens; 4 tokens and two blanks between equal neighbours
        for lead, tail in FLAGS:
            sp, tp, lp, st = _long(dec, p, np.array(tg, dtype=np.int32), lead, tail)
            assert st == 1 and lp == -np.inf and not sp.any() and not tp.any()
    assert _assert_equals_align(dec, p, np.array([1, 1, 2, 2], dtype=np.int32)) == 1
    assert _assert_equals_align(dec, p, np.array([1, 1, 2, 3], dtype=np.int32)) == 0      # exactly 5 frames


def test_steepest_path(dec, geometry):
    """T = L frames, frame t on token t, neighbours pairwise different: the only path moves two states per frame, through every
    state tile, the whole halo and the whole backtrace window.  A halo or a window one state short gives -inf."""
    W, F = geometry
    L = max(W + 2, 3 * F + 2)                     # 2L + 1 states: more than two state tiles; L - 1 frames: three frame tiles and more
    tg = (1 + np.arange(L) % 5).astype(np.int32)
    p = np.full((L, C), 0.1 / (C - 1), dtype=np.float32)
    p[np.arange(L), tg] = 0.9
    sp, tp, lp, st = _long(dec, p, tg)
    assert st == 0 and np.isfinite(lp)
    assert np.array_equal(sp, np.stack([np.arange(L), np.arange(L) + 1], 1))
    assert np.all(tp == np.float32(0.9))
    assert abs(lp - L * np.log(0.9)) <= _bound(L, L * np.log(0.9)) + 1e-6 * L
    for lead, tail in FLAGS[1:]:                  # a free end changes nothing: no frame is left for it
        sp2, _, lp2, _ = _long(dec, p, tg, lead, tail)
        assert np.array_equal(sp2, sp) and lp2 == lp


def test_flattest_path(dec, geometry):
    """3F + 5 frames of blank, then a short word: the path sits in state 0 across whole frame tiles."""
    W, F = geometry
    T0 = 3 * F + 5
    word = np.array([LABELS.index(c) for c in "hej"], dtype=np.int32)
    p = np.full((T0 + 3, C), 0.02 / (C - 1), dtype=np.float32)
    p[:T0, 0] = 0.98
    for k, c in enumerate(word):
        p[T0 + k, 0] = 0.02 / (C - 1)
        p[T0 + k, c] = 0.98
    want = lr.viterbi(p, word)
    assert want["spans"].tolist() == [[T0, T0 + 1], [T0 + 1, T0 + 2], [T0 + 2, T0 + 3]]
    for lead, tail in FLAGS:
        sp, tp, lp, st = _long(dec, p, word, lead, tail)
        assert st == 0 and np.array_equal(sp, want["spans"]) and tp.tobytes() == want["token_probs"].tobytes()
        r64 = lr.viterbi(p, word, lead, tail, dtype=np.float64)
        assert abs(lp - float(r64["path_logp"])) <= _bound(len(p), float(r64["path_logp"])) + 1e-7
    _assert_equals_align(dec, p, word)


@pytest.fixture(scope="module")
def beyond():
    """7000 peaky frames and their greedy transcript, with the float32 and the float64 reference."""
    rng = np.random.default_rng(21)
    p = _peaky(rng, 7000, 6.0)
    tg = _greedy(p)
    return p, tg, lr.viterbi(p, tg), lr.viterbi(p, tg, dtype=np.float64)


def test_beyond_the_limit_of_align(native, dec, beyond):
    """More tokens than dsmi_align takes: the test that cannot pass without dsmi_align_long."""
    p, tg, r32, r64 = beyond
    T, L = len(p), len(tg)
    assert L > native.ALIGN_MAX_TOKENS
    sp, tp, lp, st = _long(dec, p, tg)
    assert st == 0
    assert np.array_equal(sp, r32["spans"])
    assert tp.tobytes() == r32["token_probs"].tobytes()
    lab = ar.path_from_spans(sp, tg, T)
    best = float(r64["path_logp"])
    bound = T * 2.0 ** -24 * abs(best)
    print("beyond: L = %d, logp %.6f, float64 optimum %.6f, bound %.3e" % (L, lp, best, bound))
    assert abs(ar.rescore64(p, lab) - best) <= 1e-6
    assert abs(lp - best) <= bound
    with pytest.raises(native.DsmiError) as e:
        dec.align(_dev(p)[None], None, [list(tg)])
    assert e.value.code == native.DSMI_ERR_CAPACITY


@pytest.fixture(scope="module")
def ends():
    """700 junk frames, 3000 frames of speech, 400 junk frames; the transcript is the greedy text of the middle."""
    rng = np.random.default_rng(22)
    p = _peaky(rng, 4100, 6.0)
    tg = _greedy(p[700:3700])
    refs = {fl: (lr.viterbi(p, tg, *fl), float(lr.viterbi(p, tg, *fl, dtype=np.float64)["path_logp"])) for fl in FLAGS}
    return p, tg, refs, lr.viterbi(p[700:3700], tg)


def test_free_ends(dec, ends):
    p, tg, refs, ref_mid = ends
    T = len(p)
    mid = _long(dec, p[700:3700], tg)
    assert mid[3] == 0 and np.array_equal(mid[0], ref_mid["spans"])
    both = _long(dec, p, tg, True, True)
    assert both[3] == 0
    assert np.array_equal(both[0], mid[0] + 700)
    assert both[1].tobytes() == mid[1].tobytes()
    none = _long(dec, p, tg)
    assert none[3] == 0 and not np.array_equal(none[0], mid[0] + 700)
    for lead, tail in FLAGS:
        got = both if (lead and tail) else none if not (lead or tail) else _long(dec, p, tg, lead, tail)
        want, w64 = refs[(lead, tail)]
        assert np.array_equal(got[0], want["spans"]), (lead, tail)
        assert got[1].tobytes() == want["token_probs"].tobytes(), (lead, tail)
        assert abs(got[2] - w64) <= _bound(T, w64), (lead, tail, got[2], w64)
    # the free stretches cost nothing, and neither do the middle's own first and last blank frames
    assert both[2] >= mid[2]


def test_no_tokens_under_every_flag(dec, ends):
    p = ends[0]
    none = np.zeros(0, dtype=np.int32)
    for T in (1, 65, 700):
        blank64 = float(np.sum(np.log(np.maximum(p[:T, 0], ar.FLT_MIN).astype(np.float64))))
        for lead, tail in FLAGS:
            sp, tp, lp, st = _long(dec, p[:T], none, lead, tail)
            assert st == 0 and sp.shape == (0, 2) and tp.shape == (0,)
            if lead or tail:
                assert lp == 0.0
            else:
                assert abs(lp - blank64) <= _bound(T, blank64)


def test_one_handle_across_sizes_and_a_refused_call(native, beyond, ends):
    """Grow, shrink, grow on one handle: what fresh handles give.  A refused call in between writes nothing and changes nothing."""
    big_p, big_tg = beyond[0], beyond[1]
    p, tg = ends[0], ends[1]
    calls = [(p[:200], tg[:40], True, False), (big_p, big_tg, False, False), (p[:70], tg[:9], False, True), (p, tg, True, True),
             (p[:1], tg[:0], False, False)]
    one = native.NativeDecoder(LABELS, blank_index=0)
    lib = native.lib()
    for i, (q, t, lead, tail) in enumerate(calls):
        fresh = native.NativeDecoder(LABELS, blank_index=0)
        want = fresh.align_long(_dev(q), t, lead, tail)
        fresh.close()
        got = one.align_long(_dev(q), t, lead, tail)
        assert got[3] == want[3] == 0
        assert np.array_equal(got[0], want[0]) and got[1].tobytes() == want[1].tobytes() and np.float32(got[2]).tobytes() == np.float32(want[2]).tobytes(), i
        if i == 1:
            qd = _dev(p[:50])
            for kw in (dict(T=0), dict(T=-1), dict(L=-1), dict(lead=2), dict(tail=-1), dict(bad=0), dict(bad=C), dict(T=(1 << 22) + 1),
                       dict(L=(1 << 20) + 1), dict(null="probs"), dict(null="logp")):
                tgt = np.array([1, 2, 3, 4], dtype=np.int32)
                if "bad" in kw:
                    tgt[2] = kw["bad"]
                sp = np.full((4, 2), 7, dtype=np.int32)
                tp = np.full(4, 7.5, dtype=np.float32)
                lp = np.full(1, 7.5, dtype=np.float32)
                st = np.full(1, 7, dtype=np.int32)
                rc = lib.dsmi_align_long(one._h, None if kw.get("null") == "probs" else qd.data_ptr(), kw.get("T", 50), native._np_ptr(tgt),
                                         kw.get("L", 4), kw.get("lead", 0), kw.get("tail", 0), native._np_ptr(sp), native._np_ptr(tp),
                                         None if kw.get("null") == "logp" else native._np_ptr(lp), native._np_ptr(st), None)
                want_rc = native.DSMI_ERR_CAPACITY if kw.get("T", 0) > (1 << 22) or kw.get("L", 0) > (1 << 20) else native.DSMI_ERR_INVALID
                assert rc == want_rc, (kw, rc)
                assert (sp == 7).all() and (tp == 7.5).all() and (lp == 7.5).all() and (st == 7).all(), kw
                assert lib.dsmi_decoder_last_error(one._h).decode(), kw
    one.close()


# ---- the surface: a synthetic cfgA-shaped model (2 conv, 5 x BiGRU 800) as tests/test_gpu_align.py's, with weights that make it
# speak as a trained model does: sharp (mean top probability above 0.9: where the model is unsure, free ends let a transcript
# shrink into few frames, as they should), blanks between characters (synthetic.TALKATIVE's means) and, by the same means, spaces
@pytest.fixture(scope="module")
def cfga():
    from danspeech_amd import Recognizer
    from danspeech_amd.deepspeech.model import DeepSpeech
    sd = syn.make_state_dict(2, "gru", 800, 5, seed=0, fc_gain=24.0, ih_gain=6.0, blank_boost=24.0)
    w = sd["fc.0.module.1.weight"][LABELS.index(" ")].astype(np.float64)
    sd["fc.0.module.0.bias"] = (sd["fc.0.module.0.bias"] + 24.0 * w / np.dot(w, w)).astype(np.float32)      # 24 logits onto the space
    model = DeepSpeech("cfgA", rnn_type="gru", rnn_hidden_size=800, rnn_layers=5, conv_layers=2).load_state_dict(sd)
    rec = Recognizer(model=model)
    rng = np.random.default_rng(8)
    parts = [rng.normal(0, 60, 16000)]
    for i, n in enumerate([48000, 71234, 32000, 96000]):
        parts += [syn.make_clip(i, n), rng.normal(0, 60, 16000 + 4000 * i)]
    return rec, np.round(np.concatenate(parts))


def test_surface_sentences_lie_in_their_phrases(cfga):
    rec, audio = cfga
    eng = rec.danspeech_recognizer
    phrases = rec.recognize_long(audio, max_batch=3)
    assert len(phrases) == 4
    sentences = [text for _, _, text in phrases]
    assert all(eng.decoder.normalise_transcript(s) for s in sentences)
    got = rec.align_long(audio, sentences, max_batch=3)
    assert got is not None and len(got) == 4
    frame_s, rate = eng.frame_seconds(), 16000.0
    last = 0.0
    for (a, b, text), (start_s, end_s, conf, words) in zip(phrases, got):
        # inside the phrase: its last frame may reach one frame past the phrase's last sample
        assert a / rate <= start_s < end_s <= b / rate + frame_s, (a, b, start_s, end_s)
        assert 0 < conf <= 1
        assert [w for w, *_ in words] == text.split()
        assert words[0][1] == start_s and words[-1][2] == end_s
        for w, ws, we, wc in words:
            assert last <= ws < we and 0 < wc <= 1      # monotone over the whole recording
            last = we
    # the words against align_batch of each phrase with its own text.  The joined transcript has one character more per phrase
    # boundary than the phrases' own texts, the space between two sentences, and that space takes a frame next to the boundary:
    # a sentence's first and last word are compared by name only, every word between them by its frames.
    own = rec.align_batch([audio[a:b] for a, b, _ in phrases], sentences)
    compared = 0
    for (a, b, _), (_, _, _, words), alone in zip(phrases, got, own):
        if alone is None:
            continue
        assert [w for w, *_ in alone] == [w for w, *_ in words]
        for (w, ws, we, _), (_, vs, ve, _) in list(zip(words, alone))[1:-1]:
            assert round((ws - a / rate) / frame_s) == round(vs / frame_s) and round((we - a / rate) / frame_s) == round(ve / frame_s), w
            compared += 1
    assert compared >= 5


def test_surface_value_errors(cfga):
    rec, audio = cfga
    with pytest.raises(ValueError):
        rec.align_long(audio, ["hej", "  "])
    with pytest.raises(ValueError):
        rec.align_long(audio, ["hej", "x_y"])         # the blank's character is not a label of a transcript
    with pytest.raises(ValueError):
        rec.align_long(audio, ["hej 123"])
    assert rec.align_long(audio, ["a" * 30000]) is None
