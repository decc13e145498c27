"""CPU checks of CTC phrase search: the packing of phrases into workgroups (dsmi_spot_plan, host only), and the numpy
reference (tests/_spot_ref.py) against a brute force over every window and labelling and against its own float64 form.  No
kernels run."""
import numpy as np
import pytest

import _align_ref as aref
import _spot_ref as ref


# ---- dsmi_spot_plan
def _states(lens):
    return [2 * n - 1 for n in lens]


def test_plan_keeps_the_order_and_fills_groups_of_256_states():
    from danspeech_amd import _native
    assert (_native.SPOT_MAX_TOKENS, _native.SPOT_MAX_PHRASES, _native.SPOT_MAX_HITS) == (128, 4096, 64)
    # 255 + 1 states fill group 0 exactly; the next phrase opens group 1
    n, group_of, first = _native.spot_plan([128, 1, 1, 5, 128, 2])
    assert n == 4
    assert group_of.tolist() == [0, 0, 1, 1, 2, 3]              # states 255 + 1 | 1 + 9 | 255 | 3
    assert first.tolist() == [0, 255, 0, 1, 0, 0]
    # a phrase that does not fit is not split and no later phrase goes back to fill the gap
    lens = [100, 40, 1, 128, 1, 1, 64, 64, 1, 1]
    n, group_of, first = _native.spot_plan(lens)
    g, used, want = 0, 0, []
    for S in _states(lens):
        if used + S > 256:
            g, used = g + 1, 0
        want.append((g, used))
        used += S
    assert list(zip(group_of.tolist(), first.tolist())) == want
    assert n == want[-1][0] + 1 and sorted(group_of.tolist()) == group_of.tolist()
    assert group_of.tolist() == [0, 1, 1, 2, 2, 3, 3, 3, 3, 4]      # 199 | 79 + 1 | 255 + 1 | 1 + 127 + 127 + 1 | 1
    # one-token phrases: 256 to a group
    n, group_of, first = _native.spot_plan([1] * 600)
    assert n == 3 and (group_of == np.arange(600) // 256).all() and (first == np.arange(600) % 256).all()
    n, group_of, first = _native.spot_plan([1] * _native.SPOT_MAX_PHRASES)
    assert n == 16


def test_plan_refuses_bad_arguments():
    from danspeech_amd import _native
    L = _native.lib()
    out = np.zeros((2, 8), dtype=np.int32)

    def call(lens, K=None, a=out[0], b=out[1]):
        lens = np.array(lens, dtype=np.int32)
        return L.dsmi_spot_plan(_native._np_ptr(lens), len(lens) if K is None else K, None if a is None else _native._np_ptr(a),
                                None if b is None else _native._np_ptr(b))

    assert call([3, 2]) == 1
    for kw in (dict(lens=[3, 0]), dict(lens=[-1]), dict(lens=[129]), dict(lens=[1], K=0), dict(lens=[1], K=-2), dict(lens=[1], a=None),
               dict(lens=[1], b=None), dict(lens=[1], K=_native.SPOT_MAX_PHRASES + 1)):
        assert call(**kw) < 0, kw
    assert L.dsmi_spot_plan(None, 1, _native._np_ptr(out[0]), _native._np_ptr(out[1])) < 0
    with pytest.raises(_native.DsmiError):
        _native.spot_plan([])


# ---- the reference against a brute force
def test_reference_equals_brute_force():
    rng = np.random.default_rng(2)
    n = 0
    for case in range(40):
        T = int(rng.integers(1, 7))
        p = rng.dirichlet(np.ones(4) * 0.5, size=T).astype(np.float32)
        phrases = [[int(x) for x in rng.integers(1, 4, size=int(rng.integers(1, 4)))] for _ in range(3)]
        W = ref.brute_force(p, phrases)
        for k, ph in enumerate(phrases):
            E, ST = ref.tracks(p, ph)
            for f in range(T):
                best = W[k][:, f].max()
                if best == -np.inf:
                    assert E[f] == -np.inf and ST[f] == -1
                    continue
                assert abs(float(E[f]) - best) < 1e-5, (case, k, f, float(E[f]), best)
                assert 0 <= ST[f] <= f and abs(W[k][ST[f], f] - best) < 1e-5        # the carried start is a best window's
                n += 1
    assert n > 100


def test_reference_ties_and_picking_on_uniform_probabilities():
    """The hand-worked cases of include/dsmi.h's rule: every frame costs c = log(1/4)."""
    p = np.full((6, 4), 0.25, dtype=np.float32)
    c = np.log(np.float32(0.25))
    E, ST = ref.tracks(p, [1, 2])                 # token, blank, token: from frame 1 on the skip from a fresh start wins
    assert ST.tolist() == [-1, 0, 1, 2, 3, 4]
    assert E[0] == -np.inf and (E[1:] == np.float32(c + c)).all()
    assert [(s, e) for s, e, _ in ref.pick(E, ST, 5)] == [(0, 2), (2, 4), (4, 6)]        # equal scores: the lowest frame first
    assert [(s, e) for s, e, _ in ref.pick(E, ST, 2)] == [(0, 2), (2, 4)]
    E, ST = ref.tracks(p, [1, 1])                 # no skip between equal tokens: three frames
    assert ST.tolist() == [-1, -1, 0, 1, 2, 3]
    assert [(s, e) for s, e, _ in ref.pick(E, ST, 5)] == [(0, 3), (3, 6)]
    E, ST = ref.tracks(p, [3])                    # one token: one frame, every frame a hit of its own
    assert ST.tolist() == list(range(6)) and (E == c).all()
    assert [(s, e) for s, e, _ in ref.pick(E, ST, 4)] == [(0, 1), (1, 2), (2, 3), (3, 4)]
    # the threshold is on the mean: c per frame passes at min_mean_logp = c, nothing passes above it
    assert len(ref.pick(E, ST, 9, c)) == 6 and ref.pick(E, ST, 9, np.float32(c) * np.float32(0.99)) == []
    E, ST = ref.tracks(p[:2], [1, 1])             # fewer frames than the phrase needs
    assert (E == -np.inf).all() and (ST == -1).all() and ref.pick(E, ST, 3) == []
    E, ST = ref.tracks(p[:0], [1])
    assert len(E) == 0 and ref.pick(E, ST, 3) == []


# ---- float32 against float64 on the probabilities of the GPU tests
@pytest.mark.parametrize("sharp", [3.0, 6.0])
def test_reference_float32_against_float64(sharp):
    """End scores within 1e-3 (the bound of the alignment tests for the same float32 sums of lp); the carried start frames
    equal, except where float64's margin between the two best predecessors somewhere on the path is below 1e-4: such a frame
    may differ if the float64 score of its window is within 1e-3 of E64, and at most 1 % of the finite frames may."""
    rng = np.random.default_rng(int(sharp))
    finite = exempt = 0
    worst = 0.0
    for T in (501, 377, 133, 64, 9):
        p = ref.peaky(rng, T, 33, sharp)
        for L in (1, 2, 5, 12):
            ph = [int(x) for x in rng.integers(1, 33, size=L)]
            E32, S32 = ref.tracks(p, ph)
            E64, S64, MG = ref.tracks(p, ph, dtype=np.float64, margins=True)
            assert ((E32 == -np.inf) == (E64 == -np.inf)).all()
            ok = E64 > -np.inf
            finite += int(ok.sum())
            if ok.any():
                worst = max(worst, float(np.abs(E32[ok] - E64[ok]).max()))
            for f in np.nonzero(ok & (S32 != S64))[0]:
                assert MG[f] < 1e-4, (T, L, f, MG[f])
                r = aref.viterbi(p[S32[f]:f + 1], ph, dtype=np.float64)
                assert r is not None and abs(float(r["path_logp"]) - E64[f]) < 1e-3
                exempt += 1
            # the best hit's score is the alignment's of its window: the optimum is tight
            hits = ref.pick(E32, S32, 1)
            if hits:
                s, e, v = hits[0]
                assert float(aref.viterbi(p[s:e], ph)["path_logp"]) == float(v)
    print("finite frames %d, exempt %d, max |E32 - E64| %.3g" % (finite, exempt, worst))
    assert worst < 1e-3
    assert finite > 2000 and exempt <= 0.01 * finite


# ---- the recogniser surface through a stub native decoder (no GPU)
class _FakeModel(object):
    from danspeech_amd import synthetic as _syn
    labels = _syn.DANSPEECH_LABELS
    model_name = "fake"
    device = "cuda:0"
    conv_layers = 2

    def __init__(self):
        from danspeech_amd.deepspeech.utils import get_default_audio_config
        self.audio_conf = get_default_audio_config()

    def to(self, device):
        return self

    def eval(self):
        return self

    def collect(self):
        return False


class _StubNative(object):
    """Stands in for NativeDecoder.spot: clip b, phrase k has k hits [10 b + 4 n, 10 b + 4 n + len(phrase)) of score -(n + 1)."""

    def __init__(self):
        self.calls = []

    def spot(self, probs, sizes, ids, max_hits, min_mean_logp):
        self.calls.append((list(sizes), [list(t) for t in ids], max_hits, min_mean_logp))
        B, K = len(sizes), len(ids)
        hits = np.zeros((B, K, max_hits, 2), dtype=np.int32)
        scores = np.zeros((B, K, max_hits), dtype=np.float32)
        counts = np.zeros((B, K), dtype=np.int32)
        for b in range(B):
            for k in range(K):
                counts[b, k] = min(k, max_hits)
                for n in range(counts[b, k]):
                    hits[b, k, n] = (10 * b + 4 * n, 10 * b + 4 * n + len(ids[k]))
                    scores[b, k, n] = -(n + 1)
        return hits, scores, counts


def _engine(monkeypatch, stub):
    from danspeech_amd import Recognizer
    from danspeech_amd.deepspeech.decoder import Decoder
    from danspeech_amd.DanSpeechRecognizer import _BatchJob
    r = Recognizer()
    r.update_model(_FakeModel())
    eng = r.danspeech_recognizer
    monkeypatch.setattr(Decoder, "_on_gpu", staticmethod(lambda p: p))
    monkeypatch.setattr(eng.decoder, "_dec", lambda device_index, slot=0: stub)

    def enqueue(recordings, *a, **k):
        order = np.argsort([-len(x) for x in recordings], kind="stable")
        probs = np.zeros((len(recordings), 1, len(_FakeModel.labels)), dtype=np.float32)
        return _BatchJob(order, probs, np.array([len(recordings[i]) for i in order], dtype=np.int32), len(recordings), _FakeModel())
    monkeypatch.setattr(eng, "_enqueue_batch", enqueue)
    return r


def test_seconds_confidence_and_order_through_a_stub_decoder(monkeypatch):
    stub = _StubNative()
    r = _engine(monkeypatch, stub)
    labels = _FakeModel.labels
    clips = [np.zeros(300), np.zeros(100), np.zeros(500)]
    out = r.find_phrases_batch(clips, ["  Hej ", "ÅL  ok", "de"], max_hits=3, min_confidence=0.25)
    sizes, ids, max_hits, floor = stub.calls[0]
    assert sizes == [500, 300, 100] and max_hits == 3 and floor == pytest.approx(np.log(0.25))      # longest first
    assert ids == [[labels.index(c) for c in t] for t in ("hej", "ål ok", "de")]                      # normalised, caller's order
    # clip 0 of the caller is position 1 of the batch; phrase k has k hits
    assert [len(h) for h in out[0]] == [0, 1, 2] and [len(h) for h in out[2]] == [0, 1, 2]
    (a, e, conf, logp), = out[0][1]
    assert (a, e, logp) == (pytest.approx(10 * 0.02), pytest.approx(15 * 0.02), -1.0) and conf == pytest.approx(np.exp(-1 / 5))
    (a, e, conf, logp) = out[1][2][1]                      # clip 1 = position 2, second hit of "de"
    assert (a, e, logp) == (pytest.approx(24 * 0.02), pytest.approx(26 * 0.02), -2.0) and conf == pytest.approx(np.exp(-1.0))
    assert r.find_phrases(clips[2], ["hej", "ål ok", "de"], max_hits=3, min_confidence=0.25) == out[2]
    r.find_phrases(clips[0], ["hej"])
    assert stub.calls[-1][2:] == (5, -np.inf)              # no floor on the confidence by default
    assert r.find_phrases_batch(clips, []) == [[], [], []] and r.find_phrases_batch([], ["hej"]) == []


def test_bad_phrases_raise_before_the_forward(monkeypatch):
    r = _engine(monkeypatch, _StubNative())
    monkeypatch.setattr(r.danspeech_recognizer, "_enqueue_batch", lambda *a, **k: pytest.fail("GPU work before the phrase check"))
    with pytest.raises(ValueError, match="'#'"):
        r.find_phrases_batch([np.zeros(10)], ["ok", "nr #1"])
    with pytest.raises(ValueError, match="empty"):
        r.find_phrases(np.zeros(10), ["ok", " \t"])
    with pytest.raises(ValueError, match="longer than 128"):
        r.find_phrases(np.zeros(10), ["a" * 129])
    from danspeech_amd.deepspeech.decoder import GreedyDecoder
    d = GreedyDecoder(labels=_FakeModel.labels, blank_index=0)
    assert len(d.phrase_ids("a" * 128)) == 128
    with pytest.raises(ValueError):          # probs on the host: a GPU would be needed past the check
        d.spot(np.zeros((1, 4, len(_FakeModel.labels)), dtype=np.float32), ["hej!"])


def test_find_phrases_without_a_model_raises():
    from danspeech_amd import Recognizer
    from danspeech_amd.errors.recognizer_errors import ModelNotInitialized
    with pytest.raises(ModelNotInitialized):
        Recognizer().find_phrases(np.zeros(100), ["hej"])
