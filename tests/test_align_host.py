"""CPU checks of CTC forced alignment: transcript normalisation and label checks, the feasibility count, the grouping of token
spans into timed words (through a stub native decoder, no GPU), and the numpy reference (tests/_align_ref.py) against a
brute-force enumeration of every CTC path.  No kernels run."""
import numpy as np
import pytest

from danspeech_amd import synthetic as syn

import _align_ref as ref

LABELS = syn.DANSPEECH_LABELS


def _greedy():
    from danspeech_amd.deepspeech.decoder import GreedyDecoder
    return GreedyDecoder(labels=LABELS, blank_index=0)


def test_normalisation():
    from danspeech_amd.deepspeech.decoder import Decoder
    assert Decoder.normalise_transcript("  Hej   MED\tdig\n") == "hej med dig"
    assert Decoder.normalise_transcript("ÆBLE  Øl Å") == "æble øl å"
    assert Decoder.normalise_transcript(" \t ") == ""
    d = _greedy()
    assert list(d.transcript_ids("hej med")) == [LABELS.index(c) for c in "hej med"]
    assert d.transcript_ids("").shape == (0,)


@pytest.mark.parametrize("text, bad", [("hej!", "'!'"), ("a_b", "'_'"), ("år 2024", "'0', '2', '4'")])
def test_characters_that_are_not_labels_raise_before_any_gpu_work(text, bad):
    d = _greedy()
    with pytest.raises(ValueError) as e:
        d.transcript_ids(d.normalise_transcript(text))
    assert bad in str(e.value)
    with pytest.raises(ValueError):          # probs on the host: a GPU would be needed past the check
        d.align(np.zeros((1, 4, len(LABELS)), dtype=np.float32), [text])


def test_feasibility_count_with_repeated_letters():
    d = _greedy()
    assert ref.min_frames(d.transcript_ids("alle")) == 5
    assert ref.min_frames(d.transcript_ids("ll")) == 3
    assert ref.min_frames(d.transcript_ids("lll")) == 5
    assert ref.min_frames(d.transcript_ids("hej med dig")) == 11
    assert ref.min_frames([]) == 0
    # the reference's feasibility is exactly the existence of a path (brute force, 5 labels)
    rng = np.random.default_rng(0)
    for targets in ([1, 1], [1, 2, 1], [2, 2, 2], [3], [1, 2]):
        for T in range(1, 6):
            p = rng.dirichlet(np.ones(5), size=T).astype(np.float32)
            feasible = ref.min_frames(targets) <= T
            assert (ref.viterbi(p, targets) is not None) == feasible
            assert (ref.brute_force(p, targets) is not None) == feasible


def test_reference_equals_brute_force():
    rng = np.random.default_rng(1)
    n = 0
    for T in range(1, 8):
        for _ in range(6):
            L = int(rng.integers(0, 4))
            targets = [int(x) for x in rng.integers(1, 5, size=L)]
            if ref.min_frames(targets) > T:
                continue
            p = (rng.dirichlet(np.ones(5) * 0.5, size=T)).astype(np.float32)
            r = ref.viterbi(p, targets)
            best, _ = ref.brute_force(p, targets)
            lab = ref.path_from_spans(r["spans"], targets, T)
            assert ref.collapse(lab) == targets
            assert abs(float(r["path_logp"]) - best) < 1e-5
            assert abs(ref.rescore64(p, lab) - best) < 1e-5
            n += 1
    assert n > 20


def test_reference_tie_rule_on_uniform_probabilities():
    """Every path scores the same: the predecessor order s, s-1, s-2 and the trailing blank at the end decide."""
    p = np.full((5, 5), 0.2, dtype=np.float32)
    r = ref.viterbi(p, [1, 2])
    assert list(r["path"]) == [1, 3, 4, 4, 4]
    assert r["spans"].tolist() == [[0, 1], [1, 2]]
    r = ref.viterbi(p, [1, 1])                 # no skip between equal tokens
    assert list(r["path"]) == [1, 2, 3, 4, 4]
    r = ref.viterbi(p, [])
    assert list(r["path"]) == [0] * 5
    np.testing.assert_allclose(float(r["path_logp"]), 5 * np.log(0.2), rtol=1e-6)


class _FakeModel(object):
    labels = LABELS
    model_name = "fake"
    device = "cuda:0"
    conv_layers = 2

    def __init__(self, window_stride=0.01):
        self.audio_conf = dict(syn_audio_conf(), window_stride=window_stride)

    def to(self, device):
        return self

    def eval(self):
        return self

    def collect(self):
        return False


def syn_audio_conf():
    from danspeech_amd.deepspeech.utils import get_default_audio_config
    return get_default_audio_config()


class _StubNative(object):
    """Stands in for NativeDecoder.align: fixed spans, token probabilities 0.5 + k / 100, status from `infeasible`."""

    def __init__(self, infeasible=()):
        self.infeasible = set(infeasible)
        self.calls = []

    def align(self, probs, sizes, ids):
        self.calls.append((probs, None if sizes is None else list(sizes), [list(t) for t in ids]))
        B, Ls = len(ids), max(len(t) for t in ids)
        spans = np.zeros((B, Ls, 2), dtype=np.int32)
        tp = np.zeros((B, Ls), dtype=np.float32)
        for b, t in enumerate(ids):
            for k in range(len(t)):
                spans[b, k] = (3 * k + 1, 3 * k + 3)
                tp[b, k] = 0.5 + k / 100
        status = np.array([1 if b in self.infeasible else 0 for b in range(B)], dtype=np.int32)
        lp = np.where(status == 1, -np.inf, -1.0).astype(np.float32)
        return spans, tp, lp, status


def _engine(monkeypatch, stub, window_stride=0.01):
    from danspeech_amd import Recognizer
    from danspeech_amd.deepspeech.decoder import Decoder
    from danspeech_amd.DanSpeechRecognizer import _BatchJob
    r = Recognizer()
    r.update_model(_FakeModel(window_stride))
    eng = r.danspeech_recognizer
    monkeypatch.setattr(Decoder, "_on_gpu", staticmethod(lambda p: p))
    monkeypatch.setattr(eng.decoder, "_dec", lambda device_index, slot=0: stub)

    def enqueue(recordings, *a, **k):
        order = np.argsort([-len(x) for x in recordings], kind="stable")
        probs = np.zeros((len(recordings), 1, len(LABELS)), dtype=np.float32)
        return _BatchJob(order, probs, np.array([len(recordings[i]) for i in order], dtype=np.int32), len(recordings), _FakeModel())
    monkeypatch.setattr(eng, "_enqueue_batch", enqueue)
    return r


def test_words_and_seconds_through_a_stub_decoder(monkeypatch):
    stub = _StubNative(infeasible={1})        # position 1 of the longest-first order: the caller's clip 0
    r = _engine(monkeypatch, stub)
    clips = [np.zeros(300), np.zeros(100), np.zeros(500)]
    out = r.align_batch(clips, ["  Hej  Du ", "a", "Ål ok"])
    # longest first: clip 2, clip 0, clip 1; the transcripts follow that order, normalised
    assert stub.calls[0][2] == [[LABELS.index(c) for c in t] for t in ("ål ok", "hej du", "a")]
    assert stub.calls[0][1] == [500, 300, 100]
    assert out[0] is None
    assert out[1] == [("a", pytest.approx(0.02), pytest.approx(0.06), pytest.approx(0.5))]
    # "ål ok": tokens 0..4 span frames [3k+1, 3k+3); words "ål" (tokens 0, 1) and "ok" (tokens 3, 4)
    (w0, s0, e0, c0), (w1, s1, e1, c1) = out[2]
    assert (w0, w1) == ("ål", "ok")
    assert s0 == pytest.approx(1 * 0.02) and e0 == pytest.approx(6 * 0.02) and c0 == pytest.approx(0.505)
    assert s1 == pytest.approx(10 * 0.02) and e1 == pytest.approx(15 * 0.02) and c1 == pytest.approx(0.535)
    assert r.align(clips[2], "Ål ok") == out[2]


def test_frame_seconds_follow_the_hop_and_the_conv_strides(monkeypatch):
    r = _engine(monkeypatch, _StubNative(), window_stride=0.015)
    eng = r.danspeech_recognizer
    assert eng.frame_seconds() == pytest.approx(0.03)
    for layers in (1, 2, 3):
        eng.model.conv_layers = layers
        assert eng.frame_seconds() == pytest.approx(0.03)
    out = r.align(np.zeros(10), "ab")
    assert out == [("ab", pytest.approx(0.03), pytest.approx(6 * 0.03), pytest.approx(0.505))]


def test_unknown_characters_raise_before_the_forward(monkeypatch):
    r = _engine(monkeypatch, _StubNative())
    eng = r.danspeech_recognizer
    monkeypatch.setattr(eng, "_enqueue_batch", lambda *a, **k: pytest.fail("GPU work before the transcript check"))
    with pytest.raises(ValueError, match="'#'"):
        r.align_batch([np.zeros(10), np.zeros(10)], ["ok", "nr #1"])
    with pytest.raises(ValueError):
        r.align_batch([np.zeros(10)], ["a", "b"])
    assert r.align_batch([], []) == []


def test_align_without_a_model_raises():
    from danspeech_amd import Recognizer
    from danspeech_amd.errors.recognizer_errors import ModelNotInitialized
    r = Recognizer()
    with pytest.raises(ModelNotInitialized):
        r.align(np.zeros(100), "hej")
    with pytest.raises(ModelNotInitialized):
        r.align_batch([np.zeros(100)], ["hej"])
