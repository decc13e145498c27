"""GPU: ``Recognizer.stream_live`` -- raw continuous audio from several sources to per-utterance texts -- against a reference loop
in this file: the plain-Python listener (``_listen_ref.Gate``, pinned to the reference by g14), ``stream_plan.LivePasses`` and
the existing single-session ``DanSpeechRecognizer.streaming_transcribe``, one source at a time.  (``adjust_for_speech`` and
``adjust_for_ambient_noise`` are checked against their formulas in tests/test_gpu_listen_adjust.py.)"""
import audioop

import numpy as np
import pytest

import _listen_ref as R
from danspeech_amd import synthetic as syn

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CHUNK = 1024


def _stream_model(name, H, L, ctx, seed):
    from danspeech_amd.deepspeech.model import DeepSpeech
    sd = syn.make_state_dict(2, "gru", H, L, bidirectional=False, context=ctx, seed=seed, fc_gain=8.0)
    return DeepSpeech(name, rnn_type="gru", rnn_hidden_size=H, rnn_layers=L, conv_layers=2, context=ctx, bidirectional=False,
                      streaming_inference_model=True).load_state_dict(sd)


def _recording(seed, rate, bursts):
    """int16: quiet noise with loud bursts [(start_s, length_s), ...] -- far enough apart for the gate to close each utterance."""
    n = int(rate * (bursts[-1][0] + bursts[-1][1] + 1.3))
    rng = np.random.RandomState(seed)
    x = rng.randint(-30, 31, size=n).astype(np.float64)
    for j, (t0, length) in enumerate(bursts):
        a, m = int(rate * t0), int(rate * length)
        x[a:a + m] = syn.make_clip(seed * 10 + j, m)
    return x.astype(np.int16)


def _pieces(x, seed, count):
    cuts = sorted(np.random.RandomState(seed).randint(0, len(x) + 1, size=count - 1))
    return [x[a:b] for a, b in zip([0] + cuts, cuts + [len(x)])]


def _sources():
    """Three recordings of two or three bursts, fed in pieces of unequal sizes; the last one at 44.1 kHz."""
    a = _recording(1, 16000, [(0.5, 1.3), (3.0, 0.9), (5.1, 1.1)])
    b = _recording(2, 16000, [(0.0, 1.6), (2.9, 1.2)]).astype(np.float64)
    c = _recording(3, 44100, [(0.7, 1.2), (3.2, 1.4)])
    return [(_pieces(a, 11, 25), 16000), (_pieces(b, 12, 40), 16000), (_pieces(c, 13, 31), 44100)]


def _reference(rec, model, lm_partials, pieces, rate, params):
    """What real_time_streaming would yield for ONE source: listener -> (resampler) -> pass rule -> streaming_transcribe."""
    from danspeech_amd import _native
    from danspeech_amd.stream_plan import LivePasses
    rec.enable_real_time_streaming(streaming_model=model, lm_partials=lm_partials)            # a fresh parser, as a new session has
    eng = rec.danspeech_recognizer
    gate = R.Gate(CHUNK, rate, **params)
    lp = LivePasses(model.context, 16000)
    rs = _native.NativeResampler(eng.audio_parser._frontend(), rate, "polyphase", dtype=np.float64) if rate != 16000 else None
    whole = np.concatenate(pieces)
    mono = whole.astype(np.int16)
    done, pos, want, made = 0, 0, [], []
    for piece in pieces + [None]:
        yields = []
        if piece is not None:
            pos += len(piece)
            while (done + 1) * CHUNK <= pos:
                yields += gate.buffer(audioop.rms(mono[done * CHUNK:(done + 1) * CHUNK].tobytes(), 2), CHUNK)
                done += 1
        else:
            if pos > done * CHUNK:
                yields += gate.buffer(audioop.rms(mono[done * CHUNK:pos].tobytes(), 2), pos - done * CHUNK)
            yields += gate.end()
        segs = [(whole[s:s + c].astype(np.float64), bool(last)) for last, s, c in yields]
        if rs is not None:
            segs = [(rs.push(torch.from_numpy(a).cuda() if len(a) else None, is_last=last).cpu().numpy(), last) for a, last in segs]
        for parts, is_first, is_last in lp.feed(segs):
            text = eng.streaming_transcribe(np.concatenate(parts) if parts else np.zeros(0), is_last=is_last, is_first=is_first)
            made.append((is_first, is_last))
            if text:
                want.append((is_last, text))
    if rs is not None:
        rs.close()
    return want, made


@pytest.fixture(scope="module")
def arpa(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("lm") / "tiny.arpa")
    syn.make_arpa(p, order=3, n_words=300, seed=13, ngrams_per_order=900)
    return p


@pytest.mark.parametrize("lm_partials", [False, True], ids=["greedy", "lm_partials"])
def test_stream_live_equals_the_reference_loop(arpa, lm_partials):
    from danspeech_amd import Recognizer
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    model = _stream_model("stream-live", 64, 2, 20, seed=91)
    rec = Recognizer(model=model, lm=arpa) if lm_partials else Recognizer(model=model)
    model = rec.danspeech_recognizer.model
    sources = _sources()
    params = dict(energy_threshold=rec.energy_threshold, pause_threshold=rec.pause_threshold, phrase_threshold=rec.phrase_threshold,
                  non_speaking_duration=rec.non_speaking_duration)
    rec.enable_real_time_streaming(streaming_model=model, lm_partials=lm_partials)
    got = {k: [] for k in range(len(sources))}
    for k, is_last, text in rec.stream_live([iter(p) for p, _ in sources], chunk=CHUNK, sample_rate=[r for _, r in sources]):
        got[k].append((is_last, text))
    said = 0
    for k, (pieces, rate) in enumerate(sources):
        want, made = _reference(rec, model, lm_partials, pieces, rate, params)
        assert got[k] == want, k
        # the comparison is about something: every burst became an utterance of a first pass, middle passes and a closing one
        bursts = 3 if k == 0 else 2
        assert sum(1 for f, l in made if f) == bursts == sum(1 for f, l in made if l), (k, made)
        assert sum(1 for f, l in made if not f and not l) >= bursts, (k, made)
        said += len(want)
    assert said >= 3                                                          # (the seeded model says little: a few characters per source)
    rec.disable_real_time_streaming()


def test_stream_live_refusals():
    from danspeech_amd import Recognizer
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    model = _stream_model("stream-live", 64, 2, 20, seed=91)
    rec = Recognizer(model=model)
    x = _recording(5, 16000, [(0.2, 0.8)])
    with pytest.raises(RuntimeError):
        list(rec.stream_live([[x]]))
    rec.enable_real_time_streaming(streaming_model=rec.danspeech_recognizer.model)
    with pytest.raises(ValueError):
        list(rec.stream_live([[x]], resample="ratecv"))
    with pytest.raises(ValueError):
        rec.danspeech_recognizer.new_live_session(resample="ratecv")
    with pytest.raises(ValueError):
        list(rec.stream_live([[x], [x]], sample_rate=[16000]))
    rec.pause_threshold = 0.1
    with pytest.raises(ValueError):
        list(rec.stream_live([[x]]))
    rec.pause_threshold = 0.8
    assert list(rec.stream_live([[], [x[:0]]])) == []                         # sources with nothing to say
    rec.disable_real_time_streaming()
