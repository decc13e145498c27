"""Sample-rate conversion on the GPU (dsmi_resample, csrc/resample.hip) through the C ABI and the Python surface.

  ratecv     exactly the reference's results (tests/golden/g13_ratecv.npz) and exactly tests/_resample_ref.py on ragged batches
  polyphase  every output within (K + 18) 2^-52 sum_k |x[k] h[j down - k up]| of the numpy reference, K = that output's taps:
             K + 2 covers a float64 sum of K products in any order, 16 the filter (dsmi_resample_taps against numpy,
             tests/test_resample_host.py).  The reference computes the right-hand side itself.
  both       equal rates copy; features of a resampled batch = features of the same samples uploaded; refusals write nothing
  end to end recognize_files / recognize_batch / recognize_long on audio of other rates against the same calls on the
             host-reference-resampled arrays (cfgA-shaped model, ``synthetic.TALKATIVE`` weights)
"""
import ctypes as C
import wave

import numpy as np
import pytest

import _resample_ref as R
from danspeech_amd import synthetic as syn

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = -12345.678


@pytest.fixture(scope="module")
def fe():
    from danspeech_amd import _native
    assert torch.cuda.is_available()
    f = _native.NativeFrontend()
    yield f
    f.close()


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()          # (a copy: golden arrays are read-only)


def _split(out, n_out):
    out = out.cpu().numpy()
    cuts = np.concatenate(([0], np.cumsum(n_out)))
    assert cuts[-1] == len(out)
    return [out[cuts[i]:cuts[i + 1]] for i in range(len(n_out))]


# ---- ratecv ----------------------------------------------------------------------------------------------------------------
def test_ratecv_equals_the_reference_golden(fe, golden):
    g = golden("g13_ratecv")
    for c in range(int(g["n_cases"])):
        width, nch, rate = (int(v) for v in g["fmt_%d" % c])
        raw = g["raw_%d" % c]
        out, n_out = fe.resample(_dev(raw), [len(raw) // (width * nch)], rate, "ratecv", wav_format=(width, nch))
        want = g["out_%d" % c]
        assert n_out.tolist() == [len(want)], c
        assert np.array_equal(R.as_reference_array(out.cpu().numpy(), width), want), (c, width, nch, rate)


@pytest.mark.parametrize("width,nch", [(2, 1), (3, 1), (4, 1), (1, 1), (2, 2), (3, 2), (4, 2)])
def test_ratecv_ragged_batch_equals_the_numpy_reference(fe, width, nch):
    rng = np.random.default_rng(10 * width + nch)
    lim = 1 << (8 * width - 1)
    lengths = [700, 0, 1, 1333, 2, 0, 5, 3000]
    for rate in (44100, 8000, 16001, 11025):
        raws = [R.encode(rng.integers(-lim, lim, size=n * nch), width) for n in lengths]
        out, n_out = fe.resample(_dev(np.frombuffer(b"".join(raws), dtype=np.uint8)), lengths, rate, "ratecv", wav_format=(width, nch))
        got = _split(out, n_out)
        for raw, n, y in zip(raws, lengths, got):
            want = R.ratecv(R.decode(raw, width, nch), width, rate)
            assert len(y) == len(want) == R.count(R.RATECV, rate, 16000, n)
            assert np.array_equal(y, want.astype(np.float64)), (rate, n)
    # plain int16 tensors (what recognize_batch uploads) take the same path
    x = rng.integers(-32768, 32768, size=2500).astype(np.int16)
    out, n_out = fe.resample(_dev(x), [1000, 1500], 22050, "ratecv")
    got = _split(out, n_out)
    assert np.array_equal(got[0], R.ratecv(x[:1000], 2, 22050)) and np.array_equal(got[1], R.ratecv(x[1000:], 2, 22050))


# ---- polyphase -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [8000, 11025, 22050, 44100, 48000, 16001])
@pytest.mark.parametrize("kind", ["int16", "float32", "float64", "stereo16"])
def test_polyphase_within_the_summation_bound(fe, rate, kind):
    rng = np.random.default_rng(rate + len(kind))
    lengths = [1200, 0, 517, 1, 300]          # 300 < one workgroup's outputs; first and last outputs of every clip are checked
    h = R.taps(rate)[0]
    if kind == "stereo16":
        frames = [rng.integers(-32768, 32768, size=2 * n).astype("<i2") for n in lengths]
        for f in frames:
            f[:len(f) // 3] = np.where(f[:len(f) // 3] < 0, -32768, 32767)          # saturating sums among them
        pcm = _dev(np.frombuffer(np.concatenate(frames).tobytes(), dtype=np.uint8))
        xs = [R.decode(f.tobytes(), 2, 2).astype(np.float64) for f in frames]
        out, n_out = fe.resample(pcm, lengths, rate, "polyphase", wav_format=(2, 2))
    else:
        dt = {"int16": np.int16, "float32": np.float32, "float64": np.float64}[kind]
        clips = [np.round(rng.normal(0, 8000, size=n)).clip(-32768, 32767).astype(dt) if kind == "int16"
                 else (rng.normal(0, 0.3, size=n)).astype(dt) for n in lengths]
        xs = [c.astype(np.float64) for c in clips]
        out, n_out = fe.resample(_dev(np.concatenate(clips)), lengths, rate, "polyphase")
    got = _split(out, n_out)
    worst = 0.0
    for x, y in zip(xs, got):
        want, mag, K = R.polyphase(x, rate, h=h)
        assert len(y) == len(want) == R.count(R.POLYPHASE, rate, 16000, len(x))
        if len(y) == 0:
            continue
        bound = (K + 18) * 2.0 ** -52 * mag
        err = np.abs(y - want)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        bad = np.nonzero(err > bound)[0]
        assert len(bad) == 0, (rate, kind, len(x), bad[:5], err[bad[:5]], bound[bad[:5]])
    print("polyphase %5d Hz %-8s: worst |gpu - ref| / bound = %.3f" % (rate, kind, worst))


def test_polyphase_long_clip_many_workgroups(fe):
    """A clip of many workgroups (the staged span moves along the clip) and a batch whose clips end in different workgroups."""
    rng = np.random.default_rng(5)
    lengths = [44100, 30011, 22050]
    clips = [np.round(rng.normal(0, 5000, size=n)).astype(np.int16) for n in lengths]
    out, n_out = fe.resample(_dev(np.concatenate(clips)), lengths, 44100, "polyphase")
    h = R.taps(44100)[0]
    for x, y in zip(clips, _split(out, n_out)):
        want, mag, K = R.polyphase(x.astype(np.float64), 44100, h=h)
        assert len(y) == len(want) and (np.abs(y - want) <= (K + 18) * 2.0 ** -52 * mag).all()


# ---- both methods ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["polyphase", "ratecv"])
def test_equal_rates_copy_the_decoded_samples(fe, method):
    rng = np.random.default_rng(3)
    frames = rng.integers(-(1 << 23), 1 << 23, size=2 * 777)
    raw = R.encode(frames, 3)
    out, n_out = fe.resample(_dev(np.frombuffer(raw, dtype=np.uint8)), [400, 377], 16000, method, wav_format=(3, 2))
    assert n_out.tolist() == [400, 377]
    assert np.array_equal(out.cpu().numpy(), R.decode(raw, 3, 2).astype(np.float64))
    if method == "polyphase":
        x = rng.normal(0, 0.25, size=1000)
        out, n_out = fe.resample(_dev(x), [1000], 16000, method)
        assert np.array_equal(out.cpu().numpy(), x)


@pytest.mark.parametrize("method", ["polyphase", "ratecv"])
def test_features_of_a_resampled_batch_equal_features_of_the_uploaded_samples(fe, method):
    rng = np.random.default_rng(8)
    lengths = [44100, 30000, 12345]
    frames = rng.integers(-20000, 20000, size=2 * sum(lengths)).astype("<i2")
    out, n_out = fe.resample(_dev(np.frombuffer(frames.tobytes(), dtype=np.uint8)), lengths, 44100, method, wav_format=(2, 2))
    feat_a, fr_a = fe.features(out, n_out)
    feat_b, fr_b = fe.features(_dev(out.cpu().numpy().copy()), n_out)
    assert np.array_equal(fr_a, fr_b) and torch.equal(feat_a, feat_b)
    assert np.isfinite(feat_a.cpu().numpy()).all()


def test_refusals_leave_the_outputs_untouched(fe):
    from danspeech_amd import _native
    L = _native.lib()
    x16 = _dev(np.arange(-500, 500, dtype=np.int16))
    x64 = _dev(np.linspace(-1, 1, 1000))
    n = np.array([600, 400], dtype=np.int64)
    need = int(fe.resample_count(n, 44100).sum())
    out = torch.full((4096,), SENTINEL, dtype=torch.float64, device="cuda")
    n_out = np.full(2, -99, dtype=np.int64)

    def call(pcm, dtype, rate, method, cap, B=2):
        rc = L.dsmi_resample(fe._h, pcm.data_ptr(), dtype, n.ctypes.data_as(C.c_void_p), B, rate, method, out.data_ptr(), cap,
                             n_out.ctypes.data_as(C.c_void_p), None)
        torch.cuda.synchronize()
        return rc, (L.dsmi_frontend_last_error(fe._h) or b"").decode()

    for args, code, word in [((x16, 0, 0, 0, 4096), -1, "rate_in"), ((x16, 0, -44100, 1, 4096), -1, "rate_in"),
                             ((x16, 0, 44100, 2, 4096), -1, "method"), ((x16, 0, 44100, -1, 4096), -1, "method"),
                             ((x64, 2, 44100, 1, 4096), -1, "ratecv"), ((x16, 0, 44100, 0, need - 1), -8, "out_dev"),
                             ((x16, 0, 44100, 1, 3), -8, "out_dev"), ((x16, 0, 99991, 0, 4096), -8, "DSMI_RESAMPLE_MAX_TAPS"),
                             ((x16, 0, 16000 * 25, 0, 4096), -8, "DSMI_RESAMPLE_MAX_DECIMATION"), ((x16, 16 | 3, 44100, 0, 4096), -1, "stereo"),
                             ((x16, 0, 44100, 0, 4096, 0), -1, "bad")]:
        rc, msg = call(*args)
        assert rc == code and word in msg, (args[1:], rc, msg)
        assert (out == SENTINEL).all().item() and n_out.tolist() == [-99, -99], args[1:]
    rc, msg = call(x16, 0, 44100, 0, need)              # ... and the exact capacity is enough
    assert rc == 0, msg
    assert n_out.tolist() == fe.resample_count(n, 44100).tolist()
    o = out.cpu().numpy()
    assert (o[:need] != SENTINEL).all() and (o[need:] == SENTINEL).all()


def test_audio_resample_function(fe):
    from danspeech_amd import audio
    x = np.round(np.random.default_rng(4).normal(0, 4000, size=4410)).astype(np.int16)
    y = audio.resample(x, 44100)
    want, mag, K = R.polyphase(x.astype(np.float64), 44100)
    assert isinstance(y, np.ndarray) and len(y) == 1600 and (np.abs(y - want) <= (K + 18) * 2.0 ** -52 * mag).all()
    assert np.array_equal(audio.resample(x, 44100, method="ratecv"), R.ratecv(x, 2, 44100))
    yd = audio.resample(_dev(x), 44100)
    assert yd.is_cuda and np.array_equal(yd.cpu().numpy(), y)


# ---- end to end ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rec():
    from danspeech_amd import Recognizer
    from danspeech_amd.deepspeech.model import DeepSpeech
    sd = syn.make_state_dict(2, "gru", 800, 5, seed=0, **syn.TALKATIVE)
    m = DeepSpeech("resample-cfgA", rnn_type="gru", rnn_hidden_size=800, rnn_layers=5, conv_layers=2).load_state_dict(sd)
    return Recognizer(model=m)


def _write_wav(path, frames_i16, nch, rate):
    with wave.open(path, "wb") as w:
        w.setnchannels(nch); w.setsampwidth(2); w.setframerate(rate); w.writeframes(frames_i16.astype("<i2").tobytes())


def _speechlike(rng, n, rate):
    t = np.arange(n) / float(rate)
    x = 2500.0 * rng.standard_normal(n)
    for _ in range(3):
        x += rng.uniform(1000, 4000) * np.sin(2 * np.pi * rng.uniform(100, 3000) * t)
    return np.clip(np.rint(x), -16000, 16000).astype(np.int16)


def _probs(rec, feats, frames):
    eng = rec.danspeech_recognizer
    out, sizes = eng.model(feats, torch.from_numpy(np.asarray(frames).astype(np.int32)))
    torch.cuda.synchronize()
    return out.cpu().numpy(), np.asarray(sizes)


@pytest.mark.parametrize("method", ["polyphase", "ratecv"])
def test_files_and_arrays_of_other_rates_end_to_end(rec, tmp_path, method):
    from danspeech_amd.audio import load_audio
    from danspeech_amd.audio.resources import read_wav_frames_rate
    rng = np.random.default_rng(21)
    paths, decoded, rates = [], [], []
    for i, n in enumerate([88200, 61007, 44100, 70000]):                  # 44.1 kHz stereo int16, 1 .. 2 s
        f = np.stack([_speechlike(rng, n, 44100), _speechlike(rng, n, 44100)], axis=1).reshape(-1)
        paths.append(str(tmp_path / ("s%d.wav" % i))); _write_wav(paths[-1], f, 2, 44100)
        decoded.append(R.decode(f.astype("<i2").tobytes(), 2, 2)); rates.append(44100)
    for i, n in enumerate([16000, 9001, 12500]):                          # 8 kHz mono int16
        f = _speechlike(rng, n, 8000)
        paths.append(str(tmp_path / ("m%d.wav" % i))); _write_wav(paths[-1], f, 1, 8000)
        decoded.append(f.astype(np.int64)); rates.append(8000)
    m = R.RATECV if method == "ratecv" else R.POLYPHASE
    want_audio = [R.resample(x, r, m, width=2) for x, r in zip(decoded, rates)]
    want = rec.recognize_batch(want_audio)
    assert all(len(t) >= 5 for t in want), want
    # files, in shuffled order
    perm = rng.permutation(len(paths))
    got = rec.recognize_files([paths[i] for i in perm], resample=method)
    assert got == [want[i] for i in perm]
    # arrays of one rate
    idx44 = [i for i, r in enumerate(rates) if r == 44100]
    got = rec.recognize_batch([decoded[i].astype(np.float64) for i in idx44], sample_rate=44100, resample=method)
    assert got == [want[i] for i in idx44]
    # probabilities: the 44.1 kHz group through the parser's device path against the host-resampled arrays
    parser = rec.danspeech_recognizer.audio_parser
    order = sorted(idx44, key=lambda i: -len(decoded[i]))
    raws = [read_wav_frames_rate(paths[i])[0] for i in order]
    feats, frames = parser.parse_wav_frames(raws, 2, 2, rate=44100, resample=method)
    p_got, s_got = _probs(rec, feats, frames)
    feats, frames = parser.parse_batch([want_audio[i] for i in order])
    p_want, s_want = _probs(rec, feats, frames)
    assert np.array_equal(s_got, s_want)
    err = max(float(np.abs(p_got[b, :s_want[b]] - p_want[b, :s_want[b]]).max()) for b in range(len(order)))
    print("%s: max |probs(device resample) - probs(host reference resample)| = %.3g" % (method, err))
    assert err < 1e-4
    # without `resample` the header's rate is ignored, as load_audio ignores it
    assert rec.recognize_files(paths) == rec.recognize_batch([load_audio(p) for p in paths])


def _long_recording_48k(seconds=24, seed=33):
    rng = np.random.default_rng(seed)
    n = seconds * 48000
    x = rng.normal(0, 60, n)
    t = 90000
    spans = [(0, 27000)]
    while t < n - 250000:
        dur = int(rng.choice([4500, 12000, 36000, 90000, 210000]))
        spans.append((t, t + dur))
        t += dur + int(rng.choice([9000, 21000, 36000, 75000]))
    for a, b in spans:
        x[a:b] += rng.normal(0, 4000, b - a)
    return np.clip(np.rint(x), -32768, 32767)


@pytest.mark.parametrize("method", ["polyphase", "ratecv"])
def test_recognize_long_at_48k(rec, method):
    from oracle import segmentation as oseg
    x = _long_recording_48k()
    if method == "ratecv":
        ref = R.ratecv(x.astype(np.int64), 2, 48000).astype(np.float64)
    else:
        ref, mag, K = R.polyphase(x, 48000)
        # phrase lists may differ only at a hop whose energy is within the resampling bound of the threshold: none here.
        # |e_gpu - e_ref| <= sqrt(sum (dx)^2 / step) <= max |dx| <= max of the per-sample bound
        _, energies = oseg.segment(ref, energy_threshold=600, step=1024)
        assert np.abs(np.asarray(energies) - 600.0).min() > float(((K + 18) * 2.0 ** -52 * mag).max())
    want = rec.recognize_long(ref, max_batch=4)
    got = rec.recognize_long(x, max_batch=4, sample_rate=48000, resample=method)
    assert len(want) >= 3 and all(b <= len(ref) for _, b, _ in got)
    assert [(a, b) for a, b, _ in got] == [(a, b) for a, b, _ in want]
    assert [t for _, _, t in got] == [t for _, _, t in want]
