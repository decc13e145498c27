"""Sample-rate conversion, the host side (no GPU): the numpy reference of tests/_resample_ref.py against the reference's own
results (tests/golden/g13_ratecv.npz, made by tools/gen_golden_resample.py from ``AudioData.get_array_data(convert_rate=16000)``),
against ``audioop.ratecv`` and ``scipy.signal.resample_poly`` where they import, and the host-only entry points of the library
(``dsmi_resample_count``, ``dsmi_resample_taps``, the refusals that need no device) against that reference."""
import ctypes as C
import os
import wave

import numpy as np
import pytest

import _resample_ref as R

RATES = (8000, 11025, 16001, 22050, 32000, 44100, 48000, 96000)


def _cases(golden):
    g = golden("g13_ratecv")
    for c in range(int(g["n_cases"])):
        width, nch, rate = (int(v) for v in g["fmt_%d" % c])
        yield c, g["raw_%d" % c].tobytes(), width, nch, rate, g["out_%d" % c]


def test_golden_covers_what_it_should(golden):
    fmts = [(w, ch, r, len(raw) // (w * ch)) for _, raw, w, ch, r, _ in _cases(golden)]
    assert {(w, ch) for w, ch, _, _ in fmts} >= {(1, 1), (2, 1), (3, 1), (4, 1), (2, 2), (3, 2), (4, 2)}
    assert any(r < 16000 for _, _, r, _ in fmts) and any(r > 16000 for _, _, r, _ in fmts)
    assert any(np.gcd(r, 16000) == 1 for _, _, r, _ in fmts)
    assert {1, 2} <= {n for _, _, _, n in fmts}
    sat = 0
    for _, raw, w, ch, _, _ in _cases(golden):
        if ch == 2:
            x = R.decode(raw, w, 1)
            s = x[0::2] + x[1::2]
            sat += int(((s < -(1 << (8 * w - 1))) | (s > (1 << (8 * w - 1)) - 1)).sum())
    assert sat > 100          # full-scale frames whose stereo sum saturates


def test_reference_ratecv_equals_the_golden_cases(golden):
    for c, raw, width, nch, rate, want in _cases(golden):
        got = R.ratecv(R.decode(raw, width, nch), width, rate)
        assert len(got) == len(want) == R.count(R.RATECV, rate, 16000, len(raw) // (width * nch)), c
        assert np.array_equal(R.as_reference_array(got, width), want), c


def test_reference_ratecv_equals_audioop():
    audioop = pytest.importorskip("audioop")
    rng = np.random.default_rng(0)
    for width in (1, 2, 3, 4):
        lim = 1 << (8 * width - 1)
        for rate in RATES:
            for n in (0, 1, 2, 5, 4096, 44101):
                x = rng.integers(-lim, lim, size=n)
                raw = R.encode(x, width)
                if width == 1:
                    raw = audioop.bias(raw, 1, -128)            # AudioData.get_raw_data's order: bias, then ratecv
                out, _ = audioop.ratecv(raw, width, 1, rate, 16000, None)
                want = np.frombuffer(out, dtype=np.int8).astype(np.int64) if width == 1 else R.decode(out, width)
                got = R.ratecv(x, width, rate)
                assert len(got) == len(want) and np.array_equal(got, want), (width, rate, n)


def test_reference_polyphase_agrees_with_scipy():
    """Every output within (K + 18) 2^-52 sum_k |x[k] h[...]| of scipy.signal.resample_poly: K + 2 for two float64 sums of K
    terms in different orders, 16 for two filters made by different code (see the tap test below)."""
    sig = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(1)
    for rate in (8000, 11025, 22050, 44100, 48000):
        x = np.round(rng.normal(0, 1e4, 3000))
        y, mag, K = R.polyphase(x, rate)
        up, down = R.ratio(rate, 16000)
        want = sig.resample_poly(x, up, down)
        assert len(want) == len(y) == R.count(R.POLYPHASE, rate, 16000, len(x))
        bound = (K + 18) * 2.0 ** -52 * mag
        worst = float((np.abs(y - want) / np.maximum(bound, 1e-300)).max())
        print("%d Hz: max |ref - scipy| = %.3g, worst share of the bound %.3f" % (rate, np.abs(y - want).max(), worst))
        assert (np.abs(y - want) <= bound).all(), rate


@pytest.fixture(scope="module")
def L():
    from danspeech_amd import _native
    return _native.lib()


def test_count_equals_the_reference(L):
    lengths = list(range(51)) + [4096, 44101, 160000, 1 << 31, (1 << 40) + 7]
    for rate in RATES:
        for method in (R.POLYPHASE, R.RATECV):
            for n in lengths:
                assert L.dsmi_resample_count(method, rate, 16000, n) == R.count(method, rate, 16000, n), (method, rate, n)
    assert L.dsmi_resample_count(R.RATECV, 16000, 16000, 12345) == 12345 == L.dsmi_resample_count(R.POLYPHASE, 16000, 16000, 12345)
    for bad in ((2, 44100, 16000, 10), (0, 0, 16000, 10), (0, 44100, -1, 10), (1, 44100, 16000, -1)):
        assert L.dsmi_resample_count(*bad) < 0, bad


def test_taps_equal_numpy_within_16_ulp_of_the_largest_tap(L):
    """One rounding each for sin, the Bessel ratio, the products and the normalising sum, doubled: 2^-48 max|h|."""
    from danspeech_amd import _native
    for rate in RATES:
        want, up, down = R.taps(rate)
        got, up2, down2 = _native.resample_taps(rate, 16000)
        assert (up2, down2) == (up, down) and len(got) == len(want) == 20 * max(up, down) + 1
        err = float(np.abs(got - want).max())
        print("%d Hz: up %d down %d, %d taps, max |C - numpy| = %.3g = %.3f of the bound" % (rate, up, down, len(got), err, err / (2.0 ** -48 * np.abs(want).max())))
        assert err <= 2.0 ** -48 * np.abs(want).max(), rate
        assert np.array_equal(got, got[::-1]) or np.abs(got - got[::-1]).max() <= 2.0 ** -48 * np.abs(want).max()


def test_taps_agree_with_firwin():
    sig = pytest.importorskip("scipy.signal")
    for rate in (8000, 11025, 44100, 48000):
        h, up, down = R.taps(rate)
        want = sig.firwin(len(h), 1.0 / max(up, down), window=("kaiser", 5.0)) * up
        assert np.abs(h - want).max() <= 2.0 ** -48 * np.abs(want).max(), rate


def test_host_side_refusals(L):
    up, down = C.c_int(-7), C.c_int(-7)
    h = np.full(64, 7.0)
    # rates that are not positive
    assert L.dsmi_resample_taps(0, 16000, None, 0, C.byref(up), C.byref(down)) == -1
    assert L.dsmi_resample_taps(44100, 0, None, 0, C.byref(up), C.byref(down)) == -1
    assert b"positive" in L.dsmi_frontend_last_error(None)
    # the cap on the filter: 16001 -> 16000 is 320 021 taps (admitted), 99991 -> 16000 two million (refused)
    assert L.dsmi_resample_taps(16001, 16000, None, 0, C.byref(up), C.byref(down)) == 0 and (up.value, down.value) == (16000, 16001)
    up.value = down.value = -7
    assert L.dsmi_resample_taps(99991, 16000, None, 0, C.byref(up), C.byref(down)) == -8
    assert b"DSMI_RESAMPLE_MAX_TAPS" in L.dsmi_frontend_last_error(None)
    # decimation above the cap
    assert L.dsmi_resample_taps(16000 * 25, 16000, None, 0, C.byref(up), C.byref(down)) == -8
    # a taps buffer that is too small: nothing written
    assert L.dsmi_resample_taps(48000, 16000, h.ctypes.data_as(C.c_void_p), 60, C.byref(up), C.byref(down)) == -8
    assert (up.value, down.value) == (-7, -7) and (h == 7.0).all()
    assert L.dsmi_resample_taps(48000, 16000, h.ctypes.data_as(C.c_void_p), 61, C.byref(up), C.byref(down)) == 0
    assert (up.value, down.value) == (1, 3) and (h[:61] != 7.0).all() and (h[61:] == 7.0).all()
    # a null handle
    n = np.array([4], dtype=np.int64)
    assert L.dsmi_resample(None, None, 0, n.ctypes.data_as(C.c_void_p), 1, 44100, 0, None, 0, None, None) == -1


def test_read_wav_frames_rate_counts_seconds_at_the_files_rate(tmp_path):
    from danspeech_amd.audio.resources import read_wav_frames_rate, read_wav_frames
    x = (np.arange(44100 * 2) % 30000).astype("<i2")
    p = str(tmp_path / "a.wav")
    with wave.open(p, "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(44100); w.writeframes(x.tobytes())
    raw, width, nch, rate = read_wav_frames_rate(p)
    assert (width, nch, rate) == (2, 2, 44100) and raw == x.tobytes() == read_wav_frames(p)[0]
    raw, _, _, _ = read_wav_frames_rate(p, duration=0.5, offset=0.25)
    assert raw == x[2 * 11025:2 * (11025 + 22050)].tobytes()
    raw, _, _, _ = read_wav_frames_rate(p, offset=0.9)
    assert raw == x[2 * 39690:].tobytes()
    assert read_wav_frames_rate(p, offset=5.0)[0] == b""


def test_surface_keeps_its_defaults():
    """The new arguments are optional and default to today's behaviour."""
    import inspect
    from danspeech_amd import Recognizer
    from danspeech_amd.audio.parsers import SpectrogramAudioParser
    sig = inspect.signature
    assert sig(Recognizer.recognize_files).parameters["resample"].default is None
    assert sig(Recognizer.recognize_batch).parameters["sample_rate"].default is None
    assert sig(Recognizer.recognize_long).parameters["sample_rate"].default is None
    assert sig(SpectrogramAudioParser.parse_wav_frames).parameters["rate"].default is None
    assert os.path.exists(os.path.join(os.path.dirname(__file__), "golden", "g13_ratecv.npz"))
