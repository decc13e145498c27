"""The front end's bound of tests/test_gpu_frontend_accuracy.py, ``max |gpu - float64| <= M * e32`` per case and region
(tests/_frontend_cases.py), shown on the CPU to see what it claims to see -- and where it does not --, and the conditions the case
table promises (quiet and loud shares of the tone cases, deterministic generators, every code path of features.hip behind a named
case).

The emulation is oracle/features.py's ladder restated with hooks (``emulate``; with no hook it IS the fp32 oracle, bit for bit, so
the clean emulation sits at 1 x e32 by construction).  M is 4 for all three families -- the front end measures 0.63 .. 1.20 x e32 on the
MI355X (_frontend_cases.py) --, so a mutant is SEEN where it lies above ``2 * M * e32 = 8 x e32``.  The cases: the tone under the
Hann window (mfma-tone-hann, 18 frames: regions raw, quiet, loud, norm), the 65-frame noise clip (mfma-noise-10240), the 2-frame
noise clip (mfma-noise-161) and a 10 s noise clip that is not in the GPU table.  As measured (multiples of the region's e32):

  SEEN (asserted above 2 * M * e32)
  tap NQ dropped (taps 80 and 240 of every frame zero)        tone raw 7.9e5, quiet 1.5e7; noise raw 5.3e6
  samples cut to 14 mantissa bits (the split-fp16 form)       tone raw 1.2e3, quiet 2.3e4; noise raw 1.8e4
  edge-repeating pad instead of reflect                       tone raw 8.1e6; noise raw 8.2e6
  float32-accumulated DFT                                     tone QUIET 173; noise raw 114 (2 frames: 37; 10 s: 374)
  population std instead of unbiased (normalised output)      2 frames 8.9e3; tone, 18 frames 2.6e3; 65 frames 307; 10 s 25
  periodic window instead of symmetric                        tone raw 2.4e5, quiet 4.5e6; noise raw 7.1e6; 2 frames 8.2e5

  NOT SEEN, or not to be relied on
  float32-accumulated DFT on the tone outside the quiet region   loud 5.2, norm 6.6: below 8; whole raw output 9.1: at the edge, and
                                                                 the low bits of a float32 matrix product are the BLAS's -- not asserted
  population std on the un-normalised output                     1.0: not a mutant there

The float32-accumulated DFT is the reason the quiet region has an e32 of its own: the loud bins set the whole output's e32 (1.7e-7)
and the mutant's 1.6e-6 in a quiet bin is 9 x that, but 173 x the quiet region's 9e-9.  The population std is the reason the
normalised comparison uses short clips: sqrt(n / (n - 1)) - 1 is 1.6e-3 at the 322 values of two frames and 3e-6 at a 10 s clip's
161161, where it is 25 x e32 -- still above 8, by a factor of three instead of a thousand.
"""
import numpy as np
import pytest

import _f64_ref as f64
import _frontend_cases as fc
from oracle import features as of


def _cut14(fr):
    """every windowed sample cut to 14 mantissa bits"""
    m, e = np.frexp(fr)
    return np.ldexp(np.round(m * 2.0 ** 14) / 2.0 ** 14, e)


def _drop_nq(fr):
    fr = fr.copy()
    n = fr.shape[0]
    fr[n // 4] = 0.0
    fr[n - n // 4] = 0.0
    return fr


def _periodic(name, n):
    return f64.sym_window(name, n + 1)[:n]


def emulate(c, v, normalize, pad=None, window=None, frames=None, dft32=False, ddof=1):
    """oracle/features.py: spectrogram on one clip, with the mutants' hooks: the padding mode, the window table, a function of the
    windowed frames [n_fft, T], a float32-accumulated transform, the std's degrees of freedom."""
    n_fft, hop = c["n_fft"], c["hop"]
    y = f64.samples_f64(v)
    yp = y if c["pad"] == "none" else np.pad(y, n_fft // 2, mode=pad or c["pad"])
    T = 1 + (len(yp) - n_fft) // hop
    idx = np.arange(n_fft)[:, None] + hop * np.arange(T)[None, :]
    fr = yp[idx] * (window or of.window_sym)(c["window"], n_fft)[:, None]
    if frames is not None:
        fr = frames(fr)
    if dft32:
        ang = 2.0 * np.pi * ((np.arange(c["n_freq"])[:, None] * np.arange(n_fft)[None, :]) % n_fft) / n_fft
        f32 = fr.astype(np.float32)
        D = (np.cos(ang).astype(np.float32) @ f32) - 1j * (np.sin(ang).astype(np.float32) @ f32)
        assert D.dtype == np.complex64
    else:
        D = np.fft.rfft(fr, axis=0).astype(np.complex64)
    spect = np.log1p(np.abs(D)).astype(np.float32)
    if normalize:
        mean = np.float32(spect.mean(dtype=np.float64))
        std = np.float32(spect.std(dtype=np.float64, ddof=ddof))
        spect = ((spect - mean) / std).astype(np.float32)
    return spect


MUTANTS = {
    "tap NQ dropped": dict(frames=_drop_nq),
    "samples cut to 14 mantissa bits": dict(frames=_cut14),
    "edge-repeating pad": dict(pad="edge"),
    "float32-accumulated DFT": dict(dft32=True),
    "population std": dict(ddof=0),
    "periodic window": dict(window=_periodic),
}
LONG = fc._case("mfma-noise-160000", "mfma", [160000])       # a 10 s clip: not in the GPU table, the same generator makes it


def _figures(c, mutants):
    """{(mutant, region): error / e32}, {region: e32}"""
    fed, values = fc.make_case(c)
    R = fc.references(c, values)
    out, e32s = {}, {}
    for region, (src, masks) in sorted(fc.regions(c, R).items()):
        e32s[region] = fc.region_error(R["o_" + src], R[src], masks)[0]
        clean = fc.region_error([emulate(c, v, src == "norm") for v in values], R[src], masks)[0]
        assert clean == e32s[region]
        for m in mutants:
            err = fc.region_error([emulate(c, v, src == "norm", **MUTANTS[m]) for v in values], R[src], masks)[0]
            out[m, region] = err / e32s[region]
            print("%-22s %-8s %-34s %.3g = %.3g x e32" % (c["name"], region, m, err, out[m, region]))
    return out, e32s


@pytest.fixture(scope="module")
def figures():
    return {c["name"]: _figures(c, list(MUTANTS))[0] for c in (fc.BY_NAME["mfma-tone-hann"], fc.BY_NAME["mfma-noise-10240"], fc.BY_NAME["mfma-noise-161"], LONG)}


SEEN = [("tap NQ dropped", "mfma-tone-hann", "raw"), ("tap NQ dropped", "mfma-tone-hann", "quiet"), ("tap NQ dropped", "mfma-noise-10240", "raw"),
        ("samples cut to 14 mantissa bits", "mfma-tone-hann", "raw"), ("samples cut to 14 mantissa bits", "mfma-tone-hann", "quiet"),
        ("samples cut to 14 mantissa bits", "mfma-noise-10240", "raw"),
        ("edge-repeating pad", "mfma-tone-hann", "raw"), ("edge-repeating pad", "mfma-noise-10240", "raw"),
        ("float32-accumulated DFT", "mfma-tone-hann", "quiet"), ("float32-accumulated DFT", "mfma-noise-10240", "raw"),
        ("float32-accumulated DFT", "mfma-noise-161", "raw"),
        ("population std", "mfma-noise-161", "norm"), ("population std", "mfma-tone-hann", "norm"), ("population std", "mfma-noise-10240", "norm"),
        ("population std", "mfma-noise-160000", "norm"),
        ("periodic window", "mfma-tone-hann", "quiet"),
        ("periodic window", "mfma-tone-hann", "raw"), ("periodic window", "mfma-noise-10240", "raw"), ("periodic window", "mfma-noise-161", "raw")]


@pytest.mark.parametrize("mutant,case,region", SEEN)
def test_the_bound_sees(figures, mutant, case, region):
    assert figures[case][mutant, region] > 2 * fc.M["mfma"], figures[case][mutant, region]


def test_the_quiet_region_is_why_a_float32_transform_is_seen_on_the_tone(figures):
    """Over the whole output the float32-accumulated DFT is a few e32 on the tone -- the loud bins set e32 --; in the quiet region it
    is more than ten times as far out."""
    f = figures["mfma-tone-hann"]
    assert f["float32-accumulated DFT", "quiet"] > 10 * f["float32-accumulated DFT", "raw"]
    assert f["float32-accumulated DFT", "quiet"] > 10 * f["float32-accumulated DFT", "loud"]
    assert max(f["float32-accumulated DFT", r] for r in ("raw", "loud", "norm")) < 64


def test_the_population_std_fades_with_the_clips_length(figures):
    """(sqrt(n / (n - 1)) - 1) of values around 1: 1.6e-3 at 322 values, 3e-6 at 161161 -- why the normalised comparison uses short clips."""
    assert figures["mfma-noise-161"]["population std", "norm"] > 20 * figures["mfma-noise-160000"]["population std", "norm"]
    assert all(figures[n]["population std", "raw"] == 1.0 for n in figures)         # not a mutant of the un-normalised output


def test_the_emulation_without_hooks_is_the_oracle():
    for name in ("mfma-tone-blackman", "direct-22050-constant", "stream-many-noise", "mfma-hop240"):
        c = fc.BY_NAME[name]
        for v in fc.make_case(c)[1]:
            for normalize in (False, True):
                ref = of.spectrogram(f64.samples_f64(v), c["rate"], fc.WINDOW_SIZE, c["stride"], normalize, c["pad"], c["window"])
                assert np.array_equal(emulate(c, v, normalize), ref, equal_nan=True)


# ---- the conditions of the case table ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in fc.CASES if c["signal"] == "tone"])
def test_tone_cases_are_mostly_quiet_and_have_loud_bins(name):
    c = fc.BY_NAME[name]
    quiet, loud = fc.tone_shares(fc.references(c, fc.make_case(c)[1]))
    print("%s: %.1f %% of the float64 reference below %g, %.1f %% at or above 1" % (name, 100 * quiet, fc.QUIET, 100 * loud))
    assert quiet >= 0.50 and loud >= 0.02


def test_generators_are_deterministic_and_references_finite():
    for c in fc.CASES:
        a, b = fc.make_case(c), fc.make_case(c)
        for x, y in zip(a[0] + a[1], b[0] + b[1]):
            assert x == y if isinstance(x, bytes) else (x.dtype == y.dtype and np.array_equal(x, y)), c["name"]
        R = fc.references(c, a[1])
        keys = ("raw", "o_raw") + (("norm", "o_norm") if c["norm"] else ())
        assert all(np.isfinite(r).all() for k in keys for r in R[k]), c["name"]
        for region, (src, masks) in fc.regions(c, R).items():
            e32 = fc.region_error(R["o_" + src], R[src], masks)[0]
            assert 0 < e32 < 1e-5, (c["name"], region, e32)


def test_table_covers_what_it_says():
    has = lambda **kw: any(all(c[k] == v for k, v in kw.items()) for c in fc.CASES)
    frames = lambda c: [fc.frame_count(c, N) for N in c["lens"]]
    for N, fr in ((161, 2), (2559, 16), (2560, 17), (10239, 64), (10240, 65)):
        assert has(family="mfma", lens=[N], signal="noise", dtype="f64", window="hamming", pad="reflect") and fc.frame_count(fc.BY_NAME["mfma-noise-%d" % N], N) == fr
    for w in f64.WINDOWS:       # the four windows of dsmi_frontend_create, on the tone and on the 65-frame noise clip
        assert has(family="mfma", window=w, signal="tone") and has(family="mfma", window=w, signal="noise", lens=[10240])
    for d in ("f32", "i16"):    # stft_mfma_kernel<320, float> and <320, int16_t>, centred and with PAD_NONE
        assert has(family="mfma", dtype=d) and has(family="stream", n_fft=320, dtype=d, api="stream") and has(family="stream", n_fft=320, dtype="i16", api="stream_many")
    for p in ("reflect", "constant"):       # constant padding with more than one clip; t_stride past the frames into 7.0
        assert has(family="mfma", lens=[10240, 2721, 161], pad=p, t_stride=70)
    assert has(pad="constant", lens=[1, 159, 160])
    assert has(family="mfma", hop=80) and has(family="mfma", hop=240)
    for rate, n_fft, n_freq in ((8000, 160, 81), (22050, 441, 221), (32000, 640, 321), (100, 2, 2), (44100, 882, 442)):
        cs = [c for c in fc.CASES if c["family"] == "direct" and c["rate"] == rate and c["signal"] == "noise"]
        assert cs and all((c["n_fft"], c["n_freq"]) == (n_fft, n_freq) for c in cs)
        got = {f for c in cs for f in frames(c)} | {f for c in fc.CASES if c["family"] == "stream" and c["rate"] == rate for f in frames(c)}
        assert got >= {1, 8, 9}, (rate, got)          # FT = 8 frames per workgroup
    assert 80 * 882 > 64 * 1024 and 80 * int(fc.LDS_REFUSED["sampling_rate"] * fc.WINDOW_SIZE) == 307200
    assert {c["wav"] for c in fc.CASES if c["wav"]} == {(1, 1), (3, 1), (4, 1), (2, 2), (3, 2), (4, 2)}
    assert all(c["n_fft"] == 320 and c["family"] == "direct" for c in fc.CASES if c["wav"])
    assert sorted(frames(fc.BY_NAME["stream-noise-f64"])) == [1, 1, 2, 64, 65]
    for s in ("noise", "tone"):
        assert frames(fc.BY_NAME["stream-many-" + s]) == [65, 1, 17] and fc.BY_NAME["stream-many-" + s]["t_stride"] > 65
    assert has(family="stream", rate=22050, api="stream_many")          # odd n_fft: NativeFrontend._stream_frames
    # every clip that is handed over with a pitch of its own leaves frames to zero
    assert all(c["t_stride"] > max(frames(c)) for c in fc.CASES if c["t_stride"])
    # the comb walks an impulse over every tap
    c = fc.BY_NAME["mfma-comb"]
    x = np.pad(fc.make_case(c)[1][0], 160, mode="reflect")
    taps = set()
    for t in range(frames(c)[0]):
        taps |= set(np.flatnonzero(x[160 * t:160 * t + 320]).tolist())
    assert taps == set(range(320))


def test_float64_windows_are_scipys():
    import scipy.signal.windows as W
    for name in f64.WINDOWS:
        for n in (2, 160, 320, 441, 882):
            np.testing.assert_allclose(f64.sym_window(name, n), getattr(W, name)(n), rtol=0, atol=1e-15)
            np.testing.assert_allclose(of.window_sym(name, n), getattr(W, name)(n), rtol=0, atol=1e-15)


def test_stream_norm_is_the_oracle_parsers_update():
    """_f64_ref.stream_norm against oracle/streaming.py's StreamingParser over twelve chunks (alpha crosses 1.0 at the tenth)."""
    from oracle import streaming as ost
    p = ost.StreamingParser()
    state = np.zeros(3)
    rng = np.random.default_rng(3)
    for k in range(12):
        y = np.round(rng.normal(0, 3000, 320 + 160 * int(rng.integers(1, 40))))
        p.buffer = None
        got = p.parse_audio(y)
        raw = f64.spectrogram(y, 320, 160, "hamming", "none", False)
        state, mean, std = f64.stream_norm((raw.mean(), raw.std()), state)
        np.testing.assert_allclose(state, [p.input_mean, p.input_std, p.alpha], rtol=1e-6)
        assert np.abs(got - (raw - mean) / std).max() < 1e-5
