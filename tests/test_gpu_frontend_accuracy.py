"""The spectrogram front end (danspeech_amd/csrc/features.hip) against float64, at its own output.

Each case of tests/_frontend_cases.py (CASES) makes its clips, runs ``dsmi_features`` -- once with a front end that does not
normalise, once with one that does -- or the streaming parser's calls, and compares with tests/_f64_ref.py's ``spectrogram`` /
``stream_norm`` on the same sample values.  One handle at a time.

The bound (tests/_frontend_cases.py: M, the regions; tests/test_frontend_accuracy_sensitivity.py: what it would catch), per case
and region:

    max |gpu - float64| <= M[family] * e32,      e32 = max |fp32 oracle - float64| over the same region,
    the frame counts equal the reference's,
    every element at t >= frames of every clip is exactly zero -- in the buffers the cases pre-fill with 7.0 too,
    nothing is NaN,
    streaming: state3 equals the float64 restatement of the parser's update within rtol 1e-6.

An all-zero clip is pinned as it is: its normalisation is 0 / 0, NaN inside its frames as the reference's is, zero past them.

On failure the message says where the worst element sits: clip, frame with its 64-frame workgroup, 16-frame wave tile and 8-frame
group, whether the frame touches the left or right padding, bin with its even / odd tile of sixteen (or bin NH; direct kernel: the
trip of its bin loop), the error per workgroup and per bin tile.

``DSMI_RECORD_FRONTEND_ACCURACY=1`` (or =PATH) rewrites tests/frontend_accuracy_measured.json (or PATH) from the run: per case and
region e32, the GPU's max and RMS error, the ratio, and the M the ratios give.  The tests assert against M, never against that file.
"""
import json
import os

import numpy as np
import pytest

import _frontend_cases as fc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _next_pow2(v):
    p = 1.0
    while p < v:
        p *= 2.0
    while p / 2.0 >= v and p > 2.0 ** -8:
        p /= 2.0
    return p


@pytest.fixture(scope="module")
def records():
    from danspeech_amd import _native
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    _native.lib()
    recs = []
    yield recs
    where = os.environ.get("DSMI_RECORD_FRONTEND_ACCURACY")
    if where:
        path = os.path.join(ROOT, "tests", "frontend_accuracy_measured.json") if where == "1" else where
        ratios = lambda f: [(g["ratio"], r["name"], n) for r in recs if r["family"] == f for n, g in r["regions"].items() if g["ratio"] != float("inf")]
        worst = {f: max(ratios(f) or [(0.0, None, None)]) for f in fc.M}
        doc = dict(header=dict(what="tests/test_gpu_frontend_accuracy.py on one MI355X: per case and region the fp32 oracle's max error against float64 "
                                    "(e32), the front end's max and RMS error against float64, ratio = gpu_max / e32; M_derived = the next power of "
                                    "two at or above twice max_ratio",
                               device_name_torch_reports=torch.cuda.get_device_name(0), M=fc.M, max_ratio={f: w[0] for f, w in worst.items()},
                               max_ratio_at={f: "%s / %s" % w[1:] for f, w in worst.items()},
                               M_derived={f: _next_pow2(2.0 * w[0]) for f, w in worst.items()}),
                   cases=[dict(r, regions={n: {k: v for k, v in g.items() if k != "where"} for n, g in r["regions"].items()}) for r in recs])
        with open(path, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


@pytest.mark.parametrize("name", [c["name"] for c in fc.CASES])
def test_front_end_against_float64(records, name):
    c = fc.BY_NAME[name]
    rec = fc.run_on_gpu(c)
    records.append(rec)
    M = fc.M[c["family"]]
    for region, g in sorted(rec["regions"].items()):
        print("%s / %s: %d elements, e32 %.3g (rms %.3g), gpu max %.3g rms %.3g, ratio %.2f (M %g)"
              % (name, region, g["elements"], g["e32"], g["e32_rms"], g["gpu_max"], g["gpu_rms"], g["ratio"], M))
    print("%s: frames %s, past the frames %s, state3 off by %.3g" % (name, rec["frames"], rec["tail_max"], rec.get("state_rel_err", 0.0)))
    for key, fr in rec["frames"].items():
        assert fr == rec["ref_frames"], "%s output: frame counts %s, the reference's %s" % (key, fr, rec["ref_frames"])
        assert rec["tail_max"][key] == 0.0, "%s output: %g at t >= frames of a clip" % (key, rec["tail_max"][key])
        assert not rec["nan"][key], "%s output: NaN" % key
    if c["api"] != "features":
        assert rec["state_rel_err"] <= 1e-6
    failed = ["%s: max error %.3g > %g x e32 = %.3g (ratio %.2f).  %s" % (region, g["gpu_max"], M, M * g["e32"], g["ratio"], g["where"])
              for region, g in sorted(rec["regions"].items()) if not g["gpu_max"] <= M * g["e32"]]
    assert not failed, "\n".join(failed)


@pytest.mark.parametrize("pad", ["reflect", "constant"])
def test_an_all_zero_clip_is_nan_inside_its_frames_and_zero_past_them(pad):
    """(0 - 0) / 0, as the reference's: pinned so that a change is a decision.  The clip beside it is not touched by it."""
    from danspeech_amd import _native
    import _f64_ref as f64
    c = fc.BY_NAME["mfma-noise-2560"]
    x = fc.make_signal(c, 0, 2560)[1]
    fe = _native.NativeFrontend(fc.audio_conf(c, True), pad_mode=pad)
    try:
        feat, fr = fe.features(torch.from_numpy(np.concatenate([x, np.zeros(800)])).cuda(), np.array([2560, 800], dtype=np.int64))
        feat = feat.cpu().numpy()[:, 0]
    finally:
        fe.close()
    with np.errstate(invalid="ignore"):
        ref = f64.spectrogram(np.zeros(800), 320, 160, "hamming", pad, True)
    assert list(fr) == [17, 6] and ref.shape == (161, 6) and np.isnan(ref).all()
    assert np.isnan(feat[1, :, :6]).all() and not feat[1, :, 6:].any()
    assert not np.isnan(feat[0]).any()
    good = f64.spectrogram(x, 320, 160, "hamming", pad, True)
    assert np.abs(feat[0] - good).max() < 1e-4


def test_stream_frames_of_an_odd_window_length():
    """n_fft 441: a chunk of 440 samples is no frame (the library refuses it), 441 and 660 are one, 661 two."""
    from danspeech_amd import _native
    fe = _native.NativeFrontend(dict(sampling_rate=22050))
    try:
        assert (fe.n_fft, fe.hop, fe.n_freq) == (441, 220, 221)
        assert [fe._stream_frames(n) for n in (440, 441, 660, 661)] == [0, 1, 1, 2]
        state = np.zeros(3)
        with pytest.raises(_native.DsmiError) as e:
            fe.features_stream(torch.zeros(440, dtype=torch.float64).cuda(), state)
        assert e.value.code == _native.DSMI_ERR_INVALID and not state.any()
        assert tuple(fe.features_stream(torch.ones(660, dtype=torch.float64).cuda(), state).shape) == (221, 1)
    finally:
        fe.close()


def test_a_window_too_long_for_the_devices_lds_is_refused_at_creation():
    """192 kHz at 20 ms: n_fft 3840, 307200 bytes of LDS per workgroup of the direct kernel -- refused with the limit named, before
    anything is launched; 44.1 kHz (70560 bytes, above the default 64 KB) is made -- its output is a case of the table."""
    from danspeech_amd import _native
    with pytest.raises(_native.DsmiError) as e:
        _native.NativeFrontend(fc.LDS_REFUSED)
    assert e.value.code == _native.DSMI_ERR_INVALID
    assert "307200" in str(e.value) and "limit" in str(e.value) and "3840" in str(e.value)
    assert any(c["n_fft"] == 882 and c["n_freq"] == 442 for c in fc.CASES)
