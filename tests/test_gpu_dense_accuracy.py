"""The dense kernels in front of and behind the recurrent layers against float64, at their own outputs.

Conv stack: each case of tests/_dense_cases.py (CONV_CASES) builds one model of 8 hidden units and one recurrent layer -- only its
conv stack matters --, runs ``dsmi_conv_stack`` and compares with tests/_f64_ref.py's ``conv_stack`` on the same float32 features,
whose values past each clip's length are left in place.  Head: each case of HEAD_CASES builds a 1-layer model and runs ``dsmi_head``
on rows the test supplies, against ``_f64_ref.lookahead`` / ``head``.  One handle at a time.

The bound (tests/_dense_cases.py: M; tests/test_dense_accuracy_sensitivity.py: what it would catch):

    max |gpu - float64| <= M[family] * e32,      e32 = max |fp32 oracle - float64| of the same case,
    the shape equals the reference's,
    conv: outputs at t >= out_len exactly zero; the range-fallback case bit for bit what DSMI_DENSE_MODE=f32 gives;
    head: every row sums to 1 within 1e-6, nothing is NaN, the argmax is the reference's wherever its top-two margin exceeds 1e-4.

On failure the message says where the worst element sits: clip, channel and 32-channel tile, output row and its 4-row / 8-row
workgroup, output step and 64-step tile, inside the clip or past its length, the error per time tile and row group (head: row,
32-row workgroup, class and class tile).

``DSMI_RECORD_DENSE_ACCURACY=1`` (or =PATH) rewrites tests/dense_accuracy_measured.json (or PATH) from the run: per case e32, the GPU's
max and RMS error and the ratio.  The tests assert against M, never against that file.
"""
import json
import os

import pytest

import _dense_cases as dc

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
    where = os.environ.get("DSMI_RECORD_DENSE_ACCURACY")
    if where:
        path = os.path.join(ROOT, "tests", "dense_accuracy_measured.json") if where == "1" else where
        finite = lambda f: [r["ratio"] for r in recs if r["family"] == f and r["ratio"] != float("inf")]
        max_ratio = {f: max(finite(f) or [0.0]) for f in dc.M}
        doc = dict(header=dict(what="tests/test_gpu_dense_accuracy.py on one MI355X: per case the fp32 oracle's max error against float64 (e32), the kernels' "
                                    "max and RMS error against float64, ratio = gpu_max / e32; M_derived = the next power of two at or above twice max_ratio",
                               device_name_torch_reports=torch.cuda.get_device_name(0), M=dc.M, max_ratio=max_ratio,
                               M_derived={f: _next_pow2(2.0 * v) for f, v in max_ratio.items()}),
                   cases=[{k: v for k, v in r.items() if k != "where"} for r in recs])
        with open(path, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


@pytest.mark.parametrize("name", [c["name"] for c in dc.CONV_CASES])
def test_conv_stack_against_float64(records, name):
    c, = [c for c in dc.CONV_CASES if c["name"] == name]
    rec = dc.run_conv_on_gpu(c)
    records.append(rec)
    M = dc.M[c["family"]]
    print("%s: e32 %.3g (rms %.3g), gpu max %.3g rms %.3g, ratio %.2f (M %g), past the lengths %.3g"
          % (name, rec["e32"], rec["e32_rms"], rec["gpu_max"], rec["gpu_rms"], rec["ratio"], M, rec["past_len_max"]))
    assert rec["shape"] == rec["ref_shape"], rec["where"]
    assert rec["past_len_max"] == 0.0, rec["where"]
    if c["weights"] == "range":
        assert rec["same_as_f32"] is True, "a weight of 1000.0 did not send the stack to conv.hip: the output is not DSMI_DENSE_MODE=f32's"
    if name == dc.F32_CONTROL:
        assert rec["same_as_f32"] is False, "the default path gives DSMI_DENSE_MODE=f32's bits: the comparison of the range case shows nothing"
    assert rec["gpu_max"] <= M * rec["e32"], "max error %.3g > %g x e32 = %.3g (ratio %.2f).  %s" % (rec["gpu_max"], M, M * rec["e32"], rec["ratio"], rec["where"])


@pytest.mark.parametrize("name", [c["name"] for c in dc.HEAD_CASES])
def test_head_against_float64(records, name):
    c, = [c for c in dc.HEAD_CASES if c["name"] == name]
    rec = dc.run_head_on_gpu(c)
    records.append(rec)
    M = dc.M["head"]
    print("%s: e32 %.3g, gpu max %.3g rms %.3g, ratio %.2f (M %g), row sums off by %.3g, argmax differs in %d of %d clear rows"
          % (name, rec["e32"], rec["gpu_max"], rec["gpu_rms"], rec["ratio"], M, rec["row_sum_err"], rec["argmax_differs"], rec["clear_rows"]))
    assert rec["shape"] == rec["ref_shape"], rec["where"]
    assert not rec["nan"], rec["where"]
    assert rec["row_sum_err"] <= 1e-6, rec["where"]
    assert rec["argmax_differs"] == 0, rec["where"]
    assert rec["gpu_max"] <= M * rec["e32"], "max error %.3g > %g x e32 = %.3g (ratio %.2f).  %s" % (rec["gpu_max"], M, M * rec["e32"], rec["ratio"], rec["where"])


def test_head_refuses_bad_arguments_before_any_launch():
    """x_rev exactly when the model is bidirectional; 129 labels are refused when the model is made."""
    from danspeech_amd import _native, synthetic as syn
    c = dc.HEAD_CASES[0]
    cfg, sd, ac, x_fwd, x_rev = dc.make_head_case(c)
    m = _native.NativeModel(cfg, sd, audio_conf=ac, n_labels=c["C"])
    try:
        with pytest.raises(_native.DsmiError) as e:
            m.head(torch.from_numpy(x_fwd).cuda())
        assert e.value.code == _native.DSMI_ERR_INVALID and "reverse" in str(e.value)
        L = _native.lib()
        p = torch.empty((c["B"], c["To"], c["C"]), device="cuda")
        xf, xr = torch.from_numpy(x_fwd).cuda(), torch.from_numpy(x_rev).cuda()
        for B, To, a, b, out in ((0, 11, xf, xr, p), (3, 0, xf, xr, p), (3, 11, None, xr, p), (3, 11, xf, xr, None), (1 << 13, 1 << 13, xf, xr, p)):
            ptr = lambda t: None if t is None else t.data_ptr()
            assert L.dsmi_head(m._h, ptr(a), ptr(b), B, To, ptr(out), None) == _native.DSMI_ERR_INVALID
    finally:
        m.close()
    sd = syn.make_state_dict(1, "gru", 8, 1, n_labels=129, seed=1, sample_rate=100, window_size=0.02)
    with pytest.raises(_native.DsmiError):
        _native.NativeModel(dict(cfg, rnn_hidden_size=8), sd, audio_conf=ac, n_labels=129)
    cu = dc.HEAD_CASES[-2]
    assert not cu["bidir"]
    cfg, sd, ac, x_fwd, _ = dc.make_head_case(cu)
    m = _native.NativeModel(cfg, sd, audio_conf=ac, n_labels=cu["C"])
    try:
        with pytest.raises(_native.DsmiError):
            m.head(torch.from_numpy(x_fwd).cuda(), torch.from_numpy(x_fwd).cuda())
    finally:
        m.close()
