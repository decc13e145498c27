"""The streaming passes held to float64 across chunks, per kernel form: dsmi_stream_forward and dsmi_stream_forward_many on every
case of tests/_stream_cases.py (its docstring has the table and the chunk arithmetic) against tests/_f64_ref.py stream_model, with
oracle/streaming.py's own error as the unit.  One model handle at a time.

The bound (tests/_stream_cases.py: M; tests/test_stream_accuracy_sensitivity.py: what it would catch):

    outputs and None rounds are where the references have them, with the same frame counts (and where the chunk arithmetic says),
    max |gpu - float64| <= M[family] * e32,      e32 = max |fp32 oracle - float64| over the case's whole schedule,
    last_rnn_plan() after every call names the case's kernel (persist8 or steps) and no other,
    recompute_count() == 0.

On failure the message says where the worst element sits: session with its tile of 32 and position in the tile, round and chunk,
frame and whether it came from carried lookahead rows or the chunk's new ones, class, and the error per round and per session.

``DSMI_RECORD_STREAM_ACCURACY=1`` (or =PATH) rewrites tests/stream_accuracy_measured.json (or PATH) from the run: per case e32, the
GPU's max error, the ratio and the kernels that ran.  The tests assert against M, never against that file.
"""
import json
import os

import pytest

import _stream_cases as sc

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
    where = os.environ.get("DSMI_RECORD_STREAM_ACCURACY")
    if where:
        path = os.path.join(ROOT, "tests", "stream_accuracy_measured.json") if where == "1" else where
        finite = lambda f: [r["ratio"] for r in recs if r["family"] == f and r["ratio"] != float("inf")]
        max_ratio = {f: max(finite(f) or [0.0]) for f in sc.M}
        doc = dict(header=dict(what="tests/test_gpu_stream_accuracy.py on one MI355X: per case the fp32 oracle's max error against float64 over the whole "
                                    "schedule (e32), the GPU's max error against float64, ratio = gpu_max / e32, the kernels last_rnn_plan() named; "
                                    "M_derived = the next power of two at or above twice max_ratio",
                               device_name_torch_reports=torch.cuda.get_device_name(0), M=sc.M, max_ratio=max_ratio,
                               M_derived={f: _next_pow2(2.0 * v) for f, v in max_ratio.items()}),
                   cases=[{k: v for k, v in r.items() if k != "where"} for r in recs])
        with open(path, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


@pytest.mark.parametrize("name", [c["name"] for c in sc.CASES])
def test_stream_against_float64(records, name):
    c, = [c for c in sc.CASES if c["name"] == name]
    rec = sc.run_on_gpu(c)
    records.append(rec)
    M = sc.M[c["family"]]
    print("%s: %s, %d frames, e32 %.3g, gpu max %.3g, ratio %.2f (M %g), recomputed %d"
          % (name, rec["kernels"], rec["frames"], rec["e32"], rec["gpu_max"], rec["ratio"], M, rec["recomputed"]))
    assert rec["frames_as_reference"], rec["where"]
    assert rec["kernels"] == [c["kernel"]], "the recurrent layers ran on %s, the case is about %s" % (rec["kernels"], c["kernel"])
    if c["kernel"] == "persist8":      # one launch per layer: direction 0, one direction, every lane slot of the gate, a CU per workgroup
        assert rec["persist8_launches"] == [[False, 1, 0, 1, "lane", 0, 4, (c["H"] + 7) // 8]], rec["persist8_launches"]
    assert rec["recomputed"] == 0, "%d passes timed out and were recomputed per step" % rec["recomputed"]
    assert rec["e32"] > 0
    assert rec["gpu_max"] <= M * rec["e32"], "max error %.3g > %g x e32 = %.3g (ratio %.2f).  %s" % (rec["gpu_max"], M, M * rec["e32"], rec["ratio"], rec["where"])
