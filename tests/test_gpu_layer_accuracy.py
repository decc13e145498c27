"""Every recurrent kernel form against float64, at the layer's own output.

Each case of tests/_layer_cases.py builds a 2-layer model, runs ONE ``BatchRNN`` layer through ``dsmi_rnn_layer`` and compares its
output with tests/_f64_ref.py on the same float32 inputs -- at the shapes the kernels' own predicates name (rnn_plan.h: k-blocks per
wave, tiles per window, tile pairs, the width caps), ragged / equal / one-step batches, three kinds, one and two directions, layer 0
(K = 1312, no BatchNorm) and layer 1, default and saturating (``ih_gain=6``) weights.  ``last_rnn_plan()`` must name the kernel the
case is about for every launch, after any refusal fallback: a case that another kernel ran FAILS.  One handle at a time.

The bound (tests/_layer_cases.py: M; tests/test_layer_accuracy_sensitivity.py: what it would catch):

    max |gpu - float64| <= M[family] * e32,      e32 = max |fp32 oracle - float64| of the same case,
    outputs past a clip's length exactly zero,   recompute_count() == 0.

On failure the message says where the worst element sits: time step, clip and tile, unit, 16-unit group and 32-unit workgroup, inside
the clip or past its length, the error per tile and per group -- a wrong fragment and a wrong hand-off look different there.

``DSMI_RECORD_LAYER_ACCURACY=1`` (or =PATH) rewrites tests/layer_accuracy_measured.json (or PATH) from the run: per case e32, the
GPU's max and RMS error, the ratio and the kernels that ran.  The test asserts against M, never against that file.

The four-wave ring below 224 units runs in a process of its own (see `fresh` in the case table); that child skips the per-device lock
file the parent holds (DSMI_PERSIST_SHARED=1): the parent has nothing on the GPU while it waits.
"""
import json
import os
import subprocess
import sys

import pytest

import _layer_cases as lc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def records():
    from danspeech_amd import _native
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    _native.lib()
    recs = []
    yield recs
    where = os.environ.get("DSMI_RECORD_LAYER_ACCURACY")
    if where:
        path = os.path.join(ROOT, "tests", "layer_accuracy_measured.json") if where == "1" else where
        doc = dict(header=dict(what="tests/test_gpu_layer_accuracy.py on one MI355X: per case the fp32 oracle's max error against float64 (e32), "
                                    "the kernel's max and RMS error against float64, the oracle's RMS error (e32_rms), ratio = gpu_max / e32, and the kernels dsmi_debug_last_rnn_plan named",
                               device_name_torch_reports=torch.cuda.get_device_name(0), M=lc.M,
                               max_ratio={f: max([r["ratio"] for r in recs if r["kernels"] and lc.FAMILY[r["kernels"][0]] == f] or [0.0]) for f in lc.M}),
                   cases=[{k: v for k, v in r.items() if k != "where"} for r in recs])
        with open(path, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


def _in_a_fresh_process(c):
    env = dict(os.environ, DSMI_PERSIST_SHARED="1", **c["env"])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_layer_cases.py"), c["name"]], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):      # the child died on the GPU: nothing more is started on it in this run
        pytest.exit("%s: the case's process ended with %d\n%s" % (c["name"], r.returncode, r.stderr[-3000:]), returncode=3)
    lines = [l for l in r.stdout.splitlines() if l.startswith("RECORD ")]
    assert r.returncode == 0 and lines, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    return json.loads(lines[-1][len("RECORD "):])


@pytest.mark.parametrize("name", [c["name"] for c in lc.CASES])
def test_layer_output_against_float64(records, name):
    c, = [c for c in lc.CASES if c["name"] == name]
    rec = _in_a_fresh_process(c) if c["fresh"] else lc.run_on_gpu(c)
    records.append(rec)
    bound = lc.M[lc.FAMILY[c["kernel"]]] * rec["e32"]
    print("%s: ran %s, e32 %.3g, gpu max %.3g rms %.3g, ratio %.2f (M %g), past the lengths %.3g"
          % (name, "+".join(rec["kernels"]), rec["e32"], rec["gpu_max"], rec["gpu_rms"], rec["ratio"], lc.M[lc.FAMILY[c["kernel"]]], rec["past_len_max"]))
    assert rec["kernels"] and set(rec["kernels"]) == {c["kernel"]}, "the case is about %s, the layer ran %s" % (c["kernel"], rec["kernels"])
    assert c["launches"] is None or len(rec["kernels"]) == c["launches"], rec["kernels"]
    assert rec["x16"] == (c["kernel"] not in ("steps", "persist8"))
    assert rec["recomputed"] == 0
    assert rec["past_len_max"] == 0.0, rec["where"]
    assert rec["gpu_max"] <= bound, "max error %.3g > %g x e32 = %.3g (ratio %.2f).  %s" % (rec["gpu_max"], bound / rec["e32"], bound, rec["ratio"], rec["where"])


def test_every_kernel_form_was_named(records):
    """The table is about all seven RnnKernel values, and every case run so far -- each held to its own kernel above -- is on record
    with the kernels it named.  (Whatever part of the file ran, in whatever order.)"""
    assert sorted({c["kernel"] for c in lc.CASES}) == lc.KERNELS
    by_name = {c["name"]: c for c in lc.CASES}
    for r in records:
        assert r["name"] in by_name and (not r["kernels"] or set(r["kernels"]) <= set(lc.KERNELS)), r
