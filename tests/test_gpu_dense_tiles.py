"""Tiles by demand (csrc/dense_tiles.h) change which workgroup computes a tile and when, never what it computes: the
x-projection and the output of `dsmi_rnn_layer`, the output of `dsmi_conv_stack` and the probabilities of a small `dsmi_forward`
must be EQUAL, bit for bit, between a process with DSMI_DENSE_TILES=0 (every XCD an equal, fixed share of the tiles) and one
with the default.  The switch is read once per process, so each arm is a fresh child process (this file, run as a script);
DSMI_DENSE_TOKENS=0 in both, so that the two handles of the last case really run side by side.

Every shape runs twice in a row on one handle: the second launch finds the counters as the first one's last workgroup left them.
That the two arms are two forms of the kernel, not one run twice, is asserted on the workgroups each x-projection GEMM was launched
with (`dsmi_debug_xproj`): one per tile, rounded up to eight, in the static order; min(tiles, 2 x CUs) by demand.

  GRU layer 1 (K = H), B x To:
    H = 40,  3 x 5     one tile: fewer tiles than XCDs; ragged M, N and K
    H = 168, 16 x 24   eight n-tiles: the last pair holds a real second n-tile; 3 m-tiles x 4 pairs
    H = 800, 16 x 320  40 m-tiles x 19 pairs = 760 tiles on at most 512 workgroups: workgroups loop, shares are stolen
  GRU layer 0 (K = 1312, the row-major A operand) at H = 40
  conv stacks: 2 layers, B = 3, T = 70, one clip short enough for a fully masked time tile; 3 layers, B = 2, T = 130
  a whole forward (the GEMM that reads the conv layout) at H = 40
  two handles on two streams at once (two threads), H = 168: the counters are per handle
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LAYER_CASES = [  # name, H, layer, B, To, lens
    ("h40", 40, 1, 3, 5, [5, 4, 2]),
    ("h40_layer0", 40, 0, 3, 5, [5, 5, 3]),
    ("h168", 168, 1, 16, 24, [24] * 5 + [20] * 6 + [11] * 4 + [3]),
    ("h800", 800, 1, 16, 320, [320] * 4 + [301] * 6 + [255] * 5 + [97]),
]
CONV_CASES = [("conv2", 2, 3, 70, [70, 64, 9]), ("conv3", 3, 2, 130, [130, 101])]


def _model(H, conv_layers=2, seed=5):
    from danspeech_amd import _native, synthetic as syn
    cfg = dict(conv_layers=conv_layers, rnn_type="gru", rnn_hidden_size=H, rnn_layers=2, bidirectional=True, context=20)
    return _native.NativeModel(cfg, syn.make_state_dict(conv_layers, "gru", H, 2, seed=seed))


def _xproj(m):
    import ctypes as C
    from danspeech_amd import _native
    buf = np.empty(1 << 25, dtype=np.float32)
    rows, cols, wgs = C.c_int32(), C.c_int32(), C.c_int32()
    m._check(_native.lib().dsmi_debug_xproj(m._h, _native._np_ptr(buf), buf.size, C.byref(rows), C.byref(cols), C.byref(wgs)))
    return buf[:rows.value * cols.value].reshape(rows.value, cols.value).copy(), wgs.value


def _layer_twice(m, layer, x, lens, out, name):
    for rep in range(2):
        y = m.rnn_layer(layer, x, np.array(lens, dtype=np.int32))
        out["%s/y%d" % (name, rep)] = y.cpu().numpy()
        out["%s/xp%d" % (name, rep)], out["%s/wgs%d" % (name, rep)] = _xproj(m)


def _child(path):
    import threading
    import torch
    out = {}
    rng = np.random.default_rng(17)
    models = {}
    for name, H, layer, B, To, lens in LAYER_CASES:
        m = models.get(H) or models.setdefault(H, _model(H))
        I = 1312 if layer == 0 else H
        x = torch.from_numpy(rng.standard_normal((To, B, I)).astype(np.float32)).cuda()
        _layer_twice(m, layer, x, lens, out, name)
    for name, cl, B, T, lens in CONV_CASES:
        m = _model(40, conv_layers=cl, seed=7)
        feat = torch.from_numpy(rng.standard_normal((B, 1, 161, T)).astype(np.float32)).cuda()
        for rep in range(2):
            out["%s/y%d" % (name, rep)] = m.conv_stack(feat, np.array(lens, dtype=np.int32)).cpu().numpy()
        m.close()
    feat = torch.from_numpy(rng.standard_normal((3, 1, 161, 70)).astype(np.float32)).cuda()
    for rep in range(2):
        out["forward/y%d" % rep] = models[40].forward(feat, np.array([70, 64, 9], dtype=np.int32))[0].cpu().numpy()
    # two handles, each on a stream and a thread of its own, three layers each
    pair = [models[168], _model(168, seed=9)]
    xs = [torch.from_numpy(rng.standard_normal((24, 16, 168)).astype(np.float32)).cuda() for _ in pair]
    torch.cuda.synchronize()
    errors = []

    def work(k):
        try:
            with torch.cuda.stream(torch.cuda.Stream()):
                for rep in range(3):
                    y = pair[k].rnn_layer(1, xs[k], np.array(LAYER_CASES[2][5], dtype=np.int32))
                    out["pair%d/y%d" % (k, rep)] = y.cpu().numpy()
                    out["pair%d/xp%d" % (k, rep)], out["pair%d/wgs%d" % (k, rep)] = _xproj(pair[k])
        except Exception as e:      # noqa: BLE001 (reported by the parent)
            errors.append(repr(e))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for m in list(models.values()) + pair[1:]:
        m.close()
    out["n_cus"] = torch.cuda.get_device_properties(0).multi_processor_count
    np.savez(path, **out)


@pytest.fixture(scope="module")
def arms(tmp_path_factory):
    """{"static": arrays, "demand": arrays}: one child process per arm, each run once for all the tests."""
    d = tmp_path_factory.mktemp("dense_tiles")
    got = {}
    for arm, value in (("static", "0"), ("demand", None)):
        env = dict(os.environ, DSMI_DENSE_TOKENS="0", DSMI_PERSIST_SHARED="1")
        env.pop("DSMI_DENSE_TILES", None)
        if value is not None:
            env["DSMI_DENSE_TILES"] = value
        path = str(d / (arm + ".npz"))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), path], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
        if r.returncode < 0 or r.returncode in (124, 134, 137, 139):      # the child died on the GPU: nothing more is started on it in this run
            pytest.exit("dense tiles, %s arm: the child ended with %d\n%s" % (arm, r.returncode, r.stderr[-3000:]), returncode=3)
        assert r.returncode == 0, (arm, r.returncode, r.stderr[-3000:])
        with np.load(path) as z:
            got[arm] = {k: z[k] for k in z.files}
    return got


def _two_forms_ran(arms, key):
    rows, cols = arms["demand"][key.replace("/wgs", "/xp")].shape      # the GEMM's M and N: tiles of 128 rows, pairs of 128-column tiles
    mt, nu = -(-rows // 128), -(-(-(-cols // 128)) // 2)
    total = mt * nu
    static, demand = int(arms["static"][key]), int(arms["demand"][key])
    print("%s: %d x %d tiles, workgroups static %d, by demand %d" % (key, mt, nu, static, demand))
    assert static == 8 * (-(-total // 8)), (key, static, total)
    assert demand == min(total, 2 * int(arms["demand"]["n_cus"])), (key, demand, total)
    assert static != demand, key


def _equal(arms, keys):
    for k in keys:
        a, b = arms["static"][k], arms["demand"][k]
        assert a.shape == b.shape and a.size > 0, k
        assert np.isfinite(a).all(), k
        assert np.array_equal(a, b), "%s: %d of %d values differ, max |d| %.3g" % (k, int((a != b).sum()), a.size, float(np.abs(a - b).max()))


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c[0] for c in LAYER_CASES])
def test_layer_and_its_x_projection_are_bit_identical(arms, name):
    _equal(arms, ["%s/%s%d" % (name, what, rep) for what in ("xp", "y") for rep in range(2)])
    # ... and the second launch on the handle gave what the first did
    assert np.array_equal(arms["demand"][name + "/xp0"], arms["demand"][name + "/xp1"])
    for rep in range(2):
        _two_forms_ran(arms, "%s/wgs%d" % (name, rep))


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c[0] for c in CONV_CASES] + ["forward"])
def test_conv_stack_and_forward_are_bit_identical(arms, name):
    _equal(arms, ["%s/y%d" % (name, rep) for rep in range(2)])
    assert np.array_equal(arms["demand"][name + "/y0"], arms["demand"][name + "/y1"])


@pytest.mark.gpu
def test_two_handles_at_once_keep_their_own_counters(arms):
    _equal(arms, ["pair%d/%s%d" % (k, what, rep) for k in range(2) for what in ("xp", "y") for rep in range(3)])
    for k in range(2):
        assert np.array_equal(arms["demand"]["pair%d/xp0" % k], arms["demand"]["pair%d/xp2" % k])
    assert not np.array_equal(arms["demand"]["pair0/xp0"], arms["demand"]["pair1/xp0"])      # (two different models)
    for k in range(2):
        _two_forms_ran(arms, "pair%d/wgs2" % k)


if __name__ == "__main__":      # python tests/test_gpu_dense_tiles.py OUT.npz: one arm, in a process of its own
    sys.path[:0] = [ROOT]
    _child(sys.argv[1])
