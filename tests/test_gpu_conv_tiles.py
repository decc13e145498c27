"""The conv layers' two tile orders (csrc/conv_rows.h): one workgroup per tile on the grid (t-tiles, f-tiles, clips x channel tiles),
or min(tiles, 2 x CUs) workgroups that take tile after tile by demand.  The order changes which workgroup computes a tile and when,
never what it computes: the output of `dsmi_conv_stack` must be EQUAL, bit for bit, between a process with DSMI_CONV_TILES=0 and one
with DSMI_CONV_TILES=1, and each within the float64 bound of tests/test_gpu_dense_accuracy.py (max |gpu - float64| <= M * e32, the
M and e32 of tests/_dense_cases.py, reference tests/_f64_ref.py).  Both forms skip the kernel rows that read only the frequency
padding, so the bound is also what holds the skip.  The switch is read once per process, so each arm is a fresh child process (this
file, run as a script); DSMI_DENSE_TOKENS=0 in both, so that the two handles of the last case really run side by side.

  big2   2 conv layers, B = 8, T = 800, n_freq 161, ragged lengths, the shortest clip (25 output steps) shorter than a 64-step tile:
         7 x 11 x 8 = 616 tiles in either layer, more than 2 x 256 workgroups: workgroups loop and steal and meet masked tiles in the
         middle of a walk.  Twice on one handle: the second launch finds the counters as the first one's last workgroup left them.
  big3   3 conv layers, B = 5, T = 800: the third layer has 7 x 6 x 15 (5 clips x 3 channel tiles) = 630 tiles
  f2     2 layers, n_freq 2, B = 3, T = 70: one output row whose range of real kernel rows is cut at both ends
  pair   two handles on two streams at once (two threads), big2's shape, three launches each: the counters are per handle

That the two arms are two forms of the kernels, not one run twice, is asserted on the workgroups of each layer's last launch
(`dsmi_debug_conv_workgroups`): one per tile against min(tiles, 2 x CUs).

The measured ratios gpu_max / e32 go to tests/conv_tiles_measured.json when DSMI_RECORD_CONV_TILES=1 (or =PATH); they are to be set
against tests/dense_accuracy_measured.json (largest conv ratio 8.62).  The tests assert against M, never against that file."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BIG_LENS = [800, 777, 640, 515, 400, 259, 129, 50]
CASES = {  # name: (conv layers, n_freq, B, T, lens, feature seed, launches)
    "big2": (2, 161, 8, 800, BIG_LENS, 41, 2),
    "big3": (3, 161, 5, 800, [800, 650, 401, 130, 64], 42, 2),
    "f2": (2, 2, 3, 70, [70, 64, 9], 43, 2),
    "pair0": (2, 161, 8, 800, BIG_LENS, 41, 3),
    "pair1": (2, 161, 8, 800, [800, 700, 600, 500, 300, 200, 90, 40], 44, 3),      # (lengths are taken longest first)
}
WEIGHT_SEED = 23


def _case(name):
    """(cfg, state dict, audio_conf, x [B, 1, F, T] float32, lens): seeded, the same in the parent and in both children."""
    sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "tests")) if p not in sys.path]
    import _dense_cases as dc
    from danspeech_amd import synthetic as syn
    cl, n_freq, B, T, lens, seed, _ = CASES[name]
    ac = dc.AUDIO[n_freq] or {}
    cfg = dict(conv_layers=cl, rnn_type="gru", rnn_hidden_size=8, rnn_layers=1, bidirectional=True, context=20)
    sd = syn.make_state_dict(cl, "gru", 8, 1, seed=WEIGHT_SEED, sample_rate=ac.get("sampling_rate", 16000), window_size=ac.get("window_size", 0.02))
    x = np.random.default_rng(seed).standard_normal((B, 1, n_freq, T)).astype(np.float32)      # nothing zeroed past the lengths
    return cfg, sd, dc.AUDIO[n_freq], x, np.array(lens, dtype=np.int32)


def _conv_wgs(m):
    import ctypes as C
    from danspeech_amd import _native
    w = (C.c_int32 * 3)()
    n = _native.lib().dsmi_debug_conv_workgroups(m._h, w, 3)
    assert n == m.desc.conv_layers, n
    return np.array(w[:n], dtype=np.int32)


def _child(path):
    import threading
    import torch
    from danspeech_amd import _native
    out = {}

    def run(name, m):
        _, _, _, x, lens = _case(name)
        feat = torch.from_numpy(x).cuda()
        for rep in range(CASES[name][6]):
            out["%s/y%d" % (name, rep)] = m.conv_stack(feat, lens).cpu().numpy()
            out["%s/wgs%d" % (name, rep)] = _conv_wgs(m)

    def model(name):
        cfg, sd, ac, _, _ = _case(name)
        return _native.NativeModel(cfg, sd, audio_conf=ac)

    for name in ("big2", "big3", "f2"):
        m = model(name)
        try:
            run(name, m)
        finally:
            m.close()
    pair = [model("pair0"), model("pair1")]
    torch.cuda.synchronize()
    errors = []

    def work(k):
        try:
            with torch.cuda.stream(torch.cuda.Stream()):
                run("pair%d" % k, pair[k])
        except Exception as e:      # noqa: BLE001 (reported by the parent)
            errors.append(repr(e))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for m in pair:
        m.close()
    out["n_cus"] = torch.cuda.get_device_properties(0).multi_processor_count
    np.savez(path, **out)


@pytest.fixture(scope="module")
def arms(tmp_path_factory):
    """{"static": arrays, "demand": arrays}: one child process per arm, each run once for all the tests."""
    d = tmp_path_factory.mktemp("conv_tiles")
    got = {}
    for arm, value in (("static", "0"), ("demand", "1")):
        env = dict(os.environ, DSMI_DENSE_TOKENS="0", DSMI_CONV_TILES=value)
        env.pop("DSMI_DENSE_TILES", None)
        path = str(d / (arm + ".npz"))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), path], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
        if r.returncode < 0 or r.returncode in (124, 134, 137, 139):      # the child died on the GPU: nothing more is started on it in this run
            pytest.exit("conv tiles, %s arm: the child ended with %d\n%s" % (arm, r.returncode, r.stderr[-3000:]), returncode=3)
        assert r.returncode == 0, (arm, r.returncode, r.stderr[-3000:])
        with np.load(path) as z:
            got[arm] = {k: z[k] for k in z.files}
    return got


@pytest.fixture(scope="module")
def refs():
    """name -> (float64 reference, e32, out_lens): computed once on the CPU, shared, left unchanged."""
    sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "tests")) if p not in sys.path]
    import _dense_cases as dc
    from oracle import model as om
    out = {}
    for name in CASES:
        if name == "pair0":      # big2's model and input
            out[name] = out["big2"]
            continue
        cfg, sd, _, x, lens = _case(name)
        out_lens = om.get_seq_lens(lens, cfg["conv_layers"])
        ref, e32, _ = dc.conv_references(dict(depth=cfg["conv_layers"]), sd, x, out_lens)
        ref.setflags(write=False)
        out[name] = (ref, e32, out_lens)
    return out


@pytest.fixture(scope="module")
def measured():
    recs = []
    yield recs
    where = os.environ.get("DSMI_RECORD_CONV_TILES")
    if where and recs:
        path = os.path.join(ROOT, "tests", "conv_tiles_measured.json") if where == "1" else where
        doc = dict(header=dict(what="tests/test_gpu_conv_tiles.py on one MI355X: per case and tile order the fp32 oracle's max error against float64 (e32), the "
                                    "conv stack's max error against float64, ratio = gpu_max / e32; to be set against tests/dense_accuracy_measured.json",
                               max_ratio=max(r["ratio"] for r in recs)), cases=recs)
        with open(path, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


def _tiles(name, n_layers):
    """tiles of each layer's launch: t-tiles of 64 output steps x f-tiles (8 rows in layer 1, 4 behind it) x clips x 32-channel tiles"""
    from danspeech_amd.synthetic import conv_out_freq
    cl, n_freq, B, T = CASES[name][:4]
    nt = -(-((T - 1) // 2 + 1) // 64)
    return [nt * -(-conv_out_freq(n_freq, l + 1) // (8 if l == 0 else 4)) * B * (3 if l == 2 else 1) for l in range(n_layers)]


def _check(arms, refs, measured, name):
    import _dense_cases as dc
    reps = CASES[name][6]
    ref, e32, out_lens = refs[name]
    for rep in range(reps):
        k = "%s/y%d" % (name, rep)
        a, b = arms["static"][k], arms["demand"][k]
        assert a.shape == b.shape == ref.shape and a.size > 0, k
        assert np.isfinite(a).all() and np.isfinite(b).all(), k
        assert np.array_equal(a, b), "%s: %d of %d values differ between the tile orders, max |d| %.3g" % (k, int((a != b).sum()), a.size, float(np.abs(a - b).max()))
        for arm in ("static", "demand"):      # the later launches on a handle gave what the first did
            assert np.array_equal(arms[arm][k], arms[arm][name + "/y0"]), (arm, k)
    n_cus = int(arms["demand"]["n_cus"])
    tiles = _tiles(name, CASES[name][0])
    for rep in range(reps):
        st, dm = arms["static"]["%s/wgs%d" % (name, rep)].tolist(), arms["demand"]["%s/wgs%d" % (name, rep)].tolist()
        print("%s launch %d: tiles %s, workgroups static %s, by demand %s" % (name, rep, tiles, st, dm))
        assert st == tiles, (name, st, tiles)
        assert dm == [min(t, 2 * n_cus) for t in tiles], (name, dm, tiles)
    M = dc.M["conv_split"]
    c = dict(depth=CASES[name][0])
    for arm in ("static", "demand"):
        y = arms[arm][name + "/y0"]
        gpu_max = float(np.abs(y.astype(np.float64) - ref).max())
        past = dc.past_len_max(y, out_lens)
        measured.append(dict(name=name, arm=arm, e32=e32, gpu_max=gpu_max, ratio=gpu_max / e32, past_len_max=past))
        print("%s %s: e32 %.3g, gpu max %.3g, ratio %.2f (M %g), past the lengths %.3g" % (name, arm, e32, gpu_max, gpu_max / e32, M, past))
        assert past == 0.0, dc.localise_conv(c, y, ref, out_lens)
        assert gpu_max <= M * e32, "max error %.3g > %g x e32 = %.3g (ratio %.2f).  %s" % (gpu_max, M, M * e32, gpu_max / e32, dc.localise_conv(c, y, ref, out_lens))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["big2", "big3", "f2"])
def test_tile_orders_are_bit_identical_and_within_the_float64_bound(arms, refs, measured, name):
    _check(arms, refs, measured, name)
    tiles = _tiles(name, CASES[name][0])
    if name != "f2":      # the shapes are chosen so that workgroups loop: more tiles than an MI355X holds workgroups
        assert tiles[-1] > 2 * int(arms["demand"]["n_cus"]), (tiles, int(arms["demand"]["n_cus"]))


@pytest.mark.gpu
def test_two_handles_at_once_keep_their_own_counters(arms, refs, measured):
    for k in range(2):
        _check(arms, refs, measured, "pair%d" % k)
    assert np.array_equal(arms["demand"]["pair0/y0"], arms["demand"]["big2/y0"])      # (the same model and input as big2)
    assert not np.array_equal(arms["demand"]["pair0/y0"], arms["demand"]["pair1/y0"])


if __name__ == "__main__":      # python tests/test_gpu_conv_tiles.py OUT.npz: one arm, in a process of its own
    sys.path[:0] = [ROOT]
    _child(sys.argv[1])
