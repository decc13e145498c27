"""The layer-level bound of tests/test_gpu_layer_accuracy.py, ``max |kernel - float64| <= M * e32`` (tests/_layer_cases.py), shown on the
CPU to see what it claims to see -- and where it does not.  A numpy emulation of the recurrent kernels' split-fp16 product
(tests/_split_emu.py) inside the float64 layer stays under ``M * e32``; its mutants, smallest first as measured:

  W_hi * h_lo missing in ONE 32-wide k-block of one direction      (a wrong plane offset for one wave's fragment)
  W_lo * h_hi missing in the last 16 columns of K                  (a tail fragment)
  the 2^-11 fold applied as 2^-10 in one k-block
  one tile's h one step stale at one step                          (a hand-off that does not wait)
  one clip's state not frozen at its length, reverse direction     (masking: shows INSIDE the clip)

SHARP shapes -- default weights, the widths of the case table up to its widest (1280), layer 1 and layer 0: EVERY mutant lies above
``2 * M * e32``, so the bound has a factor two of room on both sides and raising M without looking fails here.  Measured multiples of
e32 for the smallest mutant: 73 (64 units), 36 (224), 13 (800), 11 (1280), 22 (LSTM 512), 12 (LSTM 1024), 24 (RNN 1280), 10 (800 and
1024, layer 0).
COARSE shapes -- saturating weights (``ih_gain=6``; _layer_cases.coarse): e32 itself is several times larger while a lost fragment
is not, and the relation does NOT hold for the three fragment mutants (measured, smallest .. largest of the three: 8.4 .. 17 x e32 at 800
units, 6.6 .. 13 at 1280, 2.2 .. 4.2 at 896 units layer 0 -- only LSTM 512 at 11 .. 21 clears the 8 asked for; the RMS error separates no better: 0.8 x the same multiples).  What is asserted there is what
holds: the emulation under M * e32, the hand-off and masking mutants far above 2 * M * e32, and -- over the table -- that every
coarse case has a sharp sibling of the same kernel, kind and width, which is the case that sees a lost fragment of that form.

One bidirectional layer, T = 60, B = 20 ragged (two tiles), `synthetic.make_state_dict` weights, inputs as the GPU cases draw them.
This file also holds the case table of the GPU test to the planner (rnn_plan.h through `host_fuzz rnnplan`, 256 CUs): every case's
launches are of the kernel the case is about, and the table covers all seven.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _layer_cases as lc
import _split_emu as emu
from danspeech_amd import synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, LENS = 60, np.array([60, 60, 58, 55, 51, 47, 41, 36, 30, 25, 19, 14, 9, 7, 3, 1, 60 - 8, 33, 12, 2])
# (the clips of the second tile are NOT in descending order with the first: the CPU programs do not need a packed batch's order)


def _mutants(H):
    nkb = (H + 31) // 32
    return [("drop_whi_hlo", dict(mutant=("drop_whi_hlo", nkb // 2))),
            ("drop_wlo_hhi_last16", dict(mutant=("drop_wlo_hhi_cols", 16))),
            ("fold_2_10", dict(mutant=("fold_2_10", nkb // 2))),
            ("stale_tile", dict(mutant=("stale", 20, slice(16, 20)))),
            ("unfrozen_clip", dict(unfrozen_clip=7))]


FRAGMENT = ("drop_whi_hlo", "drop_wlo_hhi_last16", "fold_2_10")
SHARP = [("gru", 64, 1), ("gru", 224, 1), ("gru", 800, 1), ("lstm", 512, 1), ("gru", 1280, 1), ("lstm", 1024, 1), ("rnn", 1280, 1), ("gru", 800, 0), ("gru", 1024, 0)]
COARSE = [("gru", 800, 1), ("gru", 1280, 1), ("lstm", 512, 1), ("gru", 896, 0)]


def _errors(kind, H, layer, gain):
    """e32, the clean emulation's max error, {mutant: max error}"""
    c = dict(layer=layer, kind=kind, bidir=True, T=T, B=len(LENS), H=H, gain=gain)
    sd = syn.make_state_dict(2, kind, H, 2, seed=71, ih_gain=gain)
    rng = np.random.default_rng(5)
    if layer == 0:
        x = np.clip(rng.standard_normal((T, len(LENS), syn.rnn_input_size(2))) * 2.5, 0.0, 20.0).astype(np.float32)
        x[rng.random(x.shape) < 0.01] = 20.0
    else:
        x = (rng.standard_normal((T, len(LENS), H)) * 0.5).astype(np.float32)
    ref, e32 = lc.references(c, sd, x, LENS)
    run = lambda **kw: float(np.abs(emu.batch_rnn(sd, layer, kind, x, LENS, True, layer > 0, **kw) - ref).max())
    clean = run()
    print("%s H=%d layer %d gain %g: e32 %.3g, clean emulation %.3g (%.2f x e32)" % (kind, H, layer, gain, e32, clean, clean / e32))
    errs = {}
    for name, kw in _mutants(H):
        errs[name] = run(**kw)
        print("   mutant %-20s %.3g (%.1f x e32)" % (name, errs[name], errs[name] / e32))
    return e32, clean, errs


@pytest.mark.parametrize("kind,H,layer", SHARP)
def test_the_bound_separates_the_emulation_from_its_mutants(kind, H, layer):
    e32, clean, errs = _errors(kind, H, layer, 1.0)
    M = lc.M["split"]
    assert clean <= M * e32
    for name, err in errs.items():
        assert err > 2 * M * e32, (name, err, e32)


@pytest.mark.parametrize("kind,H,layer", COARSE)
def test_saturating_weights_the_bound_sees_hand_offs_and_masking_only(kind, H, layer):
    """ih_gain = 6: the fragment mutants are NOT held to 2 * M * e32 here (module docstring; their figures are printed), the others are."""
    e32, clean, errs = _errors(kind, H, layer, 6.0)
    M = lc.M["split"]
    assert clean <= M * e32
    for name, err in errs.items():
        if name not in FRAGMENT:
            assert err > 2 * M * e32, (name, err, e32)
        else:
            assert err > clean      # (the mutant is a mutant; how many e32 it is worth here is the docstring's statement, not a bound)


def test_case_table_pairs_every_coarse_case():
    """... with a case of the same kernel, kind and width at default weights and T > 1: the one that sees a lost fragment of that form."""
    assert any(lc.coarse(c) for c in lc.CASES)
    for c in lc.CASES:
        if lc.coarse(c):
            assert lc.sharp_sibling(c), c["name"]
    # every width a sharp case runs at is at or below the widest width the relation is asserted at, per layer
    assert max(c["H"] for c in lc.CASES if not lc.coarse(c) and c["layer"] == 1 and c["kernel"] != "steps") <= max(H for _, H, l in SHARP if l == 1)
    assert max(c["H"] for c in lc.CASES if not lc.coarse(c) and c["layer"] == 0) <= max(H for _, H, l in SHARP if l == 0)


def test_the_emulation_is_the_float64_layer_when_nothing_is_split():
    """The hooks change nothing by themselves: an exact product through the `step` hook gives the reference bit for bit."""
    import _f64_ref as f64
    sd = syn.make_state_dict(2, "gru", 32, 2, seed=3)
    x = np.random.default_rng(4).standard_normal((9, 3, 32)).astype(np.float32)
    hooks = {r: dict(step=(lambda w: (lambda h, t: h @ w))(np.ascontiguousarray(f64.layer_weights(sd, 1, r)[1].T))) for r in (False, True)}
    assert np.array_equal(f64.batch_rnn(sd, 1, "gru", x, [9, 5, 1], True, True, hooks=hooks), f64.batch_rnn(sd, 1, "gru", x, [9, 5, 1], True, True))


def test_split_keeps_22_bits():
    x = np.random.default_rng(1).uniform(-1, 1, 4096).astype(np.float32)
    hi, lo = emu.split(x)
    assert np.abs(hi.astype(np.float64) + lo.astype(np.float64) / 2048.0 - x).max() <= 2.0 ** -23


def test_case_table_reaches_every_kernel():
    if not shutil.which("g++"):
        pytest.skip("no g++")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "danspeech_amd", "csrc"), "asan"], stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "danspeech_amd", "csrc", "build", "host_fuzz_asan")
    rows = "".join(lc.plan_row(c) + "\n" for c in lc.CASES)
    r = subprocess.run([exe, "rnnplan", "/dev/stdin"], input=rows, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout.splitlines()
    assert len(out) == len(lc.CASES)
    for c, text in zip(lc.CASES, out):
        kernels = [item.split()[0] for item in text.partition("|")[2].split(";")[:-1]]
        assert set(kernels) == {c["kernel"]}, (c["name"], text)
        assert c["launches"] is None or len(kernels) == c["launches"], (c["name"], text)
        assert text.startswith("x16|") == (c["kernel"] not in ("steps", "persist8")), (c["name"], text)
    assert sorted({c["kernel"] for c in lc.CASES}) == lc.KERNELS and len(lc.KERNELS) == 7
    assert 60 <= len(lc.CASES) <= 90
