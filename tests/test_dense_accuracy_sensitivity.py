"""The dense bound of tests/test_gpu_dense_accuracy.py, ``max |kernel - float64| <= M * e32`` (tests/_dense_cases.py), shown on the CPU
to see what it claims to see -- and where it does not --, and the conditions the case tables promise (ceiling shares of the hot
cases, clamp hits of the lookahead cases, the logit span of the sharp one, default-weight siblings).

A numpy emulation of the two split conv forms (tests/_split_emu.py: ConvStackEmu) stays under ``M["conv_split"] * e32`` (0.91 ..
1.37 x e32).  M is 32 -- the kernels' long float32 accumulation chains measure up to 8.6 x e32 at 161 bins (_dense_cases.py) --, so a
mutant has to reach 64 x e32 to lie above ``2 * M * e32``.  The mutants at the default-weight cases c (3 x 33 frames) and e (5 x
95), n_freq 161, conv depths 1 to 3, as measured (multiples of e32, smallest .. largest; a layer-2 mutant exists from depth 2 on):

  SEEN (asserted above 2 * M * e32 at every one of these cases)
  the W_hi * x_lo product missing for one kernel row of layer 1                             76 .. 135
  layer 1's cross terms of one kernel row folded with 2^-10                                 110 .. 223
  one kernel row of layer 2 reading the input row two below, for one output row             1.3e5 .. 5.4e5
  the mask applied at t > out_len instead of t >= out_len                                   1.0e6 .. 2.7e6

  NOT SEEN at these cases (M was not moved to fit; asserted only to be mutants at all)
  the W_lo * x_hi product missing for ONE tap (kf, kt) of layer 2                           32 .. 64: at or below 2 * M, at M itself
  the lo plane of the layer-1 output missing for one tap's 32-channel chunk of layer 2      33 .. 45
  the last output step of a 64-step tile losing its rightmost tap                           = the clean emulation (see below)

The two lost layer-2 products are whole-term mutants, which must be seen somewhere: the SHARPER case is c at n_freq 2, depth 2
(conv-c-d2-f2-default, in the GPU table).  With one input row only kernel row 10 of layer 2 meets data, a sum has 352 terms instead
of 7392, e32 is 3.3e-8 instead of 5e-7 and the GPU's ratio there is 1.03 -- and one lost tap is as large as anywhere: 158 and 154 x
e32, asserted above 2 * M * e32 (the layer-1 row mutants: 216 and 290 x).  At depth 3, n_freq 2, the same mutants reach the output through layer 3
and are 10 .. 12 x e32: not seen.  So one lost lo product per tap of conv_split.hip is caught at the 2-bin shape of depth 2 and
NOT at 161 bins, where only errors above 32 x e32 (1.7e-5 at depth 2, 8e-6 at depth 3) are.

The short halo: with To = 17 and 48 the first tile's last step IS the stack's last step, its rightmost tap reads the zero padding,
and the mutant computes what the clean kernel computes (its figure equals the clean emulation's).  The mutant needs a tile that ends
inside the batch: it is held to ``2 * M * e32`` at case a (To = 130, depth 2: step 63, inside the clips of 130 and 65 output steps),
where it measures 4.6e5 x e32.

The hot cases (HOT_GAIN) are coarse in the sense of _layer_cases.py: e32 grows with the weights (2 .. 5e-5).  Nothing is asserted
about them beyond the table's pairing: every hot case has a default-weight sibling of the same depth and shape.
"""
import numpy as np
import pytest

import _dense_cases as dc
import _f64_ref as f64
import _split_emu as emu

WHOLE_TERM = ("l2_drop_wlo_xhi", "l1_drop_whi_xlo", "l2_drop_xlo")


def _mutants(depth):
    m = [("l1_drop_whi_xlo", 20), ("l1_fold_2_10", 20), ("mask_gt",)]
    if depth > 1:       # tap (10, 5) is the kernel's centre; output row 7 is the last row of the second 4-row workgroup
        m += [("l2_drop_wlo_xhi", 10, 5), ("l2_drop_xlo", 10, 5), ("l2_ring_late", 10, 7), ("l2_halo_short",)]
    return m


def _case(shape, depth):
    """the default-weight case of that shape and depth (e at depth 1 is not in the GPU table: the same generator makes it)"""
    return dc._conv(shape, depth)


def _errors(c, mutants):
    cfg, sd, ac, x, lens, out_lens = dc.make_conv_case(c)
    ref, e32, _ = dc.conv_references(c, sd, x, out_lens)
    E = emu.ConvStackEmu(sd, x, out_lens, c["depth"])
    clean = float(np.abs(E.clean - ref).max())
    print("%s: e32 %.3g, clean emulation %.3g (%.2f x e32)" % (c["name"], e32, clean, clean / e32))
    errs = {}
    for m in mutants:
        errs[m[0]] = float(np.abs(E.run(m) - ref).max())
        print("   mutant %-18s %.3g (%.1f x e32)" % (m[0], errs[m[0]], errs[m[0]] / e32))
    return e32, clean, errs


NOT_SEEN_AT_161 = ("l2_drop_wlo_xhi", "l2_drop_xlo", "l2_halo_short")       # module docstring


@pytest.mark.parametrize("shape,depth", [(s, d) for s in "ce" for d in (1, 2, 3)])
def test_the_bound_separates_the_emulation_from_its_mutants(shape, depth):
    e32, clean, errs = _errors(_case(shape, depth), _mutants(depth))
    M = dc.M["conv_split"]
    assert clean <= M * e32
    for name, err in errs.items():
        if name == "l2_halo_short":       # not a mutant at these shapes: it IS the clean emulation
            assert err == clean
        elif name in NOT_SEEN_AT_161:     # a mutant, but one the bound does not see here; the sharper case is the next test's
            assert err > 4 * clean
        else:
            assert err > 2 * M * e32, (name, err, e32)


def test_the_whole_term_mutants_are_seen_at_the_two_bin_case():
    """conv-c-d2-f2-default: sums of 352 terms, e32 = 3e-8.  Every lost lo product -- one tap of layer 2, one kernel row of layer 1 --
    lies above 2 * M * e32 there."""
    c, = [c for c in dc.CONV_CASES if c["name"] == "conv-c-d2-f2-default"]
    e32, clean, errs = _errors(c, [("l2_drop_wlo_xhi", 10, 5), ("l2_drop_xlo", 10, 5), ("l1_drop_whi_xlo", 20), ("l1_fold_2_10", 20)])
    M = dc.M["conv_split"]
    assert clean <= M * e32 and set(WHOLE_TERM) <= set(errs)
    for name, err in errs.items():
        assert err > 2 * M * e32, (name, err, e32)


def test_a_halo_short_by_one_step_is_seen_where_a_tile_ends_inside_the_batch():
    e32, clean, errs = _errors(_case("a", 2), [("l2_halo_short",)])
    M = dc.M["conv_split"]
    assert clean <= M * e32
    assert errs["l2_halo_short"] > 2 * M * e32


def test_the_emulation_is_the_float32_oracle_when_nothing_is_split():
    """`correlate` on float32 arrays is what the emulation's products run on: by itself it agrees with the float64 one to float32 noise."""
    rng = np.random.default_rng(2)
    x, w = rng.standard_normal((2, 3, 9, 14)).astype(np.float32), rng.standard_normal((4, 3, 5, 3)).astype(np.float32)
    a, b = f64.correlate(x, w, (2, 1), (2, 1)), f64.correlate(x.astype(np.float64), w.astype(np.float64), (2, 1), (2, 1))
    assert a.dtype == np.float32 and a.shape == b.shape == (2, 4, 5, 14) and np.abs(a - b).max() < 1e-4
    hi, lo = emu.split_unscaled(rng.uniform(0, 20, 4096).astype(np.float32))
    assert np.abs(lo).max() <= 2.0 ** -7        # conv_split.hip's header: inputs in [0, 20] have lo terms up to 2^-7


# ---- the conditions of the case tables ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in dc.CONV_CASES if c["weights"] == "hot"])
def test_hot_cases_reach_the_ceiling(name):
    """Of every layer's in-length outputs (float64 reference): at least 1 % at the ceiling of 20, at least 20 % strictly inside (0, 20)."""
    c, = [c for c in dc.CONV_CASES if c["name"] == name]
    cfg, sd, ac, x, lens, out_lens = dc.make_conv_case(c)
    layers = []
    f64.conv_stack(sd, x, out_lens, c["depth"], layers_out=layers)
    assert len(layers) == c["depth"]
    for li, y in enumerate(layers):
        v = np.concatenate([y[b, :, :, :L].ravel() for b, L in enumerate(out_lens)])
        at, inside = float((v == 20.0).mean()), float(((v > 0.0) & (v < 20.0)).mean())
        print("%s layer %d (gain %g): %.1f %% at 20, %.1f %% inside (0, 20)" % (name, li + 1, dc.HOT_GAIN[li], 100 * at, 100 * inside))
        assert at >= 0.01 and inside >= 0.20


def test_case_table_pairs_every_hot_case():
    hot = [c for c in dc.CONV_CASES if c["weights"] == "hot"]
    assert {(c["shape"], c["depth"]) for c in hot} == {(s, d) for s in "ac" for d in (2, 3)}
    for c in hot:
        assert dc.default_sibling(c), c["name"]


def test_conv_table_covers_what_it_says():
    has = lambda **kw: any(all(c[k] == v for k, v in kw.items()) for c in dc.CONV_CASES)
    for s in "acd":
        for d in (1, 2, 3):
            assert has(shape=s, depth=d, n_freq=161, weights="default", env={})
    for s in "be":
        for d in (2, 3):
            assert has(shape=s, depth=d, n_freq=161, weights="default", env={})
    assert has(shape="a", depth=3, n_freq=81) and has(shape="c", depth=2, n_freq=2) and has(shape="c", depth=3, n_freq=2)
    for s in "ac":
        for d in (2, 3):
            assert has(shape=s, depth=d, env=dc.F32, family="conv_f32")
    assert has(shape="c", depth=2, weights="range", env={}, family="conv_f32")
    from danspeech_amd import synthetic as syn
    assert [syn.conv_out_freq(81, d) for d in (1, 2, 3)] == [41, 21, 11] and syn.conv_out_freq(2, 3) == 1
    c, = [c for c in dc.CONV_CASES if c["weights"] == "range"]
    w = dc.make_conv_case(c)[1]["conv.seq_module.3.weight"]
    assert np.abs(w).max() == 1000.0 > 60000.0 / 64 and (np.abs(w) >= 60000.0 / 64).sum() == 1
    # the features keep their values past each clip's length
    cfg, sd, ac, x, lens, out_lens = dc.make_conv_case(_case("a", 1))
    assert all(np.abs(x[b, :, :, L:]).min() > 0 for b, L in enumerate(lens) if L < x.shape[3])
    assert list(out_lens) == [130, 65, 64, 1]


def test_head_table_covers_what_it_says():
    bi = [c for c in dc.HEAD_CASES if c["bidir"] and not c["sharp"]]
    assert {c["C"] for c in bi if c["H"] == 100} >= {1, 29, 32, 33, 64, 65, 96, 97, 128}
    for C in (33, 97):
        assert {(c["H"], c["To"], c["B"]) for c in bi if c["C"] == C} >= {(H, To, B) for H in (8, 13, 100, 800) for To, B in dc.ROWS}
    assert sorted(To * B for To, B in dc.ROWS) == [1, 31, 32, 33, 70]
    uni = [c for c in dc.HEAD_CASES if not c["bidir"]]
    assert {(c["context"], c["To"]) for c in uni} >= {(ctx, To) for ctx in (1, 3, 20) for To in (7, 25)}
    assert sum(c["sharp"] for c in dc.HEAD_CASES) == 1


@pytest.mark.parametrize("name", [c["name"] for c in dc.HEAD_CASES if not c["bidir"] or c["sharp"]])
def test_head_cases_meet_their_conditions(name):
    """Unidirectional: both clamps of the lookahead are hit (float64 reference).  Sharp: the float64 logits span more than 200."""
    c, = [c for c in dc.HEAD_CASES if c["name"] == name]
    cfg, sd, ac, x_fwd, x_rev = dc.make_head_case(c)
    ref, e32, la, logits = dc.head_references(c, sd, x_fwd, x_rev)
    assert ref.shape == (c["B"], c["To"], c["C"]) and abs(ref.sum(axis=-1) - 1.0).max() < 1e-12
    if not c["bidir"]:
        print("%s: %d of %d lookahead outputs at 0, %d at 20" % (name, (la == 0).sum(), la.size, (la == 20).sum()))
        assert (la == 0.0).any() and (la == 20.0).any() and ((la > 0) & (la < 20)).any()
    if c["sharp"]:
        span = float((logits.max(axis=-1) - logits.min(axis=-1)).max())
        print("%s: logits span %.0f within a row" % (name, span))
        assert span > 200.0
        with np.errstate(over="ignore"):
            assert np.isinf(np.exp(logits.astype(np.float32))).any()       # ... and without the maximum subtracted, float32 exp overflows
