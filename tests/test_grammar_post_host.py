"""The host side of the CTC grammar posterior, without a GPU: the numpy reference of the recurrences (tests/_grammar_post_ref.py)
against a brute force over every frame labelling and against finite differences of its own logp (occ and visits are
derivatives); its float64 form against its np.longdouble form on the GPU test's inputs, within a quarter of the contract's
bound; that the bound tells deliberately wrong recurrences apart; Grammar.weight_of; dsmi_grammar_posterior_plan through ctypes.

``DSMI_RECORD_GRAMMAR_POST=1`` (or =PATH) rewrites tests/grammar_post_measured.json (or PATH) from the run: per case the largest
difference between the two forms of the reference for logp, occ and visits, and the bound.  The tests assert against the
bound, never against that file."""
import ctypes
import json
import os

import numpy as np
import pytest

import _grammar_post_ref as pref
import _grammar_ref as gref
from danspeech_amd import _native, synthetic as syn
from danspeech_amd.grammar import Grammar
from test_grammar_host import _random_probs, random_graph

LABELS = syn.DANSPEECH_LABELS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _all_cases():
    cases = [(name, g, probs) for name, g, probs in pref.reference_cases(LABELS)]
    cases += [(name, g, probs) for name, g, _, _, probs in pref.path_cases(len(LABELS))]
    return cases


@pytest.fixture(scope="module")
def cases():
    """The GPU test's inputs with the float64 reference of each, computed once."""
    return [(name, g, probs, pref.posterior(probs, g)) for name, g, probs in _all_cases()]


def test_reference_against_brute_force():
    rng = np.random.default_rng(11)
    reachable = 0
    for case in range(40):
        T, C = int(rng.integers(1, 6)), 4
        g = random_graph(rng, C)
        probs = _random_probs(rng, T, C, case % 4 == 0)
        want, got = pref.brute_force_sum(probs, g), pref.posterior(probs, g)
        assert (want is None) == (got["status"] == 1), case
        assert (gref.brute_force(probs, g) is None) == (want is None)
        if want is None:
            assert got["logp"] == -np.inf and not got["occ"].any() and not got["visits"].any()
            continue
        reachable += 1
        assert abs(float(got["logp"]) - want) < 1e-12 * max(1.0, abs(want)), (case, float(got["logp"]), want)
        np.testing.assert_allclose(got["occ"].sum(1), 1.0, rtol=0, atol=1e-12)
    assert reachable >= 20
    # without frames only the empty sentence
    g = gref.graph([1], [gref.START | gref.FINAL], [[]], None, True)
    assert pref.posterior(np.zeros((0, 4), np.float32), g)["logp"] == 0 and pref.posterior(np.zeros((0, 4), np.float32), gref.chain([1]))["status"] == 1


def test_occ_and_visits_are_the_derivatives_of_logp():
    """d logp / d lp(t, c) = occ[t][c] and d logp / d w[n] = visits[n], by central differences with h = 1e-4: the truncation
    is h^2 / 6 times a third derivative of order 1 and the rounding 2^-52 |logp| / h, both far below 1e-6."""
    rng = np.random.default_rng(3)
    h, checked = 1e-4, 0
    while checked < 12:
        g = random_graph(rng, 4, max_nodes=4)
        probs = _random_probs(rng, 4, 4, False)
        ref = pref.posterior(probs, g)
        if ref["status"]:
            continue
        checked += 1
        lp = np.log(np.maximum(probs, pref.FLT_MIN).astype(np.float64))
        w = gref._weights(g, np.float64)
        f = lambda lp_, w_: float(pref.posterior(probs, g, lp=lp_, weights=w_)["logp"])
        for t in range(4):
            for c in range(4):
                d = np.zeros_like(lp)
                d[t, c] = h
                assert abs((f(lp + d, w) - f(lp - d, w)) / (2 * h) - ref["occ"][t, c]) < 1e-6, (checked, t, c)
        for n in range(len(w)):
            d = np.zeros_like(w)
            d[n] = h
            assert abs((f(lp, w + d) - f(lp, w - d)) / (2 * h) - ref["visits"][n]) < 1e-6, (checked, n)


def test_shapes_keep_the_bound_small(cases):
    for name, g, probs, ref in cases:
        T, F = len(probs), pref.fan_in(g)
        assert ref["status"] == 0, name
        assert T <= 64 and F <= 64 and abs(ref["logp"]) <= 400, (name, T, F, ref["logp"])
        assert pref.bound(T, F, ref["logp"]) <= 1e-7
    assert max(pref.fan_in(g) for _, g, _, _ in cases) == 40
    assert any(len(g.labels) > 256 and len(g.labels) % 4 for _, g, _, _ in cases)
    assert any(g.weights is not None and (g.weights == -80).any() and (g.weights > 0).any() for _, g, _, _ in cases)


@pytest.mark.skipif(np.finfo(np.longdouble).nmant < 63, reason="np.longdouble is no wider than float64 here")
def test_float64_reference_is_within_a_quarter_of_the_bound(cases):
    record = {}
    for name, g, probs, ref in cases:
        wide = pref.posterior(probs, g, dtype=np.longdouble)
        T, F = len(probs), pref.fan_in(g)
        b = pref.bound(T, F, ref["logp"])
        e_logp = float(abs(np.longdouble(ref["logp"]) - wide["logp"]))
        e_occ = float(np.abs(ref["occ"].astype(np.longdouble) - wide["occ"]).max())
        e_vis = float(np.abs(ref["visits"].astype(np.longdouble) - wide["visits"]).max())
        record[name] = dict(T=T, F=F, nodes=len(g.labels), logp=float(ref["logp"]), bound=b, bound_logp=pref.bound_logp(T, F, ref["logp"]),
                            logp_diff=e_logp, occ_diff=e_occ, visits_diff=e_vis)
        print(name, record[name])
        assert e_logp <= pref.bound_logp(T, F, ref["logp"]) / 4, name
        assert e_occ <= b / 4, name
        assert e_vis <= T * b / 4, name
    where = os.environ.get("DSMI_RECORD_GRAMMAR_POST")
    if where:
        path = os.path.join(ROOT, "tests", "grammar_post_measured.json") if where == "1" else where
        with open(path, "w") as f:
            json.dump({"what": "tests/test_grammar_post_host.py: the float64 numpy reference of the grammar posterior against its np.longdouble "
                               "form on the GPU test's inputs: the largest differences, beside the contract's bound (visits holds T * bound)",
                       "cases": record}, f, indent=2)
            f.write("\n")


@pytest.mark.parametrize("variant", pref.VARIANTS)
def test_the_bound_tells_a_wrong_recurrence_apart(cases, variant):
    """Each deliberately wrong recurrence is off by more than 1000 bounds on at least one of the GPU test's inputs."""
    far = []
    for name, g, probs, ref in cases:
        bad = pref.posterior(probs, g, variant=variant)
        b = pref.bound(len(probs), pref.fan_in(g), ref["logp"])
        if bad["status"] or abs(float(bad["logp"]) - float(ref["logp"])) > 1000 * b:
            far.append(name)
    assert far, variant


def test_weight_of_is_the_weighted_path_count():
    for text in ["ja:-0.5 | nej:-1.5 tak", "(en | to:0.75)+ tak", "$d = en | to:-2 ; $d $d", "[ja | nej]", "(a | a b | a b c)* [a]"]:
        g = Grammar(text, LABELS)
        for s in g.sentences(25) + ["nej", "x", "to to to tak", "en  TO tak"]:
            want = pref.accept_logsum(g, [LABELS.index(c) for c in " ".join(s.lower().split())])
            got = g.weight_of(s)
            assert (got is None) == (want is None) == (not g.accepts(s)), (text, s)
            if want is not None:
                assert abs(got - want) < 1e-12, (text, s)
    g = Grammar("ja:-0.5 | nej:-1.5 tak", LABELS)
    assert g.weight_of("nej tak") == -1.5 and g.weight_of(" JA ") == -0.5 and g.weight_of("") is None and g.weight_of("jæ2") is None
    # two node paths spell one sentence: the unmerged automaton of "a | a" keeps both
    twice = Grammar("a | a", LABELS, _merge=False)
    assert abs(twice.weight_of("a") - np.log(2.0)) < 1e-15 and Grammar("a | a", LABELS).weight_of("a") == 0.0


def test_plan_numbers_and_refusals():
    L = _native.lib()
    info = _native.grammar_posterior_plan(32, 501, 2048, 8192)
    assert info["node_stride"] == 2048 and info["ws_bytes"] == 32 * 501 * (32 * 2048 + 16) and info["ws_bytes"] <= 1 << 30
    # LDS: two rows of float64 (tok, blk) pairs, node words and weights, 16-bit arc offsets, start nodes and arcs, the feeder's two
    # chunks of 16 x 128 doubles, the end's reduction, the list of the nodes a wave reduces
    assert info["lds_bytes"] == 32 * 2048 + 8 * 2048 + 2 * (2048 + 4) + 2 * 2048 + 2 * 8192 + 2 * 8 * 16 * 128 + 8 * 256 + 2 * (8192 // 25 + 1) + 8
    assert info["lds_bytes"] < 160 * 1024
    assert _native.grammar_posterior_plan(32, 501, 1500, 2000)["ws_bytes"] == 32 * 501 * (32 * 1500 + 16)      # the 300-word loop fits
    assert _native.grammar_posterior_plan(1, 1, 0, 0)["node_stride"] == 4 and _native.grammar_posterior_plan(3, 7, 257, 1)["node_stride"] == 260
    out = np.zeros(3, dtype=np.int64)
    ptr = out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    for args, code in [((0, 5, 1, 1), _native.DSMI_ERR_INVALID), ((5, 0, 1, 1), _native.DSMI_ERR_INVALID), ((1, 1, -1, 0), _native.DSMI_ERR_INVALID),
                       ((1, 1, 2049, 0), _native.DSMI_ERR_CAPACITY), ((1, 1, 2048, 8193), _native.DSMI_ERR_CAPACITY),
                       ((33, 501, 2048, 0), _native.DSMI_ERR_CAPACITY), ((1 << 12, 1 << 12, 0, 0), _native.DSMI_ERR_CAPACITY)]:
        assert L.dsmi_grammar_posterior_plan(*args, ptr) == code, args
        assert not out.any()
    assert L.dsmi_grammar_posterior_plan(1, 1, 1, 1, None) == _native.DSMI_ERR_INVALID
    with pytest.raises(_native.DsmiError):
        _native.grammar_posterior_plan(33, 501, 2048, 0)
