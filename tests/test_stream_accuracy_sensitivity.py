"""What the bound of tests/test_gpu_stream_accuracy.py would catch, shown on the CPU: mutants of the float64 streaming model
(tests/_f64_ref.py stream_model, through its hooks) stand in for a streaming pass that is subtly wrong, and each must lie above
``2 * M * e32`` of its case -- twice the bound, so that a wrong pass whose own rounding happens to point the other way is still
seen.  Nothing here touches the GPU.

The mutants (one carried-state mistake each; ``applies`` says which cases have the axis, and every mutant applies somewhere):

  no_carry        layer 1 alone hands zeros to the next chunk instead of h
  stale_h         every layer hands on the h of the frame before the last (the packed state's other parity)
  lstm_c_early    LSTM: c taken one live step early, in every layer
  lstm_c_run_on   LSTM: c taken after running on, on zero rows, to the longest chunk of the session's round
  neighbour       session i receives session i + 1's state (sessions that advance in lock step)
  tile_stride     session i receives session i + 32's state: the next tile's
  conv_tail_1/_2  the ten frames conv layer 1 / 2 keeps, shifted by one frame
  la_shift        the lookahead's kept rows shifted by one
  no_right_pad    the five zero frames behind an is_last chunk dropped (the leading frames are compared; fewer are yielded too)
  first_clears    an is_first that no is_last preceded also clears h / c

They run on the table's ``sens`` cases: per axis the small cases that have it (one tile and two, several tiles with ragged chunks,
out of phase for all three kinds, contexts 1 / 2 / 20, both per-step shapes).  Measured here (numpy 2, OpenBLAS; printed by the
tests): 40 x e32 .. 787000 x e32 over the 94 applicable pairs, against thresholds of 16 (M = 8) and 4 (M = 2).  The smallest is
stale_h on phase-lstm-H64-N5 at 40 x (5.1e-7), then the same mutant on tiles-lstm-H64-N70 at 60 x: an LSTM's memory is c, which the
mutant hands on intact, and the stale h enters one step's ``h W_hh^T`` only (the GRU and RNN cases of the same shapes, whose h IS the
memory, are at 1974 x and 11874 x).  Everything else is at 200 x and above (stale_h on steps-lstm-H20-N3 202 x, lstm_c_early
208 x).  So this test passes at M = 16 for the persistent family and fails at M = 32 (threshold 64 > 40); for the per-step family
it fails from M = 128 on (threshold 256 > 202).

The table's own claims, from the references alone: a case names every CARRY instantiation (kind, NPW class, MULTI) of
rnn_persist_kernel; both clamps of the lookahead are hit somewhere; no case is so flat or so saturated that e32 < 1e-9; the chunk
arithmetic (``walk``) yields the frames the float64 model and the oracle yield.
"""
import functools

import numpy as np
import pytest

import _f64_ref as f64
import _stream_cases as sc

SENS = [c for c in sc.CASES if c["sens"]]


@functools.lru_cache(maxsize=None)
def _baseline(name):
    """(cfg, sd, float64 outputs, e32) of a case, computed once"""
    c, = [c for c in sc.CASES if c["name"] == name]
    cfg, sd, _ = sc.make_case(c)
    ref, o32 = sc.references(c, sd, cfg)
    assert sc.shape_of(ref) == sc.shape_of(o32) == [[p["nout"] for p in sc.walk(c, s)] for s in sc.sessions(c)]
    return cfg, sd, ref, sc.distance(o32, ref)


def _layer(c):
    return min(1, c["layers"] - 1)


def _chunks(sched):
    return [e for e in sched if e is not None]


def _round_tcmax(c):
    """per round the longest chunk (in steps) of the sessions due"""
    scheds = sc.sessions(c)
    return [max([sc.chunk_tc(*s[r]) for s in scheds if r < len(s) and s[r] is not None] or [0]) for r in range(max(len(s) for s in scheds))]


def _run_on_steps(c, sched):
    """per chunk of the schedule: the steps from its own last one to the end of its round's longest chunk"""
    tcmax = _round_tcmax(c)
    return [tcmax[r] - sc.chunk_tc(*e) for r, e in enumerate(sched) if e is not None]


def _carry_hook(c, fn, every_layer=True):
    """fn in every layer (what a mistake in the kernel does), or in layer 1 alone"""
    L = _layer(c)
    return lambda l, hs, cs, run_on: fn(hs, cs, run_on) if every_layer or l == L else (hs[-1], cs[-1])


def _lstm_run_on(c, sched, members):
    extra, calls = _run_on_steps(c, sched), [0]

    def fn(hs, cs, run_on):
        n = extra[calls[0] // c["layers"]]      # one call per layer and chunk
        calls[0] += 1
        return hs[-1], run_on(n)[1]
    return dict(carry=_carry_hook(c, fn))


def _shift_rows(x, ctx):
    k = x.shape[0] if ctx == 1 else min(x.shape[0], ctx - 1)
    return x[-k - 1:-1] if x.shape[0] > k else np.roll(x, 1, axis=0)


def _restarts_with_state(sched):
    live = False
    for T, first, last in _chunks(sched):
        if first and live:
            return True
        live = not last
    return False


# name -> (applies(c, sched, members), hooks(c, sched, members)); a mutant is applied to every batch of a case it applies to
MUTANTS = {
    "no_carry": (lambda c, s, m: True, lambda c, s, m: dict(carry=_carry_hook(c, lambda hs, cs, run_on: (np.zeros_like(hs[-1]), cs[-1]), every_layer=False))),
    "stale_h": (lambda c, s, m: True, lambda c, s, m: dict(carry=_carry_hook(c, lambda hs, cs, run_on: (hs[-2], cs[-1])))),
    "lstm_c_early": (lambda c, s, m: c["kind"] == "lstm", lambda c, s, m: dict(carry=_carry_hook(c, lambda hs, cs, run_on: (hs[-1], cs[-2])))),
    "lstm_c_run_on": (lambda c, s, m: c["kind"] == "lstm" and any(n > 0 and not e[2] for n, e in zip(_run_on_steps(c, s), _chunks(s))), _lstm_run_on),
    "neighbour": (lambda c, s, m: len(m) >= 2, lambda c, s, m: dict(route=lambda l, B: (np.arange(B) + 1) % B)),
    "tile_stride": (lambda c, s, m: len(m) == c["N"] > 32, lambda c, s, m: dict(route=lambda l, B: (np.arange(B) + 32) % B)),
    "conv_tail_1": (lambda c, s, m: True, lambda c, s, m: dict(tail=lambda li, x: x[..., -11:-1] if li == 0 else x[..., -10:])),
    "conv_tail_2": (lambda c, s, m: True, lambda c, s, m: dict(tail=lambda li, x: x[..., -11:-1] if li == 1 else x[..., -10:])),
    "la_shift": (lambda c, s, m: True, lambda c, s, m: dict(keep=_shift_rows)),
    "no_right_pad": (lambda c, s, m: True, lambda c, s, m: dict(rpad=lambda li: 0)),
    "first_clears": (lambda c, s, m: _restarts_with_state(s), lambda c, s, m: dict(first_clears_state=True)),
}


def _applies(mut, c):
    return any(MUTANTS[mut][0](c, s, m) for s, m in sc.groups(c))


PAIRS = [(mut, c["name"]) for mut in MUTANTS for c in SENS if _applies(mut, c)]


def _mutant_distance(mut, c):
    cfg, sd, ref, e32 = _baseline(c["name"])
    applies, hooks = MUTANTS[mut]
    got = sc.run_reference(c, sd, cfg, lambda sd, cfg, s, m: f64.stream_model(sd, cfg, hooks(c, s, m) if applies(c, s, m) else None))
    return sc.distance(got, ref), e32


@pytest.mark.parametrize("mut,name", PAIRS)
def test_the_bound_sees_the_mutant(mut, name):
    c, = [c for c in SENS if c["name"] == name]
    d, e32 = _mutant_distance(mut, c)
    M = sc.M[c["family"]]
    print("%s on %s: %.3g = %.0f x e32 (%.3g); the bound is %g x" % (mut, name, d, d / e32, e32, M))
    assert d > 2.0 * M * e32, "%s on %s is %.3g = %.1f x e32: a bound of %g x e32 does not see it" % (mut, name, d, d / e32, M)


def test_every_mutant_applies_somewhere_and_the_rest_is_said():
    for mut in MUTANTS:
        on = [c["name"] for c in SENS if _applies(mut, c)]
        off = [c["name"] for c in SENS if not _applies(mut, c)]
        print("%s: applies to %d cases; does not apply to %s" % (mut, len(on), off or "none"))
        assert on, mut
    assert sorted(set(m for m, _ in PAIRS)) == sorted(MUTANTS)


def test_a_case_names_every_carry_instantiation():
    """rnn_persist_kernel<KIND, NPW, MULTI, false, true>: 3 kinds x NPW 2 / 4 / 7 / 10 x one tile / several (launch_kind)"""
    have = {(c["kind"], sc.npw_class(c["H"]), n > 32) for c in sc.CASES if c["kernel"] == "persist8" for n in sc.passes(c)}
    want = {(k, n, mu) for k in ("gru", "lstm", "rnn") for n in (2, 4, 7, 10) for mu in (False, True)}
    assert want <= have, sorted(want - have)
    # ... the edges of every class, an odd nq with several sessions, eight tiles and the split above them, both per-step reasons
    gru = {(c["H"], c["N"]) for c in sc.CASES if c["kind"] == "gru" and c["kernel"] == "persist8"}
    assert {(H, N) for H in (8, 256, 264, 512, 520, 896, 904, 1280) for N in (3, 33)} <= gru
    assert [sc.npw_class(H) for H in (8, 256, 264, 512, 520, 896, 904, 1280, 1288, 100)] == [2, 2, 4, 4, 7, 7, 10, 10, None, None]
    assert any(sc.passes(c) == [256] for c in sc.CASES) and any(sc.passes(c) == [256, 1] for c in sc.CASES)
    assert any(c["kernel"] == "steps" and c["H"] % 8 for c in sc.CASES) and any(c["path"] == "many_steps" and c["N"] > 32 for c in sc.CASES)
    assert {c["kind"] for c in sc.CASES if c["path"] == "forward"} == {"gru", "lstm", "rnn"}
    assert {c["kind"] for c in sc.CASES if c["n_freq"] == 161} == {"gru", "lstm", "rnn"}
    assert {1, 2, 20} <= {c["context"] for c in sc.CASES}


def test_the_table_has_the_chunk_edges_and_phases_it_claims():
    rows = [(c, p) for c in sc.CASES for s in c["scheds"] for p in sc.walk(c, s)]
    assert any(p["first"] and p["Tc"] == 10 for _, p in rows) and any(p["Tc"] == 16 and not p["last"] for _, p in rows)
    assert any(p["last"] and p["Tc"] == 23 for _, p in rows)
    assert {p["Tc"] & 1 for _, p in rows if not p["first"] and not p["last"]} == {0, 1}
    # the lookahead's kept rows limited by the chunk (Tc < context - 1) and by the context
    mid = [(c, p) for c, p in rows if p["nout"] and not p["last"]]
    assert any(p["Tc"] < c["context"] - 1 for c, p in mid) and any(p["Tc"] > c["context"] - 1 > 0 for c, p in mid)
    for c in sc.CASES:
        if c["name"].startswith("phase-"):
            scheds = sc.sessions(c)
            assert any(s[0] is None for s in scheds)                                                       # starts in a later round
            assert any(_restarts_with_state(s) for s in scheds)                                            # is_first, no is_last before it
            assert any(sum(1 for e in _chunks(s) if e[1]) == 2 and not _restarts_with_state(s) for s in scheds)      # two utterances, one handle
            plans = [{p["round"]: p for p in sc.walk(c, s)} for s in scheds]
            per_round = [[pl[r]["nout"] for pl in plans if r in pl] for r in range(max(len(s) for s in scheds))]
            assert any(0 in v and any(v) for v in per_round) and any(v and not any(v) for v in per_round)      # buffering beside emitting; nobody emits
    tiles = [c for c in sc.CASES if c["name"].startswith("tiles-")]
    assert {c["H"] for c in tiles} == {64, 264}
    for c in tiles:
        for r in range(1, 3):      # lengths differ inside every tile, and more chunks follow
            tcs = [sc.chunk_tc(*s[r]) for s in sc.sessions(c)]
            assert all(len(set(tcs[k:k + 32])) > 1 for k in range(0, c["N"], 32))


def test_both_clamps_of_the_lookahead_are_hit_and_no_case_is_flat():
    c, = [c for c in sc.CASES if c["name"].startswith("hot-look")]
    cfg, sd, _ = sc.make_case(c)
    lo, hi = [], []

    def probe(m):
        if m.la_buf is not None and hasattr(m, "la_pre"):
            lo.append(float(m.la_pre.min()))
            hi.append(float(m.la_pre.max()))
    ref = sc.run_reference(c, sd, cfg, lambda sd, cfg, s, m: f64.stream_model(sd, cfg), probe=probe)
    print("lookahead before the clip: min %.3g, max %.3g" % (min(lo), max(hi)))
    assert min(lo) < 0.0 and max(hi) > 20.0
    top = np.concatenate([y.max(axis=-1) for per in ref for y in per if y is not None])
    assert top.min() < 0.5 and top.max() > 0.9      # neither flat nor saturated throughout
    for c in sc.CASES:      # (also: every case's frames are what the chunk arithmetic says, in _baseline)
        assert _baseline(c["name"])[3] >= 1e-9, c["name"]
