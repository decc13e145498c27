"""What one chunk means for one streaming session (danspeech_amd/csrc/stream_host.h: stream_pass_plan, stream_pass_commit), checked
on the CPU.  `make -C danspeech_amd/csrc asan` builds tools/asan/host_fuzz.cpp with the product's header under AddressSanitizer +
UndefinedBehaviorSanitizer; its streampass mode runs one session's schedule per input line from a fresh handle and prints, per pass,
the code, every StreamPass field and the flags after the pass (and fails by itself if a refusal wrote anything).

The frame counts are held to `_reference_pass` below, a statement of the reference's MaskConvStream / LookaheadStream as frame
counting alone that shares nothing with stream_host.h; it is itself pinned to tests/_f64_ref.py stream_model on a handful of schedules."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _stream_cases as sc
from danspeech_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "danspeech_amd", "csrc", "build", "host_fuzz_asan")
PASS_FIELDS = ("padl", "padr", "ctxl", "tin0", "tin1", "to0", "to1", "buffering", "ncat", "nout", "keep")
FLAG_FIELDS = ("has_left", "has_hidden", "la_init", "la_rows", "pbase0", "pbase1")
NO_FIRST = "the first chunk of an utterance must be passed with is_first (MaskConvStream has no left context)"
TOO_SHORT = "chunk too short for the conv context"
NO_FRAMES = "lookahead: fewer buffered frames than the context (torch raises here too)"
NO_ROOM = "probs slot smaller than the frames this pass yields"
BIG = 1 << 20


@pytest.fixture(scope="module")
def exe():
    if not shutil.which("g++"):
        pytest.skip("no g++")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "danspeech_amd", "csrc"), "asan"], stdout=subprocess.DEVNULL)
    return EXE


def _run(exe, args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:allocator_may_return_null=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=900, env=env)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r.stdout


def _plans(exe, tmp_path, rows):
    """rows: (context, T_out_cap, have_probs, [(T, first, last)]) -> per row a list of passes: dict(code, why | StreamPass fields, flags)"""
    path = str(tmp_path / "schedules.txt")
    with open(path, "w") as f:
        for ctx, cap, have, sched in rows:
            f.write("%d %d %d" % (ctx, cap, have) + "".join(" | %d %d %d" % (T, first, last) for T, first, last in sched) + "\n")
    out = _run(exe, ["streampass", path]).splitlines()
    assert len(out) == len(rows)
    res = []
    for text, row in zip(out, rows):
        passes = []
        for item in text.split(" | "):
            head, _, flags = item.rpartition(" : ")
            p = dict(flags=dict(zip(FLAG_FIELDS, (int(v) for v in flags.split()))))
            code, _, rest = head.partition(" ")
            p["code"] = int(code)
            if p["code"]:
                assert rest.startswith("why=")
                p["why"] = rest[4:]
            else:
                v = [int(x) for x in rest.split()]
                assert len(v) == len(PASS_FIELDS)
                p.update(zip(PASS_FIELDS, v))
            passes.append(p)
        assert len(passes) == len(row[3])
        res.append(passes)
    return res


# ---- the reference's modules as frame counting (danspeech/deepspeech/model.py of the reference) --------------------------------
# MaskConvStream.left_1 / left_2 (:166-167); the steps BatchRNNStream.previous_hidden has taken (:213, :232-236; None: no state); the
# rows of LookaheadStream.hidden_states_buffer (:250-251)
FRESH = dict(left=(False, False), steps=None, buf=None)


def _reference_pass(state, context, T, first, last, cap=BIG, have_probs=True):
    """One streaming_forward (model.py:517-537) on `state`: (new state, dict(Tc, nout, buf, left, steps)) or (state, the reason for
    a refusal).
    The reference raises for NO_FIRST (torch.cat with None, :188) and NO_FRAMES (a Conv1d input shorter than its kernel, :270);
    TOO_SHORT is the project's own: the reference would keep a tail of fewer than ten frames (:195) and glue that; so is NO_FIRST
    after an is_last, where the reference would glue the finished utterance's tail.  NO_ROOM has no counterpart there."""
    t, left = T, list(state["left"])
    for layer in (0, 1):                       # MaskConvStream.forward, :177-199: i == 0 and i == 3 of the Sequential
        if first:
            t += 5                             # :180-181  F.pad(x, (5, 0))
        elif last:
            t += 5                             # :182-183  F.pad(x, (0, 5)) -- elif: a chunk that is both is padded in front only
        if not first:
            if not left[layer]:
                return state, NO_FIRST         # :185-191  torch.cat([self.left_1, x]) with left_1 None
            t += 10
        if not last:
            if t < 10:
                return state, TOO_SHORT        # :193-197  x[:, :, :, -10:] holds fewer than ten frames
            left[layer] = True
        else:
            left[layer] = False                # the project's own: after is_last nothing may be glued (the reference keeps the stale tail)
        stride = (2, 1)[layer]                 # :448, :451  Conv2d(kernel (., 11), stride (2, 2) then (2, 1), padding (., 5))
        t = (t + 2 * 5 - 11) // stride + 1
        if t < 1:
            return state, TOO_SHORT
    Tc = t
    steps = None if last else (state["steps"] or 0) + Tc      # BatchRNNStream.forward, :224-236: is_last drops the state, nothing else does
    carried = dict(left=tuple(left), steps=steps)
    if state["buf"] is None or first:          # LookaheadStream.forward, :256-259: buffer the chunk, a dummy comes back
        return dict(carried, buf=Tc), dict(carried, Tc=Tc, nout=0, buf=Tc)
    ncat = state["buf"] + Tc                   # :261
    buf = len(range(Tc)[-(context - 1):])      # :263  x[-(context - 1):] -- the slice itself, -0 included
    if last:
        ncat += context - 1                    # :267-268  F.pad(out, (0, context - 1))
    nout = ncat - context + 1                  # :270  Conv1d(kernel_size=context, padding=0)
    if nout < 1:
        return state, NO_FRAMES
    if not have_probs or cap < nout:
        return state, NO_ROOM
    if last:
        buf = None                             # :275-277
    return dict(carried, buf=buf), dict(carried, Tc=Tc, nout=nout, buf=buf or 0)


def _reference_walk(context, sched, cap=BIG, have_probs=True):
    """the passes of a schedule up to and including the first refused one: [dict(Tc, nout, buf, left, steps) or a reason]"""
    state, out = FRESH, []
    for T, first, last in sched:
        state, res = _reference_pass(state, context, T, first, last, cap, have_probs)
        out.append(res)
        if isinstance(res, str):
            break
    return out


def _agree(got, want, what):
    """one schedule: the plan's passes against the statement's, refusal included"""
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        if isinstance(w, str):
            assert g["code"] != 0 and g["why"] == w, (what, k, g, w)
        else:
            assert g["code"] == 0 and (g["to1"], g["nout"], g["flags"]["la_rows"]) == (w["Tc"], w["nout"], w["buf"]), (what, k, g, w)
            # the flags: a tail to glue, a state to continue from, and the parity of the steps it has taken (rnn_step.hip: step + pbase)
            par = (w["steps"] or 0) & 1
            assert g["flags"] == dict(has_left=int(all(w["left"])), has_hidden=int(w["steps"] is not None), la_init=int(w["buf"] > 0 or w["nout"] == 0),
                                      la_rows=w["buf"], pbase0=par, pbase1=par), (what, k, g, w)


SCHEDULES = [                                   # (context, schedule): every chunk edge, an is_first with no is_last before it, contexts 1 and 20
    (8, sc.utt(53, 39, 40, 17) + sc.utt(47, 41, 21)),
    (20, sc.SHORT + [(5, True, True), (6, True, False), (1, False, True)]),
    (1, [(53, True, False), (39, False, False), (45, True, False), (40, False, False), (17, False, True)]),
    (2, sc.utt(5, 1, 41, 1)),
]


@pytest.mark.parametrize("context,sched", SCHEDULES)
def test_the_statement_counts_as_the_float64_model_does(context, sched):
    import _f64_ref as f64

    class Probe(f64.stream_model):
        def lookahead(self, x, is_first, is_last):
            self.tc = x.shape[0]
            return super().lookahead(x, is_first, is_last)

    c = sc._case("count", "gru", 64, 1, [sched], context=context)
    cfg, sd, _ = sc.make_case(c)
    m = Probe(sd, cfg)
    want = _reference_walk(context, sched)
    assert len(want) == len(sched) and not any(isinstance(w, str) for w in want)
    steps = 0
    for k, ((T, first, last), w) in enumerate(zip(sched, want)):
        y = m.forward(sc.feat(c, 0, k, T), first, last)
        got = dict(Tc=m.tc, nout=0 if y is None else y.shape[1], buf=0 if m.la_buf is None else m.la_buf.shape[0],
                   steps=None if m.hidden[0] is None else steps + m.tc)
        steps = got["steps"] or 0
        assert got == {key: w[key] for key in got}, (k, got, w)
        if not last:      # the tail to glue: kept by the model exactly where the statement says there is one (after is_last the
            assert w["left"] == tuple(v is not None and v.shape[3] == 10 for v in m.left), (k, w)      # model keeps a stale one)


def _grid(context):
    """Schedules of up to four passes, grown pass by pass from the prefixes the statement accepts (a refused pass ends its schedule
    and stays in it).  The last pass of a schedule of up to three takes every T in 1..48 and every (first, last); the passes before
    it, and the fourth, take the T at which something changes: 1 (the shortest), 5 (the shortest first chunk), 40 / 41 (odd / even
    Tc: 35 / 36)."""
    every = [(T, f, l) for T in range(1, 49) for f in (True, False) for l in (True, False)]
    some = [(T, f, l) for T in (1, 5, 40, 41) for f in (True, False) for l in (True, False)]
    rows, want, level = [], [], [((), FRESH, ())]
    for depth in range(4):
        grown = []
        for sched, state, res in level:
            for e in (every if depth < 3 else some):
                st, r = _reference_pass(state, context, *e)
                rows.append((context, BIG, 1, sched + (e,)))
                want.append(res + (r,))
                if not isinstance(r, str) and e in some:
                    grown.append((sched + (e,), st, res + (r,)))
        level = grown
    return rows, want


@pytest.mark.parametrize("context", [1, 2, 8, 20])
def test_frame_counts_over_the_grid(exe, tmp_path, context):
    rows, want = _grid(context)
    scheds = {r[3] for r in rows}
    assert len(rows) > 20000
    assert any(len(s) >= 2 and s[1][1] and not s[0][2] for s in scheds)                      # an is_first with no is_last before it
    assert ((5, True, False), (1, False, False), (1, False, True)) in scheds                 # _stream_cases.SHORT
    assert {w[-1] for w in want if isinstance(w[-1], str)} == {NO_FIRST, TOO_SHORT}          # (contexts up to 20 never run out of frames)
    for g, w, r in zip(_plans(exe, tmp_path, rows), want, rows):
        _agree(g, w, r)


def test_every_schedule_of_the_case_table(exe, tmp_path):
    todo = {}
    for c in sc.CASES:
        for sched in c["scheds"]:
            todo.setdefault((c["context"], tuple(e for e in sched if e is not None)), (c, sched))
    keys = sorted(todo)
    assert len(keys) >= 12
    got = _plans(exe, tmp_path, [(ctx, BIG, 1, sched) for ctx, sched in keys])
    for key, passes in zip(keys, got):
        c, sched = todo[key]
        walk = sc.walk(c, sched)
        assert [p["code"] for p in passes] == [0] * len(walk), key
        assert [(p["nout"], p["to1"]) for p in passes] == [(w["nout"], w["Tc"]) for w in walk], key
        assert [p["ncat"] - p["to1"] if not p["buffering"] else 0 for p in passes] == [w["la_rows"] for w in walk], key
        _agree(passes, _reference_walk(key[0], key[1]), key)


def test_each_refusal_at_its_smallest_input(exe, tmp_path):
    I, Cap = _native.DSMI_ERR_INVALID, _native.DSMI_ERR_CAPACITY
    first5, mid1 = (5, True, False), (1, False, False)
    rows = [
        (1, BIG, 1, [mid1, (1, False, True)]),                    # no is_first on a fresh handle, context 1, T 1
        (1, BIG, 1, [first5, (17, False, True), mid1]),           # ... and on a finished one
        (1, BIG, 1, [(4, True, False), (1, True, False), first5]),      # a first chunk below five frames
        (27, BIG, 1, [first5, mid1]),                             # Tc 10 buffered + 16 new = 26 rows: the smallest context that has too few
        (26, BIG, 1, [first5, mid1]),                             # ... and the one below it yields one frame
        (1, 25, 1, [first5, mid1, mid1]),                         # context 1, T 1: 26 frames, room for 25
        (1, 26, 1, [first5, mid1]),                               # ... and room for 26
        (8, BIG, 0, [first5, mid1]),                              # no probs at all
        (8, 0, 0, [first5, (5, True, True)]),                     # ... which a pass that only buffers does not need
    ]
    got = _plans(exe, tmp_path, rows)
    fresh = dict(zip(FLAG_FIELDS, (0,) * 6))
    refused = lambda p, code, why: (p["code"], p.get("why")) == (code, why)
    assert all(refused(p, I, NO_FIRST) and p["flags"] == fresh for p in got[0])
    assert got[1][1]["code"] == 0 and got[1][1]["flags"] == fresh and refused(got[1][2], I, NO_FIRST) and got[1][2]["flags"] == fresh
    assert refused(got[2][0], I, TOO_SHORT) and refused(got[2][1], I, TOO_SHORT) and got[2][1]["flags"] == fresh and got[2][2]["code"] == 0
    assert (got[2][2]["to1"], got[2][2]["tin0"], got[2][2]["tin1"]) == (10, 10, 10)
    for row in (3, 5, 7):                                          # the flags after the refusal are the flags before it
        assert got[row][0]["code"] == 0 and got[row][0]["flags"] == dict(fresh, has_left=1, has_hidden=1, la_init=1, la_rows=10)
        assert got[row][1]["flags"] == got[row][0]["flags"]
    assert refused(got[3][1], I, NO_FRAMES) and (got[4][1]["code"], got[4][1]["nout"], got[4][1]["ncat"]) == (0, 1, 26)
    assert refused(got[5][1], Cap, NO_ROOM) and refused(got[5][2], Cap, NO_ROOM) and got[5][2]["flags"] == got[5][0]["flags"]
    assert (got[6][1]["code"], got[6][1]["nout"], got[6][1]["keep"], got[6][1]["flags"]["la_rows"]) == (0, 26, 16, 16)
    assert refused(got[7][1], Cap, NO_ROOM)
    assert [p["code"] for p in got[8]] == [0, 0] and got[8][1]["flags"] == dict(fresh, la_init=1, la_rows=10)
    for (ctx, cap, have, sched), passes in zip(rows, got):        # the statement refuses where the plan does, for the same reason
        want = _reference_walk(ctx, sched, cap, bool(have))
        _agree(passes[:len(want)], want, (ctx, cap, have, sched))
