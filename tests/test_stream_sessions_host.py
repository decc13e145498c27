"""CPU checks of the many-session streaming surface: the cut plan that stream_recording and stream_recordings share, the
round scheduler of stream_recordings, and the argument refusals of dsmi_stream_forward_many that happen before any HIP call."""
import ctypes

import numpy as np

from danspeech_amd.stream_plan import stream_cut_plan, stream_rounds


def _reference_cuts(n, step, ctx=20, s10=160):
    """the loop of the reference's real_time_streaming (Recognizer.py:598-667), restated over sample positions"""
    general = s10 * 2 + s10 * ((ctx - 1) * 2 - 1)
    first = general + s10 * 15
    out, lo, pos, first_pass = [], 0, 0, True
    while pos < n:
        pos = min(pos + step, n)
        last = pos >= n
        if first_pass:
            if last:
                pass
            elif pos - lo >= first:
                out.append((lo, pos, True, False)); first_pass = False; lo = pos
        elif last or pos - lo >= general:
            out.append((lo, pos, False, last)); lo = pos
    return out


def test_cut_plan_matches_the_reference_schedule():
    general = 160 * 2 + 160 * 37
    first = general + 160 * 15
    for n in (0, 100, first - 1, first, first + 1, 16000, 16000 * 4 + 333, 48000):
        for step in (512, 1024, 2048, 4000):
            plan = stream_cut_plan(n, step, 20, 160)
            assert plan == _reference_cuts(n, step)
            if plan:
                assert plan[0][2] and not plan[0][3]                     # the first pass is never the last
                assert plan[-1][1] == n and plan[-1][3]                   # the final part closes the utterance
                assert all(p[1] - p[0] >= general for p in plan[1:-1])
                assert plan[0][1] - plan[0][0] >= first
    # an utterance that ends before its first pass is discarded
    assert stream_cut_plan(first - 1, 1024, 20, 160) == []
    assert stream_cut_plan(5000, None, 20, 160) == stream_cut_plan(5000, 1024, 20, 160)


def test_round_scheduler_order_and_termination():
    plans = [stream_cut_plan(n, 1024, 20, 160) for n in (16000, 0, 40000, 9000, 70000)]
    rounds = stream_rounds(plans)
    assert len(rounds) == max(len(p) for p in plans)
    seen = {k: [] for k in range(len(plans))}
    for r in rounds:
        ks = [k for k, _ in r]
        assert ks == sorted(set(ks))                                    # never twice in one round, in index order
        for k, c in r:
            seen[k].append(c)
    for k, p in enumerate(plans):
        assert seen[k] == p                                              # each session in its own order, all of it
    assert stream_rounds([]) == [] and stream_rounds([[]]) == []


def test_forward_many_refuses_bad_arguments_without_gpu():
    from danspeech_amd import _native
    L = _native.lib()
    T = np.array([39], dtype=np.int32)
    flags = np.zeros(1, dtype=np.int32)
    tout = np.zeros(1, dtype=np.int32)
    one = (ctypes.c_void_p * 1)(None)
    p = _native._np_ptr
    assert L.dsmi_stream_forward_many(one, 0, one, p(T), p(flags), p(flags), None, 0, p(tout), None) == _native.DSMI_ERR_INVALID
    assert L.dsmi_stream_forward_many(None, 1, one, p(T), p(flags), p(flags), None, 0, p(tout), None) == _native.DSMI_ERR_INVALID
    assert L.dsmi_stream_forward_many(one, 1, None, p(T), p(flags), p(flags), None, 0, p(tout), None) == _native.DSMI_ERR_INVALID
    assert L.dsmi_stream_forward_many(one, 1, one, p(T), p(flags), p(flags), None, 0, None, None) == _native.DSMI_ERR_INVALID
    assert L.dsmi_stream_forward_many(one, _native.STREAM_MANY_MAX + 1, one, p(T), p(flags), p(flags), None, 0, p(tout), None) \
        == _native.DSMI_ERR_INVALID
    assert b"n outside" in L.dsmi_stream_last_error(None)
    # a null handle is named by its index
    assert L.dsmi_stream_forward_many(one, 1, one, p(T), p(flags), p(flags), None, 0, p(tout), None) == _native.DSMI_ERR_INVALID
    assert b"session 0" in L.dsmi_stream_last_error(None)
