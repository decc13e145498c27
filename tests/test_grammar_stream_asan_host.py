"""The host half of streaming grammar decoding (csrc/grammar_stream_host.h: grammar_stream_plan, grammar_heavy_list,
grammar_stream_check) under AddressSanitizer + UndefinedBehaviorSanitizer on the CPU: `host_fuzz_asan grammarstreamcheck`, the
stand-alone program of tools/asan/host_fuzz.cpp that tests/test_asan_host.py runs in its other modes, with nothing preloaded.  A
sanitizer report or a crash fails the test."""
from test_asan_host import _run, exe      # noqa: F401  (exe: the module-scoped fixture that builds the program)


def test_grammar_stream_plan_and_advance_check(exe):
    """The plan's numbers and refusals against the rules written out plainly, the heavy list of random pools, and random advance
    calls in exactly sized heap arrays, each good or with one fault (n, a handle twice, another net, a frame count, missing rows,
    a mode, an ended stream, max_frames, P_stride, a NULL output, the result cap): the code and the message."""
    out = _run(exe, ["grammarstreamcheck", "11", "600"]).split()
    assert out[:5] == ["600", "grammar", "stream", "calls", "ok,"], out
    assert int(out[5]) > 150 and int(out[7]) > 150 and int(out[9]) > 100, out
