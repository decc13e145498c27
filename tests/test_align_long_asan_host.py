"""The host half of dsmi_align_long (csrc/align_long_host.h: align_long_check, align_long_plan) under AddressSanitizer +
UndefinedBehaviorSanitizer on the CPU: `host_fuzz_asan alignlong`, the stand-alone program of tools/asan/host_fuzz.cpp that
tests/test_asan_host.py runs in its other modes, with nothing preloaded.  A sanitizer report or a crash fails the test."""
from test_asan_host import _run, exe      # noqa: F401  (exe: the module-scoped fixture that builds the program)


def test_align_long_argument_check_and_plan(exe):
    """Random calls with the transcript in an exactly sized heap array, each good or with one fault (a token id, a flag): the code,
    the message, and for a good call the feasibility and the geometry against the rules written out plainly; the checkpoint rows
    on either side of their cap; the refusals on the numbers alone with no array at all and nothing written."""
    out = _run(exe, ["alignlong", "7", "400"]).split()
    assert out[:4] == ["400", "align_long", "calls", "ok,"], out
    assert int(out[4]) > 100 and int(out[6]) > 50 and int(out[8]) > 10, out
