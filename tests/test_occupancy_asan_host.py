"""The host half of dsmi_occupancy (csrc/ctc_host.h: occ_check, and alt_place for the stored trellis) under AddressSanitizer +
UndefinedBehaviorSanitizer on the CPU: `host_fuzz_asan occcheck`, the stand-alone program of tools/asan/host_fuzz.cpp that
tests/test_asan_host.py runs in its other modes, with nothing preloaded.  A sanitizer report or a crash fails the test."""
from test_asan_host import _run, exe      # noqa: F401  (exe: the module-scoped fixture that builds the program)


def test_occupancy_argument_check_and_trellis_placing(exe):
    """Random calls in exactly sized heap arrays, each good or with one fault (a size, a clip index, a length, a token id): the
    code, the message, and for a good call the frames, the feasibility and the base of every candidate against the rules
    written out plainly; the stored trellis on either side of its cap; the refusals on the numbers alone with no array at all."""
    out = _run(exe, ["occcheck", "7", "400"]).split()
    assert out[:4] == ["400", "occupancy", "calls", "ok,"], out
    assert int(out[4]) > 100 and int(out[6]) > 100 and int(out[8]) > 50, out
