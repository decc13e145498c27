"""The host half of dsmi_grammar (csrc/grammar_host.h: grammar_check, grammar_plan) under AddressSanitizer +
UndefinedBehaviorSanitizer on the CPU: `host_fuzz_asan grammarcheck`, the stand-alone program of tools/asan/host_fuzz.cpp that
tests/test_asan_host.py runs in its other modes, with nothing preloaded.  A sanitizer report or a crash fails the test."""
from test_asan_host import _run, exe      # noqa: F401  (exe: the module-scoped fixture that builds the program)


def test_grammar_argument_check_and_plan(exe):
    """Random calls whose pool of graphs lies in exactly sized heap arrays, each good or with one fault (a size, a graph index, an
    offset, a label, a predecessor, a weight, no start node, no final node): the code, the message, and for a good call the
    largest graph and the plan's numbers against the rules written out plainly; one node and one arc over the limits; the
    refusals on the numbers alone with no array at all."""
    out = _run(exe, ["grammarcheck", "7", "400"]).split()
    assert out[:4] == ["400", "grammar", "calls", "ok,"], out
    assert int(out[4]) > 100 and int(out[6]) > 100 and int(out[8]) > 50, out
