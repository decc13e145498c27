"""The host half of dsmi_grammar_posterior (csrc/grammar_post_host.h: grammar_post_check, grammar_post_plan, grammar_post_pack)
under AddressSanitizer + UndefinedBehaviorSanitizer on the CPU: `host_fuzz_asan grammarpostcheck`, the stand-alone program of
tools/asan/host_fuzz.cpp that tests/test_asan_host.py runs in its other modes, with nothing preloaded.  A sanitizer report or a
crash fails the test."""
from test_asan_host import _run, exe      # noqa: F401  (exe: the module-scoped fixture that builds the program)


def test_grammar_posterior_check_plan_and_packing(exe):
    """Random calls whose pool of graphs lies in exactly sized heap arrays, each good or with one fault (a size, a label, a
    graph index, a short N_stride): the code and the message, and for a good call the plan's numbers and the packing -- every
    node's successors (the transposed arcs, an arc listed twice twice), the start lists and the label buckets -- against the
    rules written out plainly; one node and one arc over the limits, the cap on the stored trellises, and the refusals on the
    numbers alone with no array at all."""
    out = _run(exe, ["grammarpostcheck", "7", "400"]).split()
    assert out[:4] == ["400", "posterior", "calls", "ok,"], out
    assert int(out[4]) > 100 and int(out[6]) > 100 and int(out[8]) > 1000, out
