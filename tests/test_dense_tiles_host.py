"""The order in which the dense kernels hand out their output tiles (danspeech_amd/csrc/dense_tiles.h), replayed on the CPU by
tools/dense_tiles_replay.cpp under AddressSanitizer + UndefinedBehaviorSanitizer (`make -C danspeech_amd/csrc tiles`): a
stand-alone program, nothing is loaded into python.  Over the tile grids 1 x 1, 1 x 7, 3 x 3, 2 x 19, 251 x 19, 256 x 19 and
grids with a single n-unit, with every panel width, and with the labels drawing in strict turns, one label drawing everything
(all other shares stolen) and 1000 seeded random interleavings per grid: every tile is handed out exactly once and nothing past
the end.  Without stealing, a label's own tickets give the tiles of the static map the kernels had before (written out again
below), in the same order.

The replay drives the kernels' own TileTaker and tiles_leave (first, ask, next, leave) through plain counter words: the schedules
interleave whole steps, so other workgroups draw between a workgroup's early request and its redeem, and every other random order
also lets other workgroups step in front of any single add, peek or count of the stepping one (between a steal's peeks and its
add).  Every workgroup counts itself out exactly once, the last one leaves all nine words zero, and every order of a grid is one
more launch over the same words.  `switch` prints tile_switches, the rule of DSMI_DENSE_TILES / DSMI_CONV_TILES, held to a table
here."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "danspeech_amd", "csrc", "build", "dense_tiles_replay_asan")

GRIDS = [(1, 1), (1, 7), (3, 3), (2, 19), (251, 19), (256, 19), (5, 1), (251, 1)]


@pytest.fixture(scope="module")
def exe():
    if not shutil.which("g++"):
        pytest.skip("no g++")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "danspeech_amd", "csrc"), "tiles"], stdout=subprocess.DEVNULL)
    return EXE


def _run(exe, args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300, env=env)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r.stdout


def _static_map(mtiles, ntiles2, pn2):
    """The static kernels' blockIdx.x -> tile, as (label, slot) -> (m-tile, n-unit): every label ceil(total / 8) slots."""
    total = ntiles2 * mtiles
    share = (total + 7) // 8
    out = {}
    for bid in range(8 * ((total + 7) // 8)):
        idx = (bid & 7) * share + (bid >> 3)
        if (bid >> 3) >= share or idx >= total:
            continue
        panel = idx // (pn2 * mtiles)
        rem = idx - panel * (pn2 * mtiles)
        pw = min(pn2, ntiles2 - panel * pn2)
        mt = rem // pw
        out[(bid & 7, bid >> 3)] = (mt, panel * pn2 + (rem - mt * pw))
    return out


def test_every_tile_once_in_every_draw_order(exe):
    out = _run(exe, ["check", "1000"]).split()
    assert out[0] == "ok" and int(out[1]) >= sum(max(n, 3) + 1 for _, n in GRIDS) and int(out[3]) > 1000 * sum(m * n for m, n in GRIDS), out


@pytest.mark.parametrize("mtiles,nunits", GRIDS)
def test_own_share_is_the_static_map(exe, mtiles, nunits):
    for pn in range(1, max(nunits, 3) + 2):
        got = {}
        order = []
        for line in _run(exe, ["map", str(mtiles), str(nunits), str(pn)]).splitlines():
            label, ticket, mt, nu = (int(x) for x in line.split())
            got[(label, ticket)] = (mt, nu)
            order.append((label, ticket))
        ref = _static_map(mtiles, nunits, pn)
        assert got == ref, (mtiles, nunits, pn)
        assert order == sorted(ref), (mtiles, nunits, pn)          # tickets 0, 1, 2, ... of a label: its slots in order
        assert sorted(ref.values()) == [(m, n) for m in range(mtiles) for n in range(nunits)]


def _switch_rule(dense, conv, token_on):
    """The documented rule, written out again: an empty text counts as not set, "0" is the static order, any other text by demand."""
    def is_set(t):
        return t is not None and t != ""
    gemm = (dense != "0") if is_set(dense) else not token_on
    convs = (conv != "0") if is_set(conv) else (is_set(dense) and dense != "0")
    return gemm, convs


# (DSMI_DENSE_TILES, DSMI_CONV_TILES, dense token on) -> (the GEMM by demand, the convs by demand); None: not set
SWITCH_TABLE = [
    ((None, None, False), (True, False)),       # nothing set: the GEMM by demand only with the token off, the convs static
    ((None, None, True), (False, False)),
    (("", "", False), (True, False)),           # empty texts count as not set
    (("", "", True), (False, False)),
    (("0", None, False), (False, False)),       # DSMI_DENSE_TILES=0: the static order in both, whatever the token is
    (("0", None, True), (False, False)),
    (("1", None, False), (True, True)),         # any other text: by demand in both
    (("1", None, True), (True, True)),
    (("x", None, True), (True, True)),
    (("00", None, True), (True, True)),         # only the text "0" means off
    ((None, "1", True), (False, True)),         # DSMI_CONV_TILES decides for the convs alone
    ((None, "1", False), (True, True)),
    ((None, "0", False), (True, False)),
    (("0", "1", False), (False, True)),
    (("1", "0", True), (True, False)),
    (("1", "", True), (True, True)),            # an empty DSMI_CONV_TILES leaves the convs to DSMI_DENSE_TILES
    (("0", "00", True), (False, True)),
    (("", "x", True), (False, True)),
]


def test_switch_table(exe):
    texts = [None, "", "0", "1", "00", "x"]
    cases = [(d, c, t) for d in texts for c in texts for t in (False, True)]
    assert all(case in cases for case, _ in SWITCH_TABLE)
    args = []
    for d, c, t in cases:
        args += ["-" if d is None else d, "-" if c is None else c, "1" if t else "0"]
    lines = _run(exe, ["switch"] + args).splitlines()
    assert len(lines) == len(cases)
    got = {case: tuple(x == "1" for x in line.split()) for case, line in zip(cases, lines)}
    for case, want in SWITCH_TABLE:
        assert got[case] == want, (case, got[case], want)
    for case in cases:
        assert got[case] == _switch_rule(*case), (case, got[case])
