"""The conv kernels' frequency axis as pure functions (danspeech_amd/csrc/conv_rows.h), replayed on the CPU by
tools/dense_tiles_replay.cpp under AddressSanitizer + UndefinedBehaviorSanitizer (`make -C danspeech_amd/csrc tiles`): a
stand-alone program, nothing is loaded into python.

Kernel rows (`conv-rows`), for fi = 1 .. 200 and the geometries of conv1_split.hip (41 rows, pad 20, stride 2, 8 output rows per
workgroup) and conv_split.hip (21, 10, 2; 4 per workgroup), every output row f and kernel row kf: kf lies in `conv_rows_of`'s range
exactly when 0 <= SF f - PF + kf < fi; `conv_rows_wg`'s range is the union over the workgroup's live rows (f < fo), and empty past
fo; the first real kernel row of a row and of a workgroup is even in conv_split.hip's geometry, whose two-slot weight ring starts
every range in slot 0.

Tiles (`conv-check`), for grids of 1-9 t-tiles x 1-14 f-tiles x 1-12 clip tiles, on 256 CUs and on 4, with the labels drawing in
strict turns, one label drawing everything (all other shares stolen) and seeded random interleavings of the kernels' own steps
(TileTaker: first, ask, next, leave; every other random order also interleaves inside a step), launch after launch over the same
counter words: every tile is handed out exactly once and nothing past the end, every workgroup counts itself out once and the
last one leaves the words zero; a label's share is whole groups and its own tickets reproduce the static map (`conv-map`,
written out again below): the f-tiles of one (clip, t-tile) are consecutive tickets of one label, and with eight t-tiles label l
gets t-tile l clip by clip -- the workgroups the hardware gives XCD l from the grid (t-tiles, f-tiles, clips) of the static order."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "danspeech_amd", "csrc", "build", "dense_tiles_replay_asan")
N_GRIDS = 9 * 14 * 12


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


def test_kernel_row_ranges(exe):
    out = _run(exe, ["conv-rows"]).split()
    # at least every (fi, f, kf) of both geometries
    n = sum(((fi + 2 * pf - kf) // 2 + 1) * kf for kf, pf in ((41, 20), (21, 10)) for fi in range(1, 201))
    assert out[0] == "ok" and int(out[1]) >= n, out


def test_every_tile_once_in_every_draw_order(exe):
    out = _run(exe, ["conv-check", "20"]).split()
    assert out[0] == "ok" and int(out[1]) == N_GRIDS and int(out[3]) > 20 * 2 * sum(t * f * z for t in range(1, 10) for f in range(1, 15) for z in range(1, 13)), out


def _static_map(nt, nf, nz):
    """(label, ticket) -> (t-tile, f-tile, z): the groups (t-tile, z), t-tile first, dealt to the labels ceil(groups / 8) at a time."""
    groups = [(tt, z) for tt in range(nt) for z in range(nz)]
    share = (len(groups) + 7) // 8
    out = {}
    for gi, (tt, z) in enumerate(groups):
        for ft in range(nf):
            out[(gi // share, (gi % share) * nf + ft)] = (tt, ft, z)
    return out


def _hardware_map(nf, nz):
    """Eight t-tiles: the grid (8, nf, nz) of the static order, workgroups dealt to the XCDs by linear id x + 8 (y + nf z)."""
    out, slots = {}, [0] * 8
    for z in range(nz):
        for y in range(nf):
            for x in range(8):
                xcd = (x + 8 * (y + nf * z)) % 8
                out[(xcd, slots[xcd])] = (x, y, z)
                slots[xcd] += 1
    return out


@pytest.mark.parametrize("nt,nf,nz", [(1, 1, 1), (7, 11, 8), (8, 11, 64), (8, 6, 15), (2, 1, 3), (9, 14, 12), (3, 5, 1), (8, 1, 1)])
def test_own_share_is_the_static_map(exe, nt, nf, nz):
    got, order = {}, []
    for line in _run(exe, ["conv-map", str(nt), str(nf), str(nz)]).splitlines():
        label, ticket, tt, ft, z = (int(x) for x in line.split())
        got[(label, ticket)] = (tt, ft, z)
        order.append((label, ticket))
    ref = _static_map(nt, nf, nz)
    assert got == ref
    assert order == sorted(ref)
    assert sorted(ref.values()) == [(t, f, z) for t in range(nt) for f in range(nf) for z in range(nz)]
    for (label, ticket), (tt, ft, z) in got.items():          # f-neighbours: consecutive tickets of one label
        assert ft == ticket % nf and got[(label, ticket - ft)] == (tt, 0, z)
    if nt == 8:
        assert got == _hardware_map(nf, nz)
