"""Long-form CTC forced alignment on the CPU: the numpy reference (tests/_align_long_ref.py) against tests/_align_ref.py and a
brute force, the tiled scheme of csrc/align_long.hip emulated in numpy against the plain recurrence bit for bit, and the host
half of dsmi_align_long (csrc/align_long_host.h) through the library: the plan against a table written out by hand, the
refusals on the numbers, the workspace on either side of its cap.  No GPU."""
import itertools

import numpy as np
import pytest

import _align_long_ref as lr
import _align_ref as ar

FLAGS = list(itertools.product((False, True), repeat=2))


def _probs(rng, T, C, kind):
    if kind == "uniform":
        return np.full((T, C), 1.0 / C, dtype=np.float32)
    x = rng.standard_normal((T, C)) * 3.0
    e = np.exp(x - x.max(1, keepdims=True))
    return (e / e.sum(1, keepdims=True)).astype(np.float32)


def _same(a, b):
    if a is None or b is None:
        assert a is None and b is None
        return
    assert np.array_equal(a["path"], b["path"])
    assert np.array_equal(a["spans"], b["spans"])
    assert a["token_probs"].tobytes() == b["token_probs"].tobytes()
    assert np.float32(a["path_logp"]).tobytes() == np.float32(b["path_logp"]).tobytes()


@pytest.mark.parametrize("kind", ["uniform", "peaky"])
def test_flags_off_is_the_clip_reference_bit_for_bit(kind):
    rng = np.random.default_rng(11)
    for T, L in [(1, 0), (1, 1), (2, 1), (7, 3), (30, 9), (30, 15), (41, 20), (5, 4)]:
        p = _probs(rng, T, 4, kind)
        tg = rng.integers(1, 4, size=L)
        _same(lr.viterbi(p, tg), ar.viterbi(p, tg))
        r64 = lr.viterbi(p, tg, dtype=np.float64)
        if r64 is not None:
            assert np.array_equal(r64["path"], ar.viterbi(p, tg, dtype=np.float64)["path"])


@pytest.mark.parametrize("W,F", [(8, 4), (9, 3), (6, 5)])
@pytest.mark.parametrize("kind", ["uniform", "peaky"])
def test_tiled_scheme_is_the_plain_recurrence_bit_for_bit(W, F, kind):
    """Every flag combination, L = 0, frames below, at and above multiples of F, states below, at and above multiples of W: the
    path, the spans, the means, the score and every checkpoint row that the plain recurrence also has."""
    rng = np.random.default_rng(W * 100 + F)
    sizes = sorted(set(S for S in (1, 3, W - 1, W, W + 1, 2 * W + 1, 3 * W + 2) if S % 2 == 1 and S >= 1))
    done = 0
    for T in (1, 2, F, F + 1, F + 2, 2 * F + 1, 3 * F - 1, 4 * F + 3, 3 * W + 7):
        for S in sizes:
            L = (S - 1) // 2
            p = _probs(rng, T, 4, kind)
            tg = rng.integers(1, 4, size=L)
            for lead, tail in FLAGS:
                want = lr.viterbi(p, tg, lead, tail)
                got = lr.tiled(p, tg, W, F, lead, tail)
                _same(got, want)
                if want is None:
                    continue
                done += 1
                assert not np.isnan(got["rows"]).any(), "a checkpoint cell that no tile stored"
                unskipped = lr.tiled(p, tg, W, F, lead, tail, skip_unreached=False)
                assert got["rows"].tobytes() == unskipped["rows"].tobytes(), "a skipped tile must hold what the recurrence gives"
    assert done > 60       # (the rest were infeasible: more tokens than frames)


def test_steepest_and_flattest_path_through_the_tiles():
    """T = L frames of pairwise different neighbours: the only path moves two states per frame, through every halo and the whole
    backtrace window.  Then a long blank stretch: the path sits in one state across whole frame tiles."""
    W, F = 8, 4
    L = 3 * W
    tg = np.array([1 + k % 3 for k in range(L)])
    p = np.full((L, 4), 0.1 / 3, dtype=np.float32)
    p[np.arange(L), tg] = 0.9
    for run in (lambda: lr.viterbi(p, tg), lambda: lr.tiled(p, tg, W, F)):
        r = run()
        assert np.isfinite(r["path_logp"])
        assert np.array_equal(r["spans"], np.stack([np.arange(L), np.arange(L) + 1], 1))
    T = 3 * F + 5
    q = np.full((T + 3, 4), 0.02 / 3, dtype=np.float32)
    q[:T, 0] = 0.98
    for k, c in enumerate((2, 1, 3)):
        q[T + k] = 0.02 / 3
        q[T + k, c] = 0.98
    _same(lr.tiled(q, [2, 1, 3], W, F), lr.viterbi(q, [2, 1, 3]))
    assert np.array_equal(lr.viterbi(q, [2, 1, 3])["spans"], [[T, T + 1], [T + 1, T + 2], [T + 2, T + 3]])


def test_reference_agrees_with_the_brute_force():
    rng = np.random.default_rng(5)
    n = 0
    for T, tg in [(1, []), (3, []), (4, [1]), (5, [1, 2]), (5, [1, 1]), (6, [2, 1]), (6, [1, 1, 2]), (3, [1, 1])]:
        for kind in ("peaky", "uniform"):
            p = _probs(rng, T, 3, kind)
            for lead, tail in FLAGS:
                want = lr.brute_force(p, tg, lead, tail)
                got = lr.viterbi(p, tg, lead, tail, dtype=np.float64)
                if got is None:
                    assert want is None
                    continue
                n += 1
                assert abs(float(got["path_logp"]) - want) < 1e-12 * max(1.0, abs(want)), (T, tg, lead, tail)
                # the returned path itself scores what it claims: its costly frames in float64
                lab = ar.state_labels(tg)[got["path"]]
                costly = np.ones(T, dtype=bool)
                if lead:
                    costly &= got["path"] != 0
                if tail:
                    costly &= got["path"] != 2 * len(tg)
                assert abs(ar.rescore64(p[costly], lab[costly]) - want) < 1e-12 * max(1.0, abs(want))
    assert n > 40


# ---- the host half, through the library
PLAN_TABLE = [
    # T, L -> W, F, state tiles, frame tiles, checkpoint rows, bytes
    ((1, 0), (384, 64, 1, 0, 1, 4)),
    ((2, 0), (384, 64, 1, 1, 2, 8)),
    ((65, 191), (384, 64, 1, 1, 2, 2 * 383 * 4)),
    ((66, 192), (384, 64, 2, 2, 3, 3 * 385 * 4)),
    ((129, 383), (384, 64, 2, 2, 3, 3 * 767 * 4)),
    ((130, 384), (384, 64, 3, 3, 4, 4 * 769 * 4)),
    ((180000, 50000), (384, 64, 261, 2813, 2814, 1125611256)),
    ((1 << 22, 8191), (384, 64, 43, 65536, 65537, 65537 * 16383 * 4)),
]


def test_plan_against_a_table_written_by_hand():
    from danspeech_amd import _native
    keys = ("W", "F", "state_tiles", "frame_tiles", "rows", "bytes")
    for (T, L), want in PLAN_TABLE:
        got = _native.align_long_plan(T, L)
        assert tuple(got[k] for k in keys) == want, (T, L, got)
    assert PLAN_TABLE[-1][1][5] <= 4 << 30


def test_plan_refuses_what_the_numbers_refuse():
    import ctypes
    from danspeech_amd import _native
    L = _native.lib()
    info = (ctypes.c_int64 * 6)(*([-7] * 6))
    INVALID, CAPACITY = _native.DSMI_ERR_INVALID, _native.DSMI_ERR_CAPACITY
    for T, n, want in [(0, 0, INVALID), (-3, 5, INVALID), (10, -1, INVALID), (10, (1 << 20) + 1, CAPACITY), ((1 << 22) + 1, 3, CAPACITY),
                       (1 << 22, 8192, CAPACITY),                  # 65537 rows of 16385 floats: just above 4 GiB
                       (1 << 22, 1 << 20, CAPACITY)]:
        assert L.dsmi_align_long_plan(T, n, info) == want, (T, n)
        assert list(info) == [-7] * 6, "a refused plan writes nothing"
    assert L.dsmi_align_long_plan(10, 3, None) == INVALID
    assert L.dsmi_align_long_plan(1 << 22, 8191, info) == 0 and info[5] == 65537 * 16383 * 4      # just below the cap
    assert L.dsmi_align_long_plan(10, 1 << 20, info) == 0                                          # the limits themselves pass
