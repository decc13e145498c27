"""The batched edit distance off the GPU: the three references of tests/_edit_ref.py against each other and against the product's
own ``_edit_distance``, the identities of the four counts, the tie rule shown to be exercised, ``dsmi_edit_plan`` against
``np.lexsort`` of its documented rule, and the host half of ``dsmi_edit_distance`` (csrc/edit_host.h) under ASan + UBSan in the
stand-alone harness (tools/asan/host_fuzz.cpp editcheck).  No kernel runs."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from danspeech_amd.deepspeech.decoder import _edit_distance

import _edit_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "danspeech_amd", "csrc", "build", "host_fuzz_asan")

# the shapes of tests/test_gpu_edit.py's edge table (len_a, len_b)
SHAPES = [(la, lb) for la in (0, 1, 2, 63, 64, 65, 200) for lb in (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 130)]


@pytest.fixture(scope="module")
def brute_cases():
    rng = np.random.default_rng(3)
    cases = []
    for k in range(2400):
        symbols = 2 + k % 2
        a = rng.integers(0, symbols, rng.integers(0, 7)).tolist()
        b = rng.integers(0, symbols, rng.integers(0, 7)).tolist()
        cases.append((a, b, ref.all_optimal(a, b)))
    return cases


def test_brute_force_tuple_and_row_forms_agree(brute_cases):
    assert len(brute_cases) >= 2000
    for a, b, optimal in brute_cases:
        want = optimal[0]
        assert ref.tuple_dp(a, b) == want and ref.row_dp(a, b) == want, (a, b)
        assert want[0] == _edit_distance(a, b)
        assert all(v[0] == want[0] and v[1] >= want[1] for v in optimal)


def test_the_tie_rule_is_exercised(brute_cases):
    """More than one optimal count vector: the minimum distance alone does not fix the counts there."""
    assert sum(len(optimal) > 1 for _, _, optimal in brute_cases) >= 50


@pytest.mark.parametrize("symbols", [2, 4, 33])
def test_tuple_and_row_forms_agree_on_the_shape_table(symbols):
    rng = np.random.default_rng(symbols)
    for la, lb in SHAPES:
        a, b = rng.integers(0, symbols, la), rng.integers(0, symbols, lb)
        want = ref.tuple_dp(a.tolist(), b.tolist())
        assert ref.row_dp(a, b) == want, (la, lb)
        assert want[0] == _edit_distance(a.tolist(), b.tolist())
        d, s, dele, ins = want
        assert s + dele + ins == d and ins - dele == lb - la and min(s, dele, ins) >= 0
        swapped = ref.row_dp(b, a)
        assert swapped == (d, s, ins, dele), (la, lb)
    A, B = rng.integers(0, symbols, (9, 40)), rng.integers(0, symbols, (9, 70))
    assert ref.row_dp_batch(A, B).tolist() == [list(ref.tuple_dp(a.tolist(), b.tolist())) for a, b in zip(A, B)]


def _plan_by_lexsort(la, lb):
    la, lb = np.asarray(la, dtype=np.int64), np.asarray(lb, dtype=np.int64)
    seg = np.where(lb <= 16, 16, np.where(lb <= 32, 32, 64))
    work = (lb + 63) // 64 * (la + seg)
    index = np.arange(len(la))
    order = np.lexsort((index, -work, seg))                  # (the last key is the first criterion)
    return order[(la[order] > 0) & (lb[order] > 0)], seg


def test_edit_plan_is_the_documented_order():
    from danspeech_amd import _native
    rng = np.random.default_rng(9)
    for rep in range(60):
        N = int(rng.integers(1, 400))
        span = int(rng.choice([3, 20, 40, 200]))             # few distinct values: many ties
        la, lb = rng.integers(0, span, N), rng.integers(0, span, N)
        order, seg = _native.edit_plan(la, lb)
        want_order, want_seg = _plan_by_lexsort(la, lb)
        assert order.tolist() == want_order.tolist() and seg.tolist() == want_seg.tolist()
    la, lb = rng.integers(0, 20000, 300), rng.integers(0, 20000, 300)      # the plan itself takes any lengths
    la[::3], lb[::5] = la[1], 70
    order, seg = _native.edit_plan(la, lb)
    want_order, want_seg = _plan_by_lexsort(la, lb)
    assert order.tolist() == want_order.tolist() and seg.tolist() == want_seg.tolist()
    order, seg = _native.edit_plan([0, 5, 0], [3, 0, 0])
    assert order.tolist() == [] and seg.tolist() == [16, 16, 16]
    order, seg = _native.edit_plan([4096, 1, 1, 4096], [4096, 4096, 16, 17])
    assert seg.tolist() == [64, 64, 16, 32] and order.tolist() == [2, 3, 0, 1]
    for bad in (([-1, 2], [1, 1]), ([1, 2], [1, -4]), ([], [])):
        with pytest.raises(_native.DsmiError):
            _native.edit_plan(*bad)
    with pytest.raises(ValueError):
        _native.edit_plan([1, 2], [1])
    L = _native.lib()
    one = np.ones(1, dtype=np.int32)
    p = _native._np_ptr(one)
    assert L.dsmi_edit_plan(None, p, 1, p, p) < 0 and L.dsmi_edit_plan(p, None, 1, p, p) < 0
    assert L.dsmi_edit_plan(p, p, 1, None, p) < 0 and L.dsmi_edit_plan(p, p, 1, p, None) < 0 and L.dsmi_edit_plan(p, p, 0, p, p) < 0


def test_edit_host_half_under_sanitizers():
    """csrc/edit_host.h -- the argument check (the refusals on the numbers alone with null arrays), the plan, the packing of the
    upload and the unpacking of the counts -- on random calls in exactly sized heap arrays, in the stand-alone CPU program built
    with -fsanitize=address,undefined.  A sanitizer report or a broken rule fails the test."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "danspeech_amd", "csrc"), "asan"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:allocator_may_return_null=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([EXE, "editcheck", "7", "400"], capture_output=True, text=True, timeout=600, env=env)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = r.stdout.split()
    assert out[:4] == ["400", "edit", "calls", "ok,"] and int(out[4]) > 50 and int(out[6]) > 3000, out
