"""CPU checks of CTC transcript scoring: the numpy reference (tests/_score_ref.py) against a brute force over every frame
labelling, the likelihoods of all label sequences summing to one, float64's own rounding against np.longdouble, and the launch
order (dsmi_score_plan, host only) against np.lexsort.  No kernels run."""
import numpy as np
import pytest

import _align_ref as aref
import _score_ref as ref


# ---- the reference against a brute force
def test_reference_equals_brute_force():
    """T <= 6, C <= 4: every transcript some labelling collapses to (repeats and the empty one among them) to 1e-12 relative,
    and None for what no labelling collapses to."""
    rng = np.random.default_rng(3)
    checked = repeats = 0
    for T, C in ((1, 3), (2, 3), (3, 4), (5, 3), (5, 4), (6, 3), (6, 4)):
        p = rng.dirichlet(np.ones(C) * 0.5, size=T).astype(np.float32)
        sums = ref.brute_force(p)
        assert () in sums                                        # all blanks: the empty transcript
        for seq in ref.all_sequences(T, C):
            got = ref.forward(p, seq)
            if tuple(seq) not in sums:
                assert got is None and aref.min_frames(seq) > T
                continue
            want = sums[tuple(seq)]
            assert got is not None and abs(np.exp(got) - want) <= 1e-12 * want, (T, C, seq, float(np.exp(got)), want)
            checked += 1
            repeats += any(a == b for a, b in zip(seq, seq[1:]))
        assert ref.forward(p, [1, 2] * T) is None                # more tokens than frames
        assert ref.forward(p, [1] * (T // 2 + 1) + [1]) is None  # T // 2 + 2 equal tokens need 2 (T // 2) + 3 > T frames
    assert checked > 500 and repeats > 100
    assert ref.forward(np.zeros((0, 3), dtype=np.float32), []) == 0.0 and ref.forward(np.zeros((0, 3), dtype=np.float32), [1]) is None


def test_likelihoods_of_all_label_sequences_sum_to_one():
    """Every frame's softmax sums to 1 (here: to the float64 sum of its float32 entries), so the likelihoods of all label
    sequences sum to the product of the rows' sums."""
    rng = np.random.default_rng(4)
    for T, C, feasible in ((4, 3, 15), (3, 4, None), (5, 3, None)):
        p = rng.dirichlet(np.ones(C), size=T).astype(np.float32)
        lps = [ref.forward(p, seq) for seq in ref.all_sequences(T, C)]
        lps = [float(v) for v in lps if v is not None]
        if feasible is not None:
            assert len(lps) == feasible
        want = float(np.prod(p.astype(np.float64).sum(1)))
        assert abs(float(np.sum(np.exp(lps))) - want) <= 1e-12, (T, C, float(np.sum(np.exp(lps))), want)


# ---- float64's own rounding: the reference must sit far inside the bound the GPU is held to
@pytest.mark.parametrize("T, L, C, sharp", [(501, 150, 33, 3.0), (501, 150, 33, 8.0), (1501, 700, 33, 3.0), (64, 20, 33, 4.0),
                                            (200, 100, 3, 3.0)])
def test_float64_reference_against_long_double(T, L, C, sharp):
    rng = np.random.default_rng(T + L)
    p = ref.peaky(rng, T, C, sharp)
    t = [int(x) for x in rng.integers(1, C, size=L)]
    r64, rld = ref.forward(p, t), ref.forward(p, t, dtype=np.longdouble)
    assert r64 is not None and np.isfinite(r64)
    share = abs(float(np.longdouble(r64) - rld)) / ref.bound(T, rld)
    print("T %d L %d C %d sharp %g: logp %.6f, |float64 - long double| = %.3g of the bound" % (T, L, C, sharp, float(r64), share))
    assert share <= 1.0


# ---- dsmi_score_plan
def _lexsort(clip, frames, lens):
    n = np.arange(len(clip))
    return np.lexsort((n, -np.asarray(lens, dtype=np.int64), np.asarray(clip), -np.asarray(frames, dtype=np.int64)))


def test_plan_is_frames_then_clip_then_tokens_then_index():
    from danspeech_amd import _native
    assert _native.SCORE_MAX_TOKENS == 2048
    rng = np.random.default_rng(6)
    for N, B, hi in ((1, 1, 5), (7, 3, 4), (64, 5, 3), (500, 32, 40), (2048, 32, 200)):
        sizes = rng.integers(0, hi + 1, size=B)                   # few distinct values: clips tie on frames
        clip = rng.integers(0, B, size=N)
        lens = rng.integers(0, hi + 1, size=N)
        order = _native.score_plan(clip, sizes[clip], lens)
        np.testing.assert_array_equal(order, _lexsort(clip, sizes[clip], lens))
    # everything ties: the index decides
    np.testing.assert_array_equal(_native.score_plan([2] * 9, [10] * 9, [4] * 9), np.arange(9))
    # hand-worked: frames 9 before 5; within 9 frames clip 0 before clip 2; within a clip 3 tokens before 1; then the index
    order = _native.score_plan([1, 2, 0, 2, 0, 0], [5, 9, 9, 9, 9, 9], [8, 1, 1, 3, 3, 1])
    assert order.tolist() == [4, 2, 5, 3, 1, 0]


def test_plan_refuses_bad_arguments():
    from danspeech_amd import _native
    L = _native.lib()
    out = np.full(4, 7, dtype=np.int32)

    def call(clip=(0, 1), frames=(3, 4), lens=(1, 2), N=2, order=out, skip=None):
        arrs = [np.array(a, dtype=np.int32) for a in (clip, frames, lens)]
        ptrs = [None if skip == k else _native._np_ptr(a) for k, a in enumerate(arrs)]
        return L.dsmi_score_plan(ptrs[0], ptrs[1], ptrs[2], N, None if order is None else _native._np_ptr(order))

    for kw in (dict(N=0), dict(N=-1), dict(skip=0), dict(skip=1), dict(skip=2), dict(order=None), dict(clip=(0, -1)),
               dict(frames=(-3, 4)), dict(lens=(1, -2))):
        assert call(**kw) < 0, kw
        assert (out == 7).all(), kw
    assert call() == 2 and out[:2].tolist() == [1, 0] and (out[2:] == 7).all()
    with pytest.raises(_native.DsmiError):
        _native.score_plan([], [], [])
    with pytest.raises(ValueError):
        _native.score_plan([0], [1, 2], [0])
