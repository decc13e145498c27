"""The numpy reference of CTC token confidence (tests/_alt_ref.py) on the CPU: its forward-backward factorisation against the
plain forward recurrence (_score_ref.forward) run on every variant transcript itself, float64's own rounding against
np.longdouble at the flagship shape, and the posterior's elementary properties.  tests/test_gpu_alt.py holds the kernel to this
reference."""
import numpy as np
import pytest

import _align_ref as aref
import _alt_ref as alt_ref
import _score_ref as ref


def _share(got, want, T):
    return abs(float(got) - float(want)) / alt_ref.bound(T, want)


def _cases():
    """(probs, tokens): T <= 17, 3 .. 5 labels, tokens drawn from 2 or 3 labels so that repeats abound, up to T // 2 of them;
    single tokens; transcripts that need exactly the frames there are."""
    rng = np.random.default_rng(5)
    out = []
    for T in (1, 2, 3, 4, 5, 6, 7, 9, 12, 16, 17):
        for C in (3, 4, 5):
            for rep in range(14):
                p = ref.peaky(rng, T, C) if rep % 2 else rng.dirichlet(np.ones(C) * 0.5, size=T).astype(np.float32)
                L = int(rng.integers(0, T // 2 + 1)) if rep % 3 else T // 2
                y = [int(v) for v in rng.integers(1, min(C, 3 + rep % 2), size=L)]
                while aref.min_frames(y) > T:
                    y = y[:-1]
                out.append((p, y))
            out.append((ref.peaky(rng, T, C), [int(rng.integers(1, C))]))                      # L = 1
            y = []                                                                              # T = min_frames exactly
            while aref.min_frames(y) < T:
                c = int(rng.integers(1, 3))
                y.append(c if aref.min_frames(y + [c]) <= T else 3 - c)                         # (the other label costs one frame)
            assert aref.min_frames(y) == T
            out.append((rng.dirichlet(np.ones(C), size=T).astype(np.float32), y))
    return out


def test_factorisation_equals_the_forward_recurrence_of_every_variant():
    n = n_neighbour = n_join = n_inf = 0
    worst = 0.0
    for p, y in _cases():
        T, C = p.shape
        logp, alt = alt_ref.alternatives(p, y)
        assert alt.shape == (len(y), C)
        assert _share(logp, ref.forward(p, y), T) <= 1.0 / 3                 # (the forward pass alone: dsmi_score's bound)
        for k in range(len(y)):
            for c in range(C):
                want = ref.forward(p, alt_ref.variant(y, k, c))
                if want is None:
                    assert alt[k, c] == -np.inf, (T, y, k, c, alt[k, c])
                    n_inf += 1
                    continue
                share = _share(alt[k, c], want, T)
                assert share <= 1.0, (T, y, k, c, float(alt[k, c]), float(want))
                worst = max(worst, share)
                n += 1
                n_neighbour += c != 0 and ((k > 0 and y[k - 1] == c) or (k + 1 < len(y) and y[k + 1] == c))
                n_join += c == 0 and 0 < k < len(y) - 1 and y[k - 1] == y[k + 1]
    print("%d variants, %d beside an equal neighbour, %d deletions that join equal neighbours, %d infeasible; worst %.4f of the bound"
          % (n, n_neighbour, n_join, n_inf, worst))
    assert n >= 5000 and n_neighbour >= 100 and n_join >= 50 and n_inf >= 1


def test_float64_rounding_is_a_quarter_of_the_bound_at_the_flagship_shape():
    """501 frames, 150 tokens, 33 labels: float64 against np.longdouble (64 bits of mantissa on x86)."""
    if np.finfo(np.longdouble).nmant <= 52:
        pytest.skip("np.longdouble is float64 here")
    rng = np.random.default_rng(6)
    T, L, C = 501, 150, 33
    p = ref.peaky(rng, T, C, 3.0)
    y = [int(v) for v in rng.integers(1, C, size=L)]
    lp64, a64 = alt_ref.alternatives(p, y)
    lpx, ax = alt_ref.alternatives(p, y, dtype=np.longdouble)
    assert a64.dtype == np.float64 and ax.dtype == np.longdouble
    assert np.isfinite(ax).all() and np.isfinite(a64).all()
    err = np.abs(a64.astype(np.longdouble) - ax).astype(np.float64)
    lim = 24.0 * T * 2.0 ** -52 * np.maximum(1.0, np.abs(ax.astype(np.float64)))
    share = float((err / lim).max())
    print("501 x 150 x 33: float64 is within %.4f of the bound of np.longdouble" % share)
    assert share <= 0.25 and _share(lp64, lpx, T) <= 0.25


def test_posterior_rows_sum_to_one_and_the_own_label_is_the_transcript():
    rng = np.random.default_rng(7)
    for T, C, L in [(9, 4, 3), (33, 33, 11), (64, 33, 20), (40, 6, 20)]:
        p = ref.peaky(rng, T, C)
        y = [int(v) for v in rng.integers(1, C, size=L)]
        if aref.min_frames(y) > T:
            y = list(range(1, C)) * 4
            y = y[:L]
        logp, alt = alt_ref.alternatives(p, y)
        post = alt_ref.posterior(alt)
        np.testing.assert_allclose(post.sum(axis=1), 1.0, rtol=0, atol=1e-12)
        assert ((post >= 0) & (post <= 1)).all()
        for k, c in enumerate(y):
            assert _share(alt[k, c], logp, T) <= 1.0, (T, k, float(alt[k, c]), float(logp))
    assert alt_ref.alternatives(np.zeros((3, 4), dtype=np.float32), [1, 1, 1]) is None
    logp, alt = alt_ref.alternatives(ref.peaky(rng, 5, 4), [])
    assert alt.shape == (0, 4) and np.isfinite(logp)
    logp, alt = alt_ref.alternatives(np.zeros((0, 4), dtype=np.float32), [])
    assert logp == 0.0 and alt.shape == (0, 4)
