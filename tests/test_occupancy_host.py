"""The numpy reference of CTC occupancy (tests/_occ_ref.py) on the CPU: against a brute force over every frame labelling,
float64's own rounding against np.longdouble at the flagship shape and the chunk edges, against torch's CTC loss and its gradient
in float64, against autograd through a plain log-sum-exp forward recurrence that does not lean on torch's CTC backward, and its
invariants.  tests/test_gpu_occupancy.py holds the kernels to this reference."""
import numpy as np
import pytest

import _align_ref as aref
import _occ_ref as occ_ref
import _score_ref as ref

torch = pytest.importorskip("torch")


def _targets(rng, L, C):
    return [int(x) for x in rng.integers(1, C, size=L)]


@pytest.mark.parametrize("C", [3, 4])
def test_reference_equals_the_brute_force(C):
    """T in {1, 2, 5, 6}: every feasible transcript.  1e-12: the brute force adds at most 4^6 products of 6 factors."""
    rng = np.random.default_rng(210 + C)
    n = 0
    for T in (1, 2, 5, 6):
        p = rng.dirichlet(np.ones(C) * 0.5, size=T).astype(np.float32)
        for key, (total, occ, tok) in occ_ref.brute_force(p).items():
            logp, got_occ, got_tok = occ_ref.occupancy(p, list(key))
            assert abs(float(logp) - float(np.log(total))) <= 1e-12
            assert got_occ.shape == (T, C) and got_tok.shape == (T, len(key))
            assert np.abs(got_occ - occ).max() <= 1e-12, (T, key)
            assert tok.size == 0 or np.abs(got_tok - tok).max() <= 1e-12, (T, key)
            n += 1
        assert occ_ref.occupancy(p, [1, 2] * T) is None
    assert n >= 70                    # (3 labels: 74 transcripts fit, 4 labels: more)


def _longdouble_share(p, y):
    T = len(p)
    lp64, o64, k64 = occ_ref.occupancy(p, y)
    lpx, ox, kx = occ_ref.occupancy(p, y, dtype=np.longdouble)
    assert o64.dtype == np.float64 and ox.dtype == np.longdouble
    lim = occ_ref.bound(T, float(lpx))
    worst = float(np.abs(o64.astype(np.longdouble) - ox).max()) / lim
    if k64.size:
        worst = max(worst, float(np.abs(k64.astype(np.longdouble) - kx).max()) / lim)
    assert abs(float(lp64) - float(lpx)) <= ref.bound(T, float(lpx))
    return worst


def test_float64_rounding_against_longdouble():
    """501 x 150 x 33 with sharp and with flat rows, and the chunk-edge shapes: float64 against np.longdouble."""
    if np.finfo(np.longdouble).nmant <= 52:
        pytest.skip("np.longdouble is float64 here")
    rng = np.random.default_rng(206)
    worst = 0.0
    for T, L, sharp in [(501, 150, 3.0), (501, 150, 0.3), (33, 1, 4.0), (64, 30, 4.0)] + [(T, T // 3, 4.0) for T in (15, 16, 17, 31, 32)]:
        share = _longdouble_share(ref.peaky(rng, T, 33, sharp), _targets(rng, L, 33))
        print("T %3d L %3d sharp %.1f: float64 is within %.5f of the bound of np.longdouble" % (T, L, sharp, share))
        worst = max(worst, share)
    print("worst share of the bound: %.5f" % worst)
    assert worst <= 1.0


def _torch_forward(lp, y, blank=0):
    """-logp by a plain log-sum-exp forward recurrence in torch (float64, differentiable with respect to lp [T, C])."""
    lab = [blank if s % 2 == 0 else int(y[s // 2]) for s in range(2 * len(y) + 1)]
    S, ninf = len(lab), torch.tensor(-np.inf, dtype=lp.dtype)
    alpha = [lp[0, lab[s]] if s < 2 else ninf for s in range(S)]
    for t in range(1, lp.shape[0]):
        new = []
        for s in range(S):
            terms = [alpha[s]] + ([alpha[s - 1]] if s >= 1 else []) + ([alpha[s - 2]] if s >= 3 and s % 2 and lab[s] != lab[s - 2] else [])
            terms = [x for x in terms if x > -np.inf]
            new.append(torch.logsumexp(torch.stack(terms), 0) + lp[t, lab[s]] if terms else ninf)
        alpha = new
    return -torch.logsumexp(torch.stack([x for x in alpha[max(S - 2, 0):] if x > -np.inf]), 0)


def test_reference_equals_torch_ctc_loss_and_its_gradient():
    """With lp = log(P.double()) fed to torch's ctc_loss (CPU, float64, reduction='none'): the loss is -logp and occ is
    P - lp.grad (torch returns the gradient as if lp were followed by a softmax: exp(lp) - occ); and occ is -d loss / d lp of
    the plain recurrence, which autograd differentiates without torch's CTC backward."""
    rng = np.random.default_rng(207)
    cases = [(40, 33, [3, 3, 7, 1, 1, 1, 9, 2, 2]), (17, 5, [1, 2, 2, 3]), (12, 4, [])]
    cases.append((33, 33, _targets(rng, 11, 33)))
    for T, C, y in cases:
        p = ref.peaky(rng, T, C)
        logp, occ, tok = occ_ref.occupancy(p, y)
        P = torch.from_numpy(p).double()
        lp = torch.log(P).requires_grad_(True)
        loss = torch.nn.functional.ctc_loss(lp[:, None, :], torch.tensor([y], dtype=torch.long).reshape(1, -1), torch.tensor([T]),
                                            torch.tensor([len(y)]), blank=0, reduction="none", zero_infinity=False)
        loss.sum().backward()
        assert abs(float(loss[0].detach()) + float(logp)) <= 1e-11 * max(1.0, abs(float(logp)))
        assert np.abs(occ - (P - lp.grad).numpy()).max() <= 1e-12, (T, C, y)
        lp2 = torch.log(P).requires_grad_(True)
        plain = _torch_forward(lp2, y)
        plain.backward()
        assert abs(float(plain.detach()) + float(logp)) <= 1e-11 * max(1.0, abs(float(logp)))
        assert np.abs(occ + lp2.grad.numpy()).max() <= 1e-12, (T, C, y)


def test_invariants_of_the_reference():
    rng = np.random.default_rng(208)
    for T, C, L in [(9, 4, 3), (33, 33, 11), (64, 33, 20), (40, 6, 20), (100, 33, 40), (20, 5, 0)]:
        y = [5] * 40 if L == 40 else _targets(rng, L, C)
        if aref.min_frames(y) > T:
            y = (list(range(1, C)) * 8)[:L]
        logp, occ, tok = occ_ref.occupancy(ref.peaky(rng, T, C), y)
        tol = C * occ_ref.bound(T, logp)
        assert (occ >= 0).all() and (tok >= 0).all()
        assert np.abs(occ.sum(axis=1) - 1.0).max() <= tol                        # a path is in one state at every frame
        assert L == 0 or (tok.sum(axis=0) >= 1.0 - T * occ_ref.bound(T, logp)).all()       # every token lasts a frame at least
        for c in range(1, C):                                                  # a label's column collects its tokens
            cols = [k for k, v in enumerate(y) if v == c]
            assert np.abs(occ[:, c] - (tok[:, cols].sum(axis=1) if cols else 0.0)).max() <= tol
    assert occ_ref.occupancy(np.zeros((3, 4), dtype=np.float32), [1, 1, 1]) is None
    logp, occ, tok = occ_ref.occupancy(np.zeros((0, 4), dtype=np.float32), [])
    assert logp == 0.0 and occ.shape == (0, 4) and tok.shape == (0, 0)
