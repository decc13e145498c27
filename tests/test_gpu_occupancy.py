"""CTC occupancy on the GPU (dsmi_occupancy, csrc/occ.hip): occ and tok of every small transcript against a brute force over every
frame labelling, against the float64 numpy forward-backward of tests/_occ_ref.py (held to the contract's bound
32 T 2^-52 max(1, |logp| + 88)), the invariants of the GPU's own output, batch invariance on a ragged batch, the cross-check
with dsmi_score, the refusals, the CTC loss built on it against torch's on the CPU in float64, and the recogniser surface end to
end on the synthetic cfgA-shaped model of tests/test_gpu_score.py.  Every output buffer is filled with NaN before a call, so an
element the library leaves unwritten shows."""
import numpy as np
import pytest

from danspeech_amd import synthetic as syn

import _align_ref as aref
import _ctc_edge_cases as edge
import _occ_ref as occ_ref
import _score_ref as ref
from test_gpu_score import FORWARD_NOISE, _padded, _targets, cfga      # noqa: F401  (cfga: the module-scoped model fixture)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
LABELS = syn.DANSPEECH_LABELS
C33 = len(LABELS)


@pytest.fixture(scope="module")
def native():
    from danspeech_amd import _native
    if not hasattr(_native.NativeDecoder, "occupancy"):
        pytest.fail("dsmi_occupancy is missing")
    return _native


def _occupancy(native, dec, p_dev, sizes, clip, targets, want_occ=True, want_tok=True):
    """dsmi_occupancy itself, into NaN-filled device arrays and sentinel-filled host arrays: (logp, occ, tok, status) as numpy
    (occ / tok None where not asked for)."""
    B, T, C = p_dev.shape
    clip = np.ascontiguousarray(clip, dtype=np.int32).reshape(-1)
    N = len(clip)
    tg, lens = native._padded_ids(targets, None, N, 0, "%d target sequences for %d candidates")
    Ls = tg.shape[1]
    lp = np.full(N, 7.5, dtype=np.float64)
    st = np.full(N, 7, dtype=np.int32)
    occ = torch.full((N, T, C), float("nan"), dtype=torch.float64, device="cuda") if want_occ else None
    tok = torch.full((N, T, Ls), float("nan"), dtype=torch.float64, device="cuda") if want_tok else None
    rc = native.lib().dsmi_occupancy(dec._h, p_dev.data_ptr(), native._sizes_ptr(sizes), B, T, native._np_ptr(clip), native._np_ptr(tg),
                                     native._np_ptr(lens), N, Ls, native._np_ptr(lp), occ.data_ptr() if want_occ else None,
                                     tok.data_ptr() if want_tok and Ls else None, native._np_ptr(st), None)
    assert rc == 0, native.lib().dsmi_decoder_last_error(dec._h).decode()
    return lp, occ.cpu().numpy() if want_occ else None, tok.cpu().numpy() if want_tok else None, st


def _held(lp, occ, tok, status, p, t, want=None, what=""):
    """One candidate's results (occ [T_out, C], tok [T_out, L_stride]) against the reference and the contract: logp within
    dsmi_score's bound, every element within the occupancy bound, exact zeros where the contract says zero, and the
    invariants of the GPU's own output.  Returns the largest share of the occupancy bound."""
    T, C, L = len(p), p.shape[1], len(t)
    want = occ_ref.occupancy(p, t) if want is None else want
    assert status == 0 and not np.isnan(occ).any() and not np.isnan(tok).any(), what
    want_lp, want_occ, want_tok = want
    assert abs(float(lp) - float(want_lp)) <= ref.bound(T, want_lp), (what, float(lp), float(want_lp))
    lim = occ_ref.bound(T, want_lp)
    share = float(np.abs(occ[:T] - want_occ).max()) / lim if T else 0.0
    if L and T:
        share = max(share, float(np.abs(tok[:T, :L] - want_tok).max()) / lim)
    assert share <= 1.0, (what, share)
    assert (occ[T:] == 0.0).all() and (tok[T:] == 0.0).all() and (tok[:, L:] == 0.0).all(), what
    # the GPU's own output
    assert (occ >= 0.0).all() and (occ <= 1.0 + lim).all() and (tok >= 0.0).all() and (tok <= 1.0 + lim).all(), what
    if T:
        assert np.abs(occ[:T].sum(axis=1) - 1.0).max() <= C * lim, what
        assert L == 0 or (tok[:T, :L].sum(axis=0) >= 1.0 - T * lim).all(), what
        absent = [c for c in range(1, C) if c not in t]
        assert (occ[:T][:, absent] == 0.0).all(), what                       # a label the transcript lacks
    return share


# ---- every alignment, enumerated
@pytest.mark.parametrize("C", [3, 4])
def test_brute_force_small_cases(native, C):
    """T in {1, 2, 5, 6}: every feasible transcript against the shares of every frame labelling that collapses to it, and one
    infeasible.  1e-12: the brute force adds at most 4^6 products of 6 factors in float64 (a relative 4.5e-13 at the very worst)."""
    dec = native.NativeDecoder(["_", "a", "b", "c"][:C], blank_index=0)
    rng = np.random.default_rng(310 + C)
    n = 0
    for T in (1, 2, 5, 6):
        p = rng.dirichlet(np.ones(C) * 0.5, size=T).astype(np.float32)
        sums = occ_ref.brute_force(p)
        seqs = [list(k) for k in sums] + [[1, 2] * T]
        p_dev, sizes = _padded([p])
        lp, occ, tok, status = _occupancy(native, dec, p_dev, sizes, [0] * len(seqs), seqs)
        assert occ.shape == (len(seqs), T, C) and tok.shape == (len(seqs), T, 2 * T)
        assert status.tolist() == [0] * len(sums) + [1] and lp[-1] == -np.inf and (occ[-1] == 0.0).all() and (tok[-1] == 0.0).all()
        for i, seq in enumerate(seqs[:-1]):
            total, want_occ, want_tok = sums[tuple(seq)]
            assert abs(float(lp[i]) - float(np.log(total))) <= 1e-12
            assert np.abs(occ[i] - want_occ).max() <= 1e-12, (T, seq)
            assert len(seq) == 0 or np.abs(tok[i, :, :len(seq)] - want_tok).max() <= 1e-12, (T, seq)
            assert (tok[i, :, len(seq):] == 0.0).all()
            n += 1
    print("%d labels: %d transcripts" % (C, n))
    assert n >= 70
    dec.close()


# ---- the shared feeder's edges, forwards and downwards
@pytest.mark.parametrize("shape", edge.SHAPES + edge.LONG, ids=edge.name)
def test_feeder_edges(native, shape):
    """The feeder's chunk boundaries, image wrap and widths (tests/_ctc_edge_cases.py), which the backward pass meets from the
    other end: every row of both clips within the bound.  No case is left out."""
    T, C, L = shape
    probs, rows = edge.case(T, C, L)
    clip = [b for b, rs in enumerate(rows) for _ in rs]
    targets = [r for rs in rows for r in rs]
    dec = native.NativeDecoder(edge.labels(C), blank_index=0)
    p_dev, sizes = _padded(probs)
    assert p_dev.shape[1] == T and sizes[1] < T
    lp, occ, tok, status = _occupancy(native, dec, p_dev, sizes, clip, targets)
    for n, (b, t) in enumerate(zip(clip, targets)):
        _held(lp[n], occ[n], tok[n], status[n], probs[b], t, what=(n, b))
    dec.close()


# ---- the reference, computed once for the module
def _parity_cases():
    rng = np.random.default_rng(321)
    cases = []
    for T in (15, 16, 17, 31, 32, 33, 64):                       # the chunk edges
        for L in (0, 1, T // 3):
            cases.append(("T%d L%d" % (T, L), ref.peaky(rng, T, C33), _targets(rng, L)))
    for L in (127, 128, 129):                                    # S = 255, 257, 259: across the 256 threads
        cases.append(("T260 L%d" % L, ref.peaky(rng, 260, C33), _targets(rng, L)))
    cases.append(("aa runs", ref.peaky(rng, 64, C33), [1, 1, 2, 2, 2, 3, 1, 1, 7, 7, 7, 7, 2, 3, 3, 1, 9, 9, 1, 1]))
    t = [1 + k % 5 for k in range(33)]                           # exactly feasible: one token per frame, a single path
    cases.append(("single path", ref.peaky(rng, 33, C33), t))
    cases.append(("single path of a run", ref.peaky(rng, 17, C33), [4] * 9))
    cases.append(("one label owns 40 states", ref.peaky(rng, 100, C33), [5] * 40))
    cases.append(("128 labels", ref.peaky(rng, 40, 128), _targets(rng, 13, 128)))
    p, t = ref.peaky(rng, 32, C33), _targets(rng, 8)
    p[:, t[2]] = 0.0                                             # p = 0 on a needed label: the FLT_MIN clip
    cases.append(("p = 0 on a needed label", p, t))
    cases.append(("501 x 150", ref.peaky(rng, 501, C33, 3.0), _targets(rng, 150)))
    return cases


@pytest.fixture(scope="module")
def parity():
    cases = _parity_cases()
    return cases, [occ_ref.occupancy(p, t) for _, p, t in cases]


def _run_cases(native, cases):
    """One call per label count: (logp, occ [T_out, C], tok [T_out, L_stride], status) in the cases' order."""
    out = [None] * len(cases)
    for C in sorted(set(p.shape[1] for _, p, _ in cases)):
        idx = [i for i, (_, p, _) in enumerate(cases) if p.shape[1] == C]
        dec = native.NativeDecoder(LABELS if C == C33 else edge.labels(C), blank_index=0)
        p_dev, sizes = _padded([cases[i][1] for i in idx])
        lp, occ, tok, status = _occupancy(native, dec, p_dev, sizes, np.arange(len(idx)), [cases[i][2] for i in idx])
        for j, i in enumerate(idx):
            out[i] = (lp[j], occ[j], tok[j], status[j])
        dec.close()
    return out


def test_reference_parity_and_invariants_within_the_bound(native, parity):
    cases, want = parity
    got = _run_cases(native, cases)
    worst = 0.0
    for (name, p, t), w, (lp, occ, tok, status) in zip(cases, want, got):
        share = _held(lp, occ, tok, status, p, t, want=w, what=name)
        print("%-26s logp %.9f  %.4f of the bound" % (name, lp, share))
        worst = max(worst, share)
    print("worst share of the bound: %.4f" % worst)
    names = [n for n, _, _ in cases]
    # one path and no frame to spare: every gamma is 0 or 1
    i = names.index("single path")
    lim = occ_ref.bound(33, got[i][0])
    assert np.abs(got[i][2][:33, :33] - np.eye(33)).max() <= lim
    assert np.abs(got[i][1][np.arange(33), cases[i][2]] - 1.0).max() <= lim
    i = names.index("single path of a run")                      # a, blank, a, ..., a: token k at frame 2k, the blank between
    lim = occ_ref.bound(17, got[i][0])
    pattern = np.zeros((17, 9))
    pattern[2 * np.arange(9), np.arange(9)] = 1.0
    assert np.abs(got[i][2][:17, :9] - pattern).max() <= lim
    assert np.abs(got[i][1][:17, 4] - (np.arange(17) % 2 == 0)).max() <= lim and np.abs(got[i][1][:17, 0] - (np.arange(17) % 2 == 1)).max() <= lim
    assert float(want[names.index("p = 0 on a needed label")][0]) < np.log(float(ref.FLT_MIN))


def test_longest_candidate(native):
    """DSMI_OCC_MAX_TOKENS tokens on 2100 frames: the largest LDS carve, 9 states per thread, the blank's 1025 states in one sum."""
    dec = native.NativeDecoder(LABELS, blank_index=0)
    rng = np.random.default_rng(313)
    t = _targets(rng, native.OCC_MAX_TOKENS)
    T = 2100
    assert aref.min_frames(t) <= T
    p = ref.peaky(rng, T, C33, sharp=2.0)
    p_dev, sizes = _padded([p])
    lp, occ, tok, status = _occupancy(native, dec, p_dev, sizes, [0], [t])
    share = _held(lp[0], occ[0], tok[0], status[0], p, t)
    print("1024 tokens on 2100 frames: logp %.6f, %.4f of the bound" % (lp[0], share))
    dec.close()


def test_one_repeated_letter_at_the_longest(native):
    """1024 times the same letter on 2100 frames: 1024 token states under one label, 1025 under the blank."""
    dec = native.NativeDecoder(LABELS, blank_index=0)
    rng = np.random.default_rng(314)
    t = [7] * native.OCC_MAX_TOKENS
    T = 2100
    assert aref.min_frames(t) == 2047
    p = ref.peaky(rng, T, C33, sharp=1.0, blank_boost=0.5)
    p_dev, sizes = _padded([p])
    lp, occ, tok, status = _occupancy(native, dec, p_dev, sizes, [0], [t])
    share = _held(lp[0], occ[0], tok[0], status[0], p, t)
    print("1024 x one letter on 2100 frames: logp %.6f, %.4f of the bound" % (lp[0], share))
    dec.close()


# ---- a ragged batch: NaN past every clip's frames, candidates in scrambled order, each as if it were alone
def test_ragged_batch_is_batch_invariant_and_reads_no_frame_past_a_clip(native):
    dec = native.NativeDecoder(LABELS, blank_index=0)
    rng = np.random.default_rng(331)
    frames = [64, 50, 33, 17, 40]
    probs = [ref.peaky(rng, T, C33) for T in frames]
    p_dev, sizes = _padded(probs, T_out=70, fill=np.nan)
    clip, targets = [], []
    for b, count in enumerate([0, 1, 3, 12, 3]):                  # (clip 0 has no candidate)
        for k in range(count):
            clip.append(b)
            targets.append(_targets(rng, int(rng.integers(0, frames[b] // 2 + 1))))
    targets[2] = []                                               # an empty transcript
    targets[7] = [5] * 12                                         # 12 + 11 frames > 17: infeasible
    perm = rng.permutation(len(clip))
    clip, targets = [clip[i] for i in perm], [targets[i] for i in perm]
    lp, occ, tok, status = _occupancy(native, dec, p_dev, sizes, clip, targets)
    assert occ.shape[1] == 70 and tok.shape[1] == 70
    n_bad = 0
    for n, (b, t) in enumerate(zip(clip, targets)):
        if occ_ref.occupancy(probs[b], t) is None:
            assert status[n] == 1 and lp[n] == -np.inf and (occ[n] == 0.0).all() and (tok[n] == 0.0).all()
            n_bad += 1
            continue
        _held(lp[n], occ[n], tok[n], status[n], probs[b], t, what=(n, b))
        if len(t) == 0:
            assert np.abs(occ[n, :frames[b], 0] - 1.0).max() <= occ_ref.bound(frames[b], lp[n])
    assert n_bad >= 1 and any(len(t) == 0 for t in targets)
    for n, (b, t) in enumerate(zip(clip, targets)):              # alone in the call, among all the clips: the same bits
        lp1, occ1, tok1, _ = _occupancy(native, dec, p_dev, sizes, [b], [t])
        assert lp1[0] == lp[n]
        np.testing.assert_array_equal(occ1[0], occ[n])
        np.testing.assert_array_equal(tok1[0], tok[n, :, :tok1.shape[2]])
    for n in (0, 5, 11):                                         # ... and with only its own clip in the call
        p1, s1 = _padded([probs[clip[n]]])
        lp1, occ1, tok1, _ = _occupancy(native, dec, p1, s1, [0], [targets[n]])
        assert lp1[0] == lp[n]
        np.testing.assert_array_equal(occ1[0], occ[n, :occ1.shape[1]])
        np.testing.assert_array_equal(tok1[0], tok[n, :tok1.shape[1], :tok1.shape[2]])
    # one array alone: the same bits as both together
    lp_o, occ_o, none, _ = _occupancy(native, dec, p_dev, sizes, clip, targets, want_tok=False)
    assert none is None and (lp_o == lp).all()
    np.testing.assert_array_equal(occ_o, occ)
    lp_t, none, tok_t, _ = _occupancy(native, dec, p_dev, sizes, clip, targets, want_occ=False)
    assert none is None and (lp_t == lp).all()
    np.testing.assert_array_equal(tok_t, tok)
    lp_n, _, _, st_n = _occupancy(native, dec, p_dev, sizes, clip, targets, want_occ=False, want_tok=False)
    assert (lp_n == lp).all() and (st_n == status).all()
    # the binding's own call: the same bits again
    lp_b, occ_b, tok_b, st_b = dec.occupancy(p_dev, sizes, clip, targets)
    assert (lp_b == lp).all() and (st_b == status).all() and occ_b.is_cuda and occ_b.dtype == torch.float64
    np.testing.assert_array_equal(occ_b.cpu().numpy(), occ)
    np.testing.assert_array_equal(tok_b.cpu().numpy(), tok)
    # no sizes: every clip has T_out frames
    p_full, _ = _padded(probs[:1] * 2)
    lp2, occ2, tok2, st2 = _occupancy(native, dec, p_full, None, [1, 0], [[3, 4], [3, 4]])
    assert lp2[0] == lp2[1] and (occ2[0] == occ2[1]).all() and (tok2[0] == tok2[1]).all()
    _held(lp2[0], occ2[0], tok2[0], st2[0], probs[0], [3, 4])
    # no frames: the empty transcript alone is feasible, with probability 1 and nothing occupied
    lp0, occ0, tok0, st0 = _occupancy(native, dec, p_dev, np.array([0, 5, 5, 5, 5], dtype=np.int32), [0, 0], [[], [3]])
    assert lp0.tolist() == [0.0, -np.inf] and st0.tolist() == [0, 1] and (occ0 == 0.0).all() and (tok0 == 0.0).all()
    dec.close()


# ---- against the kernel that is there already
def test_logp_agrees_with_dsmi_score(native, parity):
    """The same candidates through dsmi_score: either is within dsmi_score's bound of the exact recurrence."""
    cases = [c for c in parity[0] if c[1].shape[1] == C33]
    dec = native.NativeDecoder(LABELS, blank_index=0)
    p_dev, sizes = _padded([p for _, p, _ in cases])
    targets = [t for _, _, t in cases]
    lp_s, st_s = dec.score(p_dev, sizes, np.arange(len(cases)), targets)
    lp_o, _, _, st_o = _occupancy(native, dec, p_dev, sizes, np.arange(len(cases)), targets, want_occ=False, want_tok=False)
    assert not st_s.any() and not st_o.any()
    for (name, p, _), s, o in zip(cases, lp_s, lp_o):
        assert abs(float(s) - float(o)) <= 2 * ref.bound(len(p), s), (name, float(s), float(o))
    dec.close()


# ---- refusals
def test_refusals_write_nothing(native):
    dec = native.NativeDecoder(LABELS, blank_index=0)
    L = native.lib()
    B, T, N, Ls = 2, 10, 3, 3
    probs = torch.full((B, T, C33), 1.0 / C33, device="cuda")
    ok = dict(B=B, T=T, N=N, Ls=Ls, sizes=[10, 8], clip=[1, 0, 1], tg=[[1, 2, 3], [4, 5, 0], [0, 0, 0]], lens=[3, 2, 0], probs=probs)
    occ = torch.full((4, T, C33), 7.5, dtype=torch.float64, device="cuda")
    tok = torch.full((4, T, 3), 7.5, dtype=torch.float64, device="cuda")

    def call(out=("logp", "status"), null=(), **kw):
        a = dict(ok, **kw)
        lp = np.full(4, 7.5, dtype=np.float64)
        st = np.full(4, 7, dtype=np.int32)
        occ.fill_(7.5)
        tok.fill_(7.5)
        arr = {k: np.ascontiguousarray(a[k], dtype=np.int32) for k in ("sizes", "clip", "tg", "lens")}
        rc = L.dsmi_occupancy(dec._h, None if "probs" in null else a["probs"].data_ptr(), native._np_ptr(arr["sizes"]), a["B"], a["T"],
                              None if "clip" in null else native._np_ptr(arr["clip"]), None if "tg" in null else native._np_ptr(arr["tg"]),
                              None if "lens" in null else native._np_ptr(arr["lens"]), a["N"], a["Ls"],
                              native._np_ptr(lp) if "logp" in out else None, occ.data_ptr(), tok.data_ptr(),
                              native._np_ptr(st) if "status" in out else None, None)
        torch.cuda.synchronize()
        untouched = (lp == 7.5).all() and (st == 7).all() and bool((occ == 7.5).all()) and bool((tok == 7.5).all())
        return rc, untouched, L.dsmi_decoder_last_error(dec._h).decode(), lp, st

    rc, untouched, _, lp, st = call()
    assert rc == 0 and not untouched and st[:3].tolist() == [0, 0, 0] and np.isfinite(lp[:3]).all() and lp[3] == 7.5 and st[3] == 7
    assert bool((occ[3] == 7.5).all()) and bool((tok[3] == 7.5).all()) and not bool((occ[:3] == 7.5).any()) and not bool((tok[:3] == 7.5).any())
    invalid = (dict(B=0), dict(T=0), dict(T=-3), dict(N=0), dict(N=-1), dict(Ls=-1), dict(sizes=[11, 8]), dict(sizes=[-1, 8]),
               dict(clip=[2, 0, 1]), dict(clip=[1, -1, 1]), dict(lens=[-1, 2, 0]), dict(lens=[4, 2, 0]),
               dict(tg=[[1, 0, 3], [4, 5, 0], [0, 0, 0]]), dict(tg=[[1, 2, 3], [4, C33, 0], [0, 0, 0]]),
               dict(tg=[[1, 2, -2], [4, 5, 0], [0, 0, 0]]), dict(out=("status",)), dict(out=("logp",)),
               dict(null=("probs",)), dict(null=("clip",)), dict(null=("lens",)), dict(null=("tg",)))
    for kw in invalid:
        rc, untouched, msg, *_ = call(**kw)
        assert rc == native.DSMI_ERR_INVALID and untouched and msg, (kw, rc, msg)
    rc, *_ = call(null=("tg",), Ls=0, lens=[0, 0, 0])                     # no tokens: no token array is needed
    assert rc == 0
    big = np.zeros((3, native.OCC_MAX_TOKENS + 1), dtype=np.int32)
    rc, untouched, msg, *_ = call(tg=big, Ls=native.OCC_MAX_TOKENS + 1)
    assert rc == native.DSMI_ERR_CAPACITY and untouched and "DSMI_OCC_MAX_TOKENS" in msg
    # N * L_stride > 2^24: refused on the numbers alone, before any array is read past what is there
    many = (1 << 24) // 1024 + 1
    rc, untouched, msg, *_ = call(N=many, Ls=1024, clip=np.zeros(1), lens=np.zeros(1), tg=np.zeros((1, 1024)))
    assert rc == native.DSMI_ERR_CAPACITY and untouched and "2^24" in msg
    # the stored trellis: 4 candidates of 1024 tokens on 4096 frames, 4 x 4096 x 2049 > 2^25 elements
    long_probs = torch.full((1, 4096, C33), 1.0 / C33, device="cuda")
    tg = np.tile(np.array([1, 2], dtype=np.int32), (4, 512))
    rc, untouched, msg, *_ = call(probs=long_probs, B=1, T=4096, N=4, Ls=1024, sizes=[4096], clip=np.zeros(4), lens=np.full(4, 1024), tg=tg)
    assert rc == native.DSMI_ERR_CAPACITY and untouched and "2^25" in msg
    rc, *_ = call()
    assert rc == 0
    dec.close()


# ---- the CTC loss on it, against torch's on the CPU in float64
def _torch_reference(P, sizes, ids):
    """Per clip, on its own frames: (-logp, occ [frames, C]) from torch.nn.functional.ctc_loss on the CPU in float64, fed
    lp = log(max(P, FLT_MIN)) of the float32 P the library saw: occ = P - lp.grad (tests/test_occupancy_host.py)."""
    out = []
    for b, y in enumerate(ids):
        Pb = P[b, :sizes[b]].double()
        lp = torch.log(Pb.clamp_min(float(ref.FLT_MIN))).requires_grad_(True)
        loss = torch.nn.functional.ctc_loss(lp[:, None, :], torch.tensor(y, dtype=torch.long).reshape(1, -1), torch.tensor([int(sizes[b])]),
                                            torch.tensor([len(y)]), blank=0, reduction="none")
        loss.sum().backward()
        out.append((float(loss[0].detach()), (torch.exp(lp.detach()) - lp.grad).numpy()))
    return out


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("T", [17, 33, 40])
def test_ctc_loss_and_gradient_against_torch_on_the_cpu(native, T, dtype):
    """B = 3, one clip shorter than T_out, the clips weighted 1, 0.5 and 2 so that grad_out is not all ones.  The tolerance is
    the occupancy bound (times the weight), plus 2^-24 |value| where the gradient comes back in float32."""
    from danspeech_amd.deepspeech.decoder import GreedyDecoder
    from danspeech_amd.deepspeech.loss import ctc_loss
    dt = getattr(torch, dtype)
    rng = np.random.default_rng(340 + T)
    sizes = np.array([T, T - 5, T], dtype=np.int32)
    ids = [_targets(rng, T // 3), [3, 3, 7, 1, 1], _targets(rng, 1)]
    logits = torch.from_numpy(rng.normal(size=(3, T, C33)) * 3.0).to(dt).cuda().requires_grad_(True)
    weights = torch.tensor([1.0, 0.5, 2.0], dtype=torch.float64, device="cuda")
    decoder = GreedyDecoder(LABELS, blank_index=0)
    loss = ctc_loss(logits, sizes, ids, decoder)
    assert loss.dtype == torch.float64 and loss.is_cuda and loss.shape == (3,)
    (loss * weights).sum().backward()
    assert logits.grad.dtype == dt
    P = torch.softmax(logits.detach(), -1).float().cpu()                  # the float32 probabilities the library saw
    grad = logits.grad.cpu().double().numpy()
    got = loss.detach().cpu().numpy()
    for b, (want_loss, want_occ) in enumerate(_torch_reference(P, sizes, ids)):
        n, w = int(sizes[b]), float(weights[b])
        lim = occ_ref.bound(n, want_loss)
        assert abs(float(got[b]) - want_loss) <= lim, (b, float(got[b]), want_loss)
        want = w * (P[b, :n].double().numpy() - want_occ)
        tol = w * lim + (2.0 ** -24 * np.abs(want) if dtype == "float32" else 0.0)
        err = np.abs(grad[b, :n] - want)
        print("T %d %s clip %d: loss %.9f, gradient within %.4f of its tolerance" % (T, dtype, b, float(got[b]), float((err / tol).max())))
        assert (err <= tol).all(), (b, float((err / tol).max()))
        assert (grad[b, n:] == 0.0).all()                                 # nothing past the clip's frames


def test_ctc_loss_of_an_infeasible_transcript_is_inf_with_zero_gradient(native):
    from danspeech_amd.deepspeech.decoder import GreedyDecoder
    from danspeech_amd.deepspeech.loss import ctc_loss
    rng = np.random.default_rng(341)
    logits = torch.from_numpy(rng.normal(size=(3, 17, C33))).float().cuda().requires_grad_(True)
    ids = [[1, 2, 3], [5] * 12, []]                                       # 12 + 11 frames > 17
    loss = ctc_loss(logits, None, ids, GreedyDecoder(LABELS, blank_index=0))
    assert torch.isfinite(loss[0]) and torch.isinf(loss[1]) and loss[1] > 0 and torch.isfinite(loss[2])
    loss[torch.isfinite(loss)].sum().backward()
    g = logits.grad.cpu().numpy()
    assert np.isfinite(g).all() and (g[1] == 0.0).all() and np.abs(g[0]).max() > 0 and np.abs(g[2]).max() > 0
    logits.grad = None
    ctc_loss(logits, None, ids, GreedyDecoder(LABELS, blank_index=0)).sum().backward()         # (inf in the sum: still no NaN)
    g = logits.grad.cpu().numpy()
    assert np.isfinite(g).all() and (g[1] == 0.0).all()
    with pytest.raises(ValueError):
        ctc_loss(logits, None, ids[:2], GreedyDecoder(LABELS, blank_index=0))


# ---- end to end: the synthetic cfgA-shaped model of test_gpu_score.py
def test_soft_align_batch_equals_occupancy_ids_in_callers_order(cfga):
    """Two forwards of the same batch feed the two sides (FORWARD_NOISE, tests/test_gpu_score.py): every gamma's exponent moves
    by at most 2 x frames x 2^-24 < FORWARD_NOISE, so a dwell moves by that share of itself, a centre -- a ratio of two such
    sums over frames 0 .. frames -- by at most 2 FORWARD_NOISE x frames, and a spread, to first order, by its own share plus
    the centre's move."""
    rec, clips = cfga
    eng = rec.danspeech_recognizer
    if not hasattr(eng, "soft_align_batch"):
        pytest.fail("dsmi_occupancy is missing")
    texts = rec.recognize_batch(clips)
    asked = [texts[0], "hej med dig", texts[2], "  Hej  DER", "ab" * 400]         # (the last: far more letters than frames)
    batch = rec.soft_align_batch(clips, asked)
    job = eng._enqueue_batch(clips)
    job.collect_forward()
    norm = [eng.decoder.normalise_transcript(t) for t in asked]
    ids = [eng.decoder.transcript_ids(t) for t in norm]
    direct = eng.decoder.occupancy_ids(job.probs, [ids[i] for i in job.order], job.sizes)
    assert sorted(job.order) == list(range(len(clips))) and list(job.order) != sorted(job.order)
    frame_s = eng.frame_seconds()
    n_chars = 0
    for pos, i in enumerate(job.order):
        if direct[pos] is None:
            assert batch[i] is None
            continue
        words, chars = batch[i]
        logp, occ, tok = direct[pos]
        frames = int(job.sizes[pos])
        assert np.isfinite(logp) and occ.is_cuda and tuple(occ.shape) == (frames, C33) and tuple(tok.shape) == (frames, len(norm[i]))
        tok = tok.cpu().numpy()
        np.testing.assert_allclose(occ.sum(1).cpu().numpy(), 1.0, rtol=0, atol=C33 * occ_ref.bound(frames, logp))
        assert "".join(ch for ch, *_ in chars) == norm[i] and [w for w, *_ in words] == norm[i].split()
        t = np.arange(frames)[:, None]
        dwell = tok.sum(0)
        centre = (t * tok).sum(0) / dwell
        spread = np.sqrt(((t - centre[None, :]) ** 2 * tok).sum(0) / dwell)
        shift = 2 * FORWARD_NOISE * frames * frame_s
        for k, (ch, centre_s, spread_s, dwell_s) in enumerate(chars):
            assert dwell_s >= frame_s * (1.0 - frames * occ_ref.bound(frames, logp))       # every character lasts one frame at least
            assert 0.0 <= centre_s <= (frames - 1) * frame_s + 1e-12 and spread_s >= 0.0
            assert dwell_s == pytest.approx(dwell[k] * frame_s, rel=FORWARD_NOISE)
            assert centre_s == pytest.approx(centre[k] * frame_s, abs=shift)
            assert spread_s == pytest.approx(spread[k] * frame_s, abs=shift + FORWARD_NOISE * spread[k] * frame_s)
            n_chars += 1
        k = 0
        for word, first_s, last_s in words:                       # a word runs from its first character's centre to its last's
            k = norm[i].index(word, k)
            assert first_s == chars[k][1] and last_s == chars[k + len(word) - 1][1]
            k += len(word)
    assert n_chars > 20 and batch[4] is None
    single = rec.soft_align(clips[1], asked[1])
    assert [w for w, *_ in single[0]] == ["hej", "med", "dig"]
    assert "".join(ch for ch, *_ in single[1]) == "hej med dig"
    assert rec.soft_align_batch([], []) == []
    with pytest.raises(ValueError, match="'#'"):
        rec.soft_align_batch(clips[:1], ["nr #1"])
    with pytest.raises(ValueError):
        rec.soft_align_batch(clips, asked[:2])
