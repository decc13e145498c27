"""CTC token confidence on the GPU (dsmi_alternatives, csrc/alt.hip): every variant of every small transcript against a brute
force over every frame labelling, the float64 numpy forward-backward of tests/_alt_ref.py and the plain forward recurrence of
the variants themselves (held to the contract's bound 24 T 2^-52 max(1, |value|)), batch invariance on a ragged batch, the
cross-check with dsmi_score, its refusals, and the recogniser surface end to end on the synthetic cfgA-shaped model of
tests/test_gpu_score.py."""
import numpy as np
import pytest

from danspeech_amd import synthetic as syn

import _align_ref as aref
import _alt_ref as alt_ref
import _ctc_edge_cases as edge
import _score_ref as ref
from test_gpu_score import FORWARD_NOISE, _padded, _targets, cfga      # noqa: F401  (cfga: the module-scoped model fixture)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
LABELS = syn.DANSPEECH_LABELS
C33 = len(LABELS)


@pytest.fixture(scope="module")
def native():
    from danspeech_amd import _native
    if not hasattr(_native.NativeDecoder, "alternatives"):
        pytest.fail("dsmi_alternatives is missing")
    return _native


def _share(got, want, T):
    return abs(float(got) - float(want)) / alt_ref.bound(T, want)


def _worst_share(got, want, T):
    """Every slot of one candidate against the reference's [L, C]: -inf where and only where the reference is, else the
    largest share of the bound."""
    got, want = np.asarray(got), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert not np.isnan(got).any() and ((got == -np.inf) == (want == -np.inf)).all()
    fin = np.isfinite(want)
    if not fin.any():
        return 0.0
    lim = 24.0 * max(T, 1) * 2.0 ** -52 * np.maximum(1.0, np.abs(want[fin]))
    return float((np.abs(got[fin] - want[fin]) / lim).max())


# ---- every alignment of every variant, enumerated
@pytest.mark.parametrize("C", [3, 4])
def test_brute_force_small_cases(native, C):
    """T in {1, 2, 5, 6}: every feasible transcript, every slot, every label against the sum over every frame labelling that
    collapses to the variant; -inf where no labelling does.  1e-12 in the log as in test_gpu_score.py: the brute force adds at
    most 4^6 products of 6 factors in float64 (a relative 4.5e-13 at the very worst)."""
    dec = native.NativeDecoder(["_", "a", "b", "c"][:C], blank_index=0)
    rng = np.random.default_rng(110 + C)
    n = n_inf = 0
    for T in (1, 2, 5, 6):
        p = rng.dirichlet(np.ones(C) * 0.5, size=T).astype(np.float32)
        sums = ref.brute_force(p)
        seqs = [list(k) for k in sums] + [[1, 2] * T]
        p_dev, sizes = _padded([p])
        lp, alt, status = dec.alternatives(p_dev, sizes, [0] * len(seqs), seqs)
        assert alt.shape == (len(seqs), 2 * T, C)
        assert status.tolist() == [0] * len(sums) + [1] and lp[-1] == -np.inf and (alt[-1] == -np.inf).all()
        for i, seq in enumerate(seqs[:-1]):
            assert abs(float(lp[i]) - float(np.log(sums[tuple(seq)]))) <= 1e-12
            assert (alt[i, len(seq):] == -np.inf).all()
            for k in range(len(seq)):
                for c in range(C):
                    v = tuple(alt_ref.variant(seq, k, c))
                    if v not in sums:
                        assert alt[i, k, c] == -np.inf, (T, seq, k, c, float(alt[i, k, c]))
                        n_inf += 1
                        continue
                    want = float(np.log(sums[v]))
                    assert abs(float(alt[i, k, c]) - want) <= 1e-12, (T, seq, k, c, float(alt[i, k, c]), want)
                    n += 1
    print("%d labels: %d variants, %d that fit no labelling" % (C, n, n_inf))
    assert n >= 300 and n_inf >= 1
    dec.close()


# ---- the shared feeder's edges, forwards and downwards
@pytest.mark.parametrize("shape", edge.SHAPES + edge.LONG, ids=edge.name)
def test_feeder_edges(native, shape):
    """The feeder's chunk boundaries, image wrap and widths (tests/_ctc_edge_cases.py), which the backward pass meets from the
    other end: every row of both clips, every slot against the float64 forward-backward reference, and a seeded sample of 64
    (k, c) per row against the plain forward recurrence of the variant itself.  No case is left out."""
    T, C, L = shape
    probs, rows = edge.case(T, C, L)
    clip = [b for b, rs in enumerate(rows) for _ in rs]
    targets = [r for rs in rows for r in rs]
    dec = native.NativeDecoder(edge.labels(C), blank_index=0)
    p_dev, sizes = _padded(probs)
    assert p_dev.shape[1] == T and sizes[1] < T
    lp, alt, status = dec.alternatives(p_dev, sizes, clip, targets)
    assert not status.any()
    rng = np.random.default_rng(7 * T + C)
    for n, (b, t) in enumerate(zip(clip, targets)):
        frames = len(probs[b])
        want_lp, want = alt_ref.alternatives(probs[b], t)
        assert _share(lp[n], want_lp, frames) <= 1.0, (n, b, float(lp[n]), float(want_lp))
        assert _worst_share(alt[n, :len(t)], want, frames) <= 1.0, (n, b)
        assert (alt[n, len(t):] == -np.inf).all()
        slots = [(k, c) for k in range(len(t)) for c in range(C)]
        for j in rng.permutation(len(slots))[:64]:
            k, c = slots[j]
            direct = ref.forward(probs[b], alt_ref.variant(t, k, c))
            if direct is None:
                assert alt[n, k, c] == -np.inf, (n, k, c)
            else:
                assert _share(alt[n, k, c], direct, frames) <= 1.0, (n, k, c, float(alt[n, k, c]), float(direct))
    dec.close()


# ---- the reference, computed once for the module
def _parity_cases():
    rng = np.random.default_rng(121)
    cases = []
    for T in (15, 16, 17, 31, 32, 33, 64):                       # the chunk edges
        for L in (0, 1, T // 3):
            cases.append(("T%d L%d" % (T, L), ref.peaky(rng, T, C33), _targets(rng, L)))
    for L in (127, 128, 129):                                    # S = 255, 257, 259: across the 256 threads
        cases.append(("T260 L%d" % L, ref.peaky(rng, 260, C33), _targets(rng, L)))
    cases.append(("L * C = 256", ref.peaky(rng, 40, 32), _targets(rng, 8, 32)))             # slot workgroups that are exactly full,
    cases.append(("L * C = 512", ref.peaky(rng, 40, 32), _targets(rng, 16, 32)))            # (every other case: a ragged last one)
    cases.append(("aa runs", ref.peaky(rng, 64, C33), [1, 1, 2, 2, 2, 3, 1, 1, 7, 7, 7, 7, 2, 3, 3, 1, 9, 9, 1, 1]))
    t = [1 + k % 5 for k in range(33)]                           # exactly feasible: one token per frame, a single path
    cases.append(("single path", ref.peaky(rng, 33, C33), t))
    cases.append(("single path of a run", ref.peaky(rng, 17, C33), [4] * 9))
    p, t = ref.peaky(rng, 32, C33), _targets(rng, 8)
    p[:, t[2]] = 0.0                                             # p = 0 on a needed label: the FLT_MIN clip
    cases.append(("p = 0 on a needed label", p, t))
    cases.append(("501 x 150", ref.peaky(rng, 501, C33, 3.0), _targets(rng, 150)))
    return cases


@pytest.fixture(scope="module")
def parity():
    cases = _parity_cases()
    return cases, [alt_ref.alternatives(p, t) for _, p, t in cases]


def _run_cases(native, cases):
    """One call per label count: (logp, alt rows cut to each case's length) in the cases' order."""
    out = [None] * len(cases)
    for C in sorted(set(p.shape[1] for _, p, _ in cases)):
        idx = [i for i, (_, p, _) in enumerate(cases) if p.shape[1] == C]
        dec = native.NativeDecoder(LABELS if C == C33 else edge.labels(C), blank_index=0)
        p_dev, sizes = _padded([cases[i][1] for i in idx])
        lp, alt, status = dec.alternatives(p_dev, sizes, np.arange(len(idx)), [cases[i][2] for i in idx])
        assert not status.any()
        for j, i in enumerate(idx):
            L = len(cases[i][2])
            assert (alt[j, L:] == -np.inf).all()
            out[i] = (lp[j], alt[j, :L])
        dec.close()
    return out


def test_reference_parity_within_the_bound(native, parity):
    cases, want = parity
    got = _run_cases(native, cases)
    worst = 0.0
    for (name, p, t), (want_lp, want_alt), (lp, alt) in zip(cases, want, got):
        T = len(p)
        share = max(_share(lp, want_lp, T), _worst_share(alt, want_alt, T))
        print("%-26s logp %.9f  %5d of %5d variants fit  %.4f of the bound" % (name, lp, np.isfinite(alt).sum(), alt.size, share))
        assert share <= 1.0, name
        for k, c in enumerate(t):                                # the own label: the transcript itself
            assert _share(alt[k, c], want_lp, T) <= 1.0, (name, k)
        worst = max(worst, share)
    print("worst share of the bound: %.4f" % worst)
    names = [n for n, _, _ in cases]
    single = got[names.index("single path")][1]
    # one path and no frame to spare: a variant fits no more exactly where it puts two equal tokens side by side
    t = cases[names.index("single path")][2]
    tight = sum(aref.min_frames(alt_ref.variant(t, k, c)) > 33 for k in range(len(t)) for c in range(C33))
    assert np.isinf(single).sum() == tight and tight >= len(t)
    assert got[names.index("L * C = 256")][1].size == 256 and got[names.index("501 x 150")][1].size % 256
    assert float(want[names.index("p = 0 on a needed label")][0]) < np.log(float(ref.FLT_MIN))


def test_longest_candidate(native):
    """DSMI_ALT_MAX_TOKENS tokens on 2100 frames: the largest LDS carve, 9 states per thread, 132 slot workgroups."""
    dec = native.NativeDecoder(LABELS, blank_index=0)
    rng = np.random.default_rng(113)
    t = _targets(rng, native.ALT_MAX_TOKENS)
    T = 2100
    assert aref.min_frames(t) <= T
    p = ref.peaky(rng, T, C33, sharp=2.0)
    want_lp, want = alt_ref.alternatives(p, t)
    p_dev, sizes = _padded([p])
    lp, alt, status = dec.alternatives(p_dev, sizes, [0], [t])
    share = max(_share(lp[0], want_lp, T), _worst_share(alt[0], want, T))
    print("1024 tokens on 2100 frames: logp %.6f, %.4f of the bound" % (lp[0], share))
    assert status[0] == 0 and share <= 1.0
    dec.close()


# ---- a ragged batch: NaN past every clip's frames, candidates in scrambled order, each as if it were alone
def test_ragged_batch_is_batch_invariant_and_reads_no_frame_past_a_clip(native):
    dec = native.NativeDecoder(LABELS, blank_index=0)
    rng = np.random.default_rng(131)
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
    lp, alt, status = dec.alternatives(p_dev, sizes, clip, targets)
    n_bad = 0
    for n, (b, t) in enumerate(zip(clip, targets)):
        want = alt_ref.alternatives(probs[b], t)
        if want is None:
            assert status[n] == 1 and lp[n] == -np.inf and (alt[n] == -np.inf).all()
            n_bad += 1
            continue
        assert status[n] == 0 and _share(lp[n], want[0], frames[b]) <= 1.0, (n, b, float(lp[n]), float(want[0]))
        assert _worst_share(alt[n, :len(t)], want[1], frames[b]) <= 1.0, (n, b)
        assert (alt[n, len(t):] == -np.inf).all()
    assert n_bad >= 1 and any(len(t) == 0 for t in targets)
    for n, (b, t) in enumerate(zip(clip, targets)):              # alone in the call, among all the clips: the same bits
        lp1, alt1, _ = dec.alternatives(p_dev, sizes, [b], [t])
        assert lp1[0] == lp[n]
        np.testing.assert_array_equal(alt1[0], alt[n, :alt1.shape[1]])
    for n in (0, 5, 11):                                         # ... and with only its own clip in the call
        p1, s1 = _padded([probs[clip[n]]])
        lp1, alt1, _ = dec.alternatives(p1, s1, [0], [targets[n]])
        assert lp1[0] == lp[n]
        np.testing.assert_array_equal(alt1[0], alt[n, :alt1.shape[1]])
    # no sizes: every clip has T_out frames
    p_full, _ = _padded(probs[:1] * 2)
    lp2, alt2, _ = dec.alternatives(p_full, None, [1, 0], [[3, 4], [3, 4]])
    assert lp2[0] == lp2[1] and (alt2[0] == alt2[1]).all() and _worst_share(alt2[0], alt_ref.alternatives(probs[0], [3, 4])[1], 64) <= 1.0
    # no frames: the empty transcript alone is feasible, with probability 1
    lp0, alt0, st0 = dec.alternatives(p_dev, np.array([0, 5, 5, 5, 5], dtype=np.int32), [0, 0], [[], [3]])
    assert lp0.tolist() == [0.0, -np.inf] and st0.tolist() == [0, 1] and (alt0 == -np.inf).all()
    dec.close()


# ---- against the kernel that is there already
def test_logp_agrees_with_dsmi_score(native, parity):
    """The same candidates through dsmi_score: either is within its own bound of the exact recurrence, 8 T ... and 24 T ..."""
    cases = [c for c in parity[0] if c[1].shape[1] == C33]
    dec = native.NativeDecoder(LABELS, blank_index=0)
    p_dev, sizes = _padded([p for _, p, _ in cases])
    targets = [t for _, _, t in cases]
    lp_s, st_s = dec.score(p_dev, sizes, np.arange(len(cases)), targets)
    lp_a, _, st_a = dec.alternatives(p_dev, sizes, np.arange(len(cases)), targets)
    assert not st_s.any() and not st_a.any()
    for (name, p, _), s, a in zip(cases, lp_s, lp_a):
        assert abs(float(s) - float(a)) <= ref.bound(len(p), s) + alt_ref.bound(len(p), s), (name, float(s), float(a))
    dec.close()


# ---- refusals
def test_refusals_write_nothing(native):
    dec = native.NativeDecoder(LABELS, blank_index=0)
    L = native.lib()
    B, T, N, Ls = 2, 10, 3, 3
    probs = torch.full((B, T, C33), 1.0 / C33, device="cuda")
    ok = dict(B=B, T=T, N=N, Ls=Ls, sizes=[10, 8], clip=[1, 0, 1], tg=[[1, 2, 3], [4, 5, 0], [0, 0, 0]], lens=[3, 2, 0], probs=probs)

    def call(out=("logp", "alt", "status"), **kw):
        a = dict(ok, **kw)
        lp = np.full(4, 7.5, dtype=np.float64)
        rows = np.full((4, 3, C33), 7.5, dtype=np.float64)
        st = np.full(4, 7, dtype=np.int32)
        arr = {k: np.ascontiguousarray(a[k], dtype=np.int32) for k in ("sizes", "clip", "tg", "lens")}
        rc = L.dsmi_alternatives(dec._h, a["probs"].data_ptr(), native._np_ptr(arr["sizes"]), a["B"], a["T"], native._np_ptr(arr["clip"]),
                                 native._np_ptr(arr["tg"]), native._np_ptr(arr["lens"]), a["N"], a["Ls"],
                                 native._np_ptr(lp) if "logp" in out else None, native._np_ptr(rows) if "alt" in out else None,
                                 native._np_ptr(st) if "status" in out else None, None)
        untouched = (lp == 7.5).all() and (rows == 7.5).all() and (st == 7).all()
        return rc, untouched, L.dsmi_decoder_last_error(dec._h).decode(), lp, rows, st

    rc, _, _, lp, rows, st = call()
    assert rc == 0 and st[:3].tolist() == [0, 0, 0] and np.isfinite(lp[:3]).all() and lp[3] == 7.5 and st[3] == 7
    assert np.isfinite(rows[0]).all() and np.isfinite(rows[1, :2]).all() and (rows[1, 2] == -np.inf).all() and (rows[2] == -np.inf).all()
    assert (rows[3] == 7.5).all()
    invalid = (dict(B=0), dict(T=0), dict(T=-3), dict(N=0), dict(N=-1), dict(Ls=-1), dict(sizes=[11, 8]), dict(sizes=[-1, 8]),
               dict(clip=[2, 0, 1]), dict(clip=[1, -1, 1]), dict(lens=[-1, 2, 0]), dict(lens=[4, 2, 0]),
               dict(tg=[[1, 0, 3], [4, 5, 0], [0, 0, 0]]), dict(tg=[[1, 2, 3], [4, C33, 0], [0, 0, 0]]),
               dict(tg=[[1, 2, -2], [4, 5, 0], [0, 0, 0]]), dict(out=("alt", "status")), dict(out=("logp", "alt")), dict(out=("logp", "status")))
    for kw in invalid:
        rc, untouched, msg, *_ = call(**kw)
        assert rc == native.DSMI_ERR_INVALID and untouched and msg, (kw, rc, msg)
    rc, *_ = call(out=("logp", "status"), Ls=0, lens=[0, 0, 0])          # no rows: no row array is needed
    assert rc == 0
    big = np.zeros((3, native.ALT_MAX_TOKENS + 1), dtype=np.int32)
    rc, untouched, msg, *_ = call(tg=big, Ls=native.ALT_MAX_TOKENS + 1)
    assert rc == native.DSMI_ERR_CAPACITY and untouched and "DSMI_ALT_MAX_TOKENS" in msg
    # N * L_stride * n_labels > 2^24: refused on the numbers alone, before any array is read past what is there
    many = (1 << 24) // (1024 * C33) + 1
    rc, untouched, msg, *_ = call(N=many, Ls=1024, clip=np.zeros(many), lens=np.zeros(many), tg=np.zeros((1, 1024)))
    assert rc == native.DSMI_ERR_CAPACITY and untouched and "2^24" in msg
    # the stored trellises: 5 candidates of 1024 tokens on 4096 frames, 5 x 4096 x 2049 > 2^25 elements
    long_probs = torch.full((1, 4096, C33), 1.0 / C33, device="cuda")
    tg = np.tile(np.array([1, 2], dtype=np.int32), (5, 512))
    rc, untouched, msg, *_ = call(probs=long_probs, B=1, T=4096, N=5, Ls=1024, sizes=[4096], clip=np.zeros(5), lens=np.full(5, 1024), tg=tg)
    assert rc == native.DSMI_ERR_CAPACITY and untouched and "2^25" in msg
    rc, *_ = call()
    assert rc == 0
    dec.close()


# ---- end to end: the synthetic cfgA-shaped model of test_gpu_score.py
def test_confidence_batch_equals_confidence_ids_in_callers_order(cfga):
    rec, clips = cfga
    eng = rec.danspeech_recognizer
    texts = rec.recognize_batch(clips)
    asked = [texts[0], "hej med dig", texts[2], "  Hej  DER", "ab" * 400]         # (the last: far more letters than frames)
    batch = rec.confidence_batch(clips, asked)
    job = eng._enqueue_batch(clips)
    job.collect_forward()
    norm = [eng.decoder.normalise_transcript(t) for t in asked]
    ids = [eng.decoder.transcript_ids(t) for t in norm]
    direct = eng.decoder.confidence_ids(job.probs, [ids[i] for i in job.order], job.sizes)
    assert sorted(job.order) == list(range(len(clips))) and list(job.order) != sorted(job.order)
    n_chars = 0
    for pos, i in enumerate(job.order):
        if direct[pos] is None:
            assert batch[i] is None
            continue
        words, chars = batch[i]
        logp, post = direct[pos]
        assert np.isfinite(logp) and post.shape == (len(norm[i]), C33)
        np.testing.assert_allclose(post.sum(axis=1), 1.0, rtol=0, atol=1e-12)
        assert "".join(ch for ch, *_ in chars) == norm[i] and [w for w, _ in words] == norm[i].split()
        for k, (ch, conf, other, other_conf) in enumerate(chars):
            assert conf == pytest.approx(post[k, ids[i][k]], abs=FORWARD_NOISE) and 0.0 < conf <= 1.0
            assert other != ch and 0.0 <= other_conf <= 1.0 and conf + other_conf <= 1.0 + 1e-12
            runner_up = np.delete(post[k], ids[i][k]).max()
            assert other_conf == pytest.approx(runner_up, abs=FORWARD_NOISE)
            n_chars += 1
        k = 0
        for word, conf in words:                                  # a word is as sure as its least sure character
            k = norm[i].index(word, k)
            assert conf == min(c for _, c, _, _ in chars[k:k + len(word)]) and 0.0 < conf <= 1.0
            k += len(word)
    assert n_chars > 20 and batch[4] is None
    single = rec.confidence(clips[1], asked[1])
    assert [w for w, _ in single[0]] == ["hej", "med", "dig"]
    assert "".join(ch for ch, *_ in single[1]) == "hej med dig"
    assert rec.confidence_batch([], []) == []
    with pytest.raises(ValueError, match="'#'"):
        rec.confidence_batch(clips[:1], ["nr #1"])
    with pytest.raises(ValueError):
        rec.confidence_batch(clips, asked[:2])


def test_recognize_confident_gives_the_recognised_texts(cfga):
    rec, clips = cfga
    texts = rec.recognize_batch(clips)
    out = rec.recognize_confident(clips)
    assert [t for t, _, _ in out] == texts
    for text, words, chars in out:
        assert "".join(ch for ch, *_ in chars) == text
        assert all(0.0 < conf <= 1.0 for _, conf, _, _ in chars) and all(0.0 < conf <= 1.0 for _, conf in words)
        assert len(words) == len("".join(ch for ch, *_ in chars).split())
    assert rec.danspeech_recognizer.transcribe_confident_batch([]) == []
