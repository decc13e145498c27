"""CTC transcript scoring on the GPU (dsmi_score, csrc/score.hip) against a brute force over every frame labelling and the
float64 numpy reference of tests/_score_ref.py (held to the contract's bound 8 T 2^-52 max(1, |logp|)), batch invariance on a
ragged batch, cross-checks with dsmi_align and dsmi_beam, its refusals, and the recogniser surface end to end on a synthetic
cfgA-shaped model."""
import numpy as np
import pytest

from danspeech_amd import synthetic as syn

import _align_ref as aref
import _ctc_edge_cases as edge
import _score_ref as ref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
LABELS = syn.DANSPEECH_LABELS
C33 = len(LABELS)


@pytest.fixture(scope="module")
def native():
    from danspeech_amd import _native
    return _native


def _padded(probs_list, T_out=None, fill=None):
    """[B, T_out, C] on the device with ``fill`` (default 1 / C) past each clip's frames, and the sizes."""
    T = T_out or max(len(p) for p in probs_list)
    C = probs_list[0].shape[1]
    x = np.full((len(probs_list), max(T, 1), C), 1.0 / C if fill is None else fill, dtype=np.float32)
    for b, p in enumerate(probs_list):
        x[b, :len(p)] = p
    return torch.from_numpy(x).cuda(), np.array([len(p) for p in probs_list], dtype=np.int32)


def _targets(rng, L, C=C33):
    return [int(x) for x in rng.integers(1, C, size=L)]


# ---- every alignment, enumerated
@pytest.mark.parametrize("C", [3, 4])
def test_brute_force_small_cases(native, C):
    """T in {1, 2, 5, 6}: every feasible transcript and one infeasible one against the sum over every frame labelling.  1e-12 in
    the log: the brute force adds at most 4^6 products of 6 factors in float64 (a relative 4096 x 2^-53 = 4.5e-13 at the very
    worst), the contract's bound at T = 6 and |logp| < 50 is 5.4e-13."""
    dec = native.NativeDecoder(["_", "a", "b", "c"][:C], blank_index=0)
    rng = np.random.default_rng(10 + C)
    n = 0
    for T in (1, 2, 5, 6):
        p = rng.dirichlet(np.ones(C) * 0.5, size=T).astype(np.float32)
        sums = ref.brute_force(p)
        seqs = [list(k) for k in sums] + [[1, 2] * T]
        p_dev, sizes = _padded([p])
        lp, status = dec.score(p_dev, sizes, [0] * len(seqs), seqs)
        assert status.tolist() == [0] * len(sums) + [1] and lp[-1] == -np.inf
        for k, seq in enumerate(seqs[:-1]):
            want = float(np.log(sums[tuple(seq)]))
            assert abs(float(lp[k]) - want) <= 1e-12, (T, seq, float(lp[k]), want)
            n += 1
    assert n >= 74                                               # (two labels: 3 + 5 + 23 + 43 feasible transcripts)
    dec.close()


# ---- the reference, computed once for the module
def _parity_cases():
    rng = np.random.default_rng(21)
    cases = []
    for T in (15, 16, 17, 31, 32, 33, 64):                       # the chunk edges
        for L in (0, 1, T // 3):
            cases.append(("T%d L%d" % (T, L), ref.peaky(rng, T, C33), _targets(rng, L)))
    for L in (0, 1, 127, 128, 129):                              # S = 1, 3, 255, 257, 259: across the 256 threads
        cases.append(("T260 L%d" % L, ref.peaky(rng, 260, C33), _targets(rng, L)))
    t = [1 + k % 5 for k in range(33)]                           # exactly feasible: one token per frame, a single path
    cases.append(("single path", ref.peaky(rng, 33, C33), t))
    cases.append(("single path of a run", ref.peaky(rng, 17, C33), [4] * 9))          # a, blank, a, ..., a: 17 frames
    cases.append(("aa runs", ref.peaky(rng, 64, C33), [1, 1, 2, 2, 2, 3, 1, 1, 7, 7, 7, 7, 2, 3, 3, 1, 9, 9, 1, 1]))
    p, t = ref.peaky(rng, 32, C33), _targets(rng, 8)
    p[:, t[2]] = 0.0                                             # p = 0 on a needed label: the FLT_MIN clip
    cases.append(("p = 0 on a needed label", p, t))
    cases.append(("501 x 150", ref.peaky(rng, 501, C33, 3.0), _targets(rng, 150)))
    return cases


@pytest.fixture(scope="module")
def parity():
    cases = _parity_cases()
    return cases, [ref.forward(p, t) for _, p, t in cases]


def _share_of_bound(got, want, T):
    return abs(float(got) - float(want)) / ref.bound(T, want)


def test_reference_parity_within_the_bound(native, parity):
    cases, want = parity
    assert all(w is not None and np.isfinite(w) for w in want)
    dec = native.NativeDecoder(LABELS, blank_index=0)
    p_dev, sizes = _padded([p for _, p, _ in cases])
    lp, status = dec.score(p_dev, sizes, np.arange(len(cases)), [t for _, _, t in cases])
    assert not status.any()
    worst = 0.0
    for k, (name, p, t) in enumerate(cases):
        share = _share_of_bound(lp[k], want[k], len(p))
        print("%-26s logp %.9f  %.4f of the bound" % (name, lp[k], share))
        assert share <= 1.0, (name, float(lp[k]), float(want[k]))
        worst = max(worst, share)
    print("worst share of the bound: %.4f" % worst)
    assert float(want[[n for n, _, _ in cases].index("p = 0 on a needed label")]) < np.log(float(ref.FLT_MIN))
    dec.close()


@pytest.mark.parametrize("shape", edge.SHAPES + edge.LONG, ids=edge.name)
def test_feeder_edges(native, shape):
    """The shared feeder's chunk boundaries, image wrap and widths (tests/_ctc_edge_cases.py): every row of both clips within
    the contract's bound of the float64 reference.  No point is left out: the parity cases above pass T = 15 .. 33 at 33 labels,
    but one clip per T_out, never 3 or 128 labels and never a shorter clip beside it."""
    T, C, L = shape
    probs, rows = edge.case(T, C, L)
    clip = [b for b, rs in enumerate(rows) for _ in rs]
    targets = [r for rs in rows for r in rs]
    dec = native.NativeDecoder(edge.labels(C), blank_index=0)
    p_dev, sizes = _padded(probs)
    assert p_dev.shape[1] == T and sizes[1] < T
    lp, status = dec.score(p_dev, sizes, clip, targets)
    assert not status.any()
    for n, (b, t) in enumerate(zip(clip, targets)):
        want = ref.forward(probs[b], t)
        assert want is not None and _share_of_bound(lp[n], want, len(probs[b])) <= 1.0, (n, b, float(lp[n]), float(want))
    dec.close()


def test_longest_candidate(native):
    """DSMI_SCORE_MAX_TOKENS tokens on 4200 frames: the largest LDS carve, 17 states per thread."""
    dec = native.NativeDecoder(LABELS, blank_index=0)
    rng = np.random.default_rng(13)
    t = _targets(rng, native.SCORE_MAX_TOKENS)
    T = 4200
    assert aref.min_frames(t) <= T
    p = ref.peaky(rng, T, C33, sharp=2.0)
    want = ref.forward(p, t)
    p_dev, sizes = _padded([p])
    lp, status = dec.score(p_dev, sizes, [0], [t])
    share = _share_of_bound(lp[0], want, T)
    print("2048 tokens on 4200 frames: logp %.6f, %.4f of the bound" % (lp[0], share))
    assert status[0] == 0 and share <= 1.0, (float(lp[0]), float(want))
    dec.close()


# ---- a ragged batch: NaN past every clip's frames, many candidates per clip in scrambled order, each as if scored alone
def test_ragged_batch_is_batch_invariant_and_reads_no_frame_past_a_clip(native):
    dec = native.NativeDecoder(LABELS, blank_index=0)
    rng = np.random.default_rng(31)
    frames = [64, 50, 33, 17, 40]
    probs = [ref.peaky(rng, T, C33) for T in frames]
    p_dev, sizes = _padded(probs, T_out=70, fill=np.nan)
    clip, targets = [], []
    for b, count in enumerate([0, 1, 3, 40, 3]):
        for k in range(count):
            clip.append(b)
            targets.append(_targets(rng, int(rng.integers(0, frames[b] // 2 + 1))))
    targets[2] = []                                               # an empty transcript
    targets[7] = [5] * 12                                         # 12 + 11 frames > 17: infeasible
    perm = rng.permutation(len(clip))
    clip, targets = [clip[i] for i in perm], [targets[i] for i in perm]
    lp, status = dec.score(p_dev, sizes, clip, targets)
    n_bad = 0
    for n, (b, t) in enumerate(zip(clip, targets)):
        want = ref.forward(probs[b], t)
        if want is None:
            assert status[n] == 1 and lp[n] == -np.inf
            n_bad += 1
            continue
        assert status[n] == 0 and _share_of_bound(lp[n], want, frames[b]) <= 1.0, (n, b, float(lp[n]), float(want))
    assert n_bad >= 1
    alone = np.array([dec.score(p_dev, sizes, [b], [t])[0][0] for b, t in zip(clip, targets)])
    np.testing.assert_array_equal(lp, alone)
    # ... and with only its own clip in the call
    for n in (0, 11, 30):
        p1, s1 = _padded([probs[clip[n]]])
        assert dec.score(p1, s1, [0], [targets[n]])[0][0] == lp[n]
    # no sizes: every clip has T_out frames
    p_full, _ = _padded(probs[:1] * 2)
    lp2, _ = dec.score(p_full, None, [1, 0], [[3, 4], [3, 4]])
    assert lp2[0] == lp2[1] and _share_of_bound(lp2[0], ref.forward(probs[0], [3, 4]), 64) <= 1.0
    # no frames: the empty transcript alone is feasible, with probability 1
    lp0, st0 = dec.score(p_dev, np.array([0, 5, 5, 5, 5], dtype=np.int32), [0, 0], [[], [3]])
    assert lp0.tolist() == [0.0, -np.inf] and st0.tolist() == [0, 1]
    dec.close()


# ---- against the kernels that are there already
def test_sum_over_paths_is_at_least_the_best_path(native):
    dec = native.NativeDecoder(LABELS, blank_index=0)
    rng = np.random.default_rng(41)
    frames = [501, 260, 64, 33, 9]
    probs = [ref.peaky(rng, T, C33) for T in frames]
    targets = [_targets(rng, T // 4) for T in frames]
    p_dev, sizes = _padded(probs)
    spans, _, _, st_a = dec.align(p_dev, sizes, targets)
    lp, st_s = dec.score(p_dev, sizes, np.arange(len(frames)), targets)
    assert not st_a.any() and not st_s.any()
    for b, t in enumerate(targets):
        best = aref.rescore64(probs[b], aref.path_from_spans(spans[b, :len(t)], t, frames[b]))
        assert lp[b] >= best - 1e-9, (b, float(lp[b]), best)
    dec.close()


def _real_beams(ln, sc):
    """Beams the search filled with a prefix of non-zero probability: an unfilled one is empty with score 0 behind the first,
    and a prefix no path of the frames emits (`aa` in two frames) sits in the trie with an infinite score."""
    return [p for p in range(len(ln)) if np.isfinite(sc[p]) and not (p > 0 and ln[p] == 0 and sc[p] == 0.0)]


@pytest.mark.parametrize("T, C", [(4, 3), (5, 3), (3, 4), (6, 3)])
def test_unpruned_beam_search_scores_are_the_likelihoods(native, T, C):
    """No language model, no vocabulary cut and a beam wider than the number of prefixes (at most 127 here): the prefix search
    loses nothing, so each beam's score is minus the likelihood of its transcript -- to the float32 the score is returned in,
    2^-22 max(1, |score|)."""
    dec = native.NativeDecoder(["_", "a", "b", "c"][:C], blank_index=0)
    p = np.random.default_rng(50 + T + C).dirichlet(np.ones(C), size=T).astype(np.float32)
    p_dev, sizes = _padded([p])
    tok, _, ln, sc = dec.beam(p_dev, sizes, beam_width=128, cutoff_top_n=40, cutoff_prob=1.0)
    real = _real_beams(ln[0], sc[0])
    assert len(real) == sum(1 for s in ref.all_sequences(T, C) if aref.min_frames(s) <= T)
    lp, status = dec.score(p_dev, sizes, [0] * len(real), [tok[0, q, :ln[0, q]] for q in real])
    assert not status.any()
    for k, q in enumerate(real):
        score = float(sc[0, q])
        assert abs(-score - lp[k]) <= 2.0 ** -22 * max(1.0, abs(score)), (q, score, float(lp[k]))
    dec.close()


def test_pruned_beam_search_scores_are_lower_bounds(native):
    """64 peaky frames at beam 16: pruning only loses paths."""
    dec = native.NativeDecoder(LABELS, blank_index=0)
    p = ref.peaky(np.random.default_rng(61), 64, C33)
    p_dev, sizes = _padded([p])
    tok, _, ln, sc = dec.beam(p_dev, sizes, beam_width=16, cutoff_top_n=40, cutoff_prob=1.0)
    real = _real_beams(ln[0], sc[0])
    assert len(real) == 16 and len(set(tuple(tok[0, q, :ln[0, q]]) for q in real)) == 16
    lp, status = dec.score(p_dev, sizes, [0] * len(real), [tok[0, q, :ln[0, q]] for q in real])
    assert not status.any()
    for k, q in enumerate(real):
        score = float(sc[0, q])
        assert lp[k] >= -score - 2.0 ** -22 * max(1.0, abs(score)), (q, score, float(lp[k]))
    dec.close()


# ---- refusals
def test_refusals_write_nothing(native):
    dec = native.NativeDecoder(LABELS, blank_index=0)
    L = native.lib()
    B, T, N, Ls = 2, 10, 3, 3
    probs = torch.full((B, T, C33), 1.0 / C33, device="cuda")
    ok = dict(B=B, T=T, N=N, Ls=Ls, sizes=[10, 8], clip=[1, 0, 1], tg=[[1, 2, 3], [4, 5, 0], [0, 0, 0]], lens=[3, 2, 0])

    def call(out=True, **kw):
        a = dict(ok, **kw)
        lp = np.full(4, 7.5, dtype=np.float64)
        st = np.full(4, 7, dtype=np.int32)
        arr = {k: np.ascontiguousarray(a[k], dtype=np.int32) for k in ("sizes", "clip", "tg", "lens")}
        rc = L.dsmi_score(dec._h, probs.data_ptr(), native._np_ptr(arr["sizes"]), a["B"], a["T"], native._np_ptr(arr["clip"]),
                          native._np_ptr(arr["tg"]), native._np_ptr(arr["lens"]), a["N"], a["Ls"],
                          native._np_ptr(lp) if out in (True, "logp") else None, native._np_ptr(st) if out in (True, "status") else None, None)
        untouched = (lp == 7.5).all() and (st == 7).all()
        return rc, untouched, L.dsmi_decoder_last_error(dec._h).decode(), lp, st

    rc, _, _, lp, st = call()
    assert rc == 0 and st[:3].tolist() == [0, 0, 0] and np.isfinite(lp[:3]).all() and lp[3] == 7.5 and st[3] == 7
    big = np.zeros((3, native.SCORE_MAX_TOKENS + 1), dtype=np.int32)
    invalid = (dict(B=0), dict(T=0), dict(T=-3), dict(N=0), dict(N=-1), dict(sizes=[11, 8]), dict(sizes=[-1, 8]), dict(clip=[2, 0, 1]),
               dict(clip=[1, -1, 1]), dict(lens=[-1, 2, 0]), dict(lens=[4, 2, 0]), dict(tg=[[1, 0, 3], [4, 5, 0], [0, 0, 0]]),
               dict(tg=[[1, 2, 3], [4, C33, 0], [0, 0, 0]]), dict(tg=[[1, 2, -2], [4, 5, 0], [0, 0, 0]]), dict(out="logp"), dict(out="status"))
    for kw in invalid:
        rc, untouched, msg, _, _ = call(**kw)
        assert rc == native.DSMI_ERR_INVALID and untouched and msg, (kw, rc, msg)
    rc, untouched, msg, _, _ = call(tg=big, Ls=native.SCORE_MAX_TOKENS + 1)
    assert rc == native.DSMI_ERR_CAPACITY and untouched and "DSMI_SCORE_MAX_TOKENS" in msg
    # N * L_stride > 2^24: refused on the numbers alone, before any array is read past what is there
    many = (1 << 24) // 2048 + 1
    rc, untouched, msg, _, _ = call(N=many, Ls=2048, clip=np.zeros(many), lens=np.zeros(many), tg=np.zeros((1, 2048)))
    assert rc == native.DSMI_ERR_CAPACITY and untouched and "2^24" in msg
    rc, _, _, _, _ = call()
    assert rc == 0
    dec.close()


# ---- decoders: decode_scored on probabilities that are there
def test_decode_scored_of_both_decoders():
    from danspeech_amd.deepspeech.decoder import BeamCTCDecoder, GreedyDecoder
    rng = np.random.default_rng(71)
    frames = [64, 40, 17]
    probs = [ref.peaky(rng, T, C33, sharp=5.0) for T in frames]
    p_dev, sizes = _padded(probs)
    beam = BeamCTCDecoder(LABELS, beam_width=8, blank_index=0)
    strings, offsets = beam.decode(p_dev, sizes)
    last = beam.last_scores.copy()
    s2, o2, logps = beam.decode_scored(p_dev, sizes, n_best=3)
    np.testing.assert_array_equal(beam.last_scores, last)
    assert [s[:3] for s in strings] == s2 and all(len(row) == 3 for row in logps)
    for b in range(3):
        for q in range(3):
            assert (offsets[b][q] == o2[b][q]).all()
            want = ref.forward(probs[b], beam.transcript_ids(s2[b][q]))
            assert _share_of_bound(logps[b][q], want, frames[b]) <= 1.0
            assert logps[b][q] >= -float(last[b, q]) - 2.0 ** -22 * max(1.0, abs(float(last[b, q])))
    assert len(beam.decode_scored(p_dev, sizes)[2][0]) == 8
    greedy = GreedyDecoder(LABELS, blank_index=0)
    gs, go = greedy.decode(p_dev, sizes)
    gs2, go2, glp = greedy.decode_scored(p_dev, sizes)
    assert gs == gs2 and all((a[0] == b[0]).all() for a, b in zip(go, go2))
    for b in range(3):
        assert _share_of_bound(glp[b][0], ref.forward(probs[b], greedy.transcript_ids(gs[b][0])), frames[b]) <= 1.0
    # Decoder.score: normalised, checked before any GPU work, None for what cannot fit
    out = greedy.score(p_dev, [["  Hej  DER", "hej der"], [], ["a" * 17, "ab" * 4]], sizes)
    assert out[0][0] == out[0][1] and out[1] == [] and out[2][0] is None and out[2][1] is not None
    with pytest.raises(ValueError, match="'#'"):
        greedy.score(p_dev, [["ok"], ["nr #1"], []], sizes)
    with pytest.raises(ValueError):
        greedy.score(p_dev, [["ok"]], sizes)


# ---- end to end: a synthetic cfgA-shaped model (2 conv, 5 x BiGRU 800) with sharpened FC weights
@pytest.fixture(scope="module")
def cfga():
    from danspeech_amd import Recognizer
    from danspeech_amd.deepspeech.model import DeepSpeech
    sd = syn.make_state_dict(2, "gru", 800, 5, seed=0, fc_gain=8.0)
    model = DeepSpeech("cfgA", rnn_type="gru", rnn_hidden_size=800, rnn_layers=5, conv_layers=2).load_state_dict(sd)
    rec = Recognizer(model=model)
    clips = [syn.make_clip(i, n) for i, n in enumerate([48000, 160000, 32000, 96000, 71234])]
    return rec, clips


# Two forwards of the same batch feed the two sides of the comparisons below.  Where they are not the same bits, the float32
# probabilities differ by their rounding, 2^-24 relative per frame's lp factor, which moves logp by at most frames x 2^-24 <
# 501 x 6e-8 = 3e-5 absolute: 1e-4 covers it on these clips of at most 500 frames.
FORWARD_NOISE = 1e-4


def test_score_batch_equals_score_ids_in_callers_order(cfga):
    rec, clips = cfga
    eng = rec.danspeech_recognizer
    texts = rec.recognize_batch(clips)
    cands = [[texts[i], "hej med dig", texts[(i + 1) % len(clips)], ""][:1 + i % 4] for i in range(len(clips))]
    cands[2] = cands[2] + ["a" * 1500]                           # far more letters than frames
    batch = rec.score_batch(clips, cands)
    job = eng._enqueue_batch(clips)
    job.collect_forward()
    norm = [[eng.decoder.normalise_transcript(t) for t in c] for c in cands]
    ids = [[eng.decoder.transcript_ids(t) for t in c] for c in norm]
    direct = eng.decoder.score_ids(job.probs, [ids[i] for i in job.order], job.sizes)
    sizes = job.sizes.numpy()
    assert sorted(job.order) == list(range(len(clips))) and list(job.order) != sorted(job.order)
    for pos, i in enumerate(job.order):
        assert len(batch[i]) == len(cands[i])
        feasible = [r for r in batch[i] if r is not None]
        assert sum(share for *_, share in feasible) == pytest.approx(1.0, abs=1e-12)
        for k, r in enumerate(batch[i]):
            if direct[pos][k] is None:
                assert r is None
                continue
            text, logp, conf, share = r
            assert text == norm[i][k] and logp == pytest.approx(direct[pos][k], abs=FORWARD_NOISE)
            assert conf == pytest.approx(np.exp(logp / sizes[pos]), rel=1e-12) and 0 <= share <= 1      # (0: exp underflows beside a far likelier one)
    assert batch[2][-1] is None
    single = rec.score(clips[3], cands[3])
    assert [r[0] for r in single] == [r[0] for r in batch[3]]
    # (a forward of the clip alone: another batch shape, held as test_gpu_align.py holds the same comparison)
    np.testing.assert_allclose([r[1] for r in single], [r[1] for r in batch[3]], rtol=1e-5)
    assert rec.score_batch([], []) == [] and rec.score(clips[0], []) == []
    with pytest.raises(ValueError):
        rec.score_batch(clips, cands[:2])


def test_recognize_scored_gives_the_recognised_texts_and_their_likelihoods(cfga):
    rec, clips = cfga
    eng = rec.danspeech_recognizer
    with pytest.warns(Warning):
        beams = rec.recognize_batch(clips, show_all=True)
    scored = rec.recognize_scored(clips, n_best=1)
    assert [[t for t, _ in row] for row in scored] == [list(b[:1]) for b in beams]
    # the likelihood is of the hypothesis' label sequence as it is; `score` normalises its candidates first, so the two agree
    # where the text is its own normal form -- and always with the ids scored as they are
    job = eng._enqueue_batch(clips)
    job.collect_forward()
    raw = eng.decoder.score_ids(job.probs, [[eng.decoder.transcript_ids(scored[i][0][0])] for i in job.order], job.sizes)
    via_score = rec.score_batch(clips, [[row[0][0]] for row in scored])
    n_same = 0
    for pos, i in enumerate(job.order):
        text, logp = scored[i][0]
        assert logp is not None and logp == pytest.approx(raw[pos][0], abs=FORWARD_NOISE)
        if eng.decoder.normalise_transcript(text) == text:
            assert via_score[i][0][1] == pytest.approx(logp, abs=FORWARD_NOISE)
            n_same += 1
    print("%d of %d recognised texts are their own normal form" % (n_same, len(clips)))
    assert eng.transcribe_scored_batch([]) == []
