"""Batched edit distance on the GPU (dsmi_edit_distance, csrc/edit.hip): the four counts against the references of
tests/_edit_ref.py at every lane and stripe edge, crafted pairs for the tie rule, shared pool rows, extreme token values, packed
lane segments that must not leak into each other, the large cases, capacity growth, every refusal, and the Python surface up to
Recognizer.recognize_min_risk / evaluate on a synthetic cfgA-shaped model.  Results are integers: every comparison is exact."""
import numpy as np
import pytest

from danspeech_amd import synthetic as syn

import _edit_ref as ref
import _score_ref as sref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
LABELS = syn.DANSPEECH_LABELS
C33 = len(LABELS)
I32 = np.iinfo(np.int32)


@pytest.fixture(scope="module")
def native():
    from danspeech_amd import _native
    return _native


@pytest.fixture(scope="module")
def dec(native):
    d = native.NativeDecoder(LABELS, blank_index=0)
    yield d
    d.close()


def _check(dec, pool, pairs, what=""):
    got = dec.edit_distance(pool, pairs)
    want = ref.counts_of(pool, pairs)
    assert got.dtype == np.int32 and got.shape == (len(pairs), 4)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, (what, [(tuple(pairs[n]), len(pool[pairs[n][0]]), len(pool[pairs[n][1]]), got[n].tolist(), want[n].tolist()) for n in bad[:5]])
    return got


# ---- lane and stripe edges: every len_b at which a segment width, a lane or a stripe changes, short and long a
LEN_B = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 130)
LEN_A = (0, 1, 2, 63, 64, 65, 200)


@pytest.mark.parametrize("symbols", [2, 4, 33])
def test_lane_and_stripe_edges(dec, symbols):
    rng = np.random.default_rng(symbols)
    pool, pairs = [], []
    for la in LEN_A:
        for lb in LEN_B:
            pool += [rng.integers(0, symbols, la), rng.integers(0, symbols, lb)]
            pairs.append((len(pool) - 2, len(pool) - 1))
    _check(dec, pool, pairs, "edges over %d symbols" % symbols)


# ---- crafted pairs around the stripe edge
@pytest.mark.parametrize("n", [64, 65, 128])
def test_crafted_pairs(dec, n):
    rng = np.random.default_rng(n)
    base = rng.integers(1, 30, n)
    pool, pairs = [base], []

    def add(a, b):
        pool.extend([np.asarray(a), np.asarray(b)])
        pairs.append((len(pool) - 2, len(pool) - 1))

    add(base, base.copy())                                   # identical
    add(base, base + 100)                                    # nothing in common
    for col in sorted(set([0, n - 1, min(63, n - 1), min(64, n - 1)])):      # one difference: first, last, columns 64 and 65
        other = base.copy()
        other[col] = 99
        add(base, other)
        add(other, base)
    at_shift = len(pairs)
    add(base, np.concatenate([base[1:], [77]]))              # itself shifted by one token: an insertion and a deletion against n substitutions
    add(np.concatenate([[77], base[:-1]]), base)
    alt = np.tile([1, 2], n)[:n]                             # a b a b ... against b a b a ...: (2, 0, 1, 1), never n substitutions
    add(alt, 3 - alt)
    for m in (1, n - 1, n, n + 1, 2 * n):                    # [x] * n against [x] * m
        add([5] * n, [5] * m)
        add([5] * m, [5] * n)
    got = _check(dec, pool, pairs, "crafted at %d" % n)
    assert got[0].tolist() == [0, 0, 0, 0] and got[1].tolist() == [n, n, 0, 0]
    assert got[at_shift].tolist() == [2, 0, 1, 1] and got[at_shift + 1].tolist() == [2, 0, 1, 1] and got[at_shift + 2].tolist() == [2, 0, 1, 1]


def test_shared_sequences_and_token_values(dec):
    rng = np.random.default_rng(5)
    extremes = np.array([I32.min, -1, 0, I32.max], dtype=np.int64)
    pool = [rng.integers(0, 4, L) for L in (70, 20, 33, 130, 9)]
    pool += [extremes[rng.integers(0, 4, L)] for L in (5, 40, 100)]
    pool += [np.array([0, 0, 0]), np.array([I32.min, 0, -1]), np.array([-1, -1, -1, I32.max])]
    M = len(pool)
    pairs = [(m, m) for m in range(M)] + [(0, m) for m in range(M)] + [(m, 0) for m in range(M)] + [(a, b) for a in range(5, M) for b in range(5, M)]
    got = _check(dec, pool, pairs, "shared rows and extreme tokens")
    assert (got[:M] == 0).all()


# ---- packed segments: two or four pairs share a wave and must not see each other
def test_packed_segments_do_not_leak(dec, native):
    rng = np.random.default_rng(17)
    la, lb = [], []
    for lo, n in ((1, 100), (17, 100)):                      # the 16- and 32-lane classes: wave-mates are neighbours in the order by a's length
        a_lens = rng.permutation(np.arange(1, 151))[:n]      # distinct, so neighbours differ
        ranks = np.argsort(np.argsort(-a_lens))
        la += a_lens.tolist()
        lb += (lo + ranks * 5 % 16).tolist()                 # any 4 consecutive ranks: 4 different lengths of b
    la += rng.integers(1, 150, 60).tolist()                  # one pair per wave, one to three stripes
    lb += rng.integers(33, 180, 60).tolist()
    scramble = rng.permutation(len(la))
    la, lb = np.array(la)[scramble], np.array(lb)[scramble]
    N, Ls = len(la), 192
    order, seg = native.edit_plan(la, lb)
    assert sorted(set(seg.tolist())) == [16, 32, 64] and len(order) == N
    start = 0
    for s in (16, 32):                                       # the waves as dsmi_edit_plan documents them
        members = [n for n in order if seg[n] == s]
        assert order[start:start + len(members)].tolist() == members
        for k in range(0, len(members), 64 // s):
            mates = members[k:k + 64 // s]
            assert len(set(la[mates])) == len(mates) and len(set(lb[mates])) == len(mates)
        start += len(members)
    # row 2n is a, row 2n+1 is b; past its length each row goes on with the tokens of its partner, which WOULD match
    pool = np.zeros((2 * N, Ls), dtype=np.int32)
    for n in range(N):
        long = rng.integers(0, 3, Ls)
        pool[2 * n], pool[2 * n + 1] = long, long
        pool[2 * n, :la[n]] = rng.integers(0, 3, la[n])
        pool[2 * n + 1, :lb[n]] = rng.integers(0, 3, lb[n])
    lens = np.stack([la, lb], axis=1).reshape(-1).astype(np.int32)
    pairs = np.stack([2 * np.arange(N), 2 * np.arange(N) + 1], axis=1)
    together = dec.edit_distance(pool, pairs, lens)
    alone = np.concatenate([dec.edit_distance(pool[2 * n:2 * n + 2], [(0, 1)], lens[2 * n:2 * n + 2]) for n in range(N)])
    np.testing.assert_array_equal(together, alone)
    np.testing.assert_array_equal(together, ref.counts_of([pool[m, :lens[m]] for m in range(2 * N)], pairs))


# ---- larger cases
def test_2048_pairs_of_150(dec):
    rng = np.random.default_rng(23)
    A = rng.integers(1, C33, (2048, 150))
    B = np.where(rng.random((2048, 150)) < 0.15, rng.integers(1, C33, (2048, 150)), A)      # a noisy copy, then some rows unrelated
    B[::7] = rng.integers(1, C33, (len(B[::7]), 150))
    pool = np.concatenate([A, B]).astype(np.int32)
    pairs = np.stack([np.arange(2048), np.arange(2048) + 2048], axis=1)
    got = dec.edit_distance(pool, pairs, np.full(4096, 150, dtype=np.int32))
    np.testing.assert_array_equal(got, ref.row_dp_batch(A, B))


def test_longest_sequences(dec, native):
    rng = np.random.default_rng(29)
    n = native.EDIT_MAX_TOKENS
    a = rng.integers(0, 4, n)
    b = a.copy()
    b[rng.integers(0, n, 600)] = 7
    b = np.concatenate([b[300:], rng.integers(0, 4, 300)])
    _check(dec, [a, b, np.array([a[1234]]), np.array([9])], [(0, 1), (0, 2), (0, 3), (2, 0)], "4096 x 4096, 4096 x 1")


def test_capacity_growth(dec):
    rng = np.random.default_rng(31)
    small = [rng.integers(0, 5, L) for L in (40, 70, 3, 18)]
    small_pairs = [(0, 1), (1, 0), (2, 3), (3, 1)]
    first = dec.edit_distance(small, small_pairs)
    big = [rng.integers(0, 5, 500 + k) for k in range(64)]     # (a larger pool, more pairs, and a boundary column in LDS)
    big_pairs = [(k, (k * 7 + 1) % 64) for k in range(64)]
    _check(dec, big, big_pairs, "a call that grows the workspace")
    np.testing.assert_array_equal(dec.edit_distance(small, small_pairs), first)
    np.testing.assert_array_equal(first, ref.counts_of(small, small_pairs))


def test_trivial_pairs_alone_launch_nothing(dec):
    got = dec.edit_distance([[], [1, 2, 3], []], [(0, 1), (1, 0), (0, 2), (2, 0)])
    assert got.tolist() == [[3, 0, 0, 3], [3, 0, 3, 0], [0, 0, 0, 0], [0, 0, 0, 0]]
    assert dec.edit_distance(np.zeros((2, 0), dtype=np.int32), [(0, 1)], np.zeros(2, dtype=np.int32)).tolist() == [[0, 0, 0, 0]]


# ---- refusals
def test_refusals_write_nothing(native):
    dec = native.NativeDecoder(LABELS, blank_index=0)
    L = native.lib()
    ok = dict(M=3, Ls=4, N=2, seqs=[[1, 2, 3, 4], [1, 2, 0, 0], [0, 0, 0, 0]], lens=[4, 2, 0], pa=[0, 2], pb=[1, 0])

    def call(null=(), **kw):
        a = dict(ok, **kw)
        counts = np.full((3, 4), -77, dtype=np.int32)
        arr = {k: np.ascontiguousarray(a[k], dtype=np.int32) for k in ("seqs", "lens", "pa", "pb")}
        ptr = {k: None if k in null else native._np_ptr(v) for k, v in arr.items()}
        rc = L.dsmi_edit_distance(dec._h, ptr["seqs"], ptr["lens"], a["M"], a["Ls"], ptr["pa"], ptr["pb"], a["N"],
                                  None if "counts" in null else native._np_ptr(counts), None)
        return rc, bool((counts == -77).all()), L.dsmi_decoder_last_error(dec._h).decode(), counts

    rc, _, _, counts = call()
    assert rc == 0 and counts[:2].tolist() == [[2, 0, 2, 0], [4, 0, 0, 4]] and (counts[2] == -77).all()
    invalid = (dict(M=0), dict(M=-1), dict(N=0), dict(N=-5), dict(Ls=-1), dict(lens=[5, 2, 0]), dict(lens=[4, -1, 0]), dict(pa=[3, 2]),
               dict(pa=[0, -1]), dict(pb=[1, 3]), dict(pb=[-2, 0]), dict(null=("seqs",)), dict(null=("lens",)), dict(null=("pa",)),
               dict(null=("pb",)), dict(null=("counts",)))
    for kw in invalid:
        rc, untouched, msg, _ = call(**kw)
        assert rc == native.DSMI_ERR_INVALID and untouched and msg, (kw, rc, msg)
    # on the numbers alone: the arrays are far smaller than the call declares and must not be read
    big = native.EDIT_MAX_TOKENS + 1
    rc, untouched, msg, _ = call(Ls=big)
    assert rc == native.DSMI_ERR_CAPACITY and untouched and "DSMI_EDIT_MAX_TOKENS" in msg
    rc, untouched, msg, _ = call(M=(1 << 24) // 4096 + 1, Ls=4096)
    assert rc == native.DSMI_ERR_CAPACITY and untouched and "M * L_stride" in msg
    rc, untouched, msg, _ = call(N=(1 << 24) + 1)
    assert rc == native.DSMI_ERR_CAPACITY and untouched and "N exceeds" in msg
    rc, _, _, _ = call(null=("seqs",), Ls=0, lens=[0, 0, 0])      # no columns: no pool needed
    assert rc == 0
    rc, _, _, counts = call()
    assert rc == 0 and counts[:2].tolist() == [[2, 0, 2, 0], [4, 0, 0, 4]]
    dec.close()
    with pytest.raises(native.DsmiError):
        native.edit_plan([1, -1], [2, 2])
    with pytest.raises(native.DsmiError):
        native.edit_plan([], [])


# ---- the decoders' surface
REFS = ["det er en god dag i dag", "jeg hedder søren og jeg bor i århus", "", "rødgrød med fløde", "ja ja ja nej ja", "på  gensyn   i morgen ", "hej"]
HYPS = ["det er god dag i dag dag", "jeg hedder søren jeg bor i aarhus nu", "ingenting", "", "ja nej ja ja", "på gensyn i morgen", "hej"]


def test_wer_and_cer_batches_equal_the_loops():
    from danspeech_amd.deepspeech.decoder import GreedyDecoder
    d = GreedyDecoder(LABELS, blank_index=0)
    assert d.wer_batch(REFS, HYPS) == [d.wer(r, h) for r, h in zip(REFS, HYPS)]
    assert d.cer_batch(REFS, HYPS) == [d.cer(r, h) for r, h in zip(REFS, HYPS)]
    counts, ref_lens = d.error_counts(REFS, HYPS)
    assert ref_lens.tolist() == [len(r.split()) for r in REFS]
    assert counts[0].tolist() == [2, 0, 1, 1] and counts[2].tolist() == [1, 0, 0, 1] and counts[3].tolist() == [3, 0, 3, 0]
    ccounts, cref = d.error_counts(REFS, HYPS, unit="char")
    assert cref.tolist() == [len(r.replace(" ", "")) for r in REFS] and ccounts[5].tolist() == [0, 0, 0, 0]
    # by hand: "a b c" / "a x c" 1 of 3, "d e" / "d e f" 1 of 2, "g" / "" 1 of 1 -> 3 errors over 6 words; 1 + 1 + 1 of 3 + 2 + 1 characters
    three = (["a b c", "d e", "g"], ["a x c", "d e f", ""])
    assert d.error_rate(*three) == 3 / 6 and d.error_rate(*three, unit="char") == 3 / 6
    assert d.error_rate(["a b c d", "e"], ["a b", "e"]) == 2 / 5
    with pytest.raises(ValueError, match="no token"):
        d.error_rate(["", "  "], ["a", "b"])
    with pytest.raises(ValueError, match="4097"):
        d.cer_batch(["a" * 4097], ["a"])
    with pytest.raises(ValueError):
        d.error_counts(["a"], ["a", "b"])
    with pytest.raises(ValueError):
        d.error_counts(["a"], ["a"], unit="syllable")
    assert d.wer_batch([], []) == []


def test_min_risk_known_answer():
    from danspeech_amd.deepspeech.decoder import BeamCTCDecoder
    d = BeamCTCDecoder(LABELS, beam_width=4, blank_index=0)
    ids = [d.transcript_ids(t) for t in ("a b c", "a b d", "a x d")]
    logp = np.log([0.4, 0.3, 0.3]) - 50.0                    # (only their differences matter)
    (order, risks), = d.min_risk([ids], [list(logp)])
    np.testing.assert_allclose(risks, [0.9, 0.7, 1.1], rtol=1e-12)
    assert order.tolist() == [1, 0, 2]                       # the second wins although the first is the most probable
    (order, risks), = d.min_risk([ids], [list(logp)], unit="char")
    np.testing.assert_allclose(risks, [0.9, 0.7, 1.1], rtol=1e-12)
    # all None: uniform; one hypothesis; a None among posteriors weighs 0; ties keep the decoder's order; clips of different sizes
    out = d.min_risk([ids, ids[:1], ids, [ids[0], ids[0], ids[1]], []], [[None] * 3, [-3.0], [logp[0], None, logp[2]], [-1.0, -1.0, -1.0], []])
    np.testing.assert_allclose(out[0][1], [1.0, 2 / 3, 1.0], rtol=1e-12)
    assert out[0][0].tolist() == [1, 0, 2]
    assert out[1][0].tolist() == [0] and out[1][1].tolist() == [0.0]
    np.testing.assert_allclose(out[2][1], [2 * 3 / 7, 4 / 7 + 3 / 7, 2 * 4 / 7], rtol=1e-12)
    assert out[3][0].tolist() == [0, 1, 2] and out[3][1][0] == out[3][1][1]
    assert len(out[4][0]) == 0 and len(out[4][1]) == 0
    # words: runs of spaces and leading / trailing spaces hold no word
    sp = d.space_index
    a = d.transcript_ids("hej du")
    padded = np.concatenate([[sp, sp], a[:3], [sp, sp], a[4:], [sp]])
    (order, risks), = d.min_risk([[a, padded]], [[-1.0, -2.0]])
    assert risks.tolist() == [0.0, 0.0]
    (order, risks), = d.min_risk([[a, padded]], [[-1.0, -2.0]], unit="char")
    assert risks.tolist() == [0.0, 0.0]
    with pytest.raises(ValueError):
        d.min_risk([ids], [[-1.0]])


def test_decode_min_risk_reorders_decode_scored():
    from danspeech_amd.deepspeech.decoder import BeamCTCDecoder, GreedyDecoder
    rng = np.random.default_rng(71)
    frames = [64, 40, 17]
    probs = [sref.peaky(rng, T, C33, sharp=2.0) for T in frames]
    T = max(frames)
    x = np.full((3, T, C33), 1.0 / C33, dtype=np.float32)
    for b, p in enumerate(probs):
        x[b, :len(p)] = p
    p_dev, sizes = torch.from_numpy(x).cuda(), np.array(frames, dtype=np.int32)
    beam = BeamCTCDecoder(LABELS, beam_width=16, blank_index=0)
    strings, offsets, logps = beam.decode_scored(p_dev, sizes)
    for unit in ("word", "char"):
        s2, o2, risks, l2 = beam.decode_min_risk(p_dev, sizes, unit=unit)
        for b in range(3):
            K = len(strings[b])
            assert K == 16 and len(s2[b]) == K
            toks = [s.split() if unit == "word" else list(s.replace(" ", "")) for s in strings[b]]
            table = {}
            toks = [[table.setdefault(t, len(table)) for t in row] for row in toks]
            D = np.zeros((K, K))
            for i in range(K):
                for j in range(i + 1, K):
                    D[i, j] = D[j, i] = ref.tuple_dp(toks[i], toks[j])[0]
            lp = np.array([-np.inf if v is None else v for v in logps[b]])
            w = np.exp(lp - lp.max())
            w /= w.sum()
            want = (D * w[None, :]).sum(axis=1)
            order = np.argsort(want, kind="stable")
            np.testing.assert_allclose(risks[b], want[order], rtol=1e-12, atol=0)
            assert np.argsort(np.array(risks[b]), kind="stable").tolist() == list(range(K))      # its order is the stable sort of its own risks
            assert s2[b] == [strings[b][i] for i in order] and l2[b] == [logps[b][i] for i in order]
            assert all((o2[b][q] == offsets[b][i]).all() for q, i in enumerate(order))
    greedy = GreedyDecoder(LABELS, blank_index=0)
    gs, go, gr, gl = greedy.decode_min_risk(p_dev, sizes)
    gs2, _, gl2 = greedy.decode_scored(p_dev, sizes)
    assert gs == gs2 and gl == gl2 and gr == [[0.0]] * 3


# ---- end to end: a synthetic cfgA-shaped model (2 conv, 5 x BiGRU 800) with sharpened FC weights, as tests/test_gpu_score.py
def test_recognize_min_risk_and_evaluate_end_to_end():
    from danspeech_amd import Recognizer
    from danspeech_amd.deepspeech.model import DeepSpeech
    sd = syn.make_state_dict(2, "gru", 800, 5, seed=0, fc_gain=8.0)
    model = DeepSpeech("cfgA", rnn_type="gru", rnn_hidden_size=800, rnn_layers=5, conv_layers=2).load_state_dict(sd)
    rec = Recognizer(model=model)
    clips = [syn.make_clip(i, n) for i, n in enumerate([48000, 96000, 32000])]
    texts = rec.recognize_batch(clips)
    transcripts = [texts[0], "  Hej   MED dig ", texts[2][:len(texts[2]) // 2]]
    ev = rec.evaluate(clips, transcripts)
    assert len(ev["texts"]) == 3 and all(isinstance(t, str) for t in ev["texts"])
    norm = [" ".join(t.lower().split()) for t in transcripts]
    for unit, name in (("word", "wer"), ("char", "cer")):
        split = (lambda s: s.split()) if unit == "word" else (lambda s: list(s.replace(" ", "")))
        want = np.array([ref.tuple_dp(split(r), split(h)) for r, h in zip(norm, ev["texts"])], dtype=np.int32)
        np.testing.assert_array_equal(ev[unit + "_counts"], want)
        assert ev[unit + "_ref_lens"].tolist() == [len(split(r)) for r in norm]
        assert ev[name] == want[:, 0].sum() / sum(len(split(r)) for r in norm)
    ranked = rec.recognize_min_risk(clips, n_best=4)
    assert len(ranked) == 3
    for row in ranked:
        assert 1 <= len(row) <= 4 and all(isinstance(t, str) and r >= 0.0 for t, r, _ in row)
        assert [r for _, r, _ in row] == sorted(r for _, r, _ in row) and (len(row) > 1 or row[0][1] == 0.0)
    assert rec.recognize_min_risk([]) == [] and rec.evaluate([], [])["texts"] == []
    with pytest.raises(ValueError):
        rec.evaluate(clips, transcripts[:1])
