"""LM sentence scoring on the GPU (dsmi_lm_score, csrc/lmscore.hip) against oracle/lm.py's ``Scorer`` and against
``dsmi_lm_sentence_ln``: sum, every term and the counts, bit for bit -- on sentences shown to resolve windows at every order and
at the OOV score, crafted rows (dictionary edges, empty rows, a row that loops its workgroup, the longest row), orders 2, 4 and 6,
the three table kinds, batch invariance with live garbage behind every length, a model swap, capacity growth, every refusal, and
the Python surface up to ``rescore``, ``decode_rescored`` and ``tune_lm_weights``.  Every comparison is exact."""
import numpy as np
import pytest

from oracle import klm

import _lm_score_ref as ref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
LABELS = ref.LABELS
SENTINEL = -77


@pytest.fixture(scope="module")
def native():
    from danspeech_amd import _native
    return _native


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp("lm_score")
    out = {3: ref.make_model(d, 3), "other": ref.make_model(d, 3, seed=29)}
    for order in (2, 4, 6):
        out[order] = ref.make_model(d, order, n_words=8)         # (few words: the higher orders need a dense model to exist)
    for kind, name in ((klm.PROBING, "probing"), (klm.TRIE, "trie")):
        out[name] = str(d / (name + ".klm"))
        klm.write_klm(out[3][0], out[name], kind)
    return out


@pytest.fixture(scope="module")
def dec(native, models):
    d = native.NativeDecoder(LABELS, blank_index=0)
    d.set_lm(models[3][0], 0.0, 0.0)
    yield d
    d.close()


def _spaced(rng, words):
    """The words with one or two spaces between them and sometimes spaces in front and behind."""
    text = "".join(w + " " * int(rng.integers(1, 3)) for w in words).rstrip(" ") if words else ""
    return " " * int(rng.integers(0, 3) == 0) + text + " " * int(rng.integers(0, 3) == 0)


def _want(scorer, texts):
    """What the oracle says of texts: (lm_ln, n_words, n_oov, terms)"""
    lm_ln, n_words, n_oov, terms = [], [], [], []
    for t in texts:
        words = [w for w in t.split(" ") if w]
        total, tm = ref.oracle(scorer, words)
        lm_ln.append(total); terms.append(tm); n_words.append(len(words)); n_oov.append(sum(w not in scorer.lm.vocab_set for w in words))
    return lm_ln, n_words, n_oov, terms


def _check(dec, scorer, texts, host_lm=None):
    ids = [ref.label_ids(t) for t in texts]
    lm_ln, n_words, n_oov, terms = dec.lm_score(ids, want_terms=True)
    w_ln, w_words, w_oov, w_terms = _want(scorer, texts)
    assert n_words.tolist() == w_words and n_oov.tolist() == w_oov
    assert [len(t) for t in terms] == [n + 1 if n else 2 for n in w_words]
    bad = [m for m in range(len(texts)) if terms[m].tolist() != w_terms[m] or lm_ln[m] != w_ln[m]]
    assert not bad, [(texts[m][:60], lm_ln[m], w_ln[m]) for m in bad[:5]]
    if host_lm is not None:
        for m, t in enumerate(texts):
            total, tm = host_lm.sentence_ln([host_lm.word_index(w) for w in t.split(" ") if w])
            assert total == lm_ln[m] and tm.tolist() == terms[m].tolist()
    plain = dec.lm_score(ids)
    assert plain[0].tobytes() == lm_ln.tobytes() and plain[1].tolist() == w_words and plain[2].tolist() == w_oov
    return lm_ln, n_words, n_oov, terms


def _sentences(scorer, seed, count):
    rng = np.random.default_rng(seed)
    sentences = ref.sample_sentences(scorer, rng, count)
    return sentences, [_spaced(rng, s) for s in sentences]


def test_values_against_the_oracle(dec, native, models):
    path, scorer = models[3]
    sentences, texts = _sentences(scorer, 7, 200)
    ref.assert_coverage(scorer, sentences)
    vocab = [w for w in scorer.lm.vocab if w not in ref.SPECIAL]
    vs = scorer.lm.vocab_set
    prefix = next(w[:k] for w in vocab for k in range(1, len(w)) if w[:k] not in vs)           # on the trie's path, no word ends there
    longer = next(w + c for w in vocab for c in "abc" if w + c not in vs)                      # a word, then one more letter
    one = next(w for w in vocab if len(w) == 1)
    rng = np.random.default_rng(8)
    row300 = " ".join(vocab[int(i)] for i in rng.integers(0, len(vocab), 300))
    long = ""
    while len(long) < native.LM_SCORE_MAX_TOKENS:
        long += vocab[int(rng.integers(0, len(vocab)))] + " "
    long = long[:native.LM_SCORE_MAX_TOKENS]
    crafted = [prefix, "%s %s" % (vocab[3], prefix), longer, "%s %s %s" % (longer, vocab[5], vocab[6]), one, " %s  %s " % (one, one), "", "   ",
               row300, long]
    assert len(long) == 4096 and len(row300.split()) == 300
    host = native.NativeLM(path)
    got = _check(dec, scorer, texts + crafted, host)
    host.close()
    n = len(texts)
    assert got[2][n:n + 4].tolist() == [1, 1, 1, 1] and got[2][n + 4:n + 8].tolist() == [0, 0, 0, 0]
    assert got[1][n + 6:n + 8].tolist() == [0, 0] and len(got[3][n + 6]) == 2 and got[0][n + 6] == got[0][n + 7] == scorer.get_sent_log_prob([])


@pytest.mark.parametrize("order", [2, 4, 6])
def test_orders(native, models, order):
    path, scorer = models[order]
    assert scorer.max_order == order
    d = native.NativeDecoder(LABELS, blank_index=0)
    d.set_lm(path, 0.0, 0.0)
    sentences, texts = _sentences(scorer, 30 + order, 40)
    by_order, oov = ref.coverage(scorer, sentences)
    assert by_order[order] > 0 and oov > 0
    host = native.NativeLM(path)
    _check(d, scorer, texts + ["", " "], host)
    host.close()
    d.close()


def test_table_kinds_give_the_same_bytes(dec, native, models):
    scorer = models[3][1]
    _, texts = _sentences(scorer, 11, 120)
    ids = [ref.label_ids(t) for t in texts]
    want = dec.lm_score(ids, want_terms=True)
    for name, kind in (("probing", "klm-probing"), ("trie", "klm-trie")):
        host = native.NativeLM(models[name])
        assert host.kind == kind
        host.close()
        d = native.NativeDecoder(LABELS, blank_index=0)
        d.set_lm(models[name], 0.0, 0.0)
        got = d.lm_score(ids, want_terms=True)
        d.close()
        assert got[0].tobytes() == want[0].tobytes() and got[1].tolist() == want[1].tolist() and got[2].tolist() == want[2].tolist()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[3], want[3]))


def test_batch_invariance(dec, models):
    scorer = models[3][1]
    sentences, texts = _sentences(scorer, 13, 200)
    rng = np.random.default_rng(14)
    vocab = [w for w in scorer.lm.vocab if w not in ref.SPECIAL]
    lens = np.array([len(t) for t in texts], dtype=np.int32)
    Ls = int(lens.max()) + 12
    pool = np.zeros((len(texts), Ls), dtype=np.int32)
    for m, t in enumerate(texts):                              # behind its length every row goes on with vocabulary words
        tail = t
        while len(tail) < Ls:
            tail += vocab[int(rng.integers(0, len(vocab)))] + " "
        pool[m] = ref.label_ids(tail[:Ls])
    together = dec.lm_score(pool, lens, want_terms=True)
    plain = dec.lm_score(pool, lens)
    w_ln, w_words, w_oov, w_terms = _want(scorer, texts)
    assert together[0].tolist() == w_ln and together[1].tolist() == w_words and together[2].tolist() == w_oov
    assert plain[0].tobytes() == together[0].tobytes() and plain[2].tolist() == w_oov
    for m in range(len(texts)):
        alone = dec.lm_score(pool[m:m + 1], lens[m:m + 1], want_terms=True)
        assert alone[0].tobytes() == together[0][m:m + 1].tobytes() and alone[3][0].tobytes() == together[3][m].tobytes()
        assert alone[1][0] == together[1][m] and alone[2][0] == together[2][m]
        assert dec.lm_score(pool[m:m + 1], lens[m:m + 1])[0].tobytes() == alone[0].tobytes()


def test_model_swap(native, models):
    d = native.NativeDecoder(LABELS, blank_index=0)
    (path_a, scorer_a), (path_b, scorer_b) = models[3], models["other"]
    _, texts = _sentences(scorer_a, 17, 30)
    _, more = _sentences(scorer_b, 18, 30)
    d.set_lm(path_a, 0.0, 0.0)
    first = _check(d, scorer_a, texts + more)
    d.set_lm(path_b, 0.3, 0.1)
    second = _check(d, scorer_b, texts + more)
    assert first[0].tolist() != second[0].tolist()
    d.close()


def test_growth(dec, models):
    scorer = models[3][1]
    _, small = _sentences(scorer, 19, 4)
    first = _check(dec, scorer, small)
    sentences, texts = _sentences(scorer, 20, 256)
    big = [texts[k % 256] for k in range(4096)]
    got = dec.lm_score([ref.label_ids(t) for t in big], want_terms=True)
    w_ln, w_words, w_oov, w_terms = _want(scorer, texts)
    assert got[0].tolist() == [w_ln[k % 256] for k in range(4096)] and got[2].tolist() == [w_oov[k % 256] for k in range(4096)]
    assert all(got[3][k].tolist() == w_terms[k % 256] for k in range(4096))
    again = _check(dec, scorer, small)
    assert again[0].tobytes() == first[0].tobytes()


def test_refusals_write_nothing(native, models):
    path, scorer = models[3]
    d = native.NativeDecoder(LABELS, blank_index=0)
    L = native.lib()
    a_word = next(w for w in scorer.lm.vocab if w not in ref.SPECIAL and len(w) == 3)
    row = ref.label_ids(a_word + " " + a_word).tolist()             # 7 tokens, 2 words, 3 terms
    ok = dict(M=3, Ls=7, W=3, seqs=[row, row[:3] + [0] * 4, [0] * 7], lens=[7, 3, 0])

    def call(null=(), **kw):
        a = dict(ok, **kw)
        out = dict(lm_ln=np.full(3, float(SENTINEL)), n_words=np.full(3, SENTINEL, dtype=np.int32), n_oov=np.full(3, SENTINEL, dtype=np.int32),
                   n_terms=np.full(3, SENTINEL, dtype=np.int32), terms=np.full((3, 3), float(SENTINEL)))
        arr = {k: np.ascontiguousarray(a[k], dtype=np.int32) for k in ("seqs", "lens")}
        ptr = {k: None if k in null else native._np_ptr(v) for k, v in list(arr.items()) + list(out.items())}
        rc = L.dsmi_lm_score(d._h, ptr["seqs"], ptr["lens"], a["M"], a["Ls"], ptr["lm_ln"], ptr["n_words"], ptr["n_oov"], ptr["n_terms"],
                             ptr["terms"], a["W"], None)
        return rc, all((v == SENTINEL).all() for v in out.values()), L.dsmi_decoder_last_error(d._h).decode(), out

    rc, untouched, msg, _ = call()                               # no language model yet
    assert rc == native.DSMI_ERR_INVALID and untouched and "language model" in msg
    with pytest.raises(native.DsmiError, match="language model"):
        d.lm_score([row])
    d.set_lm(path, 0.0, 0.0)

    def good():
        rc, _, _, out = call()
        want = _want(scorer, [a_word + " " + a_word, a_word, ""])
        assert rc == 0 and out["lm_ln"].tolist() == want[0] and out["n_words"].tolist() == [2, 1, 0] and out["n_oov"].tolist() == [0, 0, 0]
        assert out["n_terms"].tolist() == [3, 2, 2] and out["terms"][0].tolist() == want[3][0]
        assert out["terms"][1].tolist() == want[3][1] + [SENTINEL] and out["terms"][2].tolist() == want[3][2] + [SENTINEL]

    good()
    blank_in = [row[:2] + [0] + row[3:], row[:3] + [0] * 4, [0] * 7]
    invalid = (dict(M=0), dict(M=-2), dict(Ls=-1), dict(lens=[8, 3, 0]), dict(lens=[7, -1, 0]), dict(seqs=blank_in),
               dict(seqs=[row[:6] + [len(LABELS)], row, row]), dict(seqs=[[-1] + row[1:], row, row]), dict(null=("seqs",)), dict(null=("lens",)),
               dict(null=("lm_ln",)), dict(null=("n_words",)), dict(null=("n_oov",)), dict(null=("n_terms",)))
    for kw in invalid:
        rc, untouched, msg, _ = call(**kw)
        assert rc == native.DSMI_ERR_INVALID and untouched and msg, (kw, rc, msg)
    # on the numbers alone: the arrays are far smaller than the call declares and must not be read
    rc, untouched, msg, _ = call(Ls=native.LM_SCORE_MAX_TOKENS + 1)
    assert rc == native.DSMI_ERR_CAPACITY and untouched and "DSMI_LM_SCORE_MAX_TOKENS" in msg
    rc, untouched, msg, _ = call(M=(1 << 24) // 4096 + 1, Ls=4096)
    assert rc == native.DSMI_ERR_CAPACITY and untouched and "M * L_stride" in msg
    for W in (2, 0, -1):
        rc, untouched, msg, _ = call(W=W)
        assert rc == native.DSMI_ERR_CAPACITY and untouched and "n_terms" in msg
    rc, _, _, out = call(null=("terms",), W=-5)                  # no terms wanted: W_stride is ignored
    assert rc == 0 and out["n_terms"].tolist() == [3, 2, 2] and (out["terms"] == SENTINEL).all()
    rc, _, _, out = call(null=("seqs",), Ls=0, lens=[0, 0, 0])   # no columns: no pool needed
    assert rc == 0 and out["n_words"].tolist() == [0, 0, 0] and out["lm_ln"].tolist() == [scorer.get_sent_log_prob([])] * 3
    # garbage behind the lengths (the blank, ids out of range) is no token
    rc, _, _, out = call(seqs=[row, row[:3] + [0, -5, 99, 0], [0, 99, -1, 0, 0, 0, 0]])
    assert rc == 0 and out["n_words"].tolist() == [2, 1, 0]
    good()
    d.close()


# ---- the decoders' surface
def _beam(models, **kw):
    from danspeech_amd.deepspeech.decoder import BeamCTCDecoder
    return BeamCTCDecoder(LABELS, lm_path=models[3][0], blank_index=0, **kw)


def _spell(rng, text, sharp, T=None):
    """Probabilities [T, C] that spell ``text`` (two frames per label, a blank between equal neighbours) under noise."""
    path = []
    for k, c in enumerate(text):
        if k and text[k - 1] == c:
            path.append(0)
        path += [LABELS.index(c)] * 2
    path += [0] * ((T or len(path)) - len(path))
    z = rng.normal(size=(len(path), len(LABELS)))
    z[np.arange(len(path)), path] += sharp
    p = np.exp(z - z.max(1, keepdims=True))
    return (p / p.sum(1, keepdims=True)).astype(np.float32)


def test_lm_score_of_texts_and_rescore(models):
    scorer = models[3][1]
    d = _beam(models, alpha=0.7, beta=0.25, beam_width=8)
    _, texts = _sentences(scorer, 41, 24)
    got = d.lm_score(["  " + t.upper() + " " for t in texts], terms=True)
    ids = [ref.label_ids(" ".join(t.split())) for t in texts]
    same = d.lm_score_ids(ids, terms=True)
    w_ln, w_words, w_oov, w_terms = _want(scorer, texts)
    for a, b in zip(got[:3], same[:3]):
        assert a.tobytes() == b.tobytes()
    assert got[0].tolist() == w_ln and got[1].tolist() == w_words and got[2].tolist() == w_oov and [t.tolist() for t in got[3]] == w_terms
    assert d.lm_score([])[0].shape == (0,)
    with pytest.raises(ValueError):
        d.lm_score(["not a label: #"])
    # rescore: three clips of 8, 8 and 1 hypotheses, and one with none; a None among the scores
    rng = np.random.default_rng(42)
    lists = [ids[:8], ids[8:16], ids[16:17], []]
    logps = [list(rng.uniform(-60, -20, 8)), list(rng.uniform(-60, -20, 8)), [-3.5], []]
    logps[1][2] = None
    for eos in (True, False):
        for alpha, beta in ((None, None), (0.0, 0.0), (2.5, -0.5)):
            out = d.rescore(lists, logps, alpha, beta, eos=eos)
            a, bt = (0.7, 0.25) if alpha is None else (alpha, beta)
            at = 0
            for (order, totals), hyps, lps in zip(out, lists, logps):
                K = len(hyps)
                lm = np.array([w_ln[at + k] - (0.0 if eos else w_terms[at + k][-1]) for k in range(K)])
                lp = np.array([-np.inf if v is None else v for v in lps], dtype=np.float64)
                want = lp + a * lm + bt * np.array(w_words[at:at + K], dtype=np.float64)
                assert totals.dtype == np.float64 and totals.tolist() == want.tolist()
                assert order.tolist() == np.argsort(-want, kind="stable").tolist()
                at += K
    # a crafted tie: equal hypotheses with equal scores, and different ones at alpha = beta = 0, keep the incoming order
    (order, totals), = d.rescore([[ids[0], ids[1], ids[0], ids[1]]], [[-9.0, -5.0, -9.0, -5.0]], 0.0, 0.0)
    assert order.tolist() == [1, 3, 0, 2] and totals.tolist() == [-9.0, -5.0, -9.0, -5.0]
    (order, totals), = d.rescore([[ids[0], ids[1], ids[0]]], [[-9.0, -5.0, -9.0]])
    assert totals[0] == totals[2] and order.tolist().index(0) < order.tolist().index(2)
    # the totals are valid posteriors for min_risk
    (mr_order, risks), = d.min_risk([lists[0]], [list(d.rescore([lists[0]], [logps[0]])[0][1])])
    assert len(mr_order) == 8 and (risks >= 0).all()
    with pytest.raises(ValueError):
        d.rescore(lists, logps[:2])
    from danspeech_amd import _native
    from danspeech_amd.deepspeech.decoder import BeamCTCDecoder
    with pytest.raises(_native.DsmiError, match="language model"):
        BeamCTCDecoder(LABELS, blank_index=0).lm_score(["hej"])


@pytest.fixture(scope="module")
def clips(models):
    scorer = models[3][1]
    rng = np.random.default_rng(51)
    sentences = [s for s in ref.sample_sentences(scorer, rng, 40, max_words=5, oov_every=6) if 2 <= len(s) <= 5][:4]
    refs = [" ".join(s) for s in sentences]
    frames = [2 * len(r) + 6 + sum(a == b for a, b in zip(r, r[1:])) for r in refs]
    T = max(frames)
    x = np.stack([_spell(rng, r, 4.5, T) for r in refs])
    return refs, torch.from_numpy(x).cuda(), np.array(frames, dtype=np.int32)


def test_decode_rescored_reorders_decode_scored(models, clips):
    refs, probs, sizes = clips
    d = _beam(models, alpha=0.6, beta=0.2, beam_width=8)
    strings, offsets, logps = d.decode_scored(probs, sizes, 6)
    s2, o2, totals, l2 = d.decode_rescored(probs, sizes, 6)
    scorer = models[3][1]
    for b in range(len(refs)):
        assert sorted(s2[b]) == sorted(strings[b]) and len(s2[b]) == 6
        w_ln, w_words, _, _ = _want(scorer, strings[b])
        want = np.array([lp + 0.6 * lm + 0.2 * float(n) for lp, lm, n in zip(logps[b], w_ln, w_words)])
        order = np.argsort(-want, kind="stable")
        assert totals[b] == want[order].tolist() and s2[b] == [strings[b][i] for i in order] and l2[b] == [logps[b][i] for i in order]
        assert all((o2[b][q] == offsets[b][i]).all() for q, i in enumerate(order))
    s3, _, t3, _ = d.decode_rescored(probs, sizes, 6, alpha=0.0, beta=0.0)      # the acoustic scores alone
    assert all(t3[b] == sorted(logps[b], reverse=True) for b in range(len(refs)))


def test_tune_lm_weights_is_the_loop_over_the_grid(models, clips):
    refs, probs, sizes = clips
    scorer = models[3][1]
    d = _beam(models, alpha=0.6, beta=0.2, beam_width=8)
    alphas, betas = [0.0, 0.0, 1.5], [0.0, 0.8]                 # (two equal alphas: their grid points tie, the lower index wins)
    for unit, eos in (("word", True), ("char", False)):
        got = d.tune_lm_weights(probs, sizes, [" " + r.upper() for r in refs], alphas, betas, n_best=4, unit=unit, eos=eos)
        strings, _, logps = d.decode_scored(probs, sizes, 4)
        errors = np.zeros((3, 2), dtype=np.int64)
        for i, a in enumerate(alphas):
            for j, bt in enumerate(betas):
                for b, r in enumerate(refs):
                    w_ln, w_words, _, w_terms = _want(scorer, strings[b])
                    totals = [lp + a * (lm - (0.0 if eos else tm[-1])) + bt * float(n) for lp, lm, tm, n in zip(logps[b], w_ln, w_terms, w_words)]
                    pick = strings[b][totals.index(max(totals))]
                    errors[i, j] += d.wer(r, pick) if unit == "word" else d.cer(r, pick)
        total_ref = sum(len(r.split()) if unit == "word" else len(r.replace(" ", "")) for r in refs)
        assert got["errors"].tolist() == errors.tolist() and (got["ref_tokens"] == total_ref).all() and got["ref_tokens"].shape == (3, 2)
        flat = [(errors[i, j], i, j) for i in range(3) for j in range(2)]
        _, bi, bj = min(flat)
        assert got["best_index"] == (bi, bj) and got["best"] == (alphas[bi], betas[bj]) and got["error_rate"] == errors[bi, bj] / total_ref
        assert (errors[0] == errors[1]).all() and bi != 1
    # one grid point made to tie inside a clip: with a stubbed search, two hypotheses of equal score at alpha = beta = 0 -- the
    # first is taken, which is the wrong one here; any beta > 0 prefers the second (more words)
    word = refs[0].split()[0]
    hyps = [word, word + " " + word]
    stub = lambda probs, sizes, n_best: ([hyps], [[None, None]], [[-4.0, -4.0]], [[ref.label_ids(h) for h in hyps]])
    d._decode_scored_ids = stub
    got = d.tune_lm_weights(probs[:1], sizes[:1], [hyps[1]], [0.0], [0.0, 1.0], n_best=2)
    assert got["errors"].tolist() == [[1, 0]] and got["best_index"] == (0, 1) and got["ref_tokens"].tolist() == [[2, 2]]
