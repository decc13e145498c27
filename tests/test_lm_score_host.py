"""LM sentence scoring off the GPU: ``dsmi_lm_score_plan``'s word segmentation against Python's ``split``, its refusals,
``dsmi_lm_sentence_ln`` against oracle/lm.py's ``Scorer`` bit for bit (sum and every term) at orders 2, 3 and 4 on sentences shown
to resolve windows at every order and at the OOV score, and the host half of ``dsmi_lm_score`` (csrc/lm_score_host.h) under
ASan + UBSan in the stand-alone harness (tools/asan/host_fuzz.cpp lmscore).  No kernel runs."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _lm_score_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "danspeech_amd", "csrc", "build", "host_fuzz_asan")
ALPHABET = "ab c"            # token ids 0 .. 3; 2 is the space


@pytest.fixture(scope="module")
def native():
    from danspeech_amd import _native
    return _native


def _plan_rows(native, texts, width, rng):
    """Rows of ``width`` tokens holding ``texts`` and, behind each length, garbage that would spell further words."""
    pool = rng.integers(0, len(ALPHABET), (len(texts), width)).astype(np.int32)
    lens = np.array([len(t) for t in texts], dtype=np.int32)
    for m, t in enumerate(texts):
        pool[m, :len(t)] = [ALPHABET.index(c) for c in t]
    n_words, first, length = native.lm_score_plan(pool, lens, space=ALPHABET.index(" "))
    for m, t in enumerate(texts):
        want = [w for w in t.split(" ") if w]
        got = ["".join(ALPHABET[i] for i in pool[m, first[m, k]:first[m, k] + length[m, k]]) for k in range(n_words[m])]
        assert got == want, (t, got)
    assert first.shape[1] == max(len([w for w in t.split(" ") if w]) for t in texts)


def test_plan_is_pythons_split(native):
    rng = np.random.default_rng(41)
    crafted = ["", " ", "   ", " a", "a ", "a  b", "  ab  ca ", "a", "b" * 24, "a b a b a b a b a b a b ", " " * 24, "abc"[:2] * 12]
    _plan_rows(native, crafted, 24, rng)
    for rep in range(40):
        width = int(rng.integers(1, 60))
        texts = ["".join(rng.choice(list(ALPHABET), size=int(rng.integers(0, width + 1)), p=[0.3, 0.25, 0.3, 0.15])) for _ in range(int(rng.integers(1, 30)))]
        _plan_rows(native, texts, width, rng)
    # no space among the labels: every non-empty row is one word
    n_words, first, length = native.lm_score_plan([[0, 2, 1], [], [2]], space=-2)
    assert n_words.tolist() == [1, 0, 1] and first[:, 0].tolist() == [0, 0, 0] and length[:, 0].tolist() == [3, 0, 1]
    n_words, first, length = native.lm_score_plan(np.zeros((3, 0), dtype=np.int32), np.zeros(3, dtype=np.int32))
    assert n_words.tolist() == [0, 0, 0] and first.shape == (3, 0)


def test_plan_refusals_write_nothing(native):
    L = native.lib()
    pool = np.array([[0, 2, 1, 2], [1, 1, 1, 1]], dtype=np.int32)           # "a b ", "bbbb"
    lens = np.array([4, 4], dtype=np.int32)

    def call(null=(), M=2, Ls=4, W=2, lens=lens):
        out = {k: np.full((2, 2), -77, dtype=np.int32) for k in ("n", "first", "len")}
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        ptr = dict(seqs=native._np_ptr(pool), lens=native._np_ptr(lens), **{k: native._np_ptr(v) for k, v in out.items()})
        ptr.update({k: None for k in null})
        rc = L.dsmi_lm_score_plan(ptr["seqs"], ptr["lens"], M, Ls, 2, ptr["n"], ptr["first"], ptr["len"], W)
        return rc, all((v == -77).all() for v in out.values()), out

    rc, _, out = call()
    assert rc == 2 and out["n"].reshape(-1)[:2].tolist() == [2, 1] and out["first"].tolist() == [[0, 2], [0, -77]] and out["len"].tolist() == [[1, 1], [4, -77]]
    for kw in (dict(null=("seqs",)), dict(null=("lens",)), dict(null=("n",)), dict(null=("first",)), dict(null=("len",)), dict(M=0), dict(M=-3),
               dict(Ls=-1), dict(W=-1), dict(lens=[5, 4]), dict(lens=[4, -1]), dict(W=1)):
        rc, untouched, _ = call(**kw)
        assert rc < 0 and untouched, kw
    with pytest.raises(native.DsmiError):
        native.lm_score_plan([[0, 1]], [3])


@pytest.mark.parametrize("order", [2, 3, 4])
def test_sentence_ln_is_the_oracles(native, tmp_path, order):
    path, scorer = ref.make_model(tmp_path, order)
    rng = np.random.default_rng(100 + order)
    sentences = ref.sample_sentences(scorer, rng, 300) + [[]]
    ref.assert_coverage(scorer, sentences)
    assert any(len(s) == 12 for s in sentences) and sum(len(s) == 0 for s in sentences) >= 2
    lm = native.NativeLM(path)
    assert lm.order == order
    for words in sentences:
        ids = [lm.word_index(w) for w in words]
        assert all((i >= 0) == (w in scorer.lm.vocab_set) for i, w in zip(ids, words))
        total, terms = lm.sentence_ln(ids)
        want_total, want_terms = ref.oracle(scorer, words)
        assert len(terms) == (len(words) + 1 if words else 2)
        assert terms.tolist() == want_terms, (words, terms.tolist(), want_terms)
        assert total == want_total, (words, total, want_total)
    # <unk> itself scores as an unknown word; ids outside the file's are out of vocabulary; the refusals
    assert lm.sentence_ln([lm.word_index("<unk>")])[1].tolist() == [-1000.0, -1000.0]
    assert lm.sentence_ln([lm.vocab_size + 5, -9])[0] == -3000.0
    L = native.lib()
    one, buf = np.zeros(1, dtype=np.int32), np.full(4, -77.0)
    assert np.isnan(L.dsmi_lm_sentence_ln(None, native._np_ptr(one), 1, None, 0))
    assert np.isnan(L.dsmi_lm_sentence_ln(lm._h, native._np_ptr(one), -1, None, 0))
    assert np.isnan(L.dsmi_lm_sentence_ln(lm._h, None, 1, None, 0))
    assert np.isnan(L.dsmi_lm_sentence_ln(lm._h, native._np_ptr(one), 1, native._np_ptr(buf), 1)) and (buf == -77.0).all()
    assert np.isnan(L.dsmi_lm_sentence_ln(lm._h, None, 0, native._np_ptr(buf), 1)) and (buf == -77.0).all()
    assert L.dsmi_lm_sentence_ln(lm._h, None, 0, None, 0) == scorer.get_sent_log_prob([])
    lm.close()


def test_lm_score_host_half_under_sanitizers():
    """csrc/lm_score_host.h -- the argument check (the refusals on the numbers alone with null arrays), the word segmentation,
    the packing of the upload and the unpacking of the results -- on random calls in exactly sized heap arrays, in the
    stand-alone CPU program built with -fsanitize=address,undefined.  A sanitizer report or a broken rule fails the test."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "danspeech_amd", "csrc"), "asan"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:allocator_may_return_null=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([EXE, "lmscore", "7", "400"], capture_output=True, text=True, timeout=600, env=env)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = r.stdout.split()
    assert out[:4] == ["400", "lmscore", "calls", "ok,"] and int(out[4]) > 50 and int(out[6]) > 3000, out
