"""What the LM sentence scoring tests share (tests/test_lm_score_host.py, tests/test_gpu_lm_score.py): synthetic ARPA models with
oracle/lm.py's ``Scorer`` over them, a sentence sampler that follows the model's own n-grams (so that windows resolve at every
order, which sentences of independent words never do), the oracle's terms, and the coverage counts the tests assert."""
import numpy as np

from danspeech_amd import synthetic as syn
from oracle import lm as olm

LABELS = syn.DANSPEECH_LABELS
SPACE = LABELS.index(" ")
SPECIAL = (olm.START_TOKEN, olm.END_TOKEN, olm.UNK_TOKEN)


def make_model(directory, order, n_words=300, seed=13, ngrams_per_order=900):
    """(path of the ARPA file, oracle Scorer over it)"""
    path = str(directory / ("lm%d_%d_%d.arpa" % (order, n_words, seed)))
    syn.make_arpa(path, order=order, n_words=n_words, seed=seed, ngrams_per_order=ngrams_per_order)
    return path, olm.Scorer(0.0, 0.0, path, LABELS)


def oov_word(rng, vocab_set):
    letters = [c for c in LABELS if c not in "_ "]
    while True:
        w = "".join(rng.choice(letters, size=int(rng.integers(1, 9))))
        if w not in vocab_set:
            return w


def sample_sentences(scorer, rng, count, max_words=12, oov_every=10):
    """``count`` sentences (lists of word strings) of 0 .. max_words words: chunks that are a random vocabulary word or the
    words of a random n-gram of the model, then one word in ``oov_every`` replaced by a string outside the vocabulary."""
    vocab = [w for w in scorer.lm.vocab if w not in SPECIAL]
    grams = {}                # by order, so that the few n-grams of the highest orders are met as often as the many bigrams
    for g in scorer.lm.ngrams:
        if len(g) > 1 and not any(w in SPECIAL for w in g):
            grams.setdefault(len(g), []).append(g)
    orders = sorted(grams)
    out = []
    for _ in range(count):
        n = int(rng.integers(0, max_words + 1))
        words = []
        while len(words) < n:
            if rng.random() < 0.3:
                words.append(vocab[int(rng.integers(0, len(vocab)))])
            else:
                of = grams[orders[int(rng.integers(0, len(orders)))]]
                words.extend(of[int(rng.integers(0, len(of)))])
        words = words[:n]
        out.append([oov_word(rng, scorer.lm.vocab_set) if rng.integers(0, oov_every) == 0 else w for w in words])
    return out


def windows(scorer, words):
    k = scorer.max_order
    s = [olm.START_TOKEN] * (k if not words else k - 1) + list(words) + [olm.END_TOKEN]
    return [s[i:i + k] for i in range(len(s) - k + 1)]


def oracle(scorer, words):
    """(Scorer.get_sent_log_prob, its terms one by one through get_log_cond_prob)"""
    return scorer.get_sent_log_prob(list(words)), [scorer.get_log_cond_prob(w) for w in windows(scorer, words)]


def coverage(scorer, sentences):
    """({order: windows whose longest n-gram in the model has that order}, windows at the OOV score)"""
    by_order, oov = {k: 0 for k in range(1, scorer.max_order + 1)}, 0
    for words in sentences:
        for w in windows(scorer, words):
            if any(x not in scorer.lm.vocab_set or x == olm.UNK_TOKEN for x in w):
                oov += 1
                continue
            by_order[max(k for k in range(1, len(w) + 1) if tuple(w[-k:]) in scorer.lm.ngrams)] += 1
    return by_order, oov


def assert_coverage(scorer, sentences, least=50):
    by_order, oov = coverage(scorer, sentences)
    assert all(v >= least for v in by_order.values()) and oov >= least, (by_order, oov)


def label_ids(text):
    return np.array([LABELS.index(c) for c in text], dtype=np.int32)
