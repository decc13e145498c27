"""The host side of CTC grammar decoding, without a GPU: the grammar compiler (danspeech_amd/grammar.py) against hand-written
sentence lists, the merge against the unmerged automaton, every ValueError; the numpy reference of the recurrence
(tests/_grammar_ref.py) against the alignment reference on chain graphs and against a brute force; dsmi_grammar_plan through
ctypes."""
import ctypes

import numpy as np
import pytest

import _align_ref as aref
import _grammar_ref as gref
from danspeech_amd import _native, synthetic as syn
from danspeech_amd.grammar import Grammar

LABELS = syn.DANSPEECH_LABELS

# (grammar, every sentence it accepts) or, for a grammar with a loop, (grammar, its first sentences, shortest first)
FINITE = [
    ("tænd lyset", ["tænd lyset"]),
    ("tænd | sluk", ["sluk", "tænd"]),
    ("(tænd | sluk) lyset", ["sluk lyset", "tænd lyset"]),
    ("tænd [lyset]", ["tænd", "tænd lyset"]),
    ("[nu] tænd", ["tænd", "nu tænd"]),                                     # an optional first word
    ("[ja | nej]", ["", "ja", "nej"]),                                      # a nullable main expression
    ("(a (b | c [d])) | e", ["e", "a b", "a c", "a c d"]),                  # nesting
    ("$v = tænd | sluk ; $r = stuen | køkkenet ; $v lyset [i $r]",
     ["sluk lyset", "tænd lyset", "sluk lyset i stuen", "tænd lyset i stuen", "sluk lyset i køkkenet", "tænd lyset i køkkenet"]),
    ("$d = en | to ; $d $d", ["en en", "en to", "to en", "to to"]),          # a rule used twice expands twice
    ("ja:-0.5 | nej:-1.5 tak", ["ja", "nej tak"]),                          # weights
    ("  Tænd\n LYSET ", ["tænd lyset"]),                                    # normalised as transcripts are
]
LOOPS = [
    ("a*", ["", "a", "a a", "a a a"]),
    ("a+", ["a", "a a", "a a a"]),
    ("(en | to)+ tak", ["en tak", "to tak", "en en tak", "en to tak", "to en tak", "to to tak"]),
    ("[ja] (a b)*", ["", "ja", "a b", "ja a b", "a b a b"]),
]


@pytest.mark.parametrize("text, want", FINITE)
def test_finite_grammars_accept_exactly_their_sentences(text, want):
    g = Grammar(text, LABELS)
    assert sorted(g.sentences()) == sorted(want)
    assert g.empty_ok == ("" in want)
    for s in want:
        assert g.accepts(s), s
    for s in want:
        for bad in (s + " x", "x " + s, s[:-1], s.replace(" ", "", 1) if " " in s else s + s):
            assert g.accepts(bad) == (" ".join(bad.split()) in want), bad      # (accepts normalises)


@pytest.mark.parametrize("text, first", LOOPS)
def test_loops_enumerate_shortest_first(text, first):
    g = Grammar(text, LABELS)
    got = g.sentences(len(first))
    assert got == first
    assert all(g.accepts(s) for s in got)


def test_weights_sit_on_the_first_character():
    g = Grammar("ja:-0.5 | nej:-1.5 tak", LABELS)
    by_char = {LABELS[g.labels[n]]: float(g.weights[n]) for n in range(g.n_nodes) if g.weights[n] != 0}
    assert by_char == {"j": -0.5, "n": -1.5}
    assert gref.accept(g, [LABELS.index(c) for c in "nej tak"]) == -1.5


def test_from_sentences():
    g = Grammar.from_sentences(["Hej  med dig", "hej du", ""], LABELS)
    assert g.sentences() == ["", "hej du", "hej med dig"]
    assert g.n_nodes == len("hej med dig") + len("du")                      # the common prefix is one trie branch
    with pytest.raises(ValueError, match="not a label"):
        Grammar.from_sentences(["hej 2"], LABELS)


@pytest.mark.parametrize("text", [t for t, _ in FINITE + LOOPS] + ["(a | a b | a b c)* [a]", "$w = ab | abc | b ; $w+ | $w c"])
def test_the_merge_keeps_the_language(text):
    merged, plain = Grammar(text, LABELS), Grammar(text, LABELS, _merge=False)
    assert merged.n_nodes <= plain.n_nodes
    assert merged.sentences(60) == plain.sentences(60)
    assert merged.empty_ok == plain.empty_ok


def test_a_word_loop_becomes_a_trie():
    words = syn.make_vocabulary(120)
    text = "(" + " | ".join(words) + ")+"
    g = Grammar(text, LABELS)
    assert g.n_nodes < 2048 and g.n_arcs < 8192
    assert Grammar(text, LABELS, _merge=False, _limits=False).n_arcs > 8192
    with pytest.raises(ValueError, match=r"\d+ arcs, more than the limit of 8192"):
        Grammar(text, LABELS, _merge=False)
    assert g.accepts(words[3] + " " + words[77] + " " + words[3]) and not g.accepts(words[3] + words[77] + "q")


def test_node_limit_names_the_count():
    words = syn.make_vocabulary(1200, seed=5)
    with pytest.raises(ValueError, match=r"\d+ nodes, more than the limit of 2048"):
        Grammar(" ".join(words), LABELS)


@pytest.mark.parametrize("text, message", [
    ("(a", "not closed"), ("[a", "not closed"), ("a )", "unexpected"), ("a |", "empty"), ("", "empty"), ("a:", "takes a number"),
    (":1 a", "follows a word"), ("$ a", "name must follow"), ("$x = a", "does not end"), ("$x = a ; $x = b ; $x", "defined twice"),
    ("a2", "not a label"), ("a_b", "not a label"), ("$x = a $y ; $y = $x ; $y", "recursive"), ("$x = $x ; a", None), ("a $nope", "not defined"),
    ("a:1e99", "not finite"),
])
def test_value_errors(text, message):
    if message is None:                  # (a recursive rule that is never used is never expanded)
        assert Grammar(text, LABELS).sentences() == ["a"]
        return
    with pytest.raises(ValueError, match=message):
        Grammar(text, LABELS)


def _random_probs(rng, T, C, uniform):
    if uniform:
        return np.full((T, C), 1.0 / C, dtype=np.float32)
    p = rng.random((T, C)).astype(np.float32) ** 3 + 1e-3
    return (p / p.sum(1, keepdims=True)).astype(np.float32)


def test_reference_on_chain_graphs_is_the_alignment_reference():
    rng = np.random.default_rng(5)
    done = 0
    while done < 200:
        T, C = int(rng.integers(1, 30)), 5
        L = int(rng.integers(0, min(T, 8) + 1))
        tg = [int(v) for v in rng.integers(1, C, size=L)]
        if aref.min_frames(tg) > T:
            continue
        probs = _random_probs(rng, T, C, done % 3 == 0)
        want, got = aref.viterbi(probs, tg), gref.viterbi(probs, gref.chain(tg))
        assert np.float32(got["path_logp"]).tobytes() == np.float32(want["path_logp"]).tobytes()
        assert np.array_equal(got["nodes"], np.arange(L)) and np.array_equal(got["spans"], want["spans"])
        assert np.array_equal(got["token_probs"], want["token_probs"])
        done += 1
    assert gref.viterbi(_random_probs(rng, 2, C, False), gref.chain([1, 1])) is None      # needs three frames


def random_graph(rng, C, max_nodes=6):
    N = int(rng.integers(0, max_nodes + 1))
    labels = rng.integers(1, C, size=N)
    flags = rng.integers(0, 4, size=N)
    if N:
        flags[rng.integers(0, N)] |= gref.START
        flags[rng.integers(0, N)] |= gref.FINAL
    preds = [[int(p) for p in rng.permutation(N)[:rng.integers(0, min(N, 3) + 1)]] for _ in range(N)]      # cycles, self-loops
    weights = -2.0 * rng.random(N).astype(np.float32)
    return gref.graph(labels, flags, preds, weights, bool(rng.integers(0, 2)))


def test_reference_against_brute_force():
    rng = np.random.default_rng(11)
    reachable = 0
    for case in range(40):
        T, C = int(rng.integers(1, 6)), 4
        g = random_graph(rng, C)
        probs = _random_probs(rng, T, C, case % 4 == 0)
        best, got = gref.brute_force(probs, g), gref.viterbi(probs, g)
        assert (best is None) == (got is None), case
        if got is None:
            continue
        reachable += 1
        frames = gref.path_labels(g, got["nodes"], got["spans"], T)
        assert np.array_equal(frames, got["frame_labels"])
        assert gref.accept(g, aref.collapse(frames)) is not None
        assert abs(gref.rescore64(probs, frames, g, got["nodes"]) - best) < 1e-5
        assert abs(float(got["path_logp"]) - best) < 1e-5
    assert reachable >= 20


def test_plan_numbers_and_refusals():
    info = _native.grammar_plan(32, 501, 2048, 8192)
    assert info["node_stride"] == 2048 and info["bp_bytes"] == 2 * 32 * 501 * 2048
    # LDS: two rows of (tok, blk) pairs, node words and weights, 16-bit arc offsets and arcs, the feeder's two chunks of 16 x 128 floats
    assert info["lds_bytes"] == 16 * 2048 + 8 * 2048 + 2 * (2048 + 4) + 2 * 8192 + 2 * 4 * 16 * 128 and info["lds_bytes"] < 160 * 1024
    assert _native.grammar_plan(1, 1, 0, 0)["node_stride"] == 4 and _native.grammar_plan(3, 7, 257, 1)["node_stride"] == 260
    L = _native.lib()
    out = np.zeros(3, dtype=np.int64)
    ptr = out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    for args, code in [((0, 5, 1, 1), _native.DSMI_ERR_INVALID), ((5, 0, 1, 1), _native.DSMI_ERR_INVALID), ((1, 1, -1, 0), _native.DSMI_ERR_INVALID),
                       ((1, 1, 2049, 0), _native.DSMI_ERR_CAPACITY), ((1, 1, 2048, 8193), _native.DSMI_ERR_CAPACITY),
                       ((1 << 12, 1 << 12, 2048, 0), _native.DSMI_ERR_CAPACITY)]:
        assert L.dsmi_grammar_plan(*args, ptr) == code, args
        assert not out.any()
    assert L.dsmi_grammar_plan(1, 1, 1, 1, None) == _native.DSMI_ERR_INVALID
    assert _native.GRAMMAR_MAX_NODES == 2048 and _native.GRAMMAR_MAX_ARCS == 8192
