"""Streaming grammar decoding on the GPU (dsmi_grammar_stream_advance_many: csrc/grammar_net.hip, the kernel
csrc/grammar_stream.hip).  The contract is equality with dsmi_grammar over the rows laid end to end, bit for bit: finals against
the graph itself, partials against the graph with every node final and empty_ok, however the utterance is cut into calls and
whatever else is in the call; the heavy-node pass on either side of its threshold; many sessions against each alone; reset;
refusals that change nothing; and the recogniser surface end to end on a synthetic unidirectional model."""
import ctypes
import warnings
from types import SimpleNamespace

import numpy as np
import pytest

from danspeech_amd import synthetic as syn
from danspeech_amd.grammar import Grammar

import _grammar_ref as gref
from _spot_stream_ref import cuts_of
from test_gpu_grammar import GRAMMARS, _peaky, _render, _ring
from test_spot_stream_host import KINDS

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
LABELS = syn.DANSPEECH_LABELS
C = len(LABELS)
FRAMES = (1, 2, 15, 16, 17, 33, 64, 65, 121, 140)      # the feeder's chunk of 16, the backtrace's 64 lanes


@pytest.fixture(scope="module")
def native():
    from danspeech_amd import _native
    return _native


@pytest.fixture(scope="module")
def dec(native):
    d = native.NativeDecoder(LABELS, blank_index=0)
    yield d
    d.close()


def _all_final(g):
    """The graph a partial result is defined on: every node final, the empty sentence accepted."""
    return SimpleNamespace(labels=g.labels, flags=np.asarray(g.flags) | gref.FINAL, weights=getattr(g, "weights", None), arc_off=g.arc_off,
                           arc_pred=g.arc_pred, empty_ok=True)


def _row(out, b, F):
    """Clip b of a dsmi_grammar result, as advance_many shapes a stream's."""
    lens, nodes, spans, tp, lp, st = out
    return (int(lens[b]), nodes[b, :F].copy(), spans[b, :F].copy(), tp[b, :F].copy(), float(lp[b]), int(st[b]))


def _one_shot(dec, g, X):
    """dsmi_grammar of the single clip X (B = 1, T_out = F); the zero-frame result for no rows."""
    F = len(X)
    if F == 0:
        return (0, np.zeros(0, np.int32), np.zeros((0, 2), np.int32), np.zeros(0, np.float32), 0.0 if g.empty_ok else -np.inf, 0 if g.empty_ok else 1)
    return _row(dec.grammar(torch.from_numpy(X[None]).cuda(), None, g), 0, F)


def _prefixes(dec, g, X):
    """dsmi_grammar of every prefix of X on the all-final graph, in one call: [f] = the partial result after f frames."""
    F = len(X)
    out = [(0, np.zeros(0, np.int32), np.zeros((0, 2), np.int32), np.zeros(0, np.float32), 0.0, 0)]
    if F:
        res = dec.grammar(torch.from_numpy(np.repeat(X[None], F, 0)).cuda(), np.arange(1, F + 1, dtype=np.int32), _all_final(g))
        for f in range(1, F + 1):
            assert not res[1][f - 1, f:].any() and not res[2][f - 1, f:].any() and not res[3][f - 1, f:].any()
            out.append(_row(res, f - 1, f))
    return out


def _same(got, want, what=None):
    assert got[0] == want[0] and got[5] == want[5], (what, got[0], want[0], got[5], want[5])
    assert np.float32(got[4]).tobytes() == np.float32(want[4]).tobytes(), (what, got[4], want[4])
    for k in (1, 2, 3):
        assert got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), (what, k)
    M = got[0]
    assert not got[1][M:].any() and not got[2][M:].any() and not got[3][M:].any()


def _complete(g, res):
    """Whether the end state of a result's path is one the graph accepts."""
    return int(bool(g.empty_ok)) if res[0] == 0 else int(bool(g.flags[res[1][res[0] - 1]] & gref.FINAL))


def _run(native, streams, graphs, utts, cuts, phase=None, partial=True):
    """Advance every stream through its utterance in shared calls (stream i joins at call phase[i]); the last call of a stream has
    mode 2, the others mode 1 (or 0).  -> per stream the list of (frames so far, mode, result) of its calls."""
    n = len(streams)
    phase = phase or [0] * n
    dev = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in utts]
    at, seen = [0] * n, [[] for _ in range(n)]
    for call in range(max(p + len(c) for p, c in zip(phase, cuts))):
        who, rows, modes = [], [], []
        for i in range(n):
            k = call - phase[i]
            if 0 <= k < len(cuts[i]):
                who.append(i)
                rows.append(dev[i][at[i]:at[i] + cuts[i][k]] if cuts[i][k] else None)
                modes.append(2 if k == len(cuts[i]) - 1 else 1 if partial else 0)
                at[i] += cuts[i][k]
            elif call % 2 and k < 0:         # (an idle stream in the call: no frames, nothing due)
                who.append(i); rows.append(None); modes.append(0)
        res = native.NativeGrammarStream.advance_many([streams[i] for i in who], rows, modes)
        for i, m, r in zip(who, modes, res):
            assert (r is None) == (m == 0)
            if m:
                seen[i].append((at[i], m, r))
            assert streams[i].frames() == at[i]
    return seen


@pytest.fixture(scope="module")
def compiled():
    return {k: Grammar(v, LABELS) for k, v in GRAMMARS.items() if v}


@pytest.fixture(scope="module")
def chunked(dec, compiled):
    """Ten utterances over three graphs with their references: the one-shot final and the partial of every prefix, computed once."""
    rng = np.random.default_rng(77)
    graphs = [compiled["digits"], compiled["sentence"], _ring(7, rng, C, fan=2)]
    which = [i % 3 for i in range(len(FRAMES))]
    utts = [_peaky(rng, F, C, sharp=3.0) for F in FRAMES]
    finals = [_one_shot(dec, graphs[g], x) for g, x in zip(which, utts)]
    partials = [_prefixes(dec, graphs[g], x) for g, x in zip(which, utts)]
    assert {f[5] for f in finals} == {0, 1}      # (the sentence grammar does not fit the short utterances)
    return graphs, which, utts, finals, partials


# ---- 1. five chunkings, bit for bit
@pytest.mark.parametrize("kind", KINDS)
def test_every_chunking_gives_the_one_shot_bits(native, dec, chunked, kind):
    graphs, which, utts, finals, partials = chunked
    rng = np.random.default_rng(len(kind))
    net = native.NativeGrammarNet(dec, graphs)
    streams = [native.NativeGrammarStream(net, g, max_frames=160) for g in which]
    cuts = [cuts_of(rng, len(x), kind) for x in utts]
    if kind == "single":
        assert cuts[FRAMES.index(33)] == [1] * 33
    if kind == "empties":
        assert all(c[0] == 0 and c[-1] == 0 for c in cuts)       # an empty first call, a final call without frames
    seen = _run(native, streams, graphs, utts, cuts, phase=[i % 4 for i in range(len(utts))])
    for i, calls in enumerate(seen):
        g = graphs[which[i]]
        assert len(calls) == len(cuts[i]) and calls[-1][1] == 2 and calls[-1][0] == len(utts[i])
        for F, mode, r in calls:
            want = finals[i] if mode == 2 else partials[i][F]
            _same(r, want, (kind, i, F, mode))
            assert r[6] == (1 - r[5] if mode == 2 else _complete(g, r)), (kind, i, F, mode)
    for s in streams:
        s.close()
    net.close()


def test_against_the_numpy_reference(native, dec, compiled):
    g = compiled["digits"]
    rng = np.random.default_rng(5)
    X = _peaky(rng, 121, C, sharp=3.0)
    net = native.NativeGrammarNet(dec, g)
    s = native.NativeGrammarStream(net, 0, max_frames=121)
    (calls,) = _run(native, [s], [g], [X], [[40, 1, 80]])
    for F, mode, r in calls:
        ref = gref.viterbi(X[:F], g if mode == 2 else _all_final(g))
        r64 = gref.viterbi(X[:F], g if mode == 2 else _all_final(g), dtype=np.float64)
        assert r[5] == 0 and abs(r[4] - float(ref["path_logp"])) < 1e-3
        frames = gref.path_labels(_all_final(g) if mode == 1 else g, r[1][:r[0]], r[2][:r[0]], F)
        assert abs(gref.rescore64(X[:F], frames, g, r[1][:r[0]]) - float(r64["path_logp"])) < 1e-3
    s.close(); net.close()


def test_partials_of_a_rendered_sentence_are_its_prefixes(native, dec, compiled):
    g = compiled["sentence"]
    rng = np.random.default_rng(9)
    sentence = g.sentences(40)[-1]
    X, _ = _render(rng, g, sentence, C)
    net = native.NativeGrammarNet(dec, g)
    s = native.NativeGrammarStream(net, 0, max_frames=len(X))
    (calls,) = _run(native, [s], [g], [X], [cuts_of(rng, len(X), "random")])
    texts = [g.text_of(r[1][:r[0]]) for _, _, r in calls]
    assert texts[-1] == sentence and calls[-1][2][6] == 1
    for (F, mode, r), text in zip(calls, texts):
        assert sentence.startswith(text), (F, text)
        assert r[6] == _complete(g, r)
    assert len(set(texts)) > 2
    s.close(); net.close()


# ---- 2. the thread stride and the heavy nodes
def _two_calls(native, dec, g, X, exact=False, cut=None):
    net = native.NativeGrammarNet(dec, g)
    s = native.NativeGrammarStream(net, 0, max_frames=len(X))
    cut = len(X) // 2 if cut is None else cut
    (calls,) = _run(native, [s], [g], [X], [[cut, len(X) - cut]])
    _same(calls[0][2], _one_shot(dec, _all_final(g), X[:cut]), "partial")
    _same(calls[1][2], _one_shot(dec, g, X), "final")
    if exact:
        ref = gref.viterbi(X, g)
        r = calls[1][2]
        np.testing.assert_array_equal(r[1][:r[0]], ref["nodes"])
        np.testing.assert_array_equal(r[2][:r[0]], ref["spans"])
    s.close(); net.close()
    return calls


@pytest.mark.parametrize("N", [1, 255, 256, 257, 600])
def test_node_counts_either_side_of_the_thread_stride(native, dec, N):
    rng = np.random.default_rng(N)
    _two_calls(native, dec, _ring(N, rng, C, fan=2), _peaky(rng, 48, C, sharp=3.0), cut=17)


@pytest.mark.parametrize("fan", [32, 33])
def test_fan_in_either_side_of_the_heavy_threshold(native, dec, fan):
    rng = np.random.default_rng(fan)
    g = _ring(70, rng, C, fan=fan)
    _two_calls(native, dec, g, _peaky(rng, 40, C, sharp=3.0))
    _two_calls(native, dec, gref.graph(g.labels, g.flags, [list(g.arc_pred[g.arc_off[n]:g.arc_off[n + 1]]) for n in range(70)]),
               np.full((20, C), 1.0 / C, dtype=np.float32), exact=True)


def test_one_node_with_a_fan_in_of_300(native, dec):
    rng = np.random.default_rng(300)
    labels = rng.integers(1, C, size=301)
    preds = [[] for _ in range(300)] + [[int(p) for p in rng.permutation(300)]]
    g = gref.graph(labels, [gref.START] * 300 + [gref.FINAL], preds, -rng.random(301).astype(np.float32))
    _two_calls(native, dec, g, _peaky(rng, 40, C, sharp=3.0))
    # without weights and on uniform probabilities everything ties: the first predecessor of the list wins
    g = gref.graph(labels, [gref.START] * 300 + [gref.FINAL], preds)
    calls = _two_calls(native, dec, g, np.full((12, C), 1.0 / C, dtype=np.float32), exact=True)
    assert calls[1][2][1][0] == preds[300][0]


def test_graphs_at_the_limits(native, dec):
    rng = np.random.default_rng(2048)
    nodes = _ring(native.GRAMMAR_MAX_NODES, rng, C, fan=1)
    arcs = _ring(native.GRAMMAR_MAX_NODES, rng, C, fan=4)
    assert len(arcs.arc_pred) == native.GRAMMAR_MAX_ARCS
    for g in (nodes, arcs):
        _two_calls(native, dec, g, _peaky(rng, 64, C, sharp=3.0))


# ---- 3. many sessions equal each alone
def test_many_sessions_equal_each_alone(native, dec, compiled):
    rng = np.random.default_rng(37)
    graphs = [compiled["digits"], compiled["sentence"], _ring(300, rng, C, fan=3)]
    net = native.NativeGrammarNet(dec, graphs)
    assert (net.K, net.max_nodes, net.max_arcs) == (3, 300, 900)
    n = 37
    which = [int(rng.integers(0, 3)) for _ in range(n)]
    utts = [_peaky(rng, int(rng.integers(1, 90)), C, sharp=3.0) for _ in range(n)]
    cuts = [cuts_of(rng, len(x), KINDS[i % len(KINDS)] if KINDS[i % len(KINDS)] != "single" else "empties") for i, x in enumerate(utts)]
    phase = [int(rng.integers(0, 5)) for _ in range(n)]
    together = _run(native, [native.NativeGrammarStream(net, g, max_frames=90) for g in which], graphs, utts, cuts, phase, partial=True)
    for i in range(n):
        s = native.NativeGrammarStream(net, which[i], max_frames=90)
        (alone,) = _run(native, [s], graphs, [utts[i]], [cuts[i]])
        assert len(alone) == len(together[i])
        for (F1, m1, r1), (F2, m2, r2) in zip(alone, together[i]):
            assert (F1, m1, r1[6]) == (F2, m2, r2[6])
            _same(r1, r2, i)
        s.close()


# ---- 4. reset, and an utterance nothing accepts
def test_reset_mid_utterance_then_a_fresh_utterance(native, dec, compiled):
    g = compiled["digits"]
    rng = np.random.default_rng(4)
    net = native.NativeGrammarNet(dec, g)
    a, b = native.NativeGrammarStream(net, 0, max_frames=100), native.NativeGrammarStream(net, 0, max_frames=100)
    junk, X = _peaky(rng, 70, C, sharp=3.0), _peaky(rng, 50, C, sharp=3.0)
    a.advance(torch.from_numpy(junk).cuda(), 1)
    assert a.frames() == 70
    a.reset()
    assert a.frames() == 0
    (ca,), (cb,) = _run(native, [a], [g], [X], [[20, 30]]), _run(native, [b], [g], [X], [[20, 30]])
    for (F1, m1, r1), (F2, m2, r2) in zip(ca, cb):
        assert (F1, m1, r1[6]) == (F2, m2, r2[6])
        _same(r1, r2)
    _same(ca[-1][2], _one_shot(dec, g, X))
    # after the final result: frames are refused until a reset, a result may be asked for again
    with pytest.raises(native.DsmiError) as e:
        a.advance(torch.from_numpy(X[:3]).cuda(), 0)
    assert e.value.code == native.DSMI_ERR_INVALID and "ended" in str(e.value) and "stream 0" in str(e.value)
    _same(a.advance(None, 2), ca[-1][2])
    a.reset()
    _same(a.advance(torch.from_numpy(X).cuda(), 2), ca[-1][2])
    a.close(); b.close(); net.close()


def test_an_utterance_no_sentence_fits(native, dec, compiled):
    g = compiled["sentence"]
    rng = np.random.default_rng(6)
    X = _peaky(rng, 12, C, sharp=3.0)        # (the shortest sentence needs more frames)
    net = native.NativeGrammarNet(dec, g)
    s = native.NativeGrammarStream(net, 0, max_frames=12)
    part = s.advance(torch.from_numpy(X[:7]).cuda(), 1)
    assert part[5] == 0 and np.isfinite(part[4]) and part[6] == 0
    _same(part, _one_shot(dec, _all_final(g), X[:7]))
    fin = s.advance(torch.from_numpy(X[7:]).cuda(), 2)
    assert fin[0] == 0 and fin[4] == -np.inf and fin[5] == 1 and fin[6] == 0
    _same(fin, _one_shot(dec, g, X))
    # without frames: mode 1 the empty path, mode 2 dsmi_grammar's zero-frame result
    s.reset()
    assert s.advance(None, 1)[4:] == (0.0, 0, 0)
    assert s.advance(None, 2)[4:] == (-np.inf, 1, 0)
    s.close(); net.close()


# ---- 5. refusals change nothing
def test_refusals_change_nothing(native, dec, compiled):
    L = native.lib()
    g = compiled["digits"]
    rng = np.random.default_rng(12)
    net, other = native.NativeGrammarNet(dec, g), native.NativeGrammarNet(dec, g)
    X = _peaky(rng, 30, C, sharp=3.0)
    x_dev = torch.from_numpy(X).cuda()
    a, b, never = (native.NativeGrammarStream(net, 0, max_frames=30) for _ in range(3))
    foreign = native.NativeGrammarStream(other, 0, max_frames=30)
    done = native.NativeGrammarStream(net, 0, max_frames=30)
    done.advance(x_dev[:5], 2)
    a.advance(x_dev[:10], 0); b.advance(x_dev[:10], 0); never.advance(x_dev[:10], 0)
    i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)

    def call(streams, frames, modes, P=64, rows=True, outputs=True, n=None, null=()):
        hs = (ctypes.c_void_p * len(streams))(*[None if s is None else s._h for s in streams])
        ps = (ctypes.c_void_p * len(streams))(*[x_dev[10:].data_ptr() if rows and f > 0 else None for f in frames])
        fr, mo = i32(frames), i32(modes)
        m = len(streams)
        lens, st, cp = (np.full(m, 7, dtype=np.int32) for _ in range(3))
        nodes, spans = np.full((m, max(P, 0)), 7, dtype=np.int32), np.full((m, max(P, 0), 2), 7, dtype=np.int32)
        tp, lp = np.full((m, max(P, 0)), 7.5, dtype=np.float32), np.full(m, 7.5, dtype=np.float32)
        ptr = lambda x, name: None if (not outputs or name in null) else native._np_ptr(x)
        before = [s.frames() for s in streams if s is not None]
        rc = L.dsmi_grammar_stream_advance_many(None if "streams" in null else hs, len(streams) if n is None else n, ps,
                                                None if "frames" in null else native._np_ptr(fr), None if "mode" in null else native._np_ptr(mo), P,
                                                ptr(lens, "lens"), ptr(nodes, "nodes"), ptr(spans, "spans"), ptr(tp, "tp"), ptr(lp, "lp"), ptr(st, "st"),
                                                native._np_ptr(cp), None)
        untouched = all((x == 7).all() for x in (lens, st, cp, nodes, spans)) and (tp == 7.5).all() and (lp == 7.5).all()
        assert rc == 0 or before == [s.frames() for s in streams if s is not None]
        return rc, untouched, L.dsmi_grammar_stream_last_error(None).decode()

    INV, CAP = native.DSMI_ERR_INVALID, native.DSMI_ERR_CAPACITY
    faults = [
        (dict(streams=[a, b], frames=[1, 1], modes=[1, 1], null=("streams",)), INV, "bad grammar stream arguments"),
        (dict(streams=[a, b], frames=[1, 1], modes=[1, 1], null=("frames",)), INV, "bad grammar stream arguments"),
        (dict(streams=[a, b], frames=[1, 1], modes=[1, 1], null=("mode",)), INV, "bad grammar stream arguments"),
        (dict(streams=[a, None], frames=[1, 1], modes=[1, 1]), INV, "stream 1: null handle"),
        (dict(streams=[a, b], frames=[1, 1], modes=[1, 1], n=0), INV, "bad grammar stream arguments"),
        (dict(streams=[a, b], frames=[1, 1], modes=[1, 1], n=native.GRAMMAR_STREAM_MANY_MAX + 1), INV, "bad grammar stream arguments"),
        (dict(streams=[a, b, a], frames=[1, 1, 1], modes=[1, 1, 1]), INV, "stream 2: the same handle appears twice"),
        (dict(streams=[a, foreign], frames=[1, 1], modes=[1, 1]), INV, "stream 1: the streams of one call must belong to one net"),
        (dict(streams=[a, b], frames=[1, -1], modes=[1, 1]), INV, "stream 1: negative frame count"),
        (dict(streams=[a, b], frames=[1, 2], modes=[1, 1], rows=False), INV, "stream 0: no probabilities for 1 frames"),
        (dict(streams=[a, b], frames=[1, 1], modes=[1, 3]), INV, "stream 1: mode 3 outside 0 .. 2"),
        (dict(streams=[a, b], frames=[1, 1], modes=[-1, 1]), INV, "stream 0: mode -1 outside 0 .. 2"),
        (dict(streams=[a, done], frames=[1, 1], modes=[1, 1]), INV, "stream 1: the utterance has ended"),
        (dict(streams=[a, b], frames=[1, 5], modes=[0, 1], P=14), INV, "stream 1: P_stride 14 is below the utterance's 15 frames"),
        (dict(streams=[a, b], frames=[1, 1], modes=[0, 1], outputs=False), INV, "an output array is NULL"),
        (dict(streams=[a, b], frames=[1, 1], modes=[0, 1], null=("tp",)), INV, "an output array is NULL"),
        (dict(streams=[a, b], frames=[1, 21], modes=[1, 1]), CAP, "stream 1: the utterance would reach 31 frames, max_frames is 30"),
        (dict(streams=[a, b], frames=[1, 1], modes=[1, 1], P=(1 << 23) + 1), CAP, "n * P_stride exceeds 2^24"),
    ]
    for kw, code, text in faults:
        big = kw.get("P", 0) > 1 << 20
        if big:                         # (no arrays of 2^23 rows: the numbers alone refuse, before any output is looked at)
            hs = (ctypes.c_void_p * 2)(a._h, b._h)
            one = np.zeros(4, dtype=np.int32)
            rc = L.dsmi_grammar_stream_advance_many(hs, 2, (ctypes.c_void_p * 2)(x_dev.data_ptr(), x_dev.data_ptr()), native._np_ptr(i32([1, 1])),
                                                    native._np_ptr(i32([1, 1])), kw["P"], *([native._np_ptr(one)] * 7), None)
            untouched, msg = not one.any(), L.dsmi_grammar_stream_last_error(None).decode()
        else:
            rc, untouched, msg = call(**kw)
        assert rc == code and untouched and text in msg, (kw.get("null"), rc, msg)
        assert (a.frames(), b.frames(), done.frames()) == (10, 10, 5)
    # mode 0 only: nothing is written, no output is needed; no frames and nothing due: no launch, nothing changes
    rc, untouched, _ = call([a, b], [0, 0], [0, 0], outputs=False)
    assert rc == 0 and untouched
    # max_frames reached exactly, then one past it
    for s in (a, b, never):
        s.advance(x_dev[10:29], 0)
    rc, untouched, _ = call([a, b], [1, 1], [0, 0], outputs=False)       # (rows: x_dev[10:], so put the right row in below)
    assert rc == 0 and untouched and (a.frames(), b.frames()) == (30, 30)
    rc, untouched, msg = call([a, b], [0, 1], [0, 0])
    assert rc == CAP and untouched and "would reach 31 frames, max_frames is 30" in msg
    # the refused streams finish to the bits of one that was never refused (frame 29 was fed from row 10: so is `never`'s)
    never.advance(x_dev[10:11], 0)
    fa, fb, fn = a.advance(None, 2), b.advance(None, 2), never.advance(None, 2)
    _same(fa, fn); _same(fb, fn)
    _same(fn, _one_shot(dec, g, np.concatenate([X[:29], X[10:11]])))
    for s in (a, b, never, foreign, done):
        s.close()
    net.close(); other.close()


def test_net_refuses_what_dsmi_grammar_refuses(native, dec):
    ok = gref.graph([1, 2, 3], [1, 0, 2], [[], [0], [0, 1]], [0, -1, 0])
    native.NativeGrammarNet(dec, ok).close()
    cases = [(gref.graph([1, 0, 3], [1, 0, 2], [[], [0], [0, 1]]), "is the blank or not a label"),
             (gref.graph([1, 2, 3], [1, 0, 2], [[], [0], [0, 5]]), "outside the graph"),
             (gref.graph([1, 2, 3], [0, 0, 2], [[], [0], [0, 1]]), "no start node"),
             (gref.graph([1, 2, 3], [1, 0, 0], [[], [0], [0, 1]]), "no final node"),
             (gref.graph([1, 2, 3], [1, 0, 2], [[], [0], [0, 1]], [0, np.nan, 0]), "weight is not finite")]
    for g, text in cases:
        with pytest.raises(native.DsmiError) as e:
            native.NativeGrammarNet(dec, g)
        assert e.value.code == native.DSMI_ERR_INVALID and str(e.value).find("grammar: ") >= 0 and text in str(e.value)
    N = native.GRAMMAR_MAX_NODES + 1
    with pytest.raises(native.DsmiError) as e:
        native.NativeGrammarNet(dec, gref.graph(np.ones(N), np.full(N, 3), [[] for _ in range(N)]))
    assert e.value.code == native.DSMI_ERR_CAPACITY and "DSMI_GRAMMAR_MAX_NODES" in str(e.value)
    net = native.NativeGrammarNet(dec, ok)
    for graph, frames, code in ((1, 10, native.DSMI_ERR_INVALID), (-1, 10, native.DSMI_ERR_INVALID), (0, 0, native.DSMI_ERR_INVALID),
                                (0, native.GRAMMAR_STREAM_MAX_FRAMES + 1, native.DSMI_ERR_CAPACITY)):
        with pytest.raises(native.DsmiError) as e:
            native.NativeGrammarStream(net, graph, max_frames=frames)
        assert e.value.code == code
    net.close()


# ---- 6. the surface, on the synthetic streaming model of tests/test_gpu_spot_stream.py
def _stream_model(name, H, L, ctx, seed):
    from danspeech_amd.deepspeech.model import DeepSpeech
    sd = syn.make_state_dict(2, "gru", H, L, bidirectional=False, context=ctx, seed=seed, fc_gain=8.0)
    return DeepSpeech(name, rnn_type="gru", rnn_hidden_size=H, rnn_layers=L, conv_layers=2, context=ctx, bidirectional=False,
                      streaming_inference_model=True).load_state_dict(sd)


def test_surface_commands_and_unchanged_texts(native, monkeypatch):
    from danspeech_amd import Recognizer
    m = _stream_model("stream-grammar", 64, 2, 20, seed=99)
    audio = [syn.make_clip(20 + i, 32000 + 5311 * i) for i in range(5)]      # (two seconds and more: every recording has middle parts)
    made = []
    for cls in (native.NativeGrammarNet, native.NativeGrammarStream):
        init = cls.__init__
        monkeypatch.setattr(cls, "__init__", lambda self, *a, _init=init, **k: (made.append(type(self).__name__), _init(self, *a, **k))[1])
    rec = Recognizer()
    rec.enable_real_time_streaming(streaming_model=m)
    plain = list(rec.stream_recordings(audio, chunk_samples=1024))
    quiet = np.random.RandomState(5).randint(-30, 31, size=8000 + 20800).astype(np.float64)
    sources = [np.concatenate((quiet[:8000], a, quiet[8000:])).astype(np.int16) for a in audio[:2]]      # a burst the gate opens and closes on
    sources = [[x[i:i + 4000] for i in range(0, len(x), 4000)] for x in sources]
    live_plain = list(rec.stream_live(sources))
    assert made == [] and rec.danspeech_recognizer.take_commands() == []              # grammar=None: no handles
    finals = [t for _, last, t in plain if last]
    words = sorted(set(w for t in finals for w in t.split()))[:12] or ["ja"]
    text = "(" + " | ".join(words + ["ja", "nej"]) + ")+"
    with pytest.raises(ValueError):
        rec.enable_real_time_streaming(streaming_model=m, grammar="(ja | nej")
    assert made == []
    rec.enable_real_time_streaming(streaming_model=m, grammar=text, grammar_partials=True)
    eng = rec.danspeech_recognizer
    g = eng._grammar_spec[0]
    fed, asked = {}, []                                                                 # stream handle -> [rows] per utterance; the modes
    advance = native.NativeGrammarStream.advance_many

    def recording(streams, rows, modes):
        asked.extend(modes)
        for s, p, mode in zip(streams, rows, modes):
            fed.setdefault(id(s), [[]])[-1].append(None if p is None else p.reshape(-1, p.shape[-1]).clone())
            if mode == 2:
                fed[id(s)].append([])
        return advance(streams, rows, modes)
    monkeypatch.setattr(native.NativeGrammarStream, "advance_many", staticmethod(recording))
    heard = []
    assert list(rec.stream_recordings(audio, chunk_samples=1024, on_command=lambda *c: heard.append(c))) == plain
    assert made.count("NativeGrammarNet") == 1 and made.count("NativeGrammarStream") == len(audio)
    # every final: decode_grammar over the rows the session was fed
    got = {}
    for index, ordinal, final, item in heard:
        got.setdefault(index, []).append((ordinal, final, item))
    assert sorted(got) == list(range(len(audio)))
    frame_s = eng.frame_seconds()
    want = []
    for utterances in fed.values():
        for parts in utterances:
            rows = [p for p in parts if p is not None]
            if not parts:
                continue
            if not rows:
                want.append(("", [], 0.0) if g.empty_ok else None)
                continue
            d = eng.decoder.decode_grammar(torch.cat(rows)[None], g)[0]
            want.append(None if d is None else (d[0], [(c, a * frame_s, e * frame_s) for c, a, e, _ in d[1]], d[2]))
    have = []
    for index, items in got.items():
        assert [o for o, f, _ in items if f] == [0] and items[-1][1]              # one utterance, its final last
        for ordinal, final, item in items[:-1]:
            assert not final and isinstance(item[0], str) and item[1] in (True, False)
        fin = items[-1][2]
        have.append(fin)
        if fin is not None:
            assert g.accepts(fin[0]) and [w for w, *_ in fin[1]] == fin[0].split()
    key = lambda r: (r is None, r and r[0], r and r[2])
    assert sorted(map(key, have)) == sorted(map(key, want))
    by_text = {(w[0], w[2]): w for w in want if w is not None}
    for fin in have:
        if fin is None:
            continue
        chars = by_text[(fin[0], fin[2])][1]
        k = 0
        for word, a, e, _ in fin[1]:              # character spans: a word starts with its first character and ends with its last
            while chars[k][0] == " ":
                k += 1
            assert a == chars[k][1] and e == chars[k + len(word) - 1][2]
            k += len(word)
    assert any(f is not None for f in have)
    partials = [c for c in heard if not c[2]]
    assert len(partials) == asked.count(1) and asked.count(2) == len(audio) and 0 not in asked
    assert all(len(items) >= 2 and not items[0][1] for items in got.values())      # partials before each final
    live_heard = []
    assert list(rec.stream_live(sources, on_command=lambda *c: live_heard.append(c))) == live_plain
    assert live_heard and all(h[0] in (0, 1) for h in live_heard) and any(h[2] for h in live_heard)
    # watch and grammar together: the watch's detections are those of the watch alone
    pair = words[0][:2] if len(words[0]) >= 2 else "ja"
    monkeypatch.setattr(native.NativeGrammarStream, "advance_many", staticmethod(advance))
    rec.enable_real_time_streaming(streaming_model=m, watch=[pair], watch_confidence=0.02, watch_settle_s=0.1)
    alone = []
    assert list(rec.stream_recordings(audio, chunk_samples=1024, on_detection=lambda *d: alone.append(d))) == plain
    rec.enable_real_time_streaming(streaming_model=m, watch=[pair], watch_confidence=0.02, watch_settle_s=0.1, grammar=text)
    both, commands = [], []
    assert list(rec.stream_recordings(audio, chunk_samples=1024, on_detection=lambda *d: both.append(d), on_command=lambda *c: commands.append(c))) == plain
    assert both == alone and len(commands) == len(audio) and all(c[2] for c in commands)      # (no partials asked for: finals only)
    # an utterance longer than grammar_max_s: one warning, None, nothing refused
    rec.enable_real_time_streaming(streaming_model=m, grammar=text, grammar_max_s=0.2)
    short = []
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert list(rec.stream_recordings(audio[:1], chunk_samples=1024, on_command=lambda *c: short.append(c))) == [p for p in plain if p[0] == 0]
    assert len([x for x in w if "grammar_max_s" in str(x.message)]) == 1
    assert short == [(0, 0, True, None)]
    rec.disable_real_time_streaming()
