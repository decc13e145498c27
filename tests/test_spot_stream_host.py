"""CPU checks of the streaming phrase watch: the online picking rule on the host (dsmi_spot_watch_pick, the inline function the
kernel runs too) against the rule written out in numpy (tests/_spot_stream_ref.py), the numpy chunked trellis against the whole
one, the refusals that need no handle, and the condition under which the online rule and dsmi_spot's offline picking agree.  No
kernels run."""
import ctypes

import numpy as np
import pytest

import _spot_ref as ref
import _spot_stream_ref as sref

INT_MAX = 2 ** 31 - 1
KINDS = ("random", "single", "one", "empties", "aligned")


@pytest.fixture(scope="module")
def native():
    from danspeech_amd import _native
    return _native


def _native_pick(native, E, ST, floor, settle, cuts, flush=True, max_events=None):
    """The whole tracks through dsmi_spot_watch_pick in ``cuts``: (events, counts per call)."""
    st, at, out, counts = native.SpotPickState.fresh(), 0, [], []
    for i, c in enumerate(cuts):
        M = native.SPOT_MAX_HITS if max_events is None else max_events
        n, ev = native.spot_watch_pick(E[at:at + c], ST[at:at + c], at, flush and i == len(cuts) - 1, floor, settle, st, max(M, c + 1) if max_events is None else M)
        out += ev
        counts.append(n)
        at += c
    assert at == len(E)
    return out, counts


def _random_tracks(rng, T, span=6, levels=5):
    """Tracks as a trellis could give them -- ST[f] <= f, some frames -inf / -1 -- with few distinct scores, so that equal scores
    between overlapping windows, starts equal to an earlier end and starts one past it all occur."""
    ST = np.array([f - int(rng.integers(0, min(f, span) + 1)) for f in range(T)], dtype=np.int32)
    E = (-rng.integers(1, levels + 1, size=T)).astype(np.float32)
    dead = rng.random(T) < 0.25
    E[dead], ST[dead] = -np.inf, -1
    return E, ST


def test_pick_equals_the_rule_on_random_tracks_in_random_splits(native):
    assert native.SPOT_STREAM_MANY_MAX == 4096
    rng = np.random.default_rng(11)
    fired = ties = 0
    for case in range(300):
        T = int(rng.integers(0, 90))
        E, ST = _random_tracks(rng, T)
        floor = [-np.inf, -1.0, -0.5, -2.0][case % 4]
        settle = [1, 2, 5, 25, INT_MAX][case % 5]
        want = sref.online_pick(E, ST, floor, settle)
        assert sref.disjoint_in_time_order(want), case
        for kind in KINDS:
            cuts = sref.cuts_of(rng, T, kind)
            assert sref.online_pick(E, ST, floor, settle, cuts) == want, (case, kind)          # the rule does not depend on the cuts
            got, counts = _native_pick(native, E, ST, floor, settle, cuts)
            assert got == want, (case, kind, got, want)
            assert sum(counts) == len(want)
        no_flush, _ = _native_pick(native, E, ST, floor, settle, [T], flush=False)
        assert no_flush == [h for h in want if h[3] < T], case          # (only the flush fires at the utterance's frame count)
        fired += len(want)
        ties += sum(1 for a in range(T) for b in range(a + 1, min(T, a + 6)) if E[a] == E[b] > -np.inf and ST[b] <= a)
    assert fired > 1500 and ties > 1000


def test_pick_hand_worked_cases(native):
    inf = np.float32(-np.inf)

    def run(E, ST, floor=-np.inf, settle=2, flush=True):
        E, ST = np.array(E, dtype=np.float32), np.array(ST, dtype=np.int32)
        want = sref.online_pick(E, ST, floor, settle, flush=flush)
        for cuts in ([len(E)], [1] * len(E), [0] + [1] * len(E) + [0]):
            got, _ = _native_pick(native, E, ST, floor, settle, cuts, flush)
            assert got == want, (cuts, got, want)
        return want

    # equal scores, windows that meet: the earlier one stays and fires settle frames after ITS end
    assert run([-1, -1, inf, inf], [0, 0, -1, -1]) == [(0, 1, -1.0, 2)]
    # a strictly better one that meets the pending window replaces it
    assert run([-2, -1, inf, inf, inf], [0, 0, -1, -1, -1]) == [(0, 2, -1.0, 3)]
    # a candidate beyond the pending window fires it at once (fired = that frame) and waits itself
    assert run([-1, -1], [0, 1], settle=9) == [(0, 1, -1.0, 1), (1, 2, -1.0, 2)]
    # ST == last_end is no candidate (the windows would share a frame), ST == last_end + 1 is
    assert run([-1, inf, -1, -1], [0, -1, 0, 1], settle=1) == [(0, 1, -1.0, 1), (1, 4, -1.0, 4)]
    assert run([-1, inf, -5, -1], [0, -1, 0, 0], settle=1) == [(0, 1, -1.0, 1)]
    # E exactly the threshold product passes; the next float32 below does not
    floor = np.float32(-0.7)
    exact = floor * np.float32(3)
    assert run([inf, inf, exact], [-1, -1, 0], floor=floor) == [(0, 3, float(exact), 3)]
    assert run([inf, inf, np.nextafter(exact, inf)], [-1, -1, 0], floor=floor) == []
    # settle_frames = 1: fired at the very next frame; INT_MAX: only the flush (or a later window) fires
    assert run([-1, inf, inf], [0, -1, -1], settle=1) == [(0, 1, -1.0, 1)]
    assert run([-1] + [inf] * 40, [0] + [-1] * 40, settle=INT_MAX) == [(0, 1, -1.0, 41)]
    assert run([-1] + [inf] * 40, [0] + [-1] * 40, settle=INT_MAX, flush=False) == []
    # a flush with nothing pending, and with no frames at all
    assert run([inf, inf], [-1, -1]) == [] and run([], []) == []
    # one-frame windows, every frame a hit of its own, in time order
    assert run([-1] * 5, list(range(5)), settle=3) == [(f, f + 1, -1.0, f + 1) for f in range(5)]


def test_pick_counts_what_it_cannot_store_and_writes_nothing_past_max_events(native):
    E, ST = np.full(6, -1, dtype=np.float32), np.arange(6, dtype=np.int32)
    want = sref.online_pick(E, ST, -np.inf, 1)
    assert len(want) == 6
    st = native.SpotPickState.fresh()
    n, ev = native.spot_watch_pick(E, ST, 0, True, -np.inf, 1, st, max_events=2)
    assert n == 6 and ev == want[:2] and (st.pending, st.last_end) == (0, 5)
    st = native.SpotPickState.fresh()
    assert native.spot_watch_pick(E, ST, 0, True, -np.inf, 1, st, max_events=0) == (6, [])
    # the raw call: rows past min(count, max_events) keep the caller's values
    L = native.lib()
    hits, sc, fi = np.full((4, 2), 7, np.int32), np.full(4, 7.5, np.float32), np.full(4, 7, np.int32)
    st = native.SpotPickState.fresh()
    rc = L.dsmi_spot_watch_pick(native._np_ptr(E[:2]), native._np_ptr(ST[:2]), 2, 0, 0, -np.inf, 1, ctypes.byref(st), 4, native._np_ptr(hits),
                                native._np_ptr(sc), native._np_ptr(fi))
    assert rc == 1 and hits.tolist() == [[0, 1], [7, 7], [7, 7], [7, 7]] and sc.tolist() == [-1, 7.5, 7.5, 7.5] and fi.tolist() == [1, 7, 7, 7]
    assert (st.pending, st.ps, st.pe, st.last_end, st.pv) == (1, 1, 1, 0, -1.0)


def test_refusals_that_need_no_handle(native):
    L = native.lib()
    E, ST = np.full(3, -1, dtype=np.float32), np.arange(3, dtype=np.int32)
    out = (np.zeros((2, 2), np.int32), np.zeros(2, np.float32), np.zeros(2, np.int32))

    def pick(E=E, ST=ST, frames=3, t0=0, floor=-1.0, settle=1, state=True, M=2, outs=out):
        st = native.SpotPickState.fresh()
        before = bytes(st)
        rc = L.dsmi_spot_watch_pick(None if E is None else native._np_ptr(E), None if ST is None else native._np_ptr(ST), frames, t0, 0, floor,
                                    settle, ctypes.byref(st) if state else None, M, *[None if o is None else native._np_ptr(o) for o in outs])
        return rc, bytes(st) == before

    assert pick() == (2, False)            # frames 0 and 1 fire at frames 1 and 2; frame 2 waits
    for kw in (dict(state=False), dict(frames=-1), dict(t0=-1), dict(t0=INT_MAX - 1), dict(E=None), dict(ST=None), dict(M=-1),
               dict(outs=(None, out[1], out[2])), dict(outs=(out[0], None, out[2])), dict(outs=(out[0], out[1], None)), dict(settle=0),
               dict(settle=-3), dict(floor=float("nan"))):
        assert pick(**kw) == (native.DSMI_ERR_INVALID, True), kw
    assert pick(t0=INT_MAX - 3)[0] >= 0 and pick(frames=0, E=None, ST=None) == (0, True) and pick(M=0, outs=(None, None, None))[0] == 2
    with pytest.raises(native.DsmiError):
        native.spot_watch_pick(E, ST, 0, False, float("nan"), 1, native.SpotPickState.fresh())
    with pytest.raises(ValueError):
        native.spot_watch_pick(E, ST[:2], 0, False, -1.0, 1, native.SpotPickState.fresh())
    # the handles: a null decoder, watch or stream list is refused with a text of the calling thread's, no GPU touched
    h = ctypes.c_void_p()
    ids, lens = np.array([[1, 2]], np.int32), np.array([2], np.int32)
    assert L.dsmi_spot_watch_create(None, native._np_ptr(ids), native._np_ptr(lens), 1, 2, -1.0, 5, ctypes.byref(h)) == native.DSMI_ERR_INVALID
    assert L.dsmi_spot_watch_last_error(None) == b"bad spot watch arguments" and not h
    assert L.dsmi_spot_stream_create(None, ctypes.byref(h)) == native.DSMI_ERR_INVALID
    assert L.dsmi_spot_stream_last_error(None) == b"bad spot stream arguments" and not h
    assert L.dsmi_spot_watch_info(None, None, None, None) == native.DSMI_ERR_INVALID
    assert L.dsmi_spot_stream_reset(None) == native.DSMI_ERR_INVALID and L.dsmi_spot_stream_frames(None, None) == native.DSMI_ERR_INVALID
    L.dsmi_spot_watch_destroy(None), L.dsmi_spot_stream_destroy(None)
    fr, fl = np.zeros(2, np.int32), np.zeros(2, np.int32)
    hits, sc, fi, cn = np.full((2, 1, 1, 2), 7, np.int32), np.full((2, 1, 1), 7.5, np.float32), np.full((2, 1, 1), 7, np.int32), np.full((2, 1), 7, np.int32)
    none2 = (ctypes.c_void_p * 2)(None, None)

    def advance(ss=none2, n=2, fr=fr, fl=fl, outs=(hits, sc, fi, cn)):
        return L.dsmi_spot_stream_advance_many(ss, n, None, None if fr is None else native._np_ptr(fr), None if fl is None else native._np_ptr(fl), 1,
                                               *[None if o is None else native._np_ptr(o) for o in outs], None, None, 0, None)

    for kw in (dict(ss=None), dict(n=0), dict(n=-1), dict(n=native.SPOT_STREAM_MANY_MAX + 1), dict(fr=None), dict(fl=None),
               dict(outs=(None, sc, fi, cn)), dict(outs=(hits, None, fi, cn)), dict(outs=(hits, sc, None, cn)), dict(outs=(hits, sc, fi, None))):
        assert advance(**kw) == native.DSMI_ERR_INVALID and L.dsmi_spot_stream_last_error(None) == b"bad spot stream arguments", kw
    assert advance() == native.DSMI_ERR_INVALID and L.dsmi_spot_stream_last_error(None) == b"spot stream 0: null handle"
    assert (hits == 7).all() and (sc == 7.5).all() and (fi == 7).all() and (cn == 7).all()
    with pytest.raises(ValueError, match="^streams, probs_list and flush must have one entry per stream$"):
        native.NativeSpotStream.advance_many([object()], [], [False])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_chunked_trellis_equals_the_whole(dtype):
    rng = np.random.default_rng(4)
    n = 0
    for C, T in ((5, 1), (5, 7), (5, 40), (33, 121), (33, 64)):
        p = ref.peaky(rng, T, C, 3.0)
        for L in (1, 2, 3, 12):
            ph = [int(x) for x in rng.integers(1, C, size=L)]
            if L == 2:
                ph[1] = ph[0]                       # two equal tokens: the blank between them
            E, ST = ref.tracks(p, ph, dtype=dtype)
            for kind in KINDS:
                Ec, Sc = sref.chunked_tracks(p, ph, sref.cuts_of(rng, T, kind), dtype=dtype)
                assert Ec.dtype == E.dtype and np.array_equal(Ec.view(np.int64 if dtype is np.float64 else np.int32),
                                                              E.view(np.int64 if dtype is np.float64 else np.int32)), (C, T, L, kind)
                assert np.array_equal(Sc, ST), (C, T, L, kind)
                n += int((E > -np.inf).sum())
    assert n > 2000


# ---- where the online rule and the offline picking must agree: planted, well-separated occurrences.  tests/test_gpu_spot_stream.py
# asserts the same equality on the GPU for exactly these inputs; here the numpy references alone show that the inputs satisfy it.
PLANTED_SEEDS = (0, 1, 2)
PLANTED_FLOOR = float(np.log(0.5))
PLANTED_SETTLE = (5, 25)


def planted_case(seed):
    """(probs [T, 33], phrases as label ids) of planted seed ``seed``."""
    from danspeech_amd import synthetic as syn
    labels = syn.DANSPEECH_LABELS
    rng = np.random.default_rng(1000 + seed)
    phrases = [[labels.index(c) for c in w] for w in ("alle", "hej", "noo")]
    return sref.planted(rng, 20, len(labels), phrases, copies=2), phrases


@pytest.mark.parametrize("seed", PLANTED_SEEDS)
def test_planted_inputs_satisfy_the_condition_of_agreement(seed):
    probs, phrases = planted_case(seed)
    assert len(probs) < 400
    for ph in phrases:
        E, ST = ref.tracks(probs, ph)
        offline = sorted((s, e, float(v)) for s, e, v in ref.pick(E, ST, 64, PLANTED_FLOOR))
        assert len(offline) >= 2                                                            # both plants, at the least
        for settle in PLANTED_SETTLE + (10 ** 9,):
            online = sref.online_pick(E, ST, PLANTED_FLOOR, settle)
            assert sref.disjoint_in_time_order(online)
            assert [h[:3] for h in online] == offline, (seed, ph, settle)
