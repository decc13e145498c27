"""Streaming phrase watch on the GPU (dsmi_spot_stream_advance_many, csrc/spot_stream.hip): the tracks of a session laid end to
end against dsmi_spot on the concatenated probabilities on the same device, bit for bit and for five ways of cutting the
utterance; the events against the documented rule (tests/_spot_stream_ref.py, dsmi_spot_watch_pick) on the kernel's own tracks;
many sessions in one call against each alone; refusals, reset, the agreement with the offline search on planted occurrences,
and the recogniser surface on a synthetic streaming model."""
import ctypes

import numpy as np
import pytest

from danspeech_amd import synthetic as syn

import _align_ref as aref
import _spot_ref as ref
import _spot_stream_ref as sref
from test_spot_stream_host import KINDS, PLANTED_FLOOR, PLANTED_SEEDS, PLANTED_SETTLE, planted_case

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
LABELS = syn.DANSPEECH_LABELS
SMALL = ["_", "a", "b", "c", "d"]
LENS = [128, 1, 2, 4, 12, 2, 1, 110, 8, 1]          # groups 255 + 1 | 3 + 7 + 23 + 3 + 1 + 219 | 15 + 1: phrase 1's state 0 is thread 255
FRAMES = [1, 2, 15, 16, 17, 33, 64, 121, 140]       # utterances; 140 frames so that the 128-token phrase ends somewhere
FLOOR = float(np.log(0.05))


@pytest.fixture(scope="module")
def native():
    from danspeech_amd import _native
    return _native


def _phrases(rng, C):
    ph = [[int(x) for x in rng.integers(1, C, size=L)] for L in LENS]
    for p in ph:                                     # the long ones without equal neighbours: 128 tokens fit 140 frames
        for j in range(1, len(p)):
            if len(p) >= 100 and p[j] == p[j - 1]:
                p[j] = p[j] % (C - 1) + 1
    ph[2] = [2, 2]                                  # two equal tokens: needs the blank
    ph[3] = [LABELS.index(c) for c in "alle"] if C == len(LABELS) else [1, 3, 3, 4]      # the skip flag on and off
    ph[5] = [1, 1]
    return ph


def _run(native, watch, P, cuts_list, max_events=64, streams=None, flush_last=True):
    """Sessions out of phase: round r gives session i its r-th chunk (a session that has run out of chunks sits the round out).
    -> per session dict(calls=[(events, counts)], events, E [K, T], ST [K, T]); ``frames()`` is checked after every round."""
    n, K = len(P), watch.K
    own = streams is None
    streams = streams if streams is not None else [native.NativeSpotStream(watch) for _ in range(n)]
    start = [s.frames() for s in streams]
    at = [0] * n
    out = [dict(calls=[], events=[], E=[], ST=[]) for _ in range(n)]
    for r in range(max(len(c) for c in cuts_list)):
        idx = [i for i in range(n) if r < len(cuts_list[i])]
        chunks = [P[i][at[i]:at[i] + cuts_list[i][r]] if cuts_list[i][r] else None for i in idx]
        flush = [flush_last and r == len(cuts_list[i]) - 1 for i in idx]
        res, counts = native.NativeSpotStream.advance_many_counts([streams[i] for i in idx], chunks, flush, max_events, tracks=True)
        for i, (ev, E, ST), c in zip(idx, res, counts):
            at[i] += cuts_list[i][r]
            assert streams[i].frames() == start[i] + at[i]
            assert E.shape == (K, cuts_list[i][r]) and c.shape == (K,)
            out[i]["calls"].append((ev, c))
            out[i]["events"] += ev
            out[i]["E"].append(E), out[i]["ST"].append(ST)
    for i, o in enumerate(out):
        assert at[i] == len(P[i])
        o["E"], o["ST"] = np.concatenate(o["E"], axis=1), np.concatenate(o["ST"], axis=1)
    if own:
        for s in streams:
            s.close()
    return out


def _of_phrase(events, k):
    return [(a, e, lp, fired) for kk, a, e, lp, fired in events if kk == k]


def _check_events(native, o, floor, settle):
    """The events are exactly the documented rule on the kernel's own tracks, firing frames included, in (fired, phrase) order."""
    ev = o["events"]
    for k in range(o["E"].shape[0]):
        want = sref.online_pick(o["E"][k], o["ST"][k], floor, settle)
        assert _of_phrase(ev, k) == want, k
        n, host = native.spot_watch_pick(o["E"][k], o["ST"][k], 0, True, floor, settle, native.SpotPickState.fresh(), max(len(want), 1))
        assert n == len(want) and host == want, k
        assert sref.disjoint_in_time_order(want)
    for events, _ in o["calls"]:
        assert [(h[4], h[0]) for h in events] == sorted((h[4], h[0]) for h in events)


@pytest.fixture(scope="module", params=["small", "danspeech"])
def world(request, native):
    """One decoder, the phrases, utterances on the device and dsmi_spot's tracks of each -- the reference, computed once."""
    labels = SMALL if request.param == "small" else LABELS
    C = len(labels)
    rng = np.random.default_rng(7 if C == 5 else 8)
    dec = native.NativeDecoder(labels, blank_index=0)
    phrases = _phrases(rng, C)
    assert native.spot_plan([len(p) for p in phrases])[0] == 3 and native.spot_plan([len(p) for p in phrases])[2][1] == 255
    probs = [ref.peaky(rng, T, C, 2.0 if C == 5 else 3.0) for T in FRAMES]
    x = np.full((len(probs), max(FRAMES), C), 1.0 / C, dtype=np.float32)
    for b, p in enumerate(probs):
        x[b, :len(p)] = p
    p_dev = torch.from_numpy(x).cuda()
    sizes = np.array(FRAMES, dtype=np.int32)
    _, _, _, E, ST = dec.spot(p_dev, sizes, phrases, native.SPOT_MAX_HITS, FLOOR, tracks=True)
    P = [p_dev[b, :T] for b, T in enumerate(FRAMES)]
    yield dict(dec=dec, C=C, phrases=phrases, probs=probs, P=P, E=E, ST=ST, rng=rng)
    dec.close()


def test_tracks_bit_for_bit_and_events_for_five_chunkings(native, world):
    w = world
    watch = native.NativeSpotWatch(w["dec"], w["phrases"], FLOOR, 5)
    assert (watch.K, watch.n_groups, watch.settle_frames) == (len(LENS), 3, 5)
    B = len(FRAMES)
    cuts = [sref.cuts_of(w["rng"], FRAMES[b], kind) for kind in KINDS for b in range(B)]
    assert any(c[-1] == 0 for c in cuts) and any(0 in c[:-1] for c in cuts)          # a flush with no frames, an empty call
    outs = _run(native, watch, [w["P"][b] for _ in KINDS for b in range(B)], cuts)      # 45 sessions out of phase in every call
    finite = 0
    for j, kind in enumerate(KINDS):
        for b, T in enumerate(FRAMES):
            o = outs[j * B + b]
            assert np.array_equal(o["E"].view(np.int32), w["E"][b, :, :T].view(np.int32)), (kind, b)
            assert np.array_equal(o["ST"], w["ST"][b, :, :T]), (kind, b)
            _check_events(native, o, FLOOR, 5)
            assert o["events"] == outs[b]["events"], (kind, b)                         # identical across the chunkings
    # ... and the numpy reference, held as tests/test_gpu_spot.py holds dsmi_spot to it
    exempt = 0
    for b, p in enumerate(w["probs"]):
        for k, ph in enumerate(w["phrases"]):
            E32, S32 = sref.chunked_tracks(p, ph, sref.cuts_of(w["rng"], len(p), "random"))
            ok = E32 > -np.inf
            E, ST = outs[b]["E"][k], outs[b]["ST"][k]
            assert ((E > -np.inf) == ok).all(), (b, k)
            finite += int(ok.sum())
            assert not ok.any() or float(np.abs(E[ok] - E32[ok]).max()) < 1e-3, (b, k)
            differ = np.nonzero(ST != S32)[0]
            if len(differ):
                E64, S64, MG = ref.tracks(p, ph, dtype=np.float64, margins=True)
                for f in differ:
                    assert ok[f] and MG[f] < 1e-4, (b, k, f, MG[f])
                    r = aref.viterbi(p[ST[f]:f + 1], ph, dtype=np.float64)
                    assert r is not None and abs(float(r["path_logp"]) - E64[f]) < 1e-3, (b, k, f)
                    exempt += 1
    assert finite > 1000 and exempt <= 0.01 * finite
    assert (outs[len(FRAMES) - 1]["E"][0] > -np.inf).any()                              # the 128-token phrase ends somewhere in 140 frames
    assert sum(len(o["events"]) for o in outs[:B]) > 20
    watch.close()


def test_more_events_than_max_events(native, world):
    """settle_frames = 1 and no floor: the one-token phrase fires at every frame.  With max_events = 1 a call stores its first
    event per phrase and counts them all, and the calls after it are what they would have been."""
    w = world
    watch = native.NativeSpotWatch(w["dec"], w["phrases"], -np.inf, 1)
    b = FRAMES.index(64)
    cuts = sref.cuts_of(np.random.default_rng(1), 64, "random")
    full, = _run(native, watch, [w["P"][b]], [cuts])
    one, = _run(native, watch, [w["P"][b]], [cuts], max_events=1)
    _check_events(native, full, -np.inf, 1)
    assert np.array_equal(one["E"].view(np.int32), full["E"].view(np.int32)) and np.array_equal(one["ST"], full["ST"])
    dropped = 0
    for (ev1, c1), (ev, c) in zip(one["calls"], full["calls"]):
        assert np.array_equal(c1, c)
        for k in range(watch.K):
            assert _of_phrase(ev1, k) == _of_phrase(ev, k)[:1] and c[k] == len(_of_phrase(ev, k))
        dropped += int((c > 1).sum())
    assert dropped > 5
    with pytest.raises(native.DsmiError) as e:
        s = native.NativeSpotStream(watch)
        native.NativeSpotStream.advance_many([s], [w["P"][b][:17]], [True], max_events=1)
    assert e.value.code == native.DSMI_ERR_CAPACITY and s.frames() == 17
    s.close()
    watch.close()


def test_many_sessions_in_one_call_equal_each_alone(native, world):
    w = world
    watch = native.NativeSpotWatch(w["dec"], w["phrases"], FLOOR, 3)
    rng = np.random.default_rng(37)
    N = 37
    which = [int(rng.integers(0, len(FRAMES))) for _ in range(N)]
    cuts = [sref.cuts_of(rng, FRAMES[b], "empties" if i % 3 == 0 else "random") for i, b in enumerate(which)]
    cuts = [[0] * (i % 4) + c for i, c in enumerate(cuts)]                              # out of phase: different t0 in one call
    P = [w["P"][b] for b in which]
    together = _run(native, watch, P, cuts)
    for i in range(N):
        alone, = _run(native, watch, [P[i]], [cuts[i]])
        assert alone["events"] == together[i]["events"], i
        assert np.array_equal(alone["E"].view(np.int32), together[i]["E"].view(np.int32)) and np.array_equal(alone["ST"], together[i]["ST"]), i
        assert [c.tolist() for _, c in alone["calls"]] == [c.tolist() for _, c in together[i]["calls"]]
        _check_events(native, together[i], FLOOR, 3)
    watch.close()


def test_reset_starts_a_new_utterance(native, world):
    w = world
    watch = native.NativeSpotWatch(w["dec"], w["phrases"], FLOOR, 4)
    s = native.NativeSpotStream(watch)
    b0, b1 = FRAMES.index(121), FRAMES.index(64)
    _run(native, watch, [w["P"][b0]], [[33, 17, 71]], streams=[s], flush_last=False)      # abandoned mid-utterance, a candidate may be pending
    assert s.frames() == 121
    s.reset()
    assert s.frames() == 0
    again, = _run(native, watch, [w["P"][b1]], [[16, 17, 31]], streams=[s])
    fresh, = _run(native, watch, [w["P"][b1]], [[16, 17, 31]])
    assert again["events"] == fresh["events"] and np.array_equal(again["ST"], fresh["ST"])
    assert np.array_equal(again["E"].view(np.int32), fresh["E"].view(np.int32))
    assert np.array_equal(again["ST"], w["ST"][b1, :, :64])
    s.close()
    watch.close()


def test_refusals_change_nothing(native, world):
    w = world
    L = native.lib()
    dec, C = w["dec"], w["C"]
    watch = native.NativeSpotWatch(dec, w["phrases"][1:4], FLOOR, 2)
    other = native.NativeSpotWatch(dec, w["phrases"][1:4], FLOOR, 2)
    a, b, foreign = native.NativeSpotStream(watch), native.NativeSpotStream(watch), native.NativeSpotStream(other)
    b0 = FRAMES.index(33)
    P = w["P"][b0]
    want, = _run(native, watch, [P], [[10, 7, 16]])
    K, M, F = 3, 2, 12

    def call(ss=(a, b), n=None, probs=(P[:10], P[:7]), frames=(10, 7), flush=(0, 0), M=M, F=F, tracks=True):
        hits, sc = np.full((2, K, 2, 2), 7, np.int32), np.full((2, K, 2), 7.5, np.float32)
        fi, cn = np.full((2, K, 2), 7, np.int32), np.full((2, K), 7, np.int32)
        E, ST = np.full((2, K, 12), 7.5, np.float32), np.full((2, K, 12), 7, np.int32)
        hs = (ctypes.c_void_p * len(ss))(*[None if s is None else s._h for s in ss])
        ps = None if probs is None else (ctypes.c_void_p * len(probs))(*[None if p is None else p.data_ptr() for p in probs])
        rc = L.dsmi_spot_stream_advance_many(hs, len(ss) if n is None else n, ps, native._np_ptr(np.array(frames, np.int32)),
                                             native._np_ptr(np.array(flush, np.int32)), M, native._np_ptr(hits), native._np_ptr(sc),
                                             native._np_ptr(fi), native._np_ptr(cn), native._np_ptr(E) if tracks else None,
                                             native._np_ptr(ST) if tracks else None, F, None)
        untouched = all((x == v).all() for x, v in ((hits, 7), (sc, 7.5), (fi, 7), (cn, 7), (E, 7.5), (ST, 7)))
        return rc, untouched, L.dsmi_spot_stream_last_error(None).decode()

    INV, CAP = native.DSMI_ERR_INVALID, native.DSMI_ERR_CAPACITY
    refused = [
        (dict(ss=(a, None)), INV, "spot stream 1: null handle"),
        (dict(ss=(a, a)), INV, "spot stream 1: the same handle appears twice in one call"),
        (dict(ss=(a, foreign)), INV, "spot stream 1: the streams of one call must belong to one watch"),
        (dict(frames=(10, -1)), INV, "spot stream 1: negative frame count"),
        (dict(probs=(P[:10], None)), INV, "spot stream 1: no probabilities for 7 frames"),
        (dict(probs=None), INV, "spot stream 0: no probabilities for 10 frames"),
        (dict(M=0), INV, "spot stream: max_events outside 1 .. DSMI_SPOT_MAX_HITS (64)"),
        (dict(M=native.SPOT_MAX_HITS + 1), INV, "spot stream: max_events outside 1 .. DSMI_SPOT_MAX_HITS (64)"),
        (dict(F=9), INV, "spot stream 0: F_stride is below the frame count"),
        (dict(F=-1), INV, "spot stream: negative F_stride"),
        (dict(F=2 ** 27), CAP, "spot stream: n * K * F_stride exceeds 2^27 (the tracks)"),
        (dict(n=0), INV, "bad spot stream arguments"),
    ]
    for step in range(3):                        # before the first chunk, between chunks, before the flush
        for kw, code, text in refused:
            rc, untouched, msg = call(**kw)
            assert (rc, untouched, msg) == (code, True, text), (kw, rc, msg)
        assert a.frames() == [0, 10, 17][step] and b.frames() == 0
        cut = [10, 7, 16][step]
        ev, E, ST = native.NativeSpotStream.advance_many([a], [P[a.frames():a.frames() + cut]], [step == 2], 64, tracks=True)[0]
        assert ev == want["calls"][step][0]
        assert np.array_equal(E.view(np.int32), want["E"][:, a.frames() - cut:a.frames()].view(np.int32))
    rc, untouched, _ = call(ss=(b, a), frames=(10, 0), probs=(P[:10], None), flush=(0, 1))
    assert rc == 0 and not untouched and b.frames() == 10 and a.frames() == 33
    with pytest.raises(native.DsmiError) as e:
        native.NativeSpotWatch(dec, [[1, 0]], FLOOR, 2)
    assert e.value.code == INV and "is the blank or not a label" in e.value.msg
    for bad, code in ((dict(settle=0), INV), (dict(floor=float("nan")), INV), (dict(ids=[[1] * 129]), CAP), (dict(ids=[[C]]), INV)):
        with pytest.raises(native.DsmiError) as e:
            native.NativeSpotWatch(dec, bad.get("ids", [[1]]), bad.get("floor", FLOOR), bad.get("settle", 2))
        assert e.value.code == code and e.value.msg.startswith("spot watch"), bad
    for s in (a, b, foreign):
        s.close()
    watch.close(), other.close()


@pytest.mark.parametrize("seed", PLANTED_SEEDS)
def test_planted_occurrences_agree_with_the_offline_search(native, seed):
    """The inputs of tests/test_spot_stream_host.py::test_planted_inputs_satisfy_the_condition_of_agreement."""
    probs, phrases = planted_case(seed)
    dec = native.NativeDecoder(LABELS, blank_index=0)
    p_dev = torch.from_numpy(probs).cuda()
    hits, scores, counts = dec.spot(p_dev[None], None, phrases, 64, PLANTED_FLOOR)
    rng = np.random.default_rng(seed)
    for settle in PLANTED_SETTLE:
        watch = native.NativeSpotWatch(dec, phrases, PLANTED_FLOOR, settle)
        o, = _run(native, watch, [p_dev], [sref.cuts_of(rng, len(probs), "random")])
        for k in range(len(phrases)):
            offline = sorted((int(hits[0, k, n, 0]), int(hits[0, k, n, 1]), float(scores[0, k, n])) for n in range(counts[0, k]))
            assert len(offline) >= 2 and [h[:3] for h in _of_phrase(o["events"], k)] == offline, (seed, settle, k)
        watch.close()
    dec.close()


# ---- the surface, on the synthetic streaming model of tests/test_gpu_stream_sessions.py
def _stream_model(name, H, L, ctx, seed):
    from danspeech_amd.deepspeech.model import DeepSpeech
    sd = syn.make_state_dict(2, "gru", H, L, bidirectional=False, context=ctx, seed=seed, fc_gain=8.0)
    return DeepSpeech(name, rnn_type="gru", rnn_hidden_size=H, rnn_layers=L, conv_layers=2, context=ctx, bidirectional=False,
                      streaming_inference_model=True).load_state_dict(sd)


def test_surface_detections_and_unchanged_texts(native, monkeypatch):
    from danspeech_amd import Recognizer
    m = _stream_model("stream-watch", 64, 2, 20, seed=99)
    audio = [syn.make_clip(20 + i, 16000 + 5311 * i) for i in range(5)]
    made = []
    for cls in (native.NativeSpotWatch, native.NativeSpotStream):
        init = cls.__init__
        monkeypatch.setattr(cls, "__init__", lambda self, *a, _init=init, **k: (made.append(type(self).__name__), _init(self, *a, **k))[1])
    rec = Recognizer()
    rec.enable_real_time_streaming(streaming_model=m)
    plain = list(rec.stream_recordings(audio, chunk_samples=1024))
    quiet = np.random.RandomState(5).randint(-30, 31, size=8000 + 20800).astype(np.float64)
    sources = [np.concatenate((quiet[:8000], a, quiet[8000:])).astype(np.int16) for a in audio[:2]]      # a burst the gate opens and closes on
    sources = [[x[i:i + 4000] for i in range(0, len(x), 4000)] for x in sources]
    live_plain = list(rec.stream_live(sources))
    assert made == [] and rec.danspeech_recognizer.take_detections() == []            # watch=None: no spot handles
    words = sorted(set(t[i:i + 2] for _, last, t in plain if last for i in range(len(t) - 1) if " " not in t[i:i + 2]))[:6]
    assert words
    with pytest.raises(ValueError):
        rec.enable_real_time_streaming(streaming_model=m, watch=["ok", "nr #1"])
    rec.enable_real_time_streaming(streaming_model=m, watch=words, watch_confidence=0.02, watch_settle_s=0.1)
    eng = rec.danspeech_recognizer
    settle = eng._watch_spec[3]
    assert settle == max(1, round(0.1 / eng.frame_seconds()))
    fed = {}                                                                            # stream handle -> [(rows, flush)] per utterance
    advance = native.NativeSpotStream.advance_many_counts

    def recording(streams, probs_list, flush, *a, **k):
        for s, p, f in zip(streams, probs_list, flush):
            fed.setdefault(id(s), [[]])[-1].append(None if p is None else p.reshape(-1, p.shape[-1]).clone())
            if f:
                fed[id(s)].append([])
        return advance(streams, probs_list, flush, *a, **k)
    monkeypatch.setattr(native.NativeSpotStream, "advance_many_counts", staticmethod(recording))
    heard = []
    watched = list(rec.stream_recordings(audio, chunk_samples=1024, on_detection=lambda *d: heard.append(d)))
    assert watched == plain                                                             # what is yielded is untouched
    assert made.count("NativeSpotWatch") == 1 and made.count("NativeSpotStream") == len(audio)
    # the detections: dsmi_spot's tracks of each session's concatenated outputs, then the rule
    dec = native.NativeDecoder(LABELS, blank_index=0)
    ids = eng._watch_spec[1]
    frame_s = eng.frame_seconds()
    want = []
    for utterances in fed.values():
        for ordinal, parts in enumerate(utterances):
            rows = [p for p in parts if p is not None]
            if not rows:
                continue
            x = torch.cat(rows)
            _, _, _, E, ST = dec.spot(x[None], None, ids, 1, float(np.log(0.02)), tracks=True)
            for k in range(len(ids)):
                for a, e, lp, fired in sref.online_pick(E[0, k], ST[0, k], float(np.log(0.02)), settle):
                    want.append((ordinal, words[k], a * frame_s, e * frame_s, float(np.exp(lp / (e - a))), lp))
    assert len(heard) >= 1 and sorted(h[1:] for h in heard) == sorted(want)
    assert all(0 <= h[0] < len(audio) and h[3] < h[4] and 0.02 * (1 - 1e-6) <= h[5] <= 1 for h in heard)
    live_heard = []
    assert list(rec.stream_live(sources, on_detection=lambda *d: live_heard.append(d))) == live_plain
    assert all(h[0] in (0, 1) for h in live_heard)
    dec.close()
    rec.disable_real_time_streaming()
