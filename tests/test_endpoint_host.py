"""CPU: the live gate's host half.  tests/golden/g14_listen.json holds what the reference's ``Recognizer.listen_stream`` yielded
over seeded streams (tools/gen_golden_listen.py executed it); ``tests/_listen_ref.py`` restates the generator and must reproduce
every case exactly; the library's ``dsmi_endpoint_gate`` is then held to the restatement on those cases and on random energy
sequences fed in random splits; ``stream_plan.LivePasses`` is held to a transcription of ``real_time_streaming``'s pass rule."""
import json
import math
import os

import numpy as np
import pytest

import _listen_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
G14 = json.load(open(os.path.join(HERE, "golden", "g14_listen.json")))
CASES = G14["cases"]


def _mono(case):
    return R.fold_stereo(R.make_stream(case["recipe"], case["channels"]))


def gate_whole(energy_or_sums, lens, chunk, rate, params, splits, from_sums):
    """The library's gate over a stream of buffers fed in runs ending at ``splits`` -> yields [(is_last, start, count)] in samples."""
    from danspeech_amd import _native
    p = dict(R.DEFAULTS, **(params or {}))
    pn, hn, kn = _native.endpoint_counts(chunk, rate, p["pause_threshold"], p["phrase_threshold"], p["non_speaking_duration"], p["energy_threshold"])
    assert (pn, hn, kn) == R.buffer_counts(chunk, rate, **p)
    sums = np.asarray(energy_or_sums, dtype=np.uint64) if from_sums else np.array([int(e) * int(e) * int(l) for e, l in zip(energy_or_sums, lens)], dtype=np.uint64)
    lens = np.asarray(lens, dtype=np.int64)
    starts = np.concatenate(([0], np.cumsum(lens)))
    state = np.zeros(4, dtype=np.int64)
    out, lo = [], 0
    energies = []
    cuts = list(splits) + [len(sums)]
    for k, hi in enumerate(cuts):
        ev, e = _native.endpoint_gate(p["energy_threshold"], pn, hn, kn, state, sums[lo:hi], lens[lo:hi], end_of_stream=(k == len(cuts) - 1))
        energies += list(e)
        for first, count, last in ev:
            a, b = lo + first, lo + first + count
            assert 0 <= a <= b <= len(sums)
            out.append((bool(last), int(starts[a]), int(starts[b] - starts[a])))
        lo = hi
    return out, energies


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_reproduces_the_reference(case):
    x = _mono(case)
    assert len(x) == case["n_samples"] <= 6 * case["rate"]
    got = R.listen(x, case["chunk"], case["rate"], **(case["params"] or {}))
    assert [list(map(int, y)) for y in got] == case["yields"]


def test_golden_holds_the_cases_it_must():
    names = " ".join(c["name"] for c in CASES)
    for word in ("silence_only", "speech_in_first_buffer", "too_short_then_real", "pause_of_pause_n_c", "pause_of_pause_n_plus_1", "rms_equals_threshold",
                 "rms_threshold_plus_1", "ends_mid_phrase_short_buffer", "three_utterances", "stereo_fold_saturates", "second_parameters"):
        assert word in names
    by = {c["name"]: c for c in CASES}
    assert by["pause_of_pause_n_c1024"]["n_last"] == 2 and by["pause_of_pause_n_plus_1_c1024"]["n_last"] == 3
    assert by["rms_equals_threshold_c256"]["n_last"] == 1 and len(by["rms_equals_threshold_c256"]["yields"]) == 2
    assert by["three_utterances_c256"]["n_last"] == 4
    assert {c["chunk"] for c in CASES} == {256, 1024, 4096} and {c["source"] for c in CASES} == {"file", "bytes"}
    x = R.make_stream(by["stereo_fold_saturates_c4096"]["recipe"], 2).astype(np.int64).sum(axis=1)
    assert (x > 32767).any() and (x < -32768).any()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_host_gate_reproduces_the_restatement_on_the_golden_streams(case):
    x = _mono(case).astype(np.int64)
    chunk = case["chunk"]
    lens = [len(x[k:k + chunk]) for k in range(0, len(x), chunk)]
    sums = [int((x[k:k + chunk] ** 2).sum()) for k in range(0, len(x), chunk)]
    want = R.utterances(case["yields"])
    rng = np.random.RandomState(len(x))
    for splits in ([], sorted(rng.randint(0, len(sums) + 1, size=5)), list(range(len(sums) + 1))):
        got, e = gate_whole(sums, lens, chunk, case["rate"], case["params"], splits, True)
        assert R.utterances(got) == want
        assert e == R.energies(_mono(case), chunk)


def test_host_gate_on_random_energy_sequences_in_random_splits():
    rng = np.random.RandomState(14)
    for trial in range(200):
        chunk = int(rng.choice([256, 1024, 4096, 160, 1000]))
        rate = int(rng.choice([16000, 8000, 44100]))
        params = dict(energy_threshold=float(rng.choice([1000, 300, 999.5])), pause_threshold=float(rng.choice([0.8, 0.3, 0.1])),
                      phrase_threshold=float(rng.choice([0.3, 0.05, 0.0])), non_speaking_duration=float(rng.choice([0.35, 0.1, 0.0])))
        if params["non_speaking_duration"] > params["pause_threshold"]:
            params["non_speaking_duration"] = params["pause_threshold"]
        nb = int(rng.randint(0, 120))
        # runs of loud and quiet buffers of random lengths, energies on both sides of and at the threshold
        e = []
        while len(e) < nb:
            loud = rng.rand() < 0.5
            run = int(rng.randint(1, 3 * R.buffer_counts(chunk, rate, **params)[0] + 3))
            t = int(params["energy_threshold"])
            e += [int(rng.choice([t + 1, t + 500, 30000]) if loud else rng.choice([0, t, max(t - 1, 0)])) for _ in range(run)]
        e = e[:nb]
        lens = [chunk] * nb
        if nb and rng.rand() < 0.5:
            lens[-1] = int(rng.randint(1, chunk))
        want = R.listen(np.zeros(sum(lens), dtype=np.int16), chunk, rate, energy=e, **params)
        # (listen counts a short final buffer by the stream's length)
        splits = sorted(rng.randint(0, nb + 1, size=int(rng.randint(0, 6))))
        got, energies = gate_whole(e, lens, chunk, rate, params, splits, False)
        assert energies == e, trial
        assert R.utterances(got) == R.utterances(want), (trial, chunk, rate, params)


def test_host_gate_joins_buffers_and_bounds_its_events():
    from danspeech_amd import _native
    state = np.zeros(4, dtype=np.int64)
    pn, hn, kn = _native.endpoint_counts(1024, 16000)
    assert (pn, hn, kn) == (13, 5, 6)
    loud, quiet = 2000 * 2000 * 1024, 0
    sums = [quiet] * 8 + [loud] * 6 + [quiet] * 14
    ev, e = _native.endpoint_gate(1000, pn, hn, kn, state, sums, [1024] * len(sums))
    # the six kept buffers and the phrase up to the breaking buffer: one run of buffers with the last mark
    assert ev.tolist() == [[3, 25, 1]] and list(state) == [0, 0, 0, 0]
    assert list(e[:9]) == [0] * 8 + [2000]
    # kept buffers from an earlier run: a negative first_buffer
    state[:] = 0
    ev, _ = _native.endpoint_gate(1000, pn, hn, kn, state, [quiet] * 4, [1024] * 4)
    assert len(ev) == 0 and list(state) == [0, 4, 0, 0]
    ev, _ = _native.endpoint_gate(1000, pn, hn, kn, state, [quiet, loud, loud], [1024] * 3)
    assert ev.tolist() == [[-4, 7, 0]] and list(state) == [1, 0, 1, 0]
    ev, _ = _native.endpoint_gate(1000, pn, hn, kn, state, [], [], end_of_stream=True)
    assert ev.tolist() == [[0, 0, 1]] and list(state) == [0, 0, 0, 0]
    # every buffer breaks (pause_n = 0, phrase_n = 0): the worst case of n_buffers + 1 events is reached, never passed
    state[:] = 0
    n = 9
    ev, _ = _native.endpoint_gate(1000, 0, 0, 1, state, [loud, quiet] * n, [1024] * (2 * n), end_of_stream=True)
    assert len(ev) == n + 1 <= 2 * n + 1


def test_host_refusals():
    from danspeech_amd import _native
    L = _native.lib()
    state = np.zeros(4, dtype=np.int64)
    ok = dict(state=state, sums=[1], lens=[16])
    with pytest.raises(_native.DsmiError):
        _native.endpoint_gate(1000, -1, 5, 6, **ok)
    with pytest.raises(_native.DsmiError):
        _native.endpoint_gate(float("nan"), 13, 5, 6, **ok)
    with pytest.raises(_native.DsmiError):
        _native.endpoint_gate(1000, 13, 5, 6, state, [1], [0])                     # an empty buffer is not a buffer
    with pytest.raises(_native.DsmiError):
        _native.endpoint_gate(1000, 13, 5, 6, np.array([2, 0, 0, 0], dtype=np.int64), [1], [16])
    with pytest.raises(_native.DsmiError) as ei:
        _native.endpoint_gate(1000, 0, 0, 1, state.copy(), [10 ** 9, 0] * 3, [16] * 6, max_events=2)
    assert ei.value.code == _native.DSMI_ERR_CAPACITY
    assert list(state) == [0, 0, 0, 0]
    for bad in (dict(chunk=15), dict(chunk=65537), dict(rate=0), dict(pause_threshold=0.2, non_speaking_duration=0.35), dict(non_speaking_duration=-0.1)):
        with pytest.raises(_native.DsmiError):
            _native.endpoint_counts(**dict(dict(chunk=1024, rate=16000), **bad))
    for dt in (3, 4, 5, 1 | 16, 3 | 16):            # U8, I24, I32, stereo float, stereo U8
        with pytest.raises(_native.DsmiError):
            _native.endpoint_counts(1024, 16000, pcm_dtype=dt)
    # create refuses a bad desc before it looks at the frontend (no device is touched)
    import ctypes as C
    d = _native.EndpointerDesc(1024, 16000, 3, 1000.0, 0.8, 0.3, 0.35)
    h = C.c_void_p()
    assert L.dsmi_endpointer_create(None, C.byref(d), C.byref(h)) == _native.DSMI_ERR_INVALID
    assert b"8-bit" in L.dsmi_endpointer_last_error(None)
    assert L.dsmi_endpointer_push_many(None, 1, None, None, None, None, 0, None, None, None, 0, None, None, None) == _native.DSMI_ERR_INVALID
    assert L.dsmi_endpointer_position(None, None, None, None) == _native.DSMI_ERR_INVALID
    assert L.dsmi_endpointer_reset(None) == _native.DSMI_ERR_INVALID


def test_counts_are_the_references_float_arithmetic():
    from danspeech_amd import _native
    for chunk in (16, 160, 256, 1000, 1024, 4096, 65536):
        for rate in (8000, 11025, 16000, 44100, 48000):
            for p in ((0.8, 0.3, 0.35), (0.5, 0.2, 0.2), (0.064, 0.064, 0.064), (0.3, 0.0, 0.0)):
                spb = float(chunk) / rate
                want = tuple(int(math.ceil(v / spb)) for v in p)
                assert _native.endpoint_counts(chunk, rate, *p) == want


def test_live_passes_against_the_transcription():
    from danspeech_amd.stream_plan import LivePasses, live_requirements
    rng = np.random.RandomState(5)
    for context in (20, 4):
        first, general = R.pass_requirements(context, 16000)
        assert live_requirements(context, 16000) == (first, general)
        for trial in range(60):
            # scripted arrivals: segments of random lengths, last marks now and then (some before a first pass is possible),
            # dealt into rounds of random sizes (empty rounds among them)
            rounds, pos = [], 0
            for _ in range(int(rng.randint(1, 12))):
                arrivals = []
                for _ in range(int(rng.randint(0, 5))):
                    n = int(rng.choice([0, 256, 1024, 4096, 7000, 12000]))
                    arrivals.append((bool(rng.rand() < 0.25), np.arange(pos, pos + n)))
                    pos += n
                rounds.append(arrivals)
            want = R.passes(rounds, first, general)
            lp = LivePasses(context, 16000)
            for arrivals, w in zip(rounds, want):
                got = lp.feed([(s, l) for l, s in arrivals])
                assert [(f, l) for _, f, l in got] == [(f, l) for _, f, l in w]
                for (parts, _, _), (data, _, _) in zip(got, w):
                    assert np.array_equal(np.concatenate(parts) if parts else np.zeros(0), data)
    # the rule itself, on a script: too little, the first pass, a general pass, the last mark, then a discarded utterance whose
    # samples stand in front of the next one's (Recognizer.py:668-669 clears nothing)
    first, general = R.pass_requirements(20, 16000)
    assert (first, general) == (8640, 6240)
    lp = LivePasses(20, 16000)
    a = np.arange
    assert lp.feed([(a(8000), False)]) == []
    got = lp.feed([(a(640), False)])
    assert [(sum(map(len, p)), f, l) for p, f, l in got] == [(8640, True, False)]
    assert lp.feed([(a(6239), False)]) == []
    assert [(sum(map(len, p)), f, l) for p, f, l in lp.feed([(a(1), False)])] == [(6240, False, False)]
    assert [(sum(map(len, p)), f, l) for p, f, l in lp.feed([(a(10), True), (a(100), True), (a(8540), False)])] == [(10, False, True), (8640, True, False)]
