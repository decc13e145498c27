"""GPU: ``dsmi_endpointer_push_many`` -- the live gate's kernels and its host state machine together -- against the golden yields
of the reference's ``listen_stream`` (tests/golden/g14_listen.json) and against itself under every cutting of a stream."""
import audioop
import json
import os

import numpy as np
import pytest

import _listen_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = json.load(open(os.path.join(HERE, "golden", "g14_listen.json")))["cases"]


@pytest.fixture(scope="module")
def fe():
    from danspeech_amd import _native
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    f = _native.NativeFrontend()
    yield f
    f.close()


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _collect(segs):
    """One session's segments -> (closed utterances, open rest) as float64 arrays."""
    done, cur = [], []
    for t, last in segs:
        cur.append(t.cpu().numpy())
        if last:
            done.append(np.concatenate(cur))
            cur = []
    return done, (np.concatenate(cur) if cur else np.zeros(0))


def _run(ep, x, cuts, eos=True):
    """Pushes x[cuts[k]:cuts[k+1]] one after the other -> (closed utterances, open rest, energies)."""
    segs, en = [], []
    edges = [0] + list(cuts) + [len(x)]
    for k in range(len(edges) - 1):
        s, e = ep.push(_dev(x[edges[k]:edges[k + 1]]), end_of_stream=eos and k == len(edges) - 2, return_energies=True)
        segs += s
        en += list(e)
    done, rest = _collect(segs)
    return done, rest, en


def _same(a, b):
    return len(a[0]) == len(b[0]) and all(np.array_equal(u, v) for u, v in zip(a[0], b[0])) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_golden_cases_in_one_push(fe, case):
    from danspeech_amd import _native
    x = R.make_stream(case["recipe"], case["channels"])
    mono = R.fold_stereo(x).astype(np.float64)
    ep = _native.NativeEndpointer(fe, case["chunk"], case["rate"], channels=case["channels"], **(case["params"] or {}))
    done, rest, en = _run(ep, x, [])
    want, open_rest = R.utterances(case["yields"])
    assert open_rest == [] and len(rest) == 0 and len(done) == len(want) == case["n_last"]
    for u, idx in zip(done, want):
        assert np.array_equal(u, mono[idx])
    assert en == R.energies(R.fold_stereo(x), case["chunk"])
    assert ep.position() == (len(x), case["n_last"], 0)
    ep.close()


def _stream(seed, n, chunk):
    """Two bursts in quiet noise, sized in buffers of `chunk` so that every chunk size sees a closed utterance within n samples."""
    rng = np.random.RandomState(seed)
    x = rng.randint(-60, 61, size=n).astype(np.int16)
    pn, hn, kn = R.buffer_counts(chunk, 16000, pause_threshold=0.2, phrase_threshold=0.05, non_speaking_duration=0.1)
    a = (kn + 1) * chunk + 37
    b = a + (hn + 2) * chunk
    x[a:b] = rng.randint(-3000, 3001, size=len(x[a:b]))
    c = b + (pn + 2) * chunk + 11
    x[c:c + (hn + 1) * chunk] = rng.randint(-3000, 3001, size=len(x[c:c + (hn + 1) * chunk]))
    return x


FAST = dict(pause_threshold=0.2, phrase_threshold=0.05, non_speaking_duration=0.1)


@pytest.mark.parametrize("chunk", [256, 1024, 4096])
@pytest.mark.parametrize("kind", ["int16", "stereo", "float32", "float64"])
def test_cut_independence(fe, kind, chunk):
    from danspeech_amd import _native
    n = 32000 - 123
    x = _stream(chunk + len(kind), n, chunk)
    if kind == "stereo":
        y = np.stack([x, np.roll(x, 1) * 11], axis=1).astype(np.int16)      # the loud parts saturate the fold
        mk = dict(channels=2)
    elif kind == "int16":
        y, mk = x, {}
    else:
        y = (x.astype(np.float64) + np.random.RandomState(1).uniform(-0.49, 0.49, size=n)).astype(kind)
        mk = dict(dtype=np.dtype(kind))
    ep = _native.NativeEndpointer(fe, chunk, 16000, **FAST, **mk)
    whole = _run(ep, y, [])
    assert len(whole[0]) >= 2
    rng = np.random.RandomState(chunk)
    cuttings = {
        "random": sorted(rng.randint(0, n + 1, size=9)),
        "empty_pushes": sorted(list(rng.randint(0, n + 1, size=5)) * 3),
        "chunk_minus_1": list(range(chunk - 1, n, chunk - 1)),
        "chunk_plus_1": list(range(chunk + 1, n, chunk + 1)),
    }
    for name, cuts in cuttings.items():
        ep.reset()
        got = _run(ep, y, cuts)
        assert _same(got, whole), name
        assert got[2] == whole[2], name
    ep.close()


@pytest.mark.parametrize("kind", ["int16", "stereo", "float32", "float64"])
def test_every_sample_its_own_push(fe, kind):
    from danspeech_amd import _native
    n = 3200                                                              # 0.2 s
    x = _stream(3, n, 16)[:n]
    x[200:1500] = np.random.RandomState(2).randint(-3000, 3001, size=1300)
    if kind == "stereo":
        y, mk = np.stack([x, x], axis=1), dict(channels=2)
    elif kind == "int16":
        y, mk = x, {}
    else:
        y, mk = (x + 0.25).astype(kind), dict(dtype=np.dtype(kind))
    ep = _native.NativeEndpointer(fe, 64, 16000, pause_threshold=0.02, phrase_threshold=0.01, non_speaking_duration=0.01, **mk)
    whole = _run(ep, y, [])
    assert len(whole[0]) >= 2
    ep.reset()
    assert _same(_run(ep, y, list(range(1, n))), whole)
    ep.close()


def _mixed(fe, n_sessions):
    """Sessions that differ in type, chunk, threshold and phase -> [(make, stream, cuts)]"""
    from danspeech_amd import _native
    out = []
    for i in range(n_sessions):
        chunk = [256, 1024, 4096, 160][i % 4]
        kind = ["int16", "stereo", "float32", "float64"][(i // 4) % 4]
        n = 9000 + 701 * (i % 7)
        x = _stream(100 + i, n, chunk)
        if kind == "stereo":
            y, mk = np.stack([x, x // 2], axis=1), dict(channels=2)
        elif kind == "int16":
            y, mk = x, {}
        else:
            y, mk = (x + 0.3).astype(kind), dict(dtype=np.dtype(kind))
        make = lambda chunk=chunk, mk=mk, i=i: _native.NativeEndpointer(fe, chunk, 16000, energy_threshold=[1000, 400, 1500][i % 3], **FAST, **mk)
        cuts = sorted(np.random.RandomState(i).randint(0, n + 1, size=2))      # three rounds, each session at its own phase
        out.append((make, y, cuts))
    return out


@pytest.mark.parametrize("n_sessions", [37, 256])
def test_many_sessions_equal_each_alone(fe, n_sessions):
    from danspeech_amd import _native
    sessions = _mixed(fe, n_sessions)
    eps = [make() for make, _, _ in sessions]
    segs = [[] for _ in sessions]
    for r in range(3):
        pcms, eos = [], []
        for (_, y, cuts), ep in zip(sessions, eps):
            edges = [0] + list(cuts) + [len(y)]
            pcms.append(_dev(y[edges[r]:edges[r + 1]]))
            eos.append(r == 2 and len(y) % 2 == 0)                           # some end, some stay open
        got = _native.NativeEndpointer.push_many(eps, pcms, eos)
        for k, g in enumerate(got):
            segs[k] += g
    for k, (make, y, _) in enumerate(sessions):                              # every session alone, in one push
        ep = make()
        want = _run(ep, y, [], eos=len(y) % 2 == 0)
        assert _same(_collect(segs[k]), want[:2]), k
        assert ep.position() == eps[k].position(), k
        ep.close()
    assert sum(len(_collect(s)[0]) for s in segs) >= n_sessions // 2         # utterances were closed, not only silence carried
    for ep in eps:
        ep.close()


def test_float_samples_are_gated_rounded_and_forwarded_unrounded(fe):
    from danspeech_amd import _native
    chunk = 256
    # rounded to 1000 the buffer's rms is exactly the threshold (quiet); rounded to 1001 it is above it
    quiet = np.full(10 * chunk, 1000.4)
    loud = np.full(6 * chunk, 1000.6)
    x = np.concatenate([quiet, loud, np.full(20 * chunk, 0.3), [40000.0, -40000.0, 0.5, 1.5, 2.5]])
    ep = _native.NativeEndpointer(fe, chunk, 16000, dtype=np.float64, **FAST)
    done, rest, en = _run(ep, x, [])
    ints = np.clip(np.rint(x), -32768, 32767).astype(np.int16)
    assert en == R.energies(ints, chunk)
    assert en[:10] == [1000] * 10 and en[10:16] == [1001] * 6 and en[-1] == audioop.rms(ints[-5:].tobytes(), 2)
    want, _ = R.utterances(R.listen(ints, chunk, 16000, **FAST))
    assert len(done) == len(want) == 2
    for u, idx in zip(done, want):
        assert np.array_equal(u, x[idx])
    assert (done[0] != np.rint(done[0])).all()
    ep.close()


def test_refusals_leave_everything_unchanged_and_reset_starts_afresh(fe):
    from danspeech_amd import _native
    import ctypes as C
    L = _native.lib()
    x = _stream(9, 20000, 256)
    a = _native.NativeEndpointer(fe, 256, 16000, **FAST)
    b = _native.NativeEndpointer(fe, 1024, 16000, **FAST)
    fe2 = _native.NativeFrontend()
    c = _native.NativeEndpointer(fe2, 256, 16000, **FAST)
    want_a, want_b = _run(a, x, []), _run(b, x, [])
    a.reset(); b.reset()
    assert a.position() == (0, 0, 0)
    first = _native.NativeEndpointer.push_many([a, b], [_dev(x[:7000]), _dev(x[:5000])], [False, False])
    pos = (a.position(), b.position())
    d = _dev(x[7000:])
    out = torch.full((30000,), -7.0, dtype=torch.float64, device="cuda")

    def call(hs, ptrs, ns, eos, cap_out=30000, cap_seg=400, n=None):
        n = len(hs) if n is None else n
        H = (C.c_void_p * max(len(hs), 1))(*[h._h for h in hs])
        P = (C.c_void_p * max(len(hs), 1))(*ptrs)
        ns = np.array(ns, dtype=np.int64); eos = np.array(eos, dtype=np.int32)
        ss = np.zeros(400, dtype=np.int32); sl = np.zeros(400, dtype=np.int64); sla = np.zeros(400, dtype=np.int32)
        found = C.c_int(-5)
        rc = L.dsmi_endpointer_push_many(H, n, P, ns.ctypes.data, eos.ctypes.data, out.data_ptr(), cap_out, ss.ctypes.data, sl.ctypes.data,
                                         sla.ctypes.data, cap_seg, C.byref(found), None, None)
        return rc, (L.dsmi_endpointer_last_error(None) or b"").decode()

    p = d.data_ptr()
    refusals = [
        (call([a, b], [p, p], [10, 10], [0, 0], n=0), _native.DSMI_ERR_INVALID, "number of sessions"),
        (call([a, b], [p, p], [10, 10], [0, 0], n=257), _native.DSMI_ERR_INVALID, "number of sessions"),
        (call([a, a], [p, p], [10, 10], [0, 0]), _native.DSMI_ERR_INVALID, "session 1"),
        (call([a, c], [p, p], [10, 10], [0, 0]), _native.DSMI_ERR_INVALID, "session 1"),
        (call([a, b], [p, p], [10, -1], [0, 0]), _native.DSMI_ERR_INVALID, "session 1"),
        (call([a, b], [p, p], [13000, 13000], [0, 0], cap_out=13000), _native.DSMI_ERR_CAPACITY, "out_dev"),
        (call([a, b], [p, p], [13000, 13000], [0, 0], cap_seg=3), _native.DSMI_ERR_CAPACITY, "max_segments"),
    ]
    for (rc, text), code, word in refusals:
        assert rc == code and word in text, (rc, text, word)
    torch.cuda.synchronize()
    assert (a.position(), b.position()) == pos and bool((out == -7.0).all())
    rest = _native.NativeEndpointer.push_many([a, b], [d, _dev(x[5000:])], [True, True])
    assert _same(_collect(first[0] + rest[0]), want_a[:2]) and _same(_collect(first[1] + rest[1]), want_b[:2])
    # samples after end_of_stream are refused until the session is reset; an empty push is nothing
    assert a.push(None) == []
    rc, text = call([b, a], [p, p], [10, 10], [0, 0])
    assert rc == _native.DSMI_ERR_INVALID and "session 0" in text and "end_of_stream" in text
    with pytest.raises(_native.DsmiError):
        a.push(d)
    a.reset()
    assert a.position() == (0, 0, 0) and _same(_run(a, x, [333]), want_a)
    for h in (a, b, c):
        h.close()
    fe2.close()
    # sample types the gate cannot match exactly are refused at creation
    for dt in (3, 4, 5):
        with pytest.raises(_native.DsmiError) as ei:
            _native.NativeEndpointer(fe, 1024, 16000, pcm_dtype=dt)
        assert ei.value.code == _native.DSMI_ERR_INVALID
    for chunk in (15, 65537):
        with pytest.raises(_native.DsmiError):
            _native.NativeEndpointer(fe, chunk, 16000)
