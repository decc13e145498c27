"""Chunked sample-rate conversion, the host side (no GPU): the numpy restatement of the chunked algorithm
(tests/_resample_stream_ref.py: tail, ready count, flush) against the whole-signal reference of tests/_resample_ref.py, exactly;
against ``audioop.ratecv`` with its carried state where it imports; ``dsmi_resample_ready`` and the pure-Python schedule of
``danspeech_amd/stream_plan.py`` against brute force; the creation refusals that need no device."""
import ctypes as C

import numpy as np
import pytest

import _resample_ref as R
import _resample_stream_ref as S

RATES = (8000, 11025, 16001, 22050, 44100, 48000, 96000)
METHOD_NAME = {R.POLYPHASE: "polyphase", R.RATECV: "ratecv"}


def _run(ref, x, sizes):
    """Push ``x`` in chunks of ``sizes``; every push but the flush brings what the package's own schedule arithmetic
    (``stream_plan.resample_ready``, the Python twin of ``dsmi_resample_ready``) says is final by then."""
    from danspeech_amd import stream_plan as sp
    outs, pos, emitted = [], 0, 0
    for m, s in enumerate(sizes):
        last = m == len(sizes) - 1
        outs.append(ref.push(x[pos:pos + s], is_last=last))
        pos += s
        emitted += len(outs[-1])
        if not last:
            assert emitted == sp.resample_ready(pos, ref.rate_in, ref.rate_out, METHOD_NAME[ref.method]), (m, pos)
    assert pos == len(x) and emitted == sp.resample_count(pos, ref.rate_in, ref.rate_out, METHOD_NAME[ref.method])
    return outs


@pytest.mark.parametrize("rate", RATES + (16000,))
def test_chunked_polyphase_equals_the_whole_signal_exactly(rate):
    rng = np.random.default_rng(rate)
    n = 700 if rate != 96000 else 1500
    x = np.round(rng.normal(0, 8000, n))
    want = R.resample(x, rate, R.POLYPHASE)
    ref = S.Chunked(R.POLYPHASE, rate)
    for name, sizes in S.chunkings(n, rng, ref.kmax).items():
        got = np.concatenate(_run(ref, x, sizes))
        assert len(got) == len(want) and np.array_equal(got, want), (rate, name)
        assert (ref.total, ref.emitted) == (0, 0)                  # the flush leaves the start of a new utterance
    # the exact bound on the tail: k_hi(next output) >= total, so [k_hi - (kmax - 1), total) holds at most kmax - 1 samples
    assert ref.longest_tail <= max(ref.kmax - 1, 0) or rate == 16000
    if rate != 16000:
        assert ref.longest_tail == ref.kmax - 1                    # ... and it is reached


@pytest.mark.parametrize("rate", RATES + (16000,))
@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_chunked_ratecv_equals_the_whole_signal_exactly(rate, width):
    rng = np.random.default_rng(rate + width)
    lim = 1 << (8 * width - 1)
    n = 3001
    x = rng.integers(-lim, lim, size=n)
    want = R.ratecv(x, width, rate) if rate != 16000 else x
    ref = S.Chunked(R.RATECV, rate, width=width)
    for name, sizes in S.chunkings(n, rng, 1).items():
        got = np.concatenate(_run(ref, x, sizes))
        assert len(got) == len(want) and np.array_equal(got, want), (rate, width, name)
    assert ref.longest_tail <= 1


def test_chunked_ratecv_equals_audioop_with_its_state():
    audioop = pytest.importorskip("audioop")
    rng = np.random.default_rng(7)
    for rate in (8000, 11025, 44100, 48000, 16001):
        x = rng.integers(-32768, 32768, size=5000)
        ref = S.Chunked(R.RATECV, rate, width=2)
        for name, sizes in S.chunkings(len(x), rng, 1).items():
            state, pos, theirs = None, 0, []
            ours = _run(ref, x, sizes)
            for s in sizes:
                out, state = audioop.ratecv(R.encode(x[pos:pos + s], 2), 2, 1, rate, 16000, state)
                theirs.append(R.decode(out, 2))
                pos += s
            a, b = np.concatenate(ours), np.concatenate(theirs)
            assert np.array_equal(a, b), (rate, name)
            assert np.array_equal(a, R.ratecv(x, 2, rate))


@pytest.fixture(scope="module")
def L():
    from danspeech_amd import _native
    return _native.lib()


def test_ready_equals_brute_force_and_is_monotone(L):
    from danspeech_amd import stream_plan as sp
    for rate in RATES + (16000, 32000):
        for method in (R.POLYPHASE, R.RATECV):
            prev = 0
            for n in list(range(0, 260)) + [1000, 4097, 44101]:
                got = L.dsmi_resample_ready(method, rate, 16000, n)
                assert got == S.ready(method, rate, 16000, n) == sp.resample_ready(n, rate, 16000, METHOD_NAME[method]), (rate, method, n)
                if n < 260:
                    assert got == S.ready_brute(method, rate, 16000, n), (rate, method, n)
                count = L.dsmi_resample_count(method, rate, 16000, n)
                assert prev <= got <= count and count == sp.resample_count(n, rate, 16000, METHOD_NAME[method])
                # the flush makes up the difference, and it is the filter's lookahead: under half / up + 1 input samples' worth
                if method == R.RATECV or rate == 16000:
                    assert got == count
                else:
                    up, down = R.ratio(rate, 16000)
                    assert count - got <= -(-(10 * max(up, down)) // down) + 1
                prev = got
    for bad in ((2, 44100, 16000, 10), (0, 0, 16000, 10), (0, 44100, -1, 10), (1, 44100, 16000, -1)):
        assert L.dsmi_resample_ready(*bad) < 0, bad


def test_need_is_the_inverse_of_ready():
    from danspeech_amd import stream_plan as sp
    for rate in RATES + (16000,):
        for method in ("polyphase", "ratecv"):
            for n_out in list(range(1, 200)) + [5000]:
                need = sp.resample_need(n_out, rate, 16000, method)
                # `need` samples make n_out outputs final, one fewer does not (as far as outputs exist at all by then)
                full = sp.resample_count(need, rate, 16000, method)
                assert sp.resample_ready(need, rate, 16000, method) >= min(n_out, full), (rate, method, n_out)
                assert sp.resample_ready(need - 1, rate, 16000, method) < n_out, (rate, method, n_out)


def test_creation_refusals_that_need_no_device(L):
    h = C.c_void_p()
    err = lambda: (L.dsmi_resampler_last_error(None) or b"").decode()
    for args, word in [((None, 0, 0, 0), "rate_in"), ((None, -8000, 1, 0), "rate_in"), ((None, 44100, 2, 0), "method"),
                       ((None, 44100, -1, 0), "method"), ((None, 44100, 1, 1), "ratecv"), ((None, 44100, 1, 2), "ratecv"),
                       ((None, 44100, 0, 16 | 3), "stereo"), ((None, 44100, 0, 16 | 1), "stereo"), ((None, 44100, 0, 16 | 2), "stereo"),
                       ((None, 44100, 0, 6), "pcm_dtype"), ((None, 44100, 0, 0), "frontend")]:
        assert L.dsmi_resampler_create(*args, C.byref(h)) == -1 and word in err(), (args, err())
        assert not h.value
    assert L.dsmi_resampler_create(None, 44100, 0, 0, None) == -1
    # null handles
    assert L.dsmi_resampler_reset(None) == -1 and L.dsmi_resampler_position(None, None, None) == -1
    L.dsmi_resampler_destroy(None)
    n = np.zeros(1, dtype=np.int64)
    assert L.dsmi_resampler_push_many(None, 1, None, n.ctypes.data_as(C.c_void_p), None, None, 0, None, None) == -1
    hs = (C.c_void_p * 1)(None)
    last = np.zeros(1, dtype=np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.dsmi_resampler_push_many(hs, 1, hs, ptr(n), ptr(last), None, 0, ptr(n), None) == -1 and "session 0" in err()
    for bad_n in (0, -1, 257):
        assert L.dsmi_resampler_push_many(hs, bad_n, hs, ptr(n), ptr(last), None, 0, ptr(n), None) == -1
        assert "DSMI_RESAMPLE_STREAM_MAX" in err()


def _feed_brute(plan, n_source, rate, method):
    """Push one source sample at a time until the pass's last output is final (or the source ends, which flushes)."""
    from danspeech_amd import stream_plan as sp
    feed, pos, flushed = [], 0, False
    for lo, hi, _, is_last in plan:
        upto = pos
        while upto < n_source and (is_last or sp.resample_ready(upto, rate, 16000, method) < hi):
            upto += 1
        flush = upto >= n_source and not flushed
        feed.append((pos, upto, flush))
        flushed, pos = flushed or flush, upto
    return feed


@pytest.mark.parametrize("method", ["polyphase", "ratecv"])
def test_feed_plan_equals_brute_force_and_feeds_every_pass(method):
    from danspeech_amd import stream_plan as sp
    for rate in (8000, 11025, 16001, 44100, 48000, 16000):
        for n_source, chunk in [(rate * 2 + 17, None), (rate + 3, 2048), (rate // 2, 1024), (int(rate * 1.3), 700)]:
            n_conv = sp.resample_count(n_source, rate, 16000, method)
            plan = sp.stream_cut_plan(n_conv, chunk, 20, 160)
            feed = sp.resample_feed_plan(plan, n_source, rate, 16000, method)
            assert feed == _feed_brute(plan, n_source, rate, method), (rate, n_source, chunk)
            assert len(feed) == len(plan)
            pos, flushed = 0, False
            for (lo, hi, _, is_last), (a, b, flush) in zip(plan, feed):
                assert a == pos and b >= a                               # nothing is pushed twice, nothing is skipped
                pos, flushed = b, flushed or flush
                have = n_conv if flushed else sp.resample_ready(pos, rate, 16000, method)
                assert have >= hi, (rate, n_source, lo, hi)              # every pass's hi is ready after its push
                assert not flush or b == n_source
            if plan:
                assert pos == n_source and flushed and plan[-1][1] == n_conv
    assert sp.resample_feed_plan([], 1000, 8000) == []
    with pytest.raises(ValueError):
        sp.resample_feed_plan([(0, 10, True, False)], 100, 8000, 16000, "cubic")


def test_surface_keeps_its_defaults():
    import inspect
    from danspeech_amd import Recognizer
    from danspeech_amd.DanSpeechRecognizer import DanSpeechRecognizer
    sig = inspect.signature
    for fn in (Recognizer.stream_recording, Recognizer.stream_recordings, DanSpeechRecognizer.enable_streaming,
               DanSpeechRecognizer.new_streaming_session):
        assert sig(fn).parameters["sample_rate"].default is None and sig(fn).parameters["resample"].default == "polyphase", fn
    assert sig(Recognizer.stream_recording).parameters["chunk_samples"].default is None
