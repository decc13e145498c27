"""Chunked sample-rate conversion on the GPU (dsmi_resampler_*, csrc/resample_stream.hip) through the C ABI and the Python surface.

  chunk invariance  however an utterance is cut, the pushes' outputs laid end to end are ``np.array_equal`` to ONE dsmi_resample
                    call over the whole utterance on the same device: both methods, six sample types, seven rates and equal
                    rates, five chunkings (one of them all of one sample, the flush coming with the last sample); every push's count is the closed form, ``position`` is right after every push
  many sessions     N = 37 and N = 256 in one call, rates / methods / types mixed, out of phase, ragged: each session equals
                    its own single-handle run; a session alternates between push and push_many
  refusals          leave every handle and out_dev untouched
  features          device-tensor parts give bit-equal features to the same samples as numpy parts
  end to end        stream_recording(x, c, sample_rate=r, resample=m) == stream_recording(audio.resample(x, r, method=m), c)
"""
import ctypes as C

import numpy as np
import pytest

import _resample_ref as R
import _resample_stream_ref as S
from danspeech_amd import synthetic as syn

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

RATES = (8000, 11025, 16001, 22050, 44100, 48000, 96000, 16000)
METHODS = {"polyphase": R.POLYPHASE, "ratecv": R.RATECV}
SENTINEL = -12345.678


@pytest.fixture(scope="module")
def native():
    from danspeech_amd import _native
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _native


@pytest.fixture(scope="module")
def fe(native):
    f = native.NativeFrontend()
    yield f
    f.close()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def _signal(kind, n, rng):
    """-> (host array whose rows of ``per`` entries are one sample each, per, NativeResampler arguments)"""
    if kind == "i16":
        return np.round(rng.normal(0, 8000, n)).clip(-32768, 32767).astype(np.int16), 1, dict(dtype=np.int16)
    if kind == "f32":
        return rng.normal(0, 0.3, n).astype(np.float32), 1, dict(dtype=np.float32)
    if kind == "f64":
        return rng.normal(0, 0.3, n), 1, dict(dtype=np.float64)
    if kind == "u8":
        return np.frombuffer(R.encode(rng.integers(-128, 128, size=n), 1), dtype=np.uint8), 1, dict(wav_format=(1, 1))
    if kind == "i24":
        return np.frombuffer(R.encode(rng.integers(-(1 << 23), 1 << 23, size=n), 3), dtype=np.uint8), 3, dict(wav_format=(3, 1))
    assert kind == "stereo16"
    f = rng.integers(-32768, 32768, size=2 * n).astype("<i2")
    f[:len(f) // 3] = np.where(f[:len(f) // 3] < 0, -32768, 32767)          # saturating sums among them
    return f, 2, dict(wav_format=(2, 2))


def _whole(fe, x, n, rate, method, args):
    wav = args.get("wav_format")
    pcm = _dev(x.view(np.uint8)) if wav else _dev(x)
    out, n_out = fe.resample(pcm, [n], rate, method, wav_format=wav)
    return out.cpu().numpy()


@pytest.mark.parametrize("kind", ["i16", "f32", "f64", "u8", "i24", "stereo16"])
@pytest.mark.parametrize("method", ["polyphase", "ratecv"])
def test_chunk_invariance_bit_for_bit(native, fe, method, kind):
    if method == "ratecv" and kind in ("f32", "f64"):
        with pytest.raises(native.DsmiError, match="ratecv"):
            native.NativeResampler(fe, 44100, "ratecv", dtype=np.float32 if kind == "f32" else np.float64)
        return
    m = METHODS[method]
    for rate in RATES:
        rng = np.random.default_rng(rate + len(kind))
        n = 2500
        x, per, args = _signal(kind, n, rng)
        want = _whole(fe, x, n, rate, method, args)
        pcm = _dev(x)
        rs = native.NativeResampler(fe, rate, method, **args)
        tail = S.kmax(rate, 16000) if method == "polyphase" and rate != 16000 else 1
        for name, sizes in S.chunkings(n, rng, tail).items():
            outs, pos, emitted = [], 0, 0
            for k, s in enumerate(sizes):
                last = k == len(sizes) - 1
                outs.append(rs.push(pcm[pos * per:(pos + s) * per], is_last=last))
                pos += s
                due = (R.count(m, rate, 16000, pos) if rate != 16000 else pos) if last else S.ready(m, rate, 16000, pos)
                assert outs[-1].numel() == due - emitted, (rate, name, k)         # n_out_host is the closed form
                emitted = due
                assert rs.position() == ((0, 0) if last else (pos, emitted)), (rate, name, k)
            got = torch.cat(outs).cpu().numpy()
            assert len(got) == len(want) and np.array_equal(got, want), (method, kind, rate, name)
        rs.close()


def _mixed_sessions(native, fe, N, seed):
    rng = np.random.default_rng(seed)
    kinds = [("polyphase", 8000, "i16"), ("ratecv", 8000, "i16"), ("polyphase", 44100, "stereo16"), ("ratecv", 44100, "stereo16"),
             ("polyphase", 48000, "f64"), ("polyphase", 16000, "i16"), ("ratecv", 11025, "i24"), ("polyphase", 22050, "f32"),
             ("ratecv", 16000, "u8"), ("polyphase", 96000, "i16"), ("ratecv", 48000, "i16")]
    ses = []
    for i in range(N):
        method, rate, kind = kinds[i % len(kinds)]
        n = int(rng.integers(1, 4000))
        x, per, args = _signal(kind, n, rng)
        # ragged schedules, out of phase: rounds sat out before the first chunk, chunks of 0 samples among them
        sizes, left = [None] * int(rng.integers(0, 3)), n
        while left:
            s = int(min(left, rng.choice([0, 1, 7, 160, 700, 1500])))
            sizes.append(s)
            left -= s
        if rng.integers(0, 3) == 0:
            sizes.append(0)                                   # ... and an utterance whose last push brings nothing but the flush
        ses.append(dict(method=method, rate=rate, args=args, x=x, per=per, n=n, sizes=sizes, pcm=_dev(x)))
    return ses


@pytest.mark.parametrize("N", [37, 256])
def test_many_sessions_in_one_call_equal_each_session_alone(native, fe, N):
    ses = _mixed_sessions(native, fe, N, seed=N)
    many = [native.NativeResampler(fe, s["rate"], s["method"], **s["args"]) for s in ses]
    got = [[] for _ in ses]
    pos = [0] * N
    rounds = max(len(s["sizes"]) for s in ses)
    for r in range(rounds):
        due = [i for i, s in enumerate(ses) if r < len(s["sizes"]) and s["sizes"][r] is not None]
        chunks, last = [], []
        for i in due:
            s = ses[i]
            k = s["sizes"][r]
            chunks.append(s["pcm"][pos[i] * s["per"]:(pos[i] + k) * s["per"]] if k else None)
            pos[i] += k
            last.append(r == len(s["sizes"]) - 1)
        if due and due[0] == 0 and r % 2:                     # session 0 alternates between push and push_many
            got[0].append(many[0].push(chunks[0], last[0]))
            due, chunks, last = due[1:], chunks[1:], last[1:]
        outs = native.NativeResampler.push_many([many[i] for i in due], chunks, last)
        for i, o in zip(due, outs):
            got[i].append(o)
    for i, s in enumerate(ses):
        # its own single-handle run over the same chunks, and the whole utterance in one dsmi_resample
        alone = native.NativeResampler(fe, s["rate"], s["method"], **s["args"])
        p, outs = 0, []
        sizes = [k for k in s["sizes"] if k is not None]
        for j, k in enumerate(sizes):
            outs.append(alone.push(s["pcm"][p * s["per"]:(p + k) * s["per"]] if k else None, j == len(sizes) - 1))
            p += k
        assert len(outs) == len(got[i])
        for a, b in zip(outs, got[i]):
            assert a.numel() == b.numel() and torch.equal(a, b), i
        assert np.array_equal(torch.cat(got[i]).cpu().numpy(), _whole(fe, s["x"], s["n"], s["rate"], s["method"], s["args"])), i
        assert many[i].position() == (0, 0)
        alone.close()
    for h in many:
        h.close()


def test_refusals_leave_every_handle_and_the_output_unchanged(native, fe):
    L = native.lib()
    rng = np.random.default_rng(5)
    x = np.round(rng.normal(0, 5000, 6000)).astype(np.int16)
    pcm = _dev(x)
    fe2 = native.NativeFrontend()
    a, b, ref_a, ref_b = (native.NativeResampler(fe, r, m) for r, m in [(44100, "polyphase"), (8000, "ratecv")] * 2)
    other = native.NativeResampler(fe2, 44100, "polyphase")
    for h in (a, ref_a):
        h.push(pcm[:1000])
    for h in (b, ref_b):
        h.push(pcm[:777])
    state = [h.position() for h in (a, b)]
    F = native.DsmiError
    with pytest.raises(F, match="session 1.*twice"):
        native.NativeResampler.push_many([a, a], [pcm[1000:1500], pcm[1500:2000]], [False, False])
    with pytest.raises(F, match="session 1.*frontend"):
        native.NativeResampler.push_many([a, other], [pcm[1000:1500], pcm[1500:2000]], [False, False])
    # the raw C call: capacity one short, N = 257, a negative count
    out = torch.full((4096,), SENTINEL, dtype=torch.float64, device="cuda")
    ptr = lambda v: v.ctypes.data_as(C.c_void_p)
    hs = (C.c_void_p * 2)(a._h, b._h)
    pp = (C.c_void_p * 2)(pcm[1000:].data_ptr(), pcm[777:].data_ptr())
    ns = np.array([500, 300], dtype=np.int64)
    last = np.zeros(2, dtype=np.int32)
    n_out = np.full(2, -99, dtype=np.int64)
    need = a._due(500, False) + b._due(300, False)
    assert need > 100
    err = lambda: (L.dsmi_resampler_last_error(None) or b"").decode()
    assert L.dsmi_resampler_push_many(hs, 2, pp, ptr(ns), ptr(last), out.data_ptr(), need - 1, ptr(n_out), None) == native.DSMI_ERR_CAPACITY
    assert "out_dev" in err()
    ns_bad = np.array([500, -1], dtype=np.int64)
    assert L.dsmi_resampler_push_many(hs, 2, pp, ptr(ns_bad), ptr(last), out.data_ptr(), 4096, ptr(n_out), None) == native.DSMI_ERR_INVALID
    assert "session 1" in err()
    crowd = [native.NativeResampler(fe, 16000, "polyphase") for _ in range(257)]
    hs257 = (C.c_void_p * 257)(*[h._h for h in crowd])
    z64, z32, o257 = np.zeros(257, dtype=np.int64), np.zeros(257, dtype=np.int32), np.zeros(257, dtype=np.int64)
    assert L.dsmi_resampler_push_many(hs257, 257, hs257, ptr(z64), ptr(z32), out.data_ptr(), 4096, ptr(o257), None) == native.DSMI_ERR_INVALID
    assert "DSMI_RESAMPLE_STREAM_MAX" in err()
    assert L.dsmi_resampler_push_many(hs257, 256, hs257, ptr(z64), ptr(z32), out.data_ptr(), 4096, ptr(o257), None) == 0
    torch.cuda.synchronize()
    assert (out == SENTINEL).all().item() and n_out.tolist() == [-99, -99]
    assert [h.position() for h in (a, b)] == state
    # the next valid call gives what it would have given
    ya, yb = native.NativeResampler.push_many([a, b], [pcm[1000:1500], pcm[777:1077]], [False, False])
    assert torch.equal(ya, ref_a.push(pcm[1000:1500])) and torch.equal(yb, ref_b.push(pcm[777:1077]))
    ya, yb = native.NativeResampler.push_many([a, b], [pcm[1500:], None], [True, True])
    assert torch.equal(ya, ref_a.push(pcm[1500:], True)) and torch.equal(yb, ref_b.push(None, True))
    for h in [a, b, ref_a, ref_b, other] + crowd:
        h.close()
    fe2.close()


def test_creation_refusals_that_need_a_frontend_and_pushes_after_a_close(native, fe):
    F = native.DsmiError
    for method in ("polyphase", "ratecv"):
        # 99991 -> 16000 has two million taps; 16001 -> 16000 has 320 021 and is admitted
        with pytest.raises(F, match="DSMI_RESAMPLE_MAX_TAPS") as e:
            native.NativeResampler(fe, 99991, method)
        assert e.value.code == native.DSMI_ERR_CAPACITY
        with pytest.raises(F, match="DSMI_RESAMPLE_MAX_DECIMATION") as e:
            native.NativeResampler(fe, 16000 * 25, method)
        assert e.value.code == native.DSMI_ERR_CAPACITY
        native.NativeResampler(fe, 16000 * 24, method).close()
    native.NativeResampler(fe, 16001, "polyphase").close()
    # a handle points into its frontend: the wrapper refuses a push after either was closed
    fe2 = native.NativeFrontend()
    a, b = native.NativeResampler(fe2, 8000), native.NativeResampler(fe2, 8000)
    x = _dev(np.arange(100, dtype=np.int16))
    a.push(x)
    b.close()
    with pytest.raises(ValueError, match="session 1"):
        native.NativeResampler.push_many([a, b], [x, x], [False, False])
    assert a.position()[0] == 100
    fe2.close()
    with pytest.raises(ValueError, match="session 0"):
        a.push(x)
    a.close()


def test_a_take_beyond_what_is_final_is_refused_before_any_session_moves():
    from danspeech_amd import Recognizer
    rec = Recognizer()
    rec.update_model(_stream_model("stream-take", 64, 2, 20, seed=87))
    eng = rec.danspeech_recognizer
    eng.enable_streaming(sample_rate=8000)
    eng.audio_parser.parse_audio = lambda part, is_last=False: []          # (the model is not run)
    x = _source(5, 8000, 1.0)
    eng.streaming_transcribe(x[:4000], is_last=False, is_first=True, take=7000)
    ses = eng._session
    before = (ses.resampler.position(), ses.pending.numel())
    assert before[0][0] == 4000 and before[1] == before[0][1] - 7000 > 0
    with pytest.raises(ValueError, match="are final"):
        eng.streaming_transcribe(x[4000:4100], is_last=False, is_first=False, take=5000)
    assert (ses.resampler.position(), ses.pending.numel()) == before
    eng.set_streaming_source(None)
    with pytest.raises(ValueError, match="take must be"):
        eng.streaming_transcribe(x[:4000].astype(np.float64), is_last=False, is_first=True, take=7000)
    eng.disable_streaming()


@pytest.mark.parametrize("method", ["polyphase", "ratecv"])
def test_reset_and_the_flush(native, fe, method):
    rng = np.random.default_rng(9)
    x = np.round(rng.normal(0, 5000, 5000)).astype(np.int16)
    pcm = _dev(x)
    h = native.NativeResampler(fe, 44100, method)
    assert h.push(None, True).numel() == 0 and h.position() == (0, 0)          # the flush of an utterance with no input
    first = torch.cat([h.push(pcm[:700]), h.push(pcm[700:3000], True)])
    assert np.array_equal(first.cpu().numpy(), _whole(fe, x[:3000], 3000, 44100, method, {}))
    # after a flush the handle starts anew: a second utterance equals a fresh handle's
    fresh = native.NativeResampler(fe, 44100, method)
    for lo, hi, last in [(3000, 3001, False), (3001, 4200, False), (4200, 5000, True)]:
        assert torch.equal(h.push(pcm[lo:hi], last), fresh.push(pcm[lo:hi], last))
    # reset in mid-utterance
    h.push(pcm[:1234])
    h.reset()
    assert h.position() == (0, 0)
    second = torch.cat([h.push(pcm[100:900]), h.push(pcm[900:2000], True)])
    assert np.array_equal(second.cpu().numpy(), _whole(fe, x[100:2000], 1900, 44100, method, {}))
    h.close(); fresh.close()


def test_features_of_device_parts_equal_features_of_numpy_parts():
    from danspeech_amd.audio.parsers import InferenceSpectrogramAudioParser as P
    rng = np.random.default_rng(12)
    sizes = [5000, 733, 480, 4097, 401, 2500, 900]          # (every part at least one window: the parser asks for that)
    x = np.round(rng.normal(0, 3000, sum(sizes)))
    cuts = np.concatenate(([0], np.cumsum(sizes)))
    parts = [x[cuts[i]:cuts[i + 1]] for i in range(len(sizes))]
    on_host, on_dev = P(), P()
    for i, part in enumerate(parts):
        last = i == len(parts) - 1
        want = on_host.parse_audio(part, last)
        got = on_dev.parse_audio(_dev(part), last)
        assert len(want) == len(got)
        if len(want):
            assert want.shape == got.shape and torch.equal(want, got), i
        assert np.array_equal(on_host._state, on_dev._state)
    # parse_audio_many: five parsers out of step
    host5, dev5 = [P() for _ in range(5)], [P() for _ in range(5)]
    for r in range(4):
        chunk = [np.round(rng.normal(0, 3000, int(rng.integers(400, 6000)))) for _ in range(5)]
        if r == 3:
            chunk[2] = chunk[2][:100]                          # a closing part shorter than one window
        last = [r == 3] * 5
        want = P.parse_audio_many(host5, chunk, last)
        got = P.parse_audio_many(dev5, [_dev(c) for c in chunk], last)
        for k in range(5):
            assert len(want[k]) == len(got[k])
            if len(want[k]):
                assert torch.equal(want[k], got[k]), (r, k)
            assert np.array_equal(host5[k]._state, dev5[k]._state)


# ---- end to end ------------------------------------------------------------------------------------------------------------
def _stream_model(name, H, L, ctx, seed):
    from danspeech_amd.deepspeech.model import DeepSpeech
    sd = syn.make_state_dict(2, "gru", H, L, bidirectional=False, context=ctx, seed=seed, fc_gain=8.0)
    return DeepSpeech(name, rnn_type="gru", rnn_hidden_size=H, rnn_layers=L, conv_layers=2, context=ctx, bidirectional=False,
                      streaming_inference_model=True).load_state_dict(sd)


def _source(seed, rate, seconds):
    """int16 audio at ``rate``: a 16 kHz synthetic clip's kind of signal, made at the source's own rate"""
    rng = np.random.default_rng(seed)
    n = int(rate * seconds)
    t = np.arange(n) / float(rate)
    x = 2500.0 * rng.standard_normal(n)
    for _ in range(3):
        x += rng.uniform(1000, 4000) * np.sin(2 * np.pi * rng.uniform(100, 3000) * t)
    return np.clip(np.rint(x), -16000, 16000).astype(np.int16)


@pytest.fixture(scope="module")
def arpa(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("lm") / "s3.arpa")
    syn.make_arpa(p, order=3, n_words=300, seed=13, ngrams_per_order=900)
    return p


@pytest.mark.parametrize("lm_partials", [False, True])
@pytest.mark.parametrize("method", ["polyphase", "ratecv"])
def test_stream_recording_of_another_rate_equals_streaming_the_converted_recording(arpa, method, lm_partials):
    from danspeech_amd import Recognizer, audio
    m = _stream_model("stream-rate", 64, 2, 20, seed=87)
    rec = Recognizer(model=m, lm=arpa) if lm_partials else Recognizer()
    total = 0
    for rate, chunk in [(8000, 1024), (44100, 2048), (44100, None)]:
        x = _source(rate, rate, 2.5)
        converted = audio.resample(x, rate, method=method)
        rec.enable_real_time_streaming(streaming_model=m, lm_partials=lm_partials)
        want = list(rec.stream_recording(converted, chunk))
        rec.enable_real_time_streaming(streaming_model=m, lm_partials=lm_partials)
        got = list(rec.stream_recording(x, chunk, sample_rate=rate, resample=method))
        assert got == want, (rate, chunk)
        # ... and the engine is back at the model's rate: default arguments give today's yields
        rec.enable_real_time_streaming(streaming_model=m, lm_partials=lm_partials)
        assert list(rec.stream_recording(converted, chunk, sample_rate=None)) == want
        rec.enable_real_time_streaming(streaming_model=m, lm_partials=lm_partials)
        assert list(rec.stream_recording(converted, chunk, sample_rate=16000)) == want
        total += len(want)
    assert total >= 6
    rec.disable_real_time_streaming()


def test_stream_recordings_with_a_rate_per_recording():
    from danspeech_amd import Recognizer
    m = _stream_model("stream-rates", 64, 2, 20, seed=99)
    rec = Recognizer()
    rates = [8000, 16000, 48000, None, 8000, 48000, 16000, 44100]
    audio = [_source(40 + i, r or 16000, 1.2 + 0.37 * i) for i, r in enumerate(rates)]
    for method in ("polyphase", "ratecv"):
        rec.enable_real_time_streaming(streaming_model=m)
        got = list(rec.stream_recordings(audio, chunk_samples=2048, sample_rate=rates, resample=method))
        total = 0
        for i, (a, r) in enumerate(zip(audio, rates)):
            rec.enable_real_time_streaming(streaming_model=m)
            want = list(rec.stream_recording(a, 2048, sample_rate=r, resample=method))
            assert [(l, t) for k, l, t in got if k == i] == want, (method, i)
            total += len(want)
        assert total == len(got) and total >= len(audio)
    # one rate for all, and today's call unchanged
    rec.enable_real_time_streaming(streaming_model=m)
    same = [a for a, r in zip(audio, rates) if r == 8000]
    got = list(rec.stream_recordings(same, chunk_samples=1024, sample_rate=8000))
    for i, a in enumerate(same):
        rec.enable_real_time_streaming(streaming_model=m)
        assert [(l, t) for k, l, t in got if k == i] == list(rec.stream_recording(a, 1024, sample_rate=8000))
    rec.disable_real_time_streaming()


def test_live_parts_through_the_engine_equal_the_converted_utterance(native):
    """``enable_streaming(sample_rate=...)``: parts of a source at 8 kHz as they would arrive from a telephone line, of any
    size; what reaches the parser, laid end to end, is the conversion of the whole utterance."""
    from danspeech_amd import Recognizer, audio
    m = _stream_model("stream-live", 64, 2, 20, seed=87)
    rec = Recognizer()
    rec.update_model(m)
    eng = rec.danspeech_recognizer
    eng.enable_streaming(sample_rate=8000)
    x = _source(3, 8000, 2.0)
    seen = []
    eng.audio_parser.parse_audio = lambda part, is_last=False: (seen.append(part.cpu().numpy()), [])[1]      # (the model is not run)
    cuts = [0, 3000, 3001, 3001, 7000, 12000, len(x)]
    for k in range(len(cuts) - 1):
        eng.streaming_transcribe(x[cuts[k]:cuts[k + 1]], is_last=k == len(cuts) - 2, is_first=k == 0)
    assert np.array_equal(np.concatenate(seen), audio.resample(x, 8000))
    eng.disable_streaming()


def test_push_many_cuts_at_the_maximum_and_checks_every_session_first(native, fe):
    """257 sessions are two native calls (RESAMPLE_STREAM_MAX = 256): each session's outputs are those of the same push made alone
    on a fresh handle, and a closed handle in the second call is refused before the first call moves a session."""
    n = native.RESAMPLE_STREAM_MAX + 1
    rng = np.random.default_rng(257)
    x = np.round(rng.normal(0, 8000, (n, 8))).astype(np.int16)
    rs = [native.NativeResampler(fe, 8000, "polyphase", dtype=np.int16) for _ in range(n)]
    pcms = [_dev(row) for row in x]
    outs = native.NativeResampler.push_many(rs, pcms, [True] * n)
    assert len(outs) == n
    for i in range(n):
        alone = native.NativeResampler(fe, 8000, "polyphase", dtype=np.int16)
        want = alone.push(pcms[i], True).cpu().numpy()
        alone.close()
        assert len(want) == 16 and np.array_equal(outs[i].cpu().numpy(), want), i
    before = rs[0].position(), rs[255].position()
    rs[256].close()
    with pytest.raises(ValueError, match="session 256"):
        native.NativeResampler.push_many(rs, pcms, [False] * n)
    assert (rs[0].position(), rs[255].position()) == before
    for r in rs:
        r.close()
