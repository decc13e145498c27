"""GPU tests of the resumable beam search: dsmi_beam_stream_* / NativeBeamStream carry one utterance's CTC prefix beam search
from chunk to chunk, many sessions per launch, and after every chunk the hypotheses must be those of dsmi_beam over the
concatenated prefix -- tokens, timesteps and lengths exactly, the reported scores bit for bit (the same double totals go
through the same host-side stripping).  Then the recogniser surface: streaming with lm_partials=True."""
import ctypes

import numpy as np
import pytest

from danspeech_amd import synthetic as syn

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LABELS = syn.DANSPEECH_LABELS


@pytest.fixture(scope="module")
def native():
    from danspeech_amd import _native
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    _native.lib()
    return _native


@pytest.fixture(scope="module")
def arpas(tmp_path_factory):
    d = tmp_path_factory.mktemp("lm")
    p3, p5 = str(d / "s3.arpa"), str(d / "s5.arpa")
    syn.make_arpa(p3, order=3, n_words=300, seed=13, ngrams_per_order=900)
    syn.make_arpa(p5, order=5, n_words=300, seed=14, ngrams_per_order=900)
    return {None: None, 3: p3, 5: p5}


def _probs(T, seed, C=len(LABELS), sharp=3.0):
    rng = np.random.default_rng(seed)
    logits = rng.standard_normal((T, C)) * sharp
    logits[:, 0] += 1.5
    e = np.exp(logits - logits.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


def _chunks(rng, T, zeros=2):
    out, left = [], T
    while left > 0:
        c = int(min(left, rng.integers(1, 13)))
        out.append(c)
        left -= c
    for _ in range(zeros):
        out.insert(int(rng.integers(0, len(out) + 1)), 0)
    return out


def _decoder(native, lm_path, alpha=1.3, beta=0.2):
    dec = native.NativeDecoder(LABELS, blank_index=0)
    if lm_path:
        dec.set_lm(lm_path, alpha, beta)
    return dec


def _same_as_whole(dec, p_dev, t, res, beam, n_best, what=""):
    """res = one stream's (tok, ts, ln, sc) after t frames; the whole search over the first t rows of p_dev"""
    tok, ts, ln, sc = res
    wt, ww, wl, ws = dec.beam(p_dev[:t].unsqueeze(0).contiguous(), None, beam_width=beam)
    assert np.array_equal(ln, wl[0, :n_best]), (what, t)
    for p in range(n_best):
        L = int(ln[p])
        assert np.array_equal(tok[p, :L], wt[0, p, :L]), (what, t, p)
        assert np.array_equal(ts[p, :L], ww[0, p, :L]), (what, t, p)
    assert sc.tobytes() == ws[0, :n_best].tobytes(), (what, t, sc[:4], ws[0, :4])


@pytest.mark.parametrize("beam", [64, 128, 20])
@pytest.mark.parametrize("order", [None, 3, 5])
def test_stream_equals_whole_search_after_every_chunk(native, arpas, beam, order):
    """C = 33 at beam 64 and 128 (the specialised builds) and beam 20 (a generic build), without a scorer and with a 3- and a
    5-gram ARPA; ragged chunks with 0-frame advances among them"""
    dec = _decoder(native, arpas[order])
    T = 70
    seed = 1000 + beam + (order or 0)
    p = torch.from_numpy(_probs(T, seed)).cuda()
    st = native.NativeBeamStream(dec, beam, 40, 1.0)
    t = 0
    for c in _chunks(np.random.default_rng(seed), T):
        res = st.advance(p[t:t + c], n_best=beam)
        t += c
        assert st.frames == t
        if t > 0:
            _same_as_whole(dec, p, t, res, beam, beam, "beam %d order %s" % (beam, order))
    st.close()
    dec.close()


@pytest.mark.parametrize("N", [1, 7, 64, 300])
def test_many_sessions_out_of_phase_equal_each_session_alone(native, arpas, N):
    dec = _decoder(native, arpas[3])
    rng = np.random.default_rng(N)
    Ts = [int(rng.integers(20, 48)) for _ in range(N)]
    ps = [torch.from_numpy(_probs(T, 5000 + i)).cuda() for i, T in enumerate(Ts)]
    plans = [[0] * int(rng.integers(0, 3)) + _chunks(rng, T, zeros=1) for T in Ts]       # some start late
    many = [native.NativeBeamStream(dec, 64, 40, 1.0) for _ in range(N)]
    solo = [native.NativeBeamStream(dec, 64, 40, 1.0) for _ in range(N)]
    pos = [0] * N
    for r in range(max(len(pl) for pl in plans)):
        due = [i for i in range(N) if r < len(plans[i])]
        chunks = [ps[i][pos[i]:pos[i] + plans[i][r]] for i in due]
        got = native.NativeBeamStream.advance_many([many[i] for i in due], chunks, 2)
        for i, ch, g in zip(due, chunks, got):
            want = solo[i].advance(ch, n_best=2)
            for a, b in zip(g, want):
                assert a.tobytes() == b.tobytes(), (N, i, r)
            pos[i] += plans[i][r]
    for i in range(0, N, max(1, N // 5)):        # and the end of some against the whole search
        res = many[i].advance(None, n_best=8)
        _same_as_whole(dec, ps[i], Ts[i], res, 64, 8, "session %d" % i)
    for s in many + solo:
        s.close()
    dec.close()


def test_node_pool_grows_over_hundreds_of_one_frame_advances(native, arpas):
    """the first pool holds 8 frames' nodes: 320 frames make it double six times"""
    dec = _decoder(native, arpas[3])
    T = 320
    p = torch.from_numpy(_probs(T, 77, sharp=2.0)).cuda()
    st = native.NativeBeamStream(dec, 64, 40, 1.0)
    for t in range(T):
        res = st.advance(p[t:t + 1], n_best=64 if (t + 1) % 80 == 0 else 0)
        if res is not None:
            _same_as_whole(dec, p, t + 1, res, 64, 64, "pool")
    st.close()
    dec.close()


def test_refusals_change_nothing(native, arpas):
    L = native.lib()
    dec = _decoder(native, arpas[3])
    other = _decoder(native, arpas[3])
    T = 40
    p = torch.from_numpy(_probs(T, 91)).cuda()
    s = native.NativeBeamStream(dec, 64, 40, 1.0)
    s.advance(p[:10])
    foreign = native.NativeBeamStream(other, 64, 40, 1.0)
    narrow = native.NativeBeamStream(dec, 32, 40, 1.0)
    retired = native.NativeBeamStream(other, 64, 40, 1.0)
    other.set_lm(arpas[3], 0.5, 0.1)              # the scorer `retired` was made with is gone
    for bad in ([s, s], [s, foreign], [s, narrow], [s, retired]):
        with pytest.raises(native.DsmiError):
            native.NativeBeamStream.advance_many(bad, [p[10:15]] * len(bad), 1)
        assert s.frames == 10
    # a collect pending: the next advance is refused until it is collected
    h = (ctypes.c_void_p * 1)(s._h)
    fp = (ctypes.c_void_p * 1)(p[10:20].data_ptr())
    fr = np.array([10], dtype=np.int32)
    assert L.dsmi_beam_stream_advance_many(h, 1, fp, native._np_ptr(fr), 1, None) == 0
    with pytest.raises(native.DsmiError):
        s.advance(p[20:25])
    i32 = np.zeros(64 * 40, dtype=np.int32)
    f32 = np.zeros(64, dtype=np.float32)
    cnt = np.zeros(1, dtype=np.int32)
    assert L.dsmi_beam_stream_collect_many(h, 1, 2, 40, native._np_ptr(i32), native._np_ptr(i32), native._np_ptr(i32),
                                           native._np_ptr(f32), native._np_ptr(cnt)) != 0       # another n_best: refused
    assert L.dsmi_beam_stream_collect_many(h, 1, 1, 40, native._np_ptr(i32), native._np_ptr(i32), native._np_ptr(i32),
                                           native._np_ptr(f32), native._np_ptr(cnt)) == 0
    assert s.frames == 20
    res = s.advance(p[20:], n_best=64)
    _same_as_whole(dec, p, T, res, 64, 64, "after refusals")
    for x in (s, foreign, narrow, retired):
        x.close()
    dec.close()
    other.close()


# ---- the recogniser ---------------------------------------------------------------------------------------------------
def _stream_model(name, H, L, ctx, seed, kind="gru"):
    from danspeech_amd.deepspeech.model import DeepSpeech
    sd = syn.make_state_dict(2, kind, H, L, bidirectional=False, context=ctx, seed=seed, fc_gain=8.0)
    return DeepSpeech(name, rnn_type=kind, rnn_hidden_size=H, rnn_layers=L, conv_layers=2, context=ctx, bidirectional=False,
                      streaming_inference_model=True).load_state_dict(sd)


def _lm_recognizer(path, seed=87):
    from danspeech_amd import Recognizer
    rec = Recognizer(model=_stream_model("stream-lm", 64, 2, 20, seed=seed), lm=path)
    return rec


def test_recognizer_lm_partials(arpas):
    audio = syn.make_clip(6, 16000 * 4)
    rec = _lm_recognizer(arpas[3])
    eng = rec.danspeech_recognizer
    rec.enable_real_time_streaming(streaming_model=eng.model)
    plain = list(rec.stream_recording(audio, chunk_samples=2048))
    rec.disable_real_time_streaming()
    rec.enable_real_time_streaming(streaming_model=eng.model, lm_partials=True)
    # every middle output is the full decode of the outputs so far; the final text is the lm_partials=False one
    middles = 0
    final = None
    for lo, hi, is_first, is_last in rec._cut_plan(len(audio), 2048):
        out = eng.streaming_transcribe(audio[lo:hi], is_last=is_last, is_first=is_first)
        ses = eng._session
        if is_last:
            final = out
        elif not is_first and ses.outputs:
            assert out == eng.decoder.decode(torch.cat(ses.outputs, dim=1))[0][0][0]
            middles += 1
    assert middles >= 3
    assert plain[-1][0] is True and final == plain[-1][1]
    rec.enable_real_time_streaming(streaming_model=eng.model, lm_partials=True)
    assert list(rec.stream_recording(audio, chunk_samples=2048))[-1] == plain[-1]
    # many sessions: per index what stream_recording gives as the first recording after enable_real_time_streaming
    clips = [syn.make_clip(20 + k, 16000 * (2 + k % 3)) for k in range(5)]
    alone = {}
    for k, c in enumerate(clips):
        rec.enable_real_time_streaming(streaming_model=eng.model, lm_partials=True)
        alone[k] = list(rec.stream_recording(c, chunk_samples=2048))
    assert any(len(v) >= 3 for v in alone.values())
    got = {k: [] for k in range(len(clips))}
    for k, last, text in rec.stream_recordings(clips, chunk_samples=2048):
        got[k].append((last, text))
    assert got == alone
    rec.disable_real_time_streaming()


def test_recognizer_lm_partials_with_secondary_model_and_decoder_update(arpas):
    from danspeech_amd.deepspeech.model import DeepSpeech
    audio = syn.make_clip(7, 16000 * 3)
    rec = _lm_recognizer(arpas[3])
    eng = rec.danspeech_recognizer
    sd2 = syn.make_state_dict(2, "gru", 64, 2, seed=88, fc_gain=8.0)
    second = DeepSpeech("second", rnn_hidden_size=64, rnn_layers=2).load_state_dict(sd2)
    finals = []
    for lm_partials in (False, True):
        rec.enable_real_time_streaming(streaming_model=eng.model, secondary_model=second, lm_partials=lm_partials)
        finals.append(list(rec.stream_recording(audio, chunk_samples=2048))[-1])
        rec.disable_real_time_streaming()
    assert finals[0] == finals[1] and finals[0][0] is True
    # update_decoder mid-utterance: the final text is the full decode with the new alpha
    outs = []
    for lm_partials in (False, True):
        rec.update_decoder(alpha=1.3)
        rec.enable_real_time_streaming(streaming_model=eng.model, lm_partials=lm_partials)
        plan = rec._cut_plan(len(audio), 2048)
        res = []
        for j, (lo, hi, is_first, is_last) in enumerate(plan):
            if j == len(plan) // 2:
                rec.update_decoder(alpha=2.7)
            res.append(eng.streaming_transcribe(audio[lo:hi], is_last=is_last, is_first=is_first))
        outs.append(res[-1])
        rec.disable_real_time_streaming()
    assert outs[0] == outs[1]


def test_lm_partials_without_a_language_model_raises():
    from danspeech_amd import Recognizer
    rec = Recognizer(model=_stream_model("stream-greedy", 64, 2, 20, seed=87))
    with pytest.raises(ValueError):
        rec.enable_real_time_streaming(streaming_model=rec.danspeech_recognizer.model, lm_partials=True)
