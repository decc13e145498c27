"""GPU tests of the batched streaming pass: dsmi_stream_forward_many / NativeStream.forward_many advance many live
sessions of one unidirectional model by one chunk each, and each session must come out as if it had run alone.
Yardsticks: oracle/streaming.py per session (1e-4 on probabilities, the bound of test_gpu_streaming.py) and the
single-session GPU path (NativeStream.forward, 2e-5); dsmi_features_stream_many against dsmi_features_stream;
Recognizer.stream_recordings against stream_recording."""
import os

import numpy as np
import pytest

from danspeech_amd import synthetic as syn

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def native():
    from danspeech_amd import _native
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    _native.lib()
    return _native


def _cfg(kind, H, L, ctx):
    return dict(conv_layers=2, rnn_type=kind, rnn_hidden_size=H, rnn_layers=L, bidirectional=False, context=ctx)


class _env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _margins(p):
    """smallest top-two margin per frame of probabilities [T, C] (test_gpu_workloads.py's _margins, per frame)"""
    top2 = np.sort(p, axis=-1)[..., -2:]
    return top2[..., 1] - top2[..., 0]


def _feat(T, seed):
    return syn.make_features(1, T, seed=seed)


def _run_schedules(native, m, schedules, oracle=None, seed0=0):
    """Run every session's chunk schedule in lock-step rounds through forward_many (sessions whose schedule is over drop
    out; a session whose schedule is shifted starts later).  -> per session the list of outputs (numpy or None)."""
    n = len(schedules)
    sts = [native.NativeStream(m) for _ in range(n)]
    outs = [[] for _ in range(n)]
    rounds = max(len(s) for s in schedules)
    for r in range(rounds):
        due = [i for i in range(n) if r < len(schedules[i]) and schedules[i][r] is not None]
        feats, first, last = [], [], []
        for i in due:
            k = sum(1 for c in schedules[i][:r] if c is not None)
            chunks = [c for c in schedules[i] if c is not None]
            feats.append(torch.from_numpy(_feat(chunks[k], seed0 + 1000 * i + k)).cuda())
            first.append(k == 0)
            last.append(k == len(chunks) - 1)
        ys = native.NativeStream.forward_many([sts[i] for i in due], feats, first, last)
        for i, y in zip(due, ys):
            outs[i].append(None if y is None else y[0].cpu().numpy())
    for s in sts:
        s.close()
    return outs


def _oracle_outputs(sd, cfg, schedules, seed0=0):
    from oracle import streaming as ost
    res = []
    for i, sch in enumerate(schedules):
        om = ost.StreamingModel(sd, cfg)
        chunks = [c for c in sch if c is not None]
        res.append([(lambda r: None if r is None else r[0])(om.forward(_feat(T, seed0 + 1000 * i + k), k == 0, k == len(chunks) - 1))
                    for k, T in enumerate(chunks)])
    return res


def _single_outputs(native, m, schedules, seed0=0):
    res = []
    for i, sch in enumerate(schedules):
        st = native.NativeStream(m)
        chunks = [c for c in sch if c is not None]
        o = []
        for k, T in enumerate(chunks):
            y = st.forward(torch.from_numpy(_feat(T, seed0 + 1000 * i + k)).cuda(), k == 0, k == len(chunks) - 1)
            o.append(None if y is None else y[0].cpu().numpy())
        st.close()
        res.append(o)
    return res


def _compare(got, want, atol):
    worst = 0.0
    for g, w in zip(got, want):
        assert len(g) == len(w)
        for a, b in zip(g, w):
            assert (a is None) == (b is None)
            if a is not None:
                assert a.shape == b.shape
                worst = max(worst, float(np.abs(a - b).max()))
    assert worst < atol, worst
    return worst


# out-of-phase ragged schedules: None = the session sits this round out (it starts later)
SCHED6 = [
    [53, 39, 40, 38, 39, 17],
    [None, 60, 39, 41, 39, 39, 44, 22],
    [47, 39, 39],
    [None, None, None, 55, 38, 39],
    [41, 42, 43, 44, 45, 46, 47, 12],
    [64, 39, 39, 40, 21],
]


def test_many_vs_oracle_gru_ragged_out_of_phase(native):
    H, L, ctx = 200, 2, 20
    sd = syn.make_state_dict(2, "gru", H, L, bidirectional=False, context=ctx, seed=91, fc_gain=4.0)
    cfg = _cfg("gru", H, L, ctx)
    m = native.NativeModel(cfg, sd)
    got = _run_schedules(native, m, SCHED6, seed0=9100)
    print("gru H=200 vs oracle: %.3g" % _compare(got, _oracle_outputs(sd, cfg, SCHED6, seed0=9100), 1e-4))
    m.close()


@pytest.mark.parametrize("kind", ["lstm", "rnn"])
def test_many_vs_oracle_lstm_rnn(native, kind):
    """LSTM: the second round has chunk lengths that differ inside the batch, followed by more chunks -- the pass that
    catches a c carried from the batch's longest chunk instead of the session's own last frame."""
    H, L, ctx = 64, 3, 8
    sd = syn.make_state_dict(2, kind, H, L, bidirectional=False, context=ctx, seed=92, fc_gain=4.0)
    cfg = _cfg(kind, H, L, ctx)
    m = native.NativeModel(cfg, sd)
    sched = [[40, 21, 39, 33], [45, 57, 38, 30], [None, 50, 39, 41, 9], [39, 30, 70, 12]]
    got = _run_schedules(native, m, sched, seed0=9200)
    print("%s vs oracle: %.3g" % (kind, _compare(got, _oracle_outputs(sd, cfg, sched, seed0=9200), 1e-4)))
    m.close()


def test_many_vs_oracle_cpu_streaming_rnn_shape(native):
    """The CPUStreamingRNN shape (5 x GRU 800, context 20), N = 8, the real-time chunk sizes shifted per session."""
    H, L, ctx = 800, 5, 20
    sd = syn.make_state_dict(2, "gru", H, L, bidirectional=False, context=ctx, seed=93, fc_gain=4.0)
    cfg = _cfg("gru", H, L, ctx)
    m = native.NativeModel(cfg, sd)
    base = [54, 39, 39, 39, 39, 21]
    sched = [[None] * (i % 3) + base[:6 - (i % 2)] + ([15] if i % 2 else []) for i in range(8)]
    got = _run_schedules(native, m, sched, seed0=9300)
    print("CPUStreamingRNN shape vs oracle: %.3g" % _compare(got, _oracle_outputs(sd, cfg, sched, seed0=9300), 1e-4))
    m.close()


def _large_n_vs_single(native, mode):
    H, L, ctx = 96, 2, 20
    sd = syn.make_state_dict(2, "gru", H, L, bidirectional=False, context=ctx, seed=94, fc_gain=8.0)
    env = {"DSMI_RNN_MODE": "steps"} if mode == "steps" else {}
    with _env(**env):
        m = native.NativeModel(_cfg("gru", H, L, ctx), sd)
    for n in (37, 130):
        rng = np.random.default_rng(n)
        sched = [[None] * int(rng.integers(0, 3)) + [int(rng.integers(40, 70))] + [int(v) for v in rng.integers(30, 48, size=int(rng.integers(1, 4)))]
                 + [int(rng.integers(11, 40))] for _ in range(n)]
        got = _run_schedules(native, m, sched, seed0=9400)
        want = _single_outputs(native, m, sched, seed0=9400)
        worst = _compare(got, want, 2e-5)
        # greedy decisions equal except at frames whose top-two margin is below 1e-4
        for g, w in zip(got, want):
            for a, b in zip(g, w):
                if a is not None:
                    diff = a.argmax(-1) != b.argmax(-1)
                    assert not (diff & (_margins(b) >= 1e-4)).any()
        print("%s N=%d vs single-session path: %.3g" % (mode, n, worst))
    m.close()


def test_large_n_vs_single_session_persistent(native):
    _large_n_vs_single(native, "persist")


def test_large_n_vs_single_session_steps(native):
    _large_n_vs_single(native, "steps")


def test_n1_and_switching_paths(native):
    H, L, ctx = 72, 2, 10
    sd = syn.make_state_dict(2, "lstm", H, L, bidirectional=False, context=ctx, seed=95, fc_gain=4.0)
    m = native.NativeModel(_cfg("lstm", H, L, ctx), sd)
    chunks = [50, 39, 41, 38, 40, 25]
    xs = [torch.from_numpy(_feat(T, 9500 + k)).cuda() for k, T in enumerate(chunks)]
    ref, alt = native.NativeStream(m), native.NativeStream(m)
    for k, x in enumerate(xs):
        f, l = k == 0, k == len(xs) - 1
        a = ref.forward(x, f, l)
        b = alt.forward(x, f, l) if k % 2 == 0 else native.NativeStream.forward_many([alt], [x], [f], [l])[0]
        assert (a is None) == (b is None)
        if a is not None:
            np.testing.assert_allclose(b.cpu().numpy(), a.cpu().numpy(), rtol=0, atol=2e-5)
    ref.close(); alt.close(); m.close()


def test_refusals_change_nothing(native):
    H, L, ctx = 48, 2, 8
    sd = syn.make_state_dict(2, "gru", H, L, bidirectional=False, context=ctx, seed=96, fc_gain=4.0)
    cfg = _cfg("gru", H, L, ctx)
    m, m2 = native.NativeModel(cfg, sd), native.NativeModel(cfg, sd)
    a, b, other = native.NativeStream(m), native.NativeStream(m), native.NativeStream(m2)
    ref_a, ref_b = native.NativeStream(m), native.NativeStream(m)
    x = lambda T, s: torch.from_numpy(_feat(T, s)).cuda()
    for st in (a, ref_a):
        st.forward(x(40, 1), True, False)
    for st in (b, ref_b):
        st.forward(x(45, 2), True, False)
    fresh = native.NativeStream(m)
    F = native.DsmiError
    with pytest.raises(F, match="session 1"):
        native.NativeStream.forward_many([a, a], [x(39, 3), x(39, 4)], [False, False], [False, False])
    with pytest.raises(F, match="session 1"):
        native.NativeStream.forward_many([a, other], [x(39, 3), x(39, 4)], [False, True], [False, False])
    with pytest.raises(F, match="session 2"):
        native.NativeStream.forward_many([a, b, fresh], [x(39, 3), x(39, 4), x(39, 5)], [False, False, False], [False, False, False])
    with pytest.raises(F, match="session 1"):
        native.NativeStream.forward_many([a, fresh], [x(39, 3), x(3, 4)], [False, True], [False, False])
    # too small a probs capacity, through the raw C call (forward_many grows its buffer)
    import ctypes as C
    hs = (C.c_void_p * 2)(a._h, b._h)
    f1, f2 = x(39, 3), x(39, 4)
    fp = (C.c_void_p * 2)(f1.data_ptr(), f2.data_ptr())
    T = np.array([39, 39], dtype=np.int32); z = np.zeros(2, dtype=np.int32); tout = np.zeros(2, dtype=np.int32)
    probs = torch.empty((2, 4, m.n_labels), device="cuda")
    rc = native.lib().dsmi_stream_forward_many(hs, 2, fp, native._np_ptr(T), native._np_ptr(z), native._np_ptr(z), probs.data_ptr(), 4,
                                               native._np_ptr(tout), native._stream(m.device))
    assert rc == native.DSMI_ERR_CAPACITY
    # afterwards every session continues exactly as if none of these calls had been made
    for k, (Ta, Tb) in enumerate([(39, 41), (38, 39), (20, 33)]):
        last = k == 2
        xa, xb = x(Ta, 100 + k), x(Tb, 200 + k)
        ya, yb = native.NativeStream.forward_many([a, b], [xa, xb], [False, False], [last, last])
        ra, rb = ref_a.forward(xa, False, last), ref_b.forward(xb, False, last)
        for g, w in ((ya, ra), (yb, rb)):
            assert (g is None) == (w is None)
            if g is not None:
                np.testing.assert_allclose(g.cpu().numpy(), w.cpu().numpy(), rtol=0, atol=2e-5)
    for st in (a, b, other, ref_a, ref_b, fresh):
        st.close()
    m.close(); m2.close()


def test_timed_out_wait_is_recomputed_in_the_same_call(native):
    """DSMI_DEBUG_DROP_SIGNAL / DSMI_DEBUG_SPIN_LIMIT as tests/test_gpu_timeout.py uses them: one workgroup of layer 1 never
    signals step 5; the pass must report it (recompute count) and still equal the oracle."""
    H, L, ctx = 64, 2, 8
    sd = syn.make_state_dict(2, "gru", H, L, bidirectional=False, context=ctx, seed=97, fc_gain=4.0)
    cfg = _cfg("gru", H, L, ctx)
    with _env(DSMI_DEBUG_DROP_SIGNAL="1:2:5", DSMI_DEBUG_SPIN_LIMIT="2000"):
        m = native.NativeModel(cfg, sd)
    sched = [[45, 39, 30], [50, 40, 39]]
    got = _run_schedules(native, m, sched, seed0=9700)
    assert m.recompute_count() >= 1
    _compare(got, _oracle_outputs(sd, cfg, sched, seed0=9700), 1e-4)
    m.close()


def test_features_stream_many_equals_single_calls(native):
    fe = native.NativeFrontend()
    rng = np.random.default_rng(98)
    n = 16
    states_a = [np.zeros(3) for _ in range(n)]
    states_b = [np.zeros(3) for _ in range(n)]
    for rnd in range(3):
        lens = [int(rng.integers(500, 9000)) for _ in range(n)]
        if rnd == 2:
            lens[3] = 400                     # a short last part: still longer than one window
        parts = [np.round(rng.normal(0, 3000, k)) for k in lens]
        got = fe.features_stream_many([torch.from_numpy(p).cuda() for p in parts], states_a)
        for i in range(n):
            want = fe.features_stream(torch.from_numpy(parts[i]).cuda(), states_b[i])
            assert got[i].shape == want.shape
            np.testing.assert_allclose(got[i].cpu().numpy(), want.cpu().numpy(), rtol=0, atol=1e-6)
            np.testing.assert_array_equal(states_a[i], states_b[i])
    fe.close()


def _stream_model(name, H, L, ctx, seed):
    from danspeech_amd.deepspeech.model import DeepSpeech
    sd = syn.make_state_dict(2, "gru", H, L, bidirectional=False, context=ctx, seed=seed, fc_gain=8.0)
    return DeepSpeech(name, rnn_type="gru", rnn_hidden_size=H, rnn_layers=L, conv_layers=2, context=ctx, bidirectional=False,
                      streaming_inference_model=True).load_state_dict(sd)


@pytest.mark.parametrize("chunk,string_parts,secondary", [(1024, True, False), (2048, False, False), (2048, True, True)])
def test_stream_recordings_equals_stream_recording(chunk, string_parts, secondary):
    from danspeech_amd import Recognizer
    from danspeech_amd.deepspeech.model import DeepSpeech
    m = _stream_model("stream-many", 64, 2, 20, seed=99)
    second = None
    if secondary:
        second = DeepSpeech("second", rnn_hidden_size=64, rnn_layers=2).load_state_dict(syn.make_state_dict(2, "gru", 64, 2, seed=100, fc_gain=8.0))
    rec = Recognizer()
    rec.enable_real_time_streaming(streaming_model=m, secondary_model=second, string_parts=string_parts)
    audio = [syn.make_clip(20 + i, 16000 + 5311 * i) for i in range(12)]
    got = list(rec.stream_recordings(audio, chunk_samples=chunk))
    total = 0
    for i, a in enumerate(audio):
        # each session starts from a fresh parser: so does the first recording after enable_real_time_streaming (the streaming
        # parser carries its buffer and statistics from one utterance into the next)
        rec.enable_real_time_streaming(streaming_model=m, secondary_model=second, string_parts=string_parts)
        want = list(rec.stream_recording(a, chunk_samples=chunk))
        assert [(l, t) for k, l, t in got if k == i] == want, i
        total += len(want)
    assert total == len(got) and total >= 12
    rec.disable_real_time_streaming()
