"""What tests/test_gpu_frontend_accuracy.py (GPU) and tests/test_frontend_accuracy_sensitivity.py (CPU) share: the bound's constants,
the case table of the spectrogram front end (danspeech_amd/csrc/features.hip), the seeded signals, the two references, the error
statistics and the message that localises the worst element.  The counterparts are tests/_dense_cases.py (conv stack, head) and
tests/_layer_cases.py (recurrent layers); the rules are the same.

THE BOUND.  Per case and REGION ``e32 = max |fp32 oracle - float64|`` over the region (oracle/features.py against
tests/_f64_ref.py: ``spectrogram`` / ``stream_norm`` on the same sample values, computed on the CPU in the same run, over all clips
of the case) and the assertion ``max |gpu - float64| <= M[family] * e32`` over the same region:

  M["mfma"]    dsmi_features at n_fft 320 with float64 / float32 / int16 samples: stft_mfma_kernel<320, T>, clip_stats_kernel,
               normalize_kernel
  M["direct"]  dsmi_features at every other n_fft and on raw WAV frames: stft_logmag_kernel (+ the same two)
  M["stream"]  dsmi_features_stream / dsmi_features_stream_many (PAD_NONE; either STFT kernel, chunk_stats*_kernel,
               chunk_normalize*_kernel, stream_norm_update)

Regions.  ``raw``: the un-normalised output (a front end made with normalize=False), whole.  ``quiet`` / ``loud``: of a TONE case
the elements of ``raw`` whose float64 reference is below 0.1 / the rest -- a quiet bin is where a float32-accumulated transform
fails first (173 x e32 there, 9 x over the whole output: test_frontend_accuracy_sensitivity.py), and a maximum over the whole
output is the loud bins' e32.  ``norm``: the normalised output (normalize=True), whole.  The streaming calls only have a normalised
output: their regions are ``norm`` and, for tone cases, ``quiet`` / ``loud`` of that output by the same mask (coarser there:
a normalised quiet bin sits near -mean / std, about -3, and its e32 is the float32 rounding of THAT, 3e-7, not of 0.01).  The tone
cases of the streaming calls use the Blackman window, whose main lobe gives them bins at or above 1 in 3 % of the output.

M = the next power of two at or above twice the largest ratio measured on an MI355X over the family's cases and regions (the factor
two: other seeds).  The figures are in tests/frontend_accuracy_measured.json, written by ``DSMI_RECORD_FRONTEND_ACCURACY=1`` (with
the M they give as ``M_derived``).  The tests assert against M, never against that file.  What was measured is at the end.

THE CASES.  16 kHz, n_fft 320, hop 160 unless said; lengths in samples, ``frames = 1 + N // hop`` (PAD_NONE: 1 + (N - n_fft) // hop).
Signals: ``noise`` = synthetic.make_clip (white noise of amplitude 3000 + bursts, int16 scale; fed as float64, float32 and int16);
``tone`` = 0.5 sin(2 pi 1000 t + 0.3) + 5e-4 sin(2 pi 3050 t), unit scale, float64 / float32 (most bins are quiet: the CPU test
asserts at least 50 % of the float64 reference below 0.1 and at least 2 % at or above 1); ``comb`` = impulses of 1000.0 every 161
samples over 172 frames: frame t has them at taps t - 1 and t + 160, so the frames walk an impulse over every tap -- 0, NQ = 80,
NH = 160, 240 and 319, the special ones of the folded forms, among them -- and two impulses in a frame test the twiddle index;
``wav`` = uniform integers over the sample width's whole range with both rails in the first 100 frames (the L + R fold saturates).

Matrix-pipe form (family mfma):
  single clips   N = 161 (2 frames: the shortest clip reflect padding admits), 2559 (16: one wave tile), 2560 (17), 10239 (64: one
                 workgroup), 10240 (65); float32 and int16 at 10240 (stft_mfma_kernel<320, float>, <320, int16_t>)
  ragged         [10240, 2721, 161] in one call: non-zero offsets, workgroups and waves past a clip's last frame; t_stride 70 into a
                 buffer pre-filled with 7.0 (the binding's torch.empty never shows the kernels dirty memory), through ctypes;
                 reflect and constant padding; constant padding also [1, 159, 160]: 1, 1 and 2 frames (un-normalised only: one
                 sample is an impulse, its spectrum is flat and its own standard deviation rounding noise around zero)
  windows        hamming, hann, blackman, bartlett on the tone clip (N = 2721) and on the 65-frame noise clip
  hops           window_stride 0.005 and 0.015: hop 80 and 240 (the generator asserts what int(rate * stride) gives)
  comb           see above

Direct form (family direct): clips of 9, 8 (reflect) and 9, 1, 8 (constant) frames, FT = 8 frames per workgroup, t_stride two past
the longest clip into 7.0:
  8000 Hz   n_fft 160                   the even, folded branch
  22050 Hz  n_fft 441, hop 220          odd: the unfolded branch
  32000 Hz  n_fft 640, n_freq 321       the second trip of the bin loop (k += 256)
  100 Hz    n_fft 2, hop 1              the smallest (no centred clip has one frame there: 8 and 9)
  44100 Hz  n_fft 882, n_freq 442       70560 bytes of dynamic LDS: above the default 64 KB, raised by dsmi_frontend_create
  16 kHz    raw WAV frames of widths 1, 3, 4 mono and 2, 3, 4 stereo against the float64 reference of the DECODED samples
            (tests/_resample_ref.py: decode) -- the direct kernel at n_fft 320 with a reference of its own

Streaming (family stream, PAD_NONE):
  features_stream       one parser fed chunks of 320, 479, 480 (1, 1, 2 frames), 10400 and 10560 samples (64, 65 frames) in turn;
                        float64, float32, int16 (stft_mfma_kernel<320, T> with PAD_NONE); a tone parser; 32000 Hz
  features_stream_many  chunks of 65, 1 and 17 frames in one call, noise and tone, the sessions' states at alpha 0, 0.5 and 0.95 (both
                        branches of the update), through ctypes with t_stride two past the longest into 7.0; 22050 Hz (odd n_fft:
                        NativeFrontend._stream_frames) and 100 Hz with chunks of 1, 8 and 9 frames
  state3                against _f64_ref.stream_norm at rtol 1e-6

MEASURED on the MI355X (tests/frontend_accuracy_measured.json).  The largest ratios: mfma 1.10 (mfma-tone-hann, quiet; 0.67 .. 1.10
over all its regions), direct 1.06 (direct-wav-w2-c2, norm; 0.74 .. 1.06), stream 1.20 (stream-noise-*, norm; 0.63 .. 1.20).  Twice
that is 2.2, 2.1 and 2.4, so M is 4 for all three.  The ratios are near 1 as the code predicts: kernels and oracle round the same
float64 sums to float32 and apply a float32 hypot and log1p -- what differs is those two functions' last bit and, in the normalised
output, the last bit of the float32 mean and std (the streaming 1.20: its mean is 5.5 mixed with the dataset's, rounded once to
float32 on either side).  Nothing is above 8; nothing needed explaining or fixing.
"""
import numpy as np

M = {"mfma": 4.0, "direct": 4.0, "stream": 4.0}

WINDOW_SIZE = 0.02
QUIET = 0.1
FILL = 7.0
DTYPES = {"f64": np.float64, "f32": np.float32, "i16": np.int16}


def _case(name, family, lens, api="features", rate=16000, stride=0.01, hop=None, window="hamming", pad="reflect", signal="noise",
          dtype="f64", t_stride=None, wav=None, alphas=None, norm=True):
    """lens: samples per clip (features: one call; stream: one parser's chunks in turn; stream_many: one call).  t_stride: the time
    pitch of a 7.0-filled buffer handed over through ctypes (None: the binding allocates).  wav: (width, channels).  norm=False: only
    the un-normalised output is compared."""
    n_fft, h = int(rate * WINDOW_SIZE), int(rate * stride)
    assert h == (hop if hop is not None else n_fft // 2), (name, h)
    assert family == ("stream" if api != "features" else "mfma" if n_fft == 320 and wav is None else "direct"), name
    return dict(name=name, family=family, api=api, lens=list(lens), rate=rate, stride=stride, n_fft=n_fft, hop=h, n_freq=n_fft // 2 + 1,
                window=window, pad=pad if api == "features" else "none", signal=signal, dtype=dtype, t_stride=t_stride, wav=wav,
                alphas=alphas, norm=norm)


def _direct(rate, hop, **kw):
    """the direct form's batches at one rate: N = (frames - 1) * hop + a third of a hop"""
    n = lambda fr: (fr - 1) * hop + hop // 3
    tag = "direct-%d" % rate
    out = [_case(tag + "-reflect", "direct", [n(9), n(8)], rate=rate, hop=hop, t_stride=11, **kw)]
    if hop > 1:
        out.append(_case(tag + "-constant", "direct", [n(9), max(n(1), 1), n(8)], rate=rate, hop=hop, pad="constant", t_stride=11, **kw))
    return out


STREAM_CHUNKS = [320, 479, 480, 320 + 160 * 63, 320 + 160 * 64]
MANY_CHUNKS = [320 + 160 * 64, 401, 320 + 160 * 16]
MANY_ALPHAS = [0.0, 0.5, 0.95]

CASES = (
    [_case("mfma-noise-%d" % N, "mfma", [N]) for N in (161, 2559, 2560, 10239, 10240)]
    + [_case("mfma-noise-10240-%s" % d, "mfma", [10240], dtype=d) for d in ("f32", "i16")]
    + [_case("mfma-ragged-%s" % p, "mfma", [10240, 2721, 161], pad=p, t_stride=70) for p in ("reflect", "constant")]
    + [_case("mfma-ragged-reflect-i16", "mfma", [10240, 2721, 161], dtype="i16", t_stride=70)]
    + [_case("mfma-short-constant", "mfma", [1, 159, 160], pad="constant", t_stride=5, norm=False)]
    + [_case("mfma-tone-%s" % w, "mfma", [2721], window=w, signal="tone") for w in ("hamming", "hann", "blackman", "bartlett")]
    + [_case("mfma-tone-hann-f32", "mfma", [2721], window="hann", signal="tone", dtype="f32")]
    + [_case("mfma-noise-10240-%s" % w, "mfma", [10240], window=w) for w in ("hann", "blackman", "bartlett")]
    + [_case("mfma-hop80", "mfma", [2721, 161], stride=0.005, hop=80, t_stride=40),
       _case("mfma-hop240", "mfma", [2721, 161], stride=0.015, hop=240, t_stride=14)]
    + [_case("mfma-comb", "mfma", [171 * 160], signal="comb")]
    + _direct(8000, 80) + _direct(22050, 220) + _direct(32000, 320) + _direct(100, 1) + _direct(44100, 441)
    + [_case("direct-22050-blackman-tone", "direct", [2721], rate=22050, hop=220, window="blackman", signal="tone", dtype="f32")]
    + [_case("direct-wav-w%d-c%d" % wc, "direct", [1777, 161], signal="wav", wav=wc, t_stride=14)
       for wc in ((1, 1), (3, 1), (4, 1), (2, 2), (3, 2), (4, 2))]
    + [_case("stream-noise-%s" % d, "stream", STREAM_CHUNKS, api="stream", dtype=d) for d in ("f64", "f32", "i16")]
    + [_case("stream-tone-f32", "stream", [479, 320 + 160 * 63, 320 + 160 * 64], api="stream", signal="tone", dtype="f32", window="blackman")]
    + [_case("stream-32000", "stream", [640 + 320 * 8, 640], api="stream", rate=32000, hop=320)]
    + [_case("stream-many-%s" % s, "stream", MANY_CHUNKS, api="stream_many", signal=s, t_stride=67, alphas=MANY_ALPHAS,
             window="blackman" if s == "tone" else "hamming") for s in ("noise", "tone")]
    + [_case("stream-many-noise-i16", "stream", MANY_CHUNKS, api="stream_many", dtype="i16", alphas=MANY_ALPHAS)]
    + [_case("stream-many-22050", "stream", [441, 660, 441 + 220 * 8], api="stream_many", rate=22050, hop=220, t_stride=11, alphas=MANY_ALPHAS),
       _case("stream-many-100", "stream", [2, 9, 10], api="stream_many", rate=100, hop=1, t_stride=11, alphas=MANY_ALPHAS)])
assert len({c["name"] for c in CASES}) == len(CASES)
BY_NAME = {c["name"]: c for c in CASES}
LDS_REFUSED = dict(sampling_rate=192000, window_size=WINDOW_SIZE)       # n_fft 3840: 307200 bytes of LDS per workgroup


def audio_conf(c, normalize):
    return dict(sampling_rate=c["rate"], window_size=WINDOW_SIZE, window_stride=c["stride"], window=c["window"], normalize=normalize)


def frame_count(c, N):
    return 1 + (N - c["n_fft"]) // c["hop"] if c["pad"] == "none" else 1 + N // c["hop"]


def make_signal(c, i, N):
    """clip i of the case: (what the front end is given -- a numpy array of the case's dtype, or the bytes of raw WAV frames --,
    the sample values the references see: float64 / float32 as they are, WAV frames decoded to int64)"""
    from danspeech_amd import synthetic as syn
    if c["signal"] == "wav":
        import _resample_ref as rr
        width, channels = c["wav"]
        lim = 1 << (8 * width - 1)
        v = np.random.default_rng(500 + 10 * width + channels + 100 * i).integers(-lim, lim, size=(N, channels))
        v[:50] = lim - 1
        v[50:100] = -lim
        raw = rr.encode(v.reshape(-1), width)
        return raw, rr.decode(raw, width, channels)
    if c["signal"] == "noise":
        x = syn.make_clip(40 + i, N)
    elif c["signal"] == "tone":
        t = np.arange(N) / float(c["rate"]) + i * 0.37
        x = 0.5 * np.sin(2 * np.pi * 1000.0 * t + 0.3) + 5e-4 * np.sin(2 * np.pi * 3050.0 * t)
    else:
        assert c["signal"] == "comb", c["signal"]
        x = np.zeros(N)
        x[::161] = 1000.0
    x = x.astype(DTYPES[c["dtype"]])
    assert c["dtype"] != "i16" or c["signal"] == "noise"
    return x, x


def make_case(c):
    """-> (fed: list per clip, values: list per clip)"""
    pairs = [make_signal(c, i, N) for i, N in enumerate(c["lens"])]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def _oracle_stream(raw32, state):
    """oracle/streaming.py: StreamingParser.parse_audio's arithmetic on a float32 log1p|D| (np.mean / np.std of a float32 array are
    float32 values; the running statistics are Python floats)"""
    import _f64_ref as f64
    state[2] += f64.ALPHA_INCREMENT
    state[0] = (state[0] + float(np.mean(raw32))) / 2
    state[1] = (state[1] + float(np.std(raw32))) / 2
    mean, std = state[0], state[1]
    if state[2] < 1.0:
        mean = state[0] * state[2] + (1 - state[2]) * f64.DATASET_MEAN
        std = state[1] * state[2] + (1 - state[2]) * f64.DATASET_STD
    out = raw32.copy()
    out -= np.float32(mean)
    out /= np.float32(std)
    return out


def references(c, values):
    """Per clip the float64 reference and the fp32 oracle: dict(raw=[...], norm=[...], o_raw=[...], o_norm=[...], states=[...]).
    Streaming cases: ``norm`` is the parser's output and ``states`` the float64 state3 after each chunk."""
    import _f64_ref as f64
    from oracle import features as of
    kw64 = dict(n_fft=c["n_fft"], hop=c["hop"], window=c["window"], pad=c["pad"])
    kw32 = dict(sample_rate=c["rate"], window_size=WINDOW_SIZE, window_stride=c["stride"], pad_mode=c["pad"], window=c["window"])
    R = dict(raw=[], norm=[], o_raw=[], o_norm=[], states=[])
    s64, s32 = np.zeros(3), [0.0, 0.0, 0.0]
    for i, v in enumerate(values):
        raw = f64.spectrogram(v, normalize=False, **kw64)
        o_raw = of.spectrogram(f64.samples_f64(v), normalize=False, **kw32)
        assert raw.shape == o_raw.shape == (c["n_freq"], frame_count(c, len(v))), (c["name"], raw.shape, o_raw.shape)
        R["raw"].append(raw)
        R["o_raw"].append(o_raw)
        if c["api"] == "features" and not c["norm"]:
            continue
        if c["api"] == "features":
            R["norm"].append(f64.spectrogram(v, normalize=True, **kw64))
            R["o_norm"].append(of.spectrogram(f64.samples_f64(v), normalize=True, **kw32))
            continue
        if c["api"] == "stream_many":       # every chunk is a session of its own
            s64, s32 = np.array([0.0, 0.0, c["alphas"][i]]), [0.0, 0.0, c["alphas"][i]]
        s64, mean, std = f64.stream_norm((raw.mean(), raw.std()), s64)
        R["norm"].append((raw - mean) / std)
        R["states"].append(s64.copy())
        R["o_norm"].append(_oracle_stream(o_raw, s32))
    return R


def regions(c, R):
    """-> {region: (which output: "raw" / "norm", [bool mask per clip])}"""
    whole = [np.ones(r.shape, dtype=bool) for r in R["raw"]]
    out = {"norm": ("norm", whole)} if c["norm"] else {}
    src = "raw"
    if c["api"] == "features":
        out["raw"] = ("raw", whole)
    else:
        src = "norm"
    if c["signal"] == "tone":
        out["quiet"] = (src, [r < QUIET for r in R["raw"]])
        out["loud"] = (src, [r >= QUIET for r in R["raw"]])
    return out


def tone_shares(R):
    v = np.concatenate([r.ravel() for r in R["raw"]])
    return float((v < QUIET).mean()), float((v >= 1.0).mean())


def region_error(got, ref, masks):
    """(max, rms) of |got - ref| over the masked elements of all clips"""
    d = np.concatenate([(np.asarray(g, dtype=np.float64) - r)[m] for g, r, m in zip(got, ref, masks)])
    if d.size == 0:
        return 0.0, 0.0
    return float(np.abs(d).max()), float(np.sqrt((d ** 2).mean()))


def _ratio(gpu_max, e32):
    return gpu_max / e32 if e32 > 0 else (0.0 if gpu_max == 0 else float("inf"))


def localise(c, got, ref, masks):
    """Where the worst element is, in the units the STFT kernels are built from."""
    errs = [np.where(m, np.nan_to_num(np.abs(np.asarray(g, dtype=np.float64) - r), nan=np.inf), 0.0) for g, r, m in zip(got, ref, masks)]
    b = int(np.argmax([e.max() if e.size else 0.0 for e in errs]))
    err = errs[b]
    k, t = (int(v) for v in np.unravel_index(int(err.argmax()), err.shape))
    N, n_fft, hop, nh = c["lens"][b], c["n_fft"], c["hop"], c["n_fft"] // 2
    mfma = n_fft == 320 and c["wav"] is None
    start = t * hop - (0 if c["pad"] == "none" else nh)
    touches = "/".join(s for s, on in (("the left padding", start < 0), ("the right padding", start + n_fft > N)) if on) or "no padding"
    wg = 64 if mfma else 8
    if mfma:
        bins = "bin NH (vector pipe)" if k == nh else "%s tile %d of sixteen, row %d" % ("odd" if k & 1 else "even", (k // 2) // 16, (k // 2) % 16)
        tiles = ["%s%d: %.2g" % (p, j, float(err[par:nh:2][16 * j:16 * j + 16].max())) for par, p in ((0, "even"), (1, "odd")) for j in range(nh // 32)]
        tiles.append("NH: %.2g" % float(err[nh].max()))
    else:
        bins = "trip %d of the bin loop, thread %d (%s branch)" % (k // 256, k % 256, "unfolded" if n_fft & 1 else "folded")
        tiles = ["%d: %.2g" % (j // 16, float(err[j:j + 16].max())) for j in range(0, err.shape[0], 16)][:48]
    per_wg = ["%.2g" % float(err[:, j:j + wg].max()) for j in range(0, err.shape[1], wg)][:32]
    return ("%s (%s kernel, n_fft %d, hop %d, %s window, %s padding, %s %s): worst element %.3g at clip %d (%d samples, %d frames), frame %d "
            "(%d-frame workgroup %d, 16-frame wave tile %d, 8-frame group %d; touches %s), bin %d (%s); got %.9g, float64 %.9g; "
            "max error per %d-frame workgroup %s; per bin tile of sixteen %s"
            % (c["name"], "matrix-pipe" if mfma else "direct", n_fft, hop, c["window"], c["pad"], c["signal"], c["wav"] or c["dtype"], err[k, t], b, N,
               err.shape[1], t, wg, t // wg, t // 16, t // 8, touches, k, bins, np.asarray(got[b])[k, t], ref[b][k, t], wg, per_wg, tiles))


# ---- the GPU side ------------------------------------------------------------------------------------------------------------------
def _upload(c, fed):
    import torch
    if c["wav"] is not None:
        return torch.from_numpy(np.frombuffer(b"".join(fed), dtype=np.uint8).copy()).cuda()
    return torch.from_numpy(np.ascontiguousarray(np.concatenate(fed))).cuda()


def _split(c, feat, fr):
    """[B, F, t_stride] -> (per clip [F, frames], the largest |value| at t >= frames over all clips; NaN counts as dirty)"""
    outs = [feat[b, :, :int(fr[b])] for b in range(len(fr))]
    tails = [feat[b, :, int(fr[b]):] for b in range(len(fr))]
    tail = max([float(np.abs(np.nan_to_num(t, nan=np.inf)).max()) for t in tails if t.size] or [0.0])
    return outs, tail


def gpu_features(c, fed, normalize):
    """dsmi_features on the case's clips with a front end of its own.  -> (per clip [F, frames] float32, frames, tail max)"""
    import torch
    from danspeech_amd import _native
    fe = _native.NativeFrontend(audio_conf(c, normalize), pad_mode=c["pad"])
    try:
        pcm = _upload(c, fed)
        n = np.array(c["lens"], dtype=np.int64)
        if c["t_stride"] is None:
            feat, fr = fe.features(pcm, n, wav_format=c["wav"])
            feat = feat[:, 0]
        else:
            dt = _native._pcm_code(pcm.dtype, c["wav"], n.sum(), pcm.numel())
            feat = torch.full((len(n), c["n_freq"], c["t_stride"]), FILL, dtype=torch.float32, device="cuda")
            fr = np.full(len(n), -1, dtype=np.int32)
            fe._check(_native.lib().dsmi_features(fe._h, pcm.data_ptr(), dt, _native._np_ptr(n), len(n), feat.data_ptr(), c["t_stride"],
                                                  _native._np_ptr(fr), _native._stream(fe.device)))
        torch.cuda.synchronize()
        outs, tail = _split(c, feat.cpu().numpy(), fr)
        return outs, [int(v) for v in fr], tail
    finally:
        fe.close()


def gpu_stream(c, fed):
    """The case's chunks through dsmi_features_stream (one parser, in turn) or dsmi_features_stream_many (one call).
    -> (per chunk [F, frames] float32, frames, tail max, state3 after each chunk)"""
    import torch
    from danspeech_amd import _native
    fe = _native.NativeFrontend(audio_conf(c, True))
    try:
        L = _native.lib()
        if c["api"] == "stream":
            assert c["t_stride"] is None
            state, outs, states = np.zeros(3, dtype=np.float64), [], []
            for x in fed:
                outs.append(fe.features_stream(torch.from_numpy(x).cuda(), state).cpu().numpy())
                states.append(state.copy())
            return outs, [o.shape[1] for o in outs], 0.0, states
        states = [np.array([0.0, 0.0, a]) for a in c["alphas"]]
        if c["t_stride"] is None:
            outs = [o.cpu().numpy() for o in fe.features_stream_many([torch.from_numpy(x).cuda() for x in fed], states)]
            return outs, [o.shape[1] for o in outs], 0.0, states
        pcm = _upload(c, fed)
        n = np.array(c["lens"], dtype=np.int64)
        st = np.ascontiguousarray(np.stack(states))
        feat = torch.full((len(n), c["n_freq"], c["t_stride"]), FILL, dtype=torch.float32, device="cuda")
        fr = np.full(len(n), -1, dtype=np.int32)
        fe._check(L.dsmi_features_stream_many(fe._h, pcm.data_ptr(), _native._pcm_code(pcm.dtype), _native._np_ptr(n), len(n), _native._np_ptr(st),
                                              feat.data_ptr(), c["t_stride"], _native._np_ptr(fr), _native._stream(fe.device)))
        torch.cuda.synchronize()
        outs, tail = _split(c, feat.cpu().numpy(), fr)
        return outs, [int(v) for v in fr], tail, list(st)
    finally:
        fe.close()


def run_on_gpu(c):
    """One case on the GPU: the record (figures per region) and what the test asserts beyond the bound.  One handle at a time."""
    fed, values = make_case(c)
    R = references(c, values)
    got = {}
    rec = dict(name=c["name"], family=c["family"], ref_frames=[r.shape[1] for r in R["raw"]], frames={}, tail_max={}, nan={}, regions={})
    if c["api"] == "features":
        for key, normalize in (("raw", False), ("norm", True))[:1 + c["norm"]]:
            got[key], rec["frames"][key], rec["tail_max"][key] = gpu_features(c, fed, normalize)
    else:
        got["norm"], rec["frames"]["norm"], rec["tail_max"]["norm"], states = gpu_stream(c, fed)
        rec["state_rel_err"] = max(float(np.abs((np.asarray(s) - r) / np.where(r == 0, 1.0, r)).max()) for s, r in zip(states, R["states"]))
    for key in got:
        rec["nan"][key] = bool(any(np.isnan(g).any() for g in got[key]))
    shapes_ok = all(rec["frames"][key] == rec["ref_frames"] for key in got)
    for name, (src, masks) in sorted(regions(c, R).items()):
        e32, e32_rms = region_error(R["o_" + src], R[src], masks)
        if shapes_ok:
            gpu_max, gpu_rms = region_error(got[src], R[src], masks)
            where = localise(c, got[src], R[src], masks)
        else:
            gpu_max, gpu_rms, where = float("inf"), float("inf"), "frame counts %s, the reference's %s" % (rec["frames"], rec["ref_frames"])
        if gpu_max != gpu_max:
            gpu_max = float("inf")
        rec["regions"][name] = dict(elements=int(sum(int(m.sum()) for m in masks)), e32=e32, e32_rms=e32_rms, gpu_max=gpu_max, gpu_rms=gpu_rms,
                                    ratio=_ratio(gpu_max, e32), where=where)
    return rec
