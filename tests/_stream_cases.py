"""What tests/test_gpu_stream_accuracy.py (GPU) and tests/test_stream_accuracy_sensitivity.py (CPU) share: the bound's constants, the
case table of the streaming passes (dsmi_stream_forward, dsmi_stream_forward_many), the seeded chunks, both CPU references, the error
statistics and the message that localises the worst element.  The offline stages' counterparts are tests/_layer_cases.py and
tests/_dense_cases.py; the rules are the same.

THE BOUND.  Per case ``e32 = max |fp32 oracle - float64|`` over every probability the case's whole schedule yields
(oracle/streaming.py against tests/_f64_ref.py stream_model on the same float32 chunks, computed on the CPU in the same run) and the
assertion ``max |gpu - float64| <= M[family] * e32``:

  M["stream_split"]  the batched pass with rnn_persist.hip's carried-state kernel (``persist8``: split-fp16 recurrent product)
  M["stream_f32"]    every pass whose recurrent layers run per step (``steps``: rnn_step.hip, fp32 MFMA): the single-session call,
                     shapes the persistent kernel does not take, DSMI_RNN_MODE=steps

The test was first run at M = 32 for both families, the largest margin any stage of this composition already carries
(_dense_cases.M for the conv stack and the head; the recurrent layers have 4): a constant of the project's, not of the code under
test.  Every case passed far below it, so M was lowered by the project's rule, the next power of two at or above twice the largest
ratio measured on an MI355X over the family's cases (the factor two: other seeds): the largest ratios were 2.43 (stream_split:
hot-look-rnn-H64-N3, lookahead outputs up to 20 in front of the head, e32 1.1e-6; next 1.84, carry-rnn-H64-N3-f161; the other 47
cases 0.46 .. 1.42) and 0.995 (stream_f32: steps-lstm-H20-N3; the other seven 0.58 .. 0.93), so M is 8 and 2.  Absolute errors are
1.1e-8 .. 3.5e-8 wherever the lookahead stays inside its clamps: the probabilities' float32 resolution, as the oracle's.  The
figures per case are in tests/stream_accuracy_measured.json, written by ``DSMI_RECORD_STREAM_ACCURACY=1`` (with the M they give as
``M_derived``); the tests assert against M, never against that file.  M may rise only by the same rule and only while
tests/test_stream_accuracy_sensitivity.py still holds: its smallest mutant is at 40 x e32, so M = 16 is the most that passes there.

WHICH KERNEL.  Every case names the kernel its recurrent layers must run on, ``persist8`` or ``steps``, and the GPU test reads it
back from ``NativeModel.last_rnn_plan()`` after every call: a pass that fell back to the per-step path (launch_rnn_persist refused,
or a timed-out pass was recomputed: ``recompute_count()``) fails its case instead of passing it on the other kernel.
``rnn_persist_kernel<KIND, NPW, MULTI, false, CARRY = true>`` has 24 instantiations (rnn_persist.hip: launch_kind): the kind, the
k-pairs per wave NPW in {2, 4, 7, 10} (``npw_class``: H up to 256 / 512 / 896 / 1280) and MULTI (more than 32 sessions in the pass);
test_stream_accuracy_sensitivity.py asserts from this table alone that a case names each of them.

CHUNK ARITHMETIC (stream.hip; ``chunk_tc``).  ``to1 = (tin1 - 1) // 2 + 1`` and ``Tc = tin2``: a first chunk has tin1 = 5 + T and
tin2 = 5 + to1 (T = 5: Tc = 10, the shortest that fills the ten-frame conv context); a middle chunk tin1 = 10 + T, tin2 = 10 + to1
(T = 1: Tc = 16); a last chunk tin1 = 15 + T, tin2 = 15 + to1 (T = 1: Tc = 23); T = 39 / 40 give Tc = 35 (odd: the packed state's
parity flips), T = 41 gives 36.  ``walk`` restates the lookahead's bookkeeping on top (rows carried, frames yielded) from
oracle/streaming.py's documentation; the CPU test holds it to the float64 model, the GPU test to the frames the GPU yields.

THE CASES.  A schedule is a session's list of rounds: None (the session sits the round out) or (T, is_first, is_last).  ``utt``
writes one utterance.  Session i gets ``scheds[i % len(scheds)]``; its chunk k is ``make_features(1, T, n_freq, SEED0 + 1000 i + k)``,
as the existing streaming tests seed them.  Weights: seed 91, fc_gain 4.  Shapes are the smallest that take their branch:

  carry-*   every CARRY instantiation: GRU at both edges of every NPW class (8: waves without a k-pair; 256; 264: nq = 33, odd;
            512; 520: nq = 65; 896; 904: nq = 113; 1280), LSTM and RNN at one width per class, each at N 3 (one tile) and N 33
            (two tiles, the second holding one session: the per-tile st_h / st_c of tiles 1 and up), GRU 264 at N 64 and LSTM 64
            at N 96.  The wide ones run the SHORT schedule (5, 1, 1: Tc 10, 16, 23 -- every chunk edge, and a lookahead that keeps
            ``min(Tc, context - 1) = 16`` rows, limited by Tc) at n_freq 2 so that the float64 reference stays cheap; one case per
            kind runs at 161 bins (K = 1312, GEMM_A_CONV at B = n) on real-time sizes (53, then about 39).
  tiles-*   LSTM, 70 sessions in three tiles, three schedules interleaved so that the chunk lengths differ inside every tile, then
            more chunks: the pass that catches a ``c`` taken from the batch's longest chunk instead of the session's own last step.
  phase-*   sessions that start in later rounds; one that ends and starts its next utterance on the same handle while its
            neighbours are mid-utterance; one that sends is_first with no is_last before it (the conv context and the lookahead
            restart, h / c do not); sessions that buffer in a round where others emit; round 0, in which nobody emits.
  edge-*    contexts 1 (the reference keeps ``x[-0:]``, the whole chunk, and yields it a second time), 2 and 20 on the SHORT
            schedule and on odd / even Tc.
  n256, n257  eight tiles (kMaxMany), and the Python layer's split into two passes (256 + 1), at H 8.
  steps-*   H 100 GRU and H 20 LSTM (H % 8 != 0: not eligible, and Hs != H takes the memset branch), H 96 under
            DSMI_RNN_MODE=steps at N 1 and N 33, and ``dsmi_stream_forward`` itself for the three kinds: two utterances on one
            handle, odd and even Tc (the parity offset ``pbase``).
  hot-look  the lookahead's weights times LOOK_GAIN: both clamps of the lookahead are hit (asserted on the CPU from the reference).
"""
import numpy as np

from _dense_cases import AUDIO, _env

M = {"stream_split": 8.0, "stream_f32": 2.0}
FAMILY = {"persist8": "stream_split", "steps": "stream_f32"}
SEED0 = 9100
LOOK_GAIN = 80.0
STEPS_ENV = {"DSMI_RNN_MODE": "steps"}


def utt(*Ts):
    """one utterance: its chunk lengths -> [(T, is_first, is_last)]"""
    assert len(Ts) >= 2
    return [(T, k == 0, k == len(Ts) - 1) for k, T in enumerate(Ts)]


def chunk_tc(T, first, last):
    """recurrent steps of a chunk of T feature frames (stream.hip: tin2)"""
    ctxl, padl, padr = (0 if first else 10), (5 if first else 0), (5 if last and not first else 0)
    to1 = (ctxl + padl + T + padr - 1) // 2 + 1
    return ctxl + padl + to1 + padr


assert [chunk_tc(5, True, False), chunk_tc(1, False, False), chunk_tc(1, False, True)] == [10, 16, 23]
assert [chunk_tc(T, False, False) for T in (39, 40, 41)] == [35, 35, 36]


def npw_class(H):
    """k-pairs per wave of rnn_persist_kernel at width H (launch_kind): 2, 4, 7 or 10; None: not eligible"""
    if H % 8:
        return None
    npw = -(-(-(-(H // 8) // 2)) // 8)
    return next((n for n in (2, 4, 7, 10) if npw <= n), None)


def expected_kernel(H, path):
    return "persist8" if path == "many" and npw_class(H) is not None else "steps"


SHORT = utt(5, 1, 1)
REAL = utt(53, 39, 40, 41, 17)


def _case(name, kind, H, N, scheds, layers=2, context=20, n_freq=2, path="many", look_gain=1.0, sens=False):
    assert path in ("forward", "many", "many_steps")
    kernel = expected_kernel(H, path)
    return dict(name=name, kind=kind, H=H, layers=layers, context=context, n_freq=n_freq, N=N, scheds=scheds, path=path, kernel=kernel,
                family=FAMILY[kernel], look_gain=look_gain, sens=sens)


def _carry(kind, H, N, **kw):
    wide = H > 256
    kw.setdefault("n_freq", 2)
    return _case("carry-%s-H%d-N%d-f%d" % (kind, H, N, kw["n_freq"]), kind, H, N, [SHORT if wide else REAL], **kw)


TILES = [utt(53, 39, 40, 17), utt(53, 41, 1, 30), utt(47, 20, 39, 9)]
PHASE = [
    utt(53, 39, 40, 17),
    [None, None] + utt(53, 39, 17),                                               # starts in round 2, buffers while others emit
    utt(53, 17) + utt(47, 39, 21),                                                # ends, and starts again on the same handle
    [(53, True, False), (39, False, False), (45, True, False), (39, False, False), (17, False, True)],      # is_first, no is_last before it
    [None] + utt(60, 1, 41, 22),
]
EDGES = [SHORT, utt(39, 40, 41, 39, 1)]
TWICE = [utt(53, 39, 40, 17) + utt(47, 41, 39, 21)]

CASES = (
    [_carry("gru", H, N, sens=(H in (8, 264) and N == 33)) for H in (8, 256, 264, 512, 520, 896, 904, 1280) for N in (3, 33)]
    + [_carry("lstm", H, N) for H in (8, 512, 520, 1280) for N in (3, 33)]
    + [_carry("rnn", H, N) for H in (256, 264, 896, 904) for N in (3, 33)]
    + [_carry("gru", 264, 64), _carry("lstm", 64, 96)]
    + [_carry(kind, 64, 3, n_freq=161) for kind in ("gru", "lstm", "rnn")]
    + [_case("tiles-lstm-H%d-N70" % H, "lstm", H, 70, TILES, layers=3 if H == 64 else 2, context=8, sens=(H == 64)) for H in (64, 264)]
    + [_case("phase-%s-H64-N5" % kind, kind, 64, 5, PHASE, layers=3, context=8, sens=True) for kind in ("gru", "lstm", "rnn")]
    + [_case("edge-gru-H64-N4-ctx%d" % ctx, "gru", 64, 4, EDGES, context=ctx, sens=True) for ctx in (1, 2, 20)]
    + [_case("edge-lstm-H64-N33-ctx2", "lstm", 64, 33, [utt(39, 40, 41, 1)], context=2, sens=True)]
    + [_case("n256", "gru", 8, 256, [SHORT]), _case("n257", "gru", 8, 257, [SHORT])]
    + [_case("steps-gru-H100-N3", "gru", 100, 3, [REAL]), _case("steps-lstm-H20-N3", "lstm", 20, 3, [REAL], sens=True),
       _case("steps-gru-H96-N1-env", "gru", 96, 1, [REAL], path="many_steps"),
       _case("steps-gru-H96-N33-env", "gru", 96, 33, [REAL], path="many_steps", sens=True)]
    + [_case("steps-%s-H64-single" % kind, kind, 64, 1, TWICE, layers=3, context=8, path="forward") for kind in ("gru", "lstm", "rnn")]
    + [_case("steps-gru-H100-single", "gru", 100, 2, TILES[:2], path="forward")]
    + [_case("hot-look-rnn-H64-N3", "rnn", 64, 3, [REAL], context=20, look_gain=LOOK_GAIN)])
assert len({c["name"] for c in CASES}) == len(CASES)


def passes(c):
    """session counts of the native passes a round of all N sessions is cut into (the Python layer: 256 at most)"""
    return [min(256, c["N"] - k) for k in range(0, c["N"], 256)] if c["path"] != "forward" else [1]


def sessions(c):
    return [c["scheds"][i % len(c["scheds"])] for i in range(c["N"])]


def walk(c, sched):
    """One session's schedule by the chunk arithmetic alone: per chunk dict(round, k, T, first, last, Tc, la_rows (carried lookahead
    rows its output starts with), nout (frames yielded; 0: the pass buffers))."""
    ctx, la, out, k = c["context"], None, [], 0
    for r, e in enumerate(sched):
        if e is None:
            continue
        T, first, last = e
        Tc = chunk_tc(T, first, last)
        if la is None or first:
            row, la = dict(la_rows=0, nout=0), Tc
        else:
            ncat = la + Tc
            row = dict(la_rows=la, nout=ncat if last else ncat - (ctx - 1))
            la = None if last else (Tc if ctx == 1 else min(Tc, ctx - 1))      # x[-(context - 1):]; context 1: x[-0:]
        row.update(round=r, k=k, T=T, first=first, last=last, Tc=Tc)
        out.append(row)
        k += 1
    return out


def make_case(c):
    """(cfg, state_dict, audio_conf)"""
    from danspeech_amd import synthetic as syn
    ac = AUDIO[c["n_freq"]] or {}
    cfg = dict(conv_layers=2, rnn_type=c["kind"], rnn_hidden_size=c["H"], rnn_layers=c["layers"], bidirectional=False, context=c["context"])
    sd = syn.make_state_dict(2, c["kind"], c["H"], c["layers"], bidirectional=False, context=c["context"], seed=91, fc_gain=4.0,
                             sample_rate=ac.get("sampling_rate", 16000), window_size=ac.get("window_size", 0.02))
    if c["look_gain"] != 1.0:
        sd["lookahead.0.conv.weight"] = sd["lookahead.0.conv.weight"] * np.float32(c["look_gain"])
    return cfg, sd, AUDIO[c["n_freq"]]


def feat(c, i, k, T):
    from danspeech_amd import synthetic as syn
    return syn.make_features(1, T, n_freq=c["n_freq"], seed=SEED0 + 1000 * i + k)


def groups(c):
    """[(schedule, [session indices])]: the sessions of one schedule advance in lock step, so a reference runs them as one batch"""
    res = []
    for s in c["scheds"][:c["N"]]:
        res.append((s, [i for i in range(c["N"]) if c["scheds"][i % len(c["scheds"])] is s]))
    return res


def run_reference(c, sd, cfg, model, probe=None):
    """Every session's outputs, [N][chunks] of [T_out, C] arrays or None, from `model(sd, cfg, schedule, members)` -> an object
    with forward(x [B, 1, F, T], is_first, is_last) (the float64 stream_model or the fp32 oracle's StreamingModel), one batch per
    schedule.  probe(model): called after every forward."""
    outs = [None] * c["N"]
    for sched, members in groups(c):
        m = model(sd, cfg, sched, members)
        per = [[] for _ in members]
        for k, (T, first, last) in enumerate(e for e in sched if e is not None):
            y = m.forward(np.concatenate([feat(c, i, k, T) for i in members], axis=0), first, last)
            if probe is not None:
                probe(m)
            for j in range(len(members)):
                per[j].append(None if y is None else y[j])
        for j, i in enumerate(members):
            outs[i] = per[j]
    return outs


def references(c, sd, cfg):
    """(float64 outputs, fp32 oracle outputs)"""
    import _f64_ref as f64
    from oracle import streaming as ost
    return (run_reference(c, sd, cfg, lambda sd, cfg, sched, members: f64.stream_model(sd, cfg)),
            run_reference(c, sd, cfg, lambda sd, cfg, sched, members: ost.StreamingModel(sd, cfg)))


def shape_of(outs):
    """where outputs and None are, and how many frames: [N][chunks] of int (0: None)"""
    return [[0 if y is None else int(y.shape[0]) for y in per] for per in outs]


def distance(got, ref):
    """max |got - ref| over the frames both have (a mutant may yield fewer or more frames: the leading ones are compared);
    inf where one side yields nothing and the other something."""
    worst = 0.0
    for g, r in zip(got, ref):
        assert len(g) == len(r)
        for a, b in zip(g, r):
            if (a is None) != (b is None):
                return float("inf")
            if a is not None:
                n = min(a.shape[0], b.shape[0])
                worst = max(worst, float(np.abs(np.asarray(a[:n], dtype=np.float64) - b[:n]).max()))
    return worst


def localise(c, got, ref):
    """Where the worst element is, in the units the batched pass is built from."""
    if shape_of(got) != shape_of(ref):
        bad = [(i, k, a, b) for i, (ga, ra) in enumerate(zip(shape_of(got), shape_of(ref))) for k, (a, b) in enumerate(zip(ga, ra)) if a != b]
        return "frames yielded differ from the reference's at (session, chunk, got, reference): %s" % bad[:8]
    plans = [walk(c, s) for s in sessions(c)]
    rounds = max(len(s) for s in sessions(c))
    per_session, per_round, worst = [0.0] * c["N"], [0.0] * rounds, (-1.0,)
    for i, (ga, ra) in enumerate(zip(got, ref)):
        for k, (a, b) in enumerate(zip(ga, ra)):
            if a is None:
                continue
            err = np.abs(a.astype(np.float64) - b)
            e = float(err.max())
            per_session[i] = max(per_session[i], e)
            per_round[plans[i][k]["round"]] = max(per_round[plans[i][k]["round"]], e)
            if e > worst[0]:
                t, cl = (int(v) for v in np.unravel_index(int(err.argmax()), err.shape))
                worst = (e, i, k, t, cl, float(a[t, cl]), float(b[t, cl]))
    if worst[0] < 0:
        return "the case yields nothing"
    e, i, k, t, cl, gv, rv = worst
    p = plans[i][k]
    order = np.argsort(per_session)[::-1][:6]
    return ("worst element %.3g at session %d (tile %d, position %d of it; %d sessions in tiles of 32), round %d, its chunk %d (T %d%s%s: %d steps), "
            "frame %d of %d (%s), class %d; got %.9g, float64 %.9g; max error per round %s; largest per session %s"
            % (e, i, i // 32, i % 32, c["N"], p["round"], k, p["T"], ", is_first" if p["first"] else "", ", is_last" if p["last"] else "", p["Tc"],
               t, p["nout"], "from the %d carried lookahead rows" % p["la_rows"] if t < p["la_rows"] else "from the chunk's new rows", cl, gv, rv,
               ["%.2g" % v for v in per_round], ["%d: %.2g" % (j, per_session[j]) for j in order]))


def run_on_gpu(c):
    """One case on the GPU in this process: the record (figures, the kernels that ran) and the message for a failure.  One model
    handle, closed in `finally`."""
    import torch
    from danspeech_amd import _native
    cfg, sd, ac = make_case(c)
    scheds = sessions(c)
    with _env(STEPS_ENV if c["path"] == "many_steps" else {}):      # DSMI_RNN_MODE is read when the model is created
        m = _native.NativeModel(cfg, sd, audio_conf=ac)
    sts, kernels, launches = [], set(), set()
    got = [[] for _ in scheds]
    dev = lambda i, k, T: torch.from_numpy(feat(c, i, k, T)).cuda()

    def note():      # what the pass's last recurrent layer recorded
        x16, plan = m.last_rnn_plan()
        kernels.update(l["kernel"] for l in plan)
        launches.update((x16, len(plan)) + tuple(l[k] for k in ("at", "n", "gate", "slot0", "nslots", "cus")) for l in plan if l["kernel"] == "persist8")
    try:
        sts = [_native.NativeStream(m) for _ in scheds]
        if c["path"] == "forward":
            for i, sched in enumerate(scheds):
                for k, (T, first, last) in enumerate(e for e in sched if e is not None):
                    y = sts[i].forward(dev(i, k, T), first, last)
                    note()
                    got[i].append(None if y is None else y[0].cpu().numpy())
        else:
            for r in range(max(len(s) for s in scheds)):
                due = [i for i, s in enumerate(scheds) if r < len(s) and s[r] is not None]
                if not due:
                    continue
                ks = [len(got[i]) for i in due]
                ys = _native.NativeStream.forward_many([sts[i] for i in due], [dev(i, k, scheds[i][r][0]) for i, k in zip(due, ks)],
                                                       [scheds[i][r][1] for i in due], [scheds[i][r][2] for i in due])
                note()
                for i, y in zip(due, ys):
                    got[i].append(None if y is None else y[0].cpu().numpy())
        recomputed = m.recompute_count()
    finally:
        for s in sts:
            s.close()
        m.close()
    ref, o32 = references(c, sd, cfg)
    e32 = distance(o32, ref)
    same = shape_of(got) == shape_of(ref)
    gpu_max = distance(got, ref) if same else float("inf")
    return dict(name=c["name"], family=c["family"], kernel_expected=c["kernel"], kernels=sorted(kernels), recomputed=recomputed,
                persist8_launches=sorted(list(v) for v in launches),      # [x16, launches, at, n, gate, slot0, nslots, cus]
                frames_as_reference=same and shape_of(ref) == [[p["nout"] for p in walk(c, s)] for s in scheds],
                frames=int(sum(sum(v) for v in shape_of(ref))), e32=e32, gpu_max=gpu_max, ratio=gpu_max / e32 if e32 > 0 else float("inf"),
                where=localise(c, got, ref))
