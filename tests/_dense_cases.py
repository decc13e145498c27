"""What tests/test_gpu_dense_accuracy.py (GPU) and tests/test_dense_accuracy_sensitivity.py (CPU) share: the bound's constants, the
case tables of the conv stack and of the output head, the seeded inputs, the error statistics and the message that localises the
worst element.  The recurrent layers' counterpart is tests/_layer_cases.py; the rules are the same.

THE BOUND.  Per case ``e32 = max |fp32 oracle - float64|`` (oracle/model.py against tests/_f64_ref.py on the same float32 inputs,
computed on the CPU in the same run) and the assertion ``max |gpu - float64| <= M[family] * e32``:

  M["conv_split"]  dsmi_conv_stack on the default path: conv1_split.hip, conv_split.hip (split-fp16 MFMA)
  M["conv_f32"]    dsmi_conv_stack on conv.hip (fp32 MFMA): DSMI_DENSE_MODE=f32, and where a weight leaves the split's range
  M["head"]        dsmi_head: lookahead_kernel (unidirectional models) + head_kernel<1..4>

M = the next power of two at or above twice the largest ratio measured on an MI355X over the family's cases (the factor two: other
seeds).  The figures per case are in tests/dense_accuracy_measured.json, written by ``DSMI_RECORD_DENSE_ACCURACY=1`` (with the M they
give as ``M_derived``); the largest ratios were 8.62 (conv_split: c at depth 2), 8.09 (conv_f32: the same case) and 15.9 (head:
7 x 3 rows, context 1), so M is 32 for all three.  The tests assert against M, never against that file.

WHY THE RATIOS ARE THAT LARGE.  Conv, depth 1: 1.1 .. 1.3.  From depth 2 on: 3.9 .. 8.6 at n_freq 161 / 81 on BOTH paths alike, 1.0 ..
1.1 at n_freq 2, 2.6 .. 5.3 at hot weights -- max errors of 4 .. 5e-6 at values around 1, mostly BELOW the reference, spread evenly
over tiles, clips and row groups, with the worst element in the same output channel on either path.  Layer 2 sums 7392 products: the
oracle does so in 21 BLAS products of 352 terms each (e32 = 5 .. 7e-7), the kernels add into one float32 accumulator MFMA after
MFMA, 693 times (conv_split.hip) or 3696 times (conv.hip); the numpy emulation of the split form, which sums as the oracle does, is
at 1.2 x e32.  So the measure is generous to the kernels at 161 bins: what it calls 8 x is an honest float32 chain, and a
shorter chain (n_freq 2: 352 terms, e32 = 3e-8) is at 1.0.  Head: 0.2 .. 2.5 in 50 of the 55 cases; the other five have 1 or 21 rows, where e32 is the maximum over few rows: 2.7, 3.9 and 6.7
(one row; e32 = 3 .. 5e-8 against the 3e-7 .. 2e-6 of the larger cases, absolute errors of 1 .. 3e-7, no more than elsewhere), and
the unidirectional 7 x 3 cases of context 3 (3.4: 4.6e-6 against 1.4e-6) and context 1 (15.9: 1.2e-6 against an e32 of 7e-8).

THE CONV CASES.  Shapes (B, T, lens) are the smallest that cross every edge of the kernels' tiling; output steps are
``To = (T - 1) // 2 + 1``:

  a  4 x 259, lens 259 129 127 1   To = 130: two 64-step tiles + 2, time pitch 132 != To; clips of 65 (one past a tile), 64 (a fully
                                   masked tile follows) and 1 output steps
  b  2 x 128, equal                exactly one tile
  c  3 x 33, lens 33 32 31         To = 17: one past a 16-step MFMA column tile
  d  1 x 1                         a single output step
  e  5 x 95, lens 95 94 50 3 2     To = 48

Features are standard normal and the values past each clip's length are LEFT IN PLACE: the reference's Conv2d reads them (the first
layer's in-length outputs depend on up to five frames past the length), only outputs are masked.  Axes: conv depth 1 / 2 / 3
(``conv1<SPLIT_OUT=false>`` / ``conv1<true>`` + ``conv_split<false>`` / + ``conv_split<true>`` and the 96-channel third layer,
three 32-channel tiles per clip in blockIdx.z); n_freq 161, 81 (fo = 41 / 21 / 11: the last 4-row workgroup holds three rows) and 2
(fo = 1); default weights and ``hot`` ones -- every conv layer's weight times HOT_GAIN[layer], chosen on the CPU so that of every
layer's in-length outputs (float64 reference) at least 1 % sit at the ceiling of 20 and at least 20 % strictly inside (0, 20)
(test_dense_accuracy_sensitivity.py asserts it): the clamp, inputs up to 20 in layers 2 and 3, lo terms up to 2^-7 --;
``DSMI_DENSE_MODE=f32``; and ``range``: one weight of the last layer set to 1000.0, above 60000 / 64, with no environment variable
-- the whole stack then has to run on conv.hip (model_build.hip: conv_mode) and meets the conv_f32 bound.  (1000 * 64 is an fp16 number, so the
split kernels would compute the case as well: the bound cannot tell which path ran.  The case's output must therefore equal, bit for
bit, that of a DSMI_DENSE_MODE=f32 model of the same weights -- and the same comparison at default weights, F32_CONTROL, must differ.)

WHAT THE BOUND SEES is tests/test_dense_accuracy_sensitivity.py's subject (its docstring has the figures): with M = 32 one lost lo
product of ONE layer-2 tap is below 2 * M * e32 at n_freq 161 and seen at the n_freq 2 cases of depth 2.  The hot cases are
coarse in the sense of _layer_cases.py: e32 grows with the weights while a lost lo term does not, so each hot case has a sibling
of the same depth and shape at default weights (test_case_table_pairs_every_hot_case).

THE HEAD CASES.  1-layer models (conv depth 1 at n_freq 2: the model in front of the head is as small as it gets); the inputs are
what the test supplies.  Bidirectional: both directions uniform in (-1, 1).  Unidirectional: normal x 3 and the lookahead weights
times LOOK_GAIN (with torch's default scale the sum of `context` taps has a standard deviation of 1.7 and never reaches 20), so that
both clamps of the lookahead are hit in every such case (asserted on the CPU from the reference).  ``sharp``: fc weights times
SHARP_GAIN, the float64 logits span more than 200 -- without the maximum subtracted, expf overflows.
"""
import os

import numpy as np

M = {"conv_split": 32.0, "conv_f32": 32.0, "head": 32.0}

SHAPES = {"a": (4, 259, [259, 129, 127, 1]), "b": (2, 128, [128, 128]), "c": (3, 33, [33, 32, 31]), "d": (1, 1, [1]),
          "e": (5, 95, [95, 94, 50, 3, 2])}
AUDIO = {161: None, 81: dict(sampling_rate=8000), 2: dict(sampling_rate=100, window_size=0.02)}
HOT_GAIN = (14.0, 4.0, 4.0)         # per conv layer; see the module docstring and test_hot_cases_reach_the_ceiling
F32 = {"DSMI_DENSE_MODE": "f32"}


def _conv(shape, depth, n_freq=161, weights="default", env=None):
    env = dict(env or {})
    name = "conv-%s-d%d-f%d-%s%s" % (shape, depth, n_freq, weights, "".join("-" + v for v in env.values()))
    family = "conv_f32" if env or weights == "range" else "conv_split"
    return dict(name=name, shape=shape, depth=depth, n_freq=n_freq, weights=weights, env=env, family=family)


CONV_CASES = (
    [_conv(s, d) for s in "acd" for d in (1, 2, 3)] + [_conv(s, d) for s in "be" for d in (2, 3)]
    + [_conv("a", 3, n_freq=81), _conv("c", 2, n_freq=2), _conv("c", 3, n_freq=2)]
    + [_conv(s, d, weights="hot") for s in "ac" for d in (2, 3)]
    + [_conv(s, d, env=F32) for s in "ac" for d in (2, 3)]
    + [_conv("c", 2, weights="range")])
assert len({c["name"] for c in CONV_CASES}) == len(CONV_CASES)
F32_CONTROL = "conv-c-d2-f161-default"      # the range case's default-weight twin: its output must NOT be what DSMI_DENSE_MODE=f32 gives


def default_sibling(c):
    """The default-weight cases of a hot case's depth, shape and path: the ones that see a lost lo term."""
    return [s for s in CONV_CASES if s["weights"] == "default" and (s["shape"], s["depth"], s["n_freq"], s["env"]) == (c["shape"], c["depth"], c["n_freq"], c["env"])]


def make_conv_case(c):
    """(cfg, state_dict, audio_conf, x [B, 1, F, T] float32, lens, out_lens)"""
    from danspeech_amd import synthetic as syn
    from oracle import model as om
    B, T, lens = SHAPES[c["shape"]]
    ac = AUDIO[c["n_freq"]] or {}
    cfg = dict(conv_layers=c["depth"], rnn_type="gru", rnn_hidden_size=8, rnn_layers=1, bidirectional=True, context=20)
    sd = syn.make_state_dict(c["depth"], "gru", 8, 1, seed=23, sample_rate=ac.get("sampling_rate", 16000), window_size=ac.get("window_size", 0.02))
    last = "conv.seq_module.%d.weight" % (3 * (c["depth"] - 1))
    if c["weights"] == "hot":
        for li in range(c["depth"]):
            sd["conv.seq_module.%d.weight" % (3 * li)] = sd["conv.seq_module.%d.weight" % (3 * li)] * np.float32(HOT_GAIN[li])
    elif c["weights"] == "range":
        sd[last] = sd[last].copy()
        sd[last][5, 0, 3, 2] = 1000.0
    else:
        assert c["weights"] == "default"
    rng = np.random.default_rng(900 + 10 * T + c["depth"])
    x = rng.standard_normal((B, 1, c["n_freq"], T)).astype(np.float32)      # nothing zeroed past the lengths
    lens = np.array(lens, dtype=np.int32)
    return cfg, sd, AUDIO[c["n_freq"]], x, lens, om.get_seq_lens(lens, c["depth"])


def conv_references(c, sd, x, out_lens, layers_out=None):
    """(float64 reference, e32, the fp32 oracle's RMS error)"""
    import _f64_ref as f64
    from oracle import model as om
    ref = f64.conv_stack(sd, x, out_lens, c["depth"], layers_out=layers_out)
    e = om.conv_stack(sd, x, out_lens, c["depth"]).astype(np.float64) - ref
    return ref, float(np.abs(e).max()), float(np.sqrt((e ** 2).mean()))


def past_len_max(y, out_lens):
    return max([float(np.abs(y[b, :, :, int(L):]).max()) for b, L in enumerate(out_lens) if L < y.shape[3]] or [0.0])


def localise_conv(c, y, ref, out_lens):
    """Where the worst element is, in the units the conv kernels are built from."""
    if y.shape != ref.shape:
        return "shape %s, the reference's %s" % (y.shape, ref.shape)
    err = np.abs(y.astype(np.float64) - ref)
    b, ch, f, t = (int(v) for v in np.unravel_index(int(err.argmax()), err.shape))
    per_tile = ["%.2g" % float(err[:, :, :, k:k + 64].max()) for k in range(0, err.shape[3], 64)]
    per_rows = ["%.2g" % float(err[:, :, k:k + 4].max()) for k in range(0, err.shape[2], 4)]
    per_clip = ["%.2g" % float(err[k].max()) for k in range(err.shape[0])]
    return ("conv depth %d (last layer %d): worst element %.3g at clip %d (%d output steps: %s), channel %d (32-channel tile %d), output row %d "
            "(4-row workgroup %d, 8-row workgroup %d), output step %d (64-step tile %d, column %d of it); got %.9g, float64 %.9g; "
            "max error per 64-step tile %s; per clip %s; per 4-row group %s"
            % (c["depth"], c["depth"], err[b, ch, f, t], b, out_lens[b], "PAST the clip's length: masking" if t >= out_lens[b] else "inside the clip",
               ch, ch // 32, f, f // 4, f // 8, t, t // 64, t % 64, y[b, ch, f, t], ref[b, ch, f, t], per_tile, per_clip, per_rows[:24]))


class _env:
    """the case's environment around the creation of the model only (DSMI_DENSE_MODE is read there), restored afterwards"""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def run_conv_on_gpu(c):
    """One conv case on the GPU: the record (figures) and the message for a failure.  One handle, closed in `finally`."""
    import torch
    from danspeech_amd import _native
    cfg, sd, ac, x, lens, out_lens = make_conv_case(c)
    def run(env):
        with _env(env):
            m = _native.NativeModel(cfg, sd, audio_conf=ac)
        try:
            return m.conv_stack(torch.from_numpy(x).cuda(), lens).cpu().numpy()
        finally:
            m.close()
    y = run(c["env"])
    # which path ran: conv.hip and the split kernels differ in the low bits, so a stack that fell back to conv.hip by itself gives
    # bit for bit what DSMI_DENSE_MODE=f32 gives on the same weights, and the default path does not
    same_as_f32 = bool(np.array_equal(y, run(F32))) if c["weights"] == "range" or c["name"] == F32_CONTROL else None
    ref, e32, e32_rms = conv_references(c, sd, x, out_lens)
    same_shape = y.shape == ref.shape
    d = y.astype(np.float64) - ref if same_shape else np.full(1, np.inf)
    return dict(name=c["name"], family=c["family"], shape=list(y.shape), ref_shape=list(ref.shape), same_as_f32=same_as_f32, e32=e32, e32_rms=e32_rms,
                gpu_max=float(np.abs(d).max()), gpu_rms=float(np.sqrt((d ** 2).mean())), ref_rms=float(np.sqrt((ref ** 2).mean())),
                ratio=float(np.abs(d).max() / e32), past_len_max=past_len_max(y, out_lens) if same_shape else float("inf"),
                where=localise_conv(c, y, ref, out_lens))


# ---- the output head -----------------------------------------------------------------------------------------------------------
LOOK_GAIN = 12.0
SHARP_GAIN = 10.0
ROWS = [(1, 1), (31, 1), (8, 4), (11, 3), (7, 10)]       # (To, B): 1, 31, 32, 33 and 70 rows


def _head(C, H, To, B, bidir=True, context=20, sharp=False):
    name = "head-C%d-H%d-%dx%d-%s%s" % (C, H, To, B, "bi" if bidir else "uni-ctx%d" % context, "-sharp" if sharp else "")
    return dict(name=name, C=C, H=H, To=To, B=B, bidir=bidir, context=context, sharp=sharp, family="head")


HEAD_CASES = (
    [_head(C, 100, 11, 3) for C in (1, 29, 32, 33, 64, 65, 96, 97, 128)]                 # every NT, both sides of every tile edge
    + [_head(C, H, To, B) for C in (33, 97) for H in (8, 13, 100, 800) for To, B in ROWS if (H, To, B) != (100, 11, 3)]
    + [_head(33, 100, To, 3, bidir=False, context=ctx) for ctx in (1, 3, 20) for To in (7, 25)]
    + [_head(97, 13, 7, 3, bidir=False, context=3)]
    + [_head(33, 100, 11, 3, sharp=True)])
assert len({c["name"] for c in HEAD_CASES}) == len(HEAD_CASES)


def make_head_case(c):
    """(cfg, state_dict, audio_conf, x_fwd [To, B, H] float32, x_rev or None)"""
    from danspeech_amd import synthetic as syn
    ac = AUDIO[2]
    cfg = dict(conv_layers=1, rnn_type="gru", rnn_hidden_size=c["H"], rnn_layers=1, bidirectional=c["bidir"], context=c["context"])
    sd = syn.make_state_dict(1, "gru", c["H"], 1, bidirectional=c["bidir"], n_labels=c["C"], context=c["context"], seed=31,
                             sample_rate=ac["sampling_rate"], window_size=ac["window_size"])
    if c["sharp"]:
        sd["fc.0.module.1.weight"] = sd["fc.0.module.1.weight"] * np.float32(SHARP_GAIN)
    rng = np.random.default_rng(700 + c["C"] + c["H"] + 13 * c["To"] + c["B"])
    shape = (c["To"], c["B"], c["H"])
    if c["bidir"]:
        return cfg, sd, ac, rng.uniform(-1, 1, shape).astype(np.float32), rng.uniform(-1, 1, shape).astype(np.float32)
    sd["lookahead.0.conv.weight"] = sd["lookahead.0.conv.weight"] * np.float32(LOOK_GAIN)
    return cfg, sd, ac, (rng.standard_normal(shape) * 3.0).astype(np.float32), None


def head_references(c, sd, x_fwd, x_rev):
    """(float64 probabilities [B, To, C], e32, the float64 lookahead output or None, the float64 logits).  The fp32 oracle is
    oracle/model.py's lookahead, BatchNorm affine, matmul and softmax as its `forward` strings them together (the direction sum
    in float32, as its batch_rnn leaves it)."""
    import _f64_ref as f64
    from oracle import model as om
    if c["bidir"]:
        x64, la = x_fwd.astype(np.float64) + x_rev.astype(np.float64), None
        y32 = (x_fwd + x_rev).astype(np.float32)
    else:
        x64 = la = f64.lookahead(sd, x_fwd, c["context"])
        y32 = om.lookahead(sd, x_fwd, c["context"])
    ref = f64.head(sd, x64)
    a, b = om._bn_affine(sd, "fc.0.module.0")
    y32 = (y32 * a + b).astype(np.float32)
    To, B = x_fwd.shape[:2]
    logits = (y32.reshape(To * B, -1) @ sd["fc.0.module.1.weight"].T).reshape(To, B, -1).transpose(1, 0, 2).astype(np.float32)
    p32 = om.softmax(logits)
    return ref, float(np.abs(p32.astype(np.float64) - ref).max()), la, f64.head_logits(sd, x64)


def localise_head(c, p, ref):
    if p.shape != ref.shape:
        return "shape %s, the reference's %s" % (p.shape, ref.shape)
    err = np.abs(p.astype(np.float64) - ref)
    b, t, k = (int(v) for v in np.unravel_index(int(err.argmax()), err.shape))
    row = t * c["B"] + b
    per_tile = ["%.2g" % float(err[:, :, j:j + 32].max()) for j in range(0, err.shape[2], 32)]
    rows = np.transpose(err, (1, 0, 2)).reshape(-1, err.shape[2]).max(axis=1)
    per_wg = ["%.2g" % float(rows[j:j + 32].max()) for j in range(0, len(rows), 32)]
    return ("head_kernel<%d>: worst element %.3g at step %d, clip %d (row %d: 32-row workgroup %d, lane %d), class %d (32-class tile %d, %d classes); "
            "got %.9g, float64 %.9g; max error per class tile %s; per workgroup %s"
            % ((c["C"] + 31) // 32, err[b, t, k], t, b, row, row // 32, row % 32, k, k // 32, c["C"], p[b, t, k], ref[b, t, k], per_tile, per_wg))


def run_head_on_gpu(c):
    import torch
    from danspeech_amd import _native
    cfg, sd, ac, x_fwd, x_rev = make_head_case(c)
    m = _native.NativeModel(cfg, sd, audio_conf=ac, n_labels=c["C"])
    try:
        p = m.head(torch.from_numpy(x_fwd).cuda(), None if x_rev is None else torch.from_numpy(x_rev).cuda()).cpu().numpy()
    finally:
        m.close()
    ref, e32, _, _ = head_references(c, sd, x_fwd, x_rev)
    same_shape = p.shape == ref.shape
    d = p.astype(np.float64) - ref if same_shape else np.full(1, np.inf)
    gpu_max = float(np.abs(d).max())
    top2 = np.sort(ref, axis=-1)[..., -2:] if c["C"] > 1 else np.stack([np.zeros(ref.shape[:2]), ref[..., 0]], axis=-1)
    clear = (top2[..., 1] - top2[..., 0]) > 1e-4
    return dict(name=c["name"], family="head", shape=list(p.shape), ref_shape=list(ref.shape), e32=e32, gpu_max=gpu_max,
                gpu_rms=float(np.sqrt((d ** 2).mean())), ratio=(gpu_max / e32 if e32 > 0 else (0.0 if gpu_max == 0 else float("inf"))),
                nan=bool(np.isnan(p).any()), row_sum_err=float(np.abs(p.astype(np.float64).sum(axis=-1) - 1.0).max()),
                argmax_differs=int((p.argmax(axis=-1) != ref.argmax(axis=-1))[clear].sum()) if same_shape else -1, clear_rows=int(clear.sum()),
                where=localise_head(c, p, ref))
