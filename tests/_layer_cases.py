"""What tests/test_gpu_layer_accuracy.py (GPU) and tests/test_layer_accuracy_sensitivity.py (CPU) share: the bound's constants, the
case table, the seeded inputs, the error statistics and the message that localises the worst element.

THE BOUND.  Per case ``e32 = max |oracle.model.batch_rnn - _f64_ref.batch_rnn|`` (the fp32 oracle's own error, computed on the CPU in the
same run) and the assertion ``max |gpu - _f64_ref| <= M * e32``, with ONE M per arithmetic family:

  M["split"]  every persistent kernel (split-fp16 recurrent product; the x-projection on the split-fp16 GEMM)
  M["f32"]    the per-step path (fp32-MFMA recurrent product)

M = the next power of two at or above twice the largest ratio measured on an MI355X over the whole case table (the factor two: other
seeds, and the hardware exp / rcp of rnn_cell.h).  The measured figures per case are in tests/layer_accuracy_measured.json; the
largest ratios were 1.71 (split) and 1.54 (f32).  The RMS error is recorded beside the maximum; as a second statistic it separates
nothing the maximum does not (a lost cross term is 0.8 x as many multiples of the oracle's RMS error as of its maximum), so it is not asserted.

WHAT THE BOUND SEES, AND WHERE NOT.  M is not free: tests/test_layer_accuracy_sensitivity.py asserts, at default weights (`gain` 1:
layer 1 up to the widest case, 1280 units, and layer 0), that every mutant it knows -- the smallest is one cross term lost in one 32-wide
k-block -- lies above 2 * M * e32, so raising M without looking makes a CPU test fail.  That relation does NOT hold for the cases with
saturating weights (`gain` 6, `coarse` below): there e32 itself is large (the fp32 x-projection of weights six times as large, at layer
0 of inputs up to 20: 4e-6 .. 1e-5) while a lost cross term stays where it was, so a lost fragment is 8 .. 11 x e32 at 800 units, 7 .. 9 x
at 1280 and only 2 .. 3 x at layer 0 -- at or below the 2 * M = 8 the relation asks for, at layer 0 below M itself.  Those cases guard
what they are there for -- gates driven into saturation, the range of the split, masking, hand-offs (1e4 x e32) -- and errors above M *
e32; they cannot see a single lost fragment.  Each of them therefore has a SHARP sibling in the table: the same kernel, kind and
width at default weights with T > 1, where the fragment mutants are 10 x e32 and more (test_case_table_pairs_every_coarse_case).
"""
import json
import os
import sys

import numpy as np

M = {"split": 4.0, "f32": 4.0}
FAMILY = {"steps": "f32", "persist8": "split", "p16w8": "split", "p16w4": "split", "duo": "split", "ring8": "split", "ring4": "split"}
KERNELS = sorted(FAMILY)        # the seven RnnKernel values by the names dsmi_debug_last_rnn_plan prints


def _case(kernel, kind, H, B, T=29, lens="ragged", bidir=True, layer=1, inflight=1, windows=0, env=None, gain=1.0, fresh=False,
          launches=None, note=""):
    env = dict(env or {})
    name = "%s-%s%d-B%d-T%d-%s-%s-L%d-if%d" % (kernel, kind, H, B, T, lens, "bi" if bidir else "uni", layer, inflight)
    name += ("-w%d" % windows if windows else "") + ("-g%g" % gain if gain != 1.0 else "") + "".join("-" + v for v in env.values())
    return dict(name=name, kernel=kernel, kind=kind, H=H, B=B, T=T, lens=lens, bidir=bidir, layer=layer, inflight=inflight,
                windows=windows, env=env, gain=gain, fresh=fresh, launches=launches, note=note)


R4, R8, DUO = {"DSMI_RNN_KERNEL": "ring4"}, {"DSMI_RNN_KERNEL": "ring8"}, {"DSMI_RNN_KERNEL": "duo"}
P8 = {"DSMI_RNN_MODE": "persist8"}
STEPS_F32 = {"DSMI_RNN_MODE": "steps", "DSMI_DENSE_MODE": "f32"}

# kernel = the form dsmi_debug_last_rnn_plan must name for EVERY launch of the layer.  fresh: the case runs in a process of its own,
# started with its environment -- the four-wave form below 224 units is fenced off unless the PROCESS started with
# DSMI_RNN_KERNEL=ring4 (api.hip: ring_env), and in a process that has planned a layer before, the same request runs the eight-wave
# form without a word.  T is odd unless stated; lens: "ragged" = descending from T to 1 over the batch, "tail" = every tile full
# length but the last, which holds a clip of length T and one of length 1, "equal" = all T.
CASES = [
    # ---- the four-wave ring: k-blocks per wave 1 (waves without one) .. 14 (the four-tile cap)
    _case("ring4", "gru", 16, 33, inflight=2, env=R4, fresh=True, note="one k-block: waves without any"),
    _case("ring4", "gru", 48, 70, inflight=2, env=R4, fresh=True, note="odd number of 16-unit groups, partial last tile"),
    _case("ring4", "gru", 64, 64, inflight=2, env=R4, fresh=True, lens="tail"),
    _case("ring4", "gru", 224, 64, inflight=2, note="first unfenced width"),
    _case("ring4", "gru", 224, 17, inflight=2, env=R4, note="two real tiles padded with phantom ones"),
    _case("ring4", "lstm", 512, 48, inflight=2, note="LSTM cap: 8 k-blocks per wave"),
    _case("ring4", "lstm", 512, 64, inflight=2, gain=6.0, lens="tail"),
    _case("ring4", "gru", 800, 64, inflight=2, T=41),
    _case("ring4", "gru", 800, 64, inflight=2, T=41, gain=6.0),
    _case("ring4", "gru", 800, 64, inflight=2, lens="tail"),
    _case("ring4", "gru", 800, 64, inflight=2, lens="equal", T=20),
    _case("ring4", "gru", 800, 64, inflight=2, T=1, lens="equal"),
    _case("ring4", "gru", 800, 64, inflight=2, layer=0, note="K = 1312, no BatchNorm"),
    _case("ring4", "gru", 800, 64, inflight=2, bidir=False, note="grid.y = 1"),
    _case("ring4", "gru", 800, 1, inflight=2, env=R4),
    _case("ring4", "gru", 800, 16, inflight=2, env=R4),
    _case("ring4", "gru", 800, 32, inflight=2, env=R4),
    _case("ring4", "gru", 800, 33, inflight=2),
    _case("ring4", "gru", 800, 128, inflight=2, T=21, launches=2, note="two launches of four tiles"),
    _case("ring4", "gru", 896, 64, inflight=2, note="14 k-blocks per wave: the four-tile cap"),
    _case("ring4", "gru", 896, 40, inflight=2, gain=6.0, layer=0),
    _case("ring4", "rnn", 256, 64, inflight=2),
    _case("ring4", "lstm", 256, 40, inflight=2, bidir=False),
    # ---- the eight-wave ring
    _case("ring8", "gru", 16, 33, inflight=2, note="fenced small shape: the eight-wave form by itself"),
    _case("ring8", "gru", 64, 17, inflight=2),
    _case("ring8", "gru", 64, 64, inflight=2, gain=6.0, lens="tail"),
    _case("ring8", "gru", 800, 32, inflight=2, T=41),
    _case("ring8", "gru", 800, 17, inflight=2, gain=6.0),
    _case("ring8", "gru", 800, 1, inflight=2),
    _case("ring8", "gru", 800, 16, inflight=2, lens="equal", T=20),
    _case("ring8", "gru", 800, 64, inflight=2, env=R8, note="a window of four tiles"),
    _case("ring8", "gru", 800, 64, inflight=2, windows=2, note="set_ring_windows(2): two windows of two tiles"),
    _case("ring8", "gru", 800, 128, inflight=1, T=21, note="lone batch: four windows side by side"),
    _case("ring8", "gru", 800, 32, inflight=2, layer=0),
    _case("ring8", "gru", 800, 32, inflight=2, bidir=False),
    _case("ring8", "gru", 896, 40, inflight=2, env=R8),
    _case("ring8", "gru", 896, 33, inflight=2, env=R8, T=1, lens="equal"),
    _case("ring8", "lstm", 512, 32, inflight=2),
    _case("ring8", "rnn", 96, 64, inflight=2),
    # ---- paired tiles
    _case("duo", "gru", 64, 32, inflight=2, env=DUO),
    _case("duo", "gru", 64, 17, inflight=2, env=DUO, T=1, lens="equal"),
    _case("duo", "lstm", 512, 40, inflight=2, env=DUO, note="an odd number of tiles in pairs"),
    _case("duo", "lstm", 512, 33, inflight=2, env=DUO, gain=6.0, bidir=False),
    _case("duo", "gru", 896, 32, inflight=2, env=DUO, lens="tail"),
    _case("duo", "gru", 896, 64, inflight=2, env=DUO, layer=0, launches=1),
    _case("duo", "gru", 800, 40, inflight=2, env=DUO, gain=6.0, T=41),
    _case("duo", "gru", 800, 48, inflight=2, env=DUO),
    _case("duo", "rnn", 160, 33, inflight=1, env=DUO),
    # ---- the half-CU form of the tile-walking kernel: one tile, batches in flight, where no tile pair exists
    _case("p16w4", "gru", 64, 16, inflight=2, env=DUO),
    _case("p16w4", "gru", 64, 16, inflight=2, env=DUO, T=1, lens="equal"),
    _case("p16w4", "lstm", 512, 16, inflight=2, env=DUO, gain=6.0),
    _case("p16w4", "lstm", 512, 9, inflight=2, env=DUO, bidir=False, lens="equal", T=20),
    _case("p16w4", "gru", 896, 16, inflight=2, env=DUO, T=41),
    _case("p16w4", "gru", 896, 1, inflight=2, env=DUO, layer=0),
    # ---- whole-CU tile walker
    _case("p16w8", "gru", 16, 1),
    _case("p16w8", "gru", 800, 32, gain=6.0, note="a lone batch of up to 32 clips at the flagship width"),
    _case("p16w8", "gru", 800, 17),
    _case("p16w8", "gru", 1024, 32, note="4 k-blocks per wave"),
    _case("p16w8", "gru", 1024, 17, layer=0),
    _case("p16w8", "gru", 1200, 64, inflight=4, T=21, note="5 k-blocks per wave, four tiles walked"),
    _case("p16w8", "gru", 1200, 128, inflight=2, T=21, note="eight tiles walked: the carried-state arrays full"),
    _case("p16w8", "gru", 1280, 40, T=21, gain=6.0, lens="tail"),
    _case("p16w8", "gru", 1280, 33, T=21, note="its width cap at default weights"),
    _case("p16w8", "gru", 1280, 16, T=1, lens="equal"),
    _case("p16w8", "lstm", 1024, 33, T=21, note="LSTM cap: 4 k-blocks per wave"),
    _case("p16w8", "lstm", 1024, 16, bidir=False, T=20, lens="equal"),
    _case("p16w8", "rnn", 1280, 64, T=21),
    # ---- first generation
    _case("persist8", "gru", 8, 3, note="one workgroup per direction"),
    _case("persist8", "gru", 904, 33, note="H not a multiple of 16"),
    _case("persist8", "gru", 904, 64, T=21, layer=0, gain=6.0),
    _case("persist8", "gru", 1280, 32, env=P8, T=21, launches=2, note="its width cap; the directions one after the other"),
    _case("persist8", "gru", 1200, 24, env=P8, T=21, launches=2, lens="tail", note="two launches, the second joined"),
    _case("persist8", "lstm", 72, 40, bidir=False),
    _case("persist8", "rnn", 200, 16, T=1, lens="equal"),
    # ---- per step
    _case("steps", "gru", 100, 17),
    _case("steps", "lstm", 100, 40, bidir=False, lens="tail"),
    _case("steps", "gru", 1288, 16, T=21),
    _case("steps", "gru", 1288, 33, T=21, layer=0, gain=6.0),
    _case("steps", "gru", 800, 32, env=STEPS_F32, note="fp32 MFMA in the GEMM and the recurrent product"),
    _case("steps", "gru", 800, 64, env=STEPS_F32, gain=6.0, lens="tail", T=21),
    _case("steps", "rnn", 100, 17, T=1, lens="equal"),
    # ---- template instantiations the cases above do not reach (host_fuzz rnnforms says which shape runs which): the largest width
    # that maps to each, the smallest batch its form takes.  As many as test_case_table_reaches_every_kernel's cap on this table
    # leaves room for; the instantiations still unreached are listed in profiles/rnn_forms.txt
    _case("ring4", "gru", 512, 1, T=5, inflight=2, env=R4, note="8 k-blocks per wave"),
    _case("ring4", "gru", 768, 1, T=5, inflight=2, env=R4, note="12 k-blocks per wave"),
    _case("ring4", "rnn", 896, 1, T=5, inflight=2, env=R4, note="14 k-blocks per wave, one gate"),
    _case("ring4", "lstm", 448, 1, T=5, inflight=2, env=R4, note="7 k-blocks per wave"),
    _case("ring8", "gru", 512, 1, T=5, inflight=2, env=R8, note="4 k-blocks per wave"),
    _case("duo", "gru", 512, 17, T=5, inflight=2, env=DUO, note="4 k-blocks per wave, no tail"),
    _case("p16w4", "gru", 512, 1, T=5, inflight=2, env=DUO, note="4 k-blocks per wave"),
    _case("p16w8", "gru", 1024, 65, T=5, note="the pipelined kernel at 4 k-blocks per wave: three tiles walked"),
    _case("persist8", "gru", 888, 1, T=5, note="7 k-pairs per wave, one tile"),
]
assert len({c["name"] for c in CASES}) == len(CASES)


def coarse(c):
    """A case whose bound cannot see a single lost fragment (module docstring): saturating weights."""
    return c["gain"] != 1.0


def sharp_sibling(c):
    """The case that sees the fragment mutants for a coarse case's kernel form: same kernel, kind and width, default weights, T > 1."""
    return [s for s in CASES if not coarse(s) and s["T"] > 1 and (s["kernel"], s["kind"], s["H"]) == (c["kernel"], c["kind"], c["H"])
            and s["env"].get("DSMI_DENSE_MODE") == c["env"].get("DSMI_DENSE_MODE")]


def plan_row(c, n_cus=256, lane=0):
    """The case as an input row of `host_fuzz rnnplan` (tests/test_rnn_plan_host.py)."""
    env = c["env"]
    dense = "f32" if env.get("DSMI_DENSE_MODE") == "f32" else "split"
    return "%d %d %d %d %d %d %d %s %s %s %d" % ({"gru": 0, "lstm": 1, "rnn": 2}[c["kind"]], 2 if c["bidir"] else 1, c["H"], c["B"], c["inflight"],
                                                 c["windows"], lane, env.get("DSMI_RNN_KERNEL", "-"), env.get("DSMI_RNN_MODE", "-"), dense, n_cus)


def make_lens(c):
    B, T = c["B"], c["T"]
    if c["lens"] == "equal" or T == 1:
        return np.full(B, T, dtype=np.int32)
    if c["lens"] == "ragged":        # descending from T to 1 (a lone clip: T)
        return np.maximum(np.round(np.linspace(T, 1, B)), 1).astype(np.int32) if B > 1 else np.array([T], dtype=np.int32)
    assert c["lens"] == "tail"
    lens = np.full(B, T, dtype=np.int32)
    first = (B - 1) // 16 * 16       # the last tile: a clip of length T, then down to 1
    n = B - first
    assert n > 1, "a `tail` case needs two clips or more in its last tile"
    lens[first + 1:] = np.maximum(np.round(np.linspace(T - 1, 1, n - 1)), 1)
    return lens


def make_case(c):
    """(cfg, state_dict, x [T, B, I] float32, lens).  Layer >= 1: standard normal x 0.5, what a layer before it emits; layer 0:
    what the conv stack's Hardtanh emits -- values in [0, 20], about half of them zero, one in a hundred at the ceiling of 20.  The rows past a clip's length hold values
    like any other: the layer has to mask them."""
    from danspeech_amd import synthetic as syn
    cfg = dict(conv_layers=2, rnn_type=c["kind"], rnn_hidden_size=c["H"], rnn_layers=2, bidirectional=c["bidir"], context=20)
    sd = syn.make_state_dict(2, c["kind"], c["H"], 2, bidirectional=c["bidir"], seed=71, ih_gain=c["gain"])
    rng = np.random.default_rng(5 + c["H"] + c["B"])
    I = syn.rnn_input_size(2) if c["layer"] == 0 else c["H"]
    if c["layer"] == 0:
        x = np.clip(rng.standard_normal((c["T"], c["B"], I)) * 2.5, 0.0, 20.0).astype(np.float32)
        x[rng.random(x.shape) < 0.01] = 20.0
    else:
        x = (rng.standard_normal((c["T"], c["B"], I)) * 0.5).astype(np.float32)
    return cfg, sd, x, make_lens(c)


def references(c, sd, x, lens, rms=False):
    """(float64 reference, e32 = the fp32 oracle's max error against it[, its RMS error])"""
    import _f64_ref as f64
    from oracle import model as om
    ref = f64.batch_rnn(sd, c["layer"], c["kind"], x, lens, c["bidir"], batch_norm=c["layer"] > 0)
    o32 = om.batch_rnn(sd, c["layer"], c["kind"], x, lens, c["bidir"], c["layer"] > 0)
    e = o32.astype(np.float64) - ref
    return (ref, float(np.abs(e).max())) + ((float(np.sqrt((e ** 2).mean())),) if rms else ())


def localise(y, ref, lens):
    """Where the worst element is, in the units the kernels are built from."""
    err = np.abs(y.astype(np.float64) - ref)
    t, b, u = (int(v) for v in np.unravel_index(int(err.argmax()), err.shape))
    per_tile = [float(err[:, k:k + 16].max()) for k in range(0, err.shape[1], 16)]
    per_group = [float(err[:, :, k:k + 16].max()) for k in range(0, err.shape[2], 16)]
    worst_groups = np.argsort(per_group)[::-1][:4]
    return ("worst element %.3g at t=%d (clip length %d: %s), clip %d (tile %d), unit %d (16-unit group %d, 32-unit workgroup %d); "
            "got %.9g, float64 %.9g; max error per tile %s; largest per 16-unit group %s; max per step (first 8 steps) %s"
            % (err[t, b, u], t, lens[b], "PAST the clip's length: masking" if t >= lens[b] else "inside the clip", b, b // 16, u, u // 16, u // 32,
               y[t, b, u], ref[t, b, u], ["%.2g" % v for v in per_tile], ["%d: %.2g" % (g, per_group[g]) for g in worst_groups],
               ["%.2g" % float(err[s].max()) for s in range(min(8, err.shape[0]))]))


def run_on_gpu(c):
    """One case on the GPU in THIS process: the record (figures, the kernels that ran) and the message for a failure."""
    import torch
    from danspeech_amd import _native
    cfg, sd, x, lens = make_case(c)
    old = {k: os.environ.get(k) for k in c["env"]}
    os.environ.update(c["env"])
    try:
        m = _native.NativeModel(cfg, sd)        # DSMI_RNN_KERNEL, DSMI_RNN_MODE, DSMI_DENSE_MODE are read here
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    try:
        m.set_inflight(c["inflight"])
        if c["windows"]:
            m.set_ring_windows(c["windows"])
        y = m.rnn_layer(c["layer"], torch.from_numpy(x).cuda(), lens).cpu().numpy()
        x16, launches = m.last_rnn_plan()
        recomputed = m.recompute_count()
    finally:
        m.close()
    ref, e32, e32_rms = references(c, sd, x, lens, rms=True)
    d = y.astype(np.float64) - ref
    past = max([float(np.abs(y[L:, b]).max()) for b, L in enumerate(lens) if L < c["T"]] or [0.0])
    return dict(name=c["name"], kernels=[l["kernel"] for l in launches], x16=x16, recomputed=recomputed, e32=e32, e32_rms=e32_rms,
                gpu_max=float(np.abs(d).max()), gpu_rms=float(np.sqrt((d ** 2).mean())), ref_rms=float(np.sqrt((ref ** 2).mean())),
                ratio=float(np.abs(d).max() / e32), past_len_max=past, where=localise(y, ref, lens))


if __name__ == "__main__":      # python tests/_layer_cases.py NAME: one case in a process of its own; the record as the last line
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [here, os.path.dirname(here)]
    case, = [c for c in CASES if c["name"] == sys.argv[1]]
    print("RECORD " + json.dumps(run_on_gpu(case)))
