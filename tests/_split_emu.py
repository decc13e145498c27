"""numpy emulation of the recurrent kernels' split-fp16 product inside the float64 cell of tests/_f64_ref.py, and the
mutants tests/test_layer_accuracy_sensitivity.py holds the layer-level bound against.

The product: both operands split once, ``hi = fp16(x)``, ``lo = fp16((x - hi) * 2^11)``; per 32-wide k-block three fp16 products
with float32 accumulation -- ``hi*hi`` into one accumulator, ``hi*lo + lo*hi`` into a second one that is folded in with 2^-11 at the
end.  (An fp16 x fp16 product is exact in float32, so a float32 matmul of the fp16 values is the MFMA up to the order of its 32
additions.)  ``gh`` and the new state are rounded to float32, as the kernels store them; the cell's transcendental functions are
float64 here, the kernels' hardware ``exp`` / ``rcp`` are not emulated.

Further down: the conv stack's two split forms (``ConvStackEmu``) and the mutants tests/test_dense_accuracy_sensitivity.py holds the
dense bound against.
"""
import numpy as np

import _f64_ref as f64

KB = 32
FOLD = np.float32(2.0 ** -11)


def split(x):
    """float32 -> (hi, lo scaled by 2^11), both as float32 arrays holding fp16 values"""
    x = np.asarray(x, dtype=np.float32)
    hi = x.astype(np.float16).astype(np.float32)
    lo = ((x - hi) * np.float32(2048.0)).astype(np.float16).astype(np.float32)
    return hi, lo


class SplitProduct:
    """``step`` hook of _f64_ref.direction: h (float64, holding float32 values) -> h W_hh^T as the kernels compute it.

    mutant: None, or one of
      ("drop_whi_hlo", kb)     the W_hi * h_lo product of k-block kb is missing
      ("drop_wlo_hhi_cols", n) the W_lo * h_hi product of the last n columns of K is missing
      ("fold_2_10", kb)        k-block kb's cross terms are folded in with 2^-10
      ("stale", t, clips)      at step t the product of `clips` reads the state of the step before (a hand-off one step late)
    """

    def __init__(self, w_hh, mutant=None):
        self.whi, self.wlo = (np.ascontiguousarray(p.T) for p in split(w_hh))       # [K, G*H]
        self.K = self.whi.shape[0]
        self.mutant = mutant or ("none",)
        self.prev = None      # the state one step back (for "stale")
        self.last = None

    def __call__(self, h, t):
        h32 = h.astype(np.float32)
        self.prev, self.last = self.last, h32
        m = self.mutant
        if m[0] == "stale" and t == m[1] and self.prev is not None:
            h32 = h32.copy()
            h32[m[2]] = self.prev[m[2]]
        hhi, hlo = split(h32)
        acc = np.zeros((h.shape[0], self.whi.shape[1]), dtype=np.float32)
        cross = np.zeros_like(acc)
        for kb, k0 in enumerate(range(0, self.K, KB)):
            k = slice(k0, min(k0 + KB, self.K))
            acc += hhi[:, k] @ self.whi[k]
            a = hlo[:, k] @ self.whi[k]              # W_hi * h_lo
            wlo = self.wlo[k]
            if m[0] == "drop_wlo_hhi_cols" and k.stop > self.K - m[1]:
                wlo = wlo.copy()
                wlo[max(self.K - m[1] - k0, 0):] = 0
            b = hhi[:, k] @ wlo                      # W_lo * h_hi
            if m[0] == "drop_whi_hlo" and kb == m[1]:
                a = np.zeros_like(a)
            if m[0] == "fold_2_10" and kb == m[1]:
                a, b = a * np.float32(2), b * np.float32(2)
            cross += a + b
        return (acc + cross * FOLD).astype(np.float64)


def to_f32(h, t):
    return h.astype(np.float32).astype(np.float64)


def batch_rnn(sd, layer, kind, x, lens, bidirectional, batch_norm, mutant=None, mutant_reverse=False, unfrozen_clip=None):
    """The layer with the split-fp16 recurrent product in both directions; `mutant` in the forward direction (or the reverse one);
    unfrozen_clip: that clip's state is not frozen at its length in the REVERSE direction (its chain starts at T - 1, runs through
    the padding and enters the clip with a state that is not zero)."""
    hooks = {}
    for reverse in ((False, True) if bidirectional else (False,)):
        w_hh = sd["rnns.%d.rnn.weight_hh_l0%s" % (layer, "_reverse" if reverse else "")]
        hooks[reverse] = dict(step=SplitProduct(w_hh, mutant if reverse == mutant_reverse else None), post=to_f32)
    if unfrozen_clip is not None:
        lens_a = np.asarray(lens)
        hooks[True]["freeze"] = lambda t: (t < lens_a) | (np.arange(len(lens_a)) == unfrozen_clip)
    return f64.batch_rnn(sd, layer, kind, x, lens, bidirectional, batch_norm, hooks=hooks)


# ---- the conv stack on the split-fp16 MFMA (conv1_split.hip, conv_split.hip) -----------------------------------------------------
W_SCALE = np.float32(64.0)      # conv_split.hip packs the weights times 2^6 and divides the accumulator by it


def split_unscaled(x):
    """float32 -> (hi, lo), both as float32 arrays holding fp16 values: the operand format of layers 2 and 3"""
    x = np.asarray(x, dtype=np.float32)
    hi = x.astype(np.float16).astype(np.float32)
    return hi, (x - hi).astype(np.float16).astype(np.float32)


def _only(w, kf=None, kt=None):
    """w with everything but kernel row kf (and tap kt of it) zeroed"""
    out = np.zeros_like(w)
    sel = (slice(None), slice(None), slice(None) if kf is None else kf, slice(None) if kt is None else kt)
    out[sel] = w[sel]
    return out


def _bn32(sd, li):
    """a, b of the eval BatchNorm2d as model_build.hip computes them: float32 throughout"""
    p = "conv.seq_module.%d." % (3 * li + 1)
    f = lambda n: np.asarray(sd[p + n], dtype=np.float32)
    a = f("weight") * (np.float32(1) / np.sqrt(f("running_var") + np.float32(1e-5)))
    return a, f("bias") - f("running_mean") * a


class ConvStackEmu:
    """``dsmi_conv_stack`` on the default path, in numpy.  fp16 x fp16 products are exact in float32, so a float32 matrix product
    of the fp16 values is the MFMA up to the order of its additions.

    Layer 1 (conv1_split.hip): both operands ``hi = fp16(x)``, ``lo = fp16((x - hi) * 2^11)``; ``hi*hi`` into one float32
    accumulator, ``lo*hi + hi*lo`` into a second one folded in with 2^-11.  Layers 2 and 3 (conv_split.hip): unscaled lo terms,
    the weights times 64, the three products into ONE accumulator that the epilogue divides by 64.  Epilogue in float32: bias,
    BatchNorm affine, clip to [0, 20], zero at t >= out_len; between the layers the output is split once more.

    ``run(mutant)``, mutant None or one of
      ("l2_drop_wlo_xhi", kf, kt)   layer 2: the W_lo * x_hi product of tap (kf, kt) is missing
      ("l1_drop_whi_xlo", kf)       layer 1: the W_hi * x_lo product of kernel row kf is missing
      ("l1_fold_2_10", kf)          layer 1: kernel row kf's cross terms are folded in with 2^-10
      ("l2_ring_late", kf, f)       layer 2: for output row f, kernel row kf reads the input row two below its own (a ring slot one
                                    turn late)
      ("l2_halo_short",)            layer 2: the last output step of the first 64-step tile loses its rightmost tap (a halo short
                                    by one step)
      ("mask_gt",)                  every layer masks at t > out_len instead of t >= out_len
      ("l2_drop_xlo", kf, kt)       layer 2: the lo plane of the layer-1 output is missing for the 32-channel chunk of tap (kf, kt)
    The clean run's intermediate results are kept: a mutant recomputes from the layer it sits in."""

    def __init__(self, sd, x, out_lens, depth):
        from danspeech_amd.synthetic import CONV_SPECS
        self.sd, self.out_lens, self.depth, self.specs = sd, [int(v) for v in out_lens], depth, CONV_SPECS[:depth]
        self.x = np.asarray(x, dtype=np.float32)
        self.w = [np.asarray(sd["conv.seq_module.%d.weight" % (3 * li)], dtype=np.float32) for li in range(depth)]
        self.acc, self.inp = [None] * depth, [None] * depth        # per layer, of the clean run: accumulator(s), input planes
        self.clean = self._from(0, None, keep=True)

    # -- accumulators
    def _acc1(self, x):
        xh, xl = split(x)
        wh, wl = split(self.w[0])
        S, P = (2, 2), (20, 5)
        return f64.correlate(xh, wh, S, P), f64.correlate(xh, wl, S, P) + f64.correlate(xl, wh, S, P)

    def _wsplit(self, li):
        return split_unscaled(self.w[li] * W_SCALE)

    def _accn(self, li, xh, xl):
        wh, wl = self._wsplit(li)
        S, P = (2, 1), (10, 5)
        return f64.correlate(xh, wl, S, P) + f64.correlate(xl, wh, S, P) + f64.correlate(xh, wh, S, P)

    def _epilogue(self, li, pre, mask_off):
        co = pre.shape[1]
        a, b = _bn32(self.sd, li)
        bias = np.asarray(self.sd["conv.seq_module.%d.bias" % (3 * li)], dtype=np.float32)
        v = (pre + bias.reshape(1, co, 1, 1)) * a.reshape(1, co, 1, 1) + b.reshape(1, co, 1, 1)
        v = np.clip(v, np.float32(0), np.float32(20)).astype(np.float32)
        for i, L in enumerate(self.out_lens):
            v[i, :, :, L + mask_off:] = 0
        return v

    # -- what a mutant adds to the clean accumulator of its layer
    def _delta(self, m):
        if m[0] in ("l1_drop_whi_xlo", "l1_fold_2_10"):
            xh, xl = split(self.x)
            wh, wl = split(self.w[0])
            S, P = (2, 2), (20, 5)
            d = f64.correlate(xl, _only(wh, m[1]), S, P)
            return 0, (-d if m[0] == "l1_drop_whi_xlo" else d + f64.correlate(xh, _only(wl, m[1]), S, P)) * FOLD
        xh, xl = self.inp[1]
        wh, wl = self._wsplit(1)
        S, P = (2, 1), (10, 5)
        if m[0] == "l2_drop_wlo_xhi":
            return 1, -f64.correlate(xh, _only(wl, m[1], m[2]), S, P)
        if m[0] == "l2_drop_xlo":
            return 1, -f64.correlate(xl, _only(wh, m[1], m[2]), S, P)
        if m[0] == "l2_halo_short":
            t = min(self.acc[1].shape[3], 64) - 1
            d = np.zeros_like(self.acc[1])
            for xp, wp in ((xh, wl), (xl, wh), (xh, wh)):
                d[..., t] -= f64.correlate(xp, _only(wp, None, 10), S, P)[..., t]
            return 1, d
        assert m[0] == "l2_ring_late", m
        kf, f = m[1], m[2]
        row = 2 * f + kf - 10
        d = np.zeros_like(self.acc[1])

        def contrib(r):        # kernel row kf on input row r, every step: [B, Co, To]
            if not 0 <= r < xh.shape[2]:
                return 0.0
            return sum(f64.correlate(xp[:, :, r:r + 1, :], wp[:, :, kf:kf + 1, :], (1, 1), (0, 5)) for xp, wp in ((xh, wl), (xl, wh), (xh, wh)))[:, :, 0, :]
        d[:, :, f, :] = contrib(row - 2) - contrib(row)
        return 1, d

    def _from(self, first, mutant, keep=False):
        mask_off = 1 if mutant and mutant[0] == "mask_gt" else 0
        layer, delta = (None, None) if not mutant or mutant[0] == "mask_gt" else self._delta(mutant)
        out = None
        for li in range(first, self.depth):
            if li == 0:
                acc = self.acc[0] if first == 0 and self.acc[0] is not None and not keep else self._acc1(self.x)
                if keep:
                    self.acc[0] = acc
                pre = acc[0] + acc[1] * FOLD
            else:
                inp = self.inp[li] if out is None else split_unscaled(out)
                if keep:
                    self.inp[li] = inp
                pre = self.acc[li] if out is None else self._accn(li, *inp)
                if keep:
                    self.acc[li] = pre
            if layer == li:
                pre = pre + delta
            if li > 0:
                pre = pre * (np.float32(1) / W_SCALE)
            out = self._epilogue(li, pre.astype(np.float32), mask_off)
        return out.astype(np.float64)

    def run(self, mutant=None):
        if mutant is None:
            return self.clean
        if mutant[0] == "mask_gt":
            return self._from(0, mutant)
        layer = 0 if mutant[0].startswith("l1_") else 1
        assert layer < self.depth, "the mutant sits in a layer the stack does not have"
        return self._from(layer, mutant)
