"""numpy emulation of the recurrent kernels' split-fp16 product inside the float64 cell of tests/_f64_ref.py, and the
mutants tests/test_layer_accuracy_sensitivity.py holds the layer-level bound against.

The product: both operands split once, ``hi = fp16(x)``, ``lo = fp16((x - hi) * 2^11)``; per 32-wide k-block three fp16 products
with float32 accumulation -- ``hi*hi`` into one accumulator, ``hi*lo + lo*hi`` into a second one that is folded in with 2^-11 at the
end.  (An fp16 x fp16 product is exact in float32, so a float32 matmul of the fp16 values is the MFMA up to the order of its 32
additions.)  ``gh`` and the new state are rounded to float32, as the kernels store them; the cell's transcendental functions are
float64 here, the kernels' hardware ``exp`` / ``rcp`` are not emulated.
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
