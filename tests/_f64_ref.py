"""One ``BatchRNN`` layer in float64: the reference the layer-level accuracy tests hold the kernels (and the fp32 oracle) to.

Plain numpy, float64 throughout.  Inputs and weights are the float32 values widened exactly; nothing is rounded in between.  The
semantics are the ones oracle/model.py documents (reference model.py:114-122) -- restated here, not called:

* layers >= 1: eval-mode BatchNorm1d over the feature axis as the affine map ``x * a + b`` with ``a = w / sqrt(var + 1e-5)``,
  ``b = bias - mean * a``, on every (t, clip) row;
* ``gi = x W_ih^T + b_ih`` for every step at once; per step ``gh = h W_hh^T + b_hh`` and the cell in torch's gate order
  (GRU [r; z; n] with ``n = tanh(gi_n + r * gh_n)``, ``h' = (1 - z) n + z h``; LSTM [i; f; g; o]; RNN ``tanh(gi + gh)``);
* a packed sequence: past a clip's length its state is frozen and its output zero; the reverse chain starts at the clip's last frame;
* the output is the sum of the two directions.

``step`` may be replaced (tests/_split_emu.py puts the split-fp16 product and its mutants there): it gets the direction's float64
state and returns ``h W_hh^T`` without the bias.
"""
import numpy as np

BN_EPS = 1e-5
GATES = {"gru": 3, "lstm": 4, "rnn": 1}


def _f64(a):
    a = np.asarray(a)
    assert a.dtype in (np.float32, np.float64), a.dtype
    return a.astype(np.float64)


def sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


def bn_affine(sd, layer):
    p = "rnns.%d.batch_norm.module." % layer
    a = _f64(sd[p + "weight"]) / np.sqrt(_f64(sd[p + "running_var"]) + BN_EPS)
    return a, _f64(sd[p + "bias"]) - _f64(sd[p + "running_mean"]) * a


def cell(kind, gi, gh, h, c):
    """(h', c') of one step for every clip; gh includes b_hh."""
    H = h.shape[1]
    if kind == "gru":
        r = sigmoid(gi[:, :H] + gh[:, :H])
        z = sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
        n = np.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
        return (1.0 - z) * n + z * h, c
    if kind == "lstm":
        g = gi + gh
        cn = sigmoid(g[:, H:2 * H]) * c + sigmoid(g[:, :H]) * np.tanh(g[:, 2 * H:3 * H])
        return sigmoid(g[:, 3 * H:]) * np.tanh(cn), cn
    assert kind == "rnn", kind
    return np.tanh(gi + gh), c


def direction(kind, x, lens, w_ih, w_hh, b_ih, b_hh, reverse, step=None, freeze=None, post=None):
    """One direction on [T, B, I] float64 -> [T, B, H] float64, zero past each clip's length.

    step(h, t) -> h W_hh^T (default: the exact float64 product); freeze(t) -> bool [B], the clips whose state advances at step t
    (default ``t < lens``); post(h', t) -> h' as the next step sees it (default: unchanged).  The three hooks exist for the emulation
    and the mutants of tests/_split_emu.py; the reference itself uses none."""
    T, B, _ = x.shape
    H = w_hh.shape[1]
    G = GATES[kind]
    assert w_ih.shape[0] == G * H and w_hh.shape == (G * H, H)
    lens = np.asarray(lens)
    gi_all = (x.reshape(T * B, -1) @ w_ih.T + b_ih).reshape(T, B, G * H)
    out = np.zeros((T, B, H))
    h = np.zeros((B, H))
    c = np.zeros((B, H))
    whh_t = np.ascontiguousarray(w_hh.T)
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        valid = t < lens
        act = valid if freeze is None else freeze(t)
        if not act.any():
            continue
        gh = (h @ whh_t if step is None else step(h, t)) + b_hh
        hn, cn = cell(kind, gi_all[t], gh, h, c)
        if post is not None:
            hn = post(hn, t)
        h = np.where(act[:, None], hn, h)
        c = np.where(act[:, None], cn, c)
        out[t] = np.where(valid[:, None], h, 0.0)
    return out


def layer_weights(sd, layer, reverse):
    p = "rnns.%d.rnn." % layer
    s = "_reverse" if reverse else ""
    return tuple(_f64(sd[p + n + s]) for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"))


def batch_rnn(sd, layer, kind, x, lens, bidirectional, batch_norm, hooks=None):
    """BatchRNN.forward in float64.  x: [T, B, I] float32 (widened exactly); lens: [B], each in 1..T.  -> [T, B, H] float64.
    hooks: {reverse (bool): dict(step=, freeze=, post=)} for ``direction`` (tests/_split_emu.py)."""
    x = _f64(x)
    if batch_norm:
        a, b = bn_affine(sd, layer)
        x = x * a + b
    out = None
    for reverse in ((False, True) if bidirectional else (False,)):
        y = direction(kind, x, lens, *layer_weights(sd, layer, reverse), reverse=reverse, **((hooks or {}).get(reverse) or {}))
        out = y if out is None else out + y
    return out
