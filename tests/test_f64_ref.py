"""tests/_f64_ref.py -- the float64 BatchRNN layer, conv stack, lookahead and head the stage-level accuracy tests compare the kernels
with -- pinned on the CPU.  The BatchRNN layer: against
the fp32 oracle (oracle/model.py, independent code) on seeded cases of all three kinds, and against the reference's own outputs
(tests/golden/g3_batch_rnn.npz, all 12 tags).

The bounds are float32 noise, not agreement of two float64 programs: the oracle rounds every intermediate to float32.  Measured
here (numpy 2, OpenBLAS; printed by each test): seeded cases 1.1e-7 .. 8.7e-7, held to 2e-6 -- outputs are sums of two values
in (-1, 1), one float32 ulp there is 1.2e-7, and a chain of T <= 23 steps of K <= 96 accumulates a few of them; a semantic
difference (gate order, a mask, the start of the reverse chain, the BatchNorm's epsilon) is 1e-3 or more.  The goldens (torch's
float32 kernels): 6.5e-8 .. 3.8e-7, held to the 2e-6 tests/test_oracle_golden.py holds the oracle to.

The dense stages: against oracle/model.py's conv_stack, lookahead and the fc + softmax part of its forward, one tiny case per conv
depth.  Conv outputs are sums of up to 7392 float32 products of magnitude 1 and below, clipped to [0, 20]: measured 1.1e-6 (depth
1) .. 3e-7, held to 4e-6; a semantic difference (padding, stride, a mask, the BatchNorm's epsilon, the clip) is 1e-3 or more.
Probabilities are at most 1: measured 4e-7, held to 2e-6.

The streaming model (``stream_model``): against oracle/streaming.py on one tiny case per kind -- two utterances on one model, an
is_first with no is_last before it, chunks of 5 / 1 / 1 frames, two sessions in one batch -- held to the probabilities' 2e-6; and
against the reference's own run (tests/golden/g8_streaming.npz) at the 2e-6 tests/test_oracle_streaming.py holds the oracle to."""
import numpy as np
import pytest

import _f64_ref as f64
from danspeech_amd import synthetic as syn
from oracle import model as om

# (H, lens): ragged with a clip of length 1 and one of length T; all equal; T = 1; one clip
SHAPES = [(24, [23, 23, 17, 9, 2, 1]), (96, [12, 12, 12]), (40, [1, 1]), (16, [7])]


@pytest.mark.parametrize("kind", ["gru", "lstm", "rnn"])
@pytest.mark.parametrize("bidir", [True, False])
@pytest.mark.parametrize("layer", [0, 1])
def test_against_the_fp32_oracle(kind, bidir, layer):
    worst = 0.0
    for k, (H, lens) in enumerate(SHAPES):
        sd = syn.make_state_dict(1, kind, H, 2, bidirectional=bidir, context=3, seed=40 + k, ih_gain=1.0 + 2.0 * (k % 2),
                                 sample_rate=100, window_size=0.02)      # n_freq 2: layer 0 reads 32 features
        lens = np.array(lens)
        T, B = int(lens[0]), len(lens)
        I = sd["rnns.%d.rnn.weight_ih_l0" % layer].shape[1]
        x = (np.random.default_rng(50 + k).standard_normal((T, B, I)) * 0.7).astype(np.float32)
        ref = f64.batch_rnn(sd, layer, kind, x, lens, bidir, batch_norm=layer > 0)
        o32 = om.batch_rnn(sd, layer, kind, x, lens, bidir, layer > 0)
        assert ref.dtype == np.float64 and ref.shape == o32.shape == (T, B, H)
        for b, L in enumerate(lens):
            assert not ref[L:, b].any()
            assert np.abs(ref[:L, b]).min() > 0      # ... and nothing inside a clip is left unwritten
        worst = max(worst, float(np.abs(o32 - ref).max()))
    print("%s bidir=%d layer=%d: max |fp32 oracle - f64| = %.3g" % (kind, bidir, layer, worst))
    assert worst <= 2e-6


@pytest.mark.parametrize("kind", ["gru", "lstm", "rnn"])
@pytest.mark.parametrize("bn", [0, 1])
@pytest.mark.parametrize("bidir", [0, 1])
def test_against_the_reference_goldens(golden, kind, bn, bidir):
    g = golden("g3_batch_rnn")
    tag = "%s_bn%d_bi%d" % (kind, bn, bidir)
    sd = {"rnns.0." + k.split("__", 1)[1]: g[k] for k in g.files if k.startswith("w_%s__" % tag)}
    y = f64.batch_rnn(sd, 0, kind, g["x_bn%d" % bn], g["lens"], bool(bidir), bool(bn))
    err = float(np.abs(y - g["y_" + tag]).max())
    print("%s: max |f64 - golden| = %.3g" % (tag, err))
    assert err <= 2e-6
    for b, L in enumerate(g["lens"]):
        assert not y[L:, b].any()


def test_reverse_chain_starts_at_the_clips_last_frame():
    """A clip shorter than T, reverse direction alone: equal to the same clip run by itself at its own length."""
    sd = syn.make_state_dict(1, "gru", 16, 2, seed=7, sample_rate=100, window_size=0.02)
    x = np.random.default_rng(8).standard_normal((9, 2, 16)).astype(np.float32)
    w = f64.layer_weights(sd, 1, True)
    both = f64.direction("gru", x.astype(np.float64), [9, 4], *w, reverse=True)
    alone = f64.direction("gru", x[:4, 1:].astype(np.float64), [4], *w, reverse=True)
    # (two float64 programs: BLAS may sum a batch of two and a batch of one in different orders, nothing more)
    assert np.abs(both[:4, 1] - alone[:, 0]).max() < 1e-14 and not both[4:, 1].any()


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_conv_stack_against_the_fp32_oracle(depth):
    """3 clips of 21 / 20 / 6 frames (11 / 10 / 3 output steps), n_freq 81, features left in place past the lengths."""
    sd = syn.make_state_dict(depth, "gru", 8, 1, seed=60 + depth, sample_rate=8000)
    lens = np.array([21, 20, 6])
    x = np.random.default_rng(61).standard_normal((3, 1, 81, 21)).astype(np.float32)
    out_lens = om.get_seq_lens(lens, depth)
    layers = []
    ref = f64.conv_stack(sd, x, out_lens, depth, layers_out=layers)
    o32 = om.conv_stack(sd, x, out_lens, depth)
    assert ref.dtype == np.float64 and ref.shape == o32.shape == (3, syn.CONV_SPECS[depth - 1][1], syn.conv_out_freq(81, depth), 11)
    assert len(layers) == depth and layers[-1] is ref
    for b, L in enumerate(out_lens):
        assert not ref[b, :, :, L:].any() and ref[b, :, :, :L].any()
    assert ref.min() >= 0.0 and ref.max() <= 20.0 and (ref == 0).any()
    err = float(np.abs(o32 - ref).max())
    print("depth %d: max |fp32 oracle - f64| = %.3g" % (depth, err))
    assert err <= 4e-6
    # the convolution reads the features past a clip's length: zeroing them changes outputs inside the clip
    xz = x.copy()
    xz[2, :, :, 6:] = 0
    assert np.abs(f64.conv_stack(sd, xz, out_lens, depth)[2] - ref[2]).max() > 1e-3


def test_conv_clip_reaches_the_ceiling():
    sd = syn.make_state_dict(1, "gru", 8, 1, seed=62, sample_rate=8000)
    sd["conv.seq_module.0.weight"] = sd["conv.seq_module.0.weight"] * np.float32(20)
    x = np.random.default_rng(63).standard_normal((1, 1, 81, 9)).astype(np.float32)
    ref, o32 = f64.conv_stack(sd, x, [5], 1), om.conv_stack(sd, x, [5], 1)
    assert (ref == 20.0).any() and np.array_equal(ref == 20.0, o32 == 20.0) and np.abs(o32 - ref).max() <= 2e-5


@pytest.mark.parametrize("context,T", [(1, 5), (3, 5), (20, 7), (20, 25)])
def test_lookahead_against_the_fp32_oracle(context, T):
    sd = syn.make_state_dict(1, "gru", 24, 1, bidirectional=False, context=context, seed=64, sample_rate=100)
    sd["lookahead.0.conv.weight"] = sd["lookahead.0.conv.weight"] * np.float32(8)
    x = (np.random.default_rng(65).standard_normal((T, 3, 24)) * 3).astype(np.float32)
    ref, o32 = f64.lookahead(sd, x, context), om.lookahead(sd, x, context)
    assert ref.shape == o32.shape and (ref == 0).any() and (ref == 20).any()
    assert np.abs(o32 - ref).max() <= 2e-5         # values up to 20: one float32 ulp is 1.9e-6, `context` terms


@pytest.mark.parametrize("C,H", [(1, 8), (33, 40), (97, 13)])
def test_head_against_the_fp32_oracle(C, H):
    """oracle/model.py forward's last lines: BatchNorm affine, matmul, transpose, softmax."""
    sd = syn.make_state_dict(1, "gru", H, 1, n_labels=C, seed=66, sample_rate=100)
    x = np.random.default_rng(67).uniform(-2, 2, (6, 2, H)).astype(np.float32)
    ref = f64.head(sd, x)
    a, b = om._bn_affine(sd, "fc.0.module.0")
    y = (x * a + b).astype(np.float32)
    o32 = om.softmax((y.reshape(12, -1) @ sd["fc.0.module.1.weight"].T).reshape(6, 2, -1).transpose(1, 0, 2).astype(np.float32))
    assert ref.shape == o32.shape == (2, 6, C) and np.abs(ref.sum(axis=-1) - 1).max() < 1e-12
    err = float(np.abs(o32 - ref).max())
    print("C %d H %d: max |fp32 oracle - f64| = %.3g" % (C, H, err))
    assert err <= 2e-6


STREAM_SCHEDULE = [(5, True, False), (1, False, False), (1, False, True),                       # the shortest chunks there are
                   (30, True, False), (17, False, False), (12, True, False), (9, False, False), (7, False, True)]      # is_first, no is_last before it


@pytest.mark.parametrize("context", [1, 3])
@pytest.mark.parametrize("kind", ["gru", "lstm", "rnn"])
def test_stream_model_against_the_fp32_oracle(kind, context):
    from oracle import streaming as ost
    H, L = 24, 2
    sd = syn.make_state_dict(2, kind, H, L, bidirectional=False, context=context, seed=68, fc_gain=4.0, sample_rate=100, window_size=0.02)
    cfg = dict(conv_layers=2, rnn_type=kind, rnn_hidden_size=H, rnn_layers=L, bidirectional=False, context=context)
    m64, m32 = f64.stream_model(sd, cfg), ost.StreamingModel(sd, cfg)
    worst, frames = 0.0, []
    for k, (T, first, last) in enumerate(STREAM_SCHEDULE):
        x = syn.make_features(2, T, n_freq=2, seed=690 + k)
        y64, y32 = m64.forward(x, first, last), m32.forward(x, first, last)
        assert (y64 is None) == (y32 is None) == first                   # the first pass of an utterance yields nothing
        frames.append(0 if y64 is None else y64.shape[1])
        if y64 is not None:
            assert y64.dtype == np.float64 and y64.shape == y32.shape and y64.shape[0] == 2
            assert np.abs(y64.sum(axis=-1) - 1).max() < 1e-12
            worst = max(worst, float(np.abs(y32 - y64).max()))
        assert (m64.hidden[0] is None) == last and (m64.la_buf is None) == last
    # context 1 keeps x[-0:], the whole chunk, and yields it again: 10 + 16, 16 + 23 frames; context 3: 10 + 16 - 2, 2 + 23
    assert frames[:3] == ([0, 26, 39] if context == 1 else [0, 24, 25])
    print("%s context %d: max |fp32 oracle - f64| = %.3g" % (kind, context, worst))
    assert worst <= 2e-6


@pytest.mark.parametrize("kind", ["gru", "lstm", "rnn"])
def test_stream_model_against_the_reference_golden(golden, kind):
    """tests/test_oracle_streaming.py's case: the reference's own streaming model, two utterances on one model."""
    g = golden("g8_streaming")
    tag = "%s_c2" % kind
    chunks = [int(v) for v in g["chunks_" + tag]]
    H, L, ctx = 32, 3, 6
    sd = syn.make_state_dict(2, kind, H, L, bidirectional=False, context=ctx, seed=81, fc_gain=4.0)
    m = f64.stream_model(sd, dict(conv_layers=2, rnn_type=kind, rnn_hidden_size=H, rnn_layers=L, bidirectional=False, context=ctx))
    worst = 0.0
    for utt in range(2):
        for ci, T in enumerate(chunks):
            y = m.forward(syn.make_features(1, T, seed=8100 + 100 * utt + ci), ci == 0, ci == len(chunks) - 1)
            ref = g["probs_%s_u%d_k%d" % (tag, utt, ci)]
            if ci == 0:
                assert y is None and ref.size == 0
            else:
                assert y.shape[1:] == ref.shape
                worst = max(worst, float(np.abs(y[0] - ref).max()))
    print("%s: max |f64 - golden| = %.3g" % (tag, worst))
    assert worst <= 2e-6
