"""The CTC loss on the library's own forward-backward pass (``dsmi_occupancy``): ``-log p(transcript | logits)`` summed over
every alignment in float64, with its gradient, so that the output layer can be adapted against the same likelihood that
``Decoder.score`` reports.

The gradient is taken AT THE FLOAT32 PROBABILITIES THE LIBRARY SEES: the forward rounds ``softmax(logits)`` to float32 and the
library reads ``lp = log(max(p, FLT_MIN))`` of that.  With ``occ[t, c] = d logp / d lp(t, c)`` the gradient of ``-logp`` with
respect to the logits is ``p - occ`` (the softmax's Jacobian applied to ``-occ``; the rows of ``occ`` sum to 1).  A probability
that was clamped at ``FLT_MIN`` still receives its ``-occ``: the clamp is treated as part of the number format, not as a flat
piece of the function, so a label the transcript needs is pushed up even from p = 0."""
import numpy as np
import torch


class _CtcLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, sizes, ids, decoder):
        P = torch.softmax(logits, -1).float().contiguous()
        dec = decoder._dec(P.device.index or 0)
        B, T = P.shape[0], P.shape[1]
        sz = np.full(B, T, dtype=np.int32) if sizes is None else np.asarray(torch.as_tensor(sizes).cpu()).astype(np.int32)
        lp, occ, _, status = dec.occupancy(P, sz, np.arange(B), ids, want_tok=False)
        ctx.save_for_backward(P, occ)
        ctx.frames = torch.as_tensor(sz, device=P.device)
        ctx.feasible = torch.as_tensor(status == 0, device=P.device)
        ctx.dtype = logits.dtype
        return torch.as_tensor(-lp, device=P.device)              # (-(-inf) = inf for an infeasible transcript)

    @staticmethod
    def backward(ctx, grad_out):
        P, occ = ctx.saved_tensors
        T = P.shape[1]
        live = (torch.arange(T, device=P.device)[None, :] < ctx.frames[:, None]) & ctx.feasible[:, None]       # [B, T]
        g = (P.double() - occ) * grad_out.double()[:, None, None]
        g = torch.where(live[:, :, None], g, torch.zeros_like(g))                   # (0 * inf past an infeasible clip's loss is NaN)
        return g.to(ctx.dtype), None, None, None


def ctc_loss(logits, sizes, ids, decoder):
    """``-log p(ids[b] | logits[b])`` for every clip: CUDA float64 [B], differentiable with respect to ``logits``.
    ``logits`` [B, T, C] pre-softmax activations on the GPU (float32 or float64); ``sizes`` [B] frames per clip or None
    (= T); ``ids`` a list of B label-id sequences (``Decoder.transcript_ids``); ``decoder`` a ``Decoder`` whose labels are
    the C columns.  A transcript that cannot fit its clip's frames gives ``inf`` and a zero gradient; frames past a clip's
    size receive a zero gradient.  See the module's note on where the gradient is taken."""
    from .. import _native
    if len(ids) != len(logits):
        raise ValueError("ctc_loss: transcripts for %d clips and a batch of %d" % (len(ids), len(logits)))
    longest = max([len(t) for t in ids] + [0])
    if longest > _native.OCC_MAX_TOKENS:
        raise ValueError("transcript of %d labels is longer than %d" % (longest, _native.OCC_MAX_TOKENS))
    return _CtcLoss.apply(logits, sizes, [list(map(int, t)) for t in ids], decoder)
