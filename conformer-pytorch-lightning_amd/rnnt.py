"""RNN-T loss -- drop-in for torchaudio.functional.rnnt_loss as the reference calls it (src/model.py:107, Transducer.rnnt_loss).

    rnnt_loss(logits, targets, logit_lengths, target_lengths, blank=-1, clamp=-1, reduction="mean", fused_log_softmax=True)

Same signature and semantics: logits [B, T, U+1, V] (f32, bf16 or fp16; rows evenly spaced with unit inner stride -- a view with a row stride
ld > V, such as the joint's V+1 wide buffer, is read in place), targets [B, U], logit_lengths / target_lengths [B] (int32 or int64).
blank < 0 means V + blank; reduction "none" returns the per-utterance costs [B], "sum" their sum, "mean" costs.mean().  Differentiable
w.r.t. logits: the gradient is zero outside t < logit_lengths[b], u <= target_lengths[b], and is clamped to [-clamp, clamp] per utterance
before the upstream scale when clamp > 0 (as torchaudio does).  Lengths beyond the tensor sizes are clamped instead of checked (no host
synchronisation); an utterance with logit_lengths[b] = 0 costs +inf with a zero gradient.

The kernels are csrc/rnnt.hip (a row pass, the alpha and beta recursions in one launch, a gradient pass; include/cfm.h cfm_rnnt_*).  There is
no CPU path.  TransducerJoint.rnnt_loss runs the joint and this loss as one differentiable step without a second logits-sized buffer.
"""
import torch

import cfm

__all__ = ["rnnt_loss"]


def _i32(t, device):
    return t.to(device=device, dtype=torch.int32).contiguous()


def rnnt_loss(logits, targets, logit_lengths, target_lengths, blank=-1, clamp=-1, reduction="mean", fused_log_softmax=True):
    if reduction not in ("none", "sum", "mean"):
        raise ValueError("rnnt_loss: reduction must be 'none', 'sum' or 'mean', got %r" % (reduction,))
    if not fused_log_softmax:
        raise NotImplementedError("rnnt_loss: fused_log_softmax=False (logits that are already log-probabilities) is not built")
    cfm.require_hip(logits, targets, logit_lengths, target_lengths)
    if logits.dim() != 4:
        raise ValueError("rnnt_loss: logits must be [B, T, U+1, V], got %s" % (tuple(logits.shape),))
    B, T, U1, V = logits.shape
    if targets.dim() != 2 or tuple(targets.shape) != (B, U1 - 1) or logit_lengths.numel() != B or target_lengths.numel() != B:
        raise ValueError("rnnt_loss: targets %s / lengths %s, %s do not match logits %s" % (tuple(targets.shape), tuple(logit_lengths.shape),
                                                                                         tuple(target_lengths.shape), tuple(logits.shape)))
    b = blank + V if blank < 0 else blank
    if not 0 <= b < V:
        raise ValueError("rnnt_loss: blank %d outside a vocabulary of %d" % (blank, V))
    x = logits
    if x.stride(3) != 1 or x.stride(1) != U1 * x.stride(2) or x.stride(0) != T * U1 * x.stride(2):
        x = x.contiguous()
    from cfm import autograd as ag
    dev = logits.device
    return ag.RNNTLossFn.apply(x, _i32(targets, dev), _i32(logit_lengths, dev), _i32(target_lengths, dev), b, float(clamp), reduction)
