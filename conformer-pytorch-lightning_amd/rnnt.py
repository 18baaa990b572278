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

    rnnt_loss_packed(logits, targets, logit_lengths, target_lengths, blank=-1, clamp=-1, reduction="mean")

The same loss over a packed lattice (cfm/lattice.py): logits [M, V] hold only the valid nodes, utterance b's T_b (U_b+1) rows in (t, u) order
after those of utterances 0..b-1 (M = sum_b T_b (U_b+1), T_b = logit_lengths[b], U_b = target_lengths[b]).

    rnnt_align(logits, targets, logit_lengths, target_lengths, blank=-1)

Forced alignment on the same lattice: the best single path instead of the sum over all of them (cfm_rnnt_align, the max-plus twin of the loss's
alpha recursion; include/cfm.h states it).  Same argument conventions and dtypes as rnnt_loss; no gradient.
"""
import torch

import cfm

__all__ = ["rnnt_loss", "rnnt_loss_packed", "rnnt_align"]


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
    return ag.RNNTLossFn.apply(x, _i32(targets, dev), (_i32(logit_lengths, dev), _i32(target_lengths, dev)), b, float(clamp), reduction)


def rnnt_loss_packed(logits, targets, logit_lengths, target_lengths, blank=-1, clamp=-1, reduction="mean"):
    """rnnt_loss over a packed lattice: logits [M, V], row sum_{b'<b} T_b' (U_b'+1) + t (U_b+1) + u = node (b, t, u); targets [B, >= max U_b];
    the same costs and gradient rows as rnnt_loss on the same nodes (csrc/rnnt.hip, cfm_rnnt_packed_*).  Lengths are clipped to >= 0 and
    target_lengths to targets.size(1).  The row offsets are a prefix sum of the lengths: the lengths are copied to the host ONCE per call
    (the call's only synchronisation with the device)."""
    from cfm import lattice
    if reduction not in ("none", "sum", "mean"):
        raise ValueError("rnnt_loss_packed: reduction must be 'none', 'sum' or 'mean', got %r" % (reduction,))
    cfm.require_hip(logits, targets, logit_lengths, target_lengths)
    if logits.dim() != 2:
        raise ValueError("rnnt_loss_packed: logits must be [M, V], got %s" % (tuple(logits.shape),))
    M, V = logits.shape
    B = logit_lengths.numel()
    if targets.dim() != 2 or targets.size(0) != B or target_lengths.numel() != B or B == 0:
        raise ValueError("rnnt_loss_packed: targets %s / lengths %s, %s do not describe one batch" % (tuple(targets.shape), tuple(logit_lengths.shape),
                                                                                                    tuple(target_lengths.shape)))
    b = blank + V if blank < 0 else blank
    if not 0 <= b < V:
        raise ValueError("rnnt_loss_packed: blank %d outside a vocabulary of %d" % (blank, V))
    T, U = lattice.host_lengths(logit_lengths, target_lengths)
    T, U = T.clip(0, None), U.clip(0, targets.size(1))
    lat = lattice.Lattice.padded(T, U, max(int(T.max()), 1), int(U.max()) + 1, logits.device)
    if lat.M != M:
        raise ValueError("rnnt_loss_packed: logits have %d rows, the lengths describe %d nodes" % (M, lat.M))
    x = logits if logits.stride(1) == 1 else logits.contiguous()
    from cfm import autograd as ag
    return ag.RNNTLossFn.apply(x, _i32(targets, logits.device), lat, b, float(clamp), reduction)


@torch.no_grad()
def rnnt_align(logits, targets, logit_lengths, target_lengths, blank=-1):
    """The best single alignment of each utterance's labels to its frames over the transducer lattice.  Arguments as rnnt_loss.  Returns
    (frame int32 [B, U], token_logp f32 [B, U], score f32 [B]) on the device: frame[b, u] is the frame at which label u is emitted (nondecreasing
    in u; several labels may share a frame), token_logp[b, u] its log-probability at that node, score[b] the log-probability of the whole path
    (at most -rnnt_loss(..., reduction="none")[b]).  Entries at and beyond target_lengths[b] are -1 / -inf; an utterance with logit_lengths[b] = 0
    has no alignment: score -inf and that fill everywhere.  Ties take the blank move (later frames)."""
    cfm.require_hip(logits, targets, logit_lengths, target_lengths)
    if logits.dim() != 4:
        raise ValueError("rnnt_align: logits must be [B, T, U+1, V], got %s" % (tuple(logits.shape),))
    B, T, U1, V = logits.shape
    if targets.dim() != 2 or tuple(targets.shape) != (B, U1 - 1) or logit_lengths.numel() != B or target_lengths.numel() != B:
        raise ValueError("rnnt_align: targets %s / lengths %s, %s do not match logits %s" % (tuple(targets.shape), tuple(logit_lengths.shape),
                                                                                          tuple(target_lengths.shape), tuple(logits.shape)))
    b = blank + V if blank < 0 else blank
    if not 0 <= b < V:
        raise ValueError("rnnt_align: blank %d outside a vocabulary of %d" % (blank, V))
    x = logits.detach()
    if x.stride(3) != 1 or x.stride(1) != U1 * x.stride(2) or x.stride(0) != T * U1 * x.stride(2):
        x = x.contiguous()
    dev = logits.device
    return cfm.rnnt_align(x, _i32(targets, dev), _i32(logit_lengths, dev), _i32(target_lengths, dev), b)
