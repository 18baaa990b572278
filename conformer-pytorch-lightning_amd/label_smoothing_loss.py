"""Drop-in for the reference's src/label_smoothing_loss.py: the same constructor, the same forward(x, target), on the device.

The value is the reference's (label_smoothing_loss.py:52-80): per position the divergence between the smoothed target distribution and
log_softmax(x), summed over the positions whose target is not padding_idx and divided by the batch size (or, with normalize_length, by the
number of such positions).  It runs as cfm_lsm_loss / cfm_lsm_grad over the logits (csrc/lsm.hip, the logits form) and cfm_lsm_reduce, in f32,
without a host read, and is differentiable.  One deliberate difference: a call in which EVERY target is padding_idx returns 0 under
normalize_length, where the reference divides 0 by 0."""
import torch
import torch.nn as nn

import cfm
from cfm import autograd as _ag


class LabelSmoothingLoss(nn.Module):
    def __init__(self, size: int, padding_idx: int, smoothing: float, normalize_length: bool = False):
        super().__init__()
        if not 0.0 <= smoothing < 1.0 or (smoothing > 0.0 and size < 2):
            raise ValueError("LabelSmoothingLoss: smoothing in [0, 1) and, when it is not 0, at least two classes; got %r over %r" % (smoothing, size))
        self.padding_idx = padding_idx
        self.confidence = 1.0 - smoothing
        self.smoothing = smoothing
        self.size = size
        self.normalize_length = normalize_length

    def forward(self, x: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        """x: logits (batch, seqlen, class); target (batch, seqlen), padding_idx where a position does not count.  Returns the scalar loss."""
        cfm.require_hip(x, target)                             # no CPU path
        if x.dim() != 3 or x.size(2) != self.size or target.shape != x.shape[:2]:
            raise ValueError("LabelSmoothingLoss: x %s and target %s are not (batch, seqlen, %d) and (batch, seqlen)" % (tuple(x.shape), tuple(target.shape), self.size))
        # exactly target == padding_idx is ignored, as in the reference; any other value outside [0, size) gives NaN (the reference raises there)
        tgt = torch.where(target == self.padding_idx, torch.full_like(target, -1), torch.where(target < 0, torch.full_like(target, self.size), target))
        return _ag.LsmLogitsLossFn.apply(x, tgt, self.size, float(self.smoothing), 0 if self.normalize_length else x.size(0))
