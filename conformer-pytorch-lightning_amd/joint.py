"""Transducer joint network -- drop-in for the class of the same name in the reference's src/joint.py:4-38 (forward only).

    e = enc_ffn(enc_out)   [B*T, J]      cfm_gemm, f32
    p = pred_ffn(pred_out) [B*U, J]      cfm_gemm, f32
    a = tanh(e[b,t] + p[b,u])            cfm_joint_act: ONE 16-bit [B*T*U, J] operand (f32 in the accurate mode)
    out = ffn_out(a)       [B,T,U,V]     cfm_gemm, f32 logits with the reference's own layout (row stride V; V = 5002 is written with
                                         column-pair stores, an odd V through a V+1 wide buffer and a view)

Same constructor arguments, parameter names (`enc_ffn`, `pred_ffn`, `ffn_out`) and the attribute `activatoin` (sic) as the reference;
`forward(enc_out, pred_out, pre_project=True)` accepts the 3-D tensors of model.py:102 / :250 and the 4-D singleton-axis form of
joint.py:29-33.  `out_dtype` (default torch.float32, what the reference returns) may be set to a 16-bit type to halve the 3.3 GB the
logits take at BASELINE config 4.  `forward` has no backward: calling it in train mode with gradients enabled on parameters that require
them raises.  Training goes through `rnnt_loss(enc_out, pred_out, targets, enc_lens, target_lens, ...)`, the joint followed by the RNN-T loss
(torchaudio.functional.rnnt_loss at model.py:107; rnnt.py, csrc/rnnt.hip) as one differentiable step whose logits never leave it, so the
loss gradient overwrites them in place (cfm/autograd.py JointRNNTLossFn).
"""
import torch
import torch.nn as nn

import cfm
from cfm import packing


class TransducerJoint(nn.Module):

    def __init__(self, vocab_size, enc_output_size, pred_output_size, join_dim):
        super().__init__()
        self.activatoin = nn.Tanh()
        self.enc_ffn = nn.Linear(enc_output_size, join_dim)
        self.pred_ffn = nn.Linear(pred_output_size, join_dim)
        self.ffn_out = nn.Linear(join_dim, vocab_size)
        self.out_dtype = torch.float32
        self._pack = packing.PackCache()

    def _weights(self, prec):
        def build():
            def lin(m, pad_rows=0):
                w = m.weight.detach().float()
                b = m.bias.detach().float()
                if pad_rows:
                    w = torch.cat([w, w.new_zeros((pad_rows, w.shape[1]))])
                    b = torch.cat([b, b.new_zeros((pad_rows,))])
                wm, wlo = packing.matrix(w.contiguous(), prec)
                return wm, wlo, b.contiguous()
            V = self.ffn_out.weight.shape[0]
            return packing.Packed(enc=lin(self.enc_ffn), pred=lin(self.pred_ffn), out=lin(self.ffn_out, V & 1), V=V, Vp=V + (V & 1))
        params = [self.enc_ffn.weight, self.enc_ffn.bias, self.pred_ffn.weight, self.pred_ffn.bias, self.ffn_out.weight, self.ffn_out.bias]
        return self._pack.get(params, prec, build)

    @staticmethod
    def _rows(t, axis, what):
        """(B, T, X) or the 4-D form with a singleton at `axis` -> (B, T, f32 contiguous [B*T, X])."""
        if t.dim() == 4:
            if t.size(axis) != 1:
                raise ValueError("TransducerJoint: %s of shape %s is already broadcast; pass (B, N, X) or a singleton axis %d"
                                 % (what, tuple(t.shape), axis))
            t = t.squeeze(axis)
        if t.dim() != 3:
            raise ValueError("TransducerJoint: %s must be 3-D or 4-D, got %s" % (what, tuple(t.shape)))
        B, N, X = t.shape
        return B, N, (t if t.dtype == torch.float32 else t.float()).contiguous().view(B * N, X)

    def forward(self, enc_out, pred_out, pre_project=True):
        """Logits [B, T, U, V] (joint.py:20-38), inference only; for training use `rnnt_loss`, which also runs this joint."""
        if torch.is_grad_enabled() and self.training and any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError("TransducerJoint: backward is not built yet (forward only)")
        cfm.require_hip(enc_out, pred_out)
        prec = cfm.resolve_precision(self)
        pk = self._weights(prec)
        B, T, e = self._rows(enc_out, 2, "enc_out")
        Bp, U, p = self._rows(pred_out, 1, "pred_out")
        if Bp != B:
            raise ValueError("TransducerJoint: batch sizes differ (%d, %d)" % (B, Bp))
        if pre_project:
            e = cfm.gemm(e, pk.enc[0], bias=pk.enc[2], w_lo=pk.enc[1], out_dtype=torch.float32)
            p = cfm.gemm(p, pk.pred[0], bias=pk.pred[2], w_lo=pk.pred[1], out_dtype=torch.float32)
        if e.shape[1] != p.shape[1] or e.shape[1] != pk.out[0].shape[1]:
            raise ValueError("TransducerJoint: join dimensions differ (%d, %d, ffn_out expects %d)" % (e.shape[1], p.shape[1], pk.out[0].shape[1]))
        a = cfm.joint_act(e, p, B, T, U, prec.act_dtype)
        out = cfm.gemm(a, pk.out[0], bias=pk.out[2], w_lo=pk.out[1], out_dtype=self.out_dtype)
        out = out.view(B, T, U, pk.Vp)
        return out if pk.Vp == pk.V else out[..., :pk.V]

    def rnnt_loss(self, enc_out, pred_out, targets, enc_lens, target_lens, blank=0, clamp=-1, reduction="mean"):
        """torchaudio.functional.rnnt_loss(self(enc_out, pred_out), targets, enc_lens, target_lens, blank, clamp, reduction) as one step
        (model.py:102-113), differentiable w.r.t. enc_out [B, T, E], pred_out [B, U+1, P] and the six joint parameters; targets [B, U].
        Semantics as rnnt.rnnt_loss; the precision mode is cfm.resolve_precision(self)."""
        from cfm import autograd as ag
        if reduction not in ("none", "sum", "mean"):
            raise ValueError("TransducerJoint.rnnt_loss: reduction must be 'none', 'sum' or 'mean', got %r" % (reduction,))
        cfm.require_hip(enc_out, pred_out, targets, enc_lens, target_lens)
        if enc_out.dim() == 4:
            enc_out = enc_out.squeeze(2)
        if pred_out.dim() == 4:
            pred_out = pred_out.squeeze(1)
        if enc_out.dim() != 3 or pred_out.dim() != 3 or enc_out.size(0) != pred_out.size(0):
            raise ValueError("TransducerJoint.rnnt_loss: enc_out %s / pred_out %s must be (B, T, E) / (B, U+1, P)"
                             % (tuple(enc_out.shape), tuple(pred_out.shape)))
        B, U1 = pred_out.size(0), pred_out.size(1)
        if tuple(targets.shape) != (B, U1 - 1):
            raise ValueError("TransducerJoint.rnnt_loss: targets %s, expected (%d, %d)" % (tuple(targets.shape), B, U1 - 1))
        V = self.ffn_out.weight.shape[0]
        b = blank + V if blank < 0 else blank
        if not 0 <= b < V:
            raise ValueError("TransducerJoint.rnnt_loss: blank %d outside a vocabulary of %d" % (blank, V))
        dev = enc_out.device
        i32 = lambda t: t.to(device=dev, dtype=torch.int32).contiguous()
        params = [self.enc_ffn.weight, self.enc_ffn.bias, self.pred_ffn.weight, self.pred_ffn.bias, self.ffn_out.weight, self.ffn_out.bias]
        return ag.JointRNNTLossFn.apply(enc_out, pred_out, self, cfm.resolve_precision(self), i32(targets), i32(enc_lens), i32(target_lens), b,
                                        float(clamp), reduction, *params)
