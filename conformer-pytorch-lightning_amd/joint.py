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
loss gradient overwrites them in place (cfm/autograd.py JointRNNTLossFn).  `rnnt_loss(..., packed=True)` builds the logits for the valid cells
(b, t < enc_lens[b], u <= target_lens[b]) only (a packed lattice, cfm/lattice.py), and `forward_window(rows, groups)` runs the loss of every
micro-batch of an accumulation window through one packed lattice over the window's encoder row matrix (the same Function).
`forced_align(enc_out, pred_out, targets, enc_lens, target_lens)` (eval mode) runs the same packed joint and then cfm_rnnt_packed_align: the
best single alignment of known labels on this head, per token its emission frame and log-probability.
"""
import numpy as np
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

    def _params(self):
        return [self.enc_ffn.weight, self.enc_ffn.bias, self.pred_ffn.weight, self.pred_ffn.bias, self.ffn_out.weight, self.ffn_out.bias]

    def _blank(self, blank, what):
        V = self.ffn_out.weight.shape[0]
        b = blank + V if blank < 0 else blank
        if not 0 <= b < V:
            raise ValueError("TransducerJoint.%s: blank %d outside a vocabulary of %d" % (what, blank, V))
        return b

    def rnnt_loss(self, enc_out, pred_out, targets, enc_lens, target_lens, blank=0, clamp=-1, reduction="mean", packed=False):
        """torchaudio.functional.rnnt_loss(self(enc_out, pred_out), targets, enc_lens, target_lens, blank, clamp, reduction) as one step
        (model.py:102-113), differentiable w.r.t. enc_out [B, T, E], pred_out [B, U+1, P] and the six joint parameters; targets [B, U].
        Semantics as rnnt.rnnt_loss; the precision mode is cfm.resolve_precision(self).
        packed=True: the joint, the logits and the loss cover only the valid cells (cfm/lattice.py): the same loss and gradients for less work
        and memory on a ragged batch.  It copies the lengths to the host once per call (the packed offsets are their prefix sum)."""
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
        b = self._blank(blank, "rnnt_loss")
        dev = enc_out.device
        i32 = lambda t: t.to(device=dev, dtype=torch.int32).contiguous()
        T = enc_out.size(1)
        if packed:
            from cfm import lattice
            Tb, Ub = lattice.host_lengths(enc_lens, target_lens)
            lat = lattice.Lattice.padded(Tb.clip(0, T), Ub.clip(0, U1 - 1), T, U1, dev)
        else:
            lat = (B, T, U1, i32(enc_lens), i32(target_lens))
        return ag.JointRNNTLossFn.apply(enc_out.reshape(B * T, enc_out.size(2)), pred_out.reshape(B * U1, pred_out.size(2)), self,
                                        cfm.resolve_precision(self), lat, i32(targets), b, float(clamp), reduction, *self._params())

    def forward_window(self, rows, groups, blank=0, clamp=-1):
        """The RNN-T losses of an accumulation window through ONE packed lattice (train path; mirrors CTCDecoder.forward_window).  rows f32
        [sum B_g T'_g, E]: the window's encoder outputs as one row matrix (ConformerEncoder.forward_window(..., return_rows=True)); groups:
        [(B_g, T'_g, enc_lens_g, pred_out_g (B_g, U_g+1, P), targets_g (B_g, U_g), target_lens_g)] in row order.  Returns a 1-D tensor of the
        micro-batches' losses, entry g equal to rnnt_loss(reduction="mean") on micro-batch g alone.  The lengths of all micro-batches are
        copied to the host once per call (the lattice offsets are their prefix sum)."""
        from cfm import autograd as ag
        from cfm import lattice
        cfm.require_hip(rows)
        if rows.dim() != 2:
            raise ValueError("TransducerJoint.forward_window: rows must be [sum B*T', E], got %s" % (tuple(rows.shape),))
        b = self._blank(blank, "forward_window")
        dev = rows.device
        gs = [(int(B), int(T), el, po, tg, tl) for B, T, el, po, tg, tl in groups]
        host = lattice.host_lengths(*[g[2] for g in gs], *[g[5] for g in gs])
        Umax = max(g[3].size(1) for g in gs) - 1
        Ts, Us, e0, p0, preds, tgts, r, q = [], [], [], [], [], [], 0, 0
        for gi, (B, T, _, po, tg, _) in enumerate(gs):
            U1 = po.size(1)
            if po.dim() != 3 or po.size(0) != B or tuple(tg.shape) != (B, U1 - 1):
                raise ValueError("TransducerJoint.forward_window: group %d: pred_out %s / targets %s do not match B = %d" % (gi, tuple(po.shape), tuple(tg.shape), B))
            Ts.append(host[gi].clip(0, T))
            Us.append(host[len(gs) + gi].clip(0, U1 - 1))
            e0.append(r + np.arange(B) * T)
            p0.append(q + np.arange(B) * U1)
            preds.append(po.reshape(B * U1, po.size(2)))
            tgts.append(nn.functional.pad(tg.to(device=dev, dtype=torch.int32), (0, Umax - (U1 - 1))))
            r, q = r + B * T, q + B * U1
        if rows.size(0) != r:
            raise ValueError("TransducerJoint.forward_window: rows has %d rows, the groups describe %d" % (rows.size(0), r))
        cat = lambda xs: xs[0] if len(xs) == 1 else torch.cat(xs, 0)
        lat = lattice.Lattice(np.concatenate(Ts), np.concatenate(Us), np.concatenate(e0), np.concatenate(p0), r, q, dev)
        nll = ag.JointRNNTLossFn.apply(rows, cat(preds), self, cfm.resolve_precision(self), lat, cat(tgts).contiguous(), b, float(clamp), "none",
                                       *self._params())
        losses, s = [], 0
        for B, *_ in gs:
            losses.append(nll[s:s + B].mean())
            s += B
        return torch.stack(losses)

    @torch.no_grad()
    def forced_align(self, enc_out, pred_out, targets, enc_lens, target_lens, blank=0):
        """Forced alignment of KNOWN labels on the transducer head: the joint over the valid cells only (a packed lattice, as
        rnnt_loss(packed=True)), then cfm_rnnt_packed_align -- the best single path through the lattice (include/cfm.h states the recursion and its
        tie rule).  enc_out [B, T, E], pred_out [B, U+1, P] (the predictor over [blank] + labels), targets [B, U], enc_lens / target_lens (B,).
        Returns a list of B entries: None for an utterance without a frame, else {"score": the path's log-probability, "tokens": [(token, frame,
        logp), ...]} with the encoder frame at which each token is emitted and its log-probability there.  The results come back in one host
        transfer; lengths given as DEVICE tensors cost one more before the joint (the lattice offsets are their prefix sum, as for
        rnnt_loss(packed=True)), lengths given as lists or CPU tensors none."""
        from cfm import lattice
        if self.training:
            raise RuntimeError("TransducerJoint.forced_align is an eval-mode operation (inference only); in train mode call rnnt_loss")
        cfm.require_hip(enc_out, pred_out)
        if enc_out.dim() != 3 or pred_out.dim() != 3 or enc_out.size(0) != pred_out.size(0):
            raise ValueError("TransducerJoint.forced_align: enc_out %s / pred_out %s must be (B, T, E) / (B, U+1, P)" % (tuple(enc_out.shape), tuple(pred_out.shape)))
        B, T, U1 = enc_out.size(0), enc_out.size(1), pred_out.size(1)
        dev = enc_out.device
        targets = torch.as_tensor(targets).to(device=dev, dtype=torch.int32).contiguous()
        enc_lens, target_lens = torch.as_tensor(enc_lens), torch.as_tensor(target_lens)
        if tuple(targets.shape) != (B, U1 - 1) or enc_lens.shape != (B,) or target_lens.shape != (B,):
            raise ValueError("TransducerJoint.forced_align: %d utterances with U = %d, but targets %s, lengths %s, %s" %
                             (B, U1 - 1, tuple(targets.shape), tuple(enc_lens.shape), tuple(target_lens.shape)))
        b = self._blank(blank, "forced_align")
        prec = cfm.resolve_precision(self)
        pk = self._weights(prec)
        on_dev = [t for t in (enc_lens, target_lens) if t.is_cuda]                      # only these cost a transfer (one for both)
        host = iter(lattice.host_lengths(*on_dev)) if on_dev else None
        Tb, Ub = (next(host) if t.is_cuda else t.to(torch.int64).numpy() for t in (enc_lens, target_lens))
        Tb, Ub = Tb.clip(0, T), Ub.clip(0, U1 - 1)
        lat = lattice.Lattice.padded(Tb, Ub, T, U1, dev)
        _, _, e = self._rows(enc_out, 2, "enc_out")
        _, _, p = self._rows(pred_out, 1, "pred_out")
        e = cfm.gemm(e, pk.enc[0], bias=pk.enc[2], w_lo=pk.enc[1], out_dtype=torch.float32)
        p = cfm.gemm(p, pk.pred[0], bias=pk.pred[2], w_lo=pk.pred[1], out_dtype=torch.float32)
        if lat.M:
            a = cfm.joint_act_packed(e, p, lat, prec.act_dtype)
            logits = cfm.gemm(a, pk.out[0], bias=pk.out[2], w_lo=pk.out[1], out_dtype=self.out_dtype)
        else:
            logits = torch.empty((0, pk.Vp), dtype=self.out_dtype, device=dev)
        frame, token_logp, score = cfm.rnnt_align_packed(logits, targets, lat, b, V=pk.V)
        W = lat.U1_max - 1
        # one transfer: everything as float64 columns (frames and labels are far below 2^53)
        res = torch.cat([score.double()[:, None], frame.double(), token_logp.double(), targets.double()], 1).cpu()
        out = []
        for i in range(B):
            U = int(Ub[i])
            if Tb[i] == 0:
                out.append(None)
                continue
            fr, lp, lab = (res[i, 1 + k * W:1 + k * W + U].tolist() for k in range(3))
            out.append({"score": float(res[i, 0]), "tokens": [(int(lab[u]), int(fr[u]), lp[u]) for u in range(U)]})
        return out
