"""Packed ("compact") RNN-T lattices: the host side of include/cfm.h cfm_lattice.

Utterance b of a ragged batch owns the rows [off[b], off[b] + T[b] (U[b]+1)) of a [M, V] logits matrix; row off[b] + t (U[b]+1) + u is
lattice node (b, t, u), and there are no padded rows.  Its encoder rows are enc_row0[b] + t and its predictor rows pred_row0[b] + u, so the
same descriptor describes one padded batch (enc_row0[b] = b T') and the row matrix of an accumulation window whose micro-batches have
different T' (ConformerEncoder.forward_window(return_rows=True)).

The offsets are prefix sums of the lengths, so they are built on the host: the callers (rnnt.rnnt_loss_packed, TransducerJoint.rnnt_loss
(packed=True), TransducerJoint.forward_window) copy the lengths to the host once per call, and `Lattice` copies the offsets back through
pinned memory without waiting for the device.
"""
import numpy as np
import torch

import cfm as _c

JAB_TB = 8                      # frames per partial of cfm_joint_act_packed_bwd (csrc/joint.hip JAB_TB)


def offsets(T, U):
    """off int64 [B+1]: utterance b's rows are [off[b], off[b+1]), T[b] (U[b]+1) of them."""
    T, U = np.asarray(T, np.int64), np.asarray(U, np.int64)
    return np.concatenate([[0], np.cumsum(T * (U + 1))]).astype(np.int64)


def block_offsets(T, U, tb=JAB_TB):
    """blk_off int64 [B+1]: the rows of cfm_joint_act_packed_bwd's partials, ceil(T[b] / tb) (U[b]+1) per utterance."""
    T, U = np.asarray(T, np.int64), np.asarray(U, np.int64)
    return np.concatenate([[0], np.cumsum((T + tb - 1) // tb * (U + 1))]).astype(np.int64)


def row_nodes(T, U):
    """(b, t, u) int64 [M] each: the node of every packed row, in row order."""
    T, U = np.asarray(T, np.int64), np.asarray(U, np.int64)
    bs, ts, us = [], [], []
    for b in range(len(T)):
        t, u = np.meshgrid(np.arange(T[b]), np.arange(U[b] + 1), indexing="ij")
        bs.append(np.full(t.size, b))
        ts.append(t.reshape(-1))
        us.append(u.reshape(-1))
    cat = lambda xs: np.concatenate(xs).astype(np.int64) if xs else np.zeros(0, np.int64)
    return cat(bs), cat(ts), cat(us)


def host_lengths(*lens):
    """The given 1-D length tensors on the host as int64 numpy arrays, with ONE device-to-host copy (the one synchronisation of a packed call)."""
    n = [int(x.numel()) for x in lens]
    flat = torch.cat([x.reshape(-1).to(torch.int64) for x in lens]).cpu().numpy()
    out, i = [], 0
    for k in n:
        out.append(flat[i:i + k])
        i += k
    return out


class Lattice:
    """A cfm_lattice and the device arrays it points to.  T [B] frames, U [B] labels (host, already clipped to what the tensors hold),
    enc_row0 / pred_row0 [B] nondecreasing row bases, n_enc / n_pred the rows of the encoder / predictor matrices."""

    def __init__(self, T, U, enc_row0, pred_row0, n_enc, n_pred, device):
        T, U = np.asarray(T, np.int64), np.asarray(U, np.int64)
        B = len(T)
        if B == 0 or (T < 0).any() or (U < 0).any():
            raise ValueError("cfm.Lattice: need B > 0 utterances with T, U >= 0")
        self.B, self.T, self.U = B, T, U
        self.off_host = offsets(T, U)
        self.M = int(self.off_host[-1])
        self.T_max, self.U1_max = int(T.max()), int(U.max()) + 1
        i64 = np.concatenate([self.off_host, block_offsets(T, U), np.asarray(enc_row0, np.int64), np.asarray(pred_row0, np.int64)])
        i32 = np.concatenate([T, U]).astype(np.int32)
        pin = lambda a: torch.from_numpy(np.ascontiguousarray(a)).pin_memory().to(device, non_blocking=True)
        self.i64, self.i32 = pin(i64), pin(i32)                      # host -> device, no wait for the device
        self.off = self.i64[:B + 1]
        self.blk_off = self.i64[B + 1:2 * B + 2]
        self.n_blk = int(i64[2 * B + 1])
        self.enc_row0, self.pred_row0 = self.i64[2 * B + 2:3 * B + 2], self.i64[3 * B + 2:]
        self.T_dev, self.U_dev = self.i32[:B], self.i32[B:]
        d = _c.Lattice()
        d.B, d.T_max, d.U1_max, d.M = B, self.T_max, self.U1_max, self.M
        d.off, d.T, d.U = self.off.data_ptr(), self.T_dev.data_ptr(), self.U_dev.data_ptr()
        d.enc_row0, d.pred_row0, d.blk_off = self.enc_row0.data_ptr(), self.pred_row0.data_ptr(), self.blk_off.data_ptr()
        d.n_enc, d.n_pred = int(n_enc), int(n_pred)
        self.desc = d

    @classmethod
    def padded(cls, T, U, T_pad, U1_pad, device):
        """The valid cells of one padded batch: encoder rows b T_pad + t, predictor rows b U1_pad + u."""
        B = len(T)
        return cls(T, U, np.arange(B) * T_pad, np.arange(B) * U1_pad, B * T_pad, B * U1_pad, device)
