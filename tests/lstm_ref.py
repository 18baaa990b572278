"""float64 restatement of the multi-layer LSTM the library implements (torch.nn.LSTM(batch_first=True): gate order i, f, g, o), forward and
backward by hand, with the dropout between layers given as a KEEP MASK -- so a case with p > 0 has an oracle although the library's mask
does not come from torch's generator.  keep_masks() restates that mask on the host from csrc/cfm_common.h's keep(seed, index):
murmur3's finaliser over (index * golden ratio) ^ seed, kept iff hash >= p * 2^32; the index is the element's offset in the layer's
TIME-major [U*B, H] output and the layer below layer k uses seed + 0x9E3779B1 * k (include/cfm.h cfm_lstm_desc).

At p = 0 this must agree with float64 nn.LSTM + autograd to 1e-12 (tests/test_lstm_cpu.py) before it is trusted for p > 0.
Plain helper module: no fixtures, no GPU."""
import numpy as np
import torch


def hash32(seed, idx):
    idx = np.asarray(idx, dtype=np.uint64)
    m = np.uint64(0xFFFFFFFF)
    h = ((idx * np.uint64(0x9E3779B1)) & m) ^ np.uint64(seed & 0xFFFFFFFF)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & m
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & m
    h ^= h >> np.uint64(16)
    return h


def keep_masks(p, seed, layers, B, U, H):
    """[None, m_1, .., m_{layers-1}]: m_k float64 [B, U, H] = keep / (1 - p), what multiplies layer k - 1's output on its way into layer k."""
    out = [None]
    for k in range(1, layers):
        if p <= 0.0:
            out.append(None)
            continue
        thresh = int(float(np.float32(p)) * 4294967296.0)
        h = hash32(seed + 0x9E3779B1 * k, np.arange(U * B * H))
        scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
        m = (h >= np.uint64(thresh)).astype(np.float64).reshape(U, B, H) * scale
        out.append(torch.from_numpy(m).transpose(0, 1).contiguous())
    return out


def forward(x, weights, h0=None, c0=None, masks=None):
    """x [B, U, in], weights [(w_ih, w_hh, b_ih, b_hh)] per layer (float64), h0 / c0 [layers, B, H] or None -> (y, hn, cn, cache)."""
    B, U, _ = x.shape
    L, H = len(weights), weights[0][1].shape[1]
    hn, cn, cache, inp = [], [], [], x
    for l, (w_ih, w_hh, b_ih, b_hh) in enumerate(weights):
        if l > 0 and masks is not None and masks[l] is not None:
            inp = inp * masks[l]
        h = torch.zeros(B, H, dtype=x.dtype) if h0 is None else h0[l]
        c = torch.zeros(B, H, dtype=x.dtype) if c0 is None else c0[l]
        steps, ys = [], []
        for t in range(U):
            a = inp[:, t] @ w_ih.T + h @ w_hh.T + b_ih + b_hh
            i, f, g, o = torch.sigmoid(a[:, :H]), torch.sigmoid(a[:, H:2 * H]), torch.tanh(a[:, 2 * H:3 * H]), torch.sigmoid(a[:, 3 * H:])
            c_new = f * c + i * g
            h_new = o * torch.tanh(c_new)
            steps.append((h, c, i, f, g, o, c_new))
            h, c = h_new, c_new
            ys.append(h)
        y = torch.stack(ys, 1)
        cache.append((inp, steps))
        hn.append(h)
        cn.append(c)
        inp = y
    return inp, torch.stack(hn), torch.stack(cn), (cache, weights, masks)


def backward(state, dy, dhn=None, dcn=None):
    """-> (dx, [(dw_ih, dw_hh, db_ih, db_hh)] per layer, dh0, dc0)."""
    cache, weights, masks = state
    L = len(weights)
    grads, dh0, dc0 = [None] * L, [None] * L, [None] * L
    for l in range(L - 1, -1, -1):
        w_ih, w_hh, _, _ = weights[l]
        inp, steps = cache[l]
        B, U, H = dy.shape[0], dy.shape[1], w_hh.shape[1]
        dh = torch.zeros(B, H, dtype=dy.dtype) if dhn is None else dhn[l].clone()
        dc = torch.zeros(B, H, dtype=dy.dtype) if dcn is None else dcn[l].clone()
        dw_ih, dw_hh, db = torch.zeros_like(w_ih), torch.zeros_like(w_hh), torch.zeros(4 * H, dtype=dy.dtype)
        dinp = torch.zeros_like(inp)
        for t in range(U - 1, -1, -1):
            h_prev, c_prev, i, f, g, o, c_new = steps[t]
            dh = dh + dy[:, t]
            tc = torch.tanh(c_new)
            dc = dc + dh * o * (1 - tc * tc)
            da = torch.cat([dc * g * i * (1 - i), dc * c_prev * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)], 1)
            dw_ih += da.T @ inp[:, t]
            dw_hh += da.T @ h_prev
            db += da.sum(0)
            dinp[:, t] = da @ w_ih
            dh = da @ w_hh
            dc = dc * f
        grads[l], dh0[l], dc0[l] = (dw_ih, dw_hh, db, db.clone()), dh, dc
        dy = dinp
        if l > 0 and masks is not None and masks[l] is not None:
            dy = dy * masks[l]
    return dy, grads, torch.stack(dh0), torch.stack(dc0)
