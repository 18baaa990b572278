"""Train-mode forward + backward of the hot path as ``torch.autograd.Function``s over the C ABI (BASELINE config 3).

Each Function's ``forward`` runs the train-mode kernels and keeps what the backward needs; its ``backward`` RETURNS the gradient of
every ``nn.Parameter`` it was given (so ``.grad`` accumulation, DDP reducer hooks and gradient accumulation work as with any torch
op -- SURVEY 8b "Threading").  Nothing here computes: the arithmetic is cfm.gemm (input gradients, on transposed weight packs, with
the activation-derivative epilogues), cfm.gemm_tn (weight / bias gradients), cfm.layernorm_bwd, cfm.attention_bwd,
cfm.dwconv_bn_train(_bwd), cfm.glu_bwd, cfm.col2im_relu_bwd, cfm.conv1_wgrad, cfm.ctc_nll_train_groups / cfm.ctc_grad.

What train mode means here (reference: encoder_layer.py:49-71, convolution.py:34-49, decoder.py:18-23 under module.train()):
  * BatchNorm1d uses BATCH statistics over all B*T' positions, padded frames included (quirk Q6), and updates its running statistics;
  * every nn.Dropout is active.  Dropout is applied by the kernels from a counter-based generator (no bit-parity with torch's RNG, as
    SURVEY 2.2 notes): parity is defined and tested at p = 0;
  * the batch path's positional score term is constant along each softmax row, so linear_pos / pos_bias_v receive an exact
    zero gradient (the reference's is rounding noise ~1e-8) and the term is not evaluated; pos_bias_u rides in linear_q's bias.
"""
import ctypes

import torch

import cfm
from cfm import packing


def _gemm(*args, **kw):
    """cfm.gemm with the training tile choice (cfm.h CFM_TILE_AUTO_TRAIN: K-group tiles allowed), as csrc/train_layer.cpp launches its products."""
    kw.setdefault("tile", cfm.TILE_AUTO_TRAIN)
    return cfm.gemm(*args, **kw)


def _f32c(t):
    return (t if t.dtype == torch.float32 else t.float()).contiguous()


def draw_seed():
    """A fresh 31-bit base seed for one Function call's dropout masks, from torch's CPU generator (torch.manual_seed makes a run
    reproducible; no device round trip).  Sites add small odd offsets."""
    return int(torch.randint(0, 2 ** 31 - 1, (1,)).item())


def _drop(p, seed, site):
    return (float(p), (seed + 0x9E3779B1 * site) & 0xFFFFFFFF) if p and p > 0.0 else None


# ======================================================================================================================
# raw forward / backward pieces (no autograd inside): tensors in, tensors + saved state out
# ======================================================================================================================
def ffn_fwd(pk, x, ln, prec, alpha, act=cfm.ACT_SILU, drop_h=None, drop_o=None):
    """x f32 [M,D] -> (x + alpha * drop_o(FFN(LN(x))), saved).  ln = (gain, bias) or None (no norm, no residual: the bare module).
    drop_h: dropout on the hidden activation (feedforward.py:19); drop_o: on the branch output (encoder_layer.py:58,69); (p, seed) | None."""
    adt = prec.act_dtype
    M = x.shape[0]
    FF = pk.w1.shape[0]
    xn = cfm.layernorm(x, ln[0], ln[1], out1_dtype=adt)[0] if ln is not None else (x if x.dtype == adt else cfm.cast(x, adt))
    z = torch.empty((M, FF), dtype=adt, device=x.device)
    h = _gemm(xn, pk.w1, bias=pk.b1, w_lo=pk.w1_lo, act=act, out_dtype=adt, pre_out=z, drop=drop_h)
    if ln is not None:
        y = _gemm(h, pk.w2, bias=pk.b2, w_lo=pk.w2_lo, residual=x, alpha=alpha, drop=drop_o)
    else:
        y = _gemm(h, pk.w2, bias=pk.b2, w_lo=pk.w2_lo, out_dtype=torch.float32, drop=drop_o)
    return y, (x, xn, z, h)


def ffn_bwd(pk, saved, dy, ln, prec, alpha, act=cfm.ACT_SILU, drop_h=None, drop_o=None):
    """dy f32 [M,D] = d loss / d output -> (dx, grads).  With ln: dx = dy + dLN(...) computed in place over dy."""
    x, xn, z, h = saved
    mma, sp = prec.w_code, prec.split
    dact = cfm.ACT_DSILU if act == cfm.ACT_SILU else cfm.ACT_DRELU
    dyb = dy
    if drop_o is not None:                                          # the branch gradient through the output dropout, as a GEMM operand
        dyb, alpha = cfm.dropout_rows(dy, prec.act_dtype, alpha=alpha, drop=drop_o), 1.0
    dW2, db2 = cfm.gemm_tn(dyb, h, want_colsum=True, alpha=alpha, mma_code=mma, split=sp)
    dz = _gemm(dyb, pk.w2t, w_lo=pk.w2t_lo, act=dact, aux=z, alpha=alpha, out_dtype=prec.act_dtype, drop=drop_h)
    dW1, db1 = cfm.gemm_tn(dz, xn, want_colsum=True, mma_code=mma, split=sp)
    dxn = _gemm(dz, pk.w1t, w_lo=pk.w1t_lo, out_dtype=torch.float32)
    grads = {"w_1.weight": dW1, "w_1.bias": db1, "w_2.weight": dW2, "w_2.bias": db2}
    if ln is None:
        return dxn, grads, None
    dx, dg, db = cfm.layernorm_bwd(x, dxn, ln[0], dres=dy, dx=dy)
    return dx, grads, (dg, db)


def mhsa_fwd(mod, pk, x, ln, B, T, mask8, m_str, prec, relative, drop_a=None, drop_o=None, drop_o2=None):
    """x f32 [B*T,D] -> (x + drop_o(MHSA(LN(x))) (ln given) or MHSA(x), saved).  Batch path: no cache, positional term not evaluated.
    drop_a: dropout on the probabilities (attention.py:93); drop_o / drop_o2: on the projected output (encoder_layer.py:61; the plain
    MHSA's own dropout after linear_out, attention.py:177)."""
    adt = prec.act_dtype
    M, D = x.shape
    H, dk = mod.num_heads, mod.d_k
    xn = cfm.layernorm(x, ln[0], ln[1], out1_dtype=adt)[0] if ln is not None else (x if x.dtype == adt else cfm.cast(x, adt))
    qkv = _gemm(xn, pk.qkv_w, bias=pk.qkv_b, w_lo=pk.qkv_w_lo, out_dtype=adt)
    ctx = torch.empty((M, D), dtype=adt, device=x.device)
    lse = torch.empty((B, H, T), dtype=torch.float32, device=x.device)
    st = (T * 3 * D, 3 * D)
    cfm.attention(qkv, qkv[:, D:], qkv[:, 2 * D:], B, H, T, T, dk, st, st + (dk,), st + (dk,), ctx, mask=mask8, mask_str=m_str, mma_code=prec.w_code,
                  split=prec.split, lse=lse, drop=drop_a)
    if drop_o is None and drop_o2 is not None:
        drop_o, drop_o2 = drop_o2, None
    if ln is not None:
        y = _gemm(ctx, pk.out_w, bias=pk.out_b, w_lo=pk.out_w_lo, residual=x, alpha=1.0, drop=drop_o, drop2=drop_o2)
    else:
        y = _gemm(ctx, pk.out_w, bias=pk.out_b, w_lo=pk.out_w_lo, out_dtype=torch.float32, drop=drop_o, drop2=drop_o2)
    return y, (x, xn, qkv, ctx, lse)


def mhsa_bwd(mod, pk, saved, dy, ln, B, T, mask8, m_str, prec, relative, drop_a=None, drop_o=None, drop_o2=None):
    x, xn, qkv, ctx, lse = saved
    M, D = x.shape
    H, dk = mod.num_heads, mod.d_k
    mma, sp = prec.w_code, prec.split
    if drop_o is None and drop_o2 is not None:
        drop_o, drop_o2 = drop_o2, None
    dyb = dy if drop_o is None else cfm.dropout_rows(dy, prec.act_dtype, drop=drop_o, drop2=drop_o2)
    dWo, dbo = cfm.gemm_tn(dyb, ctx, want_colsum=True, mma_code=mma, split=sp)
    dctx = _gemm(dyb, pk.out_t, w_lo=pk.out_t_lo, out_dtype=prec.act_dtype)
    dqkv = torch.empty_like(qkv)
    st = (T * 3 * D, 3 * D)
    cfm.attention_bwd(qkv, qkv[:, D:], qkv[:, 2 * D:], ctx, dctx, lse, B, H, T, T, dk, st, st, st, dqkv, dqkv[:, D:], dqkv[:, 2 * D:], mask=mask8,
                      mask_str=m_str, mma_code=mma, split=sp, drop=drop_a)
    dWqkv, dbqkv = cfm.gemm_tn(dqkv, xn, want_colsum=True, mma_code=mma, split=sp)
    dxn = _gemm(dqkv, pk.qkv_t, w_lo=pk.qkv_t_lo, out_dtype=torch.float32)
    grads = {"linear_q.weight": dWqkv[:D], "linear_k.weight": dWqkv[D:2 * D], "linear_v.weight": dWqkv[2 * D:],
             "linear_q.bias": dbqkv[:D], "linear_k.bias": dbqkv[D:2 * D], "linear_v.bias": dbqkv[2 * D:],
             "linear_out.weight": dWo, "linear_out.bias": dbo}
    if relative:
        grads["pos_bias_u"] = dbqkv[:D].clone().view(H, dk)       # d/du of (q + u) . k^T = the column sums of dq (its own tensor: autograd
                                                                  # accumulates into what it is handed, and linear_q.bias holds the other copy)
        # softmax-invariant in the batch path (one positional row per utterance broadcast over keys, attention.py:20,84-88)
        grads["pos_bias_v"] = torch.zeros_like(mod.pos_bias_v)
        grads["linear_pos.weight"] = torch.zeros_like(mod.linear_pos.weight)
    if ln is None:
        return dxn, grads, None
    dx, dg, db = cfm.layernorm_bwd(x, dxn, ln[0], dres=dy, dx=dy)
    return dx, grads, (dg, db)


def src_attn_fwd(mod, pk, x, mem, ln, B, Tq, Tk, mask8, prec, drop_a=None, drop_o=None):
    """The decoder layer's cross-attention sub-block (decoder_layer.layer_rows): x f32 [B*Tq, D] -> (x + drop_o(SrcAttn(LN(x), mem, mem)), saved).
    mem [B*Tk, D] in the activation type; mask8 uint8 [B, 1, Tk], the key-validity mask; pk = packing.pack_src_attn_train."""
    adt = prec.act_dtype
    M, D = x.shape
    H, dk = mod.num_heads, mod.d_k
    xn = cfm.layernorm(x, ln[0], ln[1], out1_dtype=adt)[0]
    q = _gemm(xn, pk.q_w, bias=pk.q_b, w_lo=pk.q_w_lo, out_dtype=adt)
    kv = _gemm(mem, pk.kv_w, bias=pk.kv_b, w_lo=pk.kv_w_lo, out_dtype=adt)                   # k | v in one product
    ctx = torch.empty((M, D), dtype=adt, device=x.device)
    lse = torch.empty((B, H, Tq), dtype=torch.float32, device=x.device)
    cfm.attention(q, kv, kv[:, D:], B, H, Tq, Tk, dk, (Tq * D, D), (Tk * 2 * D, 2 * D, dk), (Tk * 2 * D, 2 * D, dk), ctx, mask=mask8, mask_str=(Tk, 0),
                  mma_code=prec.w_code, split=prec.split, lse=lse, drop=drop_a)
    y = _gemm(ctx, pk.out_w, bias=pk.out_b, w_lo=pk.out_w_lo, residual=x, alpha=1.0, drop=drop_o)
    return y, (x, xn, mem, q, kv, ctx, lse)


def src_attn_bwd(mod, pk, saved, dy, ln, B, Tq, Tk, mask8, prec, dmem, drop_a=None, drop_o=None):
    """dy f32 [B*Tq, D] -> (dx, grads, (dgamma, dbeta)); dx = dy + dLN(..) in place over dy.  dmem f32 [B*Tk, D] takes dkv . Wkv on top of what
    it holds (the memory's gradient, accumulated over the layers in f32)."""
    x, xn, mem, q, kv, ctx, lse = saved
    D = x.shape[1]
    H, dk = mod.num_heads, mod.d_k
    mma, sp = prec.w_code, prec.split
    dyb = dy if drop_o is None else cfm.dropout_rows(dy, prec.act_dtype, drop=drop_o)
    dWo, dbo = cfm.gemm_tn(dyb, ctx, want_colsum=True, mma_code=mma, split=sp)
    dctx = _gemm(dyb, pk.out_t, w_lo=pk.out_t_lo, out_dtype=prec.act_dtype)
    dq, dkv = torch.empty_like(q), torch.empty_like(kv)
    cfm.attention_bwd(q, kv, kv[:, D:], ctx, dctx, lse, B, H, Tq, Tk, dk, (Tq * D, D), (Tk * 2 * D, 2 * D), (Tk * 2 * D, 2 * D), dq, dkv, dkv[:, D:],
                      mask=mask8, mask_str=(Tk, 0), mma_code=mma, split=sp, drop=drop_a)
    dWq, dbq = cfm.gemm_tn(dq, xn, want_colsum=True, mma_code=mma, split=sp)
    dWkv, dbkv = cfm.gemm_tn(dkv, mem, want_colsum=True, mma_code=mma, split=sp)
    _gemm(dkv, pk.kv_t, w_lo=pk.kv_t_lo, residual=dmem, alpha=1.0, out=dmem)
    dxn = _gemm(dq, pk.q_t, w_lo=pk.q_t_lo, out_dtype=torch.float32)
    # linear_k.bias adds q . b_k to every score of a row: constant along the softmax, so its gradient is exactly zero (the column sums of dk are
    # rounding noise), as pos_bias_v's in the encoder's batch path
    grads = {"linear_q.weight": dWq, "linear_q.bias": dbq, "linear_k.weight": dWkv[:D], "linear_k.bias": torch.zeros_like(dbkv[:D]), "linear_v.weight": dWkv[D:],
             "linear_v.bias": dbkv[D:], "linear_out.weight": dWo, "linear_out.bias": dbo}
    dx, dg, db = cfm.layernorm_bwd(x, dxn, ln[0], dres=dy, dx=dy)
    return dx, grads, (dg, db)


def conv_module_fwd(mod, pk, x, ln, B, T, keep, prec, drop_o=None):
    """x f32 [B*T,D] -> (x + ConvModule(mask(LN(x))) (ln given) or ConvModule(mask(x)), saved); BatchNorm in training mode."""
    adt = prec.act_dtype
    M, D = x.shape
    if ln is not None:
        if keep is not None:
            xn = cfm.layernorm(x, ln[0], ln[1], want1=False, out2_dtype=adt, row_mask=keep)[1]
        else:
            xn = cfm.layernorm(x, ln[0], ln[1], out1_dtype=adt)[0]
    else:
        xn = x if x.dtype == adt else cfm.cast(x, adt)
    u = torch.empty((M, 2 * D), dtype=adt, device=x.device)
    # without a LayerNorm in front the padded INPUT rows are zeroed in the GEMM (mask_mode 1: acc = 0, bias kept -- quirk Q5)
    glu = _gemm(xn, pk.pw1_w, bias=pk.pw1_b, w_lo=pk.pw1_w_lo, act=cfm.ACT_GLU, out_dtype=adt, pre_out=u,
                   row_mask=keep if ln is None else None, mask_mode=1)
    bn = mod.norm
    momentum = bn.momentum if bn.momentum is not None else 1.0 / float(int(bn.num_batches_tracked) + 1)
    rm = bn.running_mean if bn.track_running_stats else None
    rv = bn.running_var if bn.track_running_stats else None
    c, stats, s = cfm.dwconv_bn_train(glu.view(B, T, D), pk.dw_w, pk.dw_b, pk.gamma, pk.beta, rm, rv, momentum, bn.eps, adt)
    if bn.track_running_stats:
        bn.num_batches_tracked += 1
    if ln is not None:
        y = _gemm(s.view(M, D), pk.pw2_w, bias=pk.pw2_b, w_lo=pk.pw2_w_lo, row_mask=keep, mask_mode=0, residual=x, alpha=1.0, drop=drop_o)
    else:
        y = _gemm(s.view(M, D), pk.pw2_w, bias=pk.pw2_b, w_lo=pk.pw2_w_lo, row_mask=keep, mask_mode=0, out_dtype=torch.float32)
    return y, (x, xn, u, glu, c, stats, s)


def conv_module_bwd(mod, pk, saved, dy, ln, B, T, keep, prec, drop_o=None):
    x, xn, u, glu, c, stats, s = saved
    M, D = x.shape
    adt, mma, sp = prec.act_dtype, prec.w_code, prec.split
    # masked OUTPUT rows have no gradient: with the branch gradient materialised (dropout), its padded rows are zeroed there and the two products
    # run unmasked (the 16-bit weight-gradient kernel without a row mask) -- as csrc/train_layer.cpp does
    dyb = dy if drop_o is None else cfm.dropout_rows(dy, adt, drop=drop_o, row_mask=keep)
    km = keep if drop_o is None else None
    dW2, db2 = cfm.gemm_tn(dyb, s.view(M, D), want_colsum=True, row_mask=km, mma_code=mma, split=sp)
    ds = _gemm(dyb, pk.pw2_t, w_lo=pk.pw2_t_lo, row_mask=km, mask_mode=1 if km is not None else 0, out_dtype=adt)
    dglu, ddw_w, ddw_b, dgamma, dbeta = cfm.dwconv_bn_train_bwd(ds.view(B, T, D), c, stats, glu.view(B, T, D), pk.dw_w, adt)
    du = cfm.glu_bwd(u, dglu.view(M, D), adt)
    # pointwise-conv-1 saw zeroed padded rows: xn already is (LayerNorm path) or is masked here (bare module)
    dW1i, db1i = cfm.gemm_tn(du, xn, want_colsum=True, mma_code=mma, split=sp) if ln is not None or keep is None else _pw1_wgrad_masked(du, xn, keep, mma, sp)
    dxn = _gemm(du, pk.pw1_t, w_lo=pk.pw1_t_lo, out_dtype=torch.float32)
    dW1 = torch.empty_like(dW1i)
    dW1[pk.idx] = dW1i                                            # undo the value / gate row interleave of the pack
    db1 = torch.empty_like(db1i)
    db1[pk.idx] = db1i
    K = pk.dw_w.shape[1]
    grads = {"pointwise_conv1.weight": dW1.view(2 * D, D, 1), "pointwise_conv1.bias": db1, "depthwise_conv.weight": ddw_w.view(D, 1, K),
             "depthwise_conv.bias": ddw_b, "norm.weight": dgamma, "norm.bias": dbeta, "pointwise_conv2.weight": dW2.view(D, D, 1),
             "pointwise_conv2.bias": db2}
    if ln is None:
        if keep is not None:
            dxn = dxn * keep.view(M, 1).to(dxn.dtype)             # bare module: d masked_fill (convolution.py:36-37)
        return dxn, grads, None
    dx, dg, db = cfm.layernorm_bwd(x, dxn, ln[0], row_mask=keep, dres=dy, dx=dy)
    return dx, grads, (dg, db)


def _pw1_wgrad_masked(du, xn, keep, mma, sp):
    """bare ConvolutionModule with a pad mask: the weight gradient sees the masked input rows (bias gradient: all rows)."""
    M = du.shape[0]
    xm = xn * keep.view(M, 1).to(xn.dtype)
    return cfm.gemm_tn(du, xm, want_colsum=True, mma_code=mma, split=sp)


def subsampling_fwd(pk, x, cmvn, prec):
    """x f32 [B,T,F] -> (y f32 [B*T2, D], saved)."""
    adt = prec.act_dtype
    B, T, F = x.shape
    C = pk.C
    T1, F1 = (T - 3) // 2 + 1, (F - 3) // 2 + 1
    T2, F2 = (T1 - 3) // 2 + 1, (F1 - 3) // 2 + 1
    h1 = cfm.conv1_relu(x, pk.w1, pk.b1, adt, cmvn=cmvn, mma=cfm.conv1_relu_mma_supported(C, adt))
    h2 = _gemm(h1, pk.w2, bias=pk.b2, w_lo=pk.w2_lo, act=cfm.ACT_RELU, conv=(C, T1, F1, T2, F2, B * T2 * F2), out_dtype=adt)
    y = _gemm(h2.view(B * T2, F2 * C), pk.wl, bias=pk.bl, w_lo=pk.wl_lo, out_dtype=torch.float32)
    return y, (x, h1, h2, (B, T, F, C, T1, F1, T2, F2), cmvn)


def subsampling_bwd(pk, saved, dy, prec):
    x, h1, h2, (B, T, F, C, T1, F1, T2, F2), cmvn = saved
    adt, mma, sp = prec.act_dtype, prec.w_code, prec.split
    Dout = pk.wl.shape[0]
    h2f = h2.view(B * T2, F2 * C)
    dWl, dbl = cfm.gemm_tn(dy, h2f, want_colsum=True, mma_code=mma, split=sp)
    dh2 = _gemm(dy, pk.wlt, w_lo=pk.wlt_lo, act=cfm.ACT_DRELU, aux=h2f, alpha=1.0, out_dtype=adt).view(B * T2 * F2, C)
    dW2, db2 = cfm.gemm_tn(dh2, h1, conv=(C, T1, F1, T2, F2), want_colsum=True, mma_code=mma, split=sp)
    dcol = _gemm(dh2, pk.w2t, w_lo=pk.w2t_lo, out_dtype=adt)
    dh1 = cfm.col2im_relu_bwd(dcol, h1, adt)
    dw1, db1 = cfm.conv1_wgrad(dh1, x, cmvn=cmvn)
    return {"conv.0.weight": dw1.t().reshape(C, 1, 3, 3), "conv.0.bias": db1,
            "conv.2.weight": dW2.view(C, 3, 3, C).permute(0, 3, 1, 2), "conv.2.bias": db2,
            "out.0.weight": dWl.view(Dout, F2, C).permute(0, 2, 1).reshape(Dout, C * F2), "out.0.bias": dbl}


# ======================================================================================================================
# autograd Functions
# ======================================================================================================================
def _params(mod):
    names, tensors = [], []
    for n, p in mod.named_parameters():
        names.append(n)
        tensors.append(p)
    return names, tensors


def _ordered(names, grads, tensors):
    out = []
    for n, p in zip(names, tensors):
        g = grads.get(n)
        if g is None:
            raise RuntimeError("no gradient was produced for parameter %s" % n)
        out.append(g.reshape(p.shape).to(p.dtype) if p.requires_grad else None)
    return out


class LayerNormFn(torch.autograd.Function):
    """nn.LayerNorm on f32 rows (encoder.py:74 after_norm)."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        x2 = _f32c(x.reshape(-1, x.shape[-1]))
        y = cfm.layernorm(x2, weight.detach(), bias.detach(), eps=eps)[0]
        ctx.save_for_backward(x2, weight)
        ctx.eps, ctx.shape = eps, x.shape
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        x2, weight = ctx.saved_tensors
        dx, dg, db = cfm.layernorm_bwd(x2, _f32c(dy.reshape(x2.shape)), weight.detach(), eps=ctx.eps)
        return dx.view(ctx.shape), dg, db, None


class FeedForwardFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mod, prec, act, *params):
        pk = packing.pack_ffn_train(mod, prec)
        x2 = _f32c(x.reshape(-1, x.shape[-1]))
        ctx.drop_h = _drop(mod.dropout.p, draw_seed(), 1) if mod.dropout.p > 0 else None
        y, saved = ffn_fwd(pk, x2, None, prec, 1.0, act, drop_h=ctx.drop_h)
        ctx.mod, ctx.prec, ctx.pk, ctx.saved, ctx.act, ctx.shape = mod, prec, pk, saved, act, x.shape
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        dx, grads, _ = ffn_bwd(ctx.pk, ctx.saved, _f32c(dy.reshape(-1, dy.shape[-1])), None, ctx.prec, 1.0, ctx.act, drop_h=ctx.drop_h)
        names, tensors = _params(ctx.mod)
        return (dx.view(ctx.shape), None, None, None) + tuple(_ordered(names, grads, tensors))


class AttentionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mod, prec, relative, mask8, m_str, *params):
        pk = packing.pack_mhsa_train(mod, prec, relative)
        B, T, D = x.shape
        p = mod.dropout.p
        seed = draw_seed() if p > 0 else 0
        drops = (_drop(p, seed, 1), None, None if relative else _drop(p, seed, 2))      # probabilities; the plain MHSA also drops its output
        y, saved = mhsa_fwd(mod, pk, _f32c(x.reshape(B * T, D)), None, B, T, mask8, m_str, prec, relative, *drops)
        ctx.args = (mod, prec, relative, mask8, m_str, pk, saved, B, T, D, drops)
        return y.view(B, T, D)

    @staticmethod
    def backward(ctx, dy):
        mod, prec, relative, mask8, m_str, pk, saved, B, T, D, drops = ctx.args
        dx, grads, _ = mhsa_bwd(mod, pk, saved, _f32c(dy.reshape(B * T, D)), None, B, T, mask8, m_str, prec, relative, *drops)
        names, tensors = _params(mod)
        return (dx.view(B, T, D), None, None, None, None, None) + tuple(_ordered(names, grads, tensors))


class ConvModuleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mod, prec, keep, *params):
        pk = packing.pack_conv_module_train(mod, prec)
        B, T, D = x.shape
        y, saved = conv_module_fwd(mod, pk, _f32c(x.reshape(B * T, D)), None, B, T, keep, prec)
        ctx.args = (mod, prec, keep, pk, saved, B, T, D)
        return y.view(B, T, D)

    @staticmethod
    def backward(ctx, dy):
        mod, prec, keep, pk, saved, B, T, D = ctx.args
        dx, grads, _ = conv_module_bwd(mod, pk, saved, _f32c(dy.reshape(B * T, D)), None, B, T, keep, prec)
        names, tensors = _params(mod)
        return (dx.view(B, T, D), None, None, None) + tuple(_ordered(names, grads, tensors))


class SubsamplingFn(torch.autograd.Function):
    """conv.0 + ReLU + conv.2 + ReLU + out.0 of the front-end (convolution.py:70-74); the fbank input gets no gradient."""

    @staticmethod
    def forward(ctx, x, mod, prec, cmvn, *params):
        pk = packing.pack_subsampling_train(mod, prec)
        y, saved = subsampling_fwd(pk, _f32c(x), cmvn, prec)
        ctx.args = (mod, prec, pk, saved)
        B, T2 = x.shape[0], saved[3][6]
        return y.view(B, T2, -1)

    @staticmethod
    def backward(ctx, dy):
        mod, prec, pk, saved = ctx.args
        grads = subsampling_bwd(pk, saved, _f32c(dy.reshape(-1, dy.shape[-1])), prec)
        names, tensors = [], []
        for n, p in mod.named_parameters():
            if n.startswith("conv.") or n.startswith("out."):
                names.append(n)
                tensors.append(p)
        return (None, None, None, None) + tuple(_ordered(names, grads, tensors))


def subsampling_params(mod):
    return [p for n, p in mod.named_parameters() if n.startswith("conv.") or n.startswith("out.")]


# ----------------------------------------------------------------------------------------------------------------------
# the blocks from ONE host call each way (csrc/train_layer.cpp cfm_encoder_train_forward / _backward): the launches of the sub-block
# helpers above, enqueued from C++ (tests/train_block_ref.py composes those helpers into a block and is the specification the tests compare
# against).  EncoderStackFn runs all blocks of the encoder over an accumulation WINDOW (round 3): the micro-batches of the window
# concatenated along the row axis (cfm.h cfm_train_group), each block's weight gradients as ONE grouped launch at the end of its backward,
# gradients written straight into the data-parallel trainer's flat buffer.  EncoderLayerFn runs one block over one micro-batch through the
# same path (one block, one row group, each weight gradient launched where it is computed).
# ----------------------------------------------------------------------------------------------------------------------
_GRAD_FIELDS = {"norm_ff_macaron.weight": "ln_ffm_g", "norm_ff_macaron.bias": "ln_ffm_b", "norm_mha.weight": "ln_mha_g", "norm_mha.bias": "ln_mha_b",
                "norm_conv.weight": "ln_conv_g", "norm_conv.bias": "ln_conv_b", "norm_ff.weight": "ln_ff_g", "norm_ff.bias": "ln_ff_b",
                "norm_final.weight": "ln_final_g", "norm_final.bias": "ln_final_b",
                "feed_forward_macaron.w_1.weight": "ffm_w1", "feed_forward_macaron.w_1.bias": "ffm_b1", "feed_forward_macaron.w_2.weight": "ffm_w2",
                "feed_forward_macaron.w_2.bias": "ffm_b2", "feed_forward.w_1.weight": "ff_w1", "feed_forward.w_1.bias": "ff_b1",
                "feed_forward.w_2.weight": "ff_w2", "feed_forward.w_2.bias": "ff_b2", "self_attn.linear_out.weight": "out_w", "self_attn.linear_out.bias": "out_b",
                "conv_module.pointwise_conv2.weight": "pw2_w", "conv_module.pointwise_conv2.bias": "pw2_b", "conv_module.depthwise_conv.weight": "dw_w",
                "conv_module.depthwise_conv.bias": "dw_b", "conv_module.norm.weight": "bn_g", "conv_module.norm.bias": "bn_b", "self_attn.pos_bias_u": "pos_bias_u"}


# gradients the kernels always write (cfm_dwconv_bn_train_bwd_groups, the pointwise-conv-1 bias column sums) whose parameter a block may lack
_DISCARDED = ("conv_module.pointwise_conv1.bias", "conv_module.depthwise_conv.bias", "conv_module.norm.weight", "conv_module.norm.bias")


def layer_grad_layout(layer, offsets=None):
    """Where each parameter's gradient lives in the block's flat gradient slab: {name: (offset, numel)} in floats (16-byte aligned), the slab
    length, and the device row-offset maps of the two fused products.  offsets: a ready-made {name: offset} (the data-parallel trainer's
    bucket layout) or None for a private slab in named_parameters order.  A block without a conv-module bias or BatchNorm affine gets a
    discard region at the end of its private slab ("discard": its offset) where those gradients go.  Cached on the layer per layout, in a
    slot keyed on the parameters' device."""
    key = None if offsets is None else tuple(sorted(offsets.items()))
    dev = next(layer.parameters()).device
    cache = packing.slot(layer, "_grad_layout").get(dev, dict)
    hit = cache.get(key)
    if hit is not None:
        return hit
    lay, n = {}, 0
    for name, p in layer.named_parameters():
        if offsets is None:
            lay[name] = (n, p.numel())
            n += (p.numel() + 3) // 4 * 4
        else:
            lay[name] = (offsets[name], p.numel())
            n = max(n, offsets[name] + p.numel())
    D = layer.encoder_dim
    discard = None
    if offsets is None and any(name not in lay for name in _DISCARDED):        # (check_params refuses such a block with a flat leaf)
        discard, n = n, n + 2 * D
    ar = torch.arange(D, dtype=torch.int64)
    qo, ko, vo = (lay["self_attn.linear_%s.weight" % c][0] for c in "qkv")
    qb, kb, vb = (lay["self_attn.linear_%s.bias" % c][0] for c in "qkv")
    qkv_row = torch.cat([qo + ar * D, ko + ar * D, vo + ar * D])
    qkv_bias = torch.cat([qb + ar, kb + ar, vb + ar])
    idx = packing.glu_interleave_index(D, torch.device("cpu"))            # GEMM row j of the interleaved pack = reference row idx[j]
    pw1_row = lay["conv_module.pointwise_conv1.weight"][0] + idx * D
    pw1_bias = lay["conv_module.pointwise_conv1.bias"][0] + idx if "conv_module.pointwise_conv1.bias" in lay else discard + idx
    hit = dict(layout=lay, numel=n, discard=discard, qkv_row=qkv_row.to(dev), qkv_bias=qkv_bias.to(dev), pw1_row=pw1_row.to(dev),
               pw1_bias=pw1_bias.to(dev))
    if "self_attn.pos_bias_u" in lay:                                    # pos_bias_u as a second destination of linear_q.bias' column sums
        u0 = lay["self_attn.pos_bias_u"][0]
        hit["qkv_bias2"] = torch.cat([u0 + ar, torch.full((2 * D,), -1, dtype=torch.int64)]).to(dev)
    cache[key] = hit
    return hit


_LN_NAMES = ("norm_ff_macaron", "norm_mha", "norm_conv", "norm_ff", "norm_final")


def _inplace_ptrs(layer):
    """The addresses the weight struct takes from the module itself rather than from the packs: the five LayerNorms' weight and bias and the
    BatchNorm's running statistics.  The packs do not see them (packing.pack_stack_train keys on the other parameters), and a replaced
    Parameter or buffer (`blk.norm_ff.weight = nn.Parameter(...)`, `bn.running_mean = t`, load_state_dict(assign=True)) keeps every
    pack -- the struct must then be rebuilt.  Reads the modules' dicts directly: ~12 pointers per block, on every train step."""
    m = layer._modules
    ptrs = []
    for name in _LN_NAMES:
        p = m[name]._parameters
        ptrs.append(p["weight"].data_ptr())
        ptrs.append(p["bias"].data_ptr())
    b = m["conv_module"]._modules["norm"]._buffers
    for name in ("running_mean", "running_var"):
        t = b.get(name)
        ptrs.append(0 if t is None else t.data_ptr())
    return tuple(ptrs)


def _build_train_weights_struct(layer, pks):
    ffm, att, cv, ff = pks
    w = cfm.LayerTrainWeights()
    for short, name in (("ffm", "norm_ff_macaron"), ("mha", "norm_mha"), ("conv", "norm_conv"), ("ff", "norm_ff"), ("final", "norm_final")):
        ln = getattr(layer, name)
        setattr(w, "ln_%s_g" % short, ln.weight.data_ptr())
        setattr(w, "ln_%s_b" % short, ln.bias.data_ptr())
    for pre, pk in (("ffm", ffm), ("ff", ff)):
        for f in ("w1", "w1_lo", "w2", "w2_lo", "w1t", "w1t_lo", "w2t", "w2t_lo", "b1", "b2"):
            setattr(w, pre + "_" + f, cfm.ptr(getattr(pk, f)))
    for f in ("qkv_w", "qkv_w_lo", "qkv_t", "qkv_t_lo", "out_w", "out_w_lo", "out_t", "out_t_lo", "qkv_b", "out_b"):
        setattr(w, f, cfm.ptr(getattr(att, f)))
    for f in ("pw1_w", "pw1_w_lo", "pw1_t", "pw1_t_lo", "pw2_w", "pw2_w_lo", "pw2_t", "pw2_t_lo", "pw1_b", "pw2_b", "dw_w", "dw_b"):
        setattr(w, f, cfm.ptr(getattr(cv, f)))
    w.bn_gamma, w.bn_beta = cv.gamma.data_ptr(), cv.beta.data_ptr()
    bn = layer.conv_module.norm
    if bn.track_running_stats:
        w.bn_running_mean, w.bn_running_var = bn.running_mean.data_ptr(), bn.running_var.data_ptr()
    w.bn_momentum = bn.momentum if bn.momentum is not None else 1.0 / float(int(bn.num_batches_tracked) + 1)
    w.bn_eps = bn.eps
    return w


_F32_SAVED = ("x1", "x2", "x3", "x4", "c", "lse", "stats")


def train_f32_layout(M, D, BHT, G, L, outputs=True):
    """Where the train path keeps its float32 saves in ONE allocation: per block x1..x4 and c [M,D], the attention's row log-sum-exp lse
    [BHT] and the BatchNorm batch statistics [G,4,D]; then (outputs) the L block outputs xs[1..L] [M,D], the last one the stack's output.
    Every region is rounded up to a multiple of 4 floats, so each starts 16 bytes into the allocation at a multiple of 16 bytes (the f32x4
    row kernels read them; B*H*T' summed over a window is odd for odd head counts).  The kernels index lse per micro-batch from the region's
    start (csrc/train_layer.cpp: sv->lse + bht0), so the padding is never read.
    Returns ([{name: (offset, floats)} per block], [(offset, floats) per block output], total floats); offsets in floats."""
    up4 = lambda n: (n + 3) // 4 * 4
    sizes = dict(x1=M * D, x2=M * D, x3=M * D, x4=M * D, c=M * D, lse=BHT, stats=G * 4 * D)
    blocks, o = [], 0
    for _ in range(L):
        regs = {}
        for name in _F32_SAVED:
            regs[name] = (o, sizes[name])
            o += up4(sizes[name])
        blocks.append(regs)
    outs = []
    if outputs:
        for _ in range(L):
            outs.append((o, M * D))
            o += up4(M * D)
    return blocks, outs, o


_SAVED_ACT = ("xn1", "z1", "h1", "xn2", "qkv", "ctx", "xn3", "u", "glu", "s", "xn4", "z2", "h2")


def _stack_grads(owner, layers, bases, lays, tag, u_table):
    """ctypes array of the blocks' gradient destinations: block i's slab starts at address bases[i], laid out as lays[i] (layer_grad_layout's
    cached dicts); cached per destination and layout.  u_table: pos_bias_u as a second destination of linear_q.bias' column sums (what the
    grouped weight gradients need) instead of a copy after the product."""
    key = (tag, u_table, tuple(bases), tuple(id(lay) for lay in lays))
    return packing.slot(owner, "_stack_g").get(key, lambda: _build_stack_grads(bases, lays, u_table))[0]


def _build_stack_grads(bases, lays, u_table):
    arr = (cfm.LayerTrainGrads * len(lays))()
    for g, base, lay in zip(arr, bases, lays):
        g.slab = base
        for name, field in _GRAD_FIELDS.items():
            if name in lay["layout"]:
                setattr(g, field, base + 4 * lay["layout"][name][0])
            elif name in _DISCARDED:                                # the kernels write it all the same: never a null pointer
                setattr(g, field, base + 4 * lay["discard"])
        g.q_bias = base + 4 * lay["layout"]["self_attn.linear_q.bias"][0]
        g.qkv_row_off, g.qkv_bias_off, g.pw1_row_off, g.pw1_bias_off = (lay[k].data_ptr() for k in ("qkv_row", "qkv_bias", "pw1_row", "pw1_bias"))
        if u_table and "qkv_bias2" in lay:
            g.qkv_bias_off2 = lay["qkv_bias2"].data_ptr()
    return arr, lays                                                # the layouts stay alive with the array keyed on their identity


def _param_grads(layers, slabs, lays):
    """The blocks' slabs as one gradient per parameter, in named_parameters order (None where no gradient is wanted)."""
    grads = []
    for l, slab, lay in zip(layers, slabs, lays):
        for name, p in l.named_parameters():
            off, n = lay["layout"][name]
            grads.append(slab[off:off + n].view(p.shape) if p.requires_grad else None)
    return tuple(grads)


def _train_forward(ctx, x, owner, layers, prec, groups, keep, flat, w_arr, pks, defer):
    """The blocks' forward (cfm_encoder_train_forward) over x f32 [M,D], the rows of the micro-batches `groups` ([(B, T, mask8 | None, (m_sb, m_sq))])
    one after the other; keep u8 [M] | None.  Keeps what _train_backward needs on ctx and returns the last block's output [M,D].
    defer: each block's weight gradients as one grouped launch at the end of its backward (cfm.h cfm_layer_train_io.defer_wgrad)."""
    dev, adt = x.device, prec.act_dtype
    L, G = len(layers), len(groups)
    l0 = layers[0]
    D, FF, H = l0.encoder_dim, l0.hidden_dim, l0.num_heads
    M = x.shape[0]
    BHT = sum(B * H * T for B, T, _, _ in groups)
    # everything the backward needs, in two allocations: act-dtype rows and f32 rows (the block outputs included)
    esz = 4 if adt == torch.float32 else 2
    widths = dict(xn1=D, z1=FF, h1=FF, xn2=D, qkv=3 * D, ctx=D, xn3=D, u=2 * D, glu=D, s=D, xn4=D, z2=FF, h2=FF)
    per_act = M * sum(widths.values())
    regions, outs, n_f32 = train_f32_layout(M, D, BHT, G, L)
    act = torch.empty((L * per_act,), dtype=adt, device=dev)
    f32 = torch.empty((n_f32,), dtype=torch.float32, device=dev)
    sv = (cfm.LayerTrainSaved * L)()
    xs = (ctypes.c_void_p * (L + 1))()
    xs[0] = x.data_ptr()
    pa, pf = act.data_ptr(), f32.data_ptr()
    for l in range(L):
        o = pa + l * per_act * esz
        for name in _SAVED_ACT:
            setattr(sv[l], name, o)
            o += M * widths[name] * esz
        for name, (off, _n) in regions[l].items():
            setattr(sv[l], name, pf + off * 4)
        xs[l + 1] = pf + outs[l][0] * 4
    garr = (cfm.TrainGroup * G)()
    row0 = 0
    for g, (B, T, m8, m_str) in zip(garr, groups):
        g.B, g.T, g.row0, g.attn_mask, g.am_sb, g.am_sq = B, T, row0, cfm.ptr(m8), m_str[0], m_str[1]
        row0 += B * T
    io = cfm.LayerTrainIO()
    io.D, io.H, io.FF, io.ktaps, io.act_dtype, io.w_dtype = D, H, FF, l0.kernel_size, prec.act_code, prec.w_code
    io.pad_valid = cfm.ptr(keep)
    p_br, p_a = l0.dropout.p, l0.self_attn.dropout.p
    io.p_hidden_m, io.p_hidden, io.p_branch, io.p_attn = l0.feed_forward_macaron.dropout.p, l0.feed_forward.dropout.p, p_br, p_a
    io.p_attn_out = 0.0 if l0.use_relative else p_a
    io.seed = draw_seed() if max(io.p_hidden_m, io.p_hidden, p_br, p_a) > 0 else 0
    io.deterministic = 1 if cfm.ops._deterministic[0] else 0
    io.n_groups, io.groups, io.defer_wgrad = G, garr, 1 if defer else 0
    ws = sum(cfm.lib().cfm_dwconv_bn_ws(B, T, D) for B, T, _, _ in groups)
    sc = cfm.LayerTrainScratch()
    sc.dwbn_ws = cfm.scratch("dwbn", ws, torch.float32, dev).data_ptr()
    cfm.call("cfm_encoder_train_forward", L, w_arr, ctypes.byref(io), sv, ctypes.byref(sc), xs)
    if l0.conv_module.norm.track_running_stats:
        torch._foreach_add_([l.conv_module.norm.num_batches_tracked for l in layers], G)
    # held: what the structs point to -- the backward reads the saves, the input rows, the masks of the groups and the pad mask
    ctx.st = (owner, layers, prec, flat, defer, w_arr, pks, io, garr, sv, xs, (act, f32, x, groups, keep), M, BHT, ws)
    return f32[outs[-1][0]:outs[-1][0] + M * D].view(M, D)


def _train_backward(ctx, dy, use_sinks):
    """The blocks' backward (cfm_encoder_train_backward) -> (dx f32 [M,D], one slab per block | None, the blocks' gradient layouts).
    use_sinks: write the gradients into the trainer's flat gradient buffer itself when every block is registered with a sink (trainer.py: its
    range of the buffer + a ready hook, called from the per-block callback; needs the atomic sums) -- nothing is then returned for the leaves
    (slabs None).  Otherwise one zero-filled slab per block, laid out as the block's flat leaf (flat) or in named_parameters order."""
    owner, layers, prec, flat, defer, w_arr, pks, io, garr, sv, xs, held, M, BHT, ws = ctx.st
    dev, adt = dy.device, prec.act_dtype
    L = len(layers)
    l0 = layers[0]
    D, FF = l0.encoder_dim, l0.hidden_dim
    sinks = [l.__dict__.get("_flat_grad_sink") for l in layers] if use_sinks else None
    if sinks is not None and any(s is None or s[0].device != dev for s in sinks):
        sinks = None
    lays = [layer_grad_layout(l, l.__dict__.get("_flat_grad_offsets") if flat else None) for l in layers]
    if sinks is not None:
        slabs = None
        g_arr = _stack_grads(owner, layers, [s[0].data_ptr() for s in sinks], lays, "sink", defer)
        io.grads_accumulate = 1
    else:
        sizes = [(l.__dict__["_flat_leaf"].numel() if flat else lay["numel"]) for l, lay in zip(layers, lays)]
        slab_all = torch.zeros((sum(sizes),), dtype=torch.float32, device=dev)
        slabs, o = [], 0
        for n in sizes:
            slabs.append(slab_all[o:o + n])
            o += n
        g_arr = _stack_grads(owner, layers, [s.data_ptr() for s in slabs], lays, "slab", defer)
        io.grads_accumulate = 0
    sc = cfm.LayerTrainScratch()
    sc.dxn = cfm.scratch("t_dxn", M * D, torch.float32, dev).data_ptr()
    for name, wd in (("dz", FF), ("dz2", FF), ("dyb", D), ("dyb2", D), ("dyb3", D), ("dyb4", D), ("du", 2 * D), ("dqkv", 3 * D), ("ds", D), ("dglu", D),
                     ("dctx", D)):
        setattr(sc, name, cfm.scratch("t_" + name, M * wd, adt, dev).data_ptr())
    sc.delta = cfm.scratch("attn_delta", BHT, torch.float32, dev).data_ptr()
    sc.ln_ws = cfm.scratch("ln_bwd", cfm.lib().cfm_layernorm_bwd_ws(M, D), torch.float32, dev).data_ptr()
    sc.dwbn_ws = cfm.scratch("dwbn", ws, torch.float32, dev).data_ptr()
    sc.dy_ws = cfm.scratch("dwbn_dy", M * D, torch.float32, dev).data_ptr()
    dyc = _f32c(dy.reshape(M, D))
    bufs = torch.empty((2, M, D), dtype=torch.float32, device=dev)
    failed = []

    def done(layer, _user):
        if sinks is not None:
            try:
                sinks[layer][1]()                                   # the trainer's ready hook: this block's bucket may be all-reduced
            except BaseException as e:                              # noqa: BLE001 -- ctypes would swallow it: re-raised below
                failed.append(e)

    cb = cfm.LAYER_DONE_FN(done)
    out = ctypes.c_void_p()
    cfm.call("cfm_encoder_train_backward", L, w_arr, ctypes.byref(io), sv, ctypes.byref(sc), g_arr, xs, dyc.data_ptr(), bufs[0].data_ptr(),
             bufs[1].data_ptr(), cb, None, ctypes.byref(out))
    if failed:
        raise failed[0]
    dx = bufs[0] if out.value == bufs[0].data_ptr() else bufs[1]
    return dx, slabs, lays


def check_params(layers, flat):
    """The weight structs and packs read the blocks' parameters through raw f32 pointers.  flat: views of the trainer's flat f32 leaf (trainer.py) --
    contiguous float32 by construction, so the walk over the module tree (~0.1 ms of host time per call; the training step is host-bound) is
    skipped; the leaf's gradient has no room for the gradients of absent parameters (layer_grad_layout's discard region)."""
    if flat:
        cvs = [l.conv_module for l in layers]
        if any(t is None for cv in cvs for t in (cv.pointwise_conv1.bias, cv.depthwise_conv.bias, cv.norm.weight, cv.norm.bias)):
            raise RuntimeError("a block registered with a flat parameter leaf (trainer.py) needs every conv-module bias and BatchNorm affine parameter")
        return
    for i, l in enumerate(layers):
        for name, p in l.named_parameters():
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise TypeError("train mode needs contiguous float32 parameters: block %d's %s is %s%s" %
                                (i, name, p.dtype, "" if p.is_contiguous() else ", not contiguous"))


class EncoderLayerFn(torch.autograd.Function):
    """One conformer block in train mode (encoder_layer.py:49-71): four residual sub-blocks + norm_final, one autograd node -- the stack path
    over one block and one micro-batch."""

    @staticmethod
    def forward(ctx, x, layer, prec, mask8, m_str, keep, *params):
        B, T, D = x.shape
        ctx.flat = len(params) == 1 and params[0] is getattr(layer, "_flat_leaf", None)
        check_params([layer], ctx.flat)
        ctx.shape = x.shape
        w_arr, pks = _stack_weights(layer, [layer], prec, ctx.flat)
        y = _train_forward(ctx, _f32c(x.reshape(B * T, D)), layer, [layer], prec, [(B, T, mask8, m_str)], keep, ctx.flat, w_arr, pks, False)
        return y.view(B, T, D)

    @staticmethod
    def backward(ctx, dy):
        dx, slabs, lays = _train_backward(ctx, dy, False)
        head = (dx.view(ctx.shape), None, None, None, None, None)
        if ctx.flat:                                              # one gradient for the block's flat parameter leaf (trainer.py)
            return head + (slabs[0],)
        return head + _param_grads(ctx.st[1], slabs, lays)


def stack_supported(layers, n_groups):
    """Whether the blocks can share one io struct over n_groups micro-batches: the same sizes and dropout rates, and -- with several micro-batches
    -- no cumulative moving average (BatchNorm momentum=None), whose factor changes from one micro-batch to the next."""
    l0 = layers[0]
    key = lambda l: (l.encoder_dim, l.hidden_dim, l.num_heads, l.kernel_size, l.use_relative, l.dropout.p, l.self_attn.dropout.p,
                     l.feed_forward_macaron.dropout.p, l.feed_forward.dropout.p, l.conv_module.norm.track_running_stats)
    return all(key(l) == key(l0) and (n_groups == 1 or l.conv_module.norm.momentum is not None) for l in layers)


def _stack_weights(owner, layers, prec, flat):
    """ctypes array of the blocks' weight structs (cached while the packs stay the same objects and _inplace_ptrs the same addresses; the
    slot keeps the packs alive beside the array)."""
    pks = packing.pack_stack_train(owner, layers, prec, layers[0].use_relative, flat)

    def build():
        arr = (cfm.LayerTrainWeights * len(layers))()
        for i, (l, pk) in enumerate(zip(layers, pks)):
            arr[i] = _build_train_weights_struct(l, pk)
        return arr, pks
    arr = packing.slot(owner, "_stack_w").get((tuple(id(pk) for pk in pks), tuple(_inplace_ptrs(l) for l in layers)), build)[0]
    for w, l in zip(arr, layers):
        bn = l.conv_module.norm
        if bn.momentum is None:                                 # cumulative moving average: the factor follows the batch count
            w.bn_momentum = 1.0 / float(int(bn.num_batches_tracked) + 1)
    return arr, pks


class EncoderStackFn(torch.autograd.Function):
    """All conformer blocks of the encoder in train mode over one accumulation window (encoder.py:72-73 under module.train())."""

    @staticmethod
    def forward(ctx, x, owner, layers, prec, groups, keep, flat, *params):
        """x f32 [M,D]: the window's rows, micro-batch after micro-batch; groups: [(B, T, mask8 | None, (m_sb, m_sq))]; keep u8 [M] | None."""
        D = layers[0].encoder_dim
        M = sum(B * T for B, T, _, _ in groups)
        if tuple(x.shape) != (M, D) or x.dtype != torch.float32 or not x.is_contiguous():
            raise RuntimeError("EncoderStackFn: rows must be contiguous float32 (%d,%d), got %s %s" % (M, D, tuple(x.shape), x.dtype))
        if len(groups) > 8:
            raise RuntimeError("EncoderStackFn: at most 8 micro-batches per window")
        w_arr, pks = _stack_weights(owner, layers, prec, flat)
        return _train_forward(ctx, x, owner, layers, prec, groups, keep, flat, w_arr, pks, True)

    @staticmethod
    def backward(ctx, dy):
        layers, flat = ctx.st[1], ctx.st[3]
        # where the gradients go: the trainer's flat gradient buffer itself (each block registered with a sink: trainer.py) -- nothing is
        # returned to autograd for the leaves -- or one zero-filled slab per block (plain autograd / deterministic sums), returned as the
        # leaves' / parameters' gradients
        dx, slabs, lays = _train_backward(ctx, dy, flat and not cfm.ops._deterministic[0])
        head = (dx, None, None, None, None, None, None)
        if slabs is None:
            return head + (None,) * len(layers)
        if flat:
            return head + tuple(slabs)
        return head + _param_grads(layers, slabs, lays)


class CTCLossFn(torch.autograd.Function):
    """The CTC heads of an accumulation window in one projection (a single batch is a window of one micro-batch): the window's rows are one [M, D]
    matrix (ConformerEncoder.forward_window), so the vocabulary projection, its weight gradient and its input gradient each run ONCE over all
    micro-batches' rows; the recursions and the per-row gradients run per micro-batch on slices of the one logits matrix (each micro-batch has its
    own T', label width and normaliser).  Returns the micro-batches' losses (sum_b nll_b / padded label length each, decoder.py:19-22) as a 1-D
    tensor."""

    @staticmethod
    def forward(ctx, rows, mod, prec, groups, weight, bias):
        """rows f32 [M, D]; groups: [(B, T, enc_lens i32 [B], labels i32 [B,U], label_lens i32 [B])], rows of micro-batch g at sum of earlier B*T."""
        pk = packing.pack_ctc_train(mod, prec)
        x2 = _f32c(rows)
        logits = _gemm(x2, pk.w, bias=pk.b, w_lo=pk.w_lo, out_dtype=torch.float32)
        problems, r0 = [], 0
        for B, T, enc_lens, labels, label_lens in groups:
            problems.append((logits[r0:r0 + B * T].view(B, T, pk.Vp), enc_lens, labels, label_lens))
            r0 += B * T
        res = cfm.ctc_nll_train_groups(problems, pk.V)         # the recursions of all micro-batches in one launch
        losses = torch.empty((len(groups),), dtype=torch.float32, device=x2.device)
        for g, ((nll, _), pr) in enumerate(zip(res, problems)):
            torch.div(nll.sum(), pr[2].size(1), out=losses[g])
        states = [st for _, st in res]
        if r0 != x2.shape[0]:
            raise RuntimeError("CTCLossFn: the micro-batches cover %d rows, the row matrix has %d" % (r0, x2.shape[0]))
        ctx.args = (prec, pk, x2, logits, states, groups)
        return losses

    @staticmethod
    def backward(ctx, gout):
        prec, pk, x2, logits, states, groups = ctx.args
        gdev = _f32c(gout.reshape(-1))
        dlog = torch.empty_like(logits)
        r0 = 0
        for gi, ((B, T, enc_lens, labels, label_lens), state) in enumerate(zip(groups, states)):
            cfm.ctc_grad(logits[r0:r0 + B * T].view(B, T, pk.Vp), pk.V, enc_lens, labels, label_lens, state, gscale=1.0 / labels.size(1),
                         gscale_dev=gdev[gi:gi + 1], out=dlog[r0:r0 + B * T].view(B, T, pk.Vp))
            r0 += B * T
        dW, db = cfm.gemm_tn(dlog, x2, want_colsum=True, mma_code=prec.w_code, split=prec.split)
        dx = _gemm(dlog, pk.wt, w_lo=pk.wt_lo, out_dtype=torch.float32)
        return dx, None, None, None, dW[:pk.V], db[:pk.V]


def _lsm_row_scale(gout, target, red):
    """g[m] of cfm.lsm_grad: the upstream gradient over the denominator (red = cfm.lsm_reduce's pair), 0 on ignored rows; no host read."""
    return (target >= 0).to(torch.float32) * (gout.reshape(()).to(torch.float32) / red[1])


class LsmLossFn(torch.autograd.Function):
    """The label-smoothing loss of an output projection over rows [M, D] (label_smoothing_loss.py:52-80 behind a Linear): sum_m loss_m / denom,
    denom = batch, or with batch = 0 the number of targets >= 0 (normalize_length), counted on the device; no valid target gives 0.
    fused=False (the default): cfm_gemm to f32 logits, kept for the backward, and the kernels' logits form.  fused=True (16-bit modes with
    D % 8 == 0 and D <= 512; otherwise ignored): cfm_lsm_loss / cfm_lsm_grad on cfm_token_logprob's product loop, the logits never stored --
    the path for a vocabulary whose logits should not be held.  Measured at the recipe's shape (992 rows, D = 256, V = 5002, bf16, MI355X):
    the fused forward is 3.5x SLOWER than the unfused pair (its 16 workgroups leave most of the device idle; scripts/bench_lsm.py),
    so it is not the default.  The projection's gradients are the existing products, as in CTCLossFn."""

    @staticmethod
    def forward(ctx, rows, target, linear, prec, smoothing, batch, fused, weight, bias):
        pk = packing.pack_vocab_train(linear, prec)
        D = rows.shape[1]
        fused = bool(fused) and not prec.split and D % 8 == 0 and D <= 512
        x = rows if rows.dtype == prec.act_dtype else cfm.cast(rows, prec.act_dtype)
        x = x if x.is_contiguous() else x.contiguous()
        target = target.reshape(-1).to(torch.int32).contiguous()
        logits = None if fused else _gemm(x, pk.w, bias=pk.b, w_lo=pk.w_lo, out_dtype=torch.float32)
        loss, lse = cfm.lsm_loss(x, pk.w, pk.b, target, pk.V, smoothing) if fused else cfm.lsm_loss(None, None, None, target, pk.V, smoothing, logits=logits)
        red = cfm.lsm_reduce(loss, target, batch)
        ctx.args = (prec, pk, x, logits, target, lse, red, smoothing)
        return red[0].clone()

    @staticmethod
    def backward(ctx, gout):
        prec, pk, x, logits, target, lse, red, smoothing = ctx.args
        g = _lsm_row_scale(gout, target, red)
        if logits is None:
            dz = cfm.lsm_grad(x, pk.w, pk.b, target, pk.V, smoothing, lse, g)
        else:
            dz = cfm.lsm_grad(None, None, None, target, pk.V, smoothing, lse, g, logits=logits, out_dtype=prec.act_dtype)
        dW, db = cfm.gemm_tn(dz, x, want_colsum=True, mma_code=prec.w_code, split=prec.split)
        dx = _gemm(dz, pk.wt, w_lo=pk.wt_lo, out_dtype=torch.float32)
        return dx, None, None, None, None, None, None, dW[:pk.V], db[:pk.V]


def _p(module):
    return float(module.p) if module.training else 0.0


class DecoderLossFn(torch.autograd.Function):
    """A whole decoder.TransformerDecoder and its label-smoothing loss in one node: embedding E[tok] * sqrt(D) + pe[position], positional dropout,
    per layer mhsa_fwd (relative=False, the [B, Lc, Lc] causal-and-length mask), src_attn_fwd, ffn_fwd(ACT_RELU); after_norm; the loss as LsmLossFn
    computes it.  memory [B, T, D] is differentiable (its gradient is the sum of the layers' dkv . Wkv, f32).  Dropout site k is
    (p, seed + 0x9E3779B1 * k): 0 positional; per layer l at 1 + 6 l: self-attention probabilities, self-attention output, source-attention
    probabilities, source-attention output, feed-forward hidden, feed-forward output.  C-entry calls per layer: 12 forward, 19 backward, and one
    cfm_dropout_rows per active branch-output dropout in the backward."""

    @staticmethod
    def forward(ctx, memory, dec, ys_in, ys_out, self_mask8, mem_mask8, prec, smoothing, batch, seed, fused, *params):
        import math
        B, Lc = ys_in.shape
        T, D = memory.shape[1], memory.shape[2]
        adt = prec.act_dtype
        mem = _f32c(memory.detach().reshape(B * T, D))
        mem = mem if adt == torch.float32 else cfm.cast(mem, adt)
        E = dec.embed[0].weight.detach()
        x = (E[ys_in.long()].double() * math.sqrt(D) + dec.position_table(Lc)[:Lc].double()).float().reshape(B * Lc, D).contiguous()
        d_pos = _drop(_p(dec.embed[1].dropout), seed, 0)
        if d_pos is not None:
            x = cfm.dropout_rows(x, torch.float32, drop=d_pos)
        saved, drops = [], []
        for l, layer in enumerate(dec.decoders):
            sa, ca, ff = layer.self_attn, layer.src_attn, layer.feed_forward
            po, k = _p(layer.dropout), 1 + 6 * l
            dr = (_drop(_p(sa.dropout), seed, k), _drop(po, seed, k + 1), _drop(_p(ca.dropout), seed, k + 2), _drop(po, seed, k + 3),
                  _drop(_p(ff.dropout), seed, k + 4), _drop(po, seed, k + 5))
            x, s1 = mhsa_fwd(sa, packing.pack_mhsa_train(sa, prec, False), x, (layer.norm1.weight, layer.norm1.bias), B, Lc, self_mask8, (Lc * Lc, Lc), prec,
                             False, drop_a=dr[0], drop_o=dr[1])
            x, s2 = src_attn_fwd(ca, packing.pack_src_attn_train(ca, prec), x, mem, (layer.norm2.weight, layer.norm2.bias), B, Lc, T, mem_mask8, prec,
                                 drop_a=dr[2], drop_o=dr[3])
            x, s3 = ffn_fwd(packing.pack_ffn_train(ff, prec), x, (layer.norm3.weight, layer.norm3.bias), prec, 1.0, act=cfm.ACT_RELU, drop_h=dr[4], drop_o=dr[5])
            saved.append((s1, s2, s3))
            drops.append(dr)
        xn = cfm.layernorm(x, dec.after_norm.weight, dec.after_norm.bias, out1_dtype=adt)[0]
        pk = packing.pack_vocab_train(dec.output_layer, prec)
        fused = bool(fused) and not prec.split and D % 8 == 0 and D <= 512
        target = ys_out.reshape(-1).to(torch.int32).contiguous()
        logits = None if fused else _gemm(xn, pk.w, bias=pk.b, w_lo=pk.w_lo, out_dtype=torch.float32)
        loss, lse = cfm.lsm_loss(xn, pk.w, pk.b, target, pk.V, smoothing) if fused else cfm.lsm_loss(None, None, None, target, pk.V, smoothing, logits=logits)
        red = cfm.lsm_reduce(loss, target, batch)
        ctx.args = (dec, prec, pk, x, xn, logits, target, lse, red, smoothing, saved, drops, d_pos, ys_in, self_mask8, mem_mask8, mem, (B, Lc, T, D),
                    memory.dtype, [id(p) for p in params])
        return red[0].clone()

    @staticmethod
    def backward(ctx, gout):
        import math
        dec, prec, pk, x, xn, logits, target, lse, red, smoothing, saved, drops, d_pos, ys_in, self_mask8, mem_mask8, mem, shape, mdt, pids = ctx.args
        B, Lc, T, D = shape
        g = _lsm_row_scale(gout, target, red)
        if logits is None:
            dz = cfm.lsm_grad(xn, pk.w, pk.b, target, pk.V, smoothing, lse, g)
        else:
            dz = cfm.lsm_grad(None, None, None, target, pk.V, smoothing, lse, g, logits=logits, out_dtype=prec.act_dtype)
        grads = {}
        dW, db = cfm.gemm_tn(dz, xn, want_colsum=True, mma_code=prec.w_code, split=prec.split)
        grads[id(dec.output_layer.weight)], grads[id(dec.output_layer.bias)] = dW[:pk.V], db[:pk.V]
        dxn = _gemm(dz, pk.wt, w_lo=pk.wt_lo, out_dtype=torch.float32)
        dx, dg, dbn = cfm.layernorm_bwd(x, dxn, dec.after_norm.weight)
        grads[id(dec.after_norm.weight)], grads[id(dec.after_norm.bias)] = dg, dbn
        dmem = torch.zeros((B * T, D), dtype=torch.float32, device=dx.device)

        def put(mod, gs):
            for name, p in mod.named_parameters():
                if name in gs:
                    grads[id(p)] = gs[name]

        for l in range(len(dec.decoders) - 1, -1, -1):
            layer, (s1, s2, s3), dr = dec.decoders[l], saved[l], drops[l]
            sa, ca, ff = layer.self_attn, layer.src_attn, layer.feed_forward
            dx, gs, (dg, dbn) = ffn_bwd(packing.pack_ffn_train(ff, prec), s3, dx, (layer.norm3.weight, layer.norm3.bias), prec, 1.0, act=cfm.ACT_RELU,
                                        drop_h=dr[4], drop_o=dr[5])
            put(ff, gs)
            grads[id(layer.norm3.weight)], grads[id(layer.norm3.bias)] = dg, dbn
            dx, gs, (dg, dbn) = src_attn_bwd(ca, packing.pack_src_attn_train(ca, prec), s2, dx, (layer.norm2.weight, layer.norm2.bias), B, Lc, T, mem_mask8,
                                             prec, dmem, drop_a=dr[2], drop_o=dr[3])
            put(ca, gs)
            grads[id(layer.norm2.weight)], grads[id(layer.norm2.bias)] = dg, dbn
            dx, gs, (dg, dbn) = mhsa_bwd(sa, packing.pack_mhsa_train(sa, prec, False), s1, dx, (layer.norm1.weight, layer.norm1.bias), B, Lc, self_mask8,
                                         (Lc * Lc, Lc), prec, False, drop_a=dr[0], drop_o=dr[1])
            put(sa, gs)
            grads[id(layer.norm1.weight)], grads[id(layer.norm1.bias)] = dg, dbn
        if d_pos is not None:
            dx = cfm.dropout_rows(dx, torch.float32, drop=d_pos)
        E = dec.embed[0].weight
        dE = torch.zeros(E.shape, dtype=torch.float32, device=dx.device)
        dE.index_add_(0, ys_in.reshape(-1).long(), dx * math.sqrt(D))
        grads[id(E)] = dE
        return (dmem.view(B, T, D).to(mdt),) + (None,) * 10 + tuple(grads.get(i) for i in pids)


class LsmLogitsLossFn(torch.autograd.Function):
    """label_smoothing_loss.LabelSmoothingLoss.forward over logits the caller holds: the kernels' logits form, f32."""

    @staticmethod
    def forward(ctx, logits, target, V, smoothing, batch):
        z = _f32c(logits.reshape(-1, logits.shape[-1]))
        target = target.reshape(-1).to(torch.int32).contiguous()
        loss, lse = cfm.lsm_loss(None, None, None, target, V, smoothing, logits=z)
        red = cfm.lsm_reduce(loss, target, batch)
        ctx.args = (z, target, lse, red, V, smoothing, logits.shape, logits.dtype)
        return red[0].clone()

    @staticmethod
    def backward(ctx, gout):
        z, target, lse, red, V, smoothing, shape, dtype = ctx.args
        dz = cfm.lsm_grad(None, None, None, target, V, smoothing, lse, _lsm_row_scale(gout, target, red), logits=z)
        return dz[:, :V].to(dtype).reshape(shape), None, None, None, None


def _rnnt_scale(gout, reduction, B):
    """(host factor, device scale) of the upstream gradient for cfm.rnnt_grad: "none" -> one per utterance, "sum" -> one, "mean" -> 1 / B."""
    if reduction == "none":
        return 1.0, _f32c(gout.reshape(-1))
    return (1.0 / B if reduction == "mean" else 1.0), _f32c(gout.reshape(1))


def _rnnt_reduce(nll, reduction):
    return nll if reduction == "none" else (nll.sum() if reduction == "sum" else nll.mean())


class RNNTLossFn(torch.autograd.Function):
    """rnnt.rnnt_loss / rnnt.rnnt_loss_packed: torchaudio.functional.rnnt_loss (model.py:107) over given logits, padded [B,T,U+1,V] with
    lens = (logit_lens, target_lens), or packed [M, V] with lens = a cfm.lattice.Lattice; the gradient is a buffer of its own (the caller's
    logits are left as they are)."""

    @staticmethod
    def forward(ctx, logits, targets, lens, blank, clamp, reduction):
        if logits.dim() == 2:
            nll, st = cfm.rnnt_nll_packed(logits, targets, lens, blank)
        else:
            nll, st = cfm.rnnt_nll(logits, targets, *lens, blank)
        ctx.args = (st, clamp, reduction)
        return _rnnt_reduce(nll, reduction)

    @staticmethod
    def backward(ctx, gout):
        st, clamp, reduction = ctx.args
        logits = st.logits
        gs, gdev = _rnnt_scale(gout, reduction, st.nll.numel())
        grad = cfm.rnnt_grad(st, torch.empty(logits.shape, dtype=logits.dtype, device=logits.device), gscale=gs, gscale_dev=gdev, clamp=clamp)
        return grad, None, None, None, None, None


class JointRNNTLossFn(torch.autograd.Function):
    """TransducerJoint.rnnt_loss and TransducerJoint.forward_window: the joint (joint.py:20-38) followed by the RNN-T loss (model.py:107),
    differentiable w.r.t. the encoder rows xe2 [n_enc, E], the predictor rows xp2 [n_pred, P] and the six joint parameters.  lat: the padded
    shape (B, T, U+1, enc_lens, target_lens) -- rows b*T + t and b*(U+1) + u -- or a packed lattice (cfm.lattice.Lattice), whose activation, logits
    and loss exist for its M valid cells only (rows outside it get exact zero gradients).  The f32 logits exist only in here, and the gradient
    overwrites them in place (f32 in the accurate mode; the 16-bit type of the backward GEMMs otherwise, in the first half of each row's bytes):
    ONE logits-sized buffer."""

    @staticmethod
    def forward(ctx, xe2, xp2, mod, prec, lat, targets, blank, clamp, reduction, *params):
        pk = packing.pack_joint_train(mod, prec)
        xe2, xp2 = _f32c(xe2), _f32c(xp2)
        e = cfm.gemm(xe2, pk.enc.w, bias=pk.enc.b, w_lo=pk.enc.w_lo, out_dtype=torch.float32)
        p = cfm.gemm(xp2, pk.pred.w, bias=pk.pred.b, w_lo=pk.pred.w_lo, out_dtype=torch.float32)
        if e.shape[1] != pk.out.w.shape[1]:
            raise ValueError("TransducerJoint: join dimensions differ (%d, ffn_out expects %d)" % (e.shape[1], pk.out.w.shape[1]))
        packed = not isinstance(lat, tuple)
        if packed:
            if lat.M == 0:
                raise ValueError("TransducerJoint: no utterance has a frame (every encoder length is 0)")
            act = cfm.joint_act_packed(e, p, lat, prec.act_dtype)
        else:
            act = cfm.joint_act(e, p, *lat[:3], prec.act_dtype)
        logits = cfm.gemm(act, pk.out.w, bias=pk.out.b, w_lo=pk.out.w_lo, out_dtype=torch.float32)
        if packed:
            nll, st = cfm.rnnt_nll_packed(logits, targets, lat, blank, V=pk.V)
        else:
            B, T, U1, enc_lens, target_lens = lat
            nll, st = cfm.rnnt_nll(logits.view(B, T, U1, pk.Vp), targets, enc_lens, target_lens, blank, V=pk.V)
        ctx.args = (pk, prec, xe2, xp2, e, p, act, logits, st, lat, clamp, reduction)
        return _rnnt_reduce(nll, reduction)

    @staticmethod
    def backward(ctx, gout):
        pk, prec, xe2, xp2, e, p, act, logits, st, lat, clamp, reduction = ctx.args
        ctx.args = None
        packed = not isinstance(lat, tuple)
        gs, gdev = _rnnt_scale(gout, reduction, lat.B if packed else lat[0])
        Vp = logits.shape[1]
        if prec.split:                                           # f32 gradient over the f32 logits, same bytes
            cfm.rnnt_grad(st, logits.view(*st.rows, Vp), gscale=gs, gscale_dev=gdev, clamp=clamp)
            dlog = logits
        else:                                                    # 16-bit gradient in the first half of each f32 row
            half = logits.view(prec.w_dtype)                     # [M, 2 Vp]
            cfm.rnnt_grad(st, half.view(*st.rows, 2 * Vp), gscale=gs, gscale_dev=gdev, clamp=clamp, cols=Vp)
            dlog = half[:, :Vp]
        dWo, dbo = cfm.gemm_tn(dlog, act, want_colsum=True, mma_code=prec.w_code, split=prec.split)
        dact = _gemm(dlog, pk.out.wt, w_lo=pk.out.wt_lo, out_dtype=torch.float32)
        del logits, dlog, st
        de, dp = cfm.joint_act_packed_bwd(e, p, dact, lat) if packed else cfm.joint_act_bwd(e, p, dact, *lat[:3])
        del dact
        dWe, dbe = cfm.gemm_tn(de, xe2, want_colsum=True, mma_code=prec.w_code, split=prec.split)
        dWp, dbp = cfm.gemm_tn(dp, xp2, want_colsum=True, mma_code=prec.w_code, split=prec.split)
        dxe = _gemm(de, pk.enc.wt, w_lo=pk.enc.wt_lo, out_dtype=torch.float32)
        dxp = _gemm(dp, pk.pred.wt, w_lo=pk.pred.wt_lo, out_dtype=torch.float32)
        V = pk.V
        return (dxe, dxp, None, None, None, None, None, None, None, dWe, dbe, dWp, dbp, dWo[:V], dbo[:V])


class LSTMSeqFn(torch.autograd.Function):
    """nn.LSTM(batch_first=True) over whole sequences on cfm.lstm_forward / cfm.lstm_backward: the RNN-T predictor's teacher-forced pass
    (predictor.RNNPredictor(fused=True)).  params: weight_ih, weight_hh, bias_ih, bias_hh per layer in nn.LSTM's order (biases present iff
    has_bias); h0 / c0 [layers, B, H] or None.  p: dropout between layers (train mode; one seed per call from draw_seed unless `seed` is given) --
    the backward regenerates the mask.  Returns (y, hn, cn).  What is kept for the backward: ONE f32 block per layer."""

    @staticmethod
    def forward(ctx, x, h0, c0, H, has_bias, p, seed, *params):
        per = 4 if has_bias else 2
        weights = [tuple(_f32c(t.detach()) for t in params[i:i + per]) + ((None, None) if not has_bias else ()) for i in range(0, len(params), per)]
        drop = None
        if p and p > 0.0 and len(weights) > 1:
            drop = (float(p), (draw_seed() if seed is None else int(seed)) & 0xFFFFFFFF)
        x = _f32c(x.detach())
        y, hn, cn, saves = cfm.lstm_forward(x, weights, H, None if h0 is None else h0.detach(), None if c0 is None else c0.detach(), drop=drop)
        ctx.args = (x, weights, H, drop, saves, has_bias, h0 is not None, c0 is not None)
        return y, hn, cn

    @staticmethod
    def backward(ctx, dy, dhn, dcn):
        x, weights, H, drop, saves, has_bias, has_h0, has_c0 = ctx.args
        if dy is None:
            dy = torch.zeros(x.shape[0], x.shape[1], H, dtype=torch.float32, device=x.device)
        dx, grads, dh0, dc0 = cfm.lstm_backward(x, weights, H, saves, _f32c(dy), None if dhn is None else _f32c(dhn), None if dcn is None else _f32c(dcn), drop=drop)
        flat = [g for gw in grads for g in (gw if has_bias else gw[:2])]
        return (dx, dh0 if has_h0 else None, dc0 if has_c0 else None, None, None, None, None, *flat)
