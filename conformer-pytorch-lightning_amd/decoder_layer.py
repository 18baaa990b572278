"""Transformer decoder layer of the attention decoder -- drop-in for the class of the same name in the reference's src/decoder_layer.py
(constructor arguments, submodule and parameter names: self_attn, src_attn, feed_forward, norm1..3), eval mode only.

The reference's forward cannot be reproduced: decoder_layer.py:51 adds `dropout(self_attn(...))` to a tensor while the attention module returns a
tuple, so the class raises on its first call.  What runs here is the evident intent, the pre-norm layer stated in tests/attention_decoder_ref.py:

    x += SelfAttn(LN1(x));   x += SrcAttn(LN2(x), memory, memory);   x += FFN_relu(LN3(x))

as cfm kernels on row matrices: cfm.layernorm, the fused q|k|v projection, cfm.attention, and the output projections and the feed-forward's second
product with the residual in the GEMM epilogue (the stream x stays float32).  `layer_rows` is the one implementation; it takes the self-attention
and the cross-attention batch shapes separately, because a rescoring pass runs self-attention over P = B*N hypotheses of Lc positions and
cross-attention as B utterances of N*Lc queries -- so the memory's keys and values are projected once per utterance and layer, not once per
hypothesis.  These entry points are eval-only and raise in train mode; the decoder is trained through decoder.AttentionLoss
(cfm.autograd.DecoderLossFn), which runs the same layer with its backward."""
import torch
import torch.nn as nn

import cfm
from attention import MultiHeadSelfAttentionModule
from cfm import packing
from feedforward import PositionwiseFeedForwardModule


def _no_training(module):
    if module.training:
        raise NotImplementedError("%s: eval mode only -- training the attention decoder needs the cross-attention backward "
                                  "(and the label-smoothing loss), which do not exist; call .eval()" % type(module).__name__)


def layer_rows(layer, x, self_shape, self_mask, memory_rows, src_shape, memory_mask, prec):
    """One decoder layer on the f32 row matrix x [R, D], in place.  self_shape = (batch, T): the rows as `batch` sequences of T for self-attention,
    self_mask uint8 [batch, T, T]; src_shape = (batch, Tq, Tk): the same rows as `batch` groups of Tq queries over memory_rows [batch * Tk, D]
    (f32), memory_mask uint8 [batch, 1, Tk]."""
    D = x.shape[1]
    sa, ca, ff = layer.self_attn, layer.src_attn, layer.feed_forward
    H, dk, adt = sa.num_heads, sa.d_k, prec.act_dtype
    pk = packing.pack_mhsa(sa, prec, False)
    Bs, Ts = self_shape
    xn, _ = cfm.layernorm(x, layer.norm1.weight, layer.norm1.bias, out1_dtype=adt)
    qkv = cfm.gemm(xn, pk.qkv_w, bias=pk.qkv_b, w_lo=pk.qkv_w_lo, out_dtype=adt)
    ctx = torch.empty_like(xn)
    cfm.attention(qkv, qkv[:, D:], qkv[:, 2 * D:], Bs, H, Ts, Ts, dk, (Ts * 3 * D, 3 * D), (Ts * 3 * D, 3 * D, dk), (Ts * 3 * D, 3 * D, dk), ctx,
                  mask=self_mask, mask_str=(Ts * Ts, Ts), mma_code=prec.w_code, split=prec.split)
    cfm.gemm(ctx, pk.out_w, bias=pk.out_b, w_lo=pk.out_w_lo, residual=x, out=x)

    pk = packing.pack_mhsa(ca, prec, False)
    Bc, Tq, Tk = src_shape
    xn, _ = cfm.layernorm(x, layer.norm2.weight, layer.norm2.bias, out1_dtype=adt)
    q = cfm.gemm(xn, pk.q_w, bias=pk.q_b, w_lo=pk.q_w_lo, out_dtype=adt)
    kv = cfm.gemm(memory_rows, pk.qkv_w[D:], bias=pk.qkv_b[D:], w_lo=None if pk.qkv_w_lo is None else pk.qkv_w_lo[D:], out_dtype=adt)     # k | v in one product
    cfm.attention(q, kv, kv[:, D:], Bc, H, Tq, Tk, dk, (Tq * D, D), (Tk * 2 * D, 2 * D, dk), (Tk * 2 * D, 2 * D, dk), ctx,
                  mask=memory_mask, mask_str=(Tk, 0), mma_code=prec.w_code, split=prec.split)
    cfm.gemm(ctx, pk.out_w, bias=pk.out_b, w_lo=pk.out_w_lo, residual=x, out=x)

    pf = packing.pack_ffn(ff, prec)
    xn, _ = cfm.layernorm(x, layer.norm3.weight, layer.norm3.bias, out1_dtype=adt)
    hid = cfm.gemm(xn, pf.w1, bias=pf.b1, w_lo=pf.w1_lo, act=cfm.ACT_RELU, out_dtype=adt)
    cfm.gemm(hid, pf.w2, bias=pf.b2, w_lo=pf.w2_lo, residual=x, out=x)
    return x


class TransformerDecoderLayer(nn.Module):

    def __init__(self, decoder_dim, num_heads, hidden_dim, dropout, self_attention_dropout, src_attention_dropout):
        super().__init__()
        self.self_attn = MultiHeadSelfAttentionModule(encoder_dim=decoder_dim, num_heads=num_heads, dropout=self_attention_dropout)
        self.src_attn = MultiHeadSelfAttentionModule(encoder_dim=decoder_dim, num_heads=num_heads, dropout=src_attention_dropout)
        self.feed_forward = PositionwiseFeedForwardModule(input_dim=decoder_dim, hidden_dim=hidden_dim, dropout=dropout, activation='relu')
        self.norm1 = nn.LayerNorm(decoder_dim, eps=1e-5)
        self.norm2 = nn.LayerNorm(decoder_dim, eps=1e-5)
        self.norm3 = nn.LayerNorm(decoder_dim, eps=1e-5)
        self.dropout = nn.Dropout(dropout)
        self.self_attn.return_cache = self.src_attn.return_cache = False       # no KV cache is kept: no cfm_kv_cache_pack launch

    def forward(self, tgt, tgt_mask, memory, memory_mask, cache=None):
        """tgt [B, L, D], tgt_mask [B, L, L], memory [B, T, D], memory_mask [B, 1, T] -> (outputs, tgt_mask, memory, memory_mask), the reference's
        return values.  The incremental form (cache) is not built."""
        _no_training(self)
        if cache is not None:
            raise NotImplementedError("TransformerDecoderLayer: incremental decoding (cache) is not built; rescoring scores whole hypotheses")
        cfm.require_hip(tgt, memory)
        B, L, D = tgt.shape
        T = memory.shape[1]
        x = tgt.detach().to(torch.float32).reshape(B * L, D).clone()
        mem = memory.detach().to(torch.float32).reshape(B * T, D).contiguous()
        with torch.no_grad():
            layer_rows(self, x, (B, L), cfm.as_u8_mask(tgt_mask.expand(B, L, L)), mem, (B, L, T), cfm.as_u8_mask(memory_mask.expand(B, 1, T)),
                       cfm.resolve_precision(self))
        return x.view(B, L, D).to(tgt.dtype), tgt_mask, memory, memory_mask
