"""One conformer block in train mode composed op by op from the cfm.autograd sub-block helpers (ffn_fwd / mhsa_fwd / conv_module_fwd and
their backward), one C-ABI call per kernel, the packs from the per-module torch-op builders.  It is the readable specification of what
csrc/train_layer.cpp enqueues from C++ for cfm.autograd.EncoderLayerFn: the same launches in the same order, the same eight dropout sites with
the same seed offsets -- so the tests compare the two bit for bit."""
import cfm
import torch
from cfm import autograd as ag
from cfm import packing


class OpByOpLayerFn(torch.autograd.Function):
    """encoder_layer.py:49-71 under module.train(): four residual sub-blocks + norm_final, one autograd node."""

    @staticmethod
    def forward(ctx, x, layer, prec, mask8, m_str, keep, *params):
        B, T, D = x.shape
        rel = layer.use_relative
        pks = (packing.pack_ffn_train(layer.feed_forward_macaron, prec), packing.pack_mhsa_train(layer.self_attn, prec, rel),
               packing.pack_conv_module_train(layer.conv_module, prec), packing.pack_ffn_train(layer.feed_forward, prec))
        ln = lambda m: (m.weight.detach(), m.bias.detach())
        x0 = ag._f32c(x.reshape(B * T, D))
        # dropout (encoder_layer.py:56-69 under module.train()): the shared nn.Dropout(feedforward_dropout) on each of the four branch
        # outputs, each FFN's own dropout on its hidden activation, the attention's on its probabilities (and, plain MHSA only, on its output)
        p_br, p_a = layer.dropout.p, layer.self_attn.dropout.p
        p_hm, p_h = layer.feed_forward_macaron.dropout.p, layer.feed_forward.dropout.p
        seed = ag.draw_seed() if max(p_br, p_a, p_hm, p_h) > 0 else 0
        dr = dict(hm=ag._drop(p_hm, seed, 1), om=ag._drop(p_br, seed, 2), a=ag._drop(p_a, seed, 3), oa=ag._drop(p_br, seed, 4),
                  oa2=None if rel else ag._drop(p_a, seed, 5), oc=ag._drop(p_br, seed, 6), h=ag._drop(p_h, seed, 7), o=ag._drop(p_br, seed, 8))
        x1, s1 = ag.ffn_fwd(pks[0], x0, ln(layer.norm_ff_macaron), prec, 0.5, drop_h=dr["hm"], drop_o=dr["om"])
        x2, s2 = ag.mhsa_fwd(layer.self_attn, pks[1], x1, ln(layer.norm_mha), B, T, mask8, m_str, prec, rel, dr["a"], dr["oa"], dr["oa2"])
        x3, s3 = ag.conv_module_fwd(layer.conv_module, pks[2], x2, ln(layer.norm_conv), B, T, keep, prec, drop_o=dr["oc"])
        x4, s4 = ag.ffn_fwd(pks[3], x3, ln(layer.norm_ff), prec, 0.5, drop_h=dr["h"], drop_o=dr["o"])
        y = cfm.layernorm(x4, *ln(layer.norm_final))[0]
        ctx.args = (layer, prec, mask8, m_str, keep, pks, (s1, s2, s3, s4, x4), B, T, D, dr)
        return y.view(B, T, D)

    @staticmethod
    def backward(ctx, dy):
        layer, prec, mask8, m_str, keep, pks, (s1, s2, s3, s4, x4), B, T, D, dr = ctx.args
        rel = layer.use_relative
        ln = lambda m: (m.weight.detach(), m.bias.detach())
        grads = {}

        def put(prefix, g, norm_name, lng):
            for k, v in g.items():
                grads[prefix + k] = v
            grads[norm_name + ".weight"], grads[norm_name + ".bias"] = lng

        d, dgf, dbf = cfm.layernorm_bwd(x4, ag._f32c(dy.reshape(B * T, D)), layer.norm_final.weight.detach())
        grads["norm_final.weight"], grads["norm_final.bias"] = dgf, dbf
        d, g, lng = ag.ffn_bwd(pks[3], s4, d, ln(layer.norm_ff), prec, 0.5, drop_h=dr["h"], drop_o=dr["o"])
        put("feed_forward.", g, "norm_ff", lng)
        d, g, lng = ag.conv_module_bwd(layer.conv_module, pks[2], s3, d, ln(layer.norm_conv), B, T, keep, prec, drop_o=dr["oc"])
        put("conv_module.", g, "norm_conv", lng)
        d, g, lng = ag.mhsa_bwd(layer.self_attn, pks[1], s2, d, ln(layer.norm_mha), B, T, mask8, m_str, prec, rel, dr["a"], dr["oa"], dr["oa2"])
        put("self_attn.", g, "norm_mha", lng)
        d, g, lng = ag.ffn_bwd(pks[0], s1, d, ln(layer.norm_ff_macaron), prec, 0.5, drop_h=dr["hm"], drop_o=dr["om"])
        put("feed_forward_macaron.", g, "norm_ff_macaron", lng)
        names, tensors = ag._params(layer)
        return (d.view(B, T, D), None, None, None, None, None) + tuple(ag._ordered(names, grads, tensors))


def block_train_forward(layer, inputs, attn_mask, pad_mask):
    """ConformerEncoderLayer.train_forward with OpByOpLayerFn in place of cfm.autograd.EncoderLayerFn."""
    from encoder_layer import _mask_args
    B, T, _ = inputs.shape
    m8, m_str = _mask_args(attn_mask, B, T, T)
    keep = None
    if pad_mask is not None and pad_mask.dim() >= 3 and pad_mask.size(2) > 0:
        keep = cfm.as_u8_mask(pad_mask).reshape(-1)
    return OpByOpLayerFn.apply(inputs, layer, cfm.resolve_precision(layer), m8, m_str, keep, *layer.parameters())
