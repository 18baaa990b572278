"""CPU guards for the caches the HIP paths keep on modules (no GPU: the caches are planted by hand, shaped like what a forward leaves).

* copy.deepcopy and pickle (torch.save) of a module holding them must succeed and give a copy WITHOUT them: the ctypes weight structs hold
  raw device pointers (unpicklable, and a copied pointer would address the original's memory), the packs belong to the original's tensors.
* the train-mode weight structs (cfm/autograd.py _stack_weights, cached in the owner's _stack_w) must be rebuilt when a LayerNorm parameter or
  a BatchNorm running buffer is replaced by a new tensor, although the weight packs they are keyed on stay the same objects.
* train mode refuses, up front, a block parameter the kernels cannot read through a raw f32 pointer."""
import copy
import io
import pickle

import pytest
import torch

import cfm
import synth
from cfm import autograd as ag
from cfm import packing

CFG = dict(input_dim=80, kernel_size=15, encoder_dim=64, dropout=0.0, attention_dropout=0.0, pos_enc_dropout=0.0, hidden_dim=136, num_heads=4,
           encoder_num_layers=2, max_len=5000, use_relative=True)


def build_objective():
    import decoder
    import encoder
    import joint
    import predictor
    import transducer
    enc = synth.load_synth_(encoder.ConformerEncoder(cmvn=None, **CFG), 5)
    ctc = synth.load_synth_(decoder.CTCDecoder(37, 64, 0.0), 6)
    torch.manual_seed(7)
    pr = predictor.RNNPredictor(37, 16, 24, 32, 0.0, 1, dropout=0.0)
    jn = joint.TransducerJoint(37, 64, 24, 48)
    return transducer.TransducerObjective(enc, pr, jn, ctc, ctc_weight=0.2, transducer_weight=0.8)


def pointer_struct():
    w = cfm.LayerTrainWeights()
    w.ln_ff_g, w.qkv_w = 0x7F0000001000, 0x7F0000002000
    return w


# every name the package caches under on a module: each holds a packing.Slot, planted through packing.slot as the code itself fetches it
CACHE_NAMES = ("_fused", "_stack_w", "_stack_g", "_pack_stack_train", "_grad_layout", "_pos_pack", "_pack_train", "_pack")
KEY = ("bf16", 0)


def fill(mod, name, value, cls=packing.Slot):
    packing.Slot.get(packing.slot(mod, name, cls), KEY, lambda: value)


def plant(obj):
    """What an eval forward and a train step leave behind, with pointer-bearing ctypes structs where the real ones sit: a slot type that
    did not empty itself on a copy would make deepcopy / pickle raise on them."""
    enc = obj.encoder
    pks = tuple(packing.Packed(w=torch.zeros(4)) for _ in range(4))
    L = len(enc.encoders)
    for owner, n in [(layer, 1) for layer in enc.encoders] + [(enc, L)]:      # a block run on its own (EncoderLayerFn) is its own owner
        fill(owner, "_stack_w", ((cfm.LayerTrainWeights * n)(pointer_struct()), (pks,) * n))
        fill(owner, "_stack_g", ((cfm.LayerTrainGrads * n)(), [dict(numel=4)] * n))
        fill(owner, "_pack_stack_train", (object(), (pks,) * n, pointer_struct()))
    for layer in enc.encoders:
        fill(layer, "_fused", (pointer_struct(), (torch.zeros(3),)))
        fill(layer, "_grad_layout", {None: dict(numel=4, table=pointer_struct())})
    for m in obj.modules():                                  # every slot the modules construct (eval packs), and a training pack beside each
        for v in list(m.__dict__.values()):
            if isinstance(v, packing.Slot):
                packing.Slot.get(v, KEY, pointer_struct)
        if hasattr(m, "weight") and isinstance(getattr(m, "weight"), torch.Tensor):
            fill(m, "_pack_train", pointer_struct(), packing.PackCache)
    fill(enc, "_pos_pack", pointer_struct(), packing.PackCache)


def slots_of(root):
    return [(type(m).__name__, k, v) for m in root.modules() for k, v in m.__dict__.items() if isinstance(v, packing.Slot)]


def assert_clean(orig, cp):
    for m in cp.modules():
        for k in CACHE_NAMES:
            v = m.__dict__.get(k)
            assert v is None or (isinstance(v, packing.Slot) and v.key is None and v.value is None), (type(m).__name__, k)
    for owner, k, v in slots_of(cp):
        assert v.key is None and v.value is None, (owner, k)
    assert {k for _, k, _ in slots_of(orig)} <= set(CACHE_NAMES)
    assert all(v.key == KEY and v.value is not None for _, _, v in slots_of(orig))     # the original keeps what was planted
    so, sc = orig.state_dict(), cp.state_dict()
    assert so.keys() == sc.keys()
    for k in so:
        assert torch.equal(so[k], sc[k]), k
        assert so[k].data_ptr() != sc[k].data_ptr(), k          # a copy, not a view of the original


def test_planted_structs_are_what_blocks_pickling():
    with pytest.raises(ValueError):
        pickle.dumps(pointer_struct())


@pytest.mark.parametrize("part", ["objective", "encoder", "ctc", "layer"])
def test_deepcopy_and_pickle_drop_pointer_caches(part):
    obj = build_objective()
    plant(obj)
    assert {k for _, k, _ in slots_of(obj)} == set(CACHE_NAMES)             # plant() reaches every kind of slot the code has
    mod ={"objective": obj, "encoder": obj.encoder, "ctc": obj.ctc, "layer": obj.encoder.encoders[1]}[part]
    cp = copy.deepcopy(mod)
    assert_clean(mod, cp)
    buf = io.BytesIO()
    torch.save(mod, buf)
    buf.seek(0)
    assert_clean(mod, torch.load(buf, weights_only=False))
    # the original keeps its caches: copying does not disturb the model being trained
    layer = obj.encoder.encoders[0]
    assert all(packing.slot(m, k).value is not None for m, k in ((layer, "_fused"), (layer, "_stack_w"), (obj.encoder, "_stack_w")))


def fake_packs():
    """(macaron FFN, attention, conv module, FFN) packs with every field _build_train_weights_struct reads, as CPU tensors."""
    t = lambda: torch.zeros(4)
    ffn = lambda: packing.Packed(**{f: t() for f in ("w1", "w1_lo", "w2", "w2_lo", "w1t", "w1t_lo", "w2t", "w2t_lo", "b1", "b2")})
    att = packing.Packed(**{f: t() for f in ("qkv_w", "qkv_w_lo", "qkv_t", "qkv_t_lo", "out_w", "out_w_lo", "out_t", "out_t_lo", "qkv_b", "out_b")})
    cv = packing.Packed(**{f: t() for f in ("pw1_w", "pw1_w_lo", "pw1_t", "pw1_t_lo", "pw2_w", "pw2_w_lo", "pw2_t", "pw2_t_lo", "pw1_b", "pw2_b",
                                            "dw_w", "dw_b", "gamma", "beta")})
    return ffn(), att, cv, ffn()


def test_train_weight_struct_follows_replaced_norm_tensors(monkeypatch):
    """One block on its own (EncoderLayerFn: the block is its own owner)."""
    import encoder_layer
    layer = encoder_layer.ConformerEncoderLayer(64, 15, 0.0, 0.0, 136, 4, True)
    pks = (fake_packs(),)
    monkeypatch.setattr(packing, "pack_stack_train", lambda owner, ls, prec, rel, flat=False: pks)
    prec = cfm.Precision("bf16")
    w = ag._stack_weights(layer, [layer], prec, False)[0]
    assert ag._stack_weights(layer, [layer], prec, False)[0] is w is packing.slot(layer, "_stack_w").value[0]     # nothing replaced: the cached array
    assert w[0].ln_ff_g == layer.norm_ff.weight.data_ptr()
    layer.norm_ff.weight = torch.nn.Parameter(torch.full((64,), 2.0))
    w2 = ag._stack_weights(layer, [layer], prec, False)[0]
    assert w2 is not w and w2[0].ln_ff_g == layer.norm_ff.weight.data_ptr()
    bn = layer.conv_module.norm
    bn.running_mean, bn.running_var = torch.ones(64), torch.full((64,), 3.0)
    w3 = ag._stack_weights(layer, [layer], prec, False)[0]
    assert w3 is not w2
    assert (w3[0].bn_running_mean, w3[0].bn_running_var) == (bn.running_mean.data_ptr(), bn.running_var.data_ptr())
    with torch.no_grad():
        layer.norm_mha.bias.add_(1.0)                                        # an in-place update keeps the address: still a hit
    assert ag._stack_weights(layer, [layer], prec, False)[0] is w3
    bn.momentum = None                                                       # cumulative moving average: refreshed on every hit
    bn.num_batches_tracked.fill_(3)
    assert ag._stack_weights(layer, [layer], prec, False)[0] is w3 and w3[0].bn_momentum == 0.25


def test_stack_weight_array_follows_replaced_norm_tensors(monkeypatch):
    import encoder
    enc = encoder.ConformerEncoder(cmvn=None, **CFG)
    layers = list(enc.encoders)
    pks = tuple(fake_packs() for _ in layers)
    monkeypatch.setattr(packing, "pack_stack_train", lambda owner, ls, prec, rel, flat=False: pks)
    prec = cfm.Precision("bf16")
    arr, _ = ag._stack_weights(enc, layers, prec, False)
    assert ag._stack_weights(enc, layers, prec, False)[0] is arr
    layers[1].norm_final.bias = torch.nn.Parameter(torch.zeros(64))
    arr2, _ = ag._stack_weights(enc, layers, prec, False)
    assert arr2 is not arr and arr2[1].ln_final_b == layers[1].norm_final.bias.data_ptr()
    layers[0].conv_module.norm.running_var = torch.ones(64)
    arr3, _ = ag._stack_weights(enc, layers, prec, False)
    assert arr3 is not arr2 and arr3[0].bn_running_var == layers[0].conv_module.norm.running_var.data_ptr()


@pytest.mark.parametrize("form", ["float64", "strided"])
def test_train_mode_refuses_non_f32_or_strided_parameters(form):
    """The weight structs read LayerNorm parameters, and the packs the conv module's vectors, through raw f32 pointers: a float64 or
    non-contiguous block parameter is a TypeError naming it, before anything runs."""
    import encoder
    import encoder_layer
    layer = encoder_layer.ConformerEncoderLayer(64, 15, 0.0, 0.0, 136, 4, True).train()
    if form == "float64":
        layer.norm_mha.weight = torch.nn.Parameter(layer.norm_mha.weight.detach().double())
        name = "norm_mha.weight"
    else:
        layer.conv_module.depthwise_conv.bias = torch.nn.Parameter(torch.zeros(64, 2)[:, 0])
        name = "conv_module.depthwise_conv.bias"
    x = torch.zeros(2, 7, 64)
    with pytest.raises(TypeError, match=name.replace(".", r"\.")):
        ag.EncoderLayerFn.apply(x, layer, cfm.Precision("bf16"), None, (0, 0), None, *layer.parameters())
    enc = encoder.ConformerEncoder(cmvn=None, **CFG).train()
    enc.encoders[1] = layer
    with pytest.raises(TypeError, match=name.replace(".", r"\.")):
        enc.forward_window([(torch.zeros(2, 40, 80), torch.tensor([40, 33]))])
