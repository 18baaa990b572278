"""CPU guards for the one key every module cache is built for (cfm.packing.weights_key) and for each consumer of it: every way a weight can
change -- in place, its storage moved, the Parameter object replaced, a raw-pointer update (the pack epoch), another precision, another
dtype -- must rebuild what was derived from it exactly once, and nothing else may.  No GPU: the builders are counted, not run."""
import types

import pytest
import torch
import torch.nn as nn

import cfm
from cfm import packing
from test_module_caches_cpu import CFG, build_objective

BF16, FP16 = cfm.Precision("bf16"), cfm.Precision("fp16")


def events(mod, name):
    """[(what, do)]: the ways parameter `name` of `mod` changes without the caller being told (another precision is the caller's to pass)."""
    def inplace():
        with torch.no_grad():
            getattr(mod, name).add_(1.0)

    def moved():
        p = getattr(mod, name)
        p.data = p.data.clone()

    def replaced():
        setattr(mod, name, nn.Parameter(getattr(mod, name).detach().clone()))

    def double():
        setattr(mod, name, nn.Parameter(getattr(mod, name).detach().double()))
    return [("add_ in place", inplace), ("p.data = clone", moved), ("Parameter replaced", replaced), ("bump_epoch", packing.bump_epoch), (".double()", double)]


def test_weights_key_sees_every_change():
    a, b = nn.Linear(8, 8), nn.Linear(8, 8)
    key = lambda *extra: packing.weights_key([a.weight, a.bias, None, b.weight, None, b.bias], *extra)
    k = key("bf16")
    assert k == key("bf16")
    assert len(k) == 2 + 4 and k[1] == "bf16"                                       # epoch, extra, then one entry per tensor: None is skipped
    assert k[2] == (a.weight.data_ptr(), a.weight._version, "cpu", torch.float32)
    assert key("fp16") != k and key() != k and key()[1:] == k[2:]
    for what, do in events(b, "weight"):
        k0 = key("bf16")
        do()
        assert key("bf16") != k0, what
        assert key("bf16") == key("bf16"), what
    t = torch.zeros(4)
    k32, ki = packing.weights_key([t]), packing.weights_key([t.view(torch.int32)])  # the same bytes read as another dtype: only the dtype differs
    assert k32 != ki and k32[1][:3] == ki[1][:3]


def test_layer_weight_struct_is_rebuilt_once_per_change(monkeypatch):
    import encoder_layer
    layer = encoder_layer.ConformerEncoderLayer(64, 15, 0.0, 0.0, 136, 4, True)
    built = []
    monkeypatch.setattr(packing, "layer_weight_struct", lambda l, prec: (built.append(prec.name) or len(built), ()))
    assert layer._weights(BF16) == 1 and layer._weights(BF16) == 1
    for mod, name in ((layer.norm_ff, "weight"), (layer.feed_forward.w_1, "bias"), (layer.conv_module.pointwise_conv2, "weight")):
        for what, do in events(mod, name):
            n = len(built)
            do()
            assert layer._weights(BF16) == n + 1 and layer._weights(BF16) == n + 1, (name, what)
    with torch.no_grad():
        layer.conv_module.norm.running_var.mul_(2.0)                                # a buffer counts as well
    n = len(built)
    assert layer._weights(BF16) == n + 1 and layer._weights(FP16) == n + 2 and layer._weights(FP16) == n + 2
    assert built[-2:] == ["bf16", "fp16"]


def test_greedy_head_packs_are_rebuilt_once_per_change():
    import greedy
    obj = build_objective()
    head = greedy._Head(obj.predictor.eval(), obj.joint.eval())
    cpu = torch.device("cpu")
    W = head.packs(cpu)
    assert head.packs(cpu) is W and "ef_w" not in W
    assert head.packs(cpu, enc_ffn=True) is W and "ef_w" in W and "ef_b" in W       # added on request, to the same packs
    for mod, name in ((obj.predictor.embed, "weight"), (obj.joint.ffn_out, "bias"), (obj.joint.enc_ffn, "weight")):
        for what, do in events(mod, name):
            k0 = head.weights_key()
            do()
            assert head.weights_key() != k0, (name, what)
            W2 = head.packs(cpu)
            assert W2 is not W and head.packs(cpu) is W2 and "ef_w" not in W2, (name, what)
            assert torch.equal(W2["embed"], obj.predictor.embed.weight.detach().float()), (name, what)
            W = W2


@pytest.fixture
def stub_plan(monkeypatch):
    class Plan:
        built, runs = 0, 0

        def __init__(self, layers, prec, relative):
            Plan.built += 1

        def valid_for(self, layers, prec):
            return True

        def run(self):
            Plan.runs += 1
            return ("packs",)
    monkeypatch.setattr(packing, "_StackPackPlan", Plan)
    return Plan


def small_encoder():
    import encoder
    return encoder.ConformerEncoder(cmvn=None, **CFG)


def test_stack_packs_walk_path_runs_the_plan_once_per_change(stub_plan):
    enc = small_encoder()
    layers = list(enc.encoders)
    get = lambda prec=BF16: packing.pack_stack_train(enc, layers, prec, True)
    assert get() == ("packs",) and get() == ("packs",) and (stub_plan.built, stub_plan.runs) == (1, 1)
    for mod, name in ((layers[0].feed_forward.w_1, "weight"), (layers[1].self_attn.linear_q, "bias")):
        for what, do in events(mod, name):
            n = stub_plan.runs
            do()
            get(), get()
            assert (stub_plan.built, stub_plan.runs) == (1, n + 1), (name, what)
    n = stub_plan.runs
    get(FP16), get(FP16)
    assert (stub_plan.built, stub_plan.runs) == (1, n + 1)                          # the plan outlives a key miss while it is valid_for
    with torch.no_grad():
        layers[0].norm_ff.weight.add_(1.0)                                          # the struct reads the LayerNorms in place: no pack of them
    get(FP16)
    assert stub_plan.runs == n + 1


def test_stack_packs_flat_path_follows_the_epoch_only(stub_plan):
    enc = small_encoder()
    layers = list(enc.encoders)
    get = lambda: packing.pack_stack_train(enc, layers, BF16, True, flat=True)
    get(), get()
    assert (stub_plan.built, stub_plan.runs) == (1, 1)
    with torch.no_grad():
        layers[0].feed_forward.w_1.weight.add_(1.0)                                 # the flat trainer's weights change through its step alone,
    get()                                                                           # which bumps the epoch: no per-tensor walk here
    assert (stub_plan.built, stub_plan.runs) == (1, 1)
    packing.bump_epoch()
    get(), get()
    assert (stub_plan.built, stub_plan.runs) == (1, 2)


def test_graph_watch_sees_in_place_updates_and_the_epoch():
    owner = types.SimpleNamespace(enc=small_encoder())
    sig = packing.graph_watch(owner)
    assert packing.graph_watch(owner) == sig
    tensors = list(owner.enc.parameters()) + list(owner.enc.buffers())
    assert any(t.dtype == torch.int64 for t in tensors) and len(tensors) > 2 * 36   # the BatchNorm counters too; two blocks and the rest
    for t in tensors:
        with torch.no_grad():
            t.add_(1)
        new = packing.graph_watch(owner)
        assert new != sig and packing.graph_watch(owner) == new
        sig = new
    packing.bump_epoch()
    assert packing.graph_watch(owner) != sig
