"""GPU: encoder_layer.BlockCall, the per-call object that ConformerEncoder._run_blocks and ConformerEncoderLayer.forward fill once and every block
of the call reuses -- one weight key per block and forward, no field of one block reaching the next, weight invalidation as before, and the route
switches read at call time.

Shapes: a 3-block encoder, D = 256, FF = 2048, H = 4, kernel 15, synthetic weights; B = 2, T = 43, lens = [43, 9]: T' = 10, one item of a single
encoder frame, 20 rows."""
import copy

import pytest
import torch

import synth
from test_ops_gpu import cfm  # noqa: F401  (cfm: the module fixture)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
CFG = dict(input_dim=80, kernel_size=15, encoder_dim=256, dropout=0.1, attention_dropout=0.1, pos_enc_dropout=0.1, hidden_dim=2048, num_heads=4,
           encoder_num_layers=3, max_len=5000, use_relative=True)
B, T, LENS = 2, 43, [43, 9]
_MASTER = {}


def build(seed=11, middle_seed=None):
    """A fresh eval encoder on the device (from a CPU master built once per seed pair); middle_seed: other weights for block 1."""
    import encoder
    if (seed, middle_seed) not in _MASTER:
        enc = synth.load_synth_(encoder.ConformerEncoder(cmvn=None, **CFG).eval(), seed)
        if middle_seed is not None:
            synth.load_synth_(enc.encoders[1], middle_seed)
        _MASTER[seed, middle_seed] = enc
    return copy.deepcopy(_MASTER[seed, middle_seed]).to(DEV)


def inputs():
    return torch.from_numpy(synth.fbank(12, B, T)).to(DEV), torch.tensor(LENS, dtype=torch.int32, device=DEV)


@pytest.fixture
def bf16(cfm):
    cfm.set_precision("bf16")
    yield cfm
    cfm.set_precision("bf16")


def count_keys(monkeypatch, enc, fn):
    """(block-weight keys per block, keys of the positional pack) computed while fn() runs."""
    from cfm import packing
    real = packing.weights_key
    marks = [blk.norm_ff.weight for blk in enc.encoders]                  # in a block's tensor list and in no other pack's
    pos = [blk.self_attn.linear_pos.weight for blk in enc.encoders]       # the positional pack's tensor list, in this order
    per_block, pos_keys = [0] * len(marks), [0]

    def counting(tensors, *extra):
        tensors = list(tensors)
        for i, m in enumerate(marks):
            per_block[i] += sum(t is m for t in tensors)
        pos_keys[0] += len(tensors) == len(pos) and all(a is b for a, b in zip(tensors, pos))
        return real(tensors, *extra)

    monkeypatch.setattr(packing, "weights_key", counting)
    try:
        with torch.no_grad():
            fn()
        torch.cuda.synchronize()
    finally:
        monkeypatch.setattr(packing, "weights_key", real)
    return per_block, pos_keys[0]


def test_forward_computes_one_weight_key_per_block(bf16, monkeypatch):
    enc = build()
    x, lens = inputs()
    for _ in range(2):                                                    # packing the weights, then a cache hit: once per block either way
        assert count_keys(monkeypatch, enc, lambda: enc(x, lens)) == ([1, 1, 1], 1)


def test_streaming_step_computes_one_weight_key_per_block(bf16, monkeypatch):
    import encoder
    enc = build()
    sb = encoder.StreamingBatch(enc, 2, 4, 2, graph=False)
    frames = torch.from_numpy(synth.fbank(13, 2, sb.window)).to(DEV)
    for _ in range(2):
        assert count_keys(monkeypatch, enc, lambda: sb.step(frames)) == ([1, 1, 1], 1)


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_no_field_of_one_block_reaches_the_next(cfm, monkeypatch, mode):
    """A forward_chunk step that takes and returns caches, CHAIN_BLOCKS off, the middle block with weights of its own, against the three blocks
    called one after the other through ConformerEncoderLayer.forward (a BlockCall each), each with its own cache, then cfm.layernorm: bit for bit.
    At D = 256 after_norm rides in the last block's final chain, which a separate LayerNorm need not match to the bit, so the encoder is made to
    take the separate one: in fp32 mode (no row chains) it does by itself, in bf16 through an after_norm.eps of 2e-5, which the fused form
    does not carry.  SPLIT_FFN_FEW_ROWS is off as well: only a streaming entry point asks for the split feed-forward, the single block never does."""
    import encoder_layer
    monkeypatch.setattr(encoder_layer, "CHAIN_BLOCKS", False)
    monkeypatch.setattr(encoder_layer, "SPLIT_FFN_FEW_ROWS", False)
    cfm.set_precision(mode)
    try:
        enc = build(middle_seed=77)
        enc.after_norm.eps = 2e-5
        x = torch.from_numpy(synth.fbank(14, 1, 62)).to(DEV)
        empty = torch.zeros((0, 0, 0, 0), device=DEV)
        with torch.no_grad():
            y1, c1, _ = enc.forward_chunk(x[:, :43].contiguous(), 0, -1, empty, empty)
            n1 = y1.size(1)
            y2, c2, _ = enc.forward_chunk(x[:, 40:62].contiguous(), n1, -1, c1, empty)
            # the same second step, block by block
            h = enc.embed.embed_frames(x[:, 40:62].contiguous(), None)
            h, _ = enc.position_encoding(h, n1)
            pos = enc.embed.position_encoding(offset=0, size=n1 + h.size(1)).to(DEV)
            caches = []
            for i, blk in enumerate(enc.encoders):
                h, _, c, _ = blk(h, torch.ones((0, 0, 0)), pos, attn_cache=c1[i:i + 1])
                caches.append(c)
            y, _ = cfm.layernorm(h.reshape(-1, 256), enc.after_norm.weight.detach(), enc.after_norm.bias.detach(), eps=enc.after_norm.eps)
        assert c2.shape == (3, 4, n1 + y2.size(1), 128) and y2.size(1) == 4
        assert torch.equal(torch.cat(caches, 0), c2)
        assert torch.equal(y.view_as(y2), y2)
        assert not torch.equal(c2[0], c2[1])
    finally:
        cfm.set_precision("bf16")


def test_replaced_parameter_invalidates_the_block_weights(bf16):
    enc = build()
    x, lens = inputs()
    with torch.no_grad():
        y0, _ = enc(x, lens)
        new = torch.from_numpy(synth.normal(15, (256,), 0.5) + 1.0).to(DEV)
        enc.encoders[1].norm_ff.weight = torch.nn.Parameter(new.clone())
        y1, _ = enc(x, lens)
        fresh = build()
        fresh.encoders[1].norm_ff.weight.copy_(new)
        y2, _ = fresh(x, lens)
    assert not torch.equal(y1, y0)
    assert torch.equal(y1, y2)


def test_chain_blocks_is_read_on_every_call(bf16, monkeypatch):
    import encoder_layer
    enc = build()
    x, lens = inputs()

    def launches():
        bf16.prof_reset(); bf16.prof_enable(True)
        try:
            with torch.no_grad():
                enc(x, lens)
            torch.cuda.synchronize()
        finally:
            bf16.prof_enable(False)
        return {k: v["calls"] for k, v in bf16.prof_table().items()}

    launches()                                                            # packs the weights
    chained = launches()
    monkeypatch.setattr(encoder_layer, "CHAIN_BLOCKS", False)
    unchained = launches()
    monkeypatch.setattr(encoder_layer, "CHAIN_BLOCKS", True)
    assert unchained != chained and sum(unchained.values()) > sum(chained.values())
    assert launches() == chained
