"""One line per case, `case-name sha256`: the bytes of every output (y, the mask, returned caches, ring and conv state after the last step) of small
ragged encoder runs that between them take every route of cfm_encoder_layer_forward (include/cfm.h cfm_route).  Run on two builds of the library, the
listings must be identical line for line: a change of csrc/encoder.cpp that only reorganises the launch lists changes no bit
(profiles/r07_layer_routes.txt).  Weights and inputs are the seeded generators of tests/synth.py; row counts are no multiple of 32 and one utterance
has 9 frames -- a single encoder frame, shorter than the depthwise halo."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "conformer-pytorch-lightning_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import cfm
import encoder
import encoder_layer
import synth

DEV = torch.device("cuda", 0)
CFG = dict(input_dim=80, kernel_size=15, encoder_dim=256, dropout=0.1, attention_dropout=0.1, pos_enc_dropout=0.1, hidden_dim=2048, num_heads=4,
           encoder_num_layers=3, max_len=5000, use_relative=True)
CFG512 = CFG | dict(encoder_dim=512, num_heads=8, encoder_num_layers=2)
CFG144 = CFG | dict(encoder_dim=144, hidden_dim=576, encoder_num_layers=2)
CHAIN_ONLY_PACKS = ("ffm_w2n", "ff_w2n", "qkv_wf", "out_wf", "pw1_wf", "pw2_wf")       # the chain packs cfm_ffn_fused does not read
FFN_PACKS = ("ffm_w1f", "ffm_w2f", "ff_w1f", "ff_w2f")


def digest(name, *tensors):
    h = hashlib.sha256()
    for t in tensors:
        t = t.detach().contiguous().cpu()
        h.update(("%s %s|" % (t.dtype, tuple(t.shape))).encode())
        h.update(t.view(torch.uint8).numpy().tobytes() if t.numel() else b"")
    print("%s %s" % (name, h.hexdigest()), flush=True)


def build(cfg, seed):
    enc = encoder.ConformerEncoder(cmvn=None, **cfg).eval()
    synth.load_synth_(enc, seed)
    return enc.to(DEV)


def withhold(enc, packs):
    """Null the packs on the cached weight structs: the blocks then take the route that does without them."""
    for blk in enc.encoders:
        w = blk._weights(cfm.resolve_precision(blk))
        for f in packs:
            setattr(w, f, None)


def utterances(name, cfg, seed, B, T, lens, mode="bf16", prepare=None):
    cfm.set_precision(mode)
    enc = build(cfg, seed)
    x = torch.from_numpy(synth.fbank(seed + 1, B, T)).to(DEV)
    lt = torch.tensor(lens, dtype=torch.int32, device=DEV)
    with torch.no_grad():
        if prepare is not None:
            enc(x, lt)                       # packs the weights, so that there is something to withhold
            prepare(enc)
        y, m = enc(x, lt)
    digest(name, y, m)


def streaming_batch(name, causal=False):
    cfm.set_precision("bf16")
    enc = build(CFG, 31)
    streams, chunk, left = 4, 4, 2
    sb = encoder.StreamingBatch(enc, streams, chunk, left, causal_conv=causal, graph=False)
    window, hop = (chunk - 1) * 4 + 7, 4 * chunk
    x = torch.from_numpy(synth.fbank(32, streams, window + 2 * hop)).to(DEV)
    outs = [sb.step(x[:, i * hop: i * hop + window].contiguous()).clone() for i in range(3)]
    digest(name, *outs, sb.kv, sb.offsets, *([sb.conv] if sb.conv is not None else []))


def chunks(name):
    cfm.set_precision("bf16")
    enc = build(CFG, 41)
    x = torch.from_numpy(synth.fbank(42, 2, 131)).to(DEV)
    empty = torch.zeros((0, 0, 0, 0), device=DEV)
    with torch.no_grad():
        y, m = enc.forward_chunk_by_chunk(x[:1], 4, 2)
        y1, c1, _ = enc.forward_chunk(x[:, :19].contiguous(), 0, 8, empty, empty)
        y2, c2, _ = enc.forward_chunk(x[:, 16:35].contiguous(), y1.size(1), 8, c1, empty)
    digest(name, y, m, y1, c1, y2, c2)


def ragged_utterances(name, split=False):
    """forward_utterances: the per-item lengths reach the blocks (cfm_layer_io.utt_len)."""
    cfm.set_precision("bf16")
    enc = build(CFG, 11)
    enc.split_small_batches = split
    x = torch.from_numpy(synth.fbank(12, 3, 210)).to(DEV)
    with torch.no_grad():
        y, out_lens = enc.forward_utterances(x, torch.tensor([210, 131, 9], dtype=torch.int32, device=DEV))
    digest(name, y, out_lens)


def streaming_batch_ragged(name, graph, steps, cfg=CFG):
    """StreamingBatch with per-stream window lengths (cfm_layer_io.stream_len): every step has a full window, a short one, 7 frames and an idle stream."""
    cfm.set_precision("bf16")
    enc = build(cfg, 31)
    streams, chunk, left = 4, 4, 2
    sb = encoder.StreamingBatch(enc, streams, chunk, left, graph=graph)
    window, hop = (chunk - 1) * 4 + 7, 4 * chunk
    x = torch.from_numpy(synth.fbank(32, streams, window + (steps - 1) * hop)).to(DEV)
    lens = [window, 11, 7, 0]
    outs = []
    for i in range(steps):
        outs.append(sb.step(x[:, i * hop: i * hop + window].contiguous(), lens[i % 4:] + lens[:i % 4]).clone())
        outs.append(sb.out_lens.clone())
    digest(name, *outs, sb.kv, sb.offsets)


def chunks_batched(name):
    """forward_chunk at B = 2 with a growing (L,B,H,Tc,2dk) cache."""
    cfm.set_precision("bf16")
    enc = build(CFG, 41)
    x = torch.from_numpy(synth.fbank(43, 2, 35)).to(DEV)
    empty = torch.zeros((0, 0, 0, 0), device=DEV)
    with torch.no_grad():
        y1, c1, _ = enc.forward_chunk(x[:, :19].contiguous(), 0, -1, empty, empty)
        y2, c2, _ = enc.forward_chunk(x[:, 16:35].contiguous(), y1.size(1), -1, c1, empty)
    assert c1.dim() == 5 and c2.size(3) == c1.size(3) + y2.size(1)
    digest(name, y1, c1, y2, c2)


def one_block(name):
    """ConformerEncoderLayer.forward in eval mode, the way the reference's encoder calls it: without and with a (1,H,Tc,2dk) cache."""
    cfm.set_precision("bf16")
    enc = build(CFG, 51)
    blk, T, Tc = enc.encoders[1], 13, 8
    x = torch.randn((1, T, 256), generator=torch.Generator().manual_seed(52)).to(DEV)
    with torch.no_grad():
        y1, _, c1, _ = blk(x, torch.ones((1, T, T), dtype=torch.bool, device=DEV), enc.embed.position_encoding(offset=0, size=T).to(DEV))
        cache = c1[:, :, T - Tc:, :].contiguous()
        y2, _, c2, _ = blk(x, torch.ones((1, T, Tc + T), dtype=torch.bool, device=DEV), enc.embed.position_encoding(offset=T - Tc, size=Tc + T).to(DEV),
                           attn_cache=cache)
    assert tuple(c2.shape) == (1, 4, Tc + T, 128)
    digest(name, y1, c1, y2, c2)


def with_setting(obj, attr, value, fn):
    keep = getattr(obj, attr)
    setattr(obj, attr, value)
    try:
        fn()
    finally:
        setattr(obj, attr, keep)


def main():
    base = dict(cfg=CFG, seed=11, B=3, T=210, lens=[210, 131, 9])                     # T' = 51: 153 rows; the last utterance is one encoder frame
    utterances("a-d256-bf16-chained", **base)
    utterances("a-d256-fp16-chained", mode="fp16", **base)
    prev = cfm.lib().cfm_set_cin_merge(0)
    try:
        utterances("b-d256-bf16-cin-merge-off", **base)
    finally:
        cfm.lib().cfm_set_cin_merge(prev)
    with_setting(encoder_layer, "CHAIN_BLOCKS", False, lambda: utterances("c-d256-bf16-chain-blocks-off", **base))
    utterances("d-d256-bf16-split-small-batches", prepare=lambda enc: setattr(enc, "split_small_batches", True), **base)
    utterances("e-d256-bf16-fused-ffn", prepare=lambda enc: withhold(enc, CHAIN_ONLY_PACKS), **base)
    utterances("f-d256-bf16-general", prepare=lambda enc: withhold(enc, CHAIN_ONLY_PACKS + FFN_PACKS), **base)
    utterances("g-d256-fp32", mode="fp32", **base)
    utterances("h-d256-bf16-absolute-positions", **(base | dict(cfg=CFG | dict(use_relative=False))))
    big = dict(cfg=CFG512, seed=47, B=3, T=400, lens=[400, 333, 270])                  # T' = 99: 297 rows
    utterances("i-d512-bf16-pair", **big)
    with_setting(encoder_layer, "PAIR_MAX_ROWS", 0, lambda: utterances("i-d512-bf16-pair-rows-0", **big))
    utterances("j-d144-bf16", **(base | dict(cfg=CFG144)))
    streaming_batch("k-streaming-batch")
    with_setting(encoder_layer, "SPLIT_FFN_FEW_ROWS", False, lambda: streaming_batch("k-streaming-batch-split-ffn-off"))
    streaming_batch("k-streaming-batch-causal-conv", causal=True)
    chunks("l-forward-chunk")
    ragged_utterances("m-forward-utterances")
    ragged_utterances("m-forward-utterances-split-small-batches", split=True)
    streaming_batch_ragged("n-streaming-batch-frame-lens", graph=False, steps=3)
    streaming_batch_ragged("n-streaming-batch-frame-lens-graph", graph=True, steps=5)
    streaming_batch_ragged("n-streaming-batch-frame-lens-absolute-positions", graph=False, steps=3, cfg=CFG | dict(use_relative=False))
    chunks_batched("o-forward-chunk-batched")
    one_block("p-one-block-forward")


if __name__ == "__main__":
    main()
