"""One conformer block, MI355X-native.

Drop-in for the reference's ``src/encoder_layer.py`` (constructor arguments, child-module and parameter names, and the
``forward(inputs, inputs_attn_mask, pos_embed, inputs_pad_mask, attn_cache, cnn_cache)`` ->
``(out, inputs_attn_mask, new_attn_cache, new_cnn_cache)`` contract of encoder_layer.py:11-71).

The whole block -- LN, 1/2 macaron FFN, LN, MHSA, LN, convolution module, LN, 1/2 FFN, final LN with every residual -- is
ONE call into libconformer_gfx950 (``cfm_encoder_layer_forward``): 4 kernel launches on the row chains (2 per block when the encoder
chains consecutive blocks; 17 on the general path) enqueued from C++ with no host synchronisation, the residual stream in f32, every
bias / activation / GLU / mask / residual add fused into a GEMM epilogue, and LayerNorm writing the next GEMM's operand dtype
directly.  The child modules (feedforward / attention / convolution) only own the parameters here; called on their own they run the
same kernels op by op.
"""
import ctypes
import functools

import torch
import torch.nn as nn

import cfm
from cfm import packing
from attention import MultiHeadSelfAttentionModule, RelativeMultiHeadSelfAttentionModule, _mask_args
from convolution import ConvolutionModule
from feedforward import PositionwiseFeedForwardModule, _inference_only

_ABSENT = torch.ones((0, 0, 0), dtype=torch.bool)
PAIR_MAX_ROWS = 4096       # include/cfm.h CFM_PAIR_MAX_ROWS: the pair-split feed-forward of the D = 512 row chains (one workgroup per CU up to 128 row tiles)
SPLIT_FFN_FEW_ROWS = True  # STREAMING steps of <= cfm_ffsplit_max_rows() (1536) rows run their feed-forwards split over FF/256 workgroups per row tile (csrc/ffnsplit.hip).  Only
# the streaming entry points ask for it (split_ffn=True): a whole-utterance forward keeps one algorithm for every batch size, so that a batch shard
# reproduces the batch bit for bit


@functools.lru_cache(maxsize=None)
def _split_max_rows():
    """The library's row limit (cfm_ffsplit_max_rows: the one reader of CFM_FFSPLIT_MAX_ROWS), asked on first use and not at import, when the library
    may not be built yet."""
    return cfm.lib().cfm_ffsplit_max_rows()


def split_rows(M, D, FF):
    """True where cfm_encoder_layer_forward takes CFM_ROUTE_FFSPLIT when given the slabs."""
    return M <= _split_max_rows() and D == 256 and FF % 256 == 0 and FF > 0


CHAIN_BLOCKS = True        # the final chain of block i also runs the macaron chain of block i+1 (one launch and one residual round trip less)
CHAIN_PACKS = ("ffm_w1f", "ffm_w2n", "ff_w1f", "ff_w2n", "qkv_wf", "out_wf", "pw1_wf", "pw2_wf")   # the fragment-major packs of the row-chain path


def chain_blocks(ws, M, D, FF, ktaps, causal, stateful, after_fused, split_ffn):
    """True when the blocks of a call are chained: block i's last launch runs block i+1's macaron chain too (cfm.h cfm_layer_io.next_w).
    The batch path on the row chains at the config-2 width: every weight struct of `ws` carries the row-chain packs, after_norm rides in the
    last block's final chain (after_fused), no attention or conv cache is returned (stateful), the convolution is not causal, and the call
    does not take the split feed-forward below."""
    return bool(CHAIN_BLOCKS and after_fused and not stateful and not causal and (D, FF, ktaps) == (256, 2048, 15) and
                all(getattr(w, f) for w in ws for f in CHAIN_PACKS) and
                not (split_ffn and SPLIT_FFN_FEW_ROWS and split_rows(M, D, FF)))


def psum_splits(M, D, FF, prec, split_ffn, chained):
    """How many partial slabs [M, D] f32 a block's feed-forwards get (cfm.h cfm_layer_scratch.psum_splits); 0 = none.  A chained block gets
    none: its macaron chain ran in the previous block's last launch."""
    if chained:
        return 0
    if split_ffn and SPLIT_FFN_FEW_ROWS and split_rows(M, D, FF) and prec.act_dtype != torch.float32:
        return FF // 256           # few rows, e.g. a streaming step: the feed-forward split over FF (csrc/ffnsplit.hip)
    if M <= PAIR_MAX_ROWS and cfm.rowchain_pair_supported(D, FF, prec):
        return 3                   # D = 512, at most 128 row tiles: split over workgroup pairs -- two partial slabs + the parked rows of the final chain
    return 0


class BlockCall:
    """What the blocks of ONE encoder call share, derived once: shape, precision, the masks and positional rows as the library wants them, the
    streaming offsets and lengths, the scratch buffers (one lookup per tag; `hid` and `psum` sized for the largest hidden_dim, since a tag names
    one arena block) and one LayerIO / LayerScratch with those fields filled.  `run` is one block: it ASSIGNS every per-block field on every call
    (None / 0 where the block has none), so nothing set for block i reaches block i+1; the structs are not copied.

    x (B,T,D) on an MI355X; attn_mask broadcastable to (B,T,cache_T+T), or the (B,1,ring_T) slot mask with ring = (offsets int32 [B], ring_T);
    pos_embed: the positional rows (None: absolute positions); pad_mask (B,1,T) | None.
    utt_len int32 [B]: a ragged batch of whole utterances, item b has utt_len[b] frames (cfm.h cfm_layer_io.utt_len); the caller masks the keys.
    stream_len int32 [B] (with ring): stream b's window has stream_len[b] encoder frames (cfm.h cfm_layer_io.stream_len).
    causal: the opt-in causal convolution for every block; None = each block's own conv_module.causal.
    split_ffn: a streaming entry point asks for the split feed-forward; chained: chain_blocks() of this call."""

    def __init__(self, x, prec, attn_mask, pos_embed, pad_mask, hidden_dims, cache_T=0, pos_shared=False, ring=None, utt_len=None,
                 stream_len=None, causal=None, split_ffn=False, chained=False):
        cfm.require_hip(x)
        if x.dtype != torch.float32 or not x.is_contiguous():
            x = x.float().contiguous()
        B, T, D = x.shape
        M, dev, adt = B * T, x.device, prec.act_dtype
        self.x, self.causal, self.cache_T, self.Tk = x, causal, cache_T, cache_T + T if ring is None else ring[1]
        pos, R = None, 0
        if pos_embed is not None:
            pos = pos_embed.reshape(-1, D)
            pos = (pos if pos.dtype == torch.float32 else pos.float()).contiguous()
            R = pos.size(0)
        m8, (m_sb, m_sq) = _mask_args(attn_mask, B, T, self.Tk)
        keep = None
        if pad_mask is not None and pad_mask.dim() >= 3 and pad_mask.size(2) > 0:
            keep = cfm.as_u8_mask(pad_mask).reshape(-1)
            if keep.numel() != M:
                raise RuntimeError("pad mask %s does not match inputs %s" % (tuple(pad_mask.shape), tuple(x.shape)))
        for name, t in (("utt_len", utt_len), ("stream_len", stream_len), ("ring offsets", ring[0] if ring is not None else None)):
            if t is not None and (t.dtype != torch.int32 or t.numel() != B or not t.is_contiguous()):
                raise RuntimeError("%s must be a contiguous int32 tensor of B entries" % name)
        cfm.require_hip(pos, m8, keep, utt_len, stream_len, ring[0] if ring is not None else None)
        self._keep = (pos, m8, keep)                   # conversions may have copied: the structs hold their addresses
        s = self.scratch = cfm.LayerScratch()
        for tag, numel in (("xn", M * D), ("hid", M * max(hidden_dims)), ("qkv", M * 3 * D), ("pos", max(R, 1) * D), ("ctx", M * D), ("glu", M * D), ("dw", M * D)):
            setattr(s, tag, cfm.scratch(tag, numel, adt, dev).data_ptr())
        self.splits = {ff: psum_splits(M, D, ff, prec, split_ffn, chained) for ff in set(hidden_dims)}
        self.psum = cfm.scratch("psum", max(self.splits.values()) * M * D, torch.float32, dev).data_ptr() if any(self.splits.values()) else None
        io = self.io = cfm.LayerIO()
        io.B, io.T, io.D, io.act_dtype, io.w_dtype = B, T, D, prec.act_code, prec.w_code
        io.attn_mask, io.am_sb, io.am_sq, io.pad_valid = cfm.ptr(m8), m_sb, m_sq, cfm.ptr(keep)
        io.pos_embed, io.pos_rows, io.pos_shared, io.cache_T = cfm.ptr(pos), R, 1 if pos_shared else 0, cache_T
        if ring is not None:
            io.stream_offset, io.ring_T = ring[0].data_ptr(), ring[1]
        io.utt_len, io.stream_len = cfm.ptr(utt_len), cfm.ptr(stream_len)
        self.stream = cfm.stream()

    def run(self, block, w, x_in, out, xn_ready=False, next_norm=None, cache=None, want_cache=False, pos_proj=None, kv_ring=None, conv_cache=None,
            next_w=None, next_out=None, macaron_done=False, after=None):
        """One block: x_in (B,T,D) f32 -> out = norm_final(block(x_in)), returns the new attention cache or None.  `w`: the block's cached weight struct.
        cache f32 (B,H,cache_T,2dk) | None; kv_ring f32 [B,H,ring_T,2dk]: the block's streaming ring (cfm.h cfm_layer_io.kv_ring); conv_cache f32
        [B,K-1,D]: the causal convolution's left context; pos_proj = (view [R, D] of the driver's all-blocks projection, row stride);
        after = (gain, bias, f32 output [B,T,D]): the encoder's after_norm in the final chain.
        next_w, next_out: this block's last launch also runs the NEXT block's macaron chain into next_out (cfm.h cfm_layer_io.next_w); the next
        block is then run with macaron_done=True on that buffer, and `out` does not hold this block's output."""
        _inference_only(block, "ConformerEncoderLayer")
        io, s = self.io, self.scratch
        B, T, D = self.x.shape
        H, K, Tk = block.num_heads, block.kernel_size, self.Tk
        io.H, io.FF, io.ktaps = H, block.hidden_dim, K
        s.psum_splits = self.splits[block.hidden_dim]
        s.psum = self.psum if s.psum_splits else None
        if cache is not None:
            cache = cache.to(device=self.x.device, dtype=torch.float32).contiguous()
            if tuple(cache.shape) != (B, H, self.cache_T, 2 * (D // H)):
                raise RuntimeError("attn_cache of shape %s, expected (%d,%d,%d,%d)" % (tuple(cache.shape), B, H, self.cache_T, 2 * (D // H)))
        if kv_ring is not None and (kv_ring.dtype != torch.float32 or tuple(kv_ring.shape) != (B, H, Tk, 2 * (D // H)) or not kv_ring.is_contiguous()):
            raise RuntimeError("ring: kv must be contiguous float32 (B,H,ring_T,2dk)")
        causal = getattr(block.conv_module, "causal", False) if self.causal is None else self.causal
        if conv_cache is not None:
            if not causal:
                raise RuntimeError("a conv cache needs the opt-in causal convolution (causal=True, or conv_module.causal = True)")
            if conv_cache.dtype != torch.float32 or tuple(conv_cache.shape) != (B, K - 1, D) or not conv_cache.is_contiguous():
                raise RuntimeError("conv_cache must be contiguous float32 (B, kernel_size-1, D)")
        if next_w is not None and (next_out.data_ptr() == out.data_ptr() or next_out.shape != out.shape or next_out.dtype != torch.float32):
            raise RuntimeError("chaining: the next block's output buffer must be a distinct float32 tensor of the same shape")
        cfm.require_hip(kv_ring, conv_cache)
        new_cache = None
        if kv_ring is None and (cache is not None or want_cache):
            new_cache = torch.empty((B, H, Tk, 2 * (D // H)), dtype=torch.float32, device=self.x.device)
        io.attn_cache, io.new_cache, io.kv_ring = cfm.ptr(cache), cfm.ptr(new_cache), cfm.ptr(kv_ring)
        io.causal_conv, io.conv_cache = 1 if causal else 0, cfm.ptr(conv_cache)
        io.pos_proj, io.pos_proj_ld = (pos_proj[0].data_ptr(), pos_proj[1]) if pos_proj is not None else (None, 0)
        io.after_g, io.after_b, io.after_out = [t.data_ptr() for t in after] if after is not None else (None, None, None)
        io.next_w = ctypes.cast(ctypes.pointer(next_w), ctypes.c_void_p) if next_w is not None else None
        io.next_x_out = cfm.ptr(next_out) if next_w is not None else None
        io.macaron_done = 1 if macaron_done else 0
        ng, nb = (next_norm.weight.data_ptr(), next_norm.bias.data_ptr()) if next_norm is not None else (None, None)
        cfm.check(cfm.lib().cfm_encoder_layer_forward(ctypes.byref(w), ctypes.byref(s), ctypes.byref(io), x_in.data_ptr(), out.data_ptr(),
                                                      1 if xn_ready else 0, ng, nb, self.stream), "cfm_encoder_layer_forward")
        return new_cache


class ConformerEncoderLayer(nn.Module):

    def __init__(self, encoder_dim, kernel_size, feedforward_dropout, attention_dropout, hidden_dim, num_heads, use_relative):
        super().__init__()
        self.feed_forward = PositionwiseFeedForwardModule(encoder_dim, feedforward_dropout, hidden_dim)
        attn_cls = RelativeMultiHeadSelfAttentionModule if use_relative else MultiHeadSelfAttentionModule
        self.self_attn = attn_cls(encoder_dim, num_heads, attention_dropout)
        self.conv_module = ConvolutionModule(encoder_dim, kernel_size, hidden_dim)     # sic: lands in `bias` (quirk Q1)
        self.feed_forward_macaron = PositionwiseFeedForwardModule(encoder_dim, feedforward_dropout, hidden_dim)
        self.norm_ff = nn.LayerNorm(encoder_dim, eps=1e-5)
        self.norm_ff_macaron = nn.LayerNorm(encoder_dim, eps=1e-5)
        self.norm_mha = nn.LayerNorm(encoder_dim, eps=1e-5)
        self.norm_conv = nn.LayerNorm(encoder_dim, eps=1e-5)
        self.norm_final = nn.LayerNorm(encoder_dim, eps=1e-5)
        self.dropout = nn.Dropout(feedforward_dropout)
        self.use_relative = bool(use_relative)
        self.encoder_dim, self.hidden_dim, self.num_heads, self.kernel_size = encoder_dim, hidden_dim, num_heads, kernel_size
        self.return_cache = True           # the reference always materialises cat(k,v) (attention.py:76)

    def _weights(self, prec):
        # the tensor list is rebuilt on every call: replacing a Parameter OBJECT (layer.norm_ff.weight = nn.Parameter(...), pruning /
        # reparametrisation, swapping a submodule) must change the key too; walking ~40 tensors is cheap next to a 5-launch block (read off
        # the modules' own dicts: parameters() + buffers() walk the tree twice and build every dotted name, 2.4x the time; weights_key
        # skips the absent entries).  The slot holds (LayerWeights, keepalive); .to() / .cuda() / .half() change address, device or dtype
        plist = [t for m in self.modules() for d in (m._parameters, m._buffers) for t in d.values()]
        key = packing.weights_key(plist, prec.name)
        return packing.slot(self, "_fused").get(key, lambda: packing.layer_weight_struct(self, prec))[0]

    def train_forward(self, inputs, inputs_attn_mask, inputs_pad_mask):
        """module.train(): the block as ONE autograd node (cfm/autograd.py EncoderLayerFn) -- BatchNorm batch statistics, every
        parameter's gradient returned from its backward.  encoder_layer.py:49-71 with the shared nn.Dropout(feedforward_dropout)."""
        from cfm import autograd as ag
        cfm.require_hip(inputs)
        B, T, D = inputs.shape
        m8, m_str = _mask_args(inputs_attn_mask, B, T, T)
        keep = None
        if inputs_pad_mask is not None and inputs_pad_mask.dim() >= 3 and inputs_pad_mask.size(2) > 0:
            keep = cfm.as_u8_mask(inputs_pad_mask).reshape(-1)
            if keep.numel() != B * T:
                raise RuntimeError("pad mask %s does not match inputs %s" % (tuple(inputs_pad_mask.shape), tuple(inputs.shape)))
        leaf = self.__dict__.get("_flat_leaf")         # set by trainer.DataParallelTrainer: the block's parameters as ONE autograd leaf
        params = (leaf,) if leaf is not None else tuple(self.parameters())
        return ag.EncoderLayerFn.apply(inputs, self, cfm.resolve_precision(self), m8, m_str, keep, *params)

    def forward(self, inputs, inputs_attn_mask, pos_embed, inputs_pad_mask=_ABSENT, attn_cache=_ABSENT, cnn_cache=_ABSENT):
        if cfm.check_mode(self, "ConformerEncoderLayer"):
            if attn_cache is not None and attn_cache.dim() == 4 and attn_cache.size(0) > 0:
                raise NotImplementedError("ConformerEncoderLayer: a KV cache in train mode (streaming is inference-only)")
            out = self.train_forward(inputs, inputs_attn_mask, inputs_pad_mask)
            return (out, inputs_attn_mask, torch.zeros((0, 0, 0, 0), dtype=torch.float32, device=inputs.device),
                    torch.zeros((0, 0, 0), dtype=inputs.dtype, device=inputs.device))
        have_cache = attn_cache is not None and attn_cache.dim() == 4 and attn_cache.size(0) > 0
        prec = cfm.resolve_precision(self)
        call = BlockCall(inputs, prec, inputs_attn_mask, pos_embed if self.use_relative else None, inputs_pad_mask, [self.hidden_dim],
                         cache_T=attn_cache.size(2) if have_cache else 0)
        out = torch.empty_like(call.x)
        new_attn_cache = call.run(self, self._weights(prec), call.x, out, cache=attn_cache if have_cache else None, want_cache=self.return_cache)
        if new_attn_cache is None:
            new_attn_cache = torch.zeros((0, 0, 0, 0), dtype=torch.float32, device=inputs.device)
        new_cnn_cache = torch.zeros((0, 0, 0), dtype=inputs.dtype, device=inputs.device)    # convolution.py:39
        return out.to(inputs.dtype), inputs_attn_mask, new_attn_cache, new_cnn_cache
