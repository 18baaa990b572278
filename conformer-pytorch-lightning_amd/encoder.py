"""Conformer encoder driver, MI355X-native: subsampling front-end, N conformer blocks, final LayerNorm; whole-utterance
``forward`` and the streaming pair ``forward_chunk`` / ``forward_chunk_by_chunk``.

Mirrors the public surface of the reference's ``src/encoder.py`` (constructor arguments :11-27, ``forward`` :54-75,
``forward_chunk`` :78-123, ``forward_chunk_by_chunk`` :125-153) so it can stand in for it; the reference's own
encoder.py also runs unchanged on top of the drop-in modules of this directory.  Differences are in HOW, not WHAT:

* masks are built on the device from the lengths (one launch each; the subsampled padding mask directly as
  ``6 + 4 j < len``), bit-identical to the reference's arange / slicing / python row loop;
* each block is one C call (2 launches on the row-chain path with consecutive blocks chained -- attention, then conv-in + depthwise + final + the next block's macaron chain --, 4 without, 17 on the general one); consecutive blocks hand over the already-normalised macaron-FFN operand
  (norm_final of block i and norm_ff_macaron of block i+1 are chained in registers);
* the batch path does not materialise the per-layer cat(k,v) cache that the reference builds and discards.
"""
import torch
import torch.nn as nn

import cfm
from cfm import packing
from attention import PositionalEncoding, RelativePositionalEncoding
from convolution import ConvolutionSubSampling
import encoder_layer
from encoder_layer import ConformerEncoderLayer
from utils import make_attn_mask, make_pad_mask

_NO_MASK = torch.ones((0, 0, 0))


class ConformerEncoder(nn.Module):

    def __init__(self, input_dim, kernel_size, encoder_dim, dropout, attention_dropout, pos_enc_dropout, hidden_dim,
                 num_heads, encoder_num_layers, cmvn=None, max_len=5000, use_relative=False, use_dynamic_chunk_size=False,
                 use_dynamic_left_chunk=False, static_chunk_size=-1):
        super().__init__()
        pe_cls = RelativePositionalEncoding if use_relative else PositionalEncoding
        self.position_encoding = pe_cls(encoder_dim, pos_enc_dropout, max_len)
        self.embed = ConvolutionSubSampling(input_dim=input_dim, output_dim=encoder_dim, pos_enc=self.position_encoding)
        self.encoders = nn.ModuleList([
            ConformerEncoderLayer(encoder_dim, kernel_size, dropout, attention_dropout, hidden_dim, num_heads, use_relative)
            for _ in range(encoder_num_layers)])
        self.encoder_dim = encoder_dim
        self.after_norm = nn.LayerNorm(encoder_dim, eps=1e-5)
        self.global_cmvn = cmvn
        self.use_dynamic_chunk_size = use_dynamic_chunk_size
        self.use_dynamic_left_chunk = use_dynamic_left_chunk
        self.static_chunk_size = static_chunk_size

    # ------------------------------------------------------------------------------------------------------------
    def _run_blocks(self, x, attn_mask, pos_embed, pad_mask, caches, keep_from, pos_shared=False, proj=None, ring=None, conv=None, streaming=False, utt_len=None,
                    stream_len=None, causal=None):
        """x (B,T',D) f32 -> after_norm(blocks(x)); returns (y, [trimmed per-layer caches] | None).
        caches: None, empty, (L,H,Tc,2dk) or batched (L,B,H,Tc,2dk); not None = the new caches are returned, rows from keep_from on.
        ring = (kv f32 [L,B,H,ring_T,2dk], offsets int32 [B]), conv = f32 [L,B,K-1,D] | None: per-stream streaming state (StreamingBatch).
        utt_len, stream_len, causal and streaming (= split_ffn) are encoder_layer.BlockCall's; the routes are picked beside it."""
        n, D, e0 = len(self.encoders), self.encoder_dim, self.encoders[0]
        if proj is None:
            proj = self._project_positions(pos_embed, x)
        prec = cfm.resolve_precision(self)
        ws = [blk._weights(prec) for blk in self.encoders]
        # after_norm rides in the last block's final chain when that block runs on the row chains (one launch less)
        fuse_after = (cfm.rowchain_supported(D, e0.hidden_dim, prec) and self.after_norm.weight.dtype == torch.float32 and self.after_norm.eps == 1e-5)
        after_w = self.after_norm.weight.detach(), self.after_norm.bias.detach()
        chain = encoder_layer.chain_blocks(ws, x.size(0) * x.size(1), D, e0.hidden_dim, e0.kernel_size,
                                           getattr(e0.conv_module, "causal", False) if causal is None else causal,
                                           caches is not None or conv is not None, fuse_after, streaming)
        have = caches is not None and caches.dim() in (4, 5) and caches.size(0) > 0
        call = encoder_layer.BlockCall(x, prec, attn_mask, pos_embed if e0.use_relative else None, pad_mask, [blk.hidden_dim for blk in self.encoders],
                                       cache_T=caches.size(-2) if have else 0, pos_shared=pos_shared, ring=None if ring is None else (ring[1], ring[0].size(3)),
                                       utt_len=utt_len, stream_len=stream_len, causal=causal, split_ffn=streaming, chained=chain)
        bufs = [torch.empty_like(call.x), torch.empty_like(call.x)]
        y_after = torch.empty_like(call.x) if fuse_after else None
        new_caches = [] if caches is not None else None
        cur = call.x
        for i, (block, w) in enumerate(zip(self.encoders, ws)):
            last, out = i + 1 == n, bufs[i & 1]
            nc = call.run(block, w, cur, out, xn_ready=i > 0, next_norm=None if last else self.encoders[i + 1].norm_ff_macaron,
                          cache=None if not have else caches[i] if caches.dim() == 5 else caches[i:i + 1], want_cache=caches is not None,
                          pos_proj=None if proj is None else (proj[:, i * D:], proj.stride(0)),
                          kv_ring=None if ring is None else ring[0][i], conv_cache=None if conv is None else conv[i],
                          next_w=None if last or not chain else ws[i + 1], next_out=bufs[(i + 1) & 1], macaron_done=chain and i > 0,
                          after=after_w + (y_after,) if fuse_after and last else None)
            if new_caches is not None:
                new_caches.append(nc[:, :, keep_from:, :])
            cur = out
        if fuse_after:
            return y_after, new_caches
        y, _ = cfm.layernorm(cur.view(-1, D), *after_w, eps=self.after_norm.eps)
        return y.view_as(cur), new_caches

    def _cmvn_args(self, inputs):
        """(inputs, cmvn tuple for the front-end): a GlobalCMVN-like module with float32 `mean` / `istd` buffers on the input's device is
        folded into the first convolution (bit-identical); anything else is applied as the module it is."""
        m = self.global_cmvn
        if m is None:
            return inputs, None
        mean, istd = getattr(m, "mean", None), getattr(m, "istd", None)
        ok = (isinstance(mean, torch.Tensor) and isinstance(istd, torch.Tensor) and mean.dtype == torch.float32 and istd.dtype == torch.float32 and
              mean.dim() == 1 and mean.shape == istd.shape and mean.numel() == inputs.size(-1) and mean.device == inputs.device and
              inputs.dtype == torch.float32)
        if not ok:
            return m(inputs), None
        return inputs, (mean.contiguous(), istd.contiguous() if getattr(m, "norm_var", True) else None)

    def _project_positions(self, pos_embed, x):
        """linear_pos of EVERY block applied to pos_embed in one GEMM: [R, D] . [L*D, D]^T -> [R, L*D] (block i reads columns
        i*D .. (i+1)*D).  The per-block projections are 8 us launches of a 32-row GEMM in the batch path otherwise."""
        if not isinstance(self.position_encoding, RelativePositionalEncoding) or pos_embed is None:
            return None
        prec = cfm.resolve_precision(self)
        ws = [blk.self_attn.linear_pos.weight for blk in self.encoders]
        pk = packing.slot(self, "_pos_pack", packing.PackCache).get(ws, prec, lambda: packing.Packed(w=packing.matrix(torch.cat([w.detach() for w in ws], 0), prec)))
        pe = pos_embed.reshape(-1, self.encoder_dim)
        pe = (pe if pe.dtype == torch.float32 else pe.float()).contiguous()
        return cfm.gemm(pe, pk.w[0], w_lo=pk.w[1], out_dtype=prec.act_dtype)

    def set_precision(self, name):
        """Pin this encoder (every drop-in module under it) to a precision mode, independent of the process default
        (cfm.set_precision): 'bf16' | 'fp16' | 'fp32' | None (follow the default again)."""
        prec = None if name is None else (name if isinstance(name, cfm.Precision) else cfm.Precision(name))
        for m in self.modules():
            m.precision = prec
        return self

    def forward(self, inputs, input_lengths, decoding_chunk_size=0, num_decoding_chunk_size=-1):
        if self.training:
            # train mode (encoder.py:54-75 under module.train()): an accumulation window of one micro-batch
            return self.forward_window([(inputs, input_lengths)], decoding_chunk_size, num_decoding_chunk_size)[0]
        inputs, cmvn = self._cmvn_args(inputs)
        cfm.require_hip(inputs, input_lengths)
        frames = inputs.size(1)
        x = self.embed.embed_frames(inputs, cmvn)
        x, pos_embed = self.position_encoding(x, 0)
        # (~make_pad_mask(len, T))[:, None, :][:, :, 2::2][:, :, 2::2]  ==  (6 + 4 j < len), built in one launch
        pad_mask = cfm.valid_mask(input_lengths, x.size(1), first=6, stride=4).unsqueeze(1)
        # (Tried: positional projection + mask on a side stream beside the front-end.  Under graph replay the fork/join costs more
        # than the ~11 us it hides and the concurrent kernels slow the first convolution: 1.697 vs 1.668 ms per step.)
        attn_mask = make_attn_mask(x, pad_mask, self.use_dynamic_chunk_size, self.use_dynamic_left_chunk,
                                   decoding_chunk_size, self.static_chunk_size, num_decoding_chunk_size)
        # split_small_batches (attribute, default False): a whole-utterance forward of <= 1536 rows (up to 6 x 1000 frames) takes the split
        # feed-forward path of the streaming steps (csrc/ffnsplit.hip) -- lower latency for a small batch; off by default because the result then
        # depends on which side of 1536 rows the batch falls (to rounding, 1e-3 of the output), and a batch shard no longer reproduces the batch bit for bit
        y, _ = self._run_blocks(x, attn_mask, pos_embed, pad_mask, None, 0, streaming=bool(getattr(self, "split_small_batches", False)))
        return y.to(inputs.dtype), pad_mask

    def forward_utterances(self, inputs, input_lengths):
        """A ragged batch of WHOLE utterances with the DECODING path's semantics (beyond the reference, which decodes at batch 1): inputs (B,T,F),
        input_lengths (B,) frames per item -> (outputs (B,T'max,D), out_lens int32 (B,)), out_lens[b] = ((len_b - 1)//2 - 1)//2, 0 below 7 frames
        (where the reference's forward_chunk_by_chunk has nothing to concatenate).  Rows [0, out_lens[b]) of item b are what the reference's
        greedy_search computes for that utterance alone -- forward_chunk(inputs[b:b+1, :len_b], 0, -1, empty, empty), model.py:202-212 --; rows at
        and past out_lens[b] are zero.  Unlike `forward` (the training path's semantics in eval mode) every item attends over its own keys with the real
        positional term from the shared rows pe[0:T'max], and its depthwise convolutions read zeros past its last frame, as at a tensor edge
        (cfm_layer_io.utt_len: a select behind the GLU).  Routes as in `forward` (split_small_batches included); no cache is materialised."""
        if self.training:
            raise NotImplementedError("ConformerEncoder.forward_utterances: whole-utterance decoding is inference-only; call .eval()")
        if not isinstance(self.position_encoding, RelativePositionalEncoding):
            raise NotImplementedError("ConformerEncoder.forward_utterances needs use_relative=True: the absolute table is indexed by batch item "
                                      "(a quirk of the reference) and would need a path of its own")
        inputs, cmvn = self._cmvn_args(inputs)
        cfm.require_hip(inputs, input_lengths)
        x = self.embed.embed_frames(inputs, cmvn)
        x, _ = self.position_encoding(x, 0)
        Ts = x.size(1)
        # keys j of item b with 6 + 4 j < len_b: the first out_lens[b] = (len_b - 3) // 4 of them (two stride-2 convolutions of 3 taps, no padding)
        keys = cfm.valid_mask(input_lengths, Ts, first=6, stride=4).unsqueeze(1)
        out_lens = torch.div(input_lengths.to(torch.int32) - 3, 4, rounding_mode="floor").clamp_(0, Ts).to(torch.int32)
        pos_embed = self.embed.position_encoding(offset=0, size=Ts)
        y, _ = self._run_blocks(x, keys, pos_embed, None, None, 0, pos_shared=True, streaming=bool(getattr(self, "split_small_batches", False)),
                                utt_len=out_lens)
        y.masked_fill_(~keys.transpose(1, 2), 0.0)
        return y.to(inputs.dtype), out_lens

    def forward_window(self, batches, decoding_chunk_size=0, num_decoding_chunk_size=-1, return_rows=False):
        """Train mode: the micro-batches of ONE accumulation window (train.sh:36 accum_grad; the weights do not change between them) in a single
        pass.  batches: [(inputs (B_g,T_g,F), lengths (B_g,)), ...]; returns [(outputs (B_g,T'_g,D), pad mask (B_g,1,T'_g)), ...], item g equal to
        what `forward(*batches[g])` returns when the micro-batches are run one after the other as the reference does (encoder.py:54-75 called
        accum_grad times; BatchNorm batch statistics per micro-batch, running statistics updated in micro-batch order; dropout masks
        differ, as between any two calls).  The rows of all micro-batches go through the block stack TOGETHER (cfm/autograd.py EncoderStackFn:
        the dense products, LayerNorms and the weight gradients see one [sum B_g*T'_g, D] row matrix; attention, depthwise convolution and
        BatchNorm run per micro-batch), so a window costs about half the launches of two passes and its weight gradient is one product.
        return_rows: also return the outputs as ONE row matrix f32 [sum B_g*T'_g, D] (what the per-micro-batch outputs are views of) -- a head that is
        row-local up to its loss (CTCDecoder.forward_window) then projects all micro-batches in one launch: returns (rows, outs)."""
        if not self.training:
            raise RuntimeError("ConformerEncoder.forward_window is the train-mode pass over an accumulation window; in eval mode call forward per batch")
        from cfm import autograd as ag
        from encoder_layer import _mask_args
        layers = list(self.encoders)
        flat = all(l.__dict__.get("_flat_leaf") is not None for l in layers)
        ag.check_params(layers, flat)
        if not ag.stack_supported(layers, len(batches)):
            # blocks that cannot share one io struct (different sizes or dropout rates; BatchNorm momentum=None over several micro-batches):
            # micro-batch after micro-batch, block by block (cfm/autograd.py EncoderLayerFn)
            outs = []
            for inputs, lengths in batches:
                inputs, cmvn = self._cmvn_args(inputs)
                cfm.require_hip(inputs, lengths)
                x, pos_embed = self.position_encoding(self.embed.embed_frames(inputs, cmvn), 0)
                pad_mask = cfm.valid_mask(lengths, x.size(1), first=6, stride=4).unsqueeze(1)
                attn_mask = make_attn_mask(x, pad_mask, self.use_dynamic_chunk_size, self.use_dynamic_left_chunk, decoding_chunk_size,
                                           self.static_chunk_size, num_decoding_chunk_size)
                for block in layers:
                    x, attn_mask, _, _ = block(x, attn_mask, pos_embed, pad_mask)
                y = ag.LayerNormFn.apply(x, self.after_norm.weight, self.after_norm.bias, self.after_norm.eps)
                outs.append((y.to(inputs.dtype), pad_mask))
            if return_rows:
                return torch.cat([y.float().reshape(-1, y.size(-1)) for y, _ in outs], 0), outs
            return outs
        prec = cfm.resolve_precision(self)
        rows, groups, keeps, shapes, pads = [], [], [], [], []
        for gi, (inputs, lengths) in enumerate(batches):
            inputs, cmvn = self._cmvn_args(inputs)
            cfm.require_hip(inputs, lengths)
            x, pos_embed = self.position_encoding(self.embed.embed_frames(inputs, cmvn), 0)
            B, T, D = x.shape
            pad_mask = cfm.valid_mask(lengths, T, first=6, stride=4).unsqueeze(1)
            attn_mask = make_attn_mask(x, pad_mask, self.use_dynamic_chunk_size, self.use_dynamic_left_chunk, decoding_chunk_size,
                                       self.static_chunk_size, num_decoding_chunk_size)
            m8, m_str = _mask_args(attn_mask, B, T, T)
            cfm.require_hip(m8)
            rows.append(x.reshape(B * T, D))
            groups.append((B, T, m8, m_str))
            keeps.append(cfm.as_u8_mask(pad_mask).reshape(-1))
            shapes.append((B, T, inputs.dtype))
            pads.append(pad_mask)
        x_rows = rows[0] if len(rows) == 1 else torch.cat(rows, 0)
        x_rows = (x_rows if x_rows.dtype == torch.float32 else x_rows.float()).contiguous()
        keep = keeps[0] if len(keeps) == 1 else torch.cat(keeps, 0)
        params = tuple(l.__dict__["_flat_leaf"] for l in layers) if flat else tuple(p for l in layers for p in l.parameters())
        y = ag.EncoderStackFn.apply(x_rows, self, layers, prec, groups, keep, flat, *params)
        y = ag.LayerNormFn.apply(y, self.after_norm.weight, self.after_norm.bias, self.after_norm.eps)
        outs, r0 = [], 0
        for (B, T, dt), pad_mask in zip(shapes, pads):
            outs.append((y[r0:r0 + B * T].view(B, T, -1).to(dt), pad_mask))
            r0 += B * T
        return (y, outs) if return_rows else outs

    def forward_chunk(self, inputs, offset, required_cache_size, attn_cache, cnn_cache, inputs_attn_mask=_NO_MASK, pos_rows=None, abs_rows=None):
        """One streaming step.  Batch 1 as in the reference: attn_cache (L,H,Tc,2dk) or empty; returns (chunk output, new attn
        cache (L,H,Tc',2dk), cnn cache (L,0,0,0) -- the reference keeps no conv context).
        Batch B > 1 (beyond the reference, whose forward_chunk only works at batch 1: SURVEY 8 row S): B streams in lockstep at
        the same `offset`, attn_cache (L,B,H,Tc,2dk) or empty, returned cache (L,B,H,Tc',2dk); item b of the result equals the
        batch-1 call on inputs[b:b+1] with attn_cache[:, b].
        pos_rows (cached + chunk, 1, D): the positional rows for this step in a caller-owned buffer instead of a slice taken at `offset`
        (StreamingSession replays one captured graph per step and refreshes that buffer between replays)."""
        if self.training:
            raise NotImplementedError("ConformerEncoder.forward_chunk: streaming is inference-only; call .eval()")
        inputs, cmvn = self._cmvn_args(inputs)
        cfm.require_hip(inputs)
        dev = inputs.device
        attn_cache = attn_cache.to(dev)
        x = self.embed.embed_frames(inputs, cmvn)
        if abs_rows is not None:                    # absolute encoding, rows in a caller-owned buffer (StreamingSession)
            x, _ = self.position_encoding(x, offset, rows=abs_rows)
        else:
            x, _ = self.position_encoding(x, offset)
        batched = inputs.size(0) > 1
        have = attn_cache.dim() == (5 if batched else 4) and attn_cache.size(0) > 0
        if batched and attn_cache.dim() == 4 and attn_cache.size(0) > 0:
            raise RuntimeError("forward_chunk with %d streams needs attn_cache of shape (L,B,H,Tc,2dk)" % inputs.size(0))
        cached = attn_cache.size(-2) if have else 0
        span = cached + x.size(1)
        pos_embed = pos_rows if pos_rows is not None else self.embed.position_encoding(offset=offset - cached, size=span)
        if pos_embed.size(0) != span:
            raise RuntimeError("forward_chunk: %d positional rows for %d keys" % (pos_embed.size(0), span))
        if required_cache_size < 0:
            keep_from = 0
        elif required_cache_size == 0:
            keep_from = span
        else:
            keep_from = max(span - required_cache_size, 0)
        caches = attn_cache if have else torch.zeros((0, 0, 0, 0), device=dev)
        y, new = self._run_blocks(x, inputs_attn_mask, pos_embed, None, caches, keep_from, pos_shared=batched, streaming=True)
        r_attn = torch.stack(new, dim=0) if batched else torch.cat(new, dim=0)
        r_cnn = torch.zeros((len(self.encoders), 0, 0, 0), dtype=x.dtype, device=dev)
        return y.to(inputs.dtype), r_attn, r_cnn

    def forward_chunk_by_chunk(self, inputs, decoding_chunk_size, num_decoding_left_chunks=-1):
        """Simulated streaming over a whole utterance: windows of (c-1)*4+7 frames every 4*c frames."""
        hop = 4 * decoding_chunk_size
        window = (decoding_chunk_size - 1) * 4 + 7
        total = inputs.size(1)
        need = decoding_chunk_size * num_decoding_left_chunks
        attn_cache = torch.zeros((0, 0, 0, 0), device=inputs.device)
        cnn_cache = torch.zeros((0, 0, 0, 0), device=inputs.device)
        pieces, offset = [], 0
        for start in range(0, total - 7 + 1, hop):
            y, attn_cache, cnn_cache = self.forward_chunk(inputs[:, start:min(start + window, total), :], offset, need,
                                                          attn_cache, cnn_cache)
            pieces.append(y)
            offset += y.size(1)
        out = torch.cat(pieces, 1)
        return out, torch.ones((out.size(0), 1, out.size(1)))


def _weights_moved(owner):
    """Whether owner.enc's weights (packing.graph_watch) differ from those of the last call, which it records in owner._sig: asked before every
    replay -- a captured graph holds raw pointers to the packed weights of its capture and is dropped then -- and called after every capture."""
    sig, owner._sig = owner._sig, packing.graph_watch(owner)
    return sig != owner._sig


class StreamingSession:
    """B streams advanced in lockstep, chunk by chunk, with ONE captured HIP graph per steady-state step.

    The eager streaming step is launch-bound (~70 launches for a 16-frame chunk).  Once the left-context cache is full every step has
    the same shapes, so the step is captured once -- static buffers for the feature window, the positional rows and the KV cache,
    the new cache copied back into the static one inside the graph -- and replayed; only the window and the positional rows are
    refreshed between replays.  Results are those of ConformerEncoder.forward_chunk (bit for bit: the same kernels on the same data).
    `step` returns a buffer that the next step overwrites."""

    def __init__(self, encoder, decoding_chunk_size, num_decoding_left_chunks):
        if num_decoding_left_chunks <= 0:
            raise ValueError("StreamingSession needs a bounded left context (num_decoding_left_chunks > 0): the step shapes must settle")
        self.enc = encoder
        self.chunk = decoding_chunk_size
        self.need = decoding_chunk_size * num_decoding_left_chunks
        self.window = (decoding_chunk_size - 1) * 4 + 7
        self.hop = 4 * decoding_chunk_size
        self.offset = 0
        self.cache = None
        self.graph = self._sig = None
        self.relative = isinstance(encoder.position_encoding, RelativePositionalEncoding)

    def _abs_rows(self, batch, dev):
        pe = self.enc.position_encoding._table_like(torch.empty(0, device=dev, dtype=torch.float32))
        return pe[self.offset: self.offset + batch]

    def step(self, frames):
        """frames (B, window, F) on the GPU -> (B, chunk, D)."""
        if frames.size(1) != self.window:
            raise ValueError("StreamingSession.step wants windows of %d frames" % self.window)
        dev = frames.device
        empty = torch.zeros((0, 0, 0, 0), device=dev)
        if self.graph is not None and _weights_moved(self):
            self.cache, self.graph = self.kv.clone(), None            # weights changed under the captured graph: back to eager, re-capture
        if self.graph is None:
            cache = self.cache if self.cache is not None else empty
            y, self.cache, _ = self.enc.forward_chunk(frames, self.offset, self.need, cache, empty)
            self.offset += y.size(1)
            if self.cache.size(-2) == self.need:
                self._capture(frames)
            return y
        self.x.copy_(frames)
        self.pos.copy_(self.enc.embed.position_encoding(offset=self.offset - self.need, size=self.need + self.chunk))
        if not self.relative:
            self.abs.copy_(self._abs_rows(frames.size(0), dev))
        self.graph.replay()
        self.offset += self.chunk
        return self.y

    def _capture(self, frames):
        enc, dev = self.enc, frames.device
        empty = torch.zeros((0, 0, 0, 0), device=dev)
        self.x = frames.clone()
        self.kv = self.cache                                       # the eager step's own result becomes the static cache (no second copy is kept)
        self.pos =enc.embed.position_encoding(offset=self.offset - self.need, size=self.need + self.chunk).clone()
        # absolute encoding (use_relative=False): the table rows added to the chunk live in a static buffer too -- sliced at `offset`
        # inside the captured region they would be frozen at the capture step's offset
        self.abs = None if self.relative else self._abs_rows(frames.size(0), dev).clone()

        def run():
            y, new_kv, _ = enc.forward_chunk(self.x, self.offset, self.need, self.kv, empty, pos_rows=self.pos, abs_rows=self.abs)
            self.kv.copy_(new_kv)
            return y
        self.graph, self.y = packing.capture_step(run, dev, [self.kv])       # warm-up and capture advanced the static cache: it is put back
        _weights_moved(self)


class StreamingBatch:
    """B independent streams, each at ITS OWN position, advanced together one chunk per step (BASELINE config 5:
    64 streams, chunk 16, cached left context) -- what the reference cannot do: its forward_chunk serves one stream at a time
    (encoder.py:78-123: the positional view fails at batch > 1) and rebuilds the attention cache with cat + slice every step (:117).

      * per-stream state lives on the device: `offsets` int32 [B] (encoder frames consumed) and, per layer, a K/V RING buffer
        f32 [B,H,need+chunk,2dk] -- frame f in slot f mod ring_T; a step writes its `chunk` new frames and moves nothing;
      * a step is: front-end on the B windows, cfm_stream_prep (slot mask + positional rows per stream from `offsets`), one projection
        of those rows for all layers, the blocks with attention over the ring under the slot mask, cfm_stream_advance;
      * no host-side scalar enters the step, so it is captured ONCE as a HIP graph and replayed (graph=True);
      * item b of the output equals the reference's batch-1 forward_chunk on stream b with its own cache and offset (tests: against
        the CPU oracle looped per stream) to the precision mode's tolerance -- not bit for bit, the softmax sums run in slot order;
      * causal_conv=True is the OPT-IN extension (not in the reference, which has no causal convolution and ignores cnn_cache):
        every block's depthwise conv becomes causal with a (K-1)-frame left context per stream.  Off = the reference's arithmetic.

    step(frames (B, (chunk-1)*4+7, F)) -> (B, chunk, D) in a buffer the next step overwrites.  reset(streams) starts new utterances.
    input_buffer() / step_resident(): the same step on windows a producer wrote into the step's own input buffer.

    step(frames, frame_lens) / step_resident(frame_lens): PER-STREAM window lengths -- a list or a tensor of B entries, stream b's window holds
    n_b valid feature frames, left-aligned, 0 <= n_b <= window (what lies behind them is ignored, whatever it holds).  This is the reference's short
    final chunk (its streaming loop ends an utterance on a window of 7 .. window-1 frames), at any step and per stream:
      * stream b has c_b = ((n_b - 1) // 2 - 1) // 2 encoder frames (0 for n_b < 7), computed on the device; `out_lens` (int32 [B], device) holds
        the last step's c_b;
      * rows [0, c_b) of item b equal the reference's batch-1 forward_chunk on window[b:b+1, :n_b] with stream b's cache and offset; rows >= c_b are
        exactly zero;
      * the stream's state advances by c_b frames: only they enter the mask, the K/V ring, the causal conv cache and the offset;
      * c_b = 0 leaves every piece of the stream's state untouched: an idle step (n_b = 0) is invisible and needs no reset;
      * the lengths live in a persistent device buffer that the captured graph reads, so ONE graph serves all lengths; the first step with lengths
        captures the length-aware form (once), which every later step -- with or without lengths -- replays.  Without lengths ever given, the step,
        its launches and its bits are what they were."""

    def __init__(self, encoder, streams, decoding_chunk_size, num_decoding_left_chunks, causal_conv=False, graph=True):
        if num_decoding_left_chunks < 0:
            raise ValueError("StreamingBatch needs a bounded left context (num_decoding_left_chunks >= 0)")
        if encoder.training:
            raise NotImplementedError("StreamingBatch: streaming is inference-only; call encoder.eval()")
        self.enc, self.B = encoder, int(streams)
        self.chunk, self.need = int(decoding_chunk_size), int(decoding_chunk_size) * int(num_decoding_left_chunks)
        self.ring_T = self.need + self.chunk
        self.window = (self.chunk - 1) * 4 + 7
        self.relative = isinstance(encoder.position_encoding, RelativePositionalEncoding)
        blk = encoder.encoders[0]
        L, H, D, K = len(encoder.encoders), blk.num_heads, encoder.encoder_dim, blk.kernel_size
        dev = next(encoder.parameters()).device
        cfm.require_hip(next(encoder.parameters()))
        self.dev = dev
        self.offsets = torch.zeros((self.B,), dtype=torch.int32, device=dev)
        self.kv = torch.zeros((L, self.B, H, self.ring_T, 2 * (D // H)), dtype=torch.float32, device=dev)      # zero: masked slots must stay finite
        self.slot_mask = torch.zeros((self.B, 1, self.ring_T), dtype=torch.uint8, device=dev)
        self.pos_rows = torch.zeros((self.B * self.ring_T, 1, D), dtype=torch.float32, device=dev)
        self.abs_rows = None if self.relative else torch.zeros((self.B, 1, D), dtype=torch.float32, device=dev)
        self.causal = bool(causal_conv)
        self.conv = torch.zeros((L, self.B, K - 1, D), dtype=torch.float32, device=dev) if self.causal else None
        self.pe = encoder.position_encoding.pe.reshape(-1, D).to(device=dev, dtype=torch.float32).contiguous()
        # host mirror of an UPPER BOUND of `offsets` (every step advances every stream by at most `chunk` -- by c_b <= chunk with frame_lens; reset() zeroes): lets step() see, without a
        # device sync, that a stream is about to read past the sinusoid table -- the reference's pe[offset:offset+size] comes back short there
        # and fails (attention.py:25-29; max_len = 5000 encoder frames = 200 s of audio); a long-lived stream here gets the table EXTENDED
        # with the same formula instead of wrong rows (cfm_stream_prep used to clamp to the last row, silently)
        self._host_off = [0] * self.B
        self.x = None
        self.use_graph, self.graph, self.y, self._sig = bool(graph), None, None, None
        self.steps = 0
        # per-stream window lengths: None until a step is given frame_lens, from then on the step is the length-aware one (whole windows = `window`)
        self.frame_lens = None
        self.out_lens = None

    def reset(self, streams=None):
        """start new utterances on the given streams (all by default): position 0, empty left context."""
        streams = None if streams is None else list(streams)
        idx = packing.stream_index(streams, self.dev)
        for b in range(self.B) if streams is None else streams:
            self._host_off[b] = 0
        self.offsets[idx] = 0
        if self.conv is not None:
            self.conv[:, idx] = 0

    def _grow_table(self, rows_needed):
        """Append sinusoid rows [len, new_len) -- the reference's formula (attention.py:12-16 / :109-115 incl. the absolute table's fp16
        rounding), existing rows untouched -- and drop the captured graph (it holds the old table's address)."""
        from attention import _sinusoid_table
        have = self.pe.size(0)
        new_len = max(2 * have, rows_needed)
        full = _sinusoid_table(new_len, self.pe.size(1), type(self.enc.position_encoding)._table_dtype).reshape(new_len, -1)
        self.pe = torch.cat([self.pe, full[have:].to(device=self.dev, dtype=torch.float32)]).contiguous()
        self.graph = None

    def _step_impl(self):
        enc = self.enc
        inputs, cmvn = enc._cmvn_args(self.x)
        x = enc.embed.embed_frames(inputs, cmvn)
        cfm.stream_prep(self.offsets, self.chunk, self.need, self.ring_T, self.pe, self.slot_mask, self.pos_rows, self.abs_rows,
                        frame_lens=self.frame_lens, out_lens=self.out_lens)
        if self.relative:
            x, _ = enc.position_encoding(x, 0)
        else:
            x, _ = enc.position_encoding(x, 0, rows=self.abs_rows)
        proj = enc._project_positions(self.pos_rows, x)
        y, _ = enc._run_blocks(x, self.slot_mask.view(torch.bool), self.pos_rows, None, None, 0, proj=proj, ring=(self.kv, self.offsets), conv=self.conv, streaming=True,
                               stream_len=self.out_lens, causal=self.causal)
        if self.out_lens is None:
            cfm.stream_advance(self.offsets, self.chunk)
        else:
            cfm.stream_advance(self.offsets, self.chunk, lens=self.out_lens, y=y)     # ... and zeroes the rows past each stream's c_b
        return y

    def step(self, frames, frame_lens=None):
        if tuple(frames.shape[:2]) != (self.B, self.window):
            raise ValueError("StreamingBatch.step wants (%d, %d, F) frames, got %s" % (self.B, self.window, tuple(frames.shape)))
        cfm.require_hip(frames)
        self._read_lens(frame_lens)                                      # before the input buffer is touched
        self.input_buffer(frames.shape[2]).copy_(frames)
        return self.step_resident(frame_lens)

    def _read_lens(self, frame_lens, name="frame_lens", buf=None):
        """packing.stream_lens with a window's rules (strict: a bad host value raises); buf None: checked only.  -> the host's list | None."""
        return packing.stream_lens("StreamingBatch", name, self.B, frame_lens, self.window, buf, strict=True)

    def _set_lens(self, frame_lens):
        """Copy this step's lengths into the persistent device buffer the (captured) step reads; the first call switches to the length-aware step."""
        if self.frame_lens is None:
            if frame_lens is None:
                return
            self.frame_lens = torch.full((self.B,), self.window, dtype=torch.int32, device=self.dev)
            self.out_lens = torch.zeros((self.B,), dtype=torch.int32, device=self.dev)
            self.graph = None                                             # captured without lengths: re-capture, once
        self._read_lens(frame_lens, buf=self.frame_lens)

    def input_buffer(self, num_features=None):
        """The (B, window, F) f32 buffer the step reads.  A producer on the same stream (fbank.StreamingFbank) writes the windows here and calls
        step_resident(): no feature tensor and no copy in between."""
        if self.x is None:
            if num_features is None:
                raise ValueError("StreamingBatch.input_buffer: the feature size is not known before the first step")
            self.x = torch.empty((self.B, self.window, int(num_features)), dtype=torch.float32, device=self.dev)
        elif num_features is not None and int(num_features) != self.x.shape[2]:
            raise ValueError("StreamingBatch: %d features per frame, the stream was started with %d" % (num_features, self.x.shape[2]))
        return self.x

    def step_resident(self, frame_lens=None, host_lens=None):
        """step() on what input_buffer() holds.  host_lens: what the host knows of a DEVICE frame_lens (B window lengths, a producer's host mirror):
        the offset bound then advances by each stream's own c_b instead of `chunk`, so that idle steps do not bring the table growth forward."""
        self.input_buffer()
        self._read_lens(frame_lens)                                       # both checked before anything is touched
        host_lens = None if host_lens is None else self._read_lens(host_lens, "host_lens")
        self._set_lens(frame_lens)
        self.steps += 1
        adv = [self.chunk] * self.B if host_lens is None else [((n - 1) // 2 - 1) // 2 if n >= 7 else 0 for n in host_lens]
        need = max(o + a for o, a in zip(self._host_off, adv))
        if need > self.pe.size(0):
            self._grow_table(need)
        self._host_off = [o + a for o, a in zip(self._host_off, adv)]
        with torch.no_grad():
            if not self.use_graph:
                return self._step_impl()
            if self.graph is not None and _weights_moved(self):
                self.graph = None                                         # weights changed under the captured graph
            if self.graph is None:
                y = self._step_impl()                                     # this step runs eagerly (it also packs the weights)
                # the warm-up's advance is put back (ring slots rewritten: same data), and out_lens -- this step's c_b -- with it; the length-aware
                # warm-up runs every stream idle (frame_lens zeroed): it touches no state at all
                self.graph, self.y = packing.capture_step(self._step_impl, self.dev, [self.offsets, self.conv, self.frame_lens, self.out_lens],
                                                          idle=None if self.frame_lens is None else self.frame_lens.zero_)
                _weights_moved(self)
                return y
            self.graph.replay()
            return self.y
