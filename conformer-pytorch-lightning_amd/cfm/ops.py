"""Tensor-level wrappers over the C ABI.  Each function validates device / dtype / layout on the host,
allocates its output with torch.empty on the same device, and enqueues on the current HIP stream."""
import ctypes

import torch

import cfm as _c

__all__ = ["dec_step_attn", "dec_beam_prune", "ctc_logprob_t", "ctc_prefix_score", "ctc_prefix_advance", "rescore_prep", "token_logprob", "rescore_combine", "lsm_loss", "lsm_grad", "lsm_reduce", "lstm_forward", "lstm_backward", "fbank", "fbank_stream", "fbank_stream_ragged", "resample", "resample_stream", "resample_group", "spec_augment", "stream_prep", "stream_advance", "dwconv_causal_bn_silu", "conv_cache_update", "dropout_rows", "dropout_mask", "set_deterministic", "gemm_tn", "gemm_tn_group", "layernorm_bwd", "glu_bwd", "dwconv_bn_train", "dwconv_bn_train_bwd", "dwconv_bn_train_groups", "dwconv_bn_train_bwd_groups", "col2im_relu_bwd", "conv1_wgrad", "attention_bwd", "attention_group", "attention_bwd_group",
           "ctc_nll_train_groups", "ctc_grad", "rnnt_nll", "rnnt_grad", "joint_act_bwd", "rnnt_nll_packed", "rnnt_align", "rnnt_align_packed", "joint_act_packed", "joint_act_packed_bwd", "ffn_split", "adam_step", "adam_clip_step", "sumsq", "scratch_stats",
           "gemm", "ffn_fused", "ffn_fused_supported", "rowchain", "rowchain_supported", "rowchain_pair_supported", "layernorm", "attention", "kv_cache_pack", "dwconv_bn_silu", "conv1_relu", "conv1_relu_mma_supported", "conv12_relu", "conv12_supported", "ctc_nll", "ctc_topk", "ctc_greedy", "ctc_greedy_state", "ctc_prefix_beam", "ctc_align", "edit_distance", "joint_act", "valid_mask", "chunk_mask",
           "attn_mask_combine", "cast", "add_rows", "scratch", "prof_enable", "prof_reset", "prof_table", "as_u8_mask"]


def _rows2d(t, name):
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError("cfm.%s: expected a 2-D tensor with unit inner stride, got shape %s strides %s" % (name, tuple(t.shape), t.stride()))
    return t


def _dense(name, **tensors):
    """Operands whose layout the C ABI cannot carry (no stride field for them): anything but a dense tensor would be read or written with
    the wrong stride, silently -- so it is an argument error here, before any launch."""
    for k, t in tensors.items():
        if t is not None and not t.is_contiguous():
            raise ValueError("cfm.%s: %s must be contiguous (the C ABI has no stride for it), got shape %s strides %s" % (name, k, tuple(t.shape), t.stride()))


_F32, _I32, _I64 = torch.float32, torch.int32, torch.int64


def _layout(op, _hint="", **specs):
    """What a group of dense arguments must be, said once: name=(tensor, dtype, extent).  dtype: a torch.dtype, a tuple of them, or None (any).
    extent: an int (that many elements whatever the shape: a [B,1] lengths tensor is an int32 [B]), a shape tuple (that rank and those sizes, None
    for an axis of any size) or None (any).  name=None is an optional argument that was not given (_opt); a tensor that is None is a required one
    that is missing.  Always contiguous, as _dense: the C ABI has no stride for these operands.  A pure function of tensor metadata (no device,
    no library); _hint is appended to the message (what the group is, or the phrase a caller knows the failure by)."""
    for name, spec in specs.items():
        if spec is None:
            continue
        t, dtype, extent = spec
        dtypes = dtype if isinstance(dtype, tuple) else (dtype,)
        if extent is None:
            fits, size = t is not None, ""
        elif isinstance(extent, int):
            fits, size = t is not None and t.numel() == extent, " of %d elements" % extent
        else:
            fits = t is not None and t.dim() == len(extent) and all(w is None or w == g for w, g in zip(extent, t.shape))
            size = " [%s]" % ", ".join("*" if w is None else str(w) for w in extent)
        if not fits or not t.is_contiguous() or (dtype is not None and t.dtype not in dtypes):
            raise ValueError("cfm.%s: %s must be contiguous%s%s (the C ABI has no stride for it), got %s%s" % (
                op, name, "" if dtype is None else " " + " or ".join(str(d)[6:] for d in dtypes), size,
                "None" if t is None else "%s %s strides %s" % (str(t.dtype)[6:], tuple(t.shape), t.stride()), _hint and ": " + _hint))


def _want(op, _hint="", **specs):
    """_layout behind the device check: a tensor that is not on the GPU is cfm.require_hip's RuntimeError before any layout complaint."""
    _c.require_hip(*[s[0] for s in specs.values() if s is not None])
    _layout(op, _hint, **specs)


def _opt(t, *spec):
    return None if t is None else (t,) + spec


def _i32(n, **tensors):
    """int32 [n]: lengths, offsets, flags per stream or per utterance -- by element count (n an int) or as the exact shape (n a tuple)."""
    return {k: (t, _I32, n) for k, t in tensors.items()}


def _strides_match(name, what, t, sb, st):
    """An operand addressed through explicit (batch, time) element strides: where the tensor itself has those axes, they must agree with
    what the call passes -- the C ABI reads the numbers, not the tensor."""
    if t is None:
        return
    if t.dim() not in (2, 3):                 # [rows, cols] or [B, T, cols]; other ranks say nothing about (batch, time)
        bad = t.stride(-1) != 1
    else:
        bad = t.stride(-1) != 1 or (t.size(-2) > 1 and t.stride(-2) != st) or (t.dim() == 3 and t.size(0) > 1 and t.stride(0) != sb)
    if bad:
        raise ValueError("cfm.%s: %s has strides %s but the call passes (batch %d, time %d) with unit inner stride" % (name, what, t.stride(), sb, st))


# A grow-only arena of reusable device buffers (workspace owned by the extension side of the boundary), keyed per
# (device, STREAM): two streams never share a scratch buffer, so forwards running concurrently on one device cannot overwrite each
# other's xn / hid / qkv.  A buffer that has been handed out is NEVER released: when a larger one is needed the old block is retired,
# not freed -- a captured HIP graph (bench.py, StreamingSession) may still hold its address.  Blocks grow by at least 1.5x, so the
# retired list stays short.
_arena = {}
_retired = []


def scratch(tag, numel, dtype, device):
    device = torch.device(device)
    key = (tag, dtype, device, torch.cuda.current_stream(device).cuda_stream)
    buf = _arena.get(key)
    if buf is None or buf.numel() < numel:
        want = max(int(numel), 1) if buf is None else max(int(numel), buf.numel() * 3 // 2)
        if buf is not None:
            _retired.append(buf)
        buf = torch.empty(want, dtype=dtype, device=device)
        _arena[key] = buf
    return buf[:numel]


def scratch_stats():
    """(live blocks, retired blocks, bytes held) -- for tests and leak hunting."""
    held = sum(b.numel() * b.element_size() for b in list(_arena.values()) + _retired)
    return len(_arena), len(_retired), held


def gemm(a, w, bias=None, w_lo=None, out=None, out_dtype=None, act=_c.ACT_NONE, residual=None, alpha=1.0, row_mask=None,
         mask_mode=0, conv=None, tile=0, n_out=None, pre_out=None, aux=None, drop=None, drop2=None, row_len=None, row_T=0):
    """out = epilogue(a[M,K] . w[N,K]^T); see include/cfm.h cfm_gemm.  conv=(C,T1,F1,T2,F2,M) selects the implicit
    3x3/stride-2 convolution over a channels-last image `a` of shape [B,T1,F1,C].  row_len (int32 [M/row_T], device) with row_T: the
    ragged-batch select behind the GLU (cfm_gemm_desc.row_len)."""
    _c.require_hip(a, w, bias, w_lo, out, residual, row_mask, row_len)
    w = _rows2d(w, "gemm(w)")
    N, K = w.shape
    if w.stride(0) != K:                         # cfm_gemm_desc has no row stride for W: a view wbuf[:, :K] would be read with stride K
        raise ValueError("cfm.gemm: w must be dense [N,K] (cfm_gemm_desc carries no row stride for W), got shape %s strides %s" % (tuple(w.shape), w.stride()))
    d = _c.GemmDesc()
    if conv is None:
        a = _rows2d(a, "gemm(a)")
        M = a.shape[0]
        if a.shape[1] != K:
            raise ValueError("cfm.gemm: a is %s but w is %s" % (tuple(a.shape), tuple(w.shape)))
        d.lda = a.stride(0)
    else:
        C, T1, F1, T2, F2, M = conv
        if not a.is_contiguous():
            raise ValueError("cfm.gemm(conv): image must be contiguous channels-last [B,T1,F1,C]")
        d.conv_C, d.conv_T1, d.conv_F1, d.conv_T2, d.conv_F2 = C, T1, F1, T2, F2
        d.lda = 0
    cols = N // 2 if act == _c.ACT_GLU else N
    if out is None:
        odt = out_dtype if out_dtype is not None else (residual.dtype if residual is not None else torch.float32)
        out = torch.empty((M, cols), dtype=odt, device=a.device)
    else:
        out = _rows2d(out, "gemm(out)")
        if out.shape[0] != M or out.shape[1] != cols:
            raise ValueError("cfm.gemm: out is %s, expected (%d,%d)" % (tuple(out.shape), M, cols))
    if residual is not None:
        residual = _rows2d(residual, "gemm(residual)")
        if residual.dtype != torch.float32 or out.dtype != torch.float32 or tuple(residual.shape) != (M, cols):
            raise ValueError("cfm.gemm: residual accumulate needs f32 residual/out of shape (%d,%d)" % (M, cols))
        d.ldr = residual.stride(0)
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() != N or not bias.is_contiguous()):
        raise ValueError("cfm.gemm: bias must be contiguous f32 [N]")
    if row_mask is not None and (row_mask.dtype != torch.uint8 or row_mask.numel() != M or not row_mask.is_contiguous()):
        raise ValueError("cfm.gemm: row_mask must be contiguous uint8 [M]")
    if w_lo is not None and (w_lo.shape != w.shape or w_lo.dtype != w.dtype or not w_lo.is_contiguous()):
        raise ValueError("cfm.gemm: w_lo must match w")
    if pre_out is not None:                      # training: acc + bias before the activation, all N columns
        _c.require_hip(pre_out)
        pre_out = _rows2d(pre_out, "gemm(pre_out)")
        if tuple(pre_out.shape) != (M, N):
            raise ValueError("cfm.gemm: pre_out is %s, expected (%d,%d)" % (tuple(pre_out.shape), M, N))
        d.C_pre, d.ld_pre, d.pre_dtype = _c.ptr(pre_out), pre_out.stride(0), _c.dt_code(pre_out)
    if aux is not None:                          # backward epilogues (ACT_DSILU / ACT_DRELU): the forward pre-activation / output
        _c.require_hip(aux)
        aux = _rows2d(aux, "gemm(aux)")
        if tuple(aux.shape) != (M, N):
            raise ValueError("cfm.gemm: aux is %s, expected (%d,%d)" % (tuple(aux.shape), M, N))
        d.aux, d.ld_aux, d.aux_dtype = _c.ptr(aux), aux.stride(0), _c.dt_code(aux)
    if drop is not None and drop[0] > 0.0:       # (p, seed): output dropout in the epilogue (train mode)
        d.drop_p, d.drop_seed = float(drop[0]), int(drop[1]) & 0xFFFFFFFF
        if drop2 is not None and drop2[0] > 0.0:
            d.drop2_p, d.drop2_seed = float(drop2[0]), int(drop2[1]) & 0xFFFFFFFF
    if row_len is not None:                      # M % row_T, mask_mode and the GLU requirement are the ABI's own checks
        _dense("gemm", row_len=row_len)
        if row_len.dtype != torch.int32:
            raise ValueError("cfm.gemm: row_len must be int32, got %s" % row_len.dtype)
        if row_T > 0 and M % row_T == 0 and row_len.numel() < M // row_T:      # every other misuse is the ABI's own argument error
            raise ValueError("cfm.gemm: row_len has %d entries, %d rows of %d need %d" % (row_len.numel(), M, row_T, M // row_T))
        d.row_len = _c.ptr(row_len)
    d.row_T = int(row_T)
    d.A, d.W, d.W_lo, d.bias, d.residual, d.row_mask, d.C = _c.ptr(a), _c.ptr(w), _c.ptr(w_lo), _c.ptr(bias), _c.ptr(residual), _c.ptr(row_mask), _c.ptr(out)
    d.ldc = out.stride(0)
    d.M, d.N, d.K = M, N, K
    d.a_dtype, d.w_dtype, d.c_dtype = _c.dt_code(a), _c.dt_code(w), _c.dt_code(out)
    d.act, d.alpha, d.tile, d.mask_mode = act, alpha, tile, mask_mode
    _c.call("cfm_gemm", ctypes.byref(d))
    return out


def ffn_fused_supported(D, FF, prec):
    return (not prec.split) and D in (144, 256) and FF % 32 == 0 and FF <= 2048


def ffn_fused(x, w1f, w2f, b1, b2, FF, act=_c.ACT_SILU, ln=None, alpha=1.0, add_x=False, ln1=None, ln2=None, out_f32=None,
              want_f32=True, out16_dtype=None, eps=1e-5):
    """One-launch feed-forward block (include/cfm.h cfm_ffn_fused).  x f32 [M,D]; ln/ln1/ln2 are (gain, bias) pairs or None.
    Returns (out_f32 | None, out16 | None)."""
    _c.require_hip(x, w1f, w2f, b1, b2, out_f32)
    x = _rows2d(x, "ffn_fused(x)")
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("cfm.ffn_fused: x must be contiguous float32 [M,D]")
    M, D = x.shape
    _dense("ffn_fused", w1f=w1f, w2f=w2f, b1=b1, b2=b2, out_f32=out_f32, **{n + "_" + s: t for n, pr in (("ln", ln), ("ln1", ln1), ("ln2", ln2)) if pr is not None
                                                                            for s, t in zip("gb", pr)})
    if out_f32 is not None and (out_f32.dtype != torch.float32 or tuple(out_f32.shape) != (M, D)):
        raise ValueError("cfm.ffn_fused: out_f32 must be float32 (%d,%d)" % (M, D))
    d = _c.FfnDesc()
    d.x, d.w1f, d.w2f, d.b1, d.b2 = _c.ptr(x), _c.ptr(w1f), _c.ptr(w2f), _c.ptr(b1), _c.ptr(b2)
    for name, pair in (("ln", ln), ("ln1", ln1), ("ln2", ln2)):
        if pair is not None:
            setattr(d, name + "_g", _c.ptr(pair[0]))
            setattr(d, name + "_b", _c.ptr(pair[1]))
    if want_f32 and out_f32 is None:
        out_f32 = torch.empty((M, D), dtype=torch.float32, device=x.device)
    out16 = torch.empty((M, D), dtype=out16_dtype, device=x.device) if out16_dtype is not None else None
    d.out_f32, d.out16 = _c.ptr(out_f32), _c.ptr(out16)
    d.M, d.D, d.FF = M, D, FF
    d.w_dtype = _c.dt_code(w1f)
    d.out16_dtype = _c.dt_code(out16) if out16 is not None else 0
    d.act, d.add_x, d.alpha, d.eps = act, 1 if add_x else 0, alpha, eps
    _c.call("cfm_ffn_fused", ctypes.byref(d))
    return out_f32, out16


def rowchain_supported(D, FF, prec):
    return (not prec.split) and bool(_c.lib().cfm_rowchain_supported(D, FF))


def rowchain_pair_supported(D, FF, prec):
    """The feed-forward split over workgroup pairs (cfm_rowchain_desc.psum_out / psum_in, D = 512)."""
    return (not prec.split) and bool(_c.lib().cfm_rowchain_pair_supported(D, FF))


def ffn_split(x, w_code, mode, psum=None, psum_b2=None, psum_alpha=1.0, ln1=None, ln2=None, rows_out=None, rows2_out=None, ln=None, w1=None, b1=None,
              n1=0, act=_c.ACT_NONE, w2=None, psum_out=None, out16=None, eps=1e-5, ring=None):
    """include/cfm.h cfm_ffn_split: the rows stage (optional reduce of partial slabs psum [G,M,D] + residual x, LN1, rows_out) followed by nothing
    (mode 0: + LN2 -> rows2_out), a projection (mode 1: out16 [M,n1]) or a feed-forward that leaves partial slabs (mode 2: psum_out [n1/256,M,D])."""
    _c.require_hip(x, psum, psum_b2, rows_out, rows2_out, w1, b1, w2, psum_out, out16)
    x = _rows2d(x, "ffn_split(x)")
    M, D = x.shape
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("cfm.ffn_split: x must be contiguous float32 rows")
    _dense("ffn_split", psum_b2=psum_b2, rows_out=rows_out, rows2_out=rows2_out, w1=w1, b1=b1, w2=w2, psum_out=psum_out,
           ring_kv=ring[0] if ring is not None else None, ring_offsets=ring[1] if ring is not None else None, **{n + "_" + sfx: t for n, pr in (("ln", ln), ("ln1", ln1), ("ln2", ln2)) if pr is not None for sfx, t in zip("gb", pr)})
    if ring is not None and (ring[0].dtype != torch.float32 or ring[0].dim() != 4 or ring[1].dtype != torch.int32):
        raise ValueError("cfm.ffn_split: ring is (kv float32 [B,H,ring_T,2dk], offsets int32 [B], frames per stream)")
    for name, t in (("rows_out", rows_out), ("rows2_out", rows2_out)):
        if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != (M, D)):
            raise ValueError("cfm.ffn_split: %s must be float32 (%d,%d)" % (name, M, D))
    if out16 is not None and (out16.dim() != 2 or out16.stride(1) != 1 or out16.shape[0] != M):
        raise ValueError("cfm.ffn_split: out16 must be [M, n1] with unit inner stride")
    d = _c.FfnSplitDesc()
    d.x, d.M, d.D, d.mode, d.w_dtype, d.eps = x.data_ptr(), M, D, mode, w_code, eps
    if psum is not None:
        if psum.dtype != torch.float32 or psum.dim() != 3 or tuple(psum.shape[1:]) != (M, D) or not psum.is_contiguous():
            raise ValueError("cfm.ffn_split: psum must be contiguous float32 [G, M, D]")
        d.psum, d.psum_b2, d.psum_splits, d.psum_alpha = psum.data_ptr(), _c.ptr(psum_b2), psum.shape[0], psum_alpha
    for name, pair in (("ln1", ln1), ("ln2", ln2), ("ln", ln)):
        if pair is not None:
            setattr(d, name + "_g", pair[0].data_ptr())
            setattr(d, name + "_b", pair[1].data_ptr())
    d.rows_out, d.rows2_out = _c.ptr(rows_out), _c.ptr(rows2_out)
    d.w1, d.b1, d.N1, d.act, d.w2, d.psum_out = _c.ptr(w1), _c.ptr(b1), n1, act, _c.ptr(w2), _c.ptr(psum_out)
    if out16 is not None:
        d.out16, d.ldo = out16.data_ptr(), out16.stride(0)
    if ring is not None:                                  # (kv f32 [B,H,ring_T,2dk], offsets int32 [B], frames per stream): mode 1 as the q|k|v projection
        kv, offs, tq = ring[:3]                           # an optional fourth entry: int32 [B], only rows t < lens[b] go into the ring (cfm.h ring_len)
        _c.require_hip(kv, offs)
        d.kv_ring, d.ring_offsets, d.ring_T, d.ring_H, d.ring_Tq = kv.data_ptr(), offs.data_ptr(), kv.shape[2], kv.shape[1], tq
        if len(ring) > 3 and ring[3] is not None:
            _want("ffn_split", ring_len=(ring[3], _I32, offs.numel()))
            d.ring_len = ring[3].data_ptr()
    _c.call("cfm_ffn_split", ctypes.byref(d))


def rowchain(M, D, w_code, x=None, head=None, ln=None, ln_mask=None, ffn=None, alpha=1.0, ln1=None, ln2=None, out_f32=None, out16=None,
             tail=None, eps=1e-5, dw=None):
    """One-launch row-local chain (include/cfm.h cfm_rowchain).
    dw = (taps f32 [D,15], bias, bn_scale, bn_shift, T): depthwise conv + BatchNorm + SiLU applied to the head input first;
    head = (a16 [M,D], w_frag, bias, residual f32 [M,D], out_mask u8 [M] | None);  ffn = (w1f, w2n, b1, b2, FF) with
    w1f = pack_frag_major(W1), w2n = pack_frag_major(W2) (natural k order, NOT ffn_fused's permuted w2f);
    tail = (w_frag, bias, N, glu, out 16-bit [M, N or N/2]);  ln/ln1/ln2 = (gain, bias)."""
    _dense("rowchain", x=x, out_f32=out_f32, out16=out16, ln_mask=ln_mask, **{n + "_" + sfx: t for n, pr in (("ln", ln), ("ln1", ln1), ("ln2", ln2)) if pr is not None for sfx, t in zip("gb", pr)})
    if head is not None:
        _dense("rowchain", head_a=head[0], head_w=head[1], head_b=head[2], head_res=head[3], head_mask=head[4])
    if tail is not None:
        _dense("rowchain", tail_w=tail[0], tail_b=tail[1], tail_out=tail[4])
    if ffn is not None:
        _dense("rowchain", w1f=ffn[0], w2n=ffn[1], b1=ffn[2], b2=ffn[3])
    if dw is not None:
        _dense("rowchain", dw_w=dw[0], dw_b=dw[1], dw_scale=dw[2], dw_shift=dw[3])
    d = _c.RowChainDesc()
    keep = [x, out_f32, out16, ln_mask]
    d.x, d.out_f32, d.out16, d.ln_mask = _c.ptr(x), _c.ptr(out_f32), _c.ptr(out16), _c.ptr(ln_mask)
    if head is not None:
        a16, hw, hb, res, hm = head
        _c.require_hip(a16, hw, hb, res, hm)
        d.head_a, d.head_w, d.head_b, d.head_res, d.head_mask = _c.ptr(a16), _c.ptr(hw), _c.ptr(hb), _c.ptr(res), _c.ptr(hm)
        keep += list(head)
    for name, pair in (("ln", ln), ("ln1", ln1), ("ln2", ln2)):
        if pair is not None:
            setattr(d, name + "_g", _c.ptr(pair[0]))
            setattr(d, name + "_b", _c.ptr(pair[1]))
    if ffn is not None:
        d.w1f, d.w2n, d.b1, d.b2, d.FF = _c.ptr(ffn[0]), _c.ptr(ffn[1]), _c.ptr(ffn[2]), _c.ptr(ffn[3]), ffn[4]
    if tail is not None:
        d.tail_w, d.tail_b, d.tail_N, d.tail_glu, d.tail_out = _c.ptr(tail[0]), _c.ptr(tail[1]), tail[2], 1 if tail[3] else 0, _c.ptr(tail[4])
    if dw is not None:
        _c.require_hip(*dw[:4])
        d.dw_w, d.dw_b, d.dw_scale, d.dw_shift, d.dw_T, d.dw_K = _c.ptr(dw[0]), _c.ptr(dw[1]), _c.ptr(dw[2]), _c.ptr(dw[3]), dw[4], dw[0].shape[1]
    _c.require_hip(x, out_f32, out16)
    d.M, d.D, d.w_dtype, d.alpha, d.eps = M, D, w_code, alpha, eps
    _c.call("cfm_rowchain", ctypes.byref(d))


def layernorm(x, g1, b1, out1=None, out1_dtype=None, g2=None, b2=None, out2=None, out2_dtype=None, row_mask=None, eps=1e-5,
              want1=True):
    """y1 = LN(x;g1,b1) -> out1 (if want1);  y2 = LN(y1;g2,b2) (or y1) masked -> out2 (if out2/out2_dtype given)."""
    _c.require_hip(x, g1, b1, g2, b2, out1, out2, row_mask)
    x = _rows2d(x, "layernorm(x)")
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("cfm.layernorm: x must be contiguous float32 [M,D]")
    M, D = x.shape
    _dense("layernorm", g1=g1, b1=b1, g2=g2, b2=b2, row_mask=row_mask)
    if want1 and out1 is None:
        out1 = torch.empty((M, D), dtype=out1_dtype or torch.float32, device=x.device)
    if out2 is None and out2_dtype is not None:
        out2 = torch.empty((M, D), dtype=out2_dtype, device=x.device)
    for o in (out1, out2):
        if o is not None and (tuple(o.shape) != (M, D) or not o.is_contiguous()):
            raise ValueError("cfm.layernorm: outputs must be contiguous [M,D]")
    _c.call("cfm_layernorm", _c.ptr(x), _c.ptr(g1), _c.ptr(b1), _c.ptr(out1), _c.dt_code(out1) if out1 is not None else 0,
            _c.ptr(g2), _c.ptr(b2), _c.ptr(out2), _c.dt_code(out2) if out2 is not None else 0,
            _c.ptr(row_mask), eps, M, D)
    return out1, out2


def as_u8_mask(mask):
    """bool / numeric mask -> contiguous uint8 0/1 view (no copy when already a contiguous bool tensor)."""
    if mask.dtype == torch.bool:
        return mask.contiguous().view(torch.uint8)
    if mask.dtype == torch.uint8:
        return mask.contiguous()
    return (mask != 0).contiguous().view(torch.uint8)


def _attn_fill(d, who, q, k, v, B, H, Tq, Tk, dk, q_str, k_str, v_str, out, p=None, p_str=(0, 0), bias_u=None, bias_v=None, mask=None,
               mask_str=(0, 0), mma_code=_c.BF16, split=False, scale=None, lse=None, drop=None):
    """Checks one attention problem and fills its cfm_attn_desc: the single and the grouped wrapper share it, so the two cannot drift."""
    _c.require_hip(q, k, v, p, out, mask, bias_u, bias_v, lse)
    if lse is not None and (lse.dtype != torch.float32 or lse.numel() != B * H * Tq or not lse.is_contiguous()):
        raise ValueError("cfm.%s: lse must be contiguous float32 [B,H,Tq]" % who)
    for what, t, strides in (("q", q, q_str), ("k", k, k_str), ("v", v, v_str)):
        # [rows, cols] and [B, T, cols] tensors carry the strides the call passes beside them; p and mask are taken on the numbers alone (their
        # rank does not say which axis is batch: a [B, Tk] pad mask and a [R, D] row matrix of positions are both 2-D)
        _strides_match(who, what, t, strides[0], strides[1])
    _dense(who, out=out, bias_u=bias_u, bias_v=bias_v)               # out is [B,Tq,H*dk] row-major: cfm_attn_desc has no stride for it
    if out.numel() != B * Tq * H * dk:
        raise ValueError("cfm.%s: out must hold [B,Tq,H*dk] = %d elements, got %s" % (who, B * Tq * H * dk, tuple(out.shape)))
    d.q, d.k, d.v, d.p, d.out = _c.ptr(q), _c.ptr(k), _c.ptr(v), _c.ptr(p), _c.ptr(out)
    d.bias_u, d.bias_v, d.mask = _c.ptr(bias_u), _c.ptr(bias_v), _c.ptr(mask)
    d.q_sb, d.q_st = q_str
    d.k_sb, d.k_st, d.k_sh = k_str
    d.v_sb, d.v_st, d.v_sh = v_str
    d.p_sb, d.p_st = p_str
    d.m_sb, d.m_sq = mask_str
    d.B, d.H, d.Tq, d.Tk, d.dk = B, H, Tq, Tk, dk
    d.q_dtype, d.kv_dtype, d.out_dtype = _c.dt_code(q), _c.dt_code(k), _c.dt_code(out)
    d.p_dtype = _c.dt_code(p) if p is not None else 0
    d.mma_dtype, d.split = mma_code, 1 if split else 0
    d.scale = scale if scale is not None else float(dk) ** -0.5
    d.lse = _c.ptr(lse)
    if drop is not None and drop[0] > 0.0:       # (p, seed): dropout on the probabilities (train mode)
        d.drop_p, d.drop_seed = float(drop[0]), int(drop[1]) & 0xFFFFFFFF


def attention(q, k, v, B, H, Tq, Tk, dk, q_str, k_str, v_str, out, p=None, p_str=(0, 0), bias_u=None, bias_v=None, mask=None,
              mask_str=(0, 0), mma_code=_c.BF16, split=False, scale=None, lse=None, drop=None):
    """Fused attention; *_str are (batch stride, time stride[, head stride]) in ELEMENTS (see include/cfm.h).  lse: optional f32 [B,H,Tq]
    output (training): the log-sum-exp of each row's scaled masked scores."""
    d = _c.AttnDesc()
    _attn_fill(d, "attention", q, k, v, B, H, Tq, Tk, dk, q_str, k_str, v_str, out, p=p, p_str=p_str, bias_u=bias_u, bias_v=bias_v, mask=mask,
               mask_str=mask_str, mma_code=mma_code, split=split, scale=scale, lse=lse, drop=drop)
    _c.call("cfm_attention", ctypes.byref(d))
    return out


def attention_group(problems):
    """The attention problems of a training window (include/cfm.h cfm_attention_group: one launch when every problem qualifies, else one each).
    problems: a list of dicts, each holding the arguments of attention() by name; returns the `out` tensors in order."""
    n = len(problems)
    if n == 0:
        raise ValueError("cfm.attention_group: no problems")
    arr = (_c.AttnDesc * n)()
    for d, kw in zip(arr, problems):
        _attn_fill(d, "attention_group", **kw)
    _c.call("cfm_attention_group", arr, n)
    return [kw["out"] for kw in problems]


def kv_cache_pack(old_cache, k, v, k_str, v_str, B, H, Tn, dk):
    """-> f32 (B,H,Tc+Tn,2dk): rows < Tc copied from old_cache, the rest taken from k / v."""
    Tc = old_cache.size(2) if old_cache is not None else 0
    if old_cache is not None:                            # by hand: a strided cache is copied, not refused, which _layout does not state
        if old_cache.dtype != torch.float32 or tuple(old_cache.shape) != (B, H, Tc, 2 * dk):
            raise ValueError("cfm.kv_cache_pack: cache must be float32 (B,H,Tc,2dk); got %s %s" % (old_cache.dtype, tuple(old_cache.shape)))
        old_cache = old_cache.contiguous()
    _c.require_hip(old_cache, k, v)
    _strides_match("kv_cache_pack", "k", k, k_str[0], k_str[1])
    _strides_match("kv_cache_pack", "v", v, v_str[0], v_str[1])
    if k.dtype != v.dtype:
        raise ValueError("cfm.kv_cache_pack: k and v must share one dtype")
    out = torch.empty((B, H, Tc + Tn, 2 * dk), dtype=torch.float32, device=k.device)
    _c.call("cfm_kv_cache_pack", _c.ptr(old_cache), Tc, _c.ptr(k), _c.ptr(v), _c.dt_code(k), k_str[0], k_str[1], v_str[0],
            v_str[1], _c.ptr(out), B, H, Tn, dk)
    return out


def dwconv_bn_silu(x, w, dw_bias, bn_scale, bn_shift, out=None, out_dtype=None):
    """x [B,T,D] channels-last -> silu(bn(depthwise(x)))."""
    _c.require_hip(x, w, dw_bias, bn_scale, bn_shift, out)
    if x.dim() != 3 or not x.is_contiguous():
        raise ValueError("cfm.dwconv_bn_silu: x must be contiguous [B,T,D]")
    B, T, D = x.shape
    _dense("dwconv_bn_silu", w=w, dw_bias=dw_bias, bn_scale=bn_scale, bn_shift=bn_shift, out=out)
    if out is None:
        out = torch.empty((B, T, D), dtype=out_dtype or x.dtype, device=x.device)
    elif out.numel() != B * T * D:
        raise ValueError("cfm.dwconv_bn_silu: out must hold [B,T,D]")
    _c.call("cfm_dwconv_bn_silu", _c.ptr(x), _c.dt_code(x), _c.ptr(w), _c.ptr(dw_bias), _c.ptr(bn_scale), _c.ptr(bn_shift),
            _c.ptr(out), _c.dt_code(out), B, T, D, w.shape[1])
    return out


def conv1_relu_mma_supported(C, out_dtype):
    return C % 16 == 0 and C <= 256 and out_dtype in (torch.bfloat16, torch.float16)


def conv1_relu(x, w9c, bias, out_dtype, cmvn=None, mma=False):
    """x [B,T,F] f32 -> relu(conv3x3 s2) channels-last [B,T1,F1,C].  cmvn = (mean [F], istd [F] | None): global CMVN folded into the
    tap loads, (x - mean) * istd, bit-identical to normalising first.  mma=True: the 9 taps as an MFMA contraction on operands rounded
    to out_dtype (16-bit; include/cfm.h cfm_conv1_relu_mma) instead of f32 FMAs."""
    _c.require_hip(x, w9c, bias)
    mean = istd = None
    if cmvn is not None:
        mean, istd = cmvn
        _c.require_hip(mean, istd)
        for t in (mean, istd):
            if t is not None and (t.dtype != torch.float32 or t.numel() != x.shape[2] or not t.is_contiguous()):
                raise ValueError("cfm.conv1_relu: cmvn statistics must be contiguous float32 [F]")
    if x.dim() != 3 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("cfm.conv1_relu: x must be contiguous float32 [B,T,F]")
    B, T, F = x.shape
    C = w9c.shape[1]
    _dense("conv1_relu", w9c=w9c, bias=bias)
    if tuple(w9c.shape) != (9, C) or w9c.dtype != torch.float32 or bias.dtype != torch.float32 or bias.numel() != C:
        raise ValueError("cfm.conv1_relu: w9c must be float32 [9,C] (tap-major) and bias float32 [C]")
    T1, F1 = (T - 3) // 2 + 1, (F - 3) // 2 + 1
    out = torch.empty((B, T1, F1, C), dtype=out_dtype, device=x.device)
    _c.call("cfm_conv1_relu_mma" if mma else "cfm_conv1_relu",
            _c.ptr(x), _c.ptr(w9c), _c.ptr(bias), _c.ptr(out), _c.dt_code(out), B, T, F, C, _c.ptr(mean), _c.ptr(istd))
    return out


def conv12_supported(C, out_dtype):
    return out_dtype in (torch.bfloat16, torch.float16) and bool(_c.lib().cfm_conv12_supported(C, _c.dt_code(out_dtype)))


def conv12_relu(x, w9c, b1, w2, b2, cmvn=None):
    """x [B,T,F] f32 -> relu(conv3x3 s2(relu(conv3x3 s2(x)))) as [B*T2*F2, C] in w2's 16-bit dtype, the first convolution recomputed inside
    the second one's operand producer (include/cfm.h cfm_conv12_relu; bit-identical to conv1_relu(mma=True) + gemm(conv=...))."""
    _c.require_hip(x, w9c, b1, w2, b2)
    mean = istd = None
    if cmvn is not None:
        mean, istd = cmvn
        _c.require_hip(mean, istd)
        for t in (mean, istd):
            if t is not None and (t.dtype != torch.float32 or t.numel() != x.shape[2] or not t.is_contiguous()):
                raise ValueError("cfm.conv12_relu: cmvn statistics must be contiguous float32 [F]")
    if x.dim() != 3 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("cfm.conv12_relu: x must be contiguous float32 [B,T,F]")
    B, T, F = x.shape
    C = w9c.shape[1]
    _dense("conv12_relu", w9c=w9c, b1=b1, b2=b2)
    if tuple(w9c.shape) != (9, C) or any(t.dtype != torch.float32 for t in (w9c, b1, b2)) or b1.numel() != C or b2.numel() != C:
        raise ValueError("cfm.conv12_relu: w9c must be float32 [9,C] (tap-major), b1 and b2 float32 [C]")
    if w2.shape != (C, 9 * C) or not w2.is_contiguous() or w2.dtype not in (torch.bfloat16, torch.float16):
        raise ValueError("cfm.conv12_relu: w2 must be a contiguous 16-bit [C, 9C] matrix")
    T1, F1 = (T - 3) // 2 + 1, (F - 3) // 2 + 1
    T2, F2 = (T1 - 3) // 2 + 1, (F1 - 3) // 2 + 1
    out = torch.empty((B * T2 * F2, C), dtype=w2.dtype, device=x.device)
    _c.call("cfm_conv12_relu", _c.ptr(x), _c.ptr(w9c), _c.ptr(b1), _c.ptr(w2), _c.ptr(b2), _c.ptr(out), _c.dt_code(out), B, T, F, C,
            _c.ptr(mean), _c.ptr(istd))
    return out


def _ctc_logits(op, logits):
    """-> (B, T) of f32 logits [B,T,ld] whose rows are evenly spaced (cfm.h passes one row stride)."""
    if logits.dim() != 3 or logits.dtype != torch.float32 or logits.stride(2) != 1 or logits.stride(0) != logits.size(1) * logits.stride(1):
        raise ValueError("cfm.%s: logits must be float32 [B,T,>=V] with contiguous rows, got %s %s strides %s" % (op, logits.dtype, tuple(logits.shape), logits.stride()))
    return logits.shape[:2]


def _ctc_args(op, logits, enc_lens, labels, label_lens):
    """The operands every CTC loss / alignment entry takes: logits, enc_lens / label_lens int32 [B], labels int32 [B,Umax].  -> (B, T)."""
    _c.require_hip(logits, enc_lens, labels, label_lens)
    B, T = _ctc_logits(op, logits)
    _layout(op, "logits has B = %d; where a count is off, the batch sizes differ" % B, labels=(labels, _I32, (B, None)), **_i32(B, enc_lens=enc_lens, label_lens=label_lens))
    return B, T


def ctc_nll(logits, V, enc_lens, labels, label_lens):
    """Per-utterance CTC negative log-likelihood from UN-normalised f32 logits [B,T,ld>=V] (log-softmax applied on the fly); blank 0.
    enc_lens / label_lens int32 [B], labels int32 [B,Umax].  Returns f32 [B] (include/cfm.h cfm_ctc_nll)."""
    B, T = _ctc_args("ctc_nll", logits, enc_lens, labels, label_lens)
    out = torch.empty((B,), dtype=torch.float32, device=logits.device)
    work = scratch("ctc_lp", B * T * (2 * labels.size(1) + 2), torch.float32, logits.device)
    _c.call("cfm_ctc_nll", _c.ptr(logits), logits.stride(1), B, T, V, _c.ptr(enc_lens), _c.ptr(labels), labels.size(1), _c.ptr(label_lens),
            _c.ptr(work), _c.ptr(out))
    return out


def ctc_topk(logits, V, lens, k, out=None):
    """Per valid frame of f32 logits [B,T,ld>=V] the k <= 16 largest log-probabilities (log-softmax applied on the fly) with their classes, in
    descending order, the lower class first among equal values, and the frame's log-sum-exp.  lens int32 [B].  Returns (idx int32 [B,T,k],
    logp f32 [B,T,k], lse f32 [B,T]); rows of frames at or beyond lens[b] are not written (out: such a triple to write into; fresh ones are
    zero-filled).  include/cfm.h cfm_ctc_topk."""
    _c.require_hip(logits, lens)
    B, T = _ctc_logits("ctc_topk", logits)
    _layout("ctc_topk", **_i32(B, lens=lens))
    k = int(k)
    if out is None:
        out = (torch.zeros((B, T, max(k, 0)), dtype=torch.int32, device=logits.device), torch.zeros((B, T, max(k, 0)), dtype=torch.float32, device=logits.device),
               torch.zeros((B, T), dtype=torch.float32, device=logits.device))
    idx, logp, lse = out
    _want("ctc_topk", "out must be (idx int32 [B,T,k], logp float32 [B,T,k], lse float32 [B,T])", idx=(idx, _I32, B * T * k), logp=(logp, _F32, B * T * k), lse=(lse, _F32, B * T))
    _c.call("cfm_ctc_topk", _c.ptr(logits), logits.stride(1), B, T, V, _c.ptr(lens), k, _c.ptr(idx), _c.ptr(logp), _c.ptr(lse))
    return idx, logp, lse


def ctc_greedy_state(B, cap, device):
    """The per-stream state of ctc_greedy for B streams and room for cap symbols each: prev int32 [B] (-1), frame_base int32 [B], count int64 [B],
    hyps int64 / frames int32 / token_logp f32 [B, cap], overflow int32 [1]."""
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=device)
    return dict(prev=torch.full((B,), -1, dtype=torch.int32, device=device), frame_base=z((B,), torch.int32), count=z((B,), torch.int64),
                hyps=z((B, cap), torch.int64), frames=z((B, cap), torch.int32), token_logp=z((B, cap), torch.float32), overflow=z((1,), torch.int32))


def _topk_args(op, idx, logp, lens):
    """ctc_topk's output as the decoders read it: idx int32 and logp f32 [B,T,k], lens int32 [B].  -> (B, T, k)."""
    _want(op, "idx int32 and logp float32 are the [B,T,k] of ctc_topk", idx=(idx, _I32, (None, None, None)), logp=(logp, _F32, tuple(idx.shape)),
          lens=(lens, _I32, idx.shape[:1].numel()))
    return idx.shape


def ctc_greedy(idx, logp, lens, V, blank=0, state=None, hyp_cap=None):
    """Best-path CTC decoding of ctc_topk's output (any k; the first column is read): per stream the classes of frames 0 .. lens[b] - 1 with
    repeats collapsed and blanks dropped are APPENDED to state (ctc_greedy_state; a fresh one with room for T symbols when None), which carries
    the last frame's class from call to call.  Returns state; the caller reads count / hyps / frames / token_logp / overflow from it.
    include/cfm.h cfm_ctc_greedy."""
    B, T, k = _topk_args("ctc_greedy", idx, logp, lens)
    S = ctc_greedy_state(B, T, idx.device) if state is None else state
    fb, cap = S.get("frame_base"), tuple(S["hyps"].shape)
    spec = {name: _opt(t, None, None) for name, t in S.items()}               # whatever else the state holds is at least dense
    spec.update(prev=(S["prev"], _I32, (B,)), count=(S["count"], _I64, (B,)), hyps=(S["hyps"], _I64, (B, None)), frames=(S["frames"], _I32, cap),
                token_logp=(S["token_logp"], _F32, cap), overflow=(S["overflow"], _I32, (1,)), frame_base=_opt(fb, _I32, (B,)))
    _want("ctc_greedy", "an entry of state (ctc_greedy_state)", **spec)
    d = _c.CtcGreedyDesc()
    d.idx, d.logp, d.ld_k, d.lens = _c.ptr(idx), _c.ptr(logp), k, _c.ptr(lens)
    d.prev, d.frame_base, d.hyps, d.count, d.frames, d.token_logp, d.overflow = (_c.ptr(S["prev"]), _c.ptr(fb), _c.ptr(S["hyps"]), _c.ptr(S["count"]), _c.ptr(S["frames"]),
                                                                                 _c.ptr(S["token_logp"]), _c.ptr(S["overflow"]))
    d.hyp_ld = S["hyps"].size(1)
    d.hyp_cap = d.hyp_ld if hyp_cap is None else int(hyp_cap)
    d.B, d.T, d.V, d.blank = B, T, int(V), int(blank)
    _c.call("cfm_ctc_greedy", ctypes.byref(d))
    return S


def ctc_prefix_beam(idx, logp, lens, V, beam=None, blank=0, out=None, nodes=None):
    """CTC prefix beam search over ctc_topk's output: idx int32 / logp f32 [B,T,k], lens int32 [B]; beam <= 16 prefixes are kept (default: k) and a
    frame offers its first min(k, beam) classes.  Returns
    (nbest_tokens int64 [B,beam,T], nbest_len int32 [B,beam], nbest_score f32 [B,beam]), best first; entry n holds nbest_len[b,n] tokens, entries
    beyond the live prefixes have length 0 and score -inf.  out: such a triple to write into; nodes: the int32 [B*beam*(T+1), 2] trie scratch.
    include/cfm.h cfm_ctc_prefix_beam."""
    B, T, k = _topk_args("ctc_prefix_beam", idx, logp, lens)
    beam = k if beam is None else int(beam)
    dev = idx.device
    if out is None:
        nb = max(beam, 0)
        out = (torch.zeros((B, nb, T), dtype=torch.int64, device=dev), torch.zeros((B, nb), dtype=torch.int32, device=dev),
               torch.zeros((B, nb), dtype=torch.float32, device=dev))
    tokens, nlen, score = out
    if nodes is None:
        nodes = scratch("ctc_beam_nodes", 2 * B * max(beam, 1) * (T + 1), torch.int32, dev)
    _want("ctc_prefix_beam", "out must be (nbest_tokens int64 [B,beam,T], nbest_len int32 [B,beam], nbest_score float32 [B,beam]), nodes int32",
          nbest_tokens=(tokens, _I64, B * beam * T), nbest_len=(nlen, _I32, B * beam), nbest_score=(score, _F32, B * beam), nodes=(nodes, _I32, None))
    d = _c.CtcBeamDesc()
    d.idx, d.logp, d.lens, d.nodes, d.n_nodes = _c.ptr(idx), _c.ptr(logp), _c.ptr(lens), _c.ptr(nodes), nodes.numel() // 2
    d.nbest_tokens, d.nbest_len, d.nbest_score = _c.ptr(tokens), _c.ptr(nlen), _c.ptr(score)
    d.B, d.T, d.V, d.k, d.beam, d.blank = B, T, int(V), k, beam, int(blank)
    _c.call("cfm_ctc_prefix_beam", ctypes.byref(d))
    return tokens, nlen, score


def ctc_align(logits, V, enc_lens, labels, label_lens, out=None):
    """CTC forced alignment: the best single alignment of each utterance's frames to its labels (blank 0, as the loss), from UN-normalised f32
    logits [B,T,ld>=V].  enc_lens / label_lens int32 [B], labels int32 [B,Umax], Umax <= 255.  Returns (path int32 [B,T], score f32 [B],
    start int32 [B,Umax], end int32 [B,Umax], token_logp f32 [B,Umax]) on the device: path[b,t] the state 0..2U of frame t (-1 at and beyond
    enc_lens[b]), score the path's log-probability, per label its first / last frame and the sum of its frames' log-probabilities (-1, -1, -inf
    beyond label_lens[b]); an utterance that has no alignment gives score -inf and that fill everywhere.  out: such a tuple to write into.
    include/cfm.h cfm_ctc_align states the recursion and its tie rule."""
    B, T = _ctc_args("ctc_align", logits, enc_lens, labels, label_lens)
    Umax, dev = labels.size(1), logits.device
    if out is None:
        out = (torch.empty((B, T), dtype=torch.int32, device=dev), torch.empty((B,), dtype=torch.float32, device=dev), torch.empty((B, Umax), dtype=torch.int32, device=dev),
               torch.empty((B, Umax), dtype=torch.int32, device=dev), torch.empty((B, Umax), dtype=torch.float32, device=dev))
    path, score, start, end, token_logp = out
    _want("ctc_align", "out must be (path int32 [B,T], score float32 [B], start int32 [B,Umax], end int32 [B,Umax], token_logp float32 [B,Umax])",
          path=(path, _I32, B * T), score=(score, _F32, B), start=(start, _I32, B * Umax), end=(end, _I32, B * Umax), token_logp=(token_logp, _F32, B * Umax))
    nbytes = int(_c.lib().cfm_ctc_align_scratch_bytes(B, T, max(Umax, 0)))
    work = scratch("ctc_lp", B * T * (2 * Umax + 2), torch.float32, dev)
    moves = scratch("ctc_align_moves", nbytes, torch.uint8, dev)
    d = _c.CtcAlignDesc()
    d.logits, d.ld, d.enc_lens, d.labels, d.label_lens = _c.ptr(logits), logits.stride(1), _c.ptr(enc_lens), _c.ptr(labels), _c.ptr(label_lens)
    d.work, d.scratch, d.scratch_bytes = _c.ptr(work), _c.ptr(moves), nbytes
    d.path, d.score, d.start, d.end, d.token_logp = _c.ptr(path), _c.ptr(score), _c.ptr(start), _c.ptr(end), _c.ptr(token_logp)
    d.B, d.T, d.V, d.Umax = B, T, int(V), Umax
    _c.call("cfm_ctc_align", ctypes.byref(d))
    return path, score, start, end, token_logp


def edit_distance(hyp, hyp_lens, ref, ref_lens, ref_index=None, counts=True, ops=False, out=None):
    """Levenshtein distance of P hypothesis-reference pairs in one launch (include/cfm.h cfm_edit_distance states the recurrence and the tie rule of
    the alignment).  hyp int32 [P,Hmax] with hyp_lens int32 [P], ref int32 [R,Umax] with ref_lens int32 [R], Hmax, Umax <= 1024; pair p is scored
    against reference ref_index[p] (int32 [P], values in [0, R): the caller's to guarantee), ref_index=None: P == R and reference p.  Returns
    (dist int32 [P], counts int32 [P,4] = (S, D, I, hits) | None, ops uint8 [P,Hmax+Umax] | None, ops_len int32 [P] | None) on the device; ops
    (1 hit, 2 substitution, 3 deletion, 4 insertion, 0 beyond ops_len) imply counts.  out: such a tuple to write into (None where not wanted).
    Nothing is read back to the host."""
    _c.require_hip(hyp, hyp_lens, ref, ref_lens, ref_index)
    _layout("edit_distance", "hyp is [P,Hmax] and ref [R,Umax]", hyp=(hyp, _I32, (None, None)), ref=(ref, _I32, (None, None)))
    (P, Hmax), (R, Umax), dev = hyp.shape, ref.shape, hyp.device
    _layout("edit_distance", "P = %d hypotheses, R = %d references; where a count is off, the batch sizes differ" % (P, R),
            ref_index=_opt(ref_index, _I32, P), **_i32(P, hyp_lens=hyp_lens), **_i32(R, ref_lens=ref_lens))
    if ref_index is None and P != R:
        raise ValueError("cfm.edit_distance: batch sizes differ: %d hypotheses for %d references and no ref_index" % (P, R))
    if P < 1 or R < 1:
        raise ValueError("cfm.edit_distance: no pair to score")
    if Hmax > 1024 or Umax > 1024:
        raise ValueError("cfm.edit_distance: Hmax=%d Umax=%d exceeds 1024 tokens" % (Hmax, Umax))
    counts = bool(counts or ops)
    if out is None:
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
        out = (i32(P), i32(P, 4) if counts else None, torch.empty((P, Hmax + Umax), dtype=torch.uint8, device=dev) if ops else None, i32(P) if ops else None)
    dist, cnt, op, op_len = out
    what = "out must be (dist int32 [P], counts int32 [P,4] | None, ops uint8 [P,Hmax+Umax] | None, ops_len int32 [P] | None) as counts / ops ask"
    _want("edit_distance", what, dist=(dist, _I32, P), counts=_opt(cnt, _I32, 4 * P), ops=_opt(op, torch.uint8, P * (Hmax + Umax)), ops_len=_opt(op_len, _I32, P))
    if (cnt is not None) != counts or (op is not None) != bool(ops) or (op_len is not None) != bool(ops):
        raise ValueError("cfm.edit_distance: " + what)
    nbytes = int(_c.lib().cfm_edit_distance_scratch_bytes(P, Hmax, Umax)) if counts else 0
    moves = scratch("edit_distance_moves", nbytes, torch.uint8, dev) if nbytes else None
    d = _c.EditDistanceDesc()
    d.hyp, d.hyp_lens, d.ref, d.ref_lens, d.ref_index = _c.ptr(hyp), _c.ptr(hyp_lens), _c.ptr(ref), _c.ptr(ref_lens), _c.ptr(ref_index)
    d.dist, d.counts, d.ops, d.ops_len = _c.ptr(dist), _c.ptr(cnt), _c.ptr(op), _c.ptr(op_len)
    d.scratch, d.scratch_bytes = _c.ptr(moves), nbytes
    d.P, d.R, d.Hmax, d.Umax = P, R, Hmax, Umax
    _c.call("cfm_edit_distance", ctypes.byref(d))
    return dist, cnt, op, op_len


def joint_act(enc, pred, B, T, U, out_dtype):
    """tanh(enc[b*T+t] + pred[b*U+u]) for every (b,t,u) as a row-major [B*T*U, J] operand (include/cfm.h cfm_joint_act).
    enc f32 [B*T,J], pred f32 [B*U,J] with unit inner stride."""
    _c.require_hip(enc, pred)
    enc, pred = _rows2d(enc, "joint_act(enc)"), _rows2d(pred, "joint_act(pred)")
    J = enc.shape[1]
    if enc.dtype != torch.float32 or pred.dtype != torch.float32 or tuple(enc.shape) != (B * T, J) or tuple(pred.shape) != (B * U, J):
        raise ValueError("cfm.joint_act: enc must be f32 [%d,J] and pred f32 [%d,J], got %s %s" % (B * T, B * U, tuple(enc.shape), tuple(pred.shape)))
    out = torch.empty((B * T * U, J), dtype=out_dtype, device=enc.device)
    _c.call("cfm_joint_act", _c.ptr(enc), enc.stride(0), _c.ptr(pred), pred.stride(0), _c.ptr(out), _c.dt_code(out), B, T, U, J)
    return out


def valid_mask(lengths, T, first=0, stride=1):
    """bool (B,T): (first + stride*t) < lengths[b]."""
    _c.require_hip(lengths)
    if lengths.dtype not in (torch.int32, torch.int64) or lengths.dim() != 1:
        raise ValueError("cfm.valid_mask: lengths must be a 1-D int32/int64 tensor")
    lengths = lengths.contiguous()
    B = lengths.numel()
    out = torch.empty((B, T), dtype=torch.uint8, device=lengths.device)
    _c.call("cfm_valid_mask", _c.ptr(lengths), 1 if lengths.dtype == torch.int64 else 0, _c.ptr(out), B, T, first, stride)
    return out.view(torch.bool)


def chunk_mask(size, chunk, left, device):
    out = torch.empty((size, size), dtype=torch.uint8, device=device)
    _c.require_hip(out)
    _c.call("cfm_chunk_mask", _c.ptr(out), size, chunk, left)
    return out.view(torch.bool)


def attn_mask_combine(valid, chunk):
    """valid bool (B,1,T) [or (B,T)] & chunk bool (T,T) -> bool (B,T,T)."""
    v = as_u8_mask(valid.reshape(valid.size(0), -1))
    c = as_u8_mask(chunk)
    _c.require_hip(v, c)
    B, T = v.shape
    out = torch.empty((B, T, T), dtype=torch.uint8, device=v.device)
    _c.call("cfm_attn_mask", _c.ptr(v), _c.ptr(c), _c.ptr(out), B, T)
    return out.view(torch.bool)


def cast(src, dtype):
    _c.require_hip(src)
    src = src.contiguous()
    out = torch.empty(src.shape, dtype=dtype, device=src.device)
    if src.numel():
        _c.call("cfm_cast", _c.ptr(src), _c.dt_code(src), _c.ptr(out), _c.dt_code(out), src.numel())
    return out


def add_rows(x, add, group):
    """x[r,:] += add[r // group, :] in place (f32)."""
    _c.require_hip(x, add)
    rows, D = x.shape
    _dense("add_rows", x=x, add=add)
    if x.dtype != torch.float32 or add.dtype != torch.float32 or add.dim() != 2 or add.shape[1] != D or add.shape[0] * group < rows:
        raise ValueError("cfm.add_rows: x f32 [rows,D] and add f32 [>= rows/group, D] expected, got %s %s" % (tuple(x.shape), tuple(add.shape)))
    _c.call("cfm_add_rows", _c.ptr(x), _c.ptr(add), rows, D, group)
    return x


# ----------------------------------------------------------------------------------------------------------------------
def prof_enable(on=True):
    _c.lib().cfm_prof_enable(1 if on else 0)


def prof_reset():
    _c.lib().cfm_prof_reset()


def prof_table():
    """Synchronise the recorded events; returns {kernel name: dict(calls, ms, flops, bytes)}."""
    L = _c.lib()
    n = L.cfm_prof_collect()
    out = {}
    name = ctypes.create_string_buffer(128)
    calls, ms, fl, by = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    for i in range(n):
        _c.check(L.cfm_prof_entry(i, name, 128, ctypes.byref(calls), ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by)), "cfm_prof_entry")
        out[name.value.decode()] = dict(calls=calls.value, ms=ms.value, flops=fl.value, bytes=by.value)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# training (include/cfm.h "Training"): thin wrappers, outputs allocated here, workspaces from the per-stream arena
# ----------------------------------------------------------------------------------------------------------------------
_deterministic = [False]


def set_deterministic(on=True):
    """Bitwise-reproducible gradients: the weight-gradient GEMM then runs ONE workgroup per output tile over all M rows (no split-M
    atomics, whose arrival order varies from run to run).  Slower on small batches; for tests and debugging."""
    _deterministic[0] = bool(on)


def gemm_tn(a, b, out=None, want_colsum=False, row_mask=None, alpha=1.0, conv=None, split=False, splits=0, mma_code=_c.BF16, accumulate=False,
            colsum=None):
    """C[N,K] (+)= alpha * a[M,N]^T . b[M,K]  (f32) and optionally colsum[N] = alpha * sum_m a[m,:]: the weight / bias gradient of a
    dense layer from its output gradient `a` and its input rows `b` (include/cfm.h cfm_gemm_tn).  conv=(C,T1,F1,T2,F2): `b` is a
    channels-last image [B,T1,F1,C] read as its 3x3 stride-2 im2col matrix.  Returns (C, colsum | None)."""
    _c.require_hip(a, b, out, row_mask, colsum)
    a = _rows2d(a, "gemm_tn(a)")
    M, N = a.shape
    d = _c.GemmTnDesc()
    if conv is None:
        b = _rows2d(b, "gemm_tn(b)")
        if b.shape[0] != M:
            raise ValueError("cfm.gemm_tn: a is %s but b is %s" % (tuple(a.shape), tuple(b.shape)))
        K = b.shape[1]
        d.ldb = b.stride(0)
    else:
        C, T1, F1, T2, F2 = conv
        _layout("gemm_tn(conv)", "the channels-last image [B,T1,F1,C]", b=(b, None, (M // (T2 * F2)) * T1 * F1 * C))
        K = 9 * C
        d.conv_C, d.conv_T1, d.conv_F1, d.conv_T2, d.conv_F2 = C, T1, F1, T2, F2
    if out is None:
        if accumulate:
            raise ValueError("cfm.gemm_tn: accumulate needs an existing out")
        if want_colsum and colsum is None and not _deterministic[0]:
            # weight and bias gradient in ONE zero-filled buffer (one fill launch instead of the library's two memsets), then accumulate
            buf = torch.zeros((N * K + N,), dtype=torch.float32, device=a.device)
            out, colsum, accumulate = buf[:N * K].view(N, K), buf[N * K:], True
        else:
            out = torch.empty((N, K), dtype=torch.float32, device=a.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (N, K) or out.stride(1) != 1:
        raise ValueError("cfm.gemm_tn: out must be float32 (%d,%d)" % (N, K))
    if want_colsum and colsum is None:
        colsum = torch.empty((N,), dtype=torch.float32, device=a.device)
    _layout("gemm_tn", colsum=_opt(colsum, _F32, N), row_mask=_opt(row_mask, torch.uint8, M))
    d.A, d.B, d.C, d.colsum, d.row_mask = _c.ptr(a), _c.ptr(b), _c.ptr(out), _c.ptr(colsum), _c.ptr(row_mask)
    d.lda, d.ldc = a.stride(0), out.stride(0)
    d.M, d.N, d.K = M, N, K
    d.a_dtype, d.b_dtype, d.mma_dtype = _c.dt_code(a), _c.dt_code(b), mma_code
    d.split, d.accumulate, d.splits, d.alpha = 1 if split else 0, 1 if accumulate else 0, (1 if _deterministic[0] else splits), alpha
    _c.call("cfm_gemm_tn", ctypes.byref(d))
    return out, colsum


def gemm_tn_group(products, mma_code=_c.BF16, splits=0):
    """Several weight-gradient products in ONE launch (include/cfm.h cfm_gemm_tn_group).  products: list of dicts with keys a [M,N], b [M,K],
    out f32 [N,K] (zero-filled or holding a running sum: the products ACCUMULATE), optional colsum f32 [N], alpha, row_off / colsum_off /
    colsum_off2 (int64 device tables; `out` / `colsum` are then the slab the offsets are relative to).  Returns nothing."""
    n = len(products)
    descs = (_c.GemmTnDesc * n)()
    for d, pr in zip(descs, products):
        a, b, out = _rows2d(pr["a"], "gemm_tn_group(a)"), _rows2d(pr["b"], "gemm_tn_group(b)"), pr["out"]
        colsum = pr.get("colsum")
        _c.require_hip(a, b, out, colsum)
        if a.shape[0] != b.shape[0] or out.dtype != torch.float32 or out.stride(-1) != 1:
            raise ValueError("cfm.gemm_tn_group: a %s and b %s with one row count and a float32 out with unit inner stride, got out %s strides %s"
                             % (tuple(a.shape), tuple(b.shape), out.dtype, out.stride()))
        d.A, d.B, d.C, d.colsum = a.data_ptr(), b.data_ptr(), out.data_ptr(), _c.ptr(colsum)
        d.lda, d.ldb = a.stride(0), b.stride(0)
        d.M, d.N, d.K = a.shape[0], a.shape[1], b.shape[1]
        # a 2-D out carries its own row stride; a flat slab (row_off scatter) has none to carry
        d.ldc = pr.get("ldc", out.stride(0) if out.dim() == 2 and pr.get("row_off") is None else d.K)
        d.a_dtype, d.b_dtype, d.mma_dtype = _c.dt_code(a), _c.dt_code(b), mma_code
        d.accumulate, d.splits, d.alpha = 1, (1 if _deterministic[0] else splits), float(pr.get("alpha", 1.0))
        tabs = {k: pr.get(k) for k in ("row_off", "colsum_off", "colsum_off2")}
        _want("gemm_tn_group", colsum=_opt(colsum, _F32, None), **{k: _opt(t, _I64, d.N) for k, t in tabs.items()})
        d.row_off, d.colsum_off, d.colsum_off2 = _c.ptr(tabs["row_off"]), _c.ptr(tabs["colsum_off"]), _c.ptr(tabs["colsum_off2"])
    _c.call("cfm_gemm_tn_group", descs, n)


def layernorm_bwd(x, dy, gamma, row_mask=None, dres=None, dx=None, eps=1e-5):
    """-> (dx, dgamma, dbeta): dx = (dres or 0) + dLayerNorm(dy) w.r.t. the norm's input x (f32 [M,D]); dx may be dres itself."""
    _c.require_hip(x, dy, gamma, row_mask, dres, dx)
    _layout("layernorm_bwd", x=(_rows2d(x, "layernorm_bwd(x)"), _F32, None))
    M, D = x.shape
    _layout("layernorm_bwd", dy=(dy, None, (M, D)), gamma=(gamma, _F32, D), row_mask=_opt(row_mask, None, M), dres=_opt(dres, _F32, (M, D)), dx=_opt(dx, _F32, (M, D)))
    if row_mask is not None and row_mask.element_size() != 1:
        raise ValueError("cfm.layernorm_bwd: row_mask is one byte per row, got %s" % row_mask.dtype)
    if dx is None:
        dx = torch.empty_like(x)
    dg = torch.empty((D,), dtype=torch.float32, device=x.device)
    db = torch.empty((D,), dtype=torch.float32, device=x.device)
    ws = scratch("ln_bwd", _c.lib().cfm_layernorm_bwd_ws(M, D), torch.float32, x.device)
    d = _c.LnBwdDesc()                      # the plain descriptor: accumulate = 0, no dx2, no chained norm
    d.x, d.dy, d.gamma, d.row_mask, d.dres = _c.ptr(x), _c.ptr(dy), _c.ptr(gamma), _c.ptr(row_mask), _c.ptr(dres)
    d.dx, d.dgamma, d.dbeta, d.ws = _c.ptr(dx), _c.ptr(dg), _c.ptr(db), _c.ptr(ws)
    d.M, d.D, d.dy_dtype, d.eps = M, D, _c.dt_code(dy), eps
    _c.call("cfm_layernorm_bwd_fused", ctypes.byref(d))
    return dx, dg, db


def glu_bwd(u, dg, out_dtype):
    """u [M,2D] (the interleaved pre-GLU columns from gemm(..., pre_out=)), dg [M,D] -> du [M,2D] same layout."""
    _c.require_hip(u, dg)
    M, D2 = u.shape
    D = D2 // 2
    _layout("glu_bwd", u=(u, None, (M, D2)), dg=(dg, None, (M, D)))
    du = torch.empty((M, D2), dtype=out_dtype, device=u.device)
    _c.call("cfm_glu_bwd", _c.ptr(u), _c.dt_code(u), _c.ptr(dg), _c.dt_code(dg), _c.ptr(du), _c.dt_code(du), M, D)
    return du


def _train_groups(who, groups, rows):
    """The contiguous cfm_train_group table of a window from its (B, T) pairs; every row matrix must be dense with sum(B*T) rows."""
    n = len(groups)
    if not 1 <= n <= 8:
        raise ValueError("cfm.%s: %d row groups (1 .. 8)" % (who, n))
    arr = (_c.TrainGroup * n)()
    row0 = 0
    for tg, (B, T) in zip(arr, groups):
        if B <= 0 or T <= 0:
            raise ValueError("cfm.%s: empty group (B=%d, T=%d)" % (who, B, T))
        tg.B, tg.T, tg.row0 = B, T, row0
        row0 += B * T
    if row0 != rows:
        raise ValueError("cfm.%s: the groups hold %d rows but the row matrices %d" % (who, row0, rows))
    return arr


def _vec_f32(D, **vecs):
    return {k: _opt(t, _F32, D) for k, t in vecs.items()}


def _dw_window_ws(groups, D, ws, who, device):
    need = sum(_c.lib().cfm_dwconv_bn_ws(B, T, D) for B, T in groups)            # include/cfm.h: the SUM over the groups
    if ws is None:
        return scratch("dwbn", need, torch.float32, device)
    if ws.dtype != torch.float32 or ws.numel() < need or not ws.is_contiguous():
        raise ValueError("cfm.%s: ws must be contiguous float32 with at least %d elements" % (who, need))
    return ws


def dwconv_bn_train_groups(g, groups, w, dw_bias, gamma, beta, running_mean=None, running_var=None, momentum=0.1, eps=1e-5, s_dtype=None, c=None, stats=None, s=None, ws=None):
    """dwconv_bn_train over the micro-batches of a window in one launch per stage (include/cfm.h cfm_dwconv_bn_train_groups): g is the window's
    [M, D] row matrix, groups its (B, T) pairs back to back.  -> (c f32 [M,D], stats f32 [n,4,D], s [M,D]); each group has its own batch
    statistics, the optional running statistics take the momentum updates group after group."""
    who = "dwconv_bn_train_groups"
    _c.require_hip(g, w, dw_bias, gamma, beta, running_mean, running_var, c, stats, s, ws)
    if g.dim() != 2:
        raise ValueError("cfm.%s: g must be the window's [M,D] row matrix" % who)
    M, D = g.shape
    n = len(groups)
    arr = _train_groups(who, groups, M)
    _layout(who, g=(g, None, (M, D)), **_vec_f32(D, dw_bias=dw_bias, gamma=gamma, beta=beta, running_mean=running_mean, running_var=running_var))
    if (running_mean is None) != (running_var is None):
        raise ValueError("cfm.%s: running_mean and running_var go together" % who)
    _layout(who, w=(w, _F32, (D, None)))
    dev = g.device
    c = torch.empty((M, D), dtype=torch.float32, device=dev) if c is None else c
    s = torch.empty((M, D), dtype=s_dtype if s_dtype is not None else g.dtype, device=dev) if s is None else s
    stats = torch.empty((n, 4, D), dtype=torch.float32, device=dev) if stats is None else stats
    _layout(who, c=(c, _F32, (M, D)), s=(s, None, (M, D)), stats=(stats, _F32, n * 4 * D))
    ws = _dw_window_ws(groups, D, ws, who, dev)
    _c.call("cfm_dwconv_bn_train_groups", _c.ptr(g), _c.dt_code(g), _c.ptr(w), _c.ptr(dw_bias), _c.ptr(gamma), _c.ptr(beta), _c.ptr(running_mean),
            _c.ptr(running_var), momentum, eps, _c.ptr(c), _c.ptr(stats), _c.ptr(s), _c.dt_code(s), _c.ptr(ws), arr, n, D, w.shape[1])
    return c, stats, s


def dwconv_bn_train_bwd_groups(ds, c, stats, g, groups, w, dg_dtype=None, accumulate=False, glu_u=None, glu_du=None, dg=None, dw_w=None, dw_b=None, dgamma=None,
                               dbeta=None, dy_ws=None, ws=None):
    """dwconv_bn_train_bwd over the micro-batches of a window (include/cfm.h cfm_dwconv_bn_train_bwd_groups): row matrices [M, D], stats [n,4,D].
    -> (dg [M,D] or None, dw_w, dw_b, dgamma, dbeta): dg per group, the four parameter gradients summed over the groups -- on top of what the
    buffers hold with accumulate (they must then be passed).  glu_u [M,2D] (with glu_du, or one is made): the GLU backward in the same launch,
    du instead of dg; returned in place of dg."""
    who = "dwconv_bn_train_bwd_groups"
    _c.require_hip(ds, c, stats, g, w, glu_u, glu_du, dg, dw_w, dw_b, dgamma, dbeta, dy_ws, ws)
    if g.dim() != 2:
        raise ValueError("cfm.%s: g must be the window's [M,D] row matrix" % who)
    M, D = g.shape
    n = len(groups)
    arr = _train_groups(who, groups, M)
    _layout(who, g=(g, None, (M, D)), ds=_opt(ds, None, (M, D)), c=_opt(c, _F32, (M, D)), stats=(stats, _F32, n * 4 * D), w=(w, _F32, (D, None)))
    dev = g.device
    K = w.shape[1]
    if glu_du is not None and glu_u is None:
        raise ValueError("cfm.%s: glu_du without glu_u" % who)
    fused = glu_u is not None
    if fused:
        if D % 16:
            raise ValueError("cfm.%s: the fused GLU backward needs D %% 16 == 0 (D=%d)" % (who, D))
        if dg is not None:
            raise ValueError("cfm.%s: dg is not written by the fused GLU backward" % who)
        if dg_dtype is not None and dg_dtype != g.dtype:
            raise ValueError("cfm.%s: the fused GLU backward needs g and dg of one dtype" % who)
        glu_du = torch.empty((M, 2 * D), dtype=g.dtype, device=dev) if glu_du is None else glu_du
        _layout(who, glu_u=(glu_u, g.dtype, (M, 2 * D)), glu_du=(glu_du, g.dtype, (M, 2 * D)))
        dg_code = _c.dt_code(g)
    else:
        dg = torch.empty((M, D), dtype=dg_dtype if dg_dtype is not None else g.dtype, device=dev) if dg is None else dg
        _layout(who, dg=(dg, None, (M, D)))
        dg_code = _c.dt_code(dg)
    given = [t is not None for t in (dw_w, dw_b, dgamma, dbeta)]
    if accumulate and not all(given):
        raise ValueError("cfm.%s: accumulate adds to dw_w, dw_b, dgamma, dbeta: pass all four" % who)
    dw_w = torch.empty((D, K), dtype=torch.float32, device=dev) if dw_w is None else dw_w
    dw_b, dgamma, dbeta = (torch.empty((D,), dtype=torch.float32, device=dev) if t is None else t for t in (dw_b, dgamma, dbeta))
    _layout(who, dw_w=(dw_w, _F32, (D, K)), **_vec_f32(D, dw_b=dw_b, dgamma=dgamma, dbeta=dbeta))
    dy_ws = scratch("dwbn_dy", M * D, torch.float32, dev) if dy_ws is None else dy_ws
    if dy_ws.dtype != torch.float32 or dy_ws.numel() < M * D or not dy_ws.is_contiguous():
        raise ValueError("cfm.%s: dy_ws must be contiguous float32 with at least M*D = %d elements" % (who, M * D))
    ws = _dw_window_ws(groups, D, ws, who, dev)
    _c.call("cfm_dwconv_bn_train_bwd_groups", _c.ptr(ds), _c.dt_code(ds), _c.ptr(c), _c.ptr(stats), _c.ptr(g), _c.dt_code(g), _c.ptr(w), _c.ptr(dg), dg_code,
            _c.ptr(dw_w), _c.ptr(dw_b), _c.ptr(dgamma), _c.ptr(dbeta), _c.ptr(dy_ws), _c.ptr(ws), arr, n, D, K,
            1 if accumulate else 0, _c.ptr(glu_u), _c.ptr(glu_du))
    return (glu_du if fused else dg), dw_w, dw_b, dgamma, dbeta


def _dense_as(t, *shape):
    """t seen as `shape` where it is dense and holds that many elements; any other tensor as it is, for the callee's checks to refuse."""
    n = 1
    for k in shape:
        n *= k
    return t.view(shape) if t.is_contiguous() and t.numel() == n else t


def dwconv_bn_train(g, w, dw_bias, gamma, beta, running_mean, running_var, momentum, eps, s_dtype):
    """g [B,T,D] -> (c f32 [B,T,D], stats f32 [4,D], s = SiLU(BatchNorm_train(c)) in s_dtype); running statistics updated in place.
    dwconv_bn_train_groups on a window of this one batch."""
    if g.dim() != 3:
        raise ValueError("cfm.dwconv_bn_train: g must be [B,T,D]")
    B, T, D = g.shape
    c, stats, s = dwconv_bn_train_groups(_dense_as(g, B * T, D), [(B, T)], w, dw_bias, gamma, beta, running_mean, running_var, momentum, eps, s_dtype)
    return c.view(B, T, D), stats.view(4, D), s.view(B, T, D)


def dwconv_bn_train_bwd(ds, c, stats, g, w, dg_dtype):
    """-> (dg [B,T,D], d taps [D,K], d conv bias [D], d BatchNorm gain [D], d BatchNorm bias [D]).  dwconv_bn_train_bwd_groups on a window of this
    one batch: g [B,T,D]; ds, c [B,T,D] or [B*T,D]; stats [4,D] as dwconv_bn_train returned it."""
    if g.dim() != 3:
        raise ValueError("cfm.dwconv_bn_train_bwd: g must be [B,T,D]")
    B, T, D = g.shape
    M = B * T
    dg, *grads = dwconv_bn_train_bwd_groups(_dense_as(ds, M, D), _dense_as(c, M, D), _dense_as(stats, 1, 4, D), _dense_as(g, M, D), [(B, T)], w, dg_dtype)
    return (dg.view(B, T, D), *grads)


def col2im_relu_bwd(dcol, h1, out_dtype):
    """dcol [B*T2*F2, 9C] (K order (kt,kf,c)), h1 [B,T1,F1,C] -> dh1 = (h1 > 0) * col2im(dcol)."""
    _c.require_hip(dcol, h1)
    B, T1, F1, C = h1.shape
    T2, F2 = (T1 - 3) // 2 + 1, (F1 - 3) // 2 + 1
    _layout("col2im_relu_bwd", dcol=(dcol, None, (B * T2 * F2, 9 * C)), h1=(h1, None, (B, T1, F1, C)))
    dh1 = torch.empty((B, T1, F1, C), dtype=out_dtype, device=h1.device)
    _c.call("cfm_col2im_relu_bwd", _c.ptr(dcol), _c.dt_code(dcol), _c.ptr(h1), _c.dt_code(h1), _c.ptr(dh1), _c.dt_code(dh1), B, T1, F1, C)
    return dh1


def conv1_wgrad(dh1, x, cmvn=None):
    """dh1 [B,T1,F1,C], x f32 [B,T,F] -> (dw [9,C] tap-major, db [C])."""
    _c.require_hip(dh1, x)
    B, T, F = x.shape
    C = dh1.shape[3]
    mean, istd = cmvn if cmvn is not None else (None, None)
    _want("conv1_wgrad", "the cmvn statistics", mean=_opt(mean, _F32, F), istd=_opt(istd, _F32, F))
    _layout("conv1_wgrad", x=(x, _F32, (B, T, F)), dh1=(dh1, None, None))
    if tuple(dh1.shape[:3]) != (B, (T - 3) // 2 + 1, (F - 3) // 2 + 1):           # a prefix test: not an extent _layout states
        raise ValueError("cfm.conv1_wgrad: dh1 must be [B,T1,F1,C] = (%d, %d, %d, C), got %s" % (B, (T - 3) // 2 + 1, (F - 3) // 2 + 1, tuple(dh1.shape)))
    dw = torch.empty((9, C), dtype=torch.float32, device=x.device)
    db = torch.empty((C,), dtype=torch.float32, device=x.device)
    ws = scratch("conv1_wgrad", _c.lib().cfm_conv1_wgrad_ws(B, T, C), torch.float32, x.device)
    _c.call("cfm_conv1_wgrad", _c.ptr(dh1), _c.dt_code(dh1), _c.ptr(x), _c.ptr(mean), _c.ptr(istd), _c.ptr(dw), _c.ptr(db), _c.ptr(ws), B, T, F, C)
    return dw, db


def _attn_bwd_fill(d, who, q, k, v, out, dout, lse, B, H, Tq, Tk, dk, q_str, k_str, v_str, dq, dkk, dv, delta, mask=None, mask_str=(0, 0), mma_code=_c.BF16,
                   split=False, scale=None, drop=None):
    """Checks one attention backward problem and fills its cfm_attn_bwd_desc (shared by the single and the grouped wrapper)."""
    _c.require_hip(q, k, v, out, dout, lse, dq, dkk, dv, mask, delta)
    _dense(who, out=out, dout=dout, lse=lse, delta=delta)            # [B,Tq,H*dk] / [B,H,Tq] row-major: no strides in cfm_attn_bwd_desc
    for what, t, (sb, st) in (("q", q, q_str), ("k", k, k_str), ("v", v, v_str), ("dq", dq, q_str), ("dk", dkk, k_str), ("dv", dv, v_str)):
        # 2-D [B*T, ...] views carry the time stride, 3-D ones both; cfm_attn_bwd_desc has ONE set of strides for an operand and its gradient
        _strides_match(who, what, t, sb, st)
    if delta.dtype != torch.float32 or delta.numel() != B * H * Tq:
        raise ValueError("cfm.%s: delta must be float32 [B,H,Tq] = %d elements, got %s %s" % (who, B * H * Tq, delta.dtype, tuple(delta.shape)))
    if lse.dtype != torch.float32 or lse.numel() != B * H * Tq or out.numel() != B * Tq * H * dk or dout.numel() != B * Tq * H * dk:
        raise ValueError("cfm.%s: lse must be float32 [B,H,Tq], out and dout [B,Tq,H*dk]" % who)
    d.q, d.k, d.v, d.mask, d.out, d.dout, d.lse = _c.ptr(q), _c.ptr(k), _c.ptr(v), _c.ptr(mask), _c.ptr(out), _c.ptr(dout), _c.ptr(lse)
    d.grad_q, d.grad_k, d.grad_v = _c.ptr(dq), _c.ptr(dkk), _c.ptr(dv)
    d.delta = _c.ptr(delta)
    d.q_sb, d.q_st = q_str
    d.k_sb, d.k_st = k_str
    d.v_sb, d.v_st = v_str
    d.m_sb, d.m_sq = mask_str
    d.B, d.H, d.Tq, d.Tk, d.dk = B, H, Tq, Tk, dk
    if not (q.dtype == k.dtype == v.dtype == out.dtype == dq.dtype == dkk.dtype == dv.dtype):
        raise ValueError("cfm.%s: q, k, v, out and the gradients must share one dtype" % who)
    d.io_dtype, d.dout_dtype, d.mma_dtype, d.split = _c.dt_code(q), _c.dt_code(dout), mma_code, 1 if split else 0
    d.scale = scale if scale is not None else float(dk) ** -0.5
    if drop is not None and drop[0] > 0.0:
        d.drop_p, d.drop_seed = float(drop[0]), int(drop[1]) & 0xFFFFFFFF


def attention_bwd(q, k, v, out, dout, lse, B, H, Tq, Tk, dk, q_str, k_str, v_str, dq, dkk, dv, mask=None, mask_str=(0, 0), mma_code=_c.BF16, split=False,
                  scale=None, drop=None, delta=None):
    """Backward of attention(); q/k/v and dq/dkk/dv share strides ((batch, time) in elements, head h at h*dk); see include/cfm.h.
    delta: optional f32 [B,H,Tq] scratch (taken from the arena when absent)."""
    _c.require_hip(q)
    if delta is None:
        delta = scratch("attn_delta", B * H * Tq, torch.float32, q.device)
    d = _c.AttnBwdDesc()
    _attn_bwd_fill(d, "attention_bwd", q, k, v, out, dout, lse, B, H, Tq, Tk, dk, q_str, k_str, v_str, dq, dkk, dv, delta, mask=mask, mask_str=mask_str,
                   mma_code=mma_code, split=split, scale=scale, drop=drop)
    _c.call("cfm_attention_bwd", ctypes.byref(d))


def attention_bwd_group(problems):
    """The attention backward problems of a training window (include/cfm.h cfm_attention_bwd_group).  problems: a list of dicts, each holding the
    arguments of attention_bwd() by name; a problem without `delta` gets its [B,H,Tq] slice of ONE arena buffer, at the running offset."""
    n = len(problems)
    if n == 0:
        raise ValueError("cfm.attention_bwd_group: no problems")
    need = [kw["B"] * kw["H"] * kw["Tq"] for kw in problems]
    _c.require_hip(problems[0]["q"])
    pool = scratch("attn_delta", sum(need), torch.float32, problems[0]["q"].device) if any(kw.get("delta") is None for kw in problems) else None
    arr = (_c.AttnBwdDesc * n)()
    off = 0
    for d, kw, m in zip(arr, problems, need):
        kw = dict(kw)
        if kw.get("delta") is None:
            kw["delta"] = pool[off:off + m]
        off += m
        _attn_bwd_fill(d, "attention_bwd_group", **kw)
    _c.call("cfm_attention_bwd_group", arr, n)


def ctc_nll_train_groups(problems, V):
    """As ctc_nll for the micro-batches of a training window (a single batch is a window of one), keeping what ctc_grad needs, with ONE launch for
    all their recursions (include/cfm.h cfm_ctc_nll_train_groups).  problems: [(logits [B,T,ld], enc_lens, labels, label_lens)]; returns
    [(nll [B], state)] with state = (work, alpha, lse, nll_shifted, beta) owned by the caller."""
    n = len(problems)
    arr = (_c.CtcGroup * n)()
    outs = []
    for g, (logits, enc_lens, labels, label_lens) in zip(arr, problems):
        B, T = _ctc_args("ctc_nll_train_groups", logits, enc_lens, labels, label_lens)
        SM = 2 * labels.size(1) + 2
        dev = logits.device
        nll, nllp = torch.empty((B,), dtype=torch.float32, device=dev), torch.empty((B,), dtype=torch.float32, device=dev)
        work, alpha, beta = (torch.empty((B, T, SM), dtype=torch.float32, device=dev) for _ in range(3))
        lse = torch.empty((B, T), dtype=torch.float32, device=dev)
        g.logits, g.ld, g.B, g.T, g.Umax = logits.data_ptr(), logits.stride(1), B, T, labels.size(1)
        g.enc_lens, g.labels, g.label_lens = enc_lens.data_ptr(), labels.data_ptr(), label_lens.data_ptr()
        g.work, g.alpha, g.lse, g.nll, g.nll_shifted, g.beta = work.data_ptr(), alpha.data_ptr(), lse.data_ptr(), nll.data_ptr(), nllp.data_ptr(), beta.data_ptr()
        outs.append((nll, (work, alpha, lse, nllp, beta)))
    _c.call("cfm_ctc_nll_train_groups", arr, n, V)
    return outs


def ctc_grad(logits, V, enc_lens, labels, label_lens, state, gscale=1.0, gscale_dev=None, out=None):
    """d (sum_b nll_b) / d logits * gscale * (*gscale_dev), f32 [B,T,ld], from one micro-batch's state of ctc_nll_train_groups."""
    _c.require_hip(gscale_dev, out)
    B, T = _ctc_args("ctc_grad", logits, enc_lens, labels, label_lens)
    work, alpha, lse, nllp, beta = state
    n = B * T * (2 * labels.size(1) + 2)
    _want("ctc_grad", "state must be the float32 (work, alpha, lse, nll_shifted, beta) of ctc_nll_train_groups for these logits",
          work=(work, _F32, n), alpha=(alpha, _F32, n), lse=(lse, _F32, B * T), nll_shifted=(nllp, _F32, B), beta=(beta, _F32, n), gscale_dev=_opt(gscale_dev, None, None))
    if out is None:
        out = torch.empty_like(logits)
    if out.dtype != torch.float32 or out.shape != logits.shape or out.stride() != logits.stride():
        raise ValueError("cfm.ctc_grad: out must match logits")
    _c.call("cfm_ctc_grad", _c.ptr(logits), logits.stride(1), B, T, V, _c.ptr(enc_lens), _c.ptr(labels), labels.size(1), _c.ptr(label_lens),
            _c.ptr(work), _c.ptr(alpha), _c.ptr(beta), _c.ptr(lse), _c.ptr(nllp), gscale, _c.ptr(gscale_dev), _c.ptr(out))
    return out


class RnntState:
    """What cfm_rnnt_grad / cfm_rnnt_packed_grad need after rnnt_nll / rnnt_nll_packed: the filled descriptor, the tensors its pointers refer to
    (kept alive here) and the leading shape of the gradient, rows = (B, T, U+1) padded or (M,) packed."""

    def __init__(self, desc, logits, tensors, rows):
        self.desc, self.logits, self.tensors, self.rows = desc, logits, tensors, rows

    @property
    def packed(self):
        return isinstance(self.desc, _c.RnntPackedDesc)

    def __getattr__(self, name):
        t = self.__dict__.get("tensors")
        if t is not None and name in t:
            return t[name]
        raise AttributeError(name)


def _rnnt_vocab(what, logits, V):
    W = logits.shape[-1]
    V = W if V is None else V
    if not 1 < V <= W:
        raise ValueError("cfm.%s: V = %d with %d columns" % (what, V, W))
    return V


def _rnnt_padded_args(what, logits, targets, logit_lens, target_lens):
    """The operands of the padded RNN-T entries: logits [B,T,U+1,>=V] with evenly spaced rows, targets int32 [B,U], lengths int32 [B].
    -> (B, T, U1, row stride)."""
    _c.require_hip(logits, targets, logit_lens, target_lens)
    if logits.dim() != 4 or logits.stride(3) != 1:
        raise ValueError("cfm.%s: logits must be [B,T,U+1,V] with unit inner stride, got %s strides %s" % (what, tuple(logits.shape), logits.stride()))
    B, T, U1 = logits.shape[:3]
    ld = logits.stride(2)
    if logits.stride(1) != U1 * ld or logits.stride(0) != T * U1 * ld:
        raise ValueError("cfm.%s: logits rows must be evenly spaced (strides %s)" % (what, logits.stride(),))
    _layout(what, "to match logits %s" % (tuple(logits.shape),), targets=(targets, _I32, (B, U1 - 1)), **_i32(B, logit_lens=logit_lens, target_lens=target_lens))
    return B, T, U1, ld


def _rnnt_packed_args(what, logits, targets, lat):
    """The operands of the packed RNN-T entries: logits [M, >=V], targets int32 [B, >= max U] contiguous."""
    _c.require_hip(logits, targets)
    if logits.dim() != 2 or logits.stride(1) != 1 or logits.shape[0] != lat.M:
        raise ValueError("cfm.%s: logits must be [M=%d, V] with unit inner stride, got %s strides %s" % (what, lat.M, tuple(logits.shape), logits.stride()))
    _layout(what, targets=(targets, _I32, (lat.B, None)))
    if targets.shape[1] < lat.U1_max - 1:
        raise ValueError("cfm.%s: targets must be int32 [B=%d, >=%d], got %s" % (what, lat.B, lat.U1_max - 1, tuple(targets.shape)))


def _rnnt_state(d, what, logits, ld, V, blank, targets, nodes, B, shift_cols):
    """The part of rnnt_nll / rnnt_nll_packed both layouts share: the V check, the state arrays (nodes: their per-node shape) and the descriptor
    fields common to cfm_rnnt_desc and cfm_rnnt_packed_desc.  An empty array gets nll's address (the C checks want a pointer; nothing is read),
    empty targets none."""
    V = _rnnt_vocab(what, logits, V)
    dev = logits.device
    f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    tens = dict(lse=f(*nodes), lp_blank=f(*nodes), lp_label=f(*nodes), alpha=f(*nodes), beta=f(*nodes), shift=f(B, shift_cols), nll=f(B),
                nll_shifted=f(B), ll_alpha=f(B), targets=targets)
    d.logits, d.ld, d.logits_dtype = logits.data_ptr(), ld, _c.dt_code(logits)
    d.V, d.blank = V, blank
    for name in ("targets", "lse", "lp_blank", "lp_label", "alpha", "beta", "shift", "nll", "nll_shifted", "ll_alpha"):
        t = tens[name]
        setattr(d, name, t.data_ptr() if t.numel() else None if name == "targets" else tens["nll"].data_ptr())
    return tens


def rnnt_nll(logits, targets, logit_lens, target_lens, blank, V=None):
    """RNN-T negative log-likelihood per utterance from UN-normalised logits [B,T,U+1,>=V] (rows evenly spaced, unit inner stride; f32 / bf16 /
    fp16), targets int32 [B,U], logit_lens / target_lens int32 [B] (include/cfm.h cfm_rnnt_nll).  V defaults to logits.size(3) (pass it when the
    last axis holds pad columns).  Returns (nll f32 [B], RnntState) -- the state carries lse / lp_blank / lp_label / alpha / beta / shift /
    nll_shifted / ll_alpha for rnnt_grad and for tests."""
    B, T, U1, ld = _rnnt_padded_args("rnnt_nll", logits, targets, logit_lens, target_lens)
    d = _c.RnntDesc()
    tens = _rnnt_state(d, "rnnt_nll", logits, ld, V, blank, targets, (B, T, U1), B, T + U1)
    tens.update(logit_lens=logit_lens, target_lens=target_lens)
    d.B, d.T, d.U1 = B, T, U1
    d.logit_lens, d.target_lens = logit_lens.data_ptr(), target_lens.data_ptr()
    _c.call("cfm_rnnt_nll", ctypes.byref(d))
    return tens["nll"], RnntState(d, logits, tens, (B, T, U1))


def rnnt_grad(state, out, gscale=1.0, gscale_dev=None, clamp=-1.0, cols=None):
    """d nll_b / d logits (clamped to +-clamp when clamp > 0) times gscale * gscale_dev (a device scalar, or [B] per utterance) into `out`, after
    rnnt_nll ([B,T,U+1,>=cols], rows evenly spaced) or rnnt_nll_packed ([M, >=cols]); f32 / bf16 / fp16 with unit inner stride, and may be the
    logits buffer itself (include/cfm.h cfm_rnnt_grad / cfm_rnnt_packed_grad).  Columns 0..cols-1 are written (default: all of out's last
    axis); V..cols-1 and every row outside the lattice get exact zeros.  Returns out."""
    _c.require_hip(out, gscale_dev)
    d, rows = state.desc, state.rows
    if out.dim() != len(rows) + 1 or out.stride(-1) != 1 or tuple(out.shape[:-1]) != rows:
        raise ValueError("cfm.rnnt_grad: out must be [%s, cols] with unit inner stride, got %s" % (",".join(map(str, rows)), tuple(out.shape)))
    if state.packed:
        if not d.lat.M:
            return out
        B, ldg = d.lat.B, out.stride(0)
    else:
        B, ldg = d.B, out.stride(2)
        if out.stride(1) != d.U1 * ldg or out.stride(0) != d.T * d.U1 * ldg:
            raise ValueError("cfm.rnnt_grad: out rows must be evenly spaced (strides %s)" % (out.stride(),))
    d.grad, d.ld_grad, d.grad_dtype = out.data_ptr(), ldg, _c.dt_code(out)
    d.grad_cols = out.size(-1) if cols is None else cols
    d.gscale, d.clamp = float(gscale), float(clamp)
    if gscale_dev is not None:
        if gscale_dev.dtype != torch.float32 or not gscale_dev.is_contiguous() or gscale_dev.numel() not in (1, B):
            raise ValueError("cfm.rnnt_grad: gscale_dev must be a contiguous float32 scalar or [B]")
        d.gscale_dev, d.gscale_stride = gscale_dev.data_ptr(), 1 if gscale_dev.numel() == B and B > 1 else 0
    else:
        d.gscale_dev, d.gscale_stride = None, 0
    if state.packed:
        _c.call("cfm_rnnt_packed_grad", ctypes.byref(d))
    else:
        _c.call("cfm_rnnt_grad", ctypes.byref(d))
    d.grad, d.gscale_dev = None, None
    return out


def joint_act_bwd(enc, pred, dact, B, T, U):
    """Backward of cfm_joint_act: (d_enc f32 [B*T,J], d_pred f32 [B*U,J]) from dact f32 [B*T*U, J] (include/cfm.h cfm_joint_act_bwd)."""
    _c.require_hip(enc, pred, dact)
    enc, pred = _rows2d(enc, "joint_act_bwd(enc)"), _rows2d(pred, "joint_act_bwd(pred)")
    J = enc.shape[1]
    if enc.dtype != torch.float32 or pred.dtype != torch.float32 or tuple(enc.shape) != (B * T, J) or tuple(pred.shape) != (B * U, J):
        raise ValueError("cfm.joint_act_bwd: enc must be f32 [%d,J] and pred f32 [%d,J], got %s %s" % (B * T, B * U, tuple(enc.shape), tuple(pred.shape)))
    _layout("joint_act_bwd", dact=(dact, _F32, (B * T * U, J)))
    de = torch.empty((B * T, J), dtype=torch.float32, device=enc.device)
    dp = torch.empty((B * U, J), dtype=torch.float32, device=enc.device)
    ws = scratch("joint_act_bwd", _c.lib().cfm_joint_act_bwd_ws(B, T, U, J), torch.float32, enc.device)
    _c.call("cfm_joint_act_bwd", enc.data_ptr(), enc.stride(0), pred.data_ptr(), pred.stride(0), dact.data_ptr(), de.data_ptr(), dp.data_ptr(),
            ws.data_ptr(), B, T, U, J)
    return de, dp


def joint_act_packed(enc, pred, lat, out_dtype):
    """tanh(enc[enc_row0[b]+t] + pred[pred_row0[b]+u]) for the valid cells of a packed lattice (cfm.lattice.Lattice) as a row-major [M, J]
    operand (include/cfm.h cfm_joint_act_packed).  enc f32 [n_enc, J], pred f32 [n_pred, J] with unit inner stride."""
    _c.require_hip(enc, pred)
    enc, pred = _rows2d(enc, "joint_act_packed(enc)"), _rows2d(pred, "joint_act_packed(pred)")
    J, d = enc.shape[1], lat.desc
    if enc.dtype != torch.float32 or pred.dtype != torch.float32 or tuple(enc.shape) != (d.n_enc, J) or tuple(pred.shape) != (d.n_pred, J):
        raise ValueError("cfm.joint_act_packed: enc must be f32 [%d,J] and pred f32 [%d,J], got %s %s" % (d.n_enc, d.n_pred, tuple(enc.shape), tuple(pred.shape)))
    out = torch.empty((lat.M, J), dtype=out_dtype, device=enc.device)
    _c.call("cfm_joint_act_packed", _c.ptr(enc), enc.stride(0), _c.ptr(pred), pred.stride(0), _c.ptr(out), _c.dt_code(out), ctypes.byref(d), J)
    return out


def joint_act_packed_bwd(enc, pred, dact, lat):
    """Backward of cfm_joint_act_packed: (d_enc f32 [n_enc,J], d_pred f32 [n_pred,J]) from dact f32 [M, J]; rows outside the lattice are exact
    zeros (include/cfm.h cfm_joint_act_packed_bwd)."""
    _c.require_hip(enc, pred, dact)
    enc, pred = _rows2d(enc, "joint_act_packed_bwd(enc)"), _rows2d(pred, "joint_act_packed_bwd(pred)")
    J, d = enc.shape[1], lat.desc
    if enc.dtype != torch.float32 or pred.dtype != torch.float32 or tuple(enc.shape) != (d.n_enc, J) or tuple(pred.shape) != (d.n_pred, J):
        raise ValueError("cfm.joint_act_packed_bwd: enc must be f32 [%d,J] and pred f32 [%d,J], got %s %s" % (d.n_enc, d.n_pred, tuple(enc.shape), tuple(pred.shape)))
    _layout("joint_act_packed_bwd", dact=(dact, _F32, (lat.M, J)))
    de = torch.empty((d.n_enc, J), dtype=torch.float32, device=enc.device)
    dp = torch.empty((d.n_pred, J), dtype=torch.float32, device=enc.device)
    ws = torch.empty((max(lat.n_blk, 1), J), dtype=torch.float32, device=enc.device)
    _c.call("cfm_joint_act_packed_bwd", enc.data_ptr(), enc.stride(0), pred.data_ptr(), pred.stride(0), dact.data_ptr(), de.data_ptr(),
            dp.data_ptr(), ws.data_ptr(), ctypes.byref(d), J)
    return de, dp


def rnnt_nll_packed(logits, targets, lat, blank, V=None):
    """RNN-T negative log-likelihood per utterance over a packed lattice (cfm.lattice.Lattice): UN-normalised logits [M, >=V] (unit inner stride;
    f32 / bf16 / fp16), targets int32 [B, >= max U] contiguous (include/cfm.h cfm_rnnt_packed_nll).  Returns (nll f32 [B], RnntState) as rnnt_nll;
    the state's lse / lp_blank / lp_label / alpha / beta are [M]."""
    _rnnt_packed_args("rnnt_nll_packed", logits, targets, lat)
    M = lat.M
    d = _c.RnntPackedDesc()
    tens = _rnnt_state(d, "rnnt_nll_packed", logits, logits.stride(0), V, blank, targets, (M,), lat.B, lat.T_max + lat.U1_max)
    tens["lattice"] = lat
    if not M:                                                          # no node: nothing is read, but the row-pass checks want a pointer
        d.logits, d.ld = tens["nll"].data_ptr(), d.V
    d.lat, d.ld_targets = lat.desc, targets.shape[1]
    _c.call("cfm_rnnt_packed_nll", ctypes.byref(d))
    return tens["nll"], RnntState(d, logits, tens, (M,))


def _rnnt_align(ad, what, logits, ld, V, blank, targets, nodes, B, Umax, out):
    """What rnnt_align / rnnt_align_packed share: the V check, the outputs (checked when the caller owns them), the work arrays from the arena
    (lse, lp_blank, lp_label [nodes], the recorded moves) and the descriptor fields both layouts have."""
    r, dev = ad.r, logits.device
    r.V, r.blank = _rnnt_vocab(what, logits, V), blank
    if out is None:
        out = (torch.empty((B, Umax), dtype=_I32, device=dev), torch.empty((B, Umax), dtype=_F32, device=dev), torch.empty((B,), dtype=_F32, device=dev))
    frame, token_logp, score = out
    _want(what, "out must be (frame int32 [B,Umax], token_logp float32 [B,Umax], score float32 [B]) with B = %d, Umax = %d" % (B, Umax),
          frame=(frame, _I32, (B, Umax)), token_logp=(token_logp, _F32, (B, Umax)), score=(score, _F32, (B,)))
    nbytes = int(_c.lib().cfm_rnnt_align_scratch_bytes(nodes))
    work = scratch("rnnt_align_work", 3 * nodes, _F32, dev)
    moves = scratch("rnnt_align_moves", nbytes, torch.uint8, dev)
    r.logits, r.ld, r.logits_dtype = logits.data_ptr(), ld, _c.dt_code(logits)
    r.targets = targets.data_ptr() if targets.numel() else None
    r.lse, r.lp_blank, r.lp_label = (work.data_ptr() + 4 * k * nodes for k in range(3))
    ad.frame, ad.token_logp, ad.score = _c.ptr(frame) or None, _c.ptr(token_logp) or None, _c.ptr(score)
    ad.scratch, ad.scratch_bytes = _c.ptr(moves) or None, nbytes
    return frame, token_logp, score


def rnnt_align(logits, targets, logit_lens, target_lens, blank, V=None, out=None):
    """RNN-T forced alignment: the best single alignment of each utterance's frames to its labels over the transducer lattice, from UN-normalised
    logits [B,T,U+1,>=V] (as rnnt_nll takes them: rows evenly spaced, unit inner stride, f32 / bf16 / fp16), targets int32 [B,U], logit_lens /
    target_lens int32 [B].  Returns (frame int32 [B,U], token_logp f32 [B,U], score f32 [B]) on the device: frame[b,u] the frame at which label u
    is emitted (nondecreasing in u), token_logp its log-probability there, score the path's log-probability; -1 / -inf beyond target_lens[b], and
    score -inf with that fill everywhere for an utterance without a frame.  out: such a tuple to write into.  include/cfm.h cfm_rnnt_align states
    the recursion and its tie rule."""
    B, T, U1, ld = _rnnt_padded_args("rnnt_align", logits, targets, logit_lens, target_lens)
    ad = _c.RnntAlignDesc()
    res = _rnnt_align(ad, "rnnt_align", logits, ld, V, blank, targets, B * T * U1, B, U1 - 1, out)
    ad.r.B, ad.r.T, ad.r.U1 = B, T, U1
    ad.r.logit_lens, ad.r.target_lens = logit_lens.data_ptr(), target_lens.data_ptr()
    _c.call("cfm_rnnt_align", ctypes.byref(ad))
    return res


def rnnt_align_packed(logits, targets, lat, blank, V=None, out=None):
    """rnnt_align over a packed lattice (cfm.lattice.Lattice): logits [M, >=V] hold the valid nodes only, targets int32 [B, >= max U] contiguous
    (include/cfm.h cfm_rnnt_packed_align).  Returns (frame int32 [B,U1_max-1], token_logp f32 [B,U1_max-1], score f32 [B]) -- the same bits as
    rnnt_align on the same nodes."""
    _rnnt_packed_args("rnnt_align_packed", logits, targets, lat)
    ad = _c.RnntPackedAlignDesc()
    res = _rnnt_align(ad, "rnnt_align_packed", logits, logits.stride(0), V, blank, targets, lat.M, lat.B, lat.U1_max - 1, out)
    if not lat.M:                                                      # no node: nothing is read, but the row-pass checks want a pointer
        ad.r.logits, ad.r.ld = res[2].data_ptr(), ad.r.V
    ad.r.lat, ad.r.ld_targets = lat.desc, targets.shape[1]
    _c.call("cfm_rnnt_packed_align", ctypes.byref(ad))
    return res


def adam_step(p, g, m, v, lr, betas, eps, weight_decay, step, grad_scale=None):
    """In-place Adam over flat float32 buffers (torch.optim.Adam's update rule); grad_scale: optional device scalar multiplied into g."""
    n = p.numel()
    _want("adam_step", "p, g, m, v are float32 buffers of one size", p=(p, _F32, n), g=(g, _F32, n), m=(m, _F32, n), v=(v, _F32, n), grad_scale=_opt(grad_scale, None, None))
    _c.call("cfm_adam_step", _c.ptr(p), _c.ptr(g), _c.ptr(m), _c.ptr(v), n, lr, betas[0], betas[1], eps, weight_decay, step, _c.ptr(grad_scale))


def adam_clip_step(p, g, m, v, lr, betas, eps, weight_decay, step, sumsq_t, clip, inv_world, zero_grad=True):
    """adam_step with the clip coefficient computed on the device from `sumsq_t` (cfm.sumsq of g), the 1/world averaging and the zeroing of g in
    the same launch (include/cfm.h cfm_adam_clip_step).  Returns the averaged gradient's norm as a 1-element device tensor, or None when
    sumsq_t is None (clip off: the kernel has nothing to take a norm from)."""
    n = p.numel()
    _want("adam_clip_step", "p, g, m, v are float32 buffers of one size", p=(p, _F32, n), g=(g, _F32, n), m=(m, _F32, n), v=(v, _F32, n), sumsq=_opt(sumsq_t, None, None))
    norm = None if sumsq_t is None else torch.empty((1,), dtype=torch.float32, device=p.device)
    _c.call("cfm_adam_clip_step", _c.ptr(p), _c.ptr(g), _c.ptr(m), _c.ptr(v), n, lr, betas[0], betas[1], eps, weight_decay, step, _c.ptr(sumsq_t),
            float(clip or 0.0), float(inv_world), 1 if zero_grad else 0, _c.ptr(norm))
    return norm


def sumsq(x):
    """sum(x^2) of a flat float32 buffer as a 1-element device tensor (no host sync)."""
    _want("sumsq", x=(x, _F32, None))
    n = x.numel()
    nb = max(1, min(1024, (n + 4095) // 4096))
    part = scratch("sumsq", nb, torch.float32, x.device)
    out = torch.empty((1,), dtype=torch.float32, device=x.device)
    _c.call("cfm_sumsq", _c.ptr(x), n, _c.ptr(part), nb, _c.ptr(out))
    return out


def dropout_rows(x, out_dtype, alpha=1.0, drop=None, drop2=None, row_mask=None):
    """y = alpha * x * keep(seed, element) / (1 - p), rows with row_mask == 0 zeroed: the gradient of a residual branch
    x + alpha * dropout(f) as a GEMM operand (include/cfm.h cfm_dropout_rows).  drop / drop2 = (p, seed) or None."""
    _c.require_hip(x, row_mask)
    M, N = _rows2d(x, "dropout_rows(x)").shape
    _layout("dropout_rows", x=(x, None, None), row_mask=_opt(row_mask, None, M))
    if row_mask is not None and row_mask.element_size() != 1:
        raise ValueError("cfm.dropout_rows: row_mask is one byte per row, got %s" % row_mask.dtype)
    y = torch.empty((M, N), dtype=out_dtype, device=x.device)
    p1, s1 = (float(drop[0]), int(drop[1]) & 0xFFFFFFFF) if drop is not None else (0.0, 0)
    p2, s2 = (float(drop2[0]), int(drop2[1]) & 0xFFFFFFFF) if drop2 is not None else (0.0, 0)
    _c.call("cfm_dropout_rows", _c.ptr(x), _c.dt_code(x), _c.ptr(y), _c.dt_code(y), _c.ptr(row_mask), alpha, p1, s1, p2, s2, M, N)
    return y


def dropout_mask(n, p, seed, device):
    """the 0/1 keep mask the kernels regenerate for (p, seed) over element indices 0..n-1 (bool tensor; for tests)."""
    out = torch.empty((n,), dtype=torch.uint8, device=device)
    _c.require_hip(out)
    _c.call("cfm_dropout_mask", _c.ptr(out), n, float(p), int(seed) & 0xFFFFFFFF)
    return out.view(torch.bool)


# ----------------------------------------------------------------------------------------------------------------------
# per-stream streaming state (include/cfm.h, csrc/stream.hip)
# ----------------------------------------------------------------------------------------------------------------------
def stream_prep(offsets, T, need, ring_T, pe, slot_mask, pos_rows, abs_rows=None, frame_lens=None, out_lens=None):
    """offsets int32 [B] -> slot_mask u8 [B,ring_T], pos_rows f32 [B,ring_T,D] (= pe[frame held by the slot]), abs_rows f32 [B,D] = pe[offset].
    frame_lens int32 [B] (with out_lens int32 [B]): per-stream window lengths in feature frames; out_lens receives the encoder frames c_b of each
    stream and the mask / rows cover the cached frames and those c_b (include/cfm.h cfm_stream_prep)."""
    B = offsets.numel()
    D = pe.shape[-1]
    _want("stream_prep", "offsets int32 [B], pe f32 [max_len,D], slot_mask [B,ring_T], pos_rows [B,ring_T,D]", offsets=(offsets, _I32, None), pe=(pe, _F32, None),
          slot_mask=(slot_mask, None, B * ring_T), pos_rows=(pos_rows, None, B * ring_T * D), abs_rows=_opt(abs_rows, None, None),
          frame_lens=_opt(frame_lens, _I32, B), out_lens=_opt(out_lens, _I32, B))
    if (frame_lens is None) != (out_lens is None):
        raise ValueError("cfm.stream_prep: frame_lens and out_lens come together")
    _c.call("cfm_stream_prep", _c.ptr(offsets), _c.ptr(frame_lens), _c.ptr(out_lens), B, T, need, ring_T, _c.ptr(pe), pe.numel() // D, D,
            _c.ptr(slot_mask), _c.ptr(pos_rows), _c.ptr(abs_rows))


def stream_advance(offsets, T, active=None, lens=None, y=None):
    """offsets[b] += T (active streams), or -- lens int32 [B] -- += lens[b], with rows t >= lens[b] of y f32 [B,T,D] (optional) set to zero."""
    B = offsets.numel()
    _want("stream_advance", offsets=(offsets, None, None), active=_opt(active, None, None), lens=_opt(lens, _I32, B), y=_opt(y, _F32, (B, T, None)))
    if lens is not None and active is not None:
        raise ValueError("cfm.stream_advance: active is not combined with lens")
    if y is not None and lens is None:
        raise ValueError("cfm.stream_advance: y comes with lens")
    D = y.shape[2] if y is not None else 0
    _c.call("cfm_stream_advance", _c.ptr(offsets), _c.ptr(active), _c.ptr(lens), _c.ptr(y), B, T, D)


def dwconv_causal_bn_silu(x, w, dw_bias, bn_scale, bn_shift, cache=None, out_dtype=None):
    """OPT-IN causal depthwise conv + folded BatchNorm + SiLU over [cache | x]; x [B,T,D], cache f32 [B,K-1,D] or None (zeros)."""
    B, T, D = x.shape
    K = w.shape[1]
    _want("dwconv_causal_bn_silu", x=(x, None, (B, T, D)), w=(w, None, None), dw_bias=_opt(dw_bias, None, None), bn_scale=_opt(bn_scale, None, None), bn_shift=_opt(bn_shift, None, None),
          cache=_opt(cache, _F32, (B, K - 1, D)))
    y = torch.empty((B, T, D), dtype=out_dtype or x.dtype, device=x.device)
    _c.call("cfm_dwconv_causal_bn_silu", _c.ptr(x), _c.dt_code(x), _c.ptr(cache), _c.ptr(w), _c.ptr(dw_bias), _c.ptr(bn_scale), _c.ptr(bn_shift), _c.ptr(y),
            _c.dt_code(y), B, T, D, K)
    return y


def conv_cache_update(x, cache, ktaps, lens=None):
    """cache <- the last ktaps-1 frames of [cache | x], or -- lens int32 [B] -- of [cache | x[:lens[b]]] per stream (unchanged at lens[b] = 0)."""
    B, T, D = x.shape
    _want("conv_cache_update", x=(x, None, (B, T, D)), cache=(cache, _F32, (B, ktaps - 1, D)), lens=_opt(lens, _I32, B))
    _c.call("cfm_conv_cache_update", _c.ptr(x), _c.dt_code(x), _c.ptr(cache), _c.ptr(lens), B, T, D, ktaps)


# ----------------------------------------------------------------------------------------------------------------------
# log-mel filter bank (include/cfm.h cfm_fbank / cfm_fbank_stream, csrc/fbank.hip)
# ----------------------------------------------------------------------------------------------------------------------
def _fbank_desc(samples, tables, out, win, shift, padded, dither, seed):
    """tables: (twiddle f64, window f64, mel weights f32, start, length, offset int32) on the device (packing.fbank_tables / pack_mel_banks)."""
    tw, wnd, mw, ms, ml, mo = tables
    _c.require_hip(samples, out, *tables)
    if samples.dim() != 2 or samples.stride(1) != 1 or samples.dtype not in (torch.int16, torch.float32):
        raise ValueError("cfm.fbank: samples must be (B, N) int16 or float32 with unit inner stride, got %s %s" % (tuple(samples.shape), samples.dtype))
    _layout("fbank", twiddle=(tw, None, None), window=(wnd, None, None), mel_w=(mw, None, None), mel_start=(ms, None, None), mel_len=(ml, None, None), mel_off=(mo, None, None),
            out=(out, _F32, (samples.shape[0], None, ms.numel())))
    B, rows, F = out.shape
    d = _c.FbankDesc()
    d.samples, d.ld, d.n_cols, d.samples_i16 = _c.ptr(samples), samples.stride(0) if B > 1 else max(samples.stride(0), samples.shape[1]), samples.shape[1], int(samples.dtype == torch.int16)
    d.twiddle, d.window, d.mel_w, d.mel_start, d.mel_len, d.mel_off, d.mel_nnz = _c.ptr(tw), _c.ptr(wnd), _c.ptr(mw), _c.ptr(ms), _c.ptr(ml), _c.ptr(mo), mw.numel()
    d.out, d.B, d.rows, d.F, d.win, d.shift, d.padded = _c.ptr(out), B, rows, F, win, shift, padded
    d.dither, d.seed = float(dither), int(seed) & 0xFFFFFFFF
    return d


def fbank(samples, lengths, tables, out, feats_length, win, shift, padded, dither=0.0, seed=0):
    """Offline: samples (B, N) int16 | f32, lengths int32 [B] -> out f32 (B, rows, F) (rows past an item's frame count zero), feats_length int32 [B]."""
    d = _fbank_desc(samples, tables, out, win, shift, padded, dither, seed)
    _want("fbank", **_i32(d.B, lengths=lengths, feats_length=feats_length))
    d.lengths, d.feats_length = _c.ptr(lengths), _c.ptr(feats_length)
    _c.call("cfm_fbank", ctypes.byref(d))


def fbank_stream(samples, state_in, state_out, tables, out, win, shift, padded, hop, dither=0.0, seed=0):
    """Streaming: state_* = (carry f32 [B, carry_n], fresh int32 [B], pos int32 [B]); in is read, out is written (the caller swaps them)."""
    d = _fbank_desc(samples, tables, out, win, shift, padded, dither, seed)
    (ci, fi, pi), (co, fo, po) = state_in, state_out
    what = "state is (carry f32 [B, n], fresh int32 [B], pos int32 [B])"
    _want("fbank_stream", what, carry_in=(ci, _F32, None), carry_out=(co, _F32, None), fresh_in=(fi, _I32, None), fresh_out=(fo, _I32, None), pos_in=(pi, _I32, None), pos_out=(po, _I32, None))
    if any(t.shape[0] != d.B for t in (ci, co, fi, fo, pi, po)):                # the leading axis alone, as ever: not an extent _layout states
        raise ValueError("cfm.fbank_stream: %s for B = %d streams" % (what, d.B))
    d.carry_in, d.fresh_in, d.pos_in, d.carry_out, d.fresh_out, d.pos_out = (_c.ptr(t) for t in (ci, fi, pi, co, fo, po))
    d.carry_n, d.hop = ci.shape[1], hop
    _c.call("cfm_fbank_stream", ctypes.byref(d))


def fbank_stream_ragged(samples, n_new, final, state_in, state_out, frame_lens, tables, out, win, shift, padded, hop, dither=0.0, seed=0):
    """Streaming with audio packets of any size (cfm_fbank_stream with n_new set): samples (B, n >= 0), n_new / final int32 [B] on the device (new samples
    per stream, utterance finished); state_* = (carry f32 [B, cap], fresh int32 [B], pos int32 [B], carry_len int32 [B]), in is read, out is written;
    frame_lens int32 [B] receives the rows each stream's window holds (the rest of `out` is written as zeros)."""
    d = _fbank_desc(samples, tables, out, win, shift, padded, dither, seed)
    if len(state_in) != 4 or len(state_out) != 4:
        raise ValueError("cfm.fbank_stream_ragged: state is (carry, fresh, pos, carry_len)")
    (ci, fi, pi, li), (co, fo, po, lo) = state_in, state_out
    _want("fbank_stream_ragged", carry_in=(ci, _F32, (d.B, None)), carry_out=(co, _F32, (d.B, None)),
          **_i32((d.B,), fresh_in=fi, fresh_out=fo, pos_in=pi, pos_out=po, carry_len_in=li, carry_len_out=lo, n_new=n_new, final=final, frame_lens=frame_lens))
    n_first = (d.rows - 1) * shift + win
    if ci.shape != co.shape or ci.shape[1] < n_first - 1:
        raise ValueError("cfm.fbank_stream_ragged: the carry buffers are two f32 [%d, >= %d], got %s and %s" % (d.B, n_first - 1, tuple(ci.shape), tuple(co.shape)))
    if len({t.data_ptr() for t in (ci, co)}) != 2 or len({t.data_ptr() for t in (fi, fo, pi, po, li, lo, n_new, final, frame_lens)}) != 9:
        raise ValueError("cfm.fbank_stream_ragged: state in and out (and the length buffers) must not alias")
    d.carry_in, d.fresh_in, d.pos_in, d.carry_len_in, d.carry_out, d.fresh_out, d.pos_out, d.carry_len_out = (_c.ptr(t) for t in (ci, fi, pi, li, co, fo, po, lo))
    d.n_new, d.final, d.frame_lens, d.carry_cap, d.hop = _c.ptr(n_new), _c.ptr(final), _c.ptr(frame_lens), ci.shape[1], hop
    _c.call("cfm_fbank_stream", ctypes.byref(d))


# ----------------------------------------------------------------------------------------------------------------------
# sample-rate conversion (include/cfm.h cfm_resample / cfm_resample_stream, csrc/resample.hip)
# ----------------------------------------------------------------------------------------------------------------------
def _resample_io(who, d, samples, out, out_lens):
    """The fields cfm_resample_desc and cfm_resample_group_desc share: samples (B, N) and out (B, cap), each with its own row stride, out_lens int32 [B]."""
    if samples.dim() != 2 or (samples.shape[1] > 0 and samples.stride(1) != 1) or samples.dtype not in (torch.int16, torch.float32):
        raise ValueError("cfm.%s: samples must be (B, N) int16 or float32 with unit inner stride, got %s %s" % (who, tuple(samples.shape), samples.dtype))
    B, N = samples.shape
    if out.dim() != 2 or out.dtype != torch.float32 or out.shape[0] != B or (out.shape[1] > 0 and out.stride(1) != 1):
        raise ValueError("cfm.%s: out must be f32 (%d, cap) with unit inner stride, got %s %s" % (who, B, tuple(out.shape), out.dtype))
    _layout(who, **_i32(B, out_lens=out_lens))
    ld = lambda t: t.stride(0) if B > 1 and t.shape[1] > 0 else max(t.stride(0), t.shape[1])      # noqa: E731
    d.samples, d.ld, d.n_cols, d.samples_i16 = _c.ptr(samples) if N else None, ld(samples), N, int(samples.dtype == torch.int16)
    d.out, d.ld_out, d.cap, d.out_lens, d.B = _c.ptr(out) if out.shape[1] else None, ld(out), out.shape[1], _c.ptr(out_lens), B
    return B


def _resample_desc(who, samples, tables, geometry, out, out_lens):
    """tables: (taps f32, first int32 [n], offset int32 [n + 1]) on the device (packing.resample_tables); geometry: (o, n, width)."""
    taps, first, off = tables
    o, n, width = geometry
    _c.require_hip(samples, out, out_lens, *tables)
    d = _c.ResampleDesc()
    _resample_io(who, d, samples, out, out_lens)
    _layout(who, "tables are (taps f32, first int32 [n], offset int32 [n + 1])", taps=(taps, _F32, None), tap_first=(first, _I32, n), tap_off=(off, _I32, n + 1))
    d.taps, d.tap_first, d.tap_off, d.n_live = _c.ptr(taps), _c.ptr(first), _c.ptr(off), taps.numel()
    d.o, d.n, d.width = o, n, width
    return d


def resample(samples, lengths, tables, geometry, out, out_lens):
    """Offline: samples (B, N) int16 | f32, lengths int32 [B] -> out f32 (B, cap) (columns at or beyond an item's ceil(n len / o) samples zero), out_lens int32 [B]."""
    d = _resample_desc("resample", samples, tables, geometry, out, out_lens)
    _want("resample", **_i32(d.B, lengths=lengths))
    d.lengths = _c.ptr(lengths)
    _c.call("cfm_resample", ctypes.byref(d))


def resample_stream(samples, n_new, final, state_in, state_out, tables, geometry, out, out_lens):
    """Streaming: samples (B, n >= 0), n_new / final int32 [B] on the device; state_* = (tail f32 [B, tail_cap], counts int64 [B, 2] = (samples seen, blocks
    emitted)), in is read, out is written (the caller swaps them).  out f32 (B, cap >= 0) receives each stream's new samples left-aligned, out_lens their count."""
    d = _resample_desc("resample_stream", samples, tables, geometry, out, out_lens)
    (ti, ci), (to, co) = state_in, state_out
    _want("resample_stream", tail_in=(ti, _F32, (d.B, None)), tail_out=(to, _F32, (d.B, None)), counts_in=(ci, _I64, (d.B, 2)), counts_out=(co, _I64, (d.B, 2)),
          **_i32((d.B,), n_new=n_new, final=final))
    if ti.shape != to.shape or ti.shape[1] < 2 * d.width + d.o:
        raise ValueError("cfm.resample_stream: the tail buffers are two f32 [%d, >= %d], got %s and %s" % (d.B, 2 * d.width + d.o, tuple(ti.shape), tuple(to.shape)))
    if len({t.data_ptr() for t in (ti, to)}) != 2 or len({t.data_ptr() for t in (ci, co)}) != 2:
        raise ValueError("cfm.resample_stream: state in and out must not alias")
    d.n_new, d.final, d.tail_in, d.tail_out, d.counts_in, d.counts_out, d.tail_cap = _c.ptr(n_new), _c.ptr(final), _c.ptr(ti), _c.ptr(to), _c.ptr(ci), _c.ptr(co), ti.shape[1]
    _c.call("cfm_resample_stream", ctypes.byref(d))


# ----------------------------------------------------------------------------------------------------------------------
# training augmentation (include/cfm.h cfm_resample_group, csrc/resample.hip; cfm_spec_augment, csrc/augment.hip)
# ----------------------------------------------------------------------------------------------------------------------
def resample_group(samples, lengths, bank, tables, banks, out, out_lens):
    """One rate pair per item: samples (B, N) int16 | f32, lengths / bank int32 [B] on the device (bank[b] indexes `banks`), tables = the G banks'
    concatenated (taps f32, first int32, offset int32) on the device or None when every bank is the identity, banks = the host geometry rows
    (o, n, width, n_live, taps_at, first_at, off_at, tile_blocks) (packing.resample_group_tables) -> out f32 (B, cap), out_lens int32 [B]."""
    taps, first, off = tables if tables is not None else (None, None, None)
    _c.require_hip(samples, lengths, bank, out, out_lens, taps, first, off)
    d = _c.ResampleGroupDesc()
    B = _resample_io("resample_group", d, samples, out, out_lens)
    _layout("resample_group", **_i32(B, lengths=lengths, bank=bank))
    if not 1 <= len(banks) <= _c.RESAMPLE_MAX_BANKS:
        raise ValueError("cfm.resample_group: %d banks, 1 .. %d" % (len(banks), _c.RESAMPLE_MAX_BANKS))
    if tables is not None:
        _layout("resample_group", "tables are (taps f32, first int32, offset int32)", taps=(taps, _F32, None), tap_first=(first, _I32, None), tap_off=(off, _I32, None))
        d.taps, d.tap_first, d.tap_off, d.n_taps, d.n_first, d.n_off = _c.ptr(taps), _c.ptr(first), _c.ptr(off), taps.numel(), first.numel(), off.numel()
    elif any(row[0] != row[1] for row in banks):
        raise ValueError("cfm.resample_group: a bank that converts needs the tables")
    d.lengths, d.bank, d.G = _c.ptr(lengths), _c.ptr(bank), len(banks)
    for g, row in enumerate(banks):
        d.banks[g] = _c.ResampleBank(*(int(v) for v in row))
    _c.call("cfm_resample_group", ctypes.byref(d))


def spec_augment(feats, lengths, ids, seed, num_t_mask, num_f_mask, max_t, max_f, masks=None):
    """SpecAugment in place: feats f32 (B, T_max, F) with unit inner stride (any row and item stride), lengths int32 [B], ids int32 [B] read as uint32 or
    None (ids[b] = b), masks int32 (B, num_t_mask + num_f_mask, 2) or None receives (start, end).  include/cfm.h cfm_spec_augment states the draws."""
    _c.require_hip(feats, lengths, ids, masks)
    if feats.dim() != 3 or feats.dtype != torch.float32 or (feats.shape[2] > 1 and feats.stride(2) != 1):
        raise ValueError("cfm.spec_augment: feats must be f32 (B, T_max, F) with unit inner stride, got %s %s strides %s" % (tuple(feats.shape), feats.dtype, feats.stride()))
    B, T, F = feats.shape
    nm = int(num_t_mask) + int(num_f_mask)
    _layout("spec_augment", lengths=(lengths, _I32, B), ids=_opt(ids, _I32, B), masks=_opt(masks, _I32, (B, nm, 2)))
    d = _c.SpecAugmentDesc()
    d.feats, d.lengths, d.ids, d.masks = _c.ptr(feats) if T and F else None, _c.ptr(lengths), _c.ptr(ids), _c.ptr(masks)
    d.row_stride = feats.stride(1) if T > 1 else max(feats.stride(1), F)
    d.item_stride = feats.stride(0) if B > 1 and T > 0 else max(feats.stride(0), T * d.row_stride)
    d.B, d.T_max, d.F, d.num_t_mask, d.num_f_mask, d.max_t, d.max_f, d.seed = B, T, F, int(num_t_mask), int(num_f_mask), int(max_t), int(max_f), int(seed) & 0xFFFFFFFF
    _c.call("cfm_spec_augment", ctypes.byref(d))
    return feats


def _lstm_desc(who, x, weights, H, drop):
    """The shape checks and the fields the forward and the backward share.  weights: per layer (w_ih, w_hh, b_ih | None, b_hh | None)."""
    L = len(weights)
    _layout(who, "x is [B, U, in]", x=(x, _F32, (None, None, None)))
    B, U, I = x.shape
    if not 1 <= L <= 4 or H % 64 or I % 64 or not 64 <= H <= 512 or not 64 <= I <= 512 or B < 1 or U < 1:
        raise ValueError("cfm.%s: 1-4 layers, hidden and input size multiples of 64 up to 512, B >= 1, U >= 1 (layers=%d in=%d H=%d B=%d U=%d): "
                         "there is no other LSTM kernel" % (who, L, I, H, B, U))
    d = _c.LstmDesc()
    d.B, d.U, d.in_, d.H, d.layers = B, U, I, H, L
    if drop is not None and drop[0] > 0.0 and L > 1:
        d.drop_p, d.seed = float(drop[0]), int(drop[1]) & 0xFFFFFFFF
    d.x = _c.ptr(x)
    for l, (w_ih, w_hh, b_ih, b_hh) in enumerate(weights):
        _want(who, "layer %d of float32 weight_ih [4H, in], weight_hh [4H, H], biases [4H]" % l, w_ih=(w_ih, _F32, (4 * H, I if l == 0 else H)), w_hh=(w_hh, _F32, (4 * H, H)),
              b_ih=_opt(b_ih, _F32, 4 * H), b_hh=_opt(b_hh, _F32, 4 * H))
        d.w_ih[l], d.w_hh[l], d.b_ih[l], d.b_hh[l] = _c.ptr(w_ih), _c.ptr(w_hh), _c.ptr(b_ih), _c.ptr(b_hh)
    return d, B, U, I, L


def _lstm_state(who, name, t, L, B, H):
    if t is None:
        return None
    _c.require_hip(t)
    if tuple(t.shape) != (L, B, H) or t.dtype != torch.float32:           # by hand: a strided state is copied, not refused, which _layout does not state
        raise ValueError("cfm.%s: %s must be float32 [layers, B, H] = (%d, %d, %d), got %s %s" % (who, name, L, B, H, tuple(t.shape), t.dtype))
    return t.contiguous()


def lstm_forward(x, weights, H, h0=None, c0=None, drop=None, out=None):
    """nn.LSTM(batch_first=True) over whole sequences (include/cfm.h cfm_lstm_forward): x [B, U, in] f32 -> (y [B, U, H], hn, cn [layers, B, H],
    saves: one f32 block per layer for lstm_backward).  drop = (p, seed): dropout between layers.  out: (y, hn, cn, saves) to write into."""
    _c.require_hip(x, h0, c0)
    d, B, U, I, L = _lstm_desc("lstm_forward", x, weights, H, drop)
    h0, c0 = _lstm_state("lstm_forward", "h0", h0, L, B, H), _lstm_state("lstm_forward", "c0", c0, L, B, H)
    n = int(_c.lib().cfm_lstm_save_floats(B, U, H))
    if out is None:
        y = torch.empty((B, U, H), dtype=torch.float32, device=x.device)
        hn, cn = torch.empty((L, B, H), dtype=torch.float32, device=x.device), torch.empty((L, B, H), dtype=torch.float32, device=x.device)
        saves = [torch.empty(n, dtype=torch.float32, device=x.device) for _ in range(L)]
    else:
        y, hn, cn, saves = out
        what = "out is (y [B,U,H], hn, cn [layers,B,H], %d save blocks of %d floats)" % (L, n)
        if len(saves) != L:
            raise ValueError("cfm.lstm_forward: %s, got %d blocks" % (what, len(saves)))
        _layout("lstm_forward", what, y=(y, None, (B, U, H)), hn=(hn, None, (L, B, H)), cn=(cn, None, (L, B, H)), **{"save%d" % i: (s, None, n) for i, s in enumerate(saves)})
    d.h0, d.c0, d.y, d.hn, d.cn = _c.ptr(h0), _c.ptr(c0), _c.ptr(y), _c.ptr(hn), _c.ptr(cn)
    for l in range(L):
        d.save[l] = _c.ptr(saves[l])
    _c.call("cfm_lstm_forward", ctypes.byref(d))
    return y, hn, cn, saves


def lstm_backward(x, weights, H, saves, dy, dhn=None, dcn=None, drop=None, out=None, work=None):
    """Gradients of lstm_forward (include/cfm.h cfm_lstm_backward) from dy [B, U, H] and optional dhn / dcn [layers, B, H]; drop as in the forward (the mask is
    regenerated).  Returns (dx [B, U, in], [(dw_ih, dw_hh, db_ih | None, db_hh | None) per layer], dh0, dc0).  out: the same structure to write
    into; work: (dg [U*B, 4H], dyl [U*B, H] | None)."""
    _c.require_hip(x, dy, dhn, dcn, *saves)
    d, B, U, I, L = _lstm_desc("lstm_backward", x, weights, H, drop)
    if tuple(dy.shape) != (B, U, H) or dy.dtype != torch.float32:         # by hand, as _lstm_state: a strided dy is copied
        raise ValueError("cfm.lstm_backward: dy must be float32 [B, U, H] = (%d, %d, %d), got %s %s" % (B, U, H, tuple(dy.shape), dy.dtype))
    dy = dy.contiguous()
    dhn, dcn = _lstm_state("lstm_backward", "dhn", dhn, L, B, H), _lstm_state("lstm_backward", "dcn", dcn, L, B, H)
    n = int(_c.lib().cfm_lstm_save_floats(B, U, H))
    if len(saves) != L:
        raise ValueError("cfm.lstm_backward: saves must be the forward's %d blocks of %d floats, got %d blocks" % (L, n, len(saves)))
    _layout("lstm_backward", "saves are the forward's %d blocks of %d floats" % (L, n), **{"save%d" % i: (s, _F32, n) for i, s in enumerate(saves)})
    dev = x.device
    if out is None:
        def e(*shape):
            return torch.empty(shape, dtype=torch.float32, device=dev)
        grads = [(e(*w[0].shape), e(*w[1].shape), None if w[2] is None else e(4 * H), None if w[3] is None else e(4 * H)) for w in weights]
        out = (e(B, U, I), grads, e(L, B, H), e(L, B, H))
    dx, grads, dh0, dc0 = out
    what = "out is (dx [B,U,in], per-layer gradients, dh0, dc0 [layers,B,H])"
    if len(grads) != L:
        raise ValueError("cfm.lstm_backward: %s, got gradients for %d layers" % (what, len(grads)))
    _layout("lstm_backward", what, dx=(dx, None, (B, U, I)), dh0=(dh0, None, (L, B, H)), dc0=(dc0, None, (L, B, H)))
    for l, (gw, w) in enumerate(zip(grads, weights)):
        if any(g_ is not None and w_ is None for g_, w_ in zip(gw, w)):
            raise ValueError("cfm.lstm_backward: layer %d: a gradient for a bias the layer does not have" % l)
        _layout("lstm_backward", "layer %d: a gradient matches its parameter" % l,
                **{k: (g_, _F32, tuple(w_.shape)) for k, g_, w_ in zip(("dw_ih", "dw_hh", "db_ih", "db_hh"), gw, w) if w_ is not None})
        d.dw_ih[l], d.dw_hh[l], d.db_ih[l], d.db_hh[l] = (_c.ptr(g_) for g_ in gw)
        d.save[l] = _c.ptr(saves[l])
    if work is None:
        work = (torch.empty((U * B, 4 * H), dtype=torch.float32, device=dev), torch.empty((U * B, H), dtype=torch.float32, device=dev) if L > 1 else None)
    dg, dyl = work
    _layout("lstm_backward", "work is (dg [U*B, 4H], dyl [U*B, H])", dg=(dg, None, (U * B, 4 * H)), dyl=(dyl, None, (U * B, H)) if L > 1 else None)
    d.dy, d.dhn, d.dcn, d.dx, d.dh0, d.dc0, d.dg, d.dyl = _c.ptr(dy), _c.ptr(dhn), _c.ptr(dcn), _c.ptr(dx), _c.ptr(dh0), _c.ptr(dc0), _c.ptr(dg), _c.ptr(dyl)
    _c.call("cfm_lstm_backward", ctypes.byref(d))
    return dx, grads, dh0, dc0


# ----------------------------------------------------------------------------------------------------------------------
# attention rescoring of n-best lists (csrc/rescore.hip)
# ----------------------------------------------------------------------------------------------------------------------
def rescore_prep(tokens, nlen, score, embed, pe, sos, eos, embed_r=None):
    """Decoder inputs from the device n-best buffers in one launch (include/cfm.h cfm_rescore_prep).  tokens int32 [B,N,Lmax], nlen int32 [B,N],
    score f32 [B,N]; embed (and embed_r: the right decoder's table, for the reversed hypotheses) f32 [V,D], pe f32 [>= Lmax + 1, D].
    Returns (x0 f32 [P*Lc, D], targets int32 [P, Lc], mask uint8 [P, Lc, Lc], x0_r | None, targets_r | None), P = B*N, Lc = Lmax + 1."""
    _c.require_hip(tokens, nlen, score, embed, pe, embed_r)
    _layout("rescore_prep", "tokens is [B,N,Lmax] and embed [V,D]", tokens=(tokens, _I32, (None, None, None)), embed=(embed, _F32, (None, None)))
    (B, N, Lmax), (V, D) = tokens.shape, embed.shape
    _layout("rescore_prep", "[B,N] and D as tokens and embed have them", nlen=(nlen, _I32, (B, N)), score=(score, _F32, (B, N)), pe=(pe, _F32, (None, D)), embed_r=_opt(embed_r, _F32, (V, D)))
    Lc = Lmax + 1
    if pe.shape[0] < Lc:
        raise ValueError("cfm.rescore_prep: %d positions but the position table has %d rows" % (Lc, pe.shape[0]))
    dev, P = tokens.device, B * N
    x0 = torch.empty((P * Lc, D), dtype=torch.float32, device=dev)
    targets = torch.empty((P, Lc), dtype=torch.int32, device=dev)
    mask = torch.empty((P, Lc, Lc), dtype=torch.uint8, device=dev)
    x0_r = torch.empty_like(x0) if embed_r is not None else None
    targets_r = torch.empty_like(targets) if embed_r is not None else None
    d = _c.RescorePrepDesc()
    d.tokens, d.nlen, d.score, d.embed, d.embed_r, d.pe = _c.ptr(tokens) if Lmax else None, _c.ptr(nlen), _c.ptr(score), _c.ptr(embed), _c.ptr(embed_r), _c.ptr(pe)
    d.x0, d.x0_r, d.targets, d.targets_r, d.mask = _c.ptr(x0), _c.ptr(x0_r), _c.ptr(targets), _c.ptr(targets_r), _c.ptr(mask)
    d.B, d.N, d.Lmax, d.D, d.V, d.sos, d.eos = B, N, Lmax, D, V, int(sos), int(eos)
    _c.call("cfm_rescore_prep", ctypes.byref(d))
    return x0, targets, mask, x0_r, targets_r


def token_logprob(x, w, bias, target, V, logits=None, want_lse=False, out=None):
    """logp[m] = log_softmax(x[m] . w^T + bias)[target[m]] over the first V classes, the logits never written (include/cfm.h cfm_token_logprob);
    0 where target < 0.  x [M,D] f32 or w's dtype (unit inner stride), w [Vp,D] bf16 / fp16 dense, bias f32 [Vp], target int32 [M].
    logits f32 [M, >= V] (unit inner stride): the reduction and the gather alone over stored logits (x, w, bias may be None).
    Returns logp f32 [M], or (logp, lse) with want_lse."""
    _c.require_hip(x, w, bias, target, logits, out)
    _layout("token_logprob", w=_opt(w, None, None), bias=_opt(bias, None, None), target=(target, _I32, (None,)), out=_opt(out, _F32, target.numel()))
    M = target.numel()
    d = _c.TokenLogprobDesc()
    if logits is not None:
        logits = _rows2d(logits, "token_logprob(logits)")
        if logits.dtype != torch.float32 or logits.shape[0] != M or logits.shape[1] < V:
            raise ValueError("cfm.token_logprob: logits must be float32 [M = %d, >= V = %d], got %s %s" % (M, V, tuple(logits.shape), logits.dtype))
        d.logits, d.ld = _c.ptr(logits), logits.stride(0) if M > 1 else logits.shape[1]
    else:
        x = _rows2d(x, "token_logprob(x)")
        if w.dim() != 2 or x.shape[1] != w.shape[1] or x.shape[0] != M or w.shape[0] < V or bias.dtype != torch.float32 or bias.numel() < V:
            raise ValueError("cfm.token_logprob: x %s, w %s, bias %s, %d targets, V = %d do not fit" % (tuple(x.shape), tuple(w.shape), tuple(bias.shape), M, V))
        d.X, d.W, d.bias, d.ldx = _c.ptr(x), _c.ptr(w), _c.ptr(bias), x.stride(0) if M > 1 else max(x.stride(0), x.shape[1])
        d.D, d.x_dtype, d.w_dtype = x.shape[1], _c.dt_code(x), _c.dt_code(w)
    logp = out if out is not None else torch.empty((M,), dtype=torch.float32, device=target.device)
    lse = torch.empty((M,), dtype=torch.float32, device=target.device) if want_lse else None
    d.target, d.logp, d.lse, d.M, d.V = _c.ptr(target), _c.ptr(logp), _c.ptr(lse), M, int(V)
    _c.call("cfm_token_logprob", ctypes.byref(d))
    return (logp, lse) if want_lse else logp


def rescore_combine(logp, nlen, score, first_pass_weight, reverse_weight=0.0, logp_r=None):
    """Per-hypothesis sums of the token log-probabilities, the weighted scores and each utterance's ranking in one launch (include/cfm.h
    cfm_rescore_combine).  logp (and logp_r) f32 [B*N*Lc], nlen int32 [B,N], score f32 [B,N].  Returns (final, left, right f32 [B,N],
    order int32 [B,N]: the hypothesis index of each rank) on the device."""
    _want("rescore_combine", "nlen and score are [B,N], logp_r holds as many values as logp", nlen=(nlen, _I32, (None, None)), score=(score, _F32, tuple(nlen.shape)),
          logp=(logp, _F32, None), logp_r=_opt(logp_r, _F32, logp.numel()))
    B, N = nlen.shape
    if logp.numel() % (B * N) or logp.numel() == 0:
        raise ValueError("cfm.rescore_combine: logp holds %d values, not a positive multiple of B*N = %d" % (logp.numel(), B * N))
    dev = logp.device
    final, left, right = (torch.empty((B, N), dtype=torch.float32, device=dev) for _ in range(3))
    order = torch.empty((B, N), dtype=torch.int32, device=dev)
    d = _c.RescoreCombineDesc()
    d.logp, d.logp_r, d.nlen, d.score = _c.ptr(logp), _c.ptr(logp_r), _c.ptr(nlen), _c.ptr(score)
    d.final_score, d.left, d.right, d.order = _c.ptr(final), _c.ptr(left), _c.ptr(right), _c.ptr(order)
    d.B, d.N, d.Lc, d.first_pass_weight, d.reverse_weight = B, N, logp.numel() // (B * N), float(first_pass_weight), float(reverse_weight)
    _c.call("cfm_rescore_combine", ctypes.byref(d))
    return final, left, right, order


# ----------------------------------------------------------------------------------------------------------------------
# label-smoothing loss of the attention decoder (csrc/lsm.hip)
# ----------------------------------------------------------------------------------------------------------------------
def _lsm_operands(op, d, x, w, bias, target, V, logits):
    """The operands that cfm_lsm_loss and cfm_lsm_grad share with cfm_token_logprob, into descriptor d; returns M."""
    _c.require_hip(x, w, bias, target, logits)
    _layout(op, w=_opt(w, None, None), bias=_opt(bias, None, None), target=(target, _I32, (None,)))
    M = target.numel()
    if logits is not None:
        logits = _rows2d(logits, op + "(logits)")
        if logits.dtype != torch.float32 or logits.shape[0] != M or logits.shape[1] < V:
            raise ValueError("cfm.%s: logits must be float32 [M = %d, >= V = %d], got %s %s" % (op, M, V, tuple(logits.shape), logits.dtype))
        d.logits, d.ld = _c.ptr(logits), logits.stride(0) if M > 1 else logits.shape[1]
    else:
        x = _rows2d(x, op + "(x)")
        if w.dim() != 2 or x.shape[1] != w.shape[1] or x.shape[0] != M or w.shape[0] < V or bias.dtype != torch.float32 or bias.numel() < V:
            raise ValueError("cfm.%s: x %s, w %s, bias %s, %d targets, V = %d do not fit" % (op, tuple(x.shape), tuple(w.shape), tuple(bias.shape), M, V))
        d.X, d.W, d.bias, d.ldx = _c.ptr(x), _c.ptr(w), _c.ptr(bias), x.stride(0) if M > 1 else max(x.stride(0), x.shape[1])
        d.D, d.x_dtype, d.w_dtype = x.shape[1], _c.dt_code(x), _c.dt_code(w)
    d.target, d.M, d.V = _c.ptr(target), M, int(V)
    return M


def lsm_loss(x, w, bias, target, V, smoothing, logits=None):
    """Per-row label-smoothing loss over the first V classes of x . w^T + bias, the logits never written (include/cfm.h cfm_lsm_loss): 0 where
    target < 0.  Operands as cfm.token_logprob; logits f32 [M, >= V]: over stored logits (x, w, bias may be None).
    Returns (loss f32 [M], lse f32 [M])."""
    d = _c.LsmLossDesc()
    M = _lsm_operands("lsm_loss", d, x, w, bias, target, V, logits)
    loss = torch.empty((M,), dtype=torch.float32, device=target.device)
    lse = torch.empty((M,), dtype=torch.float32, device=target.device)
    d.loss, d.lse, d.smoothing = _c.ptr(loss), _c.ptr(lse), float(smoothing)
    _c.call("cfm_lsm_loss", ctypes.byref(d))
    return loss, lse


def lsm_grad(x, w, bias, target, V, smoothing, lse, g, logits=None, out=None, out_dtype=None):
    """dz[m, c] = g[m] * (softmax(z_m)[c] - q_c) as [M, Vk], columns V..Vk zero, Vk = V rounded up to 8 (what cfm.gemm wants of a K extent),
    the logits recomputed and never stored (include/cfm.h cfm_lsm_grad).  lse, g f32 [M].  The fused form writes w's dtype; the logits form
    out_dtype (default float32).  out: a [M, >= Vk] tensor with unit inner stride to write into (its first Vk columns)."""
    d = _c.LsmGradDesc()
    M = _lsm_operands("lsm_grad", d, x, w, bias, target, V, logits)
    _want("lsm_grad", "one per row", lse=(lse, _F32, M), g=(g, _F32, M))
    Vk = (int(V) + 7) // 8 * 8
    dt = out.dtype if out is not None else (w.dtype if logits is None else (out_dtype or torch.float32))
    if out is None:
        out = torch.empty((M, Vk), dtype=dt, device=target.device)
    _c.require_hip(out)
    if _rows2d(out, "lsm_grad(out)").shape[0] != M or out.shape[1] < Vk:
        raise ValueError("cfm.lsm_grad: out %s for M = %d rows of Vk = %d columns" % (tuple(out.shape), M, Vk))
    d.lse, d.g, d.dz, d.ldz = _c.ptr(lse), _c.ptr(g), _c.ptr(out), out.stride(0) if M > 1 else max(out.stride(0), out.shape[1])
    d.Vk, d.dz_dtype, d.smoothing = Vk, _c.dt_code(out), float(smoothing)
    _c.call("cfm_lsm_grad", ctypes.byref(d))
    return out[:, :Vk]


def lsm_reduce(loss, target, batch=0):
    """(sum(loss) / denom, denom) as f32 [2] on the device, in a fixed order (include/cfm.h cfm_lsm_reduce): denom = batch, or with batch = 0
    the number of targets >= 0 (at least 1)."""
    _want("lsm_reduce", "one target per row", loss=(loss, _F32, None), target=(target, _I32, loss.numel()))
    out = torch.empty((2,), dtype=torch.float32, device=loss.device)
    _c.call("cfm_lsm_reduce", _c.ptr(loss), _c.ptr(target), loss.numel(), int(batch), _c.ptr(out))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# beam search with the attention decoder (csrc/attn_search.hip)
# ----------------------------------------------------------------------------------------------------------------------
def dec_step_attn(q, store, H, klen=None, slot=None, step=None, kv_new=None, out=None, cap=None, group=1, stride=0):
    """One query per (row, head) over the K | V store (include/cfm.h cfm_dec_step_attn).  q [R, D] (unit inner stride; a column view of the fused
    q|k|v product serves), store [slots, 2 D] dense, of q's dtype.  slot int32 [R, cap']: the table form; slot=None: slot(r, j) = (r // group) *
    stride + j.  klen int32: the key counts, entry r // (R // klen.numel()); klen=None: step[0] + 1 (step int32 [1] on the device).  kv_new
    [R, 2 D] (table form): this step's K | V, stored to slot(r, klen - 1) and attended to.  cap: the declared capacity (default: the table's
    columns, resp. stride).  Returns out [R, D] of q's dtype."""
    _c.require_hip(q, store, slot, klen, step, kv_new, out)
    q = _rows2d(q, "dec_step_attn(q)")
    R, H = q.shape[0], int(H)
    _layout("dec_step_attn", "store is [slots, 2 D] of q's dtype, slot int32 [R, columns], klen and step int32", store=(store, q.dtype, (None, None)),
            slot=_opt(slot, _I32, (R, None)), klen=_opt(klen, _I32, None), step=_opt(step, _I32, 1))
    D = store.shape[1] // 2
    if H < 1 or D % H or q.shape[1] != D or store.shape[1] != 2 * D:
        raise ValueError("cfm.dec_step_attn: q %s, store %s and H = %d do not fit (q [R, D], store [slots, 2 D], D %% H == 0)" % (tuple(q.shape), tuple(store.shape), H))
    if klen is None and step is None:
        raise ValueError("cfm.dec_step_attn: the key counts come from klen or from the device step counter; both are None")
    if klen is not None and (klen.numel() < 1 or R % klen.numel()):
        raise ValueError("cfm.dec_step_attn: %d key counts for %d rows" % (klen.numel(), R))
    if kv_new is not None:
        kv_new = _rows2d(kv_new, "dec_step_attn(kv_new)")
        if tuple(kv_new.shape) != (R, 2 * D) or kv_new.dtype != q.dtype:
            raise ValueError("cfm.dec_step_attn: kv_new must be [%d, %d] of q's dtype, got %s %s" % (R, 2 * D, tuple(kv_new.shape), kv_new.dtype))
    if out is None:
        out = torch.empty((R, D), dtype=q.dtype, device=q.device)
    out = _rows2d(out, "dec_step_attn(out)")
    if tuple(out.shape) != (R, D) or out.dtype != q.dtype:
        raise ValueError("cfm.dec_step_attn: out must be [%d, %d] of q's dtype, got %s %s" % (R, D, tuple(out.shape), out.dtype))
    d = _c.DecStepAttnDesc()
    d.q, d.store, d.slot, d.klen, d.step, d.kv_new, d.out = _c.ptr(q), _c.ptr(store), _c.ptr(slot), _c.ptr(klen), _c.ptr(step), _c.ptr(kv_new), _c.ptr(out)
    d.ldq, d.ld_new, d.ldo, d.slots = q.stride(0) if R > 1 else max(q.stride(0), D), 0 if kv_new is None else (kv_new.stride(0) if R > 1 else max(kv_new.stride(0), 2 * D)), \
        out.stride(0) if R > 1 else max(out.stride(0), D), store.shape[0]
    d.R, d.H, d.dk, d.io_dtype = R, H, D // H, _c.dt_code(q)
    d.slot_ld = 0 if slot is None else slot.shape[1]
    d.group, d.stride = int(group), int(stride)
    d.cap = int(cap) if cap is not None else (d.slot_ld if slot is not None else int(stride))
    d.klen_group = 1 if klen is None else R // klen.numel()
    _c.call("cfm_dec_step_attn", ctypes.byref(d))
    return out


DEC_BEAM_STATE = (("score", _F32), ("token", _I32), ("parent", _I32), ("finished", torch.uint8), ("hlen", _I32), ("klen", _I32))


def dec_beam_prune(topk_idx, topk_logp, state, embed, pe, eos, V):
    """One step's pruning and bookkeeping of the attention decoder's beam search, in place on `state` (include/cfm.h cfm_dec_beam_prune).
    topk_idx int32 / topk_logp f32 [R, k] (cfm.ctc_topk on the step's logits, viewed as rows), R = B * K.  state: a dict of device tensors --
    score f32, token / parent / hlen / klen int32, finished uint8 [R]; tokens, slots int32 [R, Lmax]; x f32 [R, D]; step, max_len int32 [B];
    done uint8 [B]; n_done, all_done int32 [1]; nbest_tokens int32 [B, K, Lmax], nbest_len int32 [B, K], nbest_score f32 [B, K].
    embed f32 [V', D], pe f32 [>= Lmax, D].  Returns state."""
    S = state
    _want("dec_beam_prune", "topk_idx int32 and topk_logp float32 are [R, k]", topk_idx=(topk_idx, _I32, (None, None)), topk_logp=(topk_logp, _F32, tuple(topk_idx.shape)),
          embed=(embed, _F32, (None, None)), nbest_tokens=(S["nbest_tokens"], _I32, (None, None, None)))
    (R, k), (B, K, Lmax), D = topk_idx.shape, S["nbest_tokens"].shape, embed.shape[1]
    if B * K != R:
        raise ValueError("cfm.dec_beam_prune: %d rows of top-k, but the n-best buffers are for %d x %d" % (R, B, K))
    spec = {n: (S[n], dt, (R,)) for n, dt in DEC_BEAM_STATE}
    spec.update(tokens=(S["tokens"], _I32, (R, Lmax)), slots=(S["slots"], _I32, (R, Lmax)), x=(S["x"], _F32, (R, D)), step=(S["step"], _I32, (B,)),
                max_len=(S["max_len"], _I32, (B,)), done=(S["done"], torch.uint8, (B,)), n_done=(S["n_done"], _I32, 1), all_done=(S["all_done"], _I32, 1),
                nbest_len=(S["nbest_len"], _I32, (B, K)), nbest_score=(S["nbest_score"], _F32, (B, K)), pe=(pe, _F32, (None, D)))
    _want("dec_beam_prune", "an entry of state (R = %d rows, B = %d, K = %d, Lmax = %d, D = %d)" % (R, B, K, Lmax, D), **spec)
    if pe.shape[0] < Lmax:
        raise ValueError("cfm.dec_beam_prune: %d positions but the position table has %d rows" % (Lmax, pe.shape[0]))
    d = _c.DecBeamPruneDesc()
    d.topk_idx, d.topk_logp, d.embed, d.pe = _c.ptr(topk_idx), _c.ptr(topk_logp), _c.ptr(embed), _c.ptr(pe)
    for n in ("max_len", "score", "token", "parent", "finished", "hlen", "klen", "tokens", "slots", "x", "step", "done", "n_done", "all_done", "nbest_tokens", "nbest_len",
              "nbest_score"):
        setattr(d, n, _c.ptr(S[n]))
    d.B, d.K, d.k_ld, d.Lmax, d.D, d.V, d.eos = B, K, k, Lmax, D, min(int(V), embed.shape[0]), int(eos)
    _c.call("cfm_dec_beam_prune", ctypes.byref(d))
    return S


def ctc_logprob_t(logits, V, lens, out=None):
    """log_softmax of the CTC head's f32 logits [B, T, ld >= V], CLASS-major: f32 [B, V, Tp], Tp = T rounded up to 4 (include/cfm.h
    cfm_ctc_logprob_t).  lens int32 [B]; elements at t >= lens[b] are not written (out: the tensor to write into; a fresh one is zero-filled)."""
    _c.require_hip(logits, lens, out)
    B, T = _ctc_logits("ctc_logprob_t", logits)
    V, Tp = int(V), (T + 3) // 4 * 4
    if out is None:
        out = torch.zeros((B, V, Tp), dtype=torch.float32, device=logits.device)
    _want("ctc_logprob_t", "out is [B, V, T rounded up to 4]", out=(out, _F32, (B, V, Tp)), **_i32(B, lens=lens))
    _c.call("cfm_ctc_logprob_t", _c.ptr(logits), logits.stride(1), B, T, V, _c.ptr(lens), _c.ptr(out))
    return out


def _ctc_prefix_desc(op, x, T, ctc_state, psi, state, K, ctc_weight, blank, eos):
    """The operands cfm_ctc_prefix_score and cfm_ctc_prefix_advance share: x f32 [B, V, Tp], ctc_state f32 [2, R, Tp, 2], psi f32 [R], and of the
    search state `state` (cfm.dec_beam_prune's dict) token, hlen, finished [R], step, done, lens [B]."""
    S = state
    _want(op, "x is the [B, V, Tp] of ctc_logprob_t", x=(x, _F32, (None, None, None)))
    B, V, Tp = x.shape
    K, T = int(K), int(T)
    R = B * K
    if (T + 3) // 4 * 4 != Tp:
        raise ValueError("cfm.%s: T = %d frames, but x has Tp = %d columns per class (T rounded up to 4)" % (op, T, Tp))
    _want(op, "ctc_state is [2, R, Tp, 2] and psi [R] with R = B * K = %d * %d" % (B, K), ctc_state=(ctc_state, _F32, (2, R, Tp, 2)), psi=(psi, _F32, (R,)),
          token=(S["token"], _I32, (R,)), hlen=(S["hlen"], _I32, (R,)), finished=(S["finished"], torch.uint8, (R,)), step=(S["step"], _I32, (B,)),
          done=(S["done"], torch.uint8, (B,)), lens=(S["lens"], _I32, (B,)))
    d = _c.CtcPrefixDesc()
    d.x, d.state, d.psi = _c.ptr(x), _c.ptr(ctc_state), _c.ptr(psi)
    for n in ("token", "hlen", "finished", "step", "done", "lens"):
        setattr(d, n, _c.ptr(S[n]))
    d.B, d.K, d.T, d.V, d.blank, d.eos, d.ctc_weight = B, K, T, V, int(blank), int(eos), float(ctc_weight)
    return d, R


def ctc_prefix_score(x, T, ctc_state, psi, topk_idx, topk_logp, state, K, ctc_weight, blank, eos, out=None):
    """One step's CTC prefix scores of every row's P attention candidates and the K best combined offers per row (include/cfm.h
    cfm_ctc_prefix_score).  topk_idx int32 / topk_logp f32 [R, P].  Returns (out_idx int32, out_logp f32, cand_psi f32), each [R, K] -- the
    first two are cfm.dec_beam_prune's top-k lists (out: such a triple to write into)."""
    d, R = _ctc_prefix_desc("ctc_prefix_score", x, T, ctc_state, psi, state, K, ctc_weight, blank, eos)
    _want("ctc_prefix_score", "topk_idx int32 and topk_logp float32 are [R, P]", topk_idx=(topk_idx, _I32, (R, None)), topk_logp=(topk_logp, _F32, tuple(topk_idx.shape)))
    if out is None:
        out = (torch.empty((R, d.K), dtype=torch.int32, device=x.device), torch.empty((R, d.K), dtype=torch.float32, device=x.device),
               torch.empty((R, d.K), dtype=torch.float32, device=x.device))
    _want("ctc_prefix_score", "out must be (out_idx int32, out_logp float32, cand_psi float32), each [R, K]", out_idx=(out[0], _I32, (R, d.K)), out_logp=(out[1], _F32, (R, d.K)),
          cand_psi=(out[2], _F32, (R, d.K)))
    d.P = topk_idx.shape[1]
    d.topk_idx, d.topk_logp, d.out_idx, d.out_logp, d.cand_psi = _c.ptr(topk_idx), _c.ptr(topk_logp), _c.ptr(out[0]), _c.ptr(out[1]), _c.ptr(out[2])
    _c.call("cfm_ctc_prefix_score", ctypes.byref(d))
    return out


def ctc_prefix_advance(x, T, ctc_state, psi, state, K, blank, eos):
    """After cfm.dec_beam_prune: the CTC state and psi of every kept unfinished row, from its parent's, into the other half of ctc_state
    (include/cfm.h cfm_ctc_prefix_advance).  state: the prune's dict (parent, token, tokens, hlen, finished, step, done, lens are read)."""
    d, R = _ctc_prefix_desc("ctc_prefix_advance", x, T, ctc_state, psi, state, K, 1.0, blank, eos)
    _want("ctc_prefix_advance", "parent is [R] and tokens [R, Lmax]", parent=(state["parent"], _I32, (R,)), tokens=(state["tokens"], _I32, (R, None)))
    d.P = d.K
    d.parent, d.tokens, d.Lmax = _c.ptr(state["parent"]), _c.ptr(state["tokens"]), state["tokens"].shape[1]
    _c.call("cfm_ctc_prefix_advance", ctypes.byref(d))
    return ctc_state, psi
