"""Device-side weight packing for the HIP kernels.

The nn.Modules keep the reference's parameter names / shapes / dtypes (so state_dicts, optimizers and DDP see what they
expect); the kernels want: 16-bit (or hi/lo bf16 split) [N,K] matrices, a fused QKV matrix, the pointwise-conv-1
rows interleaved for the in-register GLU, BatchNorm folded to scale/shift, conv kernels reordered to the implicit-GEMM K
order.  Everything derived from weights -- packs, launch plans, ctypes structs of raw device pointers -- sits in a Slot on its module and
is rebuilt when weights_key changes: the pack epoch, the precision mode, or a source tensor's address, version counter (in-place
optimizer steps bump it), device or dtype.
"""
import torch

import cfm as _c


_EPOCH = [0]


def bump_epoch():
    """Invalidate every pack: for weight updates that bypass torch's version counters (the flat-buffer Adam kernel of trainer.py writes
    through raw pointers)."""
    _EPOCH[0] += 1


def weights_key(tensors, *extra):
    """THE answer to "have these weights changed?": (pack epoch,) + extra (a precision name, a tag) + (address, version counter, device,
    dtype) per tensor; None entries are skipped.  In-place updates move the version counter, `p.data = ...` / a replaced Parameter / .to()
    the address, device or dtype, raw-pointer writes (bump_epoch) the epoch.  The only reader of the epoch and of the version counters
    besides its cheap variant graph_watch."""
    return (_EPOCH[0],) + extra + tuple((t.data_ptr(), t._version, str(t.device), t.dtype) for t in tensors if t is not None)


def graph_watch(owner):
    """What a captured graph's owner (owner.enc: its encoder) compares before every replay: changes whenever a parameter / buffer of
    owner.enc is updated in place or every pack is invalidated -- the graph holds raw pointers to the PACKED weights of the capture and
    must be re-captured then.  The cheap variant of weights_key: it runs before every replayed step, so it is one attribute read per tensor
    (~50 us for the 12-block encoder) over a tensor list built ONCE per owner, with the addresses summed at that moment (.to() /
    load_state_dict keep storage), where the full key would allocate a 300-tuple per streaming step.
    Its one known limit: a Parameter OBJECT replaced under a captured graph (`blk.norm_ff.weight = nn.Parameter(...)`) is not in the list
    and is not seen until the graph is dropped for another reason."""
    s = slot(owner, "_watch")
    if s.value is None:
        s.value = list(owner.enc.parameters()) + list(owner.enc.buffers())
        s.key = sum(t.data_ptr() for t in s.value)
    v = 0
    for t in s.value:
        v += t._version
    return _EPOCH[0], v, s.key, str(_c.resolve_precision(owner.enc))


def capture_step(run, dev, state, idle=None):
    """run() -- one step of a streaming stage on device buffers -- captured in a HIP graph: returns (graph, what the captured run() returned).
    state: the tensors run() changes (None entries are skipped); they hold their bits from before the call when it returns.  idle: called
    before the warm-up, after the state is saved -- puts the step in a form whose warm-up changes nothing outside `state`.
    One protocol for every captured step: a side stream waits on the current one; on it the state is cloned, idle() and the warm-up run() are
    run, the stream is synchronised, the state is put back, run() is captured ON THAT STREAM and the state is put back again; the current stream
    then waits on the side stream.  Warm-up and capture share a stream because the scratch arena is per (device, stream): a warm-up elsewhere
    would size another stream's arena and leave the capture to allocate.  The graph holds the addresses of everything run() touches: whoever
    replaces one of them drops the graph."""
    state = [t for t in state if t is not None]
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.no_grad(), torch.cuda.stream(stream):
        saved = [t.clone() for t in state]

        def restore():
            for t, s in zip(state, saved):
                t.copy_(s)
        if idle is not None:
            idle()
        run()                                                           # warm-up: sizes this stream's arena, allocator, lazy init
        stream.synchronize()
        restore()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            out = run()
        restore()                                                       # (capture does not execute, but keep the state explicit)
    torch.cuda.current_stream(dev).wait_stream(stream)
    return graph, out


class Packed:
    """Attribute bag of packed tensors (keeps them alive while raw pointers are in flight)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class Slot:
    """One cached value and the key it was built for -- the one way derived state is kept on a module (or on any object with a __dict__).
    A copy (copy.deepcopy, pickle, torch.save) starts EMPTY: ctypes pointers cannot be pickled, a copied pointer would still address the
    original's memory, and the packs belong to the original's tensors."""

    def __init__(self):
        self.key = self.value = None

    def __reduce__(self):
        return (type(self), ())

    def clear(self):
        self.key = self.value = None

    def get(self, key, build):
        if key != self.key:
            with torch.no_grad():
                self.value = build()
            self.key = key
        return self.value


class PackCache(Slot):
    """The slot of a module's weight pack (constructed in the module's __init__), keyed on its source tensors and the precision mode."""

    def get(self, tensors, prec, build):
        return Slot.get(self, weights_key(tensors, prec.name), build)


def slot(mod, name, cls=Slot):
    """The slot mod.__dict__[name], created empty on first use."""
    try:
        return mod.__dict__[name]
    except KeyError:
        return mod.__dict__.setdefault(name, cls())


def f32(t):
    return t.detach().to(torch.float32).contiguous()


def matrix(w, prec):
    """[N,K] float weight -> (W16, W_lo|None)."""
    w32 = w.detach().to(torch.float32)
    if prec.split:
        hi = w32.to(torch.bfloat16)
        lo = (w32 - hi.to(torch.float32)).to(torch.bfloat16)
        return hi.contiguous(), lo.contiguous()
    return w32.to(prec.w_dtype).contiguous(), None


def conv_module_vectors(mod):
    """(pointwise-conv-1 bias [2D], depthwise bias [D], BatchNorm weight [D], BatchNorm bias [D]) of a ConvolutionModule, detached: an absent
    bias reads as zeros, an absent BatchNorm affine as ones / zeros."""
    D = mod.pointwise_conv2.weight.shape[0]
    dev = mod.pointwise_conv2.weight.device
    opt = lambda t, n, fill: t.detach() if t is not None else torch.full((n,), fill, device=dev)
    return opt(mod.pointwise_conv1.bias, 2 * D, 0.0), opt(mod.depthwise_conv.bias, D, 0.0), opt(mod.norm.weight, D, 1.0), opt(mod.norm.bias, D, 0.0)


def glu_interleave_index(D, device):
    """GEMM column blk*32 + half*16 + i  takes weight row  half*D + blk*16 + i  (see gemm.hip epilogue)."""
    idx = torch.arange(2 * D, device=device)
    return ((idx % 32) // 16) * D + (idx // 32) * 16 + (idx % 16)


def pack_ffn_fragments(w1, w2, dtype):
    """Fragment-major packs for the fused FFN kernel (include/cfm.h cfm_ffn_fused, csrc/ffn.hip).

    w1 [FF,D] -> w1f[ffb][kk][lane][j] = w1[ffb*16 + (lane&15)][kk*32 + 8*(lane>>4) + j]           (K zero-padded to 32)
    w2 [D,FF] -> w2f[fs][nf][lane][j]  = w2[nf*16 + (lane&15)][fs*32 + (j<4 ? 0 : 16) + 4*(lane>>4) + (j&3)]
    so that one wavefront-load (lane*16 bytes) is one MFMA A-operand fragment, and the second product's k order is the
    order in which the first product's accumulators hold the hidden activation.
    """
    FF, D = w1.shape
    ks1 = (D + 31) // 32
    w1p = torch.zeros((FF, ks1 * 32), dtype=torch.float32, device=w1.device)
    w1p[:, :D] = w1.detach().float()
    # [ffb, l15, kk, g, j] -> [ffb, kk, g, l15, j]   (lane = g*16 + l15)
    w1f = w1p.view(FF // 16, 16, ks1, 4, 8).permute(0, 2, 3, 1, 4).contiguous().to(dtype)
    # ff = fs*32 + hi*16 + g*4 + r ;  j = hi*4 + r :  [nf, l15, fs, hi, g, r] -> [fs, nf, g, l15, hi, r]
    w2f = w2.detach().float().view(D // 16, 16, FF // 32, 2, 4, 4).permute(2, 0, 4, 1, 3, 5).contiguous().to(dtype)
    return w1f.view(-1), w2f.view(-1)


def pack_frag_major(w, dtype):
    """[N,K] -> 16-bit fragment-major w[nfrag][kk][lane][j] = W[nfrag*16 + (lane&15)][kk*32 + 8*(lane>>4) + j], K zero-padded to a
    multiple of 32 (the operand layout of the row-chain kernels: one wavefront-load of lane*16 B = one MFMA A fragment)."""
    N, K = w.shape
    ks = (K + 31) // 32
    wp = torch.zeros((N, ks * 32), dtype=torch.float32, device=w.device)
    wp[:, :K] = w.detach().float()
    return wp.view(N // 16, 16, ks, 4, 8).permute(0, 2, 3, 1, 4).contiguous().to(dtype).view(-1)


def pack_ffn(mod, prec):
    def build():
        w1, w1l = matrix(mod.w_1.weight, prec)
        w2, w2l = matrix(mod.w_2.weight, prec)
        pk = Packed(w1=w1, w1_lo=w1l, b1=f32(mod.w_1.bias), w2=w2, w2_lo=w2l, b2=f32(mod.w_2.bias), w1f=None, w2f=None, w2n=None)
        FF, D = mod.w_1.weight.shape
        if _c.ffn_fused_supported(D, FF, prec):
            pk.w1f, pk.w2f = pack_ffn_fragments(mod.w_1.weight, mod.w_2.weight, prec.w_dtype)
        if _c.rowchain_supported(D, FF, prec):
            pk.w2n = pack_frag_major(mod.w_2.weight, prec.w_dtype)      # the row chains read W2 in natural k order
            if pk.w1f is None:                                          # (D = 512: no stand-alone fused kernel, the chains only)
                pk.w1f = pack_frag_major(mod.w_1.weight, prec.w_dtype)
        return pk
    return mod._pack.get([mod.w_1.weight, mod.w_1.bias, mod.w_2.weight, mod.w_2.bias], prec, build)


def pack_mhsa(mod, prec, relative):
    srcs = [mod.linear_q.weight, mod.linear_q.bias, mod.linear_k.weight, mod.linear_k.bias, mod.linear_v.weight,
            mod.linear_v.bias, mod.linear_out.weight, mod.linear_out.bias]
    if relative:
        srcs += [mod.linear_pos.weight, mod.pos_bias_u, mod.pos_bias_v]

    def build():
        qkv, qkvl = matrix(torch.cat([mod.linear_q.weight, mod.linear_k.weight, mod.linear_v.weight], 0), prec)
        out, outl = matrix(mod.linear_out.weight, prec)
        p = Packed(qkv_w=qkv, qkv_w_lo=qkvl, qkv_b=f32(torch.cat([mod.linear_q.bias, mod.linear_k.bias, mod.linear_v.bias], 0)),
                   out_w=out, out_w_lo=outl, out_b=f32(mod.linear_out.bias), pos_w=None, pos_w_lo=None, bias_u=None, bias_v=None)
        D = mod.linear_q.weight.shape[0]
        # row views of the fused matrix for the non-self-attention call pattern (query/key/value differ)
        p.q_w, p.k_w, p.v_w = qkv[:D], qkv[D:2 * D], qkv[2 * D:]
        p.q_w_lo, p.k_w_lo, p.v_w_lo = (None, None, None) if qkvl is None else (qkvl[:D], qkvl[D:2 * D], qkvl[2 * D:])
        p.q_b, p.k_b, p.v_b = p.qkv_b[:D], p.qkv_b[D:2 * D], p.qkv_b[2 * D:]
        if relative:
            p.pos_w, p.pos_w_lo = matrix(mod.linear_pos.weight, prec)
            p.bias_u, p.bias_v = f32(mod.pos_bias_u), f32(mod.pos_bias_v)
        p.qkv_wf = p.out_wf = None
        if not prec.split and D % 16 == 0:
            p.qkv_wf = pack_frag_major(torch.cat([mod.linear_q.weight, mod.linear_k.weight, mod.linear_v.weight], 0), prec.w_dtype)
            p.out_wf = pack_frag_major(mod.linear_out.weight, prec.w_dtype)
        return p
    return mod._pack.get(srcs, prec, build)


def pack_conv_module(mod, prec):
    bn = mod.norm
    srcs = [mod.pointwise_conv1.weight, mod.pointwise_conv1.bias, mod.depthwise_conv.weight, mod.depthwise_conv.bias, bn.weight,
            bn.bias, bn.running_mean, bn.running_var, mod.pointwise_conv2.weight, mod.pointwise_conv2.bias]

    def build():
        D = mod.pointwise_conv2.weight.shape[0]
        dev = mod.pointwise_conv2.weight.device
        idx = glu_interleave_index(D, dev)
        w1 = mod.pointwise_conv1.weight.detach()[:, :, 0]
        b1, dwb, gamma, beta = conv_module_vectors(mod)
        pw1, pw1l = matrix(w1[idx], prec)
        pw2, pw2l = matrix(mod.pointwise_conv2.weight.detach()[:, :, 0], prec)
        # BatchNorm1d (eval): y = (x - mean) / sqrt(var + eps) * gamma + beta   ->   x * scale + shift
        scale = gamma.float() / torch.sqrt(bn.running_var.detach().float() + bn.eps)
        shift = beta.float() - bn.running_mean.detach().float() * scale
        pk = Packed(pw1_w=pw1, pw1_w_lo=pw1l, pw1_b=f32(b1[idx]), pw2_w=pw2, pw2_w_lo=pw2l, pw2_b=f32(mod.pointwise_conv2.bias),
                    dw_w=f32(mod.depthwise_conv.weight.detach()[:, 0, :]), dw_b=f32(dwb), bn_scale=f32(scale), bn_shift=f32(shift),
                    pw1_wf=None, pw2_wf=None)
        if not prec.split and D % 16 == 0:
            pk.pw1_wf = pack_frag_major(w1[idx], prec.w_dtype)          # same value/gate interleave as the GEMM path
            pk.pw2_wf = pack_frag_major(mod.pointwise_conv2.weight.detach()[:, :, 0], prec.w_dtype)
        return pk
    return mod._pack.get(srcs, prec, build)


def pack_subsampling(mod, prec):
    c1, c2, lin = mod.conv[0], mod.conv[2], mod.out[0]
    srcs = [c1.weight, c1.bias, c2.weight, c2.bias, lin.weight, lin.bias]

    def build():
        C = c1.weight.shape[0]
        w1 = f32(c1.weight.detach().reshape(C, 9).t())                               # [9, C] tap-major
        w2, w2l = matrix(c2.weight.detach().permute(0, 2, 3, 1).reshape(C, 9 * C), prec)   # [co][kt][kf][ci]
        Dout, CF = lin.weight.shape
        Fp = CF // C
        # reference feature order is c*F'+f (convolution.py:74); the implicit GEMM writes [.., f, c]
        wl, wll = matrix(lin.weight.detach().reshape(Dout, C, Fp).permute(0, 2, 1).reshape(Dout, Fp * C), prec)
        return Packed(w1=w1, b1=f32(c1.bias), w2=w2, w2_lo=w2l, b2=f32(c2.bias), wl=wl, wl_lo=wll, bl=f32(lin.bias), C=C, Fp=Fp)
    return mod._pack.get(srcs, prec, build)


def layer_weight_struct(layer, prec):
    """cfm.LayerWeights for one ConformerEncoderLayer (+ the Packed objects it points into)."""
    relative = layer.use_relative
    ffm = pack_ffn(layer.feed_forward_macaron, prec)
    ff = pack_ffn(layer.feed_forward, prec)
    att = pack_mhsa(layer.self_attn, prec, relative)
    cv = pack_conv_module(layer.conv_module, prec)
    norms = {}
    for short, name in (("ffm", "norm_ff_macaron"), ("mha", "norm_mha"), ("conv", "norm_conv"), ("ff", "norm_ff"), ("final", "norm_final")):
        ln = getattr(layer, name)
        norms[short] = (ln.weight.detach(), ln.bias.detach())
    for g, b in norms.values():
        if g.dtype != torch.float32 or not g.is_contiguous() or not b.is_contiguous():
            raise TypeError("LayerNorm parameters must be contiguous float32")
    w = _c.LayerWeights()
    for short, (g, b) in norms.items():
        setattr(w, "ln_%s_g" % short, g.data_ptr())
        setattr(w, "ln_%s_b" % short, b.data_ptr())
    for pre, pk in (("ffm", ffm), ("ff", ff)):
        setattr(w, pre + "_w1", pk.w1.data_ptr())
        setattr(w, pre + "_w1_lo", _c.ptr(pk.w1_lo))
        setattr(w, pre + "_w2", pk.w2.data_ptr())
        setattr(w, pre + "_w2_lo", _c.ptr(pk.w2_lo))
        setattr(w, pre + "_b1", pk.b1.data_ptr())
        setattr(w, pre + "_b2", pk.b2.data_ptr())
        setattr(w, pre + "_w1f", _c.ptr(pk.w1f))
        setattr(w, pre + "_w2f", _c.ptr(pk.w2f))
        setattr(w, pre + "_w2n", _c.ptr(pk.w2n))
    w.qkv_wf, w.out_wf, w.pw1_wf, w.pw2_wf = _c.ptr(att.qkv_wf), _c.ptr(att.out_wf), _c.ptr(cv.pw1_wf), _c.ptr(cv.pw2_wf)
    w.qkv_w, w.qkv_w_lo, w.qkv_b = att.qkv_w.data_ptr(), _c.ptr(att.qkv_w_lo), att.qkv_b.data_ptr()
    w.pos_w, w.pos_w_lo = _c.ptr(att.pos_w), _c.ptr(att.pos_w_lo)
    w.out_w, w.out_w_lo, w.out_b = att.out_w.data_ptr(), _c.ptr(att.out_w_lo), att.out_b.data_ptr()
    w.bias_u, w.bias_v = _c.ptr(att.bias_u), _c.ptr(att.bias_v)
    w.pw1_w, w.pw1_w_lo, w.pw1_b = cv.pw1_w.data_ptr(), _c.ptr(cv.pw1_w_lo), cv.pw1_b.data_ptr()
    w.pw2_w, w.pw2_w_lo, w.pw2_b = cv.pw2_w.data_ptr(), _c.ptr(cv.pw2_w_lo), cv.pw2_b.data_ptr()
    w.dw_w, w.dw_b, w.bn_scale, w.bn_shift = cv.dw_w.data_ptr(), cv.dw_b.data_ptr(), cv.bn_scale.data_ptr(), cv.bn_shift.data_ptr()
    return w, (ffm, ff, att, cv, norms)


# ----------------------------------------------------------------------------------------------------------------------
# training packs: every dense layer needs its weight twice -- [N,K] for the forward product and [K,N] for the input gradient
# (both K-contiguous for cfm_gemm) -- rebuilt when the optimizer has stepped (the parameter's version counter moves)
# ----------------------------------------------------------------------------------------------------------------------
def matrix_t(w, prec):
    """[N,K] float weight -> the packs of its transpose [K,N]."""
    return matrix(w.detach().t(), prec)


def _train_slot(mod):
    return slot(mod, "_pack_train", PackCache)


def pack_ffn_train(mod, prec):
    def build():
        w1, w1l = matrix(mod.w_1.weight, prec)
        w2, w2l = matrix(mod.w_2.weight, prec)
        w1t, w1tl = matrix_t(mod.w_1.weight, prec)
        w2t, w2tl = matrix_t(mod.w_2.weight, prec)
        return Packed(w1=w1, w1_lo=w1l, b1=f32(mod.w_1.bias), w2=w2, w2_lo=w2l, b2=f32(mod.w_2.bias), w1t=w1t, w1t_lo=w1tl, w2t=w2t, w2t_lo=w2tl)
    return _train_slot(mod).get([mod.w_1.weight, mod.w_1.bias, mod.w_2.weight, mod.w_2.bias], prec, build)


def pack_mhsa_train(mod, prec, relative):
    srcs = [mod.linear_q.weight, mod.linear_q.bias, mod.linear_k.weight, mod.linear_k.bias, mod.linear_v.weight, mod.linear_v.bias,
            mod.linear_out.weight, mod.linear_out.bias]
    if relative:
        srcs.append(mod.pos_bias_u)

    def build():
        wcat = torch.cat([mod.linear_q.weight.detach(), mod.linear_k.weight.detach(), mod.linear_v.weight.detach()], 0)
        qkv, qkvl = matrix(wcat, prec)
        qkvt, qkvtl = matrix_t(wcat, prec)
        out, outl = matrix(mod.linear_out.weight, prec)
        outt, outtl = matrix_t(mod.linear_out.weight, prec)
        bq = mod.linear_q.bias.detach().float()
        if relative:                                   # q + pos_bias_u (attention.py:81) rides in the projection's bias; the batch path's
            bq = bq + mod.pos_bias_u.detach().float().reshape(-1)      # positional term is softmax-invariant and is not evaluated
        qkv_b = torch.cat([bq, mod.linear_k.bias.detach().float(), mod.linear_v.bias.detach().float()], 0).contiguous()
        return Packed(qkv_w=qkv, qkv_w_lo=qkvl, qkv_t=qkvt, qkv_t_lo=qkvtl, qkv_b=qkv_b, out_w=out, out_w_lo=outl, out_t=outt, out_t_lo=outtl,
                      out_b=f32(mod.linear_out.bias))
    return _train_slot(mod).get(srcs, prec, build)


def pack_conv_module_train(mod, prec):
    bn = mod.norm
    srcs = [mod.pointwise_conv1.weight, mod.pointwise_conv1.bias, mod.depthwise_conv.weight, mod.depthwise_conv.bias, bn.weight, bn.bias,
            mod.pointwise_conv2.weight, mod.pointwise_conv2.bias]

    def build():
        D = mod.pointwise_conv2.weight.shape[0]
        idx = glu_interleave_index(D, mod.pointwise_conv2.weight.device)
        w1 = mod.pointwise_conv1.weight.detach()[:, :, 0][idx]
        w2 = mod.pointwise_conv2.weight.detach()[:, :, 0]
        b1, _, _, _ = conv_module_vectors(mod)
        pw1, pw1l = matrix(w1, prec)
        pw1t, pw1tl = matrix_t(w1, prec)
        pw2, pw2l = matrix(w2, prec)
        pw2t, pw2tl = matrix_t(w2, prec)
        return conv_module_train_pack(mod, idx, b1[idx], (pw1, pw1l, pw1t, pw1tl), (pw2, pw2l, pw2t, pw2tl))
    return _train_slot(mod).get(srcs, prec, build)


def conv_module_train_pack(mod, idx, pw1_b, pw1, pw2):
    """The training pack of a ConvolutionModule around its two packed matrices (w, w_lo, w^T, w^T_lo) and the interleaved pointwise-conv-1 bias."""
    _, dwb, gamma, beta = conv_module_vectors(mod)
    return Packed(pw1_w=pw1[0], pw1_w_lo=pw1[1], pw1_t=pw1[2], pw1_t_lo=pw1[3], pw1_b=f32(pw1_b), pw2_w=pw2[0], pw2_w_lo=pw2[1], pw2_t=pw2[2],
                  pw2_t_lo=pw2[3], pw2_b=f32(mod.pointwise_conv2.bias), dw_w=f32(mod.depthwise_conv.weight.detach()[:, 0, :]), dw_b=f32(dwb),
                  gamma=f32(gamma), beta=f32(beta), idx=idx)


class _LayerPackPlan:
    """The matrix jobs of one conformer block's 8 weight matrices (two feed-forwards, fused q|k|v, out-projection, the GLU-interleaved
    pointwise-conv-1, pointwise-conv-2) for cfm_pack_matrices, and their destination tensors: built once (the parameters' addresses do not
    move: the optimizer writes in place).  _StackPackPlan launches the jobs of all blocks together."""

    def __init__(self, layer, prec):
        ffm, att, cv, ff = layer.feed_forward_macaron, layer.self_attn, layer.conv_module, layer.feed_forward
        dev = ffm.w_1.weight.device
        D = cv.pointwise_conv2.weight.shape[0]
        self.idx = glu_interleave_index(D, dev)
        for t in (ffm.w_1.weight, ffm.w_2.weight, att.linear_q.weight, att.linear_k.weight, att.linear_v.weight, att.linear_out.weight,
                  cv.pointwise_conv1.weight, cv.pointwise_conv2.weight, ff.w_1.weight, ff.w_2.weight):
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise TypeError("the training packs need contiguous float32 parameters")
        wdt = torch.bfloat16 if prec.split else prec.w_dtype

        def rows_of(t, n, k, perm=None):
            r = t.data_ptr() + torch.arange(n, device=dev, dtype=torch.int64) * (k * 4)
            return r if perm is None else r[perm]

        def alloc(n, k):
            mk = lambda: torch.empty((n, k), dtype=wdt, device=dev)
            return mk(), (mk() if prec.split else None), torch.empty((k, n), dtype=wdt, device=dev), (torch.empty((k, n), dtype=wdt, device=dev) if prec.split else None)

        FF = ffm.w_1.weight.shape[0]
        specs = [("ffm_w1", rows_of(ffm.w_1.weight, FF, D), FF, D), ("ffm_w2", rows_of(ffm.w_2.weight, D, FF), D, FF),
                 ("qkv", torch.cat([rows_of(att.linear_q.weight, D, D), rows_of(att.linear_k.weight, D, D), rows_of(att.linear_v.weight, D, D)]), 3 * D, D),
                 ("out", rows_of(att.linear_out.weight, D, D), D, D),
                 ("pw1", rows_of(cv.pointwise_conv1.weight, 2 * D, D, self.idx), 2 * D, D), ("pw2", rows_of(cv.pointwise_conv2.weight, D, D), D, D),
                 ("ff_w1", rows_of(ff.w_1.weight, FF, D), FF, D), ("ff_w2", rows_of(ff.w_2.weight, D, FF), D, FF)]
        self.keep, self.out, jobs, tile0 = [], {}, [], 0
        for name, rows, n, k in specs:
            if n % 8 or k % 8:
                raise ValueError("training packs: matrix dims must be multiples of 8")
            rows = rows.contiguous()
            w, wl, wt, wtl = alloc(n, k)
            self.keep.append(rows)
            self.out[name] = (w, wl, wt, wtl)
            jobs.append([rows.data_ptr(), n, k, w.data_ptr(), _c.ptr(wl) or 0, wt.data_ptr(), _c.ptr(wtl) or 0, tile0])
            tile0 += ((n + 63) // 64) * ((k + 63) // 64)
        self.tiles = tile0
        self.jobs = torch.tensor(jobs, dtype=torch.int64).to(dev)

    def packs(self, layer, qkv_b, pw1_b):
        """The block's (macaron FFN, attention, conv module, FFN) packs around the destinations of its matrix jobs; qkv_b / pw1_b: its two gathered
        bias vectors (_StackPackPlan packs both)."""
        o = self.out

        def ffn(mod, pre):
            (w1, w1l, w1t, w1tl), (w2, w2l, w2t, w2tl) = o[pre + "_w1"], o[pre + "_w2"]
            return Packed(w1=w1, w1_lo=w1l, b1=f32(mod.w_1.bias), w2=w2, w2_lo=w2l, b2=f32(mod.w_2.bias), w1t=w1t, w1t_lo=w1tl, w2t=w2t, w2t_lo=w2tl)
        (qkv, qkvl, qkvt, qkvtl), (out, outl, outt, outtl) = o["qkv"], o["out"]
        pa = Packed(qkv_w=qkv, qkv_w_lo=qkvl, qkv_t=qkvt, qkv_t_lo=qkvtl, qkv_b=qkv_b, out_w=out, out_w_lo=outl, out_t=outt, out_t_lo=outtl,
                    out_b=f32(layer.self_attn.linear_out.bias))
        pc = conv_module_train_pack(layer.conv_module, self.idx, pw1_b, o["pw1"], o["pw2"])
        return ffn(layer.feed_forward_macaron, "ffm"), pa, pc, ffn(layer.feed_forward, "ff")


class _StackPackPlan:
    """The training packs of ALL blocks of an encoder in two launches per optimizer step -- the blocks' matrix jobs in one table
    (cfm_pack_matrices), their two small gathered vectors (fused q|k|v bias + pos_bias_u, interleaved pointwise-conv-1 bias) through
    element-pointer tables (cfm_pack_vectors) -- instead of one matrix launch and ~4 torch operations per block (12 blocks: 60 launches).
    An absent pointwise-conv-1 bias is gathered from zeros."""

    def __init__(self, layers, prec, relative):
        self.plans = [_LayerPackPlan(l, prec) for l in layers]
        dev = self.plans[0].jobs.device
        tables, off = [], 0
        for pl in self.plans:
            j = pl.jobs.clone()
            j[:, 7] += off
            off += pl.tiles
            tables.append(j)
        self.jobs, self.tiles = torch.cat(tables, 0).contiguous(), off
        pa, pb, self.vec_slices, n = [], [], [], 0
        el = lambda t: t.data_ptr() + 4 * torch.arange(t.numel(), device=dev, dtype=torch.int64)
        self.zero_bias = torch.zeros(2 * max(l.encoder_dim for l in layers), device=dev)     # what an absent pointwise-conv-1 bias reads
        for l, pl in zip(layers, self.plans):
            att, cv = l.self_attn, l.conv_module
            D = cv.pointwise_conv2.weight.shape[0]
            b1 = cv.pointwise_conv1.bias if cv.pointwise_conv1.bias is not None else self.zero_bias[:2 * D]
            for t in (att.linear_q.bias, att.linear_k.bias, att.linear_v.bias, b1) + ((att.pos_bias_u,) if relative else ()):
                if t is None or t.dtype != torch.float32 or not t.is_contiguous():
                    raise TypeError("the stack pack needs contiguous float32 bias parameters")
            zeros = torch.zeros(D, device=dev, dtype=torch.int64)
            pa += [el(att.linear_q.bias), el(att.linear_k.bias), el(att.linear_v.bias), el(b1)[pl.idx]]
            pb += [el(att.pos_bias_u) if relative else zeros, zeros, zeros, zeros, zeros]
            self.vec_slices.append((n, n + 3 * D, n + 5 * D))
            n += 5 * D
        self.pa, self.pb = torch.cat(pa).contiguous(), torch.cat(pb).contiguous()
        self.vec = torch.empty(n, dtype=torch.float32, device=dev)
        self.prec, self.layers, self.val = prec, list(layers), None
        self.ptrs = tuple(t.data_ptr() for l in layers for t in l.parameters())

    def valid_for(self, layers, prec):
        return (prec.name == self.prec.name and len(layers) == len(self.layers) and all(a is b for a, b in zip(layers, self.layers)) and
                tuple(t.data_ptr() for l in layers for t in l.parameters()) == self.ptrs)

    def run(self):
        prec = self.prec
        _c.call("cfm_pack_matrices", self.jobs.data_ptr(), self.jobs.shape[0], self.tiles, _c.BF16 if prec.split else prec.w_code, 1 if prec.split else 0)
        _c.call("cfm_pack_vectors", self.pa.data_ptr(), self.pb.data_ptr(), self.vec.data_ptr(), self.vec.numel())
        if self.val is None:        # the destinations never move (valid_for checks the sources' addresses): the same Packed objects every step, so
            # whoever caches on their identity (the stack's ctypes weight structs, cfm/autograd.py) keeps its cache across optimizer steps
            self.val = tuple(pl.packs(l, self.vec[a:b], self.vec[b:c]) for l, pl, (a, b, c) in zip(self.layers, self.plans, self.vec_slices))
        return self.val


def pack_stack_train(owner, layers, prec, relative, flat=False):
    """((macaron FFN, attention, conv module, FFN) training packs) per block for the whole stack, two launches when anything changed.
    flat: every parameter lives in the data-parallel trainer's flat buffer and changes only through its step (which bumps the pack epoch) --
    the per-tensor version walk (~300 tensors) is skipped: the key is the epoch, and the plan's valid_for (blocks and addresses) stands in
    for the rest.  The slot holds (plan, packs); the plan outlives a key miss while it is valid_for, and so do its Packed objects."""
    s = slot(owner, "_pack_stack_train")
    if flat:
        key = (_EPOCH[0], "flat", prec.name)                 # weights_key of no tensors, spelled out: this is the per-step path
        if key == s.key:
            plan, val = s.value
            if plan.valid_for(layers, prec):
                return val
            s.clear()                                        # same epoch, other blocks or addresses: neither plan nor packs survive
    else:
        key = weights_key([p for l in layers for n, p in l.named_parameters() if not n.startswith("norm_")], "walk", prec.name)
    plan = s.value[0] if s.value is not None else None

    def build():
        p = plan if plan is not None and plan.valid_for(layers, prec) else _StackPackPlan(layers, prec, relative)
        return p, p.run()
    return s.get(key, build)[1]


def pack_subsampling_train(mod, prec):
    c1, c2, lin = mod.conv[0], mod.conv[2], mod.out[0]

    def build():
        C = c1.weight.shape[0]
        w2f = c2.weight.detach().permute(0, 2, 3, 1).reshape(C, 9 * C)                      # [co][kt][kf][ci]
        Dout, CF = lin.weight.shape
        Fp = CF // C
        wlf = lin.weight.detach().reshape(Dout, C, Fp).permute(0, 2, 1).reshape(Dout, Fp * C)   # feature order f*C + c
        w2, w2l = matrix(w2f, prec)
        w2t, w2tl = matrix_t(w2f, prec)
        wl, wll = matrix(wlf, prec)
        wlt, wltl = matrix_t(wlf, prec)
        return Packed(w1=f32(c1.weight.detach().reshape(C, 9).t()), b1=f32(c1.bias), w2=w2, w2_lo=w2l, w2t=w2t, w2t_lo=w2tl, b2=f32(c2.bias),
                      wl=wl, wl_lo=wll, wlt=wlt, wlt_lo=wltl, bl=f32(lin.bias), C=C, Fp=Fp)
    return _train_slot(mod).get([c1.weight, c1.bias, c2.weight, c2.bias, lin.weight, lin.bias], prec, build)


def pack_ctc_train(mod, prec):
    def build():
        V, D = mod.ctc_lo.weight.shape
        Vp = (V + 7) // 8 * 8                          # cfm_gemm_tn wants N % 8 == 0; pad rows are zero and never read by the CTC kernels
        w = torch.zeros((Vp, D), dtype=torch.float32, device=mod.ctc_lo.weight.device)
        w[:V] = mod.ctc_lo.weight.detach()
        b = torch.zeros((Vp,), dtype=torch.float32, device=w.device)
        b[:V] = mod.ctc_lo.bias.detach()
        wm, wlo = matrix(w, prec)
        wt, wtlo = matrix_t(w, prec)
        return Packed(w=wm, w_lo=wlo, wt=wt, wt_lo=wtlo, b=b, V=V, Vp=Vp)
    return _train_slot(mod).get([mod.ctc_lo.weight, mod.ctc_lo.bias], prec, build)


def pack_src_attn_train(mod, prec):
    """Cross-attention in train mode: q from the decoder rows, k | v in one product over the memory rows; each matrix and its transpose."""
    srcs = [mod.linear_q.weight, mod.linear_q.bias, mod.linear_k.weight, mod.linear_k.bias, mod.linear_v.weight, mod.linear_v.bias,
            mod.linear_out.weight, mod.linear_out.bias]

    def build():
        wkv = torch.cat([mod.linear_k.weight.detach(), mod.linear_v.weight.detach()], 0)
        q, ql = matrix(mod.linear_q.weight, prec)
        qt, qtl = matrix_t(mod.linear_q.weight, prec)
        kv, kvl = matrix(wkv, prec)
        kvt, kvtl = matrix_t(wkv, prec)
        out, outl = matrix(mod.linear_out.weight, prec)
        outt, outtl = matrix_t(mod.linear_out.weight, prec)
        return Packed(q_w=q, q_w_lo=ql, q_t=qt, q_t_lo=qtl, q_b=f32(mod.linear_q.bias), kv_w=kv, kv_w_lo=kvl, kv_t=kvt, kv_t_lo=kvtl,
                      kv_b=torch.cat([mod.linear_k.bias.detach().float(), mod.linear_v.bias.detach().float()], 0).contiguous(),
                      out_w=out, out_w_lo=outl, out_t=outt, out_t_lo=outtl, out_b=f32(mod.linear_out.bias))
    return slot(mod, "_pack_src_train", PackCache).get(srcs, prec, build)


def pack_vocab_train(linear, prec):
    """An output projection under the label-smoothing loss: the weight padded to Vk = a multiple of 8 rows (cfm_gemm wants K % 8 == 0 of the
    transposed pack, cfm_gemm_tn N % 8 == 0; the pad rows are zero and cfm_lsm_loss / cfm_lsm_grad never read them) and its transpose."""
    def build():
        V, D = linear.weight.shape
        Vk = (V + 7) // 8 * 8
        w = torch.zeros((Vk, D), dtype=torch.float32, device=linear.weight.device)
        w[:V] = linear.weight.detach()
        b = torch.zeros((Vk,), dtype=torch.float32, device=w.device)
        b[:V] = linear.bias.detach()
        wm, wlo = matrix(w, prec)
        wt, wtlo = matrix_t(w, prec)
        return Packed(w=wm, w_lo=wlo, wt=wt, wt_lo=wtlo, b=b, V=V, Vk=Vk)
    return _train_slot(linear).get([linear.weight, linear.bias], prec, build)


def pack_joint_train(mod, prec):
    """TransducerJoint.rnnt_loss: the three projections and their transposes; ffn_out padded to Vp = a multiple of 8 rows (cfm_gemm_tn wants
    N % 8 == 0; the pad rows are zero, so are the logits' pad columns, which the RNN-T kernels never read and whose gradient is exactly 0)."""
    def build():
        def lin(m, rows=None):
            w, b = m.weight.detach().float(), m.bias.detach().float()
            if rows is not None and rows != w.shape[0]:
                w = torch.cat([w, w.new_zeros((rows - w.shape[0], w.shape[1]))])
                b = torch.cat([b, b.new_zeros((rows - b.shape[0],))])
            wm, wlo = matrix(w.contiguous(), prec)
            wt, wtlo = matrix_t(w, prec)
            return Packed(w=wm, w_lo=wlo, b=b.contiguous(), wt=wt, wt_lo=wtlo)
        V = mod.ffn_out.weight.shape[0]
        Vp = (V + 7) // 8 * 8
        return Packed(enc=lin(mod.enc_ffn), pred=lin(mod.pred_ffn), out=lin(mod.ffn_out, Vp), V=V, Vp=Vp)
    params = [mod.enc_ffn.weight, mod.enc_ffn.bias, mod.pred_ffn.weight, mod.pred_ffn.bias, mod.ffn_out.weight, mod.ffn_out.bias]
    return _train_slot(mod).get(params, prec, build)


# ----------------------------------------------------------------------------------------------------------------------
# log-mel filter bank tables (csrc/fbank.hip): host float64, no module, no cache -- fbank.KaldiFbank builds them once
# ----------------------------------------------------------------------------------------------------------------------
def mel_banks_f64(num_mel_bins, padded, sample_frequency, low_freq=20.0):
    """torchaudio.compliance.kaldi.get_mel_banks (high_freq = Nyquist, no VTLN) in float64: (num_mel_bins, padded // 2); the Nyquist bin,
    whose weight is 0, is left out.  mel(f) = 1127 ln(1 + f / 700); triangle b has edges mel(low) + (b, b + 1, b + 2) delta."""
    import math
    lo = 1127.0 * math.log(1.0 + low_freq / 700.0)
    hi = 1127.0 * math.log(1.0 + 0.5 * sample_frequency / 700.0)
    delta = (hi - lo) / (num_mel_bins + 1)
    b = torch.arange(num_mel_bins, dtype=torch.float64).unsqueeze(1)
    left, center, right = lo + b * delta, lo + (b + 1.0) * delta, lo + (b + 2.0) * delta
    mel = (1127.0 * torch.log(1.0 + sample_frequency / padded * torch.arange(padded // 2, dtype=torch.float64) / 700.0)).unsqueeze(0)
    return torch.clamp(torch.min((mel - left) / (center - left), (right - mel) / (right - center)), min=0.0)


def pack_mel_banks(num_mel_bins, padded, sample_frequency, low_freq=20.0):
    """The banks rounded to f32, sparse: per mel bin its first FFT bin, its run length and the offset of its run in one contiguous weight
    vector -> (weights f32 [nnz], start, length, offset int32 [num_mel_bins]) on the host.  A triangle is one run of non-zero weights."""
    dense = mel_banks_f64(num_mel_bins, padded, sample_frequency, low_freq).to(torch.float32)
    weights, start, length, offset = [], [], [], []
    for row in dense:
        nz = torch.nonzero(row).flatten()
        if nz.numel() == 0:
            raise ValueError("pack_mel_banks: a mel bin covers no FFT bin (%d bins over %d FFT bins at %g Hz)" % (num_mel_bins, padded // 2, sample_frequency))
        k0, k1 = int(nz[0]), int(nz[-1]) + 1
        start.append(k0)
        length.append(k1 - k0)
        offset.append(sum(length[:-1]))
        weights.append(row[k0:k1])
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)      # noqa: E731
    return torch.cat(weights).contiguous(), i32(start), i32(length), i32(offset)


def unpack_mel_banks(weights, start, length, offset, n_fft_bins):
    """Dense (num_mel_bins, n_fft_bins) f32 view of pack_mel_banks' result (tests, documentation)."""
    dense = torch.zeros((start.numel(), n_fft_bins), dtype=torch.float32)
    for b, (k0, n, o) in enumerate(zip(start.tolist(), length.tolist(), offset.tolist())):
        dense[b, k0:k0 + n] = weights[o:o + n]
    return dense


def fbank_tables(win, padded):
    """(twiddle f64 [padded, 2] = (cos, -sin)(2 pi k / padded), povey window f64 [win] = hann(win, periodic=False) ** 0.85), host float64."""
    import math
    k = torch.arange(padded, dtype=torch.float64) * (2.0 * math.pi / padded)
    twiddle = torch.stack([torch.cos(k), -torch.sin(k)], dim=1).contiguous()
    window = torch.hann_window(win, periodic=False, dtype=torch.float64).pow(0.85)
    return twiddle, window


def host_packets(owner, B, sample_lens, final, columns, upto=None):
    """The (sample_lens, final) of one streaming audio step as lists of B ints / bools, or ValueError: host values only (a list or a CPU tensor of
    integers; the host mirrors the streams' bookkeeping from them), B of each, every count in 0 .. columns (no upper bound with columns None;
    `upto` then names the bound in the message).  sample_lens None: `columns` for every stream; final None: all False.  fbank.PacketSchedule and
    resample.StreamingResampler share it."""
    vals = []
    for name, v, default in (("sample_lens", sample_lens, columns), ("final", final, False)):
        if v is None:
            v = [default] * B
        if isinstance(v, torch.Tensor):
            if v.device.type != "cpu":
                raise ValueError("%s: %s are host values (a list or a CPU tensor), the host mirrors the streams' bookkeeping; got a tensor on %s" % (owner, name, v.device))
            if v.dim() != 1 or v.dtype.is_floating_point or v.dtype.is_complex:
                raise ValueError("%s: %s must hold %d integers, got %s %s" % (owner, name, B, v.dtype, tuple(v.shape)))
            v = v.tolist()
        v = list(v)
        if len(v) != B:
            raise ValueError("%s: %d %s for %d streams" % (owner, len(v), name, B))
        vals.append(v)
    lens, final = vals
    for b, n in enumerate(lens):
        if n is None or int(n) != n or n < 0 or (columns is not None and n > columns):
            raise ValueError("%s: sample_lens[%d] = %r: a count of new samples, 0 .. %s" % (owner, b, n, upto or "the block's %d columns" % columns))
    return [int(n) for n in lens], [bool(f) for f in final]


def stream_lens(owner, name, B, value, bound, buf, default=None, strict=False):
    """One per-stream count of a streaming step (frames of a window, frames of a chunk, a final flag) read into the persistent device buffer
    `buf` ([B], any integer dtype) that the step reads; buf None: checked only, nothing written.  Returns the B counts as a list of ints when
    the host knows them, None when `value` is a device tensor (it stays on the device: no synchronisation).
      * value None: `default` (`bound` when None) for every stream.
      * host values (a list / iterable or a CPU tensor) and a device tensor alike: another count than B -> ValueError.
      * strict=False (the decoders): a host value is truncated to an int and clamped to 0 .. bound; a tensor may have any shape of B elements.
      * strict=True (StreamingBatch: the host mirrors the streams' offsets from these): a host value that is not a whole number in 0 .. bound
        -> ValueError; a tensor is 1-d int32 / int64, else ValueError.
      * a device tensor is never read on the host: its values are clamped to 0 .. bound on the device, in either mode."""
    if value is None:
        fill = bound if default is None else default
        if buf is not None:
            buf.fill_(fill)
        return [fill] * B
    if isinstance(value, torch.Tensor):
        if value.numel() != B or (strict and (value.dim() != 1 or value.dtype not in (torch.int32, torch.int64))):
            raise ValueError("%s: %s must hold %d integers, got %s %s" % (owner, name, B, value.dtype, tuple(value.shape)))
        if value.device.type != "cpu":
            if buf is not None:
                buf.copy_((value if value.dtype in (torch.int32, torch.int64) else value.to(torch.int64)).reshape(B).clamp(0, bound))
            return None
        host = value.reshape(B).tolist()
    else:
        host = list(value)
    if len(host) != B:
        raise ValueError("%s: %d %s for %d streams" % (owner, len(host), name, B))
    if strict:
        for b, n in enumerate(host):
            if int(n) != n or not 0 <= n <= bound:
                raise ValueError("%s: %s[%d] = %r, outside 0 .. %d" % (owner, name, b, n, bound))
    host = [min(max(int(n), 0), bound) for n in host]
    if buf is not None:
        buf.copy_(torch.tensor(host, dtype=buf.dtype))
    return host


def stream_index(streams, dev):
    """What a reset indexes per-stream state with: every stream (streams None) or the given ones, as a long tensor on dev."""
    return slice(None) if streams is None else torch.as_tensor(list(streams), dtype=torch.long, device=dev)


# ----------------------------------------------------------------------------------------------------------------------
# sample-rate conversion tables (csrc/resample.hip): host float64, no module, no cache -- resample.Resampler builds them once
# ----------------------------------------------------------------------------------------------------------------------
RESAMPLE_MAX_PHASES = 1024               # reduced new rate n: one int32 first-tap and one offset per phase in LDS
RESAMPLE_MAX_TABLE_BYTES = 64 * 1024     # the compact f32 tap table, whole in LDS
RESAMPLE_LIVE = 2.0 ** -60               # |h| below this is a clamped end of the window (cos^2 ~ 4e-33): dropped


def resample_geometry(orig_freq, new_freq):
    """(o, n, base, width): the rates over their gcd, the cutoff min(o, n) * 0.99 and ceil(6 o / base) taps on either side."""
    import math
    if int(orig_freq) != orig_freq or int(new_freq) != new_freq or orig_freq < 1 or new_freq < 1:
        raise ValueError("resample: whole sample rates >= 1 Hz, got %r -> %r" % (orig_freq, new_freq))
    g = math.gcd(int(orig_freq), int(new_freq))
    o, n = int(orig_freq) // g, int(new_freq) // g
    base = min(o, n) * 0.99
    return o, n, base, int(math.ceil(6 * o / base))


def resample_kernel_f64(orig_freq, new_freq):
    """torchaudio's _get_sinc_resample_kernel (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99) in float64: h [n, 2 width + o],
    h[j][k] = sinc(t) cos^2(pi t / 12) base / o at t = clamp((-j / n + (k - width) / o) base, -6, 6)."""
    import math
    o, n, base, width = resample_geometry(orig_freq, new_freq)
    i = torch.arange(-width, width + o, dtype=torch.float64).unsqueeze(0) / o
    j = torch.arange(0, -n, -1, dtype=torch.float64).unsqueeze(1) / n
    t = ((j + i) * base).clamp_(-6.0, 6.0)
    window = torch.cos(t * (math.pi / 12.0)) ** 2
    t = t * math.pi
    return torch.where(t == 0, torch.ones_like(t), torch.sin(t) / torch.where(t == 0, torch.ones_like(t), t)) * window * (base / o)


def resample_tables(orig_freq, new_freq):
    """The polyphase bank, compact: per phase its one run of live taps (|h| >= 2^-60) rounded to f32, end to end in one vector ->
    (taps f32 [total], first int32 [n]: the run's first tap k = i + width, offset int32 [n + 1]: where it starts in `taps`) on the host.
    ValueError beyond RESAMPLE_MAX_PHASES phases or RESAMPLE_MAX_TABLE_BYTES of taps: the kernel keeps the whole bank in LDS."""
    o, n, _, width = resample_geometry(orig_freq, new_freq)
    if n > RESAMPLE_MAX_PHASES:
        raise ValueError("resample_tables: %d -> %d Hz has %d phases (the new rate over the gcd); the kernel takes at most RESAMPLE_MAX_PHASES = %d"
                         % (orig_freq, new_freq, n, RESAMPLE_MAX_PHASES))
    if n * 4 > RESAMPLE_MAX_TABLE_BYTES or (2 * width + o) * 4 > 16 * RESAMPLE_MAX_TABLE_BYTES:    # before the dense bank is even built
        raise ValueError("resample_tables: %d -> %d Hz needs %d taps per phase; the compact table may hold RESAMPLE_MAX_TABLE_BYTES = %d bytes"
                         % (orig_freq, new_freq, 2 * width + o, RESAMPLE_MAX_TABLE_BYTES))
    h = resample_kernel_f64(orig_freq, new_freq)
    taps, first, offset = [], [], [0]
    for j in range(n):
        live = torch.nonzero(h[j].abs() >= RESAMPLE_LIVE).flatten()
        k0, k1 = int(live[0]), int(live[-1]) + 1
        if k1 - k0 != live.numel():
            raise ValueError("resample_tables: phase %d of %d -> %d Hz has a gap in its live taps" % (j, orig_freq, new_freq))
        first.append(k0)
        offset.append(offset[-1] + k1 - k0)
        taps.append(h[j, k0:k1].to(torch.float32))
    if offset[-1] * 4 > RESAMPLE_MAX_TABLE_BYTES:
        raise ValueError("resample_tables: %d -> %d Hz needs %d live taps, %d bytes; the compact table may hold RESAMPLE_MAX_TABLE_BYTES = %d bytes (and at most "
                         "RESAMPLE_MAX_PHASES = %d phases)" % (orig_freq, new_freq, offset[-1], offset[-1] * 4, RESAMPLE_MAX_TABLE_BYTES, RESAMPLE_MAX_PHASES))
    return torch.cat(taps).contiguous(), torch.tensor(first, dtype=torch.int32), torch.tensor(offset, dtype=torch.int32)


RESAMPLE_MAX_BANKS = 8                   # cfm_resample_group: rate pairs in one launch (CFM_RESAMPLE_MAX_BANKS)


def speed_rates(speed, sample_rate=16000):
    """The rate pair torchaudio.functional.speed resamples between for this factor: (int(speed * sample_rate), sample_rate)."""
    if not speed > 0:
        raise ValueError("speed perturbation: a factor > 0, got %r" % (speed,))
    return int(speed * int(sample_rate)), int(sample_rate)


def resample_group_tables(pairs, tile_blocks):
    """The banks of cfm_resample_group for the rate pairs [(orig, new), ...]: resample_tables of each pair that converts, end to end ->
    ((taps f32, first int32, offset int32) on the host, or None when no pair converts,
     one row (o, n, width, n_live, taps_at, first_at, off_at, tile_blocks) per pair).  A pair with equal rates is the identity bank (o = n = 1, no table).
    tile_blocks(o, n, width) is cfm_resample_tile_blocks; ValueError when it returns 0 (the bank and a tile's input span exceed the kernel's LDS), beyond
    RESAMPLE_MAX_BANKS pairs, and whatever resample_tables raises."""
    pairs = list(pairs)
    if not 1 <= len(pairs) <= RESAMPLE_MAX_BANKS:
        raise ValueError("resample_group_tables: %d rate pairs; one launch takes 1 .. RESAMPLE_MAX_BANKS = %d" % (len(pairs), RESAMPLE_MAX_BANKS))
    taps, first, offset, rows = [], [], [], []
    n_taps = n_first = n_off = 0
    for orig, new in pairs:
        o, n, _, width = resample_geometry(orig, new)
        if o == n:
            rows.append((o, n, width, 0, 0, 0, 0, 0))
            continue
        t, f, off = resample_tables(orig, new)
        tb = int(tile_blocks(o, n, width))
        if tb <= 0:
            raise ValueError("resample_group_tables: %d -> %d Hz reads %d samples per output block of %d with %d taps on either side: the bank "
                             "(RESAMPLE_MAX_TABLE_BYTES = %d) and one tile's input span do not fit the kernel's LDS" % (orig, new, o, n, width, RESAMPLE_MAX_TABLE_BYTES))
        rows.append((o, n, width, t.numel(), n_taps, n_first, n_off, tb))
        taps.append(t)
        first.append(f)
        offset.append(off)
        n_taps, n_first, n_off = n_taps + t.numel(), n_first + f.numel(), n_off + off.numel()
    if not taps:
        return None, rows
    return (torch.cat(taps).contiguous(), torch.cat(first).contiguous(), torch.cat(offset).contiguous()), rows


def unpack_resample_tables(taps, first, offset, n_taps):
    """Dense (n, n_taps) f32 view of resample_tables' result (tests, documentation)."""
    dense = torch.zeros((first.numel(), n_taps), dtype=torch.float32)
    for j, k0 in enumerate(first.tolist()):
        a, b = int(offset[j]), int(offset[j + 1])
        dense[j, k0:k0 + b - a] = taps[a:b]
    return dense
