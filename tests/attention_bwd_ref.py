"""cfm_attention_bwd restated from include/cfm.h (cfm_attn_bwd_desc) and the formulas at the top of csrc/attention_bwd.hip, not from the kernels:

    P = exp(scale s - lse), s = q'_i . k_j;  P = 0 where the pair is masked or lse = -inf          delta_i = dO_i . O_i, from the `out` that is GIVEN
    dS = P (keep / (1 - p) dP - delta) scale,  dP = dO V^T        dQ = dS K      dK = dS^T Q'      dV = (keep / (1 - p) P)^T dO

on CPU tensors, every operand addressed by the element strides the descriptor carries (attention_ref.fetch / gather, whose helpers this module
uses and does not copy).  `evaluate(P, g)` is the float64 evaluation, `evaluate(P, g, F32)` the SAME formulas in plain float32 torch with the
roundings the design adds -- the yardstick of measure_g -- and `evaluate(P, g, variant=...)` a restatement that is wrong in one named way (VARIANTS),
for the discrimination audit of tests/test_attention_bwd_ref_cpu.py.

Operands, as the kernels declare them: q', K, V and dO enter the products rounded to the MFMA type when split is off (row_frags / stage_tile:
pack_planes), unrounded in split mode (the header's "f32-accurate"); delta is the float32 dot product of the rows as they lie in memory.  `out`
and `lse` are INPUTS of the backward: given(P, keep) takes them from the float64 forward on the same operands (attention_ref.evaluate, the
dropout keep mask applied to the probabilities), rounded to the io type and to float32 -- never from cfm_attention, so the backward is isolated;
the chained cases of the GPU module pass the kernel's own out and lse instead.  The keep mask is an input too: the CPU Bernoulli mask of
problem() for the yardstick, cfm.dropout_mask on the GPU.

Bound, per element, never a norm.  With W_ij = P_ij (R_ij + E_i), R_ij = keep/(1-p) sum_e |dO_ie||v_je|, E_i = sum_e |dO_ie||O_ie|:
    |dq - ref| <= g_q S^q + ulp_io(ref),  S^q_id = scale sum_j W_ij |k_jd|
    |dk - ref| <= g_k S^k + ulp_io(ref),  S^k_jd = scale sum_i W_ij |q'_id|
    |dv - ref| <= g_v S^v + ulp_io(ref),  S^v_jd = sum_i keep/(1-p) P_ij |dO_id|
Where S = 0 the value must be exactly 0 (dq of a fully masked row; dk and dv of a key no query sees); no NaN anywhere.  The g are 4 x the worst
ratio of the float32 yardstick per class (bf16, fp16, split) and gradient over yardstick_cases() -- the cases of
tests/test_attention_bwd_matrix_gpu.py -- and never come from a kernel's output.  The yardstick's roundings: operands to the MFMA type; the
dropout-scaled P and dS rounded to the MFMA type before the second products (pack8 / pack_planes); float32 accumulation; outputs rounded to the
io type; split mode: the header's three products hi.hi + lo.hi + hi.lo on bf16 planes, for all five products.
"""
import functools
import math
from collections import namedtuple
from types import SimpleNamespace

import torch

import attention_ref as A
from attention_ref import BF16, F32, F64, MMA, Op, fetch, fetch_mask, flat, gather, product, rnd      # product: the split form on attention_ref.hilo planes
from gemm_ref import ulp

QT = KT = 64                     # queries / keys per tile of every backward kernel (csrc/attn_common.h)
GROUP_MAX = 8                    # ATTN_GROUP_MAX
DEAD = 3.0e4                     # what K and V rows hold that are masked for every query: finite (NaN there is outside the contract, as in the forward)

# shape (B, H, Tq, Tk); mask none | pad, lens (B,1,Tk), m_sq = 0 | full (B,Tq,Tk), m_sq = Tk + 3; layout fused ([B, T, 3D + ld_pad] q|k|v) | cross (q [B,Tq,D + ld_pad],
# k|v [B,Tk,2D + ld_pad]); f32: the rows are float32 (always in split mode); do32: dout float32 (do16: dout 16 bit beside float32 rows); sb_pad: rows
# between two items of a buffer, so the batch stride is not T st; qk_scale multiplies q and k (peaked rows); drop: the dropout probability;
# dead: what dead K / V rows hold (None: the ordinary random numbers)
Case = namedtuple("Case", "shape dk mma split mask layout f32 do32 do16 ld_pad sb_pad qk_scale drop dead seed",
                  defaults=(64, "bf16", False, "none", "fused", False, False, False, 0, 0, 1.0, 0.0, DEAD, 0))


# ---------------------------------------------------------------------------------------------------------------- masks
def pad_mask(B, Tk, seed):
    """attention_ref.pad_mask (item 0 about 70 % live, item 1 one live key) and, at Tk > 64 with B > 2, a last item whose first 64-key tile is wholly dead."""
    m = A.pad_mask(B, Tk, seed)
    if Tk > KT and B > 2:
        g = torch.Generator().manual_seed(seed + 1)
        m[B - 1] = (torch.rand(Tk, generator=g) < 0.7).to(torch.uint8)
        m[B - 1, :KT] = 0
        m[B - 1, Tk - 1] = 1
    return m


def lens_mask(B, T):
    """the right-padded key-validity mask of tests/test_train_ops_gpu.py::test_attention_backward."""
    lens = ([T, max(1, T - T // 4), max(1, T // 2)][:B] + [T] * max(0, B - 3))
    return (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).to(torch.uint8)


def full_mask(B, Tq, Tk, seed):
    """(B, Tq, Tk), 60 % dense.  At Tk > 64 the even rows of the last item have no live key in the first tile (and a live last key); key min(2, Tk - 1)
    of the last item is masked for every query (not at Tk = 1); row min(3, Tq - 1) of item 0 is fully masked (not at Tq = 1); no other dead row."""
    g = torch.Generator().manual_seed(seed)
    m = (torch.rand((B, Tq, Tk), generator=g) < 0.6).to(torch.uint8)
    if Tk > KT:
        m[B - 1, 0::2, :KT] = 0
        m[B - 1, 0::2, Tk - 1] = 1
    if Tk > 1:
        m[B - 1, :, min(2, Tk - 1)] = 0
    m[:, :, Tk - 1 if Tk > 3 else 0] |= (m.sum(-1) == 0).to(torch.uint8)            # no accidental dead row
    if Tq > 1:
        m[0, min(3, Tq - 1)] = 0
    return m


# ---------------------------------------------------------------------------------------------------------------- problems
@functools.lru_cache(maxsize=None)
def problem(key):
    """One descriptor on CPU tensors, made once and never written to (attention_ref.problem's conventions: bufs name -> (tensor, row stride), ops
    name -> Op).  dout [B,Tq,D] and keep (a CPU Bernoulli mask, None without dropout) beside them."""
    B, H, Tq, Tk = key.shape
    dk, D = key.dk, H * key.dk
    mma = MMA[key.mma]
    f32 = key.f32 or key.split
    io = F32 if f32 else mma
    s = 1000 * key.seed + 131 * B + 17 * Tq + Tk + 7 * H + dk + 50000
    P = SimpleNamespace(key=key, B=B, H=H, Tq=Tq, Tk=Tk, dk=dk, D=D, mma=mma, split=key.split, scale=float(dk) ** -0.5, bufs={}, ops={}, p_str=(0, 0), mask_str=(0, 0),
                        u=None, vb=None, io=io, q_dtype=io, kv_dtype=io, out_dtype=io, do_dtype=F32 if (key.do32 or (f32 and not key.do16)) else mma, drop=key.drop, keep=None)
    q, k, v = rnd((B, Tq, D), s + 1, key.qk_scale), rnd((B, Tk, D), s + 2, key.qk_scale), rnd((B, Tk, D), s + 3)
    if key.mask in ("pad", "lens"):
        m = pad_mask(B, Tk, s + 7) if key.mask == "pad" else lens_mask(B, Tk)
        P.bufs["mask"], P.mask_str = (m, Tk), (Tk, 0)
        dead = m == 0
    elif key.mask == "full":
        m_sq = Tk + 3                                           # a padded row stride: reading rows Tk apart is a different mask
        m = full_mask(B, Tq, Tk, s + 7)
        P.bufs["mask"], P.mask_str = (m, m_sq), (Tq * m_sq, m_sq)
        dead = m.sum(1) == 0
    else:
        dead = torch.zeros((B, Tk), dtype=torch.bool)
    P.dead = dead                                               # [B, Tk]: keys masked for every query
    if key.dead is not None:
        k[dead], v[dead] = key.dead, key.dead
    nan = float("nan")
    if key.layout == "fused":
        Tm, ld = max(Tq, Tk) + key.sb_pad, 3 * D + key.ld_pad
        buf = torch.full((B, Tm, 3 * D), nan)                  # rows past Tq / Tk and the rows between two items are no part of any operand
        buf[:, :Tq, :D], buf[:, :Tk, D:2 * D], buf[:, :Tk, 2 * D:] = q, k, v
        P.bufs["qkv"] = (buf.to(io), ld)
        P.ops["q"], P.ops["k"], P.ops["v"] = Op("qkv", 0, Tm * ld, ld, dk), Op("qkv", D, Tm * ld, ld, dk), Op("qkv", 2 * D, Tm * ld, ld, dk)
    else:
        qb, kvb = torch.full((B, Tq + key.sb_pad, D), nan), torch.full((B, Tk + key.sb_pad, 2 * D), nan)
        qb[:, :Tq], kvb[:, :Tk, :D], kvb[:, :Tk, D:] = q, k, v
        lq, lkv = D + key.ld_pad, 2 * D + key.ld_pad
        P.bufs["q"], P.bufs["kv"] = (qb.to(io), lq), (kvb.to(io), lkv)
        P.ops["q"] = Op("q", 0, (Tq + key.sb_pad) * lq, lq, dk)
        P.ops["k"], P.ops["v"] = Op("kv", 0, (Tk + key.sb_pad) * lkv, lkv, dk), Op("kv", D, (Tk + key.sb_pad) * lkv, lkv, dk)
    P.dout = rnd((B, Tq, D), s + 8).to(P.do_dtype)
    if key.drop:
        P.keep = torch.rand((B, H, Tq, Tk), generator=torch.Generator().manual_seed(s + 9)) >= key.drop
    return P


def owned(P, name):
    """bool over the flat buffer that holds operand `name`: the elements its gradient owns."""
    t, ld = P.bufs[P.ops[name].buf]
    own = torch.zeros(t.numel() // t.shape[-1] * ld, dtype=torch.bool)
    op, a = P.ops[name], torch.arange
    T = P.Tq if name == "q" else P.Tk
    own[(op.off + a(P.B)[:, None, None, None] * op.sb + a(P.H)[None, :, None, None] * op.sh + a(T)[None, None, :, None] * op.st + a(P.dk)).reshape(-1)] = True
    return own


# ---------------------------------------------------------------------------------------------------------------- which kernels
def tag(P):
    return "bf16x3" if P.split else ("bf16" if P.mma == BF16 else "f16")


def predicted_kernel(P):
    """A mirror of csrc/attention_bwd.hip: bwd_fast_ok (d_k, the dtypes, the % 8 strides, the 16-byte alignment of q / k / v -- element offsets in buffers
    that are 256-byte aligned; dout and out are dense allocations) and launch_bwd's MFULL choice.  -> namespace(fast, mfull, names (delta, dq, dkv))."""
    q, k, v = P.ops["q"], P.ops["k"], P.ops["v"]
    esz = 4 if P.io == F32 else 2
    al16 = all(o.off * esz % 16 == 0 for o in (q, k, v))
    fast = not P.split and P.dk == 64 and P.io == P.mma and P.do_dtype == P.mma and all(x % 8 == 0 for o in (q, k, v) for x in (o.sb, o.st)) and al16
    mfull = "mask" in P.bufs and P.mask_str[1] != 0
    f = "fast_" if fast else ""
    return SimpleNamespace(fast=fast, mfull=mfull, names=("attn_bwd_delta_fast" if fast else "attn_bwd_delta", "attn_bwd_dq_" + f + tag(P), "attn_bwd_dkv_" + f + tag(P)))


def predicted_group(Ps):
    """cfm_attention_bwd_group's groupable predicate: 2 .. 8 problems, none split, one MFMA type, one mask kind ((B,Tq,Tk) or not), every one fast.
    -> namespace(groupable, names: the profile names of the whole call)."""
    ks = [predicted_kernel(P) for P in Ps]
    ok = 2 <= len(Ps) <= GROUP_MAX and all(k.fast and k.mfull == ks[0].mfull and P.mma == Ps[0].mma for k, P in zip(ks, Ps))
    if ok:
        return SimpleNamespace(groupable=True, mfull=ks[0].mfull, names={"attn_bwd_delta_group", "attn_bwd_dq_group_" + tag(Ps[0]), "attn_bwd_dkv_group_" + tag(Ps[0])})
    return SimpleNamespace(groupable=False, mfull=None, names={n for k in ks for n in k.names})


# ---------------------------------------------------------------------------------------------------------------- the operation
def heads(x, P):
    """[B, Tq, H dk] -> [B, H, Tq, dk]"""
    return x.reshape(P.B, -1, P.H, P.dk).permute(0, 2, 1, 3)


def rows(x, P):
    """[B, H, T, dk] -> [B, T, H dk]"""
    return x.permute(0, 2, 1, 3).reshape(P.B, -1, P.D)


def keep_scale(P, keep, dt):
    """keep / (1 - p) as [B,H,Tq,Tk] (a scalar 1 without dropout)."""
    return torch.ones((), dtype=dt) if keep is None else keep.to(dt) / (1.0 - P.drop)


def forward(P, keep=None):
    """the float64 forward on the declared operands -> (out [B,Tq,D], lse [B,H,Tq]), unrounded: out = (keep / (1 - p) a) V, a and lse from attention_ref.evaluate."""
    f = A.evaluate(P)
    V = fetch(P, "v", P.Tk)
    Vr = V.double() if P.split else V.float().to(P.mma).double()
    return rows((f.a * keep_scale(P, keep, F64)) @ Vr, P), f.lse


def given(P, keep=None):
    """what the backward is handed: out rounded to the io type, lse to float32; dout and the keep mask beside them."""
    out, lse = forward(P, keep)
    return SimpleNamespace(out=out.to(P.io), lse=lse.float(), keep=keep)


def matmul(a, b, dt, split):
    """a [.., M, K] @ b [.., K, N] through attention_ref.product (float32 split: the three products)."""
    return product(a, b.transpose(-1, -2), dt, split)


def evaluate(P, g, dt=F64, variant=None):
    """-> namespace(dq [B,Tq,D], dk, dv [B,Tk,D] in dt (float32: rounded to the io type), delta [B,H,Tq]; float64 and no variant: Sq, Sk, Sv, the scales of the bounds)."""
    B, H, Tq, Tk, dk = P.B, P.H, P.Tq, P.Tk, P.dk
    kop = P.ops["k"]
    if variant == "k_sb_is_Tk_st":
        kop = kop._replace(sb=Tk * kop.st)
    Q, K, V = fetch(P, "q", Tq), fetch(P, "k", Tk, kop), fetch(P, "v", Tk)
    dO = heads(P.dout, P)
    if variant == "dout_of_head_0":
        dO = dO[:, :1].expand(B, H, Tq, dk)
    r = (lambda x: x.float()) if P.split else (lambda x: x.float().to(P.mma).float())
    Qr, Kr, Vr, dOr = r(Q), r(K), r(V), r(dO)
    live = torch.ones((B, 1, Tk), dtype=torch.bool)
    if "mask" in P.bufs:
        m_sb, m_sq = P.mask_str
        if variant == "m_sq_ignored":
            m_sq = 0
        if variant == "mask_transposed" and m_sq:
            a = torch.arange
            live = gather(flat(*P.bufs["mask"]), a(B)[:, None, None] * m_sb + a(Tk)[None, None, :] * m_sq + a(Tq)[None, :, None]) != 0
        else:
            live = fetch_mask(P, m_sb, m_sq)
    if variant == "last_key_of_tile_dropped":
        live = live & ~(torch.arange(Tk) % KT == KT - 1)
    live = live[:, None]                                        # [B, 1, Tq | 1, Tk]
    lse = g.lse.to(dt)
    if variant == "lse_plus_0.02":
        lse = lse + 0.02
    ninf = -math.inf
    dead_row = (lse == ninf)[..., None]
    keep = g.keep
    if variant == "drop_index_Tq" and keep is not None:      # element (b, h, i, j) taken at rid Tq + j where it lies at rid Tk + j
        rid = torch.arange(B * H * Tq).view(B, H, Tq, 1)
        keep = gather(keep.reshape(-1).to(torch.uint8), rid * Tq + torch.arange(Tk)) != 0
    ks = keep_scale(P, keep, dt)
    # ---- the probabilities and dS
    scale = P.scale if dt == F64 else torch.tensor(P.scale, dtype=dt)
    s = matmul(Qr, Kr.transpose(-1, -2), dt, P.split)
    ok = live & ~dead_row
    Pm = torch.where(ok, torch.exp(scale * s - torch.where(dead_row, torch.zeros_like(lse[..., None]), lse[..., None])), torch.zeros((), dtype=dt))
    if variant == "masked_keys_leak":
        Pm = torch.where(live | dead_row, Pm, torch.full_like(Pm, 1e-4))
    if variant == "masked_rows_uniform":
        Pm = torch.where(dead_row, torch.full_like(Pm, 1.0 / Tk), Pm)
    dP = matmul(dOr, Vr.transpose(-1, -2), dt, P.split)
    O = heads(g.out, P)
    delta = (dO.float() * O.float()).sum(-1) if dt == F32 else (dO.double() * O.double()).sum(-1)
    if variant == "delta_omitted":
        delta = torch.zeros_like(delta)
    Pd = ks * Pm
    dS = Pm * ((dP if variant == "dP_not_dropped" else ks * dP) - delta[..., None])
    if variant != "scale_missing":
        dS = dS * scale
    dSk, Pdk = dS, Pd
    if variant == "last_query_of_tile_dropped":                # from dK and dV only
        gone = (torch.arange(Tq) % QT == QT - 1)[:, None]
        dSk, Pdk = torch.where(gone, torch.zeros_like(dS), dS), torch.where(gone, torch.zeros_like(Pd), Pd)
    if dt == F32 and not P.split:                              # pack8 / pack_planes: the second products take P and dS in the MFMA type
        dS, dSk, Pdk = (x.to(P.mma).float() for x in (dS, dSk, Pdk))
    dq = matmul(dS, Kr, dt, P.split)
    dkk = matmul(dSk.transpose(-1, -2), Qr, dt, P.split)
    dv = matmul(Pdk.transpose(-1, -2), dOr, dt, P.split)
    res = SimpleNamespace(dq=rows(dq, P), dk=rows(dkk, P), dv=rows(dv, P), delta=delta, P=Pm)
    if dt == F32:
        res.dq, res.dk, res.dv = (x.to(P.io) for x in (res.dq, res.dk, res.dv))
    if dt == F64 and variant is None:
        aK, aQ, aV, aO = Kr.double().abs(), Qr.double().abs(), Vr.double().abs(), dOr.double().abs()
        W = Pm * (ks * (aO @ aV.transpose(-1, -2)) + (aO * O.double().abs()).sum(-1)[..., None])
        res.Sq, res.Sk, res.Sv = rows(P.scale * (W @ aK), P), rows(P.scale * (W.transpose(-1, -2) @ aQ), P), rows(Pd.transpose(-1, -2) @ aO, P)
    return res


@functools.lru_cache(maxsize=None)
def reference(key):
    """the float64 gradients of a case with the CPU keep mask of problem() (the GPU module evaluates cases with dropout on the device's mask instead)."""
    P = problem(key)
    return evaluate(P, given(P, P.keep))


# ---------------------------------------------------------------------------------------------------------------- the bound
GRADS = ("dq", "dk", "dv")


def ratio(x, ref, S, dtype):
    """worst (|x - ref| - ulp_io(ref)) / S; inf where a NaN appears or where S = 0 and the value is not exactly 0."""
    x = x.double()
    d = (x - ref).abs()
    r = (d - ulp(ref, dtype)).clamp_min(0) / S
    r = torch.where(S == 0, torch.where(x == 0, torch.zeros_like(d), torch.full_like(d, math.inf)), r)
    r = torch.where(torch.isnan(x), torch.full_like(d, math.inf), r)
    return float(r.max())


def ratios(res, ref, dtype):
    """-> (dq, dk, dv) ratios of a result (anything with .dq .dk .dv) against a float64 reference."""
    return tuple(ratio(getattr(res, n), getattr(ref, n), getattr(ref, "S" + n[1]), dtype) for n in GRADS)


def klass(key):
    return "split" if key.split else key.mma


# ---------------------------------------------------------------------------------------------------------------- the cases of the GPU matrix
SELF_SHAPES = ((1, 1, 1, 1), (2, 4, 64, 64), (3, 1, 65, 65), (2, 2, 63, 63))
CROSS_SHAPES = ((2, 2, 1, 70), (2, 2, 130, 5), (3, 1, 65, 129))
MASKS = ("none", "pad", "full")


def fast_cases(mma):
    """{no mask, pad mask, full mask} x {fused [B,T,3D+8], separate q with fused k|v} at the seven shapes; (2,2,63,63) with two rows between the items of a
    buffer (a batch stride that is not T st)."""
    return [Case(shape, mma=mma, mask=mask, layout=layout, ld_pad=8 if layout == "fused" else 0, sb_pad=2 if shape == (2, 2, 63, 63) else 0)
            for mask in MASKS for layout in ("fused", "cross") for shape in SELF_SHAPES + CROSS_SHAPES]


def general_cases(cls):
    """d_k 4, 36, 60 (one row between the items) and 64 behind ld = 3D + 4; bf16 / fp16: float32 rows with a 16-bit MFMA and no split, 16-bit rows
    with float32 dout at d_k = 64; split: 16-bit dout beside the float32 rows.  Each with no mask, a pad mask and a full mask."""
    mma, split = ("bf16", True) if cls == "split" else (cls, False)
    out = []
    for mask in MASKS:
        kw = dict(mma=mma, split=split, mask=mask)
        out += [Case((2, 2, 5, 5), dk=4, **kw), Case((1, 4, 16, 80), dk=36, layout="cross", **kw), Case((3, 2, 65, 129), dk=60, sb_pad=1, **kw),
                Case((3, 2, 65, 129), dk=64, ld_pad=4, **kw)]
        if split:
            out.append(Case((1, 4, 16, 80), dk=36, do16=True, **kw))
        else:
            out += [Case((3, 2, 65, 129), dk=64, f32=True, **kw), Case((3, 2, 65, 129), dk=64, do32=True, **kw)]
    return out


def dropout_cases(cls):
    """p = 0.1 at Tq != Tk (the element index is rid Tk + kj): fast, one per MFULL value; general, one per class."""
    if cls == "split":
        return [Case((3, 2, 65, 129), dk=60, split=True, mask="full", drop=0.1)]
    return [Case((3, 1, 65, 129), mma=cls, mask="pad", ld_pad=8, drop=0.1), Case((3, 1, 65, 129), mma=cls, mask="full", layout="cross", drop=0.1),
            Case((3, 2, 65, 129), dk=60, mma=cls, mask="full", drop=0.1)]


def peaked_cases():
    """q and k times 4: the scores spread over +-50, exp(scale s - lse) at large |s|; once on the fast path, once on the general one.  Both in bf16:
    probabilities below 2^-14 are subnormal in fp16 and lose their relative precision when pack8 rounds them, so at FP16_PEAKED the float32 yardstick
    itself stands at 0.2 (dk) and 0.4 (dv) of S (test_attention_bwd_ref_cpu.py keeps that figure) and would set a bound that no fp16 case could miss."""
    return [Case((3, 2, 63, 130), mask="pad", ld_pad=8, qk_scale=4.0), Case((3, 2, 63, 130), dk=36, mask="full", qk_scale=4.0)]


FP16_PEAKED = Case((3, 2, 63, 130), dk=36, mma="fp16", mask="full", qk_scale=4.0)      # no case of the matrix: see peaked_cases()


def both_ways_cases(mma):
    """d_k = 64 on the fast kernels (ld = 3D) and, the same operands, on the general ones (ld = 3D + 4)."""
    return [Case((3, 2, 65, 129), mma=mma, mask="full", ld_pad=pad) for pad in (0, 4)]


def group_cases(mma, mfull, n):
    """n fast problems of different shapes and one mask kind: cases of fast_cases(), so each problem's single call is the one check() made."""
    mask = "full" if mfull else "pad"
    shapes = ((2, 4, 64, 64), (3, 1, 65, 129), (2, 2, 1, 70)) if n == 3 else SELF_SHAPES + CROSS_SHAPES
    keys = [Case(s, mma=mma, mask=mask, ld_pad=8, sb_pad=2 if s == (2, 2, 63, 63) else 0) for s in shapes]
    if n == 8:
        keys.append(Case((3, 1, 65, 129), mma=mma, mask=mask, layout="cross"))
    assert len(keys) == n
    return keys


def chained_cases():
    """one per class through cfm.attention(lse=, drop=) and then cfm.attention_bwd: the reference takes the kernel's out and lse as given."""
    return [dropout_cases("bf16")[0], dropout_cases("fp16")[1], dropout_cases("split")[0]]


def yardstick_cases():
    """every Case of the GPU matrix, by class (the group and the chained cases are among them)."""
    by = {"bf16": [], "fp16": [], "split": general_cases("split") + dropout_cases("split")}
    for mma in ("bf16", "fp16"):
        by[mma] += fast_cases(mma) + general_cases(mma) + dropout_cases(mma) + both_ways_cases(mma)
    for c in peaked_cases():
        by[klass(c)].append(c)
    return by


@functools.lru_cache(maxsize=None)
def yardstick(key):
    """the float32 evaluation's (dq, dk, dv) ratios at one case, on the CPU keep mask."""
    P = problem(key)
    return ratios(evaluate(P, given(P, P.keep), F32), reference(key), P.io)


@functools.lru_cache(maxsize=None)
def measure_g():
    """-> {class: namespace(y (dq, dk, dv): the worst float32-torch ratios over the class's cases, g = 4 y: the margin of attention_ref.measure_g)}."""
    res = {}
    for cls, keys in yardstick_cases().items():
        ys = [yardstick(k) for k in keys]
        y = tuple(max(r[i] for r in ys) for i in range(3))
        res[cls] = SimpleNamespace(y=y, g=tuple(4.0 * v for v in y))
    return res


# every way a kernel could plausibly be wrong that the audit restates -> (cases of the GPU matrix, the gradients it hits): each of these gradients must
# leave the bound at one of the cases
_B = dict(mma="bf16", ld_pad=8)
_H = dict(mma="fp16", ld_pad=8)
VARIANTS = {
    "last_key_of_tile_dropped": ((Case((2, 4, 64, 64), mask="none", **_B),), ("dq", "dk", "dv")),
    "last_query_of_tile_dropped": ((Case((2, 4, 64, 64), mask="none", **_B),), ("dk", "dv")),
    "masked_keys_leak": ((Case((3, 1, 65, 129), mask="pad", **_B),), ("dq", "dk", "dv")),
    "lse_plus_0.02": ((Case((2, 2, 1, 70), mask="none", **_B), Case((2, 2, 1, 70), mask="pad", **_B), Case((3, 1, 65, 129), mask="pad", **_B), Case((3, 1, 65, 129), mask="pad", **_H)),
                      ("dq", "dk", "dv")),
    "masked_rows_uniform": ((Case((3, 1, 65, 129), mask="full", **_B),), ("dq", "dk", "dv")),
    "delta_omitted": ((Case((2, 4, 64, 64), mask="none", **_B),), ("dq", "dk")),
    "scale_missing": ((Case((2, 4, 64, 64), mask="none", **_B),), ("dq", "dk")),
    "drop_index_Tq": ((Case((3, 1, 65, 129), mask="pad", drop=0.1, **_B),), ("dq", "dk", "dv")),
    "dP_not_dropped": ((Case((3, 1, 65, 129), mask="pad", drop=0.1, **_B),), ("dq", "dk")),
    "m_sq_ignored": ((Case((3, 1, 65, 129), mask="full", **_B),), ("dq", "dk", "dv")),
    "mask_transposed": ((Case((3, 1, 65, 65), mask="full", **_B),), ("dq", "dk", "dv")),
    "k_sb_is_Tk_st": ((Case((2, 2, 63, 63), mask="none", sb_pad=2, **_B),), ("dq", "dk", "dv")),
    "dout_of_head_0": ((Case((2, 4, 64, 64), mask="none", **_B),), ("dq", "dk", "dv")),
}
# the inputs of tests/test_train_ops_gpu.py::test_attention_backward at (B,T,H,dk) = (2,249,4,64): ordinary random numbers in the dead rows
OLD_GATE_CASE = Case((2, 4, 249, 249), mask="lens", dead=None)
OLD_GATE = 3e-2
