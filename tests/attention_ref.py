"""cfm_attention restated from include/cfm.h (cfm_attn_desc), not from the kernels:  out[b,i,h,:] = softmax_j(scale ((q_i + u_h).k_j + (q_i + v_h).p_bj)) . v_j
on CPU tensors, every operand addressed by the element strides the descriptor carries (gather()).

`reference(key)` evaluates a Case in float64: out, lse, the probabilities a_ij and S_id = sum_j a_ij |v_jd|.  `evaluate(P, torch.float32)` is the
SAME formula in plain float32 torch on the same rounded operands -- the yardstick the bound is measured with (measure_g); `evaluate(P, variant=...)`
is a restatement that is wrong in one named way (VARIANTS), for the discrimination audit of tests/test_attention_ref_cpu.py.

Operands, as the kernels declare them: q + u and q + v are added in float32 and rounded to the MFMA type (without p there is no u either); f32 K / V
/ p are rounded to the MFMA type (load_row8 / pack8 on the fast path, pack_planes in the general kernel).  Split mode takes the unrounded
operands (the header's "f32-accurate"); its float32 yardstick is the header's three products hi.hi + lo.hi + hi.lo on bf16 planes, for both
the score and the P.V product.  A masked score is -inf; a fully masked row gives out = 0 and lse = -inf.

The one rounding the kernels' design adds to the float32 formula: the unnormalised probabilities exp(s - m) are rounded to the MFMA type before
the P.V product (pack8 of s[] into the next MFMA); the normaliser l = sum exp(s - m) stays float32.  The yardstick does exactly that.

Bound, per element, never a norm:  |out - ref| <= g S_id + ulp_out(ref)   and   |lse - ref| <= g_lse L_i,  L_i = scale max_j-live sum_d (|qu_id||k_jd| +
|qv_id||p_jd|); fully masked rows exactly 0 and exactly -inf; no NaN anywhere.  g and g_lse are 4 x the worst ratio of the float32 yardstick per
class (bf16, fp16, split) over yardstick_cases() -- the cases of tests/test_attention_matrix_gpu.py -- and never come from a kernel's output.
"""
import functools
import math
from collections import namedtuple
from types import SimpleNamespace

import torch

from gemm_ref import ulp

F32, BF16, F16, F64 = torch.float32, torch.bfloat16, torch.float16, torch.float64
MMA = {"bf16": BF16, "fp16": F16}
SK, KT = 256, 64                 # keys per super-tile of the fast path / per tile of the general kernel (csrc/attention.hip, attn_common.h)

# shape (B, H, Tq, Tk); pmode none | bcast (p_st = 0) | perkey | shared (p_sb = 0); mask none | pad (B,1,Tk) | full (B,Tq,Tk);
# layout fused ([B, T, 3D + ld_pad] q|k|v) | cache (q [B,Tq,D] 16 bit, K|V f32 [B,H,Tk,2dk]); f32: the fused buffer is float32 (q, K and V);
# qk_scale multiplies q and k (the rising-maximum cases); o16: out in the MFMA type instead of float32
Case = namedtuple("Case", "shape dk mma split pmode mask layout f32 ld_pad qk_scale o16 seed", defaults=(64, "bf16", False, "none", "none", "fused", False, 0, 1.0, False, 0))
Op = namedtuple("Op", "buf off sb st sh")


def rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


# ---------------------------------------------------------------------------------------------------------------- masks
def pad_mask(B, Tk, seed):
    """(B, Tk) key validity.  Item 0: about 70 % live, the last key live; item 1: one live key (key 0); the LAST item at Tk >= 257 (item 0 when B = 1):
    no live key among the first 256 (at Tk = 257 that is the utterance with one live key, and item 1 is right-padded like the others); every other item
    right-padded to a random length."""
    g = torch.Generator().manual_seed(seed)
    m = torch.zeros((B, Tk), dtype=torch.uint8)
    for b in range(B):
        if b == 0:
            m[b] = (torch.rand(Tk, generator=g) < 0.7).to(torch.uint8)
            m[b, Tk - 1] = 1
        elif b == 1 and not (Tk == SK + 1 and B > 2):
            m[b, 0] = 1
        else:
            m[b, :int(torch.randint(1, Tk + 1, (1,), generator=g))] = 1
    if Tk > SK:
        b = B - 1
        m[b] = (torch.rand(Tk, generator=g) < 0.7).to(torch.uint8)
        m[b, :SK] = 0
        m[b, Tk - 1] = 1
    return m


def full_mask(B, Tq, Tk, seed):
    """(B, Tq, Tk), 60 % dense.  Row min(3, Tq - 1) of item 0 is fully masked (not at Tq = 1); at Tk >= 257 the even rows of the last item have no
    live key among the first 256 (and a live last key)."""
    g = torch.Generator().manual_seed(seed)
    m = (torch.rand((B, Tq, Tk), generator=g) < 0.6).to(torch.uint8)
    m[:, :, 0] |= (m.sum(-1) == 0).to(torch.uint8)            # no accidental dead row
    if Tk > SK:
        m[B - 1, 0::2, :SK] = 0
        m[B - 1, 0::2, Tk - 1] = 1
    if Tq > 1:
        m[0, min(3, Tq - 1)] = 0
    return m


# ---------------------------------------------------------------------------------------------------------------- problems
@functools.lru_cache(maxsize=None)
def problem(key):
    """One descriptor on CPU tensors, made once and never written to: bufs name -> (tensor [rows.., cols], row stride ld) as they are placed in
    memory (gaps between cols and ld are no part of any operand), ops name -> Op(buffer, element offset, batch / time / head stride)."""
    B, H, Tq, Tk = key.shape
    dk, D = key.dk, H * key.dk
    mma = MMA[key.mma]
    s = 1000 * key.seed + 131 * B + 17 * Tq + Tk + 7 * H + dk
    P = SimpleNamespace(key=key, B=B, H=H, Tq=Tq, Tk=Tk, dk=dk, D=D, mma=mma, split=key.split, scale=float(dk) ** -0.5, bufs={}, ops={}, p_str=(0, 0),
                        mask_str=(0, 0), u=None, vb=None, out_dtype=mma if key.o16 else F32)
    q, k, v = rnd((B, Tq, D), s + 1, key.qk_scale), rnd((B, Tk, D), s + 2, key.qk_scale), rnd((B, Tk, D), s + 3)
    if key.layout == "fused":
        dt = F32 if key.f32 else mma
        Tm, ld = max(Tq, Tk), 3 * D + key.ld_pad
        buf = torch.zeros((B, Tm, 3 * D))
        buf[:, :Tq, :D], buf[:, :Tk, D:2 * D], buf[:, :Tk, 2 * D:] = q, k, v
        P.bufs["qkv"] = (buf.to(dt), ld)
        P.ops["q"], P.ops["k"], P.ops["v"] = Op("qkv", 0, Tm * ld, ld, dk), Op("qkv", D, Tm * ld, ld, dk), Op("qkv", 2 * D, Tm * ld, ld, dk)
        P.q_dtype = P.kv_dtype = dt
    else:
        cache = torch.cat([k.reshape(B, Tk, H, dk), v.reshape(B, Tk, H, dk)], -1).permute(0, 2, 1, 3).contiguous()      # [B, H, Tk, 2dk]
        P.bufs["q"], P.bufs["cache"] = (q.to(mma), D), (cache, 2 * dk)
        P.ops["q"] = Op("q", 0, Tq * D, D, dk)
        P.ops["k"], P.ops["v"] = Op("cache", 0, H * Tk * 2 * dk, 2 * dk, Tk * 2 * dk), Op("cache", dk, H * Tk * 2 * dk, 2 * dk, Tk * 2 * dk)
        P.q_dtype, P.kv_dtype = mma, F32
    if key.pmode != "none":
        pdt = F32 if (key.f32 and key.layout == "fused") else mma
        Bp, Tp = (1 if key.pmode == "shared" else B), (1 if key.pmode == "bcast" else Tk)
        P.bufs["p"] = (rnd((Bp, Tp, D), s + 4, 0.5).to(pdt), D)
        P.ops["p"] = Op("p", 0, 0 if key.pmode == "shared" else Tp * D, 0 if key.pmode == "bcast" else D, dk)
        P.p_str, P.p_dtype = (P.ops["p"].sb, P.ops["p"].st), pdt
        P.u, P.vb = rnd((H, dk), s + 5, 0.3), rnd((H, dk), s + 6, 0.3)
    if key.mask == "pad":
        P.bufs["mask"], P.mask_str = (pad_mask(B, Tk, s + 7), Tk), (Tk, 0)
    elif key.mask == "full":
        m_sq = Tk + 3                                           # a padded row stride: reading rows Tk apart is a different mask
        P.bufs["mask"], P.mask_str = (full_mask(B, Tq, Tk, s + 7), m_sq), (Tq * m_sq, m_sq)
    return P


def flat(t, ld):
    """the buffer as it lies in memory, gaps included: what lies outside an operand is NaN (masks: 1, "valid"), as tests/extent.py plants it."""
    cols = t.shape[-1]
    rows = t.numel() // cols
    buf = torch.full((rows, ld), 1 if t.dtype == torch.uint8 else float("nan"), dtype=t.dtype)
    buf[:, :cols] = t.reshape(rows, cols)
    return buf.reshape(-1)


def gather(fl, idx):
    """fl[idx] with whatever lies past the allocation's end read as NaN (masks: 1)."""
    oob = idx >= fl.numel()
    out = fl[idx.clamp_max(fl.numel() - 1)]
    return torch.where(oob, torch.full_like(out, 1 if fl.dtype == torch.uint8 else float("nan")), out)


def fetch(P, name, T, op=None):
    """operand `name` as [B, H, T, dk]: element (b, t, h, d) at off + b sb + t st + h sh + d."""
    op = op or P.ops[name]
    a = torch.arange
    idx = op.off + a(P.B)[:, None, None, None] * op.sb + a(P.H)[None, :, None, None] * op.sh + a(T)[None, None, :, None] * op.st + a(P.dk)
    return gather(flat(*P.bufs[op.buf]), idx)


def fetch_mask(P, m_sb, m_sq):
    a = torch.arange
    nq = P.Tq if m_sq else 1
    idx = a(P.B)[:, None, None] * m_sb + a(nq)[None, :, None] * m_sq + a(P.Tk)
    return gather(flat(*P.bufs["mask"]), idx) != 0           # [B, Tq | 1, Tk]


# ---------------------------------------------------------------------------------------------------------------- which kernel
def predicted_kernel(P):
    """A mirror of csrc/attention.hip: attn_args' `fast` predicate with its al8 alignment rule, the profile name cfm_attention picks, and
    launch_attn2's pmode / mfull / kvf32 / 128-query condition.  -> namespace(name, fast, q128, mfull, kvf32, pmode)."""
    q, k, v = P.ops["q"], P.ops["k"], P.ops["v"]
    pos = "p" in P.ops
    p_sb, p_st = P.p_str
    al8 = q.sb % 8 == 0 and q.st % 8 == 0 and k.sb % 4 == 0 and k.st % 8 == 0 and k.sh % 8 == 0 and v.sb % 4 == 0 and v.st % 8 == 0 and v.sh % 8 == 0 and \
        (not pos or (p_sb % 8 == 0 and p_st % 8 == 0))
    fast = not P.split and P.dk == 64 and P.q_dtype == P.mma and (not pos or P.p_dtype == P.mma) and P.kv_dtype in (P.mma, F32) and al8 and \
        P.Tk * k.st < 2 ** 31 and P.Tk * v.st < 2 ** 31 and P.Tk * p_st < 2 ** 31
    pmode = 0 if not pos else (1 if p_st == 0 else 2)
    mfull = "mask" in P.bufs and P.mask_str[1] != 0
    kvf32 = P.kv_dtype == F32
    pairs = P.B * P.H
    q128 = fast and not mfull and not kvf32 and pmode != 2 and P.Tq > 64 and (pairs + 7) // 8 * 8 * ((P.Tq + 127) // 128) >= 192
    tag = "bf16" if P.mma == BF16 else "f16"
    name = ("attn2" if fast else "attn") + ("_rel" if pos else "") + "_" + tag + ("x3" if P.split else "")
    return SimpleNamespace(name=name, fast=fast, q128=q128, mfull=mfull, kvf32=kvf32, pmode=pmode)


# ---------------------------------------------------------------------------------------------------------------- the operation
def hilo(x):
    hi = x.to(BF16)
    return hi.float(), (x - hi.float()).to(BF16).float()


def product(a, b, dt, split):
    """a [.., M, K] . b [.., N, K]^T.  float64: exact operands.  float32 split: the header's three products on bf16 planes."""
    if dt == F64 or not split:
        return a.to(dt) @ b.to(dt).transpose(-1, -2)
    ah, al = hilo(a)
    bh, bl = hilo(b)
    return ah @ bh.transpose(-1, -2) + al @ bh.transpose(-1, -2) + ah @ bl.transpose(-1, -2)


def online(s, V, tile, variant):
    """the online softmax over key tiles in float64, with one of two defects: alpha_one (the accumulators are not rescaled when the running maximum
    rises) or dead_tile_nan (exp(-inf - (-inf)) while no key has been live yet)."""
    ninf = float("-inf")
    m_run = torch.full(s.shape[:-1], ninf, dtype=F64)
    l = torch.zeros(s.shape[:-1], dtype=F64)
    acc = torch.zeros(s.shape[:-1] + (V.shape[-1],), dtype=F64)
    for t0 in range(0, s.shape[-1], tile):
        st, Vt = s[..., t0:t0 + tile], V[..., t0:t0 + tile, :]
        m_new = torch.maximum(m_run, st.max(-1).values)
        if variant == "dead_tile_nan":
            alpha, pv = torch.exp(m_run - m_new), torch.exp(st - m_new[..., None])
        else:
            dead = m_new == ninf
            alpha = torch.where(dead, torch.ones_like(l), torch.exp(m_run - torch.where(dead, torch.zeros_like(l), m_new)))
            pv = torch.where(dead[..., None], torch.zeros_like(st), torch.exp(st - torch.where(dead, torch.zeros_like(l), m_new)[..., None]))
        if variant == "alpha_one":
            alpha = torch.where(torch.isfinite(m_run) & (m_new > m_run), torch.ones_like(alpha), alpha)
        l = l * alpha + pv.sum(-1)
        acc = acc * alpha[..., None] + pv @ Vt
        m_run = m_new
    inv = torch.where(l > 0, 1.0 / l, torch.zeros_like(l))                   # NaN > 0 is false, as in the kernel: 0 times a NaN accumulator
    return acc * inv[..., None], torch.where(l > 0, m_run + torch.log(l), torch.full_like(l, ninf))


def evaluate(P, dt=F64, variant=None):
    """-> namespace(out [B,Tq,H*dk] in dt, lse [B,H,Tq], a [B,H,Tq,Tk] (float64 only), S [B,Tq,H*dk] and L [B,H,Tq] float64: the scales of the bounds)."""
    B, H, Tq, Tk, dk = P.B, P.H, P.Tq, P.Tk, P.dk
    pos = "p" in P.ops
    cache = P.ops["k"].buf == "cache"
    kop, vop = P.ops["k"], P.ops["v"]
    if variant == "v_at_k_half" and cache:
        vop = vop._replace(off=kop.off)
    if variant == "k_sh_is_dk" and cache:
        kop, vop = kop._replace(sh=dk), vop._replace(sh=dk)
    Q, K, V = fetch(P, "q", Tq), fetch(P, "k", Tk, kop), fetch(P, "v", Tk, vop)
    zero = torch.zeros((H, dk))
    u, vb = (P.u, P.vb) if pos else (zero, zero)
    if variant == "uv_swapped":
        u, vb = vb, u
    if variant == "bias_of_head_0":
        u, vb = u[:1].expand(H, dk), vb[:1].expand(H, dk)
    Pp = None
    if pos:
        pop = P.ops["p"]
        if variant == "p_at_j_plus_1" and pop.st:
            pop = pop._replace(off=pop.st)
        if variant == "p_of_stream_0" and pop.sb:
            pop = pop._replace(sb=0)
        if variant == "p_sb_0_ignored" and pop.sb == 0 and pop.st:
            pop = pop._replace(sb=Tk * P.D)                   # the next streams' rows of a table that has one: outside its extent
        Pp = fetch(P, "p", Tk if pop.st else 1, pop)
        if variant == "bcast_dropped" and pop.st == 0:
            Pp = torch.zeros_like(Pp)
    live = torch.ones((B, 1, Tk), dtype=torch.bool)
    if "mask" in P.bufs:
        m_sb, m_sq = P.mask_str
        if variant == "full_mask_stride_Tk" and m_sq:
            m_sq = Tk
        if variant == "pad_mask_of_batch_0" and not m_sq:
            m_sb = 0
        live = fetch_mask(P, m_sb, m_sq)
    if variant == "last_key_skipped":
        j = torch.arange(Tk)
        live = live & ~((j % SK == SK - 1) | (j == Tk - 1))
    live = live[:, None]                                        # [B, 1, Tq | 1, Tk]
    # ---- operands as the kernels declare them
    qu32, qv32 = Q.float() + u[None, :, None, :], Q.float() + vb[None, :, None, :]
    if P.split:
        if dt == F64:
            qu, qv = Q.double() + u.double()[None, :, None, :], Q.double() + vb.double()[None, :, None, :]
        else:
            qu, qv = qu32, qv32
        Kr, Vr, Pr = K.float(), V.float(), None if Pp is None else Pp.float()
    else:
        r = lambda x: x.float().to(P.mma).float()
        qu, qv, Kr, Vr, Pr = r(qu32), r(qv32), r(K), r(V), None if Pp is None else r(Pp)
    ac = product(qu, Kr, dt, P.split)
    bd = product(qv, Pr, dt, P.split) if pos else torch.zeros((), dtype=dt)
    scale = P.scale if dt == F64 else torch.tensor(P.scale, dtype=dt)
    s = scale * ac + bd if variant == "scale_on_content_only" else scale * (ac + bd)
    ninf = float("-inf")
    s = torch.where(live, s, torch.full_like(s, ninf))
    Vd = Vr.to(dt)
    if variant == "pad_keys_live":                            # keys [Tk, 256 ceil(Tk / 256)): zero rows that count as live
        npad = -Tk % SK
        s = torch.cat([s, torch.zeros(s.shape[:-1] + (npad,), dtype=dt)], -1)
        Vd = torch.cat([Vd, torch.zeros(Vd.shape[:-2] + (npad, dk), dtype=dt)], -2)
    a = None
    if variant in ("alpha_one", "dead_tile_nan"):
        out, lse = online(s, Vd, SK if predicted_kernel(P).fast else KT, variant)
    else:
        m = s.max(-1, keepdim=True).values
        dead = m == ninf
        e = torch.where(dead, torch.zeros_like(s), torch.exp(s - torch.where(dead, torch.zeros_like(m), m)))
        l = e.sum(-1, keepdim=True)
        if dt == F64:
            a = torch.where(dead, torch.zeros_like(e), e / torch.where(dead, torch.ones_like(l), l))
            out = a @ Vd
        else:                                                   # the kernels' one extra rounding: exp(s - m) in the operand type, l in float32
            if P.split:
                eh, el = hilo(e)
                vh, vl = hilo(Vd)
                acc = eh @ vh + el @ vh + eh @ vl
            else:
                acc = e.to(P.mma).float() @ Vd
            out = torch.where(dead, torch.zeros_like(acc), acc / torch.where(dead, torch.ones_like(l), l))
        lse = torch.where(dead, torch.full_like(m, ninf), m + torch.log(torch.where(dead, torch.ones_like(l), l))).squeeze(-1)
        dead = dead.squeeze(-1)
        if variant == "masked_row_mean_v":
            out = torch.where(dead[..., None], Vd.mean(-2, keepdim=True).expand_as(out), out)
        if variant == "masked_row_finite_lse":
            lse = torch.where(dead, torch.full_like(lse, -3.0e38), lse)
    res = SimpleNamespace(out=out.permute(0, 2, 1, 3).reshape(B, Tq, H * dk), lse=lse, a=a, S=None, L=None)
    if dt == F64 and variant is None:
        res.S = (a @ Vd.abs()).permute(0, 2, 1, 3).reshape(B, Tq, H * dk)
        ab = qu.double().abs() @ Kr.double().abs().transpose(-1, -2)
        if pos:
            ab = ab + qv.double().abs() @ Pr.double().abs().transpose(-1, -2)
        res.L = P.scale * torch.where(live, torch.nan_to_num(ab), torch.zeros_like(ab)).max(-1).values
    return res


@functools.lru_cache(maxsize=None)
def reference(key):
    return evaluate(problem(key))


# ---------------------------------------------------------------------------------------------------------------- the bound
def ratios(out, lse, ref, out_dtype):
    """-> (worst (|out - ref| - ulp_out) / S, worst |lse - ref| / L) over the rows with a live key; inf where a NaN appears, where a fully masked row
    is not exactly 0 / -inf or where lse is infinite on a live row."""
    o, ls = out.double(), lse.double()
    d = (o - ref.out).abs()
    ro = (d - ulp(ref.out, out_dtype)).clamp_min(0) / ref.S
    ro = torch.where(ref.S == 0, torch.where(o == 0, torch.zeros_like(d), torch.full_like(d, math.inf)), ro)
    ro = torch.where(torch.isnan(o), torch.full_like(d, math.inf), ro)
    dead = ref.lse == -math.inf
    rl = (ls - ref.lse).abs() / ref.L
    rl = torch.where(dead, torch.where(ls == -math.inf, torch.zeros_like(rl), torch.full_like(rl, math.inf)), rl)
    rl = torch.where(torch.isnan(ls) | (~dead & torch.isinf(ls)), torch.full_like(rl, math.inf), rl)
    return float(ro.max()), float(rl.max())


def klass(key):
    return "split" if key.split else key.mma


# ---------------------------------------------------------------------------------------------------------------- the cases of the GPU matrix
FAST_SHAPES = ((1, 1, 1, 1), (3, 1, 65, 257), (1, 9, 17, 513), (2, 4, 64, 256), (2, 2, 63, 255))
Q128_SHAPES = ((24, 4, 130, 130), (24, 4, 129, 257))
GENERAL_SHAPES = ((2, 2, 5, 5), (1, 4, 16, 80), (3, 2, 65, 129))


def fast_cases(mma):
    """{no p, broadcast p, per-key p} x {pad mask (no mask at the one-key shape and at 64 x 256), full mask} x {fused 16 bit, f32 cache}: the 12
    cfm_attn2_kernel instances of one type, each at five shapes; per-key p once as the shared table (p_sb = 0)."""
    out = []
    for pm in ("none", "bcast", "perkey"):
        for full in (False, True):
            for layout in ("fused", "cache"):
                for shape in FAST_SHAPES:
                    mask = "full" if full else ("none" if shape in ((1, 1, 1, 1), (2, 4, 64, 256)) else "pad")
                    out.append(Case(shape, mma=mma, pmode=pm, mask=mask, layout=layout, ld_pad=8 if shape[3] == 255 and layout == "fused" else 0,
                                    o16=layout == "fused"))
    out += [Case((3, 1, 65, 257), mma=mma, pmode="shared", mask="pad", layout=layout, o16=layout == "fused") for layout in ("fused", "cache")]
    return out


def q128_cases(mma):
    return [Case(shape, mma=mma, pmode=pm, mask=mask, o16=True) for shape in Q128_SHAPES for pm, mask in (("none", "none"), ("bcast", "pad"), ("none", "pad"), ("bcast", "none"))]


def rising_cases():
    """q and k times 4: the scores spread over +-50, so a row's dominating key falls in any tile, the last one included."""
    return [Case((3, 2, 63, 600), pmode="perkey", mask="pad", qk_scale=4.0), Case((3, 2, 63, 600), dk=36, pmode="perkey", mask="pad", qk_scale=4.0),
            Case((3, 2, 65, 150), dk=60, mma="fp16", mask="full", qk_scale=4.0)]


def general_cases(cls):
    """{bf16, fp16, split} x {p, no p} at d_k 4, 36, 60 and at 64 behind a row stride of 3D + 4; f32 q|K|V, and 16-bit q with the f32 cache."""
    mma, split = ("bf16", True) if cls == "split" else (cls, False)
    out = []
    for pm, mask in (("none", "pad"), ("perkey", "full"), ("bcast", "none"), ("shared", "pad")):
        for shape, dk in (((2, 2, 5, 5), 4), ((1, 4, 16, 80), 36), ((3, 2, 65, 129), 60), ((3, 2, 65, 129), 64)):
            out.append(Case(shape, dk=dk, mma=mma, split=split, pmode=pm, mask=mask, f32=split, ld_pad=4 if dk == 64 else 0, o16=not split and pm == "none"))
        out.append(Case((1, 4, 16, 80), dk=36, mma=mma, split=split, pmode=pm, mask=mask, f32=True))                # q f32, K / V f32
        out.append(Case((3, 2, 65, 129), dk=60, mma=mma, split=split, pmode=pm, mask=mask, layout="cache"))       # q 16 bit, K / V f32
    return out


def both_ways_cases(mma):
    """d_k = 64 on the fast path (ld = 3D) and, the same operands, on the general kernel (ld = 3D + 4)."""
    return [Case((3, 2, 65, 129), mma=mma, pmode="perkey", mask="full", ld_pad=pad) for pad in (0, 4)]


# the streaming form: ring_T slots, chunk T, need = cached frames; per call B = 3 stream offsets
RING_T, CHUNK, NEED, STREAM_H = 300, 16, 16, 2
STREAM_OFFSETS = ((0, 8, 590),        # no cached frame; fewer than `need`; slots 274 .. 299 and 0 .. 5: the live interval wraps, the first super-tile is partly dead
                  (876, 16, 299))     # slots 260 .. 291: the first super-tile is wholly dead; exactly `need`; the chunk itself wraps (slot 299, then 0 .. 14)


def stream_frames(offsets, mma, seed=0):
    """-> namespace(q [B,T,D] 16 bit, k / v / p [B, NEED + T, D] 16 bit: row NEED - cached_b + i is frame off_b - cached_b + i, the rows before hold
    nothing (NaN); cached [B])."""
    B, D = len(offsets), STREAM_H * 64
    s = 5000 + 10 * seed + sum(offsets)
    dt = MMA[mma]
    cached = [min(o, NEED) for o in offsets]
    f = SimpleNamespace(q=rnd((B, CHUNK, D), s + 1).to(dt), k=rnd((B, NEED + CHUNK, D), s + 2).to(dt), v=rnd((B, NEED + CHUNK, D), s + 3).to(dt),
                        p=rnd((B, NEED + CHUNK, D), s + 4, 0.5).to(dt), u=rnd((STREAM_H, 64), s + 5, 0.3), vb=rnd((STREAM_H, 64), s + 6, 0.3), cached=cached, offsets=offsets)
    for b, c in enumerate(cached):
        for t in (f.k, f.v, f.p):
            t[b, :NEED - c] = float("nan")
    return f


def stream_slots(off):
    """[(slot, frame)] of the live frames of a stream at offset `off`, in time order."""
    return [(fr % RING_T, fr) for fr in range(off - min(off, NEED), off + CHUNK)]


@functools.lru_cache(maxsize=None)
def stream_problem(offsets, mma, b, seed=0):
    """stream b alone, its live frames gathered in time order: plain attention, no mask, per-key p.  The GPU side reads the same frames from ring slots."""
    f = stream_frames(offsets, mma, seed)
    n, D, dk, H = f.cached[b] + CHUNK, STREAM_H * 64, 64, STREAM_H
    key = Case((1, H, CHUNK, n), mma=mma, pmode="perkey", layout="cache")
    P = SimpleNamespace(key=key, B=1, H=H, Tq=CHUNK, Tk=n, dk=dk, D=D, mma=MMA[mma], split=False, scale=dk ** -0.5, bufs={}, ops={}, mask_str=(0, 0),
                        out_dtype=F32, q_dtype=MMA[mma], kv_dtype=F32, p_dtype=MMA[mma])
    k, v = f.k[b, NEED - f.cached[b]:].float(), f.v[b, NEED - f.cached[b]:].float()
    cache = torch.cat([k.reshape(1, n, H, dk), v.reshape(1, n, H, dk)], -1).permute(0, 2, 1, 3).contiguous()
    P.bufs["q"], P.bufs["cache"], P.bufs["p"] = (f.q[b:b + 1], D), (cache, 2 * dk), (f.p[b:b + 1, NEED - f.cached[b]:], D)
    P.ops["q"], P.ops["p"] = Op("q", 0, CHUNK * D, D, dk), Op("p", 0, n * D, D, dk)
    P.ops["k"], P.ops["v"] = Op("cache", 0, H * n * 2 * dk, 2 * dk, n * 2 * dk), Op("cache", dk, H * n * 2 * dk, 2 * dk, n * 2 * dk)
    P.p_str, P.u, P.vb = (n * D, D), f.u, f.vb
    return P


@functools.lru_cache(maxsize=None)
def stream_reference(offsets, mma, b, seed=0):
    return evaluate(stream_problem(offsets, mma, b, seed))


def yardstick_cases():
    """every Case of the GPU matrix, by class."""
    by = {"bf16": [], "fp16": [], "split": general_cases("split")}
    for mma in ("bf16", "fp16"):
        by[mma] += fast_cases(mma) + q128_cases(mma) + general_cases(mma) + both_ways_cases(mma)
    for c in rising_cases():
        by[klass(c)].append(c)
    return by


@functools.lru_cache(maxsize=None)
def yardstick(key):
    """the float32 evaluation's (out ratio, lse ratio) at one case."""
    P, ref = problem(key), reference(key)
    t = evaluate(P, F32)
    return ratios(t.out, t.lse, ref, F32)


@functools.lru_cache(maxsize=None)
def measure_g():
    """-> {class: namespace(g, g_lse, y, y_lse)}: the worst float32-torch ratios y over the class's cases (the streaming problems included) and
    g = 4 y, the margin gemm_ref.measure_g uses."""
    res = {}
    for cls, keys in yardstick_cases().items():
        ys = [yardstick(k) for k in keys]
        if cls != "split":
            for offs in STREAM_OFFSETS:
                for b in range(len(offs)):
                    P, ref = stream_problem(offs, cls, b), stream_reference(offs, cls, b)
                    t = evaluate(P, F32)
                    ys.append(ratios(t.out, t.lse, ref, F32))
        y, yl = max(r[0] for r in ys), max(r[1] for r in ys)
        res[cls] = SimpleNamespace(g=4.0 * y, g_lse=4.0 * yl, y=y, y_lse=yl)
    return res


# every way a kernel could plausibly be wrong that the audit restates -> the case of the GPU matrix whose inputs must show it
_F = lambda shape, **kw: Case(shape, **kw)
VARIANTS = {
    "last_key_skipped": _F((2, 4, 64, 256), pmode="none", mask="none", o16=True),
    "pad_keys_live": _F((2, 2, 63, 255), pmode="none", mask="pad", ld_pad=8, o16=True),
    "full_mask_stride_Tk": _F((3, 1, 65, 257), pmode="none", mask="full", o16=True),
    "pad_mask_of_batch_0": _F((3, 1, 65, 257), pmode="none", mask="pad", o16=True),
    "uv_swapped": _F((3, 1, 65, 257), pmode="perkey", mask="pad", o16=True),
    "bias_of_head_0": _F((1, 9, 17, 513), pmode="perkey", mask="pad", o16=True),
    "p_at_j_plus_1": _F((3, 1, 65, 257), pmode="perkey", mask="pad", o16=True),
    "p_of_stream_0": _F((3, 1, 65, 257), pmode="perkey", mask="pad", o16=True),
    "p_sb_0_ignored": _F((3, 1, 65, 257), pmode="shared", mask="pad", o16=True),
    "bcast_dropped": _F((3, 1, 65, 257), pmode="bcast", mask="pad", o16=True),
    "alpha_one": _F((3, 2, 63, 600), pmode="perkey", mask="pad", qk_scale=4.0),
    "dead_tile_nan": _F((3, 1, 65, 257), pmode="none", mask="pad", o16=True),
    "masked_row_mean_v": _F((2, 4, 64, 256), pmode="none", mask="full", o16=True),
    "masked_row_finite_lse": _F((2, 4, 64, 256), pmode="none", mask="full", o16=True),
    "v_at_k_half": _F((2, 4, 64, 256), pmode="none", mask="none", layout="cache"),
    "k_sh_is_dk": _F((2, 4, 64, 256), pmode="none", mask="none", layout="cache"),
    "scale_on_content_only": _F((3, 1, 65, 257), pmode="perkey", mask="pad", o16=True),
}
LSE_ONLY = ("bcast_dropped",)      # constant over the keys: the softmax cancels it, only lse can tell
