"""cfm_gemm restated from include/cfm.h (cfm_gemm_desc), not from the kernel: C = epilogue(A[M,K] . W[N,K]^T) on CPU tensors.

`evaluate(p)` runs a Problem in float64 -- the reference; `evaluate(p, torch.float32)` is the SAME formula in plain float32 torch on the
same rounded operands -- the yardstick the bound is measured with (measure_g); `evaluate(p, variant=...)` is a float64 restatement that is
wrong in one named way (VARIANTS), for the discrimination audit of tests/test_gemm_ref_cpu.py.

Operand rounding: 16-bit A and W are used as given; f32 A without W_lo is rounded to W's type first; with W_lo the reference is the exact
product of f32 A with W_hi + W_lo (the float32 yardstick then is the header's three-product formula A_hi.W_hi + A_lo.W_hi + A_hi.W_lo).
Epilogue order: acc + bias (a mask_mode 1 dead row has acc = 0) -> C_pre -> activation -> dropout, second dropout on element m*N_out + n
(DSILU: on acc) -> mask_mode 0 / row_len zero the row -> residual + alpha * v -> rounding to c_dtype.
S = sum_k |a||w| + |bias| per element (GLU: of the value column) scales the bound: |out - ref| <= g * S (+ one ulp of a 16-bit output).
"""
import functools
from types import SimpleNamespace

import numpy as np
import torch

ACT_NONE, ACT_SILU, ACT_RELU, ACT_GLU, ACT_DSILU, ACT_DRELU = range(6)
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
W_DT = {"bf16": BF16, "fp16": F16}
FILL = -3.0      # what padding columns hold before a call (exact in every type)


# ---------------------------------------------------------------------------------------------------------------- dropout
def hash32(seed, idx):
    """csrc/cfm_common.h cfm_hash32 on numpy uint32 arrays (murmur3's finaliser over (idx * golden ratio) ^ seed)."""
    m = np.uint64(0xFFFFFFFF)
    h = ((idx.astype(np.uint64) * np.uint64(0x9E3779B1)) & m) ^ np.uint64(seed & 0xFFFFFFFF)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & m
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & m
    h ^= h >> np.uint64(16)
    return h.astype(np.uint32)


def keep_mask(n, p, seed):
    """keep(seed, element) for elements 0..n-1: hash >= p * 2^32, p as the float the ABI receives (cfm_make_drop)."""
    thresh = int(float(np.float32(p)) * 4294967296.0)
    return torch.from_numpy(hash32(seed, np.arange(n, dtype=np.uint64)) >= np.uint32(thresh))


def drop_scale(p):
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))      # the kernel's float constant 1 / (1 - p)


# ---------------------------------------------------------------------------------------------------------------- pieces
def im2col(img, T2, F2, order="tf"):
    """channels-last image [B,T1,F1,C] -> rows (b,t2,f2) of the 3x3 stride-2 convolution, K ordered (kt,kf,c)."""
    B, _, _, C = img.shape
    taps = [(kt, kf) for kt in range(3) for kf in range(3)] if order == "tf" else [(kt, kf) for kf in range(3) for kt in range(3)]
    cols = [img[:, kt:kt + 2 * T2 - 1:2, kf:kf + 2 * F2 - 1:2, :] for kt, kf in taps]
    return torch.stack(cols, 3).reshape(B * T2 * F2, 9 * C)


def glu_split(x):
    """[M,N] interleaved in 16-column blocks [a0..a15 | g0..g15 | a16..] -> (value, gate), N/2 columns each."""
    M, N = x.shape
    b = x.reshape(M, N // 32, 2, 16)
    return b[:, :, 0].reshape(M, N // 2), b[:, :, 1].reshape(M, N // 2)


def ulp(ref, dtype):
    """one unit in the last place of `dtype` at |ref| (float64 tensor)."""
    if dtype == F32:
        return torch.zeros_like(ref)
    mant, emin = (7, -126) if dtype == BF16 else (10, -14)
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** emin))).clamp_min(emin)
    return torch.where(torch.isfinite(ref), 2.0 ** (e - mant), torch.zeros_like(ref))


def rows_kept(p, variant=None):
    """bool [M]: rows the row_mask / row_len select keeps."""
    keep = torch.ones(p.M, dtype=torch.bool)
    if p.row_mask is not None:
        keep &= p.row_mask != 0
    if p.row_len is not None:
        m = torch.arange(p.M)
        b = m // (p.M if variant == "row_len_by_M" else p.row_T)
        t = m - b * p.row_T
        ln = p.row_len.long()[b]
        keep &= (t <= ln) if variant == "row_len_le" else (t < ln)
    return keep


# ---------------------------------------------------------------------------------------------------------------- the operation
def evaluate(p, dt=torch.float64, variant=None):
    """-> namespace(out: [M,N_out] in dt before the rounding to c_dtype, out_c: rounded to c_dtype, pre / pre_c: C_pre or None,
    S: [M,N_out] float64, S_pre: [M,N] float64)."""
    wdt = p.W.dtype
    A = p.A
    if p.conv is not None:
        C, T1, F1, T2, F2 = p.conv
        A = im2col(p.A, T2, F2, "ft" if variant == "conv_taps_ft" else "tf")
    if p.W_lo is not None:
        if dt == torch.float64:
            Ad, Wd = A.double(), p.W.double() + p.W_lo.double()
            acc = Ad @ Wd.t()
        else:                                           # the header's formula, as float32 torch evaluates it
            hi = A.to(BF16)
            lo = (A - hi.float()).to(BF16)
            acc = hi.float() @ p.W.float().t() + lo.float() @ p.W.float().t() + hi.float() @ p.W_lo.float().t()
            Ad, Wd = A.double(), p.W.double() + p.W_lo.double()
    else:
        if A.dtype == F32 and variant != "a32_not_rounded":
            A = A.to(wdt)
        Ad, Wd = A.double(), p.W.double()
        acc = A.to(dt) @ p.W.to(dt).t()
    with np.errstate(all="ignore"):
        S = torch.nan_to_num(Ad.abs(), nan=0.0, posinf=0.0) @ Wd.abs().t()
    bias = torch.zeros(p.N) if p.bias is None else p.bias
    S = S + bias.double().abs()
    dead = ~rows_kept(p, variant)
    if p.mask_mode == 1 and p.row_mask is not None:
        acc = torch.where(dead[:, None], torch.zeros_like(acc), acc)
    v = acc + bias.to(dt)
    if variant == "bias_dropped_on_dead_rows" and p.mask_mode == 1:
        v = torch.where(dead[:, None], torch.zeros_like(v), v)
    pre = v if p.pre_dtype is not None else None
    alpha = float(np.float32(p.alpha))
    glu = p.act == ACT_GLU
    S_out = glu_split(S)[0] if glu else S
    n_out = p.N // 2 if glu else p.N

    def keep(drop, ncols, stride):
        idx = (np.arange(p.M, dtype=np.uint64)[:, None] * np.uint64(stride) + np.arange(ncols, dtype=np.uint64)[None, :]) & np.uint64(0xFFFFFFFF)
        return torch.from_numpy(hash32(drop[1], idx) >= np.uint32(int(float(np.float32(drop[0])) * 4294967296.0)))

    def dropout(x, ncols, stride):
        x = torch.where(keep(p.drop, ncols, stride), x * drop_scale(p.drop[0]), torch.zeros_like(x))
        if p.drop2 is not None:
            x = torch.where(keep(p.drop2, ncols, stride), x * drop_scale(p.drop2[0]), torch.zeros_like(x))
        return x

    if glu:
        a, g = glu_split(v)
        if variant == "glu_halves_swapped":
            a, g = g, a
        elif variant == "glu_not_interleaved":
            a, g = v[:, :n_out], v[:, n_out:]
        elif variant == "glu_gate_wrong_fragment":                   # the gate of the NEXT block pair (fragment j + 2 instead of j + 1)
            g = torch.roll(g.reshape(p.M, -1, 16), -1, 1).reshape(p.M, n_out)
        v = a * torch.sigmoid(g)
    elif p.act == ACT_SILU:
        v = v * torch.sigmoid(v)
    elif p.act == ACT_RELU:
        v = torch.clamp_min(torch.nan_to_num(v, nan=0.0, posinf=float("inf"), neginf=-float("inf")), 0.0) if variant == "relu_drops_nan" else torch.relu(v)
    elif p.act == ACT_DSILU:
        if p.drop is not None:
            v = dropout(v, p.N, p.N // 2 if variant == "dsilu_mask_half_N" else p.N)
        z = p.aux.to(dt)
        s = torch.sigmoid(z)
        v = v * (alpha * s * (1.0 + z * (1.0 - s)))
    elif p.act == ACT_DRELU:
        v = torch.where(p.aux.to(dt) > 0, alpha * v, torch.zeros_like(v))
    if variant == "pre_after_activation" and pre is not None:
        pre = v
    zero_rows = dead[:, None] & (p.mask_mode == 0)
    if p.drop is not None and p.act != ACT_DSILU:
        dropped = dropout(v, n_out, n_out)
        # under mask_mode 0 the two orders are one function (a zero stays zero); a kernel that settles masked rows before the dropout
        # shows on mask_mode 1, whose dead rows carry act(bias)
        v = torch.where(dead[:, None], v, dropped) if variant == "dropout_after_mask" else dropped
    if variant != "mask_after_residual":
        v = torch.where(zero_rows, torch.zeros_like(v), v)
    if p.residual is not None:
        v = (alpha * p.residual.to(dt) if variant == "alpha_on_residual" else p.residual.to(dt)) + (v if variant == "alpha_on_residual" else alpha * v)
    if variant == "mask_after_residual":
        v = torch.where(zero_rows, torch.zeros_like(v), v)
    return SimpleNamespace(out=v, out_c=v.to(p.c_dtype), pre=pre, pre_c=None if pre is None else pre.to(p.pre_dtype), S=S_out, S_pre=S)


# ---------------------------------------------------------------------------------------------------------------- problems
def rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def padded(t, ld):
    """t [M,n] as a view of a [M,ld] buffer whose other columns hold FILL."""
    if ld is None or ld == t.shape[1]:
        return t.contiguous()
    buf = torch.full((t.shape[0], ld), FILL, dtype=t.dtype)
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


EPILOGUES = ("bias", "silu", "relu", "res", "res_inplace", "mask0_res", "mask1", "pre_silu", "dsilu", "drelu", "drop", "drop2", "drop_dsilu", "mask1_drop")
GLU_EPILOGUES = ("glu", "pre_glu", "glu_drop", "glu_mask0")
PLAIN = ("bias", "silu", "relu", "nobias")                      # what ids 7 and 8 take
# (M, N, K): the smallest shapes at which each tile can still go wrong (see tests/test_gemm_matrix_gpu.py)
SHAPE_MAIN, SHAPE_ONE, SHAPE_GLU, SHAPE_KG, SHAPE_PAIR, SHAPE_K64 = (130, 132, 72), (1, 8, 8), (33, 160, 136), (77, 132, 1096), (129, 70, 64), (130, 132, 128)
SHAPE_RAGGED = (150, 160, 136)                                  # B = 3, row_T = 50
ROW_T, ROW_LEN = 50, (50, 17, 0)
CONVS = ((1, 7, 9, 16, 32), (2, 21, 17, 64, 64))              # (B, T1, F1, C, N)
DROP, DROP2 = (0.25, 1234), (0.1, 99)


@functools.lru_cache(maxsize=None)
def problem(shape, wdt="bf16", epi="bias", a32=False, c16=False, pad=False, split=False, conv=None, seed=0):
    """One descriptor on CPU tensors, made once and never written to.  pad: every stride padded (lda = K + 8, ldc = N + 4, ldr = N + 8,
    ld_pre = N + 12, ld_aux = N + 4)."""
    M, N, K = shape
    w_dt = BF16 if split else W_DT[wdt]
    p = SimpleNamespace(M=M, N=N, K=K, W_lo=None, bias=None, residual=None, row_mask=None, mask_mode=0, act=ACT_NONE, alpha=1.0, conv=None,
                        c_dtype=w_dt if c16 else F32, pre_dtype=None, aux=None, drop=None, drop2=None, row_len=None, row_T=0, inplace=False,
                        ldc=None, ld_pre=None, epi=epi, pad=pad)
    s = 1000 * seed + 17 * M + N + K
    if conv is not None:
        B, T1, F1, C, _ = conv
        T2, F2 = (T1 - 3) // 2 + 1, (F1 - 3) // 2 + 1
        assert (M, K) == (B * T2 * F2, 9 * C)
        A = rnd((B, T1, F1, C), s + 1)
        p.conv = (C, T1, F1, T2, F2)
    else:
        A = rnd((M, K), s + 1)
    W = rnd((N, K), s + 2, K ** -0.5)
    if split:
        p.W = W.to(BF16)
        p.W_lo = (W - p.W.float()).to(BF16)
        p.A = A if conv is not None else padded(A, K + 8 if pad else None)
    else:
        p.W = W.to(w_dt)
        A = A if a32 else A.to(w_dt)
        p.A = A if conv is not None else padded(A, K + 8 if pad else None)
    n_out = N // 2 if epi in GLU_EPILOGUES or epi.startswith("row_len") else N
    p.ldc = n_out + 4 if pad else n_out
    if epi != "nobias":
        p.bias = rnd((N,), s + 3, 0.3)
    mask = (torch.rand(M, generator=torch.Generator().manual_seed(s + 4)) > 0.3).to(torch.uint8)
    if M > 2:
        mask[0], mask[M - 1] = 0, 0                 # the first row, and the last row of a ragged tile
    res = lambda: padded(rnd((M, n_out), s + 5), n_out + 8 if pad else None)
    aux_dt = F32 if a32 else w_dt
    if epi in ("silu", "relu"):
        p.act = ACT_SILU if epi == "silu" else ACT_RELU
    elif epi in ("res", "res_inplace"):
        p.residual, p.alpha, p.inplace = res(), 0.5, epi == "res_inplace"
    elif epi == "mask0_res":
        p.residual, p.alpha, p.row_mask = res(), 0.5, mask
    elif epi == "mask0":
        p.row_mask = mask
    elif epi == "mask1":
        p.row_mask, p.mask_mode = mask, 1
    elif epi == "mask0_relu_res":                   # W_lo / conv: activation, residual and a mask in one call
        p.act, p.residual, p.alpha, p.row_mask = ACT_RELU, res(), 0.5, mask
    elif epi == "mask1_silu":
        p.act, p.row_mask, p.mask_mode = ACT_SILU, mask, 1
    elif epi in ("pre_silu", "pre_glu"):
        p.act, p.pre_dtype, p.ld_pre = ACT_SILU if epi == "pre_silu" else ACT_GLU, aux_dt, N + 12 if pad else N
    elif epi in ("dsilu", "drop_dsilu"):
        p.act, p.alpha, p.aux = ACT_DSILU, 0.5, padded(rnd((M, N), s + 6, 2.0).to(aux_dt), N + 4 if pad else None)
        p.drop = DROP if epi == "drop_dsilu" else None
    elif epi == "drelu":
        p.act, p.alpha, p.aux = ACT_DRELU, 0.5, padded(torch.relu(rnd((M, N), s + 6)).to(aux_dt), N + 4 if pad else None)
    elif epi == "drop":
        p.act, p.drop = ACT_SILU, DROP
    elif epi == "mask1_drop":
        p.act, p.drop, p.row_mask, p.mask_mode = ACT_SILU, DROP, mask, 1
    elif epi == "drop2":
        p.drop, p.drop2, p.residual, p.alpha = DROP, DROP2, res(), 0.5
    elif epi == "glu":
        p.act = ACT_GLU
    elif epi == "glu_drop":
        p.act, p.drop = ACT_GLU, DROP
    elif epi == "glu_mask0":
        p.act, p.row_mask, p.residual, p.alpha = ACT_GLU, mask, res(), 0.5
    elif epi in ("row_len", "row_len_mask"):
        assert M == ROW_T * len(ROW_LEN)
        p.act, p.row_len, p.row_T = ACT_GLU, torch.tensor(ROW_LEN, dtype=torch.int32), ROW_T
        if epi == "row_len_mask":
            p.row_mask = mask
            p.row_mask[5] = 0                       # a dead row inside a live utterance, besides the ends
    else:
        assert epi in ("bias", "nobias"), epi
    return p


@functools.lru_cache(maxsize=None)
def poisoned(p_key):
    """the problem with one NaN, one +Inf and one value that overflows an fp16 output in three rows of A; -> (problem, the three rows)."""
    q = SimpleNamespace(**vars(problem(*p_key)))
    rows = (3, q.M - 2, 10)
    A = q.A.clone()
    A[rows[0], 5], A[rows[1], 7], A[rows[2], :] = float("nan"), float("inf"), 60000.0
    q.A = A
    return q, rows


def conv_shape(conv):
    B, T1, F1, C, N = conv
    return (B * ((T1 - 3) // 2 + 1) * ((F1 - 3) // 2 + 1), N, 9 * C)


def ratio(got, ref, S):
    """max over the finite reference elements of |got - ref| / S."""
    ok = torch.isfinite(ref)
    return float(((got.double() - ref).abs()[ok] / S[ok]).max()) if bool(ok.any()) else 0.0


@functools.lru_cache(maxsize=None)
def reference(p_key):
    return evaluate(problem(*p_key))


def yardstick_cases():
    """every (problem key, is_split) the float32-torch yardstick is measured on: the GPU file's cases, K up to 2048."""
    keys = []
    for wdt in ("bf16", "fp16"):
        for a32 in (False, True):
            for e in EPILOGUES:
                keys.append((SHAPE_MAIN, wdt, e, a32))
            for e in GLU_EPILOGUES:
                keys.append((SHAPE_GLU, wdt, e, a32))
            for e in ("row_len", "row_len_mask"):
                keys.append((SHAPE_RAGGED, wdt, e, a32))
            for e in PLAIN:
                keys += [(SHAPE_ONE, wdt, e, a32), (SHAPE_PAIR, wdt, e, a32), (SHAPE_K64, wdt, e, a32)]
        for e in EPILOGUES:
            keys.append((SHAPE_KG, wdt, e))
        keys.append(((64, 64, 2048), wdt, "silu"))
        for cv in CONVS:
            for e in ("silu", "relu", "mask0_relu_res", "mask1_silu"):
                keys.append((conv_shape(cv), wdt, e, False, False, False, False, cv))
    split = []
    for e in ("bias", "silu", "relu", "mask0_relu_res", "mask1_silu"):
        split += [(SHAPE_MAIN, "bf16", e, True, False, False, True), ((64, 64, 2048), "bf16", e, True, False, False, True)]
        for cv in CONVS:
            split.append((conv_shape(cv), "bf16", e, True, False, False, True, cv))
    return keys, split


@functools.lru_cache(maxsize=None)
def measure_g():
    """-> (g, g_split, worst float32-torch ratio, worst float32-torch split ratio): g = 4 x the worst |torch32 - ref| / S over the cases."""
    keys, split = yardstick_cases()
    worst = []
    for ks in (keys, split):
        w = 0.0
        for k in ks:
            p, r = problem(*k), reference(k)
            t = evaluate(p, torch.float32)
            w = max(w, ratio(t.out, r.out, r.S))
            if r.pre is not None:
                w = max(w, ratio(t.pre, r.pre, r.S_pre))
        worst.append(w)
    return 4.0 * worst[0], 4.0 * worst[1], worst[0], worst[1]


# every way the kernel could plausibly be wrong that the audit restates -> the problem whose inputs must show it
VARIANTS = {
    "mask_after_residual": (SHAPE_MAIN, "bf16", "mask0_res"),
    "bias_dropped_on_dead_rows": (SHAPE_MAIN, "bf16", "mask1"),
    "alpha_on_residual": (SHAPE_MAIN, "bf16", "res"),
    "glu_halves_swapped": (SHAPE_GLU, "bf16", "glu"),
    "glu_not_interleaved": (SHAPE_GLU, "bf16", "glu"),
    "glu_gate_wrong_fragment": (SHAPE_GLU, "bf16", "glu"),
    "pre_after_activation": (SHAPE_MAIN, "bf16", "pre_silu"),
    "dropout_after_mask": (SHAPE_MAIN, "bf16", "mask1_drop"),
    "dsilu_mask_half_N": (SHAPE_MAIN, "bf16", "drop_dsilu"),
    "row_len_le": (SHAPE_RAGGED, "bf16", "row_len"),
    "row_len_by_M": (SHAPE_RAGGED, "bf16", "row_len"),
    "conv_taps_ft": (conv_shape(CONVS[0]), "bf16", "relu", False, False, False, False, CONVS[0]),
    "a32_not_rounded": (SHAPE_MAIN, "bf16", "bias", True),
    "relu_drops_nan": "poisoned relu",
}
