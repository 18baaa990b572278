"""cfm_rowchain restated from include/cfm.h (the comment above and inside cfm_rowchain_desc), not from the kernel, on CPU tensors.

`evaluate(p)` runs a Problem in float64 on the 16-bit-rounded weights -- the reference; an intermediate is rounded to the weight type exactly where
the header has a 16-bit operand: xn, the hidden tile, y2 in front of the tail (and out16), the depthwise stage's output, the GLU rows that feed the
depthwise stage under cin_*.  `evaluate(p, torch.float32)` is the SAME formula in plain float32 torch -- the yardstick the bound is measured with
(measure_g); `evaluate(p, variant=...)` is a float64 restatement that is wrong in one named way (VARIANTS), for the audit of
tests/test_rowchain_ref_cpu.py.

Order of operations: (cin_*: r = cin_res + cin_a . Wo^T + cin_b -> cin_out = head_res; GLU(mask(LN(r)) . Wpw1^T + b), zero past glu_len, 16 bit ->
the depthwise stage's input) -> depthwise 15 taps + dw_b, * dw_scale + dw_shift, SiLU, 16 bit, zero padding at utterance edges -> head product + head_b,
head_mask zeroes the product's row, + head_res -> x (no head: x, or x + psum_alpha * (half0 + half1 + psum_b2)) -> xn = LN(x), ln_mask zeroes the
normalised row, 16 bit -> y = x + alpha * (SiLU(xn . W1^T + b1)[16 bit] . W2^T + b2) (psum_out: the two half sums of the second product alone, by
halves of FF) -> y1 = LN1(y) -> out_f32 -> (s2_*: z = y1 + s2_alpha * FFN2(LN(y1; s2_ln)) -> s2_out_f32) -> y2 = LN2(y1 or z), or xn without ln2 ->
out2_f32 (f32), out16 and the tail's input (16 bit) -> t = y2 . Wt^T + tail_b, GLU on (value, gate) pairs of 16-column fragments, rows at or past
glu_len zero -> tail_out.  tail_pair changes which workgroup computes what, not the function.

Bound, per ROW: |out - ref| <= g * max_n |ref[m, .]| (+ one ulp of a 16-bit output at the reference value); g = 4 x the worst such ratio of the float32
yardstick over cases(), separately for f32 and 16-bit outputs of each weight type and for the f32 outputs no rounded intermediate precedes (kind()).
"""
import functools
from types import SimpleNamespace

import torch

from gemm_ref import BF16, F16, F32, W_DT, glu_split, ulp  # noqa: F401  (one definition of the fragment-pair GLU and of an ulp)

RBM = 32                                                     # rows per workgroup tile
DWK, DWH = 15, 7                                             # depthwise taps, halo
FF_OF = {144: 576, 256: 2048, 512: 2048}
TAG = {"bf16": "bf16", "fp16": "f16"}                        # weight type -> the tag in a profiler name
M_PLAIN, M_PAIR = (1, 31, 32, 33, 65), (1, 33, 128, 129)
BT = ((1, 1), (4, 3), (3, 7), (5, 13), (2, 15), (2, 32), (1, 47), (3, 41), (1, 100))
BT_PAIR = BT + ((4, 32), (3, 43))                            # the paired depthwise head: one full group of 8 workgroups, and a second group for one row

INPUTS = ("x", "head_a", "head_w", "head_b", "head_res", "head_mask", "ln_g", "ln_b", "ln_mask", "w1f", "w2n", "b1", "b2", "ln1_g", "ln1_b", "ln2_g", "ln2_b",
          "tail_w", "tail_b", "dw_w", "dw_b", "dw_scale", "dw_shift", "s2_ln_g", "s2_ln_b", "s2_w1f", "s2_w2n", "s2_b1", "s2_b2", "psum_in", "psum_b2",
          "cin_a", "cin_w", "cin_b", "cin_res", "cin_ln_g", "cin_ln_b", "cin_mask", "cin_tail_w", "cin_tail_b", "glu_len")
MATRICES = ("head_w", "w1f", "w2n", "tail_w", "s2_w1f", "s2_w2n", "cin_w", "cin_tail_w")     # natural [N, K] here, fragment-major on the device
OUTPUTS = ("out_f32", "out16", "out2_f32", "tail_out", "s2_out_f32", "psum_out", "cin_out")
OUT16 = ("out16", "tail_out")                                # the 16-bit outputs

# case -> (widths, the profiler name of the instance it must reach, rows): how csrc/encoder.cpp builds each descriptor is in problem() below
INSTANCES = {
    "macaron": ((144, 256, 512), "chain_macaron_%s_d%d", "plain"),                     # macaron_chain
    "convin": ((144, 256, 512), "chain_convin_%s_d%d", "plain"),                       # conv_in_chain without lengths
    "convin_len": ((144, 256, 512), "chain_convin_%s_d%d", "bt"),                      # conv_in_chain on a ragged batch
    "final": ((144, 256, 512), "chain_final_%s_d%d", "plain"),                         # run_chain's last launch behind the depthwise kernel
    "final_after": ((144, 256, 512), "chain_final_%s_d%d", "plain"),                   # ... with the encoder's after-norm
    "qkv": ((144, 256, 512), "chain_qkv_%s_d%d", "plain"),                             # LayerNorm + q|k|v alone
    "rows": ((144, 256, 512), "chain_rows_%s_d%d", "plain"),                           # rows alone
    "dwfinal": ((144, 256), "chain_dwfinal_%s_d%d", "bt"),                             # run_chain's last launch, depthwise stage in the head
    "dwfinal_after": ((144, 256), "chain_dwfinal_%s_d%d", "bt"),
    "dwhead": ((256,), "chain_dwhead_%s_d%d", "bt"),                                   # conv_out, in place
    "dwfinal_macaron": ((256,), "chain_dwfinal_macaron_%s_d%d", "bt"),                 # run_chain_next: final_chain + next_macaron
    "cin": ((256,), "chain_convin_dwfinal_macaron_%s_d%d", "bt"),                      # run_chain_next_cin: cin_out = head_res = s2_out_f32
    "cin_apart": ((256,), "chain_convin_dwfinal_macaron_%s_d%d", "bt"),                # ... with s2_out_f32 a buffer of its own, so that cin_out is seen
    "pair_macaron_half": ((512,), "chain_macaron_half_%s_d%d", "pair"),                # run_pair 1: LN_ffm -> half feed-forwards
    "pair_qkv": ((512,), "chain_qkv_pair_%s_d%d", "pair"),                             # run_pair 2: the reduce, LN_mha, q|k|v over workgroup pairs
    "pair_convin": ((512,), "chain_convin_pair_%s_d%d", "pair"),                       # run_pair 3: conv_in_chain with park
    "pair_convin_len": ((512,), "chain_convin_pair_%s_d%d", "bt"),
    "pair_dwhead": ((512,), "chain_dwhead_pair_%s_d%d", "bt_pair"),                    # run_pair 4: conv_out on park
    "pair_final_half": ((512,), "chain_macaron_half_%s_d%d", "pair"),                  # run_pair 5: LN_ff -> half feed-forwards
    "pair_rows": ((512,), "chain_rows_%s_d%d", "pair"),                                # run_pair 6: the reduce, LN_final, in place on x
    "qkv_unpaired": ((512,), "chain_qkv_%s_d%d", "pair"),                              # run_pair 2 and 3 with tail_pair = 0: the same function
    "convin_unpaired": ((512,), "chain_convin_%s_d%d", "pair"),
}
ROWS = {"plain": tuple((m,) for m in M_PLAIN), "pair": tuple((m,) for m in M_PAIR), "bt": BT, "bt_pair": BT_PAIR}


def instance(case, D, wdt):
    return INSTANCES[case][1] % (TAG[wdt], D)


def instance_names():
    return {fmt % (tag, D) for Ds, fmt, _ in INSTANCES.values() for D in Ds for tag in TAG.values()}


def cases(wdts=("bf16", "fp16")):
    """every (case, D, wdt, rows) of the matrix; rows = (M,) or (B, T)."""
    return [(c, D, w, r) for c, (Ds, _, kind) in INSTANCES.items() for D in Ds for w in wdts for r in ROWS[kind]]


# ---------------------------------------------------------------------------------------------------------------- pieces
def frag_major(w, dtype):
    """[N, K] -> the header's fragment-major order w[((nfrag*KS + kk)*64 + lane)*8 + j] = W[nfrag*16 + (lane&15)][kk*32 + 8*(lane>>4) + j], K zero-padded to 32."""
    N, K = w.shape
    ks = (K + 31) // 32
    wp = torch.zeros((N, ks * 32), dtype=w.dtype)
    wp[:, :K] = w
    return wp.view(N // 16, 16, ks, 4, 8).permute(0, 2, 3, 1, 4).contiguous().to(dtype).view(-1)      # [nfrag, l15, kk, g, j] -> [nfrag, kk, g, l15, j]


def layernorm(x, g, b, eps, variant=None):
    D = x.shape[1]
    d = x - x.mean(1, keepdim=True)
    var = (d * d).sum(1, keepdim=True) / (D - 1 if variant == "unbiased_variance" else D)
    r = 1.0 / (torch.sqrt(var) + eps) if variant == "eps_outside_sqrt" else 1.0 / torch.sqrt(var + eps)
    return d * r * g.to(x.dtype) + b.to(x.dtype)


def glu_dead(p):
    """bool [M]: rows (b, t) with t >= glu_len[b]."""
    m = torch.arange(p.M)
    return (m % p.glu_T) >= p.glu_len.long()[m // p.glu_T]


def depthwise(a, p, dt, variant=None):
    """a [M, D] (rows [B, dw_T] flattened) -> SiLU((conv15(a) + dw_b) * dw_scale + dw_shift), zero padding at utterance edges."""
    M, T = p.M, p.dw_T
    m = torch.arange(M)[:, None]
    k = torch.arange(DWK)[None, :]
    j = m - DWH + k
    tt = (m % T) - DWH + k
    valid = (j >= 0) & (j < M) if variant == "dw_across_utterances" else (tt >= 0) & (tt < T)
    if variant == "cin_halo_shifted":                       # a halo row (one of another tile) taken one row further on
        j = torch.where((j // RBM) != (m // RBM), j + 1, j)
        valid &= (j >= 0) & (j < M)
    taps = a[j.clamp(0, M - 1)] * valid[:, :, None].to(dt)                               # [M, 15, D]
    acc = (taps * p.dw_w.to(dt).t()[None]).sum(1)
    y = (acc + p.dw_b.to(dt)) * p.dw_scale.to(dt) + p.dw_shift.to(dt)
    return y * torch.sigmoid(y)


def glu(pre, variant=None):
    a, g = glu_split(pre)
    if variant == "glu_value_gate_swapped":
        a, g = g, a
    elif variant == "glu_in_halves":
        n = pre.shape[1] // 2
        a, g = pre[:, :n], pre[:, n:]
    return a * torch.sigmoid(g)


# ---------------------------------------------------------------------------------------------------------------- the operation
def evaluate(p, dt=torch.float64, variant=None):
    """-> {output name: [M, n] in dt, before the rounding of a 16-bit output} for every output the descriptor names (psum_out: [2, M, D])."""
    wdt = W_DT[p.wdt]
    r16 = lambda t: t.to(wdt).to(dt)
    c = lambda t: t.to(dt)
    lin = lambda a, w, b: a @ c(w).t() + c(b)
    eps = p.eps
    out = {}
    zero = torch.zeros((), dtype=dt)

    def ffn(xn, w1, b1, w2):
        h = lin(xn, w1, b1)
        return r16(h * torch.sigmoid(h)) @ c(w2).t()

    head_res = None if p.head_res is None else c(p.head_res)
    a = None if p.head_a is None else c(p.head_a)
    if p.cin_a is not None:
        r = c(p.cin_res) + lin(c(p.cin_a), p.cin_w, p.cin_b)
        out["cin_out"] = head_res = r
        cn = layernorm(r, p.cin_ln_g, p.cin_ln_b, eps, variant)
        if p.cin_mask is not None:
            cn = torch.where(p.cin_mask[:, None] != 0, cn, zero)
        a = glu(lin(r16(cn), p.cin_tail_w, p.cin_tail_b), variant)
        if p.glu_len is not None and variant != "dw_reads_past_glu_len":
            a = torch.where(glu_dead(p)[:, None], zero, a)
        a = r16(a)
    if p.head_w is not None:
        if p.dw_w is not None:
            a = r16(depthwise(a, p, dt, variant))
        prod = lin(a, p.head_w, p.head_b)
        if p.head_mask is not None and variant != "head_mask_zeroes_residual":
            prod = torch.where(p.head_mask[:, None] != 0, prod, zero)
        x = head_res + prod
        if p.head_mask is not None and variant == "head_mask_zeroes_residual":
            x = torch.where(p.head_mask[:, None] != 0, x, zero)
    else:
        x = c(p.x)
        if p.psum_in is not None:
            h0, h1, pb, pa = c(p.psum_in[0]), c(p.psum_in[1]), c(p.psum_b2), p.psum_alpha
            if variant == "psum_b2_per_half":
                x = x + pa * ((h0 + pb) + (h1 + pb))
            elif variant == "psum_alpha_on_x":
                x = pa * (x + ((h0 + h1) + pb))
            else:
                x = x + pa * ((h0 + h1) + pb)
    xn = x
    if p.ln_g is not None:
        keep = None if p.ln_mask is None else p.ln_mask[:, None] != 0
        if variant == "ln_mask_before_norm" and keep is not None:
            xn = layernorm(torch.where(keep, x, zero), p.ln_g, p.ln_b, eps)
        else:
            xn = layernorm(x, p.ln_g, p.ln_b, eps, variant)
            if keep is not None:
                xn = torch.where(keep, xn, zero)
    xn32, xn = xn, r16(xn)
    if "psum_out" in p.outputs:
        h = lin(xn, p.w1f, p.b1)
        h = r16(h * torch.sigmoid(h))
        half = p.FF // 2
        w2 = c(p.w2n)
        out["psum_out"] = torch.stack([h[:, :half] @ w2[:, :half].t(), h[:, half:] @ w2[:, half:].t()])
        return out
    y = x
    if p.w1f is not None:
        f = ffn(xn, p.w1f, p.b1, p.w2n)
        if variant == "alpha_on_residual":
            y = p.alpha * (x + (f + c(p.b2)))
        elif variant == "b2_outside_alpha":
            y = x + p.alpha * f + c(p.b2)
        else:
            y = x + p.alpha * (f + c(p.b2))
    y1 = layernorm(y, p.ln1_g, p.ln1_b, eps, variant) if p.ln1_g is not None else y
    if "out_f32" in p.outputs:
        out["out_f32"] = y1
    z = y1
    if p.s2_w1f is not None:
        s2n = r16(layernorm(y1, p.s2_ln_g, p.s2_ln_b, eps, variant))
        z = (y if variant == "s2_residual_from_y" else y1) + p.s2_alpha * (ffn(s2n, p.s2_w1f, p.s2_b1, p.s2_w2n) + c(p.s2_b2))
        out["s2_out_f32"] = z
    if p.ln2_g is not None:
        y2 = layernorm(y if (variant == "ln2_on_y" and p.s2_w1f is None) else z, p.ln2_g, p.ln2_b, eps, variant)
    else:
        y2 = y1 if variant == "tail_from_y1_without_ln2" else xn32
    if "out2_f32" in p.outputs:
        out["out2_f32"] = y2
    if "out16" in p.outputs:
        out["out16"] = y2
    if p.tail_w is not None:
        t = lin(r16(y2), p.tail_w, p.tail_b)
        if p.tail_glu:
            t = glu(t, variant)
            if p.glu_len is not None:
                t = torch.where(glu_dead(p)[:, None], zero, t)
        out["tail_out"] = t
    return out


# ---------------------------------------------------------------------------------------------------------------- problems
def rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def row_mask(M, seed):
    """uint8 [M]: about a quarter zero, the first and the last row among them."""
    m = (torch.rand(M, generator=torch.Generator().manual_seed(seed)) > 0.25).to(torch.uint8)
    m[0], m[M - 1] = 0, 0
    return m


def lengths(B, T):
    """int32 [B]: T, 0, 1, T - 1 and T // 2, as many as B allows."""
    return torch.tensor(([T, 0, 1, T - 1, T // 2] * B)[:B], dtype=torch.int32).clamp_(0, T)


@functools.lru_cache(maxsize=None)
def weights(D, wdt, block=0):
    """one conformer block's row-chain operands at width D: matrices in the weight type (natural [N, K]), the rest float32."""
    dt, FF, s = W_DT[wdt], FF_OF[D], 100000 * block + 7 * D
    mat = lambda n, k, i: rnd((n, k), s + i, k ** -0.5).to(dt)
    lnp = lambda i: (1 + 0.1 * rnd((D,), s + i), 0.1 * rnd((D,), s + i + 1))
    w = SimpleNamespace(FF=FF)
    w.ffm_w1, w.ffm_w2, w.ffm_b1, w.ffm_b2 = mat(FF, D, 1), mat(D, FF, 2), rnd((FF,), s + 3, 0.1), rnd((D,), s + 4, 0.1) + 0.1
    w.ff_w1, w.ff_w2, w.ff_b1, w.ff_b2 = mat(FF, D, 5), mat(D, FF, 6), rnd((FF,), s + 7, 0.1), rnd((D,), s + 8, 0.1) - 0.1
    w.out_w, w.out_b, w.pw2_w, w.pw2_b = mat(D, D, 9), rnd((D,), s + 10, 0.1), mat(D, D, 11), rnd((D,), s + 12, 0.1)
    w.qkv_w, w.qkv_b = mat(3 * D, D, 13), rnd((3 * D,), s + 14, 0.1)
    w.pw1_w, w.pw1_b = mat(2 * D, D, 15), rnd((2 * D,), s + 16, 0.2)           # GLU-interleaved as it stands: fragment 2i = values, 2i + 1 = their gates
    w.dw_w, w.dw_b, w.bn_scale, w.bn_shift = rnd((D, DWK), s + 17, 0.3), rnd((D,), s + 18, 0.1), 1 + 0.2 * rnd((D,), s + 19), 0.1 * rnd((D,), s + 20)
    w.ln_ffm, w.ln_mha, w.ln_conv, w.ln_ff, w.ln_final, w.after = lnp(21), lnp(23), lnp(25), lnp(27), lnp(29), lnp(31)
    return w


@functools.lru_cache(maxsize=None)
def problem(case, D, wdt, rows):
    """One descriptor as csrc/encoder.cpp builds it for `case`, on CPU tensors made once and never written to.  p.<pointer field> holds the operand (matrices
    natural [N, K]), p.outputs the outputs the call names, p.alias {pointer field: the field whose buffer it shares}, p.compare [(buffer, reference output)]."""
    dt = W_DT[wdt]
    M = rows[0] if len(rows) == 1 else rows[0] * rows[1]
    B, T = (1, M) if len(rows) == 1 else rows
    w, nw = weights(D, wdt), weights(D, wdt, 1)
    s = 1000 * sorted(INSTANCES).index(case) + 13 * M + D + B
    p = SimpleNamespace(case=case, M=M, D=D, FF=w.FF, wdt=wdt, B=B, T=T, alpha=1.0, eps=1e-5, tail_N=0, tail_glu=0, dw_T=0, dw_K=0, s2_alpha=0.0, psum_alpha=0.0,
                        tail_pair=0, glu_T=0, outputs=[], alias={}, compare=[], **{n: None for n in INPUTS})

    def stream(i):                                            # the f32 residual stream: off zero mean; row 1 quiet, so that eps tells in its norm
        x = rnd((M, D), s + i, 1.5) + 0.3
        if M > 2:
            x[1] = rnd((D,), s + i + 50, 0.003)
        return x

    act16 = lambda i: rnd((M, D), s + i).to(dt)
    mask = row_mask(M, s + 40)

    def ffn(macaron, ww=w):
        p.alpha = 0.5
        (p.ln_g, p.ln_b), p.w1f, p.w2n, p.b1, p.b2 = (ww.ln_ffm, ww.ffm_w1, ww.ffm_w2, ww.ffm_b1, ww.ffm_b2) if macaron else (ww.ln_ff, ww.ff_w1, ww.ff_w2, ww.ff_b1, ww.ff_b2)

    def qkv_tail(ww=w):
        p.tail_w, p.tail_b, p.tail_N, p.tail_glu = ww.qkv_w, ww.qkv_b, 3 * D, 0
        p.outputs.append("tail_out")
        p.compare.append(("tail_out", "tail_out"))

    def conv_in(park, with_len):
        p.head_a, p.head_w, p.head_b, p.head_res = act16(1), w.out_w, w.out_b, stream(2)
        (p.ln_g, p.ln_b), p.ln_mask = w.ln_conv, mask
        p.tail_w, p.tail_b, p.tail_N, p.tail_glu = w.pw1_w, w.pw1_b, 2 * D, 1
        p.outputs += ["out_f32", "tail_out"]
        p.compare.append(("tail_out", "tail_out"))
        if park:
            p.compare.append(("out_f32", "out_f32"))
        else:
            p.alias["out_f32"] = "head_res"
            p.compare.append(("head_res", "out_f32"))
        if with_len:
            p.glu_len, p.glu_T = lengths(B, T), T

    def pw2_head(dw):
        p.head_a, p.head_w, p.head_b, p.head_res, p.head_mask = act16(3), w.pw2_w, w.pw2_b, stream(4), mask
        if dw:
            p.dw_w, p.dw_b, p.dw_scale, p.dw_shift, p.dw_T, p.dw_K = w.dw_w, w.dw_b, w.bn_scale, w.bn_shift, T, DWK

    def final(dw):
        ffn(False)
        pw2_head(dw)
        p.ln1_g, p.ln1_b = w.ln_final

    def in_place_rows():
        p.outputs.append("out_f32")
        p.alias["out_f32"] = "head_res"
        p.compare.append(("head_res", "out_f32"))

    def next_macaron():
        (p.s2_ln_g, p.s2_ln_b), p.s2_w1f, p.s2_w2n, p.s2_b1, p.s2_b2, p.s2_alpha = nw.ln_ffm, nw.ffm_w1, nw.ffm_w2, nw.ffm_b1, nw.ffm_b2, 0.5
        p.ln2_g, p.ln2_b = nw.ln_mha
        p.outputs.append("s2_out_f32")
        qkv_tail(nw)

    def reduce_rows():
        p.x, p.psum_in, p.psum_b2, p.psum_alpha = stream(5), torch.stack([rnd((M, D), s + 6, 0.5), rnd((M, D), s + 7, 0.5)]), w.ffm_b2, 0.5

    if case == "macaron":
        ffn(True)
        p.x, (p.ln2_g, p.ln2_b) = stream(8), w.ln_mha
        p.outputs += ["out_f32", "out16"]                     # (out16: y2 as the tail reads it -- the encoder leaves it NULL, the header offers it)
        p.compare += [("out_f32", "out_f32"), ("out16", "out16")]
        qkv_tail()
    elif case in ("convin", "convin_len", "convin_unpaired"):
        conv_in(False, case == "convin_len")
    elif case in ("pair_convin", "pair_convin_len"):
        conv_in(True, case == "pair_convin_len")
        p.tail_pair = 1
    elif case in ("final", "final_after", "dwfinal", "dwfinal_after"):
        final(case.startswith("dw"))
        in_place_rows()
        if case.endswith("after"):
            p.ln2_g, p.ln2_b = w.after
            p.outputs.append("out2_f32")
            p.compare.append(("out2_f32", "out2_f32"))
    elif case in ("qkv", "rows"):
        p.x, (p.ln_g, p.ln_b) = stream(9), w.ln_mha
        p.outputs.append("out_f32")
        p.compare.append(("out_f32", "out_f32"))
        if case == "qkv":
            qkv_tail()
    elif case in ("dwhead", "pair_dwhead"):
        pw2_head(True)
        if case == "dwhead":
            in_place_rows()
        else:
            p.tail_pair = 1
            p.outputs.append("out_f32")
            p.compare.append(("out_f32", "out_f32"))
    elif case == "dwfinal_macaron":
        final(True)
        next_macaron()
        p.compare.append(("s2_out_f32", "s2_out_f32"))
    elif case in ("cin", "cin_apart"):
        final(True)
        next_macaron()
        p.head_a, p.head_res = torch.full((M, D), float("nan"), dtype=dt), None     # head_a names the head but is not read; head_res is cin_out
        p.cin_a, p.cin_w, p.cin_b, p.cin_res, (p.cin_ln_g, p.cin_ln_b), p.cin_mask = act16(10), w.out_w, w.out_b, stream(11), w.ln_conv, row_mask(M, s + 41)
        p.cin_tail_w, p.cin_tail_b, p.glu_len, p.glu_T = w.pw1_w, w.pw1_b, lengths(B, T), T
        p.outputs.append("cin_out")
        p.alias["head_res"] = "cin_out"
        if case == "cin":
            p.alias["s2_out_f32"] = "cin_out"                 # the tile's rows: residual in, the next block's residual out
            p.compare.append(("cin_out", "s2_out_f32"))
        else:
            p.compare += [("cin_out", "cin_out"), ("s2_out_f32", "s2_out_f32")]
    elif case in ("pair_macaron_half", "pair_final_half"):
        ffn(case == "pair_macaron_half")
        p.x = stream(12)
        p.outputs.append("psum_out")
        p.compare.append(("psum_out", "psum_out"))
    elif case in ("pair_qkv", "qkv_unpaired"):
        reduce_rows()
        (p.ln_g, p.ln_b), p.tail_pair = w.ln_mha, int(case == "pair_qkv")
        p.outputs.append("out_f32")
        p.compare.append(("out_f32", "out_f32"))
        qkv_tail()
    elif case == "pair_rows":
        reduce_rows()
        p.psum_b2, (p.ln_g, p.ln_b) = w.ff_b2, w.ln_final
        p.outputs.append("out2_f32")
        p.alias["out2_f32"] = "x"
        p.compare.append(("x", "out2_f32"))
    else:
        raise KeyError(case)
    return p


@functools.lru_cache(maxsize=None)
def reference(key):
    return evaluate(problem(*key))


def fill_desc(cfm, p, dev):
    """a cfm.RowChainDesc for problem `p`: pointers from dev {pointer field: device tensor} (absent or None: NULL), sizes and scalars from p."""
    d = cfm.RowChainDesc()
    for name in INPUTS + OUTPUTS:
        t = dev.get(name)
        if t is not None:
            setattr(d, name, t.data_ptr())
    d.M, d.D, d.FF, d.tail_N, d.tail_glu, d.w_dtype = p.M, p.D, p.FF, p.tail_N, p.tail_glu, cfm.BF16 if p.wdt == "bf16" else cfm.F16
    d.alpha, d.eps, d.dw_T, d.dw_K, d.s2_alpha, d.psum_alpha, d.tail_pair, d.glu_T = p.alpha, p.eps, p.dw_T, p.dw_K, p.s2_alpha, p.psum_alpha, p.tail_pair, p.glu_T
    return d


# ---------------------------------------------------------------------------------------------------------------- the bound
def row_scale(ref):
    """max_n |ref[m, .]| per row, as a column."""
    return ref.abs().amax(-1, keepdim=True)


def row_ratio(got, ref, dtype):
    """max over the elements of (|got - ref| - one ulp of a 16-bit output) / max_n |ref[m, .]|; a row whose reference is all zero admits no error at all."""
    err = ((got.double() - ref).abs() - ulp(ref, dtype)).clamp_min(0)
    s = row_scale(ref).expand_as(err)
    r = torch.where(s > 0, err / s.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(r.max())


def out_dtype(p, name):
    return W_DT[p.wdt] if name in OUT16 else F32


def kind(p, name):
    """the class of output `name` that g is measured for: "direct" -- an f32 output with no rounded intermediate in front of it (rows, a reduce, a head product
    on 16-bit inputs + residual, the LayerNorm of such rows): float32 rounding is all that separates the yardstick from the reference; "<wdt>/f32" and
    "<wdt>/16bit" -- outputs behind an intermediate rounded to the weight type, whose rounding the yardstick (and a kernel) now and then takes the other way."""
    if name in OUT16:
        return p.wdt + "/16bit"
    direct = name == "cin_out" or (name in ("out_f32", "out2_f32") and p.w1f is None and p.dw_w is None)
    return "direct" if direct else p.wdt + "/f32"


KINDS = ("direct", "bf16/f32", "bf16/16bit", "fp16/f32", "fp16/16bit")


@functools.lru_cache(maxsize=None)
def measure_g():
    """-> {kind: (g, worst float32-torch ratio)}: g = 4 x the worst per-row ratio of the yardstick over cases() (16-bit outputs: beyond one ulp)."""
    worst = dict.fromkeys(KINDS, 0.0)
    for key in cases():
        p, r = problem(*key), reference(key)
        t = evaluate(p, torch.float32)
        for name, ref in r.items():
            dt = out_dtype(p, name)
            got = t[name].to(dt) if dt != F32 else t[name]
            worst[kind(p, name)] = max(worst[kind(p, name)], row_ratio(got, ref, dt))
    return {k: (4.0 * w, w) for k, w in worst.items()}


# every way the kernel could plausibly be wrong that the audit restates -> the problem whose inputs must show it
VARIANTS = {
    "alpha_on_residual": ("macaron", 144, "bf16", (33,)),
    "b2_outside_alpha": ("macaron", 144, "bf16", (33,)),
    "head_mask_zeroes_residual": ("dwhead", 256, "bf16", (5, 13)),
    "ln_mask_before_norm": ("convin", 144, "bf16", (33,)),
    "tail_from_y1_without_ln2": ("convin", 144, "bf16", (33,)),
    "ln2_on_y": ("final_after", 144, "bf16", (33,)),
    "glu_value_gate_swapped": ("convin", 144, "bf16", (33,)),
    "glu_in_halves": ("convin", 144, "bf16", (33,)),
    "dw_across_utterances": ("dwfinal", 144, "bf16", (5, 13)),
    "dw_reads_past_glu_len": ("cin_apart", 256, "bf16", (5, 13)),
    "psum_b2_per_half": ("pair_rows", 512, "bf16", (33,)),
    "psum_alpha_on_x": ("pair_qkv", 512, "bf16", (33,)),
    "s2_residual_from_y": ("dwfinal_macaron", 256, "bf16", (3, 41)),
    "cin_halo_shifted": ("cin_apart", 256, "bf16", (1, 100)),
    "eps_outside_sqrt": ("macaron", 144, "bf16", (33,)),                # its quiet row 1: variance about eps
    "unbiased_variance": ("pair_rows", 512, "bf16", (33,)),
}
