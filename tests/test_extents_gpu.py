"""GPU: every op pinned to the extents its arguments declare (tests/extent.py).

Each case runs the op ONCE with every pointer operand inside guard bands -- inputs surrounded by NaN (masks by 1), outputs pre-filled with
NaN and surrounded by 0xA5, row strides larger than the rows where the C ABI has a stride -- and asserts
  (a) the output extent matches the reference (and tolerance) the op's existing test uses (tests/test_ops_gpu.py, tests/test_train_ops_gpu.py):
      a NaN that leaked in through a zero weight, or an owned element left unwritten, fails here;
  (b) every band and gap of every operand, inputs included, is byte-identical afterwards.
Shapes: one full tile plus a ragged tail in every tiled dimension, and the degenerate single row."""
import ctypes
import math

import pytest
import torch

from extent import Guards
from test_ops_gpu import W_DT, attn_reference, cfm, relerr, rnd  # noqa: F401  (cfm: the module fixture)

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32


def close(got, ref, tol, what=""):
    """relerr below tol; NaN (unwritten / poisoned) fails because the comparison is written to be False for it"""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    e = relerr(got.float() if got.dtype != torch.float64 else got, ref)
    assert e < tol, "%s: relerr %r (tolerance %g)" % (what, e, tol)


def exact(got, ref, what=""):
    assert got.shape == ref.shape and got.dtype == ref.dtype and torch.equal(got, ref), what


def u8(mask):
    return mask.to(torch.uint8)


# ---------------------------------------------------------------------------------------------------------------- cfm_gemm
GEMM_SHAPES = [(77, 130, 72, 80, 134), (129, 70, 64, 72, 74), (5, 2, 8, 16, 4), (1, 256, 256, 264, 260)]          # M, N, K, lda, ldc


def _gemm_operands(G, M, N, K, lda, dt=BF, a_f32=False):
    a, w, bias = rnd((M, K), 61), rnd((N, K), 62, K ** -0.5).to(dt), rnd((N,), 63, 0.1)
    a = a if a_f32 else a.to(dt)
    return a, w, bias, G.inp(a, ld=lda, name="A"), G.inp(w, name="W"), G.inp(bias, name="bias")


@pytest.mark.parametrize("M,N,K,lda,ldc", GEMM_SHAPES)
@pytest.mark.parametrize("tile", [0, 1, 2, 3, 5, 6])
def test_gemm_plain(cfm, M, N, K, lda, ldc, tile):
    for odt, tol in ((F32, 2e-5), (BF, 1e-2)):
        G = Guards()
        a, w, bias, av, wv, bv = _gemm_operands(G, M, N, K, lda)
        out = G.out((M, N), odt, ld=ldc, name="C")
        cfm.gemm(av, wv, bias=bv, out=out, tile=tile)
        close(out, a.float() @ w.float().t() + bias, tol, "gemm tile %d %s" % (tile, odt))
        G.check()


@pytest.mark.parametrize("tile,M,N,K", [(9, 77, 132, 1096), (10, 77, 132, 1096), (11, 77, 132, 1096), (7, 257, 514, 128), (8, 257, 514, 128)])
def test_gemm_k_group_persistent_and_256_tiles(cfm, tile, M, N, K):
    G = Guards()
    a, w, bias, av, wv, bv = _gemm_operands(G, M, N, K, K + 8)
    out = G.out((M, N), F32, ld=N + 2, name="C")
    cfm.gemm(av, wv, bias=bv, out=out, tile=tile)
    close(out, a.float() @ w.float().t() + bias, 2e-5, "gemm tile %d" % tile)
    G.check()


@pytest.mark.parametrize("variant", ["f32_a", "w_lo", "silu", "relu", "residual", "residual_in_place", "mask_out", "mask_in"])
def test_gemm_epilogues(cfm, variant):
    M, N, K, lda, ldc, ldr = 77, 132, 72, 80, 140, 136
    G = Guards()
    a, w, bias, av, wv, bv = _gemm_operands(G, M, N, K, lda, a_f32=variant in ("f32_a", "w_lo"))
    res = rnd((M, N), 7)
    mask = u8(torch.rand(M, generator=torch.Generator().manual_seed(8)) > 0.3).cuda()
    lin = a.to(BF).float() @ w.float().t()
    if variant == "f32_a":
        out = G.out((M, N), BF, ld=ldc, name="C")
        cfm.gemm(av, wv, bias=bv, out=out)
        close(out, (lin + bias).to(BF).float(), 1e-2, variant)
    elif variant == "w_lo":
        w32 = rnd((N, K), 12, K ** -0.5)
        hi = w32.bfloat16()
        hv, lv = G.inp(hi, name="W_hi"), G.inp((w32 - hi.float()).bfloat16(), name="W_lo")
        out = G.out((M, N), F32, ld=ldc, name="C")
        cfm.gemm(av, hv, bias=bv, w_lo=lv, out=out)
        close(out, a.double() @ w32.double().t() + bias.double(), 4e-5, variant)
    elif variant in ("silu", "relu"):
        out = G.out((M, N), F32, ld=ldc, name="C")
        cfm.gemm(av, wv, bias=bv, out=out, act=cfm.ACT_SILU if variant == "silu" else cfm.ACT_RELU)
        close(out, (torch.nn.functional.silu if variant == "silu" else torch.relu)(lin + bias), 2e-5, variant)
    elif variant == "residual":
        rv, out = G.inp(res, ld=ldr, name="residual"), G.out((M, N), F32, ld=ldc, name="C")
        cfm.gemm(av, wv, bias=bv, residual=rv, alpha=0.5, out=out)
        close(out, res + 0.5 * (lin + bias), 2e-5, variant)
    elif variant == "residual_in_place":
        rv = G.io(res, ld=ldr, name="residual = C")
        cfm.gemm(av, wv, bias=bv, residual=rv, alpha=0.5, out=rv)
        close(rv, res + 0.5 * (lin + bias), 2e-5, variant)
    else:
        mv, rv, out = G.inp(mask, name="row_mask"), G.inp(res, ld=ldr, name="residual"), G.out((M, N), F32, ld=ldc, name="C")
        if variant == "mask_out":
            cfm.gemm(av, wv, bias=bv, residual=rv, alpha=1.0, row_mask=mv, out=out)
            close(out, res + (lin + bias) * mask[:, None].float(), 2e-5, variant)
        else:
            cfm.gemm(av, wv, bias=bv, row_mask=mv, mask_mode=1, out=out)
            close(out, lin * mask[:, None].float() + bias, 2e-5, variant)
    G.check()


def test_gemm_residual_needs_four_column_rows(cfm):
    """why the residual cases run at N = 132: at N = 130 (or an output stride of 134) the entry point refuses, before touching anything."""
    G = Guards()
    a, w, bias, av, wv, bv = _gemm_operands(G, 77, 130, 72, 80)
    rv, out = G.inp(rnd((77, 130), 7), ld=136, name="residual"), G.out((77, 130), F32, ld=136, name="C")
    with pytest.raises(RuntimeError, match="multiples of 4"):
        cfm.gemm(av, wv, bias=bv, residual=rv, alpha=0.5, out=out)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    G.check()


def test_gemm_glu(cfm):
    M, D = 45, 144
    G = Guards()
    a = rnd((M, D), 8).bfloat16()
    w, bias = rnd((2 * D, D), 9, D ** -0.5), rnd((2 * D,), 10, 0.2)
    idx = torch.arange(2 * D, device="cuda")
    src = ((idx % 32) // 16) * D + (idx // 32) * 16 + (idx % 16)
    av, wv, bv = G.inp(a, ld=D + 8, name="A"), G.inp(w[src].bfloat16().contiguous(), name="W"), G.inp(bias[src].contiguous(), name="bias")
    out = G.out((M, D), F32, ld=D + 4, name="C")
    cfm.gemm(av, wv, bias=bv, act=cfm.ACT_GLU, out=out)
    lin = a.float() @ w.bfloat16().float().t() + bias
    close(out, lin[:, :D] * torch.sigmoid(lin[:, D:]), 2e-5, "glu")
    G.check()


def test_gemm_preactivation_and_aux(cfm):
    """C_pre beside C (the forward's SiLU), then aux read by the backward epilogue, all with their own row strides."""
    M, N, K = 77, 136, 72
    G = Guards()
    a, w, bias, av, wv, bv = _gemm_operands(G, M, N, K, 80)
    z = a.float() @ w.float().t() + bias
    pre, h = G.out((M, N), BF, ld=N + 8, name="C_pre"), G.out((M, N), BF, ld=N + 2, name="C")
    cfm.gemm(av, wv, bias=bv, act=cfm.ACT_SILU, out=h, pre_out=pre)
    close(pre, z.to(BF).float(), 1e-2, "C_pre")
    close(h, torch.nn.functional.silu(z), 2e-2, "silu(C)")
    G.check()
    G = Guards()
    dy, w2 = rnd((M, K), 11).to(BF), rnd((N, K), 12, K ** -0.5).to(BF)
    auxv = G.inp(pre.contiguous(), ld=N + 16, name="aux")
    dz = G.out((M, N), F32, ld=N + 4, name="C")
    cfm.gemm(G.inp(dy, ld=K + 8, name="A"), G.inp(w2, name="W"), act=cfm.ACT_DSILU, aux=auxv, alpha=0.5, out=dz)
    zz = pre.float().requires_grad_(True)
    torch.nn.functional.silu(zz).backward(0.5 * (dy.float() @ w2.float().t()))
    close(dz, zz.grad, 1e-4, "dsilu")
    G.check()


def test_gemm_conv3x3s2(cfm):
    B, T1, F1, C, N = 1, 7, 9, 16, 32
    T2, F2 = (T1 - 3) // 2 + 1, (F1 - 3) // 2 + 1
    img = torch.relu(rnd((B, T1, F1, C), 14)).bfloat16()
    w, bias = rnd((N, C, 3, 3), 15, (9 * C) ** -0.5), rnd((N,), 16, 0.1)
    ref = torch.nn.functional.conv2d(img.float().permute(0, 3, 1, 2), w.bfloat16().float(), bias, stride=2)
    ref = torch.relu(ref).permute(0, 2, 3, 1).reshape(B * T2 * F2, N)
    for tile in (0, 1, 2, 3):
        G = Guards()
        out = G.out((B * T2 * F2, N), F32, ld=N + 4, name="C")
        cfm.gemm(G.inp(img, name="image"), G.inp(w.permute(0, 2, 3, 1).reshape(N, 9 * C).bfloat16().contiguous(), name="W"), bias=G.inp(bias, name="bias"),
                 act=cfm.ACT_RELU, conv=(C, T1, F1, T2, F2, B * T2 * F2), tile=tile, out=out)
        close(out, ref, 2e-5, "conv tile %d" % tile)
        G.check()


def test_wrappers_reject_layouts_the_abi_cannot_carry(cfm):
    """cfm_gemm_desc has no row stride for W (and the other ABI structs none for the operands below): a strided view is an argument error raised
    BEFORE any launch, not a silent read with the wrong stride."""
    a, bias = rnd((8, 16), 1).bfloat16(), rnd((8,), 3)
    wbuf = rnd((8, 24), 2).bfloat16()
    cfm.prof_reset(); cfm.prof_enable(True)
    try:
        with pytest.raises(ValueError, match="no row stride for W"):
            cfm.gemm(a, wbuf[:, :16], bias=bias)
        x = rnd((4, 144), 4)
        wide = torch.zeros((4, 160), device="cuda")
        g = torch.ones(144, device="cuda")
        with pytest.raises(ValueError, match="no stride for it"):
            cfm.layernorm(x, torch.ones(288, device="cuda")[::2], g)
        with pytest.raises(ValueError):
            cfm.add_rows(wide[:, :144], x[:1], 4)
        with pytest.raises(ValueError):
            cfm.dwconv_bn_silu(x.view(1, 4, 144), torch.ones((144, 15), device="cuda"), g, g, g, out=wide[:, :144].view(1, 4, 144))
        qkv = rnd((2, 5, 48), 5).bfloat16()
        with pytest.raises(ValueError):
            cfm.attention(qkv, qkv[..., 16:], qkv[..., 32:], 2, 2, 5, 5, 8, (240, 48), (240, 48, 8), (240, 48, 8), torch.empty((2, 5, 32), dtype=BF, device="cuda")[..., :16])
        with pytest.raises(ValueError):
            cfm.rowchain(4, 144, cfm.BF16, x=wide[:, :144], out_f32=x)
        with pytest.raises(ValueError):
            cfm.ffn_fused(x, g, g, g, g, 64, out_f32=wide[:, :144])
        with pytest.raises(ValueError):
            cfm.conv_cache_update(x.view(1, 4, 144), torch.zeros((1, 14, 160), device="cuda")[..., :144], 15)
        with pytest.raises(ValueError):
            cfm.gemm_tn_group([dict(a=a, b=a, out=torch.zeros((16, 32), device="cuda")[:, ::2])])
        nostride = "no stride for it"
        wide16 = torch.zeros((10, 48), dtype=BF, device="cuda")
        st = (5 * 48, 48)
        with pytest.raises(ValueError, match=nostride):            # attention_bwd: out / dout / lse are dense by contract
            cfm.attention_bwd(qkv, qkv[..., 16:], qkv[..., 32:], wide16[:, :16], wide16[:, 16:32], torch.zeros((2, 2, 5), device="cuda"), 2, 2, 5, 5, 8, st, st, st,
                              wide16, wide16[:, 16:], wide16[:, 32:])
        ctx16 = torch.zeros((10, 16), dtype=BF, device="cuda")
        with pytest.raises(ValueError, match="passes"):            # ... and a gradient shares ITS operand's strides: a dense dq beside a fused qkv does not
            cfm.attention_bwd(qkv, qkv[..., 16:], qkv[..., 32:], ctx16, ctx16, torch.zeros((2, 2, 5), device="cuda"), 2, 2, 5, 5, 8, st, st, st,
                              torch.zeros((10, 16), dtype=BF, device="cuda"), wide16[:, 16:], wide16[:, 32:])
        with pytest.raises(ValueError, match="passes"):
            cfm.kv_cache_pack(None, qkv[..., 16:], qkv[..., 32:], (5 * 32, 32), (5 * 32, 32), 2, 2, 5, 8)
        x256 = rnd((4, 256), 6)
        wide256 = torch.zeros((4, 272), device="cuda")
        with pytest.raises(ValueError, match=nostride):
            cfm.ffn_split(x256, cfm.BF16, 0, rows_out=wide256[:, :256])
        offs = torch.zeros(6, dtype=torch.int32, device="cuda")[::2]
        with pytest.raises(ValueError, match=nostride):
            cfm.stream_prep(offs, 4, 6, 10, rnd((64, 16), 7), torch.zeros((3, 10), dtype=torch.uint8, device="cuda"), torch.zeros((3, 10, 16), device="cuda"))
        with pytest.raises(ValueError, match=nostride):
            cfm.stream_advance(offs, 4)
        taps = torch.ones((144, 30), device="cuda")[:, ::2]
        with pytest.raises(ValueError, match=nostride):
            cfm.dwconv_causal_bn_silu(x.view(1, 4, 144), taps, g, g, g)
        with pytest.raises(ValueError, match=nostride):
            cfm.dwconv_bn_train(x.view(1, 4, 144), taps, g, g, g, g.clone(), g.clone(), 0.1, 1e-5, F32)
        with pytest.raises(ValueError, match=nostride):
            cfm.dwconv_bn_train_bwd(x.view(1, 4, 144), x.view(1, 4, 144), torch.zeros((4, 288), device="cuda")[:, ::2], x.view(1, 4, 144), taps.contiguous(), F32)
        w9 = rnd((16, 9), 8)
        img = rnd((1, 7, 7), 9)
        with pytest.raises(ValueError, match=nostride):            # the [C,9] weight transposed WITHOUT .contiguous(): tap-major in shape only
            cfm.conv1_relu(img, w9.t(), rnd((16,), 10), F32)
        with pytest.raises(ValueError, match=nostride):
            cfm.conv12_relu(rnd((1, 16, 16), 11), rnd((64, 9), 12).t(), rnd((64,), 13), torch.zeros((64, 576), dtype=BF, device="cuda"), rnd((64,), 14))
        with pytest.raises(ValueError, match=nostride):
            cfm.conv1_wgrad(rnd((1, 3, 3, 16), 15), img, cmvn=(rnd((14,), 16)[::2], None))
        with pytest.raises(ValueError, match=nostride):
            cfm.layernorm_bwd(x, x, torch.ones(288, device="cuda")[::2])
        with pytest.raises(ValueError, match=nostride):
            cfm.dropout_rows(x, F32, row_mask=torch.ones(8, dtype=torch.uint8, device="cuda")[::2])
        g2 = torch.ones(288, device="cuda")[::2]                     # a strided LayerNorm gain, as layernorm() refuses above
        with pytest.raises(ValueError, match=nostride):
            cfm.rowchain(4, 144, cfm.BF16, x=x, ln=(g2, g), out_f32=x.clone())
        with pytest.raises(ValueError, match=nostride):
            cfm.rowchain(4, 144, cfm.BF16, x=x, ln=(g, g), ln2=(g, g2), out_f32=x.clone())
        g256 = torch.ones(512, device="cuda")[::2]
        with pytest.raises(ValueError, match=nostride):
            cfm.ffn_split(x256, cfm.BF16, 0, ln1=(g256, g256), rows_out=torch.empty_like(x256))
        with pytest.raises(ValueError, match=nostride):
            cfm.ffn_split(x256, cfm.BF16, 1, ring=(torch.zeros((1, 4, 40, 256), device="cuda")[..., ::2], torch.zeros(1, dtype=torch.int32, device="cuda"), 4))
        lg, i3 = rnd((1, 3, 8), 17), torch.ones((1, 2), dtype=torch.int32, device="cuda")
        i1 = torch.ones(1, dtype=torch.int32, device="cuda")
        f = lambda *sh: torch.zeros(sh, device="cuda")
        with pytest.raises(ValueError, match=nostride):
            cfm.ctc_grad(lg, 8, 3 * i1, i3, i1, (f(1, 3, 6), f(1, 3, 12)[..., ::2], f(1, 3), f(1), f(1, 3, 6)))
        with pytest.raises(ValueError, match=nostride):
            cfm.gemm_tn_group([dict(a=a, b=a, out=f(16 * 16), row_off=torch.zeros(32, dtype=torch.int64, device="cuda")[::2])])
        with pytest.raises(ValueError, match="passes"):            # forward attention: q's own time stride is 48, the call says 32
            cfm.attention(qkv, qkv[..., 16:], qkv[..., 32:], 2, 2, 5, 5, 8, (160, 32), (240, 48, 8), (240, 48, 8), torch.empty((2, 5, 16), dtype=BF, device="cuda"))
        torch.cuda.synchronize()
    finally:
        cfm.prof_enable(False)
    assert cfm.prof_table() == {}, "a rejected call launched something"
    cfm.prof_reset()


# ---------------------------------------------------------------------------------------------------------------- cfm_gemm_tn
@pytest.mark.parametrize("M,N,K", [(130, 136, 72), (1, 8, 8)])
@pytest.mark.parametrize("variant", ["colsum_mask", "accumulate", "split"])
def test_gemm_tn(cfm, M, N, K, variant):
    G = Guards()
    split = variant == "split"
    a, b = rnd((M, N), 1), rnd((M, K), 2)
    a_in, b_in = (a, b) if split else (a.to(BF), b.to(BF))
    av, bv = G.inp(a_in, ld=N + 8, name="A"), G.inp(b_in, ld=K + 16, name="B")
    ar, br = a_in.double(), b_in.double()
    if variant == "colsum_mask":
        mask = (torch.rand(M, generator=torch.Generator().manual_seed(3)) > 0.2).cuda()
        out, cs = G.out((N, K), F32, ld=K + 4, name="C"), G.out((N,), F32, name="colsum")
        cfm.gemm_tn(av, bv, out=out, colsum=cs, row_mask=G.inp(u8(mask), name="row_mask"), alpha=0.5)
        close(out, 0.5 * (ar * mask[:, None]).t() @ br, 1e-4, "C")
        close(cs, 0.5 * (ar * mask[:, None]).sum(0), 1e-4, "colsum")
    elif variant == "accumulate":
        prior, pcs = rnd((N, K), 4), rnd((N,), 5)
        out, cs = G.io(prior, ld=K + 4, name="C"), G.io(pcs, name="colsum")
        cfm.gemm_tn(av, bv, out=out, colsum=cs, alpha=0.5, accumulate=True, splits=1)
        close(out, prior.double() + 0.5 * ar.t() @ br, 1e-4, "C")
        close(cs, pcs.double() + 0.5 * ar.sum(0), 1e-4, "colsum")
    else:
        out, cs = G.out((N, K), F32, ld=K + 4, name="C"), G.out((N,), F32, name="colsum")
        cfm.gemm_tn(av, bv, out=out, colsum=cs, split=True)
        close(out, ar.t() @ br, 3e-5, "C")
        close(cs, ar.sum(0), 1e-5, "colsum")
    G.check()


def test_gemm_tn_conv(cfm):
    B, T1, F1, C = 3, 9, 7, 16
    T2, F2 = (T1 - 3) // 2 + 1, (F1 - 3) // 2 + 1
    img, dy = rnd((B, T1, F1, C), 6).to(BF), rnd((B * T2 * F2, C), 7).to(BF)
    w = torch.zeros((C, C, 3, 3), dtype=torch.float64, device="cuda", requires_grad=True)
    torch.nn.functional.conv2d(img.double().permute(0, 3, 1, 2), w, stride=2).backward(dy.double().view(B, T2, F2, C).permute(0, 3, 1, 2))
    G = Guards()
    out = G.out((C, 9 * C), F32, ld=9 * C + 4, name="C")
    cfm.gemm_tn(G.inp(dy, ld=C + 8, name="A"), G.inp(img, name="image"), out=out, conv=(C, T1, F1, T2, F2))
    close(out, w.grad.permute(0, 2, 3, 1).reshape(C, 9 * C), 1e-4, "conv wgrad")
    G.check()


def test_gemm_tn_group_and_row_off_scatter(cfm):
    M, D = 257, 64
    G = Guards()
    prods, refs = [], []
    for i, (N, K) in enumerate([(D, 2 * D), (2 * D, D), (D, D)]):
        a, b = rnd((M, N), 100 + i).to(BF), rnd((M, K), 200 + i).to(BF)
        prior = rnd((N, K), 300 + i)
        prods.append(dict(a=G.inp(a, ld=N + 8, name="A%d" % i), b=G.inp(b, ld=K + 8, name="B%d" % i), out=G.io(prior, ld=K + 4, name="C%d" % i),
                          colsum=G.io(torch.zeros(N), name="colsum%d" % i), alpha=0.5 if i == 0 else 1.0))
        refs.append((prior.double() + prods[-1]["alpha"] * a.double().t() @ b.double(), prods[-1]["alpha"] * a.double().sum(0)))
    # a fused 3D x D product scattered by rows into a guarded flat slab (zero-filled: accumulate), the column sums too, the first D twice
    a, b = rnd((M, 3 * D), 110).to(BF), rnd((M, D), 210).to(BF)
    n_slab = 3 * D * D + 4 * D + 64
    slab = G.io(torch.zeros(n_slab), name="slab")
    ar = torch.arange(D, device="cuda")
    w_off, b_off, u_off = (2 * D * D + 16, 16, D * D + 16), (3 * D * D + 32 + D, 3 * D * D + 16, 3 * D * D + 48 + 2 * D), 3 * D * D + 48 + 3 * D
    tabs = [G.inp(torch.cat([w_off[j] + ar * D for j in range(3)]), name="row_off"), G.inp(torch.cat([b_off[j] + ar for j in range(3)]), name="colsum_off"),
            G.inp(torch.cat([u_off + ar, torch.full((2 * D,), -1, device="cuda", dtype=torch.int64)]), name="colsum_off2")]
    prods.append(dict(a=G.inp(a, ld=3 * D + 8, name="A_qkv"), b=G.inp(b, ld=D + 8, name="B_qkv"), out=slab, colsum=slab, row_off=tabs[0], colsum_off=tabs[1],
                      colsum_off2=tabs[2]))
    cfm.gemm_tn_group(prods)
    for i, (rw, rb) in enumerate(refs):
        close(prods[i]["out"], rw, 1e-4, "C%d" % i)
        close(prods[i]["colsum"], rb, 1e-4, "colsum%d" % i)
    rw, rb = a.double().t() @ b.double(), a.double().sum(0)
    want = torch.zeros(n_slab, dtype=torch.float64, device="cuda")
    for j in range(3):
        want[w_off[j]:w_off[j] + D * D] = rw[j * D:(j + 1) * D].reshape(-1)
        want[b_off[j]:b_off[j] + D] = rb[j * D:(j + 1) * D]
    want[u_off:u_off + D] = rb[:D]
    close(slab, want, 1e-4, "slab")
    assert bool((slab[want == 0] == 0).all()), "the scatter wrote between the parameters of the slab"
    G.check()


# ---------------------------------------------------------------------------------------------------------------- LayerNorm
LN_SHAPES = [(5, 512), (98, 144), (3, 1024), (1, 16)]


@pytest.mark.parametrize("M,D", LN_SHAPES)
def test_layernorm(cfm, M, D):
    G = Guards()
    x = rnd((M, D), 20, 2.0) + 0.5
    g1, b1, g2, b2 = 1 + 0.1 * rnd((D,), 21), 0.1 * rnd((D,), 22), 1 + 0.1 * rnd((D,), 23), 0.1 * rnd((D,), 24)
    mask = u8(torch.rand(M, generator=torch.Generator().manual_seed(25)) > 0.3).cuda()
    y1, y2 = G.out((M, D), F32, name="out1"), G.out((M, D), BF, name="out2")
    cfm.layernorm(G.inp(x, name="x"), G.inp(g1, name="g1"), G.inp(b1, name="b1"), out1=y1, g2=G.inp(g2, name="g2"), b2=G.inp(b2, name="b2"), out2=y2,
                  row_mask=G.inp(mask, name="row_mask"))
    ref1 = torch.nn.functional.layer_norm(x, (D,), g1, b1, 1e-5)
    ref2 = torch.nn.functional.layer_norm(ref1, (D,), g2, b2, 1e-5)
    close(y1, ref1, 2e-6, "out1")
    close(y2, (ref2 * mask[:, None]).bfloat16().float(), 1e-2, "out2")
    G.check()


@pytest.mark.parametrize("M,D", LN_SHAPES)
@pytest.mark.parametrize("dyt", [F32, BF])
def test_layernorm_bwd(cfm, M, D, dyt):
    x, dy = rnd((M, D), 17), rnd((M, D), 18).to(dyt)
    g, b, dres = 1 + rnd((D,), 19, 0.1), rnd((D,), 20, 0.1), rnd((M, D), 21)
    mask = (torch.rand(M, generator=torch.Generator().manual_seed(22)) > 0.3).cuda()
    xr, gr, br = x.double().requires_grad_(True), g.double().requires_grad_(True), b.double().requires_grad_(True)
    (torch.nn.functional.layer_norm(xr, (D,), gr, br, 1e-5) * mask[:, None]).backward(dy.double())
    L = cfm.lib()
    for in_place in (False, True):
        G = Guards()
        xv, dyv, gv, mv = G.inp(x, name="x"), G.inp(dy, name="dy"), G.inp(g, name="gamma"), G.inp(u8(mask), name="row_mask")
        drv = G.io(dres, name="dres = dx") if in_place else G.inp(dres, name="dres")
        dx = drv if in_place else G.out((M, D), F32, name="dx")
        dg, db, ws = G.out((D,), F32, name="dgamma"), G.out((D,), F32, name="dbeta"), G.ws(L.cfm_layernorm_bwd_ws(M, D), name="ws")
        d = cfm.LnBwdDesc()                 # the plain (non-accumulating, no-dx2) descriptor: every other field zero
        d.x, d.dy, d.gamma, d.row_mask, d.dres = xv.data_ptr(), dyv.data_ptr(), gv.data_ptr(), mv.data_ptr(), drv.data_ptr()
        d.dx, d.dgamma, d.dbeta, d.ws = dx.data_ptr(), dg.data_ptr(), db.data_ptr(), ws.data_ptr()
        d.M, d.D, d.dy_dtype, d.eps = M, D, cfm.dt_code(dy), 1e-5
        cfm.check(L.cfm_layernorm_bwd_fused(ctypes.byref(d), cfm.stream()), "cfm_layernorm_bwd_fused")
        close(dx, xr.grad + dres.double(), 2e-5, "dx")
        close(dg, gr.grad, 2e-5, "dgamma")
        close(db, br.grad, 2e-5, "dbeta")
        G.check()


@pytest.mark.parametrize("M,D", LN_SHAPES)
@pytest.mark.parametrize("variant", ["overwrite", "accumulate", "chain"])
def test_layernorm_bwd_fused(cfm, M, D, variant):
    """cfm_layernorm_bwd_fused with EVERY pointer of its descriptor placed, against what tests/test_train_ops_gpu.py compares it with: the plain (non-accumulating, no-dx2) descriptor for dx and
    the parameter sums (identical through the workspace; 1e-5 on top of a running sum with atomics), cfm_dropout_rows on dx for the 16-bit second output.
    chain: dx = dLN(dres + dLN(dy; x, gamma); chain_x, chain_gamma) against the two plain calls it folds, at that op's own 2e-5."""
    acc, chain = int(variant != "overwrite"), variant == "chain"
    x, dy, dres, gamma = rnd((M, D), 17), rnd((M, D), 18), rnd((M, D), 21), 1 + rnd((D,), 19, 0.1)
    mask = u8(torch.rand(M, generator=torch.Generator().manual_seed(22)) > 0.3).cuda()
    mask2 = u8(torch.rand(M, generator=torch.Generator().manual_seed(23)) > 0.3).cuda()
    cx, cgamma = rnd((M, D), 24), 1 + rnd((D,), 25, 0.1)
    dx_ref, dg_ref, db_ref = cfm.layernorm_bwd(x, dy, gamma, row_mask=mask, dres=dres)              # row_mask belongs to the FIRST norm, chained or not
    if chain:
        dx_ref, cdg_ref, cdb_ref = cfm.layernorm_bwd(cx, dx_ref, cgamma)
    y_ref = cfm.dropout_rows(dx_ref, BF, alpha=0.5, drop=(0.1, 77), drop2=(0.2, 78), row_mask=mask2)
    L = cfm.lib()
    G = Guards()
    base = [rnd((D,), 26 + i) for i in range(4)]
    d = cfm.LnBwdDesc()
    dx, dx2 = G.out((M, D), F32, name="dx"), G.out((M, D), BF, name="dx2")
    dg, db = (G.io(base[0], name="dgamma"), G.io(base[1], name="dbeta")) if acc else (G.out((D,), F32, name="dgamma"), G.out((D,), F32, name="dbeta"))
    d.x, d.dy, d.gamma, d.dres = (G.inp(t, name=n).data_ptr() for t, n in ((x, "x"), (dy, "dy"), (gamma, "gamma"), (dres, "dres")))
    d.row_mask = G.inp(mask, name="row_mask").data_ptr()
    d.dx2_row_mask = G.inp(mask2, name="dx2_row_mask").data_ptr()
    d.dx, d.dgamma, d.dbeta, d.dx2, d.ws = dx.data_ptr(), dg.data_ptr(), db.data_ptr(), dx2.data_ptr(), G.ws(L.cfm_layernorm_bwd_ws(M, D), name="ws").data_ptr()
    if chain:
        cdg, cdb = G.io(base[2], name="chain_dgamma"), G.io(base[3], name="chain_dbeta")
        d.chain_x, d.chain_gamma, d.chain_dgamma, d.chain_dbeta = G.inp(cx, name="chain_x").data_ptr(), G.inp(cgamma, name="chain_gamma").data_ptr(), cdg.data_ptr(), cdb.data_ptr()
    d.M, d.D, d.dy_dtype, d.dx2_dtype, d.accumulate = M, D, cfm.F32, cfm.BF16, acc
    d.eps, d.alpha2, d.p1, d.p2, d.seed1, d.seed2 = 1e-5, 0.5, 0.1, 0.2, 77, 78
    cfm.check(L.cfm_layernorm_bwd_fused(ctypes.byref(d), cfm.stream()), "cfm_layernorm_bwd_fused")
    torch.cuda.synchronize()
    near = lambda got, b, ref: float((got - b - ref).abs().max()) < 1e-5 * float(ref.abs().max()) + 1e-5
    if chain:
        close(dx, dx_ref, 2e-5, "dx")
        close(dx2, y_ref.float(), 1e-2, "dx2")                      # bf16 of a dx that may differ in its last f32 bits: the project's bf16 rounding bound
        assert near(cdg, base[2], cdg_ref) and near(cdb, base[3], cdb_ref)
        assert near(dg, base[0], dg_ref) and near(db, base[1], db_ref)
    else:
        exact(dx, dx_ref, "dx")
        exact(dx2.contiguous().view(torch.int16), y_ref.view(torch.int16), "dx2")
        if acc:
            assert near(dg, base[0], dg_ref) and near(db, base[1], db_ref)
        else:
            exact(dg, dg_ref, "dgamma")
            exact(db, db_ref, "dbeta")
    G.check()


# ---------------------------------------------------------------------------------------------------------------- attention
@pytest.mark.parametrize("B,H,Tq,Tk,dk", [(3, 8, 70, 130, 64), (2, 2, 5, 5, 8), (1, 4, 16, 80, 36)])
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("pos", ["none", "broadcast", "perkey"])
@pytest.mark.parametrize("masking", ["none", "pad", "full"])
def test_attention(cfm, B, H, Tq, Tk, dk, mode, pos, masking):
    """q / k / v are slices of one fused [B, T, 3D + pad] buffer: the gaps of each are the other two operands plus NaN padding."""
    D, pad = H * dk, 16
    ld = 3 * D + pad
    dt = {"bf16": BF, "fp32": F32}[mode]
    G = Guards()
    qkv = rnd((B, Tq, 3 * D), 30).to(dt)
    kv_src = qkv if Tk == Tq else rnd((B, Tk, 3 * D), 31).to(dt)
    qv = G.inp(qkv, ld=ld, name="qkv")
    kvv = qv if Tk == Tq else G.inp(kv_src, ld=ld, name="kv")
    u, vb = rnd((H, dk), 32, 0.3), rnd((H, dk), 33, 0.3)
    P = {"none": 0, "broadcast": 1, "perkey": Tk}[pos]
    p = rnd((B, P, D), 34).to(dt) if P else None
    pv = G.inp(p, ld=D + 8, name="p") if P else None
    mask, mv, mstr = None, None, (0, 0)
    if masking == "pad":
        lens = torch.randint(1, Tk + 1, (B,), generator=torch.Generator().manual_seed(35))
        lens[0] = Tk
        mask = (torch.arange(Tk)[None, :] < lens[:, None]).unsqueeze(1).cuda()
        mv = G.inp(u8(mask), ld=Tk + 3, name="mask")                         # (B,1,Tk): m_sb = row stride, m_sq = 0
        mstr = (Tk + 3, 0)
    elif masking == "full":
        mask = (torch.rand(B, Tq, Tk, generator=torch.Generator().manual_seed(36)) > 0.4).cuda()
        mask[:, min(3, Tq - 1), :] = False
        mv = G.inp(u8(mask), ld=Tk + 5, name="mask")                         # m_sq = Tk + 5 > Tk
        mstr = (Tq * (Tk + 5), Tk + 5)
    out = G.out((B, Tq, D), dt, name="out")
    want_lse = (pos != "perkey")
    lse = G.out((B, H, Tq), F32, name="lse") if want_lse else None
    cfm.attention(qv, kvv[..., D:], kvv[..., 2 * D:], B, H, Tq, Tk, dk, (Tq * ld, ld), (Tk * ld, ld, dk), (Tk * ld, ld, dk), out,
                  p=pv, p_str=(P * (D + 8), (D + 8) if P > 1 else 0), bias_u=G.inp(u, name="bias_u") if P else None, bias_v=G.inp(vb, name="bias_v") if P else None,
                  mask=mv, mask_str=mstr, mma_code=cfm.BF16, split=mode == "fp32", lse=lse)
    ref = attn_reference(qkv[..., :D].reshape(B, Tq, H, dk).double(), kv_src[..., D:2 * D].reshape(B, Tk, H, dk).double(),
                         kv_src[..., 2 * D:].reshape(B, Tk, H, dk).double(), p.double().reshape(B, P, H, dk) if P else None, u.double(), vb.double(), mask,
                         1 / math.sqrt(dk))
    close(out, ref, {"bf16": 2e-2, "fp32": 2e-4}[mode], "out")
    if masking == "full":
        assert float(out[:, min(3, Tq - 1)].float().abs().max()) == 0.0
    if want_lse:
        # no existing test owns a bound for lse: the scores it sums are the ones `out` is built from, so it is held to the same mode tolerance as `out`
        qh, kh = qkv[..., :D].reshape(B, Tq, H, dk).double().permute(0, 2, 1, 3), kv_src[..., D:2 * D].reshape(B, Tk, H, dk).double().permute(0, 2, 1, 3)
        sc = torch.einsum("bhid,bhjd->bhij", qh + (u.double()[None, :, None, :] if P else 0), kh)
        if P:
            sc = sc + torch.einsum("bhid,bhjd->bhij", qh + vb.double()[None, :, None, :], p.double().reshape(B, P, H, dk).permute(0, 2, 1, 3))
        sc = sc / math.sqrt(dk)
        if mask is not None:
            sc = sc.masked_fill(mask.unsqueeze(1) == 0, float("-inf"))
        lse_ref = torch.logsumexp(sc, -1)
        dead = torch.isinf(lse_ref)
        assert not bool(torch.isnan(lse).any()), "lse: an owned element was not written"
        assert torch.equal(torch.isinf(lse) & (lse < 0), dead), "lse: -inf exactly on the fully masked rows"
        close(lse.double().masked_fill(dead, 0.0), lse_ref.masked_fill(dead, 0.0), {"bf16": 2e-2, "fp32": 2e-4}[mode], "lse")
        if masking == "full":
            assert bool(dead[:, :, min(3, Tq - 1)].all())
    G.check()


def test_kv_cache_pack(cfm):
    B, H, Tn, dk = 1, 4, 5, 36
    D = H * dk
    ld = 3 * D + 8
    for Tc in (0, 3):
        G = Guards()
        qkv = rnd((B, Tn, 3 * D), 40).bfloat16()
        cache = rnd((B, H, Tc, 2 * dk), 41)
        qv = G.inp(qkv, ld=ld, name="qkv")
        cv = G.inp(cache, name="old_cache") if Tc else None
        new = G.out((B, H, Tc + Tn, 2 * dk), F32, name="new_cache")
        cfm.check(cfm.lib().cfm_kv_cache_pack(cfm.ptr(cv), Tc, qv[..., D:].data_ptr(), qv[..., 2 * D:].data_ptr(), cfm.BF16, Tn * ld, ld, Tn * ld, ld, new.data_ptr(),
                                              B, H, Tn, dk, cfm.stream()), "cfm_kv_cache_pack")
        k_new = qkv[..., D:2 * D].float().reshape(B, Tn, H, dk).permute(0, 2, 1, 3)
        v_new = qkv[..., 2 * D:].float().reshape(B, Tn, H, dk).permute(0, 2, 1, 3)
        exact(new, torch.cat([torch.cat([cache[..., :dk], k_new], 2), torch.cat([cache[..., dk:], v_new], 2)], -1), "kv_cache_pack Tc=%d" % Tc)
        G.check()


# ---------------------------------------------------------------------------------------------------------------- depthwise conv, front end
def _dw_params(G, D, K):
    w, db, sc, sh = rnd((D, K), 51, 0.3), rnd((D,), 52, 0.1), 1 + 0.2 * rnd((D,), 53), rnd((D,), 54, 0.1)
    return (w, db, sc, sh), (G.inp(w, name="taps"), G.inp(db, name="dw_bias"), G.inp(sc, name="bn_scale"), G.inp(sh, name="bn_shift"))


@pytest.mark.parametrize("B,T,D,K", [(2, 5, 16, 15), (3, 37, 144, 15), (2, 40, 32, 7)])
@pytest.mark.parametrize("dt", [BF, torch.float16, F32])
def test_dwconv_bn_silu(cfm, B, T, D, K, dt):
    G = Guards()
    x = rnd((B, T, D), 50).to(dt)
    (w, db, sc, sh), pv = _dw_params(G, D, K)
    y = G.out((B, T, D), dt, name="y")
    cfm.dwconv_bn_silu(G.inp(x, name="x"), *pv, out=y)
    ref = torch.nn.functional.conv1d(x.float().transpose(1, 2), w[:, None, :], db, padding=(K - 1) // 2, groups=D)
    ref = torch.nn.functional.silu(ref * sc[None, :, None] + sh[None, :, None]).transpose(1, 2)
    close(y, ref, {BF: 1e-2, torch.float16: 2e-3, F32: 1e-5}[dt], "dwconv")
    G.check()


FRONT = [(1, 7, 16, 7), (3, 83, 256, 83), (2, 200, 144, 80)]            # B, T, C, F


@pytest.mark.parametrize("B,T,C,F", FRONT)
@pytest.mark.parametrize("mma", [False, True])
def test_conv1_relu(cfm, B, T, C, F, mma):
    x, w, b = rnd((B, T, F), 60), rnd((C, 1, 3, 3), 61, 1 / 3), rnd((C,), 62, 0.1)
    mean, istd = rnd((F,), 63, 0.5), (1.0 + 0.2 * rnd((F,), 64)).abs() + 0.5
    T1, F1 = (T - 3) // 2 + 1, (F - 3) // 2 + 1
    L = cfm.lib()
    for odt, cmvn in ((BF, False), (BF, True)) if mma else ((F32, False), (BF, False)):
        G = Guards()
        xv, wv, bv = G.inp(x, name="x"), G.inp(w.reshape(C, 9).t().contiguous(), name="w9c"), G.inp(b, name="bias")
        mv, iv = (G.inp(mean, name="cmvn_mean"), G.inp(istd, name="cmvn_istd")) if cmvn else (None, None)
        y = G.out((B, T1, F1, C), odt, name="y")
        fn = L.cfm_conv1_relu_mma if mma else L.cfm_conv1_relu
        cfm.check(fn(xv.data_ptr(), wv.data_ptr(), bv.data_ptr(), y.data_ptr(), cfm.dt_code(odt), B, T, F, C, cfm.ptr(mv), cfm.ptr(iv), cfm.stream()), "cfm_conv1_relu")
        if mma:
            xn = (((x - mean) * istd) if cmvn else x).to(BF).double()
            ref = torch.relu(torch.nn.functional.conv2d(xn[:, None], w.to(BF).double(), b.double(), stride=2)).permute(0, 2, 3, 1)
            close(y.double(), ref, 6e-3, "conv1 mma cmvn=%s" % cmvn)
        else:
            ref = torch.relu(torch.nn.functional.conv2d(x[:, None], w, b, stride=2)).permute(0, 2, 3, 1)
            close(y, ref if odt == F32 else ref.bfloat16().float(), 2e-6 if odt == F32 else 1e-2, "conv1 %s" % odt)
        G.check()


@pytest.mark.parametrize("fm", [0, 2, 3, 4, 8, 10])
def test_conv12_relu_every_tile(cfm, fm):
    """cfm_conv12_relu == cfm_conv1_relu_mma followed by cfm_gemm(conv, ReLU), bit for bit (tests/test_frontend_gpu.py), on every row tile the
    setter can force; 3 * 20 * 20 = 1200 output rows are no multiple of 64, 96, 128, 256 or 320."""
    B, T, C, F = 3, 83, 256, 83
    T1, F1 = (T - 3) // 2 + 1, (F - 3) // 2 + 1
    T2, F2 = (T1 - 3) // 2 + 1, (F1 - 3) // 2 + 1
    x, w1, b1 = rnd((B, T, F), 60), rnd((9, C), 61, 1 / 3), rnd((C,), 62, 0.1)
    w2, b2 = rnd((C, 9 * C), 65, (9 * C) ** -0.5).to(BF), rnd((C,), 66, 0.1)
    h1 = cfm.conv1_relu(x, w1, b1, BF, mma=True)
    ref = cfm.gemm(h1, w2, bias=b2, act=cfm.ACT_RELU, conv=(C, T1, F1, T2, F2, B * T2 * F2), out_dtype=BF)
    G = Guards()
    y = G.out((B * T2 * F2, C), BF, name="y")
    args = [G.inp(t, name=n).data_ptr() for n, t in (("x", x), ("w1", w1), ("b1", b1), ("w2", w2), ("b2", b2))]
    L = cfm.lib()
    prev = L.cfm_set_conv12_tile(fm)
    try:
        cfm.check(L.cfm_conv12_relu(*args, y.data_ptr(), cfm.BF16, B, T, F, C, None, None, cfm.stream()), "cfm_conv12_relu")
        torch.cuda.synchronize()
    finally:
        L.cfm_set_conv12_tile(prev)
    assert float(ref.float().abs().max()) > 0.1
    exact(y, ref, "conv12 fm=%d" % fm)
    G.check()


# ---------------------------------------------------------------------------------------------------------------- stream.hip
def _stream_refs(offsets, T, need, ring_T, pe):
    """include/cfm.h: slot f mod ring_T holds frame f for f in [offset - min(offset, need), offset + T); pos_rows = pe[that frame]."""
    B, D = len(offsets), pe.shape[1]
    mask, frame = torch.zeros((B, ring_T), dtype=torch.uint8), torch.full((B, ring_T), -1, dtype=torch.int64)
    for b, off in enumerate(offsets):
        for f in range(off - min(off, need), off + T):
            mask[b, f % ring_T], frame[b, f % ring_T] = 1, f
    return mask, frame


@pytest.mark.parametrize("D", [16, 144])
@pytest.mark.parametrize("abs_rows", [False, True])
def test_stream_prep_and_advance(cfm, D, abs_rows):
    """include/cfm.h defines pos_rows for the slots that hold a frame; what a dead slot (slot_mask 0, never attended to) receives is unspecified there, so
    those rows are only required to be written with a row of the table (finite), not with a particular one."""
    offsets, T, need, ring_T, max_len = [0, 5, 37], 4, 6, 10, 64
    B = len(offsets)
    pe = rnd((max_len, D), 70)
    G = Guards()
    ov = G.inp(torch.tensor(offsets, dtype=torch.int32), name="offsets")
    sm, pr = G.out((B, ring_T), torch.uint8, name="slot_mask"), G.out((B, ring_T, D), F32, name="pos_rows")
    ar = G.out((B, D), F32, name="abs_rows") if abs_rows else None
    cfm.stream_prep(ov, T, need, ring_T, G.inp(pe, name="pe"), sm, pr, ar)
    mask, frame = _stream_refs(offsets, T, need, ring_T, pe)
    exact(sm.cpu(), mask, "slot_mask")
    live = mask.bool().cuda()
    exact(pr[live], pe[frame.cuda()[live]], "pos_rows of the live slots")
    assert not bool(torch.isnan(pr).any()), "pos_rows: an owned row was not written"
    if abs_rows:
        exact(ar, pe[torch.tensor(offsets, device="cuda")], "abs_rows")
    G.check()
    G = Guards()
    ov = G.io(torch.tensor(offsets, dtype=torch.int32), name="offsets")
    cfm.stream_advance(ov, T, G.inp(torch.tensor([1, 0, 1], dtype=torch.uint8), name="active"))
    exact(ov.cpu(), torch.tensor([4, 5, 41], dtype=torch.int32), "offsets")
    cfm.stream_advance(ov, T)
    exact(ov.cpu(), torch.tensor([8, 9, 45], dtype=torch.int32), "offsets, all active")
    G.check()


@pytest.mark.parametrize("H,dk", [(2, 8), (4, 36)])
def test_kv_ring_write(cfm, H, dk):
    offsets, T, ring_T = [0, 5, 37], 4, 10
    B, D = len(offsets), H * dk
    ld = 3 * D + 8
    G = Guards()
    qkv, ring0 = rnd((B, T, 3 * D), 71).bfloat16(), rnd((B, H, ring_T, 2 * dk), 72)
    qv, ring = G.inp(qkv, ld=ld, name="qkv"), G.io(ring0, name="ring")
    ov = G.inp(torch.tensor(offsets, dtype=torch.int32), name="offsets")
    cfm.check(cfm.lib().cfm_kv_ring_write(qv[..., D:].data_ptr(), qv[..., 2 * D:].data_ptr(), cfm.BF16, T * ld, ld, T * ld, ld, ring.data_ptr(), ov.data_ptr(),
                                          None, B, H, T, dk, ring_T, cfm.stream()), "cfm_kv_ring_write")
    want = ring0.clone()
    for b, off in enumerate(offsets):
        for t in range(T):
            want[b, :, (off + t) % ring_T, :dk] = qkv[b, t, D:2 * D].float().view(H, dk)
            want[b, :, (off + t) % ring_T, dk:] = qkv[b, t, 2 * D:].float().view(H, dk)
    exact(ring, want, "ring")
    G.check()


@pytest.mark.parametrize("T", [1, 3, 20])
@pytest.mark.parametrize("D", [16, 144])
@pytest.mark.parametrize("with_cache", [False, True])
def test_causal_conv_and_cache_update(cfm, T, D, with_cache):
    B, K = 3, 15
    for dt, tol in ((BF, 1e-2), (F32, 1e-5)):
        G = Guards()
        x, cache = rnd((B, T, D), 73).to(dt), rnd((B, K - 1, D), 74)
        (w, db, sc, sh), pv = _dw_params(G, D, K)
        xv = G.inp(x, name="x")
        cv = G.inp(cache, name="cache") if with_cache else None
        y = G.out((B, T, D), dt, name="y")
        cfm.check(cfm.lib().cfm_dwconv_causal_bn_silu(xv.data_ptr(), cfm.dt_code(dt), cfm.ptr(cv), *[t.data_ptr() for t in pv], y.data_ptr(), cfm.dt_code(dt), B, T, D, K,
                                                      cfm.stream()), "cfm_dwconv_causal_bn_silu")
        left = cache.double() if with_cache else torch.zeros((B, K - 1, D), dtype=torch.float64, device="cuda")
        xx = torch.cat([left, x.double()], 1)                                                    # [cache | x]
        ref = torch.nn.functional.conv1d(xx.transpose(1, 2), w.double()[:, None, :], db.double(), groups=D)
        ref = torch.nn.functional.silu(ref * sc.double()[None, :, None] + sh.double()[None, :, None]).transpose(1, 2)
        close(y.double(), ref, tol, "causal conv %s" % dt)
        G.check()
        G = Guards()
        xv, cv = G.inp(x, name="x"), G.io(cache, name="cache")
        cfm.conv_cache_update(xv, cv, K)
        exact(cv, torch.cat([cache, x.float()], 1)[:, -(K - 1):].contiguous(), "cache update")
        G.check()


# ---------------------------------------------------------------------------------------------------------------- element-wise, masks, optimizer
SIZES = [1, 1023, 4096 * 3 + 1]


@pytest.mark.parametrize("n", SIZES)
def test_cast_add_rows_dropout_sumsq(cfm, n):
    L = cfm.lib()
    x = rnd((n,), 80)
    for src, ddt in ((x, BF), (x.half(), F32), (x, torch.float16)):
        G = Guards()
        sv, dv = G.inp(src, name="src"), G.out((n,), ddt, name="dst")
        cfm.check(L.cfm_cast(sv.data_ptr(), cfm.dt_code(src), dv.data_ptr(), cfm.dt_code(ddt), n, cfm.stream()), "cfm_cast")
        exact(dv, src.to(ddt), "cast")
        G.check()
    # add_rows: n rows of 16 in groups of 3 (ragged last group)
    G = Guards()
    y, add = rnd((n, 16), 81), rnd(((n + 2) // 3, 16), 82)
    yv = G.io(y, name="x")
    cfm.add_rows(yv, G.inp(add, name="add"), 3)
    exact(yv, y + add.repeat_interleave(3, 0)[:n], "add_rows")
    G.check()
    # dropout_rows: [n, 8] with a row mask
    G = Guards()
    xm = rnd((n, 8), 83)
    rm = (torch.rand(n, generator=torch.Generator().manual_seed(84)) > 0.3).cuda()
    yv = G.out((n, 8), F32, name="y")
    cfm.check(L.cfm_dropout_rows(G.inp(xm, name="x").data_ptr(), cfm.F32, yv.data_ptr(), cfm.F32, G.inp(u8(rm), name="row_mask").data_ptr(), 0.5, 0.1, 99, 0.2, 100, n, 8,
                                 cfm.stream()), "cfm_dropout_rows")
    k = cfm.dropout_mask(n * 8, 0.1, 99, "cuda").view(n, 8) & cfm.dropout_mask(n * 8, 0.2, 100, "cuda").view(n, 8)
    close(yv, 0.5 * xm * k / (0.9 * 0.8) * rm[:, None], 1e-6, "dropout_rows")
    G.check()
    # sumsq with its partials as a workspace of exactly n_partials floats
    G = Guards()
    nb = max(1, min(1024, (n + 4095) // 4096))
    part, out = G.ws(nb, name="partials"), G.out((1,), F32, name="out")
    cfm.check(L.cfm_sumsq(G.inp(x, name="x").data_ptr(), n, part.data_ptr(), nb, out.data_ptr(), cfm.stream()), "cfm_sumsq")
    close(out, (x.double() ** 2).sum().view(1), 1e-5, "sumsq")
    G.check()


@pytest.mark.parametrize("n", SIZES)
def test_adam_steps(cfm, n):
    p, g = rnd((n,), 40), rnd((n,), 41)
    ref_p = torch.nn.Parameter(p.clone())
    opt = torch.optim.Adam([ref_p], lr=1e-3, betas=(0.9, 0.98), eps=1e-9, weight_decay=0.0)
    ref_p.grad = g * 0.37
    opt.step()
    G = Guards()
    pv, mv, vv = G.io(p, name="p"), G.io(torch.zeros(n), name="m"), G.io(torch.zeros(n), name="v")
    cfm.adam_step(pv, G.inp(g, name="g"), mv, vv, 1e-3, (0.9, 0.98), 1e-9, 0.0, 1, grad_scale=G.inp(torch.full((1,), 0.37), name="grad_scale"))
    assert float((pv - ref_p.detach()).abs().max()) < 1e-6
    G.check()
    # the clip variant: scale = inv_world (clip off) and g zeroed as it is read
    G = Guards()
    pv, gv, mv, vv = G.io(p, name="p"), G.io(g, name="g"), G.io(torch.zeros(n), name="m"), G.io(torch.zeros(n), name="v")
    ss, norm = G.inp((g.double() ** 2).sum().float().view(1), name="sumsq"), G.out((1,), F32, name="norm")
    cfm.check(cfm.lib().cfm_adam_clip_step(pv.data_ptr(), gv.data_ptr(), mv.data_ptr(), vv.data_ptr(), n, 1e-3, 0.9, 0.98, 1e-9, 0.0, 1, ss.data_ptr(), 0.0, 0.37, 1,
                                           norm.data_ptr(), cfm.stream()), "cfm_adam_clip_step")
    assert float((pv - ref_p.detach()).abs().max()) < 1e-6
    assert float(gv.abs().max()) == 0.0
    close(norm, (g.double().norm() * 0.37).view(1), 1e-5, "norm")
    G.check()


@pytest.mark.parametrize("T", SIZES)
def test_masks(cfm, T):
    """The uint8 extents are compared EXACTLY (0 / 1): an element left at the 0xFF pre-fill, or written as anything but 0 / 1, fails.  cfm_chunk_mask runs at
    every size, 12 289 squared included, and so does the combine (one batch item there: each further item is another 151 MB mask and its guards)."""
    from oracle import conformer_oracle as O
    import numpy as np
    L = cfm.lib()
    as_u8 = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.uint8))
    lens = torch.tensor([T, max(T - 37, 0), 7, 0], dtype=torch.int32)
    G = Guards()
    out = G.out((4, T), torch.uint8, name="valid")
    cfm.check(L.cfm_valid_mask(G.inp(lens, name="lengths").data_ptr(), 0, out.data_ptr(), 4, T, 0, 1, cfm.stream()), "cfm_valid_mask")
    exact(out.cpu(), as_u8(~O.pad_mask(lens.numpy(), T)), "valid mask")
    G.check()
    G = Guards()
    ch = G.out((T, T), torch.uint8, name="chunk")
    cfm.check(L.cfm_chunk_mask(ch.data_ptr(), T, 4, 2, cfm.stream()), "cfm_chunk_mask")
    chunk_ref = as_u8(O.chunk_mask(T, 4, 2)).cuda()
    exact(ch, chunk_ref, "chunk mask")
    G.check()
    B = 2 if T <= 1023 else 1
    G = Guards()
    valid = torch.arange(T)[None, :] < torch.tensor([T // 2 + 1, T][:B])[:, None]
    am = G.out((B, T, T), torch.uint8, name="attn_mask")
    cfm.check(L.cfm_attn_mask(G.inp(u8(valid), name="valid").data_ptr(), G.inp(chunk_ref, name="chunk").data_ptr(), am.data_ptr(), B, T, cfm.stream()), "cfm_attn_mask")
    exact(am, u8(valid).cuda()[:, None, :] & chunk_ref[None], "attn mask")
    G.check()


# ---------------------------------------------------------------------------------------------------------------- joint
@pytest.mark.parametrize("B,T,U,J", [(2, 5, 3, 72), (1, 1, 1, 512)])
def test_joint_act_and_bwd(cfm, B, T, U, J):
    L = cfm.lib()
    enc, pred = rnd((B * T, J), 71, 1.5), rnd((B * U, J), 72, 1.5)
    enc[0, :4] = torch.tensor([40.0, -40.0, 0.0, 1e-4])
    ref = torch.tanh(enc.view(B, T, 1, J).double() + pred.view(B, 1, U, J).double()).view(B * T * U, J)
    for odt, tol in ((F32, 5e-7), (BF, 4e-3), (torch.float16, 5e-4)):
        G = Guards()
        ev, pv, out = G.inp(enc, ld=J + 8, name="enc"), G.inp(pred, ld=J + 16, name="pred"), G.out((B * T * U, J), odt, name="out")
        cfm.check(L.cfm_joint_act(ev.data_ptr(), J + 8, pv.data_ptr(), J + 16, out.data_ptr(), cfm.dt_code(odt), B, T, U, J, cfm.stream()), "cfm_joint_act")
        err = float((out.double() - ref).abs().max())
        assert err < tol, (odt, err)
        G.check()
    # backward: d_enc = sum_u dact (1 - a^2), d_pred = sum_t (autograd of the same expression in f64).  No op-level test of it existed; the bound
    # follows from test_joint_act's own: |a - tanh| < 5e-7 gives |(1 - a^2) - (1 - tanh^2)| < 1e-6 per term, at most 5 terms of |dact| <~ 4 summed in
    # f32 (6e-8 each) against a largest gradient above 1: below 1e-5 relative.
    dact = rnd((B * T * U, J), 73)
    er, pr = enc.double().requires_grad_(True), pred.double().requires_grad_(True)
    torch.tanh(er.view(B, T, 1, J) + pr.view(B, 1, U, J)).backward(dact.double().view(B, T, U, J))
    G = Guards()
    ev, pv, dv = G.inp(enc, ld=J + 8, name="enc"), G.inp(pred, ld=J + 16, name="pred"), G.inp(dact, name="dact")
    de, dp, ws = G.out((B * T, J), F32, name="d_enc"), G.out((B * U, J), F32, name="d_pred"), G.ws(L.cfm_joint_act_bwd_ws(B, T, U, J), name="work")
    cfm.check(L.cfm_joint_act_bwd(ev.data_ptr(), J + 8, pv.data_ptr(), J + 16, dv.data_ptr(), de.data_ptr(), dp.data_ptr(), ws.data_ptr(), B, T, U, J, cfm.stream()),
              "cfm_joint_act_bwd")
    close(de, er.grad, 1e-5, "d_enc")
    close(dp, pr.grad, 1e-5, "d_pred")
    G.check()


# ---------------------------------------------------------------------------------------------------------------- CTC
@pytest.mark.parametrize("B,T,V,Umax,ld", [(4, 30, 11, 5, 16), (3, 49, 73, 9, 73)])
def test_ctc_nll_groups_and_grad(cfm, B, T, V, Umax, ld):
    """inputs as tests/test_train_ops_gpu.py test_ctc_gradient builds them; work / alpha / beta / lse are workspaces of exactly the documented size."""
    import numpy as np
    L = cfm.lib()
    if ld % 4:
        # the ABI takes row strides that are multiples of 4 floats only: ld = 73 is a loud argument error before any launch (nothing is touched),
        # and the shape then runs at the smallest stride the ABI can express, 76
        G = Guards()
        lv, iv, work, nll = G.inp(torch.zeros((B, T, ld)), name="logits"), G.inp(torch.ones((B, Umax), dtype=torch.int32), name="ints"), G.ws(B * T * (2 * Umax + 2)), G.out((B,), F32)
        with pytest.raises(RuntimeError, match="multiple of 4"):
            cfm.check(L.cfm_ctc_nll(lv.data_ptr(), ld, B, T, V, iv.data_ptr(), iv.data_ptr(), Umax, iv.data_ptr(), work.data_ptr(), nll.data_ptr(), cfm.stream()), "cfm_ctc_nll")
        torch.cuda.synchronize()
        assert bool(torch.isnan(nll).all())
        G.check()
        ld = (ld + 3) // 4 * 4
    rs = np.random.RandomState(B * 100 + T)
    logits = torch.zeros((B, T, ld), device="cuda")
    logits[:, :, :V] = rnd((B, T, V), 38, 2.0)
    enc_lens = np.sort(rs.randint(max(2 * Umax + 1, T // 2), T + 1, size=B))[::-1].copy()
    enc_lens[0] = T
    label_lens = rs.randint(1, Umax + 1, size=B)
    label_lens[0] = Umax
    labels = rs.randint(1, V, size=(B, Umax))
    labels[1, 1:3] = labels[1, 0]
    for b in range(B):
        labels[b, label_lens[b]:] = 0
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype=torch.int32)
    lr = logits[:, :, :V].detach().cpu().double().requires_grad_(True)
    per = torch.nn.functional.ctc_loss(lr.transpose(0, 1).log_softmax(2), torch.from_numpy(labels), torch.from_numpy(enc_lens), torch.from_numpy(label_lens), reduction="none")
    (per.sum() / Umax).backward()
    SM = 2 * Umax + 2
    # cfm_ctc_nll
    G = Guards()
    lv, el, lb, ll = G.inp(logits, name="logits"), G.inp(i32(enc_lens), name="enc_lens"), G.inp(i32(labels), name="labels"), G.inp(i32(label_lens), name="label_lens")
    work, nll = G.ws(B * T * SM, name="work"), G.out((B,), F32, name="nll")
    cfm.check(L.cfm_ctc_nll(lv.data_ptr(), ld, B, T, V, el.data_ptr(), lb.data_ptr(), Umax, ll.data_ptr(), work.data_ptr(), nll.data_ptr(), cfm.stream()), "cfm_ctc_nll")
    assert torch.allclose(nll.cpu().double(), per.detach(), rtol=1e-5, atol=1e-4), (nll, per)
    G.check()
    # cfm_ctc_nll_train_groups, then cfm_ctc_grad on its state
    G = Guards()
    lv, el, lb, ll = G.inp(logits, name="logits"), G.inp(i32(enc_lens), name="enc_lens"), G.inp(i32(labels), name="labels"), G.inp(i32(label_lens), name="label_lens")
    work, alpha, beta = (G.ws(B * T * SM, name=n) for n in ("work", "alpha", "beta"))
    lse, nll, nllp = G.ws(B * T, name="lse"), G.out((B,), F32, name="nll"), G.out((B,), F32, name="nll_shifted")
    arr = (cfm.CtcGroup * 1)()
    g = arr[0]
    g.logits, g.ld, g.B, g.T, g.Umax = lv.data_ptr(), ld, B, T, Umax
    g.enc_lens, g.labels, g.label_lens = el.data_ptr(), lb.data_ptr(), ll.data_ptr()
    g.work, g.alpha, g.lse, g.nll, g.nll_shifted, g.beta = work.data_ptr(), alpha.data_ptr(), lse.data_ptr(), nll.data_ptr(), nllp.data_ptr(), beta.data_ptr()
    cfm.check(L.cfm_ctc_nll_train_groups(arr, 1, V, cfm.stream()), "cfm_ctc_nll_train_groups")
    close(nll.cpu(), per.detach(), 2e-5, "nll")
    assert not bool(torch.isnan(nllp).any())
    G.check()
    gdev, grad = G.inp(torch.full((1,), 2.0), name="gscale_dev"), G.out((B, T, ld), F32, name="dlogits")
    cfm.check(L.cfm_ctc_grad(lv.data_ptr(), ld, B, T, V, el.data_ptr(), lb.data_ptr(), Umax, ll.data_ptr(), work.data_ptr(), alpha.data_ptr(), beta.data_ptr(), lse.data_ptr(),
                             nllp.data_ptr(), 0.5 / Umax, gdev.data_ptr(), grad.data_ptr(), cfm.stream()), "cfm_ctc_grad")
    if ld > V:
        assert float(grad[:, :, V:].abs().max()) == 0.0                      # NaN (unwritten pad columns) fails this too
    close(grad[:, :, :V].cpu(), lr.grad, 5e-4, "dlogits")
    for b in range(B):
        if enc_lens[b] < T:
            assert float(grad[b, int(enc_lens[b]):].abs().max()) == 0.0
    G.check()


# ---------------------------------------------------------------------------------------------------------------- attention backward
@pytest.mark.parametrize("B,T,H,dk", [(2, 65, 2, 16), (3, 37, 4, 36), (2, 100, 8, 64)])
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("mkind", ["none", "pad", "chunk"])
@pytest.mark.parametrize("general", [0, 1])
def test_attention_backward(cfm, B, T, H, dk, mode, mkind, general):
    """general = 1 forces the general kernels where d_k = 64 with 16-bit rows would take the fast family (elsewhere both runs take the general ones)."""
    from test_train_ops_gpu import _attn_ref
    D, split = H * dk, mode == "fp32"
    ld = 3 * D + 16
    dt = F32 if split else BF
    qkv, dout = rnd((B * T, 3 * D), 36, 0.7).to(dt), rnd((B * T, D), 37).to(dt)
    lens = [T, max(1, T - T // 4), max(1, T // 2)][:B]
    valid = (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).cuda()
    mask = None
    if mkind == "pad":
        mask = valid[:, None, :]
    elif mkind == "chunk":
        blk = torch.arange(T) // 8
        mask = ((blk[None, :] <= blk[:, None]) & (blk[None, :] >= blk[:, None] - 1)).cuda()[None] & valid[:, None, :]
    x = qkv.double().view(B, T, 3, H, dk).requires_grad_(True)
    _attn_ref(x[:, :, 0], x[:, :, 1], x[:, :, 2], mask, dk ** -0.5).backward(dout.double().view(B, T, D))
    g_ref = x.grad.reshape(B * T, 3 * D)
    ctx, lse = torch.empty((B * T, D), dtype=dt, device="cuda"), torch.empty((B, H, T), dtype=F32, device="cuda")
    m8 = None if mask is None else mask.contiguous().view(torch.uint8)
    mstr = (0, 0) if mask is None else (mask.shape[1] * T, T if mask.shape[1] > 1 else 0)
    st = (T * 3 * D, 3 * D)
    cfm.attention(qkv, qkv[:, D:], qkv[:, 2 * D:], B, H, T, T, dk, st, st + (dk,), st + (dk,), ctx, mask=m8, mask_str=mstr, split=split, lse=lse)
    G = Guards()
    qv, cv, dov, lv = G.inp(qkv, ld=ld, name="qkv"), G.inp(ctx, name="out"), G.inp(dout, name="dout"), G.inp(lse, name="lse")
    mv = G.inp(m8, name="mask") if m8 is not None else None
    dqkv, delta = G.out((B * T, 3 * D), dt, ld=ld, name="dqkv"), G.ws(B * H * T, name="delta")
    d = cfm.AttnBwdDesc()
    d.q, d.k, d.v, d.mask, d.out, d.dout, d.lse = qv.data_ptr(), qv[:, D:].data_ptr(), qv[:, 2 * D:].data_ptr(), cfm.ptr(mv), cv.data_ptr(), dov.data_ptr(), lv.data_ptr()
    d.grad_q, d.grad_k, d.grad_v, d.delta = dqkv.data_ptr(), dqkv[:, D:].data_ptr(), dqkv[:, 2 * D:].data_ptr(), delta.data_ptr()
    d.q_sb = d.k_sb = d.v_sb = T * ld
    d.q_st = d.k_st = d.v_st = ld
    d.m_sb, d.m_sq = mstr
    d.B, d.H, d.Tq, d.Tk, d.dk = B, H, T, T, dk
    d.io_dtype, d.dout_dtype, d.mma_dtype, d.split, d.scale = cfm.dt_code(dt), cfm.dt_code(dt), cfm.BF16, int(split), dk ** -0.5
    L = cfm.lib()
    L.cfm_attention_bwd_force_general(general)
    try:
        cfm.check(L.cfm_attention_bwd(ctypes.byref(d), cfm.stream()), "cfm_attention_bwd")
        torch.cuda.synchronize()
    finally:
        L.cfm_attention_bwd_force_general(0)
    gtol = dict(bf16=3e-2, fp32=1e-4)[mode]
    for name, sl in (("dq", slice(0, D)), ("dk", slice(D, 2 * D)), ("dv", slice(2 * D, 3 * D))):
        close(dqkv[:, sl], g_ref[:, sl], gtol, name)
    G.check()


# ---------------------------------------------------------------------------------------------------------------- depthwise + BatchNorm (train)
@pytest.mark.parametrize("B,T,D", [(1, 3, 16), (3, 37, 144)])
@pytest.mark.parametrize("dt", [F32, BF])
def test_dwconv_bn_train_fwd_bwd(cfm, B, T, D, dt):
    K, L = 15, cfm.lib()
    g = rnd((B, T, D), 23).to(dt)
    w, bias = rnd((D, K), 24, K ** -0.5), rnd((D,), 25, 0.1)
    gamma, beta = 1 + rnd((D,), 26, 0.1), rnd((D,), 27, 0.1)
    rm0, rv0 = rnd((D,), 28, 0.1), 1 + rnd((D,), 29, 0.1).abs()
    leaves = [t.double().requires_grad_(True) for t in (g.float(), w, bias, gamma, beta)]
    gr, wr, br, gar, ber = leaves
    rmr, rvr = rm0.double().clone(), rv0.double().clone()
    cr = torch.nn.functional.conv1d(gr.transpose(1, 2), wr.unsqueeze(1), br, padding=7, groups=D)
    sr = torch.nn.functional.silu(torch.nn.functional.batch_norm(cr, rmr, rvr, gar, ber, True, 0.1, 1e-5)).transpose(1, 2)
    G = Guards()
    gv, wv, bv, gav, bev = G.inp(g, name="g"), G.inp(w, name="w"), G.inp(bias, name="dw_bias"), G.inp(gamma, name="gamma"), G.inp(beta, name="beta")
    rm, rv = G.io(rm0, name="running_mean"), G.io(rv0, name="running_var")
    c, stats, s = G.out((B, T, D), F32, name="c"), G.out((1, 4, D), F32, name="stats"), G.out((B, T, D), dt, name="s")
    ws = G.ws(L.cfm_dwconv_bn_ws(B, T, D), name="ws")
    one = (cfm.TrainGroup * 1)()
    one[0].B, one[0].T, one[0].row0 = B, T, 0
    cfm.check(L.cfm_dwconv_bn_train_groups(gv.data_ptr(), cfm.dt_code(dt), wv.data_ptr(), bv.data_ptr(), gav.data_ptr(), bev.data_ptr(), rm.data_ptr(), rv.data_ptr(), 0.1,
                                           1e-5, c.data_ptr(), stats.data_ptr(), s.data_ptr(), cfm.dt_code(dt), ws.data_ptr(), one, 1, D, K, cfm.stream()),
              "cfm_dwconv_bn_train_groups")
    close(c, cr.transpose(1, 2), 1e-5, "c")
    close(s, sr, 1e-5 if dt == F32 else 1e-2, "s")
    close(rm, rmr, 1e-5, "running_mean")
    close(rv, rvr, 1e-5, "running_var")
    # stats = mean, rstd, scale = gamma * rstd, shift = beta - mean * scale (include/cfm.h) against the f64 batch statistics of c
    mean, var = cr.detach().mean((0, 2)), cr.detach().var((0, 2), unbiased=False)
    rstd = (var + 1e-5).rsqrt()
    for i, (name, ref) in enumerate((("mean", mean), ("rstd", rstd), ("scale", gamma.double() * rstd), ("shift", beta.double() - mean * gamma.double() * rstd))):
        close(stats[0, i], ref, 1e-5, "stats: " + name)             # the f32 bound this op's test uses for c and the running statistics
    G.check()
    ds = rnd((B, T, D), 30).to(dt)
    sr.backward(ds.double())
    prior = [rnd((D, K), 31), rnd((D,), 32), rnd((D,), 33), rnd((D,), 34)]
    for acc in (0, 1):
        G2 = Guards()
        dsv, cv, stv, gv2, wv2 = G2.inp(ds, name="ds"), G2.inp(c.contiguous(), name="c"), G2.inp(stats.contiguous(), name="stats"), G2.inp(g, name="g"), G2.inp(w, name="w")
        dg = G2.out((B, T, D), dt, name="dg")
        outs = [G2.io(p, name=n) for p, n in zip(prior, ("dw_w", "dw_b", "dgamma", "dbeta"))] if acc else \
               [G2.out(p.shape, F32, name=n) for p, n in zip(prior, ("dw_w", "dw_b", "dgamma", "dbeta"))]
        dy_ws, ws2 = G2.ws(B * T * D, name="dy_ws"), G2.ws(L.cfm_dwconv_bn_ws(B, T, D), name="ws")
        args = [dsv.data_ptr(), cfm.dt_code(dt), cv.data_ptr(), stv.data_ptr(), gv2.data_ptr(), cfm.dt_code(dt), wv2.data_ptr(), dg.data_ptr(), cfm.dt_code(dt)] + \
               [o.data_ptr() for o in outs] + [dy_ws.data_ptr(), ws2.data_ptr(), one, 1, D, K]
        cfm.check(L.cfm_dwconv_bn_train_bwd_groups(*args, acc, None, None, cfm.stream()), "cfm_dwconv_bn_train_bwd_groups")
        base = [p.double() if acc else torch.zeros_like(p, dtype=torch.float64) for p in prior]
        close(dg, gr.grad, 1e-4 if dt == F32 else 1e-2, "dg")
        close(outs[0].double() - base[0], wr.grad, 1e-4, "dw_w")
        close(outs[2].double() - base[2], gar.grad, 1e-4, "dgamma")
        close(outs[3].double() - base[3], ber.grad, 1e-4, "dbeta")
        assert float((outs[1].double() - base[1]).abs().max()) < 1e-3 * float(ber.grad.abs().max() + 1e-6)
        G2.check()


# ---------------------------------------------------------------------------------------------------------------- front-end backward, GLU backward
@pytest.mark.parametrize("B,T,C", [(1, 7, 16), (2, 83, 144)])
def test_frontend_backward_pieces(cfm, B, T, C):
    F, L = 80, cfm.lib()
    T1, F1 = (T - 3) // 2 + 1, (F - 3) // 2 + 1
    T2, F2 = (T1 - 3) // 2 + 1, (F1 - 3) // 2 + 1
    x, h1, dcol = rnd((B, T, F), 31), torch.relu(rnd((B, T1, F1, C), 32)), rnd((B * T2 * F2, 9 * C), 33)
    cols = dcol.double().view(B, T2 * F2, 3, 3, C).permute(0, 4, 2, 3, 1).reshape(B, C * 9, T2 * F2)
    ref = torch.nn.functional.fold(cols, (T1, F1), kernel_size=3, stride=2).permute(0, 2, 3, 1) * (h1 > 0)
    G = Guards()
    dh1 = G.out((B, T1, F1, C), F32, name="dh1")
    cfm.check(L.cfm_col2im_relu_bwd(G.inp(dcol, name="dcol").data_ptr(), cfm.F32, G.inp(h1, name="h1").data_ptr(), cfm.F32, dh1.data_ptr(), cfm.F32, B, T1, F1, C,
                                    cfm.stream()), "cfm_col2im_relu_bwd")
    close(dh1, ref, 1e-5, "dh1")
    G.check()
    w = torch.zeros((C, 1, 3, 3), dtype=torch.float64, device="cuda", requires_grad=True)
    b = torch.zeros((C,), dtype=torch.float64, device="cuda", requires_grad=True)
    mean, istd = rnd((F,), 34, 0.1), 1 + rnd((F,), 35, 0.1).abs()
    torch.nn.functional.conv2d(((x - mean) * istd).double().unsqueeze(1), w, b, stride=2).backward(dh1.double().permute(0, 3, 1, 2))
    G = Guards()
    dw, db, ws = G.out((9, C), F32, name="dw"), G.out((C,), F32, name="db"), G.ws(L.cfm_conv1_wgrad_ws(B, T, C), name="ws")
    cfm.check(L.cfm_conv1_wgrad(G.inp(dh1.contiguous(), name="dh1").data_ptr(), cfm.F32, G.inp(x, name="x").data_ptr(), G.inp(mean, name="mean").data_ptr(),
                                G.inp(istd, name="istd").data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), B, T, F, C, cfm.stream()), "cfm_conv1_wgrad")
    close(dw, w.grad.reshape(C, 9).t(), 2e-5, "dw")
    close(db, b.grad, 2e-5, "db")
    G.check()
    # GLU backward on the interleaved layout, M = B*T rows of 2C columns
    M, D = B * T, C
    z, dg = rnd((M, 2 * D), 13), rnd((M, D), 16)
    zr = z.clone().requires_grad_(True)
    zv = zr.view(M, D // 16, 2, 16)
    (zv[:, :, 0] * torch.sigmoid(zv[:, :, 1])).reshape(M, D).backward(dg)
    G = Guards()
    du = G.out((M, 2 * D), F32, name="du")
    cfm.check(L.cfm_glu_bwd(G.inp(z, name="u").data_ptr(), cfm.F32, G.inp(dg, name="dg").data_ptr(), cfm.F32, du.data_ptr(), cfm.F32, M, D, cfm.stream()), "cfm_glu_bwd")
    close(du, zr.grad, 1e-5, "du")
    G.check()


# ---------------------------------------------------------------------------------------------------------------- fused feed-forward, row chains
@pytest.mark.parametrize("M,D,FF", [(5, 144, 64), (33, 256, 2048)])
def test_ffn_fused(cfm, M, D, FF):
    from cfm import packing
    Fn = torch.nn.functional
    x = rnd((M, D), 90, 1.5) + 0.3
    w1, w2 = rnd((FF, D), 91, D ** -0.5), rnd((D, FF), 92, FF ** -0.5)
    b1, b2 = rnd((FF,), 93, 0.1), rnd((D,), 94, 0.1)
    lns = [(1 + 0.1 * rnd((D,), 95 + i), 0.1 * rnd((D,), 98 + i)) for i in range(3)]
    w1f, w2f = packing.pack_ffn_fragments(w1, w2, BF)
    a = Fn.layer_norm(x, (D,), lns[0][0], lns[0][1], 1e-5)
    h = Fn.silu(a.to(BF).float() @ w1.to(BF).float().t() + b1)
    r1 = x + 0.5 * (h.to(BF).float() @ w2.to(BF).float().t() + b2)
    r2 = Fn.layer_norm(r1, (D,), lns[2][0], lns[2][1], 1e-5)
    G = Guards()
    d = cfm.FfnDesc()
    o32, o16 = G.out((M, D), F32, name="out_f32"), G.out((M, D), BF, name="out16")
    d.x, d.w1f, d.w2f, d.b1, d.b2 = (G.inp(t, name=n).data_ptr() for t, n in ((x, "x"), (w1f, "w1f"), (w2f, "w2f"), (b1, "b1"), (b2, "b2")))
    d.ln_g, d.ln_b, d.ln2_g, d.ln2_b = (G.inp(t, name=n).data_ptr() for t, n in ((lns[0][0], "ln_g"), (lns[0][1], "ln_b"), (lns[2][0], "ln2_g"), (lns[2][1], "ln2_b")))
    d.out_f32, d.out16, d.M, d.D, d.FF = o32.data_ptr(), o16.data_ptr(), M, D, FF
    d.w_dtype, d.out16_dtype, d.act, d.add_x, d.alpha, d.eps = cfm.BF16, cfm.BF16, cfm.ACT_SILU, 1, 0.5, 1e-5
    cfm.check(cfm.lib().cfm_ffn_fused(ctypes.byref(d), cfm.stream()), "cfm_ffn_fused")
    close(o32, r1, 6e-3, "out_f32")
    close(o16, r2, 6e-3 + 1e-2, "out16")
    G.check()


@pytest.mark.parametrize("M", [1, 31, 33])
def test_rowchain_three_roles(cfm, M):
    """the macaron / conv-in / final chains as tests/test_ops_gpu.py test_rowchain_three_roles runs them (D = 144, FF = 576, bf16)."""
    from cfm import packing
    D, FF, dt, code, Fn = 144, 576, BF, cfm.BF16, torch.nn.functional
    x, a16 = rnd((M, D), 100, 1.5) + 0.3, rnd((M, D), 101).to(dt)
    w1, w2 = rnd((FF, D), 102, D ** -0.5), rnd((D, FF), 103, FF ** -0.5)
    b1, b2 = rnd((FF,), 104, 0.1), rnd((D,), 105, 0.1)
    wh, bh = rnd((D, D), 106, D ** -0.5), rnd((D,), 107, 0.1)
    wq, bq = rnd((3 * D, D), 108, D ** -0.5), rnd((3 * D,), 109, 0.1)
    wg, bg = rnd((2 * D, D), 110, D ** -0.5), rnd((2 * D,), 111, 0.2)
    lns = [(1 + 0.1 * rnd((D,), 112 + i), 0.1 * rnd((D,), 116 + i)) for i in range(3)]
    mask = u8(torch.rand(M, generator=torch.Generator().manual_seed(9)) > 0.3).cuda()
    r16 = lambda t: t.to(dt).float()
    lin = lambda a, w, b: r16(a) @ r16(w).t() + b
    ffn = lambda xn: lin(Fn.silu(lin(xn, w1, b1)), w2, b2)
    ln = lambda t, p: Fn.layer_norm(t, (D,), p[0], p[1], 1e-5)
    tol, tol16 = 8e-3, 8e-3 + 1e-2
    idx = packing.glu_interleave_index(D, "cuda")

    def placed(G):
        P = lambda t, n: G.inp(t.contiguous(), name=n)
        return dict(ffn=(P(packing.pack_frag_major(w1, dt), "w1f"), P(packing.pack_frag_major(w2, dt), "w2n"), P(b1, "b1"), P(b2, "b2"), FF),
                    lns=[(P(g, "ln%d_g" % i), P(b, "ln%d_b" % i)) for i, (g, b) in enumerate(lns)], wh=P(packing.pack_frag_major(wh, dt), "head_w"), bh=P(bh, "head_b"),
                    a16=P(a16, "head_a"), mask=P(mask, "mask"))

    # macaron
    G = Guards()
    o = placed(G)
    out, qkv = G.out((M, D), F32, name="out_f32"), G.out((M, 3 * D), dt, name="tail_out")
    cfm.rowchain(M, D, code, x=G.inp(x, name="x"), ln=o["lns"][0], ffn=o["ffn"], alpha=0.5, ln2=o["lns"][1], out_f32=out,
                 tail=(G.inp(packing.pack_frag_major(wq, dt), name="tail_w"), G.inp(bq, name="tail_b"), 3 * D, False, qkv))
    x1 = x + 0.5 * ffn(ln(x, lns[0]))
    close(out, x1, tol, "macaron out")
    close(qkv, lin(ln(x1, lns[1]), wq, bq), tol16, "qkv")
    G.check()
    # conv-in, in place over the residual
    G = Guards()
    o = placed(G)
    xi, glu = G.io(x, name="head_res = out_f32"), G.out((M, D), dt, name="tail_out")
    cfm.rowchain(M, D, code, head=(o["a16"], o["wh"], o["bh"], xi, None), ln=o["lns"][2], ln_mask=o["mask"], out_f32=xi,
                 tail=(G.inp(packing.pack_frag_major(wg[idx], dt), name="tail_w"), G.inp(bg[idx].contiguous(), name="tail_b"), 2 * D, True, glu))
    x2 = x + lin(a16.float(), wh, bh)
    close(xi, x2, tol, "conv-in residual")
    pre = lin(ln(x2, lns[2]) * mask[:, None].float(), wg, bg)
    close(glu, pre[:, :D] * torch.sigmoid(pre[:, D:]), tol16, "glu")
    G.check()
    # final, in place
    G = Guards()
    o = placed(G)
    xi = G.io(x, name="head_res = out_f32")
    cfm.rowchain(M, D, code, head=(o["a16"], o["wh"], o["bh"], xi, o["mask"]), ln=o["lns"][0], ffn=o["ffn"], alpha=0.5, ln1=o["lns"][1], out_f32=xi)
    x3 = x + lin(a16.float(), wh, bh) * mask[:, None].float()
    close(xi, ln(x3 + 0.5 * ffn(ln(x3, lns[0])), lns[1]), tol, "final")
    G.check()


@pytest.mark.parametrize("B,T,D,FF", [(1, 1, 256, 2048), (4, 3, 144, 576), (5, 32, 256, 2048)])
def test_rowchain_depthwise_input_stage(cfm, B, T, D, FF):
    """bf16: bit-identical to cfm_dwconv_bn_silu followed by the plain final chain (tests/test_ops_gpu.py)."""
    from cfm import packing
    dt, code, M = BF, cfm.BF16, B * T
    x, glu = rnd((M, D), 200, 1.2), rnd((B, T, D), 201).to(dt)
    w1, w2 = rnd((FF, D), 202, D ** -0.5), rnd((D, FF), 203, FF ** -0.5)
    b1, b2, wh, bh = rnd((FF,), 204, 0.1), rnd((D,), 205, 0.1), rnd((D, D), 206, D ** -0.5), rnd((D,), 207, 0.1)
    taps, tb, sc, sh = rnd((D, 15), 208, 0.3), rnd((D,), 209, 0.1), 1 + 0.2 * rnd((D,), 210), 0.1 * rnd((D,), 211)
    lns = [(1 + 0.1 * rnd((D,), 212 + i), 0.1 * rnd((D,), 216 + i)) for i in range(2)]
    mask = u8(torch.rand(M, generator=torch.Generator().manual_seed(10)) > 0.2).cuda()
    w1f, w2n, whf = packing.pack_frag_major(w1, dt), packing.pack_frag_major(w2, dt), packing.pack_frag_major(wh, dt)
    dwo = cfm.dwconv_bn_silu(glu, taps, tb, sc, sh, out_dtype=dt)
    ref = x.clone()
    cfm.rowchain(M, D, code, head=(dwo.view(M, D), whf, bh, ref, mask), ln=lns[0], ffn=(w1f, w2n, b1, b2, FF), alpha=0.5, ln1=lns[1], out_f32=ref)
    G = Guards()
    P = lambda t, n: G.inp(t.contiguous(), name=n)
    out = G.io(x, name="head_res = out_f32")
    cfm.rowchain(M, D, code, head=(P(glu.view(M, D), "head_a"), P(whf, "head_w"), P(bh, "head_b"), out, P(mask, "head_mask")), ln=(P(lns[0][0], "ln_g"), P(lns[0][1], "ln_b")),
                 ffn=(P(w1f, "w1f"), P(w2n, "w2n"), P(b1, "b1"), P(b2, "b2"), FF), alpha=0.5, ln1=(P(lns[1][0], "ln1_g"), P(lns[1][1], "ln1_b")), out_f32=out,
                 dw=(P(taps, "dw_w"), P(tb, "dw_b"), P(sc, "dw_scale"), P(sh, "dw_shift"), T))
    exact(out, ref, "depthwise input stage")
    G.check()


@pytest.mark.parametrize("M", [1, 45, 16])
def test_ffn_split(cfm, M):
    """the three modes as tests/test_ops_gpu.py test_ffn_split_modes runs them; the partial slabs are a workspace of exactly [FF/256, M, D]; M = 16: the K/V ring."""
    from cfm import packing
    torch.manual_seed(M)
    D, FF, dt, code = 256, 2048, BF, cfm.BF16
    x = torch.randn((M, D), device="cuda")
    w1, w2 = torch.randn((FF, D), device="cuda") / D ** 0.5, torch.randn((D, FF), device="cuda") / FF ** 0.5
    b1, b2 = 0.1 * torch.randn((FF,), device="cuda"), 0.1 * torch.randn((D,), device="cuda")
    lng = [(1 + 0.1 * torch.randn((D,), device="cuda"), 0.1 * torch.randn((D,), device="cuda")) for _ in range(4)]
    wq, bq = torch.randn((3 * D, D), device="cuda") / D ** 0.5, 0.1 * torch.randn((3 * D,), device="cuda")
    ln = lambda t, p: torch.nn.functional.layer_norm(t, (D,), p[0], p[1], 1e-5)
    r16 = lambda t: t.to(dt).float()
    G = Guards()
    P = lambda t, n: G.inp(t.contiguous(), name=n)
    slabs = G.ws((FF // 256) * M * D, name="psum_out").view(FF // 256, M, D)
    cfm.ffn_split(P(x, "x"), code, 2, ln=(P(lng[0][0], "ln_g"), P(lng[0][1], "ln_b")), w1=P(packing.pack_frag_major(w1, dt), "w1"), b1=P(b1, "b1"), n1=FF, act=cfm.ACT_SILU,
                  w2=P(packing.pack_frag_major(w2, dt), "w2"), psum_out=slabs)
    h = r16(torch.nn.functional.silu(r16(ln(x, lng[0])) @ r16(w1).t() + b1))
    close(slabs, torch.stack([h[:, g * 256:(g + 1) * 256] @ r16(w2)[:, g * 256:(g + 1) * 256].t() for g in range(FF // 256)]), 2e-3, "slabs")
    G.check()
    sl = slabs.contiguous().clone()
    G = Guards()
    P = lambda t, n: G.inp(t.contiguous(), name=n)
    y, y2 = G.out((M, D), F32, name="rows_out"), G.out((M, D), F32, name="rows2_out")
    cfm.ffn_split(P(x, "x"), code, 0, psum=P(sl, "psum"), psum_b2=P(b2, "psum_b2"), psum_alpha=0.5, ln1=(P(lng[1][0], "ln1_g"), P(lng[1][1], "ln1_b")),
                  ln2=(P(lng[2][0], "ln2_g"), P(lng[2][1], "ln2_b")), rows_out=y, rows2_out=y2)
    want = ln(x + 0.5 * (sl.sum(0) + b2), lng[1])
    close(y, want, 1e-5, "rows_out")
    close(y2, ln(want, lng[2]), 1e-5, "rows2_out")
    G.check()
    G = Guards()
    P = lambda t, n: G.inp(t.contiguous(), name=n)
    rows, qkv = G.out((M, D), F32, name="rows_out"), G.out((M, 3 * D), dt, ld=3 * D + 8, name="out16")
    ring = None
    if M % 16 == 0:
        Bs, Tq, H, dk, ring_T = M // 16, 16, 4, 64, 40
        offs = torch.randint(0, 1000, (Bs,), dtype=torch.int32)
        kv0 = rnd((Bs, H, ring_T, 2 * dk), 77)
        kv = G.io(kv0, name="kv_ring")
        ring = (kv, P(offs, "ring_offsets"), Tq)
    cfm.ffn_split(P(x, "x"), code, 1, psum=P(sl, "psum"), psum_b2=P(b2, "psum_b2"), psum_alpha=0.5, rows_out=rows, ln=(P(lng[3][0], "ln_g"), P(lng[3][1], "ln_b")),
                  w1=P(packing.pack_frag_major(wq, dt), "w1"), b1=P(bq, "b1"), n1=3 * D, out16=qkv, ring=ring)
    x1 = x + 0.5 * (sl.sum(0) + b2)
    close(rows, x1, 1e-6, "rows")
    close(qkv, r16(ln(x1, lng[3])) @ r16(wq).t() + bq, 1.2e-2, "qkv")
    if ring is not None:
        want = kv0.clone()
        q3 = qkv.contiguous().view(Bs, Tq, 3 * D).float()
        for b in range(Bs):
            for t in range(Tq):
                slot = (int(offs[b]) + t) % ring_T
                want[b, :, slot, :dk] = q3[b, t, D:2 * D].view(H, dk)
                want[b, :, slot, dk:] = q3[b, t, 2 * D:].view(H, dk)
        exact(kv, want, "kv ring")
    G.check()
