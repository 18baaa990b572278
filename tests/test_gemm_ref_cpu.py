"""CPU: tests/gemm_ref.py -- the float64 restatement of cfm_gemm that tests/test_gemm_matrix_gpu.py compares the kernels with -- checked
without the library: (a) against torch's own operators in float64 at the GPU file's shapes, (b) a discrimination audit: every way the
kernel could plausibly be wrong (gemm_ref.VARIANTS), restated in float64, differs from the right result by more than 10 x the bound on at
least one element of the very inputs the GPU test uses.  The table is printed (pytest -s)."""
import pytest
import torch
import torch.nn.functional as F

import gemm_ref as R

D = torch.float64


def lin(p):
    A = p.A.to(p.W.dtype) if p.W_lo is None else p.A
    W = p.W.double() if p.W_lo is None else p.W.double() + p.W_lo.double()
    return F.linear(A.double(), W, p.bias.double())


def deinterleave(p):
    """GEMM column blk*32 + half*16 + i holds row half*(N/2) + blk*16 + i of the plain [value | gate] weight."""
    idx = torch.arange(p.N)
    dst = ((idx % 32) // 16) * (p.N // 2) + (idx // 32) * 16 + (idx % 16)
    W, b = torch.empty_like(p.W), torch.empty_like(p.bias)
    W[dst], b[dst] = p.W, p.bias
    return W, b


@pytest.mark.parametrize("wdt", ["bf16", "fp16"])
@pytest.mark.parametrize("a32", [False, True])
def test_reference_agrees_with_torch(wdt, a32):
    eq = lambda a, b: torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12)
    for shape in (R.SHAPE_MAIN, R.SHAPE_ONE, R.SHAPE_KG, R.SHAPE_PAIR):
        for epi, f in (("bias", lambda x: x), ("silu", F.silu), ("relu", torch.relu)):
            p = R.problem(shape, wdt, epi, a32)
            eq(R.evaluate(p).out, f(lin(p)))
    p = R.problem(R.SHAPE_MAIN, wdt, "res", a32)
    eq(R.evaluate(p).out, p.residual.double() + 0.5 * lin(p))
    p = R.problem(R.SHAPE_MAIN, wdt, "mask0_res", a32)
    eq(R.evaluate(p).out, p.residual.double() + 0.5 * lin(p).masked_fill(p.row_mask[:, None] == 0, 0.0))
    p = R.problem(R.SHAPE_MAIN, wdt, "mask1", a32)
    A = p.A.to(p.W.dtype).double().masked_fill(p.row_mask[:, None] == 0, 0.0)
    eq(R.evaluate(p).out, F.linear(A, p.W.double(), p.bias.double()))
    # GLU on de-interleaved weights; C_pre holds the interleaved pre-activation
    p = R.problem(R.SHAPE_GLU, wdt, "pre_glu", a32)
    W, b = deinterleave(p)
    r = R.evaluate(p)
    eq(r.out, F.glu(F.linear(p.A.to(p.W.dtype).double(), W.double(), b.double()), dim=1))
    eq(r.pre, lin(p))
    # the backward epilogues against autograd
    for epi, f in (("dsilu", F.silu), ("drelu", torch.relu)):
        p = R.problem(R.SHAPE_MAIN, wdt, epi, a32)
        z = p.aux.double().requires_grad_(True)
        (gz,) = torch.autograd.grad(f(z), z, lin(p))
        if epi == "drelu":                       # aux is the forward OUTPUT there: relu(z) > 0 exactly where z > 0
            assert bool(((p.aux > 0) == (z > 0)).all())
        eq(R.evaluate(p).out, 0.5 * gz)
    # dropout: kept elements scaled, the rest exactly zero, about p of them
    p = R.problem(R.SHAPE_MAIN, wdt, "drop", a32)
    k = R.keep_mask(p.M * p.N, *R.DROP).reshape(p.M, p.N)
    eq(R.evaluate(p).out, torch.where(k, F.silu(lin(p)) * R.drop_scale(R.DROP[0]), torch.zeros((), dtype=D)))
    assert abs(float((~k).double().mean()) - R.DROP[0]) < 0.02
    # ragged rows
    p = R.problem(R.SHAPE_RAGGED, wdt, "row_len", a32)
    W, b = deinterleave(p)
    t = torch.arange(p.M) % R.ROW_T
    dead = t >= torch.tensor(R.ROW_LEN).repeat_interleave(R.ROW_T)
    eq(R.evaluate(p).out, F.glu(F.linear(p.A.to(p.W.dtype).double(), W.double(), b.double()), dim=1).masked_fill(dead[:, None], 0.0))


@pytest.mark.parametrize("conv", R.CONVS)
def test_reference_conv_agrees_with_conv2d(conv):
    B, T1, F1, C, N = conv
    for split in (False, True):
        p = R.problem(R.conv_shape(conv), "bf16", "relu", split, False, False, split, conv)
        W = (p.W.double() if not split else p.W.double() + p.W_lo.double()).reshape(N, 3, 3, C).permute(0, 3, 1, 2)
        img = p.A.double().permute(0, 3, 1, 2)
        ref = torch.relu(F.conv2d(img, W, p.bias.double(), stride=2)).permute(0, 2, 3, 1).reshape(p.M, N)
        torch.testing.assert_close(R.evaluate(p).out, ref, rtol=1e-12, atol=1e-12)


def test_split_reference_is_the_unrounded_product():
    p = R.problem(R.SHAPE_MAIN, "bf16", "bias", True, False, False, True)
    torch.testing.assert_close(R.evaluate(p).out, F.linear(p.A.double(), p.W.double() + p.W_lo.double(), p.bias.double()), rtol=1e-12, atol=1e-12)


def test_yardstick_and_bound():
    g, gs, t, ts = R.measure_g()
    print("float32 torch worst |d|/S: %.3g (split formula %.3g) -> g = %.3g, g_split = %.3g" % (t, ts, g, gs))
    assert 0 < t < 2.0 ** -20 and 0 < ts < 2.0 ** -12      # float32 accumulation; the three-product formula drops A_lo.W_lo


def differs(a, b):
    nan = torch.isnan(a) != torch.isnan(b)
    d = torch.nan_to_num((a - b).abs(), nan=0.0, posinf=float("inf"))
    return torch.where(nan, torch.full_like(d, float("inf")), d)


def test_every_wrong_variant_is_separated():
    g = R.measure_g()[0]
    rows = []
    for name, key in R.VARIANTS.items():
        if key == "poisoned relu":
            p = R.poisoned((R.SHAPE_MAIN, "fp16", "relu", False, True))[0]
        else:
            p = R.problem(*key)
        right, wrong = R.evaluate(p), R.evaluate(p, variant=name)
        worst = float((differs(right.out, wrong.out) / (g * right.S)).max())
        if right.pre is not None:
            worst = max(worst, float((differs(right.pre, wrong.pre) / (g * right.S_pre)).max()))
        rows.append((name, getattr(p, "epi", "?"), worst))
    print("\n%-28s %-12s %s" % ("variant", "epilogue", "worst |wrong - right| / bound"))
    for r in rows:
        print("%-28s %-12s %.3g" % r)
    for name, _, worst in rows:
        assert worst > 10.0, "%s is not separated at these inputs: %.3g x the bound" % (name, worst)
