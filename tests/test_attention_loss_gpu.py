"""GPU: the label-smoothing loss kernels of csrc/lsm.hip through the C entry (every operand between guard bands, every output NaN-prefilled:
tests/extent.py) against the float64 restatement of tests/attention_loss_ref.py, whose docstring derives every bound used here from the number
formats; then the autograd nodes and label_smoothing_loss.LabelSmoothingLoss (against the reference's own recorded results), and the ReLU
feed-forward's hidden dropout in the backward epilogue of cfm_gemm.

The module-level gates are MOD_TOL of tests/test_train_modules_gpu.py with that file's relerr (the project's gate for one module's forward and
gradients)."""
import ctypes
import functools
import itertools

import pytest
import torch

import attention_loss_ref as R
import gemm_ref
from conftest import load_golden
from extent import Guards
from test_train_modules_gpu import MOD_TOL, relerr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
MODES = ["bf16", "fp16", "fp32"]


@pytest.fixture(scope="module")
def cfm():
    import cfm as c
    return c


@pytest.fixture
def precision():
    import cfm
    before = cfm.get_precision()
    yield cfm.set_precision
    cfm.set_precision(before)


# ----------------------------------------------------------------------------------------------------------------- cfm_lsm_loss / cfm_lsm_grad
KERNEL_CASES = list(itertools.product((1, 33, 130), (37, 5002), (64, 256, 512), ("bf16", "fp16")))
kernel_case = functools.lru_cache(maxsize=None)(R.kernel_case)          # computed once, shared, never written to


def run_loss(cfm, c, V, s, logits=None, ld=None, x=None):
    G = Guards()
    d = cfm.LsmLossDesc()
    M = c["target"].numel()
    tg = G.inp(c["target"], name="target")
    loss, lse = G.out((M,), name="loss"), G.out((M,), name="lse")
    if logits is None:
        x = c["x"] if x is None else x
        xv, wv, bv = G.inp(x, name="X"), G.inp(c["w"], name="W"), G.inp(c["bias"], name="bias")
        d.X, d.W, d.bias, d.ldx, d.D, d.x_dtype, d.w_dtype = cfm.ptr(xv), cfm.ptr(wv), cfm.ptr(bv), x.shape[1], x.shape[1], cfm.dt_code(xv), cfm.dt_code(wv)
    else:
        lv = G.inp(logits, ld=ld, name="logits")
        d.logits, d.ld = cfm.ptr(lv), ld
    d.target, d.loss, d.lse, d.M, d.V, d.smoothing = cfm.ptr(tg), cfm.ptr(loss), cfm.ptr(lse), M, V, s
    rc = cfm.lib().cfm_lsm_loss(ctypes.byref(d), cfm.stream())
    assert rc == 0, cfm.lib().cfm_last_error()
    torch.cuda.synchronize()
    G.check()
    return loss.cpu(), lse.cpu()


def run_grad(cfm, c, V, s, lse, out_dtype, logits=None, ld=None, ldz_pad=0):
    """dz through the C entry as [M, Vk] with rows Vk + ldz_pad apart: the gap columns, the bands and every input are checked for stray writes."""
    G = Guards()
    d = cfm.LsmGradDesc()
    M, Vk = c["target"].numel(), (V + 7) // 8 * 8
    tg, lv, gv = G.inp(c["target"], name="target"), G.inp(lse, name="lse"), G.inp(c["g"], name="g")
    dz = G.out((M, Vk), out_dtype, ld=Vk + ldz_pad, name="dz")
    if logits is None:
        xv, wv, bv = G.inp(c["x"], name="X"), G.inp(c["w"], name="W"), G.inp(c["bias"], name="bias")
        d.X, d.W, d.bias, d.ldx, d.D, d.x_dtype, d.w_dtype = cfm.ptr(xv), cfm.ptr(wv), cfm.ptr(bv), c["x"].shape[1], c["x"].shape[1], cfm.dt_code(xv), cfm.dt_code(wv)
    else:
        zv = G.inp(logits, ld=ld, name="logits")
        d.logits, d.ld = cfm.ptr(zv), ld
    d.target, d.lse, d.g, d.dz, d.ldz = cfm.ptr(tg), cfm.ptr(lv), cfm.ptr(gv), cfm.ptr(dz), Vk + ldz_pad
    d.M, d.V, d.Vk, d.dz_dtype, d.smoothing = M, V, Vk, cfm.dt_code(dz), s
    rc = cfm.lib().cfm_lsm_grad(ctypes.byref(d), cfm.stream())
    assert rc == 0, cfm.lib().cfm_last_error()
    torch.cuda.synchronize()
    G.check()
    return dz.cpu()


def padded_logits(z, ld):
    """f32 logits [M, ld]: the columns at and past V hold +1e30, so a kernel that reads them fails."""
    out = torch.full((z.shape[0], ld), 1e30)
    out[:, :z.shape[1]] = z.float()
    return out


@pytest.mark.parametrize("s", [0.0, 0.1])
@pytest.mark.parametrize("M,V,D,dt", KERNEL_CASES, ids=lambda v: str(v))
def test_lsm_kernels_against_float64(cfm, M, V, D, dt, s):
    c = kernel_case(M, V, D, dt)
    z, tgt, live = c["z"], c["target"], c["target"] >= 0
    ref = R.rows_closed(z, tgt, s)
    ref_lse = torch.where(live, torch.logsumexp(z, -1), torch.zeros(M, dtype=torch.float64))
    # ---- forward, fused
    bound = R.loss_bound(z, s, c["delta"])
    loss, lse = run_loss(cfm, c, V, s)
    err, err_lse = float((loss.double() - ref).abs().max()), float((lse.double() - ref_lse).abs().max())
    print("fused  M=%d V=%d D=%d %s s=%g: loss |err| %.3e, lse |err| %.3e (bound %.3e)" % (M, V, D, dt, s, err, err_lse, bound))
    assert err <= bound and err_lse <= bound
    assert bool((loss[~live] == 0).all()) and bool((lse[~live] == 0).all())
    again = run_loss(cfm, c, V, s)
    assert torch.equal(again[0], loss) and torch.equal(again[1], lse)                        # the same input, the same bits
    l32, _ = run_loss(cfm, c, V, s, x=c["x"].float())                                        # f32 X (already representable) is the same computation
    assert torch.equal(l32, loss)
    # ---- forward, logits form, at two row strides; against float64 on the f32 logits it is given, and against the fused form
    Vk = (V + 7) // 8 * 8
    z32 = z.float()
    ref_u = R.rows_closed(z32.double(), tgt, s)
    bound_u = R.loss_bound(z32.double(), s, 0.0)
    for ld in (V, Vk + 8):
        lu, lse_u = run_loss(cfm, c, V, s, logits=padded_logits(z32, ld), ld=ld)
        eu = float((lu.double() - ref_u).abs().max())
        assert eu <= bound_u, ("logits form", ld, eu, bound_u)
        assert float((lu.double() - loss.double()).abs().max()) <= bound + bound_u          # the two forms agree to f32 summation order
        assert bool((lu[~live] == 0).all()) and bool((lse_u[~live] == 0).all())
    print("logits M=%d V=%d s=%g: loss |err| %.3e (bound %.3e)" % (M, V, s, eu, bound_u))
    # ---- backward, fused: the float64 gradient at the float64 lse; the kernel is handed its own forward's lse
    gref = R.grad(z, tgt, s, c["g"])
    out_dt = R.DT[dt]
    gb = R.grad_bound(gref, c["g"], c["delta"] + bound, out_dt)                             # lse itself is off by at most the forward's bound
    for pad in (0, 12):
        dz = run_grad(cfm, c, V, s, lse, out_dt, ldz_pad=pad)
        assert bool((dz[:, V:] == 0).all()), "columns V..Vk of dz are not zero"
        assert bool((dz[~live] == 0).all())
        e = (dz[:, :V].double() - gref).abs()
        assert bool((e <= gb).all()), ("fused dz", pad, float((e / gb).max()))
    assert torch.equal(run_grad(cfm, c, V, s, lse, out_dt, ldz_pad=12), dz)
    print("fused  M=%d V=%d D=%d %s s=%g: dz worst |err| / bound %.3f" % (M, V, D, dt, s, float((e / gb).max())))
    # ---- backward, logits form, every output type
    gref_u = R.grad(z32.double(), tgt, s, c["g"])
    for odt in (torch.float32, out_dt):
        du = run_grad(cfm, c, V, s, lse_u, odt, logits=padded_logits(z32, Vk + 8), ld=Vk + 8, ldz_pad=4)
        assert bool((du[:, V:] == 0).all()) and bool((du[~live] == 0).all())
        eu = (du[:, :V].double() - gref_u).abs()
        gbu = R.grad_bound(gref_u, c["g"], bound_u, odt)
        assert bool((eu <= gbu).all()), ("logits dz", odt, float((eu / gbu).max()))
        assert bool(((du[:, :V].double() - dz[:, :V].double()).abs() <= gb + gbu).all())


@pytest.mark.parametrize("V,D,dt", [(37, 64, "bf16"), (5002, 256, "fp16")])
def test_lsm_kernels_with_every_row_ignored(cfm, V, D, dt):
    """One all-ignored call: zeros everywhere, and W / bias are not read (they hold NaN / 1e30 past V and NaN bands around)."""
    c = R.kernel_case(130, V, D, dt, dead=True)
    Vk = (V + 7) // 8 * 8
    loss, lse = run_loss(cfm, c, V, 0.1)
    assert bool((loss == 0).all()) and bool((lse == 0).all())
    assert bool((run_grad(cfm, c, V, 0.1, lse, R.DT[dt], ldz_pad=4) == 0).all())
    lu, lse_u = run_loss(cfm, c, V, 0.1, logits=padded_logits(c["z"], Vk), ld=Vk)
    assert bool((lu == 0).all()) and bool((lse_u == 0).all())
    assert bool((run_grad(cfm, c, V, 0.1, lse_u, torch.float32, logits=padded_logits(c["z"], Vk), ld=Vk) == 0).all())
    red = cfm.lsm_reduce(loss.to(DEV), c["target"].to(DEV), 0).cpu()
    assert red.tolist() == [0.0, 1.0]                                                        # no valid target: loss 0, not 0 / 0


@pytest.mark.parametrize("M", [1, 33, 130, 1000])
def test_lsm_reduce(cfm, M):
    gen = torch.Generator().manual_seed(M)
    loss = torch.rand(M, generator=gen) * 9.0
    target = torch.randint(-1, 5, (M,), generator=gen).to(torch.int32)
    loss[target < 0] = 0.0
    G = Guards()
    lv, tv, out = G.inp(loss, name="loss"), G.inp(target, name="target"), G.out((2,), name="out")
    for batch, denom in ((0, max(int((target >= 0).sum()), 1)), (7, 7)):
        rc = cfm.lib().cfm_lsm_reduce(cfm.ptr(lv), cfm.ptr(tv), M, batch, cfm.ptr(out), cfm.stream())
        assert rc == 0, cfm.lib().cfm_last_error()
        torch.cuda.synchronize()
        G.check()
        got = out.cpu()
        assert float(got[1]) == float(denom)
        want = float(loss.double().sum()) / denom
        assert abs(float(got[0]) - want) <= 2.0 ** -23 * 10 * max(want, 1.0)                 # a tree of M f32 adds: depth ~ log2(M) + M / 256
        assert torch.equal(cfm.lsm_reduce(lv, tv, batch).cpu(), got)


def test_lsm_host_validation(cfm):
    x = torch.randn(4, 16, device=DEV).bfloat16()
    w = torch.randn(8, 16, device=DEV).bfloat16()
    b = torch.zeros(8, device=DEV)
    t = torch.tensor([0, 1, -1, 4], dtype=torch.int32, device=DEV)
    loss, lse = cfm.lsm_loss(x, w, b, t, 5, 0.1)
    assert float(loss[2]) == 0.0 and float(lse[2]) == 0.0 and bool((loss[[0, 1, 3]] > 0).all())
    dz = cfm.lsm_grad(x, w, b, t, 5, 0.1, lse, torch.ones(4, device=DEV))
    assert dz.shape == (4, 8) and dz.dtype == torch.bfloat16 and bool((dz[:, 5:] == 0).all()) and bool((dz[2] == 0).all())
    assert float(dz[:, :5].float().sum(1).abs().max()) < 2e-2                                # softmax - q sums to 0 per row
    with pytest.raises(RuntimeError, match="multiple of 8"):
        cfm.lsm_loss(x[:, :12].contiguous(), w[:, :12].contiguous(), b, t, 5, 0.1)
    with pytest.raises(RuntimeError, match="bf16 or fp16"):
        cfm.lsm_loss(x.float(), w.float(), b, t, 5, 0.1)
    with pytest.raises(RuntimeError, match="smoothing"):
        cfm.lsm_loss(x, w, b, t, 5, 1.0)
    with pytest.raises(ValueError, match="int32"):
        cfm.lsm_loss(x, w, b, t.long(), 5, 0.1)
    assert bool(torch.isnan(cfm.lsm_loss(x, w, b, torch.tensor([7, 0, 0, 0], dtype=torch.int32, device=DEV), 5, 0.1)[0][0]))     # target >= V


# ------------------------------------------------------------------------------------------------------------------------- the autograd nodes
def test_label_smoothing_loss_module_against_the_reference(cfm):
    """label_smoothing_loss.LabelSmoothingLoss on the device against the REFERENCE's class run in float64 (tests/golden/label_smoothing.npz)."""
    from label_smoothing_loss import LabelSmoothingLoss
    arrays, meta = load_golden("label_smoothing")
    z, t = torch.from_numpy(arrays["logits"]), torch.from_numpy(arrays["target"])
    B, L, V = z.shape
    for c in meta["cases"]:
        zz = z.float().to(DEV).requires_grad_(True)
        loss = LabelSmoothingLoss(V, meta["padding_idx"], c["smoothing"], c["normalize_length"])(zz, t.to(DEV))
        (loss * 3.0).backward()
        want, gwant = float(arrays["loss_" + c["tag"]]), torch.from_numpy(arrays["grad_" + c["tag"]]) * 3.0
        bound = B * L * R.loss_bound(z.view(-1, V), c["smoothing"], 0.0) / R.denominator(t.view(-1), B, c["normalize_length"])
        assert abs(float(loss.detach()) - want) <= bound + 2.0 ** -21 * want, (c, float(loss.detach()), want)
        assert relerr(zz.grad.cpu(), gwant) <= MOD_TOL["fp32"][1], c
        loss2 = LabelSmoothingLoss(V, meta["padding_idx"], c["smoothing"], c["normalize_length"])(zz.detach(), t.to(DEV))
        assert torch.equal(loss2, loss.detach())


@pytest.mark.parametrize("mode,fused", [("bf16", False), ("bf16", True), ("fp16", False), ("fp16", True), ("fp32", False)])
@pytest.mark.parametrize("V,D,normalize_length", [(37, 64, False), (5002, 256, True)])
def test_lsm_loss_fn_projection_gradients(cfm, precision, mode, fused, V, D, normalize_length):
    """cfm.autograd.LsmLossFn: rows -> Linear -> loss.  The loss, d loss / d rows, dW and db against float64 on the weights as the mode rounds
    them (attention_decoder_ref.round_trip's rule: 16-bit modes round the weight, fp32 keeps it)."""
    from cfm import autograd as ag
    precision(mode)
    prec = cfm.resolve_precision()
    M, B, s = 33, 4, 0.1
    gen = torch.Generator().manual_seed(V + D)
    lin = torch.nn.Linear(D, V)
    with torch.no_grad():
        lin.weight.copy_(torch.randn(V, D, generator=gen) * D ** -0.5)
        lin.bias.copy_(torch.randn(V, generator=gen))
        if mode != "fp32":
            lin.weight.copy_(lin.weight.to(R.DT[mode]).float())
    rows = torch.randn(M, D, generator=gen)
    rows = rows if mode == "fp32" else rows.to(R.DT[mode]).float()
    target = torch.randint(0, V, (M,), generator=gen).to(torch.int32)
    target[2::5], target[0], target[1] = -1, 0, V - 1
    # float64
    rr, W, b = rows.double().requires_grad_(True), lin.weight.detach().double().requires_grad_(True), lin.bias.detach().double().requires_grad_(True)
    ref = R.loss(rr @ W.t() + b, target, s, B, normalize_length)
    ref.backward()
    # device
    lin = lin.to(DEV)
    xr = rows.to(DEV).requires_grad_(True)
    loss = ag.LsmLossFn.apply(xr, target.to(DEV), lin, prec, s, 0 if normalize_length else B, fused, lin.weight, lin.bias)
    loss.backward()
    ftol, gtol = MOD_TOL[mode]
    errs = dict(loss=abs(float(loss) - float(ref)) / abs(float(ref)), dx=relerr(xr.grad.cpu(), rr.grad), dW=relerr(lin.weight.grad.cpu(), W.grad),
                db=relerr(lin.bias.grad.cpu(), b.grad))
    print("LsmLossFn %s fused=%s V=%d D=%d: %s (gates %.1e / %.1e)" % (mode, fused, V, D, ", ".join("%s %.2e" % kv for kv in errs.items()), ftol, gtol))
    assert errs["loss"] <= ftol
    assert max(errs["dx"], errs["dW"], errs["db"]) <= gtol
    assert lin.weight.grad.shape == (V, D) and lin.bias.grad.shape == (V,)
    assert bool((xr.grad[target.to(DEV) < 0] == 0).all())
    # the same call again: the same bits
    lin.zero_grad()
    x2 = rows.to(DEV).requires_grad_(True)
    l2 = ag.LsmLossFn.apply(x2, target.to(DEV), lin, prec, s, 0 if normalize_length else B, fused, lin.weight, lin.bias)
    l2.backward()
    assert torch.equal(l2, loss.detach()) and torch.equal(x2.grad, xr.grad)


# ------------------------------------------------------------------------------------------------------- ReLU hidden dropout, backward epilogue
def relu_ffn(D, FF, M, seed):
    """A bare ReLU feed-forward (w_1, w_2) whose pre-activations stay >= 0.25 away from zero on its input (the biases of w_1 alternate
    +-(1.05 S + 0.25), S = the largest |x . w|, as relu_margin_ of the training tests): no rounding difference can flip a ReLU bit."""
    gen = torch.Generator().manual_seed(seed)
    mod = torch.nn.Module()
    mod.w_1, mod.w_2 = torch.nn.Linear(D, FF), torch.nn.Linear(FF, D)
    x = torch.randn(M, D, generator=gen)
    with torch.no_grad():
        mod.w_1.weight.copy_(torch.randn(FF, D, generator=gen) * D ** -0.5)
        mod.w_2.weight.copy_(torch.randn(D, FF, generator=gen) * FF ** -0.5)
        mod.w_2.bias.copy_(torch.randn(D, generator=gen))
        S = float((x @ mod.w_1.weight.t()).abs().max())
        mod.w_1.bias.copy_((1.05 * S + 0.25) * torch.tensor([1.0, -1.0]).repeat(FF // 2))
    return mod, x, torch.randn(M, D, generator=gen)


def ffn_float64(mod, x, dy, keep):
    """The bare module in float64 with the hidden keep mask (already scaled by 1 / (1 - p)) -> (y, dx, dW1, db1, dW2, db2)."""
    W1, b1, W2, b2 = (t.detach().double() for t in (mod.w_1.weight, mod.w_1.bias, mod.w_2.weight, mod.w_2.bias))
    xd, dyd = x.double(), dy.double()
    z = xd @ W1.t() + b1
    assert float(z.abs().min()) >= 0.25
    h = torch.relu(z) * keep
    dz = (dyd @ W2) * keep * (z > 0)
    return h @ W2.t() + b2, dz @ W1, dz.t() @ xd, dz.sum(0), dyd.t() @ h, dyd.sum(0)


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
def test_relu_ffn_hidden_dropout_backward(cfm, precision, p):
    """ffn_fwd / ffn_bwd(act=ACT_RELU, drop_h): the forward's mask on element row * FF + col, restated with gemm_ref.keep_mask, reaches the gradient
    in cfm_gemm's CFM_ACT_DRELU epilogue.  fp32 mode, the module gate."""
    from cfm import autograd as ag, packing
    precision("fp32")
    prec = cfm.resolve_precision()
    D, FF, M, seed = 64, 136, 37, 0x1234567
    mod, x, dy = relu_ffn(D, FF, M, 5)
    drop = (p, seed) if p > 0 else None
    keep = gemm_ref.keep_mask(M * FF, p, seed).view(M, FF).double() * gemm_ref.drop_scale(p) if p > 0 else torch.ones(M, FF, dtype=torch.float64)
    ref = ffn_float64(mod, x, dy, keep)
    mod = mod.to(DEV)
    pk = packing.pack_ffn_train(mod, prec)
    y, saved = ag.ffn_fwd(pk, x.to(DEV), None, prec, 1.0, act=cfm.ACT_RELU, drop_h=drop)
    dx, grads, _ = ag.ffn_bwd(pk, saved, dy.to(DEV), None, prec, 1.0, act=cfm.ACT_RELU, drop_h=drop)
    got = (y, dx, grads["w_1.weight"], grads["w_1.bias"], grads["w_2.weight"], grads["w_2.bias"])
    errs = [relerr(a.cpu(), b) for a, b in zip(got, ref)]
    print("relu ffn p=%g: y %.2e dx %.2e dW1 %.2e db1 %.2e dW2 %.2e db2 %.2e" % ((p,) + tuple(errs)))
    assert errs[0] <= MOD_TOL["fp32"][0] and max(errs[1:]) <= MOD_TOL["fp32"][1]
    if p > 0:                                                   # the mask matters: the dropout-free gradient is far from this one
        assert relerr(dx.cpu(), ffn_float64(mod.cpu(), x, dy, torch.ones(M, FF, dtype=torch.float64))[1]) > 0.05


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_drelu_epilogue_without_dropout_is_the_plain_product_masked(cfm, dt):
    """drop unset: the CFM_ACT_DRELU epilogue is acc where aux > 0 and 0 elsewhere -- bit for bit the plain epilogue's f32 output of the same
    product, masked (two code paths of one launch: the backward epilogue and the plain store).  That is what is pinned here; equality with the
    previous library's bits was checked once on the device when the epilogue changed and is not a committed test."""
    gen = torch.Generator().manual_seed(11)
    M, N, K = 130, 136, 64
    a = torch.randn(M, K, generator=gen).to(R.DT[dt]).to(DEV)
    w = (torch.randn(N, K, generator=gen) * K ** -0.5).to(R.DT[dt]).to(DEV)
    aux = torch.randn(M, N, generator=gen).to(DEV)
    plain = cfm.gemm(a, w, out_dtype=torch.float32)
    drelu = cfm.gemm(a, w, out_dtype=torch.float32, act=cfm.ACT_DRELU, aux=aux, alpha=1.0)
    assert torch.equal(drelu, torch.where(aux > 0, plain, torch.zeros_like(plain)))
    # with a mask it is that output times keep / (1 - p) on element row * N + col
    p, seed = 0.25, 77
    keep = gemm_ref.keep_mask(M * N, p, seed).view(M, N).to(DEV)
    dropped = cfm.gemm(a, w, out_dtype=torch.float32, act=cfm.ACT_DRELU, aux=aux, alpha=1.0, drop=(p, seed))
    want = torch.where(keep, drelu * gemm_ref.drop_scale(p), torch.zeros_like(drelu))
    assert torch.equal(dropped, want)


# ------------------------------------------------------------------------------------------------------------------ cross-attention sub-block
def src_attn_float64(mod, ln, x, mem, klens, dy, H):
    """x + SrcAttn(LN(x), mem, mem) in float64 and, for the cotangent dy, the gradients: (y, {name: grad})."""
    B, Tq, D = x.shape
    P = {"a." + n: q.detach().double().requires_grad_(True) for n, q in mod.named_parameters()}
    P["n.weight"], P["n.bias"] = (t.detach().double().requires_grad_(True) for t in ln)
    xd, md = x.double().requires_grad_(True), mem.double().requires_grad_(True)
    mask = (torch.arange(mem.shape[1]).unsqueeze(0) < torch.tensor(klens).unsqueeze(1)).unsqueeze(1).expand(-1, Tq, -1)
    y = xd + R._mha(P, "a", R.ADR._ln(P, "n", xd), md, mask, H, None, None, None)
    names = list(P)
    gs = torch.autograd.grad(y, [xd, md] + [P[n] for n in names], dy.double())
    out = {"dx": gs[0], "dmemory": gs[1]}
    out.update({n: g for n, g in zip(names, gs[2:])})
    return y.detach(), out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("D", [256, 64])
@pytest.mark.parametrize("Tq,Tk", [(1, 5), (8, 19), (8, 5), (1, 19)])
def test_src_attn_sub_block(cfm, precision, mode, D, Tq, Tk):
    """src_attn_fwd / src_attn_bwd alone: B = 3, ragged key lengths with a length of 1, d_k = 64 (the fast kernels) and d_k = 16 (the general ones)."""
    from attention import MultiHeadSelfAttentionModule
    from cfm import autograd as ag, packing
    precision(mode)
    prec = cfm.resolve_precision()
    B, H = 3, 4
    torch.manual_seed(D + Tq * 31 + Tk)
    mod = MultiHeadSelfAttentionModule(D, H, 0.0)
    ln = (torch.randn(D) * 0.1 + 1.0, torch.randn(D) * 0.1)
    x, mem, dy = torch.randn(B, Tq, D), torch.randn(B, Tk, D), torch.randn(B, Tq, D)
    if mode != "fp32":
        mem = mem.to(R.DT[mode]).float()                        # the sub-block takes the memory in the activation type
    klens = [Tk, max(1, Tk - 2), 1]
    y_ref, g_ref = src_attn_float64(mod, ln, x, mem, klens, dy, H)
    mod = mod.to(DEV)
    lnd = tuple(t.to(DEV) for t in ln)
    pk = packing.pack_src_attn_train(mod, prec)
    mask8 = cfm.as_u8_mask((torch.arange(Tk).unsqueeze(0) < torch.tensor(klens).unsqueeze(1)).unsqueeze(1).to(DEV))
    memd = mem.to(DEV).reshape(B * Tk, D).to(prec.act_dtype).contiguous()
    y, saved = ag.src_attn_fwd(mod, pk, x.to(DEV).reshape(B * Tq, D).contiguous(), memd, lnd, B, Tq, Tk, mask8, prec)
    prior = torch.randn(B * Tk, D, generator=torch.Generator().manual_seed(1)).to(DEV)
    dmem = prior.clone()
    dx, grads, (dg, db) = ag.src_attn_bwd(mod, pk, saved, dy.to(DEV).reshape(B * Tq, D).contiguous(), lnd, B, Tq, Tk, mask8, prec, dmem)
    ftol, gtol = MOD_TOL[mode]
    got = {"dx": dx.view(B, Tq, D), "dmemory": (dmem - prior).view(B, Tk, D), "n.weight": dg, "n.bias": db}
    got.update({"a." + n: g for n, g in grads.items()})
    floor = 1e-2 * max(float(v.abs().max()) for v in g_ref.values())
    errs = {n: float((got[n].cpu().double() - g_ref[n]).abs().max()) / max(float(g_ref[n].abs().max()), floor) for n in g_ref}
    e_out = relerr(y.view(B, Tq, D).cpu(), y_ref)
    print("src_attn %s D=%d Tq=%d Tk=%d: out %.2e, worst grad %.2e (%s), dmemory %.2e" % (mode, D, Tq, Tk, e_out, max(errs.values()), max(errs, key=errs.get), errs["dmemory"]))
    assert e_out <= ftol
    assert max(errs.values()) <= gtol, sorted(errs.items(), key=lambda kv: -kv[1])[:4]
    assert float(grads["linear_k.bias"].abs().max()) == 0.0    # constant along every softmax row: exactly zero, and returned as such


# ------------------------------------------------------------------------------------------------------------------------ the whole decoder
_REF = {}


def decoder_reference(T, rw):
    if (T, rw) not in _REF:
        _REF[(T, rw)] = R.attention_loss_reference(*R.decoder_case(T), rw)
    return _REF[(T, rw)]


def run_attention_loss(cfm, dec, memory, enc_lens, labels, lengths, rw):
    import decoder
    dec.zero_grad()
    crit = decoder.AttentionLoss(dec, lsm_weight=R.DEC["lsm"], reverse_weight=rw)
    mem = memory.to(DEV).requires_grad_(True)
    T = memory.shape[1]
    mask = (torch.arange(T).unsqueeze(0) < torch.tensor(enc_lens).unsqueeze(1)).unsqueeze(1).to(DEV)
    loss, left, right = crit(mem, mask, labels.to(DEV), torch.tensor(lengths, device=DEV))
    loss.backward()
    got = {"memory": mem.grad.cpu()}
    got.update({n: q.grad.cpu() for n, q in dec.named_parameters() if q.grad is not None})
    return loss.detach(), left.detach(), right.detach(), got


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("rw", [0.0, 0.3])
@pytest.mark.parametrize("T", [5, 19])
def test_whole_decoder_loss_and_gradients(cfm, precision, mode, rw, T):
    """decoder.AttentionLoss on a BiTransformerDecoder, dropout 0: the loss, d loss / d encoder_out and every parameter's gradient against float64.
    Gate: 4 x the yardstick of the same case (attention_loss_ref.decoder_yardstick)."""
    precision(mode)
    dec, memory, enc_lens, labels, lengths = R.decoder_case(T)
    l_ref, g_ref, zmin = decoder_reference(T, rw)
    assert zmin >= 0.25, zmin
    yl, ym, yp = R.decoder_yardstick(mode, T, rw)
    loss, left, right, got = run_attention_loss(cfm, dec.to(DEV), memory, enc_lens, labels, lengths, rw)
    assert set(got) == set(g_ref), set(got) ^ set(g_ref)
    em, ep, per = R.grad_metrics(got, g_ref)
    el = abs(float(loss) - float(l_ref))
    print("decoder %s T=%d rw=%g: loss %.2e (yardstick %.2e), dmemory %.2e (%.2e), parameters %.2e (%.2e) worst %s"
          % (mode, T, rw, el, yl, em, ym, ep, yp, max((n for n in per if n != "memory"), key=per.get)))
    assert abs(float(loss) - float((1 - rw) * left + rw * right)) <= 1e-6 * abs(float(loss))
    assert el <= 4 * yl and em <= 4 * ym and ep <= 4 * yp
    # eval mode: the same value, no gradient
    import decoder
    dec.eval()
    with torch.no_grad():
        T_ = memory.shape[1]
        mask = (torch.arange(T_).unsqueeze(0) < torch.tensor(enc_lens).unsqueeze(1)).unsqueeze(1).to(DEV)
        ev = decoder.AttentionLoss(dec, lsm_weight=R.DEC["lsm"], reverse_weight=rw)(memory.to(DEV), mask, labels.to(DEV), torch.tensor(lengths, device=DEV))[0]
    assert torch.equal(ev, loss)


def test_decoder_dropout_all_sites(cfm, precision):
    """Every site at p = 0.1, fp32 mode: the loss and the gradients equal the restatement fed the restated masks, under the dropout-free fp32 gate;
    one seed twice gives the same bits, another seed does not."""
    from cfm import autograd as ag
    precision("fp32")
    T, rw, p = 19, 0.3, 0.1
    dec, memory, enc_lens, labels, lengths = R.decoder_case(T, p)
    torch.manual_seed(123)
    seeds = (ag.draw_seed(), ag.draw_seed())
    drops = dict(pos=p, self_a=p, src_a=p, out=p, hidden=p)
    l_ref, g_ref, zmin = R.attention_loss_reference(dec, memory, enc_lens, labels, lengths, rw, drops=drops, seeds=seeds)
    yl, ym, yp = R.decoder_yardstick("fp32", T, rw)
    dec = dec.to(DEV)
    torch.manual_seed(123)
    loss, _, _, got = run_attention_loss(cfm, dec, memory, enc_lens, labels, lengths, rw)
    em, ep, per = R.grad_metrics(got, g_ref)
    el = abs(float(loss) - float(l_ref))
    print("decoder dropout fp32: loss %.2e (gate %.2e), dmemory %.2e (%.2e), parameters %.2e (%.2e)" % (el, 4 * yl, em, 4 * ym, ep, 4 * yp))
    assert el <= 4 * yl and em <= 4 * ym and ep <= 4 * yp
    torch.manual_seed(123)
    loss2, _, _, got2 = run_attention_loss(cfm, dec, memory, enc_lens, labels, lengths, rw)
    assert torch.equal(loss2, loss) and all(torch.equal(got2[n], got[n]) for n in got)
    torch.manual_seed(124)
    loss3, _, _, got3 = run_attention_loss(cfm, dec, memory, enc_lens, labels, lengths, rw)
    assert not torch.equal(loss3, loss) and not torch.equal(got3["memory"], got["memory"])


# ----------------------------------------------------------------------------------------------------------------------------- the objective
def build_objective(attention_weight):
    import decoder
    import encoder
    import joint
    import predictor
    import synth
    import transducer
    V = 37
    cfg = dict(input_dim=80, kernel_size=15, encoder_dim=144, dropout=0.0, attention_dropout=0.0, pos_enc_dropout=0.0, hidden_dim=576, num_heads=4,
               encoder_num_layers=2, max_len=5000, use_relative=True)
    enc = synth.load_synth_(encoder.ConformerEncoder(cmvn=None, **cfg), 13)
    ctc = synth.load_synth_(decoder.CTCDecoder(V, 144, 0.0), 14)
    torch.manual_seed(15)
    pr = predictor.RNNPredictor(V, 16, 24, 32, 0.0, 1, dropout=0.0)
    jn = joint.TransducerJoint(V, 144, 24, 48)
    att = decoder.BiTransformerDecoder(V, 144, 4, 288, 1, 1, 0.0, 0.0, 0.0, 0.0)
    obj = transducer.TransducerObjective(enc, pr, jn, ctc, blank=0, ignore_id=-1, ctc_weight=0.2, transducer_weight=0.8, attention=att,
                                         attention_weight=attention_weight, lsm_weight=0.1, reverse_weight=0.3)
    return obj.to(DEV).train()


def objective_batch(seed, T, lens):
    import numpy as np
    import synth
    x = torch.from_numpy(synth.fbank(seed, 2, T)).to(DEV)
    lab = torch.from_numpy(np.random.RandomState(seed).randint(1, 36, size=(2, 3))).to(DEV)
    return (None, x, torch.tensor(lens, dtype=torch.int32, device=DEV), lab, torch.full((2,), 3, dtype=torch.int64, device=DEV), None)


def test_objective_with_attention_term(cfm, precision):
    precision("fp32")
    cfm.set_deterministic(True)
    try:
        obj = build_objective(0.15)
        b = objective_batch(61, 120, [120, 97])
        out = obj(b)
        parts = 0.2 * out["loss_ctc"] + 0.8 * out["loss_rnnt"] + 0.15 * out["loss_attn"]
        assert abs(float(out["loss"]) - float(parts)) <= 1e-6 * abs(float(parts)) and float(out["loss_attn"]) > 0
        # encoder gradients: the sum of the three heads' taken separately
        def head(k):                                            # a forward of its own per head: the joint's node frees its state in its backward
            o = obj(b)
            return torch.autograd.grad(o[k], o["encoder_out"])[0]
        heads = [head(k) for k in ("loss_ctc", "loss_rnnt", "loss_attn")]
        total = head("loss")
        want = 0.2 * heads[0] + 0.8 * heads[1] + 0.15 * heads[2]
        assert relerr(total, want) <= 1e-5 and float(heads[2].abs().max()) > 0
        # forward_window entries equal forward per micro-batch at dropout 0
        mbs = [b, objective_batch(62, 100, [100, 64])]
        win = obj.forward_window(mbs)
        for g, mb in enumerate(mbs):
            one = obj(mb)["loss"]
            assert abs(float(win[g]) - float(one)) <= 2e-5 * abs(float(one)), (g, float(win[g]), float(one))
    finally:
        cfm.set_deterministic(False)


def test_objective_trainer_step_lowers_the_loss(cfm, precision):
    import trainer as T
    precision("fp32")
    obj = build_objective(0.15)
    b = objective_batch(61, 120, [120, 97])
    mods = [obj.encoder, obj.ctc, obj.predictor, obj.joint, obj.attention_loss.decoder]
    tr = T.DataParallelTrainer(mods, lambda mb: obj(mb)["loss"], lr=2e-3, warmup_steps=1, accum_grad=1)
    before = float(obj(b)["loss"].detach())
    tr.step([b])
    after = float(obj(b)["loss"].detach())
    print("objective: loss %.4f -> %.4f after one optimiser step" % (before, after))
    assert after < before
