"""MI355X: the RNN-T loss (rnnt.rnnt_loss, csrc/rnnt.hip) and the fused joint + loss (TransducerJoint.rnnt_loss) against the float64 reference of
tests/rnnt_ref.py -- loss, logits gradient, alpha / beta consistency, determinism, the three precision modes, the model.py:95-113 wiring and
the config-4 size (B 16, T' 249, U 40, J 512, V 5002)."""
import copy

import numpy as np
import pytest
import torch

import rnnt_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
# fused joint + loss against the float64 chain, max|d| / max|ref| over the loss and the eight gradients, ~3x the measured worst
FUSED_TOL = {"fp32": 3e-5, "fp16": 2e-3, "bf16": 1.5e-2}      # measured 9.6e-6 / 7.0e-4 / 5.4e-3 (enc_ffn.weight in each mode)
# config 4 (bf16), d enc_out / d pred_out of a sampled utterance: d pred_out sums 249 frames of bf16 products
CONFIG4_TOL = 4e-2                                            # measured 6.2e-3 / 1.5e-2 (utterance 0)
MODES = ["bf16", "fp16", "fp32"]


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    mod = g._import_package()
    yield mod
    mod.cfm.set_precision("bf16")


def relerr(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def lattice(seed, B, T, U, V, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn((B, T, U + 1, V), generator=g) * scale
    targets = torch.randint(1, V, (B, U), generator=g, dtype=torch.int32)
    tl = torch.tensor([T] + [max(1, T - 3 * i) for i in range(1, B)], dtype=torch.int32)
    ul = torch.tensor([U] + [max(0, U - 2 * i) for i in range(1, B)], dtype=torch.int32)
    if B > 2:
        ul[2] = 0                                                  # an utterance with no labels
    return logits, targets, tl, ul


def check_zero_outside(grad, tl, ul):
    for b in range(grad.shape[0]):
        for outside in (grad[b, int(tl[b]):], grad[b, :, int(ul[b]) + 1:]):
            assert outside.numel() == 0 or float(outside.abs().max()) == 0.0


CASES = [  # B, T, U, V, blank, reduction, clamp, dtype, pad columns (row stride V + pad)
    (4, 12, 5, 5002, 0, "mean", -1, torch.float32, 0),
    (3, 9, 4, 37, -1, "sum", -1, torch.float32, 0),
    (4, 10, 6, 5001, 0, "none", -1, torch.float32, 1),
    (3, 8, 3, 64, -1, "mean", 0.02, torch.float32, 0),
    (2, 6, 70, 33, 0, "sum", -1, torch.float32, 3),                # U+1 > 64: the columns span two wavefronts
    (3, 10, 4, 5002, 0, "mean", -1, torch.float16, 0),
    (3, 10, 4, 5001, -1, "sum", -1, torch.bfloat16, 1),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "B%d_T%d_U%d_V%d_b%d_%s_c%g_%s_pad%d" % (c[:7] + (str(c[7])[6:], c[8])))
def test_loss_and_logits_gradient_match_the_float64_reference(pkg, case):
    B, T, U, V, blank, reduction, clamp, dtype, pad = case
    logits, targets, tl, ul = lattice(B * 1000 + T * 10 + U, B, T, U, V)
    buf = torch.zeros((B, T, U + 1, V + pad), dtype=dtype, device=DEV)
    buf[..., :V] = logits.to(dtype)
    x = buf[..., :V].detach().requires_grad_(True)                 # pad > 0: a view with row stride V + pad, read in place
    loss = pkg.rnnt_loss(x, targets.to(DEV), tl.to(DEV), ul.to(DEV), blank=blank, clamp=clamp, reduction=reduction)
    gout = torch.linspace(0.5, 1.5, B, device=DEV) if reduction == "none" else torch.tensor(1.0, device=DEV)
    loss.backward(gout)
    rounded = buf[..., :V].detach().float().cpu()                  # the reference sees the same (16-bit rounded) values
    ref_loss, ref_grad, ref_costs = rnnt_ref.rnnt_loss_ref(rounded, targets, tl, ul, blank=blank, clamp=clamp, reduction=reduction)
    if reduction == "none":
        ref_grad = ref_grad * gout.cpu().double()[:, None, None, None]
    costs = pkg.rnnt_loss(buf[..., :V].detach(), targets.to(DEV), tl.to(DEV), ul.to(DEV), blank=blank, reduction="none")
    assert float(((costs.cpu().double() - ref_costs).abs() / ref_costs.abs()).max()) <= 2e-5
    assert relerr(loss.detach(), ref_loss) <= 2e-5
    g = x.grad
    assert g.dtype == dtype and g.shape == x.shape
    tol = {torch.float32: 5e-4, torch.float16: 1e-3, torch.bfloat16: 8e-3}[dtype]      # 16-bit: the gradient is returned in the logits' type
    assert relerr(g.float(), ref_grad) <= tol, relerr(g.float(), ref_grad)
    check_zero_outside(g.float(), tl, ul)
    assert torch.equal(buf[..., :V].detach().float().cpu(), rounded)                     # the caller's logits are left as they were


def test_gradient_pad_columns_in_place_and_16bit_over_f32(pkg):
    cfm = pkg.cfm
    B, T, U, V, ld = 3, 7, 4, 37, 40
    logits, targets, tl, ul = lattice(5, B, T, U, V)
    buf = torch.full((B, T, U + 1, ld), 7.0, device=DEV)
    buf[..., :V] = logits.to(DEV)
    args = (targets.to(DEV), tl.to(DEV), ul.to(DEV), 0)
    nll, st = cfm.rnnt_nll(buf, *args, V=V)
    out = torch.full_like(buf, 9.0)
    cfm.rnnt_grad(st, out, gscale=0.5)
    _, ref_grad, ref_costs = rnnt_ref.rnnt_loss_ref(logits, targets, tl, ul, blank=0, reduction="sum")
    assert relerr(nll, ref_costs) <= 2e-5
    assert float(out[..., V:].abs().max()) == 0.0                  # pad columns: exact zeros
    assert relerr(out[..., :V], 0.5 * ref_grad) <= 5e-4
    check_zero_outside(out, tl, ul)
    # in place over the logits (f32) and as bf16 in the first half of each f32 row: the same values
    inplace = buf.clone()
    _, st2 = cfm.rnnt_nll(inplace, *args, V=V)
    cfm.rnnt_grad(st2, inplace, gscale=0.5)
    assert torch.equal(inplace, out)
    half = buf.clone()
    _, st3 = cfm.rnnt_nll(half, *args, V=V)
    h = half.view(torch.bfloat16)
    cfm.rnnt_grad(st3, h, gscale=0.5, cols=ld)
    assert torch.equal(h[..., :ld].float(), out.to(torch.bfloat16).float())


def test_alpha_beta_consistency(pkg):
    cfm = pkg.cfm
    for U in (40, 90):
        logits, targets, tl, ul = lattice(11 + U, 4, 30, U, 129)
        nll, st = cfm.rnnt_nll(logits.to(DEV), targets.to(DEV), tl.to(DEV), ul.to(DEV), 0)
        # alpha'[T-1, U] + lp_blank' (the forward recursion's likelihood) equals beta'[0, 0] (the backward one's) up to f32 rounding
        assert float((st.ll_alpha + st.nll_shifted).abs().max()) <= 2e-5 * max(1.0, float(st.nll_shifted.abs().max()))
        assert float(st.alpha[:, 0, 0].abs().max()) == 0.0
        _, _, ref_costs = rnnt_ref.rnnt_loss_ref(logits, targets, tl, ul, blank=0, reduction="none")
        assert float(((nll.cpu().double() - ref_costs).abs() / ref_costs.abs()).max()) <= 2e-5


def test_determinism(pkg):
    logits, targets, tl, ul = lattice(3, 4, 20, 8, 5002)
    x = logits.to(DEV)
    outs = []
    for _ in range(2):
        xi = x.clone().requires_grad_(True)
        loss = pkg.rnnt_loss(xi, targets.to(DEV), tl.to(DEV), ul.to(DEV), blank=0)
        loss.backward()
        outs.append((loss.detach(), xi.grad))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_label_limit_is_an_error(pkg):
    x = torch.zeros((1, 2, 1025, 3), device=DEV)
    with pytest.raises(RuntimeError, match="exceeds 1024"):
        pkg.rnnt_loss(x, torch.ones((1, 1024), dtype=torch.int32, device=DEV), torch.tensor([2], device=DEV), torch.tensor([1024], device=DEV))


def joint_f64(jn, xe, xp):
    """The joint of joint.py:20-38 in float64 torch ops on the parameters of `jn` (a float64 copy)."""
    e = xe @ jn.enc_ffn.weight.t() + jn.enc_ffn.bias
    p = xp @ jn.pred_ffn.weight.t() + jn.pred_ffn.bias
    return torch.tanh(e.unsqueeze(2) + p.unsqueeze(1)) @ jn.ffn_out.weight.t() + jn.ffn_out.bias


def fused_vs_f64(pkg, mode, B=3, T=9, U=4, E=40, P=24, J=64, V=37, blank=0, reduction="mean"):
    import joint
    torch.manual_seed(7)
    jn = joint.TransducerJoint(V, E, P, J).to(DEV).train()
    jn.precision = mode
    xe = torch.randn(B, T, E, device=DEV, requires_grad=True)
    xp = torch.randn(B, U + 1, P, device=DEV, requires_grad=True)
    _, targets, tl, ul = lattice(B + T, B, T, U, V)
    loss = jn.rnnt_loss(xe, xp, targets.to(DEV), tl.to(DEV), ul.to(DEV), blank=blank, reduction=reduction)
    loss.backward()
    ref = copy.deepcopy(jn).cpu().double()
    re, rp = xe.detach().cpu().double().requires_grad_(True), xp.detach().cpu().double().requires_grad_(True)
    lb, ll = rnnt_ref.lattice_logprobs(joint_f64(ref, re, rp), targets, blank)
    costs = rnnt_ref.costs_from_lattice(lb, ll, tl, ul)
    rloss = costs.mean() if reduction == "mean" else costs.sum()
    rloss.backward()
    errs = {"loss": relerr(loss.detach(), rloss.detach()), "enc_out": relerr(xe.grad, re.grad), "pred_out": relerr(xp.grad, rp.grad)}
    for (n, p), (_, q) in zip(jn.named_parameters(), ref.named_parameters()):
        errs[n] = relerr(p.grad, q.grad)
    return errs


@pytest.mark.parametrize("mode", MODES)
def test_fused_joint_and_loss_match_the_float64_chain(pkg, mode):
    errs = fused_vs_f64(pkg, mode)
    print(mode, {k: "%.1e" % v for k, v in errs.items()})
    assert len(errs) == 9
    assert max(errs.values()) <= FUSED_TOL[mode], errs


def test_model_wiring_end_to_end(pkg):
    """Transducer.rnnt_loss (model.py:95-113): add_blank -> predictor (train mode, dropout 0) -> joint + loss -> backward; the predictor's
    gradients (through torch autograd from d pred_out) against the same chain in float64."""
    import joint
    import predictor
    import utils
    torch.manual_seed(3)
    B, T, U, V, E, blank, ignore_id = 3, 11, 5, 29, 48, 0, -1
    pr = predictor.RNNPredictor(V, 32, 40, 48, 0.0, 2, dropout=0.0).to(DEV).train()
    jn = joint.TransducerJoint(V, E, 40, 64).to(DEV).train()
    jn.precision = "fp32"
    enc = torch.randn(B, T, E, device=DEV, requires_grad=True)
    labels = torch.randint(1, V, (B, U), device=DEV)
    label_lengths = torch.tensor([U, 3, 1], device=DEV)
    for b in range(B):
        labels[b, int(label_lengths[b]):] = ignore_id
    enc_lens = torch.tensor([T, 8, 5], device=DEV, dtype=torch.int32)

    def chain(prm, jnm, enc_out, lab, run_joint):
        pad = utils.add_blank(lab, blank, ignore_id)
        pred = prm(pad)
        text = torch.where(lab == ignore_id, blank, lab).to(torch.int32)
        return run_joint(jnm, enc_out, pred, text)

    loss = chain(pr, jn, enc, labels, lambda j, e, p, y: j.rnnt_loss(e, p, y, enc_lens, label_lengths.to(torch.int32), blank=blank))
    loss.backward()
    pr64, jn64 = copy.deepcopy(pr).cpu().double(), copy.deepcopy(jn).cpu().double()
    enc64 = enc.detach().cpu().double().requires_grad_(True)

    def ref_joint(j, e, p, y):
        lb, ll = rnnt_ref.lattice_logprobs(joint_f64(j, e, p), y, blank)
        return rnnt_ref.costs_from_lattice(lb, ll, enc_lens.cpu(), label_lengths.cpu()).mean()

    rloss = chain(pr64, jn64, enc64, labels.cpu(), ref_joint)
    rloss.backward()
    assert relerr(loss.detach(), rloss.detach()) <= 1e-4
    assert relerr(enc.grad, enc64.grad) <= 1e-4
    for (n, p), (_, q) in zip(pr.named_parameters(), pr64.named_parameters()):
        assert relerr(p.grad, q.grad) <= 1e-4, n


def test_config4_size(pkg):
    """B 16, T' 249, U 40, J 512, V 5002: 817 M logits.  Fused forward + backward finishes with ONE logits-sized buffer; the loss matches the
    float64 lattice over the joint's own f32 logits; sampled utterances' input gradients match a float64 chain of that utterance alone."""
    import joint
    torch.manual_seed(5)
    B, T, U, E, P, J, V = 16, 249, 40, 512, 512, 512, 5002
    jn = joint.TransducerJoint(V, E, P, J).to(DEV).train()
    jn.precision = "bf16"
    xe = torch.randn(B, T, E, device=DEV)
    xp = torch.randn(B, U + 1, P, device=DEV)
    g = torch.Generator().manual_seed(9)
    targets = torch.randint(1, V, (B, U), generator=g, dtype=torch.int32)
    tl = torch.tensor([T - 7 * i for i in range(B)], dtype=torch.int32)
    ul = torch.tensor([U - 2 * i for i in range(B)], dtype=torch.int32)
    args = (targets.to(DEV), tl.to(DEV), ul.to(DEV))
    xe.requires_grad_(True)
    xp.requires_grad_(True)
    jn.rnnt_loss(xe[:1, :8], xp[:1, :3], args[0][:1, :2], torch.tensor([8], device=DEV), torch.tensor([2], device=DEV)).backward()   # warm the packs
    xe.grad = xp.grad = None
    jn.zero_grad()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    loss = jn.rnnt_loss(xe, xp, *args)
    loss.backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    logits_bytes = B * T * (U + 1) * V * 4
    assert torch.isfinite(loss)
    assert peak < 1.5 * logits_bytes, (peak, logits_bytes)         # one logits-sized buffer, not two
    # the loss: the float64 lattice (log-softmax by torch on the GPU) over the joint's own logits of the same mode
    with torch.no_grad():
        jn.eval()
        logits = jn(xe.detach(), xp.detach())
        jn.train()
        lb, ll = rnnt_ref.lattice_logprobs(logits, args[0], 0)
        del logits
        ref_costs = rnnt_ref.costs_from_lattice(lb, ll, args[1], args[2])
    print("config 4: loss %.6f, relative error %.1e, peak %.2f GB for %.2f GB of logits" % (float(loss), relerr(loss.detach(), ref_costs.mean()),
                                                                                          peak / 1e9, logits_bytes / 1e9))
    assert relerr(loss.detach(), ref_costs.mean()) <= 1e-4
    # sampled utterances: the whole chain of one utterance in float64 on the GPU
    ref = copy.deepcopy(jn).double()
    for b in (0, B - 1):
        re = xe[b:b + 1].detach().double().requires_grad_(True)
        rp = xp[b:b + 1].detach().double().requires_grad_(True)
        lb, ll = rnnt_ref.lattice_logprobs(joint_f64(ref, re, rp), args[0][b:b + 1], 0)
        (rnnt_ref.costs_from_lattice(lb, ll, args[1][b:b + 1], args[2][b:b + 1]).sum() / B).backward()
        errs = relerr(xe.grad[b], re.grad[0]), relerr(xp.grad[b], rp.grad[0])
        print("config 4, utterance %d: d enc_out %.1e, d pred_out %.1e" % (b, errs[0], errs[1]))
        assert max(errs) <= CONFIG4_TOL, (b, errs)
        del lb, ll, re, rp
