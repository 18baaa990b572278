"""GPU: the three kernels that end every training step -- cfm_sumsq, cfm_adam_step, cfm_adam_clip_step (csrc/train.hip) -- against the
float64 restatement of tests/adam_ref.py.

Inputs (adam_ref.adam_inputs): p of order 1, g log-uniform over 1e-10 .. 1e1 with a tenth exactly zero and a few denormals, non-zero
moments independent of g.  Cases (adam_ref.CASES): sizes 1, 2, 3, 4, 5, 1023, 4096*3 + 1 and BIG = 8192*256*4 + 4*256*3 + 3 (one full
sweep of the capped grid, a partial second sweep, a three-element tail), both beta pairs, eps 1e-8 / 1e-3, weight decay 0 / 1e-2, steps
1 / 2 / 1000 / 100000, with and without a device grad_scale -- not the cross product, but every value at a tail-only size (or 5) and at a
size with quads.  The reference runs at the betas as the C ABI receives them, rounded to float32 (adam_ref.abi_betas says why).

Quantities and bounds: adam_ref.adam_errors / adam_ref.BOUNDS (the measured figures stand beside the constants).  Each bound is 4 x what
float32 plain torch (ref_step_kernels.TorchStepKernels on float32 tensors) costs on the same cases against the same reference;
tests/test_adam_ref_cpu.py re-measures that on every run.

Mutation argument -- which case catches what (each claim is checked on the CPU, tests/test_adam_ref_cpu.py::test_each_mutation_exceeds_the_bounds,
by mutating the float32 torch restatement; figures are error / bound):
  weight decay dropped (`gv += pv * weight_decay`, and `+ p[i] * weight_decay` in the tail)
                                 n = 1023, wd = 1e-2, step 1: a tenth of g is exactly zero, there wd * p is the whole gradient.  m: 1.4e6 x
  `(1.f - b1)` dropped           the same case.  m: 1.2e7 x
  `(1.f - b2)` dropped           the same case.  v: 6.6e8 x
  bc1 dropped                    the same case, step 1: 1 / bc1 = 10.  dp: 5.9e5 x, p: 3.9 x
  bc2 dropped                    the same case, beta2 = 0.999 at step 1: 1 / sqrt(bc2) = 31.6.  dp: 2e7 x, p: 128 x
  eps inside the square root, or added before the division by sqrt(bc2)
                                 n = 1023, eps = 1e-3, step 1 from zero moments: sqrt(v) / sqrt(bc2) = |g| is below eps in most
                                 elements.  dp: 5.5e5 x, p: 4 x
  tail path dropped              every size with n & 3 != 0; at n = 1023 (255 quads + 3).  m: 1.3e6 x.  At n = 1, 2, 3 nothing else runs.
  tail twin of any of the above  sizes 1, 2, 3 hold weight decay, both eps, both beta pairs and steps 1, 2, 1000
  grid-stride wrap               BIG: elements 8 388 608 .. 8 391 679 belong to the second sweep; left alone they fail like a dropped tail
  clip branch                    a scale taken from the wrong side of the threshold is off by 5e-4 of g at "just_above" / "just_below"
                                 (m: ~700 x) and by 100 x at "above"; inv_world forgotten under an active clip is a factor 8
"""
import math

import pytest
import torch

import adam_ref as R
from extent import Guards
from ref_step_kernels import TorchStepKernels
from test_ops_gpu import cfm  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu

F32 = torch.float32
ERR_ARG = -1


inputs = R.inputs            # float32 CPU tensors (p, g, m, v), made once per (n, seed) and never written to


def on_device(old):
    return [t.cuda() for t in old]


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def within(e, what):
    print("%s: %s" % (what, "  ".join("%s=%.3g" % kv for kv in sorted(e.items()))))
    for k, b in R.BOUNDS.items():
        assert e[k] <= b, "%s: %s error %r over the bound %g" % (what, k, e[k], b)


def raw_clip_step(cfm, p, g, m, v, betas, eps, wd, step, sumsq, clip, inv_world, zero_grad, norm):
    opt = lambda t: None if t is None else t.data_ptr()
    return cfm.lib().cfm_adam_clip_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), R.LR, betas[0], betas[1], eps, wd, step,
                                        opt(sumsq), clip, inv_world, zero_grad, opt(norm), cfm.stream())


# ---------------------------------------------------------------------------------------------------------------- both Adam kernels
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_adam_kernels_match_float64_reference(cfm, case):
    """cfm_adam_step against adam_ref in p, m and v; g untouched.  cfm_adam_clip_step with the clip off and inv_world = the same scale:
    the two kernels share their arithmetic, so p, m, v agree BIT FOR BIT (which puts the clip kernel's body, tail and second sweep under
    the same bounds), with g untouched (zero_grad = 0) or exactly +0.0 in every element, tail included (zero_grad = 1)."""
    n, betas, eps, wd, step, gs, zero = case
    old = inputs(n, R.case_seed(case), zero)
    ab, s = R.abi_betas(betas), None if gs is None else R.f32(gs)
    p, g, m, v = on_device(old)
    cfm.adam_step(p, g, m, v, R.LR, betas, eps, wd, step, grad_scale=None if gs is None else torch.full((1,), gs, device="cuda"))
    within(R.adam_errors((p, m, v), old, R.LR, ab, eps, wd, step, s), "adam_step " + R.case_id(case))
    assert same_bits(g, old[1]), "adam_step wrote to g"
    ss = torch.full((1,), 9.0, device="cuda")
    for zero_grad in (0, 1):
        p2, g2, m2, v2 = on_device(old)
        norm = torch.full((1,), float("nan"), device="cuda")
        cfm.check(raw_clip_step(cfm, p2, g2, m2, v2, betas, eps, wd, step, ss, 0.0, 1.0 if s is None else s, zero_grad, norm), "cfm_adam_clip_step")
        for name, a, b in (("p", p2, p), ("m", m2, m), ("v", v2, v)):
            assert same_bits(a, b), "adam_clip_step (clip off, zero_grad = %d): %s differs from adam_step's" % (zero_grad, name)
        if zero_grad:
            assert int(bits(g2).count_nonzero()) == 0, "zero_grad = 1 left %d elements of g" % int(bits(g2).count_nonzero())
        else:
            assert same_bits(g2, old[1]), "zero_grad = 0 wrote to g"
        iw = 1.0 if s is None else s
        assert abs(float(norm) - 3.0 * iw) <= 3.0 * iw * 2.0 ** -23          # sqrt(9) * inv_world, one float32 spacing


# ---------------------------------------------------------------------------------------------------------------- the clip
def _clip_args():
    c = R.CLIP_CASE
    return c["betas"], R.abi_betas(c["betas"]), c["eps"], c["wd"], c["step"]


def _check_clip(cfm, what, old, bufs, factor, inv_world, zero_grad, norm):
    betas, ab, eps, wd, step = _clip_args()
    p, g, m, v, ss = bufs
    ss_val = R.planted_sumsq(factor, inv_world)
    cfm.check(raw_clip_step(cfm, p, g, m, v, betas, eps, wd, step, ss, R.CLIP, inv_world, zero_grad, norm), "cfm_adam_clip_step")
    norm_ref, scale_ref = R.clip_scale_ref(ss_val, R.CLIP, inv_world)
    assert (scale_ref < inv_world) == (factor > 1.0)                      # the planted norm lies on the side the case names
    within(R.adam_errors((p, m, v), old, R.LR, ab, eps, wd, step, scale_ref), what)
    if norm is not None:
        assert abs(float(norm) - norm_ref) <= norm_ref * 2.0 ** -23, (what, float(norm), norm_ref)      # one float32 spacing
    if zero_grad:
        assert int(bits(g).count_nonzero()) == 0
    else:
        assert same_bits(g, old[1])


@pytest.mark.parametrize("inv_world", R.CLIP_WORLDS)
@pytest.mark.parametrize("name,factor", R.CLIP_NORMS)
def test_clip_step_small(cfm, name, factor, inv_world):
    """n = 1023 between guard bands: the planted norm well above, well below and within 1e-3 of the clip on each side, inv_world 1 and
    1/8, norm_out given and NULL, zero_grad on and off."""
    old = inputs(1023, R.CLIP_SEED)
    for with_norm in (True, False):
        zero_grad = 1 if with_norm == (inv_world == 1.0) else 0
        G = Guards()
        p, g, m, v = (G.io(t, name=k) for t, k in zip(old, "pgmv"))
        ss = G.inp(torch.full((1,), R.planted_sumsq(factor, inv_world)), name="sumsq")
        norm = G.out((1,), F32, name="norm_out") if with_norm else None
        _check_clip(cfm, "clip n=1023 %s w=%g norm_out=%s" % (name, inv_world, with_norm), old, (p, g, m, v, ss), factor, inv_world, zero_grad, norm)
        G.check()


@pytest.mark.parametrize("name,inv_world", sorted(R.CLIP_BIG))
def test_clip_step_large(cfm, name, inv_world):
    """BIG: an active clip under inv_world = 1/8 with norm_out and zero_grad, and an inactive one just below the threshold without either"""
    old = inputs(R.BIG, R.case_seed(R.CASES[-1]))
    active = name == "above"
    p, g, m, v = on_device(old)
    ss = torch.full((1,), R.planted_sumsq(dict(R.CLIP_NORMS)[name], inv_world), device="cuda")
    norm = torch.full((1,), float("nan"), device="cuda") if active else None
    _check_clip(cfm, "clip n=BIG %s w=%g" % (name, inv_world), old, (p, g, m, v, ss), dict(R.CLIP_NORMS)[name], inv_world, 1 if active else 0, norm)


@pytest.mark.parametrize("with_sumsq", [True, False])
def test_clip_off_norm_out_follows_sumsq(cfm, with_sumsq):
    """clip = 0: the scale is inv_world whatever sumsq holds; norm_out is written when sumsq is given and left alone when it is NULL."""
    betas, ab, eps, wd, step = _clip_args()
    old = inputs(1023, R.CLIP_SEED)
    G = Guards()
    p, g, m, v = (G.io(t, name=k) for t, k in zip(old, "pgmv"))
    ss = G.inp(torch.full((1,), 1e6), name="sumsq") if with_sumsq else None           # a norm of 125: far over any clip, and ignored
    norm = G.out((1,), F32, name="norm_out")                                          # pre-filled with NaN
    cfm.check(raw_clip_step(cfm, p, g, m, v, betas, eps, wd, step, ss, 0.0, 0.125, 1, norm), "cfm_adam_clip_step")
    within(R.adam_errors((p, m, v), old, R.LR, ab, eps, wd, step, 0.125), "clip off, sumsq %s" % ("given" if with_sumsq else "NULL"))
    assert int(bits(g).count_nonzero()) == 0
    if with_sumsq:
        assert float(norm) == 125.0
    else:
        assert math.isnan(float(norm)), "norm_out written without a sumsq: %r" % float(norm)
    G.check()


def test_adam_clip_step_returns_none_without_sumsq(cfm):
    old = inputs(1023, R.CLIP_SEED)
    betas, ab, eps, wd, step = _clip_args()
    p, g, m, v = on_device(old)
    assert cfm.adam_clip_step(p, g, m, v, R.LR, betas, eps, wd, step, None, 0.0, 0.5) is None
    within(R.adam_errors((p, m, v), old, R.LR, ab, eps, wd, step, 0.5), "adam_clip_step(sumsq_t=None)")
    p, g, m, v = on_device(old)
    norm = cfm.adam_clip_step(p, g, m, v, R.LR, betas, eps, wd, step, torch.full((1,), 16.0, device="cuda"), 0.0, 0.5)
    assert float(norm) == 2.0
    import trainer
    p, g, m, v = on_device(old)
    assert trainer.HipStepKernels().adam_clip_step(p, g, m, v, R.LR, betas, eps, wd, step, 0.0, 0.5) is None


# ---------------------------------------------------------------------------------------------------------------- a non-finite norm
def _stand_in_step(old_dev, ss, clip, inv_world, betas, eps, wd, step):
    """ref_step_kernels.TorchStepKernels through the clip expression of trainer.DataParallelTrainer.finish(), on device tensors.  Callers
    hand it the betas as the kernels receive them (adam_ref.abi_betas): the stand-in is not behind a float ABI, and at the unrounded
    0.999 it runs an Adam whose 1 - beta2 is 1.3e-5 away -- the same algorithm at another hyper-parameter, not a rounding error."""
    p, g, m, v = old_dev
    norm = ss.sqrt() * inv_world
    scale = (clip / (norm + 1e-6)).clamp(max=1.0) * inv_world
    TorchStepKernels().adam_step(p, g, m, v, R.LR, betas, eps, wd, step, scale)
    return norm, scale


def test_nan_norm_poisons_the_step_as_torch_does(cfm):
    """A NaN sum of squares under an active clip: the scale is NaN (torch: (clip / (nan + 1e-6)).clamp(max=1.0); clip_grad_norm_ does the
    same), so p, m and v are NaN everywhere and norm_out is NaN -- in the kernel, body and tail, and in the stand-in the CPU trainer tests
    trust."""
    betas, ab, eps, wd, step = _clip_args()
    old = inputs(1023, R.CLIP_SEED)
    ss = torch.full((1,), float("nan"), device="cuda")
    p, g, m, v = on_device(old)
    norm = cfm.adam_clip_step(p, g, m, v, R.LR, betas, eps, wd, step, ss, R.CLIP, 1.0)
    assert math.isnan(float(norm))
    for name, t in (("p", p), ("m", m), ("v", v)):
        assert bool(torch.isnan(t).all()), "%s: %d of %d elements survived a NaN norm" % (name, int((~torch.isnan(t)).sum()), t.numel())
    assert int(bits(g).count_nonzero()) == 0
    tp, tg, tm, tv = on_device(old)
    tnorm, tscale = _stand_in_step((tp, tg, tm, tv), ss, R.CLIP, 1.0, ab, eps, wd, step)
    assert math.isnan(float(tnorm)) and math.isnan(float(tscale))
    assert all(bool(torch.isnan(t).all()) for t in (tp, tm, tv))
    # clip off: the norm is only logged, the step does not depend on it
    p, g, m, v = on_device(old)
    norm = cfm.adam_clip_step(p, g, m, v, R.LR, betas, eps, wd, step, ss, 0.0, 1.0)
    assert math.isnan(float(norm))
    within(R.adam_errors((p, m, v), old, R.LR, ab, eps, wd, step, 1.0), "NaN sumsq, clip off")


def test_inf_norm_gives_a_zero_scale(cfm):
    """An infinite sum of squares: scale = clip / inf = 0, finite gradients contribute nothing, the moments only decay (no weight decay
    here, so exactly m * beta1 and v * beta2) -- kernel and stand-in alike."""
    betas, ab, eps, _, step = _clip_args()
    old = inputs(1023, R.CLIP_SEED)
    ss = torch.full((1,), float("inf"), device="cuda")
    p, g, m, v = on_device(old)
    norm = cfm.adam_clip_step(p, g, m, v, R.LR, betas, eps, 0.0, step, ss, R.CLIP, 0.125)
    assert float(norm) == float("inf")
    assert R.clip_scale_ref(float("inf"), R.CLIP, 0.125)[1] == 0.0
    within(R.adam_errors((p, m, v), old, R.LR, ab, eps, 0.0, step, 0.0), "inf sumsq, kernel")
    assert torch.equal(m.cpu(), old[2] * ab[0]) and torch.equal(v.cpu(), old[3] * ab[1])
    tp, tg, tm, tv = on_device(old)
    tnorm, tscale = _stand_in_step((tp, tg, tm, tv), ss, R.CLIP, 0.125, ab, eps, 0.0, step)
    assert float(tnorm) == float("inf") and float(tscale) == 0.0
    within(R.adam_errors((tp, tm, tv), old, R.LR, ab, eps, 0.0, step, 0.0), "inf sumsq, stand-in")
    assert all(bool(torch.isfinite(t).all()) for t in (p, m, v, tp, tm, tv))


# ---------------------------------------------------------------------------------------------------------------- sum of squares
def test_sumsq_wraps_and_has_a_tail(cfm):
    """cfm.sumsq picks 1024 workgroups = 1 << 20 elements per sweep: a full sweep, five more quads per thread of the first blocks, 3 over"""
    n = (1 << 20) + 4096 * 5 + 3
    x = inputs(n, 3000)[1]
    ref = float((x.double() ** 2).sum())
    got = float(cfm.sumsq(x.cuda()))
    print("sumsq n=%d: relative error %.3g" % (n, abs(got - ref) / ref))
    assert abs(got - ref) <= 1e-5 * ref
    # the last three elements and the second sweep carry weight of their own
    y = torch.zeros(n)
    y[-1], y[1 << 20], y[n - 4] = 3.0, 4.0, 12.0
    assert float(cfm.sumsq(y.cuda())) == 169.0


@pytest.mark.parametrize("n_partials", [1, 7, 1024, 4096])
@pytest.mark.parametrize("n", [1, 3, 1023, 4096 * 3 + 1])
def test_sumsq_raw_any_number_of_partials(cfm, n, n_partials):
    """the C entry with 1 .. 4096 workgroups, whatever n: one block looping over everything, more blocks than quads (idle blocks still
    write their zero partial), partials an exact-size workspace between guard bands"""
    x = inputs(n, 3001 + n)[1]
    if n == 1:
        x = x + 3e-5                                                       # whatever the generator drew, not a zero
    ref = float((x.double() ** 2).sum())
    G = Guards()
    part, out = G.ws(n_partials, name="partials"), G.out((1,), F32, name="out")
    cfm.check(cfm.lib().cfm_sumsq(G.inp(x, name="x").data_ptr(), n, part.data_ptr(), n_partials, out.data_ptr(), cfm.stream()), "cfm_sumsq")
    assert abs(float(out) - ref) <= 1e-5 * ref, (float(out), ref)
    assert bool(torch.isfinite(part).all())                               # every partial written
    assert abs(float(part.double().sum()) - ref) <= 1e-5 * ref
    G.check()


# ---------------------------------------------------------------------------------------------------------------- the two interfaces
def test_hip_and_torch_step_kernels_agree(cfm):
    """trainer.HipStepKernels and the stand-in of the CPU trainer tests through the same calls -- sumsq, the clip expression of
    trainer.finish(), adam_step -- on one realistic case (n = 4096*3 + 1, weight decay, clip active): each within the bounds of the
    float64 reference, and the fused HipStepKernels.adam_clip_step (what the trainer really runs) as well."""
    import trainer
    n, betas, eps, wd, step, inv_world = 4096 * 3 + 1, R.BETAS_B, 1e-8, 1e-2, 7, 0.5
    ab = R.abi_betas(betas)
    old = inputs(n, 4000)
    norm_ref, scale_ref = R.clip_scale_ref(float((old[1].double() ** 2).sum()), R.CLIP, inv_world)
    assert scale_ref < 0.1 * inv_world                                    # the clip is active
    results = {}
    for name, K in (("hip", trainer.HipStepKernels()), ("torch", TorchStepKernels())):
        p, g, m, v = on_device(old)
        norm = K.sumsq(g).sqrt() * inv_world
        scale = (R.CLIP / (norm + 1e-6)).clamp(max=1.0) * inv_world
        K.adam_step(p, g, m, v, R.LR, ab, eps, wd, step, scale)               # both at the betas the C ABI can hold (_stand_in_step)
        assert abs(float(norm) - norm_ref) <= 1e-5 * norm_ref
        within(R.adam_errors((p, m, v), old, R.LR, ab, eps, wd, step, scale_ref), "interface %s" % name)
        assert same_bits(g, old[1])
        results[name] = (p, m, v)
    p, g, m, v = on_device(old)
    norm = trainer.HipStepKernels().adam_clip_step(p, g, m, v, R.LR, betas, eps, wd, step, R.CLIP, inv_world)
    assert abs(float(norm) - norm_ref) <= 1e-5 * norm_ref
    within(R.adam_errors((p, m, v), old, R.LR, ab, eps, wd, step, scale_ref), "interface hip fused")
    assert int(bits(g).count_nonzero()) == 0
    # the unfused and the fused HIP paths differ only in where the scale is computed
    for a, b in zip(results["hip"], (p, m, v)):
        assert float((a - b).abs().max()) <= 1e-6 * float(b.abs().max())


# ---------------------------------------------------------------------------------------------------------------- argument errors
def test_optimizer_entries_reject_bad_arguments(cfm):
    L = cfm.lib()
    p, g, m, v = on_device(inputs(5, 5000))
    before = [t.clone() for t in (p, g, m, v)]
    ss, part, out = torch.ones(1, device="cuda"), torch.zeros(4096, device="cuda"), torch.zeros(1, device="cuda")
    P = lambda t: t.data_ptr()

    def adam(n=5, step=1):
        return L.cfm_adam_step(P(p), P(g), P(m), P(v), n, R.LR, 0.9, 0.98, 1e-8, 0.0, step, None, cfm.stream())

    def clip(n=5, step=1, sumsq=ss, clip_val=0.0, inv_world=1.0):
        return L.cfm_adam_clip_step(P(p), P(g), P(m), P(v), n, R.LR, 0.9, 0.98, 1e-8, 0.0, step, None if sumsq is None else P(sumsq), clip_val, inv_world, 1,
                                    None, cfm.stream())

    def sumsq(n=5, nb=1):
        return L.cfm_sumsq(P(g), n, P(part), nb, P(out), cfm.stream())

    bad = [("cfm_adam_step", lambda: adam(step=0)), ("cfm_adam_step", lambda: adam(n=0)),
           ("cfm_adam_clip_step", lambda: clip(step=0)), ("cfm_adam_clip_step", lambda: clip(n=0)),
           ("cfm_adam_clip_step", lambda: clip(inv_world=0.0)), ("cfm_adam_clip_step", lambda: clip(inv_world=-1.0)),
           ("cfm_adam_clip_step", lambda: clip(sumsq=None, clip_val=4.0)),
           ("cfm_sumsq", lambda: sumsq(n=0)), ("cfm_sumsq", lambda: sumsq(nb=0)), ("cfm_sumsq", lambda: sumsq(nb=4097))]
    for i, (entry, call) in enumerate(bad):
        rc = call()
        msg = L.cfm_last_error().decode()
        assert rc == ERR_ARG and msg.startswith(entry + ":"), (i, entry, rc, msg)
    torch.cuda.synchronize()
    assert all(same_bits(a, b) for a, b in zip((p, g, m, v), before))      # a rejected call launched nothing
    with pytest.raises(RuntimeError, match="cfm_adam_clip_step"):
        cfm.adam_clip_step(p, g, m, v, R.LR, (0.9, 0.98), 1e-8, 0.0, 1, None, 4.0, 1.0)
    with pytest.raises(RuntimeError, match="cfm_adam_step"):
        cfm.adam_step(p, g, m, v, R.LR, (0.9, 0.98), 1e-8, 0.0, 0)
    assert adam() == 0 and clip() == 0 and sumsq() == 0 and sumsq(nb=4096) == 0
    torch.cuda.synchronize()
