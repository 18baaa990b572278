"""CPU: the float64 optimizer reference of tests/adam_ref.py against torch itself, and the figures the GPU bounds of
tests/test_optimizer_gpu.py are taken from.

  adam_ref / clip_scale_ref     against torch.optim.Adam on float64 parameters and torch.nn.utils.clip_grad_norm_
  float32 plain torch           (ref_step_kernels.TorchStepKernels on float32 tensors, the clip expression of trainer.finish() in float32)
                                run through every case of the GPU file: its error against adam_ref is what float32 arithmetic costs on
                                these inputs, and adam_ref.BOUNDS is 4 x that
  mutations                     of that float32 restatement: each term of the update dropped or misplaced exceeds the bounds at the case
                                the GPU file's docstring names
"""
import math

import pytest
import torch

import adam_ref as R
from ref_step_kernels import TorchStepKernels


# ---------------------------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("betas", [R.BETAS_A, R.BETAS_B])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_adam_ref_equals_torch_adam_float64(betas, wd):
    n = 257
    p0, _, _, _ = R.adam_inputs(n, 7)
    ref_p = torch.nn.Parameter(p0.double().clone())
    opt = torch.optim.Adam([ref_p], lr=R.LR, betas=betas, eps=1e-8, weight_decay=wd)
    p, m, v = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for step in range(1, 6):
        g = R.adam_inputs(n, 70 + step)[1].double()
        ref_p.grad = g * 0.37
        opt.step()
        p, m, v = R.adam_ref(p, g, m, v, R.LR, betas, 1e-8, wd, step, 0.37)
        st = opt.state[ref_p]
        # float64 against float64, the operations in another order: 1e-12 of the update (the update is ~lr) and of the moments
        assert float((p - ref_p.detach()).abs().max()) < 1e-12 * R.LR
        assert float(((m - st["exp_avg"]).abs() / st["exp_avg"].abs().clamp_min(1e-30)).max()) < 1e-12
        assert float(((v - st["exp_avg_sq"]).abs() / st["exp_avg_sq"].clamp_min(1e-30)).max()) < 1e-12
    assert float((p - p0.double()).abs().max()) > R.LR                    # five steps moved something


@pytest.mark.parametrize("inv_world", [1.0, 0.125])
@pytest.mark.parametrize("factor", [25.0, 0.04])                         # norm = factor * clip: above and below the threshold
def test_clip_scale_ref_equals_clip_grad_norm(factor, inv_world):
    g_sum = R.adam_inputs(1023, 8)[1].double()                            # what the ranks' all-reduce leaves: the SUM of their gradients
    g_sum = g_sum * (factor * R.CLIP / inv_world / float(g_sum.norm()))
    q = torch.nn.Parameter(torch.zeros_like(g_sum))
    q.grad = g_sum * inv_world                                            # the averaged gradient is what gets clipped
    total = torch.nn.utils.clip_grad_norm_([q], R.CLIP)
    norm, scale = R.clip_scale_ref(float((g_sum ** 2).sum()), R.CLIP, inv_world)
    assert abs(norm - float(total)) < 1e-12 * norm
    assert float((g_sum * scale - q.grad).abs().max()) < 1e-12 * float(q.grad.abs().max())
    assert (scale < inv_world) == (factor > 1.0)


def test_clip_scale_ref_edges():
    assert R.clip_scale_ref(9.0, 0.0, 0.125) == (0.375, 0.125)            # clip off: the averaging alone
    assert R.clip_scale_ref(9.0, -1.0, 1.0) == (3.0, 1.0)
    assert R.clip_scale_ref(9.0, None, 1.0) == (3.0, 1.0)
    norm, scale = R.clip_scale_ref(float("nan"), R.CLIP, 1.0)
    assert math.isnan(norm) and math.isnan(scale)                         # as (clip / (nan + 1e-6)).clamp(max=1.0) in torch
    norm, scale = R.clip_scale_ref(float("inf"), R.CLIP, 0.125)
    assert math.isinf(norm) and scale == 0.0
    norm, scale = R.clip_scale_ref(float("nan"), 0.0, 0.5)                # clip off: the norm is logged, the scale does not depend on it
    assert math.isnan(norm) and scale == 0.5


# ---------------------------------------------------------------------------------------------------------------- what float32 costs
def f32_step(old, lr, betas, eps, wd, step, scale, mutate=None):
    """ref_step_kernels.TorchStepKernels.adam_step on float32 clones (mutate = None: bit for bit, asserted below), with one term of the
    update dropped or misplaced on request.  Returns (p, m, v)."""
    p, g, m, v = (t.clone() for t in old)
    b1, b2 = betas
    gs = g if scale is None else g * scale
    if mutate != "no_wd":
        gs = gs + wd * p
    m.mul_(b1).add_(gs, alpha=1.0 if mutate == "no_1mb1" else 1 - b1)
    v.mul_(b2).addcmul_(gs, gs, value=1.0 if mutate == "no_1mb2" else 1 - b2)
    bc1 = 1.0 if mutate == "no_bc1" else 1 - b1 ** step
    bc2 = 1.0 if mutate == "no_bc2" else 1 - b2 ** step
    if mutate == "eps_in_sqrt":
        den = (v / bc2 + eps).sqrt()
    elif mutate == "eps_before_bc2":
        den = (v.sqrt() + eps) / bc2 ** 0.5
    else:
        den = v.sqrt() / bc2 ** 0.5 + eps
    p.sub_((lr / bc1) * m / den)
    if mutate == "no_tail" and p.numel() & 3:                             # the n & 3 elements after the last quad keep their old values
        k = p.numel() & 3
        for new, o in ((p, old[0]), (m, old[2]), (v, old[3])):
            new[-k:] = o[-k:]
    return p, m, v


def _case_run(c, mutate=None):
    n, betas, eps, wd, step, gs, zero = c
    old = R.inputs(n, R.case_seed(c), zero)
    betas = R.abi_betas(betas)
    s = None if gs is None else R.f32(gs)
    got = f32_step(old, R.LR, betas, eps, wd, step, None if s is None else torch.full((1,), s), mutate)
    return R.adam_errors(got, old, R.LR, betas, eps, wd, step, s)


def _clip_run(n, seed, factor, inv_world):
    """the stand-in's path through trainer.finish() in float32: clip expression, then adam_step with the scale it gives"""
    c = R.CLIP_CASE
    old = R.inputs(n, seed)
    ss = torch.full((1,), R.planted_sumsq(factor, inv_world))
    norm = ss.sqrt() * inv_world
    scale = (R.CLIP / (norm + 1e-6)).clamp(max=1.0) * inv_world
    betas = R.abi_betas(c["betas"])
    got = f32_step(old, R.LR, betas, c["eps"], c["wd"], c["step"], scale)
    _, s_ref = R.clip_scale_ref(float(ss), R.CLIP, inv_world)
    return R.adam_errors(got, old, R.LR, betas, c["eps"], c["wd"], c["step"], s_ref)


def test_f32_step_is_the_stand_in():
    for c in R.CASES[:-1]:
        n, betas, eps, wd, step, gs, zero = c
        old = R.adam_inputs(n, R.case_seed(c), zero)
        s = None if gs is None else torch.full((1,), gs)
        a = f32_step(old, R.LR, betas, eps, wd, step, s)
        p, g, m, v = (t.clone() for t in old)
        TorchStepKernels().adam_step(p, g, m, v, R.LR, betas, eps, wd, step, s)
        assert all(torch.equal(x, y) for x, y in zip(a, (p, m, v)))
        assert torch.equal(g, old[1])


def test_bounds_are_four_times_what_float32_torch_costs():
    """Every case of the GPU file through float32 plain torch: the worst error per quantity is R.F32_TORCH (to the two digits written there),
    and the bounds are 4 x that.  Prints the per-case figures (pytest -s)."""
    worst = dict(p=0.0, dp=0.0, m=0.0, v=0.0)
    for c in R.CASES:
        e = _case_run(c)
        print("%-48s %s" % (R.case_id(c), "  ".join("%s=%.3g" % kv for kv in e.items())))
        worst = {k: max(worst[k], e[k]) for k in worst}
    for n in (1023, R.BIG):
        for name, factor in R.CLIP_NORMS:
            for w in R.CLIP_WORLDS:
                if n == R.BIG and (name, w) not in R.CLIP_BIG:
                    continue
                e = _clip_run(n, R.case_seed(R.CASES[-1]) if n == R.BIG else R.CLIP_SEED, factor, w)
                print("%-48s %s" % ("clip-n%d-%s-w%g" % (n, name, w), "  ".join("%s=%.3g" % kv for kv in e.items())))
                worst = {k: max(worst[k], e[k]) for k in worst}
    print("worst", worst)
    for k in worst:
        # within a tenth of the constant: the inputs come out of pow(), whose last bit belongs to the maths library in use
        assert 0.9 * R.F32_TORCH[k] < worst[k] < 1.1 * R.F32_TORCH[k], (k, worst[k], R.F32_TORCH[k])
        assert R.BOUNDS[k] == 4 * R.F32_TORCH[k]


# mutation -> (the case of R.CASES at which it shows, the quantity that exceeds its bound): test_optimizer_gpu.py's docstring in code
MUTATIONS = {
    "no_wd": (7, "m"),                 # n = 1023, wd = 1e-2: a tenth of g is zero, there wd * p is ALL of the gradient
    "no_1mb1": (7, "m"),
    "no_1mb2": (7, "v"),
    "no_bc1": (7, "dp"),               # step 1: 1 / bc1 = 10
    "no_bc2": (7, "dp"),               # step 1, beta2 = 0.999: 1 / sqrt(bc2) = 31.6
    "eps_in_sqrt": (9, "dp"),          # eps = 1e-3, zero moments: sqrt(v) < eps in every element with |g| < 1e-2
    "eps_before_bc2": (9, "dp"),       # step 1: eps / sqrt(bc2) = 31.6 eps
    "no_tail": (7, "m"),               # 1023 = 255 quads + 3
}


@pytest.mark.parametrize("mutate", sorted(MUTATIONS))
def test_each_mutation_exceeds_the_bounds(mutate):
    idx, key = MUTATIONS[mutate]
    c = R.CASES[idx]
    clean, bad = _case_run(c), _case_run(c, mutate)
    assert all(clean[k] <= R.BOUNDS[k] for k in clean), clean
    assert bad[key] > 10 * R.BOUNDS[key], (mutate, key, bad)
    if key == "dp":                                                       # the plain p quantity sees these too
        assert bad["p"] > R.BOUNDS["p"], (mutate, bad)
