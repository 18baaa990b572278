"""TEST INFRASTRUCTURE: the optimizer step of csrc/train.hip (cfm_adam_step, cfm_adam_clip_step) restated in float64, plain torch on the CPU.
Never imported by the product.

adam_ref        torch.optim.Adam's rule with L2 weight decay, one step, out of place
clip_scale_ref  the scalar glue of cfm_adam_clip_step: the averaged gradient's norm and the gradient scale that follows from it
adam_inputs     the inputs the optimizer tests share: every term of the update matters somewhere in them
"""
import functools
import math

import torch


def adam_ref(p, g, m, v, lr, betas, eps, weight_decay, step, scale):
    """One Adam step in float64.  p, g, m, v: tensors of one shape (any float dtype, any device); scale: what multiplies g (a float, a
    1-element tensor or None = 1).  Returns new (p, m, v) as float64 CPU tensors; the arguments are left as they are."""
    p, g, m, v = (t.detach().double().cpu() for t in (p, g, m, v))
    if scale is None:
        scale = 1.0
    elif isinstance(scale, torch.Tensor):
        scale = float(scale.detach().double().cpu().reshape(()))        # exact: every float32 is a float64
    b1, b2 = float(betas[0]), float(betas[1])
    gq = g * scale + weight_decay * p
    m = b1 * m + (1.0 - b1) * gq
    v = b2 * v + (1.0 - b2) * gq * gq
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    p = p - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps)
    return p, m, v


def clip_scale_ref(sumsq, clip, inv_world):
    """(norm, scale) of cfm_adam_clip_step as Python floats: norm = sqrt(sumsq) * inv_world is the AVERAGED gradient's norm,
    scale = min(1, clip / (norm + 1e-6)) * inv_world what multiplies the summed gradient (clip_grad_norm_'s coefficient times the
    averaging); clip <= 0: no clipping, scale = inv_world.  A NaN norm gives a NaN scale (Python's min() would let it through
    or not depending on the argument order: written out)."""
    sumsq = float(sumsq)
    norm = math.sqrt(sumsq) * inv_world if sumsq >= 0.0 else float("nan")
    if not clip or clip <= 0:
        return norm, float(inv_world)
    c = clip / (norm + 1e-6)
    if math.isnan(c):
        return norm, float("nan")
    return norm, (c if c < 1.0 else 1.0) * inv_world


def adam_inputs(n, seed, zero_moments=False):
    """float32 CPU tensors p, g, m, v of n elements.
    p   magnitude uniform in [0.5, 2), random sign ("of order 1", and a float32 spacing of at most 1.2e-7)
    g   magnitude log-uniform over 1e-10 .. 1e1, random sign; every 10th element (from a random offset on) exactly zero, and up to 8
        elements denormal (1e-42 .. 1e-39): the structurally zero and the vanishing gradients of a real flat buffer
    m   log-uniform over 1e-8 .. 1e0 with random sign, v log-uniform over 1e-16 .. 1e0 (>= 0): independent of g, so the old moment
        dominates in some elements and the new gradient in others; zero_moments: both zero (the first step of a run)"""
    gen = torch.Generator().manual_seed(seed)
    u = lambda: torch.rand(n, generator=gen, dtype=torch.float64)
    sign = lambda: torch.where(u() < 0.5, -1.0, 1.0).double()
    p = (0.5 + 1.5 * u()) * sign()
    g = 10.0 ** (-10.0 + 11.0 * u()) * sign()
    g[int(torch.randint(0, 10, (1,), generator=gen))::10] = 0.0
    nd = min(8, n // 8)
    if nd:
        idx = torch.randint(0, n, (nd,), generator=gen)
        g[idx] = 10.0 ** (-42.0 + 3.0 * u()[:nd]) * sign()[:nd]
    if zero_moments:
        m, v = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    else:
        m = 10.0 ** (-8.0 + 8.0 * u()) * sign()
        v = 10.0 ** (-16.0 + 16.0 * u())
    return tuple(t.float() for t in (p, g, m, v))


@functools.lru_cache(maxsize=None)
def inputs(n, seed, zero_moments=False):
    """adam_inputs, made once per (n, seed) and shared by the tests: never written to"""
    return adam_inputs(n, seed, zero_moments)


def f32(x):
    """x as the C ABI receives it: rounded to float32, held in a Python float."""
    return float(torch.tensor(x, dtype=torch.float32))


def abi_betas(betas):
    """The betas of the reference.  cfm_adam_step takes `float beta1, float beta2`, so the Adam it can run is the one at the float32
    values: 0.999 arrives as 0.99900001287..., whose 1 - beta2 differs from 0.001 by 1.3e-5 of itself (0.98: 9.5e-7, 0.9: 2.4e-7).  That is
    a perturbation of the hyper-parameter by 1.3e-8, not an arithmetic error, and no kernel behind a float ABI can undo it; measured
    against the unrounded betas it would drown everything the bounds below are there to see."""
    return f32(betas[0]), f32(betas[1])


def _ulp32(x):
    """float32 spacing at |x| (float64 tensor), normal range"""
    _, e = torch.frexp(x.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(x), e - 24)


M_FLOOR = V_FLOOR = 1e-30          # far above the float32 denormals (spacing 1.4e-45), far below every moment the inputs hold


def adam_errors(got, old, lr, betas, eps, weight_decay, step, scale):
    """Worst error of one step's results got = (p, m, v) against adam_ref on the inputs old = (p, g, m, v), each over the update's own
    scale.  Returns a dict of floats; a NaN in `got` gives a NaN, which fails every `<=`.
      p   |got - ref| / max(|p_ref - p_old|, lr * 1e-3)
      dp  the same, after half a float32 spacing of p is taken off |got - ref|: storing the new p in float32 costs up to that whatever
          the update was, and at |p| ~ 1 it is 6e-8 = 6 % of the floor lr * 1e-3 = 1e-6, so `p` alone cannot see an update that is
          wrong by less than that; `dp` is the error of the update itself.  Taken over the elements whose moments cancel less than
          two-fold (|m_ref| and v_ref at least half the size of their terms, see below): the update is m / sqrt(v), and where m is the
          difference of two near-equal terms its relative error has no bound; `p` covers those elements
      m  |got - ref| / max(b1 |m_old| + (1 - b1) (|g scale| + |wd p|), M_FLOOR)
      v   |got - ref| / max(b2 v_old + (1 - b2) (|g scale| + |wd p|)^2, V_FLOOR)
    m and v are relative errors: the denominators are |m_ref| and v_ref wherever the terms have one sign.  Where g * scale and wd * p, or
    the old moment and the new gradient, cancel, NO float32 evaluation has a bounded error relative to the result (among 8 M log-uniform
    elements the worst cancellation is ~1e5-fold), so the size of the terms is the scale there."""
    p0, g0, m0, v0 = (t.detach().double().cpu() for t in old)
    s = 1.0 if scale is None else float(scale)
    b1, b2 = betas
    rp, rm, rv = adam_ref(p0, g0, m0, v0, lr, betas, eps, weight_decay, step, s)
    gp, gm, gv = (t.detach().double().cpu() for t in got)
    gmag = (g0 * s).abs() + (weight_decay * p0).abs()
    mscale, vscale = b1 * m0.abs() + (1.0 - b1) * gmag, b2 * v0 + (1.0 - b2) * gmag * gmag
    dscale = (rp - p0).abs().clamp_min(lr * 1e-3)
    ep = (gp - rp).abs()
    uncancelled = (rm.abs() >= 0.5 * mscale) & (rv >= 0.5 * vscale)
    out = dict(p=ep / dscale,
               dp=torch.where(uncancelled, (ep - 0.5 * _ulp32(torch.maximum(gp.abs(), rp.abs()))).clamp_min(0.0) / dscale, torch.zeros_like(ep)),
               m=(gm - rm).abs() / mscale.clamp_min(M_FLOOR),
               v=(gv - rv).abs() / vscale.clamp_min(V_FLOOR))
    out = {k: (float("nan") if bool(torch.isnan(e).any()) else float(e.max())) for k, e in out.items()}
    return out


# Worst adam_errors() figure per quantity over every case below (CASES and the clip cases) -- rounded up to two digits:
#                 float32 plain torch on the CPU      the HIP kernels on an MI355X        bound = 4 x float32 torch
#   p             0.060  (half a spacing of p / floor) 0.060                              0.24
#   dp            3.8e-7                               4.2e-7   (3.6e-6 before the fix)   1.52e-6
#   m             1.8e-7                               2.0e-7                             7.2e-7
#   v             3.8e-7                               3.7e-7                             1.52e-6
# float32 torch: ref_step_kernels.TorchStepKernels.adam_step on float32 tensors, for the clip cases behind the float32 clip expression of
# trainer.finish(); tests/test_adam_ref_cpu.py::test_bounds_are_four_times_what_float32_torch_costs measures it again on every run.  The
# margin of 4 is for another legitimate order of the float operations (the kernels contract a * b + c into one rounding).
# "Before the fix": with the bias corrections as 1.f - powf(beta, step) in float on the host, dp was 3.4e-6 at n = 12289 and 3.6e-6 at
# BIG, both beta2 = 0.999 at step 2 (bc2 = 0.002 keeps 15 bits of the rounded power); every other case and quantity was as it is now.
# csrc/train.hip now takes 1 - pow(beta, step) and the square root in double and rounds once.  Measured against the UNROUNDED betas the
# kernels -- and any float32 Adam behind this ABI -- show v = 1.3e-5 (beta2 = 0.999) and dp = 6.7e-6: see abi_betas.
F32_TORCH = dict(p=0.060, dp=3.8e-7, m=1.8e-7, v=3.8e-7)
BOUNDS = {k: 4 * e for k, e in F32_TORCH.items()}

# ---------------------------------------------------------------------------------------------------------------- the cases
LR = 1e-3
BETAS_A, BETAS_B = (0.9, 0.98), (0.9, 0.999)
BIG = 8192 * 256 * 4 + 4 * 256 * 3 + 3          # one full sweep of the capped grid, a partial second one, a three-element tail

# (n, betas, eps, weight_decay, step, grad_scale, zero_moments).  Sizes 1, 2, 3 are tail only, 4 is quads only, the others both: every value
# of betas / eps / weight_decay / step / grad_scale stands at a tail-only size or 5 and at a size with quads.
CASES = [
    (1, BETAS_B, 1e-8, 1e-2, 1, None, True),
    (2, BETAS_A, 1e-3, 0.0, 2, 0.37, False),
    (3, BETAS_B, 1e-3, 1e-2, 1000, None, False),
    (4, BETAS_B, 1e-8, 1e-2, 1, 0.37, True),
    (4, BETAS_A, 1e-3, 0.0, 100000, None, False),
    (5, BETAS_A, 1e-8, 0.0, 100000, 0.37, False),
    (5, BETAS_B, 1e-3, 1e-2, 2, None, False),
    (1023, BETAS_B, 1e-8, 1e-2, 1, None, False),
    (1023, BETAS_A, 1e-3, 0.0, 2, 0.37, False),
    (1023, BETAS_B, 1e-3, 1e-2, 1, 0.37, True),
    (1023, BETAS_A, 1e-8, 1e-2, 1, None, True),
    (4096 * 3 + 1, BETAS_B, 1e-8, 1e-2, 1000, 0.37, False),
    (4096 * 3 + 1, BETAS_A, 1e-3, 1e-2, 100000, None, False),
    (4096 * 3 + 1, BETAS_B, 1e-3, 0.0, 2, None, False),
    (4096 * 3 + 1, BETAS_A, 1e-8, 0.0, 2, 0.37, False),
    (BIG, BETAS_B, 1e-8, 1e-2, 2, 0.37, False),
]


def case_id(c):
    n, betas, eps, wd, step, gs, zero = c
    return "n%d-b%g-eps%g-wd%g-step%d-%s%s" % (n, betas[1], eps, wd, step, "gs" if gs else "nogs", "-zero" if zero else "")


def case_seed(c):
    return 1000 + CASES.index(c)


# clip cases: the norm the test plants (as a multiple of the clip) x inv_world.  "well above", "well below", and within 1e-3 of the
# threshold on each side (5e-4: eight thousand float32 spacings, so float32 and float64 agree on the side)
CLIP = 4.0
CLIP_NORMS = [("above", 100.0), ("below", 0.01), ("just_above", 1.0 + 5e-4), ("just_below", 1.0 - 5e-4)]
CLIP_WORLDS = [1.0, 0.125]
CLIP_CASE = dict(betas=BETAS_B, eps=1e-8, wd=1e-2, step=1000)              # the other arguments of every clip case
CLIP_BIG = {("above", 0.125), ("just_below", 1.0)}                         # the two of the eight that also run at n = BIG
CLIP_SEED = 2000                                                           # n = 1023; at BIG the clip cases share the inputs of CASES[-1]


def planted_sumsq(norm_over_clip, inv_world, clip=CLIP):
    """the float32 sum of squares that gives sqrt(sumsq) * inv_world = norm_over_clip * clip (to float32 rounding), as a Python float"""
    return f32((norm_over_clip * clip / inv_world) ** 2)
