"""GPU: the grouped window kernels op by op -- cfm_attention_group, cfm_attention_bwd_group, cfm_dwconv_bn_train_groups, cfm_dwconv_bn_train_bwd_groups and
cfm_ctc_nll_train_groups with more than one problem -- at the smallest shapes that reach their edges.

Every case places every pointer operand with tests/extent.py (inputs between NaN bands, outputs pre-filled with NaN, workspaces at exactly the
documented size; the window operands laid out as csrc/train_layer.cpp lays them out: one qkv [M, 3D], one ctx [M, D], one lse / delta vector with
each group at its running B*H*T offset, one [M, D] row matrix for the depthwise ops) and checks
  (a) each group against the float64 reference of that group ALONE, at the tolerance the single-problem tests use;
  (b) each group bit for bit (torch.equal) against what the single-problem entry point writes for it on the same inputs;
  (c) isolation: the same grouped call with ONE group's inputs replaced leaves the outputs of every other group bit-identical;
and ends with Guards.check().  Which launch a window took (grouped or problem after problem) is read from cfm.prof_table()."""
import numpy as np
import pytest
import torch

from extent import Guards
from test_ops_gpu import W_DT, attn_reference, cfm, relerr, rnd  # noqa: F401  (cfm: the module fixture)
from test_train_ops_gpu import _attn_ref

pytestmark = pytest.mark.gpu

BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
F64 = torch.float64


def close(got, ref, tol, what=""):
    """relerr below tol; NaN (unwritten / poisoned) fails because the comparison is written to be False for it"""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    e = relerr(got.float() if got.dtype != F64 else got, ref)
    print("%-40s relerr %.3e (tolerance %g)" % (what, e, tol))
    assert e < tol, "%s: relerr %r (tolerance %g)" % (what, e, tol)


def exact(got, ref, what=""):
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    if not torch.equal(got, ref):
        bad = (got != ref) | (torch.isnan(got) & ~torch.isnan(ref))
        raise AssertionError("%s: %d of %d elements differ, first at flat index %d" % (what, int(bad.sum()), got.numel(), int(torch.nonzero(bad.reshape(-1))[0, 0])))


class Profiled:
    """with Profiled(cfm) as p: ...; p.names = the kernels the library launched inside"""

    def __init__(self, cfm):
        self.cfm, self.names = cfm, set()

    def __enter__(self):
        self.cfm.prof_reset()
        self.cfm.prof_enable(True)
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        self.cfm.prof_enable(False)
        if exc[0] is None:
            self.names = set(self.cfm.prof_table())
        self.cfm.prof_reset()
        return False


_REF = {}                          # float64 references, computed once per (problem, seed) and left unchanged


# ======================================================================================================================= attention
QT = 64                            # csrc/attn_common.h: query and key tile
SEED3 = 0x2545F491                 # stands for site_seed(seed, 3); train_layer.cpp gives group gi the seed SEED3 + 0x7F4A7C15 * gi


def group_seed(gi):
    return (SEED3 + 0x7F4A7C15 * gi) & 0xFFFFFFFF


class Prob:
    """One attention problem (B utterances of T frames, H heads of dk) with its inputs; mkind none | pad | chunk; pos: a broadcast positional term."""

    def __init__(self, B, T, H, dt, mkind="none", dk=64, pos=False, seed=0):
        self.B, self.T, self.H, self.dk, self.D, self.dt, self.mkind, self.pos, self.seed = B, T, H, dk, H * dk, dt, mkind, pos, seed
        D = self.D
        self.key = (B, T, H, dk, dt, mkind, pos, seed)
        self.qkv, self.dout = rnd((B * T, 3 * D), 1000 + seed, 0.7).to(dt), rnd((B * T, D), 2000 + seed).to(dt)
        lens = [(T, 1, max(1, T // 2), max(1, T - T // 4))[b % 4] for b in range(B)]           # utterance 1 has ONE valid frame
        valid = (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).cuda()
        self.mask, self.mstr = None, (0, 0)
        if mkind == "pad":                                                                       # (B, 1, T): m_sq == 0
            self.mask, self.mstr = valid[:, None, :].contiguous(), (T, 0)
        elif mkind == "chunk":                                                                   # (B, T, T) chunk AND pad: fully masked query rows
            blk = torch.arange(T) // 8
            chunk = ((blk[None, :] <= blk[:, None]) & (blk[None, :] >= blk[:, None] - 1)).cuda()
            self.mask, self.mstr = (chunk[None] & valid[:, None, :]).contiguous(), (T * T, T)
        self.p = self.u = self.vb = None
        if pos:
            self.p, self.u, self.vb = rnd((B, 1, D), 3000 + seed).to(dt), rnd((H, dk), 4000 + seed, 0.3), rnd((H, dk), 5000 + seed, 0.3)

    def reference(self):
        """float64: ctx [B*T, D], lse [B, H, T], d qkv [B*T, 3D] (None with a positional term: forward only)"""
        if self.key not in _REF:
            B, T, H, dk, D = self.B, self.T, self.H, self.dk, self.D
            x = self.qkv.double().view(B, T, 3, H, dk).requires_grad_(True)
            scale = dk ** -0.5
            sc = torch.einsum("bihd,bjhd->bhij", x[:, :, 0].detach(), x[:, :, 1].detach())
            if self.pos:
                o = attn_reference(x[:, :, 0].detach(), x[:, :, 1].detach(), x[:, :, 2].detach(), self.p.double().view(B, 1, H, dk), self.u.double(), self.vb.double(),
                                   self.mask, scale)
                qh, kh = x[:, :, 0].detach().permute(0, 2, 1, 3), x[:, :, 1].detach().permute(0, 2, 1, 3)
                sc = torch.einsum("bhid,bhjd->bhij", qh + self.u.double()[None, :, None, :], kh) + \
                    torch.einsum("bhid,bhjd->bhij", qh + self.vb.double()[None, :, None, :], self.p.double().view(B, 1, H, dk).permute(0, 2, 1, 3))
                grad = None
            else:
                o = _attn_ref(x[:, :, 0], x[:, :, 1], x[:, :, 2], self.mask, scale)
                o.backward(self.dout.double().view(B, T, D))
                grad = x.grad.reshape(B * T, 3 * D)
            sc = sc * scale
            if self.mask is not None:
                sc = sc.masked_fill(~self.mask.unsqueeze(1), float("-inf"))
            _REF[self.key] = (o.detach().reshape(B * T, D), torch.logsumexp(sc, -1), grad)
        return _REF[self.key]


def _fwd_args(p, q, out, lse, mask, mma, split, drop, pv=None, uv=None, vv=None):
    D, T = p.D, p.T
    st = (T * 3 * D, 3 * D)
    kw = dict(q=q, k=q[:, D:], v=q[:, 2 * D:], B=p.B, H=p.H, Tq=T, Tk=T, dk=p.dk, q_str=st, k_str=st + (p.dk,), v_str=st + (p.dk,), out=out, mask=mask, mask_str=p.mstr,
              mma_code=mma, split=split, lse=lse, drop=drop)
    if p.pos:
        kw.update(p=pv, p_str=(D, 0), bias_u=uv, bias_v=vv)
    return kw


def _bwd_args(p, q, ctx, dout, lse, dq, delta, mask, mma, split, drop):
    D, T = p.D, p.T
    st = (T * 3 * D, 3 * D)
    return dict(q=q, k=q[:, D:], v=q[:, 2 * D:], out=ctx, dout=dout, lse=lse, B=p.B, H=p.H, Tq=T, Tk=T, dk=p.dk, q_str=st, k_str=st, v_str=st, dq=dq, dkk=dq[:, D:],
                dv=dq[:, 2 * D:], delta=delta, mask=mask, mask_str=p.mstr, mma_code=mma, split=split, drop=drop)


def _u8(m):
    return None if m is None else m.view(torch.uint8)


def run_attn_window(cfm, probs, mma, split, drop_p, backward):
    """The grouped forward (and backward) over one window; the window operands are single flat allocations (with one D: exactly qkv [M, 3D], ctx [M, D]
    and the lse / delta vectors of train_layer.cpp), each problem at its running offset.  -> per problem (ctx, lse, dqkv), the launched kernel names."""
    dt = probs[0].dt
    oq = np.cumsum([0] + [p.B * p.T * 3 * p.D for p in probs])
    oc = np.cumsum([0] + [p.B * p.T * p.D for p in probs])
    ol = np.cumsum([0] + [p.B * p.H * p.T for p in probs])
    drops = [(drop_p, group_seed(i)) if drop_p else None for i in range(len(probs))]
    qkv_all = torch.cat([p.qkv.reshape(-1) for p in probs])
    G = Guards()
    qv, ctx, lse = G.inp(qkv_all, name="qkv"), G.out((int(oc[-1]),), dt, name="ctx"), G.out((int(ol[-1]),), F32, name="lse")
    masks = [G.inp(_u8(p.mask), name="mask%d" % i) for i, p in enumerate(probs)]
    rows = lambda flat, off, i, cols: flat[int(off[i]):int(off[i + 1])].view(-1, cols)
    fwd = []
    for i, p in enumerate(probs):
        pv, uv, vv = (G.inp(p.p, name="p"), G.inp(p.u, name="bias_u"), G.inp(p.vb, name="bias_v")) if p.pos else (None, None, None)
        fwd.append(_fwd_args(p, rows(qv, oq, i, 3 * p.D), rows(ctx, oc, i, p.D), lse[int(ol[i]):int(ol[i + 1])], masks[i], mma, split, drops[i], pv, uv, vv))
    with Profiled(cfm) as prof:
        cfm.attention_group(fwd)
    G.check()
    names = set(prof.names)
    dqkv = None
    if backward:
        G = Guards()
        qv, cv, lv = G.inp(qkv_all, name="qkv"), G.inp(ctx.clone(), name="ctx"), G.inp(lse.clone(), name="lse")
        dov = G.inp(torch.cat([p.dout.reshape(-1) for p in probs]), name="dout")
        masks = [G.inp(_u8(p.mask), name="mask%d" % i) for i, p in enumerate(probs)]
        dqkv, delta = G.out((int(oq[-1]),), dt, name="dqkv"), G.ws(int(ol[-1]), name="delta")                 # delta: exactly sum B*H*T floats
        bwd = [_bwd_args(p, rows(qv, oq, i, 3 * p.D), rows(cv, oc, i, p.D), rows(dov, oc, i, p.D), lv[int(ol[i]):int(ol[i + 1])], rows(dqkv, oq, i, 3 * p.D),
                         delta[int(ol[i]):int(ol[i + 1])], masks[i], mma, split, drops[i]) for i, p in enumerate(probs)]
        with Profiled(cfm) as prof:
            cfm.attention_bwd_group(bwd)
        G.check()
        names |= prof.names
    outs = [(rows(ctx, oc, i, p.D).clone(), lse[int(ol[i]):int(ol[i + 1])].view(p.B, p.H, p.T).clone(),
             rows(dqkv, oq, i, 3 * p.D).clone() if backward else None) for i, p in enumerate(probs)]
    return outs, names


def run_attn_single(cfm, p, mma, split, drop, backward):
    """Problem p alone through cfm_attention / cfm_attention_bwd, the same strides as in the window."""
    ctx, lse = torch.full((p.B * p.T, p.D), float("nan"), dtype=p.dt, device="cuda"), torch.full((p.B, p.H, p.T), float("nan"), device="cuda")
    cfm.attention(**_fwd_args(p, p.qkv, ctx, lse, _u8(p.mask), mma, split, drop, p.p, p.u, p.vb))
    dqkv = None
    if backward:
        dqkv = torch.full_like(p.qkv, float("nan"))
        kw = _bwd_args(p, p.qkv, ctx, p.dout, lse, dqkv, None, _u8(p.mask), mma, split, drop)
        cfm.attention_bwd(**kw)
    return ctx, lse, dqkv


GROUP_FWD, GROUP_BWD = "attn2_group_", ("attn_bwd_delta_group", "attn_bwd_dq_group_", "attn_bwd_dkv_group_")
CTX_TOL = {"bf16": 2e-2, "fp16": 3e-3, "fp32": 3e-5}
GRAD_TOL = {"bf16": 3e-2, "fp16": 5e-3, "fp32": 1e-4}


def check_attn_window(cfm, specs, mode, grouped, drop_p=0.0, backward=True, isolate=True):
    """specs: [(B, T, H, mkind[, dk[, pos]])].  (a) unless dropout is on (the reference has none), (b), (c) when `isolate`."""
    split = mode == "fp32"
    dt, mma = (F32 if split else W_DT[mode]), (cfm.F16 if mode == "fp16" else cfm.BF16)
    probs = [Prob(s[0], s[1], s[2], dt, s[3], *s[4:], seed=i) for i, s in enumerate(specs)]
    outs, names = run_attn_window(cfm, probs, mma, split, drop_p, backward)
    took_fwd = any(n.startswith(GROUP_FWD) for n in names)
    took_bwd = [any(n.startswith(g) for n in names) for g in GROUP_BWD]
    assert took_fwd == grouped, (sorted(names), grouped)
    if backward:
        assert took_bwd == [grouped] * 3, (sorted(names), grouped)
    for i, (p, (ctx, lse, dqkv)) in enumerate(zip(probs, outs)):
        tag = "problem %d (B=%d T=%d H=%d dk=%d %s)" % (i, p.B, p.T, p.H, p.dk, p.mkind)
        if not drop_p:                                                                                # (a)
            o_ref, lse_ref, g_ref = p.reference()
            close(ctx, o_ref, CTX_TOL[mode], tag + " ctx")
            dead = torch.isinf(lse_ref)
            assert not bool(torch.isnan(lse).any()), tag + " lse: an owned element was not written"
            assert torch.equal(torch.isinf(lse) & (lse < 0), dead), tag + " lse: -inf exactly on the fully masked rows"
            close(lse.double().masked_fill(dead, 0.0), lse_ref.masked_fill(dead, 0.0), CTX_TOL[mode], tag + " lse")
            if p.mkind == "chunk" and p.B > 1 and p.T > 16:
                assert bool(dead.any()), "the chunk mask of this problem has no fully masked row"
                assert float(ctx.view(p.B, p.T, p.H, p.dk).permute(0, 2, 1, 3)[dead].float().abs().max()) == 0.0
            if backward:
                for name, sl in (("dq", slice(0, p.D)), ("dk", slice(p.D, 2 * p.D)), ("dv", slice(2 * p.D, 3 * p.D))):
                    if float(g_ref[:, sl].abs().max()) <= 1e-30:
                        # T = 1: a softmax over ONE key is constant, dq = dk = 0 exactly and a relative error has no denominator; the kernel's
                        # dO.V - dO.O rounding residue is held to the same tolerance on the scale of the problem's whole gradient
                        assert p.T == 1 and float(dqkv[:, sl].float().abs().max()) < GRAD_TOL[mode] * float(g_ref.abs().max()), tag + " " + name
                    else:
                        close(dqkv[:, sl], g_ref[:, sl], GRAD_TOL[mode], tag + " " + name)
        one = run_attn_single(cfm, p, mma, split, (drop_p, group_seed(i)) if drop_p else None, backward)      # (b)
        exact(ctx, one[0], tag + " ctx, grouped against alone")
        exact(lse, one[1], tag + " lse, grouped against alone")
        if backward:
            assert not bool(torch.isnan(dqkv.float()).any()), tag + " dqkv: an owned element was not written"
            exact(dqkv, one[2], tag + " dqkv, grouped against alone")
    if isolate:                                                                                               # (c)
        j = len(probs) // 2
        s = specs[j]
        other = list(probs)
        other[j] = Prob(s[0], s[1], s[2], dt, s[3], *s[4:], seed=100 + j)
        outs2, _ = run_attn_window(cfm, other, mma, split, drop_p, backward)
        assert not torch.equal(outs[j][0], outs2[j][0]), "the replaced problem's output did not change"
        for i in range(len(probs)):
            if i != j:
                for a, b, what in zip(outs[i], outs2[i], ("ctx", "lse", "dqkv")):
                    if a is not None:
                        exact(b, a, "problem %d %s after problem %d's inputs changed" % (i, what, j))


# B*H is 2, 4 or 12 -- never a multiple of 8, so the padded workgroups of one problem sit in front of the next problem's first workgroup; T around the 64-row
# tile (63, 64, 65), two tiles (130) and the single frame
def _w(shapes, H, mkind):
    return [(B, T, H, mkind) for B, T in shapes]


WINDOWS = {2: ([(3, 130), (1, 64)], 4), 3: ([(2, 65), (6, 1), (1, 63)], 2),
           8: ([(1, 64), (2, 63), (6, 1), (2, 65), (1, 130), (1, 63), (2, 64), (1, 65)], 2)}


@pytest.mark.parametrize("mkind", ["none", "pad", "chunk"])
@pytest.mark.parametrize("n,mode", [(2, "bf16"), (2, "fp16"), (3, "bf16"), (3, "fp16"), (8, "bf16")])
def test_attention_window_grouped(cfm, n, mode, mkind):
    shapes, H = WINDOWS[n]
    check_attn_window(cfm, _w(shapes, H, mkind), mode, grouped=True)


@pytest.mark.parametrize("mkind", ["none", "pad", "chunk"])
def test_attention_window_dropout(cfm, mkind):
    """drop_p = 0.1 with the per-group seeds of train_layer.cpp, forward and backward the same: (b) and (c) only (the reference has no dropout)"""
    shapes, H = WINDOWS[3]
    check_attn_window(cfm, _w(shapes, H, mkind), "bf16", grouped=True, drop_p=0.1)


def test_attention_window_with_a_128_query_problem(cfm):
    """B = 24, H = 4, T = 130 without a full mask: alone it takes launch_attn2's 128-query kernel (96 pairs x 2 tiles of 128 = 192 workgroups >= 192);
    in a window it runs the 64-query body of the grouped kernel.  Bit for bit the same: the "bit-identical" comment in launch_attn2."""
    B, H, T = 24, 4, 130
    assert T > 64 and (B * H + 7) // 8 * 8 * ((T + 127) // 128) >= 192
    check_attn_window(cfm, [(B, T, H, "none"), (1, 63, H, "none")], "bf16", grouped=True)


FALLBACKS = {
    # groupable needs ONE mask kind: problem 1 has a full (B, Tq, Tk) mask, problem 0 a pad mask (mfull != mfull0)
    "mixed_masks": ([(2, 65, 2, "pad"), (2, 63, 2, "chunk")], "bf16", True),
    # groupable needs the d_k = 64 fast path for every problem: problem 1 has d_k = 36 (fast == false; backward: bwd_fast_ok needs dk == 64)
    "dk36": ([(2, 65, 2, "pad"), (2, 37, 4, "pad", 36)], "bf16", True),
    # groupable needs p == NULL: problem 1 has a positional term (forward only: the backward has none)
    "positional": ([(2, 65, 2, "pad"), (1, 63, 2, "pad", 64, True)], "bf16", False),
    # groupable needs the fast path, which the f32-accurate split mode never takes (fast needs !split; backward: !descs[i].split)
    "split": ([(2, 65, 2, "chunk"), (1, 63, 2, "chunk")], "fp32", True),
    # groupable needs n <= ATTN_GROUP_MAX = 8
    "nine": ([((1, 63), (2, 1), (1, 64))[i % 3] + (2, "pad") for i in range(9)], "bf16", True),
}


@pytest.mark.parametrize("which", sorted(FALLBACKS))
def test_attention_window_falls_back_problem_after_problem(cfm, which):
    specs, mode, backward = FALLBACKS[which]
    check_attn_window(cfm, specs, mode, grouped=False, backward=backward, isolate=False)


def test_attention_group_wrappers_reject_before_launching(cfm):
    p = Prob(2, 5, 2, BF, "pad")
    ctx, lse = torch.empty((10, 128), dtype=BF, device="cuda"), torch.empty((2, 2, 5), device="cuda")
    good = _fwd_args(p, p.qkv, ctx, lse, _u8(p.mask), cfm.BF16, False, None)
    with Profiled(cfm) as prof:
        with pytest.raises(ValueError, match="passes"):                        # q's own time stride is 384, the call says 128
            cfm.attention_group([good, dict(good, q_str=(640, 128))])
        with pytest.raises(ValueError, match="no stride for it"):
            cfm.attention_group([good, dict(good, out=torch.empty((10, 256), dtype=BF, device="cuda")[:, ::2])])
        dq = torch.empty_like(p.qkv)
        bgood = _bwd_args(p, p.qkv, ctx, p.dout, lse, dq, None, _u8(p.mask), cfm.BF16, False, None)
        with pytest.raises(ValueError, match="passes"):                        # a dense dq beside a fused qkv
            cfm.attention_bwd_group([bgood, dict(bgood, dq=torch.empty((10, 128), dtype=BF, device="cuda"))])
        with pytest.raises(ValueError, match="delta"):
            cfm.attention_bwd_group([bgood, dict(bgood, delta=torch.empty(19, device="cuda"))])
    assert prof.names == set(), "a rejected call launched something"


# ======================================================================================================================= depthwise + BatchNorm(train) + SiLU
DW_SHAPES = {1: [(3, 37)], 2: [(1, 17), (3, 15)], 3: [(1, 3), (2, 16), (3, 37)],
             8: [(2, 1), (1, 3), (3, 15), (2, 16), (1, 17), (3, 37), (1, 3), (3, 15)]}       # group boundaries inside a 16-row block and inside a neighbour's halo
K = 15


class DwWindow:
    def __init__(self, D, dt, groups, seed=0, g_swap=None, ds_swap=None):
        self.D, self.dt, self.groups = D, dt, groups
        self.r0 = np.cumsum([0] + [B * T for B, T in groups])
        M = self.M = int(self.r0[-1])
        self.g, self.ds = rnd((M, D), 23 + seed).to(dt), rnd((M, D), 30 + seed).to(dt)
        for swap, t, sd in ((g_swap, self.g, 123), (ds_swap, self.ds, 130)):                     # isolation: one group's rows replaced
            if swap is not None:
                t[self.r0[swap]:self.r0[swap + 1]] = rnd((int(self.r0[swap + 1] - self.r0[swap]), D), sd).to(dt)
        self.w, self.bias = rnd((D, K), 24, K ** -0.5), rnd((D,), 25, 0.1)
        self.gamma, self.beta = 1 + rnd((D,), 26, 0.1), rnd((D,), 27, 0.1)
        self.rm0, self.rv0 = rnd((D,), 28, 0.1), 1 + rnd((D,), 29, 0.1).abs()
        self.key = (D, dt, tuple(groups), seed)

    def rows(self, t, i):
        return t[int(self.r0[i]):int(self.r0[i + 1])]

    def reference(self):
        """float64, group after group: conv1d -> batch_norm(training=True) -> silu on that group's rows only; the running statistics updated in order;
        the parameter gradients are the sums over the groups."""
        if self.key not in _REF:
            D = self.D
            gr, wr, br, gar, ber = [t.double().requires_grad_(True) for t in (self.g.float(), self.w, self.bias, self.gamma, self.beta)]
            rm, rv = self.rm0.double().clone(), self.rv0.double().clone()
            cs, ss, stats, loss = [], [], [], 0.0
            for i, (B, T) in enumerate(self.groups):
                cr = torch.nn.functional.conv1d(self.rows(gr, i).view(B, T, D).transpose(1, 2), wr.unsqueeze(1), br, padding=7, groups=D)
                sr = torch.nn.functional.silu(torch.nn.functional.batch_norm(cr, rm, rv, gar, ber, True, 0.1, 1e-5)).transpose(1, 2).reshape(B * T, D)
                mean, var = cr.detach().mean((0, 2)), cr.detach().var((0, 2), unbiased=False)
                rstd = (var + 1e-5).rsqrt()
                stats.append(torch.stack([mean, rstd, self.gamma.double() * rstd, self.beta.double() - mean * self.gamma.double() * rstd]))
                cs.append(cr.detach().transpose(1, 2).reshape(B * T, D))
                ss.append(sr.detach())
                loss = loss + (sr * self.rows(self.ds, i).double()).sum()
            loss.backward()
            _REF[self.key] = dict(c=cs, s=ss, stats=stats, rm=rm, rv=rv, dg=gr.grad, dw_w=wr.grad, dw_b=br.grad, dgamma=gar.grad, dbeta=ber.grad)
        return _REF[self.key]


def dw_ws(cfm, groups, D):
    return sum(cfm.lib().cfm_dwconv_bn_ws(B, T, D) for B, T in groups)


def run_dw_forward(cfm, W, running=True):
    G = Guards()
    M, D, n = W.M, W.D, len(W.groups)
    gv, wv, bv, gav, bev = G.inp(W.g, name="g"), G.inp(W.w, name="w"), G.inp(W.bias, name="dw_bias"), G.inp(W.gamma, name="gamma"), G.inp(W.beta, name="beta")
    rm, rv = (G.io(W.rm0, name="running_mean"), G.io(W.rv0, name="running_var")) if running else (None, None)
    c, stats, s = G.out((M, D), F32, name="c"), G.out((n, 4 * D), F32, name="stats"), G.out((M, D), W.dt, name="s")
    ws = G.ws(dw_ws(cfm, W.groups, D), name="ws")
    cfm.dwconv_bn_train_groups(gv, W.groups, wv, bv, gav, bev, rm, rv, 0.1, 1e-5, c=c, stats=stats, s=s, ws=ws)
    G.check()
    return c.clone(), stats.clone(), s.clone(), (rm.clone() if running else None), (rv.clone() if running else None)


def run_dw_backward(cfm, W, c, stats, acc=None, glu_u=None):
    """acc: None (overwrite) or the four prior buffers.  glu_u: run the fused GLU backward (dg_out = NULL) -> du in place of dg."""
    G = Guards()
    M, D = W.M, W.D
    dsv, cv, stv, gv, wv = G.inp(W.ds, name="ds"), G.inp(c, name="c"), G.inp(stats, name="stats"), G.inp(W.g, name="g"), G.inp(W.w, name="w")
    names = ("dw_w", "dw_b", "dgamma", "dbeta")
    outs = [G.io(p, name=nm) for p, nm in zip(acc, names)] if acc else [G.out(sh, F32, name=nm) for sh, nm in zip(((D, K), (D,), (D,), (D,)), names)]
    dy_ws, ws = G.out((M, D), F32, name="dy_ws"), G.ws(dw_ws(cfm, W.groups, D), name="ws")
    if glu_u is not None:
        du = G.out((M, 2 * D), W.dt, name="glu_du")
        res = cfm.dwconv_bn_train_bwd_groups(dsv, cv, stv, gv, W.groups, wv, accumulate=bool(acc), glu_u=G.inp(glu_u, name="glu_u"), glu_du=du, dw_w=outs[0], dw_b=outs[1],
                                             dgamma=outs[2], dbeta=outs[3], dy_ws=dy_ws, ws=ws)
    else:
        dg = G.out((M, D), W.dt, name="dg")
        res = cfm.dwconv_bn_train_bwd_groups(dsv, cv, stv, gv, W.groups, wv, accumulate=bool(acc), dg=dg, dw_w=outs[0], dw_b=outs[1], dgamma=outs[2], dbeta=outs[3],
                                             dy_ws=dy_ws, ws=ws)
    G.check()
    assert not bool(torch.isnan(dy_ws).any()), "dy_ws: an owned element was not written"
    return [t.clone() for t in res]


DW_CASES = [(16, F32, 1), (16, BF, 3), (16, F32, 8), (144, F32, 2), (144, BF, 8), (144, F32, 3), (144, F16, 3), (256, BF, 2), (256, F32, 8), (256, BF, 1),
            (512, F32, 3), (512, BF, 8), (512, F32, 2)]
DW_IDS = ["D%d-%s-n%d" % (D, str(dt).split(".")[1], n) for D, dt, n in DW_CASES]


@pytest.mark.parametrize("D,dt,n", DW_CASES, ids=DW_IDS)
def test_dwconv_bn_window(cfm, D, dt, n):
    """D = 512: two channels per thread; D = 144: a partial 256-thread pass.  B*T mostly no multiple of BNB_ROWS = 16, T on both sides of DWT = 16."""
    W = DwWindow(D, dt, DW_SHAPES[n])
    R = W.reference()
    stol, gtol = (1e-5, 1e-4) if dt == F32 else (1e-2, 1e-2)
    # ---- forward
    c, stats, s, rm, rv = run_dw_forward(cfm, W)
    rm1, rv1 = W.rm0.clone(), W.rv0.clone()
    singles = []
    for i, (B, T) in enumerate(W.groups):
        tag = "group %d (B=%d T=%d)" % (i, B, T)
        close(W.rows(c, i), R["c"][i], 1e-5, tag + " c")                                                           # (a)
        close(W.rows(s, i), R["s"][i], stol, tag + " s")
        for k, name in enumerate(("mean", "rstd", "scale", "shift")):
            close(stats[i].view(4, D)[k], R["stats"][i][k], 1e-5, tag + " stats: " + name)
        one = cfm.dwconv_bn_train(W.rows(W.g, i).view(B, T, D).contiguous(), W.w, W.bias, W.gamma, W.beta, rm1, rv1, 0.1, 1e-5, dt)    # (b), running statistics in order
        singles.append(one)
        exact(W.rows(c, i), one[0].view(B * T, D), tag + " c, grouped against alone")
        exact(stats[i].view(4, D), one[1], tag + " stats, grouped against alone")
        exact(W.rows(s, i), one[2].view(B * T, D), tag + " s, grouped against alone")
    close(rm, R["rm"], 1e-5, "running_mean, updated group after group")
    close(rv, R["rv"], 1e-5, "running_var, updated group after group")
    exact(rm, rm1, "running_mean against the single-problem calls in order")
    exact(rv, rv1, "running_var against the single-problem calls in order")
    c0, stats0, s0, _, _ = run_dw_forward(cfm, W, running=False)                                                     # running_mean = running_var = NULL
    exact(c0, c, "c without running statistics"); exact(stats0, stats, "stats without running statistics"); exact(s0, s, "s without running statistics")
    if n > 1:                                                                                                        # (c)
        j = n // 2
        c2, stats2, s2, _, _ = run_dw_forward(cfm, DwWindow(D, dt, DW_SHAPES[n], g_swap=j))
        assert not torch.equal(W.rows(c2, j), W.rows(c, j))
        for i in range(n):
            if i != j:
                exact(W.rows(c2, i), W.rows(c, i), "c of group %d after group %d's input changed" % (i, j))
                exact(stats2[i], stats[i], "stats of group %d after group %d's input changed" % (i, j))
                exact(W.rows(s2, i), W.rows(s, i), "s of group %d after group %d's input changed" % (i, j))
    # ---- backward
    refs = [R["dw_w"], R["dw_b"], R["dgamma"], R["dbeta"]]
    prior = [rnd((D, K), 31), rnd((D,), 32), rnd((D,), 33), rnd((D,), 34)]
    dg = None
    for acc in (None, prior):
        got = run_dw_backward(cfm, W, c, stats, acc=acc)
        base = [p.double() if acc else torch.zeros_like(p, dtype=F64) for p in prior]
        for i, (B, T) in enumerate(W.groups):
            close(W.rows(got[0], i), W.rows(R["dg"], i), gtol, "group %d (B=%d T=%d) dg%s" % (i, B, T, " (accumulate)" if acc else ""))                  # (a)
        for k, name in ((1, "dw_w"), (3, "dgamma"), (4, "dbeta")):                                                   # sums over the groups, prior + sum with accumulate
            close(got[k].double() - base[k - 1], refs[k - 1], 1e-4, name + (" (accumulate)" if acc else ""))
        assert float((got[2].double() - base[1]).abs().max()) < 1e-3 * float(R["dbeta"].abs().max() + 1e-6)          # dw_b: tiny against dbeta
        if dg is None:
            dg = got[0]
        else:
            exact(got[0], dg, "dg with accumulate against dg without")
    for i, (B, T) in enumerate(W.groups):                                                                            # (b)
        one = cfm.dwconv_bn_train_bwd(W.rows(W.ds, i).contiguous(), singles[i][0], singles[i][1], W.rows(W.g, i).view(B, T, D).contiguous(), W.w, dt)
        exact(W.rows(dg, i), one[0].view(B * T, D), "group %d (B=%d T=%d) dg, grouped against alone" % (i, B, T))
    if n > 1:                                                                                                        # (c)
        j = n // 2
        dg2 = run_dw_backward(cfm, DwWindow(D, dt, DW_SHAPES[n], ds_swap=j), c, stats)[0]
        assert not torch.equal(W.rows(dg2, j), W.rows(dg, j))
        for i in range(n):
            if i != j:
                exact(W.rows(dg2, i), W.rows(dg, i), "dg of group %d after group %d's ds changed" % (i, j))


@pytest.mark.parametrize("D", [16, 144, 256])
@pytest.mark.parametrize("dt", [F32, BF], ids=["float32", "bfloat16"])
@pytest.mark.parametrize("n", [3, 8])
def test_dwconv_bn_window_fused_glu_backward(cfm, D, dt, n):
    """include/cfm.h: glu_u / glu_du with dg_out = NULL gives the same values as cfm_glu_bwd on the rounded dg -- bit for bit against cfm_glu_bwd applied to the
    dg the same call without the GLU pointers wrote in the same dtype, and against the float64 GLU backward of the float64 dg at the dg tolerance."""
    W = DwWindow(D, dt, DW_SHAPES[n])
    R = W.reference()
    c, stats, _, _, _ = run_dw_forward(cfm, W)
    u = rnd((W.M, 2 * D), 40).to(dt)
    plain = run_dw_backward(cfm, W, c, stats)
    fused = run_dw_backward(cfm, W, c, stats, glu_u=u)
    exact(fused[0], cfm.glu_bwd(u, plain[0], dt), "du, fused against cfm_glu_bwd on the rounded dg")
    for k, name in ((1, "dw_w"), (2, "dw_b"), (3, "dgamma"), (4, "dbeta")):
        exact(fused[k], plain[k], name + " with the GLU backward fused")
    zr = u.double().requires_grad_(True)
    zv = zr.view(W.M, D // 16, 2, 16)
    (zv[:, :, 0] * torch.sigmoid(zv[:, :, 1])).reshape(W.M, D).backward(R["dg"])
    for i, (B, T) in enumerate(W.groups):
        close(W.rows(fused[0], i), W.rows(zr.grad, i), 1e-4 if dt == F32 else 1e-2, "group %d (B=%d T=%d) du" % (i, B, T))


def test_dwconv_group_wrappers_reject_before_launching(cfm):
    D = 16
    W = DwWindow(D, F32, DW_SHAPES[2])
    wide = torch.zeros((W.M, 2 * D), device="cuda")
    st = torch.zeros((2, 4 * D), device="cuda")
    with Profiled(cfm) as prof:
        with pytest.raises(ValueError, match="no stride for it"):
            cfm.dwconv_bn_train_groups(wide[:, :D], W.groups, W.w, W.bias, W.gamma, W.beta)
        with pytest.raises(ValueError, match="no stride for it"):
            cfm.dwconv_bn_train_groups(W.g, W.groups, torch.zeros((D, 2 * K), device="cuda")[:, ::2], W.bias, W.gamma, W.beta)
        with pytest.raises(ValueError, match="rows"):
            cfm.dwconv_bn_train_groups(W.g, [(1, 17), (3, 14)], W.w, W.bias, W.gamma, W.beta)
        with pytest.raises(ValueError, match="row groups"):
            cfm.dwconv_bn_train_groups(W.g, [(1, 1)] * 9, W.w, W.bias, W.gamma, W.beta)
        with pytest.raises(ValueError, match="go together"):
            cfm.dwconv_bn_train_groups(W.g, W.groups, W.w, W.bias, W.gamma, W.beta, running_mean=W.rm0)
        with pytest.raises(ValueError, match="no stride for it"):
            cfm.dwconv_bn_train_bwd_groups(W.ds, wide[:, :D], st, W.g, W.groups, W.w)
        with pytest.raises(ValueError, match="glu_du without glu_u"):
            cfm.dwconv_bn_train_bwd_groups(W.ds, W.g, st, W.g, W.groups, W.w, glu_du=wide)
        with pytest.raises(ValueError, match="one dtype"):
            cfm.dwconv_bn_train_bwd_groups(W.ds, W.g, st, W.g, W.groups, W.w, glu_u=wide, dg_dtype=BF)
        with pytest.raises(ValueError, match="pass all four"):
            cfm.dwconv_bn_train_bwd_groups(W.ds, W.g, st, W.g, W.groups, W.w, accumulate=True)
        with pytest.raises(ValueError, match="at least"):
            cfm.dwconv_bn_train_bwd_groups(W.ds, W.g, st, W.g, W.groups, W.w, ws=torch.zeros(8, device="cuda"))
    assert prof.names == set(), "a rejected call launched something"


# ======================================================================================================================= CTC
CTC_SHAPES = [(4, 30, 5), (3, 49, 9), (2, 60, 12)]          # B, T, Umax; the vocabulary is ONE argument of the call, so a window has one V


class CtcProblem:
    def __init__(self, i, B, T, V, Umax, ld, infeasible=False, seed=0):
        self.B, self.T, self.V, self.Umax, self.ld = B, T, V, Umax, ld
        rs = np.random.RandomState(B * 100 + T + 7 * i)
        self.logits = torch.zeros((B, T, ld), device="cuda")
        self.logits[:, :, :V] = rnd((B, T, V), 38 + i + seed, 2.0)
        self.enc_lens = np.sort(rs.randint(max(2 * Umax + 1, T // 2), T + 1, size=B))[::-1].copy()
        self.enc_lens[0] = T
        self.label_lens = rs.randint(1, Umax + 1, size=B)
        self.label_lens[0] = Umax
        self.labels = rs.randint(1, V, size=(B, Umax))
        self.labels[1, 1:3] = self.labels[1, 0]
        self.bad = B - 1 if infeasible else None
        if infeasible:                                       # more labels than frames
            self.label_lens[self.bad], self.enc_lens[self.bad] = Umax, Umax - 1
        for b in range(B):
            self.labels[b, self.label_lens[b]:] = 0
        self.key = ("ctc", i, B, T, V, Umax, infeasible, seed)

    def reference(self):
        if self.key not in _REF:
            lr = self.logits[:, :, :self.V].detach().cpu().double().requires_grad_(True)
            per = torch.nn.functional.ctc_loss(lr.transpose(0, 1).log_softmax(2), torch.from_numpy(self.labels), torch.from_numpy(self.enc_lens),
                                               torch.from_numpy(self.label_lens), reduction="none", zero_infinity=False)
            ok = torch.isfinite(per)
            (per[ok].sum() / self.Umax).backward()
            _REF[self.key] = (per.detach(), lr.grad)
        return _REF[self.key]


def i32(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype=torch.int32)


def run_ctc_window(cfm, probs, n=None, expect_error=None):
    """-> per problem dict(nll, alpha, beta, lse, nll_shifted, work, operands for cfm_ctc_grad)"""
    G = Guards()
    arr = (cfm.CtcGroup * len(probs))()
    outs = []
    for g, p in zip(arr, probs):
        SM = 2 * p.Umax + 2
        o = dict(lv=G.inp(p.logits, name="logits"), el=G.inp(i32(p.enc_lens), name="enc_lens"), lb=G.inp(i32(p.labels), name="labels"), ll=G.inp(i32(p.label_lens), name="label_lens"))
        for nm in ("work", "alpha", "beta"):
            o[nm] = G.ws(p.B * p.T * SM, name=nm)
        o["lse"], o["nll"], o["nll_shifted"] = G.ws(p.B * p.T, name="lse"), G.out((p.B,), F32, name="nll"), G.out((p.B,), F32, name="nll_shifted")
        g.logits, g.ld, g.B, g.T, g.Umax = o["lv"].data_ptr(), p.ld, p.B, p.T, p.Umax
        g.enc_lens, g.labels, g.label_lens = o["el"].data_ptr(), o["lb"].data_ptr(), o["ll"].data_ptr()
        g.work, g.alpha, g.lse, g.nll, g.nll_shifted, g.beta = (o[k].data_ptr() for k in ("work", "alpha", "lse", "nll", "nll_shifted", "beta"))
        outs.append(o)
    with Profiled(cfm) as prof:
        if expect_error:
            with pytest.raises(RuntimeError, match=expect_error):
                cfm.check(cfm.lib().cfm_ctc_nll_train_groups(arr, len(probs) if n is None else n, probs[0].V, cfm.stream()), "cfm_ctc_nll_train_groups")
        else:
            cfm.check(cfm.lib().cfm_ctc_nll_train_groups(arr, len(probs) if n is None else n, probs[0].V, cfm.stream()), "cfm_ctc_nll_train_groups")
    G.check()
    return outs, prof.names, G


def ctc_window(V, n, seed_of=None):
    lds = ((V + 3) // 4 * 4, (V + 8 + 3) // 4 * 4)           # the ABI takes row strides that are multiples of 4 floats only: V + 8 rounded up as well
    return [CtcProblem(i, *CTC_SHAPES[i % 3][:2], V, CTC_SHAPES[i % 3][2], lds[i % 2], infeasible=(i == 1), seed=(seed_of or {}).get(i, 0)) for i in range(n)]


STATE = ("nll", "alpha", "beta", "lse", "nll_shifted")


def same_bits(got, ref, what):
    """alpha / beta keep slots no recursion writes (states past 2 * label_len, frames past enc_len, the pad column of the 2 * Umax + 2 row) and cfm_ctc_grad
    never reads: they hold the NaN pre-fill in both runs, so the state is compared as the 32-bit patterns it consists of"""
    exact(got.view(torch.int32), ref.view(torch.int32), what)


@pytest.mark.parametrize("n", [2, 3, 8])
@pytest.mark.parametrize("V", [11, 73])
def test_ctc_window(cfm, V, n):
    """n problems that differ in B, T, Umax and ld (V, and V + 8, each rounded up to the multiple of 4 the ABI asks for: 12 / 20 and 76 / 84); the last
    utterance of problem 1 has more labels than frames."""
    probs = ctc_window(V, n)
    outs, names, _ = run_ctc_window(cfm, probs)
    assert "ctc_alpha_beta_group" in names, sorted(names)
    L = cfm.lib()
    for i, (p, o) in enumerate(zip(probs, outs)):
        tag = "problem %d (B=%d T=%d Umax=%d ld=%d)" % (i, p.B, p.T, p.Umax, p.ld)
        per, g_ref = p.reference()
        fin = torch.isfinite(per)
        nll = o["nll"].cpu()
        assert torch.equal(torch.isinf(nll) & (nll > 0), ~fin), (tag, nll, per)                                  # (a)
        assert bool((~fin).any()) == (p.bad is not None)
        close(nll[fin], per[fin], 2e-5, tag + " nll")
        G = Guards()
        gdev, grad = G.inp(torch.full((1,), 2.0), name="gscale_dev"), G.out((p.B, p.T, p.ld), F32, name="dlogits")
        cfm.check(L.cfm_ctc_grad(o["lv"].data_ptr(), p.ld, p.B, p.T, V, o["el"].data_ptr(), o["lb"].data_ptr(), p.Umax, o["ll"].data_ptr(), o["work"].data_ptr(), o["alpha"].data_ptr(),
                                 o["beta"].data_ptr(), o["lse"].data_ptr(), o["nll_shifted"].data_ptr(), 0.5 / p.Umax, gdev.data_ptr(), grad.data_ptr(), cfm.stream()), "cfm_ctc_grad")
        G.check()
        assert float(grad[:, :, V:].abs().max()) == 0.0                                                           # NaN (unwritten pad columns) fails this too
        keep = fin.nonzero().flatten().tolist()
        close(grad[keep][:, :, :V].cpu(), g_ref[keep], 5e-4, tag + " dlogits")
        if p.bad is not None:
            assert bool(torch.isfinite(grad).all()) and float(grad[p.bad].abs().max()) == 0.0 and float(grad[0].abs().max()) > 0
        for b in range(p.B):
            if p.enc_lens[b] < p.T:
                assert float(grad[b, int(p.enc_lens[b]):].abs().max()) == 0.0
        one, _, _ = run_ctc_window(cfm, [p])                                                                      # (b)
        for k in STATE:
            same_bits(o[k], one[0][k], tag + " " + k + ", grouped against alone")
    j = n // 2                                                                                                    # (c)
    outs2, _, _ = run_ctc_window(cfm, ctc_window(V, n, seed_of={j: 500}))
    assert not torch.equal(outs2[j]["nll"], outs[j]["nll"])
    for i in range(n):
        if i != j:
            for k in STATE:
                same_bits(outs2[i][k], outs[i][k], "problem %d %s after problem %d's logits changed" % (i, k, j))


def test_ctc_window_of_nine_raises_and_writes_nothing(cfm):
    probs = [CtcProblem(i, 2, 12, 11, 3, 12) for i in range(9)]
    outs, names, _ = run_ctc_window(cfm, probs, expect_error="1 .. 8 micro-batches")            # Guards.check() inside: bands intact
    assert names == set(), "a rejected call launched something"
    for o in outs:
        for k in STATE + ("work",):
            assert bool(torch.isnan(o[k]).all()), k
