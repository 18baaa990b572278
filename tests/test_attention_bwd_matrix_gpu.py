"""GPU: cfm_attention_bwd and cfm_attention_bwd_group -- the general delta / dq / dkv kernels in bf16, fp16 and split mode, the fast dq / dkv kernels
over <BF16 | F16, MFULL>, the fast delta kernel in both types and the group forms of all the fast kernels -- against the float64 restatement of
tests/attention_bwd_ref.py.

Bound.  Per element, never a norm (attention_bwd_ref's docstring): |dq - ref| <= g_q S^q + ulp_io(ref) and the same for dk and dv, with S the sums
of absolute values that the gradient is a signed sum of; where S = 0 -- dq of a fully masked row, dk and dv of a key no query sees -- the value is
exactly 0; no NaN anywhere.  The g are not constants: attention_bwd_ref.measure_g evaluates the same formulas in plain float32 torch with the
design's roundings at these very cases and takes 4 x the worst ratio per class and gradient.  The module prints yardstick / bound / kernel
(pytest -s); DESIGN.md holds the figures of the run that introduced it.

`out` and `lse` come from the float64 forward (rounded to the io type / float32), not from cfm_attention: the backward is isolated; only
test_chained runs cfm_attention first and hands the reference the kernel's out and lse.  The dropout keep mask comes from cfm.dropout_mask.
Every pointer operand lies in a guarded allocation of tests/extent.py (inputs between NaN bands; the gradients and delta pre-filled with NaN; the
rows of a gradient buffer that belong to no operand must still hold NaN afterwards), and the profile names of each call must be the ones
attention_bwd_ref.predicted_kernel / predicted_group name -- so each case is known to reach the kernels it was written for
(test_every_instantiation_was_launched compares the sets).  K and V rows that are masked for every query hold the FINITE value 3e4 (NaN there is
outside the contract, as in the forward): a masked key that entered with any weight would miss the bound, and its dk and dv must be exactly 0.
What each wrong kernel would fail is shown on the CPU: tests/test_attention_bwd_ref_cpu.py::test_every_wrong_variant_is_separated.
"""
import time
from types import SimpleNamespace

import pytest
import torch

import attention_bwd_ref as R
import extent
from test_attention_matrix_gpu import profiled, strided
from test_ops_gpu import cfm  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu

DEV = "cuda"
RUNS = {}                                                    # Case -> what check() found, computed once
WORST = {c: [0.0, 0.0, 0.0] for c in ("bf16", "fp16", "split")}   # kernel (|d| - ulp) / S per gradient, printed by test_report_worst_ratios
LAUNCHED = set()                                             # (profile name, class, MFULL) of every call that was held to the reference
T0 = time.time()
DROP_SEED = 20240


def device_keep(cfm, P, seed):
    """the keep mask the kernels regenerate for (p, seed): element (b, h, i, j) at ((b H + h) Tq + i) Tk + j."""
    if not P.drop:
        return None
    return cfm.dropout_mask(P.B * P.H * P.Tq * P.Tk, P.drop, seed, DEV).view(P.B, P.H, P.Tq, P.Tk).cpu()


def place(G, P, g):
    """every operand of one problem in guarded allocations -> the keyword arguments of cfm.attention_bwd and the handles of the gradient buffers."""
    pl = {name: G.inp(t.reshape(-1, t.shape[-1]), ld=ld, name=name) for name, (t, ld) in P.bufs.items()}
    gr = {name: G.out((t.numel() // t.shape[-1], t.shape[-1]), t.dtype, ld=ld, name="grad of " + name) for name, (t, ld) in P.bufs.items() if name != "mask"}
    kw = dict(B=P.B, H=P.H, Tq=P.Tq, Tk=P.Tk, dk=P.dk, mma_code=cfm_code(P), split=P.split, scale=P.scale)
    for name, grad, T in (("q", "dq", P.Tq), ("k", "dkk", P.Tk), ("v", "dv", P.Tk)):
        o = P.ops[name]
        kw[name], kw[grad] = (strided(b[o.buf], o.off, (P.B, T, P.D), (o.sb, o.st, 1)) for b in (pl, gr))
        kw[name + "_str"] = (o.sb, o.st)
    if "mask" in P.bufs:
        m_sb, m_sq = P.mask_str
        kw["mask"], kw["mask_str"] = strided(pl["mask"], 0, (P.B, P.Tq if m_sq else 1, P.Tk), (m_sb, m_sq or P.Tk, 1)), P.mask_str
    kw["out"], kw["dout"], kw["lse"] = G.inp(g.out, name="out"), G.inp(P.dout, name="dout"), G.inp(g.lse, name="lse")
    kw["delta"] = G.ws(P.B * P.H * P.Tq, name="delta")                         # exactly B H Tq floats
    return kw, gr


CODES = {}


def cfm_code(P):
    return CODES["bf16" if P.mma == R.BF16 else "f16"]


def collect(P, gr, delta):
    """the gradients as [B,T,D] CPU tensors, read through the operand strides; what belongs to no operand must still be NaN; delta fully written."""
    host = {name: t.cpu() for name, t in gr.items()}
    Pg = SimpleNamespace(**dict(vars(P), bufs={name: (t, P.bufs[name][1]) for name, t in host.items()}))
    res = SimpleNamespace(**{n: R.rows(R.fetch(Pg, o, T), P) for n, o, T in (("dq", "q", P.Tq), ("dk", "k", P.Tk), ("dv", "v", P.Tk))})
    for name, t in host.items():
        own = torch.zeros(t.shape[0] * P.bufs[name][1], dtype=torch.bool)
        for o in ("q", "k", "v"):
            if P.ops[o].buf == name:
                own |= R.owned(P, o)
        assert bool(torch.isnan(R.flat(t, P.bufs[name][1])[~own].float()).all()), "the gradient buffer of %s was written outside its operands" % name
    assert not bool(torch.isnan(delta).any()), "delta: an owned element was not written"
    return res


def run(cfm, P, g, drop):
    """one cfm.attention_bwd call, every operand guarded -> (namespace(dq, dk, dv) on the CPU, the profile names seen)."""
    G = extent.Guards(DEV)
    kw, gr = place(G, P, g)
    seen = profiled(cfm, lambda: cfm.attention_bwd(drop=drop, **kw))
    G.check()
    return collect(P, gr, kw["delta"].cpu()), seen


def hold(res, ref, P, cls, what):
    """the bound of the module docstring on one result."""
    g = R.measure_g()[cls]
    for n in R.GRADS:
        assert not bool(torch.isnan(getattr(res, n).float()).any()), "%s: NaN in %s" % (what, n)
    r = R.ratios(res, ref, P.io)
    print("%s: dq %.3g of %.3g, dk %.3g of %.3g, dv %.3g of %.3g" % (what, r[0], g.g[0], r[1], g.g[1], r[2], g.g[2]))
    for i, n in enumerate(R.GRADS):
        if r[i] < float("inf"):
            WORST[cls][i] = max(WORST[cls][i], r[i])
        assert r[i] <= g.g[i], "%s: |%s - ref| beyond ulp reaches %.3g S, over g = %.3g (inf: a value that must be exactly 0 is not)" % (what, n, r[i], g.g[i])
    dead = P.dead[:, :, None].expand(P.B, P.Tk, P.D)
    assert bool((res.dk[dead] == 0).all()) and bool((res.dv[dead] == 0).all()), "%s: a key masked for every query has a gradient" % what


def describe(key, pk):
    return "%s %s dk %d mask=%s %s%s%s" % (pk.names[1], "x".join(map(str, key.shape)), key.dk, key.mask, key.layout, " x4" if key.qk_scale != 1 else "", " drop" if key.drop else "")


def check(cfm, key):
    """run the case once, hold it to the reference and to the predicted kernels; -> namespace(res, kernel, ref, g, drop)."""
    if key in RUNS:
        return RUNS[key]
    CODES.update(bf16=cfm.BF16, f16=cfm.F16)
    P = R.problem(key)
    pk = R.predicted_kernel(P)
    drop = (P.drop, DROP_SEED + len(RUNS)) if P.drop else None
    g = R.given(P, device_keep(cfm, P, drop[1]) if drop else None)
    ref = R.evaluate(P, g)
    res, seen = run(cfm, P, g, drop)
    what = describe(key, pk)
    assert seen == set(pk.names), "%s: launched %s" % (what, sorted(seen))
    LAUNCHED.update((n, R.klass(key), pk.mfull) for n in pk.names)
    hold(res, ref, P, R.klass(key), what)
    RUNS[key] = SimpleNamespace(res=res, kernel=pk, ref=ref, g=g, drop=drop)
    return RUNS[key]


# ---------------------------------------------------------------------------------------------------------------- the fast kernels
@pytest.mark.parametrize("mask", R.MASKS)
@pytest.mark.parametrize("mma", ["bf16", "fp16"])
def test_fast_kernels(cfm, mma, mask):
    """cfm_attn_bwd_{dq,dkv}_fast_kernel<HT, MFULL> and cfm_attn_delta_fast_kernel<HT>: {fused 16-bit [B,T,3D+8], separate q with fused k|v} at
    (B, H, Tq, Tk) = (1,1,1,1), (2,4,64,64), (3,1,65,65), (2,2,63,63) and, Tq != Tk, (2,2,1,70), (2,2,130,5), (3,1,65,129): on, below and past the 16-row fragment and
    the 64-row tile in both directions; (2,2,63,63) with a batch stride that is not T st."""
    keys = [k for k in R.fast_cases(mma) if k.mask == mask]
    assert len(keys) == 14
    for key in keys:
        r = check(cfm, key)
        assert r.kernel.fast and r.kernel.mfull == (mask == "full"), key


# ---------------------------------------------------------------------------------------------------------------- the general kernels
@pytest.mark.parametrize("cls", ["bf16", "fp16", "split"])
def test_general_kernels(cfm, cls):
    """cfm_attn_delta_kernel and cfm_attn_bwd_{dq,dkv}_kernel<HT, SPLIT>: d_k = 4, 36, 60, and 64 behind ld = 3D + 4; float32 rows with a 16-bit MFMA and no
    split; 16-bit rows with float32 dout at d_k = 64 (split: 16-bit dout beside float32 rows); each with no mask, a pad mask and a full mask."""
    keys = R.general_cases(cls)
    assert len(keys) == (15 if cls == "split" else 18)
    for key in keys:
        assert not check(cfm, key).kernel.fast, key


@pytest.mark.parametrize("cls", ["bf16", "fp16", "split"])
def test_dropout(cfm, cls):
    """p = 0.1 at Tq != Tk, the keep mask from cfm.dropout_mask: one fast case per MFULL value and type, one general case per class."""
    keys = R.dropout_cases(cls)
    assert len(keys) == (1 if cls == "split" else 3)
    kinds = [(check(cfm, k).kernel.fast, check(cfm, k).kernel.mfull) for k in keys]
    assert kinds == ([(False, True)] if cls == "split" else [(True, False), (True, True), (False, True)])
    for k in keys:
        keep = RUNS[k].g.keep
        assert 0.85 < float(keep.float().mean()) < 0.95 and not bool(keep.all(-1).all())


def test_peaked_rows(cfm):
    """q and k times 4: exp(scale s - lse) at |scale s| up to 50 and probabilities from e^-40 to 1.  The bound is relative to S, so it is the same one."""
    assert [check(cfm, k).kernel.fast for k in R.peaked_cases()] == [True, False]


@pytest.mark.parametrize("mma", ["bf16", "fp16"])
def test_dk64_on_both_paths(cfm, mma):
    """the same operands at ld = 3D (fast) and ld = 3D + 4 (general): each within the one bound; the two are not compared with each other."""
    fast, general = (check(cfm, k) for k in R.both_ways_cases(mma))
    assert fast.kernel.fast and not general.kernel.fast


# ---------------------------------------------------------------------------------------------------------------- the group forms
@pytest.mark.parametrize("n", [3, 8])
@pytest.mark.parametrize("mfull", [False, True])
@pytest.mark.parametrize("mma", ["bf16", "fp16"])
def test_group(cfm, mma, mfull, n):
    """cfm.attention_bwd_group with n fast problems of different shapes: the group kernels ran (profile names), every problem is within the bound and
    bit-identical to its single call."""
    keys = R.group_cases(mma, mfull, n)
    singles = [check(cfm, k) for k in keys]
    Ps = [R.problem(k) for k in keys]
    pg = R.predicted_group(Ps)
    assert pg.groupable and pg.mfull == mfull
    G = extent.Guards(DEV)
    placed = [place(G, P, s.g) for P, s in zip(Ps, singles)]
    seen = profiled(cfm, lambda: cfm.attention_bwd_group([kw for kw, _ in placed]))
    G.check()
    assert seen == pg.names, sorted(seen)
    LAUNCHED.update((name, mma, mfull) for name in pg.names)
    for key, P, s, (kw, gr) in zip(keys, Ps, singles, placed):
        res = collect(P, gr, kw["delta"].cpu())
        what = "group of %d, %s" % (n, describe(key, s.kernel))
        hold(res, s.ref, P, mma, what)
        for name in R.GRADS:
            assert torch.equal(getattr(res, name), getattr(s.res, name)), "%s: %s differs from the single call" % (what, name)


# ---------------------------------------------------------------------------------------------------------------- forward, then backward
@pytest.mark.parametrize("cls", ["bf16", "fp16", "split"])
def test_chained(cfm, cls):
    """cfm.attention(lse=, drop=) and then cfm.attention_bwd on its out and lse: the reference takes the kernel's out and lse as given."""
    CODES.update(bf16=cfm.BF16, f16=cfm.F16)
    key = {R.klass(k): k for k in R.chained_cases()}[cls]
    P = R.problem(key)
    pk = R.predicted_kernel(P)
    drop = (P.drop, DROP_SEED + 1000)
    keep = device_keep(cfm, P, drop[1])
    G = extent.Guards(DEV)
    pl = {name: G.inp(t.reshape(-1, t.shape[-1]), ld=ld, name=name) for name, (t, ld) in P.bufs.items()}
    q, k, v = (strided(pl[o.buf], o.off, (P.B, T, P.D), (o.sb, o.st, 1)) for o, T in ((P.ops["q"], P.Tq), (P.ops["k"], P.Tk), (P.ops["v"], P.Tk)))
    m_sb, m_sq = P.mask_str
    mask = strided(pl["mask"], 0, (P.B, P.Tq if m_sq else 1, P.Tk), (m_sb, m_sq or P.Tk, 1))
    out, lse = G.out((P.B, P.Tq, P.D), P.io, name="out"), G.out((P.B, P.H, P.Tq), torch.float32, name="lse")
    qo, ko, vo = P.ops["q"], P.ops["k"], P.ops["v"]
    cfm.attention(q, k, v, P.B, P.H, P.Tq, P.Tk, P.dk, (qo.sb, qo.st), (ko.sb, ko.st, P.dk), (vo.sb, vo.st, P.dk), out, mask=mask, mask_str=P.mask_str, mma_code=cfm_code(P), split=P.split, scale=P.scale, lse=lse, drop=drop)
    torch.cuda.synchronize()
    G.check()
    g = SimpleNamespace(out=out.cpu(), lse=lse.cpu(), keep=keep)
    want = R.given(P, keep)                                    # the forward is pinned elsewhere; this only says that both ops mean the same keep mask
    assert float((g.out.double() - want.out.double()).abs().max()) < 0.05 * float(want.out.double().abs().max()) and torch.equal(torch.isinf(g.lse), torch.isinf(want.lse))
    ref = R.evaluate(P, g)
    res, seen = run(cfm, P, g, drop)
    assert seen == set(pk.names), sorted(seen)
    hold(res, ref, P, cls, "chained, " + describe(key, pk))


# ---------------------------------------------------------------------------------------------------------------- what ran
def instances():
    """every kernel of csrc/attention_bwd.hip by the profile name it is launched under, with the mode it ran in (the general delta kernel is one
    kernel, counted once per mode it is launched in) and, where it is a template argument, MFULL."""
    want = set()
    for cls, tag in (("bf16", "bf16"), ("fp16", "f16"), ("split", "bf16x3")):
        want |= {("attn_bwd_delta", cls), ("attn_bwd_dq_" + tag, cls), ("attn_bwd_dkv_" + tag, cls)}
    for mma, tag in (("bf16", "bf16"), ("fp16", "f16")):
        want |= {("attn_bwd_delta_fast", mma), ("attn_bwd_delta_group", mma)}
        for mfull in (False, True):
            want |= {("attn_bwd_d%s_%s_%s" % (w, form, tag), mma, mfull) for w in ("q", "kv") for form in ("fast", "group")}
    return want


def test_every_instantiation_was_launched(cfm):
    """a set comparison, not a log: the cases above (run here if they have not run yet), each launched under the names predicted_kernel gives, cover the 27
    kernels of attention_bwd.hip in 29 (kernel, mode) pairs: 9 general (delta, dq, dkv in bf16, fp16 and split mode), 8 fast dq / dkv over <type, MFULL>, the fast
    delta in two types, and the 10 group forms of the fast kernels."""
    for mma in ("bf16", "fp16"):
        for key in R.fast_cases(mma):
            check(cfm, key)
        for mfull in (False, True):
            if ("attn_bwd_delta_group", mma, mfull) not in LAUNCHED:
                test_group(cfm, mma, mfull, 3)
    for cls in ("bf16", "fp16", "split"):
        for key in R.general_cases(cls):
            check(cfm, key)
    got = {(n, c, f) if ("_dq_" in n or "_dkv_" in n) and ("fast" in n or "group" in n) else (n, c) for n, c, f in LAUNCHED}
    want = instances()
    assert got == want and len(want) == 29, sorted(want ^ got)
    # the MFULL split of the general kernels is a run-time branch, not an instance; both sides of it ran all the same
    assert {t + (f,) for t in want if len(t) == 2 and "fast" not in t[0] and "group" not in t[0] for f in (False, True)} <= LAUNCHED


def test_report_worst_ratios(cfm):
    """not a check of its own: prints what the module measured (pytest -s), the figures DESIGN.md quotes."""
    G = R.measure_g()
    for cls in ("bf16", "fp16", "split"):
        g = G[cls]
        for i, n in enumerate(R.GRADS):
            print("%-5s %s (|d| - ulp)/S  float32 torch %.3g  bound g %.3g  kernel %.3g" % (cls, n, g.y[i], g.g[i], WORST[cls][i]))
    print("%d cases held to the reference, %.1f s since the module was imported" % (len(RUNS), time.time() - T0))
