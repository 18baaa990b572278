"""GPU: cfm_attention -- every instantiation of the d_k = 64 fast path, the 128-query form, the general kernel in bf16, fp16 and split mode, and the
streaming form read from a K/V ring -- against the float64 restatement of tests/attention_ref.py.

Bound.  Per element, never a norm: |out - ref| <= g S + ulp_out(ref), S_id = sum_j a_ij |v_jd|, and |lse - ref| <= g_lse L_i, L_i = scale max_j-live
sum_d (|qu||k_j| + |qv||p_j|); a fully masked row is exactly 0 with lse exactly -inf; no NaN anywhere.  g and g_lse are not constants:
attention_ref.measure_g evaluates the same formula in plain float32 torch on the same rounded operands at these very cases (probabilities rounded to
the operand type before P.V; split mode: the header's three products) and takes 4 x the worst ratio per class.  The module prints yardstick /
bound / kernel (pytest -s); DESIGN.md holds the figures of the run that introduced it.

Every pointer operand lies in a guarded allocation of tests/extent.py (inputs between NaN bands, outputs pre-filled with NaN), lse is requested
wherever out is, and the profile name of the launched kernel must be the family attention_ref.predicted_kernel names -- so each case is known to
reach the instantiation it was written for (test_every_instantiation_was_launched compares the sets).  What each wrong kernel would fail is shown on
the CPU: tests/test_attention_ref_cpu.py::test_every_wrong_variant_is_separated.

Streaming form: cfm_kv_ring_write fills the f32 ring, cfm_stream_prep makes the slot mask, cfm_attention reads both; the reference gathers each
stream's live frames in time order from the original K, V and p.  Dead slots hold NaN in their K half and in p; their V half holds a large
FINITE value (3e4): the kernels multiply a masked key's value by a probability of exactly zero (csrc/stream.hip: "a masked slot has to stay
finite"), as attention.py does, so a NaN there is outside the contract, while a dead value that entered with any weight would miss the bound.
"""
from types import SimpleNamespace

import pytest
import torch

import attention_ref as R
import extent
from test_ops_gpu import cfm  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu

DEV = "cuda"
RUNS = {}                                                    # Case -> what check() found, computed once
WORST = {c: [0.0, 0.0] for c in ("bf16", "fp16", "split")}  # kernel (|d| - ulp) / S and |d lse| / L, printed by test_report_worst_ratios
FAMILIES = set()


def strided(placed, off, size, strides):
    return torch.as_strided(placed, size, strides, placed.storage_offset() + off)


def profiled(cfm, f):
    cfm.prof_reset(); cfm.prof_enable(True)
    try:
        f()
        torch.cuda.synchronize()
    finally:
        cfm.prof_enable(False)
    return set(cfm.prof_table())


def run(cfm, P, b0=0, nb=None):
    """items [b0, b0 + nb) of the problem in one cfm.attention call, every operand guarded -> (out, lse on the CPU, the profile names seen)."""
    nb = P.B if nb is None else nb
    G = extent.Guards(DEV)
    pl = {name: G.inp(t.reshape(-1, t.shape[-1]), ld=ld, name=name) for name, (t, ld) in P.bufs.items()}
    qo, ko, vo = P.ops["q"], P.ops["k"], P.ops["v"]
    q = strided(pl[qo.buf], qo.off + b0 * qo.sb, (nb, P.Tq, P.D), (qo.sb, qo.st, 1))
    if ko.buf == "cache":
        k, v = (strided(pl["cache"], o.off + b0 * o.sb, (nb, P.H, P.Tk, P.dk), (o.sb, o.sh, o.st, 1)) for o in (ko, vo))
    else:
        k, v = (strided(pl[o.buf], o.off + b0 * o.sb, (nb, P.Tk, P.D), (o.sb, o.st, 1)) for o in (ko, vo))
    p = u = vb = mask = None
    if "p" in P.ops:
        p_sb, p_st = P.p_str
        p = strided(pl["p"], b0 * p_sb, (nb if p_sb else 1, P.Tk if p_st else 1, P.D), (p_sb or P.D, p_st or P.D, 1))
        u, vb = G.inp(P.u, name="bias_u"), G.inp(P.vb, name="bias_v")
    if "mask" in P.bufs:
        m_sb, m_sq = P.mask_str
        mask = strided(pl["mask"], b0 * m_sb, (nb, P.Tq if m_sq else 1, P.Tk), (m_sb, m_sq or P.Tk, 1))
    out = G.out((nb, P.Tq, P.D), P.out_dtype, name="out")
    lse = G.out((nb, P.H, P.Tq), torch.float32, name="lse")
    seen = profiled(cfm, lambda: cfm.attention(q, k, v, nb, P.H, P.Tq, P.Tk, P.dk, (qo.sb, qo.st), (ko.sb, ko.st, ko.sh), (vo.sb, vo.st, vo.sh), out, p=p, p_str=P.p_str,
                                               bias_u=u, bias_v=vb, mask=mask, mask_str=P.mask_str, mma_code=cfm.BF16 if P.mma == R.BF16 else cfm.F16,
                                               split=P.split, scale=P.scale, lse=lse))
    G.check()
    return out.cpu(), lse.cpu(), seen


def hold(out, lse, ref, P, cls, what):
    """the bound of the module docstring on one result."""
    g = R.measure_g()[cls]
    assert not bool(torch.isnan(out).any()) and not bool(torch.isnan(lse).any()), "%s: NaN in out or lse" % what
    ro, rl = R.ratios(out, lse, ref, P.out_dtype)
    if ro < float("inf") and rl < float("inf"):
        WORST[cls][0], WORST[cls][1] = max(WORST[cls][0], ro), max(WORST[cls][1], rl)
    print("%s: out %.3g of g %.3g, lse %.3g of g_lse %.3g" % (what, ro, g.g, rl, g.g_lse))
    assert ro <= g.g, "%s: |out - ref| beyond ulp reaches %.3g S, over g = %.3g (inf: a fully masked row that is not exactly 0)" % (what, ro, g.g)
    assert rl <= g.g_lse, "%s: |lse - ref| reaches %.3g L, over g_lse = %.3g (inf: a fully masked row whose lse is not -inf, or an infinite lse)" % (what, rl, g.g_lse)


def check(cfm, key):
    """run the case once, hold it to the reference and to the predicted kernel family; -> namespace(out, lse, kernel)."""
    if key in RUNS:
        return RUNS[key]
    P, ref = R.problem(key), R.reference(key)
    pk = R.predicted_kernel(P)
    out, lse, seen = run(cfm, P)
    what = "%s %s dk %d p=%s mask=%s %s%s" % (pk.name, "x".join(map(str, key.shape)), key.dk, key.pmode, key.mask, key.layout, " x4" if key.qk_scale != 1 else "")
    assert seen == {pk.name}, "%s: launched %s" % (what, sorted(seen))
    FAMILIES.add(pk.name)
    hold(out, lse, ref, P, R.klass(key), what)
    RUNS[key] = SimpleNamespace(out=out, lse=lse, kernel=pk)
    return RUNS[key]


# ---------------------------------------------------------------------------------------------------------------- the fast path
@pytest.mark.parametrize("pmode", ["none", "bcast", "perkey"])
@pytest.mark.parametrize("mma", ["bf16", "fp16"])
def test_fast_path_instances(cfm, mma, pmode):
    """cfm_attn2_kernel<HT, PMODE, MFULL, KVF32>: {pad / no mask, full mask} x {fused 16-bit q|k|v, f32 cache with k_sh = Tk 2 dk} at (B, H, Tq, Tk) =
    (1,1,1,1), (3,1,65,257), (1,9,17,513), (2,4,64,256), (2,2,63,255): B H = 1, 3, 4, 8, 9 (groups of 8 pairs: short, exact, one past), Tq and Tk on, below and
    past the 16 / 64-query and 256-key edges; an utterance with one live key, a fully masked row, an item with no live key among the first 256."""
    keys = [k for k in R.fast_cases(mma) if k.pmode == pmode or (pmode == "perkey" and k.pmode == "shared")]
    assert len(keys) == (22 if pmode == "perkey" else 20)
    inst = set()
    for key in keys:
        r = check(cfm, key)
        assert r.kernel.fast and not r.kernel.q128, key
        inst.add((r.kernel.mfull, r.kernel.kvf32))
    assert inst == {(False, False), (False, True), (True, False), (True, True)}


@pytest.mark.parametrize("mma", ["bf16", "fp16"])
def test_q128_instances_and_their_bits(cfm, mma):
    """cfm_attn2_q128_kernel<HT, 0 | 1> at 96 (b, h) pairs x 2 tiles of 128 queries = 192 workgroups; the same problem as two batches of 12 stays under
    the threshold, runs the 64-query kernel and must give the same bits (launch_attn2: "per query the same arithmetic in the same order")."""
    pmodes = set()
    for key in R.q128_cases(mma):
        r = check(cfm, key)
        assert r.kernel.q128, key
        pmodes.add(r.kernel.pmode)
        P = R.problem(key)
        assert not R.predicted_kernel(R.problem(key._replace(shape=(12,) + key.shape[1:]))).q128
        halves = [run(cfm, P, b0, 12) for b0 in (0, 12)]
        assert all(h[2] == {r.kernel.name} for h in halves)
        assert torch.equal(torch.cat([h[0] for h in halves]), r.out) and torch.equal(torch.cat([h[1] for h in halves]), r.lse), key
    assert pmodes == {0, 1}


def test_rising_maximum(cfm):
    """q and k times 4: rows whose dominating key lies in the last super-tile (fast path) or tile (general kernel) after a smaller maximum before it --
    the alpha rescale.  The bound is relative to S and L, so it is the same one."""
    kinds = set()
    for key in R.rising_cases():
        kinds.add(check(cfm, key).kernel.fast)
    assert kinds == {True, False}


# ---------------------------------------------------------------------------------------------------------------- the general kernel
@pytest.mark.parametrize("cls", ["bf16", "fp16", "split"])
def test_general_kernel(cfm, cls):
    """cfm_attn_kernel<HT, HAS_POS, SPLIT>: d_k = 4, 36, 60, and 64 behind a row stride of 3D + 4; every p and mask kind; f32 q|K|V, and 16-bit q with f32 K/V."""
    for key in R.general_cases(cls):
        assert not check(cfm, key).kernel.fast, key


@pytest.mark.parametrize("mma", ["bf16", "fp16"])
def test_dk64_on_both_paths(cfm, mma):
    """the same operands at ld = 3D (fast) and ld = 3D + 4 (general): each within the one bound; the two are not compared with each other."""
    fast, general = (check(cfm, k) for k in R.both_ways_cases(mma))
    assert fast.kernel.fast and not general.kernel.fast


# ---------------------------------------------------------------------------------------------------------------- the streaming form
def i32(x):
    return torch.tensor(x, dtype=torch.int32, device=DEV)


def ring_write(cfm, k, v, code, ring, offs, lens, B, H, T, dk):
    """k, v [B, T, H dk] dense -> ring slots (offs[b] + t) mod ring_T, rows t < lens[b] (None: all)."""
    D = H * dk
    cfm.check(cfm.lib().cfm_kv_ring_write(k.data_ptr(), v.data_ptr(), code, T * D, D, T * D, D, ring.data_ptr(), offs.data_ptr(), cfm.ptr(lens), B, H, T, dk, ring.shape[2],
                                          cfm.stream()), "cfm_kv_ring_write")


@pytest.mark.parametrize("offsets", R.STREAM_OFFSETS)
@pytest.mark.parametrize("mma", ["bf16", "fp16"])
def test_streaming_form(cfm, mma, offsets):
    f = R.stream_frames(offsets, mma)
    B, H, dk, T, RT, D = len(offsets), R.STREAM_H, 64, R.CHUNK, R.RING_T, R.STREAM_H * 64
    G = extent.Guards(DEV)
    ring0 = torch.full((B, H, RT, 2 * dk), float("nan"))
    ring0[..., dk:] = 3.0e4                                   # a dead value stays finite (module docstring)
    ring = G.io(ring0, name="ring")
    # the cached frames: one earlier write of c_b rows at offset off_b - c_b; then the chunk at off_b
    kv_prev = []
    for t in (f.k, f.v):
        prev = torch.full((B, R.NEED, D), float("nan"), dtype=t.dtype)
        for b, c in enumerate(f.cached):
            prev[b, :c] = t[b, R.NEED - c:R.NEED]
        kv_prev.append(G.inp(prev, name="earlier rows"))
    k_new, v_new = G.inp(f.k[:, R.NEED:].contiguous(), name="k"), G.inp(f.v[:, R.NEED:].contiguous(), name="v")
    code = cfm.BF16 if mma == "bf16" else cfm.F16
    for k, v, offs, lens, rows in ((kv_prev[0], kv_prev[1], i32([o - c for o, c in zip(offsets, f.cached)]), i32(f.cached), R.NEED), (k_new, v_new, i32(offsets), None, T)):
        ring_write(cfm, k, v, code, ring, offs, lens, B, H, rows, dk)
    slot_mask, pos_rows = G.out((B, RT), torch.uint8, name="slot mask"), G.out((B, RT, D), torch.float32, name="pos rows")
    cfm.stream_prep(i32(offsets), T, R.NEED, RT, G.inp(R.rnd((1024, D), 9), name="pe"), slot_mask, pos_rows)
    want_mask = torch.zeros((B, RT), dtype=torch.uint8)
    p_ring = torch.full((B, RT, D), float("nan"), dtype=f.p.dtype)
    for b, off in enumerate(offsets):
        for i, (slot, _) in enumerate(R.stream_slots(off)):
            want_mask[b, slot] = 1
            p_ring[b, slot] = f.p[b, R.NEED - f.cached[b] + i]
    assert torch.equal(slot_mask.cpu(), want_mask)
    live = ring.cpu()[want_mask[:, None, :].expand(B, H, RT) != 0]
    assert not bool(torch.isnan(live).any()) and bool((live[..., dk:] != 3.0e4).any())
    assert bool(torch.isnan(ring.cpu()[..., :dk][want_mask[:, None, :].expand(B, H, RT) == 0]).all())     # the writes touched no dead slot
    q, p = G.inp(f.q, name="q"), G.inp(p_ring, name="p")
    u, vb = G.inp(f.u, name="bias_u"), G.inp(f.vb, name="bias_v")
    out, lse = G.out((B, T, D), torch.float32, name="out"), G.out((B, H, T), torch.float32, name="lse")
    kstr = (H * RT * 2 * dk, 2 * dk, RT * 2 * dk)
    seen = profiled(cfm, lambda: cfm.attention(q, ring[..., :dk], ring[..., dk:], B, H, T, RT, dk, (T * D, D), kstr, kstr, out, p=p, p_str=(RT * D, D), bias_u=u, bias_v=vb,
                                               mask=slot_mask, mask_str=(RT, 0), mma_code=code, scale=dk ** -0.5, lse=lse))
    G.check()
    name = "attn2_rel_" + ("bf16" if mma == "bf16" else "f16")                                   # f32 K/V, per-key p, slot mask: <HT, 2, false, true>
    assert seen == {name}, sorted(seen)
    for b in range(B):
        P, ref = R.stream_problem(offsets, mma, b), R.stream_reference(offsets, mma, b)
        assert R.predicted_kernel(P).name == name
        hold(out[b:b + 1].cpu(), lse[b:b + 1].cpu(), ref, P, mma, "%s ring stream at offset %d" % (name, offsets[b]))


# ---------------------------------------------------------------------------------------------------------------- what ran
def test_every_instantiation_was_launched(cfm):
    """a set comparison, not a log: the cases above (run here if they have not run yet), each launched under the family predicted_kernel names, cover all
    24 cfm_attn2_kernel instances, the four 128-query ones and the six general kernels."""
    inst = set()
    for mma in ("bf16", "fp16"):
        for key in R.fast_cases(mma) + R.q128_cases(mma):
            k = check(cfm, key).kernel
            inst.add((mma, k.pmode, k.mfull, k.kvf32, k.q128))
    want = {(m, p, f, k, False) for m in ("bf16", "fp16") for p in (0, 1, 2) for f in (False, True) for k in (False, True)}
    want |= {(m, p, False, False, True) for m in ("bf16", "fp16") for p in (0, 1)}
    assert inst == want and len(want) == 28
    assert sum(1 for i in inst if i[3]) == 12                 # the KVF32 half
    for cls in ("bf16", "fp16", "split"):
        for key in R.general_cases(cls):
            check(cfm, key)
    assert FAMILIES >= {"attn2_bf16", "attn2_rel_bf16", "attn2_f16", "attn2_rel_f16", "attn_bf16", "attn_rel_bf16", "attn_f16", "attn_rel_f16", "attn_bf16x3", "attn_rel_bf16x3"}


def test_report_worst_ratios(cfm):
    """not a check of its own: prints what the module measured (pytest -s), the figures DESIGN.md quotes."""
    G = R.measure_g()
    for cls in ("bf16", "fp16", "split"):
        g = G[cls]
        print("\n%-5s (|d| - ulp)/S  float32 torch %.3g  bound g %.3g  kernel %.3g    |d lse|/L  float32 torch %.3g  bound g_lse %.3g  kernel %.3g"
              % (cls, g.y, g.g, WORST[cls][0], g.y_lse, g.g_lse, WORST[cls][1]))
