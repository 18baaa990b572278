"""CPU: tests/attention_bwd_ref.py -- the float64 restatement of cfm_attention_bwd that tests/test_attention_bwd_matrix_gpu.py compares the kernels
with -- checked without the library: (a) with unrounded out and lse it equals torch.autograd of a plain float64 masked-softmax attention, (b) the
float32 yardstick passes the bound it defines and has the size the number formats predict, (c) a discrimination audit: every way a kernel could
plausibly be wrong (attention_bwd_ref.VARIANTS) leaves the per-element bound at a named case of the GPU matrix, on every gradient it is said to
hit -- and two of them pass the old max-normalised gate, which is the gap this module closes, (d) predicted_kernel / predicted_group against a
hand-written table, (e) the generators produce the geometries they claim.  The tables are printed (pytest -s)."""
import math

import pytest
import torch

import attention_bwd_ref as R
from attention_bwd_ref import Case, F32, F64


def autograd(P, keep):
    """dq, dk, dv [B,T,D] of sum(out . dout), out = (keep / (1 - p) softmax_masked(scale q k^T)) v, written the way attention.py writes it."""
    r = (lambda x: x.double()) if P.split else (lambda x: x.float().to(P.mma).double())
    Q, K, V = (r(R.fetch(P, n, T)).requires_grad_(True) for n, T in (("q", P.Tq), ("k", P.Tk), ("v", P.Tk)))
    s = (Q @ K.transpose(-1, -2)) * P.scale
    if "mask" in P.bufs:
        m = P.bufs["mask"][0] != 0
        dead = ~(m[:, None, None, :] if m.dim() == 2 else m[:, None]).expand_as(s)
        sm = s.masked_fill(dead, -math.inf)
        sm = torch.where(dead.all(-1, keepdim=True), torch.zeros_like(s), sm)     # a fully masked row: a finite softmax, so that no NaN enters the backward
        a = torch.where(dead, torch.zeros_like(s), torch.softmax(sm, -1))          # ... and the masked_fill(0) of attention.py makes the row a constant
    else:
        a = torch.softmax(s, -1)
    if keep is not None:
        a = a * keep.double() / (1.0 - P.drop)
    out = R.rows(a @ V, P)
    dO = R.heads(P.dout, P)
    dO = R.rows(dO.double() if P.split else dO.float().to(P.mma).double(), P)
    (out * dO).sum().backward()
    return tuple(R.rows(torch.nan_to_num(x.grad), P) for x in (Q, K, V))


AUTOGRAD_CASES = [Case((3, 1, 65, 129), mask="full", layout="cross", drop=0.1), Case((3, 2, 65, 129), dk=60, split=True, mask="full", drop=0.1),
                  Case((3, 1, 65, 129), mma="fp16", mask="pad", ld_pad=8, drop=0.1), Case((2, 2, 130, 5), mask="full", ld_pad=8), Case((1, 1, 1, 1)),
                  Case((2, 2, 63, 63), mask="none", ld_pad=8, sb_pad=2), Case((3, 2, 65, 129), dk=64, do32=True, mask="full")]


@pytest.mark.parametrize("key", AUTOGRAD_CASES, ids=lambda k: "%s-%s-%s" % ("x".join(map(str, k.shape)), k.mask, k.layout))
def test_reference_agrees_with_autograd(key):
    """out and lse unrounded and delta from 16-bit-exact dout: float64 rounding only.  The first cases have a keep mask, fully masked rows and Tq != Tk."""
    P = R.problem(key)
    out, lse = R.forward(P, P.keep)
    if not P.split and P.do_dtype == F32:
        P = type(P)(**dict(vars(P), dout=P.dout.to(P.mma).float()))      # autograd has one dO; delta takes dout as it lies in memory
    ref = R.evaluate(P, type(P)(out=out, lse=lse, keep=P.keep))
    if key.mask == "full" and key.shape[2] > 1:
        assert bool((lse[0, :, min(3, P.Tq - 1)] == -math.inf).all())
    for got, want, name in zip((ref.dq, ref.dk, ref.dv), autograd(P, P.keep), R.GRADS):
        torch.testing.assert_close(got, want, rtol=1e-11, atol=1e-12, msg=lambda m: "%s: %s" % (name, m))
        assert not bool(torch.isnan(got).any())


def test_yardstick_passes_the_bound_it_defines():
    """float32 torch on the same rounded operands, P and dS rounded to the operand type: within g / 4 at every case, and of the size the number formats
    predict -- one rounding of a probability or of dS (unit roundoff 2^-8 bf16, 2^-11 fp16), the three-product formula's dropped lo.lo (2^-16)."""
    G = R.measure_g()
    for cls, keys in R.yardstick_cases().items():
        for k in keys:
            assert all(4.0 * y <= g for y, g in zip(R.yardstick(k), G[cls].g)), k
        print("%-5s float32 torch worst ratio dq %.3g dk %.3g dv %.3g -> g %.3g %.3g %.3g   (%d cases)" % ((cls,) + G[cls].y + G[cls].g + (len(keys),)))
    for i in range(3):
        assert 2.0 ** -13 < G["bf16"].y[i] < 1.01 * 2.0 ** -8 and 2.0 ** -16 < G["fp16"].y[i] < 1.01 * 2.0 ** -11 and 0 < G["split"].y[i] < 2.0 ** -14, (i, G)


def test_fp16_probabilities_underflow_at_peaked_rows():
    """why the peaked cases are bf16: at the same shape in fp16 the float32 yardstick itself loses dk and dv -- probabilities below 2^-14 are subnormal in
    fp16.  A property of the number format (pack8<F16> of P), kept here as a figure; dq, whose rows sum probabilities to 1, is unaffected."""
    y = R.yardstick(R.FP16_PEAKED)
    print("fp16 peaked yardstick: dq %.3g dk %.3g dv %.3g" % y)
    assert y[0] < 2.0 ** -11 and y[1] > 0.05 and y[2] > 0.05
    assert R.FP16_PEAKED not in R.yardstick_cases()["fp16"]


def test_every_wrong_variant_is_separated():
    G = R.measure_g()
    table = []
    for name, (keys, hits) in R.VARIANTS.items():
        worst = [0.0, 0.0, 0.0]
        for key in keys:
            assert key in R.yardstick_cases()[R.klass(key)], "%s: %s is not a case of the GPU matrix" % (name, key)
            P, ref, g = R.problem(key), R.reference(key), G[R.klass(key)]
            w = R.evaluate(P, R.given(P, P.keep), variant=name)
            r = [a / b for a, b in zip(R.ratios(w, ref, F32), g.g)]           # float64 values, no output rounding: the ulp term is left out
            table.append((name, r, key))
            worst = [max(a, b) for a, b in zip(worst, r)]
        for n, x in zip(R.GRADS, worst):
            if n in hits:
                assert x > 1.0, "%s is not separated on %s at these inputs: %.3g x the bound" % (name, n, x)
    print("\n%-28s %-10s %-10s %-10s %s" % ("variant", "dq / bound", "dk / bound", "dv / bound", "case"))
    for name, r, key in table:
        print("%-28s %-10.3g %-10.3g %-10.3g %s %s mask=%s%s" % (name, r[0], r[1], r[2], key.shape, key.mma, key.mask, " drop" if key.drop else ""))
    assert set(R.VARIANTS) == {"last_key_of_tile_dropped", "last_query_of_tile_dropped", "masked_keys_leak", "lse_plus_0.02", "masked_rows_uniform", "delta_omitted",
                               "scale_missing", "drop_index_Tq", "dP_not_dropped", "m_sq_ignored", "mask_transposed", "k_sb_is_Tk_st", "dout_of_head_0"}


@pytest.mark.parametrize("name", ["lse_plus_0.02", "masked_keys_leak"])
def test_old_gate_passes_what_the_bound_catches(name):
    """the gap, written down: on the inputs of test_attention_backward at (2,249,4,64) (ordinary random numbers in the dead rows) these two errors stay
    under the max-normalised bf16 gate of 3e-2 on every gradient -- and leave the per-element bound on the same inputs."""
    key = R.OLD_GATE_CASE
    P, ref = R.problem(key), R.reference(key)
    w = R.evaluate(P, R.given(P, P.keep), variant=name)
    norm = [float((getattr(w, n) - getattr(ref, n)).abs().max() / getattr(ref, n).abs().max()) for n in R.GRADS]
    r = [a / b for a, b in zip(R.ratios(w, ref, F32), R.measure_g()["bf16"].g)]
    print("%s: max-normalised %s, per-element / bound %s" % (name, ["%.3g" % x for x in norm], ["%.3g" % x for x in r]))
    assert max(norm) < R.OLD_GATE
    assert max(r) > 1.0


def test_right_evaluation_passes_as_a_variant_would_be_judged():
    """the audit's own null: the right float64 evaluation, judged like a variant, is at 0."""
    for keys, _ in R.VARIANTS.values():
        for key in keys:
            ref = R.reference(key)
            assert R.ratios(ref, ref, F32) == (0.0, 0.0, 0.0)


# (case, fast, MFULL, profile names): written by hand from bwd_fast_ok and launch_bwd
FAST_BF, FAST_H = ("attn_bwd_delta_fast", "attn_bwd_dq_fast_bf16", "attn_bwd_dkv_fast_bf16"), ("attn_bwd_delta_fast", "attn_bwd_dq_fast_f16", "attn_bwd_dkv_fast_f16")
GEN_BF, GEN_H, GEN_X3 = ("attn_bwd_delta", "attn_bwd_dq_bf16", "attn_bwd_dkv_bf16"), ("attn_bwd_delta", "attn_bwd_dq_f16", "attn_bwd_dkv_f16"), ("attn_bwd_delta", "attn_bwd_dq_bf16x3", "attn_bwd_dkv_bf16x3")
TABLE = [
    (Case((2, 4, 64, 64), ld_pad=8), True, False, FAST_BF),                                  # aligned d_k = 64
    (Case((3, 1, 65, 129), mma="fp16", mask="pad", layout="cross"), True, False, FAST_H),
    (Case((3, 1, 65, 129), mask="full", ld_pad=8), True, True, FAST_BF),
    (Case((2, 2, 63, 63), ld_pad=8, sb_pad=2), True, False, FAST_BF),                        # batch stride (T + 2) ld: still % 8
    (Case((3, 2, 65, 129), mask="full", ld_pad=4), False, True, GEN_BF),                     # ld = 3D + 4: q_st % 8 fails
    (Case((3, 2, 65, 129), do32=True), False, False, GEN_BF),                                # f32 dout beside 16-bit rows
    (Case((3, 2, 65, 129), mma="fp16", f32=True), False, False, GEN_H),                      # f32 rows are not the MFMA type
    (Case((3, 2, 65, 129), dk=60, mma="fp16"), False, False, GEN_H),
    (Case((3, 2, 65, 129), split=True), False, False, GEN_X3),                               # split: never fast, d_k = 64 or not
    (Case((1, 4, 16, 80), dk=36, split=True, do16=True, mask="full"), False, True, GEN_X3),
]


@pytest.mark.parametrize("row", TABLE, ids=lambda r: "%s-%s" % (r[3][1], "x".join(map(str, r[0].shape))))
def test_predicted_kernel(row):
    key, fast, mfull, names = row
    k = R.predicted_kernel(R.problem(key))
    assert (k.fast, k.mfull, k.names) == (fast, mfull, names)


def test_predicted_group():
    P = lambda **kw: R.problem(Case(**kw))
    pad = [P(shape=s, mask="pad", ld_pad=8) for s in ((2, 4, 64, 64), (3, 1, 65, 129), (2, 2, 1, 70))]
    g = R.predicted_group(pad)
    assert g.groupable and not g.mfull and g.names == {"attn_bwd_delta_group", "attn_bwd_dq_group_bf16", "attn_bwd_dkv_group_bf16"}
    g = R.predicted_group([P(shape=s, mma="fp16", mask="full", ld_pad=8) for s in ((2, 4, 64, 64), (3, 1, 65, 129))])
    assert g.groupable and g.mfull and g.names == {"attn_bwd_delta_group", "attn_bwd_dq_group_f16", "attn_bwd_dkv_group_f16"}
    assert R.predicted_group(pad + [P(shape=(3, 1, 65, 65), mask="none", ld_pad=8)]).groupable                      # no mask and a pad mask: one kind (not (B,Tq,Tk))
    mixed = R.predicted_group(pad + [P(shape=(3, 1, 65, 65), mask="full", ld_pad=8)])                               # mixed mask kinds
    assert not mixed.groupable and mixed.names == set(FAST_BF)
    assert not R.predicted_group([P(shape=(2, 4, 64, 64), mask="pad", ld_pad=8, seed=i) for i in range(9)]).groupable      # n = 9
    assert not R.predicted_group(pad[:1]).groupable                                                                     # n = 1
    assert not R.predicted_group(pad + [P(shape=(3, 1, 65, 129), mma="fp16", mask="pad", ld_pad=8)]).groupable          # two MFMA types
    one_general = R.predicted_group(pad + [P(shape=(3, 2, 65, 129), mask="pad", ld_pad=4)])
    assert not one_general.groupable and one_general.names == set(FAST_BF) | set(GEN_BF)
    for mma in ("bf16", "fp16"):
        for mfull in (False, True):
            for n in (3, 8):
                keys = R.group_cases(mma, mfull, n)
                g = R.predicted_group([R.problem(k) for k in keys])
                assert g.groupable and g.mfull == mfull and len({k.shape for k in keys}) >= min(n, 7) and all(k in R.fast_cases(mma) for k in keys)


def test_matrix_reaches_every_instance():
    """the cases of the GPU file, through predicted_kernel: the fast dq / dkv kernels over <type, MFULL>, the general ones in three modes."""
    seen = set()
    for mma in ("bf16", "fp16"):
        for key in R.fast_cases(mma) + R.dropout_cases(mma)[:2]:
            k = R.predicted_kernel(R.problem(key))
            assert k.fast, key
            seen.add((mma, k.mfull))
        assert [R.predicted_kernel(R.problem(k)).mfull for k in R.dropout_cases(mma)[:2]] == [False, True]
        a, b = (R.predicted_kernel(R.problem(k)).fast for k in R.both_ways_cases(mma))
        assert a and not b
    assert seen == {(m, f) for m in ("bf16", "fp16") for f in (False, True)}
    for cls in ("bf16", "fp16", "split"):
        for key in R.general_cases(cls) + R.dropout_cases(cls)[-1:]:
            assert not R.predicted_kernel(R.problem(key)).fast, key
    assert [R.predicted_kernel(R.problem(k)).fast for k in R.peaked_cases()] == [True, False]
    assert [R.klass(k) for k in R.chained_cases()] == ["bf16", "fp16", "split"] and all(k.drop for k in R.chained_cases())


def test_generators_produce_the_geometries_they_claim():
    # pad masks: an utterance with one live key; at Tk = 129 an item whose first 64-key tile is wholly dead
    m = R.problem(Case((3, 1, 65, 129), mask="pad", ld_pad=8)).bufs["mask"][0]
    assert int(m[1].sum()) == 1 and int(m[2, :64].sum()) == 0 and int(m[2, 64:].sum()) > 20 and int(m[0].sum()) > 60
    assert int(R.problem(Case((2, 2, 1, 70), mask="pad", ld_pad=8)).bufs["mask"][0][1].sum()) == 1
    # full masks: one fully masked query row inside a live tile, a key masked for every query, rows whose first tile is dead
    for shape in R.SELF_SHAPES[1:] + R.CROSS_SHAPES[1:] + ((3, 2, 65, 129),):
        P = R.problem(Case(shape, mask="full", ld_pad=8))
        m = P.bufs["mask"][0]
        dead_rows = m.sum(-1) == 0
        assert bool(dead_rows[0, 3]) and int(dead_rows.sum()) == 1 and int(m[0, 2].sum()) > 0 and int(m[0, 4].sum()) > 0, shape
        assert bool(P.dead[P.B - 1, 2]) and int(P.dead.sum()) == 1, shape
        if P.Tk > 64:
            assert int(m[P.B - 1, 0::2, :64].sum()) == 0 and int((m[P.B - 1, 0::2].sum(-1) > 0).sum()) >= (P.Tq + 1) // 2 - 1
    # dead K and V rows hold 3e4 in every head, live ones do not; the rows between two items and past Tq / Tk hold NaN
    P = R.problem(Case((3, 1, 65, 129), mask="pad", ld_pad=8))
    K, V = R.fetch(P, "k", P.Tk).float(), R.fetch(P, "v", P.Tk).float()
    dead = P.dead[:, None, :, None].expand_as(K)
    assert bool((K[dead] > 0.99 * R.DEAD).all()) and bool((V[dead] > 0.99 * R.DEAD).all()) and bool((K[~dead].abs() < 10).all()) and int(P.dead.sum()) > 100    # 3e4 is 29952 in bf16
    P = R.problem(Case((2, 2, 63, 63), ld_pad=8, sb_pad=2))
    buf = P.bufs["qkv"][0]
    assert bool(torch.isnan(buf[:, 63:].float()).all()) and not bool(torch.isnan(buf[:, :63].float()).any()) and P.ops["k"].sb == 65 * P.ops["k"].st
    assert bool(torch.isnan(R.problem(Case((2, 2, 130, 5), ld_pad=8)).bufs["qkv"][0][:, 5:, 128:].float()).all())
    # no scale of the bound lies where float32 has no relative precision; the fully masked row and the dead keys have S = 0
    for cls, keys in R.yardstick_cases().items():
        for k in keys:
            ref = R.reference(k)
            for S in (ref.Sq, ref.Sk, ref.Sv):
                assert not bool(torch.isnan(S).any()) and (not bool((S > 0).any()) or float(S[S > 0].min()) > 1e-30), k
    P, ref = R.problem(Case((3, 1, 65, 129), mask="full", ld_pad=8)), R.reference(Case((3, 1, 65, 129), mask="full", ld_pad=8))
    assert bool((ref.Sq[0, 3] == 0).all()) and bool((ref.Sk[2, 2] == 0).all()) and bool((ref.Sv[2, 2] == 0).all()) and bool((ref.dq[0, 3] == 0).all())
    # peaked rows: probabilities from e^-40 up to 1 enter, so exp(scale s - lse) is evaluated at large |s|
    for key in R.peaked_cases():
        P, ref = R.problem(key), R.reference(key)
        pm = ref.P[ref.P > 0]
        s_max = float((R.fetch(P, "q", P.Tq).double() @ R.fetch(P, "k", P.Tk).double().transpose(-1, -2)).abs()[~P.dead[:, None, None, :].expand(P.B, P.H, P.Tq, P.Tk)].max()) * P.scale
        print("%s d_k %d: largest |scale s| %.1f, smallest live probability %.3g" % (key.shape, key.dk, s_max, float(pm.min())))
        assert s_max > 40 and float(pm.min()) < 1e-25 and float(ref.P.max()) > 0.99
