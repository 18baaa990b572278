"""CPU: tests/attention_ref.py -- the float64 restatement of cfm_attention that tests/test_attention_matrix_gpu.py compares the kernels with --
checked without the library: (a) against torch's own softmax in float64, (b) the float32 yardstick passes the bound it defines at every case,
(c) a discrimination audit: every way a kernel could plausibly be wrong (attention_ref.VARIANTS) breaks the per-element bound at a named case of
the GPU matrix -- the dropped broadcast term through lse alone, (d) predicted_kernel against a hand-written table, (e) the mask and score
generators produce the geometries they claim.  The tables are printed (pytest -s)."""
import math

import pytest
import torch

import attention_ref as R
from attention_ref import Case


def plain(P):
    """the operation written the way attention.py writes it, on [B,H,T,dk] operands in float64."""
    Q, K, V = (R.fetch(P, n, T).float() for n, T in (("q", P.Tq), ("k", P.Tk), ("v", P.Tk)))
    r = (lambda x: x.to(P.mma).double()) if not P.split else (lambda x: x.double())
    if "p" in P.ops:
        Pp = R.fetch(P, "p", P.Tk if P.p_str[1] else 1).float()
        qu, qv = Q + P.u[None, :, None, :], Q + P.vb[None, :, None, :]
        if P.split:
            qu, qv = Q.double() + P.u.double()[None, :, None, :], Q.double() + P.vb.double()[None, :, None, :]
        s = r(qu) @ r(K).transpose(-1, -2) + r(qv) @ r(Pp).transpose(-1, -2)
    else:
        s = r(Q) @ r(K).transpose(-1, -2)
    s = s * P.scale
    if "mask" in P.bufs:
        m = P.bufs["mask"][0] != 0
        m = m[:, None, None, :] if m.dim() == 2 else m[:, None]
        s = s.masked_fill(~m, -math.inf)
        a = torch.softmax(s, -1).masked_fill(~m, 0.0)
    else:
        a = torch.softmax(s, -1)
    a = torch.nan_to_num(a, nan=0.0)
    return (a @ r(V)).permute(0, 2, 1, 3).reshape(P.B, P.Tq, P.D), torch.logsumexp(s, -1)


@pytest.mark.parametrize("key", [Case((3, 1, 65, 257), pmode="perkey", mask="pad"), Case((2, 4, 64, 256), mma="fp16", pmode="bcast", mask="full", layout="cache"),
                                 Case((3, 2, 65, 129), dk=60, split=True, f32=True, pmode="shared", mask="pad"), Case((1, 4, 16, 80), dk=36, pmode="none", mask="pad", f32=True),
                                 Case((1, 1, 1, 1)), Case((2, 2, 63, 255), pmode="none", mask="full", ld_pad=8)])
def test_reference_agrees_with_torch(key):
    P, ref = R.problem(key), R.reference(key)
    out, lse = plain(P)
    torch.testing.assert_close(ref.out, out, rtol=1e-11, atol=1e-12)
    torch.testing.assert_close(ref.lse, lse, rtol=1e-11, atol=1e-12)
    assert not bool(torch.isnan(ref.out).any()) and bool((ref.S >= 0).all()) and bool((ref.L[ref.lse > -math.inf] > 0).all())


def test_yardstick_passes_the_bound_it_defines():
    """float32 torch on the same rounded operands, probabilities rounded to the operand type: within g / 4 at every case, and of the size the
    number formats predict (one rounding of a probability: 2^-9 bf16, 2^-12 fp16; the three-product formula drops lo.lo: 2^-16; float32 scores)."""
    G = R.measure_g()
    for cls, keys in R.yardstick_cases().items():
        for k in keys:
            y, yl = R.yardstick(k)
            assert 4.0 * y <= G[cls].g and 4.0 * yl <= G[cls].g_lse, k
        print("%-5s float32 torch worst |d|/S %.3g -> g %.3g   worst |d lse|/L %.3g -> g_lse %.3g   (%d cases)" % (cls, G[cls].y, G[cls].g, G[cls].y_lse, G[cls].g_lse, len(keys)))
    assert 2.0 ** -12 < G["bf16"].y < 1.01 * 2.0 ** -8 and 2.0 ** -15 < G["fp16"].y < 1.01 * 2.0 ** -11 and 0 < G["split"].y < 2.0 ** -14
    assert all(0 < G[c].y_lse < 2.0 ** -19 for c in ("bf16", "fp16")) and 0 < G["split"].y_lse < 2.0 ** -14


def test_every_wrong_variant_is_separated():
    G = R.measure_g()
    rows = []
    for name, key in R.VARIANTS.items():
        assert key in R.yardstick_cases()[R.klass(key)], "%s: not a case of the GPU matrix" % name
        P, ref, g = R.problem(key), R.reference(key), G[R.klass(key)]
        w = R.evaluate(P, variant=name)
        ro, rl = R.ratios(w.out, w.lse, ref, torch.float32)           # float64 values, no output rounding: the ulp term is left out
        rows.append((name, ro / g.g, rl / g.g_lse, key))
    print("\n%-24s %-12s %-12s %s" % ("variant", "out / bound", "lse / bound", "case"))
    for name, o, l, key in rows:
        print("%-24s %-12.3g %-12.3g %s %s p=%s mask=%s %s" % (name, o, l, key.shape, key.mma, key.pmode, key.mask, key.layout))
    for name, o, l, _ in rows:
        if name in R.LSE_ONLY:
            assert o <= 1.0 and l > 10.0, "%s must leave out inside the bound and break lse: out %.3g, lse %.3g x the bound" % (name, o, l)
        else:
            assert max(o, l) > 10.0, "%s is not separated at these inputs: out %.3g, lse %.3g x the bound" % (name, o, l)


def test_right_evaluation_passes_as_a_variant_would_be_judged():
    """the audit's own null: the right float64 evaluation, judged like a variant, is at 0."""
    for key in set(R.VARIANTS.values()):
        ref = R.reference(key)
        assert R.ratios(ref.out, ref.lse, ref, torch.float32) == (0.0, 0.0)


# (case, family, fast, q128, MFULL, KVF32, PMODE): written by hand from attn_args and launch_attn2
TABLE = [
    (Case((1, 1, 1, 1)), "attn2_bf16", True, False, False, False, 0),
    (Case((3, 1, 65, 257), mma="fp16", pmode="bcast", mask="pad"), "attn2_rel_f16", True, False, False, False, 1),
    (Case((3, 1, 65, 257), pmode="perkey", mask="full", layout="cache"), "attn2_rel_bf16", True, False, True, True, 2),
    (Case((3, 1, 65, 257), pmode="shared", mask="pad", layout="cache"), "attn2_rel_bf16", True, False, False, True, 2),
    (Case((2, 2, 63, 255), pmode="none", mask="full", ld_pad=8), "attn2_bf16", True, False, True, False, 0),
    (Case((2, 2, 63, 255), pmode="none", mask="full", ld_pad=4), "attn_bf16", False, False, True, False, 0),          # q_st = 3D + 4: al8 fails
    (Case((24, 4, 130, 130), pmode="bcast", mask="pad"), "attn2_rel_bf16", True, True, False, False, 1),         # 96 pairs x 2 tiles of 128 = 192
    (Case((12, 4, 130, 130), pmode="bcast", mask="pad"), "attn2_rel_bf16", True, False, False, False, 1),        # 48 x 2 = 96 < 192
    (Case((24, 4, 64, 130)), "attn2_bf16", True, False, False, False, 0),                                        # Tq <= 64
    (Case((24, 4, 130, 130), pmode="perkey"), "attn2_rel_bf16", True, False, False, False, 2),                   # per-key p: never 128 queries
    (Case((24, 4, 130, 130), mask="full"), "attn2_bf16", True, False, True, False, 0),
    (Case((24, 4, 130, 130), layout="cache"), "attn2_bf16", True, False, False, True, 0),
    (Case((1, 4, 16, 80), dk=36, mma="fp16", pmode="perkey"), "attn_rel_f16", False, False, False, False, 2),
    (Case((3, 2, 65, 129), split=True, f32=True, pmode="bcast"), "attn_rel_bf16x3", False, False, False, True, 1),
    (Case((3, 2, 65, 129), split=True, f32=True), "attn_bf16x3", False, False, False, True, 0),
    (Case((3, 2, 65, 129), f32=True), "attn_bf16", False, False, False, True, 0),                                 # q f32 is not the MFMA type
    (Case((3, 2, 65, 129), dk=60, layout="cache", mask="pad"), "attn_bf16", False, False, False, True, 0),
]


@pytest.mark.parametrize("row", TABLE, ids=lambda r: "%s-%s" % (r[1], "x".join(map(str, r[0].shape))))
def test_predicted_kernel(row):
    key, name, fast, q128, mfull, kvf32, pmode = row
    k = R.predicted_kernel(R.problem(key))
    assert (k.name, k.fast, k.q128, k.mfull, k.kvf32, k.pmode) == (name, fast, q128, mfull, kvf32, pmode)


def test_matrix_reaches_every_fast_instance():
    """the cases of the GPU file, through predicted_kernel: all 24 cfm_attn2_kernel instances (12 of them KVF32) and the four 128-query ones."""
    seen = set()
    for mma in ("bf16", "fp16"):
        for key in R.fast_cases(mma) + R.q128_cases(mma):
            k = R.predicted_kernel(R.problem(key))
            assert k.fast, key
            seen.add((mma, k.pmode, k.mfull, k.kvf32, k.q128))
    want = {(m, p, f, k, False) for m in ("bf16", "fp16") for p in (0, 1, 2) for f in (False, True) for k in (False, True)}
    want |= {(m, p, False, False, True) for m in ("bf16", "fp16") for p in (0, 1)}
    assert seen == want
    for cls in ("bf16", "fp16", "split"):
        for key in R.general_cases(cls):
            assert not R.predicted_kernel(R.problem(key)).fast, key
    for mma in ("bf16", "fp16"):
        a, b = (R.predicted_kernel(R.problem(k)).fast for k in R.both_ways_cases(mma))
        assert a and not b


def test_generators_produce_the_geometries_they_claim():
    ninf = -math.inf
    # a pad mask: an utterance with one live key, and one whose first 256 keys are all dead while later keys live
    m = R.problem(Case((3, 1, 65, 257), mask="pad")).bufs["mask"][0]
    assert int(m[2].sum()) == 1 and int(m[2, :256].sum()) == 0 and int(m[0].sum()) > 100 and 1 < int(m[1].sum()) < 257 and int(m[1, 0]) == 1
    assert int(R.problem(Case((2, 2, 63, 255), mask="pad", ld_pad=8)).bufs["mask"][0][1].sum()) == 1
    m = R.problem(Case((1, 9, 17, 513), mask="pad")).bufs["mask"][0]
    assert int(m[0, :256].sum()) == 0 and int(m[0, 256:].sum()) > 100
    # full masks: a fully masked row, rows with a dead first super-tile, and no other dead row
    for shape in R.FAST_SHAPES[1:]:
        P = R.problem(Case(shape, mask="full"))
        m = P.bufs["mask"][0]
        dead = m.sum(-1) == 0
        assert bool(dead[0, min(3, P.Tq - 1)]) and int(dead.sum()) == 1
        assert bool((R.reference(P.key).lse[0, :, min(3, P.Tq - 1)] == ninf).all())
        if P.Tk > 256:
            rows = m[P.B - 1, 0::2]
            live_rows = rows.sum(-1) > 0
            assert int(rows[:, :256].sum()) == 0 and int(live_rows.sum()) >= rows.shape[0] - 1
    # rising maximum: rows whose largest score lies in the last super-tile / tile, after a smaller maximum in an earlier one
    for key in R.rising_cases():
        P, ref = R.problem(key), R.reference(key)
        tile = R.SK if R.predicted_kernel(P).fast else R.KT
        last = (P.Tk - 1) // tile * tile
        a = ref.a
        top = a.argmax(-1)
        live_before = a[..., :last].sum(-1) > 0
        n = int(((top >= last) & live_before & (ref.lse > ninf)).sum())
        print("%s: %d rows have their dominating key in the last tile of %d" % (key.shape, n, tile))
        assert n >= 4, key
    # the streaming offsets: no cached frame, fewer than `need`, a wrapped interval, a wholly dead first super-tile
    slots = {o: [s for s, _ in R.stream_slots(o)] for offs in R.STREAM_OFFSETS for o in offs}
    assert len(slots[0]) == R.CHUNK and len(slots[8]) == 8 + R.CHUNK and len(slots[590]) == R.NEED + R.CHUNK
    assert slots[590][0] == 274 and slots[590][-1] == 5 and min(slots[876]) == 260 and max(slots[876]) == 291 and slots[299][R.NEED] == 299 and slots[299][-1] == 14
