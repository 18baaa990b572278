"""CPU: tests/rowchain_ref.py -- the float64 restatement of cfm_rowchain that tests/test_rowchain_matrix_gpu.py compares the kernels with -- checked
without the library: (a) against torch's own operators in float64, (b) the float32 yardstick against the bound at every case of the matrix, every
reference value finite, (c) a discrimination audit: every way the kernel could plausibly be wrong (rowchain_ref.VARIANTS), restated in float64,
differs from the right result by more than 10 x the bound on at least one element of the very inputs the GPU test uses, (d) the instance names of
csrc/rowchain.hip against rowchain_ref.INSTANCES.  The tables are printed (pytest -s)."""
import os
import re

import torch
import torch.nn.functional as F

import rowchain_ref as R

HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "conformer-pytorch-lightning_amd", "csrc", "rowchain.hip")


def eq(a, b):
    torch.testing.assert_close(a, b, rtol=1e-11, atol=1e-11)


def r16(t, wdt):
    return t.to(R.W_DT[wdt]).double()


def deinterleave(w, b):
    """row blk*32 + half*16 + i of the GLU-interleaved weight is row half*(N/2) + blk*16 + i of the plain [value | gate] weight."""
    N = w.shape[0]
    idx = torch.arange(N)
    dst = ((idx % 32) // 16) * (N // 2) + (idx // 32) * 16 + (idx % 16)
    W, bb = torch.empty_like(w), torch.empty_like(b)
    W[dst], bb[dst] = w, b
    return W.double(), bb.double()


def test_reference_agrees_with_torch():
    """the three roles and the depthwise stage written with torch.nn.functional on the same rounded operands."""
    for wdt in ("bf16", "fp16"):
        ln = lambda t, pr: F.layer_norm(t, (t.shape[1],), pr[0].double(), pr[1].double(), 1e-5)
        lin = lambda a, w, b: F.linear(a, w.double(), b.double())
        # macaron
        p, w = R.problem("macaron", 144, wdt, (33,)), R.weights(144, wdt)
        r = R.evaluate(p)
        x = p.x.double()
        x1 = x + 0.5 * lin(r16(F.silu(lin(r16(ln(x, w.ln_ffm), wdt), w.ffm_w1, w.ffm_b1)), wdt), w.ffm_w2, w.ffm_b2)
        eq(r["out_f32"], x1)
        eq(r["tail_out"], lin(r16(ln(x1, w.ln_mha), wdt), w.qkv_w, w.qkv_b))
        # conv-in on a ragged batch
        p = R.problem("convin_len", 144, wdt, (5, 13))
        r = R.evaluate(p)
        x2 = p.head_res.double() + lin(p.head_a.double(), w.out_w, w.out_b)
        eq(r["out_f32"], x2)
        W, b = deinterleave(w.pw1_w, w.pw1_b)
        g = F.glu(lin(r16(ln(x2, w.ln_conv) * p.ln_mask[:, None].double(), wdt), W, b), dim=1).reshape(5, 13, 144)
        for bi, n in enumerate(p.glu_len.tolist()):
            g[bi, n:] = 0
        eq(r["tail_out"], g.reshape(65, 144))
        # depthwise stage + final chain + after-norm
        p = R.problem("dwfinal_after", 144, wdt, (5, 13))
        r = R.evaluate(p)
        a = p.head_a.double().reshape(5, 13, 144).transpose(1, 2)
        cv = F.conv1d(a, w.dw_w.double()[:, None, :], w.dw_b.double(), padding=7, groups=144).transpose(1, 2).reshape(65, 144)
        dwo = r16(F.silu(cv * w.bn_scale.double() + w.bn_shift.double()), wdt)
        x3 = p.head_res.double() + lin(dwo, w.pw2_w, w.pw2_b) * p.head_mask[:, None].double()
        y = x3 + 0.5 * lin(r16(F.silu(lin(r16(ln(x3, w.ln_ff), wdt), w.ff_w1, w.ff_b1)), wdt), w.ff_w2, w.ff_b2)
        eq(r["out_f32"], ln(y, w.ln_final))
        eq(r["out2_f32"], ln(ln(y, w.ln_final), w.after))
        # the pair split: the halves and the reduce put the macaron chain together again
        p = R.problem("pair_macaron_half", 512, wdt, (33,))
        w5 = R.weights(512, wdt)
        r = R.evaluate(p)
        x = p.x.double()
        h = r16(F.silu(lin(r16(ln(x, w5.ln_ffm), wdt), w5.ffm_w1, w5.ffm_b1)), wdt)
        eq(r["psum_out"][0] + r["psum_out"][1], F.linear(h, w5.ffm_w2.double()))
        q = R.problem("pair_qkv", 512, wdt, (33,))
        eq(R.evaluate(q)["out_f32"], q.x.double() + 0.5 * (q.psum_in[0].double() + q.psum_in[1].double() + w5.ffm_b2.double()))


def test_conv_in_stage_is_the_conv_in_chain_in_front_of_the_depthwise_chain():
    """cin_*: the same function as conv_in_chain followed by final_chain + next_macaron on its outputs."""
    for rows in ((5, 13), (1, 100)):
        p = R.problem("cin_apart", 256, "bf16", rows)
        w = R.weights(256, "bf16")
        r = R.evaluate(p)
        ci = R.SimpleNamespace(**vars(R.problem("convin_len", 256, "bf16", rows)))
        ci.head_a, ci.head_res, ci.ln_mask, ci.glu_len = p.cin_a, p.cin_res, p.cin_mask, p.glu_len
        a = R.evaluate(ci)
        eq(r["cin_out"], a["out_f32"])
        fi = R.SimpleNamespace(**vars(R.problem("dwfinal_macaron", 256, "bf16", rows)))
        fi.head_a, fi.head_res, fi.head_mask = a["tail_out"].to(torch.bfloat16), a["out_f32"], p.head_mask
        b = R.evaluate(fi)
        eq(r["s2_out_f32"], b["s2_out_f32"])
        eq(r["tail_out"], b["tail_out"])
        assert w.FF == 2048


def test_fragment_major_is_the_header_formula():
    w = torch.arange(32 * 40, dtype=torch.float32).reshape(32, 40)
    f = R.frag_major(w, torch.float32)
    KS = 2
    for nfrag, kk, lane, j in ((0, 0, 0, 0), (1, 1, 37, 5), (1, 0, 63, 7), (0, 1, 16, 0)):
        n, k = nfrag * 16 + (lane & 15), kk * 32 + 8 * (lane >> 4) + j
        assert float(f[((nfrag * KS + kk) * 64 + lane) * 8 + j]) == (float(w[n, k]) if k < 40 else 0.0)


def test_yardstick_stays_within_the_bound_and_the_reference_is_finite():
    """g = 4 x the worst float32-torch ratio; the yardstick differs from the reference by float32 rounding and, rarely, by one flipped rounding of a 16-bit
    intermediate -- one ulp (2^-8 of a bf16 operand element) of one term of a sum, so well below 2^-8 of the row's largest output."""
    G = R.measure_g()
    print("\nfloat32 torch over %d cases, worst per-row |d| / max|ref| (16-bit outputs: beyond one ulp) -> g" % len(R.cases()))
    for k in R.KINDS:
        print("%-12s %.3g -> %.3g" % (k, G[k][1], G[k][0]))
    assert 0 < G["direct"][1] < 2.0 ** -18                   # float32 rounding through a K = 512 product, a reduce and a LayerNorm
    assert all(0 < G[k][1] < 2.0 ** -8 for k in R.KINDS)
    for key in R.cases():
        p, r = R.problem(*key), R.reference(key)
        t = R.evaluate(p, torch.float32)
        assert set(r) == {ref for _, ref in p.compare} | ({"cin_out"} if key[0] == "cin" else set()), key
        for name, ref in r.items():
            assert bool(torch.isfinite(ref).all()), (key, name)
            dt = R.out_dtype(p, name)
            got = t[name] if dt == R.F32 else t[name].to(dt)
            assert R.row_ratio(got, ref, dt) <= G[R.kind(p, name)][0], (key, name)


def test_every_wrong_variant_is_separated():
    G = R.measure_g()
    table = []
    for name, key in R.VARIANTS.items():
        p = R.problem(*key)
        right, wrong = R.reference(key), R.evaluate(p, variant=name)
        worst, where = 0.0, None
        for out, ref in right.items():
            dt = R.out_dtype(p, out)
            bound = G[R.kind(p, out)][0] * R.row_scale(ref) + R.ulp(ref, dt)
            x = float(((wrong[out] - ref).abs() / bound.clamp_min(1e-300)).max())
            if x > worst:
                worst, where = x, out
        table.append((name, "%s D=%d %s" % (key[0], key[1], "x".join(map(str, key[3]))), where, worst))
    print("\n%-28s %-28s %-12s %s" % ("variant", "case", "output", "worst |wrong - right| / bound"))
    for row in table:
        print("%-28s %-28s %-12s %.3g" % row)
    for name, case, _, worst in table:
        assert worst > 10.0, "%s is not separated at %s: %.3g x the bound" % (name, case, worst)


def test_every_instance_of_the_dispatch_has_a_case():
    """the "chain_..." names of csrc/rowchain.hip == the names rowchain_ref.INSTANCES pins, for both weight types: a new instance without a case fails here."""
    with open(HIP) as f:
        names = set(re.findall(r'"(chain_[a-z0-9_]+)"', f.read()))
    assert names == R.instance_names(), (sorted(names - R.instance_names()), sorted(R.instance_names() - names))
    assert len(names) == 48
