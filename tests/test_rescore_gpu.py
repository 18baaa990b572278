"""GPU: attention rescoring of n-best lists -- the three kernels of csrc/rescore.hip through the C entry (every operand between guard bands, every
output NaN-prefilled: tests/extent.py), then decoder.TransformerDecoder / AttentionRescorer and transducer.OfflineRecognizer(attention=...) against
the float64 restatement of tests/attention_decoder_ref.py.

Tolerances.  cfm_token_logprob: |out - ref| <= g * S per row, ref in float64 on the operands as rounded, S = the target logit's sum|x||w| + |b| plus
the largest such sum of the row, g = 2 x the largest |error| / S of the SAME formula in plain float32 torch over all of this file's kernel cases
(the factor 2: the kernel sums in another order).  Module level: 4 x the float32 yardstick's error against float64 (attention_decoder_ref.yardstick,
the restatement in float32 with the weights rounded as the mode rounds them; the 4 covers the activations, which the kernels round between stages)."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import attention_decoder_ref as R
import synth
from conftest import load_golden
from extent import Guards

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}


@pytest.fixture(scope="module")
def cfm():
    import cfm as c
    return c


@pytest.fixture
def precision():
    import cfm
    before = cfm.get_precision()
    yield cfm.set_precision
    cfm.set_precision(before)


# ------------------------------------------------------------------------------------------------------------------------- cfm_token_logprob
KERNEL_CASES = [(M, V, D, dt) for M, V, D, dt in itertools.product((1, 63, 65, 130), (3, 17, 5002), (144, 256, 512), ("bf16", "fp16"))]


def logprob_case(M, V, D, dt, kind="plain"):
    """Operands as the kernel sees them (x f32, w 16-bit [Vp, D] with NaN pad rows, bias f32 [Vp] with +1e30 pad entries, targets) and the float64
    reference on the operands as rounded: (x, w, bias, target, Vp, ref logp, ref lse, S, float32-torch logp)."""
    g = torch.Generator().manual_seed(M * 7919 + V * 31 + D + (1 if dt == "fp16" else 0) + (977 if kind != "plain" else 0))
    Vp = (V + 3) // 4 * 4 + 4
    x = torch.randn(M, D, generator=g)
    w = torch.randn(Vp, D, generator=g) * (D ** -0.5)
    bias = torch.randn(Vp, generator=g)
    if kind == "span":                                          # logits spanning +-100: an unshifted exp overflows
        bias = (torch.rand(Vp, generator=g) * 200.0 - 100.0)
        bias[0], bias[V - 1] = 100.0, -100.0
    w16 = w.to(DT[dt])
    w16[V:] = float("nan")
    bias[V:] = 1e30
    target = torch.randint(0, V, (M,), generator=g).to(torch.int32)
    target[0::5], target[1::5], target[2::5] = 0, V - 1, -1
    if M == 1:
        target[0] = V - 1
    if kind == "dead" or M == 130:
        target[64:128] = -1                                     # the second tile of 64 rows is wholly dead
    xr, wr, br = x.to(DT[dt]).double(), w16[:V].double(), bias[:V].double()
    logits = xr @ wr.t() + br
    lse = torch.logsumexp(logits, -1)
    t = target.long().clamp(min=0)
    live = target >= 0
    ref = torch.where(live, logits.gather(1, t[:, None])[:, 0] - lse, torch.zeros(M, dtype=torch.float64))
    Sall = xr.abs() @ wr.abs().t() + br.abs()
    S = Sall.gather(1, t[:, None])[:, 0] + Sall.max(-1).values
    l32 = xr.float() @ wr.float().t() + br.float()
    f32 = torch.where(live, torch.log_softmax(l32, -1).gather(1, t[:, None])[:, 0], torch.zeros(M))
    return x, w16, bias, target, Vp, ref, torch.where(live, lse, torch.zeros_like(lse)), S, f32


ALL_LOGPROB = [c + ("plain",) for c in KERNEL_CASES] + [(130, 5002, 256, "bf16", "span"), (65, 17, 144, "fp16", "span"), (130, 17, 256, "bf16", "dead")]


@pytest.fixture(scope="module")
def g_bound():
    """g: 2 x the float32-torch formula's largest |error| / S over every kernel case of this file, computed once on the CPU."""
    worst = 0.0
    for case in ALL_LOGPROB:
        _, _, _, _, _, ref, _, S, f32 = logprob_case(*case)
        worst = max(worst, float(((f32.double() - ref).abs() / S).max()))
    print("cfm_token_logprob: float32 torch's largest |error| / S = %.3e, g = %.3e" % (worst, 2 * worst))
    return 2 * worst


def run_logprob(cfm, x, w16, bias, target, V, logits=None, ld=None, want_lse=True):
    G = Guards()
    d = cfm.TokenLogprobDesc()
    M = target.numel()
    tg = G.inp(target, name="target")
    logp, lse = G.out((M,), name="logp"), G.out((M,), name="lse") if want_lse else None
    if logits is None:
        xv, wv, bv = G.inp(x, name="X"), G.inp(w16, name="W"), G.inp(bias, name="bias")
        d.X, d.W, d.bias, d.ldx, d.D, d.x_dtype, d.w_dtype = cfm.ptr(xv), cfm.ptr(wv), cfm.ptr(bv), x.shape[1], x.shape[1], cfm.dt_code(xv), cfm.dt_code(wv)
    else:
        lv = G.inp(logits, ld=ld, name="logits")
        d.logits, d.ld = cfm.ptr(lv), ld
    d.target, d.logp, d.lse, d.M, d.V = cfm.ptr(tg), cfm.ptr(logp), cfm.ptr(lse), M, V
    rc = cfm.lib().cfm_token_logprob(ctypes.byref(d), cfm.stream())
    assert rc == 0, cfm.lib().cfm_last_error()
    torch.cuda.synchronize()
    G.check()
    return logp.cpu(), None if lse is None else lse.cpu()


@pytest.mark.parametrize("M,V,D,dt,kind", ALL_LOGPROB, ids=lambda v: str(v))
def test_token_logprob_against_float64(cfm, g_bound, M, V, D, dt, kind):
    x, w16, bias, target, Vp, ref, ref_lse, S, _ = logprob_case(M, V, D, dt, kind)
    got, lse = run_logprob(cfm, x, w16, bias, target, V)
    err = (got.double() - ref).abs()
    print("fused  M=%d V=%d D=%d %s %s: max |err| / S = %.3e (g = %.3e)" % (M, V, D, dt, kind, float((err / S).max()), g_bound))
    assert bool((err <= g_bound * S).all()), (float((err / S).max()), g_bound)
    assert bool(((lse.double() - ref_lse).abs() <= g_bound * S).all())
    assert bool((got[target < 0] == 0).all()) and bool((lse[target < 0] == 0).all())
    again, lse2 = run_logprob(cfm, x, w16, bias, target, V)
    assert torch.equal(again, got) and torch.equal(lse2, lse)                                # the same input, the same bits
    # 16-bit X (already rounded) is the same computation
    got16, _ = run_logprob(cfm, x.to(DT[dt]), w16, bias, target, V, want_lse=False)
    assert torch.equal(got16, got)
    # the logits form over cfm.gemm's f32 logits, at both row strides: pad columns hold +1e30 (the bias), so a kernel that reads them fails
    wd, bd = w16.clone(), bias.to(DEV)
    wd[V:] = 0
    logits = cfm.gemm(x.to(DEV), wd.to(DEV), bias=bd, out_dtype=torch.float32).cpu()
    for ld in (Vp, Vp + 8):
        unf, lse_u = run_logprob(cfm, None, None, None, target, V, logits=logits, ld=ld)
        e2 = (unf.double() - ref).abs()
        assert bool((e2 <= g_bound * S).all()), ("logits form", ld, float((e2 / S).max()), g_bound)
        assert bool(((unf.double() - got.double()).abs() <= g_bound * S).all())
        assert bool((unf[target < 0] == 0).all())
    print("logits M=%d V=%d D=%d %s %s: max |err| / S = %.3e" % (M, V, D, dt, kind, float((e2 / S).max())))


def test_token_logprob_host_validation(cfm):
    x = torch.randn(4, 16, device=DEV)
    w = torch.randn(8, 16, device=DEV).bfloat16()
    b = torch.zeros(8, device=DEV)
    t = torch.tensor([0, 1, -1, 2], dtype=torch.int32, device=DEV)
    lp, lse = cfm.token_logprob(x, w, b, t, 5, want_lse=True)
    assert lp.shape == (4,) and float(lp[2]) == 0.0 and float(lse[2]) == 0.0 and bool((lp[[0, 1, 3]] < 0).all())
    with pytest.raises(RuntimeError, match="multiple of 8"):
        cfm.token_logprob(x[:, :12].contiguous(), w[:, :12].contiguous(), b, t, 5)
    with pytest.raises(RuntimeError, match="bf16 or fp16"):
        cfm.token_logprob(x, w.float(), b, t, 5)
    with pytest.raises(ValueError, match="int32"):
        cfm.token_logprob(x, w, b, t.long(), 5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        cfm.token_logprob(x.cpu(), w, b, t, 5)
    assert bool(torch.isnan(cfm.token_logprob(x, w, b, torch.tensor([7, 0, 0, 0], dtype=torch.int32, device=DEV), 5)[0]))     # target >= V


# -------------------------------------------------------------------------------------------------------------------------- cfm_rescore_prep
@pytest.mark.parametrize("N,Lmax", [(1, 1), (3, 7), (16, 40), (3, 40), (16, 1)])
@pytest.mark.parametrize("reverse", [False, True])
def test_rescore_prep(cfm, N, Lmax, reverse):
    B, D, V = 2, 24, 19
    g = torch.Generator().manual_seed(N * 100 + Lmax)
    tokens = torch.randint(0, V - 1, (B, N, Lmax), generator=g).to(torch.int32)
    nlen = torch.randint(0, Lmax + 1, (B, N), generator=g).to(torch.int32)
    score = -torch.rand(B, N, generator=g)
    nlen[0, 0] = 0                                              # only sos -> eos
    nlen[1, N - 1] = Lmax
    if N > 1:
        nlen[1, 0] = -1                                         # unused by its length
        score[0, N - 1] = float("-inf")                         # unused by its score
    E, Er = torch.randn(V, D, generator=g), torch.randn(V, D, generator=g)
    pe = R._sinusoid_table(Lmax + 3, D)[:, 0].contiguous()
    Lc, P = Lmax + 1, B * N
    G = Guards()
    d = cfm.RescorePrepDesc()
    keep = [G.inp(tokens, name="tokens"), G.inp(nlen, name="nlen"), G.inp(score, name="score"), G.inp(E, name="embed"), G.inp(Er, name="embed_r") if reverse else None,
            G.inp(pe, name="pe")]
    d.tokens, d.nlen, d.score, d.embed, d.embed_r, d.pe = (cfm.ptr(t) for t in keep)
    x0, tg, mask = G.out((P * Lc, D), name="x0"), G.out((P, Lc), torch.int32, name="targets"), G.out((P, Lc, Lc), torch.uint8, name="mask")
    x0r, tgr = (G.out((P * Lc, D), name="x0_r"), G.out((P, Lc), torch.int32, name="targets_r")) if reverse else (None, None)
    d.x0, d.x0_r, d.targets, d.targets_r, d.mask = (cfm.ptr(t) for t in (x0, x0r, tg, tgr, mask))
    d.B, d.N, d.Lmax, d.D, d.V, d.sos, d.eos = B, N, Lmax, D, V, V - 1, V - 2
    rc = cfm.lib().cfm_rescore_prep(ctypes.byref(d), cfm.stream())
    assert rc == 0, cfm.lib().cfm_last_error()
    torch.cuda.synchronize()
    G.check()
    for rev, xg, tgg, table in ((False, x0, tg, E),) + (((True, x0r, tgr, Er),) if reverse else ()):
        tin, want_tg, want_mask = R.prep(tokens, nlen, score, V - 1, V - 2, rev)
        assert torch.equal(tgg.cpu().long(), want_tg) and torch.equal(mask.cpu().bool(), want_mask) and int(mask.max()) <= 1
        live = (want_tg >= 0).reshape(-1)
        want = (table.double()[tin] * np.sqrt(float(D)) + pe[:Lc].double()).reshape(P * Lc, D)
        got = xg.cpu()
        assert bool((got[~live] == 0).all())
        w32 = want.float()
        ulp = torch.maximum((torch.nextafter(w32, torch.full_like(w32, float("inf"))) - w32).double(), (w32 - torch.nextafter(w32, torch.full_like(w32, float("-inf")))).double())
        assert bool(((got.double() - want).abs()[live] <= ulp[live]).all())
    dead = (nlen < 0) | (score == float("-inf"))
    assert int(mask.cpu().view(B, N, -1)[dead].sum()) == 0 and bool((tg.cpu().view(B, N, -1)[dead] == -1).all())


# ----------------------------------------------------------------------------------------------------------------------- cfm_rescore_combine
@pytest.mark.parametrize("N,Lc,rw", [(1, 1, 0.0), (4, 9, 0.0), (16, 41, 0.3), (5, 33, 0.3)])
def test_rescore_combine(cfm, N, Lc, rw):
    B, fpw = 3, 0.5
    g = torch.Generator().manual_seed(N + Lc)
    logp = -torch.rand(B, N, Lc, generator=g) * 5
    logp_r = -torch.rand(B, N, Lc, generator=g) * 5
    nlen = torch.full((B, N), Lc - 1, dtype=torch.int32)
    score = -torch.rand(B, N, generator=g)
    if N >= 4:                                                  # planted exact ties and unused slots
        logp[0, 2], logp_r[0, 2], score[0, 2] = logp[0, 0], logp_r[0, 0], score[0, 0]
        logp[1, 3], logp_r[1, 3], score[1, 3] = logp[1, 1], logp_r[1, 1], score[1, 1]
        score[2, 1] = float("-inf")
        nlen[2, 2] = -1
        score[0, 1] = float("-inf")
    G = Guards()
    d = cfm.RescoreCombineDesc()
    keep = [G.inp(logp, name="logp"), G.inp(logp_r, name="logp_r") if rw > 0 else None, G.inp(nlen, name="nlen"), G.inp(score, name="score")]
    d.logp, d.logp_r, d.nlen, d.score = (cfm.ptr(t) for t in keep)
    outs = [G.out((B, N), name="final"), G.out((B, N), name="left"), G.out((B, N), name="right"), G.out((B, N), torch.int32, name="order")]
    d.final_score, d.left, d.right, d.order = (cfm.ptr(t) for t in outs)
    d.B, d.N, d.Lc, d.first_pass_weight, d.reverse_weight = B, N, Lc, fpw, rw
    rc = cfm.lib().cfm_rescore_combine(ctypes.byref(d), cfm.stream())
    assert rc == 0, cfm.lib().cfm_last_error()
    torch.cuda.synchronize()
    G.check()
    final, left, right, order = (t.cpu() for t in outs)

    def seq_sum(t):                                             # float32, one add per position, in position order
        acc = np.zeros(t.shape[:2], dtype=np.float32)
        for i in range(t.shape[2]):
            acc = (acc + t[:, :, i].numpy()).astype(np.float32)
        return acc
    wl, wr = seq_sum(logp), seq_sum(logp_r) if rw > 0 else np.zeros((B, N), dtype=np.float32)
    assert np.array_equal(left.numpy(), wl) and np.array_equal(right.numpy(), wr)
    f32 = np.float32
    att = wl if rw == 0 else (f32(1.0 - f32(rw)) * wl).astype(f32) + (f32(rw) * wr).astype(f32)
    want = (att + (f32(fpw) * score.numpy()).astype(f32)).astype(f32)
    want[((nlen < 0) | (score == float("-inf"))).numpy()] = -np.inf
    assert np.array_equal(final.numpy(), want)
    assert order.tolist() == [R.rank(row.tolist()) for row in final]
    if N >= 4:
        o = order[0].tolist()
        assert o.index(0) < o.index(2) and o[-1] == 1 and order[2].tolist()[-2:] == [1, 2]


# ------------------------------------------------------------------------------------------------------------------------------ module level
@pytest.fixture(scope="module")
def module_refs():
    """Per (seed, T): the case and the restatement's float64 results, computed once."""
    out = {}
    for seed in R.SEEDS:
        for T in R.FRAMES:
            case = R.module_case(seed, T)
            dec, memory, enc_lens, nbest = case
            targets, lengths, owner = R.forward_case(dec, nbest)
            out[seed, T] = dict(case=case, left=R.module_reference(*case, 0.0), bi=R.module_reference(*case, R.CASE["reverse_weight"]),
                                fwd=(targets, lengths, owner, R.forward_reference(dec.left_decoder.state_dict(), targets, lengths, memory, enc_lens, owner)))
    return out


@pytest.mark.parametrize("mode", ["bf16", "fp16", "fp32"])
def test_decoder_and_rescorer_against_the_restatement(cfm, precision, module_refs, mode):
    import copy
    import decoder
    precision(mode)
    c = R.CASE
    yard = {rw: [max(R.yardstick(mode, s, T, rw)[k] for s in R.SEEDS for T in R.FRAMES) for k in (0, 1)] for rw in (0.0, c["reverse_weight"])}
    gate_logits = 4 * yard[0.0][1]
    worst_logits, worst_final, exempt, total = 0.0, {0.0: 0.0, c["reverse_weight"]: 0.0}, 0, 0
    for (seed, T), ref in module_refs.items():
        dec_cpu, memory, enc_lens, nbest = ref["case"]
        dec = copy.deepcopy(dec_cpu).to(DEV).eval()
        mem = memory.to(DEV)
        targets, lengths, owner, want_logits = ref["fwd"]
        mm = (torch.arange(T).unsqueeze(0) < torch.tensor(enc_lens).unsqueeze(1)).unsqueeze(1)
        logits, zero, out_lens = dec.left_decoder(mem[owner], mm[owner].to(DEV), targets.to(DEV), lengths.to(DEV))
        assert tuple(logits.shape) == tuple(want_logits.shape) and float(zero) == 0.0 and tuple(out_lens.shape) == (len(owner), targets.shape[1])
        valid = torch.arange(targets.shape[1]).unsqueeze(0) < lengths.long().unsqueeze(1)
        worst_logits = max(worst_logits, float((logits.cpu().double() - want_logits)[valid].abs().max()))
        for rw, key in ((0.0, "left"), (c["reverse_weight"], "bi")):
            gate = 4 * yard[rw][0]
            want_final, want_left, want_right, want_order = ref[key]
            rs = decoder.AttentionRescorer(dec, first_pass_weight=c["first_pass_weight"], reverse_weight=rw)
            got = rs.rescore(mem, enc_lens, nbest, return_details=True)
            for fused in (True, False):                           # both forms of the output step
                rs.fused = fused
                tokens, nlen, score = (t.to(DEV) for t in R.pack_nbest(nbest))
                final, left, right, order = (t.cpu() for t in rs.scores(mem, torch.tensor(enc_lens), tokens, nlen, score))
                used = want_final > float("-inf")
                assert bool((final[~used] == float("-inf")).all())
                worst_final[rw] = max(worst_final[rw], float((final.double() - want_final)[used].abs().max()))
                for b in range(c["B"]):
                    total += 1
                    if R.min_gap(want_final[b].tolist()) > 2 * gate:
                        assert order[b].tolist() == want_order[b], (seed, T, rw, fused, b)
                    else:
                        exempt += 1
            for b, entries in enumerate(got):                     # the list form: the same hypotheses, re-ranked, with their details
                assert sorted(tuple(e[0]) for e in entries) == sorted(tuple(t) for t, _ in nbest[b])
                assert [e[1] for e in entries] == sorted((e[1] for e in entries), reverse=True)
                for tk, f, det in entries:
                    n = [t for t, _ in nbest[b]].index(tk)
                    assert det["first_pass"] == pytest.approx(nbest[b][n][1]) and abs(f - float(want_final[b, n])) <= gate
    print("%s: logits |err| %.3e (yardstick %.3e, gate %.3e); final left-only %.3e (yardstick %.3e), bidirectional %.3e (yardstick %.3e); %d of %d ranking checks exempt"
          % (mode, worst_logits, yard[0.0][1], gate_logits, worst_final[0.0], yard[0.0][0], worst_final[c["reverse_weight"]], yard[c["reverse_weight"]][0], exempt, total))
    assert worst_logits <= gate_logits
    for rw in worst_final:
        assert worst_final[rw] <= 4 * yard[rw][0], (rw, worst_final[rw], yard[rw][0])
    assert exempt <= 0.1 * total


def test_weight_change_invalidates_the_packs(cfm, precision, module_refs):
    import copy
    import decoder
    precision("bf16")
    dec_cpu, memory, enc_lens, nbest = module_refs[0, 5]["case"]
    dec = copy.deepcopy(dec_cpu).to(DEV).eval()
    rs = decoder.AttentionRescorer(dec)
    a = rs.rescore(memory.to(DEV), enc_lens, nbest)
    assert rs.rescore(memory.to(DEV), enc_lens, nbest) == a
    with torch.no_grad():
        dec.left_decoder.output_layer.bias[3] += 5.0
        dec.left_decoder.decoders[0].src_attn.linear_k.weight.mul_(1.5)
    assert rs.rescore(memory.to(DEV), enc_lens, nbest) != a


# ------------------------------------------------------------------------------------------------------------------------- OfflineRecognizer
def test_offline_recognizer_rescore(cfm, precision):
    import decoder
    import transducer
    from test_edit_distance_gpu import offline_recognizer
    precision("fp32")
    _, meta = load_golden("offline_asr")
    plain, (enc, pr, jn) = offline_recognizer(meta)
    V, D = meta["head"]["V"], meta["cfg"]["encoder_dim"]
    torch.manual_seed(77)
    att = decoder.BiTransformerDecoder(V, D, 4, 2 * D, 2, 1, 0.0, 0.0, 0.0, 0.0).eval().to(DEV)
    rec = transducer.OfflineRecognizer(enc, pr, jn, blank=meta["blank"], n_steps=meta["n_steps"], ctc=plain.ctc, attention=att, first_pass_weight=0.3, reverse_weight=0.3)
    lens = torch.tensor(meta["lens"], dtype=torch.int32, device=DEV)
    x = torch.from_numpy(synth.fbank(meta["xseed"], len(meta["lens"]), max(meta["lens"]))).to(DEV)
    for fn, fn_plain in ((rec.recognize_ctc, plain.recognize_ctc), (rec.recognize, plain.recognize)):
        first = fn_plain(x, lens, beam=4)
        assert fn(x, lens, beam=4) == first and fn(x, lens) == fn_plain(x, lens)              # without rescore: identical to a recogniser without attention
        got = fn(x, lens, beam=4, rescore=True)
        direct = rec.rescorer.rescore(rec.encoder_out, rec.encoder_out_lens, first)
        assert got == direct
        for a, b in zip(got, first):                                                         # a permutation of the un-rescored list
            assert sorted(tuple(t) for t, _ in a) == sorted(tuple(t) for t, _ in b)
            assert [s for _, s in a] == sorted((s for _, s in a), reverse=True)
        with pytest.raises(ValueError, match="beam=k"):
            fn(x, lens, rescore=True)
    with pytest.raises(RuntimeError, match="without an attention decoder"):
        plain.recognize(x, lens, beam=4, rescore=True)
