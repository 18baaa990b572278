"""GPU: beam search with the attention decoder -- the two kernels of csrc/attn_search.hip through the C entry (operands between guard bands,
outputs NaN-prefilled: tests/extent.py), then decoder.AttentionBeamSearch and transducer.OfflineRecognizer.recognize_attention against the float64
search of tests/attention_search_ref.py, which has no cache.

Tolerances.  cfm_dec_step_attn: |out - ref| <= g * S per (row, head) plus one rounding of the output type, ref in float64 on the operands as
rounded, S = max_j |v_j| (1 + max_j |s_j|) over the attended keys: a convex combination is bounded by max |v|, and a rounding of the exponent's
argument at magnitude |s| is a relative error |s| eps of the weight; g = 2 x the largest |error| / S of the SAME formula in plain float32 torch over
this file's own cases, computed on the CPU and printed.  cfm_dec_beam_prune: integers and scores exact.  Search: a hypothesis's
delta is (its length + 1) x the per-position gate, the gate 4 x attention_search_ref.yardstick(mode, case) (the module-level rule of
test_rescore_gpu.py); the protocol is test_rnnt_beam_gpu.py's."""
import copy
import ctypes
import math

import numpy as np
import pytest
import torch

import attention_search_ref as SR
from extent import Guards

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
EPS = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11, "fp32": 2.0 ** -24}


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


# ------------------------------------------------------------------------------------------------------------------------- cfm_dec_step_attn
# R, H, dk, dtype, form
ATTN_CASES = [(R, H, dk, dt, "table") for R in (1, 5, 33) for H, dk in ((4, 36), (4, 64), (4, 128), (1, 64)) for dt in ("bf16", "fp32")] + \
             [(5, 4, 64, "fp16", "table"), (33, 4, 36, "fp16", "append"), (5, 4, 64, "bf16", "append"), (33, 4, 128, "fp32", "append"), (5, 4, 64, "bf16", "step"),
              (6, 4, 64, "bf16", "cross"), (33, 4, 36, "fp32", "cross"), (12, 1, 64, "fp16", "cross")]
COUNTS = (1, 2, 63, 64, 65, 129, 257, 0)


def attn_case(R, H, dk, dt, form):
    """Operands as the kernel sees them and the float64 reference on the operands as rounded."""
    g = torch.Generator().manual_seed(R * 131 + H * 17 + dk + len(form) + len(dt))
    D, cap = H * dk, 257
    t = DT[dt]
    q = torch.randn(R, D, generator=g).to(t)
    c = dict(q=q, D=D, cap=cap, kv_new=None, slot=None, step=None, group=1, stride=0)
    if form == "cross":
        owners = 3
        group = R // owners
        c.update(group=group, stride=cap, slots=owners * cap, klen=torch.tensor([257, 65, 0] if R > 6 else [129, 2, 63], dtype=torch.int32))
        rows_klen = c["klen"].repeat_interleave(group)
        table = (torch.arange(R) // group * cap).unsqueeze(1) + torch.arange(cap).unsqueeze(0)
    else:
        slots = cap * 3
        # a random permutation with shared ancestors: rows are grouped in families that share a prefix of slots
        perm = torch.randperm(slots, generator=g)
        fam = torch.arange(R) % 3
        table = perm[(fam.unsqueeze(1) * cap + torch.arange(cap).unsqueeze(0)) % slots].clone()
        klen = torch.tensor([COUNTS[r % len(COUNTS)] for r in range(R)], dtype=torch.int32)
        if form == "step":
            klen = torch.full((R,), 65, dtype=torch.int32)
            c["step"] = torch.tensor([64], dtype=torch.int32)
        if form == "append":                                                            # the appended slot is the row's own: no other row names it
            table = perm[(fam.unsqueeze(1) * 64 + torch.arange(cap).unsqueeze(0)) % (3 * 64)].clone()      # families live in 192 slots ...
            spare = perm[192:192 + R]                                                   # ... and every row appends to a slot outside them
            for r in range(R):
                if klen[r] > 0:
                    table[r, klen[r] - 1] = spare[r]
            c["kv_new"] = torch.randn(R, 2 * D, generator=g).to(t)
        c.update(slots=slots, klen=None if form == "step" else klen, slot=table.to(torch.int32))
        rows_klen = klen
    store = torch.randn(c["slots"], 2 * D, generator=g).to(t)
    c.update(store=store, table=table, rows_klen=rows_klen)
    # float64 on the operands as rounded; the float32-torch restatement of the same formula beside it
    eff = store.clone()
    if c["kv_new"] is not None:
        for r in range(R):
            if rows_klen[r] > 0:
                eff[table[r, rows_klen[r] - 1]] = c["kv_new"][r]
    ref, f32, S = torch.zeros(R, D, dtype=torch.float64), torch.zeros(R, D), torch.zeros(R, H, dtype=torch.float64)
    for r in range(R):
        n = int(rows_klen[r])
        if n == 0:
            continue
        rows = eff[table[r, :n]]
        for h in range(H):
            sl = slice(h * dk, (h + 1) * dk)
            for acc, dtype in ((ref, torch.float64), (f32, torch.float32)):
                k, v, qq = rows[:, sl].to(dtype), rows[:, D + h * dk:D + (h + 1) * dk].to(dtype), q[r, sl].to(dtype)
                p = torch.softmax((k @ qq) / math.sqrt(dk), 0)
                acc[r, sl] = p @ v
            smax = float(((rows[:, sl].double() @ q[r, sl].double()) / math.sqrt(dk)).abs().max())
            S[r, h] = float(rows[:, D + h * dk:D + (h + 1) * dk].double().abs().max()) * (1.0 + smax)
    c.update(ref=ref, f32=f32, S=S.repeat_interleave(dk, 1), eff=eff)
    return c


@pytest.fixture(scope="module")
def g_attn():
    worst = 0.0
    for case in ATTN_CASES:
        c = attn_case(*case)
        live = c["S"] > 0
        worst = max(worst, float(((c["f32"].double() - c["ref"]).abs()[live] / c["S"][live]).max()))
    print("cfm_dec_step_attn: float32 torch's largest |error| / S = %.3e, g = %.3e" % (worst, 2 * worst))
    return 2 * worst


@pytest.mark.parametrize("R,H,dk,dt,form", ATTN_CASES, ids=lambda v: str(v))
def test_step_attention_against_float64(cfm, g_attn, R, H, dk, dt, form):
    c = attn_case(R, H, dk, dt, form)
    D = c["D"]
    G = Guards()
    d = cfm.DecStepAttnDesc()
    q, slot, klen, step = G.inp(c["q"], name="q"), G.inp(c["slot"], name="slot"), G.inp(c.get("klen"), name="klen"), G.inp(c["step"], name="step")
    store = G.io(c["store"], name="store") if form == "append" else G.inp(c["store"], name="store")
    kv_new = G.inp(c["kv_new"], name="kv_new")
    out = G.out((R, D), DT[dt], name="out")
    d.q, d.store, d.slot, d.klen, d.step, d.kv_new, d.out = (cfm.ptr(t) for t in (q, store, slot, klen, step, kv_new, out))
    d.ldq, d.ld_new, d.ldo, d.slots = D, 2 * D, D, c["slots"]
    d.R, d.H, d.dk, d.cap, d.io_dtype = R, H, dk, c["cap"], cfm.dt_code(q)
    d.slot_ld = 0 if slot is None else c["cap"]
    d.group, d.stride, d.klen_group = c["group"], c["stride"], c["group"]
    rc = cfm.lib().cfm_dec_step_attn(ctypes.byref(d), cfm.stream())
    assert rc == 0, cfm.lib().cfm_last_error()
    torch.cuda.synchronize()
    G.check()
    got = out.cpu().double()
    bound = g_attn * c["S"] + EPS[dt] * c["ref"].abs()                                        # + one rounding of the output type
    err = (got - c["ref"]).abs()
    live = c["S"] > 0
    print("step attention R=%d H=%d dk=%d %s %s: max |err| / S = %.3e (g = %.3e + %.1e)" % (R, H, dk, dt, form, float((err[live] / c["S"][live]).max()) if bool(live.any()) else 0.0,
                                                                                            g_attn, EPS[dt]))
    assert not torch.isnan(got).any() and bool((err <= bound).all())
    assert bool((got[c["rows_klen"] == 0] == 0).all())                                   # a key count of 0 writes zeros
    if form == "append":                                                                # exactly one slot per row, no other touched
        assert torch.equal(store.cpu().view(torch.uint8), c["eff"].view(torch.uint8))


def test_step_attention_limits(cfm):
    q = torch.zeros(4, 64, device=DEV).bfloat16()
    store = torch.zeros(32, 128, device=DEV).bfloat16()
    slot = torch.zeros(4, 8, dtype=torch.int32, device=DEV)
    klen = torch.ones(4, dtype=torch.int32, device=DEV)
    assert cfm.dec_step_attn(q, store, 4, klen=klen, slot=slot).shape == (4, 64)
    with pytest.raises(RuntimeError, match="capacity"):
        cfm.dec_step_attn(q, store, 4, klen=klen, slot=slot, cap=9)                      # a key count above the table's columns
    with pytest.raises(RuntimeError, match="capacity"):
        cfm.dec_step_attn(q, store, 4, klen=klen, group=2, stride=17)                    # the second owner's rows leave the store
    with pytest.raises(RuntimeError, match="dk"):
        cfm.dec_step_attn(torch.zeros(4, 136, device=DEV).bfloat16(), torch.zeros(32, 272, device=DEV).bfloat16(), 1, klen=klen, slot=slot)      # dk = 136
    with pytest.raises(RuntimeError, match="multiple of 8"):
        cfm.dec_step_attn(torch.zeros(4, 12, device=DEV).bfloat16(), torch.zeros(32, 24, device=DEV).bfloat16(), 1, klen=klen, slot=slot)        # D = 12
    with pytest.raises(RuntimeError, match="no CPU path"):
        cfm.dec_step_attn(q.cpu(), store, 4, klen=klen, slot=slot)


# ------------------------------------------------------------------------------------------------------------------------ cfm_dec_beam_prune
def prune_state(B, K, Lmax, D, step, g):
    """A mid-search state at the given per-utterance steps, on the CPU: dict of tensors as cfm.dec_beam_prune takes them."""
    R = B * K
    i32 = torch.int32
    S = dict(score=-torch.rand(R, generator=g) * 3, token=torch.zeros(R, dtype=i32), parent=torch.full((R,), -1, dtype=i32), finished=torch.zeros(R, dtype=torch.uint8),
             hlen=torch.zeros(R, dtype=i32), klen=torch.zeros(R, dtype=i32), tokens=torch.randint(0, 9, (R, Lmax), generator=g).to(i32),
             slots=torch.randint(0, R * Lmax, (R, Lmax), generator=g).to(i32), x=torch.zeros(R, D), step=torch.tensor(step, dtype=i32),
             max_len=torch.full((B,), Lmax, dtype=i32), done=torch.zeros(B, dtype=torch.uint8), n_done=torch.zeros(1, dtype=i32), all_done=torch.zeros(1, dtype=i32),
             nbest_tokens=torch.full((B, K, Lmax), -7, dtype=i32), nbest_len=torch.full((B, K), -7, dtype=i32), nbest_score=torch.full((B, K), 7.0))
    for b in range(B):
        S["hlen"][b * K:(b + 1) * K] = step[b]
        S["klen"][b * K:(b + 1) * K] = step[b] + 1
    return S


def run_prune(cfm, S, idx, logp, E, pe, eos, V):
    G = Guards()
    Sg = {k: G.io(v, name=k) for k, v in S.items()}
    cfm.dec_beam_prune(G.inp(idx, name="topk_idx"), G.inp(logp, name="topk_logp"), Sg, G.inp(E, name="embed"), G.inp(pe, name="pe"), eos, V)
    torch.cuda.synchronize()
    G.check()
    return {k: v.cpu() for k, v in Sg.items()}


def test_prune_against_the_specification(cfm):
    B, K, Lmax, D, V, eos = 4, 4, 6, 24, 11, 10
    g = torch.Generator().manual_seed(5)
    R = B * K
    step = [2, 3, 5, 1]                              # utterance 2 is at its last step (max_len); utterance 3 is done already
    S = prune_state(B, K, Lmax, D, step, g)
    S["done"][3], S["n_done"][0] = 1, 1
    S["token"][12:16] = torch.tensor([3, 4, 5, 6], dtype=torch.int32)
    idx = torch.stack([torch.randperm(V - 1, generator=g)[:K] for _ in range(R)]).to(torch.int32)
    logp = -torch.sort(torch.rand(R, K, generator=g) * 4).values
    # utterance 0: ties.  rows 0 and 1 have equal scores and equal first log-probabilities -> the better parent first; row 0's two best
    # classes have equal log-probabilities -> the lower class first
    S["score"][0] = S["score"][1] = -0.5
    logp[0, 0] = logp[0, 1] = logp[1, 0] = -0.25
    idx[0, 0], idx[0, 1] = 2, 7
    # utterance 1: finished carry-over.  row 4 is finished with the best score, row 5 offers eos as its best class: all kept finish -> done
    S["finished"][4], S["score"][4], S["hlen"][4] = 1, -0.01, 2
    S["tokens"][4, 2] = eos
    S["score"][5], S["score"][6], S["score"][7] = -0.02, -50.0, -60.0
    idx[5] = torch.tensor([eos, 1, 2, 3], dtype=torch.int32)
    logp[5] = torch.tensor([-0.001, -20.0, -21.0, -22.0])
    S["finished"][6] = S["finished"][7] = 1
    S["score"][6], S["score"][7] = -0.03, -0.04
    E, pe = torch.randn(V, D, generator=g), torch.randn(Lmax + 2, D, generator=g)
    before = {k: v.clone() for k, v in S.items()}
    got = run_prune(cfm, S, idx, logp, E, pe, eos, V)
    for b in range(B):
        rows = slice(b * K, (b + 1) * K)
        i = step[b]
        if b == 3:                                                                      # done: identity indices, everything frozen, x from the frozen token
            assert got["parent"][rows].tolist() == list(range(12, 16))
            for k in ("score", "token", "finished", "hlen", "klen", "tokens", "slots"):
                assert torch.equal(got[k][rows], before[k][rows]), k
            want_x = (E[before["token"][rows].long()].double() * math.sqrt(D) + pe[i].double()).float()
            assert torch.equal(got["x"][rows], want_x)
            continue
        kept = SR.prune_ref(idx[rows].numpy(), logp[rows].numpy(), before["score"][rows].numpy(), before["finished"][rows].numpy().astype(bool), K, eos)
        assert got["score"][rows].tolist() == [float(c[0]) for c in kept], b
        assert got["parent"][rows].tolist() == [b * K + c[1] for c in kept] and got["token"][rows].tolist() == [c[2] for c in kept]
        assert got["finished"][rows].tolist() == [int(c[3]) for c in kept]
        done = all(c[3] for c in kept) or i + 1 >= Lmax
        assert int(got["done"][b]) == int(done) and int(got["step"][b]) == (i if done else i + 1)
        for q, c in enumerate(kept):
            src, row = b * K + c[1], b * K + q
            was_fin = bool(before["finished"][src])
            assert got["tokens"][row, :i].tolist() == before["tokens"][src, :i].tolist() and int(got["tokens"][row, i]) == c[2]
            assert got["slots"][row, :i].tolist() == before["slots"][src, :i].tolist()
            if not done:
                assert int(got["slots"][row, i]) == int(before["slots"][src, i])
            hl = int(before["hlen"][src]) + (0 if was_fin or c[2] == eos else 1)
            assert int(got["hlen"][row]) == hl
            if not done:
                assert int(got["slots"][row, i + 1]) == (i + 1) * R + row and int(got["klen"][row]) == i + 2
            else:
                assert int(got["klen"][row]) == i + 1 and got["slots"][row, i + 1:].tolist() == before["slots"][row, i + 1:].tolist()
                assert int(got["slots"][row, i]) == i * R + row                          # the slot a frozen row keeps appending to is its own
                assert int(got["nbest_len"][b, q]) == hl and float(got["nbest_score"][b, q]) == float(c[0])
                assert got["nbest_tokens"][b, q, :hl].tolist() == got["tokens"][row, :hl].tolist() and bool((got["nbest_tokens"][b, q, hl:] == -7).all())
            want_x = (E[c[2]].double() * math.sqrt(D) + pe[i if done else i + 1].double()).float()
            assert torch.equal(got["x"][row], want_x)
        if not done:
            assert bool((got["nbest_len"][b] == -7).all()) and bool((got["nbest_score"][b] == 7.0).all())
    assert got["parent"][0:2].tolist() == [0, 0] and got["token"][0:2].tolist() == [2, 7] and got["parent"][2].item() == 1        # the planted ties
    assert got["done"].tolist() == [0, 1, 1, 1] and int(got["n_done"]) == 3 and int(got["all_done"]) == 0
    # a second step: utterance 0 runs on while the others stay as they are; their n-best buffers are not written again
    S2 = {k: v.clone() for k, v in got.items()}
    S2["nbest_tokens"][1:], S2["nbest_len"][1:], S2["nbest_score"][1:] = -9, -9, 9.0
    S2["max_len"][0] = 4
    got2 = run_prune(cfm, S2, idx, logp, E, pe, eos, V)
    assert bool((got2["nbest_len"][1:] == -9).all()) and bool((got2["nbest_score"][1:] == 9.0).all()) and bool((got2["nbest_tokens"][1:] == -9).all())
    assert got2["done"].tolist() == [1, 1, 1, 1] and int(got2["n_done"]) == 4 and int(got2["all_done"]) == 1
    assert got2["parent"][K:].tolist() == list(range(K, R)) and int(got2["nbest_len"][0, 0]) == int(got2["hlen"][0])


# ------------------------------------------------------------------------------------------------------------------------------- the search
_decoders = {}


def _decoder(case):
    if case[0] not in _decoders:
        _decoders[case[0]] = SR.decoder_for(case).to(DEV)
    return _decoders[case[0]]


def _search(case, **kw):
    import decoder
    name, B, K, T, V, D, max_len, seed, sharpen, eos_bias, modes = case
    _, memory, lens = SR.inputs(case)
    bs = decoder.AttentionBeamSearch(_decoder(case), beam=K, max_len=max_len, **kw)
    return bs, bs.search(memory.to(DEV), lens, return_device=True)


def _compare(case, mode, got):
    """The protocol of test_rnnt_beam_gpu.py.  Returns the number of clear utterances."""
    res = SR.reference(case)
    ds, gate = SR.deltas(mode, case)
    n_clear = 0
    assert len(got) == len(res)
    for b, (g, r, d) in enumerate(zip(got, res, ds)):
        ref = r["nbest"]
        assert len({tuple(t) for t, _ in g}) == len(g) or not all(f for _, _, f in ref), (case[0], b, "a string twice")
        assert len(g) == len(ref), (case[0], b, len(g), len(ref))
        errs = [abs(x[1] - y[1]) for x, y in zip(sorted(g, key=lambda x: -x[1]), ref)]
        is_clear = SR.clear(r, d)
        print("  %s %s utt %d: %s, %d entries, max score error %.2e (delta %.2e, per-position gate %.2e)" % (case[0], mode, b, "clear" if is_clear else "unclear", len(g), max(errs), d, gate))
        assert max(errs) <= d, (case[0], mode, b, max(errs), d)
        if is_clear:
            n_clear += 1
            assert [tuple(t) for t, _ in g] == [s for s, _, _ in ref], (case[0], b, g, ref)
            assert [s for _, s in g] == sorted((s for _, s in g), reverse=True)
    return n_clear


SEARCH = [(c, m) for c in SR.GPU_CASES for m in SR.MODES]                              # every case in every mode


@pytest.mark.parametrize("case,mode", SEARCH, ids=["%s-%s" % (c[0], m) for c, m in SEARCH])
def test_search_matches_the_float64_search(cfm, precision, case, mode):
    import decoder
    precision(mode)
    name, B, K, T, V, D, max_len, seed, sharpen, eos_bias, modes = case
    bs, (got, (tokens, nlen, score)) = _search(case)
    n_clear = _compare(case, mode, got)
    for b in range(B):                                                                  # unused entries: length 0, score -inf
        assert torch.all(nlen[b, len(got[b]):] == 0) and torch.all(score[b, len(got[b]):] == float("-inf"))
    claimed = mode in case[10]
    print("attention search %s %s: clear %d of %d%s, steps %d, replays %d" % (name, mode, n_clear, B, "" if claimed else " (clear share not claimed for this mode)", bs.steps, bs.replays))
    if claimed:                                                                         # where the float64 search alone is clear (asserted on the CPU)
        assert 2 * n_clear >= B
    if B >= 3:
        assert got[-1] == [([], 0.0)]                                                   # the utterance without frames
    # cache against no cache, on the device, for EVERY finished string the search returned, clear utterance or not: the rescorer's left score
    # (whole prefixes, no cache; the eos term included, as in a finished hypothesis's score) within (length + 1) x the per-position gate
    _, memory, lens = SR.inputs(case)
    left = decoder.AttentionRescorer(_decoder(case), first_pass_weight=0.0).scores(memory.to(DEV), torch.tensor(lens), tokens, nlen, score)[1].cpu()
    gate = SR.deltas(mode, case)[1]
    finished, nl, sc = bs._S["finished"].cpu().view(B, K), nlen.cpu(), score.cpu()
    checked = worst = 0
    for b in range(B):
        for n in range(K):
            if lens[b] == 0 or not bool(finished[b, n]) or float(sc[b, n]) == float("-inf"):
                continue
            err, d = abs(float(left[b, n]) - float(sc[b, n])), (int(nl[b, n]) + 1) * gate
            assert err <= d, (name, mode, b, n, float(left[b, n]), float(sc[b, n]), d)
            checked, worst = checked + 1, max(worst, err / d)
    print("  cache against no cache: %d finished hypotheses rescored, worst error / delta %.2e" % (checked, worst))
    assert checked > 0 or not bool(finished[[b for b in range(B) if lens[b] > 0]].any())


def test_graph_reuse_and_weight_updates(cfm, precision):
    import decoder
    precision("fp32")
    case = SR.GPU_CASES[1]                                                              # B = 3, beam 4
    name, B, K, T, V, D, max_len, seed, sharpen, eos_bias, modes = case
    bs, (got, _) = _search(case)
    _, (eager, _) = _search(case, use_graph=False, steps_per_replay=3)
    assert got == eager and bs._graph is not None
    # other inputs, lengths and batch size on the same object: no state is stale
    rs = np.random.RandomState(5)
    mem2 = torch.from_numpy(rs.standard_normal((5, 9, D)).astype(np.float32)).to(DEV)
    lens2 = [9, 0, 4, 7, 1]
    fresh = lambda d: decoder.AttentionBeamSearch(d, beam=K)
    again = bs.search(mem2, lens2)
    assert again == fresh(_decoder(case)).search(mem2, lens2) and again[1] == [([], 0.0)]
    _, memory, lens = SR.inputs(case)
    assert bs.search(memory.to(DEV), lens) == got
    # an in-place weight change: the result changes and is the float64 search's for the new weights
    dec2 = copy.deepcopy(SR.decoder_for(case)).to(DEV)
    bs2 = fresh(dec2)
    assert bs2.search(memory.to(DEV), lens) == got
    with torch.no_grad():
        dec2.output_layer.bias.add_(torch.linspace(-8.0, 8.0, V, device=DEV))
        dec2.decoders[0].src_attn.linear_k.weight.mul_(1.5)
    after = bs2.search(memory.to(DEV), lens)
    assert after != got and after == fresh(dec2).search(memory.to(DEV), lens)
    P = {k: v.cpu() for k, v in dec2.state_dict().items()}
    gate = 4.0 * SR.yardstick("fp32", case)
    for b in range(B):
        r = SR.search64(P, memory[b].double(), lens[b], K, SR.H, V - 1, V - 1, max_len)
        d = (max(len(t) for t, _, _ in r["nbest"]) + 1) * gate
        assert max(abs(x[1] - y[1]) for x, y in zip(sorted(after[b], key=lambda x: -x[1]), r["nbest"])) <= d
        if SR.clear(r, d):
            assert [tuple(t) for t, _ in after[b]] == [s for s, _, _ in r["nbest"]]


def test_recognizer_attention(cfm, precision):
    import decoder
    import synth
    import transducer
    from conftest import load_golden
    from test_edit_distance_gpu import offline_recognizer
    precision("fp32")
    _, meta = load_golden("offline_asr")
    plain, (enc, pr, jn) = offline_recognizer(meta)
    V, D = meta["head"]["V"], meta["cfg"]["encoder_dim"]
    torch.manual_seed(78)
    att = decoder.BiTransformerDecoder(V, D, 4, 2 * D, 2, 1, 0.0, 0.0, 0.0, 0.0).eval().to(DEV)
    with torch.no_grad():
        att.left_decoder.output_layer.weight.mul_(12.0)
        att.left_decoder.output_layer.bias[V - 1] += 2.0
    rec = transducer.OfflineRecognizer(enc, pr, jn, blank=meta["blank"], n_steps=meta["n_steps"], attention=att, first_pass_weight=0.3, reverse_weight=0.3)
    lens = torch.tensor(meta["lens"] + [0], dtype=torch.int32, device=DEV)
    x = torch.from_numpy(synth.fbank(meta["xseed"], len(meta["lens"]), max(meta["lens"])))
    x = torch.cat([x, x[:1]], 0).to(DEV)
    got = rec.recognize_attention(x, lens, beam=4)
    with torch.no_grad():
        y, out_lens = enc.forward_utterances(x, lens)
    bs = decoder.AttentionBeamSearch(att, beam=4)
    want, triple = bs.search(y, out_lens, return_device=True)
    assert got == want and got[-1] == [([], 0.0)] and all(1 <= len(n) <= 4 for n in got)
    rescored = rec.recognize_attention(x, lens, beam=4, rescore=True)
    assert rescored == rec.rescorer.rescore(y, out_lens, triple)
    for a, b in zip(rescored, got):
        assert sorted(tuple(t) for t, _ in a) == sorted(tuple(t) for t, _ in b)
    with pytest.raises(RuntimeError, match="without an attention decoder"):
        plain.recognize_attention(x, lens)
    left_only = transducer.OfflineRecognizer(enc, pr, jn, blank=meta["blank"], n_steps=meta["n_steps"], attention=att.left_decoder)
    with pytest.raises(ValueError, match="reverse_weight"):
        left_only.recognize_attention(x, lens, rescore=True)
