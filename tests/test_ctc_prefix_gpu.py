"""GPU: joint CTC/attention decoding -- the three kernels of csrc/ctc_prefix.hip through the C entry (operands between guard bands, outputs
NaN-prefilled: tests/extent.py), then decoder.JointBeamSearch and transducer.OfflineRecognizer.recognize_joint against the float64 joint search of
tests/ctc_prefix_ref.py, which has no cache and no incremental state.

Tolerances.  cfm_ctc_logprob_t: 4 x the worst error of float32 torch.log_softmax on the same logits.  cfm_ctc_prefix_score / _advance:
|value - ref| <= g (1 + |ref|), ref in float64 on the same f32 x and state, g = 4 x the worst such ratio of the SAME formulas (ctc_prefix_ref's
functions) run in float32 on the CPU over this file's own cases, printed.  Search: the protocol of test_attention_search_gpu.py with the
per-position gate 4 x [(1 - lam) x the attention yardstick + lam x the CTC-prefix yardstick] (ctc_prefix_ref.deltas).  The protocol's
score bound for unclear utterances is a property of the cases; tests/test_ctc_prefix_cpu.py checks it for them with the search emulated in float32.

Row counts.  A row belongs to an utterance (R = B * K), so R in {1, 5, 33} is exact where K = 1; with K > 1 the cases take B in {1, 5} (up to 80
rows: more than one workgroup of the advance kernel, many of the score kernel)."""
import ctypes

import numpy as np
import pytest
import torch

import ctc_prefix_ref as CP
from extent import Guards

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
NEG = float("-inf")
BLANK = 0


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


def ragged(B, T, seed):
    """Lengths that include T, 0 and 1 where B allows."""
    rs = np.random.RandomState(seed)
    lens = rs.randint(1, T + 1, B)
    lens[0] = T
    if B >= 3:
        lens[1], lens[2] = 0, 1
    if B >= 5:
        lens[3] = max(T - 1, 1)
    return [int(v) for v in lens]


# ------------------------------------------------------------------------------------------------------------------------ cfm_ctc_logprob_t
LOGPROB_CASES = [(B, T, V) for B in (1, 3) for T in (1, 2, 63, 65, 257) for V in (17, 5002)]


@pytest.mark.parametrize("B,T,V", LOGPROB_CASES, ids=lambda v: str(v))
def test_logprob_t_against_float64(cfm, B, T, V):
    g = torch.Generator().manual_seed(B * 1000 + T * 10 + V)
    Vp, Tp = (V + 3) // 4 * 4, (T + 3) // 4 * 4
    logits = torch.randn(B * T, V, generator=g) * 4.0
    lens = ragged(B, T, T + V)
    ref = torch.log_softmax(logits.double(), -1).view(B, T, V)
    f32 = torch.log_softmax(logits, -1).view(B, T, V)
    valid = torch.arange(T).view(1, T) < torch.tensor(lens).view(B, 1)                          # [B, T]
    worst32 = float((f32.double() - ref)[valid].abs().max())
    tol = 4.0 * worst32
    G = Guards()
    lg = G.inp(logits, ld=Vp, name="logits")                                                    # the pad columns V..Vp hold NaN
    ln = G.inp(torch.tensor(lens, dtype=torch.int32), name="lens")
    x = G.out((B, V, Tp), torch.float32, name="x")
    rc = cfm.lib().cfm_ctc_logprob_t(cfm.ptr(lg), Vp, B, T, V, cfm.ptr(ln), cfm.ptr(x), cfm.stream())
    assert rc == 0, cfm.lib().cfm_last_error()
    torch.cuda.synchronize()
    G.check()
    got = x.cpu()
    live = torch.zeros(B, Tp, dtype=torch.bool)
    live[:, :T] = valid
    err = (got[:, :, :T].transpose(1, 2).double() - ref).abs()[valid]
    print("logprob_t B=%d T=%d V=%d: max |err| %.3e, float32 torch %.3e, tolerance %.3e" % (B, T, V, float(err.max()), worst32, tol))
    assert bool((err <= tol).all())
    assert not torch.isnan(got.transpose(1, 2)[live]).any()                                     # every owned element written
    assert bool(torch.isnan(got.transpose(1, 2)[~live]).all())                                  # t >= lens[b] and the padding: not touched, as the header says


def test_logprob_t_limits(cfm):
    lens = torch.ones(1, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="2048"):
        cfm.ctc_logprob_t(torch.zeros(1, 2049, 20, device=DEV), 17, lens)
    with pytest.raises(ValueError, match="rounded up"):
        cfm.ctc_logprob_t(torch.zeros(1, 5, 20, device=DEV), 17, lens, out=torch.zeros(1, 17, 5, device=DEV))
    assert cfm.ctc_logprob_t(torch.zeros(1, 5, 20, device=DEV), 17, lens).shape == (1, 17, 8)


# ------------------------------------------------------------------------------------------------- cfm_ctc_prefix_score / cfm_ctc_prefix_advance
# B, K, P, T, V: every R = B * K in {1, 5, 33} at K = 1; P in {1, 4, 16} with K in {1, P / 2, P}; every T; both V
STEP_CASES = [(1, 1, 1, 1, 17), (5, 1, 1, 2, 17), (33, 1, 4, 63, 17), (5, 2, 4, 64, 17), (5, 4, 4, 65, 17), (1, 1, 16, 257, 17), (5, 8, 16, 63, 17), (5, 16, 16, 65, 17),
              (33, 1, 16, 257, 17), (1, 2, 4, 257, 5002), (5, 8, 16, 64, 5002), (5, 1, 4, 2, 5002), (5, 16, 16, 1, 5002), (3, 4, 4, 257, 17)]
LAM = (0.3, 1.0)


def step_case(B, K, P, T, V, seed=0):
    """x, the rows' states (built by running the float64 specification, then rounded to f32: the reference reads the same f32 values), the search
    state and P candidates per row."""
    rs = np.random.RandomState(B * 7919 + K * 131 + P * 17 + T + V + seed)
    R, Tp, eos = B * K, (T + 3) // 4 * 4, V - 1
    lens = ragged(B, T, T + P)
    logits = (rs.standard_normal((B, T, V)) * 3.0).astype(np.float32)
    logits[:, :, BLANK] += 2.0
    x32 = CP.log_softmax(logits.astype(np.float64)).astype(np.float32)                          # [B, T, V]
    xt = torch.full((B, V, Tp), float("nan"))
    for b in range(B):
        xt[b, :, :lens[b]] = torch.from_numpy(x32[b, :lens[b]].T.copy())                        # frames at t >= lens[b] hold NaN: nothing reads them
    x64 = x32.astype(np.float64)
    done = [int(B >= 2 and b == B - 1) for b in range(B)]                                       # the last utterance is done already
    step = [int(rs.randint(0, 4)) for _ in range(B)]
    state = torch.full((2, R, Tp, 2), float("nan"))
    psi = torch.zeros(R)
    token, hlen, finished, rows = [], [], [], []
    for r in range(R):
        b = r // K
        n = lens[b]
        L = [0, 1, 2, 3, 2][r % 5]                                                               # the empty prefix among them
        g = [int(v) for v in rs.randint(1, V - 1, L)]
        if L >= 2 and r % 3 == 0:
            g[-1] = g[-2]                                                                        # a repeated last token
        st = CP.state_of(x64[b, :n], g, BLANK)
        st = CP.State(st.gn.astype(np.float32).astype(np.float64), st.gb.astype(np.float32).astype(np.float64), float(np.float32(st.psi)), g)
        if r % 11 == 7:
            st.psi = NEG                                                                         # a row whose psi is -inf
        state[step[b] & 1, r, :n, 0], state[step[b] & 1, r, :n, 1] = torch.from_numpy(st.gn).float(), torch.from_numpy(st.gb).float()
        psi[r] = st.psi
        token.append(g[-1] if g else eos)                                                        # sos = eos starts the empty prefix
        hlen.append(L)
        finished.append(int(r % 7 == 5))
        rows.append(st)
    # candidates: distinct classes per row -- the last token, blank and eos among them where P allows
    idx = np.zeros((R, P), dtype=np.int64)
    for r in range(R):
        must = list(dict.fromkeys(([token[r]] if hlen[r] else []) + [eos, BLANK]))[:P] if r % 2 == 0 else []
        cls = (must + [k for k in rs.permutation(V).tolist() if k not in must])[:P]
        idx[r] = rs.permutation(cls)
    logp = -np.sort(rs.rand(R, P).astype(np.float32) * 6.0, 1)
    S = dict(token=torch.tensor(token, dtype=torch.int32), hlen=torch.tensor(hlen, dtype=torch.int32), finished=torch.tensor(finished, dtype=torch.uint8),
             step=torch.tensor(step, dtype=torch.int32), done=torch.tensor(done, dtype=torch.uint8), lens=torch.tensor(lens, dtype=torch.int32))
    return dict(B=B, K=K, P=P, T=T, V=V, R=R, Tp=Tp, eos=eos, lens=lens, x=xt, x64=x64, state=state, psi=psi, S=S, rows=rows, idx=torch.from_numpy(idx).int(),
                logp=torch.from_numpy(logp), done=done, finished=finished, step=step)


def score_reference(c, lam, dtype=np.float64):
    """Per live row the P offers and psi(g.c) by ctc_prefix_ref in `dtype`, ranked: [(offer, class, psi_c)] best first; None for a row the kernel
    writes as (eos, -inf, -inf)."""
    lam, att_w = float(np.float32(lam)), float(np.float32(1.0) - np.float32(lam))       # the weights as the kernel holds them: f32
    out = []
    for r, st in enumerate(c["rows"]):
        b = r // c["K"]
        n = c["lens"][b]
        if c["done"][b] or c["finished"][r] or n == 0:
            out.append(None)
            continue
        x = c["x64"][b, :n].astype(dtype)
        s = CP.State(st.gn.astype(dtype), st.gb.astype(dtype), dtype(st.psi), st.tokens)
        offers = []
        for j in range(c["P"]):
            k = int(c["idx"][r, j])
            p = CP.psi_ext(x, s, k, BLANK, c["eos"])
            d = CP.delta(p, s.psi)
            o = NEG if d == NEG else ((dtype(att_w) * dtype(c["logp"][r, j]) if lam < 1.0 else dtype(0.0)) + dtype(lam) * d)
            offers.append((float(o), k, float(p)))
        offers.sort(key=lambda o: (-o[0], o[1]))
        out.append(offers)
    return out


def advance_inputs(c, seed):
    """What the prune would leave: per row a parent within its utterance (shared and permuted), a token (the parent's last one and the blank among
    them), the strings table and the new lengths; step counts the steps taken."""
    rs = np.random.RandomState(seed)
    R, K, V, Lmax = c["R"], c["K"], c["V"], 6
    parent, token, hlen = [], [], []
    tokens = torch.zeros(R, Lmax, dtype=torch.int32)
    for r in range(R):
        b = r // K
        live = [q for q in range(b * K, b * K + K) if not c["finished"][q]] or [r]            # a kept unfinished row never has a finished parent
        p = live[int(rs.randint(0, len(live)))] if r % 2 else live[(K - 1 - r % K) % len(live)]
        g = list(c["rows"][p].tokens)
        k = int(rs.randint(1, V - 1))
        if g and r % 3 == 1:
            k = g[-1]
        if r % 13 == 6:
            k = BLANK
        parent.append(p), token.append(k), hlen.append(len(g) + 1)
        tokens[r, :len(g) + 1] = torch.tensor(g + [k], dtype=torch.int32)
    return torch.tensor(parent, dtype=torch.int32), torch.tensor(token, dtype=torch.int32), torch.tensor(hlen, dtype=torch.int32), tokens


def advance_reference(c, parent, token, dtype=np.float64):
    out = []
    for r in range(c["R"]):
        b = r // c["K"]
        n = c["lens"][b]
        if c["done"][b] or c["finished"][r] or n == 0:
            out.append(None)
            continue
        st = c["rows"][int(parent[r])]
        s = CP.State(st.gn.astype(dtype), st.gb.astype(dtype), dtype(st.psi), st.tokens)
        out.append(CP.extend(c["x64"][b, :n].astype(dtype), s, int(token[r]), BLANK))
    return out


def _ratio(a, b):
    """max |a - b| / (1 + |b|) over the finite entries of b; entries that are -inf in b must be -inf in a."""
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    inf = b == NEG
    assert bool((a[inf] == NEG).all())
    return float((np.abs(a[~inf] - b[~inf]) / (1.0 + np.abs(b[~inf]))).max()) if (~inf).any() else 0.0


@pytest.fixture(scope="module")
def g_prefix():
    """4 x the worst |float32 - float64| / (1 + |float64|) of ctc_prefix_ref's own formulas over this file's cases: psi(g.c), the offers, the advanced
    state and its psi."""
    worst = 0.0
    for case in STEP_CASES:
        c = step_case(*case)
        for lam in LAM:
            for r64, r32 in zip(score_reference(c, lam), score_reference(c, lam, np.float32)):
                if r64 is not None:
                    by = {k: (o, p) for o, k, p in r32}
                    worst = max(worst, _ratio([by[k][0] for _, k, _ in r64], [o for o, _, _ in r64]), _ratio([by[k][1] for _, k, _ in r64], [p for _, _, p in r64]))
        parent, token, _, _ = advance_inputs(c, 1)
        for s64, s32 in zip(advance_reference(c, parent, token), advance_reference(c, parent, token, np.float32)):
            if s64 is not None:
                worst = max(worst, _ratio(s32.gn, s64.gn), _ratio(s32.gb, s64.gb), _ratio([s32.psi], [s64.psi]))
    print("ctc prefix: float32's largest |error| / (1 + |value|) = %.3e, g = %.3e" % (worst, 4 * worst))
    return 4 * worst


def _desc(cfm, c, G, lam):
    d = cfm.CtcPrefixDesc()
    x, state, psi = G.inp(c["x"], name="x"), G.io(c["state"], name="state"), G.io(c["psi"], name="psi")
    S = {k: G.inp(v, name=k) for k, v in c["S"].items()}
    d.x, d.state, d.psi = cfm.ptr(x), cfm.ptr(state), cfm.ptr(psi)
    for k, v in S.items():
        setattr(d, k, cfm.ptr(v))
    d.B, d.K, d.P, d.T, d.V, d.Lmax, d.blank, d.eos, d.ctc_weight = c["B"], c["K"], c["P"], c["T"], c["V"], 6, BLANK, c["eos"], lam
    return d, state, psi


@pytest.mark.parametrize("lam", LAM)
@pytest.mark.parametrize("case", STEP_CASES, ids=lambda v: "-".join(str(s) for s in v))
def test_prefix_score_against_float64(cfm, g_prefix, case, lam):
    c = step_case(*case)
    R, K, P = c["R"], c["K"], c["P"]
    G = Guards()
    d, state, psi = _desc(cfm, c, G, lam)
    idx, logp = G.inp(c["idx"], name="topk_idx"), G.inp(c["logp"], name="topk_logp")
    out_idx, out_logp, cand_psi = G.out((R, K), torch.int32, name="out_idx"), G.out((R, K), name="out_logp"), G.out((R, K), name="cand_psi")
    d.topk_idx, d.topk_logp, d.out_idx, d.out_logp, d.cand_psi = (cfm.ptr(t) for t in (idx, logp, out_idx, out_logp, cand_psi))
    rc = cfm.lib().cfm_ctc_prefix_score(ctypes.byref(d), cfm.stream())
    assert rc == 0, cfm.lib().cfm_last_error()
    torch.cuda.synchronize()
    G.check()
    assert torch.equal(state.cpu().view(torch.int32), c["state"].view(torch.int32)) and torch.equal(psi.cpu().view(torch.int32), c["psi"].view(torch.int32))     # read only
    gi, gl, gp = out_idx.cpu().numpy(), out_logp.cpu().numpy().astype(np.float64), cand_psi.cpu().numpy().astype(np.float64)
    assert not np.isnan(gl).any() and not np.isnan(gp).any() and bool((gi >= 0).all())                  # written everywhere, no NaN
    worst = 0.0
    for r, ref in enumerate(score_reference(c, lam)):
        if ref is None:                                                                                  # finished, done or without frames: (eos, -inf, -inf)
            assert bool((gi[r] == c["eos"]).all()) and bool((gl[r] == NEG).all()) and bool((gp[r] == NEG).all()), r
            continue
        by = {k: (o, p) for o, k, p in ref}
        assert len(set(gi[r].tolist())) == K and all(int(k) in by for k in gi[r])
        bound = lambda v: g_prefix * (1.0 + abs(v))
        for q in range(K):
            o, k, p = ref[q]
            if o == NEG:                                                                                 # -inf is decided exactly: the lower class first
                assert gl[r, q] == NEG and int(gi[r, q]) == k, (r, q)
            else:
                assert abs(gl[r, q] - o) <= bound(o), (r, q, gl[r, q], o)                                # the q-th best offer, whoever holds it
                worst = max(worst, abs(gl[r, q] - o) / (1.0 + abs(o)))
                lo = ref[q - 1][0] - o if q > 0 else float("inf")
                hi = o - ref[q + 1][0] if q + 1 < P else float("inf")
                if min(lo, hi) > 2 * bound(o):                                                           # told apart from both neighbours: the same class
                    assert int(gi[r, q]) == k, (r, q, gi[r].tolist(), ref)
            pk = by[int(gi[r, q])][1]                                                                    # psi of the class the device put here
            if pk == NEG:
                assert gp[r, q] == NEG
            else:
                assert abs(gp[r, q] - pk) <= bound(pk), (r, q, gp[r, q], pk)
                worst = max(worst, abs(gp[r, q] - pk) / (1.0 + abs(pk)))
    print("prefix score %s lam=%.1f: worst |err| / (1 + |value|) = %.3e (g = %.3e)" % (case, lam, worst, g_prefix))


@pytest.mark.parametrize("case", STEP_CASES, ids=lambda v: "-".join(str(s) for s in v))
def test_prefix_advance_against_float64(cfm, g_prefix, case):
    c = step_case(*case)
    R, K = c["R"], c["K"]
    worst = 0.0
    for it in range(2):                                                                                  # two consecutive steps: both parities
        parent, token, hlen, tokens = advance_inputs(c, 1 + it)
        c["S"].update(parent=parent, token=token, hlen=hlen, tokens=tokens, step=torch.tensor([s + 1 for s in c["step"]], dtype=torch.int32))
        c["step"] = [s + 1 for s in c["step"]]
        before = c["state"].clone()
        G = Guards()
        d, state, psi = _desc(cfm, c, G, 1.0)
        d.P = K
        rc = cfm.lib().cfm_ctc_prefix_advance(ctypes.byref(d), cfm.stream())
        assert rc == 0, cfm.lib().cfm_last_error()
        torch.cuda.synchronize()
        G.check()
        got, got_psi = state.cpu(), psi.cpu()
        new_rows = []
        for r, ref in enumerate(advance_reference(c, parent, token)):
            b = r // K
            n, new, old = c["lens"][b], c["step"][b] & 1, (c["step"][b] + 1) & 1
            same = lambda a, bb: torch.equal(a.contiguous().view(torch.int32), bb.contiguous().view(torch.int32))
            assert same(got[old, r], before[old, r]), (r, "the half that was read")
            if ref is None:                                                                              # finished or done: bit-unchanged
                assert same(got[new, r], before[new, r]) and same(got_psi[r:r + 1], c["psi"][r:r + 1]), r
                new_rows.append(c["rows"][r])
                continue
            assert same(got[new, r, n:], before[new, r, n:]), (r, "frames beyond the length")
            gn, gb = got[new, r, :n, 0].numpy().astype(np.float64), got[new, r, :n, 1].numpy().astype(np.float64)
            assert not np.isnan(gn).any() and not np.isnan(gb).any() and not np.isnan(float(got_psi[r]))
            ratios = (_ratio(gn, ref.gn), _ratio(gb, ref.gb), _ratio([float(got_psi[r])], [float(ref.psi)]))
            assert max(ratios) <= g_prefix, (r, ratios, g_prefix)
            worst = max(worst, *ratios)
            new_rows.append(CP.State(gn, gb, float(got_psi[r]), ref.tokens))                             # the next step reads what the device wrote
        c["rows"], c["state"], c["psi"] = new_rows, got.clone(), got_psi.clone()
    print("prefix advance %s: worst |err| / (1 + |value|) = %.3e (g = %.3e)" % (case, worst, g_prefix))


def test_prefix_limits(cfm):
    c = step_case(1, 2, 4, 5, 17)
    S = {k: v.to(DEV) for k, v in c["S"].items()}
    x, st, psi = torch.zeros(1, 17, 8, device=DEV), torch.zeros(2, 2, 8, 2, device=DEV), torch.zeros(2, device=DEV)
    idx, logp = c["idx"].to(DEV), c["logp"].to(DEV)
    assert cfm.ctc_prefix_score(x, 5, st, psi, idx, logp, S, 2, 0.3, 0, 16)[0].shape == (2, 2)
    for kw, what in ((dict(eos=0), "differ"), (dict(eos=17), "differ"), (dict(lam=0.0), "ctc_weight"), (dict(lam=1.5), "ctc_weight")):
        with pytest.raises(RuntimeError, match=what):
            cfm.ctc_prefix_score(x, 5, st, psi, idx, logp, S, 2, kw.get("lam", 0.3), 0, kw.get("eos", 16))
    with pytest.raises(RuntimeError, match="K=2 P=1"):
        cfm.ctc_prefix_score(x, 5, st, psi, idx[:, :1].contiguous(), logp[:, :1].contiguous(), S, 2, 0.3, 0, 16)
    wide = torch.zeros(2, 17, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="P=17"):
        cfm.ctc_prefix_score(x, 5, st, psi, wide, torch.zeros(2, 17, device=DEV), S, 2, 0.3, 0, 16)
    with pytest.raises(ValueError, match="rounded up"):
        cfm.ctc_prefix_score(x, 9, st, psi, idx, logp, S, 2, 0.3, 0, 16)


# ------------------------------------------------------------------------------------------------------------------------------- the search
_heads = {}


def _modules(case):
    if case[0] not in _heads:
        dec, ctc, _, _ = CP.inputs(case)
        _heads[case[0]] = (dec.to(DEV), ctc.to(DEV))
    return _heads[case[0]]


def _search(case, **kw):
    import decoder
    name, B, K, T, V, D, max_len, seed, sharpen, eos_bias, modes, lam, pre_beam, _, _ = case
    _, _, memory, lens = CP.inputs(case)
    dec, ctc = _modules(case)
    js = decoder.JointBeamSearch(dec, ctc, beam=K, ctc_weight=lam, pre_beam=pre_beam, blank=BLANK, max_len=max_len, **kw)
    return js, js.search(memory.to(DEV), lens, return_device=True)


def _compare(case, mode, got):
    """The protocol of test_attention_search_gpu.py.  Returns the number of clear utterances."""
    res = CP.reference(case)
    ds, gate, gate_att = CP.deltas(mode, case)
    n_clear = 0
    assert len(got) == len(res)
    for b, (g, r, (d, d_att)) in enumerate(zip(got, res, ds)):
        ref = r["nbest"]
        assert len({tuple(t) for t, _ in g}) == len(g) or not all(f for _, _, f in ref), (case[0], b, "a string twice")
        is_clear = CP.clear(r, d, d_att)
        assert len(g) == len(ref), (case[0], b, len(g), len(ref))
        errs = [abs(x[1] - y[1]) for x, y in zip(sorted(g, key=lambda x: -x[1]), ref)] or [0.0]
        print("  %s %s utt %d: %s, %d entries, max score error %.2e (delta %.2e, per-position gate %.2e)" % (case[0], mode, b, "clear" if is_clear else "unclear", len(g), max(errs), d, gate))
        assert max(errs) <= d, (case[0], mode, b, max(errs), d)
        if is_clear:
            n_clear += 1
            assert [tuple(t) for t, _ in g] == [s for s, _, _ in ref], (case[0], b, g, ref)
            assert [s for _, s in g] == sorted((s for _, s in g), reverse=True)
    return n_clear


SEARCH = [(c, m) for c in CP.GPU_CASES for m in CP.MODES]


@pytest.mark.parametrize("case,mode", SEARCH, ids=["%s-%s" % (c[0], m) for c, m in SEARCH])
def test_search_matches_the_float64_joint_search(cfm, precision, case, mode):
    import decoder
    precision(mode)
    name, B, K, T, V, D, max_len, seed, sharpen, eos_bias, modes, lam, pre_beam, _, _ = case
    js, (got, (tokens, nlen, score)) = _search(case)
    n_clear = _compare(case, mode, got)
    for b in range(B):                                                                  # unused entries: length 0, score -inf
        assert torch.all(nlen[b, len(got[b]):] == 0) and torch.all(score[b, len(got[b]):] == NEG)
    claimed = mode in case[10]
    print("joint search %s %s: clear %d of %d%s, steps %d, replays %d" % (name, mode, n_clear, B, "" if claimed else " (clear share not claimed for this mode)", js.steps, js.replays))
    if claimed:                                                                         # where the float64 search alone is clear (asserted on the CPU)
        assert 2 * n_clear >= B
    if B >= 3:
        assert got[-1] == [([], 0.0)]                                                   # the utterance without frames
    # against the kernels that already exist, for EVERY finished string the search returned, clear utterance or not: (1 - lam) x the rescorer's left
    # score (whole prefixes, no cache) + lam x (minus CTCDecoder.nll of the string: the CTC loss kernel), within the string's delta
    dec, ctc = _modules(case)
    _, _, memory, lens = CP.inputs(case)
    mem = memory.to(DEV)
    left = decoder.AttentionRescorer(dec, first_pass_weight=0.0).scores(mem, torch.tensor(lens), tokens, nlen, score)[1].cpu()
    Lmax = tokens.shape[2]
    nll = ctc.nll(mem.repeat_interleave(K, 0), torch.tensor(lens).repeat_interleave(K), tokens.view(B * K, Lmax), nlen.view(B * K).clamp(min=0)).cpu().view(B, K)
    gate = CP.deltas(mode, case)[1]
    finished, nl, sc = js._S["finished"].cpu().view(B, K), nlen.cpu(), score.cpu()
    checked = worst = 0
    for b in range(B):
        for n in range(K):
            if lens[b] == 0 or not bool(finished[b, n]) or float(sc[b, n]) == NEG:
                continue
            want = (1.0 - lam) * float(left[b, n]) - lam * float(nll[b, n])
            err, d = abs(want - float(sc[b, n])), (int(nl[b, n]) + 1) * gate
            assert err <= d, (name, mode, b, n, want, float(sc[b, n]), d)
            checked, worst = checked + 1, max(worst, err / d)
    print("  against AttentionRescorer and CTCDecoder.nll: %d finished hypotheses, worst error / delta %.2e" % (checked, worst))
    assert checked > 0 or not bool(finished[[b for b in range(B) if lens[b] > 0]].any())


def test_graph_against_eager_and_reuse(cfm, precision):
    import decoder
    precision("fp32")
    case = CP.GPU_CASES[1]                                                              # B = 3, beam 4
    name, B, K, T, V, D, max_len, seed, sharpen, eos_bias, modes, lam, pre_beam, _, _ = case
    js, (got, _) = _search(case)
    _, (eager, _) = _search(case, use_graph=False, steps_per_replay=3)
    assert got == eager and js._graph is not None                                       # identical tokens, bit-identical scores
    rs = np.random.RandomState(5)
    mem2 = torch.from_numpy(rs.standard_normal((5, 9, D)).astype(np.float32)).to(DEV)   # another batch on the same object: no state is stale
    lens2 = [9, 0, 4, 7, 1]
    dec, ctc = _modules(case)
    fresh = lambda: decoder.JointBeamSearch(dec, ctc, beam=K, ctc_weight=lam, blank=BLANK)
    again = js.search(mem2, lens2)
    assert again == fresh().search(mem2, lens2) and again[1] == [([], 0.0)]
    _, _, memory, lens = CP.inputs(case)
    assert js.search(memory.to(DEV), lens) == got
    # an in-place change of the CTC head's weights: the graph goes, the result changes and is a fresh search's
    graph = js._graph
    with torch.no_grad():
        ctc.ctc_lo.bias[1:V - 1].add_(torch.linspace(-6.0, 6.0, V - 2, device=DEV))
    try:
        after = js.search(memory.to(DEV), lens)
        assert js._graph is not graph and after != got and after == fresh().search(memory.to(DEV), lens)
    finally:
        _heads.pop(case[0])                                                             # the cached head was changed: later tests rebuild it


def test_recognizer_joint(cfm, precision):
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
    blank = meta["blank"]
    rec = transducer.OfflineRecognizer(enc, pr, jn, blank=blank, n_steps=meta["n_steps"], ctc=plain.ctc, attention=att, first_pass_weight=0.3, reverse_weight=0.3)
    lens = torch.tensor(meta["lens"] + [0], dtype=torch.int32, device=DEV)
    x = torch.from_numpy(synth.fbank(meta["xseed"], len(meta["lens"]), max(meta["lens"])))
    x = torch.cat([x, x[:1]], 0).to(DEV)
    got = rec.recognize_joint(x, lens, beam=4, ctc_weight=0.4)
    with torch.no_grad():
        y, out_lens = enc.forward_utterances(x, lens)
    js = decoder.JointBeamSearch(att, plain.ctc, beam=4, ctc_weight=0.4, blank=blank)
    want, triple = js.search(y, out_lens, return_device=True)
    assert got == want and got[-1] == [([], 0.0)] and all(len(n) <= 4 for n in got)
    rescored = rec.recognize_joint(x, lens, beam=4, ctc_weight=0.4, rescore=True)
    assert rescored == rec.rescorer.rescore(y, out_lens, triple)
    for a, b in zip(rescored, got):
        assert sorted(tuple(t) for t, _ in a) == sorted(tuple(t) for t, _ in b)
    with pytest.raises(RuntimeError, match="without an attention decoder"):
        plain.recognize_joint(x, lens, beam=4)
    no_ctc = transducer.OfflineRecognizer(enc, pr, jn, blank=blank, n_steps=meta["n_steps"], attention=att)
    with pytest.raises(RuntimeError, match="without a CTC head"):
        no_ctc.recognize_joint(x, lens, beam=4)
