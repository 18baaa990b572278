"""GPU: the fused greedy-search step (csrc/greedy.hip, cfm_greedy_step) and the search around it (greedy.BatchedGreedySearch) against float64.

  * one call of cfm_greedy_step on a random, undoctored state -- tokens, LSTM state, frame index (beyond T' too), per-frame and total counts,
    lengths (0 and beyond T'), finished streams carrying a state -- built the way `search` builds it (`_state`, `_fused_weights`,
    `_fused_desc`), against tests/greedy_ref.py: the LSTM candidates, the projection, the joint's activations and the per-16-class-tile
    (max, index) pairs within a tolerance, the argmax by the margin rule, the control state after the step exactly;
  * exact ties at and across 16-class tile boundaries: the lowest index wins (torch.argmax), padding classes never;
  * whole searches at up to 64 streams (the fused step) and 65 (the torch-operation form) against the float64 loop: tokens equal up to the
    first decision whose two best float64 logits are within DELTA_SEARCH, the final (token, h, c) where no decision was that close;
  * a search object reused across weight updates (in place, `p.data = ...`, load_state_dict, a DataParallelTrainer step whose Adam kernel
    writes through raw pointers) decodes what a fresh one decodes.

Gates are about twice what the MI355X measured (measured value in the comment)."""
import numpy as np
import pytest
import torch

import greedy_ref as R
import synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")

# max|d| / max|ref| per tensor, one step on f32 MFMA products (exact f32 multiplies, K <= 768) against float64
GATE_STEP = 2e-6                 # measured 9.3e-7 (pmax, b64_cfg4_v5002)
# LSTM weights and biases x 100 (gate pre-activations up to ~190): a layer's f32 rounding error reaches the next one amplified by the
# weights, so the error is the problem's conditioning -- f32 accumulation in the kernel's k order restated on the host gives 8e-6 (4-product
# sums exact) to 5e-5 (each product rounded)
GATE_STEP_SATURATED = 6e-5       # measured 2.6e-5 (h_new)
DELTA_STEP = 1e-5                # tile / global argmax: classes within DELTA_STEP * max|logit| of the best are all correct answers
DELTA_SEARCH = 1e-4              # search: decisions whose two best float64 logits are closer than this (absolute) may go either way
GATE_SEARCH_STATE = 7e-7         # final h / c of a search that had no such decision, max|d| / max|ref|; measured 3.4e-7

# name, B, L, (E, H, P, J), V, blank, n_steps, (scale of the LSTM weights, of its biases): pre-activations beyond |x| = 30 saturate
# sigmoid / tanh, beyond 88.7 expf(-x) overflows to inf
STEP_CASES = [
    ("b1_min", 1, 1, (16, 16, 16, 16), 16, 0, 1, (1, 1)),
    ("b15_l2_v17", 15, 2, (32, 48, 16, 32), 17, 16, 3, (1, 1)),
    ("b16_l3_v31", 16, 3, (48, 16, 32, 64), 31, 0, 2, (1, 1)),
    ("b17_l4_v73", 17, 4, (16, 32, 48, 16), 73, 72, 64, (1, 1)),
    ("b33_l1_v5008", 33, 1, (64, 96, 80, 48), 5008, 0, 4, (1, 1)),
    ("b48_cfg4_v5002", 48, 2, (256, 256, 512, 512), 5002, 5001, 4, (1, 1)),
    ("b63_l3_v5002", 63, 3, (32, 64, 16, 48), 5002, 0, 3, (1, 1)),
    ("b64_l4_k768_v5008", 64, 4, (512, 256, 512, 512), 5008, 5007, 2, (1, 1)),
    ("b64_cfg4_v5002", 64, 2, (256, 256, 512, 512), 5002, 0, 64, (1, 1)),
    ("b40_saturated_bias", 40, 2, (64, 64, 32, 32), 73, 0, 3, (1, 1000)),
    ("b40_saturated", 40, 2, (64, 64, 32, 32), 73, 0, 3, (100, 100)),
]


def _np(x):
    return x.detach().cpu().numpy().copy()


def _rel(got, ref):
    ref = ref.double()
    return float((got.double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def _fused_setup(pr, jn, blank, n_steps, B, T):
    """The state, packs and descriptor exactly as BatchedGreedySearch.search builds them."""
    import greedy
    gs = greedy.BatchedGreedySearch(pr, jn, blank=blank, n_steps=n_steps, fused=True)
    S = gs._state(B, T, DEV)
    W = gs._fused_weights(DEV)
    return gs, S, W, gs._fused_desc(S, W, B, T)


def _run_step(desc):
    import ctypes
    import cfm
    cfm.check(cfm.lib().cfm_greedy_step(ctypes.byref(desc), cfm.stream()), "cfm_greedy_step")
    torch.cuda.synchronize()


def _check_step(name, S, host, P64, V, blank, n_steps, gate):
    """Everything one step wrote against the float64 restatement; returns the measured errors."""
    B = S["enc_proj"].shape[0]
    ref = R.step64(P64, host["token"], host["h"], host["c"], R.enc_rows(S, host))
    err = {k: _rel(S[k], ref[k]) for k in ("h_new", "c_new", "pred", "act")}
    z = ref["logits"]
    scale = float(z.abs().max())
    delta = DELTA_STEP * scale
    ntiles = S["pmax"].shape[0]
    zp = torch.full((B, ntiles * 16), float("-inf"), dtype=torch.float64)
    zp[:, :V] = z
    zt = zp.reshape(B, ntiles, 16)
    pmax, pidx = S["pmax"].cpu().double().t(), S["pidx"].cpu().long().t()        # (B, tiles)
    err["pmax"] = float((pmax - zt.max(-1).values).abs().max()) / scale
    kt, gap_t, near_t = R.argmax_within(zt, delta)
    assert int(pidx.min()) >= 0 and int(pidx.max()) < V, (name, "a padding class (or nothing) won a tile")
    tile0 = torch.arange(ntiles)[None, :] * 16
    assert torch.all((pidx >= tile0) & (pidx < tile0 + 16)), (name, "tile index outside its tile")
    sure = gap_t > delta
    assert torch.equal(pidx[sure], (tile0 + kt)[sure]), (name, "tile argmax", int((pidx[sure] != (tile0 + kt)[sure]).sum()))
    assert bool(near_t.gather(2, (pidx - tile0)[..., None]).all()), (name, "a tile's index is not within delta of its maximum")
    # the class the step chose: the tiles' (max, index) pairs reduced with torch.argmax's lowest-index rule -- the control kernel's reduction
    best = pmax.max(1, keepdim=True).values
    k_dev = torch.where(pmax == best, pidx, torch.full_like(pidx, 1 << 40)).min(1).values
    k64, gap, _ = R.argmax_within(z, delta)
    assert torch.equal(k_dev[gap > delta], k64[gap > delta]), (name, "argmax")
    assert bool((z.gather(1, k_dev[:, None])[:, 0] >= z.max(1).values - delta).all()), (name, "argmax not within delta of the maximum")
    exp = R.control(host, k_dev.numpy(), _np(S["h_new"]), _np(S["c_new"]), blank, n_steps)
    for k in ("token", "t", "frame_count", "count", "hyps"):
        np.testing.assert_array_equal(_np(S[k]), exp[k], err_msg="%s: %s" % (name, k))
    np.testing.assert_array_equal(_np(S["done8"]).astype(bool), exp["done"], err_msg="%s: done" % name)
    assert int(S["n_done"][0]) == exp["n_done"], (name, "n_done", int(S["n_done"][0]), exp["n_done"])
    for k in ("h", "c"):
        assert np.array_equal(_np(S[k]), exp[k]), (name, k, "state not the selected candidate / old value")
    nb = int(((k_dev.numpy() != blank) & ~host["done"]).sum())
    print("greedy step %-20s %s  gate-max %.1f  non-blank %d/%d" % (name, "  ".join("%s %.2e" % kv for kv in err.items()), ref["gate_max"], nb, B))
    bad = {k: v for k, v in err.items() if not v < gate}
    assert not bad, (name, bad, gate)
    return err, ref, k_dev


@pytest.mark.parametrize("case", STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_fused_step_matches_float64(case):
    name, B, L, (E, H, P, J), V, blank, n_steps, (wscale, bscale) = case
    pr, jn = R.modules(V, E, H, P, J, L, 300 + B + L)
    with torch.no_grad():
        for n, p in pr.rnn.named_parameters():
            p.mul_(wscale if n.startswith("weight") else bscale)
    pr, jn = pr.to(DEV), jn.to(DEV)
    P64 = R.params64(pr, jn)
    T = 7
    gs, S, W, desc = _fused_setup(pr, jn, blank, n_steps, B, T)
    assert W["Vp"] == (V + 15) // 16 * 16
    host = R.random_state(S, np.random.RandomState(1000 + B), V, n_steps)
    _run_step(desc)
    err, ref, _ = _check_step(name, S, host, P64, V, blank, n_steps, GATE_STEP_SATURATED if wscale != 1 else GATE_STEP)
    assert (ref["gate_max"] > 90.0) == (bscale != 1), ref["gate_max"]


TIE_CASES = [("v73_15_16", 73, (15, 16)), ("v73_3_last", 73, (3, 72)), ("v73_all", 73, None),
             ("v5002_15_16", 5002, (15, 16)), ("v5002_3_last", 5002, (3, 5001)), ("v5008_all", 5008, None), ("v17_all", 17, None)]


@pytest.mark.parametrize("blank", [0, -1])
@pytest.mark.parametrize("case", TIE_CASES, ids=[c[0] for c in TIE_CASES])
def test_fused_step_ties_take_the_lowest_index(case, blank):
    """ffn_out rows duplicated so that two classes (or all of them) have bit-identical logits and beat every other class by a wide margin."""
    name, V, tied = case
    blank = blank % V
    B, L, (E, H, P, J) = 17, 2, (32, 32, 32, 32)
    pr, jn = R.modules(V, E, H, P, J, L, 77)
    with torch.no_grad():
        w, b = jn.ffn_out.weight, jn.ffn_out.bias
        if tied is None:
            w.copy_(w[5].expand_as(w).clone())
            b.fill_(float(b[5]))
            expect = 0
        else:
            for i in tied:
                w[i] = w[tied[0]]
                b[i] = float(b.max()) + 10.0 if i == tied[0] else b[tied[0]]
            expect = min(tied)
    pr, jn = pr.to(DEV), jn.to(DEV)
    P64 = R.params64(pr, jn)
    T = 5
    gs, S, W, desc = _fused_setup(pr, jn, blank, 3, B, T)
    host = R.random_state(S, np.random.RandomState(55), V, 3)
    _run_step(desc)
    z = R.step64(P64, host["token"], host["h"], host["c"], R.enc_rows(S, host))["logits"]
    cls = list(range(V)) if tied is None else list(tied)
    zc = z[:, cls]
    assert float((zc.max(1).values - zc.min(1).values).max()) <= 1e-12 * float(z.abs().max())      # tied up to float64 rounding
    if tied is not None:                                 # ... and far ahead of every other class
        rest = z.clone()
        rest[:, cls] = float("-inf")
        assert float((zc.min(1).values - rest.max(1).values).min()) > 1.0
    _, _, k_dev = _check_step("tie_%s_blank%d" % (name, blank), S, host, P64, V, blank, 3, GATE_STEP)
    assert torch.all(k_dev == expect)
    live = ~host["done"]
    if expect != blank:
        assert np.all(_np(S["token"])[live] == expect)
    pidx = S["pidx"].cpu().long()
    if tied is not None:                                 # the tile(s) holding the tied classes
        for i in tied:
            assert torch.all(pidx[i // 16] == min(j for j in tied if j // 16 == i // 16))
    else:
        assert torch.all(pidx == (torch.arange(pidx.shape[0]) * 16)[:, None])


# ---------------------------------------------------------------------------------------------------------------------------------------
# whole searches
# ---------------------------------------------------------------------------------------------------------------------------------------
HEADS = {"small": dict(V=73, E=48, H=80, P=96, J=64, L=2, enc_dim=144, seed=51),
         "config4": dict(V=5002, E=256, H=256, P=512, J=512, L=2, enc_dim=512, seed=53)}


def _head(name):
    h = HEADS[name]
    pr, jn = R.modules(h["V"], h["E"], h["H"], h["P"], h["J"], h["L"], h["seed"], enc_dim=h["enc_dim"], shaped=True)
    return pr.to(DEV), jn.to(DEV), h


# head, B, n_steps, use_graph, carried start state
SEARCH_CASES = [("small", 64, 1, True, False), ("small", 64, 64, False, True), ("config4", 64, 4, True, False), ("config4", 33, 64, True, True),
                ("small", 65, 3, True, True), ("config4", 65, 2, False, False)]


@pytest.mark.parametrize("case", SEARCH_CASES, ids=["%s_b%d_n%d_%s%s" % (c[0], c[1], c[2], "graph" if c[3] else "eager", "_carried" if c[4] else "")
                                                    for c in SEARCH_CASES])
def test_search_matches_float64_loop(case):
    import greedy
    head, B, n_steps, use_graph, carried = case
    pr, jn, h = _head(head)
    T = 14
    rs = np.random.RandomState(B * 7 + n_steps)
    enc = torch.from_numpy(rs.standard_normal((B, T, h["enc_dim"])).astype(np.float32)).to(DEV)
    lens = rs.randint(0, T + 1, B)
    lens[0], lens[-1] = T, 0
    token0 = state0 = None
    if carried:
        token0 = torch.from_numpy(rs.randint(0, h["V"], B)).to(DEV)
        state0 = (torch.from_numpy(rs.uniform(-0.5, 0.5, (h["L"], B, h["H"])).astype(np.float32)).to(DEV),
                  torch.from_numpy(rs.standard_normal((h["L"], B, h["H"])).astype(np.float32)).to(DEV))
    gs = greedy.BatchedGreedySearch(pr, jn, blank=0, n_steps=n_steps, steps_per_replay=16, use_graph=use_graph)
    assert gs._fused_ok(B, DEV) == (B <= 64)
    res = gs.search(enc, lens, token=token0, state=state0)
    clean, ntok, serr = R.check_search(pr, jn, enc, lens, 0, n_steps, res, DELTA_SEARCH, token0, state0)
    # ... and continued from the state that search returned, on new frames (the float64 loop starts from the same f32 state)
    enc2 = torch.from_numpy(rs.standard_normal((B, T, h["enc_dim"])).astype(np.float32)).to(DEV)
    lens2 = rs.randint(0, T + 1, B)
    tok1, st1 = res[1]
    res2 = gs.search(enc2, lens2, token=tok1, state=st1)
    clean2, ntok2, serr2 = R.check_search(pr, jn, enc2, lens2, 0, n_steps, res2, DELTA_SEARCH, tok1, st1)
    print("greedy search %-32s clean streams %d + %d of %d, tokens %d + %d, state error %.2e" %
          (head + str(case[1:]), clean, clean2, B, ntok, ntok2, max(serr, serr2)))
    assert clean >= 0.75 * B and clean2 >= 0.75 * B, (clean, clean2)
    assert ntok >= B and ntok2 >= B
    assert max(serr, serr2) < GATE_SEARCH_STATE


@pytest.mark.parametrize("B", [64, 65])
def test_search_with_no_frames_returns_the_state_unchanged(B):
    import greedy
    pr, jn, h = _head("small")
    rs = np.random.RandomState(9)
    token0 = torch.from_numpy(rs.randint(0, h["V"], B)).to(DEV)
    state0 = tuple(torch.from_numpy(rs.standard_normal((h["L"], B, h["H"])).astype(np.float32)).to(DEV) for _ in range(2))
    enc = torch.from_numpy(rs.standard_normal((B, 6, h["enc_dim"])).astype(np.float32)).to(DEV)
    for use_graph in (True, False):
        hyps, (tok, (hh, cc)) = greedy.BatchedGreedySearch(pr, jn, n_steps=4, use_graph=use_graph).search(enc, [0] * B, token=token0, state=state0)
        assert hyps == [[]] * B
        assert torch.equal(tok, token0) and torch.equal(hh, state0[0]) and torch.equal(cc, state0[1])


# ---------------------------------------------------------------------------------------------------------------------------------------
# one search object across weight updates
# ---------------------------------------------------------------------------------------------------------------------------------------
def _update_inplace(pr, jn, rs):
    with torch.no_grad():
        for p in list(pr.parameters()) + list(jn.parameters()):
            p.add_(torch.from_numpy(0.05 * rs.standard_normal(tuple(p.shape)).astype(np.float32)).to(DEV))


def _update_data(pr, jn, rs):
    for p in list(pr.parameters()) + list(jn.parameters()):
        p.data = p.data + torch.from_numpy(0.05 * rs.standard_normal(tuple(p.shape)).astype(np.float32)).to(DEV)


def _update_state_dict(pr, jn, rs):
    for m in (pr, jn):
        m.load_state_dict({k: v + torch.from_numpy(0.05 * rs.standard_normal(tuple(v.shape)).astype(np.float32)).to(DEV)
                           for k, v in m.state_dict().items()})


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("update", ["inplace", "data", "load_state_dict", "trainer"])
def test_reused_search_follows_weight_updates(update, fused):
    """A search object kept across an update decodes with the new weights: tokens and final state equal to a freshly built object's."""
    import greedy
    import trainer as TR
    pr, jn, h = _head("small")
    B, T = 16, 12
    rs = np.random.RandomState(3)
    enc = torch.from_numpy(rs.standard_normal((B, T, h["enc_dim"])).astype(np.float32)).to(DEV)
    lens = rs.randint(1, T + 1, B)
    params = list(pr.parameters()) + list(jn.parameters())
    if update == "trainer":             # built first: the constructor re-points every parameter into its flat buffer
        tr = TR.DataParallelTrainer([pr, jn], lambda mb: sum((p * p).sum() for p in params), lr=1e-2, warmup_steps=1, accum_grad=1)
    make = lambda: greedy.BatchedGreedySearch(pr, jn, n_steps=3, steps_per_replay=8, use_graph=True, fused=fused)
    gs = make()
    before = gs.search(enc, lens)
    if update == "trainer":
        tr.step([None])
        torch.cuda.synchronize()
    else:
        {"inplace": _update_inplace, "data": _update_data, "load_state_dict": _update_state_dict}[update](pr, jn, rs)
    after = gs.search(enc, lens)
    fresh = make().search(enc, lens)
    assert not torch.equal(before[1][1][0], fresh[1][1][0]), "the update did not change the search's result"
    assert after[0] == fresh[0], "reused search: tokens of the weights before the update"
    assert torch.equal(after[1][0], fresh[1][0]) and torch.equal(after[1][1][0], fresh[1][1][0]) and torch.equal(after[1][1][1], fresh[1][1][1])
