"""GPU: the chunk-lookahead greedy step (csrc/greedy.hip: cfm_greedy_chunk_begin / cfm_greedy_chunk_step) through the C ABI, and
greedy.ChunkGreedySearch around it.

  4. one cfm_greedy_chunk_step on random states against the float64 restatement (tests/greedy_chunk_ref.py): the joint activations and the
     per-row 16-class-tile maxima within test_greedy_step_gpu.py's 2e-6 (max|d| / max|ref|), the argmax by the margin rule, the control
     state exactly (greedy_ref.control applied frame by frame), the state of streams that did not emit bit-unchanged; and
     cfm_greedy_chunk_begin's enc_ffn product and reset;
  5. whole streams: the greedy.npz utterances (V = 5002 included) in chunks of 16 exactly against chained search() calls and against the
     golden tokens; 64 ragged streams against the float64 loop (delta 1e-4) from a carried state;
  6. the captured graph is reused across chunks, re-captured after a weight change, and reset(streams) of a subset leaves the others'
     tokens identical to an undisturbed run."""
import ctypes

import numpy as np
import pytest
import torch

import greedy_chunk_ref as C
import greedy_ref as R
import synth
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")

GATE = 2e-6                      # act, pmax: the gate of cfm_greedy_step's test
GATE_LSTM_SATURATED = 6e-5       # h_new / c_new / pred with saturated gates, as in test_greedy_step_gpu.py
DELTA_STEP = 1e-5
DELTA_SEARCH = 1e-4
BLANK_BIAS = 1.5

# name, B, L, (E, H, P, J), V, blank, n_steps, chunk, LSTM bias scale
STEP_CASES = [
    ("b1_c1_min", 1, 1, (16, 16, 16, 16), 16, 0, 1, 1, 1),
    ("b15_l2_v17_c4", 15, 2, (32, 48, 16, 32), 17, 16, 3, 4, 1),
    ("b16_l3_v31_c16", 16, 3, (48, 16, 32, 64), 31, 0, 2, 16, 1),
    ("b17_l4_v73_c32", 17, 4, (16, 32, 48, 16), 73, 72, 64, 32, 1),
    ("b33_l1_v5008_c4", 33, 1, (64, 96, 80, 48), 5008, 0, 4, 4, 1),
    ("b48_cfg4_v5002_c16", 48, 2, (256, 256, 512, 512), 5002, 5001, 4, 16, 1),
    ("b63_l3_v5002_c32", 63, 3, (32, 64, 16, 48), 5002, 0, 3, 32, 1),
    ("b64_cfg4_v5002_c16", 64, 2, (256, 256, 512, 512), 5002, 0, 64, 16, 1),
    ("b64_l4_v5008_c1", 64, 4, (64, 32, 48, 32), 5008, 5007, 2, 1, 1),
    ("b40_saturated_bias_c16", 40, 2, (64, 64, 32, 32), 73, 0, 3, 16, 1000),
]


def _np(x):
    return x.detach().cpu().numpy().copy()


def _rel(got, ref):
    ref = ref.double()
    return float((got.double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def _call(cg, name):
    import cfm
    cfm.check(getattr(cfm.lib(), name)(ctypes.byref(cg._desc), cfm.stream()), name)
    torch.cuda.synchronize()


def _setup(pr, jn, B, chunk, blank, n_steps, V, seed):
    import greedy
    pr, jn = pr.to(DEV), jn.to(DEV)
    cg = greedy.ChunkGreedySearch(pr, jn, B, chunk, blank=blank, n_steps=n_steps, max_tokens=40)
    assert cg.fused
    cg._prepare()
    host = C.random_chunk_state(cg.S, np.random.RandomState(seed), V, n_steps, chunk)
    return cg, host, R.params64(pr, jn)


def _check_chunk_step(name, cg, host, P64, V, blank, n_steps, chunk, gate_lstm=GATE, hyp_cap=None):
    """Everything one cfm_greedy_chunk_step wrote against the float64 restatement.  hyp_cap: the descriptor's capacity when it was lowered
    below some counts (the overflow path).  Returns (k per compact row as the device chose it, float64 logits of those rows, rows)."""
    S, B = cg.S, cg.B
    ref = C.chunk_logits64(P64, host, S["enc_proj"])
    live = host["t"] < host["lens"]
    err = {k: _rel(S[k], ref[k]) for k in ("h_new", "c_new", "pred")} if live.any() else {}       # nothing live: the predictor launches do nothing
    # the compact row list: every frame t .. lens - 1 of every live stream, in stream order
    want = [b * chunk + f for b in range(B) if live[b] for f in range(host["t"][b], host["lens"][b])]
    n_rows = int(S["n_rows"][0])
    rows = S["rows"].cpu().numpy()[:n_rows].tolist()
    assert rows == want, (name, n_rows, len(want))
    cnt = np.where(live, host["lens"] - host["t"], 0)
    np.testing.assert_array_equal(_np(S["row_cnt"]), cnt)
    np.testing.assert_array_equal(_np(S["row_off"]), np.concatenate([[0], np.cumsum(cnt)[:-1]]))
    assert int(S["steps"][0]) == int(live.any())
    k_frames = np.full((B, chunk), -1, dtype=np.int64)
    k_dev = z = None
    if n_rows:
        idx = torch.tensor(rows)
        z = ref["logits"].reshape(B * chunk, V)[idx]
        scale = float(z.abs().max())
        delta = DELTA_STEP * scale
        err["act"] = _rel(S["act"][:n_rows], ref["act"].reshape(B * chunk, -1)[idx])
        ntiles = S["pmax"].shape[1]
        zp = torch.full((n_rows, ntiles * 16), float("-inf"), dtype=torch.float64)
        zp[:, :V] = z
        zt = zp.reshape(n_rows, ntiles, 16)
        pmax, pidx = S["pmax"][:n_rows].cpu().double(), S["pidx"][:n_rows].cpu().long()
        err["pmax"] = float((pmax - zt.max(-1).values).abs().max()) / scale
        kt, gap_t, near_t = R.argmax_within(zt, delta)
        tile0 = torch.arange(ntiles)[None, :] * 16
        assert int(pidx.min()) >= 0 and int(pidx.max()) < V, (name, "a padding class (or nothing) won a tile")
        assert torch.all((pidx >= tile0) & (pidx < tile0 + 16)), (name, "tile index outside its tile")
        sure = gap_t > delta
        assert torch.equal(pidx[sure], (tile0 + kt)[sure]), (name, "tile argmax")
        assert bool(near_t.gather(2, (pidx - tile0)[..., None]).all()), (name, "a tile's index is not within delta of its maximum")
        best = pmax.max(1, keepdim=True).values
        k_dev = torch.where(pmax == best, pidx, torch.full_like(pidx, 1 << 40)).min(1).values
        k64, gap, _ = R.argmax_within(z, delta)
        assert torch.equal(k_dev[gap > delta], k64[gap > delta]), (name, "argmax")
        assert bool((z.gather(1, k_dev[:, None])[:, 0] >= z.max(1).values - delta).all()), (name, "argmax not within delta of the maximum")
        k_frames.reshape(-1)[idx.numpy()] = k_dev.numpy()
    exp, singles = C.lookahead_by_single_steps(host, k_frames, _np(S["h_new"]), _np(S["c_new"]), blank, n_steps)
    emitted = exp["count"] != host["count"]
    over = emitted & (host["count"] >= hyp_cap) if hyp_cap is not None else np.zeros(B, dtype=bool)
    exp["hyps"][over] = host["hyps"][over]               # counted, not stored: no slot of a full buffer is written
    assert int(S["overflow"][0]) == int(over.any()), (name, "overflow flag")
    for k in ("token", "t", "frame_count", "count", "hyps"):
        np.testing.assert_array_equal(_np(S[k]), exp[k], err_msg="%s: %s" % (name, k))
    np.testing.assert_array_equal(_np(S["done8"]).astype(bool), exp["done"], err_msg="%s: done" % name)
    assert int(S["n_done"][0]) == exp["n_done"], (name, int(S["n_done"][0]), exp["n_done"])
    for k in ("h", "c"):
        got = _np(S[k])
        assert np.array_equal(got, exp[k]), (name, k, "state not the selected candidate / old value")
        assert np.array_equal(got[:, ~emitted], host[k][:, ~emitted]), (name, k, "a stream that did not emit changed")
    print("chunk step %-24s %s  rows %d  emitted %d/%d live (%d past the capacity)  single-frame steps %d" %
          (name, "  ".join("%s %.2e" % kv for kv in err.items()), n_rows, int(emitted.sum()), int(live.sum()), int(over.sum()), singles))
    bad = {k: v for k, v in err.items() if not v < (gate_lstm if k in ("h_new", "c_new", "pred") else GATE)}
    assert not bad, (name, bad)
    return k_dev, z, rows, ref


@pytest.mark.parametrize("case", STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_chunk_step_matches_float64(case):
    name, B, L, (E, H, P, J), V, blank, n_steps, chunk, bscale = case
    pr, jn = R.modules(V, E, H, P, J, L, 600 + B + L)
    with torch.no_grad():
        jn.ffn_out.bias[blank] += BLANK_BIAS
        for n, p in pr.rnn.named_parameters():
            if n.startswith("bias"):
                p.mul_(bscale)
    cg, host, P64 = _setup(pr, jn, B, chunk, blank, n_steps, V, 4000 + B)
    _call(cg, "cfm_greedy_chunk_step")
    _, _, _, ref = _check_chunk_step(name, cg, host, P64, V, blank, n_steps, chunk, GATE_LSTM_SATURATED if bscale != 1 else GATE)
    assert (ref["gate_max"] > 90.0) == (bscale != 1)


def test_chunk_step_full_hypothesis_buffer_counts_but_does_not_store():
    """hyp_cap below some streams' counts: their symbol is counted, the overflow flag set, and no slot of the buffer -- the last one
    included -- is written; decode() turns the flag into an error."""
    B, chunk, V, n_steps = 48, 16, 73, 3
    pr, jn = R.modules(V, 32, 48, 32, 64, 2, 93)
    with torch.no_grad():
        jn.ffn_out.bias[0] += BLANK_BIAS
    cg, host, P64 = _setup(pr, jn, B, chunk, 0, n_steps, V, 4100)
    cap = 12
    cg._desc.hyp_cap = cap
    live = host["t"] < host["lens"]
    b0 = int(np.flatnonzero(live)[0])                    # one live stream exactly at the capacity: the slot past the end
    cg.S["count"][b0] = cap
    host["count"][b0] = cap
    assert (live & (host["count"] > cap)).any() and (live & (host["count"] < cap)).any()
    _call(cg, "cfm_greedy_chunk_step")
    _check_chunk_step("overflow", cg, host, P64, V, 0, n_steps, chunk, hyp_cap=cap)
    assert int(cg.S["overflow"][0]) == 1
    cg.reset()
    cg.S["overflow"].zero_()
    cg._grow(2 * chunk * n_steps)                        # room for the chunk, so that decode() keeps this descriptor ...
    cg._prepare()
    cg._desc.hyp_cap = 0                                 # as if the buffer were full: the first emission overflows
    enc = torch.from_numpy(np.random.RandomState(1).standard_normal((B, chunk, 64)).astype(np.float32)).to(DEV)
    with pytest.raises(RuntimeError, match="hypothesis buffer"):
        cg.decode(enc)


TIE_CASES = [("v73_15_16", 73, (15, 16)), ("v73_3_last", 73, (3, 72)), ("v73_1_2", 73, (1, 2)), ("v73_all", 73, None),
             ("v5002_15_16", 5002, (15, 16)), ("v5002_3_last", 5002, (3, 5001)), ("v5002_31_32", 5002, (31, 32)), ("v5008_all", 5008, None), ("v17_all", 17, None)]


@pytest.mark.parametrize("blank", [0, -1, 3])
@pytest.mark.parametrize("case", TIE_CASES, ids=[c[0] for c in TIE_CASES])
def test_chunk_step_ties_take_the_lowest_index(case, blank):
    """ffn_out rows duplicated so that two classes (inside one 16-class tile, in neighbouring tiles -- 31 / 32 also in different halves of a
    wavefront's 32 classes --, first and last) or all of them have bit-identical logits on every row and beat every other class by a wide
    margin: the lowest index wins within a lane, across lane groups, across tiles (torch.argmax's rule); with blank 3 / 0 / V - 1 among the
    tied classes the tie is blank against non-blank."""
    name, V, tied = case
    blank = blank % V
    B, chunk, n_steps, L, (E, H, P, J) = 19, 16, 3, 2, (32, 32, 32, 32)
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
    cg, host, P64 = _setup(pr, jn, B, chunk, blank, n_steps, V, 4200)
    _call(cg, "cfm_greedy_chunk_step")
    k_dev, z, rows, _ = _check_chunk_step("tie_%s_blank%d" % (name, blank), cg, host, P64, V, blank, n_steps, chunk)
    cls = list(range(V)) if tied is None else list(tied)
    zc = z[:, cls]
    assert float((zc.max(1).values - zc.min(1).values).max()) <= 1e-12 * float(z.abs().max())      # tied up to float64 rounding
    if tied is not None:
        rest = z.clone()
        rest[:, cls] = float("-inf")
        assert float((zc.min(1).values - rest.max(1).values).min()) > 1.0
    assert len(rows) > 10 and torch.all(k_dev == expect)
    pidx = cg.S["pidx"][:len(rows)].cpu().long()
    if tied is not None:
        for i in tied:
            assert torch.all(pidx[:, i // 16] == min(j for j in tied if j // 16 == i // 16))
    else:
        assert torch.all(pidx == (torch.arange(pidx.shape[1]) * 16)[None, :])
    live = host["t"] < host["lens"]
    got_t, got_tok = _np(cg.S["t"]), _np(cg.S["token"])
    if expect == blank:                                  # the blank wins the tie: no emission, every live stream is done with the chunk
        assert np.array_equal(got_t[live], host["lens"][live]) and np.array_equal(got_tok, host["token"])
    else:                                                # the symbol wins it: every live stream emits on its current frame
        assert np.all(got_tok[live] == expect) and np.all((got_t[live] == host["t"][live]) | (got_t[live] == host["t"][live] + 1))


@pytest.mark.parametrize("carry", [True, False])
def test_chunk_begin_applies_enc_ffn_and_resets(carry):
    import greedy
    B, chunk, V, (E, H, P, J), D = 37, 16, 73, (32, 48, 32, 64), 144
    pr, jn = R.modules(V, E, H, P, J, 2, 91, enc_dim=D)
    pr, jn = pr.to(DEV), jn.to(DEV)
    cg = greedy.ChunkGreedySearch(pr, jn, B, chunk, n_steps=3, carry=carry, max_tokens=40)
    cg._prepare()
    S = cg.S
    rs = np.random.RandomState(5)
    host = C.random_chunk_state(S, rs, V, 3, chunk)
    S["enc_proj"].fill_(float("nan"))
    S["steps"].fill_(7)
    enc = torch.from_numpy(rs.standard_normal((B, chunk, D)).astype(np.float32)).to(DEV)
    cg._desc.enc = enc.data_ptr()
    _call(cg, "cfm_greedy_chunk_begin")
    P64 = R.params64(pr, jn)
    ref = enc.double().cpu() @ P64["j.enc_ffn.weight"].t() + P64["j.enc_ffn.bias"]
    assert _rel(S["enc_proj"], ref) < GATE
    idle = host["lens"] <= 0
    assert int(S["steps"][0]) == 0 and int(S["n_done"][0]) == int(idle.sum())
    np.testing.assert_array_equal(_np(S["done8"]).astype(bool), idle)
    assert not _np(S["t"]).any() and not _np(S["frame_count"]).any()
    np.testing.assert_array_equal(_np(S["count"]), host["count"])
    np.testing.assert_array_equal(_np(S["hyps"]), host["hyps"])
    keep = idle if not carry else np.ones(B, dtype=bool)
    np.testing.assert_array_equal(_np(S["token"])[keep], host["token"][keep])
    assert np.array_equal(_np(S["h"])[:, keep], host["h"][:, keep]) and np.array_equal(_np(S["c"])[:, keep], host["c"][:, keep])
    if not carry:
        assert not _np(S["token"])[~idle].any() and not _np(S["h"])[:, ~idle].any() and not _np(S["c"])[:, ~idle].any()


def test_limits_raise():
    import greedy
    pr, jn = R.modules(73, 48, 80, 96, 64, 2, 51)
    pr, jn = pr.to(DEV), jn.to(DEV)
    for B, chunk in ((65, 16), (4, 33)):
        with pytest.raises(RuntimeError):
            greedy.ChunkGreedySearch(pr, jn, B, chunk)
    pr2, jn2 = R.modules(73, 40, 80, 96, 64, 2, 51)
    with pytest.raises(RuntimeError):
        greedy.ChunkGreedySearch(pr2.to(DEV), jn2.to(DEV), 4, 16)


# ---------------------------------------------------------------------------------------------------------------------------------------
# whole streams
# ---------------------------------------------------------------------------------------------------------------------------------------
def _case_modules(c):
    pr, jn = R.modules(c["V"], c["embed"], c["hidden"], c["P"], c["J"], c["layers"], c["seed"], enc_dim=c["E"], shaped=True)
    return pr.to(DEV), jn.to(DEV)


def _bounds(cg, new, lens):
    most = max(len(n) for n in new)
    if not any(lens):
        assert cg.steps == 0
        return
    assert most <= cg.steps <= 1 + most, (cg.steps, most)
    assert cg.replays == max(1, -(-cg.steps // cg.steps_per_replay)), (cg.replays, cg.steps)


@pytest.mark.parametrize("use_graph", [True, False])
def test_golden_utterances_in_chunks_of_16(use_graph):
    import greedy
    g, meta = load_golden("greedy")
    assert any(c["V"] == 5002 for c in meta["cases"])
    for c in meta["cases"]:
        pr, jn = _case_modules(c)
        enc = torch.cat([torch.from_numpy(synth.normal(c["seed"] + 10 + u, (1, c["T"], c["E"]), 1.0)) for u in range(3)], 0).to(DEV)
        for carry in (True, False):
            cg = greedy.ChunkGreedySearch(pr, jn, 3, 16, n_steps=c["n_steps"], carry=carry, use_graph=use_graph, max_tokens=8)
            bs = greedy.BatchedGreedySearch(pr, jn, n_steps=c["n_steps"], steps_per_replay=8, use_graph=use_graph, fused=True)
            tok = st = None
            for piece, lens, raw in C.chunks_of(enc, c["lens"], 16):
                new = cg.decode(piece, lens)
                ref, (tok, st) = bs.search(raw, lens, token=tok if carry else None, state=st if carry else None)
                assert new == ref, (c["name"], carry, new, ref)
                _bounds(cg, new, lens)
            if carry:
                for u in range(3):
                    assert cg.hyps()[u] == g["%s_utt%d" % (c["name"], u)].tolist(), (c["name"], u)


HEADS = {"small": dict(V=73, E=48, H=80, P=96, J=64, L=2, enc_dim=144, seed=51),
         "config4": dict(V=5002, E=256, H=256, P=512, J=512, L=2, enc_dim=512, seed=53)}


def _head(name):
    h = HEADS[name]
    pr, jn = R.modules(h["V"], h["E"], h["H"], h["P"], h["J"], h["L"], h["seed"], enc_dim=h["enc_dim"], shaped=True)
    return pr.to(DEV), jn.to(DEV), h


@pytest.mark.parametrize("head,n_steps", [("small", 64), ("config4", 4), ("small", 1)])
def test_64_ragged_streams_match_float64_loop_from_a_carried_state(head, n_steps):
    import greedy
    pr, jn, h = _head(head)
    B, chunk = 64, 16
    rs = np.random.RandomState(B * 7 + n_steps)
    cg = greedy.ChunkGreedySearch(pr, jn, B, chunk, n_steps=n_steps, steps_per_replay=4)
    token0 = torch.from_numpy(rs.randint(0, h["V"], B)).to(DEV)
    state0 = (torch.from_numpy(rs.uniform(-0.5, 0.5, (h["L"], B, h["H"])).astype(np.float32)).to(DEV),
              torch.from_numpy(rs.standard_normal((h["L"], B, h["H"])).astype(np.float32)).to(DEV))
    cg.set_state(token0, state0)
    for rnd in range(2):                                 # the second chunk continues from the state the first left on the device
        enc = torch.from_numpy(rs.standard_normal((B, chunk, h["enc_dim"])).astype(np.float32)).to(DEV)
        lens = rs.randint(0, chunk + 1, B)
        lens[0], lens[-1] = chunk, 0
        tok_in, st_in = cg.state()
        new = cg.decode(enc, lens.tolist())
        _bounds(cg, new, lens.tolist())
        clean, ntok, serr = R.check_search(pr, jn, enc, lens, 0, n_steps, (new, cg.state()), DELTA_SEARCH, tok_in, st_in)
        print("chunk search %s n_steps %d round %d: clean streams %d of %d, tokens %d, steps %d, state error %.2e" % (head, n_steps, rnd, clean, B, ntok, cg.steps, serr))
        assert clean >= 0.75 * B and ntok >= B // 2 and serr < 7e-7


# ---------------------------------------------------------------------------------------------------------------------------------------
# one object across chunks, weight updates and partial resets
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_graph_reuse_recapture_and_partial_reset():
    import greedy
    pr, jn, h = _head("small")
    B, chunk, n = 16, 16, 4
    rs = np.random.RandomState(3)
    encs = [torch.from_numpy(rs.standard_normal((B, chunk, h["enc_dim"])).astype(np.float32)).to(DEV) for _ in range(n)]
    make = lambda: greedy.ChunkGreedySearch(pr, jn, B, chunk, n_steps=3, steps_per_replay=4, use_graph=True)
    cg = make()
    a = [cg.decode(e) for e in encs[:2]]
    graph = cg._graph
    assert graph is not None
    cg.decode(encs[2])
    assert cg._graph is graph, "the captured graph is reused across chunks"
    eager = greedy.ChunkGreedySearch(pr, jn, B, chunk, n_steps=3, use_graph=False)
    assert [eager.decode(e) for e in encs[:2]] == a
    # a subset starts new utterances while the others continue
    und, dis = make(), make()
    for e in encs[:2]:
        assert und.decode(e) == dis.decode(e)
    sub = [1, 5, 15]
    dis.reset(sub)
    fresh = make()
    for e in encs[2:]:
        u, d, f = und.decode(e), dis.decode(e), fresh.decode(e)
        for b in range(B):
            assert d[b] == (f[b] if b in sub else u[b]), b
    for b in range(B):
        assert dis.hyps()[b] == (fresh.hyps()[b] if b in sub else und.hyps()[b])
    # a weight change under the captured graph
    cg = make()
    before = cg.decode(encs[0])
    graph = cg._graph
    with torch.no_grad():
        for p in list(pr.parameters()) + list(jn.parameters()):
            p.add_(torch.from_numpy(0.05 * rs.standard_normal(tuple(p.shape)).astype(np.float32)).to(DEV))
    cg.reset()
    after = cg.decode(encs[0])
    assert cg._graph is not graph, "the graph holds the old packs: it must be captured again"
    assert after == make().decode(encs[0]) and after != before
