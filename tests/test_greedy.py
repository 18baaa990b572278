"""RNN-T greedy search: the reference's basic_greedy_search (model.py:215-269).

tests/golden/greedy.npz holds token sequences produced with the REFERENCE's RNNPredictor.forward_step and TransducerJoint.forward doing
every step (the loop around them restated in the generator: model.py does not import without torchaudio).  Checked against them:
  * the oracle's restatement of loop + predictor step + joint (CPU, `not gpu`);
  * the drop-in RNNPredictor (predictor.py) driven by the same loop (CPU);
  * greedy.BatchedGreedySearch -- all utterances of a case as ONE batch, control state in tensors, no per-step host decisions -- eagerly
    on the CPU here, and on the GPU with the steps captured in a HIP graph (`-m gpu`), including ragged lengths, the per-frame cap
    (n_steps 1, 3, 4) and a search continued from a carried (token, LSTM state).
Token sequences are integers: the comparison is exact.
Against float64 (tests/greedy_ref.py; the fused HIP step in tests/test_greedy_step_gpu.py): one step of the torch-operation form on a random
state, and its search by the margin rule (tokens equal up to the first decision whose two best float64 logits are within 1e-4)."""
import numpy as np
import pytest
import torch

import synth
from conftest import load_golden


def _case_modules(c):
    import joint
    import predictor
    pr = predictor.RNNPredictor(c["V"], c["embed"], c["P"], c["hidden"], 0.1, c["layers"]).eval()
    jn = joint.TransducerJoint(c["V"], c["E"], c["P"], c["J"]).eval()
    synth.load_synth_(pr, c["seed"])
    synth.load_synth_(jn, c["seed"] + 1)
    synth.greedy_joint_(jn, c["V"])
    return pr, jn


def _enc(c, u):
    return torch.from_numpy(synth.normal(c["seed"] + 10 + u, (1, c["T"], c["E"]), 1.0))


def _cases():
    g, meta = load_golden("greedy")
    return g, meta["cases"]


def test_oracle_greedy_search_matches_reference_tokens():
    from oracle import conformer_oracle as O
    g, cases = _cases()
    for c in cases:
        pr, jn = _case_modules(c)
        P = {"p." + k: v.detach() for k, v in pr.state_dict().items()}
        P.update({"j." + k: v.detach() for k, v in jn.state_dict().items()})
        for u, n in enumerate(c["lens"]):
            enc = _enc(c, u)[0]
            hyps, _ = O.rnnt_greedy_search(P, "p.", "j.", enc, n, n_steps=c["n_steps"])
            assert hyps == g["%s_utt%d" % (c["name"], u)].tolist(), (c["name"], u)
        enc = _enc(c, 0)[0]
        half = c["T"] // 2
        a, (tok, st) = O.rnnt_greedy_search(P, "p.", "j.", enc[:half], half, n_steps=c["n_steps"])
        b, _ = O.rnnt_greedy_search(P, "p.", "j.", enc[half:], c["T"] - half, n_steps=c["n_steps"], token=tok, state=st)
        assert a == g[c["name"] + "_utt0_first"].tolist() and b == g[c["name"] + "_utt0_second"].tolist()


def test_predictor_module_state_dict_and_step_semantics():
    """Parameter names / shapes of the reference's RNNPredictor, init_state, and forward_step's padding (1 = keep the old state)."""
    import predictor
    pr = predictor.RNNPredictor(73, 48, 96, 80, 0.1, 2).eval()
    names = sorted(pr.state_dict())
    assert names == sorted(["embed.weight", "projection.weight", "projection.bias"] +
                           ["rnn.%s_%s_l%d" % (a, b, l) for a in ("weight", "bias") for b in ("ih", "hh") for l in (0, 1)])
    synth.load_synth_(pr, 7)
    tok = torch.tensor([[5], [9]])
    h0, c0 = pr.init_state(tok)
    assert h0.shape == (2, 2, 80) and float(h0.abs().max()) == 0.0
    with torch.no_grad():
        out, (h1, c1) = pr.forward_step(tok, torch.zeros(2, 1), (h0, c0))
        out2, (h2, c2) = pr.forward_step(tok, torch.tensor([[0.0], [1.0]]), (h1, c1))
        full = pr(torch.tensor([[5, 5], [9, 9]]))
    assert out.shape == (2, 1, 96) and torch.allclose(full[:, 0], out[:, 0], atol=1e-6) and torch.allclose(full[:, 1], out2[:, 0], atol=1e-6)
    assert torch.equal(h2[:, 1], h1[:, 1]) and torch.equal(c2[:, 1], c1[:, 1]) and not torch.equal(h2[:, 0], h1[:, 0])


def _batched(c, g, device, use_graph, fused=False):
    import greedy
    pr, jn = _case_modules(c)
    pr, jn = pr.to(device), jn.to(device)
    enc = torch.cat([_enc(c, u) for u in range(3)], 0).to(device)
    gs = greedy.BatchedGreedySearch(pr, jn, blank=0, n_steps=c["n_steps"], steps_per_replay=8, use_graph=use_graph, fused=fused)
    hyps, _ = gs.search(enc, c["lens"])
    for u in range(3):
        assert hyps[u] == g["%s_utt%d" % (c["name"], u)].tolist(), (c["name"], u, len(hyps[u]))
    # again through the same object (captured graph reused), then a continued search: first halves, then the rest from the carried state
    hyps2, _ = gs.search(enc, c["lens"])
    assert hyps2 == hyps
    half = c["T"] // 2
    first, (tok, st) = gs_half(greedy, pr, jn, c, enc[:1, :half], [half], use_graph, fused=fused)
    second, _ = gs_half(greedy, pr, jn, c, enc[:1, half:], [c["T"] - half], use_graph, tok, st, fused=fused)
    assert first[0] == g[c["name"] + "_utt0_first"].tolist() and second[0] == g[c["name"] + "_utt0_second"].tolist()


def gs_half(greedy, pr, jn, c, enc, lens, use_graph, tok=None, st=None, fused=False):
    gs = greedy.BatchedGreedySearch(pr, jn, blank=0, n_steps=c["n_steps"], steps_per_replay=8, use_graph=use_graph, fused=fused)
    return gs.search(enc.contiguous(), lens, token=tok, state=st)


def test_batched_search_on_cpu_matches_reference_tokens():
    g, cases = _cases()
    for c in cases:
        if c["V"] > 1000:
            continue                                   # the 5002-class case runs on the GPU
        _batched(c, g, torch.device("cpu"), False)


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("use_graph", [True, False])
def test_batched_search_on_gpu_matches_reference_tokens(use_graph, fused):
    """fused: one step = six launches of csrc/greedy.hip (f32 MFMA products, LSTM cell / tanh / argmax epilogues, control kernel) instead of
    the torch-operation form; both must reproduce the reference-module tokens."""
    g, cases = _cases()
    for c in cases:
        _batched(c, g, torch.device("cuda"), use_graph, fused)


@pytest.mark.gpu
def test_fused_search_40_streams_matches_torch_form():
    """More than one 16-stream tile (B = 40, ragged lengths, some streams empty): the fused step against the torch-operation form."""
    import greedy
    g, cases = _cases()
    c = [x for x in cases if x["name"] == "small"][0]
    pr, jn = _case_modules(c)
    pr, jn = pr.cuda(), jn.cuda()
    B, T = 40, c["T"]
    enc = torch.cat([torch.from_numpy(synth.normal(700 + b, (1, T, c["E"]), 1.0)) for b in range(B)]).cuda()
    lens = [(7 * b) % (T + 1) for b in range(B)]
    res = []
    for fused in (True, False):
        gs = greedy.BatchedGreedySearch(pr, jn, blank=0, n_steps=c["n_steps"], steps_per_replay=16, use_graph=True, fused=fused)
        res.append(gs.search(enc, lens)[0])
    assert res[0] == res[1] and sum(len(h) for h in res[0]) > 50 and res[0][0] == []


# name, B, L, (E, H, P, J), V, blank, n_steps -- the torch-operation step (greedy.py _step: the CPU path, and the GPU's beyond 64 streams)
TORCH_STEP_CASES = [("b1_l1_v16", 1, 1, (16, 16, 16, 16), 16, 0, 1), ("b17_l2_v73", 17, 2, (48, 80, 96, 64), 73, 72, 3),
                    ("b65_l3_v31", 65, 3, (24, 40, 20, 36), 31, 0, 64), ("b33_l4_v5002", 33, 4, (64, 32, 48, 80), 5002, 5001, 2)]


@pytest.mark.parametrize("case", TORCH_STEP_CASES, ids=[c[0] for c in TORCH_STEP_CASES])
def test_torch_form_step_matches_float64(case):
    """One `_step` of the torch-operation form on a random state (tests/greedy_ref.py random_state) against the float64 restatement: the
    new LSTM state of the streams that emitted within 1e-6 (max|d| / max|ref|; measured 1.5e-7), everything else exactly."""
    import greedy
    import greedy_ref as R
    name, B, L, (E, H, P, J), V, blank, n_steps = case
    pr, jn = R.modules(V, E, H, P, J, L, 400 + B)
    gs = greedy.BatchedGreedySearch(pr, jn, blank=blank, n_steps=n_steps, use_graph=False, fused=False)
    S = gs._state(B, 7, torch.device("cpu"))
    host = R.random_state(S, np.random.RandomState(2000 + B), V, n_steps)
    with torch.no_grad():
        gs._step(S)
    ref = R.step64(R.params64(pr, jn), host["token"], host["h"], host["c"], R.enc_rows(S, host))
    k, gap, _ = R.argmax_within(ref["logits"], 0.0)
    assert float(gap.min()) > 1e-4 * float(ref["logits"].abs().max()), "the fixture has a near tie: the f32 argmax may go either way"
    exp = R.control(host, k.numpy(), ref["h_new"].numpy(), ref["c_new"].numpy(), blank, n_steps)
    for key in ("token", "t", "frame_count", "count", "hyps", "done"):
        np.testing.assert_array_equal(S[key].numpy(), exp[key], err_msg=key)
    nb = (k.numpy() != blank) & ~host["done"]
    assert 0 < nb.sum() < B or B == 1
    for key in ("h", "c"):
        got = S[key].numpy()
        np.testing.assert_array_equal(got[:, ~nb], host[key][:, ~nb], err_msg=key)
        new = ref[key + "_new"][:, torch.from_numpy(nb)]
        if nb.any():
            err = float(np.abs(got[:, nb] - new.numpy()).max() / float(new.abs().max()))
            assert err < 1e-6, (name, key, err)


def test_float64_search_matches_reference_tokens():
    """The margin-aware float64 loop (tests/greedy_ref.py search64, the checker of the GPU searches) reproduces the reference-module tokens
    up to its first close decision; at least one fixture utterance has none."""
    import greedy_ref as R
    g, cases = _cases()
    whole = 0
    for c in cases:
        pr, jn = _case_modules(c)
        P64 = R.params64(pr, jn)
        for u, n in enumerate(c["lens"]):
            enc_proj = _enc(c, u)[0].double() @ P64["j.enc_ffn.weight"].t() + P64["j.enc_ffn.bias"]
            hyps, _, first = R.search64(P64, enc_proj, n, 0, c["n_steps"], 1e-4)
            ref = g["%s_utt%d" % (c["name"], u)].tolist()
            assert hyps[:first] == ref[:first], (c["name"], u, first)
            whole += first is None and hyps == ref
    assert whole >= 6, whole


def test_torch_form_search_on_cpu_matches_float64_loop():
    """Eight ragged streams through the batched torch-operation form (eager, CPU) against the float64 loop by the margin rule, from a
    carried (token, LSTM state); final state of the streams without a close decision within 1e-6 (measured 7.5e-8)."""
    import greedy
    import greedy_ref as R
    g, cases = _cases()
    c = [x for x in cases if x["name"] == "small"][0]
    pr, jn = _case_modules(c)
    B, T = 8, c["T"]
    rs = np.random.RandomState(17)
    enc = torch.from_numpy(rs.standard_normal((B, T, c["E"])).astype(np.float32))
    lens = [T, 0, 3, 11, T, 7, 1, 20]
    tok0 = torch.from_numpy(rs.randint(0, c["V"], B))
    st0 = tuple(torch.from_numpy(rs.uniform(-0.5, 0.5, (c["layers"], B, c["hidden"])).astype(np.float32)) for _ in range(2))
    res = greedy.BatchedGreedySearch(pr, jn, blank=0, n_steps=c["n_steps"], use_graph=False, fused=False).search(enc, lens, token=tok0, state=st0)
    clean, ntok, serr = R.check_search(pr, jn, enc, lens, 0, c["n_steps"], res, 1e-4, tok0, st0)
    assert clean >= 6 and ntok >= 20 and serr < 1e-6, (clean, ntok, serr)
