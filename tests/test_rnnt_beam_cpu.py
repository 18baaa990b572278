"""CPU: the float64 RNN-T beam search of tests/rnnt_beam_ref.py, the specification of greedy.BeamSearch, checked on its own.

  * with nothing pruned (V = 3, at most 7 strings, beam 15) every finished hypothesis' score is the full RNN-T log-likelihood of its string
    (rnnt_ref's alpha recursion over logits made from the same predictor and joint), to 1e-9: the merging sums the alignments, all of them;
  * beam = 1 is the greedy search (greedy_ref.search64), also where that emits several symbols on a frame and where it hits max_symbols;
  * the named merge case has merges and is clear;
  * at least 80 % of the (case, utterance) pairs of the GPU test are clear: every recorded gap exceeds beam_delta."""
import numpy as np
import pytest
import torch

import greedy_ref as R
import rnnt_beam_ref as BR
import rnnt_ref


def _lattice_ll(P, enc_proj, n, tokens, blank):
    """log P(tokens | the n frames): logits[t, u] from the predictor after tokens[:u] and frame t, then rnnt_ref's recursion."""
    L, H = R.num_layers(P), P["p.rnn.weight_hh_l0"].shape[1]
    h = c = torch.zeros((L, 1, H), dtype=torch.float64)
    tok, rows = blank, []
    for u in range(len(tokens) + 1):
        st = R.step64(P, [tok] * n, h.expand(L, n, H), c.expand(L, n, H), enc_proj[:n])
        rows.append(st["logits"])                                                       # (n, V): every frame against the state after u tokens
        if u < len(tokens):
            tok, h, c = tokens[u], st["h_new"][:, :1], st["c_new"][:, :1]
    logits = torch.stack(rows, 1)[None]                                                 # (1, n, U + 1, V)
    lb, ll = rnnt_ref.lattice_logprobs(logits, torch.tensor([list(tokens) or [0]])[:, :len(tokens)], blank)
    return -float(rnnt_ref.costs_from_lattice(lb, ll, torch.tensor([n]), torch.tensor([len(tokens)]))[0])


@pytest.mark.parametrize("blank", [0, 2])
@pytest.mark.parametrize("T,max_len", [(1, 0), (1, 2), (2, 1), (3, 2)])
def test_unpruned_scores_are_the_rnnt_likelihood(T, max_len, blank):
    pr, jn = R.modules(3, 16, 16, 16, 16, 2, 900 + T, enc_dim=16)
    P = R.params64(pr, jn)
    enc_proj = torch.from_numpy(np.random.RandomState(T * 10 + max_len).standard_normal((T, 16)))
    res = BR.search64(P, enc_proj, T, 15, blank, max_symbols=max(max_len, 1), max_len=max_len)
    others = [k for k in range(3) if k != blank]
    strings = {()} | {(a,) for a in others if max_len >= 1} | {(a, b) for a in others for b in others if max_len >= 2}
    assert {s for s, _ in res["nbest"]} == strings                                      # nothing pruned: every string up to max_len finishes
    for s, score in res["nbest"]:
        assert abs(score - _lattice_ll(P, enc_proj, T, s, blank)) < 1e-9, (s, score)
    total = sum(np.exp(score) for _, score in res["nbest"])
    assert total < 1.0 + 1e-9 and (max_len < 2 or res["merges"] > 0 or T == 1)
    assert [x[1] for x in res["nbest"]] == sorted((x[1] for x in res["nbest"]), reverse=True)


def test_beam_1_is_the_greedy_search():
    cases = several = capped = 0
    for sharpen in (1.0, 10.0):
        pr, jn, h = BR.head("small", 0, sharpen)
        P = R.params64(pr, jn)
        for seed in range(12):
            rs = np.random.RandomState(700 + seed)
            n, max_symbols = int(rs.randint(1, 7)), (1, 2, 3)[seed % 3]
            enc_proj = torch.from_numpy(rs.standard_normal((n, h["J"]))) * 1.5
            want, _, _ = R.search64(P, enc_proj, n, 0, max_symbols, 0.0)
            got = BR.search64(P, enc_proj, n, 1, 0, max_symbols, max_len=n * max_symbols)
            assert len(got["nbest"]) == 1 and list(got["nbest"][0][0]) == want, (sharpen, seed, got["nbest"], want)
            cases += 1
            several += len(want) > n                                                    # more tokens than frames: a frame emitted several
            capped += len(want) == n * max_symbols                                      # every frame left because of the cap
    assert cases >= 20 and several >= 3 and capped >= 3, (cases, several, capped)


def test_the_merge_case_merges_and_is_clear():
    res, deltas = BR.reference(BR.MERGE_CASE)
    assert sum(r["merges"] for r in res) > 0
    assert all(BR.clear(r, d) for r, d in zip(res, deltas))


def test_most_gpu_cases_are_clear():
    flags = []
    for case in BR.GPU_CASES + [BR.MERGE_CASE]:
        res, deltas = BR.reference(case)
        flags += [BR.clear(r, d) for r, d in zip(res, deltas)]
        assert all(0.0 < d < 1e-2 for d in deltas), (case[0], max(deltas))
    print("clear (case, utterance) pairs: %d of %d" % (sum(flags), len(flags)))
    assert sum(flags) >= 0.8 * len(flags)


def test_no_frames_and_delta():
    pr, jn = R.modules(3, 16, 16, 16, 16, 2, 901, enc_dim=16)
    res = BR.search64(R.params64(pr, jn), torch.zeros((2, 16)), 0, 4)
    assert res["nbest"] == [((), 0.0)] and res["steps"] == 0
    assert BR.beam_delta(10, 50.0, 1e-5) == pytest.approx(2 * 10 * (2e-5 + 64 * 2.0 ** -23 + 4 * 2.0 ** -23 * 50.0))
