"""CPU: the float64 statement of RNN-T forced alignment (tests/rnnt_align_ref.py) against brute force and against the loss's float64 statement,
and the conditions on the case table that the GPU test (test_rnnt_align_gpu.py) relies on.  No GPU, nothing of the package."""
import numpy as np
import pytest
import torch

import rnnt_align_ref as ref
import rnnt_ref

VS = (3, 17, 5002)


def tiny(seed, T, U1, V=3):
    g = torch.Generator().manual_seed(seed)
    logits = 2.0 * torch.randn((1, T, U1, V), generator=g)
    targets = torch.randint(0, V - 1, (1, U1 - 1), generator=g).to(torch.int32)
    lb, ll = ref.node_logprobs(logits, targets, V - 1, V)
    return logits, targets, lb[0], ll[0]


def test_recursion_equals_brute_force_on_every_tiny_lattice():
    n_unique = 0
    for Tb in range(0, 6):
        for Ub in range(0, 5):
            for seed in range(3):
                _, _, lb, ll = tiny(100 * Tb + 10 * Ub + seed, 5, 5)
                res = ref.align64(lb, ll, Tb, Ub)
                best, frames, unique = ref.brute_force(lb, ll, Tb, Ub)
                if Tb == 0:
                    assert res["score"] == ref.NEG and not res["feasible"] and res["frames"].tolist() == [-1] * Ub
                    continue
                assert abs(res["score"] - best) <= 1e-12 * max(1.0, abs(best)), (Tb, Ub, seed)
                if unique:
                    n_unique += 1
                    assert tuple(res["frames"].tolist()) == frames, (Tb, Ub, seed)
    assert n_unique > 50


def test_tie_rule_sends_every_label_to_frame_0():
    for T, U in ((1, 2), (4, 3), (7, 1), (5, 0)):
        lb, ll = ref.node_logprobs(torch.full((1, T, U + 1, 5), ref.TIE_LOGIT), torch.ones((1, U), dtype=torch.int32), 0, 5)
        res = ref.align64(lb[0], ll[0], T, U)
        assert res["frames"].tolist() == [0] * U
        assert abs(res["score"] + (T + U) * np.log(5.0)) < 1e-12


def test_path_score_round_trip_and_invalid_lists():
    _, _, lb, ll = tiny(7, 5, 4)
    res = ref.align64(lb, ll, 5, 3)
    assert abs(ref.path_score(res["frames"], lb[:5, :4], ll[:5, :4]) - res["score"]) <= 1e-12 * abs(res["score"])
    assert ref.path_score([2, 1, 3], lb, ll) == ref.NEG and ref.path_score([0, 1, 5], lb, ll) == ref.NEG and ref.path_score([-1, 1, 2], lb, ll) == ref.NEG
    assert ref.path_score([], lb[:0], ll[:0]) == ref.NEG
    assert abs(ref.path_score([], lb[:5, :1], ll[:5, :1]) - lb[:5, 0].sum()) < 1e-12


@pytest.mark.parametrize("V", VS)
def test_case_table(V):
    """Per case of cases(V): the round trip, score <= -cost of the loss's float64 statement, the tie cases' frames, and an f32 evaluation of the same
    recursion (f32 log_softmax, f32 sums, unshifted) within delta of the float64 score with a valid path whose float64 score is within delta of the
    optimum.  Then the condition the GPU test's "identical frames" clause needs: at least three quarters of the non-tie utterances are `exact`."""
    n_exact = n_live = 0
    for case in ref.cases(V):
        logits, targets, res = ref.case_reference(V, case)
        lb, ll = rnnt_ref.lattice_logprobs(logits, targets, case.blank)
        cost = rnnt_ref.costs_from_lattice(lb, ll, torch.tensor(case.logit_lens), torch.tensor(case.target_lens))
        lb32, ll32 = torch.log_softmax(logits, -1)[..., case.blank].numpy(), None
        lp32 = torch.log_softmax(logits, -1)
        for b, r in enumerate(res):
            what = (V, case.name, b)
            if not r["feasible"]:
                assert r["Tb"] == 0 and r["score"] == ref.NEG and float(cost[b]) == float("inf"), what
                continue
            Tb, Ub = r["Tb"], r["Ub"]
            d = ref.delta(Tb, Ub, r["score"], r["lmax"])
            assert abs(ref.path_score(r["frames"], r["lb"], r["ll"]) - r["score"]) <= 1e-9 * max(1.0, abs(r["score"])), what
            assert r["score"] <= -float(cost[b]) + 1e-9 * max(1.0, abs(r["score"])), what
            assert all(a <= c for a, c in zip(r["frames"][:-1], r["frames"][1:])) and all(0 <= f < Tb for f in r["frames"]), what
            if case.kind == "tie":
                assert r["frames"].tolist() == [0] * Ub, what
                continue
            if case.kind == "peaked":
                assert abs(r["score"] + float(cost[b])) < 1e-6, what
            y = targets[b, :Ub].long().clamp(0, V - 1)
            ll32 = lp32[b, :Tb, :Ub + 1].gather(2, torch.cat([y, y.new_zeros(1)])[None, :, None].expand(Tb, Ub + 1, 1)).squeeze(2).numpy()
            r32 = ref.align64(lb32[b], ll32, Tb, Ub, dtype=np.float32)
            own = ref.path_score(r32["frames"], r["lb"], r["ll"])
            assert abs(r32["score"] - r["score"]) <= d and own > ref.NEG and abs(own - r["score"]) <= d, (what, r32["score"], r["score"], own, d)
            n_live += 1
            if ref.exact(r):
                n_exact += 1
                assert r32["frames"].tolist() == r["frames"].tolist(), what
    assert n_live >= 30 and 4 * n_exact >= 3 * n_live, (V, n_exact, n_live)
