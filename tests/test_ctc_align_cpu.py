"""CPU: the float64 statement of CTC forced alignment (tests/ctc_align_ref.py) against brute force, its tie rule, its infeasible cases, and the
classification of the case table that test_ctc_align_gpu.py runs (which cases an f32 evaluation must reproduce path for path)."""
import itertools

import numpy as np
import pytest
import torch

import ctc_align_ref as ref

NEG = float("-inf")


def test_definition_equals_brute_force():
    V, n_paths = 3, 0
    label_sets = [list(l) for U in range(4) for l in itertools.product((1, 2), repeat=U)]
    assert len(label_sets) == 15 and [1, 1, 1] in label_sets
    for n in range(1, 7):
        for k, labels in enumerate(label_sets):
            g = torch.Generator().manual_seed(100 * n + k)
            lp = ref.log_probs(2.0 * torch.randn((n, V), generator=g), V)
            res = ref.align64(lp, labels)
            score, path = ref.brute_force(lp, labels)
            what = (n, labels)
            if path is None:
                assert n < len(labels) + ref.repeats(labels) and res["score"] == NEG and not res["feasible"], what
                assert (res["path"] == -1).all() and (res["start"] == -1).all() and (res["end"] == -1).all() and (res["token_logp"] == NEG).all(), what
                continue
            assert n >= len(labels) + ref.repeats(labels) and abs(res["score"] - score) <= 1e-12, what
            assert abs(ref.path_score(res["path"], lp, ref.extended(labels, V)) - score) <= 1e-12, what
            if min(ref.decision_gap(res)) > 1e-9:
                assert tuple(res["path"].tolist()) == path, what
                n_paths += 1
            z = ref.extended(labels, V)
            for u in range(len(labels)):
                frames = [t for t in range(n) if res["path"][t] == 2 * u + 1]
                assert frames == list(range(res["start"][u], res["end"][u] + 1)) and frames, what
                assert abs(res["token_logp"][u] - sum(lp[t, z[2 * u + 1]] for t in frames)) <= 1e-12, what
    assert n_paths > 40


def test_tie_rule_on_constant_logits():
    # len 5, labels [1, 1], states (0, 1, 2, 3, 4) = (blank, 1, blank, 1, blank), every log-probability equal, so every alignment scores the same.
    # Final state: S-2 = 3 (a tie keeps the last label).  Walking back, each frame prefers stay, then s-1 (s-2 is barred between equal labels): state 3
    # stays for as long as the earlier frames can still reach it -- delta_t[3] is finite from t = 2 on (1 -> 2 -> 3), so frames 4, 3, 2 are state 3;
    # at t = 2 state 3 cannot stay (delta_1[3] = -inf) and takes s-1 = 2; delta_1[2] comes from state 1 only (delta_0[2] = -inf); frame 0 is state 1.
    lp = ref.log_probs(torch.zeros((5, 3)), 3)
    res = ref.align64(lp, [1, 1])
    assert res["path"].tolist() == [1, 2, 3, 3, 3]
    assert res["start"].tolist() == [0, 2] and res["end"].tolist() == [0, 4]
    assert abs(res["score"] - 5 * np.log(1.0 / 3.0)) <= 1e-12
    # len 4, U = 0: the single state 0 throughout
    res = ref.align64(ref.log_probs(torch.zeros((4, 3)), 3), [])
    assert res["path"].tolist() == [0, 0, 0, 0] and abs(res["score"] - 4 * np.log(1.0 / 3.0)) <= 1e-12
    # labels [1, 2], len 4: final state 3, which stays while it can -- frames 3, 2, 1, since delta_1[3] is finite through the skip: at t = 1 its stay
    # and s-1 candidates (delta_0[3], delta_0[2]) are -inf and s-2 = state 1 is the only finite one; frame 0 is state 1.
    res = ref.align64(ref.log_probs(torch.zeros((4, 3)), 3), [1, 2])
    assert res["path"].tolist() == [1, 3, 3, 3]


def test_infeasible_cases():
    lp = ref.log_probs(torch.zeros((2, 3)), 3)
    res = ref.align64(lp, [1, 1])                             # two equal labels need three frames
    assert res["score"] == NEG and res["path"].tolist() == [-1, -1] and res["start"].tolist() == [-1, -1] and res["end"].tolist() == [-1, -1]
    assert (res["token_logp"] == NEG).all() and not res["feasible"]
    res = ref.align64(lp[:0], [1], 0)                         # no frame, one label
    assert res["score"] == NEG and res["path"].tolist() == [] and res["start"].tolist() == [-1] and (res["token_logp"] == NEG).all()
    res = ref.align64(lp[:0], [], 0)                          # no frame, no label: the empty alignment, probability 1
    assert res["score"] == 0.0 and res["feasible"] and res["path"].tolist() == []


def test_labels_are_clamped_and_padding_ignored():
    g = torch.Generator().manual_seed(5)
    lp = ref.log_probs(torch.randn((9, 5), generator=g), 5)
    a, b = ref.align64(lp, [1, 9, -3, 1]), ref.align64(lp, [1, 4, 0, 1])
    assert a["score"] == b["score"] and a["path"].tolist() == b["path"].tolist()


def test_plant_gives_valid_alignments():
    for seed, (labels, T) in enumerate([([1, 1, 2], 4), ([1, 2], 2), ([], 3), ([1, 1, 1], 9), ([2, 1, 2, 2], 30)]):
        path = ref.plant(labels, T, seed)
        assert len(path) == T and ref.valid_path(path, ref.extended(labels, 3)), (labels, T, path)


@pytest.mark.parametrize("V", [3, 17, 5002])
def test_case_table_is_classified(V):
    """Named edge cases are exact (every decision on the optimal path further than delta from flipping) or constant-logit tie cases; at least two
    thirds of the seeded random cases are exact."""
    n_random = n_exact = 0
    for case in ref.cases(V):
        name, kind, T, lens, labels, Umax = case[:6]
        _, res = ref.case_reference(V, case)
        ex = [ref.exact(r, max(n, 1)) for r, n in zip(res, lens)]
        if kind == "edge":
            assert all(ex), (V, name, [ref.decision_gap(r) for r in res], [ref.delta(max(n, 1), r["score"]) for r, n in zip(res, lens)])
        elif kind == "tie":
            x = ref.case_logits(V, case)
            assert bool((x == ref.TIE_LOGIT).all())            # constant: every frame's shifted log-probabilities are exactly 0 in f32 and f64
            assert all(r["feasible"] for r in res)
        else:
            n_random += len(ex)
            n_exact += sum(ex)
    assert n_random >= 30 and 3 * n_exact >= 2 * n_random, (V, n_exact, n_random)
    feas = {c[0]: [r["feasible"] for r in ref.case_reference(V, c)[1]] for c in ref.cases(V)}
    assert feas["T==U"] == [True] and feas["T==U+repeats"] == [True] and feas["T==U+repeats-1"] == [False] and feas["ragged"] == [True, True, True]
