"""CPU (no GPU): the float64 RNN-T reference against brute-force enumeration of alignments, the loud failures of rnnt.rnnt_loss /
TransducerJoint.rnnt_loss off the GPU, and the C ABI of the RNN-T entry points (declared, exported)."""
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import rnnt_ref

HDR = os.path.join(ROOT, "include", "cfm.h")
NEW_ENTRIES = ["cfm_rnnt_nll", "cfm_rnnt_grad", "cfm_joint_act_bwd", "cfm_joint_act_bwd_ws"]


@pytest.fixture(scope="module")
def cfm():
    import cfm as c
    if not os.path.exists(c.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return c


def _case(seed, B, T, U, V):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn((B, T, U + 1, V), generator=g, dtype=torch.float64) * 2
    targets = torch.randint(0, V, (B, max(U, 0)), generator=g, dtype=torch.int32)
    return logits, targets


@pytest.mark.parametrize("T,U,V", [(1, 0, 3), (1, 2, 4), (2, 1, 3), (3, 3, 5), (4, 2, 5), (4, 3, 4), (4, 0, 2)])
@pytest.mark.parametrize("blank", [0, -1])
def test_reference_dp_equals_brute_force(T, U, V, blank):
    B = 3
    logits, targets = _case(100 * T + 10 * U + V, B, T, U, V)
    logit_lengths = torch.tensor([T, max(T - 1, 1), 1], dtype=torch.int32)
    target_lengths = torch.tensor([U, 0, max(U - 1, 0)], dtype=torch.int32)
    b = blank + V if blank < 0 else blank
    _, _, costs = rnnt_ref.rnnt_loss_ref(logits, targets, logit_lengths, target_lengths, blank=blank, reduction="none")
    for i in range(B):
        want = rnnt_ref.brute_force_cost(logits[i], targets[i], int(logit_lengths[i]), int(target_lengths[i]), b)
        assert abs(float(costs[i]) - want) <= 1e-10 * max(1.0, abs(want)), (i, float(costs[i]), want)


def test_reference_reductions_clamp_and_zero_gradient_outside_the_lattice():
    logits, targets = _case(7, 3, 4, 3, 5)
    tl, ul = torch.tensor([4, 2, 3], dtype=torch.int32), torch.tensor([3, 1, 0], dtype=torch.int32)
    none, g_none, costs = rnnt_ref.rnnt_loss_ref(logits, targets, tl, ul, blank=0, reduction="none")
    s, g_sum, _ = rnnt_ref.rnnt_loss_ref(logits, targets, tl, ul, blank=0, reduction="sum")
    m, g_mean, _ = rnnt_ref.rnnt_loss_ref(logits, targets, tl, ul, blank=0, reduction="mean")
    assert torch.allclose(s, costs.sum()) and torch.allclose(m, costs.mean())
    assert torch.allclose(g_none, g_sum) and torch.allclose(g_mean, g_sum / 3)
    assert float(g_sum[1, 2:].abs().max()) == 0.0 and float(g_sum[1, :, 2:].abs().max()) == 0.0 and float(g_sum[2, :, 1:].abs().max()) == 0.0
    # every valid node's gradient sums to zero over the vocabulary (softmax minus the node's outgoing occupancy)
    assert float(g_sum.sum(-1).abs().max()) < 1e-12
    _, g_cl, _ = rnnt_ref.rnnt_loss_ref(logits, targets, tl, ul, blank=0, clamp=0.05, reduction="sum")
    assert float(g_cl.abs().max()) <= 0.05 and torch.equal(g_cl, g_sum.clamp(-0.05, 0.05))


def test_reference_gradient_matches_finite_differences():
    logits, targets = _case(3, 1, 3, 2, 4)
    tl, ul = torch.tensor([3], dtype=torch.int32), torch.tensor([2], dtype=torch.int32)
    _, g, _ = rnnt_ref.rnnt_loss_ref(logits, targets, tl, ul, blank=0, reduction="sum")
    for idx in [(0, 0, 0, 0), (0, 1, 1, 2), (0, 2, 2, 0), (0, 2, 1, 3)]:
        h = 1e-6
        lp, lm = logits.clone(), logits.clone()
        lp[idx] += h
        lm[idx] -= h
        fd = (rnnt_ref.rnnt_loss_ref(lp, targets, tl, ul, 0, reduction="sum")[0] - rnnt_ref.rnnt_loss_ref(lm, targets, tl, ul, 0, reduction="sum")[0]) / (2 * h)
        assert abs(float(fd) - float(g[idx])) < 1e-7, (idx, float(fd), float(g[idx]))


def test_rnnt_loss_raises_off_the_gpu_and_on_bad_arguments(cfm):
    import rnnt
    logits, targets = _case(1, 2, 3, 2, 5)
    lens, tlens = torch.tensor([3, 2], dtype=torch.int32), torch.tensor([2, 1], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        rnnt.rnnt_loss(logits.float(), targets, lens, tlens)
    with pytest.raises(ValueError, match="reduction"):
        rnnt.rnnt_loss(logits.float(), targets, lens, tlens, reduction="average")
    with pytest.raises(NotImplementedError):
        rnnt.rnnt_loss(logits.float(), targets, lens, tlens, fused_log_softmax=False)
    import joint
    j = joint.TransducerJoint(7, 16, 16, 32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        j.rnnt_loss(torch.randn(2, 3, 16), torch.randn(2, 3, 16), targets, lens, tlens)


def _declared():
    text = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    return set(re.findall(r"\b(cfm_[a-z0-9_]+)\s*\(", text))


def test_header_declares_and_library_exports_the_rnnt_entries(cfm):
    names = _declared()
    lib = cfm.lib()
    for n in NEW_ENTRIES:
        assert n in names, "include/cfm.h does not declare %s" % n
        assert hasattr(lib, n), "libconformer_gfx950.so does not export %s" % n
    assert lib.cfm_joint_act_bwd_ws(2, 9, 4, 16) == 2 * 2 * 4 * 16          # two frame blocks of 8
