"""CPU (no GPU): the packed RNN-T lattice layout (cfm/lattice.py) -- offsets and row map on hand-made ragged cases, a float64 packed restatement
of the loss built on tests/rnnt_ref.py against the padded one, the loud failures off the GPU, and the C ABI of the packed entry points."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import rnnt_ref

HDR = os.path.join(ROOT, "include", "cfm.h")
NEW_ENTRIES = ["cfm_rnnt_packed_nll", "cfm_rnnt_packed_grad", "cfm_joint_act_packed", "cfm_joint_act_packed_bwd"]


@pytest.fixture(scope="module")
def cfm():
    import cfm as c
    if not os.path.exists(c.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return c


def test_offsets_and_row_map_on_ragged_cases():
    from cfm import lattice
    T, U = [3, 1, 0, 2, 1], [2, 0, 4, 0, 3]                  # T_b = 1, T_b = 0 (no rows at all), U_b = 0
    off = lattice.offsets(T, U)
    assert off.dtype == np.int64 and off.tolist() == [0, 9, 10, 10, 12, 16]
    b, t, u = lattice.row_nodes(T, U)
    assert len(b) == off[-1]
    want = [(0, tt, uu) for tt in range(3) for uu in range(3)] + [(1, 0, 0)] + [(3, 0, 0), (3, 1, 0)] + [(4, 0, uu) for uu in range(4)]
    assert list(zip(b.tolist(), t.tolist(), u.tolist())) == want
    # row off[b] + t (U_b+1) + u is node (b, t, u)
    for r, (bb, tt, uu) in enumerate(want):
        assert off[bb] + tt * (U[bb] + 1) + uu == r
    # the activation backward's per-frame-block partials: ceil(T_b / 8) (U_b+1) rows per utterance
    assert lattice.block_offsets([9, 1, 0, 16], [2, 0, 5, 1]).tolist() == [0, 6, 7, 7, 11]
    assert lattice.offsets([0], [0]).tolist() == [0, 0]
    eb, et, eu = lattice.row_nodes([0], [3])
    assert len(eb) == len(et) == len(eu) == 0


def packed_ref(rows, targets, T, U, blank, clamp=-1):
    """float64 loss over packed logits rows [M, V]: per-utterance costs [B] and d cost_b / d rows [M, V] (clamped per utterance), each
    utterance's T_b (U_b+1) rows reshaped to its own lattice and run through rnnt_ref alone."""
    from cfm import lattice
    off = lattice.offsets(T, U)
    costs = torch.empty(len(T), dtype=torch.float64)
    grad = torch.zeros(rows.shape, dtype=torch.float64)
    for b in range(len(T)):
        if T[b] == 0:
            costs[b] = float("inf")
            continue
        lg = rows[off[b]:off[b + 1]].reshape(1, T[b], U[b] + 1, -1)
        c, g, _ = rnnt_ref.rnnt_loss_ref(lg, targets[b:b + 1, :U[b]], torch.tensor([T[b]]), torch.tensor([U[b]]), blank=blank, clamp=clamp, reduction="none")
        costs[b] = c[0]
        grad[off[b]:off[b + 1]] = g.reshape(-1, rows.shape[1])
    return costs, grad


def pack(padded, T, U):
    from cfm import lattice
    b, t, u = lattice.row_nodes(T, U)
    return padded[torch.from_numpy(b), torch.from_numpy(t), torch.from_numpy(u)]


@pytest.mark.parametrize("blank,clamp", [(0, -1), (-1, -1), (0, 0.05)])
def test_float64_packed_restatement_equals_the_padded_loss(blank, clamp):
    g = torch.Generator().manual_seed(11)
    B, Tp, Up, V = 5, 5, 3, 7
    logits = torch.randn((B, Tp, Up + 1, V), generator=g, dtype=torch.float64) * 2
    targets = torch.randint(0, V, (B, Up), generator=g, dtype=torch.int32)
    T, U = [5, 1, 3, 0, 4], [3, 2, 0, 1, 1]
    costs, grad, _ = rnnt_ref.rnnt_loss_ref(logits, targets, torch.tensor(T), torch.tensor(U), blank=blank, clamp=clamp, reduction="none")
    pc, pg = packed_ref(pack(logits, T, U), targets, T, U, blank, clamp)
    assert torch.isinf(pc[3]) and torch.isinf(costs[3])
    fin = torch.isfinite(costs)
    assert torch.allclose(pc[fin], costs[fin], rtol=1e-12, atol=0)
    assert torch.allclose(pg, pack(grad, T, U), rtol=0, atol=1e-12)
    # what the packed rows leave out is exactly the padded gradient's zeros
    assert float(grad.abs().sum()) == pytest.approx(float(pg.abs().sum()), rel=1e-12)


def test_packed_api_raises_off_the_gpu(cfm):
    import joint
    import rnnt
    T, U = torch.tensor([2, 1], dtype=torch.int32), torch.tensor([1, 0], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        rnnt.rnnt_loss_packed(torch.zeros(5, 4), torch.ones(2, 1, dtype=torch.int32), T, U)
    with pytest.raises(ValueError, match="reduction"):
        rnnt.rnnt_loss_packed(torch.zeros(5, 4), torch.ones(2, 1, dtype=torch.int32), T, U, reduction="average")
    j = joint.TransducerJoint(7, 16, 16, 32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        j.rnnt_loss(torch.randn(2, 3, 16), torch.randn(2, 2, 16), torch.ones(2, 1, dtype=torch.int32), T, U, packed=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        j.forward_window(torch.randn(6, 16), [(2, 3, T, torch.randn(2, 2, 16), torch.ones(2, 1, dtype=torch.int32), U)])


def _declared():
    text = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    return set(re.findall(r"\b(cfm_[a-z0-9_]+)\s*\(", text))


def test_header_declares_and_library_exports_the_packed_entries_at_abi_307(cfm):
    names = _declared()
    lib = cfm.lib()
    for n in NEW_ENTRIES:
        assert n in names, "include/cfm.h does not declare %s" % n
        assert hasattr(lib, n), "libconformer_gfx950.so does not export %s" % n
    assert lib.cfm_version() == 307
