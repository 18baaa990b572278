"""CPU (no GPU): the float64 LSTM restatement of tests/lstm_ref.py against float64 torch.nn.LSTM + autograd, the LSTM entry points in the
header and the built library, and RNNPredictor(fused=True)'s parameters."""
import os

import numpy as np
import pytest
import torch

import lstm_ref


def lstm_case(B, U, I, H, L, seed, states=True):
    """(nn.LSTM in float64, x, h0, c0, dy, dhn, dcn): dy is zero on a ragged tail of positions per sequence, as a packed lattice leaves it."""
    g = torch.Generator().manual_seed(seed)
    rnn = torch.nn.LSTM(I, H, L, batch_first=True).double()
    with torch.no_grad():
        for p in rnn.parameters():
            p.copy_(torch.empty(p.shape, dtype=torch.float64).uniform_(-0.3, 0.3, generator=g))
    x = torch.randn(B, U, I, dtype=torch.float64, generator=g)
    h0 = torch.randn(L, B, H, dtype=torch.float64, generator=g) * 0.5 if states else None
    c0 = torch.randn(L, B, H, dtype=torch.float64, generator=g) * 0.5 if states else None
    dy = torch.randn(B, U, H, dtype=torch.float64, generator=g)
    for b in range(B):
        dy[b, U - (b * 3) % (U + 1) // 2:] = 0.0
    dhn, dcn = torch.randn(L, B, H, dtype=torch.float64, generator=g), torch.randn(L, B, H, dtype=torch.float64, generator=g)
    return rnn, x, h0, c0, dy, dhn, dcn


def layer_weights(rnn):
    return [tuple(getattr(rnn, n % l).detach() for n in ("weight_ih_l%d", "weight_hh_l%d", "bias_ih_l%d", "bias_hh_l%d")) for l in range(rnn.num_layers)]


def torch_lstm_grads(rnn, x, h0, c0, dy, dhn=None, dcn=None):
    """nn.LSTM forward + autograd in the module's dtype -> (y, hn, cn, dx, per-layer parameter gradients, dh0, dc0)."""
    rnn.zero_grad()
    x = x.clone().requires_grad_(True)
    B, L, H = x.shape[0], rnn.num_layers, rnn.hidden_size
    h0 = (torch.zeros(L, B, H, dtype=x.dtype) if h0 is None else h0.clone()).requires_grad_(True)
    c0 = (torch.zeros(L, B, H, dtype=x.dtype) if c0 is None else c0.clone()).requires_grad_(True)
    y, (hn, cn) = rnn(x, (h0, c0))
    loss = (y * dy).sum()
    if dhn is not None:
        loss = loss + (hn * dhn).sum() + (cn * dcn).sum()
    loss.backward()
    grads = [tuple(getattr(rnn, n % l).grad.clone() for n in ("weight_ih_l%d", "weight_hh_l%d", "bias_ih_l%d", "bias_hh_l%d")) for l in range(L)]
    return y.detach(), hn.detach(), cn.detach(), x.grad, grads, h0.grad, c0.grad


def flatten(res):
    y, hn, cn, dx, grads, dh0, dc0 = res
    return [("y", y), ("hn", hn), ("cn", cn), ("dx", dx), ("dh0", dh0), ("dc0", dc0)] + \
           [("%s_l%d" % (n, l), t) for l, gw in enumerate(grads) for n, t in zip(("dw_ih", "dw_hh", "db_ih", "db_hh"), gw)]


@pytest.mark.parametrize("shape", [(1, 1, 8, 8, 1), (3, 5, 8, 12, 2), (4, 6, 16, 8, 3)])
@pytest.mark.parametrize("states", [True, False])
def test_lstm_ref_equals_float64_nn_lstm(shape, states):
    B, U, I, H, L = shape
    rnn, x, h0, c0, dy, dhn, dcn = lstm_case(B, U, I, H, L, seed=sum(shape), states=states)
    want = flatten(torch_lstm_grads(rnn, x, h0, c0, dy, dhn, dcn))
    y, hn, cn, st = lstm_ref.forward(x, layer_weights(rnn), h0, c0)
    got = flatten((y, hn, cn) + lstm_ref.backward(st, dy, dhn, dcn))
    for (n, w), (_, g) in zip(want, got):
        assert float((w - g).abs().max()) <= 1e-12 * max(1.0, float(w.abs().max())), n


def test_keep_masks_have_the_requested_rate_and_unit_mean():
    m = lstm_ref.keep_masks(0.5, 1234, 3, 4, 7, 64)
    assert m[0] is None and len(m) == 3 and tuple(m[1].shape) == (4, 7, 64)
    for k in (1, 2):
        assert set(np.unique(m[k].numpy()).tolist()) == {0.0, 2.0}
        assert abs(float(m[k].mean()) - 1.0) < 0.1
    assert not torch.equal(m[1], m[2])
    assert torch.equal(m[1], lstm_ref.keep_masks(0.5, 1234, 3, 4, 7, 64)[1])
    assert lstm_ref.keep_masks(0.0, 1, 2, 1, 1, 64)[1] is None


def test_library_declares_and_exports_the_lstm_entries():
    import cfm
    if not os.path.exists(cfm.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    import test_abi_cpu
    names = test_abi_cpu.declared_functions()
    lib = cfm.lib()
    for n in ("cfm_lstm_forward", "cfm_lstm_backward", "cfm_lstm_save_floats"):
        assert n in names, "include/cfm.h does not declare %s" % n
        assert hasattr(lib, n), "libconformer_gfx950.so does not export %s" % n
    assert lib.cfm_lstm_save_floats(3, 5, 64) == 2 * 6 * 3 * 64 + 5 * 3 * 256
    assert lib.cfm_lstm_save_floats(3, 5, 64) % 4 == 0                               # a block after a block stays 16-byte aligned


def test_fused_predictor_has_the_stock_parameters():
    import predictor
    torch.manual_seed(3)
    a = predictor.RNNPredictor(50, 64, 40, 64, 0.1, 2, dropout=0.1)
    b = predictor.RNNPredictor(50, 64, 40, 64, 0.1, 2, dropout=0.1, fused=True)
    assert not a.fused and b.fused and isinstance(b.rnn, torch.nn.LSTM)
    assert list(a.state_dict().keys()) == list(b.state_dict().keys())
    assert {k: v.shape for k, v in a.state_dict().items()} == {k: v.shape for k, v in b.state_dict().items()}
    b.load_state_dict(a.state_dict())
    for k, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k]), k
    a.load_state_dict(b.state_dict())
    with pytest.raises(RuntimeError, match="no CPU path"):                            # the fused route is the library's: never the stock module quietly
        b(torch.zeros(2, 3, dtype=torch.long))
