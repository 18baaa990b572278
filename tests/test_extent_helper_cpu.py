"""CPU: the guard-band helper (tests/extent.py) flags the three kinds of subtly wrong kernel and passes a correct one.

The "kernels" are stand-ins written in torch on CPU tensors: a row-strided product out[M,N] = a[M,K] . w[N,K]^T that reaches its operands
the way a HIP kernel does -- through a base pointer and a row stride (as_strided over the placed view's storage), so it CAN run over an edge."""
import pytest
import torch

import extent

M, N, K, LDA, LDC = 5, 6, 8, 12, 10


def _operands():
    g = torch.Generator().manual_seed(5)
    a, w = torch.randn((M, K), generator=g), torch.randn((N, K), generator=g)
    G = extent.Guards("cpu")
    av, wv, ov = G.inp(a, ld=LDA, name="a"), G.inp(w, name="w"), G.out((M, N), torch.float32, ld=LDC, name="out")
    return G, a, w, av, wv, ov


def _raw(view, rows, cols, shift=0):
    """what a kernel sees: `rows` x `cols` elements from the view's base (+ shift elements) at the view's row stride"""
    return view.as_strided((rows, cols), (view.stride(0), 1), view.storage_offset() + shift)


def _verdict(G, ov, ref):
    """the per-case rule of tests/test_extents_gpu.py: (a) the extent matches the reference, (b) every band and gap is untouched"""
    err = float((ov.double() - ref.double()).abs().max())
    assert err < 1e-5, "extent differs from the reference (max |d| = %r)" % err      # NaN fails: an unwritten or poisoned element
    G.check()


def test_correct_kernel_passes():
    G, a, w, av, wv, ov = _operands()
    assert av.stride() == (LDA, 1) and ov.stride() == (LDC, 1) and torch.equal(av, a) and bool(torch.isnan(ov).all())
    ov.copy_(av @ wv.t())
    _verdict(G, ov, a @ w.t())


def test_layout_of_bands():
    for dt, es in ((torch.float32, 4), (torch.bfloat16, 2), (torch.uint8, 1), (torch.int32, 4)):
        t = torch.ones((3, 7), dtype=dt)
        for role in ("input", "inout", "output"):
            v, h = extent.place(t, ld=9, role=role)
            assert h.lead % 256 == 0 and h.flat.numel() % 256 == 0 and h.lead >= max(64 * 1024, 256 * 9 * es)
            assert h.flat.numel() - h.lead - 3 * 9 * es >= max(64 * 1024, 256 * 9 * es)       # never flush against the end
            assert v.data_ptr() == h.flat.data_ptr() + h.lead and v.stride() == (9, 1)
            gap = _raw(v, 3, 9)[:, 7:]
            if role == "input":
                assert torch.equal(v, t)
                assert bool(torch.isnan(gap).all()) if dt.is_floating_point else bool((gap == (1 if dt == torch.uint8 else 0)).all())
            else:
                assert bool((h.flat[h.lead - 64:h.lead] == 0xA5).all()) and bool((h.flat[-64:] == 0xA5).all())
                if role == "output":
                    assert bool(torch.isnan(v).all()) if dt.is_floating_point else bool((v == (0xFF if dt == torch.uint8 else -1)).all())
            h.check()
    v, h = extent.workspace(37, torch.float32, "cpu")
    assert v.shape == (37,) and v.is_contiguous()
    v.zero_()
    h.check()
    _raw(v.view(1, 37), 1, 38)[0, 37] = 0.0                                                    # one float past a workspace's documented size
    with pytest.raises(AssertionError, match="trail band"):
        h.check()
    v3, h3 = extent.place(torch.zeros((2, 3, 4)), ld=6)
    assert v3.shape == (2, 3, 4) and v3.stride() == (18, 6, 1)


@pytest.mark.parametrize("where", ["past_last_row", "gap_column", "before_base"])
def test_stray_store_is_flagged(where):
    G, a, w, av, wv, ov = _operands()
    ov.copy_(av @ wv.t())
    if where == "past_last_row":
        _raw(ov, M + 1, N)[M, 0] = 1.0
        hit = "row %d, column 0" % M
    elif where == "gap_column":
        _raw(ov, M, N + 1)[2, N] = 1.0
        hit = "gap at row 2, column %d" % N
    else:
        _raw(ov, 1, 1, shift=-1)[0, 0] = 1.0
        hit = "lead band at row -1, column %d" % (LDC - 1)
    with pytest.raises(AssertionError, match=hit):
        _verdict(G, ov, a @ w.t())


def test_store_into_an_input_is_flagged():
    G, a, w, av, wv, ov = _operands()
    ov.copy_(av @ wv.t())
    av[1, 2] += 1.0
    with pytest.raises(AssertionError, match=r"a \(input\).*extent at row 1, column 2"):
        G.check()


@pytest.mark.parametrize("what", ["gap_of_a", "row_past_w"])
def test_nan_leak_through_a_zero_weight_is_flagged(what):
    """A tail lane that reads one column / one row too far and folds it in with a zero weight: finite garbage would pass, NaN does not."""
    G, a, w, av, wv, ov = _operands()
    if what == "gap_of_a":
        a_far = _raw(av, M, K + 1)                              # column K of a: a gap
        w_pad = torch.cat([wv, torch.zeros(N, 1)], 1)           # "K tail chunk loads zeros" on one side only
        ov.copy_(a_far @ w_pad.t())
    else:
        w_far = _raw(wv, N + 1, K)                              # row N of w: the trail band
        acc = av @ w_far.t()
        ov.copy_(acc[:, :N] + 0.0 * acc[:, N:])                 # the extra column is multiplied away, not selected away
    with pytest.raises(AssertionError, match="differs from the reference"):
        _verdict(G, ov, a @ w.t())


def test_mask_over_read_admits_a_poisoned_row():
    G = extent.Guards("cpu")
    x = G.inp(torch.ones(4, 3), name="x")
    m = G.inp(torch.tensor([1, 0, 1, 1], dtype=torch.uint8), name="mask")
    rows = _raw(x, 5, 3) * _raw(m.view(1, 4), 1, 5)[0].bool()[:, None]        # reads mask[4] (band: 1 = valid) and row 4 (NaN)
    assert not bool(torch.isfinite(rows.sum()))
    G.check()


def test_unwritten_owned_element_is_flagged():
    G, a, w, av, wv, ov = _operands()
    ref = a @ w.t()
    keep = torch.ones(M, N, dtype=torch.bool)
    keep[M - 1, N - 1] = False                                  # the last pair of the last row is never stored
    ov[keep] = ref[keep]
    with pytest.raises(AssertionError, match="differs from the reference"):
        _verdict(G, ov, ref)
    G.check()                                                   # ... though no band was touched
    iv, ih = extent.out((3,), torch.int32, "cpu")
    assert bool((iv == -1).all())
