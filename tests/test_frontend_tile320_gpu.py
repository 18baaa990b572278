"""The 320-row tile of the fused front-end (csrc/frontend.hip, FM = 10: A fragments read in two groups of five, the last four
production units split into channel halves over two wavefronts, the bias loaded after the K loop) against the 256-row tile on the
same inputs: BIT-IDENTICAL -- same MFMA operands, same K order per output element -- so no tolerance.  The shapes are the smallest
that reach a partial last tile, a batch boundary inside a tile, a single partial tile whose surplus production units clamp to the
last row, all four channel slabs per tap, and C = 512 (two N halves, the full 16 KB weight-fragment table: the instance that sits
exactly at the 160 KB LDS limit).  The host's tile choice is checked without a device through cfm_conv12_plan."""
import ctypes

import pytest
import torch

DEV = "cuda"


def _inputs(B, T, F, C, dtype, use_cmvn):
    g = torch.Generator().manual_seed(320 + B * 1000 + T + C)
    x = torch.randn((B, T, F), generator=g).to(DEV)
    w1 = (torch.randn((9, C), generator=g) * 0.3).to(DEV)
    b1 = (torch.randn((C,), generator=g) * 0.2).to(DEV)
    w2 = (torch.randn((C, 9 * C), generator=g) * (1.0 / (9 * C) ** 0.5)).to(DEV).to(dtype)
    b2 = (torch.randn((C,), generator=g) * 0.1).to(DEV)
    cmvn = None
    if use_cmvn:
        cmvn = (torch.randn((F,), generator=g).to(DEV), (torch.rand((F,), generator=g) + 0.5).to(DEV))
    return x, w1, b1, w2, b2, cmvn


# (B, T, F, C, CMVN mean + istd): M = B*T2*F2 rows
CASES = [
    (2, 67, 80, 64, False),     # 570 rows: 2 tiles, the second partial; the batch boundary at row 285 inside the first
    (2, 67, 80, 256, False),    # all four channel slabs per tap
    (2, 67, 80, 256, True),
    (1, 47, 27, 128, False),    # 50 rows: one partial tile, F2 = 5; production units past M clamp to the last row
    (3, 91, 80, 512, False),    # 1 197 rows: 4 tiles x 2 N halves, eight slabs
]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("case", CASES)
def test_tile320_equals_tile256(case, dtype):
    import cfm
    B, T, F, C, use_cmvn = case
    x, w1, b1, w2, b2, cmvn = _inputs(B, T, F, C, dtype, use_cmvn)
    L = cfm.lib()
    prev = L.cfm_set_conv12_tile(8)
    try:
        ref = cfm.conv12_relu(x, w1, b1, w2, b2, cmvn=cmvn)
        assert L.cfm_set_conv12_tile(10) == 8
        got = cfm.conv12_relu(x, w1, b1, w2, b2, cmvn=cmvn)
        torch.cuda.synchronize()
    finally:
        L.cfm_set_conv12_tile(prev)
    T2, F2 = ((T - 3) // 2 + 1 - 3) // 2 + 1, ((F - 3) // 2 + 1 - 3) // 2 + 1
    assert got.shape == ref.shape and got.dtype == ref.dtype == dtype and got.numel() == B * T2 * F2 * C
    assert float(ref.float().abs().max()) > 0.1 and float((ref != 0).float().mean()) > 0.2     # a live comparison, not zeros against zeros
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16)), (case, dtype, float((got.float() - ref.float()).abs().max()))


def _plan(M, C, cus):
    import cfm
    fm_main, fm_tail = ctypes.c_int32(-1), ctypes.c_int32(-1)
    cfm.check(cfm.lib().cfm_conv12_plan(M, C, cus, ctypes.byref(fm_main), ctypes.byref(fm_tail)), "cfm_conv12_plan")
    return fm_main.value, fm_tail.value


def test_plan_needs_no_device():
    """Config 2's 151 392 rows (2.31 rounds of 256-row tiles on 256 CUs, 1.85 of 320-row tiles) go out as one launch of 320-row tiles;
    a whole number of 256-row rounds stays on them; less than a round stays one round of small tiles."""
    assert _plan(32 * 249 * 19, 256, 256) == (10, 0)
    assert _plan(131072, 256, 256) == (8, 0)
    assert _plan(20000, 256, 256) == (0, 3)
    # C = 512 runs two workgroups per row tile: config 4's 75 696 rows on 128 tiles per round are the same 2.31 / 1.85 rounds
    assert _plan(16 * 249 * 19, 512, 256) == (10, 0)
    assert _plan(65536, 512, 256) == (8, 0)


def test_setter_keeps_unknown_tiles_out():
    import cfm
    L = cfm.lib()
    prev = L.cfm_set_conv12_tile(0)
    try:
        assert L.cfm_set_conv12_tile(7) == 0 and L.cfm_set_conv12_tile(10) == 0 and L.cfm_set_conv12_tile(0) == 10
    finally:
        L.cfm_set_conv12_tile(prev)
