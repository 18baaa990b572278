"""GPU: the four streaming-state ops of csrc/stream.hip (cfm_stream_prep, cfm_kv_ring_write, cfm_conv_cache_update, cfm_stream_advance) are one kernel
each, whose per-stream length pointer may be NULL.  NULL means whole windows: the same bits as lengths that say "whole window", on everything the op
writes.  Every comparison here is exact.

Shapes: 3 streams at offsets 0 (fresh), 5 (mid-ring) and 10 (its 4 new frames wrap past ring_T = 12), T = 4 new frames, need = 8 cached ones."""
import pytest
import torch

from test_ops_gpu import cfm, rnd  # noqa: F401  (cfm: the module fixture)

pytestmark = pytest.mark.gpu

B, H, DK, D, T, NEED, RING_T, MAX_LEN = 3, 2, 8, 16, 4, 8, 12, 32
OFFSETS = [0, 5, 10]


def i32(values):
    return torch.tensor(values, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("abs_rows", [False, True])
def test_prep_without_lengths_is_prep_of_whole_windows(cfm, abs_rows):
    pe = rnd((MAX_LEN, D), 1)
    got = []
    for frame_lens in (None, i32([4 * T + 3] * B)):                       # 4T+3 feature frames are T encoder frames
        sm = torch.randint(0, 256, (B, RING_T), dtype=torch.uint8, generator=torch.Generator().manual_seed(2)).cuda()
        pr, ar = rnd((B, RING_T, D), 3), rnd((B, D), 4) if abs_rows else None
        out_lens = None if frame_lens is None else i32([-1] * B)
        cfm.stream_prep(i32(OFFSETS), T, NEED, RING_T, pe, sm, pr, ar, frame_lens, out_lens)
        got.append((sm, pr, ar, out_lens))
    (sm0, pr0, ar0, _), (sm1, pr1, ar1, out_lens) = got
    assert out_lens.tolist() == [T] * B
    assert torch.equal(sm0, sm1) and torch.equal(pr0, pr1)
    assert sm0.sum().item() == sum(min(o, NEED) + T for o in OFFSETS)     # not vacuous: the cached frames and the T new ones of every stream
    if abs_rows:
        assert torch.equal(ar0, ar1) and torch.equal(ar0, pe[OFFSETS])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_ring_write_without_lengths_is_the_write_of_whole_windows(cfm, dtype):
    qkv = rnd((B, T, 3 * H * DK), 5).to(dtype)
    k, v = qkv[..., H * DK:2 * H * DK], qkv[..., 2 * H * DK:]
    ld = qkv.stride(1)
    offs, ring0 = i32(OFFSETS), rnd((B, H, RING_T, 2 * DK), 6)
    rings = []
    for lens in (None, i32([T] * B)):
        ring = ring0.clone()
        cfm.check(cfm.lib().cfm_kv_ring_write(k.data_ptr(), v.data_ptr(), cfm.dt_code(dtype), T * ld, ld, T * ld, ld, ring.data_ptr(), offs.data_ptr(), cfm.ptr(lens),
                                              B, H, T, DK, RING_T, cfm.stream()), "cfm_kv_ring_write")
        rings.append(ring)
    assert torch.equal(rings[0], rings[1])
    changed = (rings[0] != ring0).any(dim=-1).any(dim=1)                  # [B, ring_T]
    want = torch.zeros((B, RING_T), dtype=torch.bool, device="cuda")
    for b, off in enumerate(OFFSETS):
        for t in range(T):
            want[b, (off + t) % RING_T] = True
    assert torch.equal(changed, want)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("ktaps", [3, 15])                                # K-1 < T, and K-1 > T: the cache feeds itself
def test_cache_update_without_lengths_is_the_update_of_whole_windows(cfm, ktaps, dtype):
    x, cache0 = rnd((B, T, D), 7).to(dtype), rnd((B, ktaps - 1, D), 8)
    caches = []
    for lens in (None, i32([T] * B)):
        cache = cache0.clone()
        cfm.conv_cache_update(x, cache, ktaps, lens)
        caches.append(cache)
    assert torch.equal(caches[0], caches[1])
    assert torch.equal(caches[0], torch.cat([cache0, x.float()], 1)[:, -(ktaps - 1):])


def test_advance_without_lengths_is_the_advance_by_whole_windows(cfm):
    a, b = i32(OFFSETS), i32(OFFSETS)
    cfm.stream_advance(a, T)
    cfm.stream_advance(b, T, lens=i32([T] * B))
    assert torch.equal(a, b) and a.tolist() == [o + T for o in OFFSETS]


def test_advance_of_active_streams(cfm):
    offs = i32(OFFSETS)
    cfm.stream_advance(offs, T, torch.tensor([1, 0, 1], dtype=torch.uint8, device="cuda"))
    assert offs.tolist() == [OFFSETS[0] + T, OFFSETS[1], OFFSETS[2] + T]


def test_advance_by_lengths_zeroes_the_rows_behind_them(cfm):
    lens = [0, 2, T]
    offs = i32(OFFSETS)
    y = torch.full((B, T, D), float("nan"), device="cuda")
    cfm.stream_advance(offs, T, lens=i32(lens), y=y)
    assert offs.tolist() == [o + n for o, n in zip(OFFSETS, lens)]
    for b, n in enumerate(lens):
        assert bool(torch.isnan(y[b, :n]).all()), "rows below lens[%d] are untouched" % b
        assert torch.equal(y[b, n:], torch.zeros((T - n, D), device="cuda")), "rows at and past lens[%d] are exactly zero" % b


def test_advance_rejects_active_with_lengths(cfm):
    offs, active, lens = i32(OFFSETS), torch.ones(B, dtype=torch.uint8, device="cuda"), i32([T] * B)
    with pytest.raises(ValueError):
        cfm.stream_advance(offs, T, active, lens=lens)
    with pytest.raises(RuntimeError):                                     # the C entry point checks it too
        cfm.check(cfm.lib().cfm_stream_advance(offs.data_ptr(), active.data_ptr(), lens.data_ptr(), None, B, T, 0, cfm.stream()), "cfm_stream_advance")
    assert offs.tolist() == OFFSETS


@pytest.mark.parametrize("name", ["cfm_stream_prep_len", "cfm_kv_ring_write_len", "cfm_stream_advance_len", "cfm_conv_cache_update_len"])
def test_length_twins_are_gone(cfm, name):
    assert not hasattr(cfm.lib(), name)
