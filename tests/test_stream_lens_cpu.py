"""CPU: the contract of cfm.packing.stream_lens -- the one reader of a streaming step's per-stream counts (StreamingBatch's frame_lens / host_lens,
the chunk decoders' lens, the streaming beam search's final flags) -- and of packing.stream_index, on CPU tensors as the buffer.  One table: what
ends up in the buffer, what the host is told, and the error text, under both settings of the strict / clamp flag.  The device-tensor branch
(clamped on the device, nothing returned) runs in tests/test_capture_step_gpu.py."""
import pytest
import torch

from cfm import packing

B, BOUND, STALE = 3, 8, -7
i32 = lambda v: torch.tensor(v, dtype=torch.int32)      # noqa: E731
i64 = lambda v: torch.tensor(v, dtype=torch.int64)      # noqa: E731

# (case, value, strict -> (buffer, returned host list) | the error's text, clamp -> the same)
TABLE = [
    ("None", None, ([8, 8, 8], [8, 8, 8]), ([8, 8, 8], [8, 8, 8])),
    ("list", [0, 5, 8], ([0, 5, 8], [0, 5, 8]), ([0, 5, 8], [0, 5, 8])),
    ("tuple of whole floats", (7.0, 0.0, 1.0), ([7, 0, 1], [7, 0, 1]), ([7, 0, 1], [7, 0, 1])),
    ("CPU int32 tensor", i32([8, 0, 3]), ([8, 0, 3], [8, 0, 3]), ([8, 0, 3], [8, 0, 3])),
    ("CPU int64 tensor", i64([1, 2, 3]), ([1, 2, 3], [1, 2, 3]), ([1, 2, 3], [1, 2, 3])),
    ("wrong count, list", [8, 8], r"owner: 2 lens for 3 streams", r"owner: 2 lens for 3 streams"),
    ("wrong count, tensor", i32([8, 8, 8, 8]), r"owner: lens must hold 3 integers, got torch\.int32 \(4,\)", r"owner: lens must hold 3 integers, got torch\.int32 \(4,\)"),
    ("negative", [4, -1, 0], r"owner: lens\[1\] = -1, outside 0 \.\. 8", ([4, 0, 0], [4, 0, 0])),
    ("negative, tensor", i64([-2, 4, 0]), r"owner: lens\[0\] = -2, outside 0 \.\. 8", ([0, 4, 0], [0, 4, 0])),
    ("above the bound", [4, 0, 9], r"owner: lens\[2\] = 9, outside 0 \.\. 8", ([4, 0, 8], [4, 0, 8])),
    ("above the bound, tensor", i32([11, 0, 8]), r"owner: lens\[0\] = 11, outside 0 \.\. 8", ([8, 0, 8], [8, 0, 8])),
    ("float value", [4, 2.5, 0], r"owner: lens\[1\] = 2\.5, outside 0 \.\. 8", ([4, 2, 0], [4, 2, 0])),
    ("float tensor", torch.tensor([4.0, 2.5, 9.5]), r"owner: lens must hold 3 integers, got torch\.float32 \(3,\)", ([4, 2, 8], [4, 2, 8])),
    ("2-d tensor", i64([[1], [2], [3]]), r"owner: lens must hold 3 integers, got torch\.int64 \(3, 1\)", ([1, 2, 3], [1, 2, 3])),
    ("booleans", [True, False, True], ([1, 0, 1], [1, 0, 1]), ([1, 0, 1], [1, 0, 1])),
]


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "clamp"])
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64, torch.uint8], ids=["i32", "i64", "u8"])
@pytest.mark.parametrize("case", TABLE, ids=[c[0] for c in TABLE])
def test_contract(case, dtype, strict):
    _, value, want_strict, want_clamp = case
    want = want_strict if strict else want_clamp
    buf = torch.full((B,), STALE if dtype != torch.uint8 else 77, dtype=dtype)
    before = buf.clone()
    if isinstance(want, str):
        for b in (buf, None):
            with pytest.raises(ValueError, match=want):
                packing.stream_lens("owner", "lens", B, value, BOUND, b, strict=strict)
        assert torch.equal(buf, before), "a refused value leaves the buffer as it was"
        return
    assert packing.stream_lens("owner", "lens", B, value, BOUND, None, strict=strict) == want[1]
    assert torch.equal(buf, before), "without a buffer the value is only checked"
    got = packing.stream_lens("owner", "lens", B, value, BOUND, buf, strict=strict)
    assert got == want[1] and all(type(n) is int for n in got)
    assert buf.dtype == dtype and buf.tolist() == want[0]


@pytest.mark.parametrize("strict", [True, False])
def test_default_for_none(strict):
    buf = torch.full((B,), 5, dtype=torch.uint8)
    assert packing.stream_lens("owner", "final flags", B, None, 1, buf, default=0, strict=strict) == [0, 0, 0]
    assert buf.tolist() == [0, 0, 0]
    assert packing.stream_lens("owner", "final flags", B, [2, 0, True], 1, buf, default=0, strict=False) == [1, 0, 1] and buf.tolist() == [1, 0, 1]


def test_stream_index():
    state = torch.arange(12).reshape(4, 3)
    assert packing.stream_index(None, "cpu") == slice(None)
    idx = packing.stream_index((b for b in (2, 0)), "cpu")                # any iterable, read once
    assert idx.dtype == torch.long and idx.tolist() == [2, 0]
    state[idx] = 0
    assert state.tolist() == [[0, 0, 0], [3, 4, 5], [0, 0, 0], [9, 10, 11]]
    state[packing.stream_index(None, "cpu")] = -1
    assert bool((state == -1).all())
    assert packing.stream_index([], "cpu").numel() == 0
