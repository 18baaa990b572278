"""GPU: cfm.packing.capture_step, the one "capture a streaming step in a HIP graph" protocol (encoder.StreamingSession, encoder.StreamingBatch and
the four searches of greedy.py), on a step small enough to read: cfm.stream_advance on the offsets of 3 streams plus an add into 8 floats.  And
the device branch of packing.stream_lens.  Every comparison is exact."""
import pytest
import torch

from cfm import packing
from test_ops_gpu import cfm  # noqa: F401  (cfm: the module fixture)

pytestmark = pytest.mark.gpu

T, OFFSETS, LENS = 4, [0, 5, 10], [2, 0, 4]


class Step:
    """offsets += lens (cfm_stream_advance), acc += sum(offsets); `seen` += sum(lens) and `runs` += 1 count what EVERY run() saw, warm-up included."""

    def __init__(self):
        dev = "cuda"
        self.offsets = torch.tensor(OFFSETS, dtype=torch.int32, device=dev)
        self.lens = torch.tensor(LENS, dtype=torch.int32, device=dev)
        self.acc = torch.arange(8, dtype=torch.float32, device=dev) * 0.25
        self.seen = torch.zeros((), dtype=torch.int64, device=dev)
        self.runs = torch.zeros((), dtype=torch.int64, device=dev)

    def run(self):
        import cfm as lib
        lib.stream_advance(self.offsets, T, lens=self.lens)
        self.acc.add_(self.offsets.sum().to(torch.float32))
        self.seen.add_(self.lens.sum())
        self.runs.add_(1)
        return self.acc


def test_state_is_put_back_and_replays_are_eager_runs(cfm):
    s, eager = Step(), Step()
    graph, out = packing.capture_step(s.run, torch.device("cuda"), [s.offsets, None, s.acc])  # None entries are skipped
    assert out is s.acc                                                   # what the CAPTURED run returned
    assert torch.equal(s.offsets, eager.offsets) and torch.equal(s.acc, eager.acc)           # the bits from before the call
    assert s.runs.item() == 1 and s.seen.item() == sum(LENS)              # one warm-up ran, on the real lengths; the capture executed nothing
    for n in range(1, 4):
        graph.replay()
        eager.run()
        assert torch.equal(s.offsets, eager.offsets) and torch.equal(s.acc, eager.acc), n
    assert s.offsets.tolist() == [o + 3 * n for o, n in zip(OFFSETS, LENS)]                    # not vacuous: the state did move


def test_idle_warm_up(cfm):
    s, eager = Step(), Step()
    graph, _ = packing.capture_step(s.run, torch.device("cuda"), [s.offsets, s.lens, s.acc], idle=s.lens.zero_)
    assert s.runs.item() == 1 and s.seen.item() == 0                      # the warm-up ran, and what it saw were the idled lengths
    assert s.lens.tolist() == LENS                                        # ... which are back, as the rest of the state is
    assert torch.equal(s.offsets, eager.offsets) and torch.equal(s.acc, eager.acc)
    graph.replay()
    eager.run()
    assert s.seen.item() == sum(LENS) and torch.equal(s.offsets, eager.offsets) and torch.equal(s.acc, eager.acc)


@pytest.mark.parametrize("strict", [True, False])
def test_device_lengths_are_clamped_on_the_device(cfm, strict):
    bound = 8
    value = torch.tensor([-1, 5, bound + 3], dtype=torch.int64, device="cuda")
    buf = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    assert packing.stream_lens("owner", "lens", 3, value, bound, None, strict=strict) is None and buf.tolist() == [-7] * 3
    assert packing.stream_lens("owner", "lens", 3, value, bound, buf, strict=strict) is None
    assert buf.dtype == torch.int32 and buf.tolist() == [0, 5, bound]
    assert value.tolist() == [-1, 5, bound + 3]
    with pytest.raises(ValueError, match="lens must hold 3 integers"):
        packing.stream_lens("owner", "lens", 3, value[:2], bound, buf, strict=strict)
    assert buf.tolist() == [0, 5, bound]
