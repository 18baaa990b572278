"""CPU (no GPU, no library): the argument checker of cfm/ops.py -- its layout / dtype / extent part is a pure function of tensor metadata -- and
the host-packet check fbank.PacketSchedule and resample.StreamingResampler share (cfm.packing.host_packets)."""
import types

import pytest
import torch

I32, F32 = torch.int32, torch.float32


def refused(ops, match, **specs):
    with pytest.raises(ValueError, match=match) as e:
        ops._layout("some_op", **specs)
    msg = str(e.value)
    assert msg.startswith("cfm.some_op: ") and "no stride for it" in msg
    return msg


def test_layout_accepts_what_it_states():
    from cfm import ops
    lens = torch.zeros(4, dtype=I32)
    ops._layout("some_op", lens=(lens, I32, 4), col=(lens.view(4, 1), I32, 4), grid=(torch.zeros(4, 3, 2), F32, (4, None, 2)), anything=(torch.zeros(2, 2).bool(), None, None),
                either=(torch.zeros(3, dtype=torch.int16), (torch.int16, F32), (3,)), absent=ops._opt(None, I32, 4), given=ops._opt(lens, I32, (4,)), empty=(torch.zeros(0, 5), F32, 0))
    assert ops._opt(None, I32, 4) is None and ops._opt(lens, I32, 4) == (lens, I32, 4)
    assert ops._i32(4, a=lens, b=None) == {"a": (lens, I32, 4), "b": (None, I32, 4)}


def test_layout_refusals_name_op_argument_want_and_got():
    from cfm import ops
    lens, wide = torch.zeros(4, dtype=torch.int64), torch.zeros(4, 6)
    msg = refused(ops, r"lens must be contiguous int32 of 4 elements .*got int64 \(4,\) strides \(1,\)", lens=(lens, I32, 4))        # wrong dtype
    assert "some_op" in msg and "lens" in msg
    refused(ops, r"x must be contiguous float32 \[4, 3\].*got float32 \(4, 3\) strides \(6, 2\)", x=(wide[:, ::2], F32, (4, 3)))          # a strided view
    refused(ops, r"x must be contiguous.*got float32 \(4, 3\) strides \(6, 2\)", x=(wide[:, ::2], None, None))                             # ... with nothing else asked
    refused(ops, r"lens must be contiguous int32 of 5 elements.*got int32 \(4,\)", lens=(lens.int(), I32, 5))                            # wrong element count
    refused(ops, r"lens must be contiguous int32 \[4\].*got int32 \(4, 1\)", lens=(lens.int().view(4, 1), I32, (4,)))                     # wrong exact shape: [B,1] is not [B]
    refused(ops, r"x must be contiguous float32 \[4, \*\].*got float32 \(6, 4\)", x=(wide.t().contiguous(), F32, (4, None)))               # a free axis fixes the rank and the rest
    refused(ops, r"x must be contiguous float32 \[4, \*\].*got float32 \(4,\)", x=(torch.zeros(4), F32, (4, None)))
    refused(ops, r"x must be contiguous int16 or float32.*got float64 \(2,\)", x=(torch.zeros(2, dtype=torch.float64), (torch.int16, F32), None))
    refused(ops, r"lens must be contiguous int32 of 4 elements.*got None", lens=(None, I32, 4))                                          # a required argument that is missing
    refused(ops, r"got None", **ops._i32(4, lens=None))
    refused(ops, r"got int64 \(4,\) strides \(1,\): batch sizes differ$", _hint="batch sizes differ", lens=(lens, I32, 4))
    ops._layout("some_op", lens=(lens.int().view(4, 1), I32, 4))                                                                        # [B,1] passes where a count is asked
    with pytest.raises(ValueError, match="b must be"):                                                                                 # the first offender in argument order
        ops._layout("some_op", a=(lens, torch.int64, 4), b=(lens, I32, 4), c=(lens, F32, 4))


def test_want_puts_the_device_first():
    from cfm import ops
    with pytest.raises(RuntimeError, match="no CPU path"):                                    # a CPU tensor is cfm.require_hip's error, whatever its layout
        ops._want("some_op", lens=(torch.zeros(4, 2)[:, 0], I32, 7))
    ops._want("some_op", lens=ops._opt(None, I32, 7))
    with pytest.raises(ValueError, match="got None"):
        ops._want("some_op", lens=(None, I32, 7))


def owners():
    import fbank
    import resample
    sched = fbank.PacketSchedule(3, 2, 400, 160)
    res = types.SimpleNamespace(B=3)                                                          # StreamingResampler.check reads self.B alone (the object itself needs the GPU)
    return (("StreamingFbank", lambda lens, final, columns: sched.check(lens, final, columns)),
            ("StreamingResampler", lambda lens, final, columns: resample.StreamingResampler.check(res, lens, final, columns)))


def test_host_packets_both_owners_agree_on_valid_input():
    for lens, final in (([1, 0, 10], [True, False, 1]), (torch.tensor([1, 0, 10]), torch.tensor([True, False, True])), ((1, 0, 10), None),
                        (torch.tensor([1, 0, 10], dtype=torch.int16), [0, 0, 0]), (None, None)):
        got = [check(lens, final, 10) for _, check in owners()]
        assert got[0] == got[1]
        want_final = [False] * 3 if final is None else [bool(f) for f in (final.tolist() if isinstance(final, torch.Tensor) else final)]
        assert got[0] == ([10, 10, 10] if lens is None else [1, 0, 10], want_final)
        assert all(type(n) is int for n in got[0][0]) and all(type(f) is bool for f in got[0][1])


@pytest.mark.parametrize("lens, final, match", [
    ([0, 0], None, "2 sample_lens for 3 streams"),
    ([0, 0, 0], [True] * 4, "4 final for 3 streams"),
    (torch.zeros(4, dtype=torch.int32), None, "4 sample_lens for 3 streams"),
    ([0, 0, -1], None, r"sample_lens\[2\] = -1: a count of new samples, 0 \.\. the block's 10 columns"),
    ([1.5, 0, 0], None, r"sample_lens\[0\] = 1\.5"),
    ([0, None, 0], None, r"sample_lens\[1\] = None"),
    ([11, 0, 0], None, r"sample_lens\[0\] = 11: .*10 columns"),
    (torch.tensor([0, 11, 0]), None, r"sample_lens\[1\] = 11: .*10 columns"),
    (torch.zeros(3), None, r"sample_lens must hold 3 integers, got torch\.float32 \(3,\)"),
    (torch.zeros(3, 1, dtype=torch.int32), None, "sample_lens must hold 3 integers"),
    ([0, 0, 0], torch.zeros(3), "final must hold 3 integers"),
    (torch.zeros(3, dtype=torch.int32, device="meta"), None, "sample_lens are host values .*got a tensor on meta"),
    ([0, 0, 0], torch.zeros(3, dtype=torch.bool, device="meta"), "final are host values"),
])
def test_host_packets_refusals_are_the_same_for_both_owners(lens, final, match):
    for name, check in owners():
        with pytest.raises(ValueError, match=match) as e:
            check(lens, final, 10)
        assert str(e.value).startswith(name + ": ")


def test_fbank_keeps_its_own_parts():
    import fbank
    sched = fbank.PacketSchedule(3, 2, 400, 160)
    assert sched.check([0, 3279, 0], None) == ([0, 3279, 0], [False] * 3)                     # columns=None: no column bound, accepts() is the bound
    with pytest.raises(ValueError, match=r"stream 1 is handed 3280 samples and accepts 3279"):
        sched.check([0, 3280, 0], None)
    with pytest.raises(ValueError, match=r"sample_lens\[0\] = None: a count of new samples, 0 \.\. accepts\(\)"):
        sched.check(None, None)
