"""CPU (no GPU): audio packets of any size for the streaming recognizer -- the host side.  fbank.PacketSchedule, the host mirror of the streams'
carry / position bookkeeping (csrc/fbank.hip does the same integer arithmetic on the device), against the reference's window schedule
(model.py:133-147, restated in ref_windows below); the descriptor's new fields, appended; the loud failures.  No compute entry point is called."""
import random

import pytest
import torch

WIN, SHIFT = 400, 160                                   # 25 ms frames every 10 ms at 16 kHz


def num_frames(n, win=WIN, shift=SHIFT):
    return 1 + (n - win) // shift if n >= win else 0


def ref_windows(frames, chunk):
    """The reference's loop over an utterance of `frames` feature frames: [(first frame, frames of the window)]."""
    context, stride, decoding_window = 7, 4 * chunk, (chunk - 1) * 4 + 7
    return [(cur, min(cur + decoding_window, frames) - cur) for cur in range(0, frames - context + 1, stride)]


def samples_for(frames, extra=0):
    return WIN + (frames - 1) * SHIFT + extra if frames else extra


def drive(sched, b, n, rng, cap=None, others=None):
    """Hand stream b of `sched` an utterance of n samples in random packets (0 .. accepts(), or 0 .. cap), the last one final, then drain it.
    Returns the windows of at least 7 frames it ran, [(first frame, frames)]; checks pending() against the reference on the way."""
    want = ref_windows(num_frames(n), sched.chunk)
    got, left, calls, final = [], n, 0, False
    while not final or b in sched.pending():
        calls += 1
        assert calls < 10000
        acc = sched.accepts()[b]
        assert acc >= sched.n_next                      # a stream can always take a whole block
        take = 0 if final else min(rng.randint(0, acc if cap is None else min(cap, acc)), left)
        left -= take
        final = final or left == 0
        lens, fin = [0] * sched.B, [False] * sched.B
        lens[b], fin[b] = take, final
        if others is not None:
            others(lens, fin)
        wins = sched.advance(*sched.check(lens, fin))
        first, m = wins[b]
        assert m in (0, sched.window) or (final and 0 < m < sched.window)        # buffering, a whole window, or the short last one
        if m >= 7:
            got.append((first, m))
        if final:
            assert (b in sched.pending()) == (len(got) < len(want)), (n, got, want)
        else:
            assert b not in sched.pending()             # more audio may come: what it holds is less than a window
    return got


LENGTHS_CHUNK2 = ([0, 399, 400, 1359, 1360, 1999] +
                  [samples_for(f, e) for f in (7, 8, 10, 11, 14, 15, 16, 18, 19, 22, 43, 46) for e in (0, 37, 159)])


def test_schedule_equals_the_reference_loop_for_any_packetisation():
    import fbank
    assert [num_frames(n) for n in (0, 399, 400, 1359, 1360, 1999, 2000)] == [0, 0, 1, 6, 7, 10, 11]
    assert ref_windows(14, 2) == [(0, 11)] and ref_windows(15, 2) == [(0, 11), (8, 7)] and ref_windows(19, 2) == [(0, 11), (8, 11)] and ref_windows(6, 2) == []
    ends = set()
    for chunk, lengths in ((2, LENGTHS_CHUNK2), (16, [0, 1360, samples_for(67), samples_for(66, 5), samples_for(64 + 6), samples_for(64 + 7), samples_for(3 * 64 + 40, 80)])):
        for n in lengths:
            want = ref_windows(num_frames(n), chunk)
            ends.add(want[-1][1] if want else 0)
            for seed in range(20):
                rng = random.Random(1000 * seed + n)
                sched = fbank.PacketSchedule(1, chunk, WIN, SHIFT)
                if chunk == 2:
                    assert (sched.window, sched.n_first, sched.n_next, sched.accepts()) == (11, 2000, 1280, [3279])
                got = drive(sched, 0, n, rng, cap=None if seed % 2 else 500)
                assert got == want, (chunk, n, seed, got, want)
                # the reference's loop is done: calling final again is an idle step that changes nothing
                state = (list(sched.carry), list(sched.pos))
                assert sched.pending() == [] and sched.frames(sched.carry[0]) <= 6
                (first, m), = sched.advance(*sched.check([0], [True]))
                assert m < 7 and (list(sched.carry), list(sched.pos)) == state and first == sched.pos[0]
    assert {0, 7, 8, 10, 11} <= ends


def test_streams_are_independent_and_reset_clears_the_mirror():
    import fbank
    rng = random.Random(5)
    sched = fbank.PacketSchedule(3, 2, WIN, SHIFT)

    def noise(lens, fin):                                # stream 2 keeps receiving whole blocks meanwhile; stream 1 stays silent
        lens[2] = sched.n_next
    got = drive(sched, 0, samples_for(18, 3), rng, cap=700, others=noise)
    assert got == ref_windows(18, 2)
    assert sched.carry[1] == 0 and sched.pos[1] == 0 and sched.pos[2] > 0 and sched.pos[2] % 8 == 0 and sched.carry[2] < sched.n_first
    sched.reset([0])
    assert (sched.carry[0], sched.pos[0], sched.final[0]) == (0, 0, False) and sched.pos[2] > 0
    assert drive(sched, 0, samples_for(15), rng, others=noise) == ref_windows(15, 2)
    sched.reset()
    assert sched.carry == [0, 0, 0] and sched.pos == [0, 0, 0] and sched.final == [False] * 3 and sched.pending() == []


def test_fbank_desc_ragged_fields_match_c():
    import cfm
    fields = ("seed", "n_new", "final", "carry_len_in", "carry_len_out", "frame_lens", "carry_cap")
    assert [n for n, _ in cfm.FbankDesc._fields_][-6:] == list(fields[1:])           # appended: every earlier field keeps its offset
    assert cfm.lib().cfm_version() == 307 and callable(cfm.fbank_stream_ragged)


def test_loud_failures():
    import fbank
    import transducer
    sched = fbank.PacketSchedule(3, 2, WIN, SHIFT)
    with pytest.raises(ValueError, match=r"stream 1 is handed 3280 samples and accepts 3279"):
        sched.check([0, 3280, 0], None)
    sched.advance(*sched.check([0, 1999, 0], None))
    assert sched.accepts() == [3279, 1280, 3279] and sched.carry == [0, 1999, 0]
    with pytest.raises(ValueError, match=r"stream 1 is handed 1281 samples and accepts 1280"):
        sched.check([0, 1281, 0], None)
    with pytest.raises(ValueError, match="2 sample_lens for 3 streams"):
        sched.check([0, 0], None)
    with pytest.raises(ValueError, match="4 final for 3 streams"):
        sched.check([0, 0, 0], [True] * 4)
    with pytest.raises(ValueError, match=r"sample_lens\[2\] = -1"):
        sched.check([0, 0, -1], None)
    with pytest.raises(ValueError, match=r"sample_lens\[0\] = 1\.5"):
        sched.check([1.5, 0, 0], None)
    with pytest.raises(ValueError, match=r"sample_lens\[0\] = 11: .*10 columns"):
        sched.check([11, 0, 0], None, columns=10)
    with pytest.raises(ValueError, match="host values"):
        sched.check(torch.zeros(3, dtype=torch.int32, device="meta"), None)
    with pytest.raises(ValueError, match="must hold 3 integers"):
        sched.check(torch.zeros(3), None)
    assert sched.carry == [0, 1999, 0] and sched.pos == [0, 0, 0]                   # a refused call changes nothing
    assert sched.check(torch.tensor([1, 2, 3]), torch.tensor([True, False, True])) == ([1, 2, 3], [True, False, True])
    rec = transducer.StreamingRecognizer.__new__(transducer.StreamingRecognizer)     # the argument check comes before any device work
    rec.audio = None
    with pytest.raises(ValueError, match="not both"):
        rec.step_audio(None, lens=[1, 1, 1], sample_lens=[0, 0, 0])
    with pytest.raises(ValueError, match="not both"):
        rec.step_audio(None, lens=[1, 1, 1], final=[False] * 3)
    assert rec.pending() == []
    with pytest.raises(RuntimeError, match="no CPU path"):
        fbank.StreamingFbank(2, 2, "cpu")
