"""GPU: sample-rate conversion on the device -- resample.Resampler / StreamingResampler (csrc/resample.hip) and the recognisers' sample_rate.

  1. parity: every output sample of 48 / 44.1 / 22.05 / 8 kHz -> 16 kHz against the float64 restatement of torchaudio's Resample (tests/resample_ref.py),
     gated per sample by the float32 dot product's own bound  |y_dev - y_ref| <= (k + 2) 2^-24 sum_i |h_i| |x_i|,  k the phase's live taps, the right-hand
     side computed in float64 -- for the int16 clip of tests/golden/fbank.npz read as if at the source rate and for ragged float32 batches whose lengths
     are the specification's edge cases and the two sides of the kernel's tile boundary.  (A float32 emulation on the host stays at 3.8 - 6.4 x
     2^-24 sum |h| |x|; the bound is 15 - 39 x.)  Output contract: lengths ceil(n len / o), exact zeros behind them, guard bands intact;
  2. streaming equals offline BIT FOR BIT for random packets (empty ones, one-sample ones, a final that brings no sample, a stream reset half way and
     restarted on other audio), the device's counts equal the host mirror after every call, an idle stream's state does not change by a bit, and what
     lies behind a stream's own samples (NaN) is never read;
  3. end to end with the synthetic weights: recognize_audio(sample_rate=44100) is recognize_audio on the resampled batch; a StreamingRecognizer at 44.1 kHz
     fed random packets gives the tokens and windows of a 16 kHz one fed the offline-resampled audio; accepts() is honoured."""
import functools
import random

import numpy as np
import pytest
import torch

import extent
import resample_ref as R
from conftest import load_golden
from test_fbank_gpu import long_signal
from test_stream_audio_ragged_gpu import block_of, models, packets, precision, recognizer  # noqa: F401  (precision is a fixture)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
RATES = [48000, 44100, 22050, 8000]


def tile_samples(rate):
    """Output samples per workgroup tile."""
    import cfm
    o, n, _, width = R.geometry(rate, 16000)
    return cfm.lib().cfm_resample_tile_blocks(o, n, width) * n


def run_guarded(rs, batch, lengths):
    """cfm.resample with every operand between guard bands -> (out, out_lens) on the host."""
    import cfm
    g = extent.Guards(DEV)
    x = g.inp(batch, name="samples")
    lens = g.inp(torch.tensor(lengths, dtype=torch.int32), name="lengths")
    tables = tuple(g.inp(t, name="table") for t in rs._host)
    out = g.out((batch.shape[0], rs.num_samples(batch.shape[1])), name="out")
    out_lens = g.out((batch.shape[0],), torch.int32, name="out_lens")
    cfm.resample(x, lens, tables, rs.geometry, out, out_lens)
    torch.cuda.synchronize()
    g.check()
    return out.cpu(), out_lens.cpu().tolist()


def gate(rs, rate, x, got, what):
    """Per output sample: |y_dev - y_ref| <= (k + 2) 2^-24 sum |h| |x|, everything on the right in float64.  Returns the worst ratio to 2^-24 sum |h| |x|."""
    ref, scale = R.resample(x, rate, 16000, with_bound=True)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if ref.size == 0:
        return 0.0
    off = rs._host[2].numpy().astype(np.int64)
    k = (off[1:] - off[:-1])[np.arange(ref.size) % rs.n]
    err = np.abs(got.astype(np.float64) - ref)
    bound = (k + 2) * 2.0 ** -24 * scale
    worst = float((err / np.maximum(2.0 ** -24 * scale, 1e-300)).max())
    bad = np.nonzero(err > bound)[0]
    assert bad.size == 0, "%s: %d of %d samples outside the bound, first at %d: |d| %.3e > %.3e" % (what, bad.size, ref.size, bad[0], err[bad[0]], bound[bad[0]])
    return worst


@pytest.mark.parametrize("rate", RATES)
def test_parity_with_the_float64_reference(rate):
    import resample
    rs = resample.Resampler(rate)
    o, n, width = rs.geometry
    pcm = load_golden("fbank")[0]["pcm"]
    assert pcm.dtype == np.int16
    out, out_lens = run_guarded(rs, torch.from_numpy(pcm.copy())[None], [len(pcm)])
    assert out_lens == [rs.num_samples(len(pcm))] and out.shape[1] == out_lens[0]
    worst = [gate(rs, rate, pcm, out[0].numpy(), "int16 clip at %d Hz" % rate)]
    tile = tile_samples(rate)
    assert tile % n == 0 and tile >= n
    edge = tile // n * o                                                     # an input of `edge` samples ends on the tile's last output, edge + 1 starts the next tile
    assert rs.num_samples(edge) == tile and rs.num_samples(edge + 1) > tile
    lengths = [0, 1, o - 1, o, o + 1, width, 2 * width + o + 1, edge, edge + 1]
    rng = np.random.default_rng(rate)
    for batch_lens in (lengths[0:3], lengths[3:6], lengths[6:9], [edge + 1, 0, 2 * edge + o + 5]):
        N = max(batch_lens) + 3                                               # columns no item owns
        batch = rng.standard_normal((3, N)).astype(np.float32)
        out, out_lens = run_guarded(rs, torch.from_numpy(batch), batch_lens)
        assert out_lens == [rs.num_samples(L) for L in batch_lens], (batch_lens, out_lens)
        assert out.shape[1] == rs.num_samples(N)
        for b, L in enumerate(batch_lens):
            assert bool((out[b, out_lens[b]:] == 0).all()), (batch_lens, b)
            worst.append(gate(rs, rate, batch[b, :L], out[b, :out_lens[b]].numpy(), "f32 item of %d samples at %d Hz" % (L, rate)))
    print("  %d -> 16000 Hz: worst |y_dev - y_ref| = %.2f x 2^-24 sum|h||x| (the bound is %d .. %d x)"
          % (rate, max(worst), int(rs._host[2].diff().min()) + 2, int(rs._host[2].diff().max()) + 2))


def test_equal_rates_return_the_input_and_no_cpu_path():
    import resample
    rs = resample.Resampler(16000)
    x, lens = torch.zeros((2, 50), dtype=torch.int16, device=DEV), torch.tensor([50, 20], dtype=torch.int32, device=DEV)
    y, n = rs(x, lens)
    assert y is x and n is lens
    with pytest.raises(RuntimeError, match="no CPU path"):
        resample.Resampler(8000)(x.cpu(), lens.cpu())


@pytest.mark.parametrize("rate,dtype", [(44100, torch.int16), (8000, torch.float32)])
def test_streaming_equals_offline_bit_for_bit(rate, dtype):
    import resample
    rs = resample.Resampler(rate)
    o, n, width = rs.geometry
    lengths = [9000, 4 * o + width, 12345, 7001]
    sig = long_signal()
    if dtype == torch.int16:
        utts = [sig[3000 * b: 3000 * b + L].copy() for b, L in enumerate(lengths)]
        other = sig[20000:20000 + 5000].copy()
    else:
        rng = np.random.default_rng(7)
        utts = [rng.standard_normal(L).astype(np.float32) for L in lengths]
        other = rng.standard_normal(5000).astype(np.float32)

    def offline(us):
        batch = np.zeros((len(us), max(len(u) for u in us)), utts[0].dtype)
        for b, u in enumerate(us):
            batch[b, :len(u)] = u
        y, m = rs(torch.from_numpy(batch).to(DEV), torch.tensor([len(u) for u in us], dtype=torch.int32, device=DEV))
        return [y[b, :k].clone() for b, k in enumerate(m.tolist())]
    want = offline(utts)
    want_other = offline([other])[0]
    assert [len(w) for w in want] == [rs.num_samples(L) for L in lengths]

    sr = resample.StreamingResampler(4, rate, 16000, DEV)
    g = extent.Guards(DEV)                                                    # the state buffers between guard bands
    sr._state = (g.io(sr._state[0], name="tail a"), g.io(sr._state[1], name="counts a"))
    sr._next = (g.io(sr._next[0], name="tail b"), g.io(sr._next[1], name="counts b"))
    assert sr.tail_cap == 2 * width + 2 * o and sr.flush_max == -(-n * (width + o - 1) // o)
    got = [[] for _ in range(4)]
    # stream 3 starts on `other`, is reset half way through it and restarted on its own utterance; stream 1's final arrives alone, in an empty packet
    feed, half, restarted = [utts[0], utts[1], utts[2], other], len(other) // 2, False
    cur, ended, calls, idle_checked = [0] * 4, [False] * 4, 0, False
    rng = random.Random(rate)
    while not all(ended):
        if not restarted and cur[3] == half:
            sr.reset([3])
            got[3], feed[3], cur[3], restarted = [], utts[3], 0, True
        takes, final = [], []
        for b in range(4):
            left = len(feed[b]) - cur[b]
            k = 0 if ended[b] else min(left, rng.choice([0, 1, rng.randint(0, 1500), rng.randint(0, 1500)]))
            if b == 3 and not restarted:
                k = min(k, half - cur[3])
            takes.append(k)
            final.append(not ended[b] and k == left and (b != 1 or k == 0) and (b != 3 or restarted))
        blk = block_of(feed, takes, cur, dtype, garbage="nan" if dtype == torch.float32 else "pattern")
        before = [t.clone() for t in sr._state]
        planned = sr.produces(takes, final)
        out, out_lens, host = sr.step(blk, takes, final)
        assert out_lens.tolist() == host == planned and out.shape == (4, max(host))
        assert sr._state[1].tolist() == [[c, q] for c, q in zip(sr.schedule.seen, sr.schedule.blocks)], calls
        for b in range(4):
            assert bool((out[b, host[b]:] == 0).all()), (calls, b)
            got[b].append(out[b, :host[b]].clone())
            if takes[b] == 0 and not final[b]:                               # an idle stream: not a bit of its state changes
                assert torch.equal(sr._state[0][b], before[0][b]) and torch.equal(sr._state[1][b], before[1][b]) and host[b] == 0, (calls, b)
                idle_checked = True
            elif not final[b]:
                assert host[b] % n == 0 and sr.schedule.held()[b] < width + o
        cur = [c + k for c, k in zip(cur, takes)]
        ended = [e or f for e, f in zip(ended, final)]
        calls += 1
        assert calls < 500
    torch.cuda.synchronize()
    g.check()
    assert idle_checked and restarted and calls >= 10
    for b in range(3):
        assert torch.equal(torch.cat(got[b]), want[b]), (rate, b)
    assert torch.equal(torch.cat(got[3]), want[3]), "the stream reset half way"
    assert sr.schedule.seen == [0] * 4 and sr._state[1].tolist() == [[0, 0]] * 4          # every stream ended: reset by its final packet
    assert not torch.equal(want_other[:100], want[3][:100])


# ----------------------------------------------------------------------------------------------------------------------
# end to end
# ----------------------------------------------------------------------------------------------------------------------
LENGTHS_16K = [7075, 3302, 5080, 871]                                        # five windows, the last one short; two; three; not one


@functools.lru_cache(None)
def source_utterances():
    """Stretches of the clip brought to 44.1 kHz by the float64 reference and rounded to int16: what a browser would send.  (The clip itself read as if
    at 44.1 kHz is speech slowed down 2.76 times, on which the synthetic model's streaming search emits nothing but blanks.)"""
    sig = long_signal()
    return [np.clip(np.rint(R.resample(sig[6000 * b: 6000 * b + L], 16000, 44100)), -32768, 32767).astype(np.int16) for b, L in enumerate(LENGTHS_16K)]


def test_offline_recognizer_resamples_first(precision):
    import resample
    import transducer
    precision("fp32")
    enc, pr, jn, meta = models()
    utts = source_utterances()
    src_lengths = [len(u) for u in utts]
    batch = np.zeros((4, max(src_lengths)), np.int16)
    for b, u in enumerate(utts):
        batch[b, :len(u)] = u
    x, lens = torch.from_numpy(batch).to(DEV), torch.tensor(src_lengths, dtype=torch.int32, device=DEV)
    rec = transducer.OfflineRecognizer(enc, pr, jn, blank=meta["blank"], n_steps=meta["n_steps"])
    want = rec.recognize_audio(*resample.Resampler(44100)(x, lens))
    got = rec.recognize_audio(x, lens, sample_rate=44100)
    assert got == want and sum(len(t) for t in got) > 0
    assert rec.recognize_audio(x, lens, sample_rate=16000) == rec.recognize_audio(x, lens)    # the fbank's own rate: today's path
    assert list(rec._resamplers) == [44100]


def drive(rec, utts, dtype, rng, cap, bad_call=None):
    """step_audio over the utterances in random packets of at most min(accepts(), cap) samples -> per stream the windows (first frame, frames) it ran."""
    B = len(utts)
    ran = [[] for _ in range(B)]
    for k, (takes, final, cur) in enumerate(packets(utts, rec.accepts, rec.pending, None, None, rng, cap)):
        if k == bad_call:                                                    # one sample more than accepts(): refused before any state changes
            room = rec.accepts()
            with pytest.raises(ValueError, match="accepts"):
                rec.step_audio(torch.zeros((B, room[0] + 1), dtype=dtype, device=DEV), sample_lens=[room[0] + 1] + [0] * (B - 1), final=[False] * B)
            assert rec.accepts() == room
        rec.step_audio(block_of(utts, takes, cur, dtype), sample_lens=takes, final=final)
        for b, (first, m) in enumerate(rec.audio.windows):
            if m >= 7:
                ran[b].append((first, m))
    return ran


def test_streaming_recognizer_at_44100_equals_16000_on_resampled_audio(precision):
    import resample
    import transducer
    precision("fp32")
    m = models()
    enc, pr, jn, meta = m
    utts = source_utterances()
    rs = resample.Resampler(44100)
    resampled = []
    for u in utts:
        y, k = rs(torch.from_numpy(u)[None].to(DEV), torch.tensor([len(u)], dtype=torch.int32, device=DEV))
        resampled.append(y[0, :int(k)].cpu().numpy())
    ref = recognizer(m, 4, 2)
    want = drive(ref, resampled, torch.float32, random.Random(1), 2500)
    assert sum(len(h) for h in ref.hyps()) > 0 and [len(w) for w in want][3] == 0 and len(want[0]) >= 4

    rec = transducer.StreamingRecognizer(enc, pr, jn, 4, 2, meta["left"], blank=meta["blank"], n_steps=meta["n_steps"], sample_rate=44100)
    with pytest.raises(ValueError, match="packets"):
        rec.step_audio(torch.zeros((4, 5000), dtype=torch.int16, device=DEV))                 # the whole-block form
    acc = rec.accepts()
    assert acc == [(rec.audio.accepts()[0] * 441) // 160] * 4
    got = drive(rec, utts, torch.int16, random.Random(2), 7000, bad_call=3)
    assert got == want
    assert rec.hyps() == ref.hyps()
    rec.reset()
    assert rec.resampler.schedule.seen == [0] * 4 and rec.accepts() == acc
    again = drive(rec, utts, torch.int16, random.Random(3), 3000)
    assert again == want and rec.hyps() == ref.hyps()
