"""Sample-rate conversion on the device: the reference's host-side torchaudio call

    waveform = torchaudio.transforms.Resample(orig_freq=sample_rate, new_freq=16000)(waveform)

that opens src/deploy.py:106-146 (preprocess :108-110, preprocess_stream :129-131) and src/processor.py:49-59 (resample), with torchaudio's defaults
(sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99): a polyphase FIR bank of n = new / gcd phases.  One launch of csrc/resample.hip per call; the
bank is computed on the host in float64 (cfm.packing.resample_tables) and kept compact, each phase's run of live taps.

`Resampler` is the offline half: a padded batch of waveforms in, the (waveforms, lengths) pair fbank.KaldiFbank takes out.  `StreamingResampler` is the
same filter for B streams with the state on the device: packets of any size in, each stream's newly complete output samples out.  An output sample is
one float32 fmaf chain over its live taps in ascending order, whichever call computes it: the streaming samples equal the offline ones bit for bit."""
import torch

import cfm
from cfm import packing


def _tables(orig_freq, new_freq):
    o, n, _, width = packing.resample_geometry(orig_freq, new_freq)
    host = packing.resample_tables(orig_freq, new_freq)
    if cfm.lib().cfm_resample_tile_blocks(o, n, width) <= 0:
        raise ValueError("Resampler: %d -> %d Hz reads %d samples per output block of %d with %d taps on either side: the bank (RESAMPLE_MAX_TABLE_BYTES = %d) and "
                         "one tile's input span do not fit the kernel's LDS" % (orig_freq, new_freq, o, n, width, packing.RESAMPLE_MAX_TABLE_BYTES))
    return (o, n, width), host


class Resampler:

    def __init__(self, orig_freq, new_freq=16000):
        self.orig_freq, self.new_freq = int(orig_freq), int(new_freq)
        self.geometry, self._host = _tables(orig_freq, new_freq)
        self.o, self.n, self.width = self.geometry
        self._dev = {}

    def num_samples(self, L):
        """Output samples for L input samples: ceil(n L / o)."""
        return -(-self.n * int(L) // self.o)

    def tables(self, device):
        t = self._dev.get(device)
        if t is None:
            t = self._dev[device] = tuple(x.to(device) for x in self._host)
        return t

    def forward(self, waveforms, lengths):
        """waveforms (B, N) int16 | float32, lengths (B,) samples per item ->
        (out (B, ceil(n N / o)) f32 on the input's scale with zeros past each item's samples, out_lengths int32 (B,)).  Equal rates: the input itself."""
        cfm.require_hip(waveforms, lengths)
        if self.o == self.n:                                 # torchaudio returns the waveform unchanged
            return waveforms, lengths
        B, N = waveforms.shape
        out = torch.empty((B, self.num_samples(N)), dtype=torch.float32, device=waveforms.device)
        out_lengths = torch.empty((B,), dtype=torch.int32, device=waveforms.device)
        cfm.resample(waveforms, lengths.to(torch.int32), self.tables(waveforms.device), self.geometry, out, out_lengths)
        return out, out_lengths

    __call__ = forward


class ResampleSchedule:
    """Host mirror of the streams' bookkeeping (csrc/resample.hip does the same integer arithmetic on the device, so nothing is read back).  Per stream:
    `seen` input samples c and `blocks` output blocks Q emitted (n samples each).  A call emits every whole block q >= Q with (q + 1) o + width <= c --
    all of its taps' samples have arrived; a final call emits everything up to ceil(n c / o) and leaves the stream reset."""

    def __init__(self, streams, o, n, width):
        self.B, self.o, self.n, self.width = int(streams), int(o), int(n), int(width)
        self.seen, self.blocks = [0] * self.B, [0] * self.B
        self.flush_max = -(-self.n * (self.width + self.o - 1) // self.o)      # a stream holds back at most width + o - 1 input samples

    def reset(self, streams=None):
        for b in (range(self.B) if streams is None else streams):
            self.seen[b] = self.blocks[b] = 0

    def held(self):
        """Input samples each stream has taken that no emitted block has consumed as its own (c - Q o)."""
        return [c - q * self.o for c, q in zip(self.seen, self.blocks)]

    def _one(self, b, n_new, final):
        c = self.seen[b] + n_new
        if final:
            return -(-self.n * c // self.o) - self.blocks[b] * self.n, 0, 0
        q = max(self.blocks[b], (c - self.width) // self.o)
        return (q - self.blocks[b]) * self.n, c, q

    def produces(self, sample_lens, final):
        return [self._one(b, int(sample_lens[b]), bool(final[b]))[0] for b in range(self.B)]

    def advance(self, sample_lens, final):
        out = []
        for b in range(self.B):
            k, self.seen[b], self.blocks[b] = self._one(b, int(sample_lens[b]), bool(final[b]))
            out.append(k)
        return out


class StreamingResampler:
    """B streams.  step(samples (B, n) int16 | float32, sample_lens, final=None) -> (out (B, cap) f32, out_lens int32 [B] on the device, the same lengths
    as a host list): stream b brings sample_lens[b] >= 0 new samples, left-aligned (what lies behind them in its row is never read), final[b] says its
    utterance ends with them (host values: lists or CPU tensors of B entries).  out[b, :out_lens[b]] are the stream's newly complete output samples, zeros
    behind them; cap is the largest of the lengths.  A stream holds back fewer than width + o input samples -- those whose output still waits for taps to
    arrive -- until its final packet, which flushes at most flush_max samples and leaves the stream reset for its next utterance.
    produces(sample_lens, final) gives the lengths a step would return without running it or reading the device; reset(streams) starts new utterances."""

    def __init__(self, streams, orig_freq, new_freq=16000, device="cuda"):
        self.orig_freq, self.new_freq = int(orig_freq), int(new_freq)
        self.B, self.device = int(streams), torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("cfm: StreamingResampler on %s -- this framework runs on MI355X (HIP) only; there is no CPU path" % self.device)
        self.geometry, host = _tables(orig_freq, new_freq)
        self.o, self.n, self.width = self.geometry
        if self.o == self.n:
            raise ValueError("StreamingResampler: %d -> %d Hz is no conversion; hand the samples on as they are" % (self.orig_freq, self.new_freq))
        self.tables = tuple(x.to(self.device) for x in host)
        self.schedule = ResampleSchedule(self.B, self.o, self.n, self.width)
        self.flush_max = self.schedule.flush_max
        self.tail_cap = 2 * self.width + 2 * self.o
        def state():                                         # (tail, counts = (seen, blocks))
            return (torch.zeros((self.B, self.tail_cap), dtype=torch.float32, device=self.device), torch.zeros((self.B, 2), dtype=torch.int64, device=self.device))
        self._state, self._next = state(), state()          # read by the next step / written by it: swapped after every step
        self._packet = torch.zeros((2, self.B), dtype=torch.int32, device=self.device)       # this step's (sample_lens, final)
        self.out_lens = torch.zeros((self.B,), dtype=torch.int32, device=self.device)

    def reset(self, streams=None):
        """New utterances on the given streams (all by default).  Clearing a stream's counts is what resets it (the kernel then reads its tail as the
        zero padding whatever it holds); the tail is cleared too, so that a reset stream's buffers are those of a new one bit for bit."""
        tail, counts = self._state
        if streams is None:
            counts.zero_()
            tail.zero_()
        else:
            streams = list(streams)
            idx = torch.as_tensor(streams, dtype=torch.long, device=self.device)
            counts[idx] = 0
            tail[idx] = 0
        self.schedule.reset(streams)

    def check(self, sample_lens, final, columns):
        """(sample_lens, final) as lists of B ints / bools, or ValueError: host values only."""
        return packing.host_packets("StreamingResampler", self.B, sample_lens, final, columns)

    def produces(self, sample_lens, final=None):
        return self.schedule.produces(sample_lens, final if final is not None else [False] * self.B)

    def step(self, samples, sample_lens=None, final=None):
        cfm.require_hip(samples)
        if samples.dim() != 2 or samples.shape[0] != self.B:
            raise ValueError("StreamingResampler.step wants (%d, n) samples, got %s" % (self.B, tuple(samples.shape)))
        lens, final = self.check(sample_lens, final, samples.shape[1])                      # raises before anything changes
        host = self.schedule.advance(lens, final)
        out = torch.empty((self.B, max(host)), dtype=torch.float32, device=self.device)
        self._packet.copy_(torch.tensor([lens, [int(f) for f in final]], dtype=torch.int32))
        cfm.resample_stream(samples, self._packet[0], self._packet[1], self._state, self._next, self.tables, self.geometry, out, self.out_lens)
        self._state, self._next = self._next, self._state
        return out, self.out_lens, host
