"""Kaldi-compatible log-mel filter bank on the device: the reference's host-side torchaudio call

    kaldi.fbank(waveform * (1 << 15), num_mel_bins=80, frame_length=25, frame_shift=10, dither=0.1, energy_floor=0.0, sample_frequency=16000)

of src/processor.py:175-193 (compute_fbank) and src/deploy.py:106-146 (preprocess, preprocess_stream), with torchaudio's defaults for the
rest (snip_edges, DC removal, pre-emphasis 0.97, povey window, power-of-two padding, low_freq 20, high_freq = Nyquist, power spectrum, log,
no energy column).  One launch of csrc/fbank.hip per call; tables (twiddles, window, sparse mel banks) are computed on the host in float64.

`KaldiFbank` is preprocess: a padded batch of waveforms in, the (padded_feats, feats_length) pair ConformerEncoder.forward takes out.
`StreamingFbank` is preprocess_stream for B streams with the state on the device: blocks of new samples in, the overlapping feature
windows encoder.StreamingBatch reads out.  Dither noise is a pure function of (seed, item or stream, absolute frame, sample in frame):
a frame gets the same draw however the audio was cut into calls, so the streaming features equal the offline ones bit for bit."""
import torch

import cfm
from cfm import packing

MAX_PADDED_WINDOW = 512          # csrc/fbank.hip: one wavefront transforms one frame in 2 x 4 KiB of LDS


class KaldiFbank:

    def __init__(self, num_mel_bins=80, frame_length=25, frame_shift=10, dither=0.0, sample_frequency=16000, seed=0):
        self.num_mel_bins, self.dither, self.seed = int(num_mel_bins), float(dither), int(seed)
        self.sample_frequency = float(sample_frequency)
        self.win = int(self.sample_frequency * frame_length * 0.001)
        self.shift = int(self.sample_frequency * frame_shift * 0.001)
        if self.win < 2 or self.shift < 1 or self.num_mel_bins < 1:
            raise ValueError("KaldiFbank: a frame of %d samples every %d samples, %d mel bins" % (self.win, self.shift, self.num_mel_bins))
        self.padded = max(8, 1 << (self.win - 1).bit_length())
        if self.padded > MAX_PADDED_WINDOW:
            raise ValueError("KaldiFbank: a %g ms frame at %g Hz is %d samples, padded to %d: the kernel transforms padded windows of at most %d samples"
                             % (frame_length, self.sample_frequency, self.win, self.padded, MAX_PADDED_WINDOW))
        self._host = packing.fbank_tables(self.win, self.padded) + packing.pack_mel_banks(self.num_mel_bins, self.padded, self.sample_frequency)
        self._dev = {}

    def num_frames(self, n):
        return 1 + (n - self.win) // self.shift if n >= self.win else 0

    def tables(self, device):
        t = self._dev.get(device)
        if t is None:
            t = self._dev[device] = tuple(x.to(device) for x in self._host)
        return t

    def forward(self, waveforms, lengths):
        """waveforms (B, N) int16 | float32 on the int16 scale, lengths (B,) samples per item ->
        (feats (B, max_frames, num_mel_bins) f32 with zero rows past each item's frames, feats_length int32 (B,))."""
        cfm.require_hip(waveforms, lengths)
        B, N = waveforms.shape
        rows = max(self.num_frames(N), 1)
        feats = torch.empty((B, rows, self.num_mel_bins), dtype=torch.float32, device=waveforms.device)
        feats_length = torch.empty((B,), dtype=torch.int32, device=waveforms.device)
        cfm.fbank(waveforms, lengths.to(torch.int32), self.tables(waveforms.device), feats, feats_length, self.win, self.shift, self.padded, self.dither, self.seed)
        return feats[:, :self.num_frames(N)], feats_length

    __call__ = forward


class StreamingFbank:
    """B streams, `window` = (chunk - 1) * 4 + 7 feature rows per step, of which the first window - 4 * chunk repeat the previous step's last.
    A step consumes n_next = 4 * chunk * shift new samples per stream; the last carry_n = (window - 4 * chunk - 1) * shift + win samples of
    what a stream has read are kept on the device, so a frame that starts in them and ends in the new block is read through one index map.
    A stream that was reset has no carry and reads n_first = (window - 1) * shift + win samples.

    step(samples (B, >= n_first if any stream is fresh else >= n_next), out (B, window, F) f32) -- blocks left-aligned; reset(streams)."""

    def __init__(self, streams, decoding_chunk_size, device, num_mel_bins=80, frame_length=25, frame_shift=10, dither=0.0, sample_frequency=16000, seed=0):
        self.fbank = KaldiFbank(num_mel_bins, frame_length, frame_shift, dither, sample_frequency, seed)
        self.B, self.chunk = int(streams), int(decoding_chunk_size)
        self.window, self.hop = (self.chunk - 1) * 4 + 7, 4 * self.chunk
        fb = self.fbank
        self.n_first = (self.window - 1) * fb.shift + fb.win
        self.n_next = self.hop * fb.shift
        self.carry_n = self.n_first - self.n_next            # (window - hop - 1) * shift + win = 2 * shift + win
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("cfm: StreamingFbank on %s -- this framework runs on MI355X (HIP) only; there is no CPU path" % self.device)
        def state():                                         # (carry, fresh, pos)
            return (torch.zeros((self.B, self.carry_n), dtype=torch.float32, device=self.device), torch.ones((self.B,), dtype=torch.int32, device=self.device),
                    torch.zeros((self.B,), dtype=torch.int32, device=self.device))
        self._state, self._next = state(), state()          # read by the next step / written by it: swapped after every step
        self._fresh = [True] * self.B                        # host mirror of the device flag

    def reset(self, streams=None):
        """New utterances on the given streams (all by default): their next block starts at sample 0 of frame 0."""
        fresh = self._state[1]
        if streams is None:
            fresh.fill_(1)
            self._fresh = [True] * self.B
        else:
            streams = list(streams)
            fresh[torch.as_tensor(streams, dtype=torch.long, device=self.device)] = 1
            for b in streams:
                self._fresh[b] = True

    def step(self, samples, out):
        cfm.require_hip(samples, out)
        need = self.n_first if any(self._fresh) else self.n_next
        if samples.dim() != 2 or samples.shape[0] != self.B or samples.shape[1] < need:
            raise ValueError("StreamingFbank.step wants (%d, >= %d) samples (%s), got %s" %
                             (self.B, need, "a stream was reset: its first block is %d samples" % self.n_first if need == self.n_first else "%d new samples per stream" % self.n_next,
                              tuple(samples.shape)))
        if tuple(out.shape) != (self.B, self.window, self.fbank.num_mel_bins):
            raise ValueError("StreamingFbank.step writes (%d, %d, %d) feature windows, got a buffer of %s" % (self.B, self.window, self.fbank.num_mel_bins, tuple(out.shape)))
        fb = self.fbank
        cfm.fbank_stream(samples, self._state, self._next, fb.tables(samples.device), out, fb.win, fb.shift, fb.padded, self.hop, fb.dither, fb.seed)
        self._state, self._next = self._next, self._state
        self._fresh = [False] * self.B
        return out
