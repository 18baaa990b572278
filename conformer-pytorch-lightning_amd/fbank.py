"""Kaldi-compatible log-mel filter bank on the device: the reference's host-side torchaudio call

    kaldi.fbank(waveform * (1 << 15), num_mel_bins=80, frame_length=25, frame_shift=10, dither=0.1, energy_floor=0.0, sample_frequency=16000)

of src/processor.py:175-193 (compute_fbank) and src/deploy.py:106-146 (preprocess, preprocess_stream), with torchaudio's defaults for the
rest (snip_edges, DC removal, pre-emphasis 0.97, povey window, power-of-two padding, low_freq 20, high_freq = Nyquist, power spectrum, log,
no energy column).  One launch of csrc/fbank.hip per call; tables (twiddles, window, sparse mel banks) are computed on the host in float64.

`KaldiFbank` is preprocess: a padded batch of waveforms in, the (padded_feats, feats_length) pair ConformerEncoder.forward takes out.
`StreamingFbank` is preprocess_stream for B streams with the state on the device: blocks of new samples in, the overlapping feature
windows encoder.StreamingBatch reads out.  Dither noise is a pure function of (seed, item or stream, absolute frame, sample in frame):
a frame gets the same draw however the audio was cut into calls, so the streaming features equal the offline ones bit for bit.

The one line of preprocess / preprocess_stream in front of the fbank call, torchaudio's Resample(orig_freq=sample_rate, new_freq=16000)
(deploy.py:108-110, :129-131), is resample.py (Resampler, StreamingResampler), on the device too."""
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

    def forward(self, waveforms, lengths, seed=None):
        """waveforms (B, N) int16 | float32 on the int16 scale, lengths (B,) samples per item ->
        (feats (B, max_frames, num_mel_bins) f32 with zero rows past each item's frames, feats_length int32 (B,)).
        seed: this call's dither seed instead of the object's (training draws new noise every step: augment.TrainFrontend)."""
        cfm.require_hip(waveforms, lengths)
        B, N = waveforms.shape
        rows = max(self.num_frames(N), 1)
        feats = torch.empty((B, rows, self.num_mel_bins), dtype=torch.float32, device=waveforms.device)
        feats_length = torch.empty((B,), dtype=torch.int32, device=waveforms.device)
        cfm.fbank(waveforms, lengths.to(torch.int32), self.tables(waveforms.device), feats, feats_length, self.win, self.shift, self.padded, self.dither,
                  self.seed if seed is None else seed)
        return feats[:, :self.num_frames(N)], feats_length

    __call__ = forward


class PacketSchedule:
    """Host mirror of the streams' audio bookkeeping when packets may have any size (StreamingFbank.step with sample_lens; csrc/fbank.hip does the
    same integer arithmetic on the device, so nothing is read back).  Per stream: `carry` samples waiting, `pos` the absolute feature frame that is
    row 0 of its next window, `final` whether its last packet said the utterance is over.  The windows it emits are the reference's
    greedy_search_streaming_eval loop over the stream's whole utterance (model.py:133-147), however the audio was cut:

      L = carry + new samples;  frames(L) = 1 + (L - win) // shift, 0 below win
      L >= n_first            a whole window of `window` frames; n_next samples and 4 * chunk frames go
      L <  n_first, final     the short last window of m = frames(L) frames; c = ((m - 1) // 2 - 1) // 2 encoder frames (0 below 7 frames:
                              no window at all), 4 * c frames go -- at most 6 are left, less than a window's context: the reference's loop bound
      L <  n_first otherwise  the stream buffers

    A stream accepts n_first + n_next - 1 - carry samples per call, so that its carry stays below n_first."""

    def __init__(self, streams, decoding_chunk_size, win, shift):
        self.B, self.chunk, self.win, self.shift = int(streams), int(decoding_chunk_size), int(win), int(shift)
        self.window, self.hop = (self.chunk - 1) * 4 + 7, 4 * self.chunk
        self.n_first = (self.window - 1) * self.shift + self.win
        self.n_next = self.hop * self.shift
        self.carry, self.pos, self.final = [0] * self.B, [0] * self.B, [False] * self.B

    def frames(self, n):
        return 1 + (n - self.win) // self.shift if n >= self.win else 0

    def reset(self, streams=None):
        for b in (range(self.B) if streams is None else streams):
            self.carry[b], self.pos[b], self.final[b] = 0, 0, False

    def accepts(self):
        """Samples each stream can take in the next call."""
        return [self.n_first + self.n_next - 1 - c for c in self.carry]

    def pending(self):
        """Streams whose carry still holds a window to run: call again with no new samples (and the same `final`) until this is empty."""
        return [b for b in range(self.B) if self.carry[b] >= self.n_first or (self.final[b] and self.frames(self.carry[b]) >= 7)]

    def check(self, sample_lens, final, columns=None):
        """(sample_lens, final) as lists of B ints / bools, or ValueError: host values only, and no stream may be overfilled."""
        lens, final = packing.host_packets("StreamingFbank", self.B, sample_lens, final, columns, upto=None if columns is not None else "accepts()")
        for b, (n, room) in enumerate(zip(lens, self.accepts())):
            if n > room:
                raise ValueError("StreamingFbank: stream %d is handed %d samples and accepts %d (it holds %d; a call runs one window, %d new samples, per stream)"
                                 % (b, n, room, self.carry[b], self.n_next))
        return lens, final

    def advance(self, sample_lens, final):
        """One call: -> per stream (first frame, frames) of the window it runs, frames = 0 where it runs none.  The arguments went through check()."""
        windows = []
        for b in range(self.B):
            L = self.carry[b] + sample_lens[b]
            self.final[b] = final[b]
            if L >= self.n_first:
                m, used, adv = self.window, self.n_next, self.hop
            elif final[b]:
                m = self.frames(L)
                adv = 4 * (((m - 1) // 2 - 1) // 2) if m >= 7 else 0
                used = adv * self.shift
            else:
                m = used = adv = 0
            windows.append((self.pos[b], m))
            self.carry[b], self.pos[b] = L - used, self.pos[b] + adv
        return windows


class StreamingFbank:
    """B streams, `window` = (chunk - 1) * 4 + 7 feature rows per step, of which the first window - 4 * chunk repeat the previous step's last.
    A step consumes n_next = 4 * chunk * shift new samples per stream; the last carry_n = (window - 4 * chunk - 1) * shift + win samples of
    what a stream has read are kept on the device, so a frame that starts in them and ends in the new block is read through one index map.
    A stream that was reset has no carry and reads n_first = (window - 1) * shift + win samples.

    step(samples (B, >= n_first if any stream is fresh else >= n_next), out (B, window, F) f32) -- blocks left-aligned; reset(streams).

    step(samples (B, n), out, sample_lens, final=None): audio packets of ANY size -- stream b brings sample_lens[b] >= 0 new samples, left-aligned (what
    lies behind them in its row is never read), and final[b] says its utterance ends with them.  Host values (lists or CPU tensors of B entries).  The
    stream's window then holds frame_lens[b] frames (device int32 [B], written by the kernel; rows past them are zero): a whole window once n_first
    samples are there, the utterance's short last window when it is final, else none -- PacketSchedule, the host mirror, has the rules.  It gives
    accepts() (samples each stream can take now; more is a ValueError) and pending() (streams with a window still to run: call again with
    sample_lens 0 and the same final) without reading the device.  The first such call widens the carry to n_first samples per stream, with a length
    each; from then on a call without sample_lens brings samples.shape[1] samples for every stream.  Until then nothing changes."""

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
        self._pos = [0] * self.B                             # ... and of pos, for the switch to packets of any size
        self.schedule = None                                 # PacketSchedule once a step was given sample_lens; the state is then (carry [B, n_first], fresh, pos, carry_len)
        self.frame_lens = None                               # int32 [B] on the device: the frames of each stream's last window

    def reset(self, streams=None):
        """New utterances on the given streams (all by default): their next block starts at sample 0 of frame 0."""
        fresh = self._state[1]
        if streams is None:
            fresh.fill_(1)
            streams = range(self.B)
        else:
            streams = list(streams)
            fresh[torch.as_tensor(streams, dtype=torch.long, device=self.device)] = 1
        for b in streams:
            self._fresh[b], self._pos[b] = True, 0
        if self.schedule is not None:
            self.schedule.reset(streams)

    def accepts(self):
        """Samples each stream can take in the next step(..., sample_lens)."""
        return self._schedule().accepts()

    def pending(self):
        """Streams whose carry still holds a window to run (PacketSchedule.pending)."""
        return [] if self.schedule is None else self.schedule.pending()

    def _schedule(self):
        """The host mirror; before the first step with sample_lens, what it will start from: whole blocks leave carry_n samples behind."""
        if self.schedule is not None:
            return self.schedule
        sch = PacketSchedule(self.B, self.chunk, self.fbank.win, self.fbank.shift)
        sch.carry = [0 if f else self.carry_n for f in self._fresh]
        sch.pos = list(self._pos)
        return sch

    def _widen(self):
        """The first step with sample_lens: the carry of carry_n samples becomes the head of one of n_first, with a length per stream."""
        self.schedule = self._schedule()
        def wide(state):
            carry, fresh, pos = state
            w = torch.zeros((self.B, self.n_first), dtype=torch.float32, device=self.device)
            w[:, :self.carry_n] = carry
            return (w, fresh, pos, torch.full((self.B,), self.carry_n, dtype=torch.int32, device=self.device))
        self._state, self._next = wide(self._state), wide(self._next)
        self.frame_lens = torch.zeros((self.B,), dtype=torch.int32, device=self.device)
        self._packet = torch.zeros((2, self.B), dtype=torch.int32, device=self.device)      # this step's (sample_lens, final)

    def _step_packets(self, samples, out, sample_lens, final):
        cfm.require_hip(samples, out)
        if samples.dim() != 2 or samples.shape[0] != self.B:
            raise ValueError("StreamingFbank.step wants (%d, n) samples, got %s" % (self.B, tuple(samples.shape)))
        if tuple(out.shape) != (self.B, self.window, self.fbank.num_mel_bins):
            raise ValueError("StreamingFbank.step writes (%d, %d, %d) feature windows, got a buffer of %s" % (self.B, self.window, self.fbank.num_mel_bins, tuple(out.shape)))
        lens, final = self._schedule().check(sample_lens, final, samples.shape[1])            # raises before anything changes
        if self.schedule is None:
            self._widen()
        self.windows = self.schedule.advance(lens, final)                                    # per stream (first frame, frames) of this step's window
        self._packet.copy_(torch.tensor([lens, [int(f) for f in final]], dtype=torch.int32))
        fb = self.fbank
        cfm.fbank_stream_ragged(samples, self._packet[0], self._packet[1], self._state, self._next, self.frame_lens, fb.tables(samples.device), out,
                                fb.win, fb.shift, fb.padded, self.hop, fb.dither, fb.seed)
        self._state, self._next = self._next, self._state
        self._fresh = [False] * self.B
        self._pos = list(self.schedule.pos)
        return out

    def step(self, samples, out, sample_lens=None, final=None):
        if sample_lens is not None or final is not None or self.schedule is not None:
            return self._step_packets(samples, out, sample_lens, final)
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
        self._pos = [(0 if f else p) + self.hop for f, p in zip(self._fresh, self._pos)]
        self._fresh = [False] * self.B
        return out
