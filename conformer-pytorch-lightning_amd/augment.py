"""Training augmentation on the device: the two stages of the reference's recipe between the waveform and the encoder, and the front end
that chains them -- waveforms and lengths in, the (padded_feats, feats_length) pair of ConformerEncoder.forward / forward_window out.

  SpeedPerturb    processor.speed_perturb (src/processor.py:62-77; speeds [0.9, 1.0, 1.1], exp/data_config.json:21): a speed per utterance.  The
                  definition here is torchaudio.functional.speed -- resample from int(s * rate) to rate with the default sinc/hann kernel, the
                  filter of resample.Resampler; 1.0 is the identity.  (The reference calls sox's `speed` + `rate`, which is another filter.)  One
                  launch of cfm_resample_group over the batch, whatever mix of speeds it holds.
  SpecAugment     processor.spec_aug (src/processor.py:151-172; num_t_mask 2, num_f_mask 2, max_t 50, max_f 50, data_config.json:28-33), in
                  place on the raw fbank values (before CMVN, as in the reference), one launch of cfm_spec_augment.
  TrainFrontend   dataset.py:131-167 for a padded batch: resample, speed perturbation, fbank with dither, SpecAugment -- at most four launches.

Every draw on the device is a pure function of (seed, step, item): include/cfm.h states the SpecAugment draws, fbank.py the dither's.  A step
enters a seed as seed + 0x9E3779B1 * step mod 2^32, the dropout sites' convention.  The speed of an item is drawn on the HOST (random.Random):
the host has to size the output before the launch.  Nothing is read back from the device."""
import random

import torch

import cfm
from cfm import packing

GOLDEN = 0x9E3779B1


def step_seed(seed, step):
    """The seed of training step `step`: seed + 0x9E3779B1 * step mod 2^32."""
    return (int(seed) + GOLDEN * int(step)) & 0xFFFFFFFF


class SpeedPerturb:

    def __init__(self, speeds=(0.9, 1.0, 1.1), sample_rate=16000, seed=0):
        self.speeds, self.sample_rate = tuple(float(s) for s in speeds), int(sample_rate)
        self.pairs = [packing.speed_rates(s, self.sample_rate) for s in self.speeds]
        self._host, self.banks = packing.resample_group_tables(self.pairs, cfm.lib().cfm_resample_tile_blocks)
        self.geometry = [(o, n) for o, n, *_ in self.banks]                  # per speed: o input samples become n
        self.rng = random.Random(seed)
        self._dev = {}

    def num_samples(self, L, k):
        """Output samples of an item of L samples at speeds[k]: ceil(n L / o)."""
        o, n = self.geometry[k]
        return -(-n * int(L) // o)

    def tables(self, device):
        if self._host is None:
            return None
        t = self._dev.get(device)
        if t is None:
            t = self._dev[device] = tuple(x.to(device) for x in self._host)
        return t

    def draw(self, B):
        """B indices into `speeds` from the object's generator, random.choice per item as the reference does."""
        return [self.rng.randrange(len(self.speeds)) for _ in range(B)]

    def check(self, choice, B):
        if isinstance(choice, torch.Tensor):
            if choice.device.type != "cpu":
                raise ValueError("SpeedPerturb: choice holds host values (a list or a CPU tensor), the host sizes the output from it; got a tensor on %s" % choice.device)
            if choice.dim() != 1 or choice.dtype.is_floating_point or choice.dtype.is_complex:
                raise ValueError("SpeedPerturb: choice must hold %d integers, got %s %s" % (B, choice.dtype, tuple(choice.shape)))
            choice = choice.tolist()
        choice = list(choice)
        if len(choice) != B:
            raise ValueError("SpeedPerturb: %d choices for %d items" % (len(choice), B))
        for b, k in enumerate(choice):
            if int(k) != k or not 0 <= k < len(self.speeds):
                raise ValueError("SpeedPerturb: choice[%d] = %r: an index into the %d speeds" % (b, k, len(self.speeds)))
        return [int(k) for k in choice]

    def forward(self, waveforms, lengths, choice=None):
        """waveforms (B, N) int16 | float32, lengths (B,) samples per item, choice: per item an index into `speeds` (drawn when omitted) ->
        (out (B, cap) f32 on the input's scale with zeros past each item's samples, out_lengths int32 (B,)); cap = the most N columns can become."""
        cfm.require_hip(waveforms, lengths)
        B, N = waveforms.shape
        choice = self.draw(B) if choice is None else self.check(choice, B)
        self.choice = choice
        cap = max(self.num_samples(N, k) for k in set(choice))
        out = torch.empty((B, cap), dtype=torch.float32, device=waveforms.device)
        out_lengths = torch.empty((B,), dtype=torch.int32, device=waveforms.device)
        bank = torch.tensor(choice, dtype=torch.int32).to(waveforms.device, non_blocking=True)
        cfm.resample_group(waveforms, lengths.to(torch.int32), bank, self.tables(waveforms.device), self.banks, out, out_lengths)
        return out, out_lengths

    __call__ = forward


class SpecAugment:

    def __init__(self, num_t_mask=2, num_f_mask=2, max_t=50, max_f=50, seed=0):
        self.num_t_mask, self.num_f_mask, self.max_t, self.max_f, self.seed = int(num_t_mask), int(num_f_mask), int(max_t), int(max_f), int(seed)
        if self.num_t_mask < 0 or self.num_f_mask < 0 or self.num_t_mask + self.num_f_mask > cfm.SPEC_MAX_MASKS:
            raise ValueError("SpecAugment: %d time and %d frequency masks; the kernel takes at most %d in all" % (self.num_t_mask, self.num_f_mask, cfm.SPEC_MAX_MASKS))
        if not 1 <= self.max_t <= 1 << 30 or not 1 <= self.max_f <= 1 << 30:
            raise ValueError("SpecAugment: max_t %d, max_f %d: a mask's length is drawn from 1 .. max" % (self.max_t, self.max_f))
        self.calls = 0

    def forward(self, feats, lengths, ids=None, step=None, masks=None):
        """feats (B, T_max, F) f32, masked IN PLACE and returned; lengths (B,) frames per item; ids (B,) integers that name the items in the draws
        (their low 32 bits; arange(B) when omitted); step: the training step (the object's call counter when omitted); masks: optional int32
        (B, num_t_mask + num_f_mask, 2) that receives each mask's (start, end)."""
        cfm.require_hip(feats, lengths, ids, masks)
        if step is None:
            step = self.calls
        self.calls += 1
        if ids is not None and ids.dtype != torch.int32:
            ids = (ids.to(torch.int64) & 0xFFFFFFFF).add_(1 << 31).remainder_(1 << 32).sub_(1 << 31).to(torch.int32)      # the low 32 bits, as int32
        return cfm.spec_augment(feats, lengths.to(torch.int32), ids, step_seed(self.seed, step), self.num_t_mask, self.num_f_mask, self.max_t, self.max_f, masks)

    __call__ = forward


class TrainFrontend:
    """resampler: None, a source sample rate (Hz) or a resample.Resampler to 16 kHz; speed: a SpeedPerturb or None; fbank: a fbank.KaldiFbank
    (dither 0.1 by default, the recipe's); spec: a SpecAugment or None."""

    def __init__(self, resampler=None, speed=None, fbank=None, spec=None):
        import fbank as fbank_module
        import resample
        self.fbank = fbank_module.KaldiFbank(dither=0.1) if fbank is None else fbank
        if resampler is not None and not isinstance(resampler, resample.Resampler):
            resampler = resample.Resampler(resampler, int(self.fbank.sample_frequency))
        self.resampler, self.speed, self.spec = resampler, speed, spec

    def forward(self, waveforms, lengths, step, choice=None, ids=None):
        """waveforms (B, N) int16 | float32 on the int16 scale, lengths (B,), step: the training step (it seeds the dither and the masks) ->
        (padded_feats (B, T_max, F) f32, feats_length int32 (B,)).  choice / ids: SpeedPerturb's and SpecAugment's optional arguments."""
        cfm.require_hip(waveforms, lengths)
        if self.resampler is not None:
            waveforms, lengths = self.resampler(waveforms, lengths)
        if self.speed is not None:
            waveforms, lengths = self.speed(waveforms, lengths, choice)
        feats, feats_length = self.fbank.forward(waveforms, lengths, seed=step_seed(self.fbank.seed, step))
        if self.spec is not None:
            self.spec(feats, feats_length, ids=ids, step=step)
        return feats, feats_length

    __call__ = forward
