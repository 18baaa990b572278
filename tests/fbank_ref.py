"""torchaudio.compliance.kaldi.fbank restated in torch ops (torchaudio is not a dependency), for the arguments the reference passes
(src/processor.py:175-193, src/deploy.py:106-146) and torchaudio's defaults for the rest: snip_edges, remove_dc_offset, preemphasis 0.97,
povey window, round_to_power_of_two, low_freq 20, high_freq 0 (Nyquist), use_power, use_log_fbank, no energy, no mean subtraction, no VTLN.

Parameterised by dtype: float32 is what torchaudio computes, float64 is the yardstick both it and the device are measured against.
`noise` (frames, window) replaces torchaudio's torch.randn draw when dither > 0."""
import math

import torch

EPS = 1.1920929e-07            # torch.finfo(torch.float32).eps: torchaudio floors with the float32 epsilon whatever the dtype
PREEMPHASIS = 0.97
LOW_FREQ = 20.0


def window_sizes(frame_length=25.0, frame_shift=10.0, sample_frequency=16000.0):
    """(window, shift, padded window) in samples."""
    win = int(sample_frequency * frame_length * 0.001)
    shift = int(sample_frequency * frame_shift * 0.001)
    padded = 1 << max(0, (win - 1).bit_length())
    return win, shift, padded


def num_frames(n, win=400, shift=160):
    return 1 + (n - win) // shift if n >= win else 0


def mel_scale(f):
    return 1127.0 * torch.log(1.0 + f / 700.0)


def mel_banks(num_mel_bins=80, padded=512, sample_frequency=16000.0, dtype=torch.float64):
    """(num_mel_bins, padded // 2) triangular weights; the Nyquist bin (weight 0) is left out."""
    nyquist = 0.5 * sample_frequency
    lo = 1127.0 * math.log(1.0 + LOW_FREQ / 700.0)
    hi = 1127.0 * math.log(1.0 + nyquist / 700.0)
    delta = (hi - lo) / (num_mel_bins + 1)
    b = torch.arange(num_mel_bins, dtype=dtype).unsqueeze(1)
    left, center, right = lo + b * delta, lo + (b + 1.0) * delta, lo + (b + 2.0) * delta
    mel = mel_scale(sample_frequency / padded * torch.arange(padded // 2, dtype=dtype)).unsqueeze(0)
    up = (mel - left) / (center - left)
    down = (right - mel) / (right - center)
    return torch.clamp(torch.min(up, down), min=0.0)


def fbank(w, num_mel_bins=80, frame_length=25.0, frame_shift=10.0, dither=0.0, sample_frequency=16000.0, dtype=torch.float64, noise=None):
    """w: 1-D waveform on the int16 scale -> (frames, num_mel_bins) log-mel energies in `dtype`."""
    win, shift, padded = window_sizes(frame_length, frame_shift, sample_frequency)
    w = torch.as_tensor(w).to(dtype)
    m = num_frames(w.numel(), win, shift)
    if m == 0:
        return torch.zeros((0, num_mel_bins), dtype=dtype)
    x = w.as_strided((m, win), (shift, 1)).clone()
    if dither > 0:
        x = x + dither * (torch.randn(x.shape, dtype=dtype) if noise is None else noise.to(dtype))
    x = x - x.mean(dim=1, keepdim=True)
    prev = torch.cat([x[:, :1], x[:, :-1]], dim=1)
    x = x - PREEMPHASIS * prev
    x = x * torch.hann_window(win, periodic=False, dtype=dtype).pow(0.85)
    x = torch.nn.functional.pad(x, (0, padded - win))
    power = torch.fft.rfft(x).abs().pow(2.0)[:, :padded // 2]
    mel = power @ mel_banks(num_mel_bins, padded, sample_frequency, dtype).t()
    return torch.clamp(mel, min=EPS).log()
