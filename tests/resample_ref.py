"""torchaudio.transforms.Resample restated in float64 numpy (torchaudio is not a dependency), for its default arguments: sinc_interp_hann,
lowpass_filter_width 6, rolloff 0.99 -- _get_sinc_resample_kernel + _apply_sinc_resample_kernel, the first line of the reference's
preprocess / preprocess_stream (src/deploy.py:108-110, :129-131) and processor.resample (src/processor.py:49-59).

  g = gcd(orig, new), o = orig / g, n = new / g, base = min(o, n) * 0.99, width = ceil(6 o / base)
  h[j][i] = sinc(t) cos^2(pi t / 12) base / o,  t = clamp((-j / n + i / o) base, -6, 6),  phase j < n, tap i = -width .. width + o - 1
  y[q n + j] = sum_i h[j][i] x[q o + i]   with x zero outside [0, L), cut to ceil(n L / o) samples

`resample` is the convolution form (what torchaudio computes, as one matrix product per phase bank), `resample_samples` the definition as a plain
double loop for a handful of outputs, and `StreamRef` the streaming emission rule in integers alone."""
import math

import numpy as np

LOWPASS_WIDTH = 6
ROLLOFF = 0.99


def geometry(orig_freq, new_freq):
    """(o, n, base, width) of the reduced rate pair."""
    g = math.gcd(int(orig_freq), int(new_freq))
    o, n = int(orig_freq) // g, int(new_freq) // g
    base = min(o, n) * ROLLOFF
    return o, n, base, int(math.ceil(LOWPASS_WIDTH * o / base))


def kernel(orig_freq, new_freq):
    """h as float64 [n, 2 width + o]: column k is tap i = k - width."""
    o, n, base, width = geometry(orig_freq, new_freq)
    i = np.arange(-width, width + o, dtype=np.float64)[None, :] / o
    j = np.arange(0, -n, -1, dtype=np.float64)[:, None] / n
    t = np.clip((j + i) * base, -LOWPASS_WIDTH, LOWPASS_WIDTH)
    window = np.cos(t * math.pi / LOWPASS_WIDTH / 2) ** 2
    t = t * math.pi
    safe = np.where(t == 0, 1.0, t)
    return np.where(t == 0, 1.0, np.sin(safe) / safe) * window * (base / o)


def num_samples(L, orig_freq, new_freq):
    o, n, _, _ = geometry(orig_freq, new_freq)
    return -(-n * L // o)


def resample(x, orig_freq, new_freq, with_bound=False):
    """x: 1-D waveform -> float64 [ceil(n L / o)].  with_bound: also sum_i |h_i| |x_i| per output sample (the scale of a float32 evaluation's error)."""
    o, n, _, width = geometry(orig_freq, new_freq)
    h = kernel(orig_freq, new_freq)
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    L = x.shape[0]
    xp = np.concatenate([np.zeros(width), x, np.zeros(width + o)])
    blocks = L // o + 1                                                      # conv1d with stride o over L + 2 width + o samples
    frames = np.lib.stride_tricks.as_strided(xp, (blocks, h.shape[1]), (o * xp.strides[0], xp.strides[0]))
    y = (frames @ h.T).reshape(-1)[:num_samples(L, orig_freq, new_freq)]
    if not with_bound:
        return y
    return y, (np.abs(frames) @ np.abs(h).T).reshape(-1)[:y.shape[0]]


def resample_samples(x, orig_freq, new_freq, which):
    """The definition, one output sample at a time: y[p] for p in `which`."""
    o, n, base, width = geometry(orig_freq, new_freq)
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    out = []
    for p in which:
        q, j = divmod(int(p), n)
        acc = 0.0
        for i in range(-width, width + o):
            m = q * o + i
            if not 0 <= m < x.shape[0]:
                continue
            t = min(max((-j / n + i / o) * base, -LOWPASS_WIDTH), LOWPASS_WIDTH)
            w = math.cos(t * math.pi / LOWPASS_WIDTH / 2) ** 2
            t *= math.pi
            acc += (1.0 if t == 0 else math.sin(t) / t) * w * (base / o) * x[m]
        out.append(acc)
    return np.array(out)


class StreamRef:
    """How many output samples exist after a stream has received c input samples: every whole block q with (q + 1) o + width <= c (all of its
    taps' samples are there), n samples each; ceil(n c / o) once the stream is final.  Integers only."""

    def __init__(self, orig_freq, new_freq):
        self.o, self.n, _, self.width = geometry(orig_freq, new_freq)
        self.seen = self.emitted = 0

    def exist(self, c, final):
        if final:
            return -(-self.n * c // self.o)
        return max(0, (c - self.width) // self.o) * self.n

    def push(self, n_new, final):
        """-> the samples this packet makes available."""
        self.seen += n_new
        now = self.exist(self.seen, final)
        out, self.emitted = now - self.emitted, now
        return out
