"""Launch time of the sample-rate converter (csrc/resample.hip), recorded in profiles/r16_resample.txt:

  streaming   64 streams x one 100 ms packet at 48 kHz and at 44.1 kHz, beside the fbank launch of the same 64 streams (chunk 2: one 80 ms window each)
  offline     32 utterances x 30 s at 48 kHz, against the HBM floor of bytes in + bytes out

    python scripts/bench_resample.py [--iters 200]

Times are hipEvent pairs around `iters` back-to-back launches on one stream, after a warm-up; the host-side descriptor work is part of a launch."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "conformer-pytorch-lightning_amd")]

HBM_BYTES_PER_S = 8.0e12            # MI355X peak, for the floor only


def timed(fn, iters):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters          # microseconds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    import cfm
    import fbank
    import resample
    dev = torch.device("cuda")
    print("sample-rate conversion, %s, %d launches per figure" % (torch.cuda.get_device_name(0), args.iters))
    B = 64
    for rate in (48000, 44100):
        n = rate // 10
        sr = resample.StreamingResampler(B, rate, 16000, dev)
        x = (torch.randn((B, n), device=dev) * 3000).to(torch.int16)
        lens, fin = torch.full((B,), n, dtype=torch.int32, device=dev), torch.zeros((B,), dtype=torch.int32, device=dev)
        out = torch.empty((B, (n // sr.o + 2) * sr.n), dtype=torch.float32, device=dev)     # every launch emits n / o blocks, give or take one
        state = [sr._state, sr._next]
        def step():
            cfm.resample_stream(x, lens, fin, state[0], state[1], sr.tables, sr.geometry, out, sr.out_lens)
            state.reverse()
        t = timed(step, args.iters)
        print("  streaming %5d Hz  %d streams x %d samples (100 ms) -> %d columns   %7.1f us per launch" % (rate, B, n, out.shape[1], t))
    sf = fbank.StreamingFbank(B, 2, dev)
    blk = (torch.randn((B, sf.n_first), device=dev) * 3000).to(torch.int16)
    feats = torch.empty((B, sf.window, 80), dtype=torch.float32, device=dev)
    sf.step(blk, feats, sample_lens=[sf.n_first] * B)
    pk = torch.tensor([[sf.n_next] * B, [0] * B], dtype=torch.int32, device=dev)           # a window's worth per launch: the carry stays as it is
    fb = sf.fbank
    state = [sf._state, sf._next]
    def fstep():
        cfm.fbank_stream_ragged(blk[:, :sf.n_next], pk[0], pk[1], state[0], state[1], sf.frame_lens, fb.tables(dev), feats, fb.win, fb.shift, fb.padded, sf.hop, 0.0, 0)
        state.reverse()
    print("  fbank, beside it   %d streams x %d samples (%d ms at 16 kHz), one chunk-2 window each   %7.1f us per launch" % (B, sf.n_next, sf.n_next // 16, timed(fstep, args.iters)))
    B, secs, rate = 32, 30, 48000
    rs = resample.Resampler(rate)
    x = (torch.randn((B, secs * rate), device=dev) * 3000).to(torch.int16)
    lens = torch.full((B,), secs * rate, dtype=torch.int32, device=dev)
    out = torch.empty((B, rs.num_samples(secs * rate)), dtype=torch.float32, device=dev)
    out_lens = torch.empty((B,), dtype=torch.int32, device=dev)
    t = timed(lambda: cfm.resample(x, lens, rs.tables(dev), rs.geometry, out, out_lens), max(20, args.iters // 4))
    nbytes = x.numel() * 2 + out.numel() * 4
    print("  offline   %5d Hz  %d x %d s int16 -> f32: %.1f MB in + out, %7.1f us per launch = %.2f TB/s; floor at %.0f TB/s %.1f us (%.1f x)"
          % (rate, B, secs, nbytes / 1e6, t, nbytes / t / 1e6, HBM_BYTES_PER_S / 1e12, nbytes / HBM_BYTES_PER_S * 1e6, t / (nbytes / HBM_BYTES_PER_S * 1e6)))


if __name__ == "__main__":
    main()
