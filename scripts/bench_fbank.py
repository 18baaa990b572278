"""The log-mel front-end (fbank.KaldiFbank / fbank.StreamingFbank, csrc/fbank.hip) on one MI355X, one process:

  (a) offline, 32 utterances x 10 s of int16 audio at 16 kHz -> (32, 998, 80) features;
  (b) config-5 streaming, 64 streams x chunk 16: 10 240 new samples per stream and step -> (64, 67, 80) feature windows;
  (c) the float32 torch restatement of the same arithmetic (tests/fbank_ref.py, what torchaudio computes) on 16 host threads, both shapes;
  (d) transducer.StreamingRecognizer.step_audio against step with the feature windows already resident, at config 5.

Time per call is the median over REPS calls between HIP events (a, b) or over whole steps (d).  Bytes are what the launch has to move --
every sample in once, every feature out once -- and the bound is those bytes over the measured HBM copy rate (6.3 TB/s)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "conformer-pytorch-lightning_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import cfm, bench, synth, fbank, fbank_ref
import joint, predictor, transducer

REPS, WARMUP = int(os.environ.get("REPS", "200")), int(os.environ.get("WARMUP", "20"))
STEPS = int(os.environ.get("STEPS", "100"))
HBM = 6.3e12
dev = torch.device("cuda", 0)
rs = np.random.RandomState(7)


def timed(fn, reps=REPS):
    for _ in range(WARMUP):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return ms[len(ms) // 2], ms[0], ms[-1]


def report(name, ms, n_samples, n_feats):
    byts = n_samples * 2 + n_feats * 4
    bound_us = byts / HBM * 1e6
    print("%-46s median %8.1f us (min %.1f, max %.1f) per call; %.2f MB moved, HBM bound %.2f us: %.1f x the bound, %.0f GB/s%s" %
          (name, ms[0] * 1e3, ms[1] * 1e3, ms[2] * 1e3, byts / 1e6, bound_us, ms[0] * 1e3 / bound_us, byts / (ms[0] * 1e-3) / 1e9,
           "  [launch-bound: the bound is below a launch]" if bound_us < 5 else ""))


# (a) offline
B, N = 32, 160000
wave = torch.from_numpy(np.round(rs.standard_normal((B, N)) * 3000).astype(np.int16)).to(dev)
lens = torch.full((B,), N, dtype=torch.int32, device=dev)
fb = fbank.KaldiFbank()
feats, n = fb(wave, lens)
report("(a) offline 32 x 10 s, KaldiFbank", timed(lambda: fb(wave, lens)), B * N, feats.numel())
fbd = fbank.KaldiFbank(dither=0.1)
report("(a) the same with dither 0.1", timed(lambda: fbd(wave, lens)), B * N, feats.numel())

# (b) streaming
S, chunk, left = 64, 16, 4
sf = fbank.StreamingFbank(S, chunk, dev)
out = torch.empty((S, sf.window, 80), dtype=torch.float32, device=dev)
first = torch.from_numpy(np.round(rs.standard_normal((S, sf.n_first)) * 3000).astype(np.int16)).to(dev)
block = first[:, :sf.n_next].contiguous()
sf.step(first, out)
report("(b) streaming 64 x chunk 16, StreamingFbank.step", timed(lambda: sf.step(block, out)), S * sf.n_next, out.numel())

# (c) the host restatement
torch.set_num_threads(16)
host_wave = wave.cpu()
def host(batch):
    return [fbank_ref.fbank(w, dtype=torch.float32) for w in batch]
for name, batch in (("offline 32 x 10 s", host_wave), ("streaming 64 x 10 960 samples", first.cpu())):
    host(batch)
    t = []
    for _ in range(5):
        t0 = time.perf_counter(); host(batch); t.append(time.perf_counter() - t0)
    print("(c) float32 torch restatement, 16 host threads, %-30s median %8.1f ms per call" % (name, sorted(t)[2] * 1e3))

# (d) end to end at config 5
cfm.set_precision("bf16")
enc = bench.build_encoder(dev)
V, D = 5002, enc.encoder_dim
pr = predictor.RNNPredictor(V, 256, 512, 256, 0.1, 2).eval()
jn = joint.TransducerJoint(V, D, 512, 512).eval()
synth.load_synth_(pr, 53); synth.load_synth_(jn, 54); synth.greedy_joint_(jn, V)
pr, jn = pr.to(dev), jn.to(dev)
total = WARMUP + STEPS
audio = torch.from_numpy(np.round(rs.standard_normal((S, sf.n_first + total * sf.n_next)) * 3000).astype(np.int16)).to(dev)
allf, _ = fb(audio, torch.full((S,), audio.shape[1], dtype=torch.int32, device=dev))


def run(use_audio):
    rec = transducer.StreamingRecognizer(enc, pr, jn, S, chunk, left, n_steps=4)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(total)]
    cursor = 0
    for s in range(total):
        n = sf.n_first if s == 0 else sf.n_next
        if use_audio:
            x = audio[:, cursor:cursor + n]
        else:
            x = allf[:, s * sf.hop:s * sf.hop + sf.window].contiguous()
        cursor += n
        ev[s][0].record()
        rec.step_audio(x) if use_audio else rec.step(x)
        ev[s][1].record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev[WARMUP:])
    return ms[len(ms) // 2]


res = {True: [], False: []}
for rep in range(3):
    for use_audio in (False, True):
        res[use_audio].append(run(use_audio))
a, f = sorted(res[True])[1], sorted(res[False])[1]
print("(d) config-5 recogniser, %d steps x 3 alternating repetitions: step(features resident) %.3f ms, step_audio(samples) %.3f ms per step: + %.3f ms (%.1f%%)" %
      (STEPS, f, a, a - f, 100 * (a - f) / f))
