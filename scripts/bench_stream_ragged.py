"""Cost of per-stream window lengths in the batched streaming step, config 5 (64 streams, chunk 16, left context 4 chunks, the config-2 encoder, bf16),
encoder step only (encoder.StreamingBatch, captured graph), one MI355X, one process:

  none     step(frames)                              -- lengths never given: the step as it was
  full     step(frames, [window] * B)                -- the length-aware step on whole windows
  ragged   step(frames, lens), a quarter of the streams on a short window (9, 23, 37, 51 frames and 0, cycling) in every step

STEPS steps each (default 200) after WARMUP, REPS alternating repetitions, HIP events around whole steps; per variant the median, the 10th / 90th
percentile per repetition and a sha256 over the outputs of the last 8 steps.  VARIANTS=none runs that variant only, which also works on a commit
that has no frame_lens: compare two commits' `none` lines, run alternately, for the cost of the feature when unused."""
import hashlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "conformer-pytorch-lightning_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import cfm, bench
import encoder as enc_mod

B, chunk, left = int(os.environ.get("STREAMS", "64")), 16, 4
STEPS, WARMUP, REPS = int(os.environ.get("STEPS", "200")), int(os.environ.get("WARMUP", "40")), int(os.environ.get("REPS", "3"))
VARIANTS = os.environ.get("VARIANTS", "none,full,ragged").split(",")
cfm.set_precision("bf16")
dev = torch.device("cuda", 0)
enc = bench.build_encoder(dev)
window, hop = (chunk - 1) * 4 + 7, 4 * chunk
total = WARMUP + STEPS
x = torch.from_numpy(np.random.RandomState(5).standard_normal((B, window + total * hop, 80)).astype(np.float32)).to(dev)
SHORT = [9, 23, 37, 51, 0]


def lens_of(variant, s):
    if variant == "none":
        return None
    if variant == "full":
        return [window] * B
    return [SHORT[(b // 4 + s) % len(SHORT)] if b % 4 == 3 else window for b in range(B)]


def run(variant):
    sb = enc_mod.StreamingBatch(enc, B, chunk, left)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(total)]
    h = hashlib.sha256()
    with torch.no_grad():
        for s in range(total):
            win = x[:, s * hop: s * hop + window].contiguous()
            fl = lens_of(variant, s)
            ev[s][0].record()
            y = sb.step(win) if fl is None else sb.step(win, fl)
            ev[s][1].record()
            if s >= total - 8:
                h.update(y.cpu().numpy().tobytes())
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) for a, b in ev[WARMUP:]), h.hexdigest()


for rep in range(REPS):
    for v in VARIANTS:
        t, digest = run(v)
        print("rep %d %-6s step median %.1f us  p10 %.1f  p90 %.1f  (%d steps, %d streams)  outputs sha256 %s"
              % (rep, v, 1e3 * t[len(t) // 2], 1e3 * t[len(t) // 10], 1e3 * t[len(t) * 9 // 10], STEPS, B, digest[:16]), flush=True)
