"""CTC forced alignment beside the CTC loss on the same logits, at the config-3 CTC shape (32 utterances x 249 encoder frames, V = 5002, 33 labels
each), one MI355X, one process:

  nll     cfm.ctc_nll      (rows launch + the alpha recursion: a serial chain of T' barriers on one workgroup per utterance)
  align   cfm.ctc_align    (the same rows launch + the max-plus recursion with recorded moves, the trace-back and the span pass in one launch)

The expectation under test: alignment costs the nll plus the trace-back.  HIP events around whole calls (scratch comes from the arena, so a call is
its launches), WARMUP calls first, then REPS calls, the two ops alternating; median and min..max of each, and the per-kernel times of cfm's own
profiler from one further call of each.  Synthetic logits ~ 3 N(0, 1), seeded labels, full lengths (the longest chain is what a batch waits for).
Writes profiles/r15_ctc_align.txt and prints one JSON line; no threshold."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "conformer-pytorch-lightning_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import cfm, synth

B, T, V, U = 32, 249, 5002, 33
WARMUP, REPS = int(os.environ.get("WARMUP", "20")), int(os.environ.get("REPS", "100"))
dev = torch.device("cuda", 0)
Vp = (V + 3) // 4 * 4
logits = torch.zeros((B, T, Vp), device=dev)
logits[..., :V] = torch.from_numpy(synth.normal(81, (B, T, V), 3.0)).to(dev)
g = torch.Generator().manual_seed(82)
labels = torch.randint(1, V, (B, U), generator=g).to(device=dev, dtype=torch.int32)
enc_lens = torch.full((B,), T, dtype=torch.int32, device=dev)
label_lens = torch.full((B,), U, dtype=torch.int32, device=dev)
ops = {"nll": lambda: cfm.ctc_nll(logits, V, enc_lens, labels, label_lens), "align": lambda: cfm.ctc_align(logits, V, enc_lens, labels, label_lens)}


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b)


for _ in range(WARMUP):
    for fn in ops.values():
        fn()
torch.cuda.synchronize()
ms = {k: [] for k in ops}
for _ in range(REPS):
    for k, fn in ops.items():
        ms[k].append(once(fn))
res = {"shape": {"B": B, "T": T, "V": V, "U": U}, "warmup": WARMUP, "reps": REPS}
for k, v in ms.items():
    res[k + "_us"] = {"median": round(1e3 * float(np.median(v)), 1), "min": round(1e3 * min(v), 1), "max": round(1e3 * max(v), 1)}
res["align_over_nll"] = round(res["align_us"]["median"] / res["nll_us"]["median"], 3)
nll = ops["nll"]().cpu()
path, score, start, end, token_logp = (t.cpu() for t in ops["align"]())
res["score_below_minus_nll"] = bool((score.double() <= -nll.double() + 1e-2).all())
res["mean_frames_per_token"] = round(float((end - start + 1).double().mean()), 2)
cfm.prof_enable(True); cfm.prof_reset()
for fn in ops.values():
    fn()
torch.cuda.synchronize()
res["kernels_us"] = {k: round(1e3 * v["ms"] / max(v["calls"], 1), 1) for k, v in cfm.prof_table().items() if k.startswith("ctc_")}
cfm.prof_enable(False)
line = json.dumps(res)
with open(os.path.join(ROOT, "profiles", "r15_ctc_align.txt"), "w") as f:
    f.write("scripts/bench_ctc_align.py: cfm.ctc_align beside cfm.ctc_nll on the same logits, HIP events, %d warm-up calls, %d timed calls each, alternating\n" % (WARMUP, REPS))
    f.write(line + "\n")
print(line)
