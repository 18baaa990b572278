"""RNN-T forced alignment beside the RNN-T loss forward on the same packed lattice, one MI355X, one process, two shapes:

  head   the config-4 head shape: 16 utterances, T' = 249, 100 labels each, V = 5002 (the rows dominate)
  long   4 utterances, T = 2000, U = 400, V = 32 (2399 diagonals: the recursion is the cost, not the rows)

  nll     cfm.rnnt_nll_packed     (rows launch + the alpha and beta recursions, 2 B workgroups, one barrier per diagonal)
  align   cfm.rnnt_align_packed   (the same rows launch + ONE max-plus recursion with the trace-back in the same launch)

The expectation under test: alignment costs no more than the loss forward (10 % margin for run-to-run spread).  HIP events around whole calls, WARMUP
calls first, then REPS calls, the two ops alternating; median and min..max of each, and the per-kernel times of cfm's own profiler from one further
call of each.  One trace-back variant was built (per node the frame at which its column was last entered by a label move, Ub dependent loads), so one
is timed.  The float64 reference on the host (tests/rnnt_align_ref.py, ONE utterance of the shape) is timed once, for scale.  Synthetic logits
~ 2 N(0, 1), seeded labels, full lengths (the longest chain is what a batch waits for).  Writes profiles/r16_rnnt_align.txt and prints one JSON
line per shape; no threshold."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "conformer-pytorch-lightning_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import cfm, rnnt_align_ref as ref
from cfm import lattice

SHAPES = {"head": (16, 249, 100, 5002), "long": (4, 2000, 400, 32)}
WARMUP, REPS = int(os.environ.get("WARMUP", "10")), int(os.environ.get("REPS", "50"))
dev = torch.device("cuda", 0)


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b)


lines = []
for name, (B, T, U, V) in SHAPES.items():
    lat = lattice.Lattice.padded([T] * B, [U] * B, T, U + 1, dev)
    g = torch.Generator(device=dev).manual_seed(91)
    logits = 2.0 * torch.randn((lat.M, V), generator=g, device=dev)
    targets = torch.randint(0, V - 1, (B, U), generator=torch.Generator().manual_seed(92)).to(device=dev, dtype=torch.int32)
    blank = V - 1
    ops = {"nll": lambda: cfm.rnnt_nll_packed(logits, targets, lat, blank)[0], "align": lambda: cfm.rnnt_align_packed(logits, targets, lat, blank)}
    for _ in range(WARMUP):
        for fn in ops.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in ops}
    for _ in range(REPS):
        for k, fn in ops.items():
            ms[k].append(once(fn))
    res = {"shape": {"name": name, "B": B, "T": T, "U": U, "V": V, "nodes": lat.M}, "warmup": WARMUP, "reps": REPS}
    for k, v in ms.items():
        res[k + "_us"] = {"median": round(1e3 * float(np.median(v)), 1), "min": round(1e3 * min(v), 1), "max": round(1e3 * max(v), 1)}
    res["align_over_nll"] = round(res["align_us"]["median"] / res["nll_us"]["median"], 3)
    nll = ops["nll"]().cpu()
    frame, token_logp, score = (t.cpu() for t in ops["align"]())
    lmax = float(logits.abs().max())
    res["score_below_minus_nll"] = all(float(s) <= -float(n) + ref.delta(T, U, float(s), lmax) for s, n in zip(score, nll))      # the tests' bound
    res["frames_nondecreasing"] = bool((frame[:, 1:] >= frame[:, :-1]).all())
    cfm.prof_enable(True); cfm.prof_reset()
    for fn in ops.values():
        fn()
    torch.cuda.synchronize()
    res["kernels_us"] = {k: round(1e3 * v["ms"] / max(v["calls"], 1), 1) for k, v in cfm.prof_table().items() if k.startswith("rnnt_")}
    cfm.prof_enable(False)
    # the float64 statement on the host, utterance 0 only (a Python double loop over T (U+1) nodes), and its agreement with the device
    x0 = logits[:T * (U + 1)].reshape(1, T, U + 1, V).cpu()
    lb, ll = ref.node_logprobs(x0, targets[:1].cpu(), blank, V)
    t0 = time.perf_counter()
    r = ref.align64(lb[0], ll[0], T, U)
    res["host_f64_one_utterance_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
    res["score_error_utt0"] = abs(float(score[0]) - r["score"])
    res["frames_equal_utt0"] = frame[0].tolist() == r["frames"].tolist()
    lines.append(json.dumps(res))
    print(lines[-1])
with open(os.path.join(ROOT, "profiles", "r16_rnnt_align.txt"), "w") as f:
    f.write("scripts/bench_rnnt_align.py: cfm.rnnt_align_packed beside cfm.rnnt_nll_packed on the same lattice, HIP events, %d warm-up calls, %d timed calls each, alternating\n" % (WARMUP, REPS))
    f.write("\n".join(lines) + "\n")
