"""Batched edit distance on one MI355X, one process: one cfm.edit_distance call at 64 pairs (a batch's 1-best) and at 960 pairs (64 utterances x 15
hypotheses, the references shared through ref_index), with lengths drawn around 30 tokens (word level) and around 250 tokens (subword level):

  dist     counts=False: the distance alone, no scratch
  counts   counts=True: moves recorded, the backtrace, (S, D, I, hits)
  ops      counts and the op strings
  host     the same pairs through tests/edit_distance_ref.py distance() in a Python loop (once; what a caller without the kernel does)
  torchaudio.functional.edit_distance in a loop as well, when it is importable

Hypotheses are the references with a seeded 15 % of edits (a recogniser's output, not noise: the backtrace follows long diagonals).  HIP events around
whole calls -- the scratch comes from the arena, so a call is its launch --, WARMUP calls of every variant first, then REPS calls with the variants
alternating; median and min..max.  The device results are compared with the host loop's.  Writes profiles/r17_edit_distance.txt and prints one JSON
line; no threshold."""
import json, os, random, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "conformer-pytorch-lightning_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import cfm, metrics
import edit_distance_ref as ref

WARMUP, REPS = int(os.environ.get("WARMUP", "20")), int(os.environ.get("REPS", "100"))
dev = torch.device("cuda", 0)
try:
    from torchaudio.functional import edit_distance as ta_edit_distance
except Exception:
    ta_edit_distance = None


def corrupt(rs, r, V):
    h = []
    for t in r:
        x = rs.random()
        if x < 0.05:
            continue                                           # deletion
        h.append(rs.randrange(V) if x < 0.10 else t)           # substitution
        if x > 0.95:
            h.append(rs.randrange(V))                          # insertion
    return h


def workload(n_utt, n_hyp, mean, V, seed):
    rs = random.Random(seed)
    refs = [[rs.randrange(V) for _ in range(max(1, int(rs.gauss(mean, mean / 5))))] for _ in range(n_utt)]
    hyps = [corrupt(rs, r, V) for r in refs for _ in range(n_hyp)]
    index = [u for u in range(n_utt) for _ in range(n_hyp)]
    return hyps, refs, index


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b)


def stats(v):
    return {"median": round(1e3 * float(np.median(v)), 1), "min": round(1e3 * min(v), 1), "max": round(1e3 * max(v), 1)}


res = {"warmup": WARMUP, "reps": REPS, "torchaudio": ta_edit_distance is not None, "cases": []}
for name, n_utt, n_hyp, mean, V in (("64 pairs, ~30 tokens", 64, 1, 30, 2000), ("64 pairs, ~250 tokens", 64, 1, 250, 5000),
                                    ("960 pairs, ~30 tokens", 64, 15, 30, 2000), ("960 pairs, ~250 tokens", 64, 15, 250, 5000)):
    hyps, refs, index = workload(n_utt, n_hyp, mean, V, 17)
    h, hl = metrics.pack(hyps, dev)
    r, rl = metrics.pack(refs, dev)
    ri = torch.tensor(index, dtype=torch.int32, device=dev)
    variants = {"dist": lambda: cfm.edit_distance(h, hl, r, rl, ref_index=ri, counts=False),
                "counts": lambda: cfm.edit_distance(h, hl, r, rl, ref_index=ri, counts=True),
                "ops": lambda: cfm.edit_distance(h, hl, r, rl, ref_index=ri, counts=True, ops=True)}
    for _ in range(WARMUP):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(REPS):
        for k, fn in variants.items():
            ms[k].append(once(fn))
    t0 = time.perf_counter()
    host = [ref.distance(hh, refs[u]) for hh, u in zip(hyps, index)]
    host_ms = 1e3 * (time.perf_counter() - t0)
    entry = {"case": name, "P": len(hyps), "R": len(refs), "Hmax": h.shape[1], "Umax": r.shape[1], "mean_hyp_len": round(float(np.mean([len(x) for x in hyps])), 1),
             "mean_ref_len": round(float(np.mean([len(x) for x in refs])), 1), "scratch_bytes": int(cfm.lib().cfm_edit_distance_scratch_bytes(len(hyps), h.shape[1], r.shape[1]))}
    for k, v in ms.items():
        entry[k + "_us"] = stats(v)
    entry["host_python_loop_ms"] = round(host_ms, 1)
    if ta_edit_distance is not None:
        t0 = time.perf_counter()
        ta = [ta_edit_distance(refs[u], hh) for hh, u in zip(hyps, index)]
        entry["torchaudio_loop_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
        entry["torchaudio_agrees"] = ta == host
    d, c, _, _ = variants["ops"]()
    entry["equals_host"] = d.tolist() == host and variants["dist"]()[0].tolist() == host
    entry["mean_dist"] = round(float(np.mean(host)), 2)
    res["cases"].append(entry)
line = json.dumps(res)
with open(os.path.join(ROOT, "profiles", "r17_edit_distance.txt"), "w") as f:
    f.write("scripts/bench_edit_distance.py: one cfm.edit_distance call per variant, HIP events, %d warm-up calls, %d timed calls each, the variants alternating\n" % (WARMUP, REPS))
    for e in res["cases"]:
        f.write(json.dumps(e) + "\n")
print(line)
