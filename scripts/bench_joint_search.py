"""Joint CTC/attention decoding at the deployment shape of scripts/bench_attention_search.py: 32 utterances x beam 10, T' = 249, 6 layers, D = 256,
H = 4, FF = 2048, V = 5002, bf16, eos suppressed (every utterance runs its max_len steps).  Timed by HIP events, median of `reps` runs.

  (a) decoder.JointBeamSearch.search against decoder.AttentionBeamSearch.search in the SAME process: ms per batch and per step.  The difference is
      the cost of the CTC term: a top-k of pre_beam instead of beam classes, cfm_ctc_prefix_score and cfm_ctc_prefix_advance per step, the CTC
      projection and cfm_ctc_logprob_t once per search.  This tree's attention search is ASSUMED to be the parent commit's (the change splits its
      _step into two methods and alters no launch); --parent-tree DIR (a checkout of the parent commit with its library built) checks that: the
      parent's own scripts/bench_attention_search.py runs first, in a child process on the same box, and its per-step time is recorded beside ours;
  (b) per-launch times of the three new kernels and of the top-k from the library's profiling table over one eager search.

    python scripts/bench_joint_search.py [--out profiles/NAME.txt] [--parent-tree DIR]"""
import argparse
import os
import re
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "conformer-pytorch-lightning_amd")]


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ctc-weight", type=float, default=0.3)
    ap.add_argument("--parent-tree", default=None)
    args = ap.parse_args()
    parent_line = "parent commit: not measured (no --parent-tree); this tree's attention search is assumed to launch what the parent's does"
    if args.parent_tree:                                         # before this process touches the GPU: one process at a time on the card
        run = subprocess.run([sys.executable, os.path.join(os.path.abspath(args.parent_tree), "scripts", "bench_attention_search.py"), "--reps", str(args.reps), "--baseline-steps", "2"],
                             cwd=args.parent_tree, capture_output=True, text=True, check=True)
        m = re.search(r"median of (\d+) runs ([0-9.]+) ms \(min ([0-9.]+), max ([0-9.]+)\) per batch, ([0-9.]+) ms per step", run.stdout)
        parent_line = ("parent commit's AttentionBeamSearch (its own scripts/bench_attention_search.py in a child process, same box, same session): median of %s runs %s ms "
                       "(min %s, max %s) per batch, %s ms per step" % m.groups())
    import cfm
    import decoder
    cfm.set_precision("bf16")
    dev = torch.device("cuda")
    B, K, T, D, H, FF, V, layers, steps = 32, 10, 249, 256, 4, 2048, 5002, 6, 60
    torch.manual_seed(0)
    dec = decoder.TransformerDecoder(V, D, H, FF, layers, 0.0, 0.0, 0.0, 0.0).eval().to(dev)
    ctc = decoder.CTCDecoder(V, D, 0.0).eval().to(dev)
    with torch.no_grad():
        dec.output_layer.bias[V - 1] -= 30.0                     # no hypothesis ends: every utterance runs its max_len steps
    g = torch.Generator().manual_seed(1)
    mem = torch.randn(B, T, D, generator=g).to(dev)
    lens = torch.randint(200, T + 1, (B,), generator=g).to(torch.int32).to(dev)
    att = decoder.AttentionBeamSearch(dec, beam=K, max_len=steps)
    joint = decoder.JointBeamSearch(dec, ctc, beam=K, ctc_weight=args.ctc_weight, max_len=steps)
    lines = ["joint CTC/attention beam search: B=%d beam=%d (%d rows) pre_beam=%d ctc_weight=%.2f T'=%d layers=%d D=%d H=%d FF=%d V=%d bf16, %d steps (max_len; eos suppressed), "
             "%d steps per graph" % (B, K, B * K, joint.pre_beam, joint.ctc_weight, T, layers, D, H, FF, V, steps, joint.steps_per_replay)]
    per_step = {}
    for name, s in (("attention search (this tree)", att), ("joint search", joint)):
        s.search(mem, lens)                                      # packs, buffers, the graph
        runs = [event_ms(lambda: s.search(mem, lens))[0] for _ in range(args.reps)]
        ms = statistics.median(runs)
        per_step[name] = ms / s.steps
        lines.append("%s: median of %d runs %.2f ms (min %.2f, max %.2f) per batch, %d steps, %d replays, %.3f ms per step"
                     % (name, args.reps, ms, min(runs), max(runs), s.steps, s.replays, ms / s.steps))
    lines.append(parent_line)
    a, j = per_step["attention search (this tree)"], per_step["joint search"]
    lines.append("the CTC term costs %.3f ms per step (%.1f %% of the attention search's step), the once-per-search work included" % (j - a, 100.0 * (j - a) / a))
    lines.append("memory: x %.1f MB (B V Tp 4 bytes), CTC state %.2f MB (2 R Tp 8 bytes)" % (B * V * ((T + 3) // 4 * 4) * 4 / 1e6, 2 * B * K * ((T + 3) // 4 * 4) * 8 / 1e6))
    eager = decoder.JointBeamSearch(dec, ctc, beam=K, ctc_weight=args.ctc_weight, max_len=steps, use_graph=False)
    eager.search(mem, lens)
    cfm.prof_reset()
    cfm.prof_enable(True)
    eager.search(mem, lens)
    torch.cuda.synchronize()
    table = cfm.prof_table()
    cfm.prof_enable(False)
    total = sum(r["ms"] for r in table.values()) * 1e3
    lines.append("one eager joint search of %d launched steps, the new kernels and their neighbours (cfm profiling table; %.2f ms of kernel time in all):"
                 % (eager.replays * eager.steps_per_replay, total / 1e3))
    for name in ("ctc_logprob_t", "ctc_prefix_score", "ctc_prefix_advance", "ctc_topk", "dec_beam_prune"):
        if name in table:
            r = table[name]
            lines.append("  %-20s %5d calls %9.1f us total %8.2f us per launch %5.1f %%" % (name, r["calls"], r["ms"] * 1e3, r["ms"] * 1e3 / max(r["calls"], 1), 100.0 * r["ms"] * 1e3 / max(total, 1e-9)))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
