"""Beam search with the attention decoder at the deployment shape: 32 utterances x beam 10, T' = 249, 6 layers, D = 256, H = 4, FF = 2048,
V = 5002, bf16.  Timed by HIP events, median of `reps` runs.

  (a) decoder.AttentionBeamSearch.search: ms per batch and per step, launches per step;
  (b) by kernel (cfm's profiling table over one search): cfm_dec_step_attn's time against the bytes it must read, self- and cross-attention, and
      the share of the small-M cfm_gemm launches;
  (c) the baseline -- the only thing the parent commit offers: TransformerDecoder.rows_forward over all whole prefixes at every step, the beam picked
      on the host.  Recorded, not gated; it runs `--baseline-steps` steps (default 12) and is reported per step at the mean prefix length it saw.

    python scripts/bench_attention_search.py [--out profiles/NAME.txt]"""
import argparse
import math
import os
import statistics
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


def baseline_steps(cfm, dec, mem, lens, K, steps, sos):
    """rows_forward over every whole prefix per step, log-softmax and the prune on the host side (torch top-k over B x K*V): ms per step."""
    B, T, D = mem.shape
    prec, dev = cfm.get_precision(), mem.device
    E, pe = dec.embed[0].weight.detach(), dec.position_table(steps + 1)
    memf = mem.reshape(B * T, D).contiguous()
    mem_mask = cfm.as_u8_mask(cfm.valid_mask(lens, T)).view(B, 1, T)
    tokens = torch.full((B * K, 1), sos, dtype=torch.long, device=dev)
    score = torch.zeros(B, K, device=dev)
    score[:, 1:] = float("-inf")
    pk = dec._output_pack(prec)
    times = []
    for i in range(steps):
        def one():
            L = tokens.shape[1]
            x = (E[tokens].double() * math.sqrt(D) + pe[:L].double()).float().reshape(B * K * L, D).contiguous()
            mask = cfm.as_u8_mask(torch.ones(L, L, dtype=torch.bool, device=dev).tril().expand(B * K, L, L).contiguous())
            xn = dec.rows_forward(x, (B * K, L), mask, memf, (B, K * L, T), mem_mask, prec)
            logits = cfm.gemm(xn.view(B * K, L, D)[:, -1].contiguous(), pk.w, bias=pk.b, w_lo=pk.w_lo, out_dtype=torch.float32)[:, :pk.V]
            cand = (score.view(B * K, 1) + torch.log_softmax(logits, -1)).view(B, K * pk.V)
            best, idx = cand.topk(K, dim=1)
            parent, cls = (idx // pk.V + torch.arange(B, device=dev).unsqueeze(1) * K).view(-1), (idx % pk.V).view(-1)
            return best, torch.cat([tokens[parent], cls.unsqueeze(1)], 1)
        ms, (score, tokens) = event_ms(one)
        score.cpu()                                              # the host round trip a Python beam loop makes per step
        times.append(ms)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--baseline-steps", type=int, default=12)
    args = ap.parse_args()
    import cfm
    import decoder
    cfm.set_precision("bf16")
    dev = torch.device("cuda")
    B, K, T, D, H, FF, V, layers = 32, 10, 249, 256, 4, 2048, 5002, 6
    torch.manual_seed(0)
    dec = decoder.TransformerDecoder(V, D, H, FF, layers, 0.0, 0.0, 0.0, 0.0).eval().to(dev)
    with torch.no_grad():
        dec.output_layer.bias[V - 1] -= 30.0                     # no hypothesis ends: every utterance runs its max_len steps
    g = torch.Generator().manual_seed(1)
    mem = torch.randn(B, T, D, generator=g).to(dev)
    lens = torch.randint(200, T + 1, (B,), generator=g).to(torch.int32).to(dev)
    steps = 60
    bs = decoder.AttentionBeamSearch(dec, beam=K, max_len=steps)
    bs.search(mem, lens)                                         # packs, buffers, the graph
    runs = [event_ms(lambda: bs.search(mem, lens))[0] for _ in range(args.reps)]
    ms = statistics.median(runs)
    lines = ["attention beam search: B=%d beam=%d (%d rows) T'=%d layers=%d D=%d H=%d FF=%d V=%d bf16, %d steps (max_len; eos suppressed), %d steps per graph"
             % (B, K, B * K, T, layers, D, H, FF, V, bs.steps, bs.steps_per_replay),
             "search (memory K|V projection, begin, %d replays, one host read per replay, the n-best read): median of %d runs %.2f ms (min %.2f, max %.2f) per batch, %.3f ms per step"
             % (bs.replays, args.reps, ms, min(runs), max(runs), ms / bs.steps)]
    # by kernel: one eager search under the library's profiling table
    eager = decoder.AttentionBeamSearch(dec, beam=K, max_len=steps, use_graph=False)
    eager.search(mem, lens)
    cfm.prof_reset()
    cfm.prof_enable(True)
    eager.search(mem, lens)
    torch.cuda.synchronize()
    table = cfm.prof_table()
    cfm.prof_enable(False)
    rows = [(name, r["calls"], r["ms"] * 1e3) for name, r in table.items()]
    total = sum(r[2] for r in rows)
    launches = sum(r[1] for r in rows)
    ran = eager.replays * eager.steps_per_replay                 # the steps launched: the last replay's steps past the end are idle but launched
    lines.append("one eager search of %d launched steps, by kernel (cfm profiling table): %d launches = %d memory projections before the loop + %.1f per step, %.2f ms of kernel time"
                 % (ran, launches, layers, (launches - layers) / ran, total / 1e3))
    for name, calls, us in sorted(rows, key=lambda r: -r[2]):
        lines.append("  %-24s %6d calls %10.1f us total %8.2f us each %5.1f %%" % (name, calls, us, us / max(calls, 1), 100.0 * us / max(total, 1e-9)))
    per = {name: (calls, us) for name, calls, us in rows}
    esz = 2
    mean_klen = (steps + 1) / 2.0
    mean_len = float(lens.float().mean())
    for name, keys, what, shared in (("dec_step_attn_self", mean_klen, "mean key count %.1f" % mean_klen, ""),
                                     ("dec_step_attn_cross", mean_len, "mean encoder length %.1f" % mean_len,
                                      "; the %d rows of an utterance share its %d x %d memory rows: %.2f MB unique" % (K, T, 2 * D, B * mean_len * 2 * D * esz / 1e6))):
        if name in per:
            calls, us = per[name]
            must = B * K * keys * 2 * D * esz                    # every row reads its keys and values once
            lines.append("%s: %.2f us per launch, must read %.2f MB (%s%s) -> %.0f GB/s" % (name, us / calls, must / 1e6, what, shared, must / (us / calls) / 1e3))
    gemm_us = sum(us for name, calls, us in rows if name.startswith("gemm"))
    lines.append("cfm_gemm launches (M = %d rows; the %d memory projections included): %.1f %% of the kernel time" % (B * K, layers, 100.0 * gemm_us / max(total, 1e-9)))
    # the baseline
    bt = baseline_steps(cfm, dec, mem, lens, K, args.baseline_steps, V - 1)
    lines.append("baseline (rows_forward over all whole prefixes per step + torch log-softmax / top-k + one host read), steps 1..%d: %.2f ms per step at mean prefix length %.1f "
                 "(first %.2f, last %.2f) -- against %.3f ms per step of the search"
                 % (len(bt), statistics.mean(bt[1:]), (len(bt) + 2) / 2.0, bt[1], bt[-1], ms / bs.steps))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
