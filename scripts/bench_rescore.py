"""Attention rescoring at the deployment shape: 32 utterances x 10 hypotheses of about 30 tokens, T' = 249, 6 layers, D = 256, H = 4, FF = 2048,
V = 5002, bf16.  Timed by HIP events around `iters` back-to-back calls after a warm-up, median of `reps` such blocks.

  (a) the output step alone: cfm_token_logprob fused, against the unfused form (cfm.gemm to f32 logits, then the kernel's logits form) -- the
      baseline, since nothing scored hypotheses before;
  (b) a whole AttentionRescorer.scores call (device half, no host read), fused and unfused, and split by stage.

    python scripts/bench_rescore.py [--out profiles/NAME.txt]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "conformer-pytorch-lightning_amd")]


def timed(fn, iters=20, reps=7, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / iters)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import cfm
    import decoder
    cfm.set_precision("bf16")
    prec = cfm.get_precision()
    dev = torch.device("cuda")
    B, N, T, D, H, FF, V, layers = 32, 10, 249, 256, 4, 2048, 5002, 6
    torch.manual_seed(0)
    dec = decoder.BiTransformerDecoder(V, D, H, FF, layers, layers, 0.0, 0.0, 0.0, 0.0).eval().to(dev)
    g = torch.Generator().manual_seed(1)
    nlen = torch.randint(24, 31, (B, N), generator=g).to(torch.int32)
    Lmax = int(nlen.max())
    tokens = torch.randint(0, V - 1, (B, N, Lmax), generator=g).to(torch.int32).to(dev)
    score = (-torch.rand(B, N, generator=g) * 10).to(dev)
    nlen = nlen.to(dev)
    mem = torch.randn(B, T, D, generator=g).to(dev)
    lens = torch.randint(200, T + 1, (B,), generator=g).to(torch.int32).to(dev)
    Lc, M = Lmax + 1, B * N * (Lmax + 1)
    lines = ["rescoring: B=%d N=%d Lmax=%d (Lc=%d, %d decoder rows) T'=%d layers=%d D=%d H=%d FF=%d V=%d bf16; microseconds, median (min .. max)"
             % (B, N, Lmax, Lc, M, T, layers, D, H, FF, V)]

    def say(name, t):
        lines.append("%-58s %9.1f  (%.1f .. %.1f)" % (name, t[0], t[1], t[2]))
        print(lines[-1], flush=True)

    # (a) the output step alone
    pk = dec.left_decoder._output_pack(prec)
    xn = torch.randn(M, D, generator=g).to(dev).to(prec.act_dtype)
    tg = cfm.rescore_prep(tokens, nlen, score, dec.left_decoder.embed[0].weight.detach(), dec.left_decoder.position_table(Lc), V - 1, V - 1)[1].view(-1)
    out = torch.empty(M, device=dev)
    say("(a) cfm_token_logprob fused", timed(lambda: cfm.token_logprob(xn, pk.w, pk.b, tg, V, out=out)))
    logits = torch.empty((M, pk.Vp), device=dev)
    say("(a) unfused: cfm.gemm -> f32 logits", timed(lambda: cfm.gemm(xn, pk.w, bias=pk.b, out=logits)))
    say("(a) unfused: logits form of cfm_token_logprob", timed(lambda: cfm.token_logprob(None, None, None, tg, V, logits=logits, out=out)))
    say("(a) unfused: both", timed(lambda: (cfm.gemm(xn, pk.w, bias=pk.b, out=logits), cfm.token_logprob(None, None, None, tg, V, logits=logits, out=out))))

    # (b) the whole device half
    for rw in (0.0, 0.3):
        for fused in (True, False):
            rs = decoder.AttentionRescorer(dec, reverse_weight=rw, fused=fused)
            say("(b) AttentionRescorer.scores rw=%.1f fused=%s" % (rw, fused), timed(lambda: rs.scores(mem, lens, tokens, nlen, score), iters=5, reps=5, warm=2))
    rs = decoder.AttentionRescorer(dec)
    memr = mem.reshape(B * T, D)
    mm = cfm.as_u8_mask(cfm.valid_mask(lens, T)).view(B, 1, T)
    left = dec.left_decoder
    E, pe = left.embed[0].weight.detach(), left.position_table(Lc)
    say("(b) stage: cfm_rescore_prep", timed(lambda: cfm.rescore_prep(tokens, nlen, score, E, pe, V - 1, V - 1)))
    x0, tg2, mask, _, _ = cfm.rescore_prep(tokens, nlen, score, E, pe, V - 1, V - 1)
    say("(b) stage: %d decoder layers + after_norm" % layers, timed(lambda: left.rows_forward(x0, (B * N, Lc), mask, memr, (B, N * Lc, T), mm, prec), iters=5, reps=5, warm=2))
    say("(b) stage: cfm_token_logprob fused", timed(lambda: cfm.token_logprob(xn, pk.w, pk.b, tg, V, out=out)))
    lp = cfm.token_logprob(xn, pk.w, pk.b, tg, V)
    say("(b) stage: cfm_rescore_combine", timed(lambda: cfm.rescore_combine(lp, nlen, score, 0.5)))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
