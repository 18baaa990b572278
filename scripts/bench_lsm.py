"""The label-smoothing loss at the recipe's output step: 32 utterances x 31 decoder positions (992 rows), D = 256, V = 5002, bf16.
`iters` back-to-back calls of each form after a warm-up, so that a kernel trace of this script holds each kernel many times:

    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_lsm.py

  fused     cfm_lsm_loss, cfm_lsm_grad (the logits never stored)
  unfused   cfm.gemm to f32 logits, then the two kernels' logits forms (the grad writes bf16 as the fused one does)
It also prints HIP-event times, microseconds per call, median (min .. max) of `reps` blocks."""
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
    import cfm
    from cfm import packing
    cfm.set_precision("bf16")
    prec = cfm.get_precision()
    dev = torch.device("cuda")
    B, Lc, D, V, s = 32, 31, 256, 5002, 0.1
    M = B * Lc
    g = torch.Generator().manual_seed(1)
    lin = torch.nn.Linear(D, V).to(dev)
    pk = packing.pack_vocab_train(lin, prec)
    xn = torch.randn(M, D, generator=g).to(dev).to(prec.act_dtype)
    tg = torch.randint(0, V, (M,), generator=g).to(torch.int32)
    tg[torch.rand(M, generator=g) < 0.2] = -1
    tg = tg.to(dev)
    gm = torch.full((M,), 1.0 / B, device=dev)
    print("label-smoothing loss: %d rows, D=%d V=%d (Vk=%d) bf16; microseconds, median (min .. max)" % (M, D, V, pk.Vk))

    def say(name, t):
        print("%-52s %9.1f  (%.1f .. %.1f)" % (name, t[0], t[1], t[2]), flush=True)

    loss, lse = cfm.lsm_loss(xn, pk.w, pk.b, tg, V, s)
    dz = torch.empty((M, pk.Vk), dtype=prec.act_dtype, device=dev)
    logits = torch.empty((M, pk.Vk), device=dev)
    say("fused   cfm_lsm_loss", timed(lambda: cfm.lsm_loss(xn, pk.w, pk.b, tg, V, s)))
    say("fused   cfm_lsm_grad", timed(lambda: cfm.lsm_grad(xn, pk.w, pk.b, tg, V, s, lse, gm, out=dz)))
    say("unfused cfm.gemm -> f32 logits", timed(lambda: cfm.gemm(xn, pk.w, bias=pk.b, out=logits)))
    say("unfused cfm_lsm_loss, logits form", timed(lambda: cfm.lsm_loss(None, None, None, tg, V, s, logits=logits)))
    say("unfused cfm_lsm_grad, logits form", timed(lambda: cfm.lsm_grad(None, None, None, tg, V, s, lse, gm, logits=logits, out=dz)))
    say("cfm_lsm_reduce", timed(lambda: cfm.lsm_reduce(loss, tg, B)))


if __name__ == "__main__":
    main()
