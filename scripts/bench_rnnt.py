"""Fused transducer joint + RNN-T loss, forward + backward, at the config-4 shape (B 16, T' 249, U 40, E = P = J = 512, V 5002, bf16 mode),
against the same step from stock torch ops on the GPU (F.linear, tanh, log_softmax, gather, the lattice recursion as a Python loop over
anti-diagonals, autograd).  Prints ONE JSON line: step times (device events around the whole step), peak memory of both, and the split over
the library's launches (cfm.prof_table, device events per launch) with the loss kernels' share of their HBM floor.
Usage (GPU box): python scripts/bench_rnnt.py [--steps N] [--warmup W] [--no-torch] [--no-split]
Kernel-level split for profiles/: rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_rnnt.py --steps 5 --no-torch --no-split"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "conformer-pytorch-lightning_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import cfm  # noqa: E402
import joint  # noqa: E402

HBM_TBS = 6.3                      # achievable HBM rate, TB/s (MI355X)
B, T, U, E, P, J, V = 16, 249, 40, 512, 512, 512, 5002
NEG = -1e30


def torch_step(jn, xe, xp, targets, tl, ul):
    e = F.linear(xe, jn.enc_ffn.weight, jn.enc_ffn.bias)
    p = F.linear(xp, jn.pred_ffn.weight, jn.pred_ffn.bias)
    logits = F.linear(torch.tanh(e.unsqueeze(2) + p.unsqueeze(1)), jn.ffn_out.weight, jn.ffn_out.bias)
    lp = torch.log_softmax(logits, -1)
    del logits
    lb = lp[..., 0]
    ll = torch.cat([lp[:, :, :U].gather(3, targets.long()[:, None, :, None].expand(B, T, U, 1)).squeeze(3), lp.new_full((B, T, 1), NEG)], 2)
    del lp
    u = torch.arange(U + 1, device=xe.device)
    lbf, llf = lb.reshape(B, -1), ll.reshape(B, -1)
    prev = torch.where(u == 0, 0.0, NEG).to(lb.dtype).expand(B, U + 1)
    diags = [prev]
    for d in range(1, T + U):
        t = d - u
        here = (t >= 0) & (t < T)
        up = prev + torch.where((t >= 1) & here, lbf.gather(1, ((t - 1).clamp(0, T - 1) * (U + 1) + u).expand(B, -1)), NEG)
        left = torch.cat([lb.new_full((B, 1), NEG), prev[:, :-1]], 1) + \
            torch.where((u >= 1) & here, llf.gather(1, (t.clamp(0, T - 1) * (U + 1) + (u - 1).clamp(min=0)).expand(B, -1)), NEG)
        prev = torch.where(here, torch.logaddexp(up, left), NEG)
        diags.append(prev)
    A = torch.stack(diags)
    bi = torch.arange(B, device=xe.device)
    loss = -(A[tl.long() - 1 + ul.long(), bi, ul.long()] + lb[bi, tl.long() - 1, ul.long()]).mean()
    loss.backward()
    return loss.detach()


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(steps):
        out = fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / steps, (torch.cuda.max_memory_allocated() - base) / 1e9, float(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-split", action="store_true")
    a = ap.parse_args()
    torch.manual_seed(0)
    dev = "cuda"
    cfm.set_precision("bf16")
    jn = joint.TransducerJoint(V, E, P, J).to(dev).train()
    xe = torch.randn(B, T, E, device=dev, requires_grad=True)
    xp = torch.randn(B, U + 1, P, device=dev, requires_grad=True)
    targets = torch.randint(1, V, (B, U), device=dev, dtype=torch.int32)
    tl = torch.full((B,), T, dtype=torch.int32, device=dev)
    ul = torch.full((B,), U, dtype=torch.int32, device=dev)

    def fused():
        xe.grad = xp.grad = None
        jn.zero_grad(set_to_none=True)
        loss = jn.rnnt_loss(xe, xp, targets, tl, ul)
        loss.backward()
        return loss.detach()

    res = {"metric": "rnnt_joint_loss_fwd_bwd", "shape": dict(B=B, T=T, U=U, E=E, P=P, J=J, V=V), "precision": "bf16"}
    res["fused_ms"], res["fused_peak_gb"], res["fused_loss"] = timed(fused, a.steps, a.warmup)
    rows = B * T * (U + 1)
    logits_gb = rows * (V + 6) * 4 / 1e9                              # the f32 logits buffer (V padded to 5008)
    res["logits_gb"] = round(logits_gb, 3)
    if not a.no_split:
        cfm.prof_reset()
        cfm.prof_enable(True)
        for _ in range(a.steps):
            fused()
        torch.cuda.synchronize()
        cfm.prof_enable(False)
        tab = cfm.prof_table()
        res["split_us"] = {k: round(v["ms"] * 1e3 / a.steps, 1) for k, v in sorted(tab.items())}          # per step, all calls of that name
        floor_us = {"rnnt_rows": rows * V * 4 / HBM_TBS / 1e6,                              # one read of the f32 logits
                    "rnnt_grad": rows * (V * 4 + (V + 6) * 2) / HBM_TBS / 1e6}              # read f32, write the bf16 gradient in place
        res["hbm_floor_us"] = {k: round(v, 1) for k, v in floor_us.items()}
        res["share_of_floor"] = {k: round(floor_us[k] / res["split_us"][k], 3) for k in floor_us if k in res["split_us"]}
    if not a.no_torch:
        jt = joint.TransducerJoint(V, E, P, J).to(dev)
        jt.load_state_dict(jn.state_dict())
        xe2, xp2 = xe.detach().clone().requires_grad_(True), xp.detach().clone().requires_grad_(True)
        res["torch_ms"], res["torch_peak_gb"], res["torch_loss"] = timed(lambda: torch_step(jt, xe2, xp2, targets, tl, ul), max(2, a.steps // 3), 1)
    for k in ("fused_ms", "torch_ms", "fused_peak_gb", "torch_peak_gb"):
        if k in res:
            res[k] = round(res[k], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
