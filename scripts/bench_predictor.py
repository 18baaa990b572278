#!/usr/bin/env python
"""Forward + backward of the RNN-T predictor alone (embedding -> 2 x LSTM(256) -> projection, train mode), `fused=False` (nn.LSTM: MIOpen)
against `fused=True` (csrc/lstm.hip), at the label matrices the training step hands it:
  config3   the accumulation window of BASELINE config 3: (sum B_g, Umax + 1) of two trainer.librispeech_shaped_batch micro-batches, seed 1234
  config4   B 16, U + 1 = 41
Each repetition times both paths one after the other (alternated, same process, same inputs) with HIP events around forward + backward;
the medians, the 10 % / 90 % quantiles and the launch counts of one forward + backward go to profiles/predictor_lstm.json.

    python scripts/bench_predictor.py [--reps 200] [--warmup 30] [--out profiles/predictor_lstm.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "conformer-pytorch-lightning_amd")]


def window_shape():
    import trainer as T
    rs = np.random.RandomState(1234)
    shapes = [T.librispeech_shaped_batch(rs)[2].shape for _ in range(2)]
    return sum(s[0] for s in shapes), max(s[1] for s in shapes) + 1


def launches(fn):
    """Kernel launches of one call, from the profiler's device events."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "emcpy" not in e.name and "emset" not in e.name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predictor_lstm.json"))
    a = ap.parse_args()
    import predictor
    V, E, P, H, L = 5002, 256, 256, 256, 2
    torch.manual_seed(0)
    stock = predictor.RNNPredictor(V, E, P, H, 0.1, L, dropout=0.1).cuda().train()
    fused = predictor.RNNPredictor(V, E, P, H, 0.1, L, dropout=0.1, fused=True).cuda().train()
    fused.load_state_dict(stock.state_dict())
    result = {"predictor": {"vocab": V, "embed": E, "output": P, "hidden": H, "layers": L, "dropout": 0.1}, "reps": a.reps, "warmup": a.warmup, "shapes": {}}
    for name, (B, U1) in (("config3_window", window_shape()), ("config4", (16, 41))):
        labels = torch.randint(0, V, (B, U1), device="cuda")
        dout = torch.randn(B, U1, P, device="cuda")

        def step(mod):
            mod.zero_grad(set_to_none=True)
            mod(labels).backward(dout)

        paths = {"stock": lambda: step(stock), "fused": lambda: step(fused)}
        for _ in range(a.warmup):
            for fn in paths.values():
                fn()
        times = {k: [] for k in paths}
        for _ in range(a.reps):
            for k, fn in paths.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3)
        entry = {"B": B, "U1": U1}
        for k, v in times.items():
            q = np.percentile(v, [10, 50, 90])
            entry[k] = {"median_us": round(float(q[1]), 1), "p10_us": round(float(q[0]), 1), "p90_us": round(float(q[2]), 1), "launches": launches(paths[k])}
        entry["fused_over_stock"] = round(entry["fused"]["median_us"] / entry["stock"]["median_us"], 3)
        result["shapes"][name] = entry
        print(name, json.dumps(entry))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
