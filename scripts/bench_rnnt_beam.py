"""RNN-T beam search on the config-4 head (V = 5002, E = 256, H = 256, P = 512, J = 512, L = 2), T' = 249: beam 1, 4 and 8 at B = 64 // beam
utterances, ms per call, steps taken and us per step, with greedy.BatchedGreedySearch at B = 64 on the same encoder output beside it.

    python scripts/bench_rnnt_beam.py [--calls 5] [--warmup 2] [--max-symbols 4] [--out FILE]

Needs the GPU; times are host clocks around calls that end in the search's own device read.  One JSON line per row of the table."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "conformer-pytorch-lightning_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-symbols", type=int, default=4)
    ap.add_argument("--frames", type=int, default=249)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import greedy
    import greedy_ref as R
    if not torch.cuda.is_available():
        raise SystemExit("bench_rnnt_beam.py needs the GPU")
    dev = torch.device("cuda")
    pr, jn = R.modules(5002, 256, 256, 512, 512, 2, 53, enc_dim=512, shaped=True)
    with torch.no_grad():
        jn.ffn_out.weight.mul_(10.0)                       # a peaked posterior, as the tests' heads (tests/rnnt_beam_ref.py)
    pr, jn = pr.to(dev), jn.to(dev)
    T = a.frames
    enc = torch.from_numpy(np.random.RandomState(7).standard_normal((64, T, 512)).astype(np.float32)).to(dev)
    lens = [T] * 64
    rows = []

    def timed(name, B, fn, steps_of):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.calls):
            fn()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / a.calls
        steps = steps_of()
        rows.append(dict(search=name, B=B, frames=T, ms_per_call=round(ms, 3), steps=steps, us_per_step=round(ms * 1e3 / max(steps, 1), 2)))
        print(json.dumps(rows[-1]), flush=True)

    gs = greedy.BatchedGreedySearch(pr, jn, n_steps=a.max_symbols, steps_per_replay=32)
    out = {}
    timed("greedy", 64, lambda: out.__setitem__("g", gs.search(enc, lens)), lambda: T + max(len(h) for h in out["g"][0]))   # a step emits or advances
    for beam in (1, 4, 8):
        B = 64 // beam
        bs = greedy.BeamSearch(pr, jn, beam, max_symbols=a.max_symbols, steps_per_replay=32)
        timed("beam%d" % beam, B, lambda: bs.search(enc[:B], lens[:B]), lambda: bs.steps)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
