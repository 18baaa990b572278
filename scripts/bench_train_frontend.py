"""Time of the training front end's augmentation stages (augment.py), recorded in DESIGN.md section 7:

  speed perturbation   one cfm_resample_group launch over a batch that mixes the speeds 0.9 / 1.0 / 1.1, against the route the single-pair kernel
                       allows: the items grouped by speed on the host, one resample.Resampler call per speed on the gathered rows, the results
                       scattered back into the padded batch
  the whole step       augment.TrainFrontend (speed perturbation, fbank with dither, SpecAugment) on the same batch, with the launches it makes

The batch is one dynamic batch of the recipe (trainer.librispeech_shaped_batch: frames ~ U{200..1650} while B * T_max <= 8000) at 160 samples per
frame, int16.  The two speed-perturbation routes are first compared bit for bit, then timed in alternating rounds (hipEvent pairs around `iters`
back-to-back calls on one stream, after a warm-up); the figure is the median round, the spread the extremes.

    python scripts/bench_train_frontend.py [--iters 100] [--rounds 7]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "conformer-pytorch-lightning_amd")]


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters          # microseconds


def rounds_of(fns, iters, rounds):
    """Alternate the candidates round by round -> per candidate (median, min, max) microseconds per call."""
    for fn in fns:
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(rounds):
        for t, fn in zip(times, fns):
            t.append(timed(fn, iters))
    return [(statistics.median(t), min(t), max(t)) for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_frontend: no GPU; nothing is measured without one")
    import augment
    import cfm
    import resample
    import trainer
    dev = torch.device("cuda")
    _, frames, _, _ = trainer.librispeech_shaped_batch(np.random.RandomState(1234))
    lengths = [int(f) * 160 for f in frames]
    B, N = len(lengths), max(lengths)
    x = (torch.randn((B, N), device=dev) * 3000).to(torch.int16)
    lens = torch.tensor(lengths, dtype=torch.int32, device=dev)
    sp = augment.SpeedPerturb()
    choice = [b % 3 for b in range(B)]
    cap = max(sp.num_samples(N, k) for k in set(choice))
    print("training front end, %s: %d utterances, %d .. %d samples (%.1f MB int16 in, %.1f MB f32 out), speeds %s"
          % (torch.cuda.get_device_name(0), B, min(lengths), N, B * N * 2 / 1e6, B * cap * 4 / 1e6, [sp.speeds[k] for k in choice]))

    # the grouped launch alone: operands in place
    bank = torch.tensor(choice, dtype=torch.int32, device=dev)
    out, out_lens = torch.empty((B, cap), dtype=torch.float32, device=dev), torch.empty((B,), dtype=torch.int32, device=dev)
    tables = sp.tables(dev)
    def launch():
        cfm.resample_group(x, lens, bank, tables, sp.banks, out, out_lens)

    # the route of the single-pair kernel: per speed gather, convert, scatter (index vectors in place, as the bank vector above)
    singles = [resample.Resampler(orig) for orig, _ in sp.pairs]
    index = [torch.tensor([b for b in range(B) if choice[b] == k], dtype=torch.long, device=dev) for k in range(3)]
    columns, zero = torch.arange(N, device=dev)[None, :], torch.zeros((), dtype=torch.float32, device=dev)
    def by_speed():
        y = torch.zeros((B, cap), dtype=torch.float32, device=dev)
        y_lens = torch.empty((B,), dtype=torch.int32, device=dev)
        for k, idx in enumerate(index):
            if idx.numel() == 0:
                continue
            yk, lk = singles[k](x.index_select(0, idx), lens.index_select(0, idx))
            if singles[k].o == singles[k].n:         # equal rates hand the rows back as they are: clear what lies behind each item's samples
                yk = torch.where(columns < lk[:, None], yk.to(torch.float32), zero)
            y[idx, :yk.shape[1]] = yk
            y_lens[idx] = lk
        return y, y_lens

    def whole():                                     # SpeedPerturb.forward: output allocation and the bank vector's upload included
        return sp(x, lens, choice)

    launch()
    y, y_lens = by_speed()
    z, z_lens = whole()
    torch.cuda.synchronize()
    same = True
    for name, (v, v_lens) in (("by speed", (y, y_lens)), ("SpeedPerturb.forward", (z, z_lens))):
        diff = out.view(torch.int32) != v.view(torch.int32)
        if bool(diff.any()) or not torch.equal(out_lens, v_lens):
            same = False
            where = torch.nonzero(diff)
            print("  %s differs from the grouped launch: lengths %s / %s, %d samples, first at %s: %r / %r" % (
                name, out_lens.tolist(), v_lens.tolist(), int(diff.sum()), where[0].tolist() if len(where) else None,
                float(out[tuple(where[0])]) if len(where) else None, float(v[tuple(where[0])]) if len(where) else None))
    print("  the three routes agree bit for bit: %s" % same)
    if not same:
        raise SystemExit("bench_train_frontend: the routes differ; no timing")
    names = ("cfm_resample_group, operands in place", "SpeedPerturb.forward (allocation + bank upload + launch)", "three Resampler calls on host-grouped items + gathers / scatters")
    for name, (med, lo, hi) in zip(names, rounds_of((launch, whole, by_speed), args.iters, args.rounds)):
        print("  %-68s %8.1f us  (%.1f .. %.1f over %d rounds of %d)" % (name, med, lo, hi, args.rounds, args.iters))

    front = augment.TrainFrontend(speed=sp, spec=augment.SpecAugment())
    step = [0]
    def train_step():
        step[0] += 1
        return front(x, lens, step[0], choice=choice)
    feats, feats_length = train_step()
    torch.cuda.synchronize()
    cfm.prof_reset()
    cfm.prof_enable(True)
    train_step()
    table = cfm.prof_table()
    cfm.prof_enable(False)
    cfm.prof_reset()
    (med, lo, hi), = rounds_of((train_step,), args.iters, args.rounds)
    print("  TrainFrontend step -> feats %s: %d library launches (%s) + one upload of %d int32   %8.1f us  (%.1f .. %.1f)"
          % (tuple(feats.shape), sum(v["calls"] for v in table.values()), ", ".join("%s %.1f us" % (k, v["ms"] * 1e3) for k, v in sorted(table.items())), B, med, lo, hi))


if __name__ == "__main__":
    main()
