"""The reference's full training objective (0.2 CTC + 0.8 RNN-T, train.sh) at BASELINE config 3's shapes: the config-2 encoder, V 5002, the
train.sh predictor (2 x 256 LSTM, embed 256, dim 256), join 512, accum_grad 2, clip 4, Adam, bf16, LibriSpeech-shaped micro-batches seeded as
bench.build_train_job (1234).  Prints ONE JSON line with ms per optimizer step and peak memory of
  (a) ctc_window      the CTC-only window (bench.py --mode train, config 3), for reference;
  (b) full_window     TransducerObjective.forward_window under DataParallelTrainer (packed lattice over the window);
  (c) full_loop       the micro-batch loop with the padded joint (TransducerObjective(packed=False).forward as loss_fn);
and the fused joint + loss forward + backward, packed vs padded, at the config-4 shape with uniform lengths and on one ragged micro-batch.
Usage (GPU box): python scripts/bench_transducer_train.py [--steps N] [--warmup W]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "conformer-pytorch-lightning_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import cfm  # noqa: E402

DEV = "cuda:0"


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return round(t0.elapsed_time(t1) / steps, 3), round((torch.cuda.max_memory_allocated() - base) / 1e9, 3)


def micro_batches(n=8):
    import trainer as T
    rs = np.random.RandomState(1234)
    out = []
    for _ in range(n):
        feats, lens, labels, label_lens = T.librispeech_shaped_batch(rs)
        out.append((None,) + tuple(torch.from_numpy(a).to(DEV) for a in (feats, lens, labels, label_lens)) + (None,))
    return out


def objective(packed):
    import decoder
    import encoder
    import joint
    import predictor
    import transducer
    torch.manual_seed(0)
    enc = encoder.ConformerEncoder(cmvn=None, **bench.CFG2).to(DEV).train()
    enc.set_precision("bf16")
    ctc = decoder.CTCDecoder(5002, bench.CFG2["encoder_dim"], 0.1).to(DEV).train()
    pr = predictor.RNNPredictor(5002, 256, 256, 256, 0.1, 2, dropout=0.1).to(DEV).train()
    jn = joint.TransducerJoint(5002, bench.CFG2["encoder_dim"], 256, 512).to(DEV).train()
    return transducer.TransducerObjective(enc, pr, jn, ctc, blank=0, ignore_id=-1, ctc_weight=0.2, transducer_weight=0.8, packed=packed)


def train_case(name, steps, warmup):
    import trainer as T
    if name == "ctc_window":
        _, _, tr, mbs, _ = bench.build_train_job(DEV, 0, "bf16")
        mbs = [(None,) + mb + (None,) for mb in mbs]
        run = lambda pair: tr.step([mb[1:5] for mb in pair])
    else:
        obj = objective(packed=name == "full_window")
        mods = [obj.encoder, obj.ctc, obj.predictor, obj.joint]
        tr = T.DataParallelTrainer(mods, lambda mb: obj(mb)["loss"], lr=1e-3, warmup_steps=25000, accum_grad=2, grad_clip=4.0,
                                   window_loss_fn=obj.forward_window if name == "full_window" else None)
        mbs = micro_batches()
        run = tr.step
    state = {"i": 0}

    def step():
        i = state["i"]
        state["loss"] = run([mbs[(2 * i) % len(mbs)], mbs[(2 * i + 1) % len(mbs)]])
        state["i"] = i + 1

    ms, peak = timed(step, steps, warmup)
    out = {"ms_per_step": ms, "peak_gb": peak, "loss": round(float(state["loss"]), 4)}
    del tr
    torch.cuda.empty_cache()
    return out


def joint_case(B, T, U, tl, ul, steps, warmup):
    import joint
    torch.manual_seed(1)
    jn = joint.TransducerJoint(5002, 512, 512, 512).to(DEV).train()
    jn.precision = "bf16"
    xe = torch.randn(B, T, 512, device=DEV, requires_grad=True)
    xp = torch.randn(B, U + 1, 512, device=DEV, requires_grad=True)
    targets = torch.randint(1, 5002, (B, U), dtype=torch.int32, device=DEV)
    tl, ul = torch.tensor(tl, device=DEV), torch.tensor(ul, device=DEV)
    out = {}
    for packed in (False, True):
        def step():
            xe.grad = xp.grad = None
            jn.rnnt_loss(xe, xp, targets, tl, ul, packed=packed).backward()
        ms, peak = timed(step, steps, warmup)
        out["packed" if packed else "padded"] = {"ms": ms, "peak_gb": peak}
    out["cells"] = round(float((tl * (ul + 1)).sum()) / (B * T * (U + 1)), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    cfm.set_precision("bf16")
    res = {"config": "BASELINE config 3 shapes, full objective (0.2 CTC + 0.8 RNN-T), bf16"}
    for name in ("ctc_window", "full_window", "full_loop"):
        res[name] = train_case(name, a.steps, a.warmup)
    res["joint_config4_uniform"] = joint_case(16, 249, 40, [249] * 16, [40] * 16, a.steps, a.warmup)
    mb = micro_batches(1)[0]
    lens, label_lens = mb[2].cpu().numpy(), mb[4].cpu().numpy()
    t_sub = ((lens.astype(np.int64) - 1) // 2 - 1) // 2
    res["joint_ragged_microbatch"] = joint_case(len(lens), int(t_sub.max()), int(label_lens.max()), t_sub.tolist(), label_lens.tolist(), a.steps, a.warmup)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
