"""Streaming ASR end to end at config 5 (64 streams, chunk 16, left context 4 chunks, the config-2 encoder, bf16) with the config-4 head
(V = 5002, synth.greedy_joint_ shaped), one MI355X, one process:

  (a) the composition the two halves allowed before: encoder.StreamingBatch.step, then greedy.BatchedGreedySearch.search(..., token, state)
      once per chunk (one frame decision per decoding step);
  (b) transducer.StreamingRecognizer.step (chunk-lookahead decoding, csrc/greedy.hip cfm_greedy_chunk_step).

STEPS steps each (default 200) after WARMUP, REPS alternating repetitions, HIP events around whole steps; the input is synthetic fbank, the
emission rate it produces is reported as tokens per encoder frame (BLANK_BIAS=x raises the blank's bias: fewer emissions; the plain
shaped head emits about one symbol per frame, several times what speech does at 40 ms frames).  KERNEL_TABLE=1 adds the per-kernel table of (b)'s decoder from
eager launches; for the device-side view run the script under a kernel trace with KERNEL_TABLE=0."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "conformer-pytorch-lightning_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import cfm, bench, synth
import encoder as enc_mod, greedy, joint, predictor, transducer

B, chunk, left = int(os.environ.get("STREAMS", "64")), 16, 4
STEPS, WARMUP, REPS = int(os.environ.get("STEPS", "200")), int(os.environ.get("WARMUP", "40")), int(os.environ.get("REPS", "3"))
N_STEPS = int(os.environ.get("N_STEPS", "4"))
BLANK_BIAS = float(os.environ.get("BLANK_BIAS", "0"))       # added to the blank's bias on top of synth.greedy_joint_: lowers the emission rate
cfm.set_precision("bf16")
dev = torch.device("cuda", 0)
enc = bench.build_encoder(dev)
V, D = 5002, enc.encoder_dim
pr = predictor.RNNPredictor(V, 256, 512, 256, 0.1, 2).eval()
jn = joint.TransducerJoint(V, D, 512, 512).eval()
synth.load_synth_(pr, 53); synth.load_synth_(jn, 54); synth.greedy_joint_(jn, V)
with torch.no_grad():
    jn.ffn_out.bias[0] += BLANK_BIAS
pr, jn = pr.to(dev), jn.to(dev)
window, hop = (chunk - 1) * 4 + 7, 4 * chunk
total = WARMUP + STEPS
x = torch.from_numpy(np.random.RandomState(5).standard_normal((B, window + total * hop, 80)).astype(np.float32)).to(dev)


def run_a():
    sb = enc_mod.StreamingBatch(enc, B, chunk, left)
    gs = greedy.BatchedGreedySearch(pr, jn, n_steps=N_STEPS, steps_per_replay=8, fused=True)
    tok = st = None
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(total)]
    ntok = 0
    with torch.no_grad():
        for s in range(total):
            win = x[:, s * hop: s * hop + window].contiguous()
            ev[s][0].record()
            y = sb.step(win)
            hyps, (tok, st) = gs.search(y, [chunk] * B, token=tok, state=st)
            ev[s][1].record()
            ntok += sum(len(h) for h in hyps) if s >= WARMUP else 0
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) for a, b in ev[WARMUP:]), ntok, None


def run_b():
    rec = transducer.StreamingRecognizer(enc, pr, jn, B, chunk, left, n_steps=N_STEPS)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(total)]
    ntok = 0
    for s in range(total):
        win = x[:, s * hop: s * hop + window].contiguous()
        ev[s][0].record()
        new = rec.step(win)
        ev[s][1].record()
        if s == WARMUP:
            rec.decoder.total_steps = rec.decoder.total_replays = 0
        ntok += sum(len(h) for h in new) if s >= WARMUP else 0
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) for a, b in ev[WARMUP:]), ntok, (rec.decoder.total_steps / max(1, STEPS - 1), rec.decoder.total_replays / max(1, STEPS - 1))


ONLY = os.environ.get("ONLY", "ab")                         # "b": the recogniser alone (a kernel trace of it)
res = {"a": [], "b": []}
for rep in range(REPS):
    for name, fn in (("a", run_a), ("b", run_b)):
        if name not in ONLY:
            continue
        ms, ntok, extra = fn()
        med, mean = ms[len(ms) // 2], sum(ms) / len(ms)
        res[name].append(med)
        print("rep %d (%s) %-44s median %.3f ms  mean %.3f ms per step; %.3f tokens per encoder frame%s" %
              (rep, name, "StreamingBatch.step + search() per chunk" if name == "a" else "StreamingRecognizer.step", med, mean, ntok / (STEPS * B * chunk),
               "" if extra is None else "; %.2f lookahead steps, %.2f replays per chunk" % extra))
if ONLY != "ab":
    sys.exit(0)
sa, sb_ = max(res["a"]) - min(res["a"]), max(res["b"]) - min(res["b"])
ma, mb = sorted(res["a"])[REPS // 2], sorted(res["b"])[REPS // 2]
print("streams %d chunk %d n_steps %d blank bias +%.2f, %d steps x %d repetitions: (a) %.3f ms (spread %.3f), (b) %.3f ms (spread %.3f) per step: (a) - (b) = %.3f ms, %.2fx" %
      (B, chunk, N_STEPS, BLANK_BIAS, STEPS, REPS, ma, sa, mb, sb_, ma - mb, ma / mb))

if os.environ.get("KERNEL_TABLE", "1") != "0":
    sb = enc_mod.StreamingBatch(enc, B, chunk, left)
    cg = greedy.ChunkGreedySearch(pr, jn, B, chunk, n_steps=N_STEPS, use_graph=False)
    n = 20
    with torch.no_grad():
        for s in range(8 + n):
            if s == 8:
                torch.cuda.synchronize(); cfm.prof_reset(); cfm.prof_enable(True); cg.total_steps = 0
            y = sb.step(x[:, s * hop: s * hop + window].contiguous())
            cg.decode(y)
        torch.cuda.synchronize(); cfm.prof_enable(False)
    tab = {k: e for k, e in cfm.prof_table().items() if k.startswith("greedy")}
    tot = sum(e["ms"] for e in tab.values())
    print("ChunkGreedySearch.decode, kernels (eager, %d chunks, %.2f lookahead steps per chunk): device time %.3f ms per chunk" % (n, cg.total_steps / n, tot / n))
    for k, e in sorted(tab.items(), key=lambda kv: -kv[1]["ms"]):
        print("  %-28s calls/chunk %5.1f  avg %7.2f us  share %5.1f%%" % (k, e["calls"] / n, e["ms"] / e["calls"] * 1e3, 100 * e["ms"] / tot))
