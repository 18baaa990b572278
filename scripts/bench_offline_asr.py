"""Offline ASR end to end: 32 whole utterances of randint(600, 1001) frames (sorted, longest first), the config-2 encoder in bf16 with the
config-4 head (V = 5002, synth.greedy_joint_ shaped), one MI355X, one process:

  (a) transducer.OfflineRecognizer.recognize on the ragged batch (ConformerEncoder.forward_utterances + BatchedGreedySearch.search); its
      encoder half is also timed alone;
  (b) the batch-1 loop, the only way to the same tokens before: ConformerEncoder.forward_chunk over the whole utterance + search, once per
      utterance; its encoder calls are also timed alone;
  (c) ConformerEncoder.forward on the same batch: the same rows and launches as (a)'s encoder half, the training path's semantics -- the cost
      yardstick for that half.

REPS alternating repetitions after a warm-up pass of every shape; whole passes are timed with a host clock around work that ends in a device
synchronise (the searches read their results on the host), the encoder halves with HIP events.  On a tree without OfflineRecognizer (the parent
commit) only (b) and (c) run.  BLANK_BIAS=x raises the blank's bias (fewer emissions); the emission rate is reported."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "conformer-pytorch-lightning_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import cfm, bench, synth
import greedy, joint, predictor, transducer

UTTS, REPS = int(os.environ.get("UTTS", "32")), int(os.environ.get("REPS", "3"))
N_STEPS = int(os.environ.get("N_STEPS", "4"))
BLANK_BIAS = float(os.environ.get("BLANK_BIAS", "0"))
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
rs = np.random.RandomState(7)
lens = sorted(rs.randint(600, 1001, UTTS).tolist(), reverse=True)
x = torch.from_numpy(rs.standard_normal((UTTS, lens[0], 80)).astype(np.float32)).to(dev)
lt = torch.tensor(lens, dtype=torch.int32, device=dev)
frames_out = sum((n - 3) // 4 for n in lens)
HAVE_A = hasattr(transducer, "OfflineRecognizer")
empty = torch.zeros((0, 0, 0, 0), device=dev)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    with torch.no_grad():
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


rec = transducer.OfflineRecognizer(enc, pr, jn, n_steps=N_STEPS) if HAVE_A else None
gs = greedy.BatchedGreedySearch(pr, jn, n_steps=N_STEPS)


def run_a():
    ms, hyps = timed(lambda: rec.recognize(x, lt))
    return ms, events(lambda: enc.forward_utterances(x, lt)), hyps


def loop_b():
    hyps = []
    with torch.no_grad():
        for b, n in enumerate(lens):
            y, _, _ = enc.forward_chunk(x[b:b + 1, :n], 0, -1, empty, empty)
            hyps.append(gs.search(y, [y.size(1)])[0][0])
    return hyps


def enc_b():
    for b, n in enumerate(lens):
        enc.forward_chunk(x[b:b + 1, :n], 0, -1, empty, empty)


def run_b():
    ms, hyps = timed(loop_b)
    return ms, events(enc_b), hyps


def run_c():
    ms = events(lambda: enc(x, lt))
    return ms, ms, None


cases = ([("a", "OfflineRecognizer.recognize", run_a)] if HAVE_A else []) + [("b", "forward_chunk + search per utterance", run_b), ("c", "encoder.forward (yardstick)", run_c)]
for _, _, fn in cases:                                       # warm-up: every shape of the timed passes (packs, scratch arena, captured graphs)
    fn()
res = {k: [] for k, _, _ in cases}
hyps = {}
for rep in range(REPS):
    for k, name, fn in cases:
        ms, ms_enc, h = fn()
        res[k].append((ms, ms_enc))
        hyps[k] = h
        print("rep %d (%s) %-40s %9.2f ms per pass, encoder half %8.2f ms" % (rep, k, name, ms, ms_enc), flush=True)
med = {k: (sorted(v[0] for v in r)[REPS // 2], sorted(v[1] for v in r)[REPS // 2], max(v[0] for v in r) - min(v[0] for v in r)) for k, r in res.items()}
print("%d utterances, %d..%d frames (%d encoder frames), n_steps %d, blank bias +%.2f, %d repetitions, medians:" % (UTTS, lens[-1], lens[0], frames_out, N_STEPS, BLANK_BIAS, REPS))
for k, name, _ in cases:
    ms, ms_enc, spread = med[k]
    print("  (%s) %-40s %9.2f ms (spread %.2f) = %8.1f utterances/s; encoder half %8.2f ms" % (k, name, ms, spread, UTTS / ms * 1e3, ms_enc))
if HAVE_A:
    ntok = sum(len(h) for h in hyps["a"])
    same = sum(ha == hb for ha, hb in zip(hyps["a"], hyps["b"]))
    print("  (b) / (a) = %.1fx; (a)'s encoder half / (c) = %.3f; %.3f tokens per encoder frame; %d of %d utterances with the same tokens from (a) and (b) (bf16: close decisions may differ)"
          % (med["b"][0] / med["a"][0], med["a"][1] / med["c"][1], ntok / frames_out, same, UTTS))
