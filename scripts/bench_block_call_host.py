"""Host cost of the eager encoder calls (no graph replay): wall time per call over CALLS back-to-back calls, synchronised once at the end, REPS times;
prints every repetition and the median.  (a) enc(x, lens) at the bench.py config-2 shape, 32 x 1000 frames; (b) one StreamingBatch(graph=False)
step at 64 streams, chunk 16, left context 4 chunks.  For comparing two trees in alternating processes (profiles/r19_block_call_host.txt)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "conformer-pytorch-lightning_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import cfm, bench
import encoder as enc_mod

CALLS, REPS = int(os.environ.get("CALLS", "50")), int(os.environ.get("REPS", "5"))
cfm.set_precision("bf16")
dev = torch.device("cuda", 0)
enc = bench.build_encoder(dev)


def measure(name, call, warmup=10):
    with torch.no_grad():
        for _ in range(warmup):
            call()
        reps = []
        for _ in range(REPS):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(CALLS):
                call()
            torch.cuda.synchronize(); reps.append(1e3 * (time.perf_counter() - t0) / CALLS)
    print("%s: %s ms per call, median %.4f (%d calls per repetition)" % (name, " ".join("%.4f" % r for r in reps), sorted(reps)[len(reps) // 2], CALLS), flush=True)


x, lens = bench.forward_inputs(32, 1000, 0, dev)
measure("(a) enc(x, lens) 32 x 1000", lambda: enc(x, lens))
sb = enc_mod.StreamingBatch(enc, 64, 16, 4, graph=False)
win = torch.from_numpy(np.random.RandomState(5).standard_normal((64, sb.window, 80)).astype(np.float32)).to(dev)
sb.input_buffer(80).copy_(win)
measure("(b) StreamingBatch(graph=False) step, 64 streams, chunk 16", lambda: sb.step_resident())
