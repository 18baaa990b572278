"""Driver for a counter run of the chunk-lookahead vocabulary product (cfm_mtile_kernel<1>, csrc/greedy.hip) at known row counts: the
config-4 head with the blank raised so that no stream emits -- every decode is ONE lookahead step on 64 * lens rows.  ROWS_PER_STREAM
(default "16 8 2 1": 1024 / 512 / 128 / 64 rows), REPEAT decodes each, eager launches.  Run it under a kernel trace with counters, e.g.
    rocprofv3 --kernel-trace --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_BUSY_CYCLES SQ_WAVE_CYCLES --output-format csv -d out -- python scripts/pmc_chunk_product.py
the launches of cfm_mtile_kernel<1> then come in groups of REPEAT per row count, in the order given."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "conformer-pytorch-lightning_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import synth
import greedy, joint, predictor

B, chunk, V = 64, 16, 5002
REPEAT = int(os.environ.get("REPEAT", "5"))
dev = torch.device("cuda", 0)
pr = predictor.RNNPredictor(V, 256, 512, 256, 0.1, 2).eval()
jn = joint.TransducerJoint(V, 256, 512, 512).eval()
synth.load_synth_(pr, 53); synth.load_synth_(jn, 54); synth.greedy_joint_(jn, V)
with torch.no_grad():
    jn.ffn_out.bias[0] += 50.0
pr, jn = pr.to(dev), jn.to(dev)
cg = greedy.ChunkGreedySearch(pr, jn, B, chunk, n_steps=4, use_graph=False, steps_per_replay=1)
enc = torch.from_numpy(np.random.RandomState(5).standard_normal((B, chunk, 256)).astype(np.float32)).to(dev)
for l in [int(x) for x in os.environ.get("ROWS_PER_STREAM", "16 8 2 1").split()]:
    for _ in range(REPEAT):
        new = cg.decode(enc, [l] * B)
        assert cg.steps == 1 and not any(new)
torch.cuda.synchronize()
print("done")
