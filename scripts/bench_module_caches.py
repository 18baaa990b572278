"""Host cost of the three per-step module-cache paths, no GPU: a hit of ConformerEncoderLayer._weights, the graph watch, a flat-path hit of
packing.pack_stack_train (trivial plan / the real valid_for).  Median over 1000 calls, five times each, in microseconds.

    python scripts/bench_module_caches.py CHECKOUT      (CHECKOUT: this tree or another commit's; profiles/r13_module_caches.txt alternates two)
"""
import statistics
import sys
import time
import types

root = sys.argv[1]
sys.path[:0] = [root, root + "/tests", root + "/conformer-pytorch-lightning_amd"]
import torch  # noqa: E402
import cfm  # noqa: E402
from cfm import packing  # noqa: E402
import encoder  # noqa: E402
import encoder_layer  # noqa: E402

torch.set_num_threads(1)


def med(f, n=1000):
    for _ in range(200):
        f()
    ts = []
    for _ in range(n):
        t = time.perf_counter_ns()
        f()
        ts.append(time.perf_counter_ns() - t)
    return statistics.median(ts) / 1e3


prec = cfm.Precision("bf16")
packing.layer_weight_struct = lambda l, p: (object(), ())
layer = encoder_layer.ConformerEncoderLayer(256, 15, 0.1, 0.1, 2048, 4, True).eval()
layer._weights(prec)

enc = encoder.ConformerEncoder(input_dim=80, kernel_size=15, encoder_dim=256, dropout=0.1, attention_dropout=0.1, pos_enc_dropout=0.1, hidden_dim=2048,
                               num_heads=4, encoder_num_layers=12, cmvn=None, max_len=5000, use_relative=True).eval()
owner = types.SimpleNamespace(enc=enc)
watch = getattr(packing, "graph_watch", None) or encoder._weights_signature
watch(owner)


class TrivialPlan:
    def __init__(self, layers, prec, relative):
        pass

    def valid_for(self, layers, prec):
        return True

    def run(self):
        return ("packs",)


class WalkPlan(packing._StackPackPlan):                     # the real valid_for (blocks by identity + ~300 addresses)
    def __init__(self, layers, prec, relative):
        self.prec, self.layers = prec, list(layers)
        self.ptrs = tuple(t.data_ptr() for l in layers for t in l.parameters())

    def run(self):
        return ("packs",)


layers = list(enc.encoders)
res = {}
for rep in range(5):
    res.setdefault("a_layer_weights_hit", []).append(med(lambda: layer._weights(prec)))
    res.setdefault("b_graph_watch", []).append(med(lambda: watch(owner)))
    for name, plan in (("c_flat_hit_trivial_plan", TrivialPlan), ("c_flat_hit_real_valid_for", WalkPlan)):
        packing._StackPackPlan = plan
        o = types.SimpleNamespace()
        packing.pack_stack_train(o, layers, prec, True, flat=True)
        res.setdefault(name, []).append(med(lambda: packing.pack_stack_train(o, layers, prec, True, flat=True)))
for k, v in res.items():
    print("%-28s median of 5 medians %8.2f us   (%s)" % (k, statistics.median(v), " ".join("%.2f" % x for x in v)))
