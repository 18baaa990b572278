"""CTC decoding at the config-2 shape (32 utterances x 249 encoder frames, D = 256, V = 5002), one MI355X, one process:

  greedy        decoder.CTCDecoder.greedy_search            (projection, cfm_ctc_topk k = 1, cfm_ctc_greedy, one host read)
  beam          decoder.CTCDecoder.prefix_beam_search(10)   (projection, cfm_ctc_topk k = 10, cfm_ctc_prefix_beam, one host read)
  torch_greedy  the same head with stock torch ops on the device: linear, log_softmax, argmax, then the collapse as a host loop
  torch_beam    linear, log_softmax, topk(10) on the device, then the float64 restatement's loop on the host (tests/ctc_decode_ref.py)

HIP events around whole calls (host work included: that is what a caller waits for), WARMUP calls first, the median of REPS; the device-only
part of the two torch paths (up to the copy to the host) is reported too.  Synthetic encoder output ~ N(0, 1), synthetic head with the blank's
bias raised so that about a third of the frames emit; ragged lengths 249 .. 125.  One JSON line, no threshold."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "conformer-pytorch-lightning_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import cfm, synth, decoder
import ctc_decode_ref as ref

B, T, D, V, BEAM = 32, 249, 256, 5002, 10
WARMUP, REPS, HOST_REPS = int(os.environ.get("WARMUP", "10")), int(os.environ.get("REPS", "30")), int(os.environ.get("HOST_REPS", "2"))
cfm.set_precision(os.environ.get("PRECISION", "bf16"))
dev = torch.device("cuda", 0)
head = synth.load_synth_(decoder.CTCDecoder(V, D, 0.0).eval(), 71)
with torch.no_grad():
    head.ctc_lo.bias[0] += float(os.environ.get("BLANK_BIAS", "3.0"))
head = head.to(dev)
x = torch.from_numpy(synth.normal(72, (B, T, D), 1.0)).to(dev)
lens = torch.tensor([T - (b * (T // 2)) // (B - 1) for b in range(B)], dtype=torch.int32, device=dev)
W, bias = head.ctc_lo.weight.detach(), head.ctc_lo.bias.detach()


def torch_device_part(k):
    lp = torch.log_softmax(torch.nn.functional.linear(x, W, bias).float(), -1)
    return (lp.argmax(-1), None) if k == 1 else lp.topk(k, dim=-1)


def torch_greedy():
    idx = torch_device_part(1)[0].cpu().tolist()
    n = lens.tolist()
    return [ref.best_path(idx[b], [0.0] * T, n[b], 0)[0] for b in range(B)]


def torch_beam():
    v, i = torch_device_part(BEAM)
    v, i, n = v.cpu(), i.cpu(), lens.tolist()
    return [ref.prefix_beam_search64(i[b], v[b], n[b], BEAM, 0)["nbest"] for b in range(B)]


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


with torch.no_grad():
    g_dev, g_ref = head.greedy_search(x, lens), torch_greedy()
    res = {"shape": [B, T, D, V], "beam": BEAM, "precision": cfm.get_precision().name,
           "tokens_per_frame": round(sum(len(h) for h in g_dev) / float(lens.sum()), 3),
           "greedy_equal_to_torch": sum(a == b for a, b in zip(g_dev, g_ref)), "utterances": B}
    res["greedy_ms"] = timed(lambda: head.greedy_search(x, lens), WARMUP, REPS)
    res["beam_ms"] = timed(lambda: head.prefix_beam_search(x, lens, beam=BEAM), WARMUP, REPS)
    res["torch_greedy_ms"] = timed(torch_greedy, 2, max(3, REPS // 3))
    res["torch_greedy_device_part_ms"] = timed(lambda: torch_device_part(1), WARMUP, REPS)
    res["torch_beam_ms"] = timed(torch_beam, 1, HOST_REPS)
    res["torch_beam_device_part_ms"] = timed(lambda: torch_device_part(BEAM), WARMUP, REPS)
    cfm.prof_enable(True); cfm.prof_reset()
    head.greedy_search(x, lens); head.prefix_beam_search(x, lens, beam=BEAM)
    torch.cuda.synchronize()
    res["kernels_us"] = {k: round(1e3 * v["ms"] / max(v["calls"], 1), 1) for k, v in cfm.prof_table().items() if k.startswith("ctc_")}
    cfm.prof_enable(False)
    res["greedy_speedup_vs_torch"] = round(res["torch_greedy_ms"] / res["greedy_ms"], 2)
    res["beam_speedup_vs_torch"] = round(res["torch_beam_ms"] / res["beam_ms"], 2)
    for k in list(res):
        if k.endswith("_ms"):
            res[k] = round(res[k], 4)
print(json.dumps(res))
