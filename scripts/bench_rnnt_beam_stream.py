"""Streaming RNN-T beam search on the config-4 head (V = 5002, E = 256, H = 256, P = 512, J = 512, L = 2, ffn_out x 10), chunk 16, max_symbols 4:
16 streams x beam 4 and 8 streams x beam 8 over --chunks chunks of one utterance per stream, final with the last chunk.  Per row: ms per decode
(host clock around decode, which ends in its own device reads), steps per chunk, us per step (decode time over steps, so feed, report and the
host reads are in it), replays per decode, and the report launch alone (device events around 20 launches).  Beside it, on the same box:
greedy.ChunkGreedySearch.decode at 64 streams on the same chunks, and the offline greedy.BeamSearch on the whole utterance (us per step).

    python scripts/bench_rnnt_beam_stream.py [--chunks 15] [--warmup 1] [--runs 3] [--out FILE]

Needs the GPU.  One JSON line per row."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "conformer-pytorch-lightning_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--max-symbols", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import cfm
    import greedy
    import greedy_ref as R
    if not torch.cuda.is_available():
        raise SystemExit("bench_rnnt_beam_stream.py needs the GPU")
    dev = torch.device("cuda")
    pr, jn = R.modules(5002, 256, 256, 512, 512, 2, 53, enc_dim=512, shaped=True)
    with torch.no_grad():
        jn.ffn_out.weight.mul_(10.0)                       # a peaked posterior, as the tests' heads (tests/rnnt_beam_ref.py)
    pr, jn = pr.to(dev), jn.to(dev)
    C, T = 16, 16 * a.chunks
    enc = torch.from_numpy(np.random.RandomState(7).standard_normal((64, T, 512)).astype(np.float32)).to(dev)
    rows = []

    def emit(**row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def utterance(dec, B, beam):
        """One utterance per stream, chunk by chunk: (seconds, steps, replays, tokens of the best hypotheses)."""
        dec.reset()
        torch.cuda.synchronize()
        steps = replays = 0
        t0 = time.perf_counter()
        for i in range(a.chunks):
            chunk = enc[:B, i * C:(i + 1) * C]
            out = dec.decode(chunk, None, [i == a.chunks - 1] * B) if beam else dec.decode(chunk)
            steps += dec.steps
            replays += dec.replays
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        tokens = sum(len(r["best"][0]) for r in out) if beam else sum(len(h) for h in dec.hyps())
        return dt, steps, replays, tokens

    def row(name, dec, B, beam):
        for _ in range(a.warmup):
            utterance(dec, B, beam)
        best = min((utterance(dec, B, beam) for _ in range(a.runs)), key=lambda r: r[0])
        dt, steps, replays, tokens = best
        r = dict(search=name, streams=B, beam=beam, chunk=C, chunks=a.chunks, ms_per_decode=round(dt * 1e3 / a.chunks, 3), steps_per_chunk=round(steps / a.chunks, 2),
                 us_per_step=round(dt * 1e6 / max(steps, 1), 2), replays_per_decode=round(replays / a.chunks, 2), tokens_per_stream=round(tokens / B, 1))
        if beam:
            lib, ev0, ev1 = cfm.lib(), torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            for _ in range(20):
                cfm.check(lib.cfm_rnnt_beam_stream_report(ctypes.byref(dec._descs[0]), cfm.stream()), "cfm_rnnt_beam_stream_report")
            ev1.record()
            torch.cuda.synchronize()
            r["report_us_done_streams"] = round(ev0.elapsed_time(ev1) * 1e3 / 20, 2)     # every stream is done here: the launch alone
            dec.reset()
            for i in range(a.chunks - 1):
                dec.decode(enc[:B, i * C:(i + 1) * C])
            dec.S["stable_len"].zero_()                                                 # the whole backtrace, as without the stable-prefix shortcut
            ev0.record()
            cfm.check(lib.cfm_rnnt_beam_stream_report(ctypes.byref(dec._descs[0]), cfm.stream()), "cfm_rnnt_beam_stream_report")
            ev1.record()
            torch.cuda.synchronize()
            r["report_us_full_backtrace"] = round(ev0.elapsed_time(ev1) * 1e3, 2)
            r["best_len_at_report"] = int(dec.S["best_len"].max())
        emit(**r)

    row("chunk_greedy", greedy.ChunkGreedySearch(pr, jn, 64, C, n_steps=a.max_symbols, steps_per_replay=4, fused=True), 64, 0)
    for B, beam in ((16, 4), (8, 8)):
        row("stream_beam", greedy.StreamingBeamSearch(pr, jn, B, beam, C, T, max_len=T, max_symbols=a.max_symbols, steps_per_replay=8), B, beam)
        bs = greedy.BeamSearch(pr, jn, beam, max_symbols=a.max_symbols, max_len=T, steps_per_replay=32)
        for _ in range(a.warmup + 1):
            bs.search(enc[:B], [T] * B)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.runs):
            bs.search(enc[:B], [T] * B)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / a.runs
        emit(search="offline_beam", streams=B, beam=beam, frames=T, ms_per_call=round(dt * 1e3, 3), steps=bs.steps, us_per_step=round(dt * 1e6 / max(bs.steps, 1), 2))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
