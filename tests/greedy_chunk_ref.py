"""Helpers of the chunk-lookahead greedy search tests: random chunk states, the float64 logits of every frame of a chunk, and ONE lookahead
step restated as greedy_ref.control applied frame by frame per stream -- up to and including the next emission, or the chunk's end."""
import numpy as np
import torch

import greedy_ref as R


def random_chunk_state(S, rs, V, n_steps, chunk):
    """Undoctored values in every tensor of a ChunkGreedySearch state S that one step reads: tokens, LSTM state, frame index inside the chunk
    (at and past lens too), lens 0 (idle streams), per-frame counts up to n_steps - 1, total counts; the fused step's scratch NaN / -1.
    Returns the host copy greedy_ref.control starts from (cap: control's last writable slot)."""
    L, B, H = S["h"].shape
    J = S["enc_proj"].shape[2]
    ld = S["hyps"].shape[1]
    t = rs.randint(0, chunk + 1, B)
    lens = rs.randint(0, chunk + 1, B)
    lens[::5] = 0                                        # idle
    if B > 2:
        lens[1], t[1] = chunk, 0                         # a whole chunk ahead
        t[2] = lens[2]                                   # finished exactly at lens
    fc = rs.randint(0, n_steps, B)
    fc[::3] = n_steps - 1                                # the next emission on the same frame hits the cap
    vals = dict(token=rs.randint(0, V, B), t=t, lens=lens, frame_count=fc, count=rs.randint(0, ld - 1, B), hyps=rs.randint(-5, V, (B, ld)))
    for k, v in vals.items():
        S[k].copy_(torch.from_numpy(v.astype(np.int64)))
    S["h"].copy_(torch.from_numpy(rs.uniform(-1, 1, (L, B, H)).astype(np.float32)))
    S["c"].copy_(torch.from_numpy((2.0 * rs.standard_normal((L, B, H))).astype(np.float32)))
    S["enc_proj"].copy_(torch.from_numpy(rs.standard_normal((B, chunk, J)).astype(np.float32)))
    done = t >= lens
    S["steps"].zero_()
    S["overflow"].zero_()
    S["n_done"].fill_(int(done.sum()))
    if "done8" in S:
        S["done8"].copy_(torch.from_numpy(done.astype(np.uint8)))
        for k in ("h_new", "c_new", "pred", "pp", "act", "pmax"):
            S[k].fill_(float("nan"))
        for k in ("pidx", "rows", "row_off", "row_cnt", "n_rows"):
            S[k].fill_(-1)
    host = {k: S[k].cpu().numpy().copy() for k in ("token", "t", "lens", "frame_count", "count", "hyps", "h", "c")}
    host.update(done=done.copy(), n_done=int(done.sum()), cap=ld - 1)
    return host


def chunk_logits64(P64, host, enc_proj):
    """float64: the step's LSTM candidates and projection, and act (B, chunk, J) / logits (B, chunk, V) of EVERY frame of the chunk against the
    streams' current predictor output (greedy_ref.step64 per frame)."""
    enc_proj = torch.as_tensor(enc_proj).double().cpu()
    outs = [R.step64(P64, host["token"], host["h"], host["c"], enc_proj[:, f]) for f in range(enc_proj.shape[1])]
    ref = {k: outs[0][k] for k in ("h_new", "c_new", "pred", "gate_max")}
    ref["act"] = torch.stack([o["act"] for o in outs], 1)
    ref["logits"] = torch.stack([o["logits"] for o in outs], 1)
    return ref


def lookahead_by_single_steps(host, k_frames, h_new, c_new, blank, n_steps):
    """One lookahead step = greedy_ref.control (model.py:255-267, one frame decision) applied repeatedly per stream, k_frames[b, f] the class
    of frame f against the stream's CURRENT predictor output, until the stream emitted (its predictor output changes: the lookahead ends
    there) or finished.  Returns (state after, single-frame steps the longest stream needed)."""
    out = {n: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for n, v in host.items()}
    B = len(host["token"])
    most = 0
    for b in range(B):
        s = {n: (v[b:b + 1].copy() if n not in ("h", "c") else v[:, b:b + 1].copy()) for n, v in host.items() if isinstance(v, np.ndarray)}
        s.update(n_done=0, cap=host["cap"])
        n = 0
        while not s["done"][0]:
            before = int(s["count"][0])
            s = R.control(s, [int(k_frames[b, int(s["t"][0])])], h_new[:, b:b + 1], c_new[:, b:b + 1], blank, n_steps)
            n += 1
            if int(s["count"][0]) != before:
                break
        most = max(most, n)
        for name in ("token", "t", "frame_count", "count", "hyps", "done"):
            out[name][b] = s[name][0]
        out["h"][:, b], out["c"][:, b] = s["h"][:, 0], s["c"][:, 0]
        out["n_done"] += s["n_done"]
    return out, most


def chunks_of(enc, lens, chunk):
    """(B, T, E) and per-stream lengths cut into pieces of `chunk` frames: yields (padded piece (B, chunk, E), lens of the piece, the
    unpadded piece); the last, shorter piece is zero padded and goes in through lens."""
    B, T, E = enc.shape
    for s in range(0, T, chunk):
        raw = enc[:, s:s + chunk].contiguous()
        piece = raw if raw.shape[1] == chunk else torch.cat([raw, raw.new_zeros((B, chunk - raw.shape[1], E))], 1)
        yield piece, [max(0, min(raw.shape[1], int(n) - s)) for n in lens], raw
