"""Helper, not a test: float64 beam search with the attention decoder on the CPU -- the specification of decoder.AttentionBeamSearch and
csrc/attn_search.hip's cfm_dec_beam_prune.  The reference project has no such search, so it is pinned here, on tests/attention_decoder_ref.py
(`embed`, `decoder_logits`, the parameter dict P).  It has NO cache on purpose: every step recomputes decoder_logits over the whole prefix, so
agreement with it proves the device's K/V cache.

Per utterance (memory's first n frames, beam K, sos, eos, max_len -- default n):

  1. the live set starts as [sos] at score 0; all hypotheses have the same length, step i feeds the token at position i
  2. every unfinished hypothesis: logp = log_softmax(logits at position i); it offers its K best classes (the lower class first among equal
     values) at score = parent's score + logp
  3. a hypothesis is finished once its last token is eos; a finished one offers exactly one candidate, itself, score unchanged
  4. candidates are ordered by higher score, then the better-ranked parent, then the lower class; the best K are kept, in that order (different
     parents never produce equal strings: no merging)
  5. done when all kept hypotheses are finished, or after max_len steps; the result is the kept set, best first, as (tokens without sos / eos,
     score, finished); no length normalisation, as the rescorer
  6. n = 0: [((), 0.0)], no step

What a result rests on is recorded as `gaps`; `clear(result, delta)` is true when every gap exceeds delta -- an f32 search then decides alike.
  rank    score of the last kept candidate minus score of the first dropped one
  topk    per unfinished row with more classes than K: max(logp of the last class offered - logp of the first one not offered, score of the last
          kept candidate - the score the first class not offered would have had): the classes are told apart, or neither matters
  final   differences of consecutive n-best scores
"""
import numpy as np
import torch

import attention_decoder_ref as A

NEG = float("-inf")


def order_key(c):
    """The total order of rule 4 on candidates (score, parent rank, class, ...)."""
    return (-c[0], c[1], c[2])


def prune_ref(idx, logp, score, finished, K, eos):
    """Rules 2-4 on given top-K lists, in float32 as the device adds: idx / logp [rows, >= K] per parent row (best first), score f32 [rows],
    finished bool [rows].  Returns the kept candidates, best first, as (score np.float32, parent, class, finished)."""
    cands = []
    for p in range(len(score)):
        if finished[p]:
            cands.append((np.float32(score[p]), p, int(eos), True))
            continue
        for j in range(K):
            cands.append((np.float32(np.float32(score[p]) + np.float32(logp[p][j])), p, int(idx[p][j]), False))
    cands.sort(key=lambda c: (-float(c[0]) if c[0] == c[0] else float("inf"), c[1], c[2]))
    return [(c[0], c[1], c[2], c[3] or c[2] == eos) for c in cands[:K]]


def step_logp(P, prefixes, mem, H, dtype=torch.float64, round_w=None):
    """log_softmax of the logits at the last position of equally long prefixes (sos included), recomputed over the whole prefix: [rows, V]."""
    tin = torch.tensor(prefixes, dtype=torch.long)
    R, L = tin.shape
    i = torch.arange(L)
    mask = (i.view(1, 1, L) <= i.view(1, L, 1)).expand(R, L, L)
    mm = torch.ones((R, 1, mem.shape[0]), dtype=torch.bool)
    logits = A.decoder_logits(P, tin, mask, mem.unsqueeze(0).expand(R, -1, -1), mm, H, dtype, round_w)
    return torch.log_softmax(logits[:, -1].double(), -1)


def search64(P, memory, n, beam, H, sos, eos, max_len=None, dtype=torch.float64, round_w=None):
    """One utterance: memory [T, D] of which the first n frames are valid.  Returns dict(nbest=[(tokens tuple, score, finished)] best first,
    gaps, steps)."""
    n = int(n)
    out = dict(nbest=[((), 0.0, True)], gaps=[], steps=0)
    if n == 0:
        return out
    max_len = n if max_len is None else int(max_len)
    assert beam >= 1 and max_len >= 1
    mem = memory[:n]
    live = [dict(tokens=(sos,), score=0.0, fin=False)]
    gaps = out["gaps"]
    for i in range(max_len):
        out["steps"] += 1
        rows = [r for r, a in enumerate(live) if not a["fin"]]
        logp = step_logp(P, [live[r]["tokens"] for r in rows], mem, H, dtype, round_w)
        cands, boundary = [], []
        for r, a in enumerate(live):
            if a["fin"]:
                cands.append((a["score"], r, eos, a))
                continue
            lp = logp[rows.index(r)]
            v, ix = torch.sort(lp, descending=True, stable=True)
            for j in range(min(beam, lp.numel())):
                k = int(ix[j])
                cands.append((a["score"] + float(v[j]), r, k, dict(tokens=a["tokens"] + (k,), score=a["score"] + float(v[j]), fin=k == eos)))
            if lp.numel() > beam:
                boundary.append((float(v[beam - 1] - v[beam]), a["score"] + float(v[beam])))
        cands.sort(key=order_key)
        if len(cands) > beam:
            gaps.append(cands[beam - 1][0] - cands[beam][0])
        last_kept = cands[beam - 1][0] if len(cands) >= beam else NEG
        gaps.extend(max(g, last_kept - s) for g, s in boundary)
        live = [c[3] for c in cands[:beam]]
        if all(a["fin"] for a in live):
            break
    gaps.extend(live[k]["score"] - live[k + 1]["score"] for k in range(len(live) - 1))
    strip = lambda t, fin: tuple(t[1:-1] if fin else t[1:])
    out["nbest"] = [(strip(a["tokens"], a["fin"]), a["score"], a["fin"]) for a in live]
    assert len({(h[0], h[2]) for h in out["nbest"]}) == len(out["nbest"])
    return out


def clear(res, delta):
    return all(g > delta for g in res["gaps"])


# -- seeded cases shared by the CPU and the GPU tests ---------------------------------------------------------------------------------------
H, FF, LAYERS = 4, 256, 2
# name, B, beam, T', V, D, max_len (None: the frames), seed, sharpen, eos bias, the precision modes under whose delta the float64 search ALONE calls
# at least half of the case's utterances clear, with margin (twice the delta; test_attention_search_cpu.py asserts it).  EVERY case runs on the
# device in all of MODES; the clear-share condition is asserted for the listed modes and printed for the others.
# sharpen multiplies output_layer's weights and eos_bias is added to the eos logit: a synthetic decoder's posterior is nearly uniform and never ends
# a hypothesis; the two give the peaked posterior of a trained model and strings of a few tokens.  Chosen with search64 alone.
#
# Why not every mode everywhere.  delta = (length + 1) x 4 x the float32 yardstick is about 0.2 .. 5 in bf16 and 0.03 .. 0.6 in fp16 for strings of
# 1 .. 20 tokens, and it scales with the logits: sharpening widens the gaps and the rounding error alike.  A sweep with search64 alone over
# sharpen in {6, 24, 96} x eos bias in {0, 8, 30} x max_len in {frames, 2}, and D in {144, 256}, gave as clear utterances at twice the delta
# (bf16, fp16):
#   B = 16, beam 10, V = 17     at most 3 and 12 of 16; bf16's best (sharpen 6, eos bias 30) is strings that all end at once, fp16 reaches 11 of 16
#                               with max_len = 2 at sharpen 24, eos bias 8 -- the case b16_k10_cut2
#   B = 3, beam 16, V = 5002    1 and 1 of 3 in all 38 settings: only the utterance without frames; the 16th and 17th of 5002 classes lie closer than
#                               either mode's delta at every scale
#   B = 3, beam 4, V = 17       with two utterances of real length: bf16 1 of 3 for every seed 21 .. 59 at max_len = frames or 5, 3 of 3 at
#                               max_len = 2 (b3_k4_cut2); fp16 3 of 3 (b3_k4), 2 of 3 (b3_k4_maxlen)
# So bf16 is asserted clear at beam 1 and at beam 4 with a cut-off of 2, fp16 also at beam 4 and at beam 10 with that cut-off, fp32 everywhere.
MODES = ("bf16", "fp16", "fp32")
GPU_CASES = [
    ("b1_k1", 1, 1, 12, 17, 144, None, 28, 24.0, 3.0, ("bf16", "fp16", "fp32")),
    ("b3_k4", 3, 4, 20, 17, 256, None, 49, 24.0, 3.0, ("fp16", "fp32")),
    ("b3_k4_cut2", 3, 4, 12, 17, 256, 2, 49, 24.0, 3.0, ("bf16", "fp16", "fp32")),
    ("b16_k10", 16, 10, 12, 17, 144, None, 23, 24.0, 3.0, ("fp32",)),
    ("b16_k10_cut2", 16, 10, 12, 17, 144, 2, 23, 24.0, 8.0, ("fp16", "fp32")),
    ("b3_k16_v5002", 3, 16, 14, 5002, 256, None, 28, 24.0, 8.0, ("fp32",)),
    ("b3_k4_maxlen", 3, 4, 40, 17, 144, 5, 25, 24.0, -30.0, ("fp16", "fp32")),
]


def decoder_for(case):
    """decoder.TransformerDecoder of a case on the CPU in eval mode, seeded."""
    import decoder
    name, B, K, T, V, D, max_len, seed, sharpen, eos_bias, modes = case
    torch.manual_seed(7000 + seed)
    dec = decoder.TransformerDecoder(V, D, H, FF, LAYERS, 0.1, 0.1, 0.0, 0.0).eval()
    with torch.no_grad():
        dec.output_layer.weight.mul_(sharpen)
        dec.output_layer.bias[V - 1] += eos_bias
        dec.embed[0].weight.mul_(0.25)
    return dec


def inputs(case):
    """(decoder, memory f32 [B, T', D], ragged lens (list): the first utterance is full, the last has no frame where B >= 3 -- a case of three keeps
    two utterances of real length -- and one has a single frame where B >= 4)."""
    name, B, K, T, V, D, max_len, seed, sharpen, eos_bias, modes = case
    rs = np.random.RandomState(seed)
    memory = torch.from_numpy(rs.standard_normal((B, T, D)).astype(np.float32))
    lens = rs.randint(2, T + 1, B)
    lens[0] = T
    if B >= 3:
        lens[-1] = 0
    if B >= 4:
        lens[1] = 1
    return decoder_for(case), memory, [int(v) for v in lens]


_cache = {}


def reference(case):
    """search64 per utterance of a case, computed once: the list of result dicts (sos = eos = V - 1)."""
    if case[0] not in _cache:
        name, B, K, T, V, D, max_len, seed, sharpen, eos_bias, modes = case
        dec, memory, lens = inputs(case)
        P = dec.state_dict()
        _cache[case[0]] = [search64(P, memory[b].double(), lens[b], K, H, V - 1, V - 1, max_len) for b in range(B)]
    return _cache[case[0]]


_yard = {}


def yardstick(mode, case):
    """max |float32 torch with the mode's weight rounding - float64| of the per-position log-probabilities of the float64 search's own n-best
    strings (every position of every returned hypothesis, eos included).  The GPU's per-position gate is 4 x this."""
    if (mode, case[0]) not in _yard:
        name, B, K, T, V, D, max_len, seed, sharpen, eos_bias, modes = case
        dec, memory, lens = inputs(case)
        P = dec.state_dict()
        nbest = [[(list(t), s) for t, s, _ in r["nbest"]] for r in reference(case)]
        tokens, nlen, score = A.pack_nbest(nbest, N=K)
        tin, tg, mask = A.prep(tokens, nlen, score, V - 1, V - 1)
        mm = (torch.arange(T).unsqueeze(0) < torch.tensor(lens).unsqueeze(1)).unsqueeze(1)
        args = (memory.repeat_interleave(K, 0), mm.repeat_interleave(K, 0), H)
        lp64 = A.token_logp(A.decoder_logits(P, tin, mask, *args), tg)
        lp32 = A.token_logp(A.decoder_logits(P, tin, mask, *args, torch.float32, A.round_trip(mode)), tg)
        _yard[mode, case[0]] = float((lp32.double() - lp64)[tg >= 0].abs().max())
    return _yard[mode, case[0]]


def deltas(mode, case):
    """Per utterance the margin of the device search against the float64 one: (the longest returned hypothesis + 1) x the per-position gate, and
    the gate itself (4 x yardstick)."""
    gate = 4.0 * yardstick(mode, case)
    return [(max([len(t) for t, _, _ in r["nbest"]] + [0]) + 1) * gate for r in reference(case)], gate
