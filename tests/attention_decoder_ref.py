"""Helper, not a test: the attention decoder and the rescoring of n-best lists, stated ONCE in plain torch (float64 by default).

The reference's decoder_layer.py:51 adds `dropout(self_attn(...))` to a tensor although its attention module returns a tuple, so the class raises on
its first call and model.py keeps the decoder commented out: there is no behaviour to reproduce.  This file is the definition instead -- the pre-norm
transformer decoder the loadable checkpoints (decoder.left_decoder.*, decoder.right_decoder.*) were trained with, in eval mode (no dropout):

    in = (sos, y_1..y_L), tg = (y_1..y_L, eos), Lc = L + 1
    x_i = E[in_i] * sqrt(D) + pe[i]                       pe: attention._sinusoid_table (f32), indexed by POSITION
    per layer:  x += SelfAttn(LN1(x))  mask j <= i and j < Lc;   x += SrcAttn(LN2(x), memory, memory)  mask t < enc_len;   x += FFN_relu(LN3(x))
    logits = output_layer(after_norm(x));     s(y) = sum_{i < Lc} log_softmax(logits_i)[tg_i]
    right decoder: the same on the reversed y;   att = (1 - rw) s_left + rw s_right (right only when rw > 0);   final = att + fpw * first_pass
    ranking per utterance: higher final first, an exact tie to the better first-pass rank, unused slots (first_pass = -inf or nlen < 0): -inf, last.

Everything is evaluated on PADDED batches the way the device does it ([B, N, Lmax] tokens, P = B N rows of Lc = Lmax + 1 positions, masks), so that
the invariances tests/test_attention_decoder_cpu.py asserts (a score does not depend on Lmax, N, slot or batch position) say something.
`P` is a TransformerDecoder state_dict; `dtype` and `round_w` (a function applied to every weight MATRIX of a Linear, e.g. a bf16 round trip) turn the
same code into the float32 yardstick of the GPU tolerances."""
import math

import torch

from attention import _sinusoid_table


def _lin(P, name, x, round_w):
    w = P[name + ".weight"]
    w = (round_w(w.float()) if round_w else w).to(x.dtype)
    return x @ w.t() + P[name + ".bias"].to(x.dtype)


def _ln(P, name, x):
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), P[name + ".weight"].to(x.dtype), P[name + ".bias"].to(x.dtype), 1e-5)


def _mha(P, pre, q_in, kv_in, mask, H, round_w):
    """q_in [R, Tq, D], kv_in [R, Tk, D], mask bool [R, Tq, Tk] (True: attend).  A fully masked row gives a zero context."""
    R, Tq, D = q_in.shape
    dk = D // H
    q = _lin(P, pre + ".linear_q", q_in, round_w).view(R, Tq, H, dk).transpose(1, 2)
    k = _lin(P, pre + ".linear_k", kv_in, round_w).view(R, -1, H, dk).transpose(1, 2)
    v = _lin(P, pre + ".linear_v", kv_in, round_w).view(R, -1, H, dk).transpose(1, 2)
    s = (q @ k.transpose(-1, -2)) / math.sqrt(dk)
    m = mask.unsqueeze(1)
    s = s.masked_fill(~m, float("-inf"))
    p = torch.softmax(s, dim=-1).masked_fill(~m, 0.0)
    p = torch.where(m.any(-1, keepdim=True), p, torch.zeros_like(p))
    ctx = (p @ v).transpose(1, 2).reshape(R, Tq, D)
    return _lin(P, pre + ".linear_out", ctx, round_w)


def n_layers(P):
    return 1 + max(int(k.split(".")[1]) for k in P if k.startswith("decoders."))


def embed(P, tokens_in, dtype=torch.float64):
    """tokens_in long [R, Lc] -> x0 [R, Lc, D]."""
    E = P["embed.0.weight"].to(dtype)
    D = E.shape[1]
    pe = _sinusoid_table(tokens_in.shape[1], D)[:, 0].to(dtype)
    return E[tokens_in] * math.sqrt(D) + pe


def decoder_logits(P, tokens_in, self_mask, memory, memory_mask, H, dtype=torch.float64, round_w=None):
    """tokens_in long [R, Lc], self_mask bool [R, Lc, Lc], memory [R, T, D], memory_mask bool [R, 1, T] -> logits [R, Lc, V]."""
    x = embed(P, tokens_in, dtype)
    memory = memory.to(dtype)
    for l in range(n_layers(P)):
        pre = "decoders.%d" % l
        xn = _ln(P, pre + ".norm1", x)
        x = x + _mha(P, pre + ".self_attn", xn, xn, self_mask, H, round_w)
        x = x + _mha(P, pre + ".src_attn", _ln(P, pre + ".norm2", x), memory, memory_mask.expand(-1, x.shape[1], -1), H, round_w)
        h = torch.relu(_lin(P, pre + ".feed_forward.w_1", _ln(P, pre + ".norm3", x), round_w))
        x = x + _lin(P, pre + ".feed_forward.w_2", h, round_w)
    return _lin(P, "output_layer", _ln(P, "after_norm", x), round_w)


def prep(tokens, nlen, score, sos, eos, reverse=False):
    """The padded decoder inputs of [B, N, Lmax] n-best buffers: (in long [P, Lc], targets long [P, Lc] (-1: none), mask bool [P, Lc, Lc])."""
    B, N, Lmax = tokens.shape
    Lc = Lmax + 1
    tin = torch.full((B * N, Lc), sos, dtype=torch.long)
    tg = torch.full((B * N, Lc), -1, dtype=torch.long)
    mask = torch.zeros((B * N, Lc, Lc), dtype=torch.bool)
    for p in range(B * N):
        b, n = divmod(p, N)
        if int(nlen[b, n]) < 0 or float(score[b, n]) == float("-inf"):
            continue
        L = min(int(nlen[b, n]), Lmax)
        y = tokens[b, n, :L].long()
        if reverse:
            y = y.flip(0)
        tin[p, 1:L + 1] = y
        tg[p, :L] = y
        tg[p, L] = eos
        i = torch.arange(Lc)
        mask[p] = (i.unsqueeze(0) <= i.unsqueeze(1)) & (i.unsqueeze(0) < L + 1)
    return tin, tg, mask


def token_logp(logits, tg):
    """log_softmax(logits)[tg] per position, 0 where tg < 0: [R, Lc]."""
    lp = torch.log_softmax(logits, dim=-1)
    return torch.where(tg >= 0, lp.gather(-1, tg.clamp(min=0).unsqueeze(-1)).squeeze(-1), torch.zeros_like(lp[..., 0]))


def scores(P, tokens, nlen, score, memory, enc_lens, H, sos, eos, reverse=False, dtype=torch.float64, round_w=None):
    """s(y) of every slot of the [B, N, Lmax] buffers against its utterance's memory [B, T, D]: [B, N] (0 for an unused slot)."""
    B, N, _ = tokens.shape
    tin, tg, mask = prep(tokens, nlen, score, sos, eos, reverse)
    T = memory.shape[1]
    mm = (torch.arange(T).unsqueeze(0) < torch.as_tensor(enc_lens).long().unsqueeze(1)).unsqueeze(1)          # [B, 1, T]
    logits = decoder_logits(P, tin, mask, memory.repeat_interleave(N, 0), mm.repeat_interleave(N, 0), H, dtype, round_w)
    return token_logp(logits, tg).sum(-1).view(B, N)


def rank(final):
    """The total order of one utterance's finals: indices, higher first, ties to the lower index, NaN as -inf."""
    key = [float("-inf") if f != f else f for f in final]
    return sorted(range(len(key)), key=lambda n: (-key[n], n))


def rescore(Pl, Pr, tokens, nlen, score, memory, enc_lens, H, sos, eos, first_pass_weight, reverse_weight, dtype=torch.float64, round_w=None):
    """(final, left, right [B, N], order: list of B index lists)."""
    left = scores(Pl, tokens, nlen, score, memory, enc_lens, H, sos, eos, False, dtype, round_w)
    right = torch.zeros_like(left)
    att = left
    if reverse_weight > 0:
        right = scores(Pr, tokens, nlen, score, memory, enc_lens, H, sos, eos, True, dtype, round_w)
        att = (1 - reverse_weight) * left + reverse_weight * right
    unused = (torch.as_tensor(nlen) < 0) | (score == float("-inf"))
    final = torch.where(unused, torch.full_like(att, float("-inf")), att + first_pass_weight * score.to(att.dtype).masked_fill(unused, 0.0))
    return final, left, right, [rank(row.tolist()) for row in final]


def pack_nbest(nbest, N=None, Lmax=None, pad_token=0):
    """[[(tokens, score), ...] per utterance] -> (tokens int32 [B, N, Lmax], nlen int32 [B, N] (-1: unused), score f32 [B, N] (-inf: unused))."""
    B = len(nbest)
    N = N or max(1, max(len(u) for u in nbest))
    Lmax = Lmax if Lmax is not None else max([len(t) for u in nbest for t, _ in u] + [1])
    tokens = torch.full((B, N, Lmax), pad_token, dtype=torch.int32)
    nlen = torch.full((B, N), -1, dtype=torch.int32)
    score = torch.full((B, N), float("-inf"), dtype=torch.float32)
    for b, u in enumerate(nbest):
        for n, (t, s) in enumerate(u):
            tokens[b, n, :len(t)] = torch.tensor(t, dtype=torch.int32)
            nlen[b, n] = len(t)
            score[b, n] = s
    return tokens, nlen, score


def round_trip(dt):
    """The weight rounding of a precision mode as a function on f32 matrices: bf16 / fp16 round trip, or the hi + lo bf16 split of fp32 mode."""
    if dt == "fp32":
        def f(w):
            hi = w.to(torch.bfloat16).float()
            return hi + (w - hi).to(torch.bfloat16).float()
        return f
    t = torch.bfloat16 if dt == "bf16" else torch.float16
    return lambda w: w.to(t).float()


# ---------------------------------------------------------------------------------------------------------------- the module-level case of the tests
CASE = dict(B=3, N=4, D=256, H=4, FF=512, V=37, layers=2, first_pass_weight=0.5, reverse_weight=0.3)
SEEDS, FRAMES = (0, 1, 2), (5, 19)


def module_case(seed, T):
    """(decoder.BiTransformerDecoder on the CPU in eval mode, memory f32 [B, T, D], enc_lens, nbest lists) -- seeded, the same on every machine.
    Ragged lengths, an empty hypothesis, an unused slot (utterance 2 has N - 1 entries)."""
    import decoder
    c = CASE
    torch.manual_seed(4000 + 10 * seed + T)
    dec = decoder.BiTransformerDecoder(c["V"], c["D"], c["H"], c["FF"], c["layers"], c["layers"], 0.1, 0.1, 0.0, 0.0).eval()
    with torch.no_grad():
        for d in (dec.left_decoder, dec.right_decoder):
            d.output_layer.weight.mul_(6.0)                     # scores that differ between hypotheses by more than rounding
            d.embed[0].weight.mul_(0.25)
    g = torch.Generator().manual_seed(9000 + 10 * seed + T)
    memory = torch.randn(c["B"], T, c["D"], generator=g)
    enc_lens = [T, max(1, T - 2), max(1, T // 2)]
    nbest = []
    for b in range(c["B"]):
        entries = []
        for n in range(c["N"] - (1 if b == 2 else 0)):
            L = 0 if (b, n) == (1, 2) else int(torch.randint(1, 8, (1,), generator=g))
            entries.append((torch.randint(0, c["V"] - 1, (L,), generator=g).tolist(), -1.0 - 0.125 * n - 0.25 * b))
        nbest.append(entries)
    return dec, memory, enc_lens, nbest


def module_reference(dec, memory, enc_lens, nbest, reverse_weight, dtype=torch.float64, round_w=None):
    """(final, left, right, order) of the restatement for a module_case, sos = eos = V - 1."""
    c = CASE
    tokens, nlen, score = pack_nbest(nbest)
    return rescore(dec.left_decoder.state_dict(), dec.right_decoder.state_dict(), tokens, nlen, score, memory, enc_lens, c["H"], c["V"] - 1, c["V"] - 1,
                   c["first_pass_weight"], reverse_weight, dtype, round_w)


def forward_case(dec, nbest):
    """targets long [P, L] = sos + tokens padded with eos, lengths [P] for TransformerDecoder.forward, from a module_case's hypotheses."""
    V = CASE["V"]
    hyps = [t for u in nbest for t, _ in u]
    L = max(len(t) for t in hyps) + 1
    targets = torch.full((len(hyps), L), V - 1, dtype=torch.long)
    for p, t in enumerate(hyps):
        targets[p, 1:len(t) + 1] = torch.tensor(t, dtype=torch.long)
    return targets, torch.tensor([len(t) + 1 for t in hyps], dtype=torch.int32), [b for b, u in enumerate(nbest) for _ in u]


def forward_reference(P, targets, lengths, memory, enc_lens, owner, dtype=torch.float64, round_w=None):
    """The restatement's logits [P, L, V] for forward_case's padded targets (positions past a row's length hold values nobody compares)."""
    L = targets.shape[1]
    i = torch.arange(L)
    mask = (i.view(1, 1, L) <= i.view(1, L, 1)) & (i.view(1, 1, L) < lengths.long().view(-1, 1, 1))
    T = memory.shape[1]
    mm = (torch.arange(T).unsqueeze(0) < torch.as_tensor(enc_lens).long().unsqueeze(1)).unsqueeze(1)
    return decoder_logits(P, targets, mask, memory[owner], mm[owner], CASE["H"], dtype, round_w)


def yardstick(mode, seed, T, reverse_weight):
    """max |float32 torch with the mode's weight rounding - float64| of the restatement on a module_case: (error of final over used slots, error of
    the left decoder's forward logits over valid positions).  The GPU gate is 4 x this."""
    dec, memory, enc_lens, nbest = module_case(seed, T)
    f64 = module_reference(dec, memory, enc_lens, nbest, reverse_weight)[0]
    f32 = module_reference(dec, memory, enc_lens, nbest, reverse_weight, torch.float32, round_trip(mode))[0]
    used = f64 > float("-inf")
    e_final = float((f32.double() - f64)[used].abs().max())
    targets, lengths, owner = forward_case(dec, nbest)
    P = dec.left_decoder.state_dict()
    l64 = forward_reference(P, targets, lengths, memory, enc_lens, owner)
    l32 = forward_reference(P, targets, lengths, memory, enc_lens, owner, torch.float32, round_trip(mode))
    valid = torch.arange(targets.shape[1]).unsqueeze(0) < lengths.long().unsqueeze(1)
    return e_final, float((l32.double() - l64)[valid].abs().max())


def min_gap(final_row):
    """The smallest difference between adjacent finite finals of one utterance in rank order (inf with fewer than two)."""
    v = sorted((f for f in final_row if f > float("-inf")), reverse=True)
    return min([a - b for a, b in zip(v, v[1:])] + [float("inf")])
