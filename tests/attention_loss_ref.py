"""The label-smoothing loss of the attention decoder in float64 (the reference's label_smoothing_loss.py:52-80, restated), its closed form, its
gradient, the seeded cases of the kernel tests and the bounds those tests hold the kernels to.

Definition.  Per row with target t >= 0 over V classes, smoothing s, e = s / (V - 1): q_c = 1 - s at c = t and e elsewhere;
    loss_row = sum_c q_c (log q_c - log_softmax(z)_c),  0 log 0 = 0;       loss = sum_rows loss_row / denom
denom = the batch size, or with normalize_length the number of rows with t >= 0.  Rows with t < 0 are ignored.  No valid row: 0 (the reference
divides 0 by 0 there; the one deliberate difference).  Closed form, what csrc/lsm.hip evaluates:
    loss_row = C - (1 - s - e) (z_t - lse) - e (S - V lse),   C = (1 - s) log(1 - s) + s log e,   S = sum_c z_c
Gradient: d loss / d z_c = g (softmax(z)_c - q_c), g = upstream / denom.

Bounds of the kernel tests (none of them measured on the kernels; each follows from the formats):
  delta  the worst error of one logit: D products accumulated in f32, D * 2^-24 * max_{m,c} (sum_k |x||w| + |b|); 0 in the logits form.
  loss   z_t, lse and S / V each move by at most delta and (1 - s - e) + e V <= 2, so 4 delta; plus 2e-5 for the f32 exp / log of the online
         logsumexp (relative 2^-21 on a value below 10) and s * 2^-24 * max_m sum_c |z_c| for the running f32 sum of the logits.
  dz     |g| (2 delta + 1e-5) for the probability, plus the rounding of the output format at |dz| (bf16 2^-8, fp16 2^-10 and its subnormal step
         2^-24, f32 2^-23).
Observed on MI355X (tests/test_attention_loss_gpu.py, every case): loss |error| 1.0e-6 .. 1.6e-6 in both forms against bounds of 2e-5 .. 2.6e-3;
dz at 0.05 .. 0.49 of its bound."""
import numpy as np
import torch

F64 = torch.float64
DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
OUT_EPS = {torch.bfloat16: (2.0 ** -8, 0.0), torch.float16: (2.0 ** -10, 2.0 ** -24), torch.float32: (2.0 ** -23, 0.0)}


def target_dist(target, V, s):
    """q float64 [M, V] (rows with target < 0: all zero)."""
    q = torch.full((target.numel(), V), s / (V - 1) if V > 1 else 0.0, dtype=F64)
    live = target >= 0
    q[live, target[live].long()] = 1.0 - s
    q[~live] = 0.0
    return q


def rows_kl(z, target, s):
    """The definition: per-row divergence, float64 [M]."""
    z = z.to(F64)
    q = target_dist(target, z.shape[1], s)
    logp = torch.log_softmax(z, -1)
    return torch.where(q > 0, q * (torch.log(q.clamp_min(1e-300)) - logp), torch.zeros_like(q)).sum(-1)


def rows_closed(z, target, s):
    """The closed form the kernels evaluate, float64 [M]."""
    z = z.to(F64)
    V = z.shape[1]
    e = s / (V - 1) if V > 1 else 0.0
    C = ((1 - s) * np.log(1 - s) if s < 1 else 0.0) + (s * np.log(e) if e > 0 else 0.0)
    lse = torch.logsumexp(z, -1)
    zt = z.gather(1, target.long().clamp(min=0)[:, None])[:, 0]
    r = C - (1 - s - e) * (zt - lse) - e * (z.sum(-1) - V * lse)
    return torch.where(target >= 0, r, torch.zeros_like(r))


def denominator(target, batch, normalize_length):
    return float(max(int((target >= 0).sum()), 1)) if normalize_length else float(batch)


def loss(z, target, s, batch, normalize_length=False):
    return rows_kl(z, target, s).sum() / denominator(target, batch, normalize_length)


def grad(z, target, s, g):
    """g[m] (softmax(z_m) - q_m), float64 [M, V]; g float64 [M] (ignored rows give 0 whatever g holds)."""
    z = z.to(F64)
    d = g.to(F64)[:, None] * (torch.softmax(z, -1) - target_dist(target, z.shape[1], s))
    d[target < 0] = 0.0
    return d


# ---------------------------------------------------------------------------------------------------------------------------- seeded cases
def golden_case(V=37, B=3, L=6, seed=20):
    """Logits [B, L, V] and targets [B, L] (-1: ignored) of tests/golden/label_smoothing.npz."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, L, V, generator=g, dtype=F64) * 2.0
    t = torch.randint(0, V, (B, L), generator=g)
    t[0, 4:], t[1, 0], t[2, 5], t[2, 0], t[2, 1] = -1, -1, -1, 0, V - 1
    return z, t


def kernel_case(M, V, D, dt, dead=False):
    """Operands as the kernels see them: x [M, D] and w [Vp, D] in the 16-bit type (pad rows NaN), bias f32 [Vp] (pad entries 1e30), targets with
    -1 rows, class 0 and class V - 1 (dead: every row ignored), g f32 [M]; and in float64 on the operands as rounded: logits [M, V], delta."""
    gen = torch.Generator().manual_seed(M * 7919 + V * 31 + D + (1 if dt == "fp16" else 0))
    Vp = (V + 7) // 8 * 8 + 8
    x = torch.randn(M, D, generator=gen).to(DT[dt])
    w = (torch.randn(Vp, D, generator=gen) * (D ** -0.5)).to(DT[dt])
    bias = torch.randn(Vp, generator=gen)
    w[V:], bias[V:] = float("nan"), 1e30
    target = torch.randint(0, V, (M,), generator=gen).to(torch.int32)
    target[0::5], target[1::5], target[2::5] = 0, V - 1, -1
    if M == 1:
        target[0] = V - 1
    if M == 130:
        target[64:128] = -1                                     # the second tile of 64 rows is wholly ignored
    if dead:
        target[:] = -1
    g = (torch.rand(M, generator=gen) + 0.5) * torch.where(torch.rand(M, generator=gen) < 0.5, -1.0, 1.0)
    xr, wr, br = x.double(), w[:V].double(), bias[:V].double()
    z = xr @ wr.t() + br
    delta = D * 2.0 ** -24 * float((xr.abs() @ wr.abs().t() + br.abs()).max())
    return dict(x=x, w=w, bias=bias, target=target, g=g, z=z, delta=delta, Vp=Vp)


def loss_bound(z, s, delta):
    return 4.0 * delta + 2e-5 + s * 2.0 ** -24 * float(z.abs().sum(-1).max())


def grad_bound(ref, g, delta, out_dtype):
    """float64 [M, V]: the bound on |dz - ref| per element."""
    rel, sub = OUT_EPS[out_dtype]
    return g.double().abs()[:, None] * (2.0 * delta + 1e-5) + ref.abs() * rel + sub


# ------------------------------------------------------------------------------------------------------------- the whole decoder and its loss
# The loss of a decoder.TransformerDecoder on top of attention_decoder_ref.decoder_logits (dropout-free: that function itself), gradients by torch
# autograd in float64.  With dropout the same layer structure is restated with explicit keep masks per site (decoder_logits takes none;
# tests/test_attention_loss_cpu.py pins the two to each other without masks).  Site k uses seed + 0x9E3779B1 * k: 0 positional (element
# m * D + n of the [B * Lc, D] rows); per layer l at 1 + 6 l: self-attention probabilities (element ((b * H + h) * Tq + i) * Tk + j, include/cfm.h
# cfm_attn_desc.drop_p), self-attention output (m * D + n), source-attention probabilities, source-attention output, feed-forward hidden
# (m * FF + n), feed-forward output.
# round_a (the yardstick of the 16-bit modes): a round trip through the activation type wherever the device stores an activation in it -- the
# LayerNorm outputs, q / k / v, the attention context, the hidden activation -- applied to the value forward and to its gradient backward.
#
# Measured (MI355X, BiTransformerDecoder V=37 D=256 H=4 FF=512 2+2 layers, B=3, lengths 7/3/0, lsm 0.1; yardstick = this restatement in float32
# with the mode's rounding against float64, gate = 4 x): see DESIGN 7, "Training the attention decoder".
import math

import attention_decoder_ref as ADR
import gemm_ref


class _RoundTrip(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, f):
        ctx.f = f
        return f(x)

    @staticmethod
    def backward(ctx, g):
        return ctx.f(g), None


def _ra(x, f):
    return x if f is None else _RoundTrip.apply(x, f)


def act_round_trip(mode):
    if mode == "fp32":                                          # the products of the fp32 mode split their activation operand into hi + lo bf16 too
        return ADR.round_trip("fp32")
    t = DT[mode]
    return lambda x: x.to(t).to(x.dtype)


def keep(p, seed, site, shape):
    """float64 keep / (1 - p) of dropout site `site`, elements in row-major order of `shape`; None when p = 0."""
    if not p:
        return None
    n = 1
    for s in shape:
        n *= s
    return gemm_ref.keep_mask(n, p, (seed + 0x9E3779B1 * site) & 0xFFFFFFFF).view(*shape).double() * gemm_ref.drop_scale(p)


def _mul(x, k):
    return x if k is None else x * k.to(x.dtype)


def _mha(P, pre, q_in, kv_in, mask, H, round_w, round_a, keep_a):
    R, Tq, D = q_in.shape
    dk = D // H
    q = _ra(ADR._lin(P, pre + ".linear_q", q_in, round_w), round_a).view(R, Tq, H, dk).transpose(1, 2)
    k = _ra(ADR._lin(P, pre + ".linear_k", kv_in, round_w), round_a).view(R, -1, H, dk).transpose(1, 2)
    v = _ra(ADR._lin(P, pre + ".linear_v", kv_in, round_w), round_a).view(R, -1, H, dk).transpose(1, 2)
    m = mask.unsqueeze(1)
    s = ((q @ k.transpose(-1, -2)) / math.sqrt(dk)).masked_fill(~m, float("-inf"))
    p = _mul(torch.softmax(s, dim=-1).masked_fill(~m, 0.0), keep_a)
    ctx = _ra((p @ v).transpose(1, 2).reshape(R, Tq, D), round_a)
    return ADR._lin(P, pre + ".linear_out", ctx, round_w)


def decoder_logits_sites(P, tokens_in, self_mask, memory, memory_mask, H, dtype=F64, round_w=None, round_a=None, drops=None, seed=0, zmin=None):
    """attention_decoder_ref.decoder_logits with keep masks and activation round trips.  drops: dict(pos, self_a, src_a, out, hidden) of
    probabilities.  zmin: a list that receives the smallest |ReLU pre-activation| of every layer."""
    d = drops or {}
    x = ADR.embed(P, tokens_in, dtype)
    R, Lc, D = x.shape
    T = memory.shape[1]
    x = _mul(x, keep(d.get("pos"), seed, 0, (R, Lc, D)))
    memory = _ra(memory.to(dtype), round_a)
    for l in range(ADR.n_layers(P)):
        pre, k = "decoders.%d" % l, 1 + 6 * l
        xn = _ra(ADR._ln(P, pre + ".norm1", x), round_a)
        x = x + _mul(_mha(P, pre + ".self_attn", xn, xn, self_mask, H, round_w, round_a, keep(d.get("self_a"), seed, k, (R, H, Lc, Lc))),
                     keep(d.get("out"), seed, k + 1, (R, Lc, D)))
        xn = _ra(ADR._ln(P, pre + ".norm2", x), round_a)
        x = x + _mul(_mha(P, pre + ".src_attn", xn, memory, memory_mask.expand(-1, Lc, -1), H, round_w, round_a, keep(d.get("src_a"), seed, k + 2, (R, H, Lc, T))),
                     keep(d.get("out"), seed, k + 3, (R, Lc, D)))
        z = ADR._lin(P, pre + ".feed_forward.w_1", _ra(ADR._ln(P, pre + ".norm3", x), round_a), round_w)
        if zmin is not None:
            zmin.append(float(z.detach().abs().min()))
        FF = z.shape[-1]
        h = _ra(_mul(torch.relu(z), keep(d.get("hidden"), seed, k + 4, (R, Lc, FF))), round_a)
        x = x + _mul(ADR._lin(P, pre + ".feed_forward.w_2", h, round_w), keep(d.get("out"), seed, k + 5, (R, Lc, D)))
    return ADR._lin(P, "output_layer", _ra(ADR._ln(P, "after_norm", x), round_a), round_w)


def sos_eos(labels, lengths, sos, eos):
    """Padded labels [B, U] -> (ys_in long [B, Lc] padded with eos, targets long [B, Lc] padded with -1, self mask bool [B, Lc, Lc]), Lc = max L + 1."""
    B, Lc = labels.shape[0], int(max(lengths)) + 1
    tin = torch.full((B, Lc), eos, dtype=torch.long)
    tg = torch.full((B, Lc), -1, dtype=torch.long)
    for b, L in enumerate(lengths):
        y = labels[b, :L].long()
        tin[b, 0], tin[b, 1:L + 1] = sos, y
        tg[b, :L], tg[b, L] = y, eos
    i = torch.arange(Lc)
    mask = (i.view(1, 1, Lc) <= i.view(1, Lc, 1)) & (tg >= 0).unsqueeze(1)
    return tin, tg, mask


def decoder_loss(P, labels, lengths, memory, enc_lens, H, s, sos, eos, reverse=False, dtype=F64, round_w=None, round_a=None, drops=None, seed=0, zmin=None):
    """Label-smoothed loss / batch size of one decoder (state_dict-like P) on padded labels; reverse: on each row's reversed labels."""
    if reverse:
        labels = torch.stack([torch.cat([labels[b, :L].flip(0), labels[b, L:]]) for b, L in enumerate(lengths)])
    tin, tg, mask = sos_eos(labels, lengths, sos, eos)
    T = memory.shape[1]
    mm = (torch.arange(T).unsqueeze(0) < torch.as_tensor(enc_lens).long().unsqueeze(1)).unsqueeze(1)
    if round_a is None and not drops and zmin is None:
        logits = ADR.decoder_logits(P, tin, mask, memory, mm, H, dtype, round_w)
    else:
        logits = decoder_logits_sites(P, tin, mask, memory, mm, H, dtype, round_w, round_a, drops, seed, zmin)
    return loss(logits.reshape(-1, logits.shape[-1]), tg.reshape(-1), s, labels.shape[0])


DEC = dict(B=3, V=37, D=256, H=4, FF=512, layers=2, lengths=(7, 3, 0), lsm=0.1)


def decoder_case(T, p=0.0):
    """(decoder.BiTransformerDecoder on the CPU in train mode with every dropout probability p, memory f32 [B, T, D], enc_lens, labels long [B, 7]
    padded with -1, label lengths).  The biases of every w_1 alternate +-4: no ReLU pre-activation of the case lies within 0.25 of zero (asserted
    by the tests through zmin), so a rounding difference cannot flip a ReLU bit."""
    import decoder
    c = DEC
    torch.manual_seed(5000 + T)
    dec = decoder.BiTransformerDecoder(c["V"], c["D"], c["H"], c["FF"], c["layers"], c["layers"], p, p, p, p).train()
    with torch.no_grad():
        for d in (dec.left_decoder, dec.right_decoder):
            d.embed[0].weight.mul_(0.25)
            for layer in d.decoders:
                layer.feed_forward.w_1.bias.copy_(4.0 * torch.tensor([1.0, -1.0]).repeat(c["FF"] // 2))
    g = torch.Generator().manual_seed(6000 + T)
    memory = torch.randn(c["B"], T, c["D"], generator=g)
    enc_lens = [T, max(1, T - 2), max(1, T // 2)]
    labels = torch.full((c["B"], max(c["lengths"])), -1, dtype=torch.long)
    for b, L in enumerate(c["lengths"]):
        labels[b, :L] = torch.randint(0, c["V"] - 1, (L,), generator=g)
    return dec, memory, enc_lens, labels, list(c["lengths"])


def attention_loss_reference(dec, memory, enc_lens, labels, lengths, reverse_weight, dtype=F64, round_w=None, round_a=None, drops=None, seeds=(0, 0)):
    """-> (loss_att, grads: name -> tensor for 'memory' and every parameter of dec that the loss reaches, smallest |ReLU pre-activation|)."""
    c = DEC
    names = [n for n, _ in dec.named_parameters()]
    leaves = {n: q.detach().to(dtype).requires_grad_(True) for n, q in dec.named_parameters()}
    mem = memory.to(dtype).requires_grad_(True)
    zmin = []

    def one(prefix, reverse, seed):
        P = {n[len(prefix):]: t for n, t in leaves.items() if n.startswith(prefix)}
        return decoder_loss(P, labels, lengths, mem, enc_lens, c["H"], c["lsm"], c["V"] - 1, c["V"] - 1, reverse, dtype, round_w, round_a, drops, seed, zmin)

    total = one("left_decoder.", False, seeds[0])
    if reverse_weight > 0:
        total = (1 - reverse_weight) * total + reverse_weight * one("right_decoder.", True, seeds[1])
    gs = torch.autograd.grad(total, [mem] + [leaves[n] for n in names], allow_unused=True)
    grads = {"memory": gs[0]}
    grads.update({n: g for n, g in zip(names, gs[1:]) if g is not None})
    return total.detach(), grads, min(zmin)


def grad_metrics(got, ref):
    """(error of d loss / d memory, worst error over the parameters): max |d| / max(max |ref|, floor), floor = 1e-2 x the case's largest gradient
    (conftest.grad_err's metric: structurally zero gradients -- linear_k.bias -- are noise in both)."""
    floor = 1e-2 * max(float(v.abs().max()) for v in ref.values())
    m = {n: float((got[n].double() - ref[n].double()).abs().max()) / max(float(ref[n].abs().max()), floor) for n in ref}
    return m["memory"], max(v for n, v in m.items() if n != "memory"), m


def decoder_yardstick(mode, T, reverse_weight):
    """The restatement in float32 with the mode's weight rounding (attention_decoder_ref.round_trip) and activation round trips against float64 on
    the same case: (|loss error|, d memory metric, worst parameter metric).  The GPU gate is 4 x each."""
    dec, memory, enc_lens, labels, lengths = decoder_case(T)
    l64, g64, _ = attention_loss_reference(dec, memory, enc_lens, labels, lengths, reverse_weight)
    l32, g32, _ = attention_loss_reference(dec, memory, enc_lens, labels, lengths, reverse_weight, torch.float32, ADR.round_trip(mode), act_round_trip(mode))
    em, ep, _ = grad_metrics(g32, g64)
    return abs(float(l32) - float(l64)), em, ep
