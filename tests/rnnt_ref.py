"""Float64 restatement of torchaudio.functional.rnnt_loss (fused_log_softmax=True) for the tests: log-softmax, the alpha recursion over the
(T x U+1) lattice (Graves 2012) evaluated by anti-diagonals, differentiated by torch.autograd; plus a brute-force sum over every alignment of a
tiny lattice that pins the recursion itself.  Runs on whatever device its inputs are on (CPU in the unit tests, the GPU as a checker)."""
import itertools
import math

import torch

NEG = -1e30            # "log 0" that keeps autograd finite (logaddexp of two -inf has a NaN gradient)


def lattice_logprobs(logits, targets, blank):
    """f64 (lp_blank [B,T,U1], lp_label [B,T,U1] with lp_label[..., U1-1] = NEG) from logits [B,T,U1,V]."""
    lp = torch.log_softmax(logits.double(), -1)
    B, T, U1, V = lp.shape
    lb = lp[..., blank]
    tail = lp.new_full((B, T, 1), NEG)
    if U1 == 1:
        return lb, tail
    idx = targets.long().to(lp.device).clamp(0, V - 1)[:, None, :, None].expand(B, T, U1 - 1, 1)
    ll = lp[:, :, :U1 - 1].gather(3, idx).squeeze(3)
    return lb, torch.cat([ll, tail], 2)


def alpha_diagonals(lb, ll):
    """alpha as [T+U1-1, B, U1]: entry (d, b, u) = alpha[b, d-u, u] (NEG where d-u is outside [0, T))."""
    B, T, U1 = lb.shape
    dev = lb.device
    u = torch.arange(U1, device=dev)
    lbf, llf = lb.reshape(B, T * U1), ll.reshape(B, T * U1)

    def at(flat, t, uu, ok):
        idx = (t.clamp(0, T - 1) * U1 + uu).expand(B, -1)
        return torch.where(ok, flat.gather(1, idx), flat.new_full((), NEG))

    prev = torch.where(u == 0, lb.new_zeros(()), lb.new_full((), NEG)).expand(B, U1)
    diags = [prev]
    for d in range(1, T + U1 - 1):
        t = d - u
        here = (t >= 0) & (t < T)
        up = prev + at(lbf, t - 1, u, (t >= 1) & here)
        um1 = (u - 1).clamp(min=0)
        left = torch.cat([lb.new_full((B, 1), NEG), prev[:, :-1]], 1) + at(llf, t, um1, (u >= 1) & here)
        cur = torch.where(here, torch.logaddexp(up, left), lb.new_full((), NEG))
        diags.append(cur)
        prev = cur
    return torch.stack(diags)


def costs_from_lattice(lb, ll, logit_lengths, target_lengths):
    B, T, U1 = lb.shape
    Tb = logit_lengths.long().to(lb.device).clamp(0, T)
    Ub = target_lengths.long().to(lb.device).clamp(0, U1 - 1)
    A = alpha_diagonals(lb, ll)
    bi = torch.arange(B, device=lb.device)
    t_end = (Tb - 1).clamp(min=0)
    ll_b = A[t_end + Ub, bi, Ub] + lb[bi, t_end, Ub]
    return torch.where(Tb > 0, -ll_b, lb.new_full((), math.inf))


def rnnt_loss_ref(logits, targets, logit_lengths, target_lengths, blank=-1, clamp=-1, reduction="mean"):
    """-> (loss, d loss / d logits, per-utterance costs), all f64.  The gradient is what torchaudio returns for upstream gradient 1: the
    per-utterance gradient, clamped to [-clamp, clamp] when clamp > 0, times 1/B for "mean"."""
    V = logits.shape[-1]
    blank = blank + V if blank < 0 else blank
    x = logits.detach().double().requires_grad_(True)
    lb, ll = lattice_logprobs(x, targets, blank)
    costs = costs_from_lattice(lb, ll, logit_lengths, target_lengths)
    finite = torch.isfinite(costs)
    (raw,) = torch.autograd.grad(costs[finite].sum(), x) if bool(finite.any()) else (torch.zeros_like(x),)
    if clamp > 0:
        raw = raw.clamp(-clamp, clamp)
    B = logits.shape[0]
    costs = costs.detach()
    if reduction == "none":
        return costs, raw, costs
    if reduction == "sum":
        return costs.sum(), raw, costs
    return costs.mean(), raw / B, costs


def brute_force_cost(logits, target, T, U, blank):
    """-log sum over every alignment of ONE utterance: logits [>=T, >=U+1, V], target [>=U]; every path from (0,0) takes T-1 blank moves and
    U label moves in some order and ends with the blank at (T-1, U)."""
    lp = torch.log_softmax(logits.double(), -1)
    terms = []
    for labels_at in itertools.combinations(range(T - 1 + U), U):
        t = u = 0
        s = 0.0
        for k in range(T - 1 + U):
            if k in labels_at:
                s += float(lp[t, u, int(target[u])])
                u += 1
            else:
                s += float(lp[t, u, blank])
                t += 1
        s += float(lp[T - 1, U, blank])
        terms.append(s)
    m = max(terms)
    return -(m + math.log(sum(math.exp(v - m) for v in terms)))
