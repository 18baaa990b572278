"""Helper, not a test: the CTC prefix scorer and joint CTC/attention decoding in float64 on the CPU -- the specification of csrc/ctc_prefix.hip
(cfm_ctc_logprob_t, cfm_ctc_prefix_score, cfm_ctc_prefix_advance) and of decoder.JointBeamSearch.  The reference project has no such search; the
scorer is the standard one of hybrid CTC/attention decoding, pinned here against brute-force enumeration (tests/test_ctc_prefix_cpu.py).

x [n, V] = log_softmax(CTC logits) of an utterance's n valid frames; (+) is logaddexp; blank = 0 by default; eos != blank.  A hypothesis g (its
tokens after sos) carries gamma_n[t], gamma_b[t], t < n -- the log-probabilities of all alignments of exactly g to frames 0..t that end in its last
token, respectively in blank -- and psi(g), the log-probability that the output starts with g.

  empty g       gamma_n[t] = -inf, gamma_b[t] = sum_{tau <= t} x[tau, blank], psi = 0
  candidate c   (not blank, not eos; `last` the last token of g)
                phi[t] = gamma_b[t] if c == last else gamma_n[t] (+) gamma_b[t]
                psi(g.c) = init (+) (+)_{t=1..n-1} (phi[t-1] + x[t, c]),  init = x[0, c] if g is empty else -inf       -- a REDUCTION over t
                gamma_n'[0] = init, gamma_b'[0] = -inf
                gamma_n'[t] = (gamma_n'[t-1] (+) phi[t-1]) + x[t, c],  gamma_b'[t] = (gamma_n'[t-1] (+) gamma_b'[t-1]) + x[t, blank]
  c == eos      psi(g.eos) = gamma_n[n-1] (+) gamma_b[n-1]: the CTC log-likelihood of g itself
  c == blank    -inf; the state of g.blank is -inf throughout (no hypothesis holds a blank)
  increment     delta = psi(g.c) - psi(g), -inf whenever either is -inf: no NaN is ever produced
  offer         an unfinished row's offer for class c is (1 - lam) * logp_att(c) + lam * delta, lam = ctc_weight in (0, 1] (at lam = 1 the
                attention term is dropped, not multiplied by zero)

The search is attention_search_ref.search64's with two differences: (1) each unfinished row's P = pre_beam best attention classes are its
candidates, beam <= P <= min(16, V), default min(16, V, ceil(1.5 beam)); (2) per row the K = beam best of those P by the combined offer --
descending, the lower class first among equal values -- go on to rules 3-5 of that search unchanged.  A kept candidate whose score is -inf (fewer
real candidates than places) is carried along and left out of the result.  Every function takes the array's dtype as its arithmetic: float32
inputs turn the same code into the float32 yardstick."""
import math

import numpy as np
import torch

import attention_search_ref as SR

NEG = float("-inf")


def log_softmax(logits):
    """[n, V] -> x, in the array's dtype, max-shifted."""
    z = logits - logits.max(-1, keepdims=True)
    return z - np.log(np.exp(z).sum(-1, keepdims=True, dtype=logits.dtype))


class State:
    """gamma_n, gamma_b [n], psi and the tokens of a hypothesis."""

    def __init__(self, gn, gb, psi, tokens):
        self.gn, self.gb, self.psi, self.tokens = gn, gb, psi, tuple(tokens)

    @property
    def last(self):
        return self.tokens[-1] if self.tokens else None


def start(x, blank=0):
    return State(np.full(x.shape[0], NEG, dtype=x.dtype), np.cumsum(x[:, blank], dtype=x.dtype), x.dtype.type(0.0), ())


def phi(st, c):
    with np.errstate(invalid="ignore"):
        return st.gb.copy() if c == st.last else np.logaddexp(st.gn, st.gb)


def _init(x, st, c):
    return x[0, c] if not st.tokens else x.dtype.type(NEG)


def psi_ext(x, st, c, blank, eos):
    """psi(g.c), the reduction form: a max-shifted log-sum-exp over t."""
    n = x.shape[0]
    if c == blank or n == 0:
        return x.dtype.type(NEG)
    if c == eos:
        return np.logaddexp(st.gn[n - 1], st.gb[n - 1])
    terms = np.concatenate([np.array([_init(x, st, c)], dtype=x.dtype), phi(st, c)[:n - 1] + x[1:, c]])
    m = terms.max()
    if m == NEG:
        return x.dtype.type(NEG)
    return m + np.log(np.exp(terms - m).sum(dtype=x.dtype))


def delta(psi_c, psi_g):
    return NEG if (psi_c == NEG or psi_g == NEG) else psi_c - psi_g


def offer(logp_att, d, lam):
    if d == NEG:
        return NEG
    return (1.0 - lam) * logp_att + lam * d if lam < 1.0 else lam * d


def extend(x, st, c, blank=0):
    """The state of g.c by the recursion over t; its psi is accumulated inside the recursion (the recursive form of psi_ext)."""
    n = x.shape[0]
    gn, gb = np.full(n, NEG, dtype=x.dtype), np.full(n, NEG, dtype=x.dtype)
    tokens = st.tokens + (int(c),)
    if c == blank or n == 0:
        return State(gn, gb, x.dtype.type(NEG), tokens)
    ph = phi(st, c)
    gn[0] = psi = _init(x, st, c)
    with np.errstate(invalid="ignore"):
        for t in range(1, n):
            gn[t] = np.logaddexp(gn[t - 1], ph[t - 1]) + x[t, c]
            gb[t] = np.logaddexp(gn[t - 1], gb[t - 1]) + x[t, blank]
            psi = np.logaddexp(psi, ph[t - 1] + x[t, c])
    return State(gn, gb, psi, tokens)


def state_of(x, tokens, blank=0):
    st = start(x, blank)
    for c in tokens:
        st = extend(x, st, c, blank)
    return st


def increments(x, tokens, finished, blank, eos):
    """delta at every position of a string (the eos term included when finished): what the search adds, lam aside."""
    st, out = start(x, blank), []
    for c in tokens:
        out.append(delta(psi_ext(x, st, c, blank, eos), st.psi))
        st = extend(x, st, c, blank)
    if finished:
        out.append(delta(psi_ext(x, st, eos, blank, eos), st.psi))
    return out


def default_pre_beam(beam, V):
    return min(16, V, int(math.ceil(1.5 * beam)))


def _gap(kept, dropped):
    return float("inf") if dropped == NEG else kept - dropped


def joint_search64(P, memory, n, x, beam, H, sos, eos, lam, pre_beam=None, blank=0, max_len=None, dtype=torch.float64, round_w=None):
    """One utterance: memory [T, D] and x [>= n, V] of which the first n frames are valid.  Returns dict(nbest=[(tokens, score, finished)] best
    first, gaps, att_gaps, steps).  gaps are differences of COMBINED scores (rank, final: attention_search_ref's), att_gaps differences of
    attention log-probabilities alone -- the pre-beam's boundary, max(logp of the last class admitted - logp of the first one left out, score of the
    last kept candidate - the most the first class left out could have scored: its attention term alone, delta <= 0)."""
    n = int(n)
    out = dict(nbest=[((), 0.0, True)], gaps=[], att_gaps=[], steps=0)
    if n == 0:
        return out
    x = x[:n]
    V = x.shape[1]
    Pb = default_pre_beam(beam, V) if pre_beam is None else int(pre_beam)
    assert beam <= Pb <= min(16, V) and 0.0 < lam <= 1.0 and eos != blank
    max_len = n if max_len is None else int(max_len)
    mem = memory[:n]
    live = [dict(tokens=(sos,), score=0.0, fin=False, st=start(x, blank))]
    for i in range(max_len):
        out["steps"] += 1
        rows = [r for r, a in enumerate(live) if not a["fin"]]
        logp = SR.step_logp(P, [live[r]["tokens"] for r in rows], mem, H, dtype, round_w)
        cands, every, boundary = [], [], []
        for r, a in enumerate(live):
            if a["fin"]:
                cands.append((a["score"], r, eos, a, None))
                every.append(a["score"])
                continue
            v, ix = torch.sort(logp[rows.index(r)], descending=True, stable=True)
            offers = [(float(offer(float(v[j]), delta(psi_ext(x, a["st"], int(ix[j]), blank, eos), a["st"].psi), lam)), int(ix[j])) for j in range(Pb)]
            offers.sort(key=lambda o: (-o[0], o[1]))
            every.extend(a["score"] + o for o, _ in offers)
            cands.extend((a["score"] + o, r, k, a, k) for o, k in offers[:beam])
            if V > Pb:
                boundary.append((float(v[Pb - 1] - v[Pb]), a["score"] + (1.0 - lam) * float(v[Pb])))
        cands.sort(key=SR.order_key)
        every.sort(reverse=True)
        if len(every) > beam:
            out["gaps"].append(_gap(every[beam - 1], every[beam]))
        last_kept = cands[beam - 1][0] if len(cands) >= beam else NEG
        out["att_gaps"].extend(max(g, last_kept - s) for g, s in boundary)
        live = []
        for score, r, k, a, new in cands[:beam]:
            live.append(a if new is None else dict(tokens=a["tokens"] + (k,), score=score, fin=k == eos, st=None if k == eos else extend(x, a["st"], k, blank)))
        if all(a["fin"] for a in live):
            break
    live = [a for a in live if a["score"] > NEG]
    out["gaps"].extend(live[k]["score"] - live[k + 1]["score"] for k in range(len(live) - 1))
    strip = lambda t, fin: tuple(t[1:-1] if fin else t[1:])
    out["nbest"] = [(strip(a["tokens"], a["fin"]), a["score"], a["fin"]) for a in live]
    assert len({(h[0], h[2]) for h in out["nbest"]}) == len(out["nbest"])
    return out


def clear(res, d, d_att):
    return all(g > d for g in res["gaps"]) and all(g > d_att for g in res["att_gaps"])


# -- seeded cases shared by the CPU and the GPU tests ---------------------------------------------------------------------------------------
# name, B, beam, T', V, D, max_len, seed, sharpen, eos bias, modes (attention_search_ref.GPU_CASES' columns: the decoder, memory and lengths are
# attention_search_ref.decoder_for / inputs of the same tuple), then ctc_weight, pre_beam (None: the default), the CTC head's sharpen and its blank bias.
# The last column of the first eleven is the table of CLAIMS: the precision modes under whose delta the float64 joint search alone calls at least
# half of the case's utterances clear at twice the delta (test_ctc_prefix_cpu.py asserts it; the GPU test asserts the clear share only there and
# prints it elsewhere).  The CTC head is a seeded Linear whose weights are multiplied by `ctc sharpen`: its posterior then prefers a few classes per
# frame, which separates the hypotheses by more than the modes' rounding, and whose blank logit gets `blank bias` added: most frames are blank, as with
# a trained head, so the strings have a few tokens and not one per frame.  Chosen with joint_search64 alone.
MODES = SR.MODES
GPU_CASES = [
    ("j_b1_k1", 1, 1, 12, 17, 144, None, 28, 24.0, 14.0, ("bf16", "fp16", "fp32"), 0.3, None, 6.0, 16.0),
    ("j_b3_k4", 3, 4, 20, 17, 256, None, 49, 24.0, 3.0, ("fp16", "fp32"), 0.3, None, 6.0, 16.0),
    ("j_b3_k4_cut2", 3, 4, 12, 17, 256, 2, 49, 24.0, 3.0, ("bf16", "fp16", "fp32"), 0.3, 4, 6.0, 16.0),
    ("j_b16_k10", 16, 10, 12, 17, 144, None, 23, 24.0, 3.0, ("fp32",), 0.3, None, 6.0, 12.0),
    ("j_b3_k16_v5002", 3, 16, 14, 5002, 256, None, 28, 24.0, 8.0, ("fp32",), 0.3, None, 6.0, 16.0),
    ("j_b3_k4_ctc1", 3, 4, 40, 17, 144, None, 25, 24.0, 3.0, ("fp16", "fp32"), 1.0, None, 6.0, 16.0),
]
# A sweep with joint_search64 alone over the head's sharpen in {3, 6, 12} x blank bias in {0, 4, 8, 16} gave, as clear utterances at twice the delta,
# at (6, 16): j_b3_k4 fp16 2 of 3, fp32 3 of 3 (bf16 1: only the utterance without frames, at every setting); j_b3_k4_ctc1 the same; j_b3_k4_cut2 3 of 3 in
# every mode; j_b16_k10 bf16 1, fp16 3, fp32 15 of 16; j_b3_k16_v5002 fp32 2 of 3.  j_b1_k1 (beam 1, so two candidates per step) needs the eos bias of 14:
# below it the single hypothesis outgrows its 12 frames, its score becomes -inf and the n-best list is empty.
# The protocol also bounds the sorted scores of UNCLEAR utterances by delta.  That is no theorem of a beam search: an in-delta swap early on can let a
# different hypothesis survive to the end.  It is a property of the case, so it is checked on the CPU as well (emulated below: this file's search in
# float32 on weights rounded as the mode rounds them, no kernel involved).  At blank bias 16 the B = 16 case broke it in bf16 for one utterance -- the
# emulation gives 3.62 against a delta of 2.67 at the eighth entry, (1, 3, 7) in place of (1, 3, 7, 2, 4), and the device gave 3.65 at the same entry --
# so that case has blank bias 12, where the emulation stays below 0.07 of delta in bf16 and fp16 for all 16 utterances (8, 12 and 24 all do).
BLANK = 0


def ctc_for(case):
    """decoder.CTCDecoder of a case on the CPU in eval mode, seeded (dropout 0: the search applies none anyway)."""
    import decoder
    name, V, D, seed, ctc_sharpen, blank_bias = case[0], case[4], case[5], case[7], case[13], case[14]
    torch.manual_seed(9000 + seed)
    ctc = decoder.CTCDecoder(V, D, 0.0).eval()
    with torch.no_grad():
        ctc.ctc_lo.weight.mul_(ctc_sharpen)
        ctc.ctc_lo.bias[BLANK] += blank_bias
    return ctc


def ctc_logprobs(ctc, memory, dtype=np.float64, round_w=None):
    """x [B, T, V] of the head on memory f32 [B, T, D]: float64, or float32 with the mode's weight rounding."""
    w = ctc.ctc_lo.weight.detach().float()
    w = (round_w(w) if round_w else w).numpy().astype(dtype)
    logits = memory.numpy().astype(dtype) @ w.T + ctc.ctc_lo.bias.detach().numpy().astype(dtype)
    return log_softmax(logits)


def inputs(case):
    """(decoder, ctc head, memory, lens): attention_search_ref.inputs of the case plus its CTC head."""
    dec, memory, lens = SR.inputs(case[:11])
    return dec, ctc_for(case), memory, lens


_cache = {}


def reference(case):
    """joint_search64 per utterance of a case, computed once (sos = eos = V - 1, blank 0)."""
    if case[0] not in _cache:
        name, B, K, T, V, D, max_len, seed, sharpen, eos_bias, modes, lam, pre_beam, _, _ = case
        dec, ctc, memory, lens = inputs(case)
        x = ctc_logprobs(ctc, memory)
        _cache[case[0]] = [joint_search64(dec.state_dict(), memory[b].double(), lens[b], x[b], K, SR.H, V - 1, V - 1, lam, pre_beam, BLANK, max_len) for b in range(B)]
    return _cache[case[0]]


_yard = {}


def yardsticks(mode, case):
    """(attention, CTC prefix): max |float32 with the mode's weight rounding - float64| over every position of the float64 joint search's own n-best
    strings, eos included -- of the attention log-probabilities (attention_search_ref.yardstick's computation on these strings) and of the CTC
    increments delta."""
    import attention_decoder_ref as A
    if (mode, case[0]) not in _yard:
        name, B, K, T, V, D, max_len, seed, sharpen, eos_bias, modes, lam, pre_beam, _, _ = case
        dec, ctc, memory, lens = inputs(case)
        P = dec.state_dict()
        res = reference(case)
        nbest = [[(list(t), s) for t, s, _ in r["nbest"]] for r in res]
        tokens, nlen, score = A.pack_nbest(nbest, N=K)
        tin, tg, mask = A.prep(tokens, nlen, score, V - 1, V - 1)
        mm = (torch.arange(T).unsqueeze(0) < torch.tensor(lens).unsqueeze(1)).unsqueeze(1)
        args = (memory.repeat_interleave(K, 0), mm.repeat_interleave(K, 0), SR.H)
        lp64 = A.token_logp(A.decoder_logits(P, tin, mask, *args), tg)
        lp32 = A.token_logp(A.decoder_logits(P, tin, mask, *args, torch.float32, A.round_trip(mode)), tg)
        att = float((lp32.double() - lp64)[tg >= 0].abs().max()) if bool((tg >= 0).any()) else 0.0
        x64, x32 = ctc_logprobs(ctc, memory), ctc_logprobs(ctc, memory, np.float32, A.round_trip(mode))
        worst = 0.0
        for b, r in enumerate(res):
            for t, _, fin in r["nbest"]:
                if lens[b] == 0:
                    continue
                d64 = increments(x64[b, :lens[b]], t, fin, BLANK, V - 1)
                d32 = increments(x32[b, :lens[b]], t, fin, BLANK, V - 1)
                worst = max([worst] + [abs(float(a) - float(c)) for a, c in zip(d32, d64) if c > NEG])
        _yard[mode, case[0]] = (att, worst)
    return _yard[mode, case[0]]


def deltas(mode, case):
    """Per utterance (delta, attention-only delta): (the longest returned hypothesis + 1) x the per-position gate, the gate
    4 x [(1 - lam) x the attention yardstick + lam x the CTC-prefix yardstick], resp. 4 x the attention yardstick; and the two gates."""
    att, pfx = yardsticks(mode, case)
    lam = case[11]
    gate, gate_att = 4.0 * ((1.0 - lam) * att + lam * pfx), 4.0 * att
    longest = [max([len(t) for t, _, _ in r["nbest"]] + [0]) + 1 for r in reference(case)]
    return [(L * gate, L * gate_att) for L in longest], gate, gate_att


def emulated(mode, case):
    """The worst sorted-score error / delta over a case's utterances of this file's own search run in float32 with the mode's weight rounding (both
    heads) against the float64 reference -- what the device is expected to do, with no kernel involved; inf where the n-best lists differ in length."""
    import attention_decoder_ref as A
    name, B, K, T, V, D, max_len, seed, sharpen, eos_bias, modes, lam, pre_beam, _, _ = case
    dec, ctc, memory, lens = inputs(case)
    P, ds, ref = dec.state_dict(), deltas(mode, case)[0], reference(case)
    x32 = ctc_logprobs(ctc, memory, np.float32, A.round_trip(mode))
    worst = 0.0
    for b in range(B):
        r = joint_search64(P, memory[b].double(), lens[b], x32[b].astype(np.float64), K, SR.H, V - 1, V - 1, lam, pre_beam, BLANK, max_len, torch.float32, A.round_trip(mode))
        if len(r["nbest"]) != len(ref[b]["nbest"]):
            return float("inf")
        worst = max([worst] + [abs(a[1] - c[1]) / ds[b][0] for a, c in zip(r["nbest"], ref[b]["nbest"])])
    return worst
