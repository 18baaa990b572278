"""Float64 RNN-T beam search on the CPU -- the specification of greedy.BeamSearch / csrc/greedy.hip's cfm_rnnt_beam_step.  The reference project
has no beam search, so parity is pinned here, and the restatement itself is checked against the full RNN-T likelihood (test_rnnt_beam_cpu.py).

The search is alignment-length synchronous: every live hypothesis has the same t + len.  One step (search64):

  1. logp = log_softmax(joint(enc_proj[t], pred)) per live hypothesis, pred = f(token, h, c) recomputed (greedy_ref.step64)
  2. candidates: the blank (same string, t + 1, fc = 0, the unchanged predictor input) and, unless fc == max_symbols or len == max_len, the
     `beam` best non-blank classes (the lower class first among equal values): string + k, same t, fc + 1, token k, state (h_new, c_new);
     score = parent's score + logp
  3. equal strings merge with logaddexp; only the blank candidate of h1 can meet an extension h2 + k == h1, and it keeps the blank
     candidate's state, t and fc = 0
  4. total order: higher score; then the better-ranked parent; then the blank before the extensions; then the lower class; a merged
     candidate ranks with the better of its sources.  The best `beam` are kept
  5. kept candidates with t == n are finished: they enter F, the best `beam` finished by score (an earlier entry before a later one of the
     same score); the others are the new live set, in rank order
  6. with F full, live entries with score < F's worst are dropped
  7. done when the live set is empty: at most n + max_len + 1 steps

What a result rests on is recorded as `gaps`; a case is CLEAR when every gap exceeds beam_delta: an f32 search then makes the same decisions.
  rank    score of the last kept candidate minus score of the first dropped one
  topk    per live row with more non-blank classes than `beam`: max(logp of the last class offered - logp of the first one not offered,
          score of the last kept candidate - the score the first class not offered would have had).  Either being large makes the choice
          immaterial: the classes are told apart, or neither the class at the boundary nor the one behind it is kept
  finish  F's last kept entry minus the first one dropped, when more than `beam` have finished
  prune   |score - F's worst| for every live entry compared
  final   differences of consecutive n-best scores
"""
import math

import numpy as np
import torch

import greedy_ref as R
import synth

NEG = float("-inf")


def lae(a, b):
    m = max(a, b)
    if m == NEG:
        return NEG
    return m + math.log1p(math.exp(-abs(a - b)))


def search64(P, enc_proj, n, beam, blank=0, max_symbols=64, max_len=None):
    """One utterance: P = greedy_ref.params64, enc_proj (T', J) = enc_ffn(encoder output), n valid frames.  Returns a dict: nbest
    [(tokens tuple, score)] best first, gaps (above), max_abs the largest |score| of a candidate, logit_max the largest |logit|, merges, steps,
    trace: per step the live set after it as (tokens, t, fc, score)."""
    n = int(n)
    max_len = n if max_len is None else int(max_len)
    assert 1 <= beam <= 15 and max_symbols >= 1 and max_len >= 0
    out = dict(nbest=[((), 0.0)], gaps=[], max_abs=0.0, logit_max=0.0, merges=0, steps=0, trace=[])
    if n == 0:
        return out
    L, H = R.num_layers(P), P["p.rnn.weight_hh_l0"].shape[1]
    enc_proj = torch.as_tensor(enc_proj).double().cpu()
    z = torch.zeros((L, H), dtype=torch.float64)
    A = [dict(tokens=(), t=0, fc=0, score=0.0, token=blank, h=z, c=z)]
    F, gaps = [], out["gaps"]
    while A:
        assert out["steps"] <= n + max_len, "more steps than alignments are long"
        out["steps"] += 1
        st = R.step64(P, [a["token"] for a in A], torch.stack([a["h"] for a in A], 1), torch.stack([a["c"] for a in A], 1),
                      torch.stack([enc_proj[a["t"]] for a in A]))
        out["logit_max"] = max(out["logit_max"], float(st["logits"].abs().max()))
        logp = torch.log_softmax(st["logits"], -1)
        cand, boundary = {}, []                              # string -> candidate; (row's last offered logp - first not offered, the latter's score)
        for r, a in enumerate(A):
            cand[a["tokens"]] = dict(a, t=a["t"] + 1, fc=0, score=a["score"] + float(logp[r, blank]), key=(r, 0, 0))
        for r, a in enumerate(A):
            if a["fc"] == max_symbols or len(a["tokens"]) == max_len:
                continue
            lp = logp[r].clone()
            lp[blank] = NEG
            v, i = torch.sort(lp, descending=True, stable=True)
            nb = lp.numel() - 1
            for j in range(min(beam, nb)):
                k, s = int(i[j]), a["score"] + float(v[j])
                new = dict(tokens=a["tokens"] + (k,), t=a["t"], fc=a["fc"] + 1, score=s, token=k, h=st["h_new"][:, r], c=st["c_new"][:, r], key=(r, 1, k))
                old = cand.get(new["tokens"])
                if old is None:
                    cand[new["tokens"]] = new
                else:                                        # the blank candidate of that string: its state, t and fc stay
                    assert old["key"][1] == 0 and old["t"] == new["t"]
                    old["score"], old["key"] = lae(old["score"], s), min(old["key"], new["key"])
                    out["merges"] += 1
            if nb > beam:
                boundary.append((float(v[beam - 1] - v[beam]), a["score"] + float(v[beam])))
        order = sorted(cand.values(), key=lambda x: (-x["score"], x["key"]))
        out["max_abs"] = max([out["max_abs"]] + [abs(x["score"]) for x in order])
        if len(order) > beam:
            gaps.append(order[beam - 1]["score"] - order[beam]["score"])
        last_kept = order[beam - 1]["score"] if len(order) >= beam else NEG
        gaps.extend(max(g, last_kept - s) for g, s in boundary)
        A = []
        for x in order[:beam]:
            if x["t"] < n:
                A.append(x)
                continue
            pos = len(F)
            while pos > 0 and F[pos - 1][1] < x["score"]:
                pos -= 1
            F.insert(pos, (x["tokens"], x["score"]))
            if len(F) > beam:
                gaps.append(F[beam - 1][1] - F[beam][1])
                F.pop()
        if len(F) == beam:
            worst = F[-1][1]
            gaps.extend(abs(x["score"] - worst) for x in A)
            A = [x for x in A if not x["score"] < worst]
        out["trace"].append([(x["tokens"], x["t"], x["fc"], x["score"]) for x in A])
    gaps.extend(F[i][1] - F[i + 1][1] for i in range(len(F) - 1))
    assert len({f[0] for f in F}) == len(F)
    out["nbest"] = F
    return out


def beam_delta(steps, max_abs, logit_err):
    """Margin of the f32 search against the float64 one, on a score and hence on every recorded gap (a gap is a difference of two scores:
    the bound below is used for each side's error, the factor 2 is in it).

    One log-probability logp_k = z_k - lse(z): the f32 joint's logit is off by at most logit_err (absolute: the step kernels' gate times the
    largest |logit|, which also covers the two roundings of `z_k - lse` at that magnitude); lse is 1-Lipschitz in the logits (max norm), so
    it inherits logit_err, and its own evaluation -- expf and logf to 2 ulp, a sum of V terms exp(z - max) in [1, V] accumulated as V / 64
    sequential additions per lane and six across lanes, < 100 roundings of 2^-24 for V <= 5008 -- adds less than 64 * 2^-23.
    A score is a sum over at most `steps` log-probabilities (one per step of its alignment), each addition rounding at most 2^-24 max|score|,
    and meets at most one logaddexp per step, good to a few ulp of its result: 4 * 2^-23 max(1, max|score|) per step, as
    ctc_decode_ref.beam_delta.  Twice the sum, for the two scores of a gap."""
    ulp = 2.0 ** -23
    return 2.0 * steps * ((2.0 * logit_err + 64.0 * ulp) + 4.0 * ulp * max(1.0, max_abs))


def clear(res, delta):
    return all(g > delta for g in res["gaps"])


# -- seeded cases shared by the CPU and the GPU tests ---------------------------------------------------------------------------------------
SMALL = dict(V=73, E=48, H=80, P=96, J=64, L=2, enc_dim=144, seed=51)                    # test_greedy_step_gpu.py's "small" head
CONFIG4 = dict(V=5002, E=256, H=256, P=512, J=512, L=2, enc_dim=512, seed=53)
GATE_STEP = 2e-6                 # test_greedy_step_gpu.py: one fused step's max|d| / max|ref| on the logits against float64
T_SMALL = 12

# name, head, B, beam, max_symbols, blank, max_len (None: the frames), T', input seed, sharpen.  sharpen multiplies ffn_out's weights: the
# synthetic joint's logits stay within +-1.2, a nearly uniform posterior whose candidates lie too close together for most utterances to be
# clear; x 10 gives the peaked posterior of a trained model (chosen with search64 alone, test_rnnt_beam_cpu.py asserts the clear share)
GPU_CASES = [
    ("b1_k1", "small", 1, 1, 3, 0, None, T_SMALL, 11, 10.0),
    ("b64_k1", "small", 64, 1, 1, 0, None, T_SMALL, 12, 10.0),
    ("b5_k3", "small", 5, 3, 3, 0, None, T_SMALL, 13, 10.0),
    ("b8_k8", "small", 8, 8, 1, 0, None, T_SMALL, 14, 10.0),
    ("b4_k15", "small", 4, 15, 3, 0, None, T_SMALL, 15, 10.0),
    ("b16_k4", "small", 16, 4, 3, 0, None, T_SMALL, 16, 10.0),
    ("b5_k3_blank4", "small", 5, 3, 3, 4, None, T_SMALL, 17, 10.0),
    ("b6_k4_maxlen2", "small", 6, 4, 3, 0, 2, T_SMALL, 18, 10.0),
    ("b4_k4_config4", "config4", 4, 4, 3, 0, None, 8, 19, 10.0),
]
# the extension h2 + k meets the blank candidate of h1 == h2 + k: the flat posterior of the unsharpened head keeps a string and its prefix in
# the beam together (found by searching seeds with search64 alone; every utterance is clear)
MERGE_CASE = ("merge", "small", 6, 4, 3, 0, 2, T_SMALL, 18, 1.0)


def head(name, blank=0, sharpen=1.0):
    """(predictor, joint, dims) on the CPU: greedy_ref.modules with synth.greedy_joint_'s shape; a blank other than 0 gets the blank bias too;
    ffn_out's weights times sharpen."""
    h = SMALL if name == "small" else CONFIG4
    pr, jn = R.modules(h["V"], h["E"], h["H"], h["P"], h["J"], h["L"], h["seed"], enc_dim=h["enc_dim"], shaped=True)
    if blank != 0:
        with torch.no_grad():
            jn.ffn_out.bias[blank] += 0.6 if h["V"] < 1000 else 0.8
    with torch.no_grad():
        jn.ffn_out.weight.mul_(sharpen)
    return pr, jn, h


def inputs(case):
    """enc (B, T', enc_dim) f32 and ragged lens (numpy int64) including 0, 1 and T' where B allows: the first utterance is always full."""
    name, hd, B, beam, max_symbols, blank, max_len, T, seed, sharpen = case
    h = SMALL if hd == "small" else CONFIG4
    rs = np.random.RandomState(seed)
    enc = torch.from_numpy(rs.standard_normal((B, T, h["enc_dim"])).astype(np.float32))
    lens = rs.randint(2, T + 1, B)
    lens[0] = T
    if B >= 3:
        lens[-1], lens[1] = 0, 1
    return enc, lens


_cache = {}


def reference(case):
    """search64 per utterance of a case, computed once: (list of result dicts, their delta each)."""
    if case[0] not in _cache:
        name, hd, B, beam, max_symbols, blank, max_len, T, seed, sharpen = case
        pr, jn, h = head(hd, blank, sharpen)
        P = R.params64(pr, jn)
        enc, lens = inputs(case)
        enc_proj = enc.double() @ P["j.enc_ffn.weight"].t() + P["j.enc_ffn.bias"]
        res = [search64(P, enc_proj[b], int(lens[b]), beam, blank, max_symbols, max_len) for b in range(B)]
        _cache[case[0]] = (res, [beam_delta(max(r["steps"], 1), r["max_abs"], GATE_STEP * max(r["logit_max"], 1.0)) for r in res])
    return _cache[case[0]]
