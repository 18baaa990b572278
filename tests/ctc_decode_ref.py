"""Float64 restatements of CTC decoding on the CPU -- what csrc/ctc_decode.hip is compared with.  Plain Python and torch; nothing of the package
is imported.  The reference project has no CTC decoder, so parity is pinned here, and the restatement itself is checked against brute force
(test_ctc_decode_cpu.py).

    topk64               float64 log_softmax, then a stable descending sort over the ascending class index
    best_path            argmax per frame, repeats collapsed, blanks dropped: tokens, their frames, their log-probabilities
    prefix_beam_search64 CTC prefix beam search with a dictionary keyed by the token tuple
    brute_force          every alignment of a tiny lattice: the exact log-posterior of every label string

The ranking of prefix_beam_search64 is total (include/cfm.h cfm_ctc_prefix_beam): higher score logaddexp(pb, pnb); on equal scores the candidate
that continues the better-ranked parent; then the prefix itself before its extensions; then the lower class.  A candidate fed from two sources
(a prefix that returned to the beam meets its surviving extension) ranks with the smaller of the two keys.  A score of -inf is no candidate."""
import itertools
import math

import torch

NEG = float("-inf")


def lae(a, b):
    m = max(a, b)
    if m == NEG:
        return NEG
    return m + math.log1p(math.exp(-abs(a - b)))


def topk64(logits, k):
    """logits [..., V] (any float dtype) -> (idx int64 [..., k], logp f64 [..., k], lse f64 [...]): descending, lower class first on ties."""
    x = logits.double()
    lse = torch.logsumexp(x, dim=-1)
    lp = x - lse[..., None]
    v, i = torch.sort(lp, dim=-1, descending=True, stable=True)
    return i[..., :k], v[..., :k], lse


def best_path(idx1, logp1, n, blank=0, prev=-1, frame_base=0):
    """idx1 / logp1: per frame the best class and its log-probability (sequences of length >= n).  Returns (tokens, frames, logps, last class)."""
    toks, frames, lps = [], [], []
    for t in range(n):
        c = int(idx1[t])
        if c != prev and c != blank:
            toks.append(c)
            frames.append(frame_base + t)
            lps.append(float(logp1[t]))
        prev = c
    return toks, frames, lps, prev


def prefix_beam_search64(idx, logp, n, beam, blank=0):
    """idx [T, k >= beam] classes, logp [T, k] their log-probabilities (the first `beam` columns are used), n valid frames.  Returns a dict:
    nbest        [(tokens tuple, score)] best first, at most `beam`
    frame_gaps   per frame with more candidates than the beam holds: score of the last kept minus score of the first dropped
    nbest_gaps   differences of consecutive n-best scores
    max_abs      the largest |score| among the candidates seen
    reentry      number of times an extension l + c was merged into a beam entry OLDER than l's current stay in the beam (l left the beam and
                 came back while l + c stayed)"""
    idx = [[int(c) for c in row[:beam]] for row in idx.tolist()]
    logp = [[float(p) for p in row[:beam]] for row in logp.tolist()]
    cur = [((), 0.0, NEG)]                                    # rank order: (prefix, pb, pnb)
    born = {(): -1}                                           # frame at which each beam entry's current stay began
    frame_gaps, max_abs, reentry = [], 0.0, 0
    for t in range(n):
        nxt = {}                                              # prefix -> [pb, pnb, key]

        def add(prefix, which, val, key):
            if val == NEG:
                return
            e = nxt.setdefault(prefix, [NEG, NEG, key])
            e[which] = lae(e[which], val)
            e[2] = min(e[2], key)

        present = {l for l, _, _ in cur}
        for r, (l, pb, pnb) in enumerate(cur):
            for c, p in zip(idx[t], logp[t]):
                if c == blank:
                    add(l, 0, lae(pb, pnb) + p, (r, 0, 0))
                elif l and c == l[-1]:
                    add(l, 1, pnb + p, (r, 0, 0))
                    add(l + (c,), 1, pb + p, (r, 1, c))
                    if pb + p > NEG and l + (c,) in present and born[l + (c,)] < born[l]:
                        reentry += 1
                else:
                    add(l + (c,), 1, lae(pb, pnb) + p, (r, 1, c))
                    if lae(pb, pnb) + p > NEG and l + (c,) in present and born[l + (c,)] < born[l]:
                        reentry += 1
        cand = [(l, e[0], e[1], lae(e[0], e[1]), e[2]) for l, e in nxt.items()]
        cand = [x for x in cand if x[3] > NEG]
        cand.sort(key=lambda x: (-x[3], x[4]))
        for x in cand:
            max_abs = max(max_abs, abs(x[3]))
        if len(cand) > beam:
            frame_gaps.append(cand[beam - 1][3] - cand[beam][3])
        cand = cand[:beam]
        born = {x[0]: (born[x[0]] if x[0] in present else t) for x in cand}
        cur = [(x[0], x[1], x[2]) for x in cand]
        if not cur:
            break
    nbest = [(l, lae(pb, pnb)) for l, pb, pnb in cur]
    return dict(nbest=nbest, frame_gaps=frame_gaps, nbest_gaps=[nbest[i][1] - nbest[i + 1][1] for i in range(len(nbest) - 1)], max_abs=max_abs, reentry=reentry)


def collapse(path, blank=0):
    out, prev = [], None
    for c in path:
        if c != prev and c != blank:
            out.append(c)
        prev = c
    return tuple(out)


def brute_force(lp, blank=0):
    """lp f64 [T, V] log-probabilities, V <= 4, T <= 6.  Returns {label string: log of the summed probability of its alignments}."""
    T, V = lp.shape
    assert V <= 4 and T <= 6
    rows = lp.tolist()
    acc = {}
    for path in itertools.product(range(V), repeat=T):
        s = sum(rows[t][c] for t, c in enumerate(path))
        acc.setdefault(collapse(path, blank), []).append(s)
    out = {}
    for l, vals in acc.items():
        m = max(vals)
        out[l] = m + math.log(math.fsum(math.exp(v - m) for v in vals)) if m > NEG else NEG
    return out


# -- the random cases of the prefix-beam tests: made here so that the CPU and the GPU test see the same ones ---------------------------------
BEAM_CASES = [(V, T, beam) for V in (4, 6) for T in (1, 12, 40) for beam in (1, 3, 4, 16)]


def beam_case(seed, V, T, beam, blank=0, B=4):
    """One random case: int32 idx / f32 logp [B, T, k = min(beam, V)] as a top-k of a random f32 posterior with a heavy blank, ragged lens incl. 0."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn((B, T, V), generator=g) * 1.5
    logits[..., blank] += 1.5                                 # blank probable enough that prefixes drop out and come back
    lp = torch.log_softmax(logits.double(), -1).float()
    v, i = torch.sort(lp, dim=-1, descending=True, stable=True)
    lens = torch.randint(1, T + 1, (B,), generator=g)
    lens[0] = T
    if B > 1:
        lens[-1] = 0
    k = min(beam, V)
    return i[..., :k].to(torch.int32).contiguous(), v[..., :k].contiguous(), lens.to(torch.int32)


def beam_delta(T, max_abs):
    """Margin of an f32 prefix beam search against the float64 one: each f32 logaddexp is good to a few ulp of its result, a score accumulates at
    most T of them -- delta = 4 T 2^-23 max(1, max |score|)."""
    return 4.0 * T * 2.0 ** -23 * max(1.0, max_abs)


def beam_cases_64():
    """The 64 seeded cases of test_prefix_beam: [(seed, V, T, beam)]; every (V, T, beam) combination at least twice."""
    out = []
    seed = 1000
    while len(out) < 64:
        V, T, beam = BEAM_CASES[len(out) % len(BEAM_CASES)]
        out.append((seed, V, T, beam))
        seed += 1
    return out


# A prefix leaves the beam and comes back while its extension stays, then meets it again (found by searching seeds with prefix_beam_search64
# alone; test_ctc_decode_cpu.py asserts the event and that the case is clear): (seed, V, T, beam)
REENTRY_CASE = (2017, 4, 40, 3)
