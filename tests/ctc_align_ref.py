"""Float64 statement of CTC forced alignment on the CPU -- what cfm_ctc_align (csrc/ctc.hip) is compared with.  numpy and torch on the CPU; nothing of
the package is imported.  The reference project has no forced alignment, so the algorithm is pinned here, and this statement itself is checked against
brute force (test_ctc_align_cpu.py).

For one utterance: lp[t, c] = log_softmax(logits[t, :V])[c], `length` frames, labels y_1..y_U (clamped into [0, V) as the loss clamps them), blank 0,
the extended sequence z = (0, y1, 0, ..., yU, 0) with S = 2U + 1 states.

    delta_0[s] = lp[0, z_s] for s < 2, -inf otherwise
    delta_t[s] = lp[t, z_s] + max(delta_{t-1}[s], delta_{t-1}[s-1], delta_{t-1}[s-2])     the s-2 term only where z_s != 0 and z_s != z_{s-2}

Tie rule (part of the definition): the candidates are taken in the order stay, s-1, s-2, and a later candidate replaces an earlier one only if it is
strictly greater.  The final state is S-2 (the last label) unless delta[S-1] is strictly greater; with U = 0 it is state 0.

    align64         the definition: score, path, start / end / token_logp per label, and the decision gaps along the path
    brute_force     every valid alignment of a tiny lattice, the best one
    decision_gap    how far the optimal path's decisions are from flipping
    delta           the margin of an f32 evaluation: ctc_decode_ref.beam_delta's formula
    path_score      the float64 score of ANY state path, -inf when it is not a valid alignment
    plant           a seeded valid alignment of given length
    cases()         the case table that the CPU test classifies and the GPU test runs
"""
import itertools
import random

import numpy as np
import torch

from ctc_decode_ref import beam_delta

NEG = float("-inf")


def log_probs(logits, V):
    """float64 log_softmax over the first V columns: [T, V]."""
    return torch.log_softmax(torch.as_tensor(logits)[..., :V].double(), -1).numpy()


def extended(labels, V):
    y = [min(max(int(c), 0), V - 1) for c in labels]
    z = [0] * (2 * len(y) + 1)
    z[1::2] = y
    return z


def _skip(z):
    return np.array([s >= 2 and z[s] != 0 and z[s] != z[s - 2] for s in range(len(z))])


def delta(T, score):
    return beam_delta(T, abs(score) if np.isfinite(score) else 0.0)


def align64(lp, labels, length=None):
    """lp f64 [T, V] log-probabilities, labels: the U labels (no padding), length: the valid frames (default all).  Returns a dict:
    score; path int [length] (all -1 when infeasible); start / end int [U] (-1); token_logp f64 [U] (-inf); feasible;
    gaps: per frame t >= 1 of the path, best candidate minus second-best (inf when only one is finite); final_gap: that of the final choice."""
    lp = np.asarray(lp, dtype=np.float64)
    V = lp.shape[1]
    n = lp.shape[0] if length is None else int(length)
    U = len(labels)
    z = extended(labels, V)
    S = len(z)
    bad = dict(score=NEG, path=np.full(n, -1, dtype=np.int64), start=np.full(U, -1, dtype=np.int64), end=np.full(U, -1, dtype=np.int64),
               token_logp=np.full(U, NEG), feasible=False, gaps=[], final_gap=float("inf"))
    if n == 0:
        if U == 0:
            bad.update(score=0.0, feasible=True)
        return bad
    zi, skip = np.array(z), _skip(z)
    d = np.full(S, NEG)
    d[:2] = lp[0, zi[:2]]
    moves = np.zeros((n, S), dtype=np.int64)
    cands = np.full((n, S, 3), NEG)
    for t in range(1, n):
        dp = np.concatenate([[NEG, NEG], d])
        c0, c1, c2 = d, dp[1:S + 1], np.where(skip, dp[:S], NEG)
        best, mv = c0.copy(), np.zeros(S, dtype=np.int64)
        for k, c in ((1, c1), (2, c2)):
            better = c > best                                  # strictly: an earlier candidate keeps a tie
            best, mv = np.where(better, c, best), np.where(better, k, mv)
        cands[t, :, 0], cands[t, :, 1], cands[t, :, 2] = c0, c1, c2
        moves[t] = mv
        d = best + lp[t, zi]
    fin, final_gap = 0, float("inf")
    if S >= 2:
        fin = S - 1 if d[S - 1] > d[S - 2] else S - 2
        lo, hi = sorted((d[S - 1], d[S - 2]))
        final_gap = hi - lo if lo > NEG else float("inf")
    score = float(d[fin])
    if score == NEG:
        return bad
    path = np.zeros(n, dtype=np.int64)
    s, gaps = fin, []
    for t in range(n - 1, -1, -1):
        path[t] = s
        if t > 0:
            c = np.sort(cands[t, s])[::-1]
            gaps.append(float(c[0] - c[1]) if c[1] > NEG else float("inf"))
            s -= moves[t, s]
    out = spans(path, lp, z)
    out.update(score=score, path=path, feasible=True, gaps=gaps[::-1], final_gap=final_gap)
    return out


def spans(path, lp, z):
    """start / end / token_logp per label from a state path: first and last frame whose state is 2u + 1 and the sum of lp[t, y_u] over them."""
    U = (len(z) - 1) // 2
    start, end, tl = np.full(U, -1, dtype=np.int64), np.full(U, -1, dtype=np.int64), np.full(U, NEG)
    for u in range(U):
        frames = np.nonzero(np.asarray(path) == 2 * u + 1)[0]
        if len(frames):
            start[u], end[u] = frames[0], frames[-1]
            tl[u] = float(sum(lp[t, z[2 * u + 1]] for t in range(frames[0], frames[-1] + 1)))
    return dict(start=start, end=end, token_logp=tl)


def decision_gap(res):
    """(minimum over the path's frames of best minus second-best candidate, the final choice's gap) of an align64 result."""
    return (min(res["gaps"]) if res["gaps"] else float("inf")), res["final_gap"]


def valid_path(path, z):
    """Whether the state sequence is a CTC alignment of the extended sequence z."""
    S, skip = len(z), _skip(z)
    if len(path) == 0:
        return S == 1
    if path[0] not in (0, 1) or path[0] >= S or path[-1] not in ((S - 1, S - 2) if S >= 2 else (0,)):
        return False
    for a, b in zip(path[:-1], path[1:]):
        if not (0 <= b < S and (b - a in (0, 1) or (b - a == 2 and skip[b]))):
            return False
    return True


def path_score(path, lp, z):
    """float64 score of a state path; -inf when it is not a valid alignment of z."""
    path = [int(s) for s in path]
    if not valid_path(path, z):
        return NEG
    return float(sum(lp[t, z[s]] for t, s in enumerate(path)))


def brute_force(lp, labels):
    """Every length-len state sequence that is a valid CTC alignment, len <= 6, U <= 3: (best score, its path as a tuple | None)."""
    lp = np.asarray(lp, dtype=np.float64)
    n, U = lp.shape[0], len(labels)
    assert n <= 6 and U <= 3
    z = extended(labels, lp.shape[1])
    if n == 0:
        return (0.0, ()) if U == 0 else (NEG, None)
    best, arg = NEG, None
    for path in itertools.product(range(len(z)), repeat=n):
        if valid_path(path, z):
            sc = float(sum(lp[t, z[s]] for t, s in enumerate(path)))
            if sc > best:
                best, arg = sc, path
    return best, arg


def repeats(labels):
    return sum(1 for a, b in zip(labels[:-1], labels[1:]) if a == b)


def plant(labels, T, seed):
    """A seeded valid alignment (state path, length T) of the labels; T >= U + repeats."""
    rng = random.Random(seed)
    U = len(labels)
    need = U + repeats(labels)
    assert T >= need and (T > 0 or U == 0)
    seq = []
    for u in range(U):
        if u > 0 and labels[u] == labels[u - 1]:
            seq.append(2 * u)
        seq.append(2 * u + 1)
    if not seq:
        return [0] * T
    room = T - len(seq)
    optional = [s for s in range(0, 2 * U + 1, 2) if s not in seq]
    rng.shuffle(optional)
    for s in optional:
        if room > 0 and rng.random() < 0.5:
            seq.append(s)
            room -= 1
    seq.sort()
    while len(seq) < T:
        seq.append(seq[rng.randrange(len(seq))])
    return sorted(seq)


# -- the case table: made here so that the CPU test (which classifies the cases) and the GPU test (which runs them) see the same ones ----------------
# A case is (name, kind, T, lens, labels per utterance, Umax, seed, make); its logits are made for a given V by case_logits().
#   kind "edge": a named shape; "tie": constant logits (the shifted lp' is exactly 0 in f32 and f64, the tie rule decides); "random": seeded.
#   make "randn": 2 * randn;  "const": every logit TIE_LOGIT (not 0: the GPU test's bound on token_logp is relative to max|logit|, and a constant
#   changes no log-probability);  "plant": randn plus 12 on a planted alignment's classes (long cases: |score| stays small, so delta does, and
#   the decisions along the path are clear by construction -- the shape, not the margin, is what these cases are for).
TB = 64                                                       # csrc/ctc.hip VIT_TB: frames per trace-back block
TIE_LOGIT = 3.0


def _labels(V, U, seed, pattern=None):
    """U labels in [1, V): seeded, or a pattern of letters mapped to distinct classes (a -> 1, b -> 2, ...; V = 3 keeps it to two classes)."""
    if pattern is not None:
        return [1 + (ord(ch) - ord("a")) % (V - 1) for ch in pattern]
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(1, V, (U,), generator=g)).tolist()


def cases(V):
    """[(name, kind, T, lens, labels list, Umax, seed, make)] for vocabulary V."""
    out = []
    add = lambda name, kind, T, lens, labels, Umax=None, seed=0, make="randn": out.append(
        (name, kind, T, lens, labels, Umax or max(1, max(len(l) for l in labels)), seed, make))
    add("T1-U0", "edge", 1, [1], [[]], seed=1)
    add("T1-U1", "edge", 1, [1], [_labels(V, 1, 2)], seed=2)
    ab = _labels(V, 4, 0, "abab")
    add("T==U", "edge", 4, [4], [ab], seed=3)
    aab = _labels(V, 3, 0, "aab")
    add("T==U+repeats", "edge", 4, [4], [aab], seed=4)
    add("T==U+repeats-1", "edge", 3, [3], [aab], seed=5)
    add("U0-T5", "edge", 5, [5], [[]], seed=6)
    add("ragged", "edge", 5, [0, 5, 2], [[], _labels(V, 2, 7), _labels(V, 1, 8)], Umax=4, seed=7)
    for T in (4, 5, 9):
        add("ahead-T%d" % T, "edge", T, [T], [_labels(V, 2, 10 + T)], seed=10 + T)
    for T in (67, TB - 1, TB, TB + 1, 2 * TB + 1):
        add("block-T%d" % T, "edge", T, [T, T - 3], [_labels(V, 9, 20 + T), _labels(V, 5, 21 + T)], seed=20 + T, make="plant")
    add("U128-T300", "edge", 300, [300], [_labels(V, 128, 30)], seed=30, make="plant")
    add("U255-T600", "edge", 600, [600], [_labels(V, 255, 31)], seed=31, make="plant")
    add("clamped", "edge", 9, [9], [[1, V + 5, -3, 1]], seed=32)
    add("tie-aa-T5", "tie", 5, [5], [[1, 1]], make="const")
    add("tie-U0-T4", "tie", 4, [4], [[]], make="const")
    add("tie-ab-T7", "tie", 7, [7, 3], [_labels(V, 2, 0, "ab"), _labels(V, 2, 0, "ab")], make="const")
    for i in range(12):
        T, U = (6, 2) if i % 3 == 0 else (17, 5) if i % 3 == 1 else (40, 11)
        add("random-%d" % i, "random", T, [T, max(T - 5, 1), T], [_labels(V, U, 100 + i), _labels(V, max(U - 1, 1), 200 + i), _labels(V, U, 300 + i)],
            seed=RANDOM_SEEDS[i])
    return out


# seeds of the random cases, chosen on the CPU (test_ctc_align_cpu.py asserts the share of exact cases they give for every V)
RANDOM_SEEDS = [500 + i for i in range(12)]


def case_logits(V, case):
    """f32 logits [B, T, V] of a case (frames at and beyond an utterance's length hold noise too)."""
    name, kind, T, lens, labels, Umax, seed, make = case
    B = len(lens)
    if make == "const":
        return torch.full((B, T, V), TIE_LOGIT)
    g = torch.Generator().manual_seed(1000 * seed + V)
    if make == "randn":
        return 2.0 * torch.randn((B, T, V), generator=g)
    x = torch.randn((B, T, V), generator=g)
    for b in range(B):
        z = extended(labels[b], V)
        for t, s in enumerate(plant([z[2 * u + 1] for u in range(len(labels[b]))], lens[b], seed + b)):
            x[b, t, z[s]] += 12.0
    return x


def padded_labels(labels, Umax, fill=1):
    out = torch.full((len(labels), Umax), fill, dtype=torch.int32)
    for b, l in enumerate(labels):
        if l:
            out[b, :len(l)] = torch.tensor(l, dtype=torch.int32)
    return out


_results = {}


def case_reference(V, case):
    """(logits f32 [B,T,V], [align64 result per utterance]) -- computed once per (V, case) and shared."""
    key = (V, case[0])
    if key not in _results:
        logits = case_logits(V, case)
        res = []
        for b, n in enumerate(case[3]):
            lp = log_probs(logits[b, :n], V)
            r = align64(lp, case[4][b], n)
            r["lp"] = lp
            res.append(r)
        _results[key] = (logits, res)
    return _results[key]


def exact(res, T):
    """An utterance whose every decision along the optimal path is further than delta from flipping: an f32 evaluation gives the same path."""
    return min(decision_gap(res)) > delta(T, res["score"])
