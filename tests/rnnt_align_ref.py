"""Float64 statement of RNN-T forced alignment on the CPU -- what cfm_rnnt_align / cfm_rnnt_packed_align (csrc/rnnt.hip) are compared with.  numpy
and torch on the CPU; of the tests only rnnt_ref (the loss's float64 statement, whose lattice_logprobs gives the node log-probabilities) is imported,
nothing of the package.  The reference project has no forced alignment, so the algorithm is pinned here, and this statement itself is checked against
brute force (test_rnnt_align_cpu.py).

For one utterance: lb[t,u] / ll[t,u] = the blank / label log-probability of node (t,u) (log_softmax over V; labels clamped into [0, V) as the loss
clamps them), Tb = logit_len clamped to [0, T], Ub = target_len clamped to [0, U1-1]:

    delta[0,0] = 0
    delta[t,u] = max( delta[t-1,u] + lb[t-1,u]      (blank move, only where t > 0),
                      delta[t,u-1] + ll[t,u-1] )    (label move, only where u > 0)
    score      = delta[Tb-1,Ub] + lb[Tb-1,Ub]

Tie rule (part of the definition): the blank move is taken first; the label move replaces it only if it is strictly greater.  From (Tb-1, Ub) the
recorded moves are followed back to (0,0); frame[u] is the t of the label move (t,u) -> (t,u+1), token_logp[u] = ll[frame[u], u].  Tb == 0 has no
alignment (the final blank needs a frame): score -inf.  Entries u >= Ub, and all of an utterance without an alignment, are -1 / -inf.

    node_logprobs   (lb, ll) f64 [B,T,U1] of a batch (rnnt_ref.lattice_logprobs on the first V columns)
    align64         the definition: score, frames, token_logp, and the decision gaps along the path (dtype=np.float32: the same recursion in f32)
    brute_force     every path of a tiny lattice: the best score, its frames, whether it is unique
    path_score      the float64 score of ANY frame list, -inf when it is not a valid alignment
    delta           the margin of an f32 evaluation
    exact           every decision along the optimal path is further than 2 delta from flipping
    cases(V)        the case table that the CPU test classifies and the GPU test runs
"""
import collections
import itertools

import numpy as np
import torch

import rnnt_ref

NEG = float("-inf")
F32_REL = 2e-6                                               # tests/test_greedy_step_gpu.py: the f32 figure of a log-probability, relative to max|logit|
RNNT_AHEAD = 4                                               # csrc/rnnt.hip
TIE_LOGIT = 3.0
BOOST = 12.0


def node_logprobs(logits, targets, blank, V):
    """(lb, ll) float64 numpy [B,T,U1] from logits [B,T,U1,>=V] (any float dtype, widened) and targets [B,U1-1]; ll[..., U1-1] is never read."""
    lb, ll = rnnt_ref.lattice_logprobs(torch.as_tensor(logits)[..., :V], torch.as_tensor(targets), blank)
    return lb.numpy(), ll.numpy()


def delta(Tb, Ub, score, lmax):
    """ctc_align_ref.delta's form with Tb + Ub moves in place of T frames, plus the row pass's error per move."""
    n = Tb + Ub
    return 4 * n * 2.0 ** -23 * max(1.0, abs(score) if np.isfinite(score) else 0.0) + n * F32_REL * lmax


def align64(lb, ll, Tb, Ub, dtype=np.float64):
    """lb / ll [>=Tb, >=Ub+1] node log-probabilities of ONE utterance.  Returns a dict: score; frames int64 [Ub]; token_logp [Ub]; feasible;
    gaps: |blank candidate - label candidate| at every node of the path where both moves exist (inf elsewhere), in path order."""
    Tb, Ub = int(Tb), int(Ub)
    if Tb == 0:
        return dict(score=NEG, frames=np.full(Ub, -1, dtype=np.int64), token_logp=np.full(Ub, NEG), feasible=False, gaps=[], Tb=Tb, Ub=Ub)
    lb, ll = np.asarray(lb, dtype=dtype), np.asarray(ll, dtype=dtype)
    d = np.full((Tb, Ub + 1), NEG, dtype=dtype)
    label = np.zeros((Tb, Ub + 1), dtype=bool)
    gap = np.full((Tb, Ub + 1), np.inf)
    d[0, 0] = 0
    for t in range(Tb):
        for u in range(Ub + 1):
            if t == 0 and u == 0:
                continue
            if t == 0:
                d[t, u], label[t, u] = d[t, u - 1] + ll[t, u - 1], True
            elif u == 0:
                d[t, u] = d[t - 1, u] + lb[t - 1, u]
            else:
                cb, cl = d[t - 1, u] + lb[t - 1, u], d[t, u - 1] + ll[t, u - 1]
                label[t, u] = cl > cb                                # strictly: the blank move keeps a tie
                d[t, u] = cl if label[t, u] else cb
                if np.isfinite(cb) and np.isfinite(cl):
                    gap[t, u] = abs(float(cl) - float(cb))
    score = float(d[Tb - 1, Ub] + lb[Tb - 1, Ub])
    frames, gaps = np.zeros(Ub, dtype=np.int64), []
    t, u = Tb - 1, Ub
    while (t, u) != (0, 0):
        gaps.append(float(gap[t, u]))
        if label[t, u]:
            u -= 1
            frames[u] = t
        else:
            t -= 1
    return dict(score=score, frames=frames, token_logp=np.array([float(ll[frames[k], k]) for k in range(Ub)]), feasible=True, gaps=gaps[::-1], Tb=Tb, Ub=Ub)


def path_score(frames, lb, ll):
    """float64 score of the alignment that emits label u at frame frames[u], on lb / ll [Tb, >= len(frames) + 1]; -inf for a list that is not
    nondecreasing or leaves [0, Tb-1] (and for Tb == 0)."""
    lb, ll = np.asarray(lb, dtype=np.float64), np.asarray(ll, dtype=np.float64)
    Tb, frames = lb.shape[0], [int(f) for f in frames]
    if Tb == 0 or any(f < 0 or f >= Tb for f in frames) or any(a > b for a, b in zip(frames[:-1], frames[1:])):
        return NEG
    s, t = 0.0, 0
    for u, f in enumerate(frames):
        s += float(lb[t:f, u].sum()) + float(ll[f, u])                   # the blanks of column u, then label u at frame f
        t = f
    return s + float(lb[t:Tb, len(frames)].sum())                        # the last column's blanks, the final one included


def brute_force(lb, ll, Tb, Ub):
    """Every one of the C(Tb-1+Ub, Ub) paths of a tiny lattice, as rnnt_ref.brute_force_cost with max in place of the sum:
    (best score, its frames as a tuple | None, whether no other path comes within 1e-9)."""
    assert Tb <= 6 and Ub <= 5
    if Tb == 0:
        return NEG, None, True
    scores = []
    for labels_at in itertools.combinations(range(Tb - 1 + Ub), Ub):
        t = u = 0
        s, frames = 0.0, []
        for k in range(Tb - 1 + Ub):
            if k in labels_at:
                s += float(ll[t, u])
                frames.append(t)
                u += 1
            else:
                s += float(lb[t, u])
                t += 1
        scores.append((s + float(lb[Tb - 1, Ub]), tuple(frames)))
    scores.sort(key=lambda p: -p[0])
    return scores[0][0], scores[0][1], len(scores) == 1 or scores[0][0] - scores[1][0] > 1e-9


def exact(res):
    """An utterance (a case_reference result) whose every decision along the float64 optimal path is further than 2 delta from flipping (each
    of the two candidates carries up to delta): an f32 evaluation gives the same frames."""
    return res["feasible"] and min(res["gaps"], default=float("inf")) > 2 * delta(res["Tb"], res["Ub"], res["score"], res["lmax"])


# -- the case table: made here so that the CPU test (which classifies the cases) and the GPU test (which runs them) see the same ones ----------------
#   kind "edge": a named shape; "tie": constant logits (the shifted values are exactly 0 in f32 and f64, the tie rule decides); "random": seeded;
#   "peaked": one path dominates.  make "randn": 2 * randn; "const": every logit TIE_LOGIT; "plant": randn plus BOOST on a seeded path's classes
#   (the long cases: |score| stays small, so delta does, and the decisions along the path are clear by construction -- the shape, not the margin,
#   is what these cases are for); "peak": randn plus 30 on the path.
Case = collections.namedtuple("Case", "name kind T U logit_lens target_lens blank seed make")
RANDOM_SEEDS = [700 + i for i in range(9)]                   # chosen on the CPU (test_rnnt_align_cpu.py asserts the share of exact utterances)


def cases(V):
    """The named cases for vocabulary V.  Lengths may exceed the tensor sizes or be negative (clamped)."""
    out = []
    add = lambda name, kind, T, U, tl, ul, seed, make="randn", blank=0 if V == 17 else V - 1: out.append(Case(name, kind, T, U, tl, ul, blank, seed, make))
    add("U0-T5", "edge", 5, 0, [5], [0], 1)
    add("T1-U3", "edge", 1, 3, [1], [3], 2)
    add("Tb0-beside-live", "edge", 6, 3, [6, 0, 4], [3, 2, 0], 3)
    add("ragged-clamped", "edge", 7, 4, [9, 5, -2, 7], [6, 2, 3, 4], 4)
    if V == 3:
        for U1 in (2, 255, 256, 257, 1024):
            add("U1=%d-T3" % U1, "edge", 3, U1 - 1, [3], [U1 - 1], 10 + U1, "plant")
    for T in (RNNT_AHEAD - 1, RNNT_AHEAD, RNNT_AHEAD + 1, 2 * RNNT_AHEAD + 1):
        add("ahead-T%d" % T, "edge", T, 2, [T], [2], 20 + T)
    add("T300-U2", "edge", 300, 2, [300], [2], 30, "plant")
    add("tie", "tie", 6, 3, [6, 3], [3, 2], 0, "const")
    add("peaked", "peaked", 12, 5, [12, 9], [5, 3], 40, "peak")
    for i, seed in enumerate(RANDOM_SEEDS):
        T, U = ((6, 2), (13, 5), (24, 9))[i % 3]
        add("random-%d" % i, "random", T, U, [T, max(T - 5, 1), T], [U, U, max(U - 2, 0)], seed)
    return out


def clamped_lens(case):
    return [min(max(n, 0), case.T) for n in case.logit_lens], [min(max(n, 0), case.U) for n in case.target_lens]


def plant(Tb, Ub, seed):
    """A seeded alignment: nondecreasing frames in [0, Tb-1], one per label."""
    rs = np.random.RandomState(seed)
    return sorted(int(f) for f in rs.randint(0, Tb, Ub)) if Tb > 0 else []


def case_inputs(V, case):
    """(logits f32 [B,T,U+1,V], targets int32 [B,U]): labels differ from the blank; "ragged-clamped" carries labels outside [0, V) (clamped by the
    op); nodes beyond an utterance's lengths hold noise too."""
    B, T, U = len(case.logit_lens), case.T, case.U
    g = torch.Generator().manual_seed(1000 * case.seed + V)
    targets = torch.randint(0, V - 1, (B, U), generator=g)
    targets = (targets + (targets >= case.blank).long()).to(torch.int32)
    if case.name == "ragged-clamped":
        targets[0, 1], targets[1, 0] = V + 5, -3
    if case.make == "const":
        return torch.full((B, T, U + 1, V), TIE_LOGIT), targets
    if case.make == "randn":
        return 2.0 * torch.randn((B, T, U + 1, V), generator=g), targets
    x = torch.randn((B, T, U + 1, V), generator=g)
    Tl, Ul = clamped_lens(case)
    for b in range(B):
        frames, t = plant(Tl[b], Ul[b], case.seed + b), 0
        for u, f in enumerate(frames + [Tl[b]]):                        # column u: blanks on frames t..f-1, then label u at frame f (the last column: blanks to the end)
            x[b, t:f, u, case.blank] += BOOST if case.make == "plant" else 30.0
            if u < len(frames):
                x[b, f, u, int(targets[b, u].clamp(0, V - 1))] += BOOST if case.make == "plant" else 30.0
            t = f
    return x, targets


_results = {}


def reference(logits, targets, logit_lens, target_lens, blank, V):
    """[align64 result per utterance] of a batch, each with its lb / ll [Tb, Ub+1] slices, Tb, Ub and lmax = max|logit| of the batch."""
    lb, ll = node_logprobs(logits, targets, blank, V)
    T, U1 = lb.shape[1:]
    lmax, res = float(torch.as_tensor(logits)[..., :V].double().abs().max()), []
    for b in range(lb.shape[0]):
        Tb, Ub = min(max(int(logit_lens[b]), 0), T), min(max(int(target_lens[b]), 0), U1 - 1)
        r = align64(lb[b], ll[b], Tb, Ub)
        r.update(lb=lb[b, :Tb, :Ub + 1], ll=ll[b, :Tb, :Ub + 1], lmax=lmax)
        res.append(r)
    return res


def case_reference(V, case):
    """(logits, targets, [reference result per utterance]) -- computed once per (V, case) and shared."""
    key = (V, case.name)
    if key not in _results:
        logits, targets = case_inputs(V, case)
        _results[key] = (logits, targets, reference(logits, targets, case.logit_lens, case.target_lens, case.blank, V))
    return _results[key]
