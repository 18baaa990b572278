"""Pure-Python statement of the edit distance and of ONE optimal alignment -- what cfm_edit_distance (csrc/edit_distance.hip) is compared with, by
equality.  Nothing of the package is imported.

Levenshtein distance between a hypothesis h[0:H] and a reference r[0:U] of integer tokens:

    D[i][0] = i,  D[0][j] = j,  D[i][j] = min(D[i-1][j-1] + (r[i-1] != h[j-1]), D[i-1][j] + 1, D[i][j-1] + 1)          distance = D[U][H]

The split into substitutions, deletions and insertions is not unique, so the definition fixes one alignment: backtrace from (U, H) to (0, 0), taking
the FIRST rule that applies:
    1. i > 0, j > 0 and D[i][j] == D[i-1][j-1] + (r[i-1] != h[j-1]): diagonal -- a hit when the tokens are equal, a substitution otherwise
    2. i > 0 and D[i][j] == D[i-1][j] + 1: a deletion (a reference token with no hypothesis token)
    3. an insertion
The ops are reported in forward order: 1 = hit, 2 = substitution, 3 = deletion, 4 = insertion (0 is padding).

    distance            the table's last cell
    align               (dist, (S, D, I, hits), ops)
    valid               replays ops over both sequences and checks the three identities
    distance_recursive  the same distance as a memoised recursion over (i, j), written without the table
    error_rate          (S + D + I) / reference tokens over a list of pairs: torchmetrics.WordErrorRate's figure
    cases()             the named calls the GPU test runs; expected(name) their alignments, computed once
"""
import functools
import random
import sys

HIT, SUB, DEL, INS = 1, 2, 3, 4
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
POISON = 7                                                     # the token planted in padding columns: a member of every alphabet below that has 8 symbols


def table(h, r):
    H, U = len(h), len(r)
    D = [list(range(H + 1))]
    for i in range(1, U + 1):
        prev, ri = D[-1], r[i - 1]
        cur = [i] * (H + 1)
        left = i
        for j in range(1, H + 1):
            v = prev[j - 1] + (ri != h[j - 1])
            w = prev[j] + 1
            if w < v:
                v = w
            left += 1
            if left < v:
                v = left
            cur[j] = left = v
        D.append(cur)
    return D


def distance(h, r):
    return table(h, r)[len(r)][len(h)]


def align(h, r):
    D = table(h, r)
    i, j = len(r), len(h)
    ops = []
    while i > 0 or j > 0:
        if i > 0 and j > 0 and D[i][j] == D[i - 1][j - 1] + (r[i - 1] != h[j - 1]):
            ops.append(HIT if r[i - 1] == h[j - 1] else SUB)
            i, j = i - 1, j - 1
        elif i > 0 and D[i][j] == D[i - 1][j] + 1:
            ops.append(DEL)
            i -= 1
        else:
            ops.append(INS)
            j -= 1
    ops.reverse()
    return D[len(r)][len(h)], (ops.count(SUB), ops.count(DEL), ops.count(INS), ops.count(HIT)), ops


def valid(ops, h, r, dist=None):
    """ops is an alignment of h to r: hits sit on equal tokens, substitutions on different ones, both sequences are consumed exactly; and
    S + D + I == dist (when given), hits + S + D == U, hits + S + I == H."""
    i = j = 0
    for op in ops:
        if op in (HIT, SUB):
            if i >= len(r) or j >= len(h) or (r[i] == h[j]) != (op == HIT):
                return False
            i, j = i + 1, j + 1
        elif op == DEL:
            i += 1
        elif op == INS:
            j += 1
        else:
            return False
    S, Dn, I, hits = ops.count(SUB), ops.count(DEL), ops.count(INS), ops.count(HIT)
    return (i == len(r) and j == len(h) and hits + S + Dn == len(r) and hits + S + I == len(h) and (dist is None or S + Dn + I == dist))


def distance_recursive(h, r):
    """d(i, j): the distance between r[:i] and h[:j], by what happens to the LAST tokens."""
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 4 * (len(h) + len(r)) + 100))

    @functools.lru_cache(maxsize=None)
    def d(i, j):
        if i == 0 or j == 0:
            return i + j
        if r[i - 1] == h[j - 1]:
            return min(d(i - 1, j - 1), d(i - 1, j) + 1, d(i, j - 1) + 1)
        return 1 + min(d(i - 1, j - 1), d(i - 1, j), d(i, j - 1))
    return d(len(r), len(h))


def error_rate(pairs):
    """pairs: (h, r).  Returns ((S, D, I, hits, reference tokens), rate)."""
    tot = [0, 0, 0, 0, 0]
    for h, r in pairs:
        _, c, _ = align(h, r)
        for k in range(4):
            tot[k] += c[k]
        tot[4] += len(r)
    return tuple(tot), (tot[0] + tot[1] + tot[2]) / tot[4] if tot[4] else float("nan")


# ------------------------------------------------------------------------------------------------------------------------------------- the cases
LENGTHS = (0, 1, 2, 63, 64, 65, 127, 129)


def _seq(rs, n, alphabet):
    return [alphabet[rs.randrange(len(alphabet))] for _ in range(n)]


@functools.lru_cache(maxsize=None)
def cases():
    """Named calls: (name, hyps, refs, ref_index | None, pad) -- pair p is hyps[p] against refs[ref_index[p]] (None: refs[p]); the GPU test packs
    them with `pad` extra columns on both sides, filled with POISON."""
    rs = random.Random(20240)
    A8 = list(range(8))
    out = []
    # every (H, U) of LENGTHS^2 as its own pair of one ragged call
    hyps, refs = [], []
    for H in LENGTHS:
        for U in LENGTHS:
            hyps.append(_seq(rs, H, A8))
            refs.append(_seq(rs, U, A8))
    out.append(("lengths", hyps, refs, None, 3))
    # at the limit: no padding column at all
    out.append(("limit", [_seq(rs, 1024, A8[:4]), _seq(rs, 1024, A8), []], [_seq(rs, 1024, A8[:4]), [], _seq(rs, 1024, A8)], None, 0))
    # content
    base = _seq(rs, 150, A8)
    two_h, two_r = _seq(rs, 140, [0, 1]), _seq(rs, 133, [0, 1])
    ext = [-1, INT32_MIN, INT32_MAX, 0, 1]
    content = [
        ("identical", base, list(base)),
        ("disjoint-long-hyp", _seq(rs, 90, [0, 1, 2, 3]), _seq(rs, 41, [4, 5, 6, 7])),
        ("disjoint-long-ref", _seq(rs, 41, [0, 1, 2, 3]), _seq(rs, 90, [4, 5, 6, 7])),
        ("two-symbols", two_h, two_r),
        ("two-symbols-short", _seq(rs, 9, [0, 1]), _seq(rs, 11, [0, 1])),
        ("hyp-is-prefix", base[:97], base),
        ("ref-is-prefix", base, base[:97]),
        ("hyp-is-suffix", base[53:], base),
        ("ref-is-suffix", base, base[53:]),
        ("hyp-is-strided", base[::3], base),
        ("ref-is-strided", base, base[::3]),
        ("extreme-tokens", _seq(rs, 70, ext), _seq(rs, 66, ext)),
        ("one-repeated-token", [POISON] * 30, [POISON] * 37),
    ]
    out.append(("content", [c[1] for c in content], [c[2] for c in content], None, 5))
    # shared references
    sref = [_seq(rs, 20, A8[:3]), _seq(rs, 70, A8[:3]), []]
    shyp = [_seq(rs, n, A8[:3]) for n in (18, 0, 25, 66, 3, 0, 64)]
    out.append(("shared-refs", shyp, sref, [0, 0, 0, 1, 2, 2, 2], 2))
    # batch shape
    out.append(("P1", [_seq(rs, 33, A8[:3])], [_seq(rs, 30, A8[:3])], None, 1))
    out.append(("P130", [_seq(rs, rs.randrange(0, 41), A8[:3]) for _ in range(130)], [_seq(rs, rs.randrange(0, 41), A8[:3]) for _ in range(130)], None, 1))
    return tuple(out)


CONTENT_NAMES = ("identical", "disjoint-long-hyp", "disjoint-long-ref", "two-symbols", "two-symbols-short", "hyp-is-prefix", "ref-is-prefix", "hyp-is-suffix",
                 "ref-is-suffix", "hyp-is-strided", "ref-is-strided", "extreme-tokens", "one-repeated-token")


def case(name):
    return next(c for c in cases() if c[0] == name)


@functools.lru_cache(maxsize=None)
def expected(name):
    """Per pair of the named call: (dist, (S, D, I, hits), ops).  Computed once and shared."""
    _, hyps, refs, ref_index, _ = case(name)
    return tuple(align(h, refs[p if ref_index is None else ref_index[p]]) for p, h in enumerate(hyps))
