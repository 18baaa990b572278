"""CPU: the definition that cfm_edit_distance is pinned to (tests/edit_distance_ref.py) and the host side of metrics.py.

The distance of the table equals an independent memoised recursion on every pair of sequences of length <= 4 over two letters and on seeded random
pairs up to length 12; the alignment of the tie rule is a valid alignment with the three identities; hand-built ties come out as the rule says."""
import itertools
import random

import pytest
import torch

import edit_distance_ref as ref
import metrics


def _small_pairs():
    seqs = [list(s) for n in range(5) for s in itertools.product((0, 1), repeat=n)]
    pairs = [(h, r) for h in seqs for r in seqs]
    rs = random.Random(7)
    for _ in range(400):
        k = rs.choice((2, 3, 5))
        pairs.append(([rs.randrange(k) for _ in range(rs.randrange(13))], [rs.randrange(k) for _ in range(rs.randrange(13))]))
    return pairs


PAIRS = _small_pairs()


def test_distance_equals_the_independent_recursion():
    assert len(PAIRS) == 31 * 31 + 400
    for h, r in PAIRS:
        assert ref.distance(h, r) == ref.distance_recursive(tuple(h), tuple(r)), (h, r)


def test_alignments_are_valid():
    for h, r in PAIRS:
        dist, (S, D, I, hits), ops = ref.align(h, r)
        assert dist == ref.distance(h, r) and ref.valid(ops, h, r, dist), (h, r, ops)
        assert (S, D, I, hits) == (ops.count(ref.SUB), ops.count(ref.DEL), ops.count(ref.INS), ops.count(ref.HIT))
        assert S + D + I == dist and hits + S + D == len(r) and hits + S + I == len(h)
    assert not ref.valid([ref.HIT], [1], [2]) and not ref.valid([ref.SUB], [1], [1]) and not ref.valid([ref.INS], [1], [2])
    assert not ref.valid([ref.HIT], [1], [1], dist=1)


def test_tie_rule_on_hand_built_ties():
    H, S, D, I = ref.HIT, ref.SUB, ref.DEL, ref.INS
    # r = ab, h = b: distance 1.  From (2, 1) the diagonal applies (b == b), then the deletion of a: forward (D, hit)
    assert ref.align([2], [1, 2]) == (1, (0, 1, 0, 1), [D, H])
    # r = aa, h = a: both "delete the first a" and "delete the second" cost 1; rule 1 applies at (2, 1), so the LAST a is the hit
    assert ref.align([1], [1, 1]) == (1, (0, 1, 0, 1), [D, H])
    # h = aa, r = a: the insertion comes first in forward order for the same reason
    assert ref.align([1, 1], [1]) == (1, (0, 0, 1, 1), [I, H])
    # r = ab, h = ba: distance 2 as two substitutions or as deletion + hit + insertion; the diagonal is tried first: two substitutions
    assert ref.align([2, 1], [1, 2]) == (2, (2, 0, 0, 0), [S, S])
    # r = abc, h = ac: at (3, 2) the hit; at (2, 1) the substitution b/a would cost 2 > D = 1, the deletion applies: (hit, D, hit)
    assert ref.align([1, 3], [1, 2, 3]) == (1, (0, 1, 0, 2), [H, D, H])
    # r = ab, h = xab-like prefix noise: r = [1, 2], h = [9, 1, 2] -> the insertion is the first op
    assert ref.align([9, 1, 2], [1, 2]) == (1, (0, 0, 1, 2), [I, H, H])
    # a substitution beats deletion + insertion on a tie of position: r = [1, 2, 3], h = [1, 9, 3]
    assert ref.align([1, 9, 3], [1, 2, 3]) == (1, (1, 0, 0, 2), [H, S, H])
    # r = [1, 2], h = [2, 2]: diagonal at (2, 2) is a hit, at (1, 1) a substitution (cost 1 == D[1][1])
    assert ref.align([2, 2], [1, 2]) == (1, (1, 0, 0, 1), [S, H])
    # deletion before insertion when the diagonal does not apply: r = [1, 1, 1], h = [2]; at (3, 1) D = 3 == D[2][0] + 1 (sub) -> diagonal first
    assert ref.align([2], [1, 1, 1]) == (3, (1, 2, 0, 0), [D, D, S])
    # empty sides
    assert ref.align([], []) == (0, (0, 0, 0, 0), [])
    assert ref.align([], [5, 6]) == (2, (0, 2, 0, 0), [D, D])
    assert ref.align([5, 6], []) == (2, (0, 0, 2, 0), [I, I])


def test_cases_hold_what_the_gpu_test_needs():
    names = [c[0] for c in ref.cases()]
    assert names == ["lengths", "limit", "content", "shared-refs", "P1", "P130"]
    _, hyps, refs, _, _ = ref.case("lengths")
    assert sorted((len(h), len(r)) for h, r in zip(hyps, refs)) == sorted((H, U) for H in ref.LENGTHS for U in ref.LENGTHS)
    _, hyps, refs, _, pad = ref.case("limit")
    assert [(len(h), len(r)) for h, r in zip(hyps, refs)] == [(1024, 1024), (1024, 0), (0, 1024)] and pad == 0
    _, hyps, refs, _, _ = ref.case("content")
    assert len(hyps) == len(ref.CONTENT_NAMES)
    exp = dict(zip(ref.CONTENT_NAMES, ref.expected("content")))
    assert exp["identical"][0] == 0 and exp["disjoint-long-hyp"][0] == 90 and exp["disjoint-long-ref"][0] == 90
    assert exp["hyp-is-prefix"][0] == 53 and exp["ref-is-suffix"][0] == 53 and exp["hyp-is-strided"][0] == 100 and exp["one-repeated-token"][0] == 7
    toks = set(hyps[ref.CONTENT_NAMES.index("extreme-tokens")])
    assert {-1, ref.INT32_MIN, ref.INT32_MAX} <= toks
    assert ref.case("shared-refs")[3] == [0, 0, 0, 1, 2, 2, 2] and len(ref.case("P130")[1]) == 130


def test_against_torchaudio_when_present():
    F = pytest.importorskip("torchaudio.functional")
    if not hasattr(F, "edit_distance"):
        pytest.skip("torchaudio.functional.edit_distance is not available")
    for h, r in PAIRS[::7]:
        assert ref.distance(h, r) == F.edit_distance(r, h), (h, r)


def test_pack_and_word_ids_round_trip():
    seqs = [[3, -1, 7], [], [2 ** 31 - 1, -2 ** 31], [5]]
    tokens, lens = metrics.pack(seqs, device="cpu")
    assert tokens.dtype == torch.int32 and lens.dtype == torch.int32 and tuple(tokens.shape) == (4, 3) and lens.tolist() == [3, 0, 2, 1]
    assert metrics.unpack(tokens, lens) == seqs
    t0, l0 = metrics.pack([], device="cpu")
    assert tuple(t0.shape) == (0, 0) and tuple(l0.shape) == (0,)
    t1, l1 = metrics.pack([[], []], device="cpu")
    assert tuple(t1.shape) == (2, 0) and l1.tolist() == [0, 0]
    words = metrics.WordIds()
    a = metrics.unpack(*words.encode(["the cat  sat", "", " a cat\tsat\n"], device="cpu"))
    assert a == [[0, 1, 2], [], [3, 1, 2]] and len(words) == 4
    assert words.ids_of("sat on the mat") == [2, 4, 0, 5]                                # known words keep their ids, new ones grow the table
    # a packed operand passes through, any integer dtype
    tok, ln = metrics._packed((torch.tensor([[4, 5, 0]]), [2]), "cpu", "test")
    assert tok.dtype == torch.int32 and ln.tolist() == [2]
    with pytest.raises(ValueError, match="packed operand"):
        metrics._packed((torch.tensor([[4, 5, 0]]), [2, 1]), "cpu", "test")


def test_error_rate_arithmetic_by_hand():
    """Three utterances at word level, worked by hand:
        "the cat sat on the mat" / "the cat sat on mat"   one deletion                          S D I hits = 0 1 0 5, 6 reference words
        "hello world"            / "hello there world !"  two insertions                                     0 0 2 2, 2
        "a b c"                  / "a x c"                one substitution                                   1 0 0 2, 3
    WER = (1 + 2 + 1) / 11."""
    words = metrics.WordIds()
    targets = ["the cat sat on the mat", "hello world", "a b c"]
    preds = ["the cat sat on mat", "hello there world !", "a x c"]
    pairs = [(words.ids_of(p), words.ids_of(t)) for p, t in zip(preds, targets)]
    per_pair = [ref.align(h, r)[1] for h, r in pairs]
    assert per_pair == [(0, 1, 0, 5), (0, 0, 2, 2), (1, 0, 0, 2)]
    sums, rate = ref.error_rate(pairs)
    assert sums == (1, 1, 2, 9, 11) and rate == 4 / 11
    er = metrics.ErrorRate("cpu")
    assert er.compute() != er.compute()                                                  # nan before any reference token
    for c, (h, r) in zip(per_pair, pairs):                                               # one update's arithmetic per utterance
        er.add_counts(torch.tensor([c], dtype=torch.int32), torch.tensor([len(r)], dtype=torch.int32))
    assert er.sums.dtype == torch.int64 and er.counts() == {"S": 1, "D": 1, "I": 2, "hits": 9, "ref_tokens": 11} and er.compute() == 4 / 11
    assert er.reset().counts() == {"S": 0, "D": 0, "I": 0, "hits": 0, "ref_tokens": 0}
