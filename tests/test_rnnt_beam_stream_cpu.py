"""CPU: the float64 streaming RNN-T beam search of tests/rnnt_beam_ref_stream.py, the specification of greedy.StreamingBeamSearch, against
rnnt_beam_ref.search64 on the whole utterance.

  * for every utterance of rnnt_beam_ref.GPU_CASES on the small head and of MERGE_CASE, under six splits of its frames into feeds (1, 3, 5
    per feed, everything at once, idle 0-frame feeds in the middle, a `final` that comes alone), with an explicit max_len: the same n-best
    list -- the same tuples, the same floats --, the same number of steps, the same live set after every step;
  * stable grows along every run, is a prefix of that feed's best and of every entry of the final n-best list, and for some utterance it is
    not empty before `final` (found with the reference alone);
  * a paused stream's state is the same before and after extra steps; n == 0 with final gives [((), 0.0)]."""
import pytest
import torch

import greedy_ref as R
import rnnt_beam_ref as BR
import rnnt_beam_ref_stream as BS

CASES = [c for c in BR.GPU_CASES if c[1] == "small"] + [BR.MERGE_CASE]
SPLITS = ("by1", "by3", "by5", "all", "idle", "final_alone")
explicit_max_len = BS.explicit_max_len


def _case(case):
    """(P, enc_proj (B, T', J) float64, lens, search64 per utterance with the explicit max_len), once per case."""
    return BS.reference(case)[:4]


def _prefix(a, b):
    return tuple(b[:len(a)]) == tuple(a)


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_every_split_is_the_offline_search(case, split):
    name, hd, B, beam, max_symbols, blank, max_len, T, seed, sharpen = case
    P, enc_proj, lens, want = _case(case)
    for b in range(B):
        n = int(lens[b])
        s, reports = BS.run(P, enc_proj[b], n, beam, explicit_max_len(case), BS.splits(n)[split], blank, max_symbols)
        assert s.done and reports[-1]["nbest"] == want[b]["nbest"], (name, b, split)            # tuples and floats, exactly
        assert s.steps == want[b]["steps"] and s.trace == want[b]["trace"] and s.merges == want[b]["merges"], (name, b, split)
        prev = ()
        for r in reports:
            assert _prefix(prev, r["stable"]) and _prefix(r["stable"], r["best"][0]), (name, b, split, prev, r)
            assert all(_prefix(r["stable"], tokens) for tokens, _ in want[b]["nbest"]), (name, b, split, r)
            prev = r["stable"]
        assert all(r["nbest"] is None for r in reports[:-1])


def test_stable_is_not_vacuous():
    """Some utterance has a stable prefix before its last feed; the merge case exercises merging under streaming."""
    seen = 0
    for case in CASES:
        name, hd, B, beam, max_symbols, blank, max_len, T, seed, sharpen = case
        P, enc_proj, lens, want = _case(case)
        for b in range(B):
            n = int(lens[b])
            _, reports = BS.run(P, enc_proj[b], n, beam, explicit_max_len(case), BS.splits(n)["by1"], blank, max_symbols)
            seen += any(len(r["stable"]) > 0 for r in reports[:-1])
    assert seen >= 3, seen
    assert sum(r["merges"] for r in _case(BR.MERGE_CASE)[3]) > 0


def test_a_paused_stream_does_not_change():
    case = CASES[2]
    name, hd, B, beam, max_symbols, blank, max_len, T, seed, sharpen = case
    P, enc_proj, lens, want = _case(case)
    s = BS.Stream64(P, beam, explicit_max_len(case), blank, max_symbols)
    assert s.paused() and not s.step() and s.steps == 0      # no frames: nothing can step
    s.feed(enc_proj[0, :1])
    assert s.paused() and s.steps == 0                       # one frame is the one held back
    s.feed(enc_proj[0, 1:4])
    assert s.paused() and s.steps > 0
    before = (s.live(), s.steps, len(s.trace), [a["h"].clone() for a in s.A])
    for _ in range(5):
        assert not s.step()
    assert (s.live(), s.steps, len(s.trace)) == before[:3] and all(torch.equal(a["h"], h) for a, h in zip(s.A, before[3]))
    assert max(t for _, t, _, _ in s.live()) == s.avail - 1  # it stopped because a hypothesis reached the held-back frame
    r = s.feed(enc_proj[0, 4:int(lens[0])], final=True)
    assert r["nbest"] == want[0]["nbest"]


def test_no_frames_and_final():
    pr, jn, h = BR.head("small")
    P = R.params64(pr, jn)
    s = BS.Stream64(P, 3, 4)
    assert s.feed(torch.zeros((0, h["J"])))["nbest"] is None
    r = s.feed(torch.zeros((0, h["J"])), final=True)
    assert r["nbest"] == [((), 0.0)] and r["best"] == ((), 0.0) and s.steps == 0 and s.done
