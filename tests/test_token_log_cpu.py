"""CPU: token_log.TokenLog / token_log.grow, the host side of the accumulating hypothesis buffer of greedy.ChunkGreedySearch and
decoder.CTCGreedyStream, against plain slicing of a full host copy: ragged counts over four chunks, a chunk without emissions (no read of
the buffer at all), a chunk in which only the stream with the smallest count emits (the column window's offsets), a partial reset and a
grow that keeps the old columns."""
import torch

import token_log


class _Spy:
    """The device buffer as TokenLog sees it: indexable, and it counts how often it was indexed."""

    def __init__(self, t):
        self.t, self.reads = t, 0

    def __getitem__(self, idx):
        self.reads += 1
        return self.t[idx]


def _emit(S, b, tokens):
    """What a decoding step does on the device: append at the stream's count."""
    n = int(S["count"][b])
    for k in ("hyps", "frames"):
        S[k][b, n:n + len(tokens)] = torch.tensor(tokens, dtype=S[k].dtype) * (1 if k == "hyps" else -1)
    S["count"][b] += len(tokens)


def _take(log, S):
    """One take against slicing a full host copy per stream; returns (new tokens, reads of the buffer)."""
    old, counts, spy = list(log.count), S["count"].tolist(), _Spy(S["hyps"])
    new = log.take(spy, counts)
    full = S["hyps"].clone()
    assert new == [full[b, old[b]:counts[b]].tolist() for b in range(len(counts))]
    assert log.count == counts and log.most() == max(counts)
    return new, spy.reads


def test_token_log_over_four_chunks_with_reset_and_grow():
    B = 3
    S = dict(hyps=torch.zeros((B, 2), dtype=torch.int64), frames=torch.zeros((B, 2), dtype=torch.int32), count=torch.zeros(B, dtype=torch.int64))
    log = token_log.TokenLog(B)
    assert log.hyps() == [[], [], []] and log.most() == 0
    # chunk 1: ragged counts 2, 1, 0 in a buffer of 2 columns
    _emit(S, 0, [11, 12])
    _emit(S, 1, [21])
    new, reads = _take(log, S)
    assert new == [[11, 12], [21], []] and reads == 1
    # the next chunk may add 3 per stream: 2 + 3 = 5 > 2 columns
    before = {k: S[k].clone() for k in ("hyps", "frames")}
    assert token_log.grow(S, ("hyps", "frames"), log.most() + 3)
    for k in ("hyps", "frames"):
        assert S[k].shape == (B, 5) and S[k].dtype == before[k].dtype and torch.equal(S[k][:, :2], before[k]) and not S[k][:, 2:].any()
    assert not token_log.grow(S, ("hyps", "frames"), 5) and S["hyps"].shape == (B, 5)              # it fits: nothing is replaced
    # chunk 2: nobody emits -- empty lists, and the buffer is not touched although the counts are ragged
    new, reads = _take(log, S)
    assert new == [[], [], []] and reads == 0
    # chunk 3: only the stream with the smallest count emits: the window is [0, 2), the others' slices in it are empty
    _emit(S, 2, [31, 32])
    new, reads = _take(log, S)
    assert new == [[], [], [31, 32]] and reads == 1
    assert log.hyps() == [[11, 12], [21], [31, 32]]
    # stream 1 starts a new utterance
    log.reset([1])
    for k in ("hyps", "frames", "count"):
        S[k][1] = 0
    assert log.count == [2, 0, 2] and log.hyps() == [[11, 12], [], [31, 32]]
    # chunk 4: everybody emits, stream 1 from column 0 again
    _emit(S, 0, [13, 14, 15])
    _emit(S, 1, [22, 23])
    _emit(S, 2, [33, 34])
    new, reads = _take(log, S)
    assert new == [[13, 14, 15], [22, 23], [33, 34]] and reads == 1
    assert log.hyps() == [[11, 12, 13, 14, 15], [22, 23], [31, 32, 33, 34]] and log.most() == 5
    got = log.hyps()
    got[0].append(99)                                                                   # hyps() hands out copies
    assert log.hyps()[0] == [11, 12, 13, 14, 15]
    log.reset()
    assert log.hyps() == [[], [], []] and log.count == [0, 0, 0]
