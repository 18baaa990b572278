"""The host side of a device hypothesis buffer that ACCUMULATES across chunks (greedy.ChunkGreedySearch, decoder.CTCGreedyStream)."""
import torch


class TokenLog:
    """Per stream the count the host knows (exact after every take(): most() + a chunk's most bounds the next chunk) and the tokens it has read."""

    def __init__(self, streams):
        self.count, self.tokens = [0] * streams, [[] for _ in range(streams)]

    def reset(self, streams=None):
        for b in (range(len(self.count)) if streams is None else list(streams)):
            self.count[b], self.tokens[b] = 0, []

    def hyps(self):
        return [list(h) for h in self.tokens]

    def most(self):
        return max(self.count)

    def take(self, hyps, counts):
        """hyps (streams, cap) on the device, counts: the host's list of the counts after a chunk.  Returns the tokens the chunk added per
        stream: one read of the columns [least old count, greatest new count) for all streams, none at all when nothing was emitted."""
        new = [[] for _ in counts]
        if counts != self.count:
            lo, hi = min(self.count), max(counts)
            rows = hyps[:, lo:hi].cpu()
            for b, n in enumerate(counts):
                new[b] = rows[b, self.count[b] - lo:n - lo].tolist()
                self.tokens[b].extend(new[b])
            self.count = list(counts)
        return new


def grow(S, keys, need):
    """need > cap: the (streams, cap) buffers S[k], k in keys, are replaced by zeroed ones of max(2 cap, need) columns that keep the old columns.
    Returns whether it did: whoever holds an old buffer's address (a descriptor, a captured graph) then drops it."""
    cap = S[keys[0]].shape[1]
    for k in (keys if need > cap else ()):
        t = torch.zeros((S[k].shape[0], max(2 * cap, need)), dtype=S[k].dtype, device=S[k].device)
        t[:, :cap] = S[k]
        S[k] = t
    return need > cap
