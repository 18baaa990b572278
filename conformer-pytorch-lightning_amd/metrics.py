"""Error rates on the device -- the counterpart of the reference's `torchmetrics.WordErrorRate` at the end of `validation_step`
(src/module.py:72-79, logged as `valid_wer`) -- over cfm.edit_distance (cfm_edit_distance in csrc/edit_distance.hip; include/cfm.h states the
recurrence and the tie rule that fixes the split into substitutions, deletions and insertions).

    pack(seqs)                        list of token lists -> (int32 [N, Lmax], int32 [N]) on the device: the inverse of what the recognisers return
    unpack(tokens, lens)              back to lists (one host read)
    edit_distance(hyps, refs)         per pair (dist int32 [P], counts int32 [P, 4] = (S, D, I, hits)) on the device; lists or packed pairs
    ErrorRate(device)                 update(hyps, refs) / compute() / counts() / reset(): (S + D + I) / reference tokens over everything seen
    nbest_errors(nbest, refs)         the recognisers' n-best lists against one reference each, one launch: all distances and the oracle entry
    oracle_error_rate(nbest, refs)    the oracle distances' sum over the references' total length
    WordIds                           a growing host dictionary word -> id; encode(strings) splits on whitespace as torchmetrics does

Token level is whatever the caller's ids are: recogniser tokens give a token error rate, WordIds ids give the reference's word error rate.
Costs are 1 for every op: there are no weighted costs and no character-level splitting of tokens.
"""
import torch

import cfm

MAX_LEN = 1024                                                 # cfm_edit_distance's limit on either side


def pack(seqs, device="cuda"):
    """A list of N token lists -> (int32 [N, Lmax] zero-padded, int32 [N]) on `device`, built on the host and sent in one copy each."""
    lens = [len(s) for s in seqs]
    tokens = torch.zeros((len(seqs), max(lens, default=0)), dtype=torch.int32)
    for n, s in enumerate(seqs):
        if lens[n]:
            tokens[n, :lens[n]] = torch.as_tensor(s, dtype=torch.int32)
    return tokens.to(device), torch.tensor(lens, dtype=torch.int32).to(device)


def unpack(tokens, lens):
    """The inverse of pack: a list of token lists (reads both tensors back)."""
    rows, lens = tokens.tolist(), lens.tolist()
    return [row[:n] for row, n in zip(rows, lens)]


def _packed(x, device, who):
    """Lists of token lists, or an already packed (tokens [N, L], lens [N]) pair of tensors (padded labels with their lengths: any integer dtype,
    any device) -> contiguous int32 on `device`."""
    if isinstance(x, (tuple, list)) and len(x) == 2 and isinstance(x[0], torch.Tensor):
        tokens = x[0].to(device=device, dtype=torch.int32).contiguous()
        lens = torch.as_tensor(x[1]).to(device=device, dtype=torch.int32).contiguous()
        if tokens.dim() != 2 or lens.shape != (tokens.shape[0],):
            raise ValueError("%s: a packed operand is (tokens [N, L], lens [N]), got %s and %s" % (who, tuple(tokens.shape), tuple(lens.shape)))
        return tokens, lens
    return pack(x, device)


def edit_distance(hyps, refs, ops=False, device="cuda"):
    """Pair p is hyps[p] against refs[p]; each side a list of token lists or a packed (tokens, lens) pair.  Returns (dist int32 [P],
    counts int32 [P, 4] = (S, D, I, hits)) on the device, with ops=True also (ops uint8 [P, Hmax + Umax], ops_len int32 [P]): 1 hit,
    2 substitution, 3 deletion, 4 insertion in forward order.  No host read."""
    h, hl = _packed(hyps, device, "metrics.edit_distance")
    r, rl = _packed(refs, device, "metrics.edit_distance")
    out = cfm.edit_distance(h, hl, r, rl, counts=True, ops=ops)
    return out if ops else out[:2]


class ErrorRate:
    """(S + D + I) / reference tokens, accumulated on the device: torchmetrics.WordErrorRate's update / compute / reset.

    update(hyps, refs) scores the call's pairs in one launch and adds their (S, D, I, hits, reference tokens) into an int64 [5] device tensor: no
    host read.  compute() is the rate so far (one host read; nan before any reference token), counts() the five sums, reset() clears them."""

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        self.sums = torch.zeros(5, dtype=torch.int64, device=self.device)

    def add_counts(self, counts, ref_lens):
        """counts int32 [P, 4], ref_lens [P] of already scored pairs -> into the sums (update's second half)."""
        self.sums += torch.cat((counts.sum(0, dtype=torch.int64), ref_lens.sum(dtype=torch.int64).reshape(1))).to(self.device)
        return self

    def update(self, hyps, refs):
        h, hl = _packed(hyps, self.device, "ErrorRate.update")
        r, rl = _packed(refs, self.device, "ErrorRate.update")
        _, counts, _, _ = cfm.edit_distance(h, hl, r, rl, counts=True)
        return self.add_counts(counts, rl.clamp(0, r.shape[1]))

    def counts(self):
        S, D, I, hits, n = self.sums.tolist()
        return {"S": S, "D": D, "I": I, "hits": hits, "ref_tokens": n}

    def compute(self):
        S, D, I, _, n = self.sums.tolist()
        return (S + D + I) / n if n else float("nan")

    def reset(self):
        self.sums.zero_()
        return self


def nbest_errors(nbest, refs, device="cuda"):
    """nbest: per utterance a list of (tokens, score), best first, as OfflineRecognizer.recognize(..., beam=k) and the CTC prefix beam search return
    them (lists may differ in length); refs: one reference per utterance, token lists or a packed pair.  One launch over all hypotheses, the
    utterance's reference shared through ref_index, and one host read.  Returns per utterance {"dist": [every entry's distance],
    "oracle": the index of the entry with the lowest distance -- on a tie the lowest index, the best-scored --, "oracle_dist": its distance}."""
    r, rl = _packed(refs, device, "metrics.nbest_errors")
    if len(nbest) != r.shape[0]:
        raise ValueError("metrics.nbest_errors: %d n-best lists for %d references" % (len(nbest), r.shape[0]))
    hyps, index = [], []
    for u, entries in enumerate(nbest):
        if not entries:
            raise ValueError("metrics.nbest_errors: utterance %d has no hypothesis" % u)
        hyps.extend(e[0] for e in entries)
        index.extend([u] * len(entries))                       # in [0, R) by construction
    h, hl = pack(hyps, device)
    dist = cfm.edit_distance(h, hl, r, rl, ref_index=torch.tensor(index, dtype=torch.int32).to(device), counts=False)[0].tolist()
    out, p = [], 0
    for entries in nbest:
        d = dist[p:p + len(entries)]
        p += len(entries)
        best = min(range(len(d)), key=lambda k: (d[k], k))
        out.append({"dist": d, "oracle": best, "oracle_dist": d[best]})
    return out


def oracle_error_rate(nbest, refs, device="cuda", errors=None):
    """Sum of the oracle distances over the references' total length (nan without a reference token); errors: nbest_errors' result when at hand."""
    r, rl = _packed(refs, device, "metrics.oracle_error_rate")
    errors = nbest_errors(nbest, (r, rl), device) if errors is None else errors
    n = int(rl.clamp(0, r.shape[1]).sum())
    return sum(e["oracle_dist"] for e in errors) / n if n else float("nan")


class WordIds:
    """A growing host dictionary word -> int32 id, so that word-level error rates run through the same kernel: the ids mean nothing beyond equality.
    encode(strings) splits every string on whitespace (str.split(), as torchmetrics' WordErrorRate does) and returns pack()-ed ids;
    ErrorRate().update(words.encode(predictions), words.encode(targets)) is the reference's valid_wer."""

    def __init__(self):
        self.ids = {}

    def __len__(self):
        return len(self.ids)

    def ids_of(self, text):
        return [self.ids.setdefault(w, len(self.ids)) for w in text.split()]

    def encode(self, texts, device="cuda"):
        return pack([self.ids_of(t) for t in texts], device)
