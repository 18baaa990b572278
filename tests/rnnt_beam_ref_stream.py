"""Float64 STREAMING RNN-T beam search on the CPU -- the specification of greedy.StreamingBeamSearch / csrc/greedy.hip's
cfm_rnnt_beam_stream_*.  It is rnnt_beam_ref.search64, unchanged in every decision, run on frames that arrive in pieces: the step below
is search64's loop body on a state that outlives the call (its pieces -- greedy_ref.step64, lae, the candidate order -- are imported, the
body is restated because search64 is one loop; test_rnnt_beam_stream_cpu.py holds the two to the same floats).

Per stream: `avail`, the encoder frames fed so far, and `final`, whether the utterance has ended (n = avail is then known).  Before each
step:
  final set       step exactly as search64 does with n = avail: kept candidates with t == n finish into F, F-full pruning applies, the stream
                  is done when the live set empties
  final not set   the stream steps only if every live hypothesis has t <= avail - 2; otherwise it is PAUSED and a step changes nothing

Holding back one frame: after a permitted step every candidate has t <= avail - 1 < n for any n the utterance can still turn out to have
(n == avail included: a `final` that arrives with no new frame).  So no candidate that should have finished is missed, and no live
hypothesis sits at t == n needing a finishing pass on resume.  Hence, for every split of an utterance's frames into feeds, the steps
taken, the live sets after them and the final n-best list are search64's on the whole utterance, to the last bit of the float64 scores.

max_len is explicit: n is unknown while the search runs, so search64's default (the frames) cannot apply.

Between feeds a stream reports
  best     the top-ranked live hypothesis (tokens, score); once done, the first entry of the n-best list
  stable   the longest common prefix, BY TOKENS, of the strings of all live hypotheses.  Every later live set and every finished hypothesis
           descends from the current live set, so it only grows and is a prefix of every entry of the final n-best list; once the stream is
           done it stays what it last was
"""
import torch

import greedy_ref as R
import rnnt_beam_ref as BR
from rnnt_beam_ref import NEG, lae


def common_prefix(strings):
    strings = list(strings)
    out = strings[0]
    for s in strings[1:]:
        k = 0
        while k < min(len(out), len(s)) and out[k] == s[k]:
            k += 1
        out = out[:k]
    return tuple(out)


class Stream64:
    """One utterance.  feed(frames, final) appends projected frames ((k, J), enc_ffn already applied; k may be 0), latches final, steps until
    the stream is paused or done and returns the report dict(stable, best=(tokens, score), nbest=None or [(tokens, score)] best first)."""

    def __init__(self, P, beam, max_len, blank=0, max_symbols=64):
        assert 1 <= beam <= 15 and max_symbols >= 1 and max_len >= 0
        self.P, self.beam, self.blank, self.max_symbols, self.max_len = P, int(beam), int(blank), int(max_symbols), int(max_len)
        L, H = R.num_layers(P), P["p.rnn.weight_hh_l0"].shape[1]
        z = torch.zeros((L, H), dtype=torch.float64)
        self.A = [dict(tokens=(), t=0, fc=0, score=0.0, token=self.blank, h=z, c=z)]
        self.F, self.frames, self.final, self.done = [], [], False, False
        self.steps, self.merges, self.trace, self.nbest, self.stable = 0, 0, [], None, ()

    @property
    def avail(self):
        return len(self.frames)

    def paused(self):
        return not self.done and not self.final and any(a["t"] > self.avail - 2 for a in self.A)

    def live(self):
        """The live set as search64's trace records it."""
        return [(x["tokens"], x["t"], x["fc"], x["score"]) for x in self.A]

    def step(self):
        """One step if the rule permits it (True), else nothing changes (False)."""
        if self.done or self.paused():
            return False
        if self.final and self.avail == 0:                   # search64's n == 0
            self.nbest, self.done, self.A = [((), 0.0)], True, []
            return False
        P, A, F, beam, blank = self.P, self.A, self.F, self.beam, self.blank
        n = self.avail if self.final else None               # None: no candidate can finish (every t < avail <= n)
        assert self.steps <= self.avail + self.max_len, "more steps than alignments are long"
        self.steps += 1
        st = R.step64(P, [a["token"] for a in A], torch.stack([a["h"] for a in A], 1), torch.stack([a["c"] for a in A], 1),
                      torch.stack([self.frames[a["t"]] for a in A]))
        logp = torch.log_softmax(st["logits"], -1)
        cand = {}
        for r, a in enumerate(A):
            cand[a["tokens"]] = dict(a, t=a["t"] + 1, fc=0, score=a["score"] + float(logp[r, blank]), key=(r, 0, 0))
        for r, a in enumerate(A):
            if a["fc"] == self.max_symbols or len(a["tokens"]) == self.max_len:
                continue
            lp = logp[r].clone()
            lp[blank] = NEG
            v, i = torch.sort(lp, descending=True, stable=True)
            for j in range(min(beam, lp.numel() - 1)):
                k, s = int(i[j]), a["score"] + float(v[j])
                new = dict(tokens=a["tokens"] + (k,), t=a["t"], fc=a["fc"] + 1, score=s, token=k, h=st["h_new"][:, r], c=st["c_new"][:, r], key=(r, 1, k))
                old = cand.get(new["tokens"])
                if old is None:
                    cand[new["tokens"]] = new
                else:
                    assert old["key"][1] == 0 and old["t"] == new["t"]
                    old["score"], old["key"] = lae(old["score"], s), min(old["key"], new["key"])
                    self.merges += 1
        order = sorted(cand.values(), key=lambda x: (-x["score"], x["key"]))
        A = []
        for x in order[:beam]:
            if n is None or x["t"] < n:
                assert x["t"] < self.avail
                A.append(x)
                continue
            pos = len(F)
            while pos > 0 and F[pos - 1][1] < x["score"]:
                pos -= 1
            F.insert(pos, (x["tokens"], x["score"]))
            if len(F) > beam:
                F.pop()
        if len(F) == beam:
            worst = F[-1][1]
            A = [x for x in A if not x["score"] < worst]
        self.A = A
        self.trace.append(self.live())
        if not A:
            assert len({f[0] for f in F}) == len(F)
            self.nbest, self.done = list(F), True
        return True

    def report(self):
        if self.done:
            return dict(stable=self.stable, best=self.nbest[0], nbest=list(self.nbest))
        self.stable = common_prefix(a["tokens"] for a in self.A)
        return dict(stable=self.stable, best=(self.A[0]["tokens"], self.A[0]["score"]), nbest=None)

    def feed(self, frames, final=False):
        assert not self.done or len(frames) == 0, "a done stream takes no frames"
        if not self.done:
            if len(frames):
                self.frames.extend(torch.as_tensor(frames).double().cpu().reshape(len(frames), -1))
            self.final = self.final or bool(final)
        self.step()                                          # the n == 0 result, when that is what final says
        while self.step():
            pass
        return self.report()


def splits(n):
    """name -> list of (frames in the feed, final): the ways the tests cut n frames."""
    def by(k):
        cuts = [(min(k, n - i), False) for i in range(0, n, k)] or [(0, False)]
        cuts[-1] = (cuts[-1][0], True)
        return cuts
    idle = [(min(2, n), False), (0, False), (0, False)] + [(min(3, n - i), False) for i in range(min(2, n), n, 3)]
    idle[-1] = (idle[-1][0], True)
    return {"by1": by(1), "by3": by(3), "by5": by(5), "all": [(n, True)], "idle": idle, "final_alone": by(4)[:-1] + [(by(4)[-1][0], False), (0, True)]}


def run(P, enc_proj, n, beam, max_len, cuts, blank=0, max_symbols=64):
    """The utterance's first n frames fed by `cuts`; returns (Stream64, the report after every feed)."""
    s = Stream64(P, beam, max_len, blank, max_symbols)
    reports, i = [], 0
    for k, final in cuts:
        reports.append(s.feed(enc_proj[i:i + k], final))
        i += k
    assert i == n
    return s, reports


def explicit_max_len(case):
    """A case's max_len, T' where the case leaves it to the frames: streaming has to name it, and so do the comparisons with it."""
    return case[7] if case[6] is None else case[6]


_cache = {}


def reference(case):
    """rnnt_beam_ref.reference with the explicit max_len: (P, enc_proj (B, T', J) float64, lens, search64 per utterance, their deltas), once."""
    if case[0] not in _cache:
        name, hd, B, beam, max_symbols, blank, max_len, T, seed, sharpen = case
        pr, jn, h = BR.head(hd, blank, sharpen)
        P = R.params64(pr, jn)
        enc, lens = BR.inputs(case)
        enc_proj = enc.double() @ P["j.enc_ffn.weight"].t() + P["j.enc_ffn.bias"]
        res = [BR.search64(P, enc_proj[b], int(lens[b]), beam, blank, max_symbols, explicit_max_len(case)) for b in range(B)]
        deltas = [BR.beam_delta(max(r["steps"], 1), r["max_abs"], BR.GATE_STEP * max(r["logit_max"], 1.0)) for r in res]
        _cache[case[0]] = (P, enc_proj, lens, res, deltas)
    return _cache[case[0]]


def chunk_cuts(n, per):
    """n frames fed `per` at a time, final with the last of them."""
    cuts = [(min(per, n - i), False) for i in range(0, n, per)] or [(0, False)]
    cuts[-1] = (cuts[-1][0], True)
    return cuts
