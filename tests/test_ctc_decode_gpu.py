"""GPU: CTC decoding on the device (csrc/ctc_decode.hip through cfm.ctc_topk / ctc_greedy / ctc_prefix_beam, decoder.CTCDecoder's greedy_search /
prefix_beam_search, decoder.CTCGreedyStream and the recognisers' ctc= argument) against the float64 restatements of tests/ctc_decode_ref.py.

Every kernel output lies between guard bands (tests/extent.py): extents pre-filled with NaN / -1, so an element the kernel should have left alone
is seen to be untouched and an owned one it missed fails the comparison; the logits' pad columns V..ld are NaN.

Bounds.  top-k: the project's f32 figure 2e-6 max|logit| for lse and logp, classes equal wherever the neighbouring sorted values are further
apart than that.  greedy: integers and bit-equal log-probabilities.  prefix beam: delta = 4 T 2^-23 max(1, max|score|) (ctc_decode_ref.beam_delta);
a case whose every recorded gap exceeds delta must give the restatement's strings in its order, any other its scores as a sorted multiset; which
cases are which is settled on the CPU (test_ctc_decode_cpu.py asserts the share).  End to end the logits themselves carry the fp32 mode's error
5e-5 max|logit| (tests/test_modules_gpu.py), so delta grows by 2 T times that (a log-probability is a logit minus a log-sum-exp of logits)."""
import numpy as np
import pytest
import torch

import ctc_decode_ref as ref
import greedy_ref as R
import synth
from conftest import load_golden
from extent import Guards

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
F32_REL = 2e-6                                               # tests/test_greedy_step_gpu.py
FP32_MODE_REL = 5e-5                                         # tests/test_modules_gpu.py TOL["fp32"]


@pytest.fixture(scope="module")
def cfm():
    import cfm as c
    return c


@pytest.fixture
def precision():
    import cfm
    before = cfm.get_precision()
    yield cfm.set_precision
    cfm.set_precision(before)


# ------------------------------------------------------------------------------------------------------------------------------------- top-k
TOPK_LENS = {(1, 1): [1], (3, 5): [0, 5, 2], (2, 67): [67, 40]}
_topk_refs = {}


def topk_reference(V, B, T):
    if (V, B, T) not in _topk_refs:
        g = torch.Generator().manual_seed(1000 * V + 10 * B + T)
        logits = torch.randn((B, T, V), generator=g) * 3.0
        lp = torch.log_softmax(logits.double(), -1)
        v, i = torch.sort(lp, dim=-1, descending=True, stable=True)
        _topk_refs[(V, B, T)] = (logits, v, i, torch.logsumexp(logits.double(), -1))
    return _topk_refs[(V, B, T)]


def run_topk(cfm, logits, V, lens, k, ld):
    B, T = logits.shape[:2]
    G = Guards()
    lg = G.inp(logits, ld=ld, name="logits")
    ln = G.inp(torch.tensor(lens, dtype=torch.int32), name="lens")
    idx, logp, lse = G.out((B, T, k), torch.int32, name="idx"), G.out((B, T, k), name="logp"), G.out((B, T), name="lse")
    cfm.ctc_topk(lg, V, ln, k, out=(idx, logp, lse))
    torch.cuda.synchronize()
    G.check()
    return idx.cpu(), logp.cpu(), lse.cpu()


@pytest.mark.parametrize("B,T", sorted(TOPK_LENS))
@pytest.mark.parametrize("V", [3, 17, 73, 5002])
def test_topk(cfm, V, B, T):
    logits, v64, i64, lse64 = topk_reference(V, B, T)
    lens = TOPK_LENS[(B, T)]
    Vp = (V + 3) // 4 * 4
    tol = F32_REL * float(logits.abs().max())
    valid = torch.arange(T)[None, :] < torch.tensor(lens)[:, None]
    for ld in (Vp, Vp + 8):
        for k in (1, 4, 10, 16):
            if k > V:
                with pytest.raises(RuntimeError, match="exceeds the %d classes" % V):
                    run_topk(cfm, logits, V, lens, k, ld)
                continue
            idx, logp, lse = run_topk(cfm, logits, V, lens, k, ld)
            what = (V, B, T, ld, k)
            assert float((lse[valid].double() - lse64[valid]).abs().max()) <= tol, what
            assert float((logp[valid].double() - v64[valid][:, :k]).abs().max()) <= tol, what
            # a class must be the reference's wherever its value is further than tol from both sorted neighbours (the k-th one's next included)
            vv = v64[valid]
            pad = torch.full((vv.shape[0], 1), float("inf"), dtype=torch.float64)
            gap_up = torch.cat([pad, vv[:, :-1] - vv[:, 1:]], 1)[:, :k]
            gap_dn = torch.cat([vv[:, :-1] - vv[:, 1:], pad], 1)[:, :k]
            sure = (gap_up > tol) & (gap_dn > tol)
            assert float(sure.double().mean()) > 0.9, what
            assert torch.equal(idx[valid].long()[sure], i64[valid][:, :k][sure]), what
            for b in range(B):                                                           # descending, classes distinct and in range
                for t in range(lens[b]):
                    row = idx[b, t].tolist()
                    assert len(set(row)) == k and min(row) >= 0 and max(row) < V, what
                    assert all(logp[b, t, j] >= logp[b, t, j + 1] for j in range(k - 1)), what
            # rows at or beyond lens are left untouched: the extent's fill
            assert bool((idx[~valid] == -1).all()) and bool(torch.isnan(logp[~valid]).all()) and bool(torch.isnan(lse[~valid]).all()), what


def test_topk_exact_ties_follow_the_stable_sort(cfm):
    """Equal values within a lane's four classes, across lanes, across the wavefront's 256-class round, with blank and class V - 1 among them."""
    V, k = 301, 16
    logits = (-0.125 * torch.arange(V, dtype=torch.float32)).repeat(2, 3, 1).contiguous()          # distinct, exactly representable
    logits[..., [0, 1, 2, 7, 255, 256, 260, V - 1]] = 5.0
    logits[..., [3, 64, 257]] = 4.0
    logits[1, :, [9, 10, 299, 298]] = 6.0
    i64, _, _ = ref.topk64(logits, k)
    assert i64[0, 0].tolist()[:11] == [0, 1, 2, 7, 255, 256, 260, V - 1, 3, 64, 257] and i64[1, 0].tolist()[:4] == [9, 10, 298, 299]
    for kk in (1, 4, 10, 16):
        idx, logp, _ = run_topk(cfm, logits, V, [3, 3], kk, 304 + 8)
        assert torch.equal(idx.long(), i64[..., :kk]), kk
        assert torch.equal(logp[..., 0], logp[..., min(1, kk - 1)])


# ------------------------------------------------------------------------------------------------------------------------------------ greedy
def run_greedy(cfm, seqs, T, blank, V=6, cap=None, state=None, seed=0):
    """seqs: per stream a list of classes (its length is lens[b]).  Returns (the placed state, logp, Guards)."""
    B = len(seqs)
    G = Guards()
    idx = torch.full((B, T, 1), 1, dtype=torch.int32)
    for b, s in enumerate(seqs):
        idx[b, :len(s), 0] = torch.tensor(s, dtype=torch.int32) if s else idx[b, :0, 0]
    logp = -torch.rand((B, T, 1), generator=torch.Generator().manual_seed(seed)) - 0.01
    iv, lv = G.inp(idx, name="idx"), G.inp(logp, name="logp")
    ln = G.inp(torch.tensor([len(s) for s in seqs], dtype=torch.int32), name="lens")
    cap = T if cap is None else cap
    if state is None:
        state = dict(prev=torch.full((B,), -1, dtype=torch.int32), frame_base=torch.zeros((B,), dtype=torch.int32), count=torch.zeros((B,), dtype=torch.int64),
                     overflow=torch.zeros((1,), dtype=torch.int32))
    S = {k: G.io(v, name=k) for k, v in state.items()}
    S.update(hyps=G.out((B, cap), torch.int64, name="hyps"), frames=G.out((B, cap), torch.int32, name="frames"), token_logp=G.out((B, cap), name="token_logp"))
    cfm.ctc_greedy(iv, lv, ln, V, blank=blank, state=S)
    torch.cuda.synchronize()
    G.check()
    return {k: v.cpu() for k, v in S.items()}, logp


def check_greedy(S, logp, seqs, blank, prevs=None, bases=None, cap=None):
    for b, s in enumerate(seqs):
        p0, f0 = (-1 if prevs is None else prevs[b]), (0 if bases is None else bases[b])
        toks, frames, lps, last = ref.best_path(s, logp[b, :, 0], len(s), blank, prev=p0, frame_base=f0)
        n = len(toks) if cap is None else min(len(toks), cap)
        assert int(S["count"][b]) == len(toks), b
        assert S["hyps"][b, :n].tolist() == toks[:n] and S["frames"][b, :n].tolist() == frames[:n], b
        assert S["token_logp"][b, :n].tolist() == [float(np.float32(x)) for x in lps[:n]], b          # bit for bit: the top-k's value
        assert bool((S["hyps"][b, n:] == -1).all()) and bool(torch.isnan(S["token_logp"][b, n:]).all()), b
        assert int(S["prev"][b]) == (last if s else p0) and int(S["frame_base"][b]) == f0 + len(s), b


@pytest.mark.parametrize("blank", [0, 2])
def test_greedy(cfm, blank):
    a = 3
    g = torch.Generator().manual_seed(7)
    long_seq = torch.randint(0, 4, (130,), generator=g).tolist()                         # more than one round of 64 frames
    runs = torch.randint(0, 4, (33,), generator=g).repeat_interleave(4)[:129].tolist()   # runs that straddle the rounds
    seqs = [[blank] * 10, [a] * 10, [a, a, blank, a], [], long_seq, runs, [a] * 64 + [a, 1], [1] * 65]
    S, logp = run_greedy(cfm, seqs, 130, blank)
    check_greedy(S, logp, seqs, blank)
    assert S["hyps"][2, :2].tolist() == [a, a] and int(S["count"][0]) == 0 and int(S["count"][1]) == 1 and int(S["overflow"][0]) == 0
    assert int(S["prev"][3]) == -1                                                        # lens 0: nothing changed
    # second call on the same state: a repeat across the two calls collapses, a blank between them does not
    state = {k: S[k] for k in ("prev", "frame_base", "count", "overflow")}
    nxt = [[a, 1], [a, a], [blank, a], [a], [long_seq[-1], 1], [], [1, 1], [blank, 1]]
    S2, logp2 = run_greedy(cfm, nxt, 4, blank, cap=200, state=state, seed=1)
    for b, s in enumerate(nxt):
        toks, frames, _, last = ref.best_path(s, logp2[b, :, 0], len(s), blank, prev=int(S["prev"][b]), frame_base=int(S["frame_base"][b]))
        n0 = int(S["count"][b])
        assert int(S2["count"][b]) == n0 + len(toks), b
        assert S2["hyps"][b, n0:n0 + len(toks)].tolist() == toks and S2["frames"][b, n0:n0 + len(toks)].tolist() == frames, b      # appended at count
        assert int(S2["prev"][b]) == (last if s else int(S["prev"][b])), b
    assert int(S2["overflow"][0]) == 0 and int(S2["count"][1]) == 1 and int(S2["count"][2]) == 3 and int(S2["count"][0]) == 2 and int(S2["count"][3]) == 1


def test_greedy_overflow_counts_but_does_not_store(cfm):
    seqs = [[1, 2, 3, 4, 5], [1, 1, 1]]
    S, logp = run_greedy(cfm, seqs, 5, 0, cap=2)
    assert int(S["overflow"][0]) == 1 and S["count"].tolist() == [5, 1]
    check_greedy(S, logp, seqs, 0, cap=2)


def onehot_head(V=6, D=16):
    """A CTC head whose argmax is the class its input row names: weight 10 * identity, zero bias (exact in every precision mode)."""
    import decoder
    head = decoder.CTCDecoder(V, D, 0.0).eval()
    with torch.no_grad():
        head.ctc_lo.weight.copy_(10.0 * torch.eye(V, D))
        head.ctc_lo.bias.zero_()
    return head.to(DEV)


def test_greedy_stream_chunks_reset_and_growth(cfm, precision):
    import decoder
    precision("fp32")
    head = onehot_head()
    g = torch.Generator().manual_seed(3)
    B, T = 3, 37
    seq = torch.randint(0, 4, (B, 12), generator=g).repeat_interleave(4, dim=1)[:, :T]     # runs of four: repeats straddle every chunk size
    seq[2] = torch.randint(0, 6, (T,), generator=g)
    total = [37, 22, 30]
    enc = torch.nn.functional.one_hot(seq, 16).float().to(DEV)
    lens = torch.tensor(total, dtype=torch.int32, device=DEV)
    want, det = head.greedy_search(enc, lens, return_details=True)
    for b in range(B):
        toks, frames, _, _ = ref.best_path(seq[b].tolist(), [0.0] * T, total[b], 0)
        assert want[b] == toks and det["frames"][b, :len(toks)].tolist() == frames and int(det["count"][b]) == len(toks)
    assert sum(len(w) for w in want) > 20
    for C in (1, 4, 16):
        st = decoder.CTCGreedyStream(head, B, max_tokens=2)                                # far too small: the buffer grows
        got = [[] for _ in range(B)]
        for s in range(0, T, C):
            n = [min(max(total[b] - s, 0), C) for b in range(B)]
            chunk = torch.zeros((B, C, 16), device=DEV)
            chunk[:, :min(C, T - s)] = enc[:, s:s + C]
            new = st.decode(chunk, n if s % 2 else torch.tensor(n, dtype=torch.int32, device=DEV))
            for b in range(B):
                got[b] += new[b]
        assert got == want and st.hyps() == want, C
        for b in range(B):
            assert st.S["frames"][b, :len(want[b])].tolist() == det["frames"][b, :len(want[b])].tolist(), (C, b)      # absolute frames across chunks
        assert st.S["prev"].tolist() == [int(seq[b, total[b] - 1]) for b in range(B)]
    st.reset([1])
    assert st.hyps() == [want[0], [], want[2]] and st.S["prev"].tolist()[1] == -1 and st.S["count"].tolist() == [len(want[0]), 0, len(want[2])]
    last = [int(seq[b, total[b] - 1]) for b in range(B)]
    chunk = torch.nn.functional.one_hot(torch.tensor([[last[0]], [last[1]], [last[2]]]), 16).float().to(DEV)
    new = st.decode(chunk)
    assert new[0] == [] and new[2] == [] and new[1] == ([last[1]] if last[1] != 0 else [])  # stream 1 starts afresh, the others collapse the repeat


# ------------------------------------------------------------------------------------------------------------------------------- prefix beam
def run_beam(cfm, idx, logp, lens, V, beam, blank=0):
    B, T, k = idx.shape
    G = Guards()
    iv, lv, ln = G.inp(idx, name="idx"), G.inp(logp, name="logp"), G.inp(lens, name="lens")
    tokens, nlen, score = G.out((B, beam, T), torch.int64, name="nbest_tokens"), G.out((B, beam), torch.int32, name="nbest_len"), G.out((B, beam), name="nbest_score")
    nodes = G.ws(2 * B * beam * (T + 1), torch.int32, name="nodes")
    cfm.ctc_prefix_beam(iv, lv, ln, V, beam=beam, blank=blank, out=(tokens, nlen, score), nodes=nodes)
    torch.cuda.synchronize()
    G.check()
    tokens, nlen, score = tokens.cpu(), nlen.cpu(), score.cpu()
    out = []
    for b in range(B):
        live = [n for n in range(beam) if float(score[b, n]) > float("-inf")]
        assert live == list(range(len(live))) and all(int(nlen[b, n]) == 0 for n in range(len(live), beam)), b
        out.append([(tuple(tokens[b, n, :int(nlen[b, n])].tolist()), float(score[b, n])) for n in live])
        for n in live:                                                                   # beyond a hypothesis' length: untouched
            assert bool((tokens[b, n, int(nlen[b, n]):] == -1).all()), (b, n)
    return out


def compare_beam(got, want, T, extra=0.0, what=None):
    """got: the kernel's [(tokens, score)] of one utterance; want: prefix_beam_search64's result dict.  Returns whether the case was clear."""
    delta = ref.beam_delta(T, want["max_abs"]) + extra
    clear = all(gap > delta for gap in want["frame_gaps"] + want["nbest_gaps"])
    print("beam case", what, "clear" if clear else "unclear", "delta %.3g" % delta, "score error %.3g" %
          max([abs(a[1] - b[1]) for a, b in zip(got, want["nbest"])] or [0.0]))
    assert len(got) == len(want["nbest"]), what
    if clear:
        assert [l for l, _ in got] == [l for l, _ in want["nbest"]], what
        assert all(abs(a[1] - b[1]) <= delta for a, b in zip(got, want["nbest"])), what
    else:
        assert all(abs(a - b) <= delta for a, b in zip(sorted(s for _, s in got), sorted(s for _, s in want["nbest"]))), what
    return clear


@pytest.mark.parametrize("case", ref.beam_cases_64(), ids=lambda c: "s%d-V%d-T%d-beam%d" % c)
def test_prefix_beam(cfm, case):
    seed, V, T, beam = case
    idx, logp, lens = ref.beam_case(seed, V, T, beam)
    got = run_beam(cfm, idx, logp, lens, V, beam)
    for b in range(idx.shape[0]):
        want = ref.prefix_beam_search64(idx[b], logp[b], int(lens[b]), beam, 0)
        compare_beam(got[b], want, T, what=(case, b))
    assert got[-1] == [((), 0.0)]                                                        # lens 0: the empty hypothesis, score 0


def test_prefix_beam_reentry_merges(cfm):
    """A prefix leaves the beam and comes back under a new trie node while its extension stays: the two meet again and must merge."""
    seed, V, T, beam = ref.REENTRY_CASE
    idx, logp, lens = ref.beam_case(seed, V, T, beam)
    got = run_beam(cfm, idx, logp, lens, V, beam)
    events = 0
    for b in range(idx.shape[0]):
        want = ref.prefix_beam_search64(idx[b], logp[b], int(lens[b]), beam, 0)
        events += want["reentry"]
        assert compare_beam(got[b], want, T, what=("reentry", b))                          # clear: strings, order and (merged) scores
        assert len({l for l, _ in got[b]}) == len(got[b])                                  # no string twice in the n-best
    assert events > 0


def test_prefix_beam_blank_not_zero_and_full_beam(cfm):
    idx, logp, lens = ref.beam_case(77, 6, 12, 16, blank=4, B=3)
    got = run_beam(cfm, idx, logp, lens, 6, 16, blank=4)
    for b in range(3):
        compare_beam(got[b], ref.prefix_beam_search64(idx[b], logp[b], int(lens[b]), 16, 4), 12, what=("blank4", b))


# -------------------------------------------------------------------------------------------------------------------------------- end to end
_e2e = {}


def e2e_head():
    """The offline fixture's encoder outputs (T' = 49, 40, 11, 1; D = 144), a CTCDecoder(V = 73) with synthetic weights whose seed is the first one
    that leaves every best-path decision a top-2 gap >= 1e-3 max|logit| (the fixture's own convention), the float64 logits and their results."""
    if not _e2e:
        import decoder
        g, meta = load_golden("offline_asr")
        encs = [torch.from_numpy(g["enc_%d" % b]) for b in range(4)]
        for seed in range(700, 800):
            head = synth.load_synth_(decoder.CTCDecoder(73, 144, 0.0).eval(), seed)
            W, bias = head.ctc_lo.weight.detach().double(), head.ctc_lo.bias.detach().double()
            logits = [e.double() @ W.t() + bias for e in encs]
            top2 = [torch.sort(z, dim=-1, descending=True)[0][:, :2] for z in logits]
            if min(float(((t[:, 0] - t[:, 1]) / z.abs().max()).min()) for t, z in zip(top2, logits)) >= 1e-3:
                break
        else:
            raise AssertionError("no weight seed with clear best-path decisions")
        _e2e.update(head=head, encs=encs, logits=logits, seed=seed, lmax=max(float(z.abs().max()) for z in logits))
    return _e2e


def padded(encs, fill_seed=9):
    """The utterances as one padded batch; the frames behind each length hold noise, not zeros."""
    T = max(e.shape[0] for e in encs)
    x = torch.from_numpy(synth.normal(fill_seed, (len(encs), T, encs[0].shape[1]), 3.0))
    for b, e in enumerate(encs):
        x[b, :e.shape[0]] = e
    return x, torch.tensor([e.shape[0] for e in encs], dtype=torch.int32)


def test_end_to_end_greedy_and_beam(cfm, precision):
    precision("fp32")
    E = e2e_head()
    head = E["head"].to(DEV)
    x, lens = padded(E["encs"])
    hyps, det = head.greedy_search(x.to(DEV), lens.to(DEV), return_details=True)
    nbest = head.prefix_beam_search(x.to(DEV), lens.to(DEV), beam=4)
    n_clear = 0
    for b, z in enumerate(E["logits"]):
        T = z.shape[0]
        i64, v64, _ = ref.topk64(z, 4)
        toks, frames, lps, _ = ref.best_path(i64[:, 0], v64[:, 0], T, 0)
        assert hyps[b] == toks and det["frames"][b, :len(toks)].tolist() == frames, b
        err = float((det["logp"][b, :len(toks)].double().cpu() - torch.tensor(lps, dtype=torch.float64)).abs().max()) if toks else 0.0
        assert err <= 2 * FP32_MODE_REL * E["lmax"], (b, err)
        want = ref.prefix_beam_search64(i64, v64, T, 4, 0)
        got = [(tuple(l), s) for l, s in nbest[b]]
        n_clear += compare_beam(got, want, T, extra=2 * T * FP32_MODE_REL * E["lmax"], what=("e2e", b))
    assert n_clear >= 1 and sum(len(h) for h in hyps) > 10
    # one utterance at a time gives the same: nothing behind a length is read
    for b, e in enumerate(E["encs"]):
        n = torch.tensor([e.shape[0]], dtype=torch.int32, device=DEV)
        assert head.greedy_search(e[None].to(DEV), n) == [hyps[b]]
        assert [l for l, _ in head.prefix_beam_search(e[None].to(DEV), n, beam=4)[0]] == [l for l, _ in nbest[b]]


def offline_modules(meta):
    import encoder
    enc = synth.load_synth_(encoder.ConformerEncoder(cmvn=None, **meta["cfg"]).eval(), meta["wseed"]).to(DEV)
    h = meta["head"]
    pr, jn = R.modules(h["V"], h["embed"], h["hidden"], h["P"], h["J"], h["layers"], meta["hseed"], enc_dim=meta["cfg"]["encoder_dim"], shaped=True)
    with torch.no_grad():
        jn.ffn_out.bias[meta["blank"]] += meta["blank_bias"]
    return enc, pr.to(DEV), jn.to(DEV)


def test_offline_recognizer_ctc(cfm, precision):
    import transducer
    precision("fp32")
    _, meta = load_golden("offline_asr")
    head = e2e_head()["head"].to(DEV)
    enc, pr, jn = offline_modules(meta)
    lens = meta["lens"] + [5]                                                            # 5 feature frames: no encoder frame
    x = torch.from_numpy(synth.fbank(meta["xseed"], len(meta["lens"]), max(meta["lens"])))
    x = torch.cat([x, x[:1]], 0).to(DEV)
    rec = transducer.OfflineRecognizer(enc, pr, jn, blank=meta["blank"], n_steps=meta["n_steps"], ctc=head)
    hyps = rec.recognize_ctc(x, torch.tensor(lens, dtype=torch.int32, device=DEV))
    nbest = rec.recognize_ctc(x, torch.tensor(lens, dtype=torch.int32, device=DEV), beam=4)
    out_lens = rec.encoder_out_lens.tolist()
    assert out_lens == [49, 40, 11, 1, 0] and hyps[-1] == [] and nbest[-1] == [([], 0.0)]
    for b in range(4):                                                                   # per utterance, alone: the padded batch reads nothing behind a length
        xb = x[b:b + 1, :lens[b]].contiguous()
        assert rec.recognize_ctc(xb, torch.tensor(lens[b:b + 1], dtype=torch.int32, device=DEV)) == [hyps[b]], b
        one = rec.recognize_ctc(xb, torch.tensor(lens[b:b + 1], dtype=torch.int32, device=DEV), beam=4)[0]
        assert [l for l, _ in one] == [l for l, _ in nbest[b]], b
        assert hyps[b] == head.greedy_search(rec.encoder_out, rec.encoder_out_lens)[0]
    assert sum(len(h) for h in hyps) > 10
    assert rec.recognize(x, torch.tensor(lens, dtype=torch.int32, device=DEV))[-1] == []  # the RNN-T path is still there


def test_streaming_recognizer_ctc(cfm, precision):
    import decoder
    import transducer
    precision("fp32")
    _, meta = load_golden("stream_asr")
    head = e2e_head()["head"].to(DEV)
    enc, pr, jn = offline_modules(meta)
    B, chunk = meta["streams"], meta["chunk"]
    hop, window = 4 * chunk, (chunk - 1) * 4 + 7
    feats = torch.from_numpy(synth.fbank(meta["xseed"], B, window + hop * (meta["chunks"] - 1))).to(DEV)
    kw = dict(blank=meta["blank"], n_steps=meta["n_steps"], carry=True)
    rec = transducer.StreamingRecognizer(enc, pr, jn, B, chunk, meta["left"], ctc=head, **kw)
    plain = transducer.StreamingRecognizer(enc, pr, jn, B, chunk, meta["left"], **kw)
    none = transducer.StreamingRecognizer(enc, pr, jn, B, chunk, meta["left"], ctc=None, **kw)
    assert plain.ctc_decoder is None and none.ctc_decoder is None
    alone = decoder.CTCGreedyStream(head, B, blank=meta["blank"])
    for s in range(meta["chunks"]):
        w = feats[:, s * hop: s * hop + window].contiguous()
        fl = [window, window, 0] if s == 2 else None                                     # one step with an idle stream: the lengths reach both decoders
        new = rec.step(w, frame_lens=fl)
        alone.decode(rec.encoder_out.clone(), rec.encoder_stream.out_lens if fl is not None else None)
        assert new == plain.step(w, frame_lens=fl) == none.step(w, frame_lens=fl), s
    assert rec.ctc_hyps() == alone.hyps() and sum(len(h) for h in rec.ctc_hyps()) > 10
    assert rec.hyps() == plain.hyps() == none.hyps()
    with pytest.raises(RuntimeError, match="without a CTC head"):
        plain.ctc_hyps()
    rec.reset([0])
    assert rec.ctc_hyps()[0] == [] and rec.hyps()[0] == [] and rec.ctc_hyps()[1:] == alone.hyps()[1:]
