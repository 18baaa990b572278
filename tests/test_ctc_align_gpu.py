"""GPU: CTC forced alignment on the device (cfm_ctc_align in csrc/ctc.hip through cfm.ctc_align, decoder.CTCDecoder.forced_align and
transducer.OfflineRecognizer.align / align_audio) against the float64 statement of tests/ctc_align_ref.py.

Every operand lies between guard bands (tests/extent.py): the logits' pad columns V..ld are NaN, every output is pre-filled with NaN / -1 inside and
0xA5 around, so an owned element the kernel missed fails the comparison and a stray write fails G.check().

Bounds.  score: delta = 4 T 2^-23 max(1, |score|) (ctc_decode_ref.beam_delta's formula, T the utterance's frames).  The device path must be a valid
alignment whose own float64 score is within delta of the optimum; start / end / token_logp must be consistent with the device path, token_logp within
2e-6 max|logit| x run length of its float64 value (the project's f32 figure, tests/test_greedy_step_gpu.py).  Where every decision along the float64
optimal path is further than delta from flipping (`exact`, settled on the CPU in test_ctc_align_cpu.py), and in the constant-logit tie cases, path,
start and end are the definition's.  End to end the logits carry the fp32 mode's error 5e-5 max|logit| (tests/test_modules_gpu.py), so delta grows by
2 T times that, as in test_ctc_decode_gpu.py."""
import numpy as np
import pytest
import torch

import ctc_align_ref as ref
import greedy_ref as R
import synth
from conftest import load_golden
from extent import Guards

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
F32_REL = 2e-6                                               # tests/test_greedy_step_gpu.py
FP32_MODE_REL = 5e-5                                         # tests/test_modules_gpu.py TOL["fp32"]
NEG = float("-inf")


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


def run_align(cfm, logits, V, lens, labels, llens, ld=None):
    """cfm.ctc_align between guard bands.  logits f32 [B,T,V] (CPU), lens / llens lists, labels int32 [B,Umax] (CPU).  Returns the five outputs on the CPU."""
    B, T = logits.shape[:2]
    Umax = labels.shape[1]
    G = Guards()
    lg = G.inp(logits, ld=(V + 3) // 4 * 4 if ld is None else ld, name="logits")
    ln, lab, ll = G.inp(torch.tensor(lens, dtype=torch.int32), name="enc_lens"), G.inp(labels, name="labels"), G.inp(torch.tensor(llens, dtype=torch.int32), name="label_lens")
    out = (G.out((B, T), torch.int32, name="path"), G.out((B,), name="score"), G.out((B, Umax), torch.int32, name="start"),
           G.out((B, Umax), torch.int32, name="end"), G.out((B, Umax), name="token_logp"))
    got = cfm.ctc_align(lg, V, ln, lab, ll, out=out)
    torch.cuda.synchronize()
    G.check()
    assert all(a is b for a, b in zip(got, out))
    return [t.cpu() for t in out]


def padded_cols(logits, V):
    """The logits on the device with the row stride the kernels want: a multiple of 4 columns, the pad columns zero."""
    out = torch.zeros(tuple(logits.shape[:2]) + ((V + 3) // 4 * 4,), device=DEV)
    out[..., :V] = logits.to(DEV)
    return out


def check_utterance(got, b, res, lp, labels, n, V, lmax, identical, extra=0.0, what=None):
    """One utterance of a run against its align64 result `res` (lp: its float64 log-probabilities [n, V])."""
    path, score, start, end, tl = (t[b] for t in got)
    U, z = len(labels), ref.extended(labels, V)
    path, sc = path.tolist(), float(score)
    assert path[n:] == [-1] * (len(path) - n), what                                      # beyond the utterance
    assert start[U:].tolist() == [-1] * (len(start) - U) and end[U:].tolist() == [-1] * (len(end) - U) and bool((tl[U:] == NEG).all()), what
    if not res["feasible"]:
        assert sc == NEG and path[:n] == [-1] * n and start[:U].tolist() == [-1] * U and end[:U].tolist() == [-1] * U and bool((tl[:U] == NEG).all()), what
        return
    delta = ref.delta(max(n, 1), res["score"]) + extra
    own = ref.path_score(path[:n], lp, z) if n else 0.0
    print("align", what, "score error %.3g own-path deficit %.3g delta %.3g" % (abs(sc - res["score"]), res["score"] - own, delta))
    assert abs(sc - res["score"]) <= delta, what
    assert own > NEG, what                                                               # a valid alignment: it collapses to the labels
    assert abs(own - res["score"]) <= delta, what
    sp = ref.spans(path[:n], lp, z)
    assert start[:U].tolist() == sp["start"].tolist() and end[:U].tolist() == sp["end"].tolist(), what
    for u in range(U):
        run = int(sp["end"][u] - sp["start"][u] + 1)
        err = abs(float(tl[u]) - sp["token_logp"][u])
        assert err <= F32_REL * lmax * run + extra, (what, u, err)
    if identical:
        assert path[:n] == res["path"].tolist() and start[:U].tolist() == res["start"].tolist() and end[:U].tolist() == res["end"].tolist(), what


# --------------------------------------------------------------------------------------------------------------------- kernel against the definition
N_CASES = len(ref.cases(17))


@pytest.mark.parametrize("i", range(N_CASES), ids=[c[0] for c in ref.cases(17)])
@pytest.mark.parametrize("V", [3, 17, 5002])
def test_kernel_against_the_definition(cfm, V, i):
    case = ref.cases(V)[i]
    name, kind, T, lens, labels, Umax = case[:6]
    logits, res = ref.case_reference(V, case)
    lab = ref.padded_labels(labels, Umax)
    llens = [len(l) for l in labels]
    lmax = float(logits.abs().max())
    Vp = (V + 3) // 4 * 4
    for ld in (Vp, Vp + 8):
        got = run_align(cfm, logits, V, lens, lab, llens, ld)
        for b, n in enumerate(lens):
            check_utterance(got, b, res[b], res[b]["lp"], labels[b], n, V, lmax, kind == "tie" or ref.exact(res[b], max(n, 1)), what=(name, V, ld, b))
    if name == "T==U+repeats-1":
        assert float(got[1][0]) == NEG
    if name == "ragged":
        assert float(got[1][0]) == 0.0                                                   # no frame, no label: the empty alignment


def test_host_validation(cfm):
    logits = torch.zeros((1, 4, 8), device=DEV)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="Umax=256"):
        cfm.ctc_align(logits, 5, i32([4]), torch.ones((1, 256), dtype=torch.int32, device=DEV), i32([1]))
    with pytest.raises(RuntimeError, match="row stride"):
        cfm.ctc_align(torch.zeros((1, 4, 6), device=DEV), 5, i32([4]), i32([[1]]), i32([1]))
    with pytest.raises(RuntimeError, match="row stride"):
        cfm.ctc_align(logits, 9, i32([4]), i32([[1]]), i32([1]))
    with pytest.raises(ValueError, match="batch sizes differ"):
        cfm.ctc_align(logits, 5, i32([4, 4]), i32([[1]]), i32([1]))
    with pytest.raises(ValueError, match="out must be"):
        cfm.ctc_align(logits, 5, i32([4]), i32([[1]]), i32([1]), out=tuple(torch.zeros((1, 4), device=DEV) for _ in range(5)))
    # the C entry itself: a scratch buffer one byte short, and a null output
    import ctypes
    need = cfm.lib().cfm_ctc_align_scratch_bytes(1, 4, 1)
    assert need == 1 * 4 * 4 and cfm.lib().cfm_ctc_align_scratch_bytes(32, 249, 33) == 32 * 249 * 68
    d = cfm.CtcAlignDesc()
    bufs = dict(logits=logits, enc_lens=i32([4]), labels=i32([[1]]), label_lens=i32([1]), work=torch.zeros(16, device=DEV), scratch=torch.zeros(16, dtype=torch.uint8, device=DEV),
                path=i32([0] * 4), score=torch.zeros(1, device=DEV), start=i32([0]), end=i32([0]), token_logp=torch.zeros(1, device=DEV))
    for k, v in bufs.items():
        setattr(d, k, v.data_ptr())
    d.ld, d.B, d.T, d.V, d.Umax, d.scratch_bytes = 8, 1, 4, 5, 1, need - 1
    assert cfm.lib().cfm_ctc_align(ctypes.byref(d), cfm.stream()) < 0 and b"scratch" in cfm.lib().cfm_last_error()
    d.scratch_bytes, d.token_logp = need, None
    assert cfm.lib().cfm_ctc_align(ctypes.byref(d), cfm.stream()) < 0 and b"null pointer" in cfm.lib().cfm_last_error()
    d.token_logp = bufs["token_logp"].data_ptr()
    assert cfm.lib().cfm_ctc_align(ctypes.byref(d), cfm.stream()) == 0
    torch.cuda.synchronize()
    assert bufs["path"].tolist() == [1, 1, 1, 1]                                         # constant logits, one label: the label state from frame 0 on (ties stay)


# ------------------------------------------------------------------------------------------------------- against the kernels that already exist
def test_score_is_bounded_by_the_nll(cfm):
    for V in (17, 5002):
        for case in ref.cases(V):
            if case[0] not in ("random-1", "random-2", "block-T67", "T==U+repeats-1", "ragged"):
                continue
            name, kind, T, lens, labels, Umax = case[:6]
            logits, res = ref.case_reference(V, case)
            lab, llens = ref.padded_labels(labels, Umax), [len(l) for l in labels]
            got = run_align(cfm, logits, V, lens, lab, llens)
            i32 = lambda v: torch.as_tensor(v, dtype=torch.int32).to(DEV)
            nll = cfm.ctc_nll(padded_cols(logits, V), V, i32(lens), lab.to(DEV), i32(llens)).cpu()
            for b, n in enumerate(lens):
                sc, total = float(got[1][b]), -float(nll[b])
                if not res[b]["feasible"]:
                    assert sc == NEG and total == NEG, (name, V, b)
                else:
                    assert sc <= total + ref.delta(max(n, 1), res[b]["score"]), (name, V, b, sc, total)


def test_planted_alignment_at_margin_30(cfm):
    """Logits that are 30 on one alignment's classes and 0 elsewhere: that alignment is the best path by far and carries all but e^-30 of the mass."""
    V, T = 17, 150
    labels = [[3, 3, 5, 1, 1, 1, 9, 2], [4, 4], []]
    lens = [150, 131, 70]
    planted = [ref.plant(l, n, 40 + b) for b, (l, n) in enumerate(zip(labels, lens))]
    logits = torch.zeros((3, T, V))
    for b, p in enumerate(planted):
        z = ref.extended(labels[b], V)
        for t, s in enumerate(p):
            logits[b, t, z[s]] = 30.0
    lab, llens = ref.padded_labels(labels, 8), [len(l) for l in labels]
    got = run_align(cfm, logits, V, lens, lab, llens, ld=28)
    i32 = lambda v: torch.as_tensor(v, dtype=torch.int32).to(DEV)
    nll = cfm.ctc_nll(padded_cols(logits, V), V, i32(lens), lab.to(DEV), i32(llens)).cpu()
    for b, n in enumerate(lens):
        lp = ref.log_probs(logits[b, :n], V)
        res = ref.align64(lp, labels[b], n)
        assert res["path"].tolist() == planted[b] and min(ref.decision_gap(res)) > 25.0
        check_utterance(got, b, res, lp, labels[b], n, V, 30.0, True, what=("planted", b))
        assert got[0][b, :n].tolist() == planted[b]
        assert abs(float(got[1][b]) + float(nll[b])) <= ref.delta(n, res["score"]), (b, float(got[1][b]), float(nll[b]))


def synth_head(V, D, seed):
    import decoder
    return synth.load_synth_(decoder.CTCDecoder(V, D, 0.0).eval(), seed)


def test_alignment_of_the_greedy_hypothesis_is_the_best_path(cfm, precision):
    """labels = the head's own best-path hypothesis: the best path is an alignment of it and no alignment of anything scores higher, so the forced
    alignment IS the best path -- each token starts at the frame greedy_search emitted it, and the score is the sum of the frames' top-1
    log-probabilities.  The inputs are the first seed whose float64 logits leave every valid frame a top-2 gap of 1e-3 max|logit| (20 times the fp32
    mode's error): chosen on the CPU."""
    precision("fp32")
    V, D, B, T = 17, 16, 3, 40
    lens = [40, 27, 1]
    for seed in range(900, 1000):
        head = synth_head(V, D, seed)
        x = torch.from_numpy(synth.normal(seed, (B, T, D), 1.0))
        z = x.double() @ head.ctc_lo.weight.detach().double().t() + head.ctc_lo.bias.detach().double()
        top2 = torch.sort(z, dim=-1, descending=True)[0][..., :2]
        gaps = [float((top2[b, :n, 0] - top2[b, :n, 1]).min()) for b, n in enumerate(lens)]
        if min(gaps) >= 1e-3 * float(z.abs().max()):
            break
    else:
        raise AssertionError("no seed with clear best-path decisions")
    lmax = float(z.abs().max())
    head = head.to(DEV)
    xl, ln = x.to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV)
    hyps, det = head.greedy_search(xl, ln, return_details=True)
    assert sum(len(h) for h in hyps) > 10
    Umax = max(len(h) for h in hyps)
    lab = ref.padded_labels(hyps, Umax)
    out = head.forced_align(xl, ln, lab, [len(h) for h in hyps], return_path=True)
    _, logp, _, _, _ = head._topk(xl, ln, 1, "greedy_search")
    logp, frames = logp.cpu().double(), det["frames"].cpu()
    for b, n in enumerate(lens):
        e = out[b]
        assert [t[0] for t in e["tokens"]] == hyps[b] and [t[1] for t in e["tokens"]] == frames[b, :len(hyps[b])].tolist(), b
        best = float(logp[b, :n, 0].sum())
        assert abs(e["score"] - best) <= ref.delta(n, best), (b, e["score"], best)
        lp = ref.log_probs(z[b, :n], V)                                                   # the float64 best path: the argmax of every frame
        assert [ref.extended(hyps[b], V)[s] for s in e["path"].tolist()] == lp.argmax(1).tolist(), b


# ----------------------------------------------------------------------------------------------------------------------------------------- modules
def test_forced_align_on_the_golden_head(cfm, precision):
    precision("fp32")
    g, meta = load_golden("ctc_head")
    n_exact = 0
    for c in meta["cases"]:
        name = c["name"]
        head = synth_head(c["V"], c["D"], c["wseed"])
        x = torch.from_numpy(synth.normal(c["xseed"], (c["B"], c["T"], c["D"]), 1.0))
        lens, labels, llens = (torch.from_numpy(g[name + k]) for k in ("_enc_lens", "_labels", "_label_lens"))
        z = x.double() @ head.ctc_lo.weight.detach().double().t() + head.ctc_lo.bias.detach().double()
        lmax = float(z.abs().max())
        head = head.to(DEV)
        out = head.forced_align(x.to(DEV), lens.to(DEV), labels.to(DEV), llens.to(DEV), return_path=True)
        plain = head.forced_align(x.to(DEV), lens.tolist(), labels, llens.tolist())
        assert len(out) == c["B"]
        for b in range(c["B"]):
            n, lab = int(lens[b]), labels[b, :int(llens[b])].tolist()
            lp = ref.log_probs(z[b, :n], c["V"])
            res = ref.align64(lp, lab, n)
            extra = 2 * n * FP32_MODE_REL * lmax
            delta = ref.delta(n, res["score"]) + extra
            e = out[b]
            assert res["feasible"] and e is not None and "path" not in plain[b] and plain[b] == {k: v for k, v in e.items() if k != "path"}, (name, b)
            assert e["path"].dtype == torch.int32 and e["path"].shape == (n,), (name, b)
            own = ref.path_score(e["path"].tolist(), lp, ref.extended(lab, c["V"]))
            print("forced_align", name, b, "score error %.3g own-path deficit %.3g delta %.3g" % (abs(e["score"] - res["score"]), res["score"] - own, delta))
            assert abs(e["score"] - res["score"]) <= delta and abs(own - res["score"]) <= delta, (name, b)
            sp = ref.spans(e["path"].tolist(), lp, ref.extended(lab, c["V"]))
            assert [t[0] for t in e["tokens"]] == lab and [t[1] for t in e["tokens"]] == sp["start"].tolist() and [t[2] for t in e["tokens"]] == sp["end"].tolist()
            for u, t in enumerate(e["tokens"]):
                assert abs(t[3] - sp["token_logp"][u]) <= (F32_REL * lmax + 2 * FP32_MODE_REL * lmax) * (t[2] - t[1] + 1), (name, b, u)
            if min(ref.decision_gap(res)) > delta:
                n_exact += 1
                assert e["path"].tolist() == res["path"].tolist(), (name, b)
    assert n_exact >= 1
    # an utterance without an alignment gives None; train mode and a wrong shape raise
    x = torch.from_numpy(synth.normal(3, (2, 5, c["D"]), 1.0)).to(DEV)
    out = head.forced_align(x, [5, 2], torch.tensor([[1, 2, 0], [4, 4, 0]]), [2, 2])
    assert out[1] is None and len(out[0]["tokens"]) == 2
    with pytest.raises(ValueError, match="must be \\[B, T, D\\]"):
        head.forced_align(x[0], [5], torch.tensor([[1]]), [1])
    with pytest.raises(ValueError, match="2 utterances"):
        head.forced_align(x, [5, 2, 1], torch.tensor([[1], [1]]), [1, 1])
    head.train()
    with pytest.raises(RuntimeError, match="eval-mode"):
        head.forced_align(x, [5, 2], torch.tensor([[1], [1]]), [1, 1])
    head.eval()


def offline_modules(meta):
    import encoder
    enc = synth.load_synth_(encoder.ConformerEncoder(cmvn=None, **meta["cfg"]).eval(), meta["wseed"])
    h = meta["head"]
    pr, jn = R.modules(h["V"], h["embed"], h["hidden"], h["P"], h["J"], h["layers"], meta["hseed"], enc_dim=meta["cfg"]["encoder_dim"], shaped=True)
    return enc, pr.to(DEV), jn.to(DEV)


def same_alignments(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            assert x["score"] == y["score"] and x["tokens"] == y["tokens"] and torch.equal(x["path"], y["path"])


def test_offline_recognizer_align(cfm, precision):
    import transducer
    precision("fp32")
    _, meta = load_golden("offline_asr")
    head = synth_head(73, meta["cfg"]["encoder_dim"], 700).to(DEV)
    enc, pr, jn = offline_modules(meta)
    enc = enc.to(DEV)
    lens = torch.tensor([meta["lens"][0], meta["lens"][2]], dtype=torch.int32, device=DEV)
    x = torch.from_numpy(synth.fbank(meta["xseed"], 2, max(meta["lens"]))).to(DEV)
    labels, llens = torch.tensor([[5, 9, 9, 2, 40], [7, 1, 0, 0, 0]]), [5, 2]
    rec = transducer.OfflineRecognizer(enc, pr, jn, blank=meta["blank"], n_steps=meta["n_steps"], ctc=head)
    got = rec.align(x, lens, labels, llens, return_path=True)
    out_lens = rec.encoder_out_lens.tolist()
    assert out_lens[0] != out_lens[1] and min(out_lens) >= 3
    with torch.no_grad():
        enc_out, enc_lens = enc.forward_utterances(x, lens)
    want = head.forced_align(enc_out, enc_lens, labels, llens, return_path=True)
    same_alignments(got, want)
    for b in range(2):
        assert got[b] is not None and len(got[b]["path"]) == out_lens[b] and [t[0] for t in got[b]["tokens"]] == labels[b, :llens[b]].tolist()
        assert all(0 <= t[1] <= t[2] < out_lens[b] for t in got[b]["tokens"])
    assert rec.frame_seconds(25) == 1.0                                                   # encoder frame i starts at feature frame 4 i, 10 ms each
    with pytest.raises(RuntimeError, match="without a CTC head"):
        transducer.OfflineRecognizer(enc, pr, jn, blank=meta["blank"]).align(x, lens, labels, llens)


def test_align_audio_is_align_on_the_fbank_features(cfm, precision):
    import fbank
    import transducer
    precision("fp32")
    _, meta = load_golden("offline_asr")
    rs = np.random.RandomState(5)
    n = [16000, 11213]
    samples = torch.from_numpy((3000.0 * rs.standard_normal((2, max(n)))).astype(np.int16)).to(DEV)
    lens = torch.tensor(n, dtype=torch.int32, device=DEV)
    fb = fbank.KaldiFbank()

    class Stats(torch.nn.Module):                      # global CMVN from the first utterance's log-mel rows: the synthetic encoder is made for features ~ N(0, 1)
        def __init__(self, rows):
            super().__init__()
            self.register_buffer("mean", rows.mean(0))
            self.register_buffer("istd", 1.0 / rows.std(0))

        def forward(self, x):
            return (x - self.mean) * self.istd

    enc, pr, jn = offline_modules(meta)
    enc.global_cmvn = Stats(fb(samples, lens)[0][0, :fb.num_frames(n[0])].cpu())
    enc = enc.to(DEV)
    head = synth_head(73, meta["cfg"]["encoder_dim"], 700).to(DEV)
    rec = transducer.OfflineRecognizer(enc, pr, jn, blank=meta["blank"], n_steps=meta["n_steps"], fbank=fb, ctc=head)
    labels, llens = torch.tensor([[5, 9, 9], [7, 1, 0]]), [3, 2]
    from_audio = rec.align_audio(samples, lens, labels, llens, return_path=True)
    from_feats = rec.align(*fb(samples, lens), labels, llens, return_path=True)
    same_alignments(from_audio, from_feats)
    assert all(e is not None and np.isfinite(e["score"]) for e in from_audio)
    rec_default = transducer.OfflineRecognizer(enc, pr, jn, blank=meta["blank"], n_steps=meta["n_steps"], ctc=head)      # fbank=None: KaldiFbank's defaults
    same_alignments(rec_default.align_audio(samples, lens, labels, llens, return_path=True), from_audio)
    assert rec_default.frame_seconds(25) == 1.0


# ------------------------------------------------------------------------------------------------------------------------------------ two streams
def test_two_streams_give_what_one_gives(cfm):
    """No host synchronisation inside the ABI and no scratch shared between streams: two alignments enqueued on two streams equal the same two run
    one after the other."""
    V = 17
    byname = {c[0]: c for c in ref.cases(V)}
    runs = []
    for name in ("U128-T300", "block-T129"):
        case = byname[name]
        logits, _ = ref.case_reference(V, case)
        i32 = lambda v: torch.as_tensor(v, dtype=torch.int32).to(DEV)
        runs.append((padded_cols(logits, V), i32(case[3]), ref.padded_labels(case[4], case[5]).to(DEV), i32([len(l) for l in case[4]])))
    serial = [[t.clone() for t in cfm.ctc_align(lg, V, ln, lab, ll)] for lg, ln, lab, ll in runs]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    both = []
    for st, (lg, ln, lab, ll) in zip(streams, runs):
        with torch.cuda.stream(st):
            both.append(cfm.ctc_align(lg, V, ln, lab, ll))
    torch.cuda.synchronize()
    for a, b in zip(serial, both):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    assert float(serial[0][1][0]) > NEG
