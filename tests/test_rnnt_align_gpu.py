"""GPU: RNN-T forced alignment on the device (cfm_rnnt_align / cfm_rnnt_packed_align in csrc/rnnt.hip through cfm.rnnt_align / rnnt_align_packed,
rnnt.rnnt_align, joint.TransducerJoint.forced_align and transducer.OfflineRecognizer.align(head="rnnt") / recognize(timestamps=True)) against the
float64 statement of tests/rnnt_align_ref.py.

Every operand lies between guard bands (tests/extent.py): the logits' pad columns V..ld are NaN, every output is pre-filled with NaN / -1 inside and
0xA5 around, so an owned element the kernel missed fails the comparison and a stray write fails G.check().

Bounds.  score: delta = 4 (Tb+Ub) 2^-23 max(1, |score|) + (Tb+Ub) 2e-6 max|logit| (rnnt_align_ref.delta: ctc_align_ref.delta's form over the path's
Tb + Ub moves, plus the row pass's f32 figure per move).  The device frames must be a valid alignment whose own float64 score is within delta of the
optimum; token_logp[u] within 2e-6 max|logit| of the float64 ll[frame[u], u].  Where every decision along the float64 optimal path is further than
2 delta from flipping (`exact`, settled on the CPU in test_rnnt_align_cpu.py) and in the constant-logit tie case the frames are the definition's.
End to end the logits carry the fp32 mode's error 5e-5 max|logit| (tests/test_modules_gpu.py), so delta grows by (Tb+Ub) times that."""
import ctypes

import numpy as np
import pytest
import torch

import greedy_ref as R
import rnnt_align_ref as ref
import synth
from conftest import load_golden
from extent import Guards

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
F32_REL = ref.F32_REL
FP32_MODE_REL = 5e-5                                         # tests/test_modules_gpu.py TOL["fp32"]
NEG = float("-inf")
i32 = lambda v: torch.as_tensor(v, dtype=torch.int32).to(DEV)


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


def outputs(G, B, W):
    return (G.out((B, W), torch.int32, name="frame"), G.out((B, W), name="token_logp"), G.out((B,), name="score"))


def run_padded(cfm, logits, targets, tl, ul, blank, V, ld):
    """cfm.rnnt_align between guard bands: logits [B,T,U1,V] (CPU) placed with row stride ld.  Returns (frame, token_logp, score) on the CPU."""
    B, U = targets.shape
    G = Guards()
    lg = G.inp(logits, ld=ld, name="logits")
    out = outputs(G, B, U)
    got = cfm.rnnt_align(lg, G.inp(targets, name="targets"), G.inp(torch.tensor(tl, dtype=torch.int32), name="logit_lens"),
                         G.inp(torch.tensor(ul, dtype=torch.int32), name="target_lens"), blank, V=V, out=out)
    torch.cuda.synchronize()
    G.check()
    assert all(a is b for a, b in zip(got, out))
    return [t.cpu() for t in out]


def run_packed(cfm, logits, targets, Tb, Ub, blank, V, ld):
    """cfm.rnnt_align_packed on the valid nodes of the same batch, between guard bands."""
    from cfm import lattice
    B, U = targets.shape
    T, U1 = logits.shape[1:3]
    lat = lattice.Lattice.padded(Tb, Ub, T, U1, DEV)
    rows = torch.cat([logits[b, :Tb[b], :Ub[b] + 1].reshape(-1, logits.shape[-1]) for b in range(B)])
    assert rows.shape[0] == lat.M
    G = Guards()
    out = outputs(G, B, lat.U1_max - 1)
    got = cfm.rnnt_align_packed(G.inp(rows, ld=ld, name="logits"), G.inp(targets, name="targets"), lat, blank, V=V, out=out)
    torch.cuda.synchronize()
    G.check()
    assert all(a is b for a, b in zip(got, out))
    return [t.cpu() for t in out]


def check_utterance(got, b, res, identical, extra=0.0, what=None):
    """One utterance of a run against its reference result `res` (rnnt_align_ref.reference)."""
    frame, tlp, score = (t[b] for t in got)
    Ub, sc = res["Ub"], float(score)
    assert frame[Ub:].tolist() == [-1] * (len(frame) - Ub) and bool((tlp[Ub:] == NEG).all()), what                # beyond the labels
    if not res["feasible"]:
        assert sc == NEG and frame[:Ub].tolist() == [-1] * Ub and bool((tlp[:Ub] == NEG).all()), what
        return
    delta = ref.delta(res["Tb"], Ub, res["score"], res["lmax"]) + extra
    fr = frame[:Ub].tolist()
    own = ref.path_score(fr, res["lb"], res["ll"])
    print("rnnt_align", what, "score error %.3g own-path deficit %.3g delta %.3g" % (abs(sc - res["score"]), res["score"] - own, delta))
    assert abs(sc - res["score"]) <= delta, (what, sc, res["score"], delta)
    assert own > NEG, (what, fr)                                                                                  # a valid alignment
    assert abs(own - res["score"]) <= delta, (what, own, res["score"], delta)
    for u in range(Ub):
        err = abs(float(tlp[u]) - float(res["ll"][fr[u], u]))
        assert err <= F32_REL * res["lmax"] + extra, (what, u, err)
    if identical:
        assert fr == res["frames"].tolist(), (what, fr, res["frames"].tolist())


# --------------------------------------------------------------------------------------------------------------------- kernel against the definition
CASES = [(V, c.name) for V in (3, 17, 5002) for c in ref.cases(V)]


@pytest.mark.parametrize("V,name", CASES, ids=["V%d-%s" % c for c in CASES])
def test_kernel_against_the_definition(cfm, V, name):
    case = {c.name: c for c in ref.cases(V)}[name]
    logits, targets, res = ref.case_reference(V, case)
    Tb, Ub = ref.clamped_lens(case)
    Vp = (V + 3) // 4 * 4
    runs = []
    for ld in (Vp, Vp + 8):
        got = run_padded(cfm, logits, targets, case.logit_lens, case.target_lens, case.blank, V, ld)
        packed = run_packed(cfm, logits, targets, Tb, Ub, case.blank, V, ld)
        W = packed[0].shape[1]
        for a, p in zip(got[:2], packed[:2]):                                            # the same bits on the same nodes; the padded form's further columns are fill
            assert torch.equal(a[:, :W].contiguous().view(torch.int32), p.view(torch.int32)), (name, V, ld)
        assert torch.equal(got[2].view(torch.int32), packed[2].view(torch.int32)), (name, V, ld)
        for b, r in enumerate(res):
            check_utterance(got, b, r, case.kind == "tie" or ref.exact(r), what=(name, V, ld, b))
        runs.append(got)
    for a, b in zip(*runs):                                                              # the row stride changes nothing
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (name, V)
    # against the loss on the same logits: no single path carries more than all of them
    nll = cfm.rnnt_nll(logits.to(DEV), targets.to(DEV), i32(case.logit_lens), i32(case.target_lens), case.blank)[0].cpu()
    for b, r in enumerate(res):
        sc, total = float(got[2][b]), -float(nll[b])
        if not r["feasible"]:
            assert sc == NEG and total == NEG, (name, V, b)
            continue
        delta = ref.delta(r["Tb"], r["Ub"], r["score"], r["lmax"])
        assert sc <= total + delta, (name, V, b, sc, total)
        if case.kind == "peaked":                                                        # the rest of the lattice carries < e^-25 of the mass
            assert sc >= total - 2 * delta, (name, V, b, sc, total)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_16_bit_logits(cfm, dtype):
    """rnnt.rnnt_align on 16-bit logits against the float64 reference on the same 16-bit values widened: only the arithmetic is tested."""
    import rnnt
    V = 17
    for name in ("random-1", "random-2", "ragged-clamped"):
        case = {c.name: c for c in ref.cases(V)}[name]
        logits, targets, _ = ref.case_reference(V, case)
        x = logits.to(dtype)
        res = ref.reference(x.double(), targets, case.logit_lens, case.target_lens, case.blank, V)
        got = [t.cpu() for t in rnnt.rnnt_align(x.to(DEV), targets.to(DEV), i32(case.logit_lens), i32(case.target_lens), blank=case.blank - V)]
        assert got[0].dtype == torch.int32 and got[1].dtype == torch.float32 and got[2].dtype == torch.float32
        for b, r in enumerate(res):
            check_utterance(got, b, r, ref.exact(r), what=(name, str(dtype), b))


def test_host_validation(cfm):
    z = lambda *s: torch.zeros(s, device=DEV)
    t32 = lambda *s: torch.ones(s, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match=r"cfm_rnnt_align: U\+1 = 1025 exceeds 1024"):
        cfm.rnnt_align(z(1, 1, 1025, 4), t32(1, 1024), i32([1]), i32([3]), 0)
    with pytest.raises(RuntimeError, match=r"cfm_rnnt_align: T = 8193 frames exceeds 8192"):
        cfm.rnnt_align(z(1, 8193, 1, 4), t32(1, 0), i32([1]), i32([0]), 0)
    with pytest.raises(RuntimeError, match=r"cfm_rnnt_align: blank 4 outside"):
        cfm.rnnt_align(z(1, 2, 2, 4), t32(1, 1), i32([2]), i32([1]), 4)
    with pytest.raises(RuntimeError, match=r"cfm_rnnt_align: blank -1 outside"):
        cfm.rnnt_align(z(1, 2, 2, 4), t32(1, 1), i32([2]), i32([1]), -1)
    with pytest.raises(ValueError, match=r"rnnt_align: .*out must be"):
        cfm.rnnt_align(z(1, 2, 2, 4), t32(1, 1), i32([2]), i32([1]), 0, out=(t32(1, 2), z(1, 1), z(1)))
    with pytest.raises(ValueError, match=r"rnnt_align: .*out must be"):                 # the right count in the wrong shape
        cfm.rnnt_align(z(2, 2, 4, 4), t32(2, 3), i32([2, 2]), i32([3, 3]), 0, out=(t32(3, 2), z(2, 3), z(2)))
    with pytest.raises(ValueError, match=r"rnnt_align: targets must be"):
        cfm.rnnt_align(z(2, 2, 2, 4), t32(1, 1), i32([2, 2]), i32([1, 1]), 0)
    from cfm import lattice
    lat = lattice.Lattice.padded([2], [1], 2, 2, DEV)
    with pytest.raises(RuntimeError, match=r"cfm_rnnt_packed_align: blank 4 outside"):
        cfm.rnnt_align_packed(z(4, 4), t32(1, 1), lat, 4)
    with pytest.raises(ValueError, match=r"rnnt_align_packed: .*out must be"):
        cfm.rnnt_align_packed(z(4, 4), t32(1, 1), lat, 0, out=(t32(1, 1), z(1, 1), z(2)))
    with pytest.raises(ValueError, match=r"rnnt_align_packed: logits must be \[M=4"):
        cfm.rnnt_align_packed(z(5, 4), t32(1, 1), lat, 0)
    # the C entry itself: the scratch size, a scratch buffer one byte short, and a null output
    L = cfm.lib()
    assert L.cfm_rnnt_align_scratch_bytes(0) == 0 and L.cfm_rnnt_align_scratch_bytes(3) == 8 and L.cfm_rnnt_align_scratch_bytes(16 * 249 * 101) == 2 * 16 * 249 * 101
    need = L.cfm_rnnt_align_scratch_bytes(1 * 3 * 2)
    d = cfm.RnntAlignDesc()
    bufs = dict(logits=torch.full((1, 3, 2, 4), ref.TIE_LOGIT, device=DEV), targets=t32(1, 1), logit_lens=i32([3]), target_lens=i32([1]), lse=z(6), lp_blank=z(6), lp_label=z(6))
    for k, v in bufs.items():
        setattr(d.r, k, v.data_ptr())
    d.r.ld, d.r.logits_dtype, d.r.B, d.r.T, d.r.U1, d.r.V, d.r.blank = 4, cfm.F32, 1, 3, 2, 4, 0
    frame, tlp, score, moves = i32([7]), z(1), z(1), torch.zeros(need, dtype=torch.uint8, device=DEV)
    d.frame, d.token_logp, d.score, d.scratch, d.scratch_bytes = frame.data_ptr(), tlp.data_ptr(), score.data_ptr(), moves.data_ptr(), need - 1
    assert L.cfm_rnnt_align(ctypes.byref(d), cfm.stream()) < 0 and b"cfm_rnnt_align: scratch" in L.cfm_last_error()
    d.scratch_bytes, d.score = need, None
    assert L.cfm_rnnt_align(ctypes.byref(d), cfm.stream()) < 0 and b"cfm_rnnt_align: null pointer" in L.cfm_last_error()
    d.score = score.data_ptr()
    assert L.cfm_rnnt_align(ctypes.byref(d), cfm.stream()) == 0                          # shift, alpha, beta, nll and the gradient fields are NULL
    torch.cuda.synchronize()
    assert frame.tolist() == [0] and abs(float(score) + 4 * np.log(4.0)) < 4e-5 and abs(float(tlp) + np.log(4.0)) < 1e-5     # constant logits: ties take the blank


def test_same_call_twice_gives_the_same_bits(cfm):
    V = 17
    for name in ("random-2", "T300-U2", "ragged-clamped"):
        case = {c.name: c for c in ref.cases(V)}[name]
        logits, targets, _ = ref.case_reference(V, case)
        args = (logits.to(DEV), targets.to(DEV), i32(case.logit_lens), i32(case.target_lens), case.blank)
        a = [t.clone() for t in cfm.rnnt_align(*args)]
        b = cfm.rnnt_align(*args)
        torch.cuda.synchronize()
        for x, y in zip(a, b):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), name


# ----------------------------------------------------------------------------------------------------------------------------------------- modules
def test_joint_forced_align(cfm, precision):
    """TransducerJoint.forced_align (the packed joint, then cfm_rnnt_packed_align) against the reference run on joint.forward's own logits."""
    import utils
    precision("fp32")
    V, J, B, T, U = 17, 16, 3, 9, 4
    pr, jn = R.modules(V, 16, 16, 16, J, 1, 321)
    pr, jn = pr.to(DEV), jn.to(DEV)
    enc_out = torch.from_numpy(synth.normal(322, (B, T, J), 1.0)).to(DEV)
    g = torch.Generator().manual_seed(323)
    labels = torch.randint(1, V, (B, U), generator=g)
    lens, ulens = [9, 0, 6], [4, 2, 3]
    with torch.no_grad():
        pred_out = pr(utils.add_blank(labels.to(DEV), 0, -1))
        logits = jn(enc_out, pred_out).float().cpu()
    res = ref.reference(logits, labels, lens, ulens, 0, V)
    out = jn.forced_align(enc_out, pred_out, labels, i32(lens), ulens, blank=0)
    assert len(out) == B and out[1] is None
    for b in (0, 2):
        r, e = res[b], out[b]
        extra = (r["Tb"] + r["Ub"]) * FP32_MODE_REL * r["lmax"]
        delta = ref.delta(r["Tb"], r["Ub"], r["score"], r["lmax"]) + extra
        assert [t[0] for t in e["tokens"]] == labels[b, :ulens[b]].tolist(), b
        fr = [t[1] for t in e["tokens"]]
        own = ref.path_score(fr, r["lb"], r["ll"])
        print("forced_align", b, "score error %.3g own-path deficit %.3g delta %.3g" % (abs(e["score"] - r["score"]), r["score"] - own, delta))
        assert abs(e["score"] - r["score"]) <= delta and own > NEG and abs(own - r["score"]) <= delta, (b, e["score"], r["score"], own)
        for u, t in enumerate(e["tokens"]):
            assert abs(t[2] - float(r["ll"][fr[u], u])) <= F32_REL * r["lmax"] + extra, (b, u)
        if min(r["gaps"], default=float("inf")) > 2 * delta:
            assert fr == r["frames"].tolist(), b
    with pytest.raises(ValueError, match="forced_align: 3 utterances"):
        jn.forced_align(enc_out, pred_out, labels[:2], lens, ulens)
    jn.train()
    with pytest.raises(RuntimeError, match="eval-mode"):
        jn.forced_align(enc_out, pred_out, labels, lens, ulens)
    jn.eval()


def synth_head(V, D, seed):
    import decoder
    return synth.load_synth_(decoder.CTCDecoder(V, D, 0.0).eval(), seed)


@pytest.fixture(scope="module")
def offline():
    """The golden offline recogniser's modules and a ragged feature batch."""
    import encoder
    _, meta = load_golden("offline_asr")
    enc = synth.load_synth_(encoder.ConformerEncoder(cmvn=None, **meta["cfg"]).eval(), meta["wseed"]).to(DEV)
    h = meta["head"]
    pr, jn = R.modules(h["V"], h["embed"], h["hidden"], h["P"], h["J"], h["layers"], meta["hseed"], enc_dim=meta["cfg"]["encoder_dim"], shaped=True)
    lens = torch.tensor([meta["lens"][0], meta["lens"][2]], dtype=torch.int32, device=DEV)
    x = torch.from_numpy(synth.fbank(meta["xseed"], 2, max(meta["lens"]))).to(DEV)
    return meta, enc, pr.to(DEV), jn.to(DEV), x, lens


def test_offline_recognizer_align_on_the_rnnt_head(cfm, precision, offline):
    import transducer
    import utils
    precision("fp32")
    meta, enc, pr, jn, x, lens = offline
    rec = transducer.OfflineRecognizer(enc, pr, jn, blank=meta["blank"], n_steps=meta["n_steps"])                  # no CTC head
    labels, llens = torch.tensor([[5, 9, 9, 2, 40], [7, 1, 63, 63, 63]]), [5, 2]
    got = rec.align(x, lens, labels, llens, head="rnnt")
    out_lens = rec.encoder_out_lens.tolist()
    text = torch.where(torch.arange(5)[None] < torch.tensor(llens)[:, None], labels, meta["blank"]).to(DEV)
    with torch.no_grad():
        want = jn.forced_align(rec.encoder_out, pr(utils.add_blank(text, meta["blank"], -1)), text, rec.encoder_out_lens, llens, blank=meta["blank"])
    assert got == want
    for b in range(2):
        fr = [t[1] for t in got[b]["tokens"]]
        assert [t[0] for t in got[b]["tokens"]] == labels[b, :llens[b]].tolist() and fr == sorted(fr) and all(0 <= f < out_lens[b] for f in fr), b
        assert np.isfinite(got[b]["score"]) and got[b]["score"] <= sum(t[2] for t in got[b]["tokens"]) + 1e-4
    with pytest.raises(RuntimeError, match="without a CTC head"):
        rec.align(x, lens, labels, llens)
    with pytest.raises(ValueError, match="return_path"):
        rec.align(x, lens, labels, llens, head="rnnt", return_path=True)
    with pytest.raises(ValueError, match="head must be"):
        rec.align(x, lens, labels, llens, head="attention")


def greedy_path_logp(logits, hyp, Tb, blank, n_steps):
    """The float64 log-probability of the path the greedy search took to emit `hyp`, on logits f64 [T, U+1, V] of that hypothesis: at node (t,u)
    the search emits the row's argmax (greedy_ref.argmax_within: the lowest index on ties), the next label or the blank.  None when that walk is
    no path of the lattice: the search hit its cap of n_steps symbols on a frame (it then moves on WITHOUT a blank), or an argmax within rounding
    of another went the other way on the device."""
    lp = torch.log_softmax(logits, -1)
    t = u = per_frame = 0
    s = 0.0
    while t < Tb:
        k = int(R.argmax_within(logits[t, u], 0.0)[0])
        if k != blank:
            if u >= len(hyp) or k != hyp[u] or per_frame + 1 >= n_steps:
                return None
            s, u, per_frame = s + float(lp[t, u, k]), u + 1, per_frame + 1
        else:
            s, t, per_frame = s + float(lp[t, u, blank]), t + 1, 0
    return s if u == len(hyp) else None


def test_recognize_with_timestamps(cfm, precision, offline):
    import transducer
    precision("fp32")
    meta, enc, pr, jn, x, lens = offline
    blank = meta["blank"]
    rec = transducer.OfflineRecognizer(enc, pr, jn, blank=blank, n_steps=meta["n_steps"])
    hyps = rec.recognize(x, lens)
    ts = rec.recognize(x, lens, timestamps=True)
    out_lens = rec.encoder_out_lens.tolist()
    assert sum(len(h) for h in hyps) > 4 and [e["tokens"] for e in ts] == hyps
    for b, e in enumerate(ts):
        n = len(hyps[b])
        assert len(e["frames"]) == n and len(e["logp"]) == n and e["frames"] == sorted(e["frames"]) and all(0 <= f < out_lens[b] for f in e["frames"]), b
        assert np.isfinite(e["score"]) and e["score"] <= sum(e["logp"]) + 1e-3, b
    assert rec.frame_seconds(25) == 1.0
    # with a beam: the n-best lists unchanged, and the best entries aligned
    nbest = rec.recognize(x, lens, beam=2)
    both = rec.recognize(x, lens, beam=2, timestamps=True)
    assert isinstance(both, tuple) and both[0] == nbest and [e["tokens"] for e in both[1]] == [list(n[0][0]) for n in nbest]
    assert all(e["frames"] == sorted(e["frames"]) for e in both[1])


class FixedEncoder(torch.nn.Module):
    """An encoder whose forward_utterances returns prepared outputs: the recogniser's search and alignment are under test here, not the encoder."""

    def __init__(self, out, lens):
        super().__init__()
        self.out, self.lens, self.encoder_dim = out, lens, out.shape[2]

    def forward_utterances(self, feats, lengths):
        return self.out, self.lens


def lattice_logits64(P, enc_proj, hyp, blank):
    """float64 joint logits [T, U+1, V] of one utterance over [blank] + hyp: greedy_ref's parameters, the oracle's predictor step per label."""
    from oracle import conformer_oracle as O
    L, H = R.num_layers(P), P["p.rnn.weight_hh_l0"].shape[1]
    h = c = torch.zeros((L, H), dtype=torch.float64)
    preds = []
    for token in [blank] + list(hyp):
        pred, h, c = O.predictor_step(P, "p.", token, h, c)
        preds.append(pred.reshape(-1))
    pf = torch.stack(preds) @ P["j.pred_ffn.weight"].t() + P["j.pred_ffn.bias"]
    return torch.tanh(enc_proj[:, None, :] + pf[None, :, :]) @ P["j.ffn_out.weight"].t() + P["j.ffn_out.bias"]


def test_viterbi_score_is_at_least_the_greedy_path(cfm, precision):
    """recognize(timestamps=True) aligns the greedy 1-best against itself, so its score is at least the log-probability of the path the greedy
    search itself took, on the same logits in float64, minus delta (+ the fp32 mode's share, as in test_joint_forced_align).  That path is a
    path of the lattice only while the search never hits its cap of n_steps symbols on a frame (a capped frame moves on WITHOUT a blank), and the
    synthetic heads either emit at the cap on every frame or emit nothing.  So the joint is made to depend on the label history (predictor path
    x 20, encoder path x 3, output x 8, blank bias + 8) and the inputs are the first seed whose float64 greedy search (greedy_ref.search64) emits
    tokens, never hits the cap and takes no decision within 1e-3 max|logit| (20 times the fp32 mode's error): chosen on the CPU, before the
    device is asked anything.  The encoder's outputs are given (FixedEncoder)."""
    import transducer
    precision("fp32")
    V, D, B, T, blank, n_steps = 17, 16, 3, 12, 0, 8
    lens = [12, 7, 0]
    for seed in range(400, 500):
        pr, jn = R.modules(V, 16, 16, 16, D, 1, seed, shaped=True)
        with torch.no_grad():
            jn.pred_ffn.weight.mul_(20.0)
            jn.enc_ffn.weight.mul_(3.0)
            jn.ffn_out.weight.mul_(8.0)
            jn.ffn_out.bias[blank] += 8.0
        P = R.params64(pr, jn)
        x = torch.from_numpy(synth.normal(seed + 1000, (B, T, D), 1.0))
        enc_proj = x.double() @ P["j.enc_ffn.weight"].t() + P["j.enc_ffn.bias"]
        want, logits, greedy = [], [], []
        for b in range(2):
            hyp = R.search64(P, enc_proj[b], lens[b], blank, n_steps, 0.0)[0]
            z = lattice_logits64(P, enc_proj[b], hyp, blank)
            clear = R.search64(P, enc_proj[b], lens[b], blank, n_steps, 1e-3 * float(z.abs().max()))[2] is None
            want.append(hyp), logits.append(z), greedy.append(greedy_path_logp(z, hyp, lens[b], blank, n_steps) if clear else None)
        if all(g is not None for g in greedy) and min(len(h) for h in want) >= 2:
            break
    else:
        raise AssertionError("no seed whose greedy search stays inside the lattice with clear decisions")
    rec = transducer.OfflineRecognizer(FixedEncoder(x.to(DEV), i32(lens)), pr.to(DEV), jn.to(DEV), blank=blank, n_steps=n_steps)
    hyps = rec.recognize(None, None)
    ts = rec.recognize(None, None, timestamps=True)
    assert hyps == want + [[]] and [e["tokens"] for e in ts] == hyps
    assert ts[2] == {"tokens": [], "frames": [], "logp": [], "score": NEG}                  # no encoder frame
    for b in range(2):
        e, n, lmax = ts[b], len(hyps[b]), float(logits[b].abs().max())
        delta = ref.delta(lens[b], n, greedy[b], lmax) + (lens[b] + n) * FP32_MODE_REL * lmax
        print("timestamps seed %d utterance %d: %d tokens, viterbi %.6f greedy path %.6f delta %.3g" % (seed, b, n, e["score"], greedy[b], delta))
        assert e["score"] >= greedy[b] - delta, (b, e["score"], greedy[b])                  # a Viterbi path is never worse than the greedy one
        assert e["frames"] == sorted(e["frames"]) and all(0 <= f < lens[b] for f in e["frames"]) and len(e["logp"]) == n, b


def test_defaults_are_the_code_paths_of_before(cfm, precision, offline):
    """recognize and align with their defaults, and with the new arguments spelled out at their defaults, return what the calls they wrapped
    before return: the greedy search's token lists, and the CTC head's forced alignment."""
    import transducer
    precision("fp32")
    meta, enc, pr, jn, x, lens = offline
    head = synth_head(73, meta["cfg"]["encoder_dim"], 700).to(DEV)
    rec = transducer.OfflineRecognizer(enc, pr, jn, blank=meta["blank"], n_steps=meta["n_steps"], ctc=head)
    a, b = rec.recognize(x, lens), rec.recognize(x, lens, timestamps=False)
    before = rec.search.search(rec.encoder_out, rec.encoder_out_lens)[0]
    assert a == b == before and all(isinstance(h, list) for h in a)
    labels, llens = torch.tensor([[5, 9, 9, 2, 40], [7, 1, 0, 0, 0]]), [5, 2]
    c, d = rec.align(x, lens, labels, llens, return_path=True), rec.align(x, lens, labels, llens, return_path=True, head="ctc")
    want = head.forced_align(rec.encoder_out, rec.encoder_out_lens, labels, llens, return_path=True)
    for got in (c, d):
        assert len(got) == len(want)
        for p, q in zip(got, want):
            assert p["score"] == q["score"] and p["tokens"] == q["tokens"] and torch.equal(p["path"], q["path"])
