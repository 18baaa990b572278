"""MI355X: packed RNN-T lattices -- rnnt.rnnt_loss_packed against rnnt.rnnt_loss on the same nodes, the fused packed joint + loss
(TransducerJoint.rnnt_loss(packed=True)) against the float64 chain and the padded path, its memory on a ragged batch, the window forms
(TransducerJoint.forward_window, TransducerObjective.forward_window under DataParallelTrainer) and one config-3 window."""
import copy

import numpy as np
import pytest
import torch

import rnnt_ref
import synth
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
FUSED_TOL = {"fp32": 3e-5, "fp16": 2e-3, "bf16": 1.5e-2}       # the gates of tests/test_rnnt_gpu.py
CONFIG4_TOL = 4e-2


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    mod = g._import_package()
    yield mod
    mod.cfm.set_precision("bf16")
    mod.cfm.set_deterministic(False)


def relerr(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def rows_of(padded, T, U):
    """The packed rows of a padded [B, T, U1, ...] tensor (cfm.lattice.row_nodes order)."""
    from cfm import lattice
    b, t, u = (torch.from_numpy(x).to(padded.device) for x in lattice.row_nodes(T, U))
    return padded[b, t, u]


CASES = [  # B, T, U, V, blank, reduction, clamp, dtype
    (5, 12, 5, 5002, 0, "mean", -1, torch.float32),
    (5, 9, 4, 37, -1, "sum", -1, torch.float32),
    (5, 10, 6, 5001, 0, "none", -1, torch.float32),
    (5, 8, 3, 63, -1, "mean", 0.02, torch.float32),
    (3, 6, 70, 33, 0, "sum", -1, torch.float32),               # U+1 > 64
    (5, 10, 4, 5002, 0, "none", -1, torch.float16),
    (5, 10, 4, 5001, -1, "sum", 0.05, torch.bfloat16),
]


def ragged(B, T, U):
    tl = [T, 1, max(1, T - 3), 0, max(1, T // 2)][:B]            # T_b = 1 and T_b = 0
    ul = [U, max(0, U - 1), 0, max(0, U - 2), U // 2][:B]        # U_b = 0
    return tl, ul


@pytest.mark.parametrize("case", CASES, ids=lambda c: "B%d_T%d_U%d_V%d_b%d_%s_cl%g_%s" % (c[:7] + (str(c[7])[6:],)))
def test_packed_loss_equals_padded_loss(pkg, case):
    import rnnt
    B, T, U, V, blank, reduction, clamp, dtype = case
    g = torch.Generator().manual_seed(B * 1000 + T * 10 + U)
    logits = (torch.randn((B, T, U + 1, V), generator=g) * 3).to(dtype).to(DEV)
    targets = torch.randint(1, V, (B, U), generator=g, dtype=torch.int32).to(DEV)
    tl, ul = ragged(B, T, U)
    tld, uld = torch.tensor(tl, device=DEV), torch.tensor(ul, device=DEV)
    x = logits.clone().requires_grad_(True)
    costs = rnnt.rnnt_loss(x, targets, tld, uld, blank=blank, clamp=clamp, reduction="none")
    loss = rnnt.rnnt_loss(x, targets, tld, uld, blank=blank, clamp=clamp, reduction=reduction)
    (loss.sum() if reduction == "none" else loss).backward()
    packed = rows_of(logits, tl, ul).contiguous().requires_grad_(True)
    pcosts = rnnt.rnnt_loss_packed(packed, targets, tld, uld, blank=blank, clamp=clamp, reduction="none")
    ploss = rnnt.rnnt_loss_packed(packed, targets, tld, uld, blank=blank, clamp=clamp, reduction=reduction)
    (ploss.sum() if reduction == "none" else ploss).backward()
    fin = torch.isfinite(costs)
    assert torch.equal(torch.isfinite(pcosts), fin) and (B < 4 or not bool(fin[3]))
    assert relerr(pcosts[fin], costs[fin]) <= 1e-6
    print("costs bit-identical: %s, loss %s / %s" % (torch.equal(pcosts[fin], costs[fin]), ploss.detach().cpu().numpy(), loss.detach().cpu().numpy()))
    gp, gref = packed.grad.float(), rows_of(x.grad, tl, ul).float()
    assert relerr(gp, gref) <= 1e-6
    if B >= 4:
        assert float(x.grad[3].abs().max()) == 0.0              # T_b = 0: zero gradient


def test_in_place_16bit_over_f32_and_determinism(pkg):
    import cfm
    from cfm import lattice
    B, T, U, V = 5, 11, 6, 5002
    g = torch.Generator().manual_seed(4)
    tl, ul = ragged(B, T, U)
    lat = lattice.Lattice.padded(tl, ul, T, U + 1, DEV)
    logits = (torch.randn((lat.M, V), generator=g) * 3).to(DEV)
    targets = torch.randint(1, V, (B, U), generator=g, dtype=torch.int32).to(DEV)
    gdev = torch.full((B,), 0.5, device=DEV)

    def run(out_of):
        nll, st = cfm.rnnt_nll_packed(logits, targets, lat, 0)
        return nll, out_of(st)

    nll1, ref = run(lambda st: cfm.rnnt_grad(st, torch.empty_like(logits), gscale_dev=gdev))
    nll2, ref2 = run(lambda st: cfm.rnnt_grad(st, torch.empty_like(logits), gscale_dev=gdev))
    assert torch.equal(nll1, nll2) and torch.equal(ref, ref2)       # two calls, same bits
    keep = logits.clone()
    _, inplace = run(lambda st: cfm.rnnt_grad(st, logits, gscale_dev=gdev))
    assert inplace.data_ptr() == logits.data_ptr() and torch.equal(inplace, ref)
    logits.copy_(keep)
    _, sep16 = run(lambda st: cfm.rnnt_grad(st, torch.empty((lat.M, V), dtype=torch.bfloat16, device=DEV), gscale_dev=gdev))
    half = logits.view(torch.bfloat16)
    run(lambda st: cfm.rnnt_grad(st, half, gscale_dev=gdev, cols=V))
    assert torch.equal(half[:, :V], sep16)
    assert relerr(sep16.float(), ref) <= 1e-2


def joint_f64(jn, xe, xp):
    e = xe @ jn.enc_ffn.weight.t() + jn.enc_ffn.bias
    p = xp @ jn.pred_ffn.weight.t() + jn.pred_ffn.bias
    return torch.tanh(e.unsqueeze(2) + p.unsqueeze(1)) @ jn.ffn_out.weight.t() + jn.ffn_out.bias


def fused(jn, xe, xp, targets, tl, ul, packed, reduction="mean"):
    xe, xp = xe.detach().clone().requires_grad_(True), xp.detach().clone().requires_grad_(True)
    jn.zero_grad()
    loss = jn.rnnt_loss(xe, xp, targets, tl, ul, blank=0, reduction=reduction, packed=packed)
    loss.backward()
    return [loss.detach(), xe.grad, xp.grad] + [p.grad.clone() for p in jn.parameters()]


@pytest.mark.parametrize("mode", ["bf16", "fp16", "fp32"])
def test_fused_packed_joint_matches_the_float64_chain(pkg, mode):
    import joint
    torch.manual_seed(7)
    B, T, U, E, P, J, V = 5, 9, 4, 40, 24, 64, 37
    jn = joint.TransducerJoint(V, E, P, J).to(DEV).train()
    jn.precision = mode
    xe = torch.randn(B, T, E, device=DEV)
    xp = torch.randn(B, U + 1, P, device=DEV)
    targets = torch.randint(1, V, (B, U), dtype=torch.int32, device=DEV)
    tl, ul = [9, 1, 6, 4, 5], [4, 0, 2, 1, 3]
    tld, uld = torch.tensor(tl, device=DEV), torch.tensor(ul, device=DEV)
    got = fused(jn, xe, xp, targets, tld, uld, True)
    ref = copy.deepcopy(jn).cpu().double()
    re, rp = xe.cpu().double().requires_grad_(True), xp.cpu().double().requires_grad_(True)
    lb, ll = rnnt_ref.lattice_logprobs(joint_f64(ref, re, rp), targets.cpu(), 0)
    rloss = rnnt_ref.costs_from_lattice(lb, ll, tld.cpu(), uld.cpu()).mean()
    rloss.backward()
    want = [rloss.detach(), re.grad, rp.grad] + [q.grad for q in ref.parameters()]
    errs = [relerr(a, b) for a, b in zip(got, want)]
    print(mode, ["%.1e" % e for e in errs])
    assert max(errs) <= FUSED_TOL[mode], errs
    for b in range(B):                                           # frames t >= T_b and predictor rows u > U_b: exact zeros
        assert float(got[1][b, tl[b]:].abs().sum()) == 0.0
        assert float(got[2][b, ul[b] + 1:].abs().sum()) == 0.0
    if mode == "fp32":
        pad = fused(jn, xe, xp, targets, tld, uld, False)
        errs = [relerr(a, b) for a, b in zip(got, pad)]
        assert max(errs) <= 1e-5, errs


def test_packed_memory_on_a_ragged_batch(pkg):
    import joint
    torch.manual_seed(3)
    Ts = [320, 256, 192, 128, 64, 32]
    Us = [t // 8 for t in Ts]
    B, T, U, E, P, J, V = len(Ts), Ts[0], Us[0], 256, 256, 512, 5002
    jn = joint.TransducerJoint(V, E, P, J).to(DEV).train()
    jn.precision = "bf16"
    xe = torch.randn(B, T, E, device=DEV, requires_grad=True)
    xp = torch.randn(B, U + 1, P, device=DEV, requires_grad=True)
    targets = torch.randint(1, V, (B, U), dtype=torch.int32, device=DEV)
    tl, ul = torch.tensor(Ts, device=DEV), torch.tensor(Us, device=DEV)
    cells = sum(t * (u + 1) for t, u in zip(Ts, Us)) / (B * T * (U + 1))
    peaks = {}
    for packed in (True, False, True):                           # the first call warms the weight packs and the scratch arena
        xe.grad = xp.grad = None
        jn.zero_grad()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        jn.rnnt_loss(xe, xp, targets, tl, ul, packed=packed).backward()
        torch.cuda.synchronize()
        peaks[packed] = torch.cuda.max_memory_allocated() - base
    print("valid cells %.2f of padded; peak packed %.3f GB, padded %.3f GB (ratio %.2f)" % (cells, peaks[True] / 1e9, peaks[False] / 1e9,
                                                                                           peaks[True] / peaks[False]))
    assert abs(cells - 0.37) < 0.01
    assert peaks[True] <= 0.5 * peaks[False], peaks


def window_case(pkg, mode, seed=5):
    import joint
    torch.manual_seed(seed)
    E, P, J, V = 48, 40, 64, 53
    jn = joint.TransducerJoint(V, E, P, J).to(DEV).train()
    jn.precision = mode
    shapes = [(3, 13, 5, [13, 9, 4], [5, 2, 0]), (2, 7, 3, [7, 1], [3, 1])]
    groups = []
    for B, T, U, tl, ul in shapes:
        groups.append((B, T, torch.tensor(tl, device=DEV), torch.randn(B, U + 1, P, device=DEV),
                       torch.randint(1, V, (B, U), dtype=torch.int32, device=DEV), torch.tensor(ul, device=DEV)))
    rows = torch.randn(sum(B * T for B, T, *_ in shapes), E, device=DEV)
    return jn, rows, groups


def test_joint_forward_window_equals_per_micro_batch_losses(pkg):
    jn, rows, groups = window_case(pkg, "fp32")
    rows_w = rows.clone().requires_grad_(True)
    preds_w = [g[3].clone().requires_grad_(True) for g in groups]
    losses = jn.forward_window(rows_w, [(B, T, el, pw, tg, tl) for (B, T, el, _, tg, tl), pw in zip(groups, preds_w)])
    assert losses.shape == (2,)
    (losses * torch.tensor([1.0, 0.7], device=DEV)).sum().backward()
    wgrads = [p.grad.clone() for p in jn.parameters()]
    jn.zero_grad()
    r0, drows = 0, []
    for (B, T, el, po, tg, tl), w, lw, pw in zip(groups, [1.0, 0.7], losses, preds_w):
        xe = rows[r0:r0 + B * T].view(B, T, -1).clone().requires_grad_(True)
        xp = po.clone().requires_grad_(True)
        l = jn.rnnt_loss(xe, xp, tg, el, tl, blank=0, reduction="mean")
        (w * l).backward()
        assert relerr(lw, l) <= 1e-5
        assert relerr(pw.grad, xp.grad) <= 1e-5
        drows.append(xe.grad.reshape(B * T, -1))
        r0 += B * T
    assert relerr(rows_w.grad, torch.cat(drows)) <= 1e-5
    for a, p in zip(wgrads, jn.parameters()):
        assert relerr(a, p.grad) <= 1e-5


def build_objective(pkg, V=73, P=40, J=64):
    import decoder
    import encoder
    import joint
    import predictor
    import transducer
    g, meta = load_golden("train_cfg1")
    enc = synth.load_synth_(encoder.ConformerEncoder(cmvn=None, **meta["cfg"]), meta["wseed"])
    ctc = synth.load_synth_(decoder.CTCDecoder(V, meta["cfg"]["encoder_dim"], 0.0), meta["cseed"])
    torch.manual_seed(11)
    pr = predictor.RNNPredictor(V, 32, P, 48, 0.0, 2, dropout=0.0)
    jn = joint.TransducerJoint(V, meta["cfg"]["encoder_dim"], P, J)
    obj = transducer.TransducerObjective(enc, pr, jn, ctc, blank=0, ignore_id=-1, ctc_weight=0.2, transducer_weight=0.8)
    return obj.to(DEV).train()


def micro_batches(n, seed, V=73):
    import trainer as T
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        feats, lens, labels, label_lens = T.librispeech_shaped_batch(rs, max_frames_in_batch=1600, min_len=120, max_len=400, vocab=V)
        for b in range(labels.shape[0]):
            labels[b, label_lens[b]:] = -1                        # the reference pads labels with ignore_id
        out.append((None,) + tuple(torch.from_numpy(a).to(DEV) for a in (feats, lens, labels, label_lens)) + (None,))
    return out


@pytest.mark.parametrize("mode,tol", [("fp32", 1e-5), ("bf16", 5e-3)])
def test_objective_window_under_the_trainer_equals_the_micro_batch_loop(pkg, mode, tol):
    import cfm
    import trainer as T
    cfm.set_precision(mode)
    cfm.set_deterministic(True)
    try:
        obj = build_objective(pkg)
        obj_r = copy.deepcopy(obj)
        data = micro_batches(2, 77)
        mods = lambda o: [o.encoder, o.ctc, o.predictor, o.joint]
        tr_w = T.DataParallelTrainer(mods(obj), lambda mb: obj(mb)["loss"], accum_grad=2, window_loss_fn=obj.forward_window)
        tr_l = T.DataParallelTrainer(mods(obj_r), lambda mb: obj_r(mb)["loss"], accum_grad=2)
        grads = {}
        for name, tr in (("window", tr_w), ("loop", tr_l)):
            fin = tr.finish
            tr.finish = lambda tr=tr, fin=fin, name=name: (grads.__setitem__(name, tr.flat_g.clone()), fin())[1]
        lw, ll = tr_w.step(data), tr_l.step(data)
        gw, gl = grads["window"], grads["loop"]
        print(mode, "loss window %.6f loop %.6f, grad |d| / max %.2e" % (float(lw), float(ll), float((gw - gl).abs().max() / gl.abs().max())))
        assert torch.isfinite(lw) and relerr(lw, ll) <= 1e-5
        assert float((gw - gl).abs().max() / gl.abs().max()) <= tol
    finally:
        cfm.set_precision("bf16")
        cfm.set_deterministic(False)


def test_objective_forward_equals_the_model_py_composition(pkg):
    import cfm
    import utils
    cfm.set_precision("fp32")
    try:
        obj = build_objective(pkg)
        mb = micro_batches(1, 91)[0]
        out = obj(mb)
        _, feats, lens, labels, label_lens, _ = mb
        y, m = obj.encoder(feats, lens)
        y_lens = m.squeeze(1).sum(1)
        pred = obj.predictor(utils.add_blank(labels, 0, -1))
        text = torch.where(labels == -1, 0, labels).to(torch.int32)
        l_rnnt = obj.joint.rnnt_loss(y, pred, text, y_lens.to(torch.int32), label_lens.to(torch.int32), blank=0, reduction="mean")
        l_ctc = obj.ctc(y, y_lens, labels, label_lens).sum()
        assert set(out) == {"loss", "loss_ctc", "loss_rnnt", "encoder_out", "encoder_out_lens"}
        assert relerr(out["loss_rnnt"], l_rnnt) <= 1e-5 and relerr(out["loss_ctc"], l_ctc) <= 1e-5
        assert relerr(out["loss"], 0.2 * l_ctc + 0.8 * l_rnnt) <= 1e-5
        assert torch.equal(out["encoder_out_lens"], y_lens)
    finally:
        cfm.set_precision("bf16")


def test_config3_window(pkg):
    """One full window of two LibriSpeech-shaped micro-batches (seed 1234), bf16, V 5002, J 512: TransducerJoint.forward_window against the
    padded joint per micro-batch, on the same encoder rows and predictor outputs."""
    import joint
    import trainer as T
    rs = np.random.RandomState(1234)
    E, P, J, V = 256, 256, 512, 5002
    torch.manual_seed(2)
    jn = joint.TransducerJoint(V, E, P, J).to(DEV).train()
    jn.precision = "bf16"
    groups, sizes = [], []
    for _ in range(2):
        _, lens, labels, label_lens = T.librispeech_shaped_batch(rs)
        B = len(lens)
        t_sub = ((lens.astype(np.int64) - 1) // 2 - 1) // 2          # two stride-2 kernel-3 convolutions
        Tp, U = int(t_sub.max()), labels.shape[1]
        groups.append((B, Tp, torch.from_numpy(t_sub).to(DEV), torch.randn(B, U + 1, P, device=DEV),
                       torch.from_numpy(labels).to(DEV, torch.int32), torch.from_numpy(label_lens).to(DEV)))
        sizes.append(B * Tp)
    rows = torch.randn(sum(sizes), E, device=DEV, requires_grad=True)
    preds = [g[3].requires_grad_(True) for g in groups]
    losses = jn.forward_window(rows, groups)
    assert bool(torch.isfinite(losses).all())
    losses.sum().backward()
    d_rows, d_preds = rows.grad.clone(), [p.grad.clone() for p in preds]
    r0 = 0
    for gi, (B, Tp, el, po, tg, tl) in enumerate(groups):
        xe = rows.detach()[r0:r0 + B * Tp].view(B, Tp, E).clone().requires_grad_(True)
        xp = po.detach().clone().requires_grad_(True)
        l = jn.rnnt_loss(xe, xp, tg, el, tl, blank=0, reduction="mean")
        l.backward()
        assert relerr(losses[gi].detach(), l.detach()) <= 1e-3
        for b in (0, B // 2, B - 1):
            errs = relerr(d_rows[r0 + b * Tp:r0 + (b + 1) * Tp], xe.grad[b]), relerr(d_preds[gi][b], xp.grad[b])
            print("config 3 window, micro-batch %d utterance %d: d enc rows %.1e, d pred_out %.1e" % (gi, b, errs[0], errs[1]))
            assert max(errs) <= CONFIG4_TOL, (gi, b, errs)
            assert float(xe.grad[b].abs().max()) > 0 and float(xp.grad[b].abs().max()) > 0
        r0 += B * Tp
        del xe, xp, l
