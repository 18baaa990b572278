"""MI355X: the library's LSTM (csrc/lstm.hip through cfm.autograd.LSTMSeqFn) against float64 torch.nn.LSTM on the CPU, its dropout between
layers against tests/lstm_ref.py with the mask restated on the host, its extents, its refusals, RNNPredictor(fused=True) and the
transducer objective with a fused predictor.

Tolerance: every case also runs the SAME computation in float32 on the CPU (nn.LSTM; for p > 0, where nn.LSTM cannot take a mask, the
restatement of lstm_ref in float32) and gates each tensor of the kernel at 8 x that run's max|d| / max|ref| against float64 -- the order of
the sums and the exp-based activations differ from torch's, so nothing tighter is promised; a float32 CPU error above 1e-4 fails the case
as ill-conditioned."""
import copy
import functools

import numpy as np
import pytest
import torch

import extent
import lstm_ref
import synth
from conftest import load_golden
from test_lstm_cpu import flatten, layer_weights, lstm_case, torch_lstm_grads

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(1, 1, 64, 64, 1), (3, 5, 64, 64, 2), (17, 4, 128, 64, 2), (16, 7, 256, 256, 2), (33, 3, 64, 128, 3)]
SEED = 0x5EED


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


@functools.lru_cache(maxsize=None)
def reference(shape, p):
    """(case, float64 results, float32 CPU results) of a shape, computed once; p > 0: lstm_ref with the host's mask, else nn.LSTM."""
    B, U, I, H, L = shape
    case = lstm_case(B, U, I, H, L, seed=sum(shape))
    rnn, x, h0, c0, dy, dhn, dcn = case
    if p == 0.0:
        want = flatten(torch_lstm_grads(rnn, x, h0, c0, dy, dhn, dcn))
        f = lambda t: t.float()
        cpu32 = flatten(torch_lstm_grads(copy.deepcopy(rnn).float(), f(x), f(h0), f(c0), f(dy), f(dhn), f(dcn)))
    else:
        masks = lstm_ref.keep_masks(p, SEED, L, B, U, H)
        both = []
        for dt in (torch.float64, torch.float32):
            f = lambda t: None if t is None else t.to(dt)
            w = [tuple(f(t) for t in lw) for lw in layer_weights(rnn)]
            y, hn, cn, st = lstm_ref.forward(f(x), w, f(h0), f(c0), [f(m) for m in masks])
            both.append(flatten((y, hn, cn) + lstm_ref.backward(st, f(dy), f(dhn), f(dcn))))
        want, cpu32 = both
    return case, want, cpu32


def run_kernel(case, p, seed=SEED):
    from cfm.autograd import LSTMSeqFn
    rnn, x, h0, c0, dy, dhn, dcn = case
    L, H = rnn.num_layers, rnn.hidden_size
    g = lambda t: t.float().to(DEV)
    params = [g(t).requires_grad_(True) for lw in layer_weights(rnn) for t in lw]
    xg, h0g, c0g = g(x).requires_grad_(True), g(h0).requires_grad_(True), g(c0).requires_grad_(True)
    y, hn, cn = LSTMSeqFn.apply(xg, h0g, c0g, H, True, p, seed, *params)
    ((y * g(dy)).sum() + (hn * g(dhn)).sum() + (cn * g(dcn)).sum()).backward()
    grads = [tuple(t.grad for t in params[4 * l:4 * l + 4]) for l in range(L)]
    return flatten((y.detach(), hn.detach(), cn.detach(), xg.grad, grads, h0g.grad, c0g.grad))


def check_against(want, cpu32, got, what):
    for (n, w), (_, c), (_, k) in zip(want, cpu32, got):
        e32, ek = relerr(c, w), relerr(k, w)
        print("%s %-9s f32 CPU %.2e  kernel %.2e (%.1f x)" % (what, n, e32, ek, ek / max(e32, 1e-30)))
        assert e32 <= 1e-4, "%s %s: the float32 CPU run is %.2e off float64: ill-conditioned case" % (what, n, e32)
        assert ek <= 8 * e32, "%s %s: kernel %.3e against float64, float32 CPU %.3e" % (what, n, ek, e32)


@pytest.mark.parametrize("shape", SHAPES)
def test_lstm_equals_float64_nn_lstm(pkg, shape):
    case, want, cpu32 = reference(shape, 0.0)
    check_against(want, cpu32, run_kernel(case, 0.0), str(shape))


@pytest.mark.parametrize("shape", SHAPES)
def test_lstm_dropout_between_layers_equals_the_restated_mask(pkg, shape):
    """Also pins that the backward regenerates the forward's mask: every gradient below the top layer passes through it."""
    case, want, cpu32 = reference(shape, 0.5)
    check_against(want, cpu32, run_kernel(case, 0.5), "%s p=0.5" % (shape,))


@pytest.mark.parametrize("shape", SHAPES)
def test_lstm_is_reproducible_and_seeded(pkg, shape):
    case = reference(shape, 0.0)[0]
    a, b, c = run_kernel(case, 0.5, seed=7), run_kernel(case, 0.5, seed=7), run_kernel(case, 0.5, seed=8)
    for (n, x), (_, y) in zip(a, b):
        assert torch.equal(x, y), n
    if shape[4] > 1:                                                 # one layer has no dropout site
        assert not torch.equal(a[0][1], c[0][1])
    else:
        assert torch.equal(a[0][1], c[0][1])


def test_lstm_stays_inside_its_extents(pkg):
    import cfm
    B, U, I, H, L = 17, 4, 128, 64, 2
    rnn, x, h0, c0, dy, dhn, dcn = reference((B, U, I, H, L), 0.0)[0]
    f = lambda t: t.float().to(DEV)
    weights = [tuple(f(t) for t in lw) for lw in layer_weights(rnn)]
    drop = (0.5, SEED)
    y0, hn0, cn0, sv0 = cfm.lstm_forward(f(x), weights, H, f(h0), f(c0), drop=drop)
    dx0, gr0, dh00, dc00 = cfm.lstm_backward(f(x), weights, H, sv0, f(dy), f(dhn), f(dcn), drop=drop)
    n = sv0[0].numel()
    g = extent.Guards(DEV)
    gw = [tuple(g.inp(t, name="w%d" % l) for t in lw) for l, lw in enumerate(weights)]
    gx, gh0, gc0 = g.inp(f(x), name="x"), g.inp(f(h0), name="h0"), g.inp(f(c0), name="c0")
    out = (g.out((B, U, H), name="y"), g.out((L, B, H), name="hn"), g.out((L, B, H), name="cn"), [g.out((n,), name="save%d" % l) for l in range(L)])
    y, hn, cn, sv = cfm.lstm_forward(gx, gw, H, gh0, gc0, drop=drop, out=out)
    torch.cuda.synchronize()
    g.check()
    for a, b in [(y, y0), (hn, hn0), (cn, cn0)] + list(zip(sv, sv0)):
        assert torch.equal(a, b)                                     # every owned element written (the extents were NaN)
    g = extent.Guards(DEV)
    gw = [tuple(g.inp(t, name="w%d" % l) for t in lw) for l, lw in enumerate(weights)]
    gsv = [g.inp(s, name="save%d" % l) for l, s in enumerate(sv0)]
    grads = [tuple(g.out(tuple(t.shape), name="dw%d" % l) for t in lw) for l, lw in enumerate(weights)]
    out = (g.out((B, U, I), name="dx"), grads, g.out((L, B, H), name="dh0"), g.out((L, B, H), name="dc0"))
    work = (g.out((U * B, 4 * H), name="dg"), g.out((U * B, H), name="dyl"))
    dx, gr, dh0, dc0 = cfm.lstm_backward(g.inp(f(x), name="x"), gw, H, gsv, g.inp(f(dy), name="dy"), g.inp(f(dhn), name="dhn"), g.inp(f(dcn), name="dcn"),
                                         drop=drop, out=out, work=work)
    torch.cuda.synchronize()
    g.check()
    for a, b in [(dx, dx0), (dh0, dh00), (dc0, dc00)] + [(a, b) for ga, gb in zip(gr, gr0) for a, b in zip(ga, gb)]:
        assert torch.equal(a, b)


@pytest.mark.parametrize("I,H,L", [(64, 96, 1), (64, 576, 1), (64, 64, 5), (96, 64, 1)])
def test_unsupported_sizes_raise(pkg, I, H, L):
    import predictor
    pr = predictor.RNNPredictor(20, I, 32, H, 0.0, L, dropout=0.0, fused=True).to(DEV).eval()
    with pytest.raises((ValueError, RuntimeError), match="multiples of 64|layers"):
        pr(torch.zeros(2, 3, dtype=torch.long, device=DEV))
    lib = pkg.cfm.lib()
    d = pkg.cfm.LstmDesc()
    d.B, d.U, d.in_, d.H, d.layers = 2, 3, I, H, L
    assert lib.cfm_lstm_forward(d, None) == -1 and lib.cfm_lstm_backward(d, None) == -1          # CFM_ERR_ARG before any pointer is looked at


def test_fused_predictor_equals_the_stock_module(pkg):
    import predictor
    torch.manual_seed(5)
    stock = predictor.RNNPredictor(50, 64, 40, 64, 0.1, 2, dropout=0.1).eval()
    labels = torch.randint(0, 50, (4, 6))
    with torch.no_grad():
        want = copy.deepcopy(stock).double()(labels)
        e32 = relerr(stock(labels), want)
    fused = predictor.RNNPredictor(50, 64, 40, 64, 0.1, 2, dropout=0.1, fused=True)
    fused.load_state_dict(stock.state_dict())
    stock, fused = stock.to(DEV), fused.to(DEV).eval()
    with torch.no_grad():
        got, got_stock = fused(labels.to(DEV)), stock(labels.to(DEV))
        ek = relerr(got, want)
        print("predictor (4, 6): f32 CPU %.2e, fused %.2e, stock on the GPU %.2e" % (e32, ek, relerr(got_stock, want)))
        assert e32 <= 1e-4 and ek <= 8 * e32
        cache = [t + 0.1 for t in fused.init_state(labels.to(DEV))]
        pad = torch.tensor([[0.0], [1.0], [0.0], [0.0]], device=DEV)
        a, (ha, ca) = fused.forward_step(labels[:, :1].to(DEV), pad, cache)
        b, (hb, cb) = stock.forward_step(labels[:, :1].to(DEV), pad, cache)
    assert torch.equal(a, b) and torch.equal(ha, hb) and torch.equal(ca, cb)


def build_objective(V=73, P=40, J=64):
    import decoder
    import encoder
    import joint
    import predictor
    import transducer
    g, meta = load_golden("train_cfg1")                              # the smallest encoder of the transducer tests
    cfg = dict(meta["cfg"], dropout=0.0, attention_dropout=0.0, pos_enc_dropout=0.0)
    enc = synth.load_synth_(encoder.ConformerEncoder(cmvn=None, **cfg), meta["wseed"])
    ctc = synth.load_synth_(decoder.CTCDecoder(V, cfg["encoder_dim"], 0.0), meta["cseed"])
    torch.manual_seed(11)
    pr = predictor.RNNPredictor(V, 64, P, 64, 0.0, 2, dropout=0.0)
    jn = joint.TransducerJoint(V, cfg["encoder_dim"], P, J)
    obj = transducer.TransducerObjective(enc, pr, jn, ctc, blank=0, ignore_id=-1, ctc_weight=0.2, transducer_weight=0.8)
    return obj.to(DEV).train()


def micro_batches(n, seed, V=73):
    import trainer as T
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        feats, lens, labels, label_lens = T.librispeech_shaped_batch(rs, max_frames_in_batch=1600, min_len=120, max_len=400, vocab=V)
        for b in range(labels.shape[0]):
            labels[b, label_lens[b]:] = -1
        out.append((None,) + tuple(torch.from_numpy(a).to(DEV) for a in (feats, lens, labels, label_lens)) + (None,))
    return out


def test_objective_with_a_fused_predictor_equals_the_stock_one(pkg):
    """TransducerObjective.forward and forward_window (two micro-batches of different Umax): losses and the predictor's parameter gradients
    within the window-against-loop gate of tests/test_rnnt_packed_gpu.py (1e-5 in the f32-accurate mode)."""
    cfm = pkg.cfm
    cfm.set_precision("fp32")
    cfm.set_deterministic(True)
    try:
        stock = build_objective()
        fused = copy.deepcopy(stock)
        fused.predictor.fused = True
        data = micro_batches(2, 77)
        _, feats, lens, labels, label_lens, _ = data[1]              # the second micro-batch gets a shorter label matrix: another Umax
        data[1] = (None, feats, lens, labels[:, :7].contiguous(), label_lens.clamp(max=7), None)
        assert data[0][3].shape[1] != data[1][3].shape[1]
        for what, loss_of in (("forward", lambda o: o(data[0])["loss"]), ("forward_window", lambda o: (o.forward_window(data) * torch.tensor([1.0, 0.7], device=DEV)).sum())):
            grads = {}
            for name, obj in (("stock", stock), ("fused", fused)):
                obj.zero_grad()
                loss = loss_of(obj)
                loss.backward()
                grads[name] = (loss.detach(), {k: p.grad.clone() for k, p in obj.predictor.named_parameters()})
            (ls, gs), (lf, gf) = grads["stock"], grads["fused"]
            assert torch.isfinite(lf) and relerr(lf, ls) <= 1e-5, (what, float(lf), float(ls))
            for k in gs:
                e = relerr(gf[k], gs[k])
                print("%s %s grad |d| / max %.2e" % (what, k, e))
                assert e <= 1e-5, (what, k, e)
    finally:
        cfm.set_precision("bf16")
        cfm.set_deterministic(False)
