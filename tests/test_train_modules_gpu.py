"""GPU: TRAIN-mode forward + backward of the drop-in modules (autograd Functions over the C ABI) against
 (1) the reference's own losses / parameter gradients / BatchNorm running statistics (tests/golden/train_*.npz, produced by running
     the reference in train mode with every dropout probability 0), and
 (2) the CPU oracle under torch.autograd on shapes the goldens do not cover (BASELINE config 4's d = 512, h = 8).

Gradient error metric (conftest.grad_err): max|d| / max(max|ref|, floor) per tensor, floor = 1e-2 (modules) or 1e-3 (whole encoder) of
the largest gradient of the case -- structurally-zero gradients (depthwise bias under BatchNorm, pos_bias_v, linear_pos, linear_k.bias)
are rounding noise in the reference and exact or near-exact zeros here.
Gates:  fp32 ("f32-accurate") <= 1e-3 (the north-star tolerance);  fp16 / bf16: about 1.5x what was measured on MI355X (printed).
"""
import numpy as np
import pytest
import torch

import synth
from conftest import grad_err, grad_ref_max, load_golden

pytestmark = pytest.mark.gpu

MODES = ["bf16", "fp16", "fp32"]
DEV = "cuda"
# module-level gates: (forward output, gradients)
# measured (round 3): fp32 7.1e-6 / 1.3e-5, fp16 5.2e-4 / 1.4e-3, bf16 3.5e-3 / 1.1e-2 -- gates at ~2x
MOD_TOL = {"fp32": (2e-5, 5e-5), "fp16": (1e-3, 3e-3), "bf16": (7e-3, 2.2e-2)}
# whole encoder + CTC: (loss relative, output, gradients)
# measured (round 3): fp32 2.0e-7 / 1.7e-5 / 6.6e-5, fp16 2.2e-5 / 1.2e-3 / 4.2e-3, bf16 7.4e-5 / 9.5e-3 / 3.0e-2
ENC_TOL = {"fp32": (2e-6, 4e-5, 2e-4), "fp16": (5e-5, 2e-3, 8e-3), "bf16": (2e-4, 1.5e-2, 4.5e-2)}
# The two front-end convolutions sit behind ReLUs on a few thousand positions.  A forward difference of one rounding error flips isolated
# ReLU mask bits, and each flipped bit moves an entry of a convolution's weight gradient by one full term of a ~sqrt(positions)-sized sum:
# the max-norm error of those tensors is a property of the fixture's size (T = 83..200 frames), not of the kernels (fp32 mode reproduces
# them to 1e-5 when no bit flips).  They get their own max-norm gate.
# Measured on MI355X (round 3, every reference-pinned fixture): fp32 7.4e-6 .. 5.4e-5, fp16 2.8e-2 .. 6.0e-2, bf16 7.2e-2 .. 7.9e-2.
FRONT_TOL = {"fp32": 2e-4, "fp16": 9e-2, "bf16": 1.25e-1}
# The config-4-shape case (d = 512: conv2 sums 4608 products per output, against the ORACLE, not a reference fixture) is the one where an
# fp32-mode rounding difference does flip a ReLU bit: measured 7.3e-3 max-norm at rel-L2 7.3e-4.  It keeps its own gate -- and the claim "it is
# the flips, not the kernels" is TESTED by the same case with a margin around the ReLU thresholds (`margin=True`: no pre-activation within
# 0.25 of zero), which must meet FRONT_TOL like every other case.
FRONT_TOL_CFG4_FLIPS = {"fp32": 1.2e-2, "bf16": 8e-2}
# Gradients that are ZERO in exact arithmetic: keys' bias and the batch path's positional parameters (constant along a softmax row), the
# depthwise bias (removed by BatchNorm's batch mean).  The reference holds rounding noise there (1e-8 .. 1e-5 of the largest gradient), the
# 16-bit modes somewhat more; they are checked against a 100x higher floor, i.e. as "stays negligible", not digit by digit.
STRUCT_ZERO = ("linear_k.bias", "pos_bias_v", "linear_pos.weight", "depthwise_conv.bias")


def is_front(name):
    return "conv.0." in name or "conv.2." in name


def floor_for(name, floor):
    return floor * 100.0 if name.endswith(STRUCT_ZERO) else floor


@pytest.fixture(scope="module")
def pkg():
    import cfm
    import attention
    import convolution
    import decoder
    import encoder
    import encoder_layer
    import feedforward
    assert torch.cuda.is_available()
    assert cfm.lib().cfm_device_ok() == 1, cfm.lib().cfm_last_error()

    class NS:
        pass
    ns = NS()
    ns.cfm, ns.attention, ns.convolution, ns.decoder, ns.encoder, ns.encoder_layer, ns.feedforward = (
        cfm, attention, convolution, decoder, encoder, encoder_layer, feedforward)
    yield ns
    cfm.set_precision("bf16")


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def relerr(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def pad_valid(lens, T):
    return (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).unsqueeze(1).to(DEV)


def run_case(g, tag, mod, x, call, gseed, mode, want_dx=True, ftol=None, gtol=None, skip=()):
    mod.zero_grad()
    xr = x.clone().requires_grad_(want_dx)
    out = call(mod, xr)
    G = dev(synth.normal(gseed, tuple(out.shape)))
    (out * G).sum().backward()
    ftol = MOD_TOL[mode][0] if ftol is None else ftol
    gtol = MOD_TOL[mode][1] if gtol is None else gtol
    e_out = grad_err(g, tag + ":out", out.detach().float().cpu().numpy())
    names = [k for k, p in mod.named_parameters()]
    floor = 1e-2 * max([grad_ref_max(g, tag + ":grad:" + k) for k in names] + ([grad_ref_max(g, tag + ":dx")] if want_dx else []))
    worst, worst_front = (0.0, ""), (0.0, "")
    if want_dx:
        worst = max(worst, (grad_err(g, tag + ":dx", xr.grad.float().cpu().numpy(), floor), "dx"))
    for k, p in mod.named_parameters():
        assert p.grad is not None, (tag, k)
        assert bool(torch.isfinite(p.grad).all()), (tag, k)
        if k in skip:
            continue
        e = (grad_err(g, tag + ":grad:" + k, p.grad.float().cpu().numpy(), floor_for(k, floor)), k)
        if is_front(k):
            worst_front = max(worst_front, e)
        else:
            worst = max(worst, e)
    print("  [%s] %-18s out %.3e   worst gradient %.3e (%s)   front-end convs %.3e (%s)" % (mode, tag, e_out, worst[0], worst[1], worst_front[0], worst_front[1]))
    assert e_out < ftol, (tag, mode, e_out)
    assert worst[0] < gtol, (tag, mode, worst)
    assert worst_front[0] < FRONT_TOL[mode], (tag, mode, worst_front)
    return out


@pytest.mark.parametrize("mode", MODES)
def test_module_gradients_match_reference(pkg, mode):
    g, meta = load_golden("train_mods_d144")
    D, H, FF, K, B, T = (meta[k] for k in ("D", "H", "FF", "K", "B", "T"))
    pkg.cfm.set_precision(mode)
    pad = pad_valid(meta["lens"], T)
    from oracle import conformer_oracle as O
    chunk_all = torch.from_numpy(O.chunk_mask(T, 5, 1)).to(DEV).unsqueeze(0).expand(B, T, T).contiguous()
    chunk_pad = chunk_all & pad
    rpe = pkg.attention.RelativePositionalEncoding(D, 0.0)
    pos_b = rpe.pe[0:B].to(DEV)

    x = dev(synth.normal(41, (B, T, D)))
    m = synth.load_synth_(pkg.feedforward.PositionwiseFeedForwardModule(D, 0.0, FF), 31).to(DEV).train()
    run_case(g, "ffn", m, x, lambda mod, xr: mod(xr), 61, mode)

    x = dev(synth.normal(42, (B, T, D)))
    m = synth.load_synth_(pkg.attention.RelativeMultiHeadSelfAttentionModule(D, H, 0.0), 32).to(DEV).train()
    run_case(g, "relmhsa_pad", m, x, lambda mod, xr: mod(xr, xr, xr, pad, pos_b)[0], 62, mode)
    run_case(g, "relmhsa_chunk", m, x, lambda mod, xr: mod(xr, xr, xr, chunk_all, pos_b)[0], 63, mode)
    run_case(g, "relmhsa_chunkpad", m, x, lambda mod, xr: mod(xr, xr, xr, chunk_pad, pos_b)[0], 64, mode)      # fully masked rows
    m = synth.load_synth_(pkg.attention.MultiHeadSelfAttentionModule(D, H, 0.0), 36).to(DEV).train()
    run_case(g, "mhsa_pad", m, x, lambda mod, xr: mod(xr, xr, xr, pad)[0], 65, mode)

    x = dev(synth.normal(43, (B, T, D)))
    m = synth.load_synth_(pkg.convolution.ConvolutionModule(D, K, FF), 33).to(DEV).train()
    run_case(g, "conv_pad", m, x, lambda mod, xr: mod(xr, pad)[0], 66, mode)
    rtol = 1e-5 if mode == "fp32" else 2e-2
    assert np.abs(m.norm.running_mean.cpu().numpy() - g["conv_pad:running_mean"]).max() < rtol
    assert np.abs(m.norm.running_var.cpu().numpy() - g["conv_pad:running_var"]).max() < rtol
    assert int(m.norm.num_batches_tracked) == int(g["conv_pad:num_batches_tracked"][0]) == 1

    xf = dev(synth.fbank(44, 3, 83))
    padf = pad_valid(meta["sub_lens"], 83)
    m = synth.load_synth_(pkg.convolution.ConvolutionSubSampling(80, D, pkg.attention.RelativePositionalEncoding(D, 0.0)), 34).to(DEV).train()
    run_case(g, "sub", m, xf, lambda mod, xr: mod(xr, padf)[0], 67, mode, want_dx=False)

    x = dev(synth.normal(45, (B, T, D)))
    m = synth.load_synth_(pkg.encoder_layer.ConformerEncoderLayer(D, K, 0.0, 0.0, FF, H, True), 35).to(DEV).train()
    run_case(g, "layer", m, x, lambda mod, xr: mod(xr, pad, pos_b, pad)[0], 68, mode)
    m = synth.load_synth_(pkg.encoder_layer.ConformerEncoderLayer(D, K, 0.0, 0.0, FF, H, False), 37).to(DEV).train()
    run_case(g, "layer_norel", m, x, lambda mod, xr: mod(xr, pad, None, pad)[0], 69, mode)


def build_train_case(pkg, name, mode):
    g, meta = load_golden(name)
    cfg = meta["cfg"]
    pkg.cfm.set_precision(mode)
    enc = pkg.encoder.ConformerEncoder(cmvn=None, **dict(cfg, **meta["ctor"]))
    synth.load_synth_(enc, meta["wseed"])
    dec = synth.load_synth_(pkg.decoder.CTCDecoder(meta["V"], cfg["encoder_dim"], 0.0), meta["cseed"])
    enc, dec = enc.to(DEV).train(), dec.to(DEV).train()
    x = dev(synth.fbank(meta["xseed"], meta["batch"], meta["frames"]))
    lens = torch.tensor(meta["lens"], dtype=torch.int32, device=DEV)
    return g, meta, enc, dec, x, lens


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["train_cfg1", "train_cfg1_chunk", "train_cfg2s"])
def test_encoder_ctc_training_step_matches_reference(pkg, name, mode):
    """BASELINE config 3's step at golden size: encoder (train mode) + CTC loss + backward; loss, every parameter gradient and the
    BatchNorm running statistics against the reference's."""
    g, meta, enc, dec, x, lens = build_train_case(pkg, name, mode)
    y, m = enc(x, lens, **meta["fw"])
    enc_lens = m.squeeze(1).sum(1)
    assert np.array_equal(enc_lens.cpu().numpy(), g["enc_lens"])
    loss = dec(y, enc_lens, dev(g["labels"]), dev(g["label_lens"]))
    loss.backward()
    tl, ty, tg = ENC_TOL[mode]
    e_loss = abs(float(loss) - float(g["loss"][0])) / abs(float(g["loss"][0]))
    e_y = grad_err(g, "y", y.detach().float().cpu().numpy())
    named = [("enc." + k, p) for k, p in enc.named_parameters()] + [("ctc." + k, p) for k, p in dec.named_parameters()]
    floor = 1e-3 * max(grad_ref_max(g, "grad:" + k) for k, _ in named)
    errs = []
    for k, p in named:
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
        errs.append((grad_err(g, "grad:" + k, p.grad.float().cpu().numpy(), floor_for(k, floor)), k))
    worst = max(e for e in errs if not is_front(e[1]))
    worst_front = max(e for e in errs if is_front(e[1]))
    med = float(np.median([e for e, _ in errs]))
    print("  [%s] %-16s loss %.3e   y %.3e   gradients: worst %.3e (%s), median %.3e, front-end convs %.3e (%s)" % (
        mode, name, e_loss, e_y, worst[0], worst[1], med, worst_front[0], worst_front[1]))
    assert e_loss < tl and e_y < ty, (e_loss, e_y)
    assert worst[0] < tg, worst
    assert worst_front[0] < FRONT_TOL[mode], worst_front
    rtol = 1e-5 if mode == "fp32" else 3e-2
    for k, v in enc.state_dict().items():
        if k.endswith("running_mean") or k.endswith("running_var"):
            assert np.abs(v.cpu().numpy() - g["bn:" + k]).max() < rtol, k
        if k.endswith("num_batches_tracked"):
            assert int(v) == 1


WINDOW_TOL = {"fp32": 3e-6, "fp16": 3e-6, "bf16": 3e-6}     # measured: outputs bit-identical, gradients <= 6e-7 (the order of f32 sums) in every mode


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,window_head", [("train_cfg1", False), ("train_cfg1_chunk", False), ("train_cfg1", True)])
def test_accumulation_window_equals_sequential_micro_batches(pkg, name, mode, window_head):
    """ConformerEncoder.forward_window: two micro-batches of DIFFERENT shapes in one pass (rows concatenated, attention / depthwise /
    BatchNorm per micro-batch) against the reference's procedure -- forward + backward per micro-batch, gradients accumulated
    (train.sh:36 accum_grad 2): losses, every accumulated gradient, BatchNorm running statistics (two momentum updates, in order) and
    batch counters.  The weights do not change inside a window, so the two are the same computation up to the order of f32 sums."""
    g, meta, enc, dec, x, lens = build_train_case(pkg, name, mode)
    V = meta["V"]
    x2 = dev(synth.fbank(meta["xseed"] + 5, 3, 131))
    lens2 = torch.tensor([131, 100, 64], dtype=torch.int32, device=DEV)
    rs = np.random.RandomState(5)
    lab1, ll1 = dev(g["labels"]), dev(g["label_lens"])
    ll2 = np.array([4, 3, 2])
    lab2 = np.zeros((3, 4), dtype=np.int64)
    for b in range(3):
        lab2[b, :ll2[b]] = rs.randint(1, V, size=ll2[b])
    lab2, ll2 = dev(lab2), dev(ll2)
    fw = meta["fw"]
    if "decoding_chunk_size" in fw and fw["decoding_chunk_size"] == 0:
        fw = dict(fw, decoding_chunk_size=3)                 # the dynamic-chunk case draws its width from the host RNG: pin it for both runs
    state0 = {k: v.clone() for k, v in enc.state_dict().items()}

    def run(window):
        enc.load_state_dict(state0)
        enc.zero_grad(), dec.zero_grad()
        if window and window_head:                           # the CTC heads of the window in ONE vocabulary projection (CTCDecoder.forward_window)
            rows, ((y1, m1), (y2, m2)) = enc.forward_window([(x, lens), (x2, lens2)], return_rows=True, **fw)
            l1, l2 = dec.forward_window(rows, [(y1.size(0), y1.size(1), m1.squeeze(1).sum(1), lab1, ll1), (y2.size(0), y2.size(1), m2.squeeze(1).sum(1), lab2, ll2)]).unbind(0)
            ((l1 + l2) / 2).backward()
        elif window:
            (y1, m1), (y2, m2) = enc.forward_window([(x, lens), (x2, lens2)], **fw)
            l1 = dec(y1, m1.squeeze(1).sum(1), lab1, ll1)
            l2 = dec(y2, m2.squeeze(1).sum(1), lab2, ll2)
            ((l1 + l2) / 2).backward()
        else:
            y1, m1 = enc(x, lens, **fw)
            l1 = dec(y1, m1.squeeze(1).sum(1), lab1, ll1)
            (l1 / 2).backward()
            y2, m2 = enc(x2, lens2, **fw)
            l2 = dec(y2, m2.squeeze(1).sum(1), lab2, ll2)
            (l2 / 2).backward()
        grads = {k: p.grad.clone() for k, p in list(enc.named_parameters()) + [("ctc." + k, p) for k, p in dec.named_parameters()]}
        bufs = {k: v.clone() for k, v in enc.state_dict().items() if "running" in k or "tracked" in k}
        return float(l1), float(l2), y1.detach().clone(), y2.detach().clone(), grads, bufs

    a, b = run(False), run(True)
    tol = WINDOW_TOL[mode]
    assert abs(a[0] - b[0]) <= tol * abs(a[0]) and abs(a[1] - b[1]) <= tol * abs(a[1]), (a[:2], b[:2])
    e_y = max(relerr(b[2], a[2]), relerr(b[3], a[3]))
    gmax = max(float(v.abs().max()) for v in a[4].values())
    worst = max((float((b[4][k] - v).abs().max()) / max(float(v.abs().max()), floor_for(k, 1e-3 * gmax)), k) for k, v in a[4].items())
    for k, v in a[5].items():
        if "tracked" in k:
            assert int(b[5][k]) == int(v) == int(state0[k]) + 2, k
        else:
            assert float((b[5][k] - v).abs().max()) <= max(tol, 1e-6) * max(1.0, float(v.abs().max())), k
    print("  [%s] %s window of 2 micro-batches%s vs sequential accumulation: outputs %.3e, worst gradient %.3e (%s)" % (
        mode, name, " + window CTC head" if window_head else "", e_y, worst[0], worst[1]))
    assert e_y < tol and worst[0] < tol * (6 if is_front(worst[1]) else 1), (e_y, worst)


def test_training_step_is_deterministic_and_accumulates(pkg):
    """two identical steps give bitwise-identical gradients when the weight-gradient GEMMs run unsplit ... here: accumulation semantics --
    a second backward ADDS into .grad (gradient accumulation, train.sh:36 accum_grad 2)."""
    g, meta, enc, dec, x, lens = build_train_case(pkg, "train_cfg1", "fp32")
    def step():
        y, m = enc(x, lens)
        dec(y, m.squeeze(1).sum(1), dev(g["labels"]), dev(g["label_lens"])).backward()
    step()
    g1 = {k: p.grad.clone() for k, p in enc.named_parameters()}
    step()
    gmax = max(float(v.abs().max()) for v in g1.values())
    for k, p in enc.named_parameters():
        a, b = p.grad, 2 * g1[k]                                        # BatchNorm running stats moved, the forward did not (batch statistics)
        assert float((a - b).abs().max()) <= 2e-4 * max(float(b.abs().max()), 1e-3 * gmax), k


def relu_margin_(enc, x, want=0.25):
    """Rewrite the front-end's convolution BIASES so that no ReLU pre-activation of this input lies within max(want, 5 % of the largest
    pre-activation) of zero: +-(1.05 S + want) alternating per channel, S = the largest |w * input| of that convolution -- half the channels
    always on, half always off (the backward's ReLU gating is exercised, not bypassed), the taps and the signal's variation untouched.
    Returns (measured margin) / (required margin) (plain torch CPU convolutions)."""
    import torch.nn.functional as F
    with torch.no_grad():
        c0, c2 = enc.embed.conv[0], enc.embed.conv[2]
        sign = torch.tensor([1.0, -1.0]).repeat(c0.bias.numel() // 2)
        s1 = float(F.conv2d(torch.from_numpy(x).unsqueeze(1), c0.weight, None, stride=2).abs().max())
        c0.bias.copy_((1.05 * s1 + want) * sign)
        z1 = F.conv2d(torch.from_numpy(x).unsqueeze(1), c0.weight, c0.bias, stride=2)
        a1 = torch.relu(z1)
        s2 = float(F.conv2d(a1, c2.weight, None, stride=2).abs().max())
        c2.bias.copy_((1.05 * s2 + want) * sign)
        z2 = F.conv2d(a1, c2.weight, c2.bias, stride=2)
    return min(float(z1.abs().min()) / (0.05 * s1 + want), float(z2.abs().min()) / (0.05 * s2 + want))


# (the margin variant is an f32 question -- do the front-end gradients meet the ordinary gate when no ReLU bit can flip? -- and its large biases are a
# common offset of ~20x the signal's variation on the front-end's output: ill-conditioned for 8-bit mantissas, so no bf16 case)
@pytest.mark.parametrize("mode,margin", [("fp32", False), ("bf16", False), ("fp32", True)])
def test_config4_shape_gradients_against_oracle(pkg, mode, margin):
    """d = 512, h = 8, ff = 2048 (BASELINE config 4's encoder shape), 2 layers, ragged batch: gradients against the CPU oracle under
    torch.autograd (the goldens stop at d = 256).  margin: the front-end's parameters leave >= 0.25 around every ReLU threshold, so no
    rounding difference can flip a mask bit (>= 5 % of the largest pre-activation) -- the front-end convolutions' gradients must then meet the ordinary gate."""
    from oracle import conformer_oracle as O
    from test_oracle_golden import encoder_shapes
    cfg = dict(input_dim=80, kernel_size=15, encoder_dim=512, dropout=0.0, attention_dropout=0.0, pos_enc_dropout=0.0, hidden_dim=2048, num_heads=8,
               encoder_num_layers=2, max_len=5000, use_relative=True)
    B, T, V, Umax = 3, 160, 300, 6
    lens = [160, 131, 90]
    pkg.cfm.set_precision(mode)
    enc = synth.load_synth_(pkg.encoder.ConformerEncoder(cmvn=None, **cfg), 71)
    dec = synth.load_synth_(pkg.decoder.CTCDecoder(V, 512, 0.0), 72)
    x = synth.fbank(73, B, T)
    if margin:
        got = relu_margin_(enc, x)
        assert got >= 0.999, got
    rs = np.random.RandomState(74)
    labels = rs.randint(1, V, size=(B, Umax))
    label_lens = np.array([6, 4, 3])
    for b in range(B):
        labels[b, label_lens[b]:] = 0
    # oracle (CPU, f32, autograd)
    P = {k: v.detach().clone().requires_grad_(v.dtype == torch.float32 and "running" not in k) for k, v in enc.state_dict().items()}
    Pc = {k: v.detach().clone().requires_grad_(True) for k, v in dec.state_dict().items()}
    y_o, m_o = O.encoder_forward(P, O.Config(**cfg), torch.from_numpy(x), lens, train=True)
    el = m_o.squeeze(1).sum(1).numpy()
    loss_o = O.ctc_head_loss_autograd(Pc, "", y_o, el, labels, label_lens)
    loss_o.backward()
    # device
    enc, dec = enc.to(DEV).train(), dec.to(DEV).train()
    y, m = enc(dev(x), torch.tensor(lens, dtype=torch.int32, device=DEV))
    loss = dec(y, m.squeeze(1).sum(1), dev(labels), dev(label_lens))
    loss.backward()
    tl, ty, tg = ENC_TOL[mode]
    assert abs(float(loss) - float(loss_o)) / abs(float(loss_o)) < tl
    gmax = max(float(P[k].grad.abs().max()) for k, _ in enc.named_parameters())
    worst, worst_front, worst_l2 = (0.0, ""), (0.0, ""), (0.0, "")
    for k, p in list(enc.named_parameters()) + [("ctc." + k, p) for k, p in dec.named_parameters()]:
        ref = (Pc[k[4:]] if k.startswith("ctc.") else P[k]).grad.double()
        d = p.grad.cpu().double() - ref
        e = (float(d.abs().max()) / max(float(ref.abs().max()), floor_for(k, 1e-3 * gmax)), k)
        l2 = (float(d.norm()) / max(float(ref.norm()), 1e-3 * gmax * ref.numel() ** 0.5), k)
        worst_l2 = max(worst_l2, l2)
        if is_front(k):
            worst_front = max(worst_front, e)
        else:
            worst = max(worst, e)
    print("  [%s] config-4 shape%s: loss %.5f vs %.5f, worst gradient %.3e (%s), front-end convs %.3e (%s), worst rel-L2 %.3e (%s)" % (
        mode, " (ReLU margin)" if margin else "", float(loss), float(loss_o), worst[0], worst[1], worst_front[0], worst_front[1], worst_l2[0], worst_l2[1]))
    assert worst[0] < tg, worst
    assert worst_front[0] < (FRONT_TOL if margin else FRONT_TOL_CFG4_FLIPS)[mode], worst_front
    # isolated mask flips move the L2 error far less than the max norm (measured fp32: 7.3e-4 where the max norm says 7.3e-3)
    assert worst_l2[0] < (tg if margin or mode != "fp32" else 1.5e-3), worst_l2


def test_reference_style_driver_trains_on_dropin_modules(pkg):
    """the reference's own encoder.py loop (embed -> blocks -> after_norm, encoder.py:62-74) spelled out over the drop-in modules in
    train mode gives the same loss and gradients as ConformerEncoder.forward."""
    g, meta, enc, dec, x, lens = build_train_case(pkg, "train_cfg1", "fp32")
    y, m = enc(x, lens)
    dec(y, m.squeeze(1).sum(1), dev(g["labels"]), dev(g["label_lens"])).backward()
    ref = {k: p.grad.clone() for k, p in enc.named_parameters()}
    enc.zero_grad()
    for mod in enc.modules():
        if isinstance(mod, torch.nn.BatchNorm1d):
            mod.reset_running_stats()
    pad = ~pkg.encoder.make_pad_mask(lens, x.size(1)).unsqueeze(1)
    out, pos, pad_s = enc.embed(x, pad)
    am = pkg.encoder.make_attn_mask(out, pad_s, False, False, 0, -1, -1)
    for blk in enc.encoders:
        out, am, _, _ = blk(out, am, pos, pad_s)
    out = enc.after_norm(out)           # nn.LayerNorm itself: torch's op, autograd-aware
    dec(out, pad_s.squeeze(1).sum(1), dev(g["labels"]), dev(g["label_lens"])).backward()
    gmax = max(float(v.abs().max()) for v in ref.values())
    for k, p in enc.named_parameters():
        assert float((p.grad - ref[k]).abs().max()) <= 1e-4 * max(float(ref[k].abs().max()), 1e-2 * gmax), k


@pytest.mark.parametrize("rel", [True, False])
def test_dropout_gradients_by_finite_differences(pkg, rel):
    """Train mode with ACTIVE dropout (p = 0.1 everywhere, the reference's train.sh setting).  The masks come from the kernels' counter-based
    generator, seeded from torch's CPU generator -- no bit-parity with torch's own dropout -- so the check is the derivative itself: with
    the seed re-armed before every forward the block is a fixed smooth function, and its analytic gradient (one backward) must match central
    differences along random directions, for the input and for parameters of every sub-block.  fp32 (f32-accurate) mode."""
    pkg.cfm.set_precision("fp32")
    D, H, FF, K, B, T = 144, 4, 576, 15, 2, 29
    layer = synth.load_synth_(pkg.encoder_layer.ConformerEncoderLayer(D, K, 0.1, 0.1, FF, H, rel), 35).to(DEV).train()
    pad = pad_valid([29, 21], T)
    pos_b = pkg.attention.RelativePositionalEncoding(D, 0.0).pe[0:B].to(DEV) if rel else None
    x = dev(synth.normal(45, (B, T, D)))
    G = dev(synth.normal(46, (B, T, D)))

    def loss(xv):
        torch.manual_seed(2024)                                     # same dropout masks on every call
        return float((layer(xv, pad, pos_b, pad)[0].double() * G.double()).sum())

    xr = x.clone().requires_grad_(True)
    torch.manual_seed(2024)
    out = layer(xr, pad, pos_b, pad)[0]
    (out.double() * G.double()).sum().backward()
    with torch.no_grad():
        y0 = layer.eval()(x, pad, pos_b, pad)[0]
        layer.train()
    assert float((out - y0).abs().max()) > 1e-2                      # dropout really is active
    torch.manual_seed(2024)
    assert torch.equal(layer(x, pad, pos_b, pad)[0], out.detach())   # reproducible under the same seed
    torch.manual_seed(2025)
    assert not torch.equal(layer(x, pad, pos_b, pad)[0], out.detach())
    eps = 2e-2
    v = dev(synth.normal(47, (B, T, D)))
    fd = (loss(x + eps * v) - loss(x - eps * v)) / (2 * eps)
    an = float((xr.grad.double() * v.double()).sum())
    print("  dropout 0.1, rel=%s: d/dx analytic %.5f vs central difference %.5f" % (rel, an, fd))
    assert abs(fd - an) < 2e-2 * max(abs(an), 1.0)
    for name in ("feed_forward_macaron.w_1.weight", "self_attn.linear_v.weight", "self_attn.linear_q.bias", "conv_module.pointwise_conv1.weight",
                 "conv_module.depthwise_conv.weight", "conv_module.norm.weight", "feed_forward.w_2.weight", "norm_mha.weight"):
        prm = dict(layer.named_parameters())[name]
        d = dev(synth.normal(48, tuple(prm.shape))) * float(prm.detach().abs().mean())
        an = float((prm.grad.double() * d.double()).sum())
        with torch.no_grad():
            prm.add_(eps * d)
            lp = loss(x)
            prm.sub_(2 * eps * d)
            lm = loss(x)
            prm.add_(eps * d)
        fd = (lp - lm) / (2 * eps)
        print("    %-40s analytic %.5f vs central difference %.5f" % (name, an, fd))
        assert abs(fd - an) < 3e-2 * max(abs(an), 0.5), name
    pkg.cfm.set_precision("bf16")


def strip_block_(layer, case):
    """Block forms the reference's constructors never build, made by hand: no conv-module biases (pointwise-conv-2 keeps its own), a
    BatchNorm without affine parameters, a cumulative-moving-average BatchNorm (momentum=None)."""
    cv = layer.conv_module
    if case == "conv_bias_free":
        cv.pointwise_conv1.bias = None
        cv.depthwise_conv.bias = None
    elif case == "bn_affine_free":
        cv.norm = torch.nn.BatchNorm1d(cv.norm.num_features, affine=False).to(cv.pointwise_conv2.weight.device)
    elif case == "bn_momentum_none":
        cv.norm.momentum = None
    return layer


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("rel", [True, False])
def test_composite_block_equals_op_by_op(pkg, mode, rel):
    """The block enqueued from C++ (cfm.autograd.EncoderLayerFn: csrc/train_layer.cpp, two host calls) against the op-by-op composition of
    tests/train_block_ref.py (one C-ABI call per kernel): the same launches in the same order, so with the weight-gradient products unsplit (no
    atomics) output, input gradient, every parameter gradient and the running variance are BIT-identical -- with dropout 0.1 active (same seed)
    and a ragged batch, over two steps (the second one from the cached packs and weight structs); for the reference's block and for the
    hand-made forms of strip_block_."""
    import train_block_ref
    pkg.cfm.set_precision(mode)
    pkg.cfm.set_deterministic(True)
    try:
        D, H, FF, K, B, T = 144, 4, 576, 15, 3, 37
        pad = pad_valid([37, 30, 19], T)
        pos_b = pkg.attention.RelativePositionalEncoding(D, 0.0).pe[0:B].to(DEV) if rel else None
        x = dev(synth.normal(45, (B, T, D)))
        G = dev(synth.normal(46, (B, T, D)))
        for case in ("reference", "conv_bias_free", "bn_affine_free", "bn_momentum_none"):
            layer = synth.load_synth_(pkg.encoder_layer.ConformerEncoderLayer(D, K, 0.1, 0.1, FF, H, rel), 35).to(DEV).train()
            strip_block_(layer, case)
            res = {}
            for comp in (True, False):
                layer.conv_module.norm.reset_running_stats()
                res[comp] = []
                for step in range(2):
                    layer.zero_grad()
                    xr = x.clone().requires_grad_(True)
                    torch.manual_seed(99 + step)
                    out = layer(xr, pad, pos_b, pad)[0] if comp else train_block_ref.block_train_forward(layer, xr, pad, pad)
                    (out * G).sum().backward()
                    res[comp].append((out.detach().clone(), xr.grad.clone(), {k: p.grad.clone() for k, p in layer.named_parameters()},
                                      layer.conv_module.norm.running_var.clone()))
            for got, ref in zip(res[True], res[False]):
                assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]) and torch.equal(got[3], ref[3]), case
                assert got[2].keys() == ref[2].keys(), case
                for k in got[2]:
                    assert torch.equal(got[2][k], ref[2][k]), (case, k)
    finally:
        pkg.cfm.set_deterministic(False)
        pkg.cfm.set_precision("bf16")


def test_train_mode_refuses_what_is_not_built(pkg):
    D = 144
    enc = pkg.encoder.ConformerEncoder(80, 15, D, 0.0, 0.0, 0.0, 576, 4, 1, use_relative=True).to(DEV).train()
    empty = torch.zeros((0, 0, 0, 0), device=DEV)
    with pytest.raises(NotImplementedError):
        enc.forward_chunk(torch.zeros(1, 67, 80, device=DEV), 0, 16, empty, empty)
