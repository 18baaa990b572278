"""GPU: ConformerEncoder.forward_utterances and transducer.OfflineRecognizer -- a ragged batch of whole utterances with the DECODING path's
semantics -- against the oracle's batch-1 encoder_forward_chunk per utterance (what the reference's Transducer.greedy_search computes, model.py:202-212).

Gates are the project's own (tests/test_modules_gpu.py TOL), max|d| / max|ref| over the valid rows; rows at and past out_lens[b] are exactly zero.

  1. config 1 (d = 144, 2 blocks), three precisions (+ bf16 on the fused-FFN route, whose GLU is the 16-bit cfm_gemm epilogue), lengths
     [200, 163, 47, 7, 5]: T' = 49, 40, 11, 1, 0.  Not an alias of `forward`: the last 7 valid rows of item 1 differ from it by more than 1e-3
     (the oracle's two paths are checked to differ that much on this input first);
  2. d = 256, ff = 2048, 3 blocks (first / middle / last, after_norm fused), B = 5, T = 302 (T'max = 74), T' = 74, 71, 33, 8, 1: no padding at
     all, an end inside a 4-row depthwise group (row 145 of the flattened rows), 33 = one row past a 32-row tile, an end within the 7-row halo of
     the tile boundary at row 224, a single frame.  Once per route among CHAIN, CHAIN_NEXT, CHAIN_NEXT_CIN and FFSPLIT in bf16 (the route read from
     the kernel table); fp32 takes the GENERAL route whatever the switches say and is run under each of them too;
  3. d = 512, h = 8, 2 blocks, B = 3, T' = 62, 40, 9: CFM_ROUTE_PAIR in bf16 (GENERAL in fp32);
  4. padding independence on case 2's batch: input frames t >= len_b overwritten with 50 N(0,1), valid output rows bit-identical;
  5. equal lengths, B = 4 at config 1: against forward_chunk at B = 4 (1e-6 in fp32, TOL in bf16);
  6. tokens: the reference's (tests/golden/offline_asr.npz) exactly in fp32, [] for a zero-length item appended; in bf16 on a synthetic 8-utterance
     ragged batch equal to greedy_ref.search64 on the device's own encoder output up to the first decision within 1e-4, at least 6 of 8 without one;
  7. audio: recognize_audio equals recognize on KaldiFbank's features, encoder_out bit-identical."""
import contextlib

import numpy as np
import pytest
import torch

import greedy_ref as R
import synth
from conftest import load_golden
from oracle import conformer_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
TOL = {"fp32": 5e-5, "fp16": 1e-3, "bf16": 1.2e-2}          # tests/test_modules_gpu.py
DELTA_SEARCH = 1e-4

CFG1 = dict(input_dim=80, kernel_size=15, encoder_dim=144, dropout=0.1, attention_dropout=0.1, pos_enc_dropout=0.1,
            hidden_dim=576, num_heads=4, encoder_num_layers=2, max_len=5000, use_relative=True)
CFG256 = CFG1 | dict(encoder_dim=256, hidden_dim=2048, encoder_num_layers=3)
CFG512 = CFG1 | dict(encoder_dim=512, hidden_dim=2048, num_heads=8, encoder_num_layers=2)
CASES = {   # name: (cfg, weight seed, input seed, T, lengths)
    "cfg1": (CFG1, 11, 21, 200, [200, 163, 47, 7, 5]),                   # T' = 49, 40, 11, 1, 0
    "d256": (CFG256, 61, 62, 302, [302, 288, 137, 36, 9]),               # T' = 74, 71, 33, 8, 1
    "d512": (CFG512, 63, 64, 251, [251, 165, 40]),                       # T' = 62, 40, 9
    "equal": (CFG1, 11, 23, 131, [131, 131, 131, 131]),                  # T' = 32
}
CHAIN_ONLY_PACKS = ("ffm_w2n", "ff_w2n", "qkv_wf", "out_wf", "pw1_wf", "pw2_wf")       # the chain packs cfm_ffn_fused does not read
_refs = {}


@pytest.fixture
def precision():
    import cfm
    before = cfm.get_precision()
    yield cfm.set_precision
    cfm.set_precision(before)


def build(cfg, wseed):
    import encoder
    enc = encoder.ConformerEncoder(cmvn=None, **cfg).eval()
    synth.load_synth_(enc, wseed)
    return enc


def reference(name):
    """The case's inputs and the oracle's batch-1 forward_chunk per utterance, computed once: (x (B,T,F) CPU, lens, [y_b (T'_b, D) float64])."""
    if name not in _refs:
        cfg, wseed, xseed, T, lens = CASES[name]
        enc = build(cfg, wseed)
        P = {k: v.clone() for k, v in enc.state_dict().items()}
        x = torch.from_numpy(synth.fbank(xseed, len(lens), T))
        ys = []
        with torch.no_grad():
            for b, n in enumerate(lens):
                if n < 7:
                    ys.append(torch.zeros((0, cfg["encoder_dim"]), dtype=torch.float64))
                else:
                    ys.append(O.encoder_forward_chunk(P, O.Config(**cfg), x[b:b + 1, :n], 0, -1, None)[0][0].double())
        _refs[name] = (x, lens, ys, P)
    return _refs[name]


def run(enc, x, lens):
    with torch.no_grad():
        y, out_lens = enc.forward_utterances(x.to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    return y, out_lens


def run_profiled(enc, x, lens):
    import cfm
    cfm.prof_reset(); cfm.prof_enable(True)
    try:
        y, out_lens = run(enc, x, lens)
    finally:
        cfm.prof_enable(False)
    names = set(cfm.prof_table().keys())
    cfm.prof_reset()
    return y, out_lens, names


def check_against_oracle(what, y, out_lens, ys, mode, frames, lens):
    """out_lens exact, padding rows exactly zero, valid rows within TOL[mode] of the oracle per utterance.  Returns the largest error."""
    want = [r.shape[0] for r in ys]
    assert out_lens.dtype == torch.int32 and out_lens.tolist() == want == [O.subsampled_len(n) if n >= 7 else 0 for n in lens], (out_lens.tolist(), want)
    assert y.shape == (len(ys), O.subsampled_len(frames), ys[0].shape[1]) and torch.isfinite(y).all()
    yc, worst = y.double().cpu(), 0.0
    for b, r in enumerate(ys):
        n = r.shape[0]
        assert not yc[b, n:].any(), "%s: item %d has non-zero rows past its %d frames" % (what, b, n)
        if n:
            e = float((yc[b, :n] - r).abs().max() / r.abs().max())
            print("  [%s] %s item %d (T' = %d) max|d|/max|ref| = %.3e" % (mode, what, b, n, e))
            assert np.isfinite(e) and e < TOL[mode], (what, mode, b, e)
            worst = max(worst, e)
    return worst


def starts(names, prefix):
    return any(n.startswith(prefix) for n in names)


# ---------------------------------------------------------------------------------------------- 1. config 1
@pytest.mark.parametrize("mode", ["bf16", "fp16", "fp32", "bf16-fused-ffn"])
def test_config1_ragged_batch_against_oracle_and_not_an_alias_of_forward(precision, mode):
    import cfm
    fused = mode.endswith("fused-ffn")
    mode = mode.split("-")[0]
    precision(mode)
    x, lens, ys, P = reference("cfg1")
    cfg = CASES["cfg1"][0]
    enc = build(cfg, CASES["cfg1"][1]).to(DEV)
    if fused:                                          # withhold the chain packs: each feed-forward one launch, the conv module's products through cfm_gemm
        run(enc, x, lens)
        for blk in enc.encoders:
            w = blk._weights(cfm.resolve_precision(blk))
            for f in CHAIN_ONLY_PACKS:
                setattr(w, f, None)
    y, out_lens, names = run_profiled(enc, x, lens)
    if mode == "fp32":
        assert starts(names, "gemm_bf16x3") and not starts(names, "chain_"), sorted(names)
    elif fused:
        assert starts(names, "ffn_fused") and starts(names, "dwconv") and not starts(names, "chain_"), sorted(names)
    else:
        assert starts(names, "chain_convin_%s_d144" % ("bf16" if mode == "bf16" else "f16")), sorted(names)
    check_against_oracle("config 1", y, out_lens, ys, mode, x.size(1), lens)
    # not `forward` with another mask: item 1's last 7 valid frames see GLU(bias) from its padded frames there (depthwise halo), and a degenerate positional term
    with torch.no_grad():
        y_fwd_ref, _ = O.encoder_forward(P, O.Config(**cfg), x, lens)
        y_fwd, _ = enc(x.to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV))
    n1 = ys[1].shape[0]
    ref_tail = ys[1][n1 - 7:]
    d_oracle = float((y_fwd_ref[1, n1 - 7:n1].double() - ref_tail).abs().max() / ref_tail.abs().max())
    assert d_oracle > 1e-3, "the oracle's two paths agree on this input (%.2e): the alias check would prove nothing" % d_oracle
    d_dev = float((y_fwd[1, n1 - 7:n1].double().cpu() - y[1, n1 - 7:n1].double().cpu()).abs().max() / ref_tail.abs().max())
    print("  [%s] forward vs forward_utterances, last 7 valid rows of item 1: oracle %.3e, device %.3e" % (mode, d_oracle, d_dev))
    assert d_dev > 1e-3


# ---------------------------------------------------------------------------------------------- 2. d = 256, every row-chain route
ROUTES = ["CHAIN", "CHAIN_NEXT", "CHAIN_NEXT_CIN", "FFSPLIT"]


@contextlib.contextmanager
def route_switches(enc, route):
    """The switches the route tests of tests/test_modules_gpu.py use."""
    import cfm
    import encoder_layer
    prev = cfm.lib().cfm_set_cin_merge(0 if route == "CHAIN_NEXT" else 1)
    encoder_layer.CHAIN_BLOCKS = route != "CHAIN"
    enc.split_small_batches = route == "FFSPLIT"
    try:
        yield
    finally:
        cfm.lib().cfm_set_cin_merge(prev)
        encoder_layer.CHAIN_BLOCKS = True
        enc.split_small_batches = False


def assert_route(names, route, mode):
    if mode == "fp32":                                 # no row chains in the split-precision mode: CFM_ROUTE_GENERAL whatever the switches say
        assert starts(names, "gemm_bf16x3") and not starts(names, "chain_") and not starts(names, "ffnsplit_"), sorted(names)
    elif route == "CHAIN":
        assert starts(names, "chain_convin_bf16_d256") and starts(names, "chain_dwfinal_bf16_d256"), sorted(names)
        assert not starts(names, "chain_dwfinal_macaron") and not starts(names, "chain_convin_dwfinal") and not starts(names, "ffnsplit_"), sorted(names)
    elif route == "CHAIN_NEXT":
        assert starts(names, "chain_dwfinal_macaron") and starts(names, "chain_convin_bf16_d256") and not starts(names, "chain_convin_dwfinal"), sorted(names)
    elif route == "CHAIN_NEXT_CIN":
        assert starts(names, "chain_convin_dwfinal_macaron") and not starts(names, "ffnsplit_"), sorted(names)
    elif route == "FFSPLIT":
        assert starts(names, "ffnsplit_ffn") and starts(names, "chain_dwhead") and starts(names, "chain_convin_bf16_d256"), sorted(names)
        assert not starts(names, "chain_dwfinal"), sorted(names)


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("route", ROUTES)
def test_d256_utterance_ends_on_every_route(precision, route, mode):
    precision(mode)
    x, lens, ys, _ = reference("d256")
    enc = build(*CASES["d256"][:2]).to(DEV)
    with route_switches(enc, route):
        y, out_lens, names = run_profiled(enc, x, lens)
    assert_route(names, route, mode)
    check_against_oracle("d256 %s" % route, y, out_lens, ys, mode, x.size(1), lens)


# ---------------------------------------------------------------------------------------------- 3. d = 512: the pair route
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_d512_pair_route(precision, mode):
    precision(mode)
    x, lens, ys, _ = reference("d512")
    enc = build(*CASES["d512"][:2]).to(DEV)
    y, out_lens, names = run_profiled(enc, x, lens)
    if mode == "bf16":
        assert starts(names, "chain_convin_pair_bf16_d512") and starts(names, "chain_macaron_half_bf16_d512") and starts(names, "chain_dwhead_pair"), sorted(names)
    else:
        assert starts(names, "gemm_bf16x3") and not starts(names, "chain_"), sorted(names)
    check_against_oracle("d512 pair", y, out_lens, ys, mode, x.size(1), lens)


# ---------------------------------------------------------------------------------------------- 4. padding independence
@pytest.mark.parametrize("route,mode", [(r, "bf16") for r in ROUTES] + [("CHAIN_NEXT_CIN", "fp32")])
def test_valid_rows_do_not_depend_on_what_the_padding_holds(precision, route, mode):
    """Finite values only: a NaN key times a zero weight is NaN in a flash kernel, and that is not promised."""
    precision(mode)
    x, lens, ys, _ = reference("d256")
    noisy = x.clone()
    noise = torch.from_numpy(synth.normal(77, tuple(x.shape), 50.0))
    for b, n in enumerate(lens):
        noisy[b, n:] = noise[b, n:]
    assert torch.isfinite(noisy).all() and not torch.equal(noisy, x)
    enc = build(*CASES["d256"][:2]).to(DEV)
    with route_switches(enc, route):
        y0, l0 = run(enc, x, lens)
        y1, l1 = run(enc, noisy, lens)
    assert torch.equal(l0, l1)
    for b, r in enumerate(ys):
        n = r.shape[0]
        assert torch.equal(y0[b, :n], y1[b, :n]), (route, mode, b, float((y0[b, :n] - y1[b, :n]).abs().max()))
    assert torch.equal(y0, y1)                         # (and the zero rows)


# ---------------------------------------------------------------------------------------------- 5. equal lengths
@pytest.mark.parametrize("mode,gate", [("fp32", 1e-6), ("bf16", TOL["bf16"])])
def test_equal_lengths_equal_forward_chunk_at_batch_4(precision, mode, gate):
    precision(mode)
    cfg, wseed, xseed, T, lens = CASES["equal"]
    enc = build(cfg, wseed).to(DEV)
    x = torch.from_numpy(synth.fbank(xseed, len(lens), T)).to(DEV)
    empty = torch.zeros((0, 0, 0, 0), device=DEV)
    y, out_lens = run(enc, x, lens)
    with torch.no_grad():
        y_chunk, _, _ = enc.forward_chunk(x, 0, -1, empty, empty)
    assert out_lens.tolist() == [y_chunk.size(1)] * len(lens) and y.shape == y_chunk.shape
    e = float((y.double() - y_chunk.double()).abs().max() / y_chunk.double().abs().max())
    print("  [%s] forward_utterances vs forward_chunk at B = 4: %.3e" % (mode, e))
    assert e <= gate


# ---------------------------------------------------------------------------------------------- 6. tokens
def head(meta, dev=True):
    h = meta["head"]
    pr, jn = R.modules(h["V"], h["embed"], h["hidden"], h["P"], h["J"], h["layers"], meta["hseed"], enc_dim=meta["cfg"]["encoder_dim"], shaped=True)
    with torch.no_grad():
        jn.ffn_out.bias[meta["blank"]] += meta["blank_bias"]
    return (pr.to(DEV), jn.to(DEV)) if dev else (pr, jn)


def test_recognizer_reproduces_the_reference_tokens(precision):
    """tests/golden/offline_asr.npz: the reference at batch 1 per utterance (tests/golden/make_golden_offline_asr.py).  Every recorded decision has a
    top-2 gap >= 1e-3 max|logit|, 100 x the fp32 mode's parity with the reference, so the comparison is exact and leaves no decision out."""
    import transducer
    g, meta = load_golden("offline_asr")
    assert float((g["gaps"] / g["logit_max"]).min()) >= 1e-3
    precision("fp32")
    enc = build(meta["cfg"], meta["wseed"]).to(DEV)
    pr, jn = head(meta)
    lens = meta["lens"] + [0]                          # a zero-length item appended
    x = torch.from_numpy(synth.fbank(meta["xseed"], len(meta["lens"]), max(meta["lens"])))
    x = torch.cat([x, x[:1]], 0).to(DEV)
    rec = transducer.OfflineRecognizer(enc, pr, jn, blank=meta["blank"], n_steps=meta["n_steps"])
    hyps = rec.recognize(x, torch.tensor(lens, dtype=torch.int32, device=DEV))
    assert rec.encoder_out_lens.tolist() == [O.subsampled_len(n) for n in meta["lens"]] + [0]
    for b in range(len(meta["lens"])):
        ref = g["enc_%d" % b].astype(np.float64)
        e = float(np.abs(rec.encoder_out[b, :ref.shape[0]].double().cpu().numpy() - ref).max() / np.abs(ref).max())
        assert e < TOL["fp32"], (b, e)
        assert hyps[b] == g["tokens_%d" % b].tolist(), b
    assert hyps[-1] == [] and len(hyps) == len(lens) and sum(len(h) for h in hyps) > 0


SYNTH8 = dict(xseed=501, T=260, lens=[260, 251, 214, 180, 133, 96, 51, 23])


def test_bf16_tokens_follow_the_float64_search_on_the_device_encoder_output(precision):
    """The streaming test's rule (tests/test_streaming_asr_gpu.py): tokens equal greedy_ref.search64 on the device's own encoder output up to an
    utterance's first decision whose two best float64 logits are within 1e-4; at least 6 of the 8 utterances have no such decision (for the float64
    loop on the oracle's encoder output -- no device involved -- all 8 are clean with this seed: checked when the seed was picked)."""
    import transducer
    _, meta = load_golden("offline_asr")
    precision("bf16")
    enc = build(meta["cfg"], meta["wseed"]).to(DEV)
    pr, jn = head(meta)
    x = torch.from_numpy(synth.fbank(SYNTH8["xseed"], len(SYNTH8["lens"]), SYNTH8["T"])).to(DEV)
    rec = transducer.OfflineRecognizer(enc, pr, jn, blank=meta["blank"], n_steps=meta["n_steps"])
    hyps = rec.recognize(x, torch.tensor(SYNTH8["lens"], dtype=torch.int32, device=DEV))
    out_lens = rec.encoder_out_lens.tolist()
    assert out_lens == [O.subsampled_len(n) for n in SYNTH8["lens"]]
    P64 = R.params64(pr, jn)
    enc_proj = rec.encoder_out.double().cpu() @ P64["j.enc_ffn.weight"].t() + P64["j.enc_ffn.bias"]
    clean = 0
    for b, n in enumerate(out_lens):
        ref, _, first = R.search64(P64, enc_proj[b], n, meta["blank"], meta["n_steps"], DELTA_SEARCH)
        if first is None:
            assert hyps[b] == ref, (b, hyps[b], ref)
            clean += 1
        else:
            assert hyps[b][:first] == ref[:first], (b, first)
    print("offline recognizer [bf16]: clean utterances %d of %d, tokens %s" % (clean, len(out_lens), [len(h) for h in hyps]))
    assert clean >= 6 and sum(len(h) for h in hyps) > 0


# ---------------------------------------------------------------------------------------------- 7. audio
def test_recognize_audio_is_recognize_on_the_fbank_features(precision):
    import fbank
    import transducer
    _, meta = load_golden("offline_asr")
    precision("bf16")
    rs = np.random.RandomState(5)
    n = [16000, 11213, 4000]
    samples = torch.from_numpy((3000.0 * rs.standard_normal((3, max(n)))).astype(np.int16)).to(DEV)
    lens = torch.tensor(n, dtype=torch.int32, device=DEV)
    fb = fbank.KaldiFbank()

    class Stats(torch.nn.Module):                      # global CMVN from the first utterance's log-mel rows (folded into the front-end: encoder._cmvn_args):
        def __init__(self, rows):                      # the synthetic encoder is made for features ~ N(0, 1)
            super().__init__()
            self.register_buffer("mean", rows.mean(0))
            self.register_buffer("istd", 1.0 / rows.std(0))

        def forward(self, x):
            return (x - self.mean) * self.istd

    enc = build(meta["cfg"], meta["wseed"])
    enc.global_cmvn = Stats(fb(samples, lens)[0][0, :fb.num_frames(n[0])])        # (after load_synth_, which fills every state_dict entry)
    enc = enc.to(DEV)
    pr, jn = head(meta)
    rec = transducer.OfflineRecognizer(enc, pr, jn, blank=meta["blank"], n_steps=meta["n_steps"], fbank=fb)
    from_audio = rec.recognize_audio(samples, lens)
    enc_audio, lens_audio = rec.encoder_out.clone(), rec.encoder_out_lens.clone()
    feats, feat_lens = fb(samples, lens)
    from_feats = rec.recognize(feats, feat_lens)
    assert feat_lens.tolist() == [fb.num_frames(k) for k in n]
    assert lens_audio.tolist() == rec.encoder_out_lens.tolist() == [O.subsampled_len(fb.num_frames(k)) for k in n]
    assert torch.equal(enc_audio, rec.encoder_out)
    assert from_audio == from_feats and sum(len(h) for h in from_audio) > 0
    rec_default = transducer.OfflineRecognizer(enc, pr, jn, blank=meta["blank"], n_steps=meta["n_steps"])       # fbank=None: KaldiFbank's defaults
    assert rec_default.recognize_audio(samples, lens) == from_audio
