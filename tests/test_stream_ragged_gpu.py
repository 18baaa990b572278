"""GPU: per-stream window lengths of the batched streaming step -- encoder.StreamingBatch.step(frames, frame_lens) and
transducer.StreamingRecognizer.step(frames, frame_lens=...): the reference's short final chunk (model.py:145-147), per stream and at any step.

The yardstick is the CPU oracle's batch-1 encoder_forward_chunk looped per stream on the TRUNCATED windows, with the per-precision gates of the
streaming-vs-oracle tests of tests/test_modules_gpu.py (TOL[mode] * 2, restated below).  A stream whose window gives no encoder frame (fewer than 7
feature frames) is simply not stepped in the oracle: the idle step must be invisible.

Three routes: CFG1 (D 144, chunk 4 -- window 19, the 7-frame depthwise halo is longer than the chunk; the K/V ring is filled by cfm_kv_ring_write_len),
D 256 / FF 2048 at chunk 16 with 3 streams (48 rows, a 32-row tile spans two streams; the split feed-forward route, whose q|k|v launch fills the ring)
and the D 512 width of test_streaming_config4_width_against_oracle (workgroup pairs).  fp32 takes the route of separate GEMMs at every width."""
import numpy as np
import pytest
import torch

import extent
import greedy_ref as R
import synth
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
TOL = {"fp32": 5e-5, "fp16": 1e-3, "bf16": 1.2e-2}          # tests/test_modules_gpu.py TOL; the StreamingBatch-vs-oracle tests there assert < TOL * 2
MODES = ["bf16", "fp16", "fp32"]

BASE = dict(input_dim=80, kernel_size=15, dropout=0.1, attention_dropout=0.1, pos_enc_dropout=0.1, max_len=5000, use_relative=True)
CFG144 = BASE | dict(encoder_dim=144, hidden_dim=576, num_heads=4, encoder_num_layers=2)
CFG256 = BASE | dict(encoder_dim=256, hidden_dim=2048, num_heads=4, encoder_num_layers=2)
CFG512 = BASE | dict(encoder_dim=512, hidden_dim=2048, num_heads=8, encoder_num_layers=2)


def c_of(n):
    return 0 if n < 7 else ((n - 1) // 2 - 1) // 2


def all_lens(window):
    return [window, window - 1, 15, 11, 7, 6, 0]


# name -> (cfg, weight seed, chunk, left chunks, per step the window lengths; None = step(frames) without lengths)
CASES = {
    "d144": (CFG144, 11, 4, 2, [None, all_lens(19), [19, 19, 19, 19, 19, 19, 19]]),
    "d256": (CFG256, 31, 16, 2, [None, [66, 11, 0], [67, 37, 67]]),
    "d256x7": (CFG256, 31, 16, 2, [None, all_lens(67), [67] * 7]),
    "d512": (CFG512, 57, 16, 4, [None, all_lens(67), [40, 67, 67, 67, 67, 67, 67]]),
}


@pytest.fixture
def precision():
    import cfm
    before = cfm.get_precision()
    yield cfm.set_precision
    cfm.set_precision(before)


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


_ENC, _REF = {}, {}


def encoder_of(name):
    """The case's encoder (CPU master copy, built once): every test moves a deep copy to the device under its own precision."""
    import encoder
    if name not in _ENC:
        cfg, seed = CASES[name][:2]
        _ENC[name] = synth.load_synth_(encoder.ConformerEncoder(cmvn=None, **cfg).eval(), seed)
    import copy
    return copy.deepcopy(_ENC[name]).to(DEV)


def windows_of(name):
    """(feature windows per step [steps][B, window, F] on the CPU, lengths per step with None replaced by whole windows)."""
    cfg, seed, chunk, left, steps = CASES[name]
    B, window, hop = len(steps[1]), (chunk - 1) * 4 + 7, 4 * chunk
    feats = torch.from_numpy(synth.fbank(seed + 1, B, window + hop * (len(steps) - 1)))
    return [feats[:, s * hop: s * hop + window].contiguous() for s in range(len(steps))], [[window] * B if l is None else l for l in steps]


def reference(name):
    """Oracle outputs, computed once per case and shared: ref[s][b] = (c_b, D) float32, or None where the stream has no encoder frame in step s."""
    from oracle import conformer_oracle as O
    if name not in _REF:
        cfg, seed, chunk, left, _ = CASES[name]
        if name not in _ENC:
            encoder_of(name)
        P = {k: v.detach() for k, v in _ENC[name].state_dict().items()}
        ocfg = O.Config(**cfg)
        wins, lens = windows_of(name)
        B = wins[0].size(0)
        cache, off = [None] * B, [0] * B
        ref = []
        for s, w in enumerate(wins):
            row = []
            for b in range(B):
                n = lens[s][b]
                if c_of(n) == 0:
                    row.append(None)                    # the oracle stream never sees this step
                    continue
                y, cache[b] = O.encoder_forward_chunk(P, ocfg, w[b:b + 1, :n], off[b], chunk * left, cache[b])
                assert y.size(1) == c_of(n)
                off[b] += y.size(1)
                row.append(y[0])
            ref.append(row)
        _REF[name] = ref
    return _REF[name]


def poisoned(w, lens, seed):
    """The window batch with every frame at and past lens[b] replaced by 50 N(0, 1)."""
    w = w.clone()
    noise = 50.0 * torch.from_numpy(synth.normal(seed, tuple(w.shape))).to(w.dtype)
    for b, n in enumerate(lens):
        w[b, n:] = noise[b, n:]
    return w


def run_steps(sb, name, poison=None, lens_as_tensor=False):
    wins, lens = windows_of(name)
    given = CASES[name][4]
    outs = []
    with torch.no_grad():
        for s, w in enumerate(wins):
            if poison is not None:
                w = poisoned(w, lens[s], poison + s)
            fl = given[s]
            if fl is not None and lens_as_tensor:
                fl = torch.tensor(fl, dtype=torch.int32, device=DEV)
            outs.append(sb.step(w.to(DEV), fl).clone())
            if fl is not None:
                assert sb.out_lens.tolist() == [c_of(n) for n in lens[s]]
    return outs


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["d144", "d256", "d256x7", "d512"])
def test_ragged_steps_equal_the_oracle_on_truncated_windows(precision, name, mode):
    """Full windows, a ragged step (window, window-1, 15, 11, 7, 6 and 0 frames in one batch), then every stream continues without a reset."""
    import encoder
    precision(mode)
    cfg, seed, chunk, left, _ = CASES[name]
    ref = reference(name)
    enc = encoder_of(name)
    wins, lens = windows_of(name)
    B = wins[0].size(0)
    sb = encoder.StreamingBatch(enc, B, chunk, left)
    outs = run_steps(sb, name)
    worst, total = 0.0, [0] * B
    for s, y in enumerate(outs):
        for b in range(B):
            c = c_of(lens[s][b])
            total[b] += c
            assert not bool((y[b, c:] != 0).any()), "rows past c_b must be exactly zero (step %d stream %d)" % (s, b)
            assert bool(torch.isfinite(y[b]).all()), (s, b)
            if c:
                e = relerr(y[b, :c], ref[s][b])
                print("  [%s %s] step %d stream %d: n = %d, c = %d, max|d|/max|ref| = %.3e" % (name, mode, s, b, lens[s][b], c, e))
                worst = max(worst, e)
    assert sb.offsets.tolist() == total                       # every stream advanced by its own c_b
    assert worst < TOL[mode] * 2.0, worst
    # what lies behind a stream's valid frames does not exist: the same steps with 50 N(0,1) there, and the lengths as a device tensor
    sp = encoder.StreamingBatch(enc, B, chunk, left, graph=False)
    outs_p = run_steps(sp, name, poison=1000, lens_as_tensor=True)
    for s, (y, yp) in enumerate(zip(outs, outs_p)):
        assert torch.equal(y, yp), "step %d: poisoned invalid frames changed the result" % s
    assert torch.equal(sb.offsets, sp.offsets)


@pytest.mark.parametrize("name,mode,causal", [("d144", "bf16", False), ("d256", "bf16", False), ("d256", "fp32", False), ("d144", "bf16", True)])
def test_whole_window_lengths_are_the_plain_step_bit_for_bit(precision, name, mode, causal):
    import encoder
    precision(mode)
    cfg, seed, chunk, left, _ = CASES[name]
    enc = encoder_of(name)
    wins, _ = windows_of(name)
    B, window = wins[0].size(0), wins[0].size(1)
    sa = encoder.StreamingBatch(enc, B, chunk, left, causal_conv=causal)
    sl = encoder.StreamingBatch(enc, B, chunk, left, causal_conv=causal)
    with torch.no_grad():
        for s, w in enumerate(wins):
            ya = sa.step(w.to(DEV)).clone()
            yl = sl.step(w.to(DEV), [window] * B).clone()
            assert torch.equal(ya, yl), s
    assert sa.out_lens is None and sl.out_lens.tolist() == [chunk] * B
    assert torch.equal(sa.kv, sl.kv) and torch.equal(sa.offsets, sl.offsets) and torch.equal(sa.slot_mask, sl.slot_mask) and torch.equal(sa.pos_rows, sl.pos_rows)
    if causal:
        assert torch.equal(sa.conv, sl.conv)


@pytest.mark.parametrize("name,site", [("d144", "kv_ring_write_len"), ("d256x7", "ffnsplit_proj")])
def test_ring_slots_written_are_exactly_the_valid_frames(precision, name, site):
    """Both write sites: cfm_kv_ring_write_len (D 144) and the ring write fused into the split route's q|k|v launch (D 256).  The ring starts as a
    sentinel pattern inside guard bands; a ragged step changes exactly the slots (off_b + t) mod ring_T, t < c_b, of every layer, head and stream."""
    import cfm
    import encoder
    precision("bf16")
    cfg, seed, chunk, left, _ = CASES[name]
    enc = encoder_of(name)
    wins, lens = windows_of(name)
    B = wins[0].size(0)
    sb = encoder.StreamingBatch(enc, B, chunk, left, graph=False)
    g = extent.Guards(DEV)
    sentinel = 1000.0 + torch.arange(sb.kv.numel(), dtype=torch.float32).reshape(sb.kv.shape) % 977           # finite: masked slots are multiplied by zero
    sb.kv = g.io(sentinel, name="kv ring")
    sb.offsets = g.io(sb.offsets, name="offsets")
    with torch.no_grad():
        sb.step(wins[0].to(DEV))                                   # whole windows: frames 0 .. chunk-1 of every stream
        off = sb.offsets.tolist()
        assert off == [chunk] * B
        before = sb.kv.clone()
        cfm.prof_reset(); cfm.prof_enable(True)
        sb.step(poisoned(wins[1], lens[1], 7).to(DEV), lens[1])
        torch.cuda.synchronize(); cfm.prof_enable(False)
        names = set(cfm.prof_table())
        cfm.prof_reset()
    assert any(n.startswith(site) for n in names), sorted(names)
    assert ("kv_ring_write_len" in names) == (site == "kv_ring_write_len") and "kv_ring_write" not in names, sorted(names)
    g.check()
    changed = (sb.kv != before).any(dim=-1)                        # [L, B, H, ring_T]: some element of the slot's K | V row differs
    full = (sb.kv != before).all(dim=-1)
    cs = [c_of(n) for n in lens[1]]
    for b in range(B):
        want = torch.zeros(sb.ring_T, dtype=torch.bool, device=DEV)
        for t in range(cs[b]):
            want[(off[b] + t) % sb.ring_T] = True
        assert torch.equal(changed[:, b], want.expand_as(changed[:, b])), (b, cs[b], changed[:, b].nonzero().tolist())
        assert torch.equal(full[:, b], want.expand_as(full[:, b])), b          # a written slot is written whole (sentinel >= 1000, K / V are O(1))
    assert sb.offsets.tolist() == [o + c for o, c in zip(off, cs)]


def _causal_chunk(O, P, cfg, x, offset, need, attn_cache, conv_cache):
    """oracle.encoder_forward_chunk with the OPT-IN causal convolution: the oracle's own stages, conv_module(causal=True, conv_cache=...) in the
    block, as test_causal_conv_extension restates the extension.  conv_cache: list per layer of (1, K-1, D) or None.  Returns (y, attn, conv)."""
    ones = torch.ones(1, 1, x.size(1), dtype=torch.bool)
    h, _, _ = O.subsampling(P, "embed.", x, ones, cfg.pe, offset, cfg.relative)
    tc = attn_cache.size(2) if attn_cache is not None else 0
    tk = tc + h.size(1)
    pos = cfg.pe[offset - tc:offset - tc + tk].to(h.dtype).unsqueeze(1)
    new_att, new_conv = [], []
    for li in range(cfg.layers):
        p = "encoders.%d." % li
        ln = lambda nm, t: O.layer_norm(t, P[p + nm + ".weight"], P[p + nm + ".bias"])
        h = h + 0.5 * O.ffn(P, p + "feed_forward_macaron.", ln("norm_ff_macaron", h))
        a, nc = O.rel_mhsa(P, p + "self_attn.", ln("norm_mha", h), None, pos, None if attn_cache is None else attn_cache[li:li + 1], cfg.h)
        h = h + a
        co = {}
        h = h + O.conv_module(P, p + "conv_module.", ln("norm_conv", h), None, causal=True, conv_cache=None if conv_cache is None else conv_cache[li], cache_out=co)
        h = h + 0.5 * O.ffn(P, p + "feed_forward.", ln("norm_ff", h))
        h = ln("norm_final", h)
        new_att.append(nc[:, :, max(tk - need, 0):, :])
        new_conv.append(co[p + "conv_module."])
    return O.layer_norm(h, P["after_norm.weight"], P["after_norm.bias"]), torch.cat(new_att, 0), new_conv


@pytest.mark.parametrize("mode", MODES)
def test_causal_conv_with_ragged_lengths(precision, mode):
    """causal_conv=True: the conv cache becomes the last K-1 frames of [cache | x[:c_b]] and is untouched at c_b = 0."""
    import encoder
    from oracle import conformer_oracle as O
    precision(mode)
    name = "d144"
    cfg, seed, chunk, left, _ = CASES[name]
    enc = encoder_of(name)
    wins, lens = windows_of(name)
    B = wins[0].size(0)
    sb = encoder.StreamingBatch(enc, B, chunk, left, causal_conv=True)
    outs, convs = [], []
    with torch.no_grad():
        for s, w in enumerate(wins):
            outs.append(sb.step(w.to(DEV), CASES[name][4][s]).clone())
            convs.append(sb.conv.clone())
    P = {k: v.detach().cpu() for k, v in enc.state_dict().items()}
    ocfg = O.Config(**cfg)
    worst = worst_cache = 0.0
    for b in range(B):
        att = conv = None
        off = 0
        for s, w in enumerate(wins):
            n = lens[s][b]
            c = c_of(n)
            assert not bool((outs[s][b, c:] != 0).any())
            if c == 0:
                assert torch.equal(convs[s][:, b], convs[s - 1][:, b]), "the conv cache of an idle stream changed"
                continue
            y, att, conv = _causal_chunk(O, P, ocfg, w[b:b + 1, :n], off, chunk * left, att, conv)
            off += c
            worst = max(worst, relerr(outs[s][b, :c], y[0]))
            worst_cache = max(worst_cache, relerr(convs[s][:, b], torch.cat(conv, 0)))
    print("  [%s] causal conv, ragged: outputs %.3e, conv cache %.3e" % (mode, worst, worst_cache))
    assert worst < TOL[mode] * 2.0 and worst_cache < TOL[mode] * 2.0, (worst, worst_cache)
    assert sb.offsets.tolist() == [sum(c_of(l[b]) for l in lens) for b in range(B)]


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_one_graph_serves_every_length_vector(precision, mode):
    import encoder
    precision(mode)
    name = "d144"
    cfg, seed, chunk, left, _ = CASES[name]
    enc = encoder_of(name)
    B, window, hop = 7, 19, 16
    feats = torch.from_numpy(synth.fbank(77, B, window + hop * 4)).to(DEV)
    vectors = [all_lens(19), [0, 6, 7, 19, 12, 18, 9], [19] * B, [10, 0, 19, 8, 19, 6, 15], None]
    sg, se = encoder.StreamingBatch(enc, B, chunk, left, graph=True), encoder.StreamingBatch(enc, B, chunk, left, graph=False)
    graphs = []
    with torch.no_grad():
        for s, fl in enumerate(vectors):
            w = feats[:, s * hop: s * hop + window].contiguous()
            yg, ye = sg.step(w, fl).clone(), se.step(w, fl).clone()
            graphs.append(sg.graph)
            assert torch.equal(yg, ye), s
            assert torch.equal(sg.offsets, se.offsets) and torch.equal(sg.out_lens, se.out_lens), s
    assert graphs[0] is not None and all(gr is graphs[0] for gr in graphs) and se.graph is None       # captured once, replayed with four other vectors
    assert torch.equal(sg.kv, se.kv)
    # lengths given to a step captured without them: one re-capture, then that graph stays
    sn = encoder.StreamingBatch(enc, B, chunk, left, graph=True)
    with torch.no_grad():
        sn.step(feats[:, :window].contiguous())
        first = sn.graph
        sn.step(feats[:, hop:hop + window].contiguous(), vectors[0])
        second = sn.graph
        sn.step(feats[:, 2 * hop:2 * hop + window].contiguous())
    assert first is not None and second is not None and second is not first and sn.graph is second


@pytest.mark.parametrize("carry", [True, False])
def test_recognizer_reproduces_the_reference_on_short_final_chunks(precision, carry):
    """tests/golden/stream_asr_tail.npz (make_golden_stream_tail.py): 4 utterances that end on windows of 9, 37 and 66 frames and on no extra window,
    driven as model.py:145-147 drives them, here as ONE batch whose streams end at different steps and idle afterwards.  fp32; every recorded decision
    has a top-2 gap >= 1e-3 max|logit|, so the tokens are compared exactly."""
    import encoder
    import transducer
    g, meta = load_golden("stream_asr_tail")
    assert float((g["gaps"] / g["logit_max"]).min()) >= 1e-3
    precision("fp32")
    enc = synth.load_synth_(encoder.ConformerEncoder(cmvn=None, **meta["cfg"]).eval(), meta["wseed"]).to(DEV)
    h = meta["head"]
    pr, jn = R.modules(h["V"], h["embed"], h["hidden"], h["P"], h["J"], h["layers"], meta["hseed"], enc_dim=meta["cfg"]["encoder_dim"], shaped=True)
    with torch.no_grad():
        jn.ffn_out.bias[meta["blank"]] += meta["blank_bias"]
    pr, jn = pr.to(DEV), jn.to(DEV)
    lens, chunk, wins = meta["lens"], meta["chunk"], meta["windows"]
    B, hop, window = len(lens), 4 * chunk, (chunk - 1) * 4 + 7
    steps = max(len(w) for w in wins)
    feats = torch.zeros(B, hop * (steps - 1) + window, 80)
    raw = torch.from_numpy(synth.fbank(meta["xseed"], B, max(lens)))
    for b, n in enumerate(lens):
        feats[b, :n] = raw[b, :n]
        feats[b, n:] = 50.0                                        # what lies behind an utterance's end is not read
    rec = transducer.StreamingRecognizer(enc, pr, jn, B, chunk, meta["left"], blank=meta["blank"], n_steps=meta["n_steps"], carry=carry)
    key = "carry" if carry else "nocarry"
    worst, total = 0.0, 0
    for s in range(steps):
        fl = [wins[b][s][1] - wins[b][s][0] if s < len(wins[b]) else 0 for b in range(B)]
        new = rec.step(feats[:, s * hop: s * hop + window].contiguous().to(DEV), frame_lens=fl)
        for b in range(B):
            if fl[b] == 0:
                assert new[b] == [], (b, s)
                continue
            assert new[b] == g["%s_s%d_c%d" % (key, b, s)].tolist(), (key, b, s)
            want = torch.from_numpy(g["enc_s%d_c%d" % (b, s)])
            worst = max(worst, relerr(rec.encoder_out[b, :want.size(0)], want))
            total += len(new[b])
    assert {1, 8, chunk - 1} <= {c_of(w[-1][1] - w[-1][0]) for w in wins}
    assert rec.encoder_stream.offsets.tolist() == [sum(c_of(e - c) for c, e in w) for w in wins]
    print("  streaming recognizer on short final chunks [carry=%s]: %d tokens, encoder rows vs the reference %.3e" % (carry, total, worst))
    assert total > 0 and worst < TOL["fp32"] * 2.0, worst


def test_loud_failures(precision):
    import encoder
    import transducer
    precision("bf16")
    enc = encoder_of("d144")
    sb = encoder.StreamingBatch(enc, 3, 4, 2)
    w = torch.zeros(3, 19, 80, device=DEV)
    with pytest.raises(ValueError, match="frame_lens"):
        sb.step(w, [19, 19])
    with pytest.raises(ValueError, match="frame_lens"):
        sb.step(w, [19, 20, 0])
    with pytest.raises(ValueError, match="frame_lens"):
        sb.step(w, [19, -1, 0])
    with pytest.raises(ValueError, match="frame_lens"):
        sb.step(w, torch.tensor([19, 19], dtype=torch.int32, device=DEV))
    assert sb.steps == 0 and sb.offsets.tolist() == [0, 0, 0]
    pr, jn = R.modules(73, 48, 80, 96, 64, 2, 51, enc_dim=144, shaped=True)
    rec = transducer.StreamingRecognizer(enc, pr.to(DEV), jn.to(DEV), 3, 4, 2)
    with pytest.raises(ValueError, match="not both"):
        rec.step(w, lens=[4, 4, 4], frame_lens=[19, 19, 19])
    assert rec.encoder_stream.steps == 0
