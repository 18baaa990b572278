"""CPU (no GPU): the ground the per-stream window lengths of the streaming step stand on.

  * tests/golden/stream_asr_tail.npz (make_golden_stream_tail.py ran the REFERENCE): its encoder outputs re-derived with the oracle's
    encoder_forward_chunk on the truncated windows, its tokens with the oracle's greedy search chunk by chunk -- this pins the fixture;
  * the window length -> encoder frames table, c = ((n - 1) // 2 - 1) // 2 and 0 below 7, against the oracle's front-end for n = 0 .. window;
  * cfm_layer_io.stream_len (include/cfm.h): accepted with a K/V ring (with and without the causal convolution) on the routes a streaming step takes,
    changing none of them; rejected without a ring, with utt_len and with pad_valid; attn_cache stays excluded by the ring itself."""
import numpy as np
import pytest
import torch

import greedy_ref as R
import synth
import test_layer_route_cpu as LR
from conftest import load_golden
from oracle import conformer_oracle as O

PTR = LR.PTR


@pytest.fixture(scope="module")
def cfm():
    import os
    import cfm as c
    if not os.path.exists(c.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return c


def c_of(n):
    return 0 if n < 7 else ((n - 1) // 2 - 1) // 2


def test_fixture_is_what_the_oracle_computes():
    g, meta = load_golden("stream_asr_tail")
    import encoder
    cfg, chunk, need = meta["cfg"], meta["chunk"], meta["chunk"] * meta["left"]
    window, hop = (chunk - 1) * 4 + 7, 4 * chunk
    enc = synth.load_synth_(encoder.ConformerEncoder(cmvn=None, **cfg).eval(), meta["wseed"])
    P = {k: v.detach() for k, v in enc.state_dict().items()}
    h = meta["head"]
    pr, jn = R.modules(h["V"], h["embed"], h["hidden"], h["P"], h["J"], h["layers"], meta["hseed"], enc_dim=cfg["encoder_dim"], shaped=True)
    with torch.no_grad():
        jn.ffn_out.bias[meta["blank"]] += meta["blank_bias"]
    H = {"p." + k: v.detach() for k, v in pr.state_dict().items()}
    H.update({"j." + k: v.detach() for k, v in jn.state_dict().items()})
    feats = torch.from_numpy(synth.fbank(meta["xseed"], len(meta["lens"]), max(meta["lens"])))
    assert float(g["gaps"].min()) > 0 and float((g["gaps"] / g["logit_max"]).min()) == pytest.approx(meta["min_gap_rel"]) and meta["min_gap_rel"] >= 1e-3
    finals = []
    for b, n in enumerate(meta["lens"]):
        wins = [(cur, min(cur + window, n)) for cur in range(0, n - 7 + 1, hop)]          # model.py:145-146
        assert [list(w) for w in wins] == meta["windows"][b]
        finals.append(c_of(wins[-1][1] - wins[-1][0]))
        cache, off = None, 0
        for s, (cur, end) in enumerate(wins):
            y, cache = O.encoder_forward_chunk(P, O.Config(**cfg), feats[b:b + 1, cur:end], off, need, cache)
            off += y.size(1)
            want = torch.from_numpy(g["enc_s%d_c%d" % (b, s)])
            assert y.size(1) == c_of(end - cur) == want.size(0)
            assert float((y[0] - want).abs().max()) < 1e-4 * float(want.abs().max())
            toks, _ = O.rnnt_greedy_search(H, "p.", "j.", want, want.size(0), blank=meta["blank"], n_steps=meta["n_steps"])      # no carry: a fresh search per chunk
            assert list(toks) == g["nocarry_s%d_c%d" % (b, s)].tolist(), (b, s)
    assert finals == [1, 8, chunk - 1, chunk] and meta["lens"][3] - meta["windows"][3][-1][1] == 2      # c = 1, a mid value, chunk-1; < 7 frames left over


def test_carry_tokens_are_one_search_over_the_concatenated_chunks():
    """The predictor state carried from chunk to chunk is one greedy search over the stream's whole encoder output (the per-frame cap restarts per frame)."""
    g, meta = load_golden("stream_asr_tail")
    h = meta["head"]
    pr, jn = R.modules(h["V"], h["embed"], h["hidden"], h["P"], h["J"], h["layers"], meta["hseed"], enc_dim=meta["cfg"]["encoder_dim"], shaped=True)
    with torch.no_grad():
        jn.ffn_out.bias[meta["blank"]] += meta["blank_bias"]
    H = {"p." + k: v.detach() for k, v in pr.state_dict().items()}
    H.update({"j." + k: v.detach() for k, v in jn.state_dict().items()})
    for b, wins in enumerate(meta["windows"]):
        enc_out = torch.cat([torch.from_numpy(g["enc_s%d_c%d" % (b, s)]) for s in range(len(wins))])
        toks, _ = O.rnnt_greedy_search(H, "p.", "j.", enc_out, enc_out.size(0), blank=meta["blank"], n_steps=meta["n_steps"])
        assert list(toks) == [t for s in range(len(wins)) for t in g["carry_s%d_c%d" % (b, s)].tolist()], b


def test_window_length_to_encoder_frames_table():
    import encoder
    cfg = dict(input_dim=80, kernel_size=15, encoder_dim=16, dropout=0.0, attention_dropout=0.0, pos_enc_dropout=0.0, hidden_dim=32, num_heads=2,
               encoder_num_layers=1, use_relative=True)
    enc = synth.load_synth_(encoder.ConformerEncoder(cmvn=None, **cfg).eval(), 3)
    P = {k: v.detach() for k, v in enc.state_dict().items()}
    ocfg = O.Config(**(cfg | dict(max_len=5000)))
    window = 67
    x = torch.from_numpy(synth.fbank(4, 1, window))
    for n in range(window + 1):
        if n < 7:
            assert c_of(n) == 0
            continue
        hsub, _, _ = O.subsampling(P, "embed.", x[:, :n], torch.ones(1, 1, n, dtype=torch.bool), ocfg.pe, 0, True)
        assert hsub.size(1) == c_of(n), n
    for chunk in (1, 4, 16):
        assert c_of((chunk - 1) * 4 + 7) == chunk


RING = dict(kv_ring=5 * PTR, stream_offset=6 * PTR, ring_T=200)


def test_stream_len_is_accepted_with_a_ring_and_changes_no_route(cfm):
    cases = [("CHAIN", dict()), ("CHAIN", dict(causal_conv=1, conv_cache=8 * PTR)), ("FFSPLIT", dict(psum_splits=8, M=48)),
             ("PAIR", dict(D=512, H=8, psum_splits=3, M=112)), ("GENERAL", dict(act_dtype=LR.F32)), ("CHAIN", dict(D=144, FF=576)),
             ("FUSED_FFN", dict(without=LR.NOT_FUSED_FFN_PACKS))]
    for want, kw in cases:
        w, s, io = LR.block(cfm, **(RING | kw))
        assert LR.route(cfm, w, s, io) == want
        io.stream_len = 7 * PTR
        assert LR.route(cfm, w, s, io) == want, (want, kw)
    nxt = LR.weights(cfm)
    w, s, io = LR.chained(cfm, nxt, next_x_out=3 * PTR, **RING)       # a step of more than 1536 rows: consecutive blocks chained over the ring
    before = LR.route(cfm, w, s, io)
    io.stream_len = 7 * PTR
    assert before in ("CHAIN_NEXT", "CHAIN_NEXT_CIN") and LR.route(cfm, w, s, io) == before


@pytest.mark.parametrize("kw,text", [(dict(), "stream_len"), (dict(attn_cache=5 * PTR, cache_T=4, new_cache=6 * PTR), "stream_len"),
                                     (RING | dict(pad_valid=7 * PTR), "stream_len"), (RING | dict(utt_len=7 * PTR), "utt_len"),
                                     (RING | dict(attn_cache=5 * PTR, cache_T=4), "excludes attn_cache")],
                         ids=["no_ring", "attn_cache", "pad_valid", "utt_len", "ring_and_attn_cache"])
def test_stream_len_is_rejected_elsewhere(cfm, kw, text):
    w, s, io = LR.block(cfm, **kw)
    io.stream_len = 9 * PTR
    rc, msg = LR.route(cfm, w, s, io)
    assert rc == LR.ERR_ARG and text in msg, msg
