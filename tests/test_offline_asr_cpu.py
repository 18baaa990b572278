"""CPU (no GPU): the offline recognizer's fixture and its host-side contract.

  * tests/golden/offline_asr.npz (the reference at batch 1 per utterance, tests/golden/make_golden_offline_asr.py): the oracle's
    encoder_forward_chunk reproduces the encoder outputs to 1e-6 and its rnnt_greedy_search the tokens; every recorded decision has a top-2
    gap >= 1e-3 max|logit|;
  * cfm_layer_io.utt_len (include/cfm.h): cfm_encoder_layer_route returns the same route with it as without, for each of the seven routes, and
    an argument error together with kv_ring, attn_cache, causal_conv or pad_valid (made-up addresses: the query dereferences nothing);
  * ConformerEncoder.forward_utterances raises on a CPU tensor, in train mode and with use_relative=False."""
import ctypes

import numpy as np
import pytest
import torch

import greedy_ref as R
import synth
import test_layer_route_cpu as LR
from conftest import load_golden
from oracle import conformer_oracle as O

PTR = LR.PTR
cfm = LR.cfm                     # the module-scoped fixture of the route tests (builds the library when it is missing)


@pytest.fixture(scope="module")
def fixture():
    return load_golden("offline_asr")


def _encoder(cfg, wseed):
    import encoder
    enc = encoder.ConformerEncoder(cmvn=None, **cfg).eval()
    synth.load_synth_(enc, wseed)
    return enc


def test_every_recorded_decision_is_clear(fixture):
    g, meta = fixture
    assert float((g["gaps"] / g["logit_max"]).min()) >= 1e-3
    assert len(g["gaps"]) == meta["decisions"]
    for b, n in enumerate(meta["lens"]):
        assert g["enc_%d" % b].shape == (O.subsampled_len(n), meta["cfg"]["encoder_dim"])
        assert len(g["tokens_%d" % b]) > 0 or g["enc_%d" % b].shape[0] <= 1


def test_oracle_forward_chunk_reproduces_the_encoder_outputs(fixture):
    g, meta = fixture
    enc = _encoder(meta["cfg"], meta["wseed"])
    P = {k: v.clone() for k, v in enc.state_dict().items()}
    cfg = O.Config(**meta["cfg"])
    x = torch.from_numpy(synth.fbank(meta["xseed"], len(meta["lens"]), max(meta["lens"])))
    for b, n in enumerate(meta["lens"]):
        y, _ = O.encoder_forward_chunk(P, cfg, x[b:b + 1, :n], 0, -1, None)
        ref = g["enc_%d" % b].astype(np.float64)
        err = float(np.abs(y[0].double().numpy() - ref).max() / np.abs(ref).max())
        print("offline_asr utterance %d (%d frames): oracle vs reference %.2e" % (b, n, err))
        assert y.shape[1:] == ref.shape and err <= 1e-6, (b, err)


def test_oracle_greedy_search_reproduces_the_tokens(fixture):
    g, meta = fixture
    h = meta["head"]
    pr, jn = R.modules(h["V"], h["embed"], h["hidden"], h["P"], h["J"], h["layers"], meta["hseed"], enc_dim=meta["cfg"]["encoder_dim"], shaped=True)
    with torch.no_grad():
        jn.ffn_out.bias[meta["blank"]] += meta["blank_bias"]
    P = {"p." + k: v.detach() for k, v in pr.state_dict().items()}
    P.update({"j." + k: v.detach() for k, v in jn.state_dict().items()})
    for b in range(len(meta["lens"])):
        enc_out = torch.from_numpy(g["enc_%d" % b])
        toks, _ = O.rnnt_greedy_search(P, "p.", "j.", enc_out, enc_out.size(0), blank=meta["blank"], n_steps=meta["n_steps"])
        assert list(toks) == g["tokens_%d" % b].tolist(), b


def _seven_routes(cfm):
    nxt = LR.weights(cfm)
    chained = lambda: LR.chained(cfm, nxt, next_x_out=3 * PTR)
    return [("GENERAL", lambda: LR.block(cfm, act_dtype=LR.F32), None),
            ("FUSED_FFN", lambda: LR.block(cfm, without=LR.NOT_FUSED_FFN_PACKS), None),
            ("CHAIN", lambda: LR.block(cfm), None),
            ("CHAIN_NEXT", chained, 0),
            ("CHAIN_NEXT_CIN", chained, 1),
            ("FFSPLIT", lambda: LR.block(cfm, psum_splits=8, M=1536), None),
            ("PAIR", lambda: LR.block(cfm, D=512, H=8, psum_splits=3, M=4096), None)]


def test_utt_len_changes_no_route(cfm):
    seen = []
    for want, make, cin in _seven_routes(cfm):
        prev = cfm.lib().cfm_set_cin_merge(cin) if cin is not None else None
        try:
            w, s, io = make()
            assert LR.route(cfm, w, s, io) == want
            io.utt_len = 7 * PTR
            assert LR.route(cfm, w, s, io) == want, want
            seen.append(want)
        finally:
            if prev is not None:
                cfm.lib().cfm_set_cin_merge(prev)
    assert sorted(seen) == sorted(cfm.ROUTES)


@pytest.mark.parametrize("kw", [dict(kv_ring=5 * PTR, stream_offset=6 * PTR, ring_T=200), dict(attn_cache=5 * PTR, cache_T=4, new_cache=6 * PTR),
                                dict(causal_conv=1), dict(pad_valid=5 * PTR)], ids=["kv_ring", "attn_cache", "causal_conv", "pad_valid"])
def test_utt_len_excludes_streaming_state_and_the_pad_mask(cfm, kw):
    w, s, io = LR.block(cfm, **kw)
    assert LR.route(cfm, w, s, io) in cfm.ROUTES                         # fine without utt_len ...
    io.utt_len = 7 * PTR
    rc, msg = LR.route(cfm, w, s, io)                                    # ... an argument error with it, before any launch
    assert rc == LR.ERR_ARG and "utt_len" in msg
    rc = cfm.lib().cfm_encoder_layer_forward(ctypes.byref(w), ctypes.byref(s), ctypes.byref(io), PTR, 2 * PTR, 0, None, None, None)
    assert rc == LR.ERR_ARG and "utt_len" in cfm.lib().cfm_last_error().decode()


def test_forward_utterances_fails_loudly(cfm):
    import encoder
    cfg = dict(input_dim=80, kernel_size=15, encoder_dim=16, dropout=0.0, attention_dropout=0.0, pos_enc_dropout=0.0, hidden_dim=32, num_heads=2,
               encoder_num_layers=1)
    x, lens = torch.zeros(2, 50, 80), torch.tensor([50, 31], dtype=torch.int32)
    enc = encoder.ConformerEncoder(use_relative=True, **cfg).eval()
    with pytest.raises(RuntimeError, match="no CPU path"):
        enc.forward_utterances(x, lens)
    with pytest.raises(NotImplementedError, match="inference-only"):
        enc.train().forward_utterances(x, lens)
    with pytest.raises(NotImplementedError, match="use_relative"):
        encoder.ConformerEncoder(use_relative=False, **cfg).eval().forward_utterances(x, lens)
    import transducer
    assert hasattr(transducer, "OfflineRecognizer")
