"""GPU: transducer.StreamingRecognizer -- encoder.StreamingBatch feeding greedy.ChunkGreedySearch -- against the composition the two halves
allowed before: StreamingBatch.step, then BatchedGreedySearch.search(..., token, state) once per chunk, from the same weights.

  8. bf16 and fp32: the encoder outputs are the same kernels on the same inputs (bit-identical, asserted); the tokens are equal up to a
     stream's first decision whose two best float64 logits are within 1e-4 (greedy_ref's rule, float64 loop chained over the chunks on
     the device's encoder output); at least 3 of the 4 streams have no such decision;
  9. config-5 shape (64 streams, chunk 16, 12-layer d=256 encoder, V = 5002 head), 8 steps: tokens come out, the step counter keeps its
     bounds, and the host read one counter per graph replay (replays == ceil(steps / steps_per_replay))."""
import numpy as np
import pytest
import torch

import greedy_ref as R
import synth
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
DELTA_SEARCH = 1e-4

CFG2 = dict(input_dim=80, kernel_size=15, encoder_dim=256, dropout=0.1, attention_dropout=0.1, pos_enc_dropout=0.1,
            hidden_dim=2048, num_heads=4, encoder_num_layers=12, max_len=5000, use_relative=True)


@pytest.fixture
def precision():
    import cfm
    before = cfm.get_precision()
    yield cfm.set_precision
    cfm.set_precision(before)


def _encoder(cfg, wseed):
    import encoder
    enc = encoder.ConformerEncoder(cmvn=None, **cfg).eval()
    synth.load_synth_(enc, wseed)
    return enc.to(DEV)


@pytest.mark.parametrize("carry", [True, False])
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_recognizer_equals_encoder_step_then_search_per_chunk(precision, mode, carry):
    import encoder
    import greedy
    import transducer
    precision(mode)
    _, meta = load_golden("enc_cfg1_stream")
    enc = _encoder(meta["cfg"], meta["wseed"])
    D = meta["cfg"]["encoder_dim"]
    V, n_steps = 73, 3
    pr, jn = R.modules(V, 48, 80, 96, 64, 2, 51, enc_dim=D, shaped=True)
    pr, jn = pr.to(DEV), jn.to(DEV)
    B, chunk, left, steps = 4, 16, 2, 5
    hop, window = 4 * chunk, (chunk - 1) * 4 + 7
    feats = torch.from_numpy(synth.fbank(195, B, window + hop * steps)).to(DEV)
    rec = transducer.StreamingRecognizer(enc, pr, jn, B, chunk, left, n_steps=n_steps, carry=carry)
    sb = encoder.StreamingBatch(enc, B, chunk, left)
    bs = greedy.BatchedGreedySearch(pr, jn, n_steps=n_steps, steps_per_replay=8, fused=True)
    P64 = R.params64(pr, jn)
    tok = st = None
    ref64 = [dict(tok=None, st=None, first=None, hyps=[]) for _ in range(B)]
    got, old = [[] for _ in range(B)], [[] for _ in range(B)]
    for s in range(steps):
        w = feats[:, s * hop: s * hop + window].contiguous()
        new = rec.step(w)
        y_new = rec.encoder_out.clone()                  # what this step's decoder read
        assert rec.encoder_stream.graph is not None
        y = sb.step(w).clone()
        assert y_new.shape == y.shape and torch.equal(y_new, y), "encoder outputs differ at step %d" % s
        ref, (tok, st) = bs.search(y.float(), [chunk] * B, token=tok if carry else None, state=st if carry else None)
        enc_proj = y.double().cpu() @ P64["j.enc_ffn.weight"].t() + P64["j.enc_ffn.bias"]
        for b in range(B):
            got[b] += new[b]
            old[b] += ref[b]
            r = ref64[b]
            if r["first"] is None:                       # the float64 loop continues from ITS state while no decision was close
                h, (t2, s2), first = R.search64(P64, enc_proj[b], chunk, 0, n_steps, DELTA_SEARCH, r["tok"] if carry else None, r["st"] if carry else None)
                if first is not None:
                    r["first"] = len(r["hyps"]) + first
                r["hyps"] += h
                r["tok"], r["st"] = t2, s2
    assert rec.hyps() == got
    clean = 0
    for b in range(B):
        first = ref64[b]["first"]
        if first is None:
            assert got[b] == old[b] == ref64[b]["hyps"], (mode, b)
            clean += 1
        else:
            assert got[b][:first] == old[b][:first], (mode, b, first)
    print("streaming recognizer [%s carry=%s]: clean streams %d of %d, tokens %s" % (mode, carry, clean, B, [len(x) for x in got]))
    assert clean >= 3 and min(len(x) for x in got) > 0
    # a stream between utterances, a padded final window, then a reset of one stream
    w = feats[:, :window].contiguous()
    before = rec.hyps()
    new = rec.step(w, [0, chunk, 5, 0])
    assert new[0] == [] and new[3] == [] and rec.hyps()[0] == before[0]
    rec.reset([2])
    assert rec.hyps()[2] == [] and rec.hyps()[1] == before[1] + new[1]
    assert rec.encoder_stream.offsets.tolist()[2] == 0 and rec.encoder_stream.offsets.tolist()[1] == (steps + 1) * chunk


def test_config5_shape_runs_with_one_host_read_per_replay(precision):
    import transducer
    precision("bf16")
    enc = _encoder(CFG2, 12)
    pr, jn = R.modules(5002, 256, 256, 512, 512, 2, 53, enc_dim=256, shaped=True)
    pr, jn = pr.to(DEV), jn.to(DEV)
    B, chunk, left, steps = 64, 16, 4, 8
    hop, window = 4 * chunk, (chunk - 1) * 4 + 7
    feats = torch.from_numpy(synth.fbank(96, B, window + hop * steps)).to(DEV)
    rec = transducer.StreamingRecognizer(enc, pr, jn, B, chunk, left, n_steps=4, steps_per_replay=4)
    assert rec.decoder.steps_per_replay == 4
    dec = rec.decoder
    total = 0
    for s in range(steps):
        lens = [chunk] * B if s % 3 else [chunk] * (B - 2) + [7, 0]
        new = rec.step(feats[:, s * hop: s * hop + window].contiguous(), lens)
        most = max(len(n) for n in new)
        assert all(len(n) <= lens[b] * 4 for b, n in enumerate(new))                    # n_steps symbols per frame at the most
        if s % 3 == 0:
            assert new[-1] == []                         # the idle stream
        assert most <= dec.steps <= 1 + most, (s, dec.steps, most)
        assert dec.steps < chunk + most
        assert dec.replays == max(1, -(-dec.steps // dec.steps_per_replay)), (dec.replays, dec.steps)
        total += sum(len(n) for n in new)
    print("config-5 streaming recognizer: %d tokens over %d steps, %d lookahead steps, %d replays" % (total, steps, dec.total_steps, dec.total_replays))
    assert total > 0 and [len(h) for h in rec.hyps()] == [len(h) for h in dec.hyps()] and sum(len(h) for h in rec.hyps()) == total
    assert rec.step(feats[:, :window].contiguous(), [0] * B) == [[] for _ in range(B)] and dec.steps == 0 and dec.replays == 0


@pytest.mark.parametrize("carry", [True, False])
def test_recognizer_reproduces_reference_streaming_tokens(precision, carry):
    """tests/golden/stream_asr.npz: the reference's forward_chunk / forward_step / joint driven by its streaming loops, per stream
    (tests/golden/make_golden_stream_asr.py).  Every recorded decision has a top-2 gap >= 1e-3 max|logit|, 100 x the fp32 mode's parity with
    the reference, so the comparison is exact and leaves no decision out."""
    import transducer
    g, meta = load_golden("stream_asr")
    assert float((g["gaps"] / g["logit_max"]).min()) >= 1e-3
    precision("fp32")
    enc = _encoder(meta["cfg"], meta["wseed"])
    h = meta["head"]
    pr, jn = R.modules(h["V"], h["embed"], h["hidden"], h["P"], h["J"], h["layers"], meta["hseed"], enc_dim=meta["cfg"]["encoder_dim"], shaped=True)
    with torch.no_grad():
        jn.ffn_out.bias[meta["blank"]] += meta["blank_bias"]
    pr, jn = pr.to(DEV), jn.to(DEV)
    B, chunk = meta["streams"], meta["chunk"]
    hop, window = 4 * chunk, (chunk - 1) * 4 + 7
    feats = torch.from_numpy(synth.fbank(meta["xseed"], B, window + hop * (meta["chunks"] - 1))).to(DEV)
    rec = transducer.StreamingRecognizer(enc, pr, jn, B, chunk, meta["left"], blank=meta["blank"], n_steps=meta["n_steps"], carry=carry)
    key = "carry" if carry else "nocarry"
    total = 0
    for s in range(meta["chunks"]):
        new = rec.step(feats[:, s * hop: s * hop + window].contiguous())
        for b in range(B):
            assert new[b] == g["%s_s%d_c%d" % (key, b, s)].tolist(), (key, b, s)
            total += len(new[b])
    assert total >= B * meta["chunks"]
