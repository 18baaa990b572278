#!/usr/bin/env python
"""Generate tests/golden/stream_asr.npz by RUNNING THE REFERENCE on the CPU: streaming recognition of 3 utterances, chunk by chunk --
the reference's ConformerEncoder.forward_chunk (encoder.py:78-123), RNNPredictor.forward_step (predictor.py:76-86) and
TransducerJoint.forward (joint.py:20-38) do every step, per stream; the loops around them, Transducer.greedy_search_streaming_app
(model.py:178-199, the predictor state carried from chunk to chunk) and greedy_search_streaming_eval (:126-165, cache=None and
pred_input_step=None for every chunk) with basic_greedy_search (:215-269), are restated here because model.py does not import without
torchaudio (as tests/golden/make_golden.py gen_greedy does).

Needs the reference checkout beside the repository (the path make_golden.py uses); the fixture is data only: tokens per stream and chunk
for carry true / false, the top-2 logit gap of every decision, sizes and seeds.  Utterances are whole windows long, so no short final
chunk occurs.  Seeds are searched until EVERY recorded decision has a gap >= 1e-3 max|logit| (100 x the fp32 mode's 1e-5 parity with the
reference): the token comparison of the test is then exact with no decision left out.  The smallest gap is recorded in the metadata."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))          # tests/ -> synth
sys.path.insert(0, "/root/reference/src")          # reference flat modules

import synth  # noqa: E402

import encoder as ref_encoder  # noqa: E402
import joint as ref_joint  # noqa: E402
import predictor as ref_predictor  # noqa: E402

torch.set_num_threads(8)
CFG1 = dict(input_dim=80, kernel_size=15, encoder_dim=144, dropout=0.1, attention_dropout=0.1,
            pos_enc_dropout=0.1, hidden_dim=576, num_heads=4, encoder_num_layers=2, max_len=5000,
            use_relative=True)
STREAMS, CHUNK, LEFT, CHUNKS, N_STEPS, BLANK = 3, 16, 2, 5, 3, 0
HEAD = dict(V=73, embed=48, hidden=80, P=96, J=64, layers=2)
GAP = 1e-3
# on top of synth.greedy_joint_: the synthetic encoder's output frames differ less from one another than greedy_joint_'s N(0, 1) rows, and with
# its blank bias alone every frame emits up to the cap (no blank is ever decided); + 0.5 gives ~0.6 symbols per frame.  Recorded in the metadata.
BLANK_BIAS = 0.5


def search(pr, jn, enc, n_steps, gaps, token=None, cache=None):
    """basic_greedy_search (model.py:215-269); appends (top-2 gap, max|logit|) of every decision to gaps."""
    padding = torch.zeros(1, 1)
    tok = torch.tensor([BLANK]).reshape(1, 1) if token is None else token
    cache = pr.init_state(tok) if cache is None else cache
    t, hyps, prev, per_frame, pred_out, new_cache = 0, [], True, 0, None, None
    while t < enc.size(1):
        if prev:
            pred_out, new_cache = pr.forward_step(tok, padding, cache)
        z = jn(enc[:, t:t + 1, :], pred_out).log_softmax(dim=-1).reshape(-1)
        top = z.double().topk(2).values
        gaps.append((float(top[0] - top[1]), float(jn(enc[:, t:t + 1, :], pred_out).abs().max())))
        k = z.argmax(dim=-1).squeeze()
        if k != BLANK:
            hyps.append(int(k))
            prev = True
            per_frame += 1
            tok = k.reshape(1, 1)
            cache = new_cache
        if k == BLANK or per_frame >= n_steps:
            if k == BLANK:
                prev = False
            t += 1
            per_frame = 0
    return hyps, tok, cache


def generate(wseed, hseed, xseed):
    enc = ref_encoder.ConformerEncoder(cmvn=None, **CFG1).eval()
    synth.load_synth_(enc, wseed)
    pr = ref_predictor.RNNPredictor(HEAD["V"], HEAD["embed"], HEAD["P"], HEAD["hidden"], 0.1, HEAD["layers"]).eval()
    jn = ref_joint.TransducerJoint(HEAD["V"], CFG1["encoder_dim"], HEAD["P"], HEAD["J"]).eval()
    synth.load_synth_(pr, hseed)
    synth.load_synth_(jn, hseed + 1)
    synth.greedy_joint_(jn, HEAD["V"])
    with torch.no_grad():
        jn.ffn_out.bias[BLANK] += BLANK_BIAS
    hop, window, need = 4 * CHUNK, (CHUNK - 1) * 4 + 7, CHUNK * LEFT
    feats = torch.from_numpy(synth.fbank(xseed, STREAMS, window + hop * (CHUNKS - 1)))
    empty = torch.zeros((0, 0, 0, 0))
    gaps, arrays = [], {}
    with torch.no_grad():
        for b in range(STREAMS):
            att, cnn, offset = empty, empty, 0
            tok = cache = None
            for s in range(CHUNKS):                      # model.py:178-199 (carry) and :126-165 (no carry) on the same encoder output
                y, att, cnn = enc.forward_chunk(feats[b:b + 1, s * hop: s * hop + window], offset, need, att, cnn)
                offset += y.size(1)
                assert y.size(1) == CHUNK
                hyps, tok, cache = search(pr, jn, y, N_STEPS, gaps, tok, cache)
                arrays["carry_s%d_c%d" % (b, s)] = np.asarray(hyps, dtype=np.int64)
                hyps, _, _ = search(pr, jn, y, N_STEPS, gaps)
                arrays["nocarry_s%d_c%d" % (b, s)] = np.asarray(hyps, dtype=np.int64)
    rel = min(g / m for g, m in gaps)
    return arrays, gaps, rel


def main():
    for trial in range(200):
        wseed, hseed, xseed = 11, 51 + 2 * trial, 301 + trial
        arrays, gaps, rel = generate(wseed, hseed, xseed)
        ntok = sum(len(v) for k, v in arrays.items() if k.startswith("carry"))
        print("trial %d: %d decisions, smallest gap %.3e max|logit|, %d tokens (carry)" % (trial, len(gaps), rel, ntok))
        if rel >= GAP and STREAMS * CHUNKS <= ntok <= STREAMS * CHUNKS * CHUNK * N_STEPS // 2:      # blanks and symbols both occur
            break
    else:
        raise SystemExit("no seed with every decision's gap >= %g max|logit|" % GAP)
    assert all(g >= GAP * m for g, m in gaps)            # every recorded decision
    arrays["gaps"] = np.asarray([g for g, _ in gaps], dtype=np.float64)
    arrays["logit_max"] = np.asarray([m for _, m in gaps], dtype=np.float64)
    meta = dict(cfg=CFG1, wseed=wseed, hseed=hseed, xseed=xseed, head=HEAD, streams=STREAMS, chunk=CHUNK, left=LEFT, chunks=CHUNKS, n_steps=N_STEPS,
                blank=BLANK, blank_bias=BLANK_BIAS, min_gap_rel=rel, decisions=len(gaps))
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "stream_asr.npz")
    np.savez_compressed(path, **arrays)
    print("stream_asr %.1f KB, %d arrays, smallest gap %.3e" % (os.path.getsize(path) / 1024.0, len(arrays), rel))


if __name__ == "__main__":
    main()
