#!/usr/bin/env python
"""Generate tests/golden/offline_asr.npz by RUNNING THE REFERENCE on the CPU: whole-utterance recognition of 4 utterances of different
lengths, each at batch 1 as the reference decodes -- Transducer.greedy_search (model.py:202-212): ConformerEncoder.forward_chunk_by_chunk
with the length tensor in the chunk-size slot (encoder.py:125-153; one forward_chunk over the whole utterance), then basic_greedy_search
(:215-269) over RNNPredictor.forward_step (predictor.py:76-86) and TransducerJoint.forward (joint.py:20-38).  The search loop is restated
here because model.py does not import without torchaudio (as tests/golden/make_golden_stream_asr.py does).

Needs the reference checkout beside the repository (the path make_golden.py uses); the fixture is data only: the encoder output and the tokens
per utterance, the top-2 logit gap and max|logit| of every decision, sizes and seeds.  The utterances are the first len_b frames of the rows of
ONE padded synthetic batch (the frames behind them are not zeros: a batched implementation must not read them).  Seeds are searched until
EVERY recorded decision has a gap >= 1e-3 max|logit| (100 x the fp32 mode's 1e-5 parity with the reference) and every utterance of more than
one encoder frame emits a token: the token comparison of the test is then exact with no decision left out."""
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
LENS, N_STEPS, BLANK = [200, 163, 47, 7], 3, 0
HEAD = dict(V=73, embed=48, hidden=80, P=96, J=64, layers=2)
GAP = 1e-3
BLANK_BIAS = 0.5                                   # as make_golden_stream_asr.py: blanks and symbols both occur on the synthetic encoder's frames


def search(pr, jn, enc, enc_len, n_steps, gaps):
    """basic_greedy_search (model.py:215-269); appends (top-2 gap, max|logit|) of every decision to gaps."""
    padding = torch.zeros(1, 1)
    tok = torch.tensor([BLANK]).reshape(1, 1)
    cache = pr.init_state(tok)
    t, hyps, prev, per_frame, pred_out, new_cache = 0, [], True, 0, None, None
    while t < enc_len:
        if prev:
            pred_out, new_cache = pr.forward_step(tok, padding, cache)
        logits = jn(enc[:, t:t + 1, :], pred_out)
        z = logits.log_softmax(dim=-1).reshape(-1)
        top = z.double().topk(2).values
        gaps.append((float(top[0] - top[1]), float(logits.abs().max())))
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
    return hyps


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
    feats = torch.from_numpy(synth.fbank(xseed, len(LENS), max(LENS)))
    gaps, arrays = [], {}
    with torch.no_grad():
        for b, n in enumerate(LENS):
            y, mask = enc.forward_chunk_by_chunk(feats[b:b + 1, :n], torch.tensor([n]))           # model.py:206-209
            enc_len = int(mask.squeeze(1).sum())
            assert y.size(0) == 1 and y.size(1) == enc_len == ((n - 1) // 2 - 1) // 2
            arrays["enc_%d" % b] = y[0].numpy().astype(np.float32)
            arrays["tokens_%d" % b] = np.asarray(search(pr, jn, y, enc_len, N_STEPS, gaps), dtype=np.int64)
    rel = min(g / m for g, m in gaps)
    return arrays, gaps, rel


def main():
    for trial in range(200):
        wseed, hseed, xseed = 11, 51 + 2 * trial, 401 + trial
        arrays, gaps, rel = generate(wseed, hseed, xseed)
        ntok = [len(arrays["tokens_%d" % b]) for b in range(len(LENS))]
        print("trial %d: %d decisions, smallest gap %.3e max|logit|, tokens %s" % (trial, len(gaps), rel, ntok))
        if rel >= GAP and all(k > 0 for k, n in zip(ntok, LENS) if n >= 11) and sum(ntok) < len(gaps):   # a token where T' > 1; blanks occur too
            break
    else:
        raise SystemExit("no seed with every decision's gap >= %g max|logit|" % GAP)
    assert all(g >= GAP * m for g, m in gaps)            # every recorded decision
    arrays["gaps"] = np.asarray([g for g, _ in gaps], dtype=np.float64)
    arrays["logit_max"] = np.asarray([m for _, m in gaps], dtype=np.float64)
    meta = dict(cfg=CFG1, wseed=wseed, hseed=hseed, xseed=xseed, head=HEAD, lens=LENS, n_steps=N_STEPS, blank=BLANK, blank_bias=BLANK_BIAS,
                min_gap_rel=rel, decisions=len(gaps))
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "offline_asr.npz")
    np.savez_compressed(path, **arrays)
    print("offline_asr %.1f KB, %d arrays, smallest gap %.3e" % (os.path.getsize(path) / 1024.0, len(arrays), rel))


if __name__ == "__main__":
    main()
