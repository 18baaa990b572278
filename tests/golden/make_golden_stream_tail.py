#!/usr/bin/env python
"""Generate tests/golden/stream_asr_tail.npz by RUNNING THE REFERENCE on the CPU: streaming recognition of 4 utterances whose lengths are NOT whole
windows, chunk by chunk, driven exactly as Transducer.greedy_search_streaming_eval does (model.py:145-147):

    for cur in range(0, num_frames - 7 + 1, stride):  end = min(cur + decoding_window, num_frames)

so an utterance ends on a SHORT window of 7 .. window-1 feature frames (or, with fewer than 7 frames left over, on no further window at all).  The
reference's ConformerEncoder.forward_chunk (encoder.py:78-123), RNNPredictor.forward_step (predictor.py:76-86) and TransducerJoint.forward
(joint.py:20-38) do every step, per stream; the loops around them (model.py:126-165 without the predictor carried, :178-199 with it) and
basic_greedy_search (:215-269) are restated as in make_golden_stream_asr.py, because model.py does not import without torchaudio.

Lengths window + hop k + r: the final windows give 1, 8 and chunk-1 = 15 encoder frames, and one utterance ends 2 frames behind a whole window (5 frames
left over: no extra window).  The fixture is data only: per stream and window the encoder output, the tokens for carry true / false, the top-2 logit gap of
every decision, sizes, lengths and seeds.  Seeds are searched until EVERY recorded decision has a gap >= 1e-3 max|logit| (the rule of
make_golden_stream_asr.py); the smallest gap is recorded in the metadata."""
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
CHUNK, LEFT, N_STEPS, BLANK = 16, 2, 3, 0
HOP, WINDOW = 4 * CHUNK, (CHUNK - 1) * 4 + 7
# final windows of 9, 37 and 66 frames (1, 8, 15 encoder frames) after 2, 3 and 1 whole windows; 3 whole windows and 2 frames over
LENS = [2 * HOP + 9, 3 * HOP + 37, HOP + 66, WINDOW + 2 * HOP + 2]
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


def windows(n):
    """(start, end) of every window of an utterance of n frames: model.py:145-146."""
    return [(cur, min(cur + WINDOW, n)) for cur in range(0, n - 7 + 1, HOP)]


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
    need = CHUNK * LEFT
    feats = torch.from_numpy(synth.fbank(xseed, len(LENS), max(LENS)))
    empty = torch.zeros((0, 0, 0, 0))
    gaps, arrays = [], {}
    with torch.no_grad():
        for b, n in enumerate(LENS):
            att, cnn, offset = empty, empty, 0
            tok = cache = None
            for s, (cur, end) in enumerate(windows(n)):
                y, att, cnn = enc.forward_chunk(feats[b:b + 1, cur:end], offset, need, att, cnn)
                offset += y.size(1)
                assert y.size(1) == ((end - cur - 1) // 2 - 1) // 2
                arrays["enc_s%d_c%d" % (b, s)] = y[0].numpy().astype(np.float32)
                hyps, tok, cache = search(pr, jn, y, N_STEPS, gaps, tok, cache)
                arrays["carry_s%d_c%d" % (b, s)] = np.asarray(hyps, dtype=np.int64)
                hyps, _, _ = search(pr, jn, y, N_STEPS, gaps)
                arrays["nocarry_s%d_c%d" % (b, s)] = np.asarray(hyps, dtype=np.int64)
    rel = min(g / m for g, m in gaps)
    return arrays, gaps, rel


def main():
    finals = [windows(n)[-1] for n in LENS]
    assert [((e - c - 1) // 2 - 1) // 2 for c, e in finals] == [1, 8, CHUNK - 1, CHUNK] and LENS[3] - finals[3][1] == 2
    frames = sum(((e - c - 1) // 2 - 1) // 2 for n in LENS for c, e in windows(n))
    for trial in range(200):
        wseed, hseed, xseed = 11, 51 + 2 * trial, 401 + trial
        arrays, gaps, rel = generate(wseed, hseed, xseed)
        ntok = sum(len(v) for k, v in arrays.items() if k.startswith("carry"))
        print("trial %d: %d decisions, smallest gap %.3e max|logit|, %d tokens (carry)" % (trial, len(gaps), rel, ntok))
        if rel >= GAP and len(LENS) * 2 <= ntok <= frames * N_STEPS // 2:      # blanks and symbols both occur
            break
    else:
        raise SystemExit("no seed with every decision's gap >= %g max|logit|" % GAP)
    assert all(g >= GAP * m for g, m in gaps)            # every recorded decision
    arrays["gaps"] = np.asarray([g for g, _ in gaps], dtype=np.float64)
    arrays["logit_max"] = np.asarray([m for _, m in gaps], dtype=np.float64)
    meta = dict(cfg=CFG1, wseed=wseed, hseed=hseed, xseed=xseed, head=HEAD, lens=LENS, chunk=CHUNK, left=LEFT, n_steps=N_STEPS,
                windows=[windows(n) for n in LENS], blank=BLANK, blank_bias=BLANK_BIAS, min_gap_rel=rel, decisions=len(gaps))
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "stream_asr_tail.npz")
    np.savez_compressed(path, **arrays)
    print("stream_asr_tail %.1f KB, %d arrays, smallest gap %.3e" % (os.path.getsize(path) / 1024.0, len(arrays), rel))


if __name__ == "__main__":
    main()
