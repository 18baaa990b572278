"""Chunk-lookahead greedy search (greedy.ChunkGreedySearch, the streaming recogniser's decoder) on the CPU: its torch-operation step.

  1. one lookahead step on random states equals greedy_ref.control applied frame by frame up to and including the next emission or the
     chunk's end (logits from greedy_ref.step64; every fixture decision has a top-2 gap > 1e-4 max|logit|, asserted);
  2. the utterances of tests/golden/greedy.npz in chunks of 4 and 16 frames: the tokens per chunk equal those of chained
     BatchedGreedySearch.search(..., token, state) calls cut at the same boundaries (the arbiter), their concatenation the golden
     whole-utterance tokens, a cut at T // 2 the golden halves; carry=False equals independent search() calls per chunk;
  3. the device-side step counter: max emissions <= steps <= 1 + max emissions, 1 for a live chunk without emission, 0 when every stream
     is idle, and far below frames + emissions (what the single-frame step needs) on blank-heavy chunks."""
import numpy as np
import pytest
import torch

import greedy_chunk_ref as C
import greedy_ref as R
import synth
from conftest import load_golden

CPU = torch.device("cpu")

# name, B, L, (E, H, P, J), V, blank, n_steps, chunk, seed
STEP_CASES = [("b1_c1", 1, 1, (16, 16, 16, 16), 16, 0, 1, 1, 0), ("b17_c4_n3", 17, 2, (48, 80, 96, 64), 73, 72, 3, 4, 0),
              ("b33_c16_n64", 33, 3, (24, 40, 20, 36), 31, 0, 64, 16, 0), ("b9_c32_n1", 9, 4, (32, 32, 48, 32), 97, 0, 1, 32, 0),
              ("b21_c16_n3", 21, 2, (32, 48, 32, 48), 503, 502, 3, 16, 0)]


BLANK_BIAS = 1.5


@pytest.mark.parametrize("case", STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_lookahead_step_equals_single_frame_steps(case):
    import greedy
    name, B, L, (E, H, P, J), V, blank, n_steps, chunk, seed = case
    pr, jn = R.modules(V, E, H, P, J, L, 500 + B + seed)
    with torch.no_grad():
        jn.ffn_out.bias[blank] += BLANK_BIAS             # the plain synthetic head almost never picks the blank: a lookahead would be one frame long
    cg = greedy.ChunkGreedySearch(pr, jn, B, chunk, blank=blank, n_steps=n_steps, use_graph=False, max_tokens=40)
    S = cg.S
    host = C.random_chunk_state(S, np.random.RandomState(3000 + B + seed), V, n_steps, chunk)
    assert (host["lens"] == 0).any() or B == 1
    assert (host["frame_count"] == n_steps - 1).any()
    with torch.no_grad():
        cg._step(S)
    ref = C.chunk_logits64(R.params64(pr, jn), host, S["enc_proj"])
    k, gap, _ = R.argmax_within(ref["logits"], 0.0)
    assert float(gap.min()) > 1e-4 * float(ref["logits"].abs().max()), "the fixture has a near tie: the f32 argmax may go either way"
    exp, singles = C.lookahead_by_single_steps(host, k.numpy(), ref["h_new"].numpy(), ref["c_new"].numpy(), blank, n_steps)
    for key in ("token", "t", "frame_count", "count", "hyps"):
        np.testing.assert_array_equal(S[key].numpy(), exp[key], err_msg="%s: %s" % (name, key))
    np.testing.assert_array_equal((S["t"] >= S["lens"]).numpy(), exp["done"])
    live = host["t"] < host["lens"]
    assert int(S["steps"]) == int(live.any()) and int(S["overflow"]) == 0
    emitted = exp["count"] != host["count"]
    assert not emitted[~live].any()
    for key in ("h", "c"):
        got = S[key].numpy()
        np.testing.assert_array_equal(got[:, ~emitted], host[key][:, ~emitted], err_msg=key)          # bit-unchanged
        if emitted.any():
            new = ref[key + "_new"].numpy()[:, emitted]
            assert float(np.abs(got[:, emitted] - new).max() / np.abs(new).max()) < 1e-6, (name, key)
    if chunk >= 16:
        assert emitted.any() and (live & ~emitted).any() and singles > 1, (name, emitted.sum(), singles)


def _case_modules(c):
    pr, jn = R.modules(c["V"], c["embed"], c["hidden"], c["P"], c["J"], c["layers"], c["seed"], enc_dim=c["E"], shaped=True)
    return pr, jn


def _enc(c, u):
    return torch.from_numpy(synth.normal(c["seed"] + 10 + u, (1, c["T"], c["E"]), 1.0))


def _small_cases():
    g, meta = load_golden("greedy")
    return g, [c for c in meta["cases"] if c["V"] <= 1000]


def check_steps(steps, new, lens, frames):
    """Test 3's bounds for one chunk: `new` the tokens per stream, `lens` the frames per stream."""
    most = max(len(n) for n in new)
    if not any(lens):
        assert steps == 0, steps
        return
    assert most <= steps <= 1 + most, (steps, most)
    if most == 0:
        assert steps == 1
    assert steps < frames + most or frames == 1, (steps, frames, most)


@pytest.mark.parametrize("chunk", [4, 16])
def test_chunked_decoding_equals_chained_search_and_the_golden(chunk):
    import greedy
    g, cases = _small_cases()
    assert cases
    for c in cases:
        pr, jn = _case_modules(c)
        enc = torch.cat([_enc(c, u) for u in range(3)], 0)
        for carry in (True, False):
            cg = greedy.ChunkGreedySearch(pr, jn, 3, chunk, n_steps=c["n_steps"], carry=carry, max_tokens=8)      # small: the buffer has to grow
            bs = greedy.BatchedGreedySearch(pr, jn, n_steps=c["n_steps"], use_graph=False, fused=False)
            tok = st = None
            for piece, lens, raw in C.chunks_of(enc, c["lens"], chunk):
                new = cg.decode(piece, lens)
                ref, (tok, st) = bs.search(raw, lens, token=tok if carry else None, state=st if carry else None)
                assert new == ref, (c["name"], chunk, carry, new, ref)
                check_steps(cg.steps, new, lens, max(lens))
                if carry:
                    t2, (h2, c2) = cg.state()
                    assert torch.equal(t2, tok) and torch.allclose(h2, st[0], atol=1e-6) and torch.allclose(c2, st[1], atol=1e-6)
            if carry:                                    # a chunk boundary coincides with a frame advance: the whole utterance's tokens
                for u in range(3):
                    assert cg.hyps()[u] == g["%s_utt%d" % (c["name"], u)].tolist(), (c["name"], u)


def test_cut_at_half_reproduces_the_golden_halves():
    import greedy
    g, cases = _small_cases()
    for c in cases:
        pr, jn = _case_modules(c)
        enc, half = _enc(c, 0), c["T"] // 2
        chunk = c["T"] - half
        assert chunk <= 32
        cg = greedy.ChunkGreedySearch(pr, jn, 1, chunk, n_steps=c["n_steps"])
        pieces = [torch.cat([enc[:, :half], enc.new_zeros((1, chunk - half, enc.shape[2]))], 1), enc[:, half:].contiguous()]
        first, second = cg.decode(pieces[0], [half]), cg.decode(pieces[1], [chunk])
        assert first[0] == g[c["name"] + "_utt0_first"].tolist() and second[0] == g[c["name"] + "_utt0_second"].tolist()
        assert cg.hyps()[0] == first[0] + second[0]
        cg.reset()
        assert cg.hyps() == [[]] and cg.decode(pieces[0], [half]) == first


def test_step_counter_idle_blank_only_and_blank_heavy_chunks():
    """A head whose blank wins by a wide margin except on marked frames: chunks with no emission take exactly one step, all-idle chunks none,
    and a 16-frame chunk with two emissions 3 steps where the single-frame step needs 18."""
    import greedy
    V, E, H, P, J, L = 73, 48, 80, 96, 64, 2
    pr, jn = R.modules(V, E, H, P, J, L, 51, enc_dim=64, shaped=True)
    with torch.no_grad():                                # logits = shaped head + a blank bonus that the encoder switches off on marked frames
        jn.enc_ffn.weight.zero_(); jn.enc_ffn.bias.zero_()
        jn.enc_ffn.weight[0, 0] = 1.0                    # act[0] = tanh(enc[0] + ...) ~ +-1
        jn.pred_ffn.weight[0].zero_(); jn.pred_ffn.bias[0] = 0.0
        jn.ffn_out.weight[:, 0] = 0.0
        jn.ffn_out.weight[0, 0] = 40.0                   # blank + 40 on frames with enc[0] = +5, - 40 on frames with enc[0] = -5
    B, chunk = 3, 16
    enc = torch.zeros((B, chunk, 64))
    enc[:, :, 0] = 5.0
    enc[0, 3, 0] = enc[0, 11, 0] = -5.0                  # stream 0 emits on frames 3 and 11 (n_steps 1: one symbol per frame), the others never
    cg = greedy.ChunkGreedySearch(pr, jn, B, chunk, n_steps=1)
    bs = greedy.BatchedGreedySearch(pr, jn, n_steps=1, use_graph=False, fused=False)
    new = cg.decode(enc)
    ref, _ = bs.search(enc, [chunk] * B)
    assert new == ref and [len(n) for n in new] == [2, 0, 0]
    assert cg.steps == 3                                 # single-frame steps: 16 frames + 2 emissions - 2 (the cap advances) = 16 at least
    assert chunk + 2 - cg.steps >= 10
    check_steps(cg.steps, new, [chunk] * B, chunk)
    blank_only = enc.clone()
    blank_only[:, :, 0] = 5.0
    assert cg.decode(blank_only, [16, 5, 0]) == [[], [], []] and cg.steps == 1
    assert cg.decode(blank_only, [0, 0, 0]) == [[], [], []] and cg.steps == 0 and cg.replays == 0
    assert cg.decode(enc, [0, 16, 16]) == [[], [], []] and cg.steps == 1       # stream 0 idle: its marked frames are not looked at
    last = cg.decode(enc, [12, 0, 0])
    assert [len(n) for n in last] == [2, 0, 0] and cg.steps == 2               # the last emission's cap moved t to lens: the lower end of the bound
    assert cg.hyps()[0] == new[0] + last[0]


def test_limits_and_eval_mode():
    import greedy
    pr, jn = R.modules(73, 48, 80, 96, 64, 2, 51)
    with pytest.raises(ValueError):
        greedy.ChunkGreedySearch(pr, jn, 0, 4)
    with pytest.raises(RuntimeError):
        greedy.ChunkGreedySearch(pr, jn, 2, 4, fused=True)                     # no GPU here: the fused step is not available, and says so
    cg = greedy.ChunkGreedySearch(pr, jn, 2, 4)
    with pytest.raises(ValueError):
        cg.decode(torch.zeros((2, 5, 64)))
    pr.train()
    with pytest.raises(RuntimeError):
        cg.decode(torch.zeros((2, 4, 64)))


def test_stream_asr_fixture_records_wide_margins():
    """tests/golden/stream_asr.npz (reference streaming tokens, checked on the GPU): every recorded decision's top-2 gap is >= 1e-3 max|logit|,
    blanks and symbols both occur, and carry / no-carry differ somewhere (the reference's eval-path quirk is in the fixture)."""
    g, meta = load_golden("stream_asr")
    rel = g["gaps"] / g["logit_max"]
    assert len(rel) == meta["decisions"] and float(rel.min()) >= 1e-3 and abs(float(rel.min()) - meta["min_gap_rel"]) < 1e-12
    B, n, chunk = meta["streams"], meta["chunks"], meta["chunk"]
    assert B == 3 and n >= 4 and chunk == 16 and meta["head"]["V"] <= 100
    ntok = {k: sum(len(g["%s_s%d_c%d" % (k, b, s)]) for b in range(B) for s in range(n)) for k in ("carry", "nocarry")}
    assert all(B * n <= v < B * n * chunk * meta["n_steps"] for v in ntok.values()), ntok
    assert len(rel) >= 2 * B * n * chunk                 # at least one decision per frame and mode
