"""CPU (no GPU): the float64 restatement of the attention decoder and of n-best rescoring (tests/attention_decoder_ref.py) against an independent
construction and its own invariances; the ranking rule; the modules' names against the reference's (tests/golden/attention_decoder_keys.json); and
the float32 yardstick from which tests/test_rescore_gpu.py takes its tolerances."""
import json
import math
import os

import pytest
import torch

import attention_decoder_ref as R
from conftest import ROOT


def small_decoder(D, layers, V=11, H=2, FF=24, seed=0):
    import decoder
    torch.manual_seed(seed)
    dec = decoder.TransformerDecoder(V, D, H, FF, layers, 0.1, 0.1, 0.0, 0.0).eval()
    with torch.no_grad():
        for p in dec.parameters():                             # LayerNorm weights and all biases away from their 1 / 0 defaults
            p.add_(0.1 * torch.randn(p.shape))
    return dec, {k: v.double() for k, v in dec.state_dict().items()}


@pytest.mark.parametrize("D", [16, 32])
@pytest.mark.parametrize("layers", [1, 2])
def test_restatement_equals_torchs_own_pre_norm_decoder(D, layers):
    """torch.nn.TransformerDecoderLayer(norm_first=True, activation='relu', batch_first=True) in float64 with the weights copied over."""
    V, H, FF = 11, 2, 24
    dec, P = small_decoder(D, layers, V, H, FF)
    stack = []
    for l in range(layers):
        t = torch.nn.TransformerDecoderLayer(D, H, FF, dropout=0.0, activation="relu", batch_first=True, norm_first=True, dtype=torch.float64).eval()
        pre = "decoders.%d." % l
        with torch.no_grad():
            for ours, theirs in (("self_attn", t.self_attn), ("src_attn", t.multihead_attn)):
                theirs.in_proj_weight.copy_(torch.cat([P[pre + ours + ".linear_%s.weight" % c] for c in "qkv"]))
                theirs.in_proj_bias.copy_(torch.cat([P[pre + ours + ".linear_%s.bias" % c] for c in "qkv"]))
                theirs.out_proj.weight.copy_(P[pre + ours + ".linear_out.weight"])
                theirs.out_proj.bias.copy_(P[pre + ours + ".linear_out.bias"])
            for ours, theirs in (("feed_forward.w_1", t.linear1), ("feed_forward.w_2", t.linear2), ("norm1", t.norm1), ("norm2", t.norm2), ("norm3", t.norm3)):
                theirs.weight.copy_(P[pre + ours + ".weight"])
                theirs.bias.copy_(P[pre + ours + ".bias"])
        stack.append(t)
    g = torch.Generator().manual_seed(5)
    Rn, Lc, T = 3, 6, 9
    tokens_in = torch.randint(0, V, (Rn, Lc), generator=g)
    lens, enc_lens = torch.tensor([6, 4, 1]), torch.tensor([9, 7, 2])
    memory = torch.randn(Rn, T, D, generator=g, dtype=torch.float64)
    i = torch.arange(Lc)
    mask = (i.view(1, 1, Lc) <= i.view(1, Lc, 1)) & (i.view(1, 1, Lc) < lens.view(-1, 1, 1))
    mm = (torch.arange(T).unsqueeze(0) < enc_lens.unsqueeze(1)).unsqueeze(1)
    ours = R.decoder_logits(P, tokens_in, mask, memory, mm, H)
    x = R.embed(P, tokens_in)
    with torch.no_grad():
        for t in stack:
            x = t(x, memory, tgt_mask=~(i.view(1, Lc) <= i.view(Lc, 1)), tgt_key_padding_mask=~(i.unsqueeze(0) < lens.unsqueeze(1)),
                  memory_key_padding_mask=~mm[:, 0])
        theirs = torch.nn.functional.layer_norm(x, (D,), P["after_norm.weight"], P["after_norm.bias"], 1e-5) @ P["output_layer.weight"].t() + P["output_layer.bias"]
    valid = i.unsqueeze(0) < lens.unsqueeze(1)
    err = float((ours - theirs)[valid].abs().max())
    print("D=%d layers=%d: max |restatement - torch| = %.3e" % (D, layers, err))
    assert err <= 1e-10
    # the embedding: the f32 sinusoid table by POSITION, the embedding scaled by sqrt(D)
    assert torch.equal(R.embed(P, tokens_in)[1, 2], P["embed.0.weight"][tokens_in[1, 2]] * math.sqrt(D) + R._sinusoid_table(Lc, D)[2, 0].double())


def _scores(P, nbest, memory, enc_lens, H, V, N=None, Lmax=None, reverse=False):
    tokens, nlen, score = R.pack_nbest(nbest, N, Lmax, pad_token=V - 2)
    return R.scores(P, tokens, nlen, score, memory, enc_lens, H, V - 1, V - 1, reverse)


def test_invariances_of_the_restatement():
    V, H, D = 11, 2, 16
    _, P = small_decoder(D, 2, V, H)
    g = torch.Generator().manual_seed(7)
    memory = torch.randn(2, 8, D, generator=g, dtype=torch.float64)
    enc_lens = [8, 5]
    y, z = [3, 1, 4, 1, 5], [2, 7]
    base = _scores(P, [[(y, -1.0), (z, -2.0)], [(z, -1.0)]], memory, enc_lens, H, V)
    s_y, s_z0, s_z1 = float(base[0, 0]), float(base[0, 1]), float(base[1, 0])
    # Lmax and N: more padding, more (unused) slots
    wide = _scores(P, [[(y, -1.0), (z, -2.0)], [(z, -1.0)]], memory, enc_lens, H, V, N=5, Lmax=12)
    assert abs(float(wide[0, 0]) - s_y) <= 1e-12 and abs(float(wide[0, 1]) - s_z0) <= 1e-12 and abs(float(wide[1, 0]) - s_z1) <= 1e-12
    assert float(wide[0, 4]) == 0.0 and float(wide[1, 1]) == 0.0
    # the slot, and the first-pass score, change nothing
    swapped = _scores(P, [[(z, -9.0), (y, -0.1)], [(z, -1.0)]], memory, enc_lens, H, V)
    assert abs(float(swapped[0, 1]) - s_y) <= 1e-12 and abs(float(swapped[0, 0]) - s_z0) <= 1e-12
    # the batch position: the utterances exchanged
    flipped = _scores(P, [[(z, -1.0)], [(y, -1.0), (z, -2.0)]], memory.flip(0), enc_lens[::-1], H, V)
    assert abs(float(flipped[1, 0]) - s_y) <= 1e-12 and abs(float(flipped[1, 1]) - s_z0) <= 1e-12 and abs(float(flipped[0, 0]) - s_z1) <= 1e-12
    # memory frames past enc_len are never seen
    noisy = memory.clone()
    noisy[1, 5:] = 1e3
    assert abs(float(_scores(P, [[(y, -1.0), (z, -2.0)], [(z, -1.0)]], noisy, enc_lens, H, V)[1, 0]) - s_z1) <= 1e-12
    # causality: position i does not depend on tokens after i
    tokens, nlen, score = R.pack_nbest([[(y, -1.0)], [(y[:3] + [9, 9], -1.0)]])
    tin, tg, mask = R.prep(tokens, nlen, score, V - 1, V - 1)
    mm = torch.ones((2, 1, 8), dtype=torch.bool)
    logits = R.decoder_logits(P, tin, mask, memory[:1].expand(2, -1, -1), mm, H)
    assert float((logits[0, :4] - logits[1, :4]).abs().max()) <= 1e-12 and float((logits[0, 4:] - logits[1, 4:]).abs().max()) > 1e-3
    # a palindrome scores the same reversed under shared weights
    pal = [4, 2, 6, 2, 4]
    fwd = _scores(P, [[(pal, -1.0)], [(z, -1.0)]], memory, enc_lens, H, V)
    rev = _scores(P, [[(pal, -1.0)], [(z, -1.0)]], memory, enc_lens, H, V, reverse=True)
    assert abs(float(fwd[0, 0]) - float(rev[0, 0])) <= 1e-12 and abs(float(fwd[1, 0]) - float(rev[1, 0])) > 1e-6


def test_ranking_rule_with_ties_and_unused_slots():
    inf = float("inf")
    assert R.rank([-3.0, -1.0, -2.0]) == [1, 2, 0]
    assert R.rank([-1.0, -2.0, -1.0, -2.0]) == [0, 2, 1, 3]                       # exact ties: the better first-pass rank first
    assert R.rank([-inf, -1.0, -inf, -5.0]) == [1, 3, 0, 2]                       # unused slots last, among themselves by index
    assert R.rank([float("nan"), -1.0]) == [1, 0]
    # through rescore: planted exact ties (the same hypothesis twice with the same first-pass score), an unused slot in the middle
    V, H, D = 11, 2, 16
    _, P = small_decoder(D, 1, V, H)
    memory = torch.randn(1, 4, D, dtype=torch.float64)
    tokens, nlen, score = R.pack_nbest([[([1, 2], -2.0), ([3], -1.0), ([1, 2], -2.0), ([5], -1.0)]], N=5)
    nlen[0, 3], score[0, 3] = -1, -inf
    final, left, right, order = R.rescore(P, P, tokens, nlen, score, memory, [4], H, V - 1, V - 1, 0.5, 0.0)
    assert float(final[0, 0]) == float(final[0, 2]) and float(final[0, 3]) == -inf and float(final[0, 4]) == -inf
    o = order[0]
    assert o.index(0) < o.index(2) and o[-2:] == [3, 4]
    assert float(right.abs().max()) == 0.0                                            # the right decoder is not evaluated at reverse_weight 0
    both = R.rescore(P, P, tokens, nlen, score, memory, [4], H, V - 1, V - 1, 0.5, 0.3)
    assert abs(float(both[0][0, 1]) - (0.7 * float(both[1][0, 1]) + 0.3 * float(both[2][0, 1]) - 0.5)) <= 1e-12


def test_state_dict_equals_the_references():
    import decoder
    fixture = json.load(open(os.path.join(ROOT, "tests", "golden", "attention_decoder_keys.json")))
    assert sorted(fixture) == ["bi", "transformer"]
    for case in fixture.values():
        mod = getattr(decoder, case["cls"])(**case["args"])
        assert {k: list(v.shape) for k, v in mod.state_dict().items()} == case["state"]
    assert any(k.startswith("left_decoder.decoders.1.src_attn.linear_q") for k in fixture["bi"]["state"])
    assert any(k.startswith("right_decoder.embed.0.") for k in fixture["bi"]["state"])


def test_the_references_import_line_and_train_mode():
    from decoder import CTCDecoder, BiTransformerDecoder                                # executor.py:5, deploy.py:12
    import decoder
    import decoder_layer
    assert CTCDecoder is decoder.CTCDecoder
    bi = BiTransformerDecoder(11, 16, 2, 24, 1, 1, 0.0, 0.0, 0.0, 0.0)
    assert bi.training
    x = torch.zeros(1, 3, 16)
    with pytest.raises(NotImplementedError, match="cross-attention"):
        bi(x, torch.ones(1, 1, 3, dtype=torch.bool), torch.zeros(1, 2, dtype=torch.long), torch.tensor([2]), None, 0.0)
    with pytest.raises(NotImplementedError, match="cross-attention"):
        bi.left_decoder.decoders[0](x, torch.ones(1, 3, 3, dtype=torch.bool), x, torch.ones(1, 1, 3, dtype=torch.bool))
    with pytest.raises(NotImplementedError, match="cross-attention"):
        decoder.AttentionRescorer(bi).scores(x, [3], torch.zeros(1, 1, 2, dtype=torch.int32), torch.zeros(1, 1, dtype=torch.int32), torch.zeros(1, 1))
    layer = decoder_layer.TransformerDecoderLayer(16, 2, 24, 0.0, 0.0, 0.0)
    assert layer.self_attn.return_cache is False and layer.src_attn.return_cache is False
    with pytest.raises(RuntimeError, match="no CPU path"):
        bi.eval()(x, torch.ones(1, 1, 3, dtype=torch.bool), torch.zeros(1, 2, dtype=torch.long), torch.tensor([2]), None, 0.0)
    with pytest.raises(ValueError, match="right decoder"):
        decoder.AttentionRescorer(bi.left_decoder, reverse_weight=0.3)
    r = decoder.AttentionRescorer(bi)
    assert (r.sos, r.eos, r.first_pass_weight, r.reverse_weight) == (10, 10, 0.5, 0.0)


def test_yardstick_and_the_margin_cap_of_the_chosen_seeds():
    """The float32 yardstick per precision mode (printed: DESIGN quotes it) and, by the restatement alone, that at most 10 % of the seeded
    utterances have adjacent finals closer than twice the GPU gate (4 x the yardstick), i.e. are exempt from the ranking check."""
    for rw in (0.0, R.CASE["reverse_weight"]):
        worst = {m: [0.0, 0.0] for m in ("bf16", "fp16", "fp32")}
        gaps = []
        for seed in R.SEEDS:
            for T in R.FRAMES:
                for m in worst:
                    e = R.yardstick(m, seed, T, rw)
                    worst[m] = [max(a, b) for a, b in zip(worst[m], e)]
                final = R.module_reference(*R.module_case(seed, T), rw)[0]
                gaps += [R.min_gap(row.tolist()) for row in final]
        assert len(gaps) == len(R.SEEDS) * len(R.FRAMES) * R.CASE["B"]
        for m, (e_final, e_logits) in worst.items():
            under = sum(g <= 2 * 4 * e_final for g in gaps)
            print("reverse_weight %.1f %s: yardstick final %.3e logits %.3e; gate %.3e / %.3e; %d of %d utterances under the ranking margin"
                  % (rw, m, e_final, e_logits, 4 * e_final, 4 * e_logits, under, len(gaps)))
            assert e_final > 0 and e_logits > 0
            assert under <= 0.1 * len(gaps), (m, under, sorted(gaps)[:4])
