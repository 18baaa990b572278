"""CPU: the float64 beam search of tests/attention_search_ref.py (the specification of decoder.AttentionBeamSearch) checked against things it must
equal -- an argmax loop, exhaustive enumeration, the rescorer's score of the same string -- its tie rules, its edge cases, the clear share of the
GPU cases under every mode's delta, and the host layer's argument errors."""
import itertools

import numpy as np
import pytest
import torch

import attention_decoder_ref as A
import attention_search_ref as SR


def small(V, seed, D=16, H=2, eos_bias=0.0):
    import decoder
    torch.manual_seed(seed)
    dec = decoder.TransformerDecoder(V, D, H, 32, 2, 0.1, 0.1, 0.0, 0.0).eval()
    with torch.no_grad():
        dec.output_layer.weight.mul_(8.0)
        dec.output_layer.bias[V - 1] += eos_bias
    g = torch.Generator().manual_seed(seed + 1)
    return dec, dec.state_dict(), torch.randn(7, D, generator=g).double(), H


def string_score(P, memory, n, H, tokens, eos, finished=True):
    """The rescorer's left score of one string (eos included) through attention_decoder_ref.scores; an unfinished one: without the eos term."""
    tk, nlen, score = A.pack_nbest([[(list(tokens), 0.0)]])
    if finished:
        return float(A.scores(P, tk, nlen, score, memory.unsqueeze(0), [n], H, eos, eos)[0, 0])
    tin, tg, mask = A.prep(tk, nlen, score, eos, eos)
    mm = (torch.arange(memory.shape[0]) < n).view(1, 1, -1)
    lp = A.token_logp(A.decoder_logits(P, tin, mask, memory.unsqueeze(0), mm, H), tg)
    return float(lp[0, :len(tokens)].sum())


def test_beam_1_is_the_argmax_loop():
    dec, P, memory, H = small(9, 3, eos_bias=1.0)
    eos = 8
    res = SR.search64(P, memory, 7, 1, H, eos, eos)
    prefix, score, fin = [eos], 0.0, False
    for _ in range(7):
        lp = SR.step_logp(P, [prefix], memory[:7], H)[0]
        k = int(lp.argmax())
        score += float(lp[k])
        prefix.append(k)
        if k == eos:
            fin = True
            break
    tokens, s, f = res["nbest"][0]
    assert list(tokens) == (prefix[1:-1] if fin else prefix[1:]) and f == fin and abs(s - score) <= 1e-12 and len(res["nbest"]) == 1


@pytest.mark.parametrize("V", [3, 4])
def test_a_beam_that_never_prunes_is_exhaustive_enumeration(V):
    dec, P, memory, H = small(V, 10 + V, eos_bias=0.5)
    eos, n, max_len = V - 1, 5, 3
    res = SR.search64(P, memory, n, 16, H, eos, eos, max_len=max_len)
    # all strings: finished ones of up to max_len - 1 tokens, and unfinished ones of exactly max_len tokens
    want = {}
    for L in range(max_len + 1):
        for t in itertools.product(range(V - 1), repeat=L):
            if L < max_len:
                want[(t, True)] = string_score(P, memory, n, H, t, eos, True)
            else:
                want[(t, False)] = string_score(P, memory, n, H, t, eos, False)
    if len(want) <= 16:
        got = {(t, f): s for t, s, f in res["nbest"]}
        assert set(got) == set(want) and all(abs(got[k] - want[k]) <= 1e-12 for k in want)
    else:                                                        # more strings than the beam holds: the kept ones are the best 16 of the enumeration
        best = sorted(want.items(), key=lambda kv: -kv[1])[:16]
        assert [(t, f) for t, s, f in res["nbest"]] == [k for k, _ in best]
        assert all(abs(s - w) <= 1e-12 for (t, s, f), (_, w) in zip(res["nbest"], best))
    assert [s for _, s, _ in res["nbest"]] == sorted((s for _, s, _ in res["nbest"]), reverse=True)


def test_search_and_rescoring_define_the_same_quantity():
    dec, P, memory, H = small(9, 5, eos_bias=3.0)
    res = SR.search64(P, memory, 6, 4, H, 8, 8)
    fin = [(t, s) for t, s, f in res["nbest"] if f]
    assert fin
    for t, s in fin:
        assert abs(s - string_score(P, memory, 6, H, t, 8)) <= 1e-12


def test_ties_lower_class_and_better_parent():
    dec, P, memory, H = small(6, 7)
    with torch.no_grad():                                        # classes 1 and 3 get identical output rows: equal log-probabilities everywhere
        dec.output_layer.weight[3] = dec.output_layer.weight[1]
        dec.output_layer.bias[3] = dec.output_layer.bias[1]
        dec.embed[0].weight[3] = dec.embed[0].weight[1]          # and identical embeddings: the two parents' next steps tie as well
        dec.output_layer.bias[1] += 200.0                          # the tied pair leads every step
        dec.output_layer.bias[3] += 200.0
    P = dec.state_dict()
    res = SR.search64(P, memory, 7, 5, H, 5, 5, max_len=2)
    # (1, 1), (1, 3), (3, 1), (3, 3) have one score: the better parent (class 1 ranked before class 3 at step 0) first, then the lower class
    assert [t for t, _, _ in res["nbest"][:4]] == [(1, 1), (1, 3), (3, 1), (3, 3)]
    assert len({s for _, s, _ in res["nbest"][:4]}) == 1 and not SR.clear(res, 0.0)
    one = SR.search64(P, memory, 7, 5, H, 5, 5, max_len=1)
    assert [t for t, _, _ in one["nbest"][:2]] == [(1,), (3,)] and one["nbest"][0][1] == one["nbest"][1][1]
    # the f32 pruning rule on crafted lists: equal scores -> the better parent, then the lower class
    kept = SR.prune_ref(np.array([[2, 7], [4, 1]]), np.array([[-0.25, -0.25], [-0.25, -1.0]], dtype=np.float32), np.array([-0.5, -0.5], dtype=np.float32), [False, False], 2, 9)
    assert [(c[1], c[2]) for c in kept] == [(0, 2), (0, 7)]


def test_no_frames_and_the_cut_off():
    dec, P, memory, H = small(9, 9, eos_bias=-30.0)
    assert SR.search64(P, memory, 0, 4, H, 8, 8)["nbest"] == [((), 0.0, True)]
    res = SR.search64(P, memory, 7, 3, H, 8, 8, max_len=2)
    assert res["steps"] == 2 and all(len(t) == 2 and not f for t, _, f in res["nbest"])
    assert SR.search64(P, memory, 5, 3, H, 8, 8)["steps"] == 5                       # max_len defaults to the frames


@pytest.mark.parametrize("case", SR.GPU_CASES, ids=[c[0] for c in SR.GPU_CASES])
def test_gpu_cases_are_clear_under_the_modes_they_claim(case):
    """The float64 search ALONE: at least half of each case's utterances are clear under the delta of every mode the case lists, and stay so at
    twice that delta -- the margin.  The other modes' shares are printed (attention_search_ref.GPU_CASES records the sweep behind them)."""
    res = SR.reference(case)
    B = case[1]
    assert "fp32" in case[10]
    for mode in SR.MODES:
        ds, gate = SR.deltas(mode, case)
        n1 = sum(SR.clear(r, d) for r, d in zip(res, ds))
        n2 = sum(SR.clear(r, 2 * d) for r, d in zip(res, ds))
        print("%s %s: per-position gate %.2e, clear %d of %d (at twice the delta: %d)%s" % (case[0], mode, gate, n1, B, n2, "" if mode in case[10] else " -- not claimed"))
        if mode in case[10]:
            assert 2 * n2 >= B, (case[0], mode, n1, n2)
    _, _, lens = SR.inputs(case)
    assert B < 3 or sum(n >= 2 for n in lens) >= 2                                     # a case of three keeps two utterances of real length
    covered = lambda i, m: {c[i] for c in SR.GPU_CASES if m in c[10]}
    assert covered(1, "fp32") == {1, 3, 16} and covered(2, "fp32") == {1, 4, 10, 16} and covered(4, "fp32") == {17, 5002} and covered(5, "fp32") == {144, 256}
    assert covered(2, "fp16") == {1, 4, 10} and covered(1, "fp16") == {1, 3, 16} and covered(2, "bf16") == {1, 4} and all(12 <= c[3] <= 40 for c in SR.GPU_CASES)


def test_bindings_and_argument_errors():
    import cfm
    import decoder
    names = [p[0] for p in cfm.PROTOTYPES]
    assert "cfm_dec_step_attn" in names and "cfm_dec_beam_prune" in names
    assert cfm.DecStepAttnDesc._c_name_ == "cfm_dec_step_attn_desc" and cfm.DecBeamPruneDesc._c_name_ == "cfm_dec_beam_prune_desc"
    dec = decoder.TransformerDecoder(9, 16, 2, 32, 1, 0.0, 0.0, 0.0, 0.0).eval()
    for kw in (dict(beam=0), dict(beam=17), dict(beam=10), dict(beam=4, max_len=1024), dict(beam=4, max_len=0)):      # beam <= 16, beam <= V = 9, max_len <= 1023
        with pytest.raises(ValueError):
            decoder.AttentionBeamSearch(dec, **kw)
    with pytest.raises(TypeError):
        decoder.AttentionBeamSearch(torch.nn.Linear(2, 2))
    bs = decoder.AttentionBeamSearch(dec, beam=8)
    with pytest.raises(ValueError, match="1024"):
        bs.search(torch.zeros(129, 3, 16), [3] * 129)                                  # B * beam = 1032 rows
    with pytest.raises(ValueError, match="max_len"):
        bs.search(torch.zeros(1, 1024, 16), [1024])                                    # max_len defaults to T' = 1024 steps
    with pytest.raises(ValueError, match="2048"):
        decoder.AttentionBeamSearch(dec, beam=2, max_len=8).search(torch.zeros(1, 2049, 16), [2049])      # more keys than the step attention takes
    with pytest.raises(RuntimeError, match="no CPU path"):
        bs.search(torch.zeros(2, 3, 16), [3, 2])
    dec.train()
    with pytest.raises(RuntimeError, match="eval-mode"):
        bs.search(torch.zeros(2, 3, 16), [3, 2])
    dec.eval()
    q, store = torch.zeros(4, 16), torch.zeros(8, 32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        cfm.dec_step_attn(q, store, 2, klen=torch.ones(4, dtype=torch.int32), slot=torch.zeros(4, 2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        cfm.dec_beam_prune(torch.zeros(4, 2, dtype=torch.int32), torch.zeros(4, 2), {"nbest_tokens": torch.zeros(2, 2, 3, dtype=torch.int32)}, torch.zeros(9, 16),
                           torch.zeros(8, 16), 8, 9)
