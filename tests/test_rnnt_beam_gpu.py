"""GPU: greedy.BeamSearch / cfm_rnnt_beam_step (csrc/greedy.hip) against the float64 search of tests/rnnt_beam_ref.py.

For a CLEAR utterance (every gap the reference's decisions rested on exceeds beam_delta) the strings, their order and the scores agree within
delta; for an unclear one the sorted scores agree within delta (the f32 search may have gone the other way at a decision closer than that, and
then holds a hypothesis of nearly the same score).  Everywhere: no string twice, entries beyond the finished ones have length 0 and score -inf."""
import ctypes

import numpy as np
import pytest
import torch

import greedy_ref as R
import rnnt_beam_ref as BR
import synth
from conftest import load_golden
from extent import Guards

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
_heads = {}


def _head(case):
    key = (case[1], case[5], case[9])
    if key not in _heads:
        pr, jn, h = BR.head(*key)
        _heads[key] = (pr.to(DEV), jn.to(DEV), h)
    return _heads[key]


def _search(case, **kw):
    import greedy
    name, hd, B, beam, max_symbols, blank, max_len, T, seed, sharpen = case
    pr, jn, h = _head(case)
    enc, lens = BR.inputs(case)
    bs = greedy.BeamSearch(pr, jn, beam, blank=blank, max_symbols=max_symbols, max_len=max_len, **kw)
    return bs, bs.search(enc.to(DEV), lens)


def _compare(case, got):
    """got: BeamSearch.search's result.  Returns (clear utterances, largest score error)."""
    res, deltas = BR.reference(case)
    n_clear, worst = 0, 0.0
    assert len(got) == len(res)
    for b, (g, r, d) in enumerate(zip(got, res, deltas)):
        ref = r["nbest"]
        assert len({tuple(t) for t, _ in g}) == len(g), (case[0], b, "a string twice")
        assert len(g) == len(ref), (case[0], b, len(g), len(ref))
        errs = [abs(x[1] - y[1]) for x, y in zip(sorted(g, key=lambda x: -x[1]), ref)]
        print("  %s utt %d: %s, %d entries, max score error %.2e (delta %.2e), merges %d" % (case[0], b, "clear" if BR.clear(r, d) else "unclear", len(g),
                                                                                           max(errs), d, r["merges"]))
        assert max(errs) <= d, (case[0], b, max(errs), d)
        worst = max(worst, max(errs))
        if BR.clear(r, d):
            n_clear += 1
            assert [tuple(t) for t, _ in g] == [s for s, _ in ref], (case[0], b, g, ref)
            assert [s for _, s in g] == sorted((s for _, s in g), reverse=True)
    return n_clear, worst


@pytest.mark.parametrize("case", BR.GPU_CASES, ids=[c[0] for c in BR.GPU_CASES])
def test_search_matches_the_float64_search(case):
    bs, got = _search(case)
    n_clear, worst = _compare(case, got)
    B, K = case[2], case[3]
    S = bs._S
    lens, scores = S["nbest_len"].cpu(), S["nbest_score"].cpu()
    for b in range(B):                                                                  # beyond the finished entries: length 0, score -inf
        assert torch.all(lens[b, len(got[b]):] == 0) and torch.all(scores[b, len(got[b]):] == float("-inf"))
    print("rnnt beam %s: clear %d of %d, steps %d, replays %d, worst score error %.2e" % (case[0], n_clear, B, bs.steps, bs.replays, worst))
    res, deltas = BR.reference(case)
    steps = S["step"].tolist()
    assert n_clear >= B // 2 and all(steps[b] == res[b]["steps"] for b in range(B) if BR.clear(res[b], deltas[b]))
    assert got[-1] == [([], 0.0)] or B < 3                                              # the utterance without frames


def test_beam_1_returns_the_greedy_tokens():
    import greedy
    case = BR.GPU_CASES[1]                                                              # B = 64, max_symbols = 1: at most n tokens either way
    pr, jn, h = _head(case)
    enc, lens = BR.inputs(case)
    _, got = _search(case)
    hyps, _ = greedy.BatchedGreedySearch(pr, jn, blank=case[5], n_steps=case[4]).search(enc.to(DEV), lens)
    res, deltas = BR.reference(case)
    n = 0
    for b in range(case[2]):
        if BR.clear(res[b], deltas[b]):
            assert got[b][0][0] == hyps[b], (b, got[b], hyps[b])
            n += 1
    assert n >= 48


def test_merged_scores():
    case = BR.MERGE_CASE
    res, _ = BR.reference(case)
    assert sum(r["merges"] for r in res) > 0                                            # the event, through the reference
    _, got = _search(case)
    assert _compare(case, got)[0] == case[2]                                            # every utterance clear: strings, order, scores


def test_graph_and_reuse_and_weight_updates():
    import greedy
    case = BR.GPU_CASES[5]                                                              # B = 16, beam 4
    bs, got = _search(case)
    _, eager = _search(case, use_graph=False, steps_per_replay=3)
    assert got == eager
    # other inputs and other lens on the same object: no state is stale
    pr, jn, h = _head(case)
    rs = np.random.RandomState(5)
    enc2 = torch.from_numpy(rs.standard_normal((case[2], case[7], h["enc_dim"])).astype(np.float32)).to(DEV)
    lens2 = rs.randint(0, case[7] + 1, case[2])
    fresh = lambda p, j: greedy.BeamSearch(p, j, case[3], blank=case[5], max_symbols=case[4])
    again = bs.search(enc2, lens2)
    assert again == fresh(pr, jn).search(enc2, lens2) and again != got
    # an in-place weight change
    pr2, jn2, _ = BR.head(case[1], case[5], case[9])
    pr2, jn2 = pr2.to(DEV), jn2.to(DEV)
    bs2 = fresh(pr2, jn2)
    before = bs2.search(enc2, lens2)
    assert before == again
    with torch.no_grad():
        for p in list(pr2.parameters()) + list(jn2.parameters()):
            p.add_(torch.from_numpy(0.05 * rs.standard_normal(tuple(p.shape)).astype(np.float32)).to(DEV))
    after = bs2.search(enc2, lens2)
    assert after == fresh(pr2, jn2).search(enc2, lens2) and after != before


def test_extents():
    """The C entries on guarded buffers: bands around every input, output and scratch buffer, outputs pre-filled with NaN / -1."""
    import cfm
    import greedy
    case = BR.GPU_CASES[2]                                                              # B = 5, beam 3: 15 rows
    name, hd, B, K, max_symbols, blank, max_len, T, seed, sharpen = case
    pr, jn, h = _head(case)
    enc, lens = BR.inputs(case)
    bs = greedy.BeamSearch(pr, jn, K, blank=blank, max_symbols=max_symbols, max_len=max_len)
    want = bs.search(enc.to(DEV), lens)
    g = Guards(DEV)
    W = bs._head.packs(DEV)
    Wg = {k: ([g.inp(x, name="%s[%d]" % (k, i)) for i, x in enumerate(v)] if isinstance(v, list) else g.inp(v, name=k) if isinstance(v, torch.Tensor) else v)
          for k, v in W.items()}
    S = bs._state(B, T, DEV)
    Sg = {}
    for k, v in S.items():
        if k == "enc_proj":
            Sg[k] = g.inp(jn.enc_ffn(enc.to(DEV)).detach().contiguous(), name=k)
        elif k == "lens":
            Sg[k] = g.inp(torch.from_numpy(lens.astype(np.int64)), name=k)
        elif k == "nodes":
            Sg[k] = g.ws(int(cfm.lib().cfm_rnnt_beam_nodes(B, T, S["nbest_tokens"].shape[2], K)) * 2, torch.int32, name=k).view(-1, 2)   # the documented size
        elif k == "all_done":
            Sg[k] = v
        else:
            Sg[k] = g.out(tuple(v.shape), v.dtype, name=k)
    assert Sg["nodes"].shape == S["nodes"].shape
    descs = bs._make_descs(Sg, Wg, B, T)
    lib = cfm.lib()
    cfm.check(lib.cfm_rnnt_beam_begin(ctypes.byref(descs[0]), cfm.stream()), "cfm_rnnt_beam_begin")
    for k in ("token", "t", "hash", "fc", "len", "node", "parent", "ext", "live", "n_fin", "step", "n_done", "nbest_len"):
        assert int(Sg[k].min()) >= 0, (k, "begin left an element unwritten")
    assert int(Sg["done"].max()) <= 1
    assert not torch.isnan(Sg["h"]).any() and not torch.isnan(Sg["c"]).any() and not torch.isnan(Sg["nbest_score"]).any()
    steps = 0
    while int(Sg["n_done"][0]) < B:
        for i in range(4):
            cfm.check(lib.cfm_rnnt_beam_step(ctypes.byref(descs[i & 1]), cfm.stream()), "cfm_rnnt_beam_step")
        steps += 4
        assert steps <= 2 * T + 4
    torch.cuda.synchronize()
    g.check()
    nl, ns, nt = Sg["nbest_len"].tolist(), Sg["nbest_score"].tolist(), Sg["nbest_tokens"].cpu()
    got = [[(nt[b, j, :nl[b][j]].tolist(), ns[b][j]) for j in range(K) if ns[b][j] != float("-inf")] for b in range(B)]
    assert got == want
    for b in range(B):
        for j in range(K):
            assert torch.all(nt[b, j, nl[b][j]:] == -1), (b, j, "the tail of nbest_tokens was touched")
    for k in ("h_new", "c_new", "pred", "act"):
        assert not torch.isnan(Sg[k]).any(), k


def test_recognizer_beam():
    import cfm
    import encoder
    import greedy
    import transducer
    _, meta = load_golden("offline_asr")
    before = cfm.get_precision()
    cfm.set_precision("fp32")
    try:
        enc = encoder.ConformerEncoder(cmvn=None, **meta["cfg"]).eval()
        synth.load_synth_(enc, meta["wseed"])
        enc = enc.to(DEV)
        hd = meta["head"]
        pr, jn = R.modules(hd["V"], hd["embed"], hd["hidden"], hd["P"], hd["J"], hd["layers"], meta["hseed"], enc_dim=meta["cfg"]["encoder_dim"], shaped=True)
        with torch.no_grad():
            jn.ffn_out.bias[meta["blank"]] += meta["blank_bias"]
        pr, jn = pr.to(DEV), jn.to(DEV)
        lens = meta["lens"] + [0]
        x = torch.from_numpy(synth.fbank(meta["xseed"], len(meta["lens"]), max(meta["lens"])))
        x = torch.cat([x, x[:1]], 0).to(DEV)
        lens_t = torch.tensor(lens, dtype=torch.int32, device=DEV)
        rec = transducer.OfflineRecognizer(enc, pr, jn, blank=meta["blank"], n_steps=meta["n_steps"])
        nbest = rec.recognize(x, lens_t, beam=3)
        with torch.no_grad():
            y, out_lens = enc.forward_utterances(x, lens_t)
        want = greedy.BeamSearch(pr, jn, 3, blank=meta["blank"], max_symbols=meta["n_steps"]).search(y, out_lens)
        assert nbest == want and len(nbest) == len(lens)
        assert nbest[-1] == [([], 0.0)]
        assert all(1 <= len(n) <= 3 for n in nbest) and sum(len(n[0][0]) for n in nbest) > 0
        plain = rec.recognize(x, lens_t)
        assert plain == rec.search.search(y, out_lens)[0] and plain == rec.recognize(x, lens_t, beam=None)
        assert [p for p in plain[:-1]] == [load_golden("offline_asr")[0]["tokens_%d" % b].tolist() for b in range(len(meta["lens"]))]
    finally:
        cfm.set_precision(before)


def test_wrong_sizes_raise():
    import greedy
    case = BR.GPU_CASES[0]
    pr, jn, h = _head(case)
    enc = torch.zeros((17, 4, h["enc_dim"]), device=DEV)
    with pytest.raises(RuntimeError, match="64"):
        greedy.BeamSearch(pr, jn, 4).search(enc, [4] * 17)                              # 68 rows
    with pytest.raises(ValueError, match="1..15"):
        greedy.BeamSearch(pr, jn, 16)
    with pytest.raises(RuntimeError, match="device only"):
        greedy.BeamSearch(pr, jn, 2).search(enc[:2].cpu(), [4, 4])
    pr.train()
    try:
        with pytest.raises(RuntimeError, match="eval-mode"):
            greedy.BeamSearch(pr, jn, 2).search(enc[:2], [4, 4])
    finally:
        pr.eval()


def test_weight_change_under_the_captured_graph():
    """Unchanged weights reuse descriptors and graph; a weight assigned through .data drops both, and the next search is a fresh searcher's.
    V = 17: the padded vocabulary (32) differs from it."""
    import greedy
    pr, jn = R.modules(17, 16, 16, 16, 16, 1, 31)
    pr, jn = pr.to(DEV), jn.to(DEV)
    enc = torch.from_numpy(np.random.RandomState(5).standard_normal((2, 3, 16)).astype(np.float32)).to(DEV)
    bs = greedy.BeamSearch(pr, jn, 2)
    before = bs.search(enc, [3, 2])
    graph, descs, key = bs._graph, bs._descs, bs._key_w
    assert graph is not None and bs._head.padded_vocab() == 32 and bs._descs[0].Vp == 32 and bs._descs[0].V == 17
    assert bs.search(enc, [3, 2]) == before and bs._graph is graph and bs._descs is descs and bs._key_w == key
    jn.ffn_out.bias.data = jn.ffn_out.bias.data + torch.linspace(-1.0, 1.0, 17, device=DEV)
    after = bs.search(enc, [3, 2])
    assert bs._graph is not None and bs._graph is not graph and bs._descs is not descs and bs._key_w != key
    assert after == greedy.BeamSearch(pr, jn, 2).search(enc, [3, 2]) and after != before
