"""GPU: greedy.StreamingBeamSearch / cfm_rnnt_beam_stream_* (csrc/greedy.hip) against the float64 streaming search of
tests/rnnt_beam_ref_stream.py (which test_rnnt_beam_stream_cpu.py holds equal to rnnt_beam_ref.search64 on the whole utterance), against
the offline device search, and against itself under other splits, other neighbours and guarded buffers.  The gates are
test_rnnt_beam_gpu.py's: a CLEAR utterance (every gap its decisions rested on exceeds beam_delta) has the reference's strings in its
order and scores within delta; an unclear one the sorted scores within delta."""
import ctypes

import numpy as np
import pytest
import torch

import greedy_ref as R
import rnnt_beam_ref as BR
import rnnt_beam_ref_stream as BS
import synth
from conftest import load_golden
from extent import Guards

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
NAMES = ("b5_k3", "b4_k15", "b16_k4", "b6_k4_maxlen2", "b5_k3_blank4", "b4_k4_config4")
CASES = [c for c in BR.GPU_CASES if c[0] in NAMES] + [BR.MERGE_CASE]
_heads = {}


def _head(case):
    key = (case[1], case[5], case[9])
    if key not in _heads:
        pr, jn, h = BR.head(*key)
        _heads[key] = (pr.to(DEV), jn.to(DEV), h)
    return _heads[key]


def _make(case, chunk, streams=None, **kw):
    import greedy
    name, hd, B, beam, max_symbols, blank, max_len, T, seed, sharpen = case
    pr, jn, h = _head(case)
    return greedy.StreamingBeamSearch(pr, jn, B if streams is None else streams, beam, chunk, T, max_len=BS.explicit_max_len(case), blank=blank, max_symbols=max_symbols, **kw)


def _feed_all(sb, enc, lens, per):
    """Every stream's utterance `per` frames per feed (per <= sb.chunk), final with its last frames.  Returns the records of every feed."""
    B, T, C = enc.shape[0], enc.shape[1], sb.chunk
    pad = torch.zeros((B, T + C, enc.shape[2]), device=DEV)
    pad[:, :T] = enc.to(DEV)
    out = []
    for f in range(max(1, -(-int(max(lens)) // per))):
        n = [min(per, max(int(l) - f * per, 0)) for l in lens]
        fin = [(f + 1) * per >= int(l) for l in lens]
        chunk = torch.zeros((B, C, enc.shape[2]), device=DEV)
        chunk[:, :per] = pad[:, f * per:f * per + per]
        out.append(sb.decode(chunk, n, fin))
    return out


def _nbest(records):
    assert all(r["nbest"] is not None for r in records[-1]), "a stream is not done after its final feed"
    return [r["nbest"] for r in records[-1]]


def _compare(case, got):
    """test_rnnt_beam_gpu.py's _compare against the reference with the explicit max_len.  Returns (clear utterances, largest score error)."""
    _, _, _, res, deltas = BS.reference(case)
    n_clear, worst = 0, 0.0
    assert len(got) == len(res)
    for b, (g, r, d) in enumerate(zip(got, res, deltas)):
        ref = r["nbest"]
        assert len({tuple(t) for t, _ in g}) == len(g), (case[0], b, "a string twice")
        assert len(g) == len(ref), (case[0], b, len(g), len(ref))
        errs = [abs(x[1] - y[1]) for x, y in zip(sorted(g, key=lambda x: -x[1]), ref)]
        print("  %s utt %d: %s, %d entries, max score error %.2e (delta %.2e)" % (case[0], b, "clear" if BR.clear(r, d) else "unclear", len(g), max(errs), d))
        assert max(errs) <= d, (case[0], b, max(errs), d)
        worst = max(worst, max(errs))
        if BR.clear(r, d):
            n_clear += 1
            assert [tuple(t) for t, _ in g] == [s for s, _ in ref], (case[0], b, g, ref)
            assert [s for _, s in g] == sorted((s for _, s in g), reverse=True)
    return n_clear, worst


@pytest.mark.parametrize("per", [1, 5, 0], ids=["by1", "by5", "all"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_matches_the_float64_search(case, per):
    B, T = case[2], case[7]
    per = per or T
    enc, lens = BR.inputs(case)
    sb = _make(case, per)
    got = _nbest(_feed_all(sb, enc, lens, per))
    n_clear, worst = _compare(case, got)
    _, _, _, res, deltas = BS.reference(case)
    steps = sb.S["step"].tolist()
    print("streaming rnnt beam %s by %d: clear %d of %d, steps %d, replays %d, worst score error %.2e" % (case[0], per, n_clear, B, sb.total_steps, sb.total_replays, worst))
    assert n_clear >= B // 2 and all(steps[b] == res[b]["steps"] for b in range(B) if BR.clear(res[b], deltas[b]))
    assert got[-1] == [([], 0.0)] or B < 3                                              # the utterance without frames


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_matches_the_offline_device_search(case):
    import greedy
    name, hd, B, beam, max_symbols, blank, max_len, T, seed, sharpen = case
    pr, jn, h = _head(case)
    enc, lens = BR.inputs(case)
    sb = _make(case, 5)
    got = _nbest(_feed_all(sb, enc, lens, 5))
    off = greedy.BeamSearch(pr, jn, beam, blank=blank, max_symbols=max_symbols, max_len=BS.explicit_max_len(case))
    want = off.search(enc.to(DEV), lens)
    _, _, _, res, deltas = BS.reference(case)
    s_on, s_off, n = sb.S["step"].tolist(), off._S["step"].tolist(), 0
    for b in range(B):
        if BR.clear(res[b], deltas[b]):
            n += 1
            assert [t for t, _ in got[b]] == [t for t, _ in want[b]], (name, b)
            assert max(abs(x[1] - y[1]) for x, y in zip(got[b], want[b])) <= 2 * deltas[b], (name, b)
            assert s_on[b] == s_off[b], (name, b, s_on[b], s_off[b])
    assert n >= B // 2


def test_pause_and_resume_at_odd_and_even_step_counts():
    """One frame per feed and two steps per replay: streams pause after odd and after even numbers of their own steps, and resume from the
    state the carry left in the buffer the next step reads.  The products are per row, so the result is the all-at-once one to the bit."""
    case = CASES[2]                                                                     # B = 16, beam 4
    enc, lens = BR.inputs(case)
    sb = _make(case, case[7], steps_per_replay=2)
    whole = _nbest(_feed_all(sb, enc, lens, case[7]))
    steps_whole = sb.S["step"].tolist()
    sb.reset()
    seen, recs = set(), []
    C = sb.chunk
    for f in range(case[7]):
        n = [min(1, max(int(l) - f, 0)) for l in lens]
        chunk = torch.zeros((case[2], C, enc.shape[2]), device=DEV)
        chunk[:, :1] = enc[:, f:f + 1].to(DEV)
        recs.append(sb.decode(chunk, n, [f + 1 >= int(l) for l in lens]))
        seen |= {s & 1 for s, p, d in zip(sb.S["step"].tolist(), sb.S["paused"].tolist(), sb.S["done"].tolist()) if p and not d}
    assert seen == {0, 1}, seen                                                         # both parities of a paused stream's step count occurred
    assert _nbest(recs) == whole and sb.S["step"].tolist() == steps_whole
    assert _compare(case, whole)[0] >= case[2] // 2


def test_streams_are_independent():
    """Streams that end at different feeds, one idle for two feeds, one reset mid-run and given a second utterance: each result is that of the
    same utterance decoded alone."""
    case = CASES[2]
    enc, lens = BR.inputs(case)
    enc = enc.to(DEV)
    T, C = case[7], 5
    utts = [b for b in range(case[2]) if int(lens[b]) >= 2][:5]
    alone = {}
    for u in utts:
        one = _make(case, T, streams=1)
        alone[u] = one.decode(enc[u:u + 1].contiguous(), [int(lens[u])], [True])[0]["nbest"]
        assert alone[u] is not None
    sb = _make(case, C, streams=4)
    # stream -> its runs (utterance, first feed): stream 1 is reset before feed 4 and given a second utterance, stream 2 idles for two feeds
    runs = {0: [(utts[0], 0)], 1: [(utts[1], 0), (utts[4], 4)], 2: [(utts[2], 2)], 3: [(utts[3], 0)]}
    results, rec = {}, None
    for f in range(4 + -(-T // C) + 1):
        if f == 4:
            results[(1, utts[1])] = rec[1]["nbest"]
            sb.reset([1])
        chunk, n, fin = torch.zeros((4, C, enc.shape[2]), device=DEV), [0] * 4, [False] * 4
        for s, rr in runs.items():
            started = [r for r in rr if r[1] <= f]
            if started:
                u, f0 = started[-1]
                lo = (f - f0) * C
                k = min(C, max(int(lens[u]) - lo, 0))
                chunk[s, :k], n[s], fin[s] = enc[u, lo:lo + k], k, lo + C >= int(lens[u])
        rec = sb.decode(chunk, n, fin)
        if f < 2:
            assert rec[2]["best"] == ([], 0.0) and rec[2]["nbest"] is None                # idle: nothing fed, nothing decoded
    for s, rr in runs.items():
        results[(s, rr[-1][0])] = rec[s]["nbest"]
    assert len({len(alone[u]) and tuple(alone[u][0][0]) for u in utts}) > 1              # the utterances differ
    for (s, u), got in results.items():
        assert got == alone[u], (s, u, got, alone[u])


def test_stable_and_best_follow_the_reference():
    case = CASES[2]
    name, hd, B, beam, max_symbols, blank, max_len, T, seed, sharpen = case
    P, enc_proj, lens, res, deltas = BS.reference(case)
    enc, _ = BR.inputs(case)
    per = 3
    recs = _feed_all(_make(case, per), enc, lens, per)
    compared = nonempty = 0
    for b in range(B):
        n = int(lens[b])
        _, want = BS.run(P, enc_proj[b], n, beam, BS.explicit_max_len(case), BS.chunk_cuts(n, per), blank, max_symbols)
        mine = [r[b] for r in recs]
        final_best = mine[-1]["nbest"][0][0]
        prev = []
        for f, r in enumerate(mine):
            assert r["stable"][:len(prev)] == prev and r["best"][0][:len(r["stable"])] == r["stable"], (b, f, prev, r)     # monotone; a prefix of best
            assert final_best[:len(r["stable"])] == r["stable"], (b, f)
            prev = r["stable"]
            if BR.clear(res[b], deltas[b]):
                w = want[min(f, len(want) - 1)]
                assert tuple(r["stable"]) == w["stable"] and tuple(r["best"][0]) == w["best"][0] and abs(r["best"][1] - w["best"][1]) <= deltas[b], (b, f, r, w)
                compared += 1
                nonempty += bool(r["stable"]) and r["nbest"] is None
    assert compared >= B and nonempty >= 1


def test_extents():
    """The C entries on guarded buffers: nothing outside the declared extents is written, nbest_tokens' tails and best_tokens beyond best_len
    are untouched, and the enc_proj rows nobody has fed (>= avail, NaN here) reach no result."""
    import cfm
    case = CASES[0]                                                                     # B = 5, beam 3: 15 rows
    name, hd, B, K, max_symbols, blank, max_len, T, seed, sharpen = case
    enc, lens = BR.inputs(case)
    per = 5
    want = _nbest(_feed_all(_make(case, per), enc, lens, per))
    sb = _make(case, per)
    g = Guards(DEV)
    W = sb._head.packs(DEV, enc_ffn=True)
    Wg = {k: ([g.inp(x, name="%s[%d]" % (k, i)) for i, x in enumerate(v)] if isinstance(v, list) else g.inp(v, name=k) if isinstance(v, torch.Tensor) else v)
          for k, v in W.items()}
    Sg = {}
    for k, v in sb.S.items():
        if k == "nodes":
            Sg[k] = g.ws(int(cfm.lib().cfm_rnnt_beam_nodes(B, T, sb.max_len, K)) * 2, torch.int32, name=k).view(-1, 2)     # the documented size
        elif k == "all_done":
            Sg[k] = v
        elif k in ("lens", "feed_final", "mask", "overflow"):
            Sg[k] = g.io(torch.zeros_like(v), name=k)
        else:
            Sg[k] = g.out(tuple(v.shape), v.dtype, name=k)                               # enc_proj among them: every row NaN until it is fed
    assert Sg["nodes"].shape == sb.S["nodes"].shape
    sb.S = Sg
    descs = sb._make_descs(Wg)
    lib = cfm.lib()
    cfm.check(lib.cfm_rnnt_beam_stream_reset(ctypes.byref(descs[0]), None, cfm.stream()), "cfm_rnnt_beam_stream_reset")
    for k in ("token", "t", "hash", "fc", "len", "node", "parent", "ext", "live", "n_fin", "step", "n_done", "nbest_len", "avail", "best_len", "stable_len"):
        assert int(Sg[k].min()) >= 0, (k, "reset left an element unwritten")
    assert int(Sg["done"].max()) == 0 and int(Sg["final"].max()) == 0 and int(Sg["paused"].min()) == 1 and int(Sg["n_done"][0]) == B
    assert not torch.isnan(Sg["h"]).any() and not torch.isnan(Sg["c"]).any()
    for f in range(-(-T // per)):
        n = [min(per, max(int(l) - f * per, 0)) for l in lens]
        chunk = torch.zeros((B, per, enc.shape[2]))
        chunk[:, :min(per, T - f * per)] = enc[:, f * per:f * per + per]
        x = g.inp(chunk, name="enc chunk %d" % f)
        Sg["lens"].copy_(torch.tensor(n))
        Sg["feed_final"].copy_(torch.tensor([(f + 1) * per >= int(l) for l in lens], dtype=torch.uint8))
        for d in descs:
            d.enc = x.data_ptr()
        cfm.check(lib.cfm_rnnt_beam_stream_feed(ctypes.byref(descs[0]), cfm.stream()), "cfm_rnnt_beam_stream_feed")
        steps = 0
        while int(Sg["n_done"][0]) < B:
            for i in range(4):
                cfm.check(lib.cfm_rnnt_beam_stream_step(ctypes.byref(descs[i & 1]), cfm.stream()), "cfm_rnnt_beam_stream_step")
            steps += 4
            assert steps <= 2 * T + 8
        cfm.check(lib.cfm_rnnt_beam_stream_report(ctypes.byref(descs[0]), cfm.stream()), "cfm_rnnt_beam_stream_report")
        torch.cuda.synchronize()
        avail, bl, bt = Sg["avail"].tolist(), Sg["best_len"].tolist(), Sg["best_tokens"].cpu()
        assert avail == [min(int(l), (f + 1) * per) for l in lens]
        for b in range(B):
            assert not torch.isnan(Sg["enc_proj"][b, :avail[b]]).any() and torch.isnan(Sg["enc_proj"][b, avail[b]:]).all(), (f, b)
            assert torch.all(bt[b, bl[b]:] == -1) and torch.all(bt[b, :bl[b]] >= 0), (f, b, "best_tokens beyond best_len was touched, or a token is missing")
        assert not torch.isnan(Sg["best_score"]).any() and not torch.isnan(Sg["score"][Sg["live"] != 0]).any()
    g.check()
    assert int(Sg["overflow"][0]) == 0 and int(Sg["done"].min()) == 1
    nl, ns, nt = Sg["nbest_len"].tolist(), Sg["nbest_score"].tolist(), Sg["nbest_tokens"].cpu()
    got = [[(nt[b, j, :nl[b][j]].tolist(), ns[b][j]) for j in range(K) if ns[b][j] != float("-inf")] for b in range(B)]
    assert got == want
    for b in range(B):
        for j in range(K):
            assert torch.all(nt[b, j, nl[b][j]:] == -1), (b, j, "the tail of nbest_tokens was touched")
    for k in ("h_new", "c_new", "pred", "chunk_proj"):
        assert not torch.isnan(Sg[k]).any(), k


def test_more_than_max_frames_raises_and_changes_nothing():
    case = CASES[0]
    enc, lens = BR.inputs(case)
    sb = _make(case, case[7])
    full = enc.to(DEV)
    r1 = sb.decode(full, [case[7]] + [0] * (case[2] - 1), None)
    with pytest.raises(RuntimeError, match="max_frames"):
        sb.decode(full, [1] + [0] * (case[2] - 1), None)
    r2 = sb.decode(full, [0] * case[2], [True] * case[2])
    assert r1[0]["nbest"] is None and r2[0]["nbest"] is not None
    assert r2[0]["nbest"] == _nbest(_feed_all(_make(case, case[7]), enc, lens, case[7]))[0]


def test_graph_and_weight_updates():
    import greedy
    case = CASES[2]                                                                     # B = 16, beam 4
    enc, lens = BR.inputs(case)
    sb = _make(case, 5)
    got = _nbest(_feed_all(sb, enc, lens, 5))
    assert sb._graph is not None
    eager = _make(case, 5, use_graph=False, steps_per_replay=3)
    assert eager.steps_per_replay == 4 and got == _nbest(_feed_all(eager, enc, lens, 5)) and eager._graph is None
    # other inputs on the same object after a reset: no state is stale
    rs = np.random.RandomState(5)
    enc2 = torch.from_numpy(rs.standard_normal(tuple(enc.shape)).astype(np.float32))
    lens2 = rs.randint(0, case[7] + 1, case[2])
    sb.reset()
    again = _nbest(_feed_all(sb, enc2, lens2, 5))
    assert again == _nbest(_feed_all(_make(case, 5), enc2, lens2, 5)) and again != got
    # an in-place weight change
    name, hd, B, beam, max_symbols, blank, max_len, T, seed, sharpen = case
    pr2, jn2, _ = BR.head(hd, blank, sharpen)
    pr2, jn2 = pr2.to(DEV), jn2.to(DEV)
    fresh = lambda: greedy.StreamingBeamSearch(pr2, jn2, B, beam, 5, T, max_len=BS.explicit_max_len(case), blank=blank, max_symbols=max_symbols)
    sb2 = fresh()
    assert _nbest(_feed_all(sb2, enc2, lens2, 5)) == again
    with torch.no_grad():
        for p in list(pr2.parameters()) + list(jn2.parameters()):
            p.add_(torch.from_numpy(0.05 * rs.standard_normal(tuple(p.shape)).astype(np.float32)).to(DEV))
    sb2.reset()
    after = _nbest(_feed_all(sb2, enc2, lens2, 5))
    assert after == _nbest(_feed_all(fresh(), enc2, lens2, 5)) and after != again


def test_wrong_sizes_raise():
    import greedy
    case = CASES[0]
    pr, jn, h = _head(case)
    for kw in (dict(streams=5, beam=16), dict(streams=17, beam=4), dict(streams=2, beam=0)):
        with pytest.raises(ValueError):
            greedy.StreamingBeamSearch(pr, jn, chunk=4, max_frames=8, **kw)
    assert greedy.StreamingBeamSearch(pr, jn, 2, 3, 4, 8, steps_per_replay=5).steps_per_replay == 6
    with pytest.raises(RuntimeError, match="device only"):
        greedy.StreamingBeamSearch(*BR.head("small")[:2], 2, 3, 4, 8)


def test_streaming_recognizer_with_a_beam():
    import cfm
    import encoder
    import greedy
    import transducer
    g, meta = load_golden("stream_asr")
    before = cfm.get_precision()
    cfm.set_precision("fp32")
    try:
        enc = encoder.ConformerEncoder(cmvn=None, **meta["cfg"]).eval()
        synth.load_synth_(enc, meta["wseed"])
        enc = enc.to(DEV)
        h = meta["head"]
        pr, jn = R.modules(h["V"], h["embed"], h["hidden"], h["P"], h["J"], h["layers"], meta["hseed"], enc_dim=meta["cfg"]["encoder_dim"], shaped=True)
        with torch.no_grad():
            jn.ffn_out.bias[meta["blank"]] += meta["blank_bias"]
        pr, jn = pr.to(DEV), jn.to(DEV)
        B, chunk, chunks, n_steps, blank = meta["streams"], meta["chunk"], meta["chunks"], meta["n_steps"], meta["blank"]
        hop, window, n = 4 * chunk, (chunk - 1) * 4 + 7, chunk * chunks
        feats = torch.from_numpy(synth.fbank(meta["xseed"], B, window + hop * (chunks - 1))).to(DEV)
        M = n
        rec = transducer.StreamingRecognizer(enc, pr, jn, B, chunk, meta["left"], blank=blank, n_steps=n_steps, beam=3, max_frames=n, max_len=M)
        ys, prev = [], [[] for _ in range(B)]
        for s in range(chunks):
            out = rec.step(feats[:, s * hop: s * hop + window].contiguous(), final=[s == chunks - 1] * B)
            ys.append(rec.encoder_out.clone())
            stable = rec.stable_hyps()
            for b in range(B):
                assert stable[b][:len(prev[b])] == prev[b] and rec.hyps()[b][:len(stable[b])] == stable[b]
            prev = stable
        nbest = rec.nbest()
        assert all(x is not None for x in nbest) and [o["nbest"] for o in out] == nbest and rec.hyps() == [x[0][0] for x in nbest]
        y = torch.cat(ys, 1).float()
        want = greedy.BeamSearch(pr, jn, 3, blank=blank, max_symbols=n_steps, max_len=M).search(y, [n] * B)
        P = R.params64(pr, jn)
        enc_proj = y.double().cpu() @ P["j.enc_ffn.weight"].t() + P["j.enc_ffn.bias"]
        n_clear = 0
        for b in range(B):
            r = BR.search64(P, enc_proj[b], n, 3, blank, n_steps, M)
            d = BR.beam_delta(r["steps"], r["max_abs"], BR.GATE_STEP * max(r["logit_max"], 1.0))
            print("  stream %d: %s, best %d tokens, score %.4f (float64 %.4f)" % (b, "clear" if BR.clear(r, d) else "unclear", len(nbest[b][0][0]), nbest[b][0][1], r["nbest"][0][1]))
            assert abs(nbest[b][0][1] - r["nbest"][0][1]) <= d and abs(nbest[b][0][1] - want[b][0][1]) <= 2 * d, (b, d)   # clear or not: the best score
            if BR.clear(r, d):
                n_clear += 1
                assert nbest[b][0][0] == want[b][0][0] == list(r["nbest"][0][0]), b
        print("streaming recognizer beam 3: %d of %d streams clear" % (n_clear, B))
        assert sum(len(x[0][0]) for x in nbest) > 0
        rec.reset([0])
        assert rec.hyps()[0] == [] and rec.nbest()[0] is None and rec.nbest()[1] == nbest[1]
        # beam=None is the greedy recogniser as it was: ChunkGreedySearch on the same encoder output
        plain = transducer.StreamingRecognizer(enc, pr, jn, B, chunk, meta["left"], blank=blank, n_steps=n_steps)
        assert isinstance(plain.decoder, greedy.ChunkGreedySearch) and plain.beam is None
        direct = greedy.ChunkGreedySearch(pr, jn, B, chunk, blank=blank, n_steps=n_steps, steps_per_replay=8, fused=True)
        for s in range(chunks):
            new = plain.step(feats[:, s * hop: s * hop + window].contiguous())
            assert torch.equal(plain.encoder_out, ys[s])
            assert new == direct.decode(ys[s]) and new == [g["carry_s%d_c%d" % (b, s)].tolist() for b in range(B)]
        assert plain.hyps() == direct.hyps()
        with pytest.raises(ValueError):
            plain.step(feats[:, :window].contiguous(), final=[True] * B)
        with pytest.raises(RuntimeError):
            plain.nbest()
    finally:
        cfm.set_precision(before)


def test_weight_change_under_the_captured_graph():
    """A weight assigned through .data drops descriptors and graph; the next utterance is captured again and is a fresh searcher's.
    V = 17: the padded vocabulary (32) differs from it."""
    import greedy
    pr, jn = R.modules(17, 16, 16, 16, 16, 1, 33)
    pr, jn = pr.to(DEV), jn.to(DEV)
    enc, lens = torch.from_numpy(np.random.RandomState(6).standard_normal((2, 4, 16)).astype(np.float32)), [4, 3]
    make = lambda: greedy.StreamingBeamSearch(pr, jn, 2, 2, 2, 4)                        # streams, beam, chunk, max_frames
    sb = make()
    before = _nbest(_feed_all(sb, enc, lens, 2))
    graph, descs, key = sb._graph, sb._descs, sb._key_w
    assert graph is not None and sb._head.padded_vocab() == 32 and sb._descs[0].beam.Vp == 32
    jn.ffn_out.bias.data = jn.ffn_out.bias.data + torch.linspace(-1.0, 1.0, 17, device=DEV)
    sb.reset()
    after = _nbest(_feed_all(sb, enc, lens, 2))
    assert sb._graph is not None and sb._graph is not graph and sb._descs is not descs and sb._key_w != key
    assert after == _nbest(_feed_all(make(), enc, lens, 2)) and after != before
