"""GPU: batched edit distance on the device (cfm_edit_distance in csrc/edit_distance.hip through the C entry, cfm.edit_distance, metrics.py and
transducer.OfflineRecognizer.score) against the pure-Python definition of tests/edit_distance_ref.py.

Integer dynamic programming: dist, counts, ops and ops_len are compared by EQUALITY, no tolerance anywhere.  The kernel cases run through the C entry
with every operand between guard bands (tests/extent.py), the scratch included at exactly cfm_edit_distance_scratch_bytes; outputs are pre-filled with
-1 / 0xFF, so an element the kernel owns and did not write fails the comparison -- ops must be zero from ops_len to the row's end.  Padding columns
hold a token of the alphabet (edit_distance_ref.POISON): read, it would change the answer."""
import ctypes

import pytest
import torch

import edit_distance_ref as ref
import greedy_ref as R
import synth
from conftest import load_golden
from extent import Guards

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


@pytest.fixture(scope="module")
def cfm():
    import cfm as c
    return c


@pytest.fixture
def precision():
    import cfm
    before = cfm.get_precision()
    yield cfm.set_precision
    cfm.set_precision(before)


def padded(seqs, pad):
    """Host int32 [N, Lmax + pad] with POISON in every padding column, and the lengths."""
    L = max((len(s) for s in seqs), default=0) + pad
    t = torch.full((len(seqs), L), ref.POISON, dtype=torch.int32)
    for n, s in enumerate(seqs):
        if s:
            t[n, :len(s)] = torch.tensor(s, dtype=torch.int32)
    return t, torch.tensor([len(s) for s in seqs], dtype=torch.int32)


def run_entry(cfm, hyps, refs, ref_index, pad, counts=True, ops=True):
    """The C entry between guard bands.  Returns (dist, counts | None, ops | None, ops_len | None) on the CPU."""
    h, hl = padded(hyps, pad)
    r, rl = padded(refs, pad)
    (P, Hmax), (Rn, Umax) = h.shape, r.shape
    G = Guards()
    d = cfm.EditDistanceDesc()
    keep = [G.inp(h, name="hyp"), G.inp(hl, name="hyp_lens"), G.inp(r, name="ref"), G.inp(rl, name="ref_lens"),
            None if ref_index is None else G.inp(torch.tensor(ref_index, dtype=torch.int32), name="ref_index")]
    d.hyp, d.hyp_lens, d.ref, d.ref_lens, d.ref_index = (cfm.ptr(t) if t is not None and t.numel() else None for t in keep)
    out = [G.out((P,), torch.int32, name="dist"), G.out((P, 4), torch.int32, name="counts") if counts else None,
           G.out((P, Hmax + Umax), torch.uint8, name="ops") if ops else None, G.out((P,), torch.int32, name="ops_len") if ops else None]
    d.dist, d.counts, d.ops, d.ops_len = (cfm.ptr(t) for t in out)
    nbytes = int(cfm.lib().cfm_edit_distance_scratch_bytes(P, Hmax, Umax)) if counts else 0
    ws = G.ws(nbytes, torch.uint8, name="scratch") if nbytes else None
    d.scratch, d.scratch_bytes = cfm.ptr(ws), nbytes
    d.P, d.R, d.Hmax, d.Umax = P, Rn, Hmax, Umax
    rc = cfm.lib().cfm_edit_distance(ctypes.byref(d), cfm.stream())
    assert rc == 0, cfm.lib().cfm_last_error()
    torch.cuda.synchronize()
    G.check()
    return [None if t is None else t.cpu() for t in out], (Hmax, Umax)


def check_call(got, shape, exp, what):
    dist, counts, ops, ops_len = got
    cap = shape[0] + shape[1]
    assert dist.tolist() == [e[0] for e in exp], what
    if counts is not None:
        assert counts.tolist() == [list(e[1]) for e in exp], what
    if ops is not None:
        assert ops_len.tolist() == [len(e[2]) for e in exp], what
        for p, e in enumerate(exp):
            assert ops[p].tolist() == e[2] + [0] * (cap - len(e[2])), (what, p)


# ------------------------------------------------------------------------------------------------------------- the kernel against the definition
@pytest.mark.parametrize("name", [c[0] for c in ref.cases()])
def test_kernel_against_the_definition(cfm, name):
    _, hyps, refs, ref_index, pad = ref.case(name)
    exp = ref.expected(name)
    got, shape = run_entry(cfm, hyps, refs, ref_index, pad)
    check_call(got, shape, exp, name)
    for p, (h, e) in enumerate(zip(hyps, exp)):                                          # and the device alignment is an alignment
        r = refs[p if ref_index is None else ref_index[p]]
        assert ref.valid(got[2][p, :int(got[3][p])].tolist(), h, r, int(got[0][p])), (name, p)
    # null outputs: the distance alone touches no scratch (none is passed); counts without ops are the same counts
    alone, _ = run_entry(cfm, hyps, refs, ref_index, pad, counts=False, ops=False)
    assert alone[1] is None and torch.equal(alone[0], got[0]), name
    no_ops, _ = run_entry(cfm, hyps, refs, ref_index, pad, counts=True, ops=False)
    assert no_ops[2] is None and torch.equal(no_ops[0], got[0]) and torch.equal(no_ops[1], got[1]), name


def test_padding_width_changes_nothing(cfm):
    """Hmax and Umax far beyond every length (another strip width bucket for the scratch, the same for the pairs): the same outputs."""
    _, hyps, refs, ref_index, _ = ref.case("content")
    exp = ref.expected("content")
    got, shape = run_entry(cfm, hyps, refs, ref_index, 400)
    assert shape == (550, 550)
    check_call(got, shape, exp, "content+400")


def test_shared_references_equal_per_pair_calls(cfm):
    _, hyps, refs, ref_index, pad = ref.case("shared-refs")
    assert len(refs) == 3 and len(hyps) == 7
    shared, shape = run_entry(cfm, hyps, refs, ref_index, pad)
    for p, h in enumerate(hyps):
        one, s1 = run_entry(cfm, [h], [refs[ref_index[p]]], None, pad)
        assert int(one[0][0]) == int(shared[0][p]) and one[1][0].tolist() == shared[1][p].tolist(), p
        n = int(one[3][0])
        assert n == int(shared[3][p]) and one[2][0, :n].tolist() == shared[2][p, :n].tolist(), p


def test_op_writes_into_out_and_takes_its_own_scratch(cfm):
    _, hyps, refs, ref_index, pad = ref.case("shared-refs")
    exp = ref.expected("shared-refs")
    h, hl = padded(hyps, pad)
    r, rl = padded(refs, pad)
    G = Guards()
    P, cap = len(hyps), h.shape[1] + r.shape[1]
    out = (G.out((P,), torch.int32, name="dist"), G.out((P, 4), torch.int32, name="counts"), G.out((P, cap), torch.uint8, name="ops"), G.out((P,), torch.int32, name="ops_len"))
    args = (G.inp(h), G.inp(hl), G.inp(r), G.inp(rl), G.inp(torch.tensor(ref_index, dtype=torch.int32)))
    got = cfm.edit_distance(*args, counts=True, ops=True, out=out)
    torch.cuda.synchronize()
    G.check()
    assert all(a is b for a, b in zip(got, out))
    check_call([t.cpu() for t in out], (h.shape[1], r.shape[1]), exp, "op")
    d, c, o, n = cfm.edit_distance(*args, counts=False)
    assert c is None and o is None and n is None and d.tolist() == [e[0] for e in exp]
    d, c, o, n = cfm.edit_distance(*args)
    assert o is None and n is None and c.tolist() == [list(e[1]) for e in exp]
    _, hyps, refs, _, pad = ref.case("P1")                                               # ref_index=None: pair p against reference p
    d = cfm.edit_distance(*(t.to(DEV) for t in padded(hyps, pad)), *(t.to(DEV) for t in padded(refs, pad)))[0]
    assert d.tolist() == [ref.expected("P1")[0][0]]


def test_host_validation(cfm):
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    h, hl, r, rl = i32([[1, 2, 3], [4, 5, 6]]), i32([3, 2]), i32([[1, 2], [3, 4]]), i32([2, 2])
    before = cfm.edit_distance(h, hl, r, rl)[0].tolist()
    assert before == [1, 2]
    with pytest.raises(ValueError, match="contiguous int32"):
        cfm.edit_distance(h.long(), hl, r, rl)
    with pytest.raises(ValueError, match="contiguous int32"):
        cfm.edit_distance(h, hl.float(), r, rl)
    with pytest.raises(ValueError, match="contiguous int32"):
        cfm.edit_distance(i32([[1, 2, 3, 0], [4, 5, 6, 0]])[:, :3], hl, r, rl)
    with pytest.raises(ValueError, match="contiguous int32"):
        cfm.edit_distance(h, hl, r.t(), rl)
    with pytest.raises(ValueError, match="batch sizes differ"):
        cfm.edit_distance(h, i32([3]), r, rl)
    with pytest.raises(ValueError, match="batch sizes differ"):
        cfm.edit_distance(h, hl, r[:1].contiguous(), rl[:1].contiguous())                # P != R without ref_index
    with pytest.raises(ValueError, match="batch sizes differ"):
        cfm.edit_distance(h, hl, r, rl, ref_index=i32([0]))
    with pytest.raises(ValueError, match="exceeds 1024"):
        cfm.edit_distance(torch.zeros((2, 1025), dtype=torch.int32, device=DEV), hl, r, rl)
    with pytest.raises(ValueError, match="exceeds 1024"):
        cfm.edit_distance(h, hl, torch.zeros((2, 1025), dtype=torch.int32, device=DEV), rl)
    with pytest.raises(ValueError, match="out must be"):
        cfm.edit_distance(h, hl, r, rl, out=(i32([0, 0]), None, None, None))             # counts wanted, none given
    with pytest.raises(RuntimeError, match="no CPU path"):
        cfm.edit_distance(h.cpu(), hl, r, rl)
    # the C entry itself
    lib = cfm.lib()
    assert lib.cfm_edit_distance_scratch_bytes(960, 250, 250) == 960 * 250 * 64 and lib.cfm_edit_distance_scratch_bytes(3, 1024, 1024) == 3 * 1024 * 64 * 4
    assert lib.cfm_edit_distance_scratch_bytes(2, 300, 7) == 2 * 7 * 64 * 2 and lib.cfm_edit_distance_scratch_bytes(2, 0, 7) == 0
    need = lib.cfm_edit_distance_scratch_bytes(2, 3, 2)
    bufs = dict(hyp=h, hyp_lens=hl, ref=r, ref_lens=rl, dist=i32([0, 0]), counts=i32([[0] * 4] * 2), scratch=torch.zeros(need, dtype=torch.uint8, device=DEV))
    d = cfm.EditDistanceDesc()
    for k, v in bufs.items():
        setattr(d, k, v.data_ptr())
    d.P, d.R, d.Hmax, d.Umax, d.scratch_bytes = 2, 2, 3, 2, need - 1
    assert lib.cfm_edit_distance(ctypes.byref(d), cfm.stream()) < 0 and b"scratch" in lib.cfm_last_error()
    d.scratch_bytes, d.Hmax = need, 1025
    assert lib.cfm_edit_distance(ctypes.byref(d), cfm.stream()) < 0 and b"exceeds" in lib.cfm_last_error()
    d.Hmax, d.P = 3, 0
    assert lib.cfm_edit_distance(ctypes.byref(d), cfm.stream()) < 0 and b"bad shape" in lib.cfm_last_error()
    d.P, d.Umax = 2, -1
    assert lib.cfm_edit_distance(ctypes.byref(d), cfm.stream()) < 0 and b"bad shape" in lib.cfm_last_error()
    d.Umax, d.R = 2, 3
    assert lib.cfm_edit_distance(ctypes.byref(d), cfm.stream()) < 0 and b"ref_index" in lib.cfm_last_error()
    d.R, d.ops_len = 2, bufs["dist"].data_ptr()
    assert lib.cfm_edit_distance(ctypes.byref(d), cfm.stream()) < 0 and b"go together" in lib.cfm_last_error()
    d.ops_len, d.dist = None, None
    assert lib.cfm_edit_distance(ctypes.byref(d), cfm.stream()) < 0 and b"null pointer" in lib.cfm_last_error()
    d.dist = bufs["dist"].data_ptr()
    assert lib.cfm_edit_distance(ctypes.byref(d), cfm.stream()) == 0
    torch.cuda.synchronize()
    assert bufs["dist"].tolist() == before and bufs["counts"].tolist() == [list(ref.align([1, 2, 3], [1, 2])[1]), list(ref.align([4, 5], [3, 4])[1])]


# ------------------------------------------------------------------------------------------------------------------------------ the public layer
def test_error_rate_over_three_updates(cfm):
    import metrics
    _, hyps, refs, _, _ = ref.case("P130")
    er = metrics.ErrorRate(DEV)
    pairs = list(zip(hyps, refs))
    for lo, hi in ((0, 50), (50, 51), (51, 130)):
        er.update(hyps[lo:hi], refs[lo:hi] if lo else metrics.pack(refs[lo:hi], DEV))  # lists and packed pairs alike
    sums, rate = ref.error_rate(pairs)
    assert er.sums.dtype == torch.int64 and er.sums.is_cuda
    assert tuple(er.counts().values()) == sums and er.compute() == rate
    assert er.reset().counts()["ref_tokens"] == 0
    # word level, the reference's valid_wer: decoded strings through WordIds
    words = metrics.WordIds()
    er.update(words.encode(["the cat sat on mat", "hello there world !", "a x c"]), words.encode(["the cat sat on the mat", "hello world", "a b c"]))
    assert er.counts() == {"S": 1, "D": 1, "I": 2, "hits": 9, "ref_tokens": 11} and er.compute() == 4 / 11
    dist, counts = metrics.edit_distance([[1, 2, 3], []], [[1, 3], [4]])
    assert dist.is_cuda and dist.tolist() == [1, 1] and counts.tolist() == [[0, 0, 1, 2], [0, 1, 0, 0]]


def test_nbest_errors_on_ragged_lists(cfm):
    import metrics
    import random
    rs = random.Random(3)
    seq = lambda n: [rs.randrange(4) for _ in range(n)]
    refs = [seq(12), seq(9), seq(20)]
    # 1, 3 and 15 entries; one empty hypothesis; the second list has its best distance twice (entries 1 and 2 are the reference with one token
    # dropped at either end: both at distance 1, entry 0 further away), so the tie goes to the lower index
    nbest = [[(seq(10), -1.0)],
             [([9, 9] + refs[1], -0.5), (refs[1][1:], -0.7), (refs[1][:-1], -0.9)],
             [(seq(rs.randrange(14, 26)), -float(k)) for k in range(14)] + [([], -20.0)]]
    got = metrics.nbest_errors(nbest, refs)
    want = []
    for entries, r in zip(nbest, refs):
        d = [ref.distance(e[0], r) for e in entries]
        want.append({"dist": d, "oracle": d.index(min(d)), "oracle_dist": min(d)})
    assert got == want
    assert got[1]["dist"] == [2, 1, 1] and got[1]["oracle"] == 1 and got[2]["dist"][-1] == 20
    n = sum(len(r) for r in refs)
    assert metrics.oracle_error_rate(nbest, refs) == sum(w["oracle_dist"] for w in want) / n
    assert metrics.oracle_error_rate(nbest, metrics.pack(refs, DEV)) == sum(w["oracle_dist"] for w in want) / n
    with pytest.raises(ValueError, match="no hypothesis"):
        metrics.nbest_errors([[], nbest[1], nbest[2]], refs)
    with pytest.raises(ValueError, match="n-best lists for"):
        metrics.nbest_errors(nbest[:2], refs)


def offline_recognizer(meta):
    import decoder
    import encoder
    import transducer
    enc = synth.load_synth_(encoder.ConformerEncoder(cmvn=None, **meta["cfg"]).eval(), meta["wseed"]).to(DEV)
    h = meta["head"]
    pr, jn = R.modules(h["V"], h["embed"], h["hidden"], h["P"], h["J"], h["layers"], meta["hseed"], enc_dim=meta["cfg"]["encoder_dim"], shaped=True)
    with torch.no_grad():
        jn.ffn_out.bias[meta["blank"]] += meta["blank_bias"]
    ctc = synth.load_synth_(decoder.CTCDecoder(h["V"], meta["cfg"]["encoder_dim"], 0.0).eval(), 700).to(DEV)
    return transducer.OfflineRecognizer(enc, pr.to(DEV), jn.to(DEV), blank=meta["blank"], n_steps=meta["n_steps"], ctc=ctc), (enc, pr, jn)


def labels_near(hyps):
    """Known transcripts a few edits away from the hypotheses: utterance b drops its token b, replaces its last token and gains two tokens in front."""
    out = []
    for b, h in enumerate(hyps):
        lab = [1, 2] + [t for k, t in enumerate(h) if k != b]
        if lab:
            lab[-1] = lab[-1] % 5 + 1
        out.append(lab)
    Umax = max(len(l) for l in out) + 2
    padded_labels = torch.zeros((len(out), Umax), dtype=torch.int64)                     # padded [B, Umax] as for align; the padding is ignored
    for b, l in enumerate(out):
        padded_labels[b, :len(l)] = torch.tensor(l)
        padded_labels[b, len(l):] = ref.POISON
    return out, padded_labels, [len(l) for l in out]


@pytest.mark.parametrize("head,beam", [("rnnt", None), ("ctc", None), ("rnnt", 4)])
def test_offline_recognizer_score(cfm, precision, head, beam):
    import transducer
    precision("fp32")
    _, meta = load_golden("offline_asr")
    rec, (enc, pr, jn) = offline_recognizer(meta)
    lens = torch.tensor(meta["lens"], dtype=torch.int32, device=DEV)
    x = torch.from_numpy(synth.fbank(meta["xseed"], len(meta["lens"]), max(meta["lens"]))).to(DEV)
    hyps = (rec.recognize if head == "rnnt" else rec.recognize_ctc)(x, lens, beam=beam)
    best = hyps if beam is None else [n[0][0] for n in hyps]
    assert sum(len(h) for h in best) > 0
    labels, padded_labels, llens = labels_near(best)
    got = rec.score(x, lens, padded_labels, llens, beam=beam, head=head)
    assert got["hyps"] == hyps
    exp = [ref.align(h, l) for h, l in zip(best, labels)]
    assert got["dist"].is_cuda and got["dist"].tolist() == [e[0] for e in exp] and got["counts"].tolist() == [list(e[1]) for e in exp]
    assert sum(e[0] for e in exp) > 0
    assert got["error_rate"] == ref.error_rate(list(zip(best, labels)))[1]
    if beam is None:
        assert "oracle" not in got
    else:
        want = []
        for entries, l in zip(hyps, labels):
            d = [ref.distance(e[0], l) for e in entries]
            want.append({"dist": d, "oracle": d.index(min(d)), "oracle_dist": min(d)})
        assert got["oracle"] == want and got["oracle_error_rate"] == sum(w["oracle_dist"] for w in want) / sum(llens)
    if head == "ctc":
        with pytest.raises(RuntimeError, match="without a CTC head"):
            transducer.OfflineRecognizer(enc, pr.to(DEV), jn.to(DEV), blank=meta["blank"]).score(x, lens, padded_labels, llens, head="ctc")
        with pytest.raises(ValueError, match="head must be"):
            rec.score(x, lens, padded_labels, llens, head="attention")
