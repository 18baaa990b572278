"""CPU (no GPU): the float64 restatements of CTC decoding (ctc_decode_ref.py) against brute force and against a one-line formulation, the margin
audit of the prefix-beam cases that test_ctc_decode_gpu.py runs, the C size of the two new descriptors, and the loud failures of the new entry
points (CPU tensors, train mode, a CTC head of the wrong width)."""
import ctypes
import os
import subprocess

import pytest
import torch

import ctc_decode_ref as ref
from conftest import ROOT


@pytest.fixture(scope="module")
def cfm():
    import cfm as c
    if not os.path.exists(c.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return c


TINY = [(seed, V, T) for seed, (V, T) in enumerate([(2, 1), (2, 6), (3, 4), (3, 6), (4, 3), (4, 5), (4, 6), (3, 5)])]


@pytest.mark.parametrize("seed,V,T", TINY)
@pytest.mark.parametrize("blank", [0, 1])
def test_prefix_beam_restatement_equals_brute_force(seed, V, T, blank):
    """k = V and a beam that holds every prefix of the case: the search loses nothing, so its n-best is the exact posterior of every string."""
    g = torch.Generator().manual_seed(seed)
    lp = torch.log_softmax(torch.randn((T, V), generator=g, dtype=torch.float64) * 2.0, -1)
    exact = ref.brute_force(lp, blank)
    prefixes = {l[:n] for l in exact for n in range(len(l) + 1)}
    beam = len(prefixes)
    idx, v, _ = ref.topk64(lp, V)
    got = ref.prefix_beam_search64(idx, v, T, beam, blank)
    assert len(got["nbest"]) <= beam and not got["frame_gaps"]                          # the beam never dropped a candidate
    assert {l for l, _ in got["nbest"]} == set(exact)
    for l, s in got["nbest"]:
        assert abs(s - exact[l]) <= 1e-12, (l, s, exact[l])
    want = sorted(exact.items(), key=lambda kv: -kv[1])
    assert [l for l, _ in got["nbest"]] == [l for l, _ in want]                         # (no ties in random data)
    assert all(a[1] >= b[1] for a, b in zip(got["nbest"], got["nbest"][1:]))


def test_prefix_beam_of_one_keeps_the_best_prefix_and_zero_frames_give_the_empty_string():
    g = torch.Generator().manual_seed(5)
    lp = torch.log_softmax(torch.randn((9, 5), generator=g, dtype=torch.float64), -1)
    idx, v, _ = ref.topk64(lp, 5)
    got = ref.prefix_beam_search64(idx, v, 9, 1, 0)
    assert len(got["nbest"]) == 1
    assert ref.prefix_beam_search64(idx, v, 0, 4, 0)["nbest"] == [((), 0.0)]


@pytest.mark.parametrize("blank", [0, 3])
def test_best_path_restatement_equals_unique_consecutive(blank):
    g = torch.Generator().manual_seed(11)
    for T in (1, 7, 64, 130):
        idx = torch.randint(0, 5, (T,), generator=g)
        lp = torch.randn((T,), generator=g, dtype=torch.float64)
        toks, frames, lps, last = ref.best_path(idx, lp, T, blank)
        u = torch.unique_consecutive(idx)
        assert toks == u[u != blank].tolist()
        assert [int(idx[f]) for f in frames] == toks and lps == [float(lp[f]) for f in frames] and last == int(idx[-1])
        assert all(f == 0 or int(idx[f - 1]) != int(idx[f]) for f in frames)            # the FIRST frame of each run emits
    # a repeat across two calls collapses, a blank between them does not
    a = ref.best_path([2, 2], [0.0, 0.0], 2, 0)
    assert a[0] == [2] and ref.best_path([2, 1], [0.0, 0.0], 2, 0, prev=a[3], frame_base=2)[:2] == ([1], [3])
    assert ref.best_path([0, 2], [0.0, 0.0], 2, 0, prev=2)[0] == [2]


def audit(case):
    """(clear, results per utterance) of one prefix-beam case by the restatement alone: clear iff every recorded gap exceeds delta."""
    seed, V, T, beam = case
    idx, logp, lens = ref.beam_case(seed, V, T, beam)
    clear, res = True, []
    for b in range(idx.shape[0]):
        r = ref.prefix_beam_search64(idx[b], logp[b], int(lens[b]), beam, 0)
        r["delta"] = ref.beam_delta(T, r["max_abs"])
        clear &= all(gap > r["delta"] for gap in r["frame_gaps"] + r["nbest_gaps"])
        res.append(r)
    return clear, res


def test_prefix_beam_margin_audit():
    """At most 10 % of the 64 GPU cases may be compared on scores only (some recorded gap within delta): shown here without the code under test."""
    cases = ref.beam_cases_64()
    assert len(cases) == 64 and {c[1:] for c in cases} == set(ref.BEAM_CASES)
    verdicts = [audit(c) for c in cases]
    unclear = [c for c, (ok, _) in zip(cases, verdicts) if not ok]
    print("unclear cases: %d of %d %s" % (len(unclear), len(cases), unclear))
    assert len(unclear) <= 0.10 * len(cases), unclear
    merges = sum(r["reentry"] for _, res in verdicts for r in res)
    drops = sum(len(r["frame_gaps"]) for _, res in verdicts for r in res)
    assert merges > 0 and drops > 100, (merges, drops)                                  # the cases do exercise merging and pruning


def test_reentry_case_is_clear_and_has_the_event():
    """The constructed case of the GPU test: a prefix leaves the beam and comes back while its extension stays, and the two merge."""
    clear, res = audit(ref.REENTRY_CASE)
    assert clear and sum(r["reentry"] for r in res) > 0, (clear, [r["reentry"] for r in res])


def test_new_ctypes_structs_match_c_sizes(cfm, tmp_path):
    structs = {"cfm_ctc_greedy_desc": cfm.CtcGreedyDesc, "cfm_ctc_beam_desc": cfm.CtcBeamDesc}
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "cfm.h"\nint main(){' +
                   "".join('printf("%s %%zu\\n", sizeof(%s));' % (n, n) for n in structs) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for n, cls in structs.items():
        assert int(out[n]) == ctypes.sizeof(cls), (n, out[n], ctypes.sizeof(cls))
    lib = cfm.lib()
    for name in ("cfm_ctc_topk", "cfm_ctc_greedy", "cfm_ctc_prefix_beam", "cfm_ctc_beam_nodes"):
        assert hasattr(lib, name), name
    assert lib.cfm_ctc_beam_nodes(3, 49, 4) == 3 * 4 * 50


def test_argument_errors_fail_before_any_launch(cfm):
    """Null buffers, k / beam outside 1..16, blank outside [0, V) and a short node buffer are refused on the host (no GPU needed to see it)."""
    lib = cfm.lib()
    err = lambda: lib.cfm_last_error().decode()
    assert lib.cfm_ctc_topk(None, 8, 1, 1, 5, None, 1, None, None, None, None) != 0 and "null" in err()
    p = ctypes.c_void_p(64)                                                             # a made-up address: never dereferenced
    for k in (0, 17, 6):
        assert lib.cfm_ctc_topk(p, 8, 1, 1, 5, p, k, p, p, p, None) != 0 and "k=%d" % k in err()
    d = cfm.CtcGreedyDesc()
    assert lib.cfm_ctc_greedy(ctypes.byref(d), None) != 0 and "null" in err()
    for f in ("idx", "logp", "lens", "prev", "hyps", "count", "frames", "token_logp", "overflow"):
        setattr(d, f, 64)
    d.ld_k, d.B, d.T, d.V, d.hyp_cap, d.hyp_ld = 1, 1, 1, 5, 4, 4
    for blank in (-1, 5):
        d.blank = blank
        assert lib.cfm_ctc_greedy(ctypes.byref(d), None) != 0 and "blank" in err()
    e = cfm.CtcBeamDesc()
    assert lib.cfm_ctc_prefix_beam(ctypes.byref(e), None) != 0 and "null" in err()
    for f in ("idx", "logp", "lens", "nodes", "nbest_tokens", "nbest_len", "nbest_score"):
        setattr(e, f, 64)
    e.B, e.T, e.V, e.k, e.blank, e.n_nodes = 2, 9, 5, 4, 0, 1000
    for beam in (0, 17):
        e.beam = beam
        assert lib.cfm_ctc_prefix_beam(ctypes.byref(e), None) != 0 and "beam=%d" % beam in err()
    e.beam, e.blank = 4, 5
    assert lib.cfm_ctc_prefix_beam(ctypes.byref(e), None) != 0 and "blank" in err()
    e.blank, e.n_nodes = 0, 2 * 4 * 10 - 1
    assert lib.cfm_ctc_prefix_beam(ctypes.byref(e), None) != 0 and "node buffer" in err()


def test_new_methods_raise_on_cpu_tensors_and_in_train_mode(cfm):
    import decoder
    head = decoder.CTCDecoder(7, 16, 0.0)
    x, n = torch.zeros(2, 5, 16), torch.tensor([5, 3], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="eval-mode"):
        head.train().greedy_search(x, n)
    with pytest.raises(RuntimeError, match="eval-mode"):
        head.train().prefix_beam_search(x, n, beam=3)
    head.eval()
    with pytest.raises(RuntimeError, match="no CPU path"):
        head.greedy_search(x, n)
    with pytest.raises(RuntimeError, match="no CPU path"):
        head.prefix_beam_search(x, n, beam=3)
    stream = decoder.CTCGreedyStream(head, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        stream.decode(x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        stream.reset()
    with pytest.raises(RuntimeError, match="eval-mode"):
        decoder.CTCGreedyStream(head.train(), 2).decode(x)
    idx, lp = torch.zeros((2, 5, 1), dtype=torch.int32), torch.zeros((2, 5, 1))
    for call in (lambda: cfm.ctc_topk(torch.zeros(2, 5, 8), 7, n, 1), lambda: cfm.ctc_greedy(idx, lp, n, 7), lambda: cfm.ctc_prefix_beam(idx, lp, n, 7)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()


def test_recognisers_refuse_a_ctc_head_of_the_wrong_width(cfm):
    import decoder
    import encoder
    import greedy_ref as R
    import transducer
    enc = encoder.ConformerEncoder(80, 15, 16, 0.0, 0.0, 0.0, 32, 2, 1, use_relative=True).eval()
    pred, jn = R.modules(9, 16, 16, 16, 16, 1, 3, enc_dim=16, shaped=True)
    with pytest.raises(ValueError, match="CTC head reads 24"):
        transducer.OfflineRecognizer(enc, pred, jn, ctc=decoder.CTCDecoder(9, 24, 0.0))
    with pytest.raises(ValueError, match="CTC head reads 24"):
        transducer.StreamingRecognizer(enc, pred, jn, 2, 4, 2, ctc=decoder.CTCDecoder(9, 24, 0.0))
    rec = transducer.OfflineRecognizer(enc, pred, jn, ctc=decoder.CTCDecoder(9, 16, 0.0))
    assert rec.ctc is not None
    with pytest.raises(RuntimeError, match="without a CTC head"):
        transducer.OfflineRecognizer(enc, pred, jn).recognize_ctc(torch.zeros(1, 20, 80), torch.tensor([20]))
