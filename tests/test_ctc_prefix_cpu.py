"""CPU: the float64 CTC prefix scorer and joint search of tests/ctc_prefix_ref.py (the specification of csrc/ctc_prefix.hip and
decoder.JointBeamSearch) against brute-force enumeration of alignments, the oracle's CTC loss, its own recursive form, its no-NaN rules; the joint
search against attention_search_ref.search64 and a peaked CTC head; the clear share the GPU cases claim; and the host layer's argument errors."""
import itertools
import math

import numpy as np
import pytest
import torch

import attention_search_ref as SR
import ctc_prefix_ref as CP
from test_attention_search_cpu import small, string_score

NEG = float("-inf")
BLANK, EOS = 0, 3


def collapse(path, blank=BLANK):
    out, prev = [], None
    for c in path:
        if c != prev and c != blank:
            out.append(c)
        prev = c
    return tuple(out)


def lse(values):
    values = [v for v in values if v > NEG]
    if not values:
        return NEG
    m = max(values)
    return m + math.log(sum(math.exp(v - m) for v in values))


def rand_x(T, V, seed):
    return CP.log_softmax(np.random.RandomState(seed).standard_normal((T, V)) * 2.0)


@pytest.mark.parametrize("T", [1, 2, 3, 5])
def test_specification_against_brute_force(T):
    V = 4                                                        # blank 0, the tokens 1 and 2, eos 3 (a class of x like any other, never a label)
    x = rand_x(T, V, 40 + T)
    paths = list(itertools.product(range(V), repeat=T))
    mass = {p: float(sum(x[t, c] for t, c in enumerate(p))) for p in paths}
    strings = [g for L in range(4) for g in itertools.product((1, 2), repeat=L)]      # every g up to length 3, repeated tokens included
    assert len(strings) == 15
    close = lambda a, b: (a == NEG and b == NEG) or abs(a - b) <= 1e-12
    for g in strings:
        st = CP.state_of(x, g, BLANK)
        prefix = lse(m for p, m in mass.items() if collapse(p)[:len(g)] == g)
        exact = lse(m for p, m in mass.items() if collapse(p) == g)
        assert close(float(st.psi), prefix), (T, g, float(st.psi), prefix)                # psi(g): the output starts with g
        if g:
            assert close(float(CP.psi_ext(x, CP.state_of(x, g[:-1], BLANK), g[-1], BLANK, EOS)), prefix), (T, g)
        assert close(float(CP.psi_ext(x, st, EOS, BLANK, EOS)), exact), (T, g)             # psi(g.eos): the output is exactly g
        for t in range(T):                                        # the state: frames 0..t, exactly g, by ending symbol
            heads = {h: float(sum(x[k, c] for k, c in enumerate(h))) for h in itertools.product(range(V), repeat=t + 1)}
            want_n = lse(m for h, m in heads.items() if collapse(h) == g and g and h[-1] == g[-1])
            want_b = lse(m for h, m in heads.items() if collapse(h) == g and h[-1] == BLANK)
            assert close(float(st.gn[t]), want_n) and close(float(st.gb[t]), want_b), (T, g, t)


def test_eos_is_the_ctc_likelihood_of_the_oracle():
    from oracle import conformer_oracle as O
    x = rand_x(12, 17, 3)
    for g in ((), (5,), (5, 5), (1, 2, 3, 3, 9), (16, 4, 4, 4)):
        st = CP.state_of(x, g, BLANK)
        assert abs(float(CP.psi_ext(x, st, 16, BLANK, 16)) + O.ctc_nll(x, list(g), BLANK)) <= 1e-10, g


def test_reduction_form_equals_the_recursive_form():
    x = rand_x(12, 17, 4)
    for g in ((), (5,), (5, 5), (1, 2, 3), (7, 7, 7, 2)):
        st = CP.state_of(x, g, BLANK)
        for c in range(1, 16):
            red, rec = float(CP.psi_ext(x, st, c, BLANK, 16)), float(CP.extend(x, st, c, BLANK).psi)
            assert abs(red - rec) <= 1e-12 * (1 + abs(red)), (g, c, red, rec)


def test_no_nan():
    x = rand_x(3, 5, 5)
    st = CP.state_of(x, (1, 1, 2), BLANK)                          # needs 4 frames: impossible in 3
    assert st.psi == NEG and not np.isnan(st.gn).any() and not np.isnan(st.gb).any()
    for c in range(5):
        p = CP.psi_ext(x, st, c, BLANK, 4)
        d = CP.delta(p, st.psi)
        assert p == NEG and d == NEG and CP.offer(-1.0, d, 0.3) == NEG and CP.offer(-1.0, d, 1.0) == NEG
        nxt = CP.extend(x, st, c, BLANK)
        assert nxt.psi == NEG and not np.isnan(nxt.gn).any() and not np.isnan(nxt.gb).any()
    ok = CP.state_of(x, (1,), BLANK)
    assert CP.psi_ext(x, ok, BLANK, BLANK, 4) == NEG and CP.delta(CP.psi_ext(x, ok, BLANK, BLANK, 4), ok.psi) == NEG
    blank_state = CP.extend(x, ok, BLANK, BLANK)
    assert blank_state.psi == NEG and bool((blank_state.gn == NEG).all()) and bool((blank_state.gb == NEG).all())
    assert CP.delta(-1.0, NEG) == NEG and CP.delta(NEG, NEG) == NEG and np.isfinite(CP.delta(-2.0, -1.0))
    x32 = x.astype(np.float32)                                     # the float32 run of the same code keeps its type and the rules
    s32 = CP.state_of(x32, (1, 1, 2), BLANK)
    assert s32.gn.dtype == np.float32 and s32.psi == NEG and CP.psi_ext(x32, CP.state_of(x32, (1,), BLANK), 2, BLANK, 4).dtype == np.float32


def _kept_sets(P, memory, n, beam, H, eos, steps):
    """What search64 keeps after 1 .. steps steps (eos out of reach: the search with max_len = m stops with the kept set of step m)."""
    return [[t for t, _, _ in SR.search64(P, memory, n, beam, H, eos, eos, max_len=m)["nbest"]] for m in range(1, steps + 1)]


def test_uniform_ctc_head_returns_the_attention_search():
    """x uniform: x[t, c] = -log V.  psi(h) is then log(#alignments that start with h) - n log V, and for a string WITHOUT adjacent repeats that
    count depends on its length and n alone (a repeat needs a blank between its two tokens, so it has fewer alignments and a smaller psi).  With eos
    out of reach every candidate of a step has the same length, so every repeat-free candidate gets the same delta(step, n): the combined offers are
    (1 - lam) x the attention ones plus a constant and order as in search64; a candidate with a repeat only moves down, and class 0, an ordinary
    token to search64, is the blank here and is never offered.  So where search64 keeps no string with an adjacent repeat or a class 0 at any step
    -- asserted -- the joint search with pre_beam = V keeps the same strings in the same order, and its
    score is (1 - lam) x search64's + lam x psi(string) (the increments telescope)."""
    V, n, beam, steps, lam = 9, 7, 3, 3, 0.4
    dec, P, memory, H = small(V, 39, eos_bias=-30.0)
    eos = V - 1
    kept = _kept_sets(P, memory, n, beam, H, eos, steps)
    assert all(a != b for m in kept for t in m for a, b in zip(t, t[1:])) and all(BLANK not in t for m in kept for t in m), kept      # the derivation's precondition
    x = np.full((n, V), -math.log(V))
    ref = SR.search64(P, memory, n, beam, H, eos, eos, max_len=steps)
    got = CP.joint_search64(P, memory, n, x, beam, H, eos, eos, lam, pre_beam=V, blank=BLANK, max_len=steps)
    assert [t for t, _, _ in got["nbest"]] == [t for t, _, _ in ref["nbest"]] and not any(f for _, _, f in got["nbest"])
    for (t, s, _), (_, s_att, _) in zip(got["nbest"], ref["nbest"]):
        assert abs(s - ((1 - lam) * s_att + lam * float(CP.state_of(x, t, BLANK).psi))) <= 1e-10


def test_peaked_ctc_head_pulls_the_best_path_in():
    V, n, beam, lam = 9, 6, 3, 0.7
    dec, P, memory, H = small(V, 5, eos_bias=3.0)
    eos = V - 1
    att_only = SR.search64(P, memory, n, beam, H, eos, eos)["nbest"][0][0]
    frames = [4, 4, 0, 2, 0, 0]                                    # the best path collapses to (4, 2)
    want = (4, 2)
    assert att_only != want
    probs = np.full((n, V), 1e-4 / (V - 1))
    for t, c in enumerate(frames):
        probs[t, c] = 1.0 - 1e-4
    got = CP.joint_search64(P, memory, n, np.log(probs), beam, H, eos, eos, lam, pre_beam=V, blank=BLANK)
    tokens, score, fin = got["nbest"][0]
    assert tokens == want and fin
    # the score of a finished string is (1 - lam) x the attention decoder's + lam x the CTC log-likelihood
    ctc_ll = float(CP.psi_ext(np.log(probs), CP.state_of(np.log(probs), want, BLANK), eos, BLANK, eos))
    assert abs(score - ((1 - lam) * string_score(P, memory, n, H, want, eos) + lam * ctc_ll)) <= 1e-10


def test_search_edge_cases():
    V = 9
    dec, P, memory, H = small(V, 9, eos_bias=-30.0)
    x = rand_x(7, V, 6)
    assert CP.joint_search64(P, memory, 0, x, 4, H, 8, 8, 0.3)["nbest"] == [((), 0.0, True)]
    res = CP.joint_search64(P, memory, 7, x, 3, H, 8, 8, 0.3, max_len=2)
    assert res["steps"] == 2 and all(len(t) == 2 and not f for t, _, f in res["nbest"])      # cut off: returned unfinished
    assert CP.default_pre_beam(10, 5002) == 15 and CP.default_pre_beam(16, 17) == 16 and CP.default_pre_beam(1, 17) == 2 and CP.default_pre_beam(4, 5) == 5
    one = CP.joint_search64(P, memory, 1, x, 3, H, 8, 8, 1.0, pre_beam=9)                      # one frame, CTC alone: a token, or nothing
    assert all(len(t) <= 1 for t, _, _ in one["nbest"]) and all(s > NEG for _, s, _ in one["nbest"])


# The table of claims lives beside the cases: ctc_prefix_ref.GPU_CASES, column 10.
@pytest.mark.parametrize("case", CP.GPU_CASES, ids=[c[0] for c in CP.GPU_CASES])
def test_gpu_cases_are_clear_under_the_modes_they_claim(case):
    """The float64 joint search ALONE: at least half of each case's utterances are clear at TWICE the delta of every mode the case claims (the rule
    of test_attention_search_cpu.py); the other modes' shares are printed."""
    res = CP.reference(case)
    B = case[1]
    assert "fp32" in case[10]
    for mode in CP.MODES:
        ds, gate, gate_att = CP.deltas(mode, case)
        n1 = sum(CP.clear(r, d, da) for r, (d, da) in zip(res, ds))
        n2 = sum(CP.clear(r, 2 * d, 2 * da) for r, (d, da) in zip(res, ds))
        print("%s %s: per-position gate %.2e (attention alone %.2e), clear %d of %d (at twice the delta: %d)%s" % (
            case[0], mode, gate, gate_att, n1, B, n2, "" if mode in case[10] else " -- not claimed"))
        if mode in case[10]:
            assert 2 * n2 >= B, (case[0], mode, n1, n2)
    assert any(f for r in res for _, _, f in r["nbest"]) or case[6] is not None            # finished strings, unless the case is the cut-off
    col = lambda i: {c[i] for c in CP.GPU_CASES}
    assert col(1) == {1, 3, 16} and col(2) == {1, 4, 10, 16} and col(4) == {17, 5002} and col(11) == {0.3, 1.0} and all(12 <= c[3] <= 40 for c in CP.GPU_CASES)
    assert any(c[6] is not None for c in CP.GPU_CASES) and any((c[12] or CP.default_pre_beam(c[2], c[4])) == c[2] for c in CP.GPU_CASES)
    assert all(any(m in c[10] for c in CP.GPU_CASES) for m in CP.MODES)                   # every mode is claimed somewhere


@pytest.mark.parametrize("case", CP.GPU_CASES, ids=[c[0] for c in CP.GPU_CASES])
def test_gpu_cases_keep_the_score_bound_under_emulated_rounding(case):
    """The GPU protocol bounds the sorted scores of every utterance by delta, clear or not.  That is a property of the case, not of beam search, so the
    cases are chosen to have it: the search in float32 on weights rounded as each mode rounds them stays within delta of the float64 one."""
    for mode in CP.MODES:
        ratio = CP.emulated(mode, case)
        print("%s %s: emulated worst sorted-score error / delta %.3f" % (case[0], mode, ratio))
        assert ratio <= 0.5, (case[0], mode, ratio)                # half the bound: room for the device's own arithmetic


def test_bindings_and_argument_errors():
    import cfm
    import decoder
    import transducer
    names = [p[0] for p in cfm.PROTOTYPES]
    assert all(n in names for n in ("cfm_ctc_logprob_t", "cfm_ctc_prefix_score", "cfm_ctc_prefix_advance")) and cfm.CtcPrefixDesc._c_name_ == "cfm_ctc_prefix_desc"
    dec = decoder.TransformerDecoder(9, 16, 2, 32, 1, 0.0, 0.0, 0.0, 0.0).eval()
    ctc = decoder.CTCDecoder(9, 16, 0.0).eval()
    for kw in (dict(ctc_weight=0.0), dict(ctc_weight=1.5), dict(ctc_weight=-0.1), dict(pre_beam=3), dict(pre_beam=10), dict(pre_beam=17), dict(blank=8), dict(blank=9),
               dict(beam=17), dict(beam=10)):                                            # pre_beam in beam .. min(16, V = 9); blank != eos = 8; beam <= V
        with pytest.raises(ValueError):
            decoder.JointBeamSearch(dec, ctc, **dict(dict(beam=4), **kw))
    with pytest.raises(ValueError, match="classes"):
        decoder.JointBeamSearch(dec, decoder.CTCDecoder(10, 16, 0.0).eval(), beam=4)
    with pytest.raises(TypeError):
        decoder.JointBeamSearch(dec, torch.nn.Linear(16, 9), beam=4)
    js = decoder.JointBeamSearch(dec, ctc, beam=4)
    assert js.pre_beam == 6 and decoder.JointBeamSearch(dec, ctc, beam=8).pre_beam == 9 and decoder.JointBeamSearch(dec, ctc, beam=4, ctc_weight=1.0).ctc_weight == 1.0
    with pytest.raises(RuntimeError, match="no CPU path"):
        js.search(torch.zeros(2, 3, 16), [3, 2])
    for m in (dec, ctc):
        m.train()
        with pytest.raises(RuntimeError, match="eval-mode"):
            js.search(torch.zeros(2, 3, 16), [3, 2])
        m.eval()
    with pytest.raises(RuntimeError, match="no CPU path"):
        cfm.ctc_logprob_t(torch.zeros(2, 3, 12), 9, torch.ones(2, dtype=torch.int32))
    S = dict(token=torch.zeros(4, dtype=torch.int32), hlen=torch.zeros(4, dtype=torch.int32), finished=torch.zeros(4, dtype=torch.uint8), step=torch.zeros(2, dtype=torch.int32),
             done=torch.zeros(2, dtype=torch.uint8), lens=torch.ones(2, dtype=torch.int32), parent=torch.zeros(4, dtype=torch.int32), tokens=torch.zeros(4, 3, dtype=torch.int32))
    x, st, psi = torch.zeros(2, 9, 4), torch.zeros(2, 4, 4, 2), torch.zeros(4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        cfm.ctc_prefix_score(x, 3, st, psi, torch.zeros(4, 3, dtype=torch.int32), torch.zeros(4, 3), S, 2, 0.3, 0, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        cfm.ctc_prefix_advance(x, 3, st, psi, S, 2, 0, 8)

    # the recogniser: both heads are needed
    import encoder
    import greedy_ref as R
    enc = encoder.ConformerEncoder(80, 15, 16, 0.0, 0.0, 0.0, 32, 2, 1, use_relative=True).eval()
    pr, jn = R.modules(9, 16, 16, 16, 16, 1, 7)
    feats, lens = torch.zeros(1, 50, 80), torch.tensor([50], dtype=torch.int32)
    for kw, what in ((dict(attention=dec), "without a CTC head"), (dict(ctc=ctc), "without an attention decoder")):
        rec = transducer.OfflineRecognizer(enc, pr, jn, **kw)
        with pytest.raises(RuntimeError, match=what):
            rec.recognize_joint(feats, lens, beam=4)
        with pytest.raises(RuntimeError, match=what):
            rec.recognize_joint_audio(torch.zeros(1, 8000), torch.tensor([8000]), beam=4)
    with pytest.raises(ValueError, match="reverse_weight"):
        transducer.OfflineRecognizer(enc, pr, jn, ctc=ctc, attention=dec).recognize_joint(feats, lens, beam=4, rescore=True)
