"""GPU: cfm_rowchain -- every instance of its dispatch, called on its own with the descriptor csrc/encoder.cpp builds for it -- against the float64
restatement of tests/rowchain_ref.py.

Bound.  Per row, never over the tensor: |out - ref| <= g * max_n |ref[m, .]|, plus one ulp of a 16-bit output at the reference value (double rounding).
g is not a constant: rowchain_ref.measure_g evaluates the same formula in plain float32 torch at these very cases and g = 4 x the worst ratio it finds,
separately per kind of output (rowchain_ref.kind): f32 outputs with no rounded intermediate in front of them, and the f32 and the 16-bit outputs behind
one, per weight type -- there the yardstick now and then rounds a 16-bit intermediate (xn, the hidden tile, y2, the depthwise rows) the other way than
float64 does, and so does a kernel: its MFMA sums differ from torch's in order, not in kind.  g is never measured from the kernel.  The module prints
yardstick / kernel / bound (pytest -s); DESIGN.md holds the figures of the run that introduced it.
Exact (torch.equal): a row with head_mask == 0 keeps the residual's bits; a row with ln_mask == 0 gives the tail what a zero xn row gives; GLU rows at
or past glu_len are zero; a second call gives the same bits; tail_pair = 1 and 0 give the same bits.  Every operand lies between guard bands
(tests/extent.py): NaN round inputs, 0xA5 round outputs, outputs pre-filled with NaN, inputs unchanged afterwards, psum_out a workspace of 2 M D floats.
Every call runs under the profiler and must be the one kernel rowchain_ref.INSTANCES names; the last test holds the names reached against that table.

Shapes (rowchain_ref.M_PLAIN, M_PAIR, BT): a tile is 32 rows -- M = 1, 31, 32, 33, 65; the paired instances' groups of 8 workgroups (4 tiles x 2 halves):
1 (six idle workgroups), 33, 128 (one group), 129 (a second group for one row); rows [B, T] for the depthwise stage, cin_* and glu_len: (3,7) a halo over
whole utterances, (5,13) utterance edges inside tiles, (3,41) a ragged last tile, (1,100) halos between full tiles.  What each wrong kernel would fail
is shown on the CPU: tests/test_rowchain_ref_cpu.py::test_every_wrong_variant_is_separated.
"""
import ctypes
from types import SimpleNamespace

import pytest
import torch

import rowchain_ref as R
from extent import Guards
from test_ops_gpu import cfm  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu

WORST = dict.fromkeys(R.KINDS, 0.0)      # kernel per-row ratio per kind of output (16 bit: beyond one ulp), printed by test_report_worst_ratios
REACHED = set()                          # profiler names this module's calls ran under
PAIR_DIFFERS = []                        # (case, what): where tail_pair = 1 and 0 did not give the same bits
_PACKS = {}


def packed(w, dtype):
    """the fragment-major pack of a (cached, never written) natural matrix."""
    k = (w.data_ptr(), dtype)
    if k not in _PACKS:
        _PACKS[k] = (w, R.frag_major(w.float(), dtype))
    return _PACKS[k][1]


def launch(cfm, d):
    """cfm_rowchain under the profiler -> (status, the profiler names that ran).  A device error ends the session: nothing more is launched on a device that
    has faulted."""
    cfm.prof_reset()
    cfm.prof_enable(True)
    try:
        rc = cfm.lib().cfm_rowchain(ctypes.byref(d), cfm.stream())
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("device error behind cfm_rowchain, nothing more is launched: %s" % e, returncode=3)
    finally:
        cfm.prof_enable(False)
    return rc, set(cfm.prof_table())


def run(cfm, p):
    """one cfm_rowchain call on guarded operands -> namespace(dev {field: device view}, G, seen: the profiler names that ran)."""
    dt = R.W_DT[p.wdt]
    G = Guards()
    dev = {}
    shared = set(p.alias.values())
    for name in R.INPUTS:
        t = getattr(p, name)
        if t is None:
            continue
        if name in R.MATRICES:
            t = packed(t, dt)
        dev[name] = (G.io if name in shared else G.inp)(t.contiguous(), name=name)
    for name in p.outputs:
        if name in p.alias:
            continue
        if name == "psum_out":
            dev[name] = G.ws(2 * p.M * p.D, name="psum_out").view(2, p.M, p.D)
        elif name == "tail_out":
            dev[name] = G.out((p.M, p.tail_N // 2 if p.tail_glu else p.tail_N), dt, name=name)
        else:
            dev[name] = G.out((p.M, p.D), dt if name == "out16" else torch.float32, name=name)
    for name, target in p.alias.items():
        dev[name] = dev[target]
    d = R.fill_desc(cfm, p, dev)
    rc, seen = launch(cfm, d)
    assert rc == 0, "cfm_rowchain -> %d: %s" % (rc, cfm.lib().cfm_last_error())
    return SimpleNamespace(dev=dev, G=G, seen=seen)


def within(got, ref, g, dtype, what, kind):
    """the per-row bound on every element (an element the kernel did not write is NaN and fails)."""
    err = (got.cpu().double() - ref).abs()
    u = R.ulp(ref, dtype)
    bound = g * R.row_scale(ref) + u
    bad = ~(err <= bound)
    s = R.row_scale(ref).expand_as(err)
    live = (s > 0) & torch.isfinite(err)
    if bool(live.any()):
        WORST[kind] = max(WORST[kind], float(((err - u).clamp_min(0)[live] / s[live]).max()))
    if bool(bad.any()):
        i = torch.nonzero(bad)[0].tolist()
        raise AssertionError("%s: %d elements over the bound, first at %s: got %r, reference %.9g, bound %.3g (g = %.3g)"
                             % (what, int(bad.sum()), i, float(got[tuple(i)]), float(ref[tuple(i)]), float(bound[tuple(i)]), g))


def check(cfm, key):
    """run the case, hold every output to the reference, the exact rows and the guard bands; -> the result."""
    case, D, wdt, rows = key
    p, r = R.problem(*key), R.reference(key)
    G = R.measure_g()
    what = "%s D=%d %s %s" % (case, D, wdt, "x".join(map(str, rows)))
    o = run(cfm, p)
    assert o.seen == {R.instance(case, D, wdt)}, (what, o.seen)
    REACHED.update(o.seen)
    for buf, name in p.compare:
        k = R.kind(p, name)
        within(o.dev[buf], r[name], G[k][0], R.out_dtype(p, name), what + " " + name, k)
    o.G.check()
    again = run(cfm, p)
    for buf, name in p.compare:
        assert torch.equal(again.dev[buf], o.dev[buf]), what + " " + name + ": a second call gives other bits"
    if p.head_mask is not None and p.w1f is None and "out_f32" in p.outputs:        # the rows themselves are an output: x = head_res + 0
        dead = (p.head_mask == 0).cuda()
        buf = p.alias.get("out_f32", "out_f32")
        assert torch.equal(o.dev[buf][dead], p.head_res.cuda()[dead]), what + ": a row with head_mask == 0 does not keep the residual's bits"
    if p.glu_len is not None and p.tail_glu:
        dead = R.glu_dead(p).cuda()
        assert bool((o.dev["tail_out"][dead] == 0).all()), what + ": a GLU row at or past glu_len is not zero"
    if p.ln_mask is not None and p.tail_w is not None:
        # LayerNorm with gain 0 and bias 0 makes every xn row zero: what the tail gives a zero row, from the kernel itself
        q = SimpleNamespace(**vars(p))
        q.ln_g, q.ln_b, q.ln_mask = torch.zeros(D), torch.zeros(D), None
        z = run(cfm, q)
        dead = (p.ln_mask == 0).cuda()
        assert torch.equal(o.dev["tail_out"][dead], z.dev["tail_out"][dead]), what + ": a row with ln_mask == 0 differs from a zero xn row"
    return o


def sweep(cfm, case, wdt):
    Ds, _, kind = R.INSTANCES[case]
    for D in Ds:
        for rows in R.ROWS[kind]:
            check(cfm, (case, D, wdt, rows))


# ---------------------------------------------------------------------------------------------------------------- the matrix
@pytest.mark.parametrize("wdt", ["bf16", "fp16"])
@pytest.mark.parametrize("case", sorted(R.INSTANCES))
def test_case_against_float64(cfm, case, wdt):
    """one descriptor of csrc/encoder.cpp at every width that has it and every row count of its kind."""
    sweep(cfm, case, wdt)


@pytest.mark.parametrize("wdt", ["bf16", "fp16"])
def test_tail_pair_changes_no_bit(cfm, wdt):
    """the q|k|v chain behind the reduce and the conv-in chain at D = 512: rows and tail with the tail's columns over a workgroup pair == one workgroup per
    tile.  Where they differ both are still held to the reference (test_case_against_float64) and the difference is reported, not asserted away."""
    for case in ("pair_qkv", "pair_convin", "pair_convin_len"):
        for rows in R.ROWS[R.INSTANCES[case][2]]:
            p = R.problem(case, 512, wdt, rows)
            q = SimpleNamespace(**vars(p))
            q.tail_pair = 0
            a, b = run(cfm, p), run(cfm, q)
            assert len(a.seen) == 1 and len(b.seen) == 1 and a.seen != b.seen, (a.seen, b.seen)
            for buf, name in p.compare:
                if not torch.equal(a.dev[buf], b.dev[buf]):
                    PAIR_DIFFERS.append((case, wdt, rows, name, float((a.dev[buf].double() - b.dev[buf].double()).abs().max())))
    assert not PAIR_DIFFERS, PAIR_DIFFERS


def refused(cfm, p, status, **change):
    """the descriptor with `change` applied is refused with `status` before anything is launched."""
    q = SimpleNamespace(**vars(p))
    q.alias = dict(p.alias)
    for k, v in change.items():
        setattr(q, k, v)
    dt = R.W_DT[p.wdt]
    dev = {n: (packed(getattr(q, n), dt) if n in R.MATRICES else getattr(q, n)).cuda() for n in R.INPUTS if getattr(q, n) is not None}
    for name in q.outputs:
        if name not in q.alias:
            dev[name] = torch.zeros((2 * q.M if name == "psum_out" else q.M, max(q.tail_N, q.D)), dtype=dt if name in R.OUT16 else torch.float32, device="cuda")
    for name, target in q.alias.items():
        dev[name] = dev[target]
    d = R.fill_desc(cfm, q, dev)
    rc, seen = launch(cfm, d)
    assert rc == status and not seen, (rc, seen, change)


def test_argument_errors(cfm):
    """CFM_ERR_ARG (-1) or CFM_ERR_UNSUPPORTED (-3), not a launch."""
    p = R.problem("pair_convin", 512, "bf16", (33,))
    refused(cfm, p, -1, alias={"out_f32": "head_res"})                         # tail_pair: out_f32 must not alias head_res
    refused(cfm, p, -1, D=256, tail_N=512)                                     # tail_pair away from D = 512
    p = R.problem("convin_len", 256, "bf16", (5, 13))
    refused(cfm, p, -1, glu_T=12)                                              # M % glu_T != 0
    refused(cfm, p, -1, glu_T=0)
    refused(cfm, p, -1, tail_glu=0)                                            # glu_len without a GLU
    p = R.problem("pair_qkv", 512, "bf16", (33,))
    refused(cfm, p, -1, psum_b2=None)
    p = R.problem("pair_macaron_half", 512, "bf16", (33,))
    refused(cfm, p, -1, ln1_g=R.weights(512, "bf16").ln_final[0], ln1_b=R.weights(512, "bf16").ln_final[1])      # psum_out takes no post norm
    p = R.problem("cin", 256, "bf16", (5, 13))
    refused(cfm, p, -1, cin_mask=None, cin_ln_g=None)                          # an operand of the stage missing
    refused(cfm, p, -1, glu_T=7)
    p = R.problem("dwfinal", 256, "bf16", (5, 13))
    refused(cfm, p, -1, dw_T=12)                                               # M % dw_T != 0
    refused(cfm, p, -1, dw_K=7)
    p = R.problem("macaron", 256, "bf16", (33,))
    refused(cfm, p, -1, D=128)
    refused(cfm, p, -3, tail_N=512)                                            # no instance with this tail
    torch.cuda.synchronize()


def test_every_instance_was_reached(cfm):
    """every name of rowchain_ref.INSTANCES -- the names of csrc/rowchain.hip, by tests/test_rowchain_ref_cpu.py -- ran in this module, for both weight types."""
    for case, (Ds, _, kind) in R.INSTANCES.items():                             # (run on its own: make the calls, at the smallest row count of each case)
        for D in Ds:
            for wdt in R.TAG:
                if R.instance(case, D, wdt) not in REACHED:
                    check(cfm, (case, D, wdt, R.ROWS[kind][0]))
    assert REACHED == R.instance_names(), sorted(R.instance_names() - REACHED)


def test_report_worst_ratios(cfm):
    """not a check of its own: prints what the module measured (pytest -s), the figures DESIGN.md quotes."""
    G = R.measure_g()
    print("\nper-row |d| / max|ref| (16-bit outputs: beyond one ulp)   float32 torch   kernel   bound g")
    for k in R.KINDS:
        print("%-12s %.3g   %.3g   %.3g" % (k, G[k][1], WORST[k], G[k][0]))
    print("tail_pair = 1 against 0: %s" % (PAIR_DIFFERS or "the same bits everywhere"))
