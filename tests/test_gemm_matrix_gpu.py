"""GPU: cfm_gemm -- every tile id, operand type, output type and epilogue -- against the float64 restatement of tests/gemm_ref.py.

Bound.  Per element, never a matrix norm: |out - ref| <= g * S with S = sum_k |a||w| + |bias| of that element (GLU: of its value column), plus
one ulp of a 16-bit output at the reference value (double rounding).  g is not a constant: gemm_ref.measure_g evaluates the same formula
in plain float32 torch on the same rounded operands at these very cases (K up to 2048) and g = 4 x the worst ratio it finds; split mode
(W_lo) is measured the same way, the float32 yardstick being the header's three-product formula against the float64 product of the
unrounded operands.  The module prints torch / kernel / bound (pytest -s); DESIGN.md holds the figures of the run that introduced it.
Exact (torch.equal): mask_mode 0 and row_len rows are 0 or the residual's bits; mask_mode 1 rows equal the same call on a zeroed A row; an
out-of-place C leaves the residual alone; columns [N, ldc) and the padding of C_pre keep their fill; ids 1-8 give the same bits.

Shapes (gemm_ref.SHAPE_*): 130 x 132 x 72 (a full 128 tile + 2 rows, N past 128 and no multiple of 16, a K tail), 1 x 8 x 8, 33 x 160 x 136 (GLU:
N % 32 == 0 across 64 and 128), 77 x 132 x 1096 (K groups: 18 K tiles, 9 / 5 per group, the last group's partly past K), 129 x 70 x 64 with
ldc = 70 (pair stores), 150 x 160 x 136 as 3 utterances of 50 rows with lengths 50 / 17 / 0, two convolutions.  What each wrong kernel would
fail is shown on the CPU: tests/test_gemm_ref_cpu.py::test_every_wrong_variant_is_separated.
"""
import ctypes
import functools
from types import SimpleNamespace

import pytest
import torch

import gemm_ref as R
from test_ops_gpu import cfm  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu

TILED, KGROUP = (1, 2, 3, 4, 5, 6), (9, 10, 11)
TILE_NAME = {1: "128x128", 2: "64x128", 3: "64x64", 4: "128x64", 5: "32x64", 6: "32x128", 7: "persistent_128x128", 8: "256x256",
             9: "32x64_k2", 10: "64x64_k4", 11: "64x64_k2"}
NEEDS_F32_OUT = ("res", "res_inplace", "mask0_res", "drop2", "glu_mask0", "mask0_relu_res")
WORST = {"f32": 0.0, "16bit": 0.0, "split": 0.0}      # kernel |d| / S (16 bit: (|d| - ulp) / S), printed by test_report_worst_ratios


def to_dev(t):
    """a CPU tensor -> device, keeping the row stride of a padded view (its other columns hold gemm_ref.FILL)."""
    if t is None:
        return None
    if t.is_contiguous():
        return t.cuda()
    buf = torch.full((t.shape[0], t.stride(0)), R.FILL, dtype=t.dtype, device="cuda")
    buf[:, :t.shape[1]] = t.cuda()
    return buf[:, :t.shape[1]]


@functools.lru_cache(maxsize=None)
def dev_inputs(key, poison=False):
    """the problem's inputs on the device, made once and never written to (an in-place call works on a clone of the residual)."""
    p = R.poisoned(key)[0] if poison else R.problem(*key)
    return SimpleNamespace(A=to_dev(p.A), W=p.W.cuda(), W_lo=to_dev(p.W_lo), bias=to_dev(p.bias), residual=to_dev(p.residual), row_mask=to_dev(p.row_mask),
                           aux=to_dev(p.aux), row_len=to_dev(p.row_len))


def run(cfm, p, d, tile, A=None, row_mask="same"):
    """one cfm.gemm call -> namespace(out, out_buf, pre, pre_buf, residual): out / pre are views of FILL-ed buffers of row stride ldc / ld_pre."""
    n_out = p.N // 2 if p.act == R.ACT_GLU else p.N
    res = d.residual
    if p.inplace:
        res = to_dev(p.residual)
        out_buf, out = res, res
    else:
        out_buf = torch.full((p.M, p.ldc), R.FILL, dtype=p.c_dtype, device="cuda")
        out = out_buf[:, :n_out]
    pre_buf = pre = None
    if p.pre_dtype is not None:
        pre_buf = torch.full((p.M, p.ld_pre), R.FILL, dtype=p.pre_dtype, device="cuda")
        pre = pre_buf[:, :p.N]
    conv = None if p.conv is None else p.conv + (p.M,)
    cfm.gemm(d.A if A is None else A, d.W, bias=d.bias, w_lo=d.W_lo, out=out, act=p.act, residual=res, alpha=p.alpha,
             row_mask=d.row_mask if isinstance(row_mask, str) else row_mask, mask_mode=p.mask_mode, conv=conv, tile=tile, pre_out=pre, aux=d.aux,
             drop=p.drop, drop2=p.drop2, row_len=d.row_len, row_T=p.row_T)
    return SimpleNamespace(out=out, out_buf=out_buf, pre=pre, pre_buf=pre_buf, residual=res)


def within(got, ref, ref_c, S, g, dtype, what, tag):
    """the per-element bound where the reference and its rounding are finite; elsewhere (NaN, Inf, an overflowed 16-bit output) the same value."""
    got = got.cpu()
    fin = torch.isfinite(ref) & torch.isfinite(ref_c.double())
    assert torch.equal(torch.isnan(got)[~fin], torch.isnan(ref_c)[~fin]) and torch.equal(torch.nan_to_num(got.double())[~fin], torch.nan_to_num(ref_c.double())[~fin]), \
        "%s: non-finite elements differ from the reference" % what
    err = (got.double() - ref).abs()[fin]
    u, s = R.ulp(ref, dtype)[fin], S[fin]
    if err.numel():
        WORST[tag] = max(WORST[tag], float(((err - u).clamp_min(0) / s).max()))
    bad = err > g * s + u
    assert not bool(bad.any()), "%s: %d elements over the bound, worst |d| = %.3g at S = %.3g (g = %.3g, ulp %.3g)" % (
        what, int(bad.sum()), float(err[bad].max()), float(s[bad][err[bad].argmax()]), g, float(u[bad][err[bad].argmax()]))


def check(cfm, key, tile, poison=False):
    """run the problem on `tile` and hold the result to the reference, the exact rows and the fills; -> the result."""
    p = R.poisoned(key)[0] if poison else R.problem(*key)
    r = R.evaluate(p) if poison else R.reference(key)
    d = dev_inputs(key, poison)
    split = p.W_lo is not None
    g = R.measure_g()[1 if split else 0]
    what = "tile %d %s" % (tile, key)
    o = run(cfm, p, d, tile)
    tag = "split" if split else ("f32" if p.c_dtype == R.F32 else "16bit")
    within(o.out, r.out, r.out_c, r.S, g, p.c_dtype, what, tag)
    if o.pre is not None:
        within(o.pre, r.pre, r.pre_c, r.S_pre, g, p.pre_dtype, what + " C_pre", tag if p.pre_dtype == R.F32 else "16bit")
        assert bool((o.pre_buf[:, p.N:] == R.FILL).all()), what + ": C_pre padding written"
    if not p.inplace:
        assert bool((o.out_buf[:, o.out.shape[1]:] == R.FILL).all()), what + ": columns [N, ldc) written"
        if p.residual is not None:
            assert torch.equal(o.residual, to_dev(p.residual)), what + ": residual written by an out-of-place call"
    dead = (~R.rows_kept(p)).cuda()
    if bool(dead.any()) and p.mask_mode == 0:
        want = torch.zeros_like(o.out[dead]) if p.residual is None else to_dev(p.residual)[dead]
        assert torch.equal(o.out[dead], want), what + ": a masked output row is not exactly 0 / the residual"
    if bool(dead.any()) and p.mask_mode == 1 and p.conv is None:
        A0 = d.A.clone()
        A0[dead] = 0
        o0 = run(cfm, p, d, tile, A=A0, row_mask=None)
        assert torch.equal(o.out[dead], o0.out[dead]), what + ": a masked input row differs from a zeroed A row"
    return o


def refused(cfm, key, tile):
    p, d = R.problem(*key), dev_inputs(key)
    with pytest.raises(RuntimeError, match=r"status -1"):
        run(cfm, p, d, tile)


def cross_keys(wdt, a32, c16, pad=False):
    keys = [(R.SHAPE_MAIN, wdt, e, a32, c16, pad) for e in R.EPILOGUES]
    keys += [(R.SHAPE_GLU, wdt, e, a32, c16, pad) for e in R.GLU_EPILOGUES]
    keys += [(R.SHAPE_RAGGED, wdt, e, a32, c16, pad) for e in ("row_len", "row_len_mask")]
    if not pad:
        keys += [(s, wdt, e, a32, c16) for s in (R.SHAPE_ONE, R.SHAPE_PAIR) for e in R.PLAIN]
    return [k for k in keys if not (c16 and k[2] in NEEDS_F32_OUT)]


# ---------------------------------------------------------------------------------------------------------------- the cross
@pytest.mark.parametrize("wdt", ["bf16", "fp16"])
@pytest.mark.parametrize("tile", TILED + KGROUP)
def test_every_epilogue_on_every_tile(cfm, tile, wdt):
    """tile id x weight type: every epilogue the id admits, A in 16 bit and f32, C in f32 and 16 bit, once with every stride padded, and the
    long-K shape whose K tiles do not divide among the K groups."""
    for a32 in (False, True):
        for c16 in (False, True):
            for key in cross_keys(wdt, a32, c16):
                if a32 and tile in KGROUP:
                    if key[2] in ("bias", "glu"):
                        refused(cfm, key, tile)             # K groups take 16-bit operands: CFM_ERR_ARG, nothing runs
                    continue
                check(cfm, key, tile)
    for key in cross_keys(wdt, False, False, pad=True):
        check(cfm, key, tile)
    for e in R.EPILOGUES:
        check(cfm, (R.SHAPE_KG, wdt, e), tile)
    if tile in KGROUP:                                      # the K groups meet in a fixed order: the same bits run to run
        key = (R.SHAPE_KG, wdt, "silu")
        assert torch.equal(check(cfm, key, tile).out, check(cfm, key, tile).out)


@pytest.mark.parametrize("tile", (1, 2, 3, 4))
def test_split_mode(cfm, tile):
    """W_lo (f32 A, bf16 planes) with SiLU / ReLU, residual and both masks, on a plain product and both convolutions."""
    for e in ("bias", "silu", "relu", "mask0_relu_res", "mask1_silu"):
        check(cfm, (R.SHAPE_MAIN, "bf16", e, True, False, False, True), tile)
        check(cfm, ((64, 64, 2048), "bf16", e, True, False, False, True), tile)
        for cv in R.CONVS:
            check(cfm, (R.conv_shape(cv), "bf16", e, True, False, False, True, cv), tile)


@pytest.mark.parametrize("wdt", ["bf16", "fp16"])
@pytest.mark.parametrize("tile", TILED)
def test_conv(cfm, tile, wdt):
    for cv in R.CONVS:
        for e in ("silu", "relu", "mask0_relu_res", "mask1_silu"):
            check(cfm, (R.conv_shape(cv), wdt, e, False, False, False, False, cv), tile)
        check(cfm, (R.conv_shape(cv), wdt, "relu", False, True, False, False, cv), tile)


@pytest.mark.parametrize("wdt", ["bf16", "fp16"])
@pytest.mark.parametrize("tile", (7, 8))
def test_persistent_and_256_against_float64(cfm, tile, wdt):
    for shape in (R.SHAPE_K64, R.SHAPE_PAIR, (64, 64, 2048)):
        for e in R.PLAIN if shape != (64, 64, 2048) else ("silu",):
            for c16 in (False, True):
                if shape == (64, 64, 2048) and c16:
                    continue
                check(cfm, (shape, wdt, e, False, c16), tile)
    if tile == 8:
        check(cfm, (R.conv_shape(R.CONVS[1]), wdt, "relu", False, False, False, False, R.CONVS[1]), tile)


def test_ids_a_mode_does_not_have_are_refused(cfm):
    """CFM_ERR_ARG, not a launch: split mode on 5, 6, 7, 8 and the K groups; conv on 7 and the K groups; f32 A on 7 and 8; epilogues 7 and 8 do not take."""
    for tile in (5, 6, 7, 8) + KGROUP:
        refused(cfm, (R.SHAPE_K64, "bf16", "bias", True, False, False, True), tile)
    cv = R.CONVS[1]
    for tile in (7,) + KGROUP:
        refused(cfm, (R.conv_shape(cv), "bf16", "relu", False, False, False, False, cv), tile)
    for tile in (7, 8):
        refused(cfm, (R.SHAPE_K64, "bf16", "bias", True), tile)
        for e in ("res", "mask1", "pre_silu", "drelu", "drop"):
            refused(cfm, (R.SHAPE_K64, "bf16", e), tile)
        refused(cfm, (R.SHAPE_MAIN, "bf16", "bias"), tile)      # K % 64 != 0
        refused(cfm, (R.SHAPE_GLU, "bf16", "glu"), tile)
    refused(cfm, (R.SHAPE_MAIN, "bf16", "bias"), 12)


# ---------------------------------------------------------------------------------------------------------------- same bits
@pytest.mark.parametrize("wdt", ["bf16", "fp16"])
def test_ids_without_k_groups_give_the_same_bits(cfm, wdt):
    """ids 1-6 on every epilogue, 7 and 8 on the ones they take: torch.equal with id 1 (no choice without K groups changes the K order)."""
    keys = cross_keys(wdt, False, False) + cross_keys(wdt, True, True) + cross_keys(wdt, False, False, pad=True)
    keys += [(R.SHAPE_KG, wdt, "res"), (R.SHAPE_KG, wdt, "silu")]
    for key in keys:
        p, d = R.problem(*key), dev_inputs(key)
        first = run(cfm, p, d, 1)
        for tile in TILED[1:]:
            o = run(cfm, p, d, tile)
            assert torch.equal(o.out, first.out), (tile, key)
            assert first.pre is None or torch.equal(o.pre, first.pre), (tile, key)
    for shape in (R.SHAPE_K64, R.SHAPE_PAIR):
        for e in R.PLAIN:
            for c16 in (False, True):
                key = (shape, wdt, e, False, c16)
                p, d = R.problem(*key), dev_inputs(key)
                first = run(cfm, p, d, 1)
                for tile in TILED[1:] + (7, 8):
                    assert torch.equal(run(cfm, p, d, tile).out, first.out), (tile, key)
    for cv in R.CONVS:
        key = (R.conv_shape(cv), wdt, "relu", False, False, False, False, cv)
        p, d = R.problem(*key), dev_inputs(key)
        first = run(cfm, p, d, 1)
        for tile in TILED[1:] + ((8,) if cv[3] % 64 == 0 else ()):
            assert torch.equal(run(cfm, p, d, tile).out, first.out), (tile, key)


# ---------------------------------------------------------------------------------------------------------------- the automatic choice
def profiled(cfm, f):
    cfm.prof_reset(); cfm.prof_enable(True)
    try:
        out = f()
        torch.cuda.synchronize()
    finally:
        cfm.prof_enable(False)
    return out, set(cfm.prof_table())


# (M, N, K, tile argument, kernels expected, masked): thresholds of pick_tile and of the 256 x 256 cost model in csrc/gemm.hip, with
# t128 = ceil(M/128) ceil(N/128), t64x128, t64, t32x64 alike.  masked = a row mask of ones: it changes no bit and keeps the 256 x 256 and
# persistent kernels out, so the branch of pick_tile under test decides alone.
AUTO = [
    (2048, 2048, 1024, 0, {"128x128"}, True),      # t128 = 256 >= 224, K past every short-K rule: id 1
    (4096, 2048, 64, 0, {"128x128"}, False),       # cost model: one round either way, 7.99 < 8.8 -> 128 x 128 tiles; t128 = 512, t32x64 = 4096: id 1
    (2048, 2048, 64, 0, {"32x64"}, True),          # id 1, K <= 256, t128 = 256 < 512: id 5
    (2048, 2048, 64, -1, {"64x64"}, True),         # ... under -1: K <= 256, N >= 768, t64 = 1024 >= 600: back to id 3
    (1536, 2048, 1024, 0, {"64x128"}, True),       # t128 = 192 < 224, t64x128 = 384: id 2
    (1536, 2048, 1024, -1, {"64x128"}, True),      # K groups replace ids 5 and 3 only
    (1024, 2048, 2048, 0, {"64x64"}, True),        # id 2, K >= 2048, t64x128 = 256 < 384, t64 = 512 >= 448: id 3
    (1024, 2048, 2048, -1, {"64x64_k2"}, True),    # ... under -1: K >= 1024, t64 = 512 <= 512: id 11
    (1024, 1024, 1024, 0, {"64x64"}, True),        # t64x128 = 128 < 224: id 3; t64 = 256 >= 192 keeps it
    (512, 1024, 1024, 0, {"32x64"}, True),         # id 3, t64 = 128 < 192, t32x64 = 256 >= 96: id 5
    (512, 1024, 1024, -1, {"64x64_k2"}, True),     # ... under -1: id 11
    (64, 64, 1024, 0, {"64x64"}, True),            # one tile: id 3 (t32x64 = 2 < 96)
    (2600, 2048, 512, 0, {"128x64"}, True),        # t128 = 336 in [320, 448), 256 < K <= 512: id 4; t32x64 = 2624 > 2560 keeps it (M = 2560 gives 2560: id 5)
    (2600, 2048, 512, -1, {"128x64"}, True),
    (2048, 2048, 512, 0, {"32x64"}, True),         # t128 = 256 < 320, 256 < K <= 512: id 3, then K <= 768 and t32x64 = 2048 <= 2560: id 5
    (1536, 2048, 512, 0, {"32x64"}, True),         # id 2, then K <= 768 and t32x64 = 1536: id 5
    (4096, 4096, 64, 0, {"256x256"}, False),       # cost model: t256 = 256 is one whole round, 8.8 < 2 x 7.99
    (524288, 128, 64, 0, {"persistent_128x128"}, False),   # one column of 128-wide tiles: t256 = 2048 is 8 rounds, the 4096 tiles of 128 x 128 are 8 too and cheaper; t128 >= 8 x 512: persistent
    (8320, 4096, 64, 0, {"256x256", "32x64"}, False),   # 528 tiles = 2.06 rounds: rows [0, 8192) on 256 x 256, the last 128 rows on the tail's own choice
]
ID_OF = {v: k for k, v in TILE_NAME.items()}


@pytest.mark.parametrize("M,N,K,tile,names,masked", AUTO)
def test_auto_choice(cfm, M, N, K, tile, names, masked):
    """the kernel the automatic choice launches (by profile name) and its bits: those of the explicit id (K groups) or of id 1."""
    a = R.rnd((M, K), 5).to(R.BF16).cuda()
    w = R.rnd((N, K), 6, K ** -0.5).to(R.BF16).cuda()
    bias = R.rnd((N,), 7, 0.3).cuda()
    mask = torch.ones(M, dtype=torch.uint8, device="cuda") if masked else None
    call = lambda t: cfm.gemm(a, w, bias=bias, act=cfm.ACT_SILU, out_dtype=torch.bfloat16, row_mask=mask, tile=t)
    out, seen = profiled(cfm, lambda: call(tile))
    assert seen == {"gemm_bf16_" + n for n in names}, seen
    explicit = ID_OF[next(iter(names))] if len(names) == 1 else 1
    assert torch.equal(out, call(explicit))
    if explicit not in KGROUP and explicit != 1:
        assert torch.equal(out, call(1))


def test_every_instantiation_is_launched(cfm):
    """every kernel pick_tile's switch, the persistent launch and gemm256 can name is launched by an explicit id, under its own profile name."""
    want = set()

    def one(key, tile, name):
        _, seen = profiled(cfm, lambda: check(cfm, key, tile))
        assert seen == {name}, (seen, name)
        want.add(name)

    cv = R.CONVS[1]
    for wdt, tag in (("bf16", "bf16"), ("fp16", "f16")):
        for tile in TILED + KGROUP + (7, 8):
            one((R.SHAPE_K64, wdt, "relu"), tile, "gemm_%s_%s" % (tag, TILE_NAME[tile]))
        for tile in TILED:
            one((R.SHAPE_K64, wdt, "relu", True), tile, "gemm_%s_a32_%s" % (tag, TILE_NAME[tile]))
        for tile in TILED + (8,):
            one((R.conv_shape(cv), wdt, "relu", False, False, False, False, cv), tile, "gemm_conv_%s_%s" % (tag, TILE_NAME[tile]))
    for tile in (1, 2, 3, 4):
        one((R.SHAPE_K64, "bf16", "relu", True, False, False, True), tile, "gemm_bf16x3_" + TILE_NAME[tile])
        one((R.conv_shape(cv), "bf16", "relu", True, False, False, True, cv), tile, "gemm_conv_bf16x3_" + TILE_NAME[tile])
    assert len(want) == 2 * (11 + 6 + 7) + 8


# ---------------------------------------------------------------------------------------------------------------- non-finite values
@pytest.mark.parametrize("tile", (1, 5, 9, 7, 8))
def test_nan_and_inf_rows(cfm, tile):
    """one NaN, one +Inf and one row that overflows the fp16 output: those rows are what the reference says under every activation (NaN stays NaN
    through ReLU and DRELU, as in torch), no other row changes a bit, and a mask_mode 0 dead row is 0 whatever its accumulator held."""
    plain = tile in (7, 8)
    shape = R.SHAPE_K64 if plain else R.SHAPE_MAIN
    for e in R.PLAIN if plain else ("bias", "silu", "relu", "dsilu", "drelu", "mask0", "mask1"):
        key = (shape, "fp16", e, False, True)
        q, rows = R.poisoned(key)
        o = check(cfm, key, tile, poison=True)
        clean = run(cfm, R.problem(*key), dev_inputs(key), tile)
        other = torch.ones(q.M, dtype=torch.bool, device="cuda")
        other[list(rows)] = False
        assert torch.equal(o.out[other], clean.out[other]), (tile, e)
        if e in ("bias", "relu", "drelu"):
            assert bool(torch.isnan(o.out[rows[0]]).any()), (tile, e)
        if e == "mask0":                                    # the poisoned rows as dead rows
            d = dev_inputs(key, True)
            m = d.row_mask.clone()
            m[list(rows)] = 0
            dead = run(cfm, q, d, tile, row_mask=m)
            assert bool((dead.out[list(rows)] == 0).all()), tile
    if not plain:
        key = (R.SHAPE_GLU, "fp16", "glu", False, True)
        o = check(cfm, key, tile, poison=True)


# ---------------------------------------------------------------------------------------------------------------- dropout pattern, errors
def test_dropout_mask_is_the_restated_hash(cfm):
    for n, (p, seed) in ((130 * 132, R.DROP), (4099, R.DROP2), (65, (0.5, 0xFFFFFFFF))):
        assert torch.equal(cfm.dropout_mask(n, p, seed, "cuda").cpu(), R.keep_mask(n, p, seed))


def test_argument_errors(cfm):
    key = (R.SHAPE_RAGGED, "bf16", "row_len")
    p, d = R.problem(*key), dev_inputs(key)
    kw = dict(bias=d.bias, row_len=d.row_len, row_T=R.ROW_T)
    cfm.gemm(d.A, d.W, act=cfm.ACT_GLU, **kw)
    with pytest.raises(RuntimeError, match="status -1.*row_len"):
        cfm.gemm(d.A, d.W, act=cfm.ACT_SILU, **kw)                                               # without GLU
    with pytest.raises(RuntimeError, match="status -1.*row_len"):
        cfm.gemm(d.A, d.W, act=cfm.ACT_GLU, mask_mode=1, row_mask=to_dev(R.problem(R.SHAPE_RAGGED, "bf16", "row_len_mask").row_mask), **kw)
    with pytest.raises(RuntimeError, match="status -1.*row_len"):
        cfm.gemm(d.A, d.W, act=cfm.ACT_GLU, bias=d.bias, row_len=d.row_len, row_T=40)           # 150 % 40 != 0
    with pytest.raises(RuntimeError, match="status -1.*row_len"):
        cfm.gemm(d.A, d.W, act=cfm.ACT_GLU, bias=d.bias, row_len=d.row_len, row_T=0)
    with pytest.raises(ValueError, match="int32"):
        cfm.gemm(d.A, d.W, act=cfm.ACT_GLU, bias=d.bias, row_len=d.row_len.long(), row_T=R.ROW_T)
    pk = (R.SHAPE_PAIR, "bf16", "bias")
    q, e = R.problem(*pk), dev_inputs(pk)
    with pytest.raises(RuntimeError, match="status -1.*dropout"):
        cfm.gemm(e.A, e.W, bias=e.bias, drop=R.DROP)                                             # N % 4 != 0
    # drop2 without drop: the wrapper never builds that descriptor, so straight through the ABI
    mk = (R.SHAPE_MAIN, "bf16", "bias")
    q, e = R.problem(*mk), dev_inputs(mk)
    out = torch.empty((q.M, q.N), device="cuda")
    g = cfm.GemmDesc()
    g.A, g.W, g.bias, g.C = e.A.data_ptr(), e.W.data_ptr(), e.bias.data_ptr(), out.data_ptr()
    g.lda, g.ldc, g.M, g.N, g.K = q.K, q.N, q.M, q.N, q.K
    g.a_dtype, g.w_dtype, g.c_dtype, g.alpha = cfm.BF16, cfm.BF16, cfm.F32, 1.0
    assert cfm.lib().cfm_gemm(ctypes.byref(g), cfm.stream()) == 0
    g.drop2_p, g.drop2_seed = 0.1, 1
    assert cfm.lib().cfm_gemm(ctypes.byref(g), cfm.stream()) == -1
    torch.cuda.synchronize()


def test_report_worst_ratios(cfm):
    """not a check of its own: prints what the module measured (pytest -s), the figures DESIGN.md quotes."""
    g, gs, t, ts = R.measure_g()
    print("\n|d|/S  float32 torch %.3g  bound g %.3g  kernel f32 out %.3g  kernel 16-bit out beyond one ulp %.3g" % (t, g, WORST["f32"], WORST["16bit"]))
    print("split  float32 torch %.3g  bound g %.3g  kernel %.3g" % (ts, gs, WORST["split"]))
