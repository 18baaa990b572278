"""CPU (no GPU): which launch sequence cfm_encoder_layer_forward picks (include/cfm.h cfm_route), asked through the host-only query
cfm_encoder_layer_route, and that every argument check comes before the first launch.  All device pointers here are made-up addresses:
no compute entry point is called with valid arguments, and a check that came late would show as a launch error instead of CFM_ERR_ARG."""
import ctypes
import os

import pytest

PTR = 0x10000            # stands for any device address: never dereferenced
F32, BF16 = 0, 1
ERR_ARG = -1
CHAIN_PACKS = ("ffm_w1f", "ffm_w2n", "ff_w1f", "ff_w2n", "qkv_wf", "out_wf", "pw1_wf", "pw2_wf")
NOT_FUSED_FFN_PACKS = ("ffm_w2n", "ff_w2n", "qkv_wf", "out_wf", "pw1_wf", "pw2_wf")      # the chain packs cfm_ffn_fused does not read too


@pytest.fixture(scope="module")
def cfm():
    import cfm as c
    if not os.path.exists(c.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return c


def weights(cfm, without=()):
    w = cfm.LayerWeights()
    for name, _ in w._fields_:
        setattr(w, name, None if name in without else PTR)
    return w


def block(cfm, M=100, D=256, FF=2048, H=4, psum_splits=0, without=(), **io_fields):
    """(weights, scratch, io) of one block of M rows with every pack present and dummy addresses everywhere."""
    s = cfm.LayerScratch()
    for name in ("xn", "hid", "qkv", "pos", "ctx", "glu", "dw"):
        setattr(s, name, PTR)
    if psum_splits:
        s.psum, s.psum_splits = PTR, psum_splits
    io = cfm.LayerIO()
    io.B, io.T, io.D, io.H, io.FF, io.ktaps = 1, M, D, H, FF, 15
    io.act_dtype, io.w_dtype = BF16, BF16
    for k, v in io_fields.items():
        setattr(io, k, v)
    return weights(cfm, without), s, io


def route(cfm, w, s, io, x_in=PTR, x_out=2 * PTR):
    """Route name, or (status, message) of a rejected call."""
    r = cfm.lib().cfm_encoder_layer_route(ctypes.byref(w), ctypes.byref(s), ctypes.byref(io), x_in, x_out)
    return cfm.ROUTES[r] if r >= 0 else (r, cfm.lib().cfm_last_error().decode())


def chained(cfm, nxt, **io_fields):
    """Arguments of a block whose last launch runs the macaron chain of block `nxt` as well."""
    return block(cfm, next_w=ctypes.cast(ctypes.pointer(nxt), ctypes.c_void_p), **io_fields)


ROUTE_TABLE = [
    ("d256", dict(), "CHAIN"),
    ("psum_at_threshold", dict(psum_splits=8, M=1536), "FFSPLIT"),
    ("psum_past_threshold", dict(psum_splits=8, M=1537), "CHAIN"),
    ("psum_7_taps", dict(psum_splits=8, M=64, ktaps=7), "CHAIN"),
    ("psum_macaron_done", dict(psum_splits=8, M=64, macaron_done=1), "CHAIN"),
    ("d512_pair", dict(D=512, H=8, psum_splits=3, M=4096), "PAIR"),
    ("d512_past_pair_rows", dict(D=512, H=8, psum_splits=3, M=4097), "CHAIN"),
    ("d512_two_slabs", dict(D=512, H=8, psum_splits=2), "CHAIN"),
    ("fused_ffn_d256", dict(without=NOT_FUSED_FFN_PACKS), "FUSED_FFN"),
    ("fused_ffn_d144", dict(without=NOT_FUSED_FFN_PACKS, D=144, FF=576), "FUSED_FFN"),
    ("no_fused_ffn_d512", dict(without=NOT_FUSED_FFN_PACKS, D=512, H=8), "GENERAL"),
    ("f32_all_packs", dict(act_dtype=F32), "GENERAL"),
    ("d144", dict(D=144, FF=576), "CHAIN"),
]


@pytest.mark.parametrize("name,kw,want", ROUTE_TABLE, ids=[r[0] for r in ROUTE_TABLE])
def test_route_of_one_block(cfm, name, kw, want):
    assert route(cfm, *block(cfm, **kw)) == want


def test_every_chain_pack_is_needed_for_a_chain_route(cfm):
    for pack in CHAIN_PACKS:
        assert route(cfm, *block(cfm, without=(pack,))) in ("GENERAL", "FUSED_FFN"), pack


def test_routes_of_chained_blocks(cfm):
    nxt = weights(cfm)
    assert route(cfm, *chained(cfm, nxt, next_x_out=3 * PTR)) == "CHAIN_NEXT_CIN"
    assert route(cfm, *chained(cfm, nxt, next_x_out=3 * PTR, macaron_done=1)) == "CHAIN_NEXT_CIN"
    prev = cfm.lib().cfm_set_cin_merge(0)
    try:
        assert route(cfm, *chained(cfm, nxt, next_x_out=3 * PTR)) == "CHAIN_NEXT"
        assert route(cfm, *block(cfm)) == "CHAIN"
    finally:
        cfm.lib().cfm_set_cin_merge(prev)
    assert route(cfm, *chained(cfm, nxt, next_x_out=3 * PTR)) == ("CHAIN_NEXT_CIN" if prev else "CHAIN_NEXT")
    # slabs do not turn a chained block into a split one
    w, s, io = chained(cfm, nxt, next_x_out=3 * PTR)
    s.psum, s.psum_splits = PTR, 8
    assert route(cfm, w, s, io) == ("CHAIN_NEXT_CIN" if prev else "CHAIN_NEXT")


@pytest.mark.parametrize("kw", [dict(next_x_out=3 * PTR, after_g=PTR, after_b=PTR, after_out=4 * PTR), dict(next_x_out=3 * PTR, causal_conv=1),
                                dict(next_x_out=3 * PTR, ktaps=7), dict(next_x_out=2 * PTR), dict()],
                         ids=["after_out", "causal_conv", "7_taps", "next_x_out_is_x_out", "no_next_x_out"])
def test_chaining_preconditions_are_argument_errors(cfm, kw):
    rc, msg = route(cfm, *chained(cfm, weights(cfm), **kw))
    assert rc == ERR_ARG and "chaining into the next block" in msg
    rc, msg = route(cfm, *chained(cfm, weights(cfm, without=("ffm_w2n",)), next_x_out=3 * PTR))
    assert rc == ERR_ARG and "chaining into the next block" in msg


def test_macaron_done_needs_the_chain_packs(cfm):
    rc, msg = route(cfm, *block(cfm, without=NOT_FUSED_FFN_PACKS, macaron_done=1))
    assert rc == ERR_ARG and "macaron_done" in msg
    rc, msg = route(cfm, *block(cfm, act_dtype=F32, macaron_done=1))
    assert rc == ERR_ARG and "macaron_done" in msg


def test_f32_mode_names_missing_lo_planes_before_any_launch(cfm):
    rc, msg = route(cfm, *block(cfm, act_dtype=F32, without=("pw2_w_lo",)))
    assert rc == ERR_ARG and "_lo weight planes" in msg


EARLY_ERRORS = [
    ("x_in_is_x_out", dict(), dict(x_out=PTR), "x_in and x_out must differ"),
    ("d_not_multiple_of_16", dict(D=24, FF=96), dict(), "multiple of 16"),
    ("after_out_without_after_g", dict(after_out=4 * PTR), dict(), "after_out needs after_g"),
    ("ring_without_stream_offset", dict(kv_ring=5 * PTR, ring_T=200), dict(), "ring needs stream_offset"),
    ("attn_cache_without_new_cache", dict(attn_cache=6 * PTR, cache_T=4), dict(), "needs new_cache"),
]


@pytest.mark.parametrize("name,kw,ptrs,text", EARLY_ERRORS, ids=[e[0] for e in EARLY_ERRORS])
def test_forward_rejects_bad_arguments_before_any_launch(cfm, name, kw, ptrs, text):
    w, s, io = block(cfm, **kw)
    rc, msg = route(cfm, w, s, io, **ptrs)                 # the query first: the forward call below is only made with arguments it rejects
    assert rc == ERR_ARG and text in msg
    rc = cfm.lib().cfm_encoder_layer_forward(ctypes.byref(w), ctypes.byref(s), ctypes.byref(io), ptrs.get("x_in", PTR), ptrs.get("x_out", 2 * PTR), 0, None, None, None)
    assert rc == ERR_ARG and text in cfm.lib().cfm_last_error().decode()


def test_forward_checks_the_next_block_before_any_launch(cfm):
    """next_w without next_x_out: this check used to sit behind the macaron chain, the attention and the conv-in chain."""
    w, s, io = chained(cfm, weights(cfm))
    rc, msg = route(cfm, w, s, io)
    assert rc == ERR_ARG and "chaining into the next block" in msg
    rc = cfm.lib().cfm_encoder_layer_forward(ctypes.byref(w), ctypes.byref(s), ctypes.byref(io), PTR, 2 * PTR, 0, None, None, None)
    assert rc == ERR_ARG and "chaining into the next block" in cfm.lib().cfm_last_error().decode()


def test_null_structs_are_argument_errors(cfm):
    w, s, io = block(cfm)
    assert cfm.lib().cfm_encoder_layer_route(None, ctypes.byref(s), ctypes.byref(io), PTR, 2 * PTR) == ERR_ARG
    assert cfm.lib().cfm_encoder_layer_route(ctypes.byref(w), ctypes.byref(s), ctypes.byref(io), PTR, None) == ERR_ARG


def decide(cfm, D=256, FF=2048, K=15, causal=False, stateful=False, M=100, streaming=False, without=(), mode="bf16", blocks=3):
    """(blocks chained, partial slabs per block) as ConformerEncoder._run_blocks and encoder_layer.BlockCall ask for them: after_norm is float32 with the
    default eps, so it rides in the last block's final chain wherever the row chains run."""
    import encoder_layer
    prec = cfm.Precision(mode)
    ws = [weights(cfm, without) for _ in range(blocks)]
    chain = encoder_layer.chain_blocks(ws, M, D, FF, K, causal, stateful, cfm.rowchain_supported(D, FF, prec), streaming)
    return chain, encoder_layer.psum_splits(M, D, FF, prec, streaming, chain)


# the cases of ROUTE_TABLE as the Python layer meets them -> (chain, psum splits); streaming = a streaming entry point (split_ffn), stateful = attention or conv caches
DECISION_TABLE = [
    ("d256", dict(), (True, 0)),
    ("d256_streaming_many_rows", dict(M=2048, streaming=True), (True, 0)),
    ("psum_at_threshold", dict(M=1536, streaming=True), (False, 8)),
    ("psum_past_threshold", dict(M=1537, streaming=True), (True, 0)),
    ("psum_7_taps", dict(M=64, K=7, streaming=True), (False, 8)),           # the library then leaves the slabs unused (ROUTE_TABLE: CHAIN)
    ("few_rows_not_streaming", dict(M=64), (True, 0)),
    ("caches", dict(stateful=True), (False, 0)),
    ("caches_streaming", dict(M=64, stateful=True, streaming=True), (False, 8)),
    ("causal", dict(causal=True), (False, 0)),
    ("causal_streaming", dict(M=64, causal=True, streaming=True), (False, 8)),
    ("ff_1024", dict(FF=1024, M=64, streaming=True), (False, 4)),
    ("d512_pair", dict(D=512, M=4096), (False, 3)),
    ("d512_pair_streaming", dict(D=512, M=64, streaming=True), (False, 3)),
    ("d512_past_pair_rows", dict(D=512, M=4097), (False, 0)),
    ("fused_ffn_d256", dict(without=NOT_FUSED_FFN_PACKS), (False, 0)),
    ("fused_ffn_d256_streaming", dict(without=NOT_FUSED_FFN_PACKS, M=64, streaming=True), (False, 8)),
    ("fused_ffn_d144", dict(without=NOT_FUSED_FFN_PACKS, D=144, FF=576), (False, 0)),
    ("f32_all_packs", dict(mode="fp32", M=64, streaming=True), (False, 0)),
    ("d144", dict(D=144, FF=576, M=64, streaming=True), (False, 0)),
]


@pytest.mark.parametrize("name,kw,want", DECISION_TABLE, ids=[r[0] for r in DECISION_TABLE])
def test_chain_and_psum_decisions(cfm, name, kw, want):
    assert decide(cfm, **kw) == want


def test_every_chain_pack_of_every_block_is_needed_to_chain(cfm):
    import encoder_layer
    assert encoder_layer.CHAIN_PACKS == CHAIN_PACKS
    for pack in CHAIN_PACKS:
        ws = [weights(cfm), weights(cfm, without=(pack,)), weights(cfm)]
        assert not encoder_layer.chain_blocks(ws, 100, 256, 2048, 15, False, False, True, False), pack
    assert not encoder_layer.chain_blocks([weights(cfm)], 100, 256, 2048, 15, False, False, False, False)      # after_norm not in the final chain


def test_route_switches_are_read_at_call_time(cfm, monkeypatch):
    import encoder_layer
    monkeypatch.setattr(encoder_layer, "CHAIN_BLOCKS", False)
    assert decide(cfm) == (False, 0) and decide(cfm, M=64, streaming=True) == (False, 8)
    monkeypatch.setattr(encoder_layer, "CHAIN_BLOCKS", True)
    monkeypatch.setattr(encoder_layer, "SPLIT_FFN_FEW_ROWS", False)
    assert decide(cfm, M=64, streaming=True) == (True, 0) and decide(cfm, M=64, streaming=True, stateful=True) == (False, 0)
    monkeypatch.setattr(encoder_layer, "PAIR_MAX_ROWS", 0)
    assert decide(cfm, D=512) == (False, 0)
    monkeypatch.setattr(encoder_layer, "split_rows", lambda M, D, FF: False)
    monkeypatch.setattr(encoder_layer, "SPLIT_FFN_FEW_ROWS", True)
    assert decide(cfm, M=64, streaming=True) == (True, 0)


def test_one_reader_of_the_split_threshold(cfm):
    import encoder_layer
    assert "CFM_FFSPLIT_MAX_ROWS" not in os.environ           # the library reads it once, at first use
    assert cfm.lib().cfm_ffsplit_max_rows() == 1536
    assert encoder_layer.split_rows(1536, 256, 2048) and not encoder_layer.split_rows(1537, 256, 2048)
    assert not hasattr(encoder_layer, "_SPLIT_MAX_ROWS")
    src = open(encoder_layer.__file__).read()
    assert "environ" not in src
    # ... and the library draws the line where split_rows does
    assert route(cfm, *block(cfm, psum_splits=8, M=1536)) == "FFSPLIT" and route(cfm, *block(cfm, psum_splits=8, M=1537)) == "CHAIN"
    for name in ("PAIR_MAX_ROWS", "SPLIT_FFN_FEW_ROWS", "CHAIN_BLOCKS"):
        assert hasattr(encoder_layer, name)
    assert encoder_layer.PAIR_MAX_ROWS == 4096
