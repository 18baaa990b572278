"""CPU (no GPU): the grouped window entry points (cfm_dwconv_bn_train_groups, cfm_dwconv_bn_train_bwd_groups, cfm_attention(_bwd)_group, cfm_ctc_nll_train_groups) refuse what
they cannot run BEFORE their first launch, with a message that names the cause.  All device pointers are made-up addresses (as in
tests/test_layer_route_cpu.py): a check that came late would show as a launch error instead of the argument error."""
import os

import pytest

PTR = 0x10000            # stands for any device address: never dereferenced
F32, BF16 = 0, 1
ERR_ARG = -1


@pytest.fixture(scope="module")
def cfm():
    import cfm as c
    if not os.path.exists(c.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return c


def table(cfm, shapes, row0=None):
    arr = (cfm.TrainGroup * max(len(shapes), 1))()
    r = 0
    for i, (B, T) in enumerate(shapes):
        arr[i].B, arr[i].T, arr[i].row0 = B, T, r if row0 is None else row0[i]
        r += B * T
    return arr


def dw_fwd(cfm, groups, n, D=144, ktaps=15):
    rc = cfm.lib().cfm_dwconv_bn_train_groups(PTR, BF16, PTR, PTR, PTR, PTR, PTR, PTR, 0.1, 1e-5, PTR, PTR, PTR, BF16, PTR, groups, n, D, ktaps, None)
    return rc, cfm.lib().cfm_last_error().decode()


def dw_bwd(cfm, groups, n, D=144, ktaps=15, g_dtype=BF16, dg_dtype=BF16, dg=PTR, glu_u=None, glu_du=None):
    rc = cfm.lib().cfm_dwconv_bn_train_bwd_groups(PTR, BF16, PTR, PTR, PTR, g_dtype, PTR, dg, dg_dtype, PTR, PTR, PTR, PTR, PTR, PTR, groups, n, D, ktaps, 0,
                                                  glu_u, glu_du, None)
    return rc, cfm.lib().cfm_last_error().decode()


TWO = [(3, 15), (2, 16)]


@pytest.mark.parametrize("call", [dw_fwd, dw_bwd])
def test_dw_groups_count_and_rows(cfm, call):
    for n in (0, 9):
        rc, msg = call(cfm, table(cfm, [(2, 5)] * 9), n)
        assert rc == ERR_ARG and "%d row groups (1 .. 8)" % n in msg, (n, rc, msg)
    rc, msg = call(cfm, table(cfm, TWO, row0=[0, 46]), 2)                    # group 1 must start at 3 * 15 = 45
    assert rc == ERR_ARG and "group 1" in msg and "must start at row 45" in msg, (rc, msg)
    rc, msg = call(cfm, table(cfm, TWO, row0=[1, 46]), 2)
    assert rc == ERR_ARG and "group 0" in msg and "must start at row 0" in msg, (rc, msg)


@pytest.mark.parametrize("call", [dw_fwd, dw_bwd])
def test_dw_groups_channels_and_taps(cfm, call):
    for D in (520, 6):
        rc, msg = call(cfm, table(cfm, TWO), 2, D=D)
        assert rc == ERR_ARG and "D <= 512" in msg and "(D=%d)" % D in msg, (D, rc, msg)
    rc, msg = call(cfm, table(cfm, TWO), 2, ktaps=7)
    assert rc == ERR_ARG and "7 taps (only 15 is built" in msg, (rc, msg)


def test_dw_groups_fused_glu_arguments(cfm):
    need = "the fused GLU backward needs u and du, g / dg of one dtype and D % 16 == 0"
    for kw in (dict(glu_u=PTR), dict(glu_du=PTR),                             # one without the other
               dict(glu_u=PTR, glu_du=PTR, g_dtype=BF16, dg_dtype=F32), dict(glu_u=PTR, glu_du=PTR, D=24)):
        rc, msg = dw_bwd(cfm, table(cfm, TWO), 2, **kw)
        assert rc == ERR_ARG and need in msg, (kw, rc, msg)
    rc, msg = dw_bwd(cfm, table(cfm, TWO), 2, dg=None)                        # neither dg nor the GLU pair: nothing to write
    assert rc == ERR_ARG and "null pointer" in msg, (rc, msg)


def test_attention_groups_need_problems(cfm):
    L = cfm.lib()
    fwd, bwd = (cfm.AttnDesc * 2)(), (cfm.AttnBwdDesc * 2)()
    for fn, arr, who in ((L.cfm_attention_group, fwd, "cfm_attention_group"), (L.cfm_attention_bwd_group, bwd, "cfm_attention_bwd_group")):
        for a, n in ((None, 2), (arr, 0)):
            rc = fn(a, n, None)
            msg = L.cfm_last_error().decode()
            assert rc == ERR_ARG and who + ": no problems" in msg, (who, n, rc, msg)
        rc = fn(arr, 2, None)                                                 # zeroed descriptors: refused problem by problem, before any launch
        assert rc == ERR_ARG and "null pointer" in L.cfm_last_error().decode()


def test_ctc_groups_count(cfm):
    L = cfm.lib()
    arr = (cfm.CtcGroup * 9)()
    for n in (0, 9):
        rc = L.cfm_ctc_nll_train_groups(arr, n, 11, None)
        msg = L.cfm_last_error().decode()
        assert rc == ERR_ARG and "1 .. 8 micro-batches" in msg, (n, rc, msg)


def test_wrappers_refuse_before_the_library(cfm):
    """cfm.ops: an empty window is a ValueError raised on the host."""
    with pytest.raises(ValueError, match="no problems"):
        cfm.attention_group([])
    with pytest.raises(ValueError, match="no problems"):
        cfm.attention_bwd_group([])
