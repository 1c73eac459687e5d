"""Every path of the row-wise kernels through the C ABI: dclip_amd/csrc/layernorm.hip (LayerNorm forward and
backward: all eight template instances x the three dx types x NS 2 / 3 x residual x which parameter gradients, the grid-stride
loop beyond 4096 rows, the > 64 KB LDS launches; colsum_f32 / bf16 / f16 and the partial-sum reduce) and train_bf16.hip
(transpose_to_*, mt_weights_*, rowsum_*).  Integer data is checked for equality, Gaussian data per element under a derived
bound, every output sits in a guarded NaN-filled buffer and every case asserts the kernel variant dclip_last_launch reports.
Checkers and case lists: tests/kernel_checks_rest.py; tests/test_kernel_checks_rest_cpu.py shows what they catch."""
import pytest
import torch

from tests import kernel_checks as kc
from tests import kernel_checks_rest as kr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from dclip_amd import _lib
    return _lib.load()


def stream():
    return torch.cuda.current_stream().cuda_stream


def ok(lib, rc, site=None):
    assert rc == 0, lib.dclip_last_error()
    if site is not None:
        assert lib.dclip_last_launch().decode() == site
    torch.cuda.synchronize()


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", kr.LN_FWD_CASES, ids=kc.case_id)
def test_layernorm_fwd_every_instance(dev, lib, case):
    s = kr.build_ln_fwd(case, dev)
    ok(lib, kr.launch_ln_fwd(lib, s, stream()), "layernorm_fwd" + kc.expected_ln16_variant(case.D))
    kc.record("ln_fwd", case, kr.verify_ln_fwd(s))


@pytest.mark.parametrize("case", kr.ln_bwd_cases(), ids=kr.ln_bwd_id)
def test_layernorm_bwd_every_instance_and_option(dev, lib, case):
    """D = 1536 and 2048 with dx_colsum ask for 73,728 and 98,304 bytes of dynamic LDS: they must compute like every other case."""
    s = kr.build_ln_bwd(case, dev)
    ok(lib, kr.launch_ln_bwd(lib, s, stream()), kr.expected_ln_bwd_site(case))
    fig = kr.verify_ln_bwd(s)
    if case.data == "gauss":
        print(kr.ln_bwd_id(case), fig)
    kc.record("ln_bwd", case, fig)


def test_layernorm_cases_reach_every_instance_and_option():
    cases = kr.ln_bwd_cases()
    variants = {".nc1", ".nc2", ".nc3", ".nc4", ".nc8", ".nc2.exact", ".nc3.exact", ".nc4.exact"}
    assert {kc.expected_ln16_variant(c.D) for c in kr.LN_FWD_CASES} == variants
    for v in variants:
        mine = [c for c in cases if kc.expected_ln16_variant(c.D) == v]
        assert {(c.entry, c.colsum) for c in mine} >= {("bwd", False), ("ex", True), ("ex", False), ("ex_f16", True), ("ex_f16", False)}
        assert {c.params for c in mine} == {"both", "gamma", "beta", "none"} and {c.acc for c in mine} == {0, 1}
        assert {c.res for c in mine} == {False, True} and {c.dx16 for c in mine} == {False, True} and max(c.rows for c in mine) == 4101
        assert any(c.params == "none" and not c.colsum for c in mine), "the launch without a workspace"
    assert any(c.D == 1536 and c.colsum for c in cases) and any(c.D == 2048 and c.colsum for c in cases)       # > 64 KB of LDS
    assert any(kr.ln_blocks(c.rows) < 64 for c in cases) and any(kr.ln_blocks(c.rows) > 64 for c in cases)    # reduce: P < 64, P > 64


@pytest.mark.parametrize("case", [c for c in kr.ln_bwd_cases() if c.D in (4, 768, 2048) and c.rows == 1001 and c.data == "int"],
                         ids=kr.ln_bwd_id)
def test_layernorm_bwd_refuses_a_workspace_one_byte_short(dev, lib, case):
    s = kr.build_ln_bwd(case, dev)
    need = int(lib.dclip_layernorm_bwd_workspace(case.rows, case.D))
    assert need == s.ws_floats * 4
    rc = kr.launch_ln_bwd(lib, s, stream(), workspace_bytes=need - 1)
    torch.cuda.synchronize()
    assert rc == kc.E_WORKSPACE and b"workspace" in lib.dclip_last_error()
    for g in (s.dx, s.dx16, s.colsum, s.ws):
        if g is not None:
            g.assert_guards("short workspace")
            assert bool(torch.isnan(g.get().float()).all()), "a refused call wrote to an output"


@pytest.mark.parametrize("D", [2052, 6, 0])
def test_layernorm_rejects_what_no_instance_handles(dev, lib, D):
    x = torch.zeros((4, max(D, 4)), device=dev)
    y = kc.Guarded(4, max(D, 4), device=dev)
    v = torch.ones((4,), device=dev)
    assert lib.dclip_layernorm_fwd(x.data_ptr(), x.data_ptr(), x.data_ptr(), y.ptr, None, None, 4, D, 1e-5, stream()) == kc.E_INVAL
    assert lib.dclip_layernorm_bwd(x.data_ptr(), x.data_ptr(), x.data_ptr(), v.data_ptr(), v.data_ptr(), None, y.ptr, None, None, 4, D, 0,
                                   None, 0, stream()) == kc.E_INVAL
    torch.cuda.synchronize()
    y.assert_guards("refused layernorm")
    assert bool(torch.isnan(y.get()).all())


# ---- column and row sums ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", kr.colsum_cases(), ids=kc.case_id)
def test_colsum_is_exact_on_integers(dev, lib, case):
    s = kr.build_colsum(case, dev)
    assert int(lib.dclip_colsum_f32_workspace(case.M, case.N)) == s.ws_floats * 4
    ok(lib, kr.launch_colsum(lib, s, stream()), kr.COLSUM_SITE[case.ty])
    kr.verify_colsum(s)


@pytest.mark.parametrize("ty", list(kr.COLSUM_FN))
def test_colsum_refuses_a_workspace_one_byte_short(dev, lib, ty):
    s = kr.build_colsum(kr.ColsumCase(ty, 8193, 260, 4, 0), dev)
    rc = kr.launch_colsum(lib, s, stream(), workspace_bytes=s.ws_floats * 4 - 1)
    torch.cuda.synchronize()
    assert rc == kc.E_WORKSPACE and b"workspace" in lib.dclip_last_error()
    for g in (s.out, s.ws):
        g.assert_guards("short workspace")
        assert bool(torch.isnan(g.get()).all()), "a refused call wrote to an output"


def test_colsum_cases_reach_every_split_count():
    splits = {kr.colsum_splits(c.M) for c in kr.colsum_cases()}
    assert {1, 2, 64} <= splits and max(splits) == 64 and any(c.M > 64 * 128 for c in kr.colsum_cases())


@pytest.mark.parametrize("case", kr.rowsum_cases(), ids=kc.case_id)
def test_rowsum_is_exact_on_integers(dev, lib, case):
    s = kr.build_rowsum(case, dev)
    ok(lib, kr.launch_rowsum(lib, s, stream()), "rowsum_bf16" if case.ty == "bf16" else "rowsum_f16")
    kr.verify_rowsum(s)


# ---- transpose and the multi-tensor weight conversion ------------------------------------------------------------------------------

@pytest.mark.parametrize("case", kr.trans_cases(), ids=kc.case_id)
def test_transpose_is_torchs_conversion_bit_for_bit(dev, lib, case):
    s = kr.build_trans(case, dev)
    ok(lib, kr.launch_trans(lib, s, stream()), "transpose_to_bf16" if case.ty == "bf16" else "transpose_to_f16")
    kr.verify_trans(s)


@pytest.mark.parametrize("case", kr.MTW_CASES, ids=kc.case_id)
def test_mt_weights_is_torchs_conversion_bit_for_bit(dev, lib, case):
    s = kr.build_mtw(case, dev)
    ok(lib, kr.launch_mtw(lib, s, stream()), "mt_weights_bf16" if case.ty == "bf16" else "mt_weights_f16")
    kr.verify_mtw(s)
