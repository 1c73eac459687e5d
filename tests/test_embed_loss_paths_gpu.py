"""Every path of dclip_amd/csrc/embed.hip and loss.hip through the C ABI: data movement is compared bit for bit
with the torch index expression (random bit patterns: NaN payloads included), the integer scatter-add and reductions for
equality, normalize / cosine per element under a derived bound (zero rows, the eps clamp on both sides, s = t, s = -t); one
case per grid-stride kernel lies beyond the 4096-workgroup cap; outputs are guarded and NaN-filled; im2col asserts the kernel
variant it reports.  Checkers and case lists: tests/kernel_checks_rest.py."""
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


def ok(lib, rc, site, lasts=None, first=None):
    assert rc == 0, lib.dclip_last_error()
    assert lib.dclip_last_launch().decode() == site
    assert lasts is None or lasts == [first]
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", kr.im2col_cases(), ids=kc.case_id)
def test_im2col_is_the_index_expression(dev, lib, case):
    s = kr.build_im2col(case, dev)
    ok(lib, kr.launch_im2col(lib, s, stream()), kr.expected_im2col_site(case))
    kr.verify_im2col(s)


def test_im2col_cases_reach_both_kernels_and_the_grid_cap():
    cases = kr.im2col_cases()
    assert {kr.expected_im2col_site(c) for c in cases} == {"im2col.vec", "im2col.scalar", "im2col_bf16", "im2col_f16"}
    assert any(c.offset and c.p % 4 == 0 for c in cases)
    for site, per_item in (("im2col.scalar", 1), ("im2col.vec", 4), ("im2col_bf16", 4), ("im2col_f16", 4)):
        assert any(c.B * c.C * c.H * c.H // per_item > 4096 * 256 for c in cases if kr.expected_im2col_site(c) == site), site


@pytest.mark.parametrize("case", kr.ASSEMBLE_CASES, ids=kc.case_id)
def test_vision_assemble_fwd_bwd(dev, lib, case):
    s, lasts = kr.build_assemble(case, dev), []
    ok(lib, kr.launch_assemble(lib, s, stream(), lasts), "vision_assemble_bwd", lasts, "vision_assemble_fwd")
    kr.verify_assemble(s)


@pytest.mark.parametrize("case", kr.TEXT_CASES, ids=kc.case_id)
def test_text_embed_fwd_bwd_with_the_documented_id_clamp(dev, lib, case):
    s, lasts = kr.build_text(case, dev), []
    ok(lib, kr.launch_text(lib, s, stream(), lasts), "text_embed_bwd", lasts, "text_embed_fwd")
    kr.verify_text(s)


@pytest.mark.parametrize("case", kr.EOS_CASES, ids=kc.case_id)
def test_first_eos(dev, lib, case):
    s = kr.build_eos(case, dev)
    ok(lib, kr.launch_eos(lib, s, stream()), "first_eos")
    kr.verify_eos(s)


@pytest.mark.parametrize("case", kr.ROWS_CASES, ids=kc.case_id)
def test_gather_and_scatter_rows(dev, lib, case):
    s, lasts = kr.build_rows(case, dev), []
    ok(lib, kr.launch_rows(lib, s, stream(), lasts), "scatter_rows", lasts, "gather_rows")
    kr.verify_rows(s)


def test_embed_cases_cross_the_grid_cap_once_per_kernel():
    cap = 4096 * 256
    assert any(c.B * c.S * c.D // 4 > cap and c.B * (c.S - 1) * c.D // 4 > cap for c in kr.ASSEMBLE_CASES)
    assert any(c.B * c.T * c.D // 4 > cap for c in kr.TEXT_CASES)                       # forward; the backward has 4 x the items
    assert any(c.B * c.D // 4 > cap for c in kr.ROWS_CASES) and any(c.B * c.S * c.D // 4 > cap for c in kr.ROWS_CASES)


@pytest.mark.parametrize("case", kr.NORM_CASES, ids=kc.case_id)
def test_normalize_rows_fwd_bwd(dev, lib, case):
    s, lasts = kr.build_norm(case, dev), []
    ok(lib, kr.launch_norm(lib, s, stream(), lasts), "normalize_rows_bwd", lasts, "normalize_rows_fwd")
    kc.record("normalize", case, kr.verify_norm(s))


@pytest.mark.parametrize("case", kr.COS_CASES, ids=kc.case_id)
def test_cosine_loss_fwd_bwd(dev, lib, case):
    s, lasts = kr.build_cos(case, dev), []
    ok(lib, kr.launch_cos(lib, s, stream(), lasts), "cosine_loss_bwd", lasts, "cosine_loss_fwd.reduce")
    kc.record("cosine", case, kr.verify_cos(s))


@pytest.mark.parametrize("case", kr.SUB_CASES, ids=kc.case_id)
def test_sub_reduce_is_exact_on_integers(dev, lib, case):
    s = kr.build_sub(case, dev)
    ok(lib, kr.launch_sub(lib, s, stream()), "sub_reduce")
    kr.verify_sub(s)
