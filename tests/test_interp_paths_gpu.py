"""Every path of dclip_amd/csrc/pos_interp.hip through the C ABI: the bicubic resample of the position table,
its transpose with and without `accumulate`, and the patch gather on a gh x gw grid in fp32, bf16 and fp16 (vector and scalar
forms).  Integer data at ratios 2 and 1/2: the result must EQUAL the fp64 reference.  Gaussian data: every element inside the
derived bound.  Outputs are guarded, the rows behind every operand are NaN, a refused call launches nothing and writes
nothing.  References and checkers: tests/kernel_checks_interp.py."""
import numpy as np
import pytest
import torch

from tests import kernel_checks as kc
from tests import kernel_checks_interp as ki

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC00000            # what a NaN-filled payload word holds: a slot the kernels never wrote


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


def operand(a: np.ndarray, dev):
    return kc.poisoned(torch.from_numpy(a), a.shape[1], dev)


def unwritten(g):
    return g.get().view(torch.int32) == NAN_BITS


def run_fwd(lib, dev, pos, c):
    g, gh, gw, D = c
    src, out = operand(pos, dev), kc.Guarded(1 + gh * gw, D, device=dev)
    rc = lib.dclip_pos_interp_fwd(src.data_ptr(), out.ptr, g, gh, gw, D, stream())
    assert rc == 0, lib.dclip_last_error()
    assert lib.dclip_last_launch() == b"pos_interp_fwd"
    torch.cuda.synchronize()
    out.assert_guards("pos_interp_fwd out")
    return out.get().numpy()


def run_bwd(lib, dev, dout, c, prior=None):
    g, gh, gw, D = c
    src = operand(dout, dev)
    out = kc.Guarded(1 + g * g, D, device=dev, fill=kc.NAN if prior is None else torch.from_numpy(prior))
    rc = lib.dclip_pos_interp_bwd(src.data_ptr(), out.ptr, g, gh, gw, D, 0 if prior is None else 1, stream())
    assert rc == 0, lib.dclip_last_error()
    assert lib.dclip_last_launch() == b"pos_interp_bwd"
    torch.cuda.synchronize()
    out.assert_guards("pos_interp_bwd out")
    return out.get().numpy()


@pytest.mark.parametrize("c", ki.INT_CASES, ids=ki.case_id)
def test_forward_equals_the_reference_on_integer_tables(dev, lib, c):
    g, gh, gw, D = c
    pos = ki.build_int_table(g, D)
    got = run_fwd(lib, dev, pos, c)
    ki.check_fwd_int(got, pos, c)
    if c == ki.IDENTITY_CASE:
        ki.check_bits(got, pos, "the identity returns the table")


def test_the_identity_returns_a_gaussian_table_bit_for_bit(dev, lib):
    c = ki.IDENTITY_CASE
    pos = ki.build_gauss(1 + c[0] * c[0], c[3], 4)
    ki.check_bits(run_fwd(lib, dev, pos, c), pos, "the identity returns the table")


@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accumulate"])
@pytest.mark.parametrize("c", [c for c in ki.INT_CASES if ki.bwd_exact(c)], ids=ki.case_id)
def test_backward_equals_the_reference_on_integer_gradients(dev, lib, c, accumulate):
    g, gh, gw, D = c
    dout = ki.build_int_dout(gh, gw, D)
    prior = ki.build_int_table(g, D, seed=3) if accumulate else None
    ki.check_bwd_int(run_bwd(lib, dev, dout, c, prior), dout, c, prior=prior)


@pytest.mark.parametrize("c", ki.GAUSS_CASES, ids=ki.case_id)
def test_forward_and_backward_stay_inside_the_derived_bound_on_gaussian_tables(dev, lib, c):
    g, gh, gw, D = c
    pos, dout = ki.build_gauss(1 + g * g, D, 1), ki.build_gauss(1 + gh * gw, D, 2)
    got_f, got_b = run_fwd(lib, dev, pos, c), run_bwd(lib, dev, dout, c)
    again = run_bwd(lib, dev, dout, c)
    f, b = ki.check_fwd_gauss(got_f, pos, c), ki.check_bwd_gauss(got_b, dout, c)
    print(ki.case_id(c), "worst error / bound: forward", f, "backward", b)
    ki.check_bits(again, got_b, "the backward is run-to-run identical")
    ki.check_bits(got_f[0], pos[0], "class row")


def test_interp_refusals_launch_nothing_and_write_nothing(dev, lib):
    c = (4, 8, 8, 8)
    g, gh, gw, D = c
    pos, dout = operand(ki.build_int_table(g, D), dev), operand(ki.build_int_dout(gh, gw, D), dev)
    out, dpos = kc.Guarded(1 + gh * gw, D, device=dev), kc.Guarded(1 + g * g, D, device=dev)
    lib.dclip_relu_f32(kc.Guarded(1, 64, device=dev).ptr, 64, stream())               # some other launch site
    ok_f = [pos.data_ptr(), out.ptr, g, gh, gw, D, stream()]
    ok_b = [dout.data_ptr(), dpos.ptr, g, gh, gw, D, 0, stream()]
    bad = [(0, None), (1, None), (2, 0), (2, -1), (3, 0), (4, 0), (4, -3), (5, 0), (5, 6), (5, -4)]
    for fn, ok, misaligned in ((lib.dclip_pos_interp_fwd, ok_f, [(0, pos.data_ptr() + 4), (1, out.ptr + 8)]),
                               (lib.dclip_pos_interp_bwd, ok_b, [(0, dout.data_ptr() + 4), (1, dpos.ptr + 8)])):
        for at, value in bad + misaligned:
            args = list(ok)
            args[at] = value
            assert fn(*args) == kc.E_INVAL, (at, value)
            assert lib.dclip_last_error()
            assert lib.dclip_last_launch() == b"relu_f32", "a refused call launched"
    torch.cuda.synchronize()
    for t in (out, dpos):
        t.assert_guards("refused")
        assert bool(unwritten(t).all()), "a refused call wrote"


# ------------------------------------------------------------------------------------------------ patch gather

@pytest.mark.parametrize("c", ki.RECT_CASES, ids=ki.case_id)
def test_rect_im2col_equals_the_index_expression(dev, lib, c):
    B, C, H, W, p = c
    pix = ki.build_rect_pixels(c)
    want = ki.rect_reference(pix, p)
    src = torch.full((pix.size + 64,), kc.NAN, dtype=torch.float32, device=dev)          # NaN behind the last image
    src[:pix.size] = torch.from_numpy(pix).flatten().to(dev)
    out = kc.Guarded(want.shape[0], want.shape[1], device=dev)
    assert lib.dclip_im2col_rect(src.data_ptr(), out.ptr, B, C, H, W, p, stream()) == 0, lib.dclip_last_error()
    assert lib.dclip_last_launch() == b"im2col_rect" + ki.rect_variant(c).encode()
    torch.cuda.synchronize()
    out.assert_guards("im2col_rect")
    ki.check_bits(out.get().numpy(), want, f"im2col_rect {ki.case_id(c)}")


def test_rect_im2col_takes_the_scalar_kernel_for_a_misaligned_destination(dev, lib):
    c = (2, 3, 32, 48, 16)
    B, C, H, W, p = c
    pix = ki.build_rect_pixels(c)
    want = ki.rect_reference(pix, p)
    src = torch.from_numpy(pix).to(dev)
    buf = torch.full((want.size + 8,), kc.NAN, dtype=torch.float32, device=dev)
    assert lib.dclip_im2col_rect(src.data_ptr(), buf.data_ptr() + 4, B, C, H, W, p, stream()) == 0, lib.dclip_last_error()
    assert lib.dclip_last_launch() == b"im2col_rect.scalar"
    torch.cuda.synchronize()
    ki.check_bits(buf[1:1 + want.size].cpu().numpy().reshape(want.shape), want, "misaligned destination")
    assert bool(torch.isnan(buf[0])) and bool(torch.isnan(buf[1 + want.size:]).all())


@pytest.mark.parametrize("ty", ["bf16", "f16"])
@pytest.mark.parametrize("c", [c for c in ki.RECT_CASES if c[4] % 4 == 0], ids=ki.case_id)
def test_rect_im2col_16_bit_equals_the_index_expression_and_leaves_the_padding(dev, lib, c, ty):
    B, C, H, W, p = c
    dtype = torch.bfloat16 if ty == "bf16" else torch.float16
    entry = getattr(lib, f"dclip_im2col_rect_{ty}")
    pix = ki.build_rect_pixels(c)
    want = ki.rect_reference(pix, p)                      # integers below 10: exact in both 16-bit formats
    src = torch.full((pix.size + 64,), kc.NAN, dtype=torch.float32, device=dev)
    src[:pix.size] = torch.from_numpy(pix).flatten().to(dev)
    kdim = want.shape[1]
    out = kc.Guarded(want.shape[0], kdim, ld=kdim + 8, device=dev, dtype=dtype)
    assert entry(src.data_ptr(), out.ptr, B, C, H, W, p, kdim + 8, stream()) == 0, lib.dclip_last_error()
    assert lib.dclip_last_launch() == f"im2col_rect_{ty}".encode() + ki.rect_variant(c).encode()
    torch.cuda.synchronize()
    out.assert_guards(f"im2col_rect_{ty}")               # the padding columns count as guard words
    ki.check_bits(out.get().float().numpy(), want, f"im2col_rect_{ty} {ki.case_id(c)}")


def test_rect_refusals_launch_nothing_and_write_nothing(dev, lib):
    c = (2, 3, 32, 48, 16)
    B, C, H, W, p = c
    src = torch.from_numpy(np.nan_to_num(ki.build_rect_pixels(c))).to(dev)
    rows, kdim = B * (H // p) * (W // p), C * p * p
    out = kc.Guarded(rows, kdim, device=dev)
    out16 = kc.Guarded(rows, kdim, ld=kdim + 8, device=dev, dtype=torch.bfloat16)
    lib.dclip_relu_f32(kc.Guarded(1, 64, device=dev).ptr, 64, stream())
    ok = [src.data_ptr(), out.ptr, B, C, H, W, p, stream()]
    for at, value in [(0, None), (1, None), (2, 0), (3, 0), (4, 15), (5, 15), (6, 0), (6, 33), (6, 49)]:
        args = list(ok)
        args[at] = value
        assert lib.dclip_im2col_rect(*args) == kc.E_INVAL, (at, value)
        assert lib.dclip_last_launch() == b"relu_f32", "a refused call launched"
    ok16 = [src.data_ptr(), out16.ptr, B, C, H, W, p, kdim + 8, stream()]
    for entry in (lib.dclip_im2col_rect_bf16, lib.dclip_im2col_rect_f16):
        for at, value in [(0, None), (1, None), (2, 0), (3, 0), (4, 15), (5, 15), (6, 0), (6, 14), (7, kdim - 4), (7, kdim + 2),
                          (0, src.data_ptr() + 4), (1, out16.ptr + 2)]:
            args = list(ok16)
            args[at] = value
            assert entry(*args) == kc.E_INVAL, (at, value)
            assert lib.dclip_last_launch() == b"relu_f32", "a refused call launched"
    torch.cuda.synchronize()
    out.assert_guards("refused")
    out16.assert_guards("refused")
    assert bool(unwritten(out).all()) and bool((out16.get().view(torch.int16) == kc.NAN16[torch.bfloat16]).all())


def test_the_square_entry_points_keep_their_refusals(dev, lib):
    """dclip_im2col still refuses what dclip_im2col_rect takes."""
    src = torch.zeros((1, 3, 35, 50), device=dev)
    out = kc.Guarded(6, 768, device=dev)
    assert lib.dclip_im2col(src.data_ptr(), out.ptr, 1, 3, 35, 50, 16, stream()) == kc.E_INVAL
    assert lib.dclip_im2col(src.data_ptr(), out.ptr, 1, 3, 32, 48, 16, stream()) == kc.E_INVAL
    torch.cuda.synchronize()
    assert bool(unwritten(out).all())
