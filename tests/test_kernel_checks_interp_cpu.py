"""CPU-only: the references and checkers of tests/kernel_checks_interp.py are right and sharp — the fp64 reference is torch's
float64 bicubic interpolate, the backward reference is its adjoint, every checker passes on the fault-free emulation of the
kernel's arithmetic and fails on each planted fault."""
import numpy as np
import pytest
import torch

from tests import kernel_checks_interp as ki

SMALL_INT = [c for c in ki.INT_CASES if c[3] <= 8]
SMALL_GAUSS = [(7, 10, 13, 8), (2, 1, 5, 4), (7, 1, 1, 4), (5, 8, 3, 4)]


@pytest.mark.parametrize("c", ki.TORCH_CASES, ids=ki.case_id)
def test_reference_is_torch_float64_bicubic(c):
    g, gh, gw = c
    D = 8
    pos = np.random.default_rng(g * 100 + gh).standard_normal((1 + g * g, D))
    t = torch.from_numpy(pos[1:]).reshape(1, g, g, D).permute(0, 3, 1, 2)
    want = torch.nn.functional.interpolate(t, size=(gh, gw), mode="bicubic", align_corners=False)
    want = want.permute(0, 2, 3, 1).reshape(gh * gw, D).numpy()
    got = ki.interp_reference(pos, g, gh, gw)
    assert np.array_equal(got[0], pos[0])
    worst = float(np.abs(got[1:] - want).max())
    print(ki.case_id(c), "worst |reference - torch float64|", worst)
    assert worst <= 1e-14


@pytest.mark.parametrize("c", ki.TORCH_CASES, ids=ki.case_id)
def test_backward_reference_is_the_adjoint(c):
    g, gh, gw = c
    rng = np.random.default_rng(5)
    pos, dout = rng.standard_normal((1 + g * g, 4)), rng.standard_normal((1 + gh * gw, 4))
    lhs = float((ki.interp_bwd_reference(dout, g, gh, gw) * pos).sum())
    rhs = float((dout * ki.interp_reference(pos, g, gh, gw)).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(rhs))


def test_axis_rows_sum_to_one_and_the_identity_is_exact():
    for g, go in [(7, 14), (7, 10), (14, 7), (16, 37), (1, 3), (2, 1)]:
        # four cubics of ~8 fp64 operations each on intermediates below 8: a few dozen 2^-53
        assert np.abs(ki.axis_matrix(g, go).sum(1) - 1.0).max() <= 64 * 2.0 ** -53
    idx, w = ki.axis_taps(7, 7)
    assert np.array_equal(w, np.tile([0.0, 1.0, 0.0, 0.0], (7, 1))) and np.array_equal(idx[:, 1], np.arange(7))
    assert np.array_equal(ki.axis_matrix(7, 7), np.eye(7))


def test_ratio_two_weights_are_multiples_of_2_to_the_minus_8():
    """What makes the integer cases exact: k/256 at ratio 2, k/32 at ratio 1/2."""
    for g, go, q in [(4, 8, 256), (7, 14, 256), (14, 7, 32), (2, 1, 32), (1, 2, 256)]:
        w = ki.axis_taps(g, go)[1] * q
        assert np.array_equal(w, np.round(w)), (g, go)


@pytest.mark.parametrize("c", ki.INT_CASES, ids=ki.case_id)
def test_integer_backward_cases_are_exact_in_any_order(c):
    """The equality list of the GPU test keeps a backward case only while taps x 2 x 2^16 < 2^24."""
    assert ki.bwd_exact(c), (c, int(ki.tap_counts(*c[:3]).max()))


@pytest.mark.parametrize("c", SMALL_INT, ids=ki.case_id)
def test_integer_checkers_pass_on_the_emulation(c):
    g, gh, gw, D = c
    pos, dout = ki.build_int_table(g, D), ki.build_int_dout(gh, gw, D)
    ki.check_fwd_int(ki.emulate_fwd(pos, g, gh, gw), pos, c)
    ki.check_bwd_int(ki.emulate_bwd(dout, g, gh, gw), dout, c)
    prior = ki.build_int_table(g, D, seed=3)
    ki.check_bwd_int(ki.emulate_bwd(dout, g, gh, gw, prior=prior), dout, c, prior=prior)


def test_integer_sums_are_exact_in_random_orders():
    rng = np.random.default_rng(0)
    for c in [(4, 8, 8, 4), (14, 7, 7, 4), (3, 6, 3, 4)]:
        g, gh, gw, D = c
        pos = ki.build_int_table(g, D)
        want = ki.interp_reference(pos, g, gh, gw)
        (iy, wy), (ix, wx) = ki.axis_taps(g, gh), ki.axis_taps(g, gw)
        for r in range(gh * gw):
            oy, ox = divmod(r, gw)
            terms = [(np.float32(np.float32(wy[oy, a]) * np.float32(wx[ox, b])), pos[1 + iy[oy, a] * g + ix[ox, b]])
                     for a in range(4) for b in range(4)]
            for _ in range(4):
                acc = np.zeros(D, np.float32)
                for j in rng.permutation(16):
                    acc = (acc + terms[j][0] * terms[j][1]).astype(np.float32)          # rounded product, rounded sum
                assert np.array_equal(acc.astype(np.float64), want[1 + r]), (c, r)


@pytest.mark.parametrize("c", SMALL_GAUSS, ids=ki.case_id)
def test_gaussian_checkers_pass_on_the_emulation(c):
    g, gh, gw, D = c
    pos, dout = ki.build_gauss(1 + g * g, D, 1), ki.build_gauss(1 + gh * gw, D, 2)
    f = ki.check_fwd_gauss(ki.emulate_fwd(pos, g, gh, gw), pos, c)
    b = ki.check_bwd_gauss(ki.emulate_bwd(dout, g, gh, gw), dout, c)
    print(ki.case_id(c), "worst error / bound: forward", f, "backward", b)


def test_torch_float32_coordinates_miss_the_bound_the_double_weights_keep():
    """Why the contract is the fp64 definition: torch's fp32 kernel forms the source coordinate in fp32."""
    c = (7, 10, 13, 64)
    g, gh, gw, D = c
    pos = ki.build_gauss(1 + g * g, D, 1)
    t = torch.from_numpy(pos[1:]).reshape(1, g, g, D).permute(0, 3, 1, 2)
    got = torch.nn.functional.interpolate(t, size=(gh, gw), mode="bicubic", align_corners=False)
    got = np.concatenate([pos[:1], got.permute(0, 2, 3, 1).reshape(gh * gw, D).numpy()], 0)
    bound = (16 + 8) * ki.U * ki.fwd_magnitude(pos, g, gh, gw)
    ratio = float((np.abs(got - ki.interp_reference(pos, g, gh, gw))[1:] / bound[1:]).max())
    print("torch float32 bicubic, worst error / bound at 7 -> (10, 13):", ratio)
    assert ki.check_fwd_gauss(ki.emulate_fwd(pos, g, gh, gw), pos, c) <= 1.0 < ratio


# which cases show which fault (a fault that needs gh != gw, or clamped taps with weight, cannot show everywhere)
FWD_FAULT_CASES = {"A_half": (4, 8, 8, 4), "align_corners": (4, 8, 8, 4), "drop_clamped": (4, 8, 8, 4), "swap_axes": (3, 6, 3, 4),
                   "cls_interp": (4, 8, 8, 4)}
BWD_FAULT_CASES = dict(FWD_FAULT_CASES, bwd_untransposed=(4, 8, 8, 4))


@pytest.mark.parametrize("fault", [f for f in ki.FAULTS if f in FWD_FAULT_CASES])
def test_forward_checkers_catch_each_fault(fault):
    c = FWD_FAULT_CASES[fault]
    g, gh, gw, D = c
    pos = ki.build_int_table(g, D)
    with pytest.raises(AssertionError):
        ki.check_fwd_int(ki.emulate_fwd(pos, g, gh, gw, fault=fault), pos, c)
    gc = (7, 10, 13, 8)
    gpos = ki.build_gauss(50, 8, 1)
    with pytest.raises(AssertionError):
        ki.check_fwd_gauss(ki.emulate_fwd(gpos, 7, 10, 13, fault=fault), gpos, gc)


@pytest.mark.parametrize("fault", ki.FAULTS)
def test_backward_checkers_catch_each_fault(fault):
    c = BWD_FAULT_CASES[fault]
    g, gh, gw, D = c
    dout = ki.build_int_dout(gh, gw, D)
    with pytest.raises(AssertionError):
        ki.check_bwd_int(ki.emulate_bwd(dout, g, gh, gw, fault=fault), dout, c)
    gc = (7, 10, 13, 8)
    gdout = ki.build_gauss(131, 8, 2)
    with pytest.raises(AssertionError):
        ki.check_bwd_gauss(ki.emulate_bwd(gdout, 7, 10, 13, fault=fault), gdout, gc)


@pytest.mark.parametrize("c", ki.RECT_CASES, ids=ki.case_id)
def test_rect_reference_is_the_stride_p_convolution(c):
    """rows of the gather times a filter bank = conv2d with stride p on the same pixels (trailing rows and columns ignored)."""
    B, C, H, W, p = c
    pix = ki.build_rect_pixels(c)
    cols = ki.rect_reference(pix, p)
    assert cols.shape == (B * (H // p) * (W // p), C * p * p) and not np.isnan(cols).any()
    w = np.random.default_rng(1).integers(-2, 3, (5, C, p, p)).astype(np.float64)
    clean = torch.from_numpy(np.nan_to_num(pix, nan=0.0)).double()
    want = torch.nn.functional.conv2d(clean, torch.from_numpy(w), stride=p).permute(0, 2, 3, 1).reshape(-1, 5).numpy()
    assert np.array_equal(cols.astype(np.float64) @ w.reshape(5, -1).T, want)
