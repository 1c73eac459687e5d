"""The native pieces of the split-fp16 patch embedding, each against its reference, every output inside a
NaN fence (kernel_checks.Guarded):
  1. dclip_im2col_f16x2 = dclip_split_f32_f16x2 of dclip_im2col, bit for bit;
  2. dclip_split16_front against the host rules (engine.split16_front_host) at crafted maxima, the weight copy against
     dclip_split_f32_f16x3(order 1);
  3. dclip_split_f32_f16x2_cols against dclip_split_f32_f16x2_rows_colstats (yc, col_exp, col_alpha), bit for bit;
  4. the two GEMM calls in the step's argument form against fp64 of the three products, inside the any-order bound of §9h."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_checks as kc                                      # noqa: E402
from kernel_checks_f16x3 import split_bound                     # noqa: E402

pytestmark = pytest.mark.gpu

HALF = torch.float16


def env():
    from dclip_amd import _lib, ops
    return _lib.load(), ops, torch.device("cuda:0"), ops._stream()


def bits16(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def bits32(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def scalar(v, dev):
    return torch.tensor([v], dtype=torch.float32, device=dev)


# ------------------------------------------------------------------------------------------------ 1. im2col_f16x2

@pytest.mark.parametrize("scale", ["1", "4096", "dev"])
@pytest.mark.parametrize("B,H,p", [(2, 64, 32), (3, 48, 16)])
def test_im2col_f16x2_equals_im2col_then_split(B, H, p, scale):
    lib, ops, dev, st = env()
    pix = (torch.randn((B, 3, H, H), generator=torch.Generator().manual_seed(B + p)) * 1.3).to(dev)
    pix[0, 1, 3, 5], pix[-1, 2, H - 1, H - 1], pix[0, 0, 0, 0] = 2.64, -2.1, 0.0
    rows, kdim = B * (H // p) ** 2, 3 * p * p
    cols32 = ops.im2col(pix, p)
    sdev = scalar(2.0 ** 9, dev)
    if scale == "dev":
        want = ops.split_f16x3_dev(cols32, sdev.data_ptr(), pieces=2)
        args = (1.0, sdev.data_ptr())
    else:
        want = ops.split_f16x3(cols32, float(scale), pieces=2)
        args = (float(scale), None)
    out = kc.Guarded(rows, 2 * kdim, device=dev, dtype=HALF)
    assert lib.dclip_im2col_f16x2(pix.data_ptr(), out.ptr, B, 3, H, H, p, *args, st) == 0
    assert lib.dclip_last_launch() == b"im2col_f16x2"
    got = out.get()
    assert not bool(torch.isnan(got.float()).any())
    assert torch.equal(bits16(got), bits16(want))
    out.assert_guards("im2col_f16x2")
    # the ops wrapper is the same call
    assert torch.equal(bits16(ops.im2col_f16x2(pix, p, *((1.0, args[1]) if scale == "dev" else (args[0],)))), bits16(want))


def test_im2col_f16x2_refuses_patch_14_and_odd_requests():
    lib, ops, dev, st = env()
    pix = torch.zeros((1, 3, 28, 28), device=dev)
    out = kc.Guarded(4, 2 * 588, device=dev, dtype=HALF)
    assert lib.dclip_im2col_f16x2(pix.data_ptr(), out.ptr, 1, 3, 28, 28, 14, 1.0, None, st) != 0
    assert b"multiple of 8" in lib.dclip_last_error()
    assert bool(torch.isnan(out.get().float()).all())
    out.assert_guards("refused im2col_f16x2")
    with pytest.raises(ValueError):
        ops.im2col_f16x2(pix, 14)
    pix = torch.zeros((1, 3, 32, 32), device=dev)
    out = kc.Guarded(1, 2 * 3072, device=dev, dtype=HALF)
    assert lib.dclip_im2col_f16x2(pix.data_ptr(), out.ptr, 1, 3, 32, 32, 32, 3.0, None, st) != 0          # no power of two
    assert lib.dclip_im2col_f16x2(pix.data_ptr(), out.ptr, 1, 3, 32, 64, 32, 1.0, None, st) != 0          # not square
    assert lib.dclip_im2col_f16x2(None, out.ptr, 1, 3, 32, 32, 32, 1.0, None, st) != 0
    assert bool(torch.isnan(out.get().float()).all())


# ------------------------------------------------------------------------------------------------ 2. the front plan

NAN, INF = float("nan"), float("inf")
# (name, max|pixels|, max|w|): a mantissa of exactly 0.5 and just above, zero operands, fp16's largest value, non-finite pixels
# (flag 2), a maximum that needs e < -14 (flag 1)
FRONT_CASES = [("half", 4.0, 0.05), ("above_half", 4.0 * (1 + 2.0 ** -23), 0.0625), ("zero_w", 2.64, 0.0), ("zero_image", 0.0, 0.03),
               ("max_65504", 65504.0, 0.02), ("nan_pixel", NAN, 0.05), ("inf_pixel", INF, 0.05), ("below_emin", 2.0 ** 29 * 1.5, 0.05)]


def f32(v: float) -> float:
    """v rounded to fp32, as the tensors hold it"""
    return float(torch.tensor(v, dtype=torch.float32))


def crafted(shape, top, seed, where):
    """fp32 values below |top| (finite part of it) with `top` itself at flat index `where`"""
    g = torch.Generator().manual_seed(seed)
    mag = top if math.isfinite(top) else 1.0
    x = (torch.rand(shape, generator=g) * 2 - 1) * (0.9 * mag)
    if top == 0.0:
        x.zero_()
    else:
        x.view(-1)[where] = -top if seed % 2 else top
    return x


def run_front(lib, dev, st, pix, w, wrec, w3, refresh):
    rec = kc.Guarded(1, lib.dclip_split16_front_rec_floats(), device=dev)
    nws = lib.dclip_split16_front_workspace()
    ws = kc.Guarded(1, nws // 4, device=dev)
    rc = lib.dclip_split16_front(pix.data_ptr(), pix.numel(), w.data_ptr() if w is not None else None, *(w.shape if w is not None else (0, 0)),
                                 w3.ptr if w3 is not None else None, wrec.ptr, rec.ptr, ws.ptr, nws, int(refresh), st)
    assert rc == 0, lib.dclip_last_error()
    assert lib.dclip_last_launch() == (b"split16_front.weight" if refresh else b"split16_front.plan")
    assert lib.dclip_first_launch() == b"split16_front.max"
    rec.assert_guards("front record"), ws.assert_guards("front workspace"), wrec.assert_guards("weight record")
    return rec.get()[0]


def check_record(ops, engine, rec, pmax, wmax):
    want = engine.split16_front_host(pmax, wmax)
    ints = rec.view(torch.int32)
    assert (int(ints[ops.FRONT_E]), int(ints[ops.FRONT_F]), int(ints[ops.FRONT_FLAGS])) == (want["e"], want["f"], want["flags"])
    assert float(rec[ops.FRONT_SCALE]) == 2.0 ** want["e"] and float(rec[ops.FRONT_WSCALE]) == 2.0 ** want["f"]
    assert float(rec[ops.FRONT_ALPHA]) == 2.0 ** want["a"]
    for slot, v in ((ops.FRONT_PIX_MAX, pmax), (ops.FRONT_W_MAX, wmax)):
        assert math.isnan(float(rec[slot])) if math.isnan(v) else float(rec[slot]) == v
    return want


@pytest.mark.parametrize("wshape", [(8, 768), (264, 3072)])
@pytest.mark.parametrize("name,pmax,wmax", FRONT_CASES, ids=[c[0] for c in FRONT_CASES])
def test_front_plan_follows_the_host_rules(name, pmax, wmax, wshape):
    from dclip_amd import engine
    lib, ops, dev, st = env()
    pmax, wmax = f32(pmax), f32(wmax)
    assert {"half": math.frexp(pmax)[0] == 0.5, "above_half": 0.5 < math.frexp(pmax)[0] < 0.5 + 2.0 ** -22}.get(name, True)
    # 3 x 5 x 5 x 5 = 375 pixels: no multiple of four, the maximum in the tail the vector loop does not reach
    for pshape, where in (((2, 3, 16, 16), 1000), ((5, 3, 5, 5), 374)):
        pix = crafted(pshape, pmax, 3, where).to(dev)
        w = crafted(wshape, wmax, 4, wshape[1] + 3).to(dev)
        wrec = kc.Guarded(1, lib.dclip_split16_front_wrec_floats(), device=dev)
        w3 = kc.Guarded(wshape[0], 3 * wshape[1], device=dev, dtype=HALF)
        rec = run_front(lib, dev, st, pix, w, wrec, w3, True)
        want = check_record(ops, engine, rec, pmax, wmax)
        assert want["flags"] == {"nan_pixel": 2, "inf_pixel": 2, "below_emin": 1}.get(name, 0)
        w3.assert_guards("w3")
        assert torch.equal(bits16(w3.get()), bits16(ops.split_f16x3(w, 2.0 ** want["f"], 1)))
        # the same call again: the same bits
        w3b = kc.Guarded(wshape[0], 3 * wshape[1], device=dev, dtype=HALF)
        rec2 = run_front(lib, dev, st, pix, w, wrec, w3b, True)
        assert torch.equal(bits32(rec2), bits32(rec)) and torch.equal(bits16(w3b.get()), bits16(w3.get()))
        # other pixels, the weight not refreshed: f and the weight record stay, e follows the pixels, w3 is not written
        wrec_before = bits32(wrec.get())
        pix2 = crafted(pshape, 0.75, 5, 7).to(dev)
        w3c = kc.Guarded(wshape[0], 3 * wshape[1], device=dev, dtype=HALF)
        rec3 = run_front(lib, dev, st, pix2, None, wrec, w3c, False)
        check_record(ops, engine, rec3, 0.75, wmax)
        assert torch.equal(bits32(wrec.get()), wrec_before) and bool(torch.isnan(w3c.get().float()).all())


def test_front_plan_non_finite_weight_sets_flag_2():
    from dclip_amd import engine
    lib, ops, dev, st = env()
    pix = crafted((1, 3, 8, 8), 1.0, 2, 5).to(dev)
    w = crafted((8, 64), 0.1, 2, 9)
    w[3, 7] = INF
    wrec, w3 = kc.Guarded(1, 4, device=dev), kc.Guarded(8, 192, device=dev, dtype=HALF)
    rec = run_front(lib, dev, st, pix, w.to(dev), wrec, w3, True)
    want = check_record(ops, engine, rec, 1.0, INF)
    assert want["flags"] == 2 and want["f"] == 0


# ------------------------------------------------------------------------------------------------ 3. the column-only split

def cols_data(rows, cols, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((rows, cols), generator=g) * torch.exp2(torch.randint(-20, 4, (cols,), generator=g).float())
    x[:, cols // 3] = 0.0                                                                 # an all-zero column: exponent 0, zero pieces
    x[:, cols - 1] = torch.exp(8.0 * torch.randn((rows,), generator=g)) * torch.sign(torch.randn((rows,), generator=g))   # e^(8 sigma)
    return x


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("cols", [8, 264, 768])
@pytest.mark.parametrize("rows", [64, 200, 1000])
def test_split_cols_equals_the_colstats_outputs(rows, cols, pad):
    lib, ops, dev, st = env()
    ldx = cols + pad
    x = kc.poisoned(cols_data(rows, cols, rows + cols), ldx, device=dev)
    want_y, want_ra, want_yc, want_ce, want_ca = ops.split_f16x3_rows_colstats(x[:rows, :cols], pieces=2)
    assert bool(torch.isfinite(want_ca).all()) and int(want_ce[cols // 3]) == 0
    nws = lib.dclip_split_f32_f16x2_cols_workspace(rows, cols)
    runs = []
    for _ in range(2):
        yc = kc.Guarded(rows, 2 * cols, device=dev, dtype=HALF)
        ce, ca, ws = kc.Guarded(1, cols, device=dev), kc.Guarded(1, cols, device=dev), kc.Guarded(1, nws // 4, device=dev)
        rc = lib.dclip_split_f32_f16x2_cols(x.data_ptr(), yc.ptr, ce.ptr, ca.ptr, rows, cols, ldx, ws.ptr, nws, st)
        assert rc == 0, lib.dclip_last_error()
        assert lib.dclip_last_launch() == b"split_f32_f16x2_cols.cols" and lib.dclip_first_launch() == b"split_f32_f16x2_cols.max"
        for gd, nm in ((yc, "yc"), (ce, "col_exp"), (ca, "col_alpha"), (ws, "workspace")):
            gd.assert_guards(nm)
        assert not bool(torch.isnan(ws.get()).any())                                       # every partial word is written
        runs.append((bits16(yc.get()), bits32(ce.get()[0]), bits32(ca.get()[0])))
    assert torch.equal(runs[0][0], bits16(want_yc))
    assert torch.equal(runs[0][1], want_ce.cpu()) and torch.equal(runs[0][2], bits32(want_ca))
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))
    got = ops.split_f16x2_cols(x[:rows, :cols])                                            # the wrapper: the same call
    assert torch.equal(bits16(got[0]), bits16(want_yc)) and torch.equal(got[1], want_ce) and torch.equal(bits32(got[2]), bits32(want_ca))


def test_split_cols_refuses_a_short_workspace_and_odd_widths():
    lib, ops, dev, st = env()
    x = torch.zeros((64, 16), device=dev)
    yc, ce, ca = kc.Guarded(64, 32, device=dev, dtype=HALF), kc.Guarded(1, 16, device=dev), kc.Guarded(1, 16, device=dev)
    nws = lib.dclip_split_f32_f16x2_cols_workspace(64, 16)
    ws = kc.Guarded(1, nws // 4, device=dev)
    assert lib.dclip_split_f32_f16x2_cols(x.data_ptr(), yc.ptr, ce.ptr, ca.ptr, 64, 16, 16, ws.ptr, nws - 4, st) != 0
    assert lib.dclip_split_f32_f16x2_cols(x.data_ptr(), yc.ptr, ce.ptr, ca.ptr, 64, 12, 16, ws.ptr, nws, st) != 0
    assert bool(torch.isnan(yc.get().float()).all()) and bool(torch.isnan(ce.get()).all())


# ------------------------------------------------------------------------------------------------ 4. the two GEMM calls

def test_forward_call_form_within_the_any_order_bound():
    """dclip_gemm_f16x3_scaled_dev as the patch embedding calls it: lda = 2 K, offsets (0, K, 0, 2 K), alpha from the front
    record, no bias, fp32 out — 128 x 264 x 96."""
    lib, ops, dev, st = env()
    M, N, K = 128, 264, 96
    g = torch.Generator().manual_seed(11)
    x, w = torch.randn((M, K), generator=g) * 1.2, torch.randn((N, K), generator=g) * 0.03
    pix = x.reshape(1, 1, M, K)                                                            # (any fp32 values serve as pixels)
    state = ops.split16_front_state(w.to(dev))
    rec = ops.split16_front(pix.to(dev), w.to(dev), state, True)
    a2 = ops.split_f16x3_dev(x.to(dev), rec.data_ptr() + 4 * ops.FRONT_SCALE, pieces=2)
    w3 = state["w3"]
    out = kc.Guarded(M, N, device=dev)
    rc = lib.dclip_gemm_f16x3_scaled_dev(a2.data_ptr(), w3.data_ptr(), out.ptr, None, None, M, N, K, 2 * K, 3 * K, N, 0, K, 0, 2 * K, 0, 0,
                                         rec.data_ptr() + 4 * ops.FRONT_ALPHA, st)
    assert rc == 0, lib.dclip_last_error()
    out.assert_guards("patch embedding")
    a2c, w3c, alpha = a2.cpu(), w3.cpu(), float(rec[ops.FRONT_ALPHA])
    want, bound = split_bound(a2c[:, :K], a2c[:, K:], w3c[:, :K], w3c[:, 2 * K:], K)
    err = (out.get().double() - want * alpha).abs()
    assert bool((err <= bound * alpha).all()), float((err / (bound * alpha)).max())
    ref = x.double() @ w.double().t()                                                      # and the product it stands for
    assert kc.relerr(out.get(), ref) < 1e-5


@pytest.mark.parametrize("splits", [1])
def test_weight_gradient_call_form_within_the_any_order_bound(splits):
    """dclip_gemm_f16x3_wgrad_tokmajor as patch_w's gradient calls it: M = D, N = patch_dim, lddy = 2 D, ldx = 2 patch_dim,
    (0, D), (0, patch_dim), col_alpha from the column split, act_scale = the front record's 2^e — 64 tokens x (8, 264)."""
    lib, ops, dev, st = env()
    T, D, K = 64, 8, 264
    g = torch.Generator().manual_seed(12)
    x, dy = torch.randn((T, K), generator=g) * 1.2, torch.randn((T, D), generator=g) * torch.exp2(torch.arange(D).float() - 12)
    state = ops.split16_front_state(torch.ones((D, K), device=dev))
    rec = ops.split16_front(x.reshape(1, 1, T, K).to(dev), torch.ones((D, K), device=dev), state, True)
    x2 = ops.split_f16x3_dev(x.to(dev), rec.data_ptr() + 4 * ops.FRONT_SCALE, pieces=2)
    yc, ce, ca = ops.split_f16x2_cols(dy.to(dev))
    nws = lib.dclip_gemm_f16x3_wgrad_tokmajor_workspace(D, K, splits)
    out, ws = kc.Guarded(D, K, device=dev), kc.Guarded(1, nws // 4, device=dev)
    rc = lib.dclip_gemm_f16x3_wgrad_tokmajor(yc.data_ptr(), x2.data_ptr(), out.ptr, D, K, T, 2 * D, 2 * K, K, 0, D, 0, K, ca.data_ptr(),
                                             rec.data_ptr() + 4 * ops.FRONT_SCALE, splits, ws.ptr, nws, st)
    assert rc == 0, lib.dclip_last_error()
    out.assert_guards("patch_w gradient"), ws.assert_guards("workspace")
    ycc, x2c = yc.cpu(), x2.cpu()
    want, bound = split_bound(ycc[:, :D].t(), ycc[:, D:].t(), x2c[:, :K].t(), x2c[:, K:].t(), T)
    scale = ca.cpu().double()[:, None] / float(rec[ops.FRONT_SCALE])
    err = (out.get().double() - want * scale).abs()
    assert bool((err <= bound * scale).all()), float((err / (bound * scale)).max())                  # (the scales are powers of two)
    assert kc.relerr(out.get(), dy.double().t() @ x.double()) < 1e-5
