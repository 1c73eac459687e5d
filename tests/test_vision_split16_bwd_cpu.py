"""Row-scaled split-fp16 data-gradient GEMMs, host side: the per-row exponent rule and its edge cases, the
emulated split dgrad (pieces in fp16, products and sums in fp32) against the fp64 product on six input sets, and a planted
fault — one scale for the whole tensor — that must miss the bar."""
import math

import pytest
import torch

from dclip_amd import engine


def gen(seed):
    return torch.Generator().manual_seed(seed)


def lognormal(shape, sigma, scale, g):
    return torch.randn(shape, generator=g) * torch.exp(sigma * torch.randn(shape, generator=g)) * scale


def input_sets():
    """(name, dY [M, N], W [N, K]) — the six sets of DESIGN.md §9e's table"""
    out = []
    g = gen(1)
    out.append(("iid", torch.randn((300, 768), generator=g), torch.randn((768, 264), generator=g) * 0.05))
    g = gen(2)
    out.append(("lognormal s2 1e-7", lognormal((300, 768), 2.0, 1e-7, g), torch.randn((768, 264), generator=g) * 0.05))
    g = gen(3)
    out.append(("N3072 K768 s3 1e-9", lognormal((96, 3072), 3.0, 1e-9, g), torch.randn((3072, 768), generator=g) * 0.03))
    for i, (spread, scale) in enumerate(((4.0, 1.0), (8.0, 1.0), (8.0, 1e-20))):
        g = gen(4 + i)
        dy = lognormal((300, 768), 1.0, scale, g) * torch.exp(spread * torch.randn((300, 1), generator=g))
        out.append((f"rows s{spread:g} scale {scale:g}", dy, torch.randn((768, 264), generator=g) * 0.05))
    return out


def split_w(w):
    """[hi|hi|lo] of w^T 2^f as two fp32 matrices, and 2^-f"""
    f = engine.split16_weight_exp(float(w.abs().max()))
    v = w.t().contiguous() * 2.0 ** f
    hi = v.half()
    return hi.float(), (v - hi.float()).half().float(), 2.0 ** -f


def emulated(dy, w, per_tensor=False):
    """dX of the split path: exact fp16 products, fp32 accumulation (a float32 matmul of the pieces), the two scales undone"""
    if per_tensor:
        e = engine.split16_row_exp(float(dy.abs().max()))
        v = dy * 2.0 ** e
        hi = v.half()
        a3, ra = torch.cat([hi, (v - hi.float()).half(), hi], dim=1), torch.full((dy.shape[0],), 2.0 ** -e)
    else:
        a3, ra = engine.split16_rows_host(dy)
    whi, wlo, wa = split_w(w)
    N = dy.shape[1]
    ahi, alo = a3[:, :N].float(), a3[:, N:2 * N].float()
    acc = torch.cat([ahi, alo, ahi], dim=1) @ torch.cat([whi, whi, wlo], dim=1).t()
    return (acc * wa) * ra[:, None]


def row_rel(got, want):
    """worst row-relative error: max over rows of max|got - want| / max|want| of that row (rows with a zero reference skipped)"""
    d = (got.double() - want).abs().amax(dim=1)
    s = want.abs().amax(dim=1)
    ok = s > 0
    return float((d[ok] / s[ok]).max())


def test_row_exp_edge_cases():
    f = engine.split16_row_exp
    assert f(1.0) == 13 and f(0.5) == 14 and f(2.0) == 12             # a power of two: r 2^e = 2^13 exactly
    assert f(1.9999999) == 13 and f(0.99999994) == 14                 # just below one: still inside [2^13, 2^14)
    for r in (3.0, 1e-7, 123456.0, 2.0 ** -80):
        assert 2.0 ** 13 <= r * 2.0 ** f(r) < 2.0 ** 14
    assert f(0.0) == 0 and f(float("inf")) == 0 and f(float("nan")) == 0
    assert f(2.0 ** -86) == 99 and f(2.0 ** -87) == 100 and f(2.0 ** -88) == 100 and f(2.0 ** -120) == 100     # upper clamp
    assert f(2.0 ** 113) == -100 and f(2.0 ** 112) == -99 and f(2.0 ** 120) == -100                            # lower clamp
    assert f(1e-40) == 100 and f(2.0 ** -149) == 100                  # subnormal maxima
    assert f(-3.0) == f(3.0)
    # 2^e, 2^-e and their product with any normal weight alpha 2^-f (|f| <= 26 in practice) stay normal fp32
    for e in (-100, 100):
        assert math.isfinite(2.0 ** e) and 2.0 ** (-abs(e) - 26) >= 2.0 ** -126    # the smallest normal fp32


def test_rows_host_pieces():
    x = torch.tensor([[1.0, 2.0, -4.0, 0.5, 0.0, 0.0, 3.0, 1e-3], [0.0] * 8, [float("inf")] + [1.0] * 7,
                      [float("nan")] + [1.0] * 7, [2.0 ** -120] * 8, [2.0 ** 100] * 8])
    y, ra = engine.split16_rows_host(x)
    assert y.shape == (6, 24) and y.dtype == torch.float16 and ra.dtype == torch.float32
    assert ra.tolist() == [2.0 ** -11, 1.0, 1.0, 1.0, 2.0 ** -100, 2.0 ** 87]
    assert torch.equal(y[:, :8].view(torch.int16), y[:, 16:].view(torch.int16))                                            # [hi|lo|hi]
    assert float(y[0, 2]) == -8192.0 and float(y[4, 0]) == 2.0 ** -20 and float(y[5, 0]) == 8192.0
    assert not y[1].any()
    assert not torch.isfinite(y[2, :16]).all() and not torch.isfinite(y[3, :16]).all()
    rec = (y[0, :8].double() + y[0, 8:16].double()) * float(ra[0])
    assert float((rec - x[0].double()).abs().max()) <= 2.0 ** -22 * 4.0


@pytest.fixture(scope="module")
def measured():
    out = {}
    for name, dy, w in input_sets():
        dy = dy.clone()
        dy[7].zero_()                                                                     # a zero row in every set
        want = dy.double() @ w.double()
        out[name] = (dy, w, want, row_rel(dy @ w, want))
    return out


def test_emulated_dgrad_within_4x_of_fp32(measured):
    assert len(measured) == 6
    for name, (dy, w, want, e32) in measured.items():
        got = emulated(dy, w)
        es = row_rel(got, want)
        print(f"{name}: worst row-relative error fp32 {e32:.3e} split {es:.3e} ratio {es / e32:.2f}")
        assert es <= 4 * e32, (name, es, e32)
        assert not got[7].any(), name                                                     # zero row: exactly zero
        assert bool(torch.isfinite(got).all()), name


def test_one_scale_per_tensor_fails_the_bar(measured):
    dy, w, want, e32 = measured["rows s8 scale 1"]
    es = row_rel(emulated(dy, w, per_tensor=True), want)
    print(f"per-tensor scale on the row-spread set: {es:.3e} against fp32 {e32:.3e}")
    assert es > 4 * e32


def test_switch_is_read_once():
    import os
    assert engine._VSPLIT16_BWD == (os.environ.get("DCLIP_VISION_SPLIT16_BWD", "1") != "0")
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dclip_amd", "engine.py")).read()
    assert src.count('os.environ.get("DCLIP_VISION_SPLIT16_BWD"') == 1
