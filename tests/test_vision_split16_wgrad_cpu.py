"""The numerics of the split-fp16 weight gradients, emulated on the host: dW[n,k] = sum_m dY[m,n] X[m,k] from
fp16 hi/lo pieces with fp32 sums of exact products, dY scaled by one power of two PER COLUMN (engine.split16_col_exp), X by
the forward's one scale per tensor — against the fp32 product, both measured against fp64 relative to sum |terms|; the two
scalings that do not work (one per tensor; the data-gradient's row-scaled pieces reused) as planted faults; and the rule."""
import math

import pytest
import torch

from dclip_amd import engine

TOKENS, NOUT, NIN = 1280, 96, 80


def pieces(v):
    hi = v.half()
    return hi.float(), (v - hi.float()).half().float()


def three_products(dhi, dlo, xhi, xlo):
    """hi.hi + lo.hi + hi.lo: every product of two fp16 values is exact in fp32, the sums are fp32"""
    return (dhi.t() @ xhi + dlo.t() @ xhi) + dhi.t() @ xlo


def x_split(x):
    """the forward's split of an activation: one power of two from a bound on the tensor (4x its maximum: the plan's bounds,
    products of weight statistics, are loose)"""
    e = engine.split16_act_exp(4.0 * float(x.abs().max()))
    assert e is not None
    return pieces(x * 2.0 ** e) + (2.0 ** -e,)


def wgrad_fp32(dy, x):
    return dy.t() @ x


def wgrad_per_column(dy, x):
    e = torch.tensor([engine.split16_col_exp(float(r)) for r in dy.abs().amax(dim=0).double()])
    dhi, dlo = pieces(dy * torch.exp2(e)[None, :])
    xhi, xlo, inv = x_split(x)
    return (three_products(dhi, dlo, xhi, xlo) * inv) * torch.exp2(-e)[:, None]


def wgrad_per_tensor(dy, x):
    """planted fault: ONE scale for all of dY"""
    e = engine.split16_row_exp(float(dy.abs().max()))
    dhi, dlo = pieces(dy * 2.0 ** e)
    xhi, xlo, inv = x_split(x)
    return (three_products(dhi, dlo, xhi, xlo) * inv) * 2.0 ** -e


def wgrad_row_pieces_reused(dy, x):
    """planted fault: the data gradient's row-scaled pieces of dY; the row scale lies along the contraction, so it can only be
    undone on X's rows BEFORE X is split with its one scale per tensor"""
    d3, row_alpha = engine.split16_rows_host(dy)
    n = dy.shape[1]
    dhi, dlo = d3[:, :n].float(), d3[:, n:2 * n].float()
    xhi, xlo, inv = x_split(x * row_alpha[:, None])
    return three_products(dhi, dlo, xhi, xlo) * inv


def worst(got, dy, x):
    want = dy.double().t() @ x.double()
    terms = dy.double().abs().t() @ x.double().abs()
    return float(((got.double() - want).abs() / terms).max())


def inputs(name):
    g = torch.Generator().manual_seed({"iid": 1, "rows": 2, "rows_cols": 3, "relu": 4, "tiny": 5}[name])
    dy = torch.randn((TOKENS, NOUT), generator=g)
    x = torch.randn((TOKENS, NIN), generator=g)
    rs = lambda s: torch.exp(s * torch.randn((TOKENS, 1), generator=g))      # noqa: E731
    cs = lambda s, n: torch.exp(s * torch.randn((1, n), generator=g))        # noqa: E731
    if name == "iid":
        dy = dy * 1e-7
    elif name == "rows":
        dy = dy * rs(4.0) * 1e-7
    elif name == "rows_cols":
        dy = dy * rs(4.0) * cs(4.0, NOUT) * 1e-7
    elif name == "relu":
        dy = dy * rs(4.0) * cs(4.0, NOUT) * 1e-7
        x = torch.relu(x) * cs(2.0, NIN)
    else:
        dy = dy * rs(8.0) * cs(8.0, NOUT) * 1e-20
    return dy.float(), x.float()


SETS = ("iid", "rows", "rows_cols", "relu", "tiny")


@pytest.mark.parametrize("name", SETS)
def test_per_column_split_within_4x_of_fp32(name):
    dy, x = inputs(name)
    e32, es = worst(wgrad_fp32(dy, x), dy, x), worst(wgrad_per_column(dy, x), dy, x)
    print(f"{name}: fp32 {e32:.3e}  split per column {es:.3e}  ratio {es / e32:.2f}")
    assert math.isfinite(es) and es <= 4 * e32


def test_planted_faults_miss_the_bar():
    dy, x = inputs("rows_cols")
    e32 = worst(wgrad_fp32(dy, x), dy, x)
    et, er = worst(wgrad_per_tensor(dy, x), dy, x), worst(wgrad_row_pieces_reused(dy, x), dy, x)
    print(f"rows_cols: fp32 {e32:.3e}  one scale per tensor {et:.3e}  row-scaled pieces reused {er:.3e}")
    assert et > 4 * e32 and er > 4 * e32


def test_col_exp_rule():
    ce = engine.split16_col_exp
    assert ce(0.0) == 0 and ce(float("inf")) == 0 and ce(float("nan")) == 0
    assert ce(1.0) == 13 and ce(0.75) == 14 and ce(2.0 ** 13) == 0 and ce(2.0 ** 14 - 1) == 0 and ce(2.0 ** 14) == -1
    assert ce(2.0 ** -149) == 100 and ce(2.0 ** -87) == 100 and ce(2.0 ** -86) == 99      # subnormal maxima, and the clamp
    assert ce(2.0 ** 113) == -100 and ce(2.0 ** 114) == -100 and ce(2.0 ** 112) == -99
    assert ce(-3.0) == ce(3.0)
    for r in (1e-20, 3e-8, 0.4, 77.0, 1e10):
        assert 2.0 ** 13 <= r * 2.0 ** ce(r) < 2.0 ** 14
