"""The partition rules of the column partials, on the host: each producer's row blocks cover every row once, and
folding ANY such partition gives engine.split16_col_exp of the whole-column maximum — planted columns included."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_checks_dystats as kd          # noqa: E402


def whole_column_exp(x):
    from dclip_amd import engine
    with np.errstate(all="ignore"):
        mx = np.abs(x.astype(np.float64)).max(axis=0)           # (numpy's max propagates NaN)
    return np.array([engine.split16_col_exp(float(m)) for m in mx], dtype=np.int32)


@pytest.mark.parametrize("M", [1, 64, 256, 257, 320, 12800])
def test_gemm_partition(M):
    parts = kd.gemm_partition(M)
    assert len(parts) == kd.cdiv(M, 256) and kd.is_partition(parts, M)
    assert all(int(p[0]) == 256 * i and int(p[-1]) == min(M, 256 * (i + 1)) - 1 for i, p in enumerate(parts))


@pytest.mark.parametrize("B,S", [(1, 2), (3, 50), (3, 64), (256, 50)])
def test_attention_partition(B, S):
    parts = kd.attention_partition(B, S)
    assert len(parts) == B and kd.is_partition(parts, B * S)
    assert all(np.array_equal(p // S, np.full(S, b)) for b, p in enumerate(parts))


@pytest.mark.parametrize("rows", [1, 5, 300, 4096, 4100, 12800])
def test_ln_partition(rows):
    parts = kd.ln_partition(rows)
    P = kd.ln_blocks(rows)
    assert len(parts) == P == min((rows + 3) // 4, 1024) and kd.is_partition(parts, rows)
    assert all(len(p) > 0 for p in parts)                                   # every partial row is written
    assert all(bool(np.all((p // 4) % P == b)) for b, p in enumerate(parts))
    if rows == 4100:                                                        # past the cap a block walks a second group of 4 rows
        assert list(parts[0]) == [0, 1, 2, 3, 4096, 4097, 4098, 4099] and list(parts[1]) == [4, 5, 6, 7]


@pytest.mark.parametrize("rows,cols", [(1, 8), (5, 264), (300, 16), (4100, 8)])
def test_any_partition_folds_to_the_whole_column_rule(rows, cols):
    x = kd.planted(rows, cols, 100 * rows + cols)
    want = whole_column_exp(x)
    assert list(want[:4]) == [0, 0, 0, 100]
    if rows > 1:
        assert int(want[4]) == 14 - 34                                      # 1e10 = 0.58 2^34: the 1e-30 beside it does not count
    S = 50
    groups = {"gemm": kd.gemm_partition(rows), "ln": kd.ln_partition(rows), "one": [np.arange(rows)],
              "rr3": kd.round_robin_partition(rows, 3), "rr50": kd.round_robin_partition(rows, 50)}
    if rows % S == 0:
        groups["attention"] = kd.attention_partition(rows // S, S)
    for name, parts in groups.items():
        assert kd.is_partition(parts, rows), name
        pmax, psum = kd.partials(x, parts)
        assert np.array_equal(kd.fold_col_exp(pmax), want), name
        assert pmax.dtype == np.uint32 and psum.dtype == np.float32 and pmax.shape == psum.shape == (len(parts), cols)


def test_attention_partition_folds_to_the_whole_column_rule():
    x = kd.planted(150, 24, 7)
    pmax, _ = kd.partials(x, kd.attention_partition(3, 50))
    assert np.array_equal(kd.fold_col_exp(pmax), whole_column_exp(x))


def test_row_exp_bits_is_the_engine_rule():
    from dclip_amd import engine
    vals = np.array([0.0, 1e-45, 2.0 ** -149, 2.0 ** -127, 2.0 ** -126, 1e-30, 0.5, 1.0, 16383.9, 16384.0, 1e10, 3e38, np.inf, np.nan],
                    dtype=np.float32)
    for v, b in zip(vals, kd.abs_bits(vals)):
        assert kd.row_exp_bits(b) == engine.split16_col_exp(float(v)), float(v)


def test_reduce_partials_fold_is_a_sum():
    g = np.random.default_rng(3)
    for P in (1, 5, 75, 1024):
        ps = g.standard_normal((P, 12)).astype(np.float32)
        got = kd.fold_reduce_partials(ps).astype(np.float64)
        want, mag = ps.astype(np.float64).sum(axis=0), np.abs(ps.astype(np.float64)).sum(axis=0)
        assert np.all(np.abs(got - want) <= P * 2.0 ** -24 * mag)
