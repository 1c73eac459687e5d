"""dY read once, kernel by kernel on the hardware: the single-pass split against the three-launch entry on the
same x, and the three producers of column partials — the row-scaled GEMM, the one-tile attention backward and ln_bwd — each
against its own call without statistics and against the exact maxima / fp64 sums of what it stored.  New outputs sit in
NaN-filled guarded buffers; launch sites are asserted."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_checks_dystats as kd                               # noqa: E402
from test_vision_split16_gpu import same                         # noqa: E402
from test_vision_split16_bwd_gpu import same_nan                 # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64          # elements before and after a guarded buffer


class Guarded:
    """a contiguous buffer of `shape` inside a larger one filled with all-ones bits (a NaN as a float): nothing may be written
    outside, and whatever is left unwritten inside stays visible"""

    def __init__(self, shape, dtype, dev):
        n = int(np.prod(shape))
        self.full = torch.full((n + 2 * GUARD,), -1, dtype=torch.int16 if dtype == torch.float16 else torch.int32, device=dev)
        self.t = self.full[GUARD:GUARD + n].view(dtype).view(*shape)
        self.n = n

    def intact(self):
        f = self.full.cpu()
        return bool((f[:GUARD] == -1).all()) and bool((f[GUARD + self.n:] == -1).all())

    def all_written(self):
        return not bool((self.full[GUARD:GUARD + self.n] == -1).any())


def guarded_stats(P, cols, dev):
    from dclip_amd import ops
    pm, ps = Guarded((P, cols), torch.int32, dev), Guarded((P, cols), torch.float32, dev)
    return ops.ColStats.of(pm.t, ps.t), pm, ps


def last_launch():
    from dclip_amd import _lib
    return _lib.load().dclip_last_launch()


def check_partials(stats, pm, ps, stored, parts, rows_bound, tag):
    """maxima exact, sums within rows_bound 2^-24 sum|.| of fp64, every word written, nothing outside"""
    assert pm.intact() and ps.intact(), tag
    assert pm.all_written(), tag
    x = stored.detach().cpu().numpy()
    want_max, _ = kd.partials(x, parts)
    assert np.array_equal(stats.pmax.cpu().numpy().view(np.uint32), want_max), tag
    got = stats.psum.cpu().double().numpy()
    worst = 0.0
    for p, rows in enumerate(parts):
        xd = x[rows].astype(np.float64)
        want, bound = xd.sum(axis=0), rows_bound * 2.0 ** -24 * np.abs(xd).sum(axis=0)
        assert np.all(np.abs(got[p] - want) <= bound), (tag, p)
        nz = bound > 0
        if nz.any():
            worst = max(worst, float((np.abs(got[p] - want)[nz] / bound[nz]).max()))
    return worst


# ------------------------------------------------------------------------------------------------ 1. the single pass

def check_single_pass(rows, cols, ld, P, seed):
    from dclip_amd import _lib, ops
    lib = _lib.load()
    dev = torch.device("cuda:0")
    x = kd.planted(rows, cols, seed, ld)
    xd = torch.from_numpy(x).to(dev)[:, :cols]
    assert rows == 1 or xd.stride(0) == ld
    db0 = torch.empty((cols,), dtype=torch.float32, device=dev)
    want = ops.split_f16x3_rows_colstats(xd, db=db0)                      # y, row_alpha, yc, col_exp, col_alpha
    assert last_launch() == b"split_f32_f16x3_rows_colstats.cols"
    pmax, psum = kd.partials(x[:, :cols], kd.round_robin_partition(rows, P))
    st = ops.ColStats.of(torch.from_numpy(pmax.view(np.int32)).to(dev), torch.from_numpy(psum).to(dev))
    y, ra = Guarded((rows, 3 * cols), torch.float16, dev), Guarded((rows,), torch.float32, dev)
    yc, ce = Guarded((rows, 2 * cols), torch.float16, dev), Guarded((cols,), torch.int32, dev)
    ca, db = Guarded((cols,), torch.float32, dev), Guarded((cols,), torch.float32, dev)
    rc = lib.dclip_split_f32_f16x3_rows_cols_stats(xd.data_ptr(), y.t.data_ptr(), ra.t.data_ptr(), yc.t.data_ptr(), ce.t.data_ptr(),
                                                   ca.t.data_ptr(), db.t.data_ptr(), st.pmax.data_ptr(), st.psum.data_ptr(), P, rows,
                                                   cols, ld if rows > 1 else cols, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.dclip_last_error()
    tag = (rows, cols, ld, P)
    assert last_launch() == b"split_f32_f16x3_rows_cols_stats" + (b".cached" if cols > 3072 else b".regs.nc%d" % kd.cdiv(cols // 8, 64)), tag
    assert lib.dclip_first_launch() == b"split_f32_f16x3_rows_cols_stats.finish", tag
    for g in (y, ra, yc, ce, ca, db):
        assert g.intact(), tag
    got = (y.t, ra.t, yc.t, ce.t, ca.t)                                   # (equal to `want`, so written: the fill is no value of theirs)
    assert all(same_nan(a, b) if a.dtype.is_floating_point else same(a, b) for a, b in zip(got, want)), tag
    xs = x[:, :cols].astype(np.float64)
    with np.errstate(all="ignore"):
        fin = np.isfinite(xs).all(axis=0)
        exact, bound = xs.sum(axis=0), rows * 2.0 ** -24 * np.abs(xs).sum(axis=0)
    d = db.t.cpu().double().numpy()
    assert not np.isfinite(d[~fin]).any(), tag
    err = np.abs(d[fin] - exact[fin])
    assert np.all(err <= bound[fin]), tag
    nz = bound[fin] > 0
    return float((err[nz] / bound[fin][nz]).max()) if nz.any() else 0.0


@pytest.mark.parametrize("cols", [8, 264, 768, 3080])
def test_single_pass_equals_the_three_launches(cols):
    """3080 columns: past 3072 the row is read twice, the second time from the cache (NC == 0)"""
    worst = 0.0
    for rows in (1, 5, 300):
        for pad in (8, 40):
            for P in (1, 3, 50):
                worst = max(worst, check_single_pass(rows, cols, cols + pad, P, 1000 * rows + cols + pad + P))
    print(f"single pass, {cols} columns: db worst error / bound {worst:.3f}")


def test_single_pass_refuses_bad_arguments():
    from dclip_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    x = torch.zeros((4, 16), device=dev)
    o = [torch.zeros((4, 48), dtype=torch.float16, device=dev), torch.zeros(4, device=dev), torch.zeros((4, 32), dtype=torch.float16, device=dev),
         torch.zeros(16, dtype=torch.int32, device=dev), torch.zeros(16, device=dev)]
    pm, ps = torch.zeros((1, 16), dtype=torch.int32, device=dev), torch.zeros((1, 16), device=dev)

    def call(P=1, rows=4, cols=16, ldx=16, pmax=pm):
        return lib.dclip_split_f32_f16x3_rows_cols_stats(x.data_ptr(), *(t.data_ptr() for t in o), None,
                                                         None if pmax is None else pmax.data_ptr(), ps.data_ptr(), P, rows, cols, ldx, None)
    assert call() == 0
    for kw in (dict(P=0), dict(cols=12), dict(ldx=8), dict(pmax=None), dict(rows=0)):
        assert call(**kw) != 0, kw
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. the row-scaled GEMM

@pytest.mark.parametrize("K", [64, 192])
@pytest.mark.parametrize("dgelu", [False, True])
def test_gemm_rows_stats(K, dgelu, monkeypatch):
    """M 64 / 320: one tile row, and two with the second one partial; N 8 / 264 / 520: an edge tile alone, one full tile and an
    edge, two full tiles and an edge"""
    from dclip_amd import ops
    dev = torch.device("cuda:0")
    worst = 0.0
    for M in (64, 320):
        for N in (8, 264, 520):
            monkeypatch.delenv("DCLIP_BF16_BIG_MIN", raising=False)
            assert ops.gemm_f16_rows_stats_plan(M, N, K) == 0                # fewer than 128 tiles: a register-staged kernel
            monkeypatch.setenv("DCLIP_BF16_BIG_MIN", "1")
            P = ops.gemm_f16_rows_stats_plan(M, N, K)
            assert P == kd.cdiv(M, 256)
            assert ops.gemm_f16_rows_stats_plan(M, N, K + 8) == 0            # K % 64: register-staged whatever the tile count
            g = torch.Generator().manual_seed(M * 1000 + N + K)
            a = (torch.randn((M, K), generator=g) * 8).half().to(dev)
            w = (torch.randn((N, K), generator=g) * 8).half().to(dev)
            ra = torch.exp2(torch.randint(-12, 13, (M,), generator=g).float()).to(dev)
            alpha = torch.tensor([2.0 ** -5], device=dev)
            h = (torch.randn((M, N), generator=g) * 2).to(dev) if dgelu else None
            c0 = ops.gemm_f16_rows_dev(a, w, alpha.data_ptr(), ra, dgelu_h=h)
            assert last_launch() == b"gemm_f16_scaled_rows_dev.pp"
            st, pm, ps = guarded_stats(P, N, dev)
            c1 = ops.gemm_f16_rows_dev(a, w, alpha.data_ptr(), ra, dgelu_h=h, stats=st)
            assert last_launch() == b"gemm_f16_scaled_rows_dev.stats.pp"
            assert same(c0, c1), (M, N, K, dgelu)
            assert float(c1.abs().max()) > 0
            worst = max(worst, check_partials(st, pm, ps, c1, kd.gemm_partition(M), 256, ("gemm", M, N, K, dgelu)))
            assert ps.all_written()
            with pytest.raises(ValueError):
                ops.gemm_f16_rows_dev(a, w, alpha.data_ptr(), ra, dgelu_h=h, stats=guarded_stats(P + 1, N, dev)[0])
    monkeypatch.delenv("DCLIP_BF16_BIG_MIN", raising=False)
    print(f"GEMM statistics K {K} dgelu {dgelu}: psum worst error / bound {worst:.4f}")


def test_gemm_rows_stats_refuses_the_register_staged_kernels(monkeypatch):
    from dclip_amd import _lib, ops
    lib = _lib.load()
    dev = torch.device("cuda:0")
    monkeypatch.delenv("DCLIP_BF16_BIG_MIN", raising=False)
    a, w = torch.zeros((64, 64), dtype=torch.float16, device=dev), torch.zeros((8, 64), dtype=torch.float16, device=dev)
    c, ra, al = torch.zeros((64, 8), device=dev), torch.ones(64, device=dev), torch.ones(1, device=dev)
    pm, ps = torch.zeros((1, 8), dtype=torch.int32, device=dev), torch.zeros((1, 8), device=dev)
    rc = lib.dclip_gemm_f16_scaled_rows_stats_dev(a.data_ptr(), w.data_ptr(), c.data_ptr(), None, 64, 8, 64, 64, 64, 8, 0, al.data_ptr(),
                                                  ra.data_ptr(), pm.data_ptr(), ps.data_ptr(), None)
    assert rc != 0 and b"register-staged" in lib.dclip_last_error()          # a missing kernel is an error, not a fallback
    assert ops.gemm_f16_rows_stats_plan(12800, 3072, 2304) == 50             # the step's dh
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 3. the attention backward

@pytest.mark.parametrize("S", [2, 50, 64])
@pytest.mark.parametrize("causal", [False, True])
def test_attention_bwd_stats(S, causal):
    from dclip_amd import ops
    dev = torch.device("cuda:0")
    B, H = 3, 2
    D = H * 64
    g = torch.Generator().manual_seed(S * 2 + int(causal))
    qkv = torch.randn((B * S, 3 * D), generator=g).to(dev)
    dout = (torch.randn((B * S, D), generator=g) * torch.exp(2.0 * torch.randn((B * S, 1), generator=g))).to(dev)
    out, lse = ops.attention_fwd(qkv, B, S, H, causal)
    d0 = ops.attention_bwd(qkv, out, dout, lse, B, S, H, causal)
    assert last_launch() == b"attention_bwd.lean"
    P = ops.attention_bwd_stats_plan(B, S, H)
    assert P == B
    st, pm, ps = guarded_stats(P, 3 * D, dev)
    d1 = ops.attention_bwd(qkv, out, dout, lse, B, S, H, causal, stats=st)
    name = last_launch()
    assert name == b"attention_bwd.lean.stats" and name.startswith(b"attention_bwd") and b"io16" not in name
    assert same(d0, d1)
    worst = check_partials(st, pm, ps, d1, kd.attention_partition(B, S), S, ("attention", S, causal))
    assert ps.all_written()
    print(f"attention statistics S {S} causal {causal}: psum worst error / bound {worst:.4f}")


def test_attention_bwd_stats_plan_declines():
    from dclip_amd import ops
    assert ops.attention_bwd_stats_plan(3, 1, 2) == 0                        # the one-key kernel
    assert ops.attention_bwd_stats_plan(3, 65, 2) == 0 and ops.attention_bwd_stats_plan(3, 197, 12) == 0
    assert ops.attention_bwd_stats_plan(256, 50, 12) == 256


# ------------------------------------------------------------------------------------------------ 4. LayerNorm backward

@pytest.mark.parametrize("D", [64, 520, 768])
@pytest.mark.parametrize("rows", [1, 5, 300, 4100])
def test_layernorm_bwd_stats(rows, D):
    """4100 rows: past 4096 the 1024 blocks walk a second group of rows; 520: a chunk that is not full; 768: the exact instance"""
    from dclip_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(rows * 7 + D)
    x = torch.randn((rows, D), generator=g).to(dev)
    gamma, beta = (1 + 0.1 * torch.randn(D, generator=g)).to(dev), torch.randn(D, generator=g).to(dev)
    dy = (torch.randn((rows, D), generator=g) * torch.exp(2.0 * torch.randn((rows, 1), generator=g))).to(dev)
    res = torch.randn((rows, D), generator=g).to(dev)
    _, mean, rstd = ops.layernorm_fwd(x, gamma, beta, 1e-5, save_stats=True)
    P = ops.layernorm_bwd_stats_plan(rows, D)
    assert P == kd.ln_blocks(rows)
    for want_params in (True, False):
        for dres in (res, None):
            tag = ("ln", rows, D, want_params, dres is not None)
            colsum = torch.empty(D, device=dev)
            dx0, dg0, db0 = ops.layernorm_bwd(dy, x, gamma, mean, rstd, dresidual=dres, need_param_grads=want_params, dx_colsum=colsum)
            dxp, dgp, dbp = ops.layernorm_bwd(dy, x, gamma, mean, rstd, dresidual=dres, need_param_grads=want_params)
            assert last_launch().startswith(b"layernorm_bwd.nc")
            st, pm, ps = guarded_stats(P, D, dev)
            dx1, dg1, db1 = ops.layernorm_bwd(dy, x, gamma, mean, rstd, dresidual=dres, need_param_grads=want_params, stats=st)
            assert last_launch().startswith(b"layernorm_bwd_stats.nc"), tag
            assert same(dx1, dxp) and same(dx1, dx0), tag
            if want_params:
                assert same(dg1, dgp) and same(db1, dbp), tag
            else:
                assert dg1 is None and db1 is None
            check_partials(st, pm, ps, dx1, kd.ln_partition(rows), kd.cdiv(rows, P) + 4, tag)
            assert ps.all_written(), tag
            fold = kd.fold_reduce_partials(st.psum.cpu().numpy())
            assert np.array_equal(fold.view(np.uint32), colsum.cpu().numpy().view(np.uint32)), tag     # dx_colsum, bit for bit


def test_layernorm_bwd_stats_plan_declines():
    from dclip_amd import ops
    assert ops.layernorm_bwd_stats_plan(100, 1028) == 0 and ops.layernorm_bwd_stats_plan(100, 2048) == 0
    assert ops.layernorm_bwd_stats_plan(12800, 768) == 1024 and ops.layernorm_bwd_stats_plan(100, 1024) == 25
