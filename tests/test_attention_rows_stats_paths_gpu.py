"""The statistics twin of the whole-row attention backward (65 .. 80 tokens) on the hardware: dqkv against the
form without statistics bit for bit, the column partials against the exact maxima / fp64 sums of what it stored, guarded
buffers, the launch site, the two plans' ranges, and the single-pass split fed with the partials against the three-launch one."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_checks_dystats as kd                               # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64          # elements before and after a guarded buffer
B, H = 3, 2
D = H * 64


class Guarded:
    """a contiguous buffer of `shape` inside a larger one filled with all-ones bits (a NaN as a float): nothing may be written
    outside, and whatever is left unwritten inside stays visible"""

    def __init__(self, shape, dtype, dev):
        n = int(np.prod(shape))
        self.full = torch.full((n + 2 * GUARD,), -1, dtype=torch.int32, device=dev)
        self.t = self.full[GUARD:GUARD + n].view(dtype).view(*shape)
        self.n = n

    def intact(self):
        f = self.full.cpu()
        return bool((f[:GUARD] == -1).all()) and bool((f[GUARD + self.n:] == -1).all())

    def all_written(self):
        return not bool((self.full[GUARD:GUARD + self.n] == -1).any())


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


def last_launch():
    from dclip_amd import _lib
    return _lib.load().dclip_last_launch()


def inputs(S, causal, dev):
    """as test_dystats_paths_gpu.test_attention_bwd_stats: dout with rows spread over e^(2 N(0,1))"""
    g = torch.Generator().manual_seed(S * 2 + int(causal))
    qkv = torch.randn((B * S, 3 * D), generator=g).to(dev)
    dout = (torch.randn((B * S, D), generator=g) * torch.exp(2.0 * torch.randn((B * S, 1), generator=g))).to(dev)
    return qkv, dout


def run_stats(qkv, out, dout, lse, S, causal, dev):
    from dclip_amd import ops
    pm, ps = Guarded((B, 3 * D), torch.int32, dev), Guarded((B, 3 * D), torch.float32, dev)
    dq = Guarded((B * S, 3 * D), torch.float32, dev)
    from dclip_amd import _lib
    lib = _lib.load()
    rc = lib.dclip_attention_bwd_rows_stats(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), dq.t.data_ptr(),
                                            pm.t.data_ptr(), ps.t.data_ptr(), B, S, H, int(causal),
                                            torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.dclip_last_error()
    assert last_launch() == b"attention_bwd.rows.stats"
    return ops.ColStats.of(pm.t, ps.t), pm, ps, dq


@pytest.mark.parametrize("S", [65, 77, 80])
@pytest.mark.parametrize("causal", [False, True])
def test_attention_bwd_rows_stats(S, causal):
    from dclip_amd import ops
    dev = torch.device("cuda:0")
    qkv, dout = inputs(S, causal, dev)
    out, lse = ops.attention_fwd(qkv, B, S, H, causal)
    d0 = ops.attention_bwd(qkv, out, dout, lse, B, S, H, causal)
    assert last_launch() == b"attention_bwd.rows"
    assert ops.attention_bwd_rows_stats_plan(B, S, H) == B
    tag = ("attention rows", S, causal)
    # through the wrapper: the route of engine.layer_bwd
    st_w = ops.ColStats.of(torch.full((B, 3 * D), -1, dtype=torch.int32, device=dev), torch.full((B, 3 * D), float("nan"), device=dev))
    dw = ops.attention_bwd(qkv, out, dout, lse, B, S, H, causal, rows_stats=st_w)
    assert last_launch() == b"attention_bwd.rows.stats"
    assert same(d0, dw), tag
    # through the C entry, every output in a guarded buffer
    st, pm, ps, dq = run_stats(qkv, out, dout, lse, S, causal, dev)
    assert dq.intact() and dq.all_written() and pm.intact() and ps.intact(), tag
    assert pm.all_written() and ps.all_written(), tag
    assert same(d0, dq.t), tag
    assert float(dq.t.abs().max()) > 0
    assert same(st.pmax, st_w.pmax) and same(st.psum, st_w.psum), tag
    # maxima exact, sums within rows 2^-24 sum|.| of fp64 (an in-order fp32 sum of S terms)
    x = dq.t.cpu().numpy()
    parts = kd.attention_partition(B, S)
    want_max, _ = kd.partials(x, parts)
    assert np.array_equal(st.pmax.cpu().numpy().view(np.uint32), want_max), tag
    got = st.psum.cpu().double().numpy()
    worst = 0.0
    for p, rows in enumerate(parts):
        xd = x[rows].astype(np.float64)
        want, bound = xd.sum(axis=0), S * 2.0 ** -24 * np.abs(xd).sum(axis=0)
        err = np.abs(got[p] - want)
        nz = bound > 0
        if nz.any():
            worst = max(worst, float((err[nz] / bound[nz]).max()))
        assert np.all(err <= bound), (tag, p)
    print(f"attention rows statistics S {S} causal {causal}: psum worst error / bound {worst:.4f}")
    # the same bits in every run
    st2, pm2, ps2, dq2 = run_stats(qkv, out, dout, lse, S, causal, dev)
    assert same(dq.t, dq2.t) and same(st.pmax, st2.pmax) and same(st.psum, st2.psum), tag
    # the single pass fed with these partials against the three-launch split of the same dqkv: five outputs, bit for bit
    db0, db1 = torch.empty((3 * D,), device=dev), torch.empty((3 * D,), device=dev)
    want5 = ops.split_f16x3_rows_colstats(d0, db=db0)
    got5 = ops.split_f16x3_rows_cols_stats(dq.t, st, db=db1)
    assert len(want5) == len(got5) == 5
    assert all(same(a, b) for a, b in zip(got5, want5)), tag
    # the bias gradient of the form without statistics (DCLIP_TEXT_SPLIT16_ROWS_STATS=0): per-caption sums of dqkv folded the same
    # way, the single pass's db bit for bit; in a guarded buffer, from a strided view too
    seg = Guarded((3 * D,), torch.float32, dev)
    ops.colsum_segments(d0, B, S, out=seg.t)
    assert last_launch() == b"colsum_segments_f32.finish"
    assert seg.intact() and seg.all_written() and same(seg.t, db1), tag
    wide = torch.full((B * S, 3 * D + 8), float("nan"), device=dev)
    wide[:, :3 * D] = d0
    assert same(ops.colsum_segments(wide[:, :3 * D], B, S), db1), tag
    with pytest.raises(ValueError):
        ops.colsum_segments(d0, B, S + 1)


def test_attention_bwd_rows_stats_plans():
    from dclip_amd import _lib, ops
    for S in (65, 77, 80):
        assert ops.attention_bwd_rows_stats_plan(3, S, 2) == 3
        assert ops.attention_bwd_stats_plan(3, S, 2) == 0          # the one-tile plan keeps returning 0 above 64
    for S in (1, 64, 81, 197):
        assert ops.attention_bwd_rows_stats_plan(3, S, 2) == 0
    assert ops.attention_bwd_rows_stats_plan(0, 77, 2) == 0 and ops.attention_bwd_rows_stats_plan(3, 77, 0) == 0
    assert ops.attention_bwd_rows_stats_plan(256, 77, 8) == 256
    # a missing form is an error, not a fall-back
    lib = _lib.load()
    dev = torch.device("cuda:0")
    z = torch.zeros(64 * 3 * 128, device=dev)
    rc = lib.dclip_attention_bwd_rows_stats(z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(),
                                            z.data_ptr(), 1, 64, 2, 0, None)
    assert rc != 0 and b"no such form" in lib.dclip_last_error()
    # attention_bwd(stats=...) keeps its check for the one-tile plan
    qkv = torch.zeros((77, 3 * 128), device=dev)
    o = torch.zeros((77, 128), device=dev)
    st = ops.ColStats.of(torch.zeros((1, 3 * 128), dtype=torch.int32, device=dev), torch.zeros((1, 3 * 128), device=dev))
    with pytest.raises(ValueError):
        ops.attention_bwd(qkv, o, o, torch.zeros(2 * 77, device=dev), 1, 77, 2, True, stats=st)
    with pytest.raises(ValueError):
        ops.attention_bwd(qkv[:64 * 1], o[:64], o[:64], torch.zeros(2 * 64, device=dev), 1, 64, 2, True, rows_stats=st)
    torch.cuda.synchronize()
