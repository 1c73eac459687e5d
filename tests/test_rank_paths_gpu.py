"""Every path of the ranking kernels through the C ABI: MODE_RANK of the fp32 GEMM, rank_merge_kernel and
rowdot_gather_kernel (dclip_amd/csrc/gemm_f32.hip).  Integer data: the count must EQUAL the int64 count, with exact ties,
bit-identical copies of the ground truth, gt NULL / -1 / Bk and thresholds below and above every score.  Gaussian data: every
row inside the interval that §16's GEMM bound allows, and the interval is asserted tight.  count and out are guarded, the
workspace has exactly the reported size, is NaN-filled (every partial slot must be written, the empty second sub-tile at
Bk <= 32 included) and guarded behind, operand rows behind Bq / Bk are NaN.  Checkers: tests/kernel_checks_front.py."""
import numpy as np
import pytest
import torch

from tests import kernel_checks as kc
from tests import kernel_checks_front as kf

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


def vector(n, dev):
    return kc.Guarded(1, n, device=dev, guard_rows=-(-4096 // n))


def behind(values, poison, dtype, dev):
    v = torch.as_tensor(np.asarray(values)).to(dtype)
    t = torch.full((v.numel() + 64,), poison, dtype=dtype, device=dev)
    t[:v.numel()] = v.to(dev)
    return t


def operands(s, dev):
    P = s["q"].shape[1]
    return kc.poisoned(torch.from_numpy(s["q"]), P, dev), kc.poisoned(torch.from_numpy(s["cand"]), P, dev)


def rank_count(lib, dev, q, cand, thr, gt, Bq, Bk, P, workspace_bytes=None):
    """-> (rc, count [Bq] int64 or None).  Asserts the size, the guards, the launch name and that every partial was written."""
    need = int(lib.dclip_rank_count_workspace(Bq, Bk))
    assert need == kf.rank_slots(Bk) * Bq * 4
    count, ws = vector(Bq, dev), vector(need // 4, dev)
    t = behind(thr, kc.NAN, torch.float32, dev)
    g = None if gt is None else behind(gt, kf.POISON_I32, torch.int32, dev)
    rc = lib.dclip_rank_count(q.data_ptr(), cand.data_ptr(), t.data_ptr(), None if g is None else g.data_ptr(), count.ptr, Bq, Bk, P,
                              ws.ptr, need if workspace_bytes is None else workspace_bytes, stream())
    torch.cuda.synchronize()
    count.assert_guards("count")
    ws.assert_guards("rank workspace")
    if rc != 0:
        assert bool(torch.isnan(count.get()).all()) and bool(torch.isnan(ws.get()).all()), "a refused call wrote"
        return rc, None
    assert lib.dclip_last_launch() == b"rank_count.merge"
    assert not bool(torch.isnan(ws.get()).any()), "a (slot, row) partial was not written"
    return rc, count.get().view(torch.int32).numpy()[0].astype(np.int64)


def rowdot(lib, dev, a, b, idx, Bq, Bk, P):
    out = vector(Bq, dev)
    i = None if idx is None else behind(idx, kf.POISON_I32, torch.int32, dev)
    rc = lib.dclip_rowdot_gather(a.data_ptr(), b.data_ptr(), None if i is None else i.data_ptr(), out.ptr, Bq, Bk, P, stream())
    assert rc == 0, lib.dclip_last_error()
    assert lib.dclip_last_launch() == b"rowdot_gather"
    torch.cuda.synchronize()
    out.assert_guards("rowdot out")
    return out.get().numpy()[0]


@pytest.mark.parametrize("case", kf.rank_int_cases(), ids=kf.rank_id)
def test_rank_count_equals_the_int64_count(dev, lib, case):
    s = kf.build_rank_int(case)
    q, cand = operands(s, dev)
    rc, count = rank_count(lib, dev, q, cand, s["thr"], s["gt"], case.Bq, case.Bk, case.P)
    assert rc == 0, lib.dclip_last_error()
    kf.check_rank_exact(count, s["want"], kf.rank_id(case))


@pytest.mark.parametrize("shape", kf.RANK_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_rowdot_gather_equals_the_integer_dot_with_the_documented_clamp(dev, lib, shape):
    """idx NULL pairs row i with row min(i, Bk - 1); idx -1 and Bk are clamped to 0 and Bk - 1 (include/dclip_hip.h)."""
    Bq, Bk, P = shape
    s = kf.build_rank_int(kf.RankCase(Bq, Bk, P, "given", "ties"))
    q, cand = operands(s, dev)
    assert np.array_equal(rowdot(lib, dev, q, cand, s["idx"], Bq, Bk, P).astype(np.float64), s["dot_idx"].astype(np.float64))
    assert np.array_equal(rowdot(lib, dev, q, cand, None, Bq, Bk, P).astype(np.float64), s["dot_null"].astype(np.float64))


@pytest.mark.parametrize("shape", kf.RANK_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_gaussian_rows_every_row_inside_a_tight_interval(dev, lib, shape):
    Bq, Bk, P = shape
    s = kf.build_rank_gauss(Bq, Bk, P)
    q, cand = operands(s, dev)
    own = s["cand"][s["gt"]]
    thr = rowdot(lib, dev, q, cand, s["gt"], Bq, Bk, P)
    err = np.abs(thr.astype(np.float64) - (s["q"].astype(np.float64) * own.astype(np.float64)).sum(axis=1))
    bound = kf.rowdot_bound(s["q"], own)
    print(shape, "rowdot worst got / bound", float((err / bound).max()))
    assert (err <= bound).all()
    rc, count = rank_count(lib, dev, q, cand, thr, s["gt"], Bq, Bk, P)
    assert rc == 0, lib.dclip_last_error()
    lo, hi = kf.rank_interval(s["q"], s["cand"], thr, s["gt"])
    print(shape, "slack, total", kf.check_rank_interval(count, lo, hi, str(shape)))


def test_duplicates_of_the_ground_truth_may_be_counted_and_nothing_else(dev, lib):
    """Three candidates are bit-identical to the ground truth of three rows: rowdot_gather and the MFMA tile evaluate the same
    dot product in two orders, so each duplicate may or may not score above the threshold (include/dclip_hip.h)."""
    Bq, Bk, P = 65, 129, 68
    s = kf.build_rank_gauss(Bq, Bk, P, dup=True)
    q, cand = operands(s, dev)
    thr = rowdot(lib, dev, q, cand, s["gt"], Bq, Bk, P)
    rc, count = rank_count(lib, dev, q, cand, thr, s["gt"], Bq, Bk, P)
    assert rc == 0, lib.dclip_last_error()
    lo, hi = kf.rank_interval(s["q"], s["cand"], thr, s["gt"], exclude=s["dups"])
    kf.check_rank_interval(count, lo, hi, "duplicates", extra=s["dups"].sum(axis=1))


@pytest.mark.parametrize("shape", [(3, 32, 64), (65, 129, 68), (300, 77, 64)], ids=lambda s: "-".join(map(str, s)))
def test_rank_count_refuses_a_workspace_one_byte_short_and_bad_arguments(dev, lib, shape):
    Bq, Bk, P = shape
    s = kf.build_rank_int(kf.RankCase(Bq, Bk, P, "given", "half"))
    q, cand = operands(s, dev)
    need = int(lib.dclip_rank_count_workspace(Bq, Bk))
    rc, _ = rank_count(lib, dev, q, cand, s["thr"], s["gt"], Bq, Bk, P, workspace_bytes=need - 1)
    assert rc == kc.E_WORKSPACE and b"workspace" in lib.dclip_last_error()
    count, ws, t = vector(Bq, dev), vector(need // 4, dev), behind(s["thr"], kc.NAN, torch.float32, dev)
    ok_args = [q.data_ptr(), cand.data_ptr(), t.data_ptr(), None, count.ptr, Bq, Bk, P, ws.ptr, need, stream()]
    for pos, bad in [(0, None), (1, None), (2, None), (4, None), (5, 0), (6, 0), (7, 0), (7, P + 2)]:
        args = list(ok_args)
        args[pos] = bad
        assert lib.dclip_rank_count(*args) == kc.E_INVAL, pos
    out = vector(Bq, dev)
    for pos, bad in [(0, None), (1, None), (3, None), (4, 0), (5, 0), (6, 0)]:
        args = [q.data_ptr(), cand.data_ptr(), None, out.ptr, Bq, Bk, P, stream()]
        args[pos] = bad
        assert lib.dclip_rowdot_gather(*args) == kc.E_INVAL, pos
    torch.cuda.synchronize()
    for g in (count, ws, out):
        g.assert_guards("refused")
        assert bool(torch.isnan(g.get()).all()), "a refused call wrote"
