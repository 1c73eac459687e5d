"""Every path of dclip_amd/csrc/topk.hip through the C ABI: the top-k inner-product search (MFMA tiles with
running lists, the in-workgroup merge, the split merge), the KNN select and the in-place ReLU.  Integer data: scores and
indices must EQUAL the fp64 / lexsort reference, ties and the (-inf, -1) slots of N < k included.  Gaussian data: exact
indices on every determined row and the interval properties on all rows.  Outputs are guarded, the workspace has exactly
the reported size, is NaN-filled (every partial slot must be written) and guarded behind, operand rows behind Q / N are
NaN.  Checkers: tests/kernel_checks_topk.py.

History: with the first form of the lists (separate score and index arrays) the MI355X failed
test_topk_equals_the_lexsort_reference_on_integer_rows[64-64-4-16] — 9 of 1024 slots, first at (3, 0): got (6.0, 11), want
(6.0, 5) — and the run stopped there.  The lists are 64-bit keys now; that form has not run on the hardware yet."""
import numpy as np
import pytest
import torch

from tests import kernel_checks as kc
from tests import kernel_checks_front as kf
from tests import kernel_checks_topk as kt

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


def vector(n, dev):
    return kc.Guarded(1, n, device=dev, guard_rows=-(-4096 // n))


def behind(values, poison, dtype, dev):
    v = torch.as_tensor(np.asarray(values)).to(dtype)
    t = torch.full((v.numel() + 64,), poison, dtype=dtype, device=dev)
    t[:v.numel()] = v.to(dev)
    return t


def operands(q, db, dev):
    P = q.shape[1]
    return kc.poisoned(torch.from_numpy(q), P, dev), kc.poisoned(torch.from_numpy(db), P, dev)


def unwritten(g):
    return g.get().view(torch.int32) == NAN_BITS


def topk(lib, dev, q, db, Q, N, P, k, workspace_bytes=None):
    """-> (rc, scores [Q,k] fp32, indices [Q,k] int32).  Asserts the size, the guards, the launch name and that every partial
    slot was written."""
    need = int(lib.dclip_topk_ip_workspace(Q, N, k))
    assert need == kt.workspace_bytes(Q, N, k)
    scores, indices, ws = kc.Guarded(Q, k, device=dev), kc.Guarded(Q, k, device=dev), vector(need // 4, dev)
    rc = lib.dclip_topk_ip(q.data_ptr(), db.data_ptr(), scores.ptr, indices.ptr, Q, N, P, k, ws.ptr,
                           need if workspace_bytes is None else workspace_bytes, stream())
    torch.cuda.synchronize()
    scores.assert_guards("scores")
    indices.assert_guards("indices")
    ws.assert_guards("topk workspace")
    if rc != 0:
        assert bool(unwritten(scores).all()) and bool(unwritten(indices).all()) and bool(unwritten(ws).all()), "a refused call wrote"
        return rc, None, None
    assert lib.dclip_last_launch() == b"topk_ip.merge"
    assert not bool(unwritten(ws).any()), "a (split, query, slot) partial was not written"
    assert not bool(unwritten(indices).any()), "an index slot was not written"
    ix = indices.get().view(torch.int32).numpy()
    assert ix.min() >= -1 and ix.max() < N
    return rc, scores.get().numpy(), ix


@pytest.mark.parametrize("c", kt.INT_CASES, ids=kt.case_id)
def test_topk_equals_the_lexsort_reference_on_integer_rows(dev, lib, c):
    Q, N, P, k = c
    q, db = kt.build_topk_int(Q, N, P)
    want_s, want_i = kt.topk_reference(q, db, k)
    dq, ddb = operands(q, db, dev)
    rc, s, i = topk(lib, dev, dq, ddb, Q, N, P, k)
    assert rc == 0, lib.dclip_last_error()
    kt.check_topk_exact(s, i, want_s, want_i, kt.case_id(c))


@pytest.mark.parametrize("c", kt.GAUSS_CASES, ids=kt.case_id)
def test_topk_on_gaussian_rows_exact_where_determined_inside_the_bound_everywhere(dev, lib, c):
    Q, N, P, k = c
    q, db = kt.build_topk_gauss(Q, N, P)
    ref = kt.gauss_reference(q, db, k)
    dq, ddb = operands(q, db, dev)
    rc, s, i = topk(lib, dev, dq, ddb, Q, N, P, k)
    assert rc == 0, lib.dclip_last_error()
    undetermined = kt.check_topk_gauss(s, i, ref, k, kt.case_id(c))
    err = np.abs(s.astype(np.float64) - ref["sim"][np.arange(Q)[:, None], i]) / ref["e"][np.arange(Q)[:, None], i]
    print(kt.case_id(c), "undetermined rows", undetermined, "of", Q, " worst score error / bound", float(err.max()))
    assert undetermined <= kt.UNDETERMINED_CAP * Q


def test_non_finite_rows_are_never_selected_and_form_no_index_out_of_range(dev, lib):
    """Database rows holding NaN and +inf (a score of +inf, -inf or NaN, depending on the query's signs and zeros) and a query
    row of NaN.  fp64 forms the same non-finite scores, so the reference applies as it stands: a NaN or -inf score never
    qualifies, +inf rows come first by index, and the NaN query gets (-inf, -1) in every slot."""
    Q, N, P, k = 65, 129, 68, 10
    q, db = kt.build_topk_int(Q, N, P)
    db[3, 5] = np.nan
    db[64, 0] = np.inf
    db[100, 2] = np.inf
    db[128] = np.nan
    q[7] = np.nan
    with np.errstate(invalid="ignore"):
        want_s, want_i = kt.topk_reference(q, db, k)
    assert (want_i[7] == -1).all() and not np.isin(want_i, (3, 128)).any() and np.isposinf(want_s).any()
    dq, ddb = operands(q, db, dev)
    rc, s, i = topk(lib, dev, dq, ddb, Q, N, P, k)
    assert rc == 0, lib.dclip_last_error()
    kt.check_topk_exact(s, i, want_s, want_i, "non-finite")


@pytest.mark.parametrize("c", kt.REFUSAL_SHAPES, ids=kt.case_id)
def test_topk_refuses_a_workspace_one_byte_short_and_bad_arguments(dev, lib, c):
    Q, N, P, k = c
    q, db = kt.build_topk_int(Q, N, P)
    dq, ddb = operands(q, db, dev)
    need = int(lib.dclip_topk_ip_workspace(Q, N, k))
    rc, _, _ = topk(lib, dev, dq, ddb, Q, N, P, k, workspace_bytes=need - 1)
    assert rc == kc.E_WORKSPACE and b"workspace" in lib.dclip_last_error()
    scores, indices, ws = kc.Guarded(Q, k, device=dev), kc.Guarded(Q, k, device=dev), vector(need // 4, dev)
    ok_args = [dq.data_ptr(), ddb.data_ptr(), scores.ptr, indices.ptr, Q, N, P, k, ws.ptr, need, stream()]
    for pos, bad in [(0, None), (1, None), (2, None), (3, None), (8, None), (4, 0), (4, -1), (5, 0), (5, -1), (6, 0), (6, -4),
                     (6, P + 2), (7, 0), (7, 17)]:
        args = list(ok_args)
        args[pos] = bad
        assert lib.dclip_topk_ip(*args) == kc.E_INVAL, pos
    torch.cuda.synchronize()
    for g in (scores, indices, ws):
        g.assert_guards("refused")
        assert bool(unwritten(g).all()), "a refused call wrote"


@pytest.mark.parametrize("shape", kt.SELECT_SHAPES, ids=kt.case_id)
def test_knn_select_equals_its_restatement_on_below_and_above_the_threshold(dev, lib, shape):
    Q, N, P = shape
    s = kt.build_select(Q, N, P)
    db = kc.poisoned(torch.from_numpy(s["db"]), P, dev)
    fb = kc.poisoned(torch.from_numpy(s["fb"]), P, dev)
    sim = behind(s["sim"], kc.NAN, torch.float32, dev)
    idx = behind(s["idx"], kf.POISON_I32, torch.int32, dev)
    out, source = kc.Guarded(Q, P, device=dev), vector(Q, dev)
    args = [sim.data_ptr(), idx.data_ptr(), db.data_ptr(), fb.data_ptr(), s["thresh"], out.ptr, source.ptr, Q, N, P, stream()]
    assert lib.dclip_knn_select(*args) == 0, lib.dclip_last_error()
    assert lib.dclip_last_launch() == b"knn_select"
    torch.cuda.synchronize()
    out.assert_guards("select out")
    source.assert_guards("select source")
    kt.check_select(out.get().numpy(), source.get().view(torch.int32).numpy()[0], s, kt.case_id(shape))
    fresh_out, fresh_source = kc.Guarded(Q, P, device=dev), vector(Q, dev)
    args[5], args[6] = fresh_out.ptr, fresh_source.ptr
    for pos, bad in [(0, None), (1, None), (2, None), (3, None), (5, None), (6, None), (7, 0), (8, 0), (9, 0)]:
        a = list(args)
        a[pos] = bad
        assert lib.dclip_knn_select(*a) == kc.E_INVAL, pos
    torch.cuda.synchronize()
    assert bool(unwritten(fresh_out).all()) and bool(unwritten(fresh_source).all()), "a refused call wrote"


def test_knn_select_takes_the_fallback_for_an_index_at_or_past_n_and_a_nan_similarity(dev, lib):
    Q, N, P = 5, 7, 8
    s = kt.build_select(Q, N, P)
    s["sim"][:] = 9.0
    s["idx"][:] = [0, N, 2 ** 30, 6, 3]
    s["sim"][4] = np.nan
    db, fb = kc.poisoned(torch.from_numpy(s["db"]), P, dev), kc.poisoned(torch.from_numpy(s["fb"]), P, dev)
    sim, idx = behind(s["sim"], kc.NAN, torch.float32, dev), behind(s["idx"], kf.POISON_I32, torch.int32, dev)
    out, source = kc.Guarded(Q, P, device=dev), vector(Q, dev)
    assert lib.dclip_knn_select(sim.data_ptr(), idx.data_ptr(), db.data_ptr(), fb.data_ptr(), s["thresh"], out.ptr, source.ptr,
                                Q, N, P, stream()) == 0
    torch.cuda.synchronize()
    assert source.get().view(torch.int32).numpy()[0].tolist() == [0, 1, 1, 0, 1]
    want = np.stack([s["db"][0], s["fb"][1], s["fb"][2], s["db"][6], s["fb"][4]])
    kf.check_equal(out.get().numpy(), want, "select edge rows")


@pytest.mark.parametrize("n", kt.RELU_SIZES)
def test_relu_in_place_passes_minus_zero_and_nan_through(dev, lib, n):
    x = kt.build_relu(n)
    g = kc.Guarded(1, n, device=dev, fill=torch.from_numpy(x), guard_rows=-(-4096 // n))
    assert lib.dclip_relu_f32(g.ptr, n, stream()) == 0, lib.dclip_last_error()
    assert lib.dclip_last_launch() == b"relu_f32"
    torch.cuda.synchronize()
    g.assert_guards("relu")
    kf.check_equal(g.get().numpy()[0], kt.relu_reference(x), f"relu n={n}")
    assert lib.dclip_relu_f32(None, n, stream()) == kc.E_INVAL and lib.dclip_relu_f32(g.ptr, 0, stream()) == kc.E_INVAL
