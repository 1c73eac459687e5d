"""CPU-only self-test of tests/kernel_checks_topk.py: the fault-free emulation of the top-k search, the KNN select and the
ReLU passes every case of tests/test_topk_paths_gpu.py, every planted fault is caught by its checker on at least one listed
case, the workspace formula and split rule give what was worked out by hand, and the Gaussian cases keep their share of
undetermined rows under the cap."""
import functools

import numpy as np
import pytest

from tests import kernel_checks_topk as kt


@functools.lru_cache(maxsize=None)
def int_case(c):
    Q, N, P, k = c
    q, db = kt.build_topk_int(Q, N, P)
    return q, db, kt.topk_reference(q, db, k)


@functools.lru_cache(maxsize=None)
def gauss_case(c):
    Q, N, P, k = c
    q, db = kt.build_topk_gauss(Q, N, P)
    return q, db, kt.gauss_reference(q, db, k)


def test_the_split_rule_and_the_workspace_formula():
    assert kt.plan(70, 4100) == (2, 33, 1, 33) and 4100 - 32 * 128 == 4         # many splits, a last one of 4 rows
    assert kt.plan(2, 20000) == (1, 157, 3, 53) and 20000 - 52 * 3 * 128 == 32  # three tiles per split, a last one of 32 rows
    assert kt.plan(2048, 100_000) == (32, 782, 25, 32)                          # 1024 workgroups: 4 on each of 256 CUs
    assert kt.plan(3, 32)[3] == 1 and kt.plan(65, 129)[3] == 2
    assert kt.workspace_bytes(2048, 100_000, 1) == 32 * 2048 * 8
    assert kt.workspace_bytes(2048, 1_000_000, 16) == 32 * 2048 * 16 * 8        # bounded: 8 MiB, not one slot per 32 rows
    assert max(kt.plan(1, n)[3] for n in (1, 10 ** 5, 10 ** 6, 2 ** 31 - 1)) <= kt.MAX_SPLITS


def test_integer_cases_have_the_ties_the_order_rule_is_about():
    q, db, (want_s, want_i) = int_case((300, 77, 64, 10))
    assert (want_s[:, :-1] == want_s[:, 1:]).sum() > 100
    assert (db[1] == db[0]).all() and (db[10] == db[0]).all()


@pytest.mark.parametrize("c", kt.INT_CASES, ids=kt.case_id)
def test_fault_free_emulation_equals_the_reference(c):
    q, db, (want_s, want_i) = int_case(c)
    s, i = kt.emulate_topk(q, db, c[3])
    kt.check_topk_exact(s, i, want_s, want_i, kt.case_id(c))


@pytest.mark.parametrize("fault", kt.TOPK_FAULTS)
def test_every_topk_fault_is_caught_on_a_listed_case(fault):
    caught = []
    for c in kt.INT_CASES:
        if c[1] > 1100:                      # the two large cases add nothing here: the smaller ones catch every fault
            continue
        q, db, (want_s, want_i) = int_case(c)
        s, i = kt.emulate_topk(q, db, c[3], fault=fault)
        try:
            kt.check_topk_exact(s, i, want_s, want_i, kt.case_id(c))
        except AssertionError:
            caught.append(c)
    assert caught, f"fault {fault!r} passed every case"
    print(fault, "caught on", [kt.case_id(c) for c in caught])


@pytest.mark.parametrize("c", kt.GAUSS_CASES, ids=kt.case_id)
def test_gaussian_cases_pass_the_emulation_and_stay_under_the_ambiguity_cap(c):
    Q, N, P, k = c
    q, db, ref = gauss_case(c)
    s, i = kt.emulate_topk(q, db, k)
    undetermined = kt.check_topk_gauss(s, i, ref, k, kt.case_id(c))
    print(kt.case_id(c), "undetermined rows", undetermined, "of", Q)
    assert undetermined <= kt.UNDETERMINED_CAP * Q


def test_gaussian_checker_catches_a_swapped_pair_and_a_missing_row():
    c = (65, 129, 68, 10)
    q, db, ref = gauss_case(c)
    s, i = kt.emulate_topk(q, db, c[3])
    row = int(np.flatnonzero(ref["determined"])[0])
    swapped_s, swapped_i = s.copy(), i.copy()
    swapped_i[row, [0, 1]] = swapped_i[row, [1, 0]]
    with pytest.raises(AssertionError):
        kt.check_topk_gauss(swapped_s, swapped_i, ref, c[3], "swapped")
    missing_s, missing_i = s.copy(), i.copy()
    missing_s[row, :-1], missing_i[row, :-1] = s[row, 1:], i[row, 1:]          # the best row dropped, the rest moved up
    missing_s[row, -1], missing_i[row, -1] = ref["sim"][row, ref["order"][row, -1]], ref["order"][row, -1]
    with pytest.raises(AssertionError):
        kt.check_topk_gauss(missing_s, missing_i, ref, c[3], "missing")


@pytest.mark.parametrize("shape", kt.SELECT_SHAPES, ids=kt.case_id)
def test_select_emulation_and_its_fault(shape):
    s = kt.build_select(*shape)
    out, source = kt.emulate_select(s)
    kt.check_select(out, source, s, kt.case_id(shape))
    assert {0, 1} >= set(source.tolist())
    bad_out, bad_source = kt.emulate_select(s, fault="gt")
    if shape[0] >= 3:                          # a similarity exactly on the threshold with a valid index exists
        assert 0 in source.tolist() and 1 in source.tolist()
        with pytest.raises(AssertionError):
            kt.check_select(bad_out, bad_source, s, "gt")


@pytest.mark.parametrize("n", kt.RELU_SIZES)
def test_relu_reference_passes_minus_zero_and_nan_through(n):
    x = kt.build_relu(n)
    y = kt.relu_reference(x)
    assert (np.isnan(y) == np.isnan(x)).all() and not (y < 0).any()
    zero = x == 0
    assert (np.signbit(y[zero]) == np.signbit(x[zero])).all()
    if n > 5:
        assert np.isnan(x).any() and np.signbit(x[x == 0]).any() and np.isinf(y).sum() == 1
