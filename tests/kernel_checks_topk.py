"""TEST-ONLY checkers, case lists and emulations for the top-k inner-product search, the KNN select and the in-place ReLU
(dclip_amd/csrc/topk.hip; tests/test_topk_paths_gpu.py on the GPU, tests/test_kernel_checks_topk_cpu.py without one).

Nothing here imports the product.  The emulations restate what the kernels are documented to do (include/dclip_hip.h) with
`fault=` switches that plant one subtle defect each; the CPU self-test shows that every checker passes on the fault-free
emulation and fails on its fault.

  * integer operands in [-2, 2]: every dot product is an integer below 2^24 for P <= 512, exact in fp32 in any order, and a
    row has hundreds of equal scores; database rows 1, 4, 7 and 10 are copies of row 0.  Scores and indices must EQUAL
    `topk_reference` (fp64 scores, np.lexsort on (index, -score)): the order among equal scores is part of the contract.
  * Gaussian unit rows (the generator and seeds of kernel_checks_front.build_rank_gauss): with §16's bound
    e_ij = (P + 8) 2^-24 (|q_i| . |d_j|) a row is DETERMINED when every adjacent gap among its fp64-sorted top k + 1 scores
    exceeds the sum of the two bounds; there the indices must equal the fp64 order.  On every row: indices distinct and in
    range, scores non-increasing, indices ascending among bit-equal scores, |score - fp64 score of that index| <= e, and
    no row left out has fp64 score - e above the returned k-th score.
"""
from __future__ import annotations

import numpy as np

from tests import kernel_checks_front as kf

U = 2.0 ** -24
TQ, TD, MAX_SPLITS, TARGET_WGS = 64, 128, 64, 1024
UNDETERMINED_CAP = 0.05

# (Q, N, P, k): one tile, a 64-row edge +-1, N below / at / above a 32- and a 64-row boundary, N < k, one split, many splits
INT_CASES = [(1, 1, 4, 1), (1, 1, 4, 3), (5, 5, 128, 5), (64, 64, 4, 16), (65, 129, 68, 10), (63, 31, 36, 16), (3, 32, 64, 1),
             (3, 33, 64, 3), (300, 77, 64, 10), (130, 1001, 36, 16), (37, 1000, 512, 5), (70, 4100, 64, 10), (2, 20000, 8, 4)]
# split rule by hand: (70, 4100): 2 query blocks, 33 tiles -> want 33, 1 tile per split, 33 splits, the last one of 4 rows;
# (2, 20000): 1 query block, 157 tiles -> want 64, 3 tiles per split, 53 splits, the last one ONE tile of 32 rows.
GAUSS_CASES = [(65, 129, 68, 10), (63, 31, 36, 16), (300, 77, 64, 10), (130, 1001, 36, 16), (37, 1000, 512, 3), (70, 4100, 64, 10)]
REFUSAL_SHAPES = [(3, 32, 64, 1), (65, 129, 68, 10), (300, 77, 64, 10)]
SELECT_SHAPES = [(1, 1, 4), (65, 129, 68), (300, 77, 64)]
RELU_SIZES = [1, 63, 64, 65, 4099]
TOPK_FAULTS = ["tie_high", "pad_row", "last_split", "short_unwritten"]


def case_id(c) -> str:
    return "-".join(str(v) for v in c)


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


def plan(Q: int, N: int):
    """(query blocks, tiles, tiles per split, splits): the rule written in include/dclip_hip.h."""
    qblocks, tiles = cdiv(Q, TQ), cdiv(N, TD)
    want = min(cdiv(TARGET_WGS, qblocks), MAX_SPLITS, tiles)
    per = cdiv(tiles, want)
    return qblocks, tiles, per, cdiv(tiles, per)


def workspace_bytes(Q: int, N: int, k: int) -> int:
    return plan(Q, N)[3] * Q * k * 8


def build_topk_int(Q: int, N: int, P: int):
    rng = np.random.default_rng(Q * 1000 + N)
    q = rng.integers(-2, 3, (Q, P)).astype(np.float32)
    db = rng.integers(-2, 3, (N, P)).astype(np.float32)
    for j in (1, 4, 7, 10):
        if j < N:
            db[j] = db[0]
    return q, db


def build_topk_gauss(Q: int, N: int, P: int):
    s = kf.build_rank_gauss(Q, N, P)
    return s["q"], s["cand"]


def _select(score, index, k: int, tie_high: bool = False):
    """Top k of one row's (score, index) pairs under (score descending, index ascending); NaN scores never qualify."""
    keep = ~np.isnan(score) & (score > -np.inf)
    score, index = score[keep], index[keep]
    order = np.lexsort((-index if tie_high else index, -score))[:k]
    s = np.full(k, -np.inf, np.float64)
    i = np.full(k, -1, np.int64)
    s[:len(order)] = score[order]
    i[:len(order)] = index[order]
    return s, i


def topk_reference(q, db, k: int):
    """(scores [Q,k] fp64, indices [Q,k] int64): fp64 scores (exact for the integer operands), np.lexsort on (index, -score);
    (-inf, -1) where fewer than k rows qualify."""
    sim = q.astype(np.float64) @ db.astype(np.float64).T
    idx = np.arange(db.shape[0], dtype=np.int64)
    rows = [_select(sim[i], idx, k) for i in range(len(q))]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


def emulate_topk(q, db, k: int, fault: str = None):
    """(scores [Q,k] fp32, indices [Q,k] int32) as the two launches compute them: fp32 scores, one sorted partial list per
    (split, query) in a NaN workspace, merged under the same order; outputs start as NaN / a poison index."""
    Q, N = len(q), len(db)
    _, tiles, per, splits = plan(Q, N)
    rows = tiles * TD
    pad = np.zeros((rows, db.shape[1]), np.float32)
    pad[:N] = db
    with np.errstate(invalid="ignore"):
        sim = (q.astype(np.float32) @ pad.T).astype(np.float32).astype(np.float64)
    limit = rows if fault == "pad_row" else N
    part_s = np.full((splits, Q, k), np.nan)
    part_i = np.full((splits, Q, k), kf.POISON_I32, np.int64)
    for s in range(splits):
        if fault == "last_split" and splits > 1 and s == splits - 1:
            part_s[s], part_i[s] = -np.inf, -1
            continue
        lo, hi = s * per * TD, min(min((s + 1) * per, tiles) * TD, limit)
        idx = np.arange(lo, hi, dtype=np.int64)
        for i in range(Q):
            part_s[s, i], part_i[s, i] = _select(sim[i, lo:hi], idx, k, tie_high=fault == "tie_high")
    out_s = np.full((Q, k), np.nan, np.float32)
    out_i = np.full((Q, k), kf.POISON_I32, np.int64)
    for i in range(Q):
        ps, pi = part_s[:, i].reshape(-1), part_i[:, i].reshape(-1)
        live = pi >= 0
        s_, i_ = _select(ps[live], pi[live], k, tie_high=fault == "tie_high")
        n = int((i_ >= 0).sum()) if fault == "short_unwritten" else k
        out_s[i, :n], out_i[i, :n] = s_[:n], i_[:n]
    return out_s, out_i.astype(np.int32)


def check_topk_exact(scores, indices, want_s, want_i, what: str):
    scores, indices = np.asarray(scores, np.float64), np.asarray(indices, np.int64)
    assert scores.shape == want_s.shape and indices.shape == want_i.shape, (what, scores.shape, want_s.shape)
    bad = np.argwhere((indices != want_i) | ~(scores == want_s))        # a NaN (unwritten) score is a difference
    if len(bad):
        i, j = bad[0]
        raise AssertionError(f"{what}: {len(bad)} of {scores.size} slots differ; first at ({i}, {j}): got ({scores[i, j]!r}, "
                             f"{indices[i, j]}), want ({want_s[i, j]!r}, {want_i[i, j]})")


def gauss_reference(q, db, k: int):
    """fp64 scores, §16's bound per element, the fp64 order's first k + 1 columns and which rows are determined."""
    q64, d64 = q.astype(np.float64), db.astype(np.float64)
    sim = q64 @ d64.T
    e = (q.shape[1] + 8) * U * (np.abs(q64) @ np.abs(d64).T)
    N = db.shape[0]
    m = min(k + 1, N)
    order = np.stack([np.lexsort((np.arange(N), -sim[i]))[:m] for i in range(len(q))])
    rows = np.arange(len(q))[:, None]
    s, b = sim[rows, order], e[rows, order]
    determined = ((s[:, :-1] - s[:, 1:]) > (b[:, :-1] + b[:, 1:])).all(axis=1)
    return dict(sim=sim, e=e, order=order, determined=determined)


def check_topk_gauss(scores, indices, ref, k: int, what: str) -> int:
    """Every per-row property of the module docstring; returns the number of undetermined rows."""
    scores, indices = np.asarray(scores, np.float64), np.asarray(indices, np.int64)
    sim, e = ref["sim"], ref["e"]
    Q, N = sim.shape
    n = min(k, N)
    for i in range(Q):
        s, ix = scores[i], indices[i]
        assert (ix[:n] >= 0).all() and (ix[:n] < N).all() and len(set(ix[:n].tolist())) == n, f"{what}: row {i}: indices {ix}"
        assert (ix[n:] == -1).all() and (s[n:] == -np.inf).all(), f"{what}: row {i}: slots past N are not (-inf, -1)"
        assert not np.isnan(s).any() and (s[:-1] >= s[1:]).all(), f"{what}: row {i}: scores not non-increasing: {s}"
        same = s[:n - 1] == s[1:n]
        assert (ix[:n - 1][same] < ix[1:n][same]).all(), f"{what}: row {i}: equal scores out of index order"
        err = np.abs(s[:n] - sim[i, ix[:n]])
        assert (err <= e[i, ix[:n]]).all(), f"{what}: row {i}: score error {err.max():.3e} beyond the bound"
        out = np.ones(N, bool)
        out[ix[:n]] = False
        assert (sim[i, out] - e[i, out] <= s[n - 1]).all(), f"{what}: row {i}: a better row was left out"
        if ref["determined"][i]:
            assert (ix[:n] == ref["order"][i, :n]).all(), f"{what}: determined row {i}: got {ix[:n]}, want {ref['order'][i, :n]}"
    return int((~ref["determined"]).sum())


# ------------------------------------------------------------------------------------------------ select and relu

def build_select(Q: int, N: int, P: int, thresh: float = 3.0):
    """Integer similarities exactly on, one below and one above the threshold; every fifth row has idx -1."""
    rng = np.random.default_rng(Q * 1000 + N)
    db = rng.integers(-2, 3, (N, P)).astype(np.float32)
    fb = rng.integers(3, 6, (Q, P)).astype(np.float32)                  # no value in common with the database
    sim = (thresh + (np.arange(Q) % 3) - 1).astype(np.float32)
    idx = rng.integers(0, N, Q).astype(np.int32)
    idx[np.arange(Q) % 5 == 4] = -1
    if Q >= 3:
        idx[:3] = N - 1                                                 # the three similarities on a valid last row
    return dict(db=db, fb=fb, sim=sim, idx=idx, thresh=thresh)


def emulate_select(s, fault: str = None):
    hit = (s["sim"] > s["thresh"]) if fault == "gt" else (s["sim"] >= s["thresh"])
    hit &= s["idx"] >= 0
    out = np.where(hit[:, None], s["db"][np.clip(s["idx"], 0, None)], s["fb"])
    return out.astype(np.float32), (~hit).astype(np.int32)


def check_select(out, source, s, what: str):
    want_o, want_s = emulate_select(s)
    kf.check_equal(out, want_o, what + " out")
    bad = np.flatnonzero(np.asarray(source, np.int64) != want_s)
    assert not len(bad), f"{what}: source differs on {len(bad)} rows; first row {bad[0]}"


def build_relu(n: int):
    x = np.random.default_rng(n).standard_normal(n).astype(np.float32)
    for pos, v in enumerate((-0.0, np.nan, np.inf, -np.inf, 0.0)):
        if pos < n:
            x[(pos * 13) % n if n > 5 else pos] = v
    if n == 1:
        x[0] = -0.0
    return x


def relu_reference(x):
    with np.errstate(invalid="ignore"):
        return np.where(x < 0, np.float32(0), x).astype(np.float32)     # -0.0 and NaN pass through
