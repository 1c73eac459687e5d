"""Self-test of tests/kernel_checks_split16.py, no GPU: every case of tests/test_split16_paths_gpu.py passes its
checker when the restatement fills the buffers; one planted fault at a time fails the checker relied on for it; the case lists
reach every instance and edge they were written for; and the host functions of dclip_amd.engine agree with the restatements."""
import math

import pytest
import torch

from tests import kernel_checks_rest as kr
from tests import kernel_checks_split16 as ks

INF, NAN = float("inf"), float("nan")


def fails(verify, s, match):
    with pytest.raises(AssertionError, match=match):
        verify(s)


# ---------------------------------------------------------------------------------------------------- the split itself

def test_the_reconstruction_bound_holds_with_little_room():
    """2^-22 |v| + 2^-25 over 2M log-normal values at three scales: never exceeded, and reached to within a few percent."""
    x = (torch.randn(2_000_000, generator=kr.gen(1)) * torch.exp(3.0 * torch.randn(2_000_000, generator=kr.gen(2)))).float()
    worst = 0.0
    for sexp in (0, 9, -3):
        v = x.double() * 2.0 ** sexp
        ok = v.abs() <= ks.RECON_MAX
        hi, lo = ks.host_split(x, 2.0 ** sexp)
        ratio = ((hi.double() + lo.double() - v).abs() / (ks.RECON_REL * v.abs() + ks.RECON_ABS))[ok]
        assert float(ratio.max()) <= 1.0
        worst = max(worst, float(ratio.max()))
    assert worst > 0.9


@pytest.mark.parametrize("c", ks.split_cases(), ids=ks.split_id)
def test_every_split_case_passes_on_the_restatement(c):
    s = ks.build_split(c)
    ks.emulate_split(s)
    ks.verify_split(s)


@pytest.mark.parametrize("fault,match", [("lo_truncated", "y: not the rounding"), ("lo_unscaled", "y: not the rounding"),
                                         ("order", "y: not the rounding"), ("pad", "was written at"), ("behind", "was written at"),
                                         ("scale_written", "scale: memory outside")])
def test_a_planted_split_fault_is_caught(fault, match):
    s = ks.build_split(ks.SplitCase(3, 72, 4, 8, 0, True, 9))
    ks.emulate_split(s, fault)
    fails(ks.verify_split, s, match)


def test_a_truncated_lo_also_breaks_the_reconstruction_bound():
    s = ks.build_split(ks.SplitCase(130, 520, 0, 0, 0, False, 0))
    ks.emulate_split(s, "lo_truncated")
    fails(ks.verify_split, s, r"hi\+lo: .* beyond the bound")


def test_split_cases_reach_every_situation():
    cases = ks.split_cases()
    assert {(c.rows, c.cols) for c in cases} == {(r, n) for r in (1, 3, 130) for n in (8, 72, 520)}
    for rows, cols in {(c.rows, c.cols) for c in cases}:
        mine = [c for c in cases if (c.rows, c.cols) == (rows, cols)]
        assert {(c.xpad, c.ypad, c.order) for c in mine} == {(x, y, o) for x in (0, 4) for y in (0, 8) for o in (0, 1)}
        assert {c.dev for c in mine} == {False, True} and len({c.sexp for c in mine}) == 3
    assert {(c.order, c.dev) for c in cases} == {(o, d) for o in (0, 1) for d in (False, True)}
    for c in ks.split_big_cases():
        assert c.rows * c.cols // 8 > ks.SPLIT_GRID and (c.rows - 1) * c.cols // 8 < ks.SPLIT_GRID + 8192
    assert {(c.order, c.dev) for c in ks.split_big_cases()} == {(0, True), (1, False)}
    x = ks.split_data(cases[-1])
    assert bool(torch.isnan(x).any()) and bool(torch.isinf(x).any()) and bool((x == 0).any())


# ---------------------------------------------------------------------------------------------------- the row split

@pytest.mark.parametrize("c", ks.rows_cases(), ids=ks.rows_id)
def test_every_row_split_case_passes_on_the_restatement(c):
    s = ks.build_rows(c)
    ks.emulate_rows(s)
    ks.verify_rows(s)


@pytest.mark.parametrize("fault,cols,match", [("no_tail", 520, "row_alpha: not bit-identical"), ("no_tail", 3080, "row_alpha"),
                                              ("elem0", 8, "row_alpha: not bit-identical"), ("elem0", 1032, "row_alpha"),
                                              ("clamp99", 72 * 8, "row_alpha"), ("pow2_off", 512, "row_alpha"),
                                              ("alpha_behind", 8, "row_alpha: memory outside"), ("y_behind", 8, "y: memory outside")])
def test_a_planted_row_split_fault_is_caught(fault, cols, match):
    s = ks.build_rows(ks.RowsCase(len(ks.CRAFTED), cols, 4, "crafted"))
    ks.emulate_rows(s, fault)
    fails(ks.verify_rows, s, match)


def test_each_planted_row_fault_shows_in_the_rows_crafted_for_it():
    """Which crafted rows a fault changes: the tail chunk's maximum only in last*, element 0 in every position but 0 and 4, the
    clamp in the subnormal and the huge row, the power of two in its two rows."""
    x = ks.crafted_rows(520, 1)
    want = ks.exp_rule(x.double().abs().amax(dim=1))
    changed = {f: {ks.CRAFTED[r] for r in (ks.exp_rule(ks.faulty_row_max(x, f), 99 if f == "clamp99" else 100,
                                                       1 if f == "pow2_off" else 0) != want).nonzero().flatten().tolist()}
               for f in ("no_tail", "elem0", "clamp99", "pow2_off")}
    assert changed["no_tail"] >= {"last%d" % p for p in range(8)}                # (and the rows whose special value sits there)
    assert not changed["no_tail"] & {"%s%d" % (w, p) for w in ("first", "mid") for p in range(8)}
    assert changed["elem0"] >= {"%s%d" % (w, p) for w in ("first", "last", "mid") for p in (1, 2, 3, 5, 6, 7)}
    assert not changed["elem0"] & {"first0", "first4", "mid0", "last4"}
    assert changed["clamp99"] == {"subnormal", "huge"}
    assert changed["pow2_off"] == {"pow2", "negpow2"}
    e = dict(zip(ks.CRAFTED, want.tolist()))
    assert e["zero"] == e["inf"] == e["nan"] == 0 and e["subnormal"] == 100 and e["huge"] == -100 and e["pow2"] == 14 - 3


def test_rows_cases_reach_every_situation():
    cases = ks.rows_cases()
    assert {ks.rows_variant(c.cols) for c in cases} == {".regs.nc%d" % k for k in range(1, 7)} | {".cached"}
    assert [ks.rows_variant(n) for n in ks.WIDTHS] == [".regs.nc1", ".regs.nc1", ".regs.nc2", ".regs.nc2", ".regs.nc3", ".regs.nc3",
                                                       ".regs.nc4", ".regs.nc4", ".regs.nc5", ".regs.nc5", ".regs.nc6", ".regs.nc6", ".cached"]
    for cols in ks.WIDTHS:
        mine = [c for c in cases if c.cols == cols]
        assert {c.rows for c in mine if c.kind == "random"} == {1, 3, 4, 5, 9}
        assert {c.xpad for c in mine if c.kind == "crafted"} == {0, 4} and {c.xpad for c in mine if c.kind == "random"} == {0, 4}
        x = ks.crafted_rows(cols, 3)
        a = x.abs()
        for r, kind in enumerate(ks.CRAFTED):
            if kind[:-1] in ("first", "last", "mid"):       # the maximum stands alone, three binades above the rest of its row
                top = int(a[r].argmax())
                assert top % 8 == int(kind[-1]) and top // 8 == {"first": 0, "last": cols // 8 - 1, "mid": cols // 16}[kind[:-1]]
                rest = a[r].clone()
                rest[top] = 0
                assert float(rest.max()) * 4 < float(a[r, top])
        assert math.frexp(float(a[ks.CRAFTED.index("pow2")].max()))[0] == 0.5
        assert 0 < float(a[ks.CRAFTED.index("subnormal")].max()) < 2.0 ** -126
        assert float(a[ks.CRAFTED.index("huge")].max()) >= 2.0 ** 115


# ---------------------------------------------------------------------------------------------------- the fused pass

@pytest.mark.parametrize("c", ks.col_cases(), ids=ks.col_id)
def test_every_fused_pass_case_passes_on_the_restatement(c):
    s = ks.build_col(c)
    ks.emulate_col(s)
    ks.verify_col(s)


@pytest.mark.parametrize("fault,case,match", [
    ("wave_last_row", ks.ColCase(9, 520, 4, "dyadic", True), "col_exp: not exact.*db: not exact"),
    ("wave_last_row", ks.ColCase(33, 8, 0, "dyadic", True), "db: not exact"),
    ("wave_last_row", ks.ColCase(33, 8, 0, "spread", True), "col_exp|db"),
    ("fold_W", ks.ColCase(2, 8, 0, "dyadic", True), "db: not exact"),
    ("fold_W", ks.ColCase(3, 520, 4, "spread", True), "db: .*non-finite"),
    ("neighbour_col", ks.ColCase(5, 72 * 8, 4, "dyadic", False), "yc: not the rounding"),
    ("ws_behind", ks.ColCase(5, 8, 0, "dyadic", True), "workspace: 1 of the 1024 floats"),
    ("yc_behind", ks.ColCase(5, 8, 0, "dyadic", True), "yc: memory outside"),
    ("ce_behind", ks.ColCase(5, 8, 0, "dyadic", True), "col_exp: memory outside")])
def test_a_planted_fused_pass_fault_is_caught(fault, case, match):
    s = ks.build_col(case)
    ks.emulate_col(s, fault)
    fails(ks.verify_col, s, match)


def test_a_null_db_must_stay_unwritten():
    s = ks.build_col(ks.ColCase(5, 8, 0, "dyadic", False))
    ks.emulate_col(s)
    s.db.payload[0, 3] = 1.0
    fails(ks.verify_col, s, "db: written although")


def test_col_cases_reach_every_situation():
    cases = ks.col_cases()
    assert {ks.rows_variant(c.cols) for c in cases} == {".regs.nc%d" % k for k in range(1, 7)} | {".cached"}
    for cols in ks.WIDTHS:
        mine = [c for c in cases if c.cols == cols and c.rows < 100]
        assert {c.rows for c in mine} == {1, 2, 3, 4, 5, 8, 9, 33}
        assert {c.kind for c in mine} == {"dyadic", "spread"} and {c.db for c in mine} == {False, True} and {c.xpad for c in mine} == {0, 4}
    big = [c for c in cases if c.rows == 8200]
    assert {(c.cols, c.kind) for c in big} == {(n, k) for n in (8, 520) for k in ("dyadic", "spread")}
    assert all(c.rows * c.cols // 8 > ks.SPLIT_GRID and c.kind == "dyadic" for c in ks.col_big_cases())       # (GPU only: 17M elements)
    assert ks.rows_variant(520) == ".regs.nc2"                                    # the two-chunk width
    # the waves: rows < W leaves waves without a row; at 8200 rows the cap holds and eight waves walk nine rows
    assert [ks.col_waves(r) for r in (1, 2, 3, 4, 5, 8, 9, 33, 8200)] == [4, 4, 4, 4, 4, 4, 4, 8, 1024]
    assert sum(len(range(w, 8200, 1024)) == 9 for w in range(1024)) == 8
    assert ks.col_workspace_floats(8200, 520) == 2 * 1024 * 520 and ks.col_workspace_floats(3, 8) == 2 * 4 * 8
    for rows in (1, 2, 3, 4, 5, 8, 9, 33, 8200):
        W = ks.col_waves(rows)
        r = ks.last_wave_row(rows)
        assert r % W == min(W, rows) - 1 and r + W >= rows
        x = ks.col_data(ks.ColCase(rows, 72, 0, "dyadic", True))
        top = x.abs().argmax(dim=0)
        assert set(top.tolist()) == {0, rows - 1, r}
        if rows > 2:
            assert bool((x.abs().sort(dim=0).values[-1] >= 2 * x.abs().sort(dim=0).values[-2]).all())      # the maximum stands alone
    x = ks.col_data(ks.ColCase(9, 72, 0, "spread", True))
    e = ks.exp_rule(x.double().abs().amax(dim=0))
    assert e[:4].tolist() == [0, 0, 0, 100] and int(e[4]) == 14 - 34 and not bool(x[:, 0].any()) and bool(torch.isnan(x[:, 2]).any())


# ---------------------------------------------------------------------------------------------------- LayerNorm

@pytest.mark.parametrize("c", ks.ln_cases(), ids=str)
def test_every_layernorm_case_passes_on_the_restatement(c):
    s = ks.build_ln(c)
    ks.emulate_ln(s)
    ks.verify_ln(s)


@pytest.mark.parametrize("fault,match", [("one_rounding", "y: not the rounding"), ("host_differs", "y_host against the call"),
                                         ("y_behind", "y_dev: memory outside"), ("chunk_unwritten", "y: not the rounding")])
def test_a_planted_layernorm_fault_is_caught(fault, match):
    s = ks.build_ln(ks.LnCase(516, 5, 9))
    ks.emulate_ln(s, fault)
    fails(ks.verify_ln, s, match)


def test_ln_cases_reach_every_situation():
    cases = ks.ln_cases()
    assert {ks.ln_variant(c.D) for c in cases} == {".nc1", ".nc2", ".nc3", ".nc4", ".nc8", ".nc2.exact", ".nc3.exact", ".nc4.exact"}
    want = {4: 1, 8: 1, 72: 1, 252: 1, 256: 1, 260: 2, 384: 2, 508: 2, 516: 3, 640: 3, 764: 3, 772: 4, 896: 4, 1020: 4, 1028: 8,
            1280: 8, 2044: 8, 2048: 8}
    assert all(ks.ln_variant(D) == ".nc%d" % k for D, k in want.items())
    assert {c.D for c in cases} == set(want) | {512, 768, 1024}
    for D in {c.D for c in cases}:
        assert {c.rows for c in cases if c.D == D} == {1, 3, 4, 5, 9}
    assert {c.sexp for c in cases} == {0, 9, -3, 6}


# ---------------------------------------------------------------------------------------------------- the device plan

@pytest.mark.parametrize("c", ks.PLAN_CASES, ids=ks.plan_id)
def test_every_plan_case_passes_on_the_restatement(c):
    s = ks.build_plan(c)
    ks.emulate_plan(s)
    ks.verify_plan(s)


@pytest.mark.parametrize("fault,match", [("l1_all_rows", "plan: not bit-identical"), ("stats_not_cleared", "stats: the accumulators"),
                                         ("no_flag4", "plan: not bit-identical"), ("t_last_group", "dst_t2: not the rounding"),
                                         ("dst_behind", "dst2: memory outside"), ("plan_behind", "plan: memory outside")])
def test_a_planted_plan_fault_is_caught(fault, match):
    s = ks.build_plan(ks.PLAN_CASES[3])
    ks.emulate_plan(s, fault)
    fails(ks.verify_plan, s, match)


def test_stale_statistics_change_the_plan():
    """Maxima that are not cleared show in the plan too, not only in the accumulators: the first round's weights are 4x larger."""
    s = ks.build_plan(ks.PLAN_CASES[2])
    stale, _ = ks.plan_expect(s, stats=ks.exact_stats(s, 4.0))
    fresh, _ = ks.plan_expect(s)
    assert not torch.equal(stale[:, :12], fresh[:, :12])


def test_plan_cases_reach_every_situation():
    assert ks.RECORD.size == ks.RECORD_BYTES == 48
    five = ks.build_plan(ks.PLAN_CASES[3])
    assert len(ks.build_plan(ks.PLAN_CASES[0]).recs) == 1 and len(five.recs) == 50
    _, flags = ks.plan_expect(five)
    assert flags == [0, 1, 2, 4, 5]                                               # 5: a ctx bound beyond 2^140 is also below 2^-14
    mats = [r for r in five.recs if r.dst]
    assert {r.rows for r in mats} == {8, 32, 40, 72} and {r.cols for r in mats} == {8, 64, 72, 136}
    assert any(r.cols % 64 and r.cols > 64 and r.dst_t for r in mats) and any(r.rows % 32 == 8 and r.dst_t for r in mats)
    assert any(r.dst and not r.dst_t for r in five.recs)                          # a NULL entry of dst_t
    assert any(0 < r.l1_row0 and r.l1_row0 % 32 for r in five.recs)               # l1_row0 inside a tile
    kinds = [bool(r.dst) for r in five.recs[:10]]
    assert kinds[0] is False and any(a and not b and c for a, b, c in zip(kinds, kinds[1:], kinds[2:]))     # statistics only, between
    assert five.tile0[-1] + 1 == five.tiles == 5 * (6 + 3 + 2 + 1 + 1)            # the search meets first, middle and last records
    st = ks.exact_stats(five)
    assert float(st[3, 11]) == 2.0 ** -121 and math.isnan(float(st[2, 10])) and float(st[4, 0]) * float(st[4, 2]) > 2.0 ** 140
    plan, _ = ks.plan_expect(five)
    assert float(plan[3, 7]) == 2.0 ** 127 and float(plan[3, 31]) == 2.0 ** -126 and float(plan[4, 1]) == 2.0 ** -126
    assert not bool(plan[:, 13:16].any())


# ---------------------------------------------------------------------------------------------------- the product's host functions

def test_the_engines_host_functions_agree_with_the_restatements():
    from dclip_amd import engine
    r = torch.tensor([0.0, INF, NAN, 1.0, 0.5, 0.75, 2.0 ** 14, 2.0 ** 14 * 0.999, 2.0 ** -149, 2.0 ** -130, 2.0 ** 115, 3e38, 1e-30,
                      1e10], dtype=torch.float64)
    assert ks.exp_rule(r).tolist() == [engine.split16_row_exp(float(v)) for v in r] == [engine.split16_col_exp(float(v)) for v in r]
    x = ks.crafted_rows(520, 5)
    y, ra = engine.split16_rows_host(x)
    want_y, want_ra, _ = ks.rows_expect(x)
    rep = kr.Report("split16_rows_host")
    rep.rounded16("y", y, want_y)
    rep.bits("row_alpha", ra, want_ra)
    rep.done()
    five = ks.build_plan(ks.PLAN_CASES[3])
    st = ks.exact_stats(five)
    for l in range(five.nlayers):
        row = st[l].tolist()
        rec, flags = ks.plan_rule(row, ks.PLAN_D)
        host = engine.split16_plan_host(dict(zip(engine._SPLIT16_STATS, row)), ks.PLAN_D)
        assert host["flags"] == flags
        assert [2.0 ** host["e"][k] for k in ("ln1", "ctx", "ln2", "g")] == rec[0:4]
        assert [2.0 ** host["f"][k] for k in ("qkv", "out", "fc1", "fc2")] == rec[4:8]
        assert [2.0 ** host["a"][k] for k in ("qkv", "out", "fc1", "fc2")] == rec[8:12]
    for b in (0.0, 1.0, 2.0 ** 14, 2.0 ** 14 + 1, 2.0 ** -20, 3.7, 2.0 ** 28):
        rec, flags = ks.plan_rule([b, 0.0] + [0.0] * 10, 1)
        assert flags == 0 and rec[0] == 2.0 ** engine.split16_act_exp(b)
    for w in (0.0, 1.0, 0.3, 2.0 ** 13, 1e-9):
        rec, _ = ks.plan_rule([0.0] * 8 + [w, 0.0, 0.0, 0.0], 1)
        assert rec[4] == 2.0 ** engine.split16_weight_exp(w)



# ---------------------------------------------------------------------------------------------------- the segmented weight gradient

@pytest.mark.parametrize("c", ks.seg_cases(), ids=ks.seg_id)
def test_every_segmented_gemm_case_passes_on_the_restatement(c):
    s = ks.build_seg(c)
    ks.emulate_seg(s)
    ks.verify_seg(s)


@pytest.mark.parametrize("fault,match", [("seg_twice", "C: not exact"), ("slab_left_out", "C: not exact"),
                                         ("slab_unwritten", "workspace: 1 words"), ("ws_behind", "workspace: wrote behind"),
                                         ("c_pad", "C: memory outside")])
@pytest.mark.parametrize("perm", [False, True])
def test_a_planted_segmented_gemm_fault_is_caught(fault, match, perm):
    s = ks.build_seg(ks.SegCase(264, 8, 320, 3, perm))
    ks.emulate_seg(s, fault)
    fails(ks.verify_seg, s, match)


def test_seg_cases_reach_every_situation():
    cases = ks.seg_cases()
    assert {(c.tokens, c.splits) for c in cases} == {(t, k) for t in (64, 192, 320) for k in (1, 2, 3, 7, 21)}
    sizes = {(m, n) for m in (8, 264, 520) for n in (8, 264, 520)}
    for t in (64, 192, 320):
        assert {(c.M, c.N) for c in cases if c.tokens == t} == sizes
    for k in (1, 2, 3, 7, 21):
        assert {(c.M, c.N) for c in cases if c.splits == k} == sizes
    assert {(c.M, c.N, c.perm) for c in cases} >= {(m, n, p) for m, n in sizes for p in (False, True)}
    assert [ks.seg_s_eff(320, k) for k in (1, 2, 3, 7, 21)] == [(320, 1), (192, 2), (128, 3), (64, 5), (64, 5)]      # s_eff < splits
    assert ks.seg_s_eff(64, 21) == (64, 1) and ks.seg_s_eff(192, 2) == (128, 2)
    s = ks.build_seg(ks.SegCase(8, 264, 192, 2, False))
    assert bool(torch.isnan(s.x[:, 2 * 264:]).all()) and bool(torch.isfinite(s.x[:, :2 * 264]).all())     # the step reads two pieces of X
    assert bool(torch.isnan(s.dyd[192:].float()).all()) and bool(torch.isnan(s.dyd[:, 16:].float()).all())
    assert s.ws_bytes == 3 * 2 * 8 * 264 * 4
    assert len(set(ks.build_seg(ks.SegCase(264, 8, 64, 1, True)).ca[:41].tolist())) == 41


# ---------------------------------------------------------------------------------------------------- the scaled GEMM entries

SCALED_CPU = [c for c in ks.scaled_cases() if c.kernel != "r128"] + \
             [ks.ScaledCase(e, "r128", 2047, 2044, 72, 1) for e in ("rows_dgelu", "split_dev_gelu_hg")]      # the rest of .r128: GPU only


@pytest.mark.parametrize("c", SCALED_CPU, ids=ks.scaled_id)
def test_every_scaled_gemm_case_passes_on_the_restatement(c):
    s = ks.build_scaled(c)
    ks.emulate_scaled(s)
    ks.verify_scaled(s)


@pytest.mark.parametrize("fault,entry,match", [
    ("alpha_after_bias", "scaled_dev", "C: not exact"), ("alpha_after_bias", "split_dev_gelu_hg", "h32: not exact"),
    ("row_alpha_next", "rows_dev", "C: not exact"), ("row_alpha_next", "rows_dgelu", "C: .* beyond the bound"),
    ("row_alpha_first", "rows_big", "C: "), ("aux_row_next", "rows_dgelu", "C: .* beyond the bound"),
    ("lo_dropped", "split", "C: not the rounding"), ("lo_dropped", "split_gelu", r"C \(hi\+lo\)/out_scale: .* beyond the bound"),
    ("lo_dropped", "split_dev_gelu_g", "C: not the rounding"), ("lo_negzero", "split_negzero", "C: not the rounding"),
    ("third_piece_off", "split_dev", "C: "), ("third_piece_off", "split_dev_gelu", "C: the third piece"),
    ("g32_stride_ldc", "split_dev_g32", "g32: "), ("g32_stride_ldc", "split_dev_gelu_hg", "g32: "),
    ("h32_stride_ldc", "split_dev_gelu_h", "h32: "), ("h32_stride_ldc", "split_dev_noscale_gelu_h", "h32: "),
    ("h32_is_g", "split_dev_gelu_hg", "h32: not exact")])
def test_a_planted_scaled_gemm_fault_is_caught(fault, entry, match):
    s = ks.build_scaled(ks.ScaledCase(entry, "pp", 300, 264, 128, 1))
    ks.emulate_scaled(s, fault)
    fails(ks.verify_scaled, s, match)


def test_scaled_cases_reach_every_situation():
    cases = ks.scaled_cases()
    forms = {e: ks.scaled_form(ks.ScaledCase(e, "r64", 8, 8, 8, 0)) for e in ks.GEMM_ENTRIES}
    assert {f.fn for f in forms.values()} == {"scaled", "scaled_dev", "rows_dev", "split", "split_dev"}
    for k in ("r64", "r128", "pp"):                        # every form on every kernel but the persistent one
        assert {c.entry for c in cases if c.kernel == k} == set(ks.GEMM_ENTRIES)
    assert {c.entry for c in cases if c.kernel == "pp_persist"} == set(ks.GEMM_ENTRIES) - {"scaled"}
    assert {forms[c.entry].fn for c in cases if c.kernel == "pp_persist"} == {"scaled_dev", "rows_dev", "split", "split_dev"}
    assert all(ks.scaled_site(c).endswith(".pp") for c in cases if c.kernel == "pp_persist")
    ppp = [c for c in cases if c.kernel == "ppp"]
    assert {c.entry for c in ppp} == {"scaled"} and sorted(-(-c.M // 256) * -(-c.N // 256) for c in ppp) == [1, 7, 9]
    assert all(ks.scaled_env(c) == ks.ENV_PERSIST and ks.build_scaled(c).ldc % 8 == 0 for c in ppp)
    assert {(c.M, c.N, c.K) for c in cases if c.kernel == "r128"} == {(2047, 2044, 72)}
    for c in cases:
        t128, t256 = -(-c.M // 128) * -(-c.N // 128), -(-c.M // 256) * -(-c.N // 256)
        if c.kernel == "r64":
            assert t128 < 256
        elif c.kernel == "r128":
            assert t128 >= 256 and c.K % 64 != 0
        else:
            assert c.K % 64 == 0 and t256 >= 1
    assert all(c.N % 256 and c.M % 256 for c in cases if c.kernel == "pp")       # ragged last tile row and column on the ping-pong kernel
    assert {c.cpad for c in cases if ks.scaled_is_split(c) and c.kernel == "pp"} == {0, 1}
    assert ks.build_scaled(ks.ScaledCase("split", "pp", 257, 260, 64, 1)).ldc == 784 + 8        # 3N rounded to 8 where N % 8 = 4
    # the epilogues: DGELU with aux32 (ldc > N, NaN padding and rows behind M), GELU with h32 / g32 each NULL and given
    gelu = {(f.h32, f.g32) for f in forms.values() if f.epi & ks.EPI_GELU and f.fn == "split_dev" and f.split}
    assert gelu == {(a, b) for a in (False, True) for b in (False, True)}
    assert {f.g32 for f in forms.values() if f.fn == "split_dev" and f.split and not f.epi & ks.EPI_GELU} == {False, True}
    assert {bool(f.epi & ks.EPI_DGELU) for f in forms.values() if f.fn == "rows_dev"} == {False, True}
    s = ks.build_scaled(ks.ScaledCase("rows_dgelu", "pp", 257, 260, 64, 1))
    assert s.ldc > 260 and bool(torch.isnan(s.aux_d[:, 260:]).all()) and bool(torch.isnan(s.aux_d[257:]).all())
    big = ks.build_scaled(ks.ScaledCase("rows_big", "r64", 130, 72, 40, 0))
    assert set(big.ra.tolist()) == {2.0 ** 100, 2.0 ** -60} and float(big.lin.abs().max()) < 3e38
    assert not bool(torch.isfinite(((big.a @ big.w.t()) * big.ra[:, None])).all())            # the other order overflows
