"""Self-test of tests/kernel_checks_front.py, no GPU: every case of tests/test_front_paths_gpu.py, evaluated by
the numpy restatement of the two-pass resample, equals Pillow bit for bit; one planted fault at a time fails the checker
relied on for it; the case lists contain every situation they were written for; the ranking checkers pass on an fp32
evaluation, fail on each planted fault, and their interval is tight."""
import numpy as np
import pytest
import torch

from tests import kernel_checks as kc
from tests import kernel_checks_front as kf


def emulate_crop(r, fault=None, boxes=None):
    batch, dims, bx, mh, mw = kf.crop_case(r)
    bx = bx if boxes is None else boxes
    KS = kf.ksize_for(max(mh, mw), r.S, kf.BILINEAR)
    return kf.emulate(batch, dims, kf.plan_from_boxes(bx.tolist(), r.S), r.S, mh, KS, kf.BILINEAR, None, fault), bx


def emulate_pre(S, norm, fault=None):
    batch, dims = kf.pre_batch(S)
    _, Hmax, Wmax, _ = batch.shape
    KS = kf.ksize_for(max(Hmax, Wmax), S, kf.BICUBIC)
    return kf.emulate(batch, dims, kf.plan_shortest_edge(dims.tolist(), S, fault), S, Hmax, KS, kf.BICUBIC, kf.NORMS[norm], fault)


# ---- every case equals Pillow --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("run", kf.crop_runs(), ids=kf.crop_id)
def test_every_crop_case_equals_pillow(run):
    got, boxes = emulate_crop(run)
    kf.check_equal(got, kf.crop_want(run, boxes), kf.crop_id(run))


@pytest.mark.parametrize("norm", list(kf.NORMS))
@pytest.mark.parametrize("S", kf.PRE_S)
def test_every_preprocessing_case_equals_pillow(S, norm):
    kf.check_equal(emulate_pre(S, norm), kf.pre_expected(S, norm), f"preprocess S={S} {norm}")


def ramp_crop(fault=None):
    batch, dims = kf.make_batch([kf.ramp_image()], 19, 21)
    return kf.emulate(batch, dims, kf.plan_from_boxes([(0, 0, 0, 16, 16)], 16), 16, 16, 3, kf.BILINEAR, None, fault)[0]


def ramp_pre(norm, fault=None):
    batch, dims = kf.make_batch([kf.ramp_image()], 19, 21)
    KS = kf.ksize_for(21, 16, kf.BICUBIC)
    return kf.emulate(batch, dims, kf.plan_shortest_edge(dims.tolist(), 16), 16, 19, KS, kf.BICUBIC, kf.NORMS[norm], fault)[0]


def ramp_want_crop():
    return (kf.ramp_image().astype(np.float32) / np.float32(255)).transpose(2, 0, 1)


def test_the_ramp_feeds_all_256_values_to_both_forms_of_finish():
    img = kf.ramp_image()
    assert all(sorted(img[:, :, c].ravel().tolist()) == list(range(256)) for c in range(3))
    assert not (img[:, :, 0] == img[:, :, 1]).all() and not (img[:, :, 1] == img[:, :, 2]).all()
    kf.check_equal(ramp_crop(), ramp_want_crop(), "ramp crop")
    kf.check_equal(ramp_crop(), kf.pillow_crop(img, (0, 0, 16, 16), 16), "ramp crop, Pillow")
    for norm in kf.NORMS:
        kf.check_equal(ramp_pre(norm), kf.hf_preprocess(img, 16, *kf.NORMS[norm]), "ramp preprocess")


def test_a_box_without_extent_gives_zero_planes_and_leaves_its_neighbours_alone():
    """Read from the kernels: x2 <= x1 or y2 <= y1 gives a tap count of 0 on that axis, no index is formed (the horizontal pass
    returns at y >= inH, the vertical loop is empty) and finish(0) = 0.  The restatement agrees."""
    run = kf.CropRun(16, False, "all", 0)
    boxes = np.array(kf.DEGENERATE_BOXES, np.int32)
    got, _ = emulate_crop(run, boxes=boxes)
    images = kf.crop_images(False)
    for r, box in enumerate(kf.DEGENERATE_BOXES):
        kf.check_equal(got[r], kf.pillow_crop(images[box[0]], box[1:], 16), f"box {box}")
    empty = [r for r, b in enumerate(kf.DEGENERATE_BOXES) if b[3] <= b[1] or b[4] <= b[2]]
    assert len(empty) == 4 and all(not got[r].any() for r in empty) and all(got[r].any() for r in (0, 2, 6))


# ---- planted faults ----------------------------------------------------------------------------------------------------------------

CROP_FAULTS = ["wmax", "hmax", "clamp", "trunc_w", "h_unrounded", "swap", "taps", "hwc", "tmp_stride", "mulf255"]


@pytest.mark.parametrize("fault", CROP_FAULTS)
def test_a_planted_crop_fault_is_not_equal_to_pillow(fault):
    run = kf.CropRun(16, False, "all", 13)
    if fault == "taps":                 # the 7-wide box upscaled to 64 alone: KS = 3, two taps with real weights
        batch, dims = kf.crop_batch(False)
        box = dict(kf.crop_list(64, False))["upscale_7"]
        got = kf.emulate(batch, dims, kf.plan_from_boxes([box], 64), 64, 5, 3, kf.BILINEAR, None, fault)
        with pytest.raises(AssertionError, match="differ"):
            kf.check_equal(got[0], kf.crop_expected(64, False)[box], fault)
        return
    if fault == "mulf255":
        with pytest.raises(AssertionError, match="differ"):
            kf.check_equal(ramp_crop(fault), ramp_want_crop(), fault)
        return
    got, boxes = emulate_crop(run, fault)
    with pytest.raises(AssertionError, match="differ"):
        kf.check_equal(got, kf.crop_want(run, boxes), fault)


def test_the_spare_tap_slot():
    """KS = 2 ceil(support) + 1 as in Pillow, but a tap list never has more than 2 ceil(support) = KS - 1 entries (the two
    truncations differ by at most ceil(2 support)), so "the tap list cut at KS - 1" changes nothing and no test can see it;
    the planted fault above cuts at KS - 2, which a 7-wide box upscaled to 64 on its own (KS = 3) does see.  At KS > 130 the
    last tap of a BILINEAR list has a weight that rounds to 0, so nothing but an out-of-bounds write could show there."""
    for run in (kf.CropRun(7, True, "all", 0), kf.CropRun(16, False, "all", 0)):
        got, boxes = emulate_crop(run, "taps_ks1")
        kf.check_equal(got, kf.crop_want(run, boxes), "KS - 1")
    batch, dims, boxes, mh, mw = kf.crop_case(kf.CropRun(7, True, "all", 0))
    KS = kf.ksize_for(max(mh, mw), 7, kf.BILINEAR)
    assert KS > 130 and max(int(kf.coeffs(int(b[3] - b[1]), 7, 0, 7, kf.BILINEAR, KS)[1].max()) for b in boxes) == KS - 1


def test_the_two_forms_of_finish_agree_on_every_byte():
    """`v / 255.0f` and `float(double(v) * (1 / 255))` are the same function on 0 .. 255 (the double product is within 2^-53 of
    the quotient and no quotient v / 255 lies that close to the midpoint of two floats), so exchanging them is not a fault any
    test can see: the ramp proves that, and the planted fault is the form that does differ, the fp32 product v * (1.0f / 255)."""
    v = np.arange(256)
    a = v.astype(np.float32) / np.float32(255)
    assert (a == (v.astype(np.float64) * (1 / 255)).astype(np.float32)).all()
    assert (a != v.astype(np.float32) * np.float32(1 / 255)).any()
    for fault in ("div255", "mul255"):
        kf.check_equal(ramp_crop(fault), ramp_want_crop(), fault)
        kf.check_equal(ramp_pre("clip", fault), kf.hf_preprocess(kf.ramp_image(), 16, *kf.NORMS["clip"]), fault)


# (Wmax / Hmax for iw / ih cannot show in preprocessing: its box is the image itself and no tap leaves it.)
@pytest.mark.parametrize("fault", ["left_up", "long_round", "mulf255", "chan_rev", "swap"])
@pytest.mark.parametrize("norm", list(kf.NORMS))
def test_a_planted_preprocessing_fault_is_not_equal_to_pillow(fault, norm):
    if fault == "mulf255":
        with pytest.raises(AssertionError, match="differ"):
            kf.check_equal(ramp_pre(norm, fault), kf.hf_preprocess(kf.ramp_image(), 16, *kf.NORMS[norm]), fault)
        return
    with pytest.raises(AssertionError, match="differ"):
        kf.check_equal(emulate_pre(7, norm, fault), kf.pre_expected(7, norm), fault)


def test_one_float_behind_out_breaks_the_guard_and_leaves_a_nan():
    run = kf.CropRun(2, False, "all", 0)
    got, boxes = emulate_crop(run)
    g = kc.Guarded(got.shape[0] * 3, 4, guard_rows=1024)
    flat = g.buf.view(torch.float32)
    flat[g.guard + 1:g.guard + 1 + got.size] = torch.from_numpy(got.ravel())
    with pytest.raises(AssertionError, match="was written"):
        g.assert_guards("shifted")
    with pytest.raises(AssertionError, match="differ"):
        kf.check_equal(g.get().numpy().reshape(got.shape), kf.crop_want(run, boxes), "shifted")


def test_the_documented_workspace_layout():
    assert kf.workspace_bytes(1, 1, 1, 1, kf.BILINEAR) == 256 * 3 + 3
    assert kf.workspace_bytes(257, 64, 93, 94, kf.BILINEAR) == kf.roundup(257 * 36, 256) + kf.roundup(257 * 2 * 64 * 8, 256) + \
        kf.roundup(257 * 2 * 64 * 5 * 4, 256) + 257 * 93 * 64 * 3


# ---- the lists reach what they were written for ----------------------------------------------------------------------------------

def test_crop_cases_reach_every_situation():
    runs = kf.crop_runs()
    assert {r.S for r in runs} == {1, 2, 7, 16, 64, 224} and {r.nr for r in runs} == {"one", "all", "257"}
    for S in kf.CROP_S:
        assert {(r.nr, r.extra) for r in runs if r.S == S} == {(n, e) for n in ("one", "all", "257") for e in (0, 13)}
        assert len(kf.crop_case(kf.CropRun(S, S == 7, "257", 0))[2]) == 257              # a second block of the plan kernel
        batch, dims = kf.crop_batch(S == 7)
        _, Hmax, Wmax, _ = batch.shape
        per_image = {}
        for tag, (b, x1, y1, x2, y2) in kf.crop_list(S, S == 7):
            per_image.setdefault(b, {})[tag] = (x1, y1, x2, y2)
        for b, (ih, iw) in enumerate(kf.SMALL_DIMS):
            t = per_image[b]
            assert t["full"] == (0, 0, iw, ih) and t["first_px"] == (0, 0, 1, 1) and t["last_px"] == (iw - 1, ih - 1, iw, ih)
            assert t["one_row"][3] - t["one_row"][1] == 1 and t["one_col"][2] - t["one_col"][0] == 1
            w, h = (lambda q: q[2] - q[0]), (lambda q: q[3] - q[1])
            assert w(t["w_eq_S"]) == S != h(t["w_eq_S"]) and h(t["h_eq_S"]) == S != w(t["h_eq_S"])
            assert w(t["both_eq_S"]) == h(t["both_eq_S"]) == S
            assert t["straddle_left"][0] < 0 < t["straddle_left"][2] and t["straddle_right"][0] < iw < t["straddle_right"][2]
            assert t["straddle_top"][1] < 0 < t["straddle_top"][3] and t["straddle_bottom"][1] < ih < t["straddle_bottom"][3]
            c = t["straddle_corner"]
            assert c[0] < iw < c[2] and c[1] < ih < c[3] and t["negative_origin"][0] < 0 > t["negative_origin"][1]
            assert t["outside_left"][2] <= 0 and t["outside_right"][0] >= iw and t["outside_above"][3] <= 0 and t["outside_below"][1] >= ih
            assert t["beyond_max"][2] > Wmax and t["beyond_max"][3] > Hmax and w(t["upscale_7"]) == 7
            if ih < Hmax:
                assert t["rows_ih_to_Hmax"][1] == ih and t["rows_ih_to_Hmax"][3] == Hmax
        exp = kf.crop_expected(S, S == 7)
        for tag, box in kf.crop_list(S, S == 7):
            if tag.startswith("outside") or tag == "rows_ih_to_Hmax":
                assert not exp[box].any(), (tag, box)                  # all zeros expected
    large = dict(kf.crop_list(7, True))
    assert large["large_down"][1:] == (0, 0, 640, 480) and kf.ksize_for(643, 7, kf.BILINEAR) > 130
    assert all(b[0] == 6 for _, b in kf.crop_list(224, True)) and dict(kf.crop_list(224, True))["full"][1:] == (0, 0, 640, 480)
    assert (7, 64) in {(b[3] - b[1], 64) for _, b in kf.crop_list(64, False)}           # a 7-wide box upscaled to 64


def test_preprocessing_cases_reach_every_situation():
    for S in kf.PRE_S:
        dims = kf.pre_dims(S)
        assert dims[:13] == kf.PRE_DIMS
        assert (S != 16) or {(16, 16), (16, 48), (49, 16), (15, 21)} <= set(dims)
        assert (S != 32) or (1500, 2000) in dims
    geo = [(S, h, w) + kf.pre_geometry(h, w, S) for S in kf.PRE_S for h, w in kf.pre_dims(S)]
    assert any(rem == 0 and h != w and new_long > S for S, h, w, new_long, rem, shrt in geo)          # on an integer
    assert any(rem / shrt > 0.95 for *_, rem, shrt in geo)                                              # just under one
    assert any((new_long - S) % 2 == 1 for S, _, _, new_long, _, _ in geo)                              # odd newW - S
    assert any(h == S or w == S for S, h, w, *_ in geo) and any(h == w == S for S, h, w, *_ in geo)     # a pass Pillow skips
    assert any(h == 1 and w == 1 for _, h, w, *_ in geo) and 1 in kf.PRE_S


# ================================================================================================ ranking

@pytest.mark.parametrize("case", kf.rank_int_cases(), ids=kf.rank_id)
def test_the_fp32_evaluation_of_every_integer_ranking_case_is_exact(case):
    s = kf.build_rank_int(case)
    kf.check_rank_exact(kf.emulate_rank(s["q"], s["cand"], s["thr"], s["gt"]), s["want"], kf.rank_id(case))
    if case.thr == "below":
        assert (s["want"] >= case.Bk - 1).all()
    if case.thr == "above":
        assert not s["want"].any()


def test_rank_cases_reach_every_situation():
    cases = kf.rank_int_cases()
    assert {(c.Bq, c.Bk, c.P) for c in cases} == set(kf.RANK_SHAPES)
    for shape in kf.RANK_SHAPES:
        mine = [c for c in cases if (c.Bq, c.Bk, c.P) == shape]
        assert {c.thr for c in mine} == {"ties", "half", "below", "above"}
        assert {c.gt for c in mine} >= {"given", "minus1", "Bk"} | ({"null"} if shape[1] >= shape[0] else set())
    assert any(c.Bk <= 32 for c in cases) and any(c.Bk == 33 for c in cases)              # the empty second sub-tile, and its first column
    assert any(c.Bq > 256 for c in cases)                                                  # a second block of the merge
    ties = [kf.build_rank_int(c) for c in cases if c.thr == "ties" and c.Bk > 4]
    assert all(s["ties"] > len(s["thr"]) for s in ties)                                    # many exact ties per case
    s = kf.build_rank_int(kf.RankCase(65, 129, 68, "given", "ties"))
    assert sum(bool((s["cand"][j] == s["cand"][s["given"][0]]).all()) for j in range(129)) >= 4     # copies of a ground truth
    assert (s["sim"][0, [1, 4, 7, 10]] == s["thr"][0]).all()                                         # which tie with it exactly


@pytest.mark.parametrize("fault", ["ge", "gt_counted", "pad_cols", "slot_unwritten", "merge_down"])
def test_a_planted_ranking_fault_fails_the_exact_count(fault):
    thr = {"ge": "ties", "gt_counted": "below", "pad_cols": "below", "slot_unwritten": "half", "merge_down": "half"}[fault]
    case = kf.RankCase(3, 32, 64, "given", thr) if fault == "slot_unwritten" else kf.RankCase(65, 129, 68, "given", thr)
    s = kf.build_rank_int(case)
    with pytest.raises(AssertionError, match="rows differ"):
        kf.check_rank_exact(kf.emulate_rank(s["q"], s["cand"], s["thr"], s["gt"], fault), s["want"], fault)


@pytest.mark.parametrize("shape", kf.RANK_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_the_ranking_interval_is_tight_and_holds_on_an_fp32_evaluation(shape):
    """sum (hi - lo) on these seeds: 11 of 19,350 at (37, 1000, 512), 1 of 69,571 at (130, 1001, 36), 0 elsewhere."""
    Bq, Bk, P = shape
    s = kf.build_rank_gauss(Bq, Bk, P)
    own = s["cand"][s["gt"]]
    thr32 = (s["q"] * own).sum(axis=1, dtype=np.float32)
    want = (s["q"].astype(np.float64) * own.astype(np.float64)).sum(axis=1)
    assert (np.abs(thr32 - want) <= kf.rowdot_bound(s["q"], own)).all()
    lo, hi = kf.rank_interval(s["q"], s["cand"], thr32, s["gt"])
    slack, total = kf.check_rank_interval(kf.emulate_rank(s["q"], s["cand"], thr32, s["gt"]), lo, hi, str(shape))
    print(shape, "slack", slack, "of", total)
    lo64, hi64 = kf.rank_interval(s["q"], s["cand"], want, s["gt"])
    assert int((hi64 - lo64).sum()) <= 0.005 * int(hi64.sum())
    if total:
        for fault in ("gt_counted", "slot_unwritten"):
            with pytest.raises(AssertionError):
                kf.check_rank_interval(kf.emulate_rank(s["q"], s["cand"], thr32, s["gt"], fault), lo, hi, fault)


def test_duplicates_of_the_ground_truth_may_be_counted_and_nothing_else():
    s = kf.build_rank_gauss(65, 129, 68, dup=True)
    assert (s["dups"].sum(axis=1) == 3).sum() == 3 and not s["dups"][np.arange(65), s["gt"]].any()
    thr32 = (s["q"] * s["cand"][s["gt"]]).sum(axis=1, dtype=np.float32)
    lo, hi = kf.rank_interval(s["q"], s["cand"], thr32, s["gt"], exclude=s["dups"])
    got = kf.emulate_rank(s["q"], s["cand"], thr32, s["gt"])
    kf.check_rank_interval(got, lo, hi, "duplicates", extra=s["dups"].sum(axis=1))
    with pytest.raises(AssertionError, match="outside"):
        kf.check_rank_interval(got + 4 * s["dups"].any(axis=1), lo, hi, "four more", extra=s["dups"].sum(axis=1))
