"""CPU-only: the host planner of the packed full-resolution teacher (CLIPPatchTokenizer.plan_full_resolution)
on hand-written box lists, and the launcher's --full_resolution_from_epoch."""
import pytest
import torch

from dclip_amd.clip_model import packed_crop_tables
from dclip_amd.patch_text_aggregation import CLIPPatchTokenizer

plan = CLIPPatchTokenizer.plan_full_resolution


def ints(t):
    return t.tolist()


def test_offsets_grids_cls_rows_and_max_s():
    # image 0: 32x48 -> 2x3 grid, 7 rows; 50x80 -> 3x5, 16 rows.  image 1: 16x16 -> 1x1, 2 rows; 70x33 -> 4x2, 9 rows
    boxes = [[((0, 0, 48, 32), 0.9), ((10, 20, 90, 70), 0.8)], [((3, 5, 19, 21), 0.7), ((1, 2, 34, 72), 0.6)]]
    p = plan(boxes, 16)
    assert ints(p["boxes"]) == [[0, 0, 0, 48, 32], [0, 10, 20, 90, 70], [1, 3, 5, 19, 21], [1, 1, 2, 34, 72]]
    assert ints(p["grids"]) == [[2, 3], [3, 5], [1, 1], [4, 2]]
    assert ints(p["cu_seqlens"]) == [0, 7, 23, 25, 34]
    assert ints(p["patch_offsets"]) == [0, 6, 21, 22, 30]
    assert ints(p["cls_rows"]) == [0, 7, 23, 25]
    assert p["max_S"] == 16 and p["counts"] == [2, 2] and ints(p["slots"]) == [0, 1, 2, 3]
    for k in ("boxes", "grids", "cu_seqlens", "patch_offsets", "cls_rows"):
        assert p[k].dtype == torch.int32 and p[k].device.type == "cpu" and p[k].is_contiguous(), k
    assert p["slots"].dtype == torch.int64
    # patch_offsets[n] = cu_seqlens[n] - n
    assert ints(p["patch_offsets"]) == [c - n for n, c in enumerate(ints(p["cu_seqlens"]))]


def test_coordinates_are_truncated_like_crop_boxes_gpu():
    p = plan([[((0.9, 1.9, 48.99, 33.2), 1.0), ((-0.5, -3.7, 31.9, 28.9), 1.0)]], 16)
    assert ints(p["boxes"]) == [[0, 0, 1, 48, 33], [0, 0, -3, 31, 28]]         # int(): towards zero, negatives too
    assert ints(p["grids"]) == [[2, 3], [1, 1]]                                  # 32x48 and 31x31 by floor


def test_an_image_with_a_box_without_extent_keeps_no_region():
    good = ((0, 0, 32, 32), 0.9)
    p = plan([[good, ((20, 5, 20, 40), 0.5)], [good], [((30, 40, 10, 80), 0.5), good], [good, good, good]], 16)
    assert p["counts"] == [0, 1, 0, 3]
    assert ints(p["boxes"][:, 0]) == [1, 3, 3, 3]
    assert ints(p["slots"]) == [1 * 3 + 0, 3 * 3 + 0, 3 * 3 + 1, 3 * 3 + 2]      # Rmax = 3


def test_an_image_with_a_crop_shorter_than_one_patch_keeps_no_region():
    good = ((0, 0, 32, 32), 0.9)
    p = plan([[good, ((5, 5, 15, 60), 0.5)], [good, ((5, 5, 60, 20.9), 0.5)], [good, ((5, 5, 21, 21), 0.5)]], 16)
    assert p["counts"] == [0, 0, 2]                                              # 10 px wide; 15 px high after truncation; 16x16
    assert ints(p["grids"]) == [[2, 2], [1, 1]] and ints(p["cu_seqlens"]) == [0, 5, 7]
    # the same crop is fine at a smaller patch
    assert plan([[good, ((5, 5, 15, 60), 0.5)]], 8)["counts"] == [2]


def test_an_empty_batch_and_an_image_without_boxes():
    p = plan([], 16)
    assert p["counts"] == [] and p["max_S"] == 0 and ints(p["cu_seqlens"]) == [0] and ints(p["patch_offsets"]) == [0]
    assert tuple(p["boxes"].shape) == (0, 5) and tuple(p["grids"].shape) == (0, 2) and p["slots"].numel() == 0
    p = plan([[], [((0, 0, 16, 48), 1.0)], []], 16)
    assert p["counts"] == [0, 1, 0] and ints(p["boxes"]) == [[1, 0, 0, 16, 48]] and ints(p["slots"]) == [1]
    assert ints(p["grids"]) == [[3, 1]] and p["max_S"] == 4 and ints(p["cls_rows"]) == [0]
    p = plan([[], []], 16)
    assert p["counts"] == [0, 0] and p["boxes"].shape[0] == 0


def test_tables_refuse_a_crop_smaller_than_one_patch():
    with pytest.raises(ValueError, match="smaller than one patch"):
        packed_crop_tables(torch.tensor([[0, 0, 0, 32, 32], [0, 5, 5, 15, 60]], dtype=torch.int32), 16)


def test_the_launcher_parses_full_resolution_from_epoch():
    from dclip_amd.CLIP_image_distill_training import build_parser, resolve_full_resolution_epoch
    base = ["--train_file", "x.json"]
    a = build_parser().parse_args(base + ["--full_resolution_from_epoch", "3"])
    assert a.full_resolution_from_epoch == 3 and resolve_full_resolution_epoch(a) == 3
    a = build_parser().parse_args(base + ["--full_resolution_from_epoch", "half", "--phase1_epochs", "7"])
    assert a.full_resolution_from_epoch == "half" and resolve_full_resolution_epoch(a) == 3
    a = build_parser().parse_args(base)
    assert a.full_resolution_from_epoch is None and resolve_full_resolution_epoch(a) is None
    with pytest.raises(SystemExit):
        build_parser().parse_args(base + ["--full_resolution_from_epoch", "soon"])
