"""Every path of dclip_amd/csrc/crop_resize.hip through the C ABI: both entries against Pillow itself, bit for
bit, at S = 1 .. 224, on 1 x 1 to 1500 x 2000 sources, with boxes on, across and outside every edge, NR = 1 / the list / 257,
max_crop_h / max_crop_w exact and + 13.  The batch padding, the bytes around the batch and the words behind dims and boxes are
poison, `out` is guarded and NaN-filled, the workspace has exactly the reported size, starts as 0xFF and has a guard band
behind it, and every call asserts the name dclip_last_launch reports.  Case lists and the numpy restatement that shows,
without a GPU, that every expected value is Pillow's: tests/kernel_checks_front.py, tests/test_kernel_checks_front_cpu.py."""
import ctypes

import numpy as np
import pytest
import torch

from tests import kernel_checks as kc
from tests import kernel_checks_front as kf

pytestmark = pytest.mark.gpu
PAD = 4096                      # poison bytes in front of and behind the batch; guard bytes behind the workspace


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from dclip_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def on_device():
    """{key: (allocation, pointer to the batch inside it)}: each host batch is uploaded once per module."""
    return {}


def stream():
    return torch.cuda.current_stream().cuda_stream


def upload(cache, key, batch, dev):
    """(Every tensor here is allocated and filled on the stream the kernels run on, so a buffer that is released while a launch
    is still in flight cannot be handed out and overwritten before that launch has finished.)"""
    if key not in cache:
        big = torch.from_numpy(np.random.default_rng(5).integers(1, 256, batch.size + 2 * PAD, dtype=np.uint8)).to(dev)
        big[PAD:PAD + batch.size] = torch.from_numpy(np.ascontiguousarray(batch).ravel()).to(dev)
        cache[key] = (big, big.data_ptr() + PAD)
    return cache[key][1]


def i32(values, dev):
    v = np.asarray(values, np.int32).ravel()
    t = torch.full((v.size + 64,), kf.POISON_I32, dtype=torch.int32, device=dev)
    t[:v.size] = torch.from_numpy(v).to(dev)
    return t


def out_buffer(NR, S, dev):
    return kc.Guarded(NR * 3, S * S, device=dev, guard_rows=max(8, -(-4096 // (S * S))))


class Workspace:
    def __init__(self, need, dev):
        self.need = need
        self.buf = torch.full((need + PAD,), 0xFF, dtype=torch.uint8, device=dev)

    @property
    def ptr(self):
        return self.buf.data_ptr()

    def assert_guard(self, what):
        assert bool((self.buf[self.need:] == 0xFF).all()), f"{what}: bytes behind the {self.need}-byte workspace were written"

    def assert_untouched(self, what):
        assert bool((self.buf == 0xFF).all()), f"{what}: a refused call wrote to the workspace"


def finished(lib, rc, site, out, ws, what):
    assert rc == 0, lib.dclip_last_error()
    assert lib.dclip_last_launch() == site
    torch.cuda.synchronize()
    out.assert_guards(what)
    ws.assert_guard(what)
    return out.get().numpy()


def run_crop(lib, dev, cache, key, batch, dims, boxes, S, mh, mw, workspace_bytes=None):
    B, Hmax, Wmax, _ = batch.shape
    NR = len(boxes)
    need = int(lib.dclip_crop_resize_workspace(NR, S, mh, mw))
    assert need == kf.workspace_bytes(NR, S, mh, mw, kf.BILINEAR)
    img, d, bx = upload(cache, key, batch, dev), i32(dims, dev), i32(boxes, dev)
    out, ws = out_buffer(NR, S, dev), Workspace(need, dev)
    ws.keep = (d, bx)
    rc = lib.dclip_crop_resize_u8(img, d.data_ptr(), bx.data_ptr(), out.ptr, B, Hmax, Wmax, NR, S, mh, mw, ws.ptr,
                                  need if workspace_bytes is None else workspace_bytes, stream())
    return rc, out, ws


def crop_groups():
    seen = []
    for r in kf.crop_runs():
        if (r.S, r.large, r.nr) not in seen:
            seen.append((r.S, r.large, r.nr))
    return seen


@pytest.mark.parametrize("S,large,nr", crop_groups(), ids=lambda v: str(v))
def test_crop_resize_equals_pillow_with_exact_and_generous_max_crop(dev, lib, on_device, S, large, nr):
    got = {}
    for extra in (0, 13):
        run = kf.CropRun(S, large, nr, extra)
        batch, dims, boxes, mh, mw = kf.crop_case(run)
        rc, out, ws = run_crop(lib, dev, on_device, ("crop", large), batch, dims, boxes, S, mh, mw)
        got[extra] = finished(lib, rc, b"crop_resize.v", out, ws, kf.crop_id(run)).reshape(len(boxes), 3, S, S)
        kf.check_equal(got[extra], kf.crop_want(run, boxes), kf.crop_id(run))
    kf.check_equal(got[13], got[0], "max_crop + 13 against exact")


def test_crop_resize_box_without_extent_is_three_zero_planes(dev, lib, on_device):
    """include/dclip_hip.h: x2 <= x1 or y2 <= y1 forms no index and yields zeros; the boxes either side are Pillow's."""
    batch, dims = kf.crop_batch(False)
    boxes = np.array(kf.DEGENERATE_BOXES, np.int32)
    rc, out, ws = run_crop(lib, dev, on_device, ("crop", False), batch, dims, boxes, 16, 29, 38)
    got = finished(lib, rc, b"crop_resize.v", out, ws, "degenerate").reshape(len(boxes), 3, 16, 16)
    images = kf.crop_images(False)
    for r, box in enumerate(kf.DEGENERATE_BOXES):
        kf.check_equal(got[r], kf.pillow_crop(images[box[0]], box[1:], 16), f"box {box}")


def test_crop_resize_refuses_a_short_workspace_and_bad_arguments(dev, lib, on_device):
    run = kf.CropRun(16, False, "all", 0)
    batch, dims, boxes, mh, mw = kf.crop_case(run)
    need = int(lib.dclip_crop_resize_workspace(len(boxes), 16, mh, mw))
    rc, out, ws = run_crop(lib, dev, on_device, ("crop", False), batch, dims, boxes, 16, mh, mw, workspace_bytes=need - 1)
    torch.cuda.synchronize()
    assert rc == kc.E_WORKSPACE and b"workspace" in lib.dclip_last_error()
    B, Hmax, Wmax, _ = batch.shape
    img, d, bx, NR = upload(on_device, ("crop", False), batch, dev), i32(dims, dev), i32(boxes, dev), len(boxes)
    ok_args = [img, d.data_ptr(), bx.data_ptr(), out.ptr, B, Hmax, Wmax, NR, 16, mh, mw, ws.ptr, need, stream()]
    for pos, bad in [(0, None), (1, None), (2, None), (3, None), (4, 0), (5, 0), (6, -1), (7, 0), (8, 0), (9, 0), (10, -3)]:
        args = list(ok_args)
        args[pos] = bad
        assert lib.dclip_crop_resize_u8(*args) == kc.E_INVAL, pos
    args = list(ok_args)
    args[11] = None
    assert lib.dclip_crop_resize_u8(*args) == kc.E_WORKSPACE
    torch.cuda.synchronize()
    out.assert_guards("refused")
    ws.assert_untouched("refused")
    assert bool(torch.isnan(out.get()).all()), "a refused call wrote to out"


# ---- dclip_clip_preprocess_u8 --------------------------------------------------------------------------------------------------

def run_pre(lib, dev, cache, key, batch, dims, S, norm, workspace_bytes=None):
    B, Hmax, Wmax, _ = batch.shape
    need = int(lib.dclip_clip_preprocess_workspace(B, Hmax, Wmax, S))
    assert need == kf.workspace_bytes(B, S, Hmax, Wmax, kf.BICUBIC)
    img, d = upload(cache, key, batch, dev), i32(dims, dev)
    out, ws = out_buffer(B, S, dev), Workspace(need, dev)
    ws.keep = d
    mean, std = ((ctypes.c_float * 3)(*t) for t in kf.NORMS[norm])
    rc = lib.dclip_clip_preprocess_u8(img, d.data_ptr(), out.ptr, B, Hmax, Wmax, S, mean, std, ws.ptr,
                                      need if workspace_bytes is None else workspace_bytes, stream())
    return rc, out, ws


@pytest.mark.parametrize("norm", list(kf.NORMS))
@pytest.mark.parametrize("S", kf.PRE_S)
def test_clip_preprocess_whole_list_in_one_batch_equals_the_host_library(dev, lib, on_device, S, norm):
    batch, dims = kf.pre_batch(S)
    rc, out, ws = run_pre(lib, dev, on_device, ("pre", S), batch, dims, S, norm)
    got = finished(lib, rc, b"clip_preprocess.v", out, ws, f"S={S}").reshape(len(dims), 3, S, S)
    kf.check_equal(got, kf.pre_expected(S, norm), f"preprocess S={S} {norm}")


@pytest.mark.parametrize("norm", list(kf.NORMS))
@pytest.mark.parametrize("S", kf.PRE_S)
def test_clip_preprocess_one_image_at_a_time_equals_the_host_library(dev, lib, S, norm):
    want = kf.pre_expected(S, norm)
    for n, im in enumerate(kf.pre_images(S)):
        batch, dims = kf.make_batch([im])
        rc, out, ws = run_pre(lib, dev, {}, None, batch, dims, S, norm)
        got = finished(lib, rc, b"clip_preprocess.v", out, ws, f"S={S} {im.shape}").reshape(3, S, S)
        kf.check_equal(got, want[n], f"preprocess S={S} {norm} {im.shape[:2]} alone")


def test_clip_preprocess_refuses_a_short_workspace_and_bad_arguments(dev, lib, on_device):
    batch, dims = kf.pre_batch(7)
    B, Hmax, Wmax, _ = batch.shape
    need = int(lib.dclip_clip_preprocess_workspace(B, Hmax, Wmax, 7))
    rc, out, ws = run_pre(lib, dev, on_device, ("pre", 7), batch, dims, 7, "clip", workspace_bytes=need - 1)
    torch.cuda.synchronize()
    assert rc == kc.E_WORKSPACE and b"workspace" in lib.dclip_last_error()
    img, d = upload(on_device, ("pre", 7), batch, dev), i32(dims, dev)
    mean, std = ((ctypes.c_float * 3)(*t) for t in kf.NORMS["clip"])
    ok_args = [img, d.data_ptr(), out.ptr, B, Hmax, Wmax, 7, mean, std, ws.ptr, need, stream()]
    for pos, bad in [(0, None), (1, None), (2, None), (3, 0), (4, 0), (5, -1), (6, 0), (7, None), (8, None)]:
        args = list(ok_args)
        args[pos] = bad
        assert lib.dclip_clip_preprocess_u8(*args) == kc.E_INVAL, pos
    torch.cuda.synchronize()
    out.assert_guards("refused")
    ws.assert_untouched("refused")
    assert bool(torch.isnan(out.get()).all()), "a refused call wrote to out"


# ---- the ramp: all 256 byte values through both forms of finish() ------------------------------------------------------------------

def test_the_ramp_through_both_entries(dev, lib):
    img = kf.ramp_image()
    batch, dims = kf.make_batch([img], 19, 21)
    rc, out, ws = run_crop(lib, dev, {}, None, batch, dims, np.array([(0, 0, 0, 16, 16)], np.int32), 16, 16, 16)
    got = finished(lib, rc, b"crop_resize.v", out, ws, "ramp crop").reshape(3, 16, 16)
    kf.check_equal(got, (img.astype(np.float32) / np.float32(255)).transpose(2, 0, 1), "ramp crop: float32(v) / float32(255)")
    for norm in kf.NORMS:
        rc, out, ws = run_pre(lib, dev, {}, None, batch, dims, 16, norm)
        got = finished(lib, rc, b"clip_preprocess.v", out, ws, "ramp preprocess").reshape(3, 16, 16)
        kf.check_equal(got, kf.hf_preprocess(img, 16, *kf.NORMS[norm]), f"ramp preprocess {norm}")
