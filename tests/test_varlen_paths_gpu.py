"""The four entries of the packed (variable-length) vision tower through the C ABI: the patch gather from
boxes, the assemble step with a per-crop resample of the position table, self-attention inside packed sequences and the row
gather.  Outputs live in guarded buffers, the rows behind every operand are NaN, a refused call launches nothing and writes
nothing.  References: fp64 attention (tests/kernel_checks.py, the project's tolerances), an index expression on the host and
Pillow for the gather, the existing per-crop entries (bit for bit) and the fp64 definition of tests/kernel_checks_interp.py for
the assemble step."""
import numpy as np
import pytest
import torch

from tests import kernel_checks as kc
from tests import kernel_checks_interp as ki

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC00000
HD = 64


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


def i32(values, dev):
    return torch.tensor(values, dtype=torch.int32, device=dev).contiguous()


def ok(lib, rc, site):
    assert rc == 0, lib.dclip_last_error()
    assert lib.dclip_last_launch() == site.encode()


def unwritten(g):
    return g.get().view(torch.int32) == NAN_BITS


def cumulative(lengths):
    return [0] + np.cumsum(lengths).tolist()


# ------------------------------------------------------------------------------------------------ attention

ATTN_CASES = [([1, 2, 17, 63, 64, 65, 128, 129, 5], 2), ([197, 3, 257], 1), ([64], 3)]


def run_attention(lib, dev, qkv, lengths, H, cls_only, with_lse=True):
    """(out [rows, H*64], lse [H, rows] or None) of one call; rows = T, or N with cls_only."""
    N, T, D = len(lengths), sum(lengths), H * HD
    src = kc.poisoned(qkv, 3 * D, dev)                                 # NaN rows behind the last sequence
    rows = N if cls_only else T
    out, lse = kc.Guarded(rows, D, device=dev), kc.Guarded(H, rows, device=dev)
    cu = i32(cumulative(lengths), dev)
    ok(lib, lib.dclip_attention_varlen_fwd(src.data_ptr(), cu.data_ptr(), out.ptr, lse.ptr if with_lse else None, N, max(lengths),
                                           H, int(cls_only), stream()), "attention_varlen_fwd")
    torch.cuda.synchronize()
    out.assert_guards("attention_varlen_fwd out")
    lse.assert_guards("attention_varlen_fwd lse")
    if not with_lse:
        assert bool(unwritten(lse).all()), "lse = NULL, yet the lse buffer was written"
    return out.get(), lse.get() if with_lse else None


def attention_reference(qkv, lengths, H, cls_only):
    """Per sequence (out_n, lse_n [H, rows_n]) in fp64."""
    cu, ref = cumulative(lengths), []
    for n, S in enumerate(lengths):
        q, k, v = (qkv[cu[n]:cu[n + 1]].double().view(1, S, 3, H, HD)[:, :, i] for i in range(3))
        out, lse, _, _, _ = kc.attention_math(q[:, :1] if cls_only else q, k, v, None)
        ref.append((out.reshape(-1, H * HD), lse.reshape(H, -1)))
    return ref


def per_sequence(out, lse, lengths, cls_only):
    cu = list(range(len(lengths) + 1)) if cls_only else cumulative(lengths)
    return [(out[cu[n]:cu[n + 1]], None if lse is None else lse[:, cu[n]:cu[n + 1]]) for n in range(len(lengths))]


@pytest.mark.parametrize("cls_only", [False, True], ids=["all_rows", "cls_only"])
@pytest.mark.parametrize("lengths,H", ATTN_CASES, ids=["tile_edges", "197_3_257", "one_full_tile"])
def test_varlen_attention_against_fp64_per_sequence(dev, lib, lengths, H, cls_only):
    qkv = kc._gauss((sum(lengths), 3 * H * HD), 11, 1.5)
    out, lse = run_attention(lib, dev, qkv, lengths, H, cls_only)
    got, want = per_sequence(out, lse, lengths, cls_only), attention_reference(qkv, lengths, H, cls_only)
    blocks = {}
    for n, ((o, l), (wo, wl)) in enumerate(zip(got, want)):
        blocks[f"out[{n}:S={lengths[n]}]"] = (o, wo, kc.TOL_ATTN_FWD)
        blocks[f"lse[{n}:S={lengths[n]}]"] = (l, wl, kc.TOL_LSE)
    fig = kc.check_blocks(blocks, f"attention_varlen_fwd {lengths} H={H} cls_only={cls_only}")
    print("worst out", max(v for k, v in fig.items() if k.startswith("out")), "worst lse",
          max(v for k, v in fig.items() if k.startswith("lse")))
    out2, _ = run_attention(lib, dev, qkv, lengths, H, cls_only, with_lse=False)
    assert torch.equal(out2.view(torch.int32), out.view(torch.int32)), "lse = NULL changed out"


@pytest.mark.parametrize("cls_only", [False, True], ids=["all_rows", "cls_only"])
@pytest.mark.parametrize("lengths,H,victim", [(ATTN_CASES[0][0], 2, 4), (ATTN_CASES[1][0], 1, 1)], ids=["tile_edges", "197_3_257"])
def test_a_nan_sequence_leaves_every_other_sequence_bit_identical(dev, lib, lengths, H, victim, cls_only):
    qkv = kc._gauss((sum(lengths), 3 * H * HD), 12, 1.5)
    clean = per_sequence(*run_attention(lib, dev, qkv, lengths, H, cls_only), lengths, cls_only)
    cu = cumulative(lengths)
    dirty_in = qkv.clone()
    dirty_in[cu[victim]:cu[victim + 1]] = kc.NAN
    dirty = per_sequence(*run_attention(lib, dev, dirty_in, lengths, H, cls_only), lengths, cls_only)
    for n in range(len(lengths)):
        if n == victim:
            assert bool(torch.isnan(dirty[n][0]).all())
            continue
        for a, b, name in zip(clean[n], dirty[n], ("out", "lse")):
            assert bool(torch.isfinite(b).all()), (n, name)
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"sequence {n} {name} changed with sequence {victim}"


# ------------------------------------------------------------------------------------------------ patch gather

IMAGES = [(40, 56), (33, 47)]                 # (h, w) inside one 40 x 56 batch whose padding bytes are 255


def boxes_for(p):
    """(b, x1, y1, x2, y2): inside image 0; extents that are no multiple of p; past the right and bottom edge of image 1 (into
    the batch's padding and beyond the batch); from negative coordinates; exactly one patch in the corner of image 0."""
    (h0, w0), (h1, w1) = IMAGES
    return [(0, 3, 2, 3 + 2 * p, 2 + p), (0, 5, 1, 5 + 2 * p + 5, 1 + 2 * p + 3), (1, w1 - p - 2, h1 - p - 1, w1 + p - 2, h1 + p - 1),
            (1, -5, -3, -5 + 2 * p, -3 + 2 * p), (0, w0 - p, h0 - p, w0, h0)]


def photos():
    rng = np.random.default_rng(5)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in IMAGES]


def host_crop(img, box):
    """uint8 [y2-y1, x2-x1, 3]: the image's pixels, zero outside it."""
    _, x1, y1, x2, y2 = box
    h, w = img.shape[:2]
    ys, xs = np.arange(y1, y2), np.arange(x1, x2)
    inside = ((ys >= 0) & (ys < h))[:, None] & ((xs >= 0) & (xs < w))[None, :]
    crop = img[np.clip(ys, 0, h - 1)[:, None], np.clip(xs, 0, w - 1)[None, :]]
    return np.where(inside[:, :, None], crop, np.uint8(0))


def patch_rows(crop_u8, p):
    """[gh*gw, 3*p*p] float32: uint8 -> float32, divided by 255, in the column order of im2col."""
    f = crop_u8.astype(np.float32) / np.float32(255.0)
    gh, gw = f.shape[0] // p, f.shape[1] // p
    v = f[:gh * p, :gw * p].reshape(gh, p, gw, p, 3)
    return np.ascontiguousarray(v.transpose(0, 2, 4, 1, 3)).reshape(gh * gw, 3 * p * p)


@pytest.mark.parametrize("p", [4, 16, 14])
def test_patches_from_boxes_equal_the_host_index_expression_and_pillow(dev, lib, p):
    from PIL import Image
    imgs, boxes = photos(), boxes_for(p)
    batch = np.full((2, 40, 56, 3), 255, np.uint8)
    for b, a in enumerate(imgs):
        batch[b, :a.shape[0], :a.shape[1]] = a
    crops = [host_crop(imgs[bx[0]], bx) for bx in boxes]
    for bx, c in list(zip(boxes, crops)):                                    # Pillow agrees with the host expression
        pil = np.asarray(Image.fromarray(imgs[bx[0]]).crop(bx[1:]).convert("RGB"), dtype=np.uint8)
        assert np.array_equal(pil, c), bx
    want = np.concatenate([patch_rows(c, p) for c in crops])
    counts = [((bx[4] - bx[2]) // p) * ((bx[3] - bx[1]) // p) for bx in boxes]
    assert min(counts) == 1 and max(counts) >= 4 and want.shape[0] == sum(counts)
    assert int(crops[2].min()) == 0 and int(crops[3][0, 0].max()) == 0          # outside positions are in the cases
    images = torch.from_numpy(batch).to(dev)
    out = kc.Guarded(want.shape[0], 3 * p * p, device=dev)
    dims, bxs, po = i32([list(s) for s in IMAGES], dev), i32([list(bx) for bx in boxes], dev), i32(cumulative(counts), dev)
    ok(lib, lib.dclip_patches_from_boxes_u8(images.data_ptr(), dims.data_ptr(), bxs.data_ptr(), po.data_ptr(), out.ptr, 2, 40, 56,
                                            len(boxes), p, stream()), "patches_from_boxes_u8")
    torch.cuda.synchronize()
    out.assert_guards(f"patches_from_boxes_u8 p={p}")
    ki.check_bits(out.get().numpy(), want, f"patches_from_boxes_u8 p={p}")


# ------------------------------------------------------------------------------------------------ assemble

GRIDS = [(7, 7), (1, 1), (2, 5), (10, 13), (14, 14)]


def run_assemble(lib, dev, patch, cls, pos, grids, g, D):
    lengths = [1 + gh * gw for gh, gw in grids]
    T = sum(lengths)
    assert patch.shape == (T - len(grids), D)
    srcs = [kc.poisoned(torch.from_numpy(a.reshape(-1, D)), D, dev) for a in (patch, cls, pos)]
    x = kc.Guarded(T, D, device=dev)
    d_grids, cu = i32([list(t) for t in grids], dev), i32(cumulative(lengths), dev)
    ok(lib, lib.dclip_vision_assemble_varlen(srcs[0].data_ptr(), srcs[1].data_ptr(), srcs[2].data_ptr(), d_grids.data_ptr(),
                                             cu.data_ptr(), x.ptr, g, len(grids), D, stream()), "vision_assemble_varlen")
    torch.cuda.synchronize()
    x.assert_guards("vision_assemble_varlen x")
    return x.get().numpy(), lengths, srcs


@pytest.mark.parametrize("D", [8, 768])
def test_assemble_varlen_is_bit_equal_to_the_per_crop_entries(dev, lib, D):
    g = 7
    rng = np.random.default_rng(D)
    n_patch = sum(gh * gw for gh, gw in GRIDS)
    patch, cls, pos = (rng.standard_normal(s).astype(np.float32) for s in ((n_patch, D), (D,), (1 + g * g, D)))
    got, lengths, (d_patch, d_cls, d_pos) = run_assemble(lib, dev, patch, cls, pos, GRIDS, g, D)
    cu = cumulative(lengths)
    for n, (gh, gw) in enumerate(GRIDS):
        table = torch.empty((lengths[n], D), dtype=torch.float32, device=dev)
        want = torch.empty((lengths[n], D), dtype=torch.float32, device=dev)
        assert lib.dclip_pos_interp_fwd(d_pos.data_ptr(), table.data_ptr(), g, gh, gw, D, stream()) == 0
        first = d_patch[cu[n] - n:cu[n + 1] - n - 1].contiguous()
        assert lib.dclip_vision_assemble_fwd(first.data_ptr(), d_cls.data_ptr(), table.data_ptr(), want.data_ptr(), 1, lengths[n], D,
                                             stream()) == 0
        torch.cuda.synchronize()
        ki.check_bits(got[cu[n]:cu[n + 1]], want.cpu().numpy(), f"crop {n} ({gh}x{gw}) D={D}")


@pytest.mark.parametrize("g,grid", [(7, (14, 14)), (14, (7, 7))], ids=["ratio_2", "ratio_half"])
def test_assemble_varlen_equals_the_fp64_reference_on_integer_data(dev, lib, g, grid):
    D = 8
    grids = [grid, (g, g), grid]                          # the identity between two resampled crops
    rng = np.random.default_rng(g)
    pos = ki.build_int_table(g, D)
    patch = rng.integers(-8, 9, (sum(gh * gw for gh, gw in grids), D)).astype(np.float32)
    cls = rng.integers(-8, 9, (D,)).astype(np.float32)
    got, lengths, _ = run_assemble(lib, dev, patch, cls, pos, grids, g, D)
    cu = cumulative(lengths)
    for n, (gh, gw) in enumerate(grids):
        want = ki.interp_reference(pos, g, gh, gw)
        want[0] += cls.astype(np.float64)
        want[1:] += patch[cu[n] - n:cu[n + 1] - n - 1].astype(np.float64)
        ki.check_exact(got[cu[n]:cu[n + 1]], want, f"vision_assemble_varlen g={g} crop {n} ({gh}x{gw})")


# ------------------------------------------------------------------------------------------------ row gather

def test_gather_rows_at_copies_repeated_and_unsorted_rows(dev, lib):
    T, D = 37, 12
    x = kc._gauss((T, D), 3)
    rows = [36, 0, 5, 5, 17, 0, 36, 1]
    out = kc.Guarded(len(rows), D, device=dev)
    src, idx = kc.poisoned(x, D, dev), i32(rows, dev)
    ok(lib, lib.dclip_gather_rows_at(src.data_ptr(), idx.data_ptr(), out.ptr, len(rows), T, D, stream()), "gather_rows_at")
    torch.cuda.synchronize()
    out.assert_guards("gather_rows_at")
    assert torch.equal(out.get().view(torch.int32), x[rows].view(torch.int32))


# ------------------------------------------------------------------------------------------------ refusals

def test_refusals_launch_nothing_and_write_nothing(dev, lib):
    H, D, N, T, p = 2, 8, 2, 7, 4
    f = kc.poisoned(kc._gauss((T, 3 * H * HD), 1), 3 * H * HD, dev)
    tab = i32([0, 3, 7, 0, 0, 0, 0, 0, 0, 0, 0, 0], dev)        # stands in for every int32 table; a refusal never reads it
    u8 = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=dev)
    outs = {k: kc.Guarded(T, H * HD, device=dev) for k in ("attn", "lse", "cols", "x", "rows")}
    lib.dclip_relu_f32(kc.Guarded(1, 64, device=dev).ptr, 64, stream())               # some other launch site
    s = stream()
    calls = {
        "attn": (lib.dclip_attention_varlen_fwd, [f.data_ptr(), tab.data_ptr(), outs["attn"].ptr, outs["lse"].ptr, N, 4, H, 0, s],
                 [(0, None), (1, None), (2, None), (4, 0), (4, -1), (5, 0), (6, 0), (6, -2), (0, f.data_ptr() + 4),
                  (2, outs["attn"].ptr + 8)]),
        "cols": (lib.dclip_patches_from_boxes_u8, [u8.data_ptr(), tab.data_ptr(), tab.data_ptr(), tab.data_ptr(), outs["cols"].ptr, 1, 8,
                                                   8, N, p, s],
                 [(0, None), (1, None), (2, None), (3, None), (4, None), (5, 0), (6, 0), (7, -1), (8, 0), (8, -3), (9, 0),
                  (4, outs["cols"].ptr + 4)]),
        "x": (lib.dclip_vision_assemble_varlen, [f.data_ptr(), f.data_ptr(), f.data_ptr(), tab.data_ptr(), tab.data_ptr(), outs["x"].ptr,
                                                 2, N, D, s],
              [(0, None), (1, None), (2, None), (3, None), (4, None), (5, None), (6, 0), (7, 0), (7, -1), (8, 0), (8, 6), (8, -4),
               (2, f.data_ptr() + 4), (5, outs["x"].ptr + 8)]),
        "rows": (lib.dclip_gather_rows_at, [f.data_ptr(), tab.data_ptr(), outs["rows"].ptr, N, T, D, s],
                 [(0, None), (1, None), (2, None), (3, 0), (3, -5), (4, 0), (5, 0), (5, 6), (0, f.data_ptr() + 8)]),
    }
    for name, (fn, good, bad) in calls.items():
        for at, value in bad:
            args = list(good)
            args[at] = value
            assert fn(*args) == kc.E_INVAL, (name, at, value)
            assert lib.dclip_last_error()
            assert lib.dclip_last_launch() == b"relu_f32", f"a refused {name} call launched"
    torch.cuda.synchronize()
    for name, t in outs.items():
        t.assert_guards(f"refused {name}")
        assert bool(unwritten(t).all()), f"a refused {name} call wrote"
