"""TEST-ONLY checkers and case lists for the image front end (dclip_amd/csrc/crop_resize.hip) and the ranking kernels
(MODE_RANK, rank_merge_kernel, rowdot_gather_kernel in gemm_f32.hip): DESIGN.md §19.

Nothing here imports the product or needs a GPU.  The front end is restated in numpy operation by operation — the plan
(from boxes or from the shortest edge), the coefficients in Python floats (IEEE doubles, no contraction), 22-bit weights, a
horizontal pass to uint8, a vertical pass and `finish` — so that tests/test_kernel_checks_front_cpu.py can show, without a
GPU, that every case of tests/test_front_paths_gpu.py equals Pillow and that one planted fault at a time does not.  The GPU
tests compare the kernels with Pillow itself (`pillow_crop`, `hf_preprocess`), never with this restatement.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

PREC = 22                       # Pillow's PRECISION_BITS = 32 - 8 - 2
BILINEAR, BICUBIC = 0, 1
PLAN = 9
POISON_I32 = 2 ** 30            # behind dims and boxes: an index formed from it is far outside every allocation
CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
ORDER_MEAN, ORDER_STD = (0.0, 0.5, 1.0), (0.5, 0.25, 2.0)          # shows the channel order
NORMS = {"clip": (CLIP_MEAN, CLIP_STD), "order": (ORDER_MEAN, ORDER_STD)}


def roundup(v: int, m: int) -> int:
    return -(-v // m) * m


# ------------------------------------------------------------------------------------------------ the documented layout

def ksize_for(max_in: int, S: int, filt: int) -> int:
    fs = max(max_in / S, 1.0)
    support = (2.0 if filt == BICUBIC else 1.0) * fs
    c = int(support)
    if c < support:
        c += 1
    return 2 * c + 1


def workspace_bytes(NR: int, S: int, max_h: int, max_w: int, filt: int) -> int:
    """plan | bounds | weights, each rounded up to 256 bytes, then NR x max_h x S x 3 bytes of intermediate rows."""
    KS = ksize_for(max(max_h, max_w), S, filt)
    return roundup(NR * PLAN * 4, 256) + roundup(NR * 2 * S * 2 * 4, 256) + roundup(NR * 2 * S * KS * 4, 256) + NR * max_h * S * 3


# ------------------------------------------------------------------------------------------------ the restated kernels

def _bilinear(x: float) -> float:
    if x < 0.0:
        x = -x
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x: float) -> float:
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def coeffs(in_size: int, out_size: int, off: int, S: int, filt: int, KS: int, fault: str = None):
    """(first input index [S], tap count [S], weights [S][KS]) of output indices off .. off + S of an axis."""
    f = _bicubic if filt == BICUBIC else _bilinear
    xmin_all, cnt_all, kk = np.zeros(S, np.int64), np.zeros(S, np.int64), np.zeros((S, KS), np.int64)
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = (2.0 if filt == BICUBIC else 1.0) * filterscale
    ss = 1.0 / filterscale
    cap = {"taps_ks1": KS - 1, "taps": KS - 2}.get(fault, KS)
    for xx in range(S):
        center = 0.0 + (xx + off + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        xmax = min(max(xmax, 0), cap)
        ws = [f((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for w in ws:
            ww += w
        for x, w in enumerate(ws):
            if ww != 0.0:
                w /= ww
            if fault == "trunc_w":
                kk[xx, x] = int(w * (1 << PREC))
            else:
                kk[xx, x] = int(-0.5 + w * (1 << PREC)) if w < 0 else int(0.5 + w * (1 << PREC))
        xmin_all[xx], cnt_all[xx] = xmin, xmax
    return xmin_all, cnt_all, kk


def _clip8(s):
    return np.clip(s >> PREC, 0, 255)


def _resample(arr, axis: int, xmin, cnt, kk, exact: bool = False):
    """One pass along `axis` of arr [rows][cols][3]; uint8 out (or, exact = True, the unrounded float64 value)."""
    a = np.moveaxis(arr, axis, 0)
    out = np.zeros((len(xmin),) + a.shape[1:], np.float64 if exact else np.uint8)
    for xx in range(len(xmin)):
        n, lo = int(cnt[xx]), int(xmin[xx])
        if a.dtype == np.float64:
            s = np.tensordot(kk[xx, :n].astype(np.float64), a[lo:lo + n], axes=(0, 0))
            out[xx] = np.clip(np.floor((1 << (PREC - 1)) + s).astype(np.int64) >> PREC, 0, 255)
        else:
            s = np.tensordot(kk[xx, :n], a[lo:lo + n].astype(np.int64), axes=(0, 0))
            out[xx] = s / float(1 << PREC) if exact else _clip8((1 << (PREC - 1)) + s)
    return np.moveaxis(out, 0, axis)


def crop_of(batch, dims, b: int, x1: int, y1: int, x2: int, y2: int, fault: str = None):
    """The box as the horizontal pass samples it: [y2-y1][x2-x1][3] uint8, zero outside the image's own dims."""
    _, Hmax, Wmax, _ = batch.shape
    ih, iw = int(dims[b][0]), int(dims[b][1])
    sx, sy = np.arange(x1, x2), np.arange(y1, y2)
    if fault == "clamp":
        return batch[b][np.clip(sy, 0, ih - 1)][:, np.clip(sx, 0, iw - 1)]
    lim_w, lim_h = (Wmax if fault == "wmax" else iw), (Hmax if fault == "hmax" else ih)
    ok = ((sy >= 0) & (sy < lim_h))[:, None] & ((sx >= 0) & (sx < lim_w))[None, :]
    px = batch[b][np.clip(sy, 0, Hmax - 1)][:, np.clip(sx, 0, Wmax - 1)]
    return px * ok[:, :, None].astype(np.uint8)


def finish(v, norm, fault: str = None):
    """v [S][S][3] uint8 -> [3][S][S] fp32 (norm None: ToTensor; else CLIPImageProcessor's rescale and normalize)."""
    crop_form = norm is None
    if fault in ("div255", "mul255"):
        crop_form = fault == "div255"
    if fault == "mulf255":
        x = v.astype(np.float32) * np.float32(1 / 255)
    elif crop_form:
        x = v.astype(np.float32) / np.float32(255)
    else:
        x = (v.astype(np.float64) * (1 / 255)).astype(np.float32)
    if norm is not None:
        mean, std = (np.asarray(t, np.float32) for t in norm)
        if fault == "chan_rev":
            mean, std = mean[::-1], std[::-1]
        x = (x - mean) / std
    return np.ascontiguousarray(x if fault == "hwc" else x.transpose(2, 0, 1)).reshape(3, x.shape[0], x.shape[1])


def plan_from_boxes(boxes, S: int):
    return [(b, x1, y1, x2, y2, S, S, 0, 0) for b, x1, y1, x2, y2 in boxes]


def plan_shortest_edge(dims, S: int, fault: str = None):
    plan = []
    for b, (h, w) in enumerate(dims):
        shrt, lng = (w, h) if w <= h else (h, w)
        q = S * lng / shrt                          # Python's int(size * long / short): one correctly rounded division
        new_long = int(q + 0.5) if fault == "long_round" else int(q)
        newW, newH = (S, new_long) if w <= h else (new_long, S)
        up = 1 if fault == "left_up" else 0
        plan.append((b, 0, 0, w, h, newW, newH, (newW - S + up) // 2, (newH - S + up) // 2))
    return plan


def emulate(batch, dims, plan, S: int, Hc: int, KS: int, filt: int, norm=None, fault: str = None):
    """out [NR][3][S][S] fp32 as the three launches compute it (one planted fault when `fault` names one)."""
    blocks, cache = [], {}
    for p in plan:
        key = tuple(p)
        if key not in cache:
            b, x1, y1, x2, y2, outW, outH, left, top = p
            inW, inH = x2 - x1, y2 - y1
            assert inH <= Hc, "max_crop_h is smaller than this box"
            hx = coeffs(inW, outW, left, S, filt, KS, fault)
            vy = coeffs(inH, outH, top, S, filt, KS, fault)
            src = crop_of(batch, dims, b, x1, y1, max(x2, x1), max(y2, y1), fault)
            if fault == "swap":
                res = _resample(_resample(src, 0, *vy), 1, *hx)
                tmp = None
            else:
                tmp = _resample(src, 1, *hx, exact=fault == "h_unrounded")            # [inH][S][3]
                res = _resample(tmp, 0, *vy)
            cache[key] = (tmp, vy, res)
        blocks.append(cache[key])
    if fault == "tmp_stride":                      # the vertical pass indexes the intermediate with the box height, not Hc
        flat = np.full((len(plan) * Hc + Hc, S, 3), 0xFF, np.uint8)
        for r, (tmp, _, _) in enumerate(blocks):
            flat[r * Hc:r * Hc + tmp.shape[0]] = tmp
        res_all = []
        for r, (tmp, vy, _) in enumerate(blocks):
            inH = tmp.shape[0]
            res_all.append(_resample(flat[r * inH:r * inH + max(inH, 1)], 0, *vy) if inH else blocks[r][2])
    else:
        res_all = [blk[2] for blk in blocks]
    return np.stack([finish(v, norm, fault) for v in res_all])


# ------------------------------------------------------------------------------------------------ Pillow, the reference

def pillow_crop(img, box, S: int):
    """training/image_tokenizer.py: image.crop(box) -> Resize((S, S)) -> ToTensor()."""
    from PIL import Image
    x1, y1, x2, y2 = box
    if x2 <= x1 or y2 <= y1:                      # Pillow refuses such a box; the kernels give zeros (include/dclip_hip.h)
        return np.zeros((3, S, S), np.float32)
    r = Image.fromarray(img).crop((x1, y1, x2, y2)).resize((S, S), Image.BILINEAR)
    return np.ascontiguousarray((np.asarray(r).astype(np.float32) / np.float32(255)).transpose(2, 0, 1))


def hf_preprocess(img, S: int, mean, std):
    """CLIPImageProcessor with the PIL backend, restated: shortest edge -> S (BICUBIC), centre window, rescale, normalize."""
    from PIL import Image
    h, w = img.shape[:2]
    shrt, lng = (w, h) if w <= h else (h, w)
    new_long = int(S * lng / shrt)
    newW, newH = (S, new_long) if w <= h else (new_long, S)
    r = np.asarray(Image.fromarray(img).resize((newW, newH), Image.BICUBIC))
    left, top = (newW - S) // 2, (newH - S) // 2
    x = (r[top:top + S, left:left + S].astype(np.float64) * (1 / 255)).astype(np.float32)
    x = (x - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)
    return np.ascontiguousarray(x.transpose(2, 0, 1))


# ------------------------------------------------------------------------------------------------ images and batches

def _image(h: int, w: int, seed: int):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def ramp_image():
    """16 x 16, all 256 byte values in every channel, each channel in its own order."""
    rng = np.random.default_rng(256)
    return np.stack([rng.permutation(256).astype(np.uint8).reshape(16, 16) for _ in range(3)], axis=-1)


def make_batch(images, Hmax: int = None, Wmax: int = None, seed: int = 99):
    """[B][Hmax][Wmax][3] with every byte outside an image's own dims random and NON-ZERO (poison: zero is what padding means)."""
    Hmax = Hmax or max(i.shape[0] for i in images)
    Wmax = Wmax or max(i.shape[1] for i in images)
    batch = np.random.default_rng(seed).integers(1, 256, (len(images), Hmax, Wmax, 3), dtype=np.uint8)
    for b, im in enumerate(images):
        batch[b, :im.shape[0], :im.shape[1]] = im
    return batch, np.array([im.shape[:2] for im in images], np.int32)


SMALL_DIMS = [(1, 1), (2, 3), (8, 8), (37, 53), (3, 90), (90, 3)]            # (h, w)
LARGE_DIM = (480, 640)
CROP_S = [1, 2, 7, 16, 64]
CROP_S_LARGE = 224


@functools.lru_cache(maxsize=None)
def crop_images(with_large: bool):
    dims = SMALL_DIMS + ([LARGE_DIM] if with_large else [])
    return tuple(_image(h, w, 1000 * h + w) for h, w in dims)


@functools.lru_cache(maxsize=None)
def crop_batch(with_large: bool):
    return make_batch(crop_images(with_large))


def boxes_for(b: int, ih: int, iw: int, S: int, Hmax: int, Wmax: int):
    """[(tag, (b, x1, y1, x2, y2))]: every situation the issue names, for one image."""
    t = [("full", (0, 0, iw, ih)),
         ("first_px", (0, 0, 1, 1)), ("last_px", (iw - 1, ih - 1, iw, ih)),
         ("one_row", (0, ih // 2, iw, ih // 2 + 1)), ("one_col", (iw // 2, 0, iw // 2 + 1, ih)),
         ("w_eq_S", (0, 0, S, S + 3)), ("h_eq_S", (0, 0, S + 2, S)), ("both_eq_S", (0, 0, S, S)),
         ("straddle_left", (-2, 0, iw // 2 + 1, ih)), ("straddle_right", (iw // 2, 0, iw + 3, ih)),
         ("straddle_top", (0, -3, iw, ih // 2 + 1)), ("straddle_bottom", (0, ih // 2, iw, ih + 2)),
         ("straddle_corner", (iw - 1, ih - 1, iw + 4, ih + 5)), ("negative_origin", (-3, -2, iw + 1, ih + 1)),
         ("outside_left", (-6, 0, -1, ih)), ("outside_right", (iw, 0, iw + 5, ih)),
         ("outside_above", (0, -7, iw, 0)), ("outside_below", (0, ih, iw, ih + 4)),
         ("beyond_max", (0, 0, Wmax + 3, Hmax + 2)), ("upscale_7", (0, 0, 7, 5))]
    if ih < Hmax:
        t.append(("rows_ih_to_Hmax", (0, ih, Wmax, Hmax)))
        t.append(("into_padding", (max(iw - 2, 0), max(ih - 2, 0), min(iw + 9, Wmax), min(ih + 9, Hmax))))
    return [(tag, (b,) + box) for tag, box in t]


CropRun = namedtuple("CropRun", "S large nr extra")          # nr: "one" | "all" | "257"; extra: added to max_crop_h / max_crop_w


def crop_runs():
    runs = [CropRun(S, S == 7, nr, extra) for S in CROP_S for nr in ("one", "all", "257") for extra in (0, 13)]
    return runs + [CropRun(CROP_S_LARGE, True, "all", 0), CropRun(CROP_S_LARGE, True, "all", 13)]


def crop_id(r: CropRun) -> str:
    return f"S{r.S}-{'large-' if r.large else ''}{r.nr}-max+{r.extra}"


@functools.lru_cache(maxsize=None)
def crop_list(S: int, large: bool):
    """The tagged box list of one S.  The large image gets its boxes only at S = 7 (KS > 130) and S = 224 (alone)."""
    batch, dims = crop_batch(large)
    _, Hmax, Wmax, _ = batch.shape
    if S == CROP_S_LARGE:
        b, (ih, iw) = len(dims) - 1, LARGE_DIM
        return tuple((tag, (b,) + box) for tag, box in
                     [("full", (0, 0, iw, ih)), ("w_eq_S", (100, 50, 100 + S, 400)), ("h_eq_S", (7, 200, 500, 200 + S)),
                      ("straddle_corner", (600, 440, 700, 500))])
    out = []
    for b, (ih, iw) in enumerate(dims):
        if (int(ih), int(iw)) == LARGE_DIM:
            out += [("large_down", (b, 0, 0, int(iw), int(ih))), ("large_straddle", (b, 500, 300, 660, 490))]
        else:
            out += boxes_for(b, int(ih), int(iw), S, Hmax, Wmax)
    return tuple(out)


def crop_case(r: CropRun):
    """(batch, dims, boxes [NR][5] int32, max_crop_h, max_crop_w) of one run."""
    batch, dims = crop_batch(r.large)
    boxes = [b for _, b in crop_list(r.S, r.large)]
    if r.nr == "one":
        boxes = boxes[:1]
    elif r.nr == "257":
        boxes = (boxes * (257 // len(boxes) + 1))[:257]
    boxes = np.array(boxes, np.int32)
    mh, mw = int((boxes[:, 4] - boxes[:, 2]).max()), int((boxes[:, 3] - boxes[:, 1]).max())
    return batch, dims, boxes, max(mh, 1) + r.extra, max(mw, 1) + r.extra


@functools.lru_cache(maxsize=None)
def crop_expected(S: int, large: bool):
    """{box: Pillow's [3][S][S]} for every box of crop_list(S, large): computed once, shared, never changed."""
    images = crop_images(large)
    out = {}
    for _, box in crop_list(S, large):
        if box not in out:
            out[box] = pillow_crop(images[box[0]], box[1:], S)
            out[box].setflags(write=False)
    return out


def crop_want(r: CropRun, boxes):
    exp = crop_expected(r.S, r.large)
    return np.stack([exp[tuple(int(v) for v in b)] for b in boxes])


# a zero- or negative-extent box between two good ones: no index is formed, three zero planes, neighbours unaffected
DEGENERATE_BOXES = [(3, 0, 0, 30, 20), (3, 10, 5, 10, 20), (3, 2, 1, 40, 30), (3, 20, 9, 12, 30), (3, 5, 18, 25, 18), (3, 6, 30, 20, 11),
                    (3, 1, 1, 9, 9)]

PRE_DIMS = [(1, 1), (1, 50), (50, 1), (7, 7), (7, 21), (22, 7), (6, 8), (9, 10), (100, 150), (100, 151), (100, 153), (10, 333), (64, 48)]
PRE_S = [1, 2, 7, 16, 32]


def pre_dims(S: int):
    extra = {16: [(S, S), (S, 3 * S), (3 * S + 1, S), (S - 1, S + 5)], 32: [(1500, 2000)]}.get(S, [])
    return PRE_DIMS + extra


@functools.lru_cache(maxsize=None)
def pre_images(S: int):
    return tuple(_image(h, w, 7000 * h + w) for h, w in pre_dims(S))


@functools.lru_cache(maxsize=None)
def pre_batch(S: int):
    return make_batch(pre_images(S))


@functools.lru_cache(maxsize=None)
def pre_expected(S: int, norm: str):
    out = np.stack([hf_preprocess(im, S, *NORMS[norm]) for im in pre_images(S)])
    out.setflags(write=False)
    return out


def pre_geometry(h: int, w: int, S: int):
    shrt, lng = min(h, w), max(h, w)
    new_long = int(S * lng / shrt)
    return new_long, (S * lng) % shrt, shrt


# ------------------------------------------------------------------------------------------------ checking an output

def check_equal(got, want, what: str):
    """Bit-for-bit equality of fp32 arrays (a NaN, i.e. an unwritten element, is a difference)."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got.view(np.int32) != want.view(np.int32))
    if len(bad):
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {got.size} elements differ; first at {i}: got {got[i]!r}, want {want[i]!r}")


# ================================================================================================ ranking

RANK_SHAPES = [(1, 1, 4), (5, 5, 128), (64, 64, 4), (65, 129, 68), (63, 31, 36), (3, 32, 64), (3, 33, 64), (300, 77, 64),
               (130, 1001, 36), (37, 1000, 512)]
RANK_GT = ["null", "given", "minus1", "Bk"]
RankCase = namedtuple("RankCase", "Bq Bk P gt thr")        # thr: "ties" | "half" | "below" | "above"
U = 2.0 ** -24


def rank_slots(Bk: int) -> int:
    return -(-Bk // 64) * 2                  # 64-column tiles, two 32-column sub-tiles (one per wave) each


def rank_int_cases():
    cases = []
    for n, (Bq, Bk, P) in enumerate(RANK_SHAPES):
        for k, thr in enumerate(("ties", "half", "below", "above")):
            gt = RANK_GT[(n + k) % 4]
            if gt == "null" and Bk < Bq:
                gt = "given"
            cases.append(RankCase(Bq, Bk, P, gt, thr))
        for gt in ("null", "minus1", "Bk"):                     # every gt form at every shape that allows it, on ties
            if not (gt == "null" and Bk < Bq) and RankCase(Bq, Bk, P, gt, "ties") not in cases:
                cases.append(RankCase(Bq, Bk, P, gt, "ties"))
    return cases


def rank_id(c) -> str:
    return "-".join(str(v) for v in c)


def build_rank_int(c: RankCase):
    """Integer operands in [-2, 2]; candidate rows 1, 4, 7, 10 are bit-identical copies of row 0's ground truth.  Returns the
    operands, gt as the entry takes it (None = NULL), thr fp32, the int64 count, and idx / the integer dots for rowdot_gather."""
    rng = np.random.default_rng(c.Bq * 1000 + c.Bk)
    q = rng.integers(-2, 3, (c.Bq, c.P)).astype(np.float32)
    cand = rng.integers(-2, 3, (c.Bk, c.P)).astype(np.float32)
    given = rng.integers(0, c.Bk, c.Bq).astype(np.int32)
    for j in (1, 4, 7, 10):
        if j < c.Bk and j != given[0]:
            cand[j] = cand[given[0]]                            # bit-identical copies of row 0's ground truth
    gt = {"null": None, "given": given, "minus1": np.full(c.Bq, -1, np.int32), "Bk": np.full(c.Bq, c.Bk, np.int32)}[c.gt]
    self_col = np.arange(c.Bq) if gt is None else gt
    sim = q.astype(np.int64) @ cand.astype(np.int64).T
    own = sim[np.arange(c.Bq), np.clip(given, 0, c.Bk - 1)]
    if c.thr == "ties":
        thr = own.astype(np.float64)                            # equals every duplicate's score exactly, and many others
    elif c.thr == "half":
        thr = np.median(sim, axis=1).round() + 0.5
    else:
        thr = np.full(c.Bq, (sim.min() - 1.0) if c.thr == "below" else (sim.max() + 1.0))
    cols = np.arange(c.Bk)[None, :]
    want = ((sim > thr[:, None]) & (cols != self_col[:, None])).sum(axis=1)
    idx = given.copy()
    idx[0] = -1                                                 # clamped to 0
    idx[-1] = c.Bk                                              # clamped to Bk - 1
    dot_idx = sim[np.arange(c.Bq), np.clip(idx, 0, c.Bk - 1)]
    dot_null = sim[np.arange(c.Bq), np.clip(np.arange(c.Bq), 0, c.Bk - 1)]
    return dict(q=q, cand=cand, gt=gt, thr=thr.astype(np.float32), want=want.astype(np.int64), sim=sim, idx=idx, dot_idx=dot_idx,
                dot_null=dot_null, given=given, ties=int((sim == thr[:, None]).sum()))


def emulate_rank(q, cand, thr, gt, fault: str = None):
    """count [Bq] int32 as MODE_RANK + rank_merge_kernel compute it: per (64-column tile, 32-column half) fp32 partial counts
    in a NaN workspace, summed in slot order, (int)(s + 0.5)."""
    Bq, Bk = len(q), len(cand)
    slots = rank_slots(Bk)
    part = np.full((slots, Bq), np.nan, np.float32)
    pad = np.zeros((slots * 32, cand.shape[1]), np.float32)
    pad[:Bk] = cand
    sim = (q.astype(np.float32) @ pad.T).astype(np.float32)
    self_col = np.arange(Bq) if gt is None else np.asarray(gt)
    cols = np.arange(slots * 32)[None, :]
    hit = (sim >= thr[:, None]) if fault == "ge" else (sim > thr[:, None])
    if fault != "pad_cols":
        hit &= cols < Bk
    if fault != "gt_counted":
        hit &= cols != self_col[:, None]
    for s in range(slots):
        if not (fault == "slot_unwritten" and s == slots - 1):
            part[s] = hit[:, s * 32:(s + 1) * 32].sum(axis=1)
    tot = np.zeros(Bq, np.float32)
    for s in range(slots):
        tot = tot + part[s]
    if fault == "merge_down":
        return np.nextafter(tot, np.float32(0)).astype(np.int32)
    with np.errstate(invalid="ignore"):
        return (tot + np.float32(0.5)).astype(np.int32)


def check_rank_exact(count, want, what: str):
    count, want = np.asarray(count, np.int64), np.asarray(want, np.int64)
    bad = np.flatnonzero(count != want)
    assert not len(bad), f"{what}: {len(bad)} of {len(want)} rows differ; first row {bad[0]}: got {count[bad[0]]}, want {want[bad[0]]}"


def build_rank_gauss(Bq: int, Bk: int, P: int, dup: bool = False):
    """Gaussian, L2-normalised fp32 rows, seed Bq * 1000 + Bk.  dup: three candidates are copies of the ground truth of rows
    0, Bq // 2 and Bq - 1 each (none of them anyone's ground truth)."""
    rng = np.random.default_rng(Bq * 1000 + Bk)
    q = rng.standard_normal((Bq, P))
    cand = rng.standard_normal((Bk, P))
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    cand = (cand / np.linalg.norm(cand, axis=1, keepdims=True)).astype(np.float32)
    gt = rng.integers(0, Bk, Bq).astype(np.int32)
    dups = np.zeros((Bq, Bk), bool)
    if dup:
        rows = sorted({0, Bq // 2, Bq - 1})
        free = [j for j in range(Bk) if j not in set(gt.tolist())][:3 * len(rows)]
        assert len(free) == 3 * len(rows)
        for n, i in enumerate(rows):
            for j in free[3 * n:3 * n + 3]:
                cand[j] = cand[gt[i]]
                dups[i, j] = True
    return dict(q=q, cand=cand, gt=gt, dups=dups)


def rowdot_bound(a, b):
    """(ceil(P / 64) + 7) u sum |a_k b_k|: ceil(P/64) adds per lane, six butterfly steps, one product rounding."""
    P = a.shape[1]
    return (-(-P // 64) + 7) * U * (np.abs(a.astype(np.float64)) * np.abs(b.astype(np.float64))).sum(axis=1)


def rank_interval(q, cand, thr, gt, exclude=None):
    """(lo, hi) [Bq]: the counts with every score moved against / towards the threshold by §16's GEMM bound (P + 8) u (|q| |c|)."""
    q64, c64 = q.astype(np.float64), cand.astype(np.float64)
    sim = q64 @ c64.T
    e = (q.shape[1] + 8) * U * (np.abs(q64) @ np.abs(c64).T)
    keep = np.arange(cand.shape[0])[None, :] != np.asarray(gt)[:, None]
    if exclude is not None:
        keep &= ~exclude
    t = np.asarray(thr, np.float64)[:, None]
    return ((sim > t + e) & keep).sum(axis=1), ((sim > t - e) & keep).sum(axis=1)


def check_rank_interval(count, lo, hi, what: str, extra=None):
    """lo <= count <= hi (+ extra[i]: the duplicates of the ground truth, of which 0 .. 3 may be counted) on every row, and the
    interval itself is tight: sum (hi - lo) <= 0.5 % of sum hi, so no wrong count can hide in it."""
    count = np.asarray(count, np.int64)
    top = hi + (0 if extra is None else extra)
    bad = np.flatnonzero((count < lo) | (count > top))
    assert not len(bad), f"{what}: row {bad[0]}: count {count[bad[0]]} outside [{lo[bad[0]]}, {top[bad[0]]}] ({len(bad)} rows)"
    slack, total = int((hi - lo).sum()), int(hi.sum())
    assert slack <= 0.005 * total, f"{what}: the interval is not tight: sum(hi - lo) = {slack} of sum(hi) = {total}"
    return slack, total
