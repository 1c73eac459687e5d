"""TEST-ONLY references, case lists and emulations for the position-table resample, its transpose and the patch gather on a
gh x gw grid (dclip_amd/csrc/pos_interp.hip; tests/test_interp_paths_gpu.py on the GPU, tests/test_kernel_checks_interp_cpu.py
without one).

Nothing here imports the product.  The reference is the fp64 DEFINITION (include/dclip_hip.h; what
torch.nn.functional.interpolate(mode="bicubic", align_corners=False) computes in float64): per axis a [g_out, g] weight
matrix — source coordinate x = (o + 0.5) g / g_out - 0.5, taps floor(x) - 1 .. floor(x) + 2 clamped to [0, g - 1], taps that
clamp onto one cell added, cubic-convolution weights with A = -0.75 — applied with einsum; row 0 (the class position) is
copied.  The emulation restates the kernel's fp32 evaluation (fp64 weights rounded to fp32 once, their product in fp32, one
fused multiply-add chain, a outer, b inner) with `fault=` switches that plant one defect each; the CPU self-test shows that
every checker passes on the fault-free emulation and fails on each fault.

  * integer tables in [-8, 8] at ratios 2 and 1/2: every weight is k/256 or k/32, a product of two k/65536, so each of the
    16 terms is a multiple of 2^-16 below 2^3 and every partial sum needs at most 23 bits: exact in fp32 in any order.  The
    result must EQUAL the reference.  The backward (integer dout in [-2, 2]) is exact while taps x 2 x 2^16 < 2^24 for the
    source cell with the most contributing taps (`bwd_exact`).
  * Gaussian tables: every element within (16 + 8) 2^-24 sum |wy wx pos| of the reference — 16 roundings of the chain, and 8
    for the three roundings of a weight product (2 x 2^-24 relative each on every term, generously) — formed in fp64 from
    the reference's own weights; the backward the same with the cell's tap count in place of 16.
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
A_TORCH = -0.75

# (g, gh, gw, D): ratio 2 and 1/2 per axis (or 1), one cell, one output cell, the identity last
INT_CASES = [(4, 8, 8, 4), (4, 2, 2, 128), (2, 4, 4, 8), (7, 14, 14, 4), (14, 7, 7, 4), (3, 6, 3, 4), (4, 4, 8, 4), (1, 2, 2, 4),
             (2, 1, 1, 4), (7, 7, 7, 768)]
IDENTITY_CASE = (7, 7, 7, 768)
# non-integer ratios; the last one makes 1 + 37*37 = 1370 rows (577 tokens is 24 x 24 + 1, the second and third)
GAUSS_CASES = [(7, 10, 13, 768), (16, 24, 24, 1024), (7, 24, 24, 768), (2, 1, 5, 4), (7, 1, 1, 4), (16, 37, 37, 4)]
# what the fp64 reference is compared with torch's float64 interpolate on
TORCH_CASES = [(7, 14, 14), (7, 10, 13), (14, 7, 7), (7, 7, 7), (2, 1, 5), (16, 24, 24), (7, 1, 1), (1, 3, 2)]
FAULTS = ["A_half", "align_corners", "drop_clamped", "swap_axes", "cls_interp", "bwd_untransposed"]

# (B, C, H, W, p): square one patch; two grid extents; trailing rows and columns with W % 4 != 0 (scalar kernel); patch 14
# (scalar kernel); one channel; a single column of patches
RECT_CASES = [(1, 3, 16, 16, 16), (2, 3, 32, 48, 16), (2, 3, 35, 50, 16), (1, 3, 28, 42, 14), (3, 1, 8, 12, 4), (2, 3, 64, 36, 32)]


def case_id(c) -> str:
    return "-".join(str(v) for v in c)


# ------------------------------------------------------------------------------------------------ the definition

def cubic_weights(t, A: float = A_TORCH):
    """w(t + 1), w(t), w(1 - t), w(2 - t) of the cubic convolution kernel, fp64, shape [..., 4]."""
    t = np.asarray(t, np.float64)

    def w1(x):
        return ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0

    def w2(x):
        return ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A

    return np.stack([w2(t + 1.0), w1(t), w1(1.0 - t), w2(2.0 - t)], axis=-1)


def axis_taps(g: int, go: int, A: float = A_TORCH, align_corners: bool = False, drop_clamped: bool = False):
    """(idx [go, 4] int64, w [go, 4] fp64) of one axis resampled from g to go cells."""
    o = np.arange(go, dtype=np.float64)
    if align_corners:
        x = o * ((g - 1) / (go - 1)) if go > 1 else np.zeros(go)
    else:
        x = (o + 0.5) * (g / go) - 0.5
    f = np.floor(x)
    w = cubic_weights(x - f, A)
    raw = f.astype(np.int64)[:, None] + np.arange(-1, 3)[None, :]
    idx = np.clip(raw, 0, g - 1)
    if drop_clamped:
        w = np.where(raw == idx, w, 0.0)
    return idx, w


def axis_matrix(g: int, go: int, **kw) -> np.ndarray:
    """[go, g] fp64: row o holds the four weights of output o, clamped taps added onto the cell they land on."""
    idx, w = axis_taps(g, go, **kw)
    m = np.zeros((go, g), np.float64)
    np.add.at(m, (np.arange(go)[:, None].repeat(4, 1), idx), w)
    return m


def interp_reference(pos, g: int, gh: int, gw: int) -> np.ndarray:
    """fp64 [1 + gh*gw, D] from pos [1 + g*g, D]."""
    pos = np.asarray(pos, np.float64)
    D = pos.shape[1]
    grid = np.einsum("ya,xb,abd->yxd", axis_matrix(g, gh), axis_matrix(g, gw), pos[1:].reshape(g, g, D))
    return np.concatenate([pos[:1], grid.reshape(gh * gw, D)], 0)


def interp_bwd_reference(dout, g: int, gh: int, gw: int) -> np.ndarray:
    """The transpose, fp64 [1 + g*g, D] from dout [1 + gh*gw, D]."""
    dout = np.asarray(dout, np.float64)
    D = dout.shape[1]
    grid = np.einsum("ya,xb,yxd->abd", axis_matrix(g, gh), axis_matrix(g, gw), dout[1:].reshape(gh, gw, D))
    return np.concatenate([dout[:1], grid.reshape(g * g, D)], 0)


def fwd_magnitude(pos, g: int, gh: int, gw: int) -> np.ndarray:
    """sum |wy wx pos| per output element, fp64 (the weights taken per tap: clamped taps count separately)."""
    pos = np.abs(np.asarray(pos, np.float64))
    D = pos.shape[1]
    (iy, wy), (ix, wx) = axis_taps(g, gh), axis_taps(g, gw)
    my, mx = np.zeros((gh, g)), np.zeros((gw, g))
    np.add.at(my, (np.arange(gh)[:, None].repeat(4, 1), iy), np.abs(wy))
    np.add.at(mx, (np.arange(gw)[:, None].repeat(4, 1), ix), np.abs(wx))
    grid = np.einsum("ya,xb,abd->yxd", my, mx, pos[1:].reshape(g, g, D))
    return np.concatenate([pos[:1], grid.reshape(gh * gw, D)], 0)


def bwd_magnitude(dout, g: int, gh: int, gw: int) -> np.ndarray:
    dout = np.abs(np.asarray(dout, np.float64))
    D = dout.shape[1]
    (iy, wy), (ix, wx) = axis_taps(g, gh), axis_taps(g, gw)
    my, mx = np.zeros((gh, g)), np.zeros((gw, g))
    np.add.at(my, (np.arange(gh)[:, None].repeat(4, 1), iy), np.abs(wy))
    np.add.at(mx, (np.arange(gw)[:, None].repeat(4, 1), ix), np.abs(wx))
    grid = np.einsum("ya,xb,yxd->abd", my, mx, dout[1:].reshape(gh, gw, D))
    return np.concatenate([dout[:1], grid.reshape(g * g, D)], 0)


def tap_counts(g: int, gh: int, gw: int) -> np.ndarray:
    """[g, g]: how many (destination row, a, b) taps land on each source cell — the length of the backward's chain there."""
    iy, _ = axis_taps(g, gh)
    ix, _ = axis_taps(g, gw)
    cy, cx = np.bincount(iy.ravel(), minlength=g), np.bincount(ix.ravel(), minlength=g)
    return np.outer(cy, cx)


def bwd_exact(c) -> bool:
    """Is the backward's sum on integer dout in [-2, 2] exact in fp32 in any order?  (taps x 2 x 2^16 < 2^24)"""
    g, gh, gw, _ = c
    return int(tap_counts(g, gh, gw).max()) * 2 * 2 ** 16 < 2 ** 24


# ------------------------------------------------------------------------------------------------ operands

def build_int_table(g: int, D: int, seed: int = 0) -> np.ndarray:
    return np.random.default_rng(1000 * g + D + seed).integers(-8, 9, (1 + g * g, D)).astype(np.float32)


def build_int_dout(gh: int, gw: int, D: int, seed: int = 0) -> np.ndarray:
    return np.random.default_rng(77 * gh + gw + D + seed).integers(-2, 3, (1 + gh * gw, D)).astype(np.float32)


def build_gauss(rows: int, D: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).standard_normal((rows, D)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the kernel's arithmetic

def _fmaf(w, v, acc):
    """fp32 fused multiply-add: the product of two fp32 values is exact in fp64; the sum is rounded to fp64 and then to fp32
    (a double rounding differs from the single one in about 1 of 2^29 cases: an emulation, not a bit-exact model)."""
    return (w.astype(np.float64) * v.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)


def _taps32(g, go, fault):
    idx, w = axis_taps(g, go, A=-0.5 if fault == "A_half" else A_TORCH, align_corners=fault == "align_corners",
                       drop_clamped=fault == "drop_clamped")
    return idx, w.astype(np.float32)


def emulate_fwd(pos, g: int, gh: int, gw: int, fault: str = None) -> np.ndarray:
    pos = np.asarray(pos, np.float32)
    D = pos.shape[1]
    out = np.zeros((1 + gh * gw, D), np.float32)
    if fault == "swap_axes":               # the linear row index decoded on a gw x gh grid
        (iy, wy), (ix, wx), cols = _taps32(g, gw, fault), _taps32(g, gh, fault), gh
    else:
        (iy, wy), (ix, wx), cols = _taps32(g, gh, fault), _taps32(g, gw, fault), gw
    for r in range(gh * gw):
        oy, ox = divmod(r, cols)
        acc = np.zeros(D, np.float32)
        for a in range(4):
            for b in range(4):
                w = np.float32(wy[oy, a] * wx[ox, b])
                acc = _fmaf(np.full(D, w, np.float32), pos[1 + iy[oy, a] * g + ix[ox, b]], acc)
        out[1 + r] = acc
    out[0] = out[1] if fault == "cls_interp" else pos[0]
    return out


def emulate_bwd(dout, g: int, gh: int, gw: int, prior=None, fault: str = None) -> np.ndarray:
    """Gather form: per source cell the destination rows in ascending order, a outer, b inner; `prior` (accumulate) is added
    last."""
    dout = np.asarray(dout, np.float32)
    D = dout.shape[1]
    if fault == "bwd_untransposed":        # the forward's weights applied from the destination grid back to the source grid
        iy, wy = _taps32(gh, g, None)
        ix, wx = _taps32(gw, g, None)
        out = np.zeros((1 + g * g, D), np.float32)
        for r in range(g * g):
            sy, sx = divmod(r, g)
            acc = np.zeros(D, np.float32)
            for a in range(4):
                for b in range(4):
                    w = np.float32(wy[sy, a] * wx[sx, b])
                    acc = _fmaf(np.full(D, w, np.float32), dout[1 + iy[sy, a] * gw + ix[sx, b]], acc)
            out[1 + r] = acc
        out[0] = dout[0]
    else:
        if fault == "swap_axes":
            (iy, wy), (ix, wx), cols = _taps32(g, gw, fault), _taps32(g, gh, fault), gh
        else:
            (iy, wy), (ix, wx), cols = _taps32(g, gh, fault), _taps32(g, gw, fault), gw
        out = np.zeros((1 + g * g, D), np.float32)
        for r in range(gh * gw):
            oy, ox = divmod(r, cols)
            for a in range(4):
                for b in range(4):
                    w = np.float32(wy[oy, a] * wx[ox, b])
                    s = 1 + iy[oy, a] * g + ix[ox, b]
                    out[s] = _fmaf(np.full(D, w, np.float32), dout[1 + r], out[s])
        out[0] = dout[1] if fault == "cls_interp" else dout[0]
    if prior is not None:
        out = (out + np.asarray(prior, np.float32)).astype(np.float32)
    return out


# ------------------------------------------------------------------------------------------------ checkers

def check_exact(got, want64, what: str):
    """Equality with an fp64 result that fp32 holds exactly (a NaN — an unwritten element — is a difference)."""
    got = np.asarray(got, np.float32)
    want = np.asarray(want64, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want), f"{what}: the reference is not an fp32 value"
    bad = np.argwhere(~(got.astype(np.float64) == want))
    if len(bad):
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {got.size} elements differ; first at {i}: got {got[i]!r}, want {want[i]!r}")


def check_bits(got, want, what: str):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got.view(np.int32) != want.view(np.int32))
    if len(bad):
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {got.size} elements differ in bits; first at {i}: {got[i]!r} / {want[i]!r}")


def check_bound(got, want64, bound, what: str) -> float:
    """|got - want| <= bound element-wise (a non-finite element fails).  Returns the worst error / bound."""
    got = np.asarray(got, np.float64)
    assert got.shape == want64.shape, (what, got.shape, want64.shape)
    err = np.abs(got - want64)
    bad = np.argwhere(~(err <= bound))
    if len(bad):
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {got.size} elements outside the bound; first at {i}: got {got[i]!r}, "
                             f"want {want64[i]!r}, bound {bound[i]!r}")
    return float((err / np.maximum(bound, 1e-300)).max())


def check_fwd_int(got, pos, c):
    g, gh, gw, _ = c
    check_exact(got, interp_reference(pos, g, gh, gw), f"pos_interp_fwd {case_id(c)}")


def check_bwd_int(got, dout, c, prior=None):
    g, gh, gw, _ = c
    want = interp_bwd_reference(dout, g, gh, gw)
    if prior is not None:
        want = want + np.asarray(prior, np.float64)
    check_exact(got, want, f"pos_interp_bwd {case_id(c)}")


def check_fwd_gauss(got, pos, c) -> float:
    g, gh, gw, _ = c
    bound = (16 + 8) * U * fwd_magnitude(pos, g, gh, gw)
    bound[0] = 0.0                                   # the class row is a copy
    return check_bound(got, interp_reference(pos, g, gh, gw), bound, f"pos_interp_fwd {case_id(c)}")


def check_bwd_gauss(got, dout, c) -> float:
    g, gh, gw, _ = c
    n = np.concatenate([[0], tap_counts(g, gh, gw).ravel()]).astype(np.float64)[:, None]
    bound = (n + 8) * U * bwd_magnitude(dout, g, gh, gw)
    bound[0] = 0.0
    return check_bound(got, interp_bwd_reference(dout, g, gh, gw), bound, f"pos_interp_bwd {case_id(c)}")


# ------------------------------------------------------------------------------------------------ patch gather

def build_rect_pixels(c) -> np.ndarray:
    """Integer pixels; NaN in every row >= gh*p and column >= gw*p (never read)."""
    B, C, H, W, p = c
    pix = np.random.default_rng(H * 100 + W).integers(-9, 10, (B, C, H, W)).astype(np.float32)
    pix[:, :, (H // p) * p:, :] = np.nan
    pix[:, :, :, (W // p) * p:] = np.nan
    return pix


def rect_reference(pix: np.ndarray, p: int) -> np.ndarray:
    B, C, H, W = pix.shape
    gh, gw = H // p, W // p
    v = pix[:, :, :gh * p, :gw * p].reshape(B, C, gh, p, gw, p)
    return np.ascontiguousarray(v.transpose(0, 2, 4, 1, 3, 5)).reshape(B * gh * gw, C * p * p)


def rect_variant(c) -> str:
    _, _, _, W, p = c
    return ".vec" if p % 4 == 0 and W % 4 == 0 else ".scalar"
