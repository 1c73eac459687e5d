"""TEST-ONLY checkers and case lists for the split-fp16 kernels of dclip_amd/csrc/split16.hip through the C ABI (DESIGN.md §25;
tests/test_split16_paths_gpu.py, self-tested without a GPU by tests/test_kernel_checks_split16_cpu.py).

Built on tests/kernel_checks.py and tests/kernel_checks_rest.py (Guarded, poisoned, Report, vec, the LayerNorm bound); nothing
here imports the product.  The rules are RESTATED from include/dclip_hip.h and the kernels' comments, in torch fp64 / integer
arithmetic; the CPU file then asserts that engine.split16_* agree with these restatements.  Every family has
  build_*(case, device)   operands with NaN in everything the contract says is not read, outputs in guarded NaN-filled buffers;
  launch_*(lib, s, st)    the C ABI call(s);
  *_site(case)            what dclip_last_launch() (and, for the fused pass, dclip_first_launch()) must report;
  emulate_*(s, fault)     the restatement writing the same buffers on the host; `fault` plants one defect;
  verify_*(s)             guards, then every element EXACT (bit for bit; a NaN need only be a NaN) or under a derived bound.
The split itself: v = fp32(x s), hi = fp16(v), lo = fp16(v - hi) (v - hi is exact), so |hi + lo - v| <= 2^-22 |v| + 2^-25 for a
finite |v| <= 2^14: two round-to-nearest steps of 11 bits each, plus half the spacing of fp16's subnormals."""
from __future__ import annotations

import math
import struct
from collections import namedtuple
from types import SimpleNamespace

import torch

from tests.kernel_checks import E_INVAL, E_WORKSPACE, NAN, Guarded, poisoned, roundup     # noqa: F401  (re-exported)
from tests import kernel_checks_rest as kr
from tests.kernel_checks_rest import Report, gen, vec

INF = float("inf")
HALF = torch.float16
TOP = 14                              # operands are scaled into [2^13, 2^14)
RECON_REL, RECON_ABS, RECON_MAX = 2.0 ** -22, 2.0 ** -25, 2.0 ** 14
WS_BEHIND = 1024                      # floats (4096 bytes) behind a workspace's exact size that must stay NaN


# ==================================================================================================== the rules, restated

def host_split(x: torch.Tensor, scale):
    """(hi, lo) fp16 of fp32 x times a power of two (a float, or a tensor that broadcasts): the product in fp64, rounded to fp32
    (exact unless it leaves fp32's range), hi = fp16(v), lo = fp16(v - hi) with the difference formed exactly in fp64."""
    v = (x.double() * scale).float()
    hi = v.half()
    lo = (v.double() - hi.double()).float().half()
    return hi, lo


def layout3(hi, lo, order: int):
    return torch.cat([hi, lo, hi] if order == 0 else [hi, hi, lo], dim=1)


def exp_rule(r: torch.Tensor, clamp: int = 100, pow2_shift: int = 0) -> torch.Tensor:
    """The row / column exponent of a maximum r >= 0 (fp64): r = mu 2^x with mu in [0.5, 1) gives e = 14 - x, clamped to
    [-100, 100]; 0 when r is 0, inf or NaN.  (`clamp`, `pow2_shift`: the planted faults.)"""
    mant, ex = torch.frexp(torch.where(torch.isfinite(r), r, torch.ones_like(r)))
    e = TOP - ex
    if pow2_shift:
        e = torch.where(mant == 0.5, e + pow2_shift, e)
    e = e.clamp(-clamp, clamp)
    return torch.where((r == 0) | ~torch.isfinite(r), torch.zeros_like(e), e).to(torch.int32)


def pow2(e: torch.Tensor) -> torch.Tensor:
    return torch.exp2(e.double()).float()


def rows_expect(x: torch.Tensor, e=None):
    """dclip_split_f32_f16x3_rows of a host matrix: (y fp16 [rows][3 cols] = [hi|lo|hi] of x[m] 2^e_m, row_alpha = 2^-e_m, e)."""
    if e is None:
        e = exp_rule(x.double().abs().amax(dim=1))
    hi, lo = host_split(x, torch.exp2(e.double())[:, None])
    return layout3(hi, lo, 0), pow2(-e), e


def check_pieces(rep: Report, name: str, got, want):
    rep.rounded16(name, got, want)


def check_recon(rep: Report, name: str, hi, lo, v64):
    """The independent bound: |hi + lo - v| <= 2^-22 |v| + 2^-25 wherever v is finite and |v| <= 2^14."""
    ok = torch.isfinite(v64) & (v64.abs() <= RECON_MAX)
    if bool(ok.any()):
        rep.bound(name, (hi.double() + lo.double())[ok], v64[ok], RECON_REL * v64[ok].abs() + RECON_ABS)


def trunc_lo(x, scale):
    """host_split with lo TRUNCATED towards zero (a planted fault)."""
    hi, lo = host_split(x, scale)
    d = (x.double() * scale).float().double() - hi.double()
    over = torch.isfinite(d) & (lo.double().abs() > d.abs())
    bits = lo.view(torch.int16).clone()
    bits[over] -= 1                                         # one step towards zero in sign-magnitude
    return hi, bits.view(HALF)


def spread(shape, seed, lo=-14, hi=12):
    """Gaussian values times 2^U(lo, hi) per element."""
    g = gen(seed)
    return torch.randn(tuple(shape), generator=g) * torch.exp2(torch.randint(lo, hi + 1, tuple(shape), generator=g).float())


SPECIALS = [0.0, -0.0, INF, -INF, NAN, 65504.0, 65520.0, -65519.0, 2.0 ** -24, 2.0 ** -25, -(2.0 ** -14), 1.0 + 2.0 ** -11,
            1.0 + 2.0 ** -10 + 2.0 ** -22, 2.0 ** 14, 3.0e38, 1.0e-40]


# ==================================================================================================== 1. stand-alone split

SplitCase = namedtuple("SplitCase", "rows cols xpad ypad order dev sexp")
SPLIT_ROWS, SPLIT_COLS, SPLIT_SEXP = [1, 3, 130], [8, 72, 520], [0, 9, -3]
SPLIT_BIG = (4104, 4096)              # rows cols / 8 = 2,101,248 > 8192 * 256 = 2,097,152: a second grid-stride trip
SPLIT_GRID = 8192 * 256


def split_cases():
    out, i = [], 0
    for rows in SPLIT_ROWS:
        for cols in SPLIT_COLS:
            for xpad in (0, 4):
                for ypad in (0, 8):
                    for order in (0, 1):
                        out.append(SplitCase(rows, cols, xpad, ypad, order, bool((i // 2 + i // 8) % 2), SPLIT_SEXP[i % 3]))
                        i += 1
    return out


def split_big_cases():
    return [SplitCase(*SPLIT_BIG, 0, 0, 0, True, 9), SplitCase(*SPLIT_BIG, 4, 8, 1, False, -3)]


def split_id(c) -> str:
    return f"{c.rows}x{c.cols}-ldx{c.xpad}-ldy{c.ypad}-o{c.order}-{'dev' if c.dev else 'host'}-s{c.sexp}"


def split_site(c) -> str:
    return "split_f32_f16x3" + ("_dev" if c.dev else "") + (".act" if c.order == 0 else ".weight")


def split_data(c) -> torch.Tensor:
    x = spread((c.rows, c.cols), 31 * c.rows + c.cols + c.order) * 2.0 ** -c.sexp       # |x s| mostly below 2^14
    flat = x.view(-1)
    k = min(len(SPECIALS), flat.numel() // 2)
    flat[1:2 * k:2] = torch.tensor(SPECIALS[:k]) * 2.0 ** -c.sexp
    return x


def build_split(c: SplitCase, device="cpu"):
    x = split_data(c)
    return SimpleNamespace(case=c, x=x, xd=poisoned(x, c.cols + c.xpad, device),
                           y=Guarded(c.rows, 3 * c.cols, 3 * c.cols + c.ypad, device=device, dtype=HALF),
                           scale=vec(1, device, fill=2.0 ** c.sexp))


def launch_split(lib, s, stream) -> int:
    c = s.case
    if c.dev:
        return lib.dclip_split_f32_f16x3_dev(s.xd.data_ptr(), s.y.ptr, c.rows, c.cols, c.cols + c.xpad, s.y.ld, s.scale.ptr, c.order,
                                             stream)
    return lib.dclip_split_f32_f16x3(s.xd.data_ptr(), s.y.ptr, c.rows, c.cols, c.cols + c.xpad, s.y.ld, 2.0 ** c.sexp, c.order, stream)


def emulate_split(s, fault=None):
    c = s.case
    sc = 2.0 ** c.sexp
    hi, lo = trunc_lo(s.x, sc) if fault == "lo_truncated" else host_split(s.x, sc)
    if fault == "lo_unscaled":
        lo = ((s.x.double() * sc).float().double() - hi.double()).div(sc).float().half()
    s.y.payload.copy_(layout3(hi, lo, c.order if fault != "order" else 1 - c.order))
    if fault == "pad" and c.ypad:
        s.y.mat[c.rows - 1, 3 * c.cols] = 1.0
    if fault == "behind":
        s.y.buf[s.y.guard + c.rows * s.y.ld] = 0
    if fault == "scale_written":
        s.scale.buf[s.scale.guard + 1] = 0


def verify_split(s, what=None):
    c = s.case
    rep = Report(what or f"{split_site(c)} {split_id(c)}")
    rep.guards(y=s.y, scale=s.scale)
    sc = 2.0 ** c.sexp
    hi, lo = host_split(s.x, sc)
    got = s.y.get()
    check_pieces(rep, "y", got, layout3(hi, lo, c.order))
    n = c.cols
    ghi, glo = got[:, :n], (got[:, n:2 * n] if c.order == 0 else got[:, 2 * n:])
    check_recon(rep, "hi+lo", ghi, glo, s.x.double() * sc)
    if not torch.equal(kr.ibits(s.scale.get()), kr.ibits(torch.tensor([[sc]]))):
        rep.fail("scale: the device scalar was written")
    return rep.done()


# ==================================================================================================== 2. row split

WIDTHS = [8, 512, 520, 1024, 1032, 1536, 1544, 2048, 2056, 2560, 2568, 3072, 3080]      # both sides of every chunk boundary
ROWS_ROWS = [1, 3, 4, 5, 9]
RowsCase = namedtuple("RowsCase", "rows cols xpad kind")
CRAFTED = (["first%d" % p for p in range(8)] + ["last%d" % p for p in range(8)] + ["mid%d" % p for p in range(8)] +
           ["zero", "inf", "nan", "subnormal", "huge", "pow2", "negpow2", "negmax"])


def rows_cases():
    out = [RowsCase(rows, cols, 4 * ((i + j) % 2), "random") for i, cols in enumerate(WIDTHS) for j, rows in enumerate(ROWS_ROWS)]
    out += [RowsCase(len(CRAFTED), cols, xpad, "crafted") for cols in WIDTHS for xpad in (0, 4)]
    return out


def rows_id(c) -> str:
    return f"{c.rows}x{c.cols}-ldx{c.xpad}-{c.kind}"


def rows_variant(cols: int) -> str:
    nc = -(-(cols // 8) // 64)
    return ".regs.nc%d" % max(nc, 1) if nc <= 6 else ".cached"


def rows_site(c) -> str:
    return "split_f32_f16x3_rows" + rows_variant(c.cols)


def crafted_rows(cols: int, seed: int) -> torch.Tensor:
    """One row per entry of CRAFTED.  A plain row holds values in [0.1, 0.2) with random signs and ONE maximum 1.5 2^k, three
    binades above the rest, at a chosen position of the first / last / a middle group of 8 columns."""
    g = gen(seed)
    n = len(CRAFTED)
    x = (torch.rand((n, cols), generator=g) * 0.1 + 0.1) * (torch.randint(0, 2, (n, cols), generator=g).float() * 2 - 1)
    groups = cols // 8
    for r, kind in enumerate(CRAFTED):
        k = (r * 7) % 41 - 20
        if kind[:-1] in ("first", "last", "mid"):
            grp = {"first": 0, "last": groups - 1, "mid": groups // 2}[kind[:-1]]
            x[r] *= 2.0 ** k
            x[r, grp * 8 + int(kind[-1])] = 1.5 * 2.0 ** k * (-1) ** r
        elif kind == "zero":
            x[r] = 0.0
            x[r, ::3] = -0.0
        elif kind == "inf":
            x[r, cols - 3] = -INF
        elif kind == "nan":
            x[r, cols // 2] = NAN
        elif kind == "subnormal":
            x[r] = torch.randint(-(1 << 20), 1 << 20, (cols,), generator=g).float() * 2.0 ** -149
            x[r, cols - 1] = (1 << 21) * 2.0 ** -149
        elif kind == "huge":
            x[r] *= 2.0 ** 110
            x[r, 5 % cols] = 1.25 * 2.0 ** 116
        elif kind in ("pow2", "negpow2"):
            x[r, cols - 2] = 4.0 if kind == "pow2" else -(2.0 ** -7)
            if kind == "negpow2":
                x[r] = torch.where(x[r].abs() > 2.0 ** -7, x[r] * 2.0 ** -6, x[r])
        elif kind == "negmax":
            x[r, 0] = -3.0
    return x


def rows_data(c) -> torch.Tensor:
    if c.kind == "crafted":
        return crafted_rows(c.cols, c.cols + c.xpad)
    g = gen(1000 * c.rows + c.cols)
    x = spread((c.rows, c.cols), 17 * c.rows + c.cols, -6, 0) * torch.exp2(torch.randint(-30, 31, (c.rows, 1), generator=g).float())
    for r in range(c.rows):                                # the maximum walks through the positions and the groups
        grp = (0, c.cols // 8 - 1, c.cols // 16)[(r + c.cols // 8) % 3]
        x[r, grp * 8 + (r + c.cols // 8) % 8] = x[r].abs().max() * 2.5
    return x


def build_rows(c: RowsCase, device="cpu"):
    x = rows_data(c)
    return SimpleNamespace(case=c, x=x, xd=poisoned(x, c.cols + c.xpad, device), y=Guarded(c.rows, 3 * c.cols, device=device, dtype=HALF),
                           ra=vec(c.rows, device))


def launch_rows(lib, s, stream) -> int:
    c = s.case
    return lib.dclip_split_f32_f16x3_rows(s.xd.data_ptr(), s.y.ptr, s.ra.ptr, c.rows, c.cols, c.cols + c.xpad, stream)


def faulty_row_max(x, fault):
    a = x.double().abs()
    cols = x.shape[1]
    if fault == "no_tail":                                 # the chunk past the last full 64 groups is left out of the maximum
        full = (cols // 8) // 64 * 512
        if 0 < full < cols:
            a = a[:, :full]
    if fault == "elem0":                                   # element 0 of each 4-vector stands for all four
        a = a.view(x.shape[0], -1, 4)[:, :, 0]
    return a.amax(dim=1)


def emulate_rows(s, fault=None):
    c = s.case
    r = faulty_row_max(s.x, fault)
    e = exp_rule(r, clamp=99 if fault == "clamp99" else 100, pow2_shift=1 if fault == "pow2_off" else 0)
    y, ra, _ = rows_expect(s.x, e)
    s.y.payload.copy_(y)
    s.ra.payload.copy_(ra[None])
    if fault == "alpha_behind":
        s.ra.buf[s.ra.guard + c.rows] = 0
    if fault == "y_behind":
        s.y.buf[s.y.guard + c.rows * s.y.ld] = 0


def verify_rows(s, what=None):
    c = s.case
    rep = Report(what or f"{rows_site(c)} {rows_id(c)}")
    rep.guards(y=s.y, row_alpha=s.ra)
    want_y, want_ra, e = rows_expect(s.x)
    got = s.y.get()
    rep.bits("row_alpha", s.ra.get()[0], want_ra)
    check_pieces(rep, "y", got, want_y)
    n = c.cols
    if not torch.equal(kr.ibits(got[:, :n]), kr.ibits(got[:, 2 * n:])):
        rep.fail("y: the third piece is not the first")
    check_recon(rep, "hi+lo", got[:, :n], got[:, n:2 * n], s.x.double() * torch.exp2(e.double())[:, None])
    return rep.done()


# ==================================================================================================== 3. fused pass

COL_ROWS = [1, 2, 3, 4, 5, 8, 9, 33]
COL_BIG_ROWS, COL_BIG_COLS = 8200, [8, 520]
ColCase = namedtuple("ColCase", "rows cols xpad kind db")


def col_cases():
    out = []
    for i, cols in enumerate(WIDTHS):
        for j, rows in enumerate(COL_ROWS):
            out.append(ColCase(rows, cols, 4 * ((i + j) % 2), "dyadic" if (i + j) % 2 else "spread", (i + j) % 3 != 0))
    for cols in COL_BIG_COLS:
        out += [ColCase(COL_BIG_ROWS, cols, 4, "dyadic", True), ColCase(COL_BIG_ROWS, cols, 0, "spread", True)]
    return out


def col_big_cases():
    """rows cols / 8 = 2,107,400 > 8192 * 256: the column split (split_cols_f16x2_kernel) makes a second grid-stride trip."""
    return [ColCase(COL_BIG_ROWS, 2056, 0, "dyadic", True)]


def col_id(c) -> str:
    return f"{c.rows}x{c.cols}-ldx{c.xpad}-{c.kind}-{'db' if c.db else 'nodb'}"


def col_waves(rows: int) -> int:
    """W = roundup4(min(ceil(rows / 8), 1024)): wave w takes rows w, w + W, ..."""
    return roundup(min(-(-rows // 8), 1024), 4)


def col_workspace_floats(rows: int, cols: int) -> int:
    return 2 * col_waves(rows) * cols


def col_sites(c):
    """(dclip_first_launch, dclip_last_launch)"""
    return "split_f32_f16x3_rows_colstats" + rows_variant(c.cols), "split_f32_f16x3_rows_colstats.cols"


def last_wave_row(rows: int) -> int:
    """A row that only the last wave with any row takes (its last one)."""
    W = col_waves(rows)
    w = min(W, rows) - 1
    return w + (rows - 1 - w) // W * W


def col_data(c) -> torch.Tensor:
    g = gen(13 * c.rows + c.cols + c.xpad)
    if c.kind == "dyadic":
        # integers in [-8, 8] times a power of two per column: every column sum is exact in fp32 in any order.  The column
        # maximum (16) sits in row 0, in the last row, or in a row that only the last wave takes
        x = torch.randint(-8, 9, (c.rows, c.cols), generator=g).float()
        where = (0, c.rows - 1, last_wave_row(c.rows))
        for k in range(3):
            x[where[k], k::3] = 16.0 * (-1) ** k
            for kk in range(3):                            # ... and nowhere else in that column
                if where[kk] != where[k]:
                    x[where[kk], k::3] = x[where[kk], k::3].clamp(-8, 8)
        return x * torch.exp2(torch.randint(-20, 21, (1, c.cols), generator=g).float())
    # the recipe of tests/test_vision_split16_wgrad_gpu.py, restated: rows and columns spread over e^(4 sigma); column 0 all
    # zero, 1 with one inf, 2 with one NaN, 3 subnormal only, 4 holding 1e-30 beside one 1e+10
    x = torch.randn((c.rows, c.cols), generator=g) * torch.exp(4.0 * torch.randn((c.rows, 1), generator=g)) \
        * torch.exp(4.0 * torch.randn((1, c.cols), generator=g))
    x[:, 0] = 0.0
    x[0, 1] = INF
    x[min(1, c.rows - 1), 2] = NAN
    x[:, 3] = torch.randint(1, 1 << 20, (c.rows,), generator=g).float() * 2.0 ** -149
    x[:, 4] = 1e-30
    x[c.rows // 2, 4] = 1e10
    return x


def build_col(c: ColCase, device="cpu"):
    x = col_data(c)
    floats = col_workspace_floats(c.rows, c.cols)
    return SimpleNamespace(case=c, x=x, xd=poisoned(x, c.cols + c.xpad, device), y=Guarded(c.rows, 3 * c.cols, device=device, dtype=HALF),
                           ra=vec(c.rows, device), yc=Guarded(c.rows, 2 * c.cols, device=device, dtype=HALF), ce=vec(c.cols, device),
                           ca=vec(c.cols, device), db=vec(c.cols, device), ws=vec(floats + WS_BEHIND, device), ws_bytes=4 * floats)


def launch_col(lib, s, stream, ws_bytes=None) -> int:
    c = s.case
    return lib.dclip_split_f32_f16x3_rows_colstats(s.xd.data_ptr(), s.y.ptr, s.ra.ptr, s.yc.ptr, s.ce.ptr, s.ca.ptr,
                                                   s.db.ptr if c.db else None, c.rows, c.cols, c.cols + c.xpad, s.ws.ptr,
                                                   s.ws_bytes if ws_bytes is None else ws_bytes, stream)


def emulate_col(s, fault=None):
    """The three launches as the header of the kernel states them, fp32 sums in the kernels' order; the workspace is written as
    the first launch writes it (a wave without a row writes nothing)."""
    c = s.case
    rows, cols = c.rows, c.cols
    x = s.x
    y, ra, _ = rows_expect(x)
    s.y.payload.copy_(y)
    s.ra.payload.copy_(ra[None])
    W = col_waves(rows)
    nw = min(W, rows)
    ws = s.ws.payload[0]
    pmax = ws[:W * cols].view(torch.int32).view(W, cols)
    psum = ws[W * cols:2 * W * cols].view(W, cols)
    bits = x.abs().view(torch.int32)
    for w in range(nw):
        mine = list(range(w, rows, W))
        if fault == "wave_last_row" and len(mine) > 1:
            mine = mine[:-1]
        acc = torch.zeros(cols)
        for r in mine:
            acc = acc + x[r]
        pmax[w] = bits[mine].amax(dim=0)
        psum[w] = acc
    fold = W if fault == "fold_W" else nw                  # the finish: 32 groups fold partials g, g + 32, ... then group 0 folds them
    m = torch.zeros(cols, dtype=torch.int32)
    tot = torch.zeros(cols)
    for g in range(32):
        gs = torch.zeros(cols)
        for w in range(g, fold, 32):
            m = torch.maximum(m, pmax[w])
            gs = gs + psum[w]
        tot = gs if g == 0 else tot + gs
    e = exp_rule(m.view(torch.float32).double())
    s.ce.payload.copy_(e.view(torch.float32)[None])
    s.ca.payload.copy_(pow2(-e)[None])
    if c.db:
        s.db.payload.copy_(tot[None])
    ec = torch.roll(e, 1) if fault == "neighbour_col" else e
    hi, lo = host_split(x, torch.exp2(ec.double())[None, :])
    s.yc.payload.copy_(torch.cat([hi, lo], dim=1))
    if fault == "ws_behind":
        s.ws.payload[0, 2 * W * cols] = 0.0
    if fault == "yc_behind":
        s.yc.buf[s.yc.guard + rows * s.yc.ld] = 0
    if fault == "ce_behind":
        s.ce.buf[s.ce.guard + cols] = 0


def verify_col(s, what=None):
    c = s.case
    rep = Report(what or f"rows_colstats {col_id(c)}")
    rep.guards(y=s.y, row_alpha=s.ra, yc=s.yc, col_exp=s.ce, col_alpha=s.ca, db=s.db, workspace=s.ws)
    x = s.x
    want_y, want_ra, _ = rows_expect(x)                    # §2's reference, not the sibling entry
    rep.bits("row_alpha", s.ra.get()[0], want_ra)
    check_pieces(rep, "y", s.y.get(), want_y)
    e = exp_rule(x.double().abs().amax(dim=0))
    rep.exact("col_exp", s.ce.get()[0].view(torch.int32), e)
    rep.bits("col_alpha", s.ca.get()[0], pow2(-e))
    hi, lo = host_split(x, torch.exp2(e.double())[None, :])
    yc = s.yc.get()
    check_pieces(rep, "yc", yc, torch.cat([hi, lo], dim=1))
    check_recon(rep, "yc hi+lo", yc[:, :c.cols], yc[:, c.cols:], x.double() * torch.exp2(e.double())[None, :])
    db = s.db.get()[0]
    if not c.db:
        if not bool(torch.isnan(db).all()):
            rep.fail("db: written although the pointer passed was null")
    else:
        want = x.double().sum(dim=0)
        fin = torch.isfinite(x).all(dim=0)
        if c.kind == "dyadic":
            rep.exact("db", db, want)
        else:
            if bool(torch.isfinite(db[~fin]).any()):
                rep.fail("db: a finite sum for a column that holds inf or NaN")
            rep.bound("db", db[fin], want[fin], (c.rows * 2.0 ** -24 * x.double().abs().sum(dim=0))[fin])
    tail = s.ws.get()[0, col_workspace_floats(c.rows, c.cols):]
    if not bool(torch.isnan(tail).all()):
        rep.fail(f"workspace: {int((~torch.isnan(tail)).sum())} of the {WS_BEHIND} floats behind its documented size were written")
    return rep.done()


def col_outputs(s):
    return [kr.ibits(t.get()) for t in (s.y, s.ra, s.yc, s.ce, s.ca, s.db)]


# ==================================================================================================== 4. LayerNorm with split output

LN_D = [4, 8, 72, 252, 256, 260, 384, 508, 516, 640, 764, 772, 896, 1020, 1028, 1280, 2044, 2048, 512, 768, 1024]
LN_ROWS = [1, 3, 4, 5, 9]
LN_SEXP = [0, 9, -3, 6]              # |LN(x)| stays below 2^5 for these data: nothing overflows fp16
LnCase = namedtuple("LnCase", "D rows sexp")
LN_ENTRIES = ("dev_side", "dev", "host")     # _dev with y32 / mean / rstd, _dev without them, the scalar entry


def ln_cases():
    return [LnCase(D, rows, LN_SEXP[(i + j) % 4]) for i, D in enumerate(LN_D) for j, rows in enumerate(LN_ROWS)]


def ln_variant(D: int) -> str:
    if D in (512, 768, 1024):
        return ".nc%d.exact" % (D // 256)
    nc = -(-(D // 4) // 64)
    return ".nc%d" % (max(nc, 1) if nc <= 4 else 8)


def ln_site(c, entry: str) -> str:
    return ("layernorm_fwd_f16x3" if entry == "host" else "layernorm_fwd_f16x3_dev") + ln_variant(c.D)


def build_ln(c: LnCase, device="cpu"):
    ln = kr.build_ln_fwd(kr.LnFwdCase(c.D, c.rows, True), device)          # x (NaN rows behind it), y32, mean, rstd: §18's buffers
    tail = torch.full((8,), NAN)
    ln.gd, ln.bd = torch.cat([ln.g, tail]).to(device), torch.cat([ln.b, tail]).to(device)
    return SimpleNamespace(case=c, ln=ln, scale=vec(1, device, fill=2.0 ** c.sexp),
                           y={k: Guarded(c.rows, 3 * c.D, device=device, dtype=HALF) for k in LN_ENTRIES})


def launch_ln(lib, s, stream, entry: str) -> int:
    c, ln = s.case, s.ln
    if entry == "host":
        return lib.dclip_layernorm_fwd_f16x3(ln.xd.data_ptr(), ln.gd.data_ptr(), ln.bd.data_ptr(), s.y[entry].ptr, c.rows, c.D, kr.LN_EPS,
                                             2.0 ** c.sexp, stream)
    side = entry == "dev_side"
    return lib.dclip_layernorm_fwd_f16x3_dev(ln.xd.data_ptr(), ln.gd.data_ptr(), ln.bd.data_ptr(), s.y[entry].ptr,
                                             ln.y.ptr if side else None, ln.mean.ptr if side else None, ln.rstd.ptr if side else None,
                                             c.rows, c.D, kr.LN_EPS, s.scale.ptr, stream)


def emulate_ln(s, fault=None):
    c, ln = s.case, s.ln
    kr.emulate_ln_fwd(ln)
    sc = 2.0 ** c.sexp
    y32 = ln.y.payload
    if fault == "one_rounding":                            # the split taken from the unrounded affine result
        o = ((ln.x - ln.mean.payload[0][:, None]) * ln.rstd.payload[0][:, None]).double() * ln.g.double() + ln.b.double()
        hi = (o * sc).float().half()
        lo = (o * sc - hi.double()).float().half()
    else:
        hi, lo = host_split(y32, sc)
    for k in LN_ENTRIES:
        s.y[k].payload.copy_(layout3(hi, lo, 0))
    if fault == "host_differs":
        s.y["host"].payload[c.rows - 1, c.D] = 0.5
    if fault == "y_behind":
        s.y["dev"].buf[s.y["dev"].guard + c.rows * 3 * c.D] = 0
    if fault == "chunk_unwritten" and c.D > 256:
        s.y["dev_side"].payload[:, 256:260] = NAN


def verify_ln(s, what=None):
    c, ln = s.case, s.ln
    kr.verify_ln_fwd(ln, f"layernorm_fwd_f16x3_dev y32/mean/rstd {c}")          # §18's checker on the fp32 side outputs
    rep = Report(what or f"layernorm_fwd_f16x3 {c}")
    rep.guards(scale=s.scale, **{"y_" + k: g for k, g in s.y.items()})
    sc = 2.0 ** c.sexp
    hi, lo = host_split(ln.y.get(), sc)
    got = s.y["dev_side"].get()
    check_pieces(rep, "y", got, layout3(hi, lo, 0))                              # EQUAL the host split of the RETURNED y32
    r = kr.ln_fwd_bounds(ln.x, ln.g, ln.b, c.D)
    for k in ("dev", "host"):
        g = s.y[k].get()
        rep.bits(f"y_{k} against the call with side outputs", g, got)
        back = (g[:, :c.D].double() + g[:, c.D:2 * c.D].double()) / sc
        if not torch.equal(kr.ibits(g[:, :c.D]), kr.ibits(g[:, 2 * c.D:])):
            rep.fail(f"y_{k}: the third piece is not the first")
        rep.bound(f"y_{k} (hi+lo)/scale", back, r.want, r.bnd + RECON_REL * r.want.abs() + RECON_ABS / sc)
    return rep.done()


# ==================================================================================================== 5. device plan

RECORD = struct.Struct("<QQ8i")       # src, dst, rows, cols, layer, max_slot, l1_slot, l1_row0, scale_slot, tile0 (include/dclip_hip.h)
RECORD_BYTES, PLAN_FLOATS, TILE_ROWS, NSTAT = 48, 32, 32, 12
Rec = namedtuple("Rec", "rows cols layer max_slot l1_slot l1_row0 dst dst_t scale_slot mag")
PLAN_D = 72
LAYER_FLAGS = {"clean": 0, "bound": 1, "nonfinite": 2, "tiny_weight": 4, "huge_ctx": 5}


def layer_records(layer: int, kind: str):
    """The ten tensors of a layer (statistics-only vectors between the matrices), sizes at the tile edges: rows 8, 32, 40, 72 and
    cols 8, 64, 72, 136; `mag` is the power of two its dyadic data are scaled by."""
    m = {k: 0 for k in ("ln1_w", "ln1_b", "qkv", "v_b", "out", "ln2_w", "ln2_b", "fc1", "fc1_b", "fc2")}
    if kind == "bound":
        m["ln1_w"] = 30                                    # LayerNorm bound 2^33 sqrt(D): e < -14
    if kind == "tiny_weight":
        m["fc2"] = -124                                    # max|W| = 2^-120: f = 133 > 127
    if kind == "huge_ctx":
        m["ln1_w"], m["qkv"] = 76, 60                      # b_ln1 ~ 2^83, row L1 ~ 2^70: the ctx bound is beyond 2^140
    R = lambda name, rows, cols, slot, **kw: Rec(rows, cols, layer, slot, kw.get("l1", -1), kw.get("row0", 0), kw.get("dst", False),
                                                 kw.get("t", False), kw.get("scale", -1), m[name])
    return [R("ln1_w", 1, 8, 0), R("ln1_b", 1, 64, 1),
            R("qkv", 72, 72, 8, l1=2, row0=40, dst=True, t=True, scale=4), R("v_b", 1, 8, 3),
            R("out", 40, 136, 9, dst=True, t=False, scale=5), R("ln2_w", 1, 8, 4), R("ln2_b", 1, 72, 5),
            R("fc1", 32, 64, 10, l1=6, row0=0, dst=True, t=True, scale=6), R("fc1_b", 1, 136, 7),
            R("fc2", 8, 8, 11, dst=True, t=True, scale=7)]


PlanCase = namedtuple("PlanCase", "name kinds transposed")
# transposed: True / False = dclip_split16_weights_t / _weights; "null" = _weights_t with every entry of dst_t NULL
PLAN_CASES = [PlanCase("one", None, True), PlanCase("one", None, False), PlanCase("clean", ("clean",), True),
              PlanCase("five", tuple(LAYER_FLAGS), True), PlanCase("five", tuple(LAYER_FLAGS), False),
              PlanCase("five", tuple(LAYER_FLAGS), "null")]


def plan_records(c: PlanCase):
    if c.kinds is None:
        return [Rec(40, 72, 0, 9, -1, 0, True, c.transposed, 5, 0)]
    return [r for li, kind in enumerate(c.kinds) for r in layer_records(li, kind)]


def plan_id(c) -> str:
    return f"{c.name}-{ {True: 'weights_t', False: 'weights', 'null': 'weights_t_all_null'}[c.transposed]}"


def tiles_of(r) -> int:
    return -(-r.rows // TILE_ROWS)


def record_data(r: Rec, seed: int, kind: str) -> torch.Tensor:
    """Dyadic: integers in [-8, 8] times 2^mag, so every row L1 sum is exact in fp32; rows below l1_row0 are doubled (an L1
    statistic over all rows would be too large)."""
    x = torch.randint(-8, 9, (r.rows, r.cols), generator=gen(seed)).float()
    x[r.rows // 2, r.cols - 1] = 8.0
    if r.l1_row0 > 0:
        x[:r.l1_row0] *= 2.0
    x = x * 2.0 ** r.mag
    if kind == "nonfinite" and r.max_slot == 10:
        x[0, 1], x[r.rows - 1, 3] = INF, NAN
    return x


def build_plan(c: PlanCase, device="cpu"):
    recs = plan_records(c)
    kinds = c.kinds or ("clean",)
    src = [record_data(r, 100 * i + 7, kinds[r.layer]) for i, r in enumerate(recs)]
    s = SimpleNamespace(case=c, recs=recs, src=src, nlayers=len(kinds), kinds=kinds,
                        srcd=[poisoned(x, r.cols, device) for x, r in zip(src, recs)],
                        srcd_first=[poisoned(x * 4.0, r.cols, device) for x, r in zip(src, recs)],      # the first call's larger weights
                        dst=[Guarded(r.rows, 3 * r.cols, device=device, dtype=HALF) if r.dst else None for r in recs],
                        dst_t=[Guarded(r.cols, 3 * r.rows, device=device, dtype=HALF) if r.dst and r.dst_t and c.transposed is True else None
                               for r in recs],
                        stats=vec(len(kinds) * NSTAT, device, fill=0.0), plan=vec(len(kinds) * PLAN_FLOATS, device))
    s.tile0 = [sum(tiles_of(q) for q in recs[:i]) for i in range(len(recs))]
    s.tiles = sum(tiles_of(r) for r in recs)
    return s


def pack_table(s, srcs, device):
    raw = b"".join(RECORD.pack(x.data_ptr(), d.ptr if d is not None else 0, r.rows, r.cols, r.layer, r.max_slot, r.l1_slot, r.l1_row0,
                               r.scale_slot, t0) for x, d, r, t0 in zip(srcs, s.dst, s.recs, s.tile0))
    assert len(raw) == RECORD_BYTES * len(s.recs)
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)


def exact_stats(s, scale=1.0, fault=None):
    """[layers][12] fp64: the exact maxima (all sums exact by construction)."""
    st = torch.zeros((s.nlayers, NSTAT), dtype=torch.float64)

    def fmax(a, b):                                        # the integer maximum of the bit patterns: NaN above inf above the rest
        return b if (math.isnan(b) or (not math.isnan(a) and b > a)) else a
    for x, r in zip(s.src, s.recs):
        a = (x.double() * scale).abs()
        mx = NAN if bool(torch.isnan(a).any()) else float(a.max())
        st[r.layer, r.max_slot] = fmax(float(st[r.layer, r.max_slot]), mx)
        if r.l1_slot >= 0:
            rows = a if fault == "l1_all_rows" else a[r.l1_row0:]
            sums = rows.sum(dim=1)
            l1 = NAN if bool(torch.isnan(sums).any()) else float(sums.max())
            st[r.layer, r.l1_slot] = fmax(float(st[r.layer, r.l1_slot]), l1)
    return st


def clamp_exp(e: int) -> int:
    return max(-126, min(127, e))


def plan_rule(st, D: int, fault=None):
    """One layer's 32 plan floats from its 12 statistics (Python floats = fp64, every product and sum rounded on its own):
    bounds ln = max|gamma| sqrt(D) + max|beta|, ctx = ln1 L1(W_v) + max|b_v|, g = ln2 L1(W_fc1) + max|b_fc1|; an activation
    exponent is the largest e <= 24 with bound 2^e <= 2^14 (flag 1 when e < -14; flag 2 and e = 0 for a non-finite bound), a
    weight exponent f has max|W| 2^f in [2^13, 2^14) (0 for 0; flag 2 and 0 when not finite); flag 4 when a scale or an alpha
    had to be clamped to fp32's normal range."""
    flags = 0
    sq = math.sqrt(float(D))
    ln1, ln2 = st[0] * sq + st[1], st[4] * sq + st[5]
    bounds = [ln1, ln1 * st[2] + st[3], ln2, ln2 * st[6] + st[7]]
    e, f = [], []
    for b in bounds:
        if not math.isfinite(b) or b < 0.0:
            flags |= 2
            e.append(0)
        elif b == 0.0:
            e.append(24)
        else:
            m, x = math.frexp(b)
            v = TOP - (x - 1 if m == 0.5 else x)
            if v < -14:
                flags |= 1
            e.append(min(v, 24))
    for w in st[8:12]:
        if not math.isfinite(w):
            flags |= 2
            f.append(0)
        else:
            f.append(0 if w == 0.0 else TOP - math.frexp(w)[1])
    rec = [0.0] * PLAN_FLOATS
    for i in range(4):
        if e[i] < -126:
            e[i], flags = -126, flags | (0 if fault == "no_flag4" else 4)
        if f[i] > 127:
            f[i], flags = 127, flags | (0 if fault == "no_flag4" else 4)
        if not -126 <= -(e[i] + f[i]) <= 127:
            flags |= 0 if fault == "no_flag4" else 4
        rec[i], rec[4 + i], rec[8 + i] = 2.0 ** e[i], 2.0 ** f[i], 2.0 ** clamp_exp(-(e[i] + f[i]))
        rec[28 + i] = 2.0 ** clamp_exp(-f[i])
    rec[16:28] = list(st)
    return rec, flags


def plan_expect(s, fault=None, stats=None):
    st = exact_stats(s) if stats is None else stats
    plan = torch.zeros((s.nlayers, PLAN_FLOATS), dtype=torch.float32)
    flags = []
    for l in range(s.nlayers):
        rec, fl = plan_rule(st[l].tolist(), PLAN_D, fault)
        plan[l] = torch.tensor(rec, dtype=torch.float64).float()
        plan[l, 12] = torch.tensor([fl], dtype=torch.int32).view(torch.float32)[0]
        flags.append(fl)
    return plan, flags


def launch_plan(lib, s, stream, device, names=None):
    """Two rounds: statistics and plan of LARGER weights first (the accumulators are non-zero while that plan launch clears
    them), then statistics, plan and the weight copies of the case's weights.  Returns the first non-zero return code."""
    def note(want):
        if names is not None:
            names.append((want, lib.dclip_last_launch().decode()))
    n = len(s.recs)
    s.table_first, s.table = pack_table(s, s.srcd_first, device), pack_table(s, s.srcd, device)
    for tab in (s.table_first, s.table):
        rc = lib.dclip_split16_stats(tab.data_ptr(), n, s.tiles, s.stats.ptr, stream)
        note("split16_stats")
        rc = rc or lib.dclip_split16_plan(s.stats.ptr, s.plan.ptr, s.nlayers, PLAN_D, stream)
        note("split16_plan")
        if rc:
            return rc
    if s.case.transposed:
        s.ptrs = torch.tensor([d.ptr if d is not None else 0 for d in s.dst_t], dtype=torch.int64, device=device)
        rc = lib.dclip_split16_weights_t(s.table.data_ptr(), n, s.tiles, s.plan.ptr, s.ptrs.data_ptr(), stream)
        note("split16_weights.t")
    else:
        rc = lib.dclip_split16_weights(s.table.data_ptr(), n, s.tiles, s.plan.ptr, stream)
        note("split16_weights")
    return rc


def emulate_plan(s, fault=None):
    first = exact_stats(s, 4.0)
    st = exact_stats(s, 1.0, fault)
    if fault == "stats_not_cleared":                       # the second round's maxima start from the first round's
        st = torch.where(torch.isnan(first) | (first > st), first, st)
        s.stats.payload.copy_(st.float().view(1, -1))
    else:
        s.stats.payload.zero_()
    plan, _ = plan_expect(s, fault, st)
    s.plan.payload.copy_(plan.view(1, -1))
    for x, r, d, dt in zip(s.src, s.recs, s.dst, s.dst_t):
        if d is None:
            continue
        hi, lo = host_split(x, float(plan[r.layer, r.scale_slot]))
        d.payload.copy_(layout3(hi, lo, 1))
        if dt is not None:
            t = layout3(hi.t().contiguous(), lo.t().contiguous(), 1)
            dt.payload.copy_(t)
            if fault == "t_last_group":
                for k in range(3):
                    dt.payload[:, k * r.rows + r.rows - 8:(k + 1) * r.rows] = NAN
    if fault == "dst_behind":
        d = next(d for d in s.dst if d is not None)
        d.buf[d.guard + d.rows * d.ld] = 0
    if fault == "plan_behind":
        s.plan.buf[s.plan.guard + s.nlayers * PLAN_FLOATS] = 0


def verify_plan(s, what=None):
    rep = Report(what or f"split16 plan {plan_id(s.case)}")
    rep.guards(stats=s.stats, plan=s.plan, **{f"dst{i}": d for i, d in enumerate(s.dst)}, **{f"dst_t{i}": d for i, d in enumerate(s.dst_t)})
    if bool((kr.ibits(s.stats.get()) != 0).any()):
        rep.fail("stats: the accumulators are not zero after the plan launch")
    want, flags = plan_expect(s)
    assert flags == [LAYER_FLAGS[k] for k in s.kinds], (flags, s.kinds)          # the crafted layers raise the flags they are named for
    got = s.plan.get().view(s.nlayers, PLAN_FLOATS)
    stat_nan = torch.isnan(want[:, 16:28])
    if not torch.equal(torch.isnan(got[:, 16:28]), stat_nan):
        rep.fail("plan: NaN statistics in other slots than the exact maxima")
    g, w = got.clone(), want.clone()
    g[:, 16:28][stat_nan], w[:, 16:28][stat_nan] = 0.0, 0.0                      # a NaN need only be a NaN
    rep.bits("plan", g, w)
    for i, (x, r, d, dt) in enumerate(zip(s.src, s.recs, s.dst, s.dst_t)):
        if d is None:
            continue
        hi, lo = host_split(x, float(want[r.layer, r.scale_slot]))
        check_pieces(rep, f"dst{i}", d.get(), layout3(hi, lo, 1))
        check_recon(rep, f"dst{i} hi+lo", d.get()[:, :r.cols], d.get()[:, 2 * r.cols:], x.double() * float(want[r.layer, r.scale_slot]))
        if dt is not None:                                 # the host split of the TRANSPOSED scaled weight
            ht, lt = host_split(x.t().contiguous(), float(want[r.layer, r.scale_slot]))
            check_pieces(rep, f"dst_t{i}", dt.get(), layout3(ht, lt, 1))
    return rep.done()


# ==================================================================================================== 7. segmented weight gradient

SEG_SIZES, SEG_TOKENS, SEG_SPLITS = [8, 264, 520], [64, 192, 320], [1, 2, 3, 7, 21]
SEG_ACT_EXP = 7
SegCase = namedtuple("SegCase", "M N tokens splits perm")
SEG_SITE = "gemm_f16_wgrad_tokmajor_seg3.pp_tok_seg.splitk_reduce"


def seg_cases():
    """Every (tokens, splits) pair on three of the nine (M, N), rotating: every (M, N) meets every token count and every split
    count, with both sets of segments."""
    out = []
    sizes = [(m, n) for m in SEG_SIZES for n in SEG_SIZES]
    for i, tokens in enumerate(SEG_TOKENS):
        for k, splits in enumerate(SEG_SPLITS):
            for j in range(3):
                M, N = sizes[(3 * k + j + 3 * i) % 9]
                out.append(SegCase(M, N, tokens, splits, bool((i + k + j) % 2)))
    return out


def seg_id(c) -> str:
    return f"{c.M}x{c.N}-tok{c.tokens}-s{c.splits}-{'perm' if c.perm else 'step'}"


def seg_s_eff(tokens: int, splits: int):
    """(tokens per split, splits that get any): a split takes whole K-tiles of 64 tokens."""
    kps = roundup(-(-tokens // splits), 64)
    return kps, -(-tokens // kps)


def seg_offsets(c):
    """(a_seg, w_seg): the step's segments — dY = [hi|lo] with X = [hi|lo|hi]: hi.hi + lo.hi + hi.lo — or a permuted set."""
    return ((c.M, 0, c.M), (2 * c.N, c.N, 0)) if c.perm else ((0, c.M, 0), (0, 0, c.N))


def build_seg(c: SegCase, device="cpu"):
    seed = 1000 * c.M + 10 * c.N + c.tokens + c.splits
    lddy, ldx = 2 * c.M + 8, 3 * c.N + 16
    dy, x = kr.ints((c.tokens, 2 * c.M), seed), kr.ints((c.tokens, 3 * c.N), seed + 1)
    a_seg, w_seg = seg_offsets(c)
    for t, segs, width in ((dy, a_seg, c.M), (x, w_seg, c.N)):       # columns outside every segment are NaN
        used = torch.zeros(t.shape[1], dtype=torch.bool)
        for o in segs:
            used[o:o + width] = True
        t[:, ~used] = NAN
    ca = torch.exp2(((torch.arange(c.M) * 7) % 41 - 20).float())     # distinct powers of two over any 41 consecutive rows
    _, s_eff = seg_s_eff(c.tokens, c.splits)
    floats = 3 * s_eff * c.M * c.N
    return SimpleNamespace(case=c, dy=dy, x=x, ca=ca, a_seg=a_seg, w_seg=w_seg, s_eff=s_eff, lddy=lddy, ldx=ldx,
                           dyd=poisoned(dy, lddy, device, dtype=HALF), xd=poisoned(x, ldx, device, dtype=HALF),
                           cad=vec(c.M, device, fill=ca[None]), act=vec(1, device, fill=2.0 ** SEG_ACT_EXP),
                           C=Guarded(c.M, c.N, c.N + 4, device=device), ws=vec(floats + kr.WS_TAIL, device), ws_bytes=4 * floats)


def launch_seg(lib, s, stream, ws_bytes=None) -> int:
    c = s.case
    return lib.dclip_gemm_f16_wgrad_tokmajor_seg3(s.dyd.data_ptr(), s.xd.data_ptr(), s.C.ptr, c.M, c.N, c.tokens, s.lddy, s.ldx, s.C.ld,
                                                  *s.a_seg, *s.w_seg, s.cad.ptr, s.act.ptr, c.splits, s.ws.ptr,
                                                  s.ws_bytes if ws_bytes is None else ws_bytes, stream)


def emulate_seg(s, fault=None):
    """3 s_eff fp32 slabs (segment, split), then their sum in order, divided by the activation scale, times col_alpha."""
    c = s.case
    kps, s_eff = seg_s_eff(c.tokens, c.splits)
    slabs = s.ws.payload[0, :3 * s_eff * c.M * c.N].view(3 * s_eff, c.M, c.N)
    for g in range(3):
        src = 0 if (fault == "seg_twice" and g == 2) else g
        a = s.dy[:, s.a_seg[src]:s.a_seg[src] + c.M]
        w = s.x[:, s.w_seg[src]:s.w_seg[src] + c.N]
        for k in range(s_eff):
            slabs[g * s_eff + k] = a[k * kps:(k + 1) * kps].t() @ w[k * kps:(k + 1) * kps]
    acc = torch.zeros((c.M, c.N))
    for k in range(3 * s_eff - (1 if fault == "slab_left_out" else 0)):
        acc = acc + slabs[k]
    s.C.payload.copy_((acc * 2.0 ** -SEG_ACT_EXP) * s.ca[:, None])
    if fault == "slab_unwritten":
        slabs[3 * s_eff - 1, c.M - 1, c.N - 1] = NAN
    if fault == "ws_behind":
        s.ws.payload[0, 3 * s_eff * c.M * c.N] = 0.0
    if fault == "c_pad":
        s.C.mat[0, c.N] = 0.0


def verify_seg(s, what=None):
    c = s.case
    rep = Report(what or f"wgrad_tokmajor_seg3 {seg_id(c)}")
    rep.guards(C=s.C, workspace=s.ws, col_alpha=s.cad, act_scale=s.act)
    acc = torch.zeros((c.M, c.N), dtype=torch.float64)
    for g in range(3):
        a = s.dy[:, s.a_seg[g]:s.a_seg[g] + c.M].double()
        w = s.x[:, s.w_seg[g]:s.w_seg[g] + c.N].double()
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(w).all())
        acc += a.t() @ w
    want = acc * 2.0 ** -SEG_ACT_EXP * s.ca.double()[:, None]
    assert torch.equal(want.float().double(), want)                # every expected value is exactly representable in fp32
    rep.exact("C", s.C.get(), want)
    ws = s.ws.get()[0]
    used = 3 * s.s_eff * c.M * c.N
    if bool(torch.isnan(ws[:used]).any()):
        rep.fail(f"workspace: {int(torch.isnan(ws[:used]).sum())} words of the {3 * s.s_eff} slabs were never written")
    if not bool(torch.isnan(ws[used:]).all()):
        rep.fail(f"workspace: wrote behind its documented size ({int((~torch.isnan(ws[used:])).sum())} of {kr.WS_TAIL} floats)")
    return rep.done()


# ==================================================================================================== 6. scaled GEMM entries

# §17's integer-exact checker on the five scaled entries, on every kernel they can take: A, W integers in [-2, 2], alpha a power
# of two (scalar or a guarded device float), row_alpha[m] = 2^((m mod 13) - 6), bias multiples of 2^-12 in [-1, 1], residual
# integers: every expected linear value is exact in fp32.  GELU / DGELU: §17's tolerance 1e-5 |want| + 2^-126 (1 + factor)
# against fp64 of the exact pre-activation.
EPI_BIAS, EPI_GELU, EPI_DGELU, EPI_RESIDUAL = 1, 2, 4, 8
F32_FLOOR = 2.0 ** -126
#         entry               fn           epilogue                   what else
_E = lambda fn, epi, **kw: dict(fn=fn, epi=epi, **kw)
GEMM_FORMS = {
    "scaled": _E("scaled", EPI_BIAS | EPI_RESIDUAL),
    "scaled_dev": _E("scaled_dev", EPI_BIAS | EPI_RESIDUAL),
    "rows_dev": _E("rows_dev", 0),
    "rows_dgelu": _E("rows_dev", EPI_DGELU),
    "rows_big": _E("rows_dev", 0, big=True),                                  # row_alpha 2^100 / 2^-60 beside accumulators >= 2^25
    "split": _E("split", EPI_BIAS, split=True),
    "split_gelu": _E("split", EPI_BIAS | EPI_GELU, split=True),
    "split_negzero": _E("split", EPI_BIAS, split=True, negzero=True),         # four columns whose exact result is -0
    "split_dev": _E("split_dev", EPI_BIAS, split=True),
    "split_dev_g32": _E("split_dev", EPI_BIAS, split=True, g32=True),
    "split_dev_noscale": _E("split_dev", EPI_BIAS, noscale=True),
    "split_dev_gelu": _E("split_dev", EPI_BIAS | EPI_GELU, split=True),
    "split_dev_gelu_h": _E("split_dev", EPI_BIAS | EPI_GELU, split=True, h32=True),
    "split_dev_gelu_g": _E("split_dev", EPI_BIAS | EPI_GELU, split=True, g32=True),
    "split_dev_gelu_hg": _E("split_dev", EPI_BIAS | EPI_GELU, split=True, h32=True, g32=True),
    "split_dev_noscale_gelu_h": _E("split_dev", EPI_BIAS | EPI_GELU, noscale=True, h32=True),
}
GEMM_ENTRIES = tuple(GEMM_FORMS)
GEMM_NAMES = {"scaled": "gemm_f16_scaled", "scaled_dev": "gemm_f16_scaled_dev", "rows_dev": "gemm_f16_scaled_rows_dev",
              "split": "gemm_f16_scaled_split", "split_dev": "gemm_f16_scaled_split_dev"}
ENV_PERSIST = {"DCLIP_BF16_BIG_MIN": "1", "DCLIP_BF16_PERSIST": "1", "DCLIP_BF16_PERSIST_MIN": "1"}
# kernel -> (shapes, per-call switches, the variant reported)
GEMM_KERNELS = {"r64": ([(130, 72, 40), (65, 68, 72), (63, 260, 192)], {}, "r64"),
                "r128": ([(2047, 2044, 72)], {}, "r128"),                     # K % 64 != 0 keeps it off the ping-pong kernel
                "pp": ([(257, 260, 64), (300, 264, 128), (511, 520, 192)], {"DCLIP_BF16_BIG_MIN": "1"}, "pp"),
                "pp_persist": ([(257, 260, 64)], ENV_PERSIST, "pp"),          # every entry but gemm_f16_scaled stays on .pp
                "ppp": ([(200, 256, 64), (1789, 248, 64), (600, 520, 64)], ENV_PERSIST, "ppp")}      # 1, 7 and 9 tiles
GEMM_SWITCHES = ("DCLIP_BF16_BIG_MIN", "DCLIP_BF16_PERSIST", "DCLIP_BF16_PERSIST_MIN")
GEMM_ALPHA_EXP, GEMM_OUT_EXP, GEMM_BIG_ALPHA_EXP = -3, 4, -24
ScaledCase = namedtuple("ScaledCase", "entry kernel M N K cpad")


def scaled_cases():
    out = []
    for k, (shapes, _, _) in GEMM_KERNELS.items():
        for i, shape in enumerate(shapes):
            for j, e in enumerate(GEMM_ENTRIES):
                if (k == "ppp") != (e == "scaled") and k in ("ppp", "pp_persist"):
                    continue
                out.append(ScaledCase(e, k, *shape, 1 if e == "rows_dgelu" else (i + j) % 2))       # aux32 always has ldc > N
    return out


def scaled_id(c) -> str:
    return f"{c.entry}-{c.kernel}-{c.M}x{c.N}x{c.K}-pad{c.cpad}"


def scaled_env(c) -> dict:
    return GEMM_KERNELS[c.kernel][1]


def scaled_site(c) -> str:
    return f"{GEMM_NAMES[GEMM_FORMS[c.entry]['fn']]}.{GEMM_KERNELS[c.kernel][2]}"


def scaled_form(c):
    f = dict(split=False, g32=False, h32=False, noscale=False, big=False, negzero=False)
    f.update(GEMM_FORMS[c.entry])
    return SimpleNamespace(**f)


def scaled_is_split(c) -> bool:
    return scaled_form(c).split


def build_scaled(c: ScaledCase, device="cpu"):
    f = scaled_form(c)
    seed = 1000 * c.M + 10 * c.N + c.K
    a, w = kr.ints((c.M, c.K), seed), kr.ints((c.N, c.K), seed + 1)
    bias = torch.randint(-4096, 4097, (c.N,), generator=gen(seed + 2)).float() * 2.0 ** -12
    ra = torch.exp2((torch.arange(c.M) % 13 - 6).float())
    alpha = 2.0 ** GEMM_ALPHA_EXP
    if f.big:
        a = torch.randint(0, 2, (c.M, c.K), generator=gen(seed)).float() * 8192.0 + 8192.0
        w = torch.randint(0, 2, (c.N, c.K), generator=gen(seed + 1)).float() * 4096.0 + 4096.0      # sums of multiples of 2^25: exact
        ra = torch.where(torch.arange(c.M) % 2 == 0, 2.0 ** 100, 2.0 ** -60).float()
        alpha = 2.0 ** GEMM_BIG_ALPHA_EXP
        assert float((a.double() @ w.double().t()).min()) >= 2.0 ** 29          # times 2^100 first, it would overflow
    if f.negzero:
        alpha = -alpha
        w[:4] = 0.0
        bias[:4] = -0.0
    lda = ldw = roundup(c.K, 8) + 8
    rows = f.fn == "rows_dev"
    ldc = roundup(3 * c.N, 8) + 8 * c.cpad if f.split else c.N + 4 * c.cpad
    if f.noscale or c.kernel == "ppp":                     # ldc % 8 == 0 is asked for there also with an fp32 C
        ldc = roundup(c.N, 8) + 8 * c.cpad
    res = kr.ints((c.M, c.N), seed + 3)
    lin = (a.double() @ w.double().t()) * alpha
    if rows:
        lin = lin * ra.double()[:, None]
    if f.epi & EPI_BIAS:
        lin = lin + bias.double()
    if f.epi & EPI_RESIDUAL:
        lin = lin + res.double()
    assert torch.equal(lin.float().double(), lin)                  # every expected linear value is exactly representable in fp32
    if f.negzero:
        assert bool((torch.signbit(lin[:, :4]) & (lin[:, :4] == 0)).all())
    # aux32: multiples of 1/2 in [-4, 4].  §17's tolerance is relative to |want|, and GELU' has a zero near -0.7517 where an fp32
    # evaluation (absolute error of a few 2^-24) cannot meet 1e-5 relative; on this grid |GELU'| >= 0.0064
    aux = torch.randint(-8, 9, (c.M, c.N), generator=gen(seed + 4)).float() * 0.5 if f.epi & EPI_DGELU else None
    s = SimpleNamespace(case=c, form=f, a=a, w=w, bias=bias, res=res, ra=ra, lin=lin, want=lin, epi=f.epi, lda=lda, ldw=ldw, ldc=ldc,
                        alpha_v=alpha, aux=aux,
                        A=poisoned(a, lda, device, dtype=HALF), W=poisoned(w, ldw, device, dtype=HALF),
                        bias_d=torch.cat([bias, torch.full((8,), NAN)]).to(device),
                        res_d=poisoned(res, ldc, device) if f.epi & EPI_RESIDUAL else None,
                        aux_d=poisoned(aux, ldc, device) if aux is not None else None,     # NaN in its padding and behind row M
                        ra_d=vec(c.M, device, fill=ra[None]), alpha=vec(1, device, fill=alpha),
                        out_scale=vec(1, device, fill=2.0 ** GEMM_OUT_EXP),
                        C=Guarded(c.M, 3 * c.N if f.split else c.N, ldc, device=device, dtype=HALF if f.split else torch.float32),
                        g32=Guarded(c.M, c.N, device=device) if f.g32 else None,
                        h32=Guarded(c.M, c.N, device=device) if f.h32 else None)
    if f.split:
        final = kc_quick_gelu64(lin).float() if f.epi & EPI_GELU else lin.float()
        _, lo = host_split(final, 2.0 ** GEMM_OUT_EXP)
        assert float((lo.float() != 0).float().mean()) >= 0.25, "too few non-zero lo words for a dropped lo to show"
    return s


def launch_scaled(lib, s, stream, epi=None, alpha=None, h32=False, g32=False, out_scale=False) -> int:
    """The entry of the case; the keyword arguments override one argument each (the refusals)."""
    c, f = s.case, s.form
    A, W, C, b = s.A.data_ptr(), s.W.data_ptr(), s.C.ptr, s.bias_d.data_ptr()
    r = None if s.res_d is None else s.res_d.data_ptr()
    dims = (c.M, c.N, c.K, s.lda, s.ldw, s.ldc)
    epi = f.epi if epi is None else epi
    al = s.alpha_v if alpha is None else alpha
    if f.fn == "scaled":
        return lib.dclip_gemm_f16_scaled(A, W, C, b, r, *dims, epi, 0, al, stream)
    if f.fn == "scaled_dev":
        return lib.dclip_gemm_f16_scaled_dev(A, W, C, b, r, *dims, epi, 0, s.alpha.ptr, stream)
    if f.fn == "rows_dev":
        return lib.dclip_gemm_f16_scaled_rows_dev(A, W, C, None if s.aux_d is None else s.aux_d.data_ptr(), *dims, epi, s.alpha.ptr,
                                                  s.ra_d.ptr, stream)
    if f.fn == "split":
        return lib.dclip_gemm_f16_scaled_split(A, W, C, b, *dims, epi, al, 2.0 ** GEMM_OUT_EXP, stream)
    hp = s.h32.ptr if s.h32 is not None else (h32 or None)
    gp = s.g32.ptr if s.g32 is not None else (g32 or None)
    op = None if (f.noscale or out_scale is None) else s.out_scale.ptr
    return lib.dclip_gemm_f16_scaled_split_dev(A, W, C, b, hp, gp, *dims, epi, s.alpha.ptr, op, stream)


def kc_quick_gelu64(x):
    x = x.double()
    return x / (1.0 + torch.exp(-1.702 * x))


def kc_quick_gelu_grad64(x):
    x = x.double()
    sg = 1.0 / (1.0 + torch.exp(-1.702 * x))
    return sg * (1.0 + 1.702 * x * (1.0 - sg))


def _dense_with_stride(g: Guarded, v, ld):
    """(a planted fault) the first rows of a dense [M][N] side output written with the stride of C."""
    flat = g.buf[g.guard:].view(torch.float32)
    for m in range(min(v.shape[0], 3)):
        flat[m * ld:m * ld + v.shape[1]] = v[m]


def emulate_scaled(s, fault=None):
    c, f = s.case, s.form
    acc = s.a @ s.w.t()
    al = torch.tensor(s.alpha_v)
    ra = s.ra
    if fault == "row_alpha_next":                          # the last tile of rows takes row + 1 (clamped)
        ra = torch.cat([s.ra[:-64], s.ra[-63:], s.ra[-1:]]) if c.M > 64 else torch.cat([s.ra[1:], s.ra[-1:]])
    v = acc if fault == "alpha_after_bias" else acc * al
    if f.fn == "rows_dev":
        v = (acc * ra[:, None]) * al if fault == "row_alpha_first" else v * ra[:, None]
    if s.epi & EPI_BIAS:
        v = v + s.bias
    if fault == "alpha_after_bias":
        v = v * al
    if s.epi & EPI_RESIDUAL:
        v = v + s.res
    h = v
    if s.epi & EPI_GELU:
        v = h / (1.0 + torch.exp(-1.702 * h))
    if s.epi & EPI_DGELU:
        aux = torch.cat([s.aux[1:], s.aux[-1:]]) if fault == "aux_row_next" else s.aux
        sg = 1.0 / (1.0 + torch.exp(-1.702 * aux))
        v = v * (sg * (1.0 + 1.702 * aux * (1.0 - sg)))
    if s.h32 is not None:
        s.h32.payload.copy_(v if fault == "h32_is_g" else h)
        if fault == "h32_stride_ldc":
            _dense_with_stride(s.h32, h, s.ldc)
    if s.g32 is not None:
        s.g32.payload.copy_(v)
        if fault == "g32_stride_ldc":
            _dense_with_stride(s.g32, v, s.ldc)
    if f.split:
        hi, lo = host_split(v, 2.0 ** GEMM_OUT_EXP)
        if fault == "lo_dropped":
            lo = torch.zeros_like(lo)
        if fault == "lo_negzero":
            lo = torch.where(torch.signbit(v) & (v == 0), torch.tensor(-0.0, dtype=HALF), lo)
        s.C.payload.copy_(layout3(hi, lo, 0))
        if fault == "third_piece_off":                     # the third piece at 2N + 8
            s.C.mat[:, 2 * c.N:2 * c.N + 8] = NAN
            s.C.mat[:, 2 * c.N + 8:3 * c.N + 8] = hi
    else:
        s.C.payload.copy_(v)


def verify_scaled(s, what=None):
    c, f = s.case, s.form
    rep = Report(what or scaled_id(c))
    rep.guards(C=s.C, g32=s.g32, h32=s.h32, alpha=s.alpha, out_scale=s.out_scale, row_alpha=s.ra_d)
    lin, N, os_ = s.lin, c.N, 2.0 ** GEMM_OUT_EXP
    got = s.C.get()
    want, tol = lin, None
    if s.epi & EPI_GELU:
        want = kc_quick_gelu64(lin)
        tol = 1e-5 * want.abs() + F32_FLOOR * (1.0 + lin.abs())
    if s.epi & EPI_DGELU:
        want = lin * kc_quick_gelu_grad64(s.aux)
        tol = 1e-5 * want.abs() + F32_FLOOR * (1.0 + lin.abs() * (1.0 + 1.702 * s.aux.double().abs()))
    if s.h32 is not None:
        rep.exact("h32", s.h32.get(), lin)                 # the exact pre-activation
    g32 = None
    if s.g32 is not None:
        g32 = s.g32.get()
        if tol is None:
            rep.exact("g32", g32, want)
        else:
            rep.bound("g32", g32, want, tol)
    if not f.split:
        if tol is None:
            rep.exact("C", got, want)
        else:
            rep.bound("C", got, want, tol)
        return rep.done()
    if not torch.equal(kr.ibits(got[:, :N]), kr.ibits(got[:, 2 * N:])):
        rep.fail("C: the third piece is not the first")
    hi, lo = got[:, :N], got[:, N:2 * N]
    if tol is None:
        whi, wlo = host_split(want.float(), os_)
        check_pieces(rep, "C", got, layout3(whi, wlo, 0))
        check_recon(rep, "C hi+lo", hi, lo, want * os_)
    elif g32 is not None:                                  # EQUAL the host split of the RETURNED g32
        whi, wlo = host_split(g32, os_)
        check_pieces(rep, "C", got, layout3(whi, wlo, 0))
        check_recon(rep, "C hi+lo", hi, lo, g32.double() * os_)
    else:                                                  # no fp32 result to split: the reconstruction bound around the tolerance
        rep.bound("C (hi+lo)/out_scale", (hi.double() + lo.double()) / os_, want, tol + RECON_REL * want.abs() + RECON_ABS / os_)
    return rep.done()
