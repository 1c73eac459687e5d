"""TEST-ONLY checkers for the fp32 GEMM and attention kernel paths (tests/test_gemm_paths_gpu.py,
tests/test_attention_paths_gpu.py, tests/test_teacher_ops_gpu.py) and the case lists those tests run.

Nothing here imports the product or needs a GPU: a case is built on any torch device, handed to a `launch` function (the C
ABI on the GPU, a plain fp32 torch evaluation in tests/test_kernel_checks_cpu.py) and then verified.  The CPU self-test
runs every case through the fp32 evaluation (the checkers pass on a correct result) and plants one fault at a time (they
fail on a subtly wrong one).

What the checkers are:
  * integer-exact GEMM: operands, bias, residual and the initial C are integers in [-2, 2] and alpha is a power of two, so
    every product and every partial sum, in any order, is an integer below 2^24 (4 K <= 51,200 for K <= 12,800): the fp32
    result is exact whatever the tile, split or summation order, and the check is equality with an int64 matmul.
  * guarded buffers: every output lives inside one larger allocation pre-filled with a sentinel bit pattern — a band of
    at least 128 rows before and after, and every leading-dimension padding column — which must be intact afterwards
    (compared as int32).  The payload starts as NaN, so an element a kernel never writes cannot pass as a stale value.
  * poisoned inputs: operand padding (columns K..lda, rows past the operand) is NaN; a kernel that reads padding and
    multiplies by zero instead of selecting shows up as NaN.
  * derived rounding bound (Gaussian operands): |got - want| <= (K + 8) 2^-24 (|A| |B|)_ij per element — the gamma_K bound
    of an fp32 dot product in any order plus a few roundings for alpha, bias, residual and the split-K combine.
  * block-wise error: max|got - want| / max|want| separately for out, lse, dq, dk, dv; a block whose fp64 reference is
    identically zero must be identically zero.
"""
from __future__ import annotations

import ctypes
import functools
import json
import os
from collections import namedtuple
from types import SimpleNamespace

import torch

NAN = float("nan")
SENTINEL = 0x7FC5A5A5            # a NaN with a payload: anything computed from a guard word is NaN too
GUARD_ROWS = 128                 # one full tile of rows

A_KMAJOR, B_KMAJOR = 1, 2
EPI_BIAS, EPI_GELU, EPI_DGELU, EPI_RESIDUAL, EPI_ACCUM, EPI_A_ROWSUM = 1, 2, 4, 8, 16, 32
E_INVAL, E_WORKSPACE = -1, -2

# the project's own tolerances (tests/test_ops_gpu.py), applied per block
TOL_ATTN_FWD, TOL_ATTN_BWD, TOL_LSE, TOL_GELU = 2e-5, 5e-5, 1e-5, 1e-5


def relerr(got, want) -> float:
    got = got.detach().double().cpu()
    want = want.detach().double().cpu()
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))


def roundup(x: int, m: int) -> int:
    return -(-x // m) * m


# ------------------------------------------------------------------------------------------------ guarded buffers

class Guarded:
    """A [rows][cols] fp32 matrix with leading dimension ld inside a sentinel-filled allocation."""

    def __init__(self, rows: int, cols: int, ld: int = None, device="cpu", fill=NAN, guard_rows: int = GUARD_ROWS):
        ld = cols if ld is None else ld
        assert ld >= cols and rows > 0
        self.rows, self.cols, self.ld = rows, cols, ld
        self.guard = roundup(guard_rows * ld, 64)         # keeps the payload 256-byte aligned
        self.buf = torch.full((2 * self.guard + rows * ld,), SENTINEL, dtype=torch.int32, device=device)
        self.mat = self.buf[self.guard:self.guard + rows * ld].view(torch.float32).view(rows, ld)
        self.payload = self.mat[:, :cols]
        if isinstance(fill, torch.Tensor):
            self.payload.copy_(fill.reshape(rows, cols))
        else:
            self.payload.fill_(fill)

    @property
    def ptr(self) -> int:
        return self.mat.data_ptr()

    def get(self) -> torch.Tensor:
        return self.payload.detach().cpu().clone()

    def guard_violations(self):
        """[(row, col)] relative to the payload origin of the first few words outside the payload that changed."""
        chk = self.buf.clone()
        chk[self.guard:self.guard + self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols] = SENTINEL
        bad = (chk != SENTINEL).nonzero().flatten()[:8].cpu().tolist()
        return [divmod(i - self.guard, self.ld) for i in bad]          # negative rows: the band in front

    def assert_guards(self, what: str):
        bad = self.guard_violations()
        assert not bad, f"{what}: memory outside [{self.rows}][{self.cols}] (ld {self.ld}) was written at (row, col) {bad}"


def poisoned(t: torch.Tensor, ld: int, device="cpu", extra_rows: int = 3) -> torch.Tensor:
    """t [rows][cols] stored with leading dimension ld; the padding columns and `extra_rows` rows behind it are NaN."""
    rows, cols = t.shape
    m = torch.full((rows + extra_rows, ld), NAN, dtype=torch.float32, device=device)
    m[:rows, :cols] = t.to(device)
    return m


def check_blocks(blocks, what: str):
    """blocks: {name: (got, want fp64, tolerance)}.  Returns {name: error}; one AssertionError naming every failing block."""
    figures, failed = {}, []
    for name, (got, want, tol) in blocks.items():
        got, want = got.detach().double().cpu(), want.detach().double().cpu()
        assert got.shape == want.shape, (name, got.shape, want.shape)
        if not bool(torch.isfinite(got).all()):
            figures[name] = NAN
            failed.append(f"{name}: {int((~torch.isfinite(got)).sum())} non-finite (unwritten?) elements")
        elif float(want.abs().max()) == 0.0:
            figures[name] = float(got.abs().max())
            if figures[name] != 0.0:
                failed.append(f"{name}: reference is identically zero, got max |x| = {figures[name]:.3e}")
        else:
            figures[name] = relerr(got, want)
            if not figures[name] < tol:
                failed.append(f"{name}: {figures[name]:.3e} >= {tol:.1e}")
    assert not failed, f"{what}: " + "; ".join(failed) + f"   (all blocks: {figures})"
    return figures


# ------------------------------------------------------------------------------------------------ GEMM cases

GemmCase = namedtuple("GemmCase", "M N K layout tile split epi alpha pads data table")
TILES = [(128, 128), (128, 64), (64, 128), (64, 64)]
LAYOUTS = [3, 1, 0, 2]
SPLITS = [1, 2, 3, 7]
EPILOGUES = [0, EPI_BIAS, EPI_BIAS | EPI_GELU, EPI_DGELU, EPI_BIAS | EPI_RESIDUAL, EPI_ACCUM]
PADS = [0, 4, 36]
# tests/test_ops_gpu.py's GEMM_SHAPES, then: the epilogue shape; K % 4 != 0; tiles_m % 4 == 1, 2, 3 on 128-row tiles (580,
# 700, 836 rows) and on 64-row tiles (300, 360, 420); tiles_n == 1; N % 64 != 0; K % 32 != 0; odd tile counts
SHAPES = [(128, 128, 32), (400, 768, 768), (13, 64, 36), (616, 1536, 512), (257, 132, 100), (64, 2304, 768), (1000, 64, 3072),
          (300, 256, 128), (132, 68, 77), (580, 196, 45), (700, 320, 264), (360, 64, 130), (420, 128, 33), (836, 132, 66)]
SPLIT_SHAPES = [(400, 768, 768), (616, 1536, 512), (1000, 64, 3072), (700, 320, 264), (300, 256, 128), (132, 68, 77),
                (257, 132, 100)]
MANY_TILES = (6400, 3072, 64)           # 100 x 48 = 4800 tiles of 64 x 64: the XCD remap and the magic division at scale
BENCHED_WGRAD = (768, 768, 12800)       # the out-projection weight gradient of the benched step (plan table entry)
GAUSS_SHAPES = [(257, 132, 100), (616, 1536, 512)]


def _alpha(epi: int) -> float:
    return 0.5 if epi & EPI_ACCUM else (2.0 if epi == EPI_BIAS else 1.0)


def _case(shape, layout, tile, split, epi, n, data="int", table=None) -> GemmCase:
    M, N, K = shape
    if not layout & A_KMAJOR:
        M = roundup(M, 4)               # a [K][M]-major A needs 16-byte rows of M floats
    pads = (PADS[n % 3], PADS[(n // 3) % 3], PADS[(n // 9) % 3])
    return GemmCase(M, N, K, layout, tile, split, epi, _alpha(epi), pads, data, table)


@functools.lru_cache(maxsize=None)
def integer_matrix():
    """Every integer-data GEMM case.  Part (a): shape x tile x layout, plain; (b): tile x epilogue x split with the layouts
    cycling, and layout x epilogue x split with the tiles cycling, over the shapes; (c) A_ROWSUM on the [K][M]-major layouts
    with and without split-K; (d) the many-tile launch and the benched weight gradient with the plan table on and off.
    The three leading-dimension paddings (0, 4, 36 floats beyond the minimum) cycle independently for A, B and C."""
    cases, n = [], 0
    for shape in SHAPES:
        for tile in TILES:
            for layout in LAYOUTS:
                cases.append(_case(shape, layout, tile, 1, 0, n))
                n += 1
    for ei, epi in enumerate(EPILOGUES):
        for si, split in enumerate(SPLITS):
            shapes = SHAPES if split == 1 else SPLIT_SHAPES
            for ti, tile in enumerate(TILES):          # the partner rotates with the epilogue and the split: over the six
                cases.append(_case(shapes[n % len(shapes)], LAYOUTS[(ti + ei + si) % 4], tile, split, epi, n))   # epilogues
                n += 1                                 # every tile x split meets every layout, and the other way round
            for li, layout in enumerate(LAYOUTS):
                cases.append(_case(shapes[n % len(shapes)], layout, TILES[(li + ei + si + 2) % 4], split, epi, n))
                n += 1
    for layout in (0, 2):
        for tile in TILES:
            for split in (1, 3):
                for epi in (EPI_A_ROWSUM, EPI_A_ROWSUM | EPI_ACCUM):
                    shapes = [(132, 64, 77), (1000, 64, 3072), (300, 256, 128), (100, 36, 1000)]
                    cases.append(_case(shapes[n % 4], layout, tile, split, epi, n))
                    n += 1
    cases.append(_case(MANY_TILES, 3, (64, 64), 1, 0, 0))
    cases.append(_case(MANY_TILES, 0, (64, 64), 1, EPI_BIAS, 4))
    cases.append(_case(BENCHED_WGRAD, 0, None, 0, EPI_A_ROWSUM, 0, table=True))
    cases.append(_case(BENCHED_WGRAD, 0, None, 0, EPI_A_ROWSUM, 0, table=False))
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def gaussian_matrix():
    """The thinned Gaussian subset: each tile x layout at two shapes, under the derived bound; every fourth case keeps
    the GELU pre-activation, and the split count cycles."""
    cases, n = [], 0
    for shape in GAUSS_SHAPES:
        for tile in TILES:
            for layout in LAYOUTS:
                epi = EPI_BIAS | EPI_GELU if n % 4 == 1 else 0
                cases.append(_case(shape, layout, tile, SPLITS[(n // 4) % 4] if shape[2] >= 224 else 1, epi, n, data="gauss")
                             ._replace(alpha=1.0))
                n += 1
    return tuple(cases)


def case_id(c) -> str:
    if isinstance(c, GemmCase):
        t = "plan" if c.tile is None else f"{c.tile[0]}x{c.tile[1]}"
        tab = "" if c.table is None else f"-table{int(c.table)}"
        return f"{c.M}x{c.N}x{c.K}-l{c.layout}-{t}-s{c.split}-e{c.epi}-p{c.pads[0]}.{c.pads[1]}.{c.pads[2]}-{c.data}{tab}"
    return "-".join(".".join(map(str, v)) if isinstance(v, tuple) else str(int(v) if isinstance(v, bool) else v) for v in c)


def gemm_env(c: GemmCase) -> dict:
    """Environment switches of a case (all read on every call): name -> value, None = must be unset."""
    env = {"DCLIP_GEMM_TILE": None if c.tile is None else f"{c.tile[0]}x{c.tile[1]}", "DCLIP_GEMM_PLAN_TABLE": None}
    if c.table is False:
        env["DCLIP_GEMM_PLAN_TABLE"] = "0"
    return env


def expected_splits(K: int, split: int) -> int:
    kps = roundup(-(-K // split), 32)
    return -(-K // kps)


@functools.lru_cache(maxsize=24)
def _operands(M, N, K, data):
    g = torch.Generator().manual_seed(1000003 * M + 1009 * N + K)
    if data == "int":
        a = torch.randint(-2, 3, (M, K), generator=g).float()
        b = torch.randint(-2, 3, (N, K), generator=g).float()
        acc = (a.long() @ b.long().t()).double()           # exact: the int64 matmul
        mag = None
    else:
        a = torch.randn((M, K), generator=g)
        b = torch.randn((N, K), generator=g)
        acc = a.double() @ b.double().t()
        mag = a.double().abs() @ b.double().abs().t()
    return a, b, acc, mag


def _side(shape, data, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-2, 3, shape, generator=g).float() if data == "int" else torch.randn(shape, generator=g)


def build_gemm(c: GemmCase, device="cpu"):
    """Operands (NaN-poisoned padding) and guarded outputs of a case."""
    ak, bk = bool(c.layout & A_KMAJOR), bool(c.layout & B_KMAJOR)
    a, b, acc, mag = _operands(c.M, c.N, c.K, c.data)
    s = SimpleNamespace(case=c, a=a, b=b, acc=acc, mag=mag)
    a_st = a if ak else a.t()
    b_st = b if bk else b.t()
    s.lda = roundup(a_st.shape[1], 4) + c.pads[0]
    s.ldb = roundup(b_st.shape[1], 4) + c.pads[1]
    s.ldc = c.N + c.pads[2]
    s.A = poisoned(a_st, s.lda, device)
    s.B = poisoned(b_st, s.ldb, device)
    seed = c.M + 7 * c.N + 13 * c.K
    s.bias = _side((c.N,), c.data, seed + 1) if c.epi & EPI_BIAS else None
    s.res = _side((c.M, c.N), c.data, seed + 2) if c.epi & EPI_RESIDUAL else None
    s.c0 = _side((c.M, c.N), c.data, seed + 3) if c.epi & EPI_ACCUM else None
    s.aux_in = 2.0 * torch.randn((c.M, c.N), generator=torch.Generator().manual_seed(seed + 4)) if c.epi & EPI_DGELU else None
    s.bias_d = None if s.bias is None else s.bias.to(device)
    s.res_d = None if s.res is None else poisoned(s.res, s.ldc, device)
    s.auxin_d = None if s.aux_in is None else poisoned(s.aux_in, s.ldc, device)
    s.C = Guarded(c.M, c.N, s.ldc, device, fill=NAN if s.c0 is None else s.c0)
    s.aux = Guarded(c.M, c.N, s.ldc, device) if c.epi & EPI_GELU else None
    s.rowsum = Guarded(1, c.M, c.M, device) if c.epi & EPI_A_ROWSUM else None
    return s


def launch_gemm(lib, s, stream, workspace=None, workspace_bytes=None) -> int:
    """The C ABI call of a built case; allocates the split-K workspace the library asks for unless one is given."""
    c = s.case
    if workspace is None:
        need = int(lib.dclip_gemm_f32_workspace(c.M, c.N, c.K, c.layout, c.split))
        workspace = torch.full((max(need // 4, 1),), NAN, dtype=torch.float32, device=s.A.device)
        workspace_bytes = need
    s.workspace = workspace
    aux = s.aux.ptr if s.aux is not None else (s.rowsum.ptr if s.rowsum is not None else
                                               (s.auxin_d.data_ptr() if s.auxin_d is not None else None))
    return lib.dclip_gemm_f32(s.A.data_ptr(), s.B.data_ptr(), s.C.ptr, None if s.bias_d is None else s.bias_d.data_ptr(),
                              None if s.res_d is None else s.res_d.data_ptr(), aux, c.M, c.N, c.K, s.lda, s.ldb, s.ldc,
                              c.layout, c.epi, c.alpha, c.split, workspace.data_ptr(), workspace_bytes, stream)


def gemm_plan(lib, c: GemmCase):
    out = (ctypes.c_int * 4)()
    assert lib.dclip_gemm_f32_plan(c.M, c.N, c.K, c.layout, c.split, out) == 0
    return list(out)


def assert_gemm_plan(lib, c: GemmCase):
    """The case runs the tile and split count it was written for."""
    plan = gemm_plan(lib, c)
    if c.tile is not None:
        assert plan[:2] == list(c.tile), (plan, c)
        assert plan[2] == expected_splits(c.K, c.split), (plan, c)
    elif c.table:
        assert plan[:3] == [64, 64, 7], (plan, c)              # the measured plan-table entry
    else:
        assert plan[:3] != [64, 64, 7], (plan, c)              # the cost model's own choice
    return plan


def expected_gemm_site(c: GemmCase, plan, dma: bool = True, w8: bool = False) -> str:
    """The launch-site name dclip_last_launch must report after a case: which kernel variant launch_cfg chose."""
    if plan[2] > 1:
        return "gemm_f32.splitk_reduce"
    if plan[:2] == [128, 128] and w8:
        return "gemm_f32.w8"
    return "gemm_f32.dma" if dma and plan[0] == 128 and c.layout & A_KMAJOR else "gemm_f32"


def run_gemm_on_device(lib, c: GemmCase, device, stream, dma: bool = True, w8: bool = False):
    """Build, check the plan, launch through the C ABI, check the launch site, verify.  The caller has set gemm_env(c)."""
    s = build_gemm(c, device)
    plan = assert_gemm_plan(lib, c)
    rc = launch_gemm(lib, s, stream)
    assert rc == 0, f"{case_id(c)}: rc={rc}: {lib.dclip_last_error().decode(errors='replace')}"
    site = lib.dclip_last_launch().decode()
    torch.cuda.synchronize()
    assert site == expected_gemm_site(c, plan, dma, w8), (case_id(c), site, plan)
    fig = verify_gemm(s)
    fig["site"], fig["plan"] = site, plan
    return fig


def record(kind: str, case, figures):
    """Appends one JSON line per case to the file DCLIP_KERNEL_CHECK_LOG names (measuring aid; unset: nothing)."""
    path = os.environ.get("DCLIP_KERNEL_CHECK_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"kind": kind, "case": case_id(case), "figures": figures}) + "\n")


def quick_gelu64(x):
    x = x.double()
    return x / (1.0 + torch.exp(-1.702 * x))


def quick_gelu_grad64(x):
    x = x.double()
    sg = 1.0 / (1.0 + torch.exp(-1.702 * x))
    return sg * (1.0 + 1.702 * x * (1.0 - sg))


def emulate_gemm(s):
    """The contract of dclip_gemm_f32 as a plain fp32 torch evaluation, reading and writing the case's own buffers."""
    c = s.case
    ak, bk = bool(c.layout & A_KMAJOR), bool(c.layout & B_KMAJOR)
    a = s.A[:c.M, :c.K] if ak else s.A[:c.K, :c.M].t()
    b = s.B[:c.N, :c.K] if bk else s.B[:c.K, :c.N].t()
    v = (a @ b.t()) * c.alpha
    if c.epi & EPI_BIAS:
        v = v + s.bias_d
    if c.epi & EPI_GELU:
        s.aux.payload.copy_(v)
        v = v * torch.sigmoid(1.702 * v)
    if c.epi & EPI_DGELU:
        x = s.auxin_d[:c.M, :c.N]
        sg = torch.sigmoid(1.702 * x)
        v = v * (sg * (1.0 + 1.702 * x * (1.0 - sg)))
    if c.epi & EPI_RESIDUAL:
        v = v + s.res_d[:c.M, :c.N]
    if c.epi & EPI_ACCUM:
        v = v + s.C.payload
    s.C.payload.copy_(v)
    if c.epi & EPI_A_ROWSUM:
        s.rowsum.payload.copy_(a.sum(1)[None, :])
    return 0


def rounding_bound(K: int, mag: torch.Tensor) -> torch.Tensor:
    """(K + 8) 2^-24 (|A| |B|)_ij: gamma_K of an fp32 dot product in any order, + 8 roundings for the epilogue."""
    return (K + 8) * 2.0 ** -24 * mag


def verify_gemm(s, what: str = None):
    """Guards, then the result: exact for integer data, the derived bound for Gaussian data; GELU / DGELU against fp64 of
    the stored / given aux at the project's 1e-5.  Returns the figures it measured."""
    c = s.case
    what = what or case_id(c)
    fig = {}
    s.C.assert_guards(what + " C")
    if s.aux is not None:
        s.aux.assert_guards(what + " aux")
    if s.rowsum is not None:
        s.rowsum.assert_guards(what + " rowsum")
    got = s.C.get().double()
    lin = s.acc * c.alpha
    if c.epi & EPI_BIAS:
        lin = lin + s.bias.double()
    tail = torch.zeros_like(lin)
    if c.epi & EPI_RESIDUAL:
        tail = tail + s.res.double()
    if c.epi & EPI_ACCUM:
        tail = tail + s.c0.double()

    def linear_check(name, g, w, mag, K):
        assert bool(torch.isfinite(g).all()), f"{what} {name}: {int((~torch.isfinite(g)).sum())} non-finite (unwritten?) elements"
        if c.data == "int":
            if not torch.equal(g, w):
                bad = (g != w).nonzero()
                i, j = (int(v) for v in bad[0])
                raise AssertionError(f"{what} {name}: {bad.shape[0]} elements differ from the exact integer result, first at "
                                     f"({i}, {j}): got {float(g[i, j])}, want {float(w[i, j])}")
        else:
            ratio = float(((g - w).abs() / rounding_bound(K, mag)).max())
            fig[name + "_bound_ratio"] = ratio
            assert ratio <= 1.0, f"{what} {name}: error is {ratio:.3g} x the derived bound (K + 8) 2^-24 |A||B|"

    if c.epi & EPI_GELU:
        aux = s.aux.get().double()
        linear_check("aux", aux, lin, s.mag, c.K)
        fig["gelu"] = relerr(got, quick_gelu64(aux))               # the activation of the STORED pre-activation
        assert bool(torch.isfinite(got).all()) and fig["gelu"] < TOL_GELU, f"{what}: GELU error {fig['gelu']:.3e}"
    elif c.epi & EPI_DGELU:
        fig["dgelu"] = relerr(got, lin * quick_gelu_grad64(s.aux_in) + tail)
        assert bool(torch.isfinite(got).all()) and fig["dgelu"] < TOL_GELU, f"{what}: DGELU error {fig['dgelu']:.3e}"
    else:
        linear_check("C", got, lin + tail, s.mag, c.K)
    if c.epi & EPI_A_ROWSUM:
        rs = s.rowsum.get().double().reshape(-1)
        linear_check("rowsum", rs[None, :], s.a.double().sum(1)[None, :], s.a.double().abs().sum(1)[None, :], c.K)
    return fig


# ------------------------------------------------------------------------------------------------ attention cases

HD = 64
SelfCase = namedtuple("SelfCase", "B S H causal mode")         # mode: default | tiled | fused | no_ds
CrossCase = namedtuple("CrossCase", "B Lq Lk H")
ClsCase = namedtuple("ClsCase", "B S H")
RowCase = namedtuple("RowCase", "B S H rows")

ATTN_ENV = {"default": {}, "tiled": {"DCLIP_ATTN_TILED": "1"}, "fused": {"DCLIP_ATTN_FUSED": "1"},
            "no_ds": {"DCLIP_ATTN_NO_DS": "1"}}
ATTN_SWITCHES = ("DCLIP_ATTN_TILED", "DCLIP_ATTN_FUSED", "DCLIP_ATTN_NO_DS")

_SELF_BASE = [(2, 50, 2, False), (3, 77, 2, True), (1, 197, 3, False), (2, 10, 1, True), (1, 257, 2, False), (2, 16, 2, True),
              (1, 64, 1, False), (1, 130, 1, True), (2, 65, 2, True), (2, 80, 1, False), (2, 77, 2, False), (1, 81, 1, True),
              (2, 1, 1, True), (2, 33, 2, False), (1, 48, 1, True)]          # tests/test_ops_gpu.py::test_attention_fwd_bwd
_SELF_EDGES = [17, 32, 64, 65, 80, 81, 128, 129]                             # the KT and tile boundaries


@functools.lru_cache(maxsize=None)
def self_cases():
    shapes = list(_SELF_BASE)
    for i, S in enumerate(_SELF_EDGES):
        for causal in (False, True):
            shape = (1 + i % 2, S, 1 + (i + causal) % 2, causal)
            if shape not in shapes:
                shapes.append(shape)
    cases = []
    for B, S, H, causal in shapes:
        cases.append(SelfCase(B, S, H, causal, "default"))
        cases.append(SelfCase(B, S, H, causal, "tiled"))
        if S <= 64:
            cases.append(SelfCase(B, S, H, causal, "fused"))
        if S > 80 and not causal:
            cases.append(SelfCase(B, S, H, causal, "no_ds"))
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def cross_cases():
    pairs = [(8, 75), (75, 8), (1, 64), (65, 130), (7, 4), (96, 96), (8, 8), (64, 64), (80, 80), (130, 130)]
    hb = [(1, 1), (2, 3), (8, 1), (1, 3), (2, 1), (8, 3)]
    return tuple(CrossCase(B, Lq, Lk, H) for i, (Lq, Lk) in enumerate(pairs) for H, B in (hb[i % 6], hb[(i + 3) % 6]))


CLS_CASES = tuple(ClsCase(B, S, H) for S in (1, 50, 197, 257) for B, H in ((2, 2), (1, 3)))
ROW_CASES = (RowCase(6, 77, 2, (0, 1, 63, 64, 76, 30)), RowCase(3, 77, 1, (76, 0, 64)), RowCase(1, 77, 8, (63,)))


def expected_launches(c):
    """(forward, backward) launch-site names the dispatch of attention.hip must report for a case."""
    if isinstance(c, SelfCase):
        tiled = c.mode == "tiled"
        fwd = "attention_fwd" if tiled else ("attention_fwd.rows" if c.S <= 80 else "attention_fwd.stream")
        if c.S == 1:
            bwd = "attention_bwd.one_key"                       # a single key: the exact-zero form, whatever the switch
        elif c.S <= 64:
            bwd = "attention_bwd.fused" if c.mode == "fused" else "attention_bwd.lean"
        elif tiled:
            bwd = "attention_bwd"
        elif c.S <= 80:
            bwd = "attention_bwd.rows"
        elif c.causal:
            bwd = "attention_bwd"
        elif c.S <= 512 and c.mode != "no_ds":
            bwd = "attention_bwd.stream_ds"
        else:
            bwd = "attention_bwd.stream"
        return fwd, bwd
    if isinstance(c, CrossCase):
        if c.Lq == c.Lk:        # the self-attention kernels with q / kv row strides E and 2E
            return ("attention_fwd.rows" if c.Lk <= 80 else "attention_fwd.stream"), "attention_bwd.stream"
        return "attention_fwd", "attention_bwd"
    if isinstance(c, ClsCase):
        return ("attention_fwd.rows", "attention_bwd.one_key") if c.S == 1 else ("attention_fwd", "attention_bwd")
    return "attention_fwd", None


def attention_math(q, k, v, dout, mask=None):
    """softmax(q k^T / 8 + mask) v in the dtype of its inputs ([B, L, H, 64] each) and its gradients: out, lse, dq, dk, dv."""
    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    sc = torch.einsum("bqhd,bkhd->bhqk", q, k) * 0.125
    if mask is not None:
        sc = sc + mask
    p = torch.softmax(sc, dim=-1)
    out = torch.einsum("bhqk,bkhd->bqhd", p, v)
    lse = torch.logsumexp(sc, dim=-1)                          # [B, H, Lq]
    if dout is None:
        return out.detach(), lse.detach(), None, None, None
    (out * dout).sum().backward()
    return out.detach(), lse.detach(), q.grad, k.grad, v.grad


def _causal_mask(S, dtype, device):
    return torch.full((S, S), float("-inf"), dtype=dtype, device=device).triu(1)


def _gauss(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def build_attn(c, device="cpu"):
    s = SimpleNamespace(case=c)
    if isinstance(c, SelfCase):
        D = c.H * HD
        s.qkv = _gauss((c.B * c.S, 3 * D), 1, 1.5).to(device)
        s.dout = _gauss((c.B * c.S, D), 2).to(device)
        s.out, s.lse = Guarded(c.B * c.S, D, device=device), Guarded(1, c.B * c.H * c.S, device=device)
        s.dqkv = Guarded(c.B * c.S, 3 * D, device=device)
    elif isinstance(c, CrossCase):
        E = c.H * HD
        s.q = _gauss((c.B * c.Lq, E), 3, 1.5).to(device)
        s.kv = _gauss((c.B * c.Lk, 2 * E), 4, 1.5).to(device)
        s.dout = _gauss((c.B * c.Lq, E), 5).to(device)
        s.out, s.lse = Guarded(c.B * c.Lq, E, device=device), Guarded(1, c.B * c.H * c.Lq, device=device)
        s.dq, s.dkv = Guarded(c.B * c.Lq, E, device=device), Guarded(c.B * c.Lk, 2 * E, device=device)
        s.delta = Guarded(1, c.B * c.H * c.Lq, device=device)
    elif isinstance(c, ClsCase):
        D = c.H * HD
        s.qkv = _gauss((c.B * c.S, 3 * D), 6, 1.5).to(device)
        s.dout = _gauss((c.B, D), 7).to(device)
        s.out, s.lse = Guarded(c.B, D, device=device), Guarded(1, c.B * c.H, device=device)
        s.dqkv = Guarded(c.B * c.S, 3 * D, device=device, fill=0.0)        # the zero fill the entry's contract requires
        s.delta = Guarded(1, c.B * c.H, device=device)
    else:
        D = c.H * HD
        s.qkv = _gauss((c.B * c.S, 3 * D), 8, 1.5).to(device)
        s.rows = torch.tensor(c.rows, dtype=torch.int32, device=device)
        s.out, s.lse = Guarded(c.B, D, device=device), Guarded(1, c.B * c.H, device=device)
    return s


def attn_results(s, dtype):
    """{block: tensor} of a case evaluated plainly in `dtype` (fp64: the reference; fp32: the CPU stand-in)."""
    c = s.case
    if isinstance(c, SelfCase):
        B, S, H = c.B, c.S, c.H
        q, k, v = (s.qkv.to(dtype).view(B, S, 3, H, HD)[:, :, i] for i in range(3))
        mask = _causal_mask(S, dtype, s.qkv.device) if c.causal else None
        out, lse, dq, dk, dv = attention_math(q, k, v, s.dout.to(dtype).view(B, S, H, HD), mask)
        return {"out": out.reshape(B * S, -1), "lse": lse.reshape(1, -1), "dq": dq.reshape(B * S, -1),
                "dk": dk.reshape(B * S, -1), "dv": dv.reshape(B * S, -1)}
    if isinstance(c, CrossCase):
        B, H = c.B, c.H
        q = s.q.to(dtype).view(B, c.Lq, H, HD)
        k, v = (s.kv.to(dtype).view(B, c.Lk, 2, H, HD)[:, :, i] for i in range(2))
        out, lse, dq, dk, dv = attention_math(q, k, v, s.dout.to(dtype).view(B, c.Lq, H, HD))
        return {"out": out.reshape(B * c.Lq, -1), "lse": lse.reshape(1, -1), "dq": dq.reshape(B * c.Lq, -1),
                "dk": dk.reshape(B * c.Lk, -1), "dv": dv.reshape(B * c.Lk, -1)}
    if isinstance(c, ClsCase):
        B, S, H = c.B, c.S, c.H
        q, k, v = (s.qkv.to(dtype).view(B, S, 3, H, HD)[:, :, i] for i in range(3))
        out, lse, dq0, dk, dv = attention_math(q[:, :1], k, v, s.dout.to(dtype).view(B, 1, H, HD))   # row 0 alone
        dq = torch.zeros(B, S, H * HD, dtype=dtype, device=dq0.device)
        dq[:, 0] = dq0.reshape(B, -1)
        return {"out": out.reshape(B, -1), "lse": lse.reshape(1, -1), "dq_cls": dq[:, 0].clone(),
                "dq_other_rows": dq[:, 1:].reshape(B * (S - 1), -1) if S > 1 else torch.zeros(1, 1, dtype=dtype),
                "dk": dk.reshape(B * S, -1), "dv": dv.reshape(B * S, -1)}
    B, S, H = c.B, c.S, c.H
    q, k, v = (s.qkv.to(dtype).view(B, S, 3, H, HD)[:, :, i] for i in range(3))
    rows = torch.tensor(c.rows, device=s.qkv.device)
    qr = q[torch.arange(B), rows][:, None]                                                # [B, 1, H, 64]
    mask = torch.where(torch.arange(S, device=rows.device)[None, :] <= rows[:, None], 0.0, float("-inf")).to(dtype)
    out, lse, _, _, _ = attention_math(qr, k, v, None, mask[:, None, None, :])
    return {"out": out.reshape(B, -1), "lse": lse.reshape(1, -1)}


def attn_device_blocks(s):
    """{block: tensor} read back from the guarded buffers, named as attn_results names them."""
    c = s.case
    got = {"out": s.out.get(), "lse": s.lse.get()}
    if isinstance(c, SelfCase):
        D = c.H * HD
        d = s.dqkv.get()
        got.update(dq=d[:, :D], dk=d[:, D:2 * D], dv=d[:, 2 * D:])
    elif isinstance(c, CrossCase):
        E = c.H * HD
        d = s.dkv.get()
        got.update(dq=s.dq.get(), dk=d[:, :E], dv=d[:, E:])
    elif isinstance(c, ClsCase):
        D = c.H * HD
        d = s.dqkv.get()
        dq = d[:, :D].reshape(c.B, c.S, D)
        got.update(dq_cls=dq[:, 0], dq_other_rows=dq[:, 1:].reshape(-1, D) if c.S > 1 else torch.zeros(1, 1),
                   dk=d[:, D:2 * D], dv=d[:, 2 * D:])
    return got


def emulate_attn(s):
    """Plain fp32 evaluation written into the case's buffers the way the entry points write them."""
    c = s.case
    r = attn_results(s, torch.float32)
    s.out.payload.copy_(r["out"])
    s.lse.payload.copy_(r["lse"])
    if isinstance(c, SelfCase):
        s.dqkv.payload.copy_(torch.cat([r["dq"], r["dk"], r["dv"]], 1))
    elif isinstance(c, CrossCase):
        s.dq.payload.copy_(r["dq"])
        s.dkv.payload.copy_(torch.cat([r["dk"], r["dv"]], 1))
    elif isinstance(c, ClsCase):
        D = c.H * HD
        s.dqkv.payload.view(c.B, c.S, 3 * D)[:, 0, :D] = r["dq_cls"]           # the other q rows keep the caller's zeros
        s.dqkv.payload[:, D:] = torch.cat([r["dk"], r["dv"]], 1)


def launch_attn(lib, s, stream):
    """The C ABI calls of a built case.  Returns the (forward, backward) launch-site names the library reports."""
    c = s.case

    def ok(rc, what):
        assert rc == 0, f"{what}: rc={rc}: {lib.dclip_last_error().decode(errors='replace')}"
        return lib.dclip_last_launch().decode()

    if isinstance(c, SelfCase):
        fwd = ok(lib.dclip_attention_fwd(s.qkv.data_ptr(), s.out.ptr, s.lse.ptr, c.B, c.S, c.H, int(c.causal), stream), "fwd")
        need = int(lib.dclip_attention_bwd_workspace(c.B, c.S, c.H, int(c.causal)))
        s.ws = torch.full((need // 4 + 4,), NAN, dtype=torch.float32, device=s.qkv.device)
        bwd = ok(lib.dclip_attention_bwd_ws(s.qkv.data_ptr(), s.out.ptr, s.dout.data_ptr(), s.lse.ptr, s.dqkv.ptr,
                                            s.ws.data_ptr(), need, c.B, c.S, c.H, int(c.causal), stream), "bwd")
        return fwd, bwd
    if isinstance(c, CrossCase):
        fwd = ok(lib.dclip_cross_attention_fwd(s.q.data_ptr(), s.kv.data_ptr(), s.out.ptr, s.lse.ptr, c.B, c.Lq, c.Lk, c.H,
                                               stream), "cross fwd")
        bwd = ok(lib.dclip_cross_attention_bwd(s.q.data_ptr(), s.kv.data_ptr(), s.out.ptr, s.dout.data_ptr(), s.lse.ptr,
                                               s.dq.ptr, s.dkv.ptr, s.delta.ptr, c.B, c.Lq, c.Lk, c.H, stream), "cross bwd")
        return fwd, bwd
    if isinstance(c, ClsCase):
        fwd = ok(lib.dclip_attention_cls_fwd(s.qkv.data_ptr(), s.out.ptr, s.lse.ptr, c.B, c.S, c.H, stream), "cls fwd")
        bwd = ok(lib.dclip_attention_cls_bwd(s.qkv.data_ptr(), s.out.ptr, s.dout.data_ptr(), s.lse.ptr, s.dqkv.ptr,
                                             s.delta.ptr, c.B, c.S, c.H, stream), "cls bwd")
        return fwd, bwd
    fwd = ok(lib.dclip_attention_row_fwd(s.qkv.data_ptr(), s.rows.data_ptr(), s.out.ptr, s.lse.ptr, c.B, c.S, c.H, stream),
             "row fwd")
    return fwd, None


def verify_attn(s, what: str = None):
    """Guards of every output, then out / lse / dq / dk / dv block by block against fp64."""
    c = s.case
    what = what or case_id(c)
    for name in ("out", "lse", "dqkv", "dq", "dkv", "delta"):
        if hasattr(s, name):
            getattr(s, name).assert_guards(f"{what} {name}")
    want, got = attn_results(s, torch.float64), attn_device_blocks(s)
    tol = {"out": TOL_ATTN_FWD, "lse": TOL_LSE}
    return check_blocks({k: (got[k], want[k], tol.get(k, TOL_ATTN_BWD)) for k in want}, what)
