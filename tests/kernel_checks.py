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
SENTINEL16 = 0x7FA5              # the 16-bit guard word: a NaN with a payload as bf16 (exponent 0xFF) and as fp16 (exponent 0x1F)
NAN16 = {torch.bfloat16: 0x7FC0, torch.float16: 0x7E00}      # what a 16-bit NaN payload holds (the formats' quiet NaN)
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
    """A [rows][cols] fp32 (or bf16 / fp16) matrix with leading dimension ld inside a sentinel-filled allocation."""

    def __init__(self, rows: int, cols: int, ld: int = None, device="cpu", fill=NAN, guard_rows: int = GUARD_ROWS,
                 dtype=torch.float32):
        ld = cols if ld is None else ld
        assert ld >= cols and rows > 0
        self.rows, self.cols, self.ld, self.dtype = rows, cols, ld, dtype
        self.sentinel, word = (SENTINEL, torch.int32) if dtype == torch.float32 else (SENTINEL16, torch.int16)
        self.guard = roundup(guard_rows * ld, 64)         # keeps the payload 256-byte (16-bit: 128-byte) aligned
        self.buf = torch.full((2 * self.guard + rows * ld,), self.sentinel, dtype=word, device=device)
        self.mat = self.buf[self.guard:self.guard + rows * ld].view(dtype).view(rows, ld)
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
        chk[self.guard:self.guard + self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols] = self.sentinel
        bad = (chk != self.sentinel).nonzero().flatten()[:8].cpu().tolist()
        return [divmod(i - self.guard, self.ld) for i in bad]          # negative rows: the band in front

    def assert_guards(self, what: str):
        bad = self.guard_violations()
        assert not bad, f"{what}: memory outside [{self.rows}][{self.cols}] (ld {self.ld}) was written at (row, col) {bad}"


def poisoned(t: torch.Tensor, ld: int, device="cpu", extra_rows: int = 3, dtype=torch.float32) -> torch.Tensor:
    """t [rows][cols] stored in `dtype` with leading dimension ld; the padding columns and `extra_rows` rows behind it are NaN."""
    rows, cols = t.shape
    m = torch.full((rows + extra_rows, ld), NAN, dtype=dtype, device=device)
    m[:rows, :cols] = t.to(device=device, dtype=dtype)
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


def expected_gemm_site(c: GemmCase, plan, dma: bool = True) -> str:
    """The launch-site name dclip_last_launch must report after a case: which kernel variant launch_cfg chose."""
    if plan[2] > 1:
        return "gemm_f32.splitk_reduce"
    return "gemm_f32.dma" if dma and plan[0] == 128 and c.layout & A_KMAJOR else "gemm_f32"


def run_gemm_on_device(lib, c: GemmCase, device, stream, dma: bool = True):
    """Build, check the plan, launch through the C ABI, check the launch site, verify.  The caller has set gemm_env(c)."""
    s = build_gemm(c, device)
    plan = assert_gemm_plan(lib, c)
    rc = launch_gemm(lib, s, stream)
    assert rc == 0, f"{case_id(c)}: rc={rc}: {lib.dclip_last_error().decode(errors='replace')}"
    site = lib.dclip_last_launch().decode()
    torch.cuda.synchronize()
    assert site == expected_gemm_site(c, plan, dma), (case_id(c), site, plan)
    fig = verify_gemm(s)
    fig["site"], fig["plan"] = site, plan
    return fig


def record(kind: str, case, figures):
    """Appends one JSON line per case to the file DCLIP_KERNEL_CHECK_LOG names (measuring aid; unset: nothing)."""
    path = os.environ.get("DCLIP_KERNEL_CHECK_LOG")
    if path:
        with open(path, "a") as f:
            ident = case16_id(case) if isinstance(case, Gemm16Case) else case_id(case)
            f.write(json.dumps({"kind": kind, "case": ident, "figures": figures}) + "\n")


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
SelfCase = namedtuple("SelfCase", "B S H causal mode")         # mode: default | tiled | no_ds
CrossCase = namedtuple("CrossCase", "B Lq Lk H")
ClsCase = namedtuple("ClsCase", "B S H")
RowCase = namedtuple("RowCase", "B S H rows")

ATTN_ENV = {"default": {}, "tiled": {"DCLIP_ATTN_TILED": "1"}, "no_ds": {"DCLIP_ATTN_NO_DS": "1"}}
ATTN_SWITCHES = ("DCLIP_ATTN_TILED", "DCLIP_ATTN_NO_DS")

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
            bwd = "attention_bwd.lean"
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


# ==================================================================================================================
# The 16-bit half: dclip_amd/csrc/gemm_bf16.hip and attention_bf16.hip through the C ABI.
#   * integer-exact 16-bit GEMM: integers in [-2, 2] are exact in bf16 and fp16 and the fp32 accumulator is exact (above), so
#     an fp32 C equals the exact result and a 16-bit C / saved pre-activation equals its round-to-nearest-even conversion;
#   * exact-selection attention: q_i = k_pi(i) with keys 8 x (+-1)^64 makes P exactly one-hot (the margin is computed and the
#     case refused below 120), so out == v[pi], dV is an integer sum and dQ = dK = 0, bit for bit;
#   * derived per-element bounds for Gaussian data against fp64 of the 16-bit-rounded inputs (u = half the spacing of the type).

Type16 = namedtuple("Type16", "name dtype u saturating")
TYPES16 = {"bf16": Type16("bf16", torch.bfloat16, 2.0 ** -8, False),
           "f16": Type16("f16", torch.float16, 2.0 ** -11, True),          # F16T: a finite overflow saturates at +-65504
           "f16ex": Type16("f16ex", torch.float16, 2.0 ** -11, False)}     # F16IeeeT: plain IEEE, an overflow is +-inf
F32_TINY = 2.0 ** -126           # results below the smallest normal fp32 may be flushed
F16_SUB = 2.0 ** -25             # half the spacing of the fp16 subnormals: the absolute error of rounding into that range


def round16(x: torch.Tensor, ty: Type16) -> torch.Tensor:
    """fp32 -> the 16-bit type, round to nearest even, with the type's overflow rule (dclip_amd/csrc/common.h)."""
    x = x.float()
    if ty.saturating:
        x = torch.where(torch.isfinite(x), x.clamp(-65504.0, 65504.0), x)
    return x.to(ty.dtype)


def out_floor(ty: Type16, out16: bool) -> float:
    return F32_TINY + (F16_SUB if out16 and ty.dtype == torch.float16 else 0.0)


# ------------------------------------------------------------------------------------------------ 16-bit GEMM cases

Gemm16Case = namedtuple("Gemm16Case", "entry ty M N K epi out16 save pads splits env want data")
GEMM16_NAMES = {"gemm": {"bf16": "gemm_bf16", "f16": "gemm_f16", "f16ex": "gemm_f16_ex"},
                "splitk": {"bf16": "gemm_bf16_splitk", "f16ex": "gemm_f16_splitk"},
                "tok": {"bf16": "gemm_bf16_wgrad_tokmajor", "f16ex": "gemm_f16_wgrad_tokmajor"}}
GEMM16_SWITCHES = ("DCLIP_BF16_BIG_MIN", "DCLIP_BF16_PERSIST", "DCLIP_BF16_PERSIST_MIN")   # read per call
ENV_BIG = (("DCLIP_BF16_BIG_MIN", "1"),)
ENV_PPP = (("DCLIP_BF16_BIG_MIN", "1"), ("DCLIP_BF16_PERSIST", "1"), ("DCLIP_BF16_PERSIST_MIN", "1"))
PADS16_K, PADS16_C = [0, 8, 40], [0, 4, 36]
# (epilogue, 16-bit output, aux): every combination the dispatcher accepts
EPI16 = [(0, 0, 0), (0, 1, 0), (EPI_BIAS, 0, 0), (EPI_BIAS, 1, 0), (EPI_BIAS | EPI_GELU, 0, 0), (EPI_BIAS | EPI_GELU, 1, 0),
         (EPI_BIAS | EPI_GELU, 0, 1), (EPI_BIAS | EPI_GELU, 1, 1), (EPI_DGELU, 0, 1), (EPI_DGELU, 1, 1), (EPI_BIAS | EPI_RESIDUAL, 0, 0)]
EPI16_PPP = [e for e in EPI16 if not e[0] & EPI_DGELU]              # DGELU stays on the one-tile kernel
# one short of and one past 64, 128, 256 in both M and N; N % 8 != 0 with N % 4 == 0: a partial 16-bit output vector
EDGE_SHAPES16 = [(63, 60), (65, 68), (127, 124), (129, 132), (255, 252), (257, 260), (64, 64), (13, 4), (256, 128)]
K16 = [64, 128, 192, 72, 85, 149, 4100]
BIG_SHAPES16 = EDGE_SHAPES16 + [(1000, 520), (511, 508), (300, 1028)]
K16_BIG = [64, 128, 192, 768]
R128_SHAPE = (2047, 2044)               # 16 x 16 = 256 tiles of 128 (the r128 threshold), 8 x 8 = 64 tiles of 256
BENCHED_FWD16 = (12800, 3072, 768)      # fc1 of the benched student step
PPP_SHAPES16 = [(200, 256), (1789, 248), (600, 520), (4200, 4096)]          # 1, 7, 9 and 272 tiles of 256 x 256
TOK_SHAPES16 = [(64, 64), (72, 136), (264, 248), (520, 1000)]
SPLITS16 = [1, 2, 3, 7, 64]


def epi_ok(ty: str, e) -> bool:
    return not (ty == "f16" and e[2])           # dclip_gemm_f16 has no aux argument: no saved pre-activation, no DGELU


def _c16(entry, ty, shape, K, e, n, splits=1, env=(), want="r64", data="int", kpads=PADS16_K, cpads=PADS16_C):
    pads = (kpads[n % 3], kpads[(n // 3) % 3], cpads[(n // 9) % 3 if len(cpads) == 3 else 0])
    return Gemm16Case(entry, ty, shape[0], shape[1], K, e[0], e[1], e[2], pads, splits, env, want, data)


def s_eff16(K: int, splits: int) -> int:
    return -(-K // roundup(-(-K // splits), 64))


@functools.lru_cache(maxsize=None)
def gemm16_matrix():
    """Every integer-data 16-bit GEMM case.  (a) r64: edge shapes x K with type, epilogue and padding cycling, then every type x
    epilogue; (b) r128 at 2047 x 2044; (c) pp (DCLIP_BF16_BIG_MIN=1) over shape x K and over type x epilogue; (d) ppp at 1, 7,
    9 and 272 tiles; (e) the benched forward shape; (f) split-K on r128 and pp with splits 1, 2, 3, 7, 64 and more than K / 64;
    (g) the token-major weight gradient with s_eff == 1 and > 1; (h) values beyond 65504 for the two fp16 overflow rules.
    The counter n that cycles type, epilogue and padding jumps once: (b) held four cases of a kernel that was removed
    (DESIGN.md §17b), and every case after them keeps the operands it had."""
    types, cases, n = ["bf16", "f16", "f16ex"], [], 0

    def pick(ty, n):
        e = EPI16[n % len(EPI16)]
        return e if epi_ok(ty, e) else EPI16[n % 6]
    for shape in EDGE_SHAPES16:                                              # (a)
        for K in K16:
            ty = types[n % 3]
            cases.append(_c16("gemm", ty, shape, K, pick(ty, n // 3 + n), n))
            n += 1
    for ty in types:
        for e in EPI16:
            if epi_ok(ty, e):
                cases.append(_c16("gemm", ty, EDGE_SHAPES16[n % 6], K16[n % 7], e, n))
                n += 1
    for ty, K, e in [("bf16", 64, EPI16[7]), ("f16", 85, EPI16[1]), ("f16ex", 192, EPI16[8]), ("bf16", 149, EPI16[10]),
                     ("f16ex", 72, EPI16[3]), ("f16", 128, EPI16[4])]:      # (b)
        cases.append(_c16("gemm", ty, R128_SHAPE, K, e, n, want="r128"))
        n += 1
    n += 4                                                                   # (four cases of a removed kernel)
    for shape in BIG_SHAPES16:                                               # (c)
        for K in K16_BIG:
            ty = types[n % 3]
            cases.append(_c16("gemm", ty, shape, K, pick(ty, n // 3 + n), n, env=ENV_BIG, want="pp"))
            n += 1
    for ty in types:
        for e in EPI16:
            if epi_ok(ty, e):
                cases.append(_c16("gemm", ty, BIG_SHAPES16[n % len(BIG_SHAPES16)], K16_BIG[n % 3], e, n, env=ENV_BIG, want="pp"))
                n += 1
    for ty in ("bf16", "f16"):                                               # (d): needs N % 8 == 0 and ldc % 8 == 0
        for si, shape in enumerate(PPP_SHAPES16):
            for e in (EPI16_PPP if si < 3 else EPI16_PPP[n % 3::3]):
                if epi_ok(ty, e):                # GELU with an fp32 C is not in the persistent kernel: it must stay on pp
                    cases.append(_c16("gemm", ty, shape, 64 if si == 3 else K16_BIG[n % 4], e, n, env=ENV_PPP,
                                      want="pp" if e[0] & EPI_GELU and not e[1] else "ppp", cpads=PADS16_K))
                    n += 1
    cases.append(Gemm16Case("gemm", "bf16", 600, 520, 128, EPI_BIAS, 1, 0, (8, 0, 4), 1, ENV_PPP, "pp", "int"))   # ldc % 8 != 0
    cases.append(Gemm16Case("gemm", "bf16", 600, 520, 128, EPI_DGELU, 1, 1, (8, 0, 8), 1, ENV_PPP, "pp", "int"))  # DGELU
    cases.append(_c16("gemm", "bf16", BENCHED_FWD16[:2], BENCHED_FWD16[2], EPI16[3], 0, want="pp"))                 # (e)
    for ty in ("bf16", "f16ex"):                                             # (f)
        for shape, K in [((300, 256), 149), ((132, 68), 4100), ((257, 132), 85), ((64, 64), 192), ((255, 252), 768)]:
            for splits in SPLITS16 + [K // 64 + 5]:
                want = "r64" if splits == 1 else "r128"
                cases.append(_c16("splitk", ty, shape, K, EPI16[0], n, splits=splits, want=want))
                n += 1
        for shape, K in [(R128_SHAPE, 192), ((2040, 2048), 320)]:            # 64 tiles of 256: pp from s_eff = 2
            for splits in SPLITS16[1:] + [K // 64 + 5]:
                cases.append(_c16("splitk", ty, shape, K, EPI16[0], n, splits=splits, want="pp"))
                n += 1
        cases.append(_c16("splitk", ty, BENCHED_WGRAD[:2], BENCHED_WGRAD[2], EPI16[0], n, splits=17, want="pp"))   # 16 slabs of 768 + 512
        for shape in TOK_SHAPES16:                                           # (g)
            for K, splits in [(64, 1), (64, 3), (192, 1), (192, 2), (192, 3), (192, 7), (192, 64), (320, 3)]:
                cases.append(_c16("tok", ty, shape, K, EPI16[0], n, splits=splits, want="pp_tok"))
                n += 1
        cases.append(_c16("tok", ty, BENCHED_WGRAD[:2], BENCHED_WGRAD[2], EPI16[0], n, splits=28, want="pp_tok"))
    for ty in types:                                                         # (h)
        cases.append(_c16("gemm", ty, (65, 68), 64, EPI16[1], n, data="big"))
        cases.append(_c16("gemm", ty, (257, 260), 128, EPI16[3], n + 1, env=ENV_BIG, want="pp", data="big"))
        n += 2
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def gemm16_gaussian_matrix():
    """The thinned Gaussian subset under the derived bound: each kernel variant, each type, the epilogues that round."""
    cases, n = [], 0
    for ty in ("bf16", "f16", "f16ex"):
        for e in (EPI16[0], EPI16[1], EPI16[7] if ty != "f16" else EPI16[5], EPI16[6] if ty != "f16" else EPI16[4]):
            cases.append(_c16("gemm", ty, (257, 132), 149 if n % 2 else 768, e, n, data="gauss"))
            cases.append(_c16("gemm", ty, (511, 508), 768 if n % 2 else 192, e, n + 1, env=ENV_BIG, want="pp", data="gauss"))
            n += 2
        if ty != "f16ex":
            cases.append(_c16("gemm", ty, (600, 520), 768, EPI16[5], n, env=ENV_PPP, want="ppp", data="gauss", cpads=PADS16_K))
        if ty != "f16":
            cases.append(_c16("gemm", ty, (300, 1028), 256, EPI16[9], n, env=ENV_BIG, want="pp", data="gauss"))
            cases.append(_c16("splitk", ty, (300, 256), 4100, EPI16[0], n, splits=7, want="r128", data="gauss"))
            cases.append(_c16("splitk", ty, R128_SHAPE, 320, EPI16[0], n, splits=3, want="pp", data="gauss"))
            cases.append(_c16("tok", ty, (264, 248), 1280, EPI16[0], n, splits=3, want="pp_tok", data="gauss"))
        cases.append(_c16("gemm", ty, R128_SHAPE, 85, EPI16[3], n, want="r128", data="gauss"))
        n += 1
    return tuple(cases)


def case16_id(c: Gemm16Case) -> str:
    env = "".join("-" + k[11:].lower() + v for k, v in c.env)
    return (f"{c.entry}-{c.ty}-{c.M}x{c.N}x{c.K}-e{c.epi}-o{c.out16}-a{c.save}-p{c.pads[0]}.{c.pads[1]}.{c.pads[2]}-s{c.splits}"
            f"{env}-{c.want}-{c.data}")


def gemm16_env(c: Gemm16Case) -> dict:
    env = {k: None for k in GEMM16_SWITCHES}
    env.update(dict(c.env))
    return env


def gemm16_reduces(c: Gemm16Case) -> bool:
    return (c.entry == "splitk" and c.splits != 1) or (c.entry == "tok" and s_eff16(c.K, c.splits) > 1)


def expected_gemm16_site(c: Gemm16Case) -> str:
    """What dclip_last_launch must report."""
    return GEMM16_NAMES[c.entry][c.ty] + "." + c.want + (".splitk_reduce" if gemm16_reduces(c) else "")


@functools.lru_cache(maxsize=8)
def _operands16(M, N, K, data, dtype):
    g = torch.Generator().manual_seed(1000003 * M + 1009 * N + K + 17)
    if data == "gauss":
        a = torch.randn((M, K), generator=g).to(dtype).float()
        w = torch.randn((N, K), generator=g).to(dtype).float()
        return a, w, a.double() @ w.double().t(), a.double().abs() @ w.double().abs().t()
    scale = 64.0 if data == "big" else 1.0       # "big": integers up to 128, products up to 2^14, sums beyond 65504 and below 2^24
    a = torch.randint(-2, 3, (M, K), generator=g).float() * scale
    w = torch.randint(-2, 3, (N, K), generator=g).float() * scale
    assert 4.0 * scale * scale * K < 2 ** 24
    return a, w, a @ w.t(), None                # exact in fp32: every partial sum in any order is an integer below 2^24


def build_gemm16(c: Gemm16Case, device="cpu"):
    """Operands (NaN-poisoned padding) and guarded outputs of a 16-bit case."""
    ty = TYPES16[c.ty]
    a, w, acc, mag = _operands16(c.M, c.N, c.K, c.data, ty.dtype)
    s = SimpleNamespace(case=c, ty=ty, a=a, w=w, acc=acc, mag=mag)
    tok = c.entry == "tok"                      # dY [K][lddy >= M], X [K][ldx >= N]
    a_st, w_st = (a.t(), w.t()) if tok else (a, w)
    s.lda, s.ldw = roundup(a_st.shape[1], 8) + c.pads[0], roundup(w_st.shape[1], 8) + c.pads[1]
    s.ldc = c.N + c.pads[2]
    s.A = poisoned(a_st, s.lda, device, dtype=ty.dtype)
    s.W = poisoned(w_st, s.ldw, device, dtype=ty.dtype)
    seed = c.M + 7 * c.N + 13 * c.K
    gauss = "gauss" if c.data == "gauss" else "int"
    s.bias = _side((c.N,), gauss, seed + 1) if c.epi & EPI_BIAS else None
    s.res = _side((c.M, c.N), gauss, seed + 2) if c.epi & EPI_RESIDUAL else None
    s.aux_in = None
    if c.epi & EPI_DGELU:
        s.aux_in = _side((c.M, c.N), gauss, seed + 4).to(ty.dtype).float()          # what the forward saved: a 16-bit value
    s.bias_d = None if s.bias is None else s.bias.to(device)
    s.res_d = None if s.res is None else poisoned(s.res, s.ldc, device)
    s.auxin_d = None if s.aux_in is None else poisoned(s.aux_in, s.ldc, device, dtype=ty.dtype)
    s.C = Guarded(c.M, c.N, s.ldc, device, dtype=ty.dtype if c.out16 else torch.float32)
    s.aux = Guarded(c.M, c.N, s.ldc, device, dtype=ty.dtype) if c.epi & EPI_GELU and c.save else None
    s.ws, s.ws_need = None, 0
    if gemm16_reduces(c):
        s.ws_need = s_eff16(c.K, c.splits) * c.M * c.N            # floats; 64 more behind them must stay untouched
        s.ws = Guarded(1, s.ws_need + 64, device=device, guard_rows=1)
    return s


def launch_gemm16(lib, s, stream, workspace_bytes=None) -> int:
    c = s.case
    name = "dclip_" + GEMM16_NAMES[c.entry][c.ty]
    ptr = lambda t: None if t is None else t.data_ptr()
    if c.entry == "gemm":
        aux = s.aux.ptr if s.aux is not None else ptr(s.auxin_d)
        if c.ty == "f16":
            assert aux is None
            return lib.dclip_gemm_f16(s.A.data_ptr(), s.W.data_ptr(), s.C.ptr, ptr(s.bias_d), ptr(s.res_d), c.M, c.N, c.K, s.lda,
                                      s.ldw, s.ldc, c.epi, c.out16, stream)
        fn = lib.dclip_gemm_bf16_ex if c.ty == "bf16" else lib.dclip_gemm_f16_ex
        return fn(s.A.data_ptr(), s.W.data_ptr(), s.C.ptr, ptr(s.bias_d), ptr(s.res_d), aux, c.M, c.N, c.K, s.lda, s.ldw, s.ldc,
                  c.epi, c.out16, stream)
    if workspace_bytes is None:
        workspace_bytes = (s.ws_need + 64) * 4 if s.ws is not None else 0
    return getattr(lib, name)(s.A.data_ptr(), s.W.data_ptr(), s.C.ptr, c.M, c.N, c.K, s.lda, s.ldw, s.ldc, c.splits,
                              None if s.ws is None else s.ws.ptr, workspace_bytes, stream)


def emulate_gemm16(s) -> int:
    """The documented contract as plain PyTorch: 16-bit operands, fp32 accumulate, output and aux rounded with the type's rule."""
    c, ty = s.case, s.ty
    if c.entry == "tok":
        a, w = s.A[:c.K, :c.M].float().t(), s.W[:c.K, :c.N].float().t()
    else:
        a, w = s.A[:c.M, :c.K].float(), s.W[:c.N, :c.K].float()
    v = a @ w.t()
    if c.epi & EPI_BIAS:
        v = v + s.bias_d
    if c.epi & EPI_GELU:
        if s.aux is not None:
            h = round16(v, ty)
            s.aux.payload.copy_(h)
            v = h.float()                        # the activation of what was saved
        v = v * torch.sigmoid(1.702 * v)
    if c.epi & EPI_DGELU:
        x = s.auxin_d[:c.M, :c.N].float()
        sg = torch.sigmoid(1.702 * x)
        v = v * (sg * (1.0 + 1.702 * x * (1.0 - sg)))
    if c.epi & EPI_RESIDUAL:
        v = v + s.res_d[:c.M, :c.N]
    s.C.payload.copy_(round16(v, ty) if c.out16 else v)
    if s.ws is not None:
        s.ws.payload[0, :s.ws_need] = 0.0        # the slabs were written; their values are the library's own business
    return 0


def _first_diff(g, w):
    bad = (g != w).nonzero()
    i, j = (int(v) for v in bad[0])
    return f"{bad.shape[0]} elements differ, first at ({i}, {j}): got {float(g[i, j])}, want {float(w[i, j])}"


def verify_gemm16(s, what: str = None):
    """Guards; integer data: bit-exact C and aux; Gaussian data: (K + 8) 2^-24 |A||W| + u |want|; GELU / DGELU in fp64 of the
    stored aux at 1e-5 |want| (+ u |want| for a 16-bit output) per element.  Returns the figures it measured."""
    c, ty = s.case, s.ty
    what = what or case16_id(c)
    fig = {}
    s.C.assert_guards(what + " C")
    if s.aux is not None:
        s.aux.assert_guards(what + " aux")
    if s.ws is not None:
        s.ws.assert_guards(what + " workspace")
        ws = s.ws.get()[0]
        assert bool(torch.isnan(ws[s.ws_need:]).all()), f"{what}: the workspace was written behind the s_eff slabs"
        slabs = ws[:s.ws_need].view(s_eff16(c.K, c.splits), -1)         # exactly s_eff slabs, each written in full
        unused = torch.isnan(slabs).any(1).nonzero().flatten().tolist()
        assert not unused, f"{what}: slab(s) {unused} of the {slabs.shape[0]} = cdiv(K, roundup(cdiv(K, splits), 64)) were not (fully) written"
    got = s.C.get()
    assert not bool(torch.isnan(got).any()), f"{what} C: {int(torch.isnan(got).sum())} NaN (unwritten?) elements"
    u_out = ty.u if c.out16 else 0.0
    floor = out_floor(ty, bool(c.out16))
    exact = c.data != "gauss"
    lin = s.acc.double() if not exact else s.acc                  # integer data stays in fp32: exact, and half the memory
    if c.epi & EPI_BIAS:
        lin = lin + (s.bias if exact else s.bias.double())

    def linear_check(name, g, w, to16):
        """g against w = the exact linear result (int) / the fp64 one (gauss), after rounding to 16 bits when to16."""
        if exact:
            want = round16(w, ty).float() if to16 else w
            assert torch.equal(g.float(), want), f"{what} {name}: not the exact {'rounded ' if to16 else ''}integer result: " + \
                _first_diff(g.float(), want)
        else:
            assert bool(torch.isfinite(g).all()), f"{what} {name}: non-finite elements"
            b = rounding_bound(c.K, s.mag)
            b = b + (ty.u * (w.abs() + b) + F16_SUB * (ty.dtype == torch.float16) if to16 else 0.0)
            ratio = float(((g.double() - w).abs() / b).max())
            fig[name + "_bound_ratio"] = ratio
            assert ratio <= 1.0, f"{what} {name}: error is {ratio:.3g} x the derived bound (K + 8) 2^-24 |A||W|" + \
                (" + u |want|" if to16 else "")

    def activation_check(name, want64, extra=0.0, factor=1.0):
        """factor: what the sigmoid is multiplied by — a sigmoid below the smallest normal fp32 may be flushed to zero first."""
        assert bool(torch.isfinite(got).all()), f"{what} {name}: non-finite elements"
        tol = TOL_GELU * want64.abs() + extra
        tol = tol + u_out * (want64.abs() + tol) + floor * (1.0 + factor)
        ratio = float(((got.double() - want64).abs() / tol).max())
        fig[name + "_ratio"] = ratio
        assert ratio <= 1.0, f"{what} {name}: error is {ratio:.3g} x (1e-5{' + u' if c.out16 else ''}) |want|"

    if c.epi & EPI_GELU:
        if s.aux is not None:
            aux = s.aux.get()
            assert not bool(torch.isnan(aux).any()), f"{what} aux: NaN (unwritten?) elements"
            linear_check("aux", aux, lin, True)
            activation_check("gelu", quick_gelu64(aux), factor=aux.double().abs())     # of the STORED, rounded pre-activation
        elif exact:
            activation_check("gelu", quick_gelu64(lin), factor=lin.double().abs())
        else:                                                      # |gelu'| <= 1.1: the linear bound carries over
            activation_check("gelu", quick_gelu64(lin), 1.1 * rounding_bound(c.K, s.mag), factor=lin.abs())
    elif c.epi & EPI_DGELU:
        d = quick_gelu_grad64(s.aux_in)
        activation_check("dgelu", lin.double() * d, 0.0 if exact else d.abs() * rounding_bound(c.K, s.mag),
                         factor=lin.double().abs() * (1.0 + 1.702 * s.aux_in.double().abs()))
    else:
        w = lin + (s.res if exact else s.res.double()) if c.epi & EPI_RESIDUAL else lin
        linear_check("C", got, w, bool(c.out16))
    return fig


def run_gemm16_on_device(lib, c: Gemm16Case, device, stream):
    """Build, launch through the C ABI, check the variant the library reports, verify.  The caller has set gemm16_env(c)."""
    s = build_gemm16(c, device)
    rc = launch_gemm16(lib, s, stream)
    assert rc == 0, f"{case16_id(c)}: rc={rc}: {lib.dclip_last_error().decode(errors='replace')}"
    site = lib.dclip_last_launch().decode()
    torch.cuda.synchronize()
    assert site == expected_gemm16_site(c), (case16_id(c), site)
    fig = verify_gemm16(s)
    fig["site"] = site
    if gemm16_reduces(c):
        fig["s_eff"] = s_eff16(c.K, c.splits)
    return fig


# ------------------------------------------------------------------------------------------------ once-read switches

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_ENDED_ABNORMALLY = []      # one latch for the process: set by a child that ended by signal, abort, error or timeout


def assert_no_child_ended_abnormally():
    """Nothing more is started on a card after a process on it ended abnormally: no further child, no in-process case."""
    assert not CHILD_ENDED_ABNORMALLY, f"not started: an earlier child process ended abnormally ({CHILD_ENDED_ABNORMALLY[0]})"


def run_child16(what: str, setting: dict, timeout: int = 600) -> dict:
    """`python -m tests.paths16_child what` in one fresh process under a once-read switch; returns its JSON line.  A non-zero
    exit status or a timeout sets the latch and fails the caller."""
    import subprocess
    import sys
    assert_no_child_ended_abnormally()
    env = {k: v for k, v in os.environ.items() if not k.startswith(("DCLIP_BF16_", "DCLIP_ATTN16_"))}
    env.update(setting)
    try:
        r = subprocess.run([sys.executable, "-m", "tests.paths16_child", what], cwd=REPO, env=env, capture_output=True, text=True,
                           timeout=timeout)
    except subprocess.TimeoutExpired:
        CHILD_ENDED_ABNORMALLY.append(f"{setting}: timeout")
        raise AssertionError(f"{setting}: the child did not finish in {timeout} s")
    if r.returncode != 0:
        CHILD_ENDED_ABNORMALLY.append(f"{setting}: exit status {r.returncode}")
        raise AssertionError(f"{setting}: child exit status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(out)
    assert out["switches"] == setting
    return out


# ------------------------------------------------------------------------------------------------ 16-bit attention cases

Attn16Case = namedtuple("Attn16Case", "entry ty B S H causal rows")          # entry: fwd | lse | train (lse + bwd) | row
S16_FWD = [1, 2, 17, 31, 32, 33, 50, 63, 64, 65, 77, 96, 97, 128, 129, 160, 161, 192, 197, 224, 256, 257, 258, 287, 288, 289, 320, 512]
S16_BWD = [1, 2, 17, 31, 32, 33, 50, 63, 64]
S16_ROW = [1, 50, 77, 257, 300, 512]
BH16 = [(2, 2), (1, 3), (3, 1)]
ATTN16_NAMES = {"fwd": "attention_fwd_%s", "lse": "attention_fwd_%s_lse", "bwd": "attention_bwd_%s", "row": "attention_row_fwd_%s"}


def attn16_type(c) -> Type16:
    """The forward of the frozen towers is built for the saturating fp16, the training forms for the IEEE one."""
    return TYPES16["bf16" if c.ty == "bf16" else ("f16ex" if c.entry in ("lse", "train") else "f16")]


@functools.lru_cache(maxsize=None)
def attn16_cases():
    cases = []
    for ty in ("bf16", "f16"):
        for i, S in enumerate(S16_FWD):
            for causal in (False, True):
                B, H = BH16[(i + causal) % 3]
                cases.append(Attn16Case("fwd", ty, B, S, H, causal, None))
                if S != 257 and S <= (288 if ty == "bf16" else 64):
                    cases.append(Attn16Case("train" if S <= 64 else "lse", ty, B, S, H, causal, None))
        for i, S in enumerate(S16_ROW):
            rows = tuple(min(r, S - 1) for r in (0, S - 1, 63, 64, S // 2))
            cases.append(Attn16Case("row", ty, 5, S, 1 + 2 * (i % 2), True, rows))         # B H = 5 or 15: not a multiple of 4
            cases.append(Attn16Case("row", ty, 3, S, 2, False, None))                      # rows == NULL: the CLS row, all keys
    return tuple(cases)


def expected_attn16_site(c, entry=None, tiled=False, no_xq=False) -> str:
    entry = entry or c.entry
    name = ATTN16_NAMES["lse" if entry == "train" else entry] % c.ty
    if entry == "train":
        entry, name = "lse", ATTN16_NAMES["lse"] % c.ty
    if entry in ("bwd", "row"):
        return name + (".one_key" if entry == "bwd" and c.S == 1 else "")
    if entry == "fwd" and (tiled or c.S > 288):
        return name + ".tiled"
    if entry == "fwd" and c.S == 257 and not c.causal and not no_xq:
        return name + ".head_xq"
    return name + f".head{-(-c.S // 32)}"


MIN_MARGIN = 120.0       # e^-120 and 2^-173 are below the smallest fp32 subnormal (2^-149): the other probabilities are exactly 0


def _bhsd(t, B, S, H):                 # [B*S][H*64] -> [B][H][S][64]
    return t.reshape(B, S, H, HD).permute(0, 2, 1, 3)


def _rows_of(t):                       # [B][H][S][64] -> [B*S][H*64]
    B, H, S, _ = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * S, H * HD)


def selection_data(B, S, H, causal, seed):
    """Exact-selection q, k, v, dO ([B][H][S][64], fp64 holding values exact in bf16 and fp16), pi [B][H][S] and the margin.
    Keys are 8 x (+-1)^64 and q_i = k_pi(i): the matching score is 512 after the 1/8 scale.  Causal: pi(i) <= i; every
    query i = 1 mod 3 selects ITSELF and key i + 1 is a copy of key i with its own v — a mask that lets query i see key i + 1
    splits its probability in two; no other query selects i or i + 1 (they select keys j = 0 mod 3)."""
    g = torch.Generator().manual_seed(seed)
    k = 8.0 * (2.0 * torch.randint(0, 2, (B, H, S, HD), generator=g) - 1.0).double()
    idx = torch.arange(S)
    if causal:
        own = (idx % 3 == 1) & (idx + 1 < S)
        k[:, :, idx[own] + 1] = k[:, :, idx[own]]
        pick = 3 * (torch.rand((B, H, S), generator=g) * (idx // 3 + 1)).floor().long().clamp(max=(S - 1) // 3)
        pi = torch.where(own, idx, torch.minimum(pick, 3 * (idx // 3)))
    else:
        pi = torch.stack([torch.randperm(S, generator=g) for _ in range(B * H)]).view(B, H, S)
    q = torch.gather(k, 2, pi[..., None].expand(-1, -1, -1, HD))
    v = torch.randint(-2, 3, (B, H, S, HD), generator=g).double()
    do = torch.randint(-2, 3, (B, H, S, HD), generator=g).double()
    sc = q @ k.transpose(-1, -2) * 0.125
    assert bool((torch.gather(sc, 3, pi[..., None]) == 512.0).all())
    other = sc.scatter(3, pi[..., None], float("-inf"))
    if causal:
        other = other + _causal_mask(S, torch.float64, "cpu")
    margin = float((512.0 - other).min())
    return q, k, v, do, pi, margin


def build_attn16(c: Attn16Case, device="cpu", data="select", seed=0):
    """qkv / dO (16-bit, NaN rows behind them) and guarded outputs.  data: select (exact selection; refused when the margin is
    below MIN_MARGIN) | gauss (scales of the existing tests: 1.5 forward, 1.2 training, 1.0 for dO)."""
    ty = attn16_type(c)
    B, S, H = c.B, c.S, c.H
    D = H * HD
    s = SimpleNamespace(case=c, ty=ty, data=data)
    causal = c.causal if c.entry != "row" else c.rows is not None
    if data == "select":
        q, k, v, do, s.pi, s.margin = selection_data(B, S, H, causal, 7919 * seed + 31 * S + B + 2 * H + causal)
        if s.margin < MIN_MARGIN:
            raise ValueError(f"{case_id(c)}: exact-selection margin {s.margin} < {MIN_MARGIN}: case refused")
    else:
        g = torch.Generator().manual_seed(100 + seed + S)
        scale = 1.2 if c.entry == "train" else 1.5
        q, k, v = ((torch.randn((B, H, S, HD), generator=g) * scale).to(ty.dtype).double() for _ in range(3))
        do = torch.randn((B, H, S, HD), generator=g).to(ty.dtype).double()
    s.q, s.k, s.v, s.do = q, k, v, do
    qkv = torch.cat([_rows_of(q), _rows_of(k), _rows_of(v)], 1)                  # [B*S][3 D]
    s.qkv = poisoned(qkv, 3 * D, device, dtype=ty.dtype)
    if c.entry == "row":
        s.rows = None if c.rows is None else torch.tensor([c.rows[b % len(c.rows)] for b in range(B)], dtype=torch.int32, device=device)
        s.out = Guarded(B, D, device=device, dtype=ty.dtype)
        return s
    s.out = Guarded(B * S, D, device=device, dtype=ty.dtype)
    if c.entry in ("lse", "train"):
        s.lse = Guarded(1, B * H * S, device=device)
    if c.entry == "train":
        s.dout = poisoned(_rows_of(do), D, device, dtype=ty.dtype)
        s.dqkv = Guarded(B * S, 3 * D, device=device, dtype=ty.dtype)
    return s


def _attn16_mask(c, s):
    """[B][1][Sq][S] additive mask and the query rows ([B] or None = all)."""
    S = c.S
    if c.entry == "row":
        rows = torch.zeros(c.B, dtype=torch.long) if c.rows is None else s.rows.cpu().long()
        if c.rows is None:
            return torch.zeros(c.B, 1, 1, S, dtype=torch.float64), rows
        return torch.where(torch.arange(S)[None, :] <= rows[:, None], 0.0, float("-inf")).double()[:, None, None, :], rows
    return (_causal_mask(S, torch.float64, "cpu") if c.causal else torch.zeros(S, S, dtype=torch.float64))[None, None], None


def attn16_forward(s, ty=None):
    """fp64 forward on the case's q, k, v.  ty: the documented roundings (P = exp(s - max) to the type for P V, the row sum from
    the unrounded P, the output to the type).  Returns out [B][H][Sq][64], lse, P (normalised, fp64) and eps (the score error)."""
    c = s.case
    mask, rows = _attn16_mask(c, s)
    q = s.q if rows is None else s.q[torch.arange(c.B), :, rows][:, :, None, :]
    sc = q @ s.k.transpose(-1, -2) * 0.125 + mask
    m = sc.max(-1, keepdim=True).values
    p = torch.exp(sc - m)
    l = p.sum(-1, keepdim=True)
    pr = p if ty is None or c.entry == "row" else round16(p, ty).double()       # the one-row kernel keeps P in fp32
    out = (pr @ s.v) / l
    if ty is not None:
        out = round16(out, ty).double()
    eps = 72 * 2.0 ** -24 * 0.125 * (q.abs() @ s.k.abs().transpose(-1, -2)).max(-1, keepdim=True).values
    return out, (m + torch.log(l)).squeeze(-1), p / l, eps


def attn16_backward(s, out16, lse, ty=None):
    """fp64 backward from the inputs the kernel gets (q, k, v, dO, the 16-bit `out` and the fp32 `lse` of the forward):
    p = exp(s - lse), delta = rowsum(out dO), dS = p (dP - delta) / 8.  ty: P and dS rounded to the type for the products they
    feed, dq / dk / dv rounded to the type.  Returns dq, dk, dv and the magnitudes the bound needs."""
    c = s.case
    mask, _ = _attn16_mask(c, s)
    sc = s.q @ s.k.transpose(-1, -2) * 0.125 + mask
    p = torch.exp(sc - lse[..., None])
    dp = s.do @ s.v.transpose(-1, -2)
    delta = (out16 * s.do).sum(-1, keepdim=True)
    ds = p * (dp - delta) * 0.125
    pr, dsr = (p, ds) if ty is None else (round16(p, ty).double(), round16(ds, ty).double())
    dq, dk, dv = dsr @ s.k, dsr.transpose(-1, -2) @ s.q, pr.transpose(-1, -2) @ s.do
    if ty is not None:
        dq, dk, dv = (round16(t, ty).double() for t in (dq, dk, dv))
    cancel = p * 0.125 * ((s.do.abs() @ s.v.abs().transpose(-1, -2)) + (out16.abs() * s.do.abs()).sum(-1, keepdim=True))
    return dq, dk, dv, p, ds, cancel


def attn16_slack(eps, S):
    """fp32 slack, relative to each p_ij: the score's gamma_64 error enters p (and the row sum / lse) as e^(+-2 eps), plus the
    roundings of the scale FMA, exp2, the row sum (S terms), 1 / l and the fp32 accumulation of the products."""
    return 4.0 * eps + (S + 32) * 2.0 ** -24


def attn16_out_bound(s, want, p, eps, c_p):
    """|got - want| <= (c_P u + slack) sum_j p_ij |v_jd| + u |want_id| (+ the fp16 subnormal terms): DESIGN.md §17."""
    ty, sub = s.ty, F16_SUB * (s.ty.dtype == torch.float16)
    b = (c_p * ty.u + attn16_slack(eps, s.case.S)) * (p @ s.v.abs()) + c_p * sub * s.v.abs().sum(-2, keepdim=True)
    return b + ty.u * (want.abs() + b) + sub + F32_TINY


def emulate_attn16(s):
    """The documented roundings in fp64, written into the case's buffers the way the entry points write them."""
    c, ty = s.case, s.ty
    out, lse, _, _ = attn16_forward(s, ty)
    if c.entry == "row":
        s.out.payload.copy_(out[:, :, 0].reshape(c.B, -1))
        return
    s.out.payload.copy_(_rows_of(out))
    if c.entry in ("lse", "train"):
        s.lse.payload.copy_(lse.float().reshape(1, -1))
    if c.entry == "train":
        dq, dk, dv, _, _, _ = attn16_backward(s, out, lse.float().double(), ty)
        s.dqkv.payload.copy_(torch.cat([_rows_of(dq), _rows_of(dk), _rows_of(dv)], 1))


def launch_attn16(lib, s, stream):
    """The C ABI calls of a built case.  Returns the launch-site names the library reported, in call order."""
    c = s.case
    t = c.ty

    def ok(rc, what):
        assert rc == 0, f"{what}: rc={rc}: {lib.dclip_last_error().decode(errors='replace')}"
        return lib.dclip_last_launch().decode()
    ci = int(c.causal)
    if c.entry == "fwd":
        return [ok(getattr(lib, f"dclip_attention_fwd_{t}")(s.qkv.data_ptr(), s.out.ptr, c.B, c.S, c.H, ci, stream), "fwd")]
    if c.entry == "row":
        return [ok(getattr(lib, f"dclip_attention_row_fwd_{t}")(s.qkv.data_ptr(), None if s.rows is None else s.rows.data_ptr(),
                                                                s.out.ptr, c.B, c.S, c.H, stream), "row")]
    sites = [ok(getattr(lib, f"dclip_attention_fwd_{t}_lse")(s.qkv.data_ptr(), s.out.ptr, s.lse.ptr, c.B, c.S, c.H, ci, stream), "lse")]
    if c.entry == "train":
        sites.append(ok(getattr(lib, f"dclip_attention_bwd_{t}")(s.qkv.data_ptr(), s.out.ptr, s.dout.data_ptr(), s.lse.ptr,
                                                                 s.dqkv.ptr, c.B, c.S, c.H, ci, stream), "bwd"))
    return sites


def _exact(name, got, want, what, failed):
    if bool(torch.isnan(got).any()):
        failed.append(f"{name}: {int(torch.isnan(got).sum())} NaN (unwritten?) elements")
    elif not torch.equal(got.double(), want.double()):
        failed.append(f"{name}: not bit-exact: " + _first_diff(got.double().reshape(-1, got.shape[-1]),
                                                              want.double().reshape(-1, want.shape[-1])))


def verify_attn16(s, what: str = None):
    """Guards of every output; exact-selection data: out == v[pi], lse == 512 (1e-5), dV == the rounded integer sum, dQ = dK = 0,
    all bit for bit; Gaussian data: the derived per-element bounds, per block.  Returns the worst got / bound ratio per block."""
    c, ty = s.case, s.ty
    what = what or case_id(c)
    B, S, H = c.B, c.S, c.H
    D = H * HD
    for name in ("out", "lse", "dqkv"):
        if hasattr(s, name):
            getattr(s, name).assert_guards(f"{what} {name}")
    c_p = 0.0 if c.entry == "row" else 1.0           # the one-row kernel keeps P in fp32
    want, lse_w, p, eps = attn16_forward(s)
    got_rows = s.out.get()
    got = got_rows.double().reshape(B, 1, H, HD).permute(0, 2, 1, 3) if c.entry == "row" else _bhsd(got_rows.double(), B, S, H)
    fig, failed = {}, []

    def bounded(name, g, w, b):
        if not bool(torch.isfinite(g).all()):
            fig[name] = NAN
            failed.append(f"{name}: {int((~torch.isfinite(g)).sum())} non-finite (unwritten?) elements")
        elif float(w.abs().max()) == 0.0:
            fig[name] = float(g.abs().max())
            if fig[name] != 0.0:
                failed.append(f"{name}: reference is identically zero, got max |x| = {fig[name]:.3e}")
        else:
            fig[name] = float(((g - w).abs() / b).max())
            if not fig[name] <= 1.0:
                failed.append(f"{name}: error is {fig[name]:.3g} x the derived bound")

    if s.data == "select":
        _, rows = _attn16_mask(c, s)
        pi = s.pi if rows is None else s.pi[torch.arange(B), :, rows][:, :, None]
        _exact("out", got, torch.gather(s.v, 2, pi[..., None].expand(-1, -1, -1, HD)), what, failed)
    else:
        bounded("out", got, want, attn16_out_bound(s, want, p, eps, c_p))
    if hasattr(s, "lse"):
        lse_g = s.lse.get().double().reshape(B, H, S)
        if not bool(torch.isfinite(lse_g).all()):
            failed.append("lse: non-finite (unwritten?) elements")
        else:
            fig["lse"] = float(((lse_g - lse_w).abs() / (TOL_LSE * lse_w.abs() + F32_TINY)).max()) if s.data == "select" \
                else relerr(lse_g, lse_w) / TOL_LSE
            if not fig["lse"] <= 1.0:
                failed.append(f"lse: error is {fig['lse']:.3g} x 1e-5")
    if hasattr(s, "dqkv") and not failed:
        d = s.dqkv.get().double()
        gq, gk, gv = (_bhsd(d[:, i * D:(i + 1) * D], B, S, H) for i in range(3))
        if s.data == "select":
            onehot = torch.zeros(B, H, S, S, dtype=torch.float64).scatter_(3, s.pi[..., None], 1.0)
            dv = onehot.transpose(-1, -2) @ s.do                               # integer sums below 2^8 S
            _exact("dv", gv, round16(dv, ty), what, failed)
            _exact("dq", gq, torch.zeros_like(gq), what, failed)
            _exact("dk", gk, torch.zeros_like(gk), what, failed)
        else:
            lse_in = s.lse.get().double().reshape(B, H, S)
            wq, wk, wv, pb, ds, cancel = attn16_backward(s, got, lse_in)
            u, sub, sl = ty.u, F16_SUB * (ty.dtype == torch.float16), attn16_slack(eps, S)
            e = (u + sl) * ds.abs() + 72 * 2.0 ** -24 * cancel                 # |dS_got - dS| per pair
            for name, g, w, b in (("dq", gq, wq, e @ s.k.abs() + sub * s.k.abs().sum(-2, keepdim=True)),
                                  ("dk", gk, wk, e.transpose(-1, -2) @ s.q.abs() + sub * s.q.abs().sum(-2, keepdim=True)),
                                  ("dv", gv, wv, ((u + sl) * pb).transpose(-1, -2) @ s.do.abs() + sub * s.do.abs().sum(-2, keepdim=True))):
                bounded(name, g, w, b + u * (w.abs() + b) + sub + F32_TINY)
    assert not failed, f"{what}: " + "; ".join(failed) + f"   (figures: {fig})"
    return fig


# ------------------------------------------------------------------------------------------------ cast and LayerNorm-16

CAST_SHAPES = [(1, 5, 8, 8), (3, 7, 8, 12), (5, 13, 16, 16), (17, 100, 104, 100), (4, 64, 64, 72), (33, 770, 772, 776),
               (12800, 768, 768, 768)]                                         # (rows, cols, ldx, ldy)
CAST_SPECIALS = [65504.0, -65504.0, 65520.0, -65520.0, 65519.0, 1e6, -1e6, float("inf"), float("-inf"), NAN, 2.0 ** -24, -2.0 ** -24,
                 2.0 ** -25, 3 * 2.0 ** -25, 6e-8, 1e-40, -1e-40, 2.0 ** -133, 0.0, -0.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8,
                 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 3.3895314e38]
LN16_D = [4, 100, 256, 260, 512, 516, 768, 772, 1024, 1028, 1280, 1536, 2048]
LN16_ROWS = [1, 3, 4, 5, 1001]
TOL_LN = 1e-5                    # the fp32 figure of the LayerNorm tests (tests/test_ops_gpu.py)


def cast_input(rows, cols, seed=0):
    x = torch.randn((rows, cols), generator=torch.Generator().manual_seed(seed + rows + cols)) * 100.0
    sp = torch.tensor(CAST_SPECIALS)
    flat = x.view(-1)
    n = min(flat.numel(), sp.numel())
    flat[:n] = sp[:n]
    if flat.numel() > 4 * sp.numel():
        flat[-sp.numel():] = sp                                                # and in the last rows
    return x


def expected_ln16_variant(D: int) -> str:
    if D in (512, 768, 1024):
        return f".nc{D // 256}.exact"
    nc = -(-(D // 4) // 64)
    return f".nc{nc if nc <= 4 else 8}"


def ln16_reference(x, g, b, eps):
    x = x.double()
    mu = x.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mu) ** 2).mean(1, keepdim=True) + eps)
    return (x - mu) * rstd * g.double() + b.double(), mu.squeeze(1), rstd.squeeze(1)


def verify_ln16(y, mean, rstd, x, g, b, eps, ty, what):
    """y (16-bit) against fp64 under u |want| + 1e-5 max|want| per element; mean and rstd at the fp32 figure."""
    want, mu, rs = ln16_reference(x, g, b, eps)
    assert bool(torch.isfinite(y.float()).all()), f"{what}: non-finite (unwritten?) elements"
    tol = ty.u * want.abs() + TOL_LN * float(want.abs().max()) + out_floor(ty, True)
    ratio = float(((y.double() - want).abs() / tol).max())
    assert ratio <= 1.0, f"{what}: error is {ratio:.3g} x (u |want| + 1e-5 max|want|)"
    fig = {"y_ratio": ratio}
    if mean is not None:
        fig.update(check_blocks({"mean": (mean, mu, TOL_LN), "rstd": (rstd, rs, TOL_LN)}, what))
    return fig
