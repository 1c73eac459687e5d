"""The frozen-tower kernels at config c5's own size: M = 4096 crops x 257 tokens = 1,052,672 rows at ViT-L/14's
widths on the 16-bit route, M = 526,336 on the fp32 and split-fp16 routes — tensors beyond 2^31 and 2^32 elements and bytes, where
a 32-bit product in a store offset, an lse index, a buffer offset or a wrapper's size would read or write the wrong rows without
any small-shape test noticing.  Kernel level: one launch per case through the C ABI, the launch name asserted, then check A (block
0 through the entry's existing checker and gate), check B (every period equals block 0 bit for bit) and check C (guards intact, no
NaN left).  Engine level: a two-layer ViT-L/14 tower over all crops in one pass, in every frozen precision, and the text tower.
Construction and checkers: tests/kernel_checks_large.py; tests/test_kernel_checks_large_cpu.py shows what they catch."""
import dataclasses
import time
from types import SimpleNamespace

import pytest
import torch

from tests import kernel_checks as kc
from tests import kernel_checks_f16x3 as kx
from tests import kernel_checks_large as kl
from tests import kernel_checks_rest as kr
from tests import kernel_checks_split16 as ks

pytestmark = pytest.mark.gpu

P, M16, M32, MP, PP = kl.PERIOD_ROWS, kl.M16, kl.M32, kl.MP, kl.PP
D, D3, DI, H, S = kl.D, kl.D3, kl.DI, kl.H, kl.SEQ
SKIPPED, FIGURES = [], []
SWITCHES = kc.GEMM16_SWITCHES + kc.ATTN_SWITCHES + ("DCLIP_GEMM_TILE", "DCLIP_GEMM_PLAN_TABLE", "DCLIP_F16X3_BM192", "DCLIP_F16X3_BM192_MIN",
                                                    "DCLIP_F16X3_MIN")


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


@pytest.fixture(autouse=True)
def _default_dispatch_and_figures(request, monkeypatch):
    """Every case runs the dispatch a tower gets (no tuning switch set), frees what it allocated and leaves its time and peak."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    fig = {"case": request.node.name, "seconds": round(time.perf_counter() - t0, 2), "peak_bytes": torch.cuda.max_memory_allocated()}
    FIGURES.append(fig)
    print(f"\n[large] {fig['case']}: {fig['seconds']} s, peak {fig['peak_bytes'] / kl.GIB:.2f} GiB")
    kc.record("large", (request.node.name,), fig)
    torch.cuda.empty_cache()


def need(name):
    """The case's declared budget against the free memory: skip, naming the shortfall (none on an otherwise idle MI355X)."""
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    short = kl.shortfall(name, free)
    if short:
        SKIPPED.append(name)
        pytest.skip(f"{name}: declared peak {kl.peak_bytes(name)} bytes, {short} more than the {free} free")


def launched(lib, rc, site, what):
    assert rc == 0, f"{what}: rc={rc}: {lib.dclip_last_error().decode(errors='replace')}"
    got = lib.dclip_last_launch().decode()
    torch.cuda.synchronize()
    assert got == site, (what, got, site)


def tile(t, rows, dev, period=P):
    """A builder's operand (NaN padding columns included) laid down over `rows` rows."""
    return kl.tile_rows(t[:period], rows, device=dev)


# ==================================================================================================== 16-bit route, M = 1,052,672

LN16_FN = {"bf16": "layernorm_fwd_bf16", "f16": "layernorm_fwd_f16"}


@pytest.fixture(scope="module")
def ln_block():
    ln = kr.build_ln_fwd(kr.LnFwdCase(D, P, True))           # x (a row with mean 100 x its spread), gamma, beta: §18's data
    kl.assert_rows_distinct(ln.x, "LayerNorm input")
    return ln


@pytest.mark.parametrize("ty", ["bf16", "f16"])
def test_layernorm16(dev, lib, ln_block, ty):
    need("ln16")
    t, ln = kc.TYPES16[ty], ln_block
    x = tile(ln.x, M16, dev)
    y = kl.LargeGuarded(M16, D, device=dev, dtype=t.dtype)
    g, b = ln.g.to(dev), ln.b.to(dev)
    rc = getattr(lib, "dclip_" + LN16_FN[ty])(x.data_ptr(), g.data_ptr(), b.data_ptr(), y.ptr, M16, D, kr.LN_EPS, stream())
    launched(lib, rc, LN16_FN[ty] + ".nc4.exact", "layernorm16")
    kc.verify_ln16(y.block(), None, None, ln.x, ln.g, ln.b, kr.LN_EPS, t, f"layernorm16 {ty} block 0")
    kl.assert_large(y, P, f"layernorm16 {ty}")


@pytest.mark.parametrize("ty", ["bf16", "f16"])
def test_cast(dev, lib, ty):
    need("cast")
    t = kc.TYPES16[ty]
    x0 = kc.cast_input(P, D)                                 # +-65504, +-65520, +-inf, NaN, subnormals in the first and last rows
    x = tile(x0, M16, dev)
    y = kl.LargeGuarded(M16, D, device=dev, dtype=t.dtype)
    fn = {"bf16": lib.dclip_cast_f32_bf16, "f16": lib.dclip_cast_f32_f16}[ty]
    launched(lib, fn(x.data_ptr(), y.ptr, M16, D, D, D, stream()), "cast_f32_" + ty, "cast")
    got, want = y.block(), kc.round16(x0, t)                 # tests/test_gemm16_paths_gpu.py's statement of the cast
    assert torch.equal(torch.isnan(got), torch.isnan(want)), "NaN must stay NaN, and nothing else may become one"
    g, w = torch.nan_to_num(got.float(), nan=0.0).to(t.dtype), torch.nan_to_num(want.float(), nan=0.0).to(t.dtype)
    assert torch.equal(g.view(torch.int16), w.view(torch.int16)), kc._first_diff(g.float(), w.float())
    kl.assert_large(y, P, f"cast {ty}", nan_ok=True)         # the input holds NaN: it must come out as NaN, period by period


# (name, N, K, epilogue, 16-bit output, the kernel the dispatcher's documented rule picks)
GEMM16 = {"qkv": (D3, D, kc.EPI_BIAS, 1, "pp"), "out_proj": (D, D, kc.EPI_BIAS | kc.EPI_RESIDUAL, 0, "pp"),
          "fc1": (DI, D, kc.EPI_BIAS | kc.EPI_GELU, 1, "pp"), "fc2": (D, DI, kc.EPI_BIAS | kc.EPI_RESIDUAL, 0, "pp"),
          "patch_gemm": (D, kl.PATCH_DIM, 0, 0, "r128")}


@pytest.mark.parametrize("ty", ["bf16", "f16"])
@pytest.mark.parametrize("name", list(GEMM16))
def test_gemm16(dev, lib, name, ty):
    """Integer operands: block 0 is the exact result (or its rounding), whatever the tile or the order."""
    need(name)
    N, K, epi, out16, want = GEMM16[name]
    patch = name == "patch_gemm"
    M, period = (MP, PP) if patch else (M16, P)
    if want == "pp":
        assert K % 64 == 0 and -(-M // 256) * -(-N // 256) >= 128                  # the ping-pong kernel's documented condition
    else:
        assert K % 64 != 0 and -(-M // 128) * -(-N // 128) >= 256
    c = kc.Gemm16Case("gemm", ty, period, N, K, epi, out16, 0, (0, 0, kl.LDC_PATCH - N if patch else 0), 1, (), want, "int")
    s = kc.build_gemm16(c)                                   # on the host: operands, bias, residual, the small guarded C
    kl.assert_rows_distinct(s.A[:period, :K], f"{name} A")
    A, W = tile(s.A, M, dev, period), s.W.to(dev)
    res = None if s.res_d is None else tile(s.res_d, M, dev, period)
    C = kl.LargeGuarded(M, N, s.ldc, device=dev, dtype=s.ty.dtype if out16 else torch.float32)
    fn = lib.dclip_gemm_bf16 if ty == "bf16" else lib.dclip_gemm_f16
    bias = None if s.bias is None else s.bias.to(dev)
    rc = fn(A.data_ptr(), W.data_ptr(), C.ptr, None if bias is None else bias.data_ptr(), None if res is None else res.data_ptr(),
            M, N, K, s.lda, s.ldw, s.ldc, epi, out16, stream())
    launched(lib, rc, kc.expected_gemm16_site(c), name)
    s.C.payload.copy_(C.block(period))
    fig = kc.verify_gemm16(s, f"{name} {ty} block 0")
    kl.assert_large(C, period, f"{name} {ty}")
    kc.record("large_gemm16", c, fig)


@pytest.fixture(scope="module")
def attn_block():
    """64 crops x 16 heads x 257 tokens of exact-selection data (one-hot P: out == v[pi] bit for bit), made once for both types."""
    s = kc.build_attn16(kc.Attn16Case("fwd", "bf16", kl.PERIOD_CROPS, S, H, False, None))
    kl.assert_rows_distinct(s.qkv[:P], "attention qkv")
    return s


def attn_state(blk, entry, ty):
    c = kc.Attn16Case(entry, ty, kl.PERIOD_CROPS, S, H, False, None)
    t = kc.attn16_type(c)                                    # (a SimpleNamespace copy: the data is the block's, the type the case's)
    s = type(blk)(**{**vars(blk), "case": c, "ty": t, "qkv": blk.qkv.to(t.dtype)})
    s.out = kc.Guarded(kl.PERIOD_CROPS if entry == "row" else P, D, dtype=t.dtype)
    if entry == "row":
        s.rows = None
    return s


@pytest.mark.parametrize("ty", ["bf16", "f16"])
def test_attention16_and_its_one_row_form(dev, lib, attn_block, ty):
    """attention_fwd_* over 4096 x 16 heads, then attention_row_fwd_* (the CLS row of every crop, the last crops included) on the
    same q | k | v: two launches, each asserted and checked."""
    need("attention")
    s = attn_state(attn_block, "fwd", ty)
    qkv = tile(s.qkv, M16, dev)
    out = kl.LargeGuarded(M16, D, device=dev, dtype=s.ty.dtype)
    rc = getattr(lib, f"dclip_attention_fwd_{ty}")(qkv.data_ptr(), out.ptr, kl.CROPS16, S, H, 0, stream())
    launched(lib, rc, kc.expected_attn16_site(s.case), "attention_fwd")
    assert kc.expected_attn16_site(s.case).endswith(".head_xq")
    s.out.payload.copy_(out.block())
    kc.verify_attn16(s, f"attention_fwd_{ty} block 0")
    kl.assert_large(out, P, f"attention_fwd_{ty}")
    del out
    r = attn_state(attn_block, "row", ty)
    row = kl.LargeGuarded(kl.CROPS16, D, device=dev, dtype=r.ty.dtype)
    rc = getattr(lib, f"dclip_attention_row_fwd_{ty}")(qkv.data_ptr(), None, row.ptr, kl.CROPS16, S, H, stream())
    launched(lib, rc, kc.expected_attn16_site(r.case), "attention_row_fwd")
    r.out.payload.copy_(row.block(kl.PERIOD_CROPS))
    kc.verify_attn16(r, f"attention_row_fwd_{ty} block 0")
    kl.assert_large(row, kl.PERIOD_CROPS, f"attention_row_fwd_{ty}")


@pytest.mark.parametrize("idx", [False, True], ids=["cls", "idx"])
def test_gather_rows(dev, lib, idx):
    """Row 0 (idx NULL) or row idx[b] of every crop of the fp32 residual stream, the last crops at byte offsets beyond 2^32."""
    need("gather_rows")
    s = kr.build_rows(kr.RowsCase(kl.PERIOD_CROPS, S, D, idx))
    kl.assert_rows_distinct(s.x, "gather_rows x")
    x = tile(s.xd, M16, dev)
    ids = s.idx.repeat(kl.CROPS16 // kl.PERIOD_CROPS).to(dev)
    out = kl.LargeGuarded(kl.CROPS16, D, device=dev)
    rc = lib.dclip_gather_rows(x.data_ptr(), ids.data_ptr() if idx else None, out.ptr, kl.CROPS16, S, D, stream())
    launched(lib, rc, "gather_rows", "gather_rows")
    s.out.payload.copy_(out.block(kl.PERIOD_CROPS))
    s.dx.payload.view(torch.int32).copy_(kr.rows_want(s)[1].view(torch.int32))      # (scatter_rows, the checker's other half, is not launched)
    kr.verify_rows(s, "gather_rows block 0")
    kl.assert_large(out, kl.PERIOD_CROPS, "gather_rows", nan_ok=True)              # random bit patterns: NaNs are data here


def test_im2col(dev, lib):
    """ViT-L/14's patch 14 is no multiple of 4: the fp32 scalar kernel (the 16-bit towers cast its output)."""
    need("im2col")
    c = kr.Im2colCase("f32", kl.PERIOD_CROPS, 3, 224, kl.PATCH, 0, False)
    s = kr.build_im2col(c)
    pix = tile(s.pixd, kl.CROPS16 * 3 * 224, dev, kl.PERIOD_CROPS * 3 * 224)
    cols = kl.LargeGuarded(MP, kl.PATCH_DIM, device=dev)
    kl.assert_period_breaks_wraps(PP * kl.PATCH_DIM, 4, "im2col cols")
    launched(lib, lib.dclip_im2col(pix.data_ptr(), cols.ptr, kl.CROPS16, 3, 224, 224, kl.PATCH, stream()), "im2col.scalar", "im2col")
    s.cols.payload.copy_(cols.block(PP))
    kr.verify_im2col(s, "im2col block 0")
    kl.assert_large(cols, PP, "im2col", nan_ok=True)                               # random bit patterns


def test_vision_assemble(dev, lib):
    """The entry takes no leading dimension and 256 patch rows a crop make every whole number of crops a power-of-two period of
    its input: the block is 61 crops, cut short at the end (4096 = 67 x 61 + 9)."""
    need("assemble")
    n = kl.ASSEMBLE_CROPS
    s = kr.build_assemble(kr.AssembleCase(n, S, D))
    kl.assert_rows_distinct(s.patch, "patch embeddings")
    patch = tile(s.patchd, MP, dev, n * kl.GRID2)
    x = kl.LargeGuarded(M16, D, device=dev)
    cls, pos = s.clsd.to(dev), s.posd.to(dev)
    rc = lib.dclip_vision_assemble_fwd(patch.data_ptr(), cls.data_ptr(), pos.data_ptr(), x.ptr, kl.CROPS16, S, D, stream())
    launched(lib, rc, "vision_assemble_fwd", "vision_assemble_fwd")
    s.x.payload.copy_(x.block(n * S))
    s.dpatch.payload.view(torch.int32).copy_(kr.assemble_want(s)[1].contiguous().view(torch.int32))   # (the backward is not launched)
    kr.verify_assemble(s, "vision_assemble_fwd block 0")
    kl.assert_large(x, n * S, "vision_assemble_fwd")


# ==================================================================================================== fp32 route, M = 526,336

def test_layernorm_f32(dev, lib, ln_block):
    need("ln32")
    ln = ln_block
    x = tile(ln.x, M32, dev)
    y = kl.LargeGuarded(M32, D, device=dev)
    mean, rstd = kl.LargeGuarded(M32, 1, device=dev), kl.LargeGuarded(M32, 1, device=dev)
    g, b = ln.g.to(dev), ln.b.to(dev)
    rc = lib.dclip_layernorm_fwd(x.data_ptr(), g.data_ptr(), b.data_ptr(), y.ptr, mean.ptr, rstd.ptr, M32, D, kr.LN_EPS, stream())
    launched(lib, rc, "layernorm_fwd.nc4.exact", "layernorm_fwd")
    ln.y.payload.copy_(y.block())
    ln.mean.payload.copy_(mean.block().t())
    ln.rstd.payload.copy_(rstd.block().t())
    kr.verify_ln_fwd(ln, "layernorm_fwd block 0")
    for out, what in ((y, "y"), (mean, "mean"), (rstd, "rstd")):
        kl.assert_large(out, P, "layernorm_fwd " + what)


def build_gemm_f32(c):
    """kernel_checks.build_gemm with the exact accumulator taken from the fp32 product: every partial sum of these integers is
    below 2^24 in any order (the module's own statement), so it is the int64 matmul's value, which at 16,448 x 4096 x 1024 would
    take the host minutes."""
    def operands(M, N, K, data):
        gen = torch.Generator().manual_seed(1000003 * M + 1009 * N + K)
        a = torch.randint(-2, 3, (M, K), generator=gen).float()
        b = torch.randint(-2, 3, (N, K), generator=gen).float()
        assert data == "int" and 4 * K < 2 ** 24
        return a, b, (a @ b.t()).double(), None
    keep, kc._operands = kc._operands, operands
    try:
        return kc.build_gemm(c)
    finally:
        kc._operands = keep


@pytest.mark.parametrize("name,N,epi", [("gemm32_qkv", D3, kc.EPI_BIAS), ("gemm32_fc1", DI, kc.EPI_BIAS | kc.EPI_GELU)])
def test_gemm_f32(dev, lib, name, N, epi):
    """The fp32 GEMM under its own plan (no tile forced), integer operands; with GELU the stored pre-activation is an output too."""
    need(name)
    c = kc.GemmCase(P, N, D, kc.A_KMAJOR | kc.B_KMAJOR, None, 0, epi, 1.0, (0, 0, 0), "int", None)
    s = build_gemm_f32(c)
    kl.assert_rows_distinct(s.A[:P], f"{name} A")
    A, B = tile(s.A, M32, dev), s.B.to(dev)
    C = kl.LargeGuarded(M32, N, device=dev)
    aux = kl.LargeGuarded(M32, N, device=dev) if epi & kc.EPI_GELU else None
    big = c._replace(M=M32)
    plan = kc.gemm_plan(lib, big)
    assert plan[2] == 1, plan                                # a tower-sized M is never split along K
    ws = torch.empty((4,), device=dev)
    bias = s.bias.to(dev)
    rc = lib.dclip_gemm_f32(A.data_ptr(), B.data_ptr(), C.ptr, bias.data_ptr(), None, None if aux is None else aux.ptr, M32, N, D, s.lda,
                            s.ldb, s.ldc, c.layout, epi, 1.0, 0, ws.data_ptr(), 0, stream())
    launched(lib, rc, kc.expected_gemm_site(big, plan), name)
    s.C.payload.copy_(C.block())
    if aux is not None:
        s.aux.payload.copy_(aux.block())
    kc.verify_gemm(s, f"{name} block 0")
    kl.assert_large(C, P, name)
    if aux is not None:
        kl.assert_large(aux, P, name + " aux")


@pytest.fixture(scope="module")
def attn32_block():
    qkv = kc._gauss((P, 3 * D), 1, 1.5)                      # kernel_checks.build_attn's data
    kl.assert_rows_distinct(qkv, "fp32 qkv")
    q, k, v = (qkv.double().view(kl.PERIOD_CROPS, S, 3, H, kc.HD)[:, :, i] for i in range(3))
    out, lse, _, _, _ = kc.attention_math(q, k, v, None)
    cls_out, cls_lse, _, _, _ = kc.attention_math(q[:, :1], k, v, None)
    return qkv, out.reshape(P, D), lse, cls_out.reshape(kl.PERIOD_CROPS, D), cls_lse.reshape(kl.PERIOD_CROPS, H)


def test_attention_f32_and_cls(dev, lib, attn32_block):
    """attention_fwd at S = 257 (the streamed kernel; lse [B][H][S]) and attention_cls_fwd (lse [B][H]) on the same q | k | v,
    against fp64 at the gates of tests/test_attention_paths_gpu.py."""
    need("attention32")
    qkv0, want, want_lse, want_cls, want_cls_lse = attn32_block
    qkv = tile(qkv0, M32, dev)
    out = kl.LargeGuarded(M32, D, device=dev)
    lse = kl.LargeGuarded(kl.CROPS32, H * S, device=dev)
    rc = lib.dclip_attention_fwd(qkv.data_ptr(), out.ptr, lse.ptr, kl.CROPS32, S, H, 0, stream())
    launched(lib, rc, kc.expected_launches(kc.SelfCase(kl.CROPS32, S, H, False, "default"))[0], "attention_fwd")
    kc.check_blocks({"out": (out.block(), want, kc.TOL_ATTN_FWD),
                     "lse": (lse.block(kl.PERIOD_CROPS).reshape(kl.PERIOD_CROPS, H, S), want_lse, kc.TOL_LSE)}, "attention_fwd block 0")
    kl.assert_large(out, P, "attention_fwd out")
    kl.assert_large(lse, kl.PERIOD_CROPS, "attention_fwd lse")
    del out, lse
    out = kl.LargeGuarded(kl.CROPS32, D, device=dev)
    lse = kl.LargeGuarded(kl.CROPS32, H, device=dev)
    rc = lib.dclip_attention_cls_fwd(qkv.data_ptr(), out.ptr, lse.ptr, kl.CROPS32, S, H, stream())
    launched(lib, rc, kc.expected_launches(kc.ClsCase(kl.CROPS32, S, H))[0], "attention_cls_fwd")
    kc.check_blocks({"out": (out.block(kl.PERIOD_CROPS), want_cls, kc.TOL_ATTN_FWD),
                     "lse": (lse.block(kl.PERIOD_CROPS), want_cls_lse, kc.TOL_LSE)}, "attention_cls_fwd block 0")
    kl.assert_large(out, kl.PERIOD_CROPS, "attention_cls_fwd out")
    kl.assert_large(lse, kl.PERIOD_CROPS, "attention_cls_fwd lse")


# ==================================================================================================== split-fp16 route, M = 526,336

def test_layernorm_f16x2(dev, lib, ln_block):
    """The frozen split tower's LayerNorm: y = [hi | lo] of scale * LN(x), two pieces; equal to the host split of the fp32
    LayerNorm (§25's statement), which §18's bound ties to fp64."""
    need("ln_f16x2")
    ln, sexp = ln_block, 3
    x = tile(ln.x, M32, dev)
    y = kl.LargeGuarded(M32, 2 * D, device=dev, dtype=torch.float16)
    y32 = kl.LargeGuarded(M32, D, device=dev)
    g, b = ln.g.to(dev), ln.b.to(dev)
    rc = lib.dclip_layernorm_fwd_f16x2(x.data_ptr(), g.data_ptr(), b.data_ptr(), y.ptr, y32.ptr, None, None, M32, D, kr.LN_EPS,
                                       2.0 ** sexp, None, stream())
    launched(lib, rc, "layernorm_fwd_f16x3.nc4.exact", "layernorm_fwd_f16x2")     # recorded under the three-piece twin's name
    ln.y.payload.copy_(y32.block())
    ln.mean.payload.fill_(kc.NAN)
    ln.rstd.payload.fill_(kc.NAN)
    st = ln.case
    ln.case = st._replace(stats=False)
    try:
        kr.verify_ln_fwd(ln, "layernorm_fwd_f16x2 y32 block 0")
    finally:
        ln.case = st
    hi, lo = ks.host_split(y32.block(), 2.0 ** sexp)
    rep = kr.Report("layernorm_fwd_f16x2 block 0")
    ks.check_pieces(rep, "y", y.block(), torch.cat([hi, lo], 1))
    rep.done()
    kl.assert_large(y, P, "layernorm_fwd_f16x2 y")
    kl.assert_large(y32, P, "layernorm_fwd_f16x2 y32")


def test_split_f32_f16x2(dev, lib):
    """The activation split pass at the fc1 width: [M][4096] fp32 (beyond 2^31 elements) -> [hi | lo] fp16."""
    need("split_f16x2")
    c = ks.SplitCase(P, DI, 0, 0, 0, False, 3)
    x0 = ks.split_data(c)
    kl.assert_rows_distinct(x0, "split input")
    x = tile(x0, M32, dev)
    y = kl.LargeGuarded(M32, 2 * DI, device=dev, dtype=torch.float16)
    rc = lib.dclip_split_f32_f16x2(x.data_ptr(), y.ptr, M32, DI, DI, 2 * DI, 2.0 ** c.sexp, None, stream())
    launched(lib, rc, "split_f32_f16x3.act", "split_f32_f16x2")                   # recorded under the three-piece twin's name
    hi, lo = ks.host_split(x0, 2.0 ** c.sexp)
    rep = kr.Report("split_f32_f16x2 block 0")
    got = y.block()
    ks.check_pieces(rep, "y", got, torch.cat([hi, lo], 1))
    ks.check_recon(rep, "hi+lo", got[:, :DI], got[:, DI:], x0.double() * 2.0 ** c.sexp)
    rep.done()
    kl.assert_large(y, P, "split_f32_f16x2", nan_ok=True)    # the data holds the specials of §25, NaN among them


def x3_tile_rows(M, N, has192):
    """DESIGN.md §9i's rule for the tile height of a fused call."""
    t256, t192 = -(-M // 256) * -(-N // 256), -(-M // 192) * -(-N // 256)
    if not has192 or t256 < 128:
        return 256
    return 192 if -(-t192 // 256) * 91 < -(-t256 // 256) * 100 else 256


def build_x3_block(c):
    """kernel_checks_f16x3.build_x3 for the two forms used here (no row scales, no DGELU), the same seeds and data, with the three
    products taken as ONE fp32 matmul of [hi|lo|hi] with [hi|hi|lo]: sums of at most 3 K products of integers in [-2, 2] are exact
    in fp32 in any order, and three fp64 matmuls of 16,448 x 4096 x 4096 take the host ten seconds."""
    f = kx.x3_form(c)
    assert not (f.big or f.negzero or f.noscale or f.g32 or f.h32) and f.fn in ("scaled", "split")
    M, N, K = c.M, c.N, c.K
    seed = 1000 * M + 10 * N + K
    ah, al, wh, wl = (kr.ints(sh, seed + 10 + i) for i, sh in enumerate([(M, K), (M, K), (N, K), (N, K)]))
    bias = torch.randint(-4096, 4097, (N,), generator=kr.gen(seed + 2)).float() * 2.0 ** -12
    alpha = 2.0 ** ks.GEMM_ALPHA_EXP
    a, w = torch.cat([ah, al, ah], 1), torch.cat([wh, wh, wl], 1)
    assert 4 * 3 * K < 2 ** 24
    res = kr.ints((M, N), seed + 3)
    lin = (a @ w.t()).double() * alpha
    if f.epi & ks.EPI_BIAS:
        lin = lin + bias.double()
    if f.epi & ks.EPI_RESIDUAL:
        lin = lin + res.double()
    assert torch.equal(lin.float().double(), lin)
    lda = ldw = 3 * K + 8
    ldc = kc.roundup(3 * N, 8) if f.split else N
    offs = kx.x3_offsets(c)
    return SimpleNamespace(case=c, form=f, a=a, w=w, pieces=(ah, al, wh, wl), offs=offs, bias=bias, res=res, lin=lin, want=lin, epi=f.epi,
                           lda=lda, ldw=ldw, ldc=ldc, alpha_v=alpha, aux=None, ra=torch.ones(M),
                           A=kc.poisoned(kx._place((ah, al), offs[:2], K, M), lda, dtype=torch.float16),
                           W=kc.poisoned(kx._place((wh, wl), offs[2:], K, N), ldw, dtype=torch.float16),
                           bias_d=torch.cat([bias, torch.full((8,), kc.NAN)]),
                           res_d=kc.poisoned(res, ldc) if f.epi & ks.EPI_RESIDUAL else None, aux_d=None,
                           ra_d=kr.vec(M, fill=1.0), alpha=kr.vec(1, fill=alpha), out_scale=kr.vec(1, fill=2.0 ** ks.GEMM_OUT_EXP),
                           C=kc.Guarded(M, 3 * N if f.split else N, ldc, dtype=torch.float16 if f.split else torch.float32),
                           g32=None, h32=None, pmax=None, psum=None)


@pytest.mark.parametrize("name,entry,N,K", [("f16x3_fc1", "split_gelu", DI, D), ("f16x3_fc2", "scaled", D, DI)])
def test_gemm_f16x3(dev, lib, name, entry, N, K):
    """The fused split-fp16 forward entries at the fc1 (bias + GELU, split output) and fc2 (bias + residual, fp32) shapes: four
    independent integer pieces, block 0 exact (kernel_checks_f16x3)."""
    need(name)
    c = kx.X3Case(entry, P, N, K, 0, False)
    s = build_x3_block(c)
    kl.assert_rows_distinct(s.A[:P, :2 * K], f"{name} A")
    A, W = tile(s.A, M32, dev), s.W.to(dev)
    res = None if s.res_d is None else tile(s.res_d, M32, dev)
    C = kl.LargeGuarded(M32, s.C.cols, s.ldc, device=dev, dtype=s.C.dtype)
    dims = (M32, N, K, s.lda, s.ldw, s.ldc, *s.offs)
    bias = s.bias_d.to(dev)
    if entry == "scaled":
        rc = lib.dclip_gemm_f16x3_scaled(A.data_ptr(), W.data_ptr(), C.ptr, bias.data_ptr(), res.data_ptr(), *dims, s.epi, 0, s.alpha_v,
                                         stream())
        site = "gemm_f16x3_scaled" + (".pp3_192" if x3_tile_rows(M32, N, True) == 192 else ".pp3")
    else:
        rc = lib.dclip_gemm_f16x3_scaled_split(A.data_ptr(), W.data_ptr(), C.ptr, bias.data_ptr(), *dims, s.epi, s.alpha_v,
                                               2.0 ** ks.GEMM_OUT_EXP, stream())
        site = "gemm_f16x3_scaled_split.pp3"
    launched(lib, rc, site, name)
    s.C.payload.copy_(C.block())
    kx.verify_x3(s, f"{name} block 0")
    kl.assert_large(C, P, name)


# ==================================================================================================== refusals (DESIGN.md §32's guards)

def test_gemm16_refuses_a_leading_dimension_its_tile_offsets_cannot_hold(dev, lib):
    """256 rows x ld x 2 bytes must stay below 2^31: the guard stands in front of every launch of gemm16, so small buffers do."""
    a = torch.zeros((8, 64), dtype=torch.bfloat16, device=dev)
    c = kc.Guarded(8, 64, device=dev)
    for fn in (lib.dclip_gemm_bf16, lib.dclip_gemm_f16):
        for lda, ldw in ((1 << 22, 64), (64, 1 << 22)):
            rc = fn(a.data_ptr(), a.data_ptr(), c.ptr, None, None, 8, 8, 64, lda, ldw, 64, 0, 0, stream())
            assert rc == kc.E_INVAL and b"leading dimension too large" in lib.dclip_last_error()
    torch.cuda.synchronize()
    c.assert_guards("refused gemm16")
    assert bool(torch.isnan(c.get()).all()), "a refused call wrote to its output"


def test_attention_entries_refuse_products_that_do_not_fit_an_int(dev, lib):
    """B * H (the grid), 3 * H * 64 (the row length) and attention_cls_fwd's S * 3 * H * 64 (the query stride) are ints."""
    q = torch.zeros((4, 192), dtype=torch.bfloat16, device=dev)
    q32 = torch.zeros((4, 192), device=dev)
    o16, o32, lse = kc.Guarded(4, 64, device=dev, dtype=torch.bfloat16), kc.Guarded(4, 64, device=dev), kc.Guarded(1, 64, device=dev)
    big = 1 << 16
    for ty in ("bf16", "f16"):
        assert getattr(lib, f"dclip_attention_fwd_{ty}")(q.data_ptr(), o16.ptr, big, 4, big, 0, stream()) == kc.E_INVAL
        assert b"does not fit in an int" in lib.dclip_last_error()
        assert getattr(lib, f"dclip_attention_row_fwd_{ty}")(q.data_ptr(), None, o16.ptr, big, 4, big, stream()) == kc.E_INVAL
        assert getattr(lib, f"dclip_attention_fwd_{ty}")(q.data_ptr(), o16.ptr, 1, 4, 1 << 24, 0, stream()) == kc.E_INVAL
    assert lib.dclip_attention_fwd(q32.data_ptr(), o32.ptr, lse.ptr, big, 4, big, 0, stream()) == kc.E_INVAL
    assert lib.dclip_attention_cls_fwd(q32.data_ptr(), o32.ptr, lse.ptr, 1, 1 << 16, 1 << 8, stream()) == kc.E_INVAL
    assert b"does not fit in an int" in lib.dclip_last_error()
    torch.cuda.synchronize()
    for g in (o16, o32, lse):
        g.assert_guards("refused attention")
        assert bool(torch.isnan(g.get().float()).all()), "a refused call wrote to its output"


# ==================================================================================================== engine level

def norm_err(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max() / b.double().abs().max())


@pytest.fixture(scope="module")
def tower():
    """ViT-L/14's vision widths with TWO layers (one full-size layer and the CLS-only last one), frozen; 64 crops and their fp64
    features from the oracle, made once for the four precisions."""
    from dclip_amd import config as dcfg, synth
    from dclip_amd.clip_model import from_hf_state_dict
    from oracle import dclip_oracle as O
    base = dcfg.vit_l14()
    cfg = dataclasses.replace(base, vision=dataclasses.replace(base.vision, num_hidden_layers=2),
                              text=dcfg.tiny().text, name="ViT-L/14 x 2 layers")
    sd = synth.synth_clip_state_dict(cfg, seed=5, gain=2.0)
    model = from_hf_state_dict(cfg, sd, device=torch.device("cuda:0"))
    model.requires_grad_(False)
    pix0 = synth.synth_regions(kl.PERIOD_CROPS, 1, cfg.vision, seed=2)[:, 0].contiguous()
    kl.assert_rows_distinct(pix0.reshape(kl.PERIOD_CROPS, -1), "crops")
    p64 = {k: v.double() for k, v in sd.items() if k.startswith("vision_model.") or k.startswith("visual_projection")}
    want = O.vision_tower(p64, pix0.double(), cfg.vision)
    return model, pix0, want, {}


def engine_features(tower, precision, crops):
    model, pix0, want, got = tower
    if precision not in got:
        pix = pix0.cuda().repeat(crops // kl.PERIOD_CROPS, 1, 1, 1)
        kl.assert_period_breaks_wraps(pix0.numel(), 4, "pixels")
        with torch.no_grad():
            f = model.get_image_features(pixel_values=pix, precision=precision)
            small = model.get_image_features(pixel_values=pix[:kl.PERIOD_CROPS], precision=precision)
        torch.cuda.synchronize()
        assert f.shape == (crops, want.shape[1]) and bool(torch.isfinite(f).all())
        kl.check_periodic(f, kl.PERIOD_CROPS, f"{precision} features")           # crop i equals crop i mod 64, bit for bit
        print(f"\n[large] {precision}: the first 64 of {crops} crops equal a 64-crop call bit for bit: {torch.equal(f[:64], small)}"
              f" (max difference {norm_err(f[:64], small):.2e}; not required: the tile choice may differ with M)")
        got[precision] = f[:kl.PERIOD_CROPS].cpu()
    return got[precision]


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_engine_16bit_tower_over_4096_crops(tower, precision):
    """vision_fwd_bf16 / _layer_fwd_bf16 do no chunking: 4096 crops are one pass, M = 1,052,672 in every layer-sized tensor."""
    need("engine16")
    f = engine_features(tower, precision, kl.CROPS16)
    want = tower[2]
    rel = norm_err(f, want)
    cos = float(torch.nn.functional.cosine_similarity(f.double(), want, dim=1).min())
    print(f"[large] {precision} against fp64: max rel err {rel:.2e}, min cosine {cos:.6f}")
    if precision == "bf16":
        assert rel < 3e-2 and cos > 0.999, (rel, cos)        # tests/test_bf16_gpu.py::test_frozen_vision_tower_bf16_error
    else:
        assert rel < 1e-3 and cos > 0.99999, (rel, cos)      # tests/test_fp16_gpu.py: the 1e-3 bar


def test_engine_fp32_and_split16_towers_over_2048_crops(tower):
    """precision "fp32" at tests/test_model_gpu.py's 1e-3 against fp64; "fp32-split16" at the bars of
    tests/test_vision_frozen_split16_gpu.py: within 1e-5 of "fp32", at most 4 x its error against fp64, not its bits."""
    need("engine32")
    plain = engine_features(tower, "fp32", kl.CROPS32)
    split = engine_features(tower, "fp32-split16", kl.CROPS32)
    want = tower[2]
    d, es, ep = norm_err(split, plain), norm_err(split, want), norm_err(plain, want)
    print(f"[large] fp32 against fp64 {ep:.3e}; split vs plain {d:.3e}; split against fp64 {es:.3e} (ratio {es / ep:.2f})")
    assert ep < 1e-3, ep
    assert not torch.equal(split, plain), "the split path gave the plain path's bits: it did not run"
    assert d <= 1e-5, d
    assert es <= 4 * ep, (es, ep)


def test_engine_text_tower_over_4096_captions():
    """The frozen fp32 text tower at ViT-L/14's text widths, two layers, 4096 captions x 77 = 315,392 rows ([315,392][3072] fp32
    passes 2^31 bytes).  Captions repeat every 61 with ragged first-EOS positions (77 x 61 rows a period; the last period cut
    short); tests/test_model_gpu.py's 1e-3 against the fp64 oracle on the first 61."""
    need("engine_text32")
    from dclip_amd import config as dcfg, synth
    from dclip_amd.clip_model import from_hf_state_dict
    from oracle import dclip_oracle as O
    base = dcfg.vit_l14()
    cfg = dataclasses.replace(base, vision=dcfg.tiny().vision, text=dataclasses.replace(base.text, num_hidden_layers=2),
                              name="ViT-L/14 text x 2 layers")
    sd = synth.synth_clip_state_dict(cfg, seed=6, gain=2.0)
    model = from_hf_state_dict(cfg, sd, device=torch.device("cuda:0"))
    model.requires_grad_(False)
    n = 61
    ids0 = synth.synth_input_ids(n, cfg.text, seed=3, ragged=True)
    assert len({int(v) for v in O.first_eos_index(ids0, cfg.text.eos_token_id)}) > 8         # ragged
    kl.assert_period_breaks_wraps(n * 77 * 3 * cfg.text.hidden_size, 4, "text qkv")
    ids = ids0.repeat(4096 // n + 1, 1)[:4096].cuda()
    with torch.no_grad():
        f = model.get_text_features(input_ids=ids)
    torch.cuda.synchronize()
    assert f.shape[0] == 4096 and bool(torch.isfinite(f).all())
    kl.check_periodic(f, n, "text features")
    p64 = {k: v.double() for k, v in sd.items() if k.startswith("text_model.") or k.startswith("text_projection")}
    want = O.text_tower(p64, ids0, cfg.text)
    err = norm_err(f[:n], want)
    print(f"\n[large] text tower against fp64: {err:.3e}")
    assert err < 1e-3, err


# ==================================================================================================== the record

def test_zz_no_case_was_skipped_and_the_figures():
    """Last in the file: what the budget helper skipped (nothing, on an idle card), and the per-case figures."""
    total = sum(f["seconds"] for f in FIGURES)
    print(f"\n[large] {len(FIGURES)} cases, {total:.1f} s, largest peak {max([f['peak_bytes'] for f in FIGURES] + [0]) / kl.GIB:.2f} GiB, "
          f"skipped {len(SKIPPED)}: {SKIPPED}")
    assert not SKIPPED, SKIPPED
