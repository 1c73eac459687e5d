"""Two-piece [hi|lo] split operands at kernel level.  Every producer's two-piece entry is compared bit for bit
(torch.equal) with its three-piece twin on the same input: hi and lo are the twin's first two pieces, every other output is the
twin's, and the output buffer is a view inside a larger tensor pre-filled with a sentinel, so that a store outside
[rows][2 cols] shows.  Every fused consumer reads a [hi|lo] operand that lies inside a NaN-filled tensor, NaN immediately before
its first and after its last row, and must give the bits it gives on the [hi|lo|hi] operand."""
import pytest
import torch

from dclip_amd import _lib, ops

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SENT = 0x5A5A          # fp16 bit pattern of the sentinel (as int16)
PAD = 64               # fp16 elements of sentinel / NaN on either side (a multiple of 8: 16-byte alignment is kept)


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(DEV)


def guarded(n):
    """(buffer, view of n fp16 elements in its middle), the buffer pre-filled with the sentinel."""
    buf = torch.full((n + 2 * PAD,), SENT, dtype=torch.int16, device=DEV).view(torch.float16)
    return buf, buf[PAD:PAD + n]


def intact(buf, n):
    b = buf.view(torch.int16)
    return bool((b[:PAD] == SENT).all()) and bool((b[PAD + n:] == SENT).all())


def in_nan(t):
    """A copy of the 2-D fp16 tensor t that lies inside a NaN-filled tensor: NaN right before its first and after its last row."""
    buf = torch.full((t.numel() + 2 * PAD,), float("nan"), dtype=torch.float16, device=DEV)
    v = buf[PAD:PAD + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int16 if a.dtype == torch.float16 else torch.int32),
                       b.contiguous().view(torch.int16 if b.dtype == torch.float16 else torch.int32))


def strided(x, ldx):
    """x [rows, cols] as a view with row stride ldx >= cols."""
    rows, cols = x.shape
    big = torch.full((rows, ldx), 7.0, dtype=torch.float32, device=DEV)
    big[:, :cols] = x
    return big[:, :cols]


# ------------------------------------------------------------------------------------------------ the row / row + column splits
# one column count per NC instance of the dispatch (ceil(cols / 8 / 64) = 1 .. 6, then the generic one); none but the first two
# is a multiple of 512
COLS = [8, 520, 1288, 2040, 2312, 3064, 3080]
ROWS = [1, 5, 260]


@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("rows", ROWS)
def test_split_rows(rows, cols):
    lib = _lib.load()
    ldx = cols + 8 if (rows, cols) == (5, 520) else cols
    x = strided(rnd((rows, cols), 1 + rows + cols, 3.0), ldx)
    x[0, 0] = 0.0
    y3 = torch.empty((rows, 3 * cols), dtype=torch.float16, device=DEV)
    ra3 = torch.empty((rows,), dtype=torch.float32, device=DEV)
    buf, y2 = guarded(rows * 2 * cols)
    ra2 = torch.empty_like(ra3)
    _lib.check(lib.dclip_split_f32_f16x3_rows(x.data_ptr(), y3.data_ptr(), ra3.data_ptr(), rows, cols, ldx, ops._stream()))
    _lib.check(lib.dclip_split_f32_f16x2_rows(x.data_ptr(), y2.data_ptr(), ra2.data_ptr(), rows, cols, ldx, ops._stream()))
    assert same_bits(y2.view(rows, 2 * cols), y3[:, :2 * cols]) and same_bits(ra2, ra3)
    assert same_bits(y3[:, 2 * cols:], y3[:, :cols])                     # (the third the twin still writes is the first again)
    assert intact(buf, rows * 2 * cols)


def _colstats_outputs(rows, cols):
    return (torch.empty((rows,), dtype=torch.float32, device=DEV), torch.empty((rows, 2 * cols), dtype=torch.float16, device=DEV),
            torch.empty((cols,), dtype=torch.int32, device=DEV), torch.empty((cols,), dtype=torch.float32, device=DEV))


@pytest.mark.parametrize("with_db", [False, True])
@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("rows", ROWS)
def test_split_rows_colstats_three_launches(rows, cols, with_db):
    lib = _lib.load()
    ldx = cols + 8 if (rows, cols) == (5, 520) else cols
    x = strided(rnd((rows, cols), 2 + rows + cols, 0.25), ldx)
    nbytes = lib.dclip_split_f32_f16x3_rows_colstats_workspace(rows, cols)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=DEV)
    y3 = torch.empty((rows, 3 * cols), dtype=torch.float16, device=DEV)
    buf, y2 = guarded(rows * 2 * cols)
    o3, o2 = _colstats_outputs(rows, cols), _colstats_outputs(rows, cols)
    db3 = torch.empty((cols,), dtype=torch.float32, device=DEV) if with_db else None
    db2 = torch.empty((cols,), dtype=torch.float32, device=DEV) if with_db else None
    _lib.check(lib.dclip_split_f32_f16x3_rows_colstats(x.data_ptr(), y3.data_ptr(), o3[0].data_ptr(), o3[1].data_ptr(), o3[2].data_ptr(),
                                                       o3[3].data_ptr(), ops._ptr(db3), rows, cols, ldx, ws.data_ptr(), nbytes,
                                                       ops._stream()))
    _lib.check(lib.dclip_split_f32_f16x2_rows_colstats(x.data_ptr(), y2.data_ptr(), o2[0].data_ptr(), o2[1].data_ptr(), o2[2].data_ptr(),
                                                       o2[3].data_ptr(), ops._ptr(db2), rows, cols, ldx, ws.data_ptr(), nbytes,
                                                       ops._stream()))
    assert same_bits(y2.view(rows, 2 * cols), y3[:, :2 * cols])
    assert all(same_bits(a, b) for a, b in zip(o2, o3))                  # row_alpha, yc, col_exp, col_alpha
    assert db2 is None or same_bits(db2, db3)
    assert intact(buf, rows * 2 * cols)


@pytest.mark.parametrize("with_db", [False, True])
@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("rows", ROWS)
def test_split_rows_cols_from_producer_stats(rows, cols, with_db):
    lib = _lib.load()
    ldx = cols + 8 if (rows, cols) == (5, 520) else cols
    x = strided(rnd((rows, cols), 3 + rows + cols, 40.0), ldx)
    P = 3 if rows > 2 else 1                                             # more than one partial row where there are rows for it
    parts = torch.tensor_split(x, P, dim=0)
    pmax = torch.stack([p.abs().max(dim=0).values for p in parts]).contiguous().view(torch.int32)
    psum = torch.stack([p.sum(dim=0) for p in parts]).contiguous()
    y3 = torch.empty((rows, 3 * cols), dtype=torch.float16, device=DEV)
    buf, y2 = guarded(rows * 2 * cols)
    o3, o2 = _colstats_outputs(rows, cols), _colstats_outputs(rows, cols)
    db3 = torch.empty((cols,), dtype=torch.float32, device=DEV) if with_db else None
    db2 = torch.empty((cols,), dtype=torch.float32, device=DEV) if with_db else None
    for fn, y, o, db in ((lib.dclip_split_f32_f16x3_rows_cols_stats, y3, o3, db3), (lib.dclip_split_f32_f16x2_rows_cols_stats, y2, o2, db2)):
        _lib.check(fn(x.data_ptr(), y.data_ptr(), o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), ops._ptr(db),
                      pmax.data_ptr(), psum.data_ptr(), P, rows, cols, ldx, ops._stream()))
    assert same_bits(y2.view(rows, 2 * cols), y3[:, :2 * cols])
    assert all(same_bits(a, b) for a, b in zip(o2, o3))
    assert db2 is None or same_bits(db2, db3)
    assert intact(buf, rows * 2 * cols)


def test_wrappers_return_two_pieces():
    x = rnd((260, 520), 9)
    y3, ra3 = ops.split_f16x3_rows(x)
    y2, ra2 = ops.split_f16x3_rows(x, pieces=2)
    assert tuple(y2.shape) == (260, 1040) and same_bits(y2, y3[:, :1040]) and same_bits(ra2, ra3)
    o3 = ops.split_f16x3_rows_colstats(x)
    o2 = ops.split_f16x3_rows_colstats(x, pieces=2)
    assert same_bits(o2[0], o3[0][:, :1040]) and all(same_bits(a, b) for a, b in zip(o2[1:], o3[1:]))


# ------------------------------------------------------------------------------------------------ the element-wise split and LayerNorm
@pytest.mark.parametrize("cols", [8, 520])
@pytest.mark.parametrize("rows", ROWS)
def test_split_elementwise(rows, cols):
    lib = _lib.load()
    x = rnd((rows, cols), 4 + rows + cols)
    x[0, 1] = -0.0
    scale = torch.tensor([2.0 ** 9], dtype=torch.float32, device=DEV)
    ldy = 2 * cols + 8 if rows == 5 else 2 * cols                        # a wider output row once: the gap stays untouched
    for scale_v, scale_p in ((2.0 ** 9, None), (1.0, scale.data_ptr())):
        y3 = torch.empty((rows, 3 * cols), dtype=torch.float16, device=DEV)
        if scale_p is None:
            _lib.check(lib.dclip_split_f32_f16x3(x.data_ptr(), y3.data_ptr(), rows, cols, cols, 3 * cols, scale_v, 0, ops._stream()))
        else:
            _lib.check(lib.dclip_split_f32_f16x3_dev(x.data_ptr(), y3.data_ptr(), rows, cols, cols, 3 * cols, scale_p, 0, ops._stream()))
        buf, y2 = guarded(rows * ldy)
        _lib.check(lib.dclip_split_f32_f16x2(x.data_ptr(), y2.data_ptr(), rows, cols, cols, ldy, scale_v, scale_p, ops._stream()))
        y2 = y2.view(rows, ldy)
        assert same_bits(y2[:, :2 * cols], y3[:, :2 * cols])
        assert bool((y2[:, 2 * cols:].contiguous().view(torch.int16) == SENT).all()) and intact(buf, rows * ldy)
    assert same_bits(ops.split_f16x3(x, 4.0, pieces=2), ops.split_f16x3(x, 4.0)[:, :2 * cols])
    assert same_bits(ops.split_f16x3_dev(x, scale.data_ptr(), pieces=2), ops.split_f16x3_dev(x, scale.data_ptr())[:, :2 * cols])


@pytest.mark.parametrize("save", [False, True])
@pytest.mark.parametrize("D", [64, 520, 768])
@pytest.mark.parametrize("rows", [1, 5])
def test_layernorm_fwd(rows, D, save):
    lib = _lib.load()
    x, gamma, beta = rnd((rows, D), 5 + rows + D, 2.0), rnd((D,), 6, 0.5) + 1.0, rnd((D,), 7, 0.1)
    scale = torch.tensor([2.0 ** 11], dtype=torch.float32, device=DEV)

    def outs():
        if not save:
            return None, None, None
        return (torch.empty((rows, D), dtype=torch.float32, device=DEV), torch.empty((rows,), dtype=torch.float32, device=DEV),
                torch.empty((rows,), dtype=torch.float32, device=DEV))

    y3 = torch.empty((rows, 3 * D), dtype=torch.float16, device=DEV)
    s3, s2 = outs(), outs()
    _lib.check(lib.dclip_layernorm_fwd_f16x3_dev(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y3.data_ptr(), ops._ptr(s3[0]),
                                                 ops._ptr(s3[1]), ops._ptr(s3[2]), rows, D, 1e-5, scale.data_ptr(), ops._stream()))
    buf, y2 = guarded(rows * 2 * D)
    _lib.check(lib.dclip_layernorm_fwd_f16x2(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y2.data_ptr(), ops._ptr(s2[0]),
                                             ops._ptr(s2[1]), ops._ptr(s2[2]), rows, D, 1e-5, 1.0, scale.data_ptr(), ops._stream()))
    assert same_bits(y2.view(rows, 2 * D), y3[:, :2 * D]) and intact(buf, rows * 2 * D)
    if save:
        assert all(same_bits(a, b) for a, b in zip(s2, s3))
        assert same_bits(s2[0], ops.layernorm_fwd(x, gamma, beta, 1e-5, save_stats=True)[0])
    # the host-scale form and the wrappers
    assert same_bits(ops.layernorm_fwd_f16x3(x, gamma, beta, 1e-5, 2.0 ** 11, pieces=2), y3[:, :2 * D])
    w2 = ops.layernorm_fwd_f16x3_dev(x, gamma, beta, 1e-5, scale.data_ptr(), save=save, pieces=2)
    assert same_bits(w2[0], y3[:, :2 * D]) and (not save or all(same_bits(a, b) for a, b in zip(w2[1:], s3)))


# ------------------------------------------------------------------------------------------------ the GEMM with a split output
def _operands(M, N, K, seed):
    a3 = ops.split_f16x3(rnd((M, K), seed), 2.0 ** 8)                    # [hi|lo|hi]
    w3 = ops.split_f16x3(rnd((N, K), seed + 1, 0.1), 2.0 ** 10, 1)       # [hi|hi|lo]
    return a3, w3


@pytest.mark.parametrize("extra", [False, True])
@pytest.mark.parametrize("gelu", [False, True])
@pytest.mark.parametrize("K", [32, 96])
@pytest.mark.parametrize("N", [256, 264])
@pytest.mark.parametrize("M", [256, 300])
def test_gemm_split_output(M, N, K, gelu, extra):
    lib = _lib.load()
    a3, w3 = _operands(M, N, K, 11 + M + N + K)
    bias = rnd((N,), 13)
    epi = ops.EPI_BIAS | (ops.EPI_GELU if gelu else 0)
    sg = (0, K, 0, 2 * K)
    alpha = torch.tensor([2.0 ** -18], dtype=torch.float32, device=DEV)
    oscale = torch.tensor([2.0 ** 6], dtype=torch.float32, device=DEV)

    def f32():
        return torch.empty((M, N), dtype=torch.float32, device=DEV)

    h3, g3 = (f32() if extra and gelu else None), (f32() if extra else None)
    h2, g2 = (f32() if extra and gelu else None), (f32() if extra else None)
    c3 = torch.empty((M, 3 * N), dtype=torch.float16, device=DEV)
    _lib.check(lib.dclip_gemm_f16x3_scaled_split_dev(a3.data_ptr(), w3.data_ptr(), c3.data_ptr(), bias.data_ptr(), ops._ptr(h3),
                                                     ops._ptr(g3), M, N, K, 3 * K, 3 * K, 3 * N, *sg, epi, alpha.data_ptr(),
                                                     oscale.data_ptr(), ops._stream()))
    buf, c2 = guarded(M * 2 * N)
    _lib.check(lib.dclip_gemm_f16x3_scaled_split2_dev(a3.data_ptr(), w3.data_ptr(), c2.data_ptr(), bias.data_ptr(), ops._ptr(h2),
                                                      ops._ptr(g2), M, N, K, 3 * K, 3 * K, 2 * N, *sg, epi, alpha.data_ptr(),
                                                      oscale.data_ptr(), ops._stream()))
    assert same_bits(c2.view(M, 2 * N), c3[:, :2 * N]) and intact(buf, M * 2 * N)
    assert same_bits(c3[:, 2 * N:], c3[:, :N])
    if extra:
        assert same_bits(g2, g3) and (not gelu or same_bits(h2, h3))
    if not extra:                                                        # the host-scale entries (the frozen text tower's)
        c3h = torch.empty((M, 3 * N), dtype=torch.float16, device=DEV)
        _lib.check(lib.dclip_gemm_f16x3_scaled_split(a3.data_ptr(), w3.data_ptr(), c3h.data_ptr(), bias.data_ptr(), M, N, K, 3 * K, 3 * K,
                                                     3 * N, *sg, epi, 2.0 ** -18, 2.0 ** 6, ops._stream()))
        bufh, c2h = guarded(M * 2 * N)
        _lib.check(lib.dclip_gemm_f16x3_scaled_split2(a3.data_ptr(), w3.data_ptr(), c2h.data_ptr(), bias.data_ptr(), M, N, K, 3 * K, 3 * K,
                                                      2 * N, *sg, epi, 2.0 ** -18, 2.0 ** 6, ops._stream()))
        assert same_bits(c2h.view(M, 2 * N), c3h[:, :2 * N]) and intact(bufh, M * 2 * N) and same_bits(c3h, c3)


# ------------------------------------------------------------------------------------------------ the consumers
@pytest.mark.parametrize("bm192", ["0", "2"])
@pytest.mark.parametrize("K", [32, 64])
@pytest.mark.parametrize("N", [256, 264])
@pytest.mark.parametrize("M", [192, 320])
def test_fused_kmajor_entries_read_two_pieces(M, N, K, bm192, monkeypatch):
    monkeypatch.setenv("DCLIP_F16X3_BM192", bm192)
    a3, w3 = _operands(M, N, K, 17 + M + N + K)
    a2 = in_nan(a3[:, :2 * K])
    bias, res = rnd((N,), 19), rnd((M, N), 20)
    alpha = torch.tensor([2.0 ** -18], dtype=torch.float32, device=DEV)
    oscale = torch.tensor([2.0 ** 6], dtype=torch.float32, device=DEV)
    ra = (rnd((M,), 21).abs() + 0.5)
    h = rnd((M, N), 22)
    # the plain entries, host scales
    for kw in ({}, {"bias": bias, "residual": res}, {"bias": bias, "gelu": True}, {"bias": bias, "out_f16": True},
               {"bias": bias, "gelu": True, "split_out_scale": 2.0 ** 6}):
        want = ops.gemm_f16x3(a3, w3, alpha=2.0 ** -18, **kw)
        got = ops.gemm_f16x3(a2, w3, alpha=2.0 ** -18, pieces=2, **kw)
        assert same_bits(got, want) and bool(torch.isfinite(got.float()).all()), kw
    # _dev
    for kw in ({}, {"bias": bias, "residual": res}, {"bias": bias, "gelu": True, "h32": torch.empty_like(res)},
               {"bias": bias, "gelu": True, "split_out_scale_ptr": oscale.data_ptr()}):
        want = ops.gemm_f16x3_dev(a3, w3, alpha.data_ptr(), **kw)
        got = ops.gemm_f16x3_dev(a2, w3, alpha.data_ptr(), pieces=2, **kw)
        assert same_bits(got, want) and bool(torch.isfinite(got.float()).all()), kw
    # the two-piece operand into the two-piece output
    got = ops.gemm_f16x3_dev(a2, w3, alpha.data_ptr(), pieces=2, out_pieces=2, bias=bias, gelu=True, split_out_scale_ptr=oscale.data_ptr())
    want = ops.gemm_f16x3_dev(a3, w3, alpha.data_ptr(), bias=bias, gelu=True, split_out_scale_ptr=oscale.data_ptr())
    assert same_bits(got, want[:, :2 * N])
    # _rows_dev and its statistics twin
    for dgelu in (None, h):
        want = ops.gemm_f16x3_rows_dev(a3, w3, alpha.data_ptr(), ra, dgelu_h=dgelu)
        got = ops.gemm_f16x3_rows_dev(a2, w3, alpha.data_ptr(), ra, dgelu_h=dgelu, pieces=2)
        assert same_bits(got, want) and bool(torch.isfinite(got).all())
        P = (M + 255) // 256
        st3 = ops.ColStats.of(torch.empty((P, N), dtype=torch.int32, device=DEV), torch.empty((P, N), dtype=torch.float32, device=DEV))
        st2 = ops.ColStats.of(torch.empty((P, N), dtype=torch.int32, device=DEV), torch.empty((P, N), dtype=torch.float32, device=DEV))
        want = ops.gemm_f16x3_rows_dev(a3, w3, alpha.data_ptr(), ra, dgelu_h=dgelu, stats=st3)
        got = ops.gemm_f16x3_rows_dev(a2, w3, alpha.data_ptr(), ra, dgelu_h=dgelu, stats=st2, pieces=2)
        assert same_bits(got, want) and same_bits(st2.pmax, st3.pmax) and same_bits(st2.psum, st3.psum)


@pytest.mark.parametrize("splits", [1, 2])
@pytest.mark.parametrize("tokens", [192, 448])
def test_token_major_wgrad_reads_two_pieces(tokens, splits):
    M, N = 256, 264                                                      # dW [M, N] = dY^T X: dY [tokens, M], X [tokens, N]
    dy = rnd((tokens, M), 31 + tokens)
    _, _, yc, _, col_alpha = ops.split_f16x3_rows_colstats(dy)
    x3 = ops.split_f16x3(rnd((tokens, N), 32 + tokens), 2.0 ** 8)
    x2 = in_nan(x3[:, :2 * N])
    yc2 = in_nan(yc)
    act = torch.tensor([2.0 ** 8], dtype=torch.float32, device=DEV)
    want = ops.gemm_f16x3_wgrad_tokmajor(yc, x3, M, N, col_alpha, act.data_ptr(), splits=splits)
    got = ops.gemm_f16x3_wgrad_tokmajor(yc2, x2, M, N, col_alpha, act.data_ptr(), splits=splits)
    assert same_bits(got, want) and bool(torch.isfinite(got).all())
    want = ops.gemm_f16_wgrad_tokmajor_seg3(yc, x3, M, N, col_alpha, act.data_ptr(), splits=splits)
    got = ops.gemm_f16_wgrad_tokmajor_seg3(yc2, x2, M, N, col_alpha, act.data_ptr(), splits=splits)
    assert same_bits(got, want) and bool(torch.isfinite(got).all())


def test_a_two_piece_operand_is_refused_without_its_k():
    a3, w3 = _operands(192, 256, 32, 41)
    with pytest.raises(ValueError):
        ops.gemm_f16x3(a3[:, :64].contiguous(), w3)                      # 2 K columns read as a 3 K split: 64 % 3 != 0
