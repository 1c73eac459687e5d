"""What tests/kernel_checks_large.py catches, shown without a GPU: the construction at scaled-down thresholds —
2^16 elements and 2^18 bytes stand for "the wrap" — run through a plain torch stand-in of each entry family (row-wise, GEMM +
epilogue, per-sequence attention, gather, im2col).  The stand-ins address memory the way a kernel does, offset = row * ld + col into
the flat allocation, so a fault is planted where it would sit in a kernel: in the offset arithmetic.  The stand-ins pass; each
planted fault is caught by the checker named for it; a power-of-two period does NOT catch the first fault."""
import pytest
import torch

from tests import kernel_checks as kc
from tests import kernel_checks_large as kl

TE, TB = 2 ** 16, 2 ** 18                       # the scaled wraps: elements, bytes
WRAPS = (TE, 2 * TE, TB, 2 * TB)
S, PC = 257, 2                                  # tokens per "crop", crops per period
P = PC * S                                      # 514 rows = 2 x 257
B = 80                                          # crops: 20,560 rows, 40 periods
M = B * S
COLS = 16


def gen(seed):
    return torch.Generator().manual_seed(seed)


def block(rows, cols, seed, ints=False):
    if ints:
        return torch.randint(-2, 3, (rows, cols), generator=gen(seed)).float()
    return torch.randn((rows, cols), generator=gen(seed))


# ---- the address model: what a kernel's index arithmetic makes of (row, ld) -------------------------------------------------------

def offsets(rows, ld, fault=None, itemsize=4):
    """Element offset of each row's first element.  Faults: the offset (or the byte offset) kept modulo a wrap distance."""
    o = torch.arange(rows, dtype=torch.int64) * ld
    if fault == "signed":                       # a signed 32-bit product: past the threshold it comes back as an earlier address
        o = o % TE
    elif fault == "unsigned":                   # an unsigned one wraps at twice that
        o = o % (2 * TE)
    elif fault == "bytes":                      # the element offset is right, its byte offset (x itemsize) wrapped
        o = (o * itemsize % TB) // itemsize
    else:
        assert fault is None
    return o


def load_rows(flat, off, cols):
    return flat[off[:, None] + torch.arange(cols)]


def store_rows(g, off, vals):
    """vals [n][cols] to element offsets `off` from the payload's origin, inside g's whole allocation (guards included)."""
    flat = g.buf.view(g.dtype)
    idx = g.guard + off[:, None] + torch.arange(vals.shape[1])
    flat[idx.reshape(-1)] = vals.to(g.dtype).reshape(-1)


def guarded(rows, cols, ld=None, dtype=torch.float32):
    return kl.LargeGuarded(rows, cols, ld, dtype=dtype)


# ---- the stand-ins ---------------------------------------------------------------------------------------------------------------

def rowwise(x_big, g, load=None, store=None, dtype_in_size=4, tail=None, extra_row=False):
    """A LayerNorm-like row kernel: y[r] = (x[r] - mean) * rstd, one row per "wave"."""
    rows, ld = x_big.shape[0] - 3, x_big.shape[1]
    x = load_rows(x_big.reshape(-1), offsets(rows, ld, load, dtype_in_size), ld).float()
    y = (x - x.mean(1, keepdim=True)) * torch.rsqrt(x.var(1, unbiased=False, keepdim=True) + 1e-5)
    off = offsets(rows, g.ld, store, g.buf.element_size())
    if tail == "unwritten":                     # the rows past the threshold are never reached
        keep = off < TE
        off, y = off[keep], y[keep]
    elif tail == "zeros":                       # ... or their loads came back as zeros (an out-of-range buffer load)
        y = torch.where((off < TE)[:, None], y, torch.zeros(()))
    store_rows(g, off, y)
    if extra_row:
        store_rows(g, torch.tensor([rows * g.ld]), y[-1:])


def gemm(a_big, w, bias, g, load=None, store=None):
    """C = A W^T + bias on integers, A addressed by row * lda, C by row * ldc."""
    rows, lda, K = a_big.shape[0] - 3, a_big.shape[1], w.shape[1]
    a = load_rows(a_big.reshape(-1), offsets(rows, lda, load), K)
    store_rows(g, offsets(rows, g.ld, store), a @ w.t() + bias)


def attention(qkv_big, g_out, g_lse, H, hd, lse_fault=None, load=None):
    """softmax(q k^T / sqrt(hd)) v per (crop, head); out [B*S][H*hd], lse [B][H*S] addressed as (b*H + h)*S + q."""
    rows, ld = qkv_big.shape[0] - 3, qkv_big.shape[1]
    nb = rows // S
    qkv = load_rows(qkv_big.reshape(-1), offsets(rows, ld, load), ld).view(nb, S, 3, H, hd).permute(2, 0, 3, 1, 4)
    sc = qkv[0] @ qkv[1].transpose(-1, -2) / hd ** 0.5
    out = (torch.softmax(sc, -1) @ qkv[2]).permute(0, 2, 1, 3).reshape(rows, H * hd)
    store_rows(g_out, offsets(rows, g_out.ld), out)
    lse = torch.logsumexp(sc, -1).reshape(-1)                      # [b][h][q]
    idx = torch.arange(lse.numel())
    if lse_fault == "wrapped":                                     # b*H*S formed in a narrow type
        idx = idx % TE
    flat = g_lse.buf.view(g_lse.dtype)
    flat[g_lse.guard + idx] = lse


def gather(x_big, idx, g, load=None):
    """out[b] = x[b*S + idx[b]]"""
    nb, ld = g.rows, x_big.shape[1]
    o = offsets(x_big.shape[0] - 3, ld, load)[torch.arange(nb) * S + idx]
    store_rows(g, offsets(nb, g.ld), load_rows(x_big.reshape(-1), o, ld))


def im2col(pix_big, nimg, C, Hh, p, g, load=None):
    """cols[(b, gy, gx)][(c, py, px)] = pix[b][c][gy p + py][gx p + px], the pixel addressed by one flat offset."""
    gr = Hh // p
    b, gy, gx, c, py, px = torch.meshgrid(*(torch.arange(n) for n in (nimg, gr, gr, C, p, p)), indexing="ij")
    o = ((b * C + c) * Hh + gy * p + py) * Hh + gx * p + px
    if load == "signed":
        o = o % TE
    store_rows(g, offsets(nimg * gr * gr, g.ld), pix_big.reshape(-1)[o.reshape(nimg * gr * gr, C * p * p)])


# ---- cases -----------------------------------------------------------------------------------------------------------------------

def rowwise_case(dtype=torch.float32, period=P, rows=M):
    x0 = block(period, COLS, 1)
    kl.assert_rows_distinct(x0, "x0")
    x = kl.tile_rows(x0, rows, dtype=dtype) if period == P else torch.cat([x0.repeat(rows // period, 1),
                                                                                     torch.full((3, COLS), kc.NAN)]).to(dtype)
    return x0, x, guarded(rows, COLS, dtype=dtype)


def rowwise_ref(x0, dtype=torch.float32):
    x = x0.to(dtype).float()
    return ((x - x.mean(1, keepdim=True)) * torch.rsqrt(x.var(1, unbiased=False, keepdim=True) + 1e-5)).to(dtype)


def failed(g, period=P, what="stand-in"):
    return set(kl.check_large(g, period, what))


def test_the_scaled_sizes_cross_the_scaled_wraps_and_the_period_breaks_them():
    assert M * COLS > 2 * TE and M * COLS * 2 > TB and B * 4 * S > TE
    for ld in (COLS, COLS + 4, 48, 24):
        for item in (2, 4):
            kl.assert_period_breaks_wraps(P * ld, item, "scaled", WRAPS)
    with pytest.raises(AssertionError, match="whole periods"):
        kl.assert_period_breaks_wraps(512 * COLS, 4, "a power-of-two period", WRAPS)


def test_the_real_cases_break_the_real_wraps_and_fit_their_caps():
    for name, c in kl.LARGE_CASES.items():
        assert c.rows in (kl.M16, kl.M32, kl.MP), name
        for r, ld, item, period in c.tensors:
            assert r >= period
            if r * ld * item > 2 ** 31:                              # (a one-row-per-crop output of 8 MB has nothing to wrap)
                kl.assert_period_breaks_wraps(period * ld, item, name)
        assert kl.peak_bytes(name) <= kl.cap_of(name), (name, kl.peak_bytes(name))
        x = kl.crossings(name)
        assert x["bytes_over"], f"{name}: its largest tensor crosses nothing"
    assert kl.crossings("fc1")["elements_over"] == list(kl.WRAPS) and kl.crossings("qkv")["elements_over"] == [2 ** 31]
    assert kl.crossings("gemm32_fc1")["elements_over"] == [2 ** 31] and kl.crossings("gemm32_qkv")["bytes_over"] == list(kl.WRAPS)
    assert kl.shortfall("fc2", 0) == kl.peak_bytes("fc2") and kl.shortfall("fc2", 1 << 40) == 0
    assert kl.shortfall("engine16", 10 * kl.GIB) == 54 * kl.GIB


def test_rows_distinct_notices_a_repeated_row():
    x0 = block(P, COLS, 1)
    x0[7] = x0[300]
    with pytest.raises(AssertionError, match="pairwise distinct"):
        kl.assert_rows_distinct(x0, "x0")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_rowwise_stand_in_passes(dtype):
    x0, x, g = rowwise_case(dtype)
    rowwise(x, g, dtype_in_size=x.element_size())
    assert not failed(g)
    assert torch.equal(g.block(P), rowwise_ref(x0, dtype))                                   # check A


def test_load_row_wrapped_as_signed_32_bit_is_caught_by_periodicity():
    x0, x, g = rowwise_case()
    rowwise(x, g, load="signed")
    assert failed(g) == {"periodic"}                         # every element written, nothing outside: only check B can see it
    assert torch.equal(g.block(P), rowwise_ref(x0))          # block 0 is right: check A alone would pass


def test_a_power_of_two_period_does_not_catch_that_fault():
    """The reason for the period's odd factor: 2^16 elements are 8 whole periods of 512 rows x 16, the wrapped load lands on the
    same row phase, reads the same data, and the output is periodic although the kernel is wrong."""
    x0, x, g = rowwise_case(period=512, rows=512 * 40)
    assert 512 * 40 * COLS > TE
    rowwise(x, g, load="signed")
    assert not failed(g, period=512)


def test_store_row_wrapped_leaves_nan_and_overwrites_an_earlier_row():
    x0, x, g = rowwise_case()
    rowwise(x, g, store="signed")
    f = kl.check_large(g, P, "stand-in")
    assert set(f) == {"nan", "periodic"} and "unwritten" in f["nan"]
    # the rows past the threshold landed on rows 0..: block 0 no longer holds its own result
    assert not torch.equal(g.block(P), rowwise_ref(x0))


def test_byte_offset_wrapped_with_the_element_offset_right_is_caught():
    x0, x, g = rowwise_case(torch.bfloat16)
    assert M * COLS <= 6 * TE and M * COLS * 2 > TB          # 2^18 bytes of bf16 are 2^17 elements: not the element wrap
    rowwise(x, g, load="bytes", dtype_in_size=2)
    assert failed(g) == {"periodic"}
    x0, x, g = rowwise_case(torch.bfloat16)
    rowwise(x, g, store="bytes", dtype_in_size=2)
    assert failed(g) == {"nan", "periodic"}


def test_unsigned_wrap_at_the_higher_threshold_is_caught():
    x0, x, g = rowwise_case()
    rowwise(x, g, load="unsigned")
    f = kl.check_large(g, P, "stand-in")
    assert set(f) == {"periodic"}
    first_bad = 2 * TE // COLS                                # row 8192: nothing below the higher threshold is wrong
    assert int(f["periodic"].split("global row ")[1].split(":")[0]) >= first_bad


def test_tail_never_written_is_caught_by_the_nan_check():
    x0, x, g = rowwise_case()
    rowwise(x, g, tail="unwritten")
    f = kl.check_large(g, P, "stand-in")
    assert "nan" in f and f"global row {TE // COLS}" in f["nan"]


def test_tail_written_with_zeros_is_caught_by_periodicity_only():
    x0, x, g = rowwise_case()
    rowwise(x, g, tail="zeros")
    assert failed(g) == {"periodic"}                          # zeros are not NaN: the memory check passes


def test_a_write_one_row_past_the_end_is_caught_by_the_guard():
    x0, x, g = rowwise_case()
    rowwise(x, g, extra_row=True)
    f = kl.check_large(g, P, "stand-in")
    assert set(f) == {"guard"} and f"({M}, 0)" in f["guard"]


def test_guard_check_sees_padding_columns_and_the_band_in_front():
    g = guarded(M, COLS, COLS + 4)
    g.payload.fill_(1.0)
    assert not failed(g)
    g.mat[M - 1, COLS + 1] = 0.0
    g.buf[g.guard - 1] = 0
    bad = g.guard_violations()
    assert (-1, COLS + 3) in bad and (M - 1, COLS + 1) in bad


def gemm_case():
    K, N = COLS, 24
    a0, w, bias = block(P, K, 2, ints=True), block(N, K, 3, ints=True), block(1, N, 4, ints=True)[0]
    a0[:, 0] = torch.arange(P) % 5 - 2                        # rows stay distinct on small integers
    a0[:, 1] = (torch.arange(P) // 5) % 5 - 2
    a0[:, 2] = (torch.arange(P) // 25) % 5 - 2
    a0[:, 3] = (torch.arange(P) // 125) % 5 - 2
    kl.assert_rows_distinct(a0, "a0")
    return a0, w, bias, kl.tile_rows(a0, M, K + 8), guarded(M, N, N + 4)


def test_gemm_stand_in_passes_and_its_wrapped_operand_row_and_store_are_caught():
    a0, w, bias, a, g = gemm_case()
    gemm(a, w, bias, g)
    assert not failed(g)
    assert torch.equal(g.block(P), a0 @ w.t() + bias)                                        # check A: integer-exact
    a0, w, bias, a, g = gemm_case()
    gemm(a, w, bias, g, load="signed")
    assert failed(g) == {"nan", "periodic"}                  # another row phase, and the NaN of the operand's padding columns
    a0, w, bias, a, g = gemm_case()
    gemm(a, w, bias, g, store="unsigned")
    assert failed(g) == {"guard", "nan", "periodic"}         # ... and a wrapped store crosses C's padding columns: the guard too


def attention_case():
    H, hd = 4, 4
    q0 = block(P, 3 * H * hd, 5)
    kl.assert_rows_distinct(q0, "qkv0")
    qkv = kl.tile_rows(q0, M)
    return H, hd, q0, qkv, guarded(M, H * hd), guarded(B, H * S)


def test_attention_stand_in_passes_and_a_wrapped_lse_index_is_caught():
    H, hd, q0, qkv, out, lse = attention_case()
    attention(qkv, out, lse, H, hd)
    assert not failed(out) and not failed(lse, period=PC, what="lse")
    ref_out, ref_lse = guarded(P, H * hd), guarded(PC, H * S)
    attention(kl.tile_rows(q0, P), ref_out, ref_lse, H, hd)
    assert torch.equal(out.block(P), ref_out.block(P)) and torch.equal(lse.block(PC), ref_lse.block(PC))      # check A
    H, hd, q0, qkv, out, lse = attention_case()
    attention(qkv, out, lse, H, hd, lse_fault="wrapped")
    assert not failed(out)
    f = kl.check_large(lse, PC, "lse")
    assert set(f) == {"nan", "periodic"}                      # the tail of lse unwritten, its head overwritten by other rows' values


def test_gather_stand_in_passes_and_a_wrapped_source_row_is_caught():
    x0 = block(P, COLS, 6)
    x = kl.tile_rows(x0, M)
    idx0 = torch.tensor([S - 1, 0])                           # the last row of one crop, the first of the next: period 2 crops
    idx = idx0.repeat(B // PC)
    g = guarded(B, COLS)
    gather(x, idx, g)
    assert not failed(g, period=PC)
    assert torch.equal(g.block(PC), x0.view(PC, S, COLS)[torch.arange(PC), idx0])            # check A
    g = guarded(B, COLS)
    gather(x, idx, g, load="signed")
    assert failed(g, period=PC) == {"periodic"}


def test_im2col_stand_in_passes_and_a_wrapped_pixel_offset_is_caught():
    C, Hh, p = 1, 8, 4
    nper, nimg = 2 * 257, 3 * 2 * 257                         # 514 images of 64 pixels a period; 98,688 pixels in all
    pix0 = block(nper, C * Hh * Hh, 7)
    pix = kl.tile_rows(pix0, nimg)
    assert nimg * C * Hh * Hh > TE
    rows_per = nper * (Hh // p) ** 2
    g = guarded(nimg * (Hh // p) ** 2, C * p * p)
    im2col(pix, nimg, C, Hh, p, g)
    assert not failed(g, period=rows_per)
    want = pix0.view(nper, C, Hh // p, p, Hh // p, p).permute(0, 2, 4, 1, 3, 5).reshape(rows_per, C * p * p)
    assert torch.equal(g.block(rows_per), want)                                              # check A
    g = guarded(nimg * (Hh // p) ** 2, C * p * p)
    im2col(pix, nimg, C, Hh, p, g, load="signed")
    assert failed(g, period=rows_per) == {"periodic"}


def test_check_periodic_compares_nan_bit_patterns_and_names_the_first_difference():
    out = torch.zeros(4 * P, 8)
    out[5::P, 3] = kc.NAN                                     # the same NaN in every period: periodic
    assert kl.check_periodic(out, P, "nan pattern") == 4
    out.view(torch.int32)[2 * P + 5, 3] = 0x7FC00001          # another NaN payload in period 2
    with pytest.raises(AssertionError, match=r"\(period 2, row 5, col 3\)"):
        kl.check_periodic(out, P, "nan pattern")


def test_a_period_cut_short_is_compared_with_the_head_of_block_0():
    x0 = block(P, COLS, 8)
    rows = 3 * P + 100
    x = kl.tile_rows(x0, rows)
    assert kl.check_periodic(x[:rows], P, "cut short") == 4
    x[3 * P + 99, 5] += 1.0
    with pytest.raises(AssertionError, match=r"\(period 3, row 99, col 5\)"):
        kl.check_periodic(x[:rows], P, "cut short")
