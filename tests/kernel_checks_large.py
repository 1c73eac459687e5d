"""TEST-ONLY construction and checkers for tensors beyond 2^31 elements / 4 GiB: tests/test_large_tensor_paths_gpu.py
runs the frozen-tower kernels at config c5's own row count with them, tests/test_kernel_checks_large_cpu.py shows what they catch.

Nothing here imports the product or needs a GPU.  An fp64 reference of an 8.6 GB tensor is not a test of a few seconds, and the
kernels are row-wise or sequence-wise, so:

  * input: a block x0 of PERIOD_ROWS = 64 x 257 rows (64 crops of ViT-L/14's 257 tokens; random, rows pairwise distinct) is laid
    down M / PERIOD_ROWS times.  The period has the odd factor 257 in rows, elements and bytes, so no power-of-two wrap distance
    (2^31 or 2^32 elements or bytes) is a whole number of periods: an address that wrapped lands on another row phase, on other
    data.  assert_period_breaks_wraps() states that for every tensor a case builds; a power-of-two period would hide exactly the
    fault this is for (the CPU self-test keeps that as a test).
  * check A: block 0 of the output goes to the checker the project already has for the entry at that shape (kernel_checks*.py):
    no new tolerance.
  * check B (check_periodic): every period of the output equals block 0 bit for bit, compared as integer words (NaNs compare);
    the first differing (period, row, column) is reported.  One pass over the whole tensor.
  * check C (LargeGuarded.assert_guards, check_no_nan): the output lies in a sentinel-filled allocation whose bands and
    leading-dimension padding must be intact, the payload starts as NaN and none may remain; operand padding is NaN (tiled).
  * budget: a case declares its peak device bytes (LARGE_CASES); shortfall() says by how much the free memory misses it.
"""
from __future__ import annotations

from collections import namedtuple

import torch

from tests import kernel_checks as kc

SEQ = 257                                   # tokens of a ViT-L/14 crop at 224 x 224
PERIOD_CROPS = 64
PERIOD_ROWS = PERIOD_CROPS * SEQ            # 16,448 = 2^6 x 257
CROPS16, CROPS32 = 4096, 2048               # c5: 512 pairs x 8 crops on the 16-bit route; half that batch on the fp32 routes
M16, M32 = CROPS16 * SEQ, CROPS32 * SEQ     # 1,052,672 and 526,336 rows: 64 and 32 periods
WRAPS = (2 ** 31, 2 ** 32)                  # the distances a 32-bit index or byte offset wraps by
GIB = 1 << 30
CAP16, CAP32 = 24 * GIB, 32 * GIB           # per-case ceilings of the 16-bit and the fp32 cases
D, D3, DI, H, PATCH, PATCH_DIM, GRID2 = 1024, 3072, 4096, 16, 14, 588, 256      # ViT-L/14's widths; 256 patches per crop
_WORD = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def words(t: torch.Tensor) -> torch.Tensor:
    """t as integer words of its element size (a view: strides are kept)."""
    return t if not t.is_floating_point() else t.view(_WORD[t.element_size()])


def assert_period_breaks_wraps(period_elems: int, itemsize: int, what: str, wraps=WRAPS):
    """No wrap distance, counted in elements or in bytes, is a whole number of periods of this tensor."""
    assert period_elems > 0 and itemsize > 0
    for w in wraps:
        assert w % period_elems != 0, f"{what}: {w} elements are {w // period_elems} whole periods of {period_elems} elements"
        assert w % (period_elems * itemsize) != 0, f"{what}: {w} bytes are whole periods of {period_elems * itemsize} bytes"


def assert_rows_distinct(x0: torch.Tensor, what: str):
    """Rows of the block are pairwise distinct (a 64-bit hash of each row's words; a collision could only fail a good block)."""
    w = words(x0.reshape(x0.shape[0], -1)).to(torch.int64)
    g = torch.Generator().manual_seed(12345)
    mult = (torch.randint(1, 2 ** 31, (w.shape[1],), generator=g, dtype=torch.int64) * 2 + 1).to(w.device)
    h = (w * mult).sum(1)
    assert int(torch.unique(h).numel()) == x0.shape[0], f"{what}: rows of the block are not pairwise distinct"


def tile_rows(x0: torch.Tensor, rows: int, ld: int = None, device=None, extra_rows: int = 3, dtype=None) -> torch.Tensor:
    """x0 [P][cols] laid down over `rows` rows (the last period may be cut short) with leading dimension ld:
    [rows + extra_rows][ld]; padding columns and the rows behind the operand are NaN (integer types: all ones).  Asserts the period
    property for the tensor it builds."""
    P, cols = x0.shape
    ld = cols if ld is None else ld
    dtype = dtype or x0.dtype
    device = device or x0.device
    assert ld >= cols and rows >= P
    assert_period_breaks_wraps(P * ld, torch.empty((), dtype=dtype).element_size(), f"tile_rows [{rows} / {P}][{ld}]")
    fill = kc.NAN if dtype.is_floating_point else -1
    big = torch.full((rows + extra_rows, ld), fill, dtype=dtype, device=device)
    x0 = x0.to(device=device, dtype=dtype)
    full = rows // P
    big[:full * P].view(full, P, ld)[:, :, :cols] = x0[None]
    big[full * P:rows, :cols] = x0[:rows - full * P]
    return big


class LargeGuarded(kc.Guarded):
    """kernel_checks.Guarded whose guard check reads the two bands and the padding columns only: no copy of the allocation."""

    def guard_violations(self):
        n, bad = self.rows * self.ld, []
        for base, band in ((-self.guard, self.buf[:self.guard]), (n, self.buf[self.guard + n:])):
            for i in (band != self.sentinel).nonzero().flatten()[:8].cpu().tolist():
                bad.append(divmod(base + i, self.ld))
        if self.ld > self.cols:
            pad = self.buf[self.guard:self.guard + n].view(self.rows, self.ld)[:, self.cols:]
            for r, c in (pad != self.sentinel).nonzero()[:8].cpu().tolist():
                bad.append((r, self.cols + c))
        return bad[:8]

    def block(self, period: int = PERIOD_ROWS, index: int = 0) -> torch.Tensor:
        return self.payload[index * period:(index + 1) * period].detach().cpu().clone()


def check_periodic(out: torch.Tensor, period: int, what: str) -> int:
    """Check B: out [rows][cols] (any strides) repeats its first `period` rows bit for bit; a last period cut short is compared
    with the head of block 0.  Returns the periods compared."""
    rows = out.shape[0]
    assert rows >= period, (rows, period)
    w = words(out)
    n = -(-rows // period)
    for p in range(1, n):
        blk = w[p * period:(p + 1) * period]
        first = w[:blk.shape[0]]
        if not torch.equal(blk, first):
            diff = (blk != first).nonzero()
            r, c = (int(v) for v in diff[0])
            raise AssertionError(f"{what}: period {p} differs from block 0 in {diff.shape[0]} words, first at (period {p}, row {r}, "
                                 f"col {c}) = global row {p * period + r}: {out[p * period + r, c].item()!r} against {out[r, c].item()!r}")
    return n


def check_no_nan(out: torch.Tensor, period: int, what: str):
    """Check C, payload half: the NaN the payload started as is gone everywhere (period by period: no mask of the whole tensor)."""
    rows = out.shape[0]
    for p in range(-(-rows // period)):
        blk = out[p * period:(p + 1) * period]
        nan = torch.isnan(blk)
        if bool(nan.any()):
            r, c = (int(v) for v in nan.nonzero()[0])
            raise AssertionError(f"{what}: {int(nan.sum())} NaN (unwritten?) elements in period {p}, first at global row "
                                 f"{p * period + r}, col {c}")


def check_large(g: LargeGuarded, period: int, what: str, nan_ok: bool = False):
    """Checks C and B of one guarded output; returns the names of the checks that failed with their messages (empty: passed)."""
    failed = {}
    for name, fn in (("guard", lambda: g.assert_guards(what)), ("nan", lambda: nan_ok or check_no_nan(g.payload, period, what)),
                     ("periodic", lambda: check_periodic(g.payload, period, what))):
        try:
            fn()
        except AssertionError as e:
            failed[name] = str(e)
    return failed


def assert_large(g: LargeGuarded, period: int, what: str, nan_ok: bool = False):
    failed = check_large(g, period, what, nan_ok)
    assert not failed, "; ".join(f"[{k}] {v}" for k, v in failed.items())


# ------------------------------------------------------------------------------------------------ the cases and their budgets

LargeCase = namedtuple("LargeCase", "route rows tensors")          # tensors: ((rows, ld, itemsize, period rows), ...) alive at the launch
MP = CROPS16 * GRID2                        # patch rows of 4096 crops: 1,048,576 = 2^20
# Patch-row tensors have 256 rows a crop: at a power-of-two width any whole number of crops is a power-of-two period.  Where the
# entry takes a leading dimension the output gets ldc = 1028 = 4 x 257; vision_assemble_fwd takes none, so its input repeats every
# ASSEMBLE_CROPS = 61 crops (4096 = 67 x 61 + 9: the last period is cut short).
LDC_PATCH, ASSEMBLE_CROPS = 1028, 61


def _t(rows, ld, item, period=PERIOD_ROWS):
    return (rows, ld, item, period)


PP = PERIOD_CROPS * GRID2                   # patch rows of 64 crops
LARGE_CASES = {
    # 16-bit route (bf16 and fp16), M = 1,052,672
    "ln16": LargeCase("16", M16, (_t(M16, D, 4), _t(M16, D, 2))),
    "qkv": LargeCase("16", M16, (_t(M16, D, 2), _t(M16, D3, 2))),
    "attention": LargeCase("16", M16, (_t(M16, D3, 2), _t(M16, D, 2), _t(CROPS16, D, 2, PERIOD_CROPS))),
    "out_proj": LargeCase("16", M16, (_t(M16, D, 2), _t(M16, D, 4), _t(M16, D, 4))),
    "fc1": LargeCase("16", M16, (_t(M16, D, 2), _t(M16, DI, 2))),
    "fc2": LargeCase("16", M16, (_t(M16, DI, 2), _t(M16, D, 4), _t(M16, D, 4))),
    "gather_rows": LargeCase("16", M16, (_t(M16, D, 4), _t(CROPS16, D, 4, PERIOD_CROPS))),
    "im2col": LargeCase("16", MP, (_t(CROPS16 * 3 * 224, 224, 4, PERIOD_CROPS * 3 * 224), _t(MP, PATCH_DIM, 4, PP))),
    "patch_gemm": LargeCase("16", MP, (_t(MP, 592, 2, PP), _t(MP, LDC_PATCH, 4, PP))),
    "assemble": LargeCase("16", M16, (_t(MP, D, 4, ASSEMBLE_CROPS * GRID2), _t(M16, D, 4, ASSEMBLE_CROPS * SEQ))),
    "cast": LargeCase("16", M16, (_t(M16, D, 4), _t(M16, D, 2))),
    # fp32 route, M = 526,336
    "ln32": LargeCase("32", M32, (_t(M32, D, 4), _t(M32, D, 4))),
    "gemm32_qkv": LargeCase("32", M32, (_t(M32, D, 4), _t(M32, D3, 4))),
    "gemm32_fc1": LargeCase("32", M32, (_t(M32, D, 4), _t(M32, DI, 4), _t(M32, DI, 4))),
    "attention32": LargeCase("32", M32, (_t(M32, D3, 4), _t(M32, D, 4), _t(M32, H, 4))),
    "attention32_cls": LargeCase("32", M32, (_t(M32, D3, 4), _t(CROPS32, D, 4, PERIOD_CROPS))),
    # split-fp16 frozen route, M = 526,336
    "ln_f16x2": LargeCase("split16", M32, (_t(M32, D, 4), _t(M32, 2 * D, 2))),
    "split_f16x2": LargeCase("split16", M32, (_t(M32, DI, 4), _t(M32, 2 * DI, 2))),
    "f16x3_fc1": LargeCase("split16", M32, (_t(M32, 3 * D + 8, 2), _t(M32, 3 * DI, 2))),       # §25's operands: three pieces
    "f16x3_fc2": LargeCase("split16", M32, (_t(M32, 3 * DI + 8, 2), _t(M32, D, 4), _t(M32, D, 4))),
}
SLACK = 2 * GIB                             # guard bands, weights, the comparison's temporaries, the allocator's rounding


# engine level: a two-layer ViT-L/14 tower over all crops in one pass.  What is alive at once is the engine's business (pixels,
# patch rows, the residual stream twice, a layer's LayerNorm / qkv / context / fc1 activations and the allocator's cache of the
# buffers it released); the declared peaks are twice the sum of those tensors, rounded up, and the test prints the measured one.
ENGINE_PEAKS = {"engine16": 64 * GIB, "engine32": 64 * GIB, "engine_text32": 24 * GIB}


def peak_bytes(name: str) -> int:
    if name in ENGINE_PEAKS:
        return ENGINE_PEAKS[name]
    return sum(t[0] * t[1] * t[2] for t in LARGE_CASES[name].tensors) + SLACK


def cap_of(name: str) -> int:
    """The ceiling of a kernel-level case."""
    return CAP16 if LARGE_CASES[name].route == "16" else CAP32


def shortfall(name: str, free_bytes: int) -> int:
    """Bytes by which `free_bytes` misses the case's declared peak (0: it fits)."""
    return max(0, peak_bytes(name) - int(free_bytes))


def crossings(name: str):
    """What the case's largest tensor crosses: the thresholds below its element count and its byte size."""
    r, ld, item, _ = max(LARGE_CASES[name].tensors, key=lambda t: t[0] * t[1] * t[2])
    n = r * ld
    return {"elements": n, "bytes": n * item, "elements_over": [w for w in WRAPS if n > w], "bytes_over": [w for w in WRAPS if n * item > w]}
