"""Host restatements for the column partials that the producers of a dY leave: which rows each producer folds
into which partial row, the partials themselves, the fold of the finishing kernel, and the fold that makes LayerNorm's dx_colsum.
numpy only; importable without a GPU."""
import numpy as np

F32_INF_BITS = 0x7F800000


def cdiv(a, b):
    return (a + b - 1) // b


# ---- which rows go into partial row p, per producer -------------------------------------------------------------------

def gemm_partition(M):
    """the data-gradient GEMM: partial row p = tile row p, rows 256 p .. 256 p + 255"""
    return [np.arange(256 * p, min(M, 256 * (p + 1))) for p in range(cdiv(M, 256))]


def attention_partition(B, S):
    """the attention backward: partial row b = the S tokens of image b"""
    return [np.arange(b * S, (b + 1) * S) for b in range(B)]


def ln_blocks(rows):
    return min(cdiv(rows, 4), 1024)


def ln_partition(rows):
    """ln_bwd: block b of P = min(ceil(rows / 4), 1024) walks rows 4 b + wave + 4 P k"""
    P = ln_blocks(rows)
    r = np.arange(rows)
    return [r[(r // 4) % P == b] for b in range(P)]


def round_robin_partition(rows, P):
    """any other grouping (P may exceed rows: a group without rows holds a zero maximum and a zero sum)"""
    r = np.arange(rows)
    return [r[r % P == p] for p in range(P)]


def is_partition(parts, rows):
    seen = np.concatenate([np.asarray(p, dtype=np.int64) for p in parts]) if parts else np.zeros(0, np.int64)
    return seen.size == rows and np.array_equal(np.sort(seen), np.arange(rows))


# ---- partials and folds -----------------------------------------------------------------------------------------------

def abs_bits(x):
    """bit patterns of |x| as unsigned integers: ordered like the values, inf above every finite value, NaN above inf"""
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)


def partials(x, parts):
    """pmax uint32 [P, cols] and psum fp32 [P, cols] of x [rows, cols] under a partition"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    P, cols = len(parts), x.shape[1]
    pmax, psum = np.zeros((P, cols), np.uint32), np.zeros((P, cols), np.float32)
    with np.errstate(all="ignore"):
        for p, rows in enumerate(parts):
            if len(rows):
                pmax[p] = abs_bits(x[rows]).max(axis=0)
                psum[p] = x[rows].sum(axis=0, dtype=np.float32)
    return pmax, psum


def row_exp_bits(bits):
    """split16.hip's row_exp on the bit pattern of a maximum >= 0 (engine.split16_col_exp's rule)"""
    bits = int(bits)
    if bits == 0 or bits >= F32_INF_BITS:
        return 0
    return max(-100, min(100, 14 - ((bits >> 23) - 126)))


def fold_col_exp(pmax):
    """colstats_finish_kernel's exponents: the rule applied to the maximum over the partial rows"""
    return np.array([row_exp_bits(b) for b in pmax.max(axis=0)], dtype=np.int32)


def fold_reduce_partials(psum):
    """reduce_partials_kernel's association for one output array: 64 row groups fold partials g, g + 64, ... in order; 4 threads
    fold 16 groups each in order; the last four as (a + b) + (c + d).  fp32 at every step."""
    P, cols = psum.shape
    with np.errstate(all="ignore"):
        red = np.zeros((64, cols), np.float32)
        for g in range(64):
            for p in range(g, P, 64):
                red[g] = red[g] + psum[p]
        red2 = np.zeros((4, cols), np.float32)
        for q in range(4):
            for k in range(16):
                red2[q] = red2[q] + red[q * 16 + k]
        return (red2[0] + red2[1]) + (red2[2] + red2[3])


def planted(rows, cols, seed, ld=None):
    """§9f's columns: rows and columns spread over e^(4 sigma); column 0 all zero, 1 with one inf, 2 with one NaN, 3 subnormal
    only, 4 holding 1e-30 beside one 1e+10.  [rows, ld or cols] fp32."""
    ld = ld or cols
    g = np.random.default_rng(seed)
    x = (g.standard_normal((rows, ld)) * np.exp(4.0 * g.standard_normal((rows, 1))) * np.exp(4.0 * g.standard_normal((1, ld))))
    x = x.astype(np.float32)
    x[:, 0] = 0.0
    x[0, 1] = np.inf
    x[min(1, rows - 1), 2] = np.nan
    x[:, 3] = (g.integers(1, 1 << 20, rows).astype(np.float64) * 2.0 ** -149).astype(np.float32)
    x[:, 4] = 1e-30
    x[rows // 2, 4] = 1e10
    return x
