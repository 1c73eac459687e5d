// fp32 -> two fp16 pieces, for the frozen fp32 text tower on the fp16 MFMAs.
//
// x = hi + lo with hi = fp16(x), lo = fp16(x - hi) carries 22 mantissa bits, and a product of two fp16 values is exact in the
// MFMA's fp32 accumulator, so  A W^T ~= A_hi W_hi^T + A_lo W_hi^T + A_hi W_lo^T  (the lo.lo term, 2^-22 relative, is dropped).
// The three products are ONE fp16 GEMM along K' = 3K on
//     activations [hi | lo | hi]   (order 0)        weights [hi | hi | lo]   (order 1)
// which dclip_gemm_f16_scaled evaluates as it stands.  Both kernels here write that layout: the stand-alone split of an fp32
// matrix, and LayerNorm with the split as its output (the fp32 LayerNorm result is never stored).  `scale` is a power of two
// chosen by the caller from the frozen weights so that |x scale| <= 2^14: the pieces sit high in fp16's range (lo well above
// the subnormals for every value that matters) and nothing overflows; the GEMM's alpha undoes it.  Rounding is plain IEEE
// round-to-nearest-even, no saturation: a value beyond the caller's bound becomes inf like any fp16 overflow.
#include "common.h"

namespace {

typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4s __attribute__((ext_vector_type(4)));
typedef int i32x4s __attribute__((ext_vector_type(4)));

// 8 columns per thread: two 16-byte loads, three 16-byte stores.  ORDER 2: the two-piece form [hi | lo], the third
// store — the duplicate hi no fused GEMM reads — left out; ldy >= 2 cols there.
template <int ORDER>
__global__ void __launch_bounds__(256) split_f16x3_kernel(const float* __restrict__ x, unsigned short* __restrict__ y, int rows,
                                                          int cols, int ldx, int ldy, float scale_v,
                                                          const float* __restrict__ scale_p) {
  const float scale = scale_p ? *scale_p : scale_v;   // _dev entry: the scale lives in the device plan record
  const int c8 = cols >> 3;
  const size_t total = (size_t)rows * c8;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % c8) * 8;
    const size_t r = i / c8;
    const f32x4 a = *reinterpret_cast<const f32x4*>(x + r * ldx + c);
    const f32x4 b = *reinterpret_cast<const f32x4*>(x + r * ldx + c + 4);
    u16x8 hi, lo;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      unsigned short h0, l0, h1, l1;
      split1(a[e] * scale, h0, l0);
      split1(b[e] * scale, h1, l1);
      hi[e] = h0, lo[e] = l0, hi[4 + e] = h1, lo[4 + e] = l1;
    }
    unsigned short* yr = y + r * ldy + c;
    *reinterpret_cast<u16x8*>(yr) = hi;
    *reinterpret_cast<u16x8*>(yr + cols) = ORDER == 1 ? hi : lo;
    if (ORDER != 2) *reinterpret_cast<u16x8*>(yr + 2 * cols) = ORDER == 0 ? hi : lo;
  }
}

__device__ __forceinline__ float pow2f(int e) {      // 2^e, e clamped to the normal range
  e = e < -126 ? -126 : (e > 127 ? 127 : e);
  return __builtin_bit_cast(float, (unsigned)(e + 127) << 23);
}

// Row-scaled split for the data-gradient GEMMs of the backward: dY has no bound derivable from the weights, so
// every ROW m gets its own power of two, taken from the data in the same pass.  r = max|x[m,:]| = mu 2^x (mu in [0.5, 1)):
// e_m = 14 - x clamped to [-100, 100] (r 2^e_m in [2^13, 2^14); 2^e_m, 2^-e_m and their products with a weight alpha stay
// normal fp32), e_m = 0 when r is 0 or not finite.  y[m] = [hi|lo|hi] of x[m] 2^e_m, row_alpha[m] = 2^-e_m.  A non-finite row
// yields non-finite pieces (and so a non-finite output row of the GEMM, as fp32 would); other rows are unaffected.
// One wave per row.  NC > 0: the row (cols <= 512 NC) is held in registers between the maximum and the split, read from
// memory ONCE; NC == 0 (any width): two loops over the row, the second read served by the cache.  The maximum is taken on the
// bit patterns of |x| (NaN above inf), lane-local in column order, then the xor tree: the same in every run.
__device__ __forceinline__ unsigned wave_umax_bits(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned w = (unsigned)__shfl_xor((int)v, o, 64);
    v = v > w ? v : w;
  }
  return v;
}

__device__ __forceinline__ unsigned absmax8(unsigned m, const f32x4& a, const f32x4& b) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float fa = a[e], fb = b[e];   // a copy first: a bit cast of the vector ELEMENT itself reads element 0 whatever e is
    const unsigned ua = __builtin_bit_cast(unsigned, fa) & 0x7fffffffu, ub = __builtin_bit_cast(unsigned, fb) & 0x7fffffffu;
    m = m > ua ? m : ua;
    m = m > ub ? m : ub;
  }
  return m;
}

// engine.split16_row_exp on the bit pattern of r = max|x| >= 0
__device__ __forceinline__ int row_exp(unsigned rbits) {
  if (rbits == 0u || rbits >= 0x7f800000u) return 0;
  const int e = 14 - ((int)(rbits >> 23) - 126);        // a subnormal r (biased exponent 0) asks for more than the clamp
  return e < -100 ? -100 : (e > 100 ? 100 : e);
}

// P = pieces per row: 3 = [hi|lo|hi], 2 = [hi|lo] (the same two pieces, the duplicate third not stored)
template <int P = 3>
__device__ __forceinline__ void split_store8(unsigned short* yr, int cols, const f32x4& a, const f32x4& b, float scale) {
  u16x8 hi, lo;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    unsigned short h0, l0, h1, l1;
    split1(a[e] * scale, h0, l0);
    split1(b[e] * scale, h1, l1);
    hi[e] = h0, lo[e] = l0, hi[4 + e] = h1, lo[4 + e] = l1;
  }
  *reinterpret_cast<u16x8*>(yr) = hi;
  *reinterpret_cast<u16x8*>(yr + cols) = lo;
  if (P == 3) *reinterpret_cast<u16x8*>(yr + 2 * cols) = hi;
}

template <int NC, int P = 3>
__global__ void __launch_bounds__(256) split_rows_f16x3_kernel(const float* __restrict__ x, unsigned short* __restrict__ y,
                                                               float* __restrict__ row_alpha, int rows, int cols, int ldx) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int c8 = cols >> 3;
  const float* xr = x + (size_t)row * ldx;
  unsigned short* yr = y + (size_t)row * P * cols;
  unsigned m = 0u;
  if (NC > 0) {
    f32x4 a[NC > 0 ? NC : 1], b[NC > 0 ? NC : 1];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int i = lane + 64 * c, ic = i < c8 ? i : 0;       // a chunk past the row re-reads chunk 0: same maximum
      a[c] = *reinterpret_cast<const f32x4*>(xr + ic * 8);
      b[c] = *reinterpret_cast<const f32x4*>(xr + ic * 8 + 4);
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) m = absmax8(m, a[c], b[c]);
    const int e = row_exp(wave_umax_bits(m));
    const float scale = pow2f(e);
    if (lane == 0) row_alpha[row] = pow2f(-e);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int i = lane + 64 * c;
      if (i < c8) split_store8<P>(yr + i * 8, cols, a[c], b[c], scale);
    }
  } else {
    for (int i = lane; i < c8; i += 64)
      m = absmax8(m, *reinterpret_cast<const f32x4*>(xr + i * 8), *reinterpret_cast<const f32x4*>(xr + i * 8 + 4));
    const int e = row_exp(wave_umax_bits(m));
    const float scale = pow2f(e);
    if (lane == 0) row_alpha[row] = pow2f(-e);
    for (int i = lane; i < c8; i += 64)
      split_store8<P>(yr + i * 8, cols, *reinterpret_cast<const f32x4*>(xr + i * 8), *reinterpret_cast<const f32x4*>(xr + i * 8 + 4),
                   scale);
  }
}

// ---- the weight gradients' operand: dW[n,k] = sum_m dY[m,n] X[m,k] contracts over the ROWS of dY, so the
// scale that can be undone after the product is one power of two per COLUMN n.  Three launches:
//   1. split_rows_colstats_f16x3_kernel: split_rows_f16x3_kernel's row split, statement for statement, by waves that walk
//      several rows (wave w of W takes rows w, w + W, ...) and keep, for the columns a lane owns, the running maximum of the
//      bit patterns of |x| and the fp32 sum in row order; each wave writes its two partial rows to the workspace
//      [2][W][cols] (maxima, then sums).  No atomics, no zero fill: every word read later is written here first.
//   2. colstats_finish_kernel: the partials in wave order -> col_exp[n] (row_exp on the column maximum), col_alpha[n] =
//      2^-e_n and the bias gradient db[n] = sum_m dY[m,n].
//   3. split_cols_f16x2_kernel: yc[m] = [hi | lo] of dY[m,n] 2^e_n, fp16 [rows][2 cols].
constexpr int COLSTAT_MAX_WAVES = 1024, COLSTAT_ROWS_PER_WAVE = 8;

inline int colstat_waves(int rows) {
  const int w = cdiv(rows, COLSTAT_ROWS_PER_WAVE);
  return cdiv(w < COLSTAT_MAX_WAVES ? w : COLSTAT_MAX_WAVES, 4) * 4;      // whole workgroups of 4 waves
}

__device__ __forceinline__ void colstat8(unsigned* mx, float* sm, const f32x4& a, const f32x4& b) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float fa = a[e], fb = b[e];
    const unsigned ua = __builtin_bit_cast(unsigned, fa) & 0x7fffffffu, ub = __builtin_bit_cast(unsigned, fb) & 0x7fffffffu;
    mx[e] = mx[e] > ua ? mx[e] : ua;
    mx[4 + e] = mx[4 + e] > ub ? mx[4 + e] : ub;
    sm[e] += fa;
    sm[4 + e] += fb;
  }
}

template <int NC, int P = 3>
__global__ void __launch_bounds__(256) split_rows_colstats_f16x3_kernel(const float* __restrict__ x, unsigned short* __restrict__ y,
                                                                        float* __restrict__ row_alpha, unsigned* __restrict__ pmax,
                                                                        float* __restrict__ psum, int rows, int cols, int ldx) {
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6), W = gridDim.x * 4;
  if (w >= rows) return;                                 // a wave without a row writes no partial (the finish counts min(W, rows))
  const int c8 = cols >> 3;
  unsigned* pm = pmax + (size_t)w * cols;
  float* ps = psum + (size_t)w * cols;
  if (NC > 0) {
    unsigned cm[NC > 0 ? NC : 1][8];
    float cs[NC > 0 ? NC : 1][8];
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int e = 0; e < 8; ++e) cm[c][e] = 0u, cs[c][e] = 0.f;
    for (int row = w; row < rows; row += W) {
      const float* xr = x + (size_t)row * ldx;
      unsigned short* yr = y + (size_t)row * P * cols;
      f32x4 a[NC > 0 ? NC : 1], b[NC > 0 ? NC : 1];
      unsigned m = 0u;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int i = lane + 64 * c, ic = i < c8 ? i : 0;
        a[c] = *reinterpret_cast<const f32x4*>(xr + ic * 8);
        b[c] = *reinterpret_cast<const f32x4*>(xr + ic * 8 + 4);
      }
#pragma unroll
      for (int c = 0; c < NC; ++c) m = absmax8(m, a[c], b[c]);
      const int e = row_exp(wave_umax_bits(m));
      const float scale = pow2f(e);
      if (lane == 0) row_alpha[row] = pow2f(-e);
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int i = lane + 64 * c;
        if (i < c8) split_store8<P>(yr + i * 8, cols, a[c], b[c], scale);
        colstat8(cm[c], cs[c], a[c], b[c]);              // (a chunk past the row holds chunk 0 again: never stored below)
      }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int i = lane + 64 * c;
      if (i < c8) {
        *reinterpret_cast<u32x4s*>(pm + i * 8) = u32x4s{cm[c][0], cm[c][1], cm[c][2], cm[c][3]};
        *reinterpret_cast<u32x4s*>(pm + i * 8 + 4) = u32x4s{cm[c][4], cm[c][5], cm[c][6], cm[c][7]};
        *reinterpret_cast<f32x4*>(ps + i * 8) = f32x4{cs[c][0], cs[c][1], cs[c][2], cs[c][3]};
        *reinterpret_cast<f32x4*>(ps + i * 8 + 4) = f32x4{cs[c][4], cs[c][5], cs[c][6], cs[c][7]};
      }
    }
  } else {
    // any width: the running values live in the wave's own partial rows (written by the first row, updated by the others;
    // a lane meets the same columns in every row, so its own earlier stores are all it reads back)
    bool first = true;
    for (int row = w; row < rows; row += W, first = false) {
      const float* xr = x + (size_t)row * ldx;
      unsigned short* yr = y + (size_t)row * P * cols;
      unsigned m = 0u;
      for (int i = lane; i < c8; i += 64)
        m = absmax8(m, *reinterpret_cast<const f32x4*>(xr + i * 8), *reinterpret_cast<const f32x4*>(xr + i * 8 + 4));
      const int e = row_exp(wave_umax_bits(m));
      const float scale = pow2f(e);
      if (lane == 0) row_alpha[row] = pow2f(-e);
      for (int i = lane; i < c8; i += 64) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(xr + i * 8), b = *reinterpret_cast<const f32x4*>(xr + i * 8 + 4);
        split_store8<P>(yr + i * 8, cols, a, b, scale);
        unsigned cm[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
        float cs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (!first) {
          const u32x4s m0 = *reinterpret_cast<const u32x4s*>(pm + i * 8), m1 = *reinterpret_cast<const u32x4s*>(pm + i * 8 + 4);
          const f32x4 s0 = *reinterpret_cast<const f32x4*>(ps + i * 8), s1 = *reinterpret_cast<const f32x4*>(ps + i * 8 + 4);
#pragma unroll
          for (int k = 0; k < 4; ++k) cm[k] = m0[k], cm[4 + k] = m1[k], cs[k] = s0[k], cs[4 + k] = s1[k];
        }
        colstat8(cm, cs, a, b);
        *reinterpret_cast<u32x4s*>(pm + i * 8) = u32x4s{cm[0], cm[1], cm[2], cm[3]};
        *reinterpret_cast<u32x4s*>(pm + i * 8 + 4) = u32x4s{cm[4], cm[5], cm[6], cm[7]};
        *reinterpret_cast<f32x4*>(ps + i * 8) = f32x4{cs[0], cs[1], cs[2], cs[3]};
        *reinterpret_cast<f32x4*>(ps + i * 8 + 4) = f32x4{cs[4], cs[5], cs[6], cs[7]};
      }
    }
  }
}

// 8 columns x 32 groups of partials per workgroup (cols / 8 workgroups: enough of them to hide the latency of the strided
// reads): group g folds partials g, g + 32, ... in order, then the threads of group 0 fold the 32 groups in order — one fixed
// sequence per column, the same in every run.
constexpr int FIN_COLS = 8, FIN_GROUPS = 32;
__global__ void __launch_bounds__(256) colstats_finish_kernel(const unsigned* __restrict__ pmax, const float* __restrict__ psum,
                                                              int* __restrict__ col_exp, float* __restrict__ col_alpha,
                                                              float* __restrict__ db, int nw, int cols) {
  static_assert(FIN_COLS * FIN_GROUPS == 256, "one thread per (column, group)");
  __shared__ unsigned smax[FIN_GROUPS][FIN_COLS];
  __shared__ float ssum[FIN_GROUPS][FIN_COLS];
  const int cl = threadIdx.x % FIN_COLS, g = threadIdx.x / FIN_COLS;
  const int col = blockIdx.x * FIN_COLS + cl;
  unsigned m = 0u;
  float s = 0.f;
  if (col < cols) {
#pragma unroll 4
    for (int w = g; w < nw; w += FIN_GROUPS) {
      const unsigned pm = pmax[(size_t)w * cols + col];
      m = m > pm ? m : pm;
      s += psum[(size_t)w * cols + col];
    }
  }
  smax[g][cl] = m;
  ssum[g][cl] = s;
  __syncthreads();
  if (g == 0 && col < cols) {
    for (int k = 1; k < FIN_GROUPS; ++k) {
      m = m > smax[k][cl] ? m : smax[k][cl];
      s += ssum[k][cl];
    }
    const int e = row_exp(m);
    col_exp[col] = e;
    col_alpha[col] = pow2f(-e);
    if (db) db[col] = s;
  }
}

// yc[m] = [hi | lo] of x[m,n] 2^e_n, 8 columns per thread: two 16-byte loads of x (and of the exponents), two 16-byte stores
__global__ void __launch_bounds__(256) split_cols_f16x2_kernel(const float* __restrict__ x, const int* __restrict__ col_exp,
                                                               unsigned short* __restrict__ yc, int rows, int cols, int ldx) {
  const int c8 = cols >> 3;
  const size_t total = (size_t)rows * c8;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % c8) * 8;
    const size_t r = i / c8;
    const f32x4 a = *reinterpret_cast<const f32x4*>(x + r * ldx + c);
    const f32x4 b = *reinterpret_cast<const f32x4*>(x + r * ldx + c + 4);
    const i32x4s ea = *reinterpret_cast<const i32x4s*>(col_exp + c), eb = *reinterpret_cast<const i32x4s*>(col_exp + c + 4);
    u16x8 hi, lo;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      unsigned short h0, l0, h1, l1;
      split1(a[e] * pow2f(ea[e]), h0, l0);
      split1(b[e] * pow2f(eb[e]), h1, l1);
      hi[e] = h0, lo[e] = l0, hi[4 + e] = h1, lo[4 + e] = l1;
    }
    unsigned short* yr = yc + r * 2 * cols + c;
    *reinterpret_cast<u16x8*>(yr) = hi;
    *reinterpret_cast<u16x8*>(yr + cols) = lo;
  }
}

// ---- the single pass: when the kernel that PRODUCED x left the column partials, the finish runs first and the
// column exponents are known before x is read; one wave per row then writes both splits from the same registers —
// split_rows_f16x3_kernel's row split, statement for statement, and split_cols_f16x2_kernel's statement for the same 8 columns.
__device__ __forceinline__ void split_cols_store8(unsigned short* yr, int cols, const f32x4& a, const f32x4& b,
                                                  const int* __restrict__ ce) {
  const i32x4s ea = *reinterpret_cast<const i32x4s*>(ce), eb = *reinterpret_cast<const i32x4s*>(ce + 4);
  u16x8 hi, lo;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    unsigned short h0, l0, h1, l1;
    split1(a[e] * pow2f(ea[e]), h0, l0);
    split1(b[e] * pow2f(eb[e]), h1, l1);
    hi[e] = h0, lo[e] = l0, hi[4 + e] = h1, lo[4 + e] = l1;
  }
  *reinterpret_cast<u16x8*>(yr) = hi;
  *reinterpret_cast<u16x8*>(yr + cols) = lo;
}

// split_store8 with non-temporal stores: the row split is read only by the data-gradient GEMM, which runs AFTER the weight
// gradient has read yc, so it should not push yc out of the cache on its way to memory
template <int P = 3>
__device__ __forceinline__ void split_store8_nt(unsigned short* yr, int cols, const f32x4& a, const f32x4& b, float scale) {
  u16x8 hi, lo;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    unsigned short h0, l0, h1, l1;
    split1(a[e] * scale, h0, l0);
    split1(b[e] * scale, h1, l1);
    hi[e] = h0, lo[e] = l0, hi[4 + e] = h1, lo[4 + e] = l1;
  }
  __builtin_nontemporal_store(hi, reinterpret_cast<u16x8*>(yr));
  __builtin_nontemporal_store(lo, reinterpret_cast<u16x8*>(yr + cols));
  if (P == 3) __builtin_nontemporal_store(hi, reinterpret_cast<u16x8*>(yr + 2 * cols));
}

template <int NC, int P = 3>
__global__ void __launch_bounds__(256) split_rows_cols_f16_kernel(const float* __restrict__ x, unsigned short* __restrict__ y,
                                                                  float* __restrict__ row_alpha, const int* __restrict__ col_exp,
                                                                  unsigned short* __restrict__ yc, int rows, int cols, int ldx) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int c8 = cols >> 3;
  const float* xr = x + (size_t)row * ldx;
  unsigned short* yr = y + (size_t)row * P * cols;
  unsigned short* ycr = yc + (size_t)row * 2 * cols;
  unsigned m = 0u;
  if (NC > 0) {
    f32x4 a[NC > 0 ? NC : 1], b[NC > 0 ? NC : 1];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int i = lane + 64 * c, ic = i < c8 ? i : 0;       // a chunk past the row re-reads chunk 0: same maximum
      a[c] = *reinterpret_cast<const f32x4*>(xr + ic * 8);
      b[c] = *reinterpret_cast<const f32x4*>(xr + ic * 8 + 4);
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) m = absmax8(m, a[c], b[c]);
    const int e = row_exp(wave_umax_bits(m));
    const float scale = pow2f(e);
    if (lane == 0) row_alpha[row] = pow2f(-e);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int i = lane + 64 * c;
      if (i < c8) {
        split_store8_nt<P>(yr + i * 8, cols, a[c], b[c], scale);
        split_cols_store8(ycr + i * 8, cols, a[c], b[c], col_exp + i * 8);
      }
    }
  } else {
    for (int i = lane; i < c8; i += 64)
      m = absmax8(m, *reinterpret_cast<const f32x4*>(xr + i * 8), *reinterpret_cast<const f32x4*>(xr + i * 8 + 4));
    const int e = row_exp(wave_umax_bits(m));
    const float scale = pow2f(e);
    if (lane == 0) row_alpha[row] = pow2f(-e);
    for (int i = lane; i < c8; i += 64) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(xr + i * 8), b = *reinterpret_cast<const f32x4*>(xr + i * 8 + 4);
      split_store8_nt<P>(yr + i * 8, cols, a, b, scale);
      split_cols_store8(ycr + i * 8, cols, a, b, col_exp + i * 8);
    }
  }
}

// ln_fwd_kernel (layernorm.hip) with the split [hi | lo | hi] of scale * LN(x) as its output, y [rows][3 D] fp16.  Loads,
// statistics and the normalisation are that kernel's, statement for statement; the fp32 result is pinned in a register before
// it is scaled and split, so that it is the value ln_fwd_kernel would have stored (no fusion of the affine step into the
// conversion, which would round once instead of twice).
template <int NC, bool EXACT, int P = 3>
__global__ void __launch_bounds__(256) ln_fwd_f16x3_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, unsigned short* __restrict__ y,
                                                           int rows, int D, float eps, float scale_v,
                                                           const float* __restrict__ scale_p, float* __restrict__ y32,
                                                           float* __restrict__ mean, float* __restrict__ rstd) {
  const float scale = scale_p ? *scale_p : scale_v;   // _dev entry: the scale lives in the device plan record
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int d4 = D >> 2;
  const f32x4* xr = reinterpret_cast<const f32x4*>(x + (size_t)row * D);
  f32x4 v[NC], g[NC], bt[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int i = lane + 64 * c, ic = (EXACT || i < d4) ? i : 0;
    v[c] = xr[ic];
    g[c] = reinterpret_cast<const f32x4*>(gamma)[ic];
    bt[c] = reinterpret_cast<const f32x4*>(beta)[ic];
  }
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    if (!EXACT && lane + 64 * c >= d4) v[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    s += (v[c][0] + v[c][1]) + (v[c][2] + v[c][3]);
  }
  const float mu = wave_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    if (EXACT || lane + 64 * c < d4) {
      f32x4 d = v[c] - mu;
      q += (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
    }
  }
  const float rs = rsqrtf(wave_sum(q) / (float)D + eps);
  if (lane == 0) {
    if (mean) mean[row] = mu;
    if (rstd) rstd[row] = rs;
  }
  unsigned short* yr = y + (size_t)row * P * D;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int i = lane + 64 * c;
    if (EXACT || i < d4) {
      f32x4 o = (v[c] - mu) * rs * g[c] + bt[c];
      if (y32) reinterpret_cast<f32x4*>(y32 + (size_t)row * D)[i] = o;   // ln_fwd_kernel's output, for the backward
      u16x4 hi, lo;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float oe = o[e];
        asm volatile("" : "+v"(oe));
        unsigned short h0, l0;
        split1(oe * scale, h0, l0);
        hi[e] = h0, lo[e] = l0;
      }
      *reinterpret_cast<u16x4*>(yr + i * 4) = hi;
      *reinterpret_cast<u16x4*>(yr + D + i * 4) = lo;
      if (P == 3) *reinterpret_cast<u16x4*>(yr + 2 * D + i * 4) = hi;
    }
  }
}

// g = quick_gelu(h), the statement of the GEMM epilogues (quick_gelu_f on the fp32 pre-activation they store as h32): the
// rematerialisation of an fp32 g the forward did not keep.  4 values per thread.
__global__ void __launch_bounds__(256) quick_gelu_kernel(const float* __restrict__ h, float* __restrict__ g, size_t n4) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    f32x4 v = reinterpret_cast<const f32x4*>(h)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = quick_gelu_f(v[e]);
    reinterpret_cast<f32x4*>(g)[i] = v;
  }
}

inline bool pow2(float s) { return s > 0.f && s - s == 0.f && (__builtin_bit_cast(unsigned int, s) & 0x007fffffu) == 0; }

// ------------------------------------------------------------------------------------------------------------------------
// Device-side plan for a tower whose weights CHANGE (the student's vision tower): the statistics of the
// encoder-layer weights, the power-of-two scales derived from them and the [hi|hi|lo] copies of the scaled weights are all
// made on the device, three launches over a table of records built once.  Nothing is read back by the host.
struct Split16Ref {          // 48 bytes (dclip_split16_record_bytes)
  const float* src;          // fp32 [rows][cols], cols % 8 == 0, 16-byte aligned
  unsigned short* dst;       // fp16 [rows][3 cols], the [hi|hi|lo] split of src * plan scale; null = statistics only
  int rows, cols;
  int layer;                 // which plan record
  int max_slot;              // statistic (0..11, engine._SPLIT16_STATS order) receiving max|x|
  int l1_slot;               // statistic receiving the maximum row L1 norm over rows >= l1_row0, or -1
  int l1_row0;
  int scale_slot;            // float of the plan record holding the weight scale (dst != null)
  int tile0;                 // first tile (SPLIT16_TILE_ROWS rows) of this tensor
};
static_assert(sizeof(Split16Ref) == 48, "Split16Ref layout");

constexpr int SPLIT16_TILE_ROWS = 32;
constexpr int PLAN_FLOATS = 32;   // per layer: [0..3] activation scales ln1 ctx ln2 g | [4..7] weight scales qkv out fc1 fc2 |
                                  // [8..11] alphas qkv out fc1 fc2 | [12] flags | [16..27] the twelve statistics |
                                  // [28..31] 2^-f qkv out fc1 fc2, the alphas of the backward's data-gradient GEMMs
constexpr int NSTAT = 12;

__device__ __forceinline__ const Split16Ref& find_ref(const Split16Ref* refs, int n, int tile) {
  int lo = 0, hi = n - 1;                              // last record with tile0 <= tile (uniform: scalar code)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (refs[mid].tile0 <= tile) lo = mid;
    else hi = mid - 1;
  }
  return refs[lo];
}

__device__ __forceinline__ unsigned wave_umax(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned w = (unsigned)__shfl_xor((int)v, o, 64);
    v = v > w ? v : w;
  }
  return v;
}

// max|x| and (for the rows that count) the largest row L1 norm of every record, one wave per row, into stats[layer][12] as
// the BIT PATTERNS of non-negative floats under an integer atomic max: the order of the updates cannot matter, NaN (above
// inf as an integer) survives, and a row sum is one fixed sequence (a lane adds its chunks in order, then the xor tree), so
// the result is the same in every run.  The plan kernel consumes the accumulators and clears them for the next call.
__global__ void __launch_bounds__(256) split16_stats_kernel(const Split16Ref* __restrict__ refs, int nrefs,
                                                            unsigned* __restrict__ stats) {
  const Split16Ref t = find_ref(refs, nrefs, blockIdx.x);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r0 = ((int)blockIdx.x - t.tile0) * SPLIT16_TILE_ROWS;
  const int c4 = t.cols >> 2;
  unsigned mx = 0u, l1 = 0u;
  for (int r = r0 + wave; r < min(r0 + SPLIT16_TILE_ROWS, t.rows); r += 4) {
    const f32x4* xr = reinterpret_cast<const f32x4*>(t.src + (size_t)r * t.cols);
    float s = 0.f;
    unsigned m = 0u;
    for (int i = lane; i < c4; i += 64) {
      const f32x4 v = xr[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float a = __builtin_fabsf(v[e]);
        const unsigned b = __builtin_bit_cast(unsigned, a);
        m = m > b ? m : b;
      }
      s += (__builtin_fabsf(v[0]) + __builtin_fabsf(v[1])) + (__builtin_fabsf(v[2]) + __builtin_fabsf(v[3]));
    }
    mx = mx > m ? mx : m;
    if (t.l1_slot >= 0 && r >= t.l1_row0) {          // uniform per wave
      const unsigned b = __builtin_bit_cast(unsigned, __builtin_fabsf(wave_sum(s)));
      l1 = l1 > b ? l1 : b;
    }
  }
  mx = wave_umax(mx);
  if (lane == 0) {
    atomicMax(stats + t.layer * NSTAT + t.max_slot, mx);
    if (t.l1_slot >= 0) atomicMax(stats + t.layer * NSTAT + t.l1_slot, l1);
  }
}

// engine.split16_weight_exp: f with max|W| 2^f in [2^13, 2^14); 0 for an all-zero (or, flagged, a non-finite) weight
__device__ int weight_exp(double max_abs, unsigned& flags) {
  if (!(max_abs - max_abs == 0.0)) {
    flags |= 2u;
    return 0;
  }
  if (max_abs == 0.0) return 0;
  int x;
  frexp(max_abs, &x);
  return 14 - x;
}

// engine.split16_act_exp without its fall-back: the largest e <= 24 with bound 2^e <= 2^14; where the host function returns
// None (e < -14, or the bound is not finite) the flag is set and e is what the bound asks for (0 when it is not finite).
__device__ int act_exp(double bound, unsigned& flags) {
  if (!(bound - bound == 0.0) || bound < 0.0) {
    flags |= 2u;
    return 0;
  }
  if (bound == 0.0) return 24;
  int x;
  const double m = frexp(bound, &x);
  const int e = 14 - (m == 0.5 ? x - 1 : x);
  if (e < -14) flags |= 1u;
  return e < 24 ? e : 24;
}

// One thread per layer: statistics -> bounds (engine.split16_layer_bounds, in double, products and sums rounded one by one as
// the host's are) -> exponents -> the plan record; then the accumulators are cleared for the next statistics launch.
__global__ void split16_plan_kernel(unsigned* __restrict__ stats, float* __restrict__ plan, int nlayers, double sqrt_d) {
#pragma clang fp contract(off)
  const int l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= nlayers) return;
  double st[NSTAT];
  float* rec = plan + (size_t)l * PLAN_FLOATS;
  for (int i = 0; i < NSTAT; ++i) {
    const float f = __builtin_bit_cast(float, stats[l * NSTAT + i]);
    st[i] = (double)f;
    rec[16 + i] = f;
    stats[l * NSTAT + i] = 0u;
  }
  // ln1_w ln1_b v_l1 v_b ln2_w ln2_b fc1_l1 fc1_b qkv out fc1 fc2
  unsigned flags = 0u;
  const double b_ln1 = __dadd_rn(__dmul_rn(st[0], sqrt_d), st[1]);
  const double b_ln2 = __dadd_rn(__dmul_rn(st[4], sqrt_d), st[5]);
  const double b_ctx = __dadd_rn(__dmul_rn(b_ln1, st[2]), st[3]);
  const double b_g = __dadd_rn(__dmul_rn(b_ln2, st[6]), st[7]);
  int e[4] = {act_exp(b_ln1, flags), act_exp(b_ctx, flags), act_exp(b_ln2, flags), act_exp(b_g, flags)};
  int f[4];
  for (int i = 0; i < 4; ++i) f[i] = weight_exp(st[8 + i], flags);
  for (int i = 0; i < 4; ++i) {
    // a scale outside fp32's normal range (a bound beyond 2^140, a weight below 2^-113) is clamped and flagged
    if (e[i] < -126) e[i] = -126, flags |= 4u;
    if (f[i] > 127) f[i] = 127, flags |= 4u;
    if (-(e[i] + f[i]) > 127 || -(e[i] + f[i]) < -126) flags |= 4u;
    rec[i] = pow2f(e[i]);
    rec[4 + i] = pow2f(f[i]);
    rec[8 + i] = pow2f(-(e[i] + f[i]));
  }
  rec[12] = __builtin_bit_cast(float, flags);
  rec[13] = rec[14] = rec[15] = 0.f;
  for (int i = 0; i < 4; ++i) rec[28 + i] = pow2f(-f[i]);   // the data-gradient GEMMs' alpha: the weight scale alone (§9e)
}

// [hi|hi|lo] of src * (the plan's scale for that weight) for every record with a destination: split_f16x3_kernel<1>'s
// arithmetic, 8 columns per thread, one tile of rows per workgroup.
__global__ void __launch_bounds__(256) split16_weights_kernel(const Split16Ref* __restrict__ refs, int nrefs,
                                                              const float* __restrict__ plan) {
  const Split16Ref t = find_ref(refs, nrefs, blockIdx.x);
  if (!t.dst) return;                                  // uniform
  const float scale = plan[(size_t)t.layer * PLAN_FLOATS + t.scale_slot];
  const int r0 = ((int)blockIdx.x - t.tile0) * SPLIT16_TILE_ROWS;
  const int nr = min(SPLIT16_TILE_ROWS, t.rows - r0);
  const int c8 = t.cols >> 3;
  for (int i = threadIdx.x; i < nr * c8; i += 256) {
    const int c = (i % c8) * 8;
    const size_t r = (size_t)(r0 + i / c8);
    const f32x4 a = *reinterpret_cast<const f32x4*>(t.src + r * t.cols + c);
    const f32x4 b = *reinterpret_cast<const f32x4*>(t.src + r * t.cols + c + 4);
    u16x8 hi, lo;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      unsigned short h0, l0, h1, l1;
      split1(a[e] * scale, h0, l0);
      split1(b[e] * scale, h1, l1);
      hi[e] = h0, lo[e] = l0, hi[4 + e] = h1, lo[4 + e] = l1;
    }
    unsigned short* yr = t.dst + r * 3 * t.cols + c;
    *reinterpret_cast<u16x8*>(yr) = hi;
    *reinterpret_cast<u16x8*>(yr + t.cols) = hi;
    *reinterpret_cast<u16x8*>(yr + 2 * t.cols) = lo;
  }
}

// split16_weights_kernel that also writes the transposed copies (a kernel of its own: the one above stays what it was).  Same
// arithmetic, 8 columns per thread, one tile of 32 rows per workgroup, 64 columns at a time.  dst_t (one entry per record,
// null = none): the same pieces TRANSPOSED, [cols][3 rows] = [hi|hi|lo] of (src scale)^T — the weight operand of the
// backward's data-gradient GEMMs — through an LDS transpose, 8 rows (16 bytes) per store; rows % 8 == 0 there.
__global__ void __launch_bounds__(256) split16_weights_t_kernel(const Split16Ref* __restrict__ refs, int nrefs,
                                                              const float* __restrict__ plan,
                                                              unsigned short* const* __restrict__ dst_t) {
  constexpr int TR = SPLIT16_TILE_ROWS, LDT = TR + 8;      // LDS row of a column: 32 values + 8 of padding (80 bytes)
  static_assert(TR == 32, "256 threads = 32 rows x 8 column groups");
  __shared__ __attribute__((aligned(16))) unsigned short th[64 * LDT], tl[64 * LDT];
  const int ref = (int)(&find_ref(refs, nrefs, blockIdx.x) - refs);
  const Split16Ref t = refs[ref];
  if (!t.dst) return;                                  // uniform
  unsigned short* dt = dst_t ? dst_t[ref] : nullptr;   // uniform
  const float scale = plan[(size_t)t.layer * PLAN_FLOATS + t.scale_slot];
  const int r0 = ((int)blockIdx.x - t.tile0) * TR;
  const int lr = threadIdx.x >> 3, cg = threadIdx.x & 7;
  const size_t r = (size_t)(r0 + lr);
  const bool rok = r0 + lr < t.rows;
  for (int c0 = 0; c0 < t.cols; c0 += 64) {
    const int c = c0 + cg * 8;
    u16x8 hi = {0, 0, 0, 0, 0, 0, 0, 0}, lo = hi;
    if (rok && c < t.cols) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(t.src + r * t.cols + c);
      const f32x4 b = *reinterpret_cast<const f32x4*>(t.src + r * t.cols + c + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        unsigned short h0, l0, h1, l1;
        split1(a[e] * scale, h0, l0);
        split1(b[e] * scale, h1, l1);
        hi[e] = h0, lo[e] = l0, hi[4 + e] = h1, lo[4 + e] = l1;
      }
      unsigned short* yr = t.dst + r * 3 * t.cols + c;
      *reinterpret_cast<u16x8*>(yr) = hi;
      *reinterpret_cast<u16x8*>(yr + t.cols) = hi;
      *reinterpret_cast<u16x8*>(yr + 2 * t.cols) = lo;
    }
    if (!dt) continue;                                 // uniform (a record without a transposed copy)
    __syncthreads();                                   // the previous chunk's reads of th / tl are done
#pragma unroll
    for (int e = 0; e < 8; ++e) th[(cg * 8 + e) * LDT + lr] = hi[e], tl[(cg * 8 + e) * LDT + lr] = lo[e];
    __syncthreads();
    const int tc = threadIdx.x >> 2, rg = (threadIdx.x & 3) * 8;   // column of the chunk, 8 rows of the tile
    if (c0 + tc < t.cols && r0 + rg < t.rows) {        // rows % 8 == 0: a group of 8 rows is inside or outside as a whole
      const u16x8 h = *reinterpret_cast<const u16x8*>(th + tc * LDT + rg), l = *reinterpret_cast<const u16x8*>(tl + tc * LDT + rg);
      unsigned short* yc = dt + (size_t)(c0 + tc) * 3 * t.rows + r0 + rg;
      *reinterpret_cast<u16x8*>(yc) = h;
      *reinterpret_cast<u16x8*>(yc + t.rows) = h;
      *reinterpret_cast<u16x8*>(yc + 2 * t.rows) = l;
    }
  }
}

int split_launch(const char* name, const float* x, void* y, int rows, int cols, int ldx, int ldy, float scale,
                 const float* scale_p, int order, void* stream) {
  const size_t work = (size_t)rows * (cols / 8);
  const size_t blocks = (work + 255) / 256;
  const dim3 grid((unsigned)(blocks < 1 ? 1 : (blocks > 8192 ? 8192 : blocks)));
  hipStream_t st = (hipStream_t)stream;
  if (order == 0)
    hipLaunchKernelGGL(split_f16x3_kernel<0>, grid, dim3(256), 0, st, x, (unsigned short*)y, rows, cols, ldx, ldy, scale, scale_p);
  else if (order == 1)
    hipLaunchKernelGGL(split_f16x3_kernel<1>, grid, dim3(256), 0, st, x, (unsigned short*)y, rows, cols, ldx, ldy, scale, scale_p);
  else
    hipLaunchKernelGGL(split_f16x3_kernel<2>, grid, dim3(256), 0, st, x, (unsigned short*)y, rows, cols, ldx, ldy, scale, scale_p);
  DCLIP_CHECK_LAUNCH_V(name, order == 1 ? ".weight" : ".act");
  return DCLIP_OK;
}

int split_rows_launch(const char* name, const float* x, void* y, float* row_alpha, int rows, int cols, int ldx, int pieces,
                      void* stream) {
  dim3 grid(cdiv(rows, 4)), block(256);
  hipStream_t st = (hipStream_t)stream;
  unsigned short* yy = (unsigned short*)y;
  const int nc = cdiv(cols / 8, 64);
  const char* variant;
#define SPLITROWS(NC)                                                                                               \
  do {                                                                                                              \
    if (pieces == 2)                                                                                                \
      hipLaunchKernelGGL((split_rows_f16x3_kernel<NC, 2>), grid, block, 0, st, x, yy, row_alpha, rows, cols, ldx); \
    else                                                                                                            \
      hipLaunchKernelGGL((split_rows_f16x3_kernel<NC>), grid, block, 0, st, x, yy, row_alpha, rows, cols, ldx);    \
    variant = (NC) ? ".regs.nc" #NC : ".cached";                                                                    \
  } while (0)
  if (nc <= 1) SPLITROWS(1);
  else if (nc == 2) SPLITROWS(2);
  else if (nc == 3) SPLITROWS(3);
  else if (nc == 4) SPLITROWS(4);
  else if (nc == 5) SPLITROWS(5);
  else if (nc == 6) SPLITROWS(6);
  else SPLITROWS(0);
#undef SPLITROWS
  DCLIP_CHECK_LAUNCH_V(name, variant);
  return DCLIP_OK;
}

int split_rows_colstats_launch(const char* name, const float* x, void* y, float* row_alpha, unsigned* pmax, float* psum, int rows,
                               int cols, int ldx, int pieces, void* stream) {
  dim3 grid(colstat_waves(rows) / 4), block(256);
  hipStream_t st = (hipStream_t)stream;
  unsigned short* yy = (unsigned short*)y;
  const int nc = cdiv(cols / 8, 64);
  const char* variant;
#define SPLITROWSC(NC)                                                                                                        \
  do {                                                                                                                        \
    if (pieces == 2)                                                                                                          \
      hipLaunchKernelGGL((split_rows_colstats_f16x3_kernel<NC, 2>), grid, block, 0, st, x, yy, row_alpha, pmax, psum, rows,   \
                         cols, ldx);                                                                                          \
    else                                                                                                                      \
      hipLaunchKernelGGL((split_rows_colstats_f16x3_kernel<NC>), grid, block, 0, st, x, yy, row_alpha, pmax, psum, rows,      \
                         cols, ldx);                                                                                          \
    variant = (NC) ? ".regs.nc" #NC : ".cached";                                                                              \
  } while (0)
  if (nc <= 1) SPLITROWSC(1);
  else if (nc == 2) SPLITROWSC(2);
  else if (nc == 3) SPLITROWSC(3);
  else if (nc == 4) SPLITROWSC(4);
  else if (nc == 5) SPLITROWSC(5);
  else if (nc == 6) SPLITROWSC(6);
  else SPLITROWSC(0);
#undef SPLITROWSC
  DCLIP_CHECK_LAUNCH_V(name, variant);
  dclip_note_first_launch(name, variant);   // .finish and .cols overwrite the name above
  return DCLIP_OK;
}

int split_rows_cols_launch(const char* name, const float* x, void* y, float* row_alpha, const int* col_exp, void* yc, int rows,
                           int cols, int ldx, int pieces, void* stream) {
  dim3 grid(cdiv(rows, 4)), block(256);
  hipStream_t st = (hipStream_t)stream;
  unsigned short *yy = (unsigned short*)y, *yyc = (unsigned short*)yc;
  const int nc = cdiv(cols / 8, 64);
  const char* variant;
#define SPLITROWSCOLS(NC)                                                                                                          \
  do {                                                                                                                             \
    if (pieces == 2)                                                                                                               \
      hipLaunchKernelGGL((split_rows_cols_f16_kernel<NC, 2>), grid, block, 0, st, x, yy, row_alpha, col_exp, yyc, rows, cols, ldx); \
    else                                                                                                                           \
      hipLaunchKernelGGL((split_rows_cols_f16_kernel<NC>), grid, block, 0, st, x, yy, row_alpha, col_exp, yyc, rows, cols, ldx);   \
    variant = (NC) ? ".regs.nc" #NC : ".cached";                                                                                   \
  } while (0)
  if (nc <= 1) SPLITROWSCOLS(1);
  else if (nc == 2) SPLITROWSCOLS(2);
  else if (nc == 3) SPLITROWSCOLS(3);
  else if (nc == 4) SPLITROWSCOLS(4);
  else if (nc == 5) SPLITROWSCOLS(5);
  else if (nc == 6) SPLITROWSCOLS(6);
  else SPLITROWSCOLS(0);
#undef SPLITROWSCOLS
  DCLIP_CHECK_LAUNCH_V(name, variant);
  return DCLIP_OK;
}

int ln_launch(const char* name, const float* x, const float* gamma, const float* beta, void* y, int rows, int D, float eps,
              float scale, const float* scale_p, float* y32, float* mean, float* rstd, void* stream, int pieces = 3) {
  dim3 grid(cdiv(rows, 4)), block(256);
  hipStream_t st = (hipStream_t)stream;
  const int nc = cdiv(D / 4, 64);
  unsigned short* yy = (unsigned short*)y;
  const char* variant;
#define LN16X3(NC, EX)                                                                                                      \
  do {                                                                                                                      \
    if (pieces == 2)                                                                                                        \
      hipLaunchKernelGGL((ln_fwd_f16x3_kernel<NC, EX, 2>), grid, block, 0, st, x, gamma, beta, yy, rows, D, eps, scale,     \
                         scale_p, y32, mean, rstd);                                                                         \
    else                                                                                                                    \
      hipLaunchKernelGGL((ln_fwd_f16x3_kernel<NC, EX>), grid, block, 0, st, x, gamma, beta, yy, rows, D, eps, scale,        \
                         scale_p, y32, mean, rstd);                                                                         \
    variant = (EX) ? ".nc" #NC ".exact" : ".nc" #NC;                                                                        \
  } while (0)
  if (D == 512) LN16X3(2, true);
  else if (D == 768) LN16X3(3, true);
  else if (D == 1024) LN16X3(4, true);
  else if (nc <= 1) LN16X3(1, false);
  else if (nc == 2) LN16X3(2, false);
  else if (nc == 3) LN16X3(3, false);
  else if (nc == 4) LN16X3(4, false);
  else LN16X3(8, false);
#undef LN16X3
  DCLIP_CHECK_LAUNCH_V(name, variant);
  return DCLIP_OK;
}

}  // namespace

DCLIP_API int dclip_split_f32_f16x3(const float* x, void* y, int rows, int cols, int ldx, int ldy, float scale, int order,
                                    void* stream) {
  DCLIP_REQUIRE(x && y && rows > 0 && cols > 0, "split_f32_f16x3: bad arguments");
  DCLIP_REQUIRE(cols % 8 == 0, "split_f32_f16x3: cols=%d must be a multiple of 8", cols);
  DCLIP_REQUIRE(ldx >= cols && ldx % 4 == 0 && ldy % 8 == 0 && (long)ldy >= 3L * cols,
                "split_f32_f16x3: ldx (multiple of 4, >= cols) / ldy (multiple of 8, >= 3 cols)");
  DCLIP_REQUIRE(((uintptr_t)x | (uintptr_t)y) % 16 == 0, "split_f32_f16x3: operands must be 16-byte aligned");
  DCLIP_REQUIRE(order == 0 || order == 1, "split_f32_f16x3: order is 0 ([hi|lo|hi]) or 1 ([hi|hi|lo])");
  DCLIP_REQUIRE(pow2(scale), "split_f32_f16x3: scale must be a power of two");
  return split_launch("split_f32_f16x3", x, y, rows, cols, ldx, ldy, scale, nullptr, order, stream);
}

// dclip_split_f32_f16x3 with the scale in device memory (a float of the plan record)
DCLIP_API int dclip_split_f32_f16x3_dev(const float* x, void* y, int rows, int cols, int ldx, int ldy, const float* scale,
                                        int order, void* stream) {
  DCLIP_REQUIRE(x && y && scale && rows > 0 && cols > 0, "split_f32_f16x3_dev: bad arguments");
  DCLIP_REQUIRE(cols % 8 == 0, "split_f32_f16x3_dev: cols=%d must be a multiple of 8", cols);
  DCLIP_REQUIRE(ldx >= cols && ldx % 4 == 0 && ldy % 8 == 0 && (long)ldy >= 3L * cols,
                "split_f32_f16x3_dev: ldx (multiple of 4, >= cols) / ldy (multiple of 8, >= 3 cols)");
  DCLIP_REQUIRE(((uintptr_t)x | (uintptr_t)y) % 16 == 0 && (uintptr_t)scale % 4 == 0, "split_f32_f16x3_dev: alignment");
  DCLIP_REQUIRE(order == 0 || order == 1, "split_f32_f16x3_dev: order is 0 ([hi|lo|hi]) or 1 ([hi|hi|lo])");
  return split_launch("split_f32_f16x3_dev", x, y, rows, cols, ldx, ldy, 1.f, scale, order, stream);
}

// The two-piece form of the order-0 split: y [rows][ldy >= 2 cols] = [hi|lo], bit-equal to the first two pieces of
// dclip_split_f32_f16x3(order 0) / _dev; nothing past column 2 cols of a row is written.  scale_dev (device, may be null) takes
// the place of `scale` when given.
DCLIP_API int dclip_split_f32_f16x2(const float* x, void* y, int rows, int cols, int ldx, int ldy, float scale, const float* scale_dev,
                                    void* stream) {
  DCLIP_REQUIRE(x && y && rows > 0 && cols > 0, "split_f32_f16x2: bad arguments");
  DCLIP_REQUIRE(cols % 8 == 0, "split_f32_f16x2: cols=%d must be a multiple of 8", cols);
  DCLIP_REQUIRE(ldx >= cols && ldx % 4 == 0 && ldy % 8 == 0 && (long)ldy >= 2L * cols,
                "split_f32_f16x2: ldx (multiple of 4, >= cols) / ldy (multiple of 8, >= 2 cols)");
  DCLIP_REQUIRE(((uintptr_t)x | (uintptr_t)y) % 16 == 0 && (uintptr_t)scale_dev % 4 == 0, "split_f32_f16x2: alignment");
  DCLIP_REQUIRE(scale_dev || pow2(scale), "split_f32_f16x2: scale must be a power of two");
  // (the launch is recorded under the three-piece twin's name: the same call site of the step, the same kernel but for a store)
  return split_launch(scale_dev ? "split_f32_f16x3_dev" : "split_f32_f16x3", x, y, rows, cols, ldx, ldy, scale_dev ? 1.f : scale, scale_dev, 2,
                      stream);
}

// x fp32 [rows][ldx >= cols] -> y fp16 [rows][3 cols] = [hi|lo|hi] of x[m] 2^e_m and row_alpha[m] = 2^-e_m, e_m from the row's
// own maximum (split_rows_f16x3_kernel).  One read of x for cols <= 3072 (the row stays in registers); wider rows are read twice,
// the second time from the cache.
namespace {
int split_rows_entry(const char* name, const float* x, void* y, float* row_alpha, int rows, int cols, int ldx, int pieces,
                     void* stream) {
  DCLIP_REQUIRE(x && y && row_alpha && rows > 0 && cols > 0, "%s: bad arguments", name);
  DCLIP_REQUIRE(cols % 8 == 0, "%s: cols=%d must be a multiple of 8", name, cols);
  DCLIP_REQUIRE(ldx >= cols && ldx % 4 == 0, "%s: ldx must be a multiple of 4 and >= cols", name);
  DCLIP_REQUIRE(((uintptr_t)x | (uintptr_t)y) % 16 == 0 && (uintptr_t)row_alpha % 4 == 0, "%s: alignment", name);
  return split_rows_launch(name, x, y, row_alpha, rows, cols, ldx, pieces, stream);
}
}  // namespace

DCLIP_API int dclip_split_f32_f16x3_rows(const float* x, void* y, float* row_alpha, int rows, int cols, int ldx, void* stream) {
  return split_rows_entry("split_f32_f16x3_rows", x, y, row_alpha, rows, cols, ldx, 3, stream);
}

// The two-piece form: y fp16 [rows][2 cols] = [hi|lo], bit-equal to the first two pieces of the entry above;
// row_alpha as there.  Its launches are recorded under that entry's name, as are those of the other two-piece forms below.
DCLIP_API int dclip_split_f32_f16x2_rows(const float* x, void* y, float* row_alpha, int rows, int cols, int ldx, void* stream) {
  return split_rows_entry("split_f32_f16x3_rows", x, y, row_alpha, rows, cols, ldx, 2, stream);
}

// dclip_split_f32_f16x3_rows (y and row_alpha bit-equal to it) that in the same pass over x takes the column statistics, and
// from them: col_exp[n] = the row rule applied to max|x[:,n]|, col_alpha[n] = 2^-col_exp[n], db[n] = sum_m x[m,n]
// (may be null) and yc fp16 [rows][2 cols] = [hi|lo] of x[m,n] 2^col_exp[n], the token-major operand of the segmented weight-
// gradient GEMM.  Three launches, no atomics, the same bits in every run.  workspace: dclip_split_f32_f16x3_rows_colstats_workspace.
DCLIP_API size_t dclip_split_f32_f16x3_rows_colstats_workspace(int rows, int cols) {
  if (rows <= 0 || cols <= 0) return 0;
  return (size_t)2 * colstat_waves(rows) * cols * sizeof(float);
}

namespace {
int split_rows_colstats_entry(const char* name, const float* x, void* y, float* row_alpha, void* yc, int* col_exp, float* col_alpha,
                              float* db, int rows, int cols, int ldx, void* workspace, size_t workspace_bytes, int pieces,
                              void* stream) {
  dclip_note_first_launch("", "");                     // a refused call leaves no earlier call's instance standing
  DCLIP_REQUIRE(x && y && row_alpha && yc && col_exp && col_alpha && rows > 0 && cols > 0, "%s: bad arguments", name);
  DCLIP_REQUIRE(cols % 8 == 0, "%s: cols=%d must be a multiple of 8", name, cols);
  DCLIP_REQUIRE(ldx >= cols && ldx % 4 == 0, "%s: ldx must be a multiple of 4 and >= cols", name);
  DCLIP_REQUIRE(((uintptr_t)x | (uintptr_t)y | (uintptr_t)yc | (uintptr_t)col_exp | (uintptr_t)workspace) % 16 == 0 &&
                    ((uintptr_t)row_alpha | (uintptr_t)col_alpha | (uintptr_t)db) % 4 == 0,
                "%s: alignment", name);
  const size_t need = dclip_split_f32_f16x3_rows_colstats_workspace(rows, cols);
  if (!workspace || workspace_bytes < need) {
    dclip_set_error("%s: needs %zu workspace bytes, got %zu", name, need, workspace_bytes);
    return DCLIP_EWORKSPACE;
  }
  const int W = colstat_waves(rows);
  unsigned* pmax = (unsigned*)workspace;
  float* psum = (float*)workspace + (size_t)W * cols;
  const int rc = split_rows_colstats_launch(name, x, y, row_alpha, pmax, psum, rows, cols, ldx, pieces, stream);
  if (rc != DCLIP_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(colstats_finish_kernel, dim3(cdiv(cols, FIN_COLS)), dim3(256), 0, st, (const unsigned*)pmax, (const float*)psum, col_exp,
                     col_alpha, db, W < rows ? W : rows, cols);
  DCLIP_CHECK_LAUNCH_V(name, ".finish");
  const size_t blocks = ((size_t)rows * (cols / 8) + 255) / 256;
  hipLaunchKernelGGL(split_cols_f16x2_kernel, dim3((unsigned)(blocks > 8192 ? 8192 : blocks)), dim3(256), 0, st, x, (const int*)col_exp,
                     (unsigned short*)yc, rows, cols, ldx);
  DCLIP_CHECK_LAUNCH_V(name, ".cols");
  return DCLIP_OK;
}
}  // namespace

DCLIP_API int dclip_split_f32_f16x3_rows_colstats(const float* x, void* y, float* row_alpha, void* yc, int* col_exp, float* col_alpha,
                                                  float* db, int rows, int cols, int ldx, void* workspace, size_t workspace_bytes,
                                                  void* stream) {
  return split_rows_colstats_entry("split_f32_f16x3_rows_colstats", x, y, row_alpha, yc, col_exp, col_alpha, db, rows, cols, ldx,
                                   workspace, workspace_bytes, 3, stream);
}

// The two-piece form: y fp16 [rows][2 cols] = [hi|lo], bit-equal to the first two pieces of the entry above; every
// other output and the workspace as there.
DCLIP_API int dclip_split_f32_f16x2_rows_colstats(const float* x, void* y, float* row_alpha, void* yc, int* col_exp, float* col_alpha,
                                                  float* db, int rows, int cols, int ldx, void* workspace, size_t workspace_bytes,
                                                  void* stream) {
  return split_rows_colstats_entry("split_f32_f16x3_rows_colstats", x, y, row_alpha, yc, col_exp, col_alpha, db, rows, cols, ldx,
                                   workspace, workspace_bytes, 2, stream);
}

// dclip_split_f32_f16x3_rows_colstats when the kernel that produced x has left the column partials: pmax [P][cols]
// (bit patterns of |x| maxima) and psum [P][cols] (fp32 sums), every word written.  Two launches: the finish over the P partial
// rows, then ONE pass over x that writes both splits.  y, row_alpha, col_exp, col_alpha and yc are bit-equal to the three-launch
// entry's on the same x (a maximum does not depend on how the rows were grouped); db is another association of the same sum.
namespace {
int split_rows_cols_stats_entry(const char* name, const float* x, void* y, float* row_alpha, void* yc, int* col_exp, float* col_alpha,
                                float* db, const void* pmax, const float* psum, int P, int rows, int cols, int ldx, int pieces,
                                void* stream) {
  dclip_note_first_launch("", "");
  DCLIP_REQUIRE(x && y && row_alpha && yc && col_exp && col_alpha && pmax && psum && P > 0 && rows > 0 && cols > 0,
                "%s: bad arguments", name);
  DCLIP_REQUIRE(cols % 8 == 0, "%s: cols=%d must be a multiple of 8", name, cols);
  DCLIP_REQUIRE(ldx >= cols && ldx % 4 == 0, "%s: ldx must be a multiple of 4 and >= cols", name);
  DCLIP_REQUIRE(((uintptr_t)x | (uintptr_t)y | (uintptr_t)yc | (uintptr_t)col_exp) % 16 == 0 &&
                    ((uintptr_t)row_alpha | (uintptr_t)col_alpha | (uintptr_t)db | (uintptr_t)pmax | (uintptr_t)psum) % 4 == 0,
                "%s: alignment", name);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(colstats_finish_kernel, dim3(cdiv(cols, FIN_COLS)), dim3(256), 0, st, (const unsigned*)pmax, psum, col_exp, col_alpha,
                     db, P, cols);
  DCLIP_CHECK_LAUNCH_V(name, ".finish");
  dclip_note_first_launch(name, ".finish");
  return split_rows_cols_launch(name, x, y, row_alpha, (const int*)col_exp, yc, rows, cols, ldx, pieces, stream);
}
}  // namespace

DCLIP_API int dclip_split_f32_f16x3_rows_cols_stats(const float* x, void* y, float* row_alpha, void* yc, int* col_exp, float* col_alpha,
                                                    float* db, const void* pmax, const float* psum, int P, int rows, int cols, int ldx,
                                                    void* stream) {
  return split_rows_cols_stats_entry("split_f32_f16x3_rows_cols_stats", x, y, row_alpha, yc, col_exp, col_alpha, db, pmax, psum, P, rows,
                                     cols, ldx, 3, stream);
}

// The two-piece form: y fp16 [rows][2 cols] = [hi|lo] (non-temporal stores, as above), bit-equal to the first two
// pieces of the entry above; every other output as there.
DCLIP_API int dclip_split_f32_f16x2_rows_cols_stats(const float* x, void* y, float* row_alpha, void* yc, int* col_exp, float* col_alpha,
                                                    float* db, const void* pmax, const float* psum, int P, int rows, int cols, int ldx,
                                                    void* stream) {
  return split_rows_cols_stats_entry("split_f32_f16x3_rows_cols_stats", x, y, row_alpha, yc, col_exp, col_alpha, db, pmax, psum, P, rows,
                                     cols, ldx, 2, stream);
}

// Column sums of x [B*S][cols] in the association of a producer that leaves one partial row per segment of S rows and of the
// finish over them: psum[b][c] = the fp32 sum of rows b S .. b S + S - 1 in order, then colstats_finish_kernel's
// fold over the B partial rows — bit-equal to the db that dclip_split_f32_f16x3_rows_cols_stats folds from the partials of
// dclip_attention_bwd_rows_stats / dclip_attention_bwd_stats on the same x.  For the form of a backward that runs WITHOUT the
// producer's statistics and must still return the same bias gradient.  workspace: (2 B + 2) cols 4-byte words.
// The finish is the shared kernel, launched as the single pass launches it, so that the fold is that one by construction: the
// column maxima this kernel writes and the col_exp / col_alpha the finish derives from them land in the workspace and are read
// by nobody.  That is B cols words of extra stores in a form that is switched off by default, against a second finish kernel.
namespace {
__global__ void __launch_bounds__(256) colstats_segments_kernel(const float* __restrict__ x, unsigned* __restrict__ pmax,
                                                                float* __restrict__ psum, int S, int cols, int ldx) {
  const int c = blockIdx.y * 256 + threadIdx.x, b = blockIdx.x;
  if (c >= cols) return;
  const float* p = x + (size_t)b * S * ldx + c;
  unsigned m = 0u;
  float s = 0.f;
  for (int r = 0; r < S; ++r) {
    const float v = p[(size_t)r * ldx];
    const unsigned u = __builtin_bit_cast(unsigned, v) & 0x7fffffffu;
    m = m > u ? m : u;
    s += v;
  }
  pmax[(size_t)b * cols + c] = m;
  psum[(size_t)b * cols + c] = s;
}
}  // namespace

DCLIP_API size_t dclip_colsum_segments_f32_workspace(int B, int cols) {
  return B > 0 && cols > 0 ? ((size_t)2 * B + 2) * cols * sizeof(float) : 0;
}

DCLIP_API int dclip_colsum_segments_f32(const float* x, float* db, int B, int S, int cols, int ldx, void* workspace,
                                        size_t workspace_bytes, void* stream) {
  DCLIP_REQUIRE(x && db && B > 0 && S > 0 && cols > 0 && ldx >= cols, "colsum_segments_f32: bad arguments");
  DCLIP_REQUIRE(((uintptr_t)x | (uintptr_t)db | (uintptr_t)workspace) % 4 == 0, "colsum_segments_f32: alignment");
  const size_t need = dclip_colsum_segments_f32_workspace(B, cols);
  if (!workspace || workspace_bytes < need) {
    dclip_set_error("colsum_segments_f32: needs %zu workspace bytes, got %zu", need, workspace_bytes);
    return DCLIP_EWORKSPACE;
  }
  unsigned* pmax = (unsigned*)workspace;
  float* psum = (float*)workspace + (size_t)B * cols;
  int* col_exp = (int*)workspace + (size_t)2 * B * cols;
  float* col_alpha = (float*)workspace + (size_t)2 * B * cols + cols;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(colstats_segments_kernel, dim3(B, cdiv(cols, 256)), dim3(256), 0, st, x, pmax, psum, S, cols, ldx);
  DCLIP_CHECK_LAUNCH("colsum_segments_f32");
  hipLaunchKernelGGL(colstats_finish_kernel, dim3(cdiv(cols, FIN_COLS)), dim3(256), 0, st, (const unsigned*)pmax, (const float*)psum, col_exp,
                     col_alpha, db, B, cols);
  DCLIP_CHECK_LAUNCH_V("colsum_segments_f32", ".finish");
  return DCLIP_OK;
}

DCLIP_API int dclip_layernorm_fwd_f16x3(const float* x, const float* gamma, const float* beta, void* y, int rows, int D,
                                        float eps, float scale, void* stream) {
  DCLIP_REQUIRE(x && gamma && beta && y, "layernorm_fwd_f16x3: null pointer");
  DCLIP_REQUIRE(rows > 0 && D > 0 && D % 4 == 0 && D <= 2048, "layernorm_fwd_f16x3: bad D=%d", D);
  DCLIP_REQUIRE(((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)beta) % 16 == 0 && (uintptr_t)y % 8 == 0,
                "layernorm_fwd_f16x3: alignment");
  DCLIP_REQUIRE(pow2(scale), "layernorm_fwd_f16x3: scale must be a power of two");
  return ln_launch("layernorm_fwd_f16x3", x, gamma, beta, y, rows, D, eps, scale, nullptr, nullptr, nullptr, nullptr, stream);
}

// dclip_layernorm_fwd_f16x3 with the scale in device memory; y32 / mean / rstd (each may be null) also receive what
// dclip_layernorm_fwd writes — the fp32 output and the row statistics a training forward saves — bit for bit.
DCLIP_API int dclip_layernorm_fwd_f16x3_dev(const float* x, const float* gamma, const float* beta, void* y, float* y32, float* mean,
                                            float* rstd, int rows, int D, float eps, const float* scale, void* stream) {
  DCLIP_REQUIRE(x && gamma && beta && y && scale, "layernorm_fwd_f16x3_dev: null pointer");
  DCLIP_REQUIRE(rows > 0 && D > 0 && D % 4 == 0 && D <= 2048, "layernorm_fwd_f16x3_dev: bad D=%d", D);
  DCLIP_REQUIRE(((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)y32) % 16 == 0 && (uintptr_t)y % 8 == 0 &&
                    (uintptr_t)scale % 4 == 0,
                "layernorm_fwd_f16x3_dev: alignment");
  return ln_launch("layernorm_fwd_f16x3_dev", x, gamma, beta, y, rows, D, eps, 1.f, scale, y32, mean, rstd, stream);
}

// The two-piece form: y fp16 [rows][2 D] = [hi|lo], bit-equal to the first two pieces of the entries above; y32 /
// mean / rstd (each may be null) as dclip_layernorm_fwd_f16x3_dev writes them.  scale_dev (device, may be null) takes the place of
// `scale` when given.
DCLIP_API int dclip_layernorm_fwd_f16x2(const float* x, const float* gamma, const float* beta, void* y, float* y32, float* mean,
                                        float* rstd, int rows, int D, float eps, float scale, const float* scale_dev, void* stream) {
  DCLIP_REQUIRE(x && gamma && beta && y, "layernorm_fwd_f16x2: null pointer");
  DCLIP_REQUIRE(rows > 0 && D > 0 && D % 4 == 0 && D <= 2048, "layernorm_fwd_f16x2: bad D=%d", D);
  DCLIP_REQUIRE(((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)y32) % 16 == 0 && (uintptr_t)y % 8 == 0 &&
                    (uintptr_t)scale_dev % 4 == 0,
                "layernorm_fwd_f16x2: alignment");
  DCLIP_REQUIRE(scale_dev || pow2(scale), "layernorm_fwd_f16x2: scale must be a power of two");
  return ln_launch(scale_dev ? "layernorm_fwd_f16x3_dev" : "layernorm_fwd_f16x3", x, gamma, beta, y, rows, D, eps, scale_dev ? 1.f : scale,
                   scale_dev, y32, mean, rstd, stream, 2);
}

// g[i] = quick_gelu(h[i]) for n fp32 values (n % 4 == 0, 16-byte aligned): bit-equal to the g32 the GELU epilogue of
// dclip_gemm_f16_scaled_split_dev / dclip_gemm_f16x3_scaled_split_dev stores beside the h32 it is given here.
DCLIP_API int dclip_quick_gelu_f32(const float* h, float* g, size_t n, void* stream) {
  DCLIP_REQUIRE(h && g && n > 0 && n % 4 == 0, "quick_gelu_f32: bad arguments (n a positive multiple of 4)");
  DCLIP_REQUIRE(((uintptr_t)h | (uintptr_t)g) % 16 == 0, "quick_gelu_f32: operands must be 16-byte aligned");
  const size_t blocks = cdivz(n / 4, 256);
  hipLaunchKernelGGL(quick_gelu_kernel, dim3((unsigned)(blocks > 8192 ? 8192 : blocks)), dim3(256), 0, (hipStream_t)stream, h, g, n / 4);
  DCLIP_CHECK_LAUNCH("quick_gelu_f32");
  return DCLIP_OK;
}

// ---- device plan (see Split16Ref): record size, and the three launches over a table of `nrefs` records / `tiles` tiles
DCLIP_API int dclip_split16_record_bytes(void) { return (int)sizeof(Split16Ref); }
DCLIP_API int dclip_split16_plan_floats(void) { return PLAN_FLOATS; }
DCLIP_API int dclip_split16_tile_rows(void) { return SPLIT16_TILE_ROWS; }

// stats: uint32 [nlayers][12] accumulators, zero before the first call (the plan launch clears them again)
DCLIP_API int dclip_split16_stats(const void* refs, int nrefs, int tiles, void* stats, void* stream) {
  DCLIP_REQUIRE(refs && stats && nrefs > 0 && tiles > 0, "split16_stats: bad arguments");
  hipLaunchKernelGGL(split16_stats_kernel, dim3(tiles), dim3(256), 0, (hipStream_t)stream, (const Split16Ref*)refs, nrefs,
                     (unsigned*)stats);
  DCLIP_CHECK_LAUNCH("split16_stats");
  return DCLIP_OK;
}

// plan: float [nlayers][32] records from the statistics; D = the tower's width (LayerNorm's bound is max|gamma| sqrt(D) + max|beta|)
DCLIP_API int dclip_split16_plan(void* stats, float* plan, int nlayers, int D, void* stream) {
  DCLIP_REQUIRE(stats && plan && nlayers > 0 && D > 0, "split16_plan: bad arguments");
  hipLaunchKernelGGL(split16_plan_kernel, dim3(cdiv(nlayers, 64)), dim3(64), 0, (hipStream_t)stream, (unsigned*)stats, plan, nlayers,
                     __builtin_sqrt((double)D));
  DCLIP_CHECK_LAUNCH("split16_plan");
  return DCLIP_OK;
}

// weights: the [hi|hi|lo] copies of every record with a destination, scaled by the plan
DCLIP_API int dclip_split16_weights(const void* refs, int nrefs, int tiles, const float* plan, void* stream) {
  DCLIP_REQUIRE(refs && plan && nrefs > 0 && tiles > 0, "split16_weights: bad arguments");
  hipLaunchKernelGGL(split16_weights_kernel, dim3(tiles), dim3(256), 0, (hipStream_t)stream, (const Split16Ref*)refs, nrefs, plan);
  DCLIP_CHECK_LAUNCH("split16_weights");
  return DCLIP_OK;
}

// ---- the front plan: the student's patch embedding on split operands.  Pixels have no bound derivable from a
// weight, so the activation scale comes from the data: max|pixels| every call, max|patch_w| when the weight changed, both as
// maxima of the bit patterns of |x| (NaN above inf) — block partials, then one workgroup that folds them and applies the rules
// of split16_plan_kernel (act_exp / weight_exp in double, the same clamps and flag bits).  No atomics; a maximum does not depend
// on the order of its operands, so every run gives the same bits.
//   wrec  float [4], kept by the caller between calls: 2^f | f (an int) | max|patch_w| | the weight's flag bits
//   rec   float [8], one per forward: 2^e | 2^f | alpha = 2^-(e+f) | flags | max|pixels| | max|patch_w| | e | f (ints)
namespace {
constexpr int FRONT_REC_FLOATS = 8, FRONT_WREC_FLOATS = 4, FRONT_PIX_BLOCKS = 1024, FRONT_W_BLOCKS = 64;

// blocks [0, FRONT_PIX_BLOCKS) fold the pixels, the others (if any) the weight; one partial per block
__global__ void __launch_bounds__(256) front_absmax_kernel(const float* __restrict__ pix, size_t npix, const float* __restrict__ w,
                                                           size_t nw, unsigned* __restrict__ partial) {
  __shared__ unsigned sm[4];
  const bool is_w = blockIdx.x >= FRONT_PIX_BLOCKS;
  const float* x = is_w ? w : pix;
  const size_t n = is_w ? nw : npix, n4 = n / 4;
  const size_t blk = is_w ? blockIdx.x - FRONT_PIX_BLOCKS : blockIdx.x, nblk = is_w ? FRONT_W_BLOCKS : FRONT_PIX_BLOCKS;
  unsigned m = 0u;
  for (size_t i = blk * 256 + threadIdx.x; i < n4; i += nblk * 256) {
    const f32x4 v = reinterpret_cast<const f32x4*>(x)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float f = v[e];
      const unsigned u = __builtin_bit_cast(unsigned, f) & 0x7fffffffu;
      m = m > u ? m : u;
    }
  }
  if (blk == 0 && n4 * 4 + threadIdx.x < n) {          // up to three values past the last whole group of four
    const unsigned u = __builtin_bit_cast(unsigned, x[n4 * 4 + threadIdx.x]) & 0x7fffffffu;
    m = m > u ? m : u;
  }
  m = wave_umax(m);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < 4; ++k) m = m > sm[k] ? m : sm[k];
    partial[blockIdx.x] = m;
  }
}

__device__ __forceinline__ unsigned block_umax(unsigned m, unsigned* sm) {      // the result in thread 0
  m = wave_umax(m);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int k = 1; k < 4; ++k) m = m > sm[k] ? m : sm[k];
  return m;
}

__global__ void __launch_bounds__(256) front_plan_kernel(const unsigned* __restrict__ partial, int have_w, float* __restrict__ wrec,
                                                         float* __restrict__ rec) {
  __shared__ unsigned sm[4];
  unsigned mp = 0u, mw = 0u;
  for (int i = threadIdx.x; i < FRONT_PIX_BLOCKS; i += 256) mp = mp > partial[i] ? mp : partial[i];
  mp = block_umax(mp, sm);
  if (have_w) {
    if (threadIdx.x < FRONT_W_BLOCKS) mw = partial[FRONT_PIX_BLOCKS + threadIdx.x];
    mw = block_umax(mw, sm);
  }
  if (threadIdx.x != 0) return;
  int f;
  unsigned wflags;
  float wmax;
  if (have_w) {
    wflags = 0u;
    wmax = __builtin_bit_cast(float, mw);
    f = weight_exp((double)wmax, wflags);
    if (f > 127) f = 127, wflags |= 4u;
    wrec[0] = pow2f(f);
    wrec[1] = __builtin_bit_cast(float, f);
    wrec[2] = wmax;
    wrec[3] = __builtin_bit_cast(float, wflags);
  } else {
    f = __builtin_bit_cast(int, wrec[1]);
    wmax = wrec[2];
    wflags = __builtin_bit_cast(unsigned, wrec[3]);
  }
  unsigned flags = wflags;
  const float pmax = __builtin_bit_cast(float, mp);
  int e = act_exp((double)pmax, flags);
  if (e < -126) e = -126, flags |= 4u;
  if (-(e + f) > 127 || -(e + f) < -126) flags |= 4u;
  rec[0] = pow2f(e);
  rec[1] = pow2f(f);
  rec[2] = pow2f(-(e + f));
  rec[3] = __builtin_bit_cast(float, flags);
  rec[4] = pmax;
  rec[5] = wmax;
  rec[6] = __builtin_bit_cast(float, e);
  rec[7] = __builtin_bit_cast(float, f);
}
}  // namespace

DCLIP_API int dclip_split16_front_rec_floats(void) { return FRONT_REC_FLOATS; }
DCLIP_API int dclip_split16_front_wrec_floats(void) { return FRONT_WREC_FLOATS; }
DCLIP_API size_t dclip_split16_front_workspace(void) { return (size_t)(FRONT_PIX_BLOCKS + FRONT_W_BLOCKS) * sizeof(unsigned); }

// Two launches (the maxima, the plan), three with `refresh_w`: the weight's maximum is then taken too and w3 fp16 [wrows][3 wcols]
// receives [hi|hi|lo] of w 2^f — split_f16x3_kernel<1> with the scale read from wrec, bit-equal to dclip_split_f32_f16x3(order 1)
// at that scale.  Without `refresh_w` wrec is read as the last such call left it, and w / w3 are not touched.
DCLIP_API int dclip_split16_front(const float* pixels, size_t npix, const float* w, int wrows, int wcols, void* w3, float* wrec,
                                  float* rec, void* workspace, size_t workspace_bytes, int refresh_w, void* stream) {
  dclip_note_first_launch("", "");
  DCLIP_REQUIRE(pixels && npix > 0 && wrec && rec, "split16_front: bad arguments");
  DCLIP_REQUIRE(!refresh_w || (w && w3 && wrows > 0 && wcols > 0 && wcols % 8 == 0), "split16_front: weight [rows][cols % 8 == 0]");
  DCLIP_REQUIRE(((uintptr_t)pixels | (uintptr_t)workspace) % 16 == 0 && ((uintptr_t)wrec | (uintptr_t)rec) % 4 == 0 &&
                    (!refresh_w || ((uintptr_t)w | (uintptr_t)w3) % 16 == 0),
                "split16_front: alignment");
  if (!workspace || workspace_bytes < dclip_split16_front_workspace()) {
    dclip_set_error("split16_front: needs %zu workspace bytes, got %zu", dclip_split16_front_workspace(), workspace_bytes);
    return DCLIP_EWORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  const size_t nw = refresh_w ? (size_t)wrows * wcols : 0;
  hipLaunchKernelGGL(front_absmax_kernel, dim3(FRONT_PIX_BLOCKS + (refresh_w ? FRONT_W_BLOCKS : 0)), dim3(256), 0, st, pixels, npix,
                     refresh_w ? w : nullptr, nw, (unsigned*)workspace);
  DCLIP_CHECK_LAUNCH_V("split16_front", ".max");
  dclip_note_first_launch("split16_front", ".max");
  hipLaunchKernelGGL(front_plan_kernel, dim3(1), dim3(256), 0, st, (const unsigned*)workspace, refresh_w ? 1 : 0, wrec, rec);
  DCLIP_CHECK_LAUNCH_V("split16_front", ".plan");
  if (!refresh_w) return DCLIP_OK;
  return split_launch("split16_front", w, w3, wrows, wcols, wcols, 3 * wcols, 1.f, wrec, 1, stream);
}

// ---- the column-only split of a dY whose weight gradient has no data gradient beside it (the patch embedding's, DESIGN.md
// §35): col_exp, col_alpha and yc of dclip_split_f32_f16x2_rows_colstats on the same x, bit for bit — a column maximum does not
// depend on how the rows were grouped — without the row pieces, row_alpha and db.  Three launches: the column maxima of row
// strips (one partial row per workgroup, no atomics), their fold, then split_cols_f16x2_kernel as it is.
namespace {
constexpr int COLMAX_MAX_BLOCKS = 1024, COLMAX_ROWS_PER_BLOCK = 8;
inline int colmax_blocks(int rows) {
  const int b = cdiv(rows, COLMAX_ROWS_PER_BLOCK);
  return b < COLMAX_MAX_BLOCKS ? b : COLMAX_MAX_BLOCKS;
}

// workgroup b folds rows b, b + gridDim.x, ...; a thread owns 4 columns at a time (a wave reads 1 KiB of a row per instruction)
__global__ void __launch_bounds__(256) colmax_partial_kernel(const float* __restrict__ x, unsigned* __restrict__ pmax, int rows,
                                                             int cols, int ldx) {
  const int c4n = cols >> 2;
  for (int c4 = threadIdx.x; c4 < c4n; c4 += 256) {
    unsigned m[4] = {0u, 0u, 0u, 0u};
    for (int r = blockIdx.x; r < rows; r += gridDim.x) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(x + (size_t)r * ldx + c4 * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float f = v[e];
        const unsigned u = __builtin_bit_cast(unsigned, f) & 0x7fffffffu;
        m[e] = m[e] > u ? m[e] : u;
      }
    }
    *reinterpret_cast<u32x4s*>(pmax + (size_t)blockIdx.x * cols + c4 * 4) = u32x4s{m[0], m[1], m[2], m[3]};
  }
}

// colstats_finish_kernel's fold of the maxima alone: 8 columns x 32 groups of partial rows per workgroup
__global__ void __launch_bounds__(256) colmax_finish_kernel(const unsigned* __restrict__ pmax, int* __restrict__ col_exp,
                                                            float* __restrict__ col_alpha, int nb, int cols) {
  __shared__ unsigned smax[FIN_GROUPS][FIN_COLS];
  const int cl = threadIdx.x % FIN_COLS, g = threadIdx.x / FIN_COLS;
  const int col = blockIdx.x * FIN_COLS + cl;
  unsigned m = 0u;
  if (col < cols) {
#pragma unroll 4
    for (int b = g; b < nb; b += FIN_GROUPS) {
      const unsigned pm = pmax[(size_t)b * cols + col];
      m = m > pm ? m : pm;
    }
  }
  smax[g][cl] = m;
  __syncthreads();
  if (g == 0 && col < cols) {
    for (int k = 1; k < FIN_GROUPS; ++k) m = m > smax[k][cl] ? m : smax[k][cl];
    const int e = row_exp(m);
    col_exp[col] = e;
    col_alpha[col] = pow2f(-e);
  }
}
}  // namespace

DCLIP_API size_t dclip_split_f32_f16x2_cols_workspace(int rows, int cols) {
  if (rows <= 0 || cols <= 0) return 0;
  return (size_t)colmax_blocks(rows) * cols * sizeof(unsigned);
}

DCLIP_API int dclip_split_f32_f16x2_cols(const float* x, void* yc, int* col_exp, float* col_alpha, int rows, int cols, int ldx,
                                         void* workspace, size_t workspace_bytes, void* stream) {
  const char* name = "split_f32_f16x2_cols";
  dclip_note_first_launch("", "");
  DCLIP_REQUIRE(x && yc && col_exp && col_alpha && rows > 0 && cols > 0, "%s: bad arguments", name);
  DCLIP_REQUIRE(cols % 8 == 0, "%s: cols=%d must be a multiple of 8", name, cols);
  DCLIP_REQUIRE(ldx >= cols && ldx % 4 == 0, "%s: ldx must be a multiple of 4 and >= cols", name);
  DCLIP_REQUIRE(((uintptr_t)x | (uintptr_t)yc | (uintptr_t)col_exp | (uintptr_t)workspace) % 16 == 0 && (uintptr_t)col_alpha % 4 == 0,
                "%s: alignment", name);
  const size_t need = dclip_split_f32_f16x2_cols_workspace(rows, cols);
  if (!workspace || workspace_bytes < need) {
    dclip_set_error("%s: needs %zu workspace bytes, got %zu", name, need, workspace_bytes);
    return DCLIP_EWORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  const int nb = colmax_blocks(rows);
  hipLaunchKernelGGL(colmax_partial_kernel, dim3(nb), dim3(256), 0, st, x, (unsigned*)workspace, rows, cols, ldx);
  DCLIP_CHECK_LAUNCH_V(name, ".max");
  dclip_note_first_launch(name, ".max");
  hipLaunchKernelGGL(colmax_finish_kernel, dim3(cdiv(cols, FIN_COLS)), dim3(256), 0, st, (const unsigned*)workspace, col_exp, col_alpha,
                     nb, cols);
  DCLIP_CHECK_LAUNCH_V(name, ".finish");
  const size_t blocks = ((size_t)rows * (cols / 8) + 255) / 256;
  hipLaunchKernelGGL(split_cols_f16x2_kernel, dim3((unsigned)(blocks > 8192 ? 8192 : blocks)), dim3(256), 0, st, x, (const int*)col_exp,
                     (unsigned short*)yc, rows, cols, ldx);
  DCLIP_CHECK_LAUNCH_V(name, ".cols");
  return DCLIP_OK;
}

// dclip_split16_weights that also writes, in the same launch and from the same plan scale, the TRANSPOSED copies: dst_t is a
// device array of nrefs pointers, entry i = fp16 [cols][3 rows] for record i ([hi|hi|lo] of (src scale)^T, bit-equal to
// dclip_split_f32_f16x3 of the transposed weight) or null; records with one need rows % 8 == 0 (the caller's check).
DCLIP_API int dclip_split16_weights_t(const void* refs, int nrefs, int tiles, const float* plan, const void* dst_t, void* stream) {
  DCLIP_REQUIRE(refs && plan && dst_t && nrefs > 0 && tiles > 0, "split16_weights_t: bad arguments");
  hipLaunchKernelGGL(split16_weights_t_kernel, dim3(tiles), dim3(256), 0, (hipStream_t)stream, (const Split16Ref*)refs, nrefs, plan,
                     (unsigned short* const*)dst_t);
  DCLIP_CHECK_LAUNCH_V("split16_weights", ".t");
  return DCLIP_OK;
}
