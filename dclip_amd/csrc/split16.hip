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

// hi = fp16(v), lo = fp16(v - hi).  v - float(hi) is exact in fp32 (hi is v to 11 bits), so each piece has ONE rounding
// whether or not the compiler folds the subtraction into the conversion.
__device__ __forceinline__ void split1(float v, unsigned short& hi, unsigned short& lo) {
  const _Float16 h = (_Float16)v;
  const _Float16 l = (_Float16)(v - (float)h);
  hi = __builtin_bit_cast(unsigned short, h);
  lo = __builtin_bit_cast(unsigned short, l);
}

// 8 columns per thread: two 16-byte loads, three 16-byte stores
template <int ORDER>
__global__ void __launch_bounds__(256) split_f16x3_kernel(const float* __restrict__ x, unsigned short* __restrict__ y, int rows,
                                                          int cols, int ldx, int ldy, float scale) {
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
    *reinterpret_cast<u16x8*>(yr + cols) = ORDER == 0 ? lo : hi;
    *reinterpret_cast<u16x8*>(yr + 2 * cols) = ORDER == 0 ? hi : lo;
  }
}

// ln_fwd_kernel (layernorm.hip) with the split [hi | lo | hi] of scale * LN(x) as its output, y [rows][3 D] fp16.  Loads,
// statistics and the normalisation are that kernel's, statement for statement; the fp32 result is pinned in a register before
// it is scaled and split, so that it is the value ln_fwd_kernel would have stored (no fusion of the affine step into the
// conversion, which would round once instead of twice).
template <int NC, bool EXACT>
__global__ void __launch_bounds__(256) ln_fwd_f16x3_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, unsigned short* __restrict__ y,
                                                           int rows, int D, float eps, float scale) {
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
  unsigned short* yr = y + (size_t)row * 3 * D;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int i = lane + 64 * c;
    if (EXACT || i < d4) {
      f32x4 o = (v[c] - mu) * rs * g[c] + bt[c];
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
      *reinterpret_cast<u16x4*>(yr + 2 * D + i * 4) = hi;
    }
  }
}

inline bool pow2(float s) { return s > 0.f && s - s == 0.f && (__builtin_bit_cast(unsigned int, s) & 0x007fffffu) == 0; }

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
  const size_t work = (size_t)rows * (cols / 8);
  const size_t blocks = (work + 255) / 256;
  const dim3 grid((unsigned)(blocks < 1 ? 1 : (blocks > 8192 ? 8192 : blocks)));
  hipStream_t st = (hipStream_t)stream;
  if (order == 0) hipLaunchKernelGGL(split_f16x3_kernel<0>, grid, dim3(256), 0, st, x, (unsigned short*)y, rows, cols, ldx, ldy, scale);
  else hipLaunchKernelGGL(split_f16x3_kernel<1>, grid, dim3(256), 0, st, x, (unsigned short*)y, rows, cols, ldx, ldy, scale);
  DCLIP_CHECK_LAUNCH_V("split_f32_f16x3", order == 0 ? ".act" : ".weight");
  return DCLIP_OK;
}

DCLIP_API int dclip_layernorm_fwd_f16x3(const float* x, const float* gamma, const float* beta, void* y, int rows, int D,
                                        float eps, float scale, void* stream) {
  DCLIP_REQUIRE(x && gamma && beta && y, "layernorm_fwd_f16x3: null pointer");
  DCLIP_REQUIRE(rows > 0 && D > 0 && D % 4 == 0 && D <= 2048, "layernorm_fwd_f16x3: bad D=%d", D);
  DCLIP_REQUIRE(((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)beta) % 16 == 0 && (uintptr_t)y % 8 == 0,
                "layernorm_fwd_f16x3: alignment");
  DCLIP_REQUIRE(pow2(scale), "layernorm_fwd_f16x3: scale must be a power of two");
  dim3 grid(cdiv(rows, 4)), block(256);
  hipStream_t st = (hipStream_t)stream;
  const int nc = cdiv(D / 4, 64);
  unsigned short* yy = (unsigned short*)y;
  const char* variant;
#define LN16X3(NC, EX)                                                                                            \
  do {                                                                                                            \
    hipLaunchKernelGGL((ln_fwd_f16x3_kernel<NC, EX>), grid, block, 0, st, x, gamma, beta, yy, rows, D, eps, scale); \
    variant = (EX) ? ".nc" #NC ".exact" : ".nc" #NC;                                                              \
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
  DCLIP_CHECK_LAUNCH_V("layernorm_fwd_f16x3", variant);
  return DCLIP_OK;
}
