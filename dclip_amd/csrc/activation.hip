// Stand-alone exact (erf) GELU for hidden_act="gelu" checkpoints: element-wise passes behind a bias-only fc1
// GEMM, so that no GEMM epilogue — quick-GELU everywhere — changes.
//   g  = h Phi(h),                   Phi(h) = 0.5 (1 + erf(h / sqrt 2))           (hf:activations.py GELUActivation)
//   dh = dg (Phi(h) + h phi(h)),     phi(h) = exp(-h^2 / 2) / sqrt(2 pi)
// All arithmetic is fp32; finite inputs only.  Memory-bound: 16 bytes per lane per access, 256-thread blocks, a grid capped at
// GELU_MAX_BLOCKS with a grid-stride loop, size_t indexing (a teacher's fc1 output has more than 2^32 elements).
#include "common.h"

namespace {

constexpr unsigned GELU_BLOCK = 256;
constexpr unsigned GELU_MAX_BLOCKS = 2048;      // 256 CUs x 8 blocks

// Phi(h).  0.5 + 0.5 erf(x) cancels for x < 0 (at h = -5 it keeps two digits of 2.9e-7): that side is 0.5 erfc(-x), which
// carries its relative accuracy into the tail — the 16-bit outputs are rounded from it.  x = h sqrt(1/2) rounds h's subnormals
// to erf's linear range either way: Phi = 0.5 exactly there and g = 0.5 h is rounded once.
__device__ __forceinline__ float gelu_phi_cdf(float h) {
  const float x = h * 0.70710678118654752440f;
  return h < 0.f ? 0.5f * erfcf(-x) : 0.5f + 0.5f * erff(x);
}
__device__ __forceinline__ float gelu_erf_f(float h) { return h * gelu_phi_cdf(h); }
__device__ __forceinline__ float gelu_erf_grad_f(float h) {
  const float pdf = 0.39894228040143267794f * expf(-0.5f * h * h);
  return gelu_phi_cdf(h) + h * pdf;
}

// n4 groups of four, then the n - 4 n4 tail values by the first lanes of block 0
__global__ void __launch_bounds__(GELU_BLOCK) gelu_erf_f32_kernel(const float* h, float* g, size_t n) {
  const size_t n4 = n / 4, step = (size_t)gridDim.x * blockDim.x, t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (size_t i = t0; i < n4; i += step) {
    f32x4 v = reinterpret_cast<const f32x4*>(h)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = gelu_erf_f(v[e]);
    reinterpret_cast<f32x4*>(g)[i] = v;
  }
  const size_t j = 4 * n4 + t0;
  if (j < n) g[j] = gelu_erf_f(h[j]);
}

__global__ void __launch_bounds__(GELU_BLOCK) gelu_erf_bwd_f32_kernel(const float* h, const float* dg, float* dh, size_t n) {
  const size_t n4 = n / 4, step = (size_t)gridDim.x * blockDim.x, t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (size_t i = t0; i < n4; i += step) {
    const f32x4 v = reinterpret_cast<const f32x4*>(h)[i];
    f32x4 d = reinterpret_cast<const f32x4*>(dg)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) d[e] *= gelu_erf_grad_f(v[e]);
    reinterpret_cast<f32x4*>(dh)[i] = d;
  }
  const size_t j = 4 * n4 + t0;
  if (j < n) dh[j] = dg[j] * gelu_erf_grad_f(h[j]);
}

typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));

// The fp32 activation of one stored 16-bit value, rounded once more to the type.  The fp32 product is pinned in a register first
// (F16IeeeT::bits_prod, common.h): left alone the compiler folds h * Phi into the fp16 conversion as fma(h, Phi, +0), one rounding
// instead of the two of the statement, and -0 * 0.5 + (+0) = +0 where gelu(-0) = -0.
template <typename T>
__device__ __forceinline__ unsigned short gelu_erf_16(unsigned short h) {
  float g = gelu_erf_f(T::to_f32(h));
  asm volatile("" : "+v"(g));
  return T::bits(g);
}

// T: Bf16T, or F16IeeeT (round to nearest even, a finite result beyond 65504 would be inf: |g| <= |h| never gets there)
template <typename T>
__global__ void __launch_bounds__(GELU_BLOCK) gelu_erf_16_kernel(const unsigned short* h, unsigned short* g, size_t n) {
  const size_t n8 = n / 8, step = (size_t)gridDim.x * blockDim.x, t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (size_t i = t0; i < n8; i += step) {
    u16x8 v = reinterpret_cast<const u16x8*>(h)[i];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = gelu_erf_16<T>(v[e]);
    reinterpret_cast<u16x8*>(g)[i] = v;
  }
  const size_t j = 8 * n8 + t0;
  if (j < n) g[j] = gelu_erf_16<T>(h[j]);
}

inline unsigned gelu_grid(size_t groups) {
  const size_t blocks = cdivz(groups > 0 ? groups : 1, GELU_BLOCK);      // n < one group: one block, for the tail
  return (unsigned)(blocks > GELU_MAX_BLOCKS ? GELU_MAX_BLOCKS : blocks);
}

template <typename T>
int launch_gelu_erf_16(const void* h, void* g, size_t n, void* stream, const char* what) {
  DCLIP_REQUIRE(h && g && n > 0, "%s: bad arguments (null pointer or n = 0)", what);
  DCLIP_REQUIRE(((uintptr_t)h | (uintptr_t)g) % 16 == 0, "%s: operands must be 16-byte aligned", what);
  hipLaunchKernelGGL(gelu_erf_16_kernel<T>, dim3(gelu_grid(n / 8)), dim3(GELU_BLOCK), 0, (hipStream_t)stream,
                     (const unsigned short*)h, (unsigned short*)g, n);
  return DCLIP_OK;
}

}  // namespace

DCLIP_API int dclip_gelu_erf_f32(const float* h, float* g, size_t n, void* stream) {
  DCLIP_REQUIRE(h && g && n > 0, "gelu_erf_f32: bad arguments (null pointer or n = 0)");
  DCLIP_REQUIRE(((uintptr_t)h | (uintptr_t)g) % 16 == 0, "gelu_erf_f32: operands must be 16-byte aligned");
  hipLaunchKernelGGL(gelu_erf_f32_kernel, dim3(gelu_grid(n / 4)), dim3(GELU_BLOCK), 0, (hipStream_t)stream, h, g, n);
  DCLIP_CHECK_LAUNCH("gelu_erf_f32");
  return DCLIP_OK;
}

DCLIP_API int dclip_gelu_erf_bf16(const void* h, void* g, size_t n, void* stream) {
  const int rc = launch_gelu_erf_16<Bf16T>(h, g, n, stream, "gelu_erf_bf16");
  if (rc != DCLIP_OK) return rc;
  DCLIP_CHECK_LAUNCH("gelu_erf_bf16");
  return DCLIP_OK;
}

DCLIP_API int dclip_gelu_erf_f16(const void* h, void* g, size_t n, void* stream) {
  const int rc = launch_gelu_erf_16<F16IeeeT>(h, g, n, stream, "gelu_erf_f16");
  if (rc != DCLIP_OK) return rc;
  DCLIP_CHECK_LAUNCH("gelu_erf_f16");
  return DCLIP_OK;
}

DCLIP_API int dclip_gelu_erf_bwd_f32(const float* h, const float* dg, float* dh, size_t n, void* stream) {
  DCLIP_REQUIRE(h && dg && dh && n > 0, "gelu_erf_bwd_f32: bad arguments (null pointer or n = 0)");
  DCLIP_REQUIRE(((uintptr_t)h | (uintptr_t)dg | (uintptr_t)dh) % 16 == 0, "gelu_erf_bwd_f32: operands must be 16-byte aligned");
  hipLaunchKernelGGL(gelu_erf_bwd_f32_kernel, dim3(gelu_grid(n / 4)), dim3(GELU_BLOCK), 0, (hipStream_t)stream, h, dg, dh, n);
  DCLIP_CHECK_LAUNCH("gelu_erf_bwd_f32");
  return DCLIP_OK;
}
