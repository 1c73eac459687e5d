// Shared host/device helpers for libdclip_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>

#include "../../include/dclip_hip.h"

#define DCLIP_API extern "C" __attribute__((visibility("default")))

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

void dclip_set_error(const char* fmt, ...);
void dclip_note_launch(const char* name);   // what dclip_last_launch() returns; `name` is a string literal
// a kernel-variant suffix (string literal, ".r64", ".head3", ...) appended to the name the last dclip_note_launch recorded
void dclip_note_variant(const char* variant);
// an entry of several launches whose FIRST launch has instances of its own records that one here (two string literals):
// dclip_first_launch() returns it after the later launches have overwritten dclip_last_launch()
void dclip_note_first_launch(const char* name, const char* variant);

#define DCLIP_REQUIRE(cond, ...)                         \
  do {                                                   \
    if (!(cond)) {                                       \
      dclip_set_error(__VA_ARGS__);                      \
      return DCLIP_EINVAL;                               \
    }                                                    \
  } while (0)

// Launch check that does not synchronise: hipGetLastError only reports launch-time failures.  It also records the launch
// site's name for dclip_last_launch(): a test that forces a kernel path asserts there that the path was taken.
#define DCLIP_CHECK_LAUNCH(name)                                                      \
  do {                                                                                \
    dclip_note_launch(name);                                                          \
    hipError_t e__ = hipGetLastError();                                               \
    if (e__ != hipSuccess) {                                                          \
      dclip_set_error("%s: launch failed: %s", name, hipGetErrorString(e__));         \
      return DCLIP_ELAUNCH;                                                           \
    }                                                                                 \
  } while (0)

// The 16-bit dispatchers share one body per entry family (`name` is the entry's name): they add the variant they launched.
#define DCLIP_CHECK_LAUNCH_V(name, variant) \
  do {                                      \
    DCLIP_CHECK_LAUNCH(name);               \
    dclip_note_variant(variant);            \
  } while (0)

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }
static inline size_t cdivz(size_t a, size_t b) { return (a + b - 1) / b; }

// ---- wave64 reductions (DPP/permute based shuffles; the wave is 64 lanes on gfx950) ----
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
// reduce over the 32 lanes that share (lane >> 5)
__device__ __forceinline__ float half_sum(float v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float half_max(float v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
// reduce over the 16 lanes that share (lane >> 4)
__device__ __forceinline__ float quarter_sum(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float quarter_max(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// x * sigmoid(1.702 x) (hf:activations.py:122-123).  The sigmoid's reciprocal is v_rcp_f32 (1 ulp): the IEEE division
// sequence is ~10 instructions per element, and an epilogue wave beside MFMA-issuing waves gets one instruction through
// every ~45 cycles (tools/gemm_stamps.py) — instruction count is what the epilogue costs.
__device__ __forceinline__ float quick_gelu_f(float x) { return x * __builtin_amdgcn_rcpf(1.0f + __expf(-1.702f * x)); }
__device__ __forceinline__ float quick_gelu_grad_f(float x) {
  float s = __builtin_amdgcn_rcpf(1.0f + __expf(-1.702f * x));
  return s * (1.0f + 1.702f * x * (1.0f - s));
}

// ---- the split-fp16 pieces of one value (split16.hip, and the attention forwards that write their context split)
// hi = fp16(v), lo = fp16(v - hi).  v - float(hi) is exact in fp32 (hi is v to 11 bits), so each piece has ONE rounding
// whether or not the compiler folds the subtraction into the conversion.
// v (the caller's x * scale) is pinned in a register first.  Left to itself the compiler converts the product twice: the hi it
// stores from the product, the hi it subtracts as fp16(fma(x, scale, +0)) — which is +0 for a product of -0 — and lo came out
// as -0 - (+0) = -0 where IEEE (and every other instance of this function) gives -0 - (-0) = +0.
static __device__ __forceinline__ void split1(float v, unsigned short& hi, unsigned short& lo) {
  asm volatile("" : "+v"(v));
  const _Float16 h = (_Float16)v;
  const _Float16 l = (_Float16)(v - (float)h);
  hi = __builtin_bit_cast(unsigned short, h);
  lo = __builtin_bit_cast(unsigned short, l);
}

// ---- 16-bit element types of the frozen-tower forward.  The 16-bit kernels are templates over one of these traits; loads,
// LDS layouts, the transposing LDS read and the MFMA C/D layouts do not depend on the type, only the MFMA instruction and
// the fp32 -> 16-bit rounding do.
//   Bf16T: round to nearest even (v_cvt_pk_bf16_f32); bf16 has fp32's range, NaN stays NaN.
//   F16T:  round to nearest even; a FINITE value beyond +-65504 saturates to +-65504 (a frozen forward degrades instead of
//          turning an embedding into NaN), +-inf stays +-inf and NaN stays NaN (no fminf / fmaxf clamp: those return the
//          other operand for a NaN, and the meta-teacher's NaN guards must see what the bf16 path would give them).
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));

struct Bf16T {
  typedef __bf16 elem;
  typedef bf16x8_t x8;
  // rounding of a value that is a probability (attention's P, in [0, 1] or NaN): no range handling needed
  static __device__ __forceinline__ elem cvt_unit(float x) { return (__bf16)x; }
  static __device__ __forceinline__ unsigned short bits(float x) { return __builtin_bit_cast(unsigned short, (__bf16)x); }
  static __device__ __forceinline__ unsigned short bits_prod(float a, float b) { return bits(a * b); }   // see F16IeeeT
  static __device__ __forceinline__ float to_f32(unsigned int h) { return __builtin_bit_cast(float, h << 16); }
  // the element in the low / high half of a dword
  static __device__ __forceinline__ float lo_f32(unsigned int w) { return __builtin_bit_cast(float, w << 16); }
  static __device__ __forceinline__ float hi_f32(unsigned int w) { return __builtin_bit_cast(float, w & 0xffff0000u); }
  static __device__ __forceinline__ f32x16 mfma32(x8 a, x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ f32x4 mfma16(x8 a, x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
};

struct F16T {
  typedef _Float16 elem;
  typedef f16x8_t x8;
  static __device__ __forceinline__ elem cvt_unit(float x) { return (_Float16)x; }
  static __device__ __forceinline__ unsigned short bits(float x) {
    const float a = __builtin_fabsf(x);
    const float s = (a > 65504.f && a != __builtin_inff()) ? __builtin_copysignf(65504.f, x) : x;   // false for NaN
    return __builtin_bit_cast(unsigned short, (_Float16)s);
  }
  static __device__ __forceinline__ unsigned short bits_prod(float a, float b) { return bits(a * b); }   // see F16IeeeT
  static __device__ __forceinline__ float to_f32(unsigned int h) {
    return (float)__builtin_bit_cast(_Float16, (unsigned short)h);
  }
  static __device__ __forceinline__ float lo_f32(unsigned int w) { return to_f32(w & 0xffffu); }
  static __device__ __forceinline__ float hi_f32(unsigned int w) { return to_f32(w >> 16); }
  static __device__ __forceinline__ f32x16 mfma32(x8 a, x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ f32x4 mfma16(x8 a, x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  }
};

// fp16 of the TRAINING path (student_precision="fp16"): F16T with plain IEEE round-to-nearest-even, as
// (_Float16)x does — a finite value beyond +-65504 becomes +-inf and NaN stays NaN.  An overflow of a loss-scaled gradient
// then reaches the global gradient norm, and the loss scaler skips the step and lowers its scale (torch GradScaler).
struct F16IeeeT : F16T {
  static __device__ __forceinline__ unsigned short bits(float x) { return __builtin_bit_cast(unsigned short, (_Float16)x); }
  // fp16(a b) with the product rounded to fp32 first, as bits(a * b) of the other two types is.  Without the barrier the
  // compiler fuses the multiply into this type's bare conversion (v_fma_mixlo_f16: ONE rounding), and the attention forward
  // of the training path differed from the frozen-tower one on the same fp16 input by one ulp in ~1 of 6000 elements
  // (DESIGN.md §17).
  static __device__ __forceinline__ unsigned short bits_prod(float a, float b) {
    float p = a * b;
    asm volatile("" : "+v"(p));
    return bits(p);
  }
};
