// The vision tower at another input size: the bicubic resample of the position table with its exact
// transpose, and the patch gather on a gh x gw grid.  All HBM/L2-bound gathers like embed.hip's; the existing im2col
// kernels there are left as they are, these are their twins with the grid extent g split into gh and gw.  Below them the
// packed front end of DESIGN.md §22: patch rows of many crops of different sizes cut from a uint8 batch, and the assemble step
// that resamples the position table per crop.
#include "common.h"

namespace {

inline int grid_for(size_t work) {
  size_t b = (work + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

// ---- bicubic taps (torch.nn.functional.interpolate, mode="bicubic", align_corners=False; A = -0.75) ----
// For output index o of an axis resampled from g to go cells: source coordinate x = (o + 0.5) g / go - 0.5, f = floor(x),
// t = x - f; taps f-1 .. f+2, each clamped to [0, g-1], with the cubic-convolution weights w(t+1), w(t), w(1-t), w(2-t).
// Coordinate and weights are evaluated in double from the integers and each weight is rounded to fp32 ONCE: the contract
// is the fp64 definition (torch's fp32 kernel forms x in fp32 and is less exact at non-integer ratios).  At t = 0 the
// weights are exactly 0, 1, 0, 0, so an unchanged grid returns the table bit for bit.
struct Taps {
  int idx[4];
  float w[4];
};

__device__ __forceinline__ double cubic_w1(double x) { return ((-0.75 + 2.0) * x - (-0.75 + 3.0)) * x * x + 1.0; }   // |x| <= 1
__device__ __forceinline__ double cubic_w2(double x) {                                                             // 1 < |x| < 2
  return ((-0.75 * x - 5.0 * -0.75) * x + 8.0 * -0.75) * x - 4.0 * -0.75;
}

__device__ __forceinline__ Taps axis_taps(int o, int g, int go) {
  const double x = ((double)o + 0.5) * ((double)g / (double)go) - 0.5;
  const double fl = floor(x);
  const double t = x - fl;
  const int f = (int)fl;
  Taps r;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int i = f - 1 + a;
    r.idx[a] = i < 0 ? 0 : (i > g - 1 ? g - 1 : i);
  }
  r.w[0] = (float)cubic_w2(t + 1.0);
  r.w[1] = (float)cubic_w1(t);
  r.w[2] = (float)cubic_w1(1.0 - t);
  r.w[3] = (float)cubic_w2(2.0 - t);
  return r;
}

// out[0] = pos[0]; out[1 + oy*gw + ox] = sum_a sum_b wy[a] wx[b] pos[1 + iy(a)*g + ix(b)]: one thread per (row, 4 columns),
// the 16 terms in one fmaf chain per component (a outer, b inner), so the result is a pure function of the inputs.
__global__ void __launch_bounds__(256) pos_interp_fwd_kernel(const float* __restrict__ pos, float* __restrict__ out, int g, int gh,
                                                             int gw, int D4, size_t total4) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (size_t)gridDim.x * blockDim.x) {
    const int d = (int)(i % D4);
    const int row = (int)(i / D4);
    if (row == 0) {
      reinterpret_cast<f32x4*>(out)[i] = reinterpret_cast<const f32x4*>(pos)[d];
      continue;
    }
    const int oy = (row - 1) / gw, ox = (row - 1) % gw;
    const Taps ty = axis_taps(oy, g, gh), tx = axis_taps(ox, g, gw);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int a = 0; a < 4; ++a) {
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const float w = ty.w[a] * tx.w[b];
        const f32x4 v = reinterpret_cast<const f32x4*>(pos)[(size_t)(1 + ty.idx[a] * g + tx.idx[b]) * D4 + d];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = fmaf(w, v[e], acc[e]);
      }
    }
    reinterpret_cast<f32x4*>(out)[i] = acc;
  }
}

// The exact transpose in gather form: a thread owns (source cell, 4 columns) and walks ALL gh x gw destination rows in
// ascending order, recomputing the taps of each (gh + gh*gw axis evaluations in double per thread; the grids are at most a
// few dozen cells a side) and adding the terms whose clamped tap index is its own cell — the same fp32 weights
// wy[a] * wx[b] as the forward.  A destination whose tap range [idx[0], idx[3]] misses the cell is skipped after its taps
// are formed.  No atomics.
__global__ void __launch_bounds__(256) pos_interp_bwd_kernel(const float* __restrict__ dout, float* __restrict__ dpos, int g,
                                                             int gh, int gw, int D4, int accumulate, size_t total4) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (size_t)gridDim.x * blockDim.x) {
    const int d = (int)(i % D4);
    const int row = (int)(i / D4);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (row == 0) {
      acc = reinterpret_cast<const f32x4*>(dout)[d];
    } else {
      const int sy = (row - 1) / g, sx = (row - 1) % g;
      for (int oy = 0; oy < gh; ++oy) {
        const Taps ty = axis_taps(oy, g, gh);
        if (ty.idx[0] > sy || ty.idx[3] < sy) continue;      // the clamped taps are non-decreasing in a
        for (int ox = 0; ox < gw; ++ox) {
          const Taps tx = axis_taps(ox, g, gw);
          if (tx.idx[0] > sx || tx.idx[3] < sx) continue;
          const f32x4 v = reinterpret_cast<const f32x4*>(dout)[(size_t)(1 + oy * gw + ox) * D4 + d];
#pragma unroll
          for (int a = 0; a < 4; ++a) {
#pragma unroll
            for (int b = 0; b < 4; ++b) {
              if (ty.idx[a] == sy && tx.idx[b] == sx) {
                const float w = ty.w[a] * tx.w[b];
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] = fmaf(w, v[e], acc[e]);
              }
            }
          }
        }
      }
    }
    if (accumulate) acc += reinterpret_cast<const f32x4*>(dpos)[i];
    reinterpret_cast<f32x4*>(dpos)[i] = acc;
  }
}

// ---- patch gather on a gh x gw grid ----
// cols[(b*gh*gw + gy*gw + gx)][c*p*p + py*p + px] = pixels[b][c][gy*p+py][gx*p+px]; rows >= gh*p and columns >= gw*p of the
// image are never read (a stride-p convolution ignores them too).
__global__ void __launch_bounds__(256) im2col_rect_kernel(const float* __restrict__ pix, float* __restrict__ cols, int B, int C,
                                                          int Himg, int Wimg, int p, int gh, int gw, size_t total) {
  const int kdim = C * p * p;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int k = (int)(i % kdim);
    const size_t row = i / kdim;
    const int gx = (int)(row % gw), gy = (int)((row / gw) % gh), b = (int)(row / ((size_t)gh * gw));
    const int px = k % p, py = (k / p) % p, c = k / (p * p);
    cols[i] = pix[(((size_t)b * C + c) * Himg + gy * p + py) * Wimg + gx * p + px];
  }
}

// 16 bytes in per thread: needs p % 4 == 0 AND Wimg % 4 == 0 (the load address is (gy*p + py)*Wimg + gx*p + px floats).
typedef unsigned short u16x4_r __attribute__((ext_vector_type(4)));
template <class T16>
__global__ void __launch_bounds__(256) im2col_rect_vec_kernel(const float* __restrict__ pix, void* __restrict__ cols, int B,
                                                              int C, int Himg, int Wimg, int p, int gh, int gw, int ldc,
                                                              size_t total4) {
  const int kdim4 = C * p * p / 4, p4 = p / 4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (size_t)gridDim.x * blockDim.x) {
    const int k4 = (int)(i % kdim4);
    const size_t row = i / kdim4;
    const int gx = (int)(row % gw), gy = (int)((row / gw) % gh), b = (int)(row / ((size_t)gh * gw));
    const int px = (k4 % p4) * 4, py = (k4 / p4) % p, c = k4 / (p4 * p);
    const f32x4 v = *reinterpret_cast<const f32x4*>(pix + (((size_t)b * C + c) * Himg + gy * p + py) * Wimg + gx * p + px);
    if constexpr (!__is_same(T16, float)) {
      u16x4_r o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = T16::bits(v[e]);
      *reinterpret_cast<u16x4_r*>(reinterpret_cast<unsigned short*>(cols) + row * ldc + (size_t)k4 * 4) = o;
    } else {
      *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(cols) + row * ldc + (size_t)k4 * 4) = v;
    }
  }
}

// 16-bit destination from an image whose rows are not 16-byte multiples: scalar loads, one element per thread.
template <class T16>
__global__ void __launch_bounds__(256) im2col_rect_scalar16_kernel(const float* __restrict__ pix, unsigned short* __restrict__ cols,
                                                                   int B, int C, int Himg, int Wimg, int p, int gh, int gw,
                                                                   int ldc, size_t total) {
  const int kdim = C * p * p;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int k = (int)(i % kdim);
    const size_t row = i / kdim;
    const int gx = (int)(row % gw), gy = (int)((row / gw) % gh), b = (int)(row / ((size_t)gh * gw));
    const int px = k % p, py = (k / p) % p, c = k / (p * p);
    cols[row * ldc + k] = T16::bits(pix[(((size_t)b * C + c) * Himg + gy * p + py) * Wimg + gx * p + px]);
  }
}

template <class T>
int im2col_rect16(const char* name, const float* pixels, void* cols, int B, int C, int Himg, int Wimg, int patch, int ldc,
                  void* stream) {
  DCLIP_REQUIRE(pixels && cols, "%s: null pointer", name);
  DCLIP_REQUIRE(B > 0 && C > 0 && patch > 0 && patch % 4 == 0 && Himg >= patch && Wimg >= patch,
                "%s: bad shape %dx%d patch %d (patch must be a multiple of 4, no side shorter than a patch)", name, Himg, Wimg,
                patch);
  DCLIP_REQUIRE(ldc >= C * patch * patch && ldc % 4 == 0 && (uintptr_t)pixels % 16 == 0 && (uintptr_t)cols % 8 == 0,
                "%s: ldc / alignment", name);
  const int gh = Himg / patch, gw = Wimg / patch;
  const size_t total = (size_t)B * gh * gw * C * patch * patch;
  const bool vec = Wimg % 4 == 0;
  if (vec)
    hipLaunchKernelGGL((im2col_rect_vec_kernel<T>), dim3(grid_for(total / 4)), dim3(256), 0, (hipStream_t)stream, pixels, cols, B,
                       C, Himg, Wimg, patch, gh, gw, ldc, total / 4);
  else
    hipLaunchKernelGGL((im2col_rect_scalar16_kernel<T>), dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, pixels,
                       (unsigned short*)cols, B, C, Himg, Wimg, patch, gh, gw, ldc, total);
  DCLIP_CHECK_LAUNCH(name);
  dclip_note_variant(vec ? ".vec" : ".scalar");
  return DCLIP_OK;
}

// ---- the packed (variable-length) front end of the tower ----
// Patch rows of N crops cut from a padded uint8 batch, each crop at its own size: crop n = boxes[n] = (b, x1, y1, x2, y2) has
// the grid gh = (y2-y1)/p, gw = (x2-x1)/p and owns rows po[n] .. po[n+1]-1 of cols; row gy*gw + gx, column c*p*p + py*p + px is
// pixel (y1 + gy*p + py, x1 + gx*p + px) of image b, channel c, as float / 255 (an IEEE division: ToTensor()'s value).  A
// position outside [0,h) x [0,w) of its image reads nothing and gives 0 (PIL's crop of a box past an edge); the batch's own
// padding is never what supplies that zero.  Grid (N, chunks): a workgroup serves ONE crop, so no thread searches the offset
// table.  VEC: four px per thread and a 16-byte store (p % 4 == 0).
__device__ __forceinline__ float pixel_or_zero(const uint8_t* __restrict__ img, int y, int x, int c, int h, int w, int Wmax) {
  return (y >= 0 && y < h && x >= 0 && x < w) ? (float)img[((size_t)y * Wmax + x) * 3 + c] / 255.0f : 0.0f;
}

template <bool VEC>
__global__ void __launch_bounds__(256) patches_from_boxes_kernel(const uint8_t* __restrict__ images, const int32_t* __restrict__ dims,
                                                                 const int32_t* __restrict__ boxes, const int32_t* __restrict__ po,
                                                                 float* __restrict__ cols, int B, int Hmax, int Wmax, int p) {
  const int n = blockIdx.x;
  const int b = boxes[5 * n], x1 = boxes[5 * n + 1], y1 = boxes[5 * n + 2], x2 = boxes[5 * n + 3], y2 = boxes[5 * n + 4];
  if (b < 0 || b >= B || x2 - x1 < p || y2 - y1 < p) return;            // a crop the planner would not have listed
  const int gw = (x2 - x1) / p, gh = (y2 - y1) / p;
  const int row0 = po[n];
  const long long nrows = min((long long)gh * gw, (long long)po[n + 1] - row0);    // never into the next crop's rows
  if (row0 < 0 || nrows <= 0) return;
  const int h = min(dims[2 * b], Hmax), w = min(dims[2 * b + 1], Wmax);
  const uint8_t* img = images + (size_t)b * Hmax * Wmax * 3;
  const int kdim = 3 * p * p, step = VEC ? 4 : 1, kper = kdim / step, pper = p / step;
  const size_t total = (size_t)nrows * kper;
  for (size_t i = (size_t)blockIdx.y * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.y * blockDim.x) {
    const int k = (int)(i % kper);
    const int j = (int)(i / kper);
    const int gx = j % gw, gy = j / gw;
    const int px = (k % pper) * step, py = (k / pper) % p, c = k / (pper * p);
    const int y = y1 + gy * p + py, x = x1 + gx * p + px;
    float* dst = cols + ((size_t)row0 + j) * kdim + (size_t)k * step;
    if constexpr (VEC) {
      f32x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = pixel_or_zero(img, y, x + e, c, h, w, Wmax);
      *reinterpret_cast<f32x4*>(dst) = v;
    } else {
      *dst = pixel_or_zero(img, y, x, c, h, w, Wmax);
    }
  }
}

// x rows of N crops: row cu[n] = cls + pos[0]; row cu[n] + 1 + j = patch[cu[n] - n + j] + R_n[1 + j], R_n the table resampled
// to crop n's grid (gh, gw) = grids[n] by pos_interp_fwd_kernel's arithmetic (axis_taps, one 16-term fmaf chain, a outer, b
// inner) and added by vision_assemble_fwd_kernel's statement: bit for bit what those two launches give crop by crop.
// Grid (N, chunks), one crop per workgroup.
__global__ void __launch_bounds__(256) vision_assemble_varlen_kernel(const float* __restrict__ patch, const float* __restrict__ cls,
                                                                     const float* __restrict__ pos, const int32_t* __restrict__ grids,
                                                                     const int32_t* __restrict__ cu, float* __restrict__ x, int g,
                                                                     int D4) {
  const int n = blockIdx.x;
  const int gh = grids[2 * n], gw = grids[2 * n + 1];
  const int row0 = cu[n];
  if (gh < 1 || gw < 1 || row0 < n) return;
  const long long S = min(1ll + (long long)gh * gw, (long long)cu[n + 1] - row0);  // never into the next crop's rows
  if (S <= 0) return;
  const size_t prow0 = (size_t)(row0 - n);                                         // patch_offsets[n]
  const size_t total4 = (size_t)S * D4;
  for (size_t i = (size_t)blockIdx.y * blockDim.x + threadIdx.x; i < total4; i += (size_t)gridDim.y * blockDim.x) {
    const int d = (int)(i % D4);
    const int s = (int)(i / D4);
    f32x4 v, r;
    if (s == 0) {
      v = reinterpret_cast<const f32x4*>(cls)[d];
      r = reinterpret_cast<const f32x4*>(pos)[d];
    } else {
      v = reinterpret_cast<const f32x4*>(patch)[(prow0 + (s - 1)) * D4 + d];
      const int oy = (s - 1) / gw, ox = (s - 1) % gw;
      const Taps ty = axis_taps(oy, g, gh), tx = axis_taps(ox, g, gw);
      r = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int a = 0; a < 4; ++a) {
#pragma unroll
        for (int bb = 0; bb < 4; ++bb) {
          const float wgt = ty.w[a] * tx.w[bb];
          const f32x4 t = reinterpret_cast<const f32x4*>(pos)[(size_t)(1 + ty.idx[a] * g + tx.idx[bb]) * D4 + d];
#pragma unroll
          for (int e = 0; e < 4; ++e) r[e] = fmaf(wgt, t[e], r[e]);
        }
      }
    }
    reinterpret_cast<f32x4*>(x)[((size_t)row0 + s) * D4 + d] = v + r;
  }
}

}  // namespace

DCLIP_API int dclip_pos_interp_fwd(const float* pos, float* out, int g, int gh, int gw, int D, void* stream) {
  DCLIP_REQUIRE(pos && out, "pos_interp_fwd: null pointer");
  DCLIP_REQUIRE(g >= 1 && gh >= 1 && gw >= 1 && D > 0 && D % 4 == 0 && g <= 32768 && (long long)gh * gw < (1ll << 30),
                "pos_interp_fwd: bad shape g %d -> %dx%d, D %d", g, gh, gw, D);
  DCLIP_REQUIRE(((uintptr_t)pos | (uintptr_t)out) % 16 == 0, "pos_interp_fwd: pointers must be 16-byte aligned");
  const size_t total4 = ((size_t)gh * gw + 1) * (D / 4);
  hipLaunchKernelGGL(pos_interp_fwd_kernel, dim3(grid_for(total4)), dim3(256), 0, (hipStream_t)stream, pos, out, g, gh, gw, D / 4,
                     total4);
  DCLIP_CHECK_LAUNCH("pos_interp_fwd");
  return DCLIP_OK;
}

DCLIP_API int dclip_pos_interp_bwd(const float* dout, float* dpos, int g, int gh, int gw, int D, int accumulate, void* stream) {
  DCLIP_REQUIRE(dout && dpos, "pos_interp_bwd: null pointer");
  DCLIP_REQUIRE(g >= 1 && gh >= 1 && gw >= 1 && D > 0 && D % 4 == 0 && g <= 32768 && (long long)gh * gw < (1ll << 30),
                "pos_interp_bwd: bad shape g %d -> %dx%d, D %d", g, gh, gw, D);
  DCLIP_REQUIRE(((uintptr_t)dout | (uintptr_t)dpos) % 16 == 0, "pos_interp_bwd: pointers must be 16-byte aligned");
  const size_t total4 = ((size_t)g * g + 1) * (D / 4);
  hipLaunchKernelGGL(pos_interp_bwd_kernel, dim3(grid_for(total4)), dim3(256), 0, (hipStream_t)stream, dout, dpos, g, gh, gw,
                     D / 4, accumulate ? 1 : 0, total4);
  DCLIP_CHECK_LAUNCH("pos_interp_bwd");
  return DCLIP_OK;
}

DCLIP_API int dclip_im2col_rect(const float* pixels, float* cols, int B, int C, int Himg, int Wimg, int patch, void* stream) {
  DCLIP_REQUIRE(pixels && cols, "im2col_rect: null pointer");
  DCLIP_REQUIRE(B > 0 && C > 0 && patch > 0 && Himg >= patch && Wimg >= patch,
                "im2col_rect: bad shape %dx%d patch %d (no side shorter than a patch)", Himg, Wimg, patch);
  const int gh = Himg / patch, gw = Wimg / patch;
  const size_t total = (size_t)B * gh * gw * C * patch * patch;
  const bool vec = patch % 4 == 0 && Wimg % 4 == 0 && ((uintptr_t)pixels | (uintptr_t)cols) % 16 == 0;
  if (vec)
    hipLaunchKernelGGL((im2col_rect_vec_kernel<float>), dim3(grid_for(total / 4)), dim3(256), 0, (hipStream_t)stream, pixels,
                       cols, B, C, Himg, Wimg, patch, gh, gw, C * patch * patch, total / 4);
  else
    hipLaunchKernelGGL(im2col_rect_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, pixels, cols, B, C, Himg,
                       Wimg, patch, gh, gw, total);
  DCLIP_CHECK_LAUNCH_V("im2col_rect", vec ? ".vec" : ".scalar");
  return DCLIP_OK;
}

DCLIP_API int dclip_im2col_rect_bf16(const float* pixels, void* cols, int B, int C, int Himg, int Wimg, int patch, int ldc,
                                     void* stream) {
  return im2col_rect16<Bf16T>("im2col_rect_bf16", pixels, cols, B, C, Himg, Wimg, patch, ldc, stream);
}

DCLIP_API int dclip_im2col_rect_f16(const float* pixels, void* cols, int B, int C, int Himg, int Wimg, int patch, int ldc,
                                    void* stream) {
  return im2col_rect16<F16T>("im2col_rect_f16", pixels, cols, B, C, Himg, Wimg, patch, ldc, stream);
}

// The packed front end.  A fixed number of workgroups per crop: the kernels walk a crop's rows with a stride, so any crop
// size is served and the host needs no per-crop figure.
DCLIP_API int dclip_patches_from_boxes_u8(const uint8_t* images_u8, const int32_t* dims, const int32_t* boxes,
                                          const int32_t* patch_offsets, float* cols, int B, int Hmax, int Wmax, int N, int patch,
                                          void* stream) {
  DCLIP_REQUIRE(images_u8 && dims && boxes && patch_offsets && cols, "patches_from_boxes_u8: null pointer");
  DCLIP_REQUIRE(B > 0 && Hmax > 0 && Wmax > 0 && N > 0 && patch >= 1 && patch <= 1024,
                "patches_from_boxes_u8: bad shape B=%d %dx%d N=%d patch=%d", B, Hmax, Wmax, N, patch);
  DCLIP_REQUIRE(((uintptr_t)dims | (uintptr_t)boxes | (uintptr_t)patch_offsets) % 4 == 0 && (uintptr_t)cols % 16 == 0,
                "patches_from_boxes_u8: dims / boxes / patch_offsets must be 4-byte aligned, cols 16-byte aligned");
  const bool vec = patch % 4 == 0;
  const dim3 grid(N, 16);
  if (vec)
    hipLaunchKernelGGL((patches_from_boxes_kernel<true>), grid, dim3(256), 0, (hipStream_t)stream, images_u8, dims, boxes,
                       patch_offsets, cols, B, Hmax, Wmax, patch);
  else
    hipLaunchKernelGGL((patches_from_boxes_kernel<false>), grid, dim3(256), 0, (hipStream_t)stream, images_u8, dims, boxes,
                       patch_offsets, cols, B, Hmax, Wmax, patch);
  DCLIP_CHECK_LAUNCH("patches_from_boxes_u8");
  return DCLIP_OK;
}

DCLIP_API int dclip_vision_assemble_varlen(const float* patch_emb, const float* cls, const float* pos, const int32_t* grids,
                                           const int32_t* cu_seqlens, float* x, int g, int N, int D, void* stream) {
  DCLIP_REQUIRE(patch_emb && cls && pos && grids && cu_seqlens && x, "vision_assemble_varlen: null pointer");
  DCLIP_REQUIRE(g >= 1 && g <= 32768 && N > 0 && D > 0 && D % 4 == 0, "vision_assemble_varlen: bad shape g=%d N=%d D=%d", g, N, D);
  DCLIP_REQUIRE(((uintptr_t)patch_emb | (uintptr_t)cls | (uintptr_t)pos | (uintptr_t)x) % 16 == 0 &&
                    ((uintptr_t)grids | (uintptr_t)cu_seqlens) % 4 == 0,
                "vision_assemble_varlen: float operands must be 16-byte aligned, grids / cu_seqlens 4-byte aligned");
  hipLaunchKernelGGL(vision_assemble_varlen_kernel, dim3(N, 8), dim3(256), 0, (hipStream_t)stream, patch_emb, cls, pos, grids,
                     cu_seqlens, x, g, D / 4);
  DCLIP_CHECK_LAUNCH("vision_assemble_varlen");
  return DCLIP_OK;
}
