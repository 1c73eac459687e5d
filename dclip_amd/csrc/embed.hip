// Embedding plumbing around the towers (all HBM-bound gathers / scatters).
#include "common.h"

namespace {

inline int grid_for(size_t work) {
  size_t b = (work + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

// cols[(b*g*g + gy*g + gx)][c*p*p + py*p + px] = pixels[b][c][gy*p+py][gx*p+px]
// One thread per destination element; consecutive threads walk px, so both sides move in runs of p floats.
__global__ void __launch_bounds__(256) im2col_kernel(const float* __restrict__ pix, float* __restrict__ cols, int B, int C,
                                                     int Himg, int Wimg, int p, int g, size_t total) {
  const int kdim = C * p * p;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int k = (int)(i % kdim);
    const size_t row = i / kdim;
    const int gx = (int)(row % g), gy = (int)((row / g) % g), b = (int)(row / ((size_t)g * g));
    const int px = k % p, py = (k / p) % p, c = k / (p * p);
    cols[i] = pix[(((size_t)b * C + c) * Himg + gy * p + py) * Wimg + gx * p + px];
  }
}

// Vector form for patch sizes that are multiples of 4 (ViT-B/32, ViT-B/16): a thread moves 4 consecutive px — 16 bytes
// in, 16 bytes (fp32) or 8 bytes (bf16 / fp16, for the frozen towers' 16-bit GEMM) out.  `ldc` = destination row length.
// T16: Bf16T / F16T (common.h) for a 16-bit destination, float for fp32.
typedef unsigned short u16x4_e __attribute__((ext_vector_type(4)));
template <class T16>
__global__ void __launch_bounds__(256) im2col_vec_kernel(const float* __restrict__ pix, void* __restrict__ cols, int B, int C,
                                                         int Himg, int Wimg, int p, int g, int ldc, size_t total4) {
  const int kdim4 = C * p * p / 4, p4 = p / 4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (size_t)gridDim.x * blockDim.x) {
    const int k4 = (int)(i % kdim4);
    const size_t row = i / kdim4;
    const int gx = (int)(row % g), gy = (int)((row / g) % g), b = (int)(row / ((size_t)g * g));
    const int px = (k4 % p4) * 4, py = (k4 / p4) % p, c = k4 / (p4 * p);
    const f32x4 v = *reinterpret_cast<const f32x4*>(pix + (((size_t)b * C + c) * Himg + gy * p + py) * Wimg + gx * p + px);
    if constexpr (!__is_same(T16, float)) {
      u16x4_e o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = T16::bits(v[e]);
      *reinterpret_cast<u16x4_e*>(reinterpret_cast<unsigned short*>(cols) + row * ldc + (size_t)k4 * 4) = o;
    } else {
      *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(cols) + row * ldc + (size_t)k4 * 4) = v;
    }
  }
}

// im2col_vec_kernel's gather with the split-fp16 operand of the student's patch embedding as its output: a thread
// moves 8 consecutive px (patch % 8 == 0) — two 16-byte loads, two 16-byte stores — and writes cols[row] = [hi | lo] of
// pixel * scale, fp16 [rows][2 kdim]: dclip_split_f32_f16x2's arithmetic on what dclip_im2col would have stored, element for
// element.  The fp32 columns never exist.  The scale is the device float scale_p when given.
typedef unsigned short u16x8_e __attribute__((ext_vector_type(8)));
__global__ void __launch_bounds__(256) im2col_f16x2_kernel(const float* __restrict__ pix, unsigned short* __restrict__ cols, int B,
                                                           int C, int Himg, int Wimg, int p, int g, float scale_v,
                                                           const float* __restrict__ scale_p, size_t total8) {
  const float scale = scale_p ? *scale_p : scale_v;
  const int kdim = C * p * p, kdim8 = kdim / 8, p8 = p / 8;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total8; i += (size_t)gridDim.x * blockDim.x) {
    const int k8 = (int)(i % kdim8);
    const size_t row = i / kdim8;
    const int gx = (int)(row % g), gy = (int)((row / g) % g), b = (int)(row / ((size_t)g * g));
    const int px = (k8 % p8) * 8, py = (k8 / p8) % p, c = k8 / (p8 * p);
    const float* src = pix + (((size_t)b * C + c) * Himg + gy * p + py) * Wimg + gx * p + px;
    const f32x4 v0 = *reinterpret_cast<const f32x4*>(src), v1 = *reinterpret_cast<const f32x4*>(src + 4);
    u16x8_e hi, lo;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      unsigned short h0, l0, h1, l1;
      split1(v0[e] * scale, h0, l0);
      split1(v1[e] * scale, h1, l1);
      hi[e] = h0, lo[e] = l0, hi[4 + e] = h1, lo[4 + e] = l1;
    }
    unsigned short* dst = cols + row * 2 * kdim + (size_t)k8 * 8;
    *reinterpret_cast<u16x8_e*>(dst) = hi;
    *reinterpret_cast<u16x8_e*>(dst + kdim) = lo;
  }
}

__global__ void __launch_bounds__(256) vision_assemble_fwd_kernel(const float* __restrict__ patch, const float* __restrict__ cls,
                                                                  const float* __restrict__ pos, float* __restrict__ x, int B,
                                                                  int S, int D4, size_t total4) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (size_t)gridDim.x * blockDim.x) {
    const int d = (int)(i % D4);
    const size_t tok = i / D4;
    const int s = (int)(tok % S);
    const size_t b = tok / S;
    f32x4 v = (s == 0) ? reinterpret_cast<const f32x4*>(cls)[d]
                       : reinterpret_cast<const f32x4*>(patch)[(b * (S - 1) + (s - 1)) * D4 + d];
    reinterpret_cast<f32x4*>(x)[i] = v + reinterpret_cast<const f32x4*>(pos)[(size_t)s * D4 + d];
  }
}

// dpatch[b, i, :] = dx[b, 1+i, :]
__global__ void __launch_bounds__(256) vision_assemble_bwd_kernel(const float* __restrict__ dx, float* __restrict__ dpatch, int B,
                                                                  int S, int D4, size_t total4) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (size_t)gridDim.x * blockDim.x) {
    const int d = (int)(i % D4);
    const size_t tok = i / D4;
    const int s = (int)(tok % (S - 1));
    const size_t b = tok / (S - 1);
    reinterpret_cast<f32x4*>(dpatch)[i] = reinterpret_cast<const f32x4*>(dx)[(b * S + s + 1) * D4 + d];
  }
}

__global__ void __launch_bounds__(256) text_embed_fwd_kernel(const int64_t* __restrict__ ids, const float* __restrict__ tok,
                                                             const float* __restrict__ pos, float* __restrict__ x, int T,
                                                             int D4, int vocab, size_t total4) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (size_t)gridDim.x * blockDim.x) {
    const int d = (int)(i % D4);
    const size_t bt = i / D4;
    const int t = (int)(bt % T);
    int64_t id = ids[bt];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    reinterpret_cast<f32x4*>(x)[i] =
        reinterpret_cast<const f32x4*>(tok)[(size_t)id * D4 + d] + reinterpret_cast<const f32x4*>(pos)[(size_t)t * D4 + d];
  }
}

// dtok[ids[b,t], :] += dx[b,t,:]  (float atomics: rows repeat across the batch)
__global__ void __launch_bounds__(256) text_embed_bwd_kernel(const int64_t* __restrict__ ids, const float* __restrict__ dx,
                                                             float* __restrict__ dtok, int D, int vocab, size_t total) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int d = (int)(i % D);
    const size_t bt = i / D;
    int64_t id = ids[bt];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    atomicAdd(dtok + (size_t)id * D + d, dx[i]);
  }
}

// one wave per caption: index of the first EOS id, 0 if none (argmax of an all-false row)
__global__ void __launch_bounds__(256) first_eos_kernel(const int64_t* __restrict__ ids, int32_t* __restrict__ idx, int B, int T,
                                                        int64_t eos) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  int best = 0x7fffffff;
  for (int t = lane; t < T; t += 64)
    if (ids[(size_t)b * T + t] == eos) best = min(best, t);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o, 64));
  if (lane == 0) idx[b] = (best == 0x7fffffff) ? 0 : best;
}

__global__ void __launch_bounds__(256) gather_rows_kernel(const float* __restrict__ x, const int32_t* __restrict__ idx,
                                                          float* __restrict__ out, int S, int D4, size_t total4) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (size_t)gridDim.x * blockDim.x) {
    const int d = (int)(i % D4);
    const size_t b = i / D4;
    const int s = idx ? idx[b] : 0;
    reinterpret_cast<f32x4*>(out)[i] = reinterpret_cast<const f32x4*>(x)[(b * S + s) * D4 + d];
  }
}

// dx[b,s,:] = (s == idx[b]) ? dout[b,:] : 0   — writes the whole [B,S,D] tensor in one pass
__global__ void __launch_bounds__(256) scatter_rows_kernel(const float* __restrict__ dout, const int32_t* __restrict__ idx,
                                                           float* __restrict__ dx, int S, int D4, size_t total4) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (size_t)gridDim.x * blockDim.x) {
    const int d = (int)(i % D4);
    const size_t tok = i / D4;
    const int s = (int)(tok % S);
    const size_t b = tok / S;
    const int sel = idx ? idx[b] : 0;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (s == sel) v = reinterpret_cast<const f32x4*>(dout)[b * D4 + d];
    reinterpret_cast<f32x4*>(dx)[i] = v;
  }
}

// out[n, :] = x[rows[n], :], rows anywhere in [0, T) in any order, repeats allowed (an index outside is clamped into the range,
// as the token ids of text_embed_fwd are): the residual of the packed tower's last layer on its CLS rows.
__global__ void __launch_bounds__(256) gather_rows_at_kernel(const float* __restrict__ x, const int32_t* __restrict__ rows,
                                                             float* __restrict__ out, int T, int D4, size_t total4) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (size_t)gridDim.x * blockDim.x) {
    const int d = (int)(i % D4);
    int r = rows[i / D4];
    r = r < 0 ? 0 : (r >= T ? T - 1 : r);
    reinterpret_cast<f32x4*>(out)[i] = reinterpret_cast<const f32x4*>(x)[(size_t)r * D4 + d];
  }
}

// x[cu[n] + t, :] = tok[ids[n, t], :] + pos[t, :] for t < len_n = cu[n+1] - cu[n] (at most T): the token rows of N captions
// back to back, each cut after its first EOS.  Grid (N, chunks): a workgroup serves ONE caption, so no thread
// searches the offset table; ids[n, t >= len_n] are never read and nothing is written outside [cu[n], cu[n+1]).  The table
// is clamped into [0, cu[N]] and made non-decreasing as in attn_varlen_fwd_kernel; the id clamp is text_embed_fwd_kernel's.
__global__ void __launch_bounds__(256) text_embed_varlen_kernel(const int64_t* __restrict__ ids, const int32_t* __restrict__ cu,
                                                                const float* __restrict__ tok, const float* __restrict__ pos,
                                                                float* __restrict__ x, int N, int T, int D4, int vocab) {
  const int n = blockIdx.x;
  const int Tp = cu[N];
  const int row0 = min(max(cu[n], 0), Tp);
  const int len = min(min(max(cu[n + 1], row0), Tp) - row0, T);
  const int total4 = len * D4;
  for (int i = blockIdx.y * blockDim.x + threadIdx.x; i < total4; i += gridDim.y * blockDim.x) {
    const int d = i % D4, t = i / D4;
    int64_t id = ids[(size_t)n * T + t];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    reinterpret_cast<f32x4*>(x)[((size_t)row0 + t) * D4 + d] =
        reinterpret_cast<const f32x4*>(tok)[(size_t)id * D4 + d] + reinterpret_cast<const f32x4*>(pos)[(size_t)t * D4 + d];
  }
}

// The backward of text_embed_varlen_kernel, token half: dtok[clamp(ids[n, t]), :] += dx[cu[n] + t, :] for
// t < len_n.  Same grid, table clamp and id clamp as the forward, the float atomics of text_embed_bwd_kernel (ids repeat);
// ids[n, t >= len_n] are never read.
__global__ void __launch_bounds__(256) text_embed_varlen_bwd_tok_kernel(const int64_t* __restrict__ ids, const int32_t* __restrict__ cu,
                                                                        const float* __restrict__ dx, float* __restrict__ dtok, int N,
                                                                        int T, int D, int vocab) {
  const int n = blockIdx.x;
  const int Tp = cu[N];
  const int row0 = min(max(cu[n], 0), Tp);
  const int len = min(min(max(cu[n + 1], row0), Tp) - row0, T);
  const int total = len * D;
  for (int i = blockIdx.y * blockDim.x + threadIdx.x; i < total; i += gridDim.y * blockDim.x) {
    const int d = i % D, t = i / D;
    int64_t id = ids[(size_t)n * T + t];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    atomicAdd(dtok + (size_t)id * D + d, dx[((size_t)row0 + t) * D + d]);
  }
}

// Position half: dpos[t, :] = sum over the captions with len_n > t of dx[cu[n] + t, :], for every t < T (zeros where no
// caption reaches).  One thread per 16-byte group of dpos adds in ascending n — no atomics, the same bits in every run.
__global__ void __launch_bounds__(256) text_embed_varlen_bwd_pos_kernel(const int32_t* __restrict__ cu, const float* __restrict__ dx,
                                                                        float* __restrict__ dpos, int N, int T, int D4) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= T * D4) return;
  const int d = i % D4, t = i / D4;
  const int Tp = cu[N];
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  for (int n = 0; n < N; ++n) {
    const int row0 = min(max(cu[n], 0), Tp);
    const int len = min(min(max(cu[n + 1], row0), Tp) - row0, T);
    if (t < len) s = s + reinterpret_cast<const f32x4*>(dx)[((size_t)row0 + t) * D4 + d];
  }
  reinterpret_cast<f32x4*>(dpos)[i] = s;
}

// dx[cu[n+1] - 1, :] = dout[n, :], every other row of [cu[n], cu[n+1]) zero: the ragged twin of scatter_rows_kernel.  Grid
// (N, chunks), a workgroup serves ONE caption as in text_embed_varlen_kernel; the table is clamped as there.
__global__ void __launch_bounds__(256) scatter_last_rows_kernel(const float* __restrict__ dout, const int32_t* __restrict__ cu,
                                                                float* __restrict__ dx, int N, int D4) {
  const int n = blockIdx.x;
  const int Tp = cu[N];
  const int row0 = min(max(cu[n], 0), Tp);
  const int len = min(max(cu[n + 1], row0), Tp) - row0;
  const size_t total4 = (size_t)len * D4;
  for (size_t i = (size_t)blockIdx.y * blockDim.x + threadIdx.x; i < total4; i += (size_t)gridDim.y * blockDim.x) {
    const int d = (int)(i % D4), t = (int)(i / D4);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (t == len - 1) v = reinterpret_cast<const f32x4*>(dout)[(size_t)n * D4 + d];
    reinterpret_cast<f32x4*>(dx)[((size_t)row0 + t) * D4 + d] = v;
  }
}

}  // namespace

DCLIP_API int dclip_im2col(const float* pixels, float* cols, int B, int C, int Himg, int Wimg, int patch, void* stream) {
  DCLIP_REQUIRE(pixels && cols, "im2col: null pointer");
  DCLIP_REQUIRE(B > 0 && C > 0 && patch > 0 && Himg == Wimg && Himg % patch == 0, "im2col: bad shape %dx%d patch %d", Himg,
                Wimg, patch);
  const int g = Himg / patch;
  const size_t total = (size_t)B * g * g * C * patch * patch;
  const bool vec = patch % 4 == 0 && ((uintptr_t)pixels | (uintptr_t)cols) % 16 == 0;
  if (vec)
    hipLaunchKernelGGL((im2col_vec_kernel<float>), dim3(grid_for(total / 4)), dim3(256), 0, (hipStream_t)stream, pixels, cols, B,
                       C, Himg, Wimg, patch, g, C * patch * patch, total / 4);
  else
    hipLaunchKernelGGL(im2col_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, pixels, cols, B, C, Himg, Wimg,
                       patch, g, total);
  DCLIP_CHECK_LAUNCH_V("im2col", vec ? ".vec" : ".scalar");
  return DCLIP_OK;
}

namespace {
template <class T>
int im2col16(const char* name, const float* pixels, void* cols, int B, int C, int Himg, int Wimg, int patch, int ldc,
             void* stream) {
  DCLIP_REQUIRE(pixels && cols, "%s: null pointer", name);
  DCLIP_REQUIRE(B > 0 && C > 0 && patch > 0 && patch % 4 == 0 && Himg == Wimg && Himg % patch == 0,
                "%s: bad shape %dx%d patch %d (patch must be a multiple of 4)", name, Himg, Wimg, patch);
  DCLIP_REQUIRE(ldc >= C * patch * patch && ldc % 4 == 0 && (uintptr_t)pixels % 16 == 0 && (uintptr_t)cols % 8 == 0,
                "%s: ldc / alignment", name);
  const int g = Himg / patch;
  const size_t total4 = (size_t)B * g * g * C * patch * patch / 4;
  hipLaunchKernelGGL((im2col_vec_kernel<T>), dim3(grid_for(total4)), dim3(256), 0, (hipStream_t)stream, pixels, cols, B, C,
                     Himg, Wimg, patch, g, ldc, total4);
  DCLIP_CHECK_LAUNCH(name);
  return DCLIP_OK;
}
}  // namespace

DCLIP_API int dclip_im2col_bf16(const float* pixels, void* cols, int B, int C, int Himg, int Wimg, int patch, int ldc,
                                void* stream) {
  return im2col16<Bf16T>("im2col_bf16", pixels, cols, B, C, Himg, Wimg, patch, ldc, stream);
}

DCLIP_API int dclip_im2col_f16(const float* pixels, void* cols, int B, int C, int Himg, int Wimg, int patch, int ldc,
                               void* stream) {
  return im2col16<F16T>("im2col_f16", pixels, cols, B, C, Himg, Wimg, patch, ldc, stream);
}

DCLIP_API int dclip_im2col_f16x2(const float* pixels, void* cols, int B, int C, int Himg, int Wimg, int patch, float scale,
                                 const float* scale_dev, void* stream) {
  DCLIP_REQUIRE(pixels && cols, "im2col_f16x2: null pointer");
  DCLIP_REQUIRE(B > 0 && C > 0 && patch > 0 && patch % 8 == 0 && Himg == Wimg && Himg % patch == 0,
                "im2col_f16x2: bad shape %dx%d patch %d (patch must be a multiple of 8)", Himg, Wimg, patch);
  DCLIP_REQUIRE(((uintptr_t)pixels | (uintptr_t)cols) % 16 == 0 && (uintptr_t)scale_dev % 4 == 0, "im2col_f16x2: alignment");
  DCLIP_REQUIRE(scale_dev || (scale > 0.f && scale - scale == 0.f && (__builtin_bit_cast(unsigned int, scale) & 0x007fffffu) == 0),
                "im2col_f16x2: scale must be a power of two");
  const int g = Himg / patch;
  const size_t total8 = (size_t)B * g * g * C * patch * patch / 8;
  hipLaunchKernelGGL(im2col_f16x2_kernel, dim3(grid_for(total8)), dim3(256), 0, (hipStream_t)stream, pixels, (unsigned short*)cols,
                     B, C, Himg, Wimg, patch, g, scale_dev ? 1.f : scale, scale_dev, total8);
  DCLIP_CHECK_LAUNCH("im2col_f16x2");
  return DCLIP_OK;
}

DCLIP_API int dclip_vision_assemble_fwd(const float* patch, const float* cls, const float* pos, float* x, int B, int S, int D,
                                        void* stream) {
  DCLIP_REQUIRE(patch && cls && pos && x, "vision_assemble_fwd: null pointer");
  DCLIP_REQUIRE(B > 0 && S > 1 && D % 4 == 0, "vision_assemble_fwd: bad shape");
  const size_t total4 = (size_t)B * S * D / 4;
  hipLaunchKernelGGL(vision_assemble_fwd_kernel, dim3(grid_for(total4)), dim3(256), 0, (hipStream_t)stream, patch, cls, pos, x,
                     B, S, D / 4, total4);
  DCLIP_CHECK_LAUNCH("vision_assemble_fwd");
  return DCLIP_OK;
}

DCLIP_API int dclip_vision_assemble_bwd(const float* dx, float* dpatch, int B, int S, int D, void* stream) {
  DCLIP_REQUIRE(dx && dpatch, "vision_assemble_bwd: null pointer");
  DCLIP_REQUIRE(B > 0 && S > 1 && D % 4 == 0, "vision_assemble_bwd: bad shape");
  const size_t total4 = (size_t)B * (S - 1) * D / 4;
  hipLaunchKernelGGL(vision_assemble_bwd_kernel, dim3(grid_for(total4)), dim3(256), 0, (hipStream_t)stream, dx, dpatch, B, S,
                     D / 4, total4);
  DCLIP_CHECK_LAUNCH("vision_assemble_bwd");
  return DCLIP_OK;
}

DCLIP_API int dclip_text_embed_fwd(const int64_t* ids, const float* tok, const float* pos, float* x, int B, int T, int D,
                                   int vocab, void* stream) {
  DCLIP_REQUIRE(ids && tok && pos && x, "text_embed_fwd: null pointer");
  DCLIP_REQUIRE(B > 0 && T > 0 && D % 4 == 0 && vocab > 0, "text_embed_fwd: bad shape");
  const size_t total4 = (size_t)B * T * D / 4;
  hipLaunchKernelGGL(text_embed_fwd_kernel, dim3(grid_for(total4)), dim3(256), 0, (hipStream_t)stream, ids, tok, pos, x, T,
                     D / 4, vocab, total4);
  DCLIP_CHECK_LAUNCH("text_embed_fwd");
  return DCLIP_OK;
}

DCLIP_API int dclip_text_embed_bwd(const int64_t* ids, const float* dx, float* dtok, int B, int T, int D, int vocab,
                                   void* stream) {
  DCLIP_REQUIRE(ids && dx && dtok, "text_embed_bwd: null pointer");
  DCLIP_REQUIRE(B > 0 && T > 0 && D > 0 && D % 4 == 0 && vocab > 0, "text_embed_bwd: bad shape");
  const size_t total = (size_t)B * T * D;
  hipLaunchKernelGGL(text_embed_bwd_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, ids, dx, dtok, D, vocab,
                     total);
  DCLIP_CHECK_LAUNCH("text_embed_bwd");
  return DCLIP_OK;
}

DCLIP_API int dclip_first_eos(const int64_t* ids, int32_t* idx, int B, int T, int64_t eos_id, void* stream) {
  DCLIP_REQUIRE(ids && idx && B > 0 && T > 0, "first_eos: bad arguments");
  hipLaunchKernelGGL(first_eos_kernel, dim3(cdiv(B, 4)), dim3(256), 0, (hipStream_t)stream, ids, idx, B, T, eos_id);
  DCLIP_CHECK_LAUNCH("first_eos");
  return DCLIP_OK;
}

DCLIP_API int dclip_gather_rows(const float* x, const int32_t* idx, float* out, int B, int S, int D, void* stream) {
  DCLIP_REQUIRE(x && out && B > 0 && S > 0 && D % 4 == 0, "gather_rows: bad arguments");
  const size_t total4 = (size_t)B * D / 4;
  hipLaunchKernelGGL(gather_rows_kernel, dim3(grid_for(total4)), dim3(256), 0, (hipStream_t)stream, x, idx, out, S, D / 4,
                     total4);
  DCLIP_CHECK_LAUNCH("gather_rows");
  return DCLIP_OK;
}

DCLIP_API int dclip_scatter_rows(const float* dout, const int32_t* idx, float* dx, int B, int S, int D, void* stream) {
  DCLIP_REQUIRE(dout && dx && B > 0 && S > 0 && D % 4 == 0, "scatter_rows: bad arguments");
  const size_t total4 = (size_t)B * S * D / 4;
  hipLaunchKernelGGL(scatter_rows_kernel, dim3(grid_for(total4)), dim3(256), 0, (hipStream_t)stream, dout, idx, dx, S, D / 4,
                     total4);
  DCLIP_CHECK_LAUNCH("scatter_rows");
  return DCLIP_OK;
}

DCLIP_API int dclip_gather_rows_at(const float* x, const int32_t* rows, float* out, int N, int T, int D, void* stream) {
  DCLIP_REQUIRE(x && rows && out, "gather_rows_at: null pointer");
  DCLIP_REQUIRE(N > 0 && T > 0 && D > 0 && D % 4 == 0, "gather_rows_at: bad shape N=%d T=%d D=%d", N, T, D);
  DCLIP_REQUIRE(((uintptr_t)x | (uintptr_t)out) % 16 == 0 && (uintptr_t)rows % 4 == 0,
                "gather_rows_at: x / out must be 16-byte aligned, rows 4-byte aligned");
  const size_t total4 = (size_t)N * (D / 4);
  hipLaunchKernelGGL(gather_rows_at_kernel, dim3(grid_for(total4)), dim3(256), 0, (hipStream_t)stream, x, rows, out, T, D / 4,
                     total4);
  DCLIP_CHECK_LAUNCH("gather_rows_at");
  return DCLIP_OK;
}

DCLIP_API int dclip_text_embed_varlen(const int64_t* ids, const int32_t* cu_seqlens, const float* tok, const float* pos, float* x,
                                      int N, int T, int D, int vocab, void* stream) {
  DCLIP_REQUIRE(ids && cu_seqlens && tok && pos && x, "text_embed_varlen: null pointer");
  DCLIP_REQUIRE(N > 0 && T > 0 && D > 0 && D % 4 == 0 && vocab > 0 && (long long)T * (D / 4) < (1ll << 31),
                "text_embed_varlen: bad shape N=%d T=%d D=%d vocab=%d", N, T, D, vocab);
  DCLIP_REQUIRE(((uintptr_t)tok | (uintptr_t)pos | (uintptr_t)x) % 16 == 0 && (uintptr_t)ids % 8 == 0 &&
                    (uintptr_t)cu_seqlens % 4 == 0,
                "text_embed_varlen: tok / pos / x must be 16-byte aligned, ids 8-byte, cu_seqlens 4-byte aligned");
  hipLaunchKernelGGL(text_embed_varlen_kernel, dim3(N, 4), dim3(256), 0, (hipStream_t)stream, ids, cu_seqlens, tok, pos, x, N, T,
                     D / 4, vocab);
  DCLIP_CHECK_LAUNCH("text_embed_varlen");
  return DCLIP_OK;
}

DCLIP_API int dclip_text_embed_varlen_bwd(const int64_t* ids, const int32_t* cu_seqlens, const float* dx, float* dtok, float* dpos,
                                          int N, int T, int D, int vocab, void* stream) {
  DCLIP_REQUIRE(ids && cu_seqlens && dx && (dtok || dpos), "text_embed_varlen_bwd: null pointer");
  DCLIP_REQUIRE(N > 0 && T > 0 && D > 0 && D % 4 == 0 && vocab > 0 && (long long)T * D < (1ll << 31),
                "text_embed_varlen_bwd: bad shape N=%d T=%d D=%d vocab=%d", N, T, D, vocab);
  DCLIP_REQUIRE(((uintptr_t)dx | (uintptr_t)dpos) % 16 == 0 && (uintptr_t)ids % 8 == 0 &&
                    ((uintptr_t)cu_seqlens | (uintptr_t)dtok) % 4 == 0,
                "text_embed_varlen_bwd: dx / dpos must be 16-byte aligned, ids 8-byte, cu_seqlens / dtok 4-byte aligned");
  if (dtok)
    hipLaunchKernelGGL(text_embed_varlen_bwd_tok_kernel, dim3(N, 4), dim3(256), 0, (hipStream_t)stream, ids, cu_seqlens, dx, dtok,
                       N, T, D, vocab);
  if (dpos)
    hipLaunchKernelGGL(text_embed_varlen_bwd_pos_kernel, dim3(cdiv(T * (D / 4), 256)), dim3(256), 0, (hipStream_t)stream,
                       cu_seqlens, dx, dpos, N, T, D / 4);
  DCLIP_CHECK_LAUNCH("text_embed_varlen_bwd");
  return DCLIP_OK;
}

DCLIP_API int dclip_scatter_last_rows(const float* dout, const int32_t* cu_seqlens, float* dx, int N, int D, void* stream) {
  DCLIP_REQUIRE(dout && cu_seqlens && dx, "scatter_last_rows: null pointer");
  DCLIP_REQUIRE(N > 0 && D > 0 && D % 4 == 0, "scatter_last_rows: bad shape N=%d D=%d", N, D);
  DCLIP_REQUIRE(((uintptr_t)dout | (uintptr_t)dx) % 16 == 0 && (uintptr_t)cu_seqlens % 4 == 0,
                "scatter_last_rows: dout / dx must be 16-byte aligned, cu_seqlens 4-byte aligned");
  hipLaunchKernelGGL(scatter_last_rows_kernel, dim3(N, 4), dim3(256), 0, (hipStream_t)stream, dout, cu_seqlens, dx, N, D / 4);
  DCLIP_CHECK_LAUNCH("scatter_last_rows");
  return DCLIP_OK;
}
