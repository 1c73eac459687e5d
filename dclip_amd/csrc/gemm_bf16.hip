// 16-bit-input GEMM on the bf16 / fp16 MFMAs (fp32 accumulate):  C[M,N] = epilogue( A[M,K] W[N,K]^T ), the split-K form of it,
// and the token-major weight gradient dW = dY^T X.  Callers: the frozen towers in bf16 / fp16 (BASELINE configs c3 / c5, DESIGN.md
// §9 / §9b), the bf16 / fp16 student's forward and backward (§13 / §13b), and the split-fp16 GEMMs of the fp32 towers (§9c-§9f).
//
// gemm_bf16_kernel — gemm_f32.hip's skeleton (block tile 128x128 or 64x64, 4 waves of 2x2 / 1x1 MFMA tiles,
// buffer-load staging with a scalar K walk, double-buffered XOR-swizzled LDS, LDS-transposed 16-byte epilogue) with K-tiles of
// 64 elements = the same 128-byte rows: a lane (row = lane&31, half = lane>>5) reads 16-byte slot 2s+half and holds
// k = 16s + 8*half + {0..7}, exactly one MFMA operand per ds_read_b128.  At 16x the fp32 MFMA rate it is bounded by L2 -> LDS
// traffic (64 KB per 512 MFMA cycles per workgroup), not by the matrix pipes.  gemm_bf16_pp_kernel — the 256x256 ping-pong
// kernel on LDS-DMA, one workgroup per CU, for K % 64 == 0 and at least DCLIP_BF16_BIG_MIN (default 128) tiles; also the
// token-major and segmented weight-gradient forms.  gemm_bf16_ppp_kernel is its persistent form, opt-in and measured slower
// (DCLIP_BF16_PERSIST=1, _PERSIST_MIN).  Those, DCLIP_BF16_BIG_MIN and the two plan thresholds of the fused split-fp16 entries
// (DCLIP_F16X3_MIN, DCLIP_F16X3_TOK_MIN) are the switches this file reads, each per call.
//
// Types: every kernel is a template over the 16-bit type (common.h: Bf16T, F16T, F16IeeeT); only the MFMA
// (v_mfma_f32_{32x32x16,16x16x32}_{bf16,f16}) and the rounding differ.  F16T (saturating) serves the frozen towers and the
// split-fp16 entries (dclip_gemm_f16 / _scaled* / dclip_cast_f32_f16 / dclip_layernorm_fwd_f16), F16IeeeT the fp16 training
// path (dclip_gemm_f16_ex / _splitk / _wgrad_tokmajor* / dclip_cast_f32_f16_ieee / dclip_layernorm_fwd_f16_stats).
#include "common.h"
#include <stdlib.h>
#include <type_traits>

namespace {

typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

constexpr int BKH = 64;  // K-tile in bf16 elements (128 bytes per row)

struct GemmBf16Params {
  const __bf16* A;
  const __bf16* W;
  void* C;
  const float* bias;
  const float* residual;
  int M, N, K;
  int lda, ldw, ldc;
  int epilogue;
  int out_bf16;
  int tiles_m, tiles_n;
  unsigned short* aux;   // bf16 [M][ldc]: GELU writes the pre-activation there, DGELU reads it (training path)
  int k_per_split;       // split-K (gridDim.y > 1): multiple of 64; 0 = whole K
  float* slab;           // split-K partials [split][M][N] fp32 (raw accumulators), or nullptr
  float alpha = 1.f;     // multiplies the accumulator before bias / GELU / residual (dclip_gemm_f16_scaled; 1 elsewhere)
  float out_scale = 0.f; // != 0 (dclip_gemm_f16_scaled_split): C is fp16 [M][ldc >= 3N], the [hi|lo|hi] split of out_scale * result
  // device-scaled forms (dclip_gemm_f16_scaled_dev / _split_dev; split16.hip's plan record): the scales are read from device memory
  const float* alpha_p = nullptr;      // non-null: alpha = *alpha_p
  const float* out_scale_p = nullptr;  // non-null (out_scale != 0 marks the split output): out_scale = *out_scale_p
  float* h32 = nullptr;                // split output: also the fp32 pre-activation (GELU) [M][N], or nullptr
  float* g32 = nullptr;                // split output: also the fp32 result [M][N], or nullptr
  // row-scaled form (dclip_gemm_f16_scaled_rows_dev, the split-fp16 dgrads of DESIGN.md §9e; the ROWS kernel instances only)
  const float* row_alpha = nullptr;    // [M]: C[m][:] = epi(acc * alpha * row_alpha[m]), fp32 output
  const float* aux32 = nullptr;        // fp32 [M][ldc]: the pre-activation h of DGELU (the 16-bit `aux` is not used)
  // segmented token-major form (dclip_gemm_f16_wgrad_tokmajor_seg3; the SEG kernel instance only): gridDim.y =
  // 3 seg_splits, work item y contracts its share of the K rows of segment y / seg_splits, whose operands start a_seg / w_seg
  // COLUMNS into A / W
  int seg_splits = 0;
  int a_seg[3] = {0, 0, 0}, w_seg[3] = {0, 0, 0};
  // statistics form of the row-scaled GEMM (dclip_gemm_f16_scaled_rows_stats_dev; the STATS kernel instance only):
  // partial row tile_m of pmax / psum [tiles_m][N] receives the column statistics of the C values the tile stored
  unsigned* pmax = nullptr;
  float* psum = nullptr;
};

// The ROWS epilogue of the register-staged kernel: v = acc * alpha for 4 columns of row `row`; x row_alpha, then
// gemm_f32_kernel's EPI_DGELU statement on the fp32 h, one 16-byte store.
__device__ __forceinline__ void store_rows4(const GemmBf16Params& p, f32x4 v, int row, size_t off) {
  v = v * p.row_alpha[row];
  if (p.epilogue & DCLIP_EPI_DGELU) {
    const f32x4 h = *reinterpret_cast<const f32x4*>(p.aux32 + off);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] *= quick_gelu_grad_f(h[e]);
  }
  *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(p.C) + off) = v;
}

__device__ __forceinline__ float dev_alpha(const GemmBf16Params& p) { return p.alpha_p ? *p.alpha_p : p.alpha; }
__device__ __forceinline__ float dev_out_scale(const GemmBf16Params& p) { return p.out_scale_p ? *p.out_scale_p : p.out_scale; }

// Split-output store (split16.hip has the stand-alone kernel): v = the final fp32 results of 4 consecutive columns, c = their
// place in the first third of the row; hi = fp16(v s), lo = fp16(v s - hi), written as [hi | lo | hi], N columns apart.  v is
// pinned in registers first: it is the value the fp32 epilogue would have stored, rounded to fp32 BEFORE the conversion.
// P = 2: the two-piece form [hi | lo], the duplicate third not stored.
template <int P = 3>
__device__ __forceinline__ void store_split4(unsigned short* c, int N, f32x4 v, float s) {
  u16x4 hi, lo;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float x = v[e];
    asm volatile("" : "+v"(x));
    x *= s;
    asm volatile("" : "+v"(x));   // and the product: converted twice (once as fp16(fma(x, s, +0))), a result of -0 gave lo = -0 (split16.hip, split1)
    const _Float16 h = (_Float16)x;
    const _Float16 l = (_Float16)(x - (float)h);
    hi[e] = __builtin_bit_cast(unsigned short, h);
    lo[e] = __builtin_bit_cast(unsigned short, l);
  }
  *reinterpret_cast<u16x4*>(c) = hi;
  *reinterpret_cast<u16x4*>(c + N) = lo;
  if (P == 3) *reinterpret_cast<u16x4*>(c + 2 * N) = hi;
}

// 4 consecutive 16-bit values at p (8-byte aligned) -> 4 floats
template <class T>
__device__ __forceinline__ f32x4 load16x4(const unsigned short* p) {
  const u16x4 b = *reinterpret_cast<const u16x4*>(p);
  f32x4 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = T::to_f32(b[e]);
  return v;
}

// Diagnostic build only (`make stamps`, never the product library): per-workgroup shader-clock stamps of the ping-pong
// kernel (entry / K loop start / K loop end / first pass stored / exit; real-time clock at entry and exit; where it ran) into
// a buffer of their own.  tools/bf16_gemm_stamps.py.
#ifdef DCLIP_GEMM_STAMPS
__device__ unsigned long long* g_stamps16 = nullptr;
#define PP_STAMP_V(slot, value)                                                                  \
  do {                                                                                           \
    if (threadIdx.x == 0 && g_stamps16)                                                          \
      g_stamps16[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 16 + (slot)] = (value);         \
  } while (0)
#define PP_STAMP(slot) PP_STAMP_V(slot, __builtin_amdgcn_s_memtime())
#define PP_STAMP_RT(slot) PP_STAMP_V(slot, __builtin_amdgcn_s_memrealtime())
#else
#define PP_STAMP_V(slot, value) do {} while (0)
#define PP_STAMP(slot) do {} while (0)
#define PP_STAMP_RT(slot) do {} while (0)
#endif

__device__ __forceinline__ int xcd_remap16(int bid, int nwg) {
  int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, i = bid >> 3;
  int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + i;
}

template <class T, int BM, int BN, bool ROWS = false>
__global__ void __launch_bounds__(256, 2) gemm_bf16_kernel(GemmBf16Params p) {
  typedef typename T::x8 V8;
  constexpr int WM = 2, WN = 2;
  constexpr int TM = BM / WM, TN = BN / WN;
  constexpr int MT = TM / 32, NT = TN / 32;
  constexpr int A_CHUNKS = BM * 8 / 256, B_CHUNKS = BN * 8 / 256;  // 16-byte chunks per thread per K-tile
  constexpr int ROW = BKH;                                          // bf16 elements per LDS row

  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  __bf16* As = reinterpret_cast<__bf16*>(lds_raw);     // [2][BM*64]
  __bf16* Bs = As + 2 * BM * ROW;                      // [2][BN*64]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int l31 = lane & 31, half = lane >> 5;

  constexpr int GROUP_M = 8;
  const int nwg = p.tiles_m * p.tiles_n;
  const int swz = xcd_remap16(blockIdx.x, nwg);
  const int per_group = GROUP_M * p.tiles_n;
  const int first_m = (swz / per_group) * GROUP_M;
  const int gsize = min(GROUP_M, p.tiles_m - first_m);
  const int tile_m = first_m + (swz % per_group) % gsize, tile_n = (swz % per_group) / gsize;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int kbeg = p.k_per_split ? blockIdx.y * p.k_per_split : 0;
  const int kspan = (p.k_per_split ? min(p.K, kbeg + p.k_per_split) : p.K) - kbeg;   // this work item's share of K
  const int nk = (kspan + BKH - 1) / BKH;

  const __bf16* a_org = p.A + (size_t)m0 * p.lda + kbeg;
  const __bf16* w_org = p.W + (size_t)n0 * p.ldw + kbeg;
  const int a_rows = min(BM, p.M - m0), w_rows = min(BN, p.N - n0);
  // Range checking is per DWORD: with an odd K the last valid element of the LAST row shares its dword with element K,
  // which must therefore be inside the descriptor too (it is inside the allocation: lda, ldw are multiples of 8 and
  // >= K; mask_chunk zeroes it).
  const size_t a_bytes = (((size_t)(a_rows - 1) * p.lda + (p.K - kbeg)) * 2 + 3) & ~(size_t)3,
               w_bytes = (((size_t)(w_rows - 1) * p.ldw + (p.K - kbeg)) * 2 + 3) & ~(size_t)3;
  const __amdgpu_buffer_rsrc_t a_rsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16*>(a_org), 0, (int)min(a_bytes, (size_t)0x7fffffff), 0x00020000);
  const __amdgpu_buffer_rsrc_t w_rsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16*>(w_org), 0, (int)min(w_bytes, (size_t)0x7fffffff), 0x00020000);
  int a_voff[A_CHUNKS], w_voff[B_CHUNKS];
#pragma unroll
  for (int c = 0; c < A_CHUNKS; ++c) {
    const int id = tid + c * 256;
    a_voff[c] = (min(id >> 3, a_rows - 1) * p.lda + (id & 7) * 8) * 2;
  }
#pragma unroll
  for (int c = 0; c < B_CHUNKS; ++c) {
    const int id = tid + c * 256;
    w_voff[c] = (min(id >> 3, w_rows - 1) * p.ldw + (id & 7) * 8) * 2;
  }

  f32x16 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  u32x4 ra[A_CHUNKS], rb[B_CHUNKS];

  auto load_tile = [&](int kt) {
#pragma unroll
    for (int c = 0; c < A_CHUNKS; ++c) ra[c] = __builtin_amdgcn_raw_buffer_load_b128(a_rsrc, a_voff[c], kt * (BKH * 2), 0);
#pragma unroll
    for (int c = 0; c < B_CHUNKS; ++c) rb[c] = __builtin_amdgcn_raw_buffer_load_b128(w_rsrc, w_voff[c], kt * (BKH * 2), 0);
  };
  // `krem` < 64 only in a ragged last tile: zero the elements k >= K (they would read the next row's bytes)
  auto mask_chunk = [&](u32x4 v, int slot, int krem) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int k = slot * 8 + 2 * e;
      unsigned int w = v[e];
      if (k >= krem) w = 0;
      else if (k + 1 >= krem) w &= 0xffffu;
      v[e] = w;
    }
    return v;
  };
  auto store_chunk = [&](int buf, int c, int krem) {
    if (c < A_CHUNKS) {
      const int id = tid + c * 256, row = id >> 3, slot = id & 7;
      u32x4 v = ra[c];
      if (krem < BKH) v = mask_chunk(v, slot, krem);
      *reinterpret_cast<u32x4*>(As + buf * BM * ROW + row * ROW + ((slot ^ ((row >> 1) & 7)) << 3)) = v;
    } else {
      const int cb = c - A_CHUNKS;
      const int id = tid + cb * 256, row = id >> 3, slot = id & 7;
      u32x4 v = rb[cb];
      if (krem < BKH) v = mask_chunk(v, slot, krem);
      *reinterpret_cast<u32x4*>(Bs + buf * BN * ROW + row * ROW + ((slot ^ ((row >> 1) & 7)) << 3)) = v;
    }
  };
  auto read_frags = [&](const __bf16* a, const __bf16* b, int s, V8 (&fa)[MT], V8 (&fb)[NT]) {
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const int row = wm * TM + i * 32 + l31;
      fa[i] = *reinterpret_cast<const V8*>(a + row * ROW + (((2 * s + half) ^ ((row >> 1) & 7)) << 3));
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int row = wn * TN + j * 32 + l31;
      fb[j] = *reinterpret_cast<const V8*>(b + row * ROW + (((2 * s + half) ^ ((row >> 1) & 7)) << 3));
    }
  };
  // One K-tile: 4 k-steps of MT*NT MFMAs; with `stage`, the next tile's loads go out first and its LDS writes are
  // spread behind the MFMA steps (pinned with sched_barrier, as in gemm_f32.hip).
  auto compute = [&](int buf, int kt, bool stage, int krem_next) {
    const __bf16* a = As + buf * BM * ROW;
    const __bf16* b = Bs + buf * BN * ROW;
    constexpr int NCH = A_CHUNKS + B_CHUNKS;
    V8 fa[2][MT], fb[2][NT];
    read_frags(a, b, 0, fa[0], fb[0]);
    __builtin_amdgcn_sched_barrier(0);
    if (stage) load_tile(kt + 1);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      if (s + 1 < 4) read_frags(a, b, s + 1, fa[(s + 1) & 1], fb[(s + 1) & 1]);
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
          acc[i][j] = T::mfma32(fa[s & 1][i], fb[s & 1][j], acc[i][j]);
      if (stage && s >= 1) {  // a third of the chunks goes out behind each of k-steps 1..3
        const int lo = NCH * (s - 1) / 3, hi = (s == 3) ? NCH : NCH * s / 3;
#pragma unroll
        for (int c = 0; c < NCH; ++c)
          if (c >= lo && c < hi) store_chunk(buf ^ 1, c, krem_next);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  };

  load_tile(0);
#pragma unroll
  for (int c = 0; c < A_CHUNKS + B_CHUNKS; ++c) store_chunk(0, c, kspan);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const bool stage = kt + 1 < nk;
    compute(kt & 1, kt, stage, kspan - (kt + 1) * BKH);
    __syncthreads();
  }

  // ---- epilogue: accumulators -> LDS (staging buffers are dead) -> 16-byte rows
  float* ct = reinterpret_cast<float*>(lds_raw);
  static_assert(BM * BN * 4 <= 2 * (BM + BN) * ROW * 2, "C tile must fit in the staging LDS");
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        ct[(wm * TM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half) * BN + wn * TN + j * 32 + l31] = acc[i][j][r];
  __syncthreads();
  constexpr int CHUNKS = BM * BN / 4 / 256;
#pragma unroll
  for (int q = 0; q < CHUNKS; ++q) {
    const int id = tid + q * 256;
    const int lr = id / (BN / 4), lc = (id % (BN / 4)) * 4;
    const int row = m0 + lr, col = n0 + lc;
    if (row >= p.M || col >= p.N) continue;  // N % 4 == 0: a chunk is inside or outside as a whole
    f32x4 v = *reinterpret_cast<const f32x4*>(ct + lr * BN + lc);
    if (p.slab) {   // split-K partial: raw accumulators, the reduce kernel finishes
      *reinterpret_cast<f32x4*>(p.slab + ((size_t)blockIdx.y * p.M + row) * p.N + col) = v;
      continue;
    }
    v = v * dev_alpha(p);
    if (ROWS) {
      store_rows4(p, v, row, (size_t)row * p.ldc + col);
      continue;
    }
    if (p.epilogue & DCLIP_EPI_BIAS) v += *reinterpret_cast<const f32x4*>(p.bias + col);
    const size_t off = (size_t)row * p.ldc + col;
    if (p.epilogue & DCLIP_EPI_GELU) {
      if (p.h32) *reinterpret_cast<f32x4*>(p.h32 + (size_t)row * p.N + col) = v;
      if (p.aux) {
        u16x4 h = {T::bits(v[0]), T::bits(v[1]), T::bits(v[2]), T::bits(v[3])};
        *reinterpret_cast<u16x4*>(p.aux + off) = h;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = T::to_f32(h[e]);   // gelu of what was saved
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = quick_gelu_f(v[e]);
    }
    if (p.epilogue & DCLIP_EPI_DGELU) {
      const f32x4 h = load16x4<T>(p.aux + off);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] *= quick_gelu_grad_f(h[e]);
    }
    if (p.epilogue & DCLIP_EPI_RESIDUAL) v += *reinterpret_cast<const f32x4*>(p.residual + off);
    if (p.out_scale != 0.f) {
      if (p.g32) *reinterpret_cast<f32x4*>(p.g32 + (size_t)row * p.N + col) = v;
      store_split4(reinterpret_cast<unsigned short*>(p.C) + off, p.N, v, dev_out_scale(p));
    } else if (p.out_bf16) {
      u16x4 o = {T::bits(v[0]), T::bits(v[1]), T::bits(v[2]), T::bits(v[3])};
      *reinterpret_cast<u16x4*>(reinterpret_cast<unsigned short*>(p.C) + off) = o;
    } else {
      *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(p.C) + off) = v;
    }
  }
}

// LDS-DMA (`buffer_load_dwordx4 ... lds`, gfx950) of the ping-pong kernel below: no staging registers, no ds_write.  The XOR
// swizzle is applied on the GLOBAL side — lane i of a piece owns LDS granule i, and fetches the 16 bytes that belong there; rows
// past M / N are outside the buffer descriptor and arrive as zeros.  Requires K % 64 == 0 (a ragged row tail cannot be zeroed
// on the DMA path) — every projection of the towers.
// 16 bytes per lane, global -> LDS without passing through registers: lane i lands at lds_dst + 16 i.
// (A __device__ function on purpose: with the builtin inside a lambda of the kernel template, hipcc 7.2 silently drops
// the template's host stub.)
__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t rsrc, __bf16* lds_dst, int voff, int soff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)lds_dst, 16, voff, soff, 0, 0);
}

// the register-staged kernel on BM x BM tiles (p.tiles_m / tiles_n set by the caller), its ROWS instance for a row-scaled call
template <class T, int BM>
int launch_reg(const GemmBf16Params& p, size_t lds, hipStream_t st) {
  if constexpr (std::is_same<T, F16T>::value) {   // the row-scaled entry exists for F16T only
    if (p.row_alpha) {
      hipLaunchKernelGGL((gemm_bf16_kernel<T, BM, BM, true>), dim3(p.tiles_m * p.tiles_n), dim3(256), lds, st, p);
      return DCLIP_OK;
    }
  }
  hipLaunchKernelGGL((gemm_bf16_kernel<T, BM, BM>), dim3(p.tiles_m * p.tiles_n), dim3(256), lds, st, p);
  return DCLIP_OK;
}

#define PP_BARRIER()                      \
  do {                                    \
    __builtin_amdgcn_sched_barrier(0);    \
    __builtin_amdgcn_s_barrier();         \
    __builtin_amdgcn_sched_barrier(0);    \
  } while (0)

// Epilogue of the ping-pong kernel: one wave row (128 x 256 fp32 = the whole LDS) per pass through the dead staging
// buffers.  A thread keeps ONE column group (4 columns) and walks 16 rows, 8 apart: the bias is loaded once, and the side
// operand of a pass (KIND 3 residual, KIND 2 saved pre-activation) is fetched into registers — unconditionally, from
// clamped addresses — BEFORE that pass's stores: vmcnt counts loads and stores together in issue order, so a load
// issued behind stores waits for every one of them, and a load under a per-element condition is waited for alone.
// KIND 0 bias only, 1 quick-GELU (pre-activation saved to aux when given), 2 x dGELU(aux), 3 + residual.
// The MFMAs form C^T blocks (W fragment as the A operand): accumulator register r of block (i, j) is
// C[row 16 i + l15][column 16 j + 4 quad + r] — four consecutive columns per lane, one ds_write_b128 per block.
// DEV (dclip_gemm_f16_scaled_dev / _split_dev): alpha and out_scale are read through p.alpha_p / p.out_scale_p and the fp32
// side outputs h32 / g32 are written; a kernel instance of its own, so that the code of every other caller is what it was.
// ROWS (dclip_gemm_f16_scaled_rows_dev; KIND 0 or 2, fp32 output, DEV): the kernel has already multiplied the accumulators by
// alpha and row_alpha (see there); KIND 2's side operand is the fp32 h (p.aux32) — gemm_f32_kernel's EPI_DGELU statement.
// STATS (ROWS only): C is the dY of a weight gradient, so the tile also leaves the column statistics of what it
// stored.  A thread owns 4 columns and walks 32 rows of the tile: 4 maxima of the bit patterns of |v| and 4 fp32 sums in row
// order; after the last pass the 8 waves put them into the dead LDS and threads 0..255 fold them in wave order into partial
// row m0 / 256 of p.pmax / p.psum.  Rows >= M and columns >= N contribute nothing and write nothing.
// BM (256 or 192): the tile height.  A pass is one wave row of WM = BM / 2 rows, a thread walks WM / 8 of them and
// the wave row stages its BM / 32 accumulator row blocks; every statement applied to a value is the same at both heights.
template <class T, int KIND, bool OUT16, bool DEV = false, bool ROWS = false, bool STATS = false, int BM = 256, int PIECES = 3>
__device__ __forceinline__ void pp_epilogue(const GemmBf16Params& p, const f32x4 (&acc)[BM / 32][4], float* ct, int m0, int n0,
                                            int tid, int wr, int wc, int quad, int l15) {
  constexpr int BN = 256, WM = BM / 2, NQ = WM / 8;
  static_assert(BM == 256 || (BM == 192 && !OUT16 && !STATS), "the 192-row tile has fp32 outputs and no statistics form");
  const int lc = (tid & 63) * 4, col = n0 + lc, lr0 = tid >> 6;
  const bool colok = col < p.N;                     // N % 4 == 0: a column group is inside or outside as a whole
  const int colc = colok ? col : 0;
  f32x4 bias4 = {0.f, 0.f, 0.f, 0.f};
  if (p.epilogue & DCLIP_EPI_BIAS) bias4 = *reinterpret_cast<const f32x4*>(p.bias + colc);
  const float alpha_d = DEV ? *p.alpha_p : 0.f;        // the DEV instance is launched only with alpha_p set
  static_assert(!STATS || ROWS, "the statistics form is the row-scaled one");
  unsigned smx[STATS ? 4 : 1];
  float ssm[STATS ? 4 : 1];
  if constexpr (STATS) {
#pragma unroll
    for (int e = 0; e < 4; ++e) smx[e] = 0u, ssm[e] = 0.f;
  }
#pragma unroll
  for (int hm = 0; hm < 2; ++hm) {
    const int rbase = m0 + hm * WM + lr0;
    f32x4 side[KIND == 3 || (ROWS && KIND == 2) ? NQ : 1];
    u16x4 side16[KIND == 2 && !ROWS ? NQ : 1];
    if (ROWS && KIND == 2) {
#pragma unroll
      for (int q = 0; q < NQ; ++q)
        side[q] = *reinterpret_cast<const f32x4*>(p.aux32 + (size_t)min(rbase + 8 * q, p.M - 1) * p.ldc + colc);
    }
    if (KIND == 3) {
#pragma unroll
      for (int q = 0; q < NQ; ++q)
        side[q] = *reinterpret_cast<const f32x4*>(p.residual + (size_t)min(rbase + 8 * q, p.M - 1) * p.ldc + colc);
    }
    if (KIND == 2 && !ROWS) {
#pragma unroll
      for (int q = 0; q < NQ; ++q)
        side16[q] = *reinterpret_cast<const u16x4*>(p.aux + (size_t)min(rbase + 8 * q, p.M - 1) * p.ldc + colc);
    }
    if (wr == hm) {      // 16-byte granule g of row r is stored at g ^ (r & 7): the 8 rows of a ds_write_b128 lane group spread over 32 banks
#pragma unroll
      for (int i = 0; i < BM / 32; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          *reinterpret_cast<f32x4*>(ct + (16 * i + l15) * BN + (((16 * wc + 4 * j + quad) ^ (l15 & 7)) << 2)) = acc[i][j];
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    PP_BARRIER();
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int row = rbase + 8 * q;
      f32x4 v = *reinterpret_cast<const f32x4*>(ct + (lr0 + 8 * q) * BN + (((tid & 63) ^ ((lr0 + 8 * q) & 7)) << 2));
      if (!ROWS) v = v * (DEV ? alpha_d : p.alpha) + bias4;   // ROWS: the kernel has scaled the accumulators, and there is no bias
      const size_t off = (size_t)row * p.ldc + col;
      const bool ok = row < p.M && colok;
      if (ROWS) {
        if (KIND == 2) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] *= quick_gelu_grad_f(side[q][e]);
        }
        if (ok) *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(p.C) + off) = v;
        if constexpr (STATS) if (ok) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float ve = v[e];
            const unsigned u = __builtin_bit_cast(unsigned, ve) & 0x7fffffffu;
            smx[e] = smx[e] > u ? smx[e] : u;
            ssm[e] += ve;
          }
        }
        continue;
      }
      if (KIND == 1) {
        if (DEV && !OUT16 && p.h32 && ok) *reinterpret_cast<f32x4*>(p.h32 + (size_t)row * p.N + col) = v;
        if (p.aux) {
          u16x4 h = {T::bits(v[0]), T::bits(v[1]), T::bits(v[2]), T::bits(v[3])};
          if (ok) *reinterpret_cast<u16x4*>(p.aux + off) = h;
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = T::to_f32(h[e]);   // gelu of what was saved
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = quick_gelu_f(v[e]);
      }
      if (KIND == 2) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] *= quick_gelu_grad_f(T::to_f32(side16[q][e]));
      }
      if (KIND == 3) v += side[q];
      if (!ok) continue;
      if (BM == 256 && (KIND == 0 || KIND == 1) && !OUT16 && p.out_scale != 0.f) {   // (no split output at 192 rows)
        if (DEV && p.g32) *reinterpret_cast<f32x4*>(p.g32 + (size_t)row * p.N + col) = v;
        store_split4<PIECES>(reinterpret_cast<unsigned short*>(p.C) + off, p.N, v, DEV ? *p.out_scale_p : p.out_scale);
        continue;
      }
      if (OUT16) {
        u16x4 o = {T::bits(v[0]), T::bits(v[1]), T::bits(v[2]), T::bits(v[3])};
        *reinterpret_cast<u16x4*>(reinterpret_cast<unsigned short*>(p.C) + off) = o;
      } else {
        *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(p.C) + off) = v;
      }
    }
    if (hm == 0) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // pass 0's LDS reads are done before pass 1 overwrites them
      PP_BARRIER();
      PP_STAMP(3);             // first pass: stores issued
    }
  }
  PP_STAMP(8);                 // second pass: stores issued
  if constexpr (STATS) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // pass 1's LDS reads are done before the tile is overwritten
    PP_BARRIER();
    unsigned* cu = reinterpret_cast<unsigned*>(ct);         // [8 waves][256] maxima, then [8][256] sums
    float* cs = ct + 8 * BN;
    *reinterpret_cast<u32x4*>(cu + lr0 * BN + lc) = u32x4{smx[0], smx[1], smx[2], smx[3]};
    *reinterpret_cast<f32x4*>(cs + lr0 * BN + lc) = f32x4{ssm[0], ssm[1], ssm[2], ssm[3]};
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    PP_BARRIER();
    if (tid < BN && n0 + tid < p.N) {
      unsigned m = cu[tid];
      float sm = cs[tid];
#pragma unroll
      for (int w = 1; w < 8; ++w) {
        const unsigned mw = cu[w * BN + tid];
        m = m > mw ? m : mw;
        sm += cs[w * BN + tid];
      }
      const size_t o = (size_t)(m0 / 256) * p.N + n0 + tid;
      p.pmax[o] = m;
      p.psum[o] = sm;
    }
  }
#ifdef DCLIP_GEMM_STAMPS
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
  PP_STAMP(4);                 // ... and acknowledged (diagnostic build only: the product kernel ends without waiting)
  PP_STAMP_RT(6);
}

// bf16 outputs without a side operand (qkv projection, fc1 + GELU): bias (and GELU, unless the pre-activation is to be
// saved) are applied in registers, the values are rounded to bf16 THERE, and the whole 256 x 256 tile (128 KiB as bf16)
// is staged at once — both wave rows write together (32 ds_write_b64 per wave instead of 128 ds_write_b32), one barrier
// instead of three, and the copy loop moves 16 bytes per lane: 16 LDS reads pairs + 16 stores per thread for the tile.
// 8-byte unit u of row r is stored at u ^ (r & 15): the 16 rows of a ds_write_b64 lane group cover 32 banks.
// SAVE: the staged value is the pre-activation h (written to aux); C = bf16(gelu(h)) is formed in the copy loop from the
// rounded h, as in the two-pass form.
template <class T, bool GELU, bool SAVE, bool DEV = false>
__device__ __forceinline__ void pp_epilogue_b16(const GemmBf16Params& p, const f32x4 (&acc)[8][4], unsigned short* ct, int m0,
                                                int n0, int tid, int wr, int wc, int quad, int l15) {
  constexpr int BN = 256;
  {
    f32x4 bias4[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = n0 + 64 * wc + 16 * j + 4 * quad;
      bias4[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (p.epilogue & DCLIP_EPI_BIAS) bias4[j] = *reinterpret_cast<const f32x4*>(p.bias + (col < p.N ? col : 0));
    }
    const float alpha_d = DEV ? *p.alpha_p : 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        f32x4 v = acc[i][j] * (DEV ? alpha_d : p.alpha) + bias4[j];
        if (GELU && !SAVE) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = quick_gelu_f(v[e]);
        }
        const u16x4 h = {T::bits(v[0]), T::bits(v[1]), T::bits(v[2]), T::bits(v[3])};
        const int row = 128 * wr + 16 * i + l15, unit = 16 * wc + 4 * j + quad;
        *reinterpret_cast<u16x4*>(ct + row * BN + ((unit ^ (row & 15)) << 2)) = h;
      }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  PP_BARRIER();
  PP_STAMP(3);
  const int cg = tid & 31, col = n0 + 8 * cg;       // 8 columns = two 8-byte units per thread and row
#pragma unroll 4
  for (int q = 0; q < 16; ++q) {
    const int lr = (tid >> 5) + 16 * q, row = m0 + lr;
    const u16x4 lo = *reinterpret_cast<const u16x4*>(ct + lr * BN + (((2 * cg) ^ (lr & 15)) << 2));
    const u16x4 hi = *reinterpret_cast<const u16x4*>(ct + lr * BN + (((2 * cg + 1) ^ (lr & 15)) << 2));
    if (row >= p.M || col >= p.N) continue;
    const size_t off = (size_t)row * p.ldc + col;
    const bool full = col + 8 <= p.N;               // N % 4 == 0: the second unit is inside or outside as a whole
    typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
    u16x8 o = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    if (SAVE) {
      if (full) *reinterpret_cast<u16x8*>(p.aux + off) = o;
      else *reinterpret_cast<u16x4*>(p.aux + off) = lo;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = T::bits(quick_gelu_f(T::to_f32(o[e])));
    }
    unsigned short* c = reinterpret_cast<unsigned short*>(p.C) + off;
    if (full) *reinterpret_cast<u16x8*>(c) = o;
    else *reinterpret_cast<u16x4*>(c) = u16x4{o[0], o[1], o[2], o[3]};
  }
  PP_STAMP(8);
#ifdef DCLIP_GEMM_STAMPS
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
  PP_STAMP(4);
  PP_STAMP_RT(6);
}

// ---------------------------------------------------------------------------------------------------------------
// Ping-pong variant of the 256x256x64 tile (8 waves = 2 x 4, wave tile 128x64, v_mfma_f32_16x16x32_bf16): the two
// waves of a SIMD belong to different wave rows (wr = wave >> 2) and run ONE BARRIER APART, so that while one issues
// its LDS fragment reads and the next LDS-DMA pieces the other has the matrix pipe — a K loop that runs both waves of
// a SIMD in step (one barrier per K-tile: the lock-step kernel this one replaced) measured ~4.2k cycles
// per K-tile against the 2,048 of the MFMAs alone.  Per K-tile four phases, one 64x32 quadrant of the wave tile each
// (16 MFMAs = 256 cycles):
//     phase 1  read B(qn 0) 4 + A(qm 0) 8 fragments | DMA A-half 1 of tile kt+1 | MFMA quadrant (0,0)
//     phase 2  read B(qn 1) 4                         | DMA B-half 0 of tile kt+2 | MFMA (0,1)
//     phase 3  read A(qm 1) 8                         | DMA A-half 0 of tile kt+2 | MFMA (1,1)
//     phase 4  -                                      | DMA B-half 1 of tile kt+2, vmcnt(6) | MFMA (1,0)
// each phase = [reads + DMA issue] barrier [lgkmcnt(0), MFMAs] barrier.  A "half" is the set of rows every wave needs
// for its quadrant row / column h (A: rows with bit 6 == h, B: rows with bit 5 == h), 16 DMA pieces = 2 per wave.
// Ordering (DMA data is ordered for a ds_read only by the issuing waves' counted vmcnt followed by a barrier the reader
// has passed; the groups are a barrier apart, so reads come one PHASE after the wait):
//   RAW  phase 4's vmcnt(6) leaves the three half-tiles of kt+2 in flight and retires all of kt+1, read from phase 1 of
//        kt+1 on; the last tiles wait vmcnt(0).
//   WAR  a half is re-staged two phases after its last read (A0: read phase 1, staged phase 3; B1: 2 -> 4; A1: 3 -> 1
//        of the next tile), B0 one phase after (read first in phase 1 and retired by lgkmcnt(8) BEFORE that phase's
//        first barrier).
// Every wave executes the same number of s_barrier: wave row 1 one extra before the loop, wave row 0 one after it.
// TOK (token-major operands, the weight gradients dW[out,in] = dY^T X of the bf16 training path WITHOUT the transposes):
// A = dY [K = tokens][M = out] and W = X [K][N = in] are read as they lie.  A K-tile half is then a [64 k][256 B] LDS
// image (the 64-column quadrant slices of the two wave rows / the 32-column slices of the four wave columns side by
// side), filled by DMA pieces of 4 k-rows, and the MFMA operands — lane (l15, quad) needs 8 consecutive k of ONE column —
// come out of it through the transposing LDS read (ds_read_b64_tr_b16: 4 k x 16 columns per 16 lanes, two per operand).
// 16-byte granule g of k-row r is stored at g ^ (((r & 3) << 2) | (((r >> 3) & 1) << 1)): the 4 k-rows of a read and the
// two lane groups of a half-wave (k-rows 8 apart) land on 32 different 8-byte bank pairs.  Same phases and barriers; the
// DMA order is A1(kt+1) | - | A0(kt+2) | B0, B1(kt+2) (every half re-staged at least two phases after its last read, so
// no lgkmcnt before a barrier is needed: phase 1 issues 24 reads, more than the 4-bit counter can express).
// SEG (token-major only): the contraction is three segments of K rows; the split index selects the segment, so a work item
// stays inside one segment and the K loop, phases and barriers are what they were.  Always split-K (>= 3 slabs).
// STATS (ROWS only): pp_epilogue's statistics form; nothing else differs.
// FUSED (the dclip_gemm_f16x3_* entries): the split-fp16 sum A_hi W_hi + A_lo W_hi + A_hi W_lo out of ONE staging of
// the four distinct pieces.  A K-tile is 32 logical k: k-step 0 (granules 0-3 / k-rows 0-31) holds their hi pieces, k-step 1
// (granules 4-7 / k-rows 32-63) their lo pieces, fetched from the column offsets a_seg / w_seg [0] (hi) and [1] (lo), and a
// phase issues three products per accumulator (24 MFMAs) on the same 12 fragment reads and 2 DMA pieces.  p.K is the logical K
// (a multiple of 32; the token-major form contracts whole 64-token units per split).  Same phases, barriers and counted waits.
// BM = 192 (K-major, FUSED, fp32 output): a 192 x 256 tile for the shapes whose 256-row tiles fill the chip only
// to 0.6 — a third more workgroups in the same single round, each with three quarters of the MFMAs, A reads and A pieces.  The
// wave tile is WM = 96 rows, a quadrant QM = 48 rows = IB = 3 row blocks (18 MFMAs per product and phase); the phases, the eight
// barriers per K-tile and the stagger are those above.  The A rows lie at their natural index and the B rows from row BM on; all
// fragment and piece row offsets stay multiples of 16 / 8, so both sides of the XOR swizzle hold as written.
//   A pieces  A-half h is rows WM w + QM h + r, w in {0, 1}, r < 48: 12 pieces of 8 rows where the 256 form has 16.  Piece
//        q = wave + 8 x covers w = q / 6, r = 8 (q % 6) .. for q < 12.  The choice taken for the remaining four: waves 4-7 still
//        ISSUE their second piece, with every lane outside the buffer range (no memory request, zeros), into a 1-KiB-per-wave dump
//        region behind the two buffers, inside the one LDS array and read by nobody.  So every wave issues two pieces per half,
//        and the counted waits (vmcnt(6), the prologue's) mean what they mean above — no per-wave wait counts.
//   RAW  unchanged: a wave's vmcnt(6) in phase 4 retires all of ITS pieces of tile kt+1 (dump pieces retire in order like any
//        other), the barrier behind it publishes them, and the first read of kt+1 comes a phase later.
//   WAR  unchanged in phases: A0 (96 rows: both wave rows' quadrant 0) is read in phase 1 and re-staged in phase 3, A1 read in 3
//        and re-staged in phase 1 of the next tile, B1 2 -> 4, and B0 one phase after its read.  That last one is retired before
//        phase 1's first barrier by counting the A reads issued BEHIND the four B reads: lgkmcnt(2 IB) — 6 here, 8 at 256 rows.
//        The dump region has no reader, and its writers all write zeros.
// No TOK / SEG / STATS / 16-bit or split output / persistent form at 192 rows: the host keeps those calls on 256.
// PIECES = 2: the fused K-major split-output call whose C is [hi | lo], ldc >= 2 N — the epilogue's third store left
// out, nothing else; an instance of its own (BIAS / BIAS | GELU only), so that the three-piece instances stay what they were.
template <class T, bool TOK, bool DEV = false, bool ROWS = false, bool SEG = false, bool STATS = false, bool FUSED = false,
          int BM = 256, int PIECES = 3>
__global__ void __launch_bounds__(512) gemm_bf16_pp_kernel(GemmBf16Params p) {
  static_assert(PIECES == 3 || (PIECES == 2 && FUSED && !TOK && !ROWS && BM == 256), "two pieces: the fused split-output call");
  static_assert(!SEG || (TOK && !DEV && !ROWS), "the segmented form is token-major, split-K, fp32 slabs");
  static_assert(!FUSED || !SEG, "the fused form does all three products in one work item");
  constexpr int KT = FUSED ? BKH / 2 : BKH;   // logical k per K-tile
  static_assert(!STATS || (ROWS && !TOK), "the statistics form is the row-scaled dgrad");
  static_assert(BM == 256 || (BM == 192 && FUSED && !TOK && !SEG && !STATS), "the 192-row tile is K-major, fused, no statistics");
  typedef typename T::x8 V8;
  constexpr int BN = 256, ROW = BKH;
  constexpr int WM = BM / 2, QM = WM / 2, IB = QM / 16;   // wave tile rows, quadrant rows, 16-row blocks per quadrant
  constexpr int BUF = (BM + BN) * ROW;   // bf16 elements per K-tile buffer: BM A rows then 256 B rows of 128 bytes
  constexpr int DUMP = BM == 256 ? 0 : 8 * 1024;   // bytes behind the buffers for the pieces that fetch nothing (192 rows only)
  __shared__ __attribute__((aligned(16))) unsigned char lds_raw[2 * BUF * 2 + DUMP];   // 128 KiB (120 KiB): the ONLY LDS object
  __bf16* lds = reinterpret_cast<__bf16*>(lds_raw);

  PP_STAMP(0);
  PP_STAMP_RT(5);
  PP_STAMP_V(7, (unsigned long long)__builtin_amdgcn_s_getreg((4) | (0 << 6) | (31 << 11)) |
                    ((unsigned long long)__builtin_amdgcn_s_getreg((20) | (0 << 6) | (3 << 11)) << 32));   // HW_ID, XCC_ID
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wc = wave & 3;
  const int l15 = lane & 15, quad = lane >> 4;

  constexpr int GROUP_M = 8;
  const int nwg = p.tiles_m * p.tiles_n;
  const int swz = xcd_remap16(blockIdx.x, nwg);
  const int per_group = GROUP_M * p.tiles_n;
  const int first_m = (swz / per_group) * GROUP_M;
  const int gsize = min(GROUP_M, p.tiles_m - first_m);
  const int tile_m = first_m + (swz % per_group) % gsize, tile_n = (swz % per_group) / gsize;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  // split-K (gridDim.y > 1): this work item contracts k in [kbeg, kbeg + kspan), both multiples of 64 (host check)
  int ksplit = blockIdx.y, a_col0 = 0, w_col0 = 0;
  if constexpr (SEG) {
    const int seg = (int)blockIdx.y / p.seg_splits;
    ksplit = (int)blockIdx.y - seg * p.seg_splits;
    a_col0 = seg == 0 ? p.a_seg[0] : (seg == 1 ? p.a_seg[1] : p.a_seg[2]);
    w_col0 = seg == 0 ? p.w_seg[0] : (seg == 1 ? p.w_seg[1] : p.w_seg[2]);
  }
  const int kbeg = p.k_per_split ? ksplit * p.k_per_split : 0;
  const int kspan = (p.k_per_split ? min(p.K, kbeg + p.k_per_split) : p.K) - kbeg;
  const int nk = kspan / KT;

  const __bf16* a_org = TOK ? p.A + (size_t)kbeg * p.lda + m0 + a_col0 : p.A + (size_t)m0 * p.lda + kbeg;
  const __bf16* w_org = TOK ? p.W + (size_t)kbeg * p.ldw + n0 + w_col0 : p.W + (size_t)n0 * p.ldw + kbeg;
  const int a_rows = min(BM, p.M - m0), w_rows = min(BN, p.N - n0);
  size_t a_bytes = TOK ? ((size_t)(p.K - kbeg - 1) * p.lda + a_rows) * 2 : ((size_t)(a_rows - 1) * p.lda + (p.K - kbeg)) * 2,
         w_bytes = TOK ? ((size_t)(p.K - kbeg - 1) * p.ldw + w_rows) * 2 : ((size_t)(w_rows - 1) * p.ldw + (p.K - kbeg)) * 2;
  if constexpr (FUSED) {   // the hi / lo column offsets are part of the lanes' offsets: the range ends behind the farther segment
    a_bytes += (size_t)max(p.a_seg[0], p.a_seg[1]) * 2;
    w_bytes += (size_t)max(p.w_seg[0], p.w_seg[1]) * 2;
  }
  const __amdgpu_buffer_rsrc_t a_rsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16*>(a_org), 0, (int)min(a_bytes, (size_t)0x7fffffff), 0x00020000);
  const __amdgpu_buffer_rsrc_t w_rsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16*>(w_org), 0, (int)min(w_bytes, (size_t)0x7fffffff), 0x00020000);
  // scalar byte advance per K-tile
  const int a_kstep = TOK ? KT * p.lda * 2 : KT * 2, w_kstep = TOK ? KT * p.ldw * 2 : KT * 2;
  // DMA pieces.  K-major: 8 rows x 128 B, lane i -> row i >> 3, stored slot i & 7 = logical granule slot ^ ((row >> 1) & 7);
  // A-half h: piece x of this wave covers rows 128 x + 64 h + 8 wave; B-half h: rows 64 (2 x + (wave >> 2)) + 32 h + 8 (wave & 3).
  // Token-major: 4 k-rows x 256 B of a half image, piece x of this wave = k-rows 4 (wave + 8 x) ..; lane i -> k-row i >> 4,
  // stored granule i & 15 = logical granule ^ swizzle(k-row); logical granule g of an A half-row holds columns 128 (g >> 3) +
  // 64 h + 8 (g & 7) .., of a B half-row columns 64 (g >> 2) + 32 h + 8 (g & 3) ...
  // FUSED.  K-major: logical granule g < 4 is k 8 g .. of the hi segment, g >= 4 is k 8 (g - 4) .. of the lo segment.  Token-major:
  // piece 0 (k-rows 0-31) is tokens 4 wave + (lane >> 4) of the hi columns, piece 1 (k-rows 32-63) the same tokens of the lo columns.
  int a_voff[2][2], w_voff[2][2];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int x = 0; x < 2; ++x) {
      if constexpr (FUSED) {
        if (TOK) {
          const int k = 4 * (wave + 8 * x) + (lane >> 4), tok = k & 31;
          const int lg = (lane & 15) ^ (((k & 3) << 2) | (((k >> 3) & 1) << 1));
          const int ma = 128 * (lg >> 3) + 64 * h + 8 * (lg & 7), nb = 64 * (lg >> 2) + 32 * h + 8 * (lg & 3);
          a_voff[h][x] = ma < a_rows ? (tok * p.lda + p.a_seg[x] + ma) * 2 : 0x7fffffff;
          w_voff[h][x] = nb < w_rows ? (tok * p.ldw + p.w_seg[x] + nb) * 2 : 0x7fffffff;
        } else {
          // (192 rows: piece q = wave + 8 x is rows 96 (q / 6) + 48 h + 8 (q % 6) ..; q >= 12 fetches nothing, row 192 is past a_rows)
          const int qa = wave + 8 * x;
          const int ra = (BM == 256 ? 128 * x + 64 * h + 8 * wave : qa < 12 ? WM * (qa / 6) + QM * h + 8 * (qa % 6) : BM) + (lane >> 3);
          const int ga = (lane & 7) ^ ((ra >> 1) & 7);
          a_voff[h][x] = ra < a_rows ? (ra * p.lda + (ga < 4 ? p.a_seg[0] : p.a_seg[1]) + (ga & 3) * 8) * 2 : 0x7fffffff;
          const int rb = 64 * (2 * x + (wave >> 2)) + 32 * h + 8 * (wave & 3) + (lane >> 3), gb = (lane & 7) ^ ((rb >> 1) & 7);
          w_voff[h][x] = rb < w_rows ? (rb * p.ldw + (gb < 4 ? p.w_seg[0] : p.w_seg[1]) + (gb & 3) * 8) * 2 : 0x7fffffff;
        }
      } else if (TOK) {
        const int k = 4 * (wave + 8 * x) + (lane >> 4);
        const int lg = (lane & 15) ^ (((k & 3) << 2) | (((k >> 3) & 1) << 1));
        const int ma = 128 * (lg >> 3) + 64 * h + 8 * (lg & 7), nb = 64 * (lg >> 2) + 32 * h + 8 * (lg & 3);
        a_voff[h][x] = ma < a_rows ? (k * p.lda + ma) * 2 : 0x7fffffff;     // columns past M / N -> zeros in LDS
        w_voff[h][x] = nb < w_rows ? (k * p.ldw + nb) * 2 : 0x7fffffff;
      } else {
        const int ra = 128 * x + 64 * h + 8 * wave + (lane >> 3), ga = (lane & 7) ^ ((ra >> 1) & 7);
        a_voff[h][x] = ra < a_rows ? (ra * p.lda + ga * 8) * 2 : 0x7fffffff;   // out of range -> zeros in LDS
        const int rb = 64 * (2 * x + (wave >> 2)) + 32 * h + 8 * (wave & 3) + (lane >> 3), gb = (lane & 7) ^ ((rb >> 1) & 7);
        w_voff[h][x] = rb < w_rows ? (rb * p.ldw + gb * 8) * 2 : 0x7fffffff;
      }
    }
  constexpr int HALF = 64 * 128;   // bf16 elements of a token-major half image (16 KiB): A0 | A1 | B0 | B1 per buffer
  // 192 rows: LDS element offsets of this wave's two A pieces inside a half (scalars).  The second piece of waves 4-7 goes to the
  // dump region whatever the buffer and the half: a192_in selects which.
  const int a192_e0 = (WM * (wave / 6) + 8 * (wave % 6)) * ROW;
  const bool a192_in = wave < 4;
  const int a192_e1 = a192_in ? (WM + 8 * (wave + 2)) * ROW : 2 * BUF + wave * 512;
#define PP_ISSUE_A(h, buf, kt)                                                                                          \
  do {                                                                                                                  \
    if (TOK) {                                                                                                          \
      dma16(a_rsrc, lds + (buf) * BUF + (h) * HALF + wave * 512, a_voff[h][0], (kt) * a_kstep);                         \
      dma16(a_rsrc, lds + (buf) * BUF + (h) * HALF + (wave + 8) * 512, a_voff[h][1], (kt) * a_kstep);                   \
    } else if (BM == 192) {                                                                                             \
      dma16(a_rsrc, lds + (buf) * BUF + QM * (h) * ROW + a192_e0, a_voff[h][0], (kt) * a_kstep);                        \
      dma16(a_rsrc, lds + (a192_in ? (buf) * BUF + QM * (h) * ROW : 0) + a192_e1, a_voff[h][1], (kt) * a_kstep);        \
    } else {                                                                                                            \
      dma16(a_rsrc, lds + (buf) * BUF + (64 * (h) + 8 * wave) * ROW, a_voff[h][0], (kt) * a_kstep);                     \
      dma16(a_rsrc, lds + (buf) * BUF + (128 + 64 * (h) + 8 * wave) * ROW, a_voff[h][1], (kt) * a_kstep);               \
    }                                                                                                                   \
  } while (0)
#define PP_ISSUE_B(h, buf, kt)                                                                                          \
  do {                                                                                                                  \
    if (TOK) {                                                                                                          \
      dma16(w_rsrc, lds + (buf) * BUF + (2 + (h)) * HALF + wave * 512, w_voff[h][0], (kt) * w_kstep);                   \
      dma16(w_rsrc, lds + (buf) * BUF + (2 + (h)) * HALF + (wave + 8) * 512, w_voff[h][1], (kt) * w_kstep);             \
    } else {                                                                                                            \
      dma16(w_rsrc, lds + (buf) * BUF + (BM + 64 * (wave >> 2) + 32 * (h) + 8 * (wave & 3)) * ROW, w_voff[h][0],        \
            (kt) * w_kstep);                                                                                            \
      dma16(w_rsrc, lds + (buf) * BUF + (BM + 128 + 64 * (wave >> 2) + 32 * (h) + 8 * (wave & 3)) * ROW, w_voff[h][1],  \
            (kt) * w_kstep);                                                                                            \
    }                                                                                                                   \
  } while (0)

  // fragment addresses.  K-major: row 16 blk + l15, k-step s: logical granule 4 s + quad, stored at granule ^ (l15 >> 1).
  const int sw = l15 >> 1;
  const __bf16* pa0 = lds + (WM * wr + l15) * ROW + (((0 + quad) ^ sw) << 3);
  const __bf16* pa1 = lds + (WM * wr + l15) * ROW + (((4 + quad) ^ sw) << 3);
  const __bf16* pb0 = lds + (BM + 64 * wc + l15) * ROW + (((0 + quad) ^ sw) << 3);
  const __bf16* pb1 = lds + (BM + 64 * wc + l15) * ROW + (((4 + quad) ^ sw) << 3);
  // Token-major: a lane of a 16-lane group addresses k-row 8 quad + (l15 >> 2) (+ 32 s + 4 u) at columns 4 (l15 & 3) .. of the
  // 16-column block and receives 4 consecutive k of column l15; block i of the A quadrant is granule 8 wr + 2 i + ((l15 & 3) >> 1),
  // block j of the B quadrant granule 4 wc + 2 j + ((l15 & 3) >> 1), both XOR the lane's swizzle; byte 8 (l15 & 1) inside it.
  const unsigned char* lds8 = lds_raw;
  const int tq = l15 >> 2, swzl = (tq << 2) | ((quad & 1) << 1);
  const int trow = (8 * quad + tq) * 256 + 8 * (l15 & 1);
  int ta[4], tb[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) ta[i] = trow + (((8 * wr + 2 * i + ((l15 & 3) >> 1)) ^ swzl) << 4);
#pragma unroll
  for (int j = 0; j < 2; ++j) tb[j] = trow + (((4 * wc + 2 * j + ((l15 & 3) >> 1)) ^ swzl) << 4);
  auto tr8 = [&](int byte_off) {      // 8 consecutive k of this lane's column: two transposing reads, k-rows 4 apart
    typedef short s16x4_t __attribute__((ext_vector_type(4)));
    typedef short s16x8_t __attribute__((ext_vector_type(8)));
    const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(lds8 + byte_off));
    const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(lds8 + byte_off + 1024));
    return __builtin_bit_cast(V8, s16x8_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]});
  };

  f32x4 acc[2 * IB][4];
#pragma unroll
  for (int i = 0; i < 2 * IB; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  V8 fa[IB][2], fb0[2][2], fb1[2][2];

#define PP_READ_A(qm, off)                                                                          \
  _Pragma("unroll") for (int i = 0; i < IB; ++i) {                                                  \
    if (TOK) {                                                                                      \
      fa[i][0] = tr8((off) * 2 + (qm) * (HALF * 2) + ta[i]);                                        \
      fa[i][1] = tr8((off) * 2 + (qm) * (HALF * 2) + ta[i] + 32 * 256);                             \
    } else {                                                                                        \
      fa[i][0] = *reinterpret_cast<const V8*>(pa0 + (off) + (QM * (qm) + 16 * i) * ROW);        \
      fa[i][1] = *reinterpret_cast<const V8*>(pa1 + (off) + (QM * (qm) + 16 * i) * ROW);        \
    }                                                                                               \
  }
#define PP_READ_B(fb, qn, off)                                                                      \
  _Pragma("unroll") for (int j = 0; j < 2; ++j) {                                                   \
    if (TOK) {                                                                                      \
      fb[j][0] = tr8((off) * 2 + (2 + (qn)) * (HALF * 2) + tb[j]);                                  \
      fb[j][1] = tr8((off) * 2 + (2 + (qn)) * (HALF * 2) + tb[j] + 32 * 256);                       \
    } else {                                                                                        \
      fb[j][0] = *reinterpret_cast<const V8*>(pb0 + (off) + (32 * (qn) + 16 * j) * ROW);        \
      fb[j][1] = *reinterpret_cast<const V8*>(pb1 + (off) + (32 * (qn) + 16 * j) * ROW);        \
    }                                                                                               \
  }
  // (FUSED: product s = 0 W_hi A_hi, 1 W_hi A_lo, 2 W_lo A_hi; the product index outermost keeps two MFMAs on one accumulator 8 apart)
#define PP_MFMA(qm, qn, fb)                                                                                         \
  do {                                                                                                              \
    __builtin_amdgcn_s_setprio(1);                                                                                  \
    _Pragma("unroll") for (int s = 0; s < (FUSED ? 3 : 2); ++s)                                                     \
    _Pragma("unroll") for (int i = 0; i < IB; ++i)                                                                  \
    _Pragma("unroll") for (int j = 0; j < 2; ++j)                                                                   \
      acc[IB * (qm) + i][2 * (qn) + j] =                                                                            \
          T::mfma16(fb[j][FUSED ? s >> 1 : s], fa[i][FUSED ? s & 1 : s], acc[IB * (qm) + i][2 * (qn) + j]);         \
    __builtin_amdgcn_s_setprio(0);                                                                                  \
  } while (0)

  // prologue: all of tile 0 and three halves of tile 1 (the fourth goes out in phase 1 of tile 0)
  PP_ISSUE_A(0, 0, 0);
  PP_ISSUE_B(0, 0, 0);
  PP_ISSUE_B(1, 0, 0);
  PP_ISSUE_A(1, 0, 0);
  if (nk > 1) {
    PP_ISSUE_B(0, 1, 1);
    PP_ISSUE_A(0, 1, 1);
    PP_ISSUE_B(1, 1, 1);
    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  PP_BARRIER();
  PP_STAMP(1);                 // first K-tile landed
  if (wr == 1) PP_BARRIER();   // wave row 1 runs one barrier behind wave row 0

  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1, off = cur * BUF;
    const bool n1 = kt + 1 < nk, n2 = kt + 2 < nk;
    // ---- phase 1
    PP_READ_B(fb0, 0, off);
    __builtin_amdgcn_sched_barrier(0);
    PP_READ_A(0, off);
    __builtin_amdgcn_sched_barrier(0);
    if (n1) PP_ISSUE_A(1, cur ^ 1, kt + 1);
    // the B reads are done (the 2 IB A reads behind them may be outstanding): their rows may be re-staged next phase
    if (!TOK && BM == 256) asm volatile("s_waitcnt lgkmcnt(8)" ::: "memory");
    if (!TOK && BM == 192) asm volatile("s_waitcnt lgkmcnt(6)" ::: "memory");
    PP_BARRIER();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    PP_MFMA(0, 0, fb0);
    PP_BARRIER();
    // ---- phase 2
    PP_READ_B(fb1, 1, off);
    __builtin_amdgcn_sched_barrier(0);
    if (!TOK && n2) PP_ISSUE_B(0, cur, kt + 2);
    PP_BARRIER();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    PP_MFMA(0, 1, fb1);
    PP_BARRIER();
    // ---- phase 3
    PP_READ_A(1, off);
    __builtin_amdgcn_sched_barrier(0);
    if (n2) PP_ISSUE_A(0, cur, kt + 2);
    PP_BARRIER();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    PP_MFMA(1, 1, fb1);
    PP_BARRIER();
    // ---- phase 4
    if (n2) {
      if (TOK) PP_ISSUE_B(0, cur, kt + 2);               // (token-major: B0 here instead of phase 2, see the kernel's header)
      PP_ISSUE_B(1, cur, kt + 2);
      asm volatile("s_waitcnt vmcnt(6)" ::: "memory");   // tile kt+1 has landed (this wave's pieces)
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    PP_BARRIER();
    PP_MFMA(1, 0, fb0);
    PP_BARRIER();
  }
  if (wr == 0) PP_BARRIER();   // balance the stagger: everybody is past its last MFMA phase and LDS read
  PP_STAMP(2);                 // K loop done
#undef PP_ISSUE_A
#undef PP_ISSUE_B
#undef PP_READ_A
#undef PP_READ_B
#undef PP_MFMA

  // ---- epilogue (pp_epilogue above), one instance per epilogue kind and output type
  const int kind = (p.epilogue & DCLIP_EPI_RESIDUAL) ? 3 : (p.epilogue & DCLIP_EPI_DGELU) ? 2 : (p.epilogue & DCLIP_EPI_GELU) ? 1 : 0;
  float* ct = reinterpret_cast<float*>(lds_raw);
  if constexpr (PIECES == 2) {   // split output only (host check): BIAS or BIAS | GELU
    if (kind == 1) pp_epilogue<T, 1, false, DEV, false, false, BM, 2>(p, acc, ct, m0, n0, tid, wr, wc, quad, l15);
    else pp_epilogue<T, 0, false, DEV, false, false, BM, 2>(p, acc, ct, m0, n0, tid, wr, wc, quad, l15);
    return;
  }
  if (ROWS) {             // row-scaled dgrad: fp32 output, no epilogue or DGELU on the fp32 h
    // both scales are applied to the accumulators HERE, in the order of the other kernels — (acc * alpha) * row_alpha — with
    // the 8 (6) row_alpha values of a lane fetched before any side operand: 16 more registers inside pp_epilogue would spill
    const float alpha_r = *p.alpha_p;
    float ra[2 * IB];
#pragma unroll
    for (int i = 0; i < 2 * IB; ++i) ra[i] = p.row_alpha[min(m0 + WM * wr + 16 * i + l15, p.M - 1)];
#pragma unroll
    for (int i = 0; i < 2 * IB; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = (acc[i][j] * alpha_r) * ra[i];
    if (kind == 2) pp_epilogue<T, 2, false, true, true, STATS, BM>(p, acc, ct, m0, n0, tid, wr, wc, quad, l15);
    else pp_epilogue<T, 0, false, true, true, STATS, BM>(p, acc, ct, m0, n0, tid, wr, wc, quad, l15);
    return;
  }
  if (!DEV && p.slab) {   // split-K partial: raw accumulators into this split's [M][N] slab, the reduce kernel finishes
    GemmBf16Params ps = p;
    ps.C = p.slab + (size_t)blockIdx.y * p.M * p.N;
    ps.ldc = p.N;
    ps.epilogue = 0;
    ps.alpha = 1.f;
    ps.out_scale = 0.f;
    pp_epilogue<T, 0, false, false, false, false, BM>(ps, acc, ct, m0, n0, tid, wr, wc, quad, l15);
    return;
  }
  if constexpr (BM == 192) {   // fp32 outputs only (host check)
    if (kind == 0) pp_epilogue<T, 0, false, DEV, false, false, BM>(p, acc, ct, m0, n0, tid, wr, wc, quad, l15);
    else if (kind == 1) pp_epilogue<T, 1, false, DEV, false, false, BM>(p, acc, ct, m0, n0, tid, wr, wc, quad, l15);
    else if (kind == 2) pp_epilogue<T, 2, false, DEV, false, false, BM>(p, acc, ct, m0, n0, tid, wr, wc, quad, l15);
    else pp_epilogue<T, 3, false, DEV, false, false, BM>(p, acc, ct, m0, n0, tid, wr, wc, quad, l15);
  } else if (p.out_bf16) {
    unsigned short* ct16 = reinterpret_cast<unsigned short*>(lds_raw);
    if (kind == 0) pp_epilogue_b16<T, false, false, DEV>(p, acc, ct16, m0, n0, tid, wr, wc, quad, l15);
    else if (kind == 1 && p.aux) pp_epilogue_b16<T, true, true, DEV>(p, acc, ct16, m0, n0, tid, wr, wc, quad, l15);
    else if (kind == 1) pp_epilogue_b16<T, true, false, DEV>(p, acc, ct16, m0, n0, tid, wr, wc, quad, l15);
    else pp_epilogue<T, 2, true, DEV>(p, acc, ct, m0, n0, tid, wr, wc, quad, l15);          // RESIDUAL needs an fp32 output (host check)
  } else {
    if (kind == 0) pp_epilogue<T, 0, false, DEV>(p, acc, ct, m0, n0, tid, wr, wc, quad, l15);
    else if (kind == 1) pp_epilogue<T, 1, false, DEV>(p, acc, ct, m0, n0, tid, wr, wc, quad, l15);
    else if (kind == 2) pp_epilogue<T, 2, false, DEV>(p, acc, ct, m0, n0, tid, wr, wc, quad, l15);
    else pp_epilogue<T, 3, false, DEV>(p, acc, ct, m0, n0, tid, wr, wc, quad, l15);
  }
}
#undef PP_BARRIER

// ---------------------------------------------------------------------------------------------------------------
// PERSISTENT form of the ping-pong kernel (K-major operands, no split-K): one workgroup per CU walks its share of the
// tiles, and the next tile's first K-tiles are in flight while the finished tile is stored.  With one 128-KiB workgroup
// per CU nothing else runs on the CU between two K loops: the one-tile kernel pays, per tile, the dispatch of a new
// workgroup, its address set-up and the latency of its first DMA (5-8k cycles before the first MFMA) and an epilogue that
// takes ALL of the LDS (8.6k cycles for a bf16 tile, 36k for fp32 + residual, beside a 43k-cycle K loop at K = 768:
// profiles/r02_bf16_pingpong_stamps.log).  Here, at the end of a K loop:
//   1. the NEXT tile's K-tiles 0 and 1 are requested by LDS-DMA into the two staging buffers (free: everybody is past its
//      last LDS read) — the epilogue below does not touch them;
//   2. the finished tile goes out through a SPARE 32-KiB window (the CU has 160 KiB; the staging buffers take 128): 64 rows
//      (bf16) or 32 rows (fp32) per pass — the wave row that owns them writes its accumulator blocks (bias, quick-GELU and
//      the bf16 rounding applied in registers), barrier, all 512 threads copy whole 512-byte / 1-KiB rows out with 16-byte
//      stores, barrier.  The residual (and nothing else) is a side operand of the copy: its loads are requested one pass
//      ahead — in FRONT of that pass's stores, because vmcnt retires loads and stores in issue order and a load issued
//      behind stores returns only after they are acknowledged.
// A first form stored the tile straight from the accumulators (fire-and-forget, the residual as the accumulators' initial
// value): 8-byte / 16-byte pieces of 16 different rows per store instruction are four times (bf16) / twice (fp32) the
// write requests of whole rows, and the K loop that was meant to hide them ran slower beside them — measured slower on
// most shapes, dropped (profiles/r03_bf16_persistent_direct_store_ab.log).
// Stores go through a buffer descriptor over the tile's rows: a lane whose row or column chunk lies outside C gets an
// out-of-range offset and the hardware drops its write — every thread issues the SAME number of store instructions per
// tile, which the counted waits on the DMA pieces rely on.  Same phases, barriers and counted waits inside the K loop as
// gemm_bf16_pp_kernel<false>.  Tiles: XCD x (= blockIdx & 7, the hardware's round-robin) owns the same contiguous run of
// the grouped tile order as in the one-tile-per-workgroup kernels, its 32 workgroups stride through it.
#define PP_BARRIER()                      \
  do {                                    \
    __builtin_amdgcn_sched_barrier(0);    \
    __builtin_amdgcn_s_barrier();         \
    __builtin_amdgcn_sched_barrier(0);    \
  } while (0)

template <class T>
__global__ void __launch_bounds__(512) gemm_bf16_ppp_kernel(GemmBf16Params p) {
  typedef typename T::x8 V8;
  constexpr int BM = 256, BN = 256, ROW = BKH;
  constexpr int BUF = (BM + BN) * ROW;
  constexpr int WIN = 32768;                                                    // the epilogue's window
  __shared__ __attribute__((aligned(16))) unsigned char lds_raw[2 * BUF * 2 + WIN];   // 128 + 32 KiB: the ONLY LDS object
  __bf16* lds = reinterpret_cast<__bf16*>(lds_raw);
  unsigned char* win = lds_raw + 2 * BUF * 2;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wc = wave & 3;
  const int l15 = lane & 15, quad = lane >> 4;
  const int nk = p.K / BKH;
  const int kind = (p.epilogue & DCLIP_EPI_RESIDUAL) ? 3 : (p.epilogue & DCLIP_EPI_GELU) ? 1 : 0;
  const bool out16 = p.out_bf16 != 0;

  // this workgroup's tiles: ids first, first + stride, ... < last in the grouped order (see xcd_remap16)
  constexpr int GROUP_M = 8;
  const int nwg = p.tiles_m * p.tiles_n;
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, per_xcd = gridDim.x >> 3;     // gridDim.x is a multiple of 8
  const int q8 = nwg >> 3, r8 = nwg & 7;
  const int xbase = (xcd < r8) ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8;
  const int xcount = q8 + (xcd < r8 ? 1 : 0);
  const int per_group = GROUP_M * p.tiles_n;

  const int sw = l15 >> 1;
  const __bf16* pa0 = lds + (128 * wr + l15) * ROW + (((0 + quad) ^ sw) << 3);
  const __bf16* pa1 = lds + (128 * wr + l15) * ROW + (((4 + quad) ^ sw) << 3);
  const __bf16* pb0 = lds + (BM + 64 * wc + l15) * ROW + (((0 + quad) ^ sw) << 3);
  const __bf16* pb1 = lds + (BM + 64 * wc + l15) * ROW + (((4 + quad) ^ sw) << 3);

  f32x4 acc[8][4];
  V8 fa[4][2], fb0[2][2], fb1[2][2];
  // the tile whose results sit in the accumulators (stored at the top of the next iteration)
  int pm0 = 0, pn0 = 0;
  bool pending = false;

#define PPP_ISSUE_A(h, buf, kt)                                                                                  \
  do {                                                                                                           \
    dma16(a_rsrc, lds + (buf) * BUF + (64 * (h) + 8 * wave) * ROW, a_voff[h][0], (kt) * (BKH * 2));              \
    dma16(a_rsrc, lds + (buf) * BUF + (128 + 64 * (h) + 8 * wave) * ROW, a_voff[h][1], (kt) * (BKH * 2));        \
  } while (0)
#define PPP_ISSUE_B(h, buf, kt)                                                                                  \
  do {                                                                                                           \
    dma16(w_rsrc, lds + (buf) * BUF + (BM + 64 * (wave >> 2) + 32 * (h) + 8 * (wave & 3)) * ROW, w_voff[h][0],   \
          (kt) * (BKH * 2));                                                                                     \
    dma16(w_rsrc, lds + (buf) * BUF + (BM + 128 + 64 * (wave >> 2) + 32 * (h) + 8 * (wave & 3)) * ROW,           \
          w_voff[h][1], (kt) * (BKH * 2));                                                                       \
  } while (0)
#define PPP_READ_A(qm, off)                                                                         \
  _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                   \
    fa[i][0] = *reinterpret_cast<const V8*>(pa0 + (off) + (64 * (qm) + 16 * i) * ROW);          \
    fa[i][1] = *reinterpret_cast<const V8*>(pa1 + (off) + (64 * (qm) + 16 * i) * ROW);          \
  }
#define PPP_READ_B(fb, qn, off)                                                                     \
  _Pragma("unroll") for (int j = 0; j < 2; ++j) {                                                   \
    fb[j][0] = *reinterpret_cast<const V8*>(pb0 + (off) + (32 * (qn) + 16 * j) * ROW);          \
    fb[j][1] = *reinterpret_cast<const V8*>(pb1 + (off) + (32 * (qn) + 16 * j) * ROW);          \
  }
#define PPP_MFMA(qm, qn, fb)                                                                                        \
  do {                                                                                                              \
    __builtin_amdgcn_s_setprio(1);                                                                                  \
    _Pragma("unroll") for (int s = 0; s < 2; ++s)                                                                   \
    _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                                   \
    _Pragma("unroll") for (int j = 0; j < 2; ++j)                                                                   \
      acc[4 * (qm) + i][2 * (qn) + j] =                                                                             \
          T::mfma16(fb[j][s], fa[i][s], acc[4 * (qm) + i][2 * (qn) + j]);    \
    __builtin_amdgcn_s_setprio(0);                                                                                  \
  } while (0)

  // The finished tile (pm0, pn0) out of the accumulators through the window.  Block (i, j) of this wave = rows
  // 128 wr + 16 i + l15, columns 64 wc + 16 j + 4 quad .. +3 of the tile.
  auto store_tile = [&](const f32x4 (&bias4)[4]) __attribute__((always_inline)) {
    const int rows_left = p.M - pm0;                                   // >= 1
    const int trows = min(rows_left, BM);
    const size_t org = (size_t)pm0 * p.ldc;
    const __amdgpu_buffer_rsrc_t c_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        out16 ? (void*)(reinterpret_cast<unsigned short*>(p.C) + org) : (void*)(reinterpret_cast<float*>(p.C) + org), 0,
        (int)(((size_t)(trows - 1) * p.ldc + p.N) * (out16 ? 2 : 4)), 0x00020000);
    if (out16) {
      // ---- bf16 C: 4 passes of 64 rows x 512 bytes.  8-byte unit u of row r sits at u ^ (r & 15) (see pp_epilogue_b16).
      const __amdgpu_buffer_rsrc_t x_rsrc = __builtin_amdgcn_make_buffer_rsrc(
          (void*)(p.aux ? p.aux + org : reinterpret_cast<unsigned short*>(p.C)), 0,
          (int)(((size_t)(trows - 1) * p.ldc + p.N) * 2), 0x00020000);
      const bool save = kind == 1 && p.aux;
      unsigned short* w16 = reinterpret_cast<unsigned short*>(win);
      const int cg = tid & 31, col = pn0 + 8 * cg;                     // copy: 8 columns = one 16-byte store per thread and row
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (wr == (q >> 1)) {
#pragma unroll
          for (int ii = 0; ii < 4; ++ii)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              f32x4 v = acc[4 * (q & 1) + ii][j] * p.alpha + bias4[j];
              if (kind == 1 && !save) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = quick_gelu_f(v[e]);
              }
              const u16x4 h = {T::bits(v[0]), T::bits(v[1]), T::bits(v[2]), T::bits(v[3])};
              const int row = 16 * ii + l15, unit = 16 * wc + 4 * j + quad;
              *reinterpret_cast<u16x4*>(w16 + row * BN + ((unit ^ (row & 15)) << 2)) = h;
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        PP_BARRIER();
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
          const int lr = (tid >> 5) + 16 * s4, trow = 64 * q + lr;       // row inside the pass / inside the tile
          const u16x4 lo = *reinterpret_cast<const u16x4*>(w16 + lr * BN + (((2 * cg) ^ (lr & 15)) << 2));
          const u16x4 hi = *reinterpret_cast<const u16x4*>(w16 + lr * BN + (((2 * cg + 1) ^ (lr & 15)) << 2));
          typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
          u16x8 o = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
          const int el = col < p.N ? trow * p.ldc + col : 0x3fffffff;   // N % 8 == 0 (host check): a chunk is in or out as a whole
          if (save) {
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), x_rsrc, el * 2, 0, 0);
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = T::bits(quick_gelu_f(T::to_f32(o[e])));
          }
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), c_rsrc, el * 2, 0, 0);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this pass's LDS reads are done before the next pass overwrites them
        PP_BARRIER();
      }
    } else {
      // ---- fp32 C (+ residual): 8 passes of 32 rows x 1 KiB.  16-byte granule g of row r sits at g ^ (r & 7) (see pp_epilogue).
      float* w32 = reinterpret_cast<float*>(win);
      const int gcol = tid & 63, col = pn0 + 4 * gcol, lr0 = tid >> 6;   // copy: one column group, rows lr0 + 8 k of the pass
      const bool colok = col < p.N;
      const int colc = colok ? col : 0;
      f32x4 side[2][4];                                                 // residual rows of passes q and q + 1
      auto fetch_side = [&](int q, f32x4 (&dst)[4]) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          dst[k] = *reinterpret_cast<const f32x4*>(p.residual + (size_t)min(pm0 + 32 * q + lr0 + 8 * k, p.M - 1) * p.ldc + colc);
      };
      if (kind == 3) fetch_side(0, side[0]);
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        if (kind == 3 && q + 1 < 8) fetch_side(q + 1, side[(q + 1) & 1]);
        if (wr == (q >> 2)) {
#pragma unroll
          for (int ii = 0; ii < 2; ++ii)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const f32x4 v = acc[2 * (q & 3) + ii][j] * p.alpha + bias4[j];
              *reinterpret_cast<f32x4*>(w32 + (16 * ii + l15) * BN + (((16 * wc + 4 * j + quad) ^ (l15 & 7)) << 2)) = v;
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        PP_BARRIER();
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int lr = lr0 + 8 * k, trow = 32 * q + lr;
          f32x4 v = *reinterpret_cast<const f32x4*>(w32 + lr * BN + ((gcol ^ (lr & 7)) << 2));
          if (kind == 3) v += side[q & 1][k];
          const int el = colok ? trow * p.ldc + col : 0x1fffffff;
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), c_rsrc, el * 4, 0, 0);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        PP_BARRIER();
      }
    }
  };

  for (int t = slot; t < xcount; t += per_xcd) {
    const int swz = xbase + t;
    const int first_m = (swz / per_group) * GROUP_M;
    const int gsize = min(GROUP_M, p.tiles_m - first_m);
    const int tile_m = first_m + (swz % per_group) % gsize, tile_n = (swz % per_group) / gsize;
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    const __bf16* a_org = p.A + (size_t)m0 * p.lda;
    const __bf16* w_org = p.W + (size_t)n0 * p.ldw;
    const int a_rows = min(BM, p.M - m0), w_rows = min(BN, p.N - n0);
    const size_t a_bytes = ((size_t)(a_rows - 1) * p.lda + p.K) * 2, w_bytes = ((size_t)(w_rows - 1) * p.ldw + p.K) * 2;
    const __amdgpu_buffer_rsrc_t a_rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16*>(a_org), 0, (int)min(a_bytes, (size_t)0x7fffffff), 0x00020000);
    const __amdgpu_buffer_rsrc_t w_rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16*>(w_org), 0, (int)min(w_bytes, (size_t)0x7fffffff), 0x00020000);
    int a_voff[2][2], w_voff[2][2];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int x = 0; x < 2; ++x) {
        const int ra = 128 * x + 64 * h + 8 * wave + (lane >> 3), ga = (lane & 7) ^ ((ra >> 1) & 7);
        a_voff[h][x] = ra < a_rows ? (ra * p.lda + ga * 8) * 2 : 0x7fffffff;   // out of range -> zeros in LDS
        const int rb = 64 * (2 * x + (wave >> 2)) + 32 * h + 8 * (wave & 3) + (lane >> 3), gb = (lane & 7) ^ ((rb >> 1) & 7);
        w_voff[h][x] = rb < w_rows ? (rb * p.ldw + gb * 8) * 2 : 0x7fffffff;
      }

    // ---- tile boundary.  Issue order (vmcnt retires loads and stores in THIS order, so a wait names what may still fly):
    //   [bias of the finished tile: 4 loads]  [K-tile 0: 8 DMA pieces]  [K-tile 1: 8 pieces, if any]
    //   [the finished tile's residual loads and stores, interleaved: NOPS instructions per thread, 0 on a first tile]
    // The staging buffers are free: everybody is past the previous tile's last LDS read (the K loop's closing barrier).
    f32x4 bias4[4];
    if (pending) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int col = pn0 + 64 * wc + 4 * quad + 16 * j;
        bias4[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (p.epilogue & DCLIP_EPI_BIAS) bias4[j] = *reinterpret_cast<const f32x4*>(p.bias + (col < p.N ? col : 0));
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    PPP_ISSUE_A(0, 0, 0);
    PPP_ISSUE_B(0, 0, 0);
    PPP_ISSUE_B(1, 0, 0);
    PPP_ISSUE_A(1, 0, 0);
    if (nk > 1) {
      PPP_ISSUE_B(0, 1, 1);
      PPP_ISSUE_A(0, 1, 1);
      PPP_ISSUE_B(1, 1, 1);
      PPP_ISSUE_A(1, 1, 1);
    }
    __builtin_amdgcn_sched_barrier(0);
    // vector-memory instructions one thread issues in store_tile (uniform): bf16 16 stores (+ 16 for a saved pre-activation),
    // fp32 32 stores (+ 32 residual loads)
    const int nops = !pending ? 0 : (out16 ? ((kind == 1 && p.aux) ? 32 : 16) : (kind == 3 ? 64 : 32));
    if (pending) store_tile(bias4);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // K-tile 0 has landed; what was issued after it — K-tile 1's 8 pieces and the nops above — may still be in flight
    if (nk == 1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else if (nops == 0) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if (nops == 16) asm volatile("s_waitcnt vmcnt(24)" ::: "memory");
    else if (nops == 32) asm volatile("s_waitcnt vmcnt(40)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(63)" ::: "memory");                    // 8 + 64 issued after it, 63 allowed: K-tile 0 retired
    PP_BARRIER();
    if (wr == 1) PP_BARRIER();   // wave row 1 runs one barrier behind wave row 0

    for (int kt = 0; kt < nk; ++kt) {
      const int cur = kt & 1, off = cur * BUF;
      const bool n1 = kt + 1 < nk, n2 = kt + 2 < nk;
      // ---- phase 1
      PPP_READ_B(fb0, 0, off);
      __builtin_amdgcn_sched_barrier(0);
      PPP_READ_A(0, off);
      __builtin_amdgcn_sched_barrier(0);
      if (n1 && kt > 0) PPP_ISSUE_A(1, cur ^ 1, kt + 1);   // (K-tile 1's A-half 1 went out at the tile boundary)
      asm volatile("s_waitcnt lgkmcnt(8)" ::: "memory");
      PP_BARRIER();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      PPP_MFMA(0, 0, fb0);
      PP_BARRIER();
      // ---- phase 2
      PPP_READ_B(fb1, 1, off);
      __builtin_amdgcn_sched_barrier(0);
      if (n2) PPP_ISSUE_B(0, cur, kt + 2);
      PP_BARRIER();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      PPP_MFMA(0, 1, fb1);
      PP_BARRIER();
      // ---- phase 3
      PPP_READ_A(1, off);
      __builtin_amdgcn_sched_barrier(0);
      if (n2) PPP_ISSUE_A(0, cur, kt + 2);
      PP_BARRIER();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      PPP_MFMA(1, 1, fb1);
      PP_BARRIER();
      // ---- phase 4: K-tile kt+1 has landed (this wave's pieces); the three halves of kt+2 just issued stay in flight —
      // and, in a tile's first iteration, the previous tile's stores, which sit between them in issue order
      if (n2) {
        PPP_ISSUE_B(1, cur, kt + 2);
        if (kt > 0 || nops == 0) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
        else if (nops == 16) asm volatile("s_waitcnt vmcnt(22)" ::: "memory");
        else if (nops == 32) asm volatile("s_waitcnt vmcnt(38)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(63)" ::: "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      PP_BARRIER();
      PPP_MFMA(1, 0, fb0);
      PP_BARRIER();
    }
    if (wr == 0) PP_BARRIER();   // balance the stagger: everybody is past its last MFMA phase and LDS read
    pm0 = m0;
    pn0 = n0;
    pending = true;
  }
  if (pending) {
    f32x4 bias4[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = pn0 + 64 * wc + 4 * quad + 16 * j;
      bias4[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (p.epilogue & DCLIP_EPI_BIAS) bias4[j] = *reinterpret_cast<const f32x4*>(p.bias + (col < p.N ? col : 0));
    }
    store_tile(bias4);
  }
#undef PPP_ISSUE_A
#undef PPP_ISSUE_B
#undef PPP_READ_A
#undef PPP_READ_B
#undef PPP_MFMA
}
#undef PP_BARRIER

// persistent form: K-major operands, whole K, epilogue kinds bias / GELU (+ saved pre-activation) / residual
// OPT-IN (DCLIP_BF16_PERSIST=1): measured slower than the one-tile kernel on 15 of 17 tower / student shapes in both forms
// (profiles/r03_bf16_persistent_*_ab.log) — kept as an A/B switch with its parity test, not the default.  Read per call, not
// cached: tests and A/B runs switch it inside one process.
bool persistent_enabled() { return getenv("DCLIP_BF16_PERSIST") && atoi(getenv("DCLIP_BF16_PERSIST")) != 0; }

template <class T>
int launch_ppp(GemmBf16Params p, hipStream_t st) {
  p.tiles_m = cdiv(p.M, 256);
  p.tiles_n = cdiv(p.N, 256);
  const int tiles = p.tiles_m * p.tiles_n;
  int grid = tiles < 256 ? ((tiles + 7) / 8) * 8 : 256;      // a multiple of 8: 32 (or fewer) workgroups per XCD
  hipLaunchKernelGGL(gemm_bf16_ppp_kernel<T>, dim3(grid), dim3(512), 0, st, p);
  return DCLIP_OK;
}

template <class T, bool TOK = false>
int launch_pp(GemmBf16Params p, hipStream_t st, int splits = 1) {
  p.tiles_m = cdiv(p.M, 256);
  p.tiles_n = cdiv(p.N, 256);
  if constexpr (std::is_same<T, F16T>::value && !TOK) {   // the device-scaled entries exist for F16T only
    if (p.row_alpha && p.pmax) {
      hipLaunchKernelGGL((gemm_bf16_pp_kernel<T, false, true, true, false, true>), dim3(p.tiles_m * p.tiles_n, splits), dim3(512), 0,
                         st, p);
      return DCLIP_OK;
    }
    if (p.row_alpha) {
      hipLaunchKernelGGL((gemm_bf16_pp_kernel<T, false, true, true>), dim3(p.tiles_m * p.tiles_n, splits), dim3(512), 0, st, p);
      return DCLIP_OK;
    }
    if (p.alpha_p) {
      hipLaunchKernelGGL((gemm_bf16_pp_kernel<T, false, true>), dim3(p.tiles_m * p.tiles_n, splits), dim3(512), 0, st, p);
      return DCLIP_OK;
    }
  }
  hipLaunchKernelGGL((gemm_bf16_pp_kernel<T, TOK>), dim3(p.tiles_m * p.tiles_n, splits), dim3(512), 0, st, p);
  return DCLIP_OK;
}

// y[i] = bf16(x[i]); rows of `cols` floats written with leading dimension ldy (>= cols, zero padded)
template <class T>
__global__ void __launch_bounds__(256) cast_bf16_kernel(const float* __restrict__ x, unsigned short* __restrict__ y, int rows,
                                                        int cols, int ldx, int ldy) {
  const int ld4 = ldy >> 2;
  const size_t total = (size_t)rows * ld4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % ld4) * 4;
    const size_t r = i / ld4;
    u16x4 o = {0, 0, 0, 0};
    if (c + 3 < cols) {
      f32x4 v = *reinterpret_cast<const f32x4*>(x + r * ldx + c);
      o = u16x4{T::bits(v[0]), T::bits(v[1]), T::bits(v[2]), T::bits(v[3])};
    } else {
      for (int e = 0; e < 4; ++e)
        if (c + e < cols) o[e] = T::bits(x[r * ldx + c + e]);
    }
    *reinterpret_cast<u16x4*>(y + r * ldy + c) = o;
  }
}

// LayerNorm with bf16 output (fp32 statistics and affine): one wave per row
template <class T, int NC, bool EXACT>   // EXACT: D == 256 NC, no per-chunk bounds tests; loads hoisted into one group (see layernorm.hip)
__global__ void __launch_bounds__(256) ln_fwd_bf16_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, unsigned short* __restrict__ y,
                                                          int rows, int D, float eps, float* __restrict__ mean_out,
                                                          float* __restrict__ rstd_out) {
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
  if (mean_out && lane == 0) {
    mean_out[row] = mu;
    rstd_out[row] = rs;
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int i = lane + 64 * c;
    if (EXACT || i < d4) {
      f32x4 o = (v[c] - mu) * rs * g[c] + bt[c];
      u16x4 b = {T::bits(o[0]), T::bits(o[1]), T::bits(o[2]), T::bits(o[3])};
      *reinterpret_cast<u16x4*>(y + (size_t)row * D + i * 4) = b;
    }
  }
}

// C[M][ldc] = sum over splits of slab[s][M][N], in fixed order (deterministic); one float4 per thread
__global__ void __launch_bounds__(256) splitk_reduce_bf16_kernel(const float* __restrict__ slab, float* __restrict__ C, int M,
                                                                 int N, int ldc, int splits) {
  const size_t total4 = (size_t)M * N / 4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (size_t)gridDim.x * blockDim.x) {
    f32x4 s = *reinterpret_cast<const f32x4*>(slab + i * 4);
    for (int z = 1; z < splits; ++z) s += *reinterpret_cast<const f32x4*>(slab + (size_t)z * M * N + i * 4);
    const size_t row = (i * 4) / N, col = (i * 4) % N;
    *reinterpret_cast<f32x4*>(C + row * ldc + col) = s;
  }
}

// splitk_reduce_bf16_kernel for the segmented weight gradient: C[m][:] = ((sum of slabs) (1 / *act_scale)) *
// row_scale[m].  The scalar first, as in the row-scaled dgrads: the reciprocal of a power of two is exact, and sums of 2^41
// times an activation scale's reciprocal stay far inside fp32 before a row scale of 2^+-100 meets them.
__global__ void __launch_bounds__(256) splitk_reduce_scaled_bf16_kernel(const float* __restrict__ slab, float* __restrict__ C, int M,
                                                                        int N, int ldc, int splits,
                                                                        const float* __restrict__ row_scale,
                                                                        const float* __restrict__ act_scale) {
  const float inv = 1.f / *act_scale;
  const size_t total4 = (size_t)M * N / 4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (size_t)gridDim.x * blockDim.x) {
    f32x4 s = *reinterpret_cast<const f32x4*>(slab + i * 4);
    for (int z = 1; z < splits; ++z) s += *reinterpret_cast<const f32x4*>(slab + (size_t)z * M * N + i * 4);
    const size_t row = (i * 4) / N, col = (i * 4) % N;
    *reinterpret_cast<f32x4*>(C + row * ldc + col) = (s * inv) * row_scale[row];
  }
}

inline int grid_for(size_t work) {
  size_t b = (work + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

}  // namespace

#ifdef DCLIP_GEMM_STAMPS
// [workgroups][16] uint64 on the device, or nullptr to stop stamping (diagnostic library only)
DCLIP_API int dclip_debug_set_bf16_stamps(void* buf) {
  return hipMemcpyToSymbol(HIP_SYMBOL(g_stamps16), &buf, sizeof(buf)) == hipSuccess ? DCLIP_OK : DCLIP_ELAUNCH;
}
#endif

DCLIP_API int dclip_gemm_bf16(const void* A, const void* W, void* C, const float* bias, const float* residual, int M, int N,
                              int K, int lda, int ldw, int ldc, int epilogue, int out_bf16, void* stream) {
  return dclip_gemm_bf16_ex(A, W, C, bias, residual, nullptr, M, N, K, lda, ldw, ldc, epilogue, out_bf16, stream);
}

namespace {
// the device-memory operands of the device-scaled entries (GemmBf16Params' last four members)
struct DevScales {
  const float* alpha_p;
  const float* out_scale_p;
  float* h32;
  float* g32;
  const float* row_alpha = nullptr;   // dclip_gemm_f16_scaled_rows_dev
  const float* aux32 = nullptr;
  unsigned* pmax = nullptr;           // dclip_gemm_f16_scaled_rows_stats_dev
  float* psum = nullptr;
};
inline void set_dev(GemmBf16Params& p, const DevScales* d) {
  if (d) p.alpha_p = d->alpha_p, p.out_scale_p = d->out_scale_p, p.h32 = d->h32, p.g32 = d->g32, p.row_alpha = d->row_alpha,
         p.aux32 = d->aux32, p.pmax = d->pmax, p.psum = d->psum;
}

// the dispatcher's test for the ping-pong kernel (gemm16 below)
inline int pp_big_min() { return getenv("DCLIP_BF16_BIG_MIN") ? atoi(getenv("DCLIP_BF16_BIG_MIN")) : 128; }
inline bool takes_pp(int M, int N, int K) { return K % BKH == 0 && (long)cdiv(M, 256) * cdiv(N, 256) >= pp_big_min(); }

// fp16 of the training path (F16IeeeT): the ping-pong and register-staged kernels only (no persistent instance)
template <class T>
constexpr bool kTrain16 = std::is_same<T, F16IeeeT>::value;

// The forward dispatcher of every 16-bit type: same checks, same plan.  Each kernel it can pick — ping-pong 256x256,
// register-staged 128x128 / 64x64 — has an instance per type; the persistent form (DCLIP_BF16_PERSIST) for bf16 and the
// saturating fp16.
template <class T>
int gemm16(const char* name, const void* A, const void* W, void* C, const float* bias, const float* residual, void* aux, int M,
           int N, int K, int lda, int ldw, int ldc, int epilogue, int out_bf16, void* stream, float alpha = 1.f, float out_scale = 0.f,
           const DevScales* dev = nullptr) {
  DCLIP_REQUIRE(A && W && C, "%s: null operand", name);
  DCLIP_REQUIRE(M > 0 && N > 0 && K > 0, "%s: bad shape M=%d N=%d K=%d", name, M, N, K);
  DCLIP_REQUIRE(lda % 8 == 0 && ldw % 8 == 0 && lda >= K && ldw >= K, "%s: lda/ldw must be multiples of 8 and >= K", name);
  // a tile's operand loads are buffer loads with an int byte offset (tile row * ld + k) * 2 from the tile's origin and a
  // descriptor of at most 2^31 - 1 bytes: up to 256 rows of a tile must fit
  DCLIP_REQUIRE(256L * lda * 2 < 0x7fffffffL && 256L * ldw * 2 < 0x7fffffffL, "%s: leading dimension too large", name);
  DCLIP_REQUIRE(N % 4 == 0 && ldc % 4 == 0 && ldc >= N, "%s: N / ldc must be multiples of 4", name);
  DCLIP_REQUIRE(((uintptr_t)A | (uintptr_t)W | (uintptr_t)C) % 16 == 0, "%s: operands must be 16-byte aligned", name);
  DCLIP_REQUIRE(!(epilogue & ~(DCLIP_EPI_BIAS | DCLIP_EPI_GELU | DCLIP_EPI_DGELU | DCLIP_EPI_RESIDUAL)),
                "%s: unsupported epilogue bits", name);
  DCLIP_REQUIRE(out_scale == 0.f || (!out_bf16 && !aux && !(epilogue & (DCLIP_EPI_RESIDUAL | DCLIP_EPI_DGELU)) && (long)ldc >= 3L * N),
                "%s: a split output takes BIAS | GELU only and ldc >= 3 N", name);
  DCLIP_REQUIRE(!(epilogue & DCLIP_EPI_DGELU) || ((aux || (dev && dev->aux32)) && !(epilogue & DCLIP_EPI_GELU)),
                "%s: DGELU needs aux (and no GELU)", name);
  DCLIP_REQUIRE(!aux || (uintptr_t)aux % 8 == 0, "%s: aux must be 8-byte aligned", name);
  DCLIP_REQUIRE(!(epilogue & DCLIP_EPI_BIAS) || bias, "%s: BIAS without bias", name);
  DCLIP_REQUIRE(!(epilogue & DCLIP_EPI_RESIDUAL) || (residual && !out_bf16), "%s: RESIDUAL needs an fp32 output", name);
  hipStream_t st = (hipStream_t)stream;
  // Ping-pong kernel (K % 64 == 0, at least 128 workgroups): measured faster than the register-staged 128x128 kernel on
  // every tower shape, short K included (tools/bf16_gemm_bench.py).  With fp32 outputs and K = 768 it is bound by writing C
  // (944 MB for the qkv projection of 2048 crops): one workgroup per CU cannot overlap that with the next tile's MFMAs.
  if (takes_pp(M, N, K)) {   // (DCLIP_BF16_BIG_MIN, default 128: a tuning aid, read per call)
    GemmBf16Params pb{(const __bf16*)A, (const __bf16*)W, C, bias, residual, M, N, K, lda, ldw, ldc, epilogue, out_bf16, 0, 0,
                      (unsigned short*)aux, 0, nullptr, alpha, out_scale};
    set_dev(pb, dev);
    // persistent form when a CU gets several tiles (the towers' M = 100k shapes: 14 per CU): the epilogue of one tile
    // overlaps the K loop of the next.  DGELU (an extra side operand in the epilogue) stays on the one-tile kernel, and so does
    // GELU with an fp32 C: the persistent kernel's fp32 store path applies bias and residual only (it returned the
    // pre-activation and left aux unwritten: tests/test_gemm16_paths_gpu.py).
    if constexpr (!kTrain16<T>) {
      const int persist_min = getenv("DCLIP_BF16_PERSIST_MIN") ? atoi(getenv("DCLIP_BF16_PERSIST_MIN")) : 512;
      const bool gelu_f32 = (epilogue & DCLIP_EPI_GELU) && !out_bf16;
      // (its C tile is stored through a buffer descriptor with int element offsets: 256 rows of ldc floats stay below 2^31
      // bytes, or the one-tile kernel, which addresses C with size_t, takes the call)
      if (persistent_enabled() && !(epilogue & DCLIP_EPI_DGELU) && !gelu_f32 && out_scale == 0.f && !dev && ldc % 8 == 0 &&
          256L * ldc * 4 < 0x7fffffffL && N % 8 == 0 && (long)cdiv(M, 256) * cdiv(N, 256) >= persist_min) {
        launch_ppp<T>(pb, st);
        DCLIP_CHECK_LAUNCH_V(name, ".ppp");
        return DCLIP_OK;
      }
    }
    launch_pp<T>(pb, st);
    DCLIP_CHECK_LAUNCH_V(name, ".pp");
    return DCLIP_OK;
  }
  const bool small = (long)cdiv(M, 128) * cdiv(N, 128) < 256;  // fewer tiles than CUs: use the finer tile
  const int bm = small ? 64 : 128, bn = bm;
  GemmBf16Params p{(const __bf16*)A, (const __bf16*)W, C, bias, residual, M, N, K, lda, ldw, ldc, epilogue, out_bf16,
                   cdiv(M, bm), cdiv(N, bn), (unsigned short*)aux, 0, nullptr, alpha, out_scale};
  set_dev(p, dev);
  const size_t lds = (size_t)2 * (bm + bn) * BKH * 2;
  if (small) launch_reg<T, 64>(p, lds, st);
  else launch_reg<T, 128>(p, lds, st);
  DCLIP_CHECK_LAUNCH_V(name, small ? ".r64" : ".r128");
  return DCLIP_OK;
}
}  // namespace

DCLIP_API int dclip_gemm_bf16_ex(const void* A, const void* W, void* C, const float* bias, const float* residual, void* aux,
                                 int M, int N, int K, int lda, int ldw, int ldc, int epilogue, int out_bf16, void* stream) {
  return gemm16<Bf16T>("gemm_bf16", A, W, C, bias, residual, aux, M, N, K, lda, ldw, ldc, epilogue, out_bf16, stream);
}

// fp16 forward of the frozen towers: dclip_gemm_bf16's arguments and limits, fp16 A / W / 16-bit C (rounding: common.h, F16T).
// No saved pre-activation or DGELU (training-only epilogues): aux is not an argument.
DCLIP_API int dclip_gemm_f16(const void* A, const void* W, void* C, const float* bias, const float* residual, int M, int N, int K,
                             int lda, int ldw, int ldc, int epilogue, int out_f16, void* stream) {
  DCLIP_REQUIRE(!(epilogue & DCLIP_EPI_DGELU), "gemm_f16: DGELU is a training epilogue (bf16 only)");
  return gemm16<F16T>("gemm_f16", A, W, C, bias, residual, nullptr, M, N, K, lda, ldw, ldc, epilogue, out_f16, stream);
}

// dclip_gemm_f16 with `alpha`: C = epilogue(alpha * (A W^T)) — the accumulator is scaled BEFORE bias, GELU and residual.  The
// split-fp16 text tower (split16.hip) feeds operands scaled by powers of two and undoes both scales here;
// alpha = 1 gives dclip_gemm_f16's output bit for bit.
DCLIP_API int dclip_gemm_f16_scaled(const void* A, const void* W, void* C, const float* bias, const float* residual, int M, int N,
                                    int K, int lda, int ldw, int ldc, int epilogue, int out_f16, float alpha, void* stream) {
  DCLIP_REQUIRE(!(epilogue & DCLIP_EPI_DGELU), "gemm_f16_scaled: DGELU is a training epilogue");
  DCLIP_REQUIRE(alpha == alpha && alpha - alpha == 0.f, "gemm_f16_scaled: alpha must be finite");
  return gemm16<F16T>("gemm_f16_scaled", A, W, C, bias, residual, nullptr, M, N, K, lda, ldw, ldc, epilogue, out_f16, stream, alpha);
}

// dclip_gemm_f16_scaled whose result leaves as the operand of the NEXT split GEMM: C is fp16 [M][ldc >= 3 N], the [hi|lo|hi]
// split (split16.hip) of out_scale * epilogue(alpha * (A W^T)), epilogue BIAS | GELU — fc1 + quick-GELU of the split-fp16 text
// tower without the fp32 round trip through memory.  Bit-equal to dclip_split_f32_f16x3 of dclip_gemm_f16_scaled's fp32 output.
DCLIP_API int dclip_gemm_f16_scaled_split(const void* A, const void* W, void* C, const float* bias, int M, int N, int K, int lda,
                                          int ldw, int ldc, int epilogue, float alpha, float out_scale, void* stream) {
  DCLIP_REQUIRE(alpha == alpha && alpha - alpha == 0.f, "gemm_f16_scaled_split: alpha must be finite");
  DCLIP_REQUIRE(out_scale > 0.f && out_scale - out_scale == 0.f && (__builtin_bit_cast(unsigned int, out_scale) & 0x007fffffu) == 0,
                "gemm_f16_scaled_split: out_scale must be a power of two");
  DCLIP_REQUIRE(ldc % 8 == 0, "gemm_f16_scaled_split: ldc must be a multiple of 8");
  return gemm16<F16T>("gemm_f16_scaled_split", A, W, C, bias, nullptr, nullptr, M, N, K, lda, ldw, ldc, epilogue, 0, stream, alpha,
                      out_scale);
}

// The two entries above with their scales in DEVICE memory (split16.hip's plan record): the weights of a training
// tower change every step, so alpha / out_scale are recomputed on the device and read through pointers — no host value to go
// stale in a captured graph.  Same kernels and arithmetic: at equal scales every output equals the scalar entry's bit for bit
// (the persistent kernel is not used).  _split_dev may also write the fp32 result g [M][N] and, with GELU, the fp32
// pre-activation h [M][N] (what a training forward saves), each bit-equal to dclip_gemm_f16_scaled's output for that epilogue.
DCLIP_API int dclip_gemm_f16_scaled_dev(const void* A, const void* W, void* C, const float* bias, const float* residual, int M,
                                        int N, int K, int lda, int ldw, int ldc, int epilogue, int out_f16, const float* alpha,
                                        void* stream) {
  DCLIP_REQUIRE(!(epilogue & DCLIP_EPI_DGELU), "gemm_f16_scaled_dev: DGELU is a training epilogue");
  DCLIP_REQUIRE(alpha && (uintptr_t)alpha % 4 == 0, "gemm_f16_scaled_dev: alpha must be a device pointer");
  const DevScales dev{alpha, nullptr, nullptr, nullptr};
  return gemm16<F16T>("gemm_f16_scaled_dev", A, W, C, bias, residual, nullptr, M, N, K, lda, ldw, ldc, epilogue, out_f16, stream, 1.f,
                      0.f, &dev);
}

DCLIP_API int dclip_gemm_f16_scaled_split_dev(const void* A, const void* W, void* C, const float* bias, float* h32, float* g32, int M,
                                              int N, int K, int lda, int ldw, int ldc, int epilogue, const float* alpha,
                                              const float* out_scale, void* stream) {
  DCLIP_REQUIRE(alpha && ((uintptr_t)alpha | (uintptr_t)out_scale) % 4 == 0,
                "gemm_f16_scaled_split_dev: alpha / out_scale must be device pointers");
  DCLIP_REQUIRE(ldc % 8 == 0, "gemm_f16_scaled_split_dev: ldc must be a multiple of 8");
  DCLIP_REQUIRE(((uintptr_t)h32 | (uintptr_t)g32) % 16 == 0, "gemm_f16_scaled_split_dev: h32 / g32 must be 16-byte aligned");
  DCLIP_REQUIRE(!h32 || (epilogue & DCLIP_EPI_GELU), "gemm_f16_scaled_split_dev: h32 is the pre-activation of a GELU epilogue");
  DCLIP_REQUIRE(!(epilogue & ~(DCLIP_EPI_BIAS | DCLIP_EPI_GELU)), "gemm_f16_scaled_split_dev: the epilogue is BIAS | GELU");
  // out_scale NULL: no split — C is the fp32 result [M][ldc] itself (the two-launch form: the stand-alone split pass follows)
  DCLIP_REQUIRE(out_scale || !g32, "gemm_f16_scaled_split_dev: without out_scale C is the fp32 result (g32 must be NULL)");
  const DevScales dev{alpha, out_scale, h32, g32};
  return gemm16<F16T>("gemm_f16_scaled_split_dev", A, W, C, bias, nullptr, nullptr, M, N, K, lda, ldw, ldc, epilogue, 0, stream, 1.f,
                      out_scale ? 1.f : 0.f, &dev);
}

// dclip_gemm_f16_scaled_dev for the data-gradient GEMMs of the split-fp16 backward: A is the [hi|lo|hi] split of
// dY with ONE power-of-two scale PER ROW (dclip_split_f32_f16x3_rows), so the accumulator of row m is scaled back by
// row_alpha[m] as well:  C[m][n] = epi((acc * *alpha) * row_alpha[m]),  fp32.  epilogue 0, or DCLIP_EPI_DGELU with the fp32
// pre-activation aux32 [M][ldc] (gemm_f32's statement: at equal accumulators the outputs are bit-equal).  With row_alpha == 1
// everywhere the output is dclip_gemm_f16_scaled_dev's bit for bit.  Every kernel of the dispatcher except the persistent one.
DCLIP_API int dclip_gemm_f16_scaled_rows_dev(const void* A, const void* W, float* C, const float* aux32, int M, int N, int K, int lda,
                                             int ldw, int ldc, int epilogue, const float* alpha, const float* row_alpha,
                                             void* stream) {
  DCLIP_REQUIRE(alpha && row_alpha && ((uintptr_t)alpha | (uintptr_t)row_alpha) % 4 == 0,
                "gemm_f16_scaled_rows_dev: alpha / row_alpha must be device pointers");
  DCLIP_REQUIRE(epilogue == 0 || epilogue == DCLIP_EPI_DGELU, "gemm_f16_scaled_rows_dev: the epilogue is none or DGELU");
  DCLIP_REQUIRE(!(epilogue & DCLIP_EPI_DGELU) || (aux32 && (uintptr_t)aux32 % 16 == 0),
                "gemm_f16_scaled_rows_dev: DGELU needs a 16-byte aligned fp32 aux32");
  DevScales dev{alpha, nullptr, nullptr, nullptr};
  dev.row_alpha = row_alpha;
  dev.aux32 = (epilogue & DCLIP_EPI_DGELU) ? aux32 : nullptr;
  return gemm16<F16T>("gemm_f16_scaled_rows_dev", A, W, C, nullptr, nullptr, nullptr, M, N, K, lda, ldw, ldc, epilogue, 0, stream, 1.f,
                      0.f, &dev);
}

// dclip_gemm_f16_scaled_rows_dev that also leaves the column statistics of the C it stores, for the single-pass
// split of C as the next weight gradient's dY: pmax / psum [P][N], P = dclip_gemm_f16_scaled_rows_stats_plan(M, N, K) = ceil(M /
// 256) partial rows (one per tile row), every word written; C is bit-equal to dclip_gemm_f16_scaled_rows_dev's.  The ping-pong
// kernel only: _plan returns 0 where the dispatcher takes a register-staged kernel, and the caller then takes the plain entry.
DCLIP_API int dclip_gemm_f16_scaled_rows_stats_plan(int M, int N, int K) {
  return M > 0 && N > 0 && K > 0 && takes_pp(M, N, K) ? cdiv(M, 256) : 0;
}

DCLIP_API int dclip_gemm_f16_scaled_rows_stats_dev(const void* A, const void* W, float* C, const float* aux32, int M, int N, int K,
                                                   int lda, int ldw, int ldc, int epilogue, const float* alpha, const float* row_alpha,
                                                   void* pmax, float* psum, void* stream) {
  DCLIP_REQUIRE(alpha && row_alpha && ((uintptr_t)alpha | (uintptr_t)row_alpha) % 4 == 0,
                "gemm_f16_scaled_rows_stats_dev: alpha / row_alpha must be device pointers");
  DCLIP_REQUIRE(pmax && psum && ((uintptr_t)pmax | (uintptr_t)psum) % 4 == 0, "gemm_f16_scaled_rows_stats_dev: pmax / psum");
  DCLIP_REQUIRE(epilogue == 0 || epilogue == DCLIP_EPI_DGELU, "gemm_f16_scaled_rows_stats_dev: the epilogue is none or DGELU");
  DCLIP_REQUIRE(!(epilogue & DCLIP_EPI_DGELU) || (aux32 && (uintptr_t)aux32 % 16 == 0),
                "gemm_f16_scaled_rows_stats_dev: DGELU needs a 16-byte aligned fp32 aux32");
  DCLIP_REQUIRE(dclip_gemm_f16_scaled_rows_stats_plan(M, N, K) > 0,
                "gemm_f16_scaled_rows_stats_dev: M=%d N=%d K=%d takes a register-staged kernel, which has no statistics form", M, N, K);
  DevScales dev{alpha, nullptr, nullptr, nullptr};
  dev.row_alpha = row_alpha;
  dev.aux32 = (epilogue & DCLIP_EPI_DGELU) ? aux32 : nullptr;
  dev.pmax = (unsigned*)pmax;
  dev.psum = psum;
  return gemm16<F16T>("gemm_f16_scaled_rows_dev.stats", A, W, C, nullptr, nullptr, nullptr, M, N, K, lda, ldw, ldc, epilogue, 0, stream,
                      1.f, 0.f, &dev);
}

// ---------------------------------------------------------------------------------------------------------------
// Fused split-fp16 GEMMs: C = epilogue(alpha (A_hi W_hi^T + A_lo W_hi^T + A_hi W_lo^T)) with A_hi / A_lo the K
// columns of A from column a_hi / a_lo on and W_hi / W_lo those of W from w_hi / w_lo on — the operands of the scaled entries
// above as they lie (A = [hi|lo|hi]: 0, K; W = [hi|hi|lo]: 0, 2K), each piece staged once (the FUSED kernel instances).  K is
// the LOGICAL contraction length, a multiple of 32; the ping-pong kernel only, at any M and N.  Epilogues, scales and outputs
// are those of the entry each twins; the accumulation order differs, so the values agree to fp32 rounding, not bit for bit.
namespace {
struct Segs { int a_hi, a_lo, w_hi, w_lo; };

// Tile height of a fused call: 192 rows where the 256-row tiles leave CUs idle and a third more, cheaper tiles still
// fit the same number of rounds.  has192: the call's form has a 192-row instance (K-major fp32 output, no split output, no
// statistics).  DCLIP_F16X3_BM192 (read per call): 0 never, 1 by the rule below (default), 2 wherever the instance exists (tests,
// A/Bs).  The rule: at least DCLIP_F16X3_BM192_MIN 256-row tiles (default 128, a threshold of its own, read per call) and
//     ceil(tiles192 / CUs) * r < ceil(tiles256 / CUs),   CUs = 256,
// r = the cost of a 192-row tile relative to a 256-row one: kBm192CostPct / 100, the largest ratio measured on the flagship
// step's seven single-round shapes rounded up — 0.84-0.85 at K >= 2048, 0.86-0.90 at K = 512 / 768, largest 0.903 (DESIGN.md §9i
// has the table; the model said 0.80).  With it a round more never pays (3 r >= 2, 4 r >= 3), so the rule needs no K term.
// The outputs are bit-equal at both heights.
constexpr int kBm192CostPct = 91;
int f16x3_tile_rows(int M, int N, bool has192) {
  const int mode = getenv("DCLIP_F16X3_BM192") ? atoi(getenv("DCLIP_F16X3_BM192")) : 1;
  if (!has192 || mode <= 0) return 256;
  if (mode >= 2) return 192;
  const int tiles_min = getenv("DCLIP_F16X3_BM192_MIN") ? atoi(getenv("DCLIP_F16X3_BM192_MIN")) : 128;
  const long t256 = (long)cdiv(M, 256) * cdiv(N, 256), t192 = (long)cdiv(M, 192) * cdiv(N, 256);
  if (t256 < tiles_min) return 256;
  const long r256 = (t256 + 255) / 256, r192 = (t192 + 255) / 256;
  return r192 * kBm192CostPct < r256 * 100 ? 192 : 256;
}

int gemm16x3(const char* name, const void* A, const void* W, void* C, const float* bias, const float* residual, int M, int N, int K,
             int lda, int ldw, int ldc, Segs sg, int epilogue, int out_f16, void* stream, float alpha, float out_scale,
             const DevScales* dev, int pieces = 3) {
  DCLIP_REQUIRE(A && W && C, "%s: null operand", name);
  DCLIP_REQUIRE(M > 0 && N > 0 && K > 0 && K % 32 == 0, "%s: bad shape M=%d N=%d K=%d (K: the logical length, a multiple of 32)", name,
                M, N, K);
  DCLIP_REQUIRE(lda % 8 == 0 && ldw % 8 == 0 && lda > 0 && ldw > 0, "%s: lda/ldw must be multiples of 8", name);
  DCLIP_REQUIRE(sg.a_hi >= 0 && sg.a_lo >= 0 && sg.w_hi >= 0 && sg.w_lo >= 0 && (sg.a_hi | sg.a_lo | sg.w_hi | sg.w_lo) % 8 == 0,
                "%s: segment offsets must be non-negative multiples of 8", name);
  DCLIP_REQUIRE((long)sg.a_hi + K <= lda && (long)sg.a_lo + K <= lda && (long)sg.w_hi + K <= ldw && (long)sg.w_lo + K <= ldw,
                "%s: a segment (offset + K) must lie within the leading dimension", name);
  DCLIP_REQUIRE(N % 4 == 0 && ldc % 4 == 0 && ldc >= N, "%s: N / ldc must be multiples of 4", name);
  DCLIP_REQUIRE(((uintptr_t)A | (uintptr_t)W | (uintptr_t)C) % 16 == 0, "%s: operands must be 16-byte aligned", name);
  DCLIP_REQUIRE(!(epilogue & ~(DCLIP_EPI_BIAS | DCLIP_EPI_GELU | DCLIP_EPI_DGELU | DCLIP_EPI_RESIDUAL)),
                "%s: unsupported epilogue bits", name);
  DCLIP_REQUIRE(out_scale == 0.f || (!out_f16 && !(epilogue & (DCLIP_EPI_RESIDUAL | DCLIP_EPI_DGELU)) && (long)ldc >= (long)pieces * N),
                "%s: a split output takes BIAS | GELU only and ldc >= %d N", name, pieces);
  DCLIP_REQUIRE(pieces == 3 || (pieces == 2 && out_scale != 0.f), "%s: two pieces go with a split output", name);
  DCLIP_REQUIRE(!(epilogue & DCLIP_EPI_DGELU) || (dev && dev->aux32 && !(epilogue & DCLIP_EPI_GELU)), "%s: DGELU needs aux32", name);
  DCLIP_REQUIRE(!(epilogue & DCLIP_EPI_BIAS) || bias, "%s: BIAS without bias", name);
  DCLIP_REQUIRE(!(epilogue & DCLIP_EPI_RESIDUAL) || (residual && !out_f16), "%s: RESIDUAL needs an fp32 output", name);
  // 32-bit byte offsets inside a 256-row tile (the kernel's buffer loads)
  DCLIP_REQUIRE(256L * lda * 2 < 0x7fffffffL && 256L * ldw * 2 < 0x7fffffffL, "%s: leading dimension too large", name);
  const bool has192 = !out_f16 && out_scale == 0.f && !(dev && dev->pmax);
  const int bm = f16x3_tile_rows(M, N, has192);
  GemmBf16Params p{(const __bf16*)A, (const __bf16*)W, C, bias, residual, M, N, K, lda, ldw, ldc, epilogue, out_f16, cdiv(M, bm),
                   cdiv(N, 256), nullptr, 0, nullptr, alpha, out_scale};
  set_dev(p, dev);
  p.a_seg[0] = sg.a_hi, p.a_seg[1] = sg.a_lo, p.w_seg[0] = sg.w_hi, p.w_seg[1] = sg.w_lo;
  const dim3 grid(p.tiles_m * p.tiles_n), block(512);
  hipStream_t st = (hipStream_t)stream;
  if (bm == 192) {
    if (p.row_alpha)
      hipLaunchKernelGGL((gemm_bf16_pp_kernel<F16T, false, true, true, false, false, true, 192>), grid, block, 0, st, p);
    else if (p.alpha_p)
      hipLaunchKernelGGL((gemm_bf16_pp_kernel<F16T, false, true, false, false, false, true, 192>), grid, block, 0, st, p);
    else
      hipLaunchKernelGGL((gemm_bf16_pp_kernel<F16T, false, false, false, false, false, true, 192>), grid, block, 0, st, p);
    DCLIP_CHECK_LAUNCH_V(name, ".pp3_192");
    return DCLIP_OK;
  }
  if (pieces == 2) {
    if (p.alpha_p)
      hipLaunchKernelGGL((gemm_bf16_pp_kernel<F16T, false, true, false, false, false, true, 256, 2>), grid, block, 0, st, p);
    else
      hipLaunchKernelGGL((gemm_bf16_pp_kernel<F16T, false, false, false, false, false, true, 256, 2>), grid, block, 0, st, p);
    DCLIP_CHECK_LAUNCH_V(name, ".pp3");
    return DCLIP_OK;
  }
  if (p.row_alpha && p.pmax)
    hipLaunchKernelGGL((gemm_bf16_pp_kernel<F16T, false, true, true, false, true, true>), grid, block, 0, st, p);
  else if (p.row_alpha)
    hipLaunchKernelGGL((gemm_bf16_pp_kernel<F16T, false, true, true, false, false, true>), grid, block, 0, st, p);
  else if (p.alpha_p)
    hipLaunchKernelGGL((gemm_bf16_pp_kernel<F16T, false, true, false, false, false, true>), grid, block, 0, st, p);
  else
    hipLaunchKernelGGL((gemm_bf16_pp_kernel<F16T, false, false, false, false, false, true>), grid, block, 0, st, p);
  DCLIP_CHECK_LAUNCH_V(name, ".pp3");
  return DCLIP_OK;
}
}  // namespace

// Where the step should take a fused entry: exactly where the unfused entry (contraction length 3 K) takes the ping-pong kernel.
// DCLIP_F16X3_MIN (default 128 tiles, the dispatcher's own default; a tuning aid read per call) is a threshold of its own, so that
// lowering DCLIP_BF16_BIG_MIN alone moves the unfused entries onto the ping-pong kernel and nothing else.
DCLIP_API int dclip_gemm_f16x3_plan(int M, int N, int K) {
  if (M <= 0 || N <= 0 || K <= 0 || K % 32 != 0 || !takes_pp(M, N, 3 * K)) return 0;
  const int tiles_min = getenv("DCLIP_F16X3_MIN") ? atoi(getenv("DCLIP_F16X3_MIN")) : 128;
  return (long)cdiv(M, 256) * cdiv(N, 256) >= tiles_min ? 1 : 0;
}

// Where the student's patch embedding [rows, K] x [D, K] takes the fused entry on split operands: where the plan
// above holds AND the call has at least DCLIP_PATCH_SPLIT16_MIN tiles (default 128; read per call).  A threshold of its own, so
// that lowering the two above moves the encoder layers' GEMMs onto their fused entries and leaves the patch embedding where it was.
DCLIP_API int dclip_split16_patch_plan(int rows, int D, int K) {
  if (dclip_gemm_f16x3_plan(rows, D, K) == 0) return 0;
  const int tiles_min = getenv("DCLIP_PATCH_SPLIT16_MIN") ? atoi(getenv("DCLIP_PATCH_SPLIT16_MIN")) : 128;
  return (long)cdiv(rows, 256) * cdiv(D, 256) >= tiles_min ? 1 : 0;
}

// The tile height a fused fp32-output call of this shape takes now (192 or 256): rows_form = the row-scaled entry, stats_form = its
// statistics twin (always 256).  Split-output and 16-bit-output calls always take 256.
DCLIP_API int dclip_gemm_f16x3_tile_rows(int M, int N, int K, int rows_form, int stats_form) {
  (void)K, (void)rows_form;   // every fp32-output form has the 192-row instance; the rule has no K term
  if (M <= 0 || N <= 0) return 256;
  return f16x3_tile_rows(M, N, !stats_form);
}

DCLIP_API int dclip_gemm_f16x3_scaled(const void* A, const void* W, void* C, const float* bias, const float* residual, int M, int N,
                                      int K, int lda, int ldw, int ldc, int a_hi, int a_lo, int w_hi, int w_lo, int epilogue,
                                      int out_f16, float alpha, void* stream) {
  DCLIP_REQUIRE(!(epilogue & DCLIP_EPI_DGELU), "gemm_f16x3_scaled: DGELU is a training epilogue");
  DCLIP_REQUIRE(alpha == alpha && alpha - alpha == 0.f, "gemm_f16x3_scaled: alpha must be finite");
  return gemm16x3("gemm_f16x3_scaled", A, W, C, bias, residual, M, N, K, lda, ldw, ldc, Segs{a_hi, a_lo, w_hi, w_lo}, epilogue, out_f16,
                  stream, alpha, 0.f, nullptr);
}

DCLIP_API int dclip_gemm_f16x3_scaled_split(const void* A, const void* W, void* C, const float* bias, int M, int N, int K, int lda,
                                            int ldw, int ldc, int a_hi, int a_lo, int w_hi, int w_lo, int epilogue, float alpha,
                                            float out_scale, void* stream) {
  DCLIP_REQUIRE(alpha == alpha && alpha - alpha == 0.f, "gemm_f16x3_scaled_split: alpha must be finite");
  DCLIP_REQUIRE(out_scale > 0.f && out_scale - out_scale == 0.f && (__builtin_bit_cast(unsigned int, out_scale) & 0x007fffffu) == 0,
                "gemm_f16x3_scaled_split: out_scale must be a power of two");
  DCLIP_REQUIRE(ldc % 8 == 0, "gemm_f16x3_scaled_split: ldc must be a multiple of 8");
  return gemm16x3("gemm_f16x3_scaled_split", A, W, C, bias, nullptr, M, N, K, lda, ldw, ldc, Segs{a_hi, a_lo, w_hi, w_lo}, epilogue, 0,
                  stream, alpha, out_scale, nullptr);
}

DCLIP_API int dclip_gemm_f16x3_scaled_dev(const void* A, const void* W, void* C, const float* bias, const float* residual, int M,
                                          int N, int K, int lda, int ldw, int ldc, int a_hi, int a_lo, int w_hi, int w_lo, int epilogue,
                                          int out_f16, const float* alpha, void* stream) {
  DCLIP_REQUIRE(!(epilogue & DCLIP_EPI_DGELU), "gemm_f16x3_scaled_dev: DGELU is a training epilogue");
  DCLIP_REQUIRE(alpha && (uintptr_t)alpha % 4 == 0, "gemm_f16x3_scaled_dev: alpha must be a device pointer");
  const DevScales dev{alpha, nullptr, nullptr, nullptr};
  return gemm16x3("gemm_f16x3_scaled_dev", A, W, C, bias, residual, M, N, K, lda, ldw, ldc, Segs{a_hi, a_lo, w_hi, w_lo}, epilogue,
                  out_f16, stream, 1.f, 0.f, &dev);
}

DCLIP_API int dclip_gemm_f16x3_scaled_split_dev(const void* A, const void* W, void* C, const float* bias, float* h32, float* g32,
                                                int M, int N, int K, int lda, int ldw, int ldc, int a_hi, int a_lo, int w_hi, int w_lo,
                                                int epilogue, const float* alpha, const float* out_scale, void* stream) {
  DCLIP_REQUIRE(alpha && ((uintptr_t)alpha | (uintptr_t)out_scale) % 4 == 0,
                "gemm_f16x3_scaled_split_dev: alpha / out_scale must be device pointers");
  DCLIP_REQUIRE(ldc % 8 == 0, "gemm_f16x3_scaled_split_dev: ldc must be a multiple of 8");
  DCLIP_REQUIRE(((uintptr_t)h32 | (uintptr_t)g32) % 16 == 0, "gemm_f16x3_scaled_split_dev: h32 / g32 must be 16-byte aligned");
  DCLIP_REQUIRE(!h32 || (epilogue & DCLIP_EPI_GELU), "gemm_f16x3_scaled_split_dev: h32 is the pre-activation of a GELU epilogue");
  DCLIP_REQUIRE(!(epilogue & ~(DCLIP_EPI_BIAS | DCLIP_EPI_GELU)), "gemm_f16x3_scaled_split_dev: the epilogue is BIAS | GELU");
  DCLIP_REQUIRE(out_scale || !g32, "gemm_f16x3_scaled_split_dev: without out_scale C is the fp32 result (g32 must be NULL)");
  const DevScales dev{alpha, out_scale, h32, g32};
  return gemm16x3("gemm_f16x3_scaled_split_dev", A, W, C, bias, nullptr, M, N, K, lda, ldw, ldc, Segs{a_hi, a_lo, w_hi, w_lo}, epilogue,
                  0, stream, 1.f, out_scale ? 1.f : 0.f, &dev);
}

// The two-piece forms of the two split-output entries above: C fp16 [M][ldc >= 2 N] = [hi | lo], bit-equal to the
// first two pieces of theirs; nothing past column 2 N of a row is written; h32 / g32 as there.  out_scale is required.  The launch
// is recorded under the three-piece twin's name (the same call site of the step).
DCLIP_API int dclip_gemm_f16x3_scaled_split2(const void* A, const void* W, void* C, const float* bias, int M, int N, int K, int lda,
                                             int ldw, int ldc, int a_hi, int a_lo, int w_hi, int w_lo, int epilogue, float alpha,
                                             float out_scale, void* stream) {
  DCLIP_REQUIRE(alpha == alpha && alpha - alpha == 0.f, "gemm_f16x3_scaled_split2: alpha must be finite");
  DCLIP_REQUIRE(out_scale > 0.f && out_scale - out_scale == 0.f && (__builtin_bit_cast(unsigned int, out_scale) & 0x007fffffu) == 0,
                "gemm_f16x3_scaled_split2: out_scale must be a power of two");
  DCLIP_REQUIRE(ldc % 8 == 0, "gemm_f16x3_scaled_split2: ldc must be a multiple of 8");
  DCLIP_REQUIRE(!(epilogue & ~(DCLIP_EPI_BIAS | DCLIP_EPI_GELU)), "gemm_f16x3_scaled_split2: the epilogue is BIAS | GELU");
  return gemm16x3("gemm_f16x3_scaled_split", A, W, C, bias, nullptr, M, N, K, lda, ldw, ldc, Segs{a_hi, a_lo, w_hi, w_lo}, epilogue, 0,
                  stream, alpha, out_scale, nullptr, 2);
}

DCLIP_API int dclip_gemm_f16x3_scaled_split2_dev(const void* A, const void* W, void* C, const float* bias, float* h32, float* g32,
                                                 int M, int N, int K, int lda, int ldw, int ldc, int a_hi, int a_lo, int w_hi, int w_lo,
                                                 int epilogue, const float* alpha, const float* out_scale, void* stream) {
  DCLIP_REQUIRE(alpha && out_scale && ((uintptr_t)alpha | (uintptr_t)out_scale) % 4 == 0,
                "gemm_f16x3_scaled_split2_dev: alpha / out_scale must be device pointers");
  DCLIP_REQUIRE(ldc % 8 == 0, "gemm_f16x3_scaled_split2_dev: ldc must be a multiple of 8");
  DCLIP_REQUIRE(((uintptr_t)h32 | (uintptr_t)g32) % 16 == 0, "gemm_f16x3_scaled_split2_dev: h32 / g32 must be 16-byte aligned");
  DCLIP_REQUIRE(!h32 || (epilogue & DCLIP_EPI_GELU), "gemm_f16x3_scaled_split2_dev: h32 is the pre-activation of a GELU epilogue");
  DCLIP_REQUIRE(!(epilogue & ~(DCLIP_EPI_BIAS | DCLIP_EPI_GELU)), "gemm_f16x3_scaled_split2_dev: the epilogue is BIAS | GELU");
  const DevScales dev{alpha, out_scale, h32, g32};
  return gemm16x3("gemm_f16x3_scaled_split_dev", A, W, C, bias, nullptr, M, N, K, lda, ldw, ldc, Segs{a_hi, a_lo, w_hi, w_lo}, epilogue,
                  0, stream, 1.f, 1.f, &dev, 2);
}

DCLIP_API int dclip_gemm_f16x3_scaled_rows_dev(const void* A, const void* W, float* C, const float* aux32, int M, int N, int K, int lda,
                                               int ldw, int ldc, int a_hi, int a_lo, int w_hi, int w_lo, int epilogue,
                                               const float* alpha, const float* row_alpha, void* stream) {
  DCLIP_REQUIRE(alpha && row_alpha && ((uintptr_t)alpha | (uintptr_t)row_alpha) % 4 == 0,
                "gemm_f16x3_scaled_rows_dev: alpha / row_alpha must be device pointers");
  DCLIP_REQUIRE(epilogue == 0 || epilogue == DCLIP_EPI_DGELU, "gemm_f16x3_scaled_rows_dev: the epilogue is none or DGELU");
  DCLIP_REQUIRE(!(epilogue & DCLIP_EPI_DGELU) || (aux32 && (uintptr_t)aux32 % 16 == 0),
                "gemm_f16x3_scaled_rows_dev: DGELU needs a 16-byte aligned fp32 aux32");
  DevScales dev{alpha, nullptr, nullptr, nullptr};
  dev.row_alpha = row_alpha;
  dev.aux32 = (epilogue & DCLIP_EPI_DGELU) ? aux32 : nullptr;
  return gemm16x3("gemm_f16x3_scaled_rows_dev", A, W, C, nullptr, nullptr, M, N, K, lda, ldw, ldc, Segs{a_hi, a_lo, w_hi, w_lo},
                  epilogue, 0, stream, 1.f, 0.f, &dev);
}

// Partial rows of the statistics twin: ceil(M / 256) where dclip_gemm_f16x3_plan holds, else 0.
DCLIP_API int dclip_gemm_f16x3_scaled_rows_stats_plan(int M, int N, int K) {
  return dclip_gemm_f16x3_plan(M, N, K) ? cdiv(M, 256) : 0;
}

// pmax / psum [ceil(M / 256)][N], every word written (the entry itself runs at any M, N: it has the ping-pong kernel only).
DCLIP_API int dclip_gemm_f16x3_scaled_rows_stats_dev(const void* A, const void* W, float* C, const float* aux32, int M, int N, int K,
                                                     int lda, int ldw, int ldc, int a_hi, int a_lo, int w_hi, int w_lo, int epilogue,
                                                     const float* alpha, const float* row_alpha, void* pmax, float* psum,
                                                     void* stream) {
  DCLIP_REQUIRE(alpha && row_alpha && ((uintptr_t)alpha | (uintptr_t)row_alpha) % 4 == 0,
                "gemm_f16x3_scaled_rows_stats_dev: alpha / row_alpha must be device pointers");
  DCLIP_REQUIRE(pmax && psum && ((uintptr_t)pmax | (uintptr_t)psum) % 4 == 0, "gemm_f16x3_scaled_rows_stats_dev: pmax / psum");
  DCLIP_REQUIRE(epilogue == 0 || epilogue == DCLIP_EPI_DGELU, "gemm_f16x3_scaled_rows_stats_dev: the epilogue is none or DGELU");
  DCLIP_REQUIRE(!(epilogue & DCLIP_EPI_DGELU) || (aux32 && (uintptr_t)aux32 % 16 == 0),
                "gemm_f16x3_scaled_rows_stats_dev: DGELU needs a 16-byte aligned fp32 aux32");
  DevScales dev{alpha, nullptr, nullptr, nullptr};
  dev.row_alpha = row_alpha;
  dev.aux32 = (epilogue & DCLIP_EPI_DGELU) ? aux32 : nullptr;
  dev.pmax = (unsigned*)pmax;
  dev.psum = psum;
  return gemm16x3("gemm_f16x3_scaled_rows_dev.stats", A, W, C, nullptr, nullptr, M, N, K, lda, ldw, ldc, Segs{a_hi, a_lo, w_hi, w_lo},
                  epilogue, 0, stream, 1.f, 0.f, &dev);
}

// fp16 TRAINING path: dclip_gemm_bf16_ex's arguments, epilogues and limits with fp16 A / W / aux / 16-bit C, IEEE rounding
// (common.h, F16IeeeT: an overflow becomes +-inf).  The ping-pong / register-staged kernels only (DCLIP_BF16_PERSIST does
// not apply).
DCLIP_API int dclip_gemm_f16_ex(const void* A, const void* W, void* C, const float* bias, const float* residual, void* aux,
                                int M, int N, int K, int lda, int ldw, int ldc, int epilogue, int out_f16, void* stream) {
  return gemm16<F16IeeeT>("gemm_f16_ex", A, W, C, bias, residual, aux, M, N, K, lda, ldw, ldc, epilogue, out_f16, stream);
}

// dW[M = out][N = in] fp32 = dY^T X from the operands as the backward has them: dY [K = tokens][lddy >= M], X [K][ldx >= N],
// bf16, token-major — no transposes.  Split-K over the tokens on the ping-pong kernel (token-major form), fixed-order reduce.
// dclip_gemm_bf16_wgrad_tokmajor_plan = the split count to pass, 0 when this form does not apply (K % 64, M / N % 8, too few
// work items for the chip): the caller then transposes and uses dclip_gemm_bf16_splitk.
namespace {
int tokmajor_plan(int M, int N, int K) {
  if (K % BKH != 0 || M % 8 != 0 || N % 8 != 0) return 0;
  const long t256 = (long)cdiv(M, 256) * cdiv(N, 256);
  int s = t256 >= 256 ? 1 : (int)(256 / t256);
  const int kmax = K / 512 > 0 ? K / 512 : 1;                 // at least 8 K-tiles per work item
  s = s > kmax ? kmax : s;
  s = s > 64 ? 64 : s;
  return t256 * s >= 128 ? s : 0;
}

template <class T>
int wgrad_tokmajor16(const char* name, const void* dY, const void* X, float* C, int M, int N, int K, int lddy, int ldx, int ldc,
                     int splits, void* workspace, size_t workspace_bytes, void* stream) {
  DCLIP_REQUIRE(dY && X && C, "%s: null operand", name);
  DCLIP_REQUIRE(M > 0 && N > 0 && K > 0 && K % BKH == 0 && M % 8 == 0 && N % 8 == 0 && splits >= 1 && splits <= 64,
                "%s: M=%d N=%d (multiples of 8) K=%d (multiple of 64) splits=%d", name, M, N, K, splits);
  DCLIP_REQUIRE(lddy % 8 == 0 && ldx % 8 == 0 && lddy >= M && ldx >= N && ldc % 4 == 0 && ldc >= N, "%s: leading dimensions", name);
  DCLIP_REQUIRE(((uintptr_t)dY | (uintptr_t)X | (uintptr_t)C) % 16 == 0, "%s: operands must be 16-byte aligned", name);
  const int kps = cdiv(cdiv(K, splits), BKH) * BKH;
  const int s_eff = cdiv(K, kps);
  hipStream_t st = (hipStream_t)stream;
  if (s_eff == 1) {
    GemmBf16Params pb{(const __bf16*)dY, (const __bf16*)X, C, nullptr, nullptr, M, N, K, lddy, ldx, ldc, 0, 0, 0, 0, nullptr, 0, nullptr};
    launch_pp<T, true>(pb, st, 1);
    DCLIP_CHECK_LAUNCH_V(name, ".pp_tok");
    return DCLIP_OK;
  }
  const size_t need = (size_t)s_eff * M * N * sizeof(float);
  if (!workspace || workspace_bytes < need) {
    dclip_set_error("%s: needs %zu workspace bytes, got %zu", name, need, workspace_bytes);
    return DCLIP_EWORKSPACE;
  }
  DCLIP_REQUIRE((uintptr_t)workspace % 16 == 0, "%s: workspace must be 16-byte aligned", name);
  GemmBf16Params pb{(const __bf16*)dY, (const __bf16*)X, C, nullptr, nullptr, M, N, K, lddy, ldx, ldc, 0, 0, 0, 0, nullptr, kps,
                    (float*)workspace};
  launch_pp<T, true>(pb, st, s_eff);
  DCLIP_CHECK_LAUNCH_V(name, ".pp_tok");
  hipLaunchKernelGGL(splitk_reduce_bf16_kernel, dim3(grid_for((size_t)M * N / 4)), dim3(256), 0, st, (const float*)workspace, C, M,
                     N, ldc, s_eff);
  DCLIP_CHECK_LAUNCH_V(name, ".pp_tok.splitk_reduce");
  return DCLIP_OK;
}
}  // namespace

DCLIP_API int dclip_gemm_bf16_wgrad_tokmajor_plan(int M, int N, int K) { return tokmajor_plan(M, N, K); }

DCLIP_API int dclip_gemm_bf16_wgrad_tokmajor(const void* dY, const void* X, float* C, int M, int N, int K, int lddy, int ldx,
                                             int ldc, int splits, void* workspace, size_t workspace_bytes, void* stream) {
  return wgrad_tokmajor16<Bf16T>("gemm_bf16_wgrad_tokmajor", dY, X, C, M, N, K, lddy, ldx, ldc, splits, workspace,
                                 workspace_bytes, stream);
}

// fp16 twins (training path, IEEE rounding is not involved: fp16 operands in, fp32 out)
DCLIP_API int dclip_gemm_f16_wgrad_tokmajor_plan(int M, int N, int K) { return dclip_gemm_bf16_wgrad_tokmajor_plan(M, N, K); }

DCLIP_API int dclip_gemm_f16_wgrad_tokmajor(const void* dY, const void* X, float* C, int M, int N, int K, int lddy, int ldx,
                                            int ldc, int splits, void* workspace, size_t workspace_bytes, void* stream) {
  return wgrad_tokmajor16<F16IeeeT>("gemm_f16_wgrad_tokmajor", dY, X, C, M, N, K, lddy, ldx, ldc, splits, workspace,
                                    workspace_bytes, stream);
}

// The segmented form: dW[M][N] = ((sum over three segments s of dY_s^T X_s) / *act_scale) * col_alpha[m], with
// dY_s = the M columns of dY from column a_seg[s] on and X_s = the N columns of X from w_seg[s] on, fp16 token-major
// [tokens][lddy] / [tokens][ldx].  With dY = [hi|lo] (a_seg 0, M, 0) and X = [hi|lo|hi] (w_seg 0, 0, N) the segments are the
// three products hi.hi + lo.hi + hi.lo of the split-fp16 weight gradient, out of the operands as the step already has them.
// `splits` work items per tile and segment (3 splits slabs of fp32 partials in the workspace: dclip_gemm_f16_splitk_workspace(M,
// N, 3 splits)), fixed-order reduce that also applies the two scales.  _plan: the split count, 0 = this form does not apply
// (tokens % 64, M / N % 8) and the caller takes the fp32 GEMM.
DCLIP_API int dclip_gemm_f16_wgrad_tokmajor_seg3_plan(int M, int N, int tokens) {
  if (M <= 0 || N <= 0 || tokens <= 0 || tokens % BKH != 0 || M % 8 != 0 || N % 8 != 0) return 0;
  const long items = 3L * cdiv(M, 256) * cdiv(N, 256);       // work items at one split per segment
  int s = items >= 256 ? 1 : (int)(256 / items);             // one round of 256 CUs
  const int kmax = tokens / 512 > 0 ? tokens / 512 : 1;      // at least 8 K-tiles per work item
  s = s > kmax ? kmax : s;
  return s > 21 ? 21 : s;                                    // 3 s <= 64 slabs
}

DCLIP_API int dclip_gemm_f16_wgrad_tokmajor_seg3(const void* dY, const void* X, float* C, int M, int N, int tokens, int lddy, int ldx,
                                                 int ldc, int a_seg0, int a_seg1, int a_seg2, int w_seg0, int w_seg1, int w_seg2,
                                                 const float* col_alpha, const float* act_scale, int splits, void* workspace,
                                                 size_t workspace_bytes, void* stream) {
  const char* name = "gemm_f16_wgrad_tokmajor_seg3";
  const int a_seg[3] = {a_seg0, a_seg1, a_seg2}, w_seg[3] = {w_seg0, w_seg1, w_seg2};
  DCLIP_REQUIRE(dY && X && C && col_alpha && act_scale, "%s: null operand", name);
  DCLIP_REQUIRE(M > 0 && N > 0 && tokens > 0 && tokens % BKH == 0 && M % 8 == 0 && N % 8 == 0 && splits >= 1 && splits <= 21,
                "%s: M=%d N=%d (multiples of 8) tokens=%d (multiple of 64) splits=%d (1..21)", name, M, N, tokens, splits);
  DCLIP_REQUIRE(lddy % 8 == 0 && ldx % 8 == 0 && ldc % 4 == 0 && ldc >= N, "%s: leading dimensions", name);
  for (int s = 0; s < 3; ++s)
    DCLIP_REQUIRE(a_seg[s] >= 0 && w_seg[s] >= 0 && a_seg[s] % 8 == 0 && w_seg[s] % 8 == 0 && (long)a_seg[s] + M <= lddy &&
                      (long)w_seg[s] + N <= ldx,
                  "%s: segment %d (offsets are multiples of 8, offset + width within the leading dimension)", name, s);
  DCLIP_REQUIRE(((uintptr_t)dY | (uintptr_t)X | (uintptr_t)C | (uintptr_t)workspace) % 16 == 0 &&
                    ((uintptr_t)col_alpha | (uintptr_t)act_scale) % 4 == 0, "%s: alignment", name);
  const int kps = cdiv(cdiv(tokens, splits), BKH) * BKH;
  const int s_eff = cdiv(tokens, kps);
  const size_t need = (size_t)3 * s_eff * M * N * sizeof(float);
  if (!workspace || workspace_bytes < need) {
    dclip_set_error("%s: needs %zu workspace bytes, got %zu", name, need, workspace_bytes);
    return DCLIP_EWORKSPACE;
  }
  GemmBf16Params pb{(const __bf16*)dY, (const __bf16*)X, C, nullptr, nullptr, M, N, tokens, lddy, ldx, ldc, 0, 0, 0, 0, nullptr, kps,
                    (float*)workspace};
  pb.seg_splits = s_eff;
  for (int s = 0; s < 3; ++s) pb.a_seg[s] = a_seg[s], pb.w_seg[s] = w_seg[s];
  pb.tiles_m = cdiv(M, 256);
  pb.tiles_n = cdiv(N, 256);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL((gemm_bf16_pp_kernel<F16IeeeT, true, false, false, true>), dim3(pb.tiles_m * pb.tiles_n, 3 * s_eff), dim3(512), 0,
                     st, pb);
  DCLIP_CHECK_LAUNCH_V(name, ".pp_tok_seg");
  hipLaunchKernelGGL(splitk_reduce_scaled_bf16_kernel, dim3(grid_for((size_t)M * N / 4)), dim3(256), 0, st, (const float*)workspace, C,
                     M, N, ldc, 3 * s_eff, col_alpha, act_scale);
  DCLIP_CHECK_LAUNCH_V(name, ".pp_tok_seg.splitk_reduce");
  return DCLIP_OK;
}

// The fused form of the segmented weight gradient: dW[M][N] = ((dY_hi^T X_hi + dY_lo^T X_hi + dY_hi^T X_lo) /
// *act_scale) * col_alpha[m], dY_hi / dY_lo the M columns of dY from dy_hi / dy_lo on, X_hi / X_lo the N columns of X from x_hi /
// x_lo on (the step: 0, M, 0, N).  A work item owns a token range — whole 64-token units — and does all three products for it
// out of one staging of the four pieces (the FUSED token-major kernel instance): `splits` fp32 slabs in the workspace
// (dclip_gemm_f16x3_wgrad_tokmajor_workspace(M, N, splits)), then dclip_gemm_f16_wgrad_tokmajor_seg3's fixed-order scaled reduce.
// _plan: the split count — one round of 256 work items, at least 192 tokens each (about the segmented plan's work-item count;
// swept at the step's shapes) — or 0 where the segmented form does not apply or this one would start fewer than
// DCLIP_F16X3_TOK_MIN (default 128, a tuning aid read per call) work items.
DCLIP_API int dclip_gemm_f16x3_wgrad_tokmajor_plan(int M, int N, int tokens) {
  if (dclip_gemm_f16_wgrad_tokmajor_seg3_plan(M, N, tokens) == 0) return 0;
  const long t256 = (long)cdiv(M, 256) * cdiv(N, 256);
  int s = t256 >= 256 ? 1 : (int)(256 / t256);               // one round of 256 CUs (the sweep of tools/split16_fused_bench.py)
  const int kmax = tokens / 192 > 0 ? tokens / 192 : 1;      // at least 6 K-tiles of 32 tokens per work item
  s = s > kmax ? kmax : s;
  s = s > 64 ? 64 : s;
  const int kps = cdiv(cdiv(tokens, s), BKH) * BKH;
  s = cdiv(tokens, kps);                                       // the slabs the entry will use
  const int items_min = getenv("DCLIP_F16X3_TOK_MIN") ? atoi(getenv("DCLIP_F16X3_TOK_MIN")) : 128;
  return (long)cdiv(M, 256) * cdiv(N, 256) * s >= items_min ? s : 0;
}

// `splits` slabs of M N floats, one split included (the scaled reduce always runs)
DCLIP_API size_t dclip_gemm_f16x3_wgrad_tokmajor_workspace(int M, int N, int splits) {
  return M > 0 && N > 0 && splits > 0 ? (size_t)splits * M * N * sizeof(float) : 0;
}

DCLIP_API int dclip_gemm_f16x3_wgrad_tokmajor(const void* dY, const void* X, float* C, int M, int N, int tokens, int lddy, int ldx,
                                              int ldc, int dy_hi, int dy_lo, int x_hi, int x_lo, const float* col_alpha,
                                              const float* act_scale, int splits, void* workspace, size_t workspace_bytes,
                                              void* stream) {
  const char* name = "gemm_f16x3_wgrad_tokmajor";
  DCLIP_REQUIRE(dY && X && C && col_alpha && act_scale, "%s: null operand", name);
  DCLIP_REQUIRE(M > 0 && N > 0 && tokens > 0 && tokens % BKH == 0 && M % 8 == 0 && N % 8 == 0 && splits >= 1 && splits <= 64,
                "%s: M=%d N=%d (multiples of 8) tokens=%d (multiple of 64) splits=%d (1..64)", name, M, N, tokens, splits);
  DCLIP_REQUIRE(lddy % 8 == 0 && ldx % 8 == 0 && ldc % 4 == 0 && ldc >= N, "%s: leading dimensions", name);
  DCLIP_REQUIRE(dy_hi >= 0 && dy_lo >= 0 && x_hi >= 0 && x_lo >= 0 && (dy_hi | dy_lo | x_hi | x_lo) % 8 == 0 &&
                    (long)dy_hi + M <= lddy && (long)dy_lo + M <= lddy && (long)x_hi + N <= ldx && (long)x_lo + N <= ldx,
                "%s: segments (offsets are multiples of 8, offset + width within the leading dimension)", name);
  DCLIP_REQUIRE(((uintptr_t)dY | (uintptr_t)X | (uintptr_t)C | (uintptr_t)workspace) % 16 == 0 &&
                    ((uintptr_t)col_alpha | (uintptr_t)act_scale) % 4 == 0, "%s: alignment", name);
  // 32-bit byte offsets inside a work item's token range (the kernel's buffer loads)
  DCLIP_REQUIRE((long)tokens * lddy * 2 < 0x7fffffffL && (long)tokens * ldx * 2 < 0x7fffffffL, "%s: operand too large", name);
  const int kps = cdiv(cdiv(tokens, splits), BKH) * BKH;
  const int s_eff = cdiv(tokens, kps);
  const size_t need = (size_t)s_eff * M * N * sizeof(float);
  if (!workspace || workspace_bytes < need) {
    dclip_set_error("%s: needs %zu workspace bytes, got %zu", name, need, workspace_bytes);
    return DCLIP_EWORKSPACE;
  }
  GemmBf16Params pb{(const __bf16*)dY, (const __bf16*)X, C, nullptr, nullptr, M, N, tokens, lddy, ldx, ldc, 0, 0, 0, 0, nullptr, kps,
                    (float*)workspace};
  pb.a_seg[0] = dy_hi, pb.a_seg[1] = dy_lo, pb.w_seg[0] = x_hi, pb.w_seg[1] = x_lo;
  pb.tiles_m = cdiv(M, 256);
  pb.tiles_n = cdiv(N, 256);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL((gemm_bf16_pp_kernel<F16IeeeT, true, false, false, false, false, true>), dim3(pb.tiles_m * pb.tiles_n, s_eff),
                     dim3(512), 0, st, pb);
  DCLIP_CHECK_LAUNCH_V(name, ".pp3_tok");
  hipLaunchKernelGGL(splitk_reduce_scaled_bf16_kernel, dim3(grid_for((size_t)M * N / 4)), dim3(256), 0, st, (const float*)workspace, C,
                     M, N, ldc, s_eff, col_alpha, act_scale);
  DCLIP_CHECK_LAUNCH_V(name, ".pp3_tok.splitk_reduce");
  return DCLIP_OK;
}

namespace {
template <class T>
int cast16(const char* name, const float* x, void* y, int rows, int cols, int ldx, int ldy, void* stream) {
  DCLIP_REQUIRE(x && y && rows > 0 && cols > 0, "%s: bad arguments", name);
  DCLIP_REQUIRE(ldx >= cols && ldy >= cols && ldy % 4 == 0 && ldx % 4 == 0, "%s: ldx/ldy must be multiples of 4", name);
  DCLIP_REQUIRE((uintptr_t)x % 16 == 0 && (uintptr_t)y % 8 == 0, "%s: alignment", name);
  hipLaunchKernelGGL(cast_bf16_kernel<T>, dim3(grid_for((size_t)rows * (ldy / 4))), dim3(256), 0, (hipStream_t)stream, x,
                     (unsigned short*)y, rows, cols, ldx, ldy);
  DCLIP_CHECK_LAUNCH(name);
  return DCLIP_OK;
}

template <class T>
int layernorm16(const char* name, const float* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                int rows, int D, float eps, void* stream) {
  DCLIP_REQUIRE(x && gamma && beta && y, "%s: null pointer", name);
  DCLIP_REQUIRE((mean == nullptr) == (rstd == nullptr), "%s: mean and rstd go together", name);
  DCLIP_REQUIRE(rows > 0 && D > 0 && D % 4 == 0 && D <= 2048, "%s: bad D=%d", name, D);
  dim3 grid(cdiv(rows, 4)), block(256);
  hipStream_t st = (hipStream_t)stream;
  const int nc = cdiv(D / 4, 64);
  unsigned short* yy = (unsigned short*)y;
  const char* variant;
#define LN16(NC, EX)                                                                                                         \
  do {                                                                                                                       \
    hipLaunchKernelGGL((ln_fwd_bf16_kernel<T, NC, EX>), grid, block, 0, st, x, gamma, beta, yy, rows, D, eps, mean, rstd); \
    variant = (EX) ? ".nc" #NC ".exact" : ".nc" #NC;                                                                         \
  } while (0)
  if (D == 512) LN16(2, true);
  else if (D == 768) LN16(3, true);
  else if (D == 1024) LN16(4, true);
  else if (nc <= 1) LN16(1, false);
  else if (nc == 2) LN16(2, false);
  else if (nc == 3) LN16(3, false);
  else if (nc == 4) LN16(4, false);
  else LN16(8, false);
#undef LN16
  DCLIP_CHECK_LAUNCH_V(name, variant);
  return DCLIP_OK;
}
}  // namespace

DCLIP_API int dclip_cast_f32_bf16(const float* x, void* y, int rows, int cols, int ldx, int ldy, void* stream) {
  return cast16<Bf16T>("cast_f32_bf16", x, y, rows, cols, ldx, ldy, stream);
}

DCLIP_API int dclip_cast_f32_f16(const float* x, void* y, int rows, int cols, int ldx, int ldy, void* stream) {
  return cast16<F16T>("cast_f32_f16", x, y, rows, cols, ldx, ldy, stream);
}

// fp16 training path: the same cast with IEEE rounding (beyond +-65504 -> +-inf; dclip_cast_f32_f16 saturates)
DCLIP_API int dclip_cast_f32_f16_ieee(const float* x, void* y, int rows, int cols, int ldx, int ldy, void* stream) {
  return cast16<F16IeeeT>("cast_f32_f16_ieee", x, y, rows, cols, ldx, ldy, stream);
}

DCLIP_API int dclip_layernorm_fwd_bf16(const float* x, const float* gamma, const float* beta, void* y, int rows, int D,
                                       float eps, void* stream) {
  return dclip_layernorm_fwd_bf16_stats(x, gamma, beta, y, nullptr, nullptr, rows, D, eps, stream);
}

DCLIP_API int dclip_layernorm_fwd_bf16_stats(const float* x, const float* gamma, const float* beta, void* y, float* mean,
                                             float* rstd, int rows, int D, float eps, void* stream) {
  return layernorm16<Bf16T>("layernorm_fwd_bf16", x, gamma, beta, y, mean, rstd, rows, D, eps, stream);
}

DCLIP_API int dclip_layernorm_fwd_f16(const float* x, const float* gamma, const float* beta, void* y, int rows, int D,
                                      float eps, void* stream) {
  return layernorm16<F16T>("layernorm_fwd_f16", x, gamma, beta, y, nullptr, nullptr, rows, D, eps, stream);
}

// fp16 training path: layernorm_fwd_bf16_stats with an fp16 result, IEEE rounding
DCLIP_API int dclip_layernorm_fwd_f16_stats(const float* x, const float* gamma, const float* beta, void* y, float* mean,
                                            float* rstd, int rows, int D, float eps, void* stream) {
  return layernorm16<F16IeeeT>("layernorm_fwd_f16_stats", x, gamma, beta, y, mean, rstd, rows, D, eps, stream);
}

namespace {
int splitk_plan(int M, int N, int K) {
  if (K % BKH == 0) {                                  // 256x256 ping-pong kernel, one workgroup per CU
    const long t256 = (long)cdiv(M, 256) * cdiv(N, 256);
    if (t256 >= 128 || K < 2048) return 1;
    int s = (int)(256 / t256);
    const int kmax = K / 512;                                 // at least 8 K-tiles per work item
    s = s > kmax ? kmax : s;
    s = s > 64 ? 64 : s;
    if (s >= 2 && t256 * s >= 128) return s;                  // otherwise too few work items for 256 CUs: 128x128 form below
  }
  const long tiles = (long)cdiv(M, 128) * cdiv(N, 128);
  if (tiles >= 192 || K < 2048) return 1;
  int s = (int)((768 + tiles - 1) / tiles);                 // ~3 work items per CU
  const int kmax = K / 512;                                  // at least 8 K-tiles per work item
  s = s > kmax ? kmax : s;
  return s < 2 ? 1 : (s > 64 ? 64 : s);
}

template <class T>
int splitk16(const char* name, const void* A, const void* W, float* C, int M, int N, int K, int lda, int ldw, int ldc, int splits,
             void* workspace, size_t workspace_bytes, void* stream) {
  DCLIP_REQUIRE(A && W && C, "%s: null operand", name);
  DCLIP_REQUIRE(M > 0 && N > 0 && K > 0 && splits >= 1 && splits <= 1024, "%s: bad shape", name);
  DCLIP_REQUIRE(lda % 8 == 0 && ldw % 8 == 0 && lda >= K && ldw >= K, "%s: lda/ldw must be multiples of 8 and >= K", name);
  DCLIP_REQUIRE(N % 4 == 0 && ldc % 4 == 0 && ldc >= N, "%s: N / ldc must be multiples of 4", name);
  DCLIP_REQUIRE(((uintptr_t)A | (uintptr_t)W | (uintptr_t)C) % 16 == 0, "%s: operands must be 16-byte aligned", name);
  if (splits == 1) return gemm16<T>(name, A, W, C, nullptr, nullptr, nullptr, M, N, K, lda, ldw, ldc, 0, 0, stream);
  const int kps = cdiv(cdiv(K, splits), BKH) * BKH;
  const int s_eff = cdiv(K, kps);
  const size_t need = (size_t)s_eff * M * N * sizeof(float);
  if (!workspace || workspace_bytes < need) {
    dclip_set_error("%s: needs %zu workspace bytes, got %zu", name, need, workspace_bytes);
    return DCLIP_EWORKSPACE;
  }
  DCLIP_REQUIRE((uintptr_t)workspace % 16 == 0, "%s: workspace must be 16-byte aligned", name);
  if (K % BKH == 0 && (long)cdiv(M, 256) * cdiv(N, 256) * s_eff >= 128) {
    GemmBf16Params pb{(const __bf16*)A, (const __bf16*)W, C, nullptr, nullptr, M, N, K, lda, ldw, ldc, 0, 0, 0, 0, nullptr, kps,
                      (float*)workspace};
    launch_pp<T>(pb, (hipStream_t)stream, s_eff);
    DCLIP_CHECK_LAUNCH_V(name, ".pp");
    hipLaunchKernelGGL(splitk_reduce_bf16_kernel, dim3(grid_for((size_t)M * N / 4)), dim3(256), 0, (hipStream_t)stream,
                       (const float*)workspace, C, M, N, ldc, s_eff);
    DCLIP_CHECK_LAUNCH_V(name, ".pp.splitk_reduce");
    return DCLIP_OK;
  }
  GemmBf16Params p{(const __bf16*)A, (const __bf16*)W, C, nullptr, nullptr, M, N, K, lda, ldw, ldc, 0, 0,
                   cdiv(M, 128), cdiv(N, 128), nullptr, kps, (float*)workspace};
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = (size_t)2 * (128 + 128) * BKH * 2;
  hipLaunchKernelGGL((gemm_bf16_kernel<T, 128, 128>), dim3(p.tiles_m * p.tiles_n, s_eff), dim3(256), lds, st, p);
  DCLIP_CHECK_LAUNCH_V(name, ".r128");
  hipLaunchKernelGGL(splitk_reduce_bf16_kernel, dim3(grid_for((size_t)M * N / 4)), dim3(256), 0, st, (const float*)workspace, C,
                     M, N, ldc, s_eff);
  DCLIP_CHECK_LAUNCH_V(name, ".r128.splitk_reduce");
  return DCLIP_OK;
}
}  // namespace

// Split-K form for products with few output tiles and a long contraction — the weight gradients of the bf16 training
// path, dW[out,in] = (dY^T)[out,tok] (X^T)[in,tok]^T with tok = batch x sequence (12,800 .. 25,600): `splits` work items
// per 128x128 tile write fp32 partials to the caller's workspace, a second kernel sums them in fixed order.  fp32 C, no
// epilogue.  dclip_gemm_bf16_splitk_plan returns the split count this library would choose (1 = use dclip_gemm_bf16).
DCLIP_API int dclip_gemm_bf16_splitk_plan(int M, int N, int K) { return splitk_plan(M, N, K); }

DCLIP_API size_t dclip_gemm_bf16_splitk_workspace(int M, int N, int splits) {
  return splits > 1 ? (size_t)splits * M * N * sizeof(float) : 0;
}

DCLIP_API int dclip_gemm_bf16_splitk(const void* A, const void* W, float* C, int M, int N, int K, int lda, int ldw, int ldc,
                                     int splits, void* workspace, size_t workspace_bytes, void* stream) {
  return splitk16<Bf16T>("gemm_bf16_splitk", A, W, C, M, N, K, lda, ldw, ldc, splits, workspace, workspace_bytes, stream);
}

// fp16 twins of the split-K form (training path)
DCLIP_API int dclip_gemm_f16_splitk_plan(int M, int N, int K) { return dclip_gemm_bf16_splitk_plan(M, N, K); }

DCLIP_API size_t dclip_gemm_f16_splitk_workspace(int M, int N, int splits) {
  return dclip_gemm_bf16_splitk_workspace(M, N, splits);
}

DCLIP_API int dclip_gemm_f16_splitk(const void* A, const void* W, float* C, int M, int N, int K, int lda, int ldw, int ldc,
                                    int splits, void* workspace, size_t workspace_bytes, void* stream) {
  return splitk16<F16IeeeT>("gemm_f16_splitk", A, W, C, M, N, K, lda, ldw, ldc, splits, workspace, workspace_bytes, stream);
}
