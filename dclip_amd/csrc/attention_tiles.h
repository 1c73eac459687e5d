// Tile helpers of the fp32 attention kernels (head_dim 64, v_mfma_f32_16x16x4_f32): the swizzled LDS image of a
// [64 rows][64 floats] tile, its staging from global memory and the MFMA products over it.  Shared by attention.hip
// and attention_varlen.hip; the layout is described at the top of attention.hip.
#pragma once
#include "common.h"

namespace {

constexpr int TS = 64;       // tile rows
constexpr int HD = 64;       // head dim
constexpr int SCR = 68;      // scratch row stride (floats)
constexpr float kScale = 0.125f;  // 64^-0.5

__device__ __forceinline__ int tile_off(int row, int col) {
  return row * HD + ((((col >> 2) ^ (row & 15)) << 2) | (col & 3));
}

// global rows [row0, row0+64) x 64 floats (row stride ld) -> swizzled LDS tile; rows >= nrows are zero.  In two steps so
// that the loads of SEVERAL tiles go out together: tile_fetch issues a thread's four 16-byte loads UNCONDITIONALLY (rows
// past the end read row nrows-1 and are zeroed in tile_commit) — a load under a per-row condition is waited for on its
// own, which made the staging of a workgroup 4 (per tile) serial round trips to memory.
__device__ __forceinline__ void tile_fetch(f32x4 (&v)[4], const float* __restrict__ g, int row0, int nrows, size_t ld) {
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int id = threadIdx.x + c * 256;
    const int row = min(row0 + (id >> 4), nrows - 1), slot = id & 15;
    v[c] = *reinterpret_cast<const f32x4*>(g + (size_t)row * ld + slot * 4);
  }
}
__device__ __forceinline__ void tile_commit(float* tile, f32x4 (&v)[4], int row0, int nrows) {
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int id = threadIdx.x + c * 256;
    const int row = id >> 4, slot = id & 15;
    if (row0 + row >= nrows) v[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    *reinterpret_cast<f32x4*>(tile + row * HD + ((slot ^ (row & 15)) << 2)) = v[c];
  }
}
__device__ __forceinline__ void stage_tile(float* tile, const float* __restrict__ g, int row0, int nrows, size_t ld) {
  f32x4 v[4];
  tile_fetch(v, g, row0, nrows, ld);
  tile_commit(tile, v, row0, nrows);
}
// two tiles over the same rows (K and V, Q and dO): eight loads in flight
__device__ __forceinline__ void stage_tiles2(float* ta, const float* __restrict__ ga, size_t lda, float* tb,
                                             const float* __restrict__ gb, size_t ldb, int row0, int nrows) {
  f32x4 va[4], vb[4];
  tile_fetch(va, ga, row0, nrows, lda);
  tile_fetch(vb, gb, row0, nrows, ldb);
  tile_commit(ta, va, row0, nrows);
  tile_commit(tb, vb, row0, nrows);
}

// fragment for rows [rbase, rbase+16): contraction group g
__device__ __forceinline__ f32x4 frag_k(const float* tile, int rbase, int g, int lane) {
  int row = rbase + (lane & 15);
  int slot = 4 * g + (lane >> 4);
  return *reinterpret_cast<const f32x4*>(tile + row * HD + ((slot ^ (row & 15)) << 2));
}

// acc[nt] (16 x 16 each) += A_rows(16 x 64 via regs af[g]) * T^T where T tile rows are the output columns
__device__ __forceinline__ void mma_rows_x_tileT(f32x4 (&acc)[4], const f32x4 (&af)[4], const float* tile, int lane) {
#pragma unroll
  for (int nt = 0; nt < 4; ++nt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      f32x4 bf = frag_k(tile, 16 * nt, g, lane);
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[g][r], bf[r], acc[nt], 0, 0, 0);
    }
}

// acc[nt] (16 x 16 over columns 16nt..) += P(16 x 64, per-wave scratch) * T (64 x 64 tile, row = contraction)
__device__ __forceinline__ void mma_scratch_x_tile(f32x4 (&acc)[4], const float* scr, const float* tile, int lane) {
  const int qd = lane >> 4, l15 = lane & 15;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    f32x4 pf = *reinterpret_cast<const f32x4*>(scr + l15 * SCR + 16 * g + 4 * qd);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float b = tile[tile_off(16 * g + 4 * qd + r, 16 * nt + l15)];
        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(pf[r], b, acc[nt], 0, 0, 0);
      }
  }
}

// acc[nt] += A[rbase + (lane&15)][k] * B[k][16nt + (lane&15)], A by rows of a swizzled tile, B a swizzled tile
__device__ __forceinline__ void mma_tilerows_x_tile(f32x4 (&acc)[4], const float* atile, int rbase, const float* btile,
                                                    int lane) {
  const int qd = lane >> 4, l15 = lane & 15;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    f32x4 af = frag_k(atile, rbase, g, lane);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[r], btile[tile_off(16 * g + 4 * qd + r, 16 * nt + l15)], acc[nt], 0,
                                                       0, 0);
  }
}

// The forward instances that write their context ALREADY SPLIT (template parameter SPLIT = pieces): `out` is
// then fp16 [rows][ldy >= SPLIT D] = [hi|lo] (2) or [hi|lo|hi] (3) of scale * context — split1 on the fp32 value the SPLIT = 0
// instance would have stored, so the result is bit-equal to that instance followed by the stand-alone split pass — and no lse
// is written.  The argument is a trailing parameter pack of the kernel, empty for SPLIT = 0: those instances keep their
// signature, and their code is what it was without the parameter.
struct SplitOut {
  float scale;
  int ldy;
};
__device__ __forceinline__ SplitOut split_out() { return SplitOut{1.f, 0}; }
__device__ __forceinline__ SplitOut split_out(SplitOut so) { return so; }

typedef unsigned short u16x4s __attribute__((ext_vector_type(4)));

// four consecutive columns of a row: one 8-byte store per piece.  yr = the hi piece's address, D = columns per piece.
template <int SPLIT>
__device__ __forceinline__ void split_store4(unsigned short* yr, int D, const f32x4& c, float scale) {
  u16x4s hi, lo;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    unsigned short h, l;
    split1(c[e] * scale, h, l);
    hi[e] = h, lo[e] = l;
  }
  *reinterpret_cast<u16x4s*>(yr) = hi;
  *reinterpret_cast<u16x4s*>(yr + D) = lo;
  if (SPLIT == 3) *reinterpret_cast<u16x4s*>(yr + 2 * D) = hi;
}

// one column (the tiled kernels, whose lanes own a column of 16): 2-byte stores
template <int SPLIT>
__device__ __forceinline__ void split_store1(unsigned short* yr, int D, float c, float scale) {
  unsigned short h, l;
  split1(c * scale, h, l);
  yr[0] = h;
  yr[D] = l;
  if (SPLIT == 3) yr[2 * D] = h;
}

__device__ __forceinline__ void zero4(f32x4 (&a)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) a[i] = f32x4{0.f, 0.f, 0.f, 0.f};
}

}  // namespace
