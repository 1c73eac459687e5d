// Exact top-k inner-product search on the CDNA4 matrix cores (v_mfma_f32_32x32x2_f32), and the two small kernels of the
// teacher's KNN tokenizer (in-place ReLU, threshold select).  Contract: include/dclip_hip.h; design: DESIGN.md §20.
//
// scores = database [N][P] x queries [Q][P]^T is formed tile by tile and never stored.  One workgroup (4 waves) owns a
// block of 64 queries and one contiguous split of the database, walked in tiles of 128 rows:
//   * the database tile is the MFMA's A operand and the query block its B operand, so accumulator register r of lane l
//     holds database row (r&3) + 8*(r>>2) + 4*(l>>5) of a 32-row sub-tile for query l&31: a lane owns ONE query;
//   * wave w takes queries 32*(w&1) .. +32 and the database rows 64*(w>>1) .. +64 of the tile (two accumulators);
//   * a lane keeps a sorted list of KL (score, index) pairs in registers, each pair as ONE 64-bit key whose integer order
//     is the total order (score descending, index ascending); `key > list[KL-1]` skips almost every element;
//   * rows past N and queries past Q are zero-filled in LDS and discarded BY INDEX, never by value;
//   * after the last tile the four lists of a query (two half-waves x two waves) are merged through LDS under the total
//     order (score descending, index ascending) and written as one partial list per (split, query) into the workspace.
// A second launch merges the partial lists of a query under the same order.  Every score is one fixed fmaf chain over k
// (the K loop does not depend on the split), so the result does not depend on the number of splits.  No atomics.
#include "common.h"
#include <math.h>

namespace {

constexpr int TQ = 64;        // queries per workgroup
constexpr int TD = 128;       // database rows per tile
constexpr int TK = 32;        // k per staged tile
constexpr int LDR = TK + 4;   // LDS row stride in floats: 144 B, ds_read_b128 down 16 rows touches 16 distinct 16-B slots
constexpr int MAX_SPLITS = 64;
constexpr int TARGET_WGS = 1024;   // 4 workgroups per CU on 256 CUs

struct TopkPlan {
  int qblocks, tiles, tiles_per_split, splits;
};

// A pure function of (Q, N): see the header comment of dclip_topk_ip_workspace.
TopkPlan topk_plan(int Q, int N) {
  TopkPlan pl;
  pl.qblocks = cdiv(Q, TQ);
  pl.tiles = cdiv(N, TD);
  int want = cdiv(TARGET_WGS, pl.qblocks);
  if (want > MAX_SPLITS) want = MAX_SPLITS;
  if (want > pl.tiles) want = pl.tiles;
  pl.tiles_per_split = cdiv(pl.tiles, want);
  pl.splits = cdiv(pl.tiles, pl.tiles_per_split);
  return pl;
}

// One unsigned 64-bit key per (score, index) pair whose plain integer order IS the total order (score descending, index
// ascending): the high word is the usual monotone map of a non-NaN float (-0.0 first made +0.0, so that the two zeros tie),
// the low word falls as the index rises.  Keys are unique, so no insertion or merge has a tie to break, and the result
// cannot depend on the order in which rows, half-waves or splits are met.  0 is the empty slot: a qualifying score
// (> -inf) has a non-zero high word.
typedef unsigned long long u64;

__device__ __forceinline__ u64 make_key(float s, int row) {
  unsigned b = __float_as_uint(s + 0.0f);
  b ^= (b >> 31) ? 0xffffffffu : 0x80000000u;
  return ((u64)b << 32) | (unsigned)(0x7fffffff - row);
}
__device__ __forceinline__ float key_score(u64 key) {
  if (key == 0) return -INFINITY;
  unsigned b = (unsigned)(key >> 32);
  b ^= (b >> 31) ? 0x80000000u : 0xffffffffu;
  return __uint_as_float(b);
}
__device__ __forceinline__ int key_index(u64 key) { return key == 0 ? -1 : 0x7fffffff - (int)(unsigned)key; }

// lk is sorted descending; the caller has seen key > lk[KL-1]
template <int KL>
__device__ __forceinline__ void insert_key(u64 (&lk)[KL], u64 key) {
#pragma unroll
  for (int j = KL - 1; j > 0; --j) {
    const u64 above = lk[j - 1];
    const u64 here = key > lk[j] ? key : lk[j];
    lk[j] = key > above ? above : here;       // the new key lands above slot j-1: slot j-1 moves down
  }
  lk[0] = key > lk[0] ? key : lk[0];
}

template <int KL>
__global__ void __launch_bounds__(256) topk_ip_kernel(const float* __restrict__ queries, const float* __restrict__ database,
                                                      u64* __restrict__ part, int Q, int N, int P, int k, int tiles,
                                                      int tiles_per_split) {
  constexpr int STAGE_FLOATS = (TD + TQ) * LDR;
  constexpr int LIST_FLOATS = TQ * 4 * KL * 2;   // 64-bit keys
  __shared__ __attribute__((aligned(16))) float lds[STAGE_FLOATS > LIST_FLOATS ? STAGE_FLOATS : LIST_FLOATS];
  float* As = lds;
  float* Bs = lds + TD * LDR;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, half = lane >> 5;
  const int wq = wave & 1, wd = wave >> 1;
  const int q0 = blockIdx.x * TQ;
  const int split = blockIdx.y;
  const int t_begin = split * tiles_per_split;
  const int t_end = min(t_begin + tiles_per_split, tiles);

  u64 lk[KL];
#pragma unroll
  for (int j = 0; j < KL; ++j) lk[j] = 0;

  // staging roles: float4 f = tid + 256 i  ->  row f >> 3, k = 4 (f & 7)
  const int c4 = (tid & 7) * 4;
  const int srow = tid >> 3;   // 0 .. 31

  for (int t = t_begin; t < t_end; ++t) {
    const int d0 = t * TD;
    f32x16 acc[2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;

    for (int k0 = 0; k0 < P; k0 += TK) {
      f32x4 ra[4], rb[2];
      const bool kin = k0 + c4 < P;   // P % 4 == 0: a float4 is inside or outside as a whole
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = d0 + srow + 32 * i;
        ra[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (kin && row < N) ra[i] = *(const f32x4*)(database + (size_t)row * P + k0 + c4);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int row = q0 + srow + 32 * i;
        rb[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (kin && row < Q) rb[i] = *(const f32x4*)(queries + (size_t)row * P + k0 + c4);
      }
      __syncthreads();   // the previous K-tile's reads are done
#pragma unroll
      for (int i = 0; i < 4; ++i) *(f32x4*)(As + (srow + 32 * i) * LDR + c4) = ra[i];
#pragma unroll
      for (int i = 0; i < 2; ++i) *(f32x4*)(Bs + (srow + 32 * i) * LDR + c4) = rb[i];
      __syncthreads();
      // lane half h supplies k = 8g + 4h + r to MFMA step (g, r) on both operands: any k order both sides agree on
#pragma unroll
      for (int g = 0; g < TK / 8; ++g) {
        const f32x4 fb = *(const f32x4*)(Bs + (wq * 32 + l31) * LDR + 8 * g + 4 * half);
        const f32x4 fa0 = *(const f32x4*)(As + (wd * 64 + l31) * LDR + 8 * g + 4 * half);
        const f32x4 fa1 = *(const f32x4*)(As + (wd * 64 + 32 + l31) * LDR + 8 * g + 4 * half);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa0[r], fb[r], acc[0], 0, 0, 0);
          acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa1[r], fb[r], acc[1], 0, 0, 0);
        }
      }
    }

#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = d0 + wd * 64 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        const float s = acc[a][r];
        if (row < N && s > -INFINITY) {          // false for NaN: such a row never qualifies
          const u64 key = make_key(s, row);
          if (key > lk[KL - 1]) insert_key<KL>(lk, key);
        }
      }
    }
  }

  // merge the four lists of each query through LDS (the staging space is dead behind this barrier)
  __syncthreads();
  u64* Lk = (u64*)lds;                          // [TQ][4][KL]
  {
    const int ql = wq * 32 + l31;
    const int list = wd * 2 + half;
#pragma unroll
    for (int j = 0; j < KL; ++j) Lk[(ql * 4 + list) * KL + j] = lk[j];
  }
  __syncthreads();
  if (tid < TQ && q0 + tid < Q) {
    u64 mk[KL];
#pragma unroll
    for (int j = 0; j < KL; ++j) mk[j] = Lk[(tid * 4) * KL + j];
    for (int list = 1; list < 4; ++list) {
      for (int j = 0; j < KL; ++j) {
        const u64 key = Lk[(tid * 4 + list) * KL + j];
        if (key <= mk[KL - 1]) break;           // sorted: nothing behind it can enter either (0 = empty)
        insert_key<KL>(mk, key);
      }
    }
    const size_t base = ((size_t)split * Q + (q0 + tid)) * k;
#pragma unroll
    for (int j = 0; j < KL; ++j)
      if (j < k) part[base + j] = mk[j];
  }
}

// one thread per query: merge the splits' partial lists
template <int KL>
__global__ void __launch_bounds__(256) topk_merge_kernel(const u64* __restrict__ part, float* __restrict__ scores,
                                                         int32_t* __restrict__ indices, int Q, int N, int k, int splits) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= Q) return;
  u64 mk[KL];
#pragma unroll
  for (int j = 0; j < KL; ++j) mk[j] = 0;
  for (int s = 0; s < splits; ++s) {
    const size_t base = ((size_t)s * Q + q) * k;
    for (int j = 0; j < k; ++j) {
      const u64 key = part[base + j];
      if (key <= mk[KL - 1]) break;
      insert_key<KL>(mk, key);
    }
  }
#pragma unroll
  for (int j = 0; j < KL; ++j) {
    if (j < k) {
      const int i = key_index(mk[j]);
      const bool ok = i >= 0 && i < N;          // an index outside [0, N) is never written, whatever the workspace held
      scores[(size_t)q * k + j] = ok ? key_score(mk[j]) : -INFINITY;
      indices[(size_t)q * k + j] = ok ? i : -1;
    }
  }
}

template <int KL>
void launch_topk(const float* queries, const float* database, u64* part, int Q, int N, int P, int k, const TopkPlan& pl,
                 hipStream_t st) {
  hipLaunchKernelGGL(topk_ip_kernel<KL>, dim3(pl.qblocks, pl.splits), dim3(256), 0, st, queries, database, part, Q, N, P, k,
                     pl.tiles, pl.tiles_per_split);
}

template <int KL>
void launch_merge(const u64* part, float* scores, int32_t* indices, int Q, int N, int k, int splits, hipStream_t st) {
  hipLaunchKernelGGL(topk_merge_kernel<KL>, dim3(cdiv(Q, 256)), dim3(256), 0, st, part, scores, indices, Q, N, k, splits);
}

__global__ void __launch_bounds__(256) relu_kernel(float* __restrict__ x, size_t n) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float v = x[i];
    if (v < 0.f) x[i] = 0.f;   // false for NaN and for -0.0: both stay as they are
  }
}

// one wave per row
__global__ void __launch_bounds__(256) knn_select_kernel(const float* __restrict__ sim, const int32_t* __restrict__ idx,
                                                         const float* __restrict__ database,
                                                         const float* __restrict__ fallback, float thresh,
                                                         float* __restrict__ out, int32_t* __restrict__ source, int Q, int N,
                                                         int P) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= Q) return;
  const int j = idx[row];
  const bool hit = j >= 0 && j < N && sim[row] >= thresh;   // false for a NaN similarity
  const float* src = hit ? database + (size_t)j * P : fallback + (size_t)row * P;
  for (int c = lane; c < P; c += 64) out[(size_t)row * P + c] = src[c];
  if (lane == 0) source[row] = hit ? 0 : 1;
}

}  // namespace

DCLIP_API size_t dclip_topk_ip_workspace(int Q, int N, int k) {
  if (Q <= 0 || N <= 0 || k <= 0) return 0;
  return (size_t)topk_plan(Q, N).splits * Q * k * sizeof(u64);
}

DCLIP_API int dclip_topk_ip(const float* queries, const float* database, float* scores, int32_t* indices, int Q, int N, int P,
                            int k, void* workspace, size_t workspace_bytes, void* stream) {
  DCLIP_REQUIRE(queries && database && scores && indices && workspace, "topk_ip: null pointer");
  DCLIP_REQUIRE(Q > 0 && N > 0 && P > 0 && P % 4 == 0, "topk_ip: bad shape Q=%d N=%d P=%d", Q, N, P);
  DCLIP_REQUIRE(k >= 1 && k <= 16, "topk_ip: k=%d outside 1 .. 16", k);
  DCLIP_REQUIRE((uintptr_t)workspace % 8 == 0, "topk_ip: the workspace must be 8-byte aligned");
  const TopkPlan pl = topk_plan(Q, N);
  const size_t entries = (size_t)pl.splits * Q * k;
  if (workspace_bytes < entries * sizeof(u64)) {
    dclip_set_error("topk_ip: workspace too small");
    return DCLIP_EWORKSPACE;
  }
  u64* part = (u64*)workspace;
  hipStream_t st = (hipStream_t)stream;
  if (k == 1) launch_topk<1>(queries, database, part, Q, N, P, k, pl, st);
  else if (k <= 4) launch_topk<4>(queries, database, part, Q, N, P, k, pl, st);
  else if (k <= 8) launch_topk<8>(queries, database, part, Q, N, P, k, pl, st);
  else launch_topk<16>(queries, database, part, Q, N, P, k, pl, st);
  DCLIP_CHECK_LAUNCH("topk_ip");
  if (k == 1) launch_merge<1>(part, scores, indices, Q, N, k, pl.splits, st);
  else if (k <= 4) launch_merge<4>(part, scores, indices, Q, N, k, pl.splits, st);
  else if (k <= 8) launch_merge<8>(part, scores, indices, Q, N, k, pl.splits, st);
  else launch_merge<16>(part, scores, indices, Q, N, k, pl.splits, st);
  DCLIP_CHECK_LAUNCH("topk_ip.merge");
  return DCLIP_OK;
}

DCLIP_API int dclip_relu_f32(float* x, size_t n, void* stream) {
  DCLIP_REQUIRE(x && n > 0, "relu_f32: bad arguments");
  size_t blocks = cdivz(n, 256);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(relu_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, n);
  DCLIP_CHECK_LAUNCH("relu_f32");
  return DCLIP_OK;
}

DCLIP_API int dclip_knn_select(const float* sim, const int32_t* idx, const float* database, const float* fallback, float thresh,
                               float* out, int32_t* source, int Q, int N, int P, void* stream) {
  DCLIP_REQUIRE(sim && idx && database && fallback && out && source, "knn_select: null pointer");
  DCLIP_REQUIRE(Q > 0 && N > 0 && P > 0, "knn_select: bad shape Q=%d N=%d P=%d", Q, N, P);
  hipLaunchKernelGGL(knn_select_kernel, dim3(cdiv(Q, 4)), dim3(256), 0, (hipStream_t)stream, sim, idx, database, fallback,
                     thresh, out, source, Q, N, P);
  DCLIP_CHECK_LAUNCH("knn_select");
  return DCLIP_OK;
}
