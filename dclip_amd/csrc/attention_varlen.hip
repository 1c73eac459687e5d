// Self-attention over a PACKED batch of sequences of different lengths: the frozen vision tower run on all
// region crops of a batch at their own sizes in one pass.  Forward only, fp32, non-causal.  Below it the causal twin for the
// text tower on packed captions and that twin's backward for the trainable tower.
//
// qkv [T][3*H*64] holds N sequences back to back, sequence n in rows cu[n] .. cu[n+1]-1.  The kernel is the tiled forward of
// attention.hip (attn_fwd_kernel: a 64-query tile per workgroup, 64-key tiles streamed with the online softmax, P in the
// wave's own Q rows) with b*S replaced by cu[n] and S by cu[n+1] - cu[n]; the tile helpers are shared (attention_tiles.h).
// Rows past a sequence's end are fetched from that sequence's LAST row and zeroed on commit (tile_fetch / tile_commit), so
// no lane ever holds a value of the neighbouring sequence.
#include "common.h"
#include "attention_tiles.h"

namespace {

// grid (N*H, query tiles).  CLS: only row 0 of each sequence is a query (the last layer's pruned schedule): out [N][H*64],
// lse [H][N]; otherwise out [T][H*64], lse [H][T].  T = cu[N]; every cu entry is clamped into [0, T] and made non-decreasing
// here, so a malformed table cannot send a load or a store past the T rows the caller allocated.
// SPLIT (2 / 3, every row a query): `out` is the fp16 split of so.scale * context, [T][so.ldy], and lse is not written
// (SplitOut, attention_tiles.h).
template <bool CLS, int SPLIT = 0, typename... SO>
__global__ void __launch_bounds__(256) attn_varlen_fwd_kernel(const float* __restrict__ qkv, const int32_t* __restrict__ cu,
                                                              float* __restrict__ out, float* __restrict__ lse, int N, int H,
                                                              SO... so_) {
  static_assert(!SPLIT || !CLS, "the one-row form stays fp32");
  static_assert(sizeof...(SO) == (SPLIT ? 1 : 0), "a SplitOut argument exactly for the SPLIT instances");
  const SplitOut so = split_out(so_...);
  const int n = blockIdx.x / H, h = blockIdx.x % H;
  const int T = cu[N];
  const int s0 = min(max(cu[n], 0), T);
  const int S = min(max(cu[n + 1], s0), T) - s0;
  const int Sq = CLS ? min(S, 1) : S;
  const int q0 = blockIdx.y * TS;
  if (q0 >= Sq) return;                                    // uniform over the workgroup, before any barrier

  __shared__ __attribute__((aligned(16))) float lds[3 * TS * HD];
  float* Qs = lds;
  float* Ks = lds + TS * HD;
  float* Vs = lds + 2 * TS * HD;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int qd = lane >> 4, l15 = lane & 15;
  const int D = H * HD;
  const size_t ld = (size_t)3 * D;
  const float* qbase = qkv + (size_t)s0 * ld + h * HD;
  const float* kbase = qbase + D;
  const float* vbase = qbase + 2 * D;

  {
    f32x4 vq[4], vk[4], vv[4];
    tile_fetch(vq, qbase, q0, Sq, ld);
    tile_fetch(vk, kbase, 0, S, ld);
    tile_fetch(vv, vbase, 0, S, ld);
    tile_commit(Qs, vq, q0, Sq);
    tile_commit(Ks, vk, 0, S);
    tile_commit(Vs, vv, 0, S);
  }
  __syncthreads();
  f32x4 qf[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) qf[g] = frag_k(Qs, 16 * wave, g, lane);

  float m[4], l[4];
  f32x4 o[4];
  zero4(o);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    m[r] = -INFINITY;
    l[r] = 0.f;
  }
  const int nkt = (S + TS - 1) / TS;
  for (int kt = 0; kt < nkt; ++kt) {
    if (kt > 0) {
      __syncthreads();  // everyone is done with the previous K/V tile
      stage_tiles2(Ks, kbase, ld, Vs, vbase, ld, kt * TS, S);
      __syncthreads();
    }
    f32x4 s[4];
    zero4(s);
    mma_rows_x_tileT(s, qf, Ks, lane);
    float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const int key = kt * TS + nt * 16 + l15;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = s[nt][r] * kScale;
        if (key >= S) v = -INFINITY;
        s[nt][r] = v;
        mx[r] = fmaxf(mx[r], v);
      }
    }
    float alpha[4], rs[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float mn = fmaxf(m[r], quarter_max(mx[r]));
      const float msafe = (mn == -INFINITY) ? 0.f : mn;
      alpha[r] = __expf(m[r] - msafe);  // m = -inf -> 0
      m[r] = mn;
      rs[r] = 0.f;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        float p = __expf(s[nt][r] - msafe);
        s[nt][r] = p;
        rs[r] += p;
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      l[r] = l[r] * alpha[r] + quarter_sum(rs[r]);
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        o[nt][r] *= alpha[r];
        Qs[tile_off(16 * wave + 4 * qd + r, nt * 16 + l15)] = s[nt][r];   // this wave's private rows
      }
    }
    mma_tilerows_x_tile(o, Qs, 16 * wave, Vs, lane);
  }
  const size_t orow0 = CLS ? (size_t)n : (size_t)s0;       // first output row of this sequence
  const size_t lse_ld = CLS ? (size_t)N : (size_t)T;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = q0 + 16 * wave + 4 * qd + r;
    if (row < Sq) {
      const float inv = 1.0f / l[r];
      if constexpr (SPLIT != 0) {
        unsigned short* yrow = reinterpret_cast<unsigned short*>(out) + (orow0 + row) * so.ldy + h * HD + l15;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) split_store1<SPLIT>(yrow + nt * 16, D, o[nt][r] * inv, so.scale);
      } else {
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) out[(orow0 + row) * D + h * HD + nt * 16 + l15] = o[nt][r] * inv;
      if (lse && l15 == 0) lse[(size_t)h * lse_ld + orow0 + row] = m[r] + __logf(l[r]);
      }
    }
  }
}

// The CAUSAL twin: the frozen text tower on packed captions, caption n in rows cu[n] .. cu[n+1]-1 (its first
// EOS is the last of them).  attn_fwd_kernel<true> of attention.hip with b*S replaced by cu[n]: query row i sees keys 0..i of
// its own sequence, key tiles beyond the query tile are not visited.  grid (N*H, query tiles).  LAST: the only query is the
// LAST row of each sequence, which sees all of its keys (the ragged twin of the one-row kernel behind dclip_attention_row_fwd):
// out [N][H*64], lse [H][N], grid (N*H, 1); otherwise out [T][H*64], lse [H][T].  The table is clamped as above.
// SPLIT: as in attn_varlen_fwd_kernel.
template <bool LAST, int SPLIT = 0, typename... SO>
__global__ void __launch_bounds__(256) attn_varlen_causal_fwd_kernel(const float* __restrict__ qkv, const int32_t* __restrict__ cu,
                                                                     float* __restrict__ out, float* __restrict__ lse, int N,
                                                                     int H, SO... so_) {
  static_assert(!SPLIT || !LAST, "the one-row form stays fp32");
  static_assert(sizeof...(SO) == (SPLIT ? 1 : 0), "a SplitOut argument exactly for the SPLIT instances");
  const SplitOut so = split_out(so_...);
  const int n = blockIdx.x / H, h = blockIdx.x % H;
  const int T = cu[N];
  const int s0 = min(max(cu[n], 0), T);
  const int S = min(max(cu[n + 1], s0), T) - s0;
  const int Sq = LAST ? min(S, 1) : S;                     // LAST: one query row, at sequence position S - 1
  const int q0 = blockIdx.y * TS;
  if (q0 >= Sq) return;                                    // uniform over the workgroup, before any barrier

  __shared__ __attribute__((aligned(16))) float lds[3 * TS * HD];
  float* Qs = lds;
  float* Ks = lds + TS * HD;
  float* Vs = lds + 2 * TS * HD;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int qd = lane >> 4, l15 = lane & 15;
  const int D = H * HD;
  const size_t ld = (size_t)3 * D;
  const float* kbase = qkv + (size_t)s0 * ld + h * HD + D;
  const float* vbase = kbase + D;
  const float* qbase = kbase - D + (LAST ? (size_t)(S - 1) * ld : (size_t)0);

  {
    f32x4 vq[4], vk[4], vv[4];
    tile_fetch(vq, qbase, q0, Sq, ld);
    tile_fetch(vk, kbase, 0, S, ld);
    tile_fetch(vv, vbase, 0, S, ld);
    tile_commit(Qs, vq, q0, Sq);
    tile_commit(Ks, vk, 0, S);
    tile_commit(Vs, vv, 0, S);
  }
  __syncthreads();
  f32x4 qf[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) qf[g] = frag_k(Qs, 16 * wave, g, lane);

  float m[4], l[4];
  f32x4 o[4];
  zero4(o);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    m[r] = -INFINITY;
    l[r] = 0.f;
  }
  int nkt = (S + TS - 1) / TS;
  if (!LAST) nkt = min(nkt, (int)blockIdx.y + 1);          // key tiles beyond the query tile are fully masked
  for (int kt = 0; kt < nkt; ++kt) {
    if (kt > 0) {
      __syncthreads();  // everyone is done with the previous K/V tile
      stage_tiles2(Ks, kbase, ld, Vs, vbase, ld, kt * TS, S);
      __syncthreads();
    }
    f32x4 s[4];
    zero4(s);
    mma_rows_x_tileT(s, qf, Ks, lane);
    float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const int key = kt * TS + nt * 16 + l15;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qrow = q0 + 16 * wave + 4 * qd + r;
        float v = s[nt][r] * kScale;
        if (key >= S || (!LAST && key > qrow)) v = -INFINITY;
        s[nt][r] = v;
        mx[r] = fmaxf(mx[r], v);
      }
    }
    float alpha[4], rs[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float mn = fmaxf(m[r], quarter_max(mx[r]));
      const float msafe = (mn == -INFINITY) ? 0.f : mn;
      alpha[r] = __expf(m[r] - msafe);  // m = -inf -> 0
      m[r] = mn;
      rs[r] = 0.f;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        float p = __expf(s[nt][r] - msafe);
        s[nt][r] = p;
        rs[r] += p;
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      l[r] = l[r] * alpha[r] + quarter_sum(rs[r]);
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        o[nt][r] *= alpha[r];
        Qs[tile_off(16 * wave + 4 * qd + r, nt * 16 + l15)] = s[nt][r];   // this wave's private rows
      }
    }
    mma_tilerows_x_tile(o, Qs, 16 * wave, Vs, lane);
  }
  const size_t orow0 = LAST ? (size_t)n : (size_t)s0;      // first output row of this sequence
  const size_t lse_ld = LAST ? (size_t)N : (size_t)T;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = q0 + 16 * wave + 4 * qd + r;
    if (row < Sq) {
      const float inv = 1.0f / l[r];
      if constexpr (SPLIT != 0) {
        unsigned short* yrow = reinterpret_cast<unsigned short*>(out) + (orow0 + row) * so.ldy + h * HD + l15;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) split_store1<SPLIT>(yrow + nt * 16, D, o[nt][r] * inv, so.scale);
      } else {
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) out[(orow0 + row) * D + h * HD + nt * 16 + l15] = o[nt][r] * inv;
      if (lse && l15 == 0) lse[(size_t)h * lse_ld + orow0 + row] = m[r] + __logf(l[r]);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------- causal backward
// The trainable text tower on packed captions.  attn_bwd_dq_kernel<true> / attn_bwd_dkv_kernel<true> of attention.hip with
// b*S replaced by cu[n] and lse / delta indexed [h][cu[n] + row]; q / k / v are the three column blocks of qkv, dq / dk / dv
// those of dqkv (row stride 3 D).  Every tile is staged by stage_tiles2 (rows past the sequence's end are fetched from its
// LAST row and zeroed on commit), so no lane holds a value of the neighbouring caption.  grid (N*H, cdiv(max_S, 64)); the
// table is clamped as in the forward.  A workgroup whose tile starts at or past its sequence's length returns before any
// barrier (a sequence of length 0 writes nothing).  A sequence of ONE row: the softmax is identically 1, so dq = dk = 0 and
// dv = dout exactly (attn_bwd_one_key_kernel's result) — a branch uniform over the workgroup, dq here, dk / dv in the dkv
// kernel.  No atomics: the same bits in every run.
//
// dQ for query tile blockIdx.y over key tiles 0 .. blockIdx.y; also writes delta[h][cu[n] + row] = sum_d dO * O.
__global__ void __launch_bounds__(256) attn_varlen_causal_bwd_dq_kernel(const float* __restrict__ qkv, const int32_t* __restrict__ cu,
                                                                        const float* __restrict__ out, const float* __restrict__ dout,
                                                                        const float* __restrict__ lse, float* __restrict__ dqkv,
                                                                        float* __restrict__ delta, int N, int H) {
  const int n = blockIdx.x / H, h = blockIdx.x % H;
  const int T = cu[N];
  const int s0 = min(max(cu[n], 0), T);
  const int S = min(max(cu[n + 1], s0), T) - s0;
  const int q0 = blockIdx.y * TS;
  if (q0 >= S) return;                                     // uniform over the workgroup, before any barrier
  const int D = H * HD;
  const size_t ld = (size_t)3 * D;
  float* dqbase = dqkv + (size_t)s0 * ld + h * HD;
  if (S == 1) {                                            // uniform: one key, dq is exactly zero
    if (threadIdx.x < HD) dqbase[threadIdx.x] = 0.f;
    return;
  }
  __shared__ __attribute__((aligned(16))) float t0[TS * HD];
  __shared__ __attribute__((aligned(16))) float t1[TS * HD];
  __shared__ __attribute__((aligned(16))) float scratch[4 * 16 * SCR];
  __shared__ float dl_s[TS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int qd = lane >> 4, l15 = lane & 15;
  const float* qbase = qkv + (size_t)s0 * ld + h * HD;
  const float* kbase = qbase + D;
  const float* vbase = qbase + 2 * D;
  const float* obase = out + (size_t)s0 * D + h * HD;
  const float* dobase = dout + (size_t)s0 * D + h * HD;
  const float* lse_n = lse + (size_t)h * T + s0;
  float* delta_n = delta + (size_t)h * T + s0;
  float* scr = scratch + wave * 16 * SCR;

  {  // delta: 4 threads per row, 16 floats each
    const int row = threadIdx.x >> 2, part = threadIdx.x & 3;
    float s = 0.f;
    if (q0 + row < S) {
      const f32x4* po = reinterpret_cast<const f32x4*>(obase + (size_t)(q0 + row) * D + part * 16);
      const f32x4* pd = reinterpret_cast<const f32x4*>(dobase + (size_t)(q0 + row) * D + part * 16);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        f32x4 a = po[i], c = pd[i];
        s += (a[0] * c[0] + a[1] * c[1]) + (a[2] * c[2] + a[3] * c[3]);
      }
    }
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    if (part == 0) {
      dl_s[row] = s;
      if (q0 + row < S) delta_n[q0 + row] = s;
    }
  }
  stage_tiles2(t0, qbase, ld, t1, dobase, (size_t)D, q0, S);
  __syncthreads();
  f32x4 qf[4], dof[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    qf[g] = frag_k(t0, 16 * wave, g, lane);
    dof[g] = frag_k(t1, 16 * wave, g, lane);
  }
  float lse_r[4], dl[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = q0 + 16 * wave + 4 * qd + r;
    lse_r[r] = (row < S) ? lse_n[row] : 0.f;
    dl[r] = dl_s[16 * wave + 4 * qd + r];
  }
  f32x4 dq[4];
  zero4(dq);
  const int nkt = (int)blockIdx.y + 1;                     // q0 < S: key tiles 0 .. blockIdx.y all start inside the sequence
  for (int kt = 0; kt < nkt; ++kt) {
    __syncthreads();
    stage_tiles2(t0, kbase, ld, t1, vbase, ld, kt * TS, S);
    __syncthreads();
    f32x4 s[4], dp[4];
    zero4(s);
    zero4(dp);
    mma_rows_x_tileT(s, qf, t0, lane);
    mma_rows_x_tileT(dp, dof, t1, lane);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const int key = kt * TS + nt * 16 + l15;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qrow = q0 + 16 * wave + 4 * qd + r;
        const bool masked = key >= S || key > qrow;
        const float p = masked ? 0.f : __expf(s[nt][r] * kScale - lse_r[r]);
        scr[(4 * qd + r) * SCR + nt * 16 + l15] = p * (dp[nt][r] - dl[r]) * kScale;
      }
    }
    __syncthreads();
    mma_scratch_x_tile(dq, scr, t0, lane);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = q0 + 16 * wave + 4 * qd + r;
    if (row < S)
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) dqbase[(size_t)row * ld + nt * 16 + l15] = dq[nt][r];
  }
}

// dK, dV for key tile blockIdx.y over query tiles blockIdx.y .. ; reads the delta the dQ kernel left.
__global__ void __launch_bounds__(256) attn_varlen_causal_bwd_dkv_kernel(const float* __restrict__ qkv, const int32_t* __restrict__ cu,
                                                                         const float* __restrict__ dout, const float* __restrict__ lse,
                                                                         const float* __restrict__ delta, float* __restrict__ dqkv,
                                                                         int N, int H) {
  const int n = blockIdx.x / H, h = blockIdx.x % H;
  const int T = cu[N];
  const int s0 = min(max(cu[n], 0), T);
  const int S = min(max(cu[n + 1], s0), T) - s0;
  const int k0 = blockIdx.y * TS;
  if (k0 >= S) return;                                     // uniform over the workgroup, before any barrier
  const int D = H * HD;
  const size_t ld = (size_t)3 * D;
  const float* dobase = dout + (size_t)s0 * D + h * HD;
  float* dkbase = dqkv + (size_t)s0 * ld + h * HD + D;
  float* dvbase = dkbase + D;
  if (S == 1) {                                            // uniform: one key, dk is exactly zero and dv is dout itself
    if (threadIdx.x < HD) {
      dkbase[threadIdx.x] = 0.f;
      dvbase[threadIdx.x] = dobase[threadIdx.x];
    }
    return;
  }
  __shared__ __attribute__((aligned(16))) float t0[TS * HD];
  __shared__ __attribute__((aligned(16))) float t1[TS * HD];
  __shared__ __attribute__((aligned(16))) float scratch_p[4 * 16 * SCR];
  __shared__ __attribute__((aligned(16))) float scratch_s[4 * 16 * SCR];
  __shared__ float lse_s[TS], dl_s[TS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int qd = lane >> 4, l15 = lane & 15;
  const float* qbase = qkv + (size_t)s0 * ld + h * HD;
  const float* kbase = qbase + D;
  const float* vbase = qbase + 2 * D;
  const float* lse_n = lse + (size_t)h * T + s0;
  const float* delta_n = delta + (size_t)h * T + s0;
  float* scp = scratch_p + wave * 16 * SCR;
  float* scs = scratch_s + wave * 16 * SCR;

  stage_tiles2(t0, kbase, ld, t1, vbase, ld, k0, S);
  __syncthreads();
  f32x4 kf[4], vf[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    kf[g] = frag_k(t0, 16 * wave, g, lane);
    vf[g] = frag_k(t1, 16 * wave, g, lane);
  }
  f32x4 dk[4], dv[4];
  zero4(dk);
  zero4(dv);
  const int nqt = (S + TS - 1) / TS;
  for (int qt = (int)blockIdx.y; qt < nqt; ++qt) {
    const int q0 = qt * TS;
    __syncthreads();
    stage_tiles2(t0, qbase, ld, t1, dobase, (size_t)D, q0, S);
    if (threadIdx.x < TS) {
      const int q = q0 + threadIdx.x;
      lse_s[threadIdx.x] = (q < S) ? lse_n[q] : 0.f;
      dl_s[threadIdx.x] = (q < S) ? delta_n[q] : 0.f;
    }
    __syncthreads();
    f32x4 st[4], dpt[4];
    zero4(st);
    zero4(dpt);
    mma_rows_x_tileT(st, kf, t0, lane);    // [key, q] = K Q^T
    mma_rows_x_tileT(dpt, vf, t1, lane);   // [key, q] = V dO^T
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const int ql = nt * 16 + l15, q = q0 + ql;
      const float lq = lse_s[ql], dq_ = dl_s[ql];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = k0 + 16 * wave + 4 * qd + r;
        const bool masked = key >= S || q >= S || key > q;
        const float p = masked ? 0.f : __expf(st[nt][r] * kScale - lq);
        scp[(4 * qd + r) * SCR + ql] = p;
        scs[(4 * qd + r) * SCR + ql] = p * (dpt[nt][r] - dq_) * kScale;
      }
    }
    __syncthreads();
    mma_scratch_x_tile(dv, scp, t1, lane);  // dV += P^T dO
    mma_scratch_x_tile(dk, scs, t0, lane);  // dK += dS^T Q
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int key = k0 + 16 * wave + 4 * qd + r;
    if (key < S)
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        dkbase[(size_t)key * ld + nt * 16 + l15] = dk[nt][r];
        dvbase[(size_t)key * ld + nt * 16 + l15] = dv[nt][r];
      }
  }
}

}  // namespace

DCLIP_API int dclip_attention_varlen_causal_bwd(const float* qkv, const int32_t* cu_seqlens, const float* out, const float* dout,
                                                const float* lse, float* dqkv, float* delta, int N, int max_S, int H,
                                                void* stream) {
  DCLIP_REQUIRE(qkv && cu_seqlens && out && dout && lse && dqkv && delta, "attention_varlen_causal_bwd: null pointer");
  DCLIP_REQUIRE(N > 0 && max_S > 0 && H > 0 && (long long)N * H < (1ll << 31),
                "attention_varlen_causal_bwd: bad shape N=%d max_S=%d H=%d", N, max_S, H);
  DCLIP_REQUIRE(((uintptr_t)qkv | (uintptr_t)out | (uintptr_t)dout | (uintptr_t)dqkv) % 16 == 0 &&
                    ((uintptr_t)cu_seqlens | (uintptr_t)lse | (uintptr_t)delta) % 4 == 0,
                "attention_varlen_causal_bwd: qkv / out / dout / dqkv must be 16-byte aligned, cu_seqlens / lse / delta 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(N * H, cdiv(max_S, TS));
  hipLaunchKernelGGL(attn_varlen_causal_bwd_dq_kernel, grid, dim3(256), 0, st, qkv, cu_seqlens, out, dout, lse, dqkv, delta, N, H);
  hipLaunchKernelGGL(attn_varlen_causal_bwd_dkv_kernel, grid, dim3(256), 0, st, qkv, cu_seqlens, dout, lse, delta, dqkv, N, H);
  DCLIP_CHECK_LAUNCH("attention_varlen_causal_bwd");
  return DCLIP_OK;
}

DCLIP_API int dclip_attention_varlen_fwd(const float* qkv, const int32_t* cu_seqlens, float* out, float* lse, int N, int max_S,
                                         int H, int cls_only, void* stream) {
  DCLIP_REQUIRE(qkv && cu_seqlens && out, "attention_varlen_fwd: null pointer");
  DCLIP_REQUIRE(N > 0 && max_S > 0 && H > 0 && (long long)N * H < (1ll << 31),
                "attention_varlen_fwd: bad shape N=%d max_S=%d H=%d", N, max_S, H);
  DCLIP_REQUIRE(((uintptr_t)qkv | (uintptr_t)out) % 16 == 0 && ((uintptr_t)cu_seqlens | (uintptr_t)lse) % 4 == 0,
                "attention_varlen_fwd: qkv / out must be 16-byte aligned, cu_seqlens / lse 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (cls_only)
    hipLaunchKernelGGL((attn_varlen_fwd_kernel<true>), dim3(N * H, 1), dim3(256), 0, st, qkv, cu_seqlens, out, lse, N, H);
  else
    hipLaunchKernelGGL((attn_varlen_fwd_kernel<false>), dim3(N * H, cdiv(max_S, TS)), dim3(256), 0, st, qkv, cu_seqlens, out, lse,
                       N, H);
  DCLIP_CHECK_LAUNCH("attention_varlen_fwd");
  return DCLIP_OK;
}

DCLIP_API int dclip_attention_varlen_causal_fwd(const float* qkv, const int32_t* cu_seqlens, float* out, float* lse, int N,
                                                int max_S, int H, int last_only, void* stream) {
  DCLIP_REQUIRE(qkv && cu_seqlens && out, "attention_varlen_causal_fwd: null pointer");
  DCLIP_REQUIRE(N > 0 && max_S > 0 && H > 0 && (long long)N * H < (1ll << 31),
                "attention_varlen_causal_fwd: bad shape N=%d max_S=%d H=%d", N, max_S, H);
  DCLIP_REQUIRE(((uintptr_t)qkv | (uintptr_t)out) % 16 == 0 && ((uintptr_t)cu_seqlens | (uintptr_t)lse) % 4 == 0,
                "attention_varlen_causal_fwd: qkv / out must be 16-byte aligned, cu_seqlens / lse 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (last_only)
    hipLaunchKernelGGL((attn_varlen_causal_fwd_kernel<true>), dim3(N * H, 1), dim3(256), 0, st, qkv, cu_seqlens, out, lse, N, H);
  else
    hipLaunchKernelGGL((attn_varlen_causal_fwd_kernel<false>), dim3(N * H, cdiv(max_S, TS)), dim3(256), 0, st, qkv, cu_seqlens,
                       out, lse, N, H);
  DCLIP_CHECK_LAUNCH("attention_varlen_causal_fwd");
  return DCLIP_OK;
}

// The two entries above (every row a query) writing the context ALREADY SPLIT: y fp16 [T][ldy >= pieces H 64] =
// [hi|lo] (pieces 2) or [hi|lo|hi] (3) of scale * context, bit-equal to the fp32 entry followed by dclip_split_f32_f16x2 /
// _f16x3(order 0); columns past pieces H 64 of a row are not written; no lse.
DCLIP_API int dclip_attention_varlen_fwd_f16x2(const float* qkv, const int32_t* cu_seqlens, void* y, int N, int max_S, int H,
                                               int causal, float scale, int pieces, int ldy, void* stream) {
  DCLIP_REQUIRE(qkv && cu_seqlens && y, "attention_varlen_fwd_f16x2: null pointer");
  DCLIP_REQUIRE(N > 0 && max_S > 0 && H > 0 && (long long)N * H < (1ll << 31),
                "attention_varlen_fwd_f16x2: bad shape N=%d max_S=%d H=%d", N, max_S, H);
  DCLIP_REQUIRE(pieces == 2 || pieces == 3, "attention_varlen_fwd_f16x2: pieces is 2 ([hi|lo]) or 3 ([hi|lo|hi])");
  DCLIP_REQUIRE(ldy > 0 && (long)ldy >= (long)pieces * H * HD, "attention_varlen_fwd_f16x2: ldy >= pieces H 64");
  DCLIP_REQUIRE((uintptr_t)qkv % 16 == 0 && (uintptr_t)cu_seqlens % 4 == 0 && (uintptr_t)y % 2 == 0,
                "attention_varlen_fwd_f16x2: qkv must be 16-byte, cu_seqlens 4-byte, y 2-byte aligned");
  DCLIP_REQUIRE(scale > 0.f && scale - scale == 0.f && (__builtin_bit_cast(unsigned int, scale) & 0x007fffffu) == 0,
                "attention_varlen_fwd_f16x2: scale must be a power of two");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(N * H, cdiv(max_S, TS));
  float* out = reinterpret_cast<float*>(y);                       // re-typed inside the kernel
  const SplitOut so{scale, ldy};
#define VARLEN_SPLIT(KERNEL, P) \
  hipLaunchKernelGGL((KERNEL<false, P, SplitOut>), grid, dim3(256), 0, st, qkv, cu_seqlens, out, (float*)nullptr, N, H, so)
  if (causal) {
    if (pieces == 2) VARLEN_SPLIT(attn_varlen_causal_fwd_kernel, 2);
    else VARLEN_SPLIT(attn_varlen_causal_fwd_kernel, 3);
  } else {
    if (pieces == 2) VARLEN_SPLIT(attn_varlen_fwd_kernel, 2);
    else VARLEN_SPLIT(attn_varlen_fwd_kernel, 3);
  }
#undef VARLEN_SPLIT
  DCLIP_CHECK_LAUNCH_V("attention_varlen_fwd_f16x2", causal ? ".causal" : ".full");
  return DCLIP_OK;
}
