// 16-bit MFMA attention core for the PACKED frozen towers: the ragged twins of the padded tiled kernel and of
// the one-row kernel of attention_bf16.hip.  Forward only, head dim 64, bf16 and fp16 (common.h, Bf16T / F16T).
//
// qkv [T][3*H*64] 16-bit holds N sequences back to back, sequence n in rows cu[n] .. cu[n+1]-1, T = cu[N].  Every cu entry is
// clamped into [0, T] and made non-decreasing on the device (as attn_varlen_fwd_kernel does), so a malformed table cannot send
// a load or a store past the T rows the caller allocated.
//
// attn_varlen_fwd16_kernel is attn_fwd_bf16_kernel with its arithmetic kept statement for statement (S^T = K Q^T on the
// 32x32x16 MFMAs, online max / sum per lane, P rounded by T::cvt_unit, V^T through the transposing LDS read): b*S becomes
// s0 = cu[n], S becomes cu[n+1] - cu[n], the output row s0 + query.  Key rows >= S are stored to LDS as zeros WITHOUT a load,
// Q rows past the end read row S - 1 of the same sequence: no lane ever holds a value of the neighbouring sequence.
// attn_varlen_row_fwd16_kernel is attn_row_fwd_bf16_kernel under the same substitution.
#include "common.h"

namespace {

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int HD = 64;             // head dim
constexpr int KT = 64;             // keys per LDS tile
constexpr float kScale = 0.125f;   // 64^-0.5

// (the two helpers of attention_bf16.hip, repeated)
// byte offset of 16-byte granule g (0..7) of row `row` in a [rows][64] bf16 tile
__device__ __forceinline__ int gran_off(int row, int g) { return row * 128 + ((g ^ ((row >> 1) & 7)) << 4); }

__device__ __forceinline__ s16x4 lds_tr16(const unsigned char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p);
}

// grid (N*H, query tiles of 64), 128 threads: one wave per 32 queries.  out [T][H*64].
template <class T, bool CAUSAL>
__global__ void __launch_bounds__(128) attn_varlen_fwd16_kernel(const unsigned short* __restrict__ qkv,
                                                                const int32_t* __restrict__ cu,
                                                                unsigned short* __restrict__ out, int N, int H) {
  typedef typename T::x8 V8;
  const int n = blockIdx.x / H, h = blockIdx.x % H;
  const int Tt = cu[N];
  const int s0 = min(max(cu[n], 0), Tt);
  const int S = min(max(cu[n + 1], s0), Tt) - s0;
  if ((int)(blockIdx.y * 64) >= S) return;                 // uniform over the workgroup, before any barrier (S = 0 too)

  __shared__ __attribute__((aligned(16))) unsigned char Ks[KT * 128];
  __shared__ __attribute__((aligned(16))) unsigned char Vs[KT * 128];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, half = lane >> 5;
  const int D = H * HD, ld = 3 * D;
  const int q0 = blockIdx.y * 64 + wave * 32;
  const int query = q0 + l31;
  const unsigned short* base = qkv + (size_t)s0 * ld + h * HD;

  // Q fragments (B operand): Q[query][16 s + 8 half .. +7]
  V8 qf[4];
  {
    const unsigned short* qrow = base + (size_t)min(query, S - 1) * ld + 8 * half;
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[s] = __builtin_bit_cast(V8, *reinterpret_cast<const u32x4*>(qrow + 16 * s));
  }
  f32x16 o[2];
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
  float m = -INFINITY, l = 0.f;

  int nkt = (S + KT - 1) / KT;
  if (CAUSAL) nkt = min(nkt, (int)(blockIdx.y * 64 + 63) / KT + 1);   // workgroup-uniform
  for (int kt = 0; kt < nkt; ++kt) {
    if (kt > 0) __syncthreads();
    // stage K and V tiles: 64 rows x 8 granules each, 128 threads -> 4 + 4 granules per thread
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int id = tid + c * 128, row = id >> 3, g = id & 7;
      const int key = kt * KT + row;
      u32x4 kv = {0u, 0u, 0u, 0u}, vv = {0u, 0u, 0u, 0u};
      if (key < S) {
        kv = *reinterpret_cast<const u32x4*>(base + (size_t)key * ld + D + g * 8);
        vv = *reinterpret_cast<const u32x4*>(base + (size_t)key * ld + 2 * D + g * 8);
      }
      *reinterpret_cast<u32x4*>(Ks + gran_off(row, g)) = kv;
      *reinterpret_cast<u32x4*>(Vs + gran_off(row, g)) = vv;
    }
    __syncthreads();
    const bool live = !CAUSAL || kt * KT <= q0 + 31;   // wave-uniform: this key tile holds keys <= some query of the wave
    if (!live) continue;

    // scores, transposed: st[sub][r] = S[query l31][key kt*64 + 32 sub + (r&3) + 8 (r>>2) + 4 half]
    f32x16 st[2];
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
      for (int r = 0; r < 16; ++r) st[sub][r] = 0.f;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const V8 kf = __builtin_bit_cast(V8, *reinterpret_cast<const u32x4*>(Ks + gran_off(32 * sub + l31, 2 * s + half)));
        st[sub] = T::mfma32(kf, qf[s], st[sub]);
      }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = kt * KT + 32 * sub + (r & 3) + 8 * (r >> 2) + 4 * half;
        float v = st[sub][r] * kScale;
        if (key >= S || (CAUSAL && key > query)) v = -INFINITY;
        st[sub][r] = v;
        mx = fmaxf(mx, v);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float mn = fmaxf(m, mx);
    const float msafe = (mn == -INFINITY) ? 0.f : mn;
    const float alpha = __expf(m - msafe);   // m = -inf -> 0
    m = mn;
    float rs = 0.f;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float pr = __expf(st[sub][r] - msafe);
        st[sub][r] = pr;
        rs += pr;
      }
    rs += __shfl_xor(rs, 32);
    l = l * alpha + rs;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;

    // O^T[d][query] += V^T[d][keys] P^T[keys][query], 16 keys per MFMA: step (sub, t) contracts the keys of
    // registers 8t..8t+7 = {32 sub + 16 t + 4 half + (0..3)} and {.. + 8 + (0..3)}
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        V8 pf;
#pragma unroll
        for (int e = 0; e < 8; ++e) pf[e] = T::cvt_unit(st[sub][8 * t + e]);
        const int k0 = 32 * sub + 16 * t + 4 * half;
        // transposing read: lane i = 4 q + p of each 16-lane group addresses row (key) k + q, head dims d0 + 4 p .. + 3,
        // and receives V[k .. k+3][d0 + i]
        const int i16 = lane & 15, qq = i16 >> 2, pp = i16 & 3;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          const int d0 = 32 * dt + 16 * ((lane >> 4) & 1);
          const int dcol = d0 + 4 * pp;   // first head dim of this lane's 8-byte piece
          const int ka = k0 + qq, kb = k0 + 8 + qq;
          const s16x4 lo = lds_tr16(Vs + gran_off(ka, dcol >> 3) + (dcol & 7) * 2);
          const s16x4 hi = lds_tr16(Vs + gran_off(kb, dcol >> 3) + (dcol & 7) * 2);
          typedef short s16x8 __attribute__((ext_vector_type(8)));
          const s16x8 both = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
          o[dt] = T::mfma32(__builtin_bit_cast(V8, both), pf, o[dt]);
        }
      }
  }
  if (query < S) {
    const float inv = 1.0f / l;
    unsigned short* orow = out + ((size_t)s0 + query) * D + h * HD;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        u16x4 v = {T::bits(o[dt][4 * j + 0] * inv), T::bits(o[dt][4 * j + 1] * inv), T::bits(o[dt][4 * j + 2] * inv),
                   T::bits(o[dt][4 * j + 3] * inv)};
        *reinterpret_cast<u16x4*>(orow + 32 * dt + 8 * j + 4 * half) = v;
      }
  }
}

// One query row per (sequence, head), one WAVE each (four per workgroup): `last` = 0 row 0 of the sequence (the CLS row of a
// vision tower), 1 its last row (the first EOS of a packed caption); either way the query sees all S_n keys of its own
// sequence.  P stays fp32.  out [N][H*64].  S_n is clamped to max_S (<= 64 ROW_MAXI, checked by the entry), so a table that
// disagrees with max_S cannot index past sc[]; an empty sequence returns before any load and writes nothing.
constexpr int ROW_MAXI = 8;        // keys per lane: S <= 512
template <class T>
__global__ void __launch_bounds__(256) attn_varlen_row_fwd16_kernel(const unsigned short* __restrict__ qkv,
                                                                    const int32_t* __restrict__ cu,
                                                                    unsigned short* __restrict__ out, int N, int max_S, int H,
                                                                    int last) {
  const int lane = threadIdx.x & 63;
  const int bh = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (bh >= N * H) return;
  const int b = bh / H, h = bh % H;
  const int Tt = cu[N];
  const int s0 = min(max(cu[b], 0), Tt);
  const int S = min(min(max(cu[b + 1], s0), Tt) - s0, max_S);
  if (S <= 0) return;                                         // wave-uniform; no barrier in this kernel
  const int D = H * HD, ld = 3 * D;
  const int qrow = last ? S - 1 : 0;
  const int nkeys = S;
  const unsigned short* base = qkv + (size_t)s0 * ld + h * HD;
  float q[64];
  {
    const unsigned short* qp = base + (size_t)qrow * ld;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const u32x4 w = *reinterpret_cast<const u32x4*>(qp + 8 * c);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        q[8 * c + 2 * e] = T::lo_f32(w[e]);
        q[8 * c + 2 * e + 1] = T::hi_f32(w[e]);
      }
    }
  }
  float sc[ROW_MAXI];
  float mx = -INFINITY;
#pragma unroll
  for (int i = 0; i < ROW_MAXI; ++i) {
    const int j = lane + 64 * i;
    sc[i] = -INFINITY;
    if (64 * i < nkeys) {                                     // wave-uniform
      const unsigned short* kp = base + D + (size_t)min(j, nkeys - 1) * ld;
      float a0 = 0.f, a1 = 0.f;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const u32x4 w = *reinterpret_cast<const u32x4*>(kp + 8 * c);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          a0 += q[8 * c + 2 * e] * T::lo_f32(w[e]);
          a1 += q[8 * c + 2 * e + 1] * T::hi_f32(w[e]);
        }
      }
      if (j < nkeys) sc[i] = (a0 + a1) * kScale;
      mx = fmaxf(mx, sc[i]);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < ROW_MAXI; ++i) {
    sc[i] = (64 * i < nkeys && lane + 64 * i < nkeys) ? __expf(sc[i] - mx) : 0.f;
    sum += sc[i];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
  const float inv = 1.f / sum;
  // lane d: out[d] = sum_j p_j V[j][d]
  const unsigned short* vp = base + 2 * D + lane;
  float acc0 = 0.f, acc1 = 0.f;
#pragma unroll
  for (int i = 0; i < ROW_MAXI; ++i) {
    if (64 * i >= nkeys) break;                               // wave-uniform
    const int nn = min(64, nkeys - 64 * i);
    int jj = 0;
    for (; jj + 1 < nn; jj += 2) {
      const float p0 = __shfl(sc[i], jj), p1 = __shfl(sc[i], jj + 1);
      const float v0 = T::to_f32(vp[(size_t)(64 * i + jj) * ld]);
      const float v1 = T::to_f32(vp[(size_t)(64 * i + jj + 1) * ld]);
      acc0 += p0 * v0;
      acc1 += p1 * v1;
    }
    if (jj < nn) acc0 += __shfl(sc[i], jj) * T::to_f32(vp[(size_t)(64 * i + jj) * ld]);
  }
  out[(size_t)b * D + h * HD + lane] = T::bits((acc0 + acc1) * inv);
}

template <class T>
int attention_varlen16(const char* name, const void* qkv, const int32_t* cu, void* out, int N, int max_S, int H, int causal,
                       void* stream) {
  DCLIP_REQUIRE(qkv && cu && out, "%s: null pointer", name);
  DCLIP_REQUIRE(N > 0 && max_S > 0 && H > 0 && (long long)N * H < (1ll << 31), "%s: bad shape N=%d max_S=%d H=%d", name, N,
                max_S, H);
  DCLIP_REQUIRE(((uintptr_t)qkv | (uintptr_t)out) % 16 == 0 && (uintptr_t)cu % 4 == 0,
                "%s: qkv / out must be 16-byte aligned, cu_seqlens 4-byte aligned", name);
  const dim3 grid(N * H, cdiv(max_S, 64)), block(128);
  hipStream_t st = (hipStream_t)stream;
  if (causal)
    hipLaunchKernelGGL((attn_varlen_fwd16_kernel<T, true>), grid, block, 0, st, (const unsigned short*)qkv, cu,
                       (unsigned short*)out, N, H);
  else
    hipLaunchKernelGGL((attn_varlen_fwd16_kernel<T, false>), grid, block, 0, st, (const unsigned short*)qkv, cu,
                       (unsigned short*)out, N, H);
  DCLIP_CHECK_LAUNCH(name);
  return DCLIP_OK;
}

template <class T>
int attention_varlen_row16(const char* name, const void* qkv, const int32_t* cu, void* out, int N, int max_S, int H, int last,
                           void* stream) {
  DCLIP_REQUIRE(qkv && cu && out, "%s: null pointer", name);
  DCLIP_REQUIRE(N > 0 && max_S > 0 && max_S <= 64 * ROW_MAXI && H > 0 && (long long)N * H < (1ll << 31),
                "%s: bad shape N=%d max_S=%d (<= 512) H=%d", name, N, max_S, H);
  DCLIP_REQUIRE(((uintptr_t)qkv | (uintptr_t)out) % 16 == 0 && (uintptr_t)cu % 4 == 0,
                "%s: qkv / out must be 16-byte aligned, cu_seqlens 4-byte aligned", name);
  const unsigned blocks = (unsigned)(((long long)N * H + 3) / 4);
  hipLaunchKernelGGL(attn_varlen_row_fwd16_kernel<T>, dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                     (const unsigned short*)qkv, cu, (unsigned short*)out, N, max_S, H, last ? 1 : 0);
  DCLIP_CHECK_LAUNCH(name);
  return DCLIP_OK;
}

}  // namespace

DCLIP_API int dclip_attention_varlen_fwd_bf16(const void* qkv, const int32_t* cu_seqlens, void* out, int N, int max_S, int H,
                                              int causal, void* stream) {
  return attention_varlen16<Bf16T>("attention_varlen_fwd_bf16", qkv, cu_seqlens, out, N, max_S, H, causal, stream);
}

DCLIP_API int dclip_attention_varlen_fwd_f16(const void* qkv, const int32_t* cu_seqlens, void* out, int N, int max_S, int H,
                                             int causal, void* stream) {
  return attention_varlen16<F16T>("attention_varlen_fwd_f16", qkv, cu_seqlens, out, N, max_S, H, causal, stream);
}

DCLIP_API int dclip_attention_varlen_row_fwd_bf16(const void* qkv, const int32_t* cu_seqlens, void* out, int N, int max_S,
                                                  int H, int last, void* stream) {
  return attention_varlen_row16<Bf16T>("attention_varlen_row_fwd_bf16", qkv, cu_seqlens, out, N, max_S, H, last, stream);
}

DCLIP_API int dclip_attention_varlen_row_fwd_f16(const void* qkv, const int32_t* cu_seqlens, void* out, int N, int max_S, int H,
                                                 int last, void* stream) {
  return attention_varlen_row16<F16T>("attention_varlen_row_fwd_f16", qkv, cu_seqlens, out, N, max_S, H, last, stream);
}
