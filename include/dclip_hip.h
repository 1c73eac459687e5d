/*
 * dclip_hip.h — C ABI of libdclip_hip.so: the MI355X (gfx950) kernels behind the DCLIP
 * distillation step.
 *
 * The reference (ChuckDanz/DCLIP) has no FFI of its own: every dense operation on its hot
 * path is a call into a third-party Python library (HF transformers CLIPModel, torch
 * nn.MultiheadAttention, torch.nn.functional).  Each entry point below therefore cites the
 * reference call site (path:line under /root/reference, or hf: for transformers 5.15.0
 * modeling_clip.py) whose arithmetic it replaces.  The Python binding a maintainer adds is
 * shown in INTEGRATION.md; the one this repo ships is dclip_amd/_lib.py (ctypes).
 *
 * Conventions (all entry points):
 *   - plain pointers + sizes; every pointer is DEVICE memory owned by the caller (incl.
 *     `workspace`); the library never allocates, frees or synchronises.
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *     work is enqueued on it and the call returns immediately.
 *   - tensors are row-major, contiguous unless a leading dimension is given; activations are
 *     [rows = batch*seq, features]; weights are [out, in] exactly as stored in the checkpoints.
 *   - return 0 on success, negative DCLIP_E* otherwise; dclip_last_error() gives the text of the
 *     calling thread's last failure.  No exceptions cross the ABI.
 *   - all arithmetic is IEEE fp32 (exact-f32 MFMA, v_mfma_f32_32x32x2_f32 / 16x16x4_f32).
 */
#ifndef DCLIP_HIP_H
#define DCLIP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DCLIP_ABI_VERSION 1

enum {
  DCLIP_OK = 0,
  DCLIP_EINVAL = -1,      /* bad shape / null pointer / unsupported size */
  DCLIP_EWORKSPACE = -2,  /* workspace too small */
  DCLIP_ELAUNCH = -3      /* HIP launch error (text in dclip_last_error) */
};

int dclip_abi_version(void);
const char* dclip_last_error(void);
/* Name of the calling thread's most recent kernel launch site ("" before the first): lets a test that forces a kernel
 * path with an environment switch assert that the path was taken.  The fp32 GEMM reports "gemm_f32" (register staging),
 * "gemm_f32.dma" (LDS-DMA staging) or, after a split-K, "gemm_f32.splitk_reduce"; the attention "attention_fwd.rows" /
 * ".stream" / "" (tiled) and "attention_bwd.rows" / ".lean" / ".stream_ds" / ".stream" / ".one_key" / "" (tiled).  The
 * 16-bit entries append the kernel variant to their own name: the GEMMs (gemm_bf16, gemm_f16, gemm_f16_ex, gemm_*_splitk,
 * gemm_*_wgrad_tokmajor) ".r64" / ".r128" (register-staged), ".pp" (ping-pong), ".pp_tok" (its token-major form), ".ppp"
 * (persistent) and, after a split-K, that name + ".splitk_reduce"; attention_fwd_{bf16,f16}[_lse] ".head1" .. ".head9"
 * (whole-head, NB = ceil(S / 32)),
 * ".head_xq" (257 tokens, shared last query) or ".tiled"; attention_bwd_{bf16,f16} "" or ".one_key" (S = 1);
 * layernorm_fwd_* ".nc<N>" or ".nc<N>.exact".  The fp32 LayerNorm reports its template instance the same way:
 * "layernorm_fwd", "layernorm_bwd" (dclip_layernorm_bwd and _bwd_ex) and "layernorm_bwd_f16" + ".nc1" / ".nc2" / ".nc3" /
 * ".nc4" / ".nc8" (float4 chunks per lane, NC = ceil(D / 256)) or ".nc2.exact" / ".nc3.exact" / ".nc4.exact" (D = 512, 768,
 * 1024); the partial-sum reduce that follows a backward keeps that name.  "im2col" + ".vec" (patch % 4 == 0 and both
 * pointers 16-byte aligned) or ".scalar".  The pointer stays valid until the thread's next call of this function. */
const char* dclip_last_launch(void);
/* The FIRST launch of the calling thread's most recent entry that makes several launches and whose first one has template
 * instances of its own: dclip_split_f32_f16x3_rows_colstats leaves "split_f32_f16x3_rows_colstats" + ".regs.nc1" .. ".regs.nc6"
 * / ".cached" here, while dclip_last_launch() reports its ".cols".  "" before the first such call and after a refused one (the
 * entry clears it first); same lifetime. */
const char* dclip_first_launch(void);

/* ------------------------------------------------------------------------------------------
 * GEMM  C[M,N] = epilogue( sum_k A(m,k) * B(k,n) )           (fp32 MFMA, LDS-tiled)
 * Replaces every nn.Linear / Conv2d-as-matmul on the path: q/k/v/out_proj
 * (hf:modeling_clip.py:309-311,:333), fc1/fc2 (:347-349), patch_embedding (:209),
 * visual/text_projection (:751,:713), nn.MultiheadAttention in/out projections
 * (training/patch_text_aggregation.py:33,:42), the logits matmul
 * (training/CLIP_image_distillation.py:549) and all of their autograd transposes.
 *
 * layout bits say which index is contiguous in memory:
 *   DCLIP_A_KMAJOR : A stored [M][K] (lda >= K), else stored [K][M] (lda >= M)
 *   DCLIP_B_KMAJOR : B stored [N][K] (ldb >= K, the nn.Linear weight layout), else [K][N]
 * so  forward  y = x W^T      -> A_KMAJOR | B_KMAJOR
 *     dgrad    dx = dy W      -> A_KMAJOR            (B = W read as [K=N_out][N=in])
 *     wgrad    dW = dy^T x    -> 0                   (A = dy as [K=rows][M=out], B = x as [K=rows][N=in])
 * The contiguous dimension of each operand, and ldc, must be multiples of 4 (16-byte vectors).
 *
 * epilogue bits (applied in this order to v = acc * alpha):
 *   BIAS      v += bias[n]
 *   GELU      if (aux) aux[m,n] = v;  v = v * sigmoid(1.702 v)        (hf:activations.py:122)
 *   DGELU     v *= d/dx quick_gelu (aux[m,n])                          (its backward)
 *   RESIDUAL  v += residual[m,n]   (same ld as C)
 *   ACCUM     C[m,n] += v  instead of  C[m,n] = v
 *   A_ROWSUM  additionally aux[m] = sum_k A[m,k] (aux is float[M] here; [K][M]-major A only, not with GELU/DGELU):
 *             with A = dy in the wgrad layout this is the nn.Linear BIAS gradient, read off the operand
 *             fragments the weight-gradient GEMM feeds to the matrix cores anyway — dy is not read a second time.
 * split_k > 1 partitions K over split_k workgroups per tile; partial tiles go to `workspace`
 * (dclip_gemm_f32_workspace bytes) and are summed in fixed order by a second launch, so the
 * result is run-to-run deterministic.  split_k == 0 lets the library choose.
 */
#define DCLIP_A_KMAJOR 1
#define DCLIP_B_KMAJOR 2

#define DCLIP_EPI_BIAS 1
#define DCLIP_EPI_GELU 2
#define DCLIP_EPI_DGELU 4
#define DCLIP_EPI_RESIDUAL 8
#define DCLIP_EPI_ACCUM 16
#define DCLIP_EPI_A_ROWSUM 32

size_t dclip_gemm_f32_workspace(int M, int N, int K, int layout, int split_k);
/* The plan dclip_gemm_f32 runs for this problem under the current environment (DCLIP_GEMM_TILE, DCLIP_GEMM_PLAN_TABLE):
 * out = { tile rows BM, tile columns BN, K splits, K elements per split }. */
int dclip_gemm_f32_plan(int M, int N, int K, int layout, int split_k, int out[4]);
int dclip_gemm_f32(const float* A, const float* B, float* C, const float* bias, const float* residual,
                   float* aux, int M, int N, int K, int lda, int ldb, int ldc, int layout, int epilogue,
                   float alpha, int split_k, void* workspace, size_t workspace_bytes, void* stream);

/* Column sums  out[n] (+)= sum_m X[m,n]  — bias gradients of every nn.Linear above. */
size_t dclip_colsum_f32_workspace(int M, int N);
int dclip_colsum_f32(const float* X, float* out, int M, int N, int ldx, int accumulate, void* workspace,
                     size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * LayerNorm over the last dim (biased variance, eps inside the sqrt) — nn.LayerNorm at
 * hf:modeling_clip.py:364-366 (layer_norm1/2), :642 (pre_layrnorm), :651 (post_layernorm),
 * :568 (final_layer_norm); training/patch_text_aggregation.py:35,:44 (norm_text/norm_image).
 * fwd saves mean and rstd per row.  bwd: dx = LN'(dy) (+ dresidual if non-null: the skip
 * connection's gradient is added in the same pass); dgamma/dbeta (+)= column reductions.
 */
int dclip_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean,
                        float* rstd, int rows, int D, float eps, void* stream);
size_t dclip_layernorm_bwd_workspace(int rows, int D);
int dclip_layernorm_bwd(const float* dy, const float* x, const float* gamma, const float* mean,
                        const float* rstd, const float* dresidual, float* dx, float* dgamma, float* dbeta,
                        int rows, int D, int accumulate_param_grads, void* workspace, size_t workspace_bytes,
                        void* stream);
/* The bf16 training path's form (configs c3 / c5; nothing in the reference, which is fp32-only —
 * training/CLIP_image_distill_training.py:40): the same pass also writes, when non-null,
 *   dx_bf16   [rows][D] bf16 copy of dx — the A operand of the data- and weight-gradient GEMMs that follow;
 *   dx_colsum [D]       column sums of dx — the bias gradient of the nn.Linear whose output gradient dx is
 *                       (out_proj.bias for LayerNorm2, the layer below's fc2.bias for LayerNorm1: hf:modeling_clip.py:346-383).
 * Same workspace as dclip_layernorm_bwd. */
int dclip_layernorm_bwd_ex(const float* dy, const float* x, const float* gamma, const float* mean,
                           const float* rstd, const float* dresidual, float* dx, void* dx_bf16, float* dgamma,
                           float* dbeta, float* dx_colsum, int rows, int D, int accumulate_param_grads,
                           void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Multi-head self-attention core, head_dim = 64:  O = softmax(Q K^T / 8 [+ causal]) V
 * — eager_attention_forward, hf:modeling_clip.py:259-277 (vision: no mask; text: causal,
 * :546-551).  qkv is the fused projection output [B*S, 3*H*64] = [q | k | v] per token;
 * out is [B*S, H*64]; lse [B, H, S] keeps log-sum-exp per query row for the backward, which
 * recomputes P instead of storing it.
 */
int dclip_attention_fwd(const float* qkv, float* out, float* lse, int B, int S, int H, int causal,
                        void* stream);
int dclip_attention_bwd(const float* qkv, const float* out, const float* dout, const float* lse,
                        float* dqkv, float* delta /* scratch [B*H*S] */, int B, int S, int H, int causal,
                        void* stream);
/* Workspace form of the backward (what dclip_amd.ops.attention_bwd calls).  `workspace` (16-byte aligned,
 * >= dclip_attention_bwd_workspace bytes) holds delta and — for long non-causal sequences (S > 80: the 197 tokens of
 * ViT-B/16, the 257 of ViT-L/14) — the dS^T blocks [B*H][Sp][Sp], Sp = S rounded up to 32 (S <= 512; longer sequences keep the two-kernel split): dS is formed ONCE in the dK/dV kernel
 * and read back by the dQ kernel (5 MFMA products instead of the 7 of the two-kernel recompute split); results equal
 * dclip_attention_bwd's up to the summation order of delta.  Same reference arithmetic: hf:modeling_clip.py eager
 * attention backward (autograd of :333-349). */
size_t dclip_attention_bwd_workspace(int B, int S, int H, int causal);
int dclip_attention_bwd_ws(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv,
                           void* workspace, size_t workspace_bytes, int B, int S, int H, int causal, void* stream);
/* CLS-only form for the LAST vision layer: the model reads only row 0 of the final hidden state
 * (hf:modeling_clip.py:650), so that layer's attention output is needed for one query row per (image, head).
 * out [B, H*64], lse [B, H].  _bwd writes d k / d v for every row and d q for the CLS rows of dqkv [B*S, 3*H*64];
 * the caller zero-fills dqkv first (d q of the other rows is exactly zero).  delta: scratch [B*H]. */
int dclip_attention_cls_fwd(const float* qkv, float* out, float* lse, int B, int S, int H, void* stream);
/* Same idea for the frozen text tower's last layer: one query row per caption at position rows[b] (its first EOS,
 * hf:modeling_clip.py:574-581) against keys 0..rows[b] (causal).  Forward only.  out [B, H*64], lse [B, H]. */
int dclip_attention_row_fwd(const float* qkv, const int32_t* rows, float* out, float* lse, int B, int S, int H,
                            void* stream);
int dclip_attention_cls_bwd(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv,
                            float* delta, int B, int S, int H, void* stream);

/* ------------------------------------------------------------------------------------------
 * Embedding plumbing.
 * im2col: pixel_values [B,C,Himg,Wimg] -> patch rows [B*g*g, C*p*p] so that
 *   patch_embedding (Conv2d stride=p, no bias; hf:modeling_clip.py:209-210) is one GEMM.
 * vision_assemble: x[b,0,:] = class_embedding + pos[0]; x[b,1+i,:] = patch[b,i,:] + pos[1+i]
 *   (hf:modeling_clip.py:212-217).  _bwd copies d x[:,1:,:] into compact d patch rows; d pos is the
 *   column sum of d x viewed as [B, S*D] (dclip_colsum_f32) and d class is its first D entries.
 * text_embed: x[b,t,:] = token_embedding[ids[b,t]] + position_embedding[t] (hf:modeling_clip.py:250-255);
 *   _bwd scatter-adds d x into d token_embedding (float atomics; caller zeroes or accumulates).
 *   Both clamp an id outside [0, vocab) into the table: id < 0 reads / adds into row 0, id >= vocab row vocab - 1
 *   (nn.Embedding raises there; a caller that wants the error checks its ids).  Same shape rules for both: B, T, vocab > 0,
 *   D a positive multiple of 4.
 * first_eos: index of the first EOS id per row, 0 if absent (hf:modeling_clip.py:574-581).
 * gather_rows: out[b,:] = x[b, idx[b], :] (idx == NULL: row 0, the CLS token, hf:modeling_clip.py:650);
 * scatter_rows: its transpose, writing the whole [B,S,D] gradient (zeros off the selected row).
 */
int dclip_im2col(const float* pixels, float* cols, int B, int C, int Himg, int Wimg, int patch, void* stream);
/* Same gather with a bf16 destination (row length ldc >= C*patch*patch, multiple of 4; patch % 4 == 0): the A operand
 * of the frozen towers' bf16 patch-embedding GEMM, written in one pass instead of im2col + cast.  Columns C*patch*patch..ldc
 * of a row are NOT written (they keep what the caller put there; the GEMM that follows reads K = C*patch*patch columns). */
int dclip_im2col_bf16(const float* pixels, void* cols, int B, int C, int Himg, int Wimg, int patch, int ldc, void* stream);
int dclip_vision_assemble_fwd(const float* patch, const float* cls, const float* pos, float* x, int B, int S,
                              int D, void* stream);
int dclip_vision_assemble_bwd(const float* dx, float* dpatch, int B, int S, int D, void* stream);
int dclip_text_embed_fwd(const int64_t* ids, const float* tok, const float* pos, float* x, int B, int T, int D,
                         int vocab, void* stream);
int dclip_text_embed_bwd(const int64_t* ids, const float* dx, float* dtok, int B, int T, int D, int vocab,
                         void* stream);
int dclip_first_eos(const int64_t* ids, int32_t* idx, int B, int T, int64_t eos_id, void* stream);
int dclip_gather_rows(const float* x, const int32_t* idx, float* out, int B, int S, int D, void* stream);
int dclip_scatter_rows(const float* dout, const int32_t* idx, float* dx, int B, int S, int D, void* stream);

/* ------------------------------------------------------------------------------------------
 * The vision tower at another input size (hf CLIPVisionEmbeddings.interpolate_pos_encoding).
 * pos_interp_fwd: out[0] = pos[0] (the class position); out[1 + oy*gw + ox] = the bicubic resample of the g x g grid of
 *   D-vectors pos[1..] at output cell (oy, ox) of a gh x gw grid, as torch.nn.functional.interpolate(mode="bicubic",
 *   align_corners=False) DEFINES it: per axis, source coordinate x = (o + 0.5) g / g_out - 0.5, f = floor(x), t = x - f, four
 *   taps f-1 .. f+2 each clamped to [0, g-1] (taps clamped onto one cell are each added), cubic-convolution weights with
 *   A = -0.75, no antialiasing.  x, t and the weights are evaluated in double from the integers and each weight is rounded
 *   to fp32 once (the contract is the fp64 definition, not torch's fp32 coordinate arithmetic); the 16 terms
 *   (wy[a] wx[b]) pos[iy(a), ix(b)] are added in one fmaf chain, a outer, b inner: a pure function of the inputs.
 *   (gh, gw) == (g, g) returns the table (the weights are exactly 0, 1, 0, 0).
 * pos_interp_bwd: the exact transpose, dpos[1 + sy*g + sx] = sum over destination rows in ascending order of the same
 *   fp32 weights times dout; dpos[0] = dout[0]; `accumulate` adds into dpos.  Gather form, no atomics: run-to-run identical.
 *   Both: D % 4 == 0, 1 <= g <= 32768, gh, gw >= 1 with gh*gw < 2^30 (row indices are formed in int), 16-byte aligned
 *   pointers; pos / dpos are [1 + g*g][D], out / dout [1 + gh*gw][D].
 * im2col_rect{,_bf16,_f16}: dclip_im2col{,_bf16,_f16} on a gh x gw grid, gh = Himg / patch and gw = Wimg / patch by floor
 *   (both >= 1); image rows >= gh*patch and columns >= gw*patch are never read, as a stride-`patch` convolution ignores
 *   them.  dclip_last_launch: the entry's name + ".vec" (patch % 4 == 0, Wimg % 4 == 0, 16-byte pointers) or ".scalar".
 *   The 16-bit forms keep patch % 4 == 0 and the ldc / alignment rules of dclip_im2col_bf16. */
int dclip_pos_interp_fwd(const float* pos, float* out, int g, int gh, int gw, int D, void* stream);
int dclip_pos_interp_bwd(const float* dout, float* dpos, int g, int gh, int gw, int D, int accumulate, void* stream);
int dclip_im2col_rect(const float* pixels, float* cols, int B, int C, int Himg, int Wimg, int patch, void* stream);
int dclip_im2col_rect_bf16(const float* pixels, void* cols, int B, int C, int Himg, int Wimg, int patch, int ldc, void* stream);
int dclip_im2col_rect_f16(const float* pixels, void* cols, int B, int C, int Himg, int Wimg, int patch, int ldc, void* stream);

/* ------------------------------------------------------------------------------------------
 * The frozen vision tower on a PACKED batch of crops of different sizes: the full-resolution teacher in one
 * pass.  Forward only.  N crops; crop n has the patch grid gh_n = (y2-y1)/p, gw_n = (x2-x1)/p (floor, both >= 1) and
 * S_n = 1 + gh_n gw_n token rows.  cu_seqlens [N+1] (int32) are the cumulative token rows, T = cu_seqlens[N];
 * patch_offsets [N+1] the cumulative patch rows, patch_offsets[n] = cu_seqlens[n] - n.  Both tables live on the device and are
 * built on the host from the box list.  The layers between these entries are row-wise over M = T and run unchanged.
 * patches_from_boxes_u8: replaces the per-crop host path (PIL crop + ToTensor + upload + dclip_im2col_rect).  images_u8
 *   [B][Hmax][Wmax][3], dims [B][2] = (h, w), boxes [N][5] = (b, x1, y1, x2, y2) as dclip_crop_resize_u8 takes them.  cols row
 *   patch_offsets[n] + gy*gw_n + gx, column c*p*p + py*p + px (the column order of dclip_im2col*) = pixel (y1 + gy*p + py,
 *   x1 + gx*p + px) of image b, channel c, DIVIDED by 255 (a correctly rounded fp32 division, ToTensor()'s value).  A
 *   position outside [0,h) x [0,w) of its own image gives 0 without a read (PIL's crop past an edge); the bytes of the
 *   batch's padding are never used.  Rows and columns of a crop beyond whole patches are not read.  Any patch in [1, 1024];
 *   16-byte stores when patch % 4 == 0.  cols 16-byte aligned.
 * vision_assemble_varlen: replaces dclip_pos_interp_fwd + dclip_vision_assemble_fwd per crop.  grids [N][2] = (gh, gw).  x row
 *   cu[n] = cls + pos[0]; row cu[n] + 1 + j = patch_emb[cu[n] - n + j] + R_n[1 + j], R_n = pos [1 + g*g][D] resampled to crop n's
 *   grid by the arithmetic of pos_interp_fwd (same taps, same 16-term fmaf chain) and added by vision_assemble_fwd's
 *   statement: per crop bit-equal to those two calls.  D % 4 == 0, 16-byte aligned float operands.
 * attention_varlen_fwd: replaces dclip_attention_fwd / dclip_attention_cls_fwd per crop.  qkv [T][3*H*64]; non-causal
 *   self-attention inside each sequence cu[n] .. cu[n+1]-1 and nowhere else.  cls_only = 0: out [T][H*64], lse [H][T];
 *   cls_only = 1: only row 0 of each sequence is a query, out [N][H*64], lse [H][N].  lse may be NULL.  max_S bounds the
 *   sequence lengths (it sizes the grid: query rows at or beyond max_S of a sequence are not computed).  Any S_n >= 1.
 *   A sequence's loads never leave its own rows.
 * gather_rows_at: out[n] = x[rows[n]], x [T][D], rows [N] in [0, T) in any order, repeats allowed (an index outside is
 *   clamped): replaces dclip_gather_rows (which needs equal strides) for the last layer's residual on the CLS rows.
 * Each refuses N <= 0, a bad shape, a null or misaligned pointer with DCLIP_EINVAL before any launch. */
int dclip_patches_from_boxes_u8(const uint8_t* images_u8, const int32_t* dims, const int32_t* boxes,
                                const int32_t* patch_offsets, float* cols, int B, int Hmax, int Wmax, int N, int patch,
                                void* stream);
int dclip_vision_assemble_varlen(const float* patch_emb, const float* cls, const float* pos, const int32_t* grids,
                                 const int32_t* cu_seqlens, float* x, int g, int N, int D, void* stream);
int dclip_attention_varlen_fwd(const float* qkv, const int32_t* cu_seqlens, float* out, float* lse, int N, int max_S, int H,
                               int cls_only, void* stream);
int dclip_gather_rows_at(const float* x, const int32_t* rows, float* out, int N, int T, int D, void* stream);

/* ------------------------------------------------------------------------------------------
 * The frozen text tower on PACKED captions: each caption is cut after its first EOS and the captions lie back
 * to back.  Forward (the backward is the next section).  N captions; len_n = first EOS index + 1 (1 for a caption without EOS, as dclip_first_eos returns 0
 * for it); cu_seqlens [N+1] (int32, on the device, built on the host from the token ids) are the cumulative lengths,
 * Tp = cu_seqlens[N].  Every entry is clamped into [0, Tp] and made non-decreasing on the device.  The layers between these
 * entries are row-wise over M = Tp and run unchanged; dclip_gather_rows_at at rows cu[1:] - 1 gathers the first-EOS rows.
 * text_embed_varlen: replaces dclip_text_embed_fwd.  ids [N][T] int64 (the padded matrix); x [Tp][D]:
 *   x[cu[n] + t] = tok[clamp(ids[n][t])] + pos[t] for t < min(len_n, T), the id clamp of dclip_text_embed_fwd.  ids[n][t >= len_n]
 *   are never read and nothing is written outside rows [cu[n], cu[n+1]).  D % 4 == 0; tok / pos / x 16-byte aligned.
 * attention_varlen_causal_fwd: replaces dclip_attention_fwd(causal = 1) / dclip_attention_row_fwd.  qkv [Tp][3*H*64] fp32;
 *   query row i of a sequence sees keys 0..i of that sequence and nothing else.  last_only = 0: out [Tp][H*64], lse [H][Tp];
 *   last_only = 1: the only query is the LAST row of each sequence (the first EOS, which sees the whole sequence), out
 *   [N][H*64], lse [H][N].  lse may be NULL.  max_S bounds the lengths (it sizes the grid, as in attention_varlen_fwd).
 *   A sequence's loads never leave its own rows.
 * pack_tokens_varlen: replaces dclip_pack_tokens.  tokens [Tp][P] packed, sentence [N][P], out [N][Tmax][P]; with
 *   n_b = max(len_b - 2, 0): out[b][i] = tokens[cu[b] + 1 + i] for i < n_b, zero beyond; n_b == 0 puts sentence[b] in slot 0.
 * Each refuses N <= 0, a bad shape, a null or misaligned pointer with DCLIP_EINVAL before any launch. */
int dclip_text_embed_varlen(const int64_t* ids, const int32_t* cu_seqlens, const float* tok, const float* pos, float* x, int N,
                            int T, int D, int vocab, void* stream);
int dclip_attention_varlen_causal_fwd(const float* qkv, const int32_t* cu_seqlens, float* out, float* lse, int N, int max_S,
                                      int H, int last_only, void* stream);
int dclip_pack_tokens_varlen(const float* tokens, const float* sentence, const int32_t* cu_seqlens, float* out, int N, int Tmax,
                             int P, void* stream);

/* ------------------------------------------------------------------------------------------
 * The TRAINABLE text tower on packed captions: the backward of the three ragged entries above, fp32.  Layout,
 * table and its on-device clamp as there (Tp = cu_seqlens[N]).  The gradients are the padded tower's: d x is exactly zero on
 * every row behind a first EOS, so every parameter gradient of the padded rectangle is the sum over the cut captions.
 * attention_varlen_causal_bwd: the backward of dclip_attention_varlen_causal_fwd(last_only = 0).  qkv [Tp][3*H*64], out / dout
 *   [Tp][H*64], lse [H][Tp] exactly what that entry wrote, dqkv [Tp][3*H*64] = [dq|dk|dv], delta [H][Tp] caller-provided scratch
 *   (written, then read; no meaning afterwards).  Two tiled kernels, grid (N*H, cdiv(max_S, 64)): dQ visits key tiles 0 .. its
 *   own, dK / dV query tiles from its own on.  max_S bounds the lengths (rows at or beyond max_S of a sequence are not computed).
 *   Every word of the dqkv rows of sequences of length 1 .. max_S is written and nothing else; a sequence of length 1 gets exact
 *   zeros in dq and dk and dv = dout; a sequence of length 0 writes nothing.  No atomics: bit-equal from run to run.  A
 *   sequence's loads never leave its own rows.  qkv / out / dout / dqkv 16-byte aligned.
 * text_embed_varlen_bwd: the backward of dclip_text_embed_varlen.  ids [N][T], dx [Tp][D].  dtok [vocab][D]:
 *   dtok[clamp(ids[n][t])] += dx[cu[n] + t] for t < min(len_n, T) — float atomics into the caller's buffer (zeroed or accumulating),
 *   the id clamp of dclip_text_embed_bwd; ids[n][t >= len_n] are never read.  dpos [>= T][D]: dpos[t] = sum over the captions with
 *   len_n > t of dx[cu[n] + t], added in ascending n (deterministic), WRITTEN for every t < T (zeros where no caption reaches);
 *   rows >= T are untouched.  dtok or dpos may be NULL, not both.  D % 4 == 0, T * D < 2^31; dx / dpos 16-byte aligned.
 * scatter_last_rows: the ragged twin of dclip_scatter_rows and the transpose of dclip_gather_rows_at at rows cu[1:] - 1.  dout
 *   [N][D]; the whole dx [Tp][D] is written: row cu[n+1] - 1 gets dout[n], every other row of [cu[n], cu[n+1]) zero.  D % 4 == 0,
 *   dout / dx 16-byte aligned.
 * Each refuses N <= 0, a bad shape, a null or misaligned pointer with DCLIP_EINVAL before any launch. */
int dclip_attention_varlen_causal_bwd(const float* qkv, const int32_t* cu_seqlens, const float* out, const float* dout,
                                      const float* lse, float* dqkv, float* delta, int N, int max_S, int H, void* stream);
int dclip_text_embed_varlen_bwd(const int64_t* ids, const int32_t* cu_seqlens, const float* dx, float* dtok, float* dpos, int N,
                                int T, int D, int vocab, void* stream);
int dclip_scatter_last_rows(const float* dout, const int32_t* cu_seqlens, float* dx, int N, int D, void* stream);

/* ------------------------------------------------------------------------------------------
 * 16-bit MFMA attention core for the two packed frozen towers above.  Forward only, head dim 64, no lse.
 * qkv [T][3*H*64] bf16 / fp16 (the qkv projection writes it), N sequences back to back, sequence n in rows cu[n] .. cu[n+1]-1,
 * T = cu_seqlens[N]; every table entry is clamped into [0, T] and made non-decreasing on the device.  Scores and softmax are
 * fp32; a sequence's loads never leave its own rows; an empty sequence writes nothing.
 * attention_varlen_fwd_*: the padded tiled kernel of dclip_attention_fwd_bf16 / _f16 (P rounded to the type for P V) with b*S
 *   replaced by cu[n]: bit-equal to it on equal lengths above 288.  causal = 0: every query sees all keys of its sequence (packed
 *   vision crops); causal = 1: query i sees keys 0..i (packed captions).  out [T][H*64] of the type.  max_S bounds the lengths (it
 *   sizes the grid: query rows at or beyond max_S of a sequence are not computed).
 * attention_varlen_row_fwd_*: one query row per sequence, P kept in fp32 (dclip_attention_row_fwd_bf16 / _f16 with the same
 *   substitution).  last = 0: row 0 of each sequence (CLS); last = 1: its last row (the first EOS).  Either way the query sees
 *   all keys of its own sequence.  out [N][H*64] of the type; the row of an empty sequence is left untouched.  max_S <= 512;
 *   lengths are clamped to max_S.
 * Each refuses N <= 0, H <= 0, max_S <= 0 (row: max_S > 512), N*H >= 2^31, a null pointer, qkv / out not 16-byte aligned or
 * cu_seqlens not 4-byte aligned with DCLIP_EINVAL before any launch. */
int dclip_attention_varlen_fwd_bf16(const void* qkv, const int32_t* cu_seqlens, void* out, int N, int max_S, int H, int causal,
                                    void* stream);
int dclip_attention_varlen_fwd_f16(const void* qkv, const int32_t* cu_seqlens, void* out, int N, int max_S, int H, int causal,
                                   void* stream);
int dclip_attention_varlen_row_fwd_bf16(const void* qkv, const int32_t* cu_seqlens, void* out, int N, int max_S, int H, int last,
                                        void* stream);
int dclip_attention_varlen_row_fwd_f16(const void* qkv, const int32_t* cu_seqlens, void* out, int N, int max_S, int H, int last,
                                       void* stream);

/* ------------------------------------------------------------------------------------------
 * Losses.
 * normalize_rows: xhat = x / max(||x||, eps), inv[b] = 1/max(||x||,eps)   (F.normalize,
 *   training/CLIP_image_distillation.py:545-546,:569-570; eps = 1e-12).
 *   _bwd: dx = inv * (dxhat - xhat <dxhat, xhat>); rows where the clamp was active get dxhat/eps.
 * contrastive_lse: for local rows a_i (i < Bl) against ALL columns b_j (j < Bg), both already
 *   normalised:  lse[i] = log sum_j exp(<a_i,b_j> * inv_temp),  diag[i] = <a_i, b_{i+offset}> * inv_temp.
 *   The [Bl,Bg] logits never reach HBM: MFMA tiles are reduced to per-row (max, sum-exp) partials with
 *   wave shuffles in the GEMM epilogue (training/CLIP_image_distillation.py:549,:556-557).
 * contrastive_grad: da_i = coef * sum_j ( exp(z_ij - lse_row[i]) + exp(z_ij - lse_col[j])
 *   - 2*[j == i+offset] ) * b_j   with z_ij = <a_i,b_j>*inv_temp — the gradient of
 *   (CE_rows + CE_cols) w.r.t. the normalised local rows; coef = inv_temp / (2*Bg).
 *   (This round the [Bl,Bg] weight tile is staged through `workspace`; see DESIGN.md.)
 * cosine_loss: loss_sum = sum_b (1 - cos_b), cos[b] kept for the backward, which returns
 *   ds = -coef * d cos / d s   (training/CLIP_image_distillation.py:564-576).
 * sub_reduce: out (+)= scale * sum_i (a[i] - b[i])  (b may be NULL) — fixed-order scalar reduction.
 */
int dclip_normalize_rows_fwd(const float* x, float* xhat, float* inv_norm, int B, int P, float eps, void* stream);
int dclip_normalize_rows_bwd(const float* dxhat, const float* xhat, const float* inv_norm, float* dx, int B,
                             int P, float eps, int accumulate, void* stream);
size_t dclip_contrastive_workspace(int Bl, int Bg, int P);
int dclip_contrastive_lse(const float* a_local, const float* b_global, float* lse, float* diag, int Bl, int Bg,
                          int P, int offset, float inv_temp, void* workspace, size_t workspace_bytes,
                          void* stream);
int dclip_contrastive_grad(const float* a_local, const float* b_global, const float* lse_row,
                           const float* lse_col, float* da_local, int Bl, int Bg, int P, int offset,
                           float inv_temp, float coef, void* workspace, size_t workspace_bytes, void* stream);
int dclip_cosine_loss_fwd(const float* s, const float* t, float* loss_sum, float* cos, int B, int P,
                          void* stream);
int dclip_cosine_loss_bwd(const float* s, const float* t, const float* cos, float* ds, int B, int P, float coef,
                          int accumulate, void* stream);
int dclip_sub_reduce(const float* a, const float* b, float* out, int n, float scale, int accumulate,
                     void* stream);

/* ------------------------------------------------------------------------------------------
 * Meta-teacher tail (training/patch_text_aggregation.py).
 * cross_attention: softmax(Q K^T / 8) V with separate query and key/value sequences — the core of
 *   nn.MultiheadAttention(E, heads) as called at :33 and :42 (head_dim 64, dropout 0, no masks: zero-padded
 *   rows ARE attended).  q [B*Lq, H*64]; kv [B*Lk, 2*H*64] = [k | v] (the packed in_proj rows
 *   E..3E applied in one GEMM); out [B*Lq, H*64]; lse [B,H,Lq].  Same MFMA kernels as dclip_attention_*.
 *   _bwd returns dq [B*Lq, E] and dkv [B*Lk, 2E]; delta is scratch [B*H*Lq].
 * aggregation: m = mean_l x_l; s_l = <x_l,m> / (max(|x_l|,1e-8) max(|m|,1e-8)); w = softmax(s / temperature);
 *   out[b,:] (+)= out_scale * sum_l w_l x_l   (:243-265; the 0.5/0.5 mix of :647 is out_scale + accumulate).
 *   weights [B,L] are kept for _bwd, which returns d x for d out (already including out_scale).  L <= 96.
 * pack_tokens: the token filter of training/text_tokenizer.py:195-213 plus the zero padding of
 *   patch_text_aggregation.py:606-620 on device: out[b,i,:] = tokens[b,1+i,:] for i < eos[b]-1, zero beyond;
 *   a caption with no word tokens contributes its sentence embedding as row 0.
 * mask_rows: x[b,r,:] = 0 for r >= count[b]  (zero padding of region embeddings, :555-581).
 */
int dclip_cross_attention_fwd(const float* q, const float* kv, float* out, float* lse, int B, int Lq, int Lk,
                              int H, void* stream);
int dclip_cross_attention_bwd(const float* q, const float* kv, const float* out, const float* dout,
                              const float* lse, float* dq, float* dkv, float* delta, int B, int Lq, int Lk,
                              int H, void* stream);
int dclip_aggregation_fwd(const float* x, float* out, float* weights, int B, int L, int E, float temperature,
                          float out_scale, int accumulate, void* stream);
int dclip_aggregation_bwd(const float* x, const float* weights, const float* dout, float* dx, int B, int L,
                          int E, float temperature, float out_scale, void* stream);
int dclip_pack_tokens(const float* tokens, const float* sentence, const int32_t* eos, float* out, int B, int T,
                      int Tmax, int P, void* stream);
int dclip_mask_rows(float* x, const int32_t* count, int B, int R, int E, void* stream);
/* NaN / Inf guards of the reference's teacher glue (training/patch_text_aggregation.py:497-499, :542, :649): x is
 * [groups][rows][E]; a group holding any non-finite value becomes zeros.  mode 0: detect, write flags[groups]
 * (1 = replaced) and zero in place; mode 1: zero the groups already flagged (the guard's backward). */
int dclip_sanitize_groups(float* x, int32_t* flags, int groups, int rows, int E, int mode, void* stream);

/* ------------------------------------------------------------------------------------------
 * Checkpoint consumers: retrieval and zero-shot evaluation on the similarity kernel.
 * The reference materialises caption x image similarities chunk by chunk and argsorts every row / column
 * (eval_scripts/flickr30k_eval.py:16-88, :249-266; eval_scripts/test_zero_shot_ImageNet.py:82-103).  The rank of a
 * ground truth is the number of candidates that score strictly higher, so it is computed without the matrix:
 *   rowdot_gather: out[i] = <a_i, b_{idx[i]}>            (the ground truth's own score; idx NULL = i.  The row index
 *                  is clamped to 0 .. Bk-1: idx[i] < 0 reads row 0, idx[i] >= Bk — and row i >= Bk with idx NULL —
 *                  reads row Bk-1.)
 *   rank_count:    count[i] = #{ j < Bk, j != gt[i] : <q_i, c_j> > thresh[i] }   (MFMA tiles, per-row counts in the
 *                  epilogue; gt NULL = i.  The ground truth itself is excluded so that rounding differences between
 *                  its two evaluations cannot count it as "higher than itself".)
 * Inputs are L2-normalised rows (dclip_normalize_rows_fwd).  Exact ties count as not-higher (argsort's order
 * among equal scores is unspecified in the reference).  A candidate row that is bit-identical to the ground truth
 * (Flickr30k has duplicate captions) is such a tie only in exact arithmetic: rowdot_gather and the MFMA tile add the
 * same products in two different orders, so each duplicate may or may not be counted; nothing else is affected.
 * gt[i] outside 0 .. Bk-1 (and gt NULL with i >= Bk) excludes nothing.  The workspace holds one fp32 partial count per
 * (32-column sub-tile, row), all of them written by every call, summed and rounded by the merge launch.
 */
size_t dclip_rank_count_workspace(int Bq, int Bk);
int dclip_rowdot_gather(const float* a, const float* b, const int32_t* idx, float* out, int Bq, int Bk, int P,
                        void* stream);
int dclip_rank_count(const float* queries, const float* candidates, const float* thresh, const int32_t* gt,
                     int32_t* count, int Bq, int Bk, int P, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Exact top-k inner-product search (what a flat inner-product index provides) and the two small kernels
 * of the teacher's KNN region tokenizer (training/image_tokenizer.py:215-300).  The [Q, N] score matrix is never stored.
 *   topk_ip: scores[i][j], indices[i][j] = the j-th best database row for query i under the TOTAL order (score
 *            descending, index ascending): rows of equal score come lowest index first, and which of them make the list
 *            is decided the same way.  The score is the fp32 inner product as the kernel evaluated it: one fmaf chain
 *            over k = 0 .. P-1 in a fixed order (MFMA tiles, v_mfma_f32_32x32x2_f32), the same for every row whatever
 *            the split, so the result does not depend on the number of splits (-0.0 counts as +0.0 and is returned as
 *            +0.0).  A row QUALIFIES when its score is
 *            greater than -inf: a NaN score (and a -inf one) is never selected.  When fewer than k rows qualify (N < k
 *            included) the remaining slots hold (-inf, -1).  Every index written lies in [-1, N), whatever the inputs.
 *            P % 4 == 0, 1 <= k <= 16, operands 16-byte aligned; `database` is addressed with size_t (N * P may pass 2^31).
 *            Two launches, no atomics: "topk_ip" runs a grid of ceil(Q / 64) query blocks x `splits` database splits and
 *            writes one sorted partial list per (split, query) into the workspace — every slot of it, every call;
 *            "topk_ip.merge" merges them.  With tiles = ceil(N / 128) (a workgroup walks the database 128 rows at a time)
 *              want   = min(ceil(1024 / ceil(Q / 64)), 64, tiles)      1024 = 4 workgroups on each of 256 CUs
 *              splits = ceil(tiles / ceil(tiles / want))               contiguous, equal but for a shorter last one
 *              workspace bytes = splits * Q * k * 8                    [splits][Q][k] 64-bit (score, index) keys; 8-byte aligned
 *            a pure function of (Q, N, k); Q = 2048, N = 10^5 gives 32 x 32 workgroups, and N = 10^6 at k = 16 asks 16 MiB.
 *   relu_f32:   x[i] = 0 where x[i] < 0, in place; NaN and -0.0 stay as they are.
 *   knn_select: row i of out = database row idx[i] and source[i] = 0 when 0 <= idx[i] < N and sim[i] >= thresh (false
 *            for a NaN similarity; the comparison is >= as at training/image_tokenizer.py:278); otherwise row i of
 *            out = row i of fallback and source[i] = 1.  Decided on the device: no host synchronisation.
 */
size_t dclip_topk_ip_workspace(int Q, int N, int k);
int dclip_topk_ip(const float* queries, const float* database, float* scores, int32_t* indices, int Q, int N, int P, int k,
                  void* workspace, size_t workspace_bytes, void* stream);
int dclip_relu_f32(float* x, size_t n, void* stream);
int dclip_knn_select(const float* sim, const int32_t* idx, const float* database, const float* fallback, float thresh,
                     float* out, int32_t* source, int Q, int N, int P, void* stream);

/* ------------------------------------------------------------------------------------------
 * Region-crop front end: what training/image_tokenizer.py:100-110 does per box on the
 * host with PIL — `image.crop(box)` (zero padding outside the image), `Resize((S,S))` (Pillow's antialiased
 * two-pass BILINEAR in 8-bit fixed point) and `ToTensor()` (uint8/255, CHW, no mean/std) — for all boxes of a
 * batch in three launches, bit-exact with Pillow 12.2.
 *   images [B, Hmax, Wmax, 3] uint8 (HWC, each image in the top-left corner), dims [B,2] = (h, w),
 *   boxes [NR,5] int32 = (image index, x1, y1, x2, y2),  out [NR, 3, S, S] fp32.  A box may lie partly or wholly
 *   outside its image (and outside Hmax x Wmax): what is outside dims[b] reads as zero, never the batch padding.
 *   A box without extent (x2 <= x1 or y2 <= y1), which Pillow refuses, forms no index and yields three zero planes;
 *   the other boxes of the call are unaffected.
 *   max_crop_h / max_crop_w: at least the largest (y2-y1) / (x2-x1) in `boxes`, at least 1 (they size the workspace
 *   and the tap count; a larger value changes no output bit).
 */
size_t dclip_crop_resize_workspace(int NR, int S, int max_crop_h, int max_crop_w);
int dclip_crop_resize_u8(const uint8_t* images, const int32_t* dims, const int32_t* boxes, float* out, int B,
                         int Hmax, int Wmax, int NR, int S, int max_crop_h, int max_crop_w, void* workspace,
                         size_t workspace_bytes, void* stream);

/* Student-side image preprocessing (the `clip_preprocess(images=...)` call of MultiModalDataset.__getitem__,
 * training/CLIP_image_distillation.py:349-350; arithmetic = HF CLIPImageProcessor, PIL backend): decoded RGB uint8
 * images -> shortest edge resized to S with Pillow's BICUBIC two-pass 8-bit resample (long edge = int(S*long/short)),
 * centred S x S window, float32(float64(v) * (1/255)), then (x - mean) / std in fp32, CHW.  Bit-exact with the host
 * library.  images [B,Hmax,Wmax,3] (each image in the top-left dims[b] = (h,w) corner); mean/stdv are HOST float[3].
 */
size_t dclip_clip_preprocess_workspace(int B, int Hmax, int Wmax, int S);
int dclip_clip_preprocess_u8(const uint8_t* images, const int32_t* dims, float* out, int B, int Hmax, int Wmax, int S,
                             const float* mean, const float* stdv, void* workspace, size_t workspace_bytes,
                             void* stream);

/* ------------------------------------------------------------------------------------------
 * bf16 forward path for FROZEN towers (BASELINE configs c3 / c5, "bf16 MFMA"): the teacher's region encoder
 * (training/image_tokenizer.py:119-120) and the frozen text tower never need gradients, so their GEMMs may run on
 * v_mfma_f32_32x32x16_bf16 with fp32 accumulation (16x the fp32 MFMA rate).  The residual stream, LayerNorm
 * statistics, softmax and every epilogue stay fp32; only GEMM INPUTS are bf16.  Opt-in (precision="bf16"); the
 * default everywhere, and the benched config c2, is exact fp32.
 *   gemm_bf16: C[M,N] = epilogue( A[M,K] W[N,K]^T ), A and W bf16 K-major (lda, ldw multiples of 8), C fp32 or bf16;
 *              epilogue bits BIAS | GELU | RESIDUAL (fp32 residual, fp32 output only).
 *   cast_f32_bf16: row-wise fp32 -> bf16 (round to nearest even), destination rows zero padded to ldy.
 *   layernorm_fwd_bf16: nn.LayerNorm with fp32 statistics and a bf16 result (the next GEMM's A operand).
 */
int dclip_gemm_bf16(const void* A, const void* W, void* C, const float* bias, const float* residual, int M, int N,
                    int K, int lda, int ldw, int ldc, int epilogue, int out_bf16, void* stream);
int dclip_cast_f32_bf16(const float* x, void* y, int rows, int cols, int ldx, int ldy, void* stream);
/* bf16 TRAINING path (the student of configs c3 / c5; opt-in `student_precision="bf16"`, the default and the benched
 * config c2 stay exact fp32).  Forward, dgrad and wgrad GEMMs of the trainable vision tower — the autograd of
 * `self.student.get_image_features(...)` (training/CLIP_image_distillation.py:601) — run through dclip_gemm_bf16 with fp32
 * accumulation and fp32 master weights; residual stream, LayerNorm, softmax and the attention core stay fp32.
 *   gemm_bf16_ex         dclip_gemm_bf16 + `aux` (bf16 [M][ldc]): with GELU the pre-activation (bias included) is stored
 *                        there and the activation is taken of the STORED value; with DGELU (no GELU) the result is
 *                        multiplied by quick_gelu'(aux).
 *   layernorm_fwd_bf16_stats   layernorm_fwd_bf16 that also returns mean / rstd (fp32 [rows]) for the backward.
 *   transpose_to_bf16    x [rows][cols] (fp32, or bf16 when x_is_bf16) -> yT [cols][ldyT] bf16 (ldyT >= rows, multiple
 *                        of 8, zero padded) and, if y_copy != NULL, the untransposed bf16 copy [rows][ldy]: the
 *                        token-contiguous operands of dW = (dY^T)(X^T)^T and the A operand of the dgrad GEMM.  Columns
 *                        rows..ldyT of yT are written as zeros; columns cols..ldy of y_copy are NOT written.
 *   rowsum_bf16          out[r] = sum of row r of a bf16 matrix [R][ld] (a bias gradient from dY^T). */
int dclip_gemm_bf16_ex(const void* A, const void* W, void* C, const float* bias, const float* residual, void* aux, int M,
                       int N, int K, int lda, int ldw, int ldc, int epilogue, int out_bf16, void* stream);
int dclip_layernorm_fwd_bf16_stats(const float* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                                   int rows, int D, float eps, void* stream);
int dclip_transpose_to_bf16(const void* x, int x_is_bf16, void* yT, void* y_copy, int rows, int cols, int ldx, int ldyT,
                            int ldy, void* stream);
/* Short-sequence self-attention with bf16 I/O for the bf16 training student (configs c3 / c5; eager_attention_forward,
 * hf:modeling_clip.py:259-277, arithmetic in fp32 as in dclip_attention_fwd / _bwd): qkv16 [B*S][3*H*64], out16 / dout16
 * [B*S][H*64] and dqkv16 [B*S][3*H*64] are bf16, lse [B*H][S] fp32.  Forward S <= 80, backward S <= 64. */
int dclip_attention_fwd_io16(const void* qkv16, void* out16, float* lse, int B, int S, int H, int causal, void* stream);
int dclip_attention_bwd_io16(const void* qkv16, const void* out16, const void* dout16, const float* lse, void* dqkv16, int B,
                             int S, int H, int causal, void* stream);
/* Every GEMM weight of a training tower converted in one launch (bf16 training path; no counterpart in the reference):
 * `refs` = device array of `ntensors` records {const float* src [rows][cols]; uint16* dst [rows][ld] (or null); uint16* dstT
 * [cols][ldT] (or null); int rows, cols, ld, ldT, tile0, tiles_c} (dclip_mt_weights_record_bytes() bytes each), 64x64
 * tiles: tiles_c = ceil(max(cols, ld) / 64), tile rows = ceil(max(rows, ldT) / 64), tile0 = running sum, ascending.
 * cols, ld % 4 == 0; ldT % 8 == 0; padding (ld > cols, ldT > rows) is written as zeros. */
int dclip_mt_weights_record_bytes(void);
int dclip_mt_weights_bf16(const void* refs, int ntensors, int total_tiles, void* stream);
int dclip_rowsum_bf16(const void* x, float* out, int R, int n, int ld, void* stream);
/* Split-K bf16 GEMM for the weight gradients (few output tiles, contraction over all tokens): fp32 C [M][ldc], no
 * epilogue; `splits` K-slices per 128x128 tile write fp32 partials into the caller's workspace
 * (dclip_gemm_bf16_splitk_workspace bytes), a second kernel adds them in fixed order (deterministic).
 * dclip_gemm_bf16_splitk_plan(M, N, K) = the split count to pass (1: few enough tiles already). */
int dclip_gemm_bf16_splitk_plan(int M, int N, int K);
size_t dclip_gemm_bf16_splitk_workspace(int M, int N, int splits);
int dclip_gemm_bf16_splitk(const void* A, const void* W, float* C, int M, int N, int K, int lda, int ldw, int ldc,
                           int splits, void* workspace, size_t workspace_bytes, void* stream);
/* The same weight gradient WITHOUT the transposes: dY [K = tokens][lddy >= M] and X [K][ldx >= N] bf16 as the backward has
 * them (token-major); C [M][ldc] fp32 = dY^T X.  Split-K over the tokens on the token-major form of the ping-pong kernel
 * (operands out of LDS through the transposing read), fixed-order reduce through `workspace`
 * (dclip_gemm_bf16_splitk_workspace(M, N, splits) bytes).  dclip_gemm_bf16_wgrad_tokmajor_plan(M, N, K) = the split count to
 * pass, or 0 when this form does not apply (K % 64, M or N % 8, too few work items): transpose and use
 * dclip_gemm_bf16_splitk then.  dclip_colsum_bf16: the bias gradient sum over tokens of a bf16 [M][ldx] matrix
 * (workspace as dclip_colsum_f32_workspace). */
int dclip_gemm_bf16_wgrad_tokmajor_plan(int M, int N, int K);
int dclip_gemm_bf16_wgrad_tokmajor(const void* dY, const void* X, float* C, int M, int N, int K, int lddy, int ldx, int ldc,
                                   int splits, void* workspace, size_t workspace_bytes, void* stream);
int dclip_colsum_bf16(const void* X, float* out, int M, int N, int ldx, int accumulate, void* workspace,
                      size_t workspace_bytes, void* stream);
/* Softmax attention of the frozen towers on bf16 q/k/v (the fused projection [B*S, 3*H*64] as written by
 * dclip_gemm_bf16 with out_bf16): fp32 scores / softmax, bf16 P and context [B*S, H*64].  Forward only. */
int dclip_attention_fwd_bf16(const void* qkv, void* out, int B, int S, int H, int causal, void* stream);
/* One attention output row per sequence for the LAST layer of a frozen bf16 tower: rows == NULL -> query row 0 against all
 * S keys (only the CLS row of the final hidden state is read, hf:modeling_clip.py:650); rows [B] int32 -> query row rows[b]
 * against keys 0..rows[b] (the pooled first-EOS row of the causal text tower, hf:modeling_clip.py:574-581).
 * qkv [B*S, 3*H*64] bf16, out [B, H*64] bf16, S <= 512; fp32 scores / softmax / accumulation. */
int dclip_attention_row_fwd_bf16(const void* qkv, const int32_t* rows, void* out, int B, int S, int H, void* stream);
/* Training forms of the bf16 attention (the bf16 student of configs c3 / c5; eager_attention_forward, hf:modeling_clip.py:259-277,
 * and its gradient): bf16 q/k/v, context, d(context) and dq|dk|dv; fp32 scores, softmax and dS; P and dS rounded to bf16 for
 * the products they feed.  The forward (S <= 288, not 257) also writes lse [B*H][S] fp32 = log-sum-exp of the scaled scores;
 * the backward (S <= 64) consumes it. */
int dclip_attention_fwd_bf16_lse(const void* qkv, void* out, float* lse, int B, int S, int H, int causal, void* stream);
int dclip_attention_bwd_bf16(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, int B, int S,
                             int H, int causal, void* stream);
int dclip_layernorm_fwd_bf16(const float* x, const float* gamma, const float* beta, void* y, int rows, int D,
                             float eps, void* stream);

/* ------------------------------------------------------------------------------------------
 * Optimiser tail (pulled into the timed step).
 * sumsq / clip_coef: global-norm clipping as torch.nn.utils.clip_grad_norm_ does it, which is what Lightning's
 *   Trainer(gradient_clip_val=0.5) applies (training/CLIP_image_distill_training.py:41): each tensor writes
 *   dclip_sumsq_blocks(n) partial sums; clip_coef reduces ALL partials to coef = min(1, max_norm/(norm+1e-6))
 *   on the device (no host sync) and optionally returns the norm.
 * adamw: torch.optim.AdamW update (training/CLIP_image_distillation.py:680; decoupled weight decay, bias
 *   correction from the integer `step` >= 1); the gradient is multiplied by *grad_scale (device scalar, may be
 *   NULL) first, which is where the clip coefficient goes.
 */
int dclip_sumsq_blocks(size_t n);
int dclip_sumsq_f32(const float* x, size_t n, float* partial, void* stream);
int dclip_clip_coef(const float* partial, int n, float max_norm, float* coef, float* norm_out, void* stream);
int dclip_adamw_f32(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2,
                    float eps, float weight_decay, int step, const float* grad_scale, void* stream);
/* Multi-tensor forms: ONE launch for all parameters of a group.  `refs` is a DEVICE array of `ntensors` records of
 * dclip_mt_record_bytes() bytes each: { float* p; const float* g; float* m; float* v; uint64_t n; int32_t step;
 * int32_t chunk0; } where chunk0 is the running sum of ceil(n / dclip_mt_chunk_elems()) over the preceding
 * tensors and total_chunks the sum over all.  mt_sumsq writes one partial per chunk (feed them to dclip_clip_coef);
 * mt_adamw applies the update of dclip_adamw_f32 to every tensor. */
int dclip_mt_record_bytes(void);
int dclip_mt_chunk_elems(void);
int dclip_mt_sumsq_f32(const void* refs, int ntensors, int total_chunks, float* partial, void* stream);
int dclip_mt_adamw_f32(const void* refs, int ntensors, int total_chunks, float lr, float beta1, float beta2,
                       float eps, float weight_decay, const float* grad_scale, void* stream);
/* torch.optim.Adam (L2 coupled into the gradient: g += weight_decay * p) — replaces the teacher trainer's
 * `optim.Adam(trainable_params, lr=args.learning_rate)` (training/train_contrastive_teacher.py:245-248). */
int dclip_mt_adam_f32(const void* refs, int ntensors, int total_chunks, float lr, float beta1, float beta2,
                      float eps, float weight_decay, const float* grad_scale, void* stream);

/* ------------------------------------------------------------------------------------------
 * fp16 forward path for FROZEN towers (opt-in precision="fp16"): the bf16 forward entries above with fp16 in place of
 * bf16 — same arguments, limits and kernels (one source, templated over the 16-bit type), v_mfma_f32_*_f16 with fp32
 * accumulation at the bf16 rate, 3 more mantissa bits.  Every fp32 -> fp16 rounding is round-to-nearest-even; a FINITE
 * value beyond +-65504 saturates to +-65504, +-inf and NaN pass through unchanged.  What stays fp32 is what stays fp32 on
 * the bf16 path (scores, softmax, LayerNorm statistics, residual stream, bias, epilogue).  No training forms.
 *   gemm_f16: dclip_gemm_bf16 with fp16 A / W and, with out_f16, an fp16 C (epilogue BIAS | GELU | RESIDUAL).
 *   cast_f32_f16, layernorm_fwd_f16, im2col_f16, attention_fwd_f16, attention_row_fwd_f16: their bf16 twins, fp16 out. */
int dclip_gemm_f16(const void* A, const void* W, void* C, const float* bias, const float* residual, int M, int N, int K,
                   int lda, int ldw, int ldc, int epilogue, int out_f16, void* stream);
int dclip_cast_f32_f16(const float* x, void* y, int rows, int cols, int ldx, int ldy, void* stream);
int dclip_layernorm_fwd_f16(const float* x, const float* gamma, const float* beta, void* y, int rows, int D, float eps,
                            void* stream);
int dclip_im2col_f16(const float* pixels, void* cols, int B, int C, int Himg, int Wimg, int patch, int ldc, void* stream);
int dclip_attention_fwd_f16(const void* qkv, void* out, int B, int S, int H, int causal, void* stream);
int dclip_attention_row_fwd_f16(const void* qkv, const int32_t* rows, void* out, int B, int S, int H, void* stream);

/* ------------------------------------------------------------------------------------------
 * Split-fp16 evaluation of fp32 GEMMs for the FROZEN fp32 text tower (DCLIP_TEXT_SPLIT16): an fp32 value is
 * written as hi + lo, hi = fp16(v), lo = fp16(v - hi) (22 mantissa bits, IEEE round-to-nearest-even, NO saturation), and
 * A W^T is the one fp16 GEMM [A_hi | A_lo | A_hi] [W_hi | W_hi | W_lo]^T along K' = 3K with fp32 accumulation.
 *   split_f32_f16x3      fp32 [rows][cols] (ldx) -> fp16 [rows][3 cols] (ldy >= 3 cols, a multiple of 8; columns past 3 cols
 *                        are not written) of v = x * scale; order 0 = [hi|lo|hi] (activations), 1 = [hi|hi|lo] (weights).
 *                        cols % 8 == 0, 16-byte aligned operands, `scale` a power of two (the caller keeps |v| <= 2^14).
 *   layernorm_fwd_f16x3  dclip_layernorm_fwd's arithmetic with y [rows][3 D] fp16 = the order-0 split of scale * LN(x); the
 *                        fp32 result is not stored.  Bit-equal to split_f32_f16x3 of dclip_layernorm_fwd's output.
 *   gemm_f16_scaled      dclip_gemm_f16 with `alpha`: the accumulator is multiplied by alpha BEFORE bias, GELU and residual
 *                        (alpha = 1 / (scale_A scale_W) undoes the operand scales); alpha = 1 is dclip_gemm_f16 bit for bit.
 *   gemm_f16_scaled_split  gemm_f16_scaled (epilogue BIAS | GELU) with C fp16 [M][ldc >= 3 N, a multiple of 8] = the order-0
 *                        split of out_scale * result (a power of two): bit-equal to split_f32_f16x3 of the fp32 output. */
int dclip_split_f32_f16x3(const float* x, void* y, int rows, int cols, int ldx, int ldy, float scale, int order, void* stream);
int dclip_layernorm_fwd_f16x3(const float* x, const float* gamma, const float* beta, void* y, int rows, int D, float eps,
                              float scale, void* stream);
int dclip_gemm_f16_scaled(const void* A, const void* W, void* C, const float* bias, const float* residual, int M, int N, int K,
                          int lda, int ldw, int ldc, int epilogue, int out_f16, float alpha, void* stream);
int dclip_gemm_f16_scaled_split(const void* A, const void* W, void* C, const float* bias, int M, int N, int K, int lda, int ldw,
                                int ldc, int epilogue, float alpha, float out_scale, void* stream);

/* ------------------------------------------------------------------------------------------
 * The split-fp16 entries above for a tower whose weights CHANGE every step (the student's vision forward,
 * DCLIP_VISION_SPLIT16): the scales live in DEVICE memory, are recomputed there from the weights, and are read
 * through pointers, so that no host value goes stale in a captured graph and nothing is read back.
 *   *_dev                the entry of the same name with `const float*` (device) where it takes a float; same kernels, every
 *                        output bit-equal at equal scales.  layernorm_fwd_f16x3_dev may also write dclip_layernorm_fwd's fp32
 *                        output y32 and row statistics (each may be NULL), bit for bit; gemm_f16_scaled_split_dev may also
 *                        write the fp32 result g32 [M][N] and, with GELU, the fp32 pre-activation h32 [M][N] (each may be
 *                        NULL), bit-equal to gemm_f16_scaled's output for that epilogue; with out_scale NULL there is no split
 *                        and C is the fp32 result [M][ldc] itself (g32 NULL), h32 as before.
 *   split16_stats        one launch over a table of `nrefs` records (split16_record_bytes each: src, dst, int rows, cols, layer,
 *                        max_slot, l1_slot, l1_row0, scale_slot, tile0; tiles of split16_tile_rows rows, `tiles` in
 *                        all): max|x| and the largest row L1 norm per record into stats, uint32 [layers][12] (bit patterns of
 *                        non-negative floats; zero before the first call).  The same value in every run.
 *   split16_plan         stats -> plan, float [layers][split16_plan_floats]: [0..3] activation scales 2^e (ln1, ctx, ln2, g),
 *                        [4..7] weight scales 2^f (qkv, out, fc1, fc2), [8..11] alpha = 2^-(e+f), [12] flag bits (1: an e below
 *                        -14, 2: a non-finite statistic, 4: a scale clamped to fp32's range), [16..27] the statistics; clears
 *                        stats.  Exponents by the host rules (engine.split16_*), evaluated in double.
 *   split16_weights      the [hi|hi|lo] split of src * (its plan scale) for every record with a dst, one launch. */
int dclip_split_f32_f16x3_dev(const float* x, void* y, int rows, int cols, int ldx, int ldy, const float* scale, int order,
                              void* stream);
int dclip_layernorm_fwd_f16x3_dev(const float* x, const float* gamma, const float* beta, void* y, float* y32, float* mean,
                                  float* rstd, int rows, int D, float eps, const float* scale, void* stream);
int dclip_gemm_f16_scaled_dev(const void* A, const void* W, void* C, const float* bias, const float* residual, int M, int N, int K,
                              int lda, int ldw, int ldc, int epilogue, int out_f16, const float* alpha, void* stream);
int dclip_gemm_f16_scaled_split_dev(const void* A, const void* W, void* C, const float* bias, float* h32, float* g32, int M, int N,
                                    int K, int lda, int ldw, int ldc, int epilogue, const float* alpha, const float* out_scale,
                                    void* stream);
int dclip_split16_record_bytes(void);
int dclip_split16_plan_floats(void);
int dclip_split16_tile_rows(void);
int dclip_split16_stats(const void* refs, int nrefs, int tiles, void* stats, void* stream);
int dclip_split16_plan(void* stats, float* plan, int nlayers, int D, void* stream);
int dclip_split16_weights(const void* refs, int nrefs, int tiles, const float* plan, void* stream);

/* ------------------------------------------------------------------------------------------
 * Split-fp16 DATA-GRADIENT GEMMs of the student's vision backward (DCLIP_VISION_SPLIT16_BWD): dX = dY W with dY
 * split by ROW — it has no bound derivable from the weights, so its scale comes from the data, on the device.
 *   split_f32_f16x3_rows     x fp32 [rows][ldx >= cols] -> y fp16 [rows][3 cols] = [hi|lo|hi] of x[m] 2^e_m, and
 *                            row_alpha[m] = 2^-e_m.  r = max|x[m,:]| = mu 2^x (mu in [0.5, 1)): e_m = 14 - x clamped to
 *                            [-100, 100]; e_m = 0 when r is 0 or not finite (such a row gives non-finite pieces).  One pass, the
 *                            same result in every run.  cols % 8 == 0, ldx % 4 == 0, 16-byte aligned x / y.
 *   split16_weights_t        split16_weights that also writes, in the same launch and from the same plan scale, the transposed
 *                            copies: dst_t = device array of nrefs pointers, entry i = fp16 [cols][3 rows] of record i
 *                            ([hi|hi|lo] of (src scale)^T, bit-equal to split_f32_f16x3(order 1) of the transposed weight) or
 *                            NULL; such a record needs rows % 8 == 0.
 *   gemm_f16_scaled_rows_dev C[m][n] = epi((acc * *alpha) * row_alpha[m]), fp32 [M][ldc]; epilogue 0 or DCLIP_EPI_DGELU with the
 *                            fp32 pre-activation aux32 [M][ldc] (dclip_gemm_f32's DGELU statement).  row_alpha == 1 gives
 *                            gemm_f16_scaled_dev's output bit for bit.  Any kernel of the dispatcher but the persistent one. */
int dclip_split_f32_f16x3_rows(const float* x, void* y, float* row_alpha, int rows, int cols, int ldx, void* stream);
int dclip_split16_weights_t(const void* refs, int nrefs, int tiles, const float* plan, const void* dst_t, void* stream);
int dclip_gemm_f16_scaled_rows_dev(const void* A, const void* W, float* C, const float* aux32, int M, int N, int K, int lda, int ldw,
                                   int ldc, int epilogue, const float* alpha, const float* row_alpha, void* stream);

/* ---- the student's vision WEIGHT gradients on split-fp16 operands.  dW[n][k] = sum_m dY[m][n] X[m][k] contracts
 * over the tokens, so dY gets one power of two per COLUMN n (per row of dW), taken from the column's own maximum by the rule of
 * the row split and undone after the product.
 *   split_f32_f16x3_rows_colstats   dclip_split_f32_f16x3_rows (y, row_alpha bit-equal to it) that in the same pass over x takes the
 *                            column maxima and sums, then: col_exp[n] (int), col_alpha[n] = 2^-col_exp[n], db[n] = sum_m x[m][n]
 *                            (NULL = not wanted) and yc fp16 [rows][2 cols] = [hi|lo] of x[m][n] 2^col_exp[n].  Three launches, no
 *                            atomics, the same bits in every run.  workspace: ..._colstats_workspace(rows, cols) bytes.
 *   gemm_f16_wgrad_tokmajor_seg3    C[M][ldc] fp32 = ((sum over segments s = 0..2 of dY_s^T X_s) / *act_scale) * col_alpha[m], dY_s =
 *                            columns a_seg_s .. a_seg_s + M of dY fp16 [tokens][lddy], X_s = columns w_seg_s .. w_seg_s + N of X fp16
 *                            [tokens][ldx]; offsets are multiples of 8.  `splits` work items per tile and segment, 3 splits fp32
 *                            slabs in the workspace (dclip_gemm_f16_splitk_workspace(M, N, 3 splits)), fixed-order reduce.
 *                            _plan = the split count, 0 when the form does not apply (tokens % 64, M or N % 8). */
size_t dclip_split_f32_f16x3_rows_colstats_workspace(int rows, int cols);
int dclip_split_f32_f16x3_rows_colstats(const float* x, void* y, float* row_alpha, void* yc, int* col_exp, float* col_alpha, float* db,
                                        int rows, int cols, int ldx, void* workspace, size_t workspace_bytes, void* stream);
int dclip_gemm_f16_wgrad_tokmajor_seg3_plan(int M, int N, int tokens);
int dclip_gemm_f16_wgrad_tokmajor_seg3(const void* dY, const void* X, float* C, int M, int N, int tokens, int lddy, int ldx, int ldc,
                                       int a_seg0, int a_seg1, int a_seg2, int w_seg0, int w_seg1, int w_seg2, const float* col_alpha,
                                       const float* act_scale, int splits, void* workspace, size_t workspace_bytes, void* stream);

/* ---- dY read once: the kernels that PRODUCE a dY leave its column partials, pmax [P][cols] (bit patterns of the
 * maxima of |x|, unsigned) and psum [P][cols] (fp32 sums), partial row p from the producer's p-th row block, every word written,
 * no atomics, the same bits in every run; statistics are of the values stored.  Each producer entry is the plain entry plus the
 * two pointers, its other outputs bit-equal to the plain entry's; its _plan returns P, or 0 where the form does not exist (the
 * caller then takes the plain entry and the three-launch split).
 *   split_f32_f16x3_rows_cols_stats  the finish over the P partial rows, then ONE pass over x that writes both splits: y, row_alpha,
 *                            col_exp, col_alpha, yc bit-equal to split_f32_f16x3_rows_colstats on the same x; db (NULL = not
 *                            wanted) is another association of the same sum.
 *   gemm_f16_scaled_rows_stats_dev   gemm_f16_scaled_rows_dev on the ping-pong kernel, P = ceil(M / 256); _plan is 0 where the
 *                            dispatcher takes a register-staged kernel.
 *   attention_bwd_stats      attention_bwd for 1 < S <= 64, cols = 3 D, P = B.
 *   layernorm_bwd_stats      layernorm_bwd for D <= 1024, cols = D, P = the kernel's block count; psum's rows are the partials
 *                            dx_colsum is folded from.  workspace as layernorm_bwd (needed with dgamma / dbeta only). */
int dclip_split_f32_f16x3_rows_cols_stats(const float* x, void* y, float* row_alpha, void* yc, int* col_exp, float* col_alpha, float* db,
                                          const void* pmax, const float* psum, int P, int rows, int cols, int ldx, void* stream);
int dclip_gemm_f16_scaled_rows_stats_plan(int M, int N, int K);
int dclip_gemm_f16_scaled_rows_stats_dev(const void* A, const void* W, float* C, const float* aux32, int M, int N, int K, int lda,
                                         int ldw, int ldc, int epilogue, const float* alpha, const float* row_alpha, void* pmax,
                                         float* psum, void* stream);
int dclip_attention_bwd_stats_plan(int B, int S, int H);
int dclip_attention_bwd_stats(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv, void* pmax,
                              float* psum, int B, int S, int H, int causal, void* stream);
/* attention_bwd_rows_stats: the same for 65 <= S <= 80 (the whole-row kernel's statistics twin), cols = 3 D, P = B;
 * _plan is 0 everywhere else, and attention_bwd_stats_plan stays 0 above 64. */
int dclip_attention_bwd_rows_stats_plan(int B, int S, int H);
int dclip_attention_bwd_rows_stats(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv, void* pmax,
                                   float* psum, int B, int S, int H, int causal, void* stream);
/* colsum_segments_f32: db[c] = sum of x [B*S][cols] over the rows, summed per segment of S rows in order and folded over the B
 * segments as the finish of split_f32_f16x3_rows_cols_stats folds a producer's partials: bit-equal to that entry's db for the
 * partials of attention_bwd_stats / attention_bwd_rows_stats on the same x. */
size_t dclip_colsum_segments_f32_workspace(int B, int cols);
int dclip_colsum_segments_f32(const float* x, float* db, int B, int S, int cols, int ldx, void* workspace, size_t workspace_bytes,
                              void* stream);
int dclip_layernorm_bwd_stats_plan(int rows, int D);
int dclip_layernorm_bwd_stats(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd,
                              const float* dresidual, float* dx, float* dgamma, float* dbeta, void* pmax, float* psum, int rows, int D,
                              int accumulate_param_grads, void* workspace, size_t workspace_bytes, void* stream);

/* ---- fused split-fp16 GEMMs: the three products A_hi W_hi + A_lo W_hi + A_hi W_lo of a split GEMM out of ONE
 * staging of the four distinct pieces, where the entries above contract K' = 3 K columns (or three token-major segments) and
 * stage the hi pieces twice.  Each K-major entry is the twin of the entry named after "f16x3_": the same epilogues, scales and
 * outputs, with K the LOGICAL contraction length (a multiple of 32) and four column offsets, multiples of 8 with offset + K within
 * the leading dimension: A_hi / A_lo = columns a_hi.. / a_lo.. of A, W_hi / W_lo = columns w_hi.. / w_lo.. of W ([hi|lo|hi] with
 * [hi|hi|lo]: 0, K, 0, 2 K).  No other column is read.  The ping-pong kernel only, at any M and N; the sum is accumulated in
 * another order than the 3 K form's, so the two agree to fp32 rounding and are not bit-equal.
 *   gemm_f16x3_plan          1 exactly where the 3 K form takes the ping-pong kernel (the step then takes the twin), else 0;
 *                            also 0 below DCLIP_F16X3_MIN tiles of 256 x 256 (default 128, the dispatcher's default; read per call).
 *   gemm_f16x3_scaled_rows_stats_plan   the partial rows, ceil(M / 256), where gemm_f16x3_plan is 1, else 0.
 *   gemm_f16x3_wgrad_tokmajor   gemm_f16_wgrad_tokmajor_seg3 with the segments dY_hi^T X_hi + dY_lo^T X_hi + dY_hi^T X_lo: a work
 *                            item owns a token range (whole 64-token units) and does all three; `splits` fp32 slabs
 *                            (_workspace(M, N, splits) bytes, one split included), the same fixed-order scaled reduce.  _plan = the split
 *                            count, 0 where the form does not apply or would start fewer than 128 work items
 *                            (DCLIP_F16X3_TOK_MIN, read per call).
 *   gemm_f16x3_tile_rows     the tile height (192 or 256 rows x 256 columns) a K-major fp32-output call of this shape takes now
 *                            (DESIGN.md §9i): 192 where the 256-row tiles leave CUs idle and the 192-row tiles fit the same number
 *                            of rounds.  rows_form: the row-scaled entry; stats_form: its statistics twin, which has the 256-row
 *                            tile only, as the split-output and 16-bit-output calls have.  DCLIP_F16X3_BM192 = 0 never / 1 by the
 *                            rule (default) / 2 wherever the form has the tile; DCLIP_F16X3_BM192_MIN (default 128 tiles of 256 x
 *                            256), both read per call.  The outputs are bit-equal at both heights. */
int dclip_gemm_f16x3_plan(int M, int N, int K);
int dclip_gemm_f16x3_tile_rows(int M, int N, int K, int rows_form, int stats_form);
int dclip_gemm_f16x3_scaled(const void* A, const void* W, void* C, const float* bias, const float* residual, int M, int N, int K,
                            int lda, int ldw, int ldc, int a_hi, int a_lo, int w_hi, int w_lo, int epilogue, int out_f16, float alpha,
                            void* stream);
int dclip_gemm_f16x3_scaled_split(const void* A, const void* W, void* C, const float* bias, int M, int N, int K, int lda, int ldw,
                                  int ldc, int a_hi, int a_lo, int w_hi, int w_lo, int epilogue, float alpha, float out_scale,
                                  void* stream);
int dclip_gemm_f16x3_scaled_dev(const void* A, const void* W, void* C, const float* bias, const float* residual, int M, int N, int K,
                                int lda, int ldw, int ldc, int a_hi, int a_lo, int w_hi, int w_lo, int epilogue, int out_f16,
                                const float* alpha, void* stream);
int dclip_gemm_f16x3_scaled_split_dev(const void* A, const void* W, void* C, const float* bias, float* h32, float* g32, int M, int N,
                                      int K, int lda, int ldw, int ldc, int a_hi, int a_lo, int w_hi, int w_lo, int epilogue,
                                      const float* alpha, const float* out_scale, void* stream);
int dclip_gemm_f16x3_scaled_rows_dev(const void* A, const void* W, float* C, const float* aux32, int M, int N, int K, int lda, int ldw,
                                     int ldc, int a_hi, int a_lo, int w_hi, int w_lo, int epilogue, const float* alpha,
                                     const float* row_alpha, void* stream);
int dclip_gemm_f16x3_scaled_rows_stats_plan(int M, int N, int K);
int dclip_gemm_f16x3_scaled_rows_stats_dev(const void* A, const void* W, float* C, const float* aux32, int M, int N, int K, int lda,
                                           int ldw, int ldc, int a_hi, int a_lo, int w_hi, int w_lo, int epilogue, const float* alpha,
                                           const float* row_alpha, void* pmax, float* psum, void* stream);
int dclip_gemm_f16x3_wgrad_tokmajor_plan(int M, int N, int tokens);
size_t dclip_gemm_f16x3_wgrad_tokmajor_workspace(int M, int N, int splits);
int dclip_gemm_f16x3_wgrad_tokmajor(const void* dY, const void* X, float* C, int M, int N, int tokens, int lddy, int ldx, int ldc,
                                    int dy_hi, int dy_lo, int x_hi, int x_lo, const float* col_alpha, const float* act_scale,
                                    int splits, void* workspace, size_t workspace_bytes, void* stream);

/* ---- two-piece operands: no fused entry reads the duplicate third of an [hi|lo|hi] operand, so each producer of
 * one has a twin that writes fp16 [rows][2 cols] = [hi|lo] and nothing else — hi and lo bit-equal to the first two pieces of the
 * entry named after "f16x2" / before "split2", every other output (row_alpha, yc, col_exp, col_alpha, db, y32, mean, rstd, h32, g32)
 * bit-equal to that entry's, the same limits.  The consumers are the fused entries above as they are: K-major with lda = 2 K and
 * offsets (0, K, 0, 2 K) — the weights stay [hi|hi|lo] — token-major with ldx = 2 N and (x_hi, x_lo) = (0, N); the segmented
 * gemm_f16_wgrad_tokmajor_seg3 reads it with w_seg = (0, 0, N).  The 3 K entries (gemm_f16_scaled*) cannot read it.
 *   split_f32_f16x2, layernorm_fwd_f16x2   order-0 split / LayerNorm; `scale` (a power of two) or, when not NULL, the device
 *                            float scale_dev; ldy >= 2 cols.  layernorm's y32 / mean / rstd may be NULL.
 *   split_f32_f16x2_rows, _rows_colstats, _rows_cols_stats   the row-scaled splits (the last keeps its non-temporal stores).
 *   gemm_f16x3_scaled_split2(_dev)   C fp16 [M][ldc >= 2 N, a multiple of 8]; out_scale is required (BIAS | GELU).
 * dclip_last_launch / dclip_first_launch report a two-piece entry under its three-piece twin's name and variant: the call site of
 * the step is the same, and which layout it wrote shows in the tensor's width. */
int dclip_split_f32_f16x2(const float* x, void* y, int rows, int cols, int ldx, int ldy, float scale, const float* scale_dev,
                          void* stream);
/*   quick_gelu_f32           g[i] = quick_gelu(h[i]), n fp32 values (n % 4 == 0, 16-byte aligned): bit-equal to the g32 a GELU epilogue of
 *                            the split-output entries stores beside that h32 — what a backward makes again where the forward did
 *                            not keep the fp32 g. */
int dclip_quick_gelu_f32(const float* h, float* g, size_t n, void* stream);
int dclip_layernorm_fwd_f16x2(const float* x, const float* gamma, const float* beta, void* y, float* y32, float* mean, float* rstd,
                              int rows, int D, float eps, float scale, const float* scale_dev, void* stream);
int dclip_split_f32_f16x2_rows(const float* x, void* y, float* row_alpha, int rows, int cols, int ldx, void* stream);
int dclip_split_f32_f16x2_rows_colstats(const float* x, void* y, float* row_alpha, void* yc, int* col_exp, float* col_alpha, float* db,
                                        int rows, int cols, int ldx, void* workspace, size_t workspace_bytes, void* stream);
int dclip_split_f32_f16x2_rows_cols_stats(const float* x, void* y, float* row_alpha, void* yc, int* col_exp, float* col_alpha, float* db,
                                          const void* pmax, const float* psum, int P, int rows, int cols, int ldx, void* stream);
int dclip_gemm_f16x3_scaled_split2(const void* A, const void* W, void* C, const float* bias, int M, int N, int K, int lda, int ldw,
                                   int ldc, int a_hi, int a_lo, int w_hi, int w_lo, int epilogue, float alpha, float out_scale,
                                   void* stream);
int dclip_gemm_f16x3_scaled_split2_dev(const void* A, const void* W, void* C, const float* bias, float* h32, float* g32, int M, int N,
                                       int K, int lda, int ldw, int ldc, int a_hi, int a_lo, int w_hi, int w_lo, int epilogue,
                                       const float* alpha, const float* out_scale, void* stream);

/* ---- the student's patch embedding and its weight gradient on split operands.  No GEMM of their own: the forward
 * is dclip_gemm_f16x3_scaled_dev with lda = 2 K and offsets (0, K, 0, 2 K), the weight gradient dclip_gemm_f16x3_wgrad_tokmajor
 * with (0, D), (0, K) — fc2's call forms — on the operands these entries write.
 *   im2col_f16x2           dclip_im2col's gather written as fp16 [rows][2 C p p] = [hi|lo] of pixel * scale (a power of two) or,
 *                          when not NULL, * the device float scale_dev: bit-equal to dclip_split_f32_f16x2 of dclip_im2col's
 *                          output, one pass, no fp32 columns.  Square images, patch % 8 == 0, both operands 16-byte aligned.
 *                          Launch name "im2col_f16x2".
 *   split16_front          the front plan: rec float [split16_front_rec_floats] = 2^e | 2^f | alpha = 2^-(e+f) | flag bits | max|pixels| |
 *                          max|w| | e | f (ints), e = engine.split16_act_exp(max|pixels|), f = engine.split16_weight_exp(max|w|),
 *                          evaluated in double as dclip_split16_plan does, with its flag bits (1: e < -14; 2: a non-finite maximum —
 *                          e resp. f is then 0; 4: a scale outside fp32's normal range, clamped).  refresh_w != 0: max|w| is taken
 *                          too, wrec float [split16_front_wrec_floats] = 2^f | f | max|w| | the weight's flags is rewritten and w3 fp16
 *                          [wrows][3 wcols] = [hi|hi|lo] of w 2^f, bit-equal to dclip_split_f32_f16x3(order 1) at that scale
 *                          (wcols % 8 == 0; w, w3 16-byte aligned); refresh_w == 0: wrec is read as the last such call left it and
 *                          w / w3 may be NULL.  npix values at pixels (16-byte aligned), any count.  Two launches, three with
 *                          refresh_w; no atomics, nothing read back, the same bits in every run.  workspace: split16_front_workspace
 *                          bytes, 16-byte aligned.  Launch names "split16_front.max", ".plan", ".weight".
 *   split_f32_f16x2_cols   the column-only split of a dY: col_exp, col_alpha and yc fp16 [rows][2 cols] bit-equal to the outputs of
 *                          those names of dclip_split_f32_f16x2_rows_colstats on the same x; no row pieces, no db.  The same limits
 *                          (cols % 8 == 0, ldx % 4 == 0, 16-byte alignment); three launches (".max", ".finish", ".cols"), no
 *                          atomics.  workspace: split_f32_f16x2_cols_workspace(rows, cols) bytes.
 *   split16_patch_plan     1 where the step takes this path for a patch embedding [rows, K] x [D, K]: dclip_gemm_f16x3_plan holds
 *                          and the call has at least DCLIP_PATCH_SPLIT16_MIN (default 128; read per call) tiles of 256 x 256. */
int dclip_im2col_f16x2(const float* pixels, void* cols, int B, int C, int Himg, int Wimg, int patch, float scale,
                       const float* scale_dev, void* stream);
int dclip_split16_front_rec_floats(void);
int dclip_split16_front_wrec_floats(void);
size_t dclip_split16_front_workspace(void);
int dclip_split16_front(const float* pixels, size_t npix, const float* w, int wrows, int wcols, void* w3, float* wrec, float* rec,
                        void* workspace, size_t workspace_bytes, int refresh_w, void* stream);
size_t dclip_split_f32_f16x2_cols_workspace(int rows, int cols);
int dclip_split_f32_f16x2_cols(const float* x, void* yc, int* col_exp, float* col_alpha, int rows, int cols, int ldx, void* workspace,
                               size_t workspace_bytes, void* stream);
int dclip_split16_patch_plan(int rows, int D, int K);

/* ---- attention forward that writes its context ALREADY SPLIT (the frozen towers at precision "fp32-split16"):
 * the context of a frozen split-fp16 layer is read by one consumer, the split out-projection, so the fp32 [T][D] round trip
 * through dclip_split_f32_f16x2 / _f16x3 is folded into the attention kernel's store.
 *   y fp16 [rows][ldy >= pieces H 64] = [hi|lo] (pieces 2) or [hi|lo|hi] (pieces 3) of scale * context, scale a power of two:
 *   hi = fp16(v), lo = fp16(v - hi), v = context * scale with the fp32 context dclip_attention_fwd / dclip_attention_varlen_fwd /
 *   dclip_attention_varlen_causal_fwd stores — bit-equal to that entry followed by the stand-alone split (order 0), NaN for NaN.
 *   Columns past pieces H 64 of a row are not written.  No lse: forward only.
 *   attention_fwd_f16x2          qkv [B*S][3 H 64]; the whole-row kernel for S <= 80, the streamed kernel above (DCLIP_ATTN_TILED is
 *                                not read: there is no tiled form); ldy % 4 == 0, qkv 16-byte and y 8-byte aligned.
 *   attention_varlen_fwd_f16x2   packed sequences, every row a query; causal = 0: attention_varlen_fwd, 1: _causal_fwd; the table
 *                                is clamped as there; qkv 16-byte aligned.
 * Each refuses a null pointer, a non-positive dimension, pieces outside {2, 3}, a short ldy and a scale that is not a power of
 * two with DCLIP_EINVAL before any launch. */
int dclip_attention_fwd_f16x2(const float* qkv, void* y, int B, int S, int H, int causal, float scale, int pieces, int ldy,
                              void* stream);
int dclip_attention_varlen_fwd_f16x2(const float* qkv, const int32_t* cu_seqlens, void* y, int N, int max_S, int H, int causal,
                                     float scale, int pieces, int ldy, void* stream);

/* ------------------------------------------------------------------------------------------
 * fp16 TRAINING path (opt-in student_precision="fp16" / get_image_features(precision="fp16-mixed")): fp16
 * twins of the bf16 training entries above — same arguments, limits and kernels — with plain IEEE round-to-nearest-even:
 * a finite value beyond +-65504 becomes +-inf (it does NOT saturate as the frozen fp16 entries do), NaN stays NaN, so the
 * overflow of a loss-scaled gradient reaches the gradient norm and the loss scaler skips the step.  Only the kernels of the
 * default plans have fp16 training instances: DCLIP_BF16_PERSIST does not apply to these entries.
 *   gemm_f16_ex                  dclip_gemm_bf16_ex (aux = the fp16 GELU pre-activation / dGELU input).
 *   gemm_f16_wgrad_tokmajor(_plan), gemm_f16_splitk(_plan, _workspace)   the weight-gradient forms.
 *   cast_f32_f16_ieee            dclip_cast_f32_f16 with IEEE rounding (fp32 gradients -> fp16).
 *   layernorm_fwd_f16_stats, layernorm_bwd_ex_f16 (dx_f16 = the fp16 copy of dx), transpose_to_f16, rowsum_f16,
 *   colsum_f16, mt_weights_f16 (records of dclip_mt_weights_record_bytes(), fp16 destinations).
 *   attention_fwd_f16_lse / attention_bwd_f16   S <= 64 both; P and dS rounded to fp16 for the products they feed. */
int dclip_gemm_f16_ex(const void* A, const void* W, void* C, const float* bias, const float* residual, void* aux, int M,
                      int N, int K, int lda, int ldw, int ldc, int epilogue, int out_f16, void* stream);
int dclip_gemm_f16_wgrad_tokmajor_plan(int M, int N, int K);
int dclip_gemm_f16_wgrad_tokmajor(const void* dY, const void* X, float* C, int M, int N, int K, int lddy, int ldx, int ldc,
                                  int splits, void* workspace, size_t workspace_bytes, void* stream);
int dclip_gemm_f16_splitk_plan(int M, int N, int K);
size_t dclip_gemm_f16_splitk_workspace(int M, int N, int splits);
int dclip_gemm_f16_splitk(const void* A, const void* W, float* C, int M, int N, int K, int lda, int ldw, int ldc, int splits,
                          void* workspace, size_t workspace_bytes, void* stream);
int dclip_cast_f32_f16_ieee(const float* x, void* y, int rows, int cols, int ldx, int ldy, void* stream);
int dclip_layernorm_fwd_f16_stats(const float* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                                  int rows, int D, float eps, void* stream);
int dclip_layernorm_bwd_ex_f16(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd,
                               const float* dresidual, float* dx, void* dx_f16, float* dgamma, float* dbeta, float* dx_colsum,
                               int rows, int D, int accumulate_param_grads, void* workspace, size_t workspace_bytes,
                               void* stream);
int dclip_transpose_to_f16(const void* x, int x_is_f16, void* yT, void* y_copy, int rows, int cols, int ldx, int ldyT,
                           int ldy, void* stream);
int dclip_rowsum_f16(const void* x, float* out, int R, int n, int ld, void* stream);
int dclip_colsum_f16(const void* X, float* out, int M, int N, int ldx, int accumulate, void* workspace,
                     size_t workspace_bytes, void* stream);
int dclip_mt_weights_f16(const void* refs, int ntensors, int total_tiles, void* stream);
int dclip_attention_fwd_f16_lse(const void* qkv, void* out, float* lse, int B, int S, int H, int causal, void* stream);
int dclip_attention_bwd_f16(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, int B, int S,
                            int H, int causal, void* stream);
/* Dynamic loss scaling on the device (torch.amp.GradScaler semantics; dclip_amd/amp.py).  No pass over the gradients of its
 * own: the partial sums of dclip_mt_sumsq_f32 over the SCALED gradients feed
 *   clip_coef_scaled  out[3] = { unscaled norm, found_inf (1 when the norm is not finite), min(1, max_norm/(norm+1e-6))/scale
 *                     or 0 with found_inf }: the unscaling folded into the clip coefficient (*scale is read on the device);
 *   mt_adamw_f32_skip dclip_mt_adamw_f32 with grad_scale = that out[3]: coefficient out[2]; returns without writing anything
 *                     (parameters, moments, weight decay) when out[1] is set.  Takes 1 - beta1 / 1 - beta2 (computed in
 *                     double by the caller, as torch does) in place of the betas;
 *   amp_update_scale  torch's _amp_update_scale_ on one lane: found_inf -> scale *= backoff, tracker = 0; otherwise
 *                     tracker + 1 == interval -> scale *= growth (if finite), tracker = 0; else tracker += 1. */
int dclip_clip_coef_scaled(const float* partial, int n, float max_norm, const float* scale, float* out, void* stream);
int dclip_mt_adamw_f32_skip(const void* refs, int ntensors, int total_chunks, float lr, float one_minus_beta1,
                            float one_minus_beta2, float eps, float weight_decay, const float* coef3, void* stream);
int dclip_amp_update_scale(float* scale, int* growth_tracker, const float* found_inf, float growth_factor,
                           float backoff_factor, int growth_interval, void* stream);

/* ------------------------------------------------------------------------------------------
 * Small elementwise helpers used between the ops above (all fp32, 16-byte vectorised).
 */
int dclip_axpby(const float* x, float* y, float a, float b, size_t n, void* stream); /* y = a*x + b*y */
int dclip_fill(float* y, float v, size_t n, void* stream);

/* ------------------------------------------------------------------------------------------
 * Exact (erf) GELU for hidden_act = "gelu" towers: stand-alone element-wise passes behind a bias-only fc1 GEMM;
 * every GEMM epilogue stays quick-GELU.  gelu(h) = h Phi(h) with Phi(h) = 0.5 (1 + erf(h / sqrt 2)), evaluated as 0.5 erfc(-h /
 * sqrt 2) for h < 0; gelu'(h) = Phi(h) + h phi(h), phi(h) = exp(-h^2 / 2) / sqrt(2 pi).  All arithmetic fp32; finite inputs only.
 * Any n >= 1 (16-byte vector body, scalar tail, size_t indexing: n may exceed 2^32); every pointer 16-byte aligned.
 *   gelu_erf_f32            g[i] = gelu(h[i]); g may be h.
 *   gelu_erf_bf16 / _f16    the same of n 16-bit values: gelu of the stored 16-bit value in fp32, rounded to nearest even (fp16:
 *                           IEEE, no saturation — |gelu(h)| <= |h|); g may be h.
 *   gelu_erf_bwd_f32        dh[i] = dg[i] gelu'(h[i]); dh may be dg.
 */
int dclip_gelu_erf_f32(const float* h, float* g, size_t n, void* stream);
int dclip_gelu_erf_bf16(const void* h, void* g, size_t n, void* stream);
int dclip_gelu_erf_f16(const void* h, void* g, size_t n, void* stream);
int dclip_gelu_erf_bwd_f32(const float* h, const float* dg, float* dh, size_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DCLIP_HIP_H */
