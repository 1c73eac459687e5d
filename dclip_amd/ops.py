"""Tensor-level wrappers over the C ABI (no autograd here; see functional.py).

PyTorch is plumbing only: it owns device memory and the HIP stream.  Every wrapper checks
device / dtype / contiguity on the host before a kernel sees a pointer — a faulting kernel
can reset the whole GPU host (shape checks are cheap, resets are not).
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib

A_KMAJOR, B_KMAJOR = 1, 2
EPI_BIAS, EPI_GELU, EPI_DGELU, EPI_RESIDUAL, EPI_ACCUM, EPI_A_ROWSUM = 1, 2, 4, 8, 16, 32
LAYOUT_NT = A_KMAJOR | B_KMAJOR     # y = x W^T
LAYOUT_NN = A_KMAJOR                # dx = dy W
LAYOUT_TN = 0                       # dW = dy^T x


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _f32(t: torch.Tensor, name: str) -> torch.Tensor:
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise ValueError(f"{name}: expected a contiguous float32 CUDA tensor, got {t.dtype} {t.device} "
                         f"contiguous={t.is_contiguous()}")
    return t


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


class _Workspace:
    """Grow-only scratch buffer per device (the library never allocates).  ONE buffer per device, whatever the stream:
    every launch sequence of this package runs on one stream at a time (a side stream only inside GraphedStep's
    warm-up, ordered by stream waits), and a buffer keyed by stream would be (re)allocated INSIDE a HIP-graph capture
    — from the graph's private pool, cached here beyond the graph's life and handed to the next capture on the same
    stream handle (seen as a 2e-4 drift of a replayed trainer after graph -> eager -> graph).  Outgrown buffers are
    kept alive (`retired`): a captured graph may still hold their address."""

    def __init__(self):
        self.buf = {}
        self.retired = []

    def get(self, nbytes: int, device) -> Optional[torch.Tensor]:
        if nbytes == 0:
            return None
        key = device.index
        b = self.buf.get(key)
        if b is None or b.numel() < nbytes:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("workspace growth inside a HIP-graph capture: run the step eagerly once before "
                                   "capturing (GraphedStep does)")
            if b is not None:
                self.retired.append(b)
            b = torch.empty(max(nbytes, 2 * (b.numel() if b is not None else 0), 1 << 20), dtype=torch.uint8, device=device)
            self.buf[key] = b
        return b


_ws = _Workspace()
_ws_lanes = {0: _ws}


class workspace_lane:
    """Launch sequences that run CONCURRENTLY on different streams must not share scratch memory (split-K slabs,
    LayerNorm / column-sum partials): `with ops.workspace_lane(1): ...` gives the enclosed launches a workspace of their
    own (grow-only like lane 0; sized by an eager warm-up before any HIP-graph capture)."""

    def __init__(self, lane: int):
        self.lane = lane

    def __enter__(self):
        global _ws
        self.prev = _ws
        _ws = _ws_lanes.setdefault(self.lane, _Workspace())
        return self

    def __exit__(self, *exc):
        global _ws
        _ws = self.prev
        return False


class ColStats:
    """Column partials of an fp32 dY left by the kernel that produced it: pmax int32 [P, cols] (bit patterns of
    the maxima of |x|), psum fp32 [P, cols].  Views into a persistent buffer of the current workspace lane that lives beside the
    lane's scratch: ONE set per lane, valid from the producer's launch to the split_f16x3_rows_cols_stats that consumes it —
    the next launch sequence of the backward, so nothing else asks for a set in between."""
    __slots__ = ("pmax", "psum", "P", "cols")

    def __init__(self, P: int, cols: int, device):
        ws = _stats_lanes.setdefault(id(_ws), _Workspace()).get(2 * P * cols * 4, device)
        self.pmax = ws[:P * cols * 4].view(torch.int32).view(P, cols)
        self.psum = ws[P * cols * 4:2 * P * cols * 4].view(torch.float32).view(P, cols)
        self.P, self.cols = P, cols

    @classmethod
    def of(cls, pmax: torch.Tensor, psum: torch.Tensor) -> "ColStats":
        """Partials in the caller's own contiguous tensors (int32 / fp32 [P, cols])."""
        if pmax.dtype != torch.int32 or psum.dtype != torch.float32 or pmax.shape != psum.shape or pmax.dim() != 2 or \
                not (pmax.is_contiguous() and psum.is_contiguous() and pmax.is_cuda and psum.is_cuda):
            raise ValueError("ColStats.of: pmax int32 / psum fp32, contiguous device tensors of one shape [P, cols]")
        st = cls.__new__(cls)
        st.pmax, st.psum, (st.P, st.cols) = pmax, psum, pmax.shape
        return st


_stats_lanes = {}


# ------------------------------------------------------------------------------------------- GEMM

def gemm(a: torch.Tensor, b: torch.Tensor, layout: int, *, out: Optional[torch.Tensor] = None,
         bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
         aux: Optional[torch.Tensor] = None, epilogue: int = 0, alpha: float = 1.0, split_k: int = 0,
         a_rowsum: Optional[torch.Tensor] = None) -> torch.Tensor:
    """C = epilogue(alpha * op(a) @ op(b)); see include/dclip_hip.h for layout / epilogue bits.
    `a_rowsum` (float[M], [K][M]-major A only) additionally receives sum_k A[m,k]: the bias gradient of a wgrad."""
    lib = _lib.load()
    _f32(a, "a"), _f32(b, "b")
    if a.dim() != 2 or b.dim() != 2:
        raise ValueError("gemm: 2-D operands")
    if layout & A_KMAJOR:
        M, K = a.shape
    else:
        K, M = a.shape
    if layout & B_KMAJOR:
        N, Kb = b.shape
    else:
        Kb, N = b.shape
    if K != Kb:
        raise ValueError(f"gemm: contraction mismatch {tuple(a.shape)} x {tuple(b.shape)} layout={layout}")
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    _f32(out, "out")
    if tuple(out.shape) != (M, N):
        raise ValueError(f"gemm: out shape {tuple(out.shape)} != {(M, N)}")
    if bias is not None:
        epilogue |= EPI_BIAS
        if _f32(bias, "bias").numel() != N:
            raise ValueError("gemm: bias size")
    if residual is not None:
        epilogue |= EPI_RESIDUAL
        if tuple(_f32(residual, "residual").shape) != (M, N):
            raise ValueError("gemm: residual shape")
    if aux is not None and tuple(_f32(aux, "aux").shape) != (M, N):
        raise ValueError("gemm: aux shape")
    if a_rowsum is not None:
        if aux is not None or (layout & A_KMAJOR) or _f32(a_rowsum, "a_rowsum").numel() != M:
            raise ValueError("gemm: a_rowsum needs a [K][M]-major A, no aux, and M elements")
        epilogue |= EPI_A_ROWSUM
        aux = a_rowsum
    nbytes = lib.dclip_gemm_f32_workspace(M, N, K, layout, split_k)
    ws = _ws.get(nbytes, a.device)
    _lib.check(lib.dclip_gemm_f32(a.data_ptr(), b.data_ptr(), out.data_ptr(), _ptr(bias), _ptr(residual),
                                  _ptr(aux), M, N, K, a.shape[1], b.shape[1], N, layout, epilogue,
                                  float(alpha), split_k, _ptr(ws), nbytes, _stream()), "gemm_f32")
    return out


def colsum(x: torch.Tensor, out: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    lib = _lib.load()
    _f32(x, "x")
    M, N = x.shape
    if out is None:
        out = torch.empty((N,), dtype=torch.float32, device=x.device)
        accumulate = False
    _f32(out, "out")
    if out.numel() != N:
        raise ValueError("colsum: out size")
    nbytes = lib.dclip_colsum_f32_workspace(M, N)
    ws = _ws.get(nbytes, x.device)
    _lib.check(lib.dclip_colsum_f32(x.data_ptr(), out.data_ptr(), M, N, N, int(accumulate), _ptr(ws), nbytes,
                                    _stream()), "colsum")
    return out


def colsum_segments(x: torch.Tensor, B: int, S: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Column sums of x [B*S, cols] summed per segment of S rows in order and folded over the B segments as the finish of
    split_f16x3_rows_cols_stats folds a producer's partials: the db of that entry for the partials attention_bwd leaves with
    `stats` / `rows_stats` on the same x, bit for bit."""
    lib = _lib.load()
    if x.dtype != torch.float32 or not x.is_cuda or x.dim() != 2 or x.stride(1) != 1 or x.shape[0] != B * S:
        raise ValueError("colsum_segments: x must be a 2-D fp32 device tensor [B*S, cols] with unit column stride")
    N = x.shape[1]
    if out is None:
        out = torch.empty((N,), dtype=torch.float32, device=x.device)
    if _f32(out, "out").numel() != N:
        raise ValueError("colsum_segments: out size")
    nbytes = lib.dclip_colsum_segments_f32_workspace(B, N)
    ws = _ws.get(nbytes, x.device)
    _lib.check(lib.dclip_colsum_segments_f32(x.data_ptr(), out.data_ptr(), B, S, N, x.stride(0), _ptr(ws), nbytes, _stream()),
               "colsum_segments")
    return out


# ------------------------------------------------------------------------------------------- LayerNorm

def layernorm_fwd(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, save_stats: bool = True):
    lib = _lib.load()
    _f32(x, "x"), _f32(gamma, "gamma"), _f32(beta, "beta")
    D = x.shape[-1]
    rows = x.numel() // D
    if gamma.numel() != D or beta.numel() != D:
        raise ValueError("layernorm: gamma/beta size")
    y = torch.empty_like(x)
    mean = torch.empty((rows,), dtype=torch.float32, device=x.device) if save_stats else None
    rstd = torch.empty((rows,), dtype=torch.float32, device=x.device) if save_stats else None
    _lib.check(lib.dclip_layernorm_fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), _ptr(mean),
                                       _ptr(rstd), rows, D, float(eps), _stream()), "layernorm_fwd")
    return y, mean, rstd


def layernorm_bwd(dy, x, gamma, mean, rstd, *, dresidual=None, dgamma=None, dbeta=None, accumulate=False,
                  need_param_grads=True, want_bf16: bool = False, dx_colsum: Optional[torch.Tensor] = None,
                  dtype16: torch.dtype = torch.bfloat16, stats: Optional[ColStats] = None):
    """Returns (dx, dgamma, dbeta); dgamma/dbeta are written (or accumulated into) if requested.
    `stats` (a ColStats of layernorm_bwd_stats_plan(rows, D) partial rows, > 0): the kernel also leaves the column partials of
    dx there; dx, dgamma, dbeta are bit-equal to the call without.
    16-bit training path: `want_bf16` -> returns (dx, dgamma, dbeta, dx16) with the 16-bit copy of dx (`dtype16`: bf16, or
    fp16 with IEEE rounding) from the same pass; `dx_colsum` [D] receives the column sums of dx (the bias gradient of the
    Linear that produced LayerNorm's input)."""
    lib = _lib.load()
    _f32(dy, "dy"), _f32(x, "x"), _f32(gamma, "gamma"), _f32(mean, "mean"), _f32(rstd, "rstd")
    D = x.shape[-1]
    rows = x.numel() // D
    if dy.shape != x.shape or mean.numel() != rows or rstd.numel() != rows or gamma.numel() != D:
        raise ValueError("layernorm_bwd: shape mismatch")
    if dresidual is not None and _f32(dresidual, "dresidual").shape != x.shape:
        raise ValueError("layernorm_bwd: dresidual shape")
    dx = torch.empty_like(x)
    if need_param_grads:
        if dgamma is None:
            dgamma = torch.empty_like(gamma)
            dbeta = torch.empty_like(gamma)
            accumulate = False
        _f32(dgamma, "dgamma"), _f32(dbeta, "dbeta")
        if dgamma.numel() != D or dbeta.numel() != D:
            raise ValueError("layernorm_bwd: dgamma/dbeta size")
    else:
        dgamma = dbeta = None
    if dx_colsum is not None and (_f32(dx_colsum, "dx_colsum").numel() != D):
        raise ValueError("layernorm_bwd: dx_colsum size")
    nbytes = lib.dclip_layernorm_bwd_workspace(rows, D) if (need_param_grads or dx_colsum is not None) else 0
    ws = _ws.get(nbytes, x.device)
    if stats is not None:
        if want_bf16 or dx_colsum is not None or (stats.P, stats.cols) != (layernorm_bwd_stats_plan(rows, D), D) or stats.P == 0:
            raise ValueError("layernorm_bwd: stats go with the plain fp32 call and layernorm_bwd_stats_plan's row count")
        _lib.check(lib.dclip_layernorm_bwd_stats(dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                                 _ptr(dresidual), dx.data_ptr(), _ptr(dgamma), _ptr(dbeta), stats.pmax.data_ptr(),
                                                 stats.psum.data_ptr(), rows, D, int(accumulate), _ptr(ws), nbytes, _stream()),
                   "layernorm_bwd_stats")
        return dx, dgamma, dbeta
    if not want_bf16 and dx_colsum is None:
        _lib.check(lib.dclip_layernorm_bwd(dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), mean.data_ptr(),
                                           rstd.data_ptr(), _ptr(dresidual), dx.data_ptr(), _ptr(dgamma), _ptr(dbeta),
                                           rows, D, int(accumulate), _ptr(ws), nbytes, _stream()), "layernorm_bwd")
        return dx, dgamma, dbeta
    if dtype16 not in (torch.bfloat16, torch.float16):
        raise ValueError(f"layernorm_bwd: dtype16 {dtype16}")
    dx16 = torch.empty(x.shape, dtype=dtype16, device=x.device) if want_bf16 else None
    entry = lib.dclip_layernorm_bwd_ex if dtype16 == torch.bfloat16 else lib.dclip_layernorm_bwd_ex_f16
    _lib.check(entry(dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                          _ptr(dresidual), dx.data_ptr(), _ptr(dx16), _ptr(dgamma), _ptr(dbeta),
                                          _ptr(dx_colsum), rows, D, int(accumulate), _ptr(ws), nbytes, _stream()),
               "layernorm_bwd_ex")
    return (dx, dgamma, dbeta, dx16) if want_bf16 else (dx, dgamma, dbeta)


def layernorm_bwd_stats_plan(rows: int, D: int) -> int:
    """Partial rows layernorm_bwd leaves with `stats`, 0 where that form does not exist (D > 1024)."""
    return int(_lib.load().dclip_layernorm_bwd_stats_plan(rows, D))


# ------------------------------------------------------------------------------------------- attention

def attention_fwd(qkv: torch.Tensor, B: int, S: int, H: int, causal: bool):
    lib = _lib.load()
    _f32(qkv, "qkv")
    if qkv.numel() != B * S * 3 * H * 64:
        raise ValueError(f"attention_fwd: qkv has {qkv.numel()} elements, expected B*S*3*H*64 = {B * S * 3 * H * 64}")
    out = torch.empty((B * S, H * 64), dtype=torch.float32, device=qkv.device)
    lse = torch.empty((B, H, S), dtype=torch.float32, device=qkv.device)
    _lib.check(lib.dclip_attention_fwd(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), B, S, H, int(causal),
                                       _stream()), "attention_fwd")
    return out, lse


def _split_ctx_out(what: str, rows: int, D: int, pieces: int, out: Optional[torch.Tensor], device) -> torch.Tensor:
    """The fp16 destination of an attention forward that writes its context split: fresh [rows, pieces D], or the caller's
    contiguous `out` [rows, ldy >= pieces D] (the columns past pieces D are left as they are)."""
    if pieces not in (2, 3):
        raise ValueError(f"{what}: pieces {pieces} (2 = [hi|lo], 3 = [hi|lo|hi])")
    if out is None:
        return torch.empty((rows, pieces * D), dtype=torch.float16, device=device)
    _f16(out, "out")
    if out.dim() != 2 or out.shape[0] != rows or out.shape[1] < pieces * D:
        raise ValueError(f"{what}: out {tuple(out.shape)}, expected [{rows}, >= {pieces * D}]")
    return out


def attention_fwd_f16x2(qkv: torch.Tensor, B: int, S: int, H: int, causal: bool, scale: float = 1.0, pieces: int = 2,
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """attention_fwd whose context leaves the kernel as the split operand of the next GEMM: fp16
    [B*S, pieces*H*64] = [hi|lo] (pieces 2) or [hi|lo|hi] (3) of scale * context (scale a power of two), bit-equal to
    split_f16x3(attention_fwd(qkv)[0], scale, pieces=pieces).  No lse: forward only.  `out`: see _split_ctx_out."""
    lib = _lib.load()
    _f32(qkv, "qkv")
    if qkv.numel() != B * S * 3 * H * 64:
        raise ValueError(f"attention_fwd_f16x2: qkv has {qkv.numel()} elements, expected B*S*3*H*64 = {B * S * 3 * H * 64}")
    y = _split_ctx_out("attention_fwd_f16x2", B * S, H * 64, pieces, out, qkv.device)
    _lib.check(lib.dclip_attention_fwd_f16x2(qkv.data_ptr(), y.data_ptr(), B, S, H, int(bool(causal)), float(scale), int(pieces),
                                             y.shape[1], _stream()), "attention_fwd_f16x2")
    return y


def attention_bwd_stats_plan(B: int, S: int, H: int) -> int:
    """Partial rows attention_bwd leaves with `stats` (B), 0 where that form does not exist (S == 1, S > 64)."""
    return int(_lib.load().dclip_attention_bwd_stats_plan(B, S, H))


def attention_bwd_rows_stats_plan(B: int, S: int, H: int) -> int:
    """Partial rows attention_bwd leaves with `rows_stats` (B) — the whole-row kernel's statistics twin, 65 <= S <= 80
     — and 0 everywhere else."""
    return int(_lib.load().dclip_attention_bwd_rows_stats_plan(B, S, H))


def attention_bwd(qkv, out, dout, lse, B: int, S: int, H: int, causal: bool, stats: Optional[ColStats] = None,
                  rows_stats: Optional[ColStats] = None):
    """`stats` (a ColStats of attention_bwd_stats_plan(B, S, H) partial rows, > 0, 3 H 64 columns): the kernel also leaves the
    column partials of dqkv there; dqkv is bit-equal to the call without.  `rows_stats`: the same for the
    65 .. 80-row form (attention_bwd_rows_stats_plan); one of the two at most."""
    lib = _lib.load()
    _f32(qkv, "qkv"), _f32(out, "out"), _f32(dout, "dout"), _f32(lse, "lse")
    if qkv.numel() != B * S * 3 * H * 64 or out.numel() != B * S * H * 64 or dout.numel() != out.numel() \
            or lse.numel() != B * H * S:
        raise ValueError("attention_bwd: shape mismatch")
    dqkv = torch.empty_like(qkv)
    if rows_stats is not None:
        if stats is not None:
            raise ValueError("attention_bwd: stats or rows_stats, not both")
        st = rows_stats
        if (st.P, st.cols) != (attention_bwd_rows_stats_plan(B, S, H), 3 * H * 64) or st.P == 0:
            raise ValueError("attention_bwd: rows_stats must have attention_bwd_rows_stats_plan's row count and 3 H 64 columns")
        _lib.check(lib.dclip_attention_bwd_rows_stats(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(),
                                                      dqkv.data_ptr(), st.pmax.data_ptr(), st.psum.data_ptr(), B, S, H, int(causal),
                                                      _stream()), "attention_bwd_rows_stats")
        return dqkv
    if stats is not None:
        if (stats.P, stats.cols) != (attention_bwd_stats_plan(B, S, H), 3 * H * 64) or stats.P == 0:
            raise ValueError("attention_bwd: stats must have attention_bwd_stats_plan's row count and 3 H 64 columns")
        _lib.check(lib.dclip_attention_bwd_stats(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), dqkv.data_ptr(),
                                                 stats.pmax.data_ptr(), stats.psum.data_ptr(), B, S, H, int(causal), _stream()),
                   "attention_bwd_stats")
        return dqkv
    # delta, and for long non-causal sequences the dS blocks the dK/dV kernel hands to the dQ kernel (include/dclip_hip.h)
    nbytes = int(lib.dclip_attention_bwd_workspace(B, S, H, int(causal)))
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=qkv.device)
    _lib.check(lib.dclip_attention_bwd_ws(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(),
                                          dqkv.data_ptr(), ws.data_ptr(), nbytes, B, S, H, int(causal), _stream()),
               "attention_bwd")
    return dqkv


def attention_cls_fwd(qkv: torch.Tensor, B: int, S: int, H: int):
    """Attention output of query row 0 of every image only: ([B, H*64], lse [B, H])."""
    lib = _lib.load()
    _f32(qkv, "qkv")
    if qkv.numel() != B * S * 3 * H * 64:
        raise ValueError("attention_cls_fwd: qkv size")
    out = torch.empty((B, H * 64), dtype=torch.float32, device=qkv.device)
    lse = torch.empty((B, H), dtype=torch.float32, device=qkv.device)
    _lib.check(lib.dclip_attention_cls_fwd(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), B, S, H, _stream()),
               "attention_cls_fwd")
    return out, lse


def attention_row_fwd(qkv: torch.Tensor, rows: torch.Tensor, B: int, S: int, H: int):
    """Causal attention output of ONE row per batch (sequence position rows[b]): [B, H*64]."""
    lib = _lib.load()
    _f32(qkv, "qkv"), _idx(rows, B)
    if qkv.numel() != B * S * 3 * H * 64:
        raise ValueError("attention_row_fwd: qkv size")
    out = torch.empty((B, H * 64), dtype=torch.float32, device=qkv.device)
    lse = torch.empty((B, H), dtype=torch.float32, device=qkv.device)
    _lib.check(lib.dclip_attention_row_fwd(qkv.data_ptr(), rows.data_ptr(), out.data_ptr(), lse.data_ptr(), B, S, H,
                                           _stream()), "attention_row_fwd")
    return out


def attention_cls_bwd(qkv, out, dout, lse, B: int, S: int, H: int):
    lib = _lib.load()
    _f32(qkv, "qkv"), _f32(out, "out"), _f32(dout, "dout"), _f32(lse, "lse")
    if qkv.numel() != B * S * 3 * H * 64 or out.numel() != B * H * 64 or dout.numel() != out.numel() \
            or lse.numel() != B * H:
        raise ValueError("attention_cls_bwd: shape mismatch")
    dqkv = torch.empty_like(qkv)
    _lib.check(lib.dclip_fill(dqkv.data_ptr(), 0.0, dqkv.numel(), _stream()), "fill")
    delta = torch.empty((B * H,), dtype=torch.float32, device=qkv.device)
    _lib.check(lib.dclip_attention_cls_bwd(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(),
                                           dqkv.data_ptr(), delta.data_ptr(), B, S, H, _stream()), "attention_cls_bwd")
    return dqkv


# ------------------------------------------------------------------------------------------- embeddings

def im2col(pixels: torch.Tensor, patch: int) -> torch.Tensor:
    lib = _lib.load()
    _f32(pixels, "pixel_values")
    B, Cc, Hh, Ww = pixels.shape
    if Hh != Ww or Hh % patch:
        raise ValueError(f"im2col: image {Hh}x{Ww} not a multiple of patch {patch}")
    g = Hh // patch
    cols = torch.empty((B * g * g, Cc * patch * patch), dtype=torch.float32, device=pixels.device)
    _lib.check(lib.dclip_im2col(pixels.data_ptr(), cols.data_ptr(), B, Cc, Hh, Ww, patch, _stream()), "im2col")
    return cols


def im2col_bf16(pixels: torch.Tensor, patch: int) -> torch.Tensor:
    """im2col with a bf16 result (rows padded to a multiple of 8 columns, zero filled); patch % 4 == 0."""
    lib = _lib.load()
    _f32(pixels, "pixel_values")
    B, Cc, Hh, Ww = pixels.shape
    if Hh != Ww or Hh % patch or patch % 4:
        raise ValueError(f"im2col_bf16: image {Hh}x{Ww}, patch {patch}")
    g, kdim = Hh // patch, Cc * patch * patch
    ld = (kdim + 7) // 8 * 8
    alloc = torch.zeros if ld != kdim else torch.empty
    cols = alloc((B * g * g, ld), dtype=torch.bfloat16, device=pixels.device)
    _lib.check(lib.dclip_im2col_bf16(pixels.data_ptr(), cols.data_ptr(), B, Cc, Hh, Ww, patch, ld, _stream()), "im2col_bf16")
    return cols


def vision_assemble_fwd(patch_emb, cls, pos, B: int, S: int, D: int) -> torch.Tensor:
    lib = _lib.load()
    _f32(patch_emb, "patch_emb"), _f32(cls, "class_embedding"), _f32(pos, "position_embedding")
    if patch_emb.numel() != B * (S - 1) * D or cls.numel() != D or pos.numel() != S * D:
        raise ValueError("vision_assemble_fwd: shape mismatch")
    x = torch.empty((B * S, D), dtype=torch.float32, device=patch_emb.device)
    _lib.check(lib.dclip_vision_assemble_fwd(patch_emb.data_ptr(), cls.data_ptr(), pos.data_ptr(), x.data_ptr(),
                                             B, S, D, _stream()), "vision_assemble_fwd")
    return x


def vision_assemble_bwd(dx, B: int, S: int, D: int) -> torch.Tensor:
    lib = _lib.load()
    _f32(dx, "dx")
    if dx.numel() != B * S * D:
        raise ValueError("vision_assemble_bwd: shape mismatch")
    dpatch = torch.empty((B * (S - 1), D), dtype=torch.float32, device=dx.device)
    _lib.check(lib.dclip_vision_assemble_bwd(dx.data_ptr(), dpatch.data_ptr(), B, S, D, _stream()),
               "vision_assemble_bwd")
    return dpatch


def _interp_grids(what: str, g: int, gh: int, gw: int) -> None:
    if min(g, gh, gw) < 1:
        raise ValueError(f"{what}: grids must be at least 1x1, got g={g} -> {gh}x{gw}")


def pos_interp_fwd(pos: torch.Tensor, g: int, gh: int, gw: int) -> torch.Tensor:
    """Position table [1 + g*g, D] resampled to [1 + gh*gw, D]: row 0 copied, the g x g grid bicubic (A = -0.75,
    align_corners=False, no antialiasing; weights from an fp64 evaluation)."""
    lib = _lib.load()
    _f32(pos, "position_embedding")
    _interp_grids("pos_interp_fwd", g, gh, gw)
    if pos.dim() != 2 or pos.shape[0] != 1 + g * g or pos.shape[1] % 4:
        raise ValueError(f"pos_interp_fwd: expected [1 + {g}*{g}, D % 4 == 0], got {tuple(pos.shape)}")
    out = torch.empty((1 + gh * gw, pos.shape[1]), dtype=torch.float32, device=pos.device)
    _lib.check(lib.dclip_pos_interp_fwd(pos.data_ptr(), out.data_ptr(), g, gh, gw, pos.shape[1], _stream()), "pos_interp_fwd")
    return out


def pos_interp_bwd(dout: torch.Tensor, g: int, gh: int, gw: int, out: Optional[torch.Tensor] = None,
                   accumulate: bool = False) -> torch.Tensor:
    """The transpose of pos_interp_fwd: gradient [1 + gh*gw, D] -> [1 + g*g, D], written (or with `accumulate` added) into
    `out` when given."""
    lib = _lib.load()
    _f32(dout, "dout")
    _interp_grids("pos_interp_bwd", g, gh, gw)
    if dout.dim() != 2 or dout.shape[0] != 1 + gh * gw or dout.shape[1] % 4:
        raise ValueError(f"pos_interp_bwd: expected [1 + {gh}*{gw}, D % 4 == 0], got {tuple(dout.shape)}")
    D = dout.shape[1]
    if out is None:
        if accumulate:
            raise ValueError("pos_interp_bwd: accumulate needs `out`")
        out = torch.empty((1 + g * g, D), dtype=torch.float32, device=dout.device)
    else:
        _f32(out, "out")
        if out.numel() != (1 + g * g) * D or out.device != dout.device:
            raise ValueError(f"pos_interp_bwd: out must hold [1 + {g}*{g}, {D}] on {dout.device}, got {tuple(out.shape)}")
    _lib.check(lib.dclip_pos_interp_bwd(dout.data_ptr(), out.data_ptr(), g, gh, gw, D, int(bool(accumulate)), _stream()),
               "pos_interp_bwd")
    return out


def _rect_grid(what: str, pixels: torch.Tensor, patch: int):
    _f32(pixels, "pixel_values")
    if pixels.dim() != 4:
        raise ValueError(f"{what}: expected pixel_values [B, C, H, W], got {tuple(pixels.shape)}")
    Hh, Ww = pixels.shape[2:]
    if patch < 1 or Hh < patch or Ww < patch or pixels.shape[0] < 1 or pixels.shape[1] < 1:
        raise ValueError(f"{what}: image {Hh}x{Ww} has a side shorter than one patch ({patch})")
    return Hh // patch, Ww // patch


def im2col_rect(pixels: torch.Tensor, patch: int) -> torch.Tensor:
    """im2col on a gh x gw grid (gh = H // patch, gw = W // patch; trailing rows and columns are not read)."""
    lib = _lib.load()
    gh, gw = _rect_grid("im2col_rect", pixels, patch)
    B, Cc, Hh, Ww = pixels.shape
    cols = torch.empty((B * gh * gw, Cc * patch * patch), dtype=torch.float32, device=pixels.device)
    _lib.check(lib.dclip_im2col_rect(pixels.data_ptr(), cols.data_ptr(), B, Cc, Hh, Ww, patch, _stream()), "im2col_rect")
    return cols


def _im2col_rect16(entry: str, dtype, pixels: torch.Tensor, patch: int) -> torch.Tensor:
    lib = _lib.load()
    gh, gw = _rect_grid(entry, pixels, patch)
    if patch % 4:
        raise ValueError(f"{entry}: patch {patch} must be a multiple of 4")
    B, Cc, Hh, Ww = pixels.shape
    kdim = Cc * patch * patch
    ld = (kdim + 7) // 8 * 8
    alloc = torch.zeros if ld != kdim else torch.empty
    cols = alloc((B * gh * gw, ld), dtype=dtype, device=pixels.device)
    _lib.check(getattr(lib, "dclip_" + entry)(pixels.data_ptr(), cols.data_ptr(), B, Cc, Hh, Ww, patch, ld, _stream()), entry)
    return cols


def im2col_rect_bf16(pixels: torch.Tensor, patch: int) -> torch.Tensor:
    """im2col_rect with a bf16 result (rows padded to a multiple of 8 columns, zero filled); patch % 4 == 0."""
    return _im2col_rect16("im2col_rect_bf16", torch.bfloat16, pixels, patch)


def im2col_rect_f16(pixels: torch.Tensor, patch: int) -> torch.Tensor:
    """im2col_rect with an fp16 result (rows padded to a multiple of 8 columns, zero filled); patch % 4 == 0."""
    return _im2col_rect16("im2col_rect_f16", torch.float16, pixels, patch)


def _ids(ids: torch.Tensor) -> torch.Tensor:
    if not (ids.is_cuda and ids.dtype == torch.int64 and ids.is_contiguous() and ids.dim() == 2):
        raise ValueError("input_ids: expected a contiguous int64 CUDA tensor [B, T]")
    return ids


def text_embed_fwd(ids, tok, pos) -> torch.Tensor:
    lib = _lib.load()
    _ids(ids), _f32(tok, "token_embedding"), _f32(pos, "position_embedding")
    B, T = ids.shape
    vocab, D = tok.shape
    if pos.shape[0] < T or pos.shape[1] != D:
        raise ValueError(f"text_embed_fwd: sequence {T} longer than position table {tuple(pos.shape)}")
    x = torch.empty((B * T, D), dtype=torch.float32, device=tok.device)
    _lib.check(lib.dclip_text_embed_fwd(ids.data_ptr(), tok.data_ptr(), pos.data_ptr(), x.data_ptr(), B, T, D, vocab,
                                        _stream()), "text_embed_fwd")
    return x


def text_embed_bwd(ids, dx, dtok):
    lib = _lib.load()
    _ids(ids), _f32(dx, "dx"), _f32(dtok, "dtok")
    B, T = ids.shape
    vocab, D = dtok.shape
    if dx.numel() != B * T * D:
        raise ValueError("text_embed_bwd: shape mismatch")
    _lib.check(lib.dclip_text_embed_bwd(ids.data_ptr(), dx.data_ptr(), dtok.data_ptr(), B, T, D, vocab, _stream()),
               "text_embed_bwd")
    return dtok


def first_eos(ids, eos_id: int) -> torch.Tensor:
    lib = _lib.load()
    _ids(ids)
    B, T = ids.shape
    idx = torch.empty((B,), dtype=torch.int32, device=ids.device)
    _lib.check(lib.dclip_first_eos(ids.data_ptr(), idx.data_ptr(), B, T, int(eos_id), _stream()), "first_eos")
    return idx


def _idx(idx, B):
    if idx is None:
        return None
    if not (idx.is_cuda and idx.dtype == torch.int32 and idx.is_contiguous() and idx.numel() == B):
        raise ValueError("row index: expected contiguous int32 CUDA tensor [B]")
    return idx


def gather_rows(x, idx, B: int, S: int, D: int) -> torch.Tensor:
    lib = _lib.load()
    _f32(x, "x"), _idx(idx, B)
    if x.numel() != B * S * D:
        raise ValueError("gather_rows: shape mismatch")
    out = torch.empty((B, D), dtype=torch.float32, device=x.device)
    _lib.check(lib.dclip_gather_rows(x.data_ptr(), _ptr(idx), out.data_ptr(), B, S, D, _stream()), "gather_rows")
    return out


def scatter_rows(dout, idx, B: int, S: int, D: int) -> torch.Tensor:
    lib = _lib.load()
    _f32(dout, "dout"), _idx(idx, B)
    if dout.numel() != B * D:
        raise ValueError("scatter_rows: shape mismatch")
    dx = torch.empty((B * S, D), dtype=torch.float32, device=dout.device)
    _lib.check(lib.dclip_scatter_rows(dout.data_ptr(), _ptr(idx), dx.data_ptr(), B, S, D, _stream()), "scatter_rows")
    return dx


# ------------------------------------------------------------------------------------------- losses

NORM_EPS = 1e-12


def normalize_rows_fwd(x):
    lib = _lib.load()
    _f32(x, "x")
    B, Pd = x.shape
    xhat = torch.empty_like(x)
    inv = torch.empty((B,), dtype=torch.float32, device=x.device)
    _lib.check(lib.dclip_normalize_rows_fwd(x.data_ptr(), xhat.data_ptr(), inv.data_ptr(), B, Pd, NORM_EPS, _stream()),
               "normalize_rows_fwd")
    return xhat, inv


def normalize_rows_bwd(dxhat, xhat, inv, dx=None, accumulate=False):
    lib = _lib.load()
    _f32(dxhat, "dxhat"), _f32(xhat, "xhat"), _f32(inv, "inv")
    B, Pd = xhat.shape
    if dxhat.shape != xhat.shape or inv.numel() != B:
        raise ValueError("normalize_rows_bwd: shape mismatch")
    if dx is None:
        dx = torch.empty_like(xhat)
        accumulate = False
    _f32(dx, "dx")
    _lib.check(lib.dclip_normalize_rows_bwd(dxhat.data_ptr(), xhat.data_ptr(), inv.data_ptr(), dx.data_ptr(), B, Pd,
                                            NORM_EPS, int(accumulate), _stream()), "normalize_rows_bwd")
    return dx


def contrastive_lse(a_local, b_global, offset: int, inv_temp: float):
    lib = _lib.load()
    _f32(a_local, "a_local"), _f32(b_global, "b_global")
    Bl, Pd = a_local.shape
    Bg, Pb = b_global.shape
    if Pd != Pb or not (0 <= offset and offset + Bl <= Bg):
        raise ValueError(f"contrastive_lse: shapes {tuple(a_local.shape)} {tuple(b_global.shape)} offset {offset}")
    lse = torch.empty((Bl,), dtype=torch.float32, device=a_local.device)
    diag = torch.empty((Bl,), dtype=torch.float32, device=a_local.device)
    nbytes = lib.dclip_contrastive_workspace(Bl, Bg, Pd)
    ws = _ws.get(nbytes, a_local.device)
    _lib.check(lib.dclip_contrastive_lse(a_local.data_ptr(), b_global.data_ptr(), lse.data_ptr(), diag.data_ptr(), Bl,
                                         Bg, Pd, offset, float(inv_temp), _ptr(ws), nbytes, _stream()),
               "contrastive_lse")
    return lse, diag


def contrastive_grad(a_local, b_global, lse_row, lse_col, offset: int, inv_temp: float, coef: float):
    lib = _lib.load()
    _f32(a_local, "a_local"), _f32(b_global, "b_global"), _f32(lse_row, "lse_row"), _f32(lse_col, "lse_col")
    Bl, Pd = a_local.shape
    Bg = b_global.shape[0]
    if lse_row.numel() != Bl or lse_col.numel() != Bg or b_global.shape[1] != Pd:
        raise ValueError("contrastive_grad: shape mismatch")
    da = torch.empty_like(a_local)
    nbytes = lib.dclip_contrastive_workspace(Bl, Bg, Pd)
    ws = _ws.get(nbytes, a_local.device)
    _lib.check(lib.dclip_contrastive_grad(a_local.data_ptr(), b_global.data_ptr(), lse_row.data_ptr(),
                                          lse_col.data_ptr(), da.data_ptr(), Bl, Bg, Pd, offset, float(inv_temp),
                                          float(coef), _ptr(ws), nbytes, _stream()), "contrastive_grad")
    return da


def cosine_loss_fwd(s, t):
    lib = _lib.load()
    _f32(s, "student"), _f32(t, "teacher")
    if s.shape != t.shape:
        raise ValueError(f"cosine_distillation_loss: shapes {tuple(s.shape)} vs {tuple(t.shape)} — the reference "
                         "raises here too (CLIP_image_distillation.py:573)")
    B, Pd = s.shape
    loss_sum = torch.empty((), dtype=torch.float32, device=s.device)
    cos = torch.empty((B,), dtype=torch.float32, device=s.device)
    _lib.check(lib.dclip_cosine_loss_fwd(s.data_ptr(), t.data_ptr(), loss_sum.data_ptr(), cos.data_ptr(), B, Pd,
                                         _stream()), "cosine_loss_fwd")
    return loss_sum, cos


def cosine_loss_bwd(s, t, cos, coef: float, ds=None, accumulate=False):
    lib = _lib.load()
    _f32(s, "student"), _f32(t, "teacher"), _f32(cos, "cos")
    B, Pd = s.shape
    if ds is None:
        ds = torch.empty_like(s)
        accumulate = False
    _lib.check(lib.dclip_cosine_loss_bwd(s.data_ptr(), t.data_ptr(), cos.data_ptr(), ds.data_ptr(), B, Pd, float(coef),
                                         int(accumulate), _stream()), "cosine_loss_bwd")
    return ds


def sub_reduce(a, b, scale: float, out=None, accumulate=False):
    lib = _lib.load()
    _f32(a, "a")
    if b is not None and _f32(b, "b").numel() != a.numel():
        raise ValueError("sub_reduce: size mismatch")
    if out is None:
        out = torch.empty((), dtype=torch.float32, device=a.device)
        accumulate = False
    _lib.check(lib.dclip_sub_reduce(a.data_ptr(), _ptr(b), out.data_ptr(), a.numel(), float(scale), int(accumulate),
                                    _stream()), "sub_reduce")
    return out


# ------------------------------------------------------------------------------------------- meta-teacher tail

def cross_attention_fwd(q, kv, B: int, Lq: int, Lk: int, H: int):
    lib = _lib.load()
    _f32(q, "q"), _f32(kv, "kv")
    E = H * 64
    if q.numel() != B * Lq * E or kv.numel() != B * Lk * 2 * E:
        raise ValueError(f"cross_attention_fwd: q {tuple(q.shape)} kv {tuple(kv.shape)} vs B={B} Lq={Lq} Lk={Lk} H={H}")
    out = torch.empty((B * Lq, E), dtype=torch.float32, device=q.device)
    lse = torch.empty((B, H, Lq), dtype=torch.float32, device=q.device)
    _lib.check(lib.dclip_cross_attention_fwd(q.data_ptr(), kv.data_ptr(), out.data_ptr(), lse.data_ptr(), B, Lq, Lk, H,
                                             _stream()), "cross_attention_fwd")
    return out, lse


def cross_attention_bwd(q, kv, out, dout, lse, B: int, Lq: int, Lk: int, H: int):
    lib = _lib.load()
    for n, t in (("q", q), ("kv", kv), ("out", out), ("dout", dout), ("lse", lse)):
        _f32(t, n)
    E = H * 64
    if q.numel() != B * Lq * E or kv.numel() != B * Lk * 2 * E or out.numel() != q.numel() \
            or dout.numel() != q.numel() or lse.numel() != B * H * Lq:
        raise ValueError("cross_attention_bwd: shape mismatch")
    dq = torch.empty_like(q)
    dkv = torch.empty_like(kv)
    delta = torch.empty((B * H * Lq,), dtype=torch.float32, device=q.device)
    _lib.check(lib.dclip_cross_attention_bwd(q.data_ptr(), kv.data_ptr(), out.data_ptr(), dout.data_ptr(),
                                             lse.data_ptr(), dq.data_ptr(), dkv.data_ptr(), delta.data_ptr(), B, Lq, Lk,
                                             H, _stream()), "cross_attention_bwd")
    return dq, dkv


def aggregation_fwd(x, temperature: float = 2.0, out=None, out_scale: float = 1.0, accumulate: bool = False):
    lib = _lib.load()
    _f32(x, "x")
    B, L, E = x.shape
    if out is None:
        out = torch.empty((B, E), dtype=torch.float32, device=x.device)
        accumulate = False
    _f32(out, "out")
    w = torch.empty((B, L), dtype=torch.float32, device=x.device)
    _lib.check(lib.dclip_aggregation_fwd(x.data_ptr(), out.data_ptr(), w.data_ptr(), B, L, E, float(temperature),
                                         float(out_scale), int(accumulate), _stream()), "aggregation_fwd")
    return out, w


def aggregation_bwd(x, w, dout, temperature: float = 2.0, out_scale: float = 1.0):
    lib = _lib.load()
    _f32(x, "x"), _f32(w, "weights"), _f32(dout, "dout")
    B, L, E = x.shape
    if tuple(w.shape) != (B, L) or tuple(dout.shape) != (B, E):
        raise ValueError("aggregation_bwd: shape mismatch")
    dx = torch.empty_like(x)
    _lib.check(lib.dclip_aggregation_bwd(x.data_ptr(), w.data_ptr(), dout.data_ptr(), dx.data_ptr(), B, L, E,
                                         float(temperature), float(out_scale), _stream()), "aggregation_bwd")
    return dx


def pack_tokens(tokens, sentence, eos, Tmax: int):
    lib = _lib.load()
    _f32(tokens, "tokens"), _f32(sentence, "sentence")
    B, T, Pd = tokens.shape
    _idx(eos, B)
    if tuple(sentence.shape) != (B, Pd) or not (0 < Tmax <= T):
        raise ValueError("pack_tokens: shape mismatch")
    out = torch.empty((B, Tmax, Pd), dtype=torch.float32, device=tokens.device)
    _lib.check(lib.dclip_pack_tokens(tokens.data_ptr(), sentence.data_ptr(), eos.data_ptr(), out.data_ptr(), B, T, Tmax,
                                     Pd, _stream()), "pack_tokens")
    return out


def mask_rows(x, count):
    lib = _lib.load()
    _f32(x, "x")
    B, R, E = x.shape
    _idx(count, B)
    _lib.check(lib.dclip_mask_rows(x.data_ptr(), count.data_ptr(), B, R, E, _stream()), "mask_rows")
    return x


def sanitize_groups(x: torch.Tensor, rows: int, flags: Optional[torch.Tensor] = None):
    """x viewed as [groups, rows, E]: groups holding a NaN / Inf become zeros IN PLACE.  flags=None: detect (returns
    the int32 flags); flags given: zero the flagged groups (backward of the guard)."""
    lib = _lib.load()
    _f32(x, "x")
    E = x.shape[-1]
    total_rows = x.numel() // E
    if total_rows % rows:
        raise ValueError("sanitize_groups: rows must divide the row count")
    groups = total_rows // rows
    mode = 0 if flags is None else 1
    if flags is None:
        flags = torch.empty((groups,), dtype=torch.int32, device=x.device)
    _lib.check(lib.dclip_sanitize_groups(x.data_ptr(), flags.data_ptr(), groups, rows, E, mode, _stream()),
               "sanitize_groups")
    return x, flags


# ------------------------------------------------------------------------------------------- bf16 frozen-tower path

def _bf16(t: torch.Tensor, name: str) -> torch.Tensor:
    if not (t.is_cuda and t.dtype == torch.bfloat16 and t.is_contiguous()):
        raise ValueError(f"{name}: expected a contiguous bfloat16 CUDA tensor")
    return t


def cast_bf16(x: torch.Tensor, pad_to: int = 8, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[rows, cols] fp32 -> bf16 with the row length rounded up to `pad_to` (zero filled).  `out`: refresh an existing
    copy in place (the persistent bf16 weights of a training tower: a captured HIP graph keeps reading the same buffer)."""
    lib = _lib.load()
    _f32(x, "x")
    rows, cols = x.shape
    ld = (cols + pad_to - 1) // pad_to * pad_to
    if out is not None:
        if tuple(_bf16(out, "out").shape) != (rows, ld):
            raise ValueError(f"cast_bf16: out shape {tuple(out.shape)} != {(rows, ld)}")
        y = out
    else:
        y = torch.empty((rows, ld), dtype=torch.bfloat16, device=x.device)
    _lib.check(lib.dclip_cast_f32_bf16(x.data_ptr(), y.data_ptr(), rows, cols, cols, ld, _stream()), "cast_f32_bf16")
    return y


def layernorm_fwd_bf16(x, gamma, beta, eps: float, save_stats: bool = False):
    """nn.LayerNorm with fp32 statistics and a bf16 result; with `save_stats` returns (y, mean, rstd) for the backward."""
    lib = _lib.load()
    _f32(x, "x"), _f32(gamma, "gamma"), _f32(beta, "beta")
    D = x.shape[-1]
    rows = x.numel() // D
    y = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    if not save_stats:
        _lib.check(lib.dclip_layernorm_fwd_bf16(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), rows, D,
                                                float(eps), _stream()), "layernorm_fwd_bf16")
        return y
    mean = torch.empty((rows,), dtype=torch.float32, device=x.device)
    rstd = torch.empty((rows,), dtype=torch.float32, device=x.device)
    _lib.check(lib.dclip_layernorm_fwd_bf16_stats(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(),
                                                  mean.data_ptr(), rstd.data_ptr(), rows, D, float(eps), _stream()),
               "layernorm_fwd_bf16_stats")
    return y, mean, rstd


def transpose_bf16(x: torch.Tensor, want_copy: bool = False, out: Optional[torch.Tensor] = None):
    """x [rows, cols] fp32 or bf16 -> x^T [cols, ld] bf16 with ld = rows rounded up to 8 (zero padded): the
    token-contiguous operand of a weight-gradient GEMM.  `want_copy`: also the untransposed bf16 copy [rows, cols]
    (cols % 8 == 0) from the same pass.  Returns xT or (xT, copy)."""
    lib = _lib.load()
    if not (x.is_cuda and x.is_contiguous() and x.dim() == 2 and x.dtype in (torch.float32, torch.bfloat16)):
        raise ValueError("transpose_bf16: contiguous 2-D float32 / bfloat16 CUDA tensor")
    rows, cols = x.shape
    if cols % 4:
        raise ValueError("transpose_bf16: cols must be a multiple of 4")
    ld = (rows + 7) // 8 * 8
    if out is not None:
        if tuple(_bf16(out, "out").shape) != (cols, ld):
            raise ValueError(f"transpose_bf16: out shape {tuple(out.shape)} != {(cols, ld)}")
        yT = out
    else:
        yT = torch.empty((cols, ld), dtype=torch.bfloat16, device=x.device)
    copy = None
    if want_copy:
        if cols % 8:
            raise ValueError("transpose_bf16: the bf16 copy feeds a GEMM as A: cols must be a multiple of 8")
        copy = torch.empty((rows, cols), dtype=torch.bfloat16, device=x.device)
    _lib.check(lib.dclip_transpose_to_bf16(x.data_ptr(), int(x.dtype == torch.bfloat16), yT.data_ptr(), _ptr(copy), rows,
                                           cols, cols, ld, cols, _stream()), "transpose_to_bf16")
    return (yT, copy) if want_copy else yT


def _out_f32(out: Optional[torch.Tensor], shape, device, name: str) -> torch.Tensor:
    """`out` (a caller-named destination, e.g. a gradient's slice of its all-reduce bucket) checked, or a fresh tensor."""
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    if tuple(out.shape) != tuple(shape) or out.dtype != torch.float32 or not out.is_contiguous() or not out.is_cuda:
        raise ValueError(f"{name}: out must be a contiguous float32 CUDA tensor of shape {tuple(shape)}")
    return out


def mt_weights_table(recs, dtype: torch.dtype = torch.bfloat16):
    """Device table for mt_weights_bf16 (mt_weights_f16 with dtype float16) from [(w fp32 [rows, cols...], w16 [rows, ld] or
    None, w16T [cols, ldT] or None)], w16 / w16T of `dtype`; returns (table tensor, ntensors, total tiles).  One synchronous
    upload: build it once, outside graph capture."""
    chk = _bf16 if dtype == torch.bfloat16 else _f16
    import struct
    lib = _lib.load()
    assert lib.dclip_mt_weights_record_bytes() == 48
    blob, t0 = [], 0
    dev = None
    for w, w16, w16T in recs:
        _f32(w, "w")
        dev = w.device
        rows = w.shape[0]
        cols = w.numel() // rows
        ld = w16.shape[1] if w16 is not None else cols
        ldT = w16T.shape[1] if w16T is not None else rows
        if cols % 4 or ld % 4 or ldT % 8:
            raise ValueError("mt_weights_table: cols / ld must be multiples of 4, ldT of 8")
        if w16 is not None and (tuple(chk(w16, "w16").shape) != (rows, ld)):
            raise ValueError("mt_weights_table: w16 shape")
        if w16T is not None and (tuple(chk(w16T, "w16T").shape) != (cols, ldT)):
            raise ValueError("mt_weights_table: w16T shape")
        tiles_c = (max(cols, ld) + 63) // 64
        tiles_r = (max(rows, ldT) + 63) // 64
        blob.append(struct.pack("<QQQiiiiii", w.data_ptr(), _ptr(w16) or 0, _ptr(w16T) or 0, rows, cols, ld, ldT, t0, tiles_c))
        t0 += tiles_c * tiles_r
    raw = b"".join(blob)
    table = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
    return table, len(recs), t0


def mt_weights_bf16(table: torch.Tensor, ntensors: int, total_tiles: int) -> None:
    lib = _lib.load()
    _lib.check(lib.dclip_mt_weights_bf16(table.data_ptr(), ntensors, total_tiles, _stream()), "mt_weights_bf16")


def rowsum_bf16(x: torch.Tensor, n: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Row sums (fp32) of the first n columns of a bf16 matrix [R, ld]."""
    lib = _lib.load()
    _bf16(x, "x")
    R, ld = x.shape
    n = ld if n is None else n
    out = _out_f32(out, (R,), x.device, "rowsum_bf16")
    _lib.check(lib.dclip_rowsum_bf16(x.data_ptr(), out.data_ptr(), R, n, ld, _stream()), "rowsum_bf16")
    return out


def attention_fwd_bf16(qkv: torch.Tensor, B: int, S: int, H: int, causal: bool) -> torch.Tensor:
    """qkv [B*S, 3*H*64] bf16 -> context [B*S, H*64] bf16 (frozen towers, forward only)."""
    lib = _lib.load()
    _bf16(qkv, "qkv")
    if tuple(qkv.shape) != (B * S, 3 * H * 64):
        raise ValueError(f"attention_fwd_bf16: qkv shape {tuple(qkv.shape)} != {(B * S, 3 * H * 64)}")
    out = torch.empty((B * S, H * 64), dtype=torch.bfloat16, device=qkv.device)
    _lib.check(lib.dclip_attention_fwd_bf16(qkv.data_ptr(), out.data_ptr(), B, S, H, int(causal), _stream()),
               "attention_fwd_bf16")
    return out


def attention_fwd_bf16_lse(qkv: torch.Tensor, B: int, S: int, H: int, causal: bool):
    """bf16 MFMA attention forward that also returns the log-sum-exp (training): qkv [B*S, 3*H*64] bf16 -> (context bf16, lse fp32)."""
    lib = _lib.load()
    _bf16(qkv, "qkv")
    if tuple(qkv.shape) != (B * S, 3 * H * 64):
        raise ValueError(f"attention_fwd_bf16_lse: qkv shape {tuple(qkv.shape)} != {(B * S, 3 * H * 64)}")
    out = torch.empty((B * S, H * 64), dtype=torch.bfloat16, device=qkv.device)
    lse = torch.empty((B * H, S), dtype=torch.float32, device=qkv.device)
    _lib.check(lib.dclip_attention_fwd_bf16_lse(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), B, S, H, int(causal), _stream()),
               "attention_fwd_bf16_lse")
    return out, lse


def attention_bwd_bf16(qkv, out, dout, lse, B: int, S: int, H: int, causal: bool) -> torch.Tensor:
    """Backward of attention_fwd_bf16_lse on the bf16 MFMAs (S <= 64): returns dqkv [B*S, 3*H*64] bf16."""
    lib = _lib.load()
    _bf16(qkv, "qkv"), _bf16(out, "out"), _bf16(dout, "dout"), _f32(lse, "lse")
    D = H * 64
    if tuple(qkv.shape) != (B * S, 3 * D) or tuple(out.shape) != (B * S, D) or tuple(dout.shape) != (B * S, D) \
            or lse.numel() != B * H * S:
        raise ValueError("attention_bwd_bf16: shape mismatch")
    dqkv = torch.empty_like(qkv)
    _lib.check(lib.dclip_attention_bwd_bf16(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), dqkv.data_ptr(),
                                            B, S, H, int(causal), _stream()), "attention_bwd_bf16")
    return dqkv


def attention_row_fwd_bf16(qkv: torch.Tensor, rows: Optional[torch.Tensor], B: int, S: int, H: int) -> torch.Tensor:
    """One attention output row per sequence from a bf16 qkv [B*S, 3*H*64]: row 0 against all keys (rows None: the CLS row of a
    vision tower's last layer) or row rows[b] against keys 0..rows[b] (int32 [B]: the first-EOS row of the causal text tower).
    Returns [B, H*64] bf16."""
    lib = _lib.load()
    _bf16(qkv, "qkv")
    if tuple(qkv.shape) != (B * S, 3 * H * 64):
        raise ValueError(f"attention_row_fwd_bf16: qkv shape {tuple(qkv.shape)} != {(B * S, 3 * H * 64)}")
    if rows is not None and not (rows.is_cuda and rows.dtype == torch.int32 and rows.numel() == B and rows.is_contiguous()):
        raise ValueError("attention_row_fwd_bf16: rows must be a contiguous int32 CUDA tensor [B]")
    out = torch.empty((B, H * 64), dtype=torch.bfloat16, device=qkv.device)
    _lib.check(lib.dclip_attention_row_fwd_bf16(qkv.data_ptr(), None if rows is None else rows.data_ptr(), out.data_ptr(),
                                                B, S, H, _stream()), "attention_row_fwd_bf16")
    return out


def attention_fwd_io16(qkv: torch.Tensor, B: int, S: int, H: int, causal: bool):
    """Short sequences (S <= 80), bf16 in / bf16 out, fp32 arithmetic: qkv [B*S, 3*H*64] bf16 -> (context bf16, lse fp32)."""
    lib = _lib.load()
    _bf16(qkv, "qkv")
    if tuple(qkv.shape) != (B * S, 3 * H * 64):
        raise ValueError(f"attention_fwd_io16: qkv shape {tuple(qkv.shape)} != {(B * S, 3 * H * 64)}")
    out = torch.empty((B * S, H * 64), dtype=torch.bfloat16, device=qkv.device)
    lse = torch.empty((B * H, S), dtype=torch.float32, device=qkv.device)
    _lib.check(lib.dclip_attention_fwd_io16(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), B, S, H, int(causal), _stream()),
               "attention_fwd_io16")
    return out, lse


def attention_bwd_io16(qkv, out, dout, lse, B: int, S: int, H: int, causal: bool) -> torch.Tensor:
    """Backward of attention_fwd_io16 (S <= 64): everything bf16 except lse; returns dqkv [B*S, 3*H*64] bf16."""
    lib = _lib.load()
    _bf16(qkv, "qkv"), _bf16(out, "out"), _bf16(dout, "dout"), _f32(lse, "lse")
    D = H * 64
    if tuple(qkv.shape) != (B * S, 3 * D) or tuple(out.shape) != (B * S, D) or tuple(dout.shape) != (B * S, D) \
            or lse.numel() != B * H * S:
        raise ValueError("attention_bwd_io16: shape mismatch")
    dqkv = torch.empty_like(qkv)
    _lib.check(lib.dclip_attention_bwd_io16(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), dqkv.data_ptr(),
                                            B, S, H, int(causal), _stream()), "attention_bwd_io16")
    return dqkv


def gemm_bf16(a: torch.Tensor, w: torch.Tensor, *, n: Optional[int] = None, k: Optional[int] = None,
              bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None, gelu: bool = False,
              out_bf16: bool = False, save_preact: bool = False, dgelu_of: Optional[torch.Tensor] = None,
              out: Optional[torch.Tensor] = None):
    """y = epilogue(a @ w^T): a [M, lda>=K] and w [N, ldw>=K] bf16 (K-major), fp32 accumulation; y fp32 or bf16.
    Training path: `save_preact` (with gelu) also returns the bf16 pre-activation -> (y, h); `dgelu_of=h` multiplies the
    result by quick_gelu'(h)."""
    lib = _lib.load()
    _bf16(a, "a"), _bf16(w, "w")
    M, lda = a.shape
    N, ldw = w.shape
    K = k if k is not None else min(lda, ldw)
    if n is not None:
        N = n
    epi = 0
    if bias is not None:
        epi |= EPI_BIAS
        if _f32(bias, "bias").numel() != N:
            raise ValueError("gemm_bf16: bias size")
    if gelu:
        epi |= EPI_GELU
    if residual is not None:
        epi |= EPI_RESIDUAL
        if tuple(_f32(residual, "residual").shape) != (M, N):
            raise ValueError("gemm_bf16: residual shape")
    if out is None:
        out = torch.empty((M, N), dtype=torch.bfloat16 if out_bf16 else torch.float32, device=a.device)
    elif tuple(out.shape) != (M, N) or out.dtype != (torch.bfloat16 if out_bf16 else torch.float32) or not out.is_contiguous():
        raise ValueError("gemm_bf16: out shape / dtype")
    aux = None
    if save_preact:
        if not gelu:
            raise ValueError("gemm_bf16: save_preact goes with gelu")
        aux = torch.empty((M, N), dtype=torch.bfloat16, device=a.device)
    if dgelu_of is not None:
        if gelu or tuple(_bf16(dgelu_of, "dgelu_of").shape) != (M, N):
            raise ValueError("gemm_bf16: dgelu_of must be the [M, N] bf16 pre-activation (and excludes gelu)")
        epi |= EPI_DGELU
        aux = dgelu_of
    if aux is None:
        _lib.check(lib.dclip_gemm_bf16(a.data_ptr(), w.data_ptr(), out.data_ptr(), _ptr(bias), _ptr(residual), M, N, K, lda,
                                       ldw, N, epi, int(out_bf16), _stream()), "gemm_bf16")
    else:
        _lib.check(lib.dclip_gemm_bf16_ex(a.data_ptr(), w.data_ptr(), out.data_ptr(), _ptr(bias), _ptr(residual),
                                          aux.data_ptr(), M, N, K, lda, ldw, N, epi, int(out_bf16), _stream()),
                   "gemm_bf16_ex")
    return (out, aux) if save_preact else out


def gemm_bf16_wgrad(a: torch.Tensor, w: torch.Tensor, k: int, splits: Optional[int] = None,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dW [M, N] fp32 = a[:, :k] @ w[:, :k]^T over bf16 token-contiguous operands (a = dY^T [M, ld], w = X^T [N, ld]):
    split-K when the output has few tiles (deterministic: partials summed in fixed order)."""
    lib = _lib.load()
    _bf16(a, "a"), _bf16(w, "w")
    M, lda = a.shape
    N, ldw = w.shape
    if splits is None:
        splits = lib.dclip_gemm_bf16_splitk_plan(M, N, k)
    out = _out_f32(out, (M, N), a.device, "gemm_bf16_wgrad")
    nbytes = lib.dclip_gemm_bf16_splitk_workspace(M, N, splits)
    ws = _ws.get(nbytes, a.device)
    _lib.check(lib.dclip_gemm_bf16_splitk(a.data_ptr(), w.data_ptr(), out.data_ptr(), M, N, k, lda, ldw, N, splits,
                                          _ptr(ws), nbytes, _stream()), "gemm_bf16_splitk")
    return out


def gemm_bf16_wgrad_tokmajor(dy: torch.Tensor, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """dW [out, in] fp32 = dy^T x from the token-major bf16 operands dy [tokens, out], x [tokens, in] as the backward has
    them (no transposes).  Returns None when the library's token-major form does not apply to the shape (the caller then
    transposes and uses gemm_bf16_wgrad)."""
    lib = _lib.load()
    _bf16(dy, "dy"), _bf16(x, "x")
    K, M = dy.shape
    K2, N = x.shape
    if K != K2:
        raise ValueError("gemm_bf16_wgrad_tokmajor: token counts differ")
    splits = lib.dclip_gemm_bf16_wgrad_tokmajor_plan(M, N, K)
    if splits == 0:
        return None
    out = _out_f32(out, (M, N), dy.device, "gemm_bf16_wgrad_tokmajor")
    nbytes = lib.dclip_gemm_bf16_splitk_workspace(M, N, splits)
    ws = _ws.get(nbytes, dy.device)
    _lib.check(lib.dclip_gemm_bf16_wgrad_tokmajor(dy.data_ptr(), x.data_ptr(), out.data_ptr(), M, N, K, M, N, N, splits,
                                                  _ptr(ws), nbytes, _stream()), "gemm_bf16_wgrad_tokmajor")
    return out


def colsum_bf16(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Column sums (over the rows = tokens) of a bf16 matrix, fp32 result: a bias gradient from a bf16 dY."""
    lib = _lib.load()
    _bf16(x, "x")
    M, N = x.shape
    out = _out_f32(out, (N,), x.device, "colsum_bf16")
    nbytes = lib.dclip_colsum_f32_workspace(M, N)
    ws = _ws.get(nbytes, x.device)
    _lib.check(lib.dclip_colsum_bf16(x.data_ptr(), out.data_ptr(), M, N, N, 0, _ptr(ws), nbytes, _stream()), "colsum_bf16")
    return out


# ------------------------------------------------------------------------------------------- fp16 frozen-tower path
# The bf16 forward wrappers above with fp16 tensors (include/dclip_hip.h, "fp16 forward path"): same shapes and limits,
# rounding to nearest even with finite values beyond +-65504 saturated.  Forward only: no save_preact / dgelu_of / stats.

def _f16(t: torch.Tensor, name: str) -> torch.Tensor:
    if not (t.is_cuda and t.dtype == torch.float16 and t.is_contiguous()):
        raise ValueError(f"{name}: expected a contiguous float16 CUDA tensor")
    return t


def cast_f16(x: torch.Tensor, pad_to: int = 8, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[rows, cols] fp32 -> fp16, row length rounded up to `pad_to` (zero filled); `out`: refresh an existing copy in place."""
    lib = _lib.load()
    _f32(x, "x")
    if x.dim() != 2:
        raise ValueError("cast_f16: x must be 2-D")
    rows, cols = x.shape
    ld = (cols + pad_to - 1) // pad_to * pad_to
    if out is not None:
        if tuple(_f16(out, "out").shape) != (rows, ld):
            raise ValueError(f"cast_f16: out shape {tuple(out.shape)} != {(rows, ld)}")
        y = out
    else:
        y = torch.empty((rows, ld), dtype=torch.float16, device=x.device)
    _lib.check(lib.dclip_cast_f32_f16(x.data_ptr(), y.data_ptr(), rows, cols, cols, ld, _stream()), "cast_f32_f16")
    return y


def layernorm_fwd_f16(x, gamma, beta, eps: float) -> torch.Tensor:
    """nn.LayerNorm with fp32 statistics and an fp16 result."""
    lib = _lib.load()
    _f32(x, "x"), _f32(gamma, "gamma"), _f32(beta, "beta")
    D = x.shape[-1]
    rows = x.numel() // D
    y = torch.empty(x.shape, dtype=torch.float16, device=x.device)
    _lib.check(lib.dclip_layernorm_fwd_f16(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), rows, D, float(eps),
                                           _stream()), "layernorm_fwd_f16")
    return y


def im2col_f16(pixels: torch.Tensor, patch: int) -> torch.Tensor:
    """im2col with an fp16 result (rows padded to a multiple of 8 columns, zero filled); patch % 4 == 0."""
    lib = _lib.load()
    _f32(pixels, "pixel_values")
    B, Cc, Hh, Ww = pixels.shape
    if Hh != Ww or Hh % patch or patch % 4:
        raise ValueError(f"im2col_f16: image {Hh}x{Ww}, patch {patch}")
    g, kdim = Hh // patch, Cc * patch * patch
    ld = (kdim + 7) // 8 * 8
    alloc = torch.zeros if ld != kdim else torch.empty
    cols = alloc((B * g * g, ld), dtype=torch.float16, device=pixels.device)
    _lib.check(lib.dclip_im2col_f16(pixels.data_ptr(), cols.data_ptr(), B, Cc, Hh, Ww, patch, ld, _stream()), "im2col_f16")
    return cols


def attention_fwd_f16(qkv: torch.Tensor, B: int, S: int, H: int, causal: bool) -> torch.Tensor:
    """qkv [B*S, 3*H*64] fp16 -> context [B*S, H*64] fp16 (frozen towers, forward only)."""
    lib = _lib.load()
    _f16(qkv, "qkv")
    if tuple(qkv.shape) != (B * S, 3 * H * 64):
        raise ValueError(f"attention_fwd_f16: qkv shape {tuple(qkv.shape)} != {(B * S, 3 * H * 64)}")
    out = torch.empty((B * S, H * 64), dtype=torch.float16, device=qkv.device)
    _lib.check(lib.dclip_attention_fwd_f16(qkv.data_ptr(), out.data_ptr(), B, S, H, int(causal), _stream()), "attention_fwd_f16")
    return out


def attention_row_fwd_f16(qkv: torch.Tensor, rows: Optional[torch.Tensor], B: int, S: int, H: int) -> torch.Tensor:
    """attention_row_fwd_bf16 on an fp16 qkv: [B, H*64] fp16."""
    lib = _lib.load()
    _f16(qkv, "qkv")
    if tuple(qkv.shape) != (B * S, 3 * H * 64):
        raise ValueError(f"attention_row_fwd_f16: qkv shape {tuple(qkv.shape)} != {(B * S, 3 * H * 64)}")
    if rows is not None and not (rows.is_cuda and rows.dtype == torch.int32 and rows.numel() == B and rows.is_contiguous()):
        raise ValueError("attention_row_fwd_f16: rows must be a contiguous int32 CUDA tensor [B]")
    out = torch.empty((B, H * 64), dtype=torch.float16, device=qkv.device)
    _lib.check(lib.dclip_attention_row_fwd_f16(qkv.data_ptr(), None if rows is None else rows.data_ptr(), out.data_ptr(),
                                               B, S, H, _stream()), "attention_row_fwd_f16")
    return out


def gemm_f16(a: torch.Tensor, w: torch.Tensor, *, n: Optional[int] = None, k: Optional[int] = None,
             bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None, gelu: bool = False,
             out_f16: bool = False, out: Optional[torch.Tensor] = None, alpha: Optional[float] = None,
             split_out_scale: Optional[float] = None) -> torch.Tensor:
    """y = epilogue(a @ w^T): a [M, lda>=K] and w [N, ldw>=K] fp16 (K-major), fp32 accumulation; y fp32 or fp16.  `alpha`
    (dclip_gemm_f16_scaled): the accumulator is multiplied by it before bias, GELU and residual.  `split_out_scale`
    (dclip_gemm_f16_scaled_split; bias / gelu only): y is fp16 [M, 3N], the [hi|lo|hi] split of split_out_scale * result."""
    lib = _lib.load()
    _f16(a, "a"), _f16(w, "w")
    M, lda = a.shape
    N, ldw = w.shape
    K = k if k is not None else min(lda, ldw)
    if n is not None:
        N = n
    epi = 0
    if bias is not None:
        epi |= EPI_BIAS
        if _f32(bias, "bias").numel() != N:
            raise ValueError("gemm_f16: bias size")
    if gelu:
        epi |= EPI_GELU
    if residual is not None:
        epi |= EPI_RESIDUAL
        if tuple(_f32(residual, "residual").shape) != (M, N):
            raise ValueError("gemm_f16: residual shape")
    if split_out_scale is not None:
        if residual is not None or out_f16 or out is not None:
            raise ValueError("gemm_f16: a split output takes bias / gelu only")
        y3 = torch.empty((M, 3 * N), dtype=torch.float16, device=a.device)
        _lib.check(lib.dclip_gemm_f16_scaled_split(a.data_ptr(), w.data_ptr(), y3.data_ptr(), _ptr(bias), M, N, K, lda, ldw, 3 * N,
                                                   epi, 1.0 if alpha is None else float(alpha), float(split_out_scale), _stream()),
                   "gemm_f16_scaled_split")
        return y3
    odt = torch.float16 if out_f16 else torch.float32
    if out is None:
        out = torch.empty((M, N), dtype=odt, device=a.device)
    elif tuple(out.shape) != (M, N) or out.dtype != odt or not out.is_contiguous():
        raise ValueError("gemm_f16: out shape / dtype")
    if alpha is not None:
        _lib.check(lib.dclip_gemm_f16_scaled(a.data_ptr(), w.data_ptr(), out.data_ptr(), _ptr(bias), _ptr(residual), M, N, K, lda,
                                             ldw, N, epi, int(out_f16), float(alpha), _stream()), "gemm_f16_scaled")
        return out
    _lib.check(lib.dclip_gemm_f16(a.data_ptr(), w.data_ptr(), out.data_ptr(), _ptr(bias), _ptr(residual), M, N, K, lda, ldw, N,
                                  epi, int(out_f16), _stream()), "gemm_f16")
    return out


# ------------------------------------------------------------------------------------------- split-fp16 (frozen fp32 text tower)
# fp32 x = hi + lo in two fp16 pieces (include/dclip_hip.h, "Split-fp16"): the operands of gemm_f16(alpha=...).

def split_f16x3(x: torch.Tensor, scale: float = 1.0, order: int = 0, out: Optional[torch.Tensor] = None,
                pieces: int = 3) -> torch.Tensor:
    """[rows, cols] fp32 -> fp16 [rows, 3 cols] of x * scale (a power of two): order 0 [hi|lo|hi] (activations), 1 [hi|hi|lo]
    (weights); cols % 8 == 0.  `out`: refresh an existing split in place.  `pieces` = 2 (order 0): fp16 [rows, 2 cols] = [hi|lo],
    the operand of the fused GEMMs without its unread third."""
    lib = _lib.load()
    _f32(x, "x")
    if x.dim() != 2:
        raise ValueError("split_f16x3: x must be 2-D")
    rows, cols = x.shape
    if pieces == 2:
        if order != 0 or out is not None:
            raise ValueError("split_f16x3: two pieces are the order-0 split into a fresh tensor")
        y = torch.empty((rows, 2 * cols), dtype=torch.float16, device=x.device)
        _lib.check(lib.dclip_split_f32_f16x2(x.data_ptr(), y.data_ptr(), rows, cols, cols, 2 * cols, float(scale), None, _stream()),
                   "split_f32_f16x2")
        return y
    if out is not None:
        if tuple(_f16(out, "out").shape) != (rows, 3 * cols):
            raise ValueError(f"split_f16x3: out shape {tuple(out.shape)} != {(rows, 3 * cols)}")
        y = out
    else:
        y = torch.empty((rows, 3 * cols), dtype=torch.float16, device=x.device)
    _lib.check(lib.dclip_split_f32_f16x3(x.data_ptr(), y.data_ptr(), rows, cols, cols, 3 * cols, float(scale), int(order),
                                         _stream()), "split_f32_f16x3")
    return y


def layernorm_fwd_f16x3(x, gamma, beta, eps: float, scale: float = 1.0, pieces: int = 3) -> torch.Tensor:
    """nn.LayerNorm (fp32 statistics and arithmetic) written as the [hi|lo|hi] split of scale * LN(x): [rows, 3 D] fp16; `pieces`
    = 2: [hi|lo], [rows, 2 D]."""
    lib = _lib.load()
    _f32(x, "x"), _f32(gamma, "gamma"), _f32(beta, "beta")
    D = x.shape[-1]
    rows = x.numel() // D
    if pieces == 2:
        y = torch.empty((rows, 2 * D), dtype=torch.float16, device=x.device)
        _lib.check(lib.dclip_layernorm_fwd_f16x2(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), None, None, None, rows,
                                                 D, float(eps), float(scale), None, _stream()), "layernorm_fwd_f16x2")
        return y
    y = torch.empty((rows, 3 * D), dtype=torch.float16, device=x.device)
    _lib.check(lib.dclip_layernorm_fwd_f16x3(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), rows, D, float(eps),
                                             float(scale), _stream()), "layernorm_fwd_f16x3")
    return y


# ------------------------------------------------------------------------------------------- split-fp16, scales on the device
# The wrappers above for a tower whose weights change every step (the student's vision forward): every scale
# is the ADDRESS of a float of the device plan record (split16_refresh computes it on the device), passed as an int.

def split_f16x3_dev(x: torch.Tensor, scale_ptr: int, order: int = 0, out: Optional[torch.Tensor] = None,
                    pieces: int = 3) -> torch.Tensor:
    """split_f16x3 with the scale read from device memory."""
    lib = _lib.load()
    _f32(x, "x")
    if x.dim() != 2:
        raise ValueError("split_f16x3_dev: x must be 2-D")
    rows, cols = x.shape
    if pieces == 2:
        if order != 0 or out is not None:
            raise ValueError("split_f16x3_dev: two pieces are the order-0 split into a fresh tensor")
        y = torch.empty((rows, 2 * cols), dtype=torch.float16, device=x.device)
        _lib.check(lib.dclip_split_f32_f16x2(x.data_ptr(), y.data_ptr(), rows, cols, cols, 2 * cols, 1.0, scale_ptr, _stream()),
                   "split_f32_f16x2")
        return y
    if out is not None:
        if tuple(_f16(out, "out").shape) != (rows, 3 * cols):
            raise ValueError(f"split_f16x3_dev: out shape {tuple(out.shape)} != {(rows, 3 * cols)}")
        y = out
    else:
        y = torch.empty((rows, 3 * cols), dtype=torch.float16, device=x.device)
    _lib.check(lib.dclip_split_f32_f16x3_dev(x.data_ptr(), y.data_ptr(), rows, cols, cols, 3 * cols, scale_ptr, int(order),
                                             _stream()), "split_f32_f16x3_dev")
    return y


def layernorm_fwd_f16x3_dev(x, gamma, beta, eps: float, scale_ptr: int, save: bool = False, pieces: int = 3, save32: bool = True):
    """layernorm_fwd_f16x3 with the scale read from device memory -> (y3, y, mean, rstd); with `save`, y / mean / rstd are what
    layernorm_fwd returns (bit for bit), otherwise None.  `pieces` = 2: y3 is [hi|lo], [rows, 2 D].  `save32` False: the fp32 y is
    not stored (None) even with `save`."""
    lib = _lib.load()
    _f32(x, "x"), _f32(gamma, "gamma"), _f32(beta, "beta")
    D = x.shape[-1]
    rows = x.numel() // D
    if gamma.numel() != D or beta.numel() != D:
        raise ValueError("layernorm_fwd_f16x3_dev: gamma/beta size")
    y3 = torch.empty((rows, pieces * D), dtype=torch.float16, device=x.device)
    y = torch.empty_like(x) if save and save32 else None
    mean = torch.empty((rows,), dtype=torch.float32, device=x.device) if save else None
    rstd = torch.empty((rows,), dtype=torch.float32, device=x.device) if save else None
    if pieces == 2:
        _lib.check(lib.dclip_layernorm_fwd_f16x2(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y3.data_ptr(), _ptr(y), _ptr(mean),
                                                 _ptr(rstd), rows, D, float(eps), 1.0, scale_ptr, _stream()), "layernorm_fwd_f16x2")
        return y3, y, mean, rstd
    _lib.check(lib.dclip_layernorm_fwd_f16x3_dev(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y3.data_ptr(), _ptr(y), _ptr(mean),
                                                 _ptr(rstd), rows, D, float(eps), scale_ptr, _stream()), "layernorm_fwd_f16x3_dev")
    return y3, y, mean, rstd


def quick_gelu(h: torch.Tensor) -> torch.Tensor:
    """quick_gelu(h) of a contiguous fp32 tensor (numel % 4 == 0), bit-equal to the g32 the split-output GEMMs' GELU epilogue stores
    beside that h32 (the fp32 g a backward makes again)."""
    lib = _lib.load()
    g = torch.empty_like(_f32(h, "h"))
    _lib.check(lib.dclip_quick_gelu_f32(h.data_ptr(), g.data_ptr(), h.numel(), _stream()), "quick_gelu_f32")
    return g


_GELU_ERF = {torch.float32: "dclip_gelu_erf_f32", torch.bfloat16: "dclip_gelu_erf_bf16", torch.float16: "dclip_gelu_erf_f16"}


def _same(t: torch.Tensor, like: torch.Tensor, name: str) -> torch.Tensor:
    if not (t.is_cuda and t.device == like.device and t.dtype == like.dtype and t.is_contiguous() and t.shape == like.shape):
        raise ValueError(f"{name}: expected a contiguous {like.dtype} tensor of shape {tuple(like.shape)} on {like.device}, got "
                         f"{t.dtype} {tuple(t.shape)} {t.device} contiguous={t.is_contiguous()}")
    return t


def gelu_erf(h: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Exact GELU h Phi(h) of a contiguous fp32, bf16 or fp16 tensor of any size (hidden_act="gelu"): fp32
    arithmetic; a 16-bit result is the activation of the stored 16-bit value, rounded to nearest even.  `out`: where it goes — a
    tensor like h, which may be h itself (in place); None: a new one."""
    lib = _lib.load()
    name = _GELU_ERF.get(h.dtype)
    if name is None or not (h.is_cuda and h.is_contiguous()) or h.numel() == 0:
        raise ValueError(f"gelu_erf: expected a non-empty contiguous fp32 / bf16 / fp16 CUDA tensor, got {h.dtype} {h.device} "
                         f"{tuple(h.shape)} contiguous={h.is_contiguous()}")
    g = torch.empty_like(h) if out is None else _same(out, h, "gelu_erf: out")
    _lib.check(getattr(lib, name)(h.data_ptr(), g.data_ptr(), h.numel(), _stream()), name[6:])
    return g


def gelu_erf_bwd(h: torch.Tensor, dg: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dh = dg gelu'(h), gelu'(h) = Phi(h) + h phi(h), of contiguous fp32 tensors of one shape (the backward of gelu_erf).
    `out`: a tensor like dg, which may be dg itself (in place); None: a new one."""
    lib = _lib.load()
    if _f32(h, "h").numel() == 0:
        raise ValueError("gelu_erf_bwd: empty tensor")
    _same(dg, h, "gelu_erf_bwd: dg")
    dh = torch.empty_like(dg) if out is None else _same(out, h, "gelu_erf_bwd: out")
    _lib.check(lib.dclip_gelu_erf_bwd_f32(h.data_ptr(), dg.data_ptr(), dh.data_ptr(), h.numel(), _stream()), "gelu_erf_bwd_f32")
    return dh


def gemm_f16_dev(a: torch.Tensor, w: torch.Tensor, alpha_ptr: int, *, bias: Optional[torch.Tensor] = None,
                 residual: Optional[torch.Tensor] = None, gelu: bool = False, out_f16: bool = False,
                 split_out_scale_ptr: Optional[int] = None, h32: Optional[torch.Tensor] = None,
                 g32: Optional[torch.Tensor] = None) -> torch.Tensor:
    """gemm_f16(alpha=..., split_out_scale=...) with both scales read from device memory.  With a split output, `h32` / `g32`
    [M, N] fp32 also receive the pre-activation (gelu only) and the result."""
    lib = _lib.load()
    _f16(a, "a"), _f16(w, "w")
    M, lda = a.shape
    N, ldw = w.shape
    K = min(lda, ldw)
    epi = 0
    if bias is not None:
        epi |= EPI_BIAS
        if _f32(bias, "bias").numel() != N:
            raise ValueError("gemm_f16_dev: bias size")
    if gelu:
        epi |= EPI_GELU
    if residual is not None:
        epi |= EPI_RESIDUAL
        if tuple(_f32(residual, "residual").shape) != (M, N):
            raise ValueError("gemm_f16_dev: residual shape")
    if split_out_scale_ptr is not None:
        if residual is not None or out_f16:
            raise ValueError("gemm_f16_dev: a split output takes bias / gelu only")
        for t, nm in ((h32, "h32"), (g32, "g32")):
            if t is not None and tuple(_f32(t, nm).shape) != (M, N):
                raise ValueError(f"gemm_f16_dev: {nm} shape")
        if h32 is not None and not gelu:
            raise ValueError("gemm_f16_dev: h32 is the pre-activation of a gelu epilogue")
        y3 = torch.empty((M, 3 * N), dtype=torch.float16, device=a.device)
        _lib.check(lib.dclip_gemm_f16_scaled_split_dev(a.data_ptr(), w.data_ptr(), y3.data_ptr(), _ptr(bias), _ptr(h32), _ptr(g32), M, N,
                                                       K, lda, ldw, 3 * N, epi, alpha_ptr, split_out_scale_ptr, _stream()),
                   "gemm_f16_scaled_split_dev")
        return y3
    if g32 is not None:
        raise ValueError("gemm_f16_dev: g32 goes with a split output")
    out = torch.empty((M, N), dtype=torch.float16 if out_f16 else torch.float32, device=a.device)
    if h32 is not None:      # fp32 result and fp32 pre-activation, no split
        if not gelu or residual is not None or out_f16 or tuple(_f32(h32, "h32").shape) != (M, N) or N % 8:
            raise ValueError("gemm_f16_dev: h32 [M, N] is the pre-activation of a bias / gelu epilogue with an fp32 result")
        _lib.check(lib.dclip_gemm_f16_scaled_split_dev(a.data_ptr(), w.data_ptr(), out.data_ptr(), _ptr(bias), h32.data_ptr(), None, M,
                                                       N, K, lda, ldw, N, epi, alpha_ptr, None, _stream()),
                   "gemm_f16_scaled_split_dev")
        return out
    _lib.check(lib.dclip_gemm_f16_scaled_dev(a.data_ptr(), w.data_ptr(), out.data_ptr(), _ptr(bias), _ptr(residual), M, N, K, lda, ldw,
                                             N, epi, int(out_f16), alpha_ptr, _stream()), "gemm_f16_scaled_dev")
    return out


SPLIT16_STATS = ("ln1_w", "ln1_b", "v_l1", "v_b", "ln2_w", "ln2_b", "fc1_l1", "fc1_b", "qkv", "out", "fc1", "fc2")
SPLIT16_PLAN_ACT = {"ln1": 0, "ctx": 1, "ln2": 2, "g": 3}          # floats of a plan record: activation scales,
SPLIT16_PLAN_W = {"qkv": 4, "out": 5, "fc1": 6, "fc2": 7}          # weight scales,
SPLIT16_PLAN_ALPHA = {"qkv": 8, "out": 9, "fc1": 10, "fc2": 11}    # alphas; 12 = flags, 16..27 = the statistics
SPLIT16_PLAN_FLAGS, SPLIT16_PLAN_STATS = 12, 16
SPLIT16_PLAN_WALPHA = {"qkv": 28, "out": 29, "fc1": 30, "fc2": 31}  # 2^-f: the alphas of the data-gradient GEMMs (§9e)


def split16_table(layers, transposed: bool = False):
    """The device state of split16_refresh for encoder layers given as dicts of fp32 tensors ln1_w, ln1_b, qkv_w [3D, D],
    qkv_b, out_w, ln2_w, ln2_b, fc1_w, fc1_b, fc2_w (widths multiples of 8): the record table, the statistics accumulators,
    the plan [L, 32] fp32, and per layer the [hi|hi|lo] fp16 copies {"qkv", "out", "fc1", "fc2"}.  `transposed`: also "wt",
    per layer the [hi|hi|lo] copies of the TRANSPOSED scaled weights, [in, 3 out] — the operands of the backward's
    data-gradient GEMMs (as much memory again as "w").  One synchronous upload: build it once, outside graph capture."""
    import struct
    lib = _lib.load()
    assert lib.dclip_split16_record_bytes() == 48
    nplan, trows = lib.dclip_split16_plan_floats(), lib.dclip_split16_tile_rows()
    slot = {n: i for i, n in enumerate(SPLIT16_STATS)}
    tcopies = []
    mats, vecs, copies = [], [], []            # the matrices come first in the table: the weight-split launch covers only them
    dev = layers[0]["qkv_w"].device

    def rec(li, src, rows, cols, max_slot, l1_slot=-1, l1_row0=0, dst=None, scale_slot=-1):
        if cols % 8 or src.data_ptr() % 16:
            raise ValueError("split16_table: widths must be multiples of 8 and tensors 16-byte aligned")
        (vecs if dst is None else mats).append((src.data_ptr(), _ptr(dst) or 0, rows, cols, li, max_slot, l1_slot, l1_row0, scale_slot))

    for li, L in enumerate(layers):
        for n in ("ln1_w", "ln1_b", "qkv_w", "qkv_b", "out_w", "ln2_w", "ln2_b", "fc1_w", "fc1_b", "fc2_w"):
            _f32(L[n], n)
        D = L["ln1_w"].numel()
        if tuple(L["qkv_w"].shape) != (3 * D, D) or L["qkv_b"].numel() != 3 * D:
            raise ValueError("split16_table: qkv_w must be [3D, D]")
        w = {}
        for short in ("qkv", "out", "fc1", "fc2"):
            src = L[short + "_w"]
            w[short] = torch.empty((src.shape[0], 3 * src.shape[1]), dtype=torch.float16, device=dev)
        copies.append(w)
        if transposed:
            wt = {}
            for short in ("qkv", "out", "fc1", "fc2"):
                src = L[short + "_w"]
                if src.shape[0] % 8:
                    raise ValueError("split16_table: a transposed copy needs a multiple of 8 rows")
                wt[short] = torch.empty((src.shape[1], 3 * src.shape[0]), dtype=torch.float16, device=dev)
            tcopies.append(wt)
        vb = L["qkv_b"][2 * D:]                # an address inside qkv_b: the caller re-builds the table when a tensor moves
        for n in ("ln1_w", "ln1_b", "ln2_w", "ln2_b", "fc1_b"):
            rec(li, L[n], 1, L[n].numel(), slot[n])
        rec(li, vb, 1, D, slot["v_b"])
        rec(li, L["qkv_w"], 3 * D, D, slot["qkv"], slot["v_l1"], 2 * D, w["qkv"], SPLIT16_PLAN_W["qkv"])
        rec(li, L["out_w"], L["out_w"].shape[0], L["out_w"].shape[1], slot["out"], dst=w["out"], scale_slot=SPLIT16_PLAN_W["out"])
        rec(li, L["fc1_w"], L["fc1_w"].shape[0], L["fc1_w"].shape[1], slot["fc1"], slot["fc1_l1"], 0, w["fc1"], SPLIT16_PLAN_W["fc1"])
        rec(li, L["fc2_w"], L["fc2_w"].shape[0], L["fc2_w"].shape[1], slot["fc2"], dst=w["fc2"], scale_slot=SPLIT16_PLAN_W["fc2"])
    blob, t0, wtiles = [], 0, 0
    for r in mats + vecs:
        blob.append(struct.pack("<QQiiiiiiii", *r, t0))
        t0 += (r[2] + trows - 1) // trows
        if r[1]:
            wtiles = t0
    table = torch.frombuffer(bytearray(b"".join(blob)), dtype=torch.uint8).to(dev)
    extra = {}
    if transposed:         # one pointer per matrix record, in table order (a layer's qkv, out, fc1, fc2)
        by_dst = {w[k].data_ptr(): wt[k].data_ptr() for w, wt in zip(copies, tcopies) for k in w}
        extra = {"wt": tcopies, "dst_t": torch.tensor([by_dst[r[1]] for r in mats], dtype=torch.int64).to(dev)}
    return {**extra, "table": table, "nrefs": len(blob), "tiles": t0, "wrefs": len(mats), "wtiles": wtiles, "w": copies, "L": len(layers),
            "D": layers[0]["ln1_w"].numel(),
            "stats": torch.zeros((len(layers), len(SPLIT16_STATS)), dtype=torch.int32, device=dev),
            "plan": torch.zeros((len(layers), nplan), dtype=torch.float32, device=dev)}


def split16_refresh(tab) -> None:
    """Statistics, plan and weight split of a split16_table from the CURRENT weights: three launches, nothing read back."""
    lib = _lib.load()
    st = _stream()
    _lib.check(lib.dclip_split16_stats(tab["table"].data_ptr(), tab["nrefs"], tab["tiles"], tab["stats"].data_ptr(), st),
               "split16_stats")
    _lib.check(lib.dclip_split16_plan(tab["stats"].data_ptr(), tab["plan"].data_ptr(), tab["L"], tab["D"], st), "split16_plan")
    if "dst_t" in tab:
        _lib.check(lib.dclip_split16_weights_t(tab["table"].data_ptr(), tab["wrefs"], tab["wtiles"], tab["plan"].data_ptr(),
                                               tab["dst_t"].data_ptr(), st), "split16_weights_t")
    else:
        _lib.check(lib.dclip_split16_weights(tab["table"].data_ptr(), tab["wrefs"], tab["wtiles"], tab["plan"].data_ptr(), st),
                   "split16_weights")


def split_f16x3_rows(x: torch.Tensor, pieces: int = 3):
    """[rows, cols] fp32 (row stride >= cols) -> (fp16 [rows, 3 cols], fp32 [rows]): the [hi|lo|hi] split of x[m] * 2^e_m with
    one power of two PER ROW taken from the row's own maximum (engine.split16_row_exp), and row_alpha[m] = 2^-e_m.  `pieces` = 2:
    [hi|lo], fp16 [rows, 2 cols]."""
    lib = _lib.load()
    if x.dtype != torch.float32 or not x.is_cuda or x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("split_f16x3_rows: x must be a 2-D fp32 device tensor with unit column stride")
    rows, cols = x.shape
    y = torch.empty((rows, pieces * cols), dtype=torch.float16, device=x.device)
    ra = torch.empty((rows,), dtype=torch.float32, device=x.device)
    _lib.check((lib.dclip_split_f32_f16x2_rows if pieces == 2 else lib.dclip_split_f32_f16x3_rows)(x.data_ptr(), y.data_ptr(), ra.data_ptr(), rows, cols, x.stride(0) if rows > 1 else cols,
                                              _stream()), "split_f32_f16x3_rows")
    return y, ra


def gemm_f16_rows_stats_plan(M: int, N: int, K: int) -> int:
    """Partial rows gemm_f16_rows_dev leaves with `stats` (ceil(M / 256)), 0 where the dispatcher takes a register-staged kernel,
    which has no such form."""
    return int(_lib.load().dclip_gemm_f16_scaled_rows_stats_plan(M, N, K))


def gemm_f16_rows_dev(a: torch.Tensor, w: torch.Tensor, alpha_ptr: int, row_alpha: torch.Tensor,
                      dgelu_h: Optional[torch.Tensor] = None, stats: Optional[ColStats] = None) -> torch.Tensor:
    """fp32 [M, N] = ((a w^T) * *alpha_ptr) * row_alpha[m], times quick_gelu'(dgelu_h) when given (fp32 [M, N]): gemm_f16_dev for
    an `a` split by split_f16x3_rows.  `stats` (a ColStats of gemm_f16_rows_stats_plan(M, N, K) partial rows, > 0): the kernel
    also leaves the column partials of the result there; the result is bit-equal to the call without."""
    lib = _lib.load()
    _f16(a, "a"), _f16(w, "w")
    M, lda = a.shape
    N, ldw = w.shape
    K = min(lda, ldw)
    if _f32(row_alpha, "row_alpha").numel() != M:
        raise ValueError("gemm_f16_rows_dev: row_alpha size")
    if dgelu_h is not None and tuple(_f32(dgelu_h, "dgelu_h").shape) != (M, N):
        raise ValueError("gemm_f16_rows_dev: dgelu_h shape")
    out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    if stats is not None:
        if (stats.P, stats.cols) != (gemm_f16_rows_stats_plan(M, N, K), N) or stats.P == 0:
            raise ValueError("gemm_f16_rows_dev: stats must have gemm_f16_rows_stats_plan's row count and N columns")
        _lib.check(lib.dclip_gemm_f16_scaled_rows_stats_dev(a.data_ptr(), w.data_ptr(), out.data_ptr(), _ptr(dgelu_h), M, N, K, lda, ldw,
                                                            N, EPI_DGELU if dgelu_h is not None else 0, alpha_ptr,
                                                            row_alpha.data_ptr(), stats.pmax.data_ptr(), stats.psum.data_ptr(),
                                                            _stream()), "gemm_f16_scaled_rows_stats_dev")
        return out
    _lib.check(lib.dclip_gemm_f16_scaled_rows_dev(a.data_ptr(), w.data_ptr(), out.data_ptr(), _ptr(dgelu_h), M, N, K, lda, ldw, N,
                                                  EPI_DGELU if dgelu_h is not None else 0, alpha_ptr, row_alpha.data_ptr(),
                                                  _stream()), "gemm_f16_scaled_rows_dev")
    return out


def split_f16x3_rows_colstats(x: torch.Tensor, db: Optional[torch.Tensor] = None, pieces: int = 3):
    """split_f16x3_rows that in the same pass takes the column statistics ->
    (y3, row_alpha, yc, col_exp, col_alpha): y3 / row_alpha as split_f16x3_rows gives them (bit for bit); col_exp int32 [cols] =
    engine.split16_col_exp of max|x[:, n]|, col_alpha = 2^-col_exp; yc fp16 [rows, 2 cols] = [hi|lo] of x[m, n] 2^col_exp[n];
    `db` (fp32 [cols]) receives the column sums.  `pieces` = 2: y3 is [hi|lo], fp16 [rows, 2 cols]."""
    lib = _lib.load()
    if x.dtype != torch.float32 or not x.is_cuda or x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("split_f16x3_rows_colstats: x must be a 2-D fp32 device tensor with unit column stride")
    rows, cols = x.shape
    if db is not None and (_f32(db, "db").numel() != cols):
        raise ValueError("split_f16x3_rows_colstats: db size")
    dev = x.device
    y = torch.empty((rows, pieces * cols), dtype=torch.float16, device=dev)
    ra = torch.empty((rows,), dtype=torch.float32, device=dev)
    yc = torch.empty((rows, 2 * cols), dtype=torch.float16, device=dev)
    ce = torch.empty((cols,), dtype=torch.int32, device=dev)
    ca = torch.empty((cols,), dtype=torch.float32, device=dev)
    nbytes = lib.dclip_split_f32_f16x3_rows_colstats_workspace(rows, cols)
    ws = _ws.get(nbytes, dev)
    _lib.check((lib.dclip_split_f32_f16x2_rows_colstats if pieces == 2 else lib.dclip_split_f32_f16x3_rows_colstats)(x.data_ptr(), y.data_ptr(), ra.data_ptr(), yc.data_ptr(), ce.data_ptr(),
                                                       ca.data_ptr(), _ptr(db), rows, cols, x.stride(0) if rows > 1 else cols,
                                                       _ptr(ws), nbytes, _stream()), "split_f32_f16x3_rows_colstats")
    return y, ra, yc, ce, ca


def split_f16x3_rows_cols_stats(x: torch.Tensor, stats: ColStats, db: Optional[torch.Tensor] = None, pieces: int = 3):
    """split_f16x3_rows_colstats for an x whose producer left its column partials in `stats`: the finish over
    the partial rows, then ONE pass over x.  The same five outputs, bit for bit; `db` is another association of the same sums.
    `pieces` as there."""
    lib = _lib.load()
    if x.dtype != torch.float32 or not x.is_cuda or x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("split_f16x3_rows_cols_stats: x must be a 2-D fp32 device tensor with unit column stride")
    rows, cols = x.shape
    if stats.cols != cols or stats.P <= 0:
        raise ValueError("split_f16x3_rows_cols_stats: stats columns")
    if db is not None and (_f32(db, "db").numel() != cols):
        raise ValueError("split_f16x3_rows_cols_stats: db size")
    dev = x.device
    y = torch.empty((rows, pieces * cols), dtype=torch.float16, device=dev)
    ra = torch.empty((rows,), dtype=torch.float32, device=dev)
    yc = torch.empty((rows, 2 * cols), dtype=torch.float16, device=dev)
    ce = torch.empty((cols,), dtype=torch.int32, device=dev)
    ca = torch.empty((cols,), dtype=torch.float32, device=dev)
    _lib.check((lib.dclip_split_f32_f16x2_rows_cols_stats if pieces == 2 else lib.dclip_split_f32_f16x3_rows_cols_stats)(x.data_ptr(), y.data_ptr(), ra.data_ptr(), yc.data_ptr(), ce.data_ptr(),
                                                         ca.data_ptr(), _ptr(db), stats.pmax.data_ptr(), stats.psum.data_ptr(), stats.P,
                                                         rows, cols, x.stride(0) if rows > 1 else cols, _stream()),
               "split_f32_f16x3_rows_cols_stats")
    return y, ra, yc, ce, ca


def gemm_f16_wgrad_tokmajor_seg3_plan(M: int, N: int, tokens: int) -> int:
    """The split count gemm_f16_wgrad_tokmajor_seg3 would take, 0 when the form does not apply to the shape."""
    return int(_lib.load().dclip_gemm_f16_wgrad_tokmajor_seg3_plan(M, N, tokens))


def gemm_f16_wgrad_tokmajor_seg3(dy: torch.Tensor, x: torch.Tensor, M: int, N: int, col_alpha: torch.Tensor, act_scale_ptr: int,
                                 a_seg=None, w_seg=None, splits: Optional[int] = None,
                                 out: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """dW [M, N] fp32 = ((sum of three segments dy_s^T x_s) / *act_scale_ptr) * col_alpha[m] from fp16 token-major operands
    dy [tokens, >= a_seg + M], x [tokens, >= w_seg + N].  The default segments pair dy = [hi|lo] with x =
    [hi|lo|hi]: hi.hi + lo.hi + hi.lo.  None when the form does not apply (and `splits` is left to the plan)."""
    lib = _lib.load()
    _f16(dy, "dy"), _f16(x, "x")
    if dy.dim() != 2 or x.dim() != 2 or dy.shape[0] != x.shape[0]:
        raise ValueError("gemm_f16_wgrad_tokmajor_seg3: dy / x are [tokens, ld] with the same token count")
    tokens = dy.shape[0]
    a_seg = (0, M, 0) if a_seg is None else tuple(int(v) for v in a_seg)
    w_seg = (0, 0, N) if w_seg is None else tuple(int(v) for v in w_seg)
    if splits is None:
        splits = lib.dclip_gemm_f16_wgrad_tokmajor_seg3_plan(M, N, tokens)
        if splits == 0:
            return None
    if _f32(col_alpha, "col_alpha").numel() != M:
        raise ValueError("gemm_f16_wgrad_tokmajor_seg3: col_alpha size")
    out = _out_f32(out, (M, N), dy.device, "gemm_f16_wgrad_tokmajor_seg3")
    nbytes = lib.dclip_gemm_f16_splitk_workspace(M, N, 3 * splits)
    ws = _ws.get(nbytes, dy.device)
    _lib.check(lib.dclip_gemm_f16_wgrad_tokmajor_seg3(dy.data_ptr(), x.data_ptr(), out.data_ptr(), M, N, tokens, dy.shape[1], x.shape[1],
                                                      N, a_seg[0], a_seg[1], a_seg[2], w_seg[0], w_seg[1], w_seg[2],
                                                      col_alpha.data_ptr(), act_scale_ptr, splits, _ptr(ws), nbytes, _stream()),
               "gemm_f16_wgrad_tokmajor_seg3")
    return out


# ------------------------------------------------------------------------------------------- fused split-fp16 GEMMs
# The split GEMMs above with each of the four distinct pieces staged once (include/dclip_hip.h, "fused split-fp16 GEMMs"): the same
# operands as they lie — a = [hi|lo|hi], w = [hi|hi|lo], dy = [hi|lo], x = [hi|lo|hi] — the same epilogues and outputs; the
# duplicate third is not read.  The plans say where the step takes them.

def gemm_f16x3_plan(M: int, N: int, K: int) -> int:
    """1 where the step takes a fused K-major entry for logical K (where the 3 K form takes the ping-pong kernel), else 0."""
    return int(_lib.load().dclip_gemm_f16x3_plan(M, N, K))


def gemm_f16x3_tile_rows(M: int, N: int, K: int, rows_form: bool = False, stats_form: bool = False) -> int:
    """Tile height (192 or 256) a fused K-major fp32-output call of this shape takes now."""
    return int(_lib.load().dclip_gemm_f16x3_tile_rows(M, N, K, int(rows_form), int(stats_form)))


def _x3_k(a: torch.Tensor, w: torch.Tensor, name: str, pieces: int = 3):
    """(M, N, K, lda, ldw) of a fused call.  `pieces` = 2: a is [hi|lo] [M, 2 K] — K cannot be read off a 2 K
    and a 3 K width together, so the caller says which; w is [hi|hi|lo] [N, 3 K] either way."""
    _f16(a, "a"), _f16(w, "w")
    M, lda = a.shape
    N, ldw = w.shape
    if pieces == 2:
        if lda % 2 or ldw < 3 * (lda // 2):
            raise ValueError(f"{name}: a is a [rows, 2 K] split and w a [rows, 3 K] one")
        return M, N, lda // 2, lda, ldw
    if pieces != 3:
        raise ValueError(f"{name}: pieces is 2 or 3")
    if min(lda, ldw) % 3:
        raise ValueError(f"{name}: a / w are [rows, 3 K] splits")
    K = min(lda, ldw) // 3
    return M, N, K, lda, ldw


def gemm_f16x3(a: torch.Tensor, w: torch.Tensor, *, bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
               gelu: bool = False, out_f16: bool = False, alpha: float = 1.0, split_out_scale: Optional[float] = None,
               segs=None, pieces: int = 3, out_pieces: int = 3) -> torch.Tensor:
    """gemm_f16(alpha=..., split_out_scale=...) of a = [hi|lo|hi] [M, 3K] and w = [hi|hi|lo] [N, 3K] on the fused kernel.
    `segs` = (a_hi, a_lo, w_hi, w_lo) column offsets, default (0, K, 0, 2K).  `pieces` = 2: a is [hi|lo] [M, 2K]; `out_pieces` = 2:
    a split output is [hi|lo] [M, 2N]."""
    lib = _lib.load()
    M, N, K, lda, ldw = _x3_k(a, w, "gemm_f16x3", pieces)
    sg = (0, K, 0, 2 * K) if segs is None else tuple(int(v) for v in segs)
    epi = 0
    if bias is not None:
        epi |= EPI_BIAS
        if _f32(bias, "bias").numel() != N:
            raise ValueError("gemm_f16x3: bias size")
    if gelu:
        epi |= EPI_GELU
    if residual is not None:
        epi |= EPI_RESIDUAL
        if tuple(_f32(residual, "residual").shape) != (M, N):
            raise ValueError("gemm_f16x3: residual shape")
    if split_out_scale is not None:
        if residual is not None or out_f16:
            raise ValueError("gemm_f16x3: a split output takes bias / gelu only")
        y3 = torch.empty((M, out_pieces * N), dtype=torch.float16, device=a.device)
        fn = lib.dclip_gemm_f16x3_scaled_split2 if out_pieces == 2 else lib.dclip_gemm_f16x3_scaled_split
        _lib.check(fn(a.data_ptr(), w.data_ptr(), y3.data_ptr(), _ptr(bias), M, N, K, lda, ldw, out_pieces * N, *sg, epi, float(alpha),
                      float(split_out_scale), _stream()), "gemm_f16x3_scaled_split")
        return y3
    out = torch.empty((M, N), dtype=torch.float16 if out_f16 else torch.float32, device=a.device)
    _lib.check(lib.dclip_gemm_f16x3_scaled(a.data_ptr(), w.data_ptr(), out.data_ptr(), _ptr(bias), _ptr(residual), M, N, K, lda, ldw,
                                           N, *sg, epi, int(out_f16), float(alpha), _stream()), "gemm_f16x3_scaled")
    return out


def gemm_f16x3_dev(a: torch.Tensor, w: torch.Tensor, alpha_ptr: int, *, bias: Optional[torch.Tensor] = None,
                   residual: Optional[torch.Tensor] = None, gelu: bool = False, out_f16: bool = False,
                   split_out_scale_ptr: Optional[int] = None, h32: Optional[torch.Tensor] = None,
                   g32: Optional[torch.Tensor] = None, segs=None, pieces: int = 3, out_pieces: int = 3) -> torch.Tensor:
    """gemm_f16_dev on the fused kernel: the same arguments and outputs; `pieces` / `out_pieces` as gemm_f16x3's."""
    lib = _lib.load()
    M, N, K, lda, ldw = _x3_k(a, w, "gemm_f16x3_dev", pieces)
    sg = (0, K, 0, 2 * K) if segs is None else tuple(int(v) for v in segs)
    epi = 0
    if bias is not None:
        epi |= EPI_BIAS
        if _f32(bias, "bias").numel() != N:
            raise ValueError("gemm_f16x3_dev: bias size")
    if gelu:
        epi |= EPI_GELU
    if residual is not None:
        epi |= EPI_RESIDUAL
        if tuple(_f32(residual, "residual").shape) != (M, N):
            raise ValueError("gemm_f16x3_dev: residual shape")
    if split_out_scale_ptr is not None:
        if residual is not None or out_f16:
            raise ValueError("gemm_f16x3_dev: a split output takes bias / gelu only")
        for t, nm in ((h32, "h32"), (g32, "g32")):
            if t is not None and tuple(_f32(t, nm).shape) != (M, N):
                raise ValueError(f"gemm_f16x3_dev: {nm} shape")
        if h32 is not None and not gelu:
            raise ValueError("gemm_f16x3_dev: h32 is the pre-activation of a gelu epilogue")
        y3 = torch.empty((M, out_pieces * N), dtype=torch.float16, device=a.device)
        fn = lib.dclip_gemm_f16x3_scaled_split2_dev if out_pieces == 2 else lib.dclip_gemm_f16x3_scaled_split_dev
        _lib.check(fn(a.data_ptr(), w.data_ptr(), y3.data_ptr(), _ptr(bias), _ptr(h32), _ptr(g32), M, N, K, lda, ldw, out_pieces * N,
                      *sg, epi, alpha_ptr, split_out_scale_ptr, _stream()), "gemm_f16x3_scaled_split_dev")
        return y3
    if g32 is not None:
        raise ValueError("gemm_f16x3_dev: g32 goes with a split output")
    out = torch.empty((M, N), dtype=torch.float16 if out_f16 else torch.float32, device=a.device)
    if h32 is not None:      # fp32 result and fp32 pre-activation, no split
        if not gelu or residual is not None or out_f16 or tuple(_f32(h32, "h32").shape) != (M, N) or N % 8:
            raise ValueError("gemm_f16x3_dev: h32 [M, N] is the pre-activation of a bias / gelu epilogue with an fp32 result")
        _lib.check(lib.dclip_gemm_f16x3_scaled_split_dev(a.data_ptr(), w.data_ptr(), out.data_ptr(), _ptr(bias), h32.data_ptr(), None,
                                                         M, N, K, lda, ldw, N, *sg, epi, alpha_ptr, None, _stream()),
                   "gemm_f16x3_scaled_split_dev")
        return out
    _lib.check(lib.dclip_gemm_f16x3_scaled_dev(a.data_ptr(), w.data_ptr(), out.data_ptr(), _ptr(bias), _ptr(residual), M, N, K, lda,
                                               ldw, N, *sg, epi, int(out_f16), alpha_ptr, _stream()), "gemm_f16x3_scaled_dev")
    return out


def gemm_f16x3_rows_stats_plan(M: int, N: int, K: int) -> int:
    """Partial rows gemm_f16x3_rows_dev leaves with `stats` (ceil(M / 256)) where gemm_f16x3_plan holds for logical K, else 0."""
    return int(_lib.load().dclip_gemm_f16x3_scaled_rows_stats_plan(M, N, K))


def gemm_f16x3_rows_dev(a: torch.Tensor, w: torch.Tensor, alpha_ptr: int, row_alpha: torch.Tensor,
                        dgelu_h: Optional[torch.Tensor] = None, stats: Optional[ColStats] = None, segs=None,
                        pieces: int = 3) -> torch.Tensor:
    """gemm_f16_rows_dev on the fused kernel; `stats` has ceil(M / 256) partial rows and N columns; `pieces` as gemm_f16x3's."""
    lib = _lib.load()
    M, N, K, lda, ldw = _x3_k(a, w, "gemm_f16x3_rows_dev", pieces)
    sg = (0, K, 0, 2 * K) if segs is None else tuple(int(v) for v in segs)
    if _f32(row_alpha, "row_alpha").numel() != M:
        raise ValueError("gemm_f16x3_rows_dev: row_alpha size")
    if dgelu_h is not None and tuple(_f32(dgelu_h, "dgelu_h").shape) != (M, N):
        raise ValueError("gemm_f16x3_rows_dev: dgelu_h shape")
    out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    epi = EPI_DGELU if dgelu_h is not None else 0
    if stats is not None:
        if (stats.P, stats.cols) != ((M + 255) // 256, N):
            raise ValueError("gemm_f16x3_rows_dev: stats must have ceil(M / 256) rows and N columns")
        _lib.check(lib.dclip_gemm_f16x3_scaled_rows_stats_dev(a.data_ptr(), w.data_ptr(), out.data_ptr(), _ptr(dgelu_h), M, N, K, lda,
                                                              ldw, N, *sg, epi, alpha_ptr, row_alpha.data_ptr(),
                                                              stats.pmax.data_ptr(), stats.psum.data_ptr(), _stream()),
                   "gemm_f16x3_scaled_rows_stats_dev")
        return out
    _lib.check(lib.dclip_gemm_f16x3_scaled_rows_dev(a.data_ptr(), w.data_ptr(), out.data_ptr(), _ptr(dgelu_h), M, N, K, lda, ldw, N,
                                                    *sg, epi, alpha_ptr, row_alpha.data_ptr(), _stream()),
               "gemm_f16x3_scaled_rows_dev")
    return out


def gemm_f16x3_wgrad_tokmajor_plan(M: int, N: int, tokens: int) -> int:
    """The split count gemm_f16x3_wgrad_tokmajor would take, 0 where the step keeps gemm_f16_wgrad_tokmajor_seg3 (or neither applies)."""
    return int(_lib.load().dclip_gemm_f16x3_wgrad_tokmajor_plan(M, N, tokens))


def gemm_f16x3_wgrad_tokmajor(dy: torch.Tensor, x: torch.Tensor, M: int, N: int, col_alpha: torch.Tensor, act_scale_ptr: int,
                              segs=None, splits: Optional[int] = None,
                              out: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """gemm_f16_wgrad_tokmajor_seg3's dW on the fused kernel: hi.hi + lo.hi + hi.lo of dy = [hi|lo] and x = [hi|lo|..] (three
    pieces or two: the third is not read), `segs` = (dy_hi, dy_lo, x_hi, x_lo) column offsets, default (0, M, 0, N).  None when
    the plan is 0 (and `splits` is left to it)."""
    lib = _lib.load()
    _f16(dy, "dy"), _f16(x, "x")
    if dy.dim() != 2 or x.dim() != 2 or dy.shape[0] != x.shape[0]:
        raise ValueError("gemm_f16x3_wgrad_tokmajor: dy / x are [tokens, ld] with the same token count")
    tokens = dy.shape[0]
    sg = (0, M, 0, N) if segs is None else tuple(int(v) for v in segs)
    if splits is None:
        splits = lib.dclip_gemm_f16x3_wgrad_tokmajor_plan(M, N, tokens)
        if splits == 0:
            return None
    if _f32(col_alpha, "col_alpha").numel() != M:
        raise ValueError("gemm_f16x3_wgrad_tokmajor: col_alpha size")
    out = _out_f32(out, (M, N), dy.device, "gemm_f16x3_wgrad_tokmajor")
    nbytes = lib.dclip_gemm_f16x3_wgrad_tokmajor_workspace(M, N, splits)
    ws = _ws.get(nbytes, dy.device)
    _lib.check(lib.dclip_gemm_f16x3_wgrad_tokmajor(dy.data_ptr(), x.data_ptr(), out.data_ptr(), M, N, tokens, dy.shape[1], x.shape[1],
                                                   N, *sg, col_alpha.data_ptr(), act_scale_ptr, splits, _ptr(ws), nbytes, _stream()),
               "gemm_f16x3_wgrad_tokmajor")
    return out


# ------------------------------------------------------------------------------------------- split-fp16 patch embedding
# The operands of the student's patch embedding and of its weight gradient (include/dclip_hip.h, "the student's patch embedding"):
# the GEMMs themselves are gemm_f16x3_dev and gemm_f16x3_wgrad_tokmajor above.

FRONT_SCALE, FRONT_WSCALE, FRONT_ALPHA, FRONT_FLAGS, FRONT_PIX_MAX, FRONT_W_MAX, FRONT_E, FRONT_F = range(8)   # floats of a front record


def split16_patch_plan(rows: int, D: int, K: int) -> int:
    """1 where the step takes the split path for a patch embedding [rows, K] x [D, K] (gemm_f16x3_plan and a tile threshold of
    its own, DCLIP_PATCH_SPLIT16_MIN), else 0."""
    return int(_lib.load().dclip_split16_patch_plan(rows, D, K))


def im2col_f16x2(pixels: torch.Tensor, patch: int, scale: float = 1.0, scale_ptr: Optional[int] = None) -> torch.Tensor:
    """im2col written as the two-piece split: fp16 [B*g*g, 2 C p p] = [hi|lo] of pixel * scale (a power of two; `scale_ptr`: the
    address of a device float instead), bit-equal to split_f16x3(im2col(pixels), scale, pieces=2) in one pass; patch % 8 == 0."""
    lib = _lib.load()
    _f32(pixels, "pixel_values")
    B, Cc, Hh, Ww = pixels.shape
    if patch <= 0 or Hh != Ww or Hh % patch or patch % 8:
        raise ValueError(f"im2col_f16x2: image {Hh}x{Ww}, patch {patch} (a square image of whole patches, patch % 8 == 0)")
    g = Hh // patch
    cols = torch.empty((B * g * g, 2 * Cc * patch * patch), dtype=torch.float16, device=pixels.device)
    _lib.check(lib.dclip_im2col_f16x2(pixels.data_ptr(), cols.data_ptr(), B, Cc, Hh, Ww, patch, float(scale), scale_ptr, _stream()),
               "im2col_f16x2")
    return cols


def split16_front_state(w: torch.Tensor) -> dict:
    """What split16_front keeps between calls for the weight w [D, K] (K % 8 == 0): the weight record and the [hi|hi|lo] copy."""
    lib = _lib.load()
    _f32(w, "w")
    if w.dim() != 2 or w.shape[1] % 8:
        raise ValueError("split16_front_state: w is [D, K] with K % 8 == 0")
    return {"wrec": torch.zeros((lib.dclip_split16_front_wrec_floats(),), dtype=torch.float32, device=w.device),
            "w3": torch.empty((w.shape[0], 3 * w.shape[1]), dtype=torch.float16, device=w.device)}


def split16_front(pixels: torch.Tensor, w: torch.Tensor, state: dict, refresh_w: bool) -> torch.Tensor:
    """The front plan of one forward -> its record, fp32 [8] on the device (FRONT_*): the scales 2^e from max|pixels| and 2^f from
    max|w|, alpha = 2^-(e+f) and the guard flags.  `refresh_w`: w changed — its maximum, state["wrec"] and state["w3"] = [hi|hi|lo]
    of w 2^f are made again; otherwise they are read as they stand.  Two launches, three with `refresh_w`; nothing is read back."""
    lib = _lib.load()
    _f32(pixels, "pixel_values"), _f32(w, "w")
    rec = torch.empty((lib.dclip_split16_front_rec_floats(),), dtype=torch.float32, device=pixels.device)
    w3 = state["w3"]
    if tuple(w3.shape) != (w.shape[0], 3 * w.shape[1]):
        raise ValueError("split16_front: the state was made for another weight shape")
    nbytes = lib.dclip_split16_front_workspace()
    ws = _ws.get(nbytes, pixels.device)
    _lib.check(lib.dclip_split16_front(pixels.data_ptr(), pixels.numel(), w.data_ptr(), w.shape[0], w.shape[1], w3.data_ptr(),
                                       state["wrec"].data_ptr(), rec.data_ptr(), _ptr(ws), nbytes, int(bool(refresh_w)), _stream()),
               "split16_front")
    return rec


def split_f16x2_cols(x: torch.Tensor):
    """The column-only split of a dY -> (yc, col_exp, col_alpha), bit-equal to the outputs of those names of
    split_f16x3_rows_colstats on the same x; no row pieces, no column sums."""
    lib = _lib.load()
    if x.dtype != torch.float32 or not x.is_cuda or x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("split_f16x2_cols: x must be a 2-D fp32 device tensor with unit column stride")
    rows, cols = x.shape
    dev = x.device
    yc = torch.empty((rows, 2 * cols), dtype=torch.float16, device=dev)
    ce = torch.empty((cols,), dtype=torch.int32, device=dev)
    ca = torch.empty((cols,), dtype=torch.float32, device=dev)
    nbytes = lib.dclip_split_f32_f16x2_cols_workspace(rows, cols)
    ws = _ws.get(nbytes, dev)
    _lib.check(lib.dclip_split_f32_f16x2_cols(x.data_ptr(), yc.data_ptr(), ce.data_ptr(), ca.data_ptr(), rows, cols,
                                              x.stride(0) if rows > 1 else cols, _ptr(ws), nbytes, _stream()), "split_f32_f16x2_cols")
    return yc, ce, ca


# ------------------------------------------------------------------------------------------- fp16 training path
# The bf16 training wrappers above with fp16 tensors (include/dclip_hip.h, "fp16 TRAINING path"): same shapes and limits,
# IEEE rounding — a value beyond +-65504 becomes +-inf (the frozen fp16 wrappers above saturate), so that the overflow of a
# loss-scaled gradient reaches the gradient norm (amp.DynamicLossScaler).

def cast_f16_ieee(x: torch.Tensor, pad_to: int = 8, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """cast_f16 with IEEE rounding: [rows, cols] fp32 -> fp16 [rows, cols rounded up to pad_to]; `out`: refresh in place."""
    lib = _lib.load()
    _f32(x, "x")
    if x.dim() != 2:
        raise ValueError("cast_f16_ieee: x must be 2-D")
    rows, cols = x.shape
    ld = (cols + pad_to - 1) // pad_to * pad_to
    if out is not None:
        if tuple(_f16(out, "out").shape) != (rows, ld):
            raise ValueError(f"cast_f16_ieee: out shape {tuple(out.shape)} != {(rows, ld)}")
        y = out
    else:
        y = torch.empty((rows, ld), dtype=torch.float16, device=x.device)
    _lib.check(lib.dclip_cast_f32_f16_ieee(x.data_ptr(), y.data_ptr(), rows, cols, cols, ld, _stream()), "cast_f32_f16_ieee")
    return y


def layernorm_fwd_f16_stats(x, gamma, beta, eps: float):
    """nn.LayerNorm with fp32 statistics and an fp16 result (IEEE rounding) -> (y, mean, rstd) for the backward."""
    lib = _lib.load()
    _f32(x, "x"), _f32(gamma, "gamma"), _f32(beta, "beta")
    D = x.shape[-1]
    rows = x.numel() // D
    y = torch.empty(x.shape, dtype=torch.float16, device=x.device)
    mean = torch.empty((rows,), dtype=torch.float32, device=x.device)
    rstd = torch.empty((rows,), dtype=torch.float32, device=x.device)
    _lib.check(lib.dclip_layernorm_fwd_f16_stats(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), mean.data_ptr(),
                                                 rstd.data_ptr(), rows, D, float(eps), _stream()), "layernorm_fwd_f16_stats")
    return y, mean, rstd


def transpose_f16(x: torch.Tensor, want_copy: bool = False, out: Optional[torch.Tensor] = None):
    """transpose_bf16 with fp16 results: x [rows, cols] fp32 or fp16 -> x^T [cols, rows rounded up to 8] (and the copy)."""
    lib = _lib.load()
    if not (x.is_cuda and x.is_contiguous() and x.dim() == 2 and x.dtype in (torch.float32, torch.float16)):
        raise ValueError("transpose_f16: contiguous 2-D float32 / float16 CUDA tensor")
    rows, cols = x.shape
    if cols % 4:
        raise ValueError("transpose_f16: cols must be a multiple of 4")
    ld = (rows + 7) // 8 * 8
    if out is not None:
        if tuple(_f16(out, "out").shape) != (cols, ld):
            raise ValueError(f"transpose_f16: out shape {tuple(out.shape)} != {(cols, ld)}")
        yT = out
    else:
        yT = torch.empty((cols, ld), dtype=torch.float16, device=x.device)
    copy = None
    if want_copy:
        if cols % 8:
            raise ValueError("transpose_f16: the fp16 copy feeds a GEMM as A: cols must be a multiple of 8")
        copy = torch.empty((rows, cols), dtype=torch.float16, device=x.device)
    _lib.check(lib.dclip_transpose_to_f16(x.data_ptr(), int(x.dtype == torch.float16), yT.data_ptr(), _ptr(copy), rows, cols,
                                          cols, ld, cols, _stream()), "transpose_to_f16")
    return (yT, copy) if want_copy else yT


def mt_weights_f16(table: torch.Tensor, ntensors: int, total_tiles: int) -> None:
    lib = _lib.load()
    _lib.check(lib.dclip_mt_weights_f16(table.data_ptr(), ntensors, total_tiles, _stream()), "mt_weights_f16")


def rowsum_f16(x: torch.Tensor, n: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Row sums (fp32) of the first n columns of an fp16 matrix [R, ld]."""
    lib = _lib.load()
    _f16(x, "x")
    R, ld = x.shape
    n = ld if n is None else n
    out = _out_f32(out, (R,), x.device, "rowsum_f16")
    _lib.check(lib.dclip_rowsum_f16(x.data_ptr(), out.data_ptr(), R, n, ld, _stream()), "rowsum_f16")
    return out


def colsum_f16(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Column sums of an fp16 matrix, fp32 result."""
    lib = _lib.load()
    _f16(x, "x")
    M, N = x.shape
    out = _out_f32(out, (N,), x.device, "colsum_f16")
    nbytes = lib.dclip_colsum_f32_workspace(M, N)
    ws = _ws.get(nbytes, x.device)
    _lib.check(lib.dclip_colsum_f16(x.data_ptr(), out.data_ptr(), M, N, N, 0, _ptr(ws), nbytes, _stream()), "colsum_f16")
    return out


def attention_fwd_f16_lse(qkv: torch.Tensor, B: int, S: int, H: int, causal: bool):
    """attention_fwd_bf16_lse on fp16 (S <= 64): qkv [B*S, 3*H*64] fp16 -> (context fp16, lse fp32 [B*H, S])."""
    lib = _lib.load()
    _f16(qkv, "qkv")
    if tuple(qkv.shape) != (B * S, 3 * H * 64):
        raise ValueError(f"attention_fwd_f16_lse: qkv shape {tuple(qkv.shape)} != {(B * S, 3 * H * 64)}")
    out = torch.empty((B * S, H * 64), dtype=torch.float16, device=qkv.device)
    lse = torch.empty((B * H, S), dtype=torch.float32, device=qkv.device)
    _lib.check(lib.dclip_attention_fwd_f16_lse(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), B, S, H, int(causal), _stream()),
               "attention_fwd_f16_lse")
    return out, lse


def attention_bwd_f16(qkv, out, dout, lse, B: int, S: int, H: int, causal: bool) -> torch.Tensor:
    """Backward of attention_fwd_f16_lse on the fp16 MFMAs (S <= 64): returns dqkv [B*S, 3*H*64] fp16."""
    lib = _lib.load()
    _f16(qkv, "qkv"), _f16(out, "out"), _f16(dout, "dout"), _f32(lse, "lse")
    D = H * 64
    if tuple(qkv.shape) != (B * S, 3 * D) or tuple(out.shape) != (B * S, D) or tuple(dout.shape) != (B * S, D) \
            or lse.numel() != B * H * S:
        raise ValueError("attention_bwd_f16: shape mismatch")
    dqkv = torch.empty_like(qkv)
    _lib.check(lib.dclip_attention_bwd_f16(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), dqkv.data_ptr(),
                                           B, S, H, int(causal), _stream()), "attention_bwd_f16")
    return dqkv


def gemm_f16_train(a: torch.Tensor, w: torch.Tensor, *, n: Optional[int] = None, k: Optional[int] = None,
                   bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None, gelu: bool = False,
                   out_f16: bool = False, save_preact: bool = False, dgelu_of: Optional[torch.Tensor] = None,
                   out: Optional[torch.Tensor] = None):
    """gemm_bf16 with its training epilogues on fp16 operands (dclip_gemm_f16_ex, IEEE rounding of every 16-bit output):
    `save_preact` (with gelu) also returns the fp16 pre-activation -> (y, h); `dgelu_of=h` multiplies by quick_gelu'(h)."""
    lib = _lib.load()
    _f16(a, "a"), _f16(w, "w")
    M, lda = a.shape
    N, ldw = w.shape
    K = k if k is not None else min(lda, ldw)
    if n is not None:
        N = n
    epi = 0
    if bias is not None:
        epi |= EPI_BIAS
        if _f32(bias, "bias").numel() != N:
            raise ValueError("gemm_f16_train: bias size")
    if gelu:
        epi |= EPI_GELU
    if residual is not None:
        epi |= EPI_RESIDUAL
        if tuple(_f32(residual, "residual").shape) != (M, N):
            raise ValueError("gemm_f16_train: residual shape")
    odt = torch.float16 if out_f16 else torch.float32
    if out is None:
        out = torch.empty((M, N), dtype=odt, device=a.device)
    elif tuple(out.shape) != (M, N) or out.dtype != odt or not out.is_contiguous():
        raise ValueError("gemm_f16_train: out shape / dtype")
    aux = None
    if save_preact:
        if not gelu:
            raise ValueError("gemm_f16_train: save_preact goes with gelu")
        aux = torch.empty((M, N), dtype=torch.float16, device=a.device)
    if dgelu_of is not None:
        if gelu or tuple(_f16(dgelu_of, "dgelu_of").shape) != (M, N):
            raise ValueError("gemm_f16_train: dgelu_of must be the [M, N] fp16 pre-activation (and excludes gelu)")
        epi |= EPI_DGELU
        aux = dgelu_of
    _lib.check(lib.dclip_gemm_f16_ex(a.data_ptr(), w.data_ptr(), out.data_ptr(), _ptr(bias), _ptr(residual), _ptr(aux), M, N, K,
                                     lda, ldw, N, epi, int(out_f16), _stream()), "gemm_f16_ex")
    return (out, aux) if save_preact else out


def gemm_f16_wgrad(a: torch.Tensor, w: torch.Tensor, k: int, splits: Optional[int] = None,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """gemm_bf16_wgrad on fp16 token-contiguous operands (a = dY^T [M, ld], w = X^T [N, ld]) -> dW [M, N] fp32."""
    lib = _lib.load()
    _f16(a, "a"), _f16(w, "w")
    M, lda = a.shape
    N, ldw = w.shape
    if splits is None:
        splits = lib.dclip_gemm_f16_splitk_plan(M, N, k)
    out = _out_f32(out, (M, N), a.device, "gemm_f16_wgrad")
    nbytes = lib.dclip_gemm_f16_splitk_workspace(M, N, splits)
    ws = _ws.get(nbytes, a.device)
    _lib.check(lib.dclip_gemm_f16_splitk(a.data_ptr(), w.data_ptr(), out.data_ptr(), M, N, k, lda, ldw, N, splits,
                                         _ptr(ws), nbytes, _stream()), "gemm_f16_splitk")
    return out


def gemm_f16_wgrad_tokmajor(dy: torch.Tensor, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """gemm_bf16_wgrad_tokmajor on fp16 operands dy [tokens, out], x [tokens, in]; None when the form does not apply."""
    lib = _lib.load()
    _f16(dy, "dy"), _f16(x, "x")
    K, M = dy.shape
    K2, N = x.shape
    if K != K2:
        raise ValueError("gemm_f16_wgrad_tokmajor: token counts differ")
    splits = lib.dclip_gemm_f16_wgrad_tokmajor_plan(M, N, K)
    if splits == 0:
        return None
    out = _out_f32(out, (M, N), dy.device, "gemm_f16_wgrad_tokmajor")
    nbytes = lib.dclip_gemm_f16_splitk_workspace(M, N, splits)
    ws = _ws.get(nbytes, dy.device)
    _lib.check(lib.dclip_gemm_f16_wgrad_tokmajor(dy.data_ptr(), x.data_ptr(), out.data_ptr(), M, N, K, M, N, N, splits,
                                                 _ptr(ws), nbytes, _stream()), "gemm_f16_wgrad_tokmajor")
    return out


# ------------------------------------------------------------------------------------------- crop front end

def crop_resize(images_u8: torch.Tensor, dims: torch.Tensor, boxes: torch.Tensor, size: int,
                max_crop_h: int, max_crop_w: int) -> torch.Tensor:
    """images_u8 [B,Hmax,Wmax,3] uint8, dims [B,2] int32 (h,w), boxes [NR,5] int32 (b,x1,y1,x2,y2) -> [NR,3,S,S] fp32.
    max_crop_h/w must bound the boxes' extents (the caller has the box list on the host anyway)."""
    lib = _lib.load()
    if not (images_u8.is_cuda and images_u8.dtype == torch.uint8 and images_u8.is_contiguous() and images_u8.dim() == 4
            and images_u8.shape[3] == 3):
        raise ValueError("crop_resize: images must be a contiguous uint8 CUDA tensor [B,H,W,3]")
    B, Hmax, Wmax, _ = images_u8.shape
    for t, n, shape in ((dims, "dims", (B, 2)), (boxes, "boxes", (boxes.shape[0], 5))):
        if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == shape):
            raise ValueError(f"crop_resize: {n} must be a contiguous int32 CUDA tensor {shape}")
    NR = boxes.shape[0]
    if NR == 0 or max_crop_h <= 0 or max_crop_w <= 0:
        raise ValueError("crop_resize: empty box list")
    out = torch.empty((NR, 3, size, size), dtype=torch.float32, device=images_u8.device)
    nbytes = lib.dclip_crop_resize_workspace(NR, size, max_crop_h, max_crop_w)
    ws = _ws.get(nbytes, images_u8.device)
    _lib.check(lib.dclip_crop_resize_u8(images_u8.data_ptr(), dims.data_ptr(), boxes.data_ptr(), out.data_ptr(), B, Hmax,
                                        Wmax, NR, size, max_crop_h, max_crop_w, _ptr(ws), nbytes, _stream()),
               "crop_resize_u8")
    return out


CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def clip_preprocess(images_u8: torch.Tensor, dims: torch.Tensor, size: int = 224, mean=CLIP_MEAN, std=CLIP_STD) -> torch.Tensor:
    """images_u8 [B,Hmax,Wmax,3] uint8 (image b in the top-left dims[b]=(h,w) corner) -> pixel_values [B,3,S,S] fp32:
    shortest-edge BICUBIC resize, centre crop, 1/255, (x-mean)/std — bit-exact with HF CLIPImageProcessor (PIL)."""
    import ctypes
    lib = _lib.load()
    if not (images_u8.is_cuda and images_u8.dtype == torch.uint8 and images_u8.is_contiguous() and images_u8.dim() == 4
            and images_u8.shape[3] == 3):
        raise ValueError("clip_preprocess: images must be a contiguous uint8 CUDA tensor [B,H,W,3]")
    B, Hmax, Wmax, _ = images_u8.shape
    if not (dims.is_cuda and dims.dtype == torch.int32 and dims.is_contiguous() and tuple(dims.shape) == (B, 2)):
        raise ValueError("clip_preprocess: dims must be a contiguous int32 CUDA tensor [B,2]")
    out = torch.empty((B, 3, size, size), dtype=torch.float32, device=images_u8.device)
    nbytes = lib.dclip_clip_preprocess_workspace(B, Hmax, Wmax, size)
    ws = _ws.get(nbytes, images_u8.device)
    m = (ctypes.c_float * 3)(*[float(v) for v in mean])
    s = (ctypes.c_float * 3)(*[float(v) for v in std])
    _lib.check(lib.dclip_clip_preprocess_u8(images_u8.data_ptr(), dims.data_ptr(), out.data_ptr(), B, Hmax, Wmax, size,
                                            ctypes.cast(m, ctypes.c_void_p), ctypes.cast(s, ctypes.c_void_p), _ptr(ws),
                                            nbytes, _stream()), "clip_preprocess_u8")
    return out


# ------------------------------------------------------------------------------------------- packed (variable-length) tower

def _i32(t: torch.Tensor, name: str, shape) -> torch.Tensor:
    if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == tuple(shape)):
        raise ValueError(f"{name}: expected a contiguous int32 CUDA tensor {tuple(shape)}, got {t.dtype} {t.device} {tuple(t.shape)}")
    return t


def patches_from_boxes_u8(images_u8: torch.Tensor, dims: torch.Tensor, boxes: torch.Tensor, patch_offsets: torch.Tensor,
                          total_patches: int, patch: int) -> torch.Tensor:
    """Patch rows [total_patches, 3*patch*patch] in [0,1] of the crops boxes [N,5] = (b,x1,y1,x2,y2) of images_u8
    [B,Hmax,Wmax,3] (dims [B,2] = (h,w)), crop n at rows patch_offsets[n] .. patch_offsets[n+1]-1 in the column order of im2col;
    outside its image a crop reads 0.  `total_patches` is patch_offsets[N], which the caller has on the host."""
    lib = _lib.load()
    if not (images_u8.is_cuda and images_u8.dtype == torch.uint8 and images_u8.is_contiguous() and images_u8.dim() == 4
            and images_u8.shape[3] == 3):
        raise ValueError("patches_from_boxes_u8: images must be a contiguous uint8 CUDA tensor [B,H,W,3]")
    B, Hmax, Wmax, _ = images_u8.shape
    N = boxes.shape[0]
    if N < 1 or total_patches < N or patch < 1:
        raise ValueError(f"patches_from_boxes_u8: {N} boxes, {total_patches} patch rows, patch {patch}")
    _i32(dims, "dims", (B, 2)), _i32(boxes, "boxes", (N, 5)), _i32(patch_offsets, "patch_offsets", (N + 1,))
    cols = torch.empty((total_patches, 3 * patch * patch), dtype=torch.float32, device=images_u8.device)
    _lib.check(lib.dclip_patches_from_boxes_u8(images_u8.data_ptr(), dims.data_ptr(), boxes.data_ptr(), patch_offsets.data_ptr(),
                                               cols.data_ptr(), B, Hmax, Wmax, N, patch, _stream()), "patches_from_boxes_u8")
    return cols


def vision_assemble_varlen(patch_emb, cls, pos, grids: torch.Tensor, cu_seqlens: torch.Tensor, g: int) -> torch.Tensor:
    """Token rows [T, D] of N crops: per crop the class row and its patch rows plus the position table resampled to the crop's
    grid (grids [N,2] = (gh,gw)); bit-equal per crop to vision_assemble_fwd over pos_interp_fwd.  T = patch rows + N."""
    lib = _lib.load()
    _f32(patch_emb, "patch_emb"), _f32(cls, "class_embedding"), _f32(pos, "position_embedding")
    N = grids.shape[0]
    if patch_emb.dim() != 2 or N < 1 or patch_emb.shape[0] < N:
        raise ValueError(f"vision_assemble_varlen: {N} crops, patch_emb {tuple(patch_emb.shape)}")
    D = patch_emb.shape[1]
    if D % 4 or cls.numel() != D or tuple(pos.shape) != (1 + g * g, D):
        raise ValueError(f"vision_assemble_varlen: D {D} (% 4 == 0), class_embedding {cls.numel()}, position table "
                         f"{tuple(pos.shape)} for g = {g}")
    _i32(grids, "grids", (N, 2)), _i32(cu_seqlens, "cu_seqlens", (N + 1,))
    x = torch.empty((patch_emb.shape[0] + N, D), dtype=torch.float32, device=patch_emb.device)
    _lib.check(lib.dclip_vision_assemble_varlen(patch_emb.data_ptr(), cls.data_ptr(), pos.data_ptr(), grids.data_ptr(),
                                                cu_seqlens.data_ptr(), x.data_ptr(), g, N, D, _stream()), "vision_assemble_varlen")
    return x


def attention_varlen_fwd(qkv: torch.Tensor, cu_seqlens: torch.Tensor, max_S: int, H: int, cls_only: bool = False,
                         want_lse: bool = False):
    """Non-causal self-attention inside each of the N packed sequences of qkv [T, 3*H*64] (rows cu_seqlens[n] ..
    cu_seqlens[n+1]-1; T = cu_seqlens[N]): out [T, H*64], or with `cls_only` row 0 of each sequence, [N, H*64].  `max_S` bounds
    the lengths.  Returns out, or (out, lse [H, T] / [H, N]) with `want_lse`."""
    lib = _lib.load()
    _f32(qkv, "qkv")
    N = cu_seqlens.numel() - 1
    if qkv.dim() != 2 or qkv.shape[1] != 3 * H * 64 or N < 1 or H < 1 or max_S < 1 or qkv.shape[0] < N:
        raise ValueError(f"attention_varlen_fwd: qkv {tuple(qkv.shape)}, H {H}, {N} sequences, max_S {max_S}")
    _i32(cu_seqlens, "cu_seqlens", (N + 1,))
    rows = N if cls_only else qkv.shape[0]
    out = torch.empty((rows, H * 64), dtype=torch.float32, device=qkv.device)
    lse = torch.empty((H, rows), dtype=torch.float32, device=qkv.device) if want_lse else None
    _lib.check(lib.dclip_attention_varlen_fwd(qkv.data_ptr(), cu_seqlens.data_ptr(), out.data_ptr(), _ptr(lse), N, max_S, H,
                                              int(bool(cls_only)), _stream()), "attention_varlen_fwd")
    return (out, lse) if want_lse else out


def gather_rows_at(x: torch.Tensor, rows: torch.Tensor) -> torch.Tensor:
    """out[n] = x[rows[n]]: x [T, D], rows [N] int32 in [0, T), any order."""
    lib = _lib.load()
    _f32(x, "x")
    N = rows.numel()
    if x.dim() != 2 or x.shape[1] % 4 or N < 1 or x.shape[0] < 1:
        raise ValueError(f"gather_rows_at: x {tuple(x.shape)} (D % 4 == 0), {N} rows")
    _i32(rows, "rows", (N,))
    out = torch.empty((N, x.shape[1]), dtype=torch.float32, device=x.device)
    _lib.check(lib.dclip_gather_rows_at(x.data_ptr(), rows.data_ptr(), out.data_ptr(), N, x.shape[0], x.shape[1], _stream()),
               "gather_rows_at")
    return out


# ------------------------------------------------------------------------------------------- packed captions (text tower)

def text_embed_varlen(ids, cu_seqlens: torch.Tensor, tok, pos, total_rows: int) -> torch.Tensor:
    """Token rows [Tp, D] of N captions cut after their first EOS and laid back to back: row cu_seqlens[n] + t =
    tok[ids[n, t]] + pos[t] for t < cu_seqlens[n+1] - cu_seqlens[n].  ids [N, T] is the padded id matrix (the pads are never
    read); `total_rows` is Tp = cu_seqlens[N], which the caller has on the host."""
    lib = _lib.load()
    _ids(ids), _f32(tok, "token_embedding"), _f32(pos, "position_embedding")
    N, T = ids.shape
    vocab, D = tok.shape
    if pos.shape[0] < T or pos.shape[1] != D:
        raise ValueError(f"text_embed_varlen: sequence {T} longer than position table {tuple(pos.shape)}")
    if N < 1 or D % 4 or not (N <= total_rows <= N * T):
        raise ValueError(f"text_embed_varlen: {N} captions of up to {T} ids, {total_rows} packed rows, D {D} (% 4 == 0)")
    _i32(cu_seqlens, "cu_seqlens", (N + 1,))
    x = torch.empty((total_rows, D), dtype=torch.float32, device=tok.device)
    _lib.check(lib.dclip_text_embed_varlen(ids.data_ptr(), cu_seqlens.data_ptr(), tok.data_ptr(), pos.data_ptr(), x.data_ptr(),
                                           N, T, D, vocab, _stream()), "text_embed_varlen")
    return x


def attention_varlen_causal_fwd(qkv: torch.Tensor, cu_seqlens: torch.Tensor, max_S: int, H: int, last_only: bool = False,
                                want_lse: bool = False):
    """Causal self-attention inside each of the N packed sequences of qkv [Tp, 3*H*64] (rows cu_seqlens[n] ..
    cu_seqlens[n+1]-1; Tp = cu_seqlens[N]): out [Tp, H*64], or with `last_only` the LAST row of each sequence (which sees all
    of it), [N, H*64].  `max_S` bounds the lengths.  Returns out, or (out, lse [H, Tp] / [H, N]) with `want_lse`."""
    lib = _lib.load()
    _f32(qkv, "qkv")
    N = cu_seqlens.numel() - 1
    if qkv.dim() != 2 or qkv.shape[1] != 3 * H * 64 or N < 1 or H < 1 or max_S < 1 or qkv.shape[0] < N:
        raise ValueError(f"attention_varlen_causal_fwd: qkv {tuple(qkv.shape)}, H {H}, {N} sequences, max_S {max_S}")
    _i32(cu_seqlens, "cu_seqlens", (N + 1,))
    rows = N if last_only else qkv.shape[0]
    out = torch.empty((rows, H * 64), dtype=torch.float32, device=qkv.device)
    lse = torch.empty((H, rows), dtype=torch.float32, device=qkv.device) if want_lse else None
    _lib.check(lib.dclip_attention_varlen_causal_fwd(qkv.data_ptr(), cu_seqlens.data_ptr(), out.data_ptr(), _ptr(lse), N, max_S,
                                                     H, int(bool(last_only)), _stream()), "attention_varlen_causal_fwd")
    return (out, lse) if want_lse else out


def attention_varlen_causal_bwd(qkv: torch.Tensor, cu_seqlens: torch.Tensor, out: torch.Tensor, dout: torch.Tensor,
                                lse: torch.Tensor, max_S: int, H: int) -> torch.Tensor:
    """Backward of attention_varlen_causal_fwd over every row: qkv [Tp, 3*H*64], out / dout [Tp, H*64], lse
    [H, Tp] as that call returned it with `want_lse`; returns dqkv [Tp, 3*H*64], every word written.  `max_S` bounds the
    lengths.  The delta scratch [H, Tp] comes from the current workspace lane."""
    lib = _lib.load()
    _f32(qkv, "qkv"), _f32(out, "out"), _f32(dout, "dout"), _f32(lse, "lse")
    N = cu_seqlens.numel() - 1
    if qkv.dim() != 2 or qkv.shape[1] != 3 * H * 64 or N < 1 or H < 1 or max_S < 1 or qkv.shape[0] < N:
        raise ValueError(f"attention_varlen_causal_bwd: qkv {tuple(qkv.shape)}, H {H}, {N} sequences, max_S {max_S}")
    Tp = qkv.shape[0]
    if tuple(out.shape) != (Tp, H * 64) or tuple(dout.shape) != (Tp, H * 64) or tuple(lse.shape) != (H, Tp):
        raise ValueError(f"attention_varlen_causal_bwd: out {tuple(out.shape)} / dout {tuple(dout.shape)} must be "
                         f"{(Tp, H * 64)}, lse {tuple(lse.shape)} must be {(H, Tp)}")
    _i32(cu_seqlens, "cu_seqlens", (N + 1,))
    dqkv = torch.empty_like(qkv)
    delta = _ws.get(H * Tp * 4, qkv.device)
    _lib.check(lib.dclip_attention_varlen_causal_bwd(qkv.data_ptr(), cu_seqlens.data_ptr(), out.data_ptr(), dout.data_ptr(),
                                                     lse.data_ptr(), dqkv.data_ptr(), delta.data_ptr(), N, max_S, H, _stream()),
               "attention_varlen_causal_bwd")
    return dqkv


def text_embed_varlen_bwd(ids, cu_seqlens: torch.Tensor, dx: torch.Tensor, dtok: Optional[torch.Tensor] = None,
                          dpos: Optional[torch.Tensor] = None):
    """Backward of text_embed_varlen: dx [Tp, D] packed as there.  dtok [vocab, D] is ACCUMULATED into (float
    atomics; the caller zeroes it); dpos [P >= T, D] gets rows 0 .. T-1 WRITTEN (a sum in ascending caption order, zeros where
    no caption reaches), rows beyond T untouched.  Either may be None, not both.  Returns (dtok, dpos)."""
    lib = _lib.load()
    _ids(ids), _f32(dx, "dx")
    N, T = ids.shape
    if dtok is None and dpos is None:
        raise ValueError("text_embed_varlen_bwd: neither dtok nor dpos asked for")
    if dx.dim() != 2 or dx.shape[1] % 4 or N < 1 or not (N <= dx.shape[0] <= N * T):
        raise ValueError(f"text_embed_varlen_bwd: {N} captions of up to {T} ids, dx {tuple(dx.shape)} (D % 4 == 0)")
    D = dx.shape[1]
    vocab = 1
    if dtok is not None:
        _f32(dtok, "dtok")
        if dtok.dim() != 2 or dtok.shape[1] != D:
            raise ValueError(f"text_embed_varlen_bwd: dtok {tuple(dtok.shape)} for D {D}")
        vocab = dtok.shape[0]
    if dpos is not None:
        _f32(dpos, "dpos")
        if dpos.dim() != 2 or dpos.shape[1] != D or dpos.shape[0] < T:
            raise ValueError(f"text_embed_varlen_bwd: dpos {tuple(dpos.shape)} for {T} positions, D {D}")
    _i32(cu_seqlens, "cu_seqlens", (N + 1,))
    _lib.check(lib.dclip_text_embed_varlen_bwd(ids.data_ptr(), cu_seqlens.data_ptr(), dx.data_ptr(), _ptr(dtok), _ptr(dpos), N, T,
                                               D, vocab, _stream()), "text_embed_varlen_bwd")
    return dtok, dpos


def scatter_last_rows(dout: torch.Tensor, cu_seqlens: torch.Tensor, total_rows: int) -> torch.Tensor:
    """The transpose of gather_rows_at(x, cu_seqlens[1:] - 1): dx [Tp, D] with row cu_seqlens[n+1] - 1 = dout[n] and zeros
    elsewhere, the whole tensor written.  `total_rows` is Tp = cu_seqlens[N], which the caller has on the host."""
    lib = _lib.load()
    _f32(dout, "dout")
    if dout.dim() != 2 or dout.shape[1] % 4 or dout.shape[0] < 1 or total_rows < dout.shape[0]:
        raise ValueError(f"scatter_last_rows: dout {tuple(dout.shape)} (D % 4 == 0), {total_rows} packed rows")
    N, D = dout.shape
    _i32(cu_seqlens, "cu_seqlens", (N + 1,))
    dx = torch.empty((total_rows, D), dtype=torch.float32, device=dout.device)
    _lib.check(lib.dclip_scatter_last_rows(dout.data_ptr(), cu_seqlens.data_ptr(), dx.data_ptr(), N, D, _stream()),
               "scatter_last_rows")
    return dx


def attention_varlen_fwd_f16x2(qkv: torch.Tensor, cu_seqlens: torch.Tensor, max_S: int, H: int, causal: bool = False,
                               scale: float = 1.0, pieces: int = 2, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """attention_varlen_fwd (`causal` False) / attention_varlen_causal_fwd (True) over every row, with the context written as
    the split operand of the next GEMM: fp16 [T, pieces*H*64] of scale * context, bit-equal to the fp32 entry
    followed by split_f16x3(.., scale, pieces=pieces).  `out`: see _split_ctx_out."""
    lib = _lib.load()
    _f32(qkv, "qkv")
    N = cu_seqlens.numel() - 1
    if qkv.dim() != 2 or qkv.shape[1] != 3 * H * 64 or N < 1 or H < 1 or max_S < 1 or qkv.shape[0] < N:
        raise ValueError(f"attention_varlen_fwd_f16x2: qkv {tuple(qkv.shape)}, H {H}, {N} sequences, max_S {max_S}")
    _i32(cu_seqlens, "cu_seqlens", (N + 1,))
    y = _split_ctx_out("attention_varlen_fwd_f16x2", qkv.shape[0], H * 64, pieces, out, qkv.device)
    _lib.check(lib.dclip_attention_varlen_fwd_f16x2(qkv.data_ptr(), cu_seqlens.data_ptr(), y.data_ptr(), N, max_S, H,
                                                    int(bool(causal)), float(scale), int(pieces), y.shape[1], _stream()),
               "attention_varlen_fwd_f16x2")
    return y


def pack_tokens_varlen(tokens, sentence, cu_seqlens: torch.Tensor, Tmax: int) -> torch.Tensor:
    """pack_tokens on packed token rows: tokens [Tp, P], sentence [N, P] -> [N, Tmax, P]; caption b's word tokens are rows
    cu_seqlens[b] + 1 .. cu_seqlens[b+1] - 2, zero beyond; a caption without word tokens gives its sentence row in slot 0."""
    lib = _lib.load()
    _f32(tokens, "tokens"), _f32(sentence, "sentence")
    N = cu_seqlens.numel() - 1
    if tokens.dim() != 2 or N < 1 or tuple(sentence.shape) != (N, tokens.shape[1]) or tokens.shape[1] % 4 or Tmax < 1 \
            or tokens.shape[0] < N:
        raise ValueError(f"pack_tokens_varlen: tokens {tuple(tokens.shape)}, sentence {tuple(sentence.shape)}, {N} captions, "
                         f"Tmax {Tmax}")
    _i32(cu_seqlens, "cu_seqlens", (N + 1,))
    Pd = tokens.shape[1]
    out = torch.empty((N, Tmax, Pd), dtype=torch.float32, device=tokens.device)
    _lib.check(lib.dclip_pack_tokens_varlen(tokens.data_ptr(), sentence.data_ptr(), cu_seqlens.data_ptr(), out.data_ptr(), N, Tmax,
                                            Pd, _stream()), "pack_tokens_varlen")
    return out


# ------------------------------------------------------------------------------------------- 16-bit packed attention core

def _attention_varlen16(name: str, dtype, check, qkv, cu_seqlens, max_S: int, H: int, flag: bool, one_row: bool) -> torch.Tensor:
    lib = _lib.load()
    check(qkv, "qkv")
    N = cu_seqlens.numel() - 1
    if qkv.dim() != 2 or qkv.shape[1] != 3 * H * 64 or N < 1 or H < 1 or max_S < 1 or qkv.shape[0] < N:
        raise ValueError(f"{name}: qkv {tuple(qkv.shape)}, H {H}, {N} sequences, max_S {max_S}")
    if one_row and max_S > 512:
        raise ValueError(f"{name}: max_S {max_S} > 512")
    _i32(cu_seqlens, "cu_seqlens", (N + 1,))
    out = torch.empty((N if one_row else qkv.shape[0], H * 64), dtype=dtype, device=qkv.device)
    _lib.check(getattr(lib, "dclip_" + name)(qkv.data_ptr(), cu_seqlens.data_ptr(), out.data_ptr(), N, max_S, H, int(bool(flag)),
                                             _stream()), name)
    return out


def attention_varlen_fwd_bf16(qkv: torch.Tensor, cu_seqlens: torch.Tensor, max_S: int, H: int, causal: bool = False) -> torch.Tensor:
    """Self-attention inside each of the N packed sequences of a bf16 qkv [T, 3*H*64] (rows cu_seqlens[n] .. cu_seqlens[n+1]-1;
    T = cu_seqlens[N]) on the bf16 MFMAs: context [T, H*64] bf16.  `causal`: query i sees keys 0..i of its sequence.  `max_S`
    bounds the lengths."""
    return _attention_varlen16("attention_varlen_fwd_bf16", torch.bfloat16, _bf16, qkv, cu_seqlens, max_S, H, causal, False)


def attention_varlen_fwd_f16(qkv: torch.Tensor, cu_seqlens: torch.Tensor, max_S: int, H: int, causal: bool = False) -> torch.Tensor:
    """attention_varlen_fwd_bf16 on an fp16 qkv: [T, H*64] fp16."""
    return _attention_varlen16("attention_varlen_fwd_f16", torch.float16, _f16, qkv, cu_seqlens, max_S, H, causal, False)


def attention_varlen_row_fwd_bf16(qkv: torch.Tensor, cu_seqlens: torch.Tensor, max_S: int, H: int, last: bool = False) -> torch.Tensor:
    """One attention output row per packed sequence from a bf16 qkv [T, 3*H*64]: row 0 of each sequence (the CLS row), or with
    `last` its last row (the first EOS of a packed caption), against all keys of that sequence.  [N, H*64] bf16; max_S <= 512."""
    return _attention_varlen16("attention_varlen_row_fwd_bf16", torch.bfloat16, _bf16, qkv, cu_seqlens, max_S, H, last, True)


def attention_varlen_row_fwd_f16(qkv: torch.Tensor, cu_seqlens: torch.Tensor, max_S: int, H: int, last: bool = False) -> torch.Tensor:
    """attention_varlen_row_fwd_bf16 on an fp16 qkv: [N, H*64] fp16."""
    return _attention_varlen16("attention_varlen_row_fwd_f16", torch.float16, _f16, qkv, cu_seqlens, max_S, H, last, True)


# ------------------------------------------------------------------------------------------- evaluation

def rowdot_gather(a, b, idx=None):
    lib = _lib.load()
    _f32(a, "a"), _f32(b, "b")
    Bq, Pd = a.shape
    Bk = b.shape[0]
    if b.shape[1] != Pd:
        raise ValueError("rowdot_gather: width mismatch")
    if idx is not None:
        _idx(idx, Bq)
    elif Bk < Bq:
        raise ValueError("rowdot_gather: idx=None needs Bk >= Bq")
    out = torch.empty((Bq,), dtype=torch.float32, device=a.device)
    _lib.check(lib.dclip_rowdot_gather(a.data_ptr(), b.data_ptr(), _ptr(idx), out.data_ptr(), Bq, Bk, Pd, _stream()),
               "rowdot_gather")
    return out


def rank_count(queries, candidates, thresh, gt=None):
    """count[i] = #{j != gt[i] : <queries_i, candidates_j> > thresh[i]}  (int32; gt=None means j != i)."""
    lib = _lib.load()
    _f32(queries, "queries"), _f32(candidates, "candidates"), _f32(thresh, "thresh")
    Bq, Pd = queries.shape
    Bk = candidates.shape[0]
    if candidates.shape[1] != Pd or thresh.numel() != Bq:
        raise ValueError("rank_count: shape mismatch")
    if gt is not None:
        _idx(gt, Bq)
    count = torch.empty((Bq,), dtype=torch.int32, device=queries.device)
    nbytes = lib.dclip_rank_count_workspace(Bq, Bk)
    ws = _ws.get(nbytes, queries.device)
    _lib.check(lib.dclip_rank_count(queries.data_ptr(), candidates.data_ptr(), thresh.data_ptr(), _ptr(gt),
                                    count.data_ptr(), Bq, Bk, Pd, _ptr(ws), nbytes, _stream()), "rank_count")
    return count


def topk_ip(queries, database, k: int):
    """(scores [Q,k] fp32, indices [Q,k] int32): the k best database rows per query by fp32 inner product, ordered by
    (score descending, index ascending); (-inf, -1) where fewer than k rows qualify.  See include/dclip_hip.h."""
    lib = _lib.load()
    _f32(queries, "queries"), _f32(database, "database")
    if queries.dim() != 2 or database.dim() != 2 or database.shape[1] != queries.shape[1]:
        raise ValueError("topk_ip: expected queries [Q,P] and database [N,P]")
    if database.device != queries.device:
        raise ValueError("topk_ip: operands on different devices")
    Q, Pd = queries.shape
    N = database.shape[0]
    k = int(k)
    scores = torch.empty((Q, k), dtype=torch.float32, device=queries.device)
    indices = torch.empty((Q, k), dtype=torch.int32, device=queries.device)
    nbytes = lib.dclip_topk_ip_workspace(Q, N, k)
    ws = _ws.get(nbytes, queries.device)
    _lib.check(lib.dclip_topk_ip(queries.data_ptr(), database.data_ptr(), scores.data_ptr(), indices.data_ptr(), Q, N, Pd, k,
                                 _ptr(ws), nbytes, _stream()), "topk_ip")
    return scores, indices


def relu_(x):
    """x = max(x, 0) in place (NaN stays NaN)."""
    lib = _lib.load()
    _f32(x, "x")
    _lib.check(lib.dclip_relu_f32(x.data_ptr(), x.numel(), _stream()), "relu_f32")
    return x


def knn_select(sim, idx, database, fallback, thresh: float):
    """(out [Q,P], source [Q] int32): database row idx[i] where idx[i] >= 0 and sim[i] >= thresh (source 0), else
    fallback row i (source 1).  Decided on the device."""
    lib = _lib.load()
    _f32(sim, "sim"), _f32(database, "database"), _f32(fallback, "fallback")
    if fallback.dim() != 2 or database.dim() != 2 or database.shape[1] != fallback.shape[1]:
        raise ValueError("knn_select: expected database [N,P] and fallback [Q,P]")
    Q, Pd = fallback.shape
    if sim.numel() != Q:
        raise ValueError("knn_select: sim size")
    if database.device != fallback.device or sim.device != fallback.device:
        raise ValueError("knn_select: operands on different devices")
    _idx(idx, Q)
    out = torch.empty_like(fallback)
    source = torch.empty((Q,), dtype=torch.int32, device=fallback.device)
    _lib.check(lib.dclip_knn_select(sim.data_ptr(), idx.data_ptr(), database.data_ptr(), fallback.data_ptr(), float(thresh),
                                    out.data_ptr(), source.data_ptr(), Q, database.shape[0], Pd, _stream()), "knn_select")
    return out, source


def axpby(x, y, a: float, b: float):
    """y = a*x + b*y (in place on y)."""
    lib = _lib.load()
    _f32(x, "x"), _f32(y, "y")
    if x.numel() != y.numel():
        raise ValueError("axpby: size mismatch")
    _lib.check(lib.dclip_axpby(x.data_ptr(), y.data_ptr(), float(a), float(b), x.numel(), _stream()), "axpby")
    return y
