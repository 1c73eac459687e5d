"""ctypes binding of libdclip_hip.so (the C ABI in include/dclip_hip.h).

The library is built in-tree by `make` / `__graft_entry__.build()`; there is NO fallback: if
it is missing or a symbol is absent, importing the product path fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# DCLIP_LIB_PATH: another BUILD of this library (same-box A/B runs of bench.py, tools/ab/*.so); never a fallback
LIB_PATH = os.environ.get("DCLIP_LIB_PATH") or os.path.join(_HERE, "libdclip_hip.so")

P = C.c_void_p          # device pointers and the stream
I = C.c_int
F = C.c_float
Z = C.c_size_t
L = C.c_int64

# name -> (restype, argtypes); mirrors include/dclip_hip.h declaration by declaration
SIGNATURES = {
    "dclip_abi_version": (I, []),
    "dclip_last_error": (C.c_char_p, []),
    "dclip_last_launch": (C.c_char_p, []),
    "dclip_first_launch": (C.c_char_p, []),
    "dclip_gemm_f32_workspace": (Z, [I, I, I, I, I]),
    "dclip_gemm_f32_plan": (I, [I, I, I, I, I, C.POINTER(C.c_int)]),
    "dclip_gemm_f32": (I, [P, P, P, P, P, P, I, I, I, I, I, I, I, I, F, I, P, Z, P]),
    "dclip_colsum_f32_workspace": (Z, [I, I]),
    "dclip_colsum_f32": (I, [P, P, I, I, I, I, P, Z, P]),
    "dclip_layernorm_fwd": (I, [P, P, P, P, P, P, I, I, F, P]),
    "dclip_layernorm_bwd_workspace": (Z, [I, I]),
    "dclip_layernorm_bwd": (I, [P, P, P, P, P, P, P, P, P, I, I, I, P, Z, P]),
    "dclip_layernorm_bwd_ex": (I, [P, P, P, P, P, P, P, P, P, P, P, I, I, I, P, Z, P]),
    "dclip_attention_fwd": (I, [P, P, P, I, I, I, I, P]),
    "dclip_attention_bwd": (I, [P, P, P, P, P, P, I, I, I, I, P]),
    "dclip_attention_bwd_workspace": (Z, [I, I, I, I]),
    "dclip_attention_bwd_ws": (I, [P, P, P, P, P, P, Z, I, I, I, I, P]),
    "dclip_attention_cls_fwd": (I, [P, P, P, I, I, I, P]),
    "dclip_attention_cls_bwd": (I, [P, P, P, P, P, P, I, I, I, P]),
    "dclip_attention_row_fwd": (I, [P, P, P, P, I, I, I, P]),
    "dclip_attention_row_fwd_bf16": (I, [P, P, P, I, I, I, P]),
    "dclip_im2col_bf16": (I, [P, P, I, I, I, I, I, I, P]),
    "dclip_im2col": (I, [P, P, I, I, I, I, I, P]),
    "dclip_vision_assemble_fwd": (I, [P, P, P, P, I, I, I, P]),
    "dclip_vision_assemble_bwd": (I, [P, P, I, I, I, P]),
    "dclip_text_embed_fwd": (I, [P, P, P, P, I, I, I, I, P]),
    "dclip_text_embed_bwd": (I, [P, P, P, I, I, I, I, P]),
    "dclip_first_eos": (I, [P, P, I, I, L, P]),
    "dclip_gather_rows": (I, [P, P, P, I, I, I, P]),
    "dclip_scatter_rows": (I, [P, P, P, I, I, I, P]),
    "dclip_pos_interp_fwd": (I, [P, P, I, I, I, I, P]),
    "dclip_pos_interp_bwd": (I, [P, P, I, I, I, I, I, P]),
    "dclip_im2col_rect": (I, [P, P, I, I, I, I, I, P]),
    "dclip_im2col_rect_bf16": (I, [P, P, I, I, I, I, I, I, P]),
    "dclip_im2col_rect_f16": (I, [P, P, I, I, I, I, I, I, P]),
    "dclip_patches_from_boxes_u8": (I, [P, P, P, P, P, I, I, I, I, I, P]),
    "dclip_vision_assemble_varlen": (I, [P, P, P, P, P, P, I, I, I, P]),
    "dclip_attention_varlen_fwd": (I, [P, P, P, P, I, I, I, I, P]),
    "dclip_gather_rows_at": (I, [P, P, P, I, I, I, P]),
    "dclip_text_embed_varlen": (I, [P, P, P, P, P, I, I, I, I, P]),
    "dclip_attention_varlen_causal_fwd": (I, [P, P, P, P, I, I, I, I, P]),
    "dclip_pack_tokens_varlen": (I, [P, P, P, P, I, I, I, P]),
    "dclip_attention_varlen_causal_bwd": (I, [P, P, P, P, P, P, P, I, I, I, P]),
    "dclip_text_embed_varlen_bwd": (I, [P, P, P, P, P, I, I, I, I, P]),
    "dclip_scatter_last_rows": (I, [P, P, P, I, I, P]),
    "dclip_attention_varlen_fwd_bf16": (I, [P, P, P, I, I, I, I, P]),
    "dclip_attention_varlen_fwd_f16": (I, [P, P, P, I, I, I, I, P]),
    "dclip_attention_varlen_row_fwd_bf16": (I, [P, P, P, I, I, I, I, P]),
    "dclip_attention_varlen_row_fwd_f16": (I, [P, P, P, I, I, I, I, P]),
    "dclip_normalize_rows_fwd": (I, [P, P, P, I, I, F, P]),
    "dclip_normalize_rows_bwd": (I, [P, P, P, P, I, I, F, I, P]),
    "dclip_contrastive_workspace": (Z, [I, I, I]),
    "dclip_contrastive_lse": (I, [P, P, P, P, I, I, I, I, F, P, Z, P]),
    "dclip_contrastive_grad": (I, [P, P, P, P, P, I, I, I, I, F, F, P, Z, P]),
    "dclip_cosine_loss_fwd": (I, [P, P, P, P, I, I, P]),
    "dclip_cosine_loss_bwd": (I, [P, P, P, P, I, I, F, I, P]),
    "dclip_sub_reduce": (I, [P, P, P, I, F, I, P]),
    "dclip_cross_attention_fwd": (I, [P, P, P, P, I, I, I, I, P]),
    "dclip_cross_attention_bwd": (I, [P, P, P, P, P, P, P, P, I, I, I, I, P]),
    "dclip_aggregation_fwd": (I, [P, P, P, I, I, I, F, F, I, P]),
    "dclip_aggregation_bwd": (I, [P, P, P, P, I, I, I, F, F, P]),
    "dclip_pack_tokens": (I, [P, P, P, P, I, I, I, I, P]),
    "dclip_sanitize_groups": (I, [P, P, I, I, I, I, P]),
    "dclip_mask_rows": (I, [P, P, I, I, I, P]),
    "dclip_rank_count_workspace": (Z, [I, I]),
    "dclip_rowdot_gather": (I, [P, P, P, P, I, I, I, P]),
    "dclip_rank_count": (I, [P, P, P, P, P, I, I, I, P, Z, P]),
    "dclip_topk_ip_workspace": (Z, [I, I, I]),
    "dclip_topk_ip": (I, [P, P, P, P, I, I, I, I, P, Z, P]),
    "dclip_relu_f32": (I, [P, Z, P]),
    "dclip_knn_select": (I, [P, P, P, P, F, P, P, I, I, I, P]),
    "dclip_crop_resize_workspace": (Z, [I, I, I, I]),
    "dclip_crop_resize_u8": (I, [P, P, P, P, I, I, I, I, I, I, I, P, Z, P]),
    "dclip_clip_preprocess_workspace": (Z, [I, I, I, I]),
    "dclip_clip_preprocess_u8": (I, [P, P, P, I, I, I, I, P, P, P, Z, P]),
    "dclip_gemm_bf16": (I, [P, P, P, P, P, I, I, I, I, I, I, I, I, P]),
    "dclip_attention_fwd_bf16": (I, [P, P, I, I, I, I, P]),
    "dclip_attention_fwd_bf16_lse": (I, [P, P, P, I, I, I, I, P]),
    "dclip_attention_bwd_bf16": (I, [P, P, P, P, P, I, I, I, I, P]),
    "dclip_cast_f32_bf16": (I, [P, P, I, I, I, I, P]),
    "dclip_layernorm_fwd_bf16": (I, [P, P, P, P, I, I, F, P]),
    "dclip_gemm_bf16_ex": (I, [P, P, P, P, P, P, I, I, I, I, I, I, I, I, P]),
    "dclip_layernorm_fwd_bf16_stats": (I, [P, P, P, P, P, P, I, I, F, P]),
    "dclip_transpose_to_bf16": (I, [P, I, P, P, I, I, I, I, I, P]),
    "dclip_attention_fwd_io16": (I, [P, P, P, I, I, I, I, P]),
    "dclip_attention_bwd_io16": (I, [P, P, P, P, P, I, I, I, I, P]),
    "dclip_mt_weights_record_bytes": (I, []),
    "dclip_mt_weights_bf16": (I, [P, I, I, P]),
    "dclip_rowsum_bf16": (I, [P, P, I, I, I, P]),
    "dclip_gemm_bf16_splitk_plan": (I, [I, I, I]),
    "dclip_gemm_bf16_splitk_workspace": (Z, [I, I, I]),
    "dclip_gemm_bf16_splitk": (I, [P, P, P, I, I, I, I, I, I, I, P, Z, P]),
    "dclip_gemm_bf16_wgrad_tokmajor_plan": (I, [I, I, I]),
    "dclip_gemm_bf16_wgrad_tokmajor": (I, [P, P, P, I, I, I, I, I, I, I, P, Z, P]),
    "dclip_colsum_bf16": (I, [P, P, I, I, I, I, P, Z, P]),
    "dclip_sumsq_blocks": (I, [Z]),
    "dclip_sumsq_f32": (I, [P, Z, P, P]),
    "dclip_clip_coef": (I, [P, I, F, P, P, P]),
    "dclip_adamw_f32": (I, [P, P, P, P, Z, F, F, F, F, F, I, P, P]),
    "dclip_mt_record_bytes": (I, []),
    "dclip_mt_chunk_elems": (I, []),
    "dclip_mt_sumsq_f32": (I, [P, I, I, P, P]),
    "dclip_mt_adamw_f32": (I, [P, I, I, F, F, F, F, F, P, P]),
    "dclip_mt_adam_f32": (I, [P, I, I, F, F, F, F, F, P, P]),
    "dclip_axpby": (I, [P, P, F, F, Z, P]),
    "dclip_fill": (I, [P, F, Z, P]),
    "dclip_gemm_f16": (I, [P, P, P, P, P, I, I, I, I, I, I, I, I, P]),
    "dclip_cast_f32_f16": (I, [P, P, I, I, I, I, P]),
    "dclip_layernorm_fwd_f16": (I, [P, P, P, P, I, I, F, P]),
    "dclip_im2col_f16": (I, [P, P, I, I, I, I, I, I, P]),
    "dclip_attention_fwd_f16": (I, [P, P, I, I, I, I, P]),
    "dclip_attention_row_fwd_f16": (I, [P, P, P, I, I, I, P]),
    "dclip_split_f32_f16x3": (I, [P, P, I, I, I, I, F, I, P]),
    "dclip_layernorm_fwd_f16x3": (I, [P, P, P, P, I, I, F, F, P]),
    "dclip_gemm_f16_scaled": (I, [P, P, P, P, P, I, I, I, I, I, I, I, I, F, P]),
    "dclip_gemm_f16_scaled_split": (I, [P, P, P, P, I, I, I, I, I, I, I, F, F, P]),
    "dclip_split_f32_f16x3_dev": (I, [P, P, I, I, I, I, P, I, P]),
    "dclip_layernorm_fwd_f16x3_dev": (I, [P, P, P, P, P, P, P, I, I, F, P, P]),
    "dclip_gemm_f16_scaled_dev": (I, [P, P, P, P, P, I, I, I, I, I, I, I, I, P, P]),
    "dclip_gemm_f16_scaled_split_dev": (I, [P, P, P, P, P, P, I, I, I, I, I, I, I, P, P, P]),
    "dclip_split16_record_bytes": (I, []),
    "dclip_split16_plan_floats": (I, []),
    "dclip_split16_tile_rows": (I, []),
    "dclip_split16_stats": (I, [P, I, I, P, P]),
    "dclip_split16_plan": (I, [P, P, I, I, P]),
    "dclip_split16_weights": (I, [P, I, I, P, P]),
    "dclip_split_f32_f16x3_rows": (I, [P, P, P, I, I, I, P]),
    "dclip_split16_weights_t": (I, [P, I, I, P, P, P]),
    "dclip_gemm_f16_scaled_rows_dev": (I, [P, P, P, P, I, I, I, I, I, I, I, P, P, P]),
    "dclip_split_f32_f16x3_rows_colstats_workspace": (Z, [I, I]),
    "dclip_split_f32_f16x3_rows_colstats": (I, [P, P, P, P, P, P, P, I, I, I, P, Z, P]),
    "dclip_split_f32_f16x3_rows_cols_stats": (I, [P, P, P, P, P, P, P, P, P, I, I, I, I, P]),
    "dclip_gemm_f16_scaled_rows_stats_plan": (I, [I, I, I]),
    "dclip_gemm_f16_scaled_rows_stats_dev": (I, [P, P, P, P, I, I, I, I, I, I, I, P, P, P, P, P]),
    "dclip_attention_bwd_stats_plan": (I, [I, I, I]),
    "dclip_attention_bwd_stats": (I, [P, P, P, P, P, P, P, I, I, I, I, P]),
    "dclip_colsum_segments_f32_workspace": (Z, [I, I]),
    "dclip_colsum_segments_f32": (I, [P, P, I, I, I, I, P, Z, P]),
    "dclip_attention_bwd_rows_stats_plan": (I, [I, I, I]),
    "dclip_attention_bwd_rows_stats": (I, [P, P, P, P, P, P, P, I, I, I, I, P]),
    "dclip_layernorm_bwd_stats_plan": (I, [I, I]),
    "dclip_layernorm_bwd_stats": (I, [P, P, P, P, P, P, P, P, P, P, P, I, I, I, P, Z, P]),
    "dclip_gemm_f16x3_plan": (I, [I, I, I]),
    "dclip_gemm_f16x3_tile_rows": (I, [I, I, I, I, I]),
    "dclip_gemm_f16x3_scaled": (I, [P, P, P, P, P, I, I, I, I, I, I, I, I, I, I, I, I, F, P]),
    "dclip_gemm_f16x3_scaled_split": (I, [P, P, P, P, I, I, I, I, I, I, I, I, I, I, I, F, F, P]),
    "dclip_gemm_f16x3_scaled_dev": (I, [P, P, P, P, P, I, I, I, I, I, I, I, I, I, I, I, I, P, P]),
    "dclip_gemm_f16x3_scaled_split_dev": (I, [P, P, P, P, P, P, I, I, I, I, I, I, I, I, I, I, I, P, P, P]),
    "dclip_gemm_f16x3_scaled_rows_dev": (I, [P, P, P, P, I, I, I, I, I, I, I, I, I, I, I, P, P, P]),
    "dclip_gemm_f16x3_scaled_rows_stats_plan": (I, [I, I, I]),
    "dclip_gemm_f16x3_scaled_rows_stats_dev": (I, [P, P, P, P, I, I, I, I, I, I, I, I, I, I, I, P, P, P, P, P]),
    "dclip_gemm_f16x3_wgrad_tokmajor_plan": (I, [I, I, I]),
    "dclip_gemm_f16x3_wgrad_tokmajor_workspace": (Z, [I, I, I]),
    "dclip_gemm_f16x3_wgrad_tokmajor": (I, [P, P, P, I, I, I, I, I, I, I, I, I, I, P, P, I, P, Z, P]),
    "dclip_split_f32_f16x2": (I, [P, P, I, I, I, I, F, P, P]),
    "dclip_attention_fwd_f16x2": (I, [P, P, I, I, I, I, F, I, I, P]),
    "dclip_attention_varlen_fwd_f16x2": (I, [P, P, P, I, I, I, I, F, I, I, P]),
    "dclip_quick_gelu_f32": (I, [P, P, Z, P]),
    "dclip_layernorm_fwd_f16x2": (I, [P, P, P, P, P, P, P, I, I, F, F, P, P]),
    "dclip_split_f32_f16x2_rows": (I, [P, P, P, I, I, I, P]),
    "dclip_split_f32_f16x2_rows_colstats": (I, [P, P, P, P, P, P, P, I, I, I, P, Z, P]),
    "dclip_split_f32_f16x2_rows_cols_stats": (I, [P, P, P, P, P, P, P, P, P, I, I, I, I, P]),
    "dclip_gemm_f16x3_scaled_split2": (I, [P, P, P, P, I, I, I, I, I, I, I, I, I, I, I, F, F, P]),
    "dclip_gemm_f16x3_scaled_split2_dev": (I, [P, P, P, P, P, P, I, I, I, I, I, I, I, I, I, I, I, P, P, P]),
    "dclip_im2col_f16x2": (I, [P, P, I, I, I, I, I, F, P, P]),
    "dclip_split16_front_rec_floats": (I, []),
    "dclip_split16_front_wrec_floats": (I, []),
    "dclip_split16_front_workspace": (Z, []),
    "dclip_split16_front": (I, [P, Z, P, I, I, P, P, P, P, Z, I, P]),
    "dclip_split_f32_f16x2_cols_workspace": (Z, [I, I]),
    "dclip_split_f32_f16x2_cols": (I, [P, P, P, P, I, I, I, P, Z, P]),
    "dclip_split16_patch_plan": (I, [I, I, I]),
    "dclip_gemm_f16_wgrad_tokmajor_seg3_plan": (I, [I, I, I]),
    "dclip_gemm_f16_wgrad_tokmajor_seg3": (I, [P, P, P, I, I, I, I, I, I, I, I, I, I, I, I, P, P, I, P, Z, P]),
    "dclip_gemm_f16_ex": (I, [P, P, P, P, P, P, I, I, I, I, I, I, I, I, P]),
    "dclip_gemm_f16_wgrad_tokmajor_plan": (I, [I, I, I]),
    "dclip_gemm_f16_wgrad_tokmajor": (I, [P, P, P, I, I, I, I, I, I, I, P, Z, P]),
    "dclip_gemm_f16_splitk_plan": (I, [I, I, I]),
    "dclip_gemm_f16_splitk_workspace": (Z, [I, I, I]),
    "dclip_gemm_f16_splitk": (I, [P, P, P, I, I, I, I, I, I, I, P, Z, P]),
    "dclip_cast_f32_f16_ieee": (I, [P, P, I, I, I, I, P]),
    "dclip_layernorm_fwd_f16_stats": (I, [P, P, P, P, P, P, I, I, F, P]),
    "dclip_layernorm_bwd_ex_f16": (I, [P, P, P, P, P, P, P, P, P, P, P, I, I, I, P, Z, P]),
    "dclip_transpose_to_f16": (I, [P, I, P, P, I, I, I, I, I, P]),
    "dclip_rowsum_f16": (I, [P, P, I, I, I, P]),
    "dclip_colsum_f16": (I, [P, P, I, I, I, I, P, Z, P]),
    "dclip_mt_weights_f16": (I, [P, I, I, P]),
    "dclip_attention_fwd_f16_lse": (I, [P, P, P, I, I, I, I, P]),
    "dclip_attention_bwd_f16": (I, [P, P, P, P, P, I, I, I, I, P]),
    "dclip_clip_coef_scaled": (I, [P, I, F, P, P, P]),
    "dclip_mt_adamw_f32_skip": (I, [P, I, I, F, F, F, F, F, P, P]),
    "dclip_amp_update_scale": (I, [P, P, P, F, F, I, P]),
    "dclip_gelu_erf_f32": (I, [P, P, Z, P]),
    "dclip_gelu_erf_bf16": (I, [P, P, Z, P]),
    "dclip_gelu_erf_f16": (I, [P, P, Z, P]),
    "dclip_gelu_erf_bwd_f32": (I, [P, P, P, Z, P]),
}

_lib = None


class DclipError(RuntimeError):
    pass


def load():
    """Load the shared library and bind every declared entry point (raises if any is missing)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DclipError(
            f"{LIB_PATH} not found: build it with `make` (or `python -c 'import __graft_entry__ as g; g.build()'`). "
            "dclip_amd has no CPU or PyTorch fallback for its kernels.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.dclip_abi_version() != 1:
        raise DclipError(f"ABI version mismatch: library reports {lib.dclip_abi_version()}")
    _lib = lib
    return lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = load().dclip_last_error().decode(errors="replace")
        raise DclipError(f"{what or 'dclip call'} failed (rc={rc}): {msg}")
