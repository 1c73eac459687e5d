"""Explicit forward / backward schedules of the CLIP towers over the C-ABI kernels.

No tracing compiler and no autograd inside a tower: each function below is the fixed launch
sequence for one pre-LN transformer stack (hf:modeling_clip.py:362-383) and its hand-derived
backward.  `functional.py` wraps a whole tower as ONE torch.autograd.Function so that the
reference's training scripts (`loss.backward()`, torch optimizers) keep working unchanged.

Shapes: activations are [M = B*S, D] row-major.  Per layer the forward keeps
(x, ln1, qkv, attn, lse, x1, ln2, h, g + LN statistics) for the backward; with 288 GB of HBM per
MI355X nothing is recomputed (12 layers x ~630 MB at B=256, S=50, D=768).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional

import os

import torch

from . import _lib, ops


@dataclass
class LayerParams:
    ln1_w: torch.Tensor
    ln1_b: torch.Tensor
    qkv_w: torch.Tensor      # [3D, D] = rows [q | k | v], the in-memory fusion of q_proj/k_proj/v_proj
    qkv_b: torch.Tensor
    out_w: torch.Tensor
    out_b: torch.Tensor
    ln2_w: torch.Tensor
    ln2_b: torch.Tensor
    fc1_w: torch.Tensor
    fc1_b: torch.Tensor
    fc2_w: torch.Tensor
    fc2_b: torch.Tensor

    FIELDS = ("ln1_w", "ln1_b", "qkv_w", "qkv_b", "out_w", "out_b", "ln2_w", "ln2_b", "fc1_w", "fc1_b", "fc2_w",
              "fc2_b")

    def tensors(self):
        return [getattr(self, f) for f in self.FIELDS]


class Split16Layer:
    """One layer's view of a tower's device-side split-fp16 plan (_vision_split16_plan): the [hi|hi|lo] fp16
    copies of its four GEMM weights and the ADDRESSES of its scales in the plan record.  Handed to layer_fwd /
    last_layer_fwd_cls as `sp`: their full-size GEMMs then run on the fp16 MFMAs with split operands; None = plain fp32."""
    __slots__ = ("w", "base", "wt")

    def __init__(self, w: Dict[str, torch.Tensor], base: int, wt: Optional[Dict[str, torch.Tensor]] = None):
        self.w, self.base, self.wt = w, base, wt      # wt: the transposed copies, for the backward's dgrads (§9e)

    def act(self, name: str) -> int:
        return self.base + 4 * ops.SPLIT16_PLAN_ACT[name]

    def alpha(self, name: str) -> int:
        return self.base + 4 * ops.SPLIT16_PLAN_ALPHA[name]

    def walpha(self, name: str) -> int:
        return self.base + 4 * ops.SPLIT16_PLAN_WALPHA[name]


# The three steps of a layer schedule that differ between the plain fp32 path (sp None) and the split-fp16 one: each returns
# the GEMM operand first (the fp32 tensor itself / its [hi|lo|hi] split) and the fp32 tensors the backward keeps.

def split16_pieces(consumers, plan=None, on: Optional[bool] = None, fused_k: Optional[bool] = None) -> int:
    """How many pieces the producer of a split activation / gradient operand writes: 2, [hi|lo], exactly when
    EVERY K-major GEMM that will read it — `consumers`, one (M, N, K logical) each, known at the producer's call — takes a fused
    entry, which never reads the third piece: the test _fused_k makes at the consumer (the switch DCLIP_SPLIT16_FUSED and
    ops.gemm_f16x3_plan).  3, [hi|lo|hi], everywhere else — tiny towers, shapes below DCLIP_F16X3_MIN, DCLIP_SPLIT16_FUSED=0 —
    and with DCLIP_SPLIT16_PIECES2=0.  The weight-gradient consumers address either layout and do not count.  A pure function of
    the shapes and the switches (`plan`, `on`, `fused_k`: stand-ins for ops.gemm_f16x3_plan and the two switches)."""
    on = _SPLIT16_PIECES2 if on is None else on
    fused_k = _SPLIT16_FUSED_K if fused_k is None else fused_k
    plan = ops.gemm_f16x3_plan if plan is None else plan
    consumers = list(consumers)
    return 2 if on and fused_k and consumers and all(plan(M, N, K) > 0 for M, N, K in consumers) else 3


def _ln_operand(x, w, b, eps: float, save: bool, sp: Optional[Split16Layer], name: str, pieces: int = 3, save32: bool = True):
    if sp is None:
        ln, m, r = ops.layernorm_fwd(x, w, b, eps, save_stats=save)
        return ln, ln, m, r
    return ops.layernorm_fwd_f16x3_dev(x, w, b, eps, sp.act(name), save=save, pieces=pieces, save32=save32)


class _Remat:
    """An fp32 operand of a weight gradient that the forward did not store: its shape, and how to make it again —
    bit for bit — on the rare path that reads it (linear_param_grads' fp32 GEMM)."""
    __slots__ = ("shape", "make")

    def __init__(self, shape, make):
        self.shape, self.make = tuple(shape), make


def _drops32(keep_split: bool, save: bool, sp: Optional[Split16Layer], out_f: int, in_f: int, tokens: int) -> bool:
    """Whether a forward that keeps its split operands leaves out the fp32 copy of the operand of the weight gradient dW [out_f,
    in_f]: that gradient has a split plan, so only the fp32 fall-back would read the copy — and it makes it again."""
    return bool(_VSPLIT16_DROP32 and save and keep_split and sp is not None and
                ops.gemm_f16_wgrad_tokmajor_seg3_plan(out_f, in_f, tokens) > 0)


def _a_pieces(a3, w3) -> int:
    """2 for an operand a3 = [hi|lo] [M, 2K], 3 for [hi|lo|hi]; its weight w3 is [hi|hi|lo] [N, 3K] either way."""
    return 2 if 2 * w3.shape[1] == 3 * a3.shape[1] else 3


def _fused_k(a3, w3) -> bool:
    """Whether a split GEMM of a3 [M, 3K] with w3 [N, 3K] takes its fused twin: the switch is on and the plan says
    so — exactly where the 3 K form takes the ping-pong kernel; elsewhere the call is what it was.  A two-piece a3 (§9j) is made
    only where this holds: the 3 K form cannot read it, and there is no other path."""
    if _a_pieces(a3, w3) == 2:
        K = w3.shape[1] // 3
        if not (_SPLIT16_FUSED_K and ops.gemm_f16x3_plan(a3.shape[0], w3.shape[0], K) > 0):
            raise RuntimeError(f"a two-piece split operand {tuple(a3.shape)} met a GEMM (N = {w3.shape[0]}, K = {K}) without a fused entry")
        return True
    k3 = min(a3.shape[1], w3.shape[1])
    return bool(_SPLIT16_FUSED_K and k3 % 3 == 0 and ops.gemm_f16x3_plan(a3.shape[0], w3.shape[0], k3 // 3) > 0)


def _gemm_f16_dev(a3, w3, alpha_ptr: int, out_pieces: int = 3, **kw):
    if _fused_k(a3, w3):
        return ops.gemm_f16x3_dev(a3, w3, alpha_ptr, pieces=_a_pieces(a3, w3), out_pieces=out_pieces, **kw)
    if out_pieces != 3:
        raise RuntimeError("a two-piece split output needs the fused entry")
    return ops.gemm_f16_dev(a3, w3, alpha_ptr, **kw)


def _linear(a, w, sp: Optional[Split16Layer], name: str, bias, residual=None):
    if sp is None:
        return ops.gemm(a, w, ops.LAYOUT_NT, bias=bias, residual=residual)
    return _gemm_f16_dev(a, sp.w[name], sp.alpha(name), bias=bias, residual=residual)


# The MLP activation of a tower (cfg.hidden_act).  "quick_gelu" is what every GEMM epilogue computes and what every
# call below was before the field existed, launch for launch.  "gelu" (exact erf GELU) has no epilogue: fc1 is a bias-only GEMM
# and the activation a stand-alone pass (ops.gelu_erf / ops.gelu_erf_bwd).  The choice is made in three places — _fc1_act_f32 and
# _dgelu_f32 for the fp32 schedules, _fc1_act16 for the frozen 16-bit ones; the split-fp16 plans, whose fused epilogues and
# rematerialised g are quick-GELU, decline a "gelu" tower (_split16_declines_act) and the 16-bit TRAINING path refuses it.
QUICK_GELU, GELU_ERF = "quick_gelu", "gelu"


def hidden_act(cfg) -> str:
    """A tower configuration's activation; a configuration without the field is a quick-GELU tower."""
    act = getattr(cfg, "hidden_act", QUICK_GELU)
    if act not in (QUICK_GELU, GELU_ERF):
        raise ValueError(f"hidden_act {act!r} is not supported (one of {(QUICK_GELU, GELU_ERF)})")
    return act


def _fc1_act_f32(a, p: LayerParams, act: str, save: bool = False):
    """(g, h) of the fp32 MLP: h = a fc1_w^T + b (kept only with `save`, else None), g = act(h)."""
    h = torch.empty((a.shape[0], p.fc1_w.shape[0]), dtype=torch.float32, device=a.device) if save else None
    if act == GELU_ERF:
        pre = ops.gemm(a, p.fc1_w, ops.LAYOUT_NT, bias=p.fc1_b, out=h)
        return ops.gelu_erf(pre, out=None if save else pre), h      # in place when nothing is saved
    return ops.gemm(a, p.fc1_w, ops.LAYOUT_NT, bias=p.fc1_b, aux=h, epilogue=ops.EPI_GELU), h


def _dgelu_f32(dy, w, h, act: str):
    """dh = (dy w) act'(h): the fp32 data gradient of fc2 through the activation."""
    if act == GELU_ERF:
        dg = ops.gemm(dy, w, ops.LAYOUT_NN)
        return ops.gelu_erf_bwd(h, dg, out=dg)
    return ops.gemm(dy, w, ops.LAYOUT_NN, aux=h, epilogue=ops.EPI_DGELU)


def _fc1_act16(k, a16, w16, bias, act: str):
    """16-bit g = act(a16 w16^T + bias) of a frozen 16-bit schedule (k: its _Ops16).  "gelu": the activation of the STORED 16-bit
    pre-activation, in place — the statement of the quick-GELU 16-bit epilogue (include/dclip_hip.h, 16-bit output)."""
    if act == GELU_ERF:
        h16 = k.gemm(a16, w16, bias=bias, out16=True)
        return ops.gelu_erf(h16, out=h16)
    return k.gemm(a16, w16, bias=bias, gelu=True, out16=True)


def _split16_declines_act(cfg, what: str) -> bool:
    """True — logged once — for a "gelu" tower at a split-fp16 switch: the plans' fused fc1 epilogues and the g a backward makes
    again are quick-GELU, so such a tower takes the plain fp32 path, the way a tripped weight guard falls back."""
    if hidden_act(cfg) != GELU_ERF:
        return False
    _split16_log_once(f"{what}: hidden_act='gelu' has no split-fp16 form; the tower takes the plain fp32 path")
    return True


def _fc1_gelu(a, p: LayerParams, save: bool, sp: Optional[Split16Layer], pieces: int = 3, save_g32: bool = True,
              act: str = QUICK_GELU):
    """(operand of fc2, h, g): g = act(h), h = a fc1_w^T + b kept only with `save`.  `pieces`: of the split operand;
    `save_g32` False (`sp` only): the fp32 g is not kept (None).  `sp` is quick-GELU only."""
    M, I = a.shape[0], p.fc1_w.shape[0]
    if sp is None:
        g, h = _fc1_act_f32(a, p, act, save)
        return g, h, g
    if act != QUICK_GELU:
        raise RuntimeError(f"the split-fp16 fc1 epilogue is quick-GELU: a {act!r} layer must not reach it")
    h = torch.empty((M, I), dtype=torch.float32, device=a.device) if save else None
    g = torch.empty((M, I), dtype=torch.float32, device=a.device) if save and save_g32 else None
    if _VSPLIT16_FC1_EPI:
        g3 = _gemm_f16_dev(a, sp.w["fc1"], sp.alpha("fc1"), out_pieces=pieces, bias=p.fc1_b, gelu=True,
                           split_out_scale_ptr=sp.act("g"), h32=h, g32=g)
        return g3, h, g
    # two-launch form (bit-identical results; kept for the A/B of DESIGN.md §9d): h and g leave the GEMM, g is split after it
    g = _gemm_f16_dev(a, sp.w["fc1"], sp.alpha("fc1"), bias=p.fc1_b, gelu=True, h32=h)
    return ops.split_f16x3_dev(g, sp.act("g"), pieces=pieces), h, (g if save and save_g32 else None)


def _layer_pieces(T: int, D: int, I: int, fc1_epi: bool) -> Dict[str, int]:
    """Pieces of the four split operands of an encoder layer's forward at T rows (split16_pieces): ln1 feeds qkv, the context out,
    ln2 fc1 and g fc2.  Where g leaves fc1's epilogue (`fc1_epi`) it has its two-piece form on the fused entry only."""
    pc = {"ln1": split16_pieces([(T, 3 * D, D)]), "ctx": split16_pieces([(T, D, D)]), "ln2": split16_pieces([(T, I, D)]),
          "g": split16_pieces([(T, D, I)])}
    if fc1_epi and pc["ln2"] == 3 and not (_SPLIT16_FUSED_K and ops.gemm_f16x3_plan(T, I, D) > 0):
        pc["g"] = 3
    return pc


def layer_fwd(x, p: LayerParams, B: int, S: int, H: int, causal: bool, eps: float, save: bool, sp: Optional[Split16Layer] = None,
              keep_split: bool = False, varlen=None, act: str = QUICK_GELU):
    """`act`: the MLP activation (hidden_act).  `keep_split` (with `save` and `sp`): the four [hi|lo|hi] (or [hi|lo], §9j) operands this forward produced anyway — of ln1,
    the attention context, ln2 and g — are kept as a 14th entry of `saved`, the X operands of the split-fp16 weight gradients
    (DESIGN.md §9f).  The fp32 ln1, ln2 and g are then None in `saved` wherever that weight gradient has a split plan (_drops32,
    §9j): layer_bwd makes them again if it lands on the fp32 weight gradient after all.
    `varlen` = (cu_seqlens, max_S): x holds packed captions and the attention core is the ragged causal one;
    B and S are not read then.  Causal only; with `sp` the ragged attention is followed by the split pass of its context
    (DESIGN.md §30)."""
    T, D, I = x.shape[0], x.shape[1], p.fc1_w.shape[0]
    pc = _layer_pieces(T, D, I, _VSPLIT16_FC1_EPI) if sp is not None else {}
    a1, ln1, m1, r1 = _ln_operand(x, p.ln1_w, p.ln1_b, eps, save, sp, "ln1", pc.get("ln1", 3),
                                  not _drops32(keep_split, save, sp, 3 * D, D, T))
    qkv = _linear(a1, p.qkv_w, sp, "qkv", p.qkv_b)
    if varlen is None:
        attn, lse = ops.attention_fwd(qkv, B, S, H, causal)
    else:
        if not causal:
            raise ValueError("layer_fwd: the packed layer is causal")
        attn, lse = ops.attention_varlen_causal_fwd(qkv, varlen[0], varlen[1], H, want_lse=True)
    ac = attn if sp is None else ops.split_f16x3_dev(attn, sp.act("ctx"), pieces=pc["ctx"])
    x1 = _linear(ac, p.out_w, sp, "out", p.out_b, residual=x)
    a2, ln2, m2, r2 = _ln_operand(x1, p.ln2_w, p.ln2_b, eps, save, sp, "ln2", pc.get("ln2", 3),
                                  not _drops32(keep_split, save, sp, I, D, T))
    ag, h, g = _fc1_gelu(a2, p, save, sp, pc.get("g", 3), not _drops32(keep_split, save, sp, D, I, T), act)
    x2 = _linear(ag, p.fc2_w, sp, "fc2", p.fc2_b, residual=x1)
    saved = (x, m1, r1, ln1, qkv, attn, lse, x1, m2, r2, ln2, h, g) if save else None
    if save and keep_split and sp is not None:
        saved = saved + ({"ln1": a1, "ctx": ac, "ln2": a2, "g": ag},)
    return x2, saved


def _fresh(_name: str, shape, device) -> torch.Tensor:
    return torch.empty(shape, dtype=torch.float32, device=device)


def _galloc(alloc, name: str, shape, device) -> torch.Tensor:
    """Where a parameter gradient is written.  `alloc(name, shape)` (data parallel: dist.GradSync hands out the
    parameter's slice of its persistent all-reduce bucket, so the wgrad GEMM writes straight into it) may return None."""
    t = alloc(name, shape) if alloc is not None else None
    return t if t is not None else _fresh(name, shape, device)


def linear_param_grads(dy, x, need_w: bool, need_b: bool, gr: Dict[str, torch.Tensor], wkey: str, bkey: str, alloc=None,
                       sp: Optional[Split16Layer] = None, act: Optional[str] = None, x3: Optional[torch.Tensor] = None,
                       stats=None, db_segments=None):
    """dW = dy^T x and db = colsum(dy) of one nn.Linear.  When both are wanted the bias gradient comes out of the
    weight-gradient GEMM (DCLIP_EPI_A_ROWSUM): dy is streamed once, no separate column-sum launch.
    `sp`, `act`, `x3` (the forward's [hi|lo|hi] split of x, made with the plan scale sp.act(act)): the split-fp16 weight
    gradient when the plan takes the shape — ONE pass over dy gives its row split (for _dgrad), its column
    statistics, db and its column-scaled [hi|lo] split; dW is the segmented token-major GEMM of that with x3 (x itself, which may
    be a _Remat, gives its shape only).  Returns the row
    pieces (dy3, row_alpha) for _dgrad then, None otherwise.  `stats`: the column partials (a ColStats, _with_stats) that the
    producer of dy left — dy is then read ONCE: the finish over the partials, then one pass that writes both splits (§9g).
    `db_segments` = (B, S), for a dy without partials: the bias gradient is summed per caption in the statistics form's order
    (ops.colsum_segments, §30)."""
    dev = dy.device
    if dy.dim() == 2 and dy.stride(1) == 1 and _split_wgrad_taken(need_w, sp, x3, dy.shape[1], x.shape[1], dy.shape[0]):
        M, N = dy.shape[1], x.shape[1]
        db = _galloc(alloc, bkey, (M,), dev) if need_b else None
        st = stats if _VSPLIT16_DYSTATS else None
        pc = split16_pieces([(dy.shape[0], N, M)])      # the row pieces' one reader: _dgrad's dX [tokens, in_f] = dy3 wt^T along out_f
        if st is not None:
            dy3, row_alpha, yc, _, col_alpha = ops.split_f16x3_rows_cols_stats(dy, st, db=db, pieces=pc)
        elif need_b and db_segments is not None:      # §30: the bias gradient in the statistics form's order
            dy3, row_alpha, yc, _, col_alpha = ops.split_f16x3_rows_colstats(dy, db=None, pieces=pc)
            ops.colsum_segments(dy, *db_segments, out=db)
        else:
            dy3, row_alpha, yc, _, col_alpha = ops.split_f16x3_rows_colstats(dy, db=db, pieces=pc)
        if need_b:
            gr[bkey] = db
        out = _galloc(alloc, wkey, (M, N), dev)
        if _SPLIT16_FUSED_TOK and ops.gemm_f16x3_wgrad_tokmajor_plan(M, N, dy.shape[0]) > 0:      # the fused twin (§9h)
            gr[wkey] = ops.gemm_f16x3_wgrad_tokmajor(yc, x3, M, N, col_alpha, sp.act(act), out=out)
        else:
            gr[wkey] = ops.gemm_f16_wgrad_tokmajor_seg3(yc, x3, M, N, col_alpha, sp.act(act), out=out)
        return dy3, row_alpha
    if need_w and isinstance(x, _Remat):      # the forward did not store it (§9j): made again, bit for bit
        x = x.make()
    if need_w and need_b:
        gr[bkey] = _galloc(alloc, bkey, (dy.shape[1],), dev)
        gr[wkey] = ops.gemm(dy, x, ops.LAYOUT_TN, out=_galloc(alloc, wkey, (dy.shape[1], x.shape[1]), dev), a_rowsum=gr[bkey])
    elif need_w:
        gr[wkey] = ops.gemm(dy, x, ops.LAYOUT_TN, out=_galloc(alloc, wkey, (dy.shape[1], x.shape[1]), dev))
    elif need_b:
        gr[bkey] = ops.colsum(dy, out=_galloc(alloc, bkey, (dy.shape[1],), dev))
    return None


def _split_wgrad_taken(need_w: bool, sp: Optional[Split16Layer], x3, out_f: int, in_f: int, tokens: int) -> bool:
    """Whether linear_param_grads takes the split-fp16 weight gradient for a dY [tokens, out_f] and an x [tokens, in_f]."""
    return bool(need_w and sp is not None and x3 is not None and _VSPLIT16_WGRAD and
                ops.gemm_f16_wgrad_tokmajor_seg3_plan(out_f, in_f, tokens) > 0)


def patch_split16_taken(save_with_cache: bool, grid, rows: int, D: int, patch_dim: int, backward: bool = False,
                        on: Optional[bool] = None, plan=None, wplan=None) -> bool:
    """Whether a vision forward runs its patch embedding [rows, patch_dim] x [D, patch_dim] on split-fp16 operands,
    and with `backward` whether its backward may take patch_w's gradient from the same operands.  All of: the switches
    (DCLIP_VISION_SPLIT16_PATCH under DCLIP_VISION_SPLIT16; for the backward half DCLIP_VISION_SPLIT16_BWD and _WGRAD too), a
    forward that saves for a backward with the model's split cache (`save_with_cache`), the configuration's square grid (`grid`
    None), patch_dim % 32 == 0 (ViT-L/14's 588 declines), rows % 64 == 0 and the plans: ops.split16_patch_plan (the fused K-major
    entry's plan and a tile threshold of its own) and, for the backward half, ops.gemm_f16x3_wgrad_tokmajor_plan.  A pure function
    of the shapes and the switches (`on`, `plan`, `wplan`: stand-ins for the switches and the two plans)."""
    if on is None:
        on = _VSPLIT16 and _VSPLIT16_PATCH and (not backward or (_VSPLIT16_BWD and _VSPLIT16_WGRAD))
    if not (on and save_with_cache and grid is None and rows > 0 and patch_dim % 32 == 0 and rows % 64 == 0):
        return False
    if (ops.split16_patch_plan if plan is None else plan)(rows, D, patch_dim) <= 0:
        return False
    return not backward or (ops.gemm_f16x3_wgrad_tokmajor_plan if wplan is None else wplan)(D, patch_dim, rows) > 0


class _PatchSplit:
    """What a forward that took the split patch embedding saves in place of the fp32 columns: the fp16 [hi|lo]
    columns (the same bytes; None where the backward half is not on), the forward's own front record (their scale lives in it) and
    the pixels with the patch size, from which the fp32 columns are made again on the path that needs them."""
    __slots__ = ("cols16", "rec", "pixels", "patch")

    def __init__(self, cols16, rec, pixels, patch: int):
        self.cols16, self.rec, self.pixels, self.patch = cols16, rec, pixels, patch


def _dystats_regime(tokens: int, D: int, I: int) -> bool:
    """Whether a tower's backward asks its producers of dY for column partials at all: the switch is on and the
    step is large enough for its data-gradient GEMMs to run on the ping-pong kernel (fc2's, [tokens, 3 D] x [I, 3 D], stands for
    the four).  That is where the single pass was measured and where it can pay: below it a dY fits the cache, its second read
    costs no memory traffic, the step is launch-bound, and the schedule stays §9f's, launch for launch."""
    return bool(_VSPLIT16_DYSTATS and ops.gemm_f16_rows_stats_plan(tokens, I, 3 * D) > 0)


def _with_stats(want: bool, P: int, cols: int, dev):
    """The ColStats a producer of dY is handed: only when the weight gradient that follows will take the split path
    (`want`, _split_wgrad_taken), the switch is on and the producer's plan P says yes; None = the three-launch pass as before."""
    return ops.ColStats(P, cols, dev) if want and _VSPLIT16_DYSTATS and P > 0 else None


def _attention_bwd_stats_form(B: int, S: int, H: int, causal: bool):
    """(ops.attention_bwd's keyword, partial rows) of the statistics form of the dense attention backward at S tokens: the one-tile
    kernel's up to 64 (§9g), and for the CAUSAL tower — the text tower; a vision tower of 65 .. 80 tokens keeps the schedule it
    had — the whole-row kernel's twin for 65 .. 80.  (None, 0) where there is none: dqkv then takes the
    three-launch split.  ("segments", 0): the twin exists but DCLIP_TEXT_SPLIT16_ROWS_STATS=0 switched it off — the three-launch
    split, with the bias gradient summed per caption as the twin's partials are (ops.colsum_segments), so that the switch
    changes no training result."""
    P = ops.attention_bwd_stats_plan(B, S, H)
    if P > 0:
        return "stats", P
    P = ops.attention_bwd_rows_stats_plan(B, S, H) if causal else 0
    if P > 0 and not _TSPLIT16_ROWS_STATS:
        return "segments", 0
    return ("rows_stats", P) if P > 0 else (None, 0)


def _ln_bwd(dy, x, gamma, mean, rstd, dresidual, want: bool, gr, wkey: str, bkey: str, alloc, dx_stats: bool = False):
    """LayerNorm backward -> (dx, stats); dγ / dβ land where `alloc` says.  `dx_stats`: dx is the dY of a split weight gradient
    and its column partials are asked for; `stats` is that ColStats when the kernel has the form, None otherwise."""
    D = x.shape[-1]
    st = _with_stats(dx_stats, ops.layernorm_bwd_stats_plan(x.numel() // D, D) if dx_stats else 0, D, dy.device)
    if want:
        dg = _galloc(alloc, wkey, tuple(gamma.shape), dy.device)
        db = _galloc(alloc, bkey, tuple(gamma.shape), dy.device)
        dx, dg, db = ops.layernorm_bwd(dy, x, gamma, mean, rstd, dresidual=dresidual, dgamma=dg, dbeta=db, accumulate=False, stats=st)
        gr[wkey], gr[bkey] = dg, db
    else:
        dx, _, _ = ops.layernorm_bwd(dy, x, gamma, mean, rstd, dresidual=dresidual, need_param_grads=False, stats=st)
    return dx, st


def _dgrad(dy, w, sp: Optional[Split16Layer], name: str, aux=None, rows=None, out_stats: bool = False, act: str = QUICK_GELU):
    """(dX, stats): dX = dy w (times act'(aux) when given; `sp` is quick-GELU only), the data gradient of a linear layer.  `sp` (a Split16Layer with
    transposed copies): dy is split with one scale per row and meets the [hi|hi|lo] copy of w^T on the fp16 MFMAs (DESIGN.md
    §9e); None = the plain fp32 GEMM.  dy itself stays fp32 for the weight and bias gradients.  `rows`: the row pieces
    (dy3, row_alpha) when linear_param_grads has already made them in its fused pass (§9f).  `out_stats`: dX is itself the dY of
    a split weight gradient and its column partials are asked for (§9g); `stats` is that ColStats when the GEMM's plan has the
    form, None otherwise."""
    if sp is None:
        if aux is None:
            return ops.gemm(dy, w, ops.LAYOUT_NN), None
        return _dgelu_f32(dy, w, aux, act), None
    if aux is not None and act != QUICK_GELU:
        raise RuntimeError(f"the split-fp16 data gradient's epilogue is quick-GELU: a {act!r} layer must not reach it")
    wt = sp.wt[name]
    dy3, row_alpha = rows if rows is not None else ops.split_f16x3_rows(
        dy, pieces=split16_pieces([(dy.shape[0], wt.shape[0], wt.shape[1] // 3)]))
    k3 = min(dy3.shape[1], wt.shape[1])
    if _fused_k(dy3, wt):      # the fused twin (§9h); its statistics plan is the unfused one's wherever it is taken
        K = wt.shape[1] // 3 if _a_pieces(dy3, wt) == 2 else k3 // 3
        st = _with_stats(out_stats, ops.gemm_f16x3_rows_stats_plan(dy3.shape[0], wt.shape[0], K) if out_stats else 0, wt.shape[0],
                         dy3.device)
        dx = ops.gemm_f16x3_rows_dev(dy3, wt, sp.walpha(name), row_alpha, dgelu_h=aux, stats=st, pieces=_a_pieces(dy3, wt))
    else:
        st = _with_stats(out_stats, ops.gemm_f16_rows_stats_plan(dy3.shape[0], wt.shape[0], k3) if out_stats else 0, wt.shape[0],
                         dy3.device)
        dx = ops.gemm_f16_rows_dev(dy3, wt, sp.walpha(name), row_alpha, dgelu_h=aux, stats=st)
    return dx, st


def _remat_ln(ln, x, w, b, eps: Optional[float]):
    """The saved fp32 LayerNorm output, or — where the forward left it out (§9j) — how to make it again from the saved input."""
    if ln is not None:
        return ln
    if eps is None:
        raise ValueError("the forward did not keep an fp32 LayerNorm output: the backward needs the layer's eps")
    return _Remat(x.shape, lambda: ops.layernorm_fwd(x, w, b, eps, save_stats=False)[0])


def layer_bwd(dx2, p: LayerParams, saved, B: int, S: int, H: int, causal: bool, need: Dict[str, bool], alloc=None,
              sp: Optional[Split16Layer] = None, dx_stats: bool = False, dystats: bool = False, eps: Optional[float] = None,
              varlen=None, dx2_stats=None, act: str = QUICK_GELU):
    """Returns (dx, grads, stats) with grads keyed like LayerParams.FIELDS (missing = not needed).  `varlen`, `act`: as in layer_fwd.
    `alloc(field, shape)`: see _galloc.  `sp`: the four data-gradient GEMMs take the split-fp16 path (_dgrad).  `eps`: the layer's,
    for an fp32 LayerNorm output the forward did not keep (_remat_ln, §9j).  `dystats` (the caller's decision for the whole
    tower, _dystats_regime): each kernel that produces the dY of a weight gradient that will take the split path is asked for
    its column partials (§9g), and they go to that weight gradient as a value.  `dx_stats`: the caller says so for the returned
    dx (the layer below's fc2) — `stats` is then its ColStats, or None where the kernel has no such form; `dx2_stats`: what the
    producer of dx2 returned that way (None: dx2 takes the three-launch pass)."""
    x, m1, r1, ln1, qkv, attn, lse, x1, m2, r2, ln2, h, g = saved[:13]
    s3 = saved[13] if len(saved) > 13 and sp is not None else {}      # the forward's split operands (layer_fwd, keep_split)
    gr: Dict[str, torch.Tensor] = {}
    T, D, I = x.shape[0], x.shape[1], p.fc1_w.shape[0]
    ln1, ln2 = _remat_ln(ln1, x, p.ln1_w, p.ln1_b, eps), _remat_ln(ln2, x1, p.ln2_w, p.ln2_b, eps)
    if g is None:
        g = _Remat(h.shape, lambda: ops.quick_gelu(h))
    rows = linear_param_grads(dx2, g, bool(need.get("fc2_w")), bool(need.get("fc2_b")), gr, "fc2_w", "fc2_b", alloc, sp, "g", s3.get("g"),
                              stats=dx2_stats)
    dh, dh_stats = _dgrad(dx2, p.fc2_w, sp, "fc2", aux=h, rows=rows,
                          out_stats=dystats and _split_wgrad_taken(bool(need.get("fc1_w")), sp, s3.get("ln2"), I, D, T), act=act)
    rows = linear_param_grads(dh, ln2, bool(need.get("fc1_w")), bool(need.get("fc1_b")), gr, "fc1_w", "fc1_b", alloc, sp, "ln2",
                              s3.get("ln2"), stats=dh_stats)
    dln2, _ = _dgrad(dh, p.fc1_w, sp, "fc1", rows=rows)
    del dh
    dx1, dx1_stats = _ln_bwd(dln2, x1, p.ln2_w, m2, r2, dx2, bool(need.get("ln2_w") or need.get("ln2_b")), gr, "ln2_w", "ln2_b", alloc,
                             dx_stats=dystats and _split_wgrad_taken(bool(need.get("out_w")), sp, s3.get("ctx"), D, D, T))
    rows = linear_param_grads(dx1, attn, bool(need.get("out_w")), bool(need.get("out_b")), gr, "out_w", "out_b", alloc, sp, "ctx",
                              s3.get("ctx"), stats=dx1_stats)
    dattn, _ = _dgrad(dx1, p.out_w, sp, "out", rows=rows)
    qkv_stats = dystats and _split_wgrad_taken(bool(need.get("qkv_w")), sp, s3.get("ln1"), 3 * D, D, T)
    db_segments = None
    if varlen is None:
        form, P = _attention_bwd_stats_form(B, S, H, causal) if qkv_stats else (None, 0)
        st = _with_stats(qkv_stats, P, 3 * D, dattn.device)
        dqkv = ops.attention_bwd(qkv, attn, dattn, lse, B, S, H, causal, **({form: st} if st is not None else {}))
        if form == "segments" and _VSPLIT16_DYSTATS:
            db_segments = (B, S)
    else:
        if not causal:
            raise ValueError("layer_bwd: the packed layer is causal")
        st = None      # the tiled ragged kernels have no statistics form: dqkv takes the three-launch split (§30)
        dqkv = ops.attention_varlen_causal_bwd(qkv, varlen[0], attn, dattn, lse, varlen[1], H)
    rows = linear_param_grads(dqkv, ln1, bool(need.get("qkv_w")), bool(need.get("qkv_b")), gr, "qkv_w", "qkv_b", alloc, sp, "ln1",
                              s3.get("ln1"), stats=st, db_segments=db_segments)
    dln1, _ = _dgrad(dqkv, p.qkv_w, sp, "qkv", rows=rows)
    del dqkv, rows
    dx, stats = _ln_bwd(dln1, x, p.ln1_w, m1, r1, dx1, bool(need.get("ln1_w") or need.get("ln1_b")), gr, "ln1_w", "ln1_b", alloc,
                        dx_stats=dx_stats)
    return dx, gr, stats


# --------------------------------------------------------------------------------------------- last vision layer
# After the final encoder layer the model reads ONLY the CLS row of each image (hf:modeling_clip.py:650-651).  In
# that layer everything downstream of the attention — out_proj, LayerNorm2, fc1, quick-GELU, fc2 and both residual
# adds — is row-wise, so it is evaluated for the B CLS rows instead of all B*S rows, and the attention itself for
# one query row per (image, head).  In the backward the incoming gradient is nonzero only on those rows, so the
# same restriction is exact there too (the other rows' contributions to every weight gradient are products with
# zero).  K and V, hence the qkv projection, LayerNorm1 and their gradients, stay full size.  Results are identical
# to the unpruned schedule (tests/test_model_gpu.py); 9/12 of that layer's GEMM work disappears.

def last_layer_fwd_cls(x, p: LayerParams, B: int, S: int, H: int, eps: float, save: bool, sp: Optional[Split16Layer] = None,
                       keep_split: bool = False, act: str = QUICK_GELU):
    """`sp`: the full-size qkv projection takes the split-fp16 path (layer_fwd); the M = B GEMMs stay on ops.gemm.
    `keep_split`: ln1's split is kept for the qkv weight gradient (layer_fwd)."""
    D = x.shape[1]
    a, ln1, m1, r1 = _ln_operand(x, p.ln1_w, p.ln1_b, eps, save, sp, "ln1",
                                 3 if sp is None else split16_pieces([(x.shape[0], 3 * D, D)]),
                                 not _drops32(keep_split, save, sp, 3 * D, D, x.shape[0]))
    qkv = _linear(a, p.qkv_w, sp, "qkv", p.qkv_b)
    attn, lse = ops.attention_cls_fwd(qkv, B, S, H)                       # [B, D]
    x_cls = ops.gather_rows(x, None, B, S, D)
    x1 = ops.gemm(attn, p.out_w, ops.LAYOUT_NT, bias=p.out_b, residual=x_cls)
    ln2, m2, r2 = ops.layernorm_fwd(x1, p.ln2_w, p.ln2_b, eps, save_stats=save)
    g, h = _fc1_act_f32(ln2, p, act, save)
    x2 = ops.gemm(g, p.fc2_w, ops.LAYOUT_NT, bias=p.fc2_b, residual=x1)   # [B, D] = final hidden state, CLS rows
    saved = (x, m1, r1, ln1, qkv, attn, lse, x1, m2, r2, ln2, h, g) if save else None
    if save and keep_split and sp is not None:
        saved = saved + ({"ln1": a},)
    return x2, saved


def last_layer_bwd_cls(dx2, p: LayerParams, saved, B: int, S: int, H: int, need: Dict[str, bool], alloc=None,
                       sp: Optional[Split16Layer] = None, dx_stats: bool = False, eps: Optional[float] = None,
                       act: str = QUICK_GELU):
    """dx2 [B, D] is the gradient w.r.t. the CLS rows of the final hidden state; returns (dx [B*S, D], grads, stats) — `stats`:
    dx's column partials when `dx_stats` asked for them, as layer_bwd's.  `sp`: the full-size qkv data gradient takes the
    split-fp16 path (_dgrad); the M = B GEMMs stay on ops.gemm."""
    x, m1, r1, ln1, qkv, attn, lse, x1, m2, r2, ln2, h, g = saved[:13]
    s3 = saved[13] if len(saved) > 13 and sp is not None else {}
    D = x.shape[1]
    ln1 = _remat_ln(ln1, x, p.ln1_w, p.ln1_b, eps)
    gr: Dict[str, torch.Tensor] = {}
    linear_param_grads(dx2, g, bool(need.get("fc2_w")), bool(need.get("fc2_b")), gr, "fc2_w", "fc2_b", alloc)
    dh = _dgelu_f32(dx2, p.fc2_w, h, act)
    linear_param_grads(dh, ln2, bool(need.get("fc1_w")), bool(need.get("fc1_b")), gr, "fc1_w", "fc1_b", alloc)
    dln2 = ops.gemm(dh, p.fc1_w, ops.LAYOUT_NN)
    dx1, _ = _ln_bwd(dln2, x1, p.ln2_w, m2, r2, dx2, bool(need.get("ln2_w") or need.get("ln2_b")), gr, "ln2_w", "ln2_b", alloc)
    linear_param_grads(dx1, attn, bool(need.get("out_w")), bool(need.get("out_b")), gr, "out_w", "out_b", alloc)
    dattn = ops.gemm(dx1, p.out_w, ops.LAYOUT_NN)
    dqkv = ops.attention_cls_bwd(qkv, attn, dattn, lse, B, S, H)          # [B*S, 3D]; d q only on the CLS rows
    rows = linear_param_grads(dqkv, ln1, bool(need.get("qkv_w")), bool(need.get("qkv_b")), gr, "qkv_w", "qkv_b", alloc, sp, "ln1",
                              s3.get("ln1"))
    dln1, _ = _dgrad(dqkv, p.qkv_w, sp, "qkv", rows=rows)
    del dqkv, rows
    dres = ops.scatter_rows(dx1, None, B, S, D)                           # the skip connection carries dx1 on CLS rows only
    dx, stats = _ln_bwd(dln1, x, p.ln1_w, m1, r1, dres, bool(need.get("ln1_w") or need.get("ln1_b")), gr, "ln1_w", "ln1_b", alloc,
                        dx_stats=dx_stats)      # (dqkv comes from attention_cls_bwd, which has no statistics form: three launches)
    return dx, gr, stats


# --------------------------------------------------------------------------------------------- vision tower

@dataclass
class VisionParams:
    class_embedding: torch.Tensor
    patch_w: torch.Tensor        # [D, C, p, p]
    pos: torch.Tensor            # [S, D]
    pre_w: torch.Tensor
    pre_b: torch.Tensor
    layers: List[LayerParams]
    post_w: torch.Tensor
    post_b: torch.Tensor
    proj_w: torch.Tensor         # visual_projection [P, D]

    HEAD = ("class_embedding", "patch_w", "pos", "pre_w", "pre_b")
    TAIL = ("post_w", "post_b", "proj_w")

    def tensors(self):
        out = [getattr(self, f) for f in self.HEAD]
        for l in self.layers:
            out += l.tensors()
        out += [getattr(self, f) for f in self.TAIL]
        return out

    @classmethod
    def from_tensors(cls, ts, n_layers):
        ts = list(ts)
        head = ts[:5]
        layers = [LayerParams(*ts[5 + 12 * i: 5 + 12 * (i + 1)]) for i in range(n_layers)]
        tail = ts[5 + 12 * n_layers:]
        return cls(*head, layers, *tail)

    def names(self):
        out = list(self.HEAD)
        for i in range(len(self.layers)):
            out += [f"layers.{i}.{f}" for f in LayerParams.FIELDS]
        return out + list(self.TAIL)


def _grid_seq(v, grid) -> int:
    """Tokens per image: the configuration's, or 1 + gh*gw on another patch grid (hf interpolate_pos_encoding)."""
    return v.seq_len if grid is None else 1 + grid[0] * grid[1]


def _grid_front(p: VisionParams, pixel_values: torch.Tensor, v, grid):
    """The position table resampled to a grid (gh, gw) other than the configuration's (one launch).  The pixels must make
    exactly that grid."""
    gh, gw = grid
    if (pixel_values.shape[2] // v.patch_size, pixel_values.shape[3] // v.patch_size) != (gh, gw):
        raise ValueError(f"pixel_values {tuple(pixel_values.shape)} do not make a {gh}x{gw} grid of {v.patch_size}-px patches")
    return ops.pos_interp_fwd(p.pos, v.grid, gh, gw)


def _grid_pos_grad(dpos_cols: torch.Tensor, p: VisionParams, v, grid, alloc, dev) -> torch.Tensor:
    """The position table's gradient from the [S*D] column sum taken on another grid: the transpose of the resample,
    written where `alloc` puts the parameter's gradient."""
    g, D = v.grid, v.hidden_size
    out = _galloc(alloc, "pos", (1 + g * g, D), dev)
    return ops.pos_interp_bwd(dpos_cols.view(-1, D), g, grid[0], grid[1], out=out.view(1 + g * g, D))


def vision_fwd(p: VisionParams, pixel_values: torch.Tensor, cfg, save: bool, hidden_out: Optional[list] = None, grid=None,
               split16_cache: Optional[dict] = None, split16_out: Optional[list] = None):
    """get_image_features: [B,3,H,W] -> [B,P]  (hf:modeling_clip.py:202-218, :641-651, :744-751).  `grid` = (gh, gw): run on
    that patch grid with the position table resampled to it (None: the configuration's image size, as ever).
    `split16_cache` (the model's, HipCLIPModel._vsplit16_cache): a forward that saves for the backward runs the encoder
    layers' full-size GEMMs on split-fp16 operands (DCLIP_VISION_SPLIT16) and, where patch_split16_taken says so,
    the patch embedding too (§35: the saved columns are then a _PatchSplit); a no-grad forward never does.
    `split16_out` (a list): receives what vision_bwd needs to run its data-gradient GEMMs on the same plan (Split16Bwd, §9e)
    when this forward took the split path and DCLIP_VISION_SPLIT16_BWD is on; nothing otherwise."""
    v = cfg
    B = pixel_values.shape[0]
    S, D, H = _grid_seq(v, grid), v.hidden_size, v.num_attention_heads
    front = _patch_split16_front(p, pixel_values, v, save, grid, split16_cache)
    if front is not None:                # the patch embedding on split-fp16 operands: no fp32 columns
        cols, patch, pos = *_patch_split16_fwd(p, pixel_values, v, *front), p.pos
    else:
        if grid is None:
            cols, pos = ops.im2col(pixel_values, v.patch_size), p.pos
        else:
            pos = _grid_front(p, pixel_values, v, grid)
            cols = ops.im2col_rect(pixel_values, v.patch_size)
        patch = ops.gemm(cols, p.patch_w.view(D, -1), ops.LAYOUT_NT)
    emb = ops.vision_assemble_fwd(patch, p.class_embedding, pos, B, S, D)
    del patch
    x, m0, r0 = ops.layernorm_fwd(emb, p.pre_w, p.pre_b, v.layer_norm_eps, save_stats=save)
    if hidden_out is not None:
        hidden_out.append(x)
    saved_layers = []
    prune = hidden_out is None and len(p.layers) > 0          # full hidden states are only materialised on request
    plan, keep = _train_split16(p.layers, v, save, split16_cache, split16_out, _VSPLIT16)
    act = hidden_act(v)
    for li, lp in enumerate(p.layers):
        sp = plan[li] if plan is not None else None
        if prune and li == len(p.layers) - 1:
            cls_tok, sv = last_layer_fwd_cls(x, lp, B, S, H, v.layer_norm_eps, save, sp, keep, act=act)
            saved_layers.append(sv)
            break
        x, sv = layer_fwd(x, lp, B, S, H, False, v.layer_norm_eps, save, sp, keep, act=act)
        saved_layers.append(sv)
        if hidden_out is not None:
            hidden_out.append(x)
    if not prune:
        cls_tok = ops.gather_rows(x, None, B, S, D)
    pooled, mp, rp = ops.layernorm_fwd(cls_tok, p.post_w, p.post_b, v.layer_norm_eps, save_stats=save)
    out = ops.gemm(pooled, p.proj_w, ops.LAYOUT_NT)
    saved = (cols, emb, m0, r0, saved_layers, cls_tok, mp, rp, pooled, prune, grid) if save else None
    return out, saved


# The backward of the fp32 / split-fp16 towers is assembled from the pieces below, each written once: _lowest_needed (all four
# backwards), _layers_bwd (the encoder stack of vision_bwd, text_bwd and text_bwd_packed), _vision_tail_bwd / _vision_head_bwd
# (vision_bwd and vision_bwd_bf16) and, next to the text tower, _text_tail_bwd (text_bwd and text_bwd_packed).  A schedule keeps
# what is its own: how dx enters the stack and what happens below layer 0.

def _lowest_needed(names, needd: Dict[str, bool], head, tail) -> Optional[int]:
    """The lowest layer that still needs a gradient: -1 for a parameter of the `head`, None when nothing but the `tail` does —
    the backward stops as soon as nothing below still needs one (e.g. only visual_projection trainable)."""
    lowest = None
    for n in names:
        if needd[n] and n not in tail:
            li = -1 if n in head else int(n.split(".")[1])
            lowest = li if lowest is None else min(lowest, li)
    return lowest


def _layers_bwd(dx, layers: List[LayerParams], saved_layers, needd: Dict[str, bool], grads, lowest: int, rows: int, B: int, S: int,
                H: int, causal: bool, eps: float, split16=None, varlen=None, alloc=None, on_ready=None, dcls=None,
                act: str = QUICK_GELU):
    """The encoder stack's backward from the top layer down to max(lowest, 0), fp32 or split-fp16 -> dx below the last layer
    run.  `rows`: the token rows of a full-size layer (B S, or Tp with `varlen`, layer_bwd's).  `split16`: the forward's
    Split16Bwd — the full-size data- and weight-gradient GEMMs run on its plan unless a watched parameter has changed since;
    None = the plain fp32 GEMMs (eps: what a forward on the plan left out, §9j).  `dcls` [B, D] (vision): the top layer is the
    pruned one and takes it (last_layer_bwd_cls); `dx` is not read then.  Each layer's gradients go to `grads` under
    "layers.<i>.<field>", are written where `alloc` says and reported to `on_ready` as soon as the layer is done; its saved
    activations are released.  A top layer's incoming dx may be zero in all but one row per sequence (scatter_rows): a
    row-scaled split of an all-zero row gives zero pieces and alpha = 1 (split16_row_exp(0) = 0)."""
    n_layers, bottom = len(layers), max(lowest, 0)
    D = (dx if dcls is None else dcls).shape[1]
    plan = split16.layers if split16 is not None and _VSPLIT16_BWD and split16.fresh() else None
    dystats = plan is not None and _dystats_regime(rows, D, layers[0].fc1_w.shape[0])
    dx_stats = None                                   # the column partials that came with dx (§9g): a value, layer to layer
    for i in range(n_layers - 1, bottom - 1, -1):
        lneed = {f: needd[f"layers.{i}.{f}"] for f in LayerParams.FIELDS}
        lalloc = None if alloc is None else (lambda f, shape, i=i: alloc(f"layers.{i}.{f}", shape))
        sp = plan[i] if plan is not None else None
        # dx is the dY of the layer below's fc2: its producer is asked for the column partials when that weight gradient will
        # take the split path (§9g)
        below = dystats and i - 1 >= bottom and len(saved_layers[i - 1]) > 13
        dxs = below and _split_wgrad_taken(bool(needd[f"layers.{i - 1}.fc2_w"]), plan[i - 1], saved_layers[i - 1][13].get("g"),
                                           D, layers[i - 1].fc1_w.shape[0], rows)
        if dcls is not None and i == n_layers - 1:
            dx, gr, dx_stats = last_layer_bwd_cls(dcls, layers[i], saved_layers[i], B, S, H, lneed, lalloc, sp, dxs, eps=eps, act=act)
        else:
            dx, gr, dx_stats = layer_bwd(dx, layers[i], saved_layers[i], B, S, H, causal, lneed, lalloc, sp, dxs, dystats, eps=eps,
                                         varlen=varlen, dx2_stats=dx_stats, act=act)
        saved_layers[i] = None
        for f, t in gr.items():
            grads[f"layers.{i}.{f}"] = t
        if on_ready is not None:
            on_ready({f"layers.{i}.{f}": t for f, t in gr.items()})
    return dx


def _vision_tail_bwd(p: VisionParams, d_out, cls_tok, mp, rp, pooled, needd: Dict[str, bool], grads, alloc, on_ready):
    """proj_w's gradient, dpooled and the post-LayerNorm backward -> dcls [B, D]; the tail group is reported to `on_ready`."""
    if needd["proj_w"]:
        grads["proj_w"] = ops.gemm(d_out, pooled, ops.LAYOUT_TN, out=_galloc(alloc, "proj_w", tuple(p.proj_w.shape), d_out.device))
    dpooled = ops.gemm(d_out, p.proj_w, ops.LAYOUT_NN)
    dcls, _ = _ln_bwd(dpooled, cls_tok, p.post_w, mp, rp, None, bool(needd["post_w"] or needd["post_b"]), grads, "post_w", "post_b",
                      alloc)
    if on_ready is not None:
        on_ready({n: grads[n] for n in VisionParams.TAIL if grads[n] is not None})
    return dcls


def _patch_split16_wgrad(ps: _PatchSplit, dpatch: torch.Tensor, pw: torch.Tensor, split16) -> torch.Tensor:
    """patch_w's gradient [D, patch_dim] into `pw` for a forward that took the split patch embedding: the
    column-only split of dpatch, then fc2's fused token-major weight-gradient call on it and the saved [hi|lo] columns, whose
    scale is the forward's own record.  Where the backward cannot take it after all — a switch flipped since the forward, no
    Split16Bwd or one that is no longer fresh — the fp32 columns are made again from the saved pixels (the _Remat pattern of
    §9j) and the gradient is the plain fp32 GEMM."""
    D, K = pw.shape
    if (ps.cols16 is not None and split16 is not None and
            patch_split16_taken(True, None, dpatch.shape[0], D, K, backward=True) and split16.fresh()):
        yc, _, col_alpha = ops.split_f16x2_cols(dpatch)
        got = ops.gemm_f16x3_wgrad_tokmajor(yc, ps.cols16, D, K, col_alpha, ps.rec.data_ptr() + 4 * ops.FRONT_SCALE, out=pw)
        if got is None:
            raise RuntimeError("patch-embedding weight gradient: the fused token-major kernel refused a shape its plan accepted")
        return got
    return ops.gemm(dpatch, ops.im2col(ps.pixels, ps.patch), ops.LAYOUT_TN, out=pw)


def _vision_head_bwd(p: VisionParams, dx, emb, m0, r0, cols, B: int, S: int, v, grid, needd: Dict[str, bool], grads, alloc, on_ready,
                     k16=None, split16=None):
    """Below layer 0: the pre-LayerNorm backward, the gradients of pos / class_embedding (a column sum of demb; on another
    `grid` the transpose of the resample, _grid_pos_grad) and of patch_w; the head group is reported to `on_ready`.  `k16` (the
    _Train16 of a 16-bit forward): columns saved in that type give patch_w's gradient on its token-major split-K kernel.
    `split16` (vision_bwd's): a forward that took the split patch embedding (`cols` is a _PatchSplit) gets patch_w's gradient
    from its split columns while that Split16Bwd is fresh."""
    D, dev = v.hidden_size, dx.device
    demb, _ = _ln_bwd(dx, emb, p.pre_w, m0, r0, None, bool(needd["pre_w"] or needd["pre_b"]), grads, "pre_w", "pre_b", alloc)
    if needd["pos"] or needd["class_embedding"]:
        dpos = ops.colsum(demb.view(B, S * D),
                          out=(_galloc(alloc, "pos", (S * D,), dev) if needd["pos"] and grid is None else None))
        if needd["pos"]:
            grads["pos"] = dpos.view(S, D) if grid is None else _grid_pos_grad(dpos, p, v, grid, alloc, dev)
        if needd["class_embedding"]:
            ce = _galloc(alloc, "class_embedding", (D,), dev)
            ce.copy_(dpos[:D])
            grads["class_embedding"] = ce
    if needd["patch_w"]:
        dpatch = ops.vision_assemble_bwd(demb, B, S, D)
        pw = _galloc(alloc, "patch_w", (D, p.patch_w.numel() // D), dev)
        if isinstance(cols, _PatchSplit):         # the forward took the split patch embedding
            grads["patch_w"] = _patch_split16_wgrad(cols, dpatch, pw, split16).view_as(p.patch_w)
        elif cols.dtype != torch.float32:         # token-major split-K weight gradient from the saved 16-bit columns
            got = k16.wgrad_tokmajor(k16.cast(dpatch), cols, out=pw)
            if got is None:
                raise RuntimeError("patch-embedding weight gradient: the token-major 16-bit kernel refused a shape its plan accepted")
            grads["patch_w"] = got.view_as(p.patch_w)
        else:
            grads["patch_w"] = ops.gemm(dpatch, cols, ops.LAYOUT_TN, out=pw).view_as(p.patch_w)
    if on_ready is not None:
        on_ready({n: grads[n] for n in VisionParams.HEAD if grads[n] is not None})


def vision_bwd(p: VisionParams, saved, d_out: torch.Tensor, cfg, need: List[bool], on_ready=None, alloc=None, split16=None):
    """Gradients for VisionParams.tensors() order (None where not needed).  `split16`: the forward's Split16Bwd — the
    full-size data-gradient GEMMs then run on its split-fp16 weights, unless a watched parameter has changed since.  `on_ready(dict name -> grad)` is called as
    soon as a group of gradients is final (the tail, then each layer from the top down, then the head): the
    data-parallel all-reduce of that group starts while the layers below are still being back-propagated.
    `alloc(name, shape)` may name the tensor a parameter gradient is to be written into (see _galloc)."""
    v = cfg
    cols, emb, m0, r0, saved_layers, cls_tok, mp, rp, pooled, pruned, grid = saved
    B = cls_tok.shape[0]
    S, D, H = _grid_seq(v, grid), v.hidden_size, v.num_attention_heads
    names = p.names()
    needd = dict(zip(names, need))
    grads: Dict[str, Optional[torch.Tensor]] = {n: None for n in names}
    dcls = _vision_tail_bwd(p, d_out, cls_tok, mp, rp, pooled, needd, grads, alloc, on_ready)
    lowest = _lowest_needed(names, needd, VisionParams.HEAD, VisionParams.TAIL)
    if lowest is None:
        return [grads[n] for n in names]
    dx = None if pruned else ops.scatter_rows(dcls, None, B, S, D)
    dx = _layers_bwd(dx, p.layers, saved_layers, needd, grads, lowest, B * S, B, S, H, False, v.layer_norm_eps, split16,
                     alloc=alloc, on_ready=on_ready, dcls=dcls if pruned else None, act=hidden_act(v))
    if lowest < 0:
        _vision_head_bwd(p, dx, emb, m0, r0, cols, B, S, v, grid, needd, grads, alloc, on_ready, split16=split16)
    return [grads[n] for n in names]


# --------------------------------------------------------------------------------------------- frozen towers in bf16 / fp16
# Opt-in mixed precision for towers that never receive gradients (the teacher's region encoder, the frozen text
# tower; BASELINE configs c3 / c5): GEMM inputs are bf16 or fp16 (weights converted once, activations converted by the
# producing kernel), accumulation, residual stream, LayerNorm statistics, softmax and biases stay fp32.  The forward
# functions below take the 16-bit type as `dtype` and reach the kernels of that type through _Ops16; the caller keeps one
# weight cache per type (the cache keys do not name the type).


class _Ops16:
    """The forward kernels of one 16-bit type (ops.*_bf16 or ops.*_f16)."""

    def __init__(self, dtype, gemm, layernorm, attention, attention_row, cast, im2col, im2col_rect, attention_varlen,
                 attention_varlen_row):
        self.dtype, self._gemm, self.layernorm, self.attention = dtype, gemm, layernorm, attention
        self.attention_row, self.cast, self.im2col, self.im2col_rect = attention_row, cast, im2col, im2col_rect
        self.attention_varlen, self.attention_varlen_row = attention_varlen, attention_varlen_row    # packed towers, §24

    def gemm(self, a, w, out16: bool = False, **kw):
        """y = epilogue(a w^T), a 16-bit result with `out16`."""
        if self.dtype == torch.bfloat16:
            return self._gemm(a, w, out_bf16=out16, **kw)
        return self._gemm(a, w, out_f16=out16, **kw)


_OPS16 = {
    torch.bfloat16: _Ops16(torch.bfloat16, ops.gemm_bf16, ops.layernorm_fwd_bf16, ops.attention_fwd_bf16,
                           ops.attention_row_fwd_bf16, ops.cast_bf16, ops.im2col_bf16, ops.im2col_rect_bf16,
                           ops.attention_varlen_fwd_bf16, ops.attention_varlen_row_fwd_bf16),
    torch.float16: _Ops16(torch.float16, ops.gemm_f16, ops.layernorm_fwd_f16, ops.attention_fwd_f16,
                          ops.attention_row_fwd_f16, ops.cast_f16, ops.im2col_f16, ops.im2col_rect_f16,
                          ops.attention_varlen_fwd_f16, ops.attention_varlen_row_fwd_f16),
}


# 16-bit MFMA attention core for the packed frozen towers: opt-in, read once at import like _SPLIT16 below.
_PACKED_ATTN16 = os.environ.get("DCLIP_PACKED_ATTN16", "0") != "0"
_ROW16_MAX_S = 512                                               # the one-row kernel's limit (attention_varlen16.hip, ROW_MAXI)


def packed_attn16_route(precision: str, max_S: int, one_row: bool, attn16: Optional[bool] = None) -> str:
    """Which attention core a packed frozen layer takes: "f32" — fp32 q | k | v, ops.attention_varlen*_fwd, and for the 16-bit
    precisions a cast of the context (the only route with the switch off, with precision "fp32" and with the split-fp16 plan);
    "tiled16" — 16-bit q | k | v and k.attention_varlen; "row16" — 16-bit q | k | v and k.attention_varlen_row, the last layer
    of a pooled forward (`one_row`) up to 512 tokens; above that the last layer keeps "f32", as vision_fwd_bf16 does.
    `attn16` None: the module value (DCLIP_PACKED_ATTN16)."""
    on = _PACKED_ATTN16 if attn16 is None else bool(attn16)
    if not on or precision not in ("bf16", "fp16"):
        return "f32"
    if not one_row:
        return "tiled16"
    return "row16" if max_S <= _ROW16_MAX_S else "f32"


def _w16(cache: dict, key: str, w: torch.Tensor, cast=ops.cast_bf16) -> torch.Tensor:
    """bf16 copy of a GEMM weight, PERSISTENT: entry = [tensor, version of `w` it was made from, data pointer of `w`].
    When the optimizer (or load_state_dict) has written `w` since — the version counter is shared with the Parameter a
    detached view came from — the copy is refreshed IN PLACE, so the buffer a captured HIP graph reads stays the one
    that is kept current (and a capture started on a stale entry records the cast: every replay then re-reads the fp32
    masters, HipCLIPModel.invalidate_bf16_of_trainable)."""
    e = cache.get(key)
    src = w.detach().reshape(w.shape[0], -1)
    if e is None:
        e = [cast(src.contiguous()), w._version, w.data_ptr()]
        cache[key] = e
    elif e[1] != w._version or e[2] != w.data_ptr():
        cast(src.contiguous(), out=e[0])
        e[1], e[2] = w._version, w.data_ptr()
    return e[0]


def _layer_fwd_bf16(x, p: LayerParams, c: dict, pre: str, B: int, S: int, H: int, causal: bool, eps: float,
                    dtype=torch.bfloat16, act: str = QUICK_GELU):
    k = _OPS16[dtype]
    ln1 = k.layernorm(x, p.ln1_w, p.ln1_b, eps)
    qkv = k.gemm(ln1, _w16(c, pre + "qkv", p.qkv_w, k.cast), bias=p.qkv_b, out16=True)
    attn = k.attention(qkv, B, S, H, causal)                  # 16-bit q/k/v in, 16-bit context out: no cast pass
    x1 = k.gemm(attn, _w16(c, pre + "out", p.out_w, k.cast), bias=p.out_b, residual=x)
    ln2 = k.layernorm(x1, p.ln2_w, p.ln2_b, eps)
    g = _fc1_act16(k, ln2, _w16(c, pre + "fc1", p.fc1_w, k.cast), p.fc1_b, act)
    return k.gemm(g, _w16(c, pre + "fc2", p.fc2_w, k.cast), bias=p.fc2_b, residual=x1)


def vision_fwd_bf16(p: VisionParams, pixel_values: torch.Tensor, cfg, cache: dict, dtype=torch.bfloat16,
                    grid=None) -> torch.Tensor:
    """Frozen get_image_features with 16-bit GEMM inputs (`dtype` bf16 or fp16); `cache` keeps the converted weights
    between calls (one cache per dtype).  `grid`: as in vision_fwd."""
    v = cfg
    k = _OPS16[dtype]
    B = pixel_values.shape[0]
    S, D, H = _grid_seq(v, grid), v.hidden_size, v.num_attention_heads
    if grid is None:
        pos = p.pos
        cols = (k.im2col(pixel_values, v.patch_size) if v.patch_size % 4 == 0              # one pass: gather + round
                else k.cast(ops.im2col(pixel_values, v.patch_size)))
    else:
        pos = _grid_front(p, pixel_values, v, grid)
        cols = (k.im2col_rect(pixel_values, v.patch_size) if v.patch_size % 4 == 0
                else k.cast(ops.im2col_rect(pixel_values, v.patch_size)))
    patch = k.gemm(cols, _w16(cache, "patch", p.patch_w, k.cast), k=v.patch_dim)
    x, _, _ = ops.layernorm_fwd(ops.vision_assemble_fwd(patch, p.class_embedding, pos, B, S, D), p.pre_w, p.pre_b,
                                v.layer_norm_eps, save_stats=False)
    for li, lp in enumerate(p.layers[:-1]):
        x = _layer_fwd_bf16(x, lp, cache, f"v{li}.", B, S, H, False, v.layer_norm_eps, dtype, hidden_act(v))
    lp, pre = p.layers[-1], f"v{len(p.layers) - 1}."
    # last layer on the CLS rows only (see last_layer_fwd_cls)
    ln1 = k.layernorm(x, lp.ln1_w, lp.ln1_b, v.layer_norm_eps)
    if S <= 512 and os.environ.get("DCLIP_BF16_ROW_ATTN", "1") != "0":
        # q | k | v written as 16-bit (half the bytes of the 2304-wide projection's output), one-row kernel on them
        qkv = k.gemm(ln1, _w16(cache, pre + "qkv", lp.qkv_w, k.cast), bias=lp.qkv_b, out16=True)
        attn16 = k.attention_row(qkv, None, B, S, H)
    else:
        qkv = k.gemm(ln1, _w16(cache, pre + "qkv", lp.qkv_w, k.cast), bias=lp.qkv_b)
        attn16 = k.cast(ops.attention_cls_fwd(qkv, B, S, H)[0])
    x1 = k.gemm(attn16, _w16(cache, pre + "out", lp.out_w, k.cast), bias=lp.out_b,
                residual=ops.gather_rows(x, None, B, S, D))
    ln2 = k.layernorm(x1, lp.ln2_w, lp.ln2_b, v.layer_norm_eps)
    g = _fc1_act16(k, ln2, _w16(cache, pre + "fc1", lp.fc1_w, k.cast), lp.fc1_b, hidden_act(v))
    cls_tok = k.gemm(g, _w16(cache, pre + "fc2", lp.fc2_w, k.cast), bias=lp.fc2_b, residual=x1)
    pooled, _, _ = ops.layernorm_fwd(cls_tok, p.post_w, p.post_b, v.layer_norm_eps, save_stats=False)
    return ops.gemm(pooled, p.proj_w, ops.LAYOUT_NT)          # [B,D] x [P,D]: tiny, kept in exact fp32


# --------------------------------------------------------------------------------------------- packed frozen forward
# The frozen tower over N crops of DIFFERENT sizes in one pass (the full-resolution teacher): the token rows of
# all crops lie back to back (crop n in rows cu_seqlens[n] .. cu_seqlens[n+1]-1, T rows in all).  LayerNorm, the four GEMMs and
# their epilogues are row-wise and run at M = T as they are; the assemble step, the attention core and the CLS gather have
# ragged forms (ops.vision_assemble_varlen, ops.attention_varlen_fwd, ops.gather_rows_at).  Forward only.

def vision_fwd_packed(p: VisionParams, cols: torch.Tensor, grids: torch.Tensor, cu_seqlens: torch.Tensor,
                      cls_rows: torch.Tensor, max_S: int, cfg, precision: str = "fp32", cache: Optional[dict] = None,
                      attn16: Optional[bool] = None) -> torch.Tensor:
    """cols [T - N, 3 p p] fp32 (ops.patches_from_boxes_u8), grids [N,2], cu_seqlens [N+1], cls_rows [N] (= cu_seqlens[:-1]),
    int32 on the device -> [N, P].  The schedule of vision_fwd without `save`: the last layer runs its out-projection and MLP on
    the N CLS rows only.  "bf16" / "fp16": 16-bit GEMM inputs with the persistent weight copies of `cache` (the model's cache of
    that type, as vision_fwd_bf16); the qkv projection writes fp32 for the fp32 packed attention core and the context is cast,
    or with `attn16` (packed_attn16_route) q | k | v and the context stay 16-bit around the packed MFMA core.
    "fp32-split16" (`cache`: the model's frozen split cache): the schedule of vision_fwd_frozen_split16 — layers
    0 .. L-2 on split-fp16 operands with the context written split by the packed attention entry, the last layer's full-size qkv
    projection too, its CLS-row steps in fp32; the "fp32" schedule, bit for bit, when the guard trips.  `attn16` has no effect."""
    v = cfg
    D, H, eps, act = v.hidden_size, v.num_attention_heads, v.layer_norm_eps, hidden_act(v)
    if not p.layers:
        raise ValueError("vision_fwd_packed: the tower has no encoder layer")
    if precision in ("fp32", "fp32-split16"):
        if precision == "fp32-split16" and cache is None:
            raise ValueError("vision_fwd_packed: precision 'fp32-split16' needs the model's frozen split cache")
        plan = _vision_frozen_split16_plan(p.layers, v, cache) if precision == "fp32-split16" else None
        patch = ops.gemm(cols, p.patch_w.view(D, -1), ops.LAYOUT_NT)
        emb = ops.vision_assemble_varlen(patch, p.class_embedding, p.pos, grids, cu_seqlens, v.grid)
        del patch
        x, _, _ = ops.layernorm_fwd(emb, p.pre_w, p.pre_b, eps, save_stats=False)
        if plan is not None:
            pc = _layer_pieces(x.shape[0], D, v.intermediate_size, _SPLIT16_FC1_EPI)
            ctx3 = _packed_ctx3(cu_seqlens, max_S, H, False, True)
            for lp, ent in zip(p.layers[:-1], plan[:-1]):
                x = _frozen_split16_layer(x, lp, ent, pc, eps, ctx3)
            x = _frozen_split16_last_cls(x, p.layers[-1], plan[-1], eps,
                                         lambda qkv: ops.attention_varlen_fwd(qkv, cu_seqlens, max_S, H, cls_only=True),
                                         lambda xx: ops.gather_rows_at(xx, cls_rows))
        else:
            for li, lp in enumerate(p.layers):
                last = li == len(p.layers) - 1
                ln1, _, _ = ops.layernorm_fwd(x, lp.ln1_w, lp.ln1_b, eps, save_stats=False)
                qkv = ops.gemm(ln1, lp.qkv_w, ops.LAYOUT_NT, bias=lp.qkv_b)
                attn = ops.attention_varlen_fwd(qkv, cu_seqlens, max_S, H, cls_only=last)
                x1 = ops.gemm(attn, lp.out_w, ops.LAYOUT_NT, bias=lp.out_b, residual=ops.gather_rows_at(x, cls_rows) if last else x)
                ln2, _, _ = ops.layernorm_fwd(x1, lp.ln2_w, lp.ln2_b, eps, save_stats=False)
                g, _ = _fc1_act_f32(ln2, lp, act)
                x = ops.gemm(g, lp.fc2_w, ops.LAYOUT_NT, bias=lp.fc2_b, residual=x1)    # the last layer: [N, D], the CLS rows
    else:
        if precision not in ("bf16", "fp16") or cache is None:
            raise ValueError(f"vision_fwd_packed: precision {precision!r} (16-bit precisions need the model's weight cache)")
        k = _OPS16[torch.bfloat16 if precision == "bf16" else torch.float16]
        patch = k.gemm(k.cast(cols), _w16(cache, "patch", p.patch_w, k.cast), k=v.patch_dim)
        emb = ops.vision_assemble_varlen(patch, p.class_embedding, p.pos, grids, cu_seqlens, v.grid)
        del patch
        x, _, _ = ops.layernorm_fwd(emb, p.pre_w, p.pre_b, eps, save_stats=False)
        for li, lp in enumerate(p.layers):
            last, pre = li == len(p.layers) - 1, f"v{li}."
            ln1 = k.layernorm(x, lp.ln1_w, lp.ln1_b, eps)
            route = packed_attn16_route(precision, max_S, last, attn16)
            if route == "f32":
                qkv = k.gemm(ln1, _w16(cache, pre + "qkv", lp.qkv_w, k.cast), bias=lp.qkv_b)                 # fp32 q | k | v
                attn = k.cast(ops.attention_varlen_fwd(qkv, cu_seqlens, max_S, H, cls_only=last))
            else:
                qkv = k.gemm(ln1, _w16(cache, pre + "qkv", lp.qkv_w, k.cast), bias=lp.qkv_b, out16=True)
                attn = (k.attention_varlen_row(qkv, cu_seqlens, max_S, H, last=False) if route == "row16"
                        else k.attention_varlen(qkv, cu_seqlens, max_S, H, False))
            x1 = k.gemm(attn, _w16(cache, pre + "out", lp.out_w, k.cast), bias=lp.out_b,
                        residual=ops.gather_rows_at(x, cls_rows) if last else x)
            ln2 = k.layernorm(x1, lp.ln2_w, lp.ln2_b, eps)
            g = _fc1_act16(k, ln2, _w16(cache, pre + "fc1", lp.fc1_w, k.cast), lp.fc1_b, act)
            x = k.gemm(g, _w16(cache, pre + "fc2", lp.fc2_w, k.cast), bias=lp.fc2_b, residual=x1)
    pooled, _, _ = ops.layernorm_fwd(x, p.post_w, p.post_b, eps, save_stats=False)
    return ops.gemm(pooled, p.proj_w, ops.LAYOUT_NT)


# --------------------------------------------------------------------------------------------- bf16 TRAINING (vision)
# The student's vision tower with bf16 GEMM inputs in forward, dgrad AND wgrad (BASELINE configs c3 / c5 quote the step
# in bf16; opt-in `precision="bf16"` with gradients enabled).  fp32 master weights (bf16 copies W and W^T are rebuilt
# when the optimizer has stepped), fp32 accumulation, fp32 residual stream / LayerNorm statistics / softmax; the
# attention core runs on the bf16 MFMAs for sequences up to 64 tokens (attention_bf16.hip; the fp32 kernels above that).
# The weight-gradient product dW[out,in] = dY^T X comes from the token-major split-K kernel on the operands as the backward
# has them (for shapes it declines: the C = A W^T kernel on dY^T, X^T written by ops.transpose_bf16).  The patch embedding is
# a bf16 GEMM pair too where that kernel takes its shape (_patch_embed_bf16); the pooled LayerNorm and the projection stay
# fp32; every encoder layer is run at full size (the CLS-row pruning of the fp32 schedule would keep a full-size fp32 qkv
# projection).

class _Train16:
    """The training-path kernels of one 16-bit type: ops.*_bf16, or their fp16 twins with IEEE rounding (ops.*_f16*,
    student_precision="fp16").  `plan_tokmajor` / `io16_pair` are the library plan entry and the fp32-arithmetic
    attention pair of DCLIP_BF16_ATTN_MFMA=0 (bf16 only: None for fp16, which always takes the MFMA pair)."""

    def __init__(self, dtype, gemm, cast, layernorm_stats, transpose, wgrad, wgrad_tokmajor, colsum, rowsum, attention_lse,
                 attention_bwd, mt_weights, im2col, im2col_rect, plan_tokmajor, io16_pair):
        self.dtype, self._gemm, self.cast, self._layernorm_stats = dtype, gemm, cast, layernorm_stats
        self.transpose, self.wgrad, self.wgrad_tokmajor, self.colsum, self.rowsum = transpose, wgrad, wgrad_tokmajor, colsum, rowsum
        self.attention_lse, self.attention_bwd, self.mt_weights, self.im2col = attention_lse, attention_bwd, mt_weights, im2col
        self.im2col_rect, self.plan_tokmajor, self.io16_pair = im2col_rect, plan_tokmajor, io16_pair

    def gemm(self, a, w, out16: bool = False, **kw):
        if self.dtype == torch.bfloat16:
            return self._gemm(a, w, out_bf16=out16, **kw)
        return self._gemm(a, w, out_f16=out16, **kw)

    def layernorm_stats(self, x, gamma, beta, eps):
        if self.dtype == torch.bfloat16:
            return self._layernorm_stats(x, gamma, beta, eps, save_stats=True)
        return self._layernorm_stats(x, gamma, beta, eps)


_TRAIN16 = {
    torch.bfloat16: _Train16(torch.bfloat16, ops.gemm_bf16, ops.cast_bf16, ops.layernorm_fwd_bf16, ops.transpose_bf16,
                             ops.gemm_bf16_wgrad, ops.gemm_bf16_wgrad_tokmajor, ops.colsum_bf16, ops.rowsum_bf16,
                             ops.attention_fwd_bf16_lse, ops.attention_bwd_bf16, ops.mt_weights_bf16, ops.im2col_bf16,
                             ops.im2col_rect_bf16, "dclip_gemm_bf16_wgrad_tokmajor_plan",
                             (ops.attention_fwd_io16, ops.attention_bwd_io16)),
    torch.float16: _Train16(torch.float16, ops.gemm_f16_train, ops.cast_f16_ieee, ops.layernorm_fwd_f16_stats, ops.transpose_f16,
                            ops.gemm_f16_wgrad, ops.gemm_f16_wgrad_tokmajor, ops.colsum_f16, ops.rowsum_f16,
                            ops.attention_fwd_f16_lse, ops.attention_bwd_f16, ops.mt_weights_f16, ops.im2col_f16,
                            ops.im2col_rect_f16, "dclip_gemm_f16_wgrad_tokmajor_plan", None),
}


def _w16t(cache: dict, key: str, w: torch.Tensor, dtype=torch.bfloat16) -> torch.Tensor:
    """16-bit W^T [in, ld >= out] of an nn.Linear weight [out, in]: the `W` operand of the dgrad GEMM dX = dY (W^T)^T."""
    transpose = _TRAIN16[dtype].transpose
    e = cache.get(key + ".T")
    src = w.detach().reshape(w.shape[0], -1)
    if e is None:
        e = [transpose(src.contiguous()), w._version, w.data_ptr()]
        cache[key + ".T"] = e
    elif e[1] != w._version or e[2] != w.data_ptr():
        transpose(src.contiguous(), out=e[0])
        e[1], e[2] = w._version, w.data_ptr()
    return e[0]


_TRAIN_WEIGHTS = (("qkv", "qkv_w"), ("out", "out_w"), ("fc1", "fc1_w"), ("fc2", "fc2_w"))


def refresh_train_weights(cache: dict, layers: List[LayerParams], prefix: str = "v", dtype=torch.bfloat16) -> None:
    """Bring the bf16 copies W and W^T of every encoder-layer GEMM weight of a TRAINING tower up to date before its
    forward — in ONE launch (ops.mt_weights_bf16) when, as after every optimizer step, all of them are stale: the
    per-weight path is 48 casts + 48 transposes per step for ViT-B.  The record table lives on the device next to the
    persistent copies (uploaded once, so the launch is capturable in a HIP graph).  `dtype`: the 16-bit type of the copies
    (one cache per type)."""
    t16 = _TRAIN16[dtype]
    stale = []
    for li, lp in enumerate(layers):
        for short, field in _TRAIN_WEIGHTS:
            w = getattr(lp, field)
            for key in (f"{prefix}{li}.{short}", f"{prefix}{li}.{short}.T"):
                e = cache.get(key)
                if e is None or e[1] != w._version or e[2] != w.data_ptr():
                    stale.append((key, w))
    if not stale:
        return
    tables = cache.setdefault("__mt_tables__", {})
    keys = tuple(k for k, _ in stale)
    tab = tables.get(keys)
    if tab is not None and all(cache[k][2] == w.data_ptr() for k, w in stale):
        t16.mt_weights(tab["dev"], tab["n"], tab["tiles"])
        for k, w in stale:
            cache[k][1] = w._version
        return
    # first time this set is stale: the per-weight kernels allocate / refresh the copies ...
    for key, w in stale:
        if key.endswith(".T"):
            _w16t(cache, key[:-2], w, dtype)
        else:
            _w16(cache, key, w, t16.cast)
    # ... and a table for exactly this set (all weights after an optimizer step; the trainable subset under a freeze rule)
    # is built for the following steps — not while a stream is capturing: the upload is a synchronous copy
    if torch.cuda.is_current_stream_capturing():
        return
    recs = {}
    for key, w in stale:
        base = key[:-2] if key.endswith(".T") else key
        r = recs.setdefault(base, [w, None, None])
        r[2 if key.endswith(".T") else 1] = cache[key][0]
    dev, n, tiles = ops.mt_weights_table([tuple(r) for r in recs.values()], dtype)
    tables[keys] = {"dev": dev, "n": n, "tiles": tiles}


def _attention_io16(M: int, S: int, D: int, I: int, dtype=torch.bfloat16) -> bool:
    """Short sequences on the token-major backward schedule keep q/k/v, the attention output and their gradients in bf16
    between the GEMMs and the attention kernels: the qkv projection writes bf16, no cast launches either side of the
    attention.  DCLIP_BF16_ATTN_IO16=0: fp32 attention I/O (casts) instead."""
    return S <= 64 and _tokmajor_wgrads(M, D, I, dtype) and os.environ.get("DCLIP_BF16_ATTN_IO16", "1") != "0"


def _attention_mfma16(dtype=torch.bfloat16) -> bool:
    """Which kernels serve the bf16-I/O attention of the training student: the bf16 MFMA pair (ops.attention_fwd_bf16_lse /
    attention_bwd_bf16: P and dS rounded to bf16 for the products they feed — the default) or, DCLIP_BF16_ATTN_MFMA=0, the
    fp32-arithmetic kernels with bf16 loads and stores (ops.attention_*_io16).  fp16 always takes its MFMA pair."""
    return dtype != torch.bfloat16 or os.environ.get("DCLIP_BF16_ATTN_MFMA", "1") != "0"


def layer_fwd_bf16_train(x, p: LayerParams, c: dict, pre: str, B: int, S: int, H: int, causal: bool, eps: float,
                         dtype=torch.bfloat16):
    k = _TRAIN16[dtype]
    ln1, m1, r1 = k.layernorm_stats(x, p.ln1_w, p.ln1_b, eps)
    if _attention_io16(x.shape[0], S, x.shape[1], p.fc1_w.shape[0], dtype):
        qkv = k.gemm(ln1, _w16(c, pre + "qkv", p.qkv_w, k.cast), bias=p.qkv_b, out16=True)
        attn16, lse = (k.attention_lse if _attention_mfma16(dtype) else k.io16_pair[0])(qkv, B, S, H, causal)
        attn = None
    else:
        qkv = k.gemm(ln1, _w16(c, pre + "qkv", p.qkv_w, k.cast), bias=p.qkv_b)        # fp32 out: the attention core is fp32
        attn, lse = ops.attention_fwd(qkv, B, S, H, causal)
        attn16 = k.cast(attn)
    x1 = k.gemm(attn16, _w16(c, pre + "out", p.out_w, k.cast), bias=p.out_b, residual=x)
    ln2, m2, r2 = k.layernorm_stats(x1, p.ln2_w, p.ln2_b, eps)
    g16, h16 = k.gemm(ln2, _w16(c, pre + "fc1", p.fc1_w, k.cast), bias=p.fc1_b, gelu=True, out16=True, save_preact=True)
    x2 = k.gemm(g16, _w16(c, pre + "fc2", p.fc2_w, k.cast), bias=p.fc2_b, residual=x1)
    return x2, (x, m1, r1, ln1, qkv, attn, attn16, lse, x1, m2, r2, ln2, h16, g16)


_TOKMAJOR_PLAN: Dict[tuple, bool] = {}


def _tokmajor_wgrads(M: int, D: int, I: int, dtype=torch.bfloat16) -> bool:
    """Can the four weight gradients of a layer take the token-major form (no transposes)?  One answer per layer so that
    the backward below has two straight schedules; decided once per (M, D, I) (four plan calls + an environment lookup
    per layer per backward otherwise).  DCLIP_BF16_WGRAD_TN=0, read at the first use, forces the transposing schedule."""
    key = (M, D, I, dtype)
    hit = _TOKMAJOR_PLAN.get(key)
    if hit is None:
        if os.environ.get("DCLIP_BF16_WGRAD_TN", "1") == "0":
            hit = False
        else:
            plan = getattr(_lib.load(), _TRAIN16[dtype].plan_tokmajor)
            hit = all(plan(m, n, M) > 0 for m, n in ((D, I), (I, D), (D, D), (3 * D, D)))
        _TOKMAJOR_PLAN[key] = hit
    return hit


_WGRAD_STREAMS: Dict[int, "torch.cuda.Stream"] = {}


class _SideWgrads:
    """The four weight-gradient GEMMs of a layer on a SECOND stream beside the data-gradient chain (DCLIP_BF16_WGRAD_STREAM=0
    keeps them on the main stream).  A bf16 ping-pong GEMM takes a whole CU per workgroup, and the student's data-gradient
    GEMMs have 150 tiles for 256 CUs: the weight gradient of the same dY (independent of everything downstream) takes the
    idle CUs — same box, alternating: c3 43.83 -> 43.28 ms, the c2-shaped bf16 step under graph replay 16.78 -> 16.48 ms,
    results bit-identical.  (For the fp32 GEMMs, three workgroups per CU sharing the matrix pipe, the same idea measured
    SLOWER in round 2: there is no idle CU to take.)  Fork: the side stream waits for the main stream (dY is ready); join at the end of the layer.  Operands
    are kept alive until the join (the caching allocator would hand a freed block to the main stream while the side
    stream still reads it); scratch comes from a workspace lane of its own."""

    def __init__(self, dev):
        self.on = os.environ.get("DCLIP_BF16_WGRAD_STREAM", "1") != "0" and dev.type == "cuda"
        self.keep = []
        if self.on:
            self.main = torch.cuda.current_stream(dev)
            self.side = _WGRAD_STREAMS.setdefault(dev.index, torch.cuda.Stream(device=dev))

    def run(self, fn, *operands):
        if not self.on:
            return fn()
        self.keep.extend(operands)
        self.side.wait_stream(self.main)
        with torch.cuda.stream(self.side), ops.workspace_lane(2):
            return fn()

    def join(self):
        if self.on:
            self.main.wait_stream(self.side)
            self.keep.clear()


def layer_bwd_bf16_tokmajor(dx2, p: LayerParams, c: dict, pre: str, saved, B: int, S: int, H: int, causal: bool,
                            need: Dict[str, bool], alloc=None, dx2_16=None, fc2_b=None, below_fc2_b=None, want_dx16=False,
                            dtype=torch.bfloat16):
    """layer_bwd_bf16 with the weight gradients read from the operands as they lie — dW = dY^T X on the token-major form of
    the ping-pong GEMM (ops.gemm_bf16_wgrad_tokmajor): the saved bf16 activations are used as they are, no transposed
    copies are written, and the bf16 copies of the fp32 gradients come out of the kernels that PRODUCE those gradients:
      dx2_16   bf16 copy of the incoming dx2 (LayerNorm1's backward of the layer above wrote it; None: cast here);
      fc2_b    this layer's fc2 bias gradient = column sums of dx2, already reduced by that same LayerNorm backward;
      below_fc2_b  where THIS layer's LayerNorm1 backward leaves the column sums of its dx (the layer below's fc2_b);
      want_dx16    ... and whether it writes the bf16 copy of dx for the layer below.
    Returns (dx, dx16 or None, grads)."""
    k = _TRAIN16[dtype]
    x, m1, r1, ln1, qkv, attn, attn16, lse, x1, m2, r2, ln2, h16, g16 = saved
    D = x.shape[1]
    I = g16.shape[1]
    dev = x.device
    gr: Dict[str, torch.Tensor] = {}
    wg = _SideWgrads(dev)
    # ---- fc2
    if dx2_16 is None:
        dx2_16 = k.cast(dx2)
    if need.get("fc2_w"):
        o_ = _galloc(alloc, "fc2_w", (D, I), dev)
        gr["fc2_w"] = wg.run(lambda a_=dx2_16, b_=g16: k.wgrad_tokmajor(a_, b_, out=o_), dx2_16, g16)
    if need.get("fc2_b"):
        gr["fc2_b"] = fc2_b if fc2_b is not None else ops.colsum(dx2, out=_galloc(alloc, "fc2_b", (D,), dev))
    dh16 = k.gemm(dx2_16, _w16t(c, pre + "fc2", p.fc2_w, dtype), k=D, dgelu_of=h16, out16=True)         # [M, I]
    del dx2_16
    # ---- fc1
    if need.get("fc1_w"):
        o1_ = _galloc(alloc, "fc1_w", (I, D), dev)
        gr["fc1_w"] = wg.run(lambda a_=dh16, b_=ln2: k.wgrad_tokmajor(a_, b_, out=o1_), dh16, ln2)
    if need.get("fc1_b"):
        gr["fc1_b"] = k.colsum(dh16, out=_galloc(alloc, "fc1_b", (I,), dev))
    dln2 = k.gemm(dh16, _w16t(c, pre + "fc1", p.fc1_w, dtype), k=dh16.shape[1])                          # [M, D] fp32
    del dh16
    # LayerNorm2 backward: dx1 (+ the skip connection's dx2), its bf16 copy, and out_proj's bias gradient = colsum(dx1)
    want_ln2 = bool(need.get("ln2_w") or need.get("ln2_b"))
    out_b = _galloc(alloc, "out_b", (D,), dev) if need.get("out_b") else None
    dg = _galloc(alloc, "ln2_w", (D,), dev) if want_ln2 else None
    db = _galloc(alloc, "ln2_b", (D,), dev) if want_ln2 else None
    dx1, dg, db, dx1_16 = ops.layernorm_bwd(dln2, x1, p.ln2_w, m2, r2, dresidual=dx2, dgamma=dg, dbeta=db,
                                            need_param_grads=want_ln2, want_bf16=True, dx_colsum=out_b, dtype16=dtype)
    if want_ln2:
        gr["ln2_w"], gr["ln2_b"] = dg, db
    if out_b is not None:
        gr["out_b"] = out_b
    # ---- out_proj
    if need.get("out_w"):
        o2_ = _galloc(alloc, "out_w", (D, D), dev)
        gr["out_w"] = wg.run(lambda a_=dx1_16, b_=attn16: k.wgrad_tokmajor(a_, b_, out=o2_), dx1_16, attn16)
    if qkv.dtype != torch.float32:           # 16-bit I/O attention: dO arrives as 16-bit, dq / dk / dv leave as 16-bit
        dattn16 = k.gemm(dx1_16, _w16t(c, pre + "out", p.out_w, dtype), k=D, out16=True)
        del dx1_16
        dqkv16 = (k.attention_bwd if _attention_mfma16(dtype) else k.io16_pair[1])(qkv, attn16, dattn16, lse, B, S, H, causal)
        del dattn16
        if need.get("qkv_b"):
            gr["qkv_b"] = k.colsum(dqkv16, out=_galloc(alloc, "qkv_b", (3 * D,), dev))
    else:
        dattn = k.gemm(dx1_16, _w16t(c, pre + "out", p.out_w, dtype), k=D)                               # [M, D] fp32
        del dx1_16
        dqkv = ops.attention_bwd(qkv, attn, dattn, lse, B, S, H, causal)                                 # fp32 [M, 3D]
        dqkv16 = k.cast(dqkv)
        if need.get("qkv_b"):
            gr["qkv_b"] = ops.colsum(dqkv, out=_galloc(alloc, "qkv_b", (3 * D,), dev))
        del dqkv
    # ---- qkv projection
    if need.get("qkv_w"):
        o3_ = _galloc(alloc, "qkv_w", (3 * D, D), dev)
        gr["qkv_w"] = wg.run(lambda a_=dqkv16, b_=ln1: k.wgrad_tokmajor(a_, b_, out=o3_), dqkv16, ln1)
    dln1 = k.gemm(dqkv16, _w16t(c, pre + "qkv", p.qkv_w, dtype), k=3 * D)
    del dqkv16
    want_ln1 = bool(need.get("ln1_w") or need.get("ln1_b"))
    dg = _galloc(alloc, "ln1_w", (D,), dev) if want_ln1 else None
    db = _galloc(alloc, "ln1_b", (D,), dev) if want_ln1 else None
    res = ops.layernorm_bwd(dln1, x, p.ln1_w, m1, r1, dresidual=dx1, dgamma=dg, dbeta=db, need_param_grads=want_ln1,
                            want_bf16=want_dx16, dx_colsum=below_fc2_b, dtype16=dtype)
    dx, dg, db = res[0], res[1], res[2]
    if want_ln1:
        gr["ln1_w"], gr["ln1_b"] = dg, db
    wg.join()                                  # the weight gradients are final before the caller reports / reduces them
    return dx, (res[3] if want_dx16 else None), gr


def layer_bwd_bf16(dx2, p: LayerParams, c: dict, pre: str, saved, B: int, S: int, H: int, causal: bool, need: Dict[str, bool],
                   alloc=None, dx2_16=None, fc2_b=None, below_fc2_b=None, want_dx16=False, dtype=torch.bfloat16):
    """Backward of layer_fwd_bf16_train -> (dx, dx16 or None, grads).  `alloc(field, shape)`: see _galloc — under data
    parallelism every parameter gradient (split-K weight gradients, bias column sums, LayerNorm dγ/dβ) is written straight
    into its bucket slice.  dx2_16 / fc2_b / below_fc2_b / want_dx16: see layer_bwd_bf16_tokmajor (the transposing
    schedule below ignores them, except that it fills below_fc2_b so the caller's bookkeeping holds).  `dtype`: the 16-bit
    type of the layer's forward (layer_fwd_bf16_train)."""
    k = _TRAIN16[dtype]
    x, m1, r1, ln1, qkv, attn, attn16, lse, x1, m2, r2, ln2, h16, g16 = saved
    M = x.shape[0]
    D = x.shape[1]
    I = g16.shape[1]
    dev = x.device
    if _tokmajor_wgrads(M, D, I, dtype):
        return layer_bwd_bf16_tokmajor(dx2, p, c, pre, saved, B, S, H, causal, need, alloc, dx2_16, fc2_b, below_fc2_b,
                                       want_dx16, dtype)
    gr: Dict[str, torch.Tensor] = {}
    # ---- fc2
    dx2T, dx2_16 = k.transpose(dx2, want_copy=True)
    if need.get("fc2_w"):
        gr["fc2_w"] = k.wgrad(dx2T, k.transpose(g16), M, out=_galloc(alloc, "fc2_w", (D, I), dev))
    if need.get("fc2_b"):
        gr["fc2_b"] = fc2_b if fc2_b is not None else ops.colsum(dx2, out=_galloc(alloc, "fc2_b", (D,), dev))
    dh16 = k.gemm(dx2_16, _w16t(c, pre + "fc2", p.fc2_w, dtype), k=D, dgelu_of=h16, out16=True)         # [M, I]
    del dx2T, dx2_16
    # ---- fc1
    dhT = k.transpose(dh16)
    if need.get("fc1_w"):
        gr["fc1_w"] = k.wgrad(dhT, k.transpose(ln2), M, out=_galloc(alloc, "fc1_w", (I, D), dev))
    if need.get("fc1_b"):
        gr["fc1_b"] = k.rowsum(dhT, M, out=_galloc(alloc, "fc1_b", (I,), dev))
    dln2 = k.gemm(dh16, _w16t(c, pre + "fc1", p.fc1_w, dtype), k=dh16.shape[1])                          # [M, D] fp32
    del dh16, dhT
    dx1, _ = _ln_bwd(dln2, x1, p.ln2_w, m2, r2, dx2, bool(need.get("ln2_w") or need.get("ln2_b")), gr, "ln2_w", "ln2_b", alloc)
    # ---- out_proj
    dx1T, dx1_16 = k.transpose(dx1, want_copy=True)
    if need.get("out_w"):
        gr["out_w"] = k.wgrad(dx1T, k.transpose(attn16), M, out=_galloc(alloc, "out_w", (D, D), dev))
    if need.get("out_b"):
        gr["out_b"] = ops.colsum(dx1, out=_galloc(alloc, "out_b", (D,), dev))
    dattn = k.gemm(dx1_16, _w16t(c, pre + "out", p.out_w, dtype), k=D)                                   # [M, D] fp32
    del dx1T, dx1_16
    dqkv = ops.attention_bwd(qkv, attn, dattn, lse, B, S, H, causal)                                     # fp32 [M, 3D]
    # ---- qkv projection
    dqkvT, dqkv16 = k.transpose(dqkv, want_copy=True)
    if need.get("qkv_w"):
        gr["qkv_w"] = k.wgrad(dqkvT, k.transpose(ln1), M, out=_galloc(alloc, "qkv_w", (3 * D, D), dev))
    if need.get("qkv_b"):
        gr["qkv_b"] = ops.colsum(dqkv, out=_galloc(alloc, "qkv_b", (3 * D,), dev))
    dln1 = k.gemm(dqkv16, _w16t(c, pre + "qkv", p.qkv_w, dtype), k=3 * D)
    del dqkv, dqkvT, dqkv16
    dx, _ = _ln_bwd(dln1, x, p.ln1_w, m1, r1, dx1, bool(need.get("ln1_w") or need.get("ln1_b")), gr, "ln1_w", "ln1_b", alloc)
    if below_fc2_b is not None:
        ops.colsum(dx, out=below_fc2_b)
    return dx, None, gr


_PATCH_BF16_PLAN: Dict[tuple, bool] = {}


def _patch_embed_bf16(v, rows: int, dtype=torch.bfloat16) -> bool:
    """Does the patch embedding of the TRAINING tower (the convolution as a GEMM: [rows = images x patches][3 p p] x
    [D][3 p p]^T, and its weight gradient) run on the bf16 MFMAs like the encoder layers?  Yes when the one-pass bf16
    im2col and the token-major weight-gradient kernel both apply to the shape (`DCLIP_BF16_PATCH=0`: keep it fp32, as
    rounds 2-3 had it: 0.44 + 0.43 ms of fp32 GEMM per step at 256 images against 0.05 + 0.07)."""
    key = (v.hidden_size, v.patch_dim, v.patch_size, rows, dtype)
    hit = _PATCH_BF16_PLAN.get(key)
    if hit is None:
        hit = (os.environ.get("DCLIP_BF16_PATCH", "1") != "0" and v.patch_size % 4 == 0 and v.patch_dim % 64 == 0
               and getattr(_lib.load(), _TRAIN16[dtype].plan_tokmajor)(v.hidden_size, v.patch_dim, rows) > 0)
        _PATCH_BF16_PLAN[key] = hit
    return hit


def refuse_train16(cfg) -> None:
    """16-bit TRAINING of a "gelu" tower is not built: its fc1 / fc2 GEMMs carry quick-GELU and its derivative in their epilogues
    (layer_fwd_bf16_train, layer_bwd_bf16*).  Raised before anything is launched; the frozen 16-bit forward of the same model works."""
    if hidden_act(cfg) != QUICK_GELU:
        raise NotImplementedError(f"hidden_act={hidden_act(cfg)!r}: 16-bit training (precision 'bf16' / 'fp16-mixed' with gradients, "
                                  "student_precision 'bf16' / 'fp16') is built for hidden_act='quick_gelu' only; train this tower "
                                  "at precision 'fp32', or use the 16-bit precisions under torch.no_grad()")


def vision_fwd_bf16_train(p: VisionParams, pixel_values: torch.Tensor, cfg, cache: dict, dtype=torch.bfloat16, grid=None):
    """get_image_features with gradients, 16-bit GEMM inputs (`dtype` bf16, or fp16 with IEEE rounding) in the patch
    embedding and the encoder layers; `cache` holds the weight copies of that type.  `grid`: as in vision_fwd."""
    v = cfg
    refuse_train16(v)
    k = _TRAIN16[dtype]
    B = pixel_values.shape[0]
    S, D, H = _grid_seq(v, grid), v.hidden_size, v.num_attention_heads
    pos = p.pos if grid is None else _grid_front(p, pixel_values, v, grid)
    if _patch_embed_bf16(v, B * (S - 1), dtype):
        # one pass: gather + round; kept for the wgrad
        cols = (k.im2col if grid is None else k.im2col_rect)(pixel_values, v.patch_size)
        patch = k.gemm(cols, _w16(cache, "vpatch", p.patch_w, k.cast), k=v.patch_dim)
    else:
        cols = (ops.im2col if grid is None else ops.im2col_rect)(pixel_values, v.patch_size)
        patch = ops.gemm(cols, p.patch_w.view(D, -1), ops.LAYOUT_NT)
    emb = ops.vision_assemble_fwd(patch, p.class_embedding, pos, B, S, D)
    del patch
    x, m0, r0 = ops.layernorm_fwd(emb, p.pre_w, p.pre_b, v.layer_norm_eps, save_stats=True)
    refresh_train_weights(cache, p.layers, "v", dtype)   # W and W^T of all layers, one launch per optimizer step
    saved_layers = []
    for li, lp in enumerate(p.layers):
        x, sv = layer_fwd_bf16_train(x, lp, cache, f"v{li}.", B, S, H, False, v.layer_norm_eps, dtype)
        saved_layers.append(sv)
    cls_tok = ops.gather_rows(x, None, B, S, D)
    pooled, mp, rp = ops.layernorm_fwd(cls_tok, p.post_w, p.post_b, v.layer_norm_eps, save_stats=True)
    out = ops.gemm(pooled, p.proj_w, ops.LAYOUT_NT)
    return out, (cols, emb, m0, r0, saved_layers, cls_tok, mp, rp, pooled, grid)


def vision_bwd_bf16(p: VisionParams, saved, d_out: torch.Tensor, cfg, need: List[bool], cache: dict, on_ready=None, alloc=None,
                    dtype=torch.bfloat16):
    """Backward of vision_fwd_bf16_train (of the same `dtype`); same contract as vision_bwd (`on_ready` per gradient group,
    `alloc` naming the tensor each parameter gradient is written into)."""
    v = cfg
    k = _TRAIN16[dtype]
    cols, emb, m0, r0, saved_layers, cls_tok, mp, rp, pooled, grid = saved
    B = cls_tok.shape[0]
    S, D, H = _grid_seq(v, grid), v.hidden_size, v.num_attention_heads
    names = p.names()
    needd = dict(zip(names, need))
    grads: Dict[str, Optional[torch.Tensor]] = {n: None for n in names}
    dev = d_out.device
    dcls = _vision_tail_bwd(p, d_out, cls_tok, mp, rp, pooled, needd, grads, alloc, on_ready)
    lowest = _lowest_needed(names, needd, VisionParams.HEAD, VisionParams.TAIL)
    if lowest is None:
        return [grads[n] for n in names]
    dx = ops.scatter_rows(dcls, None, B, S, D)
    dx16, fc2_b = None, None
    bottom = max(lowest, 0)
    for i in range(len(p.layers) - 1, bottom - 1, -1):
        lneed = {f: needd[f"layers.{i}.{f}"] for f in LayerParams.FIELDS}
        lalloc = None if alloc is None else (lambda f, shape, i=i: alloc(f"layers.{i}.{f}", shape))
        # this layer's LayerNorm1 backward also leaves, for the layer below, the bf16 copy of dx and its column sums (= that
        # layer's fc2 bias gradient, written where `alloc` puts it)
        below = None
        if i > bottom and needd[f"layers.{i - 1}.fc2_b"]:
            below = _galloc(alloc, f"layers.{i - 1}.fc2_b", (D,), dev)
        dx, dx16, gr = layer_bwd_bf16(dx, p.layers[i], cache, f"v{i}.", saved_layers[i], B, S, H, False, lneed, lalloc,
                                      dx2_16=dx16, fc2_b=fc2_b, below_fc2_b=below, want_dx16=i > bottom, dtype=dtype)
        fc2_b = below
        saved_layers[i] = None
        for f, t in gr.items():
            grads[f"layers.{i}.{f}"] = t
        if on_ready is not None:
            on_ready({f"layers.{i}.{f}": t for f, t in gr.items()})
    if lowest < 0:
        _vision_head_bwd(p, dx, emb, m0, r0, cols, B, S, v, grid, needd, grads, alloc, on_ready, k16=k)
    return [grads[n] for n in names]


# --------------------------------------------------------------------------------------------- text tower

@dataclass
class TextParams:
    tok: torch.Tensor            # [vocab, D]
    pos: torch.Tensor            # [Tmax, D]
    layers: List[LayerParams]
    final_w: torch.Tensor
    final_b: torch.Tensor
    proj_w: torch.Tensor         # text_projection [P, D]

    HEAD = ("tok", "pos")
    TAIL = ("final_w", "final_b", "proj_w")

    def tensors(self):
        out = [self.tok, self.pos]
        for l in self.layers:
            out += l.tensors()
        return out + [self.final_w, self.final_b, self.proj_w]

    @classmethod
    def from_tensors(cls, ts, n_layers):
        ts = list(ts)
        layers = [LayerParams(*ts[2 + 12 * i: 2 + 12 * (i + 1)]) for i in range(n_layers)]
        return cls(ts[0], ts[1], layers, *ts[2 + 12 * n_layers:])

    def names(self):
        out = list(self.HEAD)
        for i in range(len(self.layers)):
            out += [f"layers.{i}.{f}" for f in LayerParams.FIELDS]
        return out + list(self.TAIL)


def text_encoder_fwd(p: TextParams, input_ids: torch.Tensor, cfg, save: bool, hidden_out: Optional[list] = None,
                     split16_cache: Optional[dict] = None, split16_out: Optional[list] = None):
    """Embeddings + causal stack; returns the PRE-final-LN hidden states [B*T, D].  `split16_cache`, `split16_out`: as
    vision_fwd's — a forward that saves for the backward runs the layers' full-size GEMMs on the trainable text tower's own
    device plan (HipCLIPModel._tsplit16_train_cache)."""
    t = cfg
    B, T = input_ids.shape
    D, H = t.hidden_size, t.num_attention_heads
    x = ops.text_embed_fwd(input_ids, p.tok, p.pos)
    if hidden_out is not None:
        hidden_out.append(x)
    saved_layers = []
    plan, keep = _text_train_split16(p, cfg, save, split16_cache, split16_out)
    for li, lp in enumerate(p.layers):
        x, sv = layer_fwd(x, lp, B, T, H, True, t.layer_norm_eps, save, plan[li] if plan is not None else None, keep,
                          act=hidden_act(t))
        saved_layers.append(sv)
        if hidden_out is not None:
            hidden_out.append(x)
    return x, saved_layers


def text_fwd_frozen(p: TextParams, input_ids: torch.Tensor, cfg):
    """get_text_features without gradients: like text_fwd, but the LAST layer is evaluated only where it is read —
    everything after its attention on the B first-EOS rows, its attention for that one query row per caption
    (keys 0..eos, causal).  Exact; 9/12 of that layer's GEMM work is never launched."""
    t = cfg
    B, T = input_ids.shape
    D, H = t.hidden_size, t.num_attention_heads
    eos = ops.first_eos(input_ids, t.eos_token_id)
    x = ops.text_embed_fwd(input_ids, p.tok, p.pos)
    for lp in p.layers[:-1]:
        x, _ = layer_fwd(x, lp, B, T, H, True, t.layer_norm_eps, False, act=hidden_act(t))
    lp = p.layers[-1]
    ln1, _, _ = ops.layernorm_fwd(x, lp.ln1_w, lp.ln1_b, t.layer_norm_eps, save_stats=False)
    qkv = ops.gemm(ln1, lp.qkv_w, ops.LAYOUT_NT, bias=lp.qkv_b)
    attn = ops.attention_row_fwd(qkv, eos, B, T, H)
    rows = _pruned_tail_f32(attn, ops.gather_rows(x, eos, B, T, D), lp, t.layer_norm_eps, hidden_act(t))
    return _text_head(rows, p, t.layer_norm_eps)[0]


def _pruned_tail_f32(ctx_rows, x_rows, lp: LayerParams, eps: float, act: str = QUICK_GELU):
    """What follows the attention in the pruned last layer of a frozen fp32 (or split-fp16) tower, on the pooled rows only
    (M = batch, ops.gemm): out-projection + residual, LayerNorm 2, fc1 with the activation `act`, fc2 + residual.  `ctx_rows`: those rows'
    attention context, `x_rows`: their rows of the layer's input — the caller launches the one-row attention first and the row
    gather second.  Returns the final hidden state of the rows.  Used by text_fwd_frozen, text_fwd_frozen_split16,
    text_fwd_frozen_packed ("fp32" / split16) and _frozen_split16_last_cls (last_layer_fwd_cls, which saves for a backward, is
    not a copy)."""
    x1 = ops.gemm(ctx_rows, lp.out_w, ops.LAYOUT_NT, bias=lp.out_b, residual=x_rows)
    ln2, _, _ = ops.layernorm_fwd(x1, lp.ln2_w, lp.ln2_b, eps, save_stats=False)
    g, _ = _fc1_act_f32(ln2, lp, act)
    return ops.gemm(g, lp.fc2_w, ops.LAYOUT_NT, bias=lp.fc2_b, residual=x1)


def _text_head(rows, p: TextParams, eps: float, save: bool = False):
    """final_layer_norm and the projection of the pooled (first-EOS) rows [B, D] -> (out [B, P], pooled, mean, rstd); the
    statistics only with `save`.  M = B: always ops.gemm, whatever ran the layers."""
    pooled, mp, rp = ops.layernorm_fwd(rows, p.final_w, p.final_b, eps, save_stats=save)
    return ops.gemm(pooled, p.proj_w, ops.LAYOUT_NT), pooled, mp, rp


def _text_token_tail(x, p: TextParams, input_ids: torch.Tensor, cfg):
    """final_layer_norm on ALL rows, the projection and the first-EOS gather -> (sentence [B,P], tokens [B*T,P], eos [B])."""
    B, T = input_ids.shape
    ln, _, _ = ops.layernorm_fwd(x, p.final_w, p.final_b, cfg.layer_norm_eps, save_stats=False)
    tokens = ops.gemm(ln, p.proj_w, ops.LAYOUT_NT)
    eos = ops.first_eos(input_ids, cfg.eos_token_id)
    return ops.gather_rows(tokens, eos, B, T, tokens.shape[1]), tokens, eos


# --------------------------------------------------------------------------------------------- frozen fp32 text tower, split fp16
# The frozen fp32 text tower's full-size GEMMs on the fp16 MFMAs with fp32-grade error.  An fp32 value is
# hi + lo with hi = fp16(v), lo = fp16(v - hi) (22 mantissa bits); fp16 products are exact in the fp32 accumulator, so
# A W^T = A_hi W_hi^T + A_lo W_hi^T + A_hi W_lo^T up to the dropped lo.lo term — ONE fp16 GEMM along K' = 3K on
# [A_hi | A_lo | A_hi] and [W_hi | W_hi | W_lo].  Operands are scaled by powers of two (exact) so that they sit high in fp16's
# range and cannot overflow: weights by 2^f with max|W| 2^f in [2^13, 2^14), activations by 2^e with bound 2^e <= 2^14, where
# `bound` is a worst case derived from the frozen WEIGHTS alone (never from data: no host sync, no data-dependent branch in
# the step); the GEMM's alpha = 2^-(e+f) undoes both before bias / GELU / residual.  Residual stream, attention, softmax,
# LayerNorm statistics, bias and GELU are the fp32 kernels of the plain path.

_SPLIT16 = os.environ.get("DCLIP_TEXT_SPLIT16", "1") != "0"     # read once at import: no getenv on the launch path
# fc1's quick-GELU output leaves its GEMM already split (dclip_gemm_f16_scaled_split) instead of as fp32 followed by the
# stand-alone split pass; 0 = the two-launch form (bit-identical results; kept for the A/B of DESIGN.md §9c)
_SPLIT16_FC1_EPI = os.environ.get("DCLIP_TEXT_SPLIT16_FC1_EPI", "1") != "0"
_SPLIT16_TOP = 14                                               # operands are kept within 2^14 (fp16 overflows at 2^16)
_SPLIT16_EMIN, _SPLIT16_EMAX = -14, 24
_SPLIT16_LOGGED: set = set()


def text_split16_enabled() -> bool:
    return _SPLIT16


def _split16_log_once(msg: str) -> None:
    if msg not in _SPLIT16_LOGGED:
        _SPLIT16_LOGGED.add(msg)
        import logging
        logging.getLogger("dclip_amd").warning(msg)


def split16_weight_exp(max_abs: float) -> int:
    """f with max|W| 2^f in [2^13, 2^14) (0 for an all-zero weight)."""
    import math
    if max_abs == 0.0:
        return 0
    return _SPLIT16_TOP - math.frexp(max_abs)[1]             # max_abs = m 2^x, m in [0.5, 1)


def split16_act_exp(bound: float) -> Optional[int]:
    """The largest e <= 24 with bound 2^e <= 2^14; None when no e >= -14 satisfies it or the bound is not finite (guard)."""
    import math
    if not math.isfinite(bound) or bound < 0.0:
        return None
    if bound == 0.0:
        return _SPLIT16_EMAX
    m, x = math.frexp(bound)                                  # bound <= 2^x, = 2^(x-1) when m == 0.5
    e = _SPLIT16_TOP - (x - 1 if m == 0.5 else x)
    if e < _SPLIT16_EMIN:
        return None
    return min(e, _SPLIT16_EMAX)


def split16_layer_bounds(st: Dict[str, float], D: int) -> Dict[str, float]:
    """Worst-case magnitudes of the three split activations of a layer from its weight statistics `st`:
       LayerNorm output   max|gamma| sqrt(D) + max|beta|            (|x - mu| rstd <= sqrt(D) for every row)
       attention context  bound_ln1 max_n ||W_v[n,:]||_1 + max|b_v|  (a convex combination of V rows)
       GELU output        bound_ln2 max_n ||W_fc1[n,:]||_1 + max|b_fc1|   (|quick_gelu(v)| <= |v|)"""
    import math
    ln1 = st["ln1_w"] * math.sqrt(D) + st["ln1_b"]
    ln2 = st["ln2_w"] * math.sqrt(D) + st["ln2_b"]
    return {"ln1": ln1, "ctx": ln1 * st["v_l1"] + st["v_b"], "ln2": ln2, "g": ln2 * st["fc1_l1"] + st["fc1_b"]}


_SPLIT16_STATS = ("ln1_w", "ln1_b", "v_l1", "v_b", "ln2_w", "ln2_b", "fc1_l1", "fc1_b", "qkv", "out", "fc1", "fc2")
_SPLIT16_WATCHED = ("ln1_w", "ln1_b", "qkv_w", "qkv_b", "out_w", "ln2_w", "ln2_b", "fc1_w", "fc1_b", "fc2_w")


def _split16_stamp(layers: List[LayerParams]) -> tuple:
    return tuple((t._version, t.data_ptr()) for lp in layers for t in (getattr(lp, f) for f in _SPLIT16_WATCHED))


def _split16_plan(layers_p: List[LayerParams], cache: dict, what: str = "split-fp16 text tower",
                  off: str = "set DCLIP_TEXT_SPLIT16=0"):
    """Per weight version: the [hi|hi|lo] fp16 copies of W 2^f and the power-of-two activation scales of every layer, or
    None when the guard sends the tower to the plain fp32 path.  ONE device -> host read of the weight statistics, at
    cache-build time (warm-up, before any graph capture); the copies are refreshed in place when a weight changes.
    `layers_p`: the frozen tower's encoder layers (the text tower's, or the vision tower's at precision "fp32-split16",
    DESIGN.md §28); `what` heads the log records, `off` is their advice for a tower whose weights do move."""
    stamp = _split16_stamp(layers_p)
    plan = cache.get("__split16__")
    if plan is not None and plan["stamp"] == stamp:
        return plan["layers"]
    if torch.cuda.is_current_stream_capturing():
        _split16_log_once(f"{what}: weights changed while a graph is being captured; this capture takes the "
                          "plain fp32 path (run one eager step first)")
        return None
    if plan is not None:
        # frozen weights do not move: a rebuild after the first costs a host read, and one on every call (a parameter that is
        # written each step, or a non-contiguous one whose contiguous copy has a new address each call) would do so every step
        _split16_log_once(f"{what}: a weight's version or storage changed; the split copies and scales are rebuilt "
                          f"(one device-to-host read).  If a weight changes every step, {off}")
    D = layers_p[0].ln1_w.shape[0]
    rows = []
    for lp in layers_p:
        wv, bv = lp.qkv_w[2 * D:], lp.qkv_b[2 * D:]
        rows.append(torch.stack([lp.ln1_w.abs().max(), lp.ln1_b.abs().max(), wv.abs().sum(1).max(), bv.abs().max(),
                                 lp.ln2_w.abs().max(), lp.ln2_b.abs().max(), lp.fc1_w.abs().sum(1).max(), lp.fc1_b.abs().max(),
                                 lp.qkv_w.abs().max(), lp.out_w.abs().max(), lp.fc1_w.abs().max(), lp.fc2_w.abs().max()]))
    stats = torch.stack(rows).double().cpu().tolist()
    import math
    layers = []
    old = plan["layers"] if plan is not None and plan["layers"] is not None else None
    for li, (lp, row) in enumerate(zip(layers_p, stats)):
        st = dict(zip(_SPLIT16_STATS, row))
        if not all(math.isfinite(v) for v in row):
            layers = None
            _split16_log_once(f"{what}: non-finite weight in layer {li}; taking the plain fp32 path")
            break
        exps = {k: split16_act_exp(b) for k, b in split16_layer_bounds(st, D).items()}
        if any(e is None for e in exps.values()):
            layers = None
            _split16_log_once(f"{what}: an activation bound of layer {li} does not fit fp16 at any scale >= 2^-14; "
                              "taking the plain fp32 path")
            break
        ent = {"e": exps, "f": {}, "w": {}}
        for short, field in _TRAIN_WEIGHTS:
            w = getattr(lp, field)
            f = split16_weight_exp(st[short])
            prev = old[li]["w"][short] if old is not None and li < len(old) and tuple(old[li]["w"][short].shape) == (w.shape[0], 3 * w.shape[1]) else None
            ent["f"][short] = f
            ent["w"][short] = ops.split_f16x3(w.detach().contiguous(), 2.0 ** f, 1, out=prev)
        layers.append(ent)
    cache["__split16__"] = {"stamp": stamp, "layers": layers}
    return layers


def _text_frozen_split16_plan(p: TextParams, cfg, cache: dict):
    """The frozen text tower's host plan (_split16_plan's layers), or None — the plain fp32 path — when DCLIP_TEXT_SPLIT16 is
    off, the tower has no layer, a width is no multiple of 8 or the plan's own guard trips."""
    if not (_SPLIT16 and len(p.layers) > 0 and cfg.hidden_size % 8 == 0 and cfg.intermediate_size % 8 == 0):
        return None
    if _split16_declines_act(cfg, "split-fp16 text tower"):
        return None
    return _split16_plan(p.layers, cache)


def _split16_gemm(a3, ent, short: str, akey: str, **kw):
    """epilogue(A W^T) from the split operands; alpha undoes the operand scales."""
    alpha = 2.0 ** -(ent["e"][akey] + ent["f"][short])
    out_pieces = kw.pop("out_pieces", 3)
    if _fused_k(a3, ent["w"][short]):      # the fused twin (§9h)
        return ops.gemm_f16x3(a3, ent["w"][short], alpha=alpha, pieces=_a_pieces(a3, ent["w"][short]), out_pieces=out_pieces, **kw)
    if out_pieces != 3:
        raise RuntimeError("a two-piece split output needs the fused entry")
    return ops.gemm_f16(a3, ent["w"][short], alpha=alpha, **kw)


# The attention context of a frozen split layer leaves the attention kernel already split (ops.attention_fwd_f16x2 /
# ops.attention_varlen_fwd_f16x2) at precision "fp32-split16"; 0 = attention_fwd + the stand-alone split pass there
# too (bit-identical results; the A/B of §28).  The paths that existed before that precision keep the two launches.
_SPLIT16_ATTN_EPI = os.environ.get("DCLIP_SPLIT16_ATTN_EPI", "1") != "0"


def _dense_ctx3(B: int, S: int, H: int, causal: bool, fused: bool):
    """(qkv, scale, pieces) -> the split attention context of B sequences of S tokens: one launch (`fused` and the switch
    above), or the fp32 context and the split pass."""
    if fused and _SPLIT16_ATTN_EPI:
        return lambda qkv, scale, pieces: ops.attention_fwd_f16x2(qkv, B, S, H, causal, scale, pieces)
    return lambda qkv, scale, pieces: ops.split_f16x3(ops.attention_fwd(qkv, B, S, H, causal)[0], scale, pieces=pieces)


def _packed_ctx3(cu, max_S: int, H: int, causal: bool, fused: bool):
    """_dense_ctx3 for packed sequences (rows cu[n] .. cu[n+1]-1)."""
    if fused and _SPLIT16_ATTN_EPI:
        return lambda qkv, scale, pieces: ops.attention_varlen_fwd_f16x2(qkv, cu, max_S, H, causal, scale, pieces)
    attn = ops.attention_varlen_causal_fwd if causal else ops.attention_varlen_fwd
    return lambda qkv, scale, pieces: ops.split_f16x3(attn(qkv, cu, max_S, H), scale, pieces=pieces)


def _frozen_split16_layer(x, lp: LayerParams, ent, pc: Dict[str, int], eps: float, ctx3):
    """One full encoder layer of a frozen tower on the host plan's entry `ent` (_split16_plan): the four GEMMs on split-fp16
    operands, everything else the fp32 kernels.  `pc`: _layer_pieces at these rows; `ctx3`: _dense_ctx3 / _packed_ctx3."""
    e = ent["e"]
    ln1 = ops.layernorm_fwd_f16x3(x, lp.ln1_w, lp.ln1_b, eps, 2.0 ** e["ln1"], pieces=pc["ln1"])
    qkv = _split16_gemm(ln1, ent, "qkv", "ln1", bias=lp.qkv_b)
    x1 = _split16_gemm(ctx3(qkv, 2.0 ** e["ctx"], pc["ctx"]), ent, "out", "ctx", bias=lp.out_b, residual=x)
    ln2 = ops.layernorm_fwd_f16x3(x1, lp.ln2_w, lp.ln2_b, eps, 2.0 ** e["ln2"], pieces=pc["ln2"])
    if _SPLIT16_FC1_EPI:
        g3 = _split16_gemm(ln2, ent, "fc1", "ln2", bias=lp.fc1_b, gelu=True, split_out_scale=2.0 ** e["g"], out_pieces=pc["g"])
    else:
        g3 = ops.split_f16x3(_split16_gemm(ln2, ent, "fc1", "ln2", bias=lp.fc1_b, gelu=True), 2.0 ** e["g"], pieces=pc["g"])
    return _split16_gemm(g3, ent, "fc2", "g", bias=lp.fc2_b, residual=x1)


def text_fwd_frozen_split16(p: TextParams, input_ids: torch.Tensor, cfg, cache: dict):
    """text_fwd_frozen with every full-size GEMM evaluated on split-fp16 operands (see above); the last layer's EOS-row
    GEMMs (M = B), the final LayerNorm and the projection stay on ops.gemm.  `cache`: the split weights and scales, kept
    between calls.  Falls back to text_fwd_frozen when the switch is off or the guard trips."""
    t = cfg
    D = t.hidden_size
    plan = _text_frozen_split16_plan(p, t, cache)
    if plan is None:
        return text_fwd_frozen(p, input_ids, cfg)
    B, T = input_ids.shape
    H, eps = t.num_attention_heads, t.layer_norm_eps
    eos = ops.first_eos(input_ids, t.eos_token_id)
    x = ops.text_embed_fwd(input_ids, p.tok, p.pos)
    pc = _layer_pieces(x.shape[0], D, t.intermediate_size, _SPLIT16_FC1_EPI)
    ctx3 = _dense_ctx3(B, T, H, True, False)
    for lp, ent in zip(p.layers[:-1], plan[:-1]):
        x = _frozen_split16_layer(x, lp, ent, pc, eps, ctx3)
    lp, ent = p.layers[-1], plan[-1]
    ln1 = ops.layernorm_fwd_f16x3(x, lp.ln1_w, lp.ln1_b, eps, 2.0 ** ent["e"]["ln1"], pieces=pc["ln1"])
    qkv = _split16_gemm(ln1, ent, "qkv", "ln1", bias=lp.qkv_b)
    attn = ops.attention_row_fwd(qkv, eos, B, T, H)
    rows = _pruned_tail_f32(attn, ops.gather_rows(x, eos, B, T, D), lp, eps)
    return _text_head(rows, p, eps)[0]


# --------------------------------------------------------------------------------------------- frozen fp32 vision tower, split fp16
# The frozen vision tower at precision "fp32-split16" (opt-in): the host plan above on the vision tower's layers,
# in a cache of its own on the model (HipCLIPModel._vsplit16_frozen_cache) — never the student's device plan, whose buffers the
# training stream rewrites.  The patch embedding, the pre / post LayerNorm and the projection stay fp32 (pixel magnitudes have no
# bound derivable from the weights); precision "fp32" is untouched.

_VFROZEN_WHAT = "split-fp16 frozen vision tower"


def _vision_frozen_split16_plan(layers: List[LayerParams], cfg, cache: Optional[dict]):
    """The frozen vision tower's host plan (_split16_plan's layers), or None: the plain fp32 path."""
    if cache is None or not layers or cfg.hidden_size % 8 or cfg.intermediate_size % 8:
        return None
    if _split16_declines_act(cfg, _VFROZEN_WHAT):
        return None
    return _split16_plan(layers, cache, _VFROZEN_WHAT, 'use precision="fp32"')


def _frozen_split16_last_cls(x, lp: LayerParams, ent, eps: float, ctx_rows, x_rows):
    """The pruned last layer of a frozen vision schedule on the host plan: LayerNorm1 and the qkv projection at full size on
    split operands, then last_layer_fwd_cls's steps on the CLS rows — `ctx_rows(qkv)` their fp32 attention context, `x_rows(x)`
    their residual rows — on ops.gemm (M = images).  Returns the final hidden state of the CLS rows."""
    D = x.shape[1]
    ln1 = ops.layernorm_fwd_f16x3(x, lp.ln1_w, lp.ln1_b, eps, 2.0 ** ent["e"]["ln1"], pieces=split16_pieces([(x.shape[0], 3 * D, D)]))
    qkv = _split16_gemm(ln1, ent, "qkv", "ln1", bias=lp.qkv_b)
    return _pruned_tail_f32(ctx_rows(qkv), x_rows(x), lp, eps)


def vision_fwd_frozen_split16(p: VisionParams, pixel_values: torch.Tensor, cfg, cache: dict, grid=None,
                              hidden_out: Optional[list] = None) -> torch.Tensor:
    """vision_fwd(save=False) with the full-size GEMMs of the encoder layers on split-fp16 operands: [B,3,H,W] -> [B,P].  `grid`
    as in vision_fwd.  `cache`: the model's frozen split cache (copies and scales, kept between calls).  The plain fp32 forward,
    bit for bit, when the guard trips (_split16_plan) and whenever hidden states are asked for."""
    v = cfg
    plan = _vision_frozen_split16_plan(p.layers, v, cache) if hidden_out is None else None
    if plan is None:
        return vision_fwd(p, pixel_values, cfg, False, hidden_out, grid=grid)[0]
    B = pixel_values.shape[0]
    S, D, H, eps = _grid_seq(v, grid), v.hidden_size, v.num_attention_heads, v.layer_norm_eps
    if grid is None:
        cols, pos = ops.im2col(pixel_values, v.patch_size), p.pos
    else:
        pos = _grid_front(p, pixel_values, v, grid)
        cols = ops.im2col_rect(pixel_values, v.patch_size)
    patch = ops.gemm(cols, p.patch_w.view(D, -1), ops.LAYOUT_NT)
    emb = ops.vision_assemble_fwd(patch, p.class_embedding, pos, B, S, D)
    del patch, cols
    x, _, _ = ops.layernorm_fwd(emb, p.pre_w, p.pre_b, eps, save_stats=False)
    pc = _layer_pieces(x.shape[0], D, v.intermediate_size, _SPLIT16_FC1_EPI)
    ctx3 = _dense_ctx3(B, S, H, False, True)
    for lp, ent in zip(p.layers[:-1], plan[:-1]):
        x = _frozen_split16_layer(x, lp, ent, pc, eps, ctx3)
    cls_tok = _frozen_split16_last_cls(x, p.layers[-1], plan[-1], eps, lambda qkv: ops.attention_cls_fwd(qkv, B, S, H)[0],
                                       lambda xx: ops.gather_rows(xx, None, B, S, D))
    pooled, _, _ = ops.layernorm_fwd(cls_tok, p.post_w, p.post_b, eps, save_stats=False)
    return ops.gemm(pooled, p.proj_w, ops.LAYOUT_NT)


# --------------------------------------------------------------------------------------------- student's vision forward, split fp16
# The same arithmetic for a tower that TRAINS: its weights change every step, so the host-side plan above (one
# device -> host read, host floats handed to the kernels) cannot be used — a read per step is a sync in the hot path and a host
# float captured in a HIP graph is stale after the next optimizer step.  Statistics, scales and the split weight copies are
# made ON THE DEVICE by three launches (ops.split16_refresh) at the head of a forward whenever a watched parameter's version
# or address has moved, and the kernels read the scales through pointers into the plan record.  The device applies the rules
# of split16_layer_bounds / split16_act_exp / split16_weight_exp but has no fall-back: where the host guard would decline, it
# takes the exponent the bound asks for and raises a flag, which reaches the host by a copy nothing waits for.

_VSPLIT16 = os.environ.get("DCLIP_VISION_SPLIT16", "1") != "0"    # read once at import: no getenv on the launch path
# fc1 leaves its GEMM as h, g AND the split of g (one launch, three outputs); 0 = h and g from the GEMM, then the split pass
_VSPLIT16_FC1_EPI = os.environ.get("DCLIP_VISION_SPLIT16_FC1_EPI", "1") != "0"
# the backward's full-size data-gradient GEMMs on the same plan, dY split per row; 0 = the plain fp32 dgrads
_VSPLIT16_BWD = os.environ.get("DCLIP_VISION_SPLIT16_BWD", "1") != "0"
# that backward's full-size weight-gradient GEMMs too, dY split per column; 0 = the plain fp32 wgrads.  Needs
# the two switches above: the X operands are the forward's splits, and the fused dY pass is the split backward's
_VSPLIT16_WGRAD = os.environ.get("DCLIP_VISION_SPLIT16_WGRAD", "1") != "0"
# ... and the kernels that produce those dY leave the column partials, so that dY is read once; 0 = the
# three-launch pass of §9f for every dY, the parent's launch list and outputs bit for bit
_VSPLIT16_DYSTATS = os.environ.get("DCLIP_VISION_SPLIT16_DYSTATS", "1") != "0"
# The patch embedding and the gradient of its weight on split operands too: the activation scale from max|pixels|,
# taken on the device every forward, im2col writing [hi|lo] directly, the GEMMs fc2's fused call forms.  The forward half under
# DCLIP_VISION_SPLIT16, the weight-gradient half under _BWD and _WGRAD as well; 0 = ops.im2col and the two fp32 GEMMs, the
# parent's launch list and outputs bit for bit.  Depends on no other switch (patch_split16_taken)
_VSPLIT16_PATCH = os.environ.get("DCLIP_VISION_SPLIT16_PATCH", "1") != "0"
# Every split GEMM above — both towers' forwards, the data and the weight gradients — on its fused twin, which stages the hi
# pieces once, wherever that twin's plan takes the shape; 0 = the 3 K / three-segment entries everywhere, the
# parent's launch list and outputs bit for bit.  "kmajor" / "tokmajor": one form alone (the A/B of §9h).
_SPLIT16_FUSED = os.environ.get("DCLIP_SPLIT16_FUSED", "1")
_SPLIT16_FUSED_K = _SPLIT16_FUSED not in ("0", "tokmajor")
_SPLIT16_FUSED_TOK = _SPLIT16_FUSED not in ("0", "kmajor")
# The split activation / gradient operands of both towers as two pieces [hi|lo] wherever every K-major GEMM that reads one takes
# its fused twin (split16_pieces): the duplicate third of [hi|lo|hi], which no fused entry reads, is not written;
# 0 = three pieces everywhere, the parent's launches, allocations and outputs bit for bit
_SPLIT16_PIECES2 = os.environ.get("DCLIP_SPLIT16_PIECES2", "1") != "0"
# A vision forward that keeps its split operands for the weight gradients (§9f) does not also store the fp32 ln1 / ln2 / g where
# that weight gradient has a split plan (_drops32): only the fp32 fall-back reads them, and it makes them again
# (layernorm_fwd on the saved input; quick_gelu of the saved h), bit for bit.  Opt-in (1): alone against the parent it gained
# 1.0-1.6 % and missed the project's bar in one of three pairs (§9j); the default, 0, stores them as before
_VSPLIT16_DROP32 = os.environ.get("DCLIP_VISION_SPLIT16_DROP32", "0") == "1"
# The TRAINABLE text tower on the same machinery (HipCLIPModel.text_train_split16) has no switches of its own for
# the sub-features: _VSPLIT16_BWD, _WGRAD, _DYSTATS, _FC1_EPI, _DROP32, _SPLIT16_FUSED* and _PIECES2 are read inside the shared
# layer functions and act on the text path exactly as on the vision path.  Its one own switch: the statistics twin of the
# 65 .. 80-row attention backward; 0 = dqkv takes the three-launch split of §9f and qkv_b one more pass over dqkv (ops.colsum_segments), every gradient bit for bit the statistics form's
_TSPLIT16_ROWS_STATS = os.environ.get("DCLIP_TEXT_SPLIT16_ROWS_STATS", "1") != "0"
_TSPLIT16_KEY, _TSPLIT16_WHAT = "__tsplit16__", "split-fp16 trainable text tower"


def vision_split16_enabled() -> bool:
    return _VSPLIT16


def split16_plan_host(st: Dict[str, float], D: int) -> Dict[str, object]:
    """What the device plan kernel (dclip_split16_plan) makes of one layer's statistics `st` (keys _SPLIT16_STATS): the
    exponents e (activations), f (weights), a = -(e + f) (alphas) and the flag bits.  The host rules above without their
    fall-back: where split16_act_exp declines, the exponent the bound asks for is taken and a flag is set (1: e < -14,
    2: a non-finite statistic, 4: a scale outside fp32's normal range, clamped).  The reference of tests/test_vision_split16_*."""
    import math
    flags = 0
    e, f = {}, {}
    for k, b in split16_layer_bounds(st, D).items():
        x = split16_act_exp(b)
        if x is None:
            if not math.isfinite(b) or b < 0.0:
                flags |= 2
                x = 0
            else:
                flags |= 1
                m, ex = math.frexp(b)
                x = _SPLIT16_TOP - (ex - 1 if m == 0.5 else ex)
        e[k] = x
    for short, _ in _TRAIN_WEIGHTS:
        if math.isfinite(st[short]):
            f[short] = split16_weight_exp(st[short])
        else:
            flags |= 2
            f[short] = 0
    a = {}
    for short, akey in (("qkv", "ln1"), ("out", "ctx"), ("fc1", "ln2"), ("fc2", "g")):
        if e[akey] < -126:
            e[akey], flags = -126, flags | 4
        if f[short] > 127:
            f[short], flags = 127, flags | 4
        a[short] = -(e[akey] + f[short])
        if not -126 <= a[short] <= 127:
            a[short], flags = max(-126, min(127, a[short])), flags | 4
    return {"e": e, "f": f, "a": a, "flags": flags}


def split16_row_exp(r: float) -> int:
    """e with r 2^e in [2^13, 2^14) for a row maximum r = max|dY[m,:]| (r = mu 2^x, mu in [0.5, 1): e = 14 - x), clamped to
    [-100, 100] so that 2^e, 2^-e and their products with a weight alpha stay normal fp32; 0 for r = 0 or a non-finite r.
    The rule of the row-scaled split (dclip_split_f32_f16x3_rows) and the reference of its tests."""
    import math
    if r == 0.0 or not math.isfinite(r):
        return 0
    return max(-100, min(100, _SPLIT16_TOP - math.frexp(abs(r))[1]))


def split16_col_exp(r: float) -> int:
    """split16_row_exp applied to a COLUMN maximum r = max|dY[:,n]|: the exponent of the column-scaled split of the weight
    gradients' dY operand (dclip_split_f32_f16x3_rows_colstats) and the reference of its tests."""
    return split16_row_exp(r)


def split16_rows_host(x: torch.Tensor):
    """What dclip_split_f32_f16x3_rows makes of a host fp32 matrix: (fp16 [rows, 3 cols] = [hi|lo|hi], fp32 row_alpha)."""
    x = x.float()
    e = torch.tensor([split16_row_exp(float(r)) for r in x.abs().amax(dim=1).double()], dtype=torch.float32)
    v = x * torch.exp2(e)[:, None]
    hi = v.half()
    lo = (v - hi.float()).half()
    return torch.cat([hi, lo, hi], dim=1), torch.exp2(-e)


class Split16Bwd:
    """What a backward needs to run its data-gradient GEMMs on the plan of ITS forward: the layers'
    Split16Layer list and the versions / addresses of the watched parameters that the forward's refresh saw.  The split
    copies are the model's and persistent, so a parameter written — or another forward's refresh issued — between this
    forward and its backward would pair dY with other weights: fresh() is the host check (nothing read from the device)
    that sends such a backward down the plain path."""
    __slots__ = ("layers", "ent", "params", "ptrs", "versions", "epoch")

    def __init__(self, layers, ent: dict, params: List[LayerParams]):
        self.layers, self.ent, self.params = layers, ent, params
        self.ptrs = tuple(getattr(lp, f).data_ptr() for lp in params for f in _SPLIT16_WATCHED)
        self.versions = tuple(getattr(lp, f)._version for lp in params for f in _SPLIT16_WATCHED)
        self.epoch = ent["epoch"]

    def fresh(self) -> bool:
        if torch.cuda.is_current_stream_capturing():
            return True      # one capture holds the refresh, the forward and this backward: every replay re-splits first
        ok = (self.epoch == self.ent["epoch"] and
              self.ptrs == tuple(getattr(lp, f).data_ptr() for lp in self.params for f in _SPLIT16_WATCHED) and
              self.versions == tuple(getattr(lp, f)._version for lp in self.params for f in _SPLIT16_WATCHED))
        if not ok:
            _split16_log_once(self.ent.get("what", "split-fp16 vision tower") + ": a weight changed between a forward and its "
                              "backward; that backward takes the plain fp32 data-gradient GEMMs")
        return ok


def _vision_split16_flags(ent: dict) -> None:
    """Look at the flags the LAST refresh left in pinned host memory (never waited for: a flag is seen a step late).  The
    copy of the current step may be in flight while this reads: a flag is one aligned 32-bit word, so what is read is
    either the old or the new word, and a flag missed now is seen at the next look."""
    host = ent["host"]
    if host is None:
        return
    flags = host[:, ops.SPLIT16_PLAN_FLAGS].view(torch.int32)
    if bool(flags.any()):
        _split16_log_once(ent.get("what", "split-fp16 vision tower") + ": a weight statistic is non-finite or an activation bound "
                          "needs a scale below 2^-14 (layer flags " +
                          ", ".join(f"{i}:{int(f)}" for i, f in enumerate(flags.tolist()) if f) +
                          "); the forward stays on the split path with that scale and may lose accuracy (" +
                          ent.get("off", "DCLIP_VISION_SPLIT16=0") + " selects the plain fp32 path)")


def vision_split16_check_flags(cache: Optional[dict]) -> None:
    """The host's look at the guard flags for a caller that replays a captured step (graph.GraphedStep.step): a replay
    re-plans on the device and rewrites the pinned copy, but never re-enters _vision_split16_plan."""
    ent = cache.get("__vsplit16__") if cache else None
    if ent is not None:
        _vision_split16_flags(ent)
    ent = cache.get(_VPATCH16_KEY) if cache else None
    if ent is not None:
        _patch_split16_flags(ent)


# The front plan of the split patch embedding lives BESIDE the layers' table, under a key of its own in the same
# cache: what belongs to the weight (its record and [hi|hi|lo] copy, ops.split16_front_state) is kept there and made again when
# patch_w's version or address moved — always while capturing; what belongs to the pixels is a record of its own per forward,
# so that a backward finds the scale of ITS columns whatever forwards ran in between.
_VPATCH16_KEY = "__vpatch16__"


def split16_front_host(max_pixels: float, max_w: float) -> Dict[str, int]:
    """What the device front plan (dclip_split16_front) makes of max|pixels| and max|patch_w|: e = split16_act_exp, f =
    split16_weight_exp, a = -(e + f) and the flag bits of split16_plan_host (1: e < -14, 2: a non-finite maximum, 4: a scale
    outside fp32's normal range, clamped).  The reference of tests/test_patch_split16_gpu.py."""
    import math
    flags = 0
    if math.isfinite(max_w):
        f = split16_weight_exp(max_w)
    else:
        flags, f = flags | 2, 0
    if f > 127:
        f, flags = 127, flags | 4
    e = split16_act_exp(max_pixels)
    if e is None:
        if not math.isfinite(max_pixels) or max_pixels < 0.0:
            flags, e = flags | 2, 0
        else:
            flags |= 1
            m, ex = math.frexp(max_pixels)
            e = _SPLIT16_TOP - (ex - 1 if m == 0.5 else ex)
    if e < -126:
        e, flags = -126, flags | 4
    if not -126 <= -(e + f) <= 127:
        flags |= 4
    return {"e": e, "f": f, "a": max(-126, min(127, -(e + f))), "flags": flags}


def _patch_split16_flags(ent: dict) -> None:
    """_vision_split16_flags for the front record: the flags the LAST forward left in pinned memory, seen a step late."""
    host = ent["host"]
    if host is None:
        return
    flags = int(host[ops.FRONT_FLAGS:ops.FRONT_FLAGS + 1].view(torch.int32)[0])
    if flags:
        _split16_log_once(f"split-fp16 patch embedding: max|pixel_values| or max|patch_w| is non-finite, or the pixels need a scale "
                          f"below 2^-14 (flags {flags}); the forward stays on the split path with that scale and may lose accuracy "
                          "(DCLIP_VISION_SPLIT16_PATCH=0 selects the fp32 patch embedding)")


def _patch_split16_front(p: "VisionParams", pixel_values: torch.Tensor, v, save: bool, grid, cache: Optional[dict]):
    """(record, w3) of a forward that takes the split patch embedding — its front record (ops.split16_front, two launches, three
    when patch_w changed or a stream is capturing) and the [hi|hi|lo] copy of patch_w — or None: the fp32 columns and GEMM, where
    patch_split16_taken declines, the tower is a "gelu" one (it takes the plain path throughout) or the very first use arrives
    inside a graph capture."""
    D = v.hidden_size
    K = p.patch_w.numel() // D
    Bn, _, Hh, Ww = pixel_values.shape
    if v.patch_size <= 0 or Hh != Ww or Hh % v.patch_size:
        return None                                     # ops.im2col names the fault
    rows = Bn * (Hh // v.patch_size) ** 2
    if not patch_split16_taken(bool(save and cache is not None), grid, rows, D, K) or hidden_act(v) == GELU_ERF:
        return None
    w = p.patch_w.view(D, K)
    capturing = torch.cuda.is_current_stream_capturing()
    ent = cache.get(_VPATCH16_KEY)
    if ent is None or ent["ptr"] != w.data_ptr() or tuple(ent["state"]["w3"].shape) != (D, 3 * K):
        if capturing:
            _split16_log_once("split-fp16 patch embedding: first use inside a graph capture; this capture takes the fp32 patch "
                              "embedding (run one eager step first)")
            return None
        ent = {"ptr": w.data_ptr(), "version": None, "state": ops.split16_front_state(w), "host": None}
        try:
            ent["host"] = torch.zeros((8,), dtype=torch.float32).pin_memory()
        except RuntimeError:
            ent["host"] = None
        cache[_VPATCH16_KEY] = ent
    _patch_split16_flags(ent)
    rec = ops.split16_front(pixel_values, w, ent["state"], capturing or ent["version"] != w._version)
    ent["version"] = None if capturing else w._version
    if ent["host"] is not None:
        ent["host"].copy_(rec, non_blocking=True)
    return rec, ent["state"]["w3"]


def _patch_split16_fwd(p: "VisionParams", pixel_values: torch.Tensor, v, rec: torch.Tensor, w3: torch.Tensor):
    """(what the backward keeps in place of the columns, patch [rows, D] fp32): im2col written as [hi|lo] of pixel 2^e, then fc2's
    fused forward call on it and w3 with the record's alpha, no bias.  The columns are kept only where the backward half is on."""
    base = rec.data_ptr()
    cols16 = ops.im2col_f16x2(pixel_values, v.patch_size, scale_ptr=base + 4 * ops.FRONT_SCALE)
    patch = ops.gemm_f16x3_dev(cols16, w3, base + 4 * ops.FRONT_ALPHA, pieces=2)
    keep = patch_split16_taken(True, None, cols16.shape[0], w3.shape[0], w3.shape[1] // 3, backward=True)
    return _PatchSplit(cols16 if keep else None, rec, pixel_values, v.patch_size), patch


def _vision_split16_plan(layers: List[LayerParams], cfg, cache: dict, key: str = "__vsplit16__",
                         what: str = "split-fp16 vision tower", off: str = "DCLIP_VISION_SPLIT16=0"):
    """`key`, `what`, `off`: the cache entry, the log label and the way back to the plain path that a message names — the
    trainable text tower keeps its own plan under its own key.
    Per layer a Split16Layer over the model's device plan, refreshed (three launches, no host read) when a watched
    parameter changed; None = the plain path (widths not multiples of 8, or the very first call arrives inside a graph
    capture).  While a stream is capturing the refresh is always issued, so that it is part of the graph and every replay
    plans and splits the weights of that moment."""
    if len(layers) == 0 or cfg.hidden_size % 8 or cfg.intermediate_size % 8:
        return None
    capturing = torch.cuda.is_current_stream_capturing()
    ent = cache.get(key)
    ptrs = tuple(getattr(lp, f).data_ptr() for lp in layers for f in _SPLIT16_WATCHED)
    if ent is None or ent["ptrs"] != ptrs:
        if capturing:
            _split16_log_once(what + ": first use inside a graph capture; this capture takes the plain fp32 path "
                              "(run one eager step first)")
            return None
        if any(not getattr(lp, f).is_contiguous() for lp in layers for f in _SPLIT16_WATCHED):
            return None
        tab = ops.split16_table([{f: getattr(lp, f) for f in _SPLIT16_WATCHED} for lp in layers], transposed=_VSPLIT16_BWD)
        base, stride = tab["plan"].data_ptr(), 4 * tab["plan"].shape[1]
        wt = tab.get("wt")
        ent = {"ptrs": ptrs, "tab": tab, "versions": None, "host": None, "epoch": 0, "what": what, "off": off,
               "layers": [Split16Layer(w, base + li * stride, wt[li] if wt else None) for li, w in enumerate(tab["w"])]}
        try:
            ent["host"] = torch.zeros(tuple(tab["plan"].shape), dtype=torch.float32).pin_memory()
        except RuntimeError:
            ent["host"] = None
        cache[key] = ent
    versions = tuple(getattr(lp, f)._version for lp in layers for f in _SPLIT16_WATCHED)
    if capturing or ent["versions"] != versions:
        _vision_split16_flags(ent)
        ops.split16_refresh(ent["tab"])
        ent["epoch"] += 1                       # Split16Bwd.fresh: the copies a pending backward was planned on are gone
        if ent["host"] is not None:
            ent["host"].copy_(ent["tab"]["plan"], non_blocking=True)
        ent["versions"] = None if capturing else versions
    return ent["layers"]


def _train_split16(layers: List[LayerParams], cfg, save: bool, split16_cache: Optional[dict], split16_out: Optional[list],
                   on: bool = True, key: str = "__vsplit16__", what: str = "split-fp16 vision tower",
                   off: str = "DCLIP_VISION_SPLIT16=0", log_declined: bool = False):
    """(plan, keep_split) of a trainable tower's forward: the tower's device plan (_vision_split16_plan under `key`, with the
    log label `what` and the way back `off`) when the switch `on` is set, the forward saves for a backward and the caller
    handed the model's cache; (None, False) = the plain fp32 schedule.  What the backward needs to run on the same plan (a
    Split16Bwd, §9e) goes to `split16_out` when DCLIP_VISION_SPLIT16_BWD is on; keep_split: that backward's weight gradients
    take the forward's split operands (§9f).  The defaults are the vision tower's; the trainable text tower
    keeps its own plan under its own key, so neither tower's refresh touches the other's pending backward, and logs a plan that
    declined (`log_declined`)."""
    if not (on and save and split16_cache is not None):
        return None, False
    if _split16_declines_act(cfg, what):
        return None, False
    plan = _vision_split16_plan(layers, cfg, split16_cache, key, what, off)
    if plan is None:
        if log_declined:
            _split16_log_once(what + ": the plan declined (widths not multiples of 8, or first use inside a graph capture); "
                              "the tower takes the plain fp32 path")
        return None, False
    keep = False
    if split16_out is not None and _VSPLIT16_BWD and plan[0].wt is not None:
        split16_out.append(Split16Bwd(plan, split16_cache[key], layers))
        keep = _VSPLIT16_WGRAD
    return plan, keep


def _text_train_split16(p: TextParams, cfg, save: bool, split16_cache: Optional[dict], split16_out: Optional[list]):
    """_train_split16 for the trainable text tower: its own key, label and advice, and a logged decline."""
    return _train_split16(p.layers, cfg, save, split16_cache, split16_out, True, _TSPLIT16_KEY, _TSPLIT16_WHAT,
                          "text_train_split16 = False", log_declined=True)


def text_fwd(p: TextParams, input_ids: torch.Tensor, cfg, save: bool, hidden_out: Optional[list] = None,
             split16_cache: Optional[dict] = None, split16_out: Optional[list] = None):
    """get_text_features: ids [B,T] -> [B,P]  (hf:modeling_clip.py:541-586, :705-713).  LayerNorm is row-wise, so
    the first-EOS rows are gathered BEFORE final_layer_norm: only B rows are normalised and projected.
    `split16_cache`, `split16_out`: text_encoder_fwd's; the embedding, the gathered EOS rows, final_layer_norm and the projection
    (M = B) stay on ops.gemm."""
    t = cfg
    B, T = input_ids.shape
    D = t.hidden_size
    x, saved_layers = text_encoder_fwd(p, input_ids, cfg, save, hidden_out, split16_cache, split16_out)
    eos = ops.first_eos(input_ids, t.eos_token_id)
    rows = ops.gather_rows(x, eos, B, T, D)
    out, pooled, mp, rp = _text_head(rows, p, t.layer_norm_eps, save)
    saved = (input_ids, saved_layers, eos, rows, mp, rp, pooled) if save else None
    return out, saved


def _text_tail_bwd(p: TextParams, d_out, rows, mp, rp, pooled, needd: Dict[str, bool], grads):
    """proj_w's gradient, dpooled and final_layer_norm's backward -> drows [B, D], the gradient of the pooled rows."""
    if needd["proj_w"]:
        grads["proj_w"] = ops.gemm(d_out, pooled, ops.LAYOUT_TN)
    dpooled = ops.gemm(d_out, p.proj_w, ops.LAYOUT_NN)
    want = needd["final_w"] or needd["final_b"]
    drows, dg, db = ops.layernorm_bwd(dpooled, rows, p.final_w, mp, rp, need_param_grads=want)
    if want:
        grads["final_w"], grads["final_b"] = dg, db
    return drows


def text_bwd(p: TextParams, saved, d_out: torch.Tensor, cfg, need: List[bool], split16=None):
    """`split16`: the forward's Split16Bwd (text_fwd's `split16_out`); None = the plain fp32 backward."""
    t = cfg
    input_ids, saved_layers, eos, rows, mp, rp, pooled = saved
    B, T = input_ids.shape
    D, H = t.hidden_size, t.num_attention_heads
    names = p.names()
    needd = dict(zip(names, need))
    grads: Dict[str, Optional[torch.Tensor]] = {n: None for n in names}
    drows = _text_tail_bwd(p, d_out, rows, mp, rp, pooled, needd, grads)
    lowest = _lowest_needed(names, needd, TextParams.HEAD, TextParams.TAIL)
    if lowest is None:
        return [grads[n] for n in names]
    dx = ops.scatter_rows(drows, eos, B, T, D)
    dx = _layers_bwd(dx, p.layers, saved_layers, needd, grads, lowest, B * T, B, T, H, True, t.layer_norm_eps, split16,
                     act=hidden_act(t))
    if lowest < 0:
        if needd["pos"]:
            dpos = torch.zeros_like(p.pos)
            dpos[:T] = ops.colsum(dx.view(B, T * D)).view(T, D)
            grads["pos"] = dpos
        if needd["tok"]:
            dtok = torch.zeros_like(p.tok)
            grads["tok"] = ops.text_embed_bwd(input_ids, dx, dtok)
    return [grads[n] for n in names]


def _text_stack_bf16(p: TextParams, input_ids: torch.Tensor, cfg, cache: dict, n_layers: int, dtype=torch.bfloat16):
    t = cfg
    B, T = input_ids.shape
    x = ops.text_embed_fwd(input_ids, p.tok, p.pos)
    for li, lp in enumerate(p.layers[:n_layers]):
        x = _layer_fwd_bf16(x, lp, cache, f"t{li}.", B, T, t.num_attention_heads, True, t.layer_norm_eps, dtype, hidden_act(t))
    return x


def text_fwd_frozen_bf16(p: TextParams, input_ids: torch.Tensor, cfg, cache: dict, dtype=torch.bfloat16) -> torch.Tensor:
    """text_fwd_frozen with 16-bit GEMM inputs (see the note above vision_fwd_bf16)."""
    t = cfg
    k = _OPS16[dtype]
    B, T = input_ids.shape
    D, H = t.hidden_size, t.num_attention_heads
    eos = ops.first_eos(input_ids, t.eos_token_id)
    x = _text_stack_bf16(p, input_ids, cfg, cache, len(p.layers) - 1, dtype)
    lp, pre = p.layers[-1], f"t{len(p.layers) - 1}."
    ln1 = k.layernorm(x, lp.ln1_w, lp.ln1_b, t.layer_norm_eps)
    if T <= 512 and os.environ.get("DCLIP_BF16_ROW_ATTN", "1") != "0":
        qkv = k.gemm(ln1, _w16(cache, pre + "qkv", lp.qkv_w, k.cast), bias=lp.qkv_b, out16=True)
        attn16 = k.attention_row(qkv, eos, B, T, H)
    else:
        qkv = k.gemm(ln1, _w16(cache, pre + "qkv", lp.qkv_w, k.cast), bias=lp.qkv_b)
        attn16 = k.cast(ops.attention_row_fwd(qkv, eos, B, T, H))
    x1 = k.gemm(attn16, _w16(cache, pre + "out", lp.out_w, k.cast), bias=lp.out_b,
                residual=ops.gather_rows(x, eos, B, T, D))
    ln2 = k.layernorm(x1, lp.ln2_w, lp.ln2_b, t.layer_norm_eps)
    g = _fc1_act16(k, ln2, _w16(cache, pre + "fc1", lp.fc1_w, k.cast), lp.fc1_b, hidden_act(t))
    rows = k.gemm(g, _w16(cache, pre + "fc2", lp.fc2_w, k.cast), bias=lp.fc2_b, residual=x1)
    return _text_head(rows, p, t.layer_norm_eps)[0]


def text_token_level_bf16(p: TextParams, input_ids: torch.Tensor, cfg, cache: dict, dtype=torch.bfloat16):
    """text_token_level with 16-bit GEMM inputs; the token projection ([B*T,D] x [P,D]) runs in that type too."""
    t = cfg
    k = _OPS16[dtype]
    B, T = input_ids.shape
    x = _text_stack_bf16(p, input_ids, cfg, cache, len(p.layers), dtype)
    ln = k.layernorm(x, p.final_w, p.final_b, t.layer_norm_eps)
    tokens = k.gemm(ln, _w16(cache, "tproj", p.proj_w, k.cast))
    eos = ops.first_eos(input_ids, t.eos_token_id)
    sentence = ops.gather_rows(tokens, eos, B, T, tokens.shape[1])
    return sentence, tokens, eos


def text_token_level(p: TextParams, input_ids: torch.Tensor, cfg):
    """Frozen teacher text pass giving BOTH outputs of one forward (the reference runs the tower twice per caption,
    training/patch_text_aggregation.py:534 and training/CLIP_image_distillation.py:607):
      sentence [B,P]   = text_projection(final_LN(h)[first EOS])                 (text_tokenizer.py:193,:216)
      tokens   [B*T,P] = text_projection(final_LN(h)) for every position          (text_tokenizer.py:202-207)
      eos [B] int32    = first-EOS index; word tokens of caption b are rows 1 .. eos[b]-1."""
    x, _ = text_encoder_fwd(p, input_ids, cfg, save=False)
    return _text_token_tail(x, p, input_ids, cfg)


def text_token_level_split16(p: TextParams, input_ids: torch.Tensor, cfg, cache: dict):
    """text_token_level at precision "fp32-split16" (DESIGN.md §28): EVERY layer is a full layer (every row is an output), its
    four GEMMs on the split-fp16 operands of the text tower's plan (`cache`: the model's _split16_cache, the plan
    text_fwd_frozen_split16 uses), the context written split by the causal attention entry; the final LayerNorm and the
    projection stay fp32.  The plain fp32 pass, bit for bit, when the guard trips."""
    t = cfg
    D = t.hidden_size
    plan = _text_frozen_split16_plan(p, t, cache)
    if plan is None:
        return text_token_level(p, input_ids, cfg)
    B, T = input_ids.shape
    x = ops.text_embed_fwd(input_ids, p.tok, p.pos)
    pc = _layer_pieces(x.shape[0], D, t.intermediate_size, _SPLIT16_FC1_EPI)
    ctx3 = _dense_ctx3(B, T, t.num_attention_heads, True, True)
    for lp, ent in zip(p.layers, plan):
        x = _frozen_split16_layer(x, lp, ent, pc, t.layer_norm_eps, ctx3)
    return _text_token_tail(x, p, input_ids, t)


# --------------------------------------------------------------------------------------------- packed frozen text forward
# The frozen text tower on captions cut after their first EOS and laid back to back: caption n in rows
# cu_seqlens[n] .. cu_seqlens[n+1]-1, Tp rows in all.  The tower is causal and pools at the first EOS, so no result reads a row
# behind it.  As in vision_fwd_packed, LayerNorm, the GEMMs and their epilogues run at M = Tp as they are; the embedding, the
# attention core and the first-EOS gather have ragged forms (ops.text_embed_varlen, ops.attention_varlen_causal_fwd,
# ops.gather_rows_at at `last_rows`).  `tables`: HipCLIPModel._packed_text_tables (host ints max_S / Tp, the two device tables).
# These are forward only; the trainable tower on packed captions (text_fwd_packed / text_bwd_packed) is at the
# end of this file.

def _packed_text_layers(x, layers, n_layers: int, cu, max_S: int, cfg, mode: str, plan=None, cache=None,
                        attn16: Optional[bool] = None, ctx_fused: bool = False):
    """`n_layers` full layers at M = Tp.  mode "fp32" (plan None) / "split16" (plan: _split16_plan's; `ctx_fused`: the context
    leaves the attention kernel split, _packed_ctx3) / "bf16" / "fp16" (cache: the model's weight cache of that type; fp32
    q | k | v for the fp32 packed core, the context is cast — or, with `attn16`, 16-bit q | k | v and context around the packed
    MFMA core, packed_attn16_route)."""
    H, eps, act = cfg.num_attention_heads, cfg.layer_norm_eps, hidden_act(cfg)
    pc = _layer_pieces(x.shape[0], cfg.hidden_size, cfg.intermediate_size, _SPLIT16_FC1_EPI) if mode == "split16" else None
    for li, lp in enumerate(layers[:n_layers]):
        if mode == "fp32":
            ln1, _, _ = ops.layernorm_fwd(x, lp.ln1_w, lp.ln1_b, eps, save_stats=False)
            qkv = ops.gemm(ln1, lp.qkv_w, ops.LAYOUT_NT, bias=lp.qkv_b)
            attn = ops.attention_varlen_causal_fwd(qkv, cu, max_S, H)
            x1 = ops.gemm(attn, lp.out_w, ops.LAYOUT_NT, bias=lp.out_b, residual=x)
            ln2, _, _ = ops.layernorm_fwd(x1, lp.ln2_w, lp.ln2_b, eps, save_stats=False)
            g, _ = _fc1_act_f32(ln2, lp, act)
            x = ops.gemm(g, lp.fc2_w, ops.LAYOUT_NT, bias=lp.fc2_b, residual=x1)
        elif mode == "split16":
            x = _frozen_split16_layer(x, lp, plan[li], pc, eps, _packed_ctx3(cu, max_S, H, True, ctx_fused))
        else:
            k, pre = _OPS16[torch.bfloat16 if mode == "bf16" else torch.float16], f"t{li}."
            ln1 = k.layernorm(x, lp.ln1_w, lp.ln1_b, eps)
            if packed_attn16_route(mode, max_S, False, attn16) == "tiled16":
                qkv = k.gemm(ln1, _w16(cache, pre + "qkv", lp.qkv_w, k.cast), bias=lp.qkv_b, out16=True)
                attn = k.attention_varlen(qkv, cu, max_S, H, True)
            else:
                qkv = k.gemm(ln1, _w16(cache, pre + "qkv", lp.qkv_w, k.cast), bias=lp.qkv_b)                 # fp32 q | k | v
                attn = k.cast(ops.attention_varlen_causal_fwd(qkv, cu, max_S, H))
            x1 = k.gemm(attn, _w16(cache, pre + "out", lp.out_w, k.cast), bias=lp.out_b, residual=x)
            ln2 = k.layernorm(x1, lp.ln2_w, lp.ln2_b, eps)
            g = _fc1_act16(k, ln2, _w16(cache, pre + "fc1", lp.fc1_w, k.cast), lp.fc1_b, act)
            x = k.gemm(g, _w16(cache, pre + "fc2", lp.fc2_w, k.cast), bias=lp.fc2_b, residual=x1)
    return x


def _packed_text_mode(p: TextParams, cfg, precision: str, cache: Optional[dict], what: str, split16: bool):
    """(mode, plan): "fp32" takes the split-fp16 plan exactly when the padded frozen forward would (text_fwd_frozen_split16);
    "fp32-split16" (the token-level pass) whenever the guard lets it, whatever `split16` says."""
    if precision in ("fp32", "fp32-split16"):
        plan = _text_frozen_split16_plan(p, cfg, cache) if (split16 or precision == "fp32-split16") and cache is not None else None
        return ("split16" if plan is not None else "fp32"), plan
    if precision not in ("bf16", "fp16") or cache is None:
        raise ValueError(f"{what}: precision {precision!r} (16-bit precisions need the model's weight cache)")
    return precision, None


def text_fwd_frozen_packed(p: TextParams, input_ids: torch.Tensor, tables: dict, cfg, precision: str = "fp32",
                           cache: Optional[dict] = None, attn16: Optional[bool] = None) -> torch.Tensor:
    """ids [N,T] on the device (the padded matrix: the pads are never read) -> [N,P], the schedule of text_fwd_frozen /
    text_fwd_frozen_split16 / text_fwd_frozen_bf16 at M = Tp: the last layer's attention for the first-EOS row of each caption
    only (keys 0..eos, ops.attention_varlen_causal_fwd(last_only)), everything after it on those N rows.  `cache`: "fp32" the
    model's split-fp16 cache (None: the plain fp32 GEMMs), "bf16" / "fp16" the weight cache of that type.  `attn16`: the 16-bit
    packed attention core for those two (packed_attn16_route; the last layer takes the one-row kernel up to 512 tokens)."""
    t = cfg
    D, H, eps = t.hidden_size, t.num_attention_heads, t.layer_norm_eps
    if not p.layers:
        raise ValueError("text_fwd_frozen_packed: the tower has no encoder layer")
    mode, plan = _packed_text_mode(p, t, precision, cache, "text_fwd_frozen_packed", True)
    cu, last_rows, max_S = tables["cu_seqlens_dev"], tables["last_rows_dev"], tables["max_S"]
    x = ops.text_embed_varlen(input_ids, cu, p.tok, p.pos, tables["Tp"])
    x = _packed_text_layers(x, p.layers, len(p.layers) - 1, cu, max_S, t, mode, plan, cache, attn16)
    lp, li = p.layers[-1], len(p.layers) - 1
    if mode in ("fp32", "split16"):
        if mode == "split16":
            ent = plan[-1]
            ln1 = ops.layernorm_fwd_f16x3(x, lp.ln1_w, lp.ln1_b, eps, 2.0 ** ent["e"]["ln1"],
                                          pieces=split16_pieces([(x.shape[0], 3 * D, D)]))
            qkv = _split16_gemm(ln1, ent, "qkv", "ln1", bias=lp.qkv_b)
        else:
            ln1, _, _ = ops.layernorm_fwd(x, lp.ln1_w, lp.ln1_b, eps, save_stats=False)
            qkv = ops.gemm(ln1, lp.qkv_w, ops.LAYOUT_NT, bias=lp.qkv_b)
        attn = ops.attention_varlen_causal_fwd(qkv, cu, max_S, H, last_only=True)
        rows = _pruned_tail_f32(attn, ops.gather_rows_at(x, last_rows), lp, eps, hidden_act(t))
    else:
        k, pre = _OPS16[torch.bfloat16 if mode == "bf16" else torch.float16], f"t{li}."
        ln1 = k.layernorm(x, lp.ln1_w, lp.ln1_b, eps)
        if packed_attn16_route(mode, max_S, True, attn16) == "row16":
            qkv = k.gemm(ln1, _w16(cache, pre + "qkv", lp.qkv_w, k.cast), bias=lp.qkv_b, out16=True)
            ctx16 = k.attention_varlen_row(qkv, cu, max_S, H, last=True)
        else:
            qkv = k.gemm(ln1, _w16(cache, pre + "qkv", lp.qkv_w, k.cast), bias=lp.qkv_b)                     # fp32 q | k | v
            ctx16 = k.cast(ops.attention_varlen_causal_fwd(qkv, cu, max_S, H, last_only=True))
        x1 = k.gemm(ctx16, _w16(cache, pre + "out", lp.out_w, k.cast), bias=lp.out_b, residual=ops.gather_rows_at(x, last_rows))
        ln2 = k.layernorm(x1, lp.ln2_w, lp.ln2_b, eps)
        g = _fc1_act16(k, ln2, _w16(cache, pre + "fc1", lp.fc1_w, k.cast), lp.fc1_b, hidden_act(t))
        rows = k.gemm(g, _w16(cache, pre + "fc2", lp.fc2_w, k.cast), bias=lp.fc2_b, residual=x1)
    return _text_head(rows, p, eps)[0]


def text_token_level_packed(p: TextParams, input_ids: torch.Tensor, tables: dict, cfg, precision: str = "fp32",
                            cache: Optional[dict] = None, attn16: Optional[bool] = None):
    """text_token_level / text_token_level_bf16 on packed captions: (sentence [N,P], tokens [Tp,P]), every layer at M = Tp;
    the word tokens of caption n are rows cu[n] + 1 .. cu[n+1] - 2, its sentence embedding is row cu[n+1] - 1.  "fp32" runs
    the plain fp32 GEMMs, as text_token_level does; "fp32-split16" (`cache`: the model's split-fp16 text cache) every layer's
    GEMMs on split-fp16 operands with the causal attention-split entry, the final LayerNorm and the projection in fp32
    (text_token_level_split16).  `attn16`: as in text_fwd_frozen_packed (every layer is a full layer)."""
    t = cfg
    mode, plan = _packed_text_mode(p, t, precision, cache, "text_token_level_packed", False)
    cu, last_rows, max_S = tables["cu_seqlens_dev"], tables["last_rows_dev"], tables["max_S"]
    x = ops.text_embed_varlen(input_ids, cu, p.tok, p.pos, tables["Tp"])
    x = _packed_text_layers(x, p.layers, len(p.layers), cu, max_S, t, mode, plan, cache, attn16, ctx_fused=True)
    if mode in ("fp32", "split16"):
        ln, _, _ = ops.layernorm_fwd(x, p.final_w, p.final_b, t.layer_norm_eps, save_stats=False)
        tokens = ops.gemm(ln, p.proj_w, ops.LAYOUT_NT)
    else:
        k = _OPS16[torch.bfloat16 if mode == "bf16" else torch.float16]
        ln = k.layernorm(x, p.final_w, p.final_b, t.layer_norm_eps)
        tokens = k.gemm(ln, _w16(cache, "tproj", p.proj_w, k.cast))
    return ops.gather_rows_at(tokens, last_rows), tokens


# --------------------------------------------------------------------------------------------- trainable text tower, packed
# text_fwd / text_bwd at M = Tp.  d x of the padded tower is exactly zero on every row behind a first EOS, so
# every parameter gradient of the padded rectangle is the sum over the cut captions: the same gradients from Tp rows instead of
# B T.  The layer schedule is layer_fwd / layer_bwd themselves (`varlen`), plain fp32 GEMMs as the padded trainable tower runs.

def text_fwd_packed(p: TextParams, input_ids: torch.Tensor, tables: dict, cfg, save: bool, split16_cache: Optional[dict] = None,
                    split16_out: Optional[list] = None):
    """ids [N,T] on the device (the padded matrix: the pads are never read), `tables` as in text_fwd_frozen_packed -> (out [N,P],
    saved for text_bwd_packed).  `split16_cache`, `split16_out`: as text_fwd's."""
    t = cfg
    H, eps = t.num_attention_heads, t.layer_norm_eps
    cu, last_rows, max_S = tables["cu_seqlens_dev"], tables["last_rows_dev"], tables["max_S"]
    x = ops.text_embed_varlen(input_ids, cu, p.tok, p.pos, tables["Tp"])
    saved_layers = []
    plan, keep = _text_train_split16(p, cfg, save, split16_cache, split16_out)
    for li, lp in enumerate(p.layers):
        x, sv = layer_fwd(x, lp, input_ids.shape[0], max_S, H, True, eps, save, plan[li] if plan is not None else None, keep,
                          varlen=(cu, max_S), act=hidden_act(t))
        saved_layers.append(sv)
    rows = ops.gather_rows_at(x, last_rows)
    out, pooled, mp, rp = _text_head(rows, p, eps, save)
    saved = (input_ids, saved_layers, cu, max_S, tables["Tp"], rows, mp, rp, pooled) if save else None
    return out, saved


def text_bwd_packed(p: TextParams, saved, d_out: torch.Tensor, cfg, need: List[bool], split16=None):
    """text_bwd on what text_fwd_packed saved: the same `need` masks and the same cut-off below the lowest layer asked for.
    `split16`: as text_bwd's; the ragged attention backward has no statistics form, so dqkv takes the three-launch split."""
    t = cfg
    input_ids, saved_layers, cu, max_S, Tp, rows, mp, rp, pooled = saved
    N = input_ids.shape[0]
    names = p.names()
    needd = dict(zip(names, need))
    grads: Dict[str, Optional[torch.Tensor]] = {n: None for n in names}
    drows = _text_tail_bwd(p, d_out, rows, mp, rp, pooled, needd, grads)
    lowest = _lowest_needed(names, needd, TextParams.HEAD, TextParams.TAIL)
    if lowest is None:
        return [grads[n] for n in names]
    dx = ops.scatter_last_rows(drows, cu, Tp)
    dx = _layers_bwd(dx, p.layers, saved_layers, needd, grads, lowest, Tp, N, max_S, t.num_attention_heads, True, t.layer_norm_eps,
                     split16, varlen=(cu, max_S), act=hidden_act(t))
    if lowest < 0:
        dpos = torch.zeros_like(p.pos) if needd["pos"] else None
        dtok = torch.zeros_like(p.tok) if needd["tok"] else None
        grads["tok"], grads["pos"] = ops.text_embed_varlen_bwd(input_ids, cu, dx, dtok, dpos)
    return [grads[n] for n in names]
