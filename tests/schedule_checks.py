"""Cases, references and checkers for the backward SCHEDULES of dclip_amd/engine.py: which gradient each
launch produces and where it is written, under partial `need` masks.  Importable without a GPU; the GPU file
(test_schedule_grads_gpu.py) runs the engine through these, the CPU file (test_schedule_checks_cpu.py) runs a stand-in and
planted faults through the same checkers.

  reference   oracle/dclip_oracle.py (vision_tower / text_tower) in fp64 under torch autograd, objective (out * W).sum();
              for the 16-bit schedules the same oracle with O.linear replaced by RoundedLinear (DESIGN.md §13's rule);
  anchor      E = |got - want|_2 / |want|_2 per ENGINE tensor against a gate made from the reference's own errors;
  exact       completeness, mask consistency (bit-equal except where the table below says another launch makes the value),
              `alloc` (one guarded bucket) and `on_ready` (order, once each, final when reported).
"""
from __future__ import annotations

import math
from typing import Callable, Dict, FrozenSet, Iterable, List, Optional, Sequence

import torch

from oracle import dclip_oracle as O

LAYER_FIELDS = ("ln1_w", "ln1_b", "qkv_w", "qkv_b", "out_w", "out_b", "ln2_w", "ln2_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b")
HEAD = {"vision": ("class_embedding", "patch_w", "pos", "pre_w", "pre_b"), "text": ("tok", "pos")}
TAIL = {"vision": ("post_w", "post_b", "proj_w"), "text": ("final_w", "final_b", "proj_w")}
LINEARS = ("fc2", "fc1", "out", "qkv")                 # in the order a layer's backward meets them
LN_FIELDS = ("ln1_w", "ln1_b", "ln2_w", "ln2_b")

# ------------------------------------------------------------------------------------------------ gates
# fp32 routes:  E <= M32 * E_ref32 + FLOOR32, E_ref32 = the oracle evaluated by torch in fp32 against its fp64 evaluation.
#   M32 = 8: the split-fp16 operands carry 2^-22 where fp32 carries 2^-24 (x4); the MFMA / split-K summation order differs from
#   torch's (x2).  FLOOR32 = 16 * 2^-24: a tensor whose torch-fp32 evaluation happens to land within a few ulps (a short sum)
#   still passes through a chain of fp32 stores on the engine's side — d_out, the tail LayerNorm, two layers of six stored
#   gradients each — and each store is one rounding of 2^-24 relative; 16 of them, added linearly.
# 16-bit routes: E <= M16 * E_emul against the rounded-operand reference, E_emul = that reference against the fp64 oracle.
#   M16 = 4: the roundings of P / dS in the MFMA attention pair and the 16-bit stored activations, which it does not restate.
M32 = 8.0
FLOOR32 = 16 * 2.0 ** -24
M16 = 4.0


# ------------------------------------------------------------------------------------------------ names

def names(tower: str, L: int) -> List[str]:
    """engine.VisionParams.names() / TextParams.names() for L layers."""
    out = list(HEAD[tower])
    for i in range(L):
        out += [f"layers.{i}.{f}" for f in LAYER_FIELDS]
    return out + list(TAIL[tower])


_HF_FIXED = {
    "vision": {"class_embedding": "vision_model.embeddings.class_embedding",
               "patch_w": "vision_model.embeddings.patch_embedding.weight",
               "pos": "vision_model.embeddings.position_embedding.weight",
               "pre_w": "vision_model.pre_layrnorm.weight", "pre_b": "vision_model.pre_layrnorm.bias",
               "post_w": "vision_model.post_layernorm.weight", "post_b": "vision_model.post_layernorm.bias",
               "proj_w": "visual_projection.weight"},
    "text": {"tok": "text_model.embeddings.token_embedding.weight", "pos": "text_model.embeddings.position_embedding.weight",
             "final_w": "text_model.final_layer_norm.weight", "final_b": "text_model.final_layer_norm.bias",
             "proj_w": "text_projection.weight"},
}
_HF_LAYER = {"ln1": "layer_norm1", "ln2": "layer_norm2", "out": "self_attn.out_proj", "fc1": "mlp.fc1", "fc2": "mlp.fc2"}


def hf_keys(tower: str, name: str) -> List[str]:
    """The oracle (HF) keys behind one engine tensor: three for the fused qkv_w / qkv_b, concatenated along dim 0."""
    if name in _HF_FIXED[tower]:
        return [_HF_FIXED[tower][name]]
    _, i, f = name.split(".")
    short, kind = f.rsplit("_", 1)
    suffix = "weight" if kind == "w" else "bias"
    pre = f"{tower}_model.encoder.layers.{i}"
    if short == "qkv":
        return [f"{pre}.self_attn.{p}_proj.{suffix}" for p in "qkv"]
    return [f"{pre}.{_HF_LAYER[short]}.{suffix}"]


def to_engine(tower: str, L: int, by_key: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    return {n: torch.cat([by_key[k] for k in hf_keys(tower, n)], dim=0) if len(hf_keys(tower, n)) > 1 else by_key[hf_keys(tower, n)[0]]
            for n in names(tower, L)}


def engine_tensors(tower: str, L: int, sd: Dict[str, torch.Tensor], device) -> List[torch.Tensor]:
    """The fp32 tensors of engine.VisionParams / TextParams (`from_tensors` order) from an HF-keyed state dict."""
    e = to_engine(tower, L, sd)
    return [e[n].to(device=device, dtype=torch.float32).contiguous() for n in names(tower, L)]


# ------------------------------------------------------------------------------------------------ reference

def output_weighting(shape, seed: int = 11) -> torch.Tensor:
    """The fixed Gaussian W of the objective (out * W).sum(); d_out = W is what the engine's backward receives."""
    return torch.randn(tuple(shape), generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def round_to(x: torch.Tensor, dtype) -> torch.Tensor:
    """Round-to-nearest-even of fp64 values to bf16 / fp16, written out in fp64 arithmetic (no detour through fp32, which
    would round twice): x = m 2^e with m in [0.5, 1); the type keeps p significant bits down to its smallest normal
    exponent and a fixed spacing below it; beyond the largest finite value the result is infinite, as the type's is."""
    p, emin, fmax = {torch.bfloat16: (8, -125, 3.3895313892515355e38), torch.float16: (11, -13, 65504.0)}[dtype]
    assert x.dtype == torch.float64
    x = x.contiguous()
    e = ((x.view(torch.int64) >> 52) & 0x7FF) - 1022               # the exponent field itself: exact on every device
    q = ((torch.clamp(e, min=emin) - p + 1023) << 52).view(torch.float64)         # 2^(e - p), built the same way
    r = torch.round(x / q) * q                                     # torch.round: halves go to the even neighbour
    return torch.where(r.abs() > fmax, torch.sign(r) * math.inf, r)


class RoundedLinear(torch.autograd.Function):
    """DESIGN.md §13's rule for one nn.Linear on 16-bit MFMAs, everything but the operands' rounding exact:
    forward y = r(x) r(w)^T + b;  backward dx = r(dy) r(w), dw = r(dy)^T r(x), db = sum dy."""

    @staticmethod
    def forward(ctx, x, w, b, r):
        xr, wr = r(x), r(w)
        ctx.save_for_backward(xr, wr)
        ctx.r, ctx.has_b = r, b is not None
        y = xr @ wr.transpose(-1, -2)
        return y if b is None else y + b

    @staticmethod
    def backward(ctx, dy):
        xr, wr = ctx.saved_tensors
        dyr = ctx.r(dy)
        dx = dyr @ wr
        dy2, dyr2, x2 = dy.reshape(-1, dy.shape[-1]), dyr.reshape(-1, dy.shape[-1]), xr.reshape(-1, xr.shape[-1])
        return dx, dyr2.t() @ x2, (dy2.sum(0) if ctx.has_b else None), None


def rounded_linear(dtype) -> Callable:
    r = lambda t: round_to(t, dtype)                               # noqa: E731
    return lambda x, w, b=None: RoundedLinear.apply(x, w, b, r)


def _vision_on_grid(p, pixel_values, v, grid):
    """O.vision_tower on another patch grid (gh, gw): the position table resampled as hf interpolate_pos_encoding does
    (bicubic, align_corners=False: kernel_checks_interp.axis_matrix is that resample as a matrix per axis),
    everything else the oracle's own functions."""
    from tests import kernel_checks_interp as ki
    gh, gw = grid
    B, ps, g, D = pixel_values.shape[0], v.patch_size, v.grid, v.hidden_size
    w = p["vision_model.embeddings.patch_embedding.weight"].reshape(D, -1)
    cols = pixel_values.reshape(B, v.num_channels, gh, ps, gw, ps).permute(0, 2, 4, 1, 3, 5).reshape(B, gh * gw, -1)
    patches = cols @ w.t()
    pos = p["vision_model.embeddings.position_embedding.weight"]
    ah = torch.as_tensor(ki.axis_matrix(g, gh), dtype=pos.dtype, device=pos.device)
    aw = torch.as_tensor(ki.axis_matrix(g, gw), dtype=pos.dtype, device=pos.device)
    table = torch.einsum("ia,jb,abd->ijd", ah, aw, pos[1:].reshape(g, g, D)).reshape(gh * gw, D)
    x = torch.cat([p["vision_model.embeddings.class_embedding"].expand(B, 1, -1), patches], dim=1) + torch.cat([pos[:1], table], dim=0)
    x = O.layer_norm(x, p["vision_model.pre_layrnorm.weight"], p["vision_model.pre_layrnorm.bias"], v.layer_norm_eps)
    for i in range(v.num_hidden_layers):
        x = O.clip_encoder_layer(x, p, f"vision_model.encoder.layers.{i}", v.num_attention_heads, False, v.layer_norm_eps)
    pooled = O.layer_norm(x[:, 0, :], p["vision_model.post_layernorm.weight"], p["vision_model.post_layernorm.bias"], v.layer_norm_eps)
    return O.linear(pooled, p["visual_projection.weight"])


def reference(tower: str, cfg, sd: Dict[str, torch.Tensor], inputs: torch.Tensor, W: torch.Tensor, dtype=torch.float64,
              device="cpu", linear: Optional[Callable] = None, grid=None) -> Dict[str, torch.Tensor]:
    """{engine name: d (out * W).sum() / d tensor} (fp64, CPU) of the oracle evaluated in `dtype` on `device` by torch autograd;
    `linear` replaces O.linear for the evaluation (rounded_linear(...)).  `cfg` is the tower's config.  The text tower's
    causal mask is built on the CPU by the oracle, so it is evaluated there."""
    L = cfg.num_hidden_layers
    keys = [k for n in names(tower, L) for k in hf_keys(tower, n)]
    p = {k: sd[k].detach().to(device=device, dtype=dtype).requires_grad_(True) for k in keys}
    x = inputs.to(device) if tower == "text" else inputs.to(device=device, dtype=dtype)
    saved = O.linear
    try:
        if linear is not None:
            O.linear = linear
        if tower == "text":
            out = O.text_tower(p, x, cfg)
        else:
            out = O.vision_tower(p, x, cfg) if grid is None else _vision_on_grid(p, x, cfg, grid)
        (out * W.to(device=device, dtype=dtype)).sum().backward()
    finally:
        O.linear = saved
    got = to_engine(tower, L, {k: t.grad.detach().double().cpu() for k, t in p.items()})
    for n, g in got.items():
        assert float(g.norm()) > 0.0, f"the reference gradient of {n} is zero: E is undefined for it"
    return got


def _flat_pair(a: torch.Tensor, b: torch.Tensor):
    a = a.detach().reshape(-1)
    return a, b.detach().reshape(-1).to(a.device)


def rel_err(got: torch.Tensor, want: torch.Tensor) -> float:
    got, want = _flat_pair(got, want)                  # on the device of `got`: the wide shapes are not copied to the host
    assert got.shape == want.shape, (got.shape, want.shape)
    return float((got.double() - want.double()).norm() / want.double().norm())


def errors(got: Dict[str, torch.Tensor], want: Dict[str, torch.Tensor]) -> Dict[str, float]:
    return {n: rel_err(got[n], want[n]) for n in want}


def gates32(e_ref32: Dict[str, float]) -> Dict[str, float]:
    return {n: M32 * e + FLOOR32 for n, e in e_ref32.items()}


def gates16(e_emul: Dict[str, float]) -> Dict[str, float]:
    return {n: M16 * e for n, e in e_emul.items()}


def check_anchor(got: Dict[str, Optional[torch.Tensor]], want: Dict[str, torch.Tensor], gate: Dict[str, float], what: str) -> Dict[str, float]:
    """Every gradient that exists against the reference.  Returns {name: E / gate}; one AssertionError names every failure."""
    ratios, bad = {}, []
    for n, g in got.items():
        if g is None:
            continue
        e = rel_err(g.reshape(want[n].shape), want[n])
        ratios[n] = e / gate[n]
        if not e <= gate[n]:
            bad.append(f"{n}: E {e:.3e} > gate {gate[n]:.3e}")
    assert not bad, f"{what}: " + "; ".join(bad)
    return ratios


# ------------------------------------------------------------------------------------------------ masks

def _layer(i: int, fields: Iterable[str]) -> List[str]:
    return [f"layers.{i}.{f}" for f in fields]


def masks(tower: str, L: int, freeze: Optional[Dict[str, FrozenSet[str]]] = None) -> Dict[str, FrozenSet[str]]:
    """{case id: the needed engine names}.  Layers are 0 (bottom) .. L-1 (top).  `freeze`: the product's own sets for this
    tower, {"north_star": ..., "as_written": ...} as CLIPImageDistillation.set_freeze_mode leaves requires_grad (freeze_sets);
    a set that is empty (the frozen text tower) or equal to (a) is not listed twice."""
    allw = ["proj_w"] + [f"layers.{i}.{l}_w" for i in range(L) for l in LINEARS]     # patch_w is the head's: (h)
    ln_tail = TAIL[tower][:2]
    m: Dict[str, FrozenSet[str]] = {}
    m["a_everything"] = frozenset(names(tower, L))
    m["b_proj_w"] = frozenset(["proj_w"])
    m["c_tail_ln"] = frozenset(ln_tail)
    if L == 3:                                          # the one case with a middle layer
        return {"a_everything": m["a_everything"], "k_middle_fc2_b_out_b": frozenset(_layer(1, ["fc2_b", "out_b"]))}
    m["d_top_fc2_b"] = frozenset(_layer(L - 1, ["fc2_b"]))
    m["e_bottom_fc2_b"] = frozenset(_layer(0, ["fc2_b"]))
    m["f_weights"] = frozenset(allw)
    biases = [n for n in names(tower, L) if "." in n and (n.endswith("_b") or n.split(".")[-1] in LN_FIELDS)]
    m["g_biases_ln"] = frozenset(biases + list(ln_tail) + (["pre_w", "pre_b"] if tower == "vision" else []))
    if tower == "vision":
        m["h_pos"] = frozenset(["pos"])
        m["h_class_embedding"] = frozenset(["class_embedding"])
        m["h_patch_w"] = frozenset(["patch_w"])
        m["h_head"] = frozenset(HEAD["vision"])
    else:
        m["h_tok"] = frozenset(["tok"])
        m["h_pos"] = frozenset(["pos"])
    m["i_top_layer"] = frozenset(_layer(L - 1, LAYER_FIELDS))
    for mode, s in sorted((freeze or {}).items()):
        if s and s != m["a_everything"]:
            m[f"j_{mode}"] = frozenset(s)
    return m


def freeze_sets(tower: str, L: int, model) -> Dict[str, FrozenSet[str]]:
    """What CLIPImageDistillation.set_freeze_mode makes trainable in one tower of `model` (a HipCLIPModel; CPU is enough),
    as engine names — taken from the product's rule, not retyped."""
    from types import SimpleNamespace
    from dclip_amd.CLIP_image_distillation import CLIPImageDistillation
    holder = SimpleNamespace(student=model, teacher=torch.nn.Module(), freeze_mode=None)
    out = {}
    for mode in ("north_star", "as_written"):
        CLIPImageDistillation.set_freeze_mode(holder, mode)
        p = model.vision_params() if tower == "vision" else model.text_params()
        assert p.names() == names(tower, L)
        out[mode] = frozenset(n for n, t in zip(p.names(), p.tensors()) if t.requires_grad)
    for t in model.parameters():
        t.requires_grad = True
    return out


def lowest_of(tower: str, mask: Iterable[str]) -> Optional[int]:
    """The engine's `lowest`: None = nothing below the tail is needed; -1 = the head; else the lowest layer needed."""
    low = None
    for n in mask:
        if n in TAIL[tower]:
            continue
        li = -1 if n in HEAD[tower] else int(n.split(".")[1])
        low = li if low is None else min(low, li)
    return low


def layers_run(tower: str, mask: Iterable[str], L: int) -> List[int]:
    low = lowest_of(tower, mask)
    return [] if low is None else list(range(L - 1, max(low, 0) - 1, -1))


def _situations_all() -> List[str]:
    s = ["early_return.proj_w", "early_return.tail_ln", "tail.everything",
         "lowest.top.fc2_b_alone", "lowest.top.full_layer", "lowest.middle", "lowest.bottom", "lowest.head",
         "fc2_b.top_own_colsum", "fc2_b.from_above", "fc2_b.from_above.alone", "below.not_allocated",
         "layer.nothing_needed", "vision.layer.attention_projections_only", "layer.ln.want", "layer.ln.skip",
         "side_stream.busy", "side_stream.idle"]
    s += [f"{l}.{k}" for l in LINEARS for k in ("both", "w_only", "b_only", "none")]
    s += ["head.ln.want", "head.ln.skip",
          "vision.head.pos_only", "vision.head.class_embedding_only", "vision.head.pos_and_class_embedding", "vision.head.no_colsum",
          "vision.head.patch_w", "vision.head.no_patch_w", "vision.head.patch_w_without_colsum", "vision.head.everything_under_frozen_layers",
          "text.head.tok_only", "text.head.pos_only", "text.head.tok_and_pos"]
    return s


ALL_SITUATIONS = tuple(_situations_all())


def situations_of_tower(tower: str) -> FrozenSet[str]:
    """Every situation mask_situations can name for a tower (the other tower's head forms and, for the text tower, which
    has no head LayerNorm, the head.ln pair left out)."""
    other = "text" if tower == "vision" else "vision"
    return frozenset(s for s in ALL_SITUATIONS if not s.startswith(other + ".") and not (tower == "text" and s.startswith("head.ln")))


def mask_situations(tower: str, mask: Iterable[str], L: int) -> FrozenSet[str]:
    """The branch situations of the backward schedules (vision_bwd, vision_bwd_bf16, text_bwd and the layer schedules under
    them) that a `need` mask reaches, read off engine.py.  Pure; returns names from ALL_SITUATIONS only."""
    mask = frozenset(mask)
    s = set()
    tail_ln = any(n in mask for n in TAIL[tower][:2])
    low = lowest_of(tower, mask)
    if low is None:
        if "proj_w" in mask:
            s.add("early_return.proj_w")
        if tail_ln:
            s.add("early_return.tail_ln")
        return frozenset(s)
    if "proj_w" in mask and tail_ln:
        s.add("tail.everything")
    run = layers_run(tower, mask, L)
    bottom = run[-1]
    need = {i: {f for f in LAYER_FIELDS if f"layers.{i}.{f}" in mask} for i in run}
    if low == L - 1:
        if need[low] == {"fc2_b"}:
            s.add("lowest.top.fc2_b_alone")
        if need[low] == set(LAYER_FIELDS):
            s.add("lowest.top.full_layer")
    elif low > 0:
        s.add("lowest.middle")
    elif low == 0:
        s.add("lowest.bottom")
    else:
        s.add("lowest.head")
    for i in run:
        nd = need[i]
        if not nd:
            s.add("layer.nothing_needed")
        if nd == {"qkv_w", "qkv_b", "out_w", "out_b"}:
            s.add("vision.layer.attention_projections_only")
        for ln in ("ln1", "ln2"):
            s.add("layer.ln.want" if (ln + "_w" in nd or ln + "_b" in nd) else "layer.ln.skip")
        for l in LINEARS:
            w, b = l + "_w" in nd, l + "_b" in nd
            s.add(f"{l}." + ("both" if w and b else "w_only" if w else "b_only" if b else "none"))
        s.add("side_stream.busy" if any(l + "_w" in nd for l in LINEARS) else "side_stream.idle")
        if "fc2_b" in nd:
            if i == L - 1:
                s.add("fc2_b.top_own_colsum")
            else:
                s.add("fc2_b.from_above")
                if nd == {"fc2_b"}:
                    s.add("fc2_b.from_above.alone")
        if i > bottom and "fc2_b" not in need[i - 1]:
            s.add("below.not_allocated")
    if low < 0:
        hd = {n for n in HEAD[tower] if n in mask}
        if tower == "vision":
            s.add("head.ln.want" if ("pre_w" in hd or "pre_b" in hd) else "head.ln.skip")
            pos, ce = "pos" in hd, "class_embedding" in hd
            s.add("vision.head.pos_and_class_embedding" if pos and ce else "vision.head.pos_only" if pos else
                  "vision.head.class_embedding_only" if ce else "vision.head.no_colsum")
            s.add("vision.head.patch_w" if "patch_w" in hd else "vision.head.no_patch_w")
            if "patch_w" in hd and not pos and not ce:
                s.add("vision.head.patch_w_without_colsum")
            if hd == set(HEAD["vision"]) and all(not need[i] for i in run):
                s.add("vision.head.everything_under_frozen_layers")
        else:
            s.add("text.head.tok_and_pos" if hd == {"tok", "pos"} else "text.head.tok_only" if "tok" in hd else "text.head.pos_only")
    assert s <= set(ALL_SITUATIONS), s - set(ALL_SITUATIONS)
    return frozenset(s)


# ------------------------------------------------------------------------------------------------ exact checkers

def check_completeness(got: Dict[str, Optional[torch.Tensor]], mask: Iterable[str], all_names: Sequence[str], what: str):
    """A gradient exists exactly where `need` is true and is None elsewhere."""
    mask = frozenset(mask)
    assert list(got) == list(all_names), f"{what}: the result is not in names() order"
    extra = [n for n in all_names if got[n] is not None and n not in mask]
    missing = [n for n in all_names if got[n] is None and n in mask]
    assert not extra, f"{what}: a gradient was returned for a parameter that is not needed: {extra}"
    assert not missing, f"{what}: a needed gradient is missing: {missing}"


def check_text_pos_tail(dpos: torch.Tensor, T: int, what: str):
    """Captions of T < max_position_embeddings tokens never read the position rows T..: their gradient is exactly zero."""
    tail = dpos.detach().cpu()[T:]
    assert tail.numel() == 0 or not bool((tail != 0).any()), f"{what}: rows {T}.. of the position gradient are not zero"


def check_layers_run(ran: Sequence[int], tower: str, mask: Iterable[str], L: int, what: str):
    """Nothing below `lowest` is run: the layer schedules were entered for exactly L-1 .. max(lowest, 0), top down."""
    want = layers_run(tower, mask, L)
    assert list(ran) == want, f"{what}: layer backwards ran for layers {list(ran)}, the mask needs {want}"


# Which launch produces a gradient depends on the mask in ONE place: the bias gradient of a linear layer on the fp32 routes
# (engine.linear_param_grads).  Everything else is produced by the same launch whatever else is needed.
#
#   route                         weight also needed                         weight not needed
#   fp32 plain                    the weight-gradient GEMM's A_ROWSUM        ops.colsum
#   fp32 split-fp16 wgrad (§9f)   the fused split pass (rows_colstats, db)   ops.colsum
#   16-bit transposing            the same launch either way (fc2_b: colsum of dx2 / of the layer above's dx; fc1_b: rowsum of
#   16-bit token-major            dh^T / colsum of dh16; out_b, qkv_b: colsum / LayerNorm's dx_colsum) — no exception
#
# So against the full mask a bias is an exception exactly when the partial mask lacks that linear's weight.
#
# One gradient differs between two runs of the SAME mask: the text tower's `tok` (text_embed_bwd, float atomics in no fixed
# order).  It is an exception under every mask, with embed_atomic_bound.

def bias_exceptions(route_is_fp32: bool, mask: Iterable[str], full: Iterable[str]) -> FrozenSet[str]:
    if not route_is_fp32:
        return frozenset()
    mask, full = frozenset(mask), frozenset(full)
    out = set()
    for n in mask:
        f = n.split(".")[-1]
        if "." in n and f.endswith("_b") and f[:-2] in LINEARS:
            w = n[:-1] + "w"
            if w in full and w not in mask:
                out.add(n)
    return frozenset(out)


def colsum_bound(rows: int, abs_colsum: torch.Tensor) -> torch.Tensor:
    """Two fp32 column sums of the same `rows` values in different orders: each is within rows * 2^-24 * sum|x| of the exact
    sum (the derivation of §25's db); the same figure bounds their difference here."""
    return rows * 2.0 ** -24 * abs_colsum.detach().double()


def embed_atomic_bound(input_ids: torch.Tensor, dx: torch.Tensor, vocab: int) -> torch.Tensor:
    """The one gradient that is not the same from run to run: text_embed_bwd adds the rows of dx [B*T, D] into dtok[id] with
    float atomics, in no fixed order.  A row that c positions share is a sum of c fp32 values in some order, within
    c * 2^-24 * sum|x| of the exact sum per element (the column-sum bound with rows = c); a row met once is exact, a row never
    met stays zero — the bound is 2^-24 |x| and 0 there, and those differences are 0."""
    ids = input_ids.reshape(-1).to(dx.device)
    D = dx.shape[-1]
    a = torch.zeros((vocab, D), dtype=torch.float64, device=dx.device).index_add_(0, ids, dx.detach().reshape(-1, D).abs().double())
    c = torch.zeros((vocab,), dtype=torch.float64, device=dx.device).index_add_(0, ids, torch.ones_like(ids, dtype=torch.float64))
    return c[:, None] * 2.0 ** -24 * a


def check_mask_consistency(partial: Dict[str, Optional[torch.Tensor]], full: Dict[str, torch.Tensor], exceptions: Iterable[str],
                           bounds: Dict[str, torch.Tensor], what: str):
    """Every gradient produced under a partial mask against the same gradient under the full mask (same route, input and
    d_out): bit-equal, except the listed exceptions, which hold the column-sum bound of `bounds[name]`.  The entry "dx" (the
    data gradient the lowest layer that ran returned) is compared the same way when both sides have it."""
    exceptions = frozenset(exceptions)
    bad = []
    for n, g in partial.items():
        if g is None:
            continue
        f = full[n]
        assert f is not None, f"{what}: {n} is missing from the full-mask run"
        a, b = _flat_pair(g, f)
        if n in exceptions:
            d = (a.double() - b.double()).abs()
            bound = bounds[n].reshape(-1).to(d.device)
            over = d > bound
            if bool(over.any()):
                bad.append(f"{n}: another launch, but {int(over.sum())} columns differ by more than the column-sum bound "
                           f"(worst {float((d / bound.clamp_min(1e-300)).max()):.2f} x)")
        elif not torch.equal(a, b):
            bad.append(f"{n}: not bit-equal to the full-mask run (max |diff| {float((a.double() - b.double()).abs().max()):.3e})")
    assert not bad, f"{what}: " + "; ".join(bad)


class Bucket:
    """One NaN-filled fp32 allocation holding a slice per parameter gradient, NaN guard bands between the slices — what
    dist.GradSync's bucket is to the schedules.  `alloc(name, shape)` is the engine's callback."""
    GUARD = 64                                           # floats; slices start 256-byte aligned, as GradSync's do

    def __init__(self, sizes: Dict[str, int], device="cpu"):
        self.off, at = {}, self.GUARD
        for n, numel in sizes.items():
            self.off[n] = (at, numel)
            at += (numel + self.GUARD - 1) // self.GUARD * self.GUARD + self.GUARD
        self.buf = torch.full((at,), float("nan"), dtype=torch.float32, device=device)
        self.sentinel = int(self.buf[:1].view(torch.int32).item())
        self.handed: Dict[str, torch.Tensor] = {}

    def alloc(self, name: str, shape):
        assert name in self.off, f"alloc was asked for an unknown name {name!r}"
        assert name not in self.handed, f"alloc was asked twice for {name}"
        at, numel = self.off[name]
        assert math.prod(shape) == numel, f"alloc({name}, {tuple(shape)}): the parameter has {numel} elements"
        self.handed[name] = self.buf[at:at + numel].view(*shape)
        return self.handed[name]

    def check(self, got: Dict[str, Optional[torch.Tensor]], baseline: Dict[str, Optional[torch.Tensor]], what: str):
        """Every gradient was handed a slice and lives there; no NaN is left in a handed slice; everything outside the
        handed slices is untouched; the values equal the alloc=None run bit for bit."""
        for n, g in got.items():
            if g is None:
                assert n not in self.handed, f"{what}: a slice was taken for {n}, which has no gradient"
                continue
            assert n in self.handed, f"{what}: {n} was never given its slice"
            assert g.data_ptr() == self.handed[n].data_ptr() and g.numel() == self.handed[n].numel(), \
                f"{what}: {n} was returned in a tensor of its own, not in its slice"
            assert not bool(torch.isnan(self.handed[n]).any()), f"{what}: NaN left inside the slice of {n}"
            assert torch.equal(*_flat_pair(g, baseline[n])), \
                f"{what}: {n} written into its slice differs from the run without alloc"
        outside = self.buf.view(torch.int32).clone()
        for n in self.handed:
            at, numel = self.off[n]
            outside[at:at + numel] = self.sentinel
        touched = (outside != self.sentinel).nonzero().flatten()[:4].cpu().tolist()
        if touched:
            near = sorted({min(self.off.items(), key=lambda kv: min(abs(kv[1][0] - i), abs(kv[1][0] + kv[1][1] - i)))[0] for i in touched})
            raise AssertionError(f"{what}: memory outside the handed slices was written at float offsets {touched} (next to {near})")


class ReadyLog:
    """The `on_ready` callback: keeps every reported group and a clone of each gradient taken at that moment (enqueued on the
    current stream, so it sees exactly what a collective started there would see)."""

    def __init__(self):
        self.groups: List[Dict[str, torch.Tensor]] = []
        self.clones: List[Dict[str, torch.Tensor]] = []

    def __call__(self, named: Dict[str, torch.Tensor]):
        self.groups.append(dict(named))
        self.clones.append({n: t.clone() for n, t in named.items()})

    def check(self, got: Dict[str, Optional[torch.Tensor]], tower: str, mask: Iterable[str], L: int, what: str):
        """Each needed name once and no other; groups in the documented order — the tail, each layer that runs from the top
        down, the head if it runs; what was cloned inside the callback equals the final gradient bit for bit."""
        mask = frozenset(mask)
        run = layers_run(tower, mask, L)
        low = lowest_of(tower, mask)
        slots = [set(TAIL[tower])] + [set(_layer(i, LAYER_FIELDS)) for i in run] + ([set(HEAD[tower])] if low is not None and low < 0 else [])
        seen: Dict[str, int] = {}
        for g in self.groups:
            for n in g:
                seen[n] = seen.get(n, 0) + 1
        twice = sorted(n for n, c in seen.items() if c > 1)
        assert not twice, f"{what}: reported more than once: {twice}"
        assert len(self.groups) == len(slots), f"{what}: {len(self.groups)} groups reported, the schedule has {len(slots)}"
        for k, (g, slot) in enumerate(zip(self.groups, slots)):
            stray = sorted(set(g) - slot)
            assert not stray, f"{what}: group {k} carries {stray}: groups come tail first, then the layers top down, then the head"
        assert set(seen) == mask, f"{what}: reported {sorted(set(seen) - mask)} unasked, never reported {sorted(mask - set(seen))}"
        for g, c in zip(self.groups, self.clones):
            for n in g:
                assert got[n] is not None and g[n].data_ptr() == got[n].data_ptr(), f"{what}: {n} was reported in another tensor than the one returned"
                assert torch.equal(*_flat_pair(c[n], got[n])), \
                    f"{what}: {n} was reported before its last write (the value seen in the callback is not the final one)"


# ------------------------------------------------------------------------------------------------ the single-pass census
# What the split-fp16 backward (engine._layers_bwd / layer_bwd / last_layer_bwd_cls / linear_param_grads) calls for the four
# linears of every layer it runs, written down from the documented rules (§9f, §9g, §30) and NOT from running the engine:
#
#   * a linear whose weight is needed, at full row count, whose shape the weight-gradient plan takes -> the split pass;
#     it is the SINGLE pass (ops.split_f16x3_rows_cols_stats) iff the statistics regime is on and the kernel that produces its dY
#     has a statistics form on this route, the THREE-launch pass (ops.split_f16x3_rows_colstats) otherwise.  Producers:
#       fc2   the ln1 backward of the layer ABOVE (layer_bwd's or last_layer_bwd_cls's) — none for the top layer, whose dY comes
#             from scatter_rows / scatter_last_rows;
#       fc1   fc2's data-gradient GEMM;          out   the ln2 backward;
#       qkv   the dense attention backward in its "stats" (S <= 64) or "rows_stats" (causal, 65 .. 80) form — none for the pruned
#             vision top layer (attention_cls_bwd), none on the packed tower, none in the "segments" form (the twin switched off);
#     its bias comes out of that pass (db), except in the "segments" form with the regime on: ops.colsum_segments;
#   * a weight needed where the plan does not take it (rows not a multiple of 64, a stale plan) -> the fp32 GEMM (LAYOUT_TN);
#     the bias, if needed too, is its A_ROWSUM epilogue: no column sum.  The M = B linears of the pruned top layer are such
#     GEMMs too, but not at full row count: not counted;
#   * a bias needed without its weight -> one ops.colsum, whatever the plan says.

PASS_KEYS = ("single", "three", "plain_w", "colsum", "segments")
PRODUCER_KINDS = ("gemm", "ln", "attn")


def split_census(tower: str, mask: Iterable[str], L: int, *, pruned: bool, packed: bool, dystats: bool, attn_form: Optional[str],
                 wgrad_plan_ok: bool) -> List[Dict[str, object]]:
    """One record per (layer run, linear), top down, fc2 / fc1 / out / qkv: {"layer", "linear", "pass": "single" / "three" / None,
    "producer": "gemm" / "ln" / "attn" / None (of a single pass), "produced_in": the layer whose backward launches that producer,
    "plain_w", "colsum", "segments": bool, "db": where a needed bias comes from ("pass" / "segments" / "rowsum" / "colsum" / None)}.
    `pruned`: the vision tower's top layer is last_layer_bwd_cls; `packed`: the ragged text tower; `dystats`: the switch is on and
    _dystats_regime holds for the tower; `attn_form`: _attention_bwd_stats_form's first answer for the dense tower ("stats",
    "rows_stats", "segments", None); `wgrad_plan_ok`: the plan is fresh and takes the four weight-gradient shapes."""
    mask = frozenset(mask)
    assert attn_form in ("stats", "rows_stats", "segments", None), attn_form
    assert not (packed and tower != "text") and not (pruned and tower != "vision")
    out = []
    for i in layers_run(tower, mask, L):
        top = i == L - 1
        cls = pruned and top
        for l in LINEARS:
            w, b = f"layers.{i}.{l}_w" in mask, f"layers.{i}.{l}_b" in mask
            full_size = l == "qkv" or not cls
            d = {"layer": i, "linear": l, "pass": None, "producer": None, "produced_in": None, "plain_w": False, "colsum": False,
                 "segments": False, "db": None}
            if w and full_size and wgrad_plan_ok:
                if l == "fc2":
                    form = None if top else "ln"
                elif l == "fc1":
                    form = "gemm"
                elif l == "out":
                    form = "ln"
                else:
                    form = "attn" if not cls and not packed and attn_form in ("stats", "rows_stats") else None
                if not dystats:
                    form = None
                d["pass"], d["producer"] = ("single" if form else "three"), form
                if form:
                    d["produced_in"] = i + 1 if l == "fc2" else i
                d["segments"] = bool(l == "qkv" and b and dystats and not cls and not packed and attn_form == "segments")
                d["db"] = ("segments" if d["segments"] else "pass") if b else None
            elif w:
                d["plain_w"] = full_size
                d["db"] = "rowsum" if b else None
            elif b:
                d["colsum"], d["db"] = True, "colsum"
            out.append(d)
    return out


def expected_passes(tower: str, mask: Iterable[str], L: int, *, pruned: bool, packed: bool, dystats: bool, attn_form: Optional[str],
                    wgrad_plan_ok: bool) -> Dict[str, int]:
    """Calls inside linear_param_grads during one backward: "single" ops.split_f16x3_rows_cols_stats, "three"
    ops.split_f16x3_rows_colstats, "plain_w" fp32 weight-gradient ops.gemm(.., LAYOUT_TN) at full row count, "colsum" ops.colsum
    for a bias, "segments" ops.colsum_segments (split_census, summed)."""
    c = split_census(tower, mask, L, pruned=pruned, packed=packed, dystats=dystats, attn_form=attn_form, wgrad_plan_ok=wgrad_plan_ok)
    return {"single": sum(d["pass"] == "single" for d in c), "three": sum(d["pass"] == "three" for d in c),
            "plain_w": sum(d["plain_w"] for d in c), "colsum": sum(d["colsum"] for d in c), "segments": sum(d["segments"] for d in c)}


def expected_producers(tower: str, mask: Iterable[str], L: int, **route) -> Dict[int, Dict[str, int]]:
    """{layer whose backward launches them: {"gemm", "ln", "attn": statistics-producing launches}} — one per single pass and none
    else: statistics are never produced without a consumer.  Layers without any are left out."""
    out: Dict[int, Dict[str, int]] = {}
    for d in split_census(tower, mask, L, **route):
        if d["producer"]:
            k = out.setdefault(d["produced_in"], {k: 0 for k in PRODUCER_KINDS})
            k[d["producer"]] += 1
    return out


def check_census(calls: Dict[str, int], producers: Dict[int, Dict[str, int]], tower: str, mask: Iterable[str], L: int, what: str,
                 **route):
    """The counted calls and the statistics-producing launches per layer against the census."""
    want = expected_passes(tower, mask, L, **route)
    assert {k: calls.get(k, 0) for k in PASS_KEYS} == want, f"{what}: calls {dict(calls)}, the census says {want}"
    wantp = expected_producers(tower, mask, L, **route)
    gotp = {i: {k: v.get(k, 0) for k in PRODUCER_KINDS} for i, v in producers.items() if any(v.values())}
    assert gotp == wantp, f"{what}: statistics were produced in {gotp} (layer: kind: launches), the single passes need {wantp}"


SPLIT_SITUATIONS = ("split.w_only", "split.both", "split.b_only_live_plan", "producer.consumer_below", "producer.consumer_not_run",
                    "producer.in_layer_without_split_pass", "regime_on.nothing_asked", "segments.with_b", "segments.without_b")


def split_situations(tower: str, mask: Iterable[str], L: int, **route) -> FrozenSet[str]:
    """The branch situations of the split-fp16 backward that a mask reaches on a route (split_census's keywords): weight without
    bias on the split pass (the kernels are handed db=None) and with it; a bias without its weight while the layer's plan is live;
    a producer whose consumer is the fc2 of the layer below; a layer that is the lowest run although a layer lies below it (its
    ln1 backward must NOT be asked: i - 1 < bottom); a layer that produces for the layer below and takes no split pass itself; a
    backward in the regime that asks no producer at all; the "segments" form with and without the bias."""
    mask = frozenset(mask)
    c = split_census(tower, mask, L, **route)
    run = layers_run(tower, mask, L)
    s = set()
    for d in c:
        b = f"layers.{d['layer']}.{d['linear']}_b" in mask
        if d["pass"]:
            s.add("split.both" if b else "split.w_only")
        if d["colsum"] and route["wgrad_plan_ok"]:
            s.add("split.b_only_live_plan")
        if d["linear"] == "fc2" and d["producer"]:
            s.add("producer.consumer_below")
            if not any(e["pass"] for e in c if e["layer"] == d["produced_in"]):
                s.add("producer.in_layer_without_split_pass")
        if d["linear"] == "qkv" and route["attn_form"] == "segments" and d["pass"] and route["dystats"]:
            s.add("segments.with_b" if b else "segments.without_b")
    if run and run[-1] > 0 and route["dystats"] and route["wgrad_plan_ok"]:
        s.add("producer.consumer_not_run")
    if run and route["dystats"] and route["wgrad_plan_ok"] and not any(d["producer"] for d in c):
        s.add("regime_on.nothing_asked")
    assert s <= set(SPLIT_SITUATIONS)
    return frozenset(s)


def split_masks(tower: str, L: int) -> Dict[str, FrozenSet[str]]:
    """Masks the split-fp16 routes add to masks(): (m) the top layer's fc2_b and the bottom layer's fc2_w alone — the top layer takes
    no split pass and still has to produce the partials of the fc2 below, which gets no bias (db=None)."""
    return {"m_top_fc2_b_bottom_fc2_w": frozenset([f"layers.{L - 1}.fc2_b", "layers.0.fc2_w"])}
