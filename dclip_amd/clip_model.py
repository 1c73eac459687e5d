"""`HipCLIPModel`: the student / teacher CLIP towers behind the call surface the reference uses on HF
`CLIPModel`:

    model.get_image_features(pixel_values=Tensor[B,3,H,W]) -> Tensor[B,P]      (CLIP_image_distillation.py:601)
    model.get_text_features(input_ids=LongTensor[B,T], attention_mask=ignored) -> Tensor[B,P]   (:616)
    model.vision_model.named_parameters() / model.text_model.parameters()       (:504, :754)
    model.state_dict() / load_state_dict()  with HF key names (q_proj/k_proj/v_proj kept SEPARATE on disk)

Both calls return plain tensors (transformers 4.x semantics, which the reference's `.float()` calls assume).
In memory q/k/v are one fused [3D, D] parameter named `...self_attn.qkv_proj.{weight,bias}` — it contains
"proj", so the reference's freeze rule `if "proj" not in name: requires_grad = False` (:504-506) selects
exactly the same tensors as it does on the HF module.  state-dict hooks split / merge the fused tensor.

All arithmetic runs in the HIP library; there is no PyTorch fallback (importing works on CPU for
checkpoint handling, calling a tower without the GPU library raises).
"""
from __future__ import annotations

from typing import List, Optional

import torch
import torch.nn as nn

from . import engine, functional, ops
from .config import ClipConfig, TextConfig, VisionConfig


class _Affine(nn.Module):
    """Holder with HF-compatible `.weight` / `.bias` names (LayerNorm or Linear parameters)."""

    def __init__(self, w_shape, bias: bool = True, ones: bool = False):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(w_shape) if ones else torch.zeros(w_shape))
        if bias:
            self.bias = nn.Parameter(torch.zeros(w_shape[0]))
        else:
            self.register_parameter("bias", None)


class _Table(nn.Module):
    def __init__(self, rows, dim):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(rows, dim))


class HipSelfAttention(nn.Module):
    def __init__(self, dim: int):
        super().__init__()
        self.dim = dim
        self.qkv_proj = _Affine((3 * dim, dim))
        self.out_proj = _Affine((dim, dim))
        self._register_state_dict_hook(self._split_qkv)
        self._register_load_state_dict_pre_hook(self._merge_qkv)

    @staticmethod
    def _split_qkv(module, state_dict, prefix, local_metadata):
        D = module.dim
        for kind in ("weight", "bias"):
            fused = state_dict.pop(f"{prefix}qkv_proj.{kind}")
            for i, n in enumerate(("q_proj", "k_proj", "v_proj")):
                state_dict[f"{prefix}{n}.{kind}"] = fused[i * D:(i + 1) * D]
        return state_dict

    def _merge_qkv(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        for kind in ("weight", "bias"):
            keys = [f"{prefix}{n}.{kind}" for n in ("q_proj", "k_proj", "v_proj")]
            if all(k in state_dict for k in keys):
                state_dict[f"{prefix}qkv_proj.{kind}"] = torch.cat([state_dict.pop(k) for k in keys], dim=0)


class HipMLP(nn.Module):
    def __init__(self, dim, inter):
        super().__init__()
        self.fc1 = _Affine((inter, dim))
        self.fc2 = _Affine((dim, inter))


class HipEncoderLayer(nn.Module):
    def __init__(self, dim, inter):
        super().__init__()
        self.self_attn = HipSelfAttention(dim)
        self.layer_norm1 = _Affine((dim,), ones=True)
        self.mlp = HipMLP(dim, inter)
        self.layer_norm2 = _Affine((dim,), ones=True)

    def params(self) -> engine.LayerParams:
        a, m = self.self_attn, self.mlp
        return engine.LayerParams(self.layer_norm1.weight, self.layer_norm1.bias, a.qkv_proj.weight, a.qkv_proj.bias,
                                  a.out_proj.weight, a.out_proj.bias, self.layer_norm2.weight, self.layer_norm2.bias,
                                  m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias)


class HipEncoder(nn.Module):
    def __init__(self, n, dim, inter):
        super().__init__()
        self.layers = nn.ModuleList([HipEncoderLayer(dim, inter) for _ in range(n)])


class _VisionEmbeddings(nn.Module):
    def __init__(self, v: VisionConfig):
        super().__init__()
        self.class_embedding = nn.Parameter(torch.zeros(v.hidden_size))
        self.patch_embedding = nn.Module()
        self.patch_embedding.weight = nn.Parameter(torch.zeros(v.hidden_size, v.num_channels, v.patch_size, v.patch_size))
        self.position_embedding = _Table(v.seq_len, v.hidden_size)


class _TextEmbeddings(nn.Module):
    def __init__(self, t: TextConfig):
        super().__init__()
        self.token_embedding = _Table(t.vocab_size, t.hidden_size)
        self.position_embedding = _Table(t.max_position_embeddings, t.hidden_size)


class HipVisionTransformer(nn.Module):
    def __init__(self, v: VisionConfig):
        super().__init__()
        if v.head_dim != 64:
            raise ValueError("the HIP attention kernel is built for head_dim 64 (every CLIP ViT-B/L config)")
        self.config = v
        self.embeddings = _VisionEmbeddings(v)
        self.pre_layrnorm = _Affine((v.hidden_size,), ones=True)          # sic: HF key spelling
        self.encoder = HipEncoder(v.num_hidden_layers, v.hidden_size, v.intermediate_size)
        self.post_layernorm = _Affine((v.hidden_size,), ones=True)


class HipTextTransformer(nn.Module):
    def __init__(self, t: TextConfig):
        super().__init__()
        if t.head_dim != 64:
            raise ValueError("the HIP attention kernel is built for head_dim 64")
        self.config = t
        self.embeddings = _TextEmbeddings(t)
        self.encoder = HipEncoder(t.num_hidden_layers, t.hidden_size, t.intermediate_size)
        self.final_layer_norm = _Affine((t.hidden_size,), ones=True)


def packed_crop_tables(boxes: torch.Tensor, patch: int) -> dict:
    """Host tables of the packed tower (engine.vision_fwd_packed) for the crops boxes [N,5] = (b, x1, y1, x2, y2), int32 on the
    host: crop n has the grid gh = (y2 - y1) // patch, gw = (x2 - x1) // patch and 1 + gh*gw token rows.  Returns int32 host
    tensors `grids` [N,2], `cu_seqlens` [N+1] (cumulative token rows), `patch_offsets` [N+1] (= cu_seqlens[n] - n), `cls_rows`
    [N] (= cu_seqlens[:-1]) and the int `max_S`.  A crop with a side shorter than one patch is a ValueError."""
    boxes = torch.as_tensor(boxes, dtype=torch.int32).reshape(-1, 5).cpu()
    if patch < 1:
        raise ValueError(f"patch {patch}")
    gh = torch.div(boxes[:, 4] - boxes[:, 2], patch, rounding_mode="floor")
    gw = torch.div(boxes[:, 3] - boxes[:, 1], patch, rounding_mode="floor")
    if boxes.shape[0] and int(torch.minimum(gh, gw).min()) < 1:
        n = int((torch.minimum(gh, gw) < 1).nonzero()[0])
        raise ValueError(f"the crop of box {tuple(boxes[n, 1:].tolist())} is smaller than one patch ({patch}*{patch})")
    seq = (1 + gh.long() * gw.long())
    if int(seq.sum()) >= 2 ** 31:
        raise ValueError("packed crops: more than 2^31 token rows")
    cu = torch.zeros(boxes.shape[0] + 1, dtype=torch.int32)
    cu[1:] = torch.cumsum(seq, 0).to(torch.int32)
    po = cu - torch.arange(boxes.shape[0] + 1, dtype=torch.int32)
    return {"grids": torch.stack([gh, gw], 1).to(torch.int32).contiguous(), "cu_seqlens": cu, "patch_offsets": po,
            "cls_rows": cu[:-1].clone(), "max_S": int(seq.max()) if boxes.shape[0] else 0}


def packed_text_tables(input_ids_host: torch.Tensor, eos_id: int, lens=None) -> dict:
    """Host tables of the packed text tower (engine.text_fwd_frozen_packed) for the captions input_ids_host
    [N,T]: caption n keeps its rows 0 .. first EOS, len_n = first EOS index + 1, or 1 for a row without EOS (ops.first_eos
    gives 0 for it).  `lens` (a host int sequence or a CPU tensor [N]) hands the lengths over instead: every one must lie in
    [1, T], and the ids are then used for their shape only (they may live anywhere).  Without `lens` the ids must be on the
    host: nothing is read back from a device.  Returns int32 contiguous CPU tensors `lens` [N], `cu_seqlens` [N+1] (cumulative
    lengths) and `last_rows` [N] (= cu_seqlens[1:] - 1, the packed rows of the first EOS), and the ints `max_S`, `Tp`
    (= cu_seqlens[N]) and `max_tokens` (= max(max(lens) - 2, 1): the word-token padding of ops.pack_tokens_varlen)."""
    if input_ids_host.dim() != 2 or input_ids_host.shape[0] < 1 or input_ids_host.shape[1] < 1:
        raise ValueError(f"packed_text_tables: input_ids {tuple(input_ids_host.shape)}, expected [N, T]")
    N, T = input_ids_host.shape
    if lens is None:
        if input_ids_host.device.type != "cpu":
            raise ValueError("packed_text_tables: the caption lengths come from token ids on the HOST (or pass lens); ids on "
                             f"{input_ids_host.device} are never read back")
        hit = input_ids_host == int(eos_id)
        first = hit.int().argmax(dim=1)                        # 0 for a row without EOS, as ops.first_eos
        lens_t = (first + 1).to(torch.int32)
    else:
        if isinstance(lens, torch.Tensor):
            if lens.device.type != "cpu":
                raise ValueError(f"packed_text_tables: lens must be on the host, got {lens.device}")
            if lens.dtype.is_floating_point or lens.dtype == torch.bool:
                raise ValueError(f"packed_text_tables: lens must be integers, got {lens.dtype}")
            lens_t = lens.reshape(-1).to(torch.int64)
        else:
            lens_t = torch.tensor([int(v) for v in lens], dtype=torch.int64)
        if lens_t.numel() != N:
            raise ValueError(f"packed_text_tables: {lens_t.numel()} lengths for {N} captions")
        if int(lens_t.min()) < 1 or int(lens_t.max()) > T:
            bad = int(((lens_t < 1) | (lens_t > T)).nonzero()[0])
            raise ValueError(f"packed_text_tables: caption {bad} has length {int(lens_t[bad])}, outside [1, {T}]")
        lens_t = lens_t.to(torch.int32)
    lens_t = lens_t.contiguous()
    total = int(lens_t.long().sum())
    if total >= 2 ** 31:
        raise ValueError("packed captions: more than 2^31 token rows")
    cu = torch.zeros(N + 1, dtype=torch.int32)
    cu[1:] = torch.cumsum(lens_t.long(), 0).to(torch.int32)
    max_S = int(lens_t.max())
    return {"lens": lens_t, "cu_seqlens": cu, "last_rows": (cu[1:] - 1).contiguous(), "max_S": max_S, "Tp": total,
            "max_tokens": max(max_S - 2, 1)}


def text_train_split16_route(flag: bool, text_trainable: bool, capturing: bool, widths_ok: bool) -> bool:
    """Whether a gradient-enabled text forward takes the trainable tower's split-fp16 plan: the switch is on, a
    text parameter trains (gradients are needed), no stream is capturing and the widths are multiples of 8 (the plan's
    condition).  Everything else is the plain fp32 path, the tower as it runs without the switch."""
    return bool(flag and text_trainable and not capturing and widths_ok)


class HipCLIPModel(nn.Module):
    # The 16-bit MFMA attention core of the packed frozen towers for get_image_features_crops,
    # get_text_features(packed_lens=...) and text_token_level_packed at precision "bf16" / "fp16": True / False, or None for the
    # process-wide DCLIP_PACKED_ATTN16 (off unless set).
    packed_attention16: Optional[bool] = None
    # The TRAINABLE fp32 text tower — get_text_features with grad enabled and a trainable text parameter, padded or with
    # `packed_train` — with its layers' full-size GEMMs (forward, data and weight gradients) on the fp16 MFMAs from hi/lo split
    # operands.  Off: the plain fp32 GEMMs, launch for launch what the tower ran before the switch existed.
    text_train_split16: bool = False

    def __init__(self, config: Optional[ClipConfig] = None):
        super().__init__()
        self.config = config or ClipConfig()
        c = self.config
        self.logit_scale = nn.Parameter(torch.tensor(c.logit_scale_init_value))
        self.text_model = HipTextTransformer(c.text)
        self.vision_model = HipVisionTransformer(c.vision)
        self.visual_projection = _Affine((c.projection_dim, c.vision.hidden_size), bias=False)
        self.text_projection = _Affine((c.projection_dim, c.text.hidden_size), bias=False)

    # convenient aliases used by tests / smoke
    @property
    def visual_projection_weight(self):
        return self.visual_projection.weight

    def vision_params(self) -> engine.VisionParams:
        vm = self.vision_model
        e = vm.embeddings
        return engine.VisionParams(e.class_embedding, e.patch_embedding.weight, e.position_embedding.weight,
                                   vm.pre_layrnorm.weight, vm.pre_layrnorm.bias,
                                   [l.params() for l in vm.encoder.layers],
                                   vm.post_layernorm.weight, vm.post_layernorm.bias, self.visual_projection.weight)

    def text_params(self) -> engine.TextParams:
        tm = self.text_model
        return engine.TextParams(tm.embeddings.token_embedding.weight, tm.embeddings.position_embedding.weight,
                                 [l.params() for l in tm.encoder.layers],
                                 tm.final_layer_norm.weight, tm.final_layer_norm.bias, self.text_projection.weight)

    # ------------------------------------------------------------------ reference call surface
    def _vision_grid(self, pixel_values: torch.Tensor, interpolate_pos_encoding: bool):
        """None for an image of the model's own size; with `interpolate_pos_encoding` the (gh, gw) patch grid of any other
        H x W (hf CLIPVisionEmbeddings.forward: the size check applies only without the flag, and an image of the model's
        size takes the plain table either way)."""
        v = self.config.vision
        Hh, Ww = pixel_values.shape[-2], pixel_values.shape[-1]
        if Hh == v.image_size and Ww == v.image_size:
            return None
        if not interpolate_pos_encoding:
            raise ValueError(f"Input image size ({Hh}*{Ww}) doesn't match "
                             f"model ({v.image_size}*{v.image_size}).")          # hf:modeling_clip.py:204-207
        if pixel_values.dim() != 4 or Hh < v.patch_size or Ww < v.patch_size:
            raise ValueError(f"Input image size ({Hh}*{Ww}) is smaller than one patch ({v.patch_size}*{v.patch_size}).")
        return (Hh // v.patch_size, Ww // v.patch_size)

    def get_image_features(self, pixel_values: torch.Tensor = None, precision: str = "fp32",
                           interpolate_pos_encoding: bool = False, **kwargs) -> torch.Tensor:
        """precision="bf16" (opt-in): GEMM inputs in bf16 on the bf16 MFMA path, everything else fp32 — frozen forward, or
        the bf16 training path when grad is enabled and a parameter is trainable.  precision="fp16" (opt-in, frozen use
        only): the same forward with fp16 GEMM inputs (3 more mantissa bits at the bf16 rate).  precision="fp16-mixed"
        (opt-in): the fp16 TRAINING path (Lightning's "16-mixed": fp16 GEMM inputs with IEEE rounding, fp32 master weights;
        the caller scales the loss, amp.DynamicLossScaler) when grad is enabled and a parameter is trainable, otherwise the
        frozen "fp16" forward.  interpolate_pos_encoding=True (as on HF's CLIPModel): any H x W of at least one patch a side;
        the position table is resampled bicubically to the image's patch grid, rows and columns beyond the
        last whole patch are ignored.  Without the flag nothing changes, the size check included.
        precision="fp32-split16" (opt-in, frozen use only): the fp32 forward with the encoder layers' full-size
        GEMMs on the fp16 MFMAs from hi/lo split operands — fp32-grade features (the error of "fp32" itself against fp64, not
        that of "fp16") at 16-bit-pipe speed; with grad enabled and a trainable vision parameter it is a RuntimeError (training
        has its own split path under "fp32").  `packed_attention16` has no effect at this precision."""
        if pixel_values is None:
            raise ValueError("You have to specify pixel_values")
        v = self.config.vision
        grid = self._vision_grid(pixel_values, interpolate_pos_encoding)
        p = self.vision_params()
        if precision == "bf16":
            if torch.is_grad_enabled() and any(t.requires_grad for t in p.tensors()):
                # TRAINING in bf16 (configs c3 / c5): forward, dgrad and wgrad GEMMs on the bf16 MFMA kernels, fp32
                # master weights and fp32 everything else (engine.vision_fwd_bf16_train)
                engine.refuse_train16(v)                 # hidden_act="gelu": NotImplementedError, nothing launched
                return functional.VisionTowerBf16Fn.apply(pixel_values.float(), v, v.num_hidden_layers, self._bf16_cache(),
                                                          torch.bfloat16, grid, *p.tensors())
            pd = engine.VisionParams.from_tensors([t.detach() for t in p.tensors()], v.num_hidden_layers)
            return engine.vision_fwd_bf16(pd, pixel_values.float().contiguous(), v, self._bf16_cache(), grid=grid)
        if precision in ("fp16", "fp16-mixed"):
            if torch.is_grad_enabled() and any(t.requires_grad for t in p.tensors()):
                if precision == "fp16":
                    raise RuntimeError("precision='fp16' is a forward-only path for frozen towers: call it under torch.no_grad()"
                                       " (training: precision='fp16-mixed')")
                engine.refuse_train16(v)
                return functional.VisionTowerBf16Fn.apply(pixel_values.float(), v, v.num_hidden_layers, self._f16_cache(),
                                                          torch.float16, grid, *p.tensors())
            pd = engine.VisionParams.from_tensors([t.detach() for t in p.tensors()], v.num_hidden_layers)
            return engine.vision_fwd_bf16(pd, pixel_values.float().contiguous(), v, self._f16_cache(), torch.float16,
                                          grid=grid)
        if precision == "fp32-split16":
            if torch.is_grad_enabled() and any(t.requires_grad for t in p.tensors()):
                raise RuntimeError("precision='fp32-split16' is a forward-only path for frozen towers: call it under "
                                   "torch.no_grad() (training: precision='fp32' takes its own split path)")
            pd = engine.VisionParams.from_tensors([t.detach() for t in p.tensors()], v.num_hidden_layers)
            return engine.vision_fwd_frozen_split16(pd, pixel_values.float().contiguous(), v, self._vsplit16_frozen_cache(),
                                                    grid=grid)
        if precision != "fp32":
            raise ValueError(f"precision {precision!r}")
        # the split-fp16 forward (engine.vision_fwd, DCLIP_VISION_SPLIT16) is the TRAINING forward only: a no-grad call
        # (evaluation, a teacher beside the student on another stream) never touches the split copies
        train = torch.is_grad_enabled() and any(t.requires_grad for t in p.tensors())
        return functional.VisionTowerFn.apply(pixel_values.float(), v, v.num_hidden_layers, grid,
                                              self._vsplit16_cache() if train else None, *p.tensors())

    @torch.no_grad()
    def get_image_features_crops(self, images_u8: torch.Tensor, dims: torch.Tensor, boxes, precision: str = "fp32") -> torch.Tensor:
        """Image features [N, P] of N crops of a padded uint8 batch, every crop at its OWN size, in one packed pass of the
        frozen tower.  FORWARD ONLY: it runs under no_grad whatever the caller's mode and nothing is saved.
        images_u8 [B,Hmax,Wmax,3] uint8 and dims [B,2] int32 (h, w) on the device (data.GpuCollate); boxes [N,5] =
        (b, x1, y1, x2, y2) integers on the HOST (a tensor or a list).  Crop n is what PIL's crop((x1,y1,x2,y2)) + ToTensor()
        give (values in [0,1], zero outside the image, no mean / std), cut on the device; its position table is the model's,
        resampled to its patch grid as get_image_features(interpolate_pos_encoding=True) does.  A crop with a side shorter than
        one patch is a ValueError.  precision: "fp32", "bf16" or "fp16" (16-bit GEMM inputs; fp32 attention core, or the 16-bit
        packed core with `packed_attention16`), or "fp32-split16" (the fp32 pass with its full-size GEMMs on split-fp16 operands,
        get_image_features; `packed_attention16` has no effect there)."""
        if precision not in ("fp32", "bf16", "fp16", "fp32-split16"):
            raise ValueError(f"precision {precision!r}")
        v = self.config.vision
        flat = torch.as_tensor(boxes, dtype=torch.int32).reshape(-1, 5).cpu().contiguous()
        N = flat.shape[0]
        if N == 0:
            return torch.zeros((0, self.config.projection_dim), dtype=torch.float32, device=images_u8.device)
        if int(flat[:, 0].min()) < 0 or int(flat[:, 0].max()) >= images_u8.shape[0]:
            raise ValueError(f"get_image_features_crops: a box names an image outside the batch of {images_u8.shape[0]}")
        t = packed_crop_tables(flat, v.patch_size)
        # one upload for the four tables
        host = torch.cat([flat.reshape(-1), t["grids"].reshape(-1), t["cu_seqlens"], t["patch_offsets"]])
        dev_t = host.to(images_u8.device, non_blocking=False)
        bx, grids = dev_t[:5 * N].view(N, 5), dev_t[5 * N:7 * N].view(N, 2)
        cu, po = dev_t[7 * N:8 * N + 1], dev_t[8 * N + 1:]
        cols = ops.patches_from_boxes_u8(images_u8, dims, bx, po, int(t["patch_offsets"][-1]), v.patch_size)
        pd = engine.VisionParams.from_tensors([x.detach() for x in self.vision_params().tensors()], v.num_hidden_layers)
        cache = {"fp32": lambda: None, "bf16": self._bf16_cache, "fp16": self._f16_cache,
                 "fp32-split16": self._vsplit16_frozen_cache}[precision]()
        return engine.vision_fwd_packed(pd, cols, grids, cu, cu[:N], t["max_S"], v, precision, cache, self.packed_attention16)

    def _bf16_cache(self) -> dict:
        """bf16 copies of the GEMM weights: persistent buffers, each refreshed in place when ITS parameter's version
        counter has moved (optimizer step, load_state_dict) — engine._w16 / _w16t.  A frozen tower's copies are made once."""
        c = getattr(self, "_bf16_w", None)
        if c is None:
            c = {}
            object.__setattr__(self, "_bf16_w", c)
        return c

    def _f16_cache(self) -> dict:
        """fp16 copies of the GEMM weights (precision="fp16"), kept apart from the bf16 ones: the keys are the same."""
        c = getattr(self, "_f16_w", None)
        if c is None:
            c = {}
            object.__setattr__(self, "_f16_w", c)
        return c

    def _split16_cache(self) -> dict:
        """Split-fp16 copies [hi|hi|lo] of the frozen text tower's GEMM weights and the activation scales that go with them
        (engine.text_fwd_frozen_split16): built at the first frozen fp32 text forward, refreshed when a weight changes."""
        c = getattr(self, "_split16_w", None)
        if c is None:
            c = {}
            object.__setattr__(self, "_split16_w", c)
        return c

    def _vsplit16_cache(self) -> dict:
        """The vision tower's device-side split-fp16 plan (engine._vision_split16_plan): record table, plan record and the
        [hi|hi|lo] weight copies, built at the first gradient-enabled fp32 image forward and refreshed on the device whenever
        a weight has changed.  Per model, so a teacher snapshot never shares the student's copies."""
        c = getattr(self, "_vsplit16_w", None)
        if c is None:
            c = {}
            object.__setattr__(self, "_vsplit16_w", c)
        return c

    def _tsplit16_train_cache(self) -> dict:
        """The TRAINABLE text tower's device-side split-fp16 plan (`text_train_split16`): its own cache — apart
        from the frozen host plan of _split16_cache and from the vision tower's _vsplit16_cache, so a refresh of one tower never
        invalidates the other's pending backward."""
        c = getattr(self, "_tsplit16_train_w", None)
        if c is None:
            c = {}
            object.__setattr__(self, "_tsplit16_train_w", c)
        return c

    def _text_train_split16_cache(self, p) -> Optional[dict]:
        """_tsplit16_train_cache() where text_train_split16_route takes the plan for this call, else None (logged once)."""
        t = self.config.text
        flag = bool(self.text_train_split16)
        trainable = torch.is_grad_enabled() and any(x.requires_grad for x in p.tensors())
        capturing = p.tok.is_cuda and torch.cuda.is_current_stream_capturing()
        widths_ok = t.hidden_size % 8 == 0 and t.intermediate_size % 8 == 0 and t.num_hidden_layers > 0
        if text_train_split16_route(flag, trainable, capturing, widths_ok):
            return self._tsplit16_train_cache()
        if flag and trainable:
            engine._split16_log_once("split-fp16 trainable text tower: " + ("a stream is capturing" if capturing else
                                     "the widths are not multiples of 8") + "; the tower takes the plain fp32 path")
        return None

    def _vsplit16_frozen_cache(self) -> dict:
        """The FROZEN vision tower's host split-fp16 plan (precision "fp32-split16", engine.vision_fwd_frozen_split16): the
        [hi|hi|lo] weight copies and host-float scales, built at the first such forward (one device-to-host read) and rebuilt when
        a weight changes.  Never the training plan of _vsplit16_cache: that one's buffers are rewritten on the training stream."""
        c = getattr(self, "_vsplit16_frozen_w", None)
        if c is None:
            c = {}
            object.__setattr__(self, "_vsplit16_frozen_w", c)
        return c

    def invalidate_bf16_of_trainable(self) -> int:
        """Mark the bf16 (and fp16) copies of every TRAINABLE parameter stale (frozen towers keep theirs).  graph.GraphedStep calls
        this between its eager warm-up and the capture: the weight casts / transposes are then part of the captured step
        and every replay converts the CURRENT fp32 masters — without it a replay would multiply by the copies made
        at warm-up while the optimizer keeps updating the masters.  Returns the number of entries marked."""
        caches = [c for c in (getattr(self, "_bf16_w", None), getattr(self, "_f16_w", None)) if c]
        if not caches:
            return 0
        ptrs = {p.data_ptr() for p in self.parameters() if p.requires_grad}
        n = 0
        for c in caches:
            for e in c.values():
                if isinstance(e, list) and e[2] in ptrs:
                    e[1] = -1
                    n += 1
        return n

    def get_text_features(self, input_ids: torch.Tensor = None, attention_mask=None, precision: str = "fp32",
                          packed_lens=None, packed_train: bool = False, **kwargs) -> torch.Tensor:
        """`attention_mask` is accepted and ignored: under the causal mask trailing pads cannot influence the
        first-EOS row that is pooled.  precision="bf16" / "fp16": frozen forward only (see
        get_image_features).  `packed_lens` (opt-in, frozen use only): the captions' lengths on the HOST
        (first EOS index + 1; an int sequence or a CPU tensor [B]), or True when `input_ids` is a CPU tensor (the lengths
        are then derived from it).  The tower then runs on the captions cut after their first EOS and laid back to back
        — the rows behind a first EOS are read by no result — under no_grad semantics.  Lengths are never read back from
        the device: True with ids that are not on the host is a ValueError.  While a stream is capturing the padded path
        runs (a captured graph's shapes must not follow the batch).
        `packed_train` (opt-in, with `packed_lens`): with grad enabled, a trainable text parameter and
        precision "fp32", the TRAINABLE tower runs on the packed captions, forward and backward (engine.text_fwd_packed) —
        the padded tower's gradients from Tp rows instead of B T.  Without it that call is refused as before; under no_grad it
        changes nothing; a 16-bit precision keeps the forward-only error; while a stream is capturing the padded trainable
        path runs.
        `text_train_split16` (the model's attribute): the trainable fp32 tower, padded or packed, on the
        split-fp16 plan; under no_grad, with a frozen tower or while a stream is capturing it changes nothing."""
        if input_ids is None:
            raise ValueError("You have to specify input_ids")
        t = self.config.text
        if input_ids.shape[-1] > t.max_position_embeddings:
            raise ValueError(f"Sequence length must be less than max_position_embeddings (got `sequence length`: "
                             f"{input_ids.shape[-1]} and max_position_embeddings: {t.max_position_embeddings}")
        packed = packed_lens is not None and packed_lens is not False
        if packed and packed_lens is True and input_ids.device.type != "cpu":
            raise ValueError(f"packed_lens=True needs input_ids on the host (got {input_ids.device}): caption lengths are never "
                             "read back from the device; pass the lengths")
        if precision not in ("fp32", "bf16", "fp16"):
            raise ValueError(f"precision {precision!r}")
        p = self.text_params()
        if packed:
            train = torch.is_grad_enabled() and any(x.requires_grad for x in p.tensors())
            if train and not (packed_train and precision == "fp32"):
                raise RuntimeError("packed_lens is a forward-only path for frozen towers: call it under torch.no_grad()")
            dev = p.tok.device
            if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
                packed = False
            elif train:
                tables = self._packed_text_tables(input_ids, None if packed_lens is True else packed_lens, dev)
                return functional.TextTowerPackedFn.apply(input_ids.to(dev).long().contiguous(), t, t.num_hidden_layers, tables,
                                                          self._text_train_split16_cache(p), *p.tensors())
            else:
                with torch.no_grad():
                    tables = self._packed_text_tables(input_ids, None if packed_lens is True else packed_lens, dev)
                    cache = {"fp32": self._split16_cache, "bf16": self._bf16_cache, "fp16": self._f16_cache}[precision]()
                    return engine.text_fwd_frozen_packed(self.text_params_detached(), input_ids.to(dev).long().contiguous(),
                                                         tables, t, precision, cache, self.packed_attention16)
            input_ids = input_ids.to(dev)
        if precision == "bf16":
            if torch.is_grad_enabled() and any(x.requires_grad for x in p.tensors()):
                raise RuntimeError("precision='bf16' is a forward-only path for frozen towers: call it under torch.no_grad()")
            return engine.text_fwd_frozen_bf16(self.text_params_detached(), input_ids.long().contiguous(), t,
                                               self._bf16_cache())
        if precision == "fp16":
            if torch.is_grad_enabled() and any(x.requires_grad for x in p.tensors()):
                raise RuntimeError("precision='fp16' is a forward-only path for frozen towers: call it under torch.no_grad()")
            return engine.text_fwd_frozen_bf16(self.text_params_detached(), input_ids.long().contiguous(), t,
                                               self._f16_cache(), torch.float16)
        return functional.TextTowerFn.apply(input_ids.long(), t, t.num_hidden_layers, self._split16_cache(),
                                            self._text_train_split16_cache(p), *p.tensors())

    def _packed_text_tables(self, input_ids: torch.Tensor, lens, dev) -> dict:
        """packed_text_tables plus `cu_seqlens_dev` / `last_rows_dev`: ONE upload of a buffer allocated for this call (a
        staging buffer shared between calls could be rewritten while a teacher that runs a step ahead still reads it)."""
        tables = packed_text_tables(input_ids, self.config.text.eos_token_id, lens)
        N = input_ids.shape[0]
        both = torch.cat([tables["cu_seqlens"], tables["last_rows"]]).to(dev, non_blocking=False)
        tables["cu_seqlens_dev"], tables["last_rows_dev"] = both[:N + 1], both[N + 1:]
        return tables

    @torch.no_grad()
    def text_token_level_packed(self, input_ids: torch.Tensor, lens=None, precision: str = "fp32"):
        """text_token_level on packed captions: (sentence [B,P], tokens_packed [Tp,P], cu_seqlens on the device
        [B+1], tables).  Caption b's rows are tokens_packed[cu[b] : cu[b+1]] (BOS .. first EOS); `lens` as get_text_features'
        `packed_lens` (None: derived from `input_ids` on the host).  tables: packed_text_tables' result (max_tokens, ...).
        precision: as text_token_level; `packed_attention16` has no effect at "fp32" and "fp32-split16"."""
        if precision not in ("fp32", "bf16", "fp16", "fp32-split16"):
            raise ValueError(f"precision {precision!r}")
        t = self.config.text
        if input_ids.shape[-1] > t.max_position_embeddings:
            raise ValueError(f"Sequence length must be less than max_position_embeddings (got {input_ids.shape[-1]})")
        dev = self.text_projection.weight.device
        tables = self._packed_text_tables(input_ids, lens, dev)
        cache = {"fp32": lambda: None, "bf16": self._bf16_cache, "fp16": self._f16_cache,
                 "fp32-split16": self._split16_cache}[precision]()
        sent, tokens = engine.text_token_level_packed(self.text_params_detached(), input_ids.to(dev).long().contiguous(), tables,
                                                      t, precision, cache, self.packed_attention16)
        return sent, tokens, tables["cu_seqlens_dev"], tables

    @torch.no_grad()
    def text_token_level(self, input_ids: torch.Tensor, precision: str = "fp32"):
        """Frozen pass used by the meta-teacher: (sentence [B,P], tokens [B,T,P], first-EOS index [B]).  precision "bf16" / "fp16":
        16-bit GEMM inputs; "fp32-split16": the fp32 pass with every layer's GEMMs on split-fp16 operands (the text tower's
        _split16_cache plan); "fp32": the plain fp32 GEMMs."""
        t = self.config.text
        ids = input_ids.long().contiguous()
        if precision == "bf16":
            sent, tokens, eos = engine.text_token_level_bf16(self.text_params_detached(), ids, t, self._bf16_cache())
        elif precision == "fp16":
            sent, tokens, eos = engine.text_token_level_bf16(self.text_params_detached(), ids, t, self._f16_cache(),
                                                             torch.float16)
        elif precision == "fp32":
            sent, tokens, eos = engine.text_token_level(self.text_params_detached(), ids, t)
        elif precision == "fp32-split16":      # every layer's GEMMs on the text tower's split-fp16 plan
            sent, tokens, eos = engine.text_token_level_split16(self.text_params_detached(), ids, t, self._split16_cache())
        else:
            raise ValueError(f"precision {precision!r}")
        return sent, tokens.view(input_ids.shape[0], input_ids.shape[1], -1), eos

    def text_params_detached(self) -> engine.TextParams:
        p = self.text_params()
        return engine.TextParams.from_tensors([t.detach() for t in p.tensors()], len(p.layers))

    @torch.no_grad()
    def hidden_states(self, pixel_values=None, input_ids=None, interpolate_pos_encoding: bool = False) -> List[torch.Tensor]:
        """Per-layer hidden states (parity tests): [embeddings-after-pre-LN, layer 1, ...] for vision,
        [embeddings, layer 1, ...] (before final_layer_norm) for text.  `interpolate_pos_encoding`: as in get_image_features."""
        out: List[torch.Tensor] = []
        if pixel_values is not None:
            v = self.config.vision
            grid = self._vision_grid(pixel_values, interpolate_pos_encoding) if interpolate_pos_encoding else None
            p = engine.VisionParams.from_tensors([t.detach() for t in self.vision_params().tensors()],
                                                 v.num_hidden_layers)
            engine.vision_fwd(p, pixel_values.float().contiguous(), v, False, out, grid=grid)
            return [h.view(pixel_values.shape[0], -1, h.shape[-1]) for h in out]
        t = self.config.text
        engine.text_encoder_fwd(self.text_params_detached(), input_ids.long().contiguous(), t, False, out)
        return [h.view(input_ids.shape[0], input_ids.shape[1], -1) for h in out]


def from_hf_state_dict(config: ClipConfig, state_dict, device=None) -> HipCLIPModel:
    """Build a model from an HF-keyed state dict (e.g. `CLIPModel.from_pretrained(local_dir).state_dict()`)."""
    m = HipCLIPModel(config)
    missing, unexpected = m.load_state_dict(state_dict, strict=False)
    unexpected = [k for k in unexpected if "position_ids" not in k]       # 4.x checkpoints carry these buffers
    if missing or unexpected:
        raise KeyError(f"state dict mismatch: missing={missing[:5]} unexpected={unexpected[:5]}")
    return m.to(device) if device is not None else m
