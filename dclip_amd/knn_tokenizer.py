"""The teacher's KNN / projection region tokenizer: `ImageProjectionModule`, `ImageTokenizer` and `TokenizerWithKNN`
with the reference's names (training/image_projection_module.py, training/image_tokenizer.py:166-431), on the HIP kernels.

A crop's CLIP embedding is replaced by its nearest codebook entry when that entry's inner product with the L2-normalised
embedding is at or above `similarity_threshold` (:278), and otherwise by the L2-normalised output of a small frozen MLP
over (normalised embedding, box position) (:285-311).  The reference does this one crop at a time on the host with a
FAISS `IndexFlatIP`; here a whole batch of crops goes through one exact top-1 inner-product search (ops.topk_ip), three
GEMMs and one select kernel, with no host synchronisation.

Deliberate differences from the reference:
  * the codebook is read from `embeddings_json_path` alone.  training/compute_faiss.py adds every embedding to the index
    and to the dict in the same order, so the JSON in file order IS the index; `faiss_index_path` only has to exist, as
    the reference checks (:227).  The `.idx` file is NOT parsed: FAISS is not a dependency of this package, and a parser
    of its format could not be validated against it.
  * the dict value layout `{"embedding": ..., "position": ...}` that compute_faiss.py writes is understood (the reference
    builds `np.array(dict)` from it, :280), and an empty codebook disables KNN instead of reading an unbound variable (:278).
  * no per-crop prints.
"""
from __future__ import annotations

import json
import os
from typing import Optional

import torch
import torch.nn as nn

from . import ops
from .clip_model import _Affine


class _Slot(nn.Module):
    """A parameterless place holder: keeps the reference's `nn.Sequential` numbering (the ReLUs are entries 1 and 3)."""


class ImageProjectionModule(nn.Module):
    """training/image_projection_module.py: Linear(clip_dim + 4, hidden) - ReLU - Linear(hidden, hidden) - ReLU -
    Linear(hidden, clip_dim); `state_dict()` keys `projection.{0,2,4}.{weight,bias}`.  Frozen: forward only."""

    def __init__(self, clip_dim: int = 512, hidden_dim: int = 1024):
        super().__init__()
        self.clip_dim, self.hidden_dim = clip_dim, hidden_dim
        self.projection = nn.ModuleList([_Affine((hidden_dim, clip_dim + 4)), _Slot(), _Affine((hidden_dim, hidden_dim)), _Slot(),
                                         _Affine((clip_dim, hidden_dim))])
        for i in (0, 2, 4):        # nn.Linear's default initialisation
            lin = self.projection[i]
            nn.init.kaiming_uniform_(lin.weight, a=5 ** 0.5)
            bound = 1.0 / lin.weight.shape[1] ** 0.5
            nn.init.uniform_(lin.bias, -bound, bound)
        for p in self.parameters():
            p.requires_grad_(False)

    @torch.no_grad()
    def forward(self, context_features: torch.Tensor, positions: torch.Tensor) -> torch.Tensor:
        x = torch.cat([context_features.float(), positions.float()], dim=1).contiguous()
        l0, l2, l4 = self.projection[0], self.projection[2], self.projection[4]
        h = ops.relu_(ops.gemm(x, l0.weight, ops.LAYOUT_NT, bias=l0.bias))
        h = ops.relu_(ops.gemm(h, l2.weight, ops.LAYOUT_NT, bias=l2.bias))
        return ops.gemm(h, l4.weight, ops.LAYOUT_NT, bias=l4.bias)

    @classmethod
    def from_checkpoint(cls, path: str, map_location="cpu"):
        """A plain state dict, or a training checkpoint holding `model_state_dict` (training/image_tokenizer.py:195-208).
        The widths are read off `projection.0.weight` [hidden, clip_dim + 4] (the reference fixes them at 512 / 1024)."""
        ckpt = torch.load(path, map_location=map_location, weights_only=True)
        if isinstance(ckpt, dict) and "model_state_dict" in ckpt:
            ckpt = ckpt["model_state_dict"]
        hidden_dim, width = ckpt["projection.0.weight"].shape
        module = cls(width - 4, hidden_dim)
        module.load_state_dict(ckpt)
        return module.eval()


def load_codebook(embeddings_json_path: str):
    """(patch_ids in file order, embeddings [N,E] fp32 on the host).  A value is a bare list or
    {"embedding": list, "position": ...}; a list nested as [1,E] is flattened."""
    with open(embeddings_json_path, "r") as f:
        entries = json.load(f)          # a dict: json keeps the file's key order
    ids, rows = [], []
    for key, value in entries.items():
        if isinstance(value, dict):
            value = value["embedding"]
        row = torch.tensor(value, dtype=torch.float32).flatten()
        if rows and row.numel() != rows[0].numel():
            raise ValueError(f"{embeddings_json_path}: entry {key!r} has {row.numel()} values, the first entry {rows[0].numel()}")
        ids.append(key)
        rows.append(row)
    return ids, (torch.stack(rows) if rows else torch.zeros((0, 0)))


class ImageTokenizer:
    """training/image_tokenizer.py:166-326 for a batch of crops.  `clip_model` is the HipCLIPModel whose image tower
    embeds the crops (the reference loads one by name); the codebook lives on its device as one [N,E] fp32 tensor."""

    def __init__(self, clip_model, projection_model_path=None, faiss_index_path=None, embeddings_json_path=None,
                 similarity_threshold: float = 0.85, device=None):
        self.clip_model = clip_model
        self.device = torch.device(device) if device is not None else next(clip_model.parameters()).device
        self.similarity_threshold = float(similarity_threshold)
        dim = clip_model.config.projection_dim
        self.projection_module = None
        if projection_model_path and os.path.exists(projection_model_path):
            self.projection_module = ImageProjectionModule.from_checkpoint(projection_model_path).to(self.device)
            if self.projection_module.clip_dim != dim:
                raise ValueError(f"{projection_model_path}: a projection of width {self.projection_module.clip_dim}, the CLIP "
                                 f"model projects to {dim}")
        self.use_knn = False
        self.patch_ids = None
        self.codebook = None
        if faiss_index_path and embeddings_json_path and os.path.exists(faiss_index_path) \
                and os.path.exists(embeddings_json_path):
            ids, rows = load_codebook(embeddings_json_path)
            if ids:
                if rows.shape[1] != dim:
                    raise ValueError(f"{embeddings_json_path}: embeddings of width {rows.shape[1]}, the CLIP model projects to {dim}")
                self.patch_ids = ids
                self.codebook = rows.to(self.device).contiguous()
                self.use_knn = True

    def _apply(self, fn):
        """Move with the teacher that owns this tokenizer (`fn` is what nn.Module._apply hands its parameters)."""
        if self.codebook is not None:
            self.codebook = fn(self.codebook).float().contiguous()
            self.device = self.codebook.device
        if self.projection_module is not None:
            self.projection_module._apply(fn)
            self.device = self.projection_module.projection[0].weight.device
        return self

    @torch.no_grad()
    def knn_or_projection(self, embeddings: torch.Tensor, positions: Optional[torch.Tensor] = None):
        """embeddings [Q,E] (raw CLIP image features), positions [Q,4] = (x1/w, y1/h, x2/w, y2/h) or None (zeros, :298)
        -> (out [Q,E], source [Q] int32: 0 = codebook entry, 1 = fallback, similarity [Q]: the best inner product, -inf
        without a codebook).  The fallback is the L2-normalised projection, or the normalised embedding itself when there
        is no projection module (the reference's "clip" branch, :315)."""
        x, _ = ops.normalize_rows_fwd(embeddings.detach().float().contiguous())
        Q = x.shape[0]
        if self.projection_module is not None:
            if positions is None:
                positions = torch.zeros((Q, 4), dtype=torch.float32, device=x.device)
            positions = positions.to(x.device).float().reshape(Q, 4)
            fallback, _ = ops.normalize_rows_fwd(self.projection_module(x, positions))
        else:
            fallback = x
        if not self.use_knn:
            return fallback, torch.ones((Q,), dtype=torch.int32, device=x.device), \
                torch.full((Q,), float("-inf"), dtype=torch.float32, device=x.device)
        sim, idx = ops.topk_ip(x, self.codebook, 1)
        sim, idx = sim.view(Q), idx.view(Q)
        out, source = ops.knn_select(sim, idx, self.codebook, fallback, self.similarity_threshold)
        return out, source, sim


class TokenizerWithKNN:
    """The reference's holder (training/image_tokenizer.py:331-431) without the detector: `knn_tokenizer` and its
    `knn_or_projection`, batched."""

    def __init__(self, clip_model, projection_model_path=None, faiss_index_path=None, embeddings_json_path=None,
                 similarity_threshold: float = 0.85, device=None):
        self.patch_tokenizer = None
        self.knn_tokenizer = ImageTokenizer(clip_model, projection_model_path, faiss_index_path, embeddings_json_path,
                                            similarity_threshold, device)
        self.device = self.knn_tokenizer.device

    def knn_or_projection(self, embeddings: torch.Tensor, positions: Optional[torch.Tensor] = None):
        return self.knn_tokenizer.knn_or_projection(embeddings, positions)
