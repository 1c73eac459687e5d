#!/usr/bin/env python
"""Write tests/golden/vision_interp.npz and tests/golden/vision_interp_HxW.npz: the tiny vision tower run by HF transformers'
CLIPModel (eager attention, float32, CPU) with interpolate_pos_encoding=True at image sizes other than the model's, forward
and backward.

    python tools/make_vision_interp_golden.py

Third-party code only (torch, transformers); the weights are synth.synth_clip_state_dict(config.tiny(), seed=7, gain=4.0), the
ones tests/golden/towers_tiny.npz was made with (it does not carry them: they are seeded).

vision_interp.npz: sizes, r [B, P], position_embedding [1 + g*g, D] (the table the pos_table entries were resampled from) and
__versions__.  One file per size HxW (about 0.7 MB each, so that none passes 1 MiB), each with __versions__ and

    pixel_q            int8 [B,3,H,W]; pixel_values = pixel_q / 16 (exact in fp32, small on disk)
    image_emb          get_image_features(pixel_values, interpolate_pos_encoding=True).pooler_output
    pos_table          CLIPVisionEmbeddings.interpolate_pos_encoding's table [1 + gh*gw, D] (torch float32 arithmetic)
    grad.<key>         d sum(image_emb * r) / d <key>, whole, for position_embedding, class_embedding, patch_embedding, the first
                       layer's q / k / v projection weights and visual_projection
"""
import os
import sys

import numpy as np
import torch
import transformers
from transformers import CLIPConfig, CLIPModel

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from dclip_amd import config as dcfg, synth  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden")
SIZES = [(96, 96), (64, 112), (80, 50), (64, 64)]
BATCH = 2
VERSIONS = f"torch {torch.__version__}; transformers {transformers.__version__}; numpy {np.__version__}"
V = "vision_model."
GRAD_KEYS = [V + "embeddings.position_embedding.weight", V + "embeddings.class_embedding", V + "embeddings.patch_embedding.weight",
             V + "encoder.layers.0.self_attn.q_proj.weight", V + "encoder.layers.0.self_attn.k_proj.weight",
             V + "encoder.layers.0.self_attn.v_proj.weight", "visual_projection.weight"]


def hf_model(cfg: dcfg.ClipConfig, sd) -> CLIPModel:
    v, t = cfg.vision, cfg.text
    c = CLIPConfig(
        vision_config=dict(hidden_size=v.hidden_size, intermediate_size=v.intermediate_size, num_hidden_layers=v.num_hidden_layers,
                           num_attention_heads=v.num_attention_heads, image_size=v.image_size, patch_size=v.patch_size,
                           layer_norm_eps=v.layer_norm_eps, projection_dim=cfg.projection_dim),
        text_config=dict(hidden_size=t.hidden_size, intermediate_size=t.intermediate_size, num_hidden_layers=t.num_hidden_layers,
                         num_attention_heads=t.num_attention_heads, max_position_embeddings=t.max_position_embeddings,
                         vocab_size=t.vocab_size, bos_token_id=t.bos_token_id, eos_token_id=t.eos_token_id,
                         pad_token_id=t.eos_token_id, layer_norm_eps=t.layer_norm_eps, projection_dim=cfg.projection_dim),
        projection_dim=cfg.projection_dim)
    c._attn_implementation = "eager"
    m = CLIPModel(c)
    missing, unexpected = m.load_state_dict(sd, strict=False)
    missing = [k for k in missing if "position_ids" not in k]
    assert not missing and not unexpected, (missing, unexpected)
    return m.float().eval()


def pixel_q(h: int, w: int) -> np.ndarray:
    return np.random.default_rng(h * 1000 + w).integers(-32, 33, (BATCH, 3, h, w)).astype(np.int8)


def save(name: str, arrs: dict) -> None:
    path = os.path.join(GOLDEN, name)
    np.savez_compressed(path, __versions__=np.array(VERSIONS), **arrs)
    print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB, {len(arrs) + 1} arrays)")


def main():
    cfg = dcfg.tiny()
    m = hf_model(cfg, synth.synth_clip_state_dict(cfg, seed=7, gain=4.0))
    params = dict(m.named_parameters())
    r = synth.synth_embeddings(BATCH, cfg.projection_dim, seed=11)
    save("vision_interp.npz", {"sizes": np.array(SIZES, np.int32), "r": r.numpy(),
                               "position_embedding": params[GRAD_KEYS[0]].detach().numpy().copy()})
    emb = m.vision_model.embeddings
    for h, w in SIZES:
        q = pixel_q(h, w)
        pix = torch.from_numpy(q).float() / 16.0
        m.zero_grad(set_to_none=True)
        out = m.get_image_features(pixel_values=pix, interpolate_pos_encoding=True).pooler_output
        (out * r).sum().backward()
        with torch.no_grad():
            n = 1 + (h // cfg.vision.patch_size) * (w // cfg.vision.patch_size)
            table = emb.interpolate_pos_encoding(torch.zeros(1, n, cfg.vision.hidden_size), h, w)
        arrs = {"pixel_q": q, "image_emb": out.detach().numpy().copy(), "pos_table": table.reshape(n, -1).numpy().copy()}
        for k in GRAD_KEYS:
            arrs[f"grad.{k}"] = params[k].grad.detach().numpy().copy()
        save(f"vision_interp_{h}x{w}.npz", arrs)
    print(VERSIONS)


if __name__ == "__main__":
    main()
