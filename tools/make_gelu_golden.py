#!/usr/bin/env python
"""Write tests/golden/towers_gelu.npz, towers_gelu_grads_vision.npz and towers_gelu_grads_text.npz: the tiny towers with
hidden_act="gelu" (exact erf GELU) in BOTH towers, run by HF transformers' CLIPModel (eager attention, CPU) in float32 and in
float64, forward and backward.  The oracle of this repository is quick-GELU only, so HF is the reference here.

    python tools/make_gelu_golden.py

Third-party code only (torch, transformers); the weights are synth.synth_clip_state_dict(config.tiny(), seed=SEED, gain=GAIN):
seeded, not stored.  GAIN = 2.0, not the 4.0 of tests/golden/towers_tiny.npz: the fixture has to tell the two activations apart —
the quick-GELU embeddings of the same model must differ from the gelu ones by at least 10 x the 1e-3 embedding gate, so that a
tower which ignores hidden_act fails — and how far they differ is NOT monotonic in the gain.  Measured with this script's model
(relative to the largest |embedding|, image / text, x 1e-3; the activations differ by at most 0.02 anywhere, and two layers and
a final LayerNorm do not amplify that): gain 1: 3.5 / 9.8, 2: 9.8 / 9.9, 3: 7.0 / 7.4, 4: 4.0 / 4.0, 8: 6.5 / 2.5, 16: 2.0 / 0.4,
32: 0.2 / 0.2.  No gain reaches 10 on every input; at 2.0 the input seeds below do (image 10.8, text 13.7 — chosen among seeds
0 .. 11 for exactly that, which is asserted before anything is written).

towers_gelu.npz (everything but the gradients):
    pixel_q                     int8 [2,3,64,64]; pixel_values = pixel_q / 16 (exact in fp32)
    input_ids                   int64 [4,16]: BOS, words, first EOS at 1, 5, 15 and 9, then junk that is no EOS
    f32.* / f64.*               image_emb [2,P], text_emb [4,P], vision_hidden.<i> [2,S,D] (i = 0: after the pre-LayerNorm),
                                text_hidden.<i> [4,T,D] (i = 0: the embeddings; before final_layer_norm), i = 0 .. layers
    image_emb_quick / text_emb_quick   float32, the SAME model with hidden_act="quick_gelu": what a tower that ignores the field gives
    r_img [2,P], r_txt [4,P]    the objective's weights: obj = sum(image_emb r_img) + sum(text_emb r_txt)
    seed, gain                  of synth.synth_clip_state_dict: the tests rebuild the weights from them
towers_gelu_grads_{vision,text}.npz:
    grad.<HF key>               d obj / d <key> of the float64 run, stored as float32 (the gate on them is 1e-3), for GRAD_KEYS
    grad32.<HF key>             (text file only) the same of the float32 run: the reference's own fp32 error E_ref32
Every file carries __versions__.
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
SEED, GAIN = 7, 2.0
PIXEL_SEED, IDS_SEED = 10, 3            # see GAIN above
VERSIONS = f"torch {torch.__version__}; transformers {transformers.__version__}; numpy {np.__version__}"
EOS_AT = (1, 5, 15, 9)


def tower_keys(tower: str):
    L = f"{tower}.encoder.layers."
    keys = [L + f"{i}.mlp.{fc}.bias" for i in (0, 1) for fc in ("fc1", "fc2")]
    keys += [L + f"0.mlp.{fc}.weight" for fc in ("fc1", "fc2")]
    keys += [L + f"{i}.layer_norm2.{k}" for i in (0, 1) for k in ("weight", "bias")]
    keys += [L + f"0.self_attn.q_proj.{k}" for k in ("weight", "bias")]
    return keys


GRAD_KEYS = {
    "vision": tower_keys("vision_model") + ["vision_model.embeddings.patch_embedding.weight", "vision_model.embeddings.class_embedding",
                                            "vision_model.embeddings.position_embedding.weight", "visual_projection.weight"],
    "text": tower_keys("text_model") + ["text_model.embeddings.token_embedding.weight",
                                        "text_model.embeddings.position_embedding.weight", "text_projection.weight"],
}


def hf_model(cfg: dcfg.ClipConfig, sd, act: str, dtype) -> CLIPModel:
    v, t = cfg.vision, cfg.text
    c = CLIPConfig(
        vision_config=dict(hidden_size=v.hidden_size, intermediate_size=v.intermediate_size, num_hidden_layers=v.num_hidden_layers,
                           num_attention_heads=v.num_attention_heads, image_size=v.image_size, patch_size=v.patch_size,
                           layer_norm_eps=v.layer_norm_eps, projection_dim=cfg.projection_dim, hidden_act=act),
        text_config=dict(hidden_size=t.hidden_size, intermediate_size=t.intermediate_size, num_hidden_layers=t.num_hidden_layers,
                         num_attention_heads=t.num_attention_heads, max_position_embeddings=t.max_position_embeddings,
                         vocab_size=t.vocab_size, bos_token_id=t.bos_token_id, eos_token_id=t.eos_token_id,
                         pad_token_id=t.eos_token_id, layer_norm_eps=t.layer_norm_eps, projection_dim=cfg.projection_dim,
                         hidden_act=act),
        projection_dim=cfg.projection_dim)
    c._attn_implementation = "eager"
    m = CLIPModel(c)
    assert m.config.vision_config.hidden_act == act and m.config.text_config.hidden_act == act
    missing, unexpected = m.load_state_dict(sd, strict=False)
    missing = [k for k in missing if "position_ids" not in k]
    assert not missing and not unexpected, (missing, unexpected)
    return m.to(dtype).eval()


def make_input_ids(t: dcfg.TextConfig) -> np.ndarray:
    ids = np.random.default_rng(IDS_SEED).integers(1, min(t.bos_token_id, t.eos_token_id), (len(EOS_AT), t.max_position_embeddings))
    ids[:, 0] = t.bos_token_id
    for b, e in enumerate(EOS_AT):
        ids[b, e] = t.eos_token_id                  # what follows stays random words: junk behind the first EOS, never an EOS
    assert [int(np.argmax(row == t.eos_token_id)) for row in ids] == list(EOS_AT) and (ids == t.eos_token_id).sum() == len(EOS_AT)
    return ids.astype(np.int64)


def run(m: CLIPModel, pix, ids):
    """(image_emb, text_emb, vision hidden states, text hidden states) through the public call surface of the model."""
    vo = m.vision_model(pixel_values=pix, output_hidden_states=True)
    to = m.text_model(input_ids=ids, output_hidden_states=True)
    img = m.visual_projection(vo.pooler_output)
    txt = m.text_projection(to.pooler_output)
    n = m.config.vision_config.num_hidden_layers + 1
    assert len(vo.hidden_states) == n and len(to.hidden_states) == n
    return img, txt, vo.hidden_states, to.hidden_states


def relerr(a, b) -> float:
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def save(name: str, arrs: dict) -> None:
    path = os.path.join(GOLDEN, name)
    np.savez_compressed(path, __versions__=np.array(VERSIONS), **arrs)
    size = os.path.getsize(path)
    assert size < (1 << 20), (name, size)
    print(f"wrote {path}  ({size / 1024:.1f} KiB, {len(arrs) + 1} arrays)")


def main():
    cfg = dcfg.tiny()
    sd = synth.synth_clip_state_dict(cfg, seed=SEED, gain=GAIN)
    q = np.random.default_rng(PIXEL_SEED).integers(-32, 33, (2, 3, cfg.vision.image_size, cfg.vision.image_size)).astype(np.int8)
    ids_np = make_input_ids(cfg.text)
    ids = torch.from_numpy(ids_np)
    r_img = synth.synth_embeddings(2, cfg.projection_dim, seed=11)
    r_txt = synth.synth_embeddings(len(EOS_AT), cfg.projection_dim, seed=12)
    arrs = {"pixel_q": q, "input_ids": ids_np, "r_img": r_img.numpy(), "r_txt": r_txt.numpy(), "seed": np.array(SEED),
            "gain": np.array(GAIN)}
    grads = {}
    for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        m = hf_model(cfg, sd, "gelu", dtype)
        pix = torch.from_numpy(q).to(dtype) / 16.0
        img, txt, vh, th = run(m, pix, ids)
        # the same embeddings through get_*_features, the call the towers mirror
        with torch.no_grad():
            gi = m.get_image_features(pixel_values=pix)
            gt = m.get_text_features(input_ids=ids)
        gi, gt = getattr(gi, "pooler_output", gi), getattr(gt, "pooler_output", gt)
        assert torch.equal(gi, img.detach()) and torch.equal(gt, txt.detach())
        arrs[f"{tag}.image_emb"], arrs[f"{tag}.text_emb"] = img.detach().numpy().copy(), txt.detach().numpy().copy()
        for i, h in enumerate(vh):
            arrs[f"{tag}.vision_hidden.{i}"] = h.detach().numpy().copy()
        for i, h in enumerate(th):
            arrs[f"{tag}.text_hidden.{i}"] = h.detach().numpy().copy()
        ((img * r_img.to(dtype)).sum() + (txt * r_txt.to(dtype)).sum()).backward()
        params = dict(m.named_parameters())
        if tag == "f64":
            for tower, keys in GRAD_KEYS.items():
                grads[tower] = {f"grad.{k}": params[k].grad.detach().numpy().astype(np.float32) for k in keys}
        else:       # the fp32 reference's own error, for the packed-training gate 8 E_ref32 + 16 2^-24 (text tower only)
            grads32 = {f"grad32.{k}": params[k].grad.detach().numpy().copy() for k in GRAD_KEYS["text"]}
    with torch.no_grad():
        mq = hf_model(cfg, sd, "quick_gelu", torch.float32)
        img_q, txt_q, _, _ = run(mq, torch.from_numpy(q).float() / 16.0, ids)
    arrs["image_emb_quick"], arrs["text_emb_quick"] = img_q.numpy().copy(), txt_q.numpy().copy()
    sep_i, sep_t = relerr(arrs["image_emb_quick"], arrs["f64.image_emb"]), relerr(arrs["text_emb_quick"], arrs["f64.text_emb"])
    print(f"gain {GAIN}: quick-GELU against gelu embeddings, relative: image {sep_i:.3e}, text {sep_t:.3e} (needed: >= 1e-2)")
    print(f"fp32 against fp64 gelu embeddings: image {relerr(arrs['f32.image_emb'], arrs['f64.image_emb']):.3e}, "
          f"text {relerr(arrs['f32.text_emb'], arrs['f64.text_emb']):.3e}")
    assert min(sep_i, sep_t) >= 1e-2, "the two activations must differ by 10 x the 1e-3 embedding gate: choose GAIN / the input seeds so that they do"
    save("towers_gelu.npz", arrs)
    save("towers_gelu_grads_vision.npz", grads["vision"])
    save("towers_gelu_grads_text.npz", {**grads["text"], **grads32})
    print(VERSIONS)


if __name__ == "__main__":
    main()
