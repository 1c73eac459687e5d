"""hidden_act="gelu" towers end to end: HipCLIPModel at config.tiny() with seeded weights against
tests/golden/towers_gelu*.npz — HF transformers' CLIPModel with exact erf GELU in both towers, fp32 and fp64
(tools/make_gelu_golden.py; the oracle of this repository is quick-GELU only).  Forward and parameter gradients in fp32, the frozen
16-bit forwards, the packed and token-level routes, a model with one tower of each activation, and a census of the routes: a "gelu"
tower runs the stand-alone passes and never a quick-GELU epilogue or a split-fp16 entry; a "quick_gelu" tower never runs the passes.

Gates are those of the tests that cover the same route for the quick-GELU tiny tower, quoted where they are applied."""
import argparse
import dataclasses
import logging

import numpy as np
import pytest
import torch

from dclip_amd import config as dcfg, synth
from tests import schedule_checks as sc
from tests.test_model_gpu import T, hf_named_grads, relerr          # relerr: tests/test_model_gpu.py:26

pytestmark = pytest.mark.gpu

LAYERS = 2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fx(golden):
    g = golden("towers_gelu.npz")
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def grads_fx(golden):
    out = {}
    for name in ("towers_gelu_grads_vision.npz", "towers_gelu_grads_text.npz"):
        g = golden(name)
        out.update({k: g[k] for k in g.files if k != "__versions__"})
    return out


def tiny_cfg(vision="gelu", text="gelu"):
    t = dcfg.tiny()
    return dataclasses.replace(t, vision=dataclasses.replace(t.vision, hidden_act=vision), text=dataclasses.replace(t.text, hidden_act=text))


def weights(fx):
    return synth.synth_clip_state_dict(dcfg.tiny(), seed=int(fx["seed"]), gain=float(fx["gain"]))


def make_model(cfg, sd, dev):
    from dclip_amd.clip_model import from_hf_state_dict
    return from_hf_state_dict(cfg, sd, device=dev)


@pytest.fixture(scope="module")
def model(dev, fx):
    """The "gelu" model, all parameters trainable; shared, its weights never written."""
    return make_model(tiny_cfg(), weights(fx), dev)


@pytest.fixture(scope="module")
def inputs(dev, fx):
    return (torch.from_numpy(fx["pixel_q"]).float() / 16.0).to(dev), T(fx["input_ids"]).to(dev), T(fx["input_ids"])


def figures(got, want):
    """(max |got - want| / max |want|, smallest row cosine): tests/test_fullres_packed_gpu.py:41"""
    got, want = got.double().cpu(), want.double().cpu()
    return (float((got - want).abs().max() / want.abs().max()),
            float(torch.nn.functional.cosine_similarity(got, want, dim=1).min()))


# The 16-bit gates, each against the fp32 tower on the same weights and inputs.
#   bf16: tests/test_bf16_gpu.py:69, `rel < 3e-2 and float(cos) > 0.999` — the tiny tower is one of that test's two models.
#   fp16: tests/test_fp16_gpu.py:232, `rel < 1e-3 and cos > 0.99999` — set on ViT-B/32 and ViT-L/14 at gain 3.0; no test applies it
#         to the tiny tower, and tests/test_text_packed_gpu.py:110-112 records why: the quick-GELU tiny text tower in fp16 is 2.7e-3
#         (padded) and 1.5e-3 (packed) from its fp32 self, "that model is not what the gate describes".  So the fp16 gate is applied
#         where it was set — test_frozen_fp16_b32_meets_the_bar, on a "gelu" ViT-B/32 — and the tiny tower gets the bound the formats
#         give: bf16's gate over 2^3, for the three more mantissa bits fp16 rounds to (3e-2 / 8 = 3.75e-3), with fp16's cosine.
# The packed routes repeat the same pairs (tests/test_text_packed_gpu.py:126-127, tests/test_fullres_packed_gpu.py:117-118).
GATE16_B32 = {"bf16": (3e-2, 0.999), "fp16": (1e-3, 0.99999)}
GATE16 = {"bf16": (3e-2, 0.999), "fp16": (3e-2 / 8, 0.99999)}          # the tiny tower


def within16(prec, got, want, what, gate=None):
    rel, cos = figures(got, want)
    print(f"[gelu towers] {what}: {prec} against fp32: max rel err {rel:.3e}, min cosine {cos:.7f}")
    lim = (gate or GATE16)[prec]
    assert rel < lim[0] and cos > lim[1], (what, prec, rel, cos, lim)


# ------------------------------------------------------------------------------------------------ discrimination, first

def test_the_fixture_tells_the_two_activations_apart(fx):
    """The same HF model with quick-GELU is at least 10 x the 1e-3 embedding gate away: a tower that ignores hidden_act fails
    test_fp32_forward below."""
    sep_i = relerr(T(fx["image_emb_quick"]), fx["f64.image_emb"])
    sep_t = relerr(T(fx["text_emb_quick"]), fx["f64.text_emb"])
    print(f"[gelu towers] quick-GELU against gelu, HF: image {sep_i:.3e}, text {sep_t:.3e}")
    assert sep_i >= 10 * 1e-3 and sep_t >= 10 * 1e-3, (sep_i, sep_t)
    ids = fx["input_ids"]
    assert [int(np.argmax(r == dcfg.tiny().text.eos_token_id)) for r in ids] == [1, 5, 15, 9]


# ------------------------------------------------------------------------------------------------ fp32 forward

def test_fp32_forward(model, inputs, fx):
    """The gates of test_towers_tiny_forward (tests/test_model_gpu.py:68-77): hidden states < 1e-4, embeddings < 1e-3, against the
    fp32 and the fp64 rows."""
    pix, ids, _ = inputs
    for i, h in enumerate(model.hidden_states(pixel_values=pix)):
        assert relerr(h, fx[f"f32.vision_hidden.{i}"]) < 1e-4 and relerr(h, fx[f"f64.vision_hidden.{i}"]) < 1e-4, ("vision", i)
    for i, h in enumerate(model.hidden_states(input_ids=ids)):
        assert relerr(h, fx[f"f32.text_hidden.{i}"]) < 1e-4 and relerr(h, fx[f"f64.text_hidden.{i}"]) < 1e-4, ("text", i)
    with torch.no_grad():
        img, txt = model.get_image_features(pixel_values=pix), model.get_text_features(input_ids=ids)
    gimg, gtxt = model.get_image_features(pixel_values=pix), model.get_text_features(input_ids=ids)       # under grad: the saving schedules
    assert gimg.requires_grad and gtxt.requires_grad
    for what, x in (("no_grad", (img, txt)), ("grad", (gimg, gtxt))):
        e = [relerr(x[0], fx["f32.image_emb"]), relerr(x[0], fx["f64.image_emb"]), relerr(x[1], fx["f32.text_emb"]),
             relerr(x[1], fx["f64.text_emb"])]
        print(f"[gelu towers] fp32 {what}: image {e[0]:.2e} / {e[1]:.2e}, text {e[2]:.2e} / {e[3]:.2e} (against fp32 / fp64)")
        assert max(e) < 1e-3, (what, e)


def test_interpolated_position_table_route(model, dev):
    """interpolate_pos_encoding: another grid through the same layers; the unpruned and the pruned schedule agree, and the 16-bit
    forwards stay within their gates of the fp32 one."""
    pix = synth.synth_regions(2, 1, dataclasses.replace(dcfg.tiny().vision, image_size=96), seed=4)[:, 0].to(dev)
    with torch.no_grad():
        got = model.get_image_features(pixel_values=pix, interpolate_pos_encoding=True)
        hs = model.hidden_states(pixel_values=pix, interpolate_pos_encoding=True)
    from dclip_amd import ops
    v = model.config.vision
    cls_tok = hs[-1][:, 0, :].contiguous()
    p = model.vision_params()
    pooled, _, _ = ops.layernorm_fwd(cls_tok, p.post_w.detach(), p.post_b.detach(), v.layer_norm_eps, save_stats=False)
    want = ops.gemm(pooled, p.proj_w.detach(), ops.LAYOUT_NT)
    assert relerr(got, want) < 1e-5
    for prec in ("bf16", "fp16"):
        with torch.no_grad():
            within16(prec, model.get_image_features(pixel_values=pix, precision=prec, interpolate_pos_encoding=True), got, "interpolated")


# ------------------------------------------------------------------------------------------------ fp32 parameter gradients

def _objective(m, inputs, fx, dev, **text_kw):
    pix, ids, _ = inputs
    img = m.get_image_features(pixel_values=pix)
    txt = m.get_text_features(input_ids=ids, **text_kw)
    return (img * T(fx["r_img"]).to(dev)).sum() + (txt * T(fx["r_txt"]).to(dev)).sum()


def test_fp32_param_grads(dev, fx, grads_fx, inputs):
    """The gate of test_towers_tiny_param_grads (tests/test_model_gpu.py:101): < 1e-3 per stored key, everything trainable."""
    m = make_model(tiny_cfg(), weights(fx), dev)
    _objective(m, inputs, fx, dev).backward()
    grads = hf_named_grads(m)
    worst = {}
    for k, want in grads_fx.items():
        if not k.startswith("grad."):
            continue
        name = k[5:]
        worst[name] = relerr(grads[name].reshape(want.shape), want)
    print("[gelu towers] parameter gradients against fp64:", {n: f"{e:.1e}" for n, e in worst.items()})
    assert len(worst) == 31 and max(worst.values()) < 1e-3, {n: e for n, e in worst.items() if e >= 1e-3}


def _distill_module(cfg, sd, dev, freeze_mode):
    from dclip_amd.CLIP_image_distillation import CLIPImageDistillation
    from dclip_amd.patch_text_aggregation import PatchTextAggregation
    student = make_model(cfg, sd, dev)
    teacher = PatchTextAggregation(embed_dim=cfg.projection_dim, num_heads=cfg.projection_dim // 64, clip_model=student)
    teacher.load_state_dict({f"cross_modal_attention.{k}": v for k, v in
                             synth.synth_cross_modal_state_dict(cfg.projection_dim, seed=31).items()})
    hp = argparse.Namespace(learning_rate=1e-4, warmup_steps=0, total_steps=100, train_batch_size=4, eval_batch_size=4)
    return CLIPImageDistillation(hp, student, None, teacher=teacher.to(dev), freeze_mode=freeze_mode).to(dev)


@pytest.mark.parametrize("freeze_mode", ["north_star", "as_written"])
def test_distillation_step_with_a_gelu_student(dev, fx, freeze_mode):
    """CLIPImageDistillation.training_step on a "gelu" student: a finite loss, gradients on the trainable set only — the same set
    a quick-GELU student gets — and a loss that is the gelu network's, not the quick-GELU one's."""
    cfg = dcfg.tiny()
    B = 6
    batch = {"pixel_values": synth.synth_pixel_values(B, cfg.vision, seed=0), "input_ids": synth.synth_input_ids(B, cfg.text, seed=3, ragged=True),
             "teacher_image_emb": synth.synth_embeddings(B, cfg.projection_dim, seed=1),
             "teacher_text_emb": synth.synth_embeddings(B, cfg.projection_dim, seed=5)}
    seen = {}
    for act in ("gelu", "quick_gelu"):
        mod = _distill_module(tiny_cfg(act, act), weights(fx), dev, freeze_mode)
        loss = mod.training_step(batch)
        loss.backward()
        assert bool(torch.isfinite(loss)), (act, float(loss))
        have = set()
        for k, prm in mod.student.named_parameters():
            if not prm.requires_grad:
                assert prm.grad is None, (act, k)
            elif prm.grad is not None:
                assert bool(torch.isfinite(prm.grad).all()), (act, k)
                have.add(k)
        seen[act] = (float(loss.detach()), have)
    assert seen["gelu"][1] == seen["quick_gelu"][1] and seen["gelu"][1]
    if freeze_mode == "north_star":
        assert "vision_model.encoder.layers.0.mlp.fc1.weight" in seen["gelu"][1]
    else:
        assert "vision_model.encoder.layers.0.mlp.fc1.weight" not in seen["gelu"][1]
        assert "text_model.encoder.layers.0.mlp.fc1.weight" in seen["gelu"][1]
    assert abs(seen["gelu"][0] - seen["quick_gelu"][0]) > 1e-5 * abs(seen["gelu"][0])


# ------------------------------------------------------------------------------------------------ frozen 16-bit forwards

@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_frozen_16bit_forwards(model, inputs, prec):
    pix, ids, _ = inputs
    with torch.no_grad():
        img32, txt32 = model.get_image_features(pixel_values=pix), model.get_text_features(input_ids=ids)
        s32, t32, e32 = model.text_token_level(ids)
        img, txt = model.get_image_features(pixel_values=pix, precision=prec), model.get_text_features(input_ids=ids, precision=prec)
        s16, t16, e16 = model.text_token_level(ids, precision=prec)
        assert torch.equal(img, model.get_image_features(pixel_values=pix, precision=prec))
    assert torch.equal(e16, e32)
    within16(prec, img, img32, "image")
    within16(prec, txt, txt32, "text")
    within16(prec, s16, s32, "text (token pass)")


def test_frozen_fp16_b32_meets_the_bar(dev):
    """The 1e-3 embedding bar of the fp16 towers on the model, weights and inputs it was set on (tests/test_fp16_gpu.py:202-232:
    ViT-B/32, gain 3.0, four region crops of seed 2, six ragged captions of seed 3), with hidden_act="gelu" in both towers."""
    base = dcfg.vit_b32()
    cfg = dataclasses.replace(base, vision=dataclasses.replace(base.vision, hidden_act="gelu"),
                              text=dataclasses.replace(base.text, hidden_act="gelu"))
    m = make_model(cfg, synth.synth_clip_state_dict(base, seed=0, gain=3.0), dev)
    pix = synth.synth_regions(4, 1, cfg.vision, seed=2)[:, 0].to(dev)
    ids = synth.synth_input_ids(6, cfg.text, seed=3, ragged=True).to(dev)
    with torch.no_grad():
        img32, txt32, s32 = m.get_image_features(pixel_values=pix), m.get_text_features(input_ids=ids), m.text_token_level(ids)[0]
        for prec in ("fp16", "bf16"):
            within16(prec, m.get_image_features(pixel_values=pix, precision=prec), img32, "ViT-B/32 image", GATE16_B32)
            within16(prec, m.get_text_features(input_ids=ids, precision=prec), txt32, "ViT-B/32 text", GATE16_B32)
            within16(prec, m.text_token_level(ids, precision=prec)[0], s32, "ViT-B/32 text (token pass)", GATE16_B32)


def test_16bit_training_of_the_gelu_vision_tower_is_refused_and_frozen_use_works(model, inputs):
    pix = inputs[0]
    for prec in ("bf16", "fp16-mixed"):
        with pytest.raises(NotImplementedError, match="hidden_act"):
            model.get_image_features(pixel_values=pix, precision=prec)
        with torch.no_grad():
            assert bool(torch.isfinite(model.get_image_features(pixel_values=pix, precision=prec)).all())


# ------------------------------------------------------------------------------------------------ packed and token-level routes

def test_packed_text_equals_padded(model, inputs, fx):
    """tests/test_text_packed_gpu.py:95 (`e32 < 1e-3 and e64 < 1e-3` against the golden rows) and :245 (`err < 1e-3 and cos >
    0.99999` against the padded result); the 16-bit packed towers against the fp32 packed one, :126-127, with the packed 16-bit
    attention core off and on."""
    pix, ids, ids_host = inputs
    with torch.no_grad():
        padded = model.get_text_features(input_ids=ids)
        packed = model.get_text_features(input_ids=ids_host, packed_lens=True)
    assert relerr(packed, fx["f32.text_emb"]) < 1e-3 and relerr(packed, fx["f64.text_emb"]) < 1e-3
    err, cos = figures(packed, padded)
    assert err < 1e-3 and cos > 0.99999, (err, cos)
    try:
        for attn16 in (False, True):
            model.packed_attention16 = attn16
            for prec in ("bf16", "fp16"):
                with torch.no_grad():
                    within16(prec, model.get_text_features(input_ids=ids_host, packed_lens=True, precision=prec), packed,
                             f"packed text, attention16={attn16}")
    finally:
        model.packed_attention16 = None


def test_token_level_routes(model, inputs, fx):
    """text_token_level / text_token_level_packed: the sentence row is text_emb (< 1e-3, tests/test_model_gpu.py:79), the packed
    token rows are the padded ones; fp32, then one 16-bit precision with the packed attention core off and on."""
    pix, ids, ids_host = inputs
    sent, tokens, eos = model.text_token_level(ids)
    assert eos.tolist() == [1, 5, 15, 9]
    assert relerr(sent, fx["f32.text_emb"]) < 1e-3 and relerr(sent, fx["f64.text_emb"]) < 1e-3
    psent, ptok, cu, tables = model.text_token_level_packed(ids_host)
    assert relerr(psent, fx["f32.text_emb"]) < 1e-3 and relerr(psent, fx["f64.text_emb"]) < 1e-3
    hcu = tables["cu_seqlens"].tolist()
    for b in range(ids.shape[0]):
        assert relerr(ptok[hcu[b]:hcu[b + 1]], tokens[b, :hcu[b + 1] - hcu[b]]) < 1e-3, b
    within16("fp16", model.text_token_level(ids, precision="fp16")[0], sent, "token level")
    try:
        for attn16 in (False, True):
            model.packed_attention16 = attn16
            within16("fp16", model.text_token_level_packed(ids_host, precision="fp16")[0], psent, f"packed token level, attention16={attn16}")
    finally:
        model.packed_attention16 = None


def test_packed_training_gradients_equal_the_padded_ones(dev, fx, grads_fx, inputs):
    """packed_train=True.  The gate of tests/test_text_packed_train_gpu.py (sc.gates32): per tensor, the 2-norm
    relative error against fp64 is at most 8 E_ref32 + 16 * 2^-24, E_ref32 the fp32 reference's own error — for the packed AND the
    padded tower; packed against padded is printed.  (The fixture stores the fp64 gradients rounded to fp32: 2^-24 of slack the
    gate's floor covers 16 times.)"""
    pix, ids, ids_host = inputs
    r = T(fx["r_txt"]).to(dev)
    got = {}
    for what, kw in (("padded", {}), ("packed", {"packed_lens": True, "packed_train": True})):
        m = make_model(tiny_cfg(), weights(fx), dev)
        out = m.get_text_features(input_ids=ids_host if kw else ids, **kw)
        assert out.requires_grad
        (out * r).sum().backward()
        got[what] = hf_named_grads(m)
    keys = [k[7:] for k in grads_fx if k.startswith("grad32.")]
    assert len(keys) == 15
    want = {k: T(grads_fx[f"grad.{k}"]) for k in keys}
    gate = sc.gates32({k: sc.rel_err(T(grads_fx[f"grad32.{k}"]), want[k]) for k in keys})
    for what in ("padded", "packed"):
        ratios = sc.check_anchor({k: got[what][k].cpu() for k in keys}, want, gate, what)
        print(f"[gelu towers] {what} E / gate:", {k.split('text_model.')[-1]: f"{v:.3f}" for k, v in ratios.items()})
    print("[gelu towers] packed against padded:", {k.split('text_model.')[-1]: f"{sc.rel_err(got['packed'][k], got['padded'][k]):.1e}" for k in keys})


def test_packed_crops_equal_per_crop_calls(model, dev):
    """get_image_features_crops against per-crop get_image_features(interpolate_pos_encoding=True): tests/test_fullres_packed_gpu.py
    :100 (`err < 1e-3 and cos > 0.99999`); the 16-bit packed towers against the fp32 packed one, :117-118, attention core off / on."""
    from PIL import Image
    from dclip_amd.patch_text_aggregation import PatchTextAggregation
    from tests.test_fullres_packed_gpu import CROP_BOXES, flat_boxes
    teacher = PatchTextAggregation(embed_dim=model.config.projection_dim, num_heads=1, clip_model=model).to(dev)
    tok = teacher.patch_tokenizer
    images = [Image.fromarray(np.random.default_rng(b).integers(0, 255, (80, 96, 3), dtype=np.uint8)) for b in range(2)]
    u8, dims = tok._upload_u8(images)
    flat = flat_boxes([CROP_BOXES, CROP_BOXES])
    got = model.get_image_features_crops(u8, dims, flat)
    want = []
    with torch.no_grad():
        for b, x1, y1, x2, y2 in flat:
            crop = tok.full_resolution_transform(images[b].crop((x1, y1, x2, y2))).unsqueeze(0).to(dev)
            want.append(model.get_image_features(pixel_values=crop, interpolate_pos_encoding=True)[0])
    err, cos = figures(got, torch.stack(want))
    print(f"[gelu towers] packed crops against per-crop calls: max rel err {err:.3e}, min cosine {cos:.8f}")
    assert err < 1e-3 and cos > 0.99999, (err, cos)
    try:
        for attn16 in (False, True):
            model.packed_attention16 = attn16
            for prec in ("bf16", "fp16"):
                within16(prec, model.get_image_features_crops(u8, dims, flat, precision=prec), got, f"packed crops, attention16={attn16}")
    finally:
        model.packed_attention16 = None


def test_meta_teacher_on_a_gelu_model(model, dev, fx):
    """PatchTextAggregation as a teacher on a "gelu" model: the global embedding is finite and is not the quick-GELU model's."""
    from dclip_amd.patch_text_aggregation import PatchTextAggregation
    cfg = model.config
    ids = synth.synth_input_ids(3, cfg.text, seed=9, ragged=True, min_len=4).to(dev)
    regions = synth.synth_regions(3, 2, cfg.vision, seed=3).to(dev)
    out = {}
    quick = make_model(dcfg.tiny(), weights(fx), dev)
    for name, clip in (("gelu", model), ("quick_gelu", quick)):
        t = PatchTextAggregation(embed_dim=cfg.projection_dim, num_heads=cfg.projection_dim // 64, clip_model=clip)
        t.load_state_dict({f"cross_modal_attention.{k}": v for k, v in synth.synth_cross_modal_state_dict(cfg.projection_dim, seed=31).items()})
        out[name] = t.to(dev).compute_global_embedding_tensors(regions, ids, torch.tensor([2, 1, 2]))
        assert bool(torch.isfinite(out[name]).all()) and float(out[name].detach().abs().max()) > 0
    assert relerr(out["quick_gelu"], out["gelu"]) > 1e-4


# ------------------------------------------------------------------------------------------------ one tower of each activation

def test_mixed_model(dev, fx, golden, inputs):
    """Vision "gelu" (the gelu fixture's weights) beside text "quick_gelu" (the weights of towers_tiny.npz): each tower follows its
    own field."""
    g = golden("towers_tiny.npz")
    sd = weights(fx)
    quick_sd = synth.synth_clip_state_dict(dcfg.tiny(), seed=7, gain=4.0)
    for k in sd:
        if k.startswith("text_"):
            sd[k] = quick_sd[k]
    m = make_model(tiny_cfg("gelu", "quick_gelu"), sd, dev)
    with torch.no_grad():
        img = m.get_image_features(pixel_values=inputs[0])
        txt = m.get_text_features(input_ids=T(g["input_ids"]).to(dev))
    assert relerr(img, fx["f32.image_emb"]) < 1e-3 and relerr(img, fx["f64.image_emb"]) < 1e-3
    assert relerr(txt, g["f32.text_emb"]) < 1e-3 and relerr(txt, g["f64.text_emb"]) < 1e-3


# ------------------------------------------------------------------------------------------------ route census

class OpsCensus:
    """Wraps dclip_amd.ops while active: counts gelu_erf / gelu_erf_bwd, records every fp32 GEMM's epilogue bits and every call
    of an fp16 / split-fp16 entry; the 16-bit GEMMs of the frozen towers (bound at import into engine._OPS16) report `gelu=`."""

    def __init__(self, mp):
        from dclip_amd import engine, ops
        self.erf, self.erf_bwd, self.epilogues, self.f16_calls, self.gelu16 = [], 0, [], [], 0
        o_erf, o_bwd, o_gemm = ops.gelu_erf, ops.gelu_erf_bwd, ops.gemm

        def erf(h, out=None):
            self.erf.append(h.dtype)
            return o_erf(h, out=out)

        def erf_bwd(h, dg, out=None):
            self.erf_bwd += 1
            return o_bwd(h, dg, out=out)

        def gemm(a, b, layout, **kw):
            self.epilogues.append(int(kw.get("epilogue", 0)))
            return o_gemm(a, b, layout, **kw)
        mp.setattr(ops, "gelu_erf", erf), mp.setattr(ops, "gelu_erf_bwd", erf_bwd), mp.setattr(ops, "gemm", gemm)
        for name in dir(ops):
            if ("f16" in name or "split16" in name) and callable(getattr(ops, name)) and not name.startswith("_"):
                mp.setattr(ops, name, self._spy(name, getattr(ops, name)))
        for k in engine._OPS16.values():
            mp.setattr(k, "_gemm", self._spy16(k._gemm))

    def _spy(self, name, fn):
        def spy(*a, **kw):
            self.f16_calls.append(name)
            return fn(*a, **kw)
        return spy

    def _spy16(self, fn):
        def spy(*a, **kw):
            self.gelu16 += bool(kw.get("gelu"))
            return fn(*a, **kw)
        return spy

    def quick_epilogues(self):
        from dclip_amd import ops
        return sum(1 for e in self.epilogues if e & (ops.EPI_GELU | ops.EPI_DGELU))


@pytest.fixture
def switches(monkeypatch, caplog):
    """Every split-fp16 switch at its default and an empty log-once set: what a fresh process has."""
    from dclip_amd import engine
    for name, value in (("_VSPLIT16", True), ("_VSPLIT16_FC1_EPI", True), ("_VSPLIT16_BWD", True), ("_VSPLIT16_WGRAD", True),
                        ("_VSPLIT16_DYSTATS", True), ("_SPLIT16", True), ("_SPLIT16_FC1_EPI", True), ("_VSPLIT16_DROP32", False)):
        monkeypatch.setattr(engine, name, value)
    monkeypatch.setattr(engine, "_SPLIT16_LOGGED", set())
    caplog.set_level(logging.WARNING, logger="dclip_amd")
    return caplog


def declined(caplog, what):
    return [r.getMessage() for r in caplog.records if r.getMessage().startswith(what) and "hidden_act='gelu'" in r.getMessage()]


def test_census_fp32_forward_and_backward(dev, fx, inputs, monkeypatch, switches):
    m = make_model(tiny_cfg(), weights(fx), dev)
    c = OpsCensus(monkeypatch)
    for _ in range(2):                                           # twice: the fall-back is logged once
        obj = _objective(m, inputs, fx, dev)
    obj.backward()
    m.text_model.requires_grad_(False), m.text_projection.requires_grad_(False)
    with torch.no_grad():                                        # a FROZEN text tower: the split default of DCLIP_TEXT_SPLIT16
        m.get_text_features(input_ids=inputs[1])
    torch.cuda.synchronize()
    assert c.erf == [torch.float32] * (2 * 2 * LAYERS + LAYERS), c.erf          # two towers, two forwards; one frozen text forward
    assert c.erf_bwd == 2 * LAYERS                                # every layer of both towers trains
    assert c.quick_epilogues() == 0 and c.gelu16 == 0 and c.f16_calls == [], (c.quick_epilogues(), c.gelu16, c.f16_calls)
    assert len(declined(switches, "split-fp16 vision tower")) == 1 and len(declined(switches, "split-fp16 text tower")) == 1


def test_census_split16_switches(dev, fx, inputs, monkeypatch, switches):
    """precision="fp32-split16", text_train_split16 and the token-level split pass: plain fp32 with the stand-alone passes."""
    pix, ids, ids_host = inputs
    m = make_model(tiny_cfg(), weights(fx), dev)
    m.text_train_split16 = True
    c = OpsCensus(monkeypatch)
    with torch.no_grad():
        img = m.get_image_features(pixel_values=pix, precision="fp32-split16")
        sent = m.text_token_level(ids, precision="fp32-split16")[0]
        psent = m.text_token_level_packed(ids_host, precision="fp32-split16")[0]
    txt = m.get_text_features(input_ids=ids)                      # trainable, text_train_split16: declined
    ptxt = m.get_text_features(input_ids=ids_host, packed_lens=True, packed_train=True)
    (txt.sum() + ptxt.sum()).backward()
    torch.cuda.synchronize()
    assert c.erf == [torch.float32] * (5 * LAYERS) and c.erf_bwd == 2 * LAYERS, (c.erf, c.erf_bwd)
    assert c.quick_epilogues() == 0 and c.f16_calls == [], (c.quick_epilogues(), c.f16_calls)
    assert relerr(img, fx["f64.image_emb"]) < 1e-3 and relerr(sent, fx["f64.text_emb"]) < 1e-3 and relerr(psent, fx["f64.text_emb"]) < 1e-3
    assert relerr(txt, fx["f64.text_emb"]) < 1e-3 and relerr(ptxt, fx["f64.text_emb"]) < 1e-3
    for what in ("split-fp16 frozen vision tower", "split-fp16 text tower", "split-fp16 trainable text tower"):
        assert len(declined(switches, what)) == 1, (what, [r.getMessage() for r in switches.records])


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_census_frozen_16bit(model, inputs, monkeypatch, prec):
    pix, ids, ids_host = inputs
    c = OpsCensus(monkeypatch)
    with torch.no_grad():
        model.get_image_features(pixel_values=pix, precision=prec)
        model.get_text_features(input_ids=ids, precision=prec)
        model.get_text_features(input_ids=ids_host, packed_lens=True, precision=prec)
        model.text_token_level(ids, precision=prec)
    torch.cuda.synchronize()
    dtype = torch.bfloat16 if prec == "bf16" else torch.float16
    assert c.erf == [dtype] * (4 * LAYERS) and c.gelu16 == 0 and c.quick_epilogues() == 0, (c.erf, c.gelu16)


def test_census_quick_gelu_model_never_runs_the_passes(dev, fx, inputs, monkeypatch, switches):
    pix, ids, ids_host = inputs
    m = make_model(dcfg.tiny(), weights(fx), dev)
    c = OpsCensus(monkeypatch)
    _objective(m, inputs, fx, dev).backward()
    with torch.no_grad():
        m.get_text_features(input_ids=ids)
        m.get_image_features(pixel_values=pix, precision="bf16")
        m.get_text_features(input_ids=ids_host, packed_lens=True, precision="fp16")
        got = m.get_image_features(pixel_values=pix)
    torch.cuda.synchronize()
    assert c.erf == [] and c.erf_bwd == 0
    assert c.quick_epilogues() > 0 and c.gelu16 == 2 * LAYERS and c.f16_calls, "the quick-GELU routes are the parent's"
    assert not [r for r in switches.records if "hidden_act" in r.getMessage()]
    assert relerr(got, fx["image_emb_quick"]) < 1e-3              # and it computes HF's quick-GELU network
