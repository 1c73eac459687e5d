"""The packed frozen towers with the 16-bit MFMA attention core switched on: HipCLIPModel.packed_attention16
on get_image_features_crops, get_text_features(packed_lens=...) and text_token_level_packed.  (a) its error against packed fp32
beside the padded 16-bit tower's against padded fp32 on inputs both paths take; (b) ragged inputs within the frozen-tower gate;
(c) independence of the sequences in a pack; (d) the launch lists, on and off; (e) a crop above the one-row kernel's 512 tokens;
(f) the teacher and a prefetched teacher."""
import argparse
import contextlib

import pytest
import torch

from dclip_amd import config as dcfg, synth
from dclip_amd.clip_model import from_hf_state_dict, packed_text_tables
from tests.test_fullres_packed_gpu import CROP_BOXES, Census, figures, flat_boxes, photo
from tests.test_split16_gpu import _text_model
from tests.test_vision_interp_gpu import BOXES

pytestmark = pytest.mark.gpu

TILED, ROW = "attention_varlen_fwd_%s", "attention_varlen_row_fwd_%s"
F32_SITES = {"attention_varlen_fwd", "attention_varlen_causal_fwd"}
SHORT = {"bf16": "bf16", "fp16": "f16"}
GATE = (3e-2, 0.999)                                   # the frozen bf16 towers' gate (tests/test_bf16_gpu.py)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def tiny(dev):
    """The tiny model of tests/test_fullres_packed_gpu.py, frozen, and a teacher on it (for its uploads and transforms)."""
    from dclip_amd.patch_text_aggregation import PatchTextAggregation
    cfg = dcfg.tiny()
    clip = from_hf_state_dict(cfg, synth.synth_clip_state_dict(cfg, seed=7, gain=4.0), device=dev)
    clip.requires_grad_(False)
    teacher = PatchTextAggregation(embed_dim=cfg.projection_dim, num_heads=1, clip_model=clip).to(dev)
    return cfg, clip, teacher


@pytest.fixture(scope="module")
def b32(dev):
    """The synthetic ViT-B/32 of tests/test_text_packed_gpu.py (gain 3.0), frozen."""
    return _text_model(3.0, dev)


@contextlib.contextmanager
def switched(model, value):
    before = model.packed_attention16
    model.packed_attention16 = value
    try:
        yield model
    finally:
        model.packed_attention16 = before


def names(census):
    return [s.split(".")[0] for s in census.names]


def within_twice(e_new, e_ref):
    """relerr and 1 - cosine, each at most twice the padded tower's."""
    return e_new[0] <= 2.0 * e_ref[0] and (1.0 - e_new[1]) <= 2.0 * (1.0 - e_ref[1])


# ------------------------------------------------------------------------------------------------ (a) against the padded tower

@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_vision_error_beside_the_padded_16_bit_tower(dev, tiny, prec):
    """Crops of the model's own size, so the padded tower applies too.  e_ref: padded 16-bit against padded fp32; e_new: packed
    with the 16-bit core against packed fp32.  Both round q, k, v, P and the context to 16 bits and differ in summation order
    and row count: e_new <= 2 e_ref on both figures.
    Measured on an MI355X (relerr / 1 - cosine): bf16 e_ref 7.31e-3 / 3.86e-5, e_new 7.31e-3 / 3.86e-5 (fp32 core: 7.01e-3 /
    2.96e-5); fp16 e_ref 8.45e-4 / 5.83e-7, e_new 8.45e-4 / 5.83e-7 (fp32 core: 7.76e-4 / 3.18e-7).  DESIGN.md §24."""
    cfg, clip, teacher = tiny
    images = [photo(80, 96, b) for b in range(2)]
    boxes = [(0, 0, 64, 64), (16, 8, 80, 72), (32, 16, 96, 80)]
    flat = [(b, *box) for b in range(2) for box in boxes]
    u8, dims = teacher.patch_tokenizer._upload_u8(images)
    tok = teacher.patch_tokenizer
    pix = torch.stack([tok.full_resolution_transform(images[b].crop(box)) for b, *box in flat]).to(dev)
    assert tuple(pix.shape[-2:]) == (cfg.vision.image_size, cfg.vision.image_size)
    with torch.no_grad():
        padded32 = clip.get_image_features(pixel_values=pix)
        padded16 = clip.get_image_features(pixel_values=pix, precision=prec)
        packed32 = clip.get_image_features_crops(u8, dims, flat)
        with switched(clip, False):
            off = clip.get_image_features_crops(u8, dims, flat, precision=prec)
        with switched(clip, True):
            on = clip.get_image_features_crops(u8, dims, flat, precision=prec)
    e_ref, e_new, e_off = figures(padded16, padded32), figures(on, packed32), figures(off, packed32)
    print(f"vision {prec}: e_ref (padded) {e_ref[0]:.3e} / 1-cos {1 - e_ref[1]:.3e}; e_new (packed + 16-bit core) {e_new[0]:.3e} / "
          f"{1 - e_new[1]:.3e}; packed with the fp32 core {e_off[0]:.3e} / {1 - e_off[1]:.3e}")
    assert bool(torch.isfinite(on).all()) and within_twice(e_new, e_ref), (e_new, e_ref)


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_text_error_beside_the_padded_16_bit_tower(dev, b32, prec):
    """Captions that are all 77 tokens long, so nothing is cut: as above for the text tower of the synthetic ViT-B/32.
    Measured on an MI355X: bf16 e_ref 5.90e-3 / 2.01e-5, e_new 5.67e-3 / 2.16e-5 (fp32 core: 5.50e-3 / 1.82e-5); fp16 e_ref
    8.07e-4 / 3.28e-7, e_new 8.50e-4 / 3.42e-7 (fp32 core: 7.96e-4 / 3.31e-7)."""
    cfg, sd, m = b32
    ids = synth.synth_input_ids(6, cfg.text, seed=3, ragged=False)
    assert packed_text_tables(ids, cfg.text.eos_token_id)["lens"].tolist() == [77] * 6
    idd = ids.to(dev)
    with torch.no_grad():
        padded32 = m.get_text_features(input_ids=idd)
        padded16 = m.get_text_features(input_ids=idd, precision=prec)
        packed32 = m.get_text_features(input_ids=ids, packed_lens=True)
        with switched(m, False):
            off = m.get_text_features(input_ids=ids, packed_lens=True, precision=prec)
        with switched(m, True):
            on = m.get_text_features(input_ids=ids, packed_lens=True, precision=prec)
    e_ref, e_new, e_off = figures(padded16, padded32), figures(on, packed32), figures(off, packed32)
    print(f"text {prec}: e_ref (padded) {e_ref[0]:.3e} / 1-cos {1 - e_ref[1]:.3e}; e_new (packed + 16-bit core) {e_new[0]:.3e} / "
          f"{1 - e_new[1]:.3e}; packed with the fp32 core {e_off[0]:.3e} / {1 - e_off[1]:.3e}")
    assert bool(torch.isfinite(on).all()) and within_twice(e_new, e_ref), (e_new, e_ref)


# ------------------------------------------------------------------------------------------------ (b) ragged inputs

def test_ragged_crops_within_the_frozen_tower_gate(dev, tiny):
    """The boxes of tests/test_fullres_packed_gpu.py.  bf16 is gated (3e-2, cosine 0.999); fp16 is printed."""
    cfg, clip, teacher = tiny
    u8, dims = teacher.patch_tokenizer._upload_u8([photo(80, 96, b) for b in range(2)])
    flat = flat_boxes([CROP_BOXES, CROP_BOXES])
    f32 = clip.get_image_features_crops(u8, dims, flat)
    fig = {}
    with switched(clip, True):
        for prec in ("bf16", "fp16"):
            x = clip.get_image_features_crops(u8, dims, flat, precision=prec)
            assert x.shape == f32.shape and x.dtype == torch.float32 and bool(torch.isfinite(x).all())
            assert torch.equal(x, clip.get_image_features_crops(u8, dims, flat, precision=prec)), prec
            fig[prec] = figures(x, f32)
            print(f"ragged crops, packed {prec} + 16-bit core against packed fp32: {fig[prec][0]:.3e} / cosine {fig[prec][1]:.7f}")
    assert fig["bf16"][0] < GATE[0] and fig["bf16"][1] > GATE[1], fig


def test_ragged_captions_within_the_frozen_tower_gate(dev, b32):
    """The six ragged captions of tests/test_text_packed_gpu.py on the synthetic ViT-B/32.  bf16 gated, fp16 printed."""
    cfg, sd, m = b32
    ids = synth.synth_input_ids(6, cfg.text, seed=3, ragged=True)
    fig = {}
    with torch.no_grad(), switched(m, True):
        f32 = m.get_text_features(input_ids=ids, packed_lens=True)
        for prec in ("bf16", "fp16"):
            x = m.get_text_features(input_ids=ids, packed_lens=True, precision=prec)
            assert x.shape == f32.shape and x.dtype == torch.float32 and bool(torch.isfinite(x).all())
            assert torch.equal(x, m.get_text_features(input_ids=ids, packed_lens=True, precision=prec)), prec
            fig[prec] = figures(x, f32)
            print(f"ragged captions, packed {prec} + 16-bit core against packed fp32: {fig[prec][0]:.3e} / cosine {fig[prec][1]:.7f}")
    assert fig["bf16"][0] < GATE[0] and fig["bf16"][1] > GATE[1], fig


# ------------------------------------------------------------------------------------------------ (c) independence

@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_changing_one_crops_pixels_leaves_every_other_embedding_bit_identical(dev, tiny, prec):
    cfg, clip, teacher = tiny
    images = [photo(80, 96, 0), photo(40, 56, 1), photo(80, 96, 2)]
    flat = flat_boxes([CROP_BOXES, [((4, 3, 52, 35), 0.9)], CROP_BOXES[:3]])          # the middle image holds ONE crop
    u8, dims = teacher.patch_tokenizer._upload_u8(images)
    with switched(clip, True):
        before = clip.get_image_features_crops(u8, dims, flat, precision=prec)
        u8[1, :40, :56] = 255 - u8[1, :40, :56]
        after = clip.get_image_features_crops(u8, dims, flat, precision=prec)
    mid = len(CROP_BOXES)
    assert not torch.equal(before[mid], after[mid])
    keep = [i for i in range(len(flat)) if i != mid]
    assert torch.equal(before[keep], after[keep]) and bool(torch.isfinite(after).all())


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_changing_one_captions_words_leaves_every_other_caption_bit_identical(dev, tiny, prec):
    cfg, m, _ = tiny
    ids = synth.synth_input_ids(5, cfg.text, seed=6, ragged=True, min_len=4)
    lens = packed_text_tables(ids, cfg.text.eos_token_id)["lens"].tolist()
    victim = 2
    changed = ids.clone()
    changed[victim, 1:lens[victim] - 1] = (changed[victim, 1:lens[victim] - 1] + 1) % min(cfg.text.bos_token_id, cfg.text.eos_token_id)
    changed[victim, 1] = 1 if int(ids[victim, 1]) != 1 else 2
    assert packed_text_tables(changed, cfg.text.eos_token_id)["lens"].tolist() == lens and not torch.equal(changed, ids)
    keep = [b for b in range(ids.shape[0]) if b != victim]
    with torch.no_grad(), switched(m, True):
        before, after = (m.get_text_features(input_ids=x, packed_lens=True, precision=prec) for x in (ids, changed))
        (s0, t0, cu, tab), (s1, t1, _, _) = (m.text_token_level_packed(x, precision=prec) for x in (ids, changed))
    assert not torch.equal(before[victim], after[victim])
    assert torch.equal(before[keep], after[keep]) and bool(torch.isfinite(after).all())
    host_cu = tab["cu_seqlens"].tolist()
    rows = torch.ones(t0.shape[0], dtype=torch.bool)
    rows[host_cu[victim]:host_cu[victim + 1]] = False
    assert torch.equal(t0[rows.to(dev)], t1[rows.to(dev)]) and torch.equal(s0[keep], s1[keep])
    assert not torch.equal(t0[host_cu[victim] + 1], t1[host_cu[victim] + 1])


# ------------------------------------------------------------------------------------------------ (d) launch lists

@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_vision_launch_lists(dev, tiny, monkeypatch, prec):
    from dclip_amd import engine
    cfg, clip, teacher = tiny
    L, t = cfg.vision.num_hidden_layers, SHORT[prec]
    u8, dims = teacher.patch_tokenizer._upload_u8([photo(80, 96, b) for b in range(2)])
    flat = flat_boxes([CROP_BOXES, CROP_BOXES])
    seen, out = {}, {}
    monkeypatch.setattr(engine, "_PACKED_ATTN16", False)
    for value in (None, False, True):
        with switched(clip, value), Census(monkeypatch) as c:
            out[value] = clip.get_image_features_crops(u8, dims, flat, precision=prec)
        seen[value] = names(c)
    on, off = seen[True], seen[False]
    assert seen[None] == off and torch.equal(out[None], out[False])                      # unset: the module value, off
    assert off.count("attention_varlen_fwd") == L and not [s for s in off if s.startswith((TILED % t, ROW % t))], off
    assert on.count(TILED % t) == L - 1 and on.count(ROW % t) == 1 and not F32_SITES & set(on), on
    casts = f"cast_f32_{t}"
    assert off.count(casts) - on.count(casts) == L, (off.count(casts), on.count(casts))
    assert len(off) - len(on) == L
    # the module value alone switches it on too
    monkeypatch.setattr(engine, "_PACKED_ATTN16", True)
    with switched(clip, None), Census(monkeypatch) as c:
        by_env = clip.get_image_features_crops(u8, dims, flat, precision=prec)
    assert names(c) == on and torch.equal(by_env, out[True])
    # fp32: the switch changes nothing, bit for bit
    with Census(monkeypatch) as c32_off:
        with switched(clip, False):
            f_off = clip.get_image_features_crops(u8, dims, flat)
    with Census(monkeypatch) as c32_on:
        with switched(clip, True):
            f_on = clip.get_image_features_crops(u8, dims, flat)
    assert torch.equal(f_on, f_off) and c32_on.names == c32_off.names


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_text_launch_lists(dev, tiny, monkeypatch, prec):
    from dclip_amd import engine
    cfg, m, _ = tiny
    L, t = cfg.text.num_hidden_layers, SHORT[prec]
    ids = synth.synth_input_ids(5, cfg.text, seed=6, ragged=True, min_len=4)
    monkeypatch.setattr(engine, "_PACKED_ATTN16", False)
    calls = {"features": lambda p: m.get_text_features(input_ids=ids, packed_lens=True, precision=p),
             "token_level": lambda p: m.text_token_level_packed(ids, precision=p)[1]}
    want_on = {"features": (L - 1, 1), "token_level": (L, 0)}                             # (tiled causal entry, row entry)
    casts = f"cast_f32_{t}"
    with torch.no_grad():
        for what, call in calls.items():
            seen, out = {}, {}
            for value in (None, False, True):
                with switched(m, value), Census(monkeypatch) as c:
                    out[value] = call(prec)
                seen[value] = names(c)
            on, off = seen[True], seen[False]
            assert seen[None] == off and torch.equal(out[None], out[False]), what
            assert off.count("attention_varlen_causal_fwd") == L, (what, off)
            assert not [s for s in off if s.startswith((TILED % t, ROW % t))], (what, off)
            assert (on.count(TILED % t), on.count(ROW % t)) == want_on[what] and not F32_SITES & set(on), (what, on)
            assert off.count(casts) - on.count(casts) == L and len(off) - len(on) == L, (what, off, on)
            # fp32 (for the pooled forward: the split-fp16 plan, built by a first call): the switch changes nothing, bit for bit
            call("fp32")
            with switched(m, False), Census(monkeypatch) as c_off:
                a = call("fp32")
            with switched(m, True), Census(monkeypatch) as c_on:
                b = call("fp32")
            assert torch.equal(a, b) and c_on.names == c_off.names, what


# ------------------------------------------------------------------------------------------------ (e) a long crop

def test_a_crop_above_512_tokens_takes_the_fp32_cls_route_in_the_last_layer(dev, tiny, monkeypatch):
    """24 x 23 patches + CLS = 553 tokens among short crops: the full layers run the 16-bit tiled entry, the last layer the
    fp32 CLS route (the fall-back vision_fwd_bf16 has above 512 tokens); the result stays within the frozen-tower gate."""
    cfg, clip, teacher = tiny
    L, p = cfg.vision.num_hidden_layers, cfg.vision.patch_size
    u8, dims = teacher.patch_tokenizer._upload_u8([photo(24 * p + 8, 23 * p + 5, 0), photo(80, 96, 1)])
    flat = [(1, 0, 0, 48, 32), (0, 0, 0, 23 * p, 24 * p), (1, 10, 20, 90, 70), (0, 8, 8, 24, 24)]
    f32 = clip.get_image_features_crops(u8, dims, flat)
    with switched(clip, True), Census(monkeypatch) as c:
        x = clip.get_image_features_crops(u8, dims, flat, precision="bf16")
    seen = names(c)
    assert seen.count("attention_varlen_fwd") == 1 and seen.count(TILED % "bf16") == L - 1 and seen.count(ROW % "bf16") == 0, seen
    assert seen.index("attention_varlen_fwd") > max(i for i, s in enumerate(seen) if s == TILED % "bf16")
    err, cos = figures(x, f32)
    print(f"a 553-token crop among short ones, packed bf16 + 16-bit core against packed fp32: {err:.3e} / cosine {cos:.7f}")
    assert bool(torch.isfinite(x).all()) and err < GATE[0] and cos > GATE[1], (err, cos)


# ------------------------------------------------------------------------------------------------ (f) the teacher

def _bf16_teacher(cfg, dev, **kw):
    from dclip_amd.patch_text_aggregation import PatchTextAggregation
    clip = from_hf_state_dict(cfg, synth.synth_clip_state_dict(cfg, seed=7, gain=4.0), device=dev)
    clip.requires_grad_(False)
    teacher = PatchTextAggregation(embed_dim=cfg.projection_dim, num_heads=1, clip_model=clip, tower_precision="bf16",
                                   full_resolution_packed=True, packed_text=True, **kw).to(dev)
    cm = synth.synth_cross_modal_state_dict(cfg.projection_dim, seed=31)
    teacher.load_state_dict({f"cross_modal_attention.{k}": v for k, v in cm.items()})
    return teacher


def test_the_teacher_with_the_switch_on_against_off(dev, tmp_path, monkeypatch):
    cfg = dcfg.tiny()
    paths = []
    for b in range(2):
        paths.append(str(tmp_path / f"{b}.png"))
        photo(80, 96, b).save(paths[-1])
    boxes = [BOXES, BOXES[:2]]
    ids = synth.synth_input_ids(2, cfg.text, seed=9, ragged=True, min_len=4)
    res = {}
    for value in (False, True):
        teacher = _bf16_teacher(cfg, dev, packed_attention16=value)
        assert teacher._clip.packed_attention16 is value
        teacher.text_tokenizer._ids = lambda texts, keep_host=False: ids if keep_host else ids.to(dev)   # no BPE vocab offline
        teacher.full_resolution = True
        with torch.no_grad(), Census(monkeypatch) as c:
            res[value] = (teacher.compute_global_embedding_batch(paths, ["a", "b"], boxes), names(c))
    (off, off_names), (on, on_names) = res[False], res[True]
    Lv, Lt = cfg.vision.num_hidden_layers, cfg.text.num_hidden_layers
    # both towers: the vision tower's L - 1 full layers and its CLS row, the token-level text pass's L causal layers
    assert on_names.count(TILED % "bf16") == Lv - 1 + Lt and on_names.count(ROW % "bf16") == 1, on_names
    assert not F32_SITES & set(on_names) and not [s for s in off_names if s.startswith((TILED % "bf16", ROW % "bf16"))]
    assert off_names.count("attention_varlen_fwd") == Lv and off_names.count("attention_varlen_causal_fwd") == Lt
    err, cos = figures(on, off)
    print(f"teacher target, 16-bit packed core on against off (bf16 towers): {err:.3e} / cosine {cos:.7f}")
    assert on.shape == (2, cfg.projection_dim) and bool(torch.isfinite(on).all()) and err < GATE[0] and cos > GATE[1], (err, cos)


def test_a_prefetched_teacher_gives_the_bits_of_the_direct_call(dev, monkeypatch):
    from dclip_amd.CLIP_image_distillation import CLIPImageDistillation
    cfg = dcfg.tiny()
    B, R = 4, 3
    hp = argparse.Namespace(learning_rate=1e-4, warmup_steps=0, total_steps=100, train_batch_size=B, eval_batch_size=B)
    student = from_hf_state_dict(cfg, synth.synth_clip_state_dict(cfg, seed=0, gain=2.0), device=dev)
    teacher = _bf16_teacher(cfg, dev)
    assert teacher._clip.packed_attention16 is None
    mod = CLIPImageDistillation(hp, student, None, teacher=teacher, freeze_mode="north_star", packed_text=True,
                                packed_attention16=True).to(dev)
    assert mod.student.packed_attention16 is True and mod.teacher._clip.packed_attention16 is True
    ids = synth.synth_input_ids(B, cfg.text, seed=13, ragged=True)
    batch = {"pixel_values": synth.synth_pixel_values(B, cfg.vision, seed=11), "input_ids": ids,
             "regions": synth.synth_regions(B, R, cfg.vision, seed=12), "region_counts": torch.tensor([3, 1, 0, 2])}
    lens = packed_text_tables(ids, cfg.text.eos_token_id)["lens"]
    with torch.no_grad():
        direct = mod.teacher.compute_global_embedding_tensors(batch["regions"].to(dev), ids.to(dev), batch["region_counts"],
                                                              text_lens=lens).float().clone()
        sentence = mod.teacher.last_sentence_embedding.clone()
    with Census(monkeypatch) as c:
        assert mod.prefetch_teacher(batch) is True
    torch.cuda.synchronize()
    assert names(c).count(TILED % "bf16") == cfg.text.num_hidden_layers and "attention_varlen_causal_fwd" not in names(c)
    assert torch.equal(mod._prefetched[1], direct) and torch.equal(mod._prefetched[2], sentence)
    loss = mod.training_step(batch)
    torch.cuda.synchronize()
    assert mod._prefetched is None and bool(torch.isfinite(loss))
