"""The vision tower at another input size: get_image_features(..., interpolate_pos_encoding=True) through every
precision, forward and backward, against (a) a model of that size whose position table is the resampled one — bit-equal —
and (b) HF transformers' CLIPModel with the same flag (tests/golden/vision_interp*.npz, tools/make_vision_interp_golden.py);
the frozen 16-bit towers against the fp32 one; the teacher's full-resolution crops; the evaluation scripts' --image_size."""
import json

import numpy as np
import pytest
import torch

from dclip_amd import config as dcfg, ops, synth
from dclip_amd.clip_model import from_hf_state_dict

pytestmark = pytest.mark.gpu

POS_KEY = "vision_model.embeddings.position_embedding.weight"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def relerr(got, want):
    got = got.detach().double().cpu()
    want = want.detach().cpu().double() if isinstance(want, torch.Tensor) else torch.as_tensor(np.asarray(want)).double()
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))


def cosine(got, want):
    got, want = got.detach().double().cpu().reshape(-1), torch.as_tensor(np.asarray(want)).double().reshape(-1)
    return float(got @ want / (got.norm() * want.norm()))


def with_image_size(cfg: dcfg.ClipConfig, size: int) -> dcfg.ClipConfig:
    import dataclasses
    return dataclasses.replace(cfg, vision=dataclasses.replace(cfg.vision, image_size=size))


def model_pair(cfg, sd, size: int, dev):
    """(A, B): A has the configuration's image size; B the same weights, image_size = `size` and as its position table A's,
    resampled by the kernel under test."""
    a = from_hf_state_dict(cfg, sd, device=dev)
    g, gb = cfg.vision.grid, size // cfg.vision.patch_size
    sdb = {k: v.clone() for k, v in a.state_dict().items()}
    sdb[POS_KEY] = ops.pos_interp_fwd(a.vision_model.embeddings.position_embedding.weight.detach(), g, gb, gb)
    return a, from_hf_state_dict(with_image_size(cfg, size), sdb, device=dev), (g, gb)


def pixels(batch, h, w, dev, seed=0):
    return torch.randn((batch, 3, h, w), generator=torch.Generator().manual_seed(seed)).to(dev)


def vision_grads(m):
    return {k: p.grad for k, p in m.named_parameters() if p.grad is not None}


def assert_grads_match(a, b, g, gb, what):
    ga, gb_ = vision_grads(a), vision_grads(b)
    assert set(ga) == set(gb_) and POS_KEY in ga and len(ga) > 20, what
    for k in ga:
        if k != POS_KEY:
            assert torch.equal(ga[k], gb_[k]), (what, k)
    assert torch.equal(ga[POS_KEY], ops.pos_interp_bwd(gb_[POS_KEY].contiguous(), g, gb, gb)), (what, "position table")
    assert bool(torch.isfinite(ga[POS_KEY]).all()) and float(ga[POS_KEY].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ plumbing, bit-equal

@pytest.mark.parametrize("size", [96, 32])
def test_flagged_call_equals_a_model_of_that_size_with_the_resampled_table(dev, size):
    cfg = dcfg.tiny()
    a, b, (g, gb) = model_pair(cfg, synth.synth_clip_state_dict(cfg, seed=7, gain=4.0), size, dev)
    pix = pixels(3, size, size, dev)
    r = synth.synth_embeddings(3, cfg.projection_dim, seed=11).to(dev)
    with torch.no_grad():
        for prec in ("fp32", "bf16", "fp16"):
            got = a.get_image_features(pixel_values=pix, precision=prec, interpolate_pos_encoding=True)
            assert got.shape == (3, cfg.projection_dim) and bool(torch.isfinite(got).all())
            assert torch.equal(got, b.get_image_features(pixel_values=pix, precision=prec)), prec
        ha = a.hidden_states(pixel_values=pix, interpolate_pos_encoding=True)
        hb = b.hidden_states(pixel_values=pix)
        assert ha[0].shape == (3, 1 + gb * gb, cfg.vision.hidden_size)
        assert all(torch.equal(x, y) for x, y in zip(ha, hb))
    for prec in ("fp32", "bf16", "fp16-mixed"):
        a.zero_grad(set_to_none=True)
        b.zero_grad(set_to_none=True)
        oa = a.get_image_features(pixel_values=pix, precision=prec, interpolate_pos_encoding=True)
        ob = b.get_image_features(pixel_values=pix, precision=prec)
        assert torch.equal(oa, ob), prec
        (oa * r).sum().backward()
        (ob * r).sum().backward()
        assert_grads_match(a, b, g, gb, f"{size} {prec}")


def test_16_bit_training_above_64_tokens_takes_the_fp32_attention_core_under_a_grid(dev, monkeypatch):
    """144 x 144 on the tiny tower is a 9 x 9 grid, 82 tokens: above the 64 that the 16-bit attention pairs of the training
    path take (engine._attention_io16), so both 16-bit precisions run the fp32 attention core with casts.  The launch names
    show that routing; the result is bit-equal to a 144-px model holding the resampled table, as at the shorter lengths."""
    from dclip_amd import _lib
    cfg = dcfg.tiny()
    a, b, (g, gb) = model_pair(cfg, synth.synth_clip_state_dict(cfg, seed=7, gain=4.0), 144, dev)
    assert (g, gb) == (4, 9)
    pix = pixels(3, 144, 144, dev)
    r = synth.synth_embeddings(3, cfg.projection_dim, seed=11).to(dev)
    lib, check = _lib.load(), _lib.check
    for prec in ("bf16", "fp16-mixed"):
        a.zero_grad(set_to_none=True)
        b.zero_grad(set_to_none=True)
        seen = set()

        def census(rc, what=""):
            seen.add(lib.dclip_last_launch().decode())
            return check(rc, what)

        monkeypatch.setattr(_lib, "check", census)
        oa = a.get_image_features(pixel_values=pix, precision=prec, interpolate_pos_encoding=True)
        (oa * r).sum().backward()
        torch.cuda.synchronize()
        monkeypatch.setattr(_lib, "check", check)
        attn = sorted(n for n in seen if n.startswith("attention_"))
        assert any(n.split(".")[0] == "attention_fwd" for n in attn), (prec, attn)
        assert any(n.split(".")[0] == "attention_bwd" for n in attn), (prec, attn)
        assert not [n for n in attn if "16" in n], (prec, attn)
        assert {"pos_interp_fwd", "pos_interp_bwd"} <= seen, (prec, sorted(seen))
        ob = b.get_image_features(pixel_values=pix, precision=prec)
        assert torch.equal(oa, ob), prec
        (ob * r).sum().backward()
        assert_grads_match(a, b, g, gb, f"144 {prec}")


def test_the_flag_changes_nothing_at_the_models_own_size_and_the_size_check_stays(dev):
    cfg = dcfg.tiny()
    m = from_hf_state_dict(cfg, synth.synth_clip_state_dict(cfg, seed=7, gain=4.0), device=dev)
    pix = pixels(2, 64, 64, dev)
    with torch.no_grad():
        for prec in ("fp32", "bf16", "fp16"):
            assert torch.equal(m.get_image_features(pixel_values=pix, precision=prec, interpolate_pos_encoding=True),
                               m.get_image_features(pixel_values=pix, precision=prec))
        with pytest.raises(ValueError, match="doesn't match model"):
            m.get_image_features(pixel_values=pixels(2, 96, 96, dev))
        with pytest.raises(ValueError, match="doesn't match model"):
            m.get_image_features(pixel_values=pixels(2, 96, 96, dev), interpolate_pos_encoding=False)
        with pytest.raises(ValueError, match="smaller than one patch"):
            m.get_image_features(pixel_values=pixels(2, 64, 10, dev), interpolate_pos_encoding=True)
        # 70 x 70 makes the model's own 4 x 4 grid: the identity resample, trailing pixels ignored
        big = pixels(2, 70, 70, dev, seed=3)
        assert torch.equal(m.get_image_features(pixel_values=big, interpolate_pos_encoding=True),
                           m.get_image_features(pixel_values=big[:, :, :64, :64].contiguous()))


def test_two_backwards_accumulate_into_the_position_gradient(dev):
    cfg = dcfg.tiny()
    m = from_hf_state_dict(cfg, synth.synth_clip_state_dict(cfg, seed=7, gain=4.0), device=dev)
    pos = m.vision_model.embeddings.position_embedding.weight
    r = synth.synth_embeddings(2, cfg.projection_dim, seed=11).to(dev)
    batches = [pixels(2, 96, 96, dev, seed=1), pixels(2, 64, 112, dev, seed=2)]
    single = []
    for pix in batches:
        m.zero_grad(set_to_none=True)
        (m.get_image_features(pixel_values=pix, interpolate_pos_encoding=True) * r).sum().backward()
        single.append(pos.grad.clone())
    m.zero_grad(set_to_none=True)
    for pix in batches:                                   # accumulate_grad_batches = 2: no zero_grad in between
        (m.get_image_features(pixel_values=pix, interpolate_pos_encoding=True) * r).sum().backward()
    assert pos.grad.shape == pos.shape and torch.equal(pos.grad, single[0] + single[1])
    assert not torch.equal(single[0], single[1])


# ------------------------------------------------------------------------------------------------ parity with HF

GRAD_KEYS = ["vision_model.embeddings.position_embedding.weight", "vision_model.embeddings.class_embedding",
             "vision_model.embeddings.patch_embedding.weight", "vision_model.encoder.layers.0.self_attn.q_proj.weight",
             "vision_model.encoder.layers.0.self_attn.k_proj.weight", "vision_model.encoder.layers.0.self_attn.v_proj.weight",
             "visual_projection.weight"]


def test_parity_with_hf_interpolate_pos_encoding(dev, golden):
    """Embeddings within 1e-3 (norm-wise) and gradient cosine >= 0.9999 for each of the seven tensors at each of the four
    sizes, 28 pairs: the project's gates.  Measured on an MI355X: embedding error 4.7e-6, 3.8e-6, 1.4e-6, 2.0e-6
    at 96 x 96, 64 x 112, 80 x 50, 64 x 64; worst cosine over the seven tensors 1.00000000 at each size."""
    common = golden("vision_interp.npz")
    cfg = dcfg.tiny()
    m = from_hf_state_dict(cfg, synth.synth_clip_state_dict(cfg, seed=7, gain=4.0), device=dev)
    r = torch.from_numpy(common["r"]).to(dev)
    D = cfg.vision.hidden_size
    for h, w in common["sizes"].tolist():
        g = golden(f"vision_interp_{h}x{w}.npz")
        pix = (torch.from_numpy(g["pixel_q"]).float() / 16.0).to(dev)
        m.zero_grad(set_to_none=True)
        out = m.get_image_features(pixel_values=pix, interpolate_pos_encoding=True)
        (out * r).sum().backward()
        err = relerr(out, g["image_emb"])
        grads = {}
        for k, p in m.named_parameters():
            if p.grad is None:                           # the text tower
                continue
            if "layers.0.self_attn.qkv_proj.weight" in k:
                for i, n in enumerate(("q_proj", "k_proj", "v_proj")):
                    grads[k.replace("qkv_proj", n)] = p.grad[i * D:(i + 1) * D]
            else:
                grads[k] = p.grad
        cos = {k: cosine(grads[k], g[f"grad.{k}"]) for k in GRAD_KEYS}
        print(f"{h}x{w}: embedding relerr {err:.3e}, worst gradient cosine {min(cos.values()):.8f} over {len(cos)} tensors")
        assert err <= 1e-3, (h, w, err)
        for k, c in cos.items():
            assert c >= 0.9999, (h, w, k, c)


# ------------------------------------------------------------------------------------------------ 16-bit frozen towers

@pytest.mark.parametrize("hw", [(96, 96), (64, 112)], ids=["96x96", "64x112"])
def test_frozen_16_bit_towers_against_the_fp32_interpolated_result(dev, hw):
    """The gates of the frozen-tower tests at the native size: bf16 rel < 3e-2 and cosine > 0.999 (tests/test_bf16_gpu.py,
    test_frozen_vision_tower_bf16_error, which runs the tiny tower); fp16 rel < 1e-3 and cosine > 0.99999
    (tests/test_fp16_gpu.py, test_frozen_towers_f16_meet_the_bar).  Weights and input range are those tests'.
    Measured on an MI355X: bf16 7.4e-3 / 0.999974 at 96 x 96 and 6.7e-3 / 0.999967 at 64 x 112; fp16 7.0e-4 / 0.9999997 and
    7.8e-4 / 0.9999995."""
    cfg = dcfg.tiny()
    m = from_hf_state_dict(cfg, synth.synth_clip_state_dict(cfg, seed=0, gain=3.0), device=dev)
    pix = torch.rand((4, 3, *hw), generator=torch.Generator().manual_seed(2)).to(dev)
    with torch.no_grad():
        f32 = m.get_image_features(pixel_values=pix, interpolate_pos_encoding=True)
        res = {p: m.get_image_features(pixel_values=pix, precision=p, interpolate_pos_encoding=True) for p in ("bf16", "fp16")}
        again = m.get_image_features(pixel_values=pix, precision="bf16", interpolate_pos_encoding=True)
    assert torch.equal(again, res["bf16"])
    fig = {}
    for p, x in res.items():
        fig[p] = (float((x - f32).abs().max() / f32.abs().max()),
                  float(torch.nn.functional.cosine_similarity(x, f32, dim=1).min()))
        print(f"tiny at {hw[0]}x{hw[1]}: {p} tower max rel err {fig[p][0]:.2e}, min cosine {fig[p][1]:.7f}")
    assert fig["bf16"][0] < 3e-2 and fig["bf16"][1] > 0.999
    assert fig["fp16"][0] < 1e-3 and fig["fp16"][1] > 0.99999


# ------------------------------------------------------------------------------------------------ one real shape

def test_vit_b32_at_336_and_at_224_by_320(dev):
    """ViT-B/32 weights (random init) at 336 x 336: 10 x 10 whole patches + the class token = 101 tokens, the long-sequence
    attention paths at a length no CLIP configuration has; the last 16 rows and columns belong to no patch.  The result equals
    a 320-px model with the resampled table on the first 320 x 320 pixels, forward and backward.  224 x 320 (71 tokens; a
    configuration is square, so there is no such model to compare with) runs and stays finite."""
    cfg = dcfg.vit_b32()
    a, b, (g, gb) = model_pair(cfg, synth.synth_clip_state_dict(cfg, seed=0, gain=3.0), 320, dev)
    for m in (a, b):
        for p in list(m.text_model.parameters()) + [m.text_projection.weight, m.logit_scale]:
            p.requires_grad_(False)
    r = synth.synth_embeddings(2, cfg.projection_dim, seed=11).to(dev)
    pix = pixels(2, 336, 336, dev)
    oa = a.get_image_features(pixel_values=pix, interpolate_pos_encoding=True)
    ob = b.get_image_features(pixel_values=pix[:, :, :320, :320].contiguous())
    assert (g, gb) == (7, 10) and torch.equal(oa, ob) and bool(torch.isfinite(oa).all())
    (oa * r).sum().backward()
    (ob * r).sum().backward()
    assert_grads_match(a, b, g, gb, "ViT-B/32 at 336")
    del b
    a.zero_grad(set_to_none=True)
    out = a.get_image_features(pixel_values=pixels(2, 224, 320, dev, seed=5), interpolate_pos_encoding=True)
    (out * r).sum().backward()
    assert bool(torch.isfinite(out).all())
    for k, gr in vision_grads(a).items():
        assert bool(torch.isfinite(gr).all()), k
    assert a.vision_model.embeddings.position_embedding.weight.grad.shape == (50, 768)


# ------------------------------------------------------------------------------------------------ the teacher

def _teacher(dev):
    from dclip_amd.patch_text_aggregation import PatchTextAggregation
    cfg = dcfg.tiny()
    clip = from_hf_state_dict(cfg, synth.synth_clip_state_dict(cfg, seed=7, gain=4.0), device=dev)
    return cfg, clip, PatchTextAggregation(embed_dim=cfg.projection_dim, num_heads=1, clip_model=clip).to(dev)


def _photo(h, w, seed):
    from PIL import Image
    return Image.fromarray(np.random.default_rng(seed).integers(0, 255, (h, w, 3), dtype=np.uint8))


BOXES = [((0, 0, 48, 32), 0.9), ((10, 20, 90, 70), 0.8), ((40, 8, 88, 40), 0.7)]       # crops 32x48, 50x80, 32x48 (h x w)


def test_full_resolution_boxes_equal_per_crop_calls_in_box_order(dev):
    cfg, clip, teacher = _teacher(dev)
    tok = teacher.patch_tokenizer
    image = _photo(80, 96, 0)
    got = tok.encode_weighted_bounding_boxes(image, BOXES, full_resolution=True)
    assert [c for _, c in got] == [0.9, 0.8, 0.7]
    for (e, _), (box, _) in zip(got, BOXES):
        crop = tok.full_resolution_transform(image.crop(box)).unsqueeze(0).to(dev)
        assert crop.shape[2:] == (box[3] - box[1], box[2] - box[0]) and float(crop.max()) <= 1.0
        with torch.no_grad():
            want = clip.get_image_features(pixel_values=crop, interpolate_pos_encoding=True)[0]
        assert torch.equal(e, want), box
    assert not torch.equal(got[0][0], got[2][0])
    with pytest.raises(ValueError, match="smaller than one patch"):
        tok.encode_weighted_bounding_boxes(image, BOXES[:1] + [((5, 5, 15, 60), 0.5)], full_resolution=True)
    assert tok.encode_weighted_bounding_boxes(image, [], full_resolution=True) == []


def test_full_resolution_teacher_batch_and_the_zero_row(dev, tmp_path):
    cfg, clip, teacher = _teacher(dev)
    paths = []
    for b in range(2):
        paths.append(str(tmp_path / f"{b}.png"))
        _photo(80, 96, b).save(paths[-1])
    boxes = [BOXES, BOXES[:2] + [((5, 5, 15, 60), 0.5)]]           # the second image has a box 10 px wide
    ids = synth.synth_input_ids(2, cfg.text, seed=9, ragged=True, min_len=4)
    teacher.text_tokenizer._ids = lambda texts, keep_host=False: ids if keep_host else ids.to(dev)   # no BPE vocab offline
    teacher.full_resolution = True
    with torch.no_grad():
        got = teacher.compute_global_embedding_batch(paths, ["a", "b"], boxes)
        from PIL import Image
        first = teacher.patch_tokenizer.encode_weighted_bounding_boxes(Image.open(paths[0]).convert("RGB"), BOXES, True)
        emb = torch.zeros((2, 3, cfg.projection_dim), device=dev)
        emb[0] = torch.stack([e for e, _ in first])              # image 1 keeps the single zero row
        sent, tokens, eos = teacher.text_tokenizer.token_level_ids(ids.to(dev))
        text = ops.pack_tokens(tokens.contiguous(), sent, eos, max(int(eos.max()) - 1, 1))
        want = teacher.global_embedding_from_tokens(text, emb)
    assert got.shape == (2, cfg.projection_dim) and bool(torch.isfinite(got).all())
    assert torch.equal(got, want)


def test_without_full_resolution_the_teacher_launches_nothing_new(dev, tmp_path, monkeypatch):
    from dclip_amd import _lib
    cfg, clip, teacher = _teacher(dev)
    paths = []
    for b in range(2):
        paths.append(str(tmp_path / f"{b}.png"))
        _photo(80, 96, b).save(paths[-1])
    boxes = [BOXES, BOXES[:2]]
    ids = synth.synth_input_ids(2, cfg.text, seed=9, ragged=True, min_len=4)
    teacher.text_tokenizer._ids = lambda texts, keep_host=False: ids if keep_host else ids.to(dev)
    assert teacher.full_resolution is False
    lib, check, seen = _lib.load(), _lib.check, set()

    def census(rc, what=""):
        seen.add(lib.dclip_last_launch().decode())
        return check(rc, what)

    monkeypatch.setenv("DCLIP_TEACHER_TEXT_STREAM", "0")          # one stream, one thread: every launch is seen in order
    monkeypatch.setattr(_lib, "check", census)
    with torch.no_grad():
        got = teacher.compute_global_embedding_batch(paths, ["a", "b"], boxes)
    monkeypatch.setattr(_lib, "check", check)
    assert any(n.startswith("im2col") for n in seen) and "vision_assemble_fwd" in seen
    assert not [n for n in seen if n.startswith(("pos_interp", "im2col_rect"))], sorted(seen)
    with torch.no_grad():
        from PIL import Image
        regions, counts = teacher.patch_tokenizer.crop_boxes_gpu([Image.open(p).convert("RGB") for p in paths], boxes)
        want = teacher.compute_global_embedding_tensors(regions, ids.to(dev), counts)
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------ evaluation scripts

def _toy_ids(cfg, texts):
    T = cfg.text.max_position_embeddings
    ids = torch.full((len(texts), T), cfg.text.eos_token_id, dtype=torch.int64)
    ids[:, 0] = cfg.text.bos_token_id
    for b, c in enumerate(texts):
        for j, w in enumerate(c.replace(",", " ").split()[:T - 2]):
            ids[b, 1 + j] = 1 + (sum(ord(ch) * (q + 1) for q, ch in enumerate(w)) % (cfg.text.bos_token_id - 2))
    return ids


def test_flickr_eval_at_another_image_size(dev, tmp_path):
    from PIL import Image
    from dclip_amd import data, flickr30k_eval as F
    cfg = dcfg.tiny(image_size=64, patch_size=16)
    clip = from_hf_state_dict(cfg, synth.synth_clip_state_dict(cfg, seed=3, gain=3.0), device=dev)
    recs = []
    for i in range(7):
        p = tmp_path / f"im{i}.png"
        Image.fromarray(synth.synth_photo(110 + 7 * i, 130 + 3 * i, seed=i)).save(p)
        recs.append({"image_id": f"id{i}", "image_path": str(p), "captions": [f"w{i} a{j} photo" for j in range(1 + i % 3)]})
    (tmp_path / "test.json").write_text(json.dumps(recs))
    tokenizer = lambda caps: _toy_ids(cfg, caps)                  # noqa: E731
    assert F.build_parser().parse_args(["--dataset_json", "x", "--clip_path", "y", "--image_size", "96"]).image_size == 96
    m = F.evaluate_model("base", dev, max_images=100, dataset_json=str(tmp_path / "test.json"), clip_model=clip,
                         tokenizer=tokenizer, batch_size=3, image_size=96)
    pre = data.ClipImagePreprocess(96)
    with torch.no_grad():
        img = torch.cat([clip.get_image_features(pixel_values=pre(images=Image.open(r["image_path"]))["pixel_values"].to(dev),
                                                 interpolate_pos_encoding=True) for r in recs])
        caps = [c for r in recs for c in r["captions"]]
        cap = clip.get_text_features(input_ids=tokenizer(caps).to(dev))
    assert img.shape[0] == 7
    owner = [i for i, r in enumerate(recs) for _ in r["captions"]]
    sim = torch.nn.functional.normalize(cap.double(), dim=1) @ torch.nn.functional.normalize(img.double(), dim=1).t()
    rank = [(sim[c] > sim[c, owner[c]]).sum().item() for c in range(len(caps))]
    assert abs(m["t2i"]["R@1"] - np.mean([r < 1 for r in rank])) < 1e-12
    assert abs(m["t2i"]["MAP"] - np.mean([1.0 / (r + 1) for r in rank])) < 1e-9


def test_zero_shot_eval_at_another_image_size(dev, tmp_path):
    from PIL import Image
    from dclip_amd import zero_shot_eval as Z
    cfg = dcfg.tiny(image_size=64, patch_size=16)
    clip = from_hf_state_dict(cfg, synth.synth_clip_state_dict(cfg, seed=3, gain=3.0), device=dev)
    names = ["cat", "dog", "tree", "car", "bird", "boat", "cup"]
    k = 0
    for c in names:
        (tmp_path / "val" / c).mkdir(parents=True)
        for j in range(2):
            Image.fromarray(synth.synth_photo(100 + 5 * k, 120 + 3 * k, seed=k)).save(tmp_path / "val" / c / f"{j}.png")
            k += 1
    processor = lambda text=None, return_tensors="pt", padding=True: {"input_ids": _toy_ids(cfg, text)}      # noqa: E731
    res = Z.main(["--data_root", str(tmp_path / "val"), "--batch_size", "4", "--image_size", "96", "--results",
                  str(tmp_path / "r.txt")], clip_model=clip, processor=processor)
    ds = Z.ImageFolderDataset(str(tmp_path / "val"), 96)
    x = torch.stack([ds[i][0] for i in range(len(ds))]).to(dev)
    y = torch.tensor([ds[i][1] for i in range(len(ds))])
    assert x.shape[1:] == (3, 96, 96)
    mean = torch.tensor(Z.E.CLIP_MEAN, device=dev).view(1, 3, 1, 1)
    std = torch.tensor(Z.E.CLIP_STD, device=dev).view(1, 3, 1, 1)
    with torch.no_grad():
        img = clip.get_image_features(pixel_values=(x - mean) / std, interpolate_pos_encoding=True).double().cpu()
        txt = clip.get_text_features(input_ids=_toy_ids(cfg, [f"a photo of a {n}" for n in sorted(names)]).to(dev)).double().cpu()
    sim = 100.0 * torch.nn.functional.normalize(img, dim=1) @ torch.nn.functional.normalize(txt, dim=1).t()
    top5 = sim.topk(5, dim=1).indices
    assert abs(res["base"]["top1"] - float((top5[:, 0] == y).double().mean())) < 1e-12
    assert abs(res["base"]["top5"] - float((top5 == y[:, None]).any(1).double().mean())) < 1e-12
