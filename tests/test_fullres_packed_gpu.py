"""The full-resolution teacher in one packed pass: HipCLIPModel.get_image_features_crops against per-crop
get_image_features(interpolate_pos_encoding=True) on Pillow crops, the 16-bit packed towers against the fp32 one, isolation of
the crops inside a pack, the launch count (one schedule whatever the number of crops), the teacher with
`full_resolution_packed` against the per-crop teacher, and the flags that switch it on."""
import argparse

import numpy as np
import pytest
import torch

from dclip_amd import _lib, config as dcfg, synth
from dclip_amd.clip_model import from_hf_state_dict
from tests.test_vision_interp_gpu import BOXES

pytestmark = pytest.mark.gpu

# BOXES of tests/test_vision_interp_gpu.py (crops 32x48, 50x80, 32x48), one patch, and the model's own 64 x 64
CROP_BOXES = BOXES + [((8, 8, 24, 24), 0.6), ((16, 8, 80, 72), 0.5)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def setup(dev):
    from dclip_amd.patch_text_aggregation import PatchTextAggregation
    cfg = dcfg.tiny()
    clip = from_hf_state_dict(cfg, synth.synth_clip_state_dict(cfg, seed=7, gain=4.0), device=dev)
    teacher = PatchTextAggregation(embed_dim=cfg.projection_dim, num_heads=1, clip_model=clip).to(dev)
    return cfg, clip, teacher


def photo(h, w, seed):
    from PIL import Image
    return Image.fromarray(np.random.default_rng(seed).integers(0, 255, (h, w, 3), dtype=np.uint8))


def figures(got, want):
    """(max |got - want| / max |want|, smallest row cosine)"""
    got, want = got.double().cpu(), want.double().cpu()
    return (float((got - want).abs().max() / want.abs().max()),
            float(torch.nn.functional.cosine_similarity(got, want, dim=1).min()))


def flat_boxes(per_image):
    return [(b, *box) for b, boxes in enumerate(per_image) for box, _ in boxes]


class Census:
    """Every launch site the library reports while it is active, in order."""

    def __init__(self, monkeypatch):
        self.names, self._mp, self._check = [], monkeypatch, _lib.check
        lib = _lib.load()

        def census(rc, what=""):
            self.names.append(lib.dclip_last_launch().decode())
            return self._check(rc, what)
        self._census = census

    def __enter__(self):
        self._mp.setattr(_lib, "check", self._census)
        return self

    def __exit__(self, *exc):
        self._mp.setattr(_lib, "check", self._check)
        return False


@pytest.fixture(scope="module")
def packed_reference(dev, setup):
    """Two 80 x 96 photos, CROP_BOXES on each: (images, uploaded batch, dims, flat boxes, the fp32 packed result)."""
    cfg, clip, teacher = setup
    images = [photo(80, 96, b) for b in range(2)]
    u8, dims = teacher.patch_tokenizer._upload_u8(images)
    flat = flat_boxes([CROP_BOXES, CROP_BOXES])
    out = clip.get_image_features_crops(u8, dims, flat)
    torch.cuda.synchronize()
    return images, u8, dims, flat, out


def test_packed_crops_against_per_crop_calls_fp32(dev, setup, packed_reference):
    """The project's embedding bar (relative error below 1e-3, cosine above 0.99999), as gated against HF in
    tests/test_vision_interp_gpu.py.  The two differ only in the row count of the GEMMs and in the attention kernel.
    Measured on an MI355X: max rel err 3.5e-7, min cosine 1.00000000 over the 10 crops."""
    cfg, clip, teacher = setup
    images, u8, dims, flat, got = packed_reference
    tok = teacher.patch_tokenizer
    assert got.shape == (len(flat), cfg.projection_dim) and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    want = []
    with torch.no_grad():
        for b, x1, y1, x2, y2 in flat:
            crop = tok.full_resolution_transform(images[b].crop((x1, y1, x2, y2))).unsqueeze(0).to(dev)
            want.append(clip.get_image_features(pixel_values=crop, interpolate_pos_encoding=True)[0])
    err, cos = figures(got, torch.stack(want))
    print(f"packed fp32 against per-crop calls over {len(flat)} crops: max rel err {err:.3e}, min cosine {cos:.8f}")
    assert err < 1e-3 and cos > 0.99999, (err, cos)
    assert not torch.equal(got[0], got[2])                  # the same box size at another place is another crop


def test_packed_16_bit_towers_against_the_fp32_packed_result(dev, setup, packed_reference):
    """The gates of the frozen 16-bit towers (tests/test_bf16_gpu.py, tests/test_fp16_gpu.py, tests/test_vision_interp_gpu.py):
    bf16 below 3e-2 with cosine above 0.999; fp16 below 1e-3 with cosine above 0.99999.
    Measured on an MI355X: bf16 7.0e-3 / 0.9999673, fp16 7.8e-4 / 0.9999997."""
    cfg, clip, teacher = setup
    images, u8, dims, flat, f32 = packed_reference
    fig = {}
    for prec in ("bf16", "fp16"):
        x = clip.get_image_features_crops(u8, dims, flat, precision=prec)
        assert x.shape == f32.shape and x.dtype == torch.float32
        fig[prec] = figures(x, f32)
        print(f"packed {prec} against packed fp32: max rel err {fig[prec][0]:.3e}, min cosine {fig[prec][1]:.7f}")
        assert torch.equal(x, clip.get_image_features_crops(u8, dims, flat, precision=prec)), prec
    assert fig["bf16"][0] < 3e-2 and fig["bf16"][1] > 0.999, fig
    assert fig["fp16"][0] < 1e-3 and fig["fp16"][1] > 0.99999, fig


def test_the_entry_is_forward_only_and_refuses_what_it_cannot_run(dev, setup, packed_reference):
    cfg, clip, teacher = setup
    images, u8, dims, flat, f32 = packed_reference
    out = clip.get_image_features_crops(u8, dims, flat[:2])            # grad mode on, trainable parameters: still no graph
    assert not out.requires_grad and out.grad_fn is None and out.shape == (2, cfg.projection_dim)
    assert figures(out, f32[:2])[0] < 1e-3                             # a pack of two against the same crops in a pack of ten
    assert clip.get_image_features_crops(u8, dims, []).shape == (0, cfg.projection_dim)
    with pytest.raises(ValueError, match="smaller than one patch"):
        clip.get_image_features_crops(u8, dims, [(0, 5, 5, 15, 60)])
    with pytest.raises(ValueError, match="outside the batch"):
        clip.get_image_features_crops(u8, dims, [(2, 0, 0, 32, 32)])
    with pytest.raises(ValueError, match="precision"):
        clip.get_image_features_crops(u8, dims, flat[:1], precision="fp16-mixed")


def test_changing_one_crops_pixels_leaves_every_other_embedding_bit_identical(dev, setup):
    cfg, clip, teacher = setup
    images = [photo(80, 96, 0), photo(40, 56, 1), photo(80, 96, 2)]
    per_image = [CROP_BOXES, [((4, 3, 52, 35), 0.9)], CROP_BOXES[:3]]          # the middle image holds ONE crop
    flat = flat_boxes(per_image)
    u8, dims = teacher.patch_tokenizer._upload_u8(images)
    before = clip.get_image_features_crops(u8, dims, flat)
    u8[1, :40, :56] = 255 - u8[1, :40, :56]
    after = clip.get_image_features_crops(u8, dims, flat)
    mid = len(CROP_BOXES)
    assert not torch.equal(before[mid], after[mid])
    keep = [i for i in range(len(flat)) if i != mid]
    assert torch.equal(before[keep], after[keep]) and bool(torch.isfinite(after).all())


def test_packed_means_packed_one_schedule_whatever_the_number_of_crops(dev, setup, monkeypatch):
    cfg, clip, teacher = setup
    images = [photo(80, 96, b) for b in range(2)]
    u8, dims = teacher.patch_tokenizer._upload_u8(images)
    seen = {}
    for n in (3, 7):
        flat = flat_boxes([CROP_BOXES, CROP_BOXES])[:n]
        with Census(monkeypatch) as c:
            clip.get_image_features_crops(u8, dims, flat)
        seen[n] = c.names
    sites = {n: [s.split(".")[0] for s in seen[n]] for n in seen}        # a GEMM's tile variant may follow the row count
    assert len(seen[3]) == len(seen[7]) and sites[3] == sites[7], (seen[3], seen[7])
    names = set(sites[7])
    assert {"attention_varlen_fwd", "patches_from_boxes_u8", "vision_assemble_varlen", "gather_rows_at"} <= names, sorted(names)
    assert not [s for s in names if s.startswith(("im2col_rect", "pos_interp_fwd", "attention_fwd", "attention_cls"))], sorted(names)
    assert sites[7].count("attention_varlen_fwd") == cfg.vision.num_hidden_layers
    print(f"{len(seen[7])} launches for 3 crops and for 7 crops")


# ------------------------------------------------------------------------------------------------ the teacher

def _teacher_batch(cfg, teacher, dev, tmp_path):
    paths = []
    for b in range(2):
        paths.append(str(tmp_path / f"{b}.png"))
        photo(80, 96, b).save(paths[-1])
    boxes = [BOXES, BOXES[:2] + [((5, 5, 15, 60), 0.5)]]           # the second image has a box 10 px wide: it keeps the zero row
    ids = synth.synth_input_ids(2, cfg.text, seed=9, ragged=True, min_len=4)
    teacher.text_tokenizer._ids = lambda texts, keep_host=False: ids if keep_host else ids.to(dev)   # no BPE vocab offline
    return paths, boxes


def test_packed_teacher_against_the_per_crop_teacher(dev, setup, tmp_path, monkeypatch):
    """The embedding bar again (1e-3, cosine 0.99999).  Measured on an MI355X: 2.5e-7 / 1.00000000."""
    from PIL import Image
    cfg, clip, teacher = setup
    paths, boxes = _teacher_batch(cfg, teacher, dev, tmp_path)
    try:
        teacher.full_resolution = True
        with torch.no_grad():
            teacher.full_resolution_packed = False
            with Census(monkeypatch) as per_crop:
                want = teacher.compute_global_embedding_batch(paths, ["a", "b"], boxes)
            teacher.full_resolution_packed = True
            with Census(monkeypatch) as packed:
                got = teacher.compute_global_embedding_batch(paths, ["a", "b"], boxes)
            # with the flag unset the launch set of the existing mode is the parent's: none of the packed entries
            new = {"attention_varlen_fwd", "patches_from_boxes_u8", "vision_assemble_varlen", "gather_rows_at"}
            assert not new & set(per_crop.names), sorted(set(per_crop.names))
            assert {"pos_interp_fwd", "vision_assemble_fwd"} <= set(per_crop.names)
            assert any(n.startswith("im2col_rect") for n in per_crop.names)
            assert new <= set(packed.names) and not [n for n in packed.names if n.startswith(("pos_interp", "im2col"))]
            err, cos = figures(got, want)
            print(f"packed teacher against the per-crop teacher: max rel err {err:.3e}, min cosine {cos:.8f}")
            assert got.shape == (2, cfg.projection_dim) and bool(torch.isfinite(got).all())
            assert err < 1e-3 and cos > 0.99999, (err, cos)
            assert torch.equal(got[1], want[1]), "the zero-row image's target: no crop of it enters either tower"
            # a batch that is already on the device: no pixel returns to the host, Pillow is not touched
            u8, dims = teacher.patch_tokenizer._upload_u8([Image.open(p).convert("RGB") for p in paths])

            def refuse(*a, **k):
                raise AssertionError("the packed teacher touched Pillow")

            monkeypatch.setattr(Image, "fromarray", refuse)
            monkeypatch.setattr(Image, "open", refuse)
            on_device = teacher.compute_global_embedding_batch(paths, ["a", "b"], boxes, images_u8=u8, dims=dims)
            assert torch.equal(on_device, got)
    finally:
        teacher.full_resolution, teacher.full_resolution_packed = False, False


def test_encode_full_resolution_batch_pads_with_zero_rows(dev, setup):
    cfg, clip, teacher = setup
    tok = teacher.patch_tokenizer
    images = [photo(80, 96, 0), photo(80, 96, 1), photo(80, 96, 2)]
    emb, counts = tok.encode_full_resolution_batch(images, [BOXES, [], BOXES[:1]])
    assert emb.shape == (3, 3, cfg.projection_dim) and counts.tolist() == [3, 0, 1]
    assert float(emb[1].abs().max()) == 0.0 and float(emb[2, 1:].abs().max()) == 0.0 and float(emb[2, 0].abs().max()) > 0
    emb0, counts0 = tok.encode_full_resolution_batch(images, [[], [], []])
    assert emb0.shape == (3, 1, cfg.projection_dim) and counts0.tolist() == [0, 0, 0] and float(emb0.abs().max()) == 0.0


def test_knn_with_full_resolution_stays_unimplemented_and_the_default_is_off(dev, setup):
    from dclip_amd.patch_text_aggregation import PatchTextAggregation
    cfg, clip, teacher = setup
    assert teacher.full_resolution is False and teacher.full_resolution_packed is False
    t2 = PatchTextAggregation(embed_dim=cfg.projection_dim, num_heads=1, clip_model=clip, full_resolution_packed=True)
    assert t2.full_resolution_packed is True and t2.full_resolution is False
    t2.full_resolution, t2.use_knn_projection, t2.advanced_tokenizer = True, True, object()
    with pytest.raises(NotImplementedError, match="KNN"):
        t2.compute_global_embedding_batch(["x.png"], ["a"], [BOXES])


def test_full_resolution_from_epoch_flips_both_flags_at_that_epoch_and_not_before(dev, setup):
    from dclip_amd.CLIP_image_distillation import CLIPImageDistillation
    cfg = dcfg.tiny()
    B = 2
    hp = argparse.Namespace(learning_rate=1e-4, warmup_steps=0, total_steps=100, train_batch_size=B, eval_batch_size=B)
    batch = {"pixel_values": synth.synth_pixel_values(B, cfg.vision, seed=1).to(dev),
             "input_ids": synth.synth_input_ids(B, cfg.text, seed=2, ragged=True).to(dev),
             "teacher_image_emb": synth.synth_embeddings(B, cfg.projection_dim, seed=3).to(dev)}

    def module(**kw):
        student = from_hf_state_dict(cfg, synth.synth_clip_state_dict(cfg, seed=0), device=dev)
        return CLIPImageDistillation(hp, student, None, freeze_mode="north_star", **kw).to(dev)

    m = module(full_resolution_from_epoch=2)
    for epoch, want in ((0, False), (1, False), (2, True), (3, True), (1, False)):
        m.current_epoch = epoch
        assert bool(torch.isfinite(m.training_step(batch)))
        assert m.teacher.full_resolution is want and m.teacher.full_resolution_packed is want, epoch
    m = module()                                                     # the default leaves both flags alone
    assert m.full_resolution_from_epoch is None
    m.teacher.full_resolution, m.teacher.full_resolution_packed = True, False
    m.current_epoch = 5
    m.training_step(batch)
    assert m.teacher.full_resolution is True and m.teacher.full_resolution_packed is False
    with pytest.raises(ValueError):
        module(full_resolution_from_epoch=-1)
