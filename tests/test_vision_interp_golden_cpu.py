"""CPU-only: tests/golden/vision_interp.npz and vision_interp_HxW.npz (tools/make_vision_interp_golden.py) are what the GPU
test takes them for — header, sizes and shapes — and the position tables HF resampled are the fp64 reference of
tests/kernel_checks_interp.py applied to the golden's own position table, up to the error of torch's float32 bicubic kernel."""
import numpy as np

from dclip_amd import config as dcfg, synth
from tests import kernel_checks_interp as ki

SIZES = [(96, 96), (64, 112), (80, 50), (64, 64)]
V = "vision_model."
GRAD_KEYS = [V + "embeddings.position_embedding.weight", V + "embeddings.class_embedding", V + "embeddings.patch_embedding.weight",
             "visual_projection.weight"] + [V + f"encoder.layers.0.self_attn.{n}_proj.weight" for n in "qkv"]


def _versions_ok(g):
    versions = str(g["__versions__"])
    return "torch " in versions and "transformers " in versions and "numpy " in versions


def test_header_sizes_and_shapes(golden):
    common = golden("vision_interp.npz")
    cfg = dcfg.tiny()
    v = cfg.vision
    assert _versions_ok(common)
    assert common["sizes"].tolist() == [list(s) for s in SIZES]
    sd = synth.synth_clip_state_dict(cfg, seed=7, gain=4.0)
    assert np.array_equal(common["position_embedding"], sd[GRAD_KEYS[0]].numpy())     # the seeded weights of towers_tiny.npz
    assert common["r"].shape == (2, cfg.projection_dim)
    for h, w in SIZES:
        g = golden(f"vision_interp_{h}x{w}.npz")
        assert _versions_ok(g)
        q = g["pixel_q"]
        assert q.dtype == np.int8 and q.shape == (2, 3, h, w) and np.abs(q).max() <= 32
        assert g["image_emb"].shape == (2, cfg.projection_dim) and np.isfinite(g["image_emb"]).all()
        assert g["pos_table"].shape == (1 + (h // v.patch_size) * (w // v.patch_size), v.hidden_size)
        for k in GRAD_KEYS:                               # every gradient whole, at every size
            gr = g[f"grad.{k}"]
            assert gr.shape == tuple(sd[k].shape) and np.isfinite(gr).all() and np.abs(gr).max() > 0, (k, h, w)


def test_hf_position_tables_are_the_fp64_reference(golden):
    """torch's float32 kernel forms the source coordinate in fp32: for g = 4 an error of a few 2^-24 x 4 in t, times the
    cubic's slope (below 1.5) on each axis, on 16 taps of magnitude max|pos| — well inside 64 x 2^-22 x max|pos| (1.5e-5
    relative), which a wrong A, align_corners, dropped clamped taps or a transposed grid miss by orders of magnitude."""
    pos = golden("vision_interp.npz")["position_embedding"]
    grid = dcfg.tiny().vision.grid
    for h, w in SIZES:
        table = golden(f"vision_interp_{h}x{w}.npz")["pos_table"]
        gh, gw = h // 16, w // 16
        worst = float(np.abs(table.astype(np.float64) - ki.interp_reference(pos, grid, gh, gw)).max() / np.abs(pos).max())
        print(f"{h}x{w}: worst |HF table - fp64 reference| / max|pos| = {worst:.3e}")
        assert worst <= 64 * 2.0 ** -22
        if (gh, gw) == (grid, grid):
            assert np.array_equal(table, pos)
    for fault in ("A_half", "align_corners", "drop_clamped", "swap_axes"):
        wrong = ki.emulate_fwd(pos, grid, 4, 7, fault=fault).astype(np.float64)
        assert float(np.abs(wrong - ki.interp_reference(pos, grid, 4, 7)).max() / np.abs(pos).max()) > 1e-3, fault
