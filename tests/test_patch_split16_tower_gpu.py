"""The split-fp16 patch embedding at tower level: the tiny vision tower at 64 images (patch 16: patch_dim 768, a
multiple of 32; 64 x 16 = 1024 patch rows, a multiple of 64), forced onto the path with the plan thresholds lowered — the three the
other tower tests lower and the path's own, DCLIP_PATCH_SPLIT16_MIN.

Switch on against switch off: features and every parameter gradient, patch_w first, inside the project's two bars (§9c / §9d):
1e-5 norm-wise against the off run, and an error against the fp64 oracle of at most 4x the off run's own.  That the split
arithmetic itself meets both bars on these inputs was checked on the host before this file was written, with the host emulation of
the split (hi = fp16(v), lo = fp16(v - hi), fp64 of the three products) on this tower's pixels and patch weight and on a dY with
columns spread over 2^-20 .. 2^0, norm-wise: the patch embedding 8.0e-8 against fp64 where an fp32 product has 3.5e-7, and
3.6e-7 from that fp32 product; patch_w's gradient 7.9e-8 against fp64 where fp32 has 2.9e-7, 3.0e-7 from it, its worst row 1.2e-7
of the row's own size against 5.9e-7."""
import argparse
import os
import sys

import pytest
import torch

from dclip_amd import config as dcfg
from dclip_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_vision_split16_wgrad_gpu as wgrad_tests              # noqa: E402  (tower64, switches, grad_bars)
import test_vision_split16_bwd_gpu as bwd_tests                  # noqa: E402  (launches, change_weights)
from test_vision_split16_gpu import hf_named_grads, norm_err, same   # noqa: E402

pytestmark = pytest.mark.gpu

LOW = {"DCLIP_BF16_BIG_MIN": "1", "DCLIP_F16X3_MIN": "1", "DCLIP_F16X3_TOK_MIN": "1", "DCLIP_PATCH_SPLIT16_MIN": "1"}
FUSED_TOK = b"gemm_f16x3_wgrad_tokmajor.pp3_tok.splitk_reduce"
NEW = (b"im2col_f16x2", b"split16_front", b"split_f32_f16x2_cols")
PATCH_W = "vision_model.embeddings.patch_embedding.weight"


def setup(monkeypatch, patch=True):
    from dclip_amd import engine
    wgrad_tests.switches(monkeypatch, True)
    monkeypatch.setattr(engine, "_SPLIT16_FUSED_K", True)
    monkeypatch.setattr(engine, "_SPLIT16_FUSED_TOK", True)
    monkeypatch.setattr(engine, "_VSPLIT16_PATCH", patch)
    for k, v in LOW.items():
        monkeypatch.setenv(k, v)


def gemm_spy(monkeypatch):
    """the operand shapes of every ops.gemm (the fp32 pipe) call"""
    from dclip_amd import ops
    seen, real = [], ops.gemm

    def gemm(a, b, layout, **kw):
        seen.append((tuple(a.shape), tuple(b.shape), layout))
        return real(a, b, layout, **kw)

    monkeypatch.setattr(ops, "gemm", gemm)
    return seen


def with_k(seen, K):
    return [s for s in seen if K in s[0] or K in s[1]]


def test_switch_on_against_switch_off(monkeypatch):
    t = wgrad_tests.tower64()
    v = t.cfg.vision
    K, L = v.patch_dim, v.num_hidden_layers
    assert K % 32 == 0 and K not in (v.hidden_size, 3 * v.hidden_size, v.intermediate_size, t.cfg.projection_dim)
    seen = gemm_spy(monkeypatch)
    setup(monkeypatch, True)
    t.model._vsplit16_cache().clear()
    (feat, grads, _), names = bwd_tests.launches(t.step)
    assert not with_k(seen, K), with_k(seen, K)                                        # no fp32 GEMM with K = patch_dim
    assert names.count(b"im2col_f16x2") == 1 and names.count(b"split_f32_f16x2_cols.cols") == 1
    assert names.count(b"split16_front.weight") == 1 and b"im2col.vec" not in names     # (the first forward: the weight is split)
    assert sum(n == FUSED_TOK for n in names) == 4 * (L - 1) + 1 + 1                      # the layers' weight gradients and patch_w's
    (feat_2, grads_2, _), names_2 = bwd_tests.launches(t.step)
    assert names_2.count(b"split16_front.plan") == 1 and b"split16_front.weight" not in names_2      # patch_w did not change
    assert same(feat_2, feat) and all(same(grads_2[k], grads[k]) for k in grads)          # run to run
    del seen[:]
    setup(monkeypatch, False)
    (feat_o, grads_o, _), names_o = bwd_tests.launches(t.step)
    assert not any(m in n for n in names_o for m in NEW) and names_o.count(b"im2col.vec") == 1
    assert len(with_k(seen, K)) == 2                                                      # the forward and the weight gradient
    assert not same(grads[PATCH_W], grads_o[PATCH_W])
    w = t.want_grads[PATCH_W]
    d, gs, gp = norm_err(grads[PATCH_W], grads_o[PATCH_W]), norm_err(grads[PATCH_W].reshape(w.shape), w), norm_err(grads_o[PATCH_W].reshape(w.shape), w)
    print(f"patch_w gradient: on vs off {d:.3e}; vs fp64 on {gs:.3e}, off {gp:.3e}")
    assert d <= 1e-5 and gs <= 4 * gp, (d, gs, gp)
    df, ef, eo = norm_err(feat, feat_o), norm_err(feat, t.want), norm_err(feat_o, t.want)
    print(f"features: on vs off {df:.3e}; vs fp64 on {ef:.3e}, off {eo:.3e}")
    assert df <= 1e-5 and ef <= 4 * eo, (df, ef, eo)
    wgrad_tests.grad_bars(t, grads, grads_o, "tiny B 64 split patch embedding")
    t.model._vsplit16_cache().clear()


def test_graph_replay_equals_eager(monkeypatch):
    from dclip_amd.CLIP_image_distillation import CLIPImageDistillation
    from dclip_amd.clip_model import from_hf_state_dict
    from dclip_amd.graph import GraphedStep
    dev = torch.device("cuda:0")
    cfg = dcfg.tiny()
    B = 64

    def make():
        student = from_hf_state_dict(cfg, synth.synth_clip_state_dict(cfg, seed=0), device=dev)
        hp = argparse.Namespace(learning_rate=1e-4, warmup_steps=0, total_steps=100, train_batch_size=B, eval_batch_size=B)
        return CLIPImageDistillation(hp, student, None, freeze_mode="north_star").to(dev)

    def batch(seed, gain=1.0):
        return {"pixel_values": synth.synth_pixel_values(B, cfg.vision, seed=seed).to(dev) * gain,
                "input_ids": synth.synth_input_ids(B, cfg.text, seed=seed + 1, ragged=True).to(dev),
                "teacher_image_emb": synth.synth_embeddings(B, cfg.projection_dim, seed=seed + 2).to(dev)}

    def eager_step(mod, b):
        for p in mod.parameters():
            p.grad = None
        loss = mod.training_step(b)
        loss.backward()
        return loss.detach().clone(), {n: p.grad.clone() for n, p in mod.named_parameters() if p.grad is not None}

    setup(monkeypatch, True)
    eager, graphed = make(), make()
    g = GraphedStep(graphed, batch(10))
    # other pixels at another magnitude (another activation scale), then other weights: a replay plans again on the device
    for rnd_i, (seed, gain) in enumerate(((20, 1.0), (30, 37.0), (40, 1.0))):
        if rnd_i == 2:
            for mod in (eager, graphed):
                bwd_tests.change_weights(mod.student)
                with torch.no_grad():
                    mod.student.vision_model.embeddings.patch_embedding.weight.mul_(3.0)
        (le, ge), names = bwd_tests.launches(lambda: eager_step(eager, batch(seed, gain)))
        assert b"im2col_f16x2" in names and b"split_f32_f16x2_cols.cols" in names
        lg = g.step(batch(seed, gain))
        assert torch.equal(le, lg.detach()), (rnd_i, float(le), float(lg))
        gg = dict(graphed.named_parameters())
        for n, gr in ge.items():
            assert torch.equal(gr, gg[n].grad), (rnd_i, n)


class Small:
    """a tiny vision tower without an oracle: features and gradients of one step"""

    def __init__(self, cfg, B, size=None):
        from dclip_amd.clip_model import from_hf_state_dict
        self.dev = torch.device("cuda:0")
        self.cfg = cfg
        self.model = from_hf_state_dict(cfg, synth.synth_clip_state_dict(cfg, seed=5, gain=2.0), device=self.dev)
        g = torch.Generator().manual_seed(B)
        self.pix = (synth.synth_pixel_values(B, cfg.vision, seed=1) if size is None else torch.randn((B, 3, size, size), generator=g)).to(self.dev)
        self.probe = torch.randn((B, cfg.projection_dim), generator=g).to(self.dev)
        self.interp = size is not None

    def step(self, grad=True):
        for q in self.model.parameters():
            q.grad = None
        with torch.enable_grad() if grad else torch.no_grad():
            feat = self.model.get_image_features(pixel_values=self.pix, interpolate_pos_encoding=self.interp)
            if grad:
                (feat * self.probe).sum().backward()
        return feat.detach().clone(), {k: v.clone() for k, v in hf_named_grads(self.model).items()}


DECLINES = {"patch_14": lambda: (Small(dcfg.tiny(image_size=56, patch_size=14), 64), True),      # patch_dim 588
            "rows_48": lambda: (Small(dcfg.tiny(), 3), True),                                     # 3 x 16 patch rows
            "grid": lambda: (Small(dcfg.tiny(), 64, size=96), True),                              # 6 x 6 patches on the resampled table
            "no_grad": lambda: (Small(dcfg.tiny(), 64), False)}


@pytest.mark.parametrize("case", list(DECLINES))
def test_declines_are_the_switch_off_step(case, monkeypatch):
    s, grad = DECLINES[case]()
    setup(monkeypatch, True)
    s.step(grad)                                                                          # (the layers' table is built and fresh)
    (feat, grads), names = bwd_tests.launches(lambda: s.step(grad))
    assert not any(m in n for n in names for m in NEW), case
    setup(monkeypatch, False)
    (feat_o, grads_o), names_o = bwd_tests.launches(lambda: s.step(grad))
    assert names == names_o, case                                                         # launch for launch
    assert same(feat, feat_o) and set(grads) == set(grads_o) and all(same(grads[k], grads_o[k]) for k in grads_o), case


def test_the_switch_at_0_and_the_default_threshold_keep_the_fp32_patch_embedding(monkeypatch):
    s = Small(dcfg.tiny(), 64)
    setup(monkeypatch, True)
    (_, grads), names = bwd_tests.launches(s.step)
    assert b"im2col_f16x2" in names                                                       # (this tower does take the path)
    setup(monkeypatch, False)
    (feat_o, grads_o), names_o = bwd_tests.launches(s.step)
    assert not any(m in n for n in names_o for m in NEW) and not same(grads[PATCH_W], grads_o[PATCH_W])
    setup(monkeypatch, True)
    monkeypatch.delenv("DCLIP_PATCH_SPLIT16_MIN")                                         # 4 tiles of 256 x 256 < 128
    (feat_d, grads_d), names_d = bwd_tests.launches(s.step)
    assert names_d == names_o and same(feat_d, feat_o) and all(same(grads_d[k], grads_o[k]) for k in grads_o)


def test_fall_back_when_the_wgrad_switch_flips_between_forward_and_backward(monkeypatch):
    """The forward kept the split columns; at the backward DCLIP_VISION_SPLIT16_WGRAD is off: patch_w's gradient is the parent's
    fp32 GEMM of that backward's own dpatch with the fp32 columns made again from the saved pixels, bit for bit."""
    from dclip_amd import engine, ops
    s = Small(dcfg.tiny(), 64)
    setup(monkeypatch, True)
    s.step()                                                                              # (the tables are built)
    for q in s.model.parameters():
        q.grad = None
    kept, real = [], ops.vision_assemble_bwd

    def assemble_bwd(*a, **k):
        kept.append(real(*a, **k))
        return kept[-1]

    monkeypatch.setattr(ops, "vision_assemble_bwd", assemble_bwd)
    feat = s.model.get_image_features(pixel_values=s.pix)
    monkeypatch.setattr(engine, "_VSPLIT16_WGRAD", False)
    _, names = bwd_tests.launches(lambda: (feat * s.probe).sum().backward())
    assert b"im2col.vec" in names and not any(b"split_f32_f16x2_cols" in n for n in names)
    assert len(kept) == 1
    want = ops.gemm(kept[0], ops.im2col(s.pix, s.cfg.vision.patch_size), ops.LAYOUT_TN)
    got = hf_named_grads(s.model)[PATCH_W]
    assert same(got.reshape(want.shape), want)
