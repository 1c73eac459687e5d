"""Split-fp16 weight-gradient GEMMs of the student's vision backward: the fused pass over dY (row split, column
statistics, bias gradient, column-scaled split) against the host rules, the segmented token-major GEMM against fp64 on the same
pieces, and the tower — against the switch-off path and the fp64 oracle, with stale weights, under a HIP graph, run to run."""
import argparse
import os
import sys

import pytest
import torch

from dclip_amd import config as dcfg, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_vision_split16_gpu as fwd_tests                     # noqa: E402  (the §9d file: Tower, oracle and helpers)
import test_vision_split16_bwd_gpu as bwd_tests                 # noqa: E402  (the §9e file: launches, grad_bars)
from test_vision_split16_gpu import norm_err, rnd, same, scalar  # noqa: E402
from test_vision_split16_bwd_gpu import same_nan                # noqa: E402

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ 1. the fused pass over dY

def crafted_dy(rows, cols, ld, seed):
    """rows and columns spread over e^(4 sigma); column 0 all zero, 1 with one inf, 2 with one NaN, 3 subnormal only, 4 holding
    1e-30 beside one 1e+10"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((rows, ld), generator=g) * torch.exp(4.0 * torch.randn((rows, 1), generator=g)) \
        * torch.exp(4.0 * torch.randn((1, ld), generator=g))
    x[:, 0] = 0.0
    x[0, 1] = float("inf")
    x[min(1, rows - 1), 2] = float("nan")
    x[:, 3] = torch.randint(1, 1 << 20, (rows,), generator=g).float() * 2.0 ** -149
    x[:, 4] = 1e-30
    x[rows // 2, 4] = 1e10
    return x


def check_fused_pass(rows, cols, ld, seed):
    from dclip_amd import engine, ops
    dev = torch.device("cuda:0")
    x = crafted_dy(rows, cols, ld, seed)
    xd = x.to(dev)[:, :cols]
    assert rows == 1 or xd.stride(0) == ld
    xs = x[:, :cols]
    db = torch.empty((cols,), dtype=torch.float32, device=dev)
    y, ra, yc, ce, ca = ops.split_f16x3_rows_colstats(xd, db=db)
    y0, ra0 = ops.split_f16x3_rows(xd)
    assert same_nan(y, y0) and same(ra, ra0), (rows, cols, ld)
    e = torch.tensor([engine.split16_col_exp(float(r)) for r in xs.abs().amax(dim=0).double()], dtype=torch.int32)
    assert torch.equal(ce.cpu(), e), (rows, cols, ld, ce.cpu()[:8], e[:8])
    assert same(ca.cpu(), torch.exp2(-e.float())), (rows, cols, ld)
    assert int(e[0]) == 0 and int(e[1]) == 0 and int(e[2]) == 0 and int(e[3]) == 100
    v = xs * torch.exp2(e.float())[None, :]
    hi = v.half()
    lo = (v - hi.float()).half()
    assert same_nan(yc.cpu(), torch.cat([hi, lo], dim=1)), (rows, cols, ld)
    fin = torch.isfinite(xs).all(dim=0)
    assert bool(torch.isfinite(yc[:, :cols][:, fin.to(dev)].float()).all())                     # other columns are unaffected
    want = xs.double().sum(dim=0)
    bound = rows * 2.0 ** -24 * xs.double().abs().sum(dim=0)
    got = db.cpu().double()
    err = ((got - want).abs()[fin] / bound[fin].clamp_min(1e-300)).max()
    print(f"fused pass {rows}x{cols} ld {ld}: db worst error / bound {float(err):.3f}")
    assert bool(((got - want).abs()[fin] <= bound[fin]).all()), (rows, cols, ld)
    assert not bool(torch.isfinite(got[~fin]).any())
    db2 = torch.empty_like(db)
    out2 = ops.split_f16x3_rows_colstats(xd, db=db2)
    assert all(same_nan(a, b) for a, b in zip(out2, (y, ra, yc, ce, ca))) and same_nan(db2, db)


@pytest.mark.parametrize("cols", [8, 264, 768, 3072, 3080])
@pytest.mark.parametrize("pad", [8, 40])
def test_fused_pass(cols, pad):
    """3080 columns: past 3072 the running column values live in the workspace instead of registers"""
    for rows in (1, 5, 300):
        check_fused_pass(rows, cols, cols + pad, 1000 * rows + cols + pad)


def test_fused_pass_at_the_wave_cap():
    """more than 8 x 1024 rows: the number of waves (and partials) stops growing"""
    check_fused_pass(8200, 8, 16, 7)


# ------------------------------------------------------------------------------------------------ 2. the segmented GEMM

SIZES = (8, 264, 520)


def check_seg_gemm(tokens, s0, M, N, a_seg, w_seg, seed):
    from dclip_amd import ops
    dev = torch.device("cuda:0")
    lddy, ldx = 2 * M + 8, 3 * N + 16
    dy = rnd((tokens, lddy), seed, 3.0).half()
    x = rnd((tokens, ldx), seed + 1, 5.0).half()
    ca = torch.exp2(torch.randint(-20, 21, (M,), generator=torch.Generator().manual_seed(seed + 2)).float())
    act = scalar(2.0 ** 7, dev)
    got = ops.gemm_f16_wgrad_tokmajor_seg3(dy.to(dev), x.to(dev), M, N, ca.to(dev), act.data_ptr(), a_seg=a_seg, w_seg=w_seg,
                                           splits=s0)
    want = torch.zeros((M, N), dtype=torch.float64)
    terms = torch.zeros((M, N), dtype=torch.float64)
    for a0, w0 in zip(a_seg, w_seg):
        a, w = dy[:, a0:a0 + M].double(), x[:, w0:w0 + N].double()
        want += a.t() @ w
        terms += a.abs().t() @ w.abs()
    sc = (ca.double() * 2.0 ** -7)[:, None]
    slabs = 3 * min(s0, tokens // 64)
    bound = (3 * tokens + slabs) * 2.0 ** -24 * terms * sc
    err = (got.cpu().double() - want * sc).abs()
    worst = float((err / bound).max())
    assert bool((err <= bound).all()), (tokens, s0, M, N, worst)
    got2 = ops.gemm_f16_wgrad_tokmajor_seg3(dy.to(dev), x.to(dev), M, N, ca.to(dev), act.data_ptr(), a_seg=a_seg, w_seg=w_seg,
                                            splits=s0)
    assert same(got, got2)
    return worst


@pytest.mark.parametrize("tokens,s0", [(64, 1), (192, 1), (192, 2), (192, 3), (320, 3)])
def test_seg_gemm_against_fp64(tokens, s0):
    """64 tokens: one K-tile per segment; 320 tokens in 3 splits: chunks of 128, 128 and 64; 264 = one full and one edge tile"""
    from dclip_amd import _lib
    worst = 0.0
    for i, M in enumerate(SIZES):
        for j, N in enumerate(SIZES):
            step = ((0, M, 0), (0, 0, N))                                   # [hi|lo] with [hi|lo|hi], as in the step
            perm = ((M, 0, M), (2 * N, N, 0))
            a_seg, w_seg = step if (i + j) % 2 == 0 else perm
            worst = max(worst, check_seg_gemm(tokens, s0, M, N, a_seg, w_seg, 100 * i + 10 * j + tokens))
    assert _lib.load().dclip_last_launch().endswith(b"gemm_f16_wgrad_tokmajor_seg3.pp_tok_seg.splitk_reduce")
    print(f"segmented GEMM tokens {tokens} s0 {s0}: worst error / bound {worst:.4f}")


def test_seg_gemm_large_col_alpha_stays_finite():
    """col_alpha = 2^100 beside accumulators of 2^25 and more: the activation scale's reciprocal is applied first"""
    from dclip_amd import ops
    dev = torch.device("cuda:0")
    tokens, M, N = 192, 264, 8
    dy = (torch.randint(0, 2, (tokens, 2 * M), generator=torch.Generator().manual_seed(3)).float() * 2048.0 + 2048.0).half()
    x = (torch.randint(0, 2, (tokens, 3 * N), generator=torch.Generator().manual_seed(4)).float() * 1024.0 + 1024.0).half()
    ca = torch.where(torch.arange(M) % 2 == 0, 2.0 ** 100, 2.0 ** -60).float()
    act = scalar(2.0 ** 24, dev)
    got = ops.gemm_f16_wgrad_tokmajor_seg3(dy.to(dev), x.to(dev), M, N, ca.to(dev), act.data_ptr(), splits=2).cpu()
    acc = dy[:, :M].double().t() @ x[:, :N].double() + dy[:, M:].double().t() @ x[:, :N].double() \
        + dy[:, :M].double().t() @ x[:, N:2 * N].double()
    assert float(acc.min()) >= 2.0 ** 25
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got.double(), acc * 2.0 ** -24 * ca.double()[:, None])               # integers below 2^24 2^7: every sum exact


def test_seg_gemm_plan_declines():
    from dclip_amd import ops
    dev = torch.device("cuda:0")
    assert ops.gemm_f16_wgrad_tokmajor_seg3_plan(768, 768, 100) == 0
    assert ops.gemm_f16_wgrad_tokmajor_seg3_plan(4, 768, 128) == 0
    assert ops.gemm_f16_wgrad_tokmajor_seg3_plan(768, 12, 128) == 0
    assert ops.gemm_f16_wgrad_tokmajor_seg3_plan(768, 768, 12800) == 9
    assert ops.gemm_f16_wgrad_tokmajor_seg3_plan(2304, 768, 12800) == 3
    assert ops.gemm_f16_wgrad_tokmajor_seg3_plan(3072, 768, 12800) == 2
    assert ops.gemm_f16_wgrad_tokmajor_seg3_plan(128, 256, 64) == 1
    act = scalar(1.0, dev)
    for tokens, M in ((100, 8), (128, 4)):
        dy = torch.zeros((tokens, 2 * 8), dtype=torch.float16, device=dev)
        x = torch.zeros((tokens, 3 * 8), dtype=torch.float16, device=dev)
        ca = torch.ones((M,), dtype=torch.float32, device=dev)
        assert ops.gemm_f16_wgrad_tokmajor_seg3(dy, x, M, 8, ca, act.data_ptr()) is None


# ------------------------------------------------------------------------------------------------ 3. the tower

NEW = (b"split_f32_f16x3_rows_colstats", b"gemm_f16_wgrad_tokmajor_seg3")


class Tower64(fwd_tests.Tower):
    """the tiny tower at 64 images: 64 x 17 tokens, a multiple of 64, so the plan takes every full-size weight gradient"""

    def __init__(self):
        from dclip_amd.clip_model import from_hf_state_dict
        from oracle import dclip_oracle as O
        self.dev = torch.device("cuda:0")
        self.cfg = dcfg.tiny()
        self.B = 64
        self.sd = synth.synth_clip_state_dict(self.cfg, seed=5, gain=2.0)
        self.pix = synth.synth_pixel_values(self.B, self.cfg.vision, seed=1)
        self.probe = rnd((self.B, self.cfg.projection_dim), 9)
        self.model = from_hf_state_dict(self.cfg, self.sd, device=self.dev)
        self.pix_dev, self.probe_dev = self.pix.to(self.dev), self.probe.to(self.dev)
        p = {k: v.double().requires_grad_(True) for k, v in fwd_tests.vision_keys(self.sd).items()}
        feat = O.vision_tower(p, self.pix.double(), self.cfg.vision)
        (feat * self.probe.double()).sum().backward()
        self.want, self.want_grads = feat.detach(), {k: v.grad for k, v in p.items()}


_T64 = []


def tower64():
    if not _T64:
        _T64.append(Tower64())
    return _T64[0]


def switches(monkeypatch, wgrad):
    from dclip_amd import engine
    monkeypatch.setattr(engine, "_VSPLIT16", True)
    monkeypatch.setattr(engine, "_VSPLIT16_BWD", True)
    monkeypatch.setattr(engine, "_VSPLIT16_WGRAD", wgrad)


def grad_bars(t, grads, grads_off, tag):
    """§9e's bars (test_vision_split16_bwd_gpu.grad_bars), bias gradients included: every parameter gradient within 1e-5 of the
    switch-off path norm-wise, and at most 4x its error against fp64.  (A copy: that helper cannot order two keys whose
    difference is exactly zero, which is what most gradients show here.)"""
    worst_d, worst_r, bad = (0.0, ""), (0.0, ""), []
    for k, w in t.want_grads.items():
        if float(w.abs().max()) == 0.0 or k.endswith("k_proj.bias"):
            continue
        d = norm_err(grads[k], grads_off[k])
        gs, gp = norm_err(grads[k].reshape(w.shape), w), norm_err(grads_off[k].reshape(w.shape), w)
        worst_d, worst_r = max(worst_d, (d, k)), max(worst_r, (gs / gp, k))
        if d > 1e-5 or gs > 4 * gp:
            bad.append((k, d, gs, gp))
    print(f"{tag}: worst gradient split-wgrad vs off {worst_d[0]:.3e} ({worst_d[1]}); worst ratio vs fp64 {worst_r[0]:.2f} ({worst_r[1]})")
    assert not bad, (tag, bad)


def row_bars(t, grads, grads_off, tag):
    """what the column scale exists for: every ROW of every weight gradient, relative to that row's own size, at most 4x the
    switch-off path's error against fp64"""
    bad, worst = [], (0.0, None)
    for k, w in t.want_grads.items():
        if w.dim() != 2 or "encoder.layers" not in k:
            continue

        def row_rel(x):
            d, s = (x.double().cpu().reshape(w.shape) - w).abs().amax(dim=1), w.abs().amax(dim=1)
            return float((d[s > 0] / s[s > 0]).max())
        es, ep = row_rel(grads[k]), row_rel(grads_off[k])
        worst = max(worst, (es / ep, k))
        if es > 4 * ep:
            bad.append((k, es, ep))
    print(f"{tag}: worst per-row ratio split-wgrad / off against fp64 {worst[0]:.2f} ({worst[1]})")
    assert not bad, (tag, bad)


def test_tower_takes_the_split_wgrads(monkeypatch):
    t = tower64()
    L = t.cfg.vision.num_hidden_layers
    assert all(bool(torch.isfinite(w).all()) for w in t.want_grads.values())
    switches(monkeypatch, True)
    t.model._vsplit16_cache().clear()
    (feat_s, grads_s, _), names_s = bwd_tests.launches(t.step)
    n_wgrad = 4 * (L - 1) + 1
    assert sum(n.endswith(b"gemm_f16_wgrad_tokmajor_seg3.pp_tok_seg.splitk_reduce") for n in names_s) == n_wgrad
    assert sum(n.endswith(b"split_f32_f16x3_rows_colstats.cols") for n in names_s) == n_wgrad
    assert not any(n.startswith(b"split_f32_f16x3_rows.") or n == b"split_f32_f16x3_rows" for n in names_s)   # one pass per dY
    feat_2, grads_2, _ = t.step()
    assert same(feat_2, feat_s) and all(same(grads_2[k], grads_s[k]) for k in grads_s)           # run to run
    switches(monkeypatch, False)
    (feat_o, grads_o, _), names_o = bwd_tests.launches(t.step)
    assert not any(m in n for n in names_o for m in NEW)
    assert sum(b"split_f32_f16x3_rows" in n for n in names_o) == n_wgrad                         # the parent's list: §9e's
    assert same(feat_o, feat_s)                                                                  # the forward is untouched
    assert not all(same(grads_o[k], grads_s[k]) for k in grads_s)
    grad_bars(t, grads_s, grads_o, "tiny B 64")                                        # biases included
    row_bars(t, grads_s, grads_o, "tiny B 64")
    t.model._vsplit16_cache().clear()


@pytest.mark.parametrize("name", ["tiny", "vit_b32"])
def test_tower_declined_shapes_take_the_fp32_wgrads(name, monkeypatch):
    """tiny B 4 (68 tokens) and vit_b32 B 2 (100 tokens): not a multiple of 64, so the plan declines every weight gradient and
    the step is the switch-off step, launch for launch and bit for bit"""
    from dclip_amd import engine
    t = fwd_tests.tower(name)
    switches(monkeypatch, True)
    t.model._vsplit16_cache().clear()
    (feat_s, grads_s, _), names_s = bwd_tests.launches(t.step)
    assert not any(m in n for n in names_s for m in NEW)
    assert any(b"gemm_f16_scaled_rows_dev" in n for n in names_s)
    switches(monkeypatch, False)
    (feat_o, grads_o, _), names_o = bwd_tests.launches(t.step)
    core = lambda names: [n for n in names if not n.startswith(b"split16_")]      # noqa: E731  (but for the table's refresh)
    assert core(names_s) == core(names_o)
    assert same(feat_s, feat_o) and all(same(grads_s[k], grads_o[k]) for k in grads_o)
    monkeypatch.setattr(engine, "_VSPLIT16_BWD", False)
    _, grads_p, _ = t.step()
    grad_bars(t, grads_s, grads_p, name + " (declined)")
    t.model._vsplit16_cache().clear()


def test_stale_weights_take_the_switch_off_backward(monkeypatch):
    from dclip_amd import engine
    from dclip_amd.clip_model import from_hf_state_dict
    t = tower64()
    model = from_hf_state_dict(t.cfg, t.sd, device=t.dev)
    switches(monkeypatch, False)
    monkeypatch.setattr(engine, "_VSPLIT16_BWD", False)
    _, grads_o, _ = t.step(model)                                       # the plain backward
    model._vsplit16_cache().clear()                                     # a table with transposed copies from here on
    switches(monkeypatch, True)
    _, grads_s, _ = t.step(model)
    assert not all(same(grads_s[k], grads_o[k]) for k in grads_o)
    for q in model.parameters():
        q.grad = None
    feat = model.get_image_features(pixel_values=t.pix_dev)
    with torch.no_grad():
        model.vision_model.encoder.layers[0].layer_norm1.bias.add_(0.0)                   # a version bump, same values
    torch.cuda.set_sync_debug_mode("error")
    try:
        (feat * t.probe_dev).sum().backward()                            # no device -> host read, no sync
    finally:
        torch.cuda.set_sync_debug_mode("default")
    stale = {k: v for k, v in fwd_tests.hf_named_grads(model).items() if k in grads_o}
    assert all(same(stale[k], grads_o[k]) for k in grads_o)


def test_graphed_step_with_split_wgrads(monkeypatch):
    from dclip_amd import engine
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

    def batch(seed):
        return {"pixel_values": synth.synth_pixel_values(B, cfg.vision, seed=seed).to(dev),
                "input_ids": synth.synth_input_ids(B, cfg.text, seed=seed + 1, ragged=True).to(dev),
                "teacher_image_emb": synth.synth_embeddings(B, cfg.projection_dim, seed=seed + 2).to(dev)}

    def eager_step(mod, b):
        for p in mod.parameters():
            p.grad = None
        loss = mod.training_step(b)
        loss.backward()
        return loss.detach().clone(), {n: p.grad.clone() for n, p in mod.named_parameters() if p.grad is not None}

    switches(monkeypatch, True)
    eager, graphed, off = make(), make(), make()
    g = GraphedStep(graphed, batch(10))
    for rnd_i, seed in enumerate((20, 30)):
        if rnd_i == 1:
            for mod in (eager, graphed, off):
                bwd_tests.change_weights(mod.student)
        (le, ge), names = bwd_tests.launches(lambda: eager_step(eager, batch(seed)))
        assert any(NEW[1] in n for n in names)
        lg = g.step(batch(seed))
        assert torch.equal(le, lg.detach()), (rnd_i, float(le), float(lg))
        gg = dict(graphed.named_parameters())
        for n, gr in ge.items():
            assert torch.equal(gr, gg[n].grad), (rnd_i, n)
        le2, ge2 = eager_step(eager, batch(seed))
        assert torch.equal(le, le2) and all(torch.equal(ge[n], ge2[n]) for n in ge)
        monkeypatch.setattr(engine, "_VSPLIT16_WGRAD", False)
        lo, go = eager_step(off, batch(seed))
        monkeypatch.setattr(engine, "_VSPLIT16_WGRAD", True)
        assert torch.equal(le, lo)                                       # same forward
        assert not all(torch.equal(ge[n], go[n]) for n in ge)            # the split weight gradients did run
