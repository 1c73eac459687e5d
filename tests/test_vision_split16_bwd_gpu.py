"""Split-fp16 data-gradient GEMMs of the student's vision backward: the row-scaled split against the host rule,
the transposed weight copies, the row-scaled GEMM on every kernel of the dispatcher against its device-scaled twin, the dgrad
against fp64, and the tower — against the switch-off path and the fp64 oracle, with changed and with stale weights, under a HIP
graph, run to run."""
import argparse
import os
import sys

import pytest
import torch

from dclip_amd import config as dcfg, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_vision_split16_gpu as fwd_tests                     # noqa: E402  (the §9d file: its crafted layers, Tower and bars)
from test_vision_split16_gpu import bits, norm_err, rnd, same, scalar      # noqa: E402

pytestmark = pytest.mark.gpu

WEIGHTS = ("qkv", "out", "fc1", "fc2")


def same_nan(a, b):
    """bit-equal, NaN payloads aside (a NaN is a NaN in both)"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = torch.isnan(a), torch.isnan(b)
    return bool(torch.equal(na, nb)) and bool(torch.equal(bits(a)[~na], bits(b)[~nb]))


# ------------------------------------------------------------------------------------------------ 1. row split

@pytest.mark.parametrize("rows,cols,ld", [(5, 72, 72), (130, 512, 512), (33, 3072, 3072), (7, 2304, 2320), (3, 3200, 3200)])
def test_row_split_equals_host_rule(rows, cols, ld):
    """(3, 3200): past 3072 columns the row is read twice (the second time from the cache) instead of held in registers."""
    from dclip_amd import _lib, engine, ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(rows * cols)
    x = torch.randn((rows, ld), generator=g) * torch.exp(4.0 * torch.randn((rows, 1), generator=g))
    x[0] = 0.0
    x[1, cols - 1] = float("inf")
    x[2, 3] = float("nan")
    if rows > 4:
        x[3] = x[3] / x[3, :cols].abs().max() * 2.0 ** -120
        x[4] = x[4] / x[4, :cols].abs().max() * 2.0 ** 100
        x[3, 5], x[4, 5] = 2.0 ** -120, -2.0 ** 100
    xd = x.to(dev)[:, :cols]
    assert xd.stride(0) == ld
    y, ra = ops.split_f16x3_rows(xd)
    assert (b".cached" if cols > 3072 else b".regs") in _lib.load().dclip_last_launch()
    want, want_ra = engine.split16_rows_host(x[:, :cols])
    assert same(ra.cpu(), want_ra), (ra.cpu(), want_ra)
    assert same_nan(y.cpu(), want)
    assert not y[0].any() and float(ra[0]) == 1.0
    assert not bool(torch.isfinite(y[1].float()).all()) and not bool(torch.isfinite(y[2].float()).all())
    assert bool(torch.isfinite(y[3:].float()).all())
    y2, ra2 = ops.split_f16x3_rows(xd)
    assert same_nan(y2.cpu(), y.cpu()) and same(ra2, ra)


# ------------------------------------------------------------------------------------------------ 2. transposed weight copies

def test_transposed_weight_copies():
    from dclip_amd import ops
    dev = torch.device("cuda:0")
    host = fwd_tests.crafted_layers()
    layers = [{k: v.to(dev) for k, v in L.items()} for L in host]
    plain = ops.split16_table(layers)
    ops.split16_refresh(plain)
    tab = ops.split16_table(layers, transposed=True)
    ops.split16_refresh(tab)
    plan = tab["plan"].cpu()
    assert same(plan[:4], plain["plan"].cpu()[:4])                      # layer 4 holds an inf: NaN scales compare unequal
    for li in (0, 1, 3):
        for w in WEIGHTS:
            src = layers[li][w + "_w"]
            sc = float(plan[li, ops.SPLIT16_PLAN_W[w]])
            assert same(tab["w"][li][w], plain["w"][li][w]), (li, w)    # the forward copies are what they were
            assert same(tab["w"][li][w], ops.split_f16x3(src, sc, 1)), (li, w)
            assert same(tab["wt"][li][w], ops.split_f16x3(src.t().contiguous(), sc, 1)), (li, w)
            assert float(plan[li, ops.SPLIT16_PLAN_WALPHA[w]]) == 1.0 / sc, (li, w)
    assert not tab["wt"][1]["fc2"].any()                                # the all-zero weight
    with pytest.raises(ValueError):                                     # 44 rows: no 16-byte groups of 8 in the transposed copy
        ops.split16_table([{k: v.to(dev) for k, v in fwd_tests.crafted_layer(7, D=72, I=44).items()}], transposed=True)


# ------------------------------------------------------------------------------------------------ 3. rows-GEMM

def check_rows_gemm(M, N, K):
    """The row-scaled GEMM on whichever kernel the dispatcher picks for the shape under the switches that are set: row_alpha = 1
    against gemm_f16_dev bit for bit; powers of two against that output times row_alpha (exact); DGELU on an fp32 h against the
    plain output times the fp32 GEMM's own quick_gelu'(h) (ops.gemm with EPI_DGELU on a product that is exactly one)."""
    from dclip_amd import ops
    dev = torch.device("cuda:0")
    a16, w16 = rnd((M, K), 1).half().to(dev), rnd((N, K), 2, 0.1).half().to(dev)
    ap = scalar(2.0 ** -5, dev)
    base = ops.gemm_f16_dev(a16, w16, ap.data_ptr())
    ones = torch.ones((M,), dtype=torch.float32, device=dev)
    assert same(ops.gemm_f16_rows_dev(a16, w16, ap.data_ptr(), ones), base), (M, N, K)
    ra = torch.exp2(torch.randint(-30, 31, (M,), generator=torch.Generator().manual_seed(M)).float()).to(dev)
    want = base * ra[:, None]
    got = ops.gemm_f16_rows_dev(a16, w16, ap.data_ptr(), ra)
    assert same(got, want), (M, N, K)
    h = rnd((M, N), 5, 2.0).to(dev)
    e1 = torch.zeros((M, 8), dtype=torch.float32, device=dev)
    e2 = torch.zeros((8, N), dtype=torch.float32, device=dev)
    e1[:, 0] = 1.0
    e2[0] = 1.0
    dg = ops.gemm(e1, e2, ops.LAYOUT_NN, aux=h, epilogue=ops.EPI_DGELU)              # 1 * quick_gelu'(h), gemm_f32's statement
    got = ops.gemm_f16_rows_dev(a16, w16, ap.data_ptr(), ra, dgelu_h=h)
    assert same(got, want * dg), (M, N, K)
    s = torch.sigmoid(1.702 * h)
    assert norm_err(dg, s * (1.0 + 1.702 * h * (1.0 - s))) <= 1e-5                    # and that factor is quick_gelu'
    # row_alpha at the clamp of the row rule beside accumulators of 2^25 and more: (acc alpha) row_alpha stays finite where
    # acc row_alpha alone would overflow, so the order of the two scalings is part of what is checked
    big_a, big_w = (a16 * 2048.0).half(), (w16 * 32768.0).half()
    ap2 = scalar(2.0 ** -40, dev)
    base2 = ops.gemm_f16_dev(big_a, big_w, ap2.data_ptr())
    assert float(base2.abs().max()) * 2.0 ** 40 >= 2.0 ** 25 and bool(torch.isfinite(base2).all())
    ra2 = torch.where(torch.arange(M, device=dev) % 2 == 0, 2.0 ** 100, 2.0 ** -60).float()
    got2 = ops.gemm_f16_rows_dev(big_a, big_w, ap2.data_ptr(), ra2)
    assert bool(torch.isfinite(got2).all()) and same(got2, base2 * ra2[:, None]), (M, N, K)


# the selection shapes of the §9d file: register-staged 64x64 (two), register-staged 128x128, ping-pong 256x256
@pytest.mark.parametrize("M,N,K", [(130, 72, 40), (231, 1536, 512), (2048, 2048, 64), (2816, 3072, 64)])
def test_rows_gemm_equals_dev(M, N, K):
    from dclip_amd import _lib
    check_rows_gemm(M, N, K)
    want = {130: b".r64", 231: b".r64", 2048: b".r128", 2816: b".pp"}[M]
    assert _lib.load().dclip_last_launch().endswith(b"gemm_f16_scaled_rows_dev" + want), _lib.load().dclip_last_launch()


def test_rows_gemm_never_takes_the_persistent_kernel(monkeypatch):
    from dclip_amd import _lib
    monkeypatch.setenv("DCLIP_BF16_PERSIST", "1")
    check_rows_gemm(5900, 6144, 64)
    assert b".ppp" not in _lib.load().dclip_last_launch() and b".pp" in _lib.load().dclip_last_launch()


# ------------------------------------------------------------------------------------------------ 4. the dgrad end to end

def test_dgrad_against_fp64():
    """(300, 768) . (768, 264), dY with rows spread over e^(8 sigma): worst row-relative error at most 4x ops.gemm's own."""
    from dclip_amd import engine, ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(11)
    dy = torch.randn((300, 768), generator=g) * torch.exp(8.0 * torch.randn((300, 1), generator=g))
    dy[7] = 0.0
    w = torch.randn((768, 264), generator=g) * 0.05
    want = dy.double() @ w.double()
    f = engine.split16_weight_exp(float(w.abs().max()))
    wt3 = ops.split_f16x3(w.t().contiguous().to(dev), 2.0 ** f, 1)
    dy3, ra = ops.split_f16x3_rows(dy.to(dev))
    alpha = scalar(2.0 ** -f, dev)                                       # kept alive: the GEMM reads it through its address
    got = ops.gemm_f16_rows_dev(dy3, wt3, alpha.data_ptr(), ra).cpu()
    plain = ops.gemm(dy.to(dev), w.to(dev), ops.LAYOUT_NN).cpu()

    def row_rel(x):
        d, s = (x.double() - want).abs().amax(dim=1), want.abs().amax(dim=1)
        return float((d[s > 0] / s[s > 0]).max())
    es, ep = row_rel(got), row_rel(plain)
    print(f"dgrad 300x768x264, row spread sigma 8: worst row-relative error split {es:.3e} fp32 {ep:.3e} ratio {es / ep:.2f}")
    assert es <= 4 * ep
    assert not got[7].any()


# ------------------------------------------------------------------------------------------------ 5. tower

def launches(fn):
    """the library's launch names during fn()"""
    from dclip_amd import _lib
    lib = _lib.load()
    names = []
    real = _lib.check

    def spy(rc, what=""):
        names.append(lib.dclip_last_launch())
        return real(rc, what)
    _lib.check = spy
    try:
        out = fn()
    finally:
        _lib.check = real
    return out, names


def grad_bars(t, grads, grads_off, tag, want_grads=None):
    """every parameter gradient within 1e-5 of the switch-off path norm-wise, and at most 4x its error against fp64"""
    want_grads = t.want_grads if want_grads is None else want_grads
    worst_d, worst_r = (0.0, None), (0.0, None)
    bad = []
    for k, w in want_grads.items():
        if float(w.abs().max()) == 0.0 or k.endswith("k_proj.bias"):
            continue
        d = norm_err(grads[k], grads_off[k])
        gs, gp = norm_err(grads[k].reshape(w.shape), w), norm_err(grads_off[k].reshape(w.shape), w)
        worst_d = max(worst_d, (d, k))
        worst_r = max(worst_r, (gs / gp, k))
        if d > 1e-5 or gs > 4 * gp:
            bad.append((k, d, gs, gp))
    print(f"{tag}: worst gradient split-bwd vs off {worst_d[0]:.3e} ({worst_d[1]}); worst ratio vs fp64 {worst_r[0]:.2f} ({worst_r[1]})")
    assert not bad, (tag, bad)


@pytest.mark.parametrize("name", ["tiny", "vit_b32"])
def test_tower_bwd_split_against_off_and_fp64(name, monkeypatch):
    from dclip_amd import engine
    t = fwd_tests.tower(name)
    monkeypatch.setattr(engine, "_VSPLIT16", True)
    monkeypatch.setattr(engine, "_VSPLIT16_BWD", True)
    t.model._vsplit16_cache().clear()                                   # a table with transposed copies, whatever ran before
    (feat_s, grads_s, _), names_s = launches(t.step)
    assert any(b"gemm_f16_scaled_rows_dev" in n for n in names_s) and any(b"split_f32_f16x3_rows" in n for n in names_s)
    L = t.cfg.vision.num_hidden_layers
    assert sum(b"gemm_f16_scaled_rows_dev" in n for n in names_s) == 4 * (L - 1) + 1
    feat_2, grads_2, _ = t.step()
    assert same(feat_2, feat_s) and all(same(grads_2[k], grads_s[k]) for k in grads_s)           # run to run
    monkeypatch.setattr(engine, "_VSPLIT16_BWD", False)
    (feat_o, grads_o, _), names_o = launches(t.step)
    assert not any(b"gemm_f16_scaled_rows_dev" in n or b"split_f32_f16x3_rows" in n for n in names_o)
    assert same(feat_o, feat_s)                                          # the forward is untouched
    assert not all(same(grads_o[k], grads_s[k]) for k in grads_s)
    grad_bars(t, grads_s, grads_o, name)
    # switch off = the parent's schedule: the same launches and the same bits as a table built without transposed copies
    t.model._vsplit16_cache().clear()
    (feat_p, grads_p, _), names_p = launches(t.step)
    assert "wt" not in t.model._vsplit16_cache()["__vsplit16__"]["tab"]
    assert [n for n in names_p if not n.startswith(b"split16_")] == names_o             # but for the refresh of the new table
    assert b"split16_weights" in names_p and b"split16_weights.t" not in names_p
    assert same(feat_p, feat_o) and all(same(grads_p[k], grads_o[k]) for k in grads_o)
    t.model._vsplit16_cache().clear()


def change_weights(model):
    """An in-place change of every encoder-layer weight that keeps the tower well conditioned.  (The §9d file's x8 / gamma = 50
    saturates the attention: the fp64 oracle's gradients are NaN there and the fp32 path's own gradients move by O(1) under a
    change of summation order, so no 1e-5 bar between two paths can be asked of it.)"""
    with torch.no_grad():
        for layer in model.vision_model.encoder.layers:
            for n, p in layer.named_parameters():
                if n.endswith("weight") and p.dim() == 2:
                    p.mul_(1.5)
                elif "layer_norm" in n and n.endswith("weight"):
                    p.add_(0.25)


def test_changed_and_stale_weights(monkeypatch, caplog):
    import logging
    from dclip_amd import engine
    from dclip_amd.clip_model import from_hf_state_dict
    t = fwd_tests.tower("tiny")
    model = from_hf_state_dict(t.cfg, t.sd, device=t.dev)
    monkeypatch.setattr(engine, "_VSPLIT16", True)
    monkeypatch.setattr(engine, "_VSPLIT16_BWD", True)
    monkeypatch.setattr(engine, "_SPLIT16_LOGGED", set())
    t.step(model)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        change_weights(model)
        feat_s, grads_s, _ = t.step(model)                              # no device -> host read, no sync
    finally:
        torch.cuda.set_sync_debug_mode("default")
    monkeypatch.setattr(engine, "_VSPLIT16_BWD", False)
    feat_o, grads_o, _ = t.step(model)
    monkeypatch.setattr(engine, "_VSPLIT16_BWD", True)
    want, want_grads = fwd_tests.oracle_for(t, model)
    assert same(feat_s, feat_o) and not all(same(grads_s[k], grads_o[k]) for k in grads_s)
    assert all(bool(torch.isfinite(w).all()) for w in want_grads.values())
    grad_bars(t, grads_s, grads_o, "weights x1.5, gamma + 0.25", want_grads)
    # stale: a watched parameter written between the forward and its backward -> that backward is the switch-off one
    for q in model.parameters():
        q.grad = None
    feat = model.get_image_features(pixel_values=t.pix_dev)
    with torch.no_grad():
        model.vision_model.encoder.layers[0].layer_norm1.bias.add_(0.0)                   # a version bump, same values
    torch.cuda.set_sync_debug_mode("error")
    try:
        with caplog.at_level(logging.WARNING, logger="dclip_amd"):
            (feat * t.probe_dev).sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    stale = {k: v for k, v in fwd_tests.hf_named_grads(model).items() if k in grads_o}
    assert all(same(stale[k], grads_o[k]) for k in grads_o)
    assert sum("between a forward and its backward" in r.getMessage() for r in caplog.records) == 1


def test_graphed_step_with_split_backward(monkeypatch):
    from dclip_amd import engine
    from dclip_amd.CLIP_image_distillation import CLIPImageDistillation
    from dclip_amd.clip_model import from_hf_state_dict
    from dclip_amd.graph import GraphedStep
    dev = torch.device("cuda:0")
    cfg = dcfg.tiny()
    B = 6

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

    monkeypatch.setattr(engine, "_VSPLIT16", True)
    monkeypatch.setattr(engine, "_VSPLIT16_BWD", True)
    eager, graphed, off = make(), make(), make()
    g = GraphedStep(graphed, batch(10))
    assert "wt" in graphed.student._vsplit16_cache()["__vsplit16__"]["tab"]
    for rnd_i, seed in enumerate((20, 30)):
        if rnd_i == 1:
            for mod in (eager, graphed, off):
                fwd_tests.scale_weights(mod.student)
        le, ge = eager_step(eager, batch(seed))
        lg = g.step(batch(seed))
        assert torch.equal(le, lg.detach()), (rnd_i, float(le), float(lg))
        gg = dict(graphed.named_parameters())
        for n, gr in ge.items():
            assert torch.equal(gr, gg[n].grad), (rnd_i, n)
        le2, ge2 = eager_step(eager, batch(seed))
        assert torch.equal(le, le2) and all(torch.equal(ge[n], ge2[n]) for n in ge)
        monkeypatch.setattr(engine, "_VSPLIT16_BWD", False)
        lo, go = eager_step(off, batch(seed))
        monkeypatch.setattr(engine, "_VSPLIT16_BWD", True)
        assert torch.equal(le, lo)                                       # same forward
        assert not all(torch.equal(ge[n], go[n]) for n in ge)            # the split backward did run
