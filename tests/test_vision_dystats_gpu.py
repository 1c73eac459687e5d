"""dY read once in the student's vision backward, on the tower: switch on against off — weight gradients and dX
bit for bit, bias gradients within the column-sum bound, the exact count of calls that take the single pass — declined shapes,
stale weights, a HIP-graph replay, run to run."""
import argparse
import os
import sys

import pytest
import torch

from dclip_amd import config as dcfg, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import schedule_checks                                            # noqa: E402
import test_vision_split16_gpu as fwd_tests                       # noqa: E402
import test_vision_split16_bwd_gpu as bwd_tests                   # noqa: E402
import test_vision_split16_wgrad_gpu as wgrad_tests               # noqa: E402
from test_vision_split16_gpu import same                          # noqa: E402

pytestmark = pytest.mark.gpu

SINGLE = b"split_f32_f16x3_rows_cols_stats"
PRODUCERS = (b"gemm_f16_scaled_rows_dev.stats", b"attention_bwd.lean.stats", b"layernorm_bwd_stats")


def core(names):
    """the launch list but for the refresh of the split table (made by the first step after the cache was cleared)"""
    return [n for n in names if not n.startswith(b"split16_")]


def switches(monkeypatch, dystats):
    from dclip_amd import engine
    wgrad_tests.switches(monkeypatch, True)
    monkeypatch.setattr(engine, "_VSPLIT16_DYSTATS", dystats)


def spied_step(monkeypatch, t, model=None):
    """one step -> (features, gradients, launch names, calls per split entry, [(bias key, rows, sum|dY|, db)], [dx per layer])"""
    from dclip_amd import engine, ops
    calls = {"single": 0, "three": 0}
    biases, dxs = [], []
    with monkeypatch.context() as mp:
        for attr, key in (("split_f16x3_rows_cols_stats", "single"), ("split_f16x3_rows_colstats", "three")):
            def spy(*a, _orig=getattr(ops, attr), _key=key, **kw):
                calls[_key] += 1
                return _orig(*a, **kw)
            mp.setattr(ops, attr, spy)
        orig_lpg = engine.linear_param_grads

        def lpg_spy(dy, x, need_w, need_b, gr, wkey, bkey, *a, **kw):
            res = orig_lpg(dy, x, need_w, need_b, gr, wkey, bkey, *a, **kw)
            if need_b:
                biases.append((bkey, dy.shape[0], dy.abs().sum(0, dtype=torch.float64), gr[bkey].clone()))
            return res
        mp.setattr(engine, "linear_param_grads", lpg_spy)
        for name in ("layer_bwd", "last_layer_bwd_cls"):
            def layer_spy(*a, _orig=getattr(engine, name), **kw):
                res = _orig(*a, **kw)
                dxs.append(res[0].clone())
                return res
            mp.setattr(engine, name, layer_spy)
        (feat, grads, _), names = bwd_tests.launches(lambda: t.step(model))
    return feat, grads, names, calls, biases, dxs


def test_tower_reads_dy_once(monkeypatch):
    """the tiny tower at 64 images, pruned last layer: every full-size dY but the last layer's qkv (whose dY comes from
    attention_cls_bwd) arrives with its partials.  DCLIP_BF16_BIG_MIN = 1 puts the tower's GEMMs on the ping-pong kernel, as
    the flagship's are: the register-staged kernels have no statistics form."""
    t = wgrad_tests.tower64()
    L = t.cfg.vision.num_hidden_layers
    monkeypatch.setenv("DCLIP_BF16_BIG_MIN", "1")
    switches(monkeypatch, True)
    t.model._vsplit16_cache().clear()
    feat_s, grads_s, names_s, calls_s, bias_s, dx_s = spied_step(monkeypatch, t)
    assert calls_s == {"single": 4 * (L - 1), "three": 1}, calls_s                        # a condition, not a tolerance
    assert sum(n.startswith(SINGLE) for n in names_s) == 4 * (L - 1)
    assert sum(n.endswith(b"split_f32_f16x3_rows_colstats.cols") for n in names_s) == 1
    for site, per_layer in zip(PRODUCERS, (1, 1, 2)):
        assert sum(n.startswith(site) for n in names_s) == per_layer * (L - 1), (site, names_s)
    feat_2, grads_2, names_2, _, _, _ = spied_step(monkeypatch, t)
    assert core(names_2) == core(names_s) and same(feat_2, feat_s) and all(same(grads_2[k], grads_s[k]) for k in grads_s)   # run to run
    switches(monkeypatch, False)
    feat_o, grads_o, names_o, calls_o, bias_o, dx_o = spied_step(monkeypatch, t)
    assert calls_o == {"single": 0, "three": 4 * (L - 1) + 1}
    assert not any(n.startswith(SINGLE) or any(n.startswith(p) for p in PRODUCERS) for n in names_o)
    assert same(feat_o, feat_s)
    assert len(dx_o) == len(dx_s) == L and all(same(a, b) for a, b in zip(dx_s, dx_o))                     # dX of every layer
    lin_bias = lambda k: k.endswith(".bias") and "norm" not in k              # noqa: E731
    differ = [k for k in grads_o if not same(grads_s[k], grads_o[k])]
    assert all(lin_bias(k) for k in differ), differ                                # every weight gradient is bit-identical
    assert [b[0] for b in bias_s] == [b[0] for b in bias_o] and len(bias_s) >= 4 * (L - 1) + 1
    worst = 0.0
    for (key, rows, mag, db_s), (_, _, _, db_o) in zip(bias_s, bias_o):
        bound = schedule_checks.colsum_bound(rows, mag)
        err = (db_s.double() - db_o.double()).abs()
        assert bool((err <= bound).all()), key
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
    print(f"tiny B 64: {len(differ)} bias gradients differ, worst difference / column-sum bound {worst:.4f}")
    t.model._vsplit16_cache().clear()


def test_declined_plan_is_the_switch_off_step(monkeypatch):
    """tiny at 4 images (68 tokens, not a multiple of 64): the weight-gradient plan declines, so no producer is asked"""
    t = fwd_tests.tower("tiny")
    monkeypatch.setenv("DCLIP_BF16_BIG_MIN", "1")
    switches(monkeypatch, True)
    t.model._vsplit16_cache().clear()
    feat_s, grads_s, names_s, calls_s, _, _ = spied_step(monkeypatch, t)
    assert calls_s == {"single": 0, "three": 0}
    switches(monkeypatch, False)
    feat_o, grads_o, names_o, _, _, _ = spied_step(monkeypatch, t)
    assert core(names_s) == core(names_o)
    assert same(feat_s, feat_o) and all(same(grads_s[k], grads_o[k]) for k in grads_o)
    t.model._vsplit16_cache().clear()


def test_stale_weights_take_the_plain_backward(monkeypatch):
    from dclip_amd import engine
    from dclip_amd.clip_model import from_hf_state_dict
    t = wgrad_tests.tower64()
    monkeypatch.setenv("DCLIP_BF16_BIG_MIN", "1")
    model = from_hf_state_dict(t.cfg, t.sd, device=t.dev)
    switches(monkeypatch, True)
    monkeypatch.setattr(engine, "_VSPLIT16_WGRAD", False)
    monkeypatch.setattr(engine, "_VSPLIT16_BWD", False)
    _, grads_o, _ = t.step(model)                                       # the plain backward
    model._vsplit16_cache().clear()
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
        (_, names) = bwd_tests.launches(lambda: (feat * t.probe_dev).sum().backward())   # no device -> host read, no sync
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert not any(n.startswith(SINGLE) or any(n.startswith(p) for p in PRODUCERS) for n in names)
    stale = {k: v for k, v in fwd_tests.hf_named_grads(model).items() if k in grads_o}
    assert all(same(stale[k], grads_o[k]) for k in grads_o)


def test_graphed_step_reads_dy_once(monkeypatch):
    from dclip_amd.CLIP_image_distillation import CLIPImageDistillation
    from dclip_amd.clip_model import from_hf_state_dict
    from dclip_amd.graph import GraphedStep
    dev = torch.device("cuda:0")
    cfg = dcfg.tiny()
    B = 64
    monkeypatch.setenv("DCLIP_BF16_BIG_MIN", "1")

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
    eager, graphed = make(), make()
    g = GraphedStep(graphed, batch(10))
    for rnd_i, seed in enumerate((20, 30)):
        if rnd_i == 1:
            for mod in (eager, graphed):
                bwd_tests.change_weights(mod.student)
        (le, ge), names = bwd_tests.launches(lambda: eager_step(eager, batch(seed)))
        assert any(n.startswith(SINGLE) for n in names)
        lg = g.step(batch(seed))
        assert torch.equal(le, lg.detach()), (rnd_i, float(le), float(lg))
        gg = dict(graphed.named_parameters())
        for n, gr in ge.items():
            assert torch.equal(gr, gg[n].grad), (rnd_i, n)
        le2, ge2 = eager_step(eager, batch(seed))
        assert torch.equal(le, le2) and all(torch.equal(ge[n], ge2[n]) for n in ge)      # two runs are bit-identical
