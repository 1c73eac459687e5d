"""The 192-row tile of the fused split-fp16 GEMMs at tower level: with the plan thresholds lowered per call and the
tile forced (DCLIP_F16X3_BM192=2) the tiny vision tower (64 images, 64 x 17 tokens) and the frozen text tower take it wherever
the call's form has it — the launch sites are asserted — and features and every gradient are BIT-IDENTICAL to the 256-row tile
(DCLIP_F16X3_BM192=0): the tile height changes which workgroup owns a row, not what is added to it or in which order.  Eager and
graph replay agree bit for bit, two runs are bit-identical, and at default thresholds the tiny towers' launch list is the parent's."""
import os
import sys

import pytest
import torch

from dclip_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_split16_fused_gpu as fused_tests                     # noqa: E402  (lower, fused, LOW)
import test_vision_split16_bwd_gpu as bwd_tests                  # noqa: E402  (launches)
import test_vision_split16_wgrad_gpu as wgrad_tests              # noqa: E402  (tower64, switches)
import test_split16_gpu as text_tests                            # noqa: E402  (_text_model)
from test_vision_split16_gpu import same                         # noqa: E402

pytestmark = pytest.mark.gpu

T192 = (b"gemm_f16x3_scaled_dev.pp3_192", b"gemm_f16x3_scaled_rows_dev.pp3_192")


def core(names):
    """A launch list but for the split table's refresh (it runs in the first step after a change of the weights only)."""
    return [n for n in names if not n.startswith(b"split16_")]


def tile(monkeypatch, mode, low=True):
    """DCLIP_F16X3_BM192 = mode (None: unset) and the tile's own threshold lowered or at its default."""
    for k, v in (("DCLIP_F16X3_BM192", mode), ("DCLIP_F16X3_BM192_MIN", "1" if low else None)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)


def test_vision_tower_on_the_192_row_tile(monkeypatch):
    t = wgrad_tests.tower64()
    wgrad_tests.switches(monkeypatch, True)
    fused_tests.lower(monkeypatch)
    fused_tests.fused(monkeypatch, True)
    t.model._vsplit16_cache().clear()
    tile(monkeypatch, "2")
    t.step()                                                                                     # (the table's refresh)
    (feat_t, grads_t, _), names_t = bwd_tests.launches(t.step)
    names_t = core(names_t)
    for site in T192:
        assert any(n == site for n in names_t), site
    # the forms without the tile keep 256 rows: the split-output forward GEMMs and the statistics twin
    assert any(n == b"gemm_f16x3_scaled_split_dev.pp3" for n in names_t)
    assert any(n == b"gemm_f16x3_scaled_rows_dev.stats.pp3" for n in names_t)
    feat_2, grads_2, _ = t.step()
    assert same(feat_2, feat_t) and all(same(grads_2[k], grads_t[k]) for k in grads_t)           # run to run
    tile(monkeypatch, "0")
    (feat_p, grads_p, _), names_p = bwd_tests.launches(t.step)
    names_p = core(names_p)
    assert not any(n.endswith(b"_192") for n in names_p)
    assert [n.replace(b".pp3_192", b".pp3") for n in names_t] == names_p                         # launch for launch
    assert same(feat_t, feat_p), "features differ between the tile heights"
    assert set(grads_t) == set(grads_p)
    for k in grads_p:
        assert same(grads_t[k], grads_p[k]), f"gradient {k} differs between the tile heights"
    # by plan with the tile's threshold lowered: these few tiles fit one round at either height, so the plan takes 192 as well
    tile(monkeypatch, "1")
    _, names_1 = bwd_tests.launches(t.step)
    assert core(names_1) == names_t
    # default thresholds of the tile (the others still lowered), and all defaults: the parent's launch lists
    tile(monkeypatch, None, low=False)
    _, names_d = bwd_tests.launches(t.step)
    assert core(names_d) == names_p
    fused_tests.lower(monkeypatch, False)
    _, names_dd = bwd_tests.launches(t.step)
    tile(monkeypatch, "0", low=False)
    _, names_d0 = bwd_tests.launches(t.step)
    assert core(names_dd) == core(names_d0) and not any(b"gemm_f16x3" in n for n in names_dd)
    t.model._vsplit16_cache().clear()


def test_text_tower_on_the_192_row_tile(monkeypatch):
    from dclip_amd import engine
    dev = torch.device("cuda:0")
    monkeypatch.setattr(engine, "_SPLIT16", True)
    fused_tests.lower(monkeypatch)
    fused_tests.fused(monkeypatch, True)
    cfg, sd, m = text_tests._text_model(3.0, dev)
    idd = synth.synth_input_ids(3, cfg.text, seed=3, ragged=True).to(dev)
    with torch.no_grad():
        tile(monkeypatch, "0")
        m.get_text_features(input_ids=idd)                                             # the first call splits the weights
        want, names_p = bwd_tests.launches(lambda: m.get_text_features(input_ids=idd))
        assert not any(n.endswith(b"_192") for n in names_p)
        tile(monkeypatch, "2")
        got, names_t = bwd_tests.launches(lambda: m.get_text_features(input_ids=idd))
        assert any(n == b"gemm_f16x3_scaled.pp3_192" for n in names_t)
        assert any(n == b"gemm_f16x3_scaled_split.pp3" for n in names_t)               # no split output on the tile
        assert [n.replace(b".pp3_192", b".pp3") for n in names_t] == names_p
        assert torch.equal(got, want), "text features differ between the tile heights"
        assert torch.equal(m.get_text_features(input_ids=idd), got)                    # run to run
        side = torch.cuda.Stream(device=dev)                                           # eager == graph replay
        side.wait_stream(torch.cuda.current_stream(dev))
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                captured = m.get_text_features(input_ids=idd)
        torch.cuda.current_stream(dev).wait_stream(side)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured, got)
        tile(monkeypatch, None, low=False)
        fused_tests.lower(monkeypatch, False)
        _, names_d = bwd_tests.launches(lambda: m.get_text_features(input_ids=idd))
        assert not any(n.endswith(b"_192") for n in names_d)


def test_graphed_step_on_the_192_row_tile(monkeypatch):
    """The training step on the tiny towers with the tile forced: graph replay equals the eager step bit for bit, and both equal
    the eager step on the 256-row tile."""
    import argparse
    from dclip_amd import config as dcfg
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

    wgrad_tests.switches(monkeypatch, True)
    fused_tests.lower(monkeypatch)
    fused_tests.fused(monkeypatch, True)
    tile(monkeypatch, "2")
    eager, graphed, parent = make(), make(), make()
    g = GraphedStep(graphed, batch(10))
    (le, ge), names = bwd_tests.launches(lambda: eager_step(eager, batch(20)))
    assert any(n in T192 for n in names)
    lg = g.step(batch(20))
    assert torch.equal(le, lg.detach()), (float(le), float(lg))
    gg = dict(graphed.named_parameters())
    for n, gr in ge.items():
        assert torch.equal(gr, gg[n].grad), n
    tile(monkeypatch, "0")
    (lp, gp), names_p = bwd_tests.launches(lambda: eager_step(parent, batch(20)))
    assert not any(n.endswith(b"_192") for n in names_p)
    assert torch.equal(le, lp), (float(le), float(lp))
    for n, gr in gp.items():
        assert torch.equal(gr, ge[n]), n
