"""The fused split-fp16 GEMMs at tower level: with the plan thresholds lowered per call the tiny vision tower (64
images, 64 x 17 tokens) and the frozen text tower take the fused entries at every full-size GEMM — their launch-site names are
asserted — and features and every gradient stay within the bars of §9c-§9f against the switch-off path and the fp64 oracle;
eager and graph replay agree bit for bit.  At the default thresholds the tiny towers keep the parent's launch list."""
import argparse
import os
import sys

import pytest
import torch

from dclip_amd import config as dcfg, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_vision_split16_bwd_gpu as bwd_tests                  # noqa: E402  (launches, change_weights)
import test_vision_split16_wgrad_gpu as wgrad_tests              # noqa: E402  (Tower64, switches, grad_bars)
import test_split16_gpu as text_tests                            # noqa: E402  (_text_model)
from test_vision_split16_gpu import norm_err, same               # noqa: E402

pytestmark = pytest.mark.gpu

LOW = {"DCLIP_BF16_BIG_MIN": "1", "DCLIP_F16X3_MIN": "1", "DCLIP_F16X3_TOK_MIN": "1"}     # read per call by the plans: every eligible shape takes the twin
FUSED_K = (b"gemm_f16x3_scaled_dev.pp3", b"gemm_f16x3_scaled_split_dev.pp3", b"gemm_f16x3_scaled_rows_dev.pp3")
FUSED_TOK = b"gemm_f16x3_wgrad_tokmajor.pp3_tok.splitk_reduce"


def fused(monkeypatch, on):
    from dclip_amd import engine
    monkeypatch.setattr(engine, "_SPLIT16_FUSED_K", on)
    monkeypatch.setattr(engine, "_SPLIT16_FUSED_TOK", on)


def lower(monkeypatch, low=True):
    for k, v in LOW.items():
        if low:
            monkeypatch.setenv(k, v)
        else:
            monkeypatch.delenv(k, raising=False)


def test_vision_tower_takes_the_fused_entries(monkeypatch):
    t = wgrad_tests.tower64()
    L = t.cfg.vision.num_hidden_layers
    n_wgrad = 4 * (L - 1) + 1
    wgrad_tests.switches(monkeypatch, True)
    lower(monkeypatch)
    fused(monkeypatch, True)
    t.model._vsplit16_cache().clear()
    (feat_f, grads_f, _), names_f = bwd_tests.launches(t.step)
    assert sum(n == FUSED_TOK for n in names_f) == n_wgrad
    for site in FUSED_K:
        assert any(n == site or n == site.replace(b".pp3", b".stats.pp3") for n in names_f), site
    assert any(n == b"gemm_f16x3_scaled_rows_dev.stats.pp3" for n in names_f)                   # the statistics twin (§9g's regime)
    assert not any(n.startswith(b"gemm_f16_scaled") or n.startswith(b"gemm_f16_wgrad_tokmajor_seg3") for n in names_f)
    feat_2, grads_2, _ = t.step()
    assert same(feat_2, feat_f) and all(same(grads_2[k], grads_f[k]) for k in grads_f)          # run to run
    fused(monkeypatch, False)
    (feat_o, grads_o, _), names_o = bwd_tests.launches(t.step)
    assert not any(b"f16x3_scaled" in n or b"f16x3_wgrad" in n for n in names_o)
    assert sum(n.endswith(b"gemm_f16_wgrad_tokmajor_seg3.pp_tok_seg.splitk_reduce") for n in names_o) == n_wgrad
    core = lambda names: [n for n in names if not n.startswith(b"split16_")]      # noqa: E731  (but for the table's refresh)
    assert len(core(names_o)) == len(core(names_f))                                              # launch for launch
    d, e_f, e_o = norm_err(feat_f, feat_o), norm_err(feat_f, t.want), norm_err(feat_o, t.want)
    print(f"tiny B 64 features: fused vs off {d:.3e}; vs fp64 fused {e_f:.3e}, off {e_o:.3e}")
    assert d <= 1e-5 and e_f <= 4 * e_o
    wgrad_tests.grad_bars(t, grads_f, grads_o, "tiny B 64 fused")
    wgrad_tests.row_bars(t, grads_f, grads_o, "tiny B 64 fused")
    # each form alone
    for k_on, tok_on in ((True, False), (False, True)):
        from dclip_amd import engine
        monkeypatch.setattr(engine, "_SPLIT16_FUSED_K", k_on)
        monkeypatch.setattr(engine, "_SPLIT16_FUSED_TOK", tok_on)
        _, names = bwd_tests.launches(t.step)
        assert any(b"f16x3_scaled" in n for n in names) == k_on and any(b"f16x3_wgrad" in n for n in names) == tok_on
    # default thresholds: the tiny tower keeps the parent's entries, switch on or off
    lower(monkeypatch, False)
    fused(monkeypatch, True)
    (feat_d, grads_d, _), names_d = bwd_tests.launches(t.step)
    fused(monkeypatch, False)
    (feat_p, grads_p, _), names_p = bwd_tests.launches(t.step)
    assert names_d == names_p and not any(b"gemm_f16x3" in n for n in names_d)
    assert same(feat_d, feat_p) and all(same(grads_d[k], grads_p[k]) for k in grads_p)
    t.model._vsplit16_cache().clear()


@pytest.mark.parametrize("gain", [1.0, 3.0])
def test_text_tower_takes_the_fused_entries(gain, monkeypatch):
    from dclip_amd import engine
    from oracle import dclip_oracle as O
    dev = torch.device("cuda:0")
    monkeypatch.setattr(engine, "_SPLIT16", True)
    lower(monkeypatch)
    cfg, sd, m = text_tests._text_model(gain, dev)
    ids = synth.synth_input_ids(3, cfg.text, seed=3, ragged=True)
    idd = ids.to(dev)
    want = O.text_tower(O.to_dtype({k: v for k, v in sd.items() if k.startswith("text_")}, torch.float64), ids, cfg.text)
    with torch.no_grad():
        fused(monkeypatch, True)
        m.get_text_features(input_ids=idd)                                             # the first call splits the weights
        got, names = bwd_tests.launches(lambda: m.get_text_features(input_ids=idd))
        assert m._split16_cache()["__split16__"]["layers"] is not None
        assert any(n == b"gemm_f16x3_scaled.pp3" for n in names) and any(n == b"gemm_f16x3_scaled_split.pp3" for n in names)
        assert not any(n.startswith(b"gemm_f16_scaled") and n.endswith(b".pp") for n in names)
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
        fused(monkeypatch, False)
        off, names_o = bwd_tests.launches(lambda: m.get_text_features(input_ids=idd))
        assert not any(b"f16x3_scaled" in n for n in names_o) and len(names_o) == len(names)
        e_f, e_o, d = norm_err(got, want), norm_err(off, want), norm_err(got, off)
        print(f"text tower gain {gain}: fused vs fp64 {e_f:.3e}, unfused vs fp64 {e_o:.3e}, fused vs unfused {d:.3e}")
        assert e_f <= 1e-5 and d <= 1e-5 and e_f <= 4 * e_o


def test_graphed_step_with_fused_entries(monkeypatch):
    """The training step on the tiny towers: eager equals graph replay bit for bit, over a change of the weights too."""
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
    lower(monkeypatch)
    fused(monkeypatch, True)
    eager, graphed, off = make(), make(), make()
    g = GraphedStep(graphed, batch(10))
    for rnd_i, seed in enumerate((20, 30)):
        if rnd_i == 1:
            for mod in (eager, graphed, off):
                bwd_tests.change_weights(mod.student)
        (le, ge), names = bwd_tests.launches(lambda: eager_step(eager, batch(seed)))
        assert any(n == FUSED_TOK for n in names) and any(n in FUSED_K for n in names)
        lg = g.step(batch(seed))
        assert torch.equal(le, lg.detach()), (rnd_i, float(le), float(lg))
        gg = dict(graphed.named_parameters())
        for n, gr in ge.items():
            assert torch.equal(gr, gg[n].grad), (rnd_i, n)
        fused(monkeypatch, False)
        lo, go = eager_step(off, batch(seed))
        fused(monkeypatch, True)
        assert not all(torch.equal(ge[n], go[n]) for n in ge)            # the fused entries did run
        assert abs(float(le) - float(lo)) <= 1e-5 * abs(float(lo))
