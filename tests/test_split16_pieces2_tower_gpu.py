"""Two-piece split operands and the dropped fp32 copies at tower level.  With the plan thresholds lowered the tiny
vision tower (64 images, 64 x 17 tokens) and the frozen text tower take the fused entries at every full-size GEMM, so every
split operand becomes [hi|lo]; features and every gradient must equal the switch-off run bit for bit — also under a partial
freeze and when a watched weight's version moves between forward and backward (the backward then lands on the fp32 weight
gradients and makes the fp32 ln1 / ln2 / g again).  The forward's saved fp32 ln1 / ln2 / g are None exactly where their weight
gradient has a split plan."""
import os
import sys

import pytest
import torch

from dclip_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_vision_split16_wgrad_gpu as wgrad_tests              # noqa: E402  (tower64, switches)
import test_split16_gpu as text_tests                            # noqa: E402  (_text_model)
from test_vision_split16_gpu import hf_named_grads, same         # noqa: E402

pytestmark = pytest.mark.gpu

LOW = {"DCLIP_BF16_BIG_MIN": "1", "DCLIP_F16X3_MIN": "1", "DCLIP_F16X3_TOK_MIN": "1"}     # read per call by the plans


def setup(monkeypatch, low=True):
    from dclip_amd import engine
    wgrad_tests.switches(monkeypatch, True)
    monkeypatch.setattr(engine, "_SPLIT16_FUSED_K", True)
    monkeypatch.setattr(engine, "_SPLIT16_FUSED_TOK", True)
    for k, v in LOW.items():
        if low:
            monkeypatch.setenv(k, v)
        else:
            monkeypatch.delenv(k, raising=False)


def parts(monkeypatch, pieces2, drop32):
    from dclip_amd import engine
    monkeypatch.setattr(engine, "_SPLIT16_PIECES2", pieces2)
    monkeypatch.setattr(engine, "_VSPLIT16_DROP32", drop32)


def spy_saved(monkeypatch):
    """Collects what layer_fwd / last_layer_fwd_cls hand to the backward."""
    from dclip_amd import engine
    seen = []
    full, last = engine.layer_fwd, engine.last_layer_fwd_cls

    def layer_fwd(*a, **k):
        out = full(*a, **k)
        seen.append(("full", out[1]))
        return out

    def last_layer_fwd_cls(*a, **k):
        out = last(*a, **k)
        seen.append(("last", out[1]))
        return out

    monkeypatch.setattr(engine, "layer_fwd", layer_fwd)
    monkeypatch.setattr(engine, "last_layer_fwd_cls", last_layer_fwd_cls)
    return seen


def widths(sv):
    """pieces of each kept split operand of one layer's `saved`: width / the fp32 tensor's width"""
    x, h = sv[0], sv[11]
    ref = {"ln1": x.shape[1], "ctx": x.shape[1], "ln2": x.shape[1], "g": h.shape[1] if h is not None else None}
    return {k: v.shape[1] // ref[k] for k, v in sv[13].items()}


def test_vision_tower_bit_equal_and_saved_layout(monkeypatch):
    t = wgrad_tests.tower64()
    setup(monkeypatch)
    parts(monkeypatch, False, False)
    t.model._vsplit16_cache().clear()
    feat_o, grads_o, _ = t.step()
    seen = spy_saved(monkeypatch)
    for pieces2, drop32 in ((True, True), (True, False), (False, True)):
        parts(monkeypatch, pieces2, drop32)
        del seen[:]
        feat, grads, _ = t.step()
        assert same(feat, feat_o) and all(same(grads[k], grads_o[k]) for k in grads_o), (pieces2, drop32)
        assert len(seen) == t.cfg.vision.num_hidden_layers and seen[-1][0] == "last"
        for kind, sv in seen:
            want = 2 if pieces2 else 3
            assert all(w == want for w in widths(sv).values()), (kind, widths(sv))
            assert set(sv[13]) == ({"ln1", "ctx", "ln2", "g"} if kind == "full" else {"ln1"})
            # 64 x 17 tokens are a multiple of 64: every full-size weight gradient has a split plan
            dropped = [sv[i] is None for i in (3, 10, 12)]
            assert dropped == ([drop32] * 3 if kind == "full" else [drop32, False, False]), (kind, dropped)
            assert all(sv[i] is not None for i in (0, 1, 2, 4, 5, 6, 7, 8, 9, 11))      # x, statistics, qkv, attn, lse, x1, h stay
    # the default thresholds: no fused entry on the tiny tower, so three pieces everywhere; the fp32 copies still go where the
    # weight gradient has its split plan
    setup(monkeypatch, low=False)
    parts(monkeypatch, False, False)
    feat_p, grads_p, _ = t.step()
    parts(monkeypatch, True, True)
    del seen[:]
    feat_d, grads_d, _ = t.step()
    assert same(feat_d, feat_p) and all(same(grads_d[k], grads_p[k]) for k in grads_p)
    assert all(w == 3 for _, sv in seen for w in widths(sv).values())
    assert all(sv[3] is None for _, sv in seen)
    t.model._vsplit16_cache().clear()


def _fresh_model(t):
    from dclip_amd.clip_model import from_hf_state_dict
    return from_hf_state_dict(t.cfg, t.sd, device=t.dev)


def test_partial_freeze_bit_equal(monkeypatch):
    t = wgrad_tests.tower64()
    setup(monkeypatch)
    model = _fresh_model(t)
    frozen = [p for n, p in model.named_parameters() if "vision_model.encoder.layers.1." in n and "fc2.weight" in n]
    assert len(frozen) == 1
    frozen[0].requires_grad_(False)
    parts(monkeypatch, False, False)
    feat_o, grads_o, _ = t.step(model)
    parts(monkeypatch, True, True)
    feat, grads, _ = t.step(model)
    assert set(grads) == set(grads_o) and not any("layers.1.mlp.fc2.weight" in k for k in grads)
    assert same(feat, feat_o) and all(same(grads[k], grads_o[k]) for k in grads_o)


def test_stale_weights_rematerialise_bit_equal(monkeypatch):
    """A watched parameter's version moves between forward and backward: Split16Bwd.fresh() is false, every weight gradient is
    the fp32 GEMM, and its fp32 operand — not stored — is made again.  The gradients are the switch-off run's, bit for bit."""
    t = wgrad_tests.tower64()
    setup(monkeypatch)
    out = []
    for pieces2, drop32 in ((False, False), (True, True)):
        parts(monkeypatch, pieces2, drop32)
        model = _fresh_model(t)
        t.step(model)                                                   # (the table is built)
        for q in model.parameters():
            q.grad = None
        seen = spy_saved(monkeypatch)
        feat = model.get_image_features(pixel_values=t.pix_dev)
        assert all((sv[3] is None) == drop32 for _, sv in seen)
        with torch.no_grad():
            model.vision_model.encoder.layers[0].layer_norm1.bias.add_(0.0)          # a version bump, same values
        (feat * t.probe_dev).sum().backward()
        out.append((feat.detach().clone(), {k: v.clone() for k, v in hf_named_grads(model).items() if k in t.want_grads}))
    (feat_o, grads_o), (feat, grads) = out
    assert same(feat, feat_o) and set(grads) == set(grads_o) and all(same(grads[k], grads_o[k]) for k in grads_o)


def test_quick_gelu_rematerialisation_equals_the_epilogue():
    """ops.quick_gelu of the h32 the fc1 entry stored equals the g32 it stored beside it, bit for bit (M = 300, N = 264)."""
    from dclip_amd import ops
    dev = torch.device("cuda:0")
    M, N, K = 300, 264, 96
    g = torch.Generator().manual_seed(3)
    a3 = ops.split_f16x3((torch.randn((M, K), generator=g) * 2).to(dev), 2.0 ** 8)
    w3 = ops.split_f16x3((torch.randn((N, K), generator=g) * 0.2).to(dev), 2.0 ** 10, 1)
    bias = torch.randn((N,), generator=g).to(dev)
    alpha = torch.tensor([2.0 ** -18], dtype=torch.float32, device=dev)
    oscale = torch.tensor([2.0 ** 6], dtype=torch.float32, device=dev)
    for fused, pieces in ((True, 3), (True, 2), (False, 3)):
        h32, g32 = torch.empty((M, N), dtype=torch.float32, device=dev), torch.empty((M, N), dtype=torch.float32, device=dev)
        if fused:
            ops.gemm_f16x3_dev(a3, w3, alpha.data_ptr(), bias=bias, gelu=True, split_out_scale_ptr=oscale.data_ptr(), h32=h32, g32=g32,
                               out_pieces=pieces)
        else:
            ops.gemm_f16_dev(a3, w3, alpha.data_ptr(), bias=bias, gelu=True, split_out_scale_ptr=oscale.data_ptr(), h32=h32, g32=g32)
        assert float(h32.abs().max()) > 1.0 and bool((g32 < 0).any())
        assert torch.equal(ops.quick_gelu(h32).view(torch.int32), g32.view(torch.int32)), (fused, pieces)


@pytest.mark.parametrize("gain", [1.0, 3.0])
def test_text_tower_bit_equal(gain, monkeypatch):
    from dclip_amd import engine, ops
    dev = torch.device("cuda:0")
    monkeypatch.setattr(engine, "_SPLIT16", True)
    setup(monkeypatch)
    cfg, sd, m = text_tests._text_model(gain, dev)
    idd = synth.synth_input_ids(3, cfg.text, seed=3, ragged=True).to(dev)
    made = []
    real = ops.layernorm_fwd_f16x3

    def ln(*a, **k):
        y = real(*a, **k)
        made.append(y.shape[1] // a[0].shape[-1])
        return y

    monkeypatch.setattr(ops, "layernorm_fwd_f16x3", ln)
    with torch.no_grad():
        parts(monkeypatch, False, False)
        off = m.get_text_features(input_ids=idd)
        assert made and all(p == 3 for p in made)
        del made[:]
        parts(monkeypatch, True, True)
        on = m.get_text_features(input_ids=idd)
        assert made and all(p == 2 for p in made)
        assert torch.equal(on, off)
        setup(monkeypatch, low=False)                                   # the default thresholds: three pieces, the parent's calls
        del made[:]
        assert torch.equal(m.get_text_features(input_ids=idd), m.get_text_features(input_ids=idd)) and all(p == 3 for p in made)
