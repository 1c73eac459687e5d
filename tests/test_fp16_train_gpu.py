"""fp16 TRAINING path of the student's vision tower (student_precision="fp16", get_image_features(precision="fp16-mixed"))
and its device-side loss scaler (amp.DynamicLossScaler): the fp16 training kernels against fp64 on fp16-rounded operands,
the IEEE rounding rule (an overflow becomes inf), the scaler against torch.amp.GradScaler + torch.optim.AdamW, the step
against the fp32 step, the module against the fp32 CPU oracle, Trainer.fit with skipped steps, and two data-parallel ranks."""
import argparse
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from dclip_amd import config as dcfg, synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


# ------------------------------------------------------------------------------------------------ 1. kernels
@pytest.mark.parametrize("M,N,K", [(400, 768, 768), (13, 64, 72), (4096, 2048, 256)])
def test_gemm_f16_preact_dgelu_and_plain(M, N, K):
    """(4096, 2048) has 128 tiles of 256 x 256: the ping-pong kernel; the others the register-staged ones."""
    from dclip_amd import ops
    a = (rnd((M, K), 1) * 0.5).half().to(DEV)
    w = (rnd((N, K), 2) * 0.05).half().to(DEV)
    bias = rnd((N,), 3).to(DEV)
    ref = a.double() @ w.double().T + bias.double()
    g16, h16 = ops.gemm_f16_train(a, w, bias=bias, gelu=True, out_f16=True, save_preact=True)
    assert h16.dtype == torch.float16 and g16.dtype == torch.float16
    assert _rel(h16, ref) <= 1e-3
    hd = h16.double()
    gelu = hd * torch.sigmoid(1.702 * hd)
    assert _rel(g16, gelu) <= 1e-3
    y = ops.gemm_f16_train(a, w, bias=bias)                                   # fp32 out
    assert _rel(y, ref) <= 2e-6 * K ** 0.5
    dy = rnd((M, K), 4).half().to(DEV)
    w2 = (rnd((N, K), 5) * 0.05).half().to(DEV)              # the data-gradient GEMM's W^T operand: any [N, K] fp16 matrix
    d = ops.gemm_f16_train(dy, w2, dgelu_of=h16, out_f16=True)
    s = torch.sigmoid(1.702 * hd)
    refd = (dy.double() @ w2.double().T) * (s * (1 + 1.702 * hd * (1 - s)))
    assert _rel(d, refd) <= 1e-3


@pytest.mark.parametrize("M,N,K", [(768, 768, 12800), (768, 3072, 12800), (2304, 768, 400), (512, 768, 25600)])
def test_f16_weight_gradient_forms(M, N, K):
    """dW = dY^T X: the token-major split-K form and the transposing split-K form, both against fp64."""
    from dclip_amd import ops
    dy = rnd((K, M), 6).half().to(DEV)
    x = rnd((K, N), 7).half().to(DEV)
    ref = dy.double().T @ x.double()
    bar = 2e-6 * K ** 0.5
    got = ops.gemm_f16_wgrad_tokmajor(dy, x)
    if got is not None:
        assert _rel(got, ref) <= bar
    via_t = ops.gemm_f16_wgrad(ops.transpose_f16(dy), ops.transpose_f16(x), K)
    assert _rel(via_t, ref) <= bar


@pytest.mark.parametrize("rows,cols", [(64, 64), (85, 132), (12800, 768), (7, 8)])
def test_f16_transpose_cast_rowsum_colsum(rows, cols):
    from dclip_amd import ops
    x = rnd((rows, cols), rows + cols) * 3
    xd = x.to(DEV)
    want = x.half()
    yT = ops.transpose_f16(xd)
    assert torch.equal(yT[:, :rows].cpu(), want.T) and not yT[:, rows:].any()
    if cols % 8 == 0:
        yT2, copy = ops.transpose_f16(want.to(DEV), want_copy=True)
        assert torch.equal(copy.cpu(), want) and torch.equal(yT2.cpu(), yT.cpu())
    c = ops.cast_f16_ieee(xd)
    assert torch.equal(c[:, :cols].cpu(), want)
    rs = ops.rowsum_f16(yT, rows)
    assert _rel(rs.cpu(), want.double().sum(0)) <= 1e-5
    cs = ops.colsum_f16(want.to(DEV))
    assert _rel(cs.cpu(), want.double().sum(0)) <= 1e-5


def test_f16_layernorm_stats_and_backward_copy():
    from dclip_amd import ops
    x = rnd((300, 768), 8).to(DEV)
    g, b = (1 + 0.1 * rnd((768,), 9)).to(DEV), (0.1 * rnd((768,), 10)).to(DEV)
    y16, mean, rstd = ops.layernorm_fwd_f16_stats(x, g, b, 1e-5)
    ref = torch.nn.functional.layer_norm(x.double(), (768,), g.double(), b.double(), 1e-5)
    assert _rel(y16, ref) <= 1e-3
    y32, m32, r32 = ops.layernorm_fwd(x, g, b, 1e-5)
    assert torch.allclose(mean, m32, atol=1e-6) and torch.allclose(rstd, r32, rtol=1e-5)
    dy = rnd((300, 768), 11).to(DEV)
    dx, _dg, _db, dx16 = ops.layernorm_bwd(dy, x, g, mean, rstd, want_bf16=True, dtype16=torch.float16)
    assert dx16.dtype == torch.float16 and torch.equal(dx16.cpu(), dx.cpu().half())


def test_f16_mt_weights_equal_torch_half():
    from dclip_amd import engine
    from dclip_amd.clip_model import from_hf_state_dict
    cfg = dcfg.tiny()
    m = from_hf_state_dict(cfg, synth.synth_clip_state_dict(cfg, seed=0, gain=3.0), device=DEV)
    layers = m.vision_params().layers
    cache = {}
    engine.refresh_train_weights(cache, layers, "v", torch.float16)       # per-weight kernels, builds the table
    with torch.no_grad():
        for lp in layers:
            for _short, field in engine._TRAIN_WEIGHTS:
                getattr(lp, field).mul_(1.5)                               # all stale: the next refresh is ONE mt_weights_f16 launch
    engine.refresh_train_weights(cache, layers, "v", torch.float16)
    for li, lp in enumerate(layers):
        for short, field in engine._TRAIN_WEIGHTS:
            w = getattr(lp, field).detach()
            c, cT = cache[f"v{li}.{short}"][0], cache[f"v{li}.{short}.T"][0]
            assert c.dtype == torch.float16
            assert torch.equal(c[:, :w.shape[1]].cpu(), w.cpu().half())
            assert torch.equal(cT[:, :w.shape[0]].cpu(), w.cpu().half().T)


@pytest.mark.parametrize("B,S,H,causal", [(8, 50, 12, False), (3, 64, 2, False), (5, 17, 3, False), (4, 50, 8, True), (2, 1, 1, False),
                                          (3, 33, 2, True)])
def test_attention_f16_mfma_training_pair(B, S, H, causal):
    """fp16 twin of test_attention_bf16_mfma_training_pair, at a quarter of its bars."""
    from dclip_amd import ops
    D = 64 * H
    qkv16 = (rnd((B * S, 3 * D), 21) * 1.5).half().to(DEV)
    dout16 = rnd((B * S, D), 22).half().to(DEV)
    out16, lse = ops.attention_fwd_f16_lse(qkv16, B, S, H, causal)
    assert torch.equal(out16, ops.attention_fwd_f16_lse(qkv16, B, S, H, causal)[0])       # deterministic
    dq16 = ops.attention_bwd_f16(qkv16, out16, dout16, lse, B, S, H, causal)
    assert torch.equal(dq16, ops.attention_bwd_f16(qkv16, out16, dout16, lse, B, S, H, causal))
    x = qkv16.double().cpu().requires_grad_(True)
    q, k, v = [t.reshape(B, S, H, 64).permute(0, 2, 1, 3) for t in x.split(D, dim=1)]
    sc = q @ k.transpose(-1, -2) * 0.125
    if causal:
        sc = sc.masked_fill(torch.triu(torch.ones(S, S, dtype=torch.bool), 1), float("-inf"))
    ref = (torch.softmax(sc, -1) @ v).permute(0, 2, 1, 3).reshape(B * S, D)
    ref.backward(dout16.double().cpu())
    ref_lse = torch.logsumexp(sc, -1).reshape(B * H, S)
    assert float((lse.double().cpu() - ref_lse).abs().max()) < 5e-4
    assert float((out16.double().cpu() - ref.detach()).abs().max() / ref.detach().abs().max()) < 1.5e-2 / 4
    g, w = dq16.double().cpu(), x.grad
    for part, name in enumerate(("dq", "dk", "dv")):
        a, b_ = g[:, part * D:(part + 1) * D].reshape(-1), w[:, part * D:(part + 1) * D].reshape(-1)
        if float(b_.abs().max()) < 1e-9:          # S = 1: the softmax is constant, dq = dk = 0 exactly; the kernel leaves rounding noise
            assert float(a.abs().max()) < 1e-3 / 4, name
            continue
        cos = float(a @ b_ / (a.norm() * b_.norm()).clamp_min(1e-30))
        rel = float((a - b_).abs().max() / b_.abs().max().clamp_min(1e-30))
        assert 1 - cos < 2e-4 / 4 and rel < 3e-2 / 4, (name, cos, rel)


# ------------------------------------------------------------------------------------------------ 2. rounding rule
def test_f16_training_rounding_overflows_to_inf_frozen_saturates():
    from dclip_amd import ops
    x = torch.tensor([[1e5, -1e5, 70000.0, 1.0]], device=DEV)
    assert torch.equal(ops.cast_f16_ieee(x)[:, :4].cpu(), x.cpu().half())                 # +-inf, as (_Float16)x
    assert torch.isinf(ops.cast_f16_ieee(x)[0, :3]).all()
    assert float(ops.cast_f16(x)[0, 0]) == 65504.0 and float(ops.cast_f16(x)[0, 1]) == -65504.0
    # DGELU epilogue: dY W^T of 4e4 x 4 = 1.6e5 times gelu'(h = 1) ~ 1.07 -> inf (fp16 out)
    M, N, K = 16, 64, 64
    a = torch.full((M, K), 50.0, dtype=torch.float16, device=DEV)
    w = torch.full((N, K), 50.0, dtype=torch.float16, device=DEV)
    h = torch.ones((M, N), dtype=torch.float16, device=DEV)
    assert torch.isinf(ops.gemm_f16_train(a, w, dgelu_of=h, out_f16=True)).all()
    assert float(ops.gemm_f16(a, w, out_f16=True).float().max()) == 65504.0             # frozen entry: saturates
    # LayerNorm backward copy: dx beyond the range -> inf in the fp16 copy, finite in fp32
    xx = rnd((8, 512), 3).to(DEV)
    g, b = torch.ones(512, device=DEV), torch.zeros(512, device=DEV)
    _, mean, rstd = ops.layernorm_fwd(xx, g, b, 1e-5)
    dy = rnd((8, 512), 4).to(DEV) * 1e6
    dx, _, _, dx16 = ops.layernorm_bwd(dy, xx, g, mean, rstd, want_bf16=True, dtype16=torch.float16)
    assert torch.isfinite(dx).all() and torch.isinf(dx16).any()
    assert torch.equal(dx16.cpu(), dx.cpu().half())


def test_f16_subnormal_operands_count_in_the_product():
    from dclip_amd import ops
    M, N, K = 64, 64, 128
    a = torch.full((M, K), 1e-6).half()                                   # fp16 subnormals (min normal 6.1e-5)
    assert float(a[0, 0]) != 0.0 and float(a[0, 0]) < 6.1e-5
    w = torch.ones((N, K)).half()
    got = ops.gemm_f16_train(a.to(DEV), w.to(DEV))
    want = a.double().sum(1)[0]
    assert abs(float(got[0, 0]) - float(want)) <= 1e-6 * float(want)


# ------------------------------------------------------------------------------------------------ 3. scaler vs torch
def test_scaler_against_torch_gradscaler_and_adamw():
    from dclip_amd.amp import DynamicLossScaler
    from dclip_amd.optim import FusedAdamW
    shapes = [(64, 33), (1000,), (7,)]
    init = [rnd(s, 30 + i) for i, s in enumerate(shapes)]
    grads = [[rnd(s, 100 * t + i) * (0.3 + t) for i, s in enumerate(shapes)] for t in range(6)]
    ours = [x.clone().to(DEV).requires_grad_(True) for x in init]
    ref = [x.clone().to(DEV).requires_grad_(True) for x in init]
    opt = FusedAdamW(ours, lr=1e-2, weight_decay=1e-2, max_grad_norm=0.5)
    sc = DynamicLossScaler(init_scale=2.0 ** 16, growth_interval=2)
    topt = torch.optim.AdamW(ref, lr=1e-2, weight_decay=1e-2)
    tsc = torch.amp.GradScaler("cuda", init_scale=2.0 ** 16, growth_interval=2)
    scales, tscales = [], []
    for t in range(6):
        sc.scale(torch.ones((), device=DEV))                   # (creates the scalers' device state)
        tsc.scale(torch.ones((), device=DEV))
        s, ts = sc.get_scale(), tsc.get_scale()
        for p, q, g in zip(ours, ref, grads[t]):
            p.grad = (g * s).to(DEV)
            q.grad = (g * ts).to(DEV)
        if t in (1, 4):                                        # steps 2 and 5: an overflow
            ours[1].grad[3] = float("inf")
            ref[1].grad[3] = float("inf")
        sc.step(opt)
        sc.update()
        tsc.unscale_(topt)
        torch.nn.utils.clip_grad_norm_(ref, 0.5)
        tsc.step(topt)
        tsc.update()
        scales.append(sc.get_scale())
        tscales.append(tsc.get_scale())
    assert scales == tscales, (scales, tscales)
    st = opt.state_dict()["state"]
    for i, (p, q) in enumerate(zip(ours, ref)):
        assert _rel(p.detach(), q.detach()) <= 1e-6
        ts = topt.state[q]
        assert int(st[i]["step"]) == int(ts["step"]) == 4
        assert _rel(st[i]["exp_avg"], ts["exp_avg"]) <= 1e-6
        assert _rel(st[i]["exp_avg_sq"], ts["exp_avg_sq"]) <= 1e-6
    assert sc.state_dict()["_growth_tracker"] == tsc.state_dict()["_growth_tracker"]
    for p in ours:                                  # no gradient at all: no inf check is recorded, as torch raises
        p.grad = None
    with pytest.raises(RuntimeError, match="no inf check"):
        sc.step(opt)


# ------------------------------------------------------------------------------------------------ 4. step against fp32
def _named_grads(model):
    return {n: p.grad.detach().double().cpu().reshape(-1) for n, p in model.named_parameters() if p.grad is not None}


def _step(model, pix, ids, t_img, precision, loss_scale=1.0):
    from dclip_amd import functional
    for p in model.parameters():
        p.grad = None
    img = model.get_image_features(pixel_values=pix, precision=precision)
    with torch.no_grad():
        txt = model.get_text_features(input_ids=ids)
    loss = functional.cosine_distillation_loss(img, t_img) + functional.contrastive_loss(img, txt)
    (loss * loss_scale).backward()
    g = _named_grads(model)
    return float(loss.detach()), img.detach().clone(), {k: v / loss_scale for k, v in g.items()}


# gates (where the measured values are recorded): 3x the values measured on one MI355X, capped by the bars
# of the feature — embedding max-rel 1e-3 and a third of bf16's (3x the measured embedding error is above 1e-3 for every
# config, so the cap is the gate), loss 1e-4 relative.  The tiny model's loss is the one gate above 1e-4: measured 1.0004e-4
# (bf16 2.4e-4), recorded in §13b as a deviation.  (loss rel, 1 - min gradient cosine, max |gradient norm ratio - 1|)
@pytest.mark.parametrize("name,mk,B,gates", [("tiny", dcfg.tiny, 6, (3e-4, 1e-5, 1.5e-3)),
                                             ("ViT-B/32", dcfg.vit_b32, 8, (9e-5, 1e-5, 1e-3)),
                                             ("ViT-B/32", dcfg.vit_b32, 256, (1e-5, 5e-6, 1e-3)),
                                             ("ViT-B/16", dcfg.vit_b16, 4, (5e-5, 1.5e-5, 2e-3))])
def test_f16_training_step_against_fp32(name, mk, B, gates):
    """The fp16 step (loss scaled by 2^10 as the scaler would) against the exact fp32 step on the same weights and batch.
    tiny / B/32 at 8 take the transposing schedule, B/32 at 256 the token-major one, B/16 (197 tokens) the fp32 attention
    core with fp16 casts around it."""
    from dclip_amd.clip_model import from_hf_state_dict
    cfg = mk()
    m = from_hf_state_dict(cfg, synth.synth_clip_state_dict(cfg, seed=0, gain=3.0), device=DEV)
    for p in m.text_model.parameters():
        p.requires_grad = False
    m.text_projection.weight.requires_grad = False
    m.logit_scale.requires_grad = False
    pix = synth.synth_pixel_values(B, cfg.vision, seed=0).to(DEV)
    ids = synth.synth_input_ids(B, cfg.text, seed=3, ragged=True).to(DEV)
    t_img = synth.synth_embeddings(B, cfg.projection_dim, seed=1).to(DEV)
    l32, e32, g32 = _step(m, pix, ids, t_img, "fp32")
    l16, e16, g16 = _step(m, pix, ids, t_img, "fp16-mixed", 1024.0)
    l16b, e16b, g16b = _step(m, pix, ids, t_img, "fp16-mixed", 1024.0)
    lb, eb, _ = _step(m, pix, ids, t_img, "bf16")
    assert l16 == l16b and torch.equal(e16, e16b) and all(torch.equal(g16[k], g16b[k]) for k in g16)     # bit-identical
    assert set(g16) == set(g32)
    cos = {k: float(g16[k] @ g32[k] / (g16[k].norm() * g32[k].norm()).clamp_min(1e-30)) for k in g32}
    nrm = {k: float(g16[k].norm() / g32[k].norm().clamp_min(1e-30)) for k in g32}
    emb_rel, emb_rel_bf16 = _rel(e16, e32), _rel(eb, e32)
    loss_rel = abs(l16 - l32) / abs(l32)
    print(f"[{name} B={B}] fp16 embedding max rel {emb_rel:.2e} (bf16 {emb_rel_bf16:.2e}); loss rel {loss_rel:.2e} "
          f"(bf16 {abs(lb - l32) / abs(l32):.2e}); grad cosine min {min(cos.values()):.6f}; norm ratio "
          f"{min(nrm.values()):.4f}..{max(nrm.values()):.4f}")
    g_loss, g_cos, g_nrm = gates
    assert emb_rel <= 1e-3 and emb_rel <= emb_rel_bf16 / 3
    assert loss_rel <= g_loss
    assert 1 - min(cos.values()) <= g_cos
    assert 1 - g_nrm <= min(nrm.values()) and max(nrm.values()) <= 1 + g_nrm


# ------------------------------------------------------------------------------------------------ 5. module vs oracle
def test_f16_student_c3_step_vs_oracle_and_one_scaled_step_lowers_the_loss():
    from dclip_amd.amp import DynamicLossScaler
    from dclip_amd.clip_model import from_hf_state_dict
    from dclip_amd.CLIP_image_distillation import CLIPImageDistillation
    from dclip_amd.optim import FusedAdamW
    from oracle import dclip_oracle as O
    cfg = dcfg.vit_b32()
    sd = synth.synth_clip_state_dict(cfg, seed=0, gain=3.0)
    student = from_hf_state_dict(cfg, sd, device=DEV)
    hp = argparse.Namespace(learning_rate=1e-4, warmup_steps=0, total_steps=10, train_batch_size=4, eval_batch_size=4)
    mod = CLIPImageDistillation(hp, student, None, freeze_mode="north_star", student_precision="fp16").to(DEV)
    B = 4
    pix = synth.synth_pixel_values(B, cfg.vision, seed=0)
    ids = synth.synth_input_ids(B, cfg.text, seed=3, ragged=True, min_len=8)
    t_img = synth.synth_embeddings(B, cfg.projection_dim, seed=1)
    batch = {"pixel_values": pix.to(DEV), "input_ids": ids.to(DEV), "teacher_image_emb": t_img.to(DEV)}
    with torch.no_grad():
        ref = O.distill_step(sd, cfg, pix, ids, t_img)
    img = mod.student.get_image_features(pixel_values=pix.to(DEV), precision="fp16-mixed")     # grad on: the training kernels
    assert img.requires_grad
    assert _rel(img.detach().cpu(), ref["image_emb"]) <= 1e-3
    del img
    loss = mod.training_step(batch)
    got, want = float(loss.detach()), float(ref["loss"])
    print(f"c3-shaped fp16 student step: loss {got:.6f} vs fp32 oracle {want:.6f} (rel {abs(got - want) / abs(want):.2e})")
    assert abs(got - want) <= 1e-3 * abs(want)
    opt = FusedAdamW([p for p in mod.parameters() if p.requires_grad], lr=1e-3, max_grad_norm=0.5)
    sc = DynamicLossScaler()
    sc.scale(loss).backward()
    sc.step(opt)
    sc.update()
    assert float(sc.found_inf()) == 0.0
    opt.zero_grad(set_to_none=True)
    assert float(mod.training_step(batch).detach()) < got


# ------------------------------------------------------------------------------------------------ 6. Trainer
class _RecordingScaler:
    """DynamicLossScaler that records the scale after every update (a host read: tests only)."""

    def __new__(cls, **kw):
        from dclip_amd.amp import DynamicLossScaler

        class R(DynamicLossScaler):
            def update(self):
                super().update()
                self.history.append(self.get_scale())
        r = R(**kw)
        r.history = []
        return r


def _tiny_module(dev, group=None, lr=1e-3):
    from dclip_amd.clip_model import from_hf_state_dict
    from dclip_amd.CLIP_image_distillation import CLIPImageDistillation
    from dclip_amd.patch_text_aggregation import PatchTextAggregation
    cfg = dcfg.tiny()
    student = from_hf_state_dict(cfg, synth.synth_clip_state_dict(cfg, seed=7, gain=4.0), device=dev)
    teacher = PatchTextAggregation(embed_dim=cfg.projection_dim, num_heads=1, clip_model=student).to(dev)
    hp = argparse.Namespace(learning_rate=lr, warmup_steps=0, total_steps=100, train_batch_size=4, eval_batch_size=4)
    return cfg, CLIPImageDistillation(hp, student, None, teacher=teacher, freeze_mode="north_star", process_group=group,
                                      student_precision="fp16").to(dev)


def _batches(cfg, n, B):
    return [{"pixel_values": synth.synth_pixel_values(B, cfg.vision, seed=i),
             "input_ids": synth.synth_input_ids(B, cfg.text, seed=100 + i, ragged=True),
             "teacher_image_emb": synth.synth_embeddings(B, cfg.projection_dim, seed=200 + i),
             "teacher_text_emb": synth.synth_embeddings(B, cfg.projection_dim, seed=300 + i)} for i in range(n)]


def test_trainer_fp16_skips_overflowing_steps_then_trains(tmp_path):
    from dclip_amd.lightning_lite import Trainer
    cfg, mod = _tiny_module(DEV)
    params0 = {n: p.detach().clone() for n, p in mod.named_parameters() if p.requires_grad}
    sc = _RecordingScaler(init_scale=2.0 ** 40)
    data = _batches(cfg, 40, 4)
    Trainer(max_epochs=1, accumulate_grad_batches=1, gradient_clip_val=0.5, max_steps=1, loss_scaler=sc).fit(mod, data[:1], None)
    assert sc.history == [2.0 ** 39]                               # the first step overflowed: skipped, scale backed off
    assert all(torch.equal(p.detach(), params0[n]) for n, p in mod.named_parameters() if p.requires_grad)
    tr = Trainer(max_epochs=1, accumulate_grad_batches=1, gradient_clip_val=0.5, checkpoint_dir=str(tmp_path), loss_scaler=sc)
    tr.fit(mod, data, None)
    skipped = sum(1 for a, b in zip([2.0 ** 40] + sc.history, sc.history) if b < a)
    print(f"scales {sc.history[:3]} ... {sc.history[-3:]}, {skipped} skipped of {len(sc.history)}")
    assert sc.history[-1] < 2.0 ** 20 and skipped < len(sc.history) - 5       # the scale came down and training went on
    assert mod.global_step == 40 and torch.isfinite(torch.tensor(mod.logged("train_loss")))
    assert any(not torch.equal(p.detach(), params0[n]) for n, p in mod.named_parameters() if p.requires_grad)
    assert all(torch.isfinite(p).all() for p in mod.parameters())
    with torch.serialization.safe_globals([argparse.Namespace]):
        ck = torch.load(tr.saved[0][1], map_location="cpu", weights_only=True)
    assert ck["native_amp_scaling_state"]["scale"] == sc.get_scale()
    assert ck["native_amp_scaling_state"]["growth_interval"] == 2000


# ------------------------------------------------------------------------------------------------ 7. data parallel
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


# Adam's first update is ~lr x sign(g): where a gradient element is near zero, the summation order of the all-reduce can flip it
# and move the weight by 2 lr, and the steps after that see slightly different weights.  So the comparison stops at the first
# step the scaler lets through: the weights within the 1e-4 bar (a small learning rate), and — the check with teeth — the Adam
# moments, which after that one step are the clipped all-reduced gradients (1e-4 of each tensor's largest; 2e-4 squared).
DP_LR = 1e-5
DP_MAX_STEPS = 40


def _fit_keeping_optimizer(trainer, mod, batches):
    """Trainer.fit, returning the optimizer the module's configure_optimizers made (its moments are compared)."""
    box = {}
    conf = mod.configure_optimizers

    def keep():
        opts, scheds = conf()
        box["opt"] = opts[0]
        return opts, scheds
    mod.configure_optimizers = keep
    trainer.fit(mod, batches, None)
    return box["opt"]


def _moments(opt):
    st = opt.state_dict()["state"]
    return {i: (int(v["step"]), v["exp_avg"].detach().cpu(), v["exp_avg_sq"].detach().cpu()) for i, v in st.items()}


def _dp_worker(rank, world, port, n_steps, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from dclip_amd.lightning_lite import Trainer
    cfg, mod = _tiny_module(DEV, dist.group.WORLD, DP_LR)
    sc = _RecordingScaler(init_scale=2.0 ** 40)
    opt = _fit_keeping_optimizer(Trainer(max_epochs=1, accumulate_grad_batches=1, gradient_clip_val=0.5, process_group=dist.group.WORLD,
                                         bucket_mb=0.05, loss_scaler=sc), mod, _batches(cfg, 2 * n_steps, 2))
    torch.cuda.synchronize()
    out[rank] = dict(scales=list(sc.history), params={n: p.detach().cpu() for n, p in mod.named_parameters() if p.requires_grad},
                     moments=_moments(opt))
    dist.barrier()
    dist.destroy_process_group()


def _single(n_steps):
    from dclip_amd.lightning_lite import Trainer
    cfg, mod = _tiny_module(DEV, None, DP_LR)
    params0 = {n: p.detach().cpu().clone() for n, p in mod.named_parameters() if p.requires_grad}
    per_rank = _batches(cfg, 2 * n_steps, 2)
    joined = [{k: torch.cat([per_rank[2 * i][k], per_rank[2 * i + 1][k]]) for k in per_rank[0]} for i in range(n_steps)]
    sc = _RecordingScaler(init_scale=2.0 ** 40)
    opt = _fit_keeping_optimizer(Trainer(max_epochs=1, accumulate_grad_batches=1, gradient_clip_val=0.5, loss_scaler=sc), mod,
                                 joined)
    return mod, params0, sc.history, opt


def test_two_ranks_fp16_equal_single_process():
    world = 2
    # where does the single process take its first step?  (from 2^40 the scale backs off ~20 times first)
    _m, _p0, history, _o = _single(DP_MAX_STEPS)
    first = next(i for i, (a, b) in enumerate(zip([2.0 ** 40] + history, history)) if b >= a)
    n_steps = first + 1                                  # every step skipped but the last
    mod, params0, history, opt = _single(n_steps)
    assert len(history) == n_steps and history[-1] == history[-2] and all(b < a for a, b in zip(history[:-2], history[1:-1]))
    params = {n: p.detach().cpu() for n, p in mod.named_parameters() if p.requires_grad}
    moments = _moments(opt)
    assert all(st == 1 for st, _, _ in moments.values())                      # Adam counted the one taken step only
    assert any(not torch.equal(p, params0[n]) for n, p in params.items())    # ... which moved the weights
    out = mp.Manager().dict()
    mp.spawn(_dp_worker, args=(world, _free_port(), n_steps, out), nprocs=world, join=True)
    for r in range(world):
        assert out[r]["scales"] == history
        for n, p in params.items():
            assert float((out[r]["params"][n] - p).abs().max()) <= 1e-4 * float(p.abs().max()), n
        assert set(out[r]["moments"]) == set(moments)
        for i, (st, m, v) in moments.items():
            rst, rm, rv = out[r]["moments"][i]
            assert rst == st
            assert float((rm - m).abs().max()) <= 1e-4 * float(m.abs().max()), ("exp_avg", i)
            assert float((rv - v).abs().max()) <= 2e-4 * float(v.abs().max()), ("exp_avg_sq", i)
