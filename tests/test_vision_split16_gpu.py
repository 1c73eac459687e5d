"""Split-fp16 forward of the student's vision tower with its plan on the device: the plan against the host
rules, the device-scaled kernels against their scalar twins, the multi-tensor weight split, and the tower against the plain
fp32 path and the fp64 oracle — eager, with changing weights, under a HIP graph, and with the guard tripped."""
import argparse
import logging
import math

import pytest
import torch

from dclip_amd import config as dcfg, synth

pytestmark = pytest.mark.gpu

WEIGHTS = ("qkv", "out", "fc1", "fc2")
ACTS = ("ln1", "ctx", "ln2", "g")
ACT_OF = {"qkv": "ln1", "out": "ctx", "fc1": "ln2", "fc2": "g"}


def rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


def norm_err(got, want):
    return float((got.detach().double().cpu() - want.detach().double().cpu()).abs().max() / want.detach().abs().max().clamp_min(1e-300))


def scalar(v, dev):
    return torch.tensor([v], dtype=torch.float32, device=dev)


# ------------------------------------------------------------------------------------------------ 1. plan on the device

def crafted_layer(seed, D=72, I=40):
    return {"ln1_w": 1.0 + rnd((D,), seed, 0.2), "ln1_b": rnd((D,), seed + 1, 0.1), "qkv_w": rnd((3 * D, D), seed + 2, 0.08),
            "qkv_b": rnd((3 * D,), seed + 3, 0.1), "out_w": rnd((D, D), seed + 4, 0.05), "ln2_w": 1.0 + rnd((D,), seed + 5, 0.2),
            "ln2_b": rnd((D,), seed + 6, 0.1), "fc1_w": rnd((I, D), seed + 7, 0.09), "fc1_b": rnd((I,), seed + 8, 0.1),
            "fc2_w": rnd((D, I), seed + 9, 0.03)}


def crafted_layers():
    """random | an all-zero weight | a bound that is a power of two | gamma = 1e7 (e < -14) | one infinite weight"""
    L = [crafted_layer(100 * i) for i in range(5)]
    L[1]["fc2_w"].zero_()
    L[2]["ln1_w"].zero_()
    L[2]["ln1_b"].zero_()
    L[2]["ln1_b"][5] = -0.5
    L[3]["ln2_w"].fill_(1e7)
    L[4]["fc1_w"][7, 3] = float("inf")
    return L


def torch_stats(L, D):
    wv, bv = L["qkv_w"][2 * D:], L["qkv_b"][2 * D:]
    return [L["ln1_w"].abs().max(), L["ln1_b"].abs().max(), wv.abs().sum(1).max(), bv.abs().max(), L["ln2_w"].abs().max(),
            L["ln2_b"].abs().max(), L["fc1_w"].abs().sum(1).max(), L["fc1_b"].abs().max(), L["qkv_w"].abs().max(),
            L["out_w"].abs().max(), L["fc1_w"].abs().max(), L["fc2_w"].abs().max()]


@pytest.fixture(scope="module")
def planned():
    from dclip_amd import ops
    dev = torch.device("cuda:0")
    host = crafted_layers()
    layers = [{k: v.to(dev) for k, v in L.items()} for L in host]
    tab = ops.split16_table(layers)
    ops.split16_refresh(tab)
    first = tab["plan"].cpu().clone()
    ops.split16_refresh(tab)                                       # the plan launch cleared the accumulators: same again
    torch.cuda.synchronize()
    return host, layers, tab, first


def f32(v):
    return torch.tensor(v, dtype=torch.float32)


def test_device_plan_equals_host_rules(planned):
    from dclip_amd import engine, ops
    host, layers, tab, first = planned
    plan = tab["plan"].cpu()
    assert same(plan, first), "two runs of the statistics / plan launches differ"
    assert int(tab["stats"].abs().sum()) == 0
    D = 72
    flags = plan[:, ops.SPLIT16_PLAN_FLAGS].view(torch.int32).tolist()
    assert flags == [0, 0, 0, 1, 2]
    for li, L in enumerate(host):
        got = plan[li, ops.SPLIT16_PLAN_STATS:ops.SPLIT16_PLAN_STATS + 12]
        want = torch.stack(torch_stats(L, D))
        fin = torch.isfinite(want)
        assert bool(torch.equal(torch.isfinite(got), fin)), li
        assert float(((got[fin] - want[fin]).abs() / want[fin].abs().clamp_min(1e-30)).max()) <= 1e-6, li
        st = dict(zip(ops.SPLIT16_STATS, (float(v) for v in got.double())))          # the device's own statistics
        ref = engine.split16_plan_host(st, D)
        assert ref["flags"] == flags[li], li
        for a in ACTS:
            assert same(plan[li, ops.SPLIT16_PLAN_ACT[a]], f32(2.0 ** ref["e"][a])), (li, a, float(plan[li, ops.SPLIT16_PLAN_ACT[a]]))
        for w in WEIGHTS:
            assert same(plan[li, ops.SPLIT16_PLAN_W[w]], f32(2.0 ** ref["f"][w])), (li, w)
            assert same(plan[li, ops.SPLIT16_PLAN_ALPHA[w]], f32(2.0 ** ref["a"][w])), (li, w)
        if flags[li] == 0:                                                             # and the host guard agrees where it applies
            b = engine.split16_layer_bounds(st, D)
            assert ref["e"] == {k: engine.split16_act_exp(v) for k, v in b.items()}
    assert float(plan[1, ops.SPLIT16_PLAN_W["fc2"]]) == 1.0                           # all-zero weight: f = 0
    assert float(plan[2, ops.SPLIT16_PLAN_ACT["ln1"]]) == 2.0 ** 15                   # bound 0.5 exactly: 0.5 * 2^15 = 2^14
    assert float(plan[3, ops.SPLIT16_PLAN_ACT["g"]]) < 2.0 ** -14


# ------------------------------------------------------------------------------------------------ 3. multi-tensor weight split

def test_multi_tensor_weight_split(planned):
    from dclip_amd import ops
    host, layers, tab, _ = planned
    plan = tab["plan"].cpu()
    shapes = set()
    for li in (0, 1, 3):
        for w in WEIGHTS:
            src = layers[li][w + "_w"]
            shapes.add(tuple(src.shape))
            want = ops.split_f16x3(src, float(plan[li, ops.SPLIT16_PLAN_W[w]]), 1)
            assert same(tab["w"][li][w], want), (li, w)
    assert len(shapes) >= 3


# ------------------------------------------------------------------------------------------------ 2. device-scaled kernels

@pytest.mark.parametrize("rows,cols", [(5, 72), (130, 512)])
def test_split_dev_equals_scalar(rows, cols):
    from dclip_amd import ops
    dev = torch.device("cuda:0")
    x = rnd((rows, cols), rows + cols, 30.0).to(dev)
    for sc in (2.0 ** -3, 2.0 ** 7):
        s = scalar(sc, dev)
        for order in (0, 1):
            assert same(ops.split_f16x3_dev(x, s.data_ptr(), order), ops.split_f16x3(x, sc, order)), (sc, order)


@pytest.mark.parametrize("D", [72, 512, 768])
def test_layernorm_dev_equals_scalar_and_plain(D):
    from dclip_amd import ops
    dev = torch.device("cuda:0")
    rows, eps, sc = 5, 1e-5, 2.0 ** 4
    x = (rnd((rows, D), D, 3.0) + 1.0).to(dev)
    g, b = (1.0 + rnd((D,), D + 1, 0.3)).to(dev), rnd((D,), D + 2, 0.2).to(dev)
    s = scalar(sc, dev)
    ln, mean, rstd = ops.layernorm_fwd(x, g, b, eps, save_stats=True)
    y3, y, m, r = ops.layernorm_fwd_f16x3_dev(x, g, b, eps, s.data_ptr(), save=True)
    assert same(y3, ops.layernorm_fwd_f16x3(x, g, b, eps, sc))
    assert same(y, ln) and same(m, mean) and same(r, rstd)
    assert same(y3, ops.split_f16x3(y, sc, 0))
    y3n, yn, mn, rn = ops.layernorm_fwd_f16x3_dev(x, g, b, eps, s.data_ptr(), save=False)
    assert same(y3n, y3) and yn is None and mn is None and rn is None


def check_dev_gemm(M, N, K):
    """Every form of the device-scaled GEMM against its scalar twin at the same scales, bit for bit, on whichever kernel the
    dispatcher picks for the shape under the switches that are set."""
    from dclip_amd import ops
    dev = torch.device("cuda:0")
    a16, w16 = rnd((M, K), 1).half().to(dev), rnd((N, K), 2, 0.1).half().to(dev)
    bias, res = rnd((N,), 3).to(dev), rnd((M, N), 4).to(dev)
    al, so = 2.0 ** -5, 2.0 ** 3
    ap, sp = scalar(al, dev), scalar(so, dev)
    for kw in (dict(), dict(bias=bias), dict(bias=bias, residual=res), dict(bias=bias, gelu=True), dict(bias=bias, gelu=True, out_f16=True),
               dict(bias=bias, out_f16=True)):
        assert same(ops.gemm_f16_dev(a16, w16, ap.data_ptr(), **kw), ops.gemm_f16(a16, w16, k=K, alpha=al, **kw)), (M, N, K, kw)
    for kw in (dict(), dict(bias=bias), dict(bias=bias, gelu=True)):
        want = ops.gemm_f16(a16, w16, k=K, alpha=al, split_out_scale=so, **kw)
        assert same(ops.gemm_f16_dev(a16, w16, ap.data_ptr(), split_out_scale_ptr=sp.data_ptr(), **kw), want), (M, N, K, kw)
        g = torch.full((M, N), 7.0, dtype=torch.float32, device=dev)
        assert same(ops.gemm_f16_dev(a16, w16, ap.data_ptr(), split_out_scale_ptr=sp.data_ptr(), g32=g, **kw), want)
        assert same(g, ops.gemm_f16(a16, w16, k=K, alpha=al, **kw)), (M, N, K, kw)
    if N % 8:
        return
    # fc1 of a training forward: h, g = quick_gelu(h) and the split of g from one launch; and the two-launch form
    h_want = ops.gemm_f16(a16, w16, k=K, alpha=al, bias=bias)
    g_want = ops.gemm_f16(a16, w16, k=K, alpha=al, bias=bias, gelu=True)
    h = torch.full((M, N), 7.0, dtype=torch.float32, device=dev)
    g = torch.full((M, N), 7.0, dtype=torch.float32, device=dev)
    g3 = ops.gemm_f16_dev(a16, w16, ap.data_ptr(), bias=bias, gelu=True, split_out_scale_ptr=sp.data_ptr(), h32=h, g32=g)
    assert same(h, h_want) and same(g, g_want) and same(g3, ops.split_f16x3(g_want, so, 0)), (M, N, K)
    h2 = torch.full((M, N), 7.0, dtype=torch.float32, device=dev)
    g2 = ops.gemm_f16_dev(a16, w16, ap.data_ptr(), bias=bias, gelu=True, h32=h2)
    assert same(h2, h_want) and same(g2, g_want), (M, N, K)


# (130, 72, 40), (231, 1536, 512): the register-staged 64x64 kernel; (2048, 2048, 64): the register-staged 128x128 kernel;
# (2816, 3072, 64): 132 tiles of 256x256, the ping-pong kernel the tower's GEMMs run on
@pytest.mark.parametrize("M,N,K", [(130, 72, 40), (231, 1536, 512), (2048, 2048, 64), (2816, 3072, 64)])
def test_gemm_dev_equals_scalar(M, N, K):
    check_dev_gemm(M, N, K)


def test_gemm_dev_never_takes_the_persistent_kernel(monkeypatch):
    """Past the persistent kernel's threshold (576 tiles) the device-scaled forms stay on the one-tile ping-pong kernel."""
    from dclip_amd import _lib
    monkeypatch.setenv("DCLIP_BF16_PERSIST", "1")
    check_dev_gemm(5900, 6144, 64)
    assert b".ppp" not in _lib.load().dclip_last_launch()


# ------------------------------------------------------------------------------------------------ 4. tower

def vision_keys(sd):
    return {k: v for k, v in sd.items() if k.startswith("vision_model.") or k.startswith("visual_projection")}


def hf_named_grads(model):
    out = {}
    for k, p in model.named_parameters():
        if p.grad is None:
            continue
        if "qkv_proj" in k:
            D = p.grad.shape[0] // 3
            for i, n in enumerate(("q_proj", "k_proj", "v_proj")):
                out[k.replace("qkv_proj", n)] = p.grad[i * D:(i + 1) * D]
        else:
            out[k] = p.grad
    return out


class Tower:
    """One configuration: model, inputs, the fp64 oracle (computed once), and the plain-path step."""

    def __init__(self, name):
        from dclip_amd.clip_model import from_hf_state_dict
        from oracle import dclip_oracle as O
        self.dev = torch.device("cuda:0")
        self.cfg = dcfg.tiny() if name == "tiny" else dcfg.vit_b32()
        self.B = 4 if name == "tiny" else 2
        self.sd = synth.synth_clip_state_dict(self.cfg, seed=5, gain=2.0)
        self.pix = synth.synth_pixel_values(self.B, self.cfg.vision, seed=1)
        self.probe = rnd((self.B, self.cfg.projection_dim), 9)
        self.model = from_hf_state_dict(self.cfg, self.sd, device=self.dev)
        self.pix_dev, self.probe_dev = self.pix.to(self.dev), self.probe.to(self.dev)
        p = {k: v.double().requires_grad_(True) for k, v in vision_keys(self.sd).items()}
        feat = O.vision_tower(p, self.pix.double(), self.cfg.vision)
        (feat * self.probe.double()).sum().backward()
        self.want, self.want_grads = feat.detach(), {k: v.grad for k, v in p.items()}

    def step(self, model=None):
        """features and parameter gradients (HF keys) of one gradient-enabled forward + backward; nothing here touches the host"""
        m = model or self.model
        for q in m.parameters():
            q.grad = None
        feat = m.get_image_features(pixel_values=self.pix_dev)
        (feat * self.probe_dev).sum().backward()
        return feat.detach().clone(), {k: v.clone() for k, v in hf_named_grads(m).items() if k in self.want_grads}, None


_TOWERS = {}


def tower(name):
    if name not in _TOWERS:
        _TOWERS[name] = Tower(name)
    return _TOWERS[name]


def within_bars(t, feat, grads, feat_plain, grads_plain, tag, want=None, want_grads=None):
    """The project's bars: features within 1e-5 of the plain path norm-wise; against fp64, features and every parameter
    gradient at most 4x the plain path's own error."""
    want = t.want if want is None else want
    want_grads = t.want_grads if want_grads is None else want_grads
    d = norm_err(feat, feat_plain)
    es, ep = norm_err(feat, want), norm_err(feat_plain, want)
    print(f"{tag}: features split vs plain {d:.3e}; vs fp64 split {es:.3e} plain {ep:.3e} ratio {es / ep:.2f}")
    worst = (0.0, None)
    bad = []
    for k, w in want_grads.items():
        # a key bias shifts every logit of a row by the same amount and softmax does not see it: its gradient is zero in exact
        # arithmetic, what either path returns for it is rounding noise, and a ratio of two noises measures nothing
        if float(w.abs().max()) == 0.0 or k.endswith("k_proj.bias"):
            continue
        gs, gp = norm_err(grads[k].reshape(w.shape), w), norm_err(grads_plain[k].reshape(w.shape), w)
        if gs / gp > worst[0]:
            worst = (gs / gp, k)
        if gs > 4 * gp:
            bad.append((k, gs, gp))
    print(f"{tag}: worst gradient ratio split/plain vs fp64 {worst[0]:.2f} ({worst[1]})")
    assert d <= 1e-5, (tag, d)
    assert es <= 4 * ep, (tag, es, ep)
    assert not bad, (tag, bad)


def saved_layer0(model, t):
    from dclip_amd import engine
    p = model.vision_params()
    pd = engine.VisionParams.from_tensors([x.detach() for x in p.tensors()], t.cfg.vision.num_hidden_layers)
    return pd


@pytest.mark.parametrize("name", ["tiny", "vit_b32"])
def test_tower_split_against_plain_and_fp64(name, monkeypatch):
    from dclip_amd import engine
    t = tower(name)
    v = t.cfg.vision
    monkeypatch.setattr(engine, "_VSPLIT16", False)
    feat_p, grads_p, _ = t.step()
    with torch.no_grad():
        ev_p = t.model.get_image_features(pixel_values=t.pix_dev)
    pd = saved_layer0(t.model, t)
    _, sv_p = engine.vision_fwd(pd, t.pix_dev, v, True)
    monkeypatch.setattr(engine, "_VSPLIT16", True)
    feat_s, grads_s, _ = t.step()
    ent = t.model._vsplit16_cache().get("__vsplit16__")
    assert ent is not None and len(ent["layers"]) == v.num_hidden_layers                     # the split path did run
    assert not torch.equal(feat_s, feat_p)
    within_bars(t, feat_s, grads_s, feat_p, grads_p, name)
    _, sv_s = engine.vision_fwd(pd, t.pix_dev, v, True, split16_cache=t.model._vsplit16_cache())
    x, m1, r1 = sv_s[4][0][:3]
    xp, m1p, r1p = sv_p[4][0][:3]
    assert same(x, xp) and same(m1, m1p) and same(r1, r1p)
    assert same(sv_s[4][0][3], sv_p[4][0][3])                                                # fp32 ln1 of layer 0 too
    assert all(a.dtype == torch.float32 for a in sv_s[4][0] if a is not None)
    # run to run, and the two fc1 forms
    feat_2, grads_2, _ = t.step()
    assert same(feat_2, feat_s) and all(same(grads_2[k], grads_s[k]) for k in grads_s)
    monkeypatch.setattr(engine, "_VSPLIT16_FC1_EPI", not engine._VSPLIT16_FC1_EPI)
    feat_3, grads_3, _ = t.step()
    assert same(feat_3, feat_s) and all(same(grads_3[k], grads_s[k]) for k in grads_s)
    # a no-grad forward stays on the plain path: what it gave with the switch off, bit for bit
    with torch.no_grad():
        ev = t.model.get_image_features(pixel_values=t.pix_dev)
    assert same(ev, ev_p)


# ------------------------------------------------------------------------------------------------ 5. nothing baked in

def scale_weights(model):
    with torch.no_grad():
        for layer in model.vision_model.encoder.layers:
            for n, p in layer.named_parameters():
                if n.endswith("weight") and p.dim() == 2:
                    p.mul_(8.0)
                elif "layer_norm" in n and n.endswith("weight"):
                    p.fill_(50.0)


def oracle_for(t, model):
    """fp64 features and gradients of the model's CURRENT weights."""
    from oracle import dclip_oracle as O
    sd = {}
    for k, p in model.state_dict().items():
        sd[k] = p.detach().cpu()
    hf = {}
    for k, v in sd.items():
        if "qkv_proj" in k:
            D = v.shape[0] // 3
            for i, n in enumerate(("q_proj", "k_proj", "v_proj")):
                hf[k.replace("qkv_proj", n)] = v[i * D:(i + 1) * D]
        else:
            hf[k] = v
    p = {k: v.double().clone().requires_grad_(True) for k, v in vision_keys(hf).items()}
    feat = O.vision_tower(p, t.pix.double(), t.cfg.vision)
    (feat * t.probe.double()).sum().backward()
    return feat.detach(), {k: v.grad for k, v in p.items()}


def test_changed_weights_are_replanned_without_a_host_read(monkeypatch):
    from dclip_amd import engine
    from dclip_amd.clip_model import from_hf_state_dict
    t = tower("tiny")
    model = from_hf_state_dict(t.cfg, t.sd, device=t.dev)
    monkeypatch.setattr(engine, "_VSPLIT16", True)
    t.step(model)                                                           # builds the table (one upload), plans, splits
    plan_before = model._vsplit16_cache()["__vsplit16__"]["tab"]["plan"].clone()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        scale_weights(model)
        feat_s, grads_s, _ = t.step(model)                                  # no device -> host read, no sync
    finally:
        torch.cuda.set_sync_debug_mode("default")
    plan_after = model._vsplit16_cache()["__vsplit16__"]["tab"]["plan"]
    assert not torch.equal(plan_before, plan_after)
    monkeypatch.setattr(engine, "_VSPLIT16", False)
    feat_p, grads_p, _ = t.step(model)
    want, want_grads = oracle_for(t, model)
    within_bars(t, feat_s, grads_s, feat_p, grads_p, "weights x8, gamma 50", want, want_grads)


def test_graphed_step_replans_on_every_replay(monkeypatch):
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
    eager, graphed, plain = make(), make(), make()
    g = GraphedStep(graphed, batch(10))
    assert "__vsplit16__" in graphed.student._vsplit16_cache()
    for rnd_i, seed in enumerate((20, 30)):
        if rnd_i == 1:                                                      # the optimizer's part: weights move between replays
            for mod in (eager, graphed, plain):
                scale_weights(mod.student)
        le, ge = eager_step(eager, batch(seed))
        lg = g.step(batch(seed))
        assert torch.equal(le, lg.detach()), (rnd_i, float(le), float(lg))
        gg = dict(graphed.named_parameters())
        for n, gr in ge.items():
            assert torch.equal(gr, gg[n].grad), (rnd_i, n)
        le2, ge2 = eager_step(eager, batch(seed))                           # two runs of the step: bit-identical
        assert torch.equal(le, le2) and all(torch.equal(ge[n], ge2[n]) for n in ge)
        monkeypatch.setattr(engine, "_VSPLIT16", False)
        lp, gp = eager_step(plain, batch(seed))
        monkeypatch.setattr(engine, "_VSPLIT16", True)
        d = abs(float(le) - float(lp)) / abs(float(lp))
        print(f"graphed step round {rnd_i}: loss split {float(le):.8f} plain {float(lp):.8f} rel {d:.2e}")
        assert d <= 1e-5
        assert not all(torch.equal(ge[n], gp[n]) for n in ge)               # the split path did run


# ------------------------------------------------------------------------------------------------ 6. guard

def test_guard_flags_without_a_sync(monkeypatch, caplog):
    from dclip_amd import engine, ops
    from dclip_amd.clip_model import from_hf_state_dict
    t = tower("tiny")
    model = from_hf_state_dict(t.cfg, t.sd, device=t.dev)
    monkeypatch.setattr(engine, "_VSPLIT16", True)
    monkeypatch.setattr(engine, "_SPLIT16_LOGGED", set())
    t.step(model)
    with torch.no_grad():
        for ln in (model.vision_model.encoder.layers[1].layer_norm1, model.vision_model.encoder.layers[1].layer_norm2):
            ln.weight.fill_(1e7)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        feat_s, grads_s, _ = t.step(model)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    ent = model._vsplit16_cache()["__vsplit16__"]
    flags = ent["tab"]["plan"][:, ops.SPLIT16_PLAN_FLAGS].view(torch.int32).tolist()
    assert flags[1] & 1 and flags[0] == 0
    monkeypatch.setattr(engine, "_VSPLIT16", False)
    feat_p, grads_p, _ = t.step(model)
    monkeypatch.setattr(engine, "_VSPLIT16", True)
    assert bool(torch.isfinite(feat_s)[torch.isfinite(feat_p)].all())
    want, want_grads = oracle_for(t, model)
    es, ep = norm_err(feat_s, want), norm_err(feat_p, want)
    print(f"guard (gamma 1e7): features vs fp64 split {es:.3e} plain {ep:.3e} ratio {es / ep:.2f}")
    assert es <= 4 * ep
    within_bars(t, feat_s, grads_s, feat_p, grads_p, "guard (gamma 1e7)", want, want_grads)      # and every gradient
    # the flag travels by the copy issued behind the refresh; the host looks at it at the next refresh and logs once
    torch.cuda.synchronize()
    with caplog.at_level(logging.WARNING, logger="dclip_amd"):
        with torch.no_grad():
            model.vision_model.encoder.layers[0].layer_norm1.bias.add_(0.0)  # a version bump: the next forward refreshes
        t.step(model)
        t.step(model)
    msgs = [r.getMessage() for r in caplog.records if "split-fp16 vision tower" in r.getMessage()]
    assert len(msgs) == 1 and "1:1" in msgs[0], msgs
