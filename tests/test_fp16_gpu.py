"""Opt-in fp16 path for frozen towers: kernels against fp64 on fp16-rounded operands, the conversion rule, and the towers'
measured error against the fp32 towers (the 1e-3 bar that the bf16 path misses)."""
import pytest
import torch

from dclip_amd import config as dcfg, synth

pytestmark = pytest.mark.gpu


def rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def half_operands(a, w, K, dev):
    from dclip_amd import ops
    if K % 4 == 0:
        return ops.cast_f16(a.to(dev)), ops.cast_f16(w.to(dev))
    ld = (K + 7) // 8 * 8          # the cast kernel takes rows of a multiple of 4 floats: pad on the host
    a16 = torch.zeros(a.shape[0], ld, dtype=torch.float16)
    w16 = torch.zeros(w.shape[0], ld, dtype=torch.float16)
    a16[:, :K], w16[:, :K] = a.half(), w.half()
    return a16.to(dev), w16.to(dev)


def check_gemm(a16, w16, K, bias, res, tag=""):
    """Every forward epilogue of gemm_f16 against fp64 on the fp16 operands."""
    from dclip_amd import ops
    a64, w64 = a16[:, :K].double().cpu(), w16[:, :K].double().cpu()
    want0 = a64 @ w64.t()
    want = want0 + bias.double().cpu()
    tol = 2e-6 * max(1.0, K ** 0.5)
    got0 = ops.gemm_f16(a16, w16, k=K)
    assert got0.dtype == torch.float32
    assert float((got0.double().cpu() - want0).abs().max() / want0.abs().max()) < tol, tag
    got = ops.gemm_f16(a16, w16, k=K, bias=bias)
    err = float((got.double().cpu() - want).abs().max() / want.abs().max())
    assert err < tol, (tag, err)
    got2 = ops.gemm_f16(a16, w16, k=K, bias=bias, residual=res)
    assert float((got2.double().cpu() - (want + res.double().cpu())).abs().max() / want.abs().max()) < 1e-5, tag
    g16 = ops.gemm_f16(a16, w16, k=K, bias=bias, gelu=True, out_f16=True)
    ref = (want * torch.sigmoid(1.702 * want)).half().double()
    assert g16.dtype == torch.float16
    assert float((g16.cpu().double() - ref).abs().max() / ref.abs().max()) < 2e-3, tag
    q16 = ops.gemm_f16(a16, w16, k=K, bias=bias, out_f16=True)                        # the qkv projection's form
    assert float((q16.cpu().double() - want.half().double()).abs().max() / want.abs().max()) < 2e-3, tag
    return got, got2, g16, q16


@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (400, 768, 768), (257, 132, 588), (2048, 3072, 768), (13, 64, 72),
                                   (12800, 768, 3072), (128, 256, 85), (64, 64, 21), (130, 132, 149)])   # odd K too
def test_gemm_f16_matches_rounded_inputs(M, N, K):
    """Register-staged 64x64 / 128x128 kernels, and the ping-pong kernel at >= 128 256x256 tiles (12800 x 768)."""
    dev = torch.device("cuda:0")
    a, w, bias, res = rnd((M, K), 1), rnd((N, K), 2, 0.1), rnd((N,), 3).to(dev), rnd((M, N), 4).to(dev)
    a16, w16 = half_operands(a, w, K, dev)
    assert torch.equal(a16[:, :K].cpu(), a.half())
    check_gemm(a16, w16, K, bias, res, f"{M}x{N}x{K}")


@pytest.mark.parametrize("M,N,K", [(1000, 520, 64), (2048, 1024, 128), (5000, 768, 768), (4096, 2304, 768)])
def test_gemm_f16_persistent_kernel(M, N, K, monkeypatch):
    """The env-selected variant has fp16 instances too: the persistent ping-pong kernel (DCLIP_BF16_PERSIST) against the
    one-tile ping-pong kernel (bit-identical without a residual)."""
    dev = torch.device("cuda:0")
    a16, w16 = rnd((M, K), 1).half().to(dev), rnd((N, K), 2, 0.1).half().to(dev)
    bias, res = rnd((N,), 3).to(dev), rnd((M, N), 4).to(dev)
    monkeypatch.setenv("DCLIP_BF16_BIG_MIN", "1")
    monkeypatch.setenv("DCLIP_BF16_PERSIST", "0")
    one = check_gemm(a16, w16, K, bias, res, "pingpong")
    monkeypatch.setenv("DCLIP_BF16_PERSIST", "1")
    monkeypatch.setenv("DCLIP_BF16_PERSIST_MIN", "1")
    per = check_gemm(a16, w16, K, bias, res, "persistent")
    for i in (0, 2, 3):
        assert torch.equal(per[i], one[i]), i


@pytest.mark.parametrize("M,N,K", [(64, 64, 64), (300, 512, 128), (12800, 1024, 64)])      # register-staged, ping-pong
def test_f16_conversion_rule_saturates_and_keeps_nan(M, N, K):
    """A finite result beyond the fp16 range leaves as +-65504 (not inf); a NaN operand gives NaN (not a clamped value)."""
    from dclip_amd import ops
    dev = torch.device("cuda:0")
    a = torch.full((M, K), 100.0)
    w = torch.full((N, K), 100.0)
    w[1::2] = -100.0                                   # 100 * 100 * K >= 640000 in magnitude
    a[3, 5] = float("nan")
    a16, w16 = a.half().to(dev), w.half().to(dev)
    for bias in (None, torch.zeros(N, device=dev)):
        c16 = ops.gemm_f16(a16, w16, bias=bias, out_f16=True).cpu()
        c32 = ops.gemm_f16(a16, w16, bias=bias).cpu()
        ok = torch.ones(M, dtype=torch.bool)
        ok[3] = False
        assert torch.isnan(c16[3]).all() and torch.isnan(c32[3]).all()
        assert torch.equal(c16[ok, 0::2].float(), torch.full((M - 1, N // 2), 65504.0))
        assert torch.equal(c16[ok, 1::2].float(), torch.full((M - 1, N // 2), -65504.0))
        assert not torch.isinf(c16).any()
        g = ops.gemm_f16(a16, w16, bias=bias, gelu=True, out_f16=True).cpu()   # gelu(+x) = x, gelu(-x) ~ -0
        assert torch.equal(g[ok, 0::2].float(), torch.full((M - 1, N // 2), 65504.0)) and torch.isnan(g[3]).all()


def test_cast_f16_conversion_rule():
    from dclip_amd import ops
    dev = torch.device("cuda:0")
    x = torch.tensor([[1.0, -2.5, 65504.0, 65519.0, 65520.0, 1e6, -1e6, 3.4e38],
                      [float("nan"), float("inf"), float("-inf"), 6e-8, -0.0, 1e-3, 0.1, -65536.0]])
    y = ops.cast_f16(x.to(dev)).cpu()
    want = x.half()
    want[0, 4:8] = torch.tensor([65504.0, 65504.0, -65504.0, 65504.0]).half()     # saturated where .half() gives inf
    want[1, 7] = -65504.0
    assert torch.equal(y[~torch.isnan(x)], want[~torch.isnan(x)])
    assert torch.isnan(y[1, 0]) and torch.isinf(y[1, 1]) and torch.isinf(y[1, 2])


@pytest.mark.parametrize("rows,cols", [(33, 768), (7, 21), (1000, 1024)])
def test_cast_f16_equals_torch_half(rows, cols):
    from dclip_amd import ops
    dev = torch.device("cuda:0")
    x = rnd((rows, cols), 5, 30.0)
    if cols % 4:
        with pytest.raises(Exception):
            ops.cast_f16(x.to(dev))
        return
    y = ops.cast_f16(x.to(dev)).cpu()
    assert y.dtype == torch.float16 and y.shape[1] % 8 == 0
    assert torch.equal(y[:, :cols], x.half()) and float(y[:, cols:].float().abs().sum()) == 0.0


@pytest.mark.parametrize("B,S,p", [(3, 64, 16), (2, 224, 32), (5, 32, 4)])
def test_im2col_f16_equals_im2col_then_half(B, S, p):
    from dclip_amd import ops
    dev = torch.device("cuda:0")
    pix = rnd((B, 3, S, S), 11).to(dev)
    want = ops.im2col(pix, p).half()
    got = ops.im2col_f16(pix, p)
    assert got.dtype == torch.float16 and torch.equal(got[:, :want.shape[1]], want)


@pytest.mark.parametrize("D", [768, 1024, 512, 100])
def test_layernorm_f16(D):
    from dclip_amd import ops
    dev = torch.device("cuda:0")
    x, g, b = rnd((33, D), 1, 2.0), 1 + rnd((D,), 2, 0.1), rnd((D,), 3, 0.1)
    y = ops.layernorm_fwd_f16(x.to(dev), g.to(dev), b.to(dev), 1e-5)
    want = torch.nn.functional.layer_norm(x.double(), (D,), g.double(), b.double(), 1e-5)
    assert y.dtype == torch.float16
    err = (y.cpu().double() - want).abs()
    assert bool((err <= want.abs() * 2.0 ** -11 + 1e-5).all()), float(err.max())       # half an fp16 ulp + fp32 noise


def attention_ref(qkv16, B, S, H, causal):
    q, k, v = (qkv16.double().view(B, S, 3, H, 64)[:, :, i].transpose(1, 2) for i in range(3))
    s = (q @ k.transpose(-1, -2)) * 0.125
    if causal:
        s = s + torch.full((S, S), float("-inf"), dtype=torch.float64).triu(1)
    return (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B * S, H * 64)


@pytest.mark.parametrize("B,S,H,causal", [(2, 50, 2, False), (2, 77, 2, True), (1, 197, 1, False), (1, 257, 2, False),
                                          (2, 257, 2, True), (3, 64, 1, True), (2, 1, 1, False), (1, 289, 1, False),
                                          (1, 320, 2, True), (3, 96, 2, False)])       # <= 288: whole-head, beyond: tiled
def test_attention_fwd_f16(B, S, H, causal):
    """fp16 q/k/v, fp32 softmax, fp16 P and output: against an fp64 attention of the same rounded inputs."""
    from dclip_amd import ops
    dev = torch.device("cuda:0")
    qkv = rnd((B * S, 3 * H * 64), 7 + S, 1.2).half()
    want = attention_ref(qkv, B, S, H, causal)
    got = ops.attention_fwd_f16(qkv.to(dev), B, S, H, causal)
    assert got.dtype == torch.float16 and tuple(got.shape) == (B * S, H * 64)
    err = float((got.double().cpu() - want).abs().max() / want.abs().max())
    assert err < 2e-3, err            # fp16 rounding of P (2^-11 relative) and of the output


@pytest.mark.parametrize("B,S,H,use_rows", [(3, 50, 12, False), (2, 257, 16, False), (5, 77, 8, True), (2, 1, 1, False),
                                            (2, 300, 2, True), (1, 512, 1, False), (7, 197, 3, False)])
def test_attention_row_fwd_f16(B, S, H, use_rows):
    from dclip_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(S * 31 + H)
    qkv = (torch.randn(B * S, 3 * H * 64, generator=g) * 1.5).half()
    rows = torch.randint(0, S, (B,), generator=g, dtype=torch.int32) if use_rows else None
    if use_rows:
        rows[0], rows[-1] = S - 1, 0
    x = qkv.double().view(B, S, 3, H, 64)
    want = torch.empty(B, H * 64, dtype=torch.float64)
    for b in range(B):
        r = int(rows[b]) if use_rows else 0
        n = r + 1 if use_rows else S
        p = torch.softmax(torch.einsum("hd,nhd->hn", x[b, r, 0], x[b, :n, 1]) * 0.125, dim=-1)
        want[b] = torch.einsum("hn,nhd->hd", p, x[b, :n, 2]).reshape(-1)
    got = ops.attention_row_fwd_f16(qkv.to(dev), None if rows is None else rows.to(dev), B, S, H)
    assert got.dtype == torch.float16 and tuple(got.shape) == (B, H * 64)
    err = float((got.double().cpu() - want).abs().max() / want.abs().max())
    assert err < 1e-3, err                                           # the fp16 rounding of the output


def _stats(a, b):
    rel = float((a - b).abs().max() / a.abs().max())
    cos = float(torch.nn.functional.cosine_similarity(a, b, dim=1).min())
    return rel, cos


@pytest.mark.parametrize("name,mk", [("ViT-B/32", dcfg.vit_b32), ("ViT-L/14", dcfg.vit_l14)])
def test_frozen_towers_f16_meet_the_bar(name, mk):
    """The 1e-3 relative bar on embeddings: fp16 towers against the fp32 towers on the same weights and inputs (those of
    test_frozen_vision_tower_bf16_error / test_frozen_text_tower_bf16_error); bf16 printed beside for comparison."""
    from dclip_amd.clip_model import from_hf_state_dict
    dev = torch.device("cuda:0")
    cfg = mk()
    m = from_hf_state_dict(cfg, synth.synth_clip_state_dict(cfg, seed=0, gain=3.0), device=dev)
    pix = synth.synth_regions(4, 1, cfg.vision, seed=2)[:, 0].to(dev)
    ids = synth.synth_input_ids(6, cfg.text, seed=3, ragged=True).to(dev)
    with torch.no_grad():
        img32 = m.get_image_features(pixel_values=pix)
        txt32 = m.get_text_features(input_ids=ids)
        s32, t32, e32 = m.text_token_level(ids)
        out = {}
        for prec in ("fp16", "bf16", "fp16"):
            res = (m.get_image_features(pixel_values=pix, precision=prec), m.get_text_features(input_ids=ids, precision=prec),
                   m.text_token_level(ids, precision=prec))
            if prec in out:                                   # second fp16 pass, after a bf16 one: bit-identical
                assert torch.equal(res[0], out[prec][0]) and torch.equal(res[1], out[prec][1])
                assert all(torch.equal(x, y) for x, y in zip(res[2], out[prec][2]))
            out[prec] = res
    for prec in ("bf16", "fp16"):
        img, txt, (s16, t16, e16) = out[prec]
        assert torch.equal(e16, e32)
        figures = {"image": _stats(img32, img), "text": _stats(txt32, txt), "text(token pass)": _stats(s32, s16)}
        for part, (rel, cos) in figures.items():
            print(f"{name} {part}: {prec} max rel err {rel:.2e}, min cosine {cos:.7f}")
        if prec == "fp16":
            for part, (rel, cos) in figures.items():
                assert rel < 1e-3 and cos > 0.99999, (name, part, rel, cos)
            for b in range(ids.shape[0]):                     # the word-token rows the teacher reads
                n = int(e32[b])
                cos = torch.nn.functional.cosine_similarity(t32[b, 1:n], t16[b, 1:n], dim=1)
                assert float(cos.min()) > 0.99999, (b, float(cos.min()))


def test_meta_teacher_f16_towers_close_to_fp32():
    """compute_global_embedding with tower_precision='fp16' vs 'fp32' (setup of test_meta_teacher_bf16_towers_close_to_fp32)."""
    from dclip_amd.clip_model import from_hf_state_dict
    from dclip_amd.patch_text_aggregation import PatchTextAggregation
    dev = torch.device("cuda:0")
    cfg = dcfg.vit_b32()
    clip = from_hf_state_dict(cfg, synth.synth_clip_state_dict(cfg, seed=0, gain=3.0), device=dev)
    E = cfg.projection_dim
    outs = {}
    for prec in ("fp32", "fp16"):
        t = PatchTextAggregation(embed_dim=E, num_heads=E // 64, clip_model=clip, tower_precision=prec).to(dev)
        t.cross_modal_attention.load_state_dict(synth.synth_cross_modal_state_dict(E, seed=5))
        regions = synth.synth_regions(3, 4, cfg.vision, seed=2).to(dev)
        ids = synth.synth_input_ids(3, cfg.text, seed=3, ragged=True).to(dev)
        with torch.no_grad():
            outs[prec] = t.compute_global_embedding_tensors(regions, ids, torch.tensor([4, 2, 0], dtype=torch.int32))
    rel, cos = _stats(outs["fp32"], outs["fp16"])
    print(f"meta-teacher fp16 towers: max rel err {rel:.2e}, min cosine {cos:.7f}")
    assert cos > 0.9999


def test_f16_and_bf16_weight_caches_are_separate():
    """bf16, then fp16, then bf16 on one model: the second bf16 result equals the first, the fp16 one a fresh model's."""
    from dclip_amd.clip_model import from_hf_state_dict
    dev = torch.device("cuda:0")
    cfg = dcfg.tiny()
    sd = synth.synth_clip_state_dict(cfg, seed=0, gain=3.0)
    m, fresh = from_hf_state_dict(cfg, sd, device=dev), from_hf_state_dict(cfg, sd, device=dev)
    pix = synth.synth_pixel_values(3, cfg.vision, seed=2).to(dev)
    ids = synth.synth_input_ids(3, cfg.text, seed=3, ragged=True).to(dev)

    def run(model, prec):
        return (model.get_image_features(pixel_values=pix, precision=prec), model.get_text_features(input_ids=ids, precision=prec),
                *model.text_token_level(ids, precision=prec))

    with torch.no_grad():
        b1, h, b2, hf = run(m, "bf16"), run(m, "fp16"), run(m, "bf16"), run(fresh, "fp16")
    assert all(torch.equal(x, y) for x, y in zip(b1, b2))
    assert all(torch.equal(x, y) for x, y in zip(h, hf))
    assert not torch.equal(h[0], b1[0])                       # the two paths did run different arithmetic


def test_f16_is_frozen_only():
    from dclip_amd.clip_model import from_hf_state_dict
    dev = torch.device("cuda:0")
    cfg = dcfg.tiny()
    m = from_hf_state_dict(cfg, synth.synth_clip_state_dict(cfg, seed=0, gain=3.0), device=dev)
    pix = synth.synth_pixel_values(2, cfg.vision, seed=2).to(dev)
    ids = synth.synth_input_ids(2, cfg.text, seed=3, ragged=True).to(dev)
    assert any(p.requires_grad for p in m.parameters())
    with pytest.raises(RuntimeError, match="fp16"):
        m.get_image_features(pixel_values=pix, precision="fp16")
    with pytest.raises(RuntimeError, match="fp16"):
        m.get_text_features(input_ids=ids, precision="fp16")
    m.requires_grad_(False)                                   # frozen: allowed with grad enabled
    assert not m.get_image_features(pixel_values=pix, precision="fp16").requires_grad
