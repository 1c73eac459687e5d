"""Split-fp16 evaluation of the frozen fp32 text tower, the parts that need no GPU: the arithmetic claim by
emulation on the host, the choice of the power-of-two scales, the guard, and the ABI of the new entries."""
import math
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def split(x, scale=1.0):
    v = x * scale
    hi = v.half()
    lo = (v - hi.float()).half()
    return hi, lo


def gemm_split(a, w):
    """A W^T from the three fp16 products, accumulated in fp32 (the products themselves are exact in fp32)."""
    ah, al = split(a)
    wh, wl = split(w)
    a3 = torch.cat([ah, al, ah], 1).float()
    w3 = torch.cat([wh, wh, wl], 1).float()
    return a3 @ w3.t()


def relerr(got, want):
    return float((got.double() - want).abs().max() / want.abs().max())


@pytest.mark.parametrize("M,N,K", [(96, 128, 512), (64, 96, 2048)])
def test_split_gemm_is_fp32_grade(M, N, K):
    """Against fp64 of the unsplit operands the three-product GEMM errs like the fp32 GEMM (within the two mantissa bits
    between 2^-22 and 2^-24), plain fp16 operands a hundred times more."""
    a, w = rnd((M, K), 1), rnd((N, K), 2, 0.05)
    want = a.double() @ w.double().t()
    e32 = relerr(a @ w.t(), want)
    es = relerr(gemm_split(a, w), want)
    e16 = relerr(a.half().float() @ w.half().float().t(), want)
    print(f"{M}x{N}x{K}: fp32 {e32:.2e}  split {es:.2e}  fp16 {e16:.2e}")
    assert es <= 4 * e32
    assert e16 > 50 * es


def test_split_pieces_reconstruct_22_bits():
    x = rnd((4096,), 3, 10.0)
    x = x[x.abs() >= 0.25]                   # high in fp16's range, where the scales put the operands: lo is not subnormal-limited
    hi, lo = split(x)
    rec = hi.double() + lo.double()
    # |lo| <= 2^-11 |x| and lo is rounded to 11 bits: half an ulp of it is 2^-22 |x|
    assert float(((rec - x.double()).abs() / x.double().abs()).max()) <= 2.0 ** -22 * (1 + 2.0 ** -9)
    exact = torch.tensor([0.0, 1.0, -2.5, 1024.0, 2.0 ** 14 - 8.0, -0.125])
    hi, lo = split(exact)
    assert torch.equal(hi.float(), exact) and torch.equal(lo.float(), torch.zeros(6))


def _layer(x, p, heads, mm):
    """One causal pre-LN layer in fp32 with `mm(a, w)` as its four GEMMs (quick-GELU)."""
    T, D = x.shape
    ln = torch.nn.functional.layer_norm
    h = ln(x, (D,), p["g1"], p["b1"])
    qkv = mm(h, p["qkv"]) + p["qkv_b"]
    q, k, v = (t.view(T, heads, D // heads).transpose(0, 1) for t in qkv.split(D, 1))
    s = (q @ k.transpose(1, 2)) * (D // heads) ** -0.5 + torch.full((T, T), float("-inf"), dtype=x.dtype).triu(1)
    ctx = (torch.softmax(s, -1) @ v).transpose(0, 1).reshape(T, D)
    x = x + mm(ctx, p["out"]) + p["out_b"]
    h = mm(ln(x, (D,), p["g2"], p["b2"]), p["fc1"]) + p["fc1_b"]
    return x + mm(h * torch.sigmoid(1.702 * h), p["fc2"]) + p["fc2_b"]


def test_split_tower_emulation():
    """A small causal tower (4 layers, D 128, 24 tokens): split fp16 stays fp32-grade against fp64, plain fp16 does not."""
    D, T, L, heads = 128, 24, 4, 2
    layers = []
    for i in range(L):
        s = 100 * i
        layers.append({"g1": 1 + rnd((D,), s + 1, 0.1), "b1": rnd((D,), s + 2, 0.1), "g2": 1 + rnd((D,), s + 3, 0.1),
                       "b2": rnd((D,), s + 4, 0.1), "qkv": rnd((3 * D, D), s + 5, 0.2), "qkv_b": rnd((3 * D,), s + 6, 0.1),
                       "out": rnd((D, D), s + 7, 0.09), "out_b": rnd((D,), s + 8, 0.1), "fc1": rnd((4 * D, D), s + 9, 0.09),
                       "fc1_b": rnd((4 * D,), s + 10, 0.1), "fc2": rnd((D, 4 * D), s + 11, 0.05), "fc2_b": rnd((D,), s + 12, 0.1)})
    x0 = rnd((T, D), 99)

    def run(mm, dtype):
        x = x0.to(dtype)
        for p in layers:
            x = _layer(x, {k: v.to(dtype) for k, v in p.items()}, heads, mm)
        return x

    want = run(lambda a, w: a @ w.t(), torch.float64)
    e32 = relerr(run(lambda a, w: a @ w.t(), torch.float32), want)
    es = relerr(run(gemm_split, torch.float32), want)
    e16 = relerr(run(lambda a, w: a.half().float() @ w.half().float().t(), torch.float32), want)
    print(f"tower emulation: fp32 {e32:.2e}  split {es:.2e}  fp16 {e16:.2e}")
    assert es < 1e-5
    assert e16 > 20 * es


def test_scale_selection():
    from dclip_amd import engine
    for bound in (1e-3, 0.5, 1.0, 22.7, 4096.0, 16384.0, 16385.0, 1e6, 2.0 ** 28):
        e = engine.split16_act_exp(bound)
        assert e is not None and -14 <= e <= 24
        assert bound * 2.0 ** e <= 2.0 ** 14                       # nothing can overflow
        assert e == 24 or bound * 2.0 ** (e + 1) > 2.0 ** 14        # and no smaller scale than needed
    assert engine.split16_act_exp(2.0 ** 28 * 1.0001) is None       # no e >= -14 fits
    assert engine.split16_act_exp(float("inf")) is None and engine.split16_act_exp(float("nan")) is None
    assert engine.split16_act_exp(0.0) == 24
    for m in (1e-4, 0.02, 0.5, 1.0, 3.7, 100.0):
        f = engine.split16_weight_exp(m)
        assert 2.0 ** 13 <= m * 2.0 ** f < 2.0 ** 14
    assert engine.split16_weight_exp(0.0) == 0


def _stats(gamma_max, D=512, seed=0):
    wv, fc1 = rnd((D, D), seed, 0.027), rnd((4 * D, D), seed + 1, 0.094)    # the ViT-B/32 text tower's init at gain 3
    return {"ln1_w": gamma_max, "ln1_b": 0.1, "v_l1": float(wv.abs().sum(1).max()), "v_b": 0.1, "ln2_w": gamma_max,
            "ln2_b": 0.1, "fc1_l1": float(fc1.abs().sum(1).max()), "fc1_b": 0.1}


def test_bounds_and_guard():
    from dclip_amd import engine
    D = 512
    st = _stats(1.5)
    b = engine.split16_layer_bounds(st, D)
    assert b["ln1"] == pytest.approx(1.5 * math.sqrt(D) + 0.1)
    assert b["ctx"] == pytest.approx(b["ln1"] * st["v_l1"] + 0.1) and b["g"] == pytest.approx(b["ln2"] * st["fc1_l1"] + 0.1)
    exps = {k: engine.split16_act_exp(v) for k, v in b.items()}
    assert all(e is not None for e in exps.values())
    for k, e in exps.items():
        assert b[k] * 2.0 ** e <= 2.0 ** 14
    # the bound really bounds: LayerNorm of any row stays inside it
    x = rnd((64, D), 5, 100.0)
    x[0, 0] = 1e6                                                   # one dominant element: |x - mu| rstd -> sqrt(D - 1)
    g = torch.full((D,), 1.5)
    y = torch.nn.functional.layer_norm(x, (D,), g, torch.full((D,), 0.1))
    assert float(y.abs().max()) <= b["ln1"]
    # a gamma of 1e6: the GELU bound needs 2^e below 2^-14 -> the guard trips
    big = engine.split16_layer_bounds(_stats(1e6), D)
    assert engine.split16_act_exp(big["g"]) is None


def test_header_binding_and_symbols_agree():
    import ctypes
    from dclip_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "dclip_hip.h")).read(), flags=re.S)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("dclip_split_f32_f16x3", 9), ("dclip_layernorm_fwd_f16x3", 9), ("dclip_gemm_f16_scaled", 15),
                        ("dclip_gemm_f16_scaled_split", 14)):
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, src)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name), name


def test_argument_errors():
    from dclip_amd import _lib
    lib = _lib.load()
    cases = [
        (lambda: lib.dclip_split_f32_f16x3(None, None, 1, 8, 8, 24, 1.0, 0, None), b"split_f32_f16x3: bad arguments"),
        (lambda: lib.dclip_split_f32_f16x3(16, 16, 1, 12, 12, 40, 1.0, 0, None), b"multiple of 8"),
        (lambda: lib.dclip_split_f32_f16x3(16, 16, 1, 8, 8, 16, 1.0, 0, None), b"ldx"),
        (lambda: lib.dclip_split_f32_f16x3(16, 16, 1, 8, 8, 24, 1.0, 2, None), b"order"),
        (lambda: lib.dclip_split_f32_f16x3(16, 16, 1, 8, 8, 24, 3.0, 0, None), b"power of two"),
        (lambda: lib.dclip_layernorm_fwd_f16x3(None, 16, 16, 16, 4, 8, 1e-5, 1.0, None), b"layernorm_fwd_f16x3: null pointer"),
        (lambda: lib.dclip_layernorm_fwd_f16x3(16, 16, 16, 16, 4, 6, 1e-5, 1.0, None), b"layernorm_fwd_f16x3: bad D"),
        (lambda: lib.dclip_layernorm_fwd_f16x3(16, 16, 16, 16, 4, 8, 1e-5, 0.3, None), b"power of two"),
        (lambda: lib.dclip_gemm_f16_scaled(None, None, None, None, None, 4, 4, 4, 8, 8, 4, 0, 0, 1.0, None), b"gemm_f16_scaled: null operand"),
        (lambda: lib.dclip_gemm_f16_scaled(16, 16, 16, None, None, 4, 4, 4, 8, 8, 4, 0, 0, float("inf"), None), b"alpha must be finite"),
        (lambda: lib.dclip_gemm_f16_scaled_split(16, 16, 16, None, 4, 8, 8, 8, 8, 24, 0, 1.0, 3.0, None), b"out_scale must be a power of two"),
        (lambda: lib.dclip_gemm_f16_scaled_split(16, 16, 16, None, 4, 8, 8, 8, 8, 16, 0, 1.0, 2.0, None), b"ldc >= 3 N"),
        (lambda: lib.dclip_gemm_f16_scaled_split(16, 16, 16, None, 4, 8, 8, 8, 8, 24, 8, 1.0, 2.0, None), b"BIAS | GELU only"),
    ]
    for call, msg in cases:
        assert call() == -1
        assert msg in lib.dclip_last_error(), (msg, lib.dclip_last_error())


def test_switch_is_read_once():
    from dclip_amd import engine
    assert engine.text_split16_enabled() == (os.environ.get("DCLIP_TEXT_SPLIT16", "1") != "0")
    src = open(os.path.join(REPO, "dclip_amd", "engine.py")).read()
    assert src.count('os.environ.get("DCLIP_TEXT_SPLIT16"') == 1
