"""Split-fp16 evaluation of the frozen fp32 text tower on the GPU: the split kernels bit for bit against the
same three lines of torch on the host, `alpha` of the 16-bit GEMM, the split GEMM and the whole tower against fp64."""
import pytest
import torch

from dclip_amd import config as dcfg, synth

pytestmark = pytest.mark.gpu

SENTINEL = 0x1234


def rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def host_split(x, scale, order):
    v = x * scale
    hi = v.half()
    lo = (v - hi.float()).half()
    return torch.cat([hi, lo, hi] if order == 0 else [hi, hi, lo], 1)


def same_bits(got, want):
    """Bit equality of two fp16 tensors; where the host value is a NaN the device value must be a NaN (the sign and payload of
    a NaN that an operation PRODUCES, inf - inf here, are not fixed by IEEE 754 and differ between the two machines)."""
    nan = want.isnan()
    return bool(torch.equal(got.isnan(), nan)) and bool(torch.equal(got.view(torch.int16)[~nan], want.view(torch.int16)[~nan]))


# ------------------------------------------------------------------------------------------------ split kernel

@pytest.mark.parametrize("rows", [1, 3, 130])
@pytest.mark.parametrize("cols", [8, 520])
def test_split_kernel_bit_equal_to_host(rows, cols):
    from dclip_amd import _lib, ops
    lib = _lib.load()
    dev = torch.device("cuda:0")
    ldy = 3 * cols + 8                                            # 8 padding columns that must stay untouched
    for scale in (1.0, 2.0 ** -3, 2.0 ** 9):
        x = rnd((rows, cols), 7 + rows + cols, 40.0) / scale
        # 0, fp16-exact values (lo must be +-0), just under 2^14, a subnormal lo (2^-20), a negative, NaN, inf
        special = torch.tensor([0.0, -1024.0, 16383.99, 1.0 + 2.0 ** -20, -3.3, float("nan"), float("inf"), 0.1]) / scale
        x.view(-1)[:8] = special
        xd = x.to(dev)
        for order in (0, 1):
            y = torch.full((rows, ldy), SENTINEL, dtype=torch.int16, device=dev)
            _lib.check(lib.dclip_split_f32_f16x3(xd.data_ptr(), y.data_ptr(), rows, cols, cols, ldy, scale, order, ops._stream()),
                       "split")
            got = y.cpu()
            want = host_split(x, scale, order)
            assert bool((got[:, 3 * cols:] == SENTINEL).all()), "padding columns were written"
            assert same_bits(got[:, :3 * cols].view(torch.float16), want), (rows, cols, scale, order)
            w0 = want[0].view(torch.int16)
            lo0 = slice(cols, 2 * cols) if order == 0 else slice(2 * cols, 3 * cols)
            assert int(w0[lo0][0]) == 0 and int(w0[lo0][1]) in (0, -32768)          # the host reference itself: lo of exact values
            # the wrapper (ldy = 3 cols) gives the same
            assert same_bits(ops.split_f16x3(xd, scale, order).cpu(), want)


# ------------------------------------------------------------------------------------------------ LayerNorm with split output

@pytest.mark.parametrize("D", [512, 768, 1024, 72])
def test_layernorm_split_equals_split_of_layernorm(D):
    from dclip_amd import ops
    dev = torch.device("cuda:0")
    rows, eps, scale = 5, 1e-5, 2.0 ** 4
    x = (rnd((rows, D), D, 3.0) + 1.0).to(dev)
    g, b = (1.0 + rnd((D,), D + 1, 0.3)).to(dev), rnd((D,), D + 2, 0.2).to(dev)
    ln, _, _ = ops.layernorm_fwd(x, g, b, eps, save_stats=False)
    want = ops.split_f16x3(ln, scale, 0)
    got = ops.layernorm_fwd_f16x3(x, g, b, eps, scale)
    assert tuple(got.shape) == (rows, 3 * D) and got.dtype == torch.float16
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert torch.equal(want.cpu().view(torch.int16), host_split(ln.cpu(), scale, 0).view(torch.int16))


# ------------------------------------------------------------------------------------------------ alpha

# (130, 72, 40) and (300, 512, 1536): the issue's shapes (the register-staged 64x64 kernel takes both); (2048, 2048, 64): the
# register-staged 128x128 kernel; (2816, 3072, 64): 132 tiles of 256x256, the ping-pong kernel the tower's GEMMs run on
@pytest.mark.parametrize("M,N,K", [(130, 72, 40), (300, 512, 1536), (2048, 2048, 64), (2816, 3072, 64)])
def test_gemm_f16_alpha(M, N, K):
    check_alpha(M, N, K)


def check_alpha(M, N, K):
    """alpha = 1 against the entry without alpha, alpha = 2^-5 against that entry's output scaled on the host: bit-equal, on
    whichever kernel the dispatcher picks for the shape under the switches that are set."""
    from dclip_amd import ops
    dev = torch.device("cuda:0")
    a16, w16 = rnd((M, K), 1).half().to(dev), rnd((N, K), 2, 0.1).half().to(dev)
    bias, res = rnd((N,), 3).to(dev), rnd((M, N), 4).to(dev)
    al = 2.0 ** -5
    base = ops.gemm_f16(a16, w16, k=K)
    assert torch.equal(ops.gemm_f16(a16, w16, k=K, alpha=1.0), base)
    for kw in (dict(bias=bias), dict(bias=bias, residual=res), dict(bias=bias, gelu=True), dict(bias=bias, gelu=True, out_f16=True),
               dict(bias=bias, out_f16=True)):
        assert torch.equal(ops.gemm_f16(a16, w16, k=K, alpha=1.0, **kw), ops.gemm_f16(a16, w16, k=K, **kw)), kw
    # a power of two is exact: the scaled accumulator is the unscaled one times 2^-5, and each later step rounds once
    assert torch.equal(ops.gemm_f16(a16, w16, k=K, alpha=al).cpu(), base.cpu() * al)
    assert torch.equal(ops.gemm_f16(a16, w16, k=K, alpha=al, bias=bias).cpu(), base.cpu() * al + bias.cpu())
    assert torch.equal(ops.gemm_f16(a16, w16, k=K, alpha=al, bias=bias, residual=res).cpu(), (base.cpu() * al + bias.cpu()) + res.cpu())
    assert torch.equal(ops.gemm_f16(a16, w16, k=K, alpha=al, bias=bias, out_f16=True).cpu(),
                       ops.cast_f16((base * al + bias).contiguous(), pad_to=4).cpu())


@pytest.mark.parametrize("M,N,K", [(130, 72, 40), (2048, 2048, 64), (2816, 3072, 64)])      # 64x64, 128x128, ping-pong
def test_gemm_f16_split_output(M, N, K):
    check_split_output(M, N, K)


def check_split_output(M, N, K):
    """The GEMM that writes its result already split: bit-equal to the stand-alone split of the same GEMM's fp32 output."""
    from dclip_amd import ops
    dev = torch.device("cuda:0")
    a16, w16 = rnd((M, K), 1).half().to(dev), rnd((N, K), 2, 0.1).half().to(dev)
    bias = rnd((N,), 3).to(dev)
    al, so = 2.0 ** -2, 2.0 ** 5
    for kw in (dict(), dict(bias=bias), dict(bias=bias, gelu=True)):
        want = ops.split_f16x3(ops.gemm_f16(a16, w16, k=K, alpha=al, **kw), so, 0)
        got = ops.gemm_f16(a16, w16, k=K, alpha=al, split_out_scale=so, **kw)
        assert tuple(got.shape) == (M, 3 * N) and got.dtype == torch.float16
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), kw


@pytest.mark.parametrize("M,N,K", [(1000, 520, 64), (5000, 768, 768), (5900, 6144, 64)])      # 12 / 60 / 576 tiles of 256x256
def test_gemm_f16_alpha_persistent_kernel(M, N, K, monkeypatch):
    """alpha in both epilogue branches (16-bit and fp32 windows) of the persistent ping-pong kernel (DCLIP_BF16_PERSIST=1; the
    last shape passes its default threshold of 512 tiles).  A split output never takes that kernel: checked on the same shapes."""
    monkeypatch.setenv("DCLIP_BF16_PERSIST", "1")
    if M * N < 512 * 65536:
        monkeypatch.setenv("DCLIP_BF16_BIG_MIN", "1")
        monkeypatch.setenv("DCLIP_BF16_PERSIST_MIN", "1")
    check_alpha(M, N, K)
    check_split_output(M, N, K)


# ------------------------------------------------------------------------------------------------ split GEMM

def split_gemm(a, w, e, f, **kw):
    from dclip_amd import ops
    return ops.gemm_f16(ops.split_f16x3(a, 2.0 ** e, 0), ops.split_f16x3(w, 2.0 ** f, 1), alpha=2.0 ** -(e + f), **kw)


def tower_scales(a, w):
    from dclip_amd import engine
    return engine.split16_act_exp(float(a.abs().max())), engine.split16_weight_exp(float(w.abs().max()))


def norm_err(got, want):
    return float((got.double().cpu() - want).abs().max() / want.abs().max())


def check_split_gemm(a, w, e, f, tag, bar=True):
    """Plain, bias + GELU and bias + residual against fp64 of the unsplit fp32 operands: at most 4x ops.gemm's own error
    (the two mantissa bits between 2^-22 and 2^-24)."""
    from dclip_amd import ops
    dev = torch.device("cuda:0")
    M, N = a.shape[0], w.shape[0]
    bias, res = rnd((N,), 3, float(a.abs().max() * w.abs().max())), rnd((M, N), 4, float(a.abs().max() * w.abs().max()))
    ad, wd, bd, rd = a.to(dev), w.to(dev), bias.to(dev), res.to(dev)
    z = a.double() @ w.double().t()
    zb = z + bias.double()
    figures = {}
    for name, want, kw, kw32 in (
            ("plain", z, {}, {}),
            ("bias+gelu", zb * torch.sigmoid(1.702 * zb), dict(bias=bd, gelu=True), dict(bias=bd, epilogue=ops.EPI_GELU)),
            ("bias+residual", zb + res.double(), dict(bias=bd, residual=rd), dict(bias=bd, residual=rd))):
        e32 = norm_err(ops.gemm(ad, wd, ops.LAYOUT_NT, **kw32), want)
        es = norm_err(split_gemm(ad, wd, e, f, **kw), want)
        print(f"split GEMM {tag} {name}: fp32 {e32:.3e}  split {es:.3e}  ratio {es / e32:.2f}")
        figures[name] = (e32, es)
    if bar:
        for name, (e32, es) in figures.items():
            assert es <= 4 * e32, (tag, name, e32, es)
    return figures


@pytest.mark.parametrize("M,N,K", [(130, 72, 40), (231, 1536, 512)])
def test_split_gemm_against_fp64(M, N, K):
    a, w = rnd((M, K), 11, 2.0), rnd((N, K), 12, 0.05)
    check_split_gemm(a, w, *tower_scales(a, w), f"{M}x{N}x{K}")


def test_subnormal_probe():
    """A in [1e-4, 1e-3] and W about 1e-5 with scales of 1 put every lo piece (and most of W) among the fp16 subnormals: the
    error is only REPORTED (what the MFMA does with subnormal inputs).  With the tower's scales the same data
    must meet the bar."""
    M, N, K = 231, 1536, 512
    g = torch.Generator().manual_seed(21)
    a = torch.rand((M, K), generator=g) * 9e-4 + 1e-4
    w = rnd((N, K), 22, 1e-5)
    fig = check_split_gemm(a, w, 0, 0, "subnormal probe, scales 1", bar=False)
    print("subnormal probe (scales 1): " + ", ".join(f"{k} split/fp32 = {es / e32:.1f}" for k, (e32, es) in fig.items()))
    e, f = tower_scales(a, w)
    assert e > 0 and f > 0
    check_split_gemm(a, w, e, f, f"subnormal probe, scales 2^{e} 2^{f}")


# ------------------------------------------------------------------------------------------------ tower

def _text_model(gain, dev):
    from dclip_amd.clip_model import from_hf_state_dict
    cfg = dcfg.vit_b32()
    sd = synth.synth_clip_state_dict(cfg, seed=0, gain=gain)
    m = from_hf_state_dict(cfg, sd, device=dev)
    m.requires_grad_(False)
    return cfg, sd, m


@pytest.mark.parametrize("gain", [1.0, 3.0])
def test_text_tower_split16(gain, monkeypatch):
    from dclip_amd import engine
    from oracle import dclip_oracle as O
    dev = torch.device("cuda:0")
    monkeypatch.setattr(engine, "_SPLIT16", True)
    cfg, sd, m = _text_model(gain, dev)
    ids = synth.synth_input_ids(3, cfg.text, seed=3, ragged=True)
    assert ids.shape[1] == 77 and len({int((r == cfg.text.eos_token_id).int().argmax()) for r in ids}) > 1     # ragged, EOS padded
    idd = ids.to(dev)
    want = O.text_tower(O.to_dtype({k: v for k, v in sd.items() if k.startswith("text_")}, torch.float64), ids, cfg.text)
    with torch.no_grad():
        plain = engine.text_fwd_frozen(m.text_params_detached(), idd, cfg.text)
        got = m.get_text_features(input_ids=idd)
        plan = m._split16_cache()["__split16__"]["layers"]
        assert plan is not None and len(plan) == cfg.text.num_hidden_layers          # the split path did run
        assert not torch.equal(got, plain)
        e_split, e_plain = norm_err(got, want), norm_err(plain, want)
        print(f"text tower gain {gain}: split vs fp64 {e_split:.3e}, fp32 vs fp64 {e_plain:.3e}, "
              f"split vs fp32 {norm_err(got, plain.double().cpu()):.3e}")
        assert e_split <= 1e-5
        assert torch.equal(m.get_text_features(input_ids=idd), got)                    # run to run
        monkeypatch.setattr(engine, "_SPLIT16_FC1_EPI", not engine._SPLIT16_FC1_EPI)   # fc1's split epilogue / the split pass
        assert torch.equal(m.get_text_features(input_ids=idd), got)
        monkeypatch.setattr(engine, "_SPLIT16_FC1_EPI", not engine._SPLIT16_FC1_EPI)
        # eager == graph replay
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                captured = m.get_text_features(input_ids=idd)
        torch.cuda.current_stream(dev).wait_stream(side)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured, got)
        # switch off: the parent's output, bit for bit
        monkeypatch.setattr(engine, "_SPLIT16", False)
        assert torch.equal(m.get_text_features(input_ids=idd), plain)
        monkeypatch.setattr(engine, "_SPLIT16", True)
        # guard: a huge gamma sends the tower to the plain path (decided from the weights), nothing becomes inf
        for ln in (m.text_model.encoder.layers[3].layer_norm1, m.text_model.encoder.layers[3].layer_norm2):
            ln.weight.fill_(1e7)
        guarded = m.get_text_features(input_ids=idd)
        assert m._split16_cache()["__split16__"]["layers"] is None
        assert torch.equal(guarded, engine.text_fwd_frozen(m.text_params_detached(), idd, cfg.text))
        assert bool(torch.isfinite(guarded).all())
