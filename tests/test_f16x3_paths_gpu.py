"""The fused split-fp16 GEMM entries through the C ABI: every K-major twin in every epilogue form, the statistics
twin, the token-major twin, and both forms on real split data.  Outputs live in guarded NaN-filled buffers; every operand element
the contract says is not read — the duplicate third of each operand, the padding — is NaN; dclip_last_launch() is asserted in
full; the references are the restatements of tests/kernel_checks_f16x3.py (integer data: exact in fp32 in any order)."""
import pytest
import torch

from tests import kernel_checks as kc
from tests import kernel_checks_f16x3 as kx
from tests import kernel_checks_rest as kr
from tests import kernel_checks_split16 as ks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from dclip_amd import _lib
    return _lib.load()


def stream():
    return torch.cuda.current_stream().cuda_stream


def ok(lib, rc, site):
    assert rc == 0, f"{site}: rc={rc}: {lib.dclip_last_error().decode(errors='replace')}"
    assert lib.dclip_last_launch() == site.encode(), (lib.dclip_last_launch(), site)


# ------------------------------------------------------------------------------------------------ the K-major twins

@pytest.mark.parametrize("c", kx.x3_cases(), ids=kx.x3_id)
def test_fused_entries(dev, lib, c):
    s = kx.build_x3(c, dev)
    ok(lib, kx.launch_x3(lib, s, stream()), kx.x3_site(c))
    torch.cuda.synchronize()
    kc.record("f16x3", tuple(c), kx.verify_x3(s))


@pytest.mark.parametrize("K", kx.X3_K)
@pytest.mark.parametrize("dgelu", [False, True])
def test_statistics_equal_the_unfused_entrys_on_the_same_stored_c(dev, lib, monkeypatch, K, dgelu):
    """The unfused statistics entry on the whole [hi|lo|hi] x [hi|hi|lo] operands (zero columns up to a multiple of 64: it has the
    ping-pong kernel only) stores the same C — integer data, exact accumulators, the same epilogue — so pmax / psum are equal
    bit for bit."""
    monkeypatch.setenv("DCLIP_BF16_BIG_MIN", "1")
    c = kx.X3Case("rows_stats_dgelu" if dgelu else "rows_stats", 300, 264, K, 1, False)
    s = kx.build_x3(c, dev)
    ok(lib, kx.launch_x3(lib, s, stream()), kx.x3_site(c))
    K3 = kc.roundup(3 * K, 64)
    A = torch.zeros((c.M, K3), dtype=torch.float16, device=dev)
    W = torch.zeros((c.N, K3), dtype=torch.float16, device=dev)
    A[:, :3 * K], W[:, :3 * K] = s.a.to(dev).half(), s.w.to(dev).half()
    P = -(-c.M // 256)
    C2, pm2, ps2 = kc.Guarded(c.M, c.N, s.ldc, device=dev), kc.Guarded(P, c.N, device=dev), kc.Guarded(P, c.N, device=dev)
    rc = lib.dclip_gemm_f16_scaled_rows_stats_dev(A.data_ptr(), W.data_ptr(), C2.ptr, None if s.aux_d is None else s.aux_d.data_ptr(),
                                                  c.M, c.N, K3, K3, K3, s.ldc, s.epi, s.alpha.ptr, s.ra_d.ptr, pm2.ptr, ps2.ptr, stream())
    ok(lib, rc, "gemm_f16_scaled_rows_dev.stats.pp")
    torch.cuda.synchronize()
    bits = lambda g: kr.ibits(g.get())
    assert torch.equal(bits(s.C), bits(C2)), "the two entries stored different C"
    assert torch.equal(bits(s.pmax), bits(pm2)) and torch.equal(bits(s.psum), bits(ps2))
    assert not bool(torch.isnan(s.psum.get()).any())


def test_fused_refusals_launch_nothing_and_write_nothing(dev, lib):
    s = kx.build_x3(kx.X3Case("scaled", 257, 260, 64, 1, False), dev)
    lib.dclip_relu_f32(kc.Guarded(1, 64, device=dev).ptr, 64, stream())
    st = stream()
    K = 64
    assert kx.launch_x3(lib, s, st, K=48) == kc.E_INVAL and b"multiple of 32" in lib.dclip_last_error()     # K % 32 != 0
    assert kx.launch_x3(lib, s, st, K=0) == kc.E_INVAL
    for offs in [(4, K, 0, 2 * K), (0, K + 4, 0, 2 * K), (0, K, 12, 2 * K), (0, K, 0, 2 * K + 2), (-8, K, 0, 2 * K)]:                # misaligned
        assert kx.launch_x3(lib, s, st, offs=offs) == kc.E_INVAL, offs
    for offs in [(0, s.lda - K + 8, 0, 2 * K), (0, K, 0, s.ldw - K + 8), (s.lda, K, 0, 2 * K), (0, K, s.ldw - 8, 2 * K)]:            # outside ld
        assert kx.launch_x3(lib, s, st, offs=offs) == kc.E_INVAL, offs
        assert b"within the leading dimension" in lib.dclip_last_error()
    assert kx.launch_x3(lib, s, st, lda=s.lda + 4) == kc.E_INVAL and kx.launch_x3(lib, s, st, ldw=2 * K) == kc.E_INVAL
    assert lib.dclip_last_launch() == b"relu_f32", "a refused call launched"
    torch.cuda.synchronize()
    s.C.assert_guards("a refused call")
    assert bool(torch.isnan(s.C.get()).all()), "a refused call wrote"


# ------------------------------------------------------------------------------------------------ the token-major twin

@pytest.mark.parametrize("c", kx.tok_cases(), ids=kx.tok_id)
def test_fused_token_major_wgrad(dev, lib, c):
    s = kx.build_tok(c, dev)
    assert lib.dclip_gemm_f16x3_wgrad_tokmajor_workspace(c.M, c.N, s.s_eff) == s.ws_bytes
    ok(lib, kx.launch_tok(lib, s, stream()), kx.TOK_SITE)
    torch.cuda.synchronize()
    kc.record("f16x3_tok", tuple(c), kx.verify_tok(s))


def test_fused_token_major_refusals(dev, lib):
    c = kx.TokCase(264, 8, 192, 2, False)
    s = kx.build_tok(c, dev)
    lib.dclip_relu_f32(kc.Guarded(1, 64, device=dev).ptr, 64, stream())
    assert kx.launch_tok(lib, s, stream(), s.ws_bytes - 1) == kc.E_WORKSPACE
    assert str(s.ws_bytes).encode() in lib.dclip_last_error()
    good = [s.dyd.data_ptr(), s.xd.data_ptr(), s.C.ptr, c.M, c.N, c.tokens, s.lddy, s.ldx, s.C.ld, *s.offs, s.cad.ptr, s.act.ptr,
            c.splits, s.ws.ptr, s.ws_bytes, stream()]
    for at, value in [(3, 260), (4, 12), (5, 96), (15, 0), (15, 65), (6, s.lddy + 4), (7, s.ldx + 4), (8, c.N + 2), (8, c.N - 4), (9, 4),
                      (10, s.lddy - c.M + 8), (11, -8), (12, s.ldx - c.N + 8), (0, good[0] + 8), (2, good[2] + 4), (13, good[13] + 2),
                      (14, None), (13, None), (0, None)]:
        args = list(good)
        args[at] = value
        assert lib.dclip_gemm_f16x3_wgrad_tokmajor(*args) == kc.E_INVAL, (at, value)
    assert lib.dclip_last_launch() == b"relu_f32", "a refused call launched"
    torch.cuda.synchronize()
    s.C.assert_guards("a refused call")
    assert bool(torch.isnan(s.C.get()).all()) and bool(torch.isnan(s.ws.get()).all()), "a refused call wrote"


# ------------------------------------------------------------------------------------------------ real split data

def _split_pieces(shape, seed, scale):
    x = torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale
    return ks.host_split(x, 1.0)


def test_real_split_data_k_major(dev, lib, monkeypatch):
    """host_split of seeded fp32: the fused and the unfused entry each within the any-order bound of 3 K exact products
    accumulated in fp32 of the fp64 value of the same three products; two runs of the fused entry are bit-identical."""
    monkeypatch.setenv("DCLIP_BF16_BIG_MIN", "1")
    M, N, K = 300, 264, 192
    (ah, al), (wh, wl) = _split_pieces((M, K), 11, 40.0), _split_pieces((N, K), 12, 3.0)
    assert float(al.float().abs().max()) > 0 and float(wl.float().abs().max()) > 0
    want, bound = kx.split_bound(ah, al, wh, wl, K)
    A = torch.cat([ah, al, ah], 1).to(dev).contiguous()
    W = torch.cat([wh, wh, wl], 1).to(dev).contiguous()
    outs = [torch.full((M, N), float("nan"), device=dev) for _ in range(3)]
    st = stream()
    for o in outs[:2]:
        ok(lib, lib.dclip_gemm_f16x3_scaled(A.data_ptr(), W.data_ptr(), o.data_ptr(), None, None, M, N, K, 3 * K, 3 * K, N, 0, K, 0, 2 * K,
                                            0, 0, 1.0, st), "gemm_f16x3_scaled.pp3")
    ok(lib, lib.dclip_gemm_f16_scaled(A.data_ptr(), W.data_ptr(), outs[2].data_ptr(), None, None, M, N, 3 * K, 3 * K, 3 * K, N, 0, 0, 1.0, st),
       "gemm_f16_scaled.pp")
    torch.cuda.synchronize()
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "two runs of the fused entry differ"
    figs = {}
    for name, o in (("fused", outs[0]), ("unfused", outs[2])):
        err = (o.double().cpu() - want).abs()
        figs[name] = float((err / bound).max())
        print(f"k-major {name}: worst |err| / bound = {figs[name]:.4f}")
    assert figs["fused"] <= 1.0 and figs["unfused"] <= 1.0, figs


def test_real_split_data_token_major(dev, lib):
    M, N, tokens, splits = 264, 520, 192, 2
    (dh, dl), (xh, xl) = _split_pieces((tokens, M), 21, 40.0), _split_pieces((tokens, N), 22, 3.0)
    want, bound = kx.split_bound(dh.t(), dl.t(), xh.t(), xl.t(), tokens)
    dY = torch.cat([dh, dl], 1).to(dev).contiguous()
    X = torch.cat([xh, xl, xh], 1).to(dev).contiguous()
    ones = torch.ones(M, device=dev)
    act = torch.ones(1, device=dev)
    ws = torch.empty(3 * splits * M * N, device=dev)
    outs = [torch.full((M, N), float("nan"), device=dev) for _ in range(3)]
    st = stream()
    for o in outs[:2]:
        ok(lib, lib.dclip_gemm_f16x3_wgrad_tokmajor(dY.data_ptr(), X.data_ptr(), o.data_ptr(), M, N, tokens, 2 * M, 3 * N, N, 0, M, 0, N,
                                                    ones.data_ptr(), act.data_ptr(), splits, ws.data_ptr(), ws.numel() * 4, st), kx.TOK_SITE)
    ok(lib, lib.dclip_gemm_f16_wgrad_tokmajor_seg3(dY.data_ptr(), X.data_ptr(), outs[2].data_ptr(), M, N, tokens, 2 * M, 3 * N, N, 0, M, 0,
                                                   0, 0, N, ones.data_ptr(), act.data_ptr(), splits, ws.data_ptr(), ws.numel() * 4, st),
       ks.SEG_SITE)
    torch.cuda.synchronize()
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "two runs of the fused entry differ"
    figs = {}
    for name, o in (("fused", outs[0]), ("unfused", outs[2])):
        figs[name] = float(((o.double().cpu() - want).abs() / bound).max())
        print(f"token-major {name}: worst |err| / bound = {figs[name]:.4f}")
    assert figs["fused"] <= 1.0 and figs["unfused"] <= 1.0, figs
