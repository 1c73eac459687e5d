"""The 192-row tile of the fused split-fp16 GEMM entries through the C ABI.

Exactness: the integer-data cases of tests/kernel_checks_f16x3.py (four independent pieces, NaN in the duplicate third and in all
padding, guarded C) forced onto the tile with DCLIP_F16X3_BM192=2 and the launch site asserted, at the heights where the tile's
row geometry changes: M = 97 (wave row 1 holds one row), 192 (one exact tile), 193 (a second tile of one row), 300 (a second tile
with 12 rows in wave row 1), 385 (three tiles), and 1733 x 520 (tiles_m = 10 > 8: a partial rasterisation group).
Bit-equality: on operands split by the library's own split entries the same call at DCLIP_F16X3_BM192=0 and =2 stores equal bits
— every accumulator sees the same MFMAs in the same order and the same epilogue statements.
Fallbacks: the forms without the tile keep `.pp3` and the 256-row bits under =2, and =1 at default thresholds keeps `.pp3`."""
import pytest
import torch

from tests import kernel_checks as kc
from tests import kernel_checks_f16x3 as kx
from tests import kernel_checks_split16 as ks

pytestmark = pytest.mark.gpu

# forms of this file beside kernel_checks_f16x3's ("scaled" = bias + residual, "rows_dev", "rows_dgelu"): added under names of
# their own, so that module's case lists (built from its X3_ENTRIES at import) are what they were
kx.X3_FORMS.setdefault("t192_scaled_bias", dict(fn="scaled", epi=ks.EPI_BIAS))
kx.X3_FORMS.setdefault("t192_scaled_dev_res", dict(fn="scaled_dev", epi=ks.EPI_RESIDUAL))
FORMS = ["t192_scaled_bias", "scaled", "t192_scaled_dev_res", "rows_dev", "rows_dgelu"]
T_M, T_N = [97, 192, 193, 300, 385], [260, 520]


def t192_cases():
    """Every form at every K; the height, the width, the padding of C and the segment order rotate as x3_cases() does."""
    out = []
    for j, e in enumerate(FORMS):
        for i, K in enumerate(kx.X3_K):
            dgelu = bool(kx.X3_FORMS[e]["epi"] & ks.EPI_DGELU)
            out.append(kx.X3Case(e, T_M[(i + j) % 5], T_N[(i + j // 2) % 2], K, 1 if dgelu else (i + j) % 2, bool((i + j // 3) % 2)))
    out.append(kx.X3Case("scaled", 1733, 520, 64, 0, False))        # tiles_m = 10: the second rasterisation group has 2 tile rows
    return out


def site192(c) -> str:
    return kx.X3_NAMES[kx.X3_FORMS[c.entry]["fn"]] + ".pp3_192"


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


def test_the_case_list_covers_every_height_width_and_k():
    cs = t192_cases()
    assert {c.M for c in cs} >= set(T_M) and {c.N for c in cs} == set(T_N) and {c.K for c in cs} == set(kx.X3_K)
    for e in FORMS:
        assert {c.K for c in cs if c.entry == e} == set(kx.X3_K)
    for M in T_M:                                          # every height meets a short and a long K loop
        ks_ = {c.K for c in cs if c.M == M}
        assert min(ks_) <= 64 and max(ks_) >= 96, (M, ks_)


# ------------------------------------------------------------------------------------------------ exactness on integer data

@pytest.mark.parametrize("c", t192_cases(), ids=kx.x3_id)
def test_tile192_entries_exact(dev, lib, monkeypatch, c):
    monkeypatch.setenv("DCLIP_F16X3_BM192", "2")
    assert lib.dclip_gemm_f16x3_tile_rows(c.M, c.N, c.K, int(kx.X3_FORMS[c.entry]["fn"] == "rows_dev"), 0) == 192
    s = kx.build_x3(c, dev)
    ok(lib, kx.launch_x3(lib, s, stream()), site192(c))
    torch.cuda.synchronize()
    kc.record("f16x3_tile192", tuple(c), kx.verify_x3(s))


# ------------------------------------------------------------------------------------------------ bit-equality on real split data

def _operands(dev, M, N, K, seed):
    from dclip_amd import ops
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn((M, K), generator=g) * 3.0).to(dev)
    w = (torch.randn((N, K), generator=g) * 0.5).to(dev)
    o = dict(a=ops.split_f16x3(x, 4.0, 0), w=ops.split_f16x3(w, 8.0, 1),
             bias=torch.randn(N, generator=g).to(dev), res=torch.randn((M, N), generator=g).to(dev),
             h=torch.randn((M, N), generator=g).to(dev), alpha=torch.full((1,), 2.0 ** -5, device=dev))
    o["a_rows"], o["row_alpha"] = ops.split_f16x3_rows(x)
    return o


def _calls():
    """name -> (launch site without the tile suffix, call on the operands): the three instances, every epilogue kind they take."""
    from dclip_amd import ops
    ap = lambda o: o["alpha"].data_ptr()
    return {
        "plain_bias": ("gemm_f16x3_scaled", lambda o: ops.gemm_f16x3(o["a"], o["w"], bias=o["bias"], alpha=2.0 ** -5)),
        "plain_bias_gelu": ("gemm_f16x3_scaled", lambda o: ops.gemm_f16x3(o["a"], o["w"], bias=o["bias"], gelu=True, alpha=2.0 ** -5)),
        "plain_bias_res": ("gemm_f16x3_scaled",
                           lambda o: ops.gemm_f16x3(o["a"], o["w"], bias=o["bias"], residual=o["res"], alpha=2.0 ** -5)),
        "dev_none": ("gemm_f16x3_scaled_dev", lambda o: ops.gemm_f16x3_dev(o["a"], o["w"], ap(o))),
        "dev_bias_gelu": ("gemm_f16x3_scaled_dev", lambda o: ops.gemm_f16x3_dev(o["a"], o["w"], ap(o), bias=o["bias"], gelu=True)),
        "dev_res": ("gemm_f16x3_scaled_dev", lambda o: ops.gemm_f16x3_dev(o["a"], o["w"], ap(o), residual=o["res"])),
        "rows_none": ("gemm_f16x3_scaled_rows_dev", lambda o: ops.gemm_f16x3_rows_dev(o["a_rows"], o["w"], ap(o), o["row_alpha"])),
        "rows_dgelu": ("gemm_f16x3_scaled_rows_dev",
                       lambda o: ops.gemm_f16x3_rows_dev(o["a_rows"], o["w"], ap(o), o["row_alpha"], dgelu_h=o["h"])),
    }


@pytest.fixture(scope="module", params=[(300, 264, 192), (1733, 520, 96)], ids=lambda s: "x".join(map(str, s)))
def operands(request, dev):
    M, N, K = request.param
    return _operands(dev, M, N, K, 7 * M + K)


@pytest.mark.parametrize("name", list(_calls()))
def test_tile192_bits_equal_tile256(dev, lib, monkeypatch, operands, name):
    site, call = _calls()[name]
    outs = {}
    for mode, suffix in (("0", ".pp3"), ("2", ".pp3_192"), ("2", ".pp3_192")):
        monkeypatch.setenv("DCLIP_F16X3_BM192", mode)
        y = call(operands)
        assert lib.dclip_last_launch() == (site + suffix).encode(), (lib.dclip_last_launch(), site + suffix)
        outs.setdefault(mode, []).append(y)
    torch.cuda.synchronize()
    y256, (y192, again) = outs["0"][0], outs["2"]
    assert bool(torch.isfinite(y256).all()) and float(y256.abs().max()) > 0
    assert torch.equal(y192.view(torch.int32), again.view(torch.int32)), "two runs on the 192-row tile differ"
    assert torch.equal(y192.view(torch.int32), y256.view(torch.int32)), "the 192-row tile and the 256-row tile stored different bits"


# ------------------------------------------------------------------------------------------------ fallbacks

@pytest.mark.parametrize("entry", ["rows_stats", "rows_stats_dgelu", "split", "split_dev_g32", "split_dev_gelu_hg"])
def test_forms_without_the_tile_keep_256_rows(dev, lib, monkeypatch, entry):
    c = kx.X3Case(entry, 300, 264, 96, 1, False)
    got = []
    for mode in ("0", "2"):
        monkeypatch.setenv("DCLIP_F16X3_BM192", mode)
        s = kx.build_x3(c, dev)
        ok(lib, kx.launch_x3(lib, s, stream()), kx.x3_site(c))
        torch.cuda.synchronize()
        kx.verify_x3(s)
        got.append([g.get().clone() for g in (s.C, s.pmax, s.psum, s.g32, s.h32) if g is not None])
    for a, b in zip(*got):
        assert torch.equal(a.view(torch.int16 if a.dtype == torch.float16 else torch.int32),
                           b.view(torch.int16 if b.dtype == torch.float16 else torch.int32))
    assert lib.dclip_gemm_f16x3_tile_rows(c.M, c.N, c.K, 1, 1) == 256


def test_a_16_bit_output_keeps_256_rows(dev, lib, monkeypatch, operands):
    from dclip_amd import ops
    outs = []
    for mode in ("0", "2"):
        monkeypatch.setenv("DCLIP_F16X3_BM192", mode)
        outs.append(ops.gemm_f16x3(operands["a"], operands["w"], bias=operands["bias"], out_f16=True, alpha=2.0 ** -5))
        assert lib.dclip_last_launch() == b"gemm_f16x3_scaled.pp3"
    torch.cuda.synchronize()
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))


def test_the_plan_keeps_small_shapes_on_256_rows(dev, lib, monkeypatch, operands):
    """DCLIP_F16X3_BM192=1 (and unset) at the default DCLIP_F16X3_BM192_MIN: a few tiles are far below the threshold."""
    from dclip_amd import ops
    monkeypatch.delenv("DCLIP_F16X3_BM192_MIN", raising=False)
    for mode in (None, "1"):
        if mode is None:
            monkeypatch.delenv("DCLIP_F16X3_BM192", raising=False)
        else:
            monkeypatch.setenv("DCLIP_F16X3_BM192", mode)
        for name, (site, call) in _calls().items():
            call(operands)
            assert lib.dclip_last_launch() == (site + ".pp3").encode(), (mode, name, lib.dclip_last_launch())
    M, N = operands["res"].shape
    assert ops.gemm_f16x3_tile_rows(M, N, 96) == 256 and ops.gemm_f16x3_tile_rows(M, N, 96, rows_form=True) == 256
    torch.cuda.synchronize()
