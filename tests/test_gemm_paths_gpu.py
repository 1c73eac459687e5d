"""Every path of the fp32 GEMM (dclip_amd/csrc/gemm_f32.hip) through the C ABI: each tile forced with DCLIP_GEMM_TILE x each
layout x split-K x epilogue x leading-dimension padding on integer data (exact equality, guarded outputs, NaN-poisoned
operand padding), a Gaussian subset under the derived rounding bound, and the once-read switches (DCLIP_GEMM_DMA,
DCLIP_GEMM_GROUP_M) in one fresh process each.  The checkers and the case lists live in
tests/kernel_checks.py; tests/test_kernel_checks_cpu.py shows what they catch.  Every case asserts the tile, the split
count (dclip_gemm_f32_plan) and the kernel variant (dclip_last_launch) it was written for."""
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import kernel_checks as kc

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def set_env(monkeypatch, env):
    for k, v in env.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)


# ---- the once-read switches: first in the module, while this process holds little device memory ------------------------

STATIC_SETTINGS = [{"DCLIP_GEMM_DMA": "0"}, {"DCLIP_GEMM_GROUP_M": "1"}, {"DCLIP_GEMM_GROUP_M": "3"}, {"DCLIP_GEMM_GROUP_M": "8"}]
_child_ended_abnormally = []


@pytest.mark.parametrize("setting", STATIC_SETTINGS, ids=lambda s: "-".join(f"{k[11:]}{v}" for k, v in s.items()))
def test_integer_matrix_under_a_once_read_switch(setting):
    """The whole integer matrix in a fresh process per setting (the library reads these switches once).  A child that ends
    by signal, abort or timeout fails the test, and no further child is started."""
    assert not _child_ended_abnormally, f"not started: an earlier child ended abnormally ({_child_ended_abnormally[0]})"
    env = {k: v for k, v in os.environ.items() if not k.startswith("DCLIP_GEMM_")}
    env.update(setting)
    try:
        r = subprocess.run([sys.executable, "-m", "tests.gemm_paths_child"], cwd=REPO, env=env, capture_output=True, text=True,
                           timeout=600)
    except subprocess.TimeoutExpired:
        _child_ended_abnormally.append(f"{setting}: timeout")
        pytest.fail(f"{setting}: the child did not finish in 600 s")
    if r.returncode != 0:
        _child_ended_abnormally.append(f"{setting}: exit status {r.returncode}")
        pytest.fail(f"{setting}: child exit status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(out)
    assert out["switches"] == setting
    assert out["cases"] == len(kc.integer_matrix()) and not out["failed"], out["failed"][:5]
    if "DCLIP_GEMM_DMA" in setting:
        assert "gemm_f32.dma" not in out["sites"]
    else:
        assert out["sites"].get("gemm_f32.dma", 0) > 0


# ---- the matrix in this process (default statics: LDS-DMA staging on, 4 tile-rows per group) ---------------------------

@pytest.mark.parametrize("case", kc.integer_matrix(), ids=kc.case_id)
def test_integer_matrix(dev, lib, monkeypatch, case):
    set_env(monkeypatch, kc.gemm_env(case))
    fig = kc.run_gemm_on_device(lib, case, dev, stream())
    kc.record("gemm_int", case, fig)


@pytest.mark.parametrize("case", kc.gaussian_matrix(), ids=kc.case_id)
def test_gaussian_subset_under_the_derived_bound(dev, lib, monkeypatch, case):
    set_env(monkeypatch, kc.gemm_env(case))
    fig = kc.run_gemm_on_device(lib, case, dev, stream())
    print(kc.case_id(case), fig)
    kc.record("gemm_gauss", case, fig)


@pytest.mark.parametrize("tile", kc.TILES, ids=lambda t: f"{t[0]}x{t[1]}")
@pytest.mark.parametrize("split,epi", [(3, 0), (7, kc.EPI_A_ROWSUM | kc.EPI_ACCUM), (2, kc.EPI_BIAS | kc.EPI_GELU)])
def test_split_k_is_bitwise_deterministic_on_every_tile(dev, lib, monkeypatch, tile, split, epi):
    layout = 0 if epi & kc.EPI_A_ROWSUM else 3
    M, N, K = (360, 320, 896) if split == 7 else (616, 1536, 512)          # K / split a multiple of 32: exactly `split` slabs
    case = kc.GemmCase(M, N, K, layout, tile, split, epi, kc._alpha(epi), (4, 0, 36), "gauss", None)
    set_env(monkeypatch, kc.gemm_env(case))
    assert kc.assert_gemm_plan(lib, case)[2] == split
    runs = []
    for _ in range(2):
        s = kc.build_gemm(case, dev)
        assert kc.launch_gemm(lib, s, stream()) == 0
        torch.cuda.synchronize()
        kc.verify_gemm(s)
        runs.append([s.C.get()] + [g.get() for g in (s.aux, s.rowsum) if g is not None])
    for x, y in zip(*runs):
        assert torch.equal(x, y), "split-K must be run-to-run deterministic"


@pytest.mark.parametrize("tile", kc.TILES, ids=lambda t: f"{t[0]}x{t[1]}")
def test_short_split_k_workspace_is_refused_and_nothing_is_written(dev, lib, monkeypatch, tile):
    case = kc.GemmCase(300, 256, 192, 0, tile, 3, kc.EPI_A_ROWSUM, 1.0, (0, 4, 36), "int", None)
    set_env(monkeypatch, kc.gemm_env(case))
    need = int(lib.dclip_gemm_f32_workspace(case.M, case.N, case.K, case.layout, case.split))
    assert need == 3 * (case.M * case.N + case.M) * 4
    s = kc.build_gemm(case, dev)
    ws = kc.Guarded(1, need // 4, device=dev, guard_rows=1)           # a long vector: one more of itself on each side
    rc = kc.launch_gemm(lib, s, stream(), workspace=ws.mat, workspace_bytes=need - 4)
    torch.cuda.synchronize()
    assert rc == kc.E_WORKSPACE and b"workspace" in lib.dclip_last_error()
    for g in (s.C, s.rowsum, ws):
        g.assert_guards("short workspace")
        assert bool(torch.isnan(g.get()).all()), "a refused call wrote to its output"
    assert kc.launch_gemm(lib, s, stream(), workspace=ws.mat, workspace_bytes=need) == 0       # exactly enough: accepted
    torch.cuda.synchronize()
    ws.assert_guards("split-K workspace")
    kc.verify_gemm(s)


# ---- the contrastive gradient: a GEMM with lda = ldw > K = Bg over a workspace whose padding holds anything ---------------

@pytest.mark.parametrize("Bl,Bg,P,offset", [(3, 5, 64, 2), (37, 37, 768, 0), (200, 1001, 512, 400), (64, 130, 512, 66)])
def test_contrastive_lse_and_grad_on_a_poisoned_workspace(dev, lib, Bl, Bg, P, offset):
    inv_t, coef = 20.0, 0.37
    g = torch.Generator().manual_seed(Bl + Bg)
    a = torch.nn.functional.normalize(torch.randn((Bl, P), generator=g), dim=1)
    b = torch.randn((Bg, P), generator=g)
    b[offset:offset + Bl] += 0.3 * a
    b = torch.nn.functional.normalize(b, dim=1)
    z = (a.double() @ b.double().t()) * inv_t
    need = int(lib.dclip_contrastive_workspace(Bl, Bg, P))
    ws = kc.Guarded(1, need // 4, device=dev, guard_rows=1)      # NaN payload: the W padding columns Bg..ldw are poison
    ad, bd = a.to(dev), b.to(dev)
    lse, diag = kc.Guarded(1, Bl, device=dev), kc.Guarded(1, Bl, device=dev)
    rc = lib.dclip_contrastive_lse(ad.data_ptr(), bd.data_ptr(), lse.ptr, diag.ptr, Bl, Bg, P, offset, inv_t, ws.ptr, need, stream())
    assert rc == 0, lib.dclip_last_error()
    torch.cuda.synchronize()
    for gd in (lse, diag, ws):
        gd.assert_guards("contrastive_lse")
    idx = torch.arange(Bl)
    fig = kc.check_blocks({"lse": (lse.get()[0], torch.logsumexp(z, 1), 1e-5), "diag": (diag.get()[0], z[idx, idx + offset], 1e-5)},
                          "contrastive_lse")
    ws.payload.fill_(kc.NAN)
    lse_row = torch.logsumexp(z, 1).float()
    lse_col = torch.randn((Bg,), generator=g).abs() + 4.0
    w = torch.exp(z - lse_row.double()[:, None]) + torch.exp(z - lse_col.double()[None, :])
    w[idx, idx + offset] -= 2.0
    da = kc.Guarded(Bl, P, device=dev)
    lr, lc = lse_row.to(dev), lse_col.to(dev)
    rc = lib.dclip_contrastive_grad(ad.data_ptr(), bd.data_ptr(), lr.data_ptr(), lc.data_ptr(), da.ptr, Bl, Bg, P, offset, inv_t,
                                    coef, ws.ptr, need, stream())
    assert rc == 0, lib.dclip_last_error()
    assert lib.dclip_last_launch() in (b"gemm_f32", b"gemm_f32.dma")
    torch.cuda.synchronize()
    da.assert_guards("contrastive_grad")
    ws.assert_guards("contrastive_grad workspace")
    fig.update(kc.check_blocks({"da": (da.get(), coef * (w @ b.double()), 2e-5)}, "contrastive_grad"))
    print(fig)
    assert lib.dclip_contrastive_grad(ad.data_ptr(), bd.data_ptr(), lr.data_ptr(), lc.data_ptr(), da.ptr, Bl, Bg, P, offset, inv_t,
                                      coef, ws.ptr, Bl * kc.roundup(Bg, 4) * 4 - 4, stream()) == kc.E_WORKSPACE
