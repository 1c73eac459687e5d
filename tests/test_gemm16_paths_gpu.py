"""Every path of the 16-bit GEMM file (dclip_amd/csrc/gemm_bf16.hip) through the C ABI: the kernel variants x the three
element types x every epilogue the dispatcher accepts x leading-dimension padding on integer data (bit-exact C and saved
pre-activation, guarded outputs, NaN-poisoned operand padding), the two split-K entries and the token-major weight gradient
with their workspace, a Gaussian subset under the derived bound, and the cast and LayerNorm-16 kernels that live in the same
file.  Checkers and case lists: tests/kernel_checks.py; tests/test_kernel_checks16_cpu.py shows what they catch.  Every case
asserts the kernel variant dclip_last_launch reports."""
import pytest
import torch

from tests import kernel_checks as kc

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


def set_env(monkeypatch, env):
    for k, v in env.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)


@pytest.fixture(autouse=True)
def _nothing_starts_after_an_abnormal_child():
    kc.assert_no_child_ended_abnormally()


# ---- the matrix in this process ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", kc.gemm16_matrix(), ids=kc.case16_id)
def test_integer_matrix(dev, lib, monkeypatch, case):
    set_env(monkeypatch, kc.gemm16_env(case))
    fig = kc.run_gemm16_on_device(lib, case, dev, stream())
    kc.record("gemm16_int", case, fig)


@pytest.mark.parametrize("case", kc.gemm16_gaussian_matrix(), ids=kc.case16_id)
def test_gaussian_subset_under_the_derived_bound(dev, lib, monkeypatch, case):
    set_env(monkeypatch, kc.gemm16_env(case))
    fig = kc.run_gemm16_on_device(lib, case, dev, stream())
    print(kc.case16_id(case), fig)
    kc.record("gemm16_gauss", case, fig)


def test_every_variant_of_the_file_has_a_case():
    sites = {kc.expected_gemm16_site(c) for c in kc.gemm16_matrix()}
    for ty in ("gemm_bf16", "gemm_f16"):
        assert {f"{ty}.{v}" for v in ("r64", "r128", "pp", "ppp")} <= sites
    assert {"gemm_f16_ex.r64", "gemm_f16_ex.r128", "gemm_f16_ex.pp"} <= sites
    for ty in ("bf16", "f16"):
        assert {f"gemm_{ty}_splitk.r64", f"gemm_{ty}_splitk.r128.splitk_reduce", f"gemm_{ty}_splitk.pp.splitk_reduce",
                f"gemm_{ty}_wgrad_tokmajor.pp_tok", f"gemm_{ty}_wgrad_tokmajor.pp_tok.splitk_reduce"} <= sites


@pytest.mark.parametrize("ty", ["bf16", "f16ex"])
@pytest.mark.parametrize("entry,shape,splits", [("splitk", (300, 256, 149), 3), ("splitk", (2047, 2044, 192), 7),
                                                ("tok", (264, 248, 192), 7)])
def test_split_k_workspace_size_and_refusal(dev, lib, monkeypatch, ty, entry, shape, splits):
    M, N, K = shape
    case = kc._c16(entry, ty, (M, N), K, kc.EPI16[0], 4, splits=splits, want="pp_tok" if entry == "tok" else ("pp" if M > 2000 else "r128"))
    set_env(monkeypatch, kc.gemm16_env(case))
    s_eff = kc.s_eff16(K, splits)
    assert 1 < s_eff == -(-K // kc.roundup(-(-K // splits), 64)) <= splits
    need = s_eff * M * N * 4
    helper = getattr(lib, f"dclip_gemm_{'bf16' if ty == 'bf16' else 'f16'}_splitk_workspace")
    assert int(helper(M, N, s_eff)) == need and int(helper(M, N, splits)) >= need and int(helper(M, N, 1)) == 0
    s = kc.build_gemm16(case, dev)
    rc = kc.launch_gemm16(lib, s, stream(), workspace_bytes=need - 1)
    torch.cuda.synchronize()
    assert rc == kc.E_WORKSPACE and b"workspace" in lib.dclip_last_error()
    for g in (s.C, s.ws):
        g.assert_guards("short workspace")
        assert bool(torch.isnan(g.get()).all()), "a refused call wrote to its output"
    assert kc.launch_gemm16(lib, s, stream(), workspace_bytes=need) == 0          # exactly enough: accepted
    assert lib.dclip_last_launch().decode() == kc.expected_gemm16_site(case)
    torch.cuda.synchronize()
    kc.verify_gemm16(s)


def test_plans_are_consistent_with_what_the_entries_accept(lib):
    for M, N, K in [(768, 768, 12800), (3072, 768, 12800), (768, 3072, 12800), (512, 768, 6400), (300, 256, 149), (64, 64, 64)]:
        for ty in ("bf16", "f16"):
            sp = int(getattr(lib, f"dclip_gemm_{ty}_splitk_plan")(M, N, K))
            tk = int(getattr(lib, f"dclip_gemm_{ty}_wgrad_tokmajor_plan")(M, N, K))
            assert 1 <= sp <= 64 and 0 <= tk <= 64, (M, N, K, sp, tk)
            assert tk == 0 or (K % 64 == 0 and M % 8 == 0 and N % 8 == 0)
    assert int(lib.dclip_gemm_bf16_wgrad_tokmajor_plan(768, 768, 12800)) > 1 and int(lib.dclip_gemm_bf16_splitk_plan(768, 768, 12800)) > 1
    assert int(lib.dclip_gemm_bf16_splitk_plan(300, 256, 149)) == 1 and int(lib.dclip_gemm_bf16_wgrad_tokmajor_plan(300, 252, 128)) == 0


@pytest.mark.parametrize("what", ["residual_16bit_out", "dgelu_without_aux", "dgelu_on_gemm_f16"])
def test_documented_rejections_leave_the_output_untouched(dev, lib, what):
    e = {"residual_16bit_out": (kc.EPI_BIAS | kc.EPI_RESIDUAL, 1, 0), "dgelu_without_aux": (kc.EPI_DGELU, 0, 1),
         "dgelu_on_gemm_f16": (kc.EPI_DGELU, 0, 1)}[what]
    for ty in (("f16",) if what == "dgelu_on_gemm_f16" else ("bf16", "f16ex")):
        case = kc._c16("gemm", "bf16" if ty == "f16" else ty, (129, 132), 72, e, 13)
        s = kc.build_gemm16(case, dev)
        if what == "residual_16bit_out":
            rc = kc.launch_gemm16(lib, s, stream())
        elif what == "dgelu_without_aux":
            s.auxin_d = None
            rc = kc.launch_gemm16(lib, s, stream())
        else:
            rc = lib.dclip_gemm_f16(s.A.data_ptr(), s.W.data_ptr(), s.C.ptr, None, None, case.M, case.N, case.K, s.lda, s.ldw, s.ldc,
                                    kc.EPI_DGELU, 0, stream())
        torch.cuda.synchronize()
        assert rc == kc.E_INVAL and lib.dclip_last_error(), (what, ty, rc)
        s.C.assert_guards(what)
        assert bool(torch.isnan(s.C.get()).all()), "a refused call wrote to its output"


# ---- cast ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ty", ["bf16", "f16", "f16ex"])
@pytest.mark.parametrize("shape", kc.CAST_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_cast_is_the_types_rounding_bit_for_bit(dev, lib, ty, shape):
    """cols % 4 != 0, ldx > cols (NaN padding), ldy > cols (the zero fill the kernel is specified to write: asserted, and guarded
    beyond ldy), one row and 12800 x 768; +-65504, +-65520, +-1e6, +-inf, NaN and subnormals of the target type included."""
    rows, cols, ldx, ldy = shape
    t = kc.TYPES16[ty]
    x = kc.cast_input(rows, cols)
    xd = kc.poisoned(x, ldx, dev)
    y = kc.Guarded(rows, ldy, device=dev, dtype=t.dtype)
    fn = {"bf16": lib.dclip_cast_f32_bf16, "f16": lib.dclip_cast_f32_f16, "f16ex": lib.dclip_cast_f32_f16_ieee}[ty]
    assert fn(xd.data_ptr(), y.ptr, rows, cols, ldx, ldy, stream()) == 0, lib.dclip_last_error()
    torch.cuda.synchronize()
    y.assert_guards("cast")
    got, want = y.get(), kc.round16(x, t)
    assert torch.equal(torch.isnan(got[:, :cols]), torch.isnan(want)), "NaN must stay NaN, and nothing else may become one"
    g, w = torch.nan_to_num(got[:, :cols].float(), nan=0.0).to(t.dtype), torch.nan_to_num(want.float(), nan=0.0).to(t.dtype)
    assert torch.equal(g.view(torch.int16), w.view(torch.int16)), kc._first_diff(g.float(), w.float())
    assert bool((got[:, cols:].view(torch.int16) == 0).all()), "columns cols..ldy must be zero-filled"


# ---- LayerNorm-16 -------------------------------------------------------------------------------------------------------------

LN_FN = {("bf16", False): "layernorm_fwd_bf16", ("bf16", True): "layernorm_fwd_bf16_stats", ("f16", False): "layernorm_fwd_f16",
         ("f16ex", True): "layernorm_fwd_f16_stats", ("f16ex", False): "layernorm_fwd_f16_stats"}
LN_CASES = [(D, rows, ty, stats) for i, D in enumerate(kc.LN16_D) for j, rows in enumerate(kc.LN16_ROWS)
            for ty, stats in [list(LN_FN)[(i + j) % 5]]] + \
           [(D, 5, ty, stats) for D in kc.LN16_D for ty, stats in LN_FN]                  # every instance x every entry


def call_ln(lib, ty, stats, x, g, b, y, mean, rstd, rows, D):
    name = LN_FN[(ty, stats)]
    fn = getattr(lib, "dclip_" + name)
    if name.endswith("_stats"):
        rc = fn(x.data_ptr(), g.data_ptr(), b.data_ptr(), y.ptr, mean.ptr if stats else None, rstd.ptr if stats else None, rows, D,
                1e-5, stream())
        return rc, "layernorm_fwd_bf16" if ty == "bf16" else name
    return fn(x.data_ptr(), g.data_ptr(), b.data_ptr(), y.ptr, rows, D, 1e-5, stream()), name


@pytest.mark.parametrize("D,rows,ty,stats", sorted(set(LN_CASES)), ids=lambda v: str(int(v) if isinstance(v, bool) else v))
def test_layernorm16_every_instance(dev, lib, D, rows, ty, stats):
    t = kc.TYPES16[ty]
    gen = torch.Generator().manual_seed(D + rows)
    x = torch.randn((rows, D), generator=gen) * 2.0 + 1.0
    g, b = torch.randn((D,), generator=gen), torch.randn((D,), generator=gen)
    y = kc.Guarded(rows, D, device=dev, dtype=t.dtype)
    mean, rstd = kc.Guarded(1, rows, device=dev), kc.Guarded(1, rows, device=dev)
    xd = kc.poisoned(x, D, dev)                                    # NaN rows behind x
    rc, name = call_ln(lib, ty, stats, xd, g.to(dev), b.to(dev), y, mean, rstd, rows, D)
    assert rc == 0, lib.dclip_last_error()
    assert lib.dclip_last_launch().decode() == name + kc.expected_ln16_variant(D)
    torch.cuda.synchronize()
    for gd in (y, mean, rstd):
        gd.assert_guards("layernorm16")
    if not stats:
        assert bool(torch.isnan(mean.get()).all()) and bool(torch.isnan(rstd.get()).all())
    fig = kc.verify_ln16(y.get(), mean.get()[0] if stats else None, rstd.get()[0] if stats else None, x, g, b, 1e-5, t,
                         f"ln16 {ty} D={D} rows={rows}")
    kc.record("ln16", (ty, D, rows, stats), fig)


@pytest.mark.parametrize("ty,stats", list(LN_FN))
@pytest.mark.parametrize("D", [2052, 6])
def test_layernorm16_rejects_what_no_instance_handles(dev, lib, ty, stats, D):
    x = torch.zeros((4, D), device=dev)
    g = torch.ones((D,), device=dev)
    y = kc.Guarded(4, D, device=dev, dtype=kc.TYPES16[ty].dtype)
    mean, rstd = kc.Guarded(1, 4, device=dev), kc.Guarded(1, 4, device=dev)
    rc, _ = call_ln(lib, ty, stats, x, g, g, y, mean, rstd, 4, D)
    torch.cuda.synchronize()
    assert rc == kc.E_INVAL and b"bad D" in lib.dclip_last_error()
    y.assert_guards("refused layernorm")
    assert bool(torch.isnan(y.get()).all())
