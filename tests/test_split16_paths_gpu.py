"""Every launch site of dclip_amd/csrc/split16.hip through the C ABI: the stand-alone split, the row split, the
fused row / column pass, LayerNorm with split output, the device plan, the segmented weight-gradient GEMM of gemm_bf16.hip and
the five scaled GEMM entries on every kernel they can take.  Outputs live in guarded NaN-filled buffers, every
operand element the contract says is not read is NaN, dclip_last_launch() is asserted in full, and the references are the
restatements of tests/kernel_checks_split16.py (fp64 / integer arithmetic), never a sibling kernel.  A refused call launches
nothing and writes nothing."""
import pytest
import torch

from tests import kernel_checks as kc
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


def other_launch(lib, dev):
    """Some other launch site: a refused call must leave this name standing."""
    lib.dclip_relu_f32(kc.Guarded(1, 64, device=dev).ptr, 64, stream())
    assert lib.dclip_last_launch() == b"relu_f32"


def untouched(lib, *bufs):
    assert lib.dclip_last_launch() == b"relu_f32", "a refused call launched"
    torch.cuda.synchronize()
    for g in bufs:
        g.assert_guards("a refused call")
        assert bool(torch.isnan(g.get().float()).all()), "a refused call wrote"


# ------------------------------------------------------------------------------------------------ 1. the stand-alone split

@pytest.mark.parametrize("c", ks.split_cases(), ids=ks.split_id)
def test_split(dev, lib, c):
    s = ks.build_split(c, dev)
    ok(lib, ks.launch_split(lib, s, stream()), ks.split_site(c))
    torch.cuda.synchronize()
    kc.record("split16_split", tuple(c), ks.verify_split(s))


@pytest.mark.parametrize("c", ks.split_big_cases(), ids=ks.split_id)
def test_split_second_grid_stride_trip(dev, lib, c):
    """More than 8192 x 256 groups of 8 columns: the last rows are written by threads on their second trip."""
    need = 8 * c.rows * (c.cols + c.xpad) + 4 * (c.rows + 256) * (3 * c.cols + c.ypad) + (1 << 28)
    if torch.cuda.mem_get_info()[0] < need:
        pytest.skip("not enough device memory")
    s = ks.build_split(c, dev)
    ok(lib, ks.launch_split(lib, s, stream()), ks.split_site(c))
    torch.cuda.synchronize()
    kc.record("split16_split", tuple(c), ks.verify_split(s))


def test_split_refusals_launch_nothing_and_write_nothing(dev, lib):
    c = ks.SplitCase(3, 72, 4, 8, 0, True, 0)
    s = ks.build_split(c, dev)
    x, y, sc, st = s.xd.data_ptr(), s.y.ptr, s.scale.ptr, stream()
    other_launch(lib, dev)
    host = [x, y, 3, 72, 76, 224, 1.0, 0, st]
    devc = [x, y, 3, 72, 76, 224, sc, 0, st]
    bad = [(3, 76), (3, 12), (4, 74), (4, 68), (5, 208), (5, 220), (7, 2), (7, -1), (0, x + 4), (1, y + 8), (0, None), (1, None), (2, 0)]
    for at, value in bad:
        for fn, good in ((lib.dclip_split_f32_f16x3, host), (lib.dclip_split_f32_f16x3_dev, devc)):
            args = list(good)
            args[at] = value
            assert fn(*args) == kc.E_INVAL, (at, value)
            assert lib.dclip_last_error()
    for scale in (3.0, 0.0, -2.0, float("inf"), float("nan")):                  # the scalar entry: not a power of two
        args = list(host)
        args[6] = scale
        assert lib.dclip_split_f32_f16x3(*args) == kc.E_INVAL, scale
    assert lib.dclip_split_f32_f16x3_dev(*(devc[:6] + [None] + devc[7:])) == kc.E_INVAL
    assert lib.dclip_split_f32_f16x3_dev(*(devc[:6] + [sc + 2] + devc[7:])) == kc.E_INVAL
    untouched(lib, s.y)


# ------------------------------------------------------------------------------------------------ 2. the row split

@pytest.mark.parametrize("c", ks.rows_cases(), ids=ks.rows_id)
def test_row_split(dev, lib, c):
    s = ks.build_rows(c, dev)
    ok(lib, ks.launch_rows(lib, s, stream()), ks.rows_site(c))
    torch.cuda.synchronize()
    kc.record("split16_rows", tuple(c), ks.verify_rows(s))


def test_row_split_refusals(dev, lib):
    s = ks.build_rows(ks.RowsCase(3, 72, 4, "random"), dev)
    other_launch(lib, dev)
    good = [s.xd.data_ptr(), s.y.ptr, s.ra.ptr, 3, 72, 76, stream()]
    for at, value in [(4, 76), (5, 74), (5, 68), (0, good[0] + 4), (1, good[1] + 8), (2, good[2] + 2), (0, None), (1, None), (2, None), (3, 0)]:
        args = list(good)
        args[at] = value
        assert lib.dclip_split_f32_f16x3_rows(*args) == kc.E_INVAL, (at, value)
    untouched(lib, s.y, s.ra)


# ------------------------------------------------------------------------------------------------ 3. the fused pass

def run_col(lib, s):
    first, last = ks.col_sites(s.case)
    ok(lib, ks.launch_col(lib, s, stream()), last)
    assert lib.dclip_first_launch() == first.encode(), (lib.dclip_first_launch(), first)
    torch.cuda.synchronize()


@pytest.mark.parametrize("c", ks.col_cases(), ids=ks.col_id)
def test_fused_pass(dev, lib, c):
    s = ks.build_col(c, dev)
    assert lib.dclip_split_f32_f16x3_rows_colstats_workspace(c.rows, c.cols) == s.ws_bytes == 4 * ks.col_workspace_floats(c.rows, c.cols)
    run_col(lib, s)
    kc.record("split16_colstats", tuple(c), ks.verify_col(s))
    before = ks.col_outputs(s)
    run_col(lib, s)                                        # on the used workspace: the same bits
    assert all(torch.equal(a, b) for a, b in zip(before, ks.col_outputs(s)))
    ks.verify_col(s)


@pytest.mark.parametrize("c", ks.col_big_cases(), ids=ks.col_id)
def test_fused_pass_second_grid_stride_trip_of_the_column_split(dev, lib, c):
    if torch.cuda.mem_get_info()[0] < 20 * c.rows * c.cols + (1 << 28):
        pytest.skip("not enough device memory")
    s = ks.build_col(c, dev)
    run_col(lib, s)
    kc.record("split16_colstats", tuple(c), ks.verify_col(s))


@pytest.mark.parametrize("c", [ks.ColCase(5, 520, 4, "dyadic", True), ks.ColCase(8200, 8, 0, "spread", True)], ids=ks.col_id)
def test_fused_pass_refusals(dev, lib, c):
    s = ks.build_col(c, dev)
    other_launch(lib, dev)
    assert ks.launch_col(lib, s, stream(), s.ws_bytes - 1) == kc.E_WORKSPACE
    assert str(s.ws_bytes).encode() in lib.dclip_last_error()
    good = [s.xd.data_ptr(), s.y.ptr, s.ra.ptr, s.yc.ptr, s.ce.ptr, s.ca.ptr, s.db.ptr, c.rows, c.cols, c.cols + c.xpad, s.ws.ptr,
            s.ws_bytes, stream()]
    assert lib.dclip_split_f32_f16x3_rows_colstats(*(good[:10] + [None] + good[11:])) == kc.E_WORKSPACE
    for at, value in [(8, c.cols + 4), (9, c.cols - 8), (9, c.cols + 2), (0, good[0] + 4), (3, good[3] + 8), (4, good[4] + 4),
                      (10, good[10] + 4), (5, good[5] + 2), (1, None), (3, None), (4, None), (5, None), (7, 0)]:
        args = list(good)
        args[at] = value
        assert lib.dclip_split_f32_f16x3_rows_colstats(*args) == kc.E_INVAL, (at, value)
    assert lib.dclip_first_launch() == b"", "a refused call leaves no earlier call's instance name standing"
    untouched(lib, s.y, s.ra, s.yc, s.ce, s.ca, s.db, s.ws)


# ------------------------------------------------------------------------------------------------ 4. LayerNorm with split output

@pytest.mark.parametrize("c", ks.ln_cases(), ids=lambda c: f"D{c.D}-rows{c.rows}-s{c.sexp}")
def test_layernorm_split(dev, lib, c):
    s = ks.build_ln(c, dev)
    for entry in ks.LN_ENTRIES:
        ok(lib, ks.launch_ln(lib, s, stream(), entry), ks.ln_site(c, entry))
    torch.cuda.synchronize()
    kc.record("split16_ln", tuple(c), ks.verify_ln(s))


def test_layernorm_split_refusals(dev, lib):
    s = ks.build_ln(ks.LnCase(8, 3, 0), dev)
    ln, st = s.ln, stream()
    other_launch(lib, dev)
    x, g, b = ln.xd.data_ptr(), ln.gd.data_ptr(), ln.bd.data_ptr()
    for D in (6, 2052, 0):
        assert lib.dclip_layernorm_fwd_f16x3(x, g, b, s.y["host"].ptr, 3, D, kr.LN_EPS, 1.0, st) == kc.E_INVAL, D
        assert lib.dclip_layernorm_fwd_f16x3_dev(x, g, b, s.y["dev"].ptr, ln.y.ptr, ln.mean.ptr, ln.rstd.ptr, 3, D, kr.LN_EPS, s.scale.ptr,
                                                 st) == kc.E_INVAL, D
    for scale in (3.0, 0.0, -1.0, float("nan")):
        assert lib.dclip_layernorm_fwd_f16x3(x, g, b, s.y["host"].ptr, 3, 8, kr.LN_EPS, scale, st) == kc.E_INVAL, scale
    assert lib.dclip_layernorm_fwd_f16x3(x + 4, g, b, s.y["host"].ptr, 3, 8, kr.LN_EPS, 1.0, st) == kc.E_INVAL
    assert lib.dclip_layernorm_fwd_f16x3(x, g, b, s.y["host"].ptr + 4, 3, 8, kr.LN_EPS, 1.0, st) == kc.E_INVAL
    assert lib.dclip_layernorm_fwd_f16x3_dev(x, g, b, s.y["dev"].ptr, ln.y.ptr + 4, None, None, 3, 8, kr.LN_EPS, s.scale.ptr, st) == kc.E_INVAL
    assert lib.dclip_layernorm_fwd_f16x3_dev(x, g, b, s.y["dev"].ptr, None, None, None, 3, 8, kr.LN_EPS, None, st) == kc.E_INVAL
    untouched(lib, s.y["host"], s.y["dev"], ln.y, ln.mean, ln.rstd)


# ------------------------------------------------------------------------------------------------ 5. the device plan

def test_plan_constants(lib):
    assert lib.dclip_split16_record_bytes() == ks.RECORD_BYTES == 48
    assert lib.dclip_split16_plan_floats() == ks.PLAN_FLOATS == 32
    assert lib.dclip_split16_tile_rows() == ks.TILE_ROWS == 32


def test_device_plan_refusals(dev, lib):
    s = ks.build_plan(ks.PLAN_CASES[2], dev)
    tab = ks.pack_table(s, s.srcd, dev)
    ptrs = torch.zeros(len(s.recs), dtype=torch.int64, device=dev)
    other_launch(lib, dev)
    t, n, T, st = tab.data_ptr(), len(s.recs), s.tiles, stream()
    for args in [(None, n, T, s.stats.ptr, st), (t, 0, T, s.stats.ptr, st), (t, n, 0, s.stats.ptr, st), (t, n, T, None, st)]:
        assert lib.dclip_split16_stats(*args) == kc.E_INVAL, args
    for args in [(None, s.plan.ptr, 1, 72, st), (s.stats.ptr, None, 1, 72, st), (s.stats.ptr, s.plan.ptr, 0, 72, st),
                 (s.stats.ptr, s.plan.ptr, 1, 0, st)]:
        assert lib.dclip_split16_plan(*args) == kc.E_INVAL, args
    for args in [(None, n, T, s.plan.ptr, st), (t, 0, T, s.plan.ptr, st), (t, n, 0, s.plan.ptr, st), (t, n, T, None, st)]:
        assert lib.dclip_split16_weights(*args) == kc.E_INVAL, args
        assert lib.dclip_split16_weights_t(*args[:4], ptrs.data_ptr(), st) == kc.E_INVAL, args
    assert lib.dclip_split16_weights_t(t, n, T, s.plan.ptr, None, st) == kc.E_INVAL
    untouched(lib, s.plan, *[d for d in s.dst + s.dst_t if d is not None])
    s.stats.assert_guards("refused")
    assert not bool(s.stats.get().any())


@pytest.mark.parametrize("c", ks.PLAN_CASES, ids=ks.plan_id)
def test_device_plan(dev, lib, c):
    s = ks.build_plan(c, dev)
    names = []
    rc = ks.launch_plan(lib, s, stream(), dev, names)
    assert rc == 0, lib.dclip_last_error()
    assert all(want == got for want, got in names) and len(names) == 5, names
    torch.cuda.synchronize()
    kc.record("split16_plan", (c.name, c.transposed), ks.verify_plan(s))


# ------------------------------------------------------------------------------------------------ 7. the segmented weight gradient

@pytest.mark.parametrize("c", ks.seg_cases(), ids=ks.seg_id)
def test_segmented_wgrad(dev, lib, c):
    s = ks.build_seg(c, dev)
    assert lib.dclip_gemm_f16_splitk_workspace(c.M, c.N, 3 * s.s_eff) == s.ws_bytes
    ok(lib, ks.launch_seg(lib, s, stream()), ks.SEG_SITE)
    torch.cuda.synchronize()
    kc.record("split16_seg3", tuple(c), ks.verify_seg(s))


def test_segmented_wgrad_refusals(dev, lib):
    c = ks.SegCase(264, 8, 192, 2, False)
    s = ks.build_seg(c, dev)
    other_launch(lib, dev)
    assert ks.launch_seg(lib, s, stream(), s.ws_bytes - 1) == kc.E_WORKSPACE
    assert str(s.ws_bytes).encode() in lib.dclip_last_error()
    good = [s.dyd.data_ptr(), s.xd.data_ptr(), s.C.ptr, c.M, c.N, c.tokens, s.lddy, s.ldx, s.C.ld, *s.a_seg, *s.w_seg, s.cad.ptr, s.act.ptr,
            c.splits, s.ws.ptr, s.ws_bytes, stream()]
    for at, value in [(3, 260), (4, 12), (5, 100), (17, 0), (17, 22), (6, s.lddy + 4), (7, s.ldx + 4), (8, c.N + 2), (8, c.N - 4),
                      (9, 4), (10, s.lddy - c.M + 8), (13, -8), (14, s.ldx - c.N + 8), (0, good[0] + 8), (2, good[2] + 4),
                      (15, good[15] + 2), (16, None), (15, None), (0, None)]:
        args = list(good)
        args[at] = value
        assert lib.dclip_gemm_f16_wgrad_tokmajor_seg3(*args) == kc.E_INVAL, (at, value)
    untouched(lib, s.C, s.ws)


# ------------------------------------------------------------------------------------------------ 6. the scaled GEMM entries

def set_switches(monkeypatch, env):
    for k in ks.GEMM_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("c", ks.scaled_cases(), ids=ks.scaled_id)
def test_scaled_gemm_entries(dev, lib, monkeypatch, c):
    """The five entries in every form on .r64, .r128, .pp (DCLIP_BF16_BIG_MIN=1, read per call) and, for gemm_f16_scaled alone,
    .ppp; under the persistent switches the other four must still report .pp."""
    set_switches(monkeypatch, ks.scaled_env(c))
    s = ks.build_scaled(c, dev)
    ok(lib, ks.launch_scaled(lib, s, stream()), ks.scaled_site(c))
    torch.cuda.synchronize()
    kc.record("split16_scaled", tuple(c), ks.verify_scaled(s))


def test_scaled_gemm_refusals(dev, lib, monkeypatch):
    set_switches(monkeypatch, {})
    S = lambda entry: ks.build_scaled(ks.ScaledCase(entry, "r64", 65, 68, 72, 1), dev)
    extra = kc.Guarded(65, 68, device=dev)
    other_launch(lib, dev)
    st = stream()
    bufs = [extra]
    s = S("split")                                         # a split with RESIDUAL
    assert ks.launch_scaled(lib, s, st, epi=ks.EPI_BIAS | ks.EPI_RESIDUAL) == kc.E_INVAL
    for alpha in (float("inf"), float("-inf"), float("nan")):                   # non-finite alpha
        assert ks.launch_scaled(lib, s, st, alpha=alpha) == kc.E_INVAL, alpha
    bufs.append(s.C)
    s = S("scaled")
    for alpha in (float("inf"), float("nan")):
        assert ks.launch_scaled(lib, s, st, alpha=alpha) == kc.E_INVAL, alpha
    bufs.append(s.C)
    s = S("split_dev")
    assert ks.launch_scaled(lib, s, st, epi=ks.EPI_BIAS | ks.EPI_RESIDUAL) == kc.E_INVAL
    assert ks.launch_scaled(lib, s, st, h32=extra.ptr) == kc.E_INVAL            # h32 without GELU
    assert ks.launch_scaled(lib, s, st, g32=extra.ptr, out_scale=None) == kc.E_INVAL          # g32 without out_scale
    bufs.append(s.C)
    s = S("rows_dev")
    assert ks.launch_scaled(lib, s, st, epi=ks.EPI_BIAS) == kc.E_INVAL          # rows with BIAS
    assert ks.launch_scaled(lib, s, st, epi=ks.EPI_DGELU) == kc.E_INVAL         # DGELU without aux32
    bufs.append(s.C)
    assert lib.dclip_last_error()
    untouched(lib, *bufs)
