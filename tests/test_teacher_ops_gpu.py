"""The meta-teacher tail (dclip_amd/csrc/aggregation.hip) and the small helpers through the C ABI, on guarded buffers:
aggregation forward / backward against the fp64 oracle, and exact equality for pack_tokens, mask_rows, sanitize_groups,
fill, axpby; sub_reduce against an fp64 sum."""
import pytest
import torch

from oracle import dclip_oracle as O
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


def rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def ok(lib, rc):
    assert rc == 0, lib.dclip_last_error().decode(errors="replace")
    torch.cuda.synchronize()


def aggregation64(x, temperature):
    """oracle.aggregation with vector_norm in place of sqrt(sum): the same value, and a zero row back-propagates the clamp's
    zero subgradient instead of 0 * inf."""
    m = x.mean(dim=1, keepdim=True)
    nx = torch.linalg.vector_norm(x, dim=-1).clamp_min(1e-8)
    nm = torch.linalg.vector_norm(m, dim=-1).clamp_min(1e-8)
    w = torch.softmax((x * m).sum(-1) / (nx * nm) / temperature, dim=-1)
    return (x * w.unsqueeze(-1)).sum(dim=1), w


@pytest.mark.parametrize("E", [64, 512, 768])
@pytest.mark.parametrize("L", [1, 2, 75, 96])
@pytest.mark.parametrize("temperature,out_scale,accumulate,zero_row", [(2.0, 1.0, 0, False), (0.5, 0.5, 1, False),
                                                                        (2.0, 1.0, 0, True)])
def test_aggregation_fwd_bwd(dev, lib, L, E, temperature, out_scale, accumulate, zero_row):
    B = 3
    x = rnd((B, L, E), L + E, 1.5) + 0.3
    if zero_row:
        x[1, L // 2] = 0.0                         # the 1e-8 clamp of the row norm (and of the mean's, when L == 1)
    out0, dout = rnd((B, E), 2), rnd((B, E), 3)
    xd = x.double().requires_grad_(True)
    agg, w = aggregation64(xd, temperature)
    assert torch.equal(agg.detach(), O.aggregation(x.double(), temperature)) or kc.relerr(agg, O.aggregation(x.double(), temperature)) < 1e-14
    want = out_scale * agg + (out0.double() if accumulate else 0.0)
    (out_scale * agg * dout.double()).sum().backward()
    if not zero_row:                                # the oracle's own autograd, where it is defined
        xo = x.double().requires_grad_(True)
        (out_scale * O.aggregation(xo, temperature) * dout.double()).sum().backward()
        assert kc.relerr(xd.grad, xo.grad) < 1e-12
    xg, dg = x.to(dev), dout.to(dev)
    out = kc.Guarded(B, E, device=dev, fill=out0 if accumulate else kc.NAN)
    wts = kc.Guarded(B, L, device=dev)
    ok(lib, lib.dclip_aggregation_fwd(xg.data_ptr(), out.ptr, wts.ptr, B, L, E, temperature, out_scale, accumulate, stream()))
    assert lib.dclip_last_launch() == b"aggregation_fwd"
    dx = kc.Guarded(B * L, E, device=dev)
    ok(lib, lib.dclip_aggregation_bwd(xg.data_ptr(), wts.ptr, dg.data_ptr(), dx.ptr, B, L, E, temperature, out_scale, stream()))
    for g in (out, wts, dx):
        g.assert_guards("aggregation")
    fig = kc.check_blocks({"out": (out.get(), want, 1e-5), "weights": (wts.get(), w, 1e-5),
                           "dx": (dx.get(), xd.grad.reshape(B * L, E), 2e-5)}, f"aggregation L={L} E={E}")
    print(fig)


def test_aggregation_refuses_more_than_96_rows(dev, lib):
    B, L, E = 2, 97, 64
    x = rnd((B, L, E), 1).to(dev)
    out, wts, dx = kc.Guarded(B, E, device=dev), kc.Guarded(B, L, device=dev), kc.Guarded(B * L, E, device=dev)
    assert lib.dclip_aggregation_fwd(x.data_ptr(), out.ptr, wts.ptr, B, L, E, 2.0, 1.0, 0, stream()) == kc.E_INVAL
    assert lib.dclip_aggregation_bwd(x.data_ptr(), wts.ptr, out.ptr, dx.ptr, B, L, E, 2.0, 1.0, stream()) == kc.E_INVAL
    torch.cuda.synchronize()
    for g in (out, wts, dx):
        g.assert_guards("aggregation L=97")
        assert bool(torch.isnan(g.get()).all())


@pytest.mark.parametrize("T,Tmax,P", [(77, 75, 512), (16, 16, 64), (9, 4, 132)])
def test_pack_tokens(dev, lib, T, Tmax, P):
    eos = [1, T - 1, 5, 0, 2, Tmax + 1 if Tmax + 1 < T else T - 1]          # 1 and 0: no word tokens -> the sentence row
    B = len(eos)
    tokens, sentence = rnd((B, T, P), 1), rnd((B, P), 2)
    want = torch.zeros(B, Tmax, P)
    for b, e in enumerate(eos):
        n = max(e - 1, 0)
        if n == 0:
            want[b, 0] = sentence[b]
        else:
            k = min(n, Tmax)
            want[b, :k] = tokens[b, 1:1 + k]
    out = kc.Guarded(B * Tmax, P, device=dev)
    td, sd, ed = tokens.to(dev), sentence.to(dev), torch.tensor(eos, dtype=torch.int32, device=dev)
    ok(lib, lib.dclip_pack_tokens(td.data_ptr(), sd.data_ptr(), ed.data_ptr(), out.ptr, B, T, Tmax, P, stream()))
    out.assert_guards("pack_tokens")
    assert torch.equal(out.get().view(B, Tmax, P), want)


@pytest.mark.parametrize("R,E", [(7, 64), (50, 512), (1, 4)])
def test_mask_rows(dev, lib, R, E):
    count = [0, R, R // 2, 1, R + 3]                                        # none kept, all kept, ..., a count beyond R
    B = len(count)
    x = rnd((B, R, E), 3)
    want = x.clone()
    for b, c in enumerate(count):
        want[b, c:] = 0.0
    g = kc.Guarded(B * R, E, device=dev, fill=x)
    cd = torch.tensor(count, dtype=torch.int32, device=dev)
    ok(lib, lib.dclip_mask_rows(g.ptr, cd.data_ptr(), B, R, E, stream()))
    g.assert_guards("mask_rows")
    assert torch.equal(g.get().view(B, R, E), want)


@pytest.mark.parametrize("rows,E", [(1, 512), (5, 64), (75, 512), (3, 2052)])
def test_sanitize_groups(dev, lib, rows, E):
    groups = 9
    x = rnd((groups, rows, E), 4)
    x[1, rows - 1, E - 1] = float("nan")
    x[3, 0, 0] = float("inf")
    x[4, rows // 2, E // 2] = float("-inf")
    x[7, 0, 1] = 3.0e38                                                      # large but finite: kept
    bad = [0, 1, 0, 1, 1, 0, 0, 0, 0]
    want = x.clone()
    for gi, f in enumerate(bad):
        if f:
            want[gi] = 0.0
    SENT = 0x5A5A5A5A
    flags = torch.full((groups + 256,), SENT, dtype=torch.int32, device=dev)
    g = kc.Guarded(groups * rows, E, device=dev, fill=x)
    ok(lib, lib.dclip_sanitize_groups(g.ptr, flags[128:].data_ptr(), groups, rows, E, 0, stream()))
    g.assert_guards("sanitize_groups")
    assert torch.equal(g.get().view(groups, rows, E), want)
    assert flags[128:128 + groups].cpu().tolist() == bad
    assert bool((flags[:128] == SENT).all()) and bool((flags[128 + groups:] == SENT).all())
    # mode 1 (the guard's backward): zero the flagged groups, detect nothing — a NaN in an unflagged group stays
    dy = rnd((groups, rows, E), 5)
    dy[0, 0, 0] = float("nan")
    want = dy.clone()
    for gi, f in enumerate(bad):
        if f:
            want[gi] = 0.0
    g = kc.Guarded(groups * rows, E, device=dev, fill=dy)
    ok(lib, lib.dclip_sanitize_groups(g.ptr, flags[128:].data_ptr(), groups, rows, E, 1, stream()))
    g.assert_guards("sanitize_groups mode 1")
    assert torch.equal(g.get().view(torch.int32), want.reshape(groups * rows, E).view(torch.int32))
    assert flags[128:128 + groups].cpu().tolist() == bad


@pytest.mark.parametrize("rows,cols", [(1, 1), (1, 3), (1, 4099), (147, 4099)])         # the last: more floats than one grid pass
def test_fill_and_axpby(dev, lib, rows, cols):
    n = rows * cols
    y = kc.Guarded(rows, cols, device=dev)
    ok(lib, lib.dclip_fill(y.ptr, 3.25, n, stream()))
    y.assert_guards("fill")
    assert torch.equal(y.get(), torch.full((rows, cols), 3.25))
    g = torch.Generator().manual_seed(n)
    x = torch.randint(-8, 9, (rows, cols), generator=g).float()
    y0 = torch.randint(-8, 9, (rows, cols), generator=g).float()
    xd = x.to(dev)
    y = kc.Guarded(rows, cols, device=dev, fill=y0)
    ok(lib, lib.dclip_axpby(xd.data_ptr(), y.ptr, 0.5, -2.0, n, stream()))         # integers and powers of two: exact
    y.assert_guards("axpby")
    assert torch.equal(y.get(), 0.5 * x - 2.0 * y0)
    y = kc.Guarded(rows, cols, device=dev)                                         # b == 0: y is not read (NaN here)
    ok(lib, lib.dclip_axpby(xd.data_ptr(), y.ptr, 4.0, 0.0, n, stream()))
    y.assert_guards("axpby b=0")
    assert torch.equal(y.get(), 4.0 * x)
    if rows == 1:                                  # a destination that is only 4-byte aligned takes the scalar form
        y = kc.Guarded(1, n + 1, device=dev, fill=torch.cat([torch.zeros(1, 1), y0], 1))
        ok(lib, lib.dclip_axpby(xd.data_ptr(), y.ptr + 4, 2.0, 1.0, n, stream()))
        y.assert_guards("axpby unaligned")
        assert torch.equal(y.get(), torch.cat([torch.zeros(1, 1), 2.0 * x + y0], 1))


@pytest.mark.parametrize("n", [1, 5, 4096, 100003])
@pytest.mark.parametrize("with_b,accumulate", [(True, 0), (False, 0), (True, 1), (False, 1)])
def test_sub_reduce(dev, lib, n, with_b, accumulate):
    """out (+)= scale * sum(a - b): within the rounding bound of an n-term fp32 sum in any order, (n + 8) 2^-24 sum |a_i - b_i|
    (+ |out0| for the accumulate), scaled."""
    a, b = rnd((n,), 1), rnd((n,), 2)
    scale, out0 = 0.37, 1.75
    d = a.double() - (b.double() if with_b else 0.0)
    want = scale * d.sum() + (out0 if accumulate else 0.0)
    bound = (n + 8) * 2.0 ** -24 * (scale * float(d.abs().sum()) + (out0 if accumulate else 0.0))
    out = kc.Guarded(1, 1, device=dev, fill=out0 if accumulate else kc.NAN)
    ad, bd = a.to(dev), b.to(dev)
    ok(lib, lib.dclip_sub_reduce(ad.data_ptr(), bd.data_ptr() if with_b else None, out.ptr, n, scale, accumulate, stream()))
    out.assert_guards("sub_reduce")
    got = float(out.get())
    print(n, with_b, accumulate, abs(got - float(want)) / bound)
    assert abs(got - float(want)) <= bound, (got, float(want), bound)
