"""CPU-only: what the erf-GELU checkers of tests/kernel_checks_gelu.py accept and what they catch.  torch's own CPU fp32 GELU —
the function HF runs for hidden_act="gelu" — stays inside the fp32 gates on the inputs the gates were measured on and on the edge
inputs, so the reference alone does not use up the bound; every planted fault is refused."""
import pytest
import torch
import torch.nn.functional as F

from tests import kernel_checks_gelu as kg


@pytest.fixture(scope="module")
def h32():
    return kg.inputs32()


def torch_dgelu(h):
    x = h.clone().requires_grad_(True)
    F.gelu(x).sum().backward()
    return x.grad


def test_torch_fp32_passes_both_gates(h32):
    assert h32.numel() == 8400003 and bool(torch.isfinite(h32).all())
    fwd = kg.check_fwd32(F.gelu(h32), h32, "torch CPU forward")
    bwd = kg.check_bwd32(torch_dgelu(h32), h32, torch.ones_like(h32), "torch CPU backward")
    # the measurement the 8 rests on (6.07 forward at h = 2.98 and 4.87 backward on the author's draw of the random part)
    assert 4.0 < fwd <= kg.GATE and 3.0 < bwd <= kg.GATE, (fwd, bwd)


def test_torch_fp32_passes_on_the_edge_inputs():
    e = kg.edge_inputs32()
    assert int((e == 0).sum()) == 2 and int(((e != 0) & (e.abs() < 2.0 ** -126)).sum()) == 10
    kg.check_fwd32(F.gelu(e), e, "torch CPU forward, edges")
    gen = torch.Generator().manual_seed(5)
    dg = torch.randn(e.numel(), generator=gen) * 3.0
    kg.check_bwd32(torch_dgelu(e) * dg, e, dg, "torch CPU backward, edges")


def test_the_floor_is_the_formats_and_nothing_more():
    """2^-150 lets through the one thing no fp32 result can avoid — 0.5 h of an odd subnormal — and is invisible at normal size."""
    h = torch.tensor([2.0 ** -149, 3 * 2.0 ** -149], dtype=torch.float64).float()
    s = 2.0 ** -149
    for got in (torch.tensor([0.0, s], dtype=torch.float64).float(), torch.tensor([s, 2 * s], dtype=torch.float64).float()):
        # either fp32 neighbour of the exact 0.5 s and 1.5 s: |error| = 2^-150
        assert float(kg.fwd32_units(got, h).max()) == 0.0
    one = torch.tensor([1.0, -1.0, 2.0 ** -126])
    exact = kg.gelu64(one)
    off = (exact + 12.0 * kg.ULP * one.double().abs()).float()   # 12 units out: the floor does not cover it
    assert float(kg.fwd32_units(off, one).min()) > kg.GATE


FAULT_H = torch.cat([torch.linspace(-14.0, 14.0, 40001), kg.edge_inputs32()])


@pytest.mark.parametrize("name,fn", [
    ("quick_gelu", kg.quick_gelu32),
    ("tanh", lambda h: F.gelu(h, approximate="tanh")),
])
def test_forward_checker_catches_another_activation(name, fn):
    with pytest.raises(AssertionError):
        kg.check_fwd32(fn(FAULT_H), FAULT_H, name)


def test_forward_checker_catches_a_dropped_tail_element():
    h = torch.linspace(-3.0, 3.0, 1029)                          # 1024 + 5: the scalar tail of a vector kernel
    g = F.gelu(h)
    kg.check_fwd32(g, h, "intact")
    for stale in (h, torch.zeros_like(h), torch.full_like(h, float("nan"))):       # input left in place / never written / poison
        bad = g.clone()
        bad[-1] = stale[-1]
        with pytest.raises(AssertionError):
            kg.check_fwd32(bad, h, "tail dropped")


def test_backward_checker_catches_a_derivative_without_the_density_term():
    dg = torch.ones_like(FAULT_H)
    kg.check_bwd32(torch_dgelu(FAULT_H), FAULT_H, dg, "intact")
    with pytest.raises(AssertionError):
        kg.check_bwd32(kg.phi_cdf64(FAULT_H).float(), FAULT_H, dg, "Phi alone")
    with pytest.raises(AssertionError):                          # quick-GELU's derivative
        s = torch.sigmoid(1.702 * FAULT_H)
        kg.check_bwd32(s * (1 + 1.702 * FAULT_H * (1 - s)), FAULT_H, dg, "quick_gelu'")
    with pytest.raises(AssertionError):                          # dg forgotten
        kg.check_bwd32(torch_dgelu(FAULT_H), FAULT_H, dg * 2.0, "dg dropped")


# torch's form, 0.5 h (1 + erf(h / sqrt 2)) in fp32, is held to the 16-bit checker where that form has the accuracy to round
# from: 1 + erf cancels in the negative tail (at h = -3.25 it keeps 12 bits, one more than fp16 stores; 325 bf16 and 311 fp16
# inputs below that are not faithful, down to h = -13.5), and h (1 + erf) overflows above 1.7e38.  The kernels take erfc on the
# negative side and h Phi(h) and are held to EVERY finite input (tests/test_gelu_erf_paths_gpu.py).
TORCH16_LO, TORCH16_HI = -3.0, 1.0e38


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_torch_fp32_then_round_is_faithful(dtype):
    x = kg.all_finite16(dtype)
    assert x.numel() == {torch.bfloat16: 65280, torch.float16: 63488}[dtype]
    x = x[(x.float() >= TORCH16_LO) & (x.float() <= TORCH16_HI)]
    assert x.numel() > 40000 and bool((x.float().abs() < 1e-38).any() if dtype == torch.bfloat16 else (x.float().abs() < 6e-5).any())
    kg.check_faithful16(kg.torch_gelu16(x), x, f"torch CPU {dtype}")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_faithful_checker_catches_faults(dtype):
    x = kg.all_finite16(dtype)
    x = x[(x.float() >= TORCH16_LO) & (x.float() <= 8.0)]
    good = kg.torch_gelu16(x)
    with pytest.raises(AssertionError):
        kg.check_faithful16(kg.quick_gelu32(x.float()).to(dtype), x, "quick_gelu")
    with pytest.raises(AssertionError):
        kg.check_faithful16(F.gelu(x.float(), approximate="tanh").to(dtype), x, "tanh")
    i = int((x.float() - 1.0).abs().argmin())
    for step_up in (True, False):                                # two steps off the exact value's bracket, on either side
        bad = good.clone()
        bad[i] = kg._step16(kg._step16(good[i:i + 1], step_up), step_up)[0]
        with pytest.raises(AssertionError):
            kg.check_faithful16(bad, x, "two steps off")
    x, good = torch.cat([x, x[i:i + 1]]), torch.cat([good, good[i:i + 1]])     # ... with h = 1 as the last element
    kg.check_faithful16(good, x, "intact")
    bad = good.clone()
    bad[-1] = x[-1]                                              # the last element left as the input
    with pytest.raises(AssertionError):
        kg.check_faithful16(bad, x, "tail dropped")


def test_step16_walks_the_number_line():
    for dtype in (torch.bfloat16, torch.float16):
        x = kg.all_finite16(dtype)
        v = x.double()
        order = v.argsort(stable=True)
        xs, vs = x[order], v[order]
        inner = (vs[1:] > vs[:-1])                               # skip the -0 / +0 pair
        up = kg._step16(xs[:-1], True).double()
        assert bool((up[inner] == vs[1:][inner]).all())
        down = kg._step16(xs[1:], False).double()
        assert bool((down[inner] == vs[:-1][inner]).all())


def test_the_entries_refuse_bad_arguments_on_the_host():
    """n = 0, a null pointer and a pointer off by 4 bytes are refused before anything is launched: no GPU is needed to see it."""
    from dclip_amd import _lib
    lib = _lib.load()
    ptr = 4096                                   # never dereferenced: every call below is refused
    for name, nptr in (("gelu_erf_f32", 2), ("gelu_erf_bf16", 2), ("gelu_erf_f16", 2), ("gelu_erf_bwd_f32", 3)):
        fn = getattr(lib, "dclip_" + name)
        assert fn(*[ptr] * nptr, 0, None) == -1 and name.encode() in lib.dclip_last_error()
        for k in range(nptr):
            assert fn(*[None if j == k else ptr for j in range(nptr)], 64, None) == -1, (name, k)
            assert b"bad arguments" in lib.dclip_last_error()
            assert fn(*[ptr + 4 if j == k else ptr for j in range(nptr)], 64, None) == -1, (name, k)
            assert b"16-byte aligned" in lib.dclip_last_error()
