"""fp64 references, input sets and checkers of the stand-alone erf-GELU kernels (dclip_amd/csrc/activation.hip).
No GPU here: tests/test_kernel_checks_gelu_cpu.py shows that torch's own CPU fp32 GELU — the function HF runs — passes every
checker and that each planted fault is caught; tests/test_gelu_erf_paths_gpu.py runs the kernels through them.

Gates (finite inputs only):
  fp32 forward    |got - want64| <= 8 2^-24 |h| + 2^-150,  want64 = 0.5 h erfc(-h / sqrt 2) in fp64.  Relative to |h|, not to
                  |want|: |gelu(h)| <= |h|, and the negative tail cancels in any fp32 form that goes through 1 + erf.
  fp32 backward   |got - dg gelu'64(h)| <= 8 2^-24 |dg| + 2^-150,  gelu'(h) = Phi(h) + h phi(h).
  The 8: torch's CPU fp32 F.gelu against the same references, over the 8.4 million inputs of `inputs32`, reaches 6.07 (forward,
  at h = 2.98) and 4.87 (backward, dg = 1) in these units; 8 lets a kernel be as inexact as that reference and not materially worse.
  The 2^-150: half the smallest fp32 subnormal, the format's own floor.  For a normal h it is below a thousandth of the first term
  (8 2^-24 2^-126 = 2^-147); for a subnormal h = k 2^-149 with k odd the exact result 0.5 h is no fp32 number and NO fp32 result
  is nearer than 2^-150, while the first term alone would ask for 2^-170 k.
  16-bit          faithful: the result is one of the two values of the type that bracket the fp64 GELU of the 16-bit input — that
                  value itself when it is one.
"""
import math

import torch

ULP = 2.0 ** -24
GATE = 8.0
FLOOR = 2.0 ** -150
WORST_H = 2.98                                   # where torch's CPU forward is furthest off (6.07 units)
SQRT1_2 = math.sqrt(0.5)
INV_SQRT_2PI = 1.0 / math.sqrt(2.0 * math.pi)


def phi_cdf64(h: torch.Tensor) -> torch.Tensor:
    return 0.5 * torch.special.erfc(-h.double() * SQRT1_2)


def gelu64(h: torch.Tensor) -> torch.Tensor:
    """0.5 h erfc(-h / sqrt 2) in fp64: no cancellation on either side."""
    h = h.double()
    return h * phi_cdf64(h)


def dgelu64(h: torch.Tensor) -> torch.Tensor:
    h = h.double()
    return phi_cdf64(h) + h * torch.exp(-0.5 * h * h) * INV_SQRT_2PI


def quick_gelu32(h: torch.Tensor) -> torch.Tensor:
    return h * torch.sigmoid(1.702 * h)


def inputs32() -> torch.Tensor:
    """The fp32 inputs the 8 was measured on: a 4,000,001-point grid over [-14, 14], 4,000,000 samples of 3 N(0,1) and
    +-10^e for 200,001 e from -30 to 1.2 each — 8,400,003 values."""
    gen = torch.Generator().manual_seed(34)
    lg = torch.logspace(-30.0, 1.2, 200001, dtype=torch.float64)
    return torch.cat([torch.linspace(-14.0, 14.0, 4000001, dtype=torch.float64).float(),
                      torch.randn(4000000, generator=gen) * 3.0, lg.float(), -lg.float()])


def edge_inputs32() -> torch.Tensor:
    """+-0, subnormals (the smallest, an odd and an even multiple, the largest), +-14, values either side of 0 within 1e-4 and the
    worst point of torch's own forward."""
    tiny = [2.0 ** -149, 3 * 2.0 ** -149, 2.0 ** -140, 2.0 ** -127, 2.0 ** -126 - 2.0 ** -149]
    near = [1e-4, 3e-5, 1e-7, 1e-20]
    vals = [0.0, -0.0, 14.0, -14.0, WORST_H, -WORST_H] + tiny + [-v for v in tiny] + near + [-v for v in near]
    return torch.tensor(vals, dtype=torch.float64).float()


def fwd32_units(got: torch.Tensor, h: torch.Tensor) -> torch.Tensor:
    """|got - want64| - FLOOR (clamped at 0) in units of 2^-24 |h|, per element (0 where h = 0 and the result is exact)."""
    err = ((got.double().cpu() - gelu64(h.cpu())).abs() - FLOOR).clamp_min(0.0)
    return err / (ULP * h.double().cpu().abs()).clamp_min(1e-300)


def bwd32_units(got: torch.Tensor, h: torch.Tensor, dg: torch.Tensor) -> torch.Tensor:
    dg64 = dg.double().cpu()
    err = ((got.double().cpu() - dg64 * dgelu64(h.cpu())).abs() - FLOOR).clamp_min(0.0)
    return err / (ULP * dg64.abs()).clamp_min(1e-300)


def _check_finite(got: torch.Tensor, what: str) -> None:
    assert bool(torch.isfinite(got).all()), f"{what}: a non-finite result for a finite input"


def check_fwd32(got: torch.Tensor, h: torch.Tensor, what: str) -> float:
    """Asserts the fp32 forward gate; returns the worst figure (units of 2^-24 |h|)."""
    assert got.dtype == torch.float32 and got.shape == h.shape, (what, got.dtype, got.shape, h.shape)
    _check_finite(got, what)
    u = fwd32_units(got, h)
    i = int(u.argmax())
    worst = float(u.reshape(-1)[i])
    print(f"[gelu] {what}: worst forward error {worst:.3f} x 2^-24 |h| at h = {float(h.reshape(-1)[i]):.9g}")
    assert worst <= GATE, (what, worst, float(h.reshape(-1)[i]), float(got.reshape(-1)[i]))
    return worst


def check_bwd32(got: torch.Tensor, h: torch.Tensor, dg: torch.Tensor, what: str) -> float:
    assert got.dtype == torch.float32 and got.shape == h.shape == dg.shape, (what, got.dtype, got.shape)
    _check_finite(got, what)
    u = bwd32_units(got, h, dg)
    i = int(u.argmax())
    worst = float(u.reshape(-1)[i])
    print(f"[gelu] {what}: worst backward error {worst:.3f} x 2^-24 |dg| at h = {float(h.reshape(-1)[i]):.9g}")
    assert worst <= GATE, (what, worst, float(h.reshape(-1)[i]), float(dg.reshape(-1)[i]), float(got.reshape(-1)[i]))
    return worst


# ---------------------------------------------------------------------------------------------------- 16-bit

def all_finite16(dtype) -> torch.Tensor:
    """Every finite value of a 16-bit type, both zeros and the subnormals included (65,280 bf16 / 63,488 fp16 patterns)."""
    x = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(dtype)
    return x[torch.isfinite(x.float())].clone()


def _step16(x: torch.Tensor, up: bool) -> torch.Tensor:
    """The next value of x's 16-bit type above (`up`) or below x; x finite."""
    bits = x.view(torch.int16).to(torch.int32) & 0xFFFF
    neg, mag = bits >= 0x8000, bits & 0x7FFF
    away = neg != up                                   # a positive value going up, a negative one going down: |x| grows
    mag2 = torch.where(away, mag + 1, mag - 1)
    sign = torch.where(neg, 0x8000, 0)
    out = sign | mag2
    zero = mag == 0                                    # +-0: one step is the smallest subnormal of the direction's sign
    out = torch.where(zero, torch.full_like(out, 0x0001 if up else 0x8001), out)
    out = torch.where(out >= 0x8000, out - 0x10000, out)
    return out.to(torch.int16).view(x.dtype)


def faithful16_bad(got: torch.Tensor, h: torch.Tensor) -> torch.Tensor:
    """Mask of the elements of `got` that are NOT a faithful rounding of gelu64(h) to got's type."""
    assert got.dtype == h.dtype and got.dtype in (torch.bfloat16, torch.float16) and got.shape == h.shape
    got, h = got.cpu(), h.cpu()
    want = gelu64(h)
    r = want.to(got.dtype)                             # some value of the type within one step of want
    r64 = r.double()
    lo = torch.where(r64 <= want, r, _step16(r, False))
    hi = torch.where(r64 >= want, r, _step16(r, True))
    # r may be TWO steps off only through a double rounding on the way down; widen nothing, tighten instead
    lo = torch.where(_step16(lo, True).double() <= want, _step16(lo, True), lo)
    hi = torch.where(_step16(hi, False).double() >= want, _step16(hi, False), hi)
    g64 = got.double()
    ok = (g64 == lo.double()) | (g64 == hi.double())
    return ~ok | ~torch.isfinite(g64)


def check_faithful16(got: torch.Tensor, h: torch.Tensor, what: str) -> int:
    bad = faithful16_bad(got, h)
    n = int(bad.sum())
    if n:
        i = int(bad.reshape(-1).nonzero()[0])
        raise AssertionError(f"{what}: {n} of {bad.numel()} results are not faithful, first at h = {float(h.reshape(-1)[i])!r}: got "
                             f"{float(got.reshape(-1)[i])!r}, fp64 {float(gelu64(h.reshape(-1)[i:i + 1]))!r}")
    print(f"[gelu] {what}: {bad.numel()} results faithful")
    return n


def torch_gelu16(h: torch.Tensor) -> torch.Tensor:
    """What torch's CPU gives for a 16-bit tensor: fp32 math, then a round."""
    return torch.nn.functional.gelu(h.float()).to(h.dtype)
