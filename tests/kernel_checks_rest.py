"""TEST-ONLY checkers and case lists for the row-wise, embedding, loss and optimizer kernels:
dclip_amd/csrc/layernorm.hip, train_bf16.hip, embed.hip, loss.hip and optim.hip through the C ABI
(tests/test_rowwise_paths_gpu.py, tests/test_embed_loss_paths_gpu.py, tests/test_optim_paths_gpu.py).

Like tests/kernel_checks.py, which it builds on, nothing here imports the product or needs a GPU.  Every family has
  build_*(case, device)   inputs (NaN-poisoned padding) and outputs (Guarded, NaN payload or the initial value);
  launch_*(lib, s, st)    the C ABI call(s) on the buffers of s;
  emulate_*(s, fault)     a plain fp32 torch evaluation with the kernel's summation shape that writes the same buffers
                          (tests/test_kernel_checks_rest_cpu.py; `fault` plants one defect);
  verify_*(s)             guards, then every element either EXACT or under a per-element bound derived from where the
                          kernel rounds.  No comparison uses one norm per tensor, except the project's 1e-5 figure for the
                          LayerNorm statistics that §17 keeps as well (next to their derived per-element bound).
u = 2^-24 is the unit roundoff of fp32 and gamma(k) = k u / (1 - k u) the usual bound of k successive roundings."""
from __future__ import annotations

import math
import struct
from collections import namedtuple
from types import SimpleNamespace

import torch

from tests.kernel_checks import (F16_SUB, F32_TINY, LN16_D, LN16_ROWS, NAN, TOL_LN, TYPES16, Guarded, cast_input, check_blocks,
                                 expected_ln16_variant, poisoned, round16, roundup)      # cast_input carries CAST_SPECIALS

U = 2.0 ** -24
ULP = 2.0 ** -23                 # one unit in the last place relative to the value: what a "1 ulp" library function may miss by
WS_TAIL = 64                     # NaN floats behind a workspace's documented size that must stay NaN
PADS = [0, 4, 36]
TY2 = ["bf16", "f16ex"]          # the training types of train_bf16.hip / layernorm.hip (IEEE fp16)


def gamma(k: float) -> float:
    return k * U / (1.0 - k * U)


def gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(int(seed))


def ints(shape, seed, lo=-2, hi=2) -> torch.Tensor:
    return torch.randint(lo, hi + 1, tuple(shape), generator=gen(seed)).float()


def randn(shape, seed, scale=1.0) -> torch.Tensor:
    return torch.randn(tuple(shape), generator=gen(seed)) * scale


def random_bits(shape, seed) -> torch.Tensor:
    """fp32 tensor of random bit patterns (NaNs with payloads, infinities and subnormals included): pure data movement."""
    return torch.randint(-2 ** 31, 2 ** 31, tuple(shape), generator=gen(seed), dtype=torch.int64).to(torch.int32).view(torch.float32)


def ibits(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


class Report:
    """Collects per-element findings of one case; done() raises one AssertionError naming all of them."""

    def __init__(self, what: str):
        self.what, self.failed, self.fig = what, [], {}

    def fail(self, msg: str):
        self.failed.append(msg)

    def guards(self, **bufs):
        for name, g in bufs.items():
            if g is None:
                continue
            bad = g.guard_violations()
            if bad:
                self.fail(f"{name}: memory outside [{g.rows}][{g.cols}] (ld {g.ld}) was written at (row, col) {bad}")

    def _where(self, bad, got, want):
        idx = bad.nonzero()[0].tolist()
        return f"{int(bad.sum())} elements differ, first at {tuple(idx)}: got {got[tuple(idx)].item()!r}, want {want[tuple(idx)].item()!r}"

    def bits(self, name, got, want):
        """Same bit pattern in every element (NaN payloads included)."""
        got, want = got.detach().cpu(), want.detach().cpu()
        assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
        bad = ibits(got) != ibits(want)
        if bool(bad.any()):
            self.fail(f"{name}: not bit-identical: " + self._where(bad, got, want))

    def exact(self, name, got, want):
        """Equal values in every element (want holds no NaN; -0 == +0); a NaN in got is an unwritten or poisoned element."""
        got, want = got.detach().cpu().double(), want.detach().cpu().double()
        assert got.shape == want.shape, (name, got.shape, want.shape)
        bad = ~(got == want)
        if bool(bad.any()):
            self.fail(f"{name}: not exact: " + self._where(bad, got, want))

    def rounded16(self, name, got, want, signed_zero=True):
        """16-bit values: NaN exactly where want has NaN, identical bits elsewhere (infinities and, for a conversion, the sign of
        a zero included; an arithmetic result may be -0 where the fp64 reference is +0)."""
        got, want = got.detach().cpu(), want.detach().cpu()
        assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape)
        gn, wn = torch.isnan(got.float()), torch.isnan(want.float())
        bad = (gn != wn) | ((ibits(got) != ibits(want)) & ~wn)
        if not signed_zero:
            bad &= ~((got.float() == 0) & (want.float() == 0))
        if bool(bad.any()):
            self.fail(f"{name}: not the rounding of the exact value: " + self._where(bad, got.float(), want.float()))

    def bound(self, name, got, want, bnd):
        """|got - want| <= bnd per element (want fp64); records the worst ratio."""
        got, want = got.detach().cpu().double(), want.detach().cpu().double()
        bnd = torch.as_tensor(bnd, dtype=torch.float64).expand_as(want)
        assert got.shape == want.shape, (name, got.shape, want.shape)
        if not bool(torch.isfinite(got).all()):
            self.fig[name] = NAN
            self.fail(f"{name}: {int((~torch.isfinite(got)).sum())} non-finite (unwritten?) elements")
            return
        err = (got - want).abs()
        ratio = torch.where(err == 0, torch.zeros_like(err), err / bnd)
        self.fig[name] = float(ratio.max()) if ratio.numel() else 0.0
        bad = ~(err <= bnd)
        if bool(bad.any()):
            i = tuple(ratio.flatten().argmax().reshape(1).tolist()) if ratio.dim() == 1 else tuple(
                int(v) for v in (ratio == ratio.max()).nonzero()[0])
            self.fail(f"{name}: {int(bad.sum())} elements beyond the bound, worst {self.fig[name]:.3g} x at {i}: "
                      f"got {got[i].item()!r}, want {want[i].item()!r}, bound {bnd[i].item():.3e}")

    def done(self):
        assert not self.failed, f"{self.what}: " + "; ".join(self.failed) + f"   (figures: {self.fig})"
        return self.fig


def nan_tail(rep: Report, name: str, ws: Guarded, used: int):
    tail = ws.get()[0, used:]
    if not bool(torch.isnan(tail).all()):
        rep.fail(f"{name}: wrote behind its documented size ({int((~torch.isnan(tail)).sum())} of {WS_TAIL} floats)")


def vec(n: int, device="cpu", fill=NAN, dtype=torch.float32) -> Guarded:
    """A [1][n] Guarded whose sentinel bands hold about 4096 words (one row of a long vector), not 128 rows of n."""
    return Guarded(1, n, device=device, fill=fill, dtype=dtype, guard_rows=max(1, -(-4096 // n)))


def workspace(floats: int, device) -> Guarded:
    return vec(floats + WS_TAIL, device)


# ==================================================================================================== summation shapes

def wave_row_sum(groups: torch.Tensor) -> torch.Tensor:
    """groups [rows][n4]: the per-float4 partial sums of a row, in the order lane = i % 64, chunk = i // 64.  Each lane adds
    its chunks in order, then the 64 lanes are combined by the xor butterfly (32, 16, ..., 1)."""
    rows, n4 = groups.shape
    nc = -(-n4 // 64)
    g = torch.zeros((rows, nc * 64), dtype=groups.dtype)
    g[:, :n4] = groups
    g = g.view(rows, nc, 64)
    s = torch.zeros((rows, 64), dtype=groups.dtype)
    for c in range(nc):
        s = s + g[:, c]
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lane ^ o]
    return s[:, 0]


def quad(v: torch.Tensor) -> torch.Tensor:
    """[rows][D] -> [rows][D / 4]: (v0 + v1) + (v2 + v3) of each float4."""
    q = v.view(v.shape[0], -1, 4)
    return (q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3])


def reduce_partials(partial: torch.Tensor) -> torch.Tensor:
    """reduce_partials_kernel: [P][N] -> [N]; 64 row groups (p % 64) added in order, 64 -> 4 by 16 in order, then (a+b)+(c+d)."""
    P, N = partial.shape
    K = -(-P // 64)
    t = torch.zeros((K * 64, N), dtype=partial.dtype)
    t[:P] = partial
    t = t.view(K, 64, N)
    s = torch.zeros((64, N), dtype=partial.dtype)
    for k in range(K):
        s = s + t[k]
    s = s.view(4, 16, N)
    q = torch.zeros((4, N), dtype=partial.dtype)
    for k in range(16):
        q = q + s[:, k]
    return (q[0] + q[1]) + (q[2] + q[3])


def ln_blocks(rows: int) -> int:
    return min(-(-rows // 4), 1024)


def ln_block_partials(terms: torch.Tensor) -> torch.Tensor:
    """ln_bwd_kernel: [rows][D] per-row terms -> [blocks][D]; a wave adds its rows (stride 4 blocks) in order, the block adds
    its 4 waves in order."""
    rows, D = terms.shape
    blocks = ln_blocks(rows)
    stride = 4 * blocks
    K = -(-rows // stride)
    t = torch.zeros((K * stride, D), dtype=terms.dtype)
    t[:rows] = terms
    t = t.view(K, blocks, 4, D)
    acc = torch.zeros((blocks, 4, D), dtype=terms.dtype)
    for k in range(K):
        acc = acc + t[k]
    return ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]


def ln_col_depth(rows: int) -> int:
    """Additions on the longest path of one column sum of the LayerNorm backward."""
    blocks = ln_blocks(rows)
    return -(-rows // (4 * blocks)) + 3 + -(-blocks // 64) + 16 + 2


def row_depth(n: int) -> int:
    """Additions on the longest path of a row reduction over n elements (float4 groups, 64 lanes, butterfly)."""
    return -(-(n // 4) // 64) + 2 + 6


# ==================================================================================================== LayerNorm forward

LnFwdCase = namedtuple("LnFwdCase", "D rows stats")
LN_FWD_CASES = [LnFwdCase(D, rows, bool((i + j) % 2)) for i, D in enumerate(LN16_D) for j, rows in enumerate(LN16_ROWS)] + \
               [LnFwdCase(D, 5, bool(i % 2)) for i, D in enumerate(LN16_D)]
LN_EPS = 1e-5


def build_ln_fwd(c: LnFwdCase, device="cpu"):
    x = randn((c.rows, c.D), 7 * c.D + c.rows, 2.0) + 1.0
    x[0] = randn((c.D,), c.D + 1) + 100.0                  # a row whose mean is 100 x its spread: an uncentred variance shows here
    g, b = randn((c.D,), c.D + 2), randn((c.D,), c.D + 3)
    s = SimpleNamespace(case=c, x=x, g=g, b=b, xd=poisoned(x, c.D, device), gd=g.to(device), bd=b.to(device),
                        y=Guarded(c.rows, c.D, device=device), mean=vec(c.rows, device),
                        rstd=vec(c.rows, device))
    return s


def launch_ln_fwd(lib, s, stream) -> int:
    c = s.case
    return lib.dclip_layernorm_fwd(s.xd.data_ptr(), s.gd.data_ptr(), s.bd.data_ptr(), s.y.ptr, s.mean.ptr if c.stats else None,
                                   s.rstd.ptr if c.stats else None, c.rows, c.D, LN_EPS, stream)


def emulate_ln_fwd(s, fault=None):
    c = s.case
    x, g, b = s.x, s.g, s.b
    D = torch.tensor(float(c.D))
    mu = wave_row_sum(quad(x)) / D
    if fault == "uncentred":
        var = wave_row_sum(quad(x * x)) / D - mu * mu
    else:
        d = x - mu[:, None]
        var = wave_row_sum(quad(d * d)) / D
    rs = 1.0 / torch.sqrt(var + torch.tensor(LN_EPS))
    y = (x - mu[:, None]) * rs[:, None] * g + b
    if fault == "chunk_unwritten" and c.D >= 512:
        y[:, 256:512] = NAN
    s.y.payload.copy_(y)
    if c.stats:
        s.mean.payload.copy_(mu[None])
        s.rstd.payload.copy_(rs[None])


def ln_fwd_bounds(x, g, b, D: int):
    """fp64 LayerNorm of x (want, mean, rstd) and the per-element bounds of an fp32 evaluation by one wave per row:
    y: |g| rstd (e_mu + |d| (rho_rs + 3u)) + u |want|, with L = ceil(D / 256) + 8 the depth of a row sum,
    e_mu = gamma(L + 1) mean|x| the error of the mean, rho_v = gamma(L + 5) + e_mu^2 / var the relative error of the variance
    (a shift e of the mean changes sum (d - e)^2 only by D e^2, because sum d = 0) and rho_rs = rho_v / 2 + 2 ulp that of rsqrtf."""
    x, g, b = x.double(), g.double(), b.double()
    mu = x.mean(1)
    d = x - mu[:, None]
    var = (d * d).mean(1)
    rstd = 1.0 / torch.sqrt(var + LN_EPS)
    want = d * rstd[:, None] * g + b
    L = -(-D // 256) + 8
    e_mu = gamma(L + 1) * x.abs().mean(1)
    rho_v = gamma(L + 5) + e_mu ** 2 / (var + LN_EPS)
    rho_rs = 0.5 * rho_v / (1.0 - rho_v) + 2 * ULP
    bnd = g.abs() * rstd[:, None] * (e_mu[:, None] + d.abs() * (rho_rs[:, None] + 3 * U)) + U * want.abs() + F32_TINY
    return SimpleNamespace(want=want, bnd=bnd, mu=mu, rstd=rstd, e_mu=e_mu, rho_rs=rho_rs)


def verify_ln_fwd(s, what=None):
    """y, mean and rstd under the bounds of ln_fwd_bounds."""
    c = s.case
    rep = Report(what or f"layernorm_fwd {c}")
    rep.guards(y=s.y, mean=s.mean, rstd=s.rstd)
    r = ln_fwd_bounds(s.x, s.g, s.b, c.D)
    want, bnd, mu, rstd, e_mu, rho_rs = r.want, r.bnd, r.mu, r.rstd, r.e_mu, r.rho_rs
    rep.bound("y", s.y.get(), want, bnd)
    if c.stats:
        rep.bound("mean", s.mean.get()[0], mu, e_mu + U * mu.abs() + F32_TINY)
        rep.bound("rstd", s.rstd.get()[0], rstd, rho_rs * rstd)
        try:
            rep.fig.update(check_blocks({"mean_1e-5": (s.mean.get()[0], mu, TOL_LN), "rstd_1e-5": (s.rstd.get()[0], rstd, TOL_LN)},
                                        rep.what))
        except AssertionError as e:
            rep.fail(str(e))
    else:
        for name, gd in (("mean", s.mean), ("rstd", s.rstd)):
            if not bool(torch.isnan(gd.get()).all()):
                rep.fail(f"{name}: written although the pointer passed was null")
    return rep.done()


# ==================================================================================================== LayerNorm backward

# entry: "bwd" (dclip_layernorm_bwd), "ex" (dclip_layernorm_bwd_ex, bf16 copy), "ex_f16";  params: "both" | "gamma" | "beta" | "none"
LnBwdCase = namedtuple("LnBwdCase", "entry D rows res dx16 colsum params acc data")
LN_BWD_NAME = {"bwd": "layernorm_bwd", "ex": "layernorm_bwd", "ex_f16": "layernorm_bwd_f16"}
LN_BWD_TYPE = {"ex": "bf16", "ex_f16": "f16ex"}
LN_BWD_ROWS = [1, 3, 4, 5, 1001, 4101]
LN_BWD_BIG_D = [100, 260, 512, 516, 768, 772, 1024, 1028]        # one D per template instance at 4101 rows (a second row per wave)


def ln_bwd_cases():
    cases = []
    R = LN_BWD_ROWS[:4]                                   # the small row counts cycle; 1001 and 4101 rows are placed below
    for i, D in enumerate(LN16_D):
        r = lambda k: R[(i + k) % 4]                                                     # noqa: E731
        cases += [LnBwdCase("bwd", D, r(0), False, False, False, "both", 0, "int"),
                  LnBwdCase("ex", D, r(1), True, True, True, "both", 1, "int"),
                  LnBwdCase("ex_f16", D, r(2), False, True, True, "gamma", 0, "int"),
                  LnBwdCase("ex", D, r(3), True, True, False, "beta", 1, "int"),
                  LnBwdCase("ex_f16", D, r(4), True, True, False, "none", 0, "int"),     # the no-workspace launch
                  LnBwdCase("ex", D, r(5), False, False, True, "none", 0, "int"),        # column sums only
                  LnBwdCase("ex_f16", D, 1001 if i % 2 else r(6), True, False, False, "both", 1, "int"),
                  LnBwdCase("ex", D, r(7) if i % 2 else 1001, False, True, True, "both", 0, "int"),
                  LnBwdCase("bwd", D, 4, True, False, False, "gamma", 1, "int"),
                  LnBwdCase("ex_f16", D, 5, True, True, True, "both", 1, "gauss"),
                  LnBwdCase("ex", D, 1001 if i % 2 else 3, True, True, True, "both", 0, "gauss"),
                  LnBwdCase("bwd", D, 5, False, False, False, "both", 0, "gauss")]
    for i, D in enumerate(LN_BWD_BIG_D):
        cases.append(LnBwdCase(["ex", "ex_f16"][i % 2], D, 4101, True, True, True, "both", 1, "int"))
    cases.append(LnBwdCase("ex", 768, 4101, True, True, True, "both", 1, "gauss"))
    return cases


def ln_bwd_id(c) -> str:
    return (f"{c.entry}-D{c.D}-r{c.rows}-res{int(c.res)}-x16{int(c.dx16)}-cs{int(c.colsum)}-{c.params}-acc{c.acc}-{c.data}")


def ln_bwd_general(c) -> bool:
    """Integer data with non-zero c1 / c2: D a power of two (1 / D exact) and so few rows that the column sums of the dyadic dx
    stay below 24 bits; every other integer case uses rows whose two row sums are exactly zero."""
    return c.D & (c.D - 1) == 0 and c.rows <= 8


def ln_bwd_quantum(c) -> float:
    """Every exact dx of an integer case is a multiple of this."""
    return 1.0 / (8 * c.D) if ln_bwd_general(c) else (2.0 ** -6 if c.rows <= 1001 else 2.0 ** -5)      # rstd^2 / (2 D) at rstd = 1/2


def build_ln_bwd(c: LnBwdCase, device="cpu"):
    rows, D = c.rows, c.D
    seed = 13 * D + rows + 1000 * c.acc
    if c.data == "int":
        mean = ints((rows,), seed, -3, 3)
        rstd = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (rows,), generator=gen(seed + 1))]
        if ln_bwd_general(c):
            x = mean[:, None] + ints((rows, D), seed + 2)
            dy, g = ints((rows, D), seed + 3), ints((D,), seed + 4)
        else:                           # columns in pairs: same x and dy, opposite gamma -> sum dy g = sum dy g xhat = 0 in any order
            x = mean[:, None] + ints((rows, D // 2), seed + 2).repeat_interleave(2, 1)
            dy = ints((rows, D // 2), seed + 3).repeat_interleave(2, 1)
            gh = torch.tensor([-2.0, -1.0, 1.0, 2.0])[torch.randint(0, 4, (D // 2,), generator=gen(seed + 4))]
            g = torch.stack([gh, -gh], 1).reshape(D)
        # general rows: dx is a dyadic number of <= 20 bits and <= 8 of them sum exactly; zero-sum rows: dx = dy g rstd + dres is a
        # multiple of 1/64 (1/32 beyond 1001 rows) below 68 — up to 13 significant bits, more than bf16 (8) and fp16 (11) keep, so
        # dx16 is a real rounding — and the rows add up exactly (every partial sum is a multiple of the quantum, 24 bits at most)
        q = ln_bwd_quantum(c)
        dres = ints((rows, D), seed + 5, -2, 2) if ln_bwd_general(c) else ints((rows, D), seed + 5, -int(59 / q), int(59 / q)) * q
        init = [ints((D,), seed + 6 + k, -50, 50) for k in range(2)]
    else:
        x = randn((rows, D), seed + 2, 2.0) + 1.0
        xd = x.double()
        mean = xd.mean(1).float()
        rstd = (1.0 / torch.sqrt(xd.var(1, unbiased=False) + LN_EPS)).float()
        dy, g, dres = randn((rows, D), seed + 3), randn((D,), seed + 4), randn((rows, D), seed + 5)
        init = [randn((D,), seed + 6 + k, 3.0) for k in range(2)]
    ty = TYPES16[LN_BWD_TYPE[c.entry]] if c.dx16 else None
    s = SimpleNamespace(case=c, x=x, dy=dy, g=g, mean=mean, rstd=rstd, dres=dres if c.res else None, init=init, ty=ty)
    s.xd, s.dyd = poisoned(x, D, device), poisoned(dy, D, device)
    s.dresd = poisoned(dres, D, device) if c.res else None
    s.gd, s.meand, s.rstdd = g.to(device), mean.to(device), rstd.to(device)
    s.dx = Guarded(rows, D, device=device)
    s.dx16 = Guarded(rows, D, device=device, dtype=ty.dtype) if c.dx16 else None
    s.dgamma = vec(D, device, fill=init[0] if c.acc else NAN) if c.params in ("both", "gamma") else None
    s.dbeta = vec(D, device, fill=init[1] if c.acc else NAN) if c.params in ("both", "beta") else None
    s.colsum = vec(D, device, fill=init[0] if c.acc else NAN) if c.colsum else None   # always assigned
    s.ws_floats = ln_blocks(rows) * 3 * D
    s.ws = workspace(s.ws_floats, device) if (c.params != "none" or c.colsum) else None
    return s


def _p(g):
    return g.ptr if g is not None else None


def launch_ln_bwd(lib, s, stream, workspace_bytes=None) -> int:
    c = s.case
    wsb = (s.ws_floats * 4 if s.ws is not None else 0) if workspace_bytes is None else workspace_bytes
    head = (s.dyd.data_ptr(), s.xd.data_ptr(), s.gd.data_ptr(), s.meand.data_ptr(), s.rstdd.data_ptr(),
            s.dresd.data_ptr() if s.dresd is not None else None, s.dx.ptr)
    tail = (c.rows, c.D, c.acc, _p(s.ws), wsb, stream)
    if c.entry == "bwd":
        assert not c.dx16 and not c.colsum
        return lib.dclip_layernorm_bwd(*head, _p(s.dgamma), _p(s.dbeta), *tail)
    fn = lib.dclip_layernorm_bwd_ex if c.entry == "ex" else lib.dclip_layernorm_bwd_ex_f16
    return fn(*head, _p(s.dx16), _p(s.dgamma), _p(s.dbeta), _p(s.colsum), *tail)


def expected_ln_bwd_site(c) -> str:
    return LN_BWD_NAME[c.entry] + expected_ln16_variant(c.D)


def emulate_ln_bwd(s, fault=None):
    c = s.case
    x, dy, g, mu, rs = s.x, s.dy, s.g, s.mean[:, None], s.rstd[:, None]
    invD = torch.tensor(1.0) / torch.tensor(float(c.D))
    xh = (x - mu) * rs
    dyh = dy * g
    c1 = (wave_row_sum(quad(dyh * xh)) * invD)[:, None]
    c2 = (wave_row_sum(quad(dyh)) * invD)[:, None]
    o = (dyh - c2 - xh * c1) * rs
    if s.dres is not None:
        o = o + s.dres
        if fault == "dres_row_skipped":
            o[c.rows // 2] = o[c.rows // 2] - s.dres[c.rows // 2]
    if fault == "chunk_unwritten" and c.D >= 512:
        o[:, 256:512] = NAN
    s.dx.payload.copy_(o)
    if s.dx16 is not None:
        o16 = round16(o, s.ty)
        if fault == "dx16_truncated":
            o16 = (ibits(o) >> 16).to(torch.int16).view(torch.bfloat16) if s.ty.dtype == torch.bfloat16 else o16
        s.dx16.payload.copy_(o16)
    if s.ws is None:
        return
    dg = reduce_partials(ln_block_partials(dy * xh))
    db = reduce_partials(ln_block_partials(dy))
    if fault == "dgamma_dbeta_swapped":
        dg, db = db, dg
    used = ln_blocks(c.rows) * (3 if c.colsum else 2) * c.D
    s.ws.payload[0, :used] = 0.0                                   # the partials: some finite value
    if s.dgamma is not None:
        s.dgamma.payload.copy_((s.dgamma.payload[0] + dg if c.acc else dg)[None])
    if s.dbeta is not None:
        s.dbeta.payload.copy_((s.dbeta.payload[0] + db if c.acc else db)[None])
    if s.colsum is not None:
        cs = reduce_partials(ln_block_partials(torch.nan_to_num(o)))
        if fault == "colsum_accumulated" and c.acc:
            cs = s.colsum.payload[0] + cs
        s.colsum.payload.copy_(cs[None])


def ln_bwd_reference(s):
    c = s.case
    x, dy, g, mu, rs = s.x.double(), s.dy.double(), s.g.double(), s.mean.double()[:, None], s.rstd.double()[:, None]
    xh = (x - mu) * rs
    a = dy * g
    c1, c2 = (a * xh).sum(1, keepdim=True) / c.D, a.sum(1, keepdim=True) / c.D
    core = (a - c2 - xh * c1) * rs
    dx = core + (s.dres.double() if s.dres is not None else 0.0)
    return SimpleNamespace(xh=xh, a=a, c1=c1, c2=c2, dx=dx, rs=rs, dg=(dy * xh).sum(0), db=dy.sum(0), cs=dx.sum(0))


def verify_ln_bwd(s, what=None):
    """Integer data: dx, dx16 (the type's rounding of the exact dx), dgamma, dbeta and dx_colsum EXACT.  Gaussian data, with
    L = ceil(D / 256) + 8 (depth of a row sum) and Lc = ln_col_depth(rows) (depth of a column sum):
      e1 = gamma(L + 6) sum|a xh| / D, e2 = gamma(L + 4) sum|a| / D                      (a = dy g; errors of c1, c2)
      dx        rstd (e2 + |xh| e1 + 6u (|a| + |c2| + |xh c1|)) + 2u |want|
      dx16      that + u16 |want|
      dgamma    gamma(Lc + 3) sum_r |dy xh| (+ u |want| when accumulating);   dbeta  gamma(Lc) sum_r |dy| (+ u |want|)
      dx_colsum gamma(Lc) sum_r |dx| + sum_r bound(dx)."""
    c = s.case
    rep = Report(what or f"layernorm_bwd {ln_bwd_id(c)}")
    rep.guards(dx=s.dx, dx16=s.dx16, dgamma=s.dgamma, dbeta=s.dbeta, dx_colsum=s.colsum, workspace=s.ws)
    if s.ws is not None:
        nan_tail(rep, "workspace", s.ws, s.ws_floats)
    r = ln_bwd_reference(s)
    i0, i1 = s.init[0].double(), s.init[1].double()
    want_dg, want_db = r.dg + (i0 if c.acc else 0.0), r.db + (i1 if c.acc else 0.0)
    if c.data == "int":
        quantum = ln_bwd_quantum(c)
        assert bool((r.dx == r.dx.float().double()).all()) and bool((r.dx / quantum == (r.dx / quantum).round()).all()) and \
            c.rows * float(r.dx.abs().max()) / quantum <= 2 ** 24, "the construction is not exact"
        rep.exact("dx", s.dx.get(), r.dx)
        if s.dx16 is not None:
            rep.rounded16("dx16", s.dx16.get(), round16(r.dx.float(), s.ty), signed_zero=False)
        for name, gd, want in (("dgamma", s.dgamma, want_dg), ("dbeta", s.dbeta, want_db), ("dx_colsum", s.colsum, r.cs)):
            if gd is not None:
                rep.exact(name, gd.get()[0], want)
        return rep.done()
    L, Lc = -(-c.D // 256) + 8, ln_col_depth(c.rows)
    e1 = gamma(L + 6) * (r.a * r.xh).abs().sum(1, keepdim=True) / c.D
    e2 = gamma(L + 4) * r.a.abs().sum(1, keepdim=True) / c.D
    bdx = r.rs * (e2 + r.xh.abs() * e1 + 6 * U * (r.a.abs() + r.c2.abs() + (r.xh * r.c1).abs())) + 2 * U * r.dx.abs() + F32_TINY
    rep.bound("dx", s.dx.get(), r.dx, bdx)
    if s.dx16 is not None:
        rep.bound("dx16", s.dx16.get().float(), r.dx, bdx + s.ty.u * r.dx.abs() + (F16_SUB if s.ty.dtype == torch.float16 else 0.0))
    dyxh = (s.dy.double() * r.xh).abs().sum(0)
    if s.dgamma is not None:
        rep.bound("dgamma", s.dgamma.get()[0], want_dg, gamma(Lc + 3) * dyxh + c.acc * U * want_dg.abs() + F32_TINY)
    if s.dbeta is not None:
        rep.bound("dbeta", s.dbeta.get()[0], want_db, gamma(Lc) * s.dy.double().abs().sum(0) + c.acc * U * want_db.abs() + F32_TINY)
    if s.colsum is not None:
        rep.bound("dx_colsum", s.colsum.get()[0], r.cs, gamma(Lc) * r.dx.abs().sum(0) + bdx.sum(0))
    return rep.done()


# ==================================================================================================== column / row sums

ColsumCase = namedtuple("ColsumCase", "ty M N pad acc")
COLSUM_M = [1, 3, 4, 5, 127, 128, 129, 8191, 8192, 8193, 10000]
COLSUM_N = [4, 252, 256, 260, 1028]
COLSUM_FN = {"f32": "colsum_f32", "bf16": "colsum_bf16", "f16ex": "colsum_f16"}
COLSUM_SITE = {"f32": "colsum.reduce", "bf16": "colsum_bf16", "f16ex": "colsum_f16"}


def colsum_cases():
    tys = list(COLSUM_FN)
    out = []
    for i, M in enumerate(COLSUM_M):
        for j, N in enumerate(COLSUM_N):
            k = i * len(COLSUM_N) + j
            out.append(ColsumCase(tys[k % 3], M, N, PADS[(k // 3) % 3], (k // 9) % 2))
    out += [ColsumCase(ty, M, 1028, 4, acc) for ty in tys for M, acc in ((10000, 1), (129, 0), (8193, 1))]
    return sorted(set(out))


def colsum_splits(M: int) -> int:
    return max(1, min(64, -(-M // 128)))


def build_colsum(c: ColsumCase, device="cpu"):
    X = ints((c.M, c.N), c.M + c.N)
    dtype = torch.float32 if c.ty == "f32" else TYPES16[c.ty].dtype
    init = ints((c.N,), c.N + 5, -50, 50)
    s = SimpleNamespace(case=c, X=X, init=init, ldx=c.N + c.pad, Xd=poisoned(X, c.N + c.pad, device, dtype=dtype),
                        out=vec(c.N, device, fill=init if c.acc else NAN))
    s.ws_floats = colsum_splits(c.M) * c.N
    s.ws = workspace(s.ws_floats, device)
    return s


def launch_colsum(lib, s, stream, workspace_bytes=None) -> int:
    c = s.case
    fn = getattr(lib, "dclip_" + COLSUM_FN[c.ty])
    return fn(s.Xd.data_ptr(), s.out.ptr, c.M, c.N, s.ldx, c.acc, s.ws.ptr, s.ws_floats * 4 if workspace_bytes is None else workspace_bytes,
              stream)


def emulate_colsum(s, fault=None):
    c = s.case
    S = colsum_splits(c.M)
    rows_per = -(-c.M // S)
    K = -(-rows_per // 4)
    t = torch.zeros((S, K * 4, c.N))
    for y in range(S):
        blk = s.X[y * rows_per:min(c.M, (y + 1) * rows_per)]
        t[y, :blk.shape[0]] = blk
    t = t.view(S, K, 4, c.N)
    acc = torch.zeros((S, 4, c.N))
    for k in range(K):
        acc = acc + t[:, k]
    part = (acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])
    if fault == "split_dropped":
        part[S // 2] = 0.0
    if fault == "split_twice":
        part[S // 2] = part[S // 2] * 2
    s.ws.payload[0, :S * c.N] = part.reshape(-1)
    tot = reduce_partials(part)
    s.out.payload.copy_((s.out.payload[0] + tot if c.acc else tot)[None])


def verify_colsum(s, what=None):
    c = s.case
    rep = Report(what or f"colsum {c}")
    rep.guards(out=s.out, workspace=s.ws)
    nan_tail(rep, "workspace", s.ws, s.ws_floats)
    want = s.X.long().sum(0) + (s.init.long() if c.acc else 0)
    rep.exact("out", s.out.get()[0], want)
    return rep.done()


RowsumCase = namedtuple("RowsumCase", "ty R n pad")
ROWSUM_R = [1, 3, 4, 5, 1001]
ROWSUM_N = [1, 7, 8, 9, 511, 512, 513, 520, 1283]
ROWSUM_PADS = [0, 8, 40]


def rowsum_cases():
    return sorted(set([RowsumCase(TY2[(i + j) % 2], R, n, ROWSUM_PADS[(i * 9 + j) % 3]) for i, R in enumerate(ROWSUM_R)
                       for j, n in enumerate(ROWSUM_N)] + [RowsumCase(ty, 5, n, 40) for ty in TY2 for n in (513, 1283, 7)]))


def build_rowsum(c: RowsumCase, device="cpu"):
    x = ints((c.R, c.n), c.R * 7 + c.n)
    ld = roundup(c.n, 8) + c.pad
    return SimpleNamespace(case=c, x=x, ld=ld, xd=poisoned(x, ld, device, dtype=TYPES16[c.ty].dtype), out=vec(c.R, device))


def launch_rowsum(lib, s, stream) -> int:
    c = s.case
    fn = lib.dclip_rowsum_bf16 if c.ty == "bf16" else lib.dclip_rowsum_f16
    return fn(s.xd.data_ptr(), s.out.ptr, c.R, c.n, s.ld, stream)


def emulate_rowsum(s, fault=None):
    x = s.x if fault != "tail_skipped" else s.x[:, :s.case.n & ~7]
    s.out.payload.copy_(x.sum(1)[None])


def verify_rowsum(s, what=None):
    rep = Report(what or f"rowsum {s.case}")
    rep.guards(out=s.out)
    rep.exact("out", s.out.get()[0], s.x.long().sum(1))
    return rep.done()


# ==================================================================================================== transpose / mt_weights

TransCase = namedtuple("TransCase", "ty rows cols src16 xpad tpad copy")      # copy: None (no y_copy) or the pad of ldy
TRANS_ROWS = [1, 7, 63, 64, 65, 85, 513]
TRANS_COLS = [1, 3, 4, 5, 63, 64, 65, 132, 260]
TRANS_TPADS = [0, 8, 64, 72]
TRANS_COPY = [None, 0, 4]


def trans_cases():
    out = []
    for i, rows in enumerate(TRANS_ROWS):
        for j, cols in enumerate(TRANS_COLS):
            k = i * len(TRANS_COLS) + j
            out.append(TransCase(TY2[k % 2], rows, cols, bool((k // 2) % 2), PADS[k % 3], TRANS_TPADS[(k // 3) % 4], TRANS_COPY[(k // 4) % 3]))
    for k, (rows, cols) in enumerate([(65, 65), (513, 260), (1, 1), (85, 132)]):      # every option on four shapes
        out += [TransCase(ty, rows, cols, src16, PADS[(k + a) % 3], tp, cp) for a, (ty, src16, tp, cp) in enumerate(
            (t, s16, tp, cp) for t in TY2 for s16 in (False, True) for tp, cp in zip(TRANS_TPADS, [None, 0, 4, 4]))]
    return sorted(set(out), key=str)


def trans_input(rows, cols, ty, src16, seed=0):
    x = cast_input(rows, cols, seed)
    return round16(x, ty) if src16 else x


def build_trans(c: TransCase, device="cpu"):
    ty = TYPES16[c.ty]
    x = trans_input(c.rows, c.cols, ty, c.src16)
    ldx, ldyT = roundup(c.cols, 4) + c.xpad, roundup(c.rows, 8) + c.tpad
    s = SimpleNamespace(case=c, ty=ty, x=x, ldx=ldx, ldyT=ldyT, xd=poisoned(x, ldx, device, dtype=x.dtype),
                        yT=Guarded(c.cols, ldyT, device=device, dtype=ty.dtype), ycopy=None, ldy=0)
    if c.copy is not None:
        s.ldy = roundup(c.cols, 4) + c.copy
        s.ycopy = Guarded(c.rows, c.cols, s.ldy, device=device, dtype=ty.dtype)
    return s


def launch_trans(lib, s, stream) -> int:
    c = s.case
    fn = lib.dclip_transpose_to_bf16 if c.ty == "bf16" else lib.dclip_transpose_to_f16
    return fn(s.xd.data_ptr(), int(c.src16), s.yT.ptr, _p(s.ycopy), c.rows, c.cols, s.ldx, s.ldyT, s.ldy, stream)


def emulate_trans(s, fault=None):
    c = s.case
    ty = TYPES16["f16"] if fault == "saturating" else s.ty
    y = s.x if c.src16 else round16(s.x, ty)
    out = torch.zeros((c.cols, s.ldyT), dtype=s.ty.dtype)
    out[:, :c.rows] = y.t()
    if fault == "padding_unwritten":
        out[:, c.rows:] = s.yT.payload[:, c.rows:]
    s.yT.payload.copy_(out)
    if fault == "past_ldyT":
        s.yT.buf[s.yT.guard + c.cols * s.ldyT] = 0                     # one 16-bit word behind the last row
    if s.ycopy is not None:
        s.ycopy.payload.copy_(y)


def verify_trans(s, what=None):
    """yT[:, :rows] and y_copy are x.to(dtype) as torch computes it (IEEE: a finite fp32 beyond +-65504 becomes +-inf in fp16), or
    the bits of a 16-bit x; yT[:, rows:ldyT] is zero; y_copy columns cols..ldy keep the sentinel (Guarded padding)."""
    c = s.case
    rep = Report(what or f"transpose {c}")
    rep.guards(yT=s.yT, y_copy=s.ycopy)
    want = s.x if c.src16 else s.x.to(s.ty.dtype)
    got = s.yT.get()
    check = rep.bits if c.src16 else rep.rounded16
    check("yT", got[:, :c.rows], want.t().contiguous())
    if not bool((ibits(got[:, c.rows:]) == 0).all()):
        rep.fail("yT: columns rows..ldyT must be zero-filled")
    if s.ycopy is not None:
        check("y_copy", s.ycopy.get(), want)
    return rep.done()


MT_SHAPES = [(8, 8), (72, 40), (64, 64), (65, 68), (130, 260), (768, 64)]
MT_TPADS = [0, 8, 72]
MT_MODES = ["both", "dst", "dstT"]
MtwCase = namedtuple("MtwCase", "ty order shift")           # order: a permutation of range(len(MT_SHAPES)) or one index
MTW_CASES = [MtwCase(ty, order, shift) for ty in TY2 for order, shift in
             (((0, 1, 2, 3, 4, 5), 0), ((5, 3, 4, 0, 2, 1), 1), ((2, 5, 1, 4, 0, 3), 2), ((4,), 0), ((0,), 1), ((5,), 2))]


def build_mtw(c: MtwCase, device="cpu"):
    ty = TYPES16[c.ty]
    recs, tile0 = [], 0
    for pos, k in enumerate(c.order):
        rows, cols = MT_SHAPES[k]
        j = k + c.shift
        ld, ldT, mode = cols + PADS[j % 3], roundup(rows, 8) + MT_TPADS[(j // 3 + j) % 3], MT_MODES[(j + pos) % 3]
        src = cast_input(rows, cols, seed=k)
        r = SimpleNamespace(rows=rows, cols=cols, ld=ld, ldT=ldT, mode=mode, src=src, srcd=poisoned(src, cols, device),
                            dst=Guarded(rows, ld, device=device, dtype=ty.dtype) if mode != "dstT" else None,
                            dstT=Guarded(cols, ldT, device=device, dtype=ty.dtype) if mode != "dst" else None, tile0=tile0)
        r.tiles_c, r.tiles_r = -(-max(cols, ld) // 64), -(-max(rows, ldT) // 64)
        tile0 += r.tiles_c * r.tiles_r
        recs.append(r)
    blob = b"".join(struct.pack("<QQQiiiiii", r.srcd.data_ptr(), _p(r.dst) or 0, _p(r.dstT) or 0, r.rows, r.cols, r.ld, r.ldT, r.tile0,
                                r.tiles_c) for r in recs)
    table = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(device)
    return SimpleNamespace(case=c, ty=ty, recs=recs, table=table, total=tile0)


def launch_mtw(lib, s, stream) -> int:
    assert lib.dclip_mt_weights_record_bytes() == 48
    fn = lib.dclip_mt_weights_bf16 if s.case.ty == "bf16" else lib.dclip_mt_weights_f16
    return fn(s.table.data_ptr(), len(s.recs), s.total, stream)


def emulate_mtw(s, fault=None):
    for i, r in enumerate(s.recs):
        src = r.src
        if fault == "wrong_tensor_tile" and i > 0 and r.rows >= 8 and r.cols >= 8:       # the first tile holds the previous tensor's
            src = src.clone()
            prev = s.recs[i - 1].src
            h, w = min(64, r.rows, prev.shape[0]), min(64, r.cols, prev.shape[1])
            src[:h, :w] = prev[:h, :w]
        y = round16(src, s.ty)
        if r.dst is not None:
            d = torch.zeros((r.rows, r.ld), dtype=s.ty.dtype)
            d[:, :r.cols] = y
            r.dst.payload.copy_(d)
        if r.dstT is not None:
            d = torch.zeros((r.cols, r.ldT), dtype=s.ty.dtype)
            d[:, :r.rows] = y.t()
            r.dstT.payload.copy_(d)


def verify_mtw(s, what=None):
    rep = Report(what or f"mt_weights {s.case}")
    for i, r in enumerate(s.recs):
        want = r.src.to(s.ty.dtype)
        rep.guards(**{f"dst[{i}]": r.dst, f"dstT[{i}]": r.dstT})
        if r.dst is not None:
            got = r.dst.get()
            rep.rounded16(f"dst[{i}] {r.rows}x{r.cols}", got[:, :r.cols], want)
            if not bool((ibits(got[:, r.cols:]) == 0).all()):
                rep.fail(f"dst[{i}]: columns cols..ld must be zero-filled")
        if r.dstT is not None:
            got = r.dstT.get()
            rep.rounded16(f"dstT[{i}] {r.rows}x{r.cols}", got[:, :r.rows], want.t().contiguous())
            if not bool((ibits(got[:, r.rows:]) == 0).all()):
                rep.fail(f"dstT[{i}]: columns rows..ldT must be zero-filled")
    return rep.done()


# ==================================================================================================== embed.hip

Im2colCase = namedtuple("Im2colCase", "ty B C H p pad offset")       # ty: "f32" | "bf16" | "f16" (saturating);  offset: cols at base + 4 bytes
IM2COL_SCALAR = [(2, 4), (6, 12), (14, 28)]
IM2COL_VECTOR = [(4, 8), (8, 16), (16, 32), (32, 64)]


def im2col_cases():
    out = []
    for k, (p, H) in enumerate(IM2COL_SCALAR + IM2COL_VECTOR):
        for C in (1, 3):
            for B in (1, 3):
                out.append(Im2colCase("f32", B, C, H, p, 0, False))
    out.append(Im2colCase("f32", 3, 3, 16, 8, 0, True))                    # vector-eligible, misaligned destination -> scalar
    out.append(Im2colCase("f32", 1, 1, 64, 32, 0, True))
    for ty in ("bf16", "f16"):
        for k, (p, H) in enumerate(IM2COL_VECTOR):
            for j, (B, C) in enumerate(((1, 1), (3, 3), (1, 3))):
                out.append(Im2colCase(ty, B, C, H, p, PADS[(k + j) % 3], False))
    out.append(Im2colCase("f32", 8, 3, 224, 14, 0, False))                 # > 4096 workgroups: the grid-stride loops take a second turn
    out += [Im2colCase(ty, 29, 3, 224, 32, 4 if ty != "f32" else 0, False) for ty in ("f32", "bf16", "f16")]
    return out


def expected_im2col_site(c) -> str:
    if c.ty != "f32":
        return "im2col_" + c.ty
    return "im2col.vec" if c.p % 4 == 0 and not c.offset else "im2col.scalar"


def im2col_index(pix, p):
    B, C, H, _ = pix.shape
    g = H // p
    return pix.reshape(B, C, g, p, g, p).permute(0, 2, 4, 1, 3, 5).reshape(B * g * g, C * p * p)


def build_im2col(c: Im2colCase, device="cpu"):
    seed = c.B * 1000 + c.C * 100 + c.H + c.p
    if c.ty == "f32":
        pix = random_bits((c.B, c.C, c.H, c.H), seed)
    else:
        pix = cast_input(c.B * c.C * c.H, c.H, seed).reshape(c.B, c.C, c.H, c.H)
    g = c.H // c.p
    rows, kdim = c.B * g * g, c.C * c.p * c.p
    s = SimpleNamespace(case=c, pix=pix, rows=rows, kdim=kdim, ldc=kdim + c.pad,
                        pixd=poisoned(pix.reshape(-1, c.H), c.H, device))          # NaN rows behind the last image
    if c.ty == "f32":
        s.cols = vec(rows * kdim + 1, device) if c.offset else Guarded(rows, kdim, device=device)
    else:
        s.cols = Guarded(rows, kdim, s.ldc, device=device, dtype=TYPES16[c.ty].dtype)
    return s


def launch_im2col(lib, s, stream) -> int:
    c = s.case
    if c.ty == "f32":
        return lib.dclip_im2col(s.pixd.data_ptr(), s.cols.ptr + (4 if c.offset else 0), c.B, c.C, c.H, c.H, c.p, stream)
    fn = lib.dclip_im2col_bf16 if c.ty == "bf16" else lib.dclip_im2col_f16
    return fn(s.pixd.data_ptr(), s.cols.ptr, c.B, c.C, c.H, c.H, c.p, s.ldc, stream)


def emulate_im2col(s, fault=None):
    c = s.case
    pix = s.pix.transpose(2, 3) if fault == "pxpy_swapped" else s.pix
    want = im2col_index(pix, c.p)
    if c.ty != "f32":
        want = round16(want, TYPES16[c.ty])
    if c.offset:
        s.cols.payload[0, 1:] = want.reshape(-1)
    else:
        s.cols.payload.copy_(want)


def verify_im2col(s, what=None):
    """fp32: the bit patterns of the torch index expression (random bits: NaN payloads included).  16-bit: its rounding in the
    type (bf16, or the SATURATING fp16 of the frozen towers); columns C p^2..ldc keep the sentinel (Guarded padding)."""
    c = s.case
    rep = Report(what or f"im2col {c}")
    rep.guards(cols=s.cols)
    want = im2col_index(s.pix, c.p)
    if c.ty == "f32":
        got = s.cols.get()
        if c.offset:
            if not bool(torch.isnan(got[0, :1]).all()):
                rep.fail("cols: the float in front of the misaligned destination was written")
            got = got[0, 1:].reshape(s.rows, s.kdim)
        rep.bits("cols", got, want.contiguous())
    else:
        rep.rounded16("cols", s.cols.get(), round16(want, TYPES16[c.ty]))
    return rep.done()


AssembleCase = namedtuple("AssembleCase", "B S D")
ASSEMBLE_CASES = [AssembleCase(B, S, D) for B in (1, 3) for S in (2, 5, 50) for D in (4, 64, 772)] + [AssembleCase(28, 197, 768)]


def build_assemble(c: AssembleCase, device="cpu"):
    seed = c.B + 10 * c.S + c.D
    patch, cls, pos = randn((c.B * (c.S - 1), c.D), seed), randn((c.D,), seed + 1), randn((c.S, c.D), seed + 2)
    dx = random_bits((c.B * c.S, c.D), seed + 3)
    return SimpleNamespace(case=c, patch=patch, cls=cls, pos=pos, dx=dx, patchd=poisoned(patch, c.D, device), clsd=cls.to(device),
                           posd=poisoned(pos, c.D, device), dxd=poisoned(dx, c.D, device), x=Guarded(c.B * c.S, c.D, device=device),
                           dpatch=Guarded(c.B * (c.S - 1), c.D, device=device))


def launch_assemble(lib, s, stream, lasts=None) -> int:
    c = s.case
    rc = lib.dclip_vision_assemble_fwd(s.patchd.data_ptr(), s.clsd.data_ptr(), s.posd.data_ptr(), s.x.ptr, c.B, c.S, c.D, stream)
    if lasts is not None:
        lasts.append(lib.dclip_last_launch().decode())
    return rc or lib.dclip_vision_assemble_bwd(s.dxd.data_ptr(), s.dpatch.ptr, c.B, c.S, c.D, stream)


def assemble_want(s, fault=None):
    c = s.case
    x = torch.cat([s.cls.expand(c.B, 1, c.D), s.patch.view(c.B, c.S - 1, c.D)], 1)
    if fault == "class_on_patch0":
        x[:, 1] = s.cls
    return (x + s.pos).reshape(c.B * c.S, c.D), s.dx.view(c.B, c.S, c.D)[:, 1:].reshape(-1, c.D)


def emulate_assemble(s, fault=None):
    x, dp = assemble_want(s, fault)
    s.x.payload.copy_(x)
    s.dpatch.payload.copy_(dp)


def verify_assemble(s, what=None):
    rep = Report(what or f"vision_assemble {s.case}")
    rep.guards(x=s.x, dpatch=s.dpatch)
    x, dp = assemble_want(s)
    rep.bits("x", s.x.get(), x)                      # one fp32 add of finite values: the same bits as torch's
    rep.bits("dpatch", s.dpatch.get(), dp.contiguous())
    return rep.done()


TextCase = namedtuple("TextCase", "B T D vocab ids")                  # ids: "edge" | "same" | "random"
TEXT_CASES = [TextCase(B, T, D, 50, kind) for (B, T), kind in zip(((2, 1), (3, 8), (2, 77), (5, 8), (1, 77), (3, 1)),
                                                                   ("edge", "edge", "edge", "same", "random", "same"))
              for D in (4, 64)] + [TextCase(64, 77, 1024, 50, "edge")]
TEXT_EDGE_IDS = [0, 49, -1, 50, 2 ** 40, -2 ** 40, 17, 2 ** 31, 2 ** 32 + 3]


def build_text(c: TextCase, device="cpu"):
    seed = c.B * 100 + c.T + c.D
    n = c.B * c.T
    ids = torch.randint(0, c.vocab, (n,), generator=gen(seed))
    if c.ids == "edge":
        e = torch.tensor(TEXT_EDGE_IDS)
        ids[:min(n, e.numel())] = e[:n]
        ids[-1] = c.vocab - 1 if n > 1 else ids[-1]
    elif c.ids == "same":
        ids[:] = 7
    tok, pos = randn((c.vocab, c.D), seed + 1), randn((c.T, c.D), seed + 2)
    dx, dtok0 = ints((n, c.D), seed + 3), ints((c.vocab, c.D), seed + 4, -50, 50)
    idsd = torch.cat([ids, torch.full((8,), 2 ** 62)]).to(device)                  # ids behind the last caption would be far outside
    return SimpleNamespace(case=c, ids=ids, tok=tok, pos=pos, dx=dx, dtok0=dtok0, idsd=idsd, tokd=poisoned(tok, c.D, device),
                           posd=poisoned(pos, c.D, device), dxd=poisoned(dx, c.D, device), x=Guarded(n, c.D, device=device),
                           dtok=Guarded(c.vocab, c.D, device=device, fill=dtok0))


def launch_text(lib, s, stream, lasts=None) -> int:
    c = s.case
    rc = lib.dclip_text_embed_fwd(s.idsd.data_ptr(), s.tokd.data_ptr(), s.posd.data_ptr(), s.x.ptr, c.B, c.T, c.D, c.vocab, stream)
    if lasts is not None:
        lasts.append(lib.dclip_last_launch().decode())
    return rc or lib.dclip_text_embed_bwd(s.idsd.data_ptr(), s.dxd.data_ptr(), s.dtok.ptr, c.B, c.T, c.D, c.vocab, stream)


def text_want(s):
    c = s.case
    ids = s.ids.clamp(0, c.vocab - 1)                                  # the documented clamp
    x = s.tok[ids] + s.pos.repeat(c.B, 1)
    dtok = s.dtok0.long().index_add(0, ids, s.dx.long())
    return x, dtok


def emulate_text(s, fault=None):
    x, dtok = text_want(s)
    s.x.payload.copy_(x)
    s.dtok.payload.copy_(dtok.float())


def verify_text(s, what=None):
    rep = Report(what or f"text_embed {s.case}")
    rep.guards(x=s.x, dtok=s.dtok)
    x, dtok = text_want(s)
    rep.bits("x", s.x.get(), x)
    rep.exact("dtok", s.dtok.get(), dtok)                 # integer atomics: order-independent, exact
    return rep.done()


EosCase = namedtuple("EosCase", "B T eos")
EOS_CASES = [EosCase(B, T, 49407 if (i + j) % 3 else 2 ** 33 + 5) for i, B in enumerate((1, 4, 5, 9)) for j, T in enumerate((1, 63, 64, 65, 77, 200))]


def build_eos(c: EosCase, device="cpu"):
    ids = torch.randint(0, 1000, (c.B, c.T), generator=gen(c.B * 1000 + c.T))
    places = [(0,), (63,), (64,), (c.T - 1,), (), (c.T // 2, c.T - 1), (5, 6, 7), (c.T - 1, 0), (64, 63)]
    for b in range(c.B):
        at = sorted({t for t in places[(b + c.T) % len(places)] if t < c.T})
        for t in at:
            ids[b, t] = c.eos
    if c.eos >= 2 ** 31:                                             # an id that equals the EOS id in its low 32 bits only
        for b in range(c.B):
            if int(ids[b, 0]) != c.eos:
                ids[b, 0] = c.eos & 0xFFFFFFFF
    idsd = torch.cat([ids.reshape(-1), torch.full((64,), c.eos)]).to(device)       # EOS ids behind the last row must not be seen
    return SimpleNamespace(case=c, ids=ids, idsd=idsd, idx=vec(c.B, device))


def launch_eos(lib, s, stream) -> int:
    return lib.dclip_first_eos(s.idsd.data_ptr(), s.idx.ptr, s.case.B, s.case.T, s.case.eos, stream)


def eos_want(s):
    hit = s.ids == s.case.eos
    return torch.where(hit.any(1), hit.int().argmax(1), torch.zeros(s.case.B, dtype=torch.long)).to(torch.int32)


def emulate_eos(s, fault=None):
    hit = s.ids == s.case.eos
    got = eos_want(s)
    if fault == "last_eos":
        last = s.case.T - 1 - hit.flip(1).int().argmax(1)
        got = torch.where(hit.any(1), last, torch.zeros_like(last)).to(torch.int32)
    s.idx.payload.view(torch.int32).copy_(got[None])


def verify_eos(s, what=None):
    rep = Report(what or f"first_eos {s.case}")
    rep.guards(idx=s.idx)
    got = s.idx.get().view(torch.int32)[0]
    want = eos_want(s)
    if not torch.equal(got, want):
        rep.fail(f"idx: got {got.tolist()}, want {want.tolist()}")
    return rep.done()


RowsCase = namedtuple("RowsCase", "B S D idx")                      # idx: False = NULL (row 0)
ROWS_CASES = [RowsCase(B, S, D, idx) for B in (1, 3) for S in (1, 5) for D in (4, 772) for idx in (False, True)] + \
             [RowsCase(28, 197, 768, True), RowsCase(4200, 2, 1024, True)]          # scatter / gather beyond 4096 workgroups


def build_rows(c: RowsCase, device="cpu"):
    seed = c.B + 10 * c.S + c.D
    x, dout = random_bits((c.B * c.S, c.D), seed), random_bits((c.B, c.D), seed + 1)
    idx = torch.randint(0, c.S, (c.B,), generator=gen(seed + 2)).to(torch.int32)
    idx[0], idx[-1] = c.S - 1, (0 if c.B > 1 else c.S - 1)
    return SimpleNamespace(case=c, x=x, dout=dout, idx=idx, xd=poisoned(x, c.D, device), doutd=poisoned(dout, c.D, device),
                           idxd=idx.to(device), out=Guarded(c.B, c.D, device=device), dx=Guarded(c.B * c.S, c.D, device=device))


def launch_rows(lib, s, stream, lasts=None) -> int:
    c = s.case
    ip = s.idxd.data_ptr() if c.idx else None
    rc = lib.dclip_gather_rows(s.xd.data_ptr(), ip, s.out.ptr, c.B, c.S, c.D, stream)
    if lasts is not None:
        lasts.append(lib.dclip_last_launch().decode())
    return rc or lib.dclip_scatter_rows(s.doutd.data_ptr(), ip, s.dx.ptr, c.B, c.S, c.D, stream)


def rows_want(s):
    c = s.case
    sel = s.idx.long() if c.idx else torch.zeros(c.B, dtype=torch.long)
    out = s.x.view(c.B, c.S, c.D)[torch.arange(c.B), sel]
    dx = torch.zeros((c.B, c.S, c.D))
    dx.view(torch.int32)[torch.arange(c.B), sel] = s.dout.view(torch.int32)
    return out.contiguous(), dx.view(c.B * c.S, c.D)


def emulate_rows(s, fault=None):
    out, dx = rows_want(s)
    s.out.payload.copy_(out)
    if fault == "unselected_unwritten":
        keep = s.dx.payload.clone()
        sel = dx.view(torch.int32) != 0
        keep.view(torch.int32)[sel] = dx.view(torch.int32)[sel]
        dx = keep
    s.dx.payload.view(torch.int32).copy_(dx.view(torch.int32))


def verify_rows(s, what=None):
    rep = Report(what or f"gather/scatter_rows {s.case}")
    rep.guards(out=s.out, dx=s.dx)
    out, dx = rows_want(s)
    rep.bits("out", s.out.get(), out)
    rep.bits("dx", s.dx.get(), dx)
    return rep.done()


# ==================================================================================================== loss.hip

NormCase = namedtuple("NormCase", "B P inv acc")
LOSS_B = [1, 3, 4, 5, 9]
LOSS_P = [4, 64, 252, 256, 260, 512, 768]
NORM_CASES = [NormCase(B, P, bool((i + j) % 3), (i + j) % 2) for i, B in enumerate(LOSS_B) for j, P in enumerate(LOSS_P)]
NORM_EPS = 1e-12


def special_rows(x, eps=NORM_EPS):
    """Row 0 zero, row 1 with a norm below eps (non-zero), row 2 just above eps — as far as the matrix has rows."""
    B, P = x.shape
    x[0] = 0.0
    if B > 1:
        x[1] = 0.0
        x[1, :2] = torch.tensor([3e-13, -4e-13])          # norm 5e-13 < eps
    if B > 2:
        x[2] = 0.0
        x[2, P - 1], x[2, 0] = 1.2e-12, 0.9e-12           # norm 1.5e-12 > eps
    return x


def build_norm(c: NormCase, device="cpu"):
    seed = 31 * c.B + c.P
    x = special_rows(randn((c.B, c.P), seed, 3.0))
    xd64 = x.double()
    nrm = xd64.norm(dim=1)
    inv32 = torch.where(nrm >= NORM_EPS, (1.0 / nrm.clamp_min(NORM_EPS)).float(), torch.tensor(1.0) / torch.tensor(NORM_EPS))
    xhat32 = (xd64 * inv32.double()[:, None]).float()               # the backward's inputs: fp32 values close to the forward's results
    dxhat, dx0 = randn((c.B, c.P), seed + 1), randn((c.B, c.P), seed + 2)
    return SimpleNamespace(case=c, x=x, inv32=inv32, xhat32=xhat32, dxhat=dxhat, dx0=dx0, xd=poisoned(x, c.P, device),
                           invd=inv32.to(device), xhatd=poisoned(xhat32, c.P, device), dxhatd=poisoned(dxhat, c.P, device),
                           xhat=Guarded(c.B, c.P, device=device), inv=vec(c.B, device),
                           dx=Guarded(c.B, c.P, device=device, fill=dx0 if c.acc else NAN))


def launch_norm(lib, s, stream, lasts=None) -> int:
    c = s.case
    rc = lib.dclip_normalize_rows_fwd(s.xd.data_ptr(), s.xhat.ptr, s.inv.ptr if c.inv else None, c.B, c.P, NORM_EPS, stream)
    if lasts is not None:
        lasts.append(lib.dclip_last_launch().decode())
    return rc or lib.dclip_normalize_rows_bwd(s.dxhatd.data_ptr(), s.xhatd.data_ptr(), s.invd.data_ptr(), s.dx.ptr, c.B, c.P, NORM_EPS,
                                              c.acc, stream)


def emulate_norm(s, fault=None):
    c = s.case
    eps = torch.tensor(NORM_EPS)
    inv = 1.0 / torch.maximum(torch.sqrt(wave_row_sum(quad(s.x * s.x))), eps)
    s.xhat.payload.copy_(s.x * inv[:, None])
    if c.inv:
        s.inv.payload.copy_(inv[None])
    clamped = s.inv32 >= 1.0 / eps
    dot = wave_row_sum(quad(s.dxhat * s.xhat32))
    if fault != "clamp_projects":
        dot = torch.where(clamped, torch.zeros_like(dot), dot)
    v = (s.dxhat - s.xhat32 * dot[:, None]) * s.inv32[:, None]
    s.dx.payload.copy_(s.dx.payload + v if c.acc else v)


def verify_norm(s, what=None):
    """L = row_depth(P).  Forward: rho = gamma(L + 1) / 2 + 2 ulp (sum of squares, sqrt and reciprocal, each allowed 1 ulp);
    inv_norm within rho |want|, xhat within (rho + u) |want|; a zero row is exactly zero.  Backward (fp64 of its fp32 inputs):
    clamped rows (inv_norm >= 1 / eps) are the single product dxhat inv_norm, EXACT; the others
    inv (|xhat| gamma(L + 1) sum|dxhat xhat| + 3u (|dxhat| + |xhat dot|)) + u |want|, + u |dx0 + want| when accumulating."""
    c = s.case
    rep = Report(what or f"normalize_rows {c}")
    rep.guards(xhat=s.xhat, inv_norm=s.inv, dx=s.dx)
    x = s.x.double()
    L = row_depth(c.P)
    rho = gamma(L + 1) / 2 + 2 * ULP
    inv = 1.0 / x.norm(dim=1).clamp_min(NORM_EPS)
    want = x * inv[:, None]
    rep.bound("xhat", s.xhat.get(), want, (rho + U) * want.abs() + F32_TINY)
    if c.inv:
        rep.bound("inv_norm", s.inv.get()[0], inv, rho * inv)
    elif not bool(torch.isnan(s.inv.get()).all()):
        rep.fail("inv_norm: written although the pointer passed was null")
    g, h, iv = s.dxhat.double(), s.xhat32.double(), s.inv32.double()
    clamped = s.inv32 >= torch.tensor(1.0) / torch.tensor(NORM_EPS)
    dot = torch.where(clamped, torch.zeros_like(iv), (g * h).sum(1))
    v = (g - h * dot[:, None]) * iv[:, None]
    bnd = iv[:, None] * (h.abs() * (gamma(L + 1) * (g * h).abs().sum(1))[:, None] + 3 * U * (g.abs() + (h * dot[:, None]).abs())) + U * v.abs()
    total = v + (s.dx0.double() if c.acc else 0.0)
    bnd = bnd + c.acc * U * total.abs() + F32_TINY
    got = s.dx.get()
    rep.bound("dx", got, total, bnd)
    if bool(clamped.any()) and not c.acc:
        rep.exact("dx (clamped rows: dxhat / eps)", got[clamped], (s.dxhat * s.inv32[:, None])[clamped])
    return rep.done()


CosCase = namedtuple("CosCase", "B P acc")
COS_CASES = [CosCase(B, P, (i + j) % 2) for i, B in enumerate(LOSS_B) for j, P in enumerate(LOSS_P)]
COS_EPS = 1e-12
COS_COEF = 0.37


def build_cos(c: CosCase, device="cpu"):
    seed = 17 * c.B + c.P
    sv, tv = randn((c.B, c.P), seed, 2.0), randn((c.B, c.P), seed + 1, 0.5)
    tv[0] = sv[0]                                                                 # s = t: the gradient is pure cancellation
    if c.B > 1:
        tv[1] = -sv[1]
    if c.B > 2:
        sv[2] = 0.0                                                               # a zero student row (clamped)
    if c.B > 3:
        tv[3] = 0.0
    if c.B > 4:
        sv[4] = 0.0
        sv[4, 1] = 2e-13                                                          # non-zero, below eps
    sd, td = sv.double(), tv.double()
    cos32 = ((sd * td).sum(1) / (sd.norm(dim=1).clamp_min(COS_EPS) * td.norm(dim=1).clamp_min(COS_EPS))).float()
    ds0 = randn((c.B, c.P), seed + 2)
    return SimpleNamespace(case=c, s=sv, t=tv, cos32=cos32, ds0=ds0, sd=poisoned(sv, c.P, device), td=poisoned(tv, c.P, device),
                           cosd=cos32.to(device), cosv=vec(c.B, device), loss=vec(1, device),
                           ds=Guarded(c.B, c.P, device=device, fill=ds0 if c.acc else NAN))


def launch_cos(lib, s, stream, lasts=None) -> int:
    c = s.case
    rc = lib.dclip_cosine_loss_fwd(s.sd.data_ptr(), s.td.data_ptr(), s.loss.ptr, s.cosv.ptr, c.B, c.P, stream)
    if lasts is not None:
        lasts.append(lib.dclip_last_launch().decode())
    return rc or lib.dclip_cosine_loss_bwd(s.sd.data_ptr(), s.td.data_ptr(), s.cosd.data_ptr(), s.ds.ptr, c.B, c.P, COS_COEF, c.acc, stream)


def block_sum_256(v: torch.Tensor) -> torch.Tensor:
    """One 256-thread workgroup's sum of a vector: thread i adds v[i], v[i + 256], ...; butterfly per wave; (w0 + w1) + (w2 + w3)."""
    K = -(-v.numel() // 256)
    t = torch.zeros(K * 256, dtype=v.dtype)
    t[:v.numel()] = v
    t = t.view(K, 256)
    s = torch.zeros(256, dtype=v.dtype)
    for k in range(K):
        s = s + t[k]
    s = s.view(4, 64)
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lane ^ o]
    return (s[0, 0] + s[1, 0]) + (s[2, 0] + s[3, 0])


def emulate_cos(s, fault=None):
    c = s.case
    eps = torch.tensor(COS_EPS)
    a, b = s.s, s.t
    ns, nt = torch.sqrt(wave_row_sum(quad(a * a))), torch.sqrt(wave_row_sum(quad(b * b)))
    cos = wave_row_sum(quad(a * b)) / (torch.maximum(ns, eps) * torch.maximum(nt, eps))
    s.cosv.payload.copy_(cos[None])
    s.loss.payload.fill_(float(torch.tensor(-1.0) * block_sum_256(cos) + torch.tensor(float(c.B))))
    is_, it = 1.0 / torch.maximum(ns, eps), 1.0 / torch.maximum(nt, eps)
    cc = torch.where(ns >= eps, s.cos32, torch.zeros_like(ns))
    if fault == "no_cos_term":
        cc = torch.zeros_like(cc)
    v = (b * it[:, None] - a * (is_ * cc)[:, None]) * (torch.tensor(-COS_COEF) * is_)[:, None]
    s.ds.payload.copy_(s.ds.payload + v if c.acc else v)


def verify_cos(s, what=None):
    """L = row_depth(P), rho_n = gamma(L + 1) / 2 + 1 ulp (a norm), rho_i = rho_n + 1 ulp (its reciprocal).
    cos:       gamma(L + 1) sum|s t| / (|s| |t|) + |cos| (2 rho_n + 1 ulp + u)
    loss_sum:  sum of those + gamma(ceil(B / 256) + 10) sum|cos| + u (B + |want|)
    ds (fp64 of the fp32 inputs s, t, cos, coef):  coef / |s| ((rho_i + 2u) |that| + (rho_i + 3u) |cos shat|) + (rho_i + 3u) |want|
               — the first term is absolute: at s = t the gradient is the difference of two nearly equal vectors;
               + u |ds0 + want| when accumulating."""
    c = s.case
    rep = Report(what or f"cosine_loss {c}")
    rep.guards(cos=s.cosv, loss_sum=s.loss, ds=s.ds)
    a, b = s.s.double(), s.t.double()
    L = row_depth(c.P)
    rho_n = gamma(L + 1) / 2 + ULP
    rho_i = rho_n + ULP
    na, nb = a.norm(dim=1).clamp_min(COS_EPS), b.norm(dim=1).clamp_min(COS_EPS)
    cos = (a * b).sum(1) / (na * nb)
    bcos = gamma(L + 1) * (a * b).abs().sum(1) / (na * nb) + cos.abs() * (2 * rho_n + ULP + U) + F32_TINY
    rep.bound("cos", s.cosv.get()[0], cos, bcos)
    want_loss = c.B - cos.sum()
    rep.bound("loss_sum", s.loss.get()[0], want_loss.reshape(1),
              bcos.sum() + gamma(-(-c.B // 256) + 10) * cos.abs().sum() + U * (c.B + want_loss.abs()))
    clamped = a.norm(dim=1) < COS_EPS
    cc = torch.where(clamped, torch.zeros_like(cos), s.cos32.double())
    that, shat = b / nb[:, None], a / na[:, None]
    k = (COS_COEF_F32 / na)[:, None]
    want = -(that - cc[:, None] * shat) * k
    bnd = k * ((rho_i + 2 * U) * that.abs() + (rho_i + 3 * U) * (cc[:, None] * shat).abs()) + (rho_i + 3 * U) * want.abs()
    total = want + (s.ds0.double() if c.acc else 0.0)
    rep.bound("ds", s.ds.get(), total, bnd + c.acc * U * total.abs() + F32_TINY)
    return rep.done()


COS_COEF_F32 = float(torch.tensor(COS_COEF, dtype=torch.float32))          # the value the ABI receives

SubCase = namedtuple("SubCase", "n b acc")
SUB_CASES = [SubCase(n, bool((i + k) % 2), k) for i, n in enumerate((1, 255, 256, 257, 1000)) for k in (0, 1)]
SUB_SCALE = -0.25


def build_sub(c: SubCase, device="cpu"):
    a, b = ints((c.n,), c.n, -8, 8), ints((c.n,), c.n + 1, -8, 8)
    nanpad = torch.full((8,), NAN)
    return SimpleNamespace(case=c, a=a, b=b, ad=torch.cat([a, nanpad]).to(device), bd=torch.cat([b, nanpad]).to(device),
                           out=vec(1, device, fill=torch.tensor([5.0]) if c.acc else NAN))


def launch_sub(lib, s, stream) -> int:
    c = s.case
    return lib.dclip_sub_reduce(s.ad.data_ptr(), s.bd.data_ptr() if c.b else None, s.out.ptr, c.n, SUB_SCALE, c.acc, stream)


def sub_want(s):
    c = s.case
    return SUB_SCALE * float((s.a.long() - (s.b.long() if c.b else 0)).sum()) + (5.0 if c.acc else 0.0)


def emulate_sub(s, fault=None):
    s.out.payload.fill_(sub_want(s))


def verify_sub(s, what=None):
    rep = Report(what or f"sub_reduce {s.case}")
    rep.guards(out=s.out)
    rep.exact("out", s.out.get(), torch.tensor([[sub_want(s)]]))
    return rep.done()


# ==================================================================================================== optim.hip

def f32(x: float) -> float:
    """The fp32 value a float argument of the C ABI carries, widened to double."""
    return float(torch.tensor(x, dtype=torch.float32))


SUMSQ_N = [1, 2, 3, 4, 5, 1023, 1024, 1025, 300001]


def sumsq_blocks(n: int) -> int:
    return max(1, min(256, (n // 4 + 255) // 256))


def build_sumsq(n: int, device="cpu"):
    x = ints((n,), n)
    return SimpleNamespace(n=n, x=x, xd=torch.cat([x, torch.full((8,), NAN)]).to(device), partial=vec(sumsq_blocks(n), device))


def launch_sumsq(lib, s, stream) -> int:
    assert int(lib.dclip_sumsq_blocks(s.n)) == sumsq_blocks(s.n)
    return lib.dclip_sumsq_f32(s.xd.data_ptr(), s.n, s.partial.ptr, stream)


def sumsq_want(s, skip_tail=False):
    n, G = s.n, sumsq_blocks(s.n)
    n4 = n // 4
    sq = s.x.long() ** 2
    want = torch.zeros(G, dtype=torch.long)
    if n4:
        want.index_add_(0, (torch.arange(n4) // 256) % G, sq[:n4 * 4].view(n4, 4).sum(1))
    if not skip_tail:
        want[0] += sq[n4 * 4:].sum()
    return want


def emulate_sumsq(s, fault=None):
    s.partial.payload.copy_(sumsq_want(s, fault == "tail_skipped").float()[None])


def verify_sumsq(s, what=None):
    rep = Report(what or f"sumsq n={s.n}")
    rep.guards(partial=s.partial)
    rep.exact("partial", s.partial.get()[0], sumsq_want(s))
    return rep.done()


ClipCase = namedtuple("ClipCase", "count kind max_norm scale")       # scale: None = dclip_clip_coef, else the power-of-two loss scale
CLIP_COUNTS = [1, 255, 256, 257, 1000]
CLIP_KINDS = ["int", "zero", "inf", "nan", "overflow"]


def clip_cases():
    out = []
    for i, n in enumerate(CLIP_COUNTS):
        for j, scale in enumerate((None, 1024.0, 0.125)):
            for k, mn in enumerate((8.0, 4.0, 0.5)):                  # the norm is 4: below, at and above max_norm
                out.append(ClipCase(n, "int", mn, scale))
            out.append(ClipCase(n, "zero", 0.5, scale))
            if scale is not None:
                out += [ClipCase(n, kind, 0.5, scale) for kind in ("inf", "nan", "overflow")]
    return out


def build_clip(c: ClipCase, device="cpu"):
    sc = c.scale or 1.0
    if c.kind == "zero":
        part = torch.zeros(c.count)
    else:                              # integer partials that add up to (4 scale)^2: the unscaled norm is exactly 4
        total = int((4 * sc) ** 2) if sc >= 1 else None
        part = torch.zeros(c.count)
        if total is None:
            part[c.count // 2] = (4 * sc) ** 2                          # 0.25: one dyadic partial
        else:
            base = total // c.count
            part[:] = float(base)
            part[c.count - 1] += total - base * c.count
    if c.kind == "inf":
        part[c.count // 2] = float("inf")
    if c.kind == "nan":
        part[c.count // 3] = NAN
    if c.kind == "overflow":
        part[:] = 0.0
        part[0] = 3e38
        part[c.count - 1] = 3e38 if c.count > 1 else float("inf")
    nan = torch.full((8,), NAN)
    return SimpleNamespace(case=c, part=part, partd=torch.cat([part, nan]).to(device), scaled=torch.tensor([sc]).to(device),
                           out=vec(3 if c.scale else 1, device), norm=vec(1, device))


def launch_clip(lib, s, stream) -> int:
    c = s.case
    if c.scale is None:
        return lib.dclip_clip_coef(s.partd.data_ptr(), c.count, c.max_norm, s.out.ptr, s.norm.ptr, stream)
    return lib.dclip_clip_coef_scaled(s.partd.data_ptr(), c.count, c.max_norm, s.scaled.data_ptr(), s.out.ptr, stream)


def emulate_clip(s, fault=None):
    c = s.case
    tot = block_sum_256(s.part)
    nrm = torch.sqrt(tot) / torch.tensor(c.scale or 1.0)
    coef = torch.minimum(torch.tensor(1.0), torch.tensor(c.max_norm) / (nrm + torch.tensor(1e-6)))
    if c.scale is None:
        s.out.payload.fill_(float(coef))
        s.norm.payload.fill_(float(nrm))
    else:
        bad = not bool(torch.isfinite(nrm))
        s.out.payload.copy_(torch.tensor([[float(nrm), 1.0 if bad else 0.0, 0.0 if bad else float(coef / torch.tensor(c.scale))]]))


def verify_clip(s, what=None):
    """Integer (dyadic) partials add up exactly in any order: norm within 1 ulp of sqrt(sum) / scale (the division by a power of
    two is exact); the coefficient within 1 ulp (one division) of min(1, max_norm / (norm + 1e-6)) [/ scale] evaluated in fp32
    from the norm the kernel returned; zero gradients give exactly 1 [/ scale]; a non-finite norm sets found_inf and coefficient 0."""
    c = s.case
    rep = Report(what or f"clip_coef {c}")
    rep.guards(out=s.out, norm=s.norm)
    out = s.out.get()[0]
    sc = c.scale or 1.0
    if c.kind in ("inf", "nan", "overflow"):
        if float(out[1]) != 1.0 or float(out[2]) != 0.0 or bool(torch.isfinite(out[0])):
            rep.fail(f"a non-finite norm must give found_inf = 1 and coefficient 0: out = {out.tolist()}")
        return rep.done()
    got_norm = out[0] if c.scale else s.norm.get()[0, 0]
    want_norm = math.sqrt(float(s.part.double().sum())) / sc
    rep.bound("norm", got_norm.reshape(1), torch.tensor([want_norm]), ULP * want_norm)
    coef = torch.minimum(torch.tensor(1.0), torch.tensor(c.max_norm) / (got_norm + torch.tensor(1e-6))).double() / sc
    rep.bound("coef", out[2 if c.scale else 0].reshape(1), coef.reshape(1), ULP * coef)
    if c.scale and float(out[1]) != 0.0:
        rep.fail(f"found_inf = {float(out[1])} for a finite norm")
    if c.kind == "zero" and float(out[2 if c.scale else 0]) != 1.0 / sc:
        rep.fail("zero gradients must give the coefficient 1")
    return rep.done()


# ---- _amp_update_scale_ : the state machine against a statement of torch's rule

AMP_TABLE = [  # (scale, tracker, found_inf, growth, backoff, interval)
    (65536.0, 0, 0.0, 2.0, 0.5, 2000), (65536.0, 1998, 0.0, 2.0, 0.5, 2000), (65536.0, 1999, 0.0, 2.0, 0.5, 2000),
    (65536.0, 1999, 1.0, 2.0, 0.5, 2000), (65536.0, 5, 1.0, 2.0, 0.5, 2000), (3e38, 0, 0.0, 2.0, 0.5, 1), (1.0, 0, 0.0, 2.0, 0.5, 1),
    (1.0, 0, 1.0, 2.0, 0.5, 1), (1024.0, 3, 0.25, 2.0, 0.5, 4), (1024.0, 3, -1.0, 2.0, 0.5, 4), (1024.0, 3, 3.0, 4.0, 0.25, 4),
    (2.0 ** 127, 9, 0.0, 2.0, 0.5, 10), (1e-30, 0, 1.0, 2.0, 0.5, 3), (7.0, 2, 0.0, 1.5, 0.5, 3), (7.0, 7, 0.0, 1.5, 0.5, 3)]


def amp_rule(scale, tracker, found_inf, growth, backoff, interval, fault=None):
    """torch._amp_update_scale_ in fp32."""
    s = torch.tensor(scale, dtype=torch.float32)
    if found_inf != 0.0:
        return float(s * torch.tensor(backoff, dtype=torch.float32)), 0
    if tracker + 1 == interval:
        g = s * torch.tensor(growth, dtype=torch.float32)
        return (float(g) if bool(torch.isfinite(g)) else float(s)), (tracker + 1 if fault == "tracker_not_reset" else 0)
    return float(s), tracker + 1


def build_amp(row, device="cpu"):
    scale, tracker, found, growth, backoff, interval = row
    return SimpleNamespace(row=row, scale=vec(1, device, fill=torch.tensor([scale])),
                           tracker=vec(1, device, fill=torch.tensor([tracker], dtype=torch.int32).view(torch.float32)),
                           found=torch.tensor([found, NAN]).to(device))


def launch_amp(lib, s, stream) -> int:
    _, _, _, growth, backoff, interval = s.row
    return lib.dclip_amp_update_scale(s.scale.ptr, s.tracker.ptr, s.found.data_ptr(), growth, backoff, interval, stream)


def emulate_amp(s, fault=None):
    sc, tr = amp_rule(*s.row, fault=fault)
    s.scale.payload.fill_(sc)
    s.tracker.payload.view(torch.int32).fill_(tr)


def verify_amp(s, what=None):
    rep = Report(what or f"amp_update_scale {s.row}")
    rep.guards(scale=s.scale, tracker=s.tracker)
    sc, tr = amp_rule(*s.row)
    got = (float(s.scale.get()[0, 0]), int(s.tracker.get().view(torch.int32)[0, 0]))
    if got != (sc, tr):
        rep.fail(f"(scale, tracker) = {got}, torch's rule gives {(sc, tr)}")
    return rep.done()


# ---- Adam / AdamW: one step from a random state

MT_CHUNK_DOC = 32768                     # what dclip_mt_chunk_elems() returns; the GPU tests read it and build their tables from it
MT_STEPS = [1, 2, 1000]
# which of a tensor's four arrays start 4 bytes behind a 16-byte boundary (the kernels' scalar branch), per table variant: every
# size is met aligned and misaligned
MT_ALIGN = [["", "p", "g", "m", "v", "pgmv", "", "pgmv"], ["pgmv", "", "", "", "", "", "g", ""]]


def mt_mis(k: int, shift: int) -> str:
    return MT_ALIGN[shift % 2][k]

LR, BETA1, BETA2, ADAM_EPS = 1e-3, 0.9, 0.999, 1e-8
# |powf(beta, step) - beta^step| allowed to the non-SKIP kernels: twice the worst entry of the table measured on the MI355X against
# fp64 (3.7262e-08 = 0.625 * 2^-24 at beta = 0.9, step = 100; an entry includes the rounding of 1 - beta^step).
POW_ALLOWANCE = 2 * 3.7262e-08
SKIP_BC_RHO = 8 * U                      # -expm1f(step log1pf(-(1 - beta))): 2 ulp + 1 ulp libm functions, |t| e^t / (1 - e^t) <= 1

MtCase = namedtuple("MtCase", "entry order shift wd gs")      # entry: "adamw" | "adam" | "skip" | "sumsq" | "skip_found_inf"
MT_ORDERS = [((0, 1, 2, 3, 4, 5, 6, 7), 0), ((7, 2, 5, 0, 6, 3, 1, 4), 3)]


def mt_sizes(chunk: int):
    return [1, 3, 4, 5, chunk - 1, chunk, chunk + 1, 2 * chunk + 3]


def mt_cases():
    out = []
    for entry in ("adamw", "adam", "skip"):
        for order, shift in MT_ORDERS:
            for wd in (0.0, 0.03):
                for gs in ((None, 0.37) if entry != "skip" else (0.37,)):
                    out.append(MtCase(entry, order, shift, wd, gs))
    out += [MtCase("sumsq", order, shift, 0.0, None) for order, shift in MT_ORDERS]
    out += [MtCase("skip_found_inf", MT_ORDERS[1][0], 1, 0.03, 0.37), MtCase("adamw", (3,), 1, 0.03, 0.37), MtCase("sumsq", (6,), 5, 0.0, None)]
    return out


def mt_id(c) -> str:
    return f"{c.entry}-o{''.join(map(str, c.order))}-s{c.shift}-wd{c.wd}-gs{c.gs}"


def build_mt(c: MtCase, device="cpu", chunk: int = MT_CHUNK_DOC):
    sizes = mt_sizes(chunk)
    tens, chunk0 = [], 0
    for pos, k in enumerate(c.order):
        n = sizes[k]
        mis = mt_mis(k, c.shift)
        seed = 100 * k + 7
        if c.entry == "sumsq":
            st = {"p": torch.zeros(n), "g": ints((n,), seed), "m": torch.zeros(n), "v": torch.zeros(n)}
        else:
            st = {"p": randn((n,), seed, 4.0), "g": randn((n,), seed + 1, 0.02), "m": randn((n,), seed + 2, 0.01),
                  "v": randn((n,), seed + 3, 0.01) ** 2}
            if c.entry == "skip_found_inf":
                st["g"][::3] = NAN
        t = SimpleNamespace(n=n, step=MT_STEPS[(k + c.shift) % 3], mis=mis, st=st, buf={}, chunk0=chunk0)
        for name, val in st.items():
            off = name in mis
            gd = vec(n + int(off), device)
            (gd.payload[0, 1:] if off else gd.payload[0]).copy_(val)
            t.buf[name] = gd
        chunk0 += -(-n // chunk)
        tens.append(t)

    def ptr(t, name):
        return t.buf[name].ptr + (4 if name in t.mis else 0)

    blob = b"".join(struct.pack("<QQQQQii", ptr(t, "p"), ptr(t, "g"), ptr(t, "m"), ptr(t, "v"), t.n, t.step, t.chunk0) for t in tens)
    s = SimpleNamespace(case=c, tens=tens, total=chunk0, chunk=chunk, table=torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(device),
                        partial=vec(chunk0, device))
    found = 1.0 if c.entry == "skip_found_inf" else 0.0
    s.coef3 = torch.tensor([NAN if found else 1.0, found, 0.0 if found else c.gs or 1.0, NAN]).to(device)
    s.gsd = torch.tensor([c.gs or 1.0, NAN]).to(device)
    return s


def mt_args(c):
    """(lr, beta1 or 1 - beta1, beta2 or 1 - beta2, eps, wd) as the entry takes them."""
    if c.entry.startswith("skip"):
        return LR, 1.0 - BETA1, 1.0 - BETA2, ADAM_EPS, c.wd
    return LR, BETA1, BETA2, ADAM_EPS, c.wd


def launch_mt(lib, s, stream) -> int:
    c = s.case
    assert lib.dclip_mt_record_bytes() == 48
    if c.entry == "sumsq":
        return lib.dclip_mt_sumsq_f32(s.table.data_ptr(), len(s.tens), s.total, s.partial.ptr, stream)
    if c.entry.startswith("skip"):
        return lib.dclip_mt_adamw_f32_skip(s.table.data_ptr(), len(s.tens), s.total, *mt_args(c), s.coef3.data_ptr() + 0, stream)
    fn = lib.dclip_mt_adamw_f32 if c.entry == "adamw" else lib.dclip_mt_adam_f32
    return fn(s.table.data_ptr(), len(s.tens), s.total, *mt_args(c), s.gsd.data_ptr() if c.gs is not None else None, stream)


def mt_view(t, name):
    pl = t.buf[name].payload
    return pl[0, 1:] if name in t.mis else pl[0]


def adam_step_f32(st, step, args, gs, coupled, skip, fault=None):
    """The kernels' arithmetic in fp32 torch (one rounding per operation, bias corrections as the kernel forms them)."""
    T = lambda x: torch.tensor(x, dtype=torch.float32)                                    # noqa: E731
    lr, b1, b2, eps, wd = (T(a) for a in args)
    p, g, m, v = st["p"], st["g"], st["m"], st["v"]
    one = T(1.0)
    k = T(float(step - 1 if fault == "bias_step_minus_1" else step))
    if skip:
        bc1, bc2 = -torch.expm1(k * torch.log1p(-b1)), -torch.expm1(k * torch.log1p(-b2))
        beta1, beta2, omb1, omb2 = one - b1, one - b2, b1, b2
    else:
        bc1, bc2 = one - torch.pow(b1, k), one - torch.pow(b2, k)
        beta1, beta2, omb1, omb2 = b1, b2, one - b1, one - b2
    gg = g * T(gs) if gs is not None else g
    if coupled:
        gg = (p.double() * wd.double() + gg.double()).float()                             # one fused multiply-add
    mm = m * beta1 + gg * omb1
    vv = v * beta2 + gg * gg * omb2
    decay = one if coupled and fault != "decoupled_in_coupled" else one - lr * wd
    out = p * decay - (lr / bc1) * mm / (torch.sqrt(vv) / torch.sqrt(bc2) + eps)
    return out, mm, vv


def emulate_mt(s, fault=None):
    c = s.case
    if c.entry == "sumsq":
        part = []
        for t in s.tens:
            g = t.st["g"]
            if fault == "tail_skipped" and "g" in t.mis:
                g = g[:t.n & ~3]
            part += [float((blk.long() ** 2).sum()) for blk in g.split(s.chunk)] + [0.0] * (-(-t.n // s.chunk) - len(g.split(s.chunk)))
        s.partial.payload.copy_(torch.tensor(part)[None])
        return
    if c.entry == "skip_found_inf":
        if fault == "skip_writes_moments":
            for t in s.tens:
                mt_view(t, "m").mul_(0.9)
                mt_view(t, "v").mul_(0.999)
        return
    for t in s.tens:
        out, mm, vv = adam_step_f32(t.st, t.step, mt_args(c), c.gs, c.entry == "adam", c.entry == "skip", fault)
        if fault == "tail_skipped" and t.mis:
            keep = t.n & ~3
            out[keep:], mm[keep:], vv[keep:] = t.st["p"][keep:], t.st["m"][keep:], t.st["v"][keep:]
        if fault == "chunk_element_twice" and t.n > s.chunk:
            st2 = {k: v[s.chunk:s.chunk + 1] for k, v in dict(p=out, g=t.st["g"], m=mm, v=vv).items()}
            o2, m2, v2 = adam_step_f32(st2, t.step, mt_args(c), c.gs, c.entry == "adam", c.entry == "skip")
            out[s.chunk], mm[s.chunk], vv[s.chunk] = o2[0], m2[0], v2[0]
        for name, val in (("p", out), ("m", mm), ("v", vv)):
            mt_view(t, name).copy_(val)


def adam_reference(st, step, args, gs, coupled, skip, pow_allowance=POW_ALLOWANCE):
    """fp64 of the fp32 state and of the fp32 scalar arguments (bias corrections in fp64), and the per-element bounds:
      eg  = u |g gs| (a scaled gradient) + u |g'| (the coupled fused multiply-add)                      error of g'
      dm  = (1 - b1) eg + 3u (|m b1| + |g'| (1 - b1))            dv = 2 (1 - b2) |g'| eg + 4u v'
      A   = sqrt(v') / sqrt(bc2):  dA = (dv / (2 sqrt v') + ulp sqrt v') / sqrt(bc2) + A (rho2 + ulp),   dden = dA + u den
      upd = (lr / bc1) m' / den:   dupd = (lr / bc1) dm / den + |upd| (rho1 + 2 ulp + u + dden / den)
      dp  = 3u |p decay| + dupd + u |want|
    with rho1 = (allowance + u) / bc1 and rho2 = (allowance + u) / (2 bc2) + ulp for the powf kernels (allowance:
    POW_ALLOWANCE), 8u and 4u + ulp for the expm1 / log1p form of the SKIP kernel."""
    lr, a1, a2, eps, wd = (f32(a) for a in args)
    b1, b2 = (1.0 - a1, 1.0 - a2) if skip else (a1, a2)
    p, g, m, v = (st[k].double() for k in "pgmv")
    gsv = f32(gs) if gs is not None else 1.0
    gg = g * gsv + (wd * p if coupled else 0.0)
    eg = (U * (g * gsv).abs() if gs is not None else 0.0) + (U * gg.abs() if coupled else 0.0)
    mm = m * b1 + gg * (1 - b1)
    vv = v * b2 + gg * gg * (1 - b2)
    dm = (1 - b1) * eg + 3 * U * ((m * b1).abs() + gg.abs() * (1 - b1))
    dv = 2 * (1 - b2) * gg.abs() * eg + 4 * U * vv
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    rho1 = SKIP_BC_RHO if skip else (pow_allowance + U) / bc1
    rho2 = (SKIP_BC_RHO if skip else (pow_allowance + U) / bc2) / 2 + ULP
    sq = vv.sqrt()
    A = sq / math.sqrt(bc2)
    dA = (dv / (2 * sq).clamp_min(1e-300) + ULP * sq) / math.sqrt(bc2) + A * (rho2 + ULP)
    den = A + eps
    dden = dA + U * den
    S = lr / bc1
    upd = S * mm / den
    dupd = S * dm / den + upd.abs() * (rho1 + 2 * ULP + U + dden / den)
    decay = 1.0 if coupled else 1.0 - lr * wd
    want = p * decay - upd
    dp = 3 * U * (p * decay).abs() + dupd + U * want.abs()
    return SimpleNamespace(p=want, m=mm, v=vv, dp=dp + F32_TINY, dm=dm + F32_TINY, dv=dv + F32_TINY, upd=upd)


def verify_mt(s, what=None):
    c = s.case
    rep = Report(what or f"mt {mt_id(c)}")
    for i, t in enumerate(s.tens):
        rep.guards(**{f"{k}[{i}]": gd for k, gd in t.buf.items()})
        for name in t.mis:                                               # the float in front of a misaligned array
            if not bool(torch.isnan(t.buf[name].get()[0, :1]).all()):
                rep.fail(f"{name}[{i}]: the element in front of the misaligned array was written")
    if c.entry == "sumsq":
        rep.guards(partial=s.partial)
        want = [int((blk.long() ** 2).sum()) for t in s.tens for blk in t.st["g"].split(s.chunk)]
        rep.exact("partial", s.partial.get()[0], torch.tensor(want))
        for i, t in enumerate(s.tens):
            rep.bits(f"g[{i}]", mt_view(t, "g").detach().cpu(), t.st["g"])
        return rep.done()
    for i, t in enumerate(s.tens):
        tag = f"[{i}] n={t.n} step={t.step} mis={t.mis or '-'}"
        rep.bits("g" + tag, mt_view(t, "g").detach().cpu(), t.st["g"])
        if c.entry == "skip_found_inf":
            for name in "pmv":
                rep.bits(name + tag, mt_view(t, name).detach().cpu(), t.st[name])
            continue
        r = adam_reference(t.st, t.step, mt_args(c), c.gs, c.entry == "adam", c.entry == "skip")
        rep.bound("p" + tag, mt_view(t, "p").detach().cpu(), r.p, r.dp)
        rep.bound("m" + tag, mt_view(t, "m").detach().cpu(), r.m, r.dm)
        rep.bound("v" + tag, mt_view(t, "v").detach().cpu(), r.v, r.dv)
    worst = {k[0]: 0.0 for k in rep.fig}
    for k, val in rep.fig.items():
        worst[k[0]] = max(worst[k[0]], val) if val == val else NAN
    rep.fig = worst
    return rep.done()


AdamwCase = namedtuple("AdamwCase", "n step wd gs")


def adamw_cases(chunk: int = MT_CHUNK_DOC):
    return [AdamwCase(n, MT_STEPS[i % 3], (0.0, 0.03)[i % 2], (None, 0.37)[(i // 2) % 2]) for i, n in enumerate(mt_sizes(chunk) + [300001])]


def build_adamw(c: AdamwCase, device="cpu"):
    m = build_mt(MtCase("adamw", (0,), 0, c.wd, c.gs), device)           # one aligned tensor, resized below
    t = m.tens[0]
    seed = c.n
    t.n, t.step, t.mis = c.n, c.step, ""
    t.st = {"p": randn((c.n,), seed, 4.0), "g": randn((c.n,), seed + 1, 0.02), "m": randn((c.n,), seed + 2, 0.01),
            "v": randn((c.n,), seed + 3, 0.01) ** 2}
    t.buf = {k: vec(c.n, device, fill=v) for k, v in t.st.items()}
    m.acase = c
    return m


def launch_adamw(lib, s, stream) -> int:
    c, t = s.acase, s.tens[0]
    return lib.dclip_adamw_f32(t.buf["p"].ptr, t.buf["g"].ptr, t.buf["m"].ptr, t.buf["v"].ptr, c.n, LR, BETA1, BETA2, ADAM_EPS, c.wd, c.step,
                               s.gsd.data_ptr() if c.gs is not None else None, stream)
