"""The four stand-alone erf-GELU entries (dclip_amd/csrc/activation.hip) through the C ABI, one launch per case:
every length at which the kernels take another path (below one vector, the scalar tail, one block, one sweep of the capped grid
+- 1, more than two sweeps), in place and into guarded buffers, on inputs that include +-0, subnormals, +-14, the neighbourhood of
0 and the worst point of torch's own forward; dclip_last_launch() is asserted after each call.  Gates, references and checkers:
tests/kernel_checks_gelu.py (tests/test_kernel_checks_gelu_cpu.py shows what they catch).  Refused calls are refused on the host:
they return an error, launch nothing and touch nothing.  One case runs the bf16 entry in place at 2^32 + 2051 elements."""
import threading

import pytest
import torch

from tests import kernel_checks_gelu as kg

pytestmark = pytest.mark.gpu

BLOCK, MAX_BLOCKS = 256, 2048                                # activation.hip: GELU_BLOCK, GELU_MAX_BLOCKS
SWEEP = {4: MAX_BLOCKS * BLOCK * 4, 2: MAX_BLOCKS * BLOCK * 8}      # elements one sweep of the capped grid covers, by element size
GUARD = 64                                                   # elements either side of a guarded output (a multiple of 16 bytes)
TYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def lengths(elem_bytes):
    s = SWEEP[elem_bytes]
    return [1, 3, 4, 5, 7, 8, 9, 255, 1024 + 1, s - 1, s, s + 1, 2 * s + s // 3 + 5]


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


def launched(lib, rc, site):
    assert rc == 0, f"{site}: rc={rc}: {lib.dclip_last_error().decode(errors='replace')}"
    got = lib.dclip_last_launch().decode()
    torch.cuda.synchronize()
    assert got == site, (got, site)


@pytest.fixture(scope="module")
def pool32():
    """The edge inputs, then 4099 samples of 3 N(0,1): 4127 values, a length no vector width divides, repeated over each case."""
    gen = torch.Generator().manual_seed(34)
    return torch.cat([kg.edge_inputs32(), torch.randn(4099, generator=gen) * 3.0])


def pool16(dtype):
    """Every finite value of the type, in an order that mixes magnitudes and signs (65,280 / 63,488 values)."""
    x = kg.all_finite16(dtype)
    return x[torch.randperm(x.numel(), generator=torch.Generator().manual_seed(16))]


def repeat(pool, n, shift=0):
    idx = (torch.arange(n) + shift) % pool.numel()
    return pool[idx]


class Guarded:
    """n elements inside a NaN-filled buffer with GUARD elements either side; .t is the 16-byte aligned middle."""

    def __init__(self, n, dtype, dev):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device=dev)
        self.t = self.buf[GUARD:GUARD + n]
        assert self.t.data_ptr() % 16 == 0

    def intact(self):
        return bool(torch.isnan(self.buf[:GUARD]).all()) and bool(torch.isnan(self.buf[GUARD + self.n:]).all())


# ---------------------------------------------------------------------------------------------------- fp32 forward and backward

@pytest.mark.parametrize("n", lengths(4))
def test_gelu_erf_f32(dev, lib, pool32, n):
    h_host = repeat(pool32, n, shift=n % 7)
    h = Guarded(n, torch.float32, dev)
    h.t.copy_(h_host)
    g = Guarded(n, torch.float32, dev)
    launched(lib, lib.dclip_gelu_erf_f32(h.t.data_ptr(), g.t.data_ptr(), n, stream()), "gelu_erf_f32")
    assert g.intact() and h.intact(), "a guard region was written"
    assert torch.equal(h.t.cpu().view(torch.int32), h_host.view(torch.int32)), "out of place: the input changed"
    out = g.t.cpu()
    kg.check_fwd32(out, h_host, f"gelu_erf_f32 n={n}")
    launched(lib, lib.dclip_gelu_erf_f32(h.t.data_ptr(), h.t.data_ptr(), n, stream()), "gelu_erf_f32")      # g = h
    assert h.intact(), "in place: a guard region was written"
    assert torch.equal(h.t.cpu().view(torch.int32), out.view(torch.int32)), "in place differs from out of place"


@pytest.mark.parametrize("n", lengths(4))
def test_gelu_erf_bwd_f32(dev, lib, pool32, n):
    h_host = repeat(pool32, n, shift=n % 5)
    dg_host = repeat(torch.randn(4111, generator=torch.Generator().manual_seed(n % 1000)) * 2.0, n)
    h, dg, dh = Guarded(n, torch.float32, dev), Guarded(n, torch.float32, dev), Guarded(n, torch.float32, dev)
    h.t.copy_(h_host), dg.t.copy_(dg_host)
    launched(lib, lib.dclip_gelu_erf_bwd_f32(h.t.data_ptr(), dg.t.data_ptr(), dh.t.data_ptr(), n, stream()), "gelu_erf_bwd_f32")
    assert h.intact() and dg.intact() and dh.intact(), "a guard region was written"
    assert torch.equal(h.t.cpu().view(torch.int32), h_host.view(torch.int32)) and \
        torch.equal(dg.t.cpu().view(torch.int32), dg_host.view(torch.int32)), "out of place: an input changed"
    out = dh.t.cpu()
    kg.check_bwd32(out, h_host, dg_host, f"gelu_erf_bwd_f32 n={n}")
    launched(lib, lib.dclip_gelu_erf_bwd_f32(h.t.data_ptr(), dg.t.data_ptr(), dg.t.data_ptr(), n, stream()), "gelu_erf_bwd_f32")   # dh = dg
    assert dg.intact(), "in place: a guard region was written"
    assert torch.equal(dg.t.cpu().view(torch.int32), out.view(torch.int32)), "in place differs from out of place"


def test_fp32_worst_errors_on_the_measured_input_set(dev, lib):
    """The figures DESIGN.md §34 quotes beside torch's 6.07 / 4.87: the kernels over the 8.4 million inputs the gate was measured on."""
    h_host = kg.inputs32()
    n = h_host.numel()
    h, g = h_host.to(dev), torch.empty(n, dtype=torch.float32, device=dev)
    launched(lib, lib.dclip_gelu_erf_f32(h.data_ptr(), g.data_ptr(), n, stream()), "gelu_erf_f32")
    kg.check_fwd32(g.cpu(), h_host, "gelu_erf_f32 on inputs32")
    ones = torch.ones(n, dtype=torch.float32, device=dev)
    launched(lib, lib.dclip_gelu_erf_bwd_f32(h.data_ptr(), ones.data_ptr(), g.data_ptr(), n, stream()), "gelu_erf_bwd_f32")
    kg.check_bwd32(g.cpu(), h_host, torch.ones(n), "gelu_erf_bwd_f32 on inputs32, dg = 1")


# ---------------------------------------------------------------------------------------------------- 16-bit

@pytest.mark.parametrize("ty", ["bf16", "f16"])
@pytest.mark.parametrize("n", lengths(2))
def test_gelu_erf_16(dev, lib, ty, n):
    dtype, fn, site = TYPES[ty], getattr(lib, "dclip_gelu_erf_" + ty), "gelu_erf_" + ty
    h_host = repeat(pool16(dtype), n, shift=n % 11)
    h = Guarded(n, dtype, dev)
    h.t.copy_(h_host)
    g = Guarded(n, dtype, dev)
    launched(lib, fn(h.t.data_ptr(), g.t.data_ptr(), n, stream()), site)
    assert g.intact() and h.intact(), "a guard region was written"
    assert torch.equal(h.t.cpu().view(torch.int16), h_host.view(torch.int16)), "out of place: the input changed"
    out = g.t.cpu()
    kg.check_faithful16(out, h_host, f"{site} n={n}")
    launched(lib, fn(h.t.data_ptr(), h.t.data_ptr(), n, stream()), site)                                     # g = h
    assert h.intact(), "in place: a guard region was written"
    assert torch.equal(h.t.cpu().view(torch.int16), out.view(torch.int16)), "in place differs from out of place"


@pytest.mark.parametrize("ty", ["bf16", "f16"])
def test_gelu_erf_16_is_the_activation_of_the_stored_value_in_fp32(dev, lib, ty):
    """Every finite input of the type, once: faithful, sign-symmetric where it must be (gelu(+-0) = +-0) and never larger than |h|."""
    dtype, fn = TYPES[ty], getattr(lib, "dclip_gelu_erf_" + ty)
    h_host = kg.all_finite16(dtype)
    h, g = h_host.to(dev), torch.empty(h_host.numel(), dtype=dtype, device=dev)
    launched(lib, fn(h.data_ptr(), g.data_ptr(), h_host.numel(), stream()), "gelu_erf_" + ty)
    out = g.cpu()
    kg.check_faithful16(out, h_host, f"gelu_erf_{ty}, every finite input")
    assert bool((out.float().abs() <= h_host.float().abs()).all())
    z = h_host.float() == 0
    assert torch.equal(out[z].view(torch.int16), h_host[z].view(torch.int16)), "gelu(+-0) = +-0"


# ---------------------------------------------------------------------------------------------------- refused calls

def in_fresh_thread(fn):
    """dclip_last_launch() is per thread: a thread that has launched nothing reports ""."""
    box = {}

    def run():
        try:
            box["v"] = fn()
        except BaseException as e:          # noqa: BLE001 - handed to the caller
            box["e"] = e
    t = threading.Thread(target=run)
    t.start()
    t.join()
    if "e" in box:
        raise box["e"]
    return box["v"]


@pytest.mark.parametrize("ty", ["f32", "bf16", "f16", "bwd_f32"])
def test_refused_calls_launch_nothing(dev, lib, ty):
    dtype = TYPES.get(ty, torch.float32)
    n = 1029
    bufs = [Guarded(n, dtype, dev) for _ in range(3)]
    for i, b in enumerate(bufs):
        b.t.copy_(torch.linspace(-3.0, 3.0, n) + i)
    before = [b.buf.clone() for b in bufs]
    p = [b.t.data_ptr() for b in bufs]
    fn = getattr(lib, "dclip_gelu_erf_" + ty)
    nptr = 3 if ty == "bwd_f32" else 2
    cases = [("n = 0", p[:nptr], 0)]
    for k in range(nptr):
        cases.append((f"null pointer {k}", [None if j == k else p[j] for j in range(nptr)], n))
        cases.append((f"pointer {k} off by 4 bytes", [p[j] + 4 if j == k else p[j] for j in range(nptr)], n - 8))
    st = stream()

    def refused():
        seen = []
        for what, ptrs, cnt in cases:
            rc = fn(*ptrs, cnt, st)
            seen.append((what, rc, lib.dclip_last_launch(), lib.dclip_last_error()))
        return seen
    for what, rc, last, err in in_fresh_thread(refused):
        assert rc == -1, (what, rc)
        assert last == b"", (what, "a refused call launched", last)
        assert b"gelu_erf_" + ty.encode() in err, (what, err)
    torch.cuda.synchronize()
    for b, was in zip(bufs, before):
        assert torch.equal(b.buf.view(torch.int16 if dtype != torch.float32 else torch.int32),
                           was.view(torch.int16 if dtype != torch.float32 else torch.int32)), "a refused call wrote"


# ---------------------------------------------------------------------------------------------------- beyond 2^32 elements

LARGE_N = 2 ** 32 + 2051
LARGE_BYTES = 2 * LARGE_N + (1 << 30)        # the tensor, and 1 GiB for the chunk-wise comparison's temporaries


def test_gelu_erf_bf16_in_place_beyond_2_32_elements(dev, lib):
    """config c5's fc1 output has 4.3e9 elements: a 32-bit element count or offset would stop short of, or wrap inside, this
    tensor.  The input is one period of 65,536 values repeated; the output is compared on the device, chunk by chunk and bit for
    bit, with the entry's own output for one period (checked against fp64 first); the odd tail of 2051 too."""
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < LARGE_BYTES:
        pytest.skip(f"gelu_erf_bf16 at 2^32 + 2051 elements: declared peak {LARGE_BYTES} bytes, {LARGE_BYTES - free} more than the {free} free")
    P = 65536
    fin = pool16(torch.bfloat16)
    period_host = torch.cat([fin, fin[:P - fin.numel()]])
    period = period_host.to(dev)
    ref = torch.empty_like(period)
    launched(lib, lib.dclip_gelu_erf_bf16(period.data_ptr(), ref.data_ptr(), P, stream()), "gelu_erf_bf16")
    kg.check_faithful16(ref.cpu(), period_host, "gelu_erf_bf16, one period")
    x = torch.empty(LARGE_N, dtype=torch.bfloat16, device=dev)
    body = x[:2 ** 32].view(P, P)
    body.copy_(period.expand(P, P))
    x[2 ** 32:].copy_(period[:2051])
    launched(lib, lib.dclip_gelu_erf_bf16(x.data_ptr(), x.data_ptr(), LARGE_N, stream()), "gelu_erf_bf16")
    ref_bits, rows = ref.view(torch.int16), 2048
    bad = torch.zeros((), dtype=torch.int64, device=dev)
    for r0 in range(0, P, rows):
        bad += (body[r0:r0 + rows].view(torch.int16) != ref_bits).sum()
    assert int(bad) == 0, f"{int(bad)} elements of the body differ from the first period's output"
    assert torch.equal(x[2 ** 32:].view(torch.int16), ref_bits[:2051]), "the tail past 2^32 differs"
