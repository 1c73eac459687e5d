"""The 16-bit packed attention core through the C ABI: dclip_attention_varlen_fwd_{bf16,f16} and
dclip_attention_varlen_row_fwd_{bf16,f16}.  Outputs live in guarded buffers, the rows behind every operand are NaN, a refused
call launches nothing and writes nothing.  Exact-selection data per sequence (out == v[pi] bit for bit: a key seen across a
seam or past a mask splits a probability), Gaussian data under the derived per-element bound of tests/kernel_checks.py against
fp64, bit-equality with the padded kernels on equal lengths, and isolation of the sequences inside a pack."""
import pytest
import torch

from tests import kernel_checks as kc
from tests import kernel_checks_varlen16 as kv

pytestmark = pytest.mark.gpu

TYPES = ["bf16", "f16"]
# the wave (32), tile (64) and tower lengths at which masking, the causal tile cut and the sequence seam can go wrong
FULL_CASES = [([1, 2, 17, 31, 32, 33, 63, 64, 65, 128, 129, 5], 2), ([197, 3, 257], 1), ([64], 3)]
CAUSAL_CASES = [([1, 2, 17, 31, 32, 33, 63, 64, 65, 77, 5], 2), ([128, 129, 3], 1), ([64], 3)]
TILED_CASES = [("full", l, h) for l, h in FULL_CASES] + [("causal", l, h) for l, h in CAUSAL_CASES]
ROW_CASES = [([1, 2, 50, 63, 64, 65, 77, 257, 300, 512, 5], 1), ([1, 64, 65], 3)]       # 11 waves: not a multiple of 4


def case_id(v):
    return "-".join(map(str, v)) if isinstance(v, list) else str(v)


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


def check_selection(lib, dev, pack):
    kv.assert_margins(pack)
    out = kv.run_pack(lib, dev, stream(), pack)
    bad = kv.selection_failures(pack, out)
    assert not bad, f"{pack.mode} {pack.tyname} {pack.lengths} H={pack.H}: not v[pi] bit for bit in (sequence, first difference) {bad}"


def check_bound(lib, dev, pack):
    out = kv.run_pack(lib, dev, stream(), pack)
    ratios = [r for r in kv.bound_ratios(pack, out) if r is not None]
    print(f"{pack.mode} {pack.tyname} {pack.lengths} H={pack.H}: worst got / bound {max(ratios):.3f}")
    assert max(ratios) <= 1.0, f"error above the derived bound: per sequence got / bound {ratios}"


# ------------------------------------------------------------------------------------------------ tiled entry

@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("mode,lengths,H", TILED_CASES, ids=case_id)
def test_tiled_exact_selection_per_sequence(dev, lib, mode, lengths, H, ty):
    check_selection(lib, dev, kv.build_pack(lengths, H, ty, mode, "select"))


@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("mode,lengths,H", TILED_CASES, ids=case_id)
def test_tiled_gaussian_within_the_derived_bound(dev, lib, mode, lengths, H, ty):
    """Measured on an MI355X: see the table of DESIGN.md §24."""
    check_bound(lib, dev, kv.build_pack(lengths, H, ty, mode, "gauss"))


@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("S", [320, 512])
def test_tiled_equals_the_padded_tiled_kernel_bit_for_bit(dev, lib, S, causal, ty):
    """Two equal sequences above 288 tokens, where the padded entry takes its tiled kernel: the same arithmetic, the same bits."""
    H, N = 2, 2
    pack = kv.build_pack([S] * N, H, ty, "causal" if causal else "full", "gauss", seed=3)
    got = kv.run_pack(lib, dev, stream(), pack)
    src = kc.poisoned(pack.qkv, 3 * H * kc.HD, dev, dtype=pack.ty.dtype)
    ref = kc.Guarded(N * S, H * kc.HD, device=dev, dtype=pack.ty.dtype)
    rc = getattr(lib, f"dclip_attention_fwd_{ty}")(src.data_ptr(), ref.ptr, N, S, H, int(causal), stream())
    assert rc == 0, lib.dclip_last_error()
    assert lib.dclip_last_launch() == f"attention_fwd_{ty}.tiled".encode()
    torch.cuda.synchronize()
    want = ref.get()
    assert bool(torch.isfinite(want.float()).all())
    assert torch.equal(kv.bits(got), kv.bits(want))


@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("mode,lengths,H,victim", [("full", FULL_CASES[0][0], 2, 5), ("causal", CAUSAL_CASES[1][0], 1, 1)],
                         ids=case_id)
def test_a_nan_sequence_leaves_every_other_sequence_bit_identical(dev, lib, mode, lengths, H, victim, ty):
    pack = kv.build_pack(lengths, H, ty, mode, "gauss", seed=1)
    clean = kv.per_sequence(pack, kv.run_pack(lib, dev, stream(), pack))
    dirty_in = pack.qkv.clone()
    dirty_in[pack.cu[victim]:pack.cu[victim + 1]] = kc.NAN
    dirty = kv.per_sequence(pack, kv.run_pack(lib, dev, stream(), pack, qkv=dirty_in))
    for n in range(len(lengths)):
        if n == victim:
            assert bool(torch.isnan(dirty[n]).all())
            continue
        assert bool(torch.isfinite(dirty[n].float()).all()), n
        assert torch.equal(kv.bits(clean[n]), kv.bits(dirty[n])), f"sequence {n} changed with sequence {victim}"


@pytest.mark.parametrize("ty", TYPES)
def test_huge_later_keys_change_no_earlier_row(dev, lib, ty):
    """A causal 65-row sequence between two others with k of rows 64.. set to 1e4: rows 0..63 see none of them."""
    lengths, H = [5, 65, 9], 2
    D = H * kc.HD
    pack = kv.build_pack(lengths, H, ty, "causal", "gauss", seed=2)
    clean = kv.per_sequence(pack, kv.run_pack(lib, dev, stream(), pack))
    huge = pack.qkv.clone()
    huge[pack.cu[1] + 64:pack.cu[2], D:2 * D] = 1e4
    after = kv.per_sequence(pack, kv.run_pack(lib, dev, stream(), pack, qkv=huge))
    for n in (0, 2):
        assert torch.equal(kv.bits(clean[n]), kv.bits(after[n])), n
    assert bool(torch.isfinite(after[1].float()).all())
    assert torch.equal(kv.bits(clean[1][:64]), kv.bits(after[1][:64]))
    assert not torch.equal(kv.bits(clean[1][64]), kv.bits(after[1][64]))


@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("mode", ["full", "causal"])
def test_tiled_an_empty_sequence_between_two_others(dev, lib, mode, ty):
    pack = kv.build_pack([5, 0, 9], 2, ty, mode, "select")
    check_selection(lib, dev, pack)
    check_bound(lib, dev, kv.build_pack([5, 0, 9], 2, ty, mode, "gauss"))


# ------------------------------------------------------------------------------------------------ row entry

@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("mode", ["cls", "last"])
@pytest.mark.parametrize("lengths,H", ROW_CASES, ids=case_id)
def test_row_exact_selection_per_sequence(dev, lib, lengths, H, mode, ty):
    check_selection(lib, dev, kv.build_pack(lengths, H, ty, mode, "select"))


@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("mode", ["cls", "last"])
@pytest.mark.parametrize("lengths,H", ROW_CASES, ids=case_id)
def test_row_gaussian_within_the_derived_bound(dev, lib, lengths, H, mode, ty):
    """c_P = 0: the one-row kernel keeps P in fp32.  Measured on an MI355X: see the table of DESIGN.md §24."""
    check_bound(lib, dev, kv.build_pack(lengths, H, ty, mode, "gauss"))


@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("mode", ["cls", "last"])
def test_row_equals_the_padded_row_kernel_bit_for_bit(dev, lib, mode, ty):
    N, S, H = 5, 77, 2
    pack = kv.build_pack([S] * N, H, ty, mode, "gauss", seed=4)
    got = kv.run_pack(lib, dev, stream(), pack)
    src = kc.poisoned(pack.qkv, 3 * H * kc.HD, dev, dtype=pack.ty.dtype)
    ref = kc.Guarded(N, H * kc.HD, device=dev, dtype=pack.ty.dtype)
    rows = torch.full((N,), S - 1, dtype=torch.int32, device=dev) if mode == "last" else None
    rc = getattr(lib, f"dclip_attention_row_fwd_{ty}")(src.data_ptr(), None if rows is None else rows.data_ptr(), ref.ptr, N, S, H,
                                                       stream())
    assert rc == 0, lib.dclip_last_error()
    torch.cuda.synchronize()
    want = ref.get()
    assert bool(torch.isfinite(want.float()).all())
    assert torch.equal(kv.bits(got), kv.bits(want))


@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("mode", ["cls", "last"])
def test_row_an_empty_sequence_keeps_its_output_row(dev, lib, mode, ty):
    pack = kv.build_pack([5, 0, 9], 2, ty, mode, "select")
    kv.assert_margins(pack)
    out = kv.run_pack(lib, dev, stream(), pack)
    assert kv.is_poison(out[1]), "the empty sequence's output row was written"
    assert not kv.selection_failures(pack, out)
    gauss = kv.build_pack([5, 0, 9], 2, ty, mode, "gauss")
    out = kv.run_pack(lib, dev, stream(), gauss)
    assert kv.is_poison(out[1])
    assert max(r for r in kv.bound_ratios(gauss, out) if r is not None) <= 1.0


# ------------------------------------------------------------------------------------------------ refusals

@pytest.mark.parametrize("ty", TYPES)
def test_refusals_launch_nothing_and_write_nothing(dev, lib, ty):
    H, N, T = 2, 2, 7
    D = H * kc.HD
    dtype = kc.TYPES16[ty].dtype
    f = kc.poisoned(kc._gauss((T, 3 * D), 1), 3 * D, dev, dtype=dtype)
    tab = torch.tensor([0, 3, 7, 0, 0, 0, 0, 0], dtype=torch.int32, device=dev)     # a refusal never reads it
    outs = {k: kc.Guarded(T, D, device=dev, dtype=dtype) for k in ("tiled", "row")}
    lib.dclip_relu_f32(kc.Guarded(1, 64, device=dev).ptr, 64, stream())               # some other launch site
    s = stream()
    common = [(0, None), (1, None), (2, None), (3, 0), (3, -1), (4, 0), (4, -1), (5, 0), (5, -2), (3, 2 ** 30),
              (0, f.data_ptr() + 8), (1, tab.data_ptr() + 2)]
    calls = {
        "tiled": (getattr(lib, f"dclip_attention_varlen_fwd_{ty}"),
                  [f.data_ptr(), tab.data_ptr(), outs["tiled"].ptr, N, 4, H, 0, s], common + [(2, outs["tiled"].ptr + 8)]),
        "row": (getattr(lib, f"dclip_attention_varlen_row_fwd_{ty}"),
                [f.data_ptr(), tab.data_ptr(), outs["row"].ptr, N, 4, H, 0, s], common + [(2, outs["row"].ptr + 8), (4, 513)]),
    }
    for name, (fn, good, bad) in calls.items():
        for at, value in bad:
            args = list(good)
            args[at] = value
            assert fn(*args) == kc.E_INVAL, (name, at, value)
            assert lib.dclip_last_error()
            assert lib.dclip_last_launch() == b"relu_f32", f"a refused {name} call launched"
    torch.cuda.synchronize()
    for name, t in outs.items():
        t.assert_guards(f"refused {name}")
        assert kv.is_poison(t.get()), f"a refused {name} call wrote"
