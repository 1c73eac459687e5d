"""Every path of the 16-bit attention file (dclip_amd/csrc/attention_bf16.hip) through the C ABI: the whole-head forward at every
NB and its boundaries, the shared-last-query kernel at 257 tokens, the tiled forward, the lse forward, the two-wave backward
and the one-row forward, for both types and both causal settings.  Every case runs twice in guarded buffers: on exact-selection
data (bit-exact out and dV, dQ = dK = 0) and on Gaussian data under the derived per-element bounds.  DCLIP_ATTN16_TILED and
DCLIP_ATTN16_NO_XQ (once-read) run the forward list in one fresh process each.  Checkers and case lists:
tests/kernel_checks.py; every case asserts the kernel variant dclip_last_launch reports."""
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


@pytest.fixture(autouse=True)
def _nothing_starts_after_an_abnormal_child():
    kc.assert_no_child_ended_abnormally()


N_FWD = 2 * sum(1 for c in kc.attn16_cases() if c.entry == "fwd")


def test_forward_list_on_the_tiled_kernel_alone():
    out = kc.run_child16("attention", {"DCLIP_ATTN16_TILED": "1"})
    assert out["cases"] == N_FWD and not out["failed"], out["failed"][:5]
    assert set(out["sites"]) == {"attention_fwd_bf16.tiled", "attention_fwd_f16.tiled"}


def test_forward_list_without_the_shared_last_query():
    out = kc.run_child16("attention", {"DCLIP_ATTN16_NO_XQ": "1"})
    assert out["cases"] == N_FWD and not out["failed"], out["failed"][:5]
    assert not any(k.endswith("head_xq") for k in out["sites"]) and out["sites"]["attention_fwd_bf16.head9"] >= 8


@pytest.mark.parametrize("data", ["select", "gauss"])
@pytest.mark.parametrize("case", kc.attn16_cases(), ids=kc.case_id)
def test_attention16(dev, lib, case, data):
    s = kc.build_attn16(case, dev, data)
    sites = kc.launch_attn16(lib, s, stream())
    torch.cuda.synchronize()
    want = [kc.expected_attn16_site(case, "lse"), kc.expected_attn16_site(case, "bwd")][:len(sites)] \
        if case.entry in ("lse", "train") else [kc.expected_attn16_site(case)]
    assert sites == want, (kc.case_id(case), sites)
    fig = kc.verify_attn16(s, f"{kc.case_id(case)}-{data}")
    fig["sites"] = sites
    if case.entry in ("lse", "train"):                   # out of the lse entry == out of the plain entry, bit for bit
        plain = kc.Guarded(case.B * case.S, case.H * kc.HD, device=dev, dtype=s.ty.dtype)
        assert getattr(lib, f"dclip_attention_fwd_{case.ty}")(s.qkv.data_ptr(), plain.ptr, case.B, case.S, case.H, int(case.causal),
                                                              stream()) == 0
        torch.cuda.synchronize()
        plain.assert_guards("plain forward")
        assert torch.equal(plain.get().view(torch.int16), s.out.get().view(torch.int16)), "the lse entry's out differs from the plain entry's"
    kc.record("attn16_" + data, case, {k: v for k, v in fig.items()})


def test_every_launch_site_of_the_file_has_a_case():
    sites = set()
    for c in kc.attn16_cases():
        sites.add(kc.expected_attn16_site(c))
        if c.entry in ("lse", "train"):
            sites.add(kc.expected_attn16_site(c, "lse"))
        if c.entry == "train":
            sites.add(kc.expected_attn16_site(c, "bwd"))
    for ty in ("bf16", "f16"):
        assert {f"attention_fwd_{ty}.head{nb}" for nb in range(1, 10)} | {f"attention_fwd_{ty}.head_xq", f"attention_fwd_{ty}.tiled",
                f"attention_bwd_{ty}", f"attention_bwd_{ty}.one_key", f"attention_row_fwd_{ty}"} <= sites
    assert {f"attention_fwd_bf16_lse.head{nb}" for nb in range(1, 10)} | {"attention_fwd_f16_lse.head1", "attention_fwd_f16_lse.head2"} <= sites
    for causal in (False, True):                         # both causal instances of every NB
        assert {-(-c.S // 32) for c in kc.attn16_cases() if c.entry == "fwd" and c.causal == causal and c.S <= 288} == set(range(1, 10))


@pytest.mark.parametrize("entry,ty,S", [("lse", "bf16", 257), ("lse", "bf16", 289), ("lse", "f16", 65), ("train", "bf16", 65),
                                        ("train", "f16", 65)])
def test_documented_rejections(dev, lib, entry, ty, S):
    """Refused on the host before any launch: the outputs keep their NaN payload."""
    case = kc.Attn16Case(entry, ty, 2, S, 2, False, None)
    s = kc.build_attn16(case, dev, "gauss")
    t, ci = ty, 0
    if entry == "lse":
        rc = getattr(lib, f"dclip_attention_fwd_{t}_lse")(s.qkv.data_ptr(), s.out.ptr, s.lse.ptr, 2, S, 2, ci, stream())
    else:
        s.lse.payload.fill_(0.0)
        s.out.payload.fill_(0.0)
        rc = getattr(lib, f"dclip_attention_bwd_{t}")(s.qkv.data_ptr(), s.out.ptr, s.dout.data_ptr(), s.lse.ptr, s.dqkv.ptr, 2, S, 2, ci,
                                                      stream())
    torch.cuda.synchronize()
    assert rc == kc.E_INVAL and lib.dclip_last_error()
    for name in ("out", "lse", "dqkv"):
        if hasattr(s, name):
            getattr(s, name).assert_guards("refused " + name)
    target = s.out if entry == "lse" else s.dqkv
    assert bool(torch.isnan(target.get()).all()), "a refused call wrote to its output"
