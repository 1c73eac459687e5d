"""Every path of dclip_amd/csrc/optim.hip through the C ABI: the sum-of-squares partials (exact on integers,
exactly dclip_sumsq_blocks(n) / total_chunks entries written), the two clip coefficients, the loss-scale state machine
against torch's rule, and one Adam / AdamW / SKIP step from a random state per element under a derived bound against fp64 —
on tables whose tensors straddle the chunk size, start 4 bytes behind a 16-byte boundary (the kernels' scalar branch, which
torch's allocator never produces) and carry different step counts.  Checkers and case lists: tests/kernel_checks_rest.py."""
import pytest
import torch

from tests import kernel_checks as kc
from tests import kernel_checks_rest as kr

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
    assert rc == 0, lib.dclip_last_error()
    assert lib.dclip_last_launch().decode() == site
    torch.cuda.synchronize()


@pytest.mark.parametrize("n", kr.SUMSQ_N)
def test_sumsq_partials_are_exact_on_integers(dev, lib, n):
    s = kr.build_sumsq(n, dev)
    ok(lib, kr.launch_sumsq(lib, s, stream()), "sumsq")
    kr.verify_sumsq(s)


@pytest.mark.parametrize("case", kr.clip_cases(), ids=kc.case_id)
def test_clip_coefficients(dev, lib, case):
    s = kr.build_clip(case, dev)
    ok(lib, kr.launch_clip(lib, s, stream()), "clip_coef_scaled" if case.scale else "clip_coef")
    kr.verify_clip(s)


@pytest.mark.parametrize("row", kr.AMP_TABLE, ids=kc.case_id)
def test_amp_update_scale_follows_torchs_rule(dev, lib, row):
    s = kr.build_amp(row, dev)
    ok(lib, kr.launch_amp(lib, s, stream()), "amp_update_scale")
    kr.verify_amp(s)


MT_SITE = {"adamw": "mt_adamw", "adam": "mt_adam", "skip": "mt_adamw_skip", "skip_found_inf": "mt_adamw_skip", "sumsq": "mt_sumsq"}


@pytest.mark.parametrize("case", kr.mt_cases(), ids=kr.mt_id)
def test_multi_tensor_entries_one_step(dev, lib, case):
    chunk = int(lib.dclip_mt_chunk_elems())
    s = kr.build_mt(case, dev, chunk)
    assert s.total == sum(-(-t.n // chunk) for t in s.tens)
    ok(lib, kr.launch_mt(lib, s, stream()), MT_SITE[case.entry])
    fig = kr.verify_mt(s)
    print(kr.mt_id(case), fig)
    kc.record("mt", tuple(case), fig)


def test_multi_tensor_cases_reach_both_branches_of_every_entry():
    for entry in ("adamw", "adam", "skip", "sumsq"):
        seen = set()
        for c in kr.mt_cases():
            if c.entry == entry:
                sizes = kr.mt_sizes(kr.MT_CHUNK_DOC)
                seen |= {(sizes[k], kr.mt_mis(k, c.shift)) for k in c.order}
        assert {m for _, m in seen} >= ({"", "g"} if entry == "sumsq" else {"", "p", "g", "m", "v", "pgmv"}), (entry, seen)
        for n in kr.mt_sizes(kr.MT_CHUNK_DOC):
            assert any(m == "" for k, m in seen if k == n) and any(m != "" for k, m in seen if k == n), (entry, n)


@pytest.mark.parametrize("case", kr.adamw_cases(), ids=kc.case_id)
def test_adamw_single_tensor_one_step(dev, lib, case):
    s = kr.build_adamw(case, dev)
    ok(lib, kr.launch_adamw(lib, s, stream()), "adamw")
    print(case, kr.verify_mt(s))


def test_adamw_refuses_misaligned_tensors(dev, lib):
    s = kr.build_adamw(kr.AdamwCase(64, 1, 0.0, None), dev)
    t = s.tens[0]
    rc = lib.dclip_adamw_f32(t.buf["p"].ptr + 4, t.buf["g"].ptr, t.buf["m"].ptr, t.buf["v"].ptr, 60, kr.LR, kr.BETA1, kr.BETA2, kr.ADAM_EPS,
                             0.0, 1, None, stream())
    torch.cuda.synchronize()
    assert rc == kc.E_INVAL and b"aligned" in lib.dclip_last_error()
    assert torch.equal(t.buf["p"].get()[0], t.st["p"])
