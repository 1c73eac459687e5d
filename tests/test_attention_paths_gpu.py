"""Every forward and backward kernel of the fp32 attention (dclip_amd/csrc/attention.hip) through the C ABI against fp64:
self-attention under the default dispatch and under DCLIP_ATTN_TILED / _FUSED / _NO_DS, cross-attention (including the
equal-length cases that take the self-attention kernels with q / kv row strides E and 2E), the CLS-only entries and the
one-row entry.  Outputs are guarded, errors are judged per block (out, lse, dq, dk, dv) at the project's figures, lse is
compared with fp64 logsumexp, and every case asserts the launch sites dclip_last_launch reports.  Checkers and case lists:
tests/kernel_checks.py."""
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


def run(lib, dev, monkeypatch, case, env):
    for k in kc.ATTN_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s = kc.build_attn(case, dev)
    sites = kc.launch_attn(lib, s, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert sites == kc.expected_launches(case), (case, sites)
    fig = kc.verify_attn(s)
    print(kc.case_id(case), sites, fig)
    kc.record("attn", case, dict(fig, sites=list(sites)))
    return fig


@pytest.mark.parametrize("case", kc.self_cases(), ids=kc.case_id)
def test_self_attention(dev, lib, monkeypatch, case):
    run(lib, dev, monkeypatch, case, kc.ATTN_ENV[case.mode])


@pytest.mark.parametrize("case", kc.cross_cases(), ids=kc.case_id)
def test_cross_attention(dev, lib, monkeypatch, case):
    run(lib, dev, monkeypatch, case, {})


@pytest.mark.parametrize("case", kc.CLS_CASES, ids=kc.case_id)
def test_cls_attention(dev, lib, monkeypatch, case):
    """Forward: row 0 of the full fp64 attention; backward: the fp64 gradient of that row alone, q gradients of the other
    rows exactly zero."""
    run(lib, dev, monkeypatch, case, {})


@pytest.mark.parametrize("case", kc.ROW_CASES, ids=kc.case_id)
def test_row_attention(dev, lib, monkeypatch, case):
    run(lib, dev, monkeypatch, case, {})
