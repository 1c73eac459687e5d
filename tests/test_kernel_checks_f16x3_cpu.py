"""Self-test of tests/kernel_checks_f16x3.py, no GPU: every case of tests/test_f16x3_paths_gpu.py passes its
checker when the restatement fills the buffers; one planted fault at a time fails the checker relied on for it; the case lists
reach every form and edge they were written for; and the plans of the library say what the header says."""
import pytest
import torch

from tests import kernel_checks_f16x3 as kx
from tests import kernel_checks_split16 as ks


def fails(verify, s, match):
    with pytest.raises(AssertionError, match=match):
        verify(s)


# ---------------------------------------------------------------------------------------------------- the K-major twins

@pytest.mark.parametrize("c", kx.x3_cases(), ids=kx.x3_id)
def test_every_fused_case_passes_on_the_restatement(c):
    s = kx.build_x3(c)
    kx.emulate_x3(s)
    kx.verify_x3(s)


@pytest.mark.parametrize("entry", ["scaled", "rows_dgelu", "split_dev_gelu_hg", "rows_stats"])
@pytest.mark.parametrize("fault", kx.PRODUCT_FAULTS)
@pytest.mark.parametrize("perm", [False, True])
def test_a_planted_product_fault_is_caught(fault, entry, perm):
    s = kx.build_x3(kx.X3Case(entry, 300, 264, 96, 1, perm))
    kx.emulate_x3(s, fault)
    fails(kx.verify_x3, s, "C|h32")


@pytest.mark.parametrize("fault,entry,match", [
    ("alpha_after_bias", "scaled_dev", "C: not exact"), ("row_alpha_next", "rows_dev", "C: not exact"),
    ("row_alpha_next", "rows_stats", "C: not exact"), ("aux_row_next", "rows_stats_dgelu", "C: .* beyond the bound"),
    ("lo_dropped", "split", "C: not the rounding"), ("third_piece_off", "split_dev", "C: "),
    ("g32_stride_ldc", "split_dev_g32", "g32: "), ("h32_is_g", "split_dev_gelu_hg", "h32: not exact")])
def test_a_planted_epilogue_fault_is_caught(fault, entry, match):
    s = kx.build_x3(kx.X3Case(entry, 300, 264, 64, 1, False))
    kx.emulate_x3(s, fault)
    fails(kx.verify_x3, s, match)


@pytest.mark.parametrize("fault,match", [("stats_all_rows", "pmax"), ("stats_sum_order", "psum")])
def test_a_planted_statistics_fault_is_caught(fault, match):
    s = kx.build_x3(kx.X3Case("rows_stats", 300, 264, 64, 1, False))
    kx.emulate_x3(s, fault)
    fails(kx.verify_x3, s, match)


def test_the_statistics_restatement_is_the_column_maximum_and_sum():
    C = torch.randint(-64, 65, (300, 8)).float() * 0.25        # dyadic: the sums are exact in any order
    pm, ps = kx.tile_stats(C)
    assert pm.shape == ps.shape == (2, 8)
    assert torch.equal(pm.view(torch.float32), torch.stack([C[:256].abs().amax(0), C[256:].abs().amax(0)]))
    assert torch.equal(ps, torch.stack([C[:256].sum(0), C[256:].sum(0)]))


def test_fused_cases_reach_every_situation():
    cases = kx.x3_cases()
    assert set(kx.X3_ENTRIES) == set(ks.GEMM_ENTRIES) | {"rows_stats", "rows_stats_dgelu"}
    for e in kx.X3_ENTRIES:
        mine = [c for c in cases if c.entry == e]
        assert [c.K for c in mine] == kx.X3_K and len({(c.M, c.N) for c in mine}) == 3
    for K in kx.X3_K:
        assert {(c.M, c.N) for c in cases if c.K == K} == set(kx.X3_SHAPES)
    assert {(c.M, c.N) for c in cases} == {(M, N) for M, N, _ in ks.GEMM_KERNELS["pp"][0]}
    assert {c.perm for c in cases} == {False, True} and {c.cpad for c in cases} == {0, 1}
    assert {kx.X3_FORMS[c.entry]["fn"] for c in cases} == set(kx.X3_NAMES)
    s = kx.build_x3(kx.X3Case("scaled", 257, 260, 32, 0, False))
    A, W = s.A.float(), s.W.float()
    assert bool(torch.isfinite(A[:257, :64]).all()) and bool(torch.isnan(A[:257, 64:]).all()) and bool(torch.isnan(A[257:]).all())
    assert bool(torch.isfinite(W[:260, :32]).all()) and bool(torch.isnan(W[:260, 32:64]).all()) and bool(torch.isfinite(W[:260, 64:96]).all())
    assert bool(torch.isnan(W[:260, 96:]).all()) and s.lda == s.ldw == 104
    s = kx.build_x3(kx.X3Case("scaled", 257, 260, 32, 0, True))
    assert s.offs == (64, 0, 32, 0) and bool(torch.isnan(s.A.float()[:257, 32:64]).all()) and bool(torch.isnan(s.W.float()[:260, 64:]).all())
    ah, al, wh, wl = s.pieces                              # four independent matrices: no product equals another
    assert not torch.equal(ah, al) and not torch.equal(wh, wl)
    assert not torch.equal(ah @ wl.t(), al @ wh.t()) and bool((al @ wl.t() != 0).any())


# ---------------------------------------------------------------------------------------------------- the token-major twin

@pytest.mark.parametrize("c", kx.tok_cases(), ids=kx.tok_id)
def test_every_token_major_case_passes_on_the_restatement(c):
    s = kx.build_tok(c)
    kx.emulate_tok(s)
    kx.verify_tok(s)


@pytest.mark.parametrize("fault,match", [("product_dropped", "C: not exact"), ("product_swapped", "C: not exact"),
                                         ("lo_lo_added", "C: not exact"), ("tokens_shifted", "C: not exact"),
                                         ("slab_left_out", "C: not exact"), ("slab_unwritten", "workspace: 1 words"),
                                         ("ws_behind", "workspace: wrote behind"), ("c_pad", "C: memory outside")])
@pytest.mark.parametrize("perm", [False, True])
def test_a_planted_token_major_fault_is_caught(fault, match, perm):
    s = kx.build_tok(kx.TokCase(264, 8, 192, 2, perm))
    kx.emulate_tok(s, fault)
    fails(kx.verify_tok, s, match)


def test_token_major_cases_reach_every_situation():
    cases = kx.tok_cases()
    assert {(c.tokens, c.splits) for c in cases} == {(t, k) for t in (64, 128, 192, 1088) for k in (1, 2, 3)}
    sizes = {(m, n) for m in ks.SEG_SIZES for n in ks.SEG_SIZES}
    for t in kx.TOK_TOKENS:
        assert {(c.M, c.N) for c in cases if c.tokens == t} == sizes
    assert {(c.M, c.N, c.perm) for c in cases} >= {(m, n, p) for m, n in sizes for p in (False, True)}
    assert [ks.seg_s_eff(1088, k) for k in (1, 2, 3)] == [(1088, 1), (576, 2), (384, 3)]       # 34, 18 + 16, 12 + 12 + 10 K-tiles of 32
    assert ks.seg_s_eff(64, 3) == (64, 1) and ks.seg_s_eff(128, 3) == (64, 2)                  # s_eff < splits
    s = kx.build_tok(kx.TokCase(8, 264, 192, 2, False))
    assert bool(torch.isnan(s.xd.float()[:192, 2 * 264:]).all()) and bool(torch.isfinite(s.xd.float()[:192, :2 * 264]).all())
    assert s.ws_bytes == 2 * 8 * 264 * 4


# ---------------------------------------------------------------------------------------------------- the plans (host code)

def test_the_plans_say_what_the_header_says(monkeypatch):
    from dclip_amd import _lib
    lib = _lib.load()
    for k in ("DCLIP_BF16_BIG_MIN", "DCLIP_F16X3_MIN", "DCLIP_F16X3_TOK_MIN"):
        monkeypatch.delenv(k, raising=False)
    # K-major: 1 exactly where the 3 K form takes the ping-pong kernel (3 K % 64 == 0 and at least 128 tiles)
    for M, N, K, want in [(12800, 2304, 768, 1), (12800, 768, 3072, 1), (19712, 512, 2048, 1), (19712, 1536, 512, 1),
                          (1088, 192, 64, 0), (12800, 2304, 96, 0), (12800, 2304, 760, 0), (0, 8, 64, 0)]:
        assert lib.dclip_gemm_f16x3_plan(M, N, K) == want, (M, N, K)
        assert lib.dclip_gemm_f16x3_scaled_rows_stats_plan(M, N, K) == want * -(-M // 256)
        if want:
            assert lib.dclip_gemm_f16_scaled_rows_stats_plan(M, N, 3 * K) == -(-M // 256)
    monkeypatch.setenv("DCLIP_BF16_BIG_MIN", "1")                               # alone it moves the unfused entries only
    assert lib.dclip_gemm_f16x3_plan(1088, 192, 64) == 0 and lib.dclip_gemm_f16_scaled_rows_stats_plan(1088, 192, 192) == 5
    monkeypatch.setenv("DCLIP_F16X3_MIN", "1")
    assert lib.dclip_gemm_f16x3_plan(1088, 192, 64) == 1 and lib.dclip_gemm_f16x3_plan(1088, 192, 96) == 0
    monkeypatch.delenv("DCLIP_BF16_BIG_MIN")
    assert lib.dclip_gemm_f16x3_plan(1088, 192, 64) == 0                        # never where the 3 K form is register-staged
    # token-major: one round of 256 work items in whole 64-token units, 0 below 128 work items
    for M, N, want in [(2304, 768, 9), (768, 768, 25), (3072, 768, 7), (768, 3072, 7)]:
        assert lib.dclip_gemm_f16x3_wgrad_tokmajor_plan(M, N, 12800) == want, (M, N)
        assert -(-M // 256) * -(-N // 256) * want >= 128
    assert lib.dclip_gemm_f16x3_wgrad_tokmajor_plan(192, 64, 1088) == 0          # the tiny tower keeps the segmented form
    assert lib.dclip_gemm_f16_wgrad_tokmajor_seg3_plan(192, 64, 1088) > 0
    assert lib.dclip_gemm_f16x3_wgrad_tokmajor_plan(768, 768, 12801) == 0
    monkeypatch.setenv("DCLIP_F16X3_TOK_MIN", "1")
    assert lib.dclip_gemm_f16x3_wgrad_tokmajor_plan(192, 64, 1088) == 5


def test_refusals_need_no_gpu():
    from dclip_amd import _lib
    lib = _lib.load()
    p = 4096                                               # never dereferenced: every case below is refused before a launch
    good = [p, p, p, None, None, 256, 256, 64, 200, 200, 256, 0, 64, 0, 128, 0, 0, 1.0, None]
    assert lib.dclip_gemm_f16x3_scaled(*good[:7], 0, *good[8:]) == -1
    for at, value in [(7, 48), (7, 72), (11, 4), (12, 68), (13, -8), (14, 130), (12, 144), (14, 144), (8, 196), (9, 190), (10, 254),
                      (0, p + 8), (0, None)]:
        args = list(good)
        args[at] = value
        assert lib.dclip_gemm_f16x3_scaled(*args) == -1, (at, value)
        assert lib.dclip_last_error()
    tok = [p, p, p, 64, 64, 128, 136, 200, 64, 0, 64, 0, 64, p, p, 2, p, 1 << 20, None]
    for at, value in [(5, 96), (3, 60), (9, 4), (10, 80), (12, 144), (11, -8), (15, 0), (15, 65), (6, 132), (8, 62), (13, None)]:
        args = list(tok)
        args[at] = value
        assert lib.dclip_gemm_f16x3_wgrad_tokmajor(*args) == -1, (at, value)
    args = list(tok)
    args[17] = 2 * 64 * 64 * 4 - 1
    assert lib.dclip_gemm_f16x3_wgrad_tokmajor(*args) == -2 and b"32768" in lib.dclip_last_error()
