"""CPU-only: the 16-bit checkers of tests/kernel_checks.py pass on a plain PyTorch evaluation that applies the
documented roundings — operands in 16 bits, fp32 accumulation, output and aux rounded with the type's rule; attention in fp64
with P and dS rounded to the type — for every case the GPU path tests run, and fail on each of a set of planted faults, each
caught by the checker that is relied on for it: the exact checks for the structural faults, the derived bounds for the faults
only a bound can see."""
import pytest
import torch

from tests import kernel_checks as kc

D = "cpu"


def run(case, fault=None, before=None):
    s = kc.build_gemm16(case, D)
    if before:
        before(s)
    kc.emulate_gemm16(s)
    if fault:
        fault(s)
    return kc.verify_gemm16(s)


def first(pred, cases=None):
    return next(c for c in (cases or kc.gemm16_matrix()) if pred(c))


def run_attn(case, data, fault=None, mask_edit=None):
    s = kc.build_attn16(case, D, data)
    orig = kc._attn16_mask
    if mask_edit:                                  # the emulation alone sees the wrong mask; the checker keeps the right one
        def wrong(c, s_):
            m, rows = orig(c, s_)
            m = m.expand(c.B, 1, m.shape[2], c.S).clone()
            mask_edit(m)
            return m, rows
        kc._attn16_mask = wrong
    try:
        kc.emulate_attn16(s)
    finally:
        kc._attn16_mask = orig
    if fault:
        fault(s)
    return kc.verify_attn16(s)


# ------------------------------------------------------------------------------------------------ the cases themselves

def test_the_matrix_reaches_every_variant_type_epilogue_and_padding():
    m = kc.gemm16_matrix()
    assert len({kc.case16_id(c) for c in m}) == len(m)
    assert all(c.N % 4 == 0 and 4 * c.K <= 51200 for c in m)
    for want in ("r64", "pp"):
        for ty in ("bf16", "f16", "f16ex"):
            mine = [c for c in m if c.entry == "gemm" and c.want == want and c.ty == ty and c.data == "int"]
            assert {(c.epi, c.out16, c.save) for c in mine} == {e for e in kc.EPI16 if kc.epi_ok(ty, e)}, (want, ty)
            assert {c.pads[0] for c in mine} == {c.pads[1] for c in mine} == {0, 8, 40} and {c.pads[2] for c in mine} >= {0, 4, 36}
        assert {c.K for c in m if c.want == want and c.entry == "gemm"} >= ({64, 128, 192, 72, 85, 149, 4100} if want == "r64" else {64, 128, 192})
    ppp = [c for c in m if c.want == "ppp"]
    assert {-(-c.M // 256) * -(-c.N // 256) for c in ppp} == {1, 7, 9, 272}
    for entry in ("splitk", "tok"):
        for ty in ("bf16", "f16ex"):
            mine = [c for c in m if c.entry == entry and c.ty == ty]
            assert any(kc.s_eff16(c.K, c.splits) < c.splits for c in mine) and any(c.K % kc.roundup(-(-c.K // c.splits), 64) for c in mine)
            assert {1, 2, 3, 7, 64} <= {c.splits for c in mine}
            assert {c.pads[0] for c in mine} == {c.pads[1] for c in mine} == {0, 8, 40}
    assert any(c.entry == "tok" and kc.s_eff16(c.K, c.splits) == 1 for c in m)
    assert (12800, 3072, 768) in {(c.M, c.N, c.K) for c in m} and (768, 768, 12800) in {(c.M, c.N, c.K) for c in m}


def test_integer_products_stay_exact_through_both_16_bit_types():
    a, w, acc, _ = kc._operands16(96, 80, 12800, "int", torch.bfloat16)
    assert float((a.abs() @ w.abs().t()).max()) < 2 ** 24
    for dt in (torch.bfloat16, torch.float16):
        assert torch.equal(a.to(dt).float(), a) and torch.equal(w.to(dt).float(), w)
    assert torch.equal(acc.double(), (a.long() @ w.long().t()).double())


@pytest.mark.parametrize("entry", ["gemm", "splitk", "tok"])
def test_integer_matrix_passes_on_the_documented_roundings(entry):
    for c in kc.gemm16_matrix():
        if c.entry == entry:
            run(c)


def test_gaussian_cases_pass_and_the_bound_is_not_vacuous():
    worst16, worst32 = 0.0, 0.0
    for c in kc.gemm16_gaussian_matrix():
        fig = run(c)
        r = max(v for k, v in fig.items() if k.endswith("ratio"))
        if c.out16 or c.save:
            worst16 = max(worst16, r)
        else:
            worst32 = max(worst32, r)
    assert 0.5 < worst16 <= 1.0            # one rounding to 16 bits reaches u |want|: the bound has no slack to hide in
    assert 0.0 < worst32 < 0.5


def test_attention_cases_pass_on_the_documented_roundings_and_the_margin_holds():
    worst, margin = {}, float("inf")
    for c in kc.attn16_cases():
        for data in ("select", "gauss"):
            s = kc.build_attn16(c, D, data)
            kc.emulate_attn16(s)
            fig = kc.verify_attn16(s)
            if data == "select":
                margin = min(margin, s.margin)
                assert all(v == 0.0 for v in fig.values()), (c, fig)          # lse == 512 exactly; everything else is bit-exact
            else:
                for k, v in fig.items():
                    worst[k] = max(worst.get(k, 0.0), v)
    assert margin == 208.0, margin                                          # seed 0, the one the GPU tests use
    assert all(0.3 < worst[k] <= 1.0 for k in ("out", "dq", "dk", "dv")), worst   # the bounds are reached to within ~2x
    others = min(kc.build_attn16(c, D, "select", seed).margin for seed in (1, 2) for c in kc.attn16_cases())
    assert others == 192.0, others                                          # smallest over seeds 0-2; MIN_MARGIN is 120


def test_a_selection_case_with_too_small_a_margin_is_refused(monkeypatch):
    monkeypatch.setattr(kc, "MIN_MARGIN", 600.0)
    with pytest.raises(ValueError, match="case refused"):
        kc.build_attn16(kc.Attn16Case("fwd", "bf16", 1, 50, 1, False, None), D, "select")


def test_round16_follows_each_types_overflow_rule():
    x = torch.tensor([65504.0, 65519.0, 65520.0, 1e6, -1e6, float("inf"), kc.NAN, 2.0 ** -25, 3 * 2.0 ** -25])
    sat, ieee = kc.round16(x, kc.TYPES16["f16"]).float(), kc.round16(x, kc.TYPES16["f16ex"]).float()
    assert sat[:7].tolist()[:6] == [65504.0, 65504.0, 65504.0, 65504.0, -65504.0, float("inf")] and bool(torch.isnan(sat[6]))
    assert ieee.tolist()[:6] == [65504.0, 65504.0, float("inf"), float("inf"), float("-inf"), float("inf")]
    assert sat[7:].tolist() == [0.0, 2.0 ** -23] and ieee[7:].tolist() == [0.0, 2.0 ** -23]       # ties to even in the subnormals
    assert float(kc.round16(torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8]), kc.TYPES16["bf16"]).float().sum()) == 2.0 + 2.0 ** -6


def test_layernorm16_checker_passes_on_fp32_and_sees_a_truncated_output():
    g = torch.Generator().manual_seed(3)
    x, ga, be = torch.randn((5, 772), generator=g) * 2 + 1, torch.randn((772,), generator=g), torch.randn((772,), generator=g)
    mu = x.mean(1, keepdim=True)
    rs = torch.rsqrt(((x - mu) ** 2).mean(1, keepdim=True) + 1e-5)
    y = (x - mu) * rs * ga + be
    for ty in kc.TYPES16.values():
        kc.verify_ln16(kc.round16(y, ty), mu[:, 0], rs[:, 0], x, ga, be, 1e-5, ty, "ln")
    trunc = (y.view(torch.int32) & -65536).view(torch.float32).bfloat16()
    with pytest.raises(AssertionError, match="x \\(u \\|want\\|"):
        kc.verify_ln16(trunc, None, None, x, ga, be, 1e-5, kc.TYPES16["bf16"], "ln")
    with pytest.raises(AssertionError, match="rstd"):
        kc.verify_ln16(kc.round16(y, kc.TYPES16["bf16"]), mu[:, 0], rs[:, 0] * (1 + 1e-4), x, ga, be, 1e-5, kc.TYPES16["bf16"], "ln")


# ------------------------------------------------------------------------------------------------ planted GEMM faults

K12800 = first(lambda c: c.K == 12800 and c.entry == "splitk" and c.ty == "bf16")
OUT16 = first(lambda c: c.entry == "gemm" and c.out16 and c.epi == kc.EPI_BIAS and c.M >= 255 and c.pads[2] == 4)
SAVE32 = first(lambda c: c.save and c.epi & kc.EPI_GELU and not c.out16 and c.K >= 192, kc.gemm16_gaussian_matrix())


def test_fault_one_k_element_dropped_at_k_12800():
    def drop(s):
        k = int((s.a[5] * s.w[7]).nonzero()[0])
        s.C.payload[5, 7] -= s.a[5, k] * s.w[7, k]
    with pytest.raises(AssertionError, match="not the exact integer result"):
        run(K12800, drop)


def test_fault_one_tile_transposed_in_place():
    def transpose(s):
        s.C.payload[64:128, 128:192] = s.C.payload[64:128, 128:192].t().clone()
    with pytest.raises(AssertionError, match="not the exact rounded integer result"):
        run(OUT16, transpose)


def test_fault_one_tile_never_written():
    """On memory the allocator hands back from the previous, identical call the tile still holds the right answer; on the
    16-bit NaN payload it does not."""
    s = kc.build_gemm16(OUT16, D)
    assert bool((s.C.payload.view(torch.int16) == kc.NAN16[s.ty.dtype]).all())
    with pytest.raises(AssertionError, match=r"NaN \(unwritten\?\)"):
        run(OUT16, lambda s: s.C.payload[64:128, 0:64].fill_(kc.NAN))


def test_fault_one_16_bit_element_outside_the_output():
    one = 0x3F80 if OUT16.ty == "bf16" else 0x3C00
    with pytest.raises(AssertionError, match=r"outside .* was written at \(row, col\) \[\(17, %d\)\]" % OUT16.N):
        run(OUT16, lambda s: s.C.mat.view(torch.int16).__setitem__((17, OUT16.N), one))          # the ldc padding
    with pytest.raises(AssertionError, match=r"\(%d, 3\)" % OUT16.M):
        run(OUT16, lambda s: s.C.buf.__setitem__(s.C.guard + s.C.rows * s.C.ld + 3, one))       # one row past M
    with pytest.raises(AssertionError, match=r"\(-1, "):
        run(OUT16, lambda s: s.C.buf.__setitem__(s.C.guard - 2, 0))                              # in front of row 0
    aux = first(lambda c: c.save and c.epi & kc.EPI_GELU and c.pads[2])
    with pytest.raises(AssertionError, match="aux: memory outside"):
        run(aux, lambda s: s.aux.mat.view(torch.int16).__setitem__((0, aux.N + 1), 0))
    sk = first(lambda c: c.entry == "splitk" and c.splits == 3)
    with pytest.raises(AssertionError, match="behind the s_eff slabs"):
        run(sk, lambda s: s.ws.payload.__setitem__((0, s.ws_need + 5), 0.0))


def truncate16(v, ty):
    """fp32 -> 16 bits by dropping the low bits (round toward zero) instead of round to nearest even."""
    if ty.dtype == torch.bfloat16:
        return (v.view(torch.int32) & -65536).view(torch.float32).bfloat16()
    h = v.half()
    over = h.float().abs() > v.abs()
    return torch.where(over, (h.view(torch.int16) - 1).view(torch.float16), h)


@pytest.mark.parametrize("ty", ["bf16", "f16ex"])
def test_fault_16_bit_output_truncated_instead_of_rounded(ty):
    def trunc(s):
        v = s.A[:s.case.M, :s.case.K].float() @ s.W[:s.case.N, :s.case.K].float().t()
        if s.case.epi & kc.EPI_BIAS:
            v = v + s.bias_d
        s.C.payload.copy_(truncate16(v.contiguous(), s.ty))
    plain = lambda c: c.entry == "gemm" and c.ty == ty and c.out16 and not c.epi & ~kc.EPI_BIAS
    with pytest.raises(AssertionError, match="x the derived bound"):                # the bound: the checker relied on for it
        run(first(lambda c: plain(c) and c.K >= 85, kc.gemm16_gaussian_matrix()), trunc)
    big = first(lambda c: plain(c) and c.K >= 768 and c.data == "int")
    if ty == "bf16":                                                               # integers beyond 2^8 are rounded too
        with pytest.raises(AssertionError, match="not the exact rounded integer result"):
            run(big, trunc)


def test_fault_fp16_overflow_rule_of_the_other_type():
    sat = first(lambda c: c.data == "big" and c.ty == "f16")
    ieee = first(lambda c: c.data == "big" and c.ty == "f16ex")
    s = kc.build_gemm16(ieee, D)
    kc.emulate_gemm16(s)
    assert bool(torch.isinf(s.C.get()).any())                                       # the case does overflow
    with pytest.raises(AssertionError, match="got 65504.0, want inf"):
        run(ieee, lambda s: s.C.payload.copy_(s.C.payload.float().clamp(-65504, 65504)))
    with pytest.raises(AssertionError, match="got inf, want 65504.0"):
        run(sat, lambda s: s.C.payload.copy_(torch.where(s.C.payload.float().abs() >= 65504, s.C.payload.float() * 2, s.C.payload.float())))


def test_fault_aux_rounded_but_gelu_of_the_unrounded_value():
    def mix(s):
        v = s.A[:s.case.M, :s.case.K].float() @ s.W[:s.case.N, :s.case.K].float().t() + s.bias_d
        s.C.payload.copy_(v * torch.sigmoid(1.702 * v))                              # aux stays the rounded value
    with pytest.raises(AssertionError, match=r"gelu: error is .* x \(1e-5\) \|want\|"):
        run(SAVE32, mix)


def test_fault_padding_read_and_multiplied_by_zero():
    """A kernel that loads the K padding and relies on a zero in the other operand: NaN * 0 = NaN."""
    c = first(lambda c: c.entry == "gemm" and c.pads[0] and c.epi == 0 and not c.out16)
    s = kc.build_gemm16(c, D)
    a = s.A[:c.M, :c.K + 8].float()                                                  # eight padding columns come along
    w = torch.cat([s.W[:c.N, :c.K].float(), torch.zeros(c.N, 8)], 1)
    s.C.payload.copy_(a @ w.t())
    with pytest.raises(AssertionError, match="NaN"):
        kc.verify_gemm16(s)
    t = first(lambda c: c.entry == "tok" and c.pads[0])                              # token-major: columns M..lddy of dY
    s = kc.build_gemm16(t, D)
    kc.emulate_gemm16(s)
    s.C.payload[t.M - 1] += (s.A[:t.K, t.M:t.M + 1].float() * 0.0).sum()
    with pytest.raises(AssertionError, match="NaN"):
        kc.verify_gemm16(s)


@pytest.mark.parametrize("entry", ["splitk", "tok"])
def test_fault_one_slab_unused(entry):
    """A library that splits into fewer slabs than cdiv(K, roundup(cdiv(K, splits), 64)) gives the right C and leaves a slab
    of the workspace as it was."""
    c = first(lambda c: c.entry == entry and kc.s_eff16(c.K, c.splits) == 3 and c.K == 192)
    with pytest.raises(AssertionError, match=r"slab\(s\) \[2\] of the 3 .* were not \(fully\) written"):
        run(c, lambda s: s.ws.payload[0, 2 * c.M * c.N:3 * c.M * c.N].fill_(kc.NAN))
    with pytest.raises(AssertionError, match=r"slab\(s\) \[1\] of the 3"):
        run(c, lambda s: s.ws.payload.__setitem__((0, c.M * c.N + 7), kc.NAN))


@pytest.mark.parametrize("entry", ["splitk", "tok"])
def test_fault_a_split_k_slab_added_twice_or_left_out(entry):
    c = first(lambda c: c.entry == entry and kc.s_eff16(c.K, c.splits) == 3 and c.K == 192)

    def slab(s, sign):
        s.C.payload.add_(sign * (s.a[:, 64:128] @ s.w[:, 64:128].t()))
    for sign in (1.0, -1.0):
        with pytest.raises(AssertionError, match="not the exact integer result"):
            run(c, lambda s: slab(s, sign))


# ------------------------------------------------------------------------------------------------ planted attention faults

NONCAUSAL = kc.Attn16Case("fwd", "bf16", 2, 50, 2, False, None)
CAUSAL = kc.Attn16Case("fwd", "f16", 2, 77, 2, True, None)
TRAIN = kc.Attn16Case("train", "bf16", 3, 33, 2, True, None)


def test_fault_the_last_key_dropped():
    with pytest.raises(AssertionError, match="out: not bit-exact"):
        run_attn(NONCAUSAL, "select", mask_edit=lambda m: m[..., -1].fill_(float("-inf")))


def test_fault_causal_mask_shifted_by_one_on_one_query():
    i = 40                                          # 40 = 1 mod 3: selects itself, key 41 is its copy with another v
    def sees_one_more(m):
        m[..., i, i + 1] = 0.0
    def sees_one_less(m):
        m[..., i, i] = float("-inf")
    for edit in (sees_one_more, sees_one_less):
        with pytest.raises(AssertionError, match="out: not bit-exact"):
            run_attn(CAUSAL, "select", mask_edit=edit)


def test_fault_heads_swapped():
    def swap(s):
        p = s.out.payload
        t = p[:, :64].clone()
        p[:, :64] = p[:, 64:128]
        p[:, 64:128] = t
    with pytest.raises(AssertionError, match="out: not bit-exact"):
        run_attn(NONCAUSAL, "select", swap)


def test_fault_dk_scaled_by_one_plus_two_u():
    """Only a bound can see this (dK of the selection data is zero): the derived bound does — on the keys few queries see, the
    bound is u |dS||q| + u |dK| = 2 u |dK|, and the documented roundings already use part of it."""
    Dm = TRAIN.H * kc.HD
    def scale(s):
        dk = s.dqkv.payload[:, Dm:2 * Dm].float() * (1.0 + 2.0 * s.ty.u)
        s.dqkv.payload[:, Dm:2 * Dm] = dk.to(s.ty.dtype)
    run_attn(TRAIN, "select", scale)
    with pytest.raises(AssertionError, match="dk: error is .* x the derived bound") as e:
        run_attn(TRAIN, "gauss", scale)
    assert "dq:" not in str(e.value).split("(figures")[0] and "dv:" not in str(e.value).split("(figures")[0]


def test_fault_lse_off_by_1e_3():
    with pytest.raises(AssertionError, match="lse: error is"):
        run_attn(TRAIN, "gauss", lambda s: s.lse.payload.add_(1e-3))


def test_fault_the_257th_query_takes_the_row_of_query_256():
    c = kc.Attn16Case("fwd", "bf16", 1, 257, 3, False, None)
    def copy_row(s):
        s.out.payload[256] = s.out.payload[255]
    with pytest.raises(AssertionError, match="out: not bit-exact"):
        run_attn(c, "select", copy_row)


def test_fault_attention_outputs_unwritten_or_overrun():
    with pytest.raises(AssertionError, match=r"out: 64 NaN \(unwritten\?\)"):
        run_attn(NONCAUSAL, "select", lambda s: s.out.payload[49, :64].fill_(kc.NAN))
    with pytest.raises(AssertionError, match="dqkv: memory outside"):
        run_attn(TRAIN, "select", lambda s: s.dqkv.buf.__setitem__(s.dqkv.guard + s.dqkv.rows * s.dqkv.ld, 0))
    with pytest.raises(AssertionError, match="dq: not bit-exact"):
        run_attn(TRAIN, "select", lambda s: s.dqkv.payload.__setitem__((5, 3), 2.0 ** -20))
