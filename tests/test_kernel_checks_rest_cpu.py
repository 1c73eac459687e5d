"""CPU-only: the checkers of tests/kernel_checks_rest.py pass on a plain PyTorch fp32 evaluation with the
kernels' summation shapes for every case the GPU path tests run — which also shows that the exact constructions are exact in
fp32 and that every derived bound holds with room (worst got / bound ratio below 1) — and fail on each of a set of planted
faults, each caught by the checker that is relied on for it."""
import pytest
import torch

from tests import kernel_checks as kc
from tests import kernel_checks_rest as kr

FAMILIES = {
    "ln_fwd": (lambda: kr.LN_FWD_CASES, kr.build_ln_fwd, kr.emulate_ln_fwd, kr.verify_ln_fwd),
    "ln_bwd": (kr.ln_bwd_cases, kr.build_ln_bwd, kr.emulate_ln_bwd, kr.verify_ln_bwd),
    "colsum": (kr.colsum_cases, kr.build_colsum, kr.emulate_colsum, kr.verify_colsum),
    "rowsum": (kr.rowsum_cases, kr.build_rowsum, kr.emulate_rowsum, kr.verify_rowsum),
    "transpose": (kr.trans_cases, kr.build_trans, kr.emulate_trans, kr.verify_trans),
    "mt_weights": (lambda: kr.MTW_CASES, kr.build_mtw, kr.emulate_mtw, kr.verify_mtw),
    "im2col": (kr.im2col_cases, kr.build_im2col, kr.emulate_im2col, kr.verify_im2col),
    "assemble": (lambda: kr.ASSEMBLE_CASES, kr.build_assemble, kr.emulate_assemble, kr.verify_assemble),
    "text_embed": (lambda: kr.TEXT_CASES, kr.build_text, kr.emulate_text, kr.verify_text),
    "first_eos": (lambda: kr.EOS_CASES, kr.build_eos, kr.emulate_eos, kr.verify_eos),
    "rows": (lambda: kr.ROWS_CASES, kr.build_rows, kr.emulate_rows, kr.verify_rows),
    "normalize": (lambda: kr.NORM_CASES, kr.build_norm, kr.emulate_norm, kr.verify_norm),
    "cosine": (lambda: kr.COS_CASES, kr.build_cos, kr.emulate_cos, kr.verify_cos),
    "sub_reduce": (lambda: kr.SUB_CASES, kr.build_sub, kr.emulate_sub, kr.verify_sub),
    "sumsq": (lambda: kr.SUMSQ_N, kr.build_sumsq, kr.emulate_sumsq, kr.verify_sumsq),
    "clip": (kr.clip_cases, kr.build_clip, kr.emulate_clip, kr.verify_clip),
    "amp": (lambda: kr.AMP_TABLE, kr.build_amp, kr.emulate_amp, kr.verify_amp),
    "mt": (kr.mt_cases, kr.build_mt, kr.emulate_mt, kr.verify_mt),
    "adamw": (kr.adamw_cases, kr.build_adamw, kr.emulate_mt, kr.verify_mt),
}
# the worst got / bound ratio of every bounded quantity on the fp32 emulation (DESIGN.md §18 quotes these)
WORST = {}


def run(family, case, fault=None):
    _, build, emulate, verify = FAMILIES[family]
    s = build(case)
    emulate(s, fault) if fault else emulate(s)
    return verify(s)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_every_case_passes_on_the_fp32_emulation_and_every_bound_has_room(family):
    cases = FAMILIES[family][0]()
    assert len({str(c) for c in cases}) == len(cases), "duplicate cases"
    worst = {}
    for c in cases:
        for k, v in (run(family, c) or {}).items():
            worst[k] = max(worst.get(k, 0.0), v)
    WORST[family] = worst
    print(family, len(cases), "cases; worst got / bound:", {k: round(v, 3) for k, v in worst.items()})
    assert all(v < 1.0 for v in worst.values()), worst


def test_the_exact_layernorm_constructions_are_exact_in_fp32():
    """Both constructions, in a plain fp32 evaluation: dx needs no more than 24 bits and the two row sums of the paired-column
    rows are exactly zero for a D that is no power of two (1 / D is rounded there)."""
    for c in kr.ln_bwd_cases():
        if c.data != "int" or c.rows > 8:
            continue
        s = kr.build_ln_bwd(c)
        xh = (s.x - s.mean[:, None]) * s.rstd[:, None]
        a = s.dy * s.g
        if not kr.ln_bwd_general(c):
            assert float(kr.wave_row_sum(kr.quad(a * xh)).abs().max()) == 0.0 and float(kr.wave_row_sum(kr.quad(a)).abs().max()) == 0.0
            assert float((a * xh).sum(1).abs().max()) == 0.0 and float(a.flip(1).sum(1).abs().max()) == 0.0      # any order
        r = kr.ln_bwd_reference(s)
        assert torch.equal(r.dx.float().double(), r.dx)
        if s.ty is not None and c.res and not kr.ln_bwd_general(c) and c.rows * c.D >= 64:       # the 16-bit copy is a real rounding: some element needs more bits than the type has
            assert not torch.equal(kc.round16(r.dx.float(), s.ty).double(), r.dx)


def first(family, pred):
    return next(c for c in FAMILIES[family][0]() if pred(c))


FAULTS = [
    ("dres_row_skipped", "ln_bwd", lambda c: c.res and c.data == "int" and c.rows == 5, "dx: not exact"),
    ("colsum_accumulated", "ln_bwd", lambda c: c.colsum and c.acc and c.data == "int", "dx_colsum: not exact"),
    ("chunk_unwritten", "ln_fwd", lambda c: c.D == 768, "y: "),
    ("chunk_unwritten", "ln_bwd", lambda c: c.D == 1024 and c.data == "int", "dx: not exact"),
    ("dgamma_dbeta_swapped", "ln_bwd", lambda c: c.params == "both" and c.data == "int" and c.rows > 1, "dgamma: not exact"),
    ("dx16_truncated", "ln_bwd", lambda c: c.entry == "ex" and c.dx16 and c.data == "int" and c.rows >= 4 and c.D >= 256, "dx16: not the rounding"),
    ("uncentred", "ln_fwd", lambda c: c.stats and c.D == 512, "rstd: "),
    ("split_dropped", "colsum", lambda c: c.M == 8193, "out: not exact"),
    ("split_twice", "colsum", lambda c: c.M == 129, "out: not exact"),
    ("padding_unwritten", "transpose", lambda c: c.tpad == 72, "must be zero-filled"),
    ("past_ldyT", "transpose", lambda c: c.rows == 65, "memory outside"),
    ("wrong_tensor_tile", "mt_weights", lambda c: len(c.order) > 1, "not the rounding"),
    ("saturating", "transpose", lambda c: c.ty == "f16ex" and not c.src16 and c.rows * c.cols >= 16, "not the rounding"),
    ("pxpy_swapped", "im2col", lambda c: c.p == 6, "cols: not bit-identical"),
    ("pxpy_swapped", "im2col", lambda c: c.ty == "bf16" and c.p == 8, "cols: not the rounding"),
    ("class_on_patch0", "assemble", lambda c: c.S == 5, "x: not bit-identical"),
    ("last_eos", "first_eos", lambda c: c.B == 9 and c.T == 77, "idx: got"),
    ("unselected_unwritten", "rows", lambda c: c.S == 5, "dx: not bit-identical"),
    ("clamp_projects", "normalize", lambda c: c.B >= 3 and not c.acc, "clamped rows"),
    ("no_cos_term", "cosine", lambda c: c.B >= 5, "ds: "),
    ("bias_step_minus_1", "mt", lambda c: c.entry == "adamw", "p["),
    ("bias_step_minus_1", "mt", lambda c: c.entry == "skip", "p["),
    ("decoupled_in_coupled", "mt", lambda c: c.entry == "adam" and c.wd > 0, "p["),
    ("tail_skipped", "mt", lambda c: c.entry == "adamw", "p["),
    ("tail_skipped", "mt", lambda c: c.entry == "sumsq", "partial: not exact"),
    ("tail_skipped", "sumsq", lambda n: n == 1023, "partial: not exact"),
    ("tail_skipped", "rowsum", lambda c: c.n == 513, "out: not exact"),
    ("chunk_element_twice", "mt", lambda c: c.entry == "adam", "[6] n="),
    ("skip_writes_moments", "mt", lambda c: c.entry == "skip_found_inf", "not bit-identical"),
    ("tracker_not_reset", "amp", lambda r: r[1] + 1 == r[5] and r[2] == 0.0 and r[5] > 1, "torch's rule"),
]


@pytest.mark.parametrize("fault,family,pred,message", FAULTS, ids=[f"{f[1]}-{f[0]}" for f in FAULTS])
def test_each_planted_fault_is_caught_by_the_checker_relied_on(fault, family, pred, message):
    case = first(family, pred)
    run(family, case)                                      # the same case passes without the fault
    with pytest.raises(AssertionError) as e:
        run(family, case, fault)
    assert message in str(e.value), str(e.value)[:600]


def test_the_uncentred_variance_is_seen_by_the_bound_alone():
    """A row with mean 100 x its spread: y and rstd leave their derived bounds, the 1e-5 figure on max|rstd| may not notice."""
    case = first("ln_fwd", lambda c: c.stats and c.D == 512)
    with pytest.raises(AssertionError) as e:
        run("ln_fwd", case, "uncentred")
    assert "rstd: " in str(e.value) and "beyond the bound" in str(e.value)


def test_the_cosine_fault_is_invisible_at_s_equal_t_without_the_absolute_term():
    """Missing cos * shat changes the s = t row by its whole (cancelling) value and the s != t rows by a relative error."""
    case = first("cosine", lambda c: c.B >= 5 and not c.acc)
    with pytest.raises(AssertionError) as e:
        run("cosine", case, "no_cos_term")
    assert "beyond the bound" in str(e.value)
