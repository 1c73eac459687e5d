"""CPU-only: the checkers of tests/kernel_checks.py pass on a correct fp32 evaluation of every case the GPU path tests run,
and fail on each of a set of planted faults — the evidence that those tests would notice a subtly wrong kernel."""
import pytest
import torch

from tests import kernel_checks as kc

D = "cpu"


def run(case, fault=None, before=None):
    s = kc.build_gemm(case, D)
    if before:
        before(s)
    kc.emulate_gemm(s)
    if fault:
        fault(s)
    return kc.verify_gemm(s)


def first(pred, cases=None):
    return next(c for c in (cases or kc.integer_matrix()) if pred(c))


# ------------------------------------------------------------------------------------------------ the cases themselves

def test_integer_products_are_exact_in_fp32_at_k_12800():
    M, N, K = 96, 80, 12800
    a, b, acc, _ = kc._operands(M, N, K, "int")
    assert float((a.abs() @ b.abs().t()).max()) < 2 ** 24            # every partial sum in any order is below 2^24
    assert float(a.double().abs().max()) == 2.0
    assert torch.equal((a @ b.t()).double(), acc)
    assert torch.equal(acc, (a.long() @ b.long().t()).double())


def test_the_shape_list_has_every_edge_the_kernels_have():
    shapes = kc.SHAPES
    assert any(m % 64 for m, n, k in shapes) and any(n % 4 == 0 and n % 64 for m, n, k in shapes)
    assert any(k % 32 for m, n, k in shapes) and any(k % 4 for m, n, k in shapes)
    for bm in (64, 128):
        assert {-(-m // bm) % 4 for m, n, k in shapes} >= {1, 2, 3}, bm
    assert any(n <= 64 for m, n, k in shapes)                                   # tiles_n == 1
    assert any((-(-m // 64) * -(-n // 64)) % 8 for m, n, k in shapes)           # a tile count that is not a multiple of 8
    assert -(-kc.MANY_TILES[0] // 64) * -(-kc.MANY_TILES[1] // 64) >= 4000
    m = kc.integer_matrix()
    assert all(n % 4 == 0 and (c.layout & 1 or M % 4 == 0) for c in m for M, n in [(c.M, c.N)])     # nothing to skip
    assert all(c.K <= 12800 and c.alpha in (0.5, 1.0, 2.0) for c in m)
    for tile in kc.TILES:
        for layout in kc.LAYOUTS:
            mine = [c for c in m if c.tile == tile and c.layout == layout]
            assert {c.pads[0] for c in mine} == {c.pads[1] for c in mine} == {c.pads[2] for c in mine} == {0, 4, 36}
            assert {c.M for c in mine if c.epi == 0 and c.split == 1} >= {kc.roundup(s[0], 1 if layout & 1 else 4) for s in shapes}
        for epi in kc.EPILOGUES:
            assert len({kc.expected_splits(c.K, c.split) for c in m if c.tile == tile and c.epi == epi}) >= 3   # effective
            assert {c.split for c in m if c.tile == tile and c.epi == epi} == {1, 2, 3, 7}
        assert 7 in {kc.expected_splits(c.K, c.split) for c in m if c.tile == tile}
        for layout in kc.LAYOUTS:
            for split in (2, 3, 7):
                assert any(c.tile == tile and c.layout == layout and c.split == split and kc.expected_splits(c.K, split) > 1
                           for c in m), (tile, layout, split)
        rs = [c for c in m if c.tile == tile and c.epi & kc.EPI_A_ROWSUM]
        assert {(c.layout, c.split) for c in rs} == {(0, 1), (0, 3), (2, 1), (2, 3)}
    assert len({kc.case_id(c) for c in m}) == len(m)


@pytest.mark.parametrize("tile", kc.TILES + [None], ids=str)
def test_integer_matrix_passes_on_a_correct_fp32_evaluation(tile):
    for c in kc.integer_matrix():
        if c.tile == tile:
            run(c)


def test_gaussian_cases_pass_on_a_correct_fp32_evaluation():
    worst = 0.0
    for c in kc.gaussian_matrix():
        fig = run(c)
        worst = max([worst] + [v for k, v in fig.items() if k.endswith("bound_ratio")])
    assert 0.0 < worst < 0.5            # fp32 BLAS sits well inside the derived bound; the bound is not vacuous either


@pytest.mark.parametrize("cases", [kc.self_cases, kc.cross_cases, lambda: kc.CLS_CASES, lambda: kc.ROW_CASES],
                         ids=["self", "cross", "cls", "row"])
def test_attention_cases_pass_on_a_correct_fp32_evaluation(cases):
    seen = set()
    for c in cases():
        key = c._replace(mode="default") if isinstance(c, kc.SelfCase) else c        # the switches do not exist on the CPU
        if key in seen:
            continue
        seen.add(key)
        s = kc.build_attn(c, D)
        kc.emulate_attn(s)
        fig = kc.verify_attn(s)
        assert all(v < 2e-6 for v in fig.values()), (c, fig)             # >= 10x headroom inside the project's figures
        if isinstance(c, kc.SelfCase) and c.S == 1:
            assert fig["dq"] == 0.0 and fig["dk"] == 0.0                 # the identically-zero blocks
        if isinstance(c, kc.ClsCase):
            assert fig["dq_other_rows"] == 0.0


def test_every_dispatch_branch_of_the_attention_has_a_case():
    names = set()
    for c in list(kc.self_cases()) + list(kc.cross_cases()) + list(kc.CLS_CASES) + list(kc.ROW_CASES):
        names.update(n for n in kc.expected_launches(c) if n)
    assert names == {"attention_fwd.rows", "attention_fwd.stream", "attention_fwd", "attention_bwd.rows", "attention_bwd.lean",
                     "attention_bwd.stream_ds", "attention_bwd.stream", "attention_bwd",
                     "attention_bwd.one_key"}
    kt = {-(-c.S // 16) for c in kc.self_cases() if c.mode == "default" and c.S <= 80}
    assert kt == {1, 2, 3, 4, 5}                                         # every instance of the whole-row forward


# ------------------------------------------------------------------------------------------------ planted faults

BIG = first(lambda c: c.K == 12800)
MID = first(lambda c: (c.M, c.N, c.K) == (300, 256, 128) and c.epi == 0 and c.split == 1 and c.layout == 3)
PADDED = first(lambda c: c.pads[2] == 4 and c.epi == 0 and c.M >= 128)


def test_fault_one_k_element_dropped_at_k_12800():
    def drop(s):
        k = int((s.a[5] * s.b[7]).nonzero()[0])
        s.C.payload[5, 7] -= s.a[5, k] * s.b[7, k]
    with pytest.raises(AssertionError, match="differ from the exact integer result"):
        run(BIG, drop)


def test_fault_two_output_tiles_swapped():
    def swap(s):
        p = s.C.payload
        t = p[0:64, 0:64].clone()
        p[0:64, 0:64] = p[64:128, 64:128]
        p[64:128, 64:128] = t
    with pytest.raises(AssertionError, match="differ"):
        run(MID, swap)


def test_fault_one_tile_transposed_in_place():
    def transpose(s):
        s.C.payload[64:128, 128:192] = s.C.payload[64:128, 128:192].t().clone()
    with pytest.raises(AssertionError, match="differ"):
        run(MID, transpose)


def test_fault_one_tile_left_at_its_stale_but_correct_value():
    """A kernel that never writes one tile: on memory the allocator hands back from the previous, identical call the tile
    still holds the right answer; on the NaN-filled payload it does not."""
    def skip_tile(s, prefill):
        s.C.payload[64:128, 0:64] = prefill
    s = kc.build_gemm(MID, D)
    kc.emulate_gemm(s)
    previous = s.C.get()
    skip_tile(s, previous[64:128, 0:64])
    assert torch.equal(s.C.get().double(), s.acc)                    # the reused block hides the missing tile
    with pytest.raises(AssertionError, match="non-finite"):
        run(MID, lambda t: skip_tile(t, kc.NAN))


def test_fault_one_float_written_into_the_ldc_padding():
    def spill(s):
        s.C.mat[17, PADDED.N] = 1.0
    with pytest.raises(AssertionError, match=r"outside .* was written at \(row, col\) \[\(17, %d\)\]" % PADDED.N):
        run(PADDED, spill)


def test_fault_one_float_written_one_row_past_m():
    def spill(s):
        s.C.buf[s.C.guard + s.C.rows * s.C.ld + 3] = 0x3F800000
    with pytest.raises(AssertionError, match=r"\(%d, 3\)" % MID.M):
        run(MID, spill)
    with pytest.raises(AssertionError, match=r"\(-1, "):             # and one float in front of row 0
        run(MID, lambda s: s.C.buf.__setitem__(s.C.guard - 2, 0))


def test_fault_aux_and_rowsum_are_guarded_too():
    gelu = first(lambda c: c.epi & kc.EPI_GELU and c.pads[2])
    with pytest.raises(AssertionError, match="aux: memory outside"):
        run(gelu, lambda s: s.aux.mat.__setitem__((0, gelu.N + 1), 0.0))
    rs = first(lambda c: c.epi & kc.EPI_A_ROWSUM)
    with pytest.raises(AssertionError, match="rowsum: memory outside"):
        run(rs, lambda s: s.rowsum.buf.__setitem__(s.rowsum.guard + rs.M, 0))


def test_fault_operands_rounded_to_bf16():
    def to_bf16(s):
        s.A.copy_(s.A.bfloat16().float())
        s.B.copy_(s.B.bfloat16().float())
    g = first(lambda c: c.epi == 0 and c.K == 512, kc.gaussian_matrix())
    with pytest.raises(AssertionError, match="x the derived bound"):
        run(g, before=to_bf16)
    run(first(lambda c: c.K == 512 and c.epi == 0), before=to_bf16)      # integers survive bf16: only the bound sees this


def test_fault_padding_read_and_multiplied_by_zero():
    """A kernel that loads the K padding and relies on a zero in the other operand: NaN * 0 = NaN."""
    c = first(lambda c: c.layout == 3 and c.pads[0] and c.K % 4 == 0 and c.epi == 0)
    s = kc.build_gemm(c, D)
    a = torch.nan_to_num(s.A[:c.M, :c.K + 4], nan=kc.NAN)                           # four padding columns come along
    b = torch.cat([s.B[:c.N, :c.K], torch.zeros(c.N, 4)], 1)
    s.C.payload.copy_(a @ b.t())
    with pytest.raises(AssertionError, match="non-finite"):
        kc.verify_gemm(s)


def test_fault_dk_scaled_while_dq_and_dv_are_exact():
    c = kc.SelfCase(2, 50, 2, False, "default")
    s = kc.build_attn(c, D)
    kc.emulate_attn(s)
    s.dqkv.payload[:, 128:256] *= 1.0 + 1e-3
    with pytest.raises(AssertionError, match=r"dk: 1\.0\d*e-03 >= 5\.0e-05") as e:
        kc.verify_attn(s)
    assert "dq:" not in str(e.value).split("(all blocks")[0] and "dv:" not in str(e.value).split("(all blocks")[0]


def test_fault_attention_outputs_unwritten_or_overrun():
    c = kc.CrossCase(2, 8, 75, 1)
    s = kc.build_attn(c, D)
    kc.emulate_attn(s)
    s.lse.payload[0, 3] = kc.NAN                                      # a query row whose lse was never stored
    with pytest.raises(AssertionError, match="lse: 1 non-finite"):
        kc.verify_attn(s)
    s = kc.build_attn(c, D)
    kc.emulate_attn(s)
    s.dkv.buf[s.dkv.guard + s.dkv.rows * s.dkv.ld] = 0                # dK of a key row past Lk
    with pytest.raises(AssertionError, match="dkv: memory outside"):
        kc.verify_attn(s)
    cls = kc.ClsCase(2, 50, 2)
    s = kc.build_attn(cls, D)
    kc.emulate_attn(s)
    s.dqkv.payload[51, 5] = 1e-30                                     # a q gradient in a non-CLS row
    with pytest.raises(AssertionError, match="dq_other_rows: reference is identically zero"):
        kc.verify_attn(s)
