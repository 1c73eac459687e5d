"""No GPU: the schedule harness of tests/schedule_checks.py checked on itself.  A stand-in for the engine's
backward (the oracle's own gradients, handed out in the engine's order through `alloc` and `on_ready`) passes every checker on
every mask; every planted fault fails the checker that is relied on for it; the mask list reaches every branch situation and
no mask is idle; the rounded-operand linear layer and its rounding are what DESIGN.md §13 says."""
import pytest
import torch

from dclip_amd import config as dcfg, synth
from oracle import dclip_oracle as O
from tests import schedule_checks as sc

B = 6
T_SHORT = 9


@pytest.fixture(scope="module")
def tiny():
    cfg = dcfg.tiny()
    sd = synth.synth_clip_state_dict(cfg, seed=7, gain=4.0)
    pix = synth.synth_pixel_values(B, cfg.vision, seed=0)
    ids = synth.synth_input_ids(B, cfg.text, seed=3, ragged=True)
    W = sc.output_weighting((B, cfg.projection_dim))
    out = {"cfg": cfg, "sd": sd, "pix": pix, "ids": ids, "W": W}
    for tower, tcfg, x in (("vision", cfg.vision, pix), ("text", cfg.text, ids)):
        r64 = sc.reference(tower, tcfg, sd, x, W)
        r32 = sc.reference(tower, tcfg, sd, x, W, dtype=torch.float32)
        emul = {ty: sc.reference(tower, tcfg, sd, x, W, linear=sc.rounded_linear(ty)) for ty in (torch.bfloat16, torch.float16)}
        out[tower] = {"r64": r64, "r32": r32, "emul": emul, "e_ref32": sc.errors(r32, r64),
                      "e_emul": {ty: sc.errors(emul[ty], r64) for ty in emul}}
    return out


def standin(full, tower, mask, L, on_ready=None, alloc=None, fault=None):
    """The engine's backward contract on ready-made gradients: names() order, None where not needed, gradients written where
    `alloc` says, groups reported tail / layers top down / head.  `fault` plants one bookkeeping error."""
    mask = frozenset(mask)
    got = {n: None for n in sc.names(tower, L)}

    def produce(n):
        val = full[n].float().clone()
        if alloc is not None and fault != "fresh_tensor":
            slot = alloc(n, tuple(val.shape))
            slot.copy_(val)
            if fault == "slice_overrun" and n == "layers.1.out_b":
                slot.as_strided((1,), (1,), slot.storage_offset() + slot.numel()).fill_(1.0)       # one element past the slice's end
            val = slot
        got[n] = val

    def report(group):
        if on_ready is None:
            return
        named = {n: got[n] for n in group if got[n] is not None}
        if fault == "reported_early" and "layers.1.fc1_w" in named:
            got["layers.1.fc1_w"].zero_()                                            # the side stream has not written yet ...
            on_ready(named)
            got["layers.1.fc1_w"].copy_(full["layers.1.fc1_w"].float())              # ... and does after the report
            return
        on_ready(named)
        if fault == "group_twice" and group and group[0].startswith("layers.1."):
            on_ready(named)

    for n in sc.TAIL[tower]:
        if n in mask:
            produce(n)
    report(sc.TAIL[tower])
    low = sc.lowest_of(tower, mask)
    if low is None:
        return got
    run = sc.layers_run(tower, mask, L)
    for i in (reversed(run) if fault == "layers_reversed" else run):
        group = [f"layers.{i}.{f}" for f in sc.LAYER_FIELDS]
        for n in group:
            if n in mask:
                produce(n)
        report(group)
    if low < 0:
        for n in sc.HEAD[tower]:
            if n in mask:
                produce(n)
        report(sc.HEAD[tower])
    if fault == "unneeded_returned":
        got["layers.0.ln1_w"] = full["layers.0.ln1_w"].float().clone()
    if fault == "needed_missing":
        got["layers.1.qkv_b"] = None
    return got


def _sizes(full):
    return {n: t.numel() for n, t in full.items()}


# ------------------------------------------------------------------------------------------------ the reference itself

def test_reference_has_no_zero_tensor_and_its_own_errors_are_small(tiny):
    """The builder asserts |want| > 0 per engine tensor (the k bias alone is zero by softmax's shift invariance; fused into
    qkv_b it is not).  E_ref32 is a few 1e-6; E_emul follows the type's precision: bf16 2^-9, fp16 2^-12 per operand."""
    for tower in ("vision", "text"):
        t = tiny[tower]
        worst32 = max(t["e_ref32"].items(), key=lambda kv: kv[1])
        print(f"{tower}: E_ref32 max {worst32[1]:.2e} ({worst32[0]}); E_emul max bf16 {max(t['e_emul'][torch.bfloat16].values()):.2e}, "
              f"fp16 {max(t['e_emul'][torch.float16].values()):.2e}")
        assert worst32[1] < 1e-4
        assert 1e-4 < max(t["e_emul"][torch.bfloat16].values()) < 0.1
        assert 1e-5 < max(t["e_emul"][torch.float16].values()) < 0.0125
        D = tiny["cfg"].vision.hidden_size
        for i in range(2):
            kb = t["r64"][f"layers.{i}.qkv_b"][D:2 * D]
            assert float(kb.norm()) < 1e-9 * float(t["r64"][f"layers.{i}.qkv_b"].norm())


# ------------------------------------------------------------------------------------------------ the stand-in passes

@pytest.mark.parametrize("tower", ["vision", "text"])
def test_standin_passes_every_checker_on_every_mask(tiny, tower):
    t, L = tiny[tower], 2
    all_names = sc.names(tower, L)
    full32 = standin(t["r32"], tower, all_names, L)
    for gate, got_full, want in ((sc.gates32(t["e_ref32"]), full32, t["r64"]),
                                 (sc.gates16(t["e_emul"][torch.bfloat16]), standin(t["emul"][torch.bfloat16], tower, all_names, L),
                                  t["emul"][torch.bfloat16])):
        for mid, mask in sc.masks(tower, L).items():
            what = f"{tower} {mid}"
            base = standin(got_full, tower, mask, L)
            sc.check_completeness(base, mask, all_names, what)
            sc.check_anchor(base, want, gate, what)
            sc.check_mask_consistency(base, got_full, (), {}, what)
            bucket, log = sc.Bucket(_sizes(want)), sc.ReadyLog()
            got = standin(got_full, tower, mask, L, on_ready=log, alloc=bucket.alloc)
            bucket.check(got, base, what)
            log.check(got, tower, mask, L, what)


# ------------------------------------------------------------------------------------------------ planted faults

def _anchor32(tiny, tower, got, mask=None):
    t = tiny[tower]
    sc.check_anchor(got if mask is None else {n: (g if n in mask else None) for n, g in got.items()}, t["r64"],
                    sc.gates32(t["e_ref32"]), "planted")


def _anchor16(tiny, tower, got, ty):
    t = tiny[tower]
    sc.check_anchor(got, t["emul"][ty], sc.gates16(t["e_emul"][ty]), "planted")


def _plant(tiny, tower, fn):
    """(fp32 stand-in with the fault, bf16 stand-in with it, fp16 ...): fn edits a dict of gradients in place."""
    t = tiny[tower]
    out = []
    for src in (t["r32"], t["emul"][torch.bfloat16], t["emul"][torch.float16]):
        g = {n: v.clone() for n, v in src.items()}
        fn(g)
        out.append(g)
    return out


def _caught_by_all_three_anchors(tiny, tower, fn, name):
    g32, gbf, gfp = _plant(tiny, tower, fn)
    for run in (lambda: _anchor32(tiny, tower, g32), lambda: _anchor16(tiny, tower, gbf, torch.bfloat16),
                lambda: _anchor16(tiny, tower, gfp, torch.float16)):
        with pytest.raises(AssertionError, match=name.replace(".", r"\.")):
            run()


def test_fault_fc2_b_taken_from_the_layer_above(tiny):
    def f(g):
        g["layers.0.fc2_b"] = g["layers.1.fc2_b"].clone()
    _caught_by_all_three_anchors(tiny, "vision", f, "layers.0.fc2_b")


def test_fault_bias_gradient_missing_the_cls_rows(tiny):
    """layers.0.fc2_b is the column sum of d/d(layer 0's output) over all B*S rows; the planted value sums the patch rows only."""
    cfg, sd = tiny["cfg"], tiny["sd"]
    p = {k: v.double() for k, v in sd.items()}
    hidden0 = {}
    saved = O.clip_encoder_layer

    def spy(x, pp, pre, heads, causal, eps):
        y = saved(x, pp, pre, heads, causal, eps)
        if pre.endswith("layers.0"):
            y.retain_grad()
            hidden0["x"] = y
        return y
    for k in p:
        p[k].requires_grad_(True)
    O.clip_encoder_layer = spy
    try:
        out = O.vision_tower(p, tiny["pix"].double(), cfg.vision)
    finally:
        O.clip_encoder_layer = saved
    (out * tiny["W"]).sum().backward()
    d = hidden0["x"].grad                                         # [B, S, D]
    assert sc.rel_err(d.sum((0, 1)), tiny["vision"]["r64"]["layers.0.fc2_b"]) < 1e-12
    wrong = d[:, 1:].sum((0, 1))

    def f(g):
        g["layers.0.fc2_b"] = wrong.to(g["layers.0.fc2_b"].dtype)
    _caught_by_all_three_anchors(tiny, "vision", f, "layers.0.fc2_b")


def test_fault_residual_branch_dropped_from_one_dx(tiny):
    """Layer 1's backward hands down dx without the skip connection's term: every gradient below it is wrong, and the anchor
    names them (the tensors of layer 1 itself stay right)."""
    cfg, sd = tiny["cfg"], tiny["sd"]
    saved = O.clip_encoder_layer

    def no_skip_gradient(x, pp, pre, heads, causal, eps):
        if not pre.endswith("layers.1"):
            return saved(x, pp, pre, heads, causal, eps)
        h = O.layer_norm(x, pp[f"{pre}.layer_norm1.weight"], pp[f"{pre}.layer_norm1.bias"], eps)
        x = x.detach() + O.clip_self_attention(h, pp, f"{pre}.self_attn", heads, causal)      # same values, no gradient through the skip
        h = O.layer_norm(x, pp[f"{pre}.layer_norm2.weight"], pp[f"{pre}.layer_norm2.bias"], eps)
        h = O.quick_gelu(O.linear(h, pp[f"{pre}.mlp.fc1.weight"], pp[f"{pre}.mlp.fc1.bias"]))
        return x + O.linear(h, pp[f"{pre}.mlp.fc2.weight"], pp[f"{pre}.mlp.fc2.bias"])
    O.clip_encoder_layer = no_skip_gradient
    try:
        wrong = sc.reference("vision", cfg.vision, sd, tiny["pix"], tiny["W"], dtype=torch.float32)
    finally:
        O.clip_encoder_layer = saved
    with pytest.raises(AssertionError) as e:
        _anchor32(tiny, "vision", wrong)
    msg = str(e.value)
    assert "layers.0.fc2_b" in msg and "pos:" in msg and "layers.0.qkv_w" in msg
    assert "layers.1.fc2_w" not in msg and "proj_w" not in msg


def test_fault_one_weight_gradient_scaled_by_1_01(tiny):
    """Relied on: the fp32 anchor (1e-2 against gates of a few 1e-5).  The fp16 gate sees it too; bf16's E_emul for this tensor
    is printed — a 1 % scale is within bf16's own rounding noise there, which is why the bookkeeping checks are exact ones."""
    def f(g):
        g["layers.0.fc1_w"] = g["layers.0.fc1_w"] * 1.01
    g32, gbf, gfp = _plant(tiny, "vision", f)
    with pytest.raises(AssertionError, match=r"layers\.0\.fc1_w"):
        _anchor32(tiny, "vision", g32)
    print("4 x E_emul of layers.0.fc1_w: bf16", 4 * tiny["vision"]["e_emul"][torch.bfloat16]["layers.0.fc1_w"],
          "fp16", 4 * tiny["vision"]["e_emul"][torch.float16]["layers.0.fc1_w"])


def test_fault_gradient_returned_for_a_parameter_not_needed(tiny):
    mask = sc.masks("vision", 2)["i_top_layer"]
    got = standin(tiny["vision"]["r32"], "vision", mask, 2, fault="unneeded_returned")
    with pytest.raises(AssertionError, match="not needed.*layers.0.ln1_w"):
        sc.check_completeness(got, mask, sc.names("vision", 2), "planted")


def test_fault_needed_gradient_missing(tiny):
    mask = sc.masks("vision", 2)["i_top_layer"]
    got = standin(tiny["vision"]["r32"], "vision", mask, 2, fault="needed_missing")
    with pytest.raises(AssertionError, match="missing.*layers.1.qkv_b"):
        sc.check_completeness(got, mask, sc.names("vision", 2), "planted")


def test_fault_layers_run_below_lowest():
    mask = sc.masks("vision", 2)["d_top_fc2_b"]
    sc.check_layers_run([1], "vision", mask, 2, "ok")
    with pytest.raises(AssertionError, match="ran for layers"):
        sc.check_layers_run([1, 0], "vision", mask, 2, "planted")


def test_fault_dpos_rows_past_T_not_zero(tiny):
    cfg, sd = tiny["cfg"], tiny["sd"]
    ids = tiny["ids"][:, :T_SHORT].clone()
    ids[:, -1] = cfg.text.eos_token_id
    ref = sc.reference("text", cfg.text, sd, ids, tiny["W"])
    assert ref["pos"].shape[0] == cfg.text.max_position_embeddings > T_SHORT
    sc.check_text_pos_tail(ref["pos"], T_SHORT, "ok")
    wrong = ref["pos"].clone()
    wrong[T_SHORT + 2, 5] = 1e-30                                  # far below any tolerance: the check is exact
    with pytest.raises(AssertionError, match="position gradient"):
        sc.check_text_pos_tail(wrong, T_SHORT, "planted")


def test_fault_class_embedding_taken_from_row_1(tiny):
    def f(g):
        g["class_embedding"] = g["pos"][1].clone()
    _caught_by_all_three_anchors(tiny, "vision", f, "class_embedding")


def test_fault_k_slice_of_qkv_b_filled_with_the_q_slice(tiny):
    D = tiny["cfg"].vision.hidden_size

    def f(g):
        g["layers.1.qkv_b"][D:2 * D] = g["layers.1.qkv_b"][:D]
    _caught_by_all_three_anchors(tiny, "vision", f, "layers.1.qkv_b")


@pytest.mark.parametrize("fault,match", [("slice_overrun", "outside the handed slices.*layers.1.out_b"),
                                         ("fresh_tensor", "never given its slice")])
def test_fault_alloc(tiny, fault, match):
    full = standin(tiny["vision"]["r32"], "vision", sc.names("vision", 2), 2)
    bucket = sc.Bucket(_sizes(full))
    got = standin(full, "vision", sc.names("vision", 2), 2, alloc=bucket.alloc, fault=fault)
    with pytest.raises(AssertionError, match=match):
        bucket.check(got, full, "planted")


def test_fault_alloc_value_differs_or_nan_left(tiny):
    full = standin(tiny["vision"]["r32"], "vision", sc.names("vision", 2), 2)
    for edit, match in ((lambda g: g["layers.0.fc2_w"].view(-1)[7:8].fill_(float("nan")), "NaN left"),
                        (lambda g: g["layers.0.fc2_w"].view(-1)[7:8].mul_(1.0 + 2.0 ** -23), "differs from the run without alloc")):
        bucket = sc.Bucket(_sizes(full))
        got = standin(full, "vision", sc.names("vision", 2), 2, alloc=bucket.alloc)
        edit(got)
        with pytest.raises(AssertionError, match=match):
            bucket.check(got, full, "planted")


@pytest.mark.parametrize("fault,match", [("group_twice", "more than once"), ("reported_early", "before its last write.*|reported before"),
                                         ("layers_reversed", "groups come tail first")])
def test_fault_on_ready(tiny, fault, match):
    full = standin(tiny["vision"]["r32"], "vision", sc.names("vision", 2), 2)
    log = sc.ReadyLog()
    got = standin(full, "vision", sc.names("vision", 2), 2, on_ready=log, fault=fault)
    with pytest.raises(AssertionError, match=match):
        log.check(got, "vision", sc.names("vision", 2), 2, "planted")


def test_fault_mask_consistency_and_its_exception_bound():
    """A gradient that changes with the mask without being a listed exception fails; a listed one holds the column-sum bound
    rows * 2^-24 * sum|x| and fails one ulp-scale step beyond it."""
    rows, D = 300, 8
    x = torch.randn((rows, D), generator=torch.Generator().manual_seed(1))
    s = x.sum(0)
    bound = sc.colsum_bound(rows, x.abs().sum(0))
    other = (s.double() + 0.9 * bound).float()
    full = {"layers.0.fc2_b": s, "layers.0.fc2_w": x}
    sc.check_mask_consistency({"layers.0.fc2_b": other}, full, {"layers.0.fc2_b"}, {"layers.0.fc2_b": bound}, "ok")
    with pytest.raises(AssertionError, match="not bit-equal"):
        sc.check_mask_consistency({"layers.0.fc2_b": other}, full, (), {}, "planted")
    with pytest.raises(AssertionError, match="column-sum bound"):
        sc.check_mask_consistency({"layers.0.fc2_b": (s.double() + 1.5 * bound).float()}, full, {"layers.0.fc2_b"},
                                  {"layers.0.fc2_b": bound}, "planted")
    names2 = sc.names("vision", 2)
    part = sc.masks("vision", 2)["g_biases_ln"]
    assert sc.bias_exceptions(True, part, names2) == frozenset(f"layers.{i}.{l}_b" for i in range(2) for l in sc.LINEARS)
    assert sc.bias_exceptions(False, part, names2) == frozenset()
    assert sc.bias_exceptions(True, names2, names2) == frozenset()
    assert sc.bias_exceptions(True, sc.masks("vision", 2)["i_top_layer"], names2) == frozenset()


# ------------------------------------------------------------------------------------------------ mask coverage

def _all_masks(tower, freeze=None):
    m = {(mid, 2): mk for mid, mk in sc.masks(tower, 2, freeze).items()}
    m.update({(mid, 3): mk for mid, mk in sc.masks(tower, 3).items() if mid != "a_everything"})
    return m


@pytest.fixture(scope="module")
def freeze():
    from dclip_amd.clip_model import HipCLIPModel
    model = HipCLIPModel(dcfg.tiny())
    return {tower: sc.freeze_sets(tower, 2, model) for tower in ("vision", "text")}


@pytest.mark.parametrize("tower", ["vision", "text"])
def test_masks_reach_every_situation(tower, freeze):
    """The list reaches every situation mask_situations can name for the tower, and every mask reaches one that no other
    does: removing any one mask fails here."""
    ms = _all_masks(tower, freeze[tower])
    reach = {k: sc.mask_situations(tower, mk, k[1]) for k, mk in ms.items()}
    union = frozenset().union(*reach.values())
    assert union == sc.situations_of_tower(tower), (sorted(sc.situations_of_tower(tower) - union), sorted(union - sc.situations_of_tower(tower)))
    for k in ms:
        rest = frozenset().union(*(r for kk, r in reach.items() if kk != k))
        assert reach[k] - rest, f"mask {k} reaches nothing the other masks do not: delete it as redundant"
    assert set(sc.situations_of_tower("vision")) | set(sc.situations_of_tower("text")) == set(sc.ALL_SITUATIONS)


def test_freeze_masks_are_the_products_own(freeze):
    """(j): north_star trains the whole vision tower (= mask (a), listed once) and nothing of the text tower; as_written trains
    the vision tower's attention projections and its visual projection, and the whole text tower (= (a) again)."""
    v, t = freeze["vision"], freeze["text"]
    assert v["north_star"] == frozenset(sc.names("vision", 2)) and t["north_star"] == frozenset()
    assert t["as_written"] == frozenset(sc.names("text", 2))
    assert v["as_written"] == frozenset(["proj_w"] + [f"layers.{i}.{f}" for i in range(2) for f in ("qkv_w", "qkv_b", "out_w", "out_b")])
    assert "j_as_written" in sc.masks("vision", 2, v) and "j_north_star" not in sc.masks("vision", 2, v)
    assert not [k for k in sc.masks("text", 2, t) if k.startswith("j_")]


# ------------------------------------------------------------------------------------------------ the rounded-operand linear

@pytest.mark.parametrize("ty", [torch.bfloat16, torch.float16])
def test_round_to_is_the_types_round_to_nearest_even(ty):
    p = 8 if ty == torch.bfloat16 else 11
    x = torch.randn(4096, generator=torch.Generator().manual_seed(2)) * torch.logspace(-6, 3, 4096)
    x = torch.cat([x, torch.tensor([0.0, 1.0, -1.0, 3.0e-6, 6.0e-8, 1.0e-7, 60000.0])])
    assert torch.equal(sc.round_to(x.double(), ty), x.to(ty).double())          # fp32 -> 16 bits is one rounding in torch
    ulp = 2.0 ** (1 - p)                                                        # spacing in [1, 2)
    ties = torch.tensor([1 + 0.5 * ulp, 1 + 1.5 * ulp, 1 + 2.5 * ulp, -(1 + 0.5 * ulp)], dtype=torch.float64)
    assert sc.round_to(ties, ty).tolist() == [1.0, 1 + 2 * ulp, 1 + 2 * ulp, -1.0]            # halves go to the even neighbour
    # a double just above a tie goes up, although its detour through fp32 would land ON the tie and go down to even
    above = torch.tensor([1 + 0.5 * ulp + 2.0 ** -40], dtype=torch.float64)
    assert sc.round_to(above, ty).item() == 1 + ulp
    assert sc.round_to(torch.tensor([1e39, -1e39], dtype=torch.float64), ty).tolist() == [float("inf"), float("-inf")]


@pytest.mark.parametrize("ty", [torch.bfloat16, torch.float16])
def test_rounded_linear_against_a_direct_computation(ty):
    gen = torch.Generator().manual_seed(3)
    x = torch.randn((5, 8), generator=gen, dtype=torch.float64, requires_grad=True)
    w = torch.randn((3, 8), generator=gen, dtype=torch.float64, requires_grad=True)
    b = torch.randn((3,), generator=gen, dtype=torch.float64, requires_grad=True)
    dy = torch.randn((5, 3), generator=gen, dtype=torch.float64)
    r = lambda t: sc.round_to(t, ty)                                # noqa: E731
    y = sc.rounded_linear(ty)(x, w, b)
    y.backward(dy)
    assert torch.equal(y.detach(), r(x.detach()) @ r(w.detach()).t() + b.detach())
    assert torch.equal(x.grad, r(dy) @ r(w.detach()))
    assert torch.equal(w.grad, r(dy).t() @ r(x.detach()))
    assert torch.equal(b.grad, dy.sum(0))
    assert not torch.equal(r(dy), dy)                               # the example does round something
    # a batched input (the oracle's [B, S, D]) and no bias (the projections)
    x3 = torch.randn((2, 5, 8), generator=gen, dtype=torch.float64, requires_grad=True)
    dy3 = torch.randn((2, 5, 3), generator=gen, dtype=torch.float64)
    w.grad = None
    sc.rounded_linear(ty)(x3, w).backward(dy3)
    assert torch.equal(w.grad, r(dy3).reshape(10, 3).t() @ r(x3.detach()).reshape(10, 8))
    assert torch.equal(x3.grad, r(dy3) @ r(w.detach()))


def test_embed_atomic_bound_is_zero_where_nothing_is_summed():
    """A token met once is exact and one never met is zero, whatever the order of the atomics; a shared row gets
    c * 2^-24 * sum|x| — and a difference beyond that fails the consistency check."""
    ids = torch.tensor([[3, 5, 5], [5, 7, 3]])
    dx = torch.randn((6, 4), generator=torch.Generator().manual_seed(4))
    b = sc.embed_atomic_bound(ids, dx, 9)
    assert b.shape == (9, 4) and float(b[[0, 1, 2, 4, 6, 8]].abs().sum()) == 0.0
    assert torch.equal(b[7], 2.0 ** -24 * dx[4].abs().double())
    assert torch.equal(b[5], 3 * 2.0 ** -24 * (dx[1].abs().double() + dx[2].abs().double() + dx[3].abs().double()))
    full = {"tok": torch.zeros((9, 4)).index_add_(0, ids.reshape(-1), dx)}
    other = {"tok": full["tok"].clone()}
    other["tok"][5, 0] += 0.5 * float(b[5, 0])
    sc.check_mask_consistency(other, full, {"tok"}, {"tok": b}, "ok")
    other["tok"][1, 2] = 1e-30                                   # a row no token names
    with pytest.raises(AssertionError, match="column-sum bound"):
        sc.check_mask_consistency(other, full, {"tok"}, {"tok": b}, "planted")


# ------------------------------------------------------------------------------------------------ the single-pass census

V_PRUNED = dict(pruned=True, packed=False, dystats=True, attn_form="stats", wgrad_plan_ok=True)          # vision, tiny B = 64
V_UNPRUNED = dict(V_PRUNED, pruned=False)
V_OFF = dict(V_PRUNED, dystats=False)
T_TWIN = dict(pruned=False, packed=False, dystats=True, attn_form="rows_stats", wgrad_plan_ok=True)     # text, T = 77, B = 64
T_SEG = dict(T_TWIN, attn_form="segments")
T_PACKED = dict(T_TWIN, packed=True, attn_form=None)
T_DECLINED = dict(T_PACKED, wgrad_plan_ok=False)                                                        # 249 rows
T_STALE = dict(T_TWIN, dystats=False, attn_form=None, wgrad_plan_ok=False)
CENSUS_ROUTES = {"v_pruned": ("vision", V_PRUNED), "v_unpruned": ("vision", V_UNPRUNED), "v_off": ("vision", V_OFF), "t_twin": ("text", T_TWIN),
                 "t_seg": ("text", T_SEG), "t_packed": ("text", T_PACKED), "t_declined": ("text", T_DECLINED), "t_stale": ("text", T_STALE)}


def _passes(single=0, three=0, plain_w=0, colsum=0, segments=0):
    return {"single": single, "three": three, "plain_w": plain_w, "colsum": colsum, "segments": segments}


def _split_masks(tower, L):
    m = dict(sc.masks(tower, L))
    m.update(sc.split_masks(tower, L))
    return m


def test_expected_passes_on_hand_worked_masks():
    """Vision, pruned top layer, L = 2 (L = 3 for (k)), the regime on, the plan live.  Layer 1 is last_layer_bwd_cls: only its qkv
    is a full-size linear, and attention_cls_bwd has no statistics form; its fc2 / fc1 / out run at M = B on ops.gemm and are not
    counted, but a bias of theirs without its weight still costs a colsum."""
    m = _split_masks("vision", 2)
    ep = lambda mask, L=2, **kw: sc.expected_passes("vision", mask, L, **dict(V_PRUNED, **kw))        # noqa: E731
    # (a) layer 1: qkv three.  layer 0: fc2 (partials from layer 1's ln1 backward), fc1 (fc2's dgrad), out (ln2 backward), qkv
    #     (attention_bwd.lean.stats): four single passes; every bias comes out of its pass or its GEMM's A_ROWSUM
    assert ep(m["a_everything"]) == _passes(single=4, three=1)
    # (e) layers.0.fc2_b alone: layers 1 and 0 run, no weight anywhere: one colsum, no pass, no producer
    assert ep(m["e_bottom_fc2_b"]) == _passes(colsum=1)
    assert sc.expected_producers("vision", m["e_bottom_fc2_b"], 2, **V_PRUNED) == {}
    # (f) the weights without their biases: the passes of (a), each handed db=None
    assert ep(m["f_weights"]) == _passes(single=4, three=1)
    # (g) every bias, no weight: four colsums per layer (the top layer's three M = B biases included)
    assert ep(m["g_biases_ln"]) == _passes(colsum=8)
    # top layer only: layer 0 is not run; layer 1's qkv three, its ln1 backward is NOT asked (i - 1 < bottom)
    assert ep(m["i_top_layer"]) == _passes(three=1)
    assert sc.expected_producers("vision", m["i_top_layer"], 2, **V_PRUNED) == {}
    # (k) L = 3, the middle layer's fc2_b and out_b: layers 2 and 1 run, two colsums
    assert ep(sc.masks("vision", 3)["k_middle_fc2_b_out_b"], L=3) == _passes(colsum=2)
    # (m) layers.1.fc2_b and layers.0.fc2_w only: layer 1 one colsum (its fc2 at M = B) and its ln1 backward produces for layer 0's
    #     fc2, which takes the single pass without a bias
    assert ep(m["m_top_fc2_b_bottom_fc2_w"]) == _passes(single=1, colsum=1)
    assert sc.expected_producers("vision", m["m_top_fc2_b_bottom_fc2_w"], 2, **V_PRUNED) == {1: {"gemm": 0, "ln": 1, "attn": 0}}
    # (a) again: who produces where — layer 1's ln1 backward for layer 0's fc2; in layer 0 the dgrad, the ln2 backward, the attention
    assert sc.expected_producers("vision", m["a_everything"], 2, **V_PRUNED) == {1: {"gemm": 0, "ln": 1, "attn": 0}, 0: {"gemm": 1, "ln": 1, "attn": 1}}
    # the switch off: the same five passes, all three-launch; L = 3: 4 (L - 1) single and 1 three
    assert ep(m["a_everything"], dystats=False) == _passes(three=5)
    assert sc.expected_passes("vision", sc.names("vision", 3), 3, **V_PRUNED) == _passes(single=8, three=1)
    # unpruned: the top layer is a layer_bwd; its fc2's dY comes from scatter_rows (three), its qkv gets partials too
    assert ep(m["a_everything"], pruned=False) == _passes(single=7, three=1)
    assert ep(m["i_top_layer"], pruned=False) == _passes(single=3, three=1)


def test_expected_passes_of_the_text_routes():
    m = _split_masks("text", 2)
    ep = lambda mask, kw: sc.expected_passes("text", mask, 2, **kw)                                  # noqa: E731
    # the twin: layer 1's fc2 three (scatter_rows), everything else single — 4 L passes, dqkv's L among the single ones
    assert ep(m["a_everything"], T_TWIN) == ep(m["f_weights"], T_TWIN) == _passes(single=7, three=1)
    assert ep(m["g_biases_ln"], T_TWIN) == _passes(colsum=8)
    assert ep(m["i_top_layer"], T_TWIN) == _passes(single=3, three=1)
    # the twin switched off: both qkv three, and ops.colsum_segments where qkv_b is needed beside qkv_w
    assert ep(m["a_everything"], T_SEG) == _passes(single=5, three=3, segments=2)
    assert ep(m["f_weights"], T_SEG) == _passes(single=5, three=3)
    assert ep(m["g_biases_ln"], T_SEG) == _passes(colsum=8)
    # packed: no statistics form for dqkv, no segments either
    assert ep(m["a_everything"], T_PACKED) == _passes(single=5, three=3)
    assert ep(m["m_top_fc2_b_bottom_fc2_w"], T_PACKED) == _passes(single=1, colsum=1)
    # 249 rows / a stale plan: the fp32 GEMMs, a colsum only for a bias without its weight
    for kw in (T_DECLINED, T_STALE):
        assert ep(m["a_everything"], kw) == ep(m["f_weights"], kw) == _passes(plain_w=8)
        assert ep(m["g_biases_ln"], kw) == _passes(colsum=8)
        assert ep(m["e_bottom_fc2_b"], kw) == _passes(colsum=1)
        assert sc.expected_producers("text", m["a_everything"], 2, **kw) == {}


def standin_schedule(tower, mask, L, *, pruned, packed, dystats, attn_form, wgrad_plan_ok, fault=None):
    """The split-fp16 backward walked the way engine._layers_bwd walks it — top down, each producer's decision taken where the
    engine takes it — counting what it would call: (calls, {layer: producers}, [biases written]).  Written on its own, not from
    split_census; `fault` plants one scheduling error."""
    mask = frozenset(mask)
    need = lambda i, f: f"layers.{i}.{f}" in mask                                                    # noqa: E731
    calls, producers, written = _passes(), {}, []
    low = sc.lowest_of(tower, mask)
    if low is None:
        return calls, producers, written
    bottom = max(low, 0)

    def produce(i, kind):
        producers.setdefault(i, {k: 0 for k in sc.PRODUCER_KINDS})[kind] += 1

    def taken(i, l, full=True):
        return need(i, l + "_w") and wgrad_plan_ok and full

    def lpg(i, l, stats, full=True, segments=False):
        w, b = need(i, l + "_w"), need(i, l + "_b")
        if taken(i, l, full):
            if stats and fault != "consumer_ignores_stats":
                calls["single"] += 1
            else:
                calls["three"] += 1
                calls["segments"] += int(b and segments)
            if b or fault == "db_without_need_b":
                written.append(f"layers.{i}.{l}_b")
        elif w:
            calls["plain_w"] += int(full)
            if b:
                written.append(f"layers.{i}.{l}_b")
        elif b:
            calls["colsum"] += 1
            written.append(f"layers.{i}.{l}_b")

    dx_stats = False
    for i in range(L - 1, bottom - 1, -1):
        below = dystats and i - 1 >= (0 if fault == "producer_below_bottom" else bottom)
        dxs = below and (taken(i - 1, "fc2") or (fault in ("stats_for_frozen_weight", "producer_below_bottom") and wgrad_plan_ok))
        cls = pruned and i == L - 1
        lpg(i, "fc2", dx_stats, not cls)
        if cls:
            lpg(i, "fc1", False, False)
            lpg(i, "out", False, False)
            lpg(i, "qkv", False)
        else:
            st = dystats and taken(i, "fc1")
            if st:
                produce(i, "gemm")
            lpg(i, "fc1", st)
            st = dystats and taken(i, "out")
            if st:
                produce(i, "ln")
            lpg(i, "out", st)
            q = dystats and taken(i, "qkv") and not packed
            st = q and attn_form in ("stats", "rows_stats")
            if st:
                produce(i, "attn")
            lpg(i, "qkv", st, segments=q and attn_form == "segments")
        if dxs:
            produce(i, "ln")
        dx_stats = dxs
    return calls, producers, written


@pytest.mark.parametrize("route", sorted(CENSUS_ROUTES))
def test_standin_schedule_agrees_with_the_census_on_every_mask(route):
    tower, kw = CENSUS_ROUTES[route]
    for L in (2, 3):
        for mid, mask in _split_masks(tower, L).items():
            calls, producers, written = standin_schedule(tower, mask, L, **kw)
            sc.check_census(calls, producers, tower, mask, L, f"{route} {mid} L{L}", **kw)
            assert sorted(written) == sorted(n for n in mask if "." in n and n.split(".")[-1] in ("fc2_b", "fc1_b", "out_b", "qkv_b"))
            assert sum(sum(v.values()) for v in producers.values()) == calls["single"]              # nothing produced without a consumer


@pytest.mark.parametrize("fault,tower,kw,mid,match", [
    ("stats_for_frozen_weight", "vision", V_PRUNED, "g_biases_ln", "statistics were produced"),
    ("stats_for_frozen_weight", "text", T_TWIN, "e_bottom_fc2_b", "statistics were produced"),
    ("consumer_ignores_stats", "vision", V_PRUNED, "a_everything", "calls .*the census says"),
    ("consumer_ignores_stats", "text", T_PACKED, "m_top_fc2_b_bottom_fc2_w", "calls .*the census says"),
    ("producer_below_bottom", "vision", V_PRUNED, "i_top_layer", "statistics were produced"),
    ("producer_below_bottom", "text", T_TWIN, "d_top_fc2_b", "statistics were produced")])
def test_fault_census(fault, tower, kw, mid, match):
    mask = _split_masks(tower, 2)[mid]
    calls, producers, _ = standin_schedule(tower, mask, 2, **kw)
    sc.check_census(calls, producers, tower, mask, 2, "ok", **kw)
    calls, producers, _ = standin_schedule(tower, mask, 2, fault=fault, **kw)
    with pytest.raises(AssertionError, match=match):
        sc.check_census(calls, producers, tower, mask, 2, "planted", **kw)


def test_fault_db_written_although_the_bias_is_not_needed(tiny):
    """A split pass that writes db under a mask without the bias (f): the gradient comes back, and completeness names it."""
    mask = sc.masks("vision", 2)["f_weights"]
    _, _, written = standin_schedule("vision", mask, 2, fault="db_without_need_b", **V_PRUNED)
    assert "layers.0.fc2_b" in written and not standin_schedule("vision", mask, 2, **V_PRUNED)[2]
    got = standin(tiny["vision"]["r32"], "vision", mask, 2)
    sc.check_completeness(got, mask, sc.names("vision", 2), "ok")
    for n in written:
        got[n] = tiny["vision"]["r32"][n].float().clone()
    with pytest.raises(AssertionError, match="not needed.*layers.0.fc2_b"):
        sc.check_completeness(got, mask, sc.names("vision", 2), "planted")


def test_fault_fc1_b_finished_from_the_partials_of_dx2(tiny):
    """The finish over a producer's partials handed the wrong ColStats: fc1_b's first D columns are the column sums of dx2 (that is
    fc2_b), the rest is what the buffer held.  The anchor names it under the full mask (all three gates); under a mask without
    fc1_w the bias is a plain colsum of the right tensor, and mask consistency finds the full-mask value far outside the
    column-sum bound of dh."""
    cfg, sd, D = tiny["cfg"], tiny["sd"], tiny["cfg"].vision.hidden_size

    def f(g):
        b = torch.zeros_like(g["layers.0.fc1_b"])
        b[:D] = g["layers.0.fc2_b"]
        g["layers.0.fc1_b"] = b
    _caught_by_all_three_anchors(tiny, "vision", f, "layers.0.fc1_b")
    # |dh| of layer 0, summed per column: dh is the gradient of quick_gelu's input
    seen, saved = [], O.quick_gelu

    def spy(x):
        x.retain_grad()
        seen.append(x)
        return saved(x)
    p = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    O.quick_gelu = spy
    try:
        out = O.vision_tower(p, tiny["pix"].double(), cfg.vision)
    finally:
        O.quick_gelu = saved
    (out * tiny["W"]).sum().backward()
    dh = seen[0].grad.reshape(-1, seen[0].shape[-1])
    assert sc.rel_err(dh.sum(0), tiny["vision"]["r64"]["layers.0.fc1_b"]) < 1e-12
    bound = {"layers.0.fc1_b": sc.colsum_bound(dh.shape[0], dh.abs().sum(0))}
    names2 = sc.names("vision", 2)
    mask = sc.masks("vision", 2)["g_biases_ln"]
    exc = sc.bias_exceptions(True, mask, names2)
    assert "layers.0.fc1_b" in exc
    bounds = {n: (bound[n] if n in bound else torch.full_like(tiny["vision"]["r64"][n], float("inf"))) for n in exc}
    right = standin(tiny["vision"]["r32"], "vision", names2, 2)
    part = standin(tiny["vision"]["r32"], "vision", mask, 2)
    sc.check_mask_consistency(part, right, exc, bounds, "ok")
    wrong = dict(right)
    f(wrong)
    with pytest.raises(AssertionError, match=r"layers\.0\.fc1_b: another launch.*column-sum bound"):
        sc.check_mask_consistency(part, wrong, exc, bounds, "planted")


def test_split_masks_reach_every_split_situation(freeze):
    """masks() + split_masks() reach every situation the split-fp16 backward's own branches create (schedule_checks.SPLIT_SITUATIONS)
    on the routes of §31, and every mask still reaches a situation — of §26's or of these — that no other mask does."""
    reach = {}
    for tower in ("vision", "text"):
        ms = _all_masks(tower, freeze[tower])
        ms.update({(mid, 2): mk for mid, mk in sc.split_masks(tower, 2).items()})
        for k, mk in ms.items():
            r = set(sc.mask_situations(tower, mk, k[1]))
            for route, (t, kw) in CENSUS_ROUTES.items():
                if t == tower:
                    r |= {f"{route}:{s}" for s in sc.split_situations(tower, mk, k[1], **kw)}
            reach[(tower,) + k] = r
    bare = {s.split(":", 1)[1] for r in reach.values() for s in r if ":" in s}
    assert bare == set(sc.SPLIT_SITUATIONS), (sorted(set(sc.SPLIT_SITUATIONS) - bare), sorted(bare - set(sc.SPLIT_SITUATIONS)))
    for tower in ("vision", "text"):
        mine = {k: r for k, r in reach.items() if k[0] == tower}
        for k in mine:
            rest = set().union(*(r for kk, r in mine.items() if kk != k))
            assert mine[k] - rest, f"mask {k} reaches nothing the other masks do not"
    # the situations by name, where they are expected
    v = lambda mid, L=2: sc.split_situations("vision", _split_masks("vision", L)[mid], L, **V_PRUNED)        # noqa: E731
    assert "split.w_only" in v("f_weights") and "split.both" in v("a_everything") and "split.b_only_live_plan" in v("e_bottom_fc2_b")
    assert "producer.consumer_below" in v("a_everything") and "producer.consumer_not_run" in v("i_top_layer")
    assert "producer.consumer_not_run" in v("k_middle_fc2_b_out_b", 3) and "regime_on.nothing_asked" in v("g_biases_ln")
    assert "producer.in_layer_without_split_pass" in v("m_top_fc2_b_bottom_fc2_w")
    t = lambda mid: sc.split_situations("text", _split_masks("text", 2)[mid], 2, **T_SEG)                    # noqa: E731
    assert "segments.with_b" in t("a_everything") and "segments.without_b" in t("f_weights") and "segments.with_b" not in t("f_weights")
