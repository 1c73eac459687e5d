"""No GPU: the harness of tests/head_checks.py checked on itself.  A stand-in for the product's head (the oracle
evaluated by torch in fp32, wrapped in autograd Functions that keep the product's contracts: `ds * g`, None for the teacher,
need_x, replaced_flag) passes every checker on every case; every planted fault fails the checker that is relied on for it; the
case lists reach every row of the route table; every reference tensor is non-zero (or declared zero) before a GPU sees it."""
import contextlib
import os

import pytest
import torch

from dclip_amd.patch_text_aggregation import CrossModalAttention
from oracle import dclip_oracle as O
from tests import head_checks as hc


# ------------------------------------------------------------------------------------------------ the stand-in

class OracleFn(torch.autograd.Function):
    """fn(*leaves) -> tuple of tensors, evaluated and differentiated by torch in fp32.  kind "loss": the backward is formed
    with upstream 1 and multiplied afterwards (`ds * g`), `grad_to` names the operands that get one; kind "block" / "pool":
    the product's need_x and replaced_flag contracts."""

    @staticmethod
    def forward(ctx, be, fn, kind, grad_to, *xs):
        with torch.enable_grad():
            leaves = [x.detach().float().contiguous().clone().requires_grad_(True) for x in xs]
            outs = fn(*leaves)
        ctx.be, ctx.kind, ctx.grad_to, ctx.leaves, ctx.outs, ctx.calls = be, kind, grad_to, leaves, outs, 0
        res = [o.detach().clone() for o in outs]
        if kind == "pool":
            flag = ~torch.isfinite(res[0]).all()
            if bool(flag):
                res[0] = torch.zeros_like(res[0])
            ctx.replaced_flag = flag
        return tuple(res)

    @staticmethod
    def backward(ctx, *gs):
        be, fault = ctx.be, ctx.be.fault
        ctx.calls += 1
        need = ctx.needs_input_grad[4:]
        if ctx.kind == "loss":
            idx = [i for i in range(len(ctx.leaves)) if need[i] and (i in ctx.grad_to or fault == "teacher_gets_a_gradient")]
            base = torch.autograd.grad(ctx.outs[0], [ctx.leaves[i] for i in idx], retain_graph=True)
            g = gs[0]
            scale = (lambda d: d) if fault == "ds_not_times_g" else (lambda d: d * g * g) if fault == "ds_times_g_twice" else (lambda d: d * g)
            out = [None] * len(ctx.leaves)
            for i, d in zip(idx, base):
                out[i] = scale(d)
            return (None, None, None, None, *out)
        idx = [i for i in range(len(ctx.leaves)) if need[i]]
        flag = getattr(ctx, "replaced_flag", None)
        replaced = flag is not None and bool(flag)
        gs = [torch.zeros_like(g) if (replaced and ctx.kind == "pool") else g.contiguous() for g in gs]
        got = torch.autograd.grad(ctx.outs, [ctx.leaves[i] for i in idx], gs, retain_graph=True, allow_unused=True)
        out = [None] * len(ctx.leaves)
        for i, d in zip(idx, got):
            out[i] = torch.zeros_like(ctx.leaves[i]) if d is None else d
            if replaced and fault != "guard3_zeroes_d_out_only":
                out[i] = torch.zeros_like(out[i])
        if ctx.kind == "block":
            be.log(hc.block_routes(ctx.T, ctx.R)[2:])
            if fault == "need_x_one_ulp" and (need[0] or need[1]):
                out[2] = torch.nextafter(out[2], torch.full_like(out[2], float("inf")))
            if fault == "second_backward_one_ulp" and ctx.calls == 2:
                out[5] = torch.nextafter(out[5], torch.full_like(out[5], float("inf")))
        return (None, None, None, None, *out)


class StandinBlock(CrossModalAttention):
    """The product's parameter holder (same names and order) around the oracle."""

    def forward(self, text, patches):
        be, H = self.be, self.num_heads

        def fn(t, p, *params):
            return O.cross_modal_attention(dict(zip(hc.PARAMS, params)), t, p, H)
        at, ai = OracleFn.apply(be, fn, "block", None, text, patches, *self._params())
        if at.grad_fn is not None:
            at.grad_fn.T, at.grad_fn.R = text.shape[1], patches.shape[1]
        be.log(hc.block_routes(text.shape[1], patches.shape[1], backward=False))
        return at, ai


class StandinTeacher:
    def __init__(self, be, cfg, clip_sd, cm_sd):
        self.be, self.cfg, self.sd = be, cfg, clip_sd
        self.cross_modal_attention = be.block(cfg.projection_dim, cfg.projection_dim // 64, cm_sd)
        self.last_sentence_embedding = None

    def compute_global_embedding_tensors(self, regions, ids, counts=None, max_tokens=None):
        B, R = regions.shape[:2]
        with torch.no_grad():
            emb = O.vision_tower(self.sd, regions.reshape(B * R, *regions.shape[2:]), self.cfg.vision).view(B, R, -1)
            if counts is not None:
                rmax = max(int(counts.max()), 1)
                if self.be.fault != "padded_region_row_leaks":
                    keep = torch.arange(R)[None, :, None] < counts.long()[:, None, None]
                    emb = torch.where(keep, emb, torch.zeros_like(emb))          # mask_rows: before the guard, NaN rows included
                emb = emb[:, :rmax].contiguous()
            tokens, _n, sent = O.teacher_token_embeddings(self.sd, ids, self.cfg.text)
            if max_tokens is not None and max_tokens > tokens.shape[1]:
                tokens = torch.cat([tokens, tokens.new_zeros(B, max_tokens - tokens.shape[1], tokens.shape[2])], dim=1)
        self.last_sentence_embedding = sent
        return self.be.global_from_tokens(self.cross_modal_attention, tokens, emb)


class Standin:
    device = torch.device("cpu")

    def __init__(self, fault=None):
        self.fault = fault
        self._log = None

    def log(self, names):
        if self._log is not None:
            if self.fault == "wrong_launch_name":
                names = ["attention_bwd.lean" if n == "attention_bwd.stream" else n for n in names]
            self._log += names

    @contextlib.contextmanager
    def watch(self):
        self._log = []
        try:
            yield self._log
        finally:
            self._log = None

    def cosine(self, s, t):
        return OracleFn.apply(self, lambda a, b: (O.cosine_distillation_loss(a, b),), "loss", (0,), s, t)[0]

    def contrastive(self, i, t, temperature):
        return OracleFn.apply(self, lambda a, b: (O.contrastive_loss(a, b, temperature),), "loss", (0, 1), i, t)[0]

    def distill_losses(self, si, st, ti, tt, temperature):
        l_img, l_txt, l_con = self.cosine(si, ti), self.cosine(st, tt), self.contrastive(si, st, temperature)
        return {"loss": l_img + l_txt + 1.0 * l_con, "loss_image": l_img, "loss_text": l_txt, "loss_contrastive": l_con}

    def bridge(self, student_dim, teacher_dim):
        class Bridge(torch.nn.Module):
            def __init__(self):
                super().__init__()
                self.register_buffer("weight", O.bridge_weight(student_dim, teacher_dim))

            @torch.no_grad()
            def forward(self, t):
                return O.linear(t.float(), self.weight)
        return Bridge()

    def block(self, E, H, sd):
        b = StandinBlock(E, H)
        b.load_state_dict(sd)
        b.be = self
        return b

    def pool(self, at, ai, temperature):
        side = 1.0 if self.fault == "mix_on_one_side_only" else 0.5
        return OracleFn.apply(self, lambda a, b: (0.5 * hc.aggregation_ref(a, temperature) + side * hc.aggregation_ref(b, temperature),),
                              "pool", None, at, ai)[0]

    def aggregation(self, x, temperature):
        return OracleFn.apply(self, lambda a: (hc.aggregation_ref(a, temperature),), "agg", None, x)[0]

    def global_from_tokens(self, block, text, patches):
        if not (text.requires_grad or patches.requires_grad):
            text, patches = text.detach().clone(), patches.detach().clone()
            row_ok = torch.isfinite(patches).all(dim=-1, keepdim=True)
            if self.fault == "guard1_zeroes_the_whole_image":
                row_ok = row_ok.all(dim=1, keepdim=True).expand_as(row_ok)
            patches = torch.where(row_ok, patches, torch.zeros_like(patches))
            cap_ok = torch.isfinite(text).flatten(1).all(dim=1).view(-1, 1, 1)
            text = torch.where(cap_ok, text, torch.zeros_like(text))
        at, ai = block(text, patches)
        out = self.pool(at, ai, 2.0)
        if out.grad_fn is not None and at.grad_fn is not None:
            at.grad_fn.replaced_flag = out.grad_fn.replaced_flag
        return out

    def teacher(self, cfg, clip_sd, cm_sd, packed_text):
        return StandinTeacher(self, cfg, clip_sd, cm_sd)


@pytest.fixture(scope="module")
def be():
    return Standin()


def show(what, ref, ratios):
    n32 = max(ref.e_ref32, key=ref.e_ref32.get)
    n, r = hc.worst(ratios)
    print(f"{what}: E_ref32 max {ref.e_ref32[n32]:.2e} ({n32}); worst E/gate {r:.3f} ({n})")


# ------------------------------------------------------------------------------------------------ the stand-in passes

@pytest.mark.parametrize("kind", ["cosine", "contrastive"])
@pytest.mark.parametrize("c", hc.LOSS_CASES, ids=lambda c: c.id)
def test_standin_loss_cases(be, kind, c):
    show(f"{kind} {c.id}", hc.loss_ref(kind, c), hc.check_loss_case(be, kind, c))


@pytest.mark.parametrize("kind", ["cosine", "contrastive"])
@pytest.mark.parametrize("cid", ["6x64", "33x512", "6x768to512.bridge"])
def test_standin_loss_linearity(be, kind, cid):
    c = hc.LOSS_BY_ID[cid]
    hc.check_linearity(lambda g: hc.run_loss(be, kind, c, g), hc.loss_ref(kind, c), f"{kind} {cid}")


def test_standin_teacher_operand_bridge_and_shared_operand(be):
    hc.check_teacher_operand(be, hc.LOSS_BY_ID["6x64"])
    hc.check_bridge(be, hc.LOSS_BY_ID["6x768to512.bridge"])
    for cid in ("6x64", "33x512"):
        c = hc.LOSS_BY_ID[cid]
        show(f"distill_losses {cid}", hc.distill_ref(c), hc.check_shared_operand(be, c))
    hc.check_linearity(lambda g: hc.run_distill(be, hc.LOSS_BY_ID["6x64"], g), hc.distill_ref(hc.LOSS_BY_ID["6x64"]), "distill_losses 6x64")


@pytest.mark.parametrize("c", hc.BLOCK_CASES, ids=lambda c: c.id)
def test_standin_block_cases(be, c):
    show(f"block {c.id}", hc.block_ref(c), hc.check_block_case(be, c))


@pytest.mark.parametrize("cid", ["ragged", "square", "one_key"])
def test_standin_block_exact_checkers(be, cid):
    c = hc.BLOCK_BY_ID[cid]
    hc.check_linearity(lambda g: hc.run_block(be, c, g)[0], hc.block_ref(c), f"block {cid}")
    hc.check_need_x(be, c)
    for frozen in hc.FROZEN_SETS.values():
        hc.check_frozen(be, c, frozen)
    hc.check_repeatability(be, c)


@pytest.mark.parametrize("kind", ["global", "agg"])
@pytest.mark.parametrize("c", hc.POOL_CASES, ids=lambda c: c.id)
def test_standin_pool_cases(be, kind, c):
    show(f"{kind} pool {c.id}", hc.pool_ref(kind, c), hc.check_pool_case(be, kind, c))
    hc.check_linearity(lambda g: hc.run_pool(be, kind, c, g), hc.pool_ref(kind, c), f"{kind} pool {c.id}")


@pytest.mark.parametrize("cid", ["ragged", "square"])
def test_standin_guards(be, cid):
    c = hc.BLOCK_BY_ID[cid]
    hc.check_guards_1_2(be, c)
    hc.check_guard_3(be, c)


@pytest.mark.parametrize("c", hc.GLUE_CASES, ids=lambda c: c.id)
def test_standin_glue_cases(be, c):
    show(f"glue {c.id}", hc.glue_ref(c), hc.check_glue_case(be, c))


def test_standin_row_independence(be):
    hc.check_row_independence(be, hc.GLUE_BY_ID["counts_3_1_0_2"])


def test_trainer_filter_leaves_exactly_the_blocks_12_tensors():
    from dclip_amd import config as dcfg
    from dclip_amd.clip_model import HipCLIPModel
    from dclip_amd.patch_text_aggregation import PatchTextAggregation
    cfg = dcfg.tiny()
    teacher = PatchTextAggregation(embed_dim=cfg.projection_dim, num_heads=1, clip_model=HipCLIPModel(cfg))
    hc.check_trainer_filter(teacher)


# ------------------------------------------------------------------------------------------------ the case lists

def test_cases_reach_every_row_of_the_route_table():
    """Every (forward, backward) pair of the table is reached by a block case in one direction at least, the glue reaches the
    one-key and the tiled rows, and the equal-length rows hold for 1 x 1 (whole-row forward, one-key backward) too."""
    reached = {}
    for c in hc.BLOCK_CASES:
        for pair in (hc.route(c.T, c.R), hc.route(c.R, c.T)):
            reached.setdefault(pair, []).append(c.id)
    for row, pair in hc.ROUTE_TABLE.items():
        assert pair in reached, f"no block case reaches: {row}"
    assert ("attention_fwd.rows", "attention_bwd.one_key") in reached                    # 1 x 1
    assert hc.route(70, 70) == ("attention_fwd.rows", "attention_bwd.stream") and hc.route(81, 81)[0] == "attention_fwd.stream"
    glue = {hc.route(*hc.glue_shapes(c)) for c in hc.GLUE_CASES}
    assert ("attention_fwd", "attention_bwd.one_key") in glue and ("attention_fwd", "attention_bwd") in glue
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(hc.__file__))), "dclip_amd", "csrc", "attention.hip")) as f:
        text = f.read()
    for pair in reached:
        for name in pair:
            assert f'DCLIP_CHECK_LAUNCH("{name}")' in text, f"attention.hip reports no launch site {name}"


def test_every_reference_tensor_is_nonzero_or_declared_zero():
    """Building a Ref asserts |want| > 0 per tensor (or exact zero where the case declares it); all of them are built here."""
    n = 0
    for c in hc.LOSS_CASES:
        for kind in ("cosine", "contrastive"):
            n += len(hc.loss_ref(kind, c).want)
    for c in (hc.LOSS_BY_ID["6x64"], hc.LOSS_BY_ID["33x512"]):
        n += len(hc.distill_ref(c).want)
    for c in hc.BLOCK_CASES:
        assert set(hc.block_ref(c).want) == set(hc.BLOCK_TENSORS)
        n += len(hc.block_ref(c).want)
    for c in hc.POOL_CASES:
        n += len(hc.pool_ref("global", c).want) + len(hc.pool_ref("agg", c).want)
    for c in hc.GLUE_CASES:
        r = hc.glue_ref(c)
        assert set(r.want) == set(hc.GLUE_NAMES)
        assert (len(r.zero) == 1) == (c.id == "counts_all_zero")
        n += len(r.want)
    base, longer = hc.glue_ref(hc.GLUE_BY_ID["counts_3_1_0_2"]), hc.glue_ref(hc.GLUE_BY_ID["max_tokens_plus_3"])
    assert hc.rel_err(longer.want["out.global"], base.want["out.global"]) > 1e-3, "three more zero token rows do not change the result"
    for cid in ("ragged", "square"):
        n += len(hc.global_ref(hc.BLOCK_BY_ID[cid]).want) + len(hc.global_ref(hc.BLOCK_BY_ID[cid], 0, (1, hc.BLOCK_BY_ID[cid].R - 1)).want)
    print(n, "reference tensors")
    assert hc.loss_ref("contrastive", hc.LOSS_BY_ID["1x64"]).absolute and hc.loss_ref("cosine", hc.LOSS_BY_ID["2x64.identical"]).absolute


# ------------------------------------------------------------------------------------------------ planted faults

RAGGED, SQUARE = hc.BLOCK_BY_ID["ragged"], hc.BLOCK_BY_ID["square"]


def _block_fault(c, edit, name):
    """`edit(got)` changes the stand-in's results; the anchor must name `name`."""
    got, _ = hc.run_block(Standin(), c)
    edit(got)
    with pytest.raises(AssertionError, match=name.replace(".", r"\.")):
        hc.anchor(got, hc.block_ref(c), "planted")


def test_fault_weight_gradient_scaled_by_1_01():
    for c in (RAGGED, hc.BLOCK_BY_ID["c3_width"]):
        for n in hc.D_PARAMS:
            def f(g, n=n):
                g[n] = g[n] * 1.01
            _block_fault(c, f, n)
    got = hc.run_loss(Standin(), "cosine", hc.LOSS_BY_ID["33x512"])
    got["d.student"] = got["d.student"] * 1.01
    with pytest.raises(AssertionError, match="d.student"):
        hc.anchor(got, hc.loss_ref("cosine", hc.LOSS_BY_ID["33x512"]), "planted")


def test_fault_k_third_of_in_proj_bias_filled_with_the_q_third():
    E = RAGGED.E

    def f(g):
        b = g["d.text_to_image.in_proj_bias"].clone()
        b[E:2 * E] = b[:E]
        g["d.text_to_image.in_proj_bias"] = b
    _block_fault(RAGGED, f, "d.text_to_image.in_proj_bias")


def _spied_block(c):
    """The fp64 oracle with the intermediate gradients the planted values need: per direction the outputs of its q, k, v
    projections and the input of its LayerNorm, each with its gradient."""
    d = hc.block_data(c)
    lin, ln = [], []
    saved_linear, saved_ln = O.linear, O.layer_norm

    def spy_linear(x, w, b=None):
        y = saved_linear(x, w, b)
        y.retain_grad()
        lin.append(y)
        return y

    def spy_ln(x, w, b, eps=1e-5):
        x.retain_grad()
        ln.append(x)
        return saved_ln(x, w, b, eps)
    O.linear, O.layer_norm = spy_linear, spy_ln
    try:
        p = {k: v.double().requires_grad_(True) for k, v in d["sd"].items()}
        t, q = d["text"].double().requires_grad_(True), d["patches"].double().requires_grad_(True)
        at, ai = O.cross_modal_attention(p, t, q, c.H)
    finally:
        O.linear, O.layer_norm = saved_linear, saved_ln
    ((at * d["Wt"]).sum() + (ai * d["Wi"]).sum()).backward()
    assert len(lin) == 8 and len(ln) == 2             # q, k, v, out of text <- patches, then of patches <- text
    return {"p": p, "text": t, "patches": q, "t2i": lin[:4], "i2t": lin[4:], "pre_t": ln[0], "pre_i": ln[1]}


def test_fault_kv_weight_gradient_written_from_xq():
    """d_in_w[E:] = dkv^T xkv; the planted value multiplies by xq (the square case, where the shapes allow it)."""
    c, E = SQUARE, SQUARE.E
    s = _spied_block(c)
    dk, dv = s["t2i"][1].grad.reshape(-1, E), s["t2i"][2].grad.reshape(-1, E)
    right = torch.cat([dk.t() @ s["patches"].detach().reshape(-1, E), dv.t() @ s["patches"].detach().reshape(-1, E)])
    assert hc.rel_err(right, s["p"]["text_to_image.in_proj_weight"].grad[E:]) < 1e-12
    wrong = torch.cat([dk.t() @ s["text"].detach().reshape(-1, E), dv.t() @ s["text"].detach().reshape(-1, E)])

    def f(g):
        w = g["d.text_to_image.in_proj_weight"].clone()
        w[E:] = wrong.float()
        g["d.text_to_image.in_proj_weight"] = w
    _block_fault(c, f, "d.text_to_image.in_proj_weight")


def test_fault_residual_term_dropped_from_dxq():
    s = _spied_block(RAGGED)

    def f(g):
        g["d.text"] = (g["d.text"].double() - s["pre_t"].grad).float()
    _block_fault(RAGGED, f, "d.text")


def test_fault_d_text_missing_the_other_directions_dxkv():
    c, E = RAGGED, RAGGED.E
    s = _spied_block(c)
    W = s["p"]["image_to_text.in_proj_weight"].detach()
    dxkv_i = s["i2t"][1].grad @ W[E:2 * E] + s["i2t"][2].grad @ W[2 * E:]
    dxq_t = s["t2i"][0].grad @ s["p"]["text_to_image.in_proj_weight"].detach()[:E] + s["pre_t"].grad
    assert hc.rel_err(dxq_t + dxkv_i, s["text"].grad) < 1e-12

    def f(g):
        g["d.text"] = (g["d.text"].double() - dxkv_i).float()
    _block_fault(c, f, "d.text")


def test_fault_mix_applied_to_one_side_only():
    c = hc.POOL_BY_ID["L33.identical_rows"]
    with pytest.raises(AssertionError, match="out.pooled"):
        hc.check_pool_case(Standin("mix_on_one_side_only"), "global", c)
    with pytest.raises(AssertionError, match="0.5"):
        hc.check_pool_case(Standin("mix_on_one_side_only"), "global", hc.POOL_BY_ID["L1"])


@pytest.mark.parametrize("fault", ["ds_not_times_g", "ds_times_g_twice"])
def test_fault_upstream_gradient(fault):
    """Both pass at g = 1, so only linearity can see them."""
    be, c = Standin(fault), hc.LOSS_BY_ID["6x64"]
    for kind in ("cosine", "contrastive"):
        hc.check_loss_case(be, kind, c)
        with pytest.raises(AssertionError, match="is not g times the g=1 gradient"):
            hc.check_linearity(lambda g: hc.run_loss(be, kind, c, g), hc.loss_ref(kind, c), "planted")
    with pytest.raises(AssertionError, match="is not g times the g=1 gradient"):
        hc.check_linearity(lambda g: hc.run_distill(be, c, g), hc.distill_ref(c), "planted")


def test_fault_gradient_returned_for_the_teacher_operand():
    with pytest.raises(AssertionError, match="returned for the teacher operand"):
        hc.check_teacher_operand(Standin("teacher_gets_a_gradient"), hc.LOSS_BY_ID["6x64"])
    with pytest.raises(AssertionError, match="a teacher target received a gradient"):
        hc.run_distill(Standin("teacher_gets_a_gradient"), hc.LOSS_BY_ID["6x64"])


def test_fault_parameter_gradients_one_ulp_off_with_need_x_on():
    hc.check_block_case(Standin("need_x_one_ulp"), RAGGED)                   # invisible to the gate
    with pytest.raises(AssertionError, match="not bit-equal: d.text_to_image.in_proj_weight"):
        hc.check_need_x(Standin("need_x_one_ulp"), RAGGED)


def test_fault_padded_region_row_leaks():
    with pytest.raises(AssertionError, match="at or beyond region_counts leaks"):
        hc.check_row_independence(Standin("padded_region_row_leaks"), hc.GLUE_BY_ID["counts_3_1_0_2"])


def test_fault_guard3_zeroes_d_out_only():
    with pytest.raises(AssertionError, match="NaN reached d"):
        hc.check_guard_3(Standin("guard3_zeroes_d_out_only"), RAGGED)


def test_fault_guard1_zeroes_the_whole_image():
    with pytest.raises(AssertionError, match="zeroing exactly one region row"):
        hc.check_guards_1_2(Standin("guard1_zeroes_the_whole_image"), RAGGED)


def test_fault_gradient_present_for_a_frozen_parameter(monkeypatch):
    real = hc.run_block

    def leaky(be, c, *a, frozen=(), **k):
        got, names = real(be, c, *a, frozen=frozen, **k)
        if frozen:
            got["d." + frozen[0]] = torch.zeros(1)
        return got, names
    monkeypatch.setattr(hc, "run_block", leaky)
    with pytest.raises(AssertionError, match="present for a frozen parameter"):
        hc.check_frozen(Standin(), RAGGED, hc.FROZEN_SETS["both_layernorms"])


def test_fault_second_backward_one_ulp_off():
    with pytest.raises(AssertionError, match="the second backward over the same graph"):
        hc.check_repeatability(Standin("second_backward_one_ulp"), RAGGED)


def test_fault_wrong_launch_name():
    with pytest.raises(AssertionError, match="the cross-attention calls reported"):
        hc.check_block_case(Standin("wrong_launch_name"), SQUARE)
    with pytest.raises(AssertionError, match="the cross-attention calls reported"):
        hc.check_routes(["attention_fwd", "attention_fwd", "attention_bwd", "attention_bwd"], 9, 1, "planted")
