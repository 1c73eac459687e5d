"""Cases, references and checkers for the layer ABOVE the towers: the two loss Functions and `distill_losses`,
`TeacherBridge`, `CrossModalFn`, `GlobalPoolFn` / `AggregationFn`, and the glue of `PatchTextAggregation`.  Importable without
a GPU.  The GPU file (test_head_grads_gpu.py) runs the product through these, the CPU file (test_head_checks_cpu.py) runs a
stand-in (the oracle in torch fp32) and planted faults through the same checkers.

  backend     every runner takes a `be` object presenting the product's interface: `device`, `cosine(s, t)`,
              `contrastive(i, t, temperature)`, `distill_losses(si, st, ti, tt, temperature)`, `bridge(student_dim, teacher_dim)`,
              `block(E, H, state_dict)`, `pool(at, ai, temperature)`, `aggregation(x, temperature)`,
              `global_from_tokens(block, text, patches)`, `teacher(cfg, clip_sd, cm_sd, packed_text)` and `watch()`, a context
              manager yielding the list of launch names of the cross-attention calls made inside it;
  reference   oracle/dclip_oracle.py, every input and parameter in fp64, torch autograd; objective the loss itself, or
              (out * W).sum() with a seeded Gaussian W;
  anchor      E = |got - want|_2 / |want|_2 per tensor, no tensor left out, gate 8 * E_ref32 + 16 * 2^-24 (§26's, unchanged),
              E_ref32 = the same oracle evaluated by torch in fp32;
  exact       linearity in the upstream gradient, need_x, frozen subsets, the teacher operand, the shared operand, row
              independence of the padding, the three guards, the launch route, repeatability.
Names: "out.*" are values, "d.*" gradients (they scale with the upstream gradient)."""
from __future__ import annotations

import functools
from collections import namedtuple
from typing import Callable, Dict, Iterable, List, Optional, Sequence

import torch

from dclip_amd import config as dcfg, synth
from oracle import dclip_oracle as O
from tests.schedule_checks import FLOOR32, M32, output_weighting, rel_err

PARAMS = ("text_to_image.in_proj_weight", "text_to_image.in_proj_bias", "text_to_image.out_proj.weight", "text_to_image.out_proj.bias",
          "image_to_text.in_proj_weight", "image_to_text.in_proj_bias", "image_to_text.out_proj.weight", "image_to_text.out_proj.bias",
          "norm_text.weight", "norm_text.bias", "norm_image.weight", "norm_image.bias")
D_PARAMS = tuple("d." + n for n in PARAMS)
NAN = float("nan")


# ------------------------------------------------------------------------------------------------ reference and anchor

class Ref:
    """want (fp64), the fp32 oracle's own error and the gate per tensor, from `evaluate(dtype) -> {name: tensor}`.
    `absolute`: {name: scale} for tensors whose reference value is zero (or a rounding of zero): they are compared as
    |got - want|_2 <= 16 * 2^-24 * scale, the scale being the size of the terms that cancel (stated at the case)."""

    def __init__(self, evaluate: Callable, absolute: Optional[Dict[str, float]] = None, what: str = "", zero: Iterable[str] = ()):
        """`zero`: tensors that are exactly zero by construction (stated at the case); the reference must say so in both
        types and the code under test must return exact zeros."""
        self.what = what
        self.zero = frozenset(zero)
        self.want = {n: t.detach().double().cpu() for n, t in evaluate(torch.float64).items()}
        self.r32 = {n: t.detach().double().cpu() for n, t in evaluate(torch.float32).items()}
        self.absolute = dict(absolute or {})
        self.e_ref32, self.gate = {}, {}
        for n, w in self.want.items():
            assert bool(torch.isfinite(w).all()), f"{what}: the reference of {n} is not finite"
            if n in self.zero:
                assert not bool((w != 0).any()) and not bool((self.r32[n] != 0).any()), f"{what}: {n} is declared zero and is not"
                self.e_ref32[n] = self.gate[n] = 0.0
                continue
            if n in self.absolute:
                self.e_ref32[n] = float((self.r32[n] - w).norm())
                self.gate[n] = FLOOR32 * self.absolute[n]
                continue
            assert float(w.norm()) > 0.0, f"{what}: the reference of {n} is zero: E is undefined for it"
            self.e_ref32[n] = rel_err(self.r32[n], w)
            self.gate[n] = M32 * self.e_ref32[n] + FLOOR32


def err_of(got: torch.Tensor, want: torch.Tensor, absolute: bool) -> float:
    got = got.detach().reshape(-1).double()
    want = want.detach().reshape(-1).double().to(got.device)
    assert got.shape == want.shape, (got.shape, want.shape)
    d = float((got - want).norm())
    return d if absolute else d / float(want.norm())


def anchor(got: Dict[str, Optional[torch.Tensor]], ref: Ref, what: str, scale: float = 1.0,
           absent: Iterable[str] = ()) -> Dict[str, float]:
    """Every tensor of the reference against `got` ("d.*" scaled by the upstream gradient `scale`); a tensor may be missing
    only if `absent` names it.  Returns {name: E / gate}; one AssertionError names every failure."""
    absent = frozenset(absent)
    ratios, bad = {}, []
    for n, w in ref.want.items():
        g = got.get(n)
        if n in absent:
            assert g is None, f"{what}: {n} exists although nothing asked for it"
            continue
        assert g is not None, f"{what}: {n} is missing"
        if n in ref.zero:
            ratios[n] = 0.0
            if bool((g != 0).any()):
                bad.append(f"{n}: not exactly zero")
            continue
        s = scale if n.startswith("d.") else 1.0
        e = err_of(g, w * s, n in ref.absolute)
        gate = ref.gate[n] * (abs(s) if n in ref.absolute else 1.0)
        ratios[n] = e / gate
        if not e <= gate:
            bad.append(f"{n}: E {e:.3e} > gate {gate:.3e}")
    assert not bad, f"{what}: " + "; ".join(bad)
    return ratios


def bit_equal(a: Dict[str, Optional[torch.Tensor]], b: Dict[str, Optional[torch.Tensor]], names: Iterable[str], what: str):
    bad = []
    for n in names:
        x, y = a.get(n), b.get(n)
        assert x is not None and y is not None, f"{what}: {n} is missing"
        if not torch.equal(x.detach().reshape(-1), y.detach().reshape(-1).to(x.device)):
            bad.append(f"{n} (max |diff| {float((x.double().reshape(-1) - y.double().reshape(-1).to(x.device)).abs().max()):.3e})")
    assert not bad, f"{what}: not bit-equal: " + "; ".join(bad)


def worst(ratios: Dict[str, float]):
    n = max(ratios, key=ratios.get)
    return n, ratios[n]


def put(x: torch.Tensor, device) -> torch.Tensor:
    """A fresh copy on `device`: the cached case data is never handed out (on the CPU .to() would return the tensor itself)."""
    return x.detach().clone().to(device)


def _randn(shape, seed, dtype=torch.float32):
    return torch.randn(tuple(shape), generator=torch.Generator().manual_seed(seed), dtype=dtype)


# ------------------------------------------------------------------------------------------------ loss head

LossCase = namedtuple("LossCase", "id B P temperature variant")
LOSS_CASES = (
    LossCase("1x64", 1, 64, 0.05, "plain"),
    LossCase("2x64", 2, 64, 0.05, "plain"),
    LossCase("2x64.identical", 2, 64, 0.05, "identical"),          # student identical to teacher: the cosine loss is 0
    LossCase("6x64", 6, 64, 0.05, "plain"),
    LossCase("6x64.t1", 6, 64, 1.0, "plain"),
    LossCase("6x64.zero_row", 6, 64, 0.05, "zero_row"),
    LossCase("6x64.noncontig", 6, 64, 0.05, "noncontig"),
    LossCase("6x64.bf16", 6, 64, 0.05, "bf16"),
    LossCase("6x64.fp16", 6, 64, 0.05, "fp16"),
    LossCase("33x512", 33, 512, 0.05, "plain"),
    LossCase("6x768to512.bridge", 6, 512, 0.05, "bridge"),
)
LOSS_BY_ID = {c.id: c for c in LOSS_CASES}
TYPED = {"bf16": torch.bfloat16, "fp16": torch.float16}
BRIDGE_FROM = 768


@functools.lru_cache(maxsize=None)
def loss_data(c: LossCase):
    """(student [B,P], teacher [B,P] or [B,768] before the bridge), fp32 values.  From 6 rows on: rows 0 and 1 of the student
    identical, row 2 of the student equal to its teacher row, row 3 of norm 1e4, row 4 of norm 1e-4."""
    s = _randn((c.B, c.P), 100 + c.B + c.P)
    t = _randn((c.B, BRIDGE_FROM if c.variant == "bridge" else c.P), 200 + c.B + c.P)
    if c.B >= 6 and c.variant != "bridge":
        s[1] = s[0]
        s[2] = t[2]
    if c.B >= 6:
        s[3] *= 1e4 / s[3].norm()
        s[4] *= 1e-4 / s[4].norm()
    if c.variant == "zero_row":
        s[5] = 0.0
    if c.variant == "identical":
        s = t.clone()
    if c.variant in TYPED:
        s = s.to(TYPED[c.variant]).float()
    return s, t


def _loss_eval(kind: str, c: LossCase):
    s, t = loss_data(c)

    def evaluate(dtype):
        sd = s.to(dtype).clone().requires_grad_(True)
        td = t.to(dtype)
        if c.variant == "bridge":
            td = O.linear(td, O.bridge_weight(c.P, BRIDGE_FROM).to(dtype))
        td = td.detach().requires_grad_(True)
        loss = O.cosine_distillation_loss(sd, td) if kind == "cosine" else O.contrastive_loss(sd, td, c.temperature)
        loss.backward()
        out = {"out.loss": loss, "d.student": sd.grad}
        if kind == "contrastive":
            out["d.text"] = td.grad
        return out
    return evaluate


@functools.lru_cache(maxsize=None)
def loss_ref(kind: str, c: LossCase) -> Ref:
    s, t = loss_data(c)
    absolute = None
    if kind == "cosine" and c.variant == "identical":
        # loss = mean(1 - cos) with cos = 1: compared absolutely as the issue says; the gradient's rows are
        # (that - cos shat) / (B |s|), two unit vectors that cancel: scale = |(1 / (B |s_b|))_b|_2
        absolute = {"out.loss": 1.0, "d.student": float((1.0 / (c.B * s.double().norm(dim=1))).norm())}
    if kind == "contrastive" and c.variant == "identical":
        # every positive logit is 1/T = 20 and the negatives lie far below: the loss, 2e-8, is the difference lse - z_bb of two
        # numbers of size 1/T that the kernels form by two routes (the similarity GEMM, a row dot product), each with its own
        # roundings of 2^-24 relative; the oracle in fp32 returns 0 for it.  So: absolute, on the scale 1/T of its terms
        absolute = {"out.loss": 1.0 / c.temperature}
    if kind == "contrastive" and c.B == 1:
        # one pair: lse = z, the loss is exactly 0; the gradient is (1/T) (p - 1) that / |x| with p = 1
        absolute = {"out.loss": 1.0, "d.student": float(1.0 / c.temperature / s.double().norm()),
                    "d.text": float(1.0 / c.temperature / t.double().norm())}
    return Ref(_loss_eval(kind, c), absolute, f"{kind} {c.id}")


def run_loss(be, kind: str, c: LossCase, g: float = 1.0, form: str = "case", teacher_grad: bool = False):
    """One forward and backward of a loss Function under upstream gradient g.  form "case": the operand as the variant says
    (a column slice of a wider tensor, a 16-bit tensor); "plain": the same values, contiguous fp32."""
    s, t = loss_data(c)
    dev = be.device
    extra = {}
    if form == "case" and c.variant == "noncontig":
        wide = torch.full((c.B, c.P + 7), 3.0)
        wide[:, 3:3 + c.P] = s
        wide = put(wide, dev).requires_grad_(True)
        s_in, leaf = wide[:, 3:3 + c.P], wide
        assert not s_in.is_contiguous()
    elif form == "case" and c.variant in TYPED:
        leaf = put(s.to(TYPED[c.variant]), dev).requires_grad_(True)
        s_in = leaf
    else:
        leaf = put(s, dev).requires_grad_(True)
        s_in = leaf
    t_in = put(t, dev)
    if c.variant == "bridge":
        bridge = be.bridge(c.P, BRIDGE_FROM)
        t_in = bridge(t_in)
        assert not t_in.requires_grad and t_in.grad_fn is None, "the bridge's output carries a graph"
        extra["bridge"] = bridge
    if kind == "contrastive" or teacher_grad:
        t_in = t_in.detach().requires_grad_(True)
    loss = be.cosine(s_in, t_in) if kind == "cosine" else be.contrastive(s_in, t_in, c.temperature)
    loss.backward(torch.tensor(g, dtype=loss.dtype, device=loss.device))
    got = {"out.loss": loss.detach(), "d.student": leaf.grad, "teacher.grad": t_in.grad, **extra}
    if form == "case" and c.variant == "noncontig":
        got["d.student"] = leaf.grad[:, 3:3 + c.P]
        rest = torch.cat([leaf.grad[:, :3], leaf.grad[:, 3 + c.P:]], dim=1)
        assert not bool((rest != 0).any()), f"{kind} {c.id}: a gradient was written outside the column slice"
    if kind == "contrastive":
        got["d.text"] = t_in.grad
    return got


def check_loss_case(be, kind: str, c: LossCase) -> Dict[str, float]:
    what = f"{kind} {c.id}"
    ref = loss_ref(kind, c)
    names = [n for n in ref.want if n.startswith("d.")]
    if c.variant in ("noncontig",) + tuple(TYPED):
        # the Fns call .float() / .contiguous(): the same values give the same bits, whatever the operand's layout or type;
        # autograd rounds the gradient once to a 16-bit operand's type
        plain = run_loss(be, kind, c, form="plain")
        ratios = anchor(plain, ref, what)
        got = run_loss(be, kind, c)
        bit_equal(got, plain, ["out.loss"], what)
        for n in names:
            want = plain[n].to(TYPED[c.variant]) if (c.variant in TYPED and n == "d.student") else plain[n]
            assert got[n].dtype == want.dtype and torch.equal(got[n], want), f"{what}: {n} differs from the contiguous fp32 operand's"
        return ratios
    got = run_loss(be, kind, c)
    for n in ["out.loss"] + names:
        assert bool(torch.isfinite(got[n]).all()), f"{what}: {n} is not finite"
    return anchor(got, ref, what)


POW2 = (2.0 ** 16, 2.0 ** -3)            # what the fp16 student's loss scaler sends
THIRD = 1.0 / 3.0


def check_linearity(run: Callable[[float], Dict[str, torch.Tensor]], ref: Ref, what: str, names: Optional[Sequence[str]] = None):
    """Every gradient under upstream g = 2^16 and 2^-3 is g times the g = 1 gradient bit for bit, the value does not move;
    g = 1/3 is held against the gate."""
    names = [n for n in ref.want if n.startswith("d.")] if names is None else list(names)
    base = run(1.0)
    for g in POW2:
        got = run(g)
        bit_equal(got, base, [n for n in ref.want if n.startswith("out.")], f"{what} g={g}")
        bit_equal(got, {n: base[n] * g for n in names}, names, f"{what}: upstream g={g} is not g times the g=1 gradient")
    return anchor(run(THIRD), ref, f"{what} g=1/3", scale=THIRD)


def check_teacher_operand(be, c: LossCase):
    """A teacher that requires a gradient gets none from the cosine loss, and the student's is unchanged by asking."""
    base = run_loss(be, "cosine", c)
    got = run_loss(be, "cosine", c, teacher_grad=True)
    assert got["teacher.grad"] is None, f"cosine {c.id}: a gradient was returned for the teacher operand"
    bit_equal(got, base, ["out.loss", "d.student"], f"cosine {c.id} with a teacher that requires a gradient")


def check_bridge(be, c: LossCase):
    got = run_loss(be, "cosine", c)
    bridge = got["bridge"]
    assert list(bridge.parameters()) == [], "the bridge has a Parameter: AdamW would see it"
    assert "weight" in dict(bridge.named_buffers()) and bridge.weight.grad is None and not bridge.weight.requires_grad
    assert torch.equal(bridge.weight.detach().cpu(), O.bridge_weight(c.P, BRIDGE_FROM)), "the bridge is not the oracle's matrix"


# ---- distill_losses: student_image feeds two loss nodes

@functools.lru_cache(maxsize=None)
def distill_data(c: LossCase):
    s_img, t_img = loss_data(c)
    return s_img, _randn((c.B, c.P), 300 + c.B), t_img, _randn((c.B, c.P), 400 + c.B)


@functools.lru_cache(maxsize=None)
def distill_ref(c: LossCase) -> Ref:
    si, st, ti, tt = distill_data(c)

    def evaluate(dtype):
        a, b = si.to(dtype).clone().requires_grad_(True), st.to(dtype).clone().requires_grad_(True)
        l_img = O.cosine_distillation_loss(a, ti.to(dtype))
        l_txt = O.cosine_distillation_loss(b, tt.to(dtype))
        l_con = O.contrastive_loss(a, b, c.temperature)
        d_cos, = torch.autograd.grad(l_img, a, retain_graph=True)
        d_con, = torch.autograd.grad(l_con, a, retain_graph=True)
        loss = l_img + l_txt + 1.0 * l_con
        loss.backward()
        return {"out.loss": loss, "out.loss_image": l_img, "out.loss_text": l_txt, "out.loss_contrastive": l_con,
                "d.student_image": a.grad, "d.student_text": b.grad, "d.image.cosine_branch": d_cos, "d.image.contrastive_branch": d_con}
    return Ref(evaluate, None, f"distill_losses {c.id}")


def run_distill(be, c: LossCase, g: float = 1.0):
    si, st, ti, tt = (put(x, be.device) for x in distill_data(c))
    a, b = si.clone().requires_grad_(True), st.clone().requires_grad_(True)
    ti, tt = ti.requires_grad_(True), tt.requires_grad_(True)
    out = be.distill_losses(a, b, ti, tt, c.temperature)
    assert torch.equal(out["loss"].detach(), (out["loss_image"] + out["loss_text"] + out["loss_contrastive"]).detach()), \
        "loss is not loss_image + loss_text + loss_contrastive bit for bit"
    out["loss"].backward(torch.tensor(g, dtype=out["loss"].dtype, device=out["loss"].device))
    assert ti.grad is None and tt.grad is None, "distill_losses: a teacher target received a gradient"
    a2 = si.clone().requires_grad_(True)
    be.cosine(a2, ti.detach()).backward(torch.tensor(g, device=be.device))
    a3, b3 = si.clone().requires_grad_(True), st.clone().requires_grad_(True)
    be.contrastive(a3, b3, c.temperature).backward(torch.tensor(g, device=be.device))
    got = {"out." + k: v.detach() for k, v in out.items()}
    got.update({"d.student_image": a.grad, "d.student_text": b.grad, "d.image.cosine_branch": a2.grad, "d.image.contrastive_branch": a3.grad})
    return got


def check_shared_operand(be, c: LossCase) -> Dict[str, float]:
    got = run_distill(be, c)
    both = got["d.image.cosine_branch"] + got["d.image.contrastive_branch"]
    assert torch.equal(got["d.student_image"], both), \
        f"distill_losses {c.id}: student_image.grad is not the sum of its two branches " \
        f"(max |diff| {float((got['d.student_image'] - both).abs().max()):.3e})"
    return anchor(got, distill_ref(c), f"distill_losses {c.id}")


# ------------------------------------------------------------------------------------------------ attention routes

ROUTE_TABLE = {                       # the issue's table, as (forward, backward) names of attention.hip's launch_fwd / launch_bwd
    "Lq == Lk <= 80: whole-row forward, streamed backward": ("attention_fwd.rows", "attention_bwd.stream"),
    "Lk == 1: general forward, one-key backward": ("attention_fwd", "attention_bwd.one_key"),
    "everything else: the tiled pair": ("attention_fwd", "attention_bwd"),
}


def route(Lq: int, Lk: int):
    """(forward, backward) launch names of one cross-attention direction, read off launch_fwd / launch_bwd: the forward asks
    Lq == Lk first (so 1 x 1 takes the whole-row kernel), the backward asks Lk == 1 first; with q at row stride E and kv at 2E
    (lddq != lddkv) an equal-length backward passes the rows and lean kernels by and takes the streamed pair."""
    fwd = ("attention_fwd.rows" if Lk <= 80 else "attention_fwd.stream") if Lq == Lk else "attention_fwd"
    bwd = "attention_bwd.one_key" if Lk == 1 else ("attention_bwd.stream" if Lq == Lk else "attention_bwd")
    return fwd, bwd


def block_routes(T: int, R: int, backward: bool = True) -> List[str]:
    """The names in call order: text <- patches forward, patches <- text forward, then the two backwards in that order."""
    (f1, b1), (f2, b2) = route(T, R), route(R, T)
    return [f1, f2] + ([b1, b2] if backward else [])


# ------------------------------------------------------------------------------------------------ cross-modal block

BlockCase = namedtuple("BlockCase", "id E H B T R")
BLOCK_CASES = (
    BlockCase("ragged", 128, 2, 3, 7, 4),
    BlockCase("square", 128, 2, 2, 5, 5),
    BlockCase("one_key", 64, 1, 3, 9, 1),
    BlockCase("1x1", 64, 1, 2, 1, 1),
    BlockCase("over_a_tile", 128, 2, 2, 75, 33),
    BlockCase("square_70", 64, 1, 2, 70, 70),
    BlockCase("c3_width", 512, 8, 2, 7, 3),
)
BLOCK_BY_ID = {c.id: c for c in BLOCK_CASES}
BLOCK_TENSORS = ("out.at", "out.ai", "d.text", "d.patch") + D_PARAMS


@functools.lru_cache(maxsize=None)
def block_data(c: BlockCase):
    seed = 1000 + 7 * c.E + 31 * c.T + c.R
    sd = synth.synth_cross_modal_state_dict(c.E, seed=seed)
    return {"sd": sd, "text": _randn((c.B, c.T, c.E), seed + 1), "patches": _randn((c.B, c.R, c.E), seed + 2),
            "Wt": output_weighting((c.B, c.T, c.E), seed + 3), "Wi": output_weighting((c.B, c.R, c.E), seed + 4)}


def block_eval(c: BlockCase, d=None):
    d = block_data(c) if d is None else d

    def evaluate(dtype):
        p = {k: v.to(dtype).clone().requires_grad_(True) for k, v in d["sd"].items()}
        t, q = d["text"].to(dtype).clone().requires_grad_(True), d["patches"].to(dtype).clone().requires_grad_(True)
        at, ai = O.cross_modal_attention(p, t, q, c.H)
        ((at * d["Wt"].to(dtype)).sum() + (ai * d["Wi"].to(dtype)).sum()).backward()
        out = {"out.at": at, "out.ai": ai, "d.text": t.grad, "d.patch": q.grad}
        out.update({"d." + n: p[n].grad for n in PARAMS})
        return out
    return evaluate


@functools.lru_cache(maxsize=None)
def block_ref(c: BlockCase) -> Ref:
    return Ref(block_eval(c), None, f"block {c.id}")


def params_of(block) -> Dict[str, torch.Tensor]:
    p = dict(block.named_parameters())
    assert tuple(p) == PARAMS, tuple(p)
    return p


def run_block(be, c: BlockCase, g: float = 1.0, text_rg: bool = True, patch_rg: bool = True, frozen: Iterable[str] = (),
              backwards: int = 1, d=None):
    """(results, launch names).  `backwards` = 2: two backward passes over one graph (retain_graph), results of the second
    under "second.*"."""
    d = block_data(c) if d is None else d
    dev = be.device
    block = be.block(c.E, c.H, d["sd"])
    p = params_of(block)
    for n in frozen:
        p[n].requires_grad_(False)
    t = put(d["text"], dev).requires_grad_(text_rg)
    q = put(d["patches"], dev).requires_grad_(patch_rg)
    with be.watch() as names:
        at, ai = block(t, q)
        obj = (at * d["Wt"].float().to(dev)).sum() + (ai * d["Wi"].float().to(dev)).sum()
        leaves = [x for x in [t, q] + list(p.values()) if x.requires_grad]
        got = {"out.at": at.detach(), "out.ai": ai.detach()}
        if leaves:
            up = torch.tensor(g, dtype=obj.dtype, device=dev)
            if backwards == 1:
                obj.backward(up)
                grads = {id(x): x.grad for x in leaves}
            else:
                first = torch.autograd.grad(obj, leaves, up, retain_graph=True)
                second = torch.autograd.grad(obj, leaves, up, retain_graph=True)
                grads = {id(x): v for x, v in zip(leaves, first)}
                again = {id(x): v for x, v in zip(leaves, second)}
    for n, x in (("d.text", t), ("d.patch", q)) + tuple(("d." + k, v) for k, v in p.items()):
        got[n] = grads.get(id(x)) if leaves else None
        if backwards == 2:
            got["second." + n] = again.get(id(x))
    return got, list(names)


def check_block_case(be, c: BlockCase) -> Dict[str, float]:
    what = f"block {c.id}"
    got, names = run_block(be, c)
    ratios = anchor(got, block_ref(c), what)
    check_routes(names, c.T, c.R, what)
    E = c.E
    for direction, Lk in (("text_to_image", c.R), ("image_to_text", c.T)):
        if Lk != 1:
            continue                    # a single key: softmax of one, so nothing reaches q and k
        for n in (f"d.{direction}.in_proj_weight", f"d.{direction}.in_proj_bias"):
            assert not bool((got[n][:2 * E] != 0).any()), f"{what}: the q / k thirds of {n} are not exactly zero with one key"
            assert bool((got[n][2 * E:] != 0).any()), f"{what}: the v third of {n} is zero"
    return ratios


def check_routes(names: Sequence[str], T: int, R: int, what: str, backward: bool = True):
    want = block_routes(T, R, backward)
    assert list(names) == want, f"{what}: the cross-attention calls reported {list(names)}, the dispatch for T={T}, R={R} is {want}"


def check_need_x(be, c: BlockCase):
    """The 12 parameter gradients are bit-equal whether text / patches ask for a gradient or not; d_text / d_patch exist
    exactly when asked for."""
    what = f"block {c.id}"
    base, _ = run_block(be, c, text_rg=False, patch_rg=False)               # the teacher trainer's case
    assert base["d.text"] is None and base["d.patch"] is None
    anchor(base, block_ref(c), what + " need_x off", absent=("d.text", "d.patch"))
    for trg, prg in ((True, True), (True, False), (False, True)):
        got, _ = run_block(be, c, text_rg=trg, patch_rg=prg)
        w = f"{what} text.requires_grad={trg} patches.requires_grad={prg}"
        assert (got["d.text"] is not None) == trg and (got["d.patch"] is not None) == prg, f"{w}: input gradients exist where not asked, or are missing"
        bit_equal(got, base, D_PARAMS, w + " against neither")
        anchor(got, block_ref(c), w, absent=[n for n, on in (("d.text", trg), ("d.patch", prg)) if not on])


FROZEN_SETS = {"one_direction": tuple(n for n in PARAMS if n.startswith("image_to_text.")),
               "both_layernorms": tuple(n for n in PARAMS if n.startswith("norm_"))}


def check_frozen(be, c: BlockCase, frozen: Sequence[str]):
    """`.grad is None` exactly on the frozen parameters, every other gradient bit-equal to the all-trainable run."""
    what = f"block {c.id} frozen {sorted(frozen)}"
    base, _ = run_block(be, c)
    got, _ = run_block(be, c, frozen=frozen)
    extra = [n for n in frozen if got["d." + n] is not None]
    assert not extra, f"{what}: a gradient is present for a frozen parameter: {extra}"
    rest = [n for n in BLOCK_TENSORS if n.startswith("d.") and n[2:] not in frozen]
    missing = [n for n in rest if got[n] is None]
    assert not missing, f"{what}: missing {missing}"
    bit_equal(got, base, rest, what)


def check_repeatability(be, c: BlockCase):
    got, _ = run_block(be, c, backwards=2)
    names = [n for n in BLOCK_TENSORS if n.startswith("d.")]
    bit_equal({n: got["second." + n] for n in names}, got, names, f"block {c.id}: the second backward over the same graph")
    anchor(got, block_ref(c), f"block {c.id} first of two backwards")


# ------------------------------------------------------------------------------------------------ pooling

PoolCase = namedtuple("PoolCase", "id B Lt Li E special")
POOL_CASES = (
    PoolCase("L1", 3, 1, 1, 128, ""),
    PoolCase("L2.zero_row", 3, 2, 2, 128, "zero_row"),
    PoolCase("L33.identical_rows", 3, 33, 5, 128, "identical"),
    PoolCase("L96.zero_row", 2, 96, 96, 64, "zero_row"),
)
POOL_BY_ID = {c.id: c for c in POOL_CASES}
POOL_T = 2.0


def aggregation_ref(x: torch.Tensor, temperature: float) -> torch.Tensor:
    """O.aggregation with vector_norm in place of sqrt(sum): the same value (asserted where the references are built), and an
    all-zero row back-propagates the clamp's zero subgradient where sqrt's derivative gives 0 * inf."""
    m = x.mean(dim=1, keepdim=True)
    nx = torch.clamp(torch.linalg.vector_norm(x, dim=-1), min=1e-8)
    nm = torch.clamp(torch.linalg.vector_norm(m, dim=-1), min=1e-8)
    w = O.softmax_lastdim((x * m).sum(-1) / (nx * nm) / temperature)
    return (x * w.unsqueeze(-1)).sum(dim=1)


@functools.lru_cache(maxsize=None)
def pool_data(c: PoolCase):
    seed = 2000 + 3 * c.Lt + c.Li
    at, ai = _randn((c.B, c.Lt, c.E), seed) * 1.5 + 0.3, _randn((c.B, c.Li, c.E), seed + 1) * 1.5 + 0.3
    if c.special == "zero_row":
        at[1, c.Lt // 2] = 0.0
        ai[0, c.Li - 1] = 0.0
    if c.special == "identical":
        at[1, 7] = at[1, 20]
        ai[2, 0] = ai[2, 4]
    return {"at": at, "ai": ai, "W": output_weighting((c.B, c.E), seed + 2)}


@functools.lru_cache(maxsize=None)
def pool_ref(kind: str, c: PoolCase) -> Ref:
    d = pool_data(c)

    def evaluate(dtype):
        a, b = d["at"].to(dtype).clone().requires_grad_(True), d["ai"].to(dtype).clone().requires_grad_(True)
        if kind == "global":
            out = 0.5 * aggregation_ref(a, POOL_T) + 0.5 * aggregation_ref(b, POOL_T)
        else:
            out = aggregation_ref(a, POOL_T)
        if dtype == torch.float64:
            theirs = 0.5 * O.aggregation(a, POOL_T) + 0.5 * O.aggregation(b, POOL_T) if kind == "global" else O.aggregation(a, POOL_T)
            assert rel_err(out, theirs.detach()) < 1e-14, "aggregation_ref is not the oracle's aggregation"
        (out * d["W"].to(dtype)).sum().backward()
        res = {"out.pooled": out, "d.at": a.grad}
        if kind == "global":
            res["d.ai"] = b.grad
        return res
    return Ref(evaluate, None, f"{kind} pool {c.id}")


def run_pool(be, kind: str, c: PoolCase, g: float = 1.0):
    d = pool_data(c)
    dev = be.device
    a, b = put(d["at"], dev).requires_grad_(True), put(d["ai"], dev).requires_grad_(True)
    out = be.pool(a, b, POOL_T) if kind == "global" else be.aggregation(a, POOL_T)
    W = d["W"].float().to(dev)
    (out * W).sum().backward(torch.tensor(g, device=dev))
    got = {"out.pooled": out.detach(), "d.at": a.grad, "x.W": W, "x.at": a.detach(), "x.ai": b.detach()}
    if kind == "global":
        got["d.ai"] = b.grad
    return got


def check_pool_case(be, kind: str, c: PoolCase) -> Dict[str, float]:
    what = f"{kind} pool {c.id}"
    got = run_pool(be, kind, c)
    if c.Lt == 1 and c.Li == 1:                            # w = 1, out = x, dx = out_scale * d_out: bit for bit
        if kind == "global":
            assert torch.equal(got["out.pooled"], 0.5 * got["x.at"][:, 0] + 0.5 * got["x.ai"][:, 0]), f"{what}: out is not 0.5 at + 0.5 ai"
            assert torch.equal(got["d.at"][:, 0], 0.5 * got["x.W"]) and torch.equal(got["d.ai"][:, 0], 0.5 * got["x.W"]), \
                f"{what}: dx is not 0.5 d_out on both sides"
        else:
            assert torch.equal(got["out.pooled"], got["x.at"][:, 0]) and torch.equal(got["d.at"][:, 0], got["x.W"]), f"{what}: out = x, dx = d_out"
    return anchor(got, pool_ref(kind, c), what)


# ------------------------------------------------------------------------------------------------ tokens -> global: the guards

@functools.lru_cache(maxsize=None)
def global_ref(c: BlockCase, zero_caption: int = -1, zero_region=(-1, -1)) -> Ref:
    """O.global_embedding on the blocks as given (rows already zeroed where a guard would), objective (global * W).sum()."""
    d = block_data(c)
    text, patches = d["text"].clone(), d["patches"].clone()
    if zero_caption >= 0:
        text[zero_caption] = 0.0
    if zero_region[0] >= 0:
        patches[zero_region[0], zero_region[1]] = 0.0
    W = output_weighting((c.B, c.E), 77)

    def evaluate(dtype):
        p = {k: v.to(dtype).clone().requires_grad_(True) for k, v in d["sd"].items()}
        out = O.global_embedding(p, text.to(dtype), patches.to(dtype), c.H)
        (out * W.to(dtype)).sum().backward()
        res = {"out.global": out}
        res.update({"d." + n: p[n].grad for n in PARAMS})
        return res
    return Ref(evaluate, None, f"global {c.id}")


def run_global(be, c: BlockCase, text: torch.Tensor, patches: torch.Tensor, block=None, sd=None, inputs_rg: bool = False):
    d = block_data(c)
    dev = be.device
    block = be.block(c.E, c.H, d["sd"] if sd is None else sd) if block is None else block
    p = params_of(block)
    for x in p.values():
        x.grad = None
    t, q = put(text, dev).requires_grad_(inputs_rg), put(patches, dev).requires_grad_(inputs_rg)
    with be.watch() as names:
        out = be.global_from_tokens(block, t, q)
        (out * output_weighting((c.B, c.E), 77).float().to(dev)).sum().backward()
    got = {"out.global": out.detach(), "d.text": t.grad, "d.patch": q.grad}
    got.update({"d." + n: x.grad for n, x in p.items()})
    return got, list(names)


GLOBAL_NAMES = ("out.global",) + D_PARAMS


def check_guards_1_2(be, c: BlockCase):
    """(1) a non-finite region embedding zeroes that row only, (2) a non-finite token zeroes that caption's block only: the
    results equal, bit for bit, the run on inputs zeroed by hand, and that run holds the gate against the fp64 reference on
    the zeroed inputs."""
    d = block_data(c)
    what = f"guards (1)(2) {c.id}"
    b_cap, (b_reg, r_reg) = 0, (1, c.R - 1)
    text, patches = d["text"].clone(), d["patches"].clone()
    text[b_cap, c.T // 2, 7] = float("inf")
    patches[b_reg, r_reg, 5] = NAN
    zt, zp = d["text"].clone(), d["patches"].clone()
    zt[b_cap] = 0.0
    zp[b_reg, r_reg] = 0.0
    got, _ = run_global(be, c, text, patches)
    by_hand, _ = run_global(be, c, zt, zp)
    for n in GLOBAL_NAMES:
        assert bool(torch.isfinite(got[n]).all()), f"{what}: {n} is not finite"
    bit_equal(got, by_hand, GLOBAL_NAMES, what + ": not the result of zeroing exactly one region row and one caption")
    return anchor(got, global_ref(c, b_cap, (b_reg, r_reg)), what, absent=())


def check_guard_3(be, c: BlockCase):
    """A NaN made inside the block (norm_text.weight): the output is exactly zero, every parameter gradient and d_text /
    d_patch is exactly zero and not NaN, and the next clean pass through the same module is bit-equal to a fresh module's."""
    d = block_data(c)
    what = f"guard (3) {c.id}"
    bad = {k: v.clone() for k, v in d["sd"].items()}
    bad["norm_text.weight"][3] = NAN
    block = be.block(c.E, c.H, bad)
    for rg in (True, False):
        got, _ = run_global(be, c, d["text"], d["patches"], block=block, inputs_rg=rg)
        names = GLOBAL_NAMES + (("d.text", "d.patch") if rg else ())
        for n in names:
            assert got[n] is not None, f"{what}: {n} is missing"
            assert not bool(torch.isnan(got[n]).any()), f"{what}: NaN reached {n}"
            assert not bool((got[n] != 0).any()), f"{what}: {n} is not exactly zero"
    block.load_state_dict(d["sd"])
    clean, _ = run_global(be, c, d["text"], d["patches"], block=block)
    fresh, _ = run_global(be, c, d["text"], d["patches"])
    bit_equal(clean, fresh, GLOBAL_NAMES, what + ": the clean pass after a replaced batch")
    return anchor(clean, global_ref(c), what + " clean pass")


# ------------------------------------------------------------------------------------------------ the glue

GlueCase = namedtuple("GlueCase", "id counts lens extra_tokens")
# lens: caption lengths BOS .. first EOS (2 = no word token: its sentence row goes to slot 0); T = 16 positions, R = 3 regions
GLUE_R = 3
GLUE_CASES = (
    GlueCase("counts_3_1_0_2", (3, 1, 0, 2), (7, 2, 5, 9), 0),
    GlueCase("counts_all_zero", (0, 0, 0, 0), (7, 2, 5, 9), 0),           # rmax = 1: one zero row each
    GlueCase("counts_one_full", (1, 3, 2, 1), (4, 6, 3, 5), 0),
    GlueCase("counts_none", None, (7, 2, 5, 9), 0),
    GlueCase("max_tokens_plus_3", (3, 1, 0, 2), (7, 2, 5, 9), 3),         # three more zero rows: attended, LayerNorm'd, pooled
)
GLUE_BY_ID = {c.id: c for c in GLUE_CASES}
CLIP_SEED, CM_SEED = 7, 31


@functools.lru_cache(maxsize=None)
def glue_cfg():
    return dcfg.tiny()


@functools.lru_cache(maxsize=None)
def glue_weights():
    cfg = glue_cfg()
    return synth.synth_clip_state_dict(cfg, seed=CLIP_SEED, gain=4.0), synth.synth_cross_modal_state_dict(cfg.projection_dim, seed=CM_SEED)


@functools.lru_cache(maxsize=None)
def glue_data(c: GlueCase):
    cfg = glue_cfg()
    B, T = len(c.lens), cfg.text.max_position_embeddings
    regions = synth.synth_regions(B, GLUE_R, cfg.vision, seed=3)
    ids = torch.randint(1, cfg.text.bos_token_id, (B, T), generator=torch.Generator().manual_seed(9), dtype=torch.int64)
    ids[:, 0] = cfg.text.bos_token_id
    for b, n in enumerate(c.lens):
        ids[b, n - 1:] = cfg.text.eos_token_id
    need = max(max(c.lens) - 2, 1)
    counts = None if c.counts is None else torch.tensor(c.counts, dtype=torch.int32)
    return {"regions": regions, "ids": ids, "counts": counts, "max_tokens": need + c.extra_tokens, "needed_tokens": need}


def glue_shapes(c: GlueCase):
    """(Tmax, Rmax) of the blocks the glue builds."""
    d = glue_data(c)
    return d["max_tokens"], (GLUE_R if c.counts is None else max(max(c.counts), 1))


@functools.lru_cache(maxsize=None)
def glue_ref(c: GlueCase) -> Ref:
    """O.teacher_step fed the oracle's own tower outputs in the evaluation's dtype; the [B, Tmax, E] / [B, Rmax, E] blocks are
    exactly those the glue builds (asserted against glue_shapes)."""
    cfg, d = glue_cfg(), glue_data(c)
    clip_sd, cm_sd = glue_weights()
    E, heads = cfg.projection_dim, cfg.projection_dim // 64
    counts = [GLUE_R] * len(c.lens) if c.counts is None else list(c.counts)

    def evaluate(dtype):
        teacher = O.to_dtype(clip_sd, dtype)
        with torch.no_grad():
            embs = [O.vision_tower(teacher, d["regions"][b, :n].to(dtype), cfg.vision) if n > 0 else torch.zeros(0, E, dtype=dtype)
                    for b, n in enumerate(counts)]
            patches = O.pad_regions(embs, E)
            tokens, _n, sent = O.teacher_token_embeddings(teacher, d["ids"], cfg.text)
            assert tokens.shape[1] == d["needed_tokens"]
            if d["max_tokens"] > tokens.shape[1]:
                tokens = torch.cat([tokens, torch.zeros(tokens.shape[0], d["max_tokens"] - tokens.shape[1], E, dtype=dtype)], dim=1)
            assert (tokens.shape[1], patches.shape[1]) == glue_shapes(c)
        p = {k: v.to(dtype).clone().requires_grad_(True) for k, v in cm_sd.items()}
        r = O.teacher_step(p, tokens, patches, sent, heads)
        r["loss"].backward()
        res = {"out.loss": r["loss"], "out.global": r["image_emb"]}
        res.update({"d." + n: p[n].grad for n in PARAMS})
        return res
    # no region anywhere: the one key is a zero row, so q and k get nothing (softmax of one) and v's weight gradient is dv^T 0
    zero = ("d.text_to_image.in_proj_weight",) if glue_shapes(c)[1] == 1 and max(counts) == 0 else ()
    return Ref(evaluate, None, f"glue {c.id}", zero)


GLUE_NAMES = ("out.loss", "out.global") + D_PARAMS


def run_glue(be, c: GlueCase, packed_text: bool = False, regions=None, ids=None, teacher=None):
    """compute_global_embedding_tensors, then contrastive_loss(global, last_sentence_embedding) as train_contrastive_teacher
    takes it.  packed_text: the ids stay on the host (the packed pass derives the lengths there)."""
    cfg, d = glue_cfg(), glue_data(c)
    clip_sd, cm_sd = glue_weights()
    dev = be.device
    t = be.teacher(cfg, clip_sd, cm_sd, packed_text) if teacher is None else teacher
    p = params_of(t.cross_modal_attention)
    for x in p.values():
        x.grad = None
    regions = d["regions"] if regions is None else regions
    ids = d["ids"] if ids is None else ids
    with be.watch() as names:
        glob = t.compute_global_embedding_tensors(regions.to(dev), ids if packed_text else ids.to(dev), d["counts"], d["max_tokens"])
        loss = be.contrastive(glob, t.last_sentence_embedding, 0.05)
        loss.backward()
    got = {"out.loss": loss.detach(), "out.global": glob.detach()}
    got.update({"d." + n: x.grad for n, x in p.items()})
    return got, list(names), t


def check_glue_case(be, c: GlueCase, packed_text: bool = False) -> Dict[str, float]:
    what = f"glue {c.id}" + (" packed_text" if packed_text else "")
    got, names, _ = run_glue(be, c, packed_text)
    Tmax, Rmax = glue_shapes(c)
    check_routes(names, Tmax, Rmax, what)
    return anchor(got, glue_ref(c), what)


def check_row_independence(be, c: GlueCase, packed_text: bool = False):
    """Region rows at or beyond region_counts[b] and token ids behind the first EOS do not exist for the function: changed
    (NaN pixels included: mask_rows runs before guard (1)), no output or gradient bit moves."""
    assert c.counts is not None
    d = glue_data(c)
    cfg = glue_cfg()
    what = f"glue {c.id}" + (" packed_text" if packed_text else "")
    base, _, _ = run_glue(be, c, packed_text)
    regions = d["regions"].clone()
    for b, n in enumerate(c.counts):
        for r in range(n, GLUE_R):
            regions[b, r] = NAN if (b + r) % 2 == 0 else 5.0
    got, _, _ = run_glue(be, c, packed_text, regions=regions)
    bit_equal(got, base, GLUE_NAMES, what + ": a region row at or beyond region_counts leaks")
    ids = d["ids"].clone()
    for b, n in enumerate(c.lens):
        if n < ids.shape[1]:
            ids[b, n:] = torch.randint(1, cfg.text.bos_token_id, (ids.shape[1] - n,), generator=torch.Generator().manual_seed(b))
    got, _, _ = run_glue(be, c, packed_text, ids=ids)
    bit_equal(got, base, GLUE_NAMES, what + ": a token behind the first EOS leaks")


def trainer_filter(module) -> List[str]:
    """train_contrastive_teacher.main's rule (everything frozen, then every name holding one of its keys trainable) applied to
    `module`: the two loops are taken from main's own source, not retyped.  Returns the trainable names."""
    import inspect
    import textwrap
    from dclip_amd import train_contrastive_teacher as tct
    src = inspect.getsource(tct.main)
    start, end = src.index("    for param in teacher.parameters():"), src.index("    trainable = ")
    rule = textwrap.dedent(src[start:end])
    assert "requires_grad = False" in rule and "requires_grad = True" in rule, rule
    exec(compile(rule, "train_contrastive_teacher.main", "exec"), {"teacher": module})
    return [n for n, p in module.named_parameters() if p.requires_grad]


def check_trainer_filter(module):
    names = trainer_filter(module)
    want = ["cross_modal_attention." + n for n in PARAMS]
    assert names == want, f"the trainer's name filter leaves {names} trainable"
    assert [n for n, _ in module.named_parameters()] == want, "the teacher holds parameters besides the block's 12"
