"""Every backward schedule of dclip_amd/engine.py that produces parameter gradients, under partial `need` masks, against the
fp64 oracle under autograd (cases, reference and checkers: tests/schedule_checks.py).  The tests go through
engine.vision_fwd / vision_bwd, vision_fwd_bf16_train / vision_bwd_bf16 and text_fwd / text_bwd with explicit `need` lists;
every case asserts the route it took (the route predicate and a launch name), so a shape that no longer reaches a schedule
fails instead of quietly testing the other one."""
import dataclasses

import pytest
import torch

from dclip_amd import config as dcfg, synth
from tests import schedule_checks as sc

pytestmark = pytest.mark.gpu

BF16, FP16 = torch.bfloat16, torch.float16
TY = {"bf16": BF16, "fp16": FP16}


def _dev():
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ shapes

@dataclasses.dataclass(frozen=True)
class Shape:
    name: str
    tower: str
    width: str            # "tiny" (D = 128, I = 256) or "wide" (ViT-B/32's widths, small projection)
    L: int
    B: int
    grid: tuple = None    # vision: another patch grid (gh, gw)
    T: int = None         # text: tokens per caption

    def config(self):
        if self.width == "tiny":
            return dcfg.tiny(layers=self.L)
        v = dcfg.VisionConfig(hidden_size=768, intermediate_size=3072, num_hidden_layers=self.L, num_attention_heads=12,
                              image_size=224, patch_size=32)
        return dataclasses.replace(dcfg.tiny(layers=self.L), vision=v, name=f"wide{self.L}")


TINY = Shape("tiny", "vision", "tiny", 2, 6)
TINY3 = Shape("tiny3", "vision", "tiny", 3, 6)
TINY64 = Shape("tiny_b64", "vision", "tiny", 2, 64)              # 1088 tokens = 17 x 64: the segmented weight gradient applies
TINY_GRID = Shape("tiny_3x5", "vision", "tiny", 2, 6, grid=(3, 5))
WIDE = Shape("wide2_b192", "vision", "wide", 2, 192)             # 9600 tokens = 150 x 64, 9408 patch rows = 147 x 64
WIDE3 = Shape("wide3_b192", "vision", "wide", 3, 192)
WIDE_GRID = Shape("wide2_9x9_b96", "vision", "wide", 2, 96, grid=(9, 9))     # S = 82 > 64; 7872 tokens = 123 x 64
TEXT16 = Shape("text_t16", "text", "tiny", 2, 6, T=16)
TEXT9 = Shape("text_t9", "text", "tiny", 2, 6, T=9)              # below max_position_embeddings = 16
TEXT3 = Shape("text3_t16", "text", "tiny", 3, 6, T=16)


class Problem:
    """One shape's parameters, input, d_out and references; everything is made once (module scope) and never written."""

    def __init__(self, shape: Shape):
        self.shape, dev = shape, _dev()
        cfg = shape.config()
        self.cfg = cfg
        self.tcfg = cfg.vision if shape.tower == "vision" else cfg.text
        self.sd = synth.synth_clip_state_dict(cfg, seed=7, gain=4.0 if shape.width == "tiny" else 3.0)
        if shape.tower == "vision":
            v = cfg.vision
            if shape.grid is None:
                x = synth.synth_pixel_values(shape.B, v, seed=0)
            else:
                x = torch.randn((shape.B, 3, shape.grid[0] * v.patch_size, shape.grid[1] * v.patch_size),
                                generator=torch.Generator().manual_seed(5))
            self.x = x.to(dev)
        else:
            ids = synth.synth_input_ids(shape.B, cfg.text, seed=3, ragged=True)[:, :shape.T].clone()
            ids[:, -1] = cfg.text.eos_token_id                     # a caption cut short still ends in EOS
            ids[1, 2] = ids[1, 1]                                  # a repeated token id inside one caption ...
            ids[2, 1] = ids[1, 1]                                  # ... and across captions: rows of dtok that accumulate
            assert len({int(e) for e in (ids == cfg.text.eos_token_id).int().argmax(1)}) > 2          # ragged
            self.x = ids.to(dev)
        self.W64 = sc.output_weighting((shape.B, cfg.projection_dim))
        self.d_out = self.W64.float().to(dev)
        self.tensors = sc.engine_tensors(shape.tower, shape.L, self.sd, dev)
        self.names = sc.names(shape.tower, shape.L)
        self.sizes = {n: t.numel() for n, t in zip(self.names, self.tensors)}
        self._refs = {}
        # the fp64 oracle runs on the device for the vision tower (the wide shapes are ~1 TFLOP of fp64); the oracle builds the
        # text tower's causal mask on the host, so that tower is evaluated there
        self.ref_dev = dev if shape.tower == "vision" else "cpu"

    def _reference(self, dtype, linear=None):
        x = self.x if self.shape.tower == "text" else self.x.double()
        r = sc.reference(self.shape.tower, self.tcfg, self.sd, x.cpu() if self.ref_dev == "cpu" else x, self.W64, dtype=dtype,
                         device=self.ref_dev, linear=linear, grid=self.shape.grid)
        return {n: t.to(_dev()) for n, t in r.items()}

    def ref(self, key):
        """'r64' (the anchor of the fp32 routes), 'e_ref32', or a 16-bit type: (the rounded-operand reference, E_emul)."""
        if key not in self._refs:
            if key == "r64":
                self._refs[key] = self._reference(torch.float64)
            elif key == "e_ref32":
                self._refs[key] = sc.errors(self._reference(torch.float32), self.ref("r64"))
            else:
                emul = self._reference(torch.float64, linear=sc.rounded_linear(key))
                self._refs[key] = (emul, sc.errors(emul, self.ref("r64")))
        return self._refs[key]

    def need(self, mask):
        return [n in mask for n in self.names]


class Store:
    def __init__(self):
        self.problems, self.full, self.figures, self.freeze = {}, {}, {}, None

    def problem(self, shape: Shape) -> Problem:
        if shape.name not in self.problems:
            self.problems[shape.name] = Problem(shape)
        return self.problems[shape.name]

    def freeze_sets(self, tower):
        if self.freeze is None:
            from dclip_amd.clip_model import HipCLIPModel
            model = HipCLIPModel(dcfg.tiny())                     # on the host: the rule reads names only
            self.freeze = {t: sc.freeze_sets(t, 2, model) for t in ("vision", "text")}
        return self.freeze[tower]

    def note(self, route, ratios):
        """Worst E / gate per route and tensor family, printed at the end of the module (DESIGN.md §26's table)."""
        fam = self.figures.setdefault(route, {})
        for n, r in ratios.items():
            f = n.split(".")[-1]
            if r > fam.get(f, (0.0, ""))[0]:
                fam[f] = (r, n)


@pytest.fixture(scope="module")
def store():
    s = Store()
    yield s
    for route, fam in sorted(s.figures.items()):
        worst = max(fam.values())
        print(f"\n[schedule grads] {route}: worst E/gate {worst[0]:.3f} ({worst[1]}); per family " +
              ", ".join(f"{f} {r:.3f}" for f, (r, _) in sorted(fam.items())))
    for name, p in sorted(s.problems.items()):
        if "e_ref32" in p._refs:
            w = max(p._refs["e_ref32"].items(), key=lambda kv: kv[1])
            print(f"[schedule grads] {name}: E_ref32 max {w[1]:.2e} ({w[0]})")
        for ty in (BF16, FP16):
            if ty in p._refs:
                w = max(p._refs[ty][1].items(), key=lambda kv: kv[1])
                lo = min(p._refs[ty][1].items(), key=lambda kv: kv[1])
                print(f"[schedule grads] {name}: E_emul {ty} max {w[1]:.2e} ({w[0]}), min {lo[1]:.2e} ({lo[0]})")


# ------------------------------------------------------------------------------------------------ routes

@dataclasses.dataclass(frozen=True)
class Route:
    name: str
    kind: str                 # "fp32" (engine.vision_fwd / vision_bwd), "16" (vision_fwd_bf16_train / vision_bwd_bf16), "text"
    shape: Shape
    ty: str = None            # "bf16" / "fp16" for kind "16"
    pruned: bool = True       # fp32: hidden_out=None (last_layer_*_cls) or a list (layer_* at full size throughout)
    split: tuple = (False, False, False)       # engine._VSPLIT16, _VSPLIT16_BWD, _VSPLIT16_WGRAD
    stale: bool = False       # bump a watched weight's version between forward and backward
    env: tuple = ()
    tokmajor: bool = False    # what _tokmajor_wgrads must answer
    io16: bool = False        # ... and _attention_io16
    full_masks: bool = False  # the whole mask list, or (a), (e), (f), (j)
    precision: str = None     # the HipCLIPModel precision string of this route


R_PLAIN = Route("fp32_plain_pruned", "fp32", TINY, full_masks=True, precision="fp32")
R_UNPRUNED = Route("fp32_plain_unpruned", "fp32", TINY, pruned=False, full_masks=True)
R_PLAIN3 = Route("fp32_plain_pruned_L3", "fp32", TINY3)
R_SPLIT_F = Route("fp32_split16_fwd", "fp32", TINY64, split=(True, False, False))
R_SPLIT_FB = Route("fp32_split16_fwd_dgrad", "fp32", TINY64, split=(True, True, False))
R_SPLIT_ALL = Route("fp32_split16_fwd_dgrad_wgrad", "fp32", TINY64, split=(True, True, True), full_masks=True, precision="fp32")
R_SPLIT_STALE = Route("fp32_split16_stale_backward", "fp32", TINY64, split=(True, True, True), stale=True)
R_GRID = Route("fp32_plain_grid_3x5", "fp32", TINY_GRID)
R_TR = {t: Route(f"{t}_transposing", "16", TINY, ty=t, full_masks=True, precision="bf16" if t == "bf16" else "fp16-mixed") for t in TY}
R_TR3 = Route("bf16_transposing_L3", "16", TINY3, ty="bf16")
R_TOK = {t: Route(f"{t}_tokmajor_mfma", "16", WIDE, ty=t, tokmajor=True, io16=True, full_masks=True,
                  precision="bf16" if t == "bf16" else "fp16-mixed") for t in TY}
R_TOK3 = Route("bf16_tokmajor_mfma_L3", "16", WIDE3, ty="bf16", tokmajor=True, io16=True)
R_TOK_IO16 = Route("bf16_tokmajor_io16_fp32_arithmetic", "16", WIDE, ty="bf16", tokmajor=True, io16=True, env=(("DCLIP_BF16_ATTN_MFMA", "0"),))
R_TOK_F32ATTN = Route("bf16_tokmajor_fp32_attention", "16", WIDE, ty="bf16", tokmajor=True, env=(("DCLIP_BF16_ATTN_IO16", "0"),))
R_TOK_GRID = Route("bf16_tokmajor_grid_9x9", "16", WIDE_GRID, ty="bf16", tokmajor=True)
R_TOK_NOSIDE = Route("bf16_tokmajor_no_side_stream", "16", WIDE, ty="bf16", tokmajor=True, io16=True, env=(("DCLIP_BF16_WGRAD_STREAM", "0"),))
R_TEXT = Route("text_fp32_t16", "text", TEXT16, full_masks=True, precision="fp32")
R_TEXT9 = Route("text_fp32_t9", "text", TEXT9, full_masks=True)
R_TEXT3 = Route("text_fp32_L3", "text", TEXT3)

FEW = ("a_everything", "e_bottom_fc2_b", "f_weights", "j_as_written")


def route_masks(route: Route, store: Store):
    tower = route.shape.tower
    if route.shape.L == 3:
        return sc.masks(tower, 3)
    m = sc.masks(tower, 2, store.freeze_sets(tower))
    return m if route.full_masks else {k: v for k, v in m.items() if k in FEW}


def _mask_ids(route: Route):
    tower = route.shape.tower
    if route.shape.L == 3:
        return list(sc.masks(tower, 3))
    ids = list(sc.masks(tower, 2)) + (["j_as_written"] if tower == "vision" else [])        # (j) is checked against the product below
    return ids if route.full_masks else [k for k in ids if k in FEW]


# ------------------------------------------------------------------------------------------------ running one case

class Trace:
    """What a run did, seen from outside the schedules: which layer backwards were entered and the dx each returned, the
    |dy| column sums of every linear_param_grads call (the bound of a bias that another launch makes), and the launch site
    reported right after each watched call."""

    def __init__(self):
        self.layers, self.dx, self.colabs, self.launch, self.current = [], {}, {}, [], None

    def launches(self, what: str):
        return [l for w, l in self.launch if w == what]


def _instrument(monkeypatch, trace: Trace, params, route: Route):
    from dclip_amd import _lib, engine, ops
    lib = _lib.load()
    ids = {id(lp): i for i, lp in enumerate(params.layers)}

    def layer_spy(name):
        orig = getattr(engine, name)

        def spy(dx2, p, *a, **kw):
            if name != "layer_bwd_bf16_tokmajor":
                trace.layers.append(ids[id(p)])
                trace.current = ids[id(p)]
            else:
                trace.launch.append(("layer_bwd_bf16_tokmajor", ""))
            res = orig(dx2, p, *a, **kw)
            if name != "layer_bwd_bf16_tokmajor":
                trace.dx[ids[id(p)]] = res[0]
            return res
        monkeypatch.setattr(engine, name, spy)

    for name in ("layer_bwd", "last_layer_bwd_cls", "layer_bwd_bf16", "layer_bwd_bf16_tokmajor"):
        layer_spy(name)

    orig_lpg = engine.linear_param_grads

    def lpg_spy(dy, x, need_w, need_b, gr, wkey, bkey, *a, **kw):
        trace.colabs[f"layers.{trace.current}.{bkey}"] = (dy.shape[0], dy.abs().sum(0, dtype=torch.float64))
        return orig_lpg(dy, x, need_w, need_b, gr, wkey, bkey, *a, **kw)
    monkeypatch.setattr(engine, "linear_param_grads", lpg_spy)

    def watch(obj, attr, label=None):
        orig = getattr(obj, attr)

        def spy(*a, **kw):
            res = orig(*a, **kw)
            trace.launch.append((label or attr, lib.dclip_last_launch().decode()))
            return res
        monkeypatch.setattr(obj, attr, spy)

    for attr in ("gemm_f16_rows_dev", "gemm_f16_wgrad_tokmajor_seg3", "gemm_f16_dev", "attention_bwd", "attention_cls_bwd", "pos_interp_bwd",
                 "split_f16x3_rows_colstats", "colsum", "text_embed_bwd"):
        watch(ops, attr)
    if route.kind == "16":
        k = engine._TRAIN16[TY[route.ty]]
        for attr in ("wgrad", "wgrad_tokmajor", "attention_bwd"):
            watch(k, attr, "k." + attr)
        if k.io16_pair is not None:
            fwd, bwd = k.io16_pair

            def bwd_spy(*a, **kw):
                res = bwd(*a, **kw)
                trace.launch.append(("k.io16_bwd", lib.dclip_last_launch().decode()))
                return res
            monkeypatch.setattr(k, "io16_pair", (fwd, bwd_spy))


def _set_route(monkeypatch, route: Route):
    from dclip_amd import engine
    for var in ("DCLIP_BF16_WGRAD_TN", "DCLIP_BF16_ATTN_IO16", "DCLIP_BF16_ATTN_MFMA", "DCLIP_BF16_WGRAD_STREAM", "DCLIP_BF16_PATCH"):
        monkeypatch.delenv(var, raising=False)
    for k_, v_ in route.env:
        monkeypatch.setenv(k_, v_)
    engine._TOKMAJOR_PLAN.clear()
    engine._PATCH_BF16_PLAN.clear()
    monkeypatch.setattr(engine, "_VSPLIT16", route.split[0])
    monkeypatch.setattr(engine, "_VSPLIT16_BWD", route.split[1])
    monkeypatch.setattr(engine, "_VSPLIT16_WGRAD", route.split[2])


def run(store: Store, route: Route, mask, on_ready=None, alloc=None, instrument=True):
    """One forward and one backward of `route` under `mask` -> ({name: gradient or None}, Trace).  Asserts the route."""
    prob = store.problem(route.shape)
    with pytest.MonkeyPatch.context() as mp:        # the spies and switches of THIS run only: undone when it returns
        return _run(mp, prob, route, mask, on_ready, alloc, instrument)


def _run(monkeypatch, prob: Problem, route: Route, mask, on_ready, alloc, instrument):
    from dclip_amd import engine
    _set_route(monkeypatch, route)
    trace = Trace()
    L, need = route.shape.L, prob.need(mask)
    if route.kind == "text":
        p = engine.TextParams.from_tensors(prob.tensors, L)
        if instrument:
            _instrument(monkeypatch, trace, p, route)
        _out, saved = engine.text_fwd(p, prob.x, prob.tcfg, True)
        grads = engine.text_bwd(p, saved, prob.d_out, prob.tcfg, need)
    elif route.kind == "fp32":
        p = engine.VisionParams.from_tensors(prob.tensors, L)
        if instrument:
            _instrument(monkeypatch, trace, p, route)
        cache, split16 = {}, []
        _out, saved = engine.vision_fwd(p, prob.x, prob.tcfg, True, hidden_out=None if route.pruned else [], grid=route.shape.grid,
                                        split16_cache=cache if route.split[0] else None, split16_out=split16)
        assert saved[9] is route.pruned
        if route.split[0]:
            assert "__vsplit16__" in cache, "the forward did not plan the split-fp16 path"
            assert bool(split16) == route.split[1]
            assert (len(saved[4][0]) == 14) == (route.split[1] and route.split[2])          # the forward kept its split operands
        if route.stale:
            p.layers[0].fc1_w.add_(0.0)                          # same values, another version: the plan is no longer this forward's
            assert not split16[0].fresh()
        grads = engine.vision_bwd(p, saved, prob.d_out, prob.tcfg, need, on_ready, alloc, split16=split16[0] if split16 else None)
    else:
        ty = TY[route.ty]
        v, B = prob.tcfg, route.shape.B
        S = engine._grid_seq(v, route.shape.grid)
        p = engine.VisionParams.from_tensors(prob.tensors, L)
        if instrument:
            _instrument(monkeypatch, trace, p, route)
        assert engine._tokmajor_wgrads(B * S, v.hidden_size, v.intermediate_size, ty) is route.tokmajor
        assert engine._attention_io16(B * S, S, v.hidden_size, v.intermediate_size, ty) is route.io16
        cache16 = {}                                             # the weight copies: the backward reads what the forward made
        _out, saved = engine.vision_fwd_bf16_train(p, prob.x, v, cache16, ty, grid=route.shape.grid)
        patch16 = engine._patch_embed_bf16(v, B * (S - 1), ty)
        assert saved[0].dtype == (ty if patch16 else torch.float32)
        if route.shape is WIDE or route.shape is WIDE3:
            assert patch16, "9408 patch rows: the 16-bit patch embedding is the default there"
        if route.shape is WIDE_GRID:
            assert not patch16 and (B * (S - 1)) % 64 != 0
        qkv = saved[4][0][4]
        assert (qkv.dtype == ty) is route.io16
        grads = engine.vision_bwd_bf16(p, saved, prob.d_out, v, need, cache16, on_ready, alloc, ty)
    torch.cuda.synchronize()
    got = dict(zip(prob.names, grads))
    if instrument:
        _assert_route(route, trace, mask, prob)
    return got, trace


def _assert_route(route: Route, trace: Trace, mask, prob: Problem):
    """The launch names that prove the route, from the sites reported right after the watched calls."""
    tower, L = route.shape.tower, route.shape.L
    sc.check_layers_run(trace.layers, tower, mask, L, route.name)
    run_layers = sc.layers_run(tower, mask, L)
    wants_w = any(n.split(".")[-1] in ("fc2_w", "fc1_w", "out_w", "qkv_w") and int(n.split(".")[1]) in run_layers for n in mask if "." in n)
    if route.kind == "16":
        assert bool(trace.launches("layer_bwd_bf16_tokmajor")) == (route.tokmajor and bool(run_layers))
        if route.tokmajor:
            assert not trace.launches("k.wgrad")
            if wants_w:
                site = "gemm_bf16_wgrad_tokmajor" if route.ty == "bf16" else "gemm_f16_wgrad_tokmajor"
                assert trace.launches("k.wgrad_tokmajor") and all(l.startswith(site) for l in trace.launches("k.wgrad_tokmajor")), trace.launch
        else:
            assert not trace.launches("k.wgrad_tokmajor")
            if wants_w:
                site = "gemm_bf16_splitk" if route.ty == "bf16" else "gemm_f16_splitk"
                assert trace.launches("k.wgrad") and all(l.startswith(site) for l in trace.launches("k.wgrad")), trace.launch
        if run_layers:
            mfma = route.io16 and not dict(route.env).get("DCLIP_BF16_ATTN_MFMA") == "0"
            if mfma:
                assert len(trace.launches("k.attention_bwd")) == len(run_layers) and not trace.launches("attention_bwd"), trace.launch
                assert all(l.startswith("attention_bwd_" + ("bf16" if route.ty == "bf16" else "f16")) for l in trace.launches("k.attention_bwd")), trace.launch
            elif route.io16:
                assert all(l.startswith("attention_bwd_io16") for l in trace.launches("k.io16_bwd")) and len(trace.launches("k.io16_bwd")) == len(run_layers)
            else:
                got = trace.launches("attention_bwd")
                assert len(got) == len(run_layers) and all(l.startswith("attention_bwd") and "io16" not in l for l in got), trace.launch
    elif route.kind == "fp32":
        split_bwd = route.split[1] and not route.stale
        assert bool(trace.launches("gemm_f16_rows_dev")) == (split_bwd and bool(run_layers)), trace.launch
        assert bool(trace.launches("gemm_f16_wgrad_tokmajor_seg3")) == (split_bwd and route.split[2] and wants_w), trace.launch
        assert all(l.startswith("gemm_f16_wgrad_tokmajor_seg3") for l in trace.launches("gemm_f16_wgrad_tokmajor_seg3"))
        assert all(l.startswith("gemm_f16_scaled_rows_dev") for l in trace.launches("gemm_f16_rows_dev")), trace.launch
        assert bool(trace.launches("gemm_f16_dev")) == route.split[0]
        if L - 1 in run_layers:
            assert bool(trace.launches("attention_cls_bwd")) == route.pruned
    if tower == "vision" and route.shape.grid is not None:
        assert (trace.launches("pos_interp_bwd") == ["pos_interp_bwd"]) == ("pos" in mask), trace.launch
    if tower == "text":
        assert bool(trace.launches("text_embed_bwd")) == ("tok" in mask)


def anchor(store: Store, route: Route, got, what):
    prob = store.problem(route.shape)
    if route.kind == "16":
        want, e_emul = prob.ref(TY[route.ty])
        gate = sc.gates16(e_emul)
    else:
        want, gate = prob.ref("r64"), sc.gates32(prob.ref("e_ref32"))
    ratios = sc.check_anchor(got, want, gate, what)          # its message carries E and the gate of every failing tensor
    store.note(route.name, ratios)
    return ratios


def full_run(store: Store, route: Route):
    """The full-mask run of a route: made once, shared by every partial mask of that route, never written."""
    if route.name not in store.full:
        prob = store.problem(route.shape)
        got, trace = run(store, route, frozenset(prob.names))
        store.full[route.name] = (got, trace)
    return store.full[route.name]


def check_case(store: Store, route: Route, mid: str):
    prob = store.problem(route.shape)
    mask = route_masks(route, store)[mid]
    what = f"{route.name} {mid}"
    full, ftrace = full_run(store, route)
    got, trace = run(store, route, mask)
    sc.check_completeness(got, mask, prob.names, what)
    anchor(store, route, got, what)
    exc = sc.bias_exceptions(route.kind != "16", mask, prob.names)
    bounds = {n: sc.colsum_bound(*ftrace.colabs[n]) for n in exc}
    if route.kind == "text" and "tok" in mask:                   # float atomics: no fixed order, even under one mask
        exc = exc | {"tok"}
        bounds["tok"] = sc.embed_atomic_bound(prob.x, ftrace.dx[0], prob.tcfg.vocab_size)
    sc.check_mask_consistency(got, full, exc, bounds, what)
    run_layers = sc.layers_run(route.shape.tower, mask, route.shape.L)
    if run_layers:
        b = run_layers[-1]
        assert torch.equal(trace.dx[b], ftrace.dx[b]), f"{what}: the dx layer {b} returned differs from the full-mask run's"
    if route.shape.tower == "text" and got["pos"] is not None:
        sc.check_text_pos_tail(got["pos"], route.shape.T, what)
    return got


# ------------------------------------------------------------------------------------------------ the cases

def _cases(routes):
    return [pytest.param(r, m, id=f"{r.name}-{m}") for r in routes for m in _mask_ids(r)]


ALL_ROUTES = [R_PLAIN, R_UNPRUNED, R_PLAIN3, R_SPLIT_F, R_SPLIT_FB, R_SPLIT_ALL, R_SPLIT_STALE, R_GRID, R_TR["bf16"], R_TR["fp16"], R_TR3,
              R_TOK["bf16"], R_TOK["fp16"], R_TOK3, R_TOK_IO16, R_TOK_F32ATTN, R_TOK_GRID, R_TOK_NOSIDE, R_TEXT, R_TEXT9, R_TEXT3]


@pytest.mark.parametrize("route,mid", _cases(ALL_ROUTES))
def test_schedule_gradients(store, route, mid):
    check_case(store, route, mid)


def test_listed_freeze_masks_are_the_products_own(store):
    """(j) comes from CLIPImageDistillation.set_freeze_mode: north_star is mask (a) for the vision tower and nothing for the
    text tower, as_written is listed for the vision tower and is mask (a) for the text tower."""
    v, t = store.freeze_sets("vision"), store.freeze_sets("text")
    assert v["north_star"] == frozenset(sc.names("vision", 2)) and not t["north_star"] and t["as_written"] == frozenset(sc.names("text", 2))
    assert set(sc.masks("vision", 2, v)) == set(_mask_ids(R_PLAIN)) and set(sc.masks("text", 2, t)) == set(_mask_ids(R_TEXT))


@pytest.mark.parametrize("mid", FEW)
def test_side_stream_off_is_bit_equal_to_side_stream_on(store, mid):
    mask = route_masks(R_TOK_NOSIDE, store)[mid]
    off, _ = run(store, R_TOK_NOSIDE, mask)
    on, _ = run(store, R_TOK["bf16"], mask)
    for n in off:
        assert (off[n] is None) == (on[n] is None), n
        if off[n] is not None:
            assert torch.equal(off[n], on[n]), f"{n}: the side stream changes the value"


@pytest.mark.parametrize("route", [R_PLAIN, R_UNPRUNED, R_TR["bf16"], R_TOK["bf16"], R_TOK["fp16"]], ids=lambda r: r.name)
@pytest.mark.parametrize("mid", ["a_everything", "j_as_written", "g_biases_ln"])
def test_alloc_and_on_ready(store, route, mid):
    """Every gradient lands in its slice of one guarded bucket, bit-equal to the run without `alloc`; `on_ready` reports each
    needed name once, tail / layers top down / head, and what it reports is final (the side stream has been joined)."""
    prob = store.problem(route.shape)
    mask = route_masks(route, store)[mid]
    what = f"{route.name} {mid} alloc/on_ready"
    base, _ = run(store, route, mask)
    bucket, log = sc.Bucket(prob.sizes, device=_dev()), sc.ReadyLog()
    got, _ = run(store, route, mask, on_ready=log, alloc=bucket.alloc)
    sc.check_completeness(got, mask, prob.names, what)
    bucket.check(got, base, what)
    log.check(got, "vision", mask, route.shape.L, what)


@pytest.mark.parametrize("route", [R_PLAIN, R_SPLIT_ALL, R_TR["bf16"], R_TR["fp16"], R_TOK["bf16"], R_TOK["fp16"], R_TEXT], ids=lambda r: r.name)
def test_module_pass_equals_the_engine_level_result(monkeypatch, store, route):
    """Through HipCLIPModel with requires_grad flags: .grad is None exactly on the frozen parameters and equals the
    engine-level result of the same route bit for bit."""
    from dclip_amd.clip_model import from_hf_state_dict
    prob = store.problem(route.shape)
    tower = route.shape.tower
    masks = route_masks(route, store)
    mask = masks["j_as_written"] if tower == "vision" else masks["i_top_layer"]
    want, _ = run(store, route, mask)
    _set_route(monkeypatch, route)
    model = from_hf_state_dict(prob.cfg, prob.sd, device=_dev())
    for t in model.parameters():
        t.requires_grad = False
    params = model.vision_params() if tower == "vision" else model.text_params()
    assert params.names() == prob.names
    for n, t in zip(prob.names, params.tensors()):
        t.requires_grad = n in mask
    if tower == "vision":
        out = model.get_image_features(pixel_values=prob.x, precision=route.precision)
    else:
        out = model.get_text_features(input_ids=prob.x)
    out.backward(prob.d_out)
    torch.cuda.synchronize()
    for n, t in zip(prob.names, params.tensors()):
        assert (t.grad is None) == (n not in mask), n
        if n in mask:
            assert torch.equal(t.grad.reshape(-1), want[n].reshape(-1)), f"{route.name}: {n} through the module differs from the engine-level run"
    others = [n for n, t in model.named_parameters() if t.grad is not None and not any(t is q for q in params.tensors())]
    assert not others, others
