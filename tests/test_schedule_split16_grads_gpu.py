"""The split-fp16 backward with the dY-statistics regime ON, under partial `need` masks: engine._layers_bwd for the
vision tower, the padded text tower and the packed text tower on their device plans, through §26's machinery
(tests/schedule_checks.py, tests/test_schedule_grads_gpu.py) — completeness, the layers run, the fp64 anchor with gates32, mask
consistency against the route's own full-mask run, the dx of the lowest layer run — and the single-pass census
(schedule_checks.expected_passes / expected_producers): which split pass every weight gradient takes, where every bias comes
from, and that column statistics are produced exactly where a single pass consumes them.  Every case asserts its route."""
import dataclasses
import time

import pytest
import torch

from dclip_amd import config as dcfg, synth
from dclip_amd.clip_model import packed_text_tables
from tests import schedule_checks as sc
from tests import test_schedule_grads_gpu as g
from tests.test_text_train_split16_gpu import PACKED_LENS, PACKED_LENS_ODD, make_ids, padded_lens
from tests.test_vision_dystats_gpu import PRODUCERS

pytestmark = pytest.mark.gpu

L2 = 2
BIG = (("DCLIP_BF16_BIG_MIN", "1"),)             # the tower's GEMMs on the ping-pong kernel: the register-staged ones have no statistics form
T0 = time.time()


# ------------------------------------------------------------------------------------------------ shapes and problems

TINY3_64 = g.Shape("tiny3_b64", "vision", "tiny", 3, 64)         # 1088 tokens, three layers: two producer -> consumer hops


@dataclasses.dataclass(frozen=True)
class TextShape:
    name: str
    seq: int                  # config.tiny(seq=...): positions per caption
    lens: tuple               # caption lengths (the first EOS at lens[n] - 1)
    packed: bool = False
    seed: int = 5
    tower: str = "text"
    L: int = L2

    @property
    def T(self):
        return self.seq

    @property
    def rows(self):
        return sum(self.lens) if self.packed else len(self.lens) * self.seq


def _padded77_lens():
    lens = padded_lens()                                           # 2, 77, 65, 64 and 60 random lengths in 3 .. 76
    lens[4] = 1                                                    # ... and the EOS alone
    return tuple(lens)


def _lean_lens():
    lens = torch.randint(3, 17, (64,), generator=torch.Generator().manual_seed(4)).tolist()
    lens[0], lens[1], lens[2], lens[3] = 1, 2, 16, 15
    return tuple(lens)


TEXT77 = TextShape("text_t77_b64", 77, _padded77_lens())                      # 4928 rows: the 65 .. 80-row statistics twin
TEXT77_L3 = TextShape("text3_t77_b64", 77, _padded77_lens(), L=3)               # a middle layer: (k), and two hops for (m)
TEXT16 = TextShape("text_t16_b64", 16, _lean_lens())                          # 1024 rows: the causal lean statistics form
PACKED = TextShape("text_packed_256", 77, tuple(PACKED_LENS), packed=True, seed=8)
PACKED_ODD = TextShape("text_packed_249", 77, tuple(PACKED_LENS_ODD), packed=True, seed=9)


def text_ids(cfg, shape: TextShape):
    """make_ids' captions with one word id repeated inside the longest caption and once more in another caption; verified
    with packed_text_tables on the host, as make_ids does."""
    ids = make_ids(cfg, shape.lens, shape.seed)
    order = sorted(range(len(shape.lens)), key=lambda n: -shape.lens[n])
    c, d = order[0], order[1]
    assert shape.lens[c] >= 4 and shape.lens[d] >= 3
    ids[c, 2] = ids[c, 1]
    ids[d, 1] = ids[c, 1]
    assert packed_text_tables(ids, cfg.text.eos_token_id)["lens"].tolist() == list(shape.lens)
    assert int((ids[c, :shape.lens[c]] == ids[c, 1]).sum()) >= 2 and int(ids[d, 1]) == int(ids[c, 1])
    return ids


class TextProblem:
    """config.tiny(seq), gain 2.0 (the gain of test_text_train_split16_gpu.Problem: the device plan raises no flag), the fp64
    oracle on the host (sc.reference on the PADDED ids, for the packed tower too).  Made once per shape, never written."""

    def __init__(self, shape: TextShape):
        self.shape, dev = shape, g._dev()
        self.cfg = dcfg.tiny(layers=shape.L, seq=shape.seq)
        self.tcfg = self.cfg.text
        self.sd = synth.synth_clip_state_dict(self.cfg, seed=7, gain=2.0)
        self.ids = text_ids(self.cfg, shape)
        if shape.seq == 77:
            assert {1, 2, 64, 65, 77} <= set(shape.lens)
        else:
            assert {1, 2, shape.seq - 1, shape.seq} <= set(shape.lens)
        self.x = self.ids.to(dev)
        self.names = sc.names("text", shape.L)
        self.W64 = sc.output_weighting((len(shape.lens), self.cfg.projection_dim))
        self.d_out = self.W64.float().to(dev)
        self.tensors = sc.engine_tensors("text", shape.L, self.sd, dev)
        self.sizes = {n: t.numel() for n, t in zip(self.names, self.tensors)}
        self._refs = {}
        if shape.packed:
            tab = packed_text_tables(self.ids, self.tcfg.eos_token_id)
            assert tab["Tp"] == shape.rows
            tab["cu_seqlens_dev"], tab["last_rows_dev"] = tab["cu_seqlens"].to(dev), tab["last_rows"].to(dev)
            self.tables = tab
            self.embed_ids = torch.cat([self.ids[n, :S] for n, S in enumerate(shape.lens)])
        else:
            self.embed_ids = self.ids

    def _reference(self, dtype):
        r = sc.reference("text", self.tcfg, self.sd, self.ids, self.W64, dtype=dtype)
        return {n: t.to(g._dev()) for n, t in r.items()}

    def ref(self, key):
        if key not in self._refs:
            if key == "r64":
                self._refs[key] = self._reference(torch.float64)
            else:
                assert key == "e_ref32"
                self._refs[key] = sc.errors(self._reference(torch.float32), self.ref("r64"))
        return self._refs[key]

    def need(self, mask):
        return [n in mask for n in self.names]


class Store(g.Store):
    def __init__(self):
        super().__init__()
        self.runs = {}

    def problem(self, shape):
        if shape.name not in self.problems:
            self.problems[shape.name] = TextProblem(shape) if isinstance(shape, TextShape) else g.Problem(shape)
        return self.problems[shape.name]


@pytest.fixture(scope="module")
def store():
    s = Store()
    yield s
    for route, fam in sorted(s.figures.items()):
        worst = max(fam.values())
        print(f"\n[split16 schedule grads] {route}: worst E/gate {worst[0]:.3f} ({worst[1]}); per family " +
              ", ".join(f"{f} {r:.3f}" for f, (r, _) in sorted(fam.items())))
    for name, p in sorted(s.problems.items()):
        if "e_ref32" in p._refs:
            w = max(p._refs["e_ref32"].items(), key=lambda kv: kv[1])
            print(f"[split16 schedule grads] {name}: E_ref32 max {w[1]:.2e} ({w[0]})")
    print(f"[split16 schedule grads] wall time since import {time.time() - T0:.1f} s, {len(s.runs)} distinct runs")


# ------------------------------------------------------------------------------------------------ routes

ALL = None
AEFJ = ("a_everything", "e_bottom_fc2_b", "f_weights", "j_as_written")
AEFG = ("a_everything", "e_bottom_fc2_b", "f_weights", "g_biases_ln")


@dataclasses.dataclass(frozen=True)
class XRoute:
    name: str
    shape: object
    masks: tuple = ALL            # None: the whole list of the tower (+ schedule_checks.split_masks)
    pruned: bool = False          # vision: hidden_out=None, the top layer is last_layer_bwd_cls
    dystats: bool = True          # engine._VSPLIT16_DYSTATS
    drop32: bool = False          # engine._VSPLIT16_DROP32
    stale: bool = False           # a watched weight's version bumped between forward and backward
    rows_stats: bool = True       # engine._TSPLIT16_ROWS_STATS
    attn_form: str = None         # what _attention_bwd_stats_form must answer first for the dense tower on this route
    attn_site: bytes = None       # the attention backward's launch name where partials are asked for ...
    attn_plain: bytes = None      # ... and where they are not
    wgrad_plan: bool = True       # the weight-gradient plan takes the four shapes

    @property
    def tower(self):
        return self.shape.tower

    @property
    def packed(self):
        return bool(getattr(self.shape, "packed", False))

    @property
    def live(self):
        """the backward runs on the plan and the plan takes the weight gradients"""
        return self.wgrad_plan and not self.stale

    def census_kw(self):
        return dict(pruned=self.pruned, packed=self.packed, dystats=self.dystats and self.live, attn_form=self.attn_form if self.live else None,
                    wgrad_plan_ok=self.live)


V = dict(attn_form="stats", attn_site=b"attention_bwd.lean.stats", attn_plain=b"attention_bwd.lean")
X_V = XRoute("vision_dystats_pruned", g.TINY64, pruned=True, **V)
X_V3 = XRoute("vision_dystats_pruned_L3", TINY3_64, pruned=True, **V)
X_VU = XRoute("vision_dystats_unpruned", g.TINY64, masks=AEFJ, **V)
X_VOFF = XRoute("vision_dystats_switch_off", g.TINY64, masks=AEFJ, pruned=True, dystats=False, **V)
X_VDROP = XRoute("vision_dystats_drop32", g.TINY64, masks=AEFG, pruned=True, drop32=True, **V)
X_VDROP_STALE = XRoute("vision_dystats_drop32_stale", g.TINY64, masks=AEFG, pruned=True, drop32=True, stale=True, **V)
X_VSTALE = XRoute("vision_dystats_stale", g.TINY64, masks=AEFG, pruned=True, stale=True, **V)     # the pair of the one above only
X_T = XRoute("text_split16_rows_stats", TEXT77, attn_form="rows_stats", attn_site=b"attention_bwd.rows.stats", attn_plain=b"attention_bwd.rows")
X_T3 = XRoute("text_split16_rows_stats_L3", TEXT77_L3, attn_form="rows_stats", attn_site=b"attention_bwd.rows.stats", attn_plain=b"attention_bwd.rows")
X_TSEG = XRoute("text_split16_rows_stats_off", TEXT77, masks=AEFG, rows_stats=False, attn_form="segments", attn_plain=b"attention_bwd.rows")
X_TLEAN = XRoute("text_split16_lean_stats", TEXT16, **V)
X_TSTALE = XRoute("text_split16_stale", TEXT77, masks=AEFG, stale=True, attn_form="rows_stats", attn_plain=b"attention_bwd.rows")
X_P = XRoute("text_packed_split16", PACKED)
X_PODD = XRoute("text_packed_split16_249_rows", PACKED_ODD, masks=AEFG, wgrad_plan=False)

ROUTES = [X_V, X_V3, X_VU, X_VOFF, X_VDROP, X_VDROP_STALE, X_T, X_T3, X_TSEG, X_TLEAN, X_TSTALE, X_P, X_PODD]


def mask_ids(xr: XRoute):
    tower, L = xr.tower, xr.shape.L
    ids = list(sc.masks(tower, L)) + (["j_as_written"] if tower == "vision" and L == 2 else [])
    ids += list(sc.split_masks(tower, L))
    if xr.masks is not None:
        ids = [k for k in ids if k in xr.masks]
        assert len(ids) == len(xr.masks), (xr.name, ids)
    return ids


def route_masks(xr: XRoute, store: Store):
    tower, L = xr.tower, xr.shape.L
    m = dict(sc.masks(tower, L, store.freeze_sets(tower) if L == 2 else None))
    m.update(sc.split_masks(tower, L))
    return m


# ------------------------------------------------------------------------------------------------ what one run did

class Census:
    """Calls of the five ops of the census made inside linear_param_grads, the statistics-producing calls per layer (a ColStats
    handed to the kernel that makes a dY, and the launch name reported right after it), the attention backward's launch per
    layer, and what the forward kept."""

    def __init__(self, mp, rows: int):
        from dclip_amd import _lib, engine, ops
        lib = _lib.load()
        self.calls = {k: 0 for k in sc.PASS_KEYS}
        self.producers, self.producer_names, self.attn, self.varlen, self.dropped = {}, [], [], [], []
        self.layer, self.in_lpg, self.need_b, self.db_fault = None, 0, None, []
        self.stats_of, self.foreign_stats = {}, []                # address of a produced dY -> the ColStats its producer was handed
        last = lambda: lib.dclip_last_launch()                    # noqa: E731

        self.layer_index = {}                                      # ln1_w's address -> layer (bind)

        def layer_spy(name):
            orig = getattr(engine, name)

            def spy(dx2, p, *a, **kw):
                self.layer = self.layer_index[p.ln1_w.data_ptr()]
                try:
                    return orig(dx2, p, *a, **kw)
                finally:
                    self.layer = None
            mp.setattr(engine, name, spy)
        for name in ("layer_bwd", "last_layer_bwd_cls"):
            layer_spy(name)

        orig_lpg = engine.linear_param_grads

        def lpg(dy, x, need_w, need_b, gr, wkey, bkey, *a, **kw):
            self.in_lpg, self.need_b = self.in_lpg + 1, (bool(need_b), f"layers.{self.layer}.{bkey}")
            try:
                return orig_lpg(dy, x, need_w, need_b, gr, wkey, bkey, *a, **kw)
            finally:
                self.in_lpg -= 1
        mp.setattr(engine, "linear_param_grads", lpg)

        def passes(attr, key):
            orig = getattr(ops, attr)

            def spy(*a, **kw):
                assert self.in_lpg, f"{attr} was called outside linear_param_grads"
                self.calls[key] += 1
                if kw.get("db") is not None and not self.need_b[0]:
                    self.db_fault.append(self.need_b[1])          # a split pass was handed a db nobody needs
                if key == "single" and self.stats_of.pop(a[0].data_ptr(), None) is not a[1]:
                    self.foreign_stats.append(self.need_b[1])     # partials that the producer of THIS dY did not leave
                return orig(*a, **kw)
            mp.setattr(ops, attr, spy)
        passes("split_f16x3_rows_cols_stats", "single")
        passes("split_f16x3_rows_colstats", "three")

        orig_gemm, orig_colsum, orig_seg = ops.gemm, ops.colsum, ops.colsum_segments

        def gemm(a, b, layout, *rest, **kw):
            if self.in_lpg and layout == ops.LAYOUT_TN and a.shape[0] == rows:
                self.calls["plain_w"] += 1
            return orig_gemm(a, b, layout, *rest, **kw)
        mp.setattr(ops, "gemm", gemm)

        def colsum(*a, **kw):
            if self.in_lpg:
                self.calls["colsum"] += 1
            return orig_colsum(*a, **kw)
        mp.setattr(ops, "colsum", colsum)

        def colsum_segments(*a, **kw):
            assert self.in_lpg
            self.calls["segments"] += 1
            return orig_seg(*a, **kw)
        mp.setattr(ops, "colsum_segments", colsum_segments)

        def producer(attr, kind, keys=("stats",)):
            orig = getattr(ops, attr)

            def spy(*a, **kw):
                res = orig(*a, **kw)
                name = last()
                handed = any(kw.get(k) is not None for k in keys)
                assert handed == (b".stats" in name or name.startswith(b"layernorm_bwd_stats")), (attr, name, handed)
                if handed:
                    st = next(kw[k] for k in keys if kw.get(k) is not None)
                    self.stats_of[(res[0] if isinstance(res, tuple) else res).data_ptr()] = st
                    self.producers.setdefault(self.layer, {k: 0 for k in sc.PRODUCER_KINDS})[kind] += 1
                    self.producer_names.append(name)
                if attr == "attention_bwd":
                    self.attn.append((self.layer, name, bool(a[7])))
                return res
            mp.setattr(ops, attr, spy)
        producer("gemm_f16_rows_dev", "gemm")
        producer("gemm_f16x3_rows_dev", "gemm")
        producer("layernorm_bwd", "ln")
        producer("attention_bwd", "attn", ("stats", "rows_stats"))

        orig_varlen = ops.attention_varlen_causal_bwd

        def varlen(*a, **kw):
            self.varlen.append(self.layer)
            return orig_varlen(*a, **kw)
        mp.setattr(ops, "attention_varlen_causal_bwd", varlen)

        for name, idx in (("layer_fwd", (3, 10, 12)), ("last_layer_fwd_cls", (3,))):
            def fwd_spy(*a, _orig=getattr(engine, name), _idx=idx, **kw):
                out, saved = _orig(*a, **kw)
                self.dropped.append(all(saved[i] is None for i in _idx))
                return out, saved
            mp.setattr(engine, name, fwd_spy)

    def bind(self, tensors, head: int, L: int):
        self.layer_index.update({tensors[head + 12 * i].data_ptr(): i for i in range(L)})


TEXT_ROUTE = g.Route("text_split16", "text", None)                # for g._instrument: anything but kind "16"


def _run(mp, prob, xr: XRoute, mask):
    from dclip_amd import engine, ops
    mp.setattr(engine, "_VSPLIT16_DYSTATS", xr.dystats)
    mp.setattr(engine, "_VSPLIT16_DROP32", xr.drop32)
    mp.setattr(engine, "_TSPLIT16_ROWS_STATS", xr.rows_stats)
    mp.setenv("DCLIP_BF16_BIG_MIN", "1")
    shape = xr.shape
    v = prob.tcfg
    D, I, H = v.hidden_size, v.intermediate_size, v.num_attention_heads
    census = Census(mp, _rows(xr))
    if xr.tower == "vision":
        census.bind(prob.tensors, len(sc.HEAD["vision"]), shape.L)
        route = g.Route(xr.name, "fp32", shape, pruned=xr.pruned, split=(True, True, True), stale=xr.stale, env=BIG)
        got, trace = g._run(mp, prob, route, mask, None, None, True)             # asserts §26's route predicates and launch names
        S = engine._grid_seq(v, None)
        assert (engine._attention_bwd_stats_form(shape.B, S, H, False)[0] == xr.attn_form) and ops.attention_bwd_stats_plan(shape.B, S, H) > 0
    else:
        for k in ("_VSPLIT16_BWD", "_VSPLIT16_WGRAD"):
            mp.setattr(engine, k, True)
        trace = g.Trace()
        p = engine.TextParams.from_tensors(prob.tensors, shape.L)
        census.bind(prob.tensors, len(sc.HEAD["text"]), shape.L)
        g._instrument(mp, trace, p, TEXT_ROUTE)
        cache, split16 = {}, []
        if xr.packed:
            _out, saved = engine.text_fwd_packed(p, prob.x, prob.tables, v, True, split16_cache=cache, split16_out=split16)
        else:
            _out, saved = engine.text_fwd(p, prob.x, v, True, split16_cache=cache, split16_out=split16)
        assert engine._TSPLIT16_KEY in cache, "the forward did not plan the split-fp16 path"
        assert split16, "the forward handed nothing to the backward: split16_out is empty"
        assert all(len(sv) == 14 for sv in saved[1]), "the forward did not keep its split operands"
        if xr.stale:
            p.layers[0].fc1_w.add_(0.0)                            # same values, another version
            assert not split16[0].fresh()
        need = prob.need(mask)
        if xr.packed:
            grads = engine.text_bwd_packed(p, saved, prob.d_out, v, need, split16=split16[0])
        else:
            grads = engine.text_bwd(p, saved, prob.d_out, v, need, split16=split16[0])
        torch.cuda.synchronize()
        host = cache[engine._TSPLIT16_KEY]["host"]
        if host is not None:                                       # the device plan declined nothing: no guard flag (gain 2.0)
            assert not bool(host[:, ops.SPLIT16_PLAN_FLAGS].view(torch.int32).any()), "the device plan raised a flag: pick another gain"
        got = dict(zip(prob.names, grads))
        if not xr.packed:
            B, T = prob.x.shape
            form = engine._attention_bwd_stats_form(B, T, H, True)[0]
            assert form == xr.attn_form, (form, xr.attn_form)
    rows = _rows(xr)
    assert ops.gemm_f16_rows_stats_plan(rows, I, 3 * D) > 0, "the shape no longer reaches the statistics regime"
    assert engine._dystats_regime(rows, D, I) is xr.dystats
    assert (ops.gemm_f16_wgrad_tokmajor_seg3_plan(3 * D, D, rows) > 0) is xr.wgrad_plan
    _assert_xroute(xr, trace, census, mask, prob)
    return got, trace, census


def _rows(xr: XRoute):
    if xr.tower == "vision":
        return xr.shape.B * 17                                     # tiny: a 4 x 4 grid and the class token
    return xr.shape.rows


def _assert_xroute(xr: XRoute, trace, census: Census, mask, prob):
    """What proves the route, beyond §26's predicates (g._assert_route, vision): the layers run, the census, the launch names
    of the producers, the attention backward's form per layer, what the forward dropped, a stale or declined plan's launches."""
    tower, L = xr.tower, xr.shape.L
    what = f"{xr.name}"
    sc.check_layers_run(trace.layers, tower, mask, L, what)
    run_layers = sc.layers_run(tower, mask, L)
    kw = xr.census_kw()
    sc.check_census(census.calls, census.producers, tower, mask, L, what, **kw)
    assert not census.db_fault, f"{what}: a split pass was handed a db for a bias that is not needed: {census.db_fault}"
    assert not census.foreign_stats, f"{what}: a single pass finished from partials of another tensor: {census.foreign_stats}"
    assert not census.stats_of, f"{what}: statistics were produced and never consumed ({len(census.stats_of)} sets)"
    cen = sc.split_census(tower, mask, L, **kw)
    kinds = {d["producer"] for d in cen if d["producer"]}
    for kind, prefix in (("gemm", PRODUCERS[0]), ("attn", xr.attn_site), ("ln", PRODUCERS[2])):
        names = [n for n in census.producer_names if n.startswith(prefix)] if prefix else []
        assert bool(names) == (kind in kinds), (what, kind, census.producer_names)
    assert len(census.producer_names) == sum(sum(v.values()) for v in census.producers.values())
    if tower == "vision":
        assert PRODUCERS[1] == b"attention_bwd.lean.stats" and all(not causal for _, _, causal in census.attn)
        assert census.dropped == [xr.drop32] * L, census.dropped
        assert len(census.attn) == len([i for i in run_layers if not (xr.pruned and i == L - 1)])
    else:
        assert census.dropped == [False] * L
    if not xr.packed:
        qkv = {d["layer"]: d["producer"] == "attn" for d in cen if d["linear"] == "qkv"}
        for layer, name, causal in census.attn:
            assert causal == (tower == "text")
            assert name == (xr.attn_site if qkv[layer] else xr.attn_plain), (what, layer, name)
        assert not census.varlen
    else:
        assert census.varlen == run_layers and not census.attn, (census.varlen, census.attn)
        assert not any(d["linear"] == "qkv" and d["pass"] == "single" for d in cen)
    if tower == "text":
        assert bool(trace.launches("gemm_f16_dev")), trace.launch                # the forward ran on the plan
        assert bool(trace.launches("gemm_f16_rows_dev")) == (not xr.stale and bool(run_layers)), trace.launch
        wants_w = any(d["pass"] for d in cen)
        assert bool(trace.launches("gemm_f16_wgrad_tokmajor_seg3")) == wants_w, trace.launch
        assert bool(trace.launches("text_embed_bwd")) == ("tok" in mask and not xr.packed)
    if not xr.live:
        assert not census.producer_names and census.calls["single"] == census.calls["three"] == 0
        assert not trace.launches("gemm_f16_wgrad_tokmajor_seg3")
    if xr.stale:
        assert not trace.launches("gemm_f16_rows_dev"), trace.launch


def run(store: Store, xr: XRoute, mid: str):
    """One forward and backward of `xr` under mask `mid`, made once and shared: ({name: gradient or None}, Trace, Census)."""
    key = (xr.name, mid)
    if key not in store.runs:
        prob = store.problem(xr.shape)
        mask = route_masks(xr, store)[mid]
        with pytest.MonkeyPatch.context() as mp:
            store.runs[key] = _run(mp, prob, xr, mask)
    return store.runs[key]


def bias_bounds(exc, trace):
    return {n: sc.colsum_bound(*trace.colabs[n]) for n in exc}


def check_case(store: Store, xr: XRoute, mid: str):
    prob = store.problem(xr.shape)
    mask = route_masks(xr, store)[mid]
    tower, L = xr.tower, xr.shape.L
    what = f"{xr.name} {mid}"
    full, ftrace, _ = run(store, xr, "a_everything")
    got, trace, _ = run(store, xr, mid)
    sc.check_completeness(got, mask, prob.names, what)
    ratios = sc.check_anchor(got, prob.ref("r64"), sc.gates32(prob.ref("e_ref32")), what)
    store.note(xr.name, ratios)
    exc = sc.bias_exceptions(True, mask, prob.names)
    bounds = bias_bounds(exc, ftrace)
    if tower == "text" and "tok" in mask:
        exc = exc | {"tok"}
        bounds["tok"] = sc.embed_atomic_bound(prob.embed_ids, ftrace.dx[0], prob.tcfg.vocab_size)
    sc.check_mask_consistency(got, full, exc, bounds, what)
    run_layers = sc.layers_run(tower, mask, L)
    if run_layers:
        b = run_layers[-1]
        assert torch.equal(trace.dx[b], ftrace.dx[b]), f"{what}: the dx layer {b} returned differs from the full-mask run's"
    if tower == "text" and got["pos"] is not None:
        sc.check_text_pos_tail(got["pos"], xr.shape.T, what)


# ------------------------------------------------------------------------------------------------ the cases

@pytest.mark.parametrize("xr,mid", [pytest.param(r, m, id=f"{r.name}-{m}") for r in ROUTES for m in mask_ids(r)])
def test_split16_schedule_gradients(store, xr, mid):
    check_case(store, xr, mid)


def test_full_mask_census_is_what_the_tower_tests_assert():
    """{"single": 4 (L - 1), "three": 1} of test_vision_dystats_gpu.test_tower_reads_dy_once, and test_switch_on_launch_list's
    counts for the padded text tower: 4 L passes, dqkv's L among the single ones."""
    for L in (2, 3):
        full = sc.names("vision", L)
        assert sc.expected_passes("vision", full, L, **X_V.census_kw()) == \
            {"single": 4 * (L - 1), "three": 1, "plain_w": 0, "colsum": 0, "segments": 0}
        assert sc.expected_passes("vision", full, L, **X_VOFF.census_kw())["three"] == 4 * (L - 1) + 1
    t = sc.expected_passes("text", sc.names("text", L2), L2, **X_T.census_kw())
    assert t["single"] + t["three"] == 4 * L2 and t["single"] >= L2 and t == {"single": 4 * L2 - 1, "three": 1, "plain_w": 0, "colsum": 0, "segments": 0}
    s = sc.expected_passes("text", sc.names("text", L2), L2, **X_TSEG.census_kw())
    assert s["single"] + s["three"] == 4 * L2 and s["three"] >= L2 and s["segments"] == L2


@pytest.mark.parametrize("mid", AEFJ)
def test_statistics_switch_off_changes_no_weight_gradient_and_no_dx(store, mid):
    """DCLIP_VISION_SPLIT16_DYSTATS=0 under the same mask: every weight gradient (everything but the linear biases) and every
    layer's dx bit for bit; the biases, folded from the producer's partials on one side and summed by the three-launch pass or
    ops.colsum on the other, within the column-sum bound."""
    on, t_on, c_on = run(store, X_V, mid)
    off, t_off, c_off = run(store, X_VOFF, mid)
    assert not c_off.producer_names and c_off.calls["single"] == 0
    assert c_on.calls["single"] + c_on.calls["three"] == c_off.calls["three"]
    assert t_on.layers == t_off.layers and all(torch.equal(t_on.dx[i], t_off.dx[i]) for i in t_on.layers)
    for n in on:
        assert (on[n] is None) == (off[n] is None), n
        if on[n] is None:
            continue
        f = n.split(".")[-1]
        if "." in n and f.endswith("_b") and f[:-2] in sc.LINEARS:
            d = (on[n].double() - off[n].double()).abs()
            assert bool((d <= sc.colsum_bound(*t_on.colabs[n]).to(d.device)).all()), f"{mid}: {n} beyond the column-sum bound"
        else:
            assert torch.equal(on[n], off[n]), f"{mid}: {n} changes with the statistics switch"


@pytest.mark.parametrize("mid", AEFG)
def test_rows_stats_switch_off_changes_no_gradient(store, mid):
    """§30's claim under partial masks: with DCLIP_TEXT_SPLIT16_ROWS_STATS=0 every gradient but tok (float atomics) is bit-equal
    to the statistics twin's run of the same mask."""
    on, t_on, _ = run(store, X_T, mid)
    off, t_off, c_off = run(store, X_TSEG, mid)
    assert not any(n.startswith(b"attention_bwd") for n in c_off.producer_names)
    assert all(torch.equal(t_on.dx[i], t_off.dx[i]) for i in t_on.layers)
    for n in on:
        assert (on[n] is None) == (off[n] is None), n
        if on[n] is not None and n != "tok":
            assert torch.equal(on[n], off[n]), f"{mid}: {n} changes with DCLIP_TEXT_SPLIT16_ROWS_STATS"


@pytest.mark.parametrize("mid", AEFG)
def test_dropped_fp32_operands_change_no_gradient(store, mid):
    """_VSPLIT16_DROP32: what the forward leaves out is read by no fresh backward and made again, bit for bit, by a stale one."""
    for a, b in ((X_VDROP, X_V), (X_VDROP_STALE, X_VSTALE)):
        got, trace, _ = run(store, a, mid)
        want, wtrace, _ = run(store, b, mid)
        for n in got:
            assert (got[n] is None) == (want[n] is None) and (got[n] is None or torch.equal(got[n], want[n])), n
        assert all(torch.equal(trace.dx[i], wtrace.dx[i]) for i in trace.layers)
