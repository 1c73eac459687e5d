"""The TRAINABLE fp32 text tower on the split-fp16 MFMAs (`text_train_split16`), padded and packed: the launch
list with the switch on and off, run-to-run bits, the project's two error bars (§9e / §9f) against the switch-off path and the
fp64 oracle, the declined weight-gradient plan, the attention statistics switch, a partially frozen tower, a parameter written
between forward and backward, and one training step of the as-written freeze set with both towers' plans alive."""
import argparse
import re

import pytest
import torch

from dclip_amd import config as dcfg, synth
from dclip_amd.clip_model import from_hf_state_dict, packed_text_tables
from tests import schedule_checks as sc

pytestmark = pytest.mark.gpu

L = 2
B = 64                                  # 64 x 77 = 4,928 rows, a multiple of 64: every full-size weight gradient takes the plan
TOK = "tok"                             # its gradient is summed with float atomics: not the same bits from run to run
FWD = ("gemm_f16x3_dev", "gemm_f16_dev")
DGRAD = ("gemm_f16x3_rows_dev", "gemm_f16_rows_dev")
WGRAD = ("gemm_f16x3_wgrad_tokmajor", "gemm_f16_wgrad_tokmajor_seg3")
PASSES = ("split_f16x3_rows_cols_stats", "split_f16x3_rows_colstats")
SPLIT_NAMES = re.compile(rb"gemm_f16|split_f32_f16|split16_|layernorm_fwd_f16|\.stats")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def make_ids(cfg, lens, seed=5):
    """[N, seq] ids: BOS, words, the first EOS at lens[n] - 1, EOS pads (a caption of length 1 is the EOS alone)."""
    t = cfg.text
    g = torch.Generator().manual_seed(seed)
    ids = torch.full((len(lens), t.max_position_embeddings), t.eos_token_id, dtype=torch.int64)
    for n, S in enumerate(lens):
        if S > 1:
            ids[n, :S - 1] = torch.randint(0, min(t.bos_token_id, t.eos_token_id), (S - 1,), generator=g)
            ids[n, 0] = t.bos_token_id
    assert packed_text_tables(ids, t.eos_token_id)["lens"].tolist() == list(lens)
    return ids


class Problem:
    """config.tiny(seq=77), gain 2.0, N captions of `lens`; the fp64 oracle's output and gradients under a random probe.  Made
    once per shape, never written."""

    def __init__(self, dev, lens, seed):
        from oracle import dclip_oracle as O
        self.dev = dev
        self.cfg = dcfg.tiny(seq=77)
        self.t = self.cfg.text
        self.lens = list(lens)
        self.sd = synth.synth_clip_state_dict(self.cfg, seed=7, gain=2.0)
        self.ids = make_ids(self.cfg, lens, seed)
        self.ids_dev = self.ids.to(dev)
        self.names = sc.names("text", L)
        self.W64 = sc.output_weighting((len(lens), self.cfg.projection_dim))
        self.d_out = self.W64.float().to(dev)
        self.want = sc.reference("text", self.t, self.sd, self.ids, self.W64)
        with torch.no_grad():
            txt = {k: v for k, v in self.sd.items() if k.startswith("text_")}
            self.want_out = O.text_tower(O.to_dtype(txt, torch.float64), self.ids, self.t).double()

    def model(self, on):
        m = from_hf_state_dict(self.cfg, self.sd, device=self.dev)
        m.text_train_split16 = bool(on)
        return m


def padded_lens():
    """EOS at mixed positions, positions 1 and 76 among them (length = position + 1)"""
    g = torch.Generator().manual_seed(3)
    lens = torch.randint(3, 77, (B,), generator=g).tolist()
    lens[0], lens[1], lens[2], lens[3] = 2, 77, 65, 64
    return lens


@pytest.fixture(scope="module")
def prob(dev):
    return Problem(dev, padded_lens(), 5)


@pytest.fixture(scope="module")
def prob4(dev):
    return Problem(dev, [2, 77, 30, 65], 6)            # 4 x 77 = 308 rows: not a multiple of 64


PACKED_LENS = [1, 2, 64, 65, 77, 47]                   # 256 rows; one row, one word, a full tile, one row past it, the table's end
PACKED_LENS_ODD = [1, 2, 64, 65, 77, 40]               # 249 rows: not a multiple of 64


@pytest.fixture(scope="module")
def packed(dev):
    return Problem(dev, PACKED_LENS, 8)


@pytest.fixture(scope="module")
def packed_odd(dev):
    return Problem(dev, PACKED_LENS_ODD, 9)


class Spy:
    """launch names (the library's last launch after every checked call) and calls per ops entry during a block"""

    def __init__(self, mp, big_rows=None):
        from dclip_amd import _lib, ops
        self.names, self.calls, self.big_gemms, self.varlen_dqkv, self.dqkv_abs = [], {}, [], [], []
        lib, real = _lib.load(), _lib.check

        def check(rc, what=""):
            self.names.append(lib.dclip_last_launch())
            return real(rc, what)
        mp.setattr(_lib, "check", check)
        for attr in FWD + DGRAD + WGRAD + PASSES + ("split_f16x3_rows", "split_f16x3_dev"):
            def spy(*a, _orig=getattr(ops, attr), _key=attr, **kw):
                self.calls[_key] = self.calls.get(_key, 0) + 1
                return _orig(*a, **kw)
            mp.setattr(ops, attr, spy)

        def gemm(a, w, *rest, _orig=ops.gemm, **kw):
            if big_rows is not None and a.shape[0] == big_rows:        # forward, dgrad and wgrad all have the token rows in a
                self.big_gemms.append((tuple(a.shape), tuple(w.shape)))
            return _orig(a, w, *rest, **kw)
        mp.setattr(ops, "gemm", gemm)

        def attn_bwd(*a, _orig=ops.attention_bwd, **kw):
            d = _orig(*a, **kw)
            self.dqkv_abs.append((d.shape[0], d.abs().sum(0, dtype=torch.float64)))
            return d
        mp.setattr(ops, "attention_bwd", attn_bwd)

        def varlen_bwd(*a, _orig=ops.attention_varlen_causal_bwd, **kw):
            d = _orig(*a, **kw)
            self.varlen_dqkv.append(d.clone())
            return d
        mp.setattr(ops, "attention_varlen_causal_bwd", varlen_bwd)

    def n(self, group):
        return sum(self.calls.get(k, 0) for k in group)

    def count(self, name):
        return sum(x == name for x in self.names)


def run(prob, model, packed_lens=None, spy_rows=None, between=None):
    """one gradient-enabled forward and backward through the public call -> (features, {engine name: gradient or None}, Spy)"""
    for q in model.parameters():
        q.grad = None
    kw = {} if packed_lens is None else {"packed_lens": packed_lens, "packed_train": True}
    with pytest.MonkeyPatch.context() as mp:
        spy = Spy(mp, spy_rows)
        feat = model.get_text_features(input_ids=prob.ids_dev, **kw)
        if between is not None:
            between()
        (feat * prob.d_out).sum().backward()
        torch.cuda.synchronize()
    p = model.text_params()
    grads = {n: (None if t.grad is None else t.grad.detach().clone()) for n, t in zip(p.names(), p.tensors())}
    return feat.detach(), grads, spy


def norm_err(got, want):
    got, want = got.detach().double().cpu().reshape(-1), want.detach().double().cpu().reshape(-1)
    return float((got - want).norm() / want.norm())


def grad_bars(prob, on, off, tag, names=None):
    """The project's bars of §9e / §9f: every parameter gradient — tok, pos and the biases included — within 1e-5 of the
    switch-off path norm-wise, and its error against fp64 at most 4x the switch-off path's own."""
    worst_d, worst_r, bad = (0.0, ""), (0.0, ""), []
    for n in (prob.names if names is None else names):
        d = norm_err(on[n], off[n])
        es, ep = norm_err(on[n], prob.want[n]), norm_err(off[n], prob.want[n])
        worst_d, worst_r = max(worst_d, (d, n)), max(worst_r, (es / ep, n))
        if d > 1e-5 or es > 4 * ep:
            bad.append((n, d, es, ep))
    print(f"{tag}: worst gradient on vs off {worst_d[0]:.3e} ({worst_d[1]}); worst ratio of errors against fp64 {worst_r[0]:.2f} "
          f"({worst_r[1]})")
    assert not bad, (tag, bad)


def row_bars(prob, on, off, tag, names=None):
    """§9f's per-row bar for the 2-D layer weights: every ROW of the gradient, relative to that row's own size, at most 4x the
    switch-off path's error against fp64."""
    worst, bad = (0.0, ""), []
    for n in (prob.names if names is None else names):
        w = prob.want[n]
        if w.dim() != 2 or not n.startswith("layers."):
            continue

        def row_rel(x):
            d, s = (x.double().cpu().reshape(w.shape) - w).abs().amax(dim=1), w.abs().amax(dim=1)
            return float((d[s > 0] / s[s > 0]).max())
        es, ep = row_rel(on[n]), row_rel(off[n])
        worst = max(worst, (es / ep, n))
        if es > 4 * ep:
            bad.append((n, es, ep))
    print(f"{tag}: worst per-row ratio on / off against fp64 {worst[0]:.2f} ({worst[1]})")
    assert not bad, (tag, bad)


def same_but_tok(a, b):
    return all((a[n] is None and b[n] is None) or torch.equal(a[n], b[n]) for n in a if n != TOK)


def tok_close(prob, a, b):
    """two sums of the same terms in another order (float atomics): far inside the 1e-5 bar"""
    return norm_err(a[TOK], b[TOK]) <= 1e-5


# ------------------------------------------------------------------------------------------------ the padded tower

@pytest.fixture(scope="module")
def runs(prob):
    """the switch on (twice) and off at B = 64 with the tower's GEMMs on the ping-pong kernel, as the flagship's are
    (DCLIP_BF16_BIG_MIN = 1: the register-staged kernels have no statistics form); shared, never written"""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("DCLIP_BF16_BIG_MIN", "1")
        m_on, m_off = prob.model(True), prob.model(False)
        on = run(prob, m_on, spy_rows=B * 77)
        on2 = run(prob, m_on)
        off = run(prob, m_off, spy_rows=B * 77)
    return on, on2, off


def test_switch_on_launch_list(prob, runs):
    (feat, grads, spy), _, _ = runs
    assert not spy.big_gemms, spy.big_gemms                            # no fp32 GEMM of a full-size layer shape
    assert spy.n(FWD) == 4 * L and spy.n(DGRAD) == 4 * L and spy.n(WGRAD) == 4 * L, spy.calls
    assert spy.count(b"attention_bwd.rows.stats") == L and spy.count(b"attention_bwd.rows") == 0, spy.names
    assert spy.n(PASSES) == 4 * L and spy.calls.get("split_f16x3_rows", 0) == 0, spy.calls     # one split pass per dY
    assert spy.calls.get("split_f16x3_rows_cols_stats", 0) >= L                                  # dqkv's among them
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads.values())


def test_two_runs_are_bit_identical(prob, runs):
    (feat, grads, _), (feat2, grads2, _), _ = runs
    assert torch.equal(feat, feat2) and same_but_tok(grads, grads2) and tok_close(prob, grads, grads2)


def test_switch_off_is_the_plain_schedule(prob, runs, dev):
    from dclip_amd import engine
    _, _, (feat, grads, spy) = runs
    assert not any(SPLIT_NAMES.search(n) for n in spy.names), spy.names
    assert spy.n(FWD) + spy.n(DGRAD) + spy.n(WGRAD) + spy.n(PASSES) == 0 and len(spy.big_gemms) == 12 * L
    assert spy.count(b"attention_bwd.rows") == L
    # the schedule functions called as before the switch existed: the same launches, the same bits
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("DCLIP_BF16_BIG_MIN", "1")
        direct = Spy(mp)
        p = engine.TextParams.from_tensors(sc.engine_tensors("text", L, prob.sd, dev), L)
        out, saved = engine.text_fwd(p, prob.ids_dev, prob.t, True)
        g = dict(zip(prob.names, engine.text_bwd(p, saved, prob.d_out, prob.t, [True] * len(prob.names))))
        torch.cuda.synchronize()
    assert torch.equal(out, feat)
    assert direct.names == spy.names
    assert same_but_tok(g, grads) and tok_close(prob, g, grads)


def test_error_bars(prob, runs):
    (feat_on, g_on, _), _, (feat_off, g_off, _) = runs
    assert not same_but_tok(g_on, g_off)
    grad_bars(prob, g_on, g_off, "text tiny B 64")
    row_bars(prob, g_on, g_off, "text tiny B 64")
    e_on, e_off = norm_err(feat_on, prob.want_out), norm_err(feat_off, prob.want_out)
    print(f"text tiny B 64: features against fp64 on {e_on:.3e}, off {e_off:.3e}")
    assert e_on <= 4 * e_off, (e_on, e_off)


@pytest.fixture(scope="module")
def rows_stats_off(prob):
    """the switch on with DCLIP_TEXT_SPLIT16_ROWS_STATS = 0 (read once at import: the module attribute is what it sets)"""
    from dclip_amd import engine
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("DCLIP_BF16_BIG_MIN", "1")
        mp.setattr(engine, "_TSPLIT16_ROWS_STATS", False)
        return run(prob, prob.model(True))


def test_rows_stats_switch_off_gives_the_same_gradients(prob, runs, rows_stats_off):
    """With DCLIP_TEXT_SPLIT16_ROWS_STATS=0 dqkv takes the three-launch split, and every gradient is bit-identical to the
    statistics form: dqkv and its two splits are the same bits in both, and qkv_b — which the single pass folds from the producer's
    per-caption partials — is summed per caption and folded the same way by ops.colsum_segments in the form without them.  tok apart:
    float atomics, not the same bits in any two runs."""
    (feat, grads, _), _, _ = runs
    feat0, grads0, spy = rows_stats_off
    assert spy.count(b"attention_bwd.rows.stats") == 0 and spy.count(b"attention_bwd.rows") == L
    assert spy.count(b"colsum_segments_f32.finish") == L
    assert spy.n(PASSES) == 4 * L and spy.calls.get("split_f16x3_rows_colstats", 0) >= L and spy.calls.get("split_f16x3_rows", 0) == 0
    assert torch.equal(feat0, feat)
    differ = [n for n in grads if n != TOK and not torch.equal(grads[n], grads0[n])]
    print("DCLIP_TEXT_SPLIT16_ROWS_STATS=0: gradients that differ from the statistics form:", differ)
    assert not differ and tok_close(prob, grads, grads0)


def test_rows_stats_switch_off_qkv_bias_bit_identical(prob, runs, rows_stats_off):
    """the qkv bias gradients alone: the one kind of gradient whose association depends on who summed it (the producer's
    per-caption partials or a pass over dqkv) is the same bits with the statistics form on and off"""
    (_, grads, _), _, _ = runs
    _, grads0, _ = rows_stats_off
    differ = [n for n in grads if n.endswith(".qkv_b") and not torch.equal(grads[n], grads0[n])]
    print("DCLIP_TEXT_SPLIT16_ROWS_STATS=0: qkv bias gradients that differ from the statistics form:",
          {n: f"{norm_err(grads[n], grads0[n]):.3e}" for n in differ})
    assert not differ and all(float(grads[n].abs().max()) > 0 for n in grads if n.endswith(".qkv_b"))


def test_declined_wgrad_plan_takes_the_fp32_wgrads(prob4, monkeypatch):
    """B = 4 (308 rows, not a multiple of 64): the weight-gradient plan declines — the step is the one with the weight-gradient
    switch off, bit for bit — and the forwards and data gradients still split"""
    from dclip_amd import engine
    m = prob4.model(True)
    feat, grads, spy = run(prob4, m, spy_rows=4 * 77)
    assert spy.n(WGRAD) == 0 and spy.n(PASSES) == 0 and spy.n(FWD) == 4 * L and spy.n(DGRAD) == 4 * L, spy.calls
    assert len(spy.big_gemms) == 4 * L, spy.big_gemms                     # the fp32 weight gradients
    monkeypatch.setattr(engine, "_VSPLIT16_WGRAD", False)
    feat_w, grads_w, spy_w = run(prob4, m)
    core = lambda names: [n for n in names if not n.startswith(b"split16_")]      # noqa: E731  (but for the table's refresh)
    assert core(spy_w.names) == core(spy.names)
    assert torch.equal(feat, feat_w) and same_but_tok(grads, grads_w) and tok_close(prob4, grads, grads_w)
    monkeypatch.setattr(engine, "_VSPLIT16_WGRAD", True)
    _, grads_off, _ = run(prob4, prob4.model(False))
    grad_bars(prob4, grads, grads_off, "text tiny B 4 (declined)")


@pytest.mark.parametrize("which", ["padded", "packed"])
def test_partially_frozen_tower(which, prob, packed, monkeypatch):
    """only the top layer and the projection train: frozen tensors get no gradient, the bars hold for the rest, and the backward
    stops above layer 0 — on the padded tower (B = 64) and on the packed one (PACKED_LENS, 256 rows), whose layer loop is the
    same one"""
    monkeypatch.setenv("DCLIP_BF16_BIG_MIN", "1")
    pr = prob if which == "padded" else packed
    kw = {} if which == "padded" else {"packed_lens": packed_text_tables(pr.ids, pr.t.eos_token_id)["lens"]}
    tag = ("text tiny B 64" if which == "padded" else "packed text tiny, 256 rows") + ", top layer + projection"
    live = [n for n in pr.names if n.startswith(f"layers.{L - 1}.") or n == "proj_w"]
    out = {}
    for on in (True, False):
        m = pr.model(on)
        p = m.text_params()
        for n, t in zip(p.names(), p.tensors()):
            t.requires_grad_(n in live)
        out[on] = run(pr, m, **kw)
    (_, g_on, spy), (_, g_off, _) = out[True], out[False]
    assert all((g_on[n] is None) == (n not in live) for n in pr.names), [n for n in pr.names if g_on[n] is not None]
    assert spy.n(FWD) == 4 * L and spy.n(DGRAD) == 4 and spy.n(WGRAD) == 4, spy.calls     # the backward stops below the top layer
    grad_bars(pr, g_on, g_off, tag, live)
    row_bars(pr, g_on, g_off, tag, live)


def test_parameter_written_between_forward_and_backward(prob, monkeypatch):
    monkeypatch.setenv("DCLIP_BF16_BIG_MIN", "1")
    m = prob.model(True)
    run(prob, m)                                                          # the plan exists

    def bump():
        with torch.no_grad():
            m.text_model.encoder.layers[0].layer_norm1.bias.add_(0.0)     # a version bump, same values
    feat, grads, spy = run(prob, m, between=bump)
    assert spy.n(FWD) == 4 * L and spy.n(DGRAD) == 0 and spy.n(WGRAD) == 0, spy.calls      # Split16Bwd.fresh said no
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    _, grads_off, _ = run(prob, prob.model(False))
    grad_bars(prob, grads, grads_off, "text tiny B 64, stale weights")


@pytest.mark.parametrize("which", ["padded", "packed"])
def test_stale_weights_with_dropped_fp32_operands(which, prob, packed, monkeypatch):
    """DCLIP_VISION_SPLIT16_DROP32=1 acts on the text path as on the vision path: the forward on the plan leaves out the fp32
    ln1 / ln2 / g wherever the weight gradient has a split plan.  A weight written before the backward sends that backward down
    the plain fp32 GEMMs, which make those operands again (eps reaches layer_bwd on that path too): the gradients are those of
    the same stale backward with the operands stored, bit for bit."""
    from dclip_amd import engine
    pr = prob if which == "padded" else packed
    kw = {} if which == "padded" else {"packed_lens": packed_text_tables(pr.ids, pr.t.eos_token_id)["lens"]}
    monkeypatch.setenv("DCLIP_BF16_BIG_MIN", "1")
    out = {}
    for drop32 in (False, True):
        monkeypatch.setattr(engine, "_VSPLIT16_DROP32", drop32)
        m = pr.model(True)
        run(pr, m, **kw)                                                  # the plan exists
        dropped = []
        orig = engine.layer_fwd

        def fwd_spy(*a, _orig=orig, **k):
            x2, saved = _orig(*a, **k)
            dropped.append(saved[3] is None and saved[10] is None and saved[12] is None)
            return x2, saved
        monkeypatch.setattr(engine, "layer_fwd", fwd_spy)

        def bump():
            with torch.no_grad():
                m.text_model.encoder.layers[0].layer_norm1.bias.add_(0.0)
        feat, grads, spy = run(pr, m, between=bump, **kw)
        monkeypatch.setattr(engine, "layer_fwd", orig)
        assert dropped == [drop32] * L, dropped
        assert spy.n(FWD) == 4 * L and spy.n(DGRAD) == 0 and spy.n(WGRAD) == 0, spy.calls
        out[drop32] = (feat, grads)
    (feat0, g0), (feat1, g1) = out[False], out[True]
    assert torch.equal(feat0, feat1) and same_but_tok(g0, g1) and tok_close(pr, g0, g1)
    assert all(bool(torch.isfinite(g).all()) for g in g1.values())


def test_all_zero_rows_split_to_zero_pieces_and_unit_alpha(dev):
    """the top layer's incoming dx (scatter_rows) is zero in all but one row per caption"""
    from dclip_amd import engine, ops
    x = torch.zeros((128, 128), device=dev)
    x[5] = torch.randn(128, generator=torch.Generator().manual_seed(1)).to(dev)
    x[77, 3] = 2.0 ** -140
    assert engine.split16_row_exp(0.0) == 0
    for pieces in (2, 3):
        y, ra = ops.split_f16x3_rows(x, pieces=pieces)
        y2, ra2, yc, ce, ca = ops.split_f16x3_rows_colstats(x, pieces=pieces)
        zero = [r for r in range(128) if r not in (5, 77)]
        for yy, aa in ((y, ra), (y2, ra2)):
            assert bool((yy[zero].view(torch.int16) == 0).all()) and bool((aa[zero] == 1.0).all())
            assert bool(torch.isfinite(yy.float()).all()) and bool(torch.isfinite(aa).all())
            assert float(yy[5].float().abs().max()) > 0


# ------------------------------------------------------------------------------------------------ one training step

def test_as_written_training_step(dev, monkeypatch):
    """freeze_mode="as_written" trains the vision projections and the whole text tower: both towers' plans are alive in one step
    and neither refresh invalidates the other's pending backward.  The loss is within §9d's 1e-5 of the switch-off loss."""
    from dclip_amd.CLIP_image_distillation import CLIPImageDistillation
    cfg = dcfg.tiny()
    Bs, R = 4, 3
    batch = {"pixel_values": synth.synth_pixel_values(Bs, cfg.vision, seed=11),
             "input_ids": synth.synth_input_ids(Bs, cfg.text, seed=13, ragged=True),
             "regions": synth.synth_regions(Bs, R, cfg.vision, seed=12), "region_counts": torch.tensor([3, 1, 0, 2]),
             "teacher_text_emb": synth.synth_embeddings(Bs, cfg.projection_dim, seed=14)}

    def module(**kw):
        hp = argparse.Namespace(learning_rate=1e-4, warmup_steps=0, total_steps=100, train_batch_size=Bs, eval_batch_size=Bs)
        student = from_hf_state_dict(cfg, synth.synth_clip_state_dict(cfg, seed=0, gain=2.0), device=dev)
        mod = CLIPImageDistillation(hp, student, None, freeze_mode="as_written", **kw).to(dev)
        cm = synth.synth_cross_modal_state_dict(cfg.projection_dim, seed=31)
        mod.teacher.load_state_dict({f"cross_modal_attention.{k}": v for k, v in cm.items()})
        return mod

    def step(mod):
        for q in mod.parameters():
            q.grad = None
        with pytest.MonkeyPatch.context() as mp:
            spy = Spy(mp)
            loss = mod.training_step(batch)
            loss.backward()
            torch.cuda.synchronize()
        grads = {k: q.grad.detach().clone() for k, q in mod.student.named_parameters() if q.grad is not None}
        return loss.detach(), grads, spy

    on, off = module(text_train_split16=True), module()
    assert on.text_train_split16 is True and off.text_train_split16 is False and off.student.text_train_split16 is False
    l_off, g_off, s_off = step(off)
    for rnd_i in range(2):                                  # the second step refreshes neither plan: nothing was written
        l_on, g_on, s_on = step(on)
        assert on.student.text_train_split16 is True
        Lv, Lt = cfg.vision.num_hidden_layers, cfg.text.num_hidden_layers
        assert s_on.n(DGRAD) == s_off.n(DGRAD) + 4 * Lt and s_off.n(DGRAD) == 4 * (Lv - 1) + 1, (s_on.calls, s_off.calls)
        assert s_on.n(FWD) == s_off.n(FWD) + 4 * Lt
        rel = abs(float(l_on) - float(l_off)) / abs(float(l_off))
        print(f"as_written step {rnd_i}: loss on {float(l_on):.8f} off {float(l_off):.8f} rel {rel:.2e}")
        assert rel <= 1e-5
        # norm-wise against the switch-off gradient, except where that gradient is zero in exact arithmetic and both paths return
        # rounding noise (the key bias: softmax does not see a shift of a row's logits, §9d; a tensor that is all zero): those
        # are held to the size of the noise instead, 1e-5 of the largest gradient entry of the step
        assert set(g_on) == set(g_off)
        top = max(float(g.abs().max()) for g in g_off.values())
        for k in g_off:
            assert bool(torch.isfinite(g_on[k]).all()), k
            if float(g_off[k].abs().max()) > 0 and not k.endswith("k_proj.bias"):
                assert norm_err(g_on[k], g_off[k]) <= 1e-5, k
            else:
                assert float((g_on[k] - g_off[k]).abs().max()) <= 1e-5 * top, k
    assert set(on.student._tsplit16_train_cache()) == {"__tsplit16__"} and set(on.student._vsplit16_cache()) == {"__vsplit16__"}
    assert not off.student._tsplit16_train_cache()


# ------------------------------------------------------------------------------------------------ packed captions

def run_packed_pair(prob):
    tab = packed_text_tables(prob.ids, prob.t.eos_token_id)
    assert tab["lens"].tolist() == prob.lens and tab["Tp"] == sum(prob.lens)
    on = run(prob, prob.model(True), packed_lens=tab["lens"], spy_rows=tab["Tp"])
    off = run(prob, prob.model(False), packed_lens=tab["lens"], spy_rows=tab["Tp"])
    return on, off


def test_packed_tower_on_the_split_plan(packed):
    (feat_on, g_on, spy), (feat_off, g_off, spy_off) = run_packed_pair(packed)
    assert sum(packed.lens) % 64 == 0
    assert not spy.big_gemms and spy.n(FWD) == 4 * L and spy.n(DGRAD) == 4 * L and spy.n(WGRAD) == 4 * L, (spy.calls, spy.big_gemms)
    assert spy.calls.get("split_f16x3_dev", 0) >= L                       # the ragged attention's context is split after it
    assert spy.count(b"attention_bwd.rows.stats") == 0 and not any(n.startswith(b"attention_bwd") for n in spy.names)
    assert len(spy.varlen_dqkv) == L and spy.n(PASSES) == 4 * L and spy.calls.get("split_f16x3_rows", 0) == 0
    D = packed.t.hidden_size
    for d in spy.varlen_dqkv:                                             # caption 0 is one row: dq and dk are exact zeros
        assert packed.lens[0] == 1 and bool((d[0, :2 * D] == 0).all())
    assert not any(SPLIT_NAMES.search(n) for n in spy_off.names) and len(spy_off.big_gemms) == 12 * L
    grad_bars(packed, g_on, g_off, "packed text tiny, 256 rows")
    row_bars(packed, g_on, g_off, "packed text tiny, 256 rows")
    e_on, e_off = norm_err(feat_on, packed.want_out), norm_err(feat_off, packed.want_out)
    assert e_on <= 4 * e_off, (e_on, e_off)


def test_packed_rows_not_a_multiple_of_64_take_the_fp32_wgrads(packed_odd):
    (feat_on, g_on, spy), (feat_off, g_off, _) = run_packed_pair(packed_odd)
    assert sum(packed_odd.lens) % 64 != 0
    assert spy.n(WGRAD) == 0 and spy.n(PASSES) == 0 and len(spy.big_gemms) == 4 * L, (spy.calls, spy.big_gemms)
    assert spy.n(FWD) == 4 * L and spy.n(DGRAD) == 4 * L
    grad_bars(packed_odd, g_on, g_off, "packed text tiny, 249 rows")
