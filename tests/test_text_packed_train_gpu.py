"""The TRAINABLE text tower on packed captions: engine.text_fwd_packed / text_bwd_packed against the fp64
oracle on the padded ids (§26's gate, which the padded text_fwd / text_bwd must pass in the same test), under partial `need`
masks, from run to run and from caption to caption; HipCLIPModel.get_text_features(packed_train=True); and the training step
with `packed_text_train` against the padded step: losses, gradients, the launch list, and the cases in which the padded path
must still run."""
import argparse

import pytest
import torch

from dclip_amd import config as dcfg, synth
from dclip_amd.clip_model import from_hf_state_dict, packed_text_tables
from tests import schedule_checks as sc
from tests.test_fullres_packed_gpu import Census

pytestmark = pytest.mark.gpu

LENS = [2, 3, 17, 64, 65, 80]                 # one row of words; inside one tile; a full tile; one row into the second; the table's end
NEW_SITES = {"attention_varlen_causal_bwd", "text_embed_varlen_bwd", "scatter_last_rows"}
L = 2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def sites(census):
    return {s.split(".")[0] for s in census.names}


def make_ids(cfg, lens, seed=5):
    """[N, seq] ids: BOS, words, EOS at lens[n] - 1, EOS pads; word ids repeat inside a caption and across captions."""
    t = cfg.text
    g = torch.Generator().manual_seed(seed)
    ids = torch.full((len(lens), t.max_position_embeddings), t.eos_token_id, dtype=torch.int64)
    for n, S in enumerate(lens):
        ids[n, :S - 1] = torch.randint(0, min(t.bos_token_id, t.eos_token_id), (S - 1,), generator=g)
        ids[n, 0] = t.bos_token_id
    ids[2, 2] = ids[2, 1]
    ids[3, 1] = ids[2, 1]
    assert packed_text_tables(ids, t.eos_token_id)["lens"].tolist() == list(lens)
    return ids


class Problem:
    """The case of the issue: tiny(seq=80), two layers, gain 2.0, six captions of LENS.  Made once, never written."""

    def __init__(self, dev):
        self.cfg = dcfg.tiny(seq=80)
        self.t = self.cfg.text
        self.sd = synth.synth_clip_state_dict(self.cfg, seed=7, gain=2.0)
        self.ids = make_ids(self.cfg, LENS)
        self.ids_dev = self.ids.to(dev)
        self.names = sc.names("text", L)
        self.W64 = sc.output_weighting((len(LENS), self.cfg.projection_dim))
        self.d_out = self.W64.float().to(dev)
        self.tensors = sc.engine_tensors("text", L, self.sd, dev)
        tab = packed_text_tables(self.ids, self.t.eos_token_id)
        tab["cu_seqlens_dev"], tab["last_rows_dev"] = tab["cu_seqlens"].to(dev), tab["last_rows"].to(dev)
        self.tables = tab
        self.packed_ids = torch.cat([self.ids[n, :S] for n, S in enumerate(LENS)])
        # fp64 oracle on the PADDED ids, and the same oracle evaluated in fp32 (E_ref32): gradients and the output
        from oracle import dclip_oracle as O
        self.want = sc.reference("text", self.t, self.sd, self.ids, self.W64)
        ref32 = sc.reference("text", self.t, self.sd, self.ids, self.W64, dtype=torch.float32)
        with torch.no_grad():
            txt = {k: v for k, v in self.sd.items() if k.startswith("text_")}
            self.want["out"] = O.text_tower(O.to_dtype(txt, torch.float64), self.ids, self.t).double()
            ref32["out"] = O.text_tower(O.to_dtype(txt, torch.float32), self.ids, self.t).double()
        self.e_ref32 = sc.errors(ref32, self.want)
        self.gate = sc.gates32(self.e_ref32)

    def params(self):
        from dclip_amd import engine
        return engine.TextParams.from_tensors(self.tensors, L)

    def need(self, mask):
        return [n in mask for n in self.names]


@pytest.fixture(scope="module")
def prob(dev):
    return Problem(dev)


class Trace:
    def __init__(self):
        self.layers, self.dx, self.colabs, self.current = [], {}, {}, None


def run_packed(prob, mask, d_out=None, ids_dev=None, monkeypatch=None):
    """One forward and one backward of the packed tower under `mask` -> (out, {name: gradient or None}, Trace, Census)."""
    from dclip_amd import engine
    p, trace = prob.params(), Trace()
    with pytest.MonkeyPatch.context() as mp:
        index = {id(lp): i for i, lp in enumerate(p.layers)}
        orig_bwd, orig_lpg = engine.layer_bwd, engine.linear_param_grads

        def bwd_spy(dx2, lp, *a, **kw):
            assert kw.get("varlen") is not None, "the packed schedule called layer_bwd without its table"
            trace.layers.append(index[id(lp)])
            trace.current = index[id(lp)]
            res = orig_bwd(dx2, lp, *a, **kw)
            trace.dx[index[id(lp)]] = res[0]
            return res

        def lpg_spy(dy, x, need_w, need_b, gr, wkey, bkey, *a, **kw):
            trace.colabs[f"layers.{trace.current}.{bkey}"] = (dy.shape[0], dy.abs().sum(0, dtype=torch.float64))
            return orig_lpg(dy, x, need_w, need_b, gr, wkey, bkey, *a, **kw)
        mp.setattr(engine, "layer_bwd", bwd_spy)
        mp.setattr(engine, "linear_param_grads", lpg_spy)
        out, saved = engine.text_fwd_packed(p, prob.ids_dev if ids_dev is None else ids_dev, prob.tables, prob.t, True)
        with Census(mp) as census:
            grads = engine.text_bwd_packed(p, saved, prob.d_out if d_out is None else d_out, prob.t, prob.need(mask))
        torch.cuda.synchronize()
    return out, dict(zip(prob.names, grads)), trace, census


@pytest.fixture(scope="module")
def full(prob):
    """The full-mask run: made once, shared, never written."""
    return run_packed(prob, frozenset(prob.names))


def tok_bound(prob, trace):
    return sc.embed_atomic_bound(prob.packed_ids, trace.dx[0], prob.t.vocab_size)


# ------------------------------------------------------------------------------------------------ (a) fp64 oracle

def test_packed_gradients_against_the_fp64_oracle_on_the_padded_ids(dev, prob, full):
    """Gate: sc.gates32 of the fp32 oracle's own error, 8 E_ref32 + 16 * 2^-24 per tensor, for the output and
    every gradient of the packed tower AND of the padded text_fwd / text_bwd.  The packed-against-padded difference is printed,
    not gated.
    Measured on an MI355X: E_ref32 1.8e-7 ... 9.6e-7; worst E / gate packed 0.143 (layers.0.qkv_b), padded 0.137 (final_w); packed
    against padded 0 (final_b) ... 7.3e-7 (layers.0.ln1_w), output 3.8e-7."""
    from dclip_amd import engine
    out, got, trace, _ = full
    assert out.shape == (len(LENS), prob.cfg.projection_dim) and out.dtype == torch.float32
    print("E_ref32:", {n: f"{e:.2e}" for n, e in prob.e_ref32.items()})
    p = prob.params()
    pout, saved = engine.text_fwd(p, prob.ids_dev, prob.t, True)
    padded = dict(zip(prob.names, engine.text_bwd(p, saved, prob.d_out, prob.t, prob.need(prob.names))))
    torch.cuda.synchronize()
    r_padded = sc.check_anchor(dict(padded, out=pout), prob.want, prob.gate, "padded text_fwd / text_bwd")
    r_packed = sc.check_anchor(dict(got, out=out), prob.want, prob.gate, "text_fwd_packed / text_bwd_packed")
    assert set(r_packed) == set(prob.names) | {"out"}
    diff = {n: sc.rel_err(got[n], padded[n]) for n in prob.names}
    diff["out"] = sc.rel_err(out, pout)
    print("packed E / gate:", {n: f"{r:.3f}" for n, r in r_packed.items()})
    print("padded E / gate:", {n: f"{r:.3f}" for n, r in r_padded.items()})
    print("packed against padded:", {n: f"{e:.2e}" for n, e in diff.items()})
    print(f"worst E / gate: packed {max(r_packed.values()):.3f}, padded {max(r_padded.values()):.3f}; "
          f"worst packed against padded {max(diff.values()):.2e}")
    sc.check_text_pos_tail(got["pos"], prob.t.max_position_embeddings, "packed")


# ------------------------------------------------------------------------------------------------ (b) masks

def _masks(prob):
    from dclip_amd.clip_model import HipCLIPModel
    everything = frozenset(prob.names)
    as_written = sc.freeze_sets("text", L, HipCLIPModel(prob.cfg))["as_written"]
    return {"everything": everything, "as_written": as_written, "tail_only": frozenset(sc.TAIL["text"]),
            "layer_1_only": frozenset(f"layers.1.{f}" for f in sc.LAYER_FIELDS), "pos_without_tok": frozenset(["pos"]),
            "tok_without_pos": frozenset(["tok"]), "bottom_fc2_b": frozenset(["layers.0.fc2_b"])}


@pytest.mark.parametrize("mid", ["everything", "as_written", "tail_only", "layer_1_only", "pos_without_tok", "tok_without_pos",
                                 "bottom_fc2_b"])
def test_need_masks(dev, prob, full, mid):
    mask = _masks(prob)[mid]
    what = f"packed text {mid}"
    _, fgot, ftrace, _ = full
    out, got, trace, census = run_packed(prob, mask)
    sc.check_completeness(got, mask, prob.names, what)
    sc.check_anchor(got, prob.want, prob.gate, what)
    exc = sc.bias_exceptions(True, mask, prob.names)
    bounds = {n: sc.colsum_bound(*ftrace.colabs[n]) for n in exc}
    if "tok" in mask:
        exc = exc | {"tok"}
        bounds["tok"] = tok_bound(prob, ftrace)
    sc.check_mask_consistency(got, fgot, exc, bounds, what)
    sc.check_layers_run(trace.layers, "text", mask, L, what)
    if trace.layers:
        b = trace.layers[-1]
        assert torch.equal(trace.dx[b], ftrace.dx[b]), f"{what}: the dx layer {b} returned differs from the full-mask run's"
    if got["pos"] is not None:
        sc.check_text_pos_tail(got["pos"], prob.t.max_position_embeddings, what)
    names = [s.split(".")[0] for s in census.names]
    assert names.count("attention_varlen_causal_bwd") == len(sc.layers_run("text", mask, L)), names
    assert names.count("scatter_last_rows") == (1 if sc.lowest_of("text", mask) is not None else 0), names
    assert names.count("text_embed_varlen_bwd") == (1 if mask & {"tok", "pos"} else 0), names
    assert not {"attention_bwd", "text_embed_bwd", "scatter_rows"} & set(names), names
    if mid == "as_written":
        assert mask == frozenset(prob.names)                  # the product trains the whole text tower there
    if mid == "tail_only":
        assert not NEW_SITES & set(names) and not trace.layers
    if mid == "layer_1_only":
        assert trace.layers == [1] and "text_embed_varlen_bwd" not in names
    if mid == "pos_without_tok":
        assert got["tok"] is None and got["pos"] is not None


# ------------------------------------------------------------------------------------------------ (c), (d)

def test_two_runs_are_bit_equal_except_tok(dev, prob, full):
    out0, g0, t0, _ = full
    out1, g1, _, _ = run_packed(prob, frozenset(prob.names))
    assert torch.equal(out0, out1)
    for n in prob.names:
        if n != "tok":
            assert torch.equal(g0[n], g1[n]), n
    d = (g0["tok"].double() - g1["tok"].double()).abs()
    assert bool((d <= 2 * tok_bound(prob, t0).to(dev)).all())          # each run is within the bound of the exact sum


def test_changing_one_captions_words_changes_no_other_captions_gradient(dev, prob):
    """Only the OTHER captions' output rows are weighted: the victim's rows then carry exact zeros through the whole backward,
    and every gradient except tok (atomics) is bit-identical whatever its words are."""
    victim = 3
    changed = prob.ids.clone()
    words = slice(1, LENS[victim] - 1)
    changed[victim, words] = (changed[victim, words] + 1) % min(prob.t.bos_token_id, prob.t.eos_token_id)
    assert packed_text_tables(changed, prob.t.eos_token_id)["lens"].tolist() == LENS and not torch.equal(changed, prob.ids)
    d_out = prob.d_out.clone()
    d_out[victim] = 0
    out0, g0, _, _ = run_packed(prob, frozenset(prob.names), d_out=d_out)
    out1, g1, _, _ = run_packed(prob, frozenset(prob.names), d_out=d_out, ids_dev=changed.to(dev))
    keep = [n for n in range(len(LENS)) if n != victim]
    assert not torch.equal(out0[victim], out1[victim]) and torch.equal(out0[keep], out1[keep])
    for n in prob.names:
        assert bool(torch.isfinite(g1[n]).all()), n
        if n != "tok":
            assert torch.equal(g0[n], g1[n]), n


# ------------------------------------------------------------------------------------------------ (e) public surface

def test_get_text_features_packed_train(dev, prob, full, monkeypatch):
    out, fgot, ftrace, _ = full
    m = from_hf_state_dict(prob.cfg, prob.sd, device=dev)
    lens = prob.tables["lens"]
    with Census(monkeypatch) as c:
        got = m.get_text_features(input_ids=prob.ids_dev, packed_lens=lens, packed_train=True)
        assert got.requires_grad and torch.equal(got, out)
        (got * prob.d_out).sum().backward()
    torch.cuda.synchronize()
    assert NEW_SITES <= sites(c) and not {"text_embed_fwd", "first_eos", "text_embed_bwd", "scatter_rows", "attention_bwd"} & sites(c)
    p = m.text_params()
    bound = tok_bound(prob, ftrace).to(dev)
    for n, t in zip(p.names(), p.tensors()):
        assert t.grad is not None, n
        if n == "tok":
            assert bool(((t.grad.double() - fgot[n].double()).abs() <= 2 * bound).all())
        else:
            assert torch.equal(t.grad, fgot[n]), n
    assert torch.equal(m.get_text_features(input_ids=prob.ids, packed_lens=True, packed_train=True), out)      # host ids
    # without the switch: today's refusal, word for word
    with pytest.raises(RuntimeError, match="packed_lens is a forward-only path for frozen towers: call it under torch.no_grad"):
        m.get_text_features(input_ids=prob.ids_dev, packed_lens=lens)
    with pytest.raises(RuntimeError, match="packed_lens is a forward-only path for frozen towers: call it under torch.no_grad"):
        m.get_text_features(input_ids=prob.ids_dev, packed_lens=lens, packed_train=False)
    # a 16-bit precision under grad: forward only
    for prec in ("bf16", "fp16"):
        with pytest.raises(RuntimeError, match="forward-only path for frozen towers: call it under torch.no_grad"):
            m.get_text_features(input_ids=prob.ids_dev, packed_lens=lens, packed_train=True, precision=prec)
    # under no_grad the switch changes nothing
    with torch.no_grad():
        a = m.get_text_features(input_ids=prob.ids_dev, packed_lens=lens)
        with Census(monkeypatch) as c:
            b = m.get_text_features(input_ids=prob.ids_dev, packed_lens=lens, packed_train=True)
        assert torch.equal(a, b) and not b.requires_grad and "attention_varlen_causal_fwd" in sites(c)
    # a frozen tower under grad: the frozen packed path, as without the switch
    frozen = from_hf_state_dict(prob.cfg, prob.sd, device=dev).requires_grad_(False)
    assert torch.equal(frozen.get_text_features(input_ids=prob.ids_dev, packed_lens=lens, packed_train=True),
                       frozen.get_text_features(input_ids=prob.ids_dev, packed_lens=lens))


def test_under_capture_the_padded_trainable_path_runs(dev, prob, monkeypatch):
    m = from_hf_state_dict(prob.cfg, prob.sd, device=dev)
    lens = prob.tables["lens"]
    eager = m.get_text_features(input_ids=prob.ids_dev).detach()          # warm-up: the workspace is sized before the capture
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    graph = torch.cuda.CUDAGraph()
    with Census(monkeypatch) as c:
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                captured = m.get_text_features(input_ids=prob.ids_dev, packed_lens=lens, packed_train=True)
    torch.cuda.current_stream(dev).wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    assert captured.requires_grad and torch.equal(captured.detach(), eager)
    assert {"text_embed_fwd", "first_eos"} <= sites(c) and not {"text_embed_varlen", "attention_varlen_causal_fwd"} & sites(c)


# ------------------------------------------------------------------------------------------------ (f) the step

B, R = 4, 3


def _batch(cfg, ids_on=None):
    ids = synth.synth_input_ids(B, cfg.text, seed=13, ragged=True)
    return {"pixel_values": synth.synth_pixel_values(B, cfg.vision, seed=11), "input_ids": ids if ids_on is None else ids.to(ids_on),
            "regions": synth.synth_regions(B, R, cfg.vision, seed=12), "region_counts": torch.tensor([3, 1, 0, 2]),
            "teacher_text_emb": synth.synth_embeddings(B, cfg.projection_dim, seed=14)}


def _module(cfg, dev, **kw):
    from dclip_amd.CLIP_image_distillation import CLIPImageDistillation
    hp = argparse.Namespace(learning_rate=1e-4, warmup_steps=0, total_steps=100, train_batch_size=B, eval_batch_size=B)
    student = from_hf_state_dict(cfg, synth.synth_clip_state_dict(cfg, seed=0, gain=2.0), device=dev)
    mod = CLIPImageDistillation(hp, student, None, freeze_mode="as_written", **kw).to(dev)
    cm = synth.synth_cross_modal_state_dict(cfg.projection_dim, seed=31)
    mod.teacher.load_state_dict({f"cross_modal_attention.{k}": v for k, v in cm.items()})
    return mod


def _run_step(mod, batch, monkeypatch):
    with Census(monkeypatch) as c:
        loss = mod.training_step(batch)
        loss.backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().clone() for k, p in mod.student.named_parameters() if p.grad is not None}
    return loss.detach(), {k: float(v) for k, v in mod.last_losses.items()}, grads, c


def test_step_with_packed_text_train_against_the_padded_step(dev, monkeypatch):
    """The gates of tests/test_text_packed_gpu.py's step test: the three losses within 1e-3 relative, gradient cosine >= 0.9999
    per tensor.  Measured on an MI355X: losses within 2.2e-7, gradient cosines 1.00000000 over 38 tensors."""
    cfg = dcfg.tiny()
    batch = _batch(cfg)
    mod_on = _module(cfg, dev, packed_text_train=True)
    assert mod_on.packed_text_train is True and mod_on.packed_text is False and mod_on.teacher.packed_text is False
    l1, parts1, g1, c1 = _run_step(mod_on, batch, monkeypatch)
    mod_off = _module(cfg, dev, packed_text_train=False)
    assert mod_off.packed_text_train is False
    l0, parts0, g0, c0 = _run_step(mod_off, batch, monkeypatch)
    lp, partsp, gp, cp = _run_step(_module(cfg, dev), batch, monkeypatch)           # a module built without the argument
    rel = {k: abs(parts1[k] - parts0[k]) / abs(parts0[k]) for k in parts0}
    gcos = {k: float(torch.nn.functional.cosine_similarity(g0[k].double().flatten(), g1[k].double().flatten(), dim=0)) for k in g0}
    print(f"losses rel {rel}; worst gradient cosine {min(gcos.values()):.8f} over {len(gcos)} tensors")
    assert set(parts0) == {"loss_image", "loss_text", "loss_contrastive"} and all(v <= 1e-3 for v in rel.values()), rel
    text_grads = [k for k in g0 if k.startswith("text_model.") or k.startswith("text_projection")]
    assert set(g0) == set(g1) and len(text_grads) > 12 * cfg.text.num_hidden_layers and min(gcos.values()) >= 0.9999, gcos
    on, off = sites(c1), sites(c0)
    assert NEW_SITES <= on and "text_embed_bwd" not in on, sorted(on)
    assert {"text_embed_varlen", "attention_varlen_causal_fwd"} <= on
    assert not NEW_SITES & off and {"text_embed_bwd", "scatter_rows"} <= off, sorted(off)
    # scatter_rows: the text tower's launch is gone (the vision tower's CLS backward has launches of its own under that name)
    count = lambda c: [x.split(".")[0] for x in c.names].count("scatter_rows")      # noqa: E731
    assert count(c1) == count(c0) - 1, (count(c1), count(c0))
    layers = cfg.text.num_hidden_layers
    assert [x.split(".")[0] for x in c1.names].count("attention_varlen_causal_bwd") == layers
    assert c0.names == cp.names and torch.equal(l0, lp)
    # the teacher's frozen passes follow `packed_text` alone: with it off they stay padded
    assert "pack_tokens_varlen" not in on and "pack_tokens" in on


def test_without_host_lengths_the_padded_path_runs(dev, monkeypatch):
    cfg = dcfg.tiny()
    batch = _batch(cfg, ids_on=dev)                                       # ids on the device, no text_lens
    l0, parts0, g0, c0 = _run_step(_module(cfg, dev), batch, monkeypatch)
    l1, parts1, g1, c1 = _run_step(_module(cfg, dev, packed_text_train=True), batch, monkeypatch)
    assert torch.equal(l0, l1) and parts0 == parts1 and c0.names == c1.names and not NEW_SITES & sites(c1)
    tok = "text_model.embeddings.token_embedding.weight"                  # float atomics: not the same bits from run to run
    assert set(g0) == set(g1) and tok in g0 and all(torch.equal(g0[k], g1[k]) for k in g0 if k != tok)
    assert float(torch.nn.functional.cosine_similarity(g0[tok].double().flatten(), g1[tok].double().flatten(), dim=0)) >= 0.9999
    # the same batch with its lengths handed over: packed
    lens = packed_text_tables(batch["input_ids"].cpu(), cfg.text.eos_token_id)["lens"]
    _, parts2, _, c2 = _run_step(_module(cfg, dev, packed_text_train=True), dict(batch, text_lens=lens), monkeypatch)
    assert NEW_SITES <= sites(c2)
    assert all(abs(parts2[k] - parts0[k]) <= 1e-3 * abs(parts0[k]) for k in parts0), (parts0, parts2)
