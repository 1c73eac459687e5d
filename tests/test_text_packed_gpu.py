"""The frozen text tower on packed captions: HipCLIPModel.get_text_features(packed_lens=...) against the fp64
oracle and the golden tiny tower, the 16-bit packed towers against the fp32 one, isolation of the captions inside a pack, the
packed token-level pass against the padded one, and the teacher / training step with `packed_text` against the padded step:
targets, losses, gradients, the launch list, and the cases in which the padded path must still run."""
import argparse

import numpy as np
import pytest
import torch

from dclip_amd import config as dcfg, synth
from dclip_amd.clip_model import from_hf_state_dict, packed_text_tables
from tests.test_fullres_packed_gpu import Census, figures
from tests.test_split16_gpu import _text_model, norm_err

pytestmark = pytest.mark.gpu

NEW_SITES = {"attention_varlen_causal_fwd", "text_embed_varlen", "pack_tokens_varlen"}
PADDED_SITES = {"text_embed_fwd", "first_eos", "pack_tokens"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def sites(census):
    return {s.split(".")[0] for s in census.names}


# ------------------------------------------------------------------------------------------------ (a) fp64 oracle, ViT-B/32

@pytest.mark.parametrize("gain", [1.0, 3.0])
def test_packed_text_tower_against_the_fp64_oracle(dev, gain, monkeypatch):
    """The gate tests/test_split16_gpu.py applies to the padded path on the same model and ids: error against fp64 <= 1e-5,
    with the split-fp16 plan on (it must have run) and with it off.
    Measured on an MI355X (max |got - want| / max |want|): gain 1.0 split 1.12e-6, plain 1.20e-6 (padded: 1.12e-6, 1.01e-6), packed
    against padded 8.5e-7 / 1.1e-6; gain 3.0 split 1.17e-6, plain 1.08e-6 (padded: 1.19e-6, 1.03e-6), packed against padded
    1.3e-6 / 9.4e-7."""
    from dclip_amd import engine
    from oracle import dclip_oracle as O
    monkeypatch.setattr(engine, "_SPLIT16", True)
    cfg, sd, m = _text_model(gain, dev)
    ids = synth.synth_input_ids(3, cfg.text, seed=3, ragged=True)
    lens = packed_text_tables(ids, cfg.text.eos_token_id)["lens"]
    assert len(set(lens.tolist())) > 1 and int(lens.sum()) < ids.numel()                  # ragged: fewer rows than the rectangle
    want = O.text_tower(O.to_dtype({k: v for k, v in sd.items() if k.startswith("text_")}, torch.float64), ids, cfg.text)
    idd = ids.to(dev)
    with torch.no_grad():
        got = m.get_text_features(input_ids=ids, packed_lens=True)               # host ids: lengths derived
        plan = m._split16_cache()["__split16__"]["layers"]
        assert plan is not None and len(plan) == cfg.text.num_hidden_layers       # the split path did run
        assert got.shape == want.shape and got.dtype == torch.float32 and not got.requires_grad
        assert torch.equal(m.get_text_features(input_ids=idd, packed_lens=lens), got)             # device ids + host lengths
        assert torch.equal(m.get_text_features(input_ids=idd, packed_lens=lens.tolist()), got)    # run to run
        padded = m.get_text_features(input_ids=idd)
        monkeypatch.setattr(engine, "_SPLIT16", False)
        plain = m.get_text_features(input_ids=idd, packed_lens=lens)
        plain_padded = m.get_text_features(input_ids=idd)
        assert torch.equal(m.get_text_features(input_ids=idd, packed_lens=lens), plain)
    assert not torch.equal(plain, got)
    e_split, e_plain = norm_err(got, want), norm_err(plain, want)
    print(f"packed text tower gain {gain}: split vs fp64 {e_split:.3e}, plain fp32 vs fp64 {e_plain:.3e}; packed vs padded: "
          f"split {norm_err(got, padded.double().cpu()):.3e}, plain {norm_err(plain, plain_padded.double().cpu()):.3e}; "
          f"padded vs fp64: split {norm_err(padded, want):.3e}, plain {norm_err(plain_padded, want):.3e}")
    assert e_split <= 1e-5 and e_plain <= 1e-5, (e_split, e_plain)


# ------------------------------------------------------------------------------------------------ tiny tower

@pytest.fixture(scope="module")
def tiny(dev):
    cfg = dcfg.tiny()
    sd = synth.synth_clip_state_dict(cfg, seed=7, gain=4.0)
    m = from_hf_state_dict(cfg, sd, device=dev)
    m.requires_grad_(False)
    return cfg, sd, m


def relerr(got, want):
    got = got.detach().double().cpu()
    want = torch.as_tensor(np.asarray(want)).double() if not isinstance(want, torch.Tensor) else want.detach().double().cpu()
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))


def test_packed_tiny_tower_against_the_golden_embeddings(dev, tiny, golden):
    """(b) tests/test_model_gpu.py's bar for the padded path: 1e-3 against f32.text_emb and f64.text_emb."""
    g = golden("towers_tiny.npz")
    cfg, sd, m = tiny
    ids = torch.from_numpy(np.asarray(g["input_ids"]))
    txt = m.get_text_features(input_ids=ids, packed_lens=True)
    e32, e64 = relerr(txt, g["f32.text_emb"]), relerr(txt, g["f64.text_emb"])
    print(f"packed tiny tower against the golden file: f32 {e32:.3e}, f64 {e64:.3e}")
    assert e32 < 1e-3 and e64 < 1e-3
    sent, tokens, cu, tables = m.text_token_level_packed(ids)
    assert relerr(sent, g["f32.text_emb"]) < 1e-3
    lh = torch.from_numpy(np.asarray(g["f32.text_last_hidden"]))
    want_tok = lh @ m.text_projection.weight.detach().cpu().t()
    host_cu = tables["cu_seqlens"].tolist()
    assert cu.tolist() == host_cu and tokens.shape == (tables["Tp"], cfg.projection_dim)
    for b in range(ids.shape[0]):
        assert relerr(tokens[host_cu[b]:host_cu[b + 1]], want_tok[b, :host_cu[b + 1] - host_cu[b]]) < 1e-3, b


def test_packed_16_bit_towers_against_the_fp32_packed_result(dev):
    """(c) The gates of the frozen 16-bit towers: bf16 below 3e-2 with cosine above 0.999; fp16 below 1e-3 with cosine above
    0.99999 — on the model and the ids those gates were set on for the padded path (tests/test_fp16_gpu.py, tests/test_bf16_gpu.py:
    ViT-B/32, gain 3.0, six ragged captions of seed 3).
    Measured on an MI355X: bf16 6.4e-3 / 0.9999800, fp16 8.0e-4 / 0.9999996.  (On the tiny tower at gain 4.0 the PADDED fp16 tower
    is 2.7e-3 from the padded fp32 one and the packed one 1.5e-3 from the packed fp32 one: that model is not what the gate
    describes.  DESIGN.md §23.)"""
    cfg, sd, m = _text_model(3.0, dev)
    ids = synth.synth_input_ids(6, cfg.text, seed=3, ragged=True)
    with torch.no_grad():
        f32 = m.get_text_features(input_ids=ids, packed_lens=True)
        fig = {}
        for prec in ("bf16", "fp16"):
            x = m.get_text_features(input_ids=ids, packed_lens=True, precision=prec)
            assert x.shape == f32.shape and x.dtype == torch.float32
            fig[prec] = figures(x, f32)
            padded = m.get_text_features(input_ids=ids.to(dev), precision=prec)
            print(f"packed {prec} against packed fp32: max rel err {fig[prec][0]:.3e}, min cosine {fig[prec][1]:.7f}; "
                  f"against padded {prec}: {figures(x, padded)[0]:.3e}")
            assert torch.equal(x, m.get_text_features(input_ids=ids, packed_lens=True, precision=prec)), prec
    assert fig["bf16"][0] < 3e-2 and fig["bf16"][1] > 0.999, fig
    assert fig["fp16"][0] < 1e-3 and fig["fp16"][1] > 0.99999, fig


def test_changing_one_captions_words_leaves_every_other_caption_bit_identical(dev, tiny):
    """(d)"""
    cfg, sd, m = tiny
    ids = synth.synth_input_ids(5, cfg.text, seed=6, ragged=True, min_len=4)
    lens = packed_text_tables(ids, cfg.text.eos_token_id)["lens"].tolist()
    victim = 2
    changed = ids.clone()
    changed[victim, 1:lens[victim] - 1] = (changed[victim, 1:lens[victim] - 1] + 1) % min(cfg.text.bos_token_id, cfg.text.eos_token_id)
    changed[victim, 1] = 1 if int(ids[victim, 1]) != 1 else 2
    assert packed_text_tables(changed, cfg.text.eos_token_id)["lens"].tolist() == lens and not torch.equal(changed, ids)
    keep = [b for b in range(ids.shape[0]) if b != victim]
    for prec in ("fp32", "bf16"):
        before, after = (m.get_text_features(input_ids=x, packed_lens=True, precision=prec) for x in (ids, changed))
        assert not torch.equal(before[victim], after[victim]), prec
        assert torch.equal(before[keep], after[keep]) and bool(torch.isfinite(after).all()), prec
        (s0, t0, cu, tab), (s1, t1, _, _) = (m.text_token_level_packed(x, precision=prec) for x in (ids, changed))
        host_cu = tab["cu_seqlens"].tolist()
        rows = torch.ones(t0.shape[0], dtype=torch.bool)
        rows[host_cu[victim]:host_cu[victim + 1]] = False
        assert torch.equal(t0[rows.to(dev)], t1[rows.to(dev)]) and torch.equal(s0[keep], s1[keep]), prec
        assert not torch.equal(t0[host_cu[victim] + 1], t1[host_cu[victim] + 1]), prec


def test_packed_token_level_against_the_padded_token_level(dev, tiny):
    """(e) The [B, Tmax, P] block and the sentence at the embedding bar (< 1e-3, cosine > 0.99999); the zero rows bit-zero.
    Measured on an MI355X, fp32: sentence 4.5e-7 / 1.00000000, block 4.2e-7 / 1.00000000.  The 16-bit pairs are printed only
    (bf16 1.9e-2, fp16 1.3e-3 on the block): their two sides differ in the attention core's I/O type, not only in the rows."""
    from dclip_amd import ops
    cfg, sd, m = tiny
    ids = synth.synth_input_ids(6, cfg.text, seed=8, ragged=True)
    ids[1, 1:] = cfg.text.eos_token_id                                       # a caption without word tokens: its sentence row
    for prec in ("fp32", "bf16", "fp16"):
        sent, tokens, cu, tables = m.text_token_level_packed(ids, precision=prec)
        block = ops.pack_tokens_varlen(tokens, sent, cu, tables["max_tokens"])
        p_sent, p_tokens, eos = m.text_token_level(ids.to(dev), precision=prec)
        assert tables["max_tokens"] == max(int(eos.max()) - 1, 1)
        want = ops.pack_tokens(p_tokens.contiguous(), p_sent, eos, tables["max_tokens"])
        assert block.shape == want.shape and bool(torch.isfinite(block).all())
        fs, fb = figures(sent, p_sent), figures(block.flatten(1), want.flatten(1))
        print(f"packed token level {prec} against padded: sentence {fs[0]:.3e} / {fs[1]:.8f}, block {fb[0]:.3e} / {fb[1]:.8f}")
        if prec == "fp32":                                                    # the 16-bit pair differs in its attention core's I/O
            assert fs[0] < 1e-3 and fs[1] > 0.99999 and fb[0] < 1e-3 and fb[1] > 0.99999, (fs, fb)
        zero = want.abs().sum(-1) == 0
        assert bool(zero.any()) and torch.equal(block[zero].view(torch.int32), torch.zeros_like(block[zero]).view(torch.int32))
        assert torch.equal(block[1, 0], sent[1])


# ------------------------------------------------------------------------------------------------ (f) teacher and step

B, R = 4, 3


def _batch(cfg, ids_on=None, text_target=False):
    """text_target: a given sentence target.  With the default teacher the student's text features ARE the teacher's sentence
    embeddings, the text loss is zero up to rounding and has no relative error; a given target keeps it away from zero."""
    ids = synth.synth_input_ids(B, cfg.text, seed=13, ragged=True)
    batch = {"pixel_values": synth.synth_pixel_values(B, cfg.vision, seed=11),
             "input_ids": ids if ids_on is None else ids.to(ids_on),
             "regions": synth.synth_regions(B, R, cfg.vision, seed=12), "region_counts": torch.tensor([3, 1, 0, 2])}
    if text_target:
        batch["teacher_text_emb"] = synth.synth_embeddings(B, cfg.projection_dim, seed=14)
    return batch


def _module(cfg, dev, packed, own_teacher=True, **kw):
    """own_teacher: the default teacher (a snapshot of the student: one text pass serves both); otherwise a teacher on another
    CLIP, so the student's own frozen text forward runs."""
    from dclip_amd.CLIP_image_distillation import CLIPImageDistillation
    from dclip_amd.patch_text_aggregation import PatchTextAggregation
    hp = argparse.Namespace(learning_rate=1e-4, warmup_steps=0, total_steps=100, train_batch_size=B, eval_batch_size=B)
    student = from_hf_state_dict(cfg, synth.synth_clip_state_dict(cfg, seed=0, gain=2.0), device=dev)
    teacher = None
    if not own_teacher:
        other = from_hf_state_dict(cfg, synth.synth_clip_state_dict(cfg, seed=1, gain=2.0), device=dev)
        other.requires_grad_(False)
        teacher = PatchTextAggregation(embed_dim=cfg.projection_dim, num_heads=1, clip_model=other).to(dev)
    mod = CLIPImageDistillation(hp, student, None, teacher=teacher, freeze_mode="north_star", packed_text=packed, **kw).to(dev)
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


@pytest.mark.parametrize("route", ["shared_sentence", "side_stream", "plain_call"])
def test_step_with_packed_text_against_the_padded_step(dev, monkeypatch, route):
    """Teacher target at the embedding bar, the three losses within 1e-3 relative, gradient cosine >= 0.9999 per tensor; the
    launch list holds the three new sites and none of the padded text sites, and with the flag off none of the new ones.
    The three routes are the three places the step's frozen text features come from.
    Measured on an MI355X: teacher target 1.3e-7 ... 1.7e-7 / 1.00000000, losses within 2.2e-7, gradient cosines 1.00000000."""
    cfg = dcfg.tiny()
    kw = {"own_teacher": route == "shared_sentence"}
    batch = _batch(cfg, text_target=route == "shared_sentence")
    res = {}
    for packed in (False, True):
        mod = _module(cfg, dev, packed, **kw)
        if route == "plain_call":
            mod.overlap_frozen_text = False
        with torch.no_grad():
            target = mod.teacher.compute_global_embedding_tensors(batch["regions"].to(dev), batch["input_ids"],
                                                                  batch["region_counts"]).clone()
        res[packed] = (target, *_run_step(mod, batch, monkeypatch))
    (t0, l0, parts0, g0, c0), (t1, l1, parts1, g1, c1) = res[False], res[True]
    err, cos = figures(t1, t0)
    rel = {k: abs(parts1[k] - parts0[k]) / abs(parts0[k]) for k in parts0}
    gcos = {k: float(torch.nn.functional.cosine_similarity(g0[k].double().flatten(), g1[k].double().flatten(), dim=0)) for k in g0}
    print(f"{route}: teacher target {err:.3e} / {cos:.8f}; losses rel {rel}; worst gradient cosine {min(gcos.values()):.8f} over "
          f"{len(gcos)} tensors")
    assert err < 1e-3 and cos > 0.99999, (err, cos)
    assert set(parts0) == {"loss_image", "loss_text", "loss_contrastive"} and all(v <= 1e-3 for v in rel.values()), rel
    assert set(g0) == set(g1) and len(g0) > 0 and min(gcos.values()) >= 0.9999, gcos
    on, off = sites(c1), sites(c0)
    assert NEW_SITES <= on and not (PADDED_SITES & on), sorted(on)
    assert not (NEW_SITES & off) and PADDED_SITES <= off, sorted(off)
    if route != "shared_sentence":
        layers = cfg.text.num_hidden_layers                                   # the teacher's token pass + the student's frozen pass
        assert [s.split(".")[0] for s in c1.names].count("attention_varlen_causal_fwd") == 2 * layers
        assert [s.split(".")[0] for s in c1.names].count("text_embed_varlen") == 2


def test_without_host_lengths_the_flag_changes_nothing(dev, monkeypatch):
    cfg = dcfg.tiny()
    batch = _batch(cfg, ids_on=dev, text_target=True)                         # ids on the device, no text_lens
    l0, parts0, g0, c0 = _run_step(_module(cfg, dev, False), batch, monkeypatch)
    l1, parts1, g1, c1 = _run_step(_module(cfg, dev, True), batch, monkeypatch)
    assert torch.equal(l0, l1) and parts0 == parts1 and c0.names == c1.names and not (NEW_SITES & sites(c1))
    assert all(torch.equal(g0[k], g1[k]) for k in g0)
    # the same batch with its lengths handed over beside max_tokens: packed again
    lens = packed_text_tables(batch["input_ids"].cpu(), cfg.text.eos_token_id)["lens"]
    l2, parts2, g2, c2 = _run_step(_module(cfg, dev, True), dict(batch, text_lens=lens), monkeypatch)
    assert NEW_SITES <= sites(c2) and not (PADDED_SITES & sites(c2))
    assert all(abs(parts2[k] - parts0[k]) <= 1e-3 * abs(parts0[k]) for k in parts0), (parts0, parts2)


def test_a_prefetched_teacher_runs_packed_too(dev, monkeypatch):
    """prefetch_teacher hands the host lengths to the teacher: the step it feeds holds no padded text launch, and its losses
    are those of the step whose teacher ran inside it."""
    cfg = dcfg.tiny()
    batch = _batch(cfg, text_target=True)
    _, parts0, _, _ = _run_step(_module(cfg, dev, True), batch, monkeypatch)
    mod = _module(cfg, dev, True)
    with Census(monkeypatch) as c:
        assert mod.prefetch_teacher(batch) is True
        loss = mod.training_step(batch)
    torch.cuda.synchronize()
    assert mod._prefetched is None and bool(torch.isfinite(loss))
    assert NEW_SITES <= sites(c) and not (PADDED_SITES & sites(c)), sorted(sites(c))
    parts = {k: float(v) for k, v in mod.last_losses.items()}
    assert all(abs(parts[k] - parts0[k]) <= 1e-3 * abs(parts0[k]) for k in parts0), (parts0, parts)


def test_under_capture_the_padded_path_runs_and_a_trainable_tower_is_refused(dev, tiny, monkeypatch):
    cfg, sd, m = tiny
    ids = synth.synth_input_ids(3, cfg.text, seed=9, ragged=True)
    lens = packed_text_tables(ids, cfg.text.eos_token_id)["lens"]
    idd = ids.to(dev)
    with torch.no_grad():
        eager_padded = m.get_text_features(input_ids=idd)                   # warm-up: the split plan is built before the capture
        eager_packed = m.get_text_features(input_ids=idd, packed_lens=lens)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        graph = torch.cuda.CUDAGraph()
        with Census(monkeypatch) as c:
            with torch.cuda.stream(side):
                with torch.cuda.graph(graph, stream=side):
                    captured = m.get_text_features(input_ids=idd, packed_lens=lens)
        torch.cuda.current_stream(dev).wait_stream(side)
        graph.replay()
        torch.cuda.synchronize()
    assert not (NEW_SITES & sites(c)) and {"text_embed_fwd", "first_eos"} <= sites(c), sorted(sites(c))
    assert torch.equal(captured, eager_padded) and figures(eager_packed, eager_padded)[0] < 1e-3
    # a trainable text tower: the forward-only error of the 16-bit frozen paths
    trainable = from_hf_state_dict(cfg, sd, device=dev)
    with pytest.raises(RuntimeError, match="forward-only path for frozen towers: call it under torch.no_grad"):
        trainable.get_text_features(input_ids=idd, packed_lens=lens)
    with torch.no_grad():
        assert torch.equal(trainable.get_text_features(input_ids=idd, packed_lens=lens), eager_packed)
    with pytest.raises(ValueError, match="never"):
        m.get_text_features(input_ids=idd, packed_lens=True)
