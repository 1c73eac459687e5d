"""Frozen fp32 vision tower on split-fp16 operands, precision "fp32-split16" (DESIGN.md §28): the attention entries that write
their context already split against the two-launch pair they replace, bit for bit; the dense and the packed tower against the
plain fp32 path and the fp64 oracle; the guard, a HIP-graph capture, the teacher, and the token-level text pass."""
import logging

import pytest
import torch

from dclip_amd import config as dcfg, synth

pytestmark = pytest.mark.gpu

P = "fp32-split16"
LOW = {"DCLIP_BF16_BIG_MIN": "1", "DCLIP_F16X3_MIN": "1", "DCLIP_F16X3_TOK_MIN": "1"}     # read per call by the GEMM plans
SENTINEL = -7.0


def rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))


def same_bits(got, want):
    """Bit equality of two fp16 tensors; where the reference value is a NaN the other must be a NaN, whatever its bits
    (tests/test_split16_gpu.py::same_bits)."""
    nan = want.isnan()
    return bool(torch.equal(got.isnan(), nan)) and bool(torch.equal(got.view(torch.int16)[~nan], want.view(torch.int16)[~nan]))


def norm_err(got, want):
    return float((got.detach().double().cpu() - want.detach().double().cpu()).abs().max() / want.detach().abs().max().clamp_min(1e-300))


# ------------------------------------------------------------------------------------------------ 1. attention-split kernels

H = 2
D = H * 64
SCALES = (1.0, 2.0 ** -3, 2.0 ** 9)


def crafted_qkv(rows, first, last, seed):
    """qkv [rows, 3 D]: random, except that in the sequence of rows first[0] .. first[1]-1 every query scores 512 on key 0 and 0
    on every other key (their probabilities underflow to exactly 0) and V of key 0 is +-1024: the context of those rows is the
    fp16-exact +-1024, whose lo is a zero.  One +inf in V at row `last` (a masked key's 0 * inf, and inf - inf in the split, are
    NaNs)."""
    qkv = rnd((rows, 3 * D), seed)
    a, b = first
    qkv[a:b, :2 * D] = 0.0
    for h in range(H):
        qkv[a:b, h * 64] = 64.0                              # q . k0 / 8 = 512
        qkv[a, D + h * 64] = 64.0
    qkv[a, 2 * D:] = 1024.0
    qkv[a, 2 * D + 1::2] = -1024.0
    qkv[last, 2 * D + 5] = float("inf")
    return qkv


def check_split_entry(run_split, ref32, rows):
    """run_split(scale, pieces, out) against split_f16x3(ref32, scale, pieces) for every scale and layout, into a destination
    with 8 padding columns that must keep their sentinel."""
    from dclip_amd import ops
    seen_zero_lo = seen_nan = False
    for pieces in (2, 3):
        for scale in SCALES:
            want = ops.split_f16x3(ref32, scale, pieces=pieces)
            out = torch.full((rows, pieces * D + 8), SENTINEL, dtype=torch.float16, device=ref32.device)
            got = run_split(scale, pieces, out)
            assert got.data_ptr() == out.data_ptr()
            assert same_bits(out[:, :pieces * D], want), (pieces, scale)
            assert bool((out[:, pieces * D:] == SENTINEL).all()), (pieces, scale)
            fresh = run_split(scale, pieces, None)
            assert tuple(fresh.shape) == (rows, pieces * D) and same_bits(fresh, want), (pieces, scale)
            lo = want[:, D:2 * D]
            seen_zero_lo |= bool(((want[:, :D].abs() == 1024.0 * scale) & (lo == 0)).any())
            seen_nan |= bool(want.isnan().any())
    return seen_zero_lo, seen_nan


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("S", [1, 17, 50, 80, 81, 197])
def test_attention_split_entry_bit_equal_to_attention_then_split(S, causal):
    """Whole-row kernel (S <= 80) and streamed kernel (81, 197), B = 2, H = 2."""
    from dclip_amd import _lib, ops
    dev = torch.device("cuda:0")
    B = 2
    qkv = crafted_qkv(B * S, (0, S), B * S - 1, 10 * S + causal).to(dev)          # sequence 0: V = 1024; sequence 1: one inf
    ref32, _ = ops.attention_fwd(qkv, B, S, H, causal)
    zero_lo, nan = check_split_entry(lambda sc, pc, out: ops.attention_fwd_f16x2(qkv, B, S, H, causal, sc, pc, out=out), ref32, B * S)
    assert (b".rows" if S <= 80 else b".stream") in _lib.load().dclip_last_launch()
    assert zero_lo                                           # an fp16-exact context value was among the inputs
    if causal and S > 1:
        assert nan                                           # ... and a NaN (a masked key times inf)


@pytest.mark.parametrize("causal", [False, True])
def test_packed_attention_split_entry_bit_equal_to_attention_then_split(causal):
    from dclip_amd import ops
    dev = torch.device("cuda:0")
    lens = [1, 2, 50, 145, 257]
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32)
    T = int(cu[-1])
    qkv = crafted_qkv(T, (3, 53), T - 1, 77 + causal).to(dev)                       # the 50-token sequence: context = +-1024
    cu = cu.to(dev)
    attn = ops.attention_varlen_causal_fwd if causal else ops.attention_varlen_fwd
    ref32 = attn(qkv, cu, max(lens), H)
    zero_lo, nan = check_split_entry(lambda sc, pc, out: ops.attention_varlen_fwd_f16x2(qkv, cu, max(lens), H, causal, sc, pc, out=out),
                                     ref32, T)
    assert zero_lo and (nan or not causal)


def test_attention_split_entries_refuse_bad_arguments():
    from dclip_amd import ops
    dev = torch.device("cuda:0")
    qkv = rnd((4, 3 * D), 0).to(dev)
    cu = torch.tensor([0, 4], dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match="pieces"):
        ops.attention_fwd_f16x2(qkv, 1, 4, H, False, 1.0, 4)
    with pytest.raises(ValueError, match="out"):
        ops.attention_fwd_f16x2(qkv, 1, 4, H, False, 1.0, 2, out=torch.empty((4, 2 * D - 8), dtype=torch.float16, device=dev))
    with pytest.raises(Exception, match="power of two"):
        ops.attention_fwd_f16x2(qkv, 1, 4, H, False, 3.0, 2)
    with pytest.raises(Exception, match="power of two"):
        ops.attention_varlen_fwd_f16x2(qkv, cu, 4, H, False, 0.0, 2)


# ------------------------------------------------------------------------------------------------ 2. dense tower

def vision_keys(sd):
    return {k: v for k, v in sd.items() if k.startswith("vision_model.") or k.startswith("visual_projection")}


def fp64_features(sd, pix, v, pos=None):
    """oracle.dclip_oracle.vision_tower in fp64; on a patch grid other than the configuration's (`pos`: the position table
    resampled to it, [1 + gh gw, D]) the same functions on the rectangular grid."""
    from oracle import dclip_oracle as O
    p = {k: t.double() for k, t in vision_keys(sd).items()}
    if pos is None:
        return O.vision_tower(p, pix.double(), v)
    B, C, ps = pix.shape[0], v.num_channels, v.patch_size
    gh, gw = pix.shape[2] // ps, pix.shape[3] // ps
    w = p["vision_model.embeddings.patch_embedding.weight"].reshape(v.hidden_size, -1)
    cols = pix.double()[:, :, :gh * ps, :gw * ps].reshape(B, C, gh, ps, gw, ps).permute(0, 2, 4, 1, 3, 5).reshape(B, gh * gw, -1)
    x = torch.cat([p["vision_model.embeddings.class_embedding"].expand(B, 1, -1), cols @ w.t()], dim=1) + pos.double()
    x = O.layer_norm(x, p["vision_model.pre_layrnorm.weight"], p["vision_model.pre_layrnorm.bias"], v.layer_norm_eps)
    for i in range(v.num_hidden_layers):
        x = O.clip_encoder_layer(x, p, f"vision_model.encoder.layers.{i}", v.num_attention_heads, False, v.layer_norm_eps)
    pooled = O.layer_norm(x[:, 0, :], p["vision_model.post_layernorm.weight"], p["vision_model.post_layernorm.bias"], v.layer_norm_eps)
    return O.linear(pooled, p["visual_projection.weight"])


class Tower:
    """One configuration: a frozen model and its state dict (made once)."""

    def __init__(self, name):
        from dclip_amd.clip_model import from_hf_state_dict
        self.dev = torch.device("cuda:0")
        self.cfg = dcfg.tiny() if name == "tiny" else dcfg.vit_b32()
        self.sd = synth.synth_clip_state_dict(self.cfg, seed=5, gain=2.0)
        self.model = from_hf_state_dict(self.cfg, self.sd, device=self.dev)
        self.model.requires_grad_(False)


_TOWERS = {}


def tower(name):
    if name not in _TOWERS:
        _TOWERS[name] = Tower(name)
    return _TOWERS[name]


def check_dense(t, pix, tag, interp=False, pieces=None):
    """The bars of DESIGN.md §9c / §9d on one input: within 1e-5 of precision "fp32"; against fp64 at most 4x the plain path's own
    error; not the plain path's bits; run to run bit-identical; "fp32" untouched by the split calls."""
    from dclip_amd import engine, ops
    v = t.cfg.vision
    kw = {"interpolate_pos_encoding": True} if interp else {}
    pix_dev = pix.to(t.dev)
    with torch.no_grad():
        plain0 = t.model.get_image_features(pixel_values=pix_dev, **kw)
        got = t.model.get_image_features(pixel_values=pix_dev, precision=P, **kw)
        again = t.model.get_image_features(pixel_values=pix_dev, precision=P, **kw)
        plain1 = t.model.get_image_features(pixel_values=pix_dev, **kw)
        pos = None
        if interp:
            pos = ops.pos_interp_fwd(t.model.vision_params().pos.detach(), v.grid, pix.shape[2] // v.patch_size,
                                     pix.shape[3] // v.patch_size).cpu()
    plan = t.model._vsplit16_frozen_cache().get("__split16__")
    assert plan is not None and plan["layers"] is not None and len(plan["layers"]) == v.num_hidden_layers     # the plan was built
    assert got.shape == plain0.shape and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    assert not torch.equal(got, plain0), "the split path gave the plain path's bits: it did not run"
    assert same(again, got), "run to run"
    assert same(plain1, plain0), 'precision="fp32" changed after a split call'
    want = fp64_features(t.sd, pix, v, pos)
    d, es, ep = norm_err(got, plain0), norm_err(got, want), norm_err(plain0, want)
    print(f"{tag}: split vs plain {d:.3e}; vs fp64 split {es:.3e} plain {ep:.3e} ratio {es / ep:.2f}")
    if pieces is not None:
        rows = pix.shape[0] * (1 + (pix.shape[2] // v.patch_size) * (pix.shape[3] // v.patch_size))
        pc = engine._layer_pieces(rows, v.hidden_size, v.intermediate_size, engine._SPLIT16_FC1_EPI)
        assert set(pc.values()) == {pieces}, pc
    assert d <= 1e-5, (tag, d)
    assert es <= 4 * ep, (tag, es, ep)


def test_tiny_tower_against_plain_and_fp64():
    """B = 4 x 17 tokens: the register-staged GEMM kernels, three pieces, the whole-row attention kernel."""
    t = tower("tiny")
    check_dense(t, synth.synth_pixel_values(4, t.cfg.vision, seed=1), "tiny", pieces=3)


def test_vit_b32_tower_on_the_fused_kernels_with_two_pieces(monkeypatch):
    """B = 2 x 50 tokens with the plans' thresholds at 1: the fused ping-pong kernel and [hi|lo] operands at M = 100."""
    for k, val in LOW.items():
        monkeypatch.setenv(k, val)
    t = tower("vit_b32")
    check_dense(t, synth.synth_pixel_values(2, t.cfg.vision, seed=1), "vit_b32", pieces=2)


def test_tiny_tower_on_a_3_by_5_grid():
    t = tower("tiny")
    ps = t.cfg.vision.patch_size
    check_dense(t, rnd((4, 3, 3 * ps, 5 * ps), 21), "tiny 3x5", interp=True, pieces=3)


def test_tiny_tower_on_a_197_token_grid():
    """14 x 14 patches: the streamed attention kernel."""
    from dclip_amd import _lib
    t = tower("tiny")
    ps = t.cfg.vision.patch_size
    check_dense(t, rnd((1, 3, 14 * ps, 14 * ps), 22), "tiny 14x14", interp=True)
    with torch.no_grad():
        from dclip_amd import ops
        qkv = rnd((197, 3 * D), 3).to(t.dev)
        ops.attention_fwd_f16x2(qkv, 1, 197, H, False, 1.0, 2)
    assert b"attention_fwd_f16x2.stream" in _lib.load().dclip_last_launch()


def test_attention_switch_is_bit_identical(monkeypatch):
    """The A/B switch of §28: the context from attention_fwd + the split pass gives the same features, bit for bit."""
    from dclip_amd import engine
    t = tower("tiny")
    pix = synth.synth_pixel_values(4, t.cfg.vision, seed=1).to(t.dev)
    with torch.no_grad():
        a = t.model.get_image_features(pixel_values=pix, precision=P)
        monkeypatch.setattr(engine, "_SPLIT16_ATTN_EPI", not engine._SPLIT16_ATTN_EPI)
        b = t.model.get_image_features(pixel_values=pix, precision=P)
    assert same(a, b)


def test_hidden_states_and_training_are_refused_or_plain():
    from dclip_amd import engine
    from dclip_amd.clip_model import from_hf_state_dict
    t = tower("tiny")
    v = t.cfg.vision
    pix = synth.synth_pixel_values(2, v, seed=1).to(t.dev)
    pd = engine.VisionParams.from_tensors([x.detach() for x in t.model.vision_params().tensors()], v.num_hidden_layers)
    hid, hid_plain = [], []
    with torch.no_grad():
        a = engine.vision_fwd_frozen_split16(pd, pix, v, t.model._vsplit16_frozen_cache(), hidden_out=hid)
        b, _ = engine.vision_fwd(pd, pix, v, False, hid_plain)
    assert same(a, b) and len(hid) == len(hid_plain) == v.num_hidden_layers + 1 and all(same(x, y) for x, y in zip(hid, hid_plain))
    trainable = from_hf_state_dict(t.cfg, t.sd, device=t.dev)
    with pytest.raises(RuntimeError, match="forward-only"):
        trainable.get_image_features(pixel_values=pix, precision=P)
    with torch.no_grad():
        assert same(trainable.get_image_features(pixel_values=pix, precision=P), t.model.get_image_features(pixel_values=pix, precision=P))
    assert trainable._vsplit16_frozen_cache() is not trainable._vsplit16_cache()


# ------------------------------------------------------------------------------------------------ 3. guard

def test_guard_takes_the_plain_path_bit_for_bit_and_logs_once(monkeypatch, caplog):
    from dclip_amd import engine
    from dclip_amd.clip_model import from_hf_state_dict
    t = tower("tiny")
    monkeypatch.setattr(engine, "_SPLIT16_LOGGED", set())
    model = from_hf_state_dict(t.cfg, t.sd, device=t.dev).requires_grad_(False)
    with torch.no_grad():
        model.vision_model.encoder.layers[0].layer_norm2.weight.fill_(1e7)
    pix = synth.synth_pixel_values(4, t.cfg.vision, seed=1).to(t.dev)
    with caplog.at_level(logging.WARNING, logger="dclip_amd"), torch.no_grad():
        plain = model.get_image_features(pixel_values=pix)
        got = model.get_image_features(pixel_values=pix, precision=P)
        again = model.get_image_features(pixel_values=pix, precision=P)
    assert same(got, plain) and same(again, plain)
    assert not bool(torch.isinf(got).any())
    msgs = [r.getMessage() for r in caplog.records if "split-fp16 frozen vision tower" in r.getMessage()]
    assert len(msgs) == 1 and "layer 0" in msgs[0] and "plain fp32 path" in msgs[0], msgs


# ------------------------------------------------------------------------------------------------ 4. capture

def test_frozen_forward_replays_from_a_graph_bit_equal_to_eager():
    t = tower("tiny")
    pix = synth.synth_pixel_values(4, t.cfg.vision, seed=1).to(t.dev)
    with torch.no_grad():
        eager = t.model.get_image_features(pixel_values=pix, precision=P)        # warm-up: the plan is built here
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = t.model.get_image_features(pixel_values=pix, precision=P)
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
    assert same(out, eager)


# ------------------------------------------------------------------------------------------------ 5. packed

def test_packed_crops_within_1e5_of_fp32():
    """One-patch crop (2 tokens), a 50-token crop, a 91-token crop (two key tiles), and a second image's crops, in one pack."""
    t = tower("tiny")
    ps = t.cfg.vision.patch_size
    u8 = torch.randint(0, 256, (2, 10 * ps, 11 * ps, 3), generator=torch.Generator().manual_seed(4), dtype=torch.uint8).to(t.dev)
    dims = torch.tensor([[10 * ps, 11 * ps], [9 * ps, 8 * ps]], dtype=torch.int32, device=t.dev)
    boxes = [(0, 3, 5, 3 + ps, 5 + ps), (0, 0, 0, 7 * ps, 7 * ps), (0, 2, 1, 2 + 10 * ps, 1 + 9 * ps), (1, 8, 8, 8 + 3 * ps, 8 + 2 * ps),
             (1, 0, 0, 7 * ps, 7 * ps)]
    plain = t.model.get_image_features_crops(u8, dims, boxes)
    got = t.model.get_image_features_crops(u8, dims, boxes, precision=P)
    d = norm_err(got, plain)
    print(f"packed crops: split vs plain {d:.3e}")
    assert got.shape == plain.shape and not torch.equal(got, plain)
    assert d <= 1e-5, d
    assert same(got, t.model.get_image_features_crops(u8, dims, boxes, precision=P))
    assert same(plain, t.model.get_image_features_crops(u8, dims, boxes))


# ------------------------------------------------------------------------------------------------ 6. teacher, text side

def test_teacher_target_within_1e5_of_the_fp32_teachers():
    from dclip_amd.patch_text_aggregation import PatchTextAggregation
    t = tower("tiny")
    E = t.cfg.projection_dim
    regions = synth.synth_regions(2, 2, t.cfg.vision, seed=2).to(t.dev)
    ids = synth.synth_input_ids(2, t.cfg.text, seed=3, ragged=True).to(t.dev)
    out = {}
    for prec in ("fp32", P):
        teacher = PatchTextAggregation(embed_dim=E, num_heads=1, clip_model=t.model, tower_precision=prec).to(t.dev)
        teacher.cross_modal_attention.load_state_dict(synth.synth_cross_modal_state_dict(E, seed=5))
        assert teacher.patch_tokenizer.precision == prec and teacher.text_tokenizer.precision == prec
        with torch.no_grad():
            out[prec] = teacher.compute_global_embedding_tensors(regions, ids, torch.tensor([2, 2], dtype=torch.int32))
    d = norm_err(out[P], out["fp32"])
    print(f"teacher target: split vs fp32 {d:.3e}")
    assert d <= 1e-5 and not torch.equal(out[P], out["fp32"]), d


def test_text_token_level_within_1e5_of_fp32():
    """3 ragged captions x 77 positions (the text tower of ViT-B/32 would be slow to build: the tiny one at seq 77), padded and
    packed."""
    from dclip_amd.clip_model import from_hf_state_dict
    dev = torch.device("cuda:0")
    cfg = dcfg.tiny(seq=77)
    model = from_hf_state_dict(cfg, synth.synth_clip_state_dict(cfg, seed=5, gain=2.0), device=dev).requires_grad_(False)
    ids = synth.synth_input_ids(3, cfg.text, seed=3, ragged=True)
    s0, t0, e0 = model.text_token_level(ids.to(dev))
    s1, t1, e1 = model.text_token_level(ids.to(dev), precision=P)
    assert torch.equal(e0, e1) and t1.shape == t0.shape == (3, 77, cfg.projection_dim)
    ds, dt = norm_err(s1, s0), norm_err(t1, t0)
    print(f"text_token_level: sentence {ds:.3e} tokens {dt:.3e}")
    assert ds <= 1e-5 and dt <= 1e-5, (ds, dt)
    assert not torch.equal(t1, t0)
    p0 = model.text_token_level_packed(ids)
    p1 = model.text_token_level_packed(ids, precision=P)
    dps, dpt = norm_err(p1[0], p0[0]), norm_err(p1[1], p0[1])
    print(f"text_token_level_packed: sentence {dps:.3e} tokens {dpt:.3e}")
    assert dps <= 1e-5 and dpt <= 1e-5 and not torch.equal(p1[1], p0[1]), (dps, dpt)
    s2, t2, _ = model.text_token_level(ids.to(dev))
    assert same(s2, s0) and same(t2, t0)                      # "fp32" is what it was
