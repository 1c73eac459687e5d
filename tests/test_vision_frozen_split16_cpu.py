"""Precision "fp32-split16" without a device: the string is accepted or refused at every constructor and launcher
parser, the generalised host plan keeps its guard on any tower's layers, and the new C entries refuse bad arguments before a
launch."""
import inspect
import logging

import pytest
import torch

from dclip_amd import config as dcfg

P = "fp32-split16"


@pytest.fixture(scope="module")
def clip():
    from dclip_amd.clip_model import HipCLIPModel
    return HipCLIPModel(dcfg.tiny())


def test_launcher_parsers_take_the_new_choice_and_refuse_others():
    from dclip_amd import flickr30k_eval, train_contrastive_teacher, zero_shot_eval
    z = zero_shot_eval.build_parser()
    assert z.parse_args(["--data_root", "x", "--precision", P]).precision == P
    f = flickr30k_eval.build_parser()
    f_args = [a for act in f._actions if act.required for a in (act.option_strings[0], "x")]
    assert f.parse_args(f_args + ["--precision", P]).precision == P
    t = train_contrastive_teacher.build_parser()
    t_args = [a for act in t._actions if act.required for a in (act.option_strings[0], "x")]
    assert t.parse_args(t_args + ["--tower_precision", P]).tower_precision == P
    assert t.parse_args(t_args).tower_precision == "fp32"
    for parser, base, flag in ((z, ["--data_root", "x"], "--precision"), (f, f_args, "--precision"), (t, t_args, "--tower_precision")):
        with pytest.raises(SystemExit):
            parser.parse_args(base + [flag, "fp32-split"])


def test_constructors_take_the_new_string_and_refuse_others(clip):
    from dclip_amd.patch_text_aggregation import CLIPPatchTokenizer, CLIPTextTokenizer, PatchTextAggregation, TOWER_PRECISIONS
    assert TOWER_PRECISIONS == ("fp32", "bf16", "fp16", P)
    E = clip.config.projection_dim
    t = PatchTextAggregation(embed_dim=E, num_heads=1, clip_model=clip, tower_precision=P)
    assert t.patch_tokenizer.precision == P and t.text_tokenizer.precision == P
    assert CLIPPatchTokenizer(clip, precision=P).precision == P and CLIPTextTokenizer(clip, precision=P).precision == P
    for bad in ("fp32-split", "fp16-mixed", "split16"):
        with pytest.raises(ValueError, match="precision"):
            PatchTextAggregation(embed_dim=E, num_heads=1, clip_model=clip, tower_precision=bad)
        with pytest.raises(ValueError, match="precision"):
            CLIPPatchTokenizer(clip, precision=bad)
        with pytest.raises(ValueError, match="precision"):
            CLIPTextTokenizer(clip, precision=bad)


def test_eval_helpers_route_the_text_side_to_fp32(clip):
    from dclip_amd import eval as E
    assert E.PRECISIONS == ("fp32", "bf16", "fp16", P)
    assert [E.text_precision(p) for p in E.PRECISIONS] == ["fp32", "bf16", "fp16", "fp32"]
    enc_i, enc_t = E.encoders(clip, P)
    assert callable(enc_i) and callable(enc_t)
    with pytest.raises(ValueError, match="precision"):
        E.encoders(clip, "fp32-split")


def test_model_entries_refuse_before_any_device_work(clip):
    v = clip.config.vision
    pix = torch.zeros(1, 3, v.image_size, v.image_size)
    with pytest.raises(RuntimeError, match="forward-only"):              # grad enabled, trainable parameters
        clip.get_image_features(pixel_values=pix, precision=P)
    with pytest.raises(ValueError, match="precision"):
        clip.get_image_features(pixel_values=pix, precision="fp32-split")
    with pytest.raises(ValueError, match="precision"):
        clip.get_image_features_crops(torch.zeros(1, 32, 32, 3, dtype=torch.uint8), torch.tensor([[32, 32]], dtype=torch.int32),
                                      [(0, 0, 0, 16, 16)], precision="fp32-split")
    with pytest.raises(ValueError, match="precision"):
        clip.text_token_level(torch.zeros(1, 4, dtype=torch.long), precision="fp32-split")
    with pytest.raises(ValueError, match="precision"):
        clip.text_token_level_packed(torch.zeros(1, 4, dtype=torch.long), precision="fp32-split")
    assert clip._vsplit16_frozen_cache() is clip._vsplit16_frozen_cache()
    assert clip._vsplit16_frozen_cache() is not clip._vsplit16_cache() and clip._vsplit16_frozen_cache() is not clip._split16_cache()


def test_packed_attention16_has_no_effect_at_this_precision():
    from dclip_amd import engine
    for one_row in (False, True):
        for attn16 in (None, False, True):
            assert engine.packed_attn16_route(P, 50, one_row, attn16) == "f32"


def test_host_plan_takes_any_towers_layers_and_keeps_its_guard(clip, monkeypatch, caplog):
    """_split16_plan reads a list of LayerParams only; its guard — a non-finite weight, a bound that needs e < -14 — answers None
    (the plain fp32 path) before anything is split, under the caller's log prefix."""
    from dclip_amd import engine
    sig = inspect.signature(engine._split16_plan)
    assert list(sig.parameters)[:3] == ["layers_p", "cache", "what"]
    assert sig.parameters["what"].default == "split-fp16 text tower"            # the text tower's records read as they did
    monkeypatch.setattr(engine, "_SPLIT16_LOGGED", set())
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)      # no device here: nothing is capturing
    with torch.no_grad():
        for p in clip.parameters():
            p.normal_(0.0, 0.02, generator=torch.Generator().manual_seed(1))
        for tower in (clip.vision_model, clip.text_model):
            for layer in tower.encoder.layers:
                layer.layer_norm1.weight.fill_(1.0), layer.layer_norm2.weight.fill_(1.0)
    vl, tl = clip.vision_params().layers, clip.text_params().layers
    with torch.no_grad():
        vl[0].ln2_w.fill_(1e7)                      # layer 0: the guard answers before any weight is split on a device
        tl[0].fc1_w[3, 5] = float("inf")
    with caplog.at_level(logging.WARNING, logger="dclip_amd"):
        cache_v, cache_t = {}, {}
        assert engine._vision_frozen_split16_plan(vl, clip.config.vision, cache_v) is None
        assert engine._vision_frozen_split16_plan(vl, clip.config.vision, cache_v) is None          # cached: no second record
        assert engine._split16_plan(tl, cache_t) is None
        assert engine._vision_frozen_split16_plan(vl, clip.config.vision, None) is None
        assert engine._vision_frozen_split16_plan([], clip.config.vision, {}) is None
    msgs = [r.getMessage() for r in caplog.records]
    assert len(msgs) == 2, msgs
    assert msgs[0].startswith("split-fp16 frozen vision tower: an activation bound of layer 0") and "plain fp32 path" in msgs[0]
    assert msgs[1].startswith("split-fp16 text tower: non-finite weight in layer 0")
    assert cache_v["__split16__"]["layers"] is None and cache_t["__split16__"]["layers"] is None
    # the rule the guard applied: the GELU bound of that layer, from its own statistics, asks for an exponent below -14
    D = clip.config.vision.hidden_size
    lp = engine.LayerParams(*[t.detach() for t in vl[0].tensors()])
    st = {"ln1_w": float(lp.ln1_w.abs().max()), "ln1_b": float(lp.ln1_b.abs().max()), "v_l1": float(lp.qkv_w[2 * D:].abs().sum(1).max()),
          "v_b": float(lp.qkv_b[2 * D:].abs().max()), "ln2_w": float(lp.ln2_w.abs().max()), "ln2_b": float(lp.ln2_b.abs().max()),
          "fc1_l1": float(lp.fc1_w.abs().sum(1).max()), "fc1_b": float(lp.fc1_b.abs().max())}
    exps = {k: engine.split16_act_exp(v) for k, v in engine.split16_layer_bounds(st, D).items()}
    assert exps["g"] is None and exps["ln1"] is not None and exps["ctx"] is not None, exps


def test_new_entries_refuse_bad_arguments_without_a_gpu():
    from dclip_amd import _lib
    lib = _lib.load()
    ptr = 4096                                   # never dereferenced: every case below is refused before a launch
    D = 128
    dense = [  # qkv, y, B, S, H, causal, scale, pieces, ldy
        ((None, ptr, 1, 4, 2, 0, 1.0, 2, 2 * D), b"null pointer"),
        ((ptr, ptr, 0, 4, 2, 0, 1.0, 2, 2 * D), b"bad shape"),
        ((ptr, ptr, 1, 4, 2, 0, 1.0, 4, 4 * D), b"pieces"),
        ((ptr, ptr, 1, 4, 2, 0, 1.0, 3, 2 * D), b"ldy"),
        ((ptr, ptr, 1, 4, 2, 0, 1.0, 2, 2 * D + 2), b"ldy"),
        ((ptr, ptr + 2, 1, 4, 2, 0, 1.0, 2, 2 * D), b"aligned"),
        ((ptr, ptr, 1, 4, 2, 0, 3.0, 2, 2 * D), b"power of two"),
        ((ptr, ptr, 1, 4, 2, 0, float("inf"), 2, 2 * D), b"power of two"),
    ]
    for args, msg in dense:
        assert lib.dclip_attention_fwd_f16x2(*args, None) == -1, args
        assert msg in lib.dclip_last_error(), (args, lib.dclip_last_error())
    packed = [  # qkv, cu, y, N, max_S, H, causal, scale, pieces, ldy
        ((ptr, None, ptr, 1, 4, 2, 0, 1.0, 2, 2 * D), b"null pointer"),
        ((ptr, ptr, ptr, 0, 4, 2, 0, 1.0, 2, 2 * D), b"bad shape"),
        ((ptr, ptr, ptr, 1, 0, 2, 1, 1.0, 2, 2 * D), b"bad shape"),
        ((ptr, ptr, ptr, 1, 4, 2, 1, 1.0, 1, 2 * D), b"pieces"),
        ((ptr, ptr, ptr, 1, 4, 2, 0, 1.0, 3, 3 * D - 1), b"ldy"),
        ((ptr + 4, ptr, ptr, 1, 4, 2, 0, 1.0, 2, 2 * D), b"aligned"),
        ((ptr, ptr, ptr, 1, 4, 2, 0, -2.0, 2, 2 * D), b"power of two"),
    ]
    for args, msg in packed:
        assert lib.dclip_attention_varlen_fwd_f16x2(*args, None) == -1, args
        assert msg in lib.dclip_last_error(), (args, lib.dclip_last_error())
