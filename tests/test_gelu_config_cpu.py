"""CPU-only: hidden_act travels from an HF configuration into VisionConfig / TextConfig, a configuration without it
is a quick-GELU model, and the one route that is not built for "gelu" — 16-bit training of the vision tower — refuses before the
library is entered."""
import dataclasses
from types import SimpleNamespace

import pytest
import torch

from dclip_amd import config as dcfg


def duck(vision_act, text_act):
    t = dcfg.tiny()

    def ns(c, act):
        d = dataclasses.asdict(c)
        d.pop("hidden_act")
        if act is not None:
            d["hidden_act"] = act
        return SimpleNamespace(**d)
    return SimpleNamespace(vision_config=ns(t.vision, vision_act), text_config=ns(t.text, text_act), projection_dim=t.projection_dim,
                           logit_scale_init_value=t.logit_scale_init_value)


@pytest.mark.parametrize("v_act,t_act", [("gelu", "gelu"), ("gelu", "quick_gelu"), ("quick_gelu", "gelu"), ("quick_gelu", "quick_gelu")])
def test_from_hf_keeps_each_towers_own_activation(v_act, t_act):
    c = dcfg.from_hf(duck(v_act, t_act))
    assert (c.vision.hidden_act, c.text.hidden_act) == (v_act, t_act)
    tiny = dcfg.tiny()
    assert dataclasses.replace(c.vision, hidden_act="quick_gelu") == tiny.vision
    assert dataclasses.replace(c.text, hidden_act="quick_gelu") == tiny.text


def test_from_hf_without_the_field_is_quick_gelu():
    c = dcfg.from_hf(duck(None, None))
    assert c.vision.hidden_act == c.text.hidden_act == "quick_gelu"


@pytest.mark.parametrize("v_act,t_act", [("gelu", "gelu"), ("quick_gelu", "gelu"), ("gelu", "quick_gelu")])
def test_from_hf_on_a_real_hf_config(v_act, t_act):
    transformers = pytest.importorskip("transformers")
    hf = transformers.CLIPConfig(vision_config=dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
                                                    image_size=64, patch_size=16, hidden_act=v_act),
                                 text_config=dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
                                                  max_position_embeddings=16, vocab_size=512, hidden_act=t_act),
                                 projection_dim=64)
    c = dcfg.from_hf(hf)
    assert (c.vision.hidden_act, c.text.hidden_act) == (v_act, t_act)
    assert dcfg.from_hf(transformers.CLIPConfig()).vision.hidden_act == "quick_gelu"      # HF's own default: OpenAI's release


@pytest.mark.parametrize("bad", ["gelu_new", "relu", "gelu_pytorch_tanh", "GELU", ""])
@pytest.mark.parametrize("tower", ["vision", "text"])
def test_unknown_activations_raise_naming_the_value(bad, tower):
    hf = duck(bad, "gelu") if tower == "vision" else duck("gelu", bad)
    with pytest.raises(ValueError, match=repr(bad)):
        dcfg.from_hf(hf)


def test_the_field_is_last_and_positional_construction_is_unchanged():
    assert [f.name for f in dataclasses.fields(dcfg.VisionConfig)][-1] == "hidden_act"
    assert [f.name for f in dataclasses.fields(dcfg.TextConfig)][-1] == "hidden_act"
    assert dcfg.VisionConfig(768, 3072, 12, 12, 224, 32, 3, 1e-5) == dcfg.VisionConfig()
    assert dcfg.TextConfig(512, 2048, 12, 8, 77, 49408, 49406, 49407, 1e-5) == dcfg.TextConfig()
    for mk in dcfg.NAMED.values():
        c = mk()
        assert c.vision.hidden_act == c.text.hidden_act == "quick_gelu"


def test_to_dict_round_trips_and_an_old_dict_is_quick_gelu():
    t = dcfg.tiny()
    c = dataclasses.replace(t, vision=dataclasses.replace(t.vision, hidden_act="gelu"))
    d = c.to_dict()
    assert d["vision"]["hidden_act"] == "gelu" and d["text"]["hidden_act"] == "quick_gelu"
    assert dcfg.ClipConfig.from_dict(d) == c
    old = c.to_dict()
    del old["vision"]["hidden_act"], old["text"]["hidden_act"]          # a checkpoint written before the field existed
    assert dcfg.ClipConfig.from_dict(old) == t
    d["text"]["hidden_act"] = "relu"
    with pytest.raises(ValueError, match="'relu'"):
        dcfg.ClipConfig.from_dict(d)


def gelu_tiny(vision="gelu", text="gelu"):
    t = dcfg.tiny()
    return dataclasses.replace(t, vision=dataclasses.replace(t.vision, hidden_act=vision),
                               text=dataclasses.replace(t.text, hidden_act=text))


@pytest.mark.parametrize("precision", ["bf16", "fp16-mixed"])
def test_16bit_training_of_a_gelu_vision_tower_raises_before_the_library(monkeypatch, precision):
    from dclip_amd import _lib, engine
    from dclip_amd.clip_model import HipCLIPModel

    def entered(*a, **k):
        raise AssertionError("the library was entered")
    monkeypatch.setattr(_lib, "load", entered)
    m = HipCLIPModel(gelu_tiny(text="quick_gelu"))
    pix = torch.zeros(2, 3, 64, 64)
    with pytest.raises(NotImplementedError, match="hidden_act"):
        m.get_image_features(pixel_values=pix, precision=precision)
    # the engine's own entry refuses too, whoever calls it
    p = engine.VisionParams.from_tensors([t.detach() for t in m.vision_params().tensors()], 2)
    with pytest.raises(NotImplementedError, match="hidden_act"):
        engine.vision_fwd_bf16_train(p, pix, m.config.vision, {}, torch.bfloat16 if precision == "bf16" else torch.float16)
    # a quick-GELU tower of the same shape goes on to the library (which the patch reports)
    with pytest.raises(AssertionError, match="the library was entered"):
        HipCLIPModel(dcfg.tiny()).get_image_features(pixel_values=pix, precision=precision)


def test_student_precision_reaches_the_same_refusal():
    """CLIPImageDistillation hands student_precision to get_image_features as "bf16" / "fp16-mixed": the two cases above."""
    from dclip_amd.CLIP_image_distillation import CLIPImageDistillation
    assert CLIPImageDistillation._image_precision(SimpleNamespace(student_precision="fp16")) == "fp16-mixed"
    assert CLIPImageDistillation._image_precision(SimpleNamespace(student_precision="bf16")) == "bf16"


def test_engine_reads_a_config_without_the_field_as_quick_gelu():
    from dclip_amd import engine
    assert engine.hidden_act(SimpleNamespace()) == "quick_gelu"
    assert engine.hidden_act(gelu_tiny().vision) == "gelu"
    with pytest.raises(ValueError, match="'relu'"):
        engine.hidden_act(SimpleNamespace(hidden_act="relu"))
