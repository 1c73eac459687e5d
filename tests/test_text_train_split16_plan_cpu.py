"""The trainable text tower on the split-fp16 plan, the part that needs no GPU: the route's truth table, the
switch from the launcher to the model, and the two new C entries in the header and the Python prototypes."""
import argparse
import itertools
import os
import re

import pytest
import torch

from dclip_amd import config as dcfg
from dclip_amd.clip_model import HipCLIPModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_routing_decision():
    """The plan exactly when the switch is on, gradients are needed, nothing is capturing and the widths are multiples of 8."""
    from dclip_amd.CLIP_image_distillation import packed_text_train_route, text_train_split16_route
    from dclip_amd import clip_model
    assert text_train_split16_route is clip_model.text_train_split16_route and callable(packed_text_train_route)
    for flag, trainable, capturing, widths_ok in itertools.product((False, True), repeat=4):
        want = flag and trainable and not capturing and widths_ok
        assert text_train_split16_route(flag, trainable, capturing, widths_ok) is want, (flag, trainable, capturing, widths_ok)


def test_the_launchers_and_the_flag():
    """The student launcher carries --text_train_split16, default off; the teacher launcher trains no text tower and rejects it."""
    from dclip_amd import CLIP_image_distill_training as student_launcher, train_contrastive_teacher as teacher_launcher
    p = student_launcher.build_parser()
    off, on = p.parse_args(["--train_file", "x.json"]), p.parse_args(["--train_file", "x.json", "--text_train_split16"])
    assert off.text_train_split16 is False and on.text_train_split16 is True
    assert on.packed_text_train is False and on.packed_text is False       # it implies nothing about the packed switches
    both = p.parse_args(["--train_file", "x.json", "--text_train_split16", "--packed_text_train"])
    assert both.text_train_split16 is True and both.packed_text_train is True
    with pytest.raises(SystemExit):
        teacher_launcher.build_parser().parse_args(["--train_file", "x.json", "--text_train_split16"])


def test_the_switch_reaches_the_module_and_the_model():
    from dclip_amd.CLIP_image_distillation import CLIPImageDistillation
    cfg = dcfg.tiny()
    assert HipCLIPModel.text_train_split16 is False and HipCLIPModel(cfg).text_train_split16 is False
    hp = argparse.Namespace(learning_rate=1e-4, warmup_steps=0, total_steps=10, train_batch_size=2, eval_batch_size=2)
    off = CLIPImageDistillation(hp, HipCLIPModel(cfg), None)
    on = CLIPImageDistillation(hp, HipCLIPModel(cfg), None, text_train_split16=True)
    assert off.text_train_split16 is False and on.text_train_split16 is True
    assert on.packed_text_train is False and on.packed_text is False
    m = HipCLIPModel(cfg)
    # its own cache: neither the frozen host plan's nor the vision tower's
    c = m._tsplit16_train_cache()
    assert c == {} and c is m._tsplit16_train_cache() and c is not m._split16_cache() and c is not m._vsplit16_cache()
    # the model's routing: off, under no_grad and with a frozen tower there is no plan cache to hand to the schedule
    p = m.text_params()
    assert m._text_train_split16_cache(p) is None
    m.text_train_split16 = True
    assert m._text_train_split16_cache(p) is c
    with torch.no_grad():
        assert m._text_train_split16_cache(p) is None
    m.requires_grad_(False)
    assert m._text_train_split16_cache(m.text_params()) is None


def test_the_schedules_take_the_two_arguments():
    import inspect
    from dclip_amd import engine
    for fn in (engine.text_encoder_fwd, engine.text_fwd, engine.text_fwd_packed):
        sig = inspect.signature(fn).parameters
        assert sig["split16_cache"].default is None and sig["split16_out"].default is None, fn.__name__
    for fn in (engine.text_bwd, engine.text_bwd_packed):
        assert inspect.signature(fn).parameters["split16"].default is None, fn.__name__
    # the generalised device plan keeps the vision tower's key and label by default
    sig = inspect.signature(engine._vision_split16_plan).parameters
    assert sig["key"].default == "__vsplit16__" and sig["what"].default == "split-fp16 vision tower"
    assert engine._TSPLIT16_KEY != sig["key"].default


def test_header_and_prototypes_agree_on_the_new_entries():
    from dclip_amd import _lib
    with open(os.path.join(ROOT, "include", "dclip_hip.h")) as f:
        header = f.read()
    for name in ("dclip_attention_bwd_rows_stats_plan", "dclip_attention_bwd_rows_stats"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        res, proto = _lib.SIGNATURES[name]
        assert res is _lib.I and len(args) == len(proto), (name, args, proto)
        for a, ct in zip(args, proto):
            assert ("*" in a) == (ct is _lib.P), (name, a, ct)
    # the statistics entry has the signature of the one-tile form
    one = re.search(r"\bint\s+dclip_attention_bwd_stats\s*\(([^;]*?)\)\s*;", header, re.S).group(1)
    rows = re.search(r"\bint\s+dclip_attention_bwd_rows_stats\s*\(([^;]*?)\)\s*;", header, re.S).group(1)
    assert re.sub(r"\s+", " ", one) == re.sub(r"\s+", " ", rows)

