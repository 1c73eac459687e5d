"""The trainable text tower on packed captions, the part that needs no GPU: the launcher's switch, where the
step sends the student's text features, and the fp64 statement the feature rests on — the padded tower's parameter gradients
are the sums of the gradients of the cut captions."""
import argparse
import itertools

import pytest
import torch

from dclip_amd import config as dcfg, synth
from dclip_amd.clip_model import HipCLIPModel, packed_text_tables
from tests import schedule_checks as sc


def test_the_launchers_and_the_flag():
    """The student launcher carries --packed_text_train, default off.  The teacher launcher trains no text tower (its CLIP
    towers are frozen; only the cross-modal block trains): it does not take the flag."""
    from dclip_amd import CLIP_image_distill_training as student_launcher, train_contrastive_teacher as teacher_launcher
    p = student_launcher.build_parser()
    off, on = p.parse_args(["--train_file", "x.json"]), p.parse_args(["--train_file", "x.json", "--packed_text_train"])
    assert off.packed_text_train is False and on.packed_text_train is True
    assert on.packed_text is False                                        # it implies nothing about --packed_text
    assert p.parse_args(["--train_file", "x.json", "--packed_text"]).packed_text_train is False
    with pytest.raises(SystemExit):
        teacher_launcher.build_parser().parse_args(["--train_file", "x.json", "--packed_text_train"])


def test_the_flag_reaches_the_module_and_not_its_teacher():
    from dclip_amd.CLIP_image_distillation import CLIPImageDistillation
    cfg = dcfg.tiny()
    hp = argparse.Namespace(learning_rate=1e-4, warmup_steps=0, total_steps=10, train_batch_size=2, eval_batch_size=2)
    off = CLIPImageDistillation(hp, HipCLIPModel(cfg), None)
    on = CLIPImageDistillation(hp, HipCLIPModel(cfg), None, packed_text_train=True)
    assert off.packed_text_train is False and on.packed_text_train is True
    assert on.packed_text is False and on.teacher.packed_text is False
    # host lengths for the trainable path: a batch entry, else ids on the host; none for ids that are elsewhere or with the flag off
    ids = synth.synth_input_ids(3, cfg.text, seed=2, ragged=True)
    want = packed_text_tables(ids, cfg.text.eos_token_id)["lens"]
    assert torch.equal(on._host_text_lens(ids, train=True), want) and torch.equal(on._host_text_lens(batch={"input_ids": ids}, train=True), want)
    assert on._host_text_lens(batch={"input_ids": ids.to("meta"), "text_lens": [3, 4, 5]}, train=True) == [3, 4, 5]
    assert on._host_text_lens(batch={"input_ids": ids.to("meta")}, train=True) is None
    assert on._host_text_lens(ids) is None                                # the frozen passes follow `packed_text`, which is off
    assert off._host_text_lens(ids, train=True) is None


def test_the_routing_decision():
    """Packed exactly when the switch is on, the tower trains, host lengths exist and nothing is capturing."""
    from dclip_amd.CLIP_image_distillation import packed_text_train_route
    for flag, trainable, lens, capturing in itertools.product((False, True), repeat=4):
        want = flag and trainable and lens and not capturing
        assert packed_text_train_route(flag, trainable, lens, capturing) is want, (flag, trainable, lens, capturing)


def test_a_trainable_tower_is_still_refused_without_the_switch():
    m = HipCLIPModel(dcfg.tiny())                                          # fresh parameters require grad
    ids = synth.synth_input_ids(2, m.config.text, seed=1, ragged=True)
    for kw in ({}, {"packed_train": False}, {"packed_train": True, "precision": "bf16"}, {"packed_train": True, "precision": "fp16"}):
        with pytest.raises(RuntimeError, match="packed_lens is a forward-only path for frozen towers: call it under torch.no_grad"):
            m.get_text_features(input_ids=ids, packed_lens=True, **kw)


def test_padded_oracle_gradients_are_the_sums_over_the_cut_captions():
    """fp64, the case of tests/test_text_packed_train_gpu.py: tiny(seq=80), gain 2.0, lengths [2, 3, 17, 64, 65, 80].  d x is
    exactly zero on every row behind a first EOS, so each parameter gradient of the padded rectangle equals the sum of the
    gradients of the captions cut after their first EOS, to 1e-12 (‖a − b‖ / ‖b‖)."""
    from tests.test_text_packed_train_gpu import LENS, make_ids
    cfg = dcfg.tiny(seq=80)
    sd = synth.synth_clip_state_dict(cfg, seed=7, gain=2.0)
    ids = make_ids(cfg, LENS)
    W = sc.output_weighting((len(LENS), cfg.projection_dim))
    padded = sc.reference("text", cfg.text, sd, ids, W)
    total = None
    for b, S in enumerate(LENS):
        # one caption alone may leave a gradient at zero (a two-token caption reads two position rows): add the raw tensors
        keys = [k for n in sc.names("text", 2) for k in sc.hf_keys("text", n)]
        p = {k: sd[k].detach().double().requires_grad_(True) for k in keys}
        from oracle import dclip_oracle as O
        (O.text_tower(p, ids[b:b + 1, :S], cfg.text) * W[b:b + 1]).sum().backward()
        g = sc.to_engine("text", 2, {k: (t.grad if t.grad is not None else torch.zeros_like(t)) for k, t in p.items()})
        total = g if total is None else {n: total[n] + g[n] for n in g}
    worst = {n: sc.rel_err(total[n], padded[n]) for n in padded}
    print("worst", max(worst.values()))
    assert max(worst.values()) <= 1e-12, worst
