"""Host side of the packed text tower: the planner's tables spelled out, the refusals that keep caption lengths
from ever being read back from a device, the launchers' flags, and the equivalence the feature rests on — the fp64 oracle on a
caption cut after its first EOS equals the padded oracle's row."""
import pytest
import torch

from dclip_amd import config as dcfg, synth
from dclip_amd.clip_model import HipCLIPModel, packed_text_tables

EOS = 9


def ids_matrix():
    """[6, 8]: EOS at T-1; EOS at 0; no EOS; several EOS (first at 3); the usual EOS padding (first at 2); EOS at 1."""
    return torch.tensor([[1, 2, 3, 4, 5, 6, 7, EOS],
                         [EOS, 1, 2, 3, 4, 5, 6, 7],
                         [1, 2, 3, 4, 5, 6, 7, 8],
                         [1, 2, 3, EOS, 4, EOS, 5, EOS],
                         [1, 2, EOS, EOS, EOS, EOS, EOS, EOS],
                         [1, EOS, 2, 3, 4, 5, 6, 7]], dtype=torch.int64)


def test_tables_spelled_out():
    t = packed_text_tables(ids_matrix(), EOS)
    assert t["lens"].tolist() == [8, 1, 1, 4, 3, 2]
    assert t["cu_seqlens"].tolist() == [0, 8, 9, 10, 14, 17, 19]
    assert t["last_rows"].tolist() == [7, 8, 9, 13, 16, 18]
    assert (t["max_S"], t["Tp"], t["max_tokens"]) == (8, 19, 6)
    for k in ("lens", "cu_seqlens", "last_rows"):
        assert t[k].dtype == torch.int32 and t[k].device.type == "cpu" and t[k].is_contiguous(), k
    for k in ("max_S", "Tp", "max_tokens"):
        assert type(t[k]) is int, k
    # lens agrees with the device kernel's rule (first EOS, 0 when absent) as the host expression states it
    first = (ids_matrix() == EOS).int().argmax(dim=1)
    assert t["lens"].tolist() == (first + 1).tolist()


def test_max_tokens_never_drops_below_one():
    short = torch.tensor([[EOS, 0, 0], [1, EOS, 0]], dtype=torch.int64)
    t = packed_text_tables(short, EOS)
    assert t["lens"].tolist() == [1, 2] and t["max_tokens"] == 1 and t["max_S"] == 2 and t["Tp"] == 3
    t = packed_text_tables(torch.tensor([[1, 2, EOS]], dtype=torch.int64), EOS)
    assert t["max_tokens"] == 1 and t["cu_seqlens"].tolist() == [0, 3] and t["last_rows"].tolist() == [2]


@pytest.mark.parametrize("make", [list, lambda v: torch.tensor(v, dtype=torch.int64), lambda v: torch.tensor(v, dtype=torch.int32)],
                         ids=["list", "int64", "int32"])
def test_given_lens_are_taken_as_they_are(make):
    ids = ids_matrix()
    given = [8, 1, 1, 4, 3, 2]
    a, b = packed_text_tables(ids, EOS), packed_text_tables(ids, EOS, lens=make(given))
    for k in a:
        assert torch.equal(a[k], b[k]) if isinstance(a[k], torch.Tensor) else a[k] == b[k], k
    assert b["lens"].dtype == torch.int32 and b["lens"].is_contiguous()
    # the ids are then used for their shape alone: a tensor without storage does
    c = packed_text_tables(torch.empty((6, 8), dtype=torch.int64, device="meta"), EOS, lens=make(given))
    assert c["cu_seqlens"].tolist() == a["cu_seqlens"].tolist()
    # lengths other than the first EOS are the caller's to give (a caption cut earlier)
    d = packed_text_tables(ids, EOS, lens=make([2, 1, 8, 4, 3, 2]))
    assert d["cu_seqlens"].tolist() == [0, 2, 3, 11, 15, 18, 20] and d["max_S"] == 8 and d["max_tokens"] == 6


@pytest.mark.parametrize("bad", [[0, 1, 1, 4, 3, 2], [9, 1, 1, 4, 3, 2], [8, 1, 1, 4, 3, -2], [8, 1, 1, 4, 3], [8, 1, 1, 4, 3, 2, 1]],
                         ids=["zero", "beyond_T", "negative", "too_few", "too_many"])
def test_given_lens_out_of_range_are_refused(bad):
    with pytest.raises(ValueError):
        packed_text_tables(ids_matrix(), EOS, lens=bad)


def test_refusals_of_the_planner():
    with pytest.raises(ValueError):
        packed_text_tables(ids_matrix(), EOS, lens=torch.tensor([8.0, 1, 1, 4, 3, 2]))
    with pytest.raises(ValueError):
        packed_text_tables(ids_matrix()[0], EOS)                       # not [N, T]
    with pytest.raises(ValueError, match="never read back"):
        packed_text_tables(torch.empty((2, 8), dtype=torch.int64, device="meta"), EOS)
    with pytest.raises(ValueError):
        packed_text_tables(ids_matrix(), EOS, lens=torch.empty((6,), dtype=torch.int32, device="meta"))


class _DeviceIds:
    """Stands in for token ids that live on a GPU: a shape and a device, nothing to read."""
    shape = (2, 8)
    device = torch.device("cuda", 0)

    def dim(self):
        return 2


@pytest.mark.parametrize("ids", [_DeviceIds(), torch.empty((2, 8), dtype=torch.int64, device="meta")], ids=["cuda_stub", "meta"])
def test_packed_lens_true_with_ids_off_the_host_is_a_value_error(ids):
    m = HipCLIPModel(dcfg.tiny())
    with pytest.raises(ValueError, match="never"):
        m.get_text_features(input_ids=ids, packed_lens=True)
    with torch.no_grad(), pytest.raises(ValueError, match="never"):
        m.get_text_features(input_ids=ids, packed_lens=True, precision="bf16")


def test_packed_lens_with_a_trainable_text_tower_raises_the_forward_only_error():
    m = HipCLIPModel(dcfg.tiny())                                          # fresh parameters require grad
    ids = synth.synth_input_ids(2, m.config.text, seed=1, ragged=True)
    with pytest.raises(RuntimeError, match="forward-only path for frozen towers: call it under torch.no_grad"):
        m.get_text_features(input_ids=ids, packed_lens=True)
    with pytest.raises(RuntimeError, match="forward-only path for frozen towers: call it under torch.no_grad"):
        m.get_text_features(input_ids=ids, packed_lens=[3, 4])


def test_the_launchers_carry_the_flag():
    from dclip_amd import CLIP_image_distill_training as student_launcher, train_contrastive_teacher as teacher_launcher
    p = student_launcher.build_parser()
    assert p.parse_args(["--train_file", "x.json"]).packed_text is False
    assert p.parse_args(["--train_file", "x.json", "--packed_text"]).packed_text is True
    p = teacher_launcher.build_parser()
    assert p.parse_args(["--train_file", "x.json"]).packed_text is False
    assert p.parse_args(["--train_file", "x.json", "--packed_text"]).packed_text is True


def test_the_flag_reaches_the_module_and_its_teacher():
    import argparse
    from dclip_amd.CLIP_image_distillation import CLIPImageDistillation
    from dclip_amd.patch_text_aggregation import PatchTextAggregation
    cfg = dcfg.tiny()
    hp = argparse.Namespace(learning_rate=1e-4, warmup_steps=0, total_steps=10, train_batch_size=2, eval_batch_size=2)
    off = CLIPImageDistillation(hp, HipCLIPModel(cfg), None)
    assert off.packed_text is False and off.teacher.packed_text is False
    on = CLIPImageDistillation(hp, HipCLIPModel(cfg), None, packed_text=True)
    assert on.packed_text is True and on.teacher.packed_text is True
    t = PatchTextAggregation(embed_dim=cfg.projection_dim, num_heads=1, clip_model=HipCLIPModel(cfg), packed_text=True)
    assert t.packed_text is True
    assert PatchTextAggregation(embed_dim=cfg.projection_dim, num_heads=1, clip_model=HipCLIPModel(cfg)).packed_text is False
    # host lengths: a batch entry, else ids on the host; none for ids that are elsewhere
    ids = synth.synth_input_ids(3, cfg.text, seed=2, ragged=True)
    want = packed_text_tables(ids, cfg.text.eos_token_id)["lens"]
    assert torch.equal(on._host_text_lens(batch={"input_ids": ids}), want) and torch.equal(on._host_text_lens(ids), want)
    assert on._host_text_lens(batch={"input_ids": ids.to("meta"), "text_lens": [3, 4, 5]}) == [3, 4, 5]
    assert on._host_text_lens(batch={"input_ids": ids.to("meta")}) is None
    assert off._host_text_lens(ids) is None and off._host_text_lens(batch={"input_ids": ids, "text_lens": [3, 4, 5]}) is None
    assert t._packed_text_lens(ids) is True and t._packed_text_lens(ids.to("meta")) is None
    assert t._packed_text_lens(ids.to("meta"), [3, 4, 5]) == [3, 4, 5]


def test_the_fp64_oracle_on_a_cut_caption_equals_the_padded_row():
    """What the feature rests on: the tower is causal and pools at the first EOS, so rows behind it reach no result."""
    from oracle import dclip_oracle as O
    cfg = dcfg.tiny()
    sd = O.to_dtype({k: v for k, v in synth.synth_clip_state_dict(cfg, seed=7, gain=4.0).items() if k.startswith("text_")},
                    torch.float64)
    ids = synth.synth_input_ids(5, cfg.text, seed=4, ragged=True)
    ids[4, 2:] = torch.tensor([cfg.text.eos_token_id, 5, cfg.text.eos_token_id] + [7] * (ids.shape[1] - 5))   # words after an EOS
    lens = packed_text_tables(ids, cfg.text.eos_token_id)["lens"].tolist()
    assert len(set(lens)) > 2 and lens[4] == 3
    with torch.no_grad():
        padded = O.text_tower(sd, ids, cfg.text)
        for b, L in enumerate(lens):
            cut = O.text_tower(sd, ids[b:b + 1, :L], cfg.text)
            err = float((cut[0] - padded[b]).abs().max() / padded[b].abs().max())
            assert err <= 1e-12, (b, L, err)
