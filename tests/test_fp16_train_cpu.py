"""CPU-only checks of the fp16 student (student_precision="fp16"): the module builds, the launcher takes the switch, the
loss scaler validates its arguments and keeps GradScaler's state-dict keys, checkpoints carry its state, and the new C
entries reject bad arguments without a GPU."""
import argparse

import pytest
import torch

from dclip_amd import config as dcfg
from dclip_amd.clip_model import HipCLIPModel


def _hp():
    return argparse.Namespace(learning_rate=1e-3, warmup_steps=0, total_steps=10, train_batch_size=2, eval_batch_size=2)


def test_module_builds_with_an_fp16_student_on_the_cpu():
    from dclip_amd.CLIP_image_distillation import CLIPImageDistillation
    mod = CLIPImageDistillation(_hp(), HipCLIPModel(dcfg.tiny()), None, freeze_mode="north_star", student_precision="fp16")
    assert mod.student_precision == "fp16"
    assert mod._image_precision() == "fp16-mixed"
    with pytest.raises(ValueError, match="fp8"):
        CLIPImageDistillation(_hp(), HipCLIPModel(dcfg.tiny()), None, student_precision="fp8")


def test_launcher_parses_the_student_precision():
    from dclip_amd.CLIP_image_distill_training import build_parser
    p = build_parser()
    assert p.parse_args(["--train_file", "x.json"]).student_precision == "fp32"
    assert p.parse_args(["--train_file", "x.json", "--student_precision", "fp16"]).student_precision == "fp16"
    assert p.parse_args(["--train_file", "x.json", "--student_precision", "bf16"]).student_precision == "bf16"
    with pytest.raises(SystemExit):
        p.parse_args(["--train_file", "x.json", "--student_precision", "fp8"])


@pytest.mark.parametrize("kw", [dict(init_scale=0.0), dict(init_scale=-1.0), dict(init_scale=float("inf")),
                                dict(growth_factor=1.0), dict(backoff_factor=1.0), dict(backoff_factor=0.0),
                                dict(growth_interval=0), dict(growth_interval=2.5), dict(growth_interval=True)])
def test_scaler_rejects_bad_arguments(kw):
    from dclip_amd.amp import DynamicLossScaler
    with pytest.raises(ValueError):
        DynamicLossScaler(**kw)


def test_scaler_state_dict_round_trips_with_gradscaler_keys():
    from dclip_amd.amp import DynamicLossScaler
    s = DynamicLossScaler(init_scale=2.0 ** 10, growth_factor=4.0, backoff_factor=0.25, growth_interval=7)
    sd = s.state_dict()
    assert set(sd) == {"scale", "growth_factor", "backoff_factor", "growth_interval", "_growth_tracker"}
    assert sd == {"scale": 1024.0, "growth_factor": 4.0, "backoff_factor": 0.25, "growth_interval": 7, "_growth_tracker": 0}
    t = DynamicLossScaler()
    t.load_state_dict(dict(sd, scale=512.0, _growth_tracker=3))
    assert t.state_dict() == dict(sd, scale=512.0, _growth_tracker=3)
    assert t.get_scale() == 512.0
    with pytest.raises(RuntimeError):
        t.load_state_dict({})


def test_checkpoint_holds_the_scaler_state(tmp_path):
    from dclip_amd.amp import DynamicLossScaler
    from dclip_amd.CLIP_image_distillation import CLIPImageDistillation
    from dclip_amd.lightning_lite import save_checkpoint
    mod = CLIPImageDistillation(_hp(), HipCLIPModel(dcfg.tiny()), None, student_precision="fp16")
    s = DynamicLossScaler(init_scale=2.0 ** 20, growth_interval=5)
    path = save_checkpoint(str(tmp_path / "a.ckpt"), mod, scaler=s)
    with torch.serialization.safe_globals([argparse.Namespace]):
        ck = torch.load(path, map_location="cpu", weights_only=True)
    assert ck["native_amp_scaling_state"] == s.state_dict()
    assert "native_amp_scaling_state" not in torch.load(save_checkpoint(str(tmp_path / "b.ckpt"), mod), weights_only=True)


def test_new_entries_reject_bad_arguments_without_a_gpu():
    from dclip_amd import _lib
    lib = _lib.load()
    cases = [
        (lambda: lib.dclip_gemm_f16_ex(None, None, None, None, None, None, 4, 4, 4, 8, 8, 4, 0, 0, None), b"gemm_f16_ex: null operand"),
        (lambda: lib.dclip_gemm_f16_ex(16, 16, 16, None, None, None, 4, 4, 4, 8, 8, 4, 4, 0, None), b"gemm_f16_ex: DGELU needs aux"),
        (lambda: lib.dclip_gemm_f16_splitk(None, None, None, 4, 4, 4, 8, 8, 4, 1, None, 0, None), b"gemm_f16_splitk: null operand"),
        (lambda: lib.dclip_gemm_f16_wgrad_tokmajor(16, 16, 16, 8, 8, 60, 8, 8, 8, 1, None, 0, None), b"gemm_f16_wgrad_tokmajor: M=8"),
        (lambda: lib.dclip_cast_f32_f16_ieee(None, None, 1, 4, 4, 4, None), b"cast_f32_f16_ieee: bad arguments"),
        (lambda: lib.dclip_layernorm_fwd_f16_stats(16, 16, 16, 16, 16, None, 4, 8, 1e-5, None), b"layernorm_fwd_f16_stats: mean and rstd"),
        (lambda: lib.dclip_layernorm_bwd_ex_f16(None, None, None, None, None, None, None, None, None, None, None, 4, 8, 0, None, 0,
                                                None), b"layernorm_bwd_f16: null pointer"),
        (lambda: lib.dclip_transpose_to_f16(16, 0, 16, None, 4, 4, 4, 6, 4, None), b"transpose_to_f16: ldyT"),
        (lambda: lib.dclip_rowsum_f16(None, None, 4, 4, 8, None), b"rowsum_f16: bad arguments"),
        (lambda: lib.dclip_colsum_f16(16, 16, 4, 6, 8, 0, None, 0, None), b"colsum_f16: bad shape"),
        (lambda: lib.dclip_mt_weights_f16(None, 1, 1, None), b"mt_weights_f16: bad arguments"),
        (lambda: lib.dclip_attention_fwd_f16_lse(16, 16, 16, 1, 65, 1, 0, None), b"attention_fwd_f16_lse: B=1 S=65 (<= 64"),
        (lambda: lib.dclip_attention_bwd_f16(16, 16, 16, 16, 16, 1, 65, 1, 0, None), b"attention_bwd_f16: B=1 S=65 (<= 64)"),
        (lambda: lib.dclip_clip_coef_scaled(None, 1, 0.5, None, None, None), b"clip_coef_scaled: bad arguments"),
        (lambda: lib.dclip_mt_adamw_f32_skip(16, 1, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, None, None), b"mt_adamw_skip: bad arguments"),
        (lambda: lib.dclip_amp_update_scale(16, 16, 16, 2.0, 0.5, 0, None), b"amp_update_scale: bad arguments"),
    ]
    for call, msg in cases:
        assert call() == -1, msg
        assert msg in lib.dclip_last_error(), (msg, lib.dclip_last_error())
    # the bf16 entries that now share their code with these keep their messages
    assert lib.dclip_attention_bwd_bf16(16, 16, 16, 16, 16, 1, 65, 1, 0, None) == -1
    assert lib.dclip_last_error() == b"attention_bwd_bf16: B=1 S=65 (<= 64) H=1"
    assert lib.dclip_attention_fwd_bf16_lse(16, 16, 16, 1, 289, 1, 0, None) == -1
    assert lib.dclip_last_error() == b"attention_fwd_bf16_lse: B=1 S=289 (<= 288, not 257) H=1"
    # plans: the fp16 forms are the bf16 plans
    for m, n, k in ((768, 3072, 12800), (2304, 768, 400), (512, 768, 25600)):
        assert lib.dclip_gemm_f16_splitk_plan(m, n, k) == lib.dclip_gemm_bf16_splitk_plan(m, n, k)
        assert lib.dclip_gemm_f16_wgrad_tokmajor_plan(m, n, k) == lib.dclip_gemm_bf16_wgrad_tokmajor_plan(m, n, k)


def test_trainer_refuses_graphs_and_plain_optimizers_for_the_fp16_student():
    from dclip_amd.CLIP_image_distillation import CLIPImageDistillation
    from dclip_amd.lightning_lite import Trainer
    mod = CLIPImageDistillation(_hp(), HipCLIPModel(dcfg.tiny()), None, student_precision="fp16")
    with pytest.raises(RuntimeError, match="use_hip_graph"):
        Trainer(use_hip_graph=True).fit(mod, [], None)
    with pytest.raises(RuntimeError, match="FusedAdamW"):              # on the CPU the module's optimizer is torch.optim.AdamW
        Trainer().fit(mod, [], None)
