"""CPU-only checks of the opt-in fp16 frozen-tower path: argument errors of the new entries and wrappers need no GPU, the
command lines take the new precision switch (default fp32), and the meta-teacher accepts "fp16"."""
import pytest
import torch

from dclip_amd import config as dcfg


def _lib():
    from dclip_amd import _lib
    return _lib, _lib.load()


def test_f16_entries_reject_bad_arguments_without_a_gpu():
    _l, lib = _lib()
    cases = [
        (lambda: lib.dclip_gemm_f16(None, None, None, None, None, 4, 4, 4, 8, 8, 4, 0, 0, None), b"gemm_f16: null operand"),
        (lambda: lib.dclip_gemm_f16(16, 16, 16, None, None, 0, 4, 4, 8, 8, 4, 0, 0, None), b"gemm_f16: bad shape"),
        (lambda: lib.dclip_gemm_f16(16, 16, 16, None, None, 4, 4, 4, 6, 8, 4, 0, 0, None), b"gemm_f16: lda/ldw"),
        (lambda: lib.dclip_gemm_f16(16, 16, 16, None, None, 4, 6, 4, 8, 8, 8, 0, 0, None), b"gemm_f16: N / ldc"),
        (lambda: lib.dclip_gemm_f16(16, 16, 16, None, 16, 4, 4, 4, 8, 8, 4, 8, 1, None), b"gemm_f16: RESIDUAL"),
        (lambda: lib.dclip_gemm_f16(16, 16, 16, None, None, 4, 4, 4, 8, 8, 4, 4, 0, None), b"gemm_f16: DGELU"),
        (lambda: lib.dclip_cast_f32_f16(None, None, 1, 4, 4, 4, None), b"cast_f32_f16: bad arguments"),
        (lambda: lib.dclip_cast_f32_f16(16, 16, 1, 6, 6, 8, None), b"cast_f32_f16: ldx/ldy"),
        (lambda: lib.dclip_layernorm_fwd_f16(16, 16, 16, 16, 4, 6, 1e-5, None), b"layernorm_fwd_f16: bad D"),
        (lambda: lib.dclip_layernorm_fwd_f16(None, 16, 16, 16, 4, 8, 1e-5, None), b"layernorm_fwd_f16: null pointer"),
        (lambda: lib.dclip_im2col_f16(16, 16, 1, 3, 32, 32, 6, 108, None), b"im2col_f16: bad shape"),
        (lambda: lib.dclip_im2col_f16(16, 16, 1, 3, 32, 32, 16, 100, None), b"im2col_f16: ldc / alignment"),
        (lambda: lib.dclip_attention_fwd_f16(None, 16, 1, 50, 1, 0, None), b"attention_fwd_f16: null pointer"),
        (lambda: lib.dclip_attention_fwd_f16(16, 16, 1, 0, 1, 0, None), b"attention_fwd_f16: bad shape"),
        (lambda: lib.dclip_attention_fwd_f16(8, 16, 1, 50, 1, 0, None), b"attention_fwd_f16: 16-byte alignment"),
        (lambda: lib.dclip_attention_row_fwd_f16(16, None, 16, 1, 513, 1, None), b"attention_row_fwd_f16: B=1 S=513"),
        (lambda: lib.dclip_attention_row_fwd_f16(None, None, 16, 1, 50, 1, None), b"attention_row_fwd_f16: null pointer"),
    ]
    for call, msg in cases:
        assert call() == -1, msg
        assert msg in lib.dclip_last_error(), (msg, lib.dclip_last_error())


def test_bf16_entries_keep_their_messages():
    """The bf16 entries now share their checks with the fp16 ones: their error texts are unchanged."""
    _l, lib = _lib()
    assert lib.dclip_gemm_bf16(None, None, None, None, None, 4, 4, 4, 8, 8, 4, 0, 0, None) == -1
    assert lib.dclip_last_error() == b"gemm_bf16: null operand"
    assert lib.dclip_attention_fwd_bf16(16, 16, 1, 0, 1, 0, None) == -1
    assert lib.dclip_last_error() == b"attention_fwd_bf16: bad shape B=1 S=0 H=1"
    assert lib.dclip_layernorm_fwd_bf16(16, 16, 16, 16, 4, 6, 1e-5, None) == -1
    assert lib.dclip_last_error() == b"layernorm_fwd_bf16: bad D=6"


def test_f16_wrappers_check_dtype_and_device_on_the_host():
    from dclip_amd import ops
    a = torch.zeros(4, 8, dtype=torch.float16)
    with pytest.raises(ValueError, match="float16"):
        ops.gemm_f16(a, a)                                        # CPU tensors
    with pytest.raises(ValueError, match="float16"):
        ops.attention_fwd_f16(torch.zeros(50, 192, dtype=torch.float16), 1, 50, 1, False)
    with pytest.raises(ValueError, match="float16"):
        ops.attention_row_fwd_f16(torch.zeros(50, 192, dtype=torch.bfloat16), None, 1, 50, 1)
    with pytest.raises(ValueError, match="float32"):
        ops.cast_f16(torch.zeros(4, 8, dtype=torch.float16))
    with pytest.raises(ValueError, match="float32"):
        ops.layernorm_fwd_f16(torch.zeros(4, 8), torch.ones(8), torch.zeros(8), 1e-5)
    with pytest.raises(ValueError, match="float32"):
        ops.im2col_f16(torch.zeros(1, 3, 32, 32, dtype=torch.float16), 16)


def test_command_lines_take_the_precision_switch():
    from dclip_amd import flickr30k_eval, train_contrastive_teacher, zero_shot_eval
    t = train_contrastive_teacher.build_parser()
    assert t.parse_args(["--train_file", "x.json"]).tower_precision == "fp32"
    assert t.parse_args(["--train_file", "x.json", "--tower_precision", "fp16"]).tower_precision == "fp16"
    f = flickr30k_eval.build_parser()
    base = ["--dataset_json", "d.json", "--clip_path", "c"]
    assert f.parse_args(base).precision == "fp32"
    assert f.parse_args(base + ["--precision", "fp16"]).precision == "fp16"
    z = zero_shot_eval.build_parser()
    assert z.parse_args(["--data_root", "r"]).precision == "fp32"
    assert z.parse_args(["--data_root", "r", "--precision", "fp16"]).precision == "fp16"
    for p, args in ((t, ["--train_file", "x.json", "--tower_precision"]), (f, base + ["--precision"]),
                    (z, ["--data_root", "r", "--precision"])):
        with pytest.raises(SystemExit):
            p.parse_args(args + ["fp8"])


def test_meta_teacher_accepts_fp16_towers():
    from dclip_amd.clip_model import HipCLIPModel
    from dclip_amd.patch_text_aggregation import PatchTextAggregation
    cfg = dcfg.tiny()
    clip = HipCLIPModel(cfg)
    t = PatchTextAggregation(embed_dim=cfg.projection_dim, num_heads=1, clip_model=clip, tower_precision="fp16")
    assert t.text_tokenizer.precision == "fp16" and t.patch_tokenizer.precision == "fp16"
    with pytest.raises(ValueError):
        PatchTextAggregation(embed_dim=cfg.projection_dim, num_heads=1, clip_model=clip, tower_precision="fp8")


def test_model_rejects_unknown_precision_before_any_kernel():
    from dclip_amd.clip_model import HipCLIPModel
    cfg = dcfg.tiny()
    m = HipCLIPModel(cfg)
    with pytest.raises(ValueError):
        m.get_text_features(input_ids=torch.zeros(1, 4, dtype=torch.long), precision="fp8")
    from dclip_amd import eval as E
    with pytest.raises(ValueError):
        E.encoders(m, "fp8")
