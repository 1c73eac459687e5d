"""Split-fp16 forward of the student's vision tower, the parts that need no GPU: the host mirror of the device
plan (engine.split16_plan_host) on crafted statistics, and the ABI of the device-scaled entries."""
import ctypes
import math
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STATS = ("ln1_w", "ln1_b", "v_l1", "v_b", "ln2_w", "ln2_b", "fc1_l1", "fc1_b", "qkv", "out", "fc1", "fc2")


def stats(**kw):
    st = {"ln1_w": 1.2, "ln1_b": 0.1, "v_l1": 3.5, "v_b": 0.2, "ln2_w": 0.9, "ln2_b": 0.3, "fc1_l1": 5.0, "fc1_b": 0.4,
          "qkv": 0.11, "out": 0.07, "fc1": 0.2, "fc2": 0.05}
    st.update(kw)
    return st


def test_stat_names_agree():
    from dclip_amd import engine, ops
    assert engine._SPLIT16_STATS == STATS == ops.SPLIT16_STATS


def test_plan_host_follows_the_host_rules():
    from dclip_amd import engine
    D = 72
    st = stats()
    plan = engine.split16_plan_host(st, D)
    b = engine.split16_layer_bounds(st, D)
    assert plan["flags"] == 0
    assert plan["e"] == {k: engine.split16_act_exp(v) for k, v in b.items()}
    assert plan["f"] == {k: engine.split16_weight_exp(st[k]) for k in ("qkv", "out", "fc1", "fc2")}
    assert plan["a"] == {"qkv": -(plan["e"]["ln1"] + plan["f"]["qkv"]), "out": -(plan["e"]["ctx"] + plan["f"]["out"]),
                         "fc1": -(plan["e"]["ln2"] + plan["f"]["fc1"]), "fc2": -(plan["e"]["g"] + plan["f"]["fc2"])}
    for k, e in plan["e"].items():
        assert b[k] * 2.0 ** e <= 2.0 ** 14 < b[k] * 2.0 ** (e + 1)


def test_plan_host_zero_weight_and_power_of_two_bound():
    from dclip_amd import engine
    plan = engine.split16_plan_host(stats(fc2=0.0, ln1_w=0.0, ln1_b=0.5), 72)     # LayerNorm-1 bound = 0.5 exactly
    assert plan["flags"] == 0
    assert plan["f"]["fc2"] == 0
    assert plan["e"]["ln1"] == 15                                                # 0.5 * 2^15 = 2^14: the bound itself fits
    assert engine.split16_plan_host(stats(ln1_w=0.0, ln1_b=0.5000001), 72)["e"]["ln1"] == 14
    zero = engine.split16_plan_host(stats(ln2_w=0.0, ln2_b=0.0, fc1_b=0.0), 72)
    assert zero["e"]["ln2"] == 24 and zero["e"]["g"] == 24 and zero["flags"] == 0


def test_plan_host_has_no_fall_back():
    """gamma = 1e7: an activation scale below 2^-14.  The host guard declines (None); the device rule takes that exponent and
    flags it.  A non-finite statistic: flag 2, exponent 0."""
    from dclip_amd import engine
    D = 72
    st = stats(ln2_w=1e7)
    b = engine.split16_layer_bounds(st, D)
    assert engine.split16_act_exp(b["g"]) is None
    plan = engine.split16_plan_host(st, D)
    assert plan["flags"] == 1
    for k in ("ln2", "g"):
        e = plan["e"][k]
        assert b[k] * 2.0 ** e <= 2.0 ** 14 < b[k] * 2.0 ** (e + 1)
    assert plan["e"]["g"] < -14
    inf = engine.split16_plan_host(stats(fc1=math.inf, fc1_l1=math.inf), D)
    assert inf["flags"] == 2 and inf["f"]["fc1"] == 0 and inf["e"]["g"] == 0
    assert inf["e"]["ln1"] == engine.split16_plan_host(stats(), D)["e"]["ln1"]     # the other layers' exponents do not move
    nan = engine.split16_plan_host(stats(ln1_w=math.nan), D)
    assert nan["flags"] == 2 and nan["e"]["ln1"] == 0 and nan["e"]["ctx"] == 0
    # scales beyond fp32's normal range are clamped and flagged
    huge = engine.split16_plan_host(stats(ln1_w=3e38, v_l1=3e38), D)
    assert huge["flags"] & 4 and huge["e"]["ctx"] == -126


def test_header_binding_and_symbols_agree():
    from dclip_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "dclip_hip.h")).read(), flags=re.S)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("dclip_split_f32_f16x3_dev", 9), ("dclip_layernorm_fwd_f16x3_dev", 12), ("dclip_gemm_f16_scaled_dev", 15),
                        ("dclip_gemm_f16_scaled_split_dev", 16), ("dclip_split16_stats", 5), ("dclip_split16_plan", 5),
                        ("dclip_split16_weights", 5)):
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, src)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name), name
    # a device-scaled entry differs from its scalar twin only in the type of the scale arguments
    for name in ("dclip_split_f32_f16x3", "dclip_gemm_f16_scaled"):
        a, b = _lib.SIGNATURES[name][1], _lib.SIGNATURES[name + "_dev"][1]
        assert len(a) == len(b) and all(x is y or x is ctypes.c_float for x, y in zip(a, b))
    assert lib.dclip_split16_record_bytes() == 48 and lib.dclip_split16_plan_floats() == 32


def test_argument_errors():
    from dclip_amd import _lib
    lib = _lib.load()
    cases = [
        (lambda: lib.dclip_split_f32_f16x3_dev(16, 16, 1, 8, 8, 24, None, 0, None), b"split_f32_f16x3_dev: bad arguments"),
        (lambda: lib.dclip_split_f32_f16x3_dev(16, 16, 1, 12, 12, 40, 16, 0, None), b"multiple of 8"),
        (lambda: lib.dclip_split_f32_f16x3_dev(16, 16, 1, 8, 8, 24, 16, 2, None), b"order"),
        (lambda: lib.dclip_layernorm_fwd_f16x3_dev(16, 16, 16, 16, None, None, None, 4, 8, 1e-5, None, None), b"null pointer"),
        (lambda: lib.dclip_layernorm_fwd_f16x3_dev(16, 16, 16, 16, None, None, None, 4, 6, 1e-5, 16, None), b"bad D"),
        (lambda: lib.dclip_gemm_f16_scaled_dev(16, 16, 16, None, None, 4, 4, 4, 8, 8, 4, 0, 0, None, None), b"alpha must be a device pointer"),
        (lambda: lib.dclip_gemm_f16_scaled_split_dev(16, 16, 16, None, None, None, 4, 8, 8, 8, 8, 24, 0, None, 16, None), b"device pointers"),
        (lambda: lib.dclip_gemm_f16_scaled_split_dev(16, 16, 16, None, 16, None, 4, 8, 8, 8, 8, 24, 0, 16, 16, None), b"pre-activation of a GELU"),
        (lambda: lib.dclip_gemm_f16_scaled_split_dev(16, 16, 16, None, None, 16, 4, 8, 8, 8, 8, 24, 0, 16, None, None), b"g32 must be NULL"),
        (lambda: lib.dclip_gemm_f16_scaled_split_dev(16, 16, 16, None, None, None, 4, 8, 8, 8, 8, 24, 8, 16, 16, None), b"BIAS | GELU"),
        (lambda: lib.dclip_split16_stats(None, 1, 1, 16, None), b"split16_stats: bad arguments"),
        (lambda: lib.dclip_split16_plan(16, None, 1, 8, None), b"split16_plan: bad arguments"),
        (lambda: lib.dclip_split16_weights(16, 0, 1, 16, None), b"split16_weights: bad arguments"),
    ]
    for call, msg in cases:
        assert call() == -1
        assert msg in lib.dclip_last_error(), (msg, lib.dclip_last_error())


def test_switch_is_read_once():
    from dclip_amd import engine
    assert engine.vision_split16_enabled() == (os.environ.get("DCLIP_VISION_SPLIT16", "1") != "0")
    src = open(os.path.join(REPO, "dclip_amd", "engine.py")).read()
    assert src.count('os.environ.get("DCLIP_VISION_SPLIT16"') == 1
    for f in ("split16.hip", "gemm_bf16.hip"):
        assert "DCLIP_VISION" not in open(os.path.join(REPO, "dclip_amd", "csrc", f)).read()      # no getenv on the launch path
