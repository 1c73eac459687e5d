"""The gate of the split-fp16 patch embedding, engine.patch_split16_taken, as a pure function of shapes and
switches: taken on the benched configurations' shapes (c2: ViT-B/32, c4: ViT-B/16, 256 images), declined by ViT-L/14 (patch_dim
588), by a patch-row count that is no multiple of 64, on another grid, without the model's cache and under the thresholds.  The two
plans are restated here (dclip_split16_patch_plan: dclip_gemm_f16x3_plan and at least 128 tiles of 256 x 256;
dclip_gemm_f16x3_wgrad_tokmajor_plan) and compared with the library where it loads.  The host rule of the front plan
(engine.split16_front_host) is checked at the corners the device test uses."""
import itertools
import math

import pytest

from dclip_amd import engine

TILES_MIN = 128          # the default of DCLIP_F16X3_MIN, DCLIP_BF16_BIG_MIN, DCLIP_PATCH_SPLIT16_MIN and DCLIP_F16X3_TOK_MIN


def cdiv(a, b):
    return -(-a // b)


def plan(rows, D, K, tiles_min=TILES_MIN):
    ok = rows > 0 and D > 0 and K > 0 and K % 32 == 0 and (3 * K) % 64 == 0
    return 1 if ok and cdiv(rows, 256) * cdiv(D, 256) >= tiles_min else 0


def wplan(M, N, tokens, items_min=TILES_MIN):
    if M <= 0 or N <= 0 or tokens <= 0 or tokens % 64 or M % 8 or N % 8:
        return 0
    t256 = cdiv(M, 256) * cdiv(N, 256)
    s = 1 if t256 >= 256 else 256 // t256
    s = min(s, max(tokens // 192, 1), 64)
    s = cdiv(tokens, cdiv(cdiv(tokens, s), 64) * 64)
    return s if t256 * s >= items_min else 0


# (rows, D, patch_dim) of 256 images
C2 = (256 * 49, 768, 3 * 32 * 32)          # ViT-B/32: 12,544 x 768 x 3,072
C4 = (256 * 196, 768, 3 * 16 * 16)         # ViT-B/16: 50,176 x 768 x 768
L14 = (256 * 256, 1024, 3 * 14 * 14)       # c5's ViT-L/14 teacher: patch_dim 588
TINY64 = (64 * 16, 128, 768)               # the tiny tower of the GPU tests: 4 tiles


def taken(shape, backward=False, save=True, grid=None, on=True, tiles_min=TILES_MIN):
    return engine.patch_split16_taken(save, grid, *shape, backward=backward, on=on,
                                      plan=lambda r, d, k: plan(r, d, k, tiles_min), wplan=lambda m, n, t: wplan(m, n, t, tiles_min))


def test_the_benched_shapes_are_taken_and_l14_declines():
    for shape in (C2, C4):
        assert taken(shape) and taken(shape, backward=True), shape
    assert L14[2] % 32 != 0 and not taken(L14) and not taken(L14, backward=True)
    assert not taken(L14, tiles_min=1)                                        # whatever the thresholds say


def test_the_gate_is_the_conjunction():
    for on, save, grid in itertools.product((False, True), (False, True), (None, (7, 7))):
        assert taken(C2, on=on, save=save, grid=grid) == (on and save and grid is None)
    assert not taken((C2[0] + 32, C2[1], C2[2]))                              # rows % 64
    assert not taken((255 * 49, 768, 3072))                                   # 12,495 rows
    assert not taken((C2[0], C2[1], 3 * 12 * 12))                             # patch 12: 432 is no multiple of 32
    assert not taken((0, 768, 3072))
    assert not taken(TINY64) and not taken(TINY64, backward=True)             # under the thresholds
    assert taken(TINY64, tiles_min=1) and taken(TINY64, backward=True, tiles_min=1)
    # the backward half needs its own plan as well
    assert engine.patch_split16_taken(True, None, *C2, backward=True, on=True, plan=plan, wplan=lambda m, n, t: 0) is False
    assert engine.patch_split16_taken(True, None, *C2, backward=False, on=True, plan=plan, wplan=lambda m, n, t: 0) is True


def test_the_switches_nest(monkeypatch):
    for vs, patch, bwd, wgrad in itertools.product((False, True), repeat=4):
        monkeypatch.setattr(engine, "_VSPLIT16", vs)
        monkeypatch.setattr(engine, "_VSPLIT16_PATCH", patch)
        monkeypatch.setattr(engine, "_VSPLIT16_BWD", bwd)
        monkeypatch.setattr(engine, "_VSPLIT16_WGRAD", wgrad)
        assert engine.patch_split16_taken(True, None, *C2, plan=plan, wplan=wplan) == (vs and patch)
        assert engine.patch_split16_taken(True, None, *C2, backward=True, plan=plan, wplan=wplan) == (vs and patch and bwd and wgrad)


def test_the_library_agrees(monkeypatch):
    try:
        from dclip_amd import _lib
        lib = _lib.load()
    except (OSError, ImportError) as e:
        pytest.skip(f"the library does not load here: {e}")
    for var in ("DCLIP_F16X3_MIN", "DCLIP_BF16_BIG_MIN", "DCLIP_PATCH_SPLIT16_MIN", "DCLIP_F16X3_TOK_MIN"):
        monkeypatch.delenv(var, raising=False)
    for shape in (C2, C4, L14, TINY64, (C2[0] + 32, 768, 3072)):
        rows, D, K = shape
        assert lib.dclip_split16_patch_plan(rows, D, K) == plan(rows, D, K), shape
        assert lib.dclip_gemm_f16x3_wgrad_tokmajor_plan(D, K, rows) == wplan(D, K, rows), shape
    for name in ("_VSPLIT16", "_VSPLIT16_PATCH", "_VSPLIT16_BWD", "_VSPLIT16_WGRAD"):
        monkeypatch.setattr(engine, name, True)
    assert engine.patch_split16_taken(True, None, *C2, backward=True) and engine.patch_split16_taken(True, None, *C4, backward=True)
    assert not engine.patch_split16_taken(True, None, *L14) and not engine.patch_split16_taken(True, None, *TINY64)
    # the path's own threshold: lowering the other three leaves the tiny tower's patch embedding where it was
    for var in ("DCLIP_F16X3_MIN", "DCLIP_BF16_BIG_MIN", "DCLIP_F16X3_TOK_MIN"):
        monkeypatch.setenv(var, "1")
    assert lib.dclip_gemm_f16x3_plan(*TINY64) == 1 and not engine.patch_split16_taken(True, None, *TINY64)
    monkeypatch.setenv("DCLIP_PATCH_SPLIT16_MIN", "1")
    assert engine.patch_split16_taken(True, None, *TINY64, backward=True)


def test_front_host_rule():
    f = engine.split16_front_host
    assert f(4.0, 0.05) == {"e": 12, "f": 18, "a": -30, "flags": 0}                       # 4 = 0.5 2^3: 4 2^12 = 2^14 exactly
    assert f(math.nextafter(4.0, 5.0), 0.05)["e"] == 11
    assert f(0.0, 0.03) == {"e": 24, "f": 19, "a": -43, "flags": 0}
    assert f(2.64, 0.0) == {"e": 12, "f": 0, "a": -12, "flags": 0}
    assert f(65504.0, 0.02)["e"] == -2
    assert f(float("nan"), 0.05) == {"e": 0, "f": 18, "a": -18, "flags": 2} == f(float("inf"), 0.05)
    assert f(1.0, float("inf")) == {"e": 14, "f": 0, "a": -14, "flags": 2}
    assert f(2.0 ** 29 * 1.5, 0.05) == {"e": -16, "f": 18, "a": -2, "flags": 1}
    assert f(2.0 ** 127, 2.0 ** -149) == {"e": -113, "f": 127, "a": -14, "flags": 5}       # f = 162 clamped
