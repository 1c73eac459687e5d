"""The tile-height rule of the fused split-fp16 GEMMs, restated: 192 rows where the 256-row tiles leave CUs idle
and a third more, cheaper tiles still fit the same number of rounds.  Checked at the flagship step's twelve K-major shapes, at
c4's 25 216-row shapes and under the threshold; compared with dclip_gemm_f16x3_tile_rows where the library loads."""
import pytest

CUS = 256
COST_PCT = 91            # a 192-row tile's cost relative to a 256-row one, per cent (gemm_bf16.hip, kBm192CostPct)
TILES_MIN = 128          # DCLIP_F16X3_BM192_MIN's default


def cdiv(a, b):
    return -(-a // b)


def tile_rows(M, N, stats_form=False, mode=1, tiles_min=TILES_MIN):
    if stats_form or mode <= 0:
        return 256
    if mode >= 2:
        return 192
    t256, t192 = cdiv(M, 256) * cdiv(N, 256), cdiv(M, 192) * cdiv(N, 256)
    if t256 < tiles_min:
        return 256
    return 192 if cdiv(t192, CUS) * COST_PCT < cdiv(t256, CUS) * 100 else 256


# (name, M, N, K logical): batch 256 x 50 vision tokens = 12 800 rows, 256 x 77 text tokens = 19 712 rows
STEP_192 = [("v.out", 12800, 768, 768), ("v.fc2", 12800, 768, 3072), ("d.qkv", 12800, 768, 2304), ("d.out", 12800, 768, 768),
            ("d.fc1", 12800, 768, 3072), ("t.out", 19712, 512, 512), ("t.fc2", 19712, 512, 2048)]
STEP_256 = [("v.qkv", 12800, 2304, 768), ("t.qkv", 19712, 1536, 512), ("v.fc1", 12800, 3072, 768), ("d.fc2", 12800, 3072, 768),
            ("t.fc1", 19712, 2048, 512)]
C4 = [("out", 25216, 768, 768, 192), ("fc2", 25216, 768, 3072, 192), ("qkv", 25216, 2304, 768, 256), ("fc1", 25216, 3072, 768, 256)]
SMALL = [(300, 264, 96), (1733, 520, 64), (12800, 512, 768), (6400, 768, 768), (127 * 256, 256, 64)]


def test_the_step_takes_192_rows_on_its_seven_single_round_shapes_only():
    for name, M, N, K in STEP_192:
        assert cdiv(cdiv(M, 256) * cdiv(N, 256), CUS) == 1 and cdiv(cdiv(M, 192) * cdiv(N, 256), CUS) == 1, name
        assert tile_rows(M, N) == 192, name
    for name, M, N, K in STEP_256:
        assert cdiv(cdiv(M, 192) * cdiv(N, 256), CUS) == cdiv(cdiv(M, 256) * cdiv(N, 256), CUS) + 1, name   # a round more
        assert tile_rows(M, N) == 256, name


def test_tile_counts_of_the_selected_shapes():
    assert cdiv(12800, 192) * 3 == 201 and cdiv(19712, 192) * 2 == 206        # 67 x 3 and 103 x 2 tiles: still one round
    assert 12800 - 66 * 192 == 128 and 19712 - 102 * 192 == 128               # the last tile row is partial: 128 rows


def test_c4_shapes():
    for name, M, N, K, want in C4:
        assert tile_rows(M, N) == want, name
    assert (cdiv(25216, 256) * 3, cdiv(25216, 192) * 3) == (297, 396)         # two rounds at either height


def test_under_the_threshold_and_the_other_modes():
    for M, N, K in SMALL:
        assert cdiv(M, 256) * cdiv(N, 256) < TILES_MIN and tile_rows(M, N) == 256, (M, N)
        assert tile_rows(M, N, mode=2) == 192 and tile_rows(M, N, mode=0) == 256 and tile_rows(M, N, stats_form=True, mode=2) == 256
    assert tile_rows(128 * 256, 256) == 192 and tile_rows(300, 264, tiles_min=1) == 192
    for name, M, N, K in STEP_192:
        assert tile_rows(M, N, mode=0) == 256 and tile_rows(M, N, stats_form=True) == 256, name


def test_the_library_agrees(monkeypatch):
    try:
        from dclip_amd import _lib
        lib = _lib.load()
    except (OSError, ImportError) as e:
        pytest.skip(f"the library does not load here: {e}")
    shapes = [s[1:4] for s in STEP_192 + STEP_256 + C4] + SMALL + [(128 * 256, 256, 64)]
    for mode in (None, "0", "1", "2"):
        for tiles_min in (None, "1"):
            for var, val in (("DCLIP_F16X3_BM192", mode), ("DCLIP_F16X3_BM192_MIN", tiles_min)):
                if val is None:
                    monkeypatch.delenv(var, raising=False)
                else:
                    monkeypatch.setenv(var, val)
            for M, N, K in shapes:
                for rows_form, stats_form in ((0, 0), (1, 0), (1, 1)):
                    want = tile_rows(M, N, bool(stats_form), 1 if mode is None else int(mode), TILES_MIN if tiles_min is None else 1)
                    assert lib.dclip_gemm_f16x3_tile_rows(M, N, K, rows_form, stats_form) == want, (mode, tiles_min, M, N, K, stats_form)
