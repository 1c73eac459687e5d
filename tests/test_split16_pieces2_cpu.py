"""The producer rule of the two-piece split operands, engine.split16_pieces, as a pure function of shapes and
switches: two pieces exactly where every K-major reader of the operand has the fused plan, three elsewhere.  The plan is
restated here (dclip_gemm_f16x3_plan: a logical K that is a multiple of 32 whose 3 K form takes the ping-pong kernel, and at
least 128 tiles of 256 x 256) and compared with the library where it loads."""
import itertools

import pytest

from dclip_amd import engine

TILES_MIN = 128          # DCLIP_F16X3_MIN's and DCLIP_BF16_BIG_MIN's default


def cdiv(a, b):
    return -(-a // b)


def plan(M, N, K, tiles_min=TILES_MIN):
    return 1 if M > 0 and N > 0 and K > 0 and K % 32 == 0 and (3 * K) % 64 == 0 and cdiv(M, 256) * cdiv(N, 256) >= tiles_min else 0


# the benched step: batch 256 x 50 vision tokens (ViT-B/32), 256 x 77 text tokens; (operand, its K-major reader (M, N, K logical))
T, D, I = 12800, 768, 3072
VISION = [("ln1 -> qkv", (T, 3 * D, D)), ("ctx -> out", (T, D, D)), ("ln2 -> fc1", (T, I, D)), ("g -> fc2", (T, D, I)),
          ("dx2 rows -> fc2 dgrad", (T, I, D)), ("dh rows -> fc1 dgrad", (T, D, I)), ("dx1 rows -> out dgrad", (T, D, D)),
          ("dqkv rows -> qkv dgrad", (T, D, 3 * D))]
TT, TD, TI = 19712, 512, 2048
TEXT = [("ln1 -> qkv", (TT, 3 * TD, TD)), ("ctx -> out", (TT, TD, TD)), ("ln2 -> fc1", (TT, TI, TD)), ("g -> fc2", (TT, TD, TI))]
SMALL = [(1088, 192, 64), (300, 264, 96), (6400, 768, 768), (12800, 512, 768), (127 * 256, 256, 64)]


def test_rule_is_the_conjunction_of_the_switches_and_every_readers_plan():
    yes, no = (12800, 768, 768), (1088, 192, 64)
    assert plan(*yes) == 1 and plan(*no) == 0
    for on, fused_k in itertools.product((False, True), repeat=2):
        for consumers in ([yes], [yes, yes], [no], [yes, no], [no, yes]):
            want = 2 if on and fused_k and all(plan(*c) for c in consumers) else 3
            assert engine.split16_pieces(consumers, plan=plan, on=on, fused_k=fused_k) == want, (on, fused_k, consumers)
        assert engine.split16_pieces([], plan=plan, on=on, fused_k=fused_k) == 3          # nobody reads it fused: the parent's layout


def test_the_step_gives_two_pieces_for_all_eight_vision_operands_and_the_text_towers():
    for name, c in VISION + TEXT:
        assert engine.split16_pieces([c], plan=plan, on=True, fused_k=True) == 2, name
        assert engine.split16_pieces([c], plan=plan, on=False, fused_k=True) == 3, name
        assert engine.split16_pieces([c], plan=plan, on=True, fused_k=False) == 3, name


def test_three_pieces_under_the_threshold():
    for c in SMALL:
        assert cdiv(c[0], 256) * cdiv(c[1], 256) < TILES_MIN
        assert engine.split16_pieces([c], plan=plan, on=True, fused_k=True) == 3, c
        low = engine.split16_pieces([c], plan=lambda M, N, K: plan(M, N, K, 1), on=True, fused_k=True)
        assert low == (2 if (3 * c[2]) % 64 == 0 else 3), c              # (K = 96: 3 K = 288 is no multiple of the 64-wide K-tile)
    assert engine.split16_pieces([(128 * 256, 256, 48)], plan=plan, on=True, fused_k=True) == 3       # K not a multiple of 32


def test_the_library_and_the_layer_tables_agree(monkeypatch):
    try:
        from dclip_amd import _lib
        lib = _lib.load()
    except (OSError, ImportError) as e:
        pytest.skip(f"the library does not load here: {e}")
    for var in ("DCLIP_F16X3_MIN", "DCLIP_BF16_BIG_MIN"):
        monkeypatch.delenv(var, raising=False)
    for _, c in VISION + TEXT:
        assert lib.dclip_gemm_f16x3_plan(*c) == plan(*c) == 1
    for c in SMALL + [(128 * 256, 256, 48)]:
        assert lib.dclip_gemm_f16x3_plan(*c) == plan(*c) == 0
    monkeypatch.setattr(engine, "_SPLIT16_FUSED_K", True)
    monkeypatch.setattr(engine, "_SPLIT16_PIECES2", True)
    two, three = {"ln1": 2, "ctx": 2, "ln2": 2, "g": 2}, {"ln1": 3, "ctx": 3, "ln2": 3, "g": 3}
    for fc1_epi in (True, False):
        assert engine._layer_pieces(T, D, I, fc1_epi) == two and engine._layer_pieces(TT, TD, TI, fc1_epi) == two
        assert engine._layer_pieces(1088, 64, 256, fc1_epi) == three
    # qkv and fc1 over the threshold, out and fc2 (N = D) under it: the operands the latter two read keep three pieces
    assert engine._layer_pieces(12800, 512, 2048, True) == {"ln1": 2, "ctx": 3, "ln2": 2, "g": 3}
    monkeypatch.setattr(engine, "_SPLIT16_PIECES2", False)
    assert engine._layer_pieces(T, D, I, True) == three
    monkeypatch.setattr(engine, "_SPLIT16_PIECES2", True)
    monkeypatch.setattr(engine, "_SPLIT16_FUSED_K", False)
    assert engine._layer_pieces(T, D, I, True) == three
