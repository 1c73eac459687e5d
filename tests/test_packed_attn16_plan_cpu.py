"""Host side of the 16-bit packed attention core: the four entries in the binding, the header and the built
library; the switch's default; the route function spelled out; the model attribute and the launchers' flag; and the checks of
tests/kernel_checks_varlen16.py on a fp64 emulation of the kernels' documented roundings — which pass, and which fail once one
key of the next sequence is made visible across a seam."""
import argparse
import ctypes
import itertools
import os

import pytest
import torch

from dclip_amd import config as dcfg
from dclip_amd.clip_model import HipCLIPModel
from tests import kernel_checks as kc
from tests import kernel_checks_varlen16 as kv
from tests.test_abi_cpu import declared_symbols

ENTRIES = ["dclip_attention_varlen_fwd_bf16", "dclip_attention_varlen_fwd_f16", "dclip_attention_varlen_row_fwd_bf16",
           "dclip_attention_varlen_row_fwd_f16"]


def test_the_four_entries_are_bound_declared_and_exported():
    from dclip_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    exported = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == 8, name
        assert name in declared_symbols(), name
        assert hasattr(exported, name), f"{name} not exported"
    assert _lib.load().dclip_abi_version() == 1


def test_refusals_do_not_need_a_gpu():
    from dclip_amd import _lib
    lib = _lib.load()
    ptr = 4096                                   # never dereferenced: every case below is refused before a launch
    good = [ptr, ptr, ptr, 2, 4, 2, 0, None]
    bad = [(0, None), (1, None), (2, None), (3, 0), (3, -1), (4, 0), (4, -1), (5, 0), (5, -2), (3, 2 ** 30), (0, ptr + 8),
           (2, ptr + 8), (1, ptr + 2)]
    for name in ENTRIES:
        for at, value in bad + ([(4, 513)] if "_row_" in name else []):
            args = list(good)
            args[at] = value
            assert getattr(lib, name)(*args) == kc.E_INVAL, (name, at, value)
            assert name[len("dclip_"):].encode() in lib.dclip_last_error(), (name, lib.dclip_last_error())


def test_the_switch_is_off_by_default():
    """The value is read once at import: this process's (unset: False), and a child's with the variable set."""
    import subprocess
    import sys
    from dclip_amd import engine
    assert engine._PACKED_ATTN16 is (os.environ.get("DCLIP_PACKED_ATTN16", "0") != "0")
    if "DCLIP_PACKED_ATTN16" not in os.environ:
        assert engine._PACKED_ATTN16 is False
    code = "from dclip_amd import engine; print(engine._PACKED_ATTN16, engine.packed_attn16_route('bf16', 77, False))"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for value, want in (("1", "True tiled16"), ("0", "False f32")):
        out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, DCLIP_PACKED_ATTN16=value), cwd=root,
                             capture_output=True, text=True, check=True, timeout=300)
        assert out.stdout.strip() == want, (value, out.stdout, out.stderr)


def test_the_route_spelled_out(monkeypatch):
    from dclip_amd import engine
    route = engine.packed_attn16_route
    want = {}
    for prec, max_S, one_row, on in itertools.product(("fp32", "split16", "bf16", "fp16"), (1, 512, 513), (False, True),
                                                      (False, True)):
        if not on or prec in ("fp32", "split16"):
            want[prec, max_S, one_row, on] = "f32"                  # off, fp32 or the split-fp16 plan: today's route
        elif not one_row:
            want[prec, max_S, one_row, on] = "tiled16"              # full layers, any length
        else:
            want[prec, max_S, one_row, on] = "row16" if max_S <= 512 else "f32"
    assert want["bf16", 512, True, True] == "row16" and want["fp16", 513, True, True] == "f32"
    assert want["bf16", 513, False, True] == "tiled16" and want["bf16", 1, True, False] == "f32"
    for key, r in want.items():
        assert route(*key) == r, key
    # None: the module value
    for module_value in (False, True):
        monkeypatch.setattr(engine, "_PACKED_ATTN16", module_value)
        for prec, max_S, one_row in itertools.product(("fp32", "bf16", "fp16"), (1, 512, 513), (False, True)):
            assert route(prec, max_S, one_row, None) == want[prec, max_S, one_row, module_value]
            assert route(prec, max_S, one_row) == want[prec, max_S, one_row, module_value]
            assert route(prec, max_S, one_row, not module_value) == want[prec, max_S, one_row, not module_value]


def test_the_model_attribute_and_the_flag():
    from dclip_amd import CLIP_image_distill_training as student_launcher, train_contrastive_teacher as teacher_launcher
    from dclip_amd.CLIP_image_distillation import CLIPImageDistillation
    from dclip_amd.patch_text_aggregation import PatchTextAggregation
    cfg = dcfg.tiny()
    assert HipCLIPModel.packed_attention16 is None and HipCLIPModel(cfg).packed_attention16 is None
    for launcher in (student_launcher, teacher_launcher):
        p = launcher.build_parser()
        assert p.parse_args(["--train_file", "x.json"]).packed_attention16 is False
        assert p.parse_args(["--train_file", "x.json", "--packed_attention16"]).packed_attention16 is True
    m = HipCLIPModel(cfg)
    assert PatchTextAggregation(embed_dim=cfg.projection_dim, num_heads=1, clip_model=m)._clip.packed_attention16 is None
    assert PatchTextAggregation(embed_dim=cfg.projection_dim, num_heads=1, clip_model=m, packed_attention16=True)._clip \
        .packed_attention16 is True
    assert m.packed_attention16 is True
    assert PatchTextAggregation(embed_dim=cfg.projection_dim, num_heads=1, clip_model=m, packed_attention16=False)._clip \
        .packed_attention16 is False
    hp = argparse.Namespace(learning_rate=1e-4, warmup_steps=0, total_steps=10, train_batch_size=2, eval_batch_size=2)
    off = CLIPImageDistillation(hp, HipCLIPModel(cfg), None)
    assert off.packed_attention16 is None and off.student.packed_attention16 is None
    assert off.teacher._clip.packed_attention16 is None
    on = CLIPImageDistillation(hp, HipCLIPModel(cfg), None, packed_attention16=True)
    assert on.packed_attention16 is True and on.student.packed_attention16 is True and on.teacher._clip.packed_attention16 is True


# ------------------------------------------------------------------------------------------------ the checks can pass and fail

GPU_LENGTHS = {"full": [([1, 2, 17, 31, 32, 33, 63, 64, 65, 128, 129, 5], 2), ([197, 3, 257], 1), ([64], 3)],
               "causal": [([1, 2, 17, 31, 32, 33, 63, 64, 65, 77, 5], 2), ([128, 129, 3], 1), ([64], 3)],
               "cls": [([1, 2, 50, 63, 64, 65, 77, 257, 300, 512, 5], 1), ([1, 64, 65], 3)],
               "last": [([1, 2, 50, 63, 64, 65, 77, 257, 300, 512, 5], 1), ([1, 64, 65], 3)]}


@pytest.mark.parametrize("mode", kv.MODES)
def test_the_selection_margins_of_the_gpu_cases(mode):
    """The exact-selection data of tests/test_varlen16_paths_gpu.py: every sequence's margin is at least MIN_MARGIN, so every
    probability but the selected one is exactly 0 in fp32."""
    for lengths, H in GPU_LENGTHS[mode] + [([5, 0, 9], 2)]:
        pack = kv.build_pack(lengths, H, "bf16", mode, "select")
        kv.assert_margins(pack)
        assert min(m for m in kv.margins(pack) if m is not None) >= kc.MIN_MARGIN


@pytest.mark.parametrize("ty", ["bf16", "f16"])
@pytest.mark.parametrize("mode", kv.MODES)
def test_an_emulation_of_the_documented_roundings_passes_both_checks(mode, ty):
    lengths, H = [5, 33, 0, 65, 9], 2
    sel = kv.build_pack(lengths, H, ty, mode, "select")
    kv.assert_margins(sel)
    assert kv.selection_failures(sel, kv.emulate_pack(sel)) == []
    gauss = kv.build_pack(lengths, H, ty, mode, "gauss")
    out = kv.emulate_pack(gauss)
    ratios = [r for r in kv.bound_ratios(gauss, out) if r is not None]
    assert len(ratios) == 4 and max(ratios) <= 1.0, ratios
    # the emulation is the per-sequence one of tests/kernel_checks.py
    for n, (got, s) in enumerate(zip(kv.per_sequence(gauss, out), gauss.seqs)):
        if s is not None:
            want = kc.attn16_forward(s, gauss.ty)[0]
            assert torch.equal(got, want.permute(0, 2, 1, 3).reshape(got.shape)), n


@pytest.mark.parametrize("mode", kv.MODES)
def test_a_key_of_the_next_sequence_seen_across_the_seam_fails_the_selection_check(mode):
    """Sequence 1 also sees the first key row of sequence 2.  That row is made the worst neighbour a pack can hold: per head a
    twin of the key one query of sequence 1 selects, with a value of its own — the probability splits in two and v[pi] is
    missed.  (A random +-8 key scores at most 512 - 16 and stays invisible, as any masked-in key does in this data.)"""
    lengths, H, n = [5, 33, 65, 9], 2, 1
    pack = kv.build_pack(lengths, H, "bf16", mode, "select")
    S = lengths[n]
    s, nxt = pack.seqs[n], pack.seqs[n + 1]
    qr = kv.query_row(pack, n) if pack.row else S - 1                           # a query of sequence 1: the row entry's, else the last
    picked = s.pi[0, :, qr]                                                     # [H]: the key that query selects
    nxt.k[0, :, 0] = s.k[0, torch.arange(H), picked]
    nxt.v[0, :, 0] = s.v[0, torch.arange(H), picked] + 1.0
    clean = kv.emulate_pack(pack)
    assert n not in [m for m, _ in kv.selection_failures(pack, clean)]
    leaked = kv.emulate_pack(pack, leak=(n, nxt.k[0, :, 0], nxt.v[0, :, 0]))
    bad = dict(kv.selection_failures(pack, leaked))
    assert n in bad, bad
    got, want = kv.per_sequence(pack, leaked)[n], kv.selection_want(pack)[n]
    assert torch.equal(got[-1], want[-1] + 0.5)                                 # half of each of the two values
    # and the Gaussian bound notices a foreign key too
    gauss = kv.build_pack(lengths, H, "bf16", mode, "gauss")
    g2 = gauss.seqs[n + 1]
    out = kv.emulate_pack(gauss, leak=(n, g2.k[0, :, 0], g2.v[0, :, 0]))
    ratios = kv.bound_ratios(gauss, out)
    assert ratios[n] > 1.0 and all(r <= 1.0 for m, r in enumerate(ratios) if m != n), ratios
