"""The layer above the towers on the GPU: functional.CosineDistillationLossFn / ContrastiveLossFn,
distill_losses, TeacherBridge, CrossModalFn, GlobalPoolFn / AggregationFn and the glue of PatchTextAggregation, through the
cases and checkers of tests/head_checks.py: every tensor against the fp64 oracle under §26's fp32 gate, and the exact checkers
(linearity in the upstream gradient, need_x, frozen subsets, teacher operand, shared operand, row independence of the padding,
the three guards, the launch route of every cross-attention call, repeatability).  Each case prints its worst E / gate."""
import contextlib
from types import SimpleNamespace

import pytest
import torch

from tests import head_checks as hc

pytestmark = pytest.mark.gpu


class Product:
    """The product's own functions behind the interface head_checks runs."""

    def __init__(self, device):
        self.device = device

    @contextlib.contextmanager
    def watch(self):
        """The launch site dclip_last_launch reports right after every cross-attention call."""
        from dclip_amd import _lib, ops
        lib, names = _lib.load(), []
        saved = ops.cross_attention_fwd, ops.cross_attention_bwd

        def spy(fn):
            def call(*a, **k):
                out = fn(*a, **k)
                names.append(lib.dclip_last_launch().decode())
                return out
            return call
        ops.cross_attention_fwd, ops.cross_attention_bwd = spy(saved[0]), spy(saved[1])
        try:
            yield names
        finally:
            ops.cross_attention_fwd, ops.cross_attention_bwd = saved

    def cosine(self, s, t):
        from dclip_amd import functional
        return functional.cosine_distillation_loss(s, t)

    def contrastive(self, i, t, temperature):
        from dclip_amd import functional
        return functional.contrastive_loss(i, t, temperature)

    def distill_losses(self, si, st, ti, tt, temperature):
        from dclip_amd.CLIP_image_distillation import distill_losses
        return distill_losses(si, st, ti, tt, temperature)

    def bridge(self, student_dim, teacher_dim):
        from dclip_amd.CLIP_image_distillation import TeacherBridge
        return TeacherBridge(student_dim, teacher_dim).to(self.device)

    def block(self, E, H, sd):
        from dclip_amd.patch_text_aggregation import CrossModalAttention
        b = CrossModalAttention(E, H)
        b.load_state_dict(sd)
        return b.to(self.device)

    def pool(self, at, ai, temperature):
        from dclip_amd.patch_text_aggregation import GlobalPoolFn
        return GlobalPoolFn.apply(at, ai, temperature)

    def aggregation(self, x, temperature):
        from dclip_amd.patch_text_aggregation import AggregationFn
        return AggregationFn.apply(x, temperature)

    def global_from_tokens(self, block, text, patches):
        from dclip_amd.patch_text_aggregation import PatchTextAggregation
        return PatchTextAggregation.global_embedding_from_tokens(SimpleNamespace(cross_modal_attention=block), text, patches)

    def teacher(self, cfg, clip_sd, cm_sd, packed_text):
        from dclip_amd.clip_model import from_hf_state_dict
        from dclip_amd.patch_text_aggregation import PatchTextAggregation
        clip = from_hf_state_dict(cfg, clip_sd, device=self.device)
        t = PatchTextAggregation(embed_dim=cfg.projection_dim, num_heads=cfg.projection_dim // 64, clip_model=clip,
                                 packed_text=packed_text)
        t.load_state_dict({f"cross_modal_attention.{k}": v for k, v in cm_sd.items()})
        return t.to(self.device)


@pytest.fixture(scope="module")
def be():
    assert torch.cuda.is_available()
    return Product(torch.device("cuda:0"))


def show(what, ref, ratios):
    n32 = max(ref.e_ref32, key=ref.e_ref32.get)
    n, r = hc.worst(ratios)
    print(f"HEAD {what}: E_ref32 max {ref.e_ref32[n32]:.2e} ({n32}); worst E/gate {r:.3f} ({n})")


# ------------------------------------------------------------------------------------------------ loss head

@pytest.mark.parametrize("kind", ["cosine", "contrastive"])
@pytest.mark.parametrize("c", hc.LOSS_CASES, ids=lambda c: c.id)
def test_loss_cases(be, kind, c):
    show(f"{kind} {c.id}", hc.loss_ref(kind, c), hc.check_loss_case(be, kind, c))


@pytest.mark.parametrize("kind", ["cosine", "contrastive"])
@pytest.mark.parametrize("cid", ["6x64", "33x512", "6x768to512.bridge"])
def test_loss_linearity_in_the_upstream_gradient(be, kind, cid):
    c = hc.LOSS_BY_ID[cid]
    ref = hc.loss_ref(kind, c)
    show(f"{kind} {cid} g=1/3", ref, hc.check_linearity(lambda g: hc.run_loss(be, kind, c, g), ref, f"{kind} {cid}"))


def test_teacher_operand_and_bridge(be):
    hc.check_teacher_operand(be, hc.LOSS_BY_ID["6x64"])
    hc.check_teacher_operand(be, hc.LOSS_BY_ID["6x768to512.bridge"])
    hc.check_bridge(be, hc.LOSS_BY_ID["6x768to512.bridge"])


@pytest.mark.parametrize("cid", ["6x64", "33x512"])
def test_distill_losses_shared_operand(be, cid):
    c = hc.LOSS_BY_ID[cid]
    show(f"distill_losses {cid}", hc.distill_ref(c), hc.check_shared_operand(be, c))
    if cid == "6x64":
        hc.check_linearity(lambda g: hc.run_distill(be, c, g), hc.distill_ref(c), f"distill_losses {cid}")


# ------------------------------------------------------------------------------------------------ cross-modal block

@pytest.mark.parametrize("c", hc.BLOCK_CASES, ids=lambda c: c.id)
def test_block_cases(be, c):
    """Outputs, d_text / d_patch and the 12 parameter gradients under the gate; the four launch names; exact zeros in the q / k
    thirds of a one-key direction."""
    show(f"block {c.id}", hc.block_ref(c), hc.check_block_case(be, c))


@pytest.mark.parametrize("c", hc.BLOCK_CASES, ids=lambda c: c.id)
def test_block_linearity_in_the_upstream_gradient(be, c):
    ref = hc.block_ref(c)
    show(f"block {c.id} g=1/3", ref, hc.check_linearity(lambda g: hc.run_block(be, c, g)[0], ref, f"block {c.id}"))


@pytest.mark.parametrize("c", hc.BLOCK_CASES, ids=lambda c: c.id)
def test_block_need_x(be, c):
    hc.check_need_x(be, c)


@pytest.mark.parametrize("which", sorted(hc.FROZEN_SETS))
@pytest.mark.parametrize("cid", ["ragged", "square", "one_key", "c3_width"])
def test_block_frozen_subsets(be, cid, which):
    hc.check_frozen(be, hc.BLOCK_BY_ID[cid], hc.FROZEN_SETS[which])


@pytest.mark.parametrize("c", hc.BLOCK_CASES, ids=lambda c: c.id)
def test_block_two_backwards_over_one_graph(be, c):
    hc.check_repeatability(be, c)


# ------------------------------------------------------------------------------------------------ pooling

@pytest.mark.parametrize("kind", ["global", "agg"])
@pytest.mark.parametrize("c", hc.POOL_CASES, ids=lambda c: c.id)
def test_pool_cases(be, kind, c):
    ref = hc.pool_ref(kind, c)
    show(f"{kind} pool {c.id}", ref, hc.check_pool_case(be, kind, c))
    hc.check_linearity(lambda g: hc.run_pool(be, kind, c, g), ref, f"{kind} pool {c.id}")


# ------------------------------------------------------------------------------------------------ guards

@pytest.mark.parametrize("cid", ["ragged", "square", "one_key"])
def test_guards_1_and_2(be, cid):
    c = hc.BLOCK_BY_ID[cid]
    show(f"guards (1)(2) {cid}", hc.global_ref(c, 0, (1, c.R - 1)), hc.check_guards_1_2(be, c))


@pytest.mark.parametrize("cid", ["ragged", "square"])
def test_guard_3(be, cid):
    c = hc.BLOCK_BY_ID[cid]
    show(f"guard (3) {cid}, the clean pass after it", hc.global_ref(c), hc.check_guard_3(be, c))


# ------------------------------------------------------------------------------------------------ glue

@pytest.fixture(scope="module")
def glue_results():
    return {}


@pytest.mark.parametrize("packed_text", [False, True], ids=["padded", "packed_text"])
@pytest.mark.parametrize("c", hc.GLUE_CASES, ids=lambda c: c.id)
def test_glue_cases(be, glue_results, c, packed_text):
    """compute_global_embedding_tensors + contrastive_loss(global, last_sentence_embedding) against O.teacher_step fed the
    oracle's own tower outputs; both text paths; the launch names of the block the glue built."""
    what = f"glue {c.id}" + (" packed_text" if packed_text else "")
    got, names, _ = hc.run_glue(be, c, packed_text)
    hc.check_routes(names, *hc.glue_shapes(c), what)
    show(what, hc.glue_ref(c), hc.anchor(got, hc.glue_ref(c), what))
    glue_results[(c.id, packed_text)] = got
    other = glue_results.get((c.id, not packed_text))
    if other is not None:                                  # reported, not required
        same = all(torch.equal(got[n], other[n]) for n in hc.GLUE_NAMES)
        print(f"HEAD glue {c.id}: packed_text and the padded path bit-equal: {same}")


@pytest.mark.parametrize("packed_text", [False, True], ids=["padded", "packed_text"])
def test_glue_row_independence_of_the_padding(be, packed_text):
    hc.check_row_independence(be, hc.GLUE_BY_ID["counts_3_1_0_2"], packed_text)


def test_trainer_filter_on_the_device(be):
    clip_sd, cm_sd = hc.glue_weights()
    hc.check_trainer_filter(be.teacher(hc.glue_cfg(), clip_sd, cm_sd, False))
