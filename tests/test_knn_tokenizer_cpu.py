"""CPU-only host logic of the KNN / projection tokenizer (dclip_amd/knn_tokenizer.py): the codebook JSON in both layouts
that training/compute_faiss.py writes, both checkpoint forms, the reference's existence checks, the teacher's constructor
with the three paths, and `knn_or_projection` against a plain-torch stand-in of the ops it calls (kernel parity is
tests/test_topk_paths_gpu.py and tests/test_knn_tokenizer_gpu.py)."""
import json
from types import SimpleNamespace

import pytest
import torch

import tests.cpu_ops_shim as shim
from dclip_amd import config as dcfg, knn_tokenizer as kt, synth
from dclip_amd.clip_model import from_hf_state_dict
from dclip_amd.patch_text_aggregation import PatchTextAggregation

E, HID, N = 64, 32, 9


def _gemm(a, b, layout, bias=None):
    assert layout == 3
    return torch.nn.functional.linear(a, b, bias)


def _topk_ip(q, db, k):
    s = q @ db.t()
    order = torch.stack([torch.tensor(sorted(range(db.shape[0]), key=lambda j: (-float(r[j]), j))[:k]) for r in s])
    return torch.gather(s, 1, order), order.to(torch.int32)


def _knn_select(sim, idx, db, fb, thresh):
    hit = (idx >= 0) & (sim >= thresh)
    return torch.where(hit[:, None], db[idx.long().clamp_min(0)], fb), (~hit).to(torch.int32)


OPS = SimpleNamespace(normalize_rows_fwd=shim.normalize_rows_fwd, gemm=_gemm, relu_=lambda x: x.clamp_(min=0), topk_ip=_topk_ip,
                      knn_select=_knn_select, LAYOUT_NT=3)


@pytest.fixture
def stand_in(monkeypatch):
    monkeypatch.setattr(kt, "ops", OPS)


@pytest.fixture(scope="module")
def clip():
    cfg = dcfg.tiny(proj=E)
    return from_hf_state_dict(cfg, synth.synth_clip_state_dict(cfg, seed=7))


def codebook_rows():
    g = torch.Generator().manual_seed(3)
    rows = torch.randn(N, E, generator=g)
    return rows / rows.norm(dim=1, keepdim=True)


def write_files(tmp_path, layout="list", checkpoint="plain", idx=True):
    rows = codebook_rows()
    ids = [f"img{(7 * i) % N}.jpg_patch{i}" for i in range(N)]           # not sorted: file order is what counts
    if layout == "list":
        entries = {k: r.tolist() for k, r in zip(ids, rows)}
    elif layout == "nested":
        entries = {k: [r.tolist()] for k, r in zip(ids, rows)}          # [1, E], as embedding.tolist() of a [1, E] array
    else:
        entries = {k: {"embedding": [r.tolist()], "position": [0.1, 0.2, 0.3, 0.4]} for k, r in zip(ids, rows)}
    js = tmp_path / "embeddings.json"
    js.write_text(json.dumps(entries))
    torch.manual_seed(5)
    module = kt.ImageProjectionModule(E, HID)
    sd = {k: v.clone() for k, v in module.state_dict().items()}
    ck = tmp_path / "projection.pt"
    torch.save(sd if checkpoint == "plain" else {"epoch": 3, "model_state_dict": sd, "loss": 0.5}, ck)
    ix = tmp_path / "patches.idx"
    if idx:
        ix.write_bytes(b"not parsed")
    return str(ck), str(ix), str(js), ids, rows, sd


@pytest.mark.parametrize("layout", ["list", "nested", "dict"])
def test_codebook_json_loads_in_every_layout_in_file_order(tmp_path, layout):
    _, _, js, ids, rows, _ = write_files(tmp_path, layout)
    got_ids, got = kt.load_codebook(js)
    assert got_ids == ids
    assert got.dtype == torch.float32 and got.shape == (N, E) and torch.equal(got, rows)


def test_projection_module_has_the_reference_keys_and_shapes():
    sd = kt.ImageProjectionModule().state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == {
        "projection.0.weight": (1024, 516), "projection.0.bias": (1024,), "projection.2.weight": (1024, 1024),
        "projection.2.bias": (1024,), "projection.4.weight": (512, 1024), "projection.4.bias": (512,)}
    reference = torch.nn.Sequential(torch.nn.Linear(516, 1024), torch.nn.ReLU(), torch.nn.Linear(1024, 1024), torch.nn.ReLU(),
                                    torch.nn.Linear(1024, 512))
    assert list(sd) == ["projection." + k for k in reference.state_dict()]
    assert not any(p.requires_grad for p in kt.ImageProjectionModule(8, 4).parameters())


@pytest.mark.parametrize("checkpoint", ["plain", "full"])
def test_both_checkpoint_forms_load(tmp_path, checkpoint):
    ck, _, _, _, _, sd = write_files(tmp_path, checkpoint=checkpoint)
    module = kt.ImageProjectionModule.from_checkpoint(ck)
    assert (module.clip_dim, module.hidden_dim) == (E, HID) and not module.training
    for k, v in module.state_dict().items():
        assert torch.equal(v, sd[k]), k


def test_a_missing_index_file_disables_knn_and_does_not_raise(tmp_path, clip, stand_in):
    ck, ix, js, _, rows, _ = write_files(tmp_path, idx=False)
    tok = kt.ImageTokenizer(clip, ck, ix, js)
    assert not tok.use_knn and tok.codebook is None and tok.projection_module is not None
    out, source, sim = tok.knn_or_projection(rows[:3].clone())
    assert source.tolist() == [1, 1, 1] and bool(torch.isinf(sim).all())
    want = torch.nn.functional.normalize(tok.projection_module(rows[:3], torch.zeros(3, 4)), dim=1)
    assert torch.allclose(out, want, atol=1e-6)


def test_the_teacher_constructor_takes_the_three_paths(tmp_path, clip):
    """Raised NotImplementedError before the KNN tokenizer existed."""
    ck, ix, js, ids, rows, _ = write_files(tmp_path, "dict", "full")
    teacher = PatchTextAggregation(embed_dim=E, num_heads=1, similarity_threshold=0.9, projection_model_path=ck,
                                   faiss_index_path=ix, embeddings_json_path=js, clip_model=clip)
    assert teacher.use_knn_projection and type(teacher.advanced_tokenizer).__name__ == "TokenizerWithKNN"
    tok = teacher.advanced_tokenizer.knn_tokenizer
    assert tok.use_knn and tok.patch_ids == ids and torch.equal(tok.codebook, rows) and tok.similarity_threshold == 0.9
    assert sorted(teacher.state_dict()) == sorted("cross_modal_attention." + k for k in teacher.cross_modal_attention.state_dict())
    assert teacher.load_caches("nowhere.pkl") is teacher and teacher.knn_cache == {}


def test_empty_paths_leave_the_tokenizer_off(clip):
    teacher = PatchTextAggregation(embed_dim=E, num_heads=1, clip_model=clip, projection_model_path="", faiss_index_path=None)
    assert teacher.use_knn_projection is False and teacher.advanced_tokenizer is None


def test_knn_or_projection_host_logic_against_the_stand_in(tmp_path, clip, stand_in):
    ck, ix, js, _, rows, _ = write_files(tmp_path)
    tok = kt.TokenizerWithKNN(clip, ck, ix, js, similarity_threshold=0.85)
    g = torch.Generator().manual_seed(11)
    far = torch.randn(4, E, generator=g)
    queries = torch.cat([3.0 * rows[[4, 0]], far])                     # scaled copies: the search sees them normalised
    pos = torch.rand(6, 4, generator=g)
    out, source, sim = tok.knn_or_projection(queries, pos)
    assert source.tolist() == [0, 0, 1, 1, 1, 1]
    assert torch.equal(out[:2], rows[[4, 0]]) and bool((sim[:2] > 0.999).all()) and bool((sim[2:] < 0.85).all())
    module = tok.knn_tokenizer.projection_module
    xn = torch.nn.functional.normalize(far, dim=1)
    sd = module.state_dict()
    h = torch.relu(torch.nn.functional.linear(torch.cat([xn, pos[2:]], 1), sd["projection.0.weight"], sd["projection.0.bias"]))
    h = torch.relu(torch.nn.functional.linear(h, sd["projection.2.weight"], sd["projection.2.bias"]))
    want = torch.nn.functional.normalize(torch.nn.functional.linear(h, sd["projection.4.weight"], sd["projection.4.bias"]), dim=1)
    assert torch.allclose(out[2:], want, atol=1e-6)
    zeros = tok.knn_or_projection(queries, None)[0]                    # None positions are zeros (:298)
    assert torch.equal(zeros, tok.knn_or_projection(queries, torch.zeros(6, 4))[0]) and not torch.equal(zeros[2:], out[2:])
    plain = kt.ImageTokenizer(clip, None, ix, js)                      # no projection module: the "clip" branch
    out, source, _ = plain.knn_or_projection(queries)
    assert source.tolist() == [0, 0, 1, 1, 1, 1] and torch.equal(out[:2], rows[[4, 0]])
    assert torch.allclose(out[2:], xn, atol=1e-7)


def test_the_knn_path_queries_with_processor_crops_and_box_positions(tmp_path, clip):
    """compute_global_embedding_batch's host side with the tokenizer on: each crop goes through the CLIP processor (not
    patch_transform), positions are [x1/w, y1/h, x2/w, y2/h] (training/patch_text_aggregation.py:315), an image with a box
    without extent keeps no region."""
    import numpy as np
    from PIL import Image
    from dclip_amd.data import ClipImagePreprocess
    ck, ix, js, _, _, _ = write_files(tmp_path)
    teacher = PatchTextAggregation(embed_dim=E, num_heads=1, projection_model_path=ck, faiss_index_path=ix,
                                   embeddings_json_path=js, clip_model=clip)
    rng = np.random.default_rng(0)
    images = [Image.fromarray(rng.integers(0, 256, (90, 120, 3), dtype=np.uint8)), Image.fromarray(rng.integers(0, 256, (70, 50, 3), dtype=np.uint8)),
              Image.fromarray(rng.integers(0, 256, (40, 40, 3), dtype=np.uint8))]
    boxes = [[((10, 20, 70, 80), 0.9), ((0, 0, 120, 90), 0.5)], [((5, 5, 45, 65), 0.7)], [((3, 3, 3, 30), 0.4), ((1, 1, 20, 20), 0.3)]]
    regions, counts, positions = teacher._knn_query_crops(images, boxes)
    s = clip.config.vision.image_size
    assert counts.tolist() == [2, 1, 0] and regions.shape == (3, 2, 3, s, s) and positions.shape == (3, 2, 4)
    pre = ClipImagePreprocess(size=s)
    assert torch.equal(regions[0, 0], pre.image(images[0].crop((10, 20, 70, 80)))) and torch.equal(regions[1, 0], pre.image(images[1].crop((5, 5, 45, 65))))
    assert not torch.equal(regions[0, 0], teacher.patch_tokenizer.patch_transform(images[0].crop((10, 20, 70, 80))))
    assert torch.equal(positions[0, 0], torch.tensor([10 / 120, 20 / 90, 70 / 120, 80 / 90])) and torch.equal(positions[0, 1], torch.tensor([0.0, 0.0, 1.0, 1.0]))
    assert torch.equal(positions[1, 0], torch.tensor([5 / 50, 5 / 70, 45 / 50, 65 / 70]))
    assert not regions[1, 1].any() and not regions[2].any() and not positions[2].any()
