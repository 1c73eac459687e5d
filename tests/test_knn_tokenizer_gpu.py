"""The KNN / projection tokenizer on the GPU (dclip_amd/knn_tokenizer.py): the projection MLP against fp64,
`knn_or_projection` on a 129-entry codebook, a tiny-tower teacher built with and without the three paths, and
`eval.retrieve_topk` against `ops.rank_count`."""
import json

import pytest
import torch

from dclip_amd import config as dcfg, eval as deval, knn_tokenizer as ktok, ops, synth
from dclip_amd.clip_model import from_hf_state_dict
from dclip_amd.patch_text_aggregation import PatchTextAggregation
from tests import kernel_checks_front as kf
from tests import kernel_checks_topk as kt

pytestmark = pytest.mark.gpu

E, HID, N = 64, 96, 129
U = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def clip(dev):
    cfg = dcfg.tiny(proj=E)
    return from_hf_state_dict(cfg, synth.synth_clip_state_dict(cfg, seed=7, gain=3.0), device=dev)


def unit_rows(n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, E, generator=g)
    return x / x.norm(dim=1, keepdim=True)


def write_files(tmp_path, rows, hidden=HID):
    js = tmp_path / "embeddings.json"
    js.write_text(json.dumps({f"patch{i}": {"embedding": [r.tolist()], "position": [0, 0, 1, 1]} for i, r in enumerate(rows)}))
    torch.manual_seed(5)
    ck = tmp_path / "projection.pt"
    torch.save({"model_state_dict": ktok.ImageProjectionModule(E, hidden).state_dict()}, ck)
    ix = tmp_path / "patches.idx"
    ix.write_bytes(b"not parsed")
    return str(ck), str(ix), str(js)


def mlp_fp64(sd, x, pos):
    """fp64 forward and the §16 GEMM bound (K + 8) 2^-24 (|a| |W|^T + |b|) of every layer, carried through the next layers
    (ReLU does not grow an error)."""
    h = torch.cat([x, pos], 1).double()
    bound = torch.zeros_like(h)
    for i in (0, 2, 4):
        w, b = sd[f"projection.{i}.weight"].double().cpu(), sd[f"projection.{i}.bias"].double().cpu()
        own = (w.shape[1] + 8) * U * ((h.abs() + bound) @ w.abs().t() + b.abs())
        bound = bound @ w.abs().t() + own
        h = h @ w.t() + b
        if i < 4:
            h = torch.relu(h)
    return h, bound


@pytest.mark.parametrize("Q", [1, 5, 65])
def test_projection_module_matches_fp64_inside_the_summed_gemm_bound(dev, Q):
    torch.manual_seed(9)
    module = ktok.ImageProjectionModule().to(dev)                      # the reference's widths: 516 -> 1024 -> 1024 -> 512
    g = torch.Generator().manual_seed(Q)
    x = torch.randn(Q, 512, generator=g)
    x = x / x.norm(dim=1, keepdim=True)
    pos = torch.rand(Q, 4, generator=g)
    got = module(x.to(dev), pos.to(dev)).cpu().double()
    want, bound = mlp_fp64(module.state_dict(), x, pos)
    ratio = float(((got - want).abs() / bound).max())
    print("Q", Q, "worst got / bound", ratio)
    assert got.shape == (Q, 512) and ratio <= 1.0


def test_knn_or_projection_on_a_129_entry_codebook(dev, clip, tmp_path):
    rows = unit_rows(N, 3)
    ck, ix, js = write_files(tmp_path, rows)
    tok = ktok.TokenizerWithKNN(clip, ck, ix, js, similarity_threshold=0.85)
    assert tok.knn_tokenizer.codebook.shape == (N, E) and tok.knn_tokenizer.codebook.is_cuda
    copies = [128, 0, 64, 77, 31]
    far = unit_rows(60, 11)
    queries = torch.cat([2.5 * rows[copies], far]).to(dev)             # 65 queries; the copies are scaled, not bit-equal, on entry
    pos = torch.rand(65, 4, generator=torch.Generator().manual_seed(2)).to(dev)
    out, source, sim = tok.knn_or_projection(queries, pos)
    assert source.cpu().tolist() == [0] * 5 + [1] * 60
    assert torch.equal(out[:5].cpu(), rows[copies]), "a retrieved embedding is the codebook entry, bit for bit"
    assert bool((sim[:5] > 0.9999).all()) and bool((sim[5:] < 0.85).all())
    xn, _ = ops.normalize_rows_fwd(queries)
    want, _ = ops.normalize_rows_fwd(tok.knn_tokenizer.projection_module(xn, pos))
    assert torch.equal(out[5:], want[5:])
    best = (xn.cpu().double() @ rows.double().t()).max(dim=1).values
    assert float((sim.cpu().double() - best).abs().max()) < (E + 8) * U
    plain = ktok.ImageTokenizer(clip, None, ix, js)                    # no projection module: the "clip" branch
    out, source, _ = plain.knn_or_projection(queries)
    assert source.cpu().tolist() == [0] * 5 + [1] * 60 and torch.equal(out[5:], xn[5:]) and torch.equal(out[:5].cpu(), rows[copies])


def teacher_inputs(clip, dev):
    cfg = clip.config
    regions = synth.synth_regions(3, 4, cfg.vision, seed=2).to(dev)
    ids = synth.synth_input_ids(3, cfg.text, seed=3, ragged=True).to(dev)
    counts = torch.tensor([4, 2, 0], dtype=torch.int32)
    return regions, ids, counts


def by_hand(teacher, regions, ids, counts, substitute=None):
    """compute_global_embedding_tensors restated from its parts."""
    B, R = regions.shape[:2]
    with torch.no_grad():
        emb = teacher.patch_tokenizer.encode_regions(regions.reshape(B * R, *regions.shape[2:]))
        if substitute is not None:
            emb = substitute(emb)
        emb = ops.mask_rows(emb.view(B, R, -1).contiguous(), counts.to(emb.device))[:, :max(int(counts.max()), 1)].contiguous()
        sent, tokens, eos = teacher.text_tokenizer.token_level_ids(ids)
        text = ops.pack_tokens(tokens.contiguous(), sent, eos, max(int(eos.max()) - 1, 1))
        return teacher.global_embedding_from_tokens(text, emb)


def test_teacher_with_the_three_paths_substitutes_region_embeddings(dev, clip, tmp_path):
    regions, ids, counts = teacher_inputs(clip, dev)
    with torch.no_grad():
        plain = PatchTextAggregation(embed_dim=E, num_heads=1, clip_model=clip).to(dev)
        emb = plain.patch_tokenizer.encode_regions(regions.reshape(12, *regions.shape[2:]))
        known, _ = ops.normalize_rows_fwd(emb[[0, 3, 5]].contiguous())        # three regions are codebook entries
    rows = torch.cat([unit_rows(N - 3, 3), known.cpu()])
    ck, ix, js = write_files(tmp_path, rows)
    teacher = PatchTextAggregation(embed_dim=E, num_heads=1, similarity_threshold=0.9999, projection_model_path=ck,
                                   faiss_index_path=ix, embeddings_json_path=js, clip_model=clip).to(dev)
    teacher.cross_modal_attention.load_state_dict(synth.synth_cross_modal_state_dict(E, seed=5))
    plain.cross_modal_attention.load_state_dict(synth.synth_cross_modal_state_dict(E, seed=5))
    assert teacher.use_knn_projection and teacher.advanced_tokenizer.knn_tokenizer.codebook.is_cuda
    pos = torch.rand(3, 4, 4, generator=torch.Generator().manual_seed(4)).to(dev)
    with torch.no_grad():
        got = teacher.compute_global_embedding_tensors(regions, ids, counts, region_positions=pos)
    sources = []

    def substitute(e):
        out, source, sim = teacher.advanced_tokenizer.knn_or_projection(e, pos.reshape(12, 4))
        sources.append(source.cpu().tolist())
        print("similarities", [round(v, 5) for v in sim.cpu().tolist()], "sources", sources[0])
        return out

    want = by_hand(teacher, regions, ids, counts, substitute)
    assert torch.equal(got, want) and bool(torch.isfinite(got).all())
    assert [sources[0][i] for i in (0, 3, 5)] == [0, 0, 0] and 1 in sources[0]
    # with the paths empty the branch is not entered: the output is the one its parts give without the tokenizer
    with torch.no_grad():
        off = plain.compute_global_embedding_tensors(regions, ids, counts)
    assert plain.advanced_tokenizer is None and torch.equal(off, by_hand(plain, regions, ids, counts))
    assert not torch.equal(off, got)


def test_retrieve_topk_agrees_with_rank_count_on_determined_rows(dev):
    Q, G, P, k = 130, 1001, 36, 10
    s = kf.build_rank_gauss(Q, G, P)
    q, g = torch.from_numpy(s["q"]).to(dev), torch.from_numpy(s["cand"]).to(dev)
    gt = torch.from_numpy(s["gt"]).to(dev)
    gt[:20] = torch.arange(20, dtype=torch.int32, device=dev)          # make some ground truths easy: q_i close to g_i
    q[:20] = g[:20] + 0.05 * q[:20]
    scores, indices = deval.retrieve_topk(q, g, k)
    z_scores, z_indices = deval.zero_shot_topk(q, g, 5)
    assert torch.equal(z_indices, indices[:, :5]) and torch.equal(z_scores, scores[:, :5])
    qn, gn = deval._normalised(q), deval._normalised(g)
    rank = ops.rank_count(qn, gn, ops.rowdot_gather(qn, gn, gt), gt).cpu().numpy()
    ref = kt.gauss_reference(qn.cpu().numpy(), gn.cpu().numpy(), k)
    undetermined = kt.check_topk_gauss(scores.cpu().numpy(), indices.cpu().numpy(), ref, k, "retrieve_topk")
    inside = (indices.cpu() == gt.cpu()[:, None]).any(dim=1).numpy()
    det = ref["determined"]
    print("undetermined rows", undetermined, "of", Q, " ground truth retrieved on", int(inside.sum()), "rows")
    assert inside[:20].all() and (inside[det] == (rank[det] < k)).all() and undetermined <= 0.05 * Q
