"""The TRAINABLE fp32 text tower on the split-fp16 plan (`text_train_split16`) against the plain fp32 GEMMs, in one
process, alternating.  Three measurements:

  tower   ViT-B/32 text tower, random weights, every text parameter trainable, B = --batch: one call = get_text_features under
          grad plus the backward of a fixed weighting.  Four legs — padded plain (the tower as it runs without the switch),
          padded split, packed plain (`packed_train`, §29), packed split — on two sets of ids, those of
          tools/packed_text_train_bench.py: seeded ragged lengths from a clipped normal (an ASSUMPTION about caption lengths,
          not a dataset statistic) and every caption 77 tokens long.  Also lists the launch names the split legs' GEMMs land on.
  attn    the attention backward plus the split of dqkv at B = --batch, S = 77, H = 8, causal: attention_bwd.rows and the
          three-launch split against attention_bwd.rows.stats and the single pass.
  step    one as_written training_step (vision projections and the whole text tower train; teacher image embedding given) plus
          its backward, `text_train_split16` off against on.

Every leg is warmed once; then the legs alternate for --pairs rounds, a timed window is --calls calls and ends in a device
synchronise.  Prints ms per call as median (min … max) per leg, and one JSON line.

usage: python tools/text_train_split16_bench.py [--what tower attn step] [--batch 256] [--pairs 5] [--calls 5] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from dclip_amd import config as dcfg, synth  # noqa: E402
from dclip_amd.clip_model import from_hf_state_dict, packed_text_tables  # noqa: E402
from tools.packed_text_bench import ragged_ids  # noqa: E402


def alternate(legs, pairs, calls, tag):
    """legs: {name: fn(n)} (fn runs n calls and synchronises) -> {name: [ms per call, one per round]}"""
    for fn in legs.values():
        fn(1)
    ms = {k: [] for k in legs}
    for r in range(pairs):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(calls)
            ms[k].append(1e3 * (time.perf_counter() - t0) / calls)
        print(f"[{tag}] round {r}: " + ", ".join(f"{k} {v[-1]:.3f} ms" for k, v in ms.items()))
    for k, v in ms.items():
        print(f"[{tag}] {k}: median of {pairs} {statistics.median(v):.3f} ms (min {min(v):.3f} … max {max(v):.3f})")
    return ms


def launch_names(fn):
    from dclip_amd import _lib
    lib, real, names = _lib.load(), _lib.check, []

    def spy(rc, what=""):
        names.append(lib.dclip_last_launch().decode())
        return real(rc, what)
    _lib.check = spy
    try:
        fn()
    finally:
        _lib.check = real
    return names


def bench_tower(args, dev, result):
    cfg = dcfg.vit_b32()
    clip = from_hf_state_dict(cfg, synth.synth_clip_state_dict(cfg, seed=0, gain=3.0), device=dev)
    clip.requires_grad_(False)
    params = dict(zip(clip.text_params().names(), clip.text_params().tensors()))
    for p in params.values():
        p.requires_grad_(True)
    W = torch.randn((args.batch, cfg.projection_dim), generator=torch.Generator().manual_seed(11)).to(dev)
    sets = {"ragged": ragged_ids(args.batch, cfg.text, args.mean, args.sd, args.longest, args.seed),
            "all77": synth.synth_input_ids(args.batch, cfg.text, seed=args.seed + 1, ragged=False)}
    print(f"caption lengths of the ragged set: clipped normal(mean {args.mean}, sd {args.sd}) in [3, {args.longest}], seed {args.seed} "
          "— an assumption, not a dataset statistic")
    for name, ids in sets.items():
        t = packed_text_tables(ids, cfg.text.eos_token_id)
        lens, idd = t["lens"], ids.to(dev)
        print(f"[{name}] B {ids.shape[0]}, Tmax {ids.shape[1]} ({ids.shape[0] * ids.shape[1]} padded rows), Tp {t['Tp']} packed rows")

        def call(packed, split, n=1):
            clip.text_train_split16 = split
            for _ in range(n):
                for p in params.values():
                    p.grad = None
                kw = {"packed_lens": lens, "packed_train": True} if packed else {}
                out = clip.get_text_features(input_ids=idd, **kw)
                (out * W).sum().backward()
            torch.cuda.synchronize()
            return out.detach(), {k: p.grad.detach().clone() for k, p in params.items()}

        legs = {"padded plain": (False, False), "padded split": (False, True), "packed plain": (True, False),
                "packed split": (True, True)}
        ref = {k: call(*v) for k, v in legs.items()}
        rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())      # noqa: E731
        diffs = {}
        for packed in ("padded", "packed"):
            (o1, g1), (o0, g0) = ref[packed + " split"], ref[packed + " plain"]
            worst = max(g0, key=lambda k: rel(g1[k], g0[k]))
            diffs[packed] = {"out": rel(o1, o0), "grad": rel(g1[worst], g0[worst]), "grad_tensor": worst}
            print(f"[{name}] {packed} split against plain, norm-wise: output {diffs[packed]['out']:.3e}, worst gradient "
                  f"{diffs[packed]['grad']:.3e} ({worst})")
        del ref
        lands = {}
        for packed in (False, True):
            names = launch_names(lambda: call(packed, True))
            lands["packed" if packed else "padded"] = sorted({n for n in names if n.startswith("gemm_f") or "attention" in n})
            print(f"[{name}] {'packed' if packed else 'padded'} split lands on: " + ", ".join(lands["packed" if packed else "padded"]))
        ms = alternate({k: (lambda n, v=v: call(*v, n=n)) for k, v in legs.items()}, args.pairs, args.calls, name)
        result["tower_" + name] = {"Tmax": ids.shape[1], "Tp": t["Tp"], "ms": ms, "median_ms": {k: statistics.median(v) for k, v in ms.items()},
                                   "diff": diffs, "lands_on": lands}
    clip.text_train_split16 = False


def bench_attn(args, dev, result):
    from dclip_amd import ops
    B, S, H = args.batch, 77, 8
    D = H * 64
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn((B * S, 3 * D), generator=g).to(dev)
    dout = torch.randn((B * S, D), generator=g).to(dev)
    out, lse = ops.attention_fwd(qkv, B, S, H, True)
    db = torch.empty((3 * D,), device=dev)
    P = ops.attention_bwd_rows_stats_plan(B, S, H)

    def three(n):
        for _ in range(n):
            d = ops.attention_bwd(qkv, out, dout, lse, B, S, H, True)
            r = ops.split_f16x3_rows_colstats(d, db=db, pieces=args.pieces)
        torch.cuda.synchronize()
        return d, r

    def single(n):
        for _ in range(n):
            st = ops.ColStats(P, 3 * D, dev)
            d = ops.attention_bwd(qkv, out, dout, lse, B, S, H, True, rows_stats=st)
            r = ops.split_f16x3_rows_cols_stats(d, st, db=db, pieces=args.pieces)
        torch.cuda.synchronize()
        return d, r

    (d0, r0), (d1, r1) = three(1), single(1)
    same = torch.equal(d0, d1) and all(torch.equal(a.view(torch.int16) if a.dtype == torch.float16 else a,
                                                   b.view(torch.int16) if b.dtype == torch.float16 else b) for a, b in zip(r0, r1))
    print(f"[attn] B {B} S {S} H {H} causal, pieces {args.pieces}: outputs of the two forms bit-equal: {same}")
    ms = alternate({"rows + three-launch split": three, "rows.stats + single pass": single}, args.pairs, 10 * args.calls, "attn")
    result["attn"] = {"B": B, "S": S, "H": H, "ms": ms, "median_ms": {k: statistics.median(v) for k, v in ms.items()}, "bit_equal": same}


def bench_step(args, dev, result):
    from dclip_amd.CLIP_image_distillation import CLIPImageDistillation
    from dclip_amd.patch_text_aggregation import PatchTextAggregation
    cfg = dcfg.vit_b32()
    B = args.batch
    student = from_hf_state_dict(cfg, synth.synth_clip_state_dict(cfg, seed=0), device=dev)
    teacher = PatchTextAggregation(embed_dim=cfg.projection_dim, num_heads=cfg.projection_dim // 64, clip_model=student).to(dev)
    teacher.cross_modal_attention.load_state_dict(
        {k: v.to(dev) for k, v in synth.synth_cross_modal_state_dict(teacher.embed_dim, seed=31).items()})
    hp = argparse.Namespace(learning_rate=1e-6, warmup_steps=0, total_steps=10 ** 6, train_batch_size=B, eval_batch_size=B)
    module = CLIPImageDistillation(hp, student, None, teacher=teacher, freeze_mode="as_written").to(dev)
    batch = {"pixel_values": synth.synth_pixel_values(B, cfg.vision, seed=0).to(dev),
             "input_ids": synth.synth_input_ids(B, cfg.text, seed=100).to(dev),
             "teacher_image_emb": synth.synth_embeddings(B, cfg.projection_dim, seed=1000).to(dev),
             "teacher_text_emb": synth.synth_embeddings(B, cfg.projection_dim, seed=1001).to(dev)}
    losses = {}

    def step(split, n):
        module.text_train_split16 = split
        for _ in range(n):
            for p in module.parameters():
                p.grad = None
            loss = module.training_step(batch)
            loss.backward()
        torch.cuda.synchronize()
        losses[split] = float(loss.detach())

    ms = alternate({"as_written plain": lambda n: step(False, n), "as_written split": lambda n: step(True, n)}, args.pairs, args.calls,
                   "step")
    print(f"[step] as_written, B {B}, captions 77 tokens: loss plain {losses[False]:.8f}, split {losses[True]:.8f}")
    result["step"] = {"B": B, "ms": ms, "median_ms": {k: statistics.median(v) for k, v in ms.items()},
                      "loss": {"plain": losses[False], "split": losses[True]}}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", nargs="+", default=["tower", "attn", "step"], choices=["tower", "attn", "step"])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--mean", type=float, default=20.0, help="mean caption length in tokens, BOS and EOS included (an assumption)")
    ap.add_argument("--sd", type=float, default=8.0)
    ap.add_argument("--max", type=int, default=77, dest="longest")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5, help="calls per timed window")
    ap.add_argument("--pieces", type=int, default=2, choices=[2, 3], help="attn: pieces of the row split (2 at the flagship shapes)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = torch.device("cuda:0")
    result = {"batch": args.batch, "pairs": args.pairs, "calls": args.calls}
    for what in args.what:
        {"tower": bench_tower, "attn": bench_attn, "step": bench_step}[what](args, dev, result)
    print(json.dumps(result))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    return result


if __name__ == "__main__":
    main()
