"""The full-resolution meta-teacher at a c3-shaped batch: the per-crop path (one tower forward per crop size, crops cut by
Pillow on the host) against the packed path (one tower pass, crops cut on the device), in one process.

A seeded batch of synthetic photos (about 480 x 640) with boxes whose sides are drawn from 32 .. 320 px, the ViT-B/32 teacher
(random weights) in fp32 and in bf16.  Both paths get the batch as data.GpuCollate hands it over (images_u8 / dims on the
device).  After one warm-up call of each, the two paths alternate; every timed window is one teacher call and ends in a
device synchronise.  Prints ms per teacher call (each pair, then median and spread), the launches of one call of each path
and the largest relative difference of the two targets.  --attn16 adds, for bf16 and fp16, the leg "packed + 16-bit core" (the
packed pass with HipCLIPModel.packed_attention16 on), which alternates with the other two under the same protocol.

usage: python tools/fullres_teacher_bench.py [--images 64] [--boxes 8] [--pairs 3] [--precisions fp32 bf16] [--attn16]
       [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from dclip_amd import _lib, config as dcfg, synth  # noqa: E402
from dclip_amd.clip_model import from_hf_state_dict  # noqa: E402
from dclip_amd.patch_text_aggregation import PatchTextAggregation  # noqa: E402


def make_batch(n_images: int, n_boxes: int, seed: int):
    """(HWC uint8 arrays, per-image [((x1, y1, x2, y2), confidence)]): sides 32 .. 320 px, every box inside its image."""
    rng = np.random.default_rng(seed)
    images, boxes = [], []
    for i in range(n_images):
        h, w = 480 + int(rng.integers(-16, 17)), 640 + int(rng.integers(-16, 17))
        images.append(synth.synth_photo(h, w, seed=seed + i))
        bx = []
        for _ in range(n_boxes):
            bw, bh = int(rng.integers(32, 321)), int(rng.integers(32, 321))
            x1, y1 = int(rng.integers(0, w - bw + 1)), int(rng.integers(0, h - bh + 1))
            bx.append(((x1, y1, x1 + bw, y1 + bh), float(rng.uniform(0.3, 1.0))))
        boxes.append(bx)
    return images, boxes


def count_launches(fn):
    lib, check, n = _lib.load(), _lib.check, [0]
    sites = set()

    def census(rc, what=""):
        n[0] += 1
        sites.add(lib.dclip_last_launch().decode().split(".")[0])
        return check(rc, what)

    _lib.check = census
    try:
        out = fn()
    finally:
        _lib.check = check
    return out, n[0], sorted(sites)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--boxes", type=int, default=8)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--precisions", nargs="+", default=["fp32", "bf16"], choices=["fp32", "bf16", "fp16"])
    ap.add_argument("--attn16", action="store_true",
                    help="bf16 / fp16: add the leg `packed + 16-bit core` (HipCLIPModel.packed_attention16), alternating with the others")
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = torch.device("cuda:0")
    cfg = dcfg.vit_b32()
    clip = from_hf_state_dict(cfg, synth.synth_clip_state_dict(cfg, seed=0, gain=3.0), device=dev)
    images, boxes = make_batch(args.images, args.boxes, args.seed)
    ids = synth.synth_input_ids(args.images, cfg.text, seed=args.seed + 1, ragged=True, min_len=4).to(dev)
    paths = [f"synthetic{i}" for i in range(args.images)]
    result = {"images": args.images, "boxes_per_image": args.boxes, "pairs": args.pairs, "tower": cfg.name}
    for prec in args.precisions:
        teacher = PatchTextAggregation(embed_dim=cfg.projection_dim, num_heads=cfg.projection_dim // 64, clip_model=clip,
                                       tower_precision=prec).to(dev)
        teacher.full_resolution = True
        u8, dims = teacher.patch_tokenizer._upload_u8(images)
        plan = teacher.patch_tokenizer.plan_full_resolution(boxes, cfg.vision.patch_size)
        print(f"[{prec}] {args.images} images, {sum(plan['counts'])} crops kept, {int(plan['cu_seqlens'][-1])} packed token rows, "
              f"longest sequence {plan['max_S']}, {len(set(map(tuple, plan['grids'].tolist())))} distinct grids")

        def call(packed: bool, attn16: bool = False):
            teacher.full_resolution_packed = packed
            clip.packed_attention16 = attn16
            with torch.no_grad():
                out = teacher.compute_global_embedding_batch(paths, ids, boxes, images_u8=u8, dims=dims)
            torch.cuda.synchronize()
            return out

        # warm-up of both paths (weight copies, workspaces, code objects), with the launch census and the comparison
        want, n_crop, sites_crop = count_launches(lambda: call(False))
        got, n_pack, sites_pack = count_launches(lambda: call(True))
        diff = float((got - want).abs().max() / want.abs().max())
        cos = float(torch.nn.functional.cosine_similarity(got.double(), want.double(), dim=1).min())
        print(f"[{prec}] launches per teacher call: per-crop {n_crop}, packed {n_pack}")
        print(f"[{prec}] packed-only launch sites: {[s for s in sites_pack if s not in sites_crop]}")
        print(f"[{prec}] largest relative difference of the two targets {diff:.3e}, smallest cosine {cos:.8f}")
        # --attn16 (16-bit precisions): a third leg, the packed pass with the 16-bit packed attention core
        legs = [("per_crop", False, False), ("packed", True, False)]
        if args.attn16 and prec != "fp32":
            legs.append(("packed16", True, True))
            got16, n_pack16, _ = count_launches(lambda: call(True, True))              # its warm-up
            d16 = float((got16 - got).abs().max() / got.abs().max())
            c16 = float(torch.nn.functional.cosine_similarity(got16.double(), got.double(), dim=1).min())
            print(f"[{prec}] packed + 16-bit core: {n_pack16} launches per teacher call; against the packed target: largest relative "
                  f"difference {d16:.3e}, smallest cosine {c16:.8f}")
        ms = {name: [] for name, _, _ in legs}
        for pair in range(args.pairs):
            for name, packed, a16 in legs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call(packed, a16)
                ms[name].append(1e3 * (time.perf_counter() - t0))
            print(f"[{prec}] pair {pair}: " + ", ".join(f"{name} {ms[name][-1]:.1f} ms" for name in ms))
        med = {k: statistics.median(v) for k, v in ms.items()}
        if "packed16" in ms:
            print(f"[{prec}] packed + 16-bit core {med['packed16']:.2f} ms (min {min(ms['packed16']):.2f}, max {max(ms['packed16']):.2f}) "
                  f"against packed {med['packed']:.2f} (min {min(ms['packed']):.2f}, max {max(ms['packed']):.2f}); packed / packed16 "
                  f"{med['packed'] / med['packed16']:.2f}")
        clip.packed_attention16 = None
        print(f"[{prec}] ms per teacher call, median of {args.pairs}: per-crop {med['per_crop']:.1f} "
              f"(min {min(ms['per_crop']):.1f}, max {max(ms['per_crop']):.1f}), packed {med['packed']:.1f} "
              f"(min {min(ms['packed']):.1f}, max {max(ms['packed']):.1f}); ratio {med['per_crop'] / med['packed']:.2f}")
        result[prec] = {"ms": ms, "median_ms": med, "launches": {"per_crop": n_crop, "packed": n_pack},
                        "max_rel_diff": diff, "min_cosine": cos, "crops": sum(plan["counts"]),
                        "token_rows": int(plan["cu_seqlens"][-1]), "max_S": plan["max_S"]}
    print(json.dumps(result))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    return result


if __name__ == "__main__":
    main()
