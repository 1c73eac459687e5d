"""The frozen ViT-B/32 vision tower at precision "fp32" / "fp32-split16" / "fp16" (DESIGN.md §28): time and error, in one
process, interleaved.  Three workloads:

  dense    get_image_features on 2048 x 50 tokens (c3's region batch: 256 images x 8 crops, 102 400 rows)
  packed   get_image_features_crops on 64 images x 8 boxes, every crop at its own size
  teacher  PatchTextAggregation.compute_global_embedding_tensors at 64 captions x 8 regions (region tower + token-level text
           pass + the cross-modal block)

Per round every path runs once, in the order fp32, fp32-split16, split16_pass, fp16; `split16_pass` is "fp32-split16" with the
attention context written as fp32 and split by the stand-alone pass (engine._SPLIT16_ATTN_EPI off: the A/B of §28, bit-identical
results).  Each figure is HIP-event time over `--iters` calls after a warm-up of every path; every round is printed, then the
median over rounds with the norm-wise error max|a - b| / max|b| and the minimum cosine against the fp32 path on the same weights.

usage: python tools/frozen_vision_split16_bench.py [--rounds 5] [--iters 2] [--only dense,packed,teacher] [--log out.log]
"""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from dclip_amd import config as dcfg, engine, synth  # noqa: E402
from dclip_amd.clip_model import from_hf_state_dict  # noqa: E402
from dclip_amd.patch_text_aggregation import PatchTextAggregation  # noqa: E402

P = "fp32-split16"
PATHS = ("fp32", P, "split16_pass", "fp16")


def event_ms(fn, n):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def errors(ref, got):
    rel = float((got.float() - ref).abs().max() / ref.abs().max())
    cos = float(torch.nn.functional.cosine_similarity(got.float(), ref, dim=1).min())
    return rel, cos


def with_attn_epi(on, fn):
    def run():
        keep = engine._SPLIT16_ATTN_EPI
        engine._SPLIT16_ATTN_EPI = on
        try:
            return fn()
        finally:
            engine._SPLIT16_ATTN_EPI = keep
    return run


def crop_boxes(n_images, per_image, side, patch, seed):
    """`per_image` boxes in each of `n_images` side x side images: widths and heights of 1 .. side // patch patches."""
    g = torch.Generator().manual_seed(seed)
    boxes = []
    for b in range(n_images):
        for _ in range(per_image):
            gw, gh = (int(torch.randint(1, side // patch + 1, (1,), generator=g)) for _ in range(2))
            x1 = int(torch.randint(0, side - gw * patch + 1, (1,), generator=g))
            y1 = int(torch.randint(0, side - gh * patch + 1, (1,), generator=g))
            boxes.append((b, x1, y1, x1 + gw * patch, y1 + gh * patch))
    return boxes


def workloads(m, cfg, dev, only):
    """{name: (description, {path: callable returning [rows, P] features})}"""
    v = cfg.vision
    out = {}
    if "dense" in only:
        pix = torch.rand((2048, 3, v.image_size, v.image_size), device=dev, generator=torch.Generator(device=dev).manual_seed(2))
        f = lambda prec: (lambda: m.get_image_features(pixel_values=pix, precision=prec))          # noqa: E731
        out["dense"] = (f"dense tower ViT-B/32, {pix.shape[0]} x {v.seq_len} tokens",
                        {"fp32": f("fp32"), P: with_attn_epi(True, f(P)), "split16_pass": with_attn_epi(False, f(P)), "fp16": f("fp16")})
    if "packed" in only:
        side = 448
        u8 = torch.randint(0, 256, (64, side, side, 3), generator=torch.Generator().manual_seed(4), dtype=torch.uint8).to(dev)
        dims = torch.tensor([[side, side]] * 64, dtype=torch.int32, device=dev)
        boxes = crop_boxes(64, 8, side, v.patch_size, 6)
        rows = sum(1 + ((b[4] - b[2]) // v.patch_size) * ((b[3] - b[1]) // v.patch_size) for b in boxes)
        f = lambda prec: (lambda: m.get_image_features_crops(u8, dims, boxes, precision=prec))      # noqa: E731
        out["packed"] = (f"packed tower ViT-B/32, 64 images x 8 boxes, {rows} token rows",
                         {"fp32": f("fp32"), P: with_attn_epi(True, f(P)), "split16_pass": with_attn_epi(False, f(P)), "fp16": f("fp16")})
    if "teacher" in only:
        E = cfg.projection_dim
        regions = torch.rand((64, 8, 3, v.image_size, v.image_size), device=dev, generator=torch.Generator(device=dev).manual_seed(2))
        ids = synth.synth_input_ids(64, cfg.text, seed=3, ragged=True).to(dev)
        counts = torch.full((64,), 8, dtype=torch.int32)
        teachers = {}
        for prec in ("fp32", P, "fp16"):
            t = PatchTextAggregation(embed_dim=E, num_heads=E // 64, clip_model=m, tower_precision=prec).to(dev)
            t.cross_modal_attention.load_state_dict(synth.synth_cross_modal_state_dict(E, seed=5))
            teachers[prec] = t
        f = lambda prec: (lambda: teachers[prec].compute_global_embedding_tensors(regions, ids, counts))   # noqa: E731
        out["teacher"] = ("teacher call, 64 captions x 8 regions (ViT-B/32 towers)",
                          {"fp32": f("fp32"), P: with_attn_epi(True, f(P)), "split16_pass": with_attn_epi(False, f(P)), "fp16": f("fp16")})
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--only", default="dense,packed,teacher")
    ap.add_argument("--gain", type=float, default=1.0)
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this tool measures on the GPU: none found")
    dev = torch.device("cuda:0")
    cfg = dcfg.vit_b32()
    m = from_hf_state_dict(cfg, synth.synth_clip_state_dict(cfg, seed=7, gain=args.gain, device=dev), device=dev)
    m.requires_grad_(False)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    with torch.no_grad():
        for name, (what, fns) in workloads(m, cfg, dev, args.only.split(",")).items():
            res = {k: fns[k]() for k in PATHS}                  # warm-up (weight copies, plans) and the outputs compared
            plan = m._vsplit16_frozen_cache().get("__split16__")
            if plan is None or plan["layers"] is None:
                raise SystemExit("the guard sent the split path to fp32: nothing to measure")
            if not torch.equal(res[P], res["split16_pass"]):
                raise SystemExit(f"{name}: the two attention forms differ")
            times = {k: [] for k in PATHS}
            for r in range(args.rounds):
                for k in PATHS:
                    times[k].append(event_ms(fns[k], args.iters))
                say(f"{name} round {r}: " + " | ".join(f"{k} {times[k][-1]:.2f} ms" for k in PATHS)
                    + f" | split16 faster than fp32: {times[P][-1] < times['fp32'][-1]}")
            med = {k: statistics.median(times[k]) for k in PATHS}
            err = {k: errors(res["fp32"], res[k]) for k in PATHS if k != "fp32"}
            say(f"{what}: median of {args.rounds} rounds: fp32 {med['fp32']:.2f} ms | {P} {med[P]:.2f} ms (err {err[P][0]:.2e}, cos "
                f"{err[P][1]:.7f}) | with the stand-alone split pass {med['split16_pass']:.2f} ms | fp16 {med['fp16']:.2f} ms (err "
                f"{err['fp16'][0]:.2e}, cos {err['fp16'][1]:.7f}) | fp32/{P} {med['fp32'] / med[P]:.2f}x | pass/epilogue "
                f"{med['split16_pass'] / med[P]:.3f}x | faster than fp32 in {sum(a < b for a, b in zip(times[P], times['fp32']))} of "
                f"{args.rounds} rounds")
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
