"""Frozen towers in fp32 / bf16 / fp16: time and error, in one process, interleaved.

  towers  c3's region encoder (ViT-B/32 x 2048 crops), c5's (ViT-L/14 x 512 crops), the text tower at 256 x 77: per round
          every precision runs once (fp32, bf16, fp16, ...), the median over rounds is reported with the max relative error
          (max|a - b| / max|a|) and min cosine of the 16-bit embeddings against the fp32 ones.
  steps   the c3 and c5 steps of bench.build_workload (student bf16, the teacher's towers bf16 vs fp16; fwd + bwd + AdamW,
          eager, no teacher prefetch), interleaved likewise, with the relative error of the first step's loss against the same
          step with fp32 towers.

usage: python tools/fp16_tower_bench.py [--rounds 5] [--steps 3] [--skip-steps] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from dclip_amd import config as dcfg, synth  # noqa: E402
from dclip_amd.clip_model import from_hf_state_dict  # noqa: E402

PRECS = ("fp32", "bf16", "fp16")


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


def towers(dev, rounds):
    out = []
    cases = [("c3 region encoder ViT-B/32 x 2048", dcfg.vit_b32, "image", 2048),
             ("c5 region encoder ViT-L/14 x 512", dcfg.vit_l14, "image", 512),
             ("text tower ViT-B/32 256 x 77", dcfg.vit_b32, "text", 256)]
    for name, mk, kind, B in cases:
        cfg = mk()
        m = from_hf_state_dict(cfg, synth.synth_clip_state_dict(cfg, seed=7, device=dev), device=dev)
        m.requires_grad_(False)
        if kind == "image":
            x = synth.synth_regions(B // 8, 8, cfg.vision, seed=2).reshape(B, 3, cfg.vision.image_size, -1).to(dev)
            fns = {p: (lambda p=p: m.get_image_features(pixel_values=x, precision=p)) for p in PRECS}
        else:
            x = synth.synth_input_ids(B, cfg.text, seed=3).to(dev)
            fns = {p: (lambda p=p: m.get_text_features(input_ids=x, precision=p)) for p in PRECS}
        with torch.no_grad():
            res = {p: fns[p]() for p in PRECS}                 # warm-up (weight casts) and the outputs compared
            times = {p: [] for p in PRECS}
            for _ in range(rounds):
                for p in PRECS:
                    times[p].append(event_ms(fns[p], 3))
        row = {"case": name}
        for p in PRECS:
            row[p + "_ms"] = statistics.median(times[p])
            if p != "fp32":
                row[p + "_max_rel"], row[p + "_min_cos"] = errors(res["fp32"], res[p])
        row["fp16_vs_bf16"] = row["fp16_ms"] / row["bf16_ms"]
        print(f"{name}: fp32 {row['fp32_ms']:.2f} ms | bf16 {row['bf16_ms']:.2f} ms (max rel {row['bf16_max_rel']:.2e}, "
              f"cos {row['bf16_min_cos']:.6f}) | fp16 {row['fp16_ms']:.2f} ms (max rel {row['fp16_max_rel']:.2e}, "
              f"cos {row['fp16_min_cos']:.6f}) | fp16/bf16 {row['fp16_vs_bf16']:.3f}", flush=True)
        out.append(row)
        del m, res
        torch.cuda.empty_cache()
    return out


def steps(dev, rounds, n):
    import bench
    from dclip_amd import optim
    out = []
    for which, spec in (("c3", ("c3", "ViT-B/32", "ViT-B/32", 256, 8, "bf16")),
                        ("c5", ("c5", "ViT-B/32", "ViT-L/14", 512, 8, "bf16"))):
        runs, loss0 = {}, {}
        for tp in PRECS:
            module, _, _, batch = bench.build_workload(*spec, tp, dev, None, 0, fast_teacher_init=True)
            opt = optim.FusedAdamW([p for p in module.parameters() if p.requires_grad], lr=1e-6, max_grad_norm=0.5)

            def one(module=module, batch=batch, opt=opt):
                loss = module.training_step(batch)
                loss.backward()
                opt.step()
                opt.zero_grad(set_to_none=True)
                return loss.detach()
            loss0[tp] = float(one())                        # same seeds and weights: first-step losses are comparable
            if tp == "fp32":
                del module, batch, opt
                torch.cuda.empty_cache()
                continue
            one()
            runs[tp] = one
        times = {tp: [] for tp in runs}
        for _ in range(rounds):
            for tp in runs:
                times[tp].append(event_ms(runs[tp], n))
        row = {"case": f"{which} step"}
        for tp in runs:
            row[tp + "_ms"] = statistics.median(times[tp])
            row[tp + "_loss_rel"] = abs(loss0[tp] - loss0["fp32"]) / abs(loss0["fp32"])
        row["fp16_vs_bf16"] = row["fp16_ms"] / row["bf16_ms"]
        print(f"{which} step (towers bf16 vs fp16, student bf16): bf16 {row['bf16_ms']:.2f} ms (loss rel {row['bf16_loss_rel']:.2e}) | "
              f"fp16 {row['fp16_ms']:.2f} ms (loss rel {row['fp16_loss_rel']:.2e}) | fp16/bf16 {row['fp16_vs_bf16']:.3f}",
              flush=True)
        out.append(row)
        del runs
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3, help="steps per timed sample of the c3 / c5 step")
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = towers(dev, args.rounds)
    if not args.skip_steps:
        rows += steps(dev, args.rounds, args.steps)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        json.dump(rows, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
