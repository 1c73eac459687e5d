"""The fp16 student (student_precision="fp16") against the bf16 one: time and error, in one process, interleaved.

  c3     the c3 step of bench.build_workload (ViT-B/32 student at 256 images, meta-teacher on 8 crops per image): student
         bf16 / fp16 x teacher towers bf16 / fp16; fwd + bwd + optimizer (fp16: scaled loss, DynamicLossScaler.step/update).
  c2     the c2-shaped student step (ViT-B/32 at 256, teacher image embedding given) in bf16 and fp16.
  tail   the optimizer tail alone on ViT-B/32-sized gradients: FusedAdamW.step (clip + AdamW) against the loss-scaled step
         (clip_coef_scaled + the skipping AdamW) and the scale update.
For every step variant the first step's loss and the student's image embedding are compared with the fp32 student on the
same weights and batch (max |a - b| / max |b|).  Per round every variant runs once; the median over rounds is reported.

usage: python tools/fp16_student_bench.py [--rounds 5] [--steps 3] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402


def event_ms(fn, n):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def make_step(workload, student_precision, tower_precision, dev):
    """(one step fn, first-step loss, student image embedding of the batch before any update) for one variant."""
    import bench
    from dclip_amd import optim
    from dclip_amd.amp import DynamicLossScaler
    spec = ("c3", "ViT-B/32", "ViT-B/32", 256, 8) if workload == "c3" else ("c2", "ViT-B/32", None, 256, 8)
    module, _, _, batch = bench.build_workload(*spec, student_precision, tower_precision, dev, None, 0, fast_teacher_init=True)
    img_prec = "fp16-mixed" if student_precision == "fp16" else student_precision
    with torch.no_grad():
        emb = module.student.get_image_features(pixel_values=batch["pixel_values"], precision=img_prec).float().clone()
    opt = optim.FusedAdamW([p for p in module.parameters() if p.requires_grad], lr=1e-6, max_grad_norm=0.5)
    scaler = DynamicLossScaler() if student_precision == "fp16" else None

    def one():
        loss = module.training_step(batch)
        if scaler is None:
            loss.backward()
            opt.step()
        else:
            scaler.scale(loss).backward()
            scaler.step(opt)
            scaler.update()
        opt.zero_grad(set_to_none=True)
        return loss.detach()
    loss0 = float(one())
    return one, loss0, emb


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def steps(dev, rounds, n):
    variants = {"c3 student bf16, towers bf16": ("c3", "bf16", "bf16"), "c3 student fp16, towers bf16": ("c3", "fp16", "bf16"),
                "c3 student bf16, towers fp16": ("c3", "bf16", "fp16"), "c3 student fp16, towers fp16": ("c3", "fp16", "fp16"),
                "c2 student bf16": ("c2", "bf16", "fp32"), "c2 student fp16": ("c2", "fp16", "fp32")}
    ref = {}
    for wl in ("c3", "c2"):                      # the fp32 student on the same weights and batch (towers fp32)
        one, l32, e32 = make_step(wl, "fp32", "fp32", dev)
        ref[wl] = (l32, e32)
        del one
        torch.cuda.empty_cache()
    fns, rows = {}, {}
    for name, (wl, sp, tp) in variants.items():
        one, l0, emb = make_step(wl, sp, tp, dev)
        one()
        fns[name] = one
        l32, e32 = ref[wl]
        rows[name] = {"case": name, "loss_rel": abs(l0 - l32) / abs(l32), "emb_max_rel": rel(emb, e32)}
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k in fns:
            times[k].append(event_ms(fns[k], n))
    for k in fns:
        rows[k]["ms"] = statistics.median(times[k])
        r = rows[k]
        print(f"{k}: {r['ms']:.2f} ms | loss rel {r['loss_rel']:.2e} | image embedding max rel {r['emb_max_rel']:.2e}",
              flush=True)
    for a, b in (("c3 student fp16, towers bf16", "c3 student bf16, towers bf16"),
                 ("c3 student fp16, towers fp16", "c3 student bf16, towers fp16"), ("c2 student fp16", "c2 student bf16")):
        rows[a]["fp16_vs_bf16"] = rows[a]["ms"] / rows[b]["ms"]
        print(f"step ratio {a} / {b}: {rows[a]['fp16_vs_bf16']:.3f}", flush=True)
    return list(rows.values())


def tail(dev, rounds, n):
    from dclip_amd import config as dcfg, optim, synth
    from dclip_amd.amp import DynamicLossScaler
    from dclip_amd.clip_model import from_hf_state_dict
    cfg = dcfg.vit_b32()
    m = from_hf_state_dict(cfg, synth.synth_clip_state_dict(cfg, seed=0, device=dev), device=dev)
    params = list(m.vision_model.parameters()) + [m.visual_projection.weight]
    gen = torch.Generator(device=dev).manual_seed(0)
    for p in params:
        p.grad = torch.randn(p.shape, generator=gen, device=dev) * 1e-3
    opt = optim.FusedAdamW(params, lr=1e-9, max_grad_norm=0.5)
    sc = DynamicLossScaler(init_scale=1.0)
    sc.scale(torch.ones((), device=dev))

    def scaled():
        sc.step(opt)
        sc.update()
    fns = {"tail FusedAdamW.step (clip + AdamW)": opt.step, "tail scaled step + scale update": scaled}
    for f in fns.values():
        f()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            times[k].append(event_ms(f, n))
    out = []
    npar = sum(p.numel() for p in params) / 1e6
    for k in fns:
        ms = statistics.median(times[k])
        out.append({"case": k, "ms": ms})
        print(f"{k}: {ms * 1000:.1f} us ({npar:.1f} M parameters)", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3, help="steps per timed sample (x10 for the optimizer tail)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = tail(dev, args.rounds, 10 * args.steps)
    rows += steps(dev, args.rounds, args.steps)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        json.dump(rows, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
