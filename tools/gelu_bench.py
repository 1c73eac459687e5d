"""What hidden_act="gelu" costs while its activation is a stand-alone pass, in one process, interleaved, median
over rounds, device events around work that ends in a synchronise:

  1. fc1 as a bias-only GEMM followed by the erf-GELU pass, against fc1 with the fused quick-GELU epilogue, at the fc1 shapes of
     the c2 student (fp32 12,800 x 3072 and 19,712 x 2048) and of the 16-bit teachers (bf16 102,400 x 3072, 526,336 x 4096);
  2. the pass alone, as GB/s of the bytes it must move (one read and one write of [M, I]) and as a share of the HBM peak;
  3. a frozen ViT-B/32 model end to end — image tower and text tower — under both activations, per precision.  At "fp32" the
     quick-GELU text tower takes the split-fp16 plan by default and a "gelu" tower cannot: the plain fp32 quick-GELU tower
     (DCLIP_TEXT_SPLIT16 off) is timed beside them, so that the activation's own cost can be read apart from the lost plan.

usage: python tools/gelu_bench.py [--rounds 7] [--batch 256] [--skip-large] [--json out.json]
"""
import argparse
import dataclasses
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from dclip_amd import config as dcfg, engine, ops, synth  # noqa: E402
from dclip_amd.clip_model import from_hf_state_dict  # noqa: E402

HBM_PEAK_GBS = 8000.0                  # MI355X: 8 TB/s
FC1_SHAPES = [("fp32", 12800, 3072, 768), ("fp32", 19712, 2048, 512), ("bf16", 102400, 3072, 768), ("bf16", 526336, 4096, 1024)]


def event_ms(fn, n):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def interleaved(fns, rounds, n):
    for f in fns.values():              # warm-up: every shape of the timed window
        f()
        f()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            times[k].append(event_ms(f, n))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def fc1_case(kind, M, I, K, rounds, dev):
    gen = torch.Generator(device=dev).manual_seed(M)
    a = torch.randn((M, K), device=dev, generator=gen)
    w = torch.randn((I, K), device=dev, generator=gen) * K ** -0.5
    b = torch.randn((I,), device=dev, generator=gen) * 0.1
    reps = 3 if M * I > 1 << 30 else 10
    if kind == "fp32":
        out = torch.empty((M, I), device=dev)
        fns = {"fused quick-GELU": lambda: ops.gemm(a, w, ops.LAYOUT_NT, bias=b, epilogue=ops.EPI_GELU, out=out),
               "bias-only GEMM": lambda: ops.gemm(a, w, ops.LAYOUT_NT, bias=b, out=out),
               "bias-only GEMM + erf pass": lambda: ops.gelu_erf(ops.gemm(a, w, ops.LAYOUT_NT, bias=b, out=out), out=out),
               "erf pass alone": lambda: ops.gelu_erf(out, out=out)}
        elem = 4
    else:
        a16, w16 = ops.cast_bf16(a), ops.cast_bf16(w)
        out = torch.empty((M, I), dtype=torch.bfloat16, device=dev)
        fns = {"fused quick-GELU": lambda: ops.gemm_bf16(a16, w16, bias=b, gelu=True, out_bf16=True, out=out),
               "bias-only GEMM": lambda: ops.gemm_bf16(a16, w16, bias=b, out_bf16=True, out=out),
               "bias-only GEMM + erf pass": lambda: ops.gelu_erf(ops.gemm_bf16(a16, w16, bias=b, out_bf16=True, out=out), out=out),
               "erf pass alone": lambda: ops.gelu_erf(out, out=out)}
        elem = 2
    t = interleaved(fns, rounds, reps)
    gbs = 2.0 * M * I * elem / (t["erf pass alone"][0] * 1e-3) / 1e9
    row = {"case": f"fc1 {kind} {M} x {I} (K = {K})", **{k + " ms": v[0] for k, v in t.items()},
           **{k + " min..max ms": [v[1], v[2]] for k, v in t.items()}, "erf pass GB/s": gbs, "erf pass share of HBM peak": gbs / HBM_PEAK_GBS,
           "unfused minus fused ms": t["bias-only GEMM + erf pass"][0] - t["fused quick-GELU"][0]}
    print(f"{row['case']}: " + " | ".join(f"{k} {v[0]:.3f} ms ({v[1]:.3f}..{v[2]:.3f})" for k, v in t.items()) +
          f" | pass {gbs:.0f} GB/s = {100 * gbs / HBM_PEAK_GBS:.0f} % of the HBM peak (memory-bound: 2 x {M * I * elem / 1e6:.0f} MB) | "
          f"unfused - fused {row['unfused minus fused ms']:+.3f} ms", flush=True)
    return row


def tower_case(batch, rounds, dev):
    rows = []
    base = dcfg.vit_b32()
    sd = synth.synth_clip_state_dict(base, seed=7, gain=1.0)
    models = {}
    for act in ("quick_gelu", "gelu"):
        cfg = dataclasses.replace(base, vision=dataclasses.replace(base.vision, hidden_act=act), text=dataclasses.replace(base.text, hidden_act=act))
        models[act] = from_hf_state_dict(cfg, sd, device=dev).requires_grad_(False)
    pix = synth.synth_pixel_values(batch, base.vision, seed=0).to(dev)
    ids = synth.synth_input_ids(batch, base.text, seed=3, ragged=True).to(dev)

    def text_plain_quick():
        engine._SPLIT16 = False
        try:
            return models["quick_gelu"].get_text_features(input_ids=ids)
        finally:
            engine._SPLIT16 = True
    with torch.no_grad():
        for prec in ("fp32", "bf16", "fp16"):
            fns = {f"image {a}": (lambda a=a: models[a].get_image_features(pixel_values=pix, precision=prec)) for a in models}
            fns.update({f"text {a}": (lambda a=a: models[a].get_text_features(input_ids=ids, precision=prec)) for a in models})
            if prec == "fp32":
                fns["text quick_gelu, plain fp32 GEMMs"] = text_plain_quick
            t = interleaved(fns, rounds, 3)
            row = {"case": f"frozen ViT-B/32, {batch} images x 50 tokens / {batch} captions x 77 tokens, {prec}",
                   **{k + " ms": v[0] for k, v in t.items()}, **{k + " min..max ms": [v[1], v[2]] for k, v in t.items()}}
            rows.append(row)
            print(f"{row['case']}: " + " | ".join(f"{k} {v[0]:.3f} ms ({v[1]:.3f}..{v[2]:.3f})" for k, v in t.items()), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--skip-large", action="store_true", help="leave out the 526,336 x 4096 shape (4.3 GB of bf16 output)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gelu_bench needs the GPU: a time taken anywhere else says nothing about it")
    dev = torch.device("cuda:0")
    prop = torch.cuda.get_device_properties(dev)
    box = {"device": prop.name, "compute units": prop.multi_processor_count, "clock MHz": getattr(prop, "clock_rate", 0) / 1e3,
           "memory GiB": prop.total_memory / 2 ** 30, "torch": torch.__version__, "hip": torch.version.hip, "rounds": args.rounds,
           "timing": "device events around repeated calls, median (min..max) over interleaved rounds"}
    print("box:", box, flush=True)
    rows = [{"box": box}]
    for kind, M, I, K in FC1_SHAPES:
        if args.skip_large and M * I > 1 << 30:
            continue
        rows.append(fc1_case(kind, M, I, K, args.rounds, dev))
        torch.cuda.empty_cache()
    rows += tower_case(args.batch, args.rounds, dev)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        json.dump(rows, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
