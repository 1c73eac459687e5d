"""The frozen ViT-B/32 text tower at 256 x 77 in fp32 / split fp16 / plain fp16: time and error, in one process, interleaved.

Per round every path runs once (fp32, split, fp16, ...); the median over rounds is reported with the max relative error
(max|a - b| / max|a|) and min cosine of the embeddings against the fp32 path on the same weights.  `fp32` is
engine.text_fwd_frozen, `split` engine.text_fwd_frozen_split16 with fc1's GELU output split in the GEMM's
epilogue, `split_pass` the same with the stand-alone split pass instead, `fp16` get_text_features(precision="fp16").

usage: python tools/text_tower_split16_bench.py [--rounds 5] [--batch 256] [--gain 1.0] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from dclip_amd import config as dcfg, engine, synth  # noqa: E402
from dclip_amd.clip_model import from_hf_state_dict  # noqa: E402

PATHS = ("fp32", "split", "split_pass", "fp16")


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


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--gain", type=float, default=1.0)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not engine.text_split16_enabled():
        raise SystemExit("DCLIP_TEXT_SPLIT16=0 is set: the split path is switched off")
    dev = torch.device("cuda:0")
    cfg = dcfg.vit_b32()
    m = from_hf_state_dict(cfg, synth.synth_clip_state_dict(cfg, seed=7, gain=args.gain, device=dev), device=dev)
    m.requires_grad_(False)
    x = synth.synth_input_ids(args.batch, cfg.text, seed=3).to(dev)
    p, cache = m.text_params_detached(), m._split16_cache()
    def split(fc1_epilogue):
        engine._SPLIT16_FC1_EPI = fc1_epilogue
        return engine.text_fwd_frozen_split16(p, x, cfg.text, cache)

    fns = {"fp32": lambda: engine.text_fwd_frozen(p, x, cfg.text),
           "split": lambda: split(True), "split_pass": lambda: split(False),
           "fp16": lambda: m.get_text_features(input_ids=x, precision="fp16")}
    with torch.no_grad():
        res = {k: fns[k]() for k in PATHS}                  # warm-up (weight copies, scales) and the outputs compared
        if cache["__split16__"]["layers"] is None:
            raise SystemExit("the guard sent the split path to fp32: nothing to measure")
        times = {k: [] for k in PATHS}
        for _ in range(args.rounds):
            for k in PATHS:
                times[k].append(event_ms(fns[k], 3))
    row = {"case": f"text tower ViT-B/32 {args.batch} x {x.shape[1]}, gain {args.gain}"}
    for k in PATHS:
        row[k + "_ms"] = statistics.median(times[k])
        if k != "fp32":
            row[k + "_max_rel"], row[k + "_min_cos"] = errors(res["fp32"], res[k])
    print(f"{row['case']}: fp32 {row['fp32_ms']:.2f} ms | split {row['split_ms']:.2f} ms (max rel {row['split_max_rel']:.2e}, "
          f"cos {row['split_min_cos']:.7f}) | split with the stand-alone pass after fc1 {row['split_pass_ms']:.2f} ms | fp16 {row['fp16_ms']:.2f} ms (max rel {row['fp16_max_rel']:.2e}, "
          f"cos {row['fp16_min_cos']:.7f}) | fp32/split {row['fp32_ms'] / row['split_ms']:.2f}x", flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        json.dump([row], open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
