"""The weight-gradient GEMMs of the student's ViT-B/32 vision backward at batch x 50 tokens: the plain fp32 TN GEMM (with its
bias-gradient epilogue) against the segmented split-fp16 token-major GEMM, in one process, interleaved, median
over rounds — per shape with the split count the plan picks and its neighbours — and the fused pass over dY (row split + column
statistics + bias gradient + column-scaled split) against the row split alone, per width, in us and TB/s.

usage: python tools/vision_tower_split16_wgrad_bench.py [--rounds 5] [--batch 256] [--json out.json]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from dclip_amd import config as dcfg, ops  # noqa: E402
from vision_tower_split16_bench import interleaved  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    v = dcfg.vit_b32().vision
    T, D, I = args.batch * v.seq_len, v.hidden_size, v.intermediate_size
    rows = []
    act = torch.ones((1,), device=dev)
    dys = {w: torch.randn((T, w), device=dev) * 1e-4 for w in (D, 3 * D, I)}
    xs = {w: torch.randn((T, w), device=dev) for w in (D, I)}
    x3 = {w: ops.split_f16x3(x, 1.0, 0) for w, x in xs.items()}

    # ---- per weight gradient: dW [out, in] = dY [T, out]^T X [T, in]
    for label, out_w, in_w in (("fc2_w", D, I), ("fc1_w", I, D), ("out_w", D, D), ("qkv_w", 3 * D, D)):
        dy, x = dys[out_w], xs[in_w]
        _, _, yc, _, ca = ops.split_f16x3_rows_colstats(dy)
        s0 = ops.gemm_f16_wgrad_tokmajor_seg3_plan(out_w, in_w, T)
        db = torch.empty((out_w,), device=dev)
        dw = torch.empty((out_w, in_w), device=dev)
        fns = {"fp32": (lambda dy=dy, x=x, dw=dw, db=db: ops.gemm(dy, x, ops.LAYOUT_TN, out=dw, a_rowsum=db))}
        for s in sorted({max(1, s0 - 1), max(1, s0), min(21, max(1, s0) + 1), min(21, 2 * max(1, s0))}):
            fns[f"seg3 s0={s}" + (" (plan)" if s == s0 else "")] = (
                lambda yc=yc, ca=ca, s=s, dw=dw, in_w=in_w, out_w=out_w: ops.gemm_f16_wgrad_tokmajor_seg3(
                    yc, x3[in_w], out_w, in_w, ca, act.data_ptr(), splits=s, out=dw))
        t = interleaved(fns, args.rounds, 5)
        rows.append({"case": f"{label} {out_w}x{in_w}, {T} tokens", "plan_s0": s0, **{k + "_us": 1e3 * x for k, x in t.items()}})
        print(f"{label:6s} dW {out_w}x{in_w}, {T} tokens: " + " | ".join(f"{k} {1e3 * x:.0f} us" for k, x in t.items()), flush=True)

    # ---- the pass over dY: bytes = 4 read + 6 written (row split); + 4 read + 4 written (column-scaled split)
    for w, dy in dys.items():
        db = torch.empty((w,), device=dev)
        t = interleaved({"rows": lambda dy=dy: ops.split_f16x3_rows(dy),
                         "fused": lambda dy=dy, db=db: ops.split_f16x3_rows_colstats(dy, db=db)}, args.rounds, 5)
        rows.append({"case": f"dY pass, {T} x {w}", **{k + "_us": 1e3 * x for k, x in t.items()}})
        print(f"dY pass {T} x {w}: row split {1e3 * t['rows']:.0f} us ({T * w * 10 / (t['rows'] * 1e-3) / 1e12:.2f} TB/s) | fused row + "
              f"column pass {1e3 * t['fused']:.0f} us ({T * w * 18 / (t['fused'] * 1e-3) / 1e12:.2f} TB/s)", flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        json.dump(rows, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
