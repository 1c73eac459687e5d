#!/usr/bin/env python3
"""Per shape: the fused split-fp16 entry (dclip_gemm_f16x3_*) on the 256-row tile against the 192-row tile,
interleaved in one process, median of 7 windows of 20 calls of HIP-event time.  Shapes: the flagship step's twelve K-major GEMMs
— the vision forward (M = 12,800, the device-scale entry), the frozen text tower (M = 19,712, the plain entry) and the vision data
gradients (the row-scaled entry); out / fc2 carry the residual as in the step.  The tile is chosen per window through
DCLIP_F16X3_BM192 = 0 / 2, so the five shapes the plan leaves on 256 rows are on record too; `plan` is what the library takes.
  --reps N     repeat the whole table N times (a class that loses must lose in every repetition to leave the rule)
Run on the GPU box."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from dclip_amd import ops

dev = torch.device("cuda:0")
VIS, TXT = 12800, 19712
SHAPES = [("v.qkv", VIS, 2304, 768), ("v.out", VIS, 768, 768), ("v.fc1", VIS, 3072, 768), ("v.fc2", VIS, 768, 3072),
          ("t.qkv", TXT, 1536, 512), ("t.out", TXT, 512, 512), ("t.fc1", TXT, 2048, 512), ("t.fc2", TXT, 512, 2048),
          ("d.qkv", VIS, 768, 2304), ("d.out", VIS, 768, 768), ("d.fc1", VIS, 768, 3072), ("d.fc2", VIS, 3072, 768)]


def f16(shape, seed):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * 8).half().to(dev)


def call(name, M, N, K):
    one = torch.ones(1, device=dev)
    a, w = f16((M, 3 * K), 1), f16((N, 3 * K), 2)
    bias = torch.zeros(N, device=dev)
    res = torch.zeros((M, N), device=dev) if name[2:] in ("out", "fc2") else None
    if name[0] == "v":
        return lambda: ops.gemm_f16x3_dev(a, w, one.data_ptr(), bias=bias, residual=res)
    if name[0] == "t":
        return lambda: ops.gemm_f16x3(a, w, bias=bias, residual=res)
    ra = torch.ones(M, device=dev)
    return lambda: ops.gemm_f16x3_rows_dev(a, w, one.data_ptr(), ra)


def window(fn, mode, iters):
    os.environ["DCLIP_F16X3_BM192"] = mode
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def pair(fn, iters, windows=7):
    """Median microseconds on the 256-row and the 192-row tile, measured alternately, and each arm's spread."""
    for mode in ("0", "2"):
        window(fn, mode, 3)
    t = {"0": [], "2": []}
    for _ in range(windows):
        for mode in ("0", "2"):
            t[mode].append(window(fn, mode, iters))
    return (statistics.median(t["0"]), statistics.median(t["2"]), max(t["0"]) - min(t["0"]), max(t["2"]) - min(t["2"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=1)
    args = ap.parse_args()
    keep = os.environ.pop("DCLIP_F16X3_BM192", None)
    for rep in range(args.reps):
        print(f"{'shape':6s} {'M':>6s} {'N':>5s} {'K':>5s} {'tiles 256/192':>13s} {'plan':>5s} {'256 us':>8s} {'192 us':>8s} {'ratio':>6s} "
              f"{'spread us':>12s} {'best TF/s':>9s}")
        s256 = s192 = splan = 0.0
        for name, M, N, K in SHAPES:
            os.environ.pop("DCLIP_F16X3_BM192", None)
            plan = ops.gemm_f16x3_tile_rows(M, N, K, rows_form=name[0] == "d")
            t256, t192, d256, d192 = pair(call(name, M, N, K), args.iters)
            s256, s192, splan = s256 + t256, s192 + t192, splan + (t192 if plan == 192 else t256)
            tiles = f"{-(-M // 256) * -(-N // 256)}/{-(-M // 192) * -(-N // 256)}"
            print(f"{name:6s} {M:6d} {N:5d} {K:5d} {tiles:>13s} {plan:5d} {t256:8.1f} {t192:8.1f} {t192 / t256:6.3f} {d256:5.1f}/{d192:<5.1f} "
                  f"{6.0 * M * N * K / min(t256, t192) / 1e6:9.1f}", flush=True)
        print(f"repetition {rep + 1}: one call each, all on 256 rows {s256:.1f} us, all on 192 rows {s192:.1f} us, by plan {splan:.1f} us "
              f"({splan / s256:.3f})", flush=True)
    if keep is not None:
        os.environ["DCLIP_F16X3_BM192"] = keep


if __name__ == "__main__":
    main()
