#!/usr/bin/env python3
"""Per shape: the fused split-fp16 entry (dclip_gemm_f16x3_*) against the entry it twins, interleaved in one
process, median of 7 windows of HIP-event time.  Shapes: the vision forward (M = 12,800) and the frozen text tower (M = 19,712),
the data-gradient transposes of the vision shapes (row-scaled entry), and the four weight gradients at 12,800 tokens.
  --sweep      the token-major twin at every split count 1..40 beside its plan and the segmented entry
  --only WHICH --shape NAME --iters N    one entry on one shape, for a counter run of its own (rocprofv3 --pmc FETCH_SIZE)
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
FWD = [("v.qkv", VIS, 2304, 768), ("v.out", VIS, 768, 768), ("v.fc1", VIS, 3072, 768), ("v.fc2", VIS, 768, 3072),
       ("t.qkv", TXT, 1536, 512), ("t.out", TXT, 512, 512), ("t.fc1", TXT, 2048, 512), ("t.fc2", TXT, 512, 2048)]
DGRAD = [("d.qkv", VIS, 768, 2304), ("d.out", VIS, 768, 768), ("d.fc1", VIS, 768, 3072), ("d.fc2", VIS, 3072, 768)]
WGRAD = [("w.qkv", 2304, 768, VIS), ("w.out", 768, 768, VIS), ("w.fc1", 3072, 768, VIS), ("w.fc2", 768, 3072, VIS)]


def f16(shape, seed):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * 8).half().to(dev)


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def pair(fa, fb, iters, reps=7):
    """Median microseconds of two callables measured alternately."""
    for fn in (fa, fb):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(window(fa, iters))
        tb.append(window(fb, iters))
    return statistics.median(ta), statistics.median(tb), (max(ta) - min(ta)), (max(tb) - min(tb))


def calls(name, M, N, K):
    """(unfused, fused) callables of one shape."""
    one = torch.ones(1, device=dev)
    if name[0] in "vt":
        a, w = f16((M, 3 * K), 1), f16((N, 3 * K), 2)
        bias = torch.zeros(N, device=dev)
        return (lambda: ops.gemm_f16_dev(a, w, one.data_ptr(), bias=bias)), (lambda: ops.gemm_f16x3_dev(a, w, one.data_ptr(), bias=bias))
    if name[0] == "d":
        a, w = f16((M, 3 * K), 1), f16((N, 3 * K), 2)
        ra = torch.ones(M, device=dev)
        return (lambda: ops.gemm_f16_rows_dev(a, w, one.data_ptr(), ra)), (lambda: ops.gemm_f16x3_rows_dev(a, w, one.data_ptr(), ra))
    dy, x = f16((K, 2 * M), 1), f16((K, 3 * N), 2)
    ca = torch.ones(M, device=dev)
    out = torch.empty((M, N), device=dev)
    return (lambda: ops.gemm_f16_wgrad_tokmajor_seg3(dy, x, M, N, ca, one.data_ptr(), out=out),
            lambda s=None: ops.gemm_f16x3_wgrad_tokmajor(dy, x, M, N, ca, one.data_ptr(), splits=s or ops.gemm_f16x3_wgrad_tokmajor_plan(M, N, K) or
                                                          3 * ops.gemm_f16_wgrad_tokmajor_seg3_plan(M, N, K), out=out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--only", choices=["fused", "unfused"])
    ap.add_argument("--shape")
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    shapes = FWD + DGRAD + WGRAD
    if args.only:
        name, M, N, K = [s for s in shapes if s[0] == args.shape][0]
        fn = calls(name, M, N, K)[args.only == "fused"]
        for _ in range(args.iters):
            fn()
        torch.cuda.synchronize()
        print(f"{name} {args.only}: {args.iters} calls")
        return
    if args.sweep:
        for name, M, N, K in WGRAD:
            un, fu = calls(name, M, N, K)
            plan = ops.gemm_f16x3_wgrad_tokmajor_plan(M, N, K)
            res = {}
            for s in range(1, 41):
                t_un, t_fu, _, _ = pair(un, lambda: fu(s), args.iters, reps=3)
                res[s] = t_fu
            best = sorted(res.items(), key=lambda kv: kv[1])[:6]
            print(f"{name:6s} seg3 {t_un:7.1f} us | plan s={plan}: {res.get(plan, float('nan')):7.1f} us | best " +
                  " ".join(f"s{s}:{t:.1f}" for s, t in best), flush=True)
        return
    print(f"{'shape':6s} {'M':>6s} {'N':>5s} {'K':>6s} {'unfused us':>11s} {'fused us':>9s} {'ratio':>6s} {'spread un/fu us':>16s} {'fused TF/s':>10s}")
    tot_u = tot_f = 0.0
    for name, M, N, K in shapes:
        un, fu = calls(name, M, N, K)
        t_un, t_fu, s_un, s_fu = pair(un, fu, args.iters)
        tot_u, tot_f = tot_u + t_un, tot_f + t_fu
        print(f"{name:6s} {M:6d} {N:5d} {K:6d} {t_un:11.1f} {t_fu:9.1f} {t_fu / t_un:6.3f} {s_un:7.1f}/{s_fu:<7.1f} {6.0 * M * N * K / t_fu / 1e6:10.1f}",
              flush=True)
    print(f"sum of one call each: unfused {tot_u:.1f} us, fused {tot_f:.1f} us, ratio {tot_f / tot_u:.3f}")


if __name__ == "__main__":
    main()
