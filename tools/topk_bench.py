#!/usr/bin/env python3
"""Top-k inner-product search: ops.topk_ip against torch.mm + torch.topk in the same process (run on the GPU box).

   python tools/topk_bench.py [--seconds 1.5]

Two shapes (Q, N, P, k): the codebook search of a c3 step's 2048 crops against 10^5 patches at k = 1, and a Flickr30k
evaluation's 5000 captions against 1000 images at k = 10.  Each side is warmed up, then timed with device events over a
window of at least --seconds, the two sides alternating in three rounds (the spread is printed).  Also printed: the peak
device memory each side allocates beyond its operands, and the shader clock rocm-smi reports while the search runs.
One JSON line per shape; DESIGN.md §20 quotes them."""
import argparse
import json
import os
import re
import subprocess
import sys
import threading

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=1.5, help="least length of one timed window")
ap.add_argument("--rounds", type=int, default=3)
args = ap.parse_args()

import torch
from dclip_amd import _lib, ops

if not torch.cuda.is_available():
    sys.exit("topk_bench: no GPU (a timing taken anywhere else says nothing)")
dev = torch.device("cuda:0")
SHAPES = [("codebook c3", 2048, 100_000, 512, 1), ("flickr t2i", 5000, 1000, 512, 10)]


def unit(rows, cols, seed):
    x = torch.randn(rows, cols, generator=torch.Generator().manual_seed(seed))
    return (x / x.norm(dim=1, keepdim=True)).to(dev)


def ours(q, db, k):
    return ops.topk_ip(q, db, k)


def theirs(q, db, k):
    return torch.topk(torch.mm(q, db.t()), k, dim=1)


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters          # ms per call


def iterations(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    return max(3, int(args.seconds * 1e3 / max(window(fn, 3), 1e-3)) + 1)


def peak_extra(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - before
    del out
    return peak


def shader_clock(sample):
    try:
        txt = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        m = re.search(r"sclk clock level: \S+ \((\d+)Mhz\)", txt)
        sample.append(int(m.group(1)) if m else None)
    except Exception:
        sample.append(None)


for name, Q, N, P, k in SHAPES:
    q, db = unit(Q, P, 1), unit(N, P, 2)
    a, b = lambda: ours(q, db, k), lambda: theirs(q, db, k)
    s_a, i_a = a()
    s_b, i_b = b()
    torch.cuda.synchronize()
    same = float((i_a.long() == i_b).float().mean())
    n_a, n_b = iterations(a), iterations(b)
    clock = []
    probe = threading.Thread(target=shader_clock, args=(clock,))
    t_a, t_b = [], []
    for r in range(args.rounds):
        if r == 0:
            probe.start()                     # samples while the first window of the search runs
        t_a.append(window(a, n_a))
        t_b.append(window(b, n_b))
    probe.join()
    flop = 2.0 * Q * N * P
    ws = int(_lib.load().dclip_topk_ip_workspace(Q, N, k))
    print(json.dumps({
        "shape": name, "Q": Q, "N": N, "P": P, "k": k,
        "topk_ip_ms": [round(t, 4) for t in t_a], "mm_topk_ms": [round(t, 4) for t in t_b],
        "topk_ip_tflops": round(flop / min(t_a) / 1e9, 1), "mm_topk_tflops": round(flop / min(t_b) / 1e9, 1),
        "calls_per_window": [n_a, n_b], "indices_equal_share": round(same, 6),
        "topk_ip_workspace_bytes": ws, "topk_ip_peak_extra_bytes": peak_extra(a), "mm_topk_peak_extra_bytes": peak_extra(b),
        "sclk_mhz_during_search": clock[0] if clock else None}), flush=True)
