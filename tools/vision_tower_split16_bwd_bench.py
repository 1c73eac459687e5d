"""The student's ViT-B/32 vision backward at 256 x 50 tokens: plain fp32 data-gradient GEMMs against the split-fp16 ones with a
scale per row of dY, in one process, interleaved, median over rounds.  Both backwards follow the same split-fp16
forward.

Also, per data-gradient GEMM of an encoder layer at M = batch * 50 (K' = 3 x the layer's output width): the row-scaled GEMM on
each kernel the library has for it (the dispatcher's own choice, the register-staged 128x128 tile, the 128x128 LDS-DMA tile),
the plain fp32 NN GEMM it replaces, the row-split pass per width (768, 2304, 3072) and the weight refresh with and without the
transposed copies.

usage: python tools/vision_tower_split16_bwd_bench.py [--rounds 5] [--batch 256] [--gain 1.0] [--json out.json]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from dclip_amd import config as dcfg, engine, ops, synth  # noqa: E402
from dclip_amd.clip_model import from_hf_state_dict  # noqa: E402
from vision_tower_split16_bench import Env, interleaved  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--gain", type=float, default=1.0)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = dcfg.vit_b32()
    v = cfg.vision
    m = from_hf_state_dict(cfg, synth.synth_clip_state_dict(cfg, seed=7, gain=args.gain, device=dev), device=dev)
    pix = synth.synth_pixel_values(args.batch, v, seed=0).to(dev)
    p = engine.VisionParams.from_tensors([t.detach() for t in m.vision_params().tensors()], v.num_hidden_layers)
    need = [True] * len(p.tensors())
    cache = m._vsplit16_cache()
    engine._VSPLIT16 = engine._VSPLIT16_BWD = True
    d_out = torch.randn((args.batch, cfg.projection_dim), device=dev)
    rows = []

    # ---- the backward alone: every timed call re-runs the (untimed) forward, which the backward consumes
    def timed_backward(split):
        def run():
            s16 = []
            _, saved = engine.vision_fwd(p, pix, v, True, split16_cache=cache, split16_out=s16)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            grads = engine.vision_bwd(p, saved, d_out, v, need, split16=s16[0] if split else None)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1), grads
        return run
    runs = {"plain": timed_backward(False), "split": timed_backward(True)}
    ref, got = runs["plain"]()[1], runs["split"]()[1]
    times = {k: [] for k in runs}
    for _ in range(args.rounds):
        for k, f in runs.items():
            times[k].append(f()[0])
    t = {k: sorted(x)[len(x) // 2] for k, x in times.items()}
    rel = max(float((g - r).abs().max() / r.abs().max().clamp_min(1e-30)) for g, r in zip(got, ref) if r is not None)
    rows.append({"case": f"vision backward ViT-B/32 {args.batch} x {v.seq_len}, gain {args.gain}", **{k + "_ms": x for k, x in t.items()},
                 "max_rel_grad": rel})
    print(f"{rows[-1]['case']}: plain {t['plain']:.3f} ms | split {t['split']:.3f} ms | plain/split {t['plain'] / t['split']:.2f}x | "
          f"worst parameter gradient, norm-wise {rel:.2e}", flush=True)
    del ref, got

    # ---- the refresh with and without the transposed copies
    tab = cache["__vsplit16__"]["tab"]
    tab_fwd = {k: x for k, x in tab.items() if k != "dst_t"}
    t = interleaved({"with": lambda: ops.split16_refresh(tab), "without": lambda: ops.split16_refresh(tab_fwd)}, args.rounds, 5)
    rows.append({"case": "statistics + plan + weight split, 12 layers", "with_transposed_us": 1e3 * t["with"], "forward_only_us": 1e3 * t["without"]})
    print(f"statistics + plan + weight split of {tab['L']} layers: {t['with'] * 1e3:.1f} us with the transposed copies | "
          f"{t['without'] * 1e3:.1f} us without", flush=True)

    # ---- per data-gradient GEMM: dX [M, in] = dY [M, out] W [out, in]
    M, D, I = args.batch * v.seq_len, v.hidden_size, v.intermediate_size
    lp, sp = p.layers[0], cache["__vsplit16__"]["layers"][0]
    one = torch.ones((1,), device=dev)
    dys = {w: torch.randn((M, w), device=dev) for w in (D, 3 * D, I)}
    split = {w: ops.split_f16x3_rows(x) for w, x in dys.items()}
    h = torch.randn((M, I), device=dev)
    kernels = {"default": {}, "r128": dict(DCLIP_BF16_BIG_MIN="1000000")}
    shapes = {"dh (fc2)": ("fc2", D, lp.fc2_w, h), "dln2 (fc1)": ("fc1", I, lp.fc1_w, None), "dattn (out)": ("out", D, lp.out_w, None),
              "dln1 (qkv)": ("qkv", 3 * D, lp.qkv_w, None)}
    for label, (name, width, w, aux) in shapes.items():
        dy, (dy3, ra) = dys[width], split[width]
        fns = {"fp32": (lambda dy=dy, w=w, aux=aux: engine._dgrad(dy, w, None, name, aux)[0])}
        for kn, env in kernels.items():
            def f(env=env, dy3=dy3, ra=ra, name=name, aux=aux):
                with Env(**env):
                    ops.gemm_f16_rows_dev(dy3, sp.wt[name], one.data_ptr(), ra, dgelu_h=aux)
            fns[kn] = f
        t = interleaved(fns, args.rounds, 5)
        rows.append({"case": f"{label} {M}x{w.shape[1]}x{3 * w.shape[0]}", **{k + "_us": 1e3 * x for k, x in t.items()}})
        print(f"{label:11s} M {M} N {w.shape[1]} K' {3 * w.shape[0]}: " + " | ".join(f"{k} {1e3 * x:.0f} us" for k, x in t.items()), flush=True)

    # ---- the row-split pass per width
    t = interleaved({str(w): (lambda x=x: ops.split_f16x3_rows(x)) for w, x in dys.items()}, args.rounds, 5)
    rows.append({"case": f"row-split pass, {M} rows", **{k + "_us": 1e3 * x for k, x in t.items()}})
    print(f"row-split pass, {M} rows: " + " | ".join(f"{k} columns {1e3 * x:.0f} us ({M * int(k) * 10 / (x * 1e-3) / 1e12:.2f} TB/s)"
                                                     for k, x in t.items()), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        json.dump(rows, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
