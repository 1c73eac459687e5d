"""The student's ViT-B/32 vision forward (the gradient-enabled, saving one) at 256 x 50 tokens: plain fp32 against split fp16
with the device-side plan, in one process, interleaved, median over rounds.

Also, per GEMM of an encoder layer at M = batch * 50 (K' = 3K): the time of the device-scaled split GEMM on each kernel the
library has for it (the dispatcher's own choice, the register-staged 128x128 tile, the 128x128 LDS-DMA tile), the plain fp32
GEMM it replaces, the two forms of fc1 (h, g and the split of g from one launch / h and g from the GEMM and the stand-alone
split pass), and the three launches that re-plan and re-split the weights.

usage: python tools/vision_tower_split16_bench.py [--rounds 5] [--batch 256] [--gain 1.0] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from dclip_amd import config as dcfg, engine, ops, synth  # noqa: E402
from dclip_amd.clip_model import from_hf_state_dict  # noqa: E402


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
    for f in fns.values():
        f()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            times[k].append(event_ms(f, n))
    return {k: statistics.median(v) for k, v in times.items()}


class Env:
    """Environment switches of the 16-bit GEMM dispatcher that are read per call."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update(self.kw)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


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
    cache = m._vsplit16_cache()
    rows = []

    # ---- the tower
    def tower(split):
        engine._VSPLIT16 = split
        return engine.vision_fwd(p, pix, v, True, split16_cache=cache)[0]

    def tower_form(epi):
        engine._VSPLIT16_FC1_EPI = epi
        return tower(True)

    ref, got = tower(False), tower(True)
    t = interleaved({"plain": lambda: tower(False), "split": lambda: tower_form(True), "split_fc1_pass": lambda: tower_form(False)},
                    args.rounds, 3)
    engine._VSPLIT16_FC1_EPI = True
    rel = float((got - ref).abs().max() / ref.abs().max())
    row = {"case": f"vision forward ViT-B/32 {args.batch} x {v.seq_len}, gain {args.gain}", **{k + "_ms": x for k, x in t.items()},
           "max_rel": rel}
    rows.append(row)
    print(f"{row['case']}: plain {t['plain']:.3f} ms | split {t['split']:.3f} ms | split, stand-alone pass after fc1 "
          f"{t['split_fc1_pass']:.3f} ms | plain/split {t['plain'] / t['split']:.2f}x | max rel {rel:.2e}", flush=True)

    # ---- the refresh (statistics, plan, weight split)
    tab = cache["__vsplit16__"]["tab"]
    t = interleaved({"refresh": lambda: ops.split16_refresh(tab)}, args.rounds, 5)
    rows.append({"case": "statistics + plan + weight split, 12 layers", "ms": t["refresh"]})
    print(f"statistics + plan + weight split of {tab['L']} layers: {t['refresh'] * 1e3:.1f} us", flush=True)

    # ---- per GEMM
    M, D, I = args.batch * v.seq_len, v.hidden_size, v.intermediate_size
    lp, sp = p.layers[0], cache["__vsplit16__"]["layers"][0]
    x = torch.randn((M, D), device=dev)
    xi = torch.randn((M, I), device=dev)
    one = torch.ones((1,), device=dev)
    a3, a3i = ops.split_f16x3(x, 1.0), ops.split_f16x3(xi, 1.0)
    kernels = {"default": {}, "r128": dict(DCLIP_BF16_BIG_MIN="1000000")}
    shapes = {"qkv": (a3, x, lp.qkv_w, lp.qkv_b, None), "out": (a3, x, lp.out_w, lp.out_b, x), "fc2": (a3i, xi, lp.fc2_w, lp.fc2_b, x)}
    for name, (a, a32, w, b, res) in shapes.items():
        fns = {"fp32": lambda: ops.gemm(a32, w, ops.LAYOUT_NT, bias=b, residual=res)}
        for kn, env in kernels.items():
            def f(env=env):
                with Env(**env):
                    ops.gemm_f16_dev(a, sp.w[name], one.data_ptr(), bias=b, residual=res)
            fns[kn] = f
        t = interleaved(fns, args.rounds, 5)
        rows.append({"case": f"{name} {M}x{w.shape[0]}x{3 * w.shape[1]}", **{k + "_us": 1e3 * x for k, x in t.items()}})
        print(f"{name:4s} M {M} N {w.shape[0]} K' {3 * w.shape[1]}: " + " | ".join(f"{k} {1e3 * x:.0f} us" for k, x in t.items()), flush=True)
    h = torch.empty((M, I), device=dev)
    g = torch.empty((M, I), device=dev)
    fns = {"fp32": lambda: ops.gemm(x, lp.fc1_w, ops.LAYOUT_NT, bias=lp.fc1_b, aux=h, epilogue=ops.EPI_GELU)}
    for kn, env in kernels.items():
        def epi(env=env):
            with Env(**env):
                ops.gemm_f16_dev(a3, sp.w["fc1"], one.data_ptr(), bias=lp.fc1_b, gelu=True, split_out_scale_ptr=one.data_ptr(), h32=h, g32=g)

        def two(env=env):
            with Env(**env):
                ops.split_f16x3_dev(ops.gemm_f16_dev(a3, sp.w["fc1"], one.data_ptr(), bias=lp.fc1_b, gelu=True, h32=h), one.data_ptr())
        fns[kn + " one launch"], fns[kn + " gemm+split"] = epi, two
    t = interleaved(fns, args.rounds, 5)
    rows.append({"case": f"fc1 {M}x{I}x{3 * D}", **{k + "_us": 1e3 * x for k, x in t.items()}})
    print(f"fc1  M {M} N {I} K' {3 * D}: " + " | ".join(f"{k} {1e3 * x:.0f} us" for k, x in t.items()), flush=True)
    fns = {"layernorm fp32": lambda: ops.layernorm_fwd(x, lp.ln1_w, lp.ln1_b, 1e-5),
           "layernorm split + fp32": lambda: ops.layernorm_fwd_f16x3_dev(x, lp.ln1_w, lp.ln1_b, 1e-5, one.data_ptr(), save=True),
           "split pass": lambda: ops.split_f16x3_dev(x, one.data_ptr())}
    t = interleaved(fns, args.rounds, 5)
    rows.append({"case": f"row-wise passes {M}x{D}", **{k + "_us": 1e3 * x for k, x in t.items()}})
    print(f"row-wise M {M} D {D}: " + " | ".join(f"{k} {1e3 * x:.0f} us" for k, x in t.items()), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        json.dump(rows, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
