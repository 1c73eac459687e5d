"""The TRAINABLE text tower at B = 256, forward and backward: the padded [B, T] rectangle (T = the batch's longest caption)
against the packed captions (each cut after its first EOS, laid back to back), in one process.

ViT-B/32 text tower, random weights, every text parameter trainable.  One call = get_text_features under grad plus the backward
of a fixed weighting (out * W).sum().  Two sets of token ids, those of tools/packed_text_bench.py: (1) seeded ragged lengths
drawn from a clipped normal (--mean / --sd / --max tokens, BOS and EOS included) — an ASSUMPTION about caption lengths, not a
statistic of any dataset: none has been measured for this project; (2) every caption 77 tokens long, the worst case for the
packed path (its tiled attention backward against the padded path's whole-row kernel).  After one warm-up call of each path
the two alternate for --pairs pairs; a timed window is --calls calls and ends in a device synchronise.  Prints the realised
mean and maximum length, Tp / (B * Tmax), ms per call as median (min … max), the largest relative difference of the outputs
and of the gradients, and the peak allocated memory of a call of each path.

usage: python tools/packed_text_train_bench.py [--batch 256] [--mean 20] [--sd 8] [--max 77] [--pairs 3] [--calls 5] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from dclip_amd import config as dcfg, synth  # noqa: E402
from dclip_amd.clip_model import from_hf_state_dict, packed_text_tables  # noqa: E402
from tools.packed_text_bench import ragged_ids  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--mean", type=float, default=20.0, help="mean caption length in tokens, BOS and EOS included (an assumption)")
    ap.add_argument("--sd", type=float, default=8.0)
    ap.add_argument("--max", type=int, default=77, dest="longest")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--calls", type=int, default=5, help="forward + backward calls per timed window")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = torch.device("cuda:0")
    cfg = dcfg.vit_b32()
    clip = from_hf_state_dict(cfg, synth.synth_clip_state_dict(cfg, seed=0, gain=3.0), device=dev)
    clip.requires_grad_(False)
    params = dict(zip(clip.text_params().names(), clip.text_params().tensors()))
    for p in params.values():
        p.requires_grad_(True)
    W = torch.randn((args.batch, cfg.projection_dim), generator=torch.Generator().manual_seed(11)).to(dev)
    sets = {"ragged": ragged_ids(args.batch, cfg.text, args.mean, args.sd, args.longest, args.seed),
            "all77": synth.synth_input_ids(args.batch, cfg.text, seed=args.seed + 1, ragged=False)}
    print(f"caption lengths of the ragged set: clipped normal(mean {args.mean}, sd {args.sd}) in [3, {args.longest}], seed {args.seed} "
          "— an assumption, not a dataset statistic")
    result = {"batch": args.batch, "pairs": args.pairs, "calls": args.calls, "tower": cfg.name}
    for name, ids in sets.items():
        t = packed_text_tables(ids, cfg.text.eos_token_id)
        lens, idd = t["lens"], ids.to(dev)
        fill = t["Tp"] / (ids.shape[0] * ids.shape[1])
        print(f"[{name}] B {ids.shape[0]}, Tmax {ids.shape[1]}, realised mean length {float(lens.float().mean()):.2f}, max {t['max_S']}, "
              f"Tp {t['Tp']}, Tp / (B * Tmax) = {fill:.3f}")

        def call(packed: bool, n: int = 1):
            for _ in range(n):
                for p in params.values():
                    p.grad = None
                kw = {"packed_lens": lens, "packed_train": True} if packed else {}
                out = clip.get_text_features(input_ids=idd, **kw)
                (out * W).sum().backward()
            torch.cuda.synchronize()
            return out.detach(), {k: p.grad.detach().clone() for k, p in params.items()}

        legs = [("padded", False), ("packed", True)]
        res, peak = {}, {}
        for which, packed in legs:                       # warm-up of each (code objects, workspace), then one call for its peak
            call(packed)
            for p in params.values():
                p.grad = None
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            res[which] = call(packed)
            peak[which] = (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20
        (o0, g0), (o1, g1) = res["padded"], res["packed"]
        rel = lambda a, b: float((a - b).abs().max() / b.abs().max())      # noqa: E731
        d_out = rel(o1, o0)
        d_grad = {k: rel(g1[k], g0[k]) for k in g0}
        worst = max(d_grad, key=d_grad.get)
        del res, o0, o1, g0, g1
        ms = {which: [] for which, _ in legs}
        for pair in range(args.pairs):
            for which, packed in legs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call(packed, args.calls)
                ms[which].append(1e3 * (time.perf_counter() - t0) / args.calls)
            print(f"[{name}] pair {pair}: " + ", ".join(f"{which} {ms[which][-1]:.3f} ms" for which in ms))
        med = {k: statistics.median(v) for k, v in ms.items()}
        print(f"[{name}] ms per forward + backward, median of {args.pairs}: padded {med['padded']:.3f} (min {min(ms['padded']):.3f} … max "
              f"{max(ms['padded']):.3f}), packed {med['packed']:.3f} (min {min(ms['packed']):.3f} … max {max(ms['packed']):.3f}); "
              f"padded / packed {med['padded'] / med['packed']:.2f}")
        print(f"[{name}] largest relative difference: outputs {d_out:.3e}, gradients {d_grad[worst]:.3e} ({worst}); peak allocated above "
              f"the resident state: padded {peak['padded']:.1f} MiB, packed {peak['packed']:.1f} MiB")
        result[name] = {"Tmax": ids.shape[1], "mean_len": float(lens.float().mean()), "max_len": t["max_S"], "Tp": t["Tp"], "fill": fill,
                        "ms": ms, "median_ms": med, "max_rel_diff_out": d_out, "max_rel_diff_grad": d_grad[worst],
                        "max_rel_diff_grad_tensor": worst, "peak_mib": peak}
    print(json.dumps(result))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    return result


if __name__ == "__main__":
    main()
