"""The frozen text tower at B = 256: the padded [B, T] rectangle (T = the batch's longest caption, what `padding=True` gives)
against the packed captions (each cut after its first EOS, laid back to back), in one process.

ViT-B/32 text tower, random weights.  Two sets of token ids: (1) seeded ragged lengths drawn from a clipped normal
(--mean / --sd / --max tokens, BOS and EOS included) — an ASSUMPTION about caption lengths, not a statistic of any dataset: none
has been measured for this project; (2) every caption 77 tokens long, the worst case for the packed path and what bench.py's
synthetic ids are.  For fp32 (the split-fp16 plan, the default), bf16 and fp16: after one warm-up call of each path the two
alternate for --pairs pairs; a timed window is --calls get_text_features calls and ends in a device synchronise.  Prints the
realised mean and maximum length, Tp / (B * Tmax), ms per call (each pair, then the median and the spread) and the largest
relative difference of the two outputs.  --attn16 adds, for bf16 and fp16, the leg "packed + 16-bit core" (the packed tower with
HipCLIPModel.packed_attention16 on), which alternates with the other two under the same protocol.

usage: python tools/packed_text_bench.py [--batch 256] [--mean 20] [--sd 8] [--max 77] [--pairs 3] [--calls 10] [--attn16]
       [--json out.json]
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


def ragged_ids(batch: int, cfg, mean: float, sd: float, longest: int, seed: int) -> torch.Tensor:
    """[B, Tmax] int64 as the CLIP tokenizer pads them (EOS id behind the first EOS); lengths (BOS .. EOS) from a normal
    clipped into [3, longest], Tmax = the batch's longest caption."""
    gen = torch.Generator().manual_seed(seed)
    lens = (torch.randn(batch, generator=gen) * sd + mean).round().clamp(3, min(longest, cfg.max_position_embeddings)).long()
    T = int(lens.max())
    ids = torch.randint(1, min(cfg.bos_token_id, cfg.eos_token_id), (batch, T), generator=gen, dtype=torch.int64)
    ids[:, 0] = cfg.bos_token_id
    for b in range(batch):
        ids[b, int(lens[b]) - 1:] = cfg.eos_token_id
    return ids


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--mean", type=float, default=20.0, help="mean caption length in tokens, BOS and EOS included (an assumption)")
    ap.add_argument("--sd", type=float, default=8.0)
    ap.add_argument("--max", type=int, default=77, dest="longest")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10, help="get_text_features calls per timed window")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--precisions", nargs="+", default=["fp32", "bf16", "fp16"], choices=["fp32", "bf16", "fp16"])
    ap.add_argument("--attn16", action="store_true",
                    help="bf16 / fp16: add the leg `packed + 16-bit core` (HipCLIPModel.packed_attention16), alternating with the others")
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = torch.device("cuda:0")
    cfg = dcfg.vit_b32()
    clip = from_hf_state_dict(cfg, synth.synth_clip_state_dict(cfg, seed=0, gain=3.0), device=dev)
    clip.requires_grad_(False)
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
        result[name] = {"Tmax": ids.shape[1], "mean_len": float(lens.float().mean()), "max_len": t["max_S"], "Tp": t["Tp"],
                        "fill": fill}
        for prec in args.precisions:
            def call(packed: bool, n: int = 1, attn16: bool = False):
                clip.packed_attention16 = attn16
                with torch.no_grad():
                    for _ in range(n):
                        out = clip.get_text_features(input_ids=idd, precision=prec, packed_lens=lens if packed else None)
                torch.cuda.synchronize()
                return out

            # --attn16 (16-bit precisions): a third leg, the packed tower with the 16-bit packed attention core
            legs = [("padded", False, False), ("packed", True, False)]
            if args.attn16 and prec != "fp32":
                legs.append(("packed16", True, True))
            outs = {which: call(packed, 1, a16) for which, packed, a16 in legs}     # warm-up of each (weight copies, plan, code objects)
            want, got = outs["padded"], outs["packed"]
            diff = float((got - want).abs().max() / want.abs().max())
            ms = {which: [] for which, _, _ in legs}
            for pair in range(args.pairs):
                for which, packed, a16 in legs:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    call(packed, args.calls, a16)
                    ms[which].append(1e3 * (time.perf_counter() - t0) / args.calls)
                print(f"[{name} {prec}] pair {pair}: " + ", ".join(f"{which} {ms[which][-1]:.3f} ms" for which in ms))
            med = {k: statistics.median(v) for k, v in ms.items()}
            print(f"[{name} {prec}] ms per call, median of {args.pairs}: padded {med['padded']:.3f} (min {min(ms['padded']):.3f}, max "
                  f"{max(ms['padded']):.3f}), packed {med['packed']:.3f} (min {min(ms['packed']):.3f}, max {max(ms['packed']):.3f}); "
                  f"padded / packed {med['padded'] / med['packed']:.2f}; largest relative difference of the outputs {diff:.3e}")
            result[name][prec] = {"ms": ms, "median_ms": med, "max_rel_diff": diff}
            if "packed16" in ms:
                d16 = float((outs["packed16"] - want).abs().max() / want.abs().max())
                print(f"[{name} {prec}] packed + 16-bit core {med['packed16']:.3f} (min {min(ms['packed16']):.3f}, max "
                      f"{max(ms['packed16']):.3f}); packed / packed16 {med['packed'] / med['packed16']:.2f}, padded / packed16 "
                      f"{med['padded'] / med['packed16']:.2f}; largest relative difference to the padded output {d16:.3e}")
                result[name][prec]["max_rel_diff_packed16"] = d16
            clip.packed_attention16 = None
    print(json.dumps(result))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    return result


if __name__ == "__main__":
    main()
