"""Student launcher — `main(args)` as in training/CLIP_image_distill_training.py:20-45, with the Lightning pieces it
uses restated in lightning_lite.py.  Models are loaded from a LOCAL path (`--clip_path`), never by hub name.

`--devices N` (the reference hard-codes `devices=1`, :39) trains data-parallel on N GPUs of one node: run as a script
it starts its N ranks itself (`python -m torch.distributed.run --nproc-per-node N` as a CHILD process, before anything
has touched the GPU); under torch.distributed.run it joins the rendezvous it is given."""
from __future__ import annotations

import argparse
import os
from typing import Optional

import torch

from .CLIP_image_distillation import CLIPImageDistillation
from .lightning_lite import Trainer


def main(args, clip_model=None, clip_preprocess=None, train_batches=None, val_batches=None, **module_kwargs):
    devices = int(getattr(args, "devices", 1) or 1)
    if devices > 1 and torch.cuda.is_available():
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % max(1, torch.cuda.device_count()))
        device = torch.device("cuda", torch.cuda.current_device())
    else:
        device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    if clip_model is None:
        if not getattr(args, "clip_path", None) or not os.path.isdir(args.clip_path):
            raise SystemExit("--clip_path must name a local directory with HF CLIP weights (nothing is downloaded)")
        from transformers import CLIPModel, CLIPProcessor
        clip_model = CLIPModel.from_pretrained(args.clip_path, local_files_only=True).to(device)
        clip_preprocess = CLIPProcessor.from_pretrained(args.clip_path, local_files_only=True)
    module_kwargs.setdefault("student_precision", getattr(args, "student_precision", "fp32"))
    module_kwargs.setdefault("full_resolution_from_epoch", resolve_full_resolution_epoch(args))
    module_kwargs.setdefault("packed_text", bool(getattr(args, "packed_text", False)))
    module_kwargs.setdefault("packed_attention16", True if getattr(args, "packed_attention16", False) else None)
    module_kwargs.setdefault("packed_text_train", bool(getattr(args, "packed_text_train", False)))
    module_kwargs.setdefault("text_train_split16", bool(getattr(args, "text_train_split16", False)))
    model = CLIPImageDistillation(args, clip_model, clip_preprocess, **module_kwargs).to(device)
    trainer = Trainer(max_epochs=args.phase1_epochs, accelerator="gpu", devices=devices, precision=32,
                      gradient_clip_val=0.5, accumulate_grad_batches=4, checkpoint_dir=args.checkpoint_dir,
                      save_top_k=10, max_steps=getattr(args, "max_steps", None))
    trainer.fit(model, train_batches, val_batches)
    return model, trainer


def _epoch_or_half(value: str):
    return "half" if value == "half" else int(value)


def resolve_full_resolution_epoch(args) -> Optional[int]:
    """--full_resolution_from_epoch as an epoch number: `half` is phase1_epochs // 2 (training/CLIP_image_distillation.py:723-729)."""
    v = getattr(args, "full_resolution_from_epoch", None)
    return args.phase1_epochs // 2 if v == "half" else v


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser()
    parser = CLIPImageDistillation.add_model_specific_args(parser)
    parser.add_argument("--checkpoint_dir", type=str, default="./checkpoints")          # :50
    parser.add_argument("--phase1_epochs", type=int, default=2)                          # :51
    parser.add_argument("--clip_path", type=str, default=None)
    parser.add_argument("--devices", type=int, default=1, help="GPUs of this node (one process per GPU, RCCL)")
    parser.add_argument("--student_precision", choices=("fp32", "bf16", "fp16"), default="fp32",
                        help="GEMM inputs of the student's vision tower: fp32 (the reference), bf16, or fp16 with a dynamic "
                             "loss scale (Lightning's precision='16-mixed')")
    parser.add_argument("--full_resolution_from_epoch", type=_epoch_or_half, default=None, metavar="N|half",
                        help="from this epoch on the meta-teacher encodes region crops at their own size, in one packed tower "
                             "pass; `half` = phase1_epochs // 2, the reference's rule (default: never)")
    parser.add_argument("--packed_text", action="store_true",
                        help="run the frozen text towers on captions cut after their first EOS and laid back to back "
                             "(lengths from the tokenizer's host output; default: the padded [B, T] rectangle)")
    parser.add_argument("--packed_text_train", action="store_true",
                        help="where the student's text tower trains, run it on captions cut after their first EOS and laid "
                             "back to back, forward and backward (lengths from the tokenizer's host output; default: the "
                             "padded [B, T] rectangle)")
    parser.add_argument("--text_train_split16", action="store_true",
                        help="where the student's text tower trains, run its layers' full-size fp32 GEMMs (forward, data and "
                             "weight gradients) on the fp16 MFMAs from hi/lo split operands at fp32-grade error (default: the "
                             "plain fp32 GEMMs)")
    parser.add_argument("--packed_attention16", action="store_true",
                        help="16-bit packed frozen towers keep q, k, v and the context in 16 bits and run the packed MFMA "
                             "attention core (default: fp32 q | k | v, the fp32 packed core and a cast)")
    return parser


def launch_ranks(devices: int, module: str, argv) -> int:
    """`python -m torch.distributed.run --nnodes=1 --nproc-per-node devices -m module argv...` as a child process; returns
    its exit code.  Called before this process has touched the GPU; never an exec."""
    import socket
    import subprocess
    import sys
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")          # dmabuf IPC: what RCCL needs on this driver
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // devices)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={devices}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), "-m", module] + list(argv)
    return subprocess.run(cmd, env=env).returncode


if __name__ == "__main__":
    import sys
    _args = build_parser().parse_args()
    if _args.devices > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(launch_ranks(_args.devices, "dclip_amd.CLIP_image_distill_training", sys.argv[1:]))
    main(_args)
