"""dclip_amd — MI355X-native DCLIP distillation step."""
import os as _os

# The pool's host driver only supports dmabuf IPC; RCCL / device-tensor sharing across ranks fails with
# `hipIpcGetMemHandle: invalid argument` otherwise.  It has to be in the environment before the process's first HIP
# call, so it is defaulted at package import (importing torch does not initialise HIP).
_os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

__version__ = "0.2.0"

# A process that has used the GPU must not run GPU finalizers in a FORKED child (DataLoader workers, multiprocessing
# managers): a child inherits the parent's unreachable-but-uncollected reference cycles — a module holding device tensors
# recorded on a side stream, HIP events — and its first garbage collection would free them there, through a HIP runtime that
# does not exist in the child (a segmentation fault in the child's collector thread).  Collecting in the parent right before
# every fork leaves the child no such garbage.
import gc as _gc

_os.register_at_fork(before=_gc.collect)
