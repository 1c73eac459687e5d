"""`DynamicLossScaler`: torch.amp.GradScaler semantics for the fp16 student (student_precision="fp16", Lightning's
precision="16-mixed"), kept on the device.

The scale and the growth tracker live in device memory.  The unscaling is folded into the fused optimizer's clip coefficient
(FusedAdamW.step_scaled: dclip_mt_sumsq_f32 -> dclip_clip_coef_scaled -> dclip_mt_adamw_f32_skip), so the scaler adds no pass
over the gradients, and the skip decision is a found-inf flag the AdamW kernel reads on the device: the step path never waits
for a device-to-host read.  Order per optimizer step, as in Lightning: unscale, clip, step (skipped when the gradient norm is
not finite), update.

One documented difference from torch: the skip test looks at the global norm, not at each element, so a finite gradient whose
sum of squares overflows fp32 (a norm above about 1.8e19) counts as an overflow too."""
from __future__ import annotations

import math
from typing import Optional

import torch

from . import _lib


class DynamicLossScaler:
    def __init__(self, init_scale: float = 2.0 ** 16, growth_factor: float = 2.0, backoff_factor: float = 0.5,
                 growth_interval: int = 2000):
        init_scale = float(init_scale)
        if not (math.isfinite(init_scale) and init_scale > 0.0):
            raise ValueError(f"DynamicLossScaler: init_scale must be a positive finite number, got {init_scale}")
        if not float(growth_factor) > 1.0:
            raise ValueError(f"DynamicLossScaler: growth_factor must be > 1, got {growth_factor}")
        if not 0.0 < float(backoff_factor) < 1.0:
            raise ValueError(f"DynamicLossScaler: backoff_factor must be in (0, 1), got {backoff_factor}")
        if isinstance(growth_interval, bool) or not isinstance(growth_interval, int) or growth_interval < 1:
            raise ValueError(f"DynamicLossScaler: growth_interval must be a positive int, got {growth_interval!r}")
        self._init_scale = init_scale
        self._growth_factor = float(growth_factor)
        self._backoff_factor = float(backoff_factor)
        self._growth_interval = int(growth_interval)
        self._init_tracker = 0
        self._scale: Optional[torch.Tensor] = None       # fp32 [1] on the device, made at the first scale()
        self._tracker: Optional[torch.Tensor] = None     # int32 [1]
        self._out: Optional[torch.Tensor] = None         # fp32 [3]: unscaled norm, found_inf, clip coefficient / scale
        self._optimizer = None                           # the optimizer last stepped (its skipped step may be pending)
        self._stepped = False

    def _lazy_init(self, device: torch.device) -> None:
        if self._scale is None:
            self._scale = torch.full((1,), self._init_scale, dtype=torch.float32, device=device)
            self._tracker = torch.full((1,), self._init_tracker, dtype=torch.int32, device=device)
            self._out = torch.zeros(3, dtype=torch.float32, device=device)

    # ------------------------------------------------------------------ GradScaler surface of the training loop
    def scale(self, loss: torch.Tensor) -> torch.Tensor:
        """loss * scale (a device multiply: no host read)."""
        if not loss.is_cuda:
            raise ValueError("DynamicLossScaler.scale: the loss must be a CUDA tensor")
        self._lazy_init(loss.device)
        return loss * self._scale

    def step(self, optimizer) -> None:
        """Unscale, clip (optimizer.max_grad_norm) and step — the step changes nothing (parameters, moments, the Adam step
        count) when the gradient norm is not finite.  The optimizer must have the fused path (FusedAdamW.step_scaled)."""
        if not hasattr(optimizer, "step_scaled"):
            raise TypeError(f"DynamicLossScaler.step: {type(optimizer).__name__} has no fused scaled step (use optim.FusedAdamW)")
        if self._scale is None:
            raise RuntimeError("DynamicLossScaler.step: no loss was scaled before the step")
        if not optimizer.step_scaled(self):
            # torch's GradScaler: "No inf checks were recorded for this optimizer." — update() must not act on an old flag
            raise RuntimeError("DynamicLossScaler.step: no parameter of the optimizer has a gradient (no inf check recorded)")
        self._optimizer = optimizer
        self._stepped = True

    def update(self) -> None:
        """torch's _amp_update_scale_ on the device: back off after a skipped step, grow after growth_interval clean ones."""
        if self._scale is None:
            return
        if not self._stepped:
            raise RuntimeError("DynamicLossScaler.update: no step() was recorded before update()")
        lib = _lib.load()
        _lib.check(lib.dclip_amp_update_scale(self._scale.data_ptr(), self._tracker.data_ptr(), self._out.data_ptr() + 4,
                                              self._growth_factor, self._backoff_factor, self._growth_interval,
                                              torch.cuda.current_stream(self._scale.device).cuda_stream), "amp_update_scale")
        self._stepped = False

    def get_scale(self) -> float:
        """The current scale (a host read: for logging, not for the step path)."""
        return float(self._scale.item()) if self._scale is not None else self._init_scale

    def found_inf(self) -> Optional[torch.Tensor]:
        """Device flag (fp32, 1.0 = skipped) of the last step(), or None before the first one."""
        return None if self._out is None else self._out[1]

    # ------------------------------------------------------------------ checkpoints (GradScaler's keys)
    def _settle(self) -> None:
        if self._optimizer is not None:
            self._optimizer.settle_scaled_step()

    def state_dict(self) -> dict:
        self._settle()
        tracker = int(self._tracker.item()) if self._tracker is not None else self._init_tracker
        return {"scale": self.get_scale(), "growth_factor": self._growth_factor, "backoff_factor": self._backoff_factor,
                "growth_interval": self._growth_interval, "_growth_tracker": tracker}

    def load_state_dict(self, state_dict: dict) -> None:
        if not state_dict:
            raise RuntimeError("DynamicLossScaler.load_state_dict: the state dict is empty")
        self._init_scale = float(state_dict["scale"])
        self._growth_factor = float(state_dict["growth_factor"])
        self._backoff_factor = float(state_dict["backoff_factor"])
        self._growth_interval = int(state_dict["growth_interval"])
        self._init_tracker = int(state_dict["_growth_tracker"])
        if self._scale is not None:
            self._scale.fill_(self._init_scale)
            self._tracker.fill_(self._init_tracker)
