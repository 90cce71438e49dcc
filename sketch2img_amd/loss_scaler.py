"""DynamicLossScaler: the reference's GradScaler (accelerate mixed_precision="fp16") for the three trainers, opt-in through their
``scaler=`` keyword.  Without one the trainers keep their static power-of-two loss scale.

Protocol of one training step (lgp_train.train_step / sat_train.train_step with scaler=):

    s = scaler.scale                       resolves the previous step's verdict first (a 4-byte copy), so s is final
    seed the backward with s               the seed kernels take the scale by value
    backward, all_reduce
    v = scaler.check(g[, gt])              skg_nonfinite_flag over every flat gradient into ONE device flag; nothing waits
    opt.step(g, scaler=scaler, scale=s)    skg_adamw_step_guarded on that flag, for every optimizer; nothing waits
    ...                                    bool(v), scaler.scale or the next check() resolve the verdict

Resolving reads the flag back and applies torch's update rule (torch._amp_update_scale_): on a hit scale *= backoff_factor and the
growth tracker returns to 0; otherwise the tracker advances and, on reaching growth_interval, scale *= growth_factor and the tracker
returns to 0.  It then tells every optimizer that stepped under the verdict whether its tentative step counts: step_count - and with it
the bias correction and the position in the LR schedule - advances only on a clean verdict, and a skipped step has left p, m, v and
the fp16 copy untouched on the device (the guarded kernel returned at once).

Invariants: the scale and both factors are powers of two, so the scale divides out of the gradients exactly and a scaler started at a
trainer's static LOSS_SCALE reproduces the static path bit for bit; one flag and one verdict cover all optimizers of a step (the
reference has one GradScaler for SatMixin and tower: both step or neither); the verdict is taken after the all-reduce, where a
non-finite value in any rank's addend has made the sum non-finite on every rank, so the ranks agree without a collective of their own.

state_dict() / load_state_dict() use torch.amp.GradScaler's keys, so the scaler.pt of an accelerate checkpoint loads as data.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional

import torch

from . import ops


def _power_of_two(x: float) -> bool:
    return x > 0.0 and math.isfinite(x) and math.frexp(x)[0] == 0.5


class Verdict:
    """What check() returns.  bool(v): whether the optimizers' step counted (the gradients were finite); it resolves the verdict."""

    def __init__(self, scaler: "DynamicLossScaler"):
        self._scaler = scaler
        self.found_inf: Optional[bool] = None       # None until resolved

    @property
    def resolved(self) -> bool:
        return self.found_inf is not None

    def __bool__(self) -> bool:
        if self.found_inf is None:
            self._scaler.resolve()
        return not self.found_inf

    def __repr__(self) -> str:
        return "Verdict(pending)" if self.found_inf is None else f"Verdict(stepped={not self.found_inf})"


class DynamicLossScaler:
    def __init__(self, device, init_scale: float = 65536.0, growth_factor: float = 2.0, backoff_factor: float = 0.5,
                 growth_interval: int = 2000):
        """torch.amp.GradScaler's defaults.  The scale and the two factors must be powers of two (growth > 1, backoff < 1)."""
        assert _power_of_two(float(init_scale)), "the loss scale must be a power of two"
        assert _power_of_two(float(growth_factor)) and growth_factor > 1.0, "the growth factor must be a power of two above 1"
        assert _power_of_two(float(backoff_factor)) and backoff_factor < 1.0, "the backoff factor must be a power of two below 1"
        assert int(growth_interval) >= 1
        self.dev = torch.device(device)
        self.flag = torch.zeros(1, device=self.dev, dtype=torch.float32)
        self._scale = float(init_scale)
        self.growth_factor, self.backoff_factor = float(growth_factor), float(backoff_factor)
        self.growth_interval = int(growth_interval)
        self._growth_tracker = 0
        self.verdict: Optional[Verdict] = None      # the last check()'s
        self._steppers: List = []                   # optimizers that queued a guarded step under the pending verdict
        self._host = None                           # pinned landing place of the flag + the event that says it has landed
        self._event = None

    # ------------------------------------------------------------------------------------------ the state machine
    def update(self, found_inf: bool) -> float:
        """torch._amp_update_scale_ on the host: one verdict in, the new scale out."""
        if found_inf:
            self._scale *= self.backoff_factor
            self._growth_tracker = 0
        else:
            self._growth_tracker += 1
            if self._growth_tracker == self.growth_interval:
                self._scale *= self.growth_factor
                self._growth_tracker = 0
        assert _power_of_two(self._scale), f"the loss scale left fp32's powers of two: {self._scale}"
        return self._scale

    @property
    def scale(self) -> float:
        """The scale to seed the next backward with; a pending verdict is resolved first."""
        self.resolve()
        return self._scale

    @property
    def growth_tracker(self) -> int:
        self.resolve()
        return self._growth_tracker

    @property
    def pending(self) -> bool:
        return self.verdict is not None and not self.verdict.resolved

    # ------------------------------------------------------------------------------------------ one step
    @torch.no_grad()
    def check(self, *flat_grads: torch.Tensor) -> Verdict:
        """Queue the finiteness test of every flat fp32 gradient into the one flag (reset by the first) and the 4-byte copy of the
        flag to the host.  Nothing waits; the guarded steps that follow on the stream read the flag on the device."""
        assert flat_grads, "check() needs at least one gradient vector"
        self.resolve()
        for i, g in enumerate(flat_grads):
            ops.nonfinite_flag(g, self.flag, reset=(i == 0))
        if self.flag.is_cuda:
            if self._host is None:
                self._host = torch.zeros(1, dtype=torch.float32).pin_memory()
                self._event = torch.cuda.Event()
            self._host.copy_(self.flag, non_blocking=True)
            self._event.record(torch.cuda.current_stream(self.dev))
        self.verdict = Verdict(self)
        return self.verdict

    def register(self, optimizer) -> None:
        """An optimizer has queued its guarded step under the pending verdict (FlatAdamW.step(scaler=) calls this)."""
        assert self.pending, "step(scaler=) comes after scaler.check() of the same gradients"
        assert all(o is not optimizer for o in self._steppers), "one guarded step per optimizer and verdict"
        self._steppers.append(optimizer)

    def resolve(self) -> None:
        """Read the pending verdict (if any), update scale and tracker, settle the optimizers that stepped under it."""
        v = self.verdict
        if v is None or v.resolved:
            return
        if self._event is not None:
            self._event.synchronize()
            found = float(self._host[0]) != 0.0
        else:
            found = float(self.flag[0]) != 0.0
        v.found_inf = found
        self.update(found)
        steppers, self._steppers = self._steppers, []
        for o in steppers:
            o.settle(not found)

    # ------------------------------------------------------------------------------------------ checkpoint
    def state_dict(self) -> Dict[str, float]:
        """torch.amp.GradScaler.state_dict()'s five keys."""
        self.resolve()
        return {"scale": self._scale, "growth_factor": self.growth_factor, "backoff_factor": self.backoff_factor,
                "growth_interval": self.growth_interval, "_growth_tracker": self._growth_tracker}

    def load_state_dict(self, sd: Dict[str, float]) -> None:
        want = {"scale", "growth_factor", "backoff_factor", "growth_interval", "_growth_tracker"}
        assert set(sd) == want, f"a GradScaler state dict has the keys {sorted(want)}, got {sorted(sd)}"
        self.resolve()
        scale, growth, backoff = float(sd["scale"]), float(sd["growth_factor"]), float(sd["backoff_factor"])
        assert _power_of_two(scale) and _power_of_two(growth) and growth > 1.0 and _power_of_two(backoff) and backoff < 1.0, \
            "the scale and the factors must be powers of two"
        self._scale, self.growth_factor, self.backoff_factor = scale, growth, backoff
        self.growth_interval, self._growth_tracker = int(sd["growth_interval"]), int(sd["_growth_tracker"])
