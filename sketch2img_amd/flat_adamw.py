"""The optimizer state the three trainers (lgp_train, sat_train, clip_vision_train) share: one flat fp32 master vector, its fp16
working copy, AdamW's m / v, views of all of them by state-dict key, and the LR schedules.

What replaces the reference's accelerate fp16 autocast + GradScaler + bitsandbytes AdamW8bit: fp16 compute on the working copy, fp32
masters, plain fp32 AdamW (skg_adamw_step divides the gradient scale out and refreshes the fp16 copy).  The gradient scale is a static
power of two by default; the reference's GradScaler - scale halved and step skipped on overflow, doubled after growth_interval good
steps - is step(scaler=) with a loss_scaler.DynamicLossScaler (verdict on the device, skg_adamw_step_guarded, no host wait).
"""
from __future__ import annotations

import math
from typing import Callable, Dict, Iterable, Optional, Sequence, Tuple

import torch

from . import ops


def constant_with_warmup(step: int, warmup: int) -> float:
    """diffusers "constant_with_warmup": min(1, step / warmup) (reference trainer.py:133-138)."""
    return 1.0 if warmup <= 0 else min(1.0, float(step) / float(max(1, warmup)))


def cosine_with_restarts(step: int, warmup: int, total: int, cycles: int = 1) -> float:
    """The multiplier diffusers' get_cosine_with_hard_restarts_schedule_with_warmup applies at optimizer step `step`."""
    if step < warmup:
        return float(step) / float(max(1, warmup))
    p = float(step - warmup) / float(max(1, total - warmup))
    if p >= 1.0:
        return 0.0
    return max(0.0, 0.5 * (1.0 + math.cos(math.pi * ((float(cycles) * p) % 1.0))))


class FlatAdamW:
    def __init__(self, shapes: Sequence[Tuple[str, Sequence[int]]], state_dict: Dict[str, torch.Tensor], device, lr: float, betas,
                 eps: float, weight_decay: float, schedule: Callable[[int], float], grad_scale: float, frozen: Iterable[str] = ()):
        """shapes: (key, shape) in the order of the vector; every tensor starts at a multiple of 8 elements (16-byte aligned in the
        fp16 copy).  frozen keys are laid out last, at and beyond n_opt: AdamW runs on [0, n_opt), weight decay included, the way
        torch's AdamW skips a parameter whose gradient is None.  schedule(step_count) -> the multiplier of lr.  grad_scale: what
        the gradients handed to step() carry."""
        self.dev = torch.device(device)
        self.lr, self.betas, self.eps, self.wd = lr, betas, eps, weight_decay
        self.schedule, self.grad_scale = schedule, float(grad_scale)
        self.step_count = 0
        # a step ran since what a trainer derives from the fp16 copy (the injector's / the tower's packs) was built: set by a static
        # step that ran and by settle(True); the trainer reads and clears it before it refreshes its packs
        self.stale = False
        frozen = set(frozen)
        self.layout: Dict[str, Tuple[int, torch.Size]] = {}
        off = 0
        for part in (False, True):
            if part:
                self.n_opt = off
            for k, shp in shapes:
                if (k in frozen) == part:
                    assert tuple(state_dict[k].shape) == tuple(shp), (k, tuple(state_dict[k].shape), tuple(shp))
                    self.layout[k] = (off, torch.Size(shp))
                    off += (math.prod(shp) + 7) // 8 * 8
        self.n = off
        self.p = torch.zeros(off, device=self.dev, dtype=torch.float32)
        for k, (o, shp) in self.layout.items():
            self.p[o:o + shp.numel()] = state_dict[k].detach().to(self.dev, torch.float32).reshape(-1)
        self.p16 = self.p.to(torch.float16)
        self.m = torch.zeros_like(self.p)
        self.v = torch.zeros_like(self.p)

    # ------------------------------------------------------------------------------------------ views
    def _at(self, key: str) -> Tuple[int, torch.Size]:
        return self.layout[key]

    def _view(self, vec: torch.Tensor, key: str) -> torch.Tensor:
        o, shp = self._at(key)
        return vec[o:o + shp.numel()].view(shp)

    def w16(self, key: str) -> torch.Tensor:
        return self._view(self.p16, key)

    def w32(self, key: str) -> torch.Tensor:
        return self._view(self.p, key)

    def grad_view(self, g: torch.Tensor, key: str) -> torch.Tensor:
        return self._view(g, key)

    def new_grad(self) -> torch.Tensor:
        return torch.zeros(self.n, device=self.dev, dtype=torch.float32)

    # ------------------------------------------------------------------------------------------ collective
    def all_reduce(self, g: torch.Tensor, bucket_bytes: int = 15 << 20) -> torch.Tensor:
        """Average the flat gradient over the ranks: dist.allreduce_mean_ (15 MB buckets like the reference's DDP, bucket_cap_mb =
        15).  No-op on one rank."""
        from .dist import allreduce_mean_
        return allreduce_mean_(g, bucket_bytes)

    # ------------------------------------------------------------------------------------------ optimizer
    def current_lr(self) -> float:
        return self.lr * self.schedule(self.step_count)

    @torch.no_grad()
    def step(self, g: torch.Tensor, checked: bool = False, scaler=None, scale: Optional[float] = None):
        """AdamW on the masters (g carries grad_scale), fp16 copy refreshed.  A non-finite gradient skips the step: False, before
        any kernel runs, with p, m, v, p16 and the step count untouched (the static-scale form of GradScaler's skipped step).
        checked=True: the caller has already found g finite (sat_train.train_step with a tower decides for both optimizers at
        once), or wants no test (it costs a device synchronisation).

        scaler (a loss_scaler.DynamicLossScaler whose check() has been queued over g) + scale (what g carries: the scaler's scale
        when the backward was seeded, times the trainer's own static factor where it has one): the step is queued behind the
        scaler's device flag (skg_adamw_step_guarded) as step step_count + 1 at the LR of step_count, and nothing waits.  Returns
        the scaler's pending verdict; step_count advances when it resolves clean (settle), so a skipped step leaves step count,
        LR schedule position, p, m, v and p16 as they were."""
        if scaler is not None:
            assert scale is not None and scale > 0.0, "step(scaler=) needs scale=: what the gradient carries"
            scaler.register(self)
            n = self.n_opt
            ops.adamw_step_guarded(self.p[:n], g[:n], self.m[:n], self.v[:n], self.p16[:n], self.current_lr(), self.betas[0],
                                   self.betas[1], self.eps, self.wd, self.step_count + 1, 1.0 / float(scale), scaler.flag)
            return scaler.verdict
        if not checked and not bool(torch.isfinite(g).all()):
            return False
        lr = self.current_lr()
        self.step_count += 1
        n = self.n_opt
        ops.adamw_step(self.p[:n], g[:n], self.m[:n], self.v[:n], self.p16[:n], lr, self.betas[0], self.betas[1], self.eps, self.wd,
                       self.step_count, 1.0 / self.grad_scale)
        self.stale = True
        return True

    def settle(self, stepped: bool) -> None:
        """The scaler's verdict on the guarded step queued by step(scaler=): only a step that ran counts (and leaves packs stale)."""
        if stepped:
            self.step_count += 1
            self.stale = True

    def state_dict(self, keys: Optional[Iterable[str]] = None) -> Dict[str, torch.Tensor]:
        """Clones of the fp32 masters under their keys, in the order of `keys` (default: the vector's)."""
        return {k: self.w32(k).clone() for k in (self.layout if keys is None else keys)}
