"""The optimizer state the three trainers (lgp_train, sat_train, clip_vision_train) share: one flat fp32 master vector, its fp16
working copy, AdamW's m / v, views of all of them by state-dict key, and the LR schedules.

What replaces the reference's accelerate fp16 autocast + GradScaler + bitsandbytes AdamW8bit: fp16 compute on the working copy, fp32
masters, plain fp32 AdamW (skg_adamw_step divides the gradient scale out and refreshes the fp16 copy).  The gradient scale is a static
power of two by default; the reference's GradScaler - scale halved and step skipped on overflow, doubled after growth_interval good
steps - is step(scaler=) with a loss_scaler.DynamicLossScaler (verdict on the device, skg_adamw_step_guarded, no host wait).

state_bits = 8 is the counterpart of AdamW8bit's state: m and v as one uint8 code per element plus one fp32 absmax per block of at
most 2048 elements (block-wise dynamic quantisation, Dettmers et al., "8-bit Optimizers via Block-wise Quantization", restated in
DESIGN.md section 15 - not bitsandbytes' binaries, and no checkpoint compatibility with them), tensors below min_8bit_size keeping
fp32 moments; one launch of skg_adamw8_step over a block table built here.  The default stays fp32.
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


Q8_BLOCK = 2048


def quant_maps() -> Tuple[torch.Tensor, torch.Tensor]:
    """The two 256-entry fp32 maps, sorted ascending: signed (for m) and unsigned (for v).  Decade i = 0 ... 6 contributes the
    midpoints of k equal-width cells on [0.1, 1], times 10^(i - 6): k = 2^i and both signs in the signed map, k = 2^(i + 1) in the
    unsigned one; each map also holds 0 and 1.  A value is (0.1 + 0.9 * (j + 0.5) / k) / 10^(6 - i) evaluated in that order in
    float64 and rounded once to fp32."""
    def decades(k0: int):
        return [(0.1 + 0.9 * (j + 0.5) / (k0 << i)) / 10.0 ** (6 - i) for i in range(7) for j in range(k0 << i)]
    pos = decades(1)
    signed = torch.tensor(sorted([-x for x in pos] + [0.0] + pos + [1.0]), dtype=torch.float64).to(torch.float32)
    unsigned = torch.tensor(sorted([0.0] + decades(2) + [1.0]), dtype=torch.float64).to(torch.float32)
    assert signed.numel() == unsigned.numel() == 256 and float(signed[127]) == 0.0 and float(unsigned[0]) == 0.0
    return signed, unsigned


def quant_table(signed: torch.Tensor, unsigned: torch.Tensor) -> torch.Tensor:
    """What skg_adamw8_step reads, 4 x 256 fp32: each map followed by its 255 thresholds mid[j] = 0.5f * (q[j] + q[j + 1]), computed
    here in fp32 (the device never recomputes them), and one unused slot."""
    tab = torch.full((4, 256), float("inf"), dtype=torch.float32)
    for r, q in ((0, signed), (2, unsigned)):
        tab[r] = q
        tab[r + 1, :255] = 0.5 * (q[:-1] + q[1:])
    return tab.reshape(-1)


def build_rows(layout: Dict[str, Tuple[int, torch.Size]], n_opt: int, min_8bit_size: int):
    """The block table of skg_adamw8_step over the optimised part [0, n_opt) of a layout: rows (int64 [R, 4]: offset into the flat
    vector, length <= 2048, offset into the state arrays, 1 = 8-bit / 0 = fp32), spans {key: (is8, state offset, first row, rows)},
    and the lengths of the code arrays and of the compact fp32 moment arrays.  A block is at most 2048 consecutive elements of ONE
    tensor, counted from its first element, so the last block of a tensor is short and no row touches the padding between tensors;
    a tensor with fewer than min_8bit_size elements keeps fp32 moments; frozen keys (at and beyond n_opt) get no row.  Every
    tensor starts at a multiple of 8 in its state array too (the kernel's 8-byte code loads)."""
    rows, spans, used = [], {}, [0, 0]
    for k, (off, shp) in layout.items():
        n = shp.numel()
        if off >= n_opt or n == 0:
            continue
        is8 = int(n >= min_8bit_size)
        spans[k] = (bool(is8), used[is8], len(rows), (n + Q8_BLOCK - 1) // Q8_BLOCK)
        rows += [(off + b, min(Q8_BLOCK, n - b), used[is8] + b, is8) for b in range(0, n, Q8_BLOCK)]
        used[is8] += (n + 7) // 8 * 8
    return torch.tensor(rows, dtype=torch.int64).reshape(-1, 4), spans, used[1], used[0]


class FlatAdamW:
    def __init__(self, shapes: Sequence[Tuple[str, Sequence[int]]], state_dict: Dict[str, torch.Tensor], device, lr: float, betas,
                 eps: float, weight_decay: float, schedule: Callable[[int], float], grad_scale: float, frozen: Iterable[str] = (),
                 state_bits: int = 32, min_8bit_size: int = 4096):
        """shapes: (key, shape) in the order of the vector; every tensor starts at a multiple of 8 elements (16-byte aligned in the
        fp16 copy).  frozen keys are laid out last, at and beyond n_opt: AdamW runs on [0, n_opt), weight decay included, the way
        torch's AdamW skips a parameter whose gradient is None.  schedule(step_count) -> the multiplier of lr.  grad_scale: what
        the gradients handed to step() carry.  state_bits: 32 (m, v in fp32) or 8 (uint8 codes + one absmax per block of 2048; tensors
        below min_8bit_size elements keep fp32 moments; self.m / self.v do not exist)."""
        assert state_bits in (32, 8), "state_bits: 32 or 8"
        self.state_bits, self.min_8bit_size = int(state_bits), int(min_8bit_size)
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
        if self.state_bits == 32:
            self.m = torch.zeros_like(self.p)
            self.v = torch.zeros_like(self.p)
            return
        rows, self.spans, n_codes, n_small = build_rows(self.layout, self.n_opt, self.min_8bit_size)
        self.rows = rows.to(self.dev)
        self.qmap1, self.qmap2 = quant_maps()
        self.qtab = quant_table(self.qmap1, self.qmap2).to(self.dev)
        # zero state: the zero codes (127 signed, 0 unsigned) under absmax 0; the arrays are never empty (the kernel takes no null)
        self.state1 = torch.full((max(n_codes, 8),), 127, device=self.dev, dtype=torch.uint8)
        self.state2 = torch.zeros(max(n_codes, 8), device=self.dev, dtype=torch.uint8)
        self.absmax1 = torch.zeros(max(rows.shape[0], 1), device=self.dev, dtype=torch.float32)
        self.absmax2 = torch.zeros_like(self.absmax1)
        self.m32 = torch.zeros(max(n_small, 8), device=self.dev, dtype=torch.float32)
        self.v32 = torch.zeros_like(self.m32)

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
            if self.state_bits == 8:
                self._step8(g, self.current_lr(), self.step_count + 1, 1.0 / float(scale), scaler.flag)
            else:
                ops.adamw_step_guarded(self.p[:n], g[:n], self.m[:n], self.v[:n], self.p16[:n], self.current_lr(), self.betas[0],
                                       self.betas[1], self.eps, self.wd, self.step_count + 1, 1.0 / float(scale), scaler.flag)
            return scaler.verdict
        if not checked and not bool(torch.isfinite(g).all()):
            return False
        lr = self.current_lr()
        self.step_count += 1
        n = self.n_opt
        if self.state_bits == 8:
            self._step8(g, lr, self.step_count, 1.0 / self.grad_scale, None)
        else:
            ops.adamw_step(self.p[:n], g[:n], self.m[:n], self.v[:n], self.p16[:n], lr, self.betas[0], self.betas[1], self.eps,
                           self.wd, self.step_count, 1.0 / self.grad_scale)
        self.stale = True
        return True

    def _step8(self, g: torch.Tensor, lr: float, step: int, inv_scale: float, flag) -> None:
        n = self.n_opt
        if self.rows.shape[0] == 0:                               # everything frozen: nothing to step
            return
        ops.adamw8_step(self.p[:n], g[:n], self.p16[:n], self.state1, self.state2, self.absmax1, self.absmax2, self.m32, self.v32,
                        self.rows, self.qtab, lr, self.betas[0], self.betas[1], self.eps, self.wd, step, inv_scale, flag)

    def settle(self, stepped: bool) -> None:
        """The scaler's verdict on the guarded step queued by step(scaler=): only a step that ran counts (and leaves packs stale)."""
        if stepped:
            self.step_count += 1
            self.stale = True

    def state_dict(self, keys: Optional[Iterable[str]] = None) -> Dict[str, torch.Tensor]:
        """Clones of the fp32 masters under their keys, in the order of `keys` (default: the vector's)."""
        return {k: self.w32(k).clone() for k in (self.layout if keys is None else keys)}

    # ------------------------------------------------------------------------------------------ optimizer state
    def _opt_keys(self):
        return [k for k, (o, shp) in self.layout.items() if o < self.n_opt and shp.numel() > 0]

    def state_bytes(self) -> int:
        """Bytes of what the optimizer keeps beside the masters and their fp16 copy: m / v, or codes, absmax, the small tensors' fp32
        moments and the maps with their thresholds (the block table, 32 bytes per row, is layout and not counted)."""
        held = (self.m, self.v) if self.state_bits == 32 else (self.state1, self.state2, self.absmax1, self.absmax2, self.m32,
                                                               self.v32, self.qtab)
        return sum(t.numel() * t.element_size() for t in held)

    def optimizer_state_dict(self) -> dict:
        """{"step", "state_bits", "state": {key: moments}} for the optimised keys (the masters travel in state_dict()).  fp32 moments:
        exp_avg / exp_avg_sq in the tensor's shape.  8-bit: state1 / state2 (uint8, the tensor's shape) with absmax1 / absmax2 (one
        float per block of 2048), and the two maps once as qmap1 / qmap2.  Clones, on the optimizer's device."""
        out = {"step": self.step_count, "state_bits": self.state_bits, "state": {}}
        for k in self._opt_keys():
            o, shp = self.layout[k]
            n = shp.numel()
            if self.state_bits == 32:
                out["state"][k] = {"exp_avg": self.m[o:o + n].view(shp).clone(), "exp_avg_sq": self.v[o:o + n].view(shp).clone()}
                continue
            is8, so, r0, nr = self.spans[k]
            if is8:
                out["state"][k] = {"state1": self.state1[so:so + n].view(shp).clone(), "state2": self.state2[so:so + n].view(shp).clone(),
                                   "absmax1": self.absmax1[r0:r0 + nr].clone(), "absmax2": self.absmax2[r0:r0 + nr].clone()}
            else:
                out["state"][k] = {"exp_avg": self.m32[so:so + n].view(shp).clone(), "exp_avg_sq": self.v32[so:so + n].view(shp).clone()}
        if self.state_bits == 8:
            out["qmap1"], out["qmap2"] = self.qmap1.clone(), self.qmap2.clone()
        return out

    @torch.no_grad()
    def load_optimizer_state_dict(self, sd: dict) -> None:
        """What optimizer_state_dict() of an optimizer with the same state_bits, keys, shapes and min_8bit_size returned; anything
        else raises ValueError before a buffer is written."""
        if sd.get("state_bits") != self.state_bits:
            raise ValueError(f"optimizer state with state_bits = {sd.get('state_bits')} cannot be loaded into state_bits = "
                             f"{self.state_bits}: the two forms do not convert")
        keys = self._opt_keys()
        if list(sd["state"]) != keys:
            odd = sorted(set(sd["state"]) ^ set(keys))
            raise ValueError(f"optimizer state holds other keys than this optimizer: {odd[:4] if odd else 'same keys, other order'}")
        want = {}
        for k in keys:
            shp = self.layout[k][1]
            is8 = self.state_bits == 8 and self.spans[k][0]
            want[k] = {"state1": (torch.uint8, shp), "state2": (torch.uint8, shp), "absmax1": (torch.float32, (self.spans[k][3],)),
                       "absmax2": (torch.float32, (self.spans[k][3],))} if is8 else \
                {"exp_avg": (torch.float32, shp), "exp_avg_sq": (torch.float32, shp)}
            got = sd["state"][k]
            if set(got) != set(want[k]) or any(got[f].dtype != d or tuple(got[f].shape) != tuple(s) for f, (d, s) in want[k].items()):
                raise ValueError(f"optimizer state of {k}: expected {sorted(want[k])} of shape {tuple(shp)} (min_8bit_size = "
                                 f"{self.min_8bit_size}), found {({f: tuple(t.shape) for f, t in got.items()})}")
        if self.state_bits == 8 and not (torch.equal(sd["qmap1"].cpu(), self.qmap1) and torch.equal(sd["qmap2"].cpu(), self.qmap2)):
            raise ValueError("optimizer state was quantised with other maps than this optimizer's")
        for k in keys:
            o, shp = self.layout[k]
            n, got = shp.numel(), sd["state"][k]
            put = lambda vec, at, f, cnt: vec[at:at + cnt].copy_(got[f].reshape(-1))
            if self.state_bits == 32:
                put(self.m, o, "exp_avg", n), put(self.v, o, "exp_avg_sq", n)
                continue
            is8, so, r0, nr = self.spans[k]
            if is8:
                put(self.state1, so, "state1", n), put(self.state2, so, "state2", n)
                put(self.absmax1, r0, "absmax1", nr), put(self.absmax2, r0, "absmax2", nr)
            else:
                put(self.m32, so, "exp_avg", n), put(self.v32, so, "exp_avg_sq", n)
        self.step_count = int(sd["step"])
