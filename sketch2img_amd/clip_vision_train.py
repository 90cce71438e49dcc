"""Optimizer state of the CLIP vision tower for the SatMixin training step (reference trainer: modules/clip_guided_trainer.py:116-119
puts ``sketch_encoder.parameters()`` into the same optimizer as the 16 injected modules; :264 saves it as sketch_encoder_model.pt).

HipClipTowerTrainer is a flat_adamw.FlatAdamW (flat fp32 master vector, its fp16 working copy, AdamW's m / v) that drives
clip_vision.HipCLIPVision.forward_train / backward on views of the working copy.  Same hyper-parameters and the same
cosine_with_restarts schedule as sat_train.HipSatTrainer (one optimizer in the reference); sat_train.train_step(tower=...) steps both
or neither.

Layout: transformers' tensors, every one 16-byte aligned in the fp16 copy, with q_proj / k_proj / v_proj of a layer adjacent (weights,
then biases) so that the fused [3D, D] / [3D] operands of the forward and ONE wgrad launch of the backward are plain views;
state_dict() hands the three back under their own names.  ``post_layernorm.*`` sits behind the optimised part of the vector (elements >= n_opt):
last_hidden_state never reads it, so nothing writes its gradient slots, and torch's AdamW skips a parameter whose gradient is None -
weight decay included - so step() updates the first n_opt elements only.  It passes through state_dict() unchanged.

Seam scale: d loss / d sketch_state arrives as fp32 x sat_train.LOSS_SCALE and is cast to fp16 for the tower's backward.  SEAM_SCALE is
the extra power of two applied at that cast and divided out again through adamw_step's inv_grad_scale (DESIGN.md section 12,
tools/clip_loss_scale.py, profiles/clip_loss_scale.txt).
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import torch

from .clip_vision import HipCLIPVision, strip_prefix
from .config import CLIPVisionConfig
from .flat_adamw import FlatAdamW, cosine_with_restarts
from .sat_train import LOSS_SCALE
from .synthetic import clip_vision_param_shapes

# 2^8 on top of LOSS_SCALE = 2^13.  profiles/clip_loss_scale.txt: at the 16 x 16, B = 2 test size the tower's gradients are flat from
# 2^0 to 2^15 and overflow at 2^18; SD1.5's 4 x 4 x 64 x 64 batch seeds the backward 2^5 lower, so there the plateau is 2^5 .. 2^20 and
# factor 1 falls off it (it is 2^-5 here: between the 2^-6 row, 8 of 65 tensors over 1 %, and the 2^-3 row, worst 3.4e-3).  2^8 is 2^3
# above the lower edge at SD1.5's size and 2^7 below the upper edge at the test size.
SEAM_SCALE = 256.0
_FROZEN = ("post_layernorm.weight", "post_layernorm.bias")


def flat_order(cfg: CLIPVisionConfig):
    """Key order of the flat vector: the state dict's, except that every layer starts with q / k / v weights, then q / k / v biases
    (so the fused operands are views); post_layernorm.* comes last, behind what the optimizer updates."""
    keys = ["embeddings.class_embedding", "embeddings.patch_embedding.weight", "embeddings.position_embedding.weight",
            "pre_layrnorm.weight", "pre_layrnorm.bias"]
    for l in range(cfg.num_hidden_layers):
        p = f"encoder.layers.{l}"
        keys += [f"{p}.self_attn.{n}.{t}" for t in ("weight", "bias") for n in ("q_proj", "k_proj", "v_proj")]
        keys += [f"{p}.{n}.{t}" for n in ("self_attn.out_proj", "layer_norm1", "mlp.fc1", "mlp.fc2", "layer_norm2")
                 for t in ("weight", "bias")]
    return keys + list(_FROZEN)


class HipClipTowerTrainer(FlatAdamW):
    def __init__(self, cfg: CLIPVisionConfig, state_dict: Dict[str, torch.Tensor], device="cuda", lr: float = 2e-4,
                 betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2, warmup_steps: int = 150,
                 total_steps: int = 10000, num_cycles: int = 1, seam_scale: float = SEAM_SCALE, state_bits: int = 32,
                 min_8bit_size: int = 4096):
        # state_bits / min_8bit_size: FlatAdamW's (8: block-wise quantised m / v, the reference's AdamW8bit)
        self.cfg = cfg
        self.seam_scale = float(seam_scale)
        assert math.frexp(self.seam_scale)[0] == 0.5, "the seam scale must be a power of two"
        D = cfg.hidden_size
        assert D % 8 == 0, "q / k / v must stay adjacent: hidden_size % 8 == 0"
        shapes = clip_vision_param_shapes(cfg)
        super().__init__([(k, shapes[k]) for k in flat_order(cfg)], strip_prefix(state_dict), device, lr, betas, eps, weight_decay,
                         lambda s: cosine_with_restarts(s, warmup_steps, total_steps, num_cycles),
                         LOSS_SCALE * self.seam_scale, frozen=_FROZEN, state_bits=state_bits, min_8bit_size=min_8bit_size)
        # the fused views: q, k, v of a layer are adjacent and unpadded (D * D and D are multiples of 8)
        self.fused: Dict[str, Tuple[int, torch.Size]] = {}
        for l in range(cfg.num_hidden_layers):
            p = f"encoder.layers.{l}.self_attn"
            self.fused[p + ".qkv.weight"] = (self.layout[p + ".q_proj.weight"][0], torch.Size((3 * D, D)))
            self.fused[p + ".qkv.bias"] = (self.layout[p + ".q_proj.bias"][0], torch.Size((3 * D,)))
        self.vision: Optional[HipCLIPVision] = None        # built (packs and all) by the first forward_train

    def _at(self, key: str) -> Tuple[int, torch.Size]:
        return self.layout[key] if key in self.layout else self.fused[key]

    # ------------------------------------------------------------------------------------------ fwd + bwd
    def forward_train(self, pixel_values: torch.Tensor):
        """-> (sketch tokens fp16 [B, N, D], what backward consumes)."""
        self.refresh()
        return self.vision.forward_train(pixel_values)

    def refresh(self) -> None:
        """Bring what the tower derives from the working copy up to date (its padded and transposed packs): a no-op unless an
        optimizer step has run since the last call (FlatAdamW.stale).  forward_train calls it; a caller may do so earlier, after
        step()."""
        if self.vision is None:
            self.vision = HipCLIPVision(self.cfg, None, self.dev, views=(self.w16, self.w32, self.grad_view))
        elif self.stale:
            self.vision.refresh()
        self.stale = False

    def backward(self, kept: dict, d_tokens: torch.Tensor, g: torch.Tensor) -> None:
        """d_tokens fp16 [B, N, D], scaled by LOSS_SCALE * seam_scale -> += into the flat fp32 gradient g (same scale)."""
        self.vision.backward(kept, d_tokens, g)

    def seam(self, dstate: torch.Tensor) -> torch.Tensor:
        """d loss / d sketch_state fp32 (x LOSS_SCALE) -> the fp16 seed of the tower's backward (x LOSS_SCALE * seam_scale)."""
        return (dstate * self.seam_scale).to(torch.float16)

    # ------------------------------------------------------------------------------------------ optimizer
    # FlatAdamW.step as it is: g carries LOSS_SCALE * seam_scale (under a scaler: the scaler's scale at the seed x seam_scale), AdamW
    # runs on [0, n_opt), and a step that ran leaves the tower's packs stale
    def state_dict(self) -> Dict[str, torch.Tensor]:
        """The reference's sketch_encoder_model.pt: fp32 masters under transformers' CLIPVisionModel keys, in its order."""
        return super().state_dict(clip_vision_param_shapes(self.cfg))
