"""ControlNet conditioning (diffusers ControlNetModel) on the libskg.so kernels: the weights' facade, the trunk, the hint
encoder and what the sampler carries through a trajectory.

A ControlNet is the UNet's encoder - conv_in, the down blocks, the mid block - on weights of its own, fed with the noisy latents
plus an encoding of a control image (a line drawing, a scribble, canny edges).  Each of its n + 1 feature maps goes through a
1x1 "zero convolution" and is added to the matching skip of the main UNet (the last one to the mid block's output), times the
conditioning scale.  Here:

  * ``ControlNetModel``   reads / validates a diffusers-layout checkpoint (``from_pretrained``), copies a UNet (``from_unet``), or
                          draws seeded synthetic weights (``from_pretrained(None, unet_config=...)``, the explicit opt-in);
  * ``HipControlNet``     the engine: a ``HipUNet(need_backward=False)`` over the encoder keys whose walk is ``down_only`` continued
                          through ``mid_block`` (all fp16, whatever the main UNet's mode), the hint encoder (csrc/condembed.hip for
                          the three pixel-resolution layers, the implicit GEMM + SiLU for the other five), the zero convolutions'
                          weights as ``HipUNet.forward(control=)`` takes them;
  * ``Control``           one call's conditioning: net, hint rows, scale and the step window (``HipSampler.sample(control=)``).

The key layout follows diffusers' ``ControlNetModel.state_dict()`` as its source spells it.  No real checkpoint was available
where this was written: the layout is checked against that list of names and shapes only.
"""
from __future__ import annotations

import json
import os
from types import SimpleNamespace
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import ops, synthetic
from .config import UNetConfig
from .packs import _h, pack_conv, pack_conv_small

ENCODER_PREFIXES = ("conv_in", "time_embedding", "down_blocks", "mid_block")
EMBED = "controlnet_cond_embedding"


def check_cond_channels(cc: Sequence[int]) -> Tuple[int, ...]:
    """conditioning_embedding_out_channels this implementation covers: four entries; the pixel-resolution layers are the
    small-channel kernel's (16 -> 16 -> 32), the rest the implicit GEMM's (multiples of 32)."""
    cc = tuple(int(c) for c in cc)
    if len(cc) != 4:
        raise NotImplementedError(f"conditioning_embedding_out_channels {cc}: four entries (diffusers' default (16, 32, 96, 256)) expected")
    if cc[0] != 16 or cc[1] != 32 or cc[2] % 32 or cc[3] % 32:
        raise NotImplementedError(f"conditioning_embedding_out_channels {cc}: (16, 32, multiples of 32) is what the hint encoder's kernels take")
    return cc


def _controlnet_config(c: dict) -> Tuple[UNetConfig, Tuple[int, ...]]:
    """(UNetConfig, conditioning_embedding_out_channels) of a ControlNetModel config.json; fields that change the graph and are
    not covered are rejected, never ignored."""
    from .modules.pipeline import _config_from_json
    unsupported = []
    for k, ok in (("global_pool_conditions", False), ("class_embed_type", None), ("addition_embed_type", None),
                  ("conditioning_channels", 3), ("controlnet_conditioning_channel_order", "rgb"), ("num_class_embeds", None)):
        if c.get(k, ok) != ok:
            unsupported.append(f"{k}={c.get(k)!r}")
    if unsupported:
        raise NotImplementedError("controlnet config.json asks for features this package does not implement: " + "; ".join(unsupported))
    cc = check_cond_channels(c.get("conditioning_embedding_out_channels", synthetic.COND_EMBED_CHANNELS))
    return _config_from_json(c, "controlnet config.json"), cc


def _validate(sd: Dict[str, torch.Tensor], cfg: UNetConfig, cc: Tuple[int, ...], what: str):
    want = synthetic.controlnet_param_shapes(cfg, cc)
    missing = [k for k in want if k not in sd]
    extra = [k for k in sd if k not in want]
    wrong = [k for k in want if k in sd and tuple(sd[k].shape) != tuple(want[k])
             and tuple(sd[k].shape) != tuple(want[k]) + (1, 1) and tuple(sd[k].shape) + (1, 1) != tuple(want[k])]
    if missing or wrong or extra:
        raise ValueError(f"{what}: the checkpoint does not match the ControlNet of {cfg}: {len(missing)} missing keys (e.g. "
                         f"{missing[:3]}), {len(wrong)} shape mismatches (e.g. {wrong[:3]}), {len(extra)} unexpected keys (e.g. {extra[:3]})")


class ControlNetModel:
    """Stands where diffusers' ``ControlNetModel`` is: ``from_pretrained`` / ``from_unet``, ``.to()``, ``.state_dict()``,
    ``.config``, plus the engine (``.hip``)."""

    def __init__(self, cfg: UNetConfig, state_dict: Dict[str, torch.Tensor], device="cpu",
                 cond_channels: Tuple[int, ...] = synthetic.COND_EMBED_CHANNELS):
        self.cfg, self.cond_channels = cfg, check_cond_channels(cond_channels)
        _validate(state_dict, cfg, self.cond_channels, "ControlNetModel")
        self.config = SimpleNamespace(in_channels=cfg.in_channels, cross_attention_dim=cfg.cross_attention_dim,
                                      block_out_channels=tuple(cfg.block_out_channels), layers_per_block=cfg.layers_per_block,
                                      conditioning_channels=3, conditioning_embedding_out_channels=self.cond_channels,
                                      global_pool_conditions=False)
        self.dtype = torch.float16
        self._state_dict = state_dict
        self._device = torch.device(device)
        self._hip: Optional[HipControlNet] = None

    @classmethod
    def from_pretrained(cls, folder: Optional[str] = None, unet_config: Optional[UNetConfig] = None, torch_dtype=None, **kwargs):
        """``folder``: a local diffusers-layout ControlNet folder - ``config.json`` and ``diffusion_pytorch_model{,.fp16}.safetensors``
        or ``.bin``.  ``None`` (with ``unet_config``, default SD1.5) is the explicit opt-in to seeded synthetic weights, whose zero
        convolutions are not zero.  A path that does not resolve to weights raises."""
        if folder is None:
            from .config import SD15
            cfg = unet_config or SD15
            return cls(cfg, synthetic.controlnet_state_dict(cfg))
        from .modules.pipeline import load_diffusers_weights
        sd = load_diffusers_weights(str(folder), "ControlNetModel.from_pretrained")
        cj = os.path.join(str(folder), "config.json")
        if os.path.exists(cj):
            cfg, cc = _controlnet_config(json.load(open(cj)))
        else:
            from .config import SD15
            cfg, cc = unet_config or SD15, synthetic.COND_EMBED_CHANNELS
        if unet_config is not None and unet_config != cfg:
            raise ValueError(f"ControlNetModel.from_pretrained: config.json describes {cfg}, unet_config= is {unet_config}")
        return cls(cfg, sd, cond_channels=cc)      # (validates the key set and every shape)

    @classmethod
    def from_unet(cls, unet, conditioning_embedding_out_channels: Sequence[int] = synthetic.COND_EMBED_CHANNELS,
                  seed: int = synthetic.CONTROLNET_WEIGHT_SEED):
        """diffusers' constructor of that name: the UNet's encoder weights copied, every zero convolution zero - the net then
        changes nothing until it is trained -, the hint encoder seeded random.  ``unet``: ``pipe.unet`` (anything with ``.cfg`` and
        ``.state_dict()``)."""
        cfg, cc = unet.cfg, check_cond_channels(conditioning_embedding_out_channels)
        src = unet.state_dict()
        rnd = synthetic.controlnet_state_dict(cfg, seed, cc)
        sd = {}
        for k, v in rnd.items():
            if k.split(".")[0] in ENCODER_PREFIXES:
                sd[k] = src[k].detach().clone()
            elif k.startswith("controlnet_down_blocks.") or k.startswith("controlnet_mid_block."):
                sd[k] = torch.zeros_like(v)
            else:
                sd[k] = v
        return cls(cfg, sd, getattr(unet, "device", "cpu"), cc)

    @property
    def device(self):
        return self._device

    def to(self, device=None, dtype=None):
        if device is not None and torch.device(device) != self._device:
            self._device, self._hip = torch.device(device), None
        return self

    def state_dict(self):
        return self._state_dict

    @property
    def hip(self) -> "HipControlNet":
        if self._hip is None:
            if self._device.type != "cuda":
                raise RuntimeError("sketch2img_amd computes on the GPU only: call controlnet.to('cuda') first")
            self._hip = HipControlNet(self.cfg, self._state_dict, self._device, self.cond_channels)
        return self._hip


class HipControlNet:
    """The engine of one ControlNet on one device."""

    def __init__(self, cfg: UNetConfig, state_dict: Dict[str, torch.Tensor], device="cuda",
                 cond_channels: Tuple[int, ...] = synthetic.COND_EMBED_CHANNELS):
        from .unet import HipUNet
        self.cfg, self.dev = cfg, torch.device(device)
        self.cond_channels = check_cond_channels(cond_channels)
        sd = state_dict
        # the trunk: all fp16 (the default representation) whatever the main UNet's mode, forward only
        self.trunk = HipUNet(cfg, {k: v for k, v in sd.items() if k.split(".")[0] in ENCODER_PREFIXES}, self.dev,
                             need_backward=False, residual_fp32=False)
        dev = self.dev
        # hint encoder: (pack, bias, stride, small-channel kernel?) per layer, SiLU behind every one but the last
        names = ["conv_in"] + [f"blocks.{i}" for i in range(6)] + ["conv_out"]
        self.embed_layers: List[Tuple[torch.Tensor, torch.Tensor, int, bool]] = []
        for li, n in enumerate(names):
            w, b = sd[f"{EMBED}.{n}.weight"], sd[f"{EMBED}.{n}.bias"]
            small = li < 3
            stride = 2 if li in (2, 4, 6) else 1
            self.embed_layers.append((pack_conv_small(w, dev) if small else pack_conv(w, dev), _h(b, dev), stride, small))
        n = synthetic.controlnet_num_residuals(cfg)
        zc = [(sd[f"controlnet_down_blocks.{k}.weight"], sd[f"controlnet_down_blocks.{k}.bias"]) for k in range(n)]
        zc.append((sd["controlnet_mid_block.weight"], sd["controlnet_mid_block.bias"]))
        self.zero_convs = [(_h(w.reshape(w.shape[0], w.shape[1]), dev), _h(b, dev)) for w, b in zc]

    # -------------------------------------------------------------- hoisted precompute (the trunk's own, as HipUNet's)
    def prepare_context(self, ehs: torch.Tensor):
        self.trunk.prepare_context(ehs)

    def prepare_timesteps(self, timesteps: Sequence[int]):
        self.trunk.prepare_timesteps(timesteps)

    @property
    def ctx(self):
        return self.trunk.ctx

    # -------------------------------------------------------------- hint encoder
    @torch.no_grad()
    def embed(self, image: torch.Tensor) -> torch.Tensor:
        """Control image, fp32 [B, 3, height, width] in [0, 1] (both sides multiples of 8) -> fp16 NHWC [B*(height/8)*(width/8), C0]:
        ControlNetConditioningEmbedding - conv_in, six blocks (every second one stride 2), conv_out; SiLU behind all but the last."""
        if image.dim() != 4 or image.shape[1] != 3 or image.shape[2] % 8 or image.shape[3] % 8 or not image.is_floating_point():
            raise ValueError(f"control image: a float tensor [B, 3, height, width] with sides multiples of 8 expected, got {tuple(image.shape)}")
        x = image.to(self.dev, torch.float32).contiguous()
        B, _, H, W = x.shape
        last = len(self.embed_layers) - 1
        for li, (wp, b, stride, small) in enumerate(self.embed_layers):
            if small:
                x = ops.conv3x3_small(x, wp, B, H, W, stride, bias=b, silu=True)
            else:
                x = ops.conv3x3(x, wp, B, H, W, ops.CONV_S2 if stride == 2 else ops.CONV_S1, bias=b)
                if li != last:
                    ops.silu(x, out=x)
            if stride == 2:
                H, W = H // 2, W // 2
        return x

    def hint_rows(self, hint: torch.Tensor, images: int, rows: int) -> torch.Tensor:
        """The encoder's output for `images` control images -> the trunk's `hint` for `rows` batch rows: image s (the one image,
        when there is one) at every row r with r % S == s - the rows are [uncond rows of all samples ; cond rows of all samples], or
        the S cond rows alone."""
        per = hint.shape[0] // images
        S = images if images > 1 else 1
        if rows % S:
            raise ValueError(f"{images} control images for {rows} batch rows")
        h3 = hint.view(images, per, hint.shape[1])
        full = h3.repeat(rows // S, 1, 1) if images > 1 else h3.expand(rows, -1, -1)
        return full.reshape(rows * per, hint.shape[1]).contiguous()

    # -------------------------------------------------------------- trunk
    @torch.no_grad()
    def forward(self, x32: torch.Tensor, t, rows: int, H: int, W: Optional[int], hint: torch.Tensor) -> List[torch.Tensor]:
        """x32: the main UNet's input (fp16 [rows*H*W, CIN_PAD], all rows: no shared CFG front), hint [rows*H*W, C0] ->
        the n + 1 features (n skips in production order, then the mid block's output) the zero convolutions read."""
        W = H if W is None else W
        if tuple(hint.shape) != (rows * H * W, self.cfg.block_out_channels[0]):
            raise ValueError(f"hint {tuple(hint.shape)}: [{rows * H * W}, {self.cfg.block_out_channels[0]}] expected - the control image "
                             f"has to be 8x the latents' {H} x {W}")
        skips, mid = self.trunk.forward(x32, t, rows, H, want_taps=False, want_eps=False, down_only=True, through_mid=True,
                                        hint=hint, W=W)
        return skips + [mid]


class Control:
    """One call's conditioning, as HipSampler.sample(control=) takes it: the engine (its context prepared for the call's rows),
    the hint for all rows, the conditioning scale and diffusers' step window [start, end] in fractions of the executed steps."""

    def __init__(self, net: HipControlNet, hint: torch.Tensor, scale: float = 1.0, start: float = 0.0, end: float = 1.0):
        self.net, self.hint, self.scale, self.start, self.end = net, hint, float(scale), float(start), float(end)

    def active(self, n: int, N: int) -> bool:
        """diffusers' controlnet_keep for executed step n of N: 1 - (n / N < start or (n + 1) / N > end)."""
        return not (n / N < self.start or (n + 1) / N > self.end)

    def key(self) -> tuple:
        return ("controlled", self.scale, self.start, self.end, tuple(self.hint.shape))

    def with_hint(self, hint: torch.Tensor) -> "Control":
        return Control(self.net, hint, self.scale, self.start, self.end)
