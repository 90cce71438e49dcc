"""CPU restatement of diffusers' ControlNetModel, composed from oracle.unet's own functions.  TEST INFRASTRUCTURE.

ControlNet is not part of the reference project; what is restated here is diffusers' `ControlNetModel.forward` and the way
`UNet2DConditionModel.forward` consumes `down_block_additional_residuals` / `mid_block_additional_residual`:

  * `cond_embedding`       ControlNetConditioningEmbedding: conv_in, six blocks (every second one stride 2), conv_out, SiLU behind
                           all but the last (`round_fp16=True`: every layer's output rounded to fp16 - what any implementation that
                           stores fp16 between the layers pays);
  * `controlnet_forward`   time embedding, conv_in(x) + hint, the down blocks, the mid block, the zero convolutions -> the n + 1
                           residuals (n skips in production order, then mid);
  * `unet_forward_controlled`   oracle.unet.unet_forward's twin: residual k times the scale is added to skip k, the last one to `h`
                           behind the mid block.  With all-zero residuals it IS unet_forward, bit for bit.
Weights are flat dicts with the diffusers key names (sketch2img_amd.synthetic.controlnet_state_dict)."""
from typing import Dict, List, Sequence

import torch
import torch.nn.functional as F

from oracle.unet import _gn, _r, resnet_forward, timestep_embedding, transformer2d_forward

EMBED = "controlnet_cond_embedding"
EMBED_LAYERS = ["conv_in"] + [f"blocks.{i}" for i in range(6)] + ["conv_out"]
EMBED_STRIDES = [1, 1, 2, 1, 2, 1, 2, 1]


def cond_embedding(W: Dict[str, torch.Tensor], image: torch.Tensor, round_fp16: bool = False) -> torch.Tensor:
    """image [B, 3, H, W] in [0, 1] -> [B, C0, H/8, W/8]."""
    rnd = (lambda v: v.half().float()) if round_fp16 else (lambda v: v)
    h = rnd(image.float())
    for li, (n, s) in enumerate(zip(EMBED_LAYERS, EMBED_STRIDES)):
        h = F.conv2d(h, W[f"{EMBED}.{n}.weight"], W[f"{EMBED}.{n}.bias"], stride=s, padding=1)
        if li != len(EMBED_LAYERS) - 1:
            h = F.silu(h)
        h = rnd(h)
    return h


def _temb_act(cfg, W, x, t):
    tt = torch.as_tensor(t).reshape(-1).expand(x.shape[0])
    temb = _r(timestep_embedding(tt, cfg.block_out_channels[0]).to(x.dtype), "temb")
    temb = _r(F.linear(temb, W["time_embedding.linear_1.weight"], W["time_embedding.linear_1.bias"]), "temb")
    temb = _r(F.linear(_r(F.silu(temb), "temb"), W["time_embedding.linear_2.weight"], W["time_embedding.linear_2.bias"]), "temb")
    return _r(F.silu(temb), "temb")


def _down_path(cfg, W, h, temb_act, ehs, inject=None):
    """The down blocks from conv_in's output on -> (h, skips)."""
    nb = len(cfg.block_out_channels)
    skips = [h]
    for i in range(nb):
        for j in range(cfg.layers_per_block):
            h = resnet_forward(cfg, W, f"down_blocks.{i}.resnets.{j}", h, temb_act)
            if i < nb - 1:
                h = transformer2d_forward(cfg, W, f"down_blocks.{i}.attentions.{j}", h, ehs, cfg.num_heads[i], inject)
            skips.append(h)
        if i < nb - 1:
            p = f"down_blocks.{i}.downsamplers.0.conv"
            h = _r(F.conv2d(_r(h, "rop_dn"), W[p + ".weight"], W[p + ".bias"], stride=2, padding=1), "res")
            skips.append(h)
    return h, skips


def _mid(cfg, W, h, temb_act, ehs, inject=None):
    h = resnet_forward(cfg, W, "mid_block.resnets.0", h, temb_act)
    h = transformer2d_forward(cfg, W, "mid_block.attentions.0", h, ehs, cfg.num_heads[-1], inject)
    return resnet_forward(cfg, W, "mid_block.resnets.1", h, temb_act)


def controlnet_forward(cfg, Wc: Dict[str, torch.Tensor], x: torch.Tensor, t, ehs: torch.Tensor, hint: torch.Tensor,
                       zero_convs: bool = True) -> List[torch.Tensor]:
    """x [rows, 4, h, w], hint [rows, C0, h, w] (cond_embedding's output, rows repeated by the caller) -> the n + 1 residuals
    (zero_convs=False: the trunk's features in front of them)."""
    temb_act = _temb_act(cfg, Wc, x, t)
    h = F.conv2d(x, Wc["conv_in.weight"], Wc["conv_in.bias"], padding=1) + hint
    h, skips = _down_path(cfg, Wc, h, temb_act, ehs)
    feats = skips + [_mid(cfg, Wc, h, temb_act, ehs)]
    if not zero_convs:
        return feats
    n = len(skips)
    keys = [f"controlnet_down_blocks.{k}" for k in range(n)] + ["controlnet_mid_block"]
    return [F.conv2d(f, Wc[k + ".weight"].reshape(f.shape[1], f.shape[1], 1, 1), Wc[k + ".bias"]) for f, k in zip(feats, keys)]


def unet_forward_controlled(cfg, W: Dict[str, torch.Tensor], x: torch.Tensor, t, ehs: torch.Tensor,
                            residuals: Sequence[torch.Tensor], scale: float = 1.0) -> torch.Tensor:
    """oracle.unet.unet_forward with down_block_additional_residuals / mid_block_additional_residual = scale * residuals -> eps."""
    nb = len(cfg.block_out_channels)
    temb_act = _temb_act(cfg, W, x, t)
    h = _r(F.conv2d(_r(x, "res"), W["conv_in.weight"], W["conv_in.bias"], padding=1), "res")
    h, skips = _down_path(cfg, W, h, temb_act, ehs)
    assert len(residuals) == len(skips) + 1
    skips = [s + scale * r for s, r in zip(skips, residuals[:-1])]
    h = _mid(cfg, W, h, temb_act, ehs)
    h = h + scale * residuals[-1]
    rev_heads = tuple(reversed(cfg.num_heads))
    for i in range(nb):
        for j in range(cfg.layers_per_block + 1):
            h = torch.cat([h, skips.pop()], dim=1)
            h = resnet_forward(cfg, W, f"up_blocks.{i}.resnets.{j}", h, temb_act)
            if i > 0:
                h = transformer2d_forward(cfg, W, f"up_blocks.{i}.attentions.{j}", h, ehs, rev_heads[i])
        if i < nb - 1:
            p = f"up_blocks.{i}.upsamplers.0.conv"
            h = F.interpolate(h, scale_factor=2.0, mode="nearest")
            h = _r(F.conv2d(_r(h, "rop_up"), W[p + ".weight"], W[p + ".bias"], padding=1), "res")
    h = _r(F.silu(_gn(h, W, "conv_norm_out", cfg.norm_groups, 1e-5)), "norm")
    return _r(F.conv2d(h, W["conv_out.weight"], W["conv_out.bias"], padding=1), "res")


def controlled_eps(cfg, W, Wc, x, t, ehs, image, scale: float = 1.0) -> torch.Tensor:
    """The whole controlled evaluation: image [1 or S, 3, 8h, 8w] -> hint, repeated over the rows ([uncond ; cond] halves or the
    cond rows alone), trunk, zero convolutions, twin."""
    hint = cond_embedding(Wc, image)
    rows = x.shape[0]
    hint = hint.repeat(rows // hint.shape[0], 1, 1, 1)
    return unet_forward_controlled(cfg, W, x, t, ehs, controlnet_forward(cfg, Wc, x, t, ehs, hint), scale)
