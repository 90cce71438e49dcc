"""What the two CLIP towers (clip_text.py, clip_vision.py) share: the transformer layer stack, the per-layer weight pack, the
accessors a pack is read through, and the checkpoint / device plumbing of the two transformers-style facades.
"""
from __future__ import annotations

import os
from typing import Callable, Dict, List, Optional, Tuple

import torch

from . import ops
from .packs import _h


def _round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def strip_prefix(sd: Dict[str, torch.Tensor], prefix: str) -> Dict[str, torch.Tensor]:
    """transformers 4.x prefixes a tower's keys (``text_model.`` / ``vision_model.``); 5.x does not.  Both load."""
    return {(k[len(prefix):] if k.startswith(prefix) else k): v for k, v in sd.items()}


def state_dict_accessors(sd: Dict[str, torch.Tensor], dev) -> Tuple[Callable, Callable]:
    """(h16, f32) of an inference tower: key -> the state dict's tensor as fp16 on the device / as fp32 where it lies.  The fused
    ``...self_attn.qkv.weight`` / ``.bias`` keys concatenate q_proj, k_proj, v_proj.  (A training tower passes its trainer's
    w16 / w32 instead: views of the working copy and of the masters, the fused keys included.)"""
    def f32(key: str) -> torch.Tensor:
        if ".self_attn.qkv." in key:
            return torch.cat([sd[key.replace("qkv", n)].detach().float() for n in ("q_proj", "k_proj", "v_proj")])
        return sd[key].detach().float()
    return (lambda key: _h(f32(key), dev)), f32


def pack_layers(W: Dict[str, torch.Tensor], h16: Callable, num_layers: int) -> None:
    """The per-layer part of a tower's pack: q | k | v as one [3D, D] operand (+ bias) and the five sub-modules."""
    for l in range(num_layers):
        p = f"encoder.layers.{l}"
        W[p + ".qkv.weight"], W[p + ".qkv.bias"] = h16(p + ".self_attn.qkv.weight"), h16(p + ".self_attn.qkv.bias")
        for n in ("self_attn.out_proj", "mlp.fc1", "mlp.fc2", "layer_norm1", "layer_norm2"):
            W[f"{p}.{n}.weight"], W[f"{p}.{n}.bias"] = h16(f"{p}.{n}.weight"), h16(f"{p}.{n}.bias")


def encoder_layers(x: torch.Tensor, W: Dict[str, torch.Tensor], cfg, B: int, Lp: int, N: int, act: Callable, causal: bool,
                   stash: Optional[List[dict]] = None) -> torch.Tensor:
    """The layer stack of either tower on x fp16 [B * Lp, D] (N of every Lp rows are keys).  Eight launches per layer:
    LN1 -> fused q|k|v GEMM -> attention -> out_proj + residual -> LN2 -> fc1 -> act -> fc2 + residual.
    causal=True (text): the causal kernel on the transposed V columns (one ops.transpose more); False (vision): row-major V.
    stash: a list that gets one dict per layer (x1 s1 h1 qkv a lse x2 s2 h2 f act) for HipCLIPVision.backward; the LayerNorms then
    also return (mean, rstd), attention returns lse and the activation writes out of place so that f survives.  These switches
    change no bits of x.  Without a stash the activation runs in place."""
    D, H, eps = cfg.hidden_size, cfg.num_attention_heads, cfg.layer_norm_eps
    d, keep = D // H, stash is not None
    pair = (lambda r: r) if keep else (lambda r: (r, None))
    form = dict(causal=True) if causal else dict(v_rows=True)
    for l in range(cfg.num_hidden_layers):
        p = f"encoder.layers.{l}"
        h1, s1 = pair(ops.layernorm(x, W[p + ".layer_norm1.weight"], W[p + ".layer_norm1.bias"], eps, want_stats=keep))
        qkv = ops.gemm(h1, W[p + ".qkv.weight"], bias=W[p + ".qkv.bias"])
        v = ops.transpose(qkv[:, 2 * D:]) if causal else qkv[:, 2 * D:]
        # a is both out_proj's operand and the attention output O that the backward's delta = rowsum(dO . O) needs
        a, lse = pair(ops.attn_fwd(qkv[:, :D], qkv[:, D:2 * D], v, B, H, Lp, N, Lp, d, d ** -0.5, want_lse=keep, **form))
        x2 = ops.gemm(a, W[p + ".self_attn.out_proj.weight"], bias=W[p + ".self_attn.out_proj.bias"], residual=x)
        h2, s2 = pair(ops.layernorm(x2, W[p + ".layer_norm2.weight"], W[p + ".layer_norm2.bias"], eps, want_stats=keep))
        f = ops.gemm(h2, W[p + ".mlp.fc1.weight"], bias=W[p + ".mlp.fc1.bias"])
        g = act(f, out=None if keep else f)
        if keep:
            stash.append(dict(x1=x, s1=s1, h1=h1, qkv=qkv, a=a, lse=lse, x2=x2, s2=s2, h2=h2, f=f, act=g))
        x = ops.gemm(g, W[p + ".mlp.fc2.weight"], bias=W[p + ".mlp.fc2.bias"], residual=x2)
    return x


class CLIPFacade:
    """What CLIPTextModel and CLIPVisionModel share of transformers' surface: ``state_dict`` / ``load_state_dict(sd)``,
    ``.to(device)``, ``.eval()``, ``.device`` / ``.dtype`` / ``.config``.  A subclass sets ENGINE (the Hip* class that runs the
    tower, built by the first ``.to('cuda')``), PREFIX (transformers 4.x's key prefix) and WHAT (its name in the error below)."""
    ENGINE: Callable = None
    PREFIX = WHAT = ""

    def __init__(self, cfg, state_dict: Optional[Dict[str, torch.Tensor]], synthetic_sd: Callable):
        self.cfg = self.config = cfg
        self._sd = strip_prefix(state_dict, self.PREFIX) if state_dict is not None else synthetic_sd(cfg)
        self._hip = None
        self.device, self.dtype = torch.device("cpu"), torch.float16

    @staticmethod
    def read_folder(path: Optional[str]) -> Optional[Dict[str, torch.Tensor]]:
        """The tensors of ``model.safetensors`` or ``pytorch_model.bin`` in a checkpoint folder; None when there is neither."""
        if path and os.path.isdir(path):
            st, pt = os.path.join(path, "model.safetensors"), os.path.join(path, "pytorch_model.bin")
            if os.path.exists(st):
                from safetensors.torch import load_file
                return load_file(st)
            if os.path.exists(pt):
                return torch.load(pt, map_location="cpu")
        return None

    def state_dict(self):
        return self._sd

    def load_state_dict(self, sd, strict: bool = True):
        sd = strip_prefix(sd, self.PREFIX)
        missing = [k for k in self._sd if k not in sd and "position_ids" not in k]
        if strict and missing:
            raise RuntimeError(f"{type(self).__name__}.load_state_dict: missing keys {missing[:4]} ...")
        self._sd = {k: v for k, v in sd.items() if "position_ids" not in k}
        if self._hip is not None:
            self._hip = self.ENGINE(self.cfg, self._sd, self.device)
        return self

    def to(self, device=None, dtype=None):
        if isinstance(device, torch.dtype):
            device, dtype = None, device
        if device is not None:
            self.device = torch.device(device)
            if self.device.type == "cuda":
                if self._hip is None:
                    self._hip = self.ENGINE(self.cfg, self._sd, self.device)
                else:
                    self._hip.to(self.device)
        return self

    def eval(self):
        return self

    def engine(self):
        if self._hip is None:
            raise RuntimeError(f"{type(self).__name__}: call .to('cuda') first - {self.WHAT} runs on libskg.so kernels only")
        return self._hip
