"""CLIP vision tower (ViT) on the libskg.so kernels: the producer of the sketch tokens for the CLIP-guided variant.

Replaces ``CLIPVisionModel(...)(pixel_values, output_hidden_states=True).last_hidden_state`` at
modules/clip_guided_inf.py:49-54,103 (third-party transformers; restated and PINNED against transformers' own class in
oracle/clip_vision.py + tests/golden/clip_vision_tiny.npz).  Runs once per image; SURVEY.md section 8f rank 3.

Layout: tokens fp16 [B * Lp, D] with every image's 1 + g*g tokens padded to Lp = a multiple of 8 rows (257 -> 264) so
the transposed V panel keeps 16-byte aligned rows; pad rows are never read as keys (Nkv = 257) and are dropped at the
end.  Patch embedding = GEMM over the unfolded 14x14x3 patches (K = 588 zero-padded to 608), q/k/v fused into one GEMM
(with bias), flash attention (d = 64), out-proj / fc2 GEMMs with the residual in the epilogue, quick_gelu and LayerNorm
kernels.  The image pre-processing (CLIPImageProcessor: resize, crop, normalise) stays with the caller.
"""
from __future__ import annotations

import os
from typing import Dict, Optional

import torch

from . import ops
from .config import CLIPVisionConfig, VIT_L_14
from .unet import _h


def _round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def strip_prefix(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """transformers 4.x prefixes the tower's keys with ``vision_model.``; 5.x does not.  Both load."""
    return {(k[len("vision_model."):] if k.startswith("vision_model.") else k): v for k, v in sd.items()}


class HipCLIPVision:
    def __init__(self, cfg: CLIPVisionConfig, state_dict: Optional[Dict[str, torch.Tensor]], device="cuda", views=None):
        """state_dict: transformers' tensors, packed to fp16 once (inference).  For training pass state_dict=None and
        views=(w16, w32, grad_view) instead: w16(key) -> fp16 view of a trainer's working copy under transformers' key names,
        plus the fused ``encoder.layers.L.self_attn.qkv.weight`` [3D, D] / ``.qkv.bias`` [3D] (clip_vision_train.HipClipTowerTrainer
        lays q, k, v out contiguously); w32(key) -> the fp32 master of the same tensor; grad_view(flat, key) -> fp32 view of a flat
        gradient under the same names, as for inject.HipClipInjectorTrain.  refresh() after every optimizer step."""
        self.cfg, self.dev = cfg, torch.device(device)
        self.Lp = _round_up(cfg.num_tokens, 8)
        self.Kp = _round_up(3 * cfg.patch_size ** 2, 32)
        self.views = views
        if views is None:
            self.W = self._pack(strip_prefix(state_dict))
            self._pos_rep: Dict[int, torch.Tensor] = {}
        else:
            assert state_dict is None, "a training tower reads the trainer's working copy, not a state dict"
            self.w16, self.w32, self.grad_view = views
            self.refresh()

    def _pack(self, sd):
        cfg, dev = self.cfg, self.dev
        W: Dict[str, torch.Tensor] = {}
        D = cfg.hidden_size
        pe = sd["embeddings.patch_embedding.weight"].detach().float().reshape(D, -1)         # [D, 3*P*P] (c, y, x)
        W["patch"] = _h(torch.nn.functional.pad(pe, (0, self.Kp - pe.shape[1])), dev)
        pos = torch.zeros(self.Lp, D)
        pos[:cfg.num_tokens] = sd["embeddings.position_embedding.weight"].detach().float()
        pos[0] += sd["embeddings.class_embedding"].detach().float()                           # cls token + its position
        W["pos"] = _h(pos, dev)
        for k in ("pre_layrnorm.weight", "pre_layrnorm.bias"):
            W[k] = _h(sd[k].detach().float(), dev)
        for l in range(cfg.num_hidden_layers):
            p = f"encoder.layers.{l}"
            W[p + ".qkv.weight"] = _h(torch.cat([sd[f"{p}.self_attn.{n}.weight"].detach().float()
                                                 for n in ("q_proj", "k_proj", "v_proj")]), dev)
            W[p + ".qkv.bias"] = _h(torch.cat([sd[f"{p}.self_attn.{n}.bias"].detach().float()
                                               for n in ("q_proj", "k_proj", "v_proj")]), dev)
            for n in ("self_attn.out_proj", "mlp.fc1", "mlp.fc2", "layer_norm1", "layer_norm2"):
                W[f"{p}.{n}.weight"] = _h(sd[f"{p}.{n}.weight"].detach().float(), dev)
                W[f"{p}.{n}.bias"] = _h(sd[f"{p}.{n}.bias"].detach().float(), dev)
        return W

    def to(self, device):
        if torch.device(device) != self.dev:
            if self.views is not None:
                raise RuntimeError("HipCLIPVision: a training tower's weights are views of its trainer's vectors and cannot move")
            self.dev = torch.device(device)
            self.W = {k: v.to(self.dev) for k, v in self.W.items()}
            self._pos_rep = {}
        return self

    @torch.no_grad()
    def last_hidden_state(self, pixel_values: torch.Tensor) -> torch.Tensor:
        """pixel_values [B, 3, S, S] (already CLIP-normalised) -> fp16 [B, 1 + (S/P)^2, D]."""
        cfg, W = self.cfg, self.W
        B, _, S, S2 = pixel_values.shape
        P, D, H = cfg.patch_size, cfg.hidden_size, cfg.num_attention_heads
        if S != cfg.image_size or S2 != S:
            raise ValueError(f"CLIP vision tower expects {cfg.image_size}x{cfg.image_size} images, got {S}x{S2}")
        g, N, Lp, d = S // P, cfg.num_tokens, self.Lp, D // H
        # unfold the non-overlapping patches: pure data movement (no arithmetic) done with torch views
        x = pixel_values.to(self.dev, torch.float32).reshape(B, 3, g, P, g, P).permute(0, 2, 4, 1, 3, 5)
        cols = torch.zeros(B * g * g, self.Kp, device=self.dev, dtype=torch.float16)
        cols[:, :3 * P * P] = x.reshape(B * g * g, 3 * P * P)
        tok = torch.zeros(B, Lp, D, device=self.dev, dtype=torch.float16)
        emb = ops.gemm(cols, W["patch"])                                       # [B*g*g, D]
        tok[:, 1:N] = emb.view(B, g * g, D)
        if B not in self._pos_rep:
            self._pos_rep[B] = W["pos"].repeat(B, 1).contiguous()
        x = ops.axpby(tok.view(B * Lp, D), self._pos_rep[B])                   # + position (+ class) embedding
        x = ops.layernorm(x, W["pre_layrnorm.weight"], W["pre_layrnorm.bias"], cfg.layer_norm_eps)
        scale = d ** -0.5
        for l in range(cfg.num_hidden_layers):
            p = f"encoder.layers.{l}"
            h = ops.layernorm(x, W[p + ".layer_norm1.weight"], W[p + ".layer_norm1.bias"], cfg.layer_norm_eps)
            qkv = ops.gemm(h, W[p + ".qkv.weight"], bias=W[p + ".qkv.bias"])
            a = ops.attn_fwd(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], B, H, Lp, N, Lp, d, scale, v_rows=True)
            x = ops.gemm(a, W[p + ".self_attn.out_proj.weight"], bias=W[p + ".self_attn.out_proj.bias"], residual=x)
            h = ops.layernorm(x, W[p + ".layer_norm2.weight"], W[p + ".layer_norm2.bias"], cfg.layer_norm_eps)
            f = ops.gemm(h, W[p + ".mlp.fc1.weight"], bias=W[p + ".mlp.fc1.bias"])
            ops.quick_gelu(f, out=f)
            x = ops.gemm(f, W[p + ".mlp.fc2.weight"], bias=W[p + ".mlp.fc2.bias"], residual=x)
        return x.view(B, Lp, D)[:, :N].contiguous()

    # ---- training: the weights are views of a trainer's fp16 working copy ----------------------------------------------------------
    def refresh(self):
        """Rebuild what is derived from the working copy (once per optimizer step): the zero-padded patch pack, the position (+ class)
        rows, the repeated position buffer, and the transposed packs the data-gradient GEMMs read (ops.transpose)."""
        assert self.views is not None, "refresh() belongs to a training tower (views=...)"
        cfg, dev, w = self.cfg, self.dev, self.w16
        D = cfg.hidden_size
        W: Dict[str, torch.Tensor] = {}
        patch = torch.zeros(D, self.Kp, device=dev, dtype=torch.float16)
        patch[:, :3 * cfg.patch_size ** 2] = w("embeddings.patch_embedding.weight").reshape(D, -1)
        W["patch"] = patch
        # from the fp32 masters, as _pack does: row 0 = fp16(pos32[0] + class32), one rounding, so that an inference tower built from
        # the trainer's state_dict() gives the training forward's bits (rows >= 1 equal the working copy either way)
        pos = torch.zeros(self.Lp, D, device=dev, dtype=torch.float32)
        pos[:cfg.num_tokens] = self.w32("embeddings.position_embedding.weight")
        pos[0] += self.w32("embeddings.class_embedding")
        W["pos"] = pos.to(torch.float16)
        for k in ("pre_layrnorm.weight", "pre_layrnorm.bias"):
            W[k] = w(k)
        self.WT: Dict[str, torch.Tensor] = {}
        for l in range(cfg.num_hidden_layers):
            p = f"encoder.layers.{l}"
            W[p + ".qkv.weight"], W[p + ".qkv.bias"] = w(p + ".self_attn.qkv.weight"), w(p + ".self_attn.qkv.bias")
            for n in ("self_attn.out_proj", "mlp.fc1", "mlp.fc2", "layer_norm1", "layer_norm2"):
                W[f"{p}.{n}.weight"], W[f"{p}.{n}.bias"] = w(f"{p}.{n}.weight"), w(f"{p}.{n}.bias")
            for n in ("qkv", "self_attn.out_proj", "mlp.fc1", "mlp.fc2"):
                self.WT[f"{p}.{n}"] = ops.transpose(W[f"{p}.{n}.weight"])
        self.W, self._pos_rep = W, {}

    @torch.no_grad()
    def forward_train(self, pixel_values: torch.Tensor):
        """last_hidden_state with a stash: the same launches in the same order (bit-identical tokens), the LayerNorm launches also
        return (mean, rstd), attention returns lse and quick_gelu writes out of place so that the fc1 output survives.
        -> (tokens fp16 [B, N, D], kept)."""
        cfg, W = self.cfg, self.W
        B, _, S, S2 = pixel_values.shape
        P, D, H = cfg.patch_size, cfg.hidden_size, cfg.num_attention_heads
        if S != cfg.image_size or S2 != S:
            raise ValueError(f"CLIP vision tower expects {cfg.image_size}x{cfg.image_size} images, got {S}x{S2}")
        g, N, Lp, d = S // P, cfg.num_tokens, self.Lp, D // H
        x = pixel_values.to(self.dev, torch.float32).reshape(B, 3, g, P, g, P).permute(0, 2, 4, 1, 3, 5)
        cols = torch.zeros(B * g * g, self.Kp, device=self.dev, dtype=torch.float16)
        cols[:, :3 * P * P] = x.reshape(B * g * g, 3 * P * P)
        tok = torch.zeros(B, Lp, D, device=self.dev, dtype=torch.float16)
        emb = ops.gemm(cols, W["patch"])
        tok[:, 1:N] = emb.view(B, g * g, D)
        if B not in self._pos_rep:
            self._pos_rep[B] = W["pos"].repeat(B, 1).contiguous()
        x0 = ops.axpby(tok.view(B * Lp, D), self._pos_rep[B])
        eps = cfg.layer_norm_eps
        x, st0 = ops.layernorm(x0, W["pre_layrnorm.weight"], W["pre_layrnorm.bias"], eps, want_stats=True)
        scale = d ** -0.5
        layers = []
        for l in range(cfg.num_hidden_layers):
            p = f"encoder.layers.{l}"
            h1, s1 = ops.layernorm(x, W[p + ".layer_norm1.weight"], W[p + ".layer_norm1.bias"], eps, want_stats=True)
            qkv = ops.gemm(h1, W[p + ".qkv.weight"], bias=W[p + ".qkv.bias"])
            a, lse = ops.attn_fwd(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], B, H, Lp, N, Lp, d, scale, want_lse=True, v_rows=True)
            x2 = ops.gemm(a, W[p + ".self_attn.out_proj.weight"], bias=W[p + ".self_attn.out_proj.bias"], residual=x)
            h2, s2 = ops.layernorm(x2, W[p + ".layer_norm2.weight"], W[p + ".layer_norm2.bias"], eps, want_stats=True)
            f = ops.gemm(h2, W[p + ".mlp.fc1.weight"], bias=W[p + ".mlp.fc1.bias"])
            act = ops.quick_gelu(f)
            # a is both out_proj's operand and the attention output O that delta = rowsum(dO . O) needs
            layers.append(dict(x1=x, s1=s1, h1=h1, qkv=qkv, a=a, lse=lse, x2=x2, s2=s2, h2=h2, f=f, act=act))
            x = ops.gemm(act, W[p + ".mlp.fc2.weight"], bias=W[p + ".mlp.fc2.bias"], residual=x2)
        return x.view(B, Lp, D)[:, :N].contiguous(), dict(B=B, cols=cols, x0=x0, st0=st0, layers=layers)

    def embedding_fold(self, dX0: torch.Tensor, B: int) -> torch.Tensor:
        """dX0 fp16 [B * Lp, D] -> fp32 [N, D]: row n = sum over the images of their row n, in ascending image order (skg_colsum_f16
        over the [B, Lp * D] view: one image per chunk up to 32 images, the chunks folded in order; no atomics)."""
        D = self.cfg.hidden_size
        assert dX0.shape == (B * self.Lp, D) and dX0.is_contiguous()
        return ops.colsum(dX0.view(B, self.Lp * D)).view(self.Lp, D)[:self.cfg.num_tokens]

    @torch.no_grad()
    def backward(self, kept: dict, d_tokens: torch.Tensor, g: torch.Tensor) -> None:
        """d_tokens fp16 [B, N, D] = d loss / d tokens -> every parameter gradient accumulated (+=) into self.grad_view(g, key), fp32
        views of the caller's flat vector (the fused qkv keys included).  The pixels get no gradient.

        The Lp - N pad rows of every image are live queries in the forward but never keys, so their gradient is zero everywhere
        provided (1) the seed buffer is zeroed before the N token rows of each image are copied in and (2) the [B * Lp, 3D] buffer
        dq / dk / dv land in is zeroed (the strided dk / dv launch leaves rows >= N untouched).  Both are done below; nothing else
        masks.  No atomics anywhere in the chain: two runs give the same bits."""
        cfg, W, WT = self.cfg, self.W, self.WT
        B, D, H, N, Lp, P = kept["B"], cfg.hidden_size, cfg.num_attention_heads, cfg.num_tokens, self.Lp, cfg.patch_size
        d, M = D // H, kept["B"] * self.Lp
        scale = d ** -0.5
        assert d_tokens.shape == (B, N, D) and d_tokens.dtype == torch.float16
        gv = lambda k: self.grad_view(g, k)
        acc = dict(accumulate=True)
        dx = torch.zeros(M, D, device=self.dev, dtype=torch.float16)                       # (1)
        ops.batch_copy(d_tokens.contiguous().view(B * N, D), N, dx, Lp, B, N)
        for l in reversed(range(cfg.num_hidden_layers)):
            p, k = f"encoder.layers.{l}", kept["layers"][l]
            # x3 = x2 + fc2(quick_gelu(fc1(LN2(x2))))
            ops.wgrad(dx, k["act"], gv(p + ".mlp.fc2.weight"), gv(p + ".mlp.fc2.bias"), **acc)
            df = ops.gemm(dx, WT[p + ".mlp.fc2"])
            ops.quick_gelu_bwd(k["f"], df, out=df)
            ops.wgrad(df, k["h2"], gv(p + ".mlp.fc1.weight"), gv(p + ".mlp.fc1.bias"), **acc)
            dh = ops.gemm(df, WT[p + ".mlp.fc1"])
            ops.layernorm_param_grads(k["x2"], dh, k["s2"], gv(p + ".layer_norm2.weight"), gv(p + ".layer_norm2.bias"), **acc)
            dx2 = ops.layernorm_bwd(k["x2"], dh, W[p + ".layer_norm2.weight"], k["s2"], residual=dx)
            # x2 = x1 + out_proj(attention(qkv(LN1(x1))))
            ops.wgrad(dx2, k["a"], gv(p + ".self_attn.out_proj.weight"), gv(p + ".self_attn.out_proj.bias"), **acc)
            da = ops.gemm(dx2, WT[p + ".self_attn.out_proj"])
            qkv = k["qkv"]
            Q, K, V = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
            dqkv = torch.zeros(M, 3 * D, device=self.dev, dtype=torch.float16)            # (2)
            _, delta = ops.attn_bwd_dq_delta(Q, K, V, da, k["a"], k["lse"], B, H, Lp, N, Lp, d, scale, out=dqkv[:, :D])
            ops.attn_bwd_dkv_strided(Q, K, V, da, k["lse"], delta, B, H, Lp, N, Lp, d, scale, dqkv[:, D:2 * D], dqkv[:, 2 * D:])
            ops.wgrad(dqkv, k["h1"], gv(p + ".self_attn.qkv.weight"), gv(p + ".self_attn.qkv.bias"), **acc)
            dh = ops.gemm(dqkv, WT[p + ".qkv"])
            ops.layernorm_param_grads(k["x1"], dh, k["s1"], gv(p + ".layer_norm1.weight"), gv(p + ".layer_norm1.bias"), **acc)
            dx = ops.layernorm_bwd(k["x1"], dh, W[p + ".layer_norm1.weight"], k["s1"], residual=dx2)
        # front: pre_layrnorm, the position / class embedding (the pack adds the two in row 0), the patch embedding
        ops.layernorm_param_grads(kept["x0"], dx, kept["st0"], gv("pre_layrnorm.weight"), gv("pre_layrnorm.bias"), **acc)
        dx0 = ops.layernorm_bwd(kept["x0"], dx, W["pre_layrnorm.weight"], kept["st0"])
        dpos = self.embedding_fold(dx0, B)
        gv("embeddings.position_embedding.weight").add_(dpos)
        gv("embeddings.class_embedding").add_(dpos[0])
        dpatch = torch.empty(B * (N - 1), D, device=self.dev, dtype=torch.float16)
        ops.batch_copy(dx0[1:], Lp, dpatch, N - 1, B, N - 1)
        dwp = ops.wgrad(dpatch, kept["cols"])                                              # [D, Kp]: the first 3 P^2 columns are real
        gv("embeddings.patch_embedding.weight").view(D, 3 * P * P).add_(dwp[:, :3 * P * P])


class _VisionOutput:
    def __init__(self, last_hidden_state):
        self.last_hidden_state = last_hidden_state


class CLIPVisionModel:
    """Facade with the surface modules/clip_guided_inf.py:49-54,103 uses of transformers.CLIPVisionModel:
    ``from_pretrained(path)``, ``load_state_dict(sd)``, ``.to(device, dtype=)``, ``.device`` / ``.dtype``,
    ``model(pixel_values, output_hidden_states=True).last_hidden_state``."""

    def __init__(self, cfg: CLIPVisionConfig = VIT_L_14, state_dict: Optional[Dict[str, torch.Tensor]] = None):
        from . import synthetic
        self.cfg = self.config = cfg
        self._sd = strip_prefix(state_dict) if state_dict is not None else synthetic.clip_vision_state_dict(cfg)
        self._hip: Optional[HipCLIPVision] = None
        self.device, self.dtype = torch.device("cpu"), torch.float16

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path=None, config: Optional[CLIPVisionConfig] = None, **kwargs):
        sd = None
        if pretrained_model_name_or_path and os.path.isdir(pretrained_model_name_or_path):
            st = os.path.join(pretrained_model_name_or_path, "model.safetensors")
            pt = os.path.join(pretrained_model_name_or_path, "pytorch_model.bin")
            if os.path.exists(st):
                from safetensors.torch import load_file
                sd = load_file(st)
            elif os.path.exists(pt):
                sd = torch.load(pt, map_location="cpu")
            if sd is not None:
                sd = {k: v for k, v in sd.items() if k.startswith(("vision_model.", "embeddings.", "encoder.",
                                                                   "pre_layrnorm.", "post_layernorm."))}
        return cls(config or VIT_L_14, sd)

    def state_dict(self):
        return self._sd

    def load_state_dict(self, sd, strict: bool = True):
        sd = strip_prefix(sd)
        missing = [k for k in self._sd if k not in sd and "position_ids" not in k]
        if strict and missing:
            raise RuntimeError(f"CLIPVisionModel.load_state_dict: missing keys {missing[:4]} ...")
        self._sd = {k: v for k, v in sd.items() if "position_ids" not in k}
        if self._hip is not None:
            self._hip = HipCLIPVision(self.cfg, self._sd, self.device)
        return self

    def to(self, device=None, dtype=None):
        if isinstance(device, torch.dtype):
            device, dtype = None, device
        if device is not None:
            self.device = torch.device(device)
            if self.device.type == "cuda":
                if self._hip is None:
                    self._hip = HipCLIPVision(self.cfg, self._sd, self.device)
                else:
                    self._hip.to(self.device)
        return self

    def eval(self):
        return self

    # what modules/clip_guided_trainer.py:117,157 calls on the tower; the training itself is clip_vision_train.HipClipTowerTrainer
    def train(self, mode: bool = True):
        return self

    def requires_grad_(self, requires_grad: bool = True):
        return self

    def parameters(self):
        """The state dict's tensors (the reference chains them into its optimizer's parameter list)."""
        return iter(self._sd.values())

    def __call__(self, pixel_values, output_hidden_states: bool = False, **kwargs):
        if self._hip is None:
            raise RuntimeError("CLIPVisionModel: call .to('cuda') first - the tower runs on libskg.so kernels only")
        return _VisionOutput(self._hip.last_hidden_state(pixel_values))
