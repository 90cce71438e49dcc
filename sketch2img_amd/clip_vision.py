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

from typing import Dict, List, Optional

import torch

from . import clip_encoder, ops
from .clip_encoder import CLIPFacade, _round_up, encoder_layers, pack_layers, state_dict_accessors
from .config import CLIPVisionConfig, VIT_L_14


def strip_prefix(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    return clip_encoder.strip_prefix(sd, "vision_model.")


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
            self._pack(*state_dict_accessors(strip_prefix(state_dict), self.dev))
        else:
            assert state_dict is None, "a training tower reads the trainer's working copy, not a state dict"
            self.w16, self.w32, self.grad_view = views
            self.refresh()

    def _pack(self, w, w32):
        """W, read through w(key) -> fp16 tensor and w32(key) -> fp32 tensor (the fused qkv keys included): the patch weights
        [D, 3 P^2 (c, y, x)] zero-padded to Kp columns, the position rows padded to Lp with row 0 = fp16(pos32[0] + class32) - the
        cls token plus its position, ONE rounding of the fp32 sum, so that an inference tower built from a trainer's state_dict()
        gives the training forward's bits - and the layers."""
        cfg, D = self.cfg, self.cfg.hidden_size
        W: Dict[str, torch.Tensor] = {}
        pe = w("embeddings.patch_embedding.weight").reshape(D, -1)
        W["patch"] = torch.nn.functional.pad(pe, (0, self.Kp - pe.shape[1]))
        pos32 = w32("embeddings.position_embedding.weight")
        pos = torch.zeros(self.Lp, D, device=pos32.device, dtype=torch.float32)
        pos[:cfg.num_tokens] = pos32
        pos[0] += w32("embeddings.class_embedding")
        W["pos"] = pos.to(self.dev, torch.float16)
        for k in ("pre_layrnorm.weight", "pre_layrnorm.bias"):
            W[k] = w(k)
        pack_layers(W, w, cfg.num_hidden_layers)
        self.W, self._pos_rep = W, {}

    def to(self, device):
        if torch.device(device) != self.dev:
            if self.views is not None:
                raise RuntimeError("HipCLIPVision: a training tower's weights are views of its trainer's vectors and cannot move")
            self.dev = torch.device(device)
            self.W = {k: v.to(self.dev) for k, v in self.W.items()}
            self._pos_rep = {}
        return self

    def _forward(self, pixel_values: torch.Tensor, stash: Optional[List[dict]] = None):
        """-> (tokens fp16 [B, N, D], what the backward needs of the front).  stash: see clip_encoder.encoder_layers."""
        cfg, W = self.cfg, self.W
        B, _, S, S2 = pixel_values.shape
        P, D = cfg.patch_size, cfg.hidden_size
        if S != cfg.image_size or S2 != S:
            raise ValueError(f"CLIP vision tower expects {cfg.image_size}x{cfg.image_size} images, got {S}x{S2}")
        g, N, Lp = S // P, cfg.num_tokens, self.Lp
        # unfold the non-overlapping patches: pure data movement (no arithmetic) done with torch views
        x = pixel_values.to(self.dev, torch.float32).reshape(B, 3, g, P, g, P).permute(0, 2, 4, 1, 3, 5)
        cols = torch.zeros(B * g * g, self.Kp, device=self.dev, dtype=torch.float16)
        cols[:, :3 * P * P] = x.reshape(B * g * g, 3 * P * P)
        tok = torch.zeros(B, Lp, D, device=self.dev, dtype=torch.float16)
        emb = ops.gemm(cols, W["patch"])                                       # [B*g*g, D]
        tok[:, 1:N] = emb.view(B, g * g, D)
        if B not in self._pos_rep:
            self._pos_rep[B] = W["pos"].repeat(B, 1).contiguous()
        x0 = ops.axpby(tok.view(B * Lp, D), self._pos_rep[B])                  # + position (+ class) embedding
        keep = stash is not None
        x = ops.layernorm(x0, W["pre_layrnorm.weight"], W["pre_layrnorm.bias"], cfg.layer_norm_eps, want_stats=keep)
        x, st0 = x if keep else (x, None)
        x = encoder_layers(x, W, cfg, B, Lp, N, ops.quick_gelu, causal=False, stash=stash)
        return x.view(B, Lp, D)[:, :N].contiguous(), dict(B=B, cols=cols, x0=x0, st0=st0, layers=stash)

    @torch.no_grad()
    def last_hidden_state(self, pixel_values: torch.Tensor) -> torch.Tensor:
        """pixel_values [B, 3, S, S] (already CLIP-normalised) -> fp16 [B, 1 + (S/P)^2, D]."""
        return self._forward(pixel_values)[0]

    # ---- training: the weights are views of a trainer's fp16 working copy ----------------------------------------------------------
    def refresh(self):
        """Rebuild what is derived from the working copy (once per optimizer step): the pack, and the transposed packs the
        data-gradient GEMMs read (ops.transpose)."""
        assert self.views is not None, "refresh() belongs to a training tower (views=...)"
        self._pack(self.w16, self.w32)
        self.WT: Dict[str, torch.Tensor] = {}
        for l in range(self.cfg.num_hidden_layers):
            for n in ("qkv", "self_attn.out_proj", "mlp.fc1", "mlp.fc2"):
                self.WT[f"encoder.layers.{l}.{n}"] = ops.transpose(self.W[f"encoder.layers.{l}.{n}.weight"])

    @torch.no_grad()
    def forward_train(self, pixel_values: torch.Tensor):
        """last_hidden_state with a stash: the same launches in the same order (bit-identical tokens).
        -> (tokens fp16 [B, N, D], kept: B cols x0 st0 layers)."""
        return self._forward(pixel_values, stash=[])

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


class CLIPVisionModel(CLIPFacade):
    """Facade with the surface modules/clip_guided_inf.py:49-54,103 uses of transformers.CLIPVisionModel:
    ``from_pretrained(path)``, ``load_state_dict(sd)``, ``.to(device, dtype=)``, ``.device`` / ``.dtype``,
    ``model(pixel_values, output_hidden_states=True).last_hidden_state``."""
    ENGINE, PREFIX, WHAT = HipCLIPVision, "vision_model.", "the tower"

    def __init__(self, cfg: CLIPVisionConfig = VIT_L_14, state_dict: Optional[Dict[str, torch.Tensor]] = None):
        from . import synthetic
        super().__init__(cfg, state_dict, synthetic.clip_vision_state_dict)

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path=None, config: Optional[CLIPVisionConfig] = None, **kwargs):
        sd = cls.read_folder(pretrained_model_name_or_path)
        if sd is not None:
            sd = {k: v for k, v in sd.items() if k.startswith(("vision_model.", "embeddings.", "encoder.",
                                                               "pre_layrnorm.", "post_layernorm."))}
        return cls(config or VIT_L_14, sd)

    # what modules/clip_guided_trainer.py:117,157 calls on the tower; the training itself is clip_vision_train.HipClipTowerTrainer
    def train(self, mode: bool = True):
        return self

    def requires_grad_(self, requires_grad: bool = True):
        return self

    def parameters(self):
        """The state dict's tensors (the reference chains them into its optimizer's parameter list)."""
        return iter(self._sd.values())

    def __call__(self, pixel_values, output_hidden_states: bool = False, **kwargs):
        return _VisionOutput(self.engine().last_hidden_state(pixel_values))
