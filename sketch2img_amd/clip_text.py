"""CLIP text encoder on the libskg.so kernels: prompts -> the (B, L, D) conditioning the UNet cross-attends to.

Replaces ``self.text_encoder(text_input_ids)[0]`` inside StableDiffusionPipeline._encode_prompt, which the reference
calls at modules/pipeline.py:55-57 (third-party transformers CLIPTextModel; restated and PINNED against transformers'
own class in oracle/clip_text.py + tests/golden/clip_text_tiny.npz).  Runs once per prompt batch.

Layout: tokens fp16 [B * Lp, D], every prompt's L (= 77) tokens padded to Lp = a multiple of 8 rows (80) so the
transposed V panel keeps 16-byte aligned rows; pad rows are never read as keys (Nkv = L) and are dropped at the end.
The token-embedding row gather is data movement (torch.index_select on the fp16 table); q/k/v are one GEMM with bias,
the causal softmax(QK^T)V is the flash kernel's CAUSAL instantiation (skg_attn_fwd with SKG_ATTN_CAUSAL), out-proj / fc2 carry the
residual in the GEMM epilogue, quick_gelu (SD 1.x) or exact gelu (SD 2.x) and LayerNorm are their own kernels.
Tokenisation (BPE) is host-side text processing and stays with transformers' CLIPTokenizer (`PromptEncoder`).

Long prompts (`encode_tokens`, the reference's modules/clip_guided_trainer.py:40-66 fed by modules/dataset.py:114-123 and
:204-211): an id matrix wider than 77 is cut into 75-token windows, each wrapped in BOS / EOS and encoded on its own, and the
hidden states are concatenated along the sequence axis: L = width + 2 * windows keys, 78 ... 231 for the reference's
max_length = 225.  All windows of a batch go through the layer stack in ONE pass, as (windows * B) rows of 77 tokens: the encoder
is causal and row-local, so the shorter last window rides along padded behind its EOS and its pad rows are dropped.
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional

import torch

from . import clip_encoder, ops
from .clip_encoder import CLIPFacade, _round_up, encoder_layers, pack_layers, state_dict_accessors
from .config import CLIPTextConfig, SD15_TEXT, SD21_TEXT


def strip_prefix(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    return clip_encoder.strip_prefix(sd, "text_model.")


class HipCLIPText:
    def __init__(self, cfg: CLIPTextConfig, state_dict: Dict[str, torch.Tensor], device="cuda"):
        if cfg.hidden_act not in ("quick_gelu", "gelu"):
            raise ValueError(f"CLIP text encoder: unsupported hidden_act {cfg.hidden_act!r}")
        self.cfg, self.dev = cfg, torch.device(device)
        h16, _ = state_dict_accessors(strip_prefix(state_dict), self.dev)
        W = self.W = {"tok": h16("embeddings.token_embedding.weight"), "pos": h16("embeddings.position_embedding.weight")}
        for k in ("final_layer_norm.weight", "final_layer_norm.bias"):
            W[k] = h16(k)
        pack_layers(W, h16, cfg.num_hidden_layers)

    def to(self, device):
        if torch.device(device) != self.dev:
            self.dev = torch.device(device)
            self.W = {k: v.to(self.dev) for k, v in self.W.items()}
        return self

    @torch.no_grad()
    def last_hidden_state(self, input_ids: torch.Tensor) -> torch.Tensor:
        """input_ids int [B, L <= max_position_embeddings] -> fp16 [B, L, D] (final_layer_norm applied)."""
        cfg, W = self.cfg, self.W
        B, L = input_ids.shape
        if L > cfg.max_position_embeddings:
            raise ValueError(f"CLIP text encoder: {L} tokens > max_position_embeddings {cfg.max_position_embeddings}")
        ids = input_ids.to(self.dev, torch.long)
        if int(ids.min()) < 0 or int(ids.max()) >= cfg.vocab_size:
            raise ValueError("CLIP text encoder: token id outside the vocabulary")
        D, Lp = cfg.hidden_size, _round_up(L, 8)
        tok = torch.zeros(B, Lp, D, device=self.dev, dtype=torch.float16)
        pos = torch.zeros(B, Lp, D, device=self.dev, dtype=torch.float16)
        tok[:, :L] = W["tok"].index_select(0, ids.reshape(-1)).view(B, L, D)       # row gather: data movement only
        pos[:, :L] = W["pos"][:L]
        x = ops.axpby(tok.view(B * Lp, D), pos.view(B * Lp, D))
        act = ops.quick_gelu if cfg.hidden_act == "quick_gelu" else ops.gelu
        x = encoder_layers(x, W, cfg, B, Lp, L, act, causal=True)
        x = ops.layernorm(x, W["final_layer_norm.weight"], W["final_layer_norm.bias"], cfg.layer_norm_eps)
        return x.view(B, Lp, D)[:, :L].contiguous()


class _TextOutput(tuple):
    """``out[0]`` and ``out.last_hidden_state`` both work, like transformers' BaseModelOutputWithPooling."""

    def __new__(cls, last_hidden_state):
        self = super().__new__(cls, (last_hidden_state,))
        self.last_hidden_state = last_hidden_state
        return self


def _config_from_folder(path: Optional[str]) -> CLIPTextConfig:
    import json
    if path and os.path.exists(os.path.join(path, "config.json")):
        with open(os.path.join(path, "config.json")) as f:
            c = json.load(f)
        c = c.get("text_config", c) if "hidden_size" not in c else c
        keys = CLIPTextConfig.__dataclass_fields__.keys()
        return CLIPTextConfig(**{k: c[k] for k in keys if k in c})
    return SD15_TEXT


class CLIPTextModel(CLIPFacade):
    """Facade with the surface diffusers' _encode_prompt uses of transformers.CLIPTextModel: ``from_pretrained(path)``,
    ``load_state_dict(sd)``, ``.to(device)``, ``.device`` / ``.dtype`` / ``.config``, ``model(input_ids)[0]``."""
    ENGINE, PREFIX, WHAT = HipCLIPText, "text_model.", "the encoder"

    def __init__(self, cfg: CLIPTextConfig = SD15_TEXT, state_dict: Optional[Dict[str, torch.Tensor]] = None):
        from . import synthetic
        super().__init__(cfg, state_dict, synthetic.clip_text_state_dict)

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path=None, config: Optional[CLIPTextConfig] = None,
                        subfolder: Optional[str] = None, **kwargs):
        path = pretrained_model_name_or_path
        if path and subfolder:
            path = os.path.join(path, subfolder)
        sd = cls.read_folder(path)
        if sd is not None:
            sd = {k: v for k, v in sd.items() if "position_ids" not in k}
        return cls(config or _config_from_folder(path), sd)

    def __call__(self, input_ids, attention_mask=None, **kwargs):
        return _TextOutput(self.engine().last_hidden_state(input_ids))


WINDOW = 75          # tokens of the prompt per window; with BOS and EOS a window is the encoder's 77 positions


def split_windows(input_ids, bos_token_id: int, eos_token_id: int) -> List[torch.Tensor]:
    """The id matrices `encode_tokens` encodes, in order (host only).  input_ids int [B, W]: W <= 77 is taken as is; otherwise
    consecutive windows of 75 columns of the RAW ids - the prompt's own BOS / EOS and the collate padding stay inside - each as
    [BOS, window, EOS]; the last window is as short as what is left, so the widths sum to W + 2 * windows."""
    ids = torch.as_tensor(input_ids)
    if ids.dim() != 2:
        raise ValueError(f"encode_tokens: input_ids must be [B, W], got {tuple(ids.shape)}")
    B, W = ids.shape
    if W <= WINDOW + 2:
        return [ids]
    ids = ids.to(torch.long)
    bos = torch.full((B, 1), bos_token_id, dtype=torch.long, device=ids.device)
    eos = torch.full((B, 1), eos_token_id, dtype=torch.long, device=ids.device)
    return [torch.cat([bos, ids[:, c:c + WINDOW], eos], 1) for c in range(0, W, WINDOW)]


def encode_tokens(tokenizer, text_encoder, input_ids) -> torch.Tensor:
    """modules/clip_guided_trainer.py:40-66 on the HIP text encoder: int [B, W] -> fp16 [B, L, D], L = W (W <= 77) or
    W + 2 * ceil(W / 75).  Of ``tokenizer`` only ``bos_token_id`` / ``eos_token_id`` are read; ``text_encoder`` is the
    `CLIPTextModel` facade.  One pass through the layer stack for all windows (see the module docstring)."""
    wins = split_windows(input_ids, tokenizer.bos_token_id, tokenizer.eos_token_id)
    if len(wins) == 1:
        return text_encoder(wins[0])[0]
    B, full = wins[0].shape
    last = wins[-1]
    if last.shape[1] < full:      # pad rows behind the window's EOS: causal attention keeps them out of the rows in front
        pad = torch.full((B, full - last.shape[1]), tokenizer.eos_token_id, dtype=last.dtype, device=last.device)
        last = torch.cat([last, pad], 1)
    h = text_encoder(torch.cat(wins[:-1] + [last], 0))[0]
    return torch.cat([h[i * B:(i + 1) * B, :w.shape[1]] for i, w in enumerate(wins)], 1)


class PromptEncoder:
    """``(list[str]) -> (B, L, D)``: the tokenizer + text-encoder half of diffusers' _encode_prompt
    (modules/pipeline.py:55-57): pad to ``model_max_length`` with truncation, then ``text_encoder(ids)[0]`` (L = 77).
    ``tokenizer`` is any callable with transformers' tokenizer call convention (CLIPTokenizer in practice).

    ``max_length`` (an integer; 225 is the reference trainer's) selects the long-prompt path instead: tokenise without padding
    and truncate at ``max_length`` (modules/dataset.py:114-123), pad the batch to its longest prompt with ``tokenizer.pad``
    (``collate_fn``, :204-211), then `encode_tokens`: L = W (W <= 77) or W + 2 * ceil(W / 75) for the padded width W, up to
    231.  All prompts of one call share one L."""

    def __init__(self, tokenizer, text_model: CLIPTextModel, max_length: Optional[int] = None):
        if max_length is not None and int(max_length) < 1:
            raise ValueError(f"PromptEncoder: max_length must be positive, got {max_length}")
        self.tokenizer, self.text_model = tokenizer, text_model
        self.max_length = None if max_length is None else int(max_length)

    @classmethod
    def from_pretrained(cls, folder: str, max_length: Optional[int] = None):
        """``folder`` is a diffusers checkpoint directory with ``tokenizer/`` and ``text_encoder/`` inside."""
        from transformers import CLIPTokenizer          # BPE tables + host-side string processing only
        tok = CLIPTokenizer.from_pretrained(os.path.join(folder, "tokenizer"))
        return cls(tok, CLIPTextModel.from_pretrained(folder, subfolder="text_encoder"), max_length)

    def to(self, device):
        self.text_model.to(device)
        return self

    def tokenize(self, prompts: List[str]) -> torch.Tensor:
        """The long-prompt id matrix int [B, W] (``max_length`` set): unpadded truncated ids, padded to the longest."""
        ids = self.tokenizer(list(prompts), padding="do_not_pad", truncation=True, max_length=self.max_length)["input_ids"]
        return torch.as_tensor(self.tokenizer.pad({"input_ids": ids}, padding=True, return_tensors="pt")["input_ids"])

    def __call__(self, prompts: List[str]) -> torch.Tensor:
        if self.max_length is not None:
            return encode_tokens(self.tokenizer, self.text_model, self.tokenize(prompts))
        L = getattr(self.tokenizer, "model_max_length", None) or self.text_model.cfg.max_position_embeddings
        L = min(L, self.text_model.cfg.max_position_embeddings)
        enc = self.tokenizer(list(prompts), padding="max_length", max_length=L, truncation=True, return_tensors="pt")
        return self.text_model(enc["input_ids"])[0]
