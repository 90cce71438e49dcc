"""Injected attention (the reference's SatMixin / AttnModule step 1.5) on the libskg.so kernels.

  * CLIP-token variant      modules/clip_guided_attn.py:111-125
        s = sketch_proj(state); z = sketch_norm(cat([h, s], 1)); a = sketch_attn(z)[:, :N]; h += scale*conv1x1(a)
  * UNet-feature variant    modules/sketch_guided_attn.py:120-132
        z = sketch_norm(h); a = sketch_attn(z, encoder_hidden_states=res_sample); h += scale*conv1x1(a)

What does not depend on the latent is hoisted to ``set_state`` / ``set_res_samples`` (once per image): the
projected + normalised sketch tokens and, for the feature variant, the K / V projections of the residual
samples.  LayerNorm is per token, so LayerNorm(cat([h, s])) == cat(LayerNorm(h), LayerNorm(s)): the sketch
tokens are normalised once and copied into the tail of the per-step token buffer.

Buffers, CLIP variant, per block: K / V [rows][N + T_pad][2C] with T = 257 sketch tokens padded to a multiple of 8.
The sketch tokens' K / V rows do not depend on the latent and are written once per image; each step the image
tokens' K / V go straight into the first N slots of every batch row (one GEMM per row, no copy), the queries are
the N image tokens only (the reference slices the sketch-query outputs away, clip_guided_attn.py:119) and the
last padding keys are masked by Nkv < kv_stride.
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Sequence

import torch

from . import ops
from .config import UNetConfig
from .unet import _fresh, _hi, _layernorm, _produce

SKETCH_TOKENS = 257
CLIP_DIM = 1024


def transformer_block_paths(cfg: UNetConfig) -> List[str]:
    """BasicTransformerBlock paths in unet.named_modules() order: down, up, mid (SatMixin.blocks order)."""
    nb = len(cfg.block_out_channels)
    out = []
    for i in range(nb - 1):
        out += [f"down_blocks.{i}.attentions.{j}.transformer_blocks.0" for j in range(cfg.layers_per_block)]
    for i in range(1, nb):
        out += [f"up_blocks.{i}.attentions.{j}.transformer_blocks.0" for j in range(cfg.layers_per_block + 1)]
    out.append("mid_block.attentions.0.transformer_blocks.0")
    return out


def block_dims(cfg: UNetConfig):
    boc = cfg.block_out_channels
    rev, rev_heads = tuple(reversed(boc)), tuple(reversed(cfg.num_heads))
    out = []
    for p in transformer_block_paths(cfg):
        parts = p.split(".")
        if parts[0] == "down_blocks":
            out.append((p, boc[int(parts[1])], cfg.num_heads[int(parts[1])]))
        elif parts[0] == "up_blocks":
            out.append((p, rev[int(parts[1])], rev_heads[int(parts[1])]))
        else:
            out.append((p, boc[-1], cfg.num_heads[-1]))
    return out


def module_name(block_path: str) -> str:
    """modules/clip_guided_attn.py:14-19: "sketch_attn." + path with '.' -> '_'."""
    return ("sketch_attn." + block_path).replace(".", "_")


def route_res_samples(res_samples: Sequence[Sequence[torch.Tensor]]) -> List[torch.Tensor]:
    """modules/sketch_guided_attn.py:29-40."""
    down, up = (), ()
    mid = (res_samples[-1][-1],)
    for layers in res_samples:
        if len(layers) == 3:
            down += (layers[0], layers[1])
            up += (layers[0], layers[1], layers[1])
    return list(down + up[::-1] + mid)


_ROWS_KV = os.environ.get("SKG_INJ_ROWS", "1") != "0"        # A/B switch: large maps, K / V of all batch rows in one launch
_BATCH_KV = os.environ.get("SKG_INJ_BATCH", "1") != "0"      # A/B switch (bench.py on one box)


class HipInjector:
    """Callable installed as ``HipUNet.inject``; ``variant`` is 'clip' or 'sketch'.  What HipUNet asks of an injector: the call
    per block below and ``check_rows(rows)`` before its first launch (``halves_equal``, where present, extends the shared CFG front)."""

    def __init__(self, cfg: UNetConfig, state_dict: Dict[str, torch.Tensor], variant: str, device):
        assert variant in ("clip", "sketch")
        self.cfg, self.variant, self.dev = cfg, variant, torch.device(device)
        self.scale = 1.0
        self.W: Dict[str, Dict[str, torch.Tensor]] = {}
        self.per_image: Dict[str, dict] = {}
        self.halves_equal = False      # set_res_samples: both CFG halves carry the same sketch features (checked, not assumed)
        h16 = lambda t: t.detach().to(self.dev, torch.float16).contiguous()
        for path, c, heads in block_dims(cfg):
            n = module_name(path)
            w = dict(C=c, heads=heads,
                     ng=h16(state_dict[f"{n}.sketch_norm.weight"]), nb=h16(state_dict[f"{n}.sketch_norm.bias"]),
                     wq=h16(state_dict[f"{n}.sketch_attn.to_q.weight"]),
                     wkv=h16(torch.cat([state_dict[f"{n}.sketch_attn.to_k.weight"],
                                        state_dict[f"{n}.sketch_attn.to_v.weight"]], 0)),
                     wo=h16(state_dict[f"{n}.sketch_attn.to_out.0.weight"]),
                     bo=h16(state_dict[f"{n}.sketch_attn.to_out.0.bias"]),
                     wc=h16(state_dict[f"{n}.sketch_conv.weight"].reshape(c, c)),
                     bc=h16(state_dict[f"{n}.sketch_conv.bias"]))
            if variant == "clip":
                w["wqkv"] = torch.cat([w["wq"], w["wkv"]], 0).contiguous()
                w["wp"] = h16(state_dict[f"{n}.sketch_proj.weight"])
                w["bp"] = h16(state_dict[f"{n}.sketch_proj.bias"])
            self.W[path] = w

    def set_scale(self, scale: float):
        self.scale = float(scale)

    # ---- once per image ---------------------------------------------------------------------------------
    def set_state(self, sketch_state: Optional[torch.Tensor]):
        """CLIP variant.  sketch_state [rows, 257, 1024] (uncond rows zero, modules/clip_guided_inf.py:107)."""
        self.per_image = {}
        if sketch_state is None:
            return
        rows, T, D = sketch_state.shape
        st = sketch_state.to(self.dev, torch.float16).reshape(rows * T, D).contiguous()
        for path, w in self.W.items():
            s = ops.gemm(st, w["wp"], bias=w["bp"])
            zs = ops.layernorm(s, w["ng"], w["nb"])
            self.per_image[path] = dict(kvs=ops.gemm(zs, w["wkv"]), rows=rows, T=T, bufs={})

    def set_res_samples(self, res_samples: Optional[Sequence[Sequence[torch.Tensor]]]):
        """Feature variant.  res_samples: per down block a tuple of NCHW tensors [rows, C, h, w]."""
        self.per_image = {}
        self.halves_equal = False
        if res_samples is None:
            return
        routed = route_res_samples(res_samples)
        # the SketchEncoder usually sees the same sketch for the uncond and the cond row of a sample: when the two halves of
        # EVERY routed tensor are equal (checked here, once per image) the injected attention is text-independent too and
        # HipUNet's shared CFG front extends through it
        self.halves_equal = all(r.shape[0] % 2 == 0 and torch.equal(r[: r.shape[0] // 2], r[r.shape[0] // 2:]) for r in routed)
        for (path, w), r in zip(self.W.items(), routed):
            rows, C, hh, ww = r.shape
            assert C == w["C"]
            tok = r.to(self.dev, torch.float16).permute(0, 2, 3, 1).reshape(rows * hh * ww, C).contiguous()
            kv = ops.gemm(tok, w["wkv"])                       # res_sample is used un-normalised (:127)
            self.per_image[path] = dict(K=kv[:, :C], V=kv[:, C:], rows=rows, N=hh * ww)

    def check_rows(self, rows: int) -> None:
        """HipUNet.forward calls this before its first launch: the state / res samples set for this image hold one row per
        batch row of the evaluation (S cond rows without CFG, [uncond rows; cond rows] with it)."""
        for path, pi in self.per_image.items():
            if pi["rows"] != rows:
                raise ValueError(f"the injector's {'state' if self.variant != 'sketch' else 'res samples'} hold {pi['rows']} rows, "
                                 f"the UNet evaluates {rows} ({path})")

    # ---- per UNet evaluation ------------------------------------------------------------------------------
    def __call__(self, path: str, h, rows: int, N: int, heads: int, cond_only: bool = False, out=None):
        """cond_only (sketch variant, halves_equal): h holds the cond rows only (rows // 2 of them); K / V of the cond half.
        h (and out) may be ops.Pair objects - HipUNet's accuracy mode: the stream enters sketch_norm as hi + lo and the scaled
        injection is added to the pair in fp32 (the result is a pair again)."""
        pair = isinstance(h, ops.Pair)
        pi = self.per_image.get(path)
        if pi is None:
            if out is not None:
                for src, dst in ((h.hi, out.hi), (h.lo, out.lo)) if pair else ((h, out),):
                    ops.batch_copy(src, src.shape[0], dst, src.shape[0], 1, src.shape[0])
                return out
            return h
        norm = lambda g, b: _layernorm(h, g, b)
        # h + scale * conv1x1(o), on a pair in fp32 (the result is a pair again)
        res = _fresh(h, *_hi(h).shape) if pair and out is None else out
        last = lambda o, wc, bc: _produce("gemm", o, wc, out=res, bias=bc, residual=h, alpha=self.scale)[0]
        w = self.W[path]
        C = w["C"]
        dh = C // heads
        scale = dh ** -0.5
        if self.variant == "sketch":
            assert pi["rows"] == rows and pi["N"] == N
            K, V, r = pi["K"], pi["V"], rows
            if cond_only:
                assert self.halves_equal
                r = rows // 2
                K, V = K[r * N:], V[r * N:]
            z = norm(w["ng"], w["nb"])
            q = ops.gemm(z, w["wq"])
            a = ops.attn_fwd(q, K, V, r, heads, N, N, N, dh, scale, v_rows=True)
            o = ops.gemm(a, w["wo"], bias=w["bo"])
            return last(o, w["wc"], w["bc"])
        # CLIP variant: self-attention of the N image-token queries over [N image tokens ; T sketch tokens]
        assert pi["rows"] == rows
        T = pi["T"]
        L = (N + T + 7) // 8 * 8
        kvbuf = pi["bufs"].get(N)
        if kvbuf is None:
            kvbuf = torch.zeros(rows * L, 2 * C, device=self.dev, dtype=torch.float16)
            ops.batch_copy(pi["kvs"], T, kvbuf[N:], L, rows, T)     # K / V of the normalised sketch tokens, once per image
            pi["bufs"][N] = kvbuf
        zh = norm(w["ng"], w["nb"])
        # K / V of the image tokens go to rows [b L, b L + N) of the [rows * L, 2C] buffer (the sketch tokens sit behind them).
        # Large maps: one GEMM per batch row straight into place (each launch fills the chip).  Small maps - a batch row is
        # under 256 tiles of 128 x 160 - : ONE GEMM over all rows for q, k and v into a dense buffer + one strided copy of the
        # k | v columns, 2 launches instead of 1 + `rows` launches of ~10-25 us each (round 3: ~12 800 of config 5's 16 000
        # GEMM launches per batch were these; same-box A/B 2.218 -> 2.266 images/s)
        if _BATCH_KV and rows > 2 and ((N + 127) // 128) * ((2 * C + 159) // 160) < 256:
            dense = ops.gemm(zh, w["wqkv"])
            q = dense[:, :C]
            ops.batch_copy(dense[:, C:], N, kvbuf, L, rows, N)
        else:
            q = ops.gemm(zh, w["wq"])
            if _ROWS_KV and C % 64 == 0:      # one launch: row block b of the product -> rows [b L, b L + N) of the K / V buffer
                ops.gemm_rows(zh, w["wkv"], kvbuf, N, L)
            else:
                for b in range(rows):
                    ops.gemm(zh[b * N:(b + 1) * N], w["wkv"], out=kvbuf[b * L:b * L + N])
        a = ops.attn_fwd(q, kvbuf[:, :C], kvbuf[:, C:], rows, heads, N, N + T, L, dh, scale, v_rows=True)
        o = ops.gemm(a, w["wo"], bias=w["bo"])
        return last(o, w["wc"], w["bc"])


class HipClipInjectorTrain:
    """The CLIP-token injector with a stash and a backward: what sat_train.HipSatTrainer installs as ``HipUNet.inject`` while it
    differentiates one sample (rows = 1).  Nothing is hoisted: the weights change every optimizer step, so sketch_proj, the
    LayerNorm of the sketch tokens and their K / V are evaluated inside every forward.

    forward (per block, N image tokens, T sketch tokens, L = ceil8(N + T)):
        x   = [h ; sketch_proj(state)]                    [N + T, C]   (h copied, the projection written behind it)
        z   = sketch_norm(x), (mean, rstd) per row        one launch over both row groups
        qkv = z . [Wq ; Wk ; Wv]^T                        [L, 3C], rows >= N + T zero; only the first N rows of q are queries
        a   = attention(q[:N], k, v; Nkv = N + T, kv_stride = L), lse
        o   = to_out(a);  out = h + scale * conv1x1(o)
    kept for the backward: x, the statistics, z, qkv, a, lse, o.

    backward(d out) -> d h (the residual path added), the gradients of the block's 12 tensors accumulated (+=, scaled like
    d out) into the flat fp32 vector handed to begin(), and d loss / d state += ds . W_proj (fp32 [T, 1024]): the seam where a
    CLIP-vision backward can attach.  Weight gradients: ops.wgrad on the row-major operands (column views of qkv / d qkv), bias
    gradients in the same pass, LayerNorm's through ops.layernorm_param_grads.

    begin() with [B, T, 1024] tensors: the same block on B samples in one walk (rows = B, HipUNet.forward(diff_from=0)) - see
    _call_batched for the layout.  The one-sample form keeps its launches."""

    def __init__(self, cfg: UNetConfig, w16, grad_view, device):
        """w16(key) -> fp16 view of the working copy; grad_view(flat, key) -> fp32 view (state-dict key names)."""
        self.cfg, self.dev = cfg, torch.device(device)
        self.w16, self.grad_view = w16, grad_view
        self.scale = 1.0
        self.dims = {p: (module_name(p), c, heads) for p, c, heads in block_dims(cfg)}
        self.state16: Optional[torch.Tensor] = None
        self.stash: Dict[str, dict] = {}
        self.g: Optional[torch.Tensor] = None
        self.dstate: Optional[torch.Tensor] = None
        self.batch: Optional[int] = None
        self.packs: Dict[str, dict] = {}

    def set_scale(self, scale: float):
        self.scale = float(scale)

    def refresh(self):
        """Rebuild the concatenated / transposed operands from the fp16 working copy (once per optimizer step)."""
        self.packs = {}
        for path, (n, c, heads) in self.dims.items():
            w = self.w16
            wqkv = torch.cat([w(f"{n}.sketch_attn.to_q.weight"), w(f"{n}.sketch_attn.to_k.weight"),
                              w(f"{n}.sketch_attn.to_v.weight")], 0).contiguous()
            wo, wc, wp = w(f"{n}.sketch_attn.to_out.0.weight"), w(f"{n}.sketch_conv.weight").reshape(c, c), w(f"{n}.sketch_proj.weight")
            self.packs[path] = dict(wqkv=wqkv, wqkvT=ops.transpose(wqkv), wo=wo, woT=ops.transpose(wo), wc=wc, wcT=ops.transpose(wc),
                                    wp=wp, wpT=ops.transpose(wp))

    def begin(self, state16: torch.Tensor, g: torch.Tensor, dstate: torch.Tensor):
        """One sample: its sketch tokens fp16 [T, 1024], the flat gradient vector to accumulate into, its d state [T, 1024] fp32.
        B samples in one UNet walk (rows = B): state16 fp16 [B, T, 1024] and d state fp32 [B, T, 1024] (B = 1 included)."""
        assert state16.dtype == torch.float16 and state16.dim() in (2, 3) and state16.shape[-1] == CLIP_DIM
        assert dstate.dtype == torch.float32 and dstate.shape == state16.shape, "d state: fp32, the shape of the state"
        assert state16.dim() == 2 or dstate.is_contiguous()
        self.batch = state16.shape[0] if state16.dim() == 3 else None      # None: the one-sample form
        self.state16, self.g, self.dstate, self.stash = state16.contiguous(), g, dstate, {}

    def end(self):
        self.state16 = self.g = self.dstate = self.batch = None
        self.stash = {}

    def check_rows(self, rows: int) -> None:
        """The injectors' protocol (HipInjector.check_rows): HipUNet.forward calls this before its first launch.  begin() holds the
        tokens of one sample, so the evaluation has one row - or of B samples ([B, T, 1024]), one row each."""
        have = 1 if self.batch is None else self.batch
        if rows != have:
            raise ValueError(f"the training injector holds the sketch tokens of {have} sample{'s' * (have != 1)}, the UNet evaluates {rows} rows")

    # ---- forward (HipUNet._tr_fwd calls this) ---------------------------------------------------------------------------------
    def __call__(self, path: str, h, rows: int, N: int, heads: int, cond_only: bool = False, out=None):
        if self.batch is not None:
            return self._call_batched(path, h, rows, N, heads, cond_only, out)
        assert rows == 1 and not cond_only and not isinstance(h, ops.Pair), "training evaluates one all-fp16 sample at a time"
        n, C, hd = self.dims[path]
        assert hd == heads and h.shape == (N, C)
        pk, w = self.packs[path], self.w16
        T = self.state16.shape[0]
        NT, L = N + T, (N + T + 7) // 8 * 8
        dh = C // heads
        x = torch.empty(NT, C, device=self.dev, dtype=torch.float16)
        ops.batch_copy(h, N, x, N, 1, N)
        ops.gemm(self.state16, pk["wp"], out=x[N:], bias=w(f"{n}.sketch_proj.bias"))
        z, st = ops.layernorm(x, w(f"{n}.sketch_norm.weight"), w(f"{n}.sketch_norm.bias"), want_stats=True)
        qkv = torch.zeros(L, 3 * C, device=self.dev, dtype=torch.float16)
        ops.gemm(z, pk["wqkv"], out=qkv[:NT])
        a, lse = ops.attn_fwd(qkv[:N, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], 1, heads, N, NT, L, dh, dh ** -0.5, want_lse=True,
                              v_rows=True)
        o = ops.gemm(a, pk["wo"], bias=w(f"{n}.sketch_attn.to_out.0.bias"))
        res = ops.gemm(o, pk["wc"], out, bias=w(f"{n}.sketch_conv.bias"), residual=h, alpha=self.scale)
        self.stash[path] = dict(x=x, st=st, z=z, qkv=qkv, a=a, lse=lse, o=o, N=N, heads=heads)
        return res

    # ---- backward (HipUNet._tr_bwd calls this through backward_eps(inject_bwd=)) ---------------------------------------------------
    def backward(self, path: str, dout):
        if self.batch is not None:
            return self._backward_batched(path, dout)
        n, C, heads = self.dims[path]
        s, pk, w = self.stash.pop(path), self.packs[path], self.w16
        N, T = s["N"], self.state16.shape[0]
        NT, L = N + T, (N + T + 7) // 8 * 8
        dh = C // heads
        sc = dh ** -0.5
        gv = lambda k: self.grad_view(self.g, f"{n}.{k}")
        acc = dict(accumulate=True)
        x, z, qkv = s["x"], s["z"], s["qkv"]
        # out = h + scale * (o . Wc^T + bc)
        ops.wgrad(dout, s["o"], gv("sketch_conv.weight"), gv("sketch_conv.bias"), alpha=self.scale, **acc)
        do = ops.gemm(dout, pk["wcT"], alpha=self.scale)
        ops.wgrad(do, s["a"], gv("sketch_attn.to_out.0.weight"), gv("sketch_attn.to_out.0.bias"), **acc)
        da = ops.gemm(do, pk["woT"])
        # attention: queries = the N image rows, keys / values = all N + T rows of the padded buffer
        dqkv = torch.zeros(L, 3 * C, device=self.dev, dtype=torch.float16)
        Q, K, V = qkv[:N, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
        _, delta = ops.attn_bwd_dq_delta(Q, K, V, da, s["a"], s["lse"], 1, heads, N, NT, L, dh, sc, out=dqkv[:N, :C])
        ops.attn_bwd_dkv_strided(Q, K, V, da, s["lse"], delta, 1, heads, N, NT, L, dh, sc, dqkv[:, C:2 * C], dqkv[:, 2 * C:])
        ops.wgrad(dqkv[:N, :C], z[:N], gv("sketch_attn.to_q.weight"), **acc)
        ops.wgrad(dqkv[:NT, C:2 * C], z, gv("sketch_attn.to_k.weight"), **acc)
        ops.wgrad(dqkv[:NT, 2 * C:], z, gv("sketch_attn.to_v.weight"), **acc)
        dz = ops.gemm(dqkv[:NT], pk["wqkvT"])
        ops.layernorm_param_grads(x, dz, s["st"], gv("sketch_norm.weight"), gv("sketch_norm.bias"), **acc)
        dx = ops.layernorm_bwd(x, dz, w(f"{n}.sketch_norm.weight"), s["st"])
        ds = dx[N:]
        ops.wgrad(ds, self.state16, gv("sketch_proj.weight"), gv("sketch_proj.bias"), **acc)
        self.dstate += ops.gemm(ds, pk["wpT"], out_f32=True)
        return ops.axpby(dx[:N], dout)

    # ---- B samples in one walk (begin() with [B, T, 1024]) ------------------------------------------------------------------------
    # Image rows h [B N, C] and token rows s [B T, C] stay two contiguous tensors - LayerNorm is per row, so the concatenated x is
    # never built.  K / V of both are gathered per sample into ONE zeroed buffer [B L, 2C], L = ceil8(N + T): sample b's image keys
    # in rows [b L, b L + N), its sketch keys behind them, the pad rows zero and masked by Nkv < kv_stride.  The attention trio runs
    # with batch = B; every weight gradient contracts over all samples' rows in one launch per operand pair (to_k / to_v: one over
    # the image rows and one over the token rows, in that fixed order): no atomics, bit-repeatable.
    def _call_batched(self, path: str, h, rows: int, N: int, heads: int, cond_only: bool, out):
        B = self.batch
        assert rows == B and not cond_only and not isinstance(h, ops.Pair), "batched training evaluates B all-fp16 samples, one row each"
        n, C, hd = self.dims[path]
        assert hd == heads and h.shape == (B * N, C)
        pk, w = self.packs[path], self.w16
        T = self.state16.shape[1]
        NT, L = N + T, (N + T + 7) // 8 * 8
        dh = C // heads
        ng, nb = w(f"{n}.sketch_norm.weight"), w(f"{n}.sketch_norm.bias")
        s = ops.gemm(self.state16.view(B * T, CLIP_DIM), pk["wp"], bias=w(f"{n}.sketch_proj.bias"))
        zh, sth = ops.layernorm(h, ng, nb, want_stats=True)
        zs, sts = ops.layernorm(s, ng, nb, want_stats=True)
        qkv = ops.gemm(zh, pk["wqkv"])                               # [B N, 3C]: q of the image rows (the only queries), their k | v
        kvs = ops.gemm(zs, pk["wqkv"][C:])                           # [B T, 2C]: k | v of the sketch tokens
        kv = torch.zeros(B * L, 2 * C, device=self.dev, dtype=torch.float16)
        ops.batch_copy(qkv[:, C:], N, kv, L, B, N)
        ops.batch_copy(kvs, T, kv[N:], L, B, T)
        q = qkv[:, :C]
        a, lse = ops.attn_fwd(q, kv[:, :C], kv[:, C:], B, heads, N, NT, L, dh, dh ** -0.5, want_lse=True, v_rows=True)
        o = ops.gemm(a, pk["wo"], bias=w(f"{n}.sketch_attn.to_out.0.bias"))
        res = ops.gemm(o, pk["wc"], out, bias=w(f"{n}.sketch_conv.bias"), residual=h, alpha=self.scale)
        self.stash[path] = dict(h=h, s=s, sth=sth, sts=sts, zh=zh, zs=zs, q=q, kv=kv, a=a, lse=lse, o=o, N=N, L=L, heads=heads)
        return res

    def _backward_batched(self, path: str, dout):
        n, C, heads = self.dims[path]
        st, pk, w = self.stash.pop(path), self.packs[path], self.w16
        B, T, N, L = self.batch, self.state16.shape[1], st["N"], st["L"]
        NT = N + T
        dh = C // heads
        sc = dh ** -0.5
        gv = lambda k: self.grad_view(self.g, f"{n}.{k}")
        acc = dict(accumulate=True)
        if "wkvT" not in pk:      # (the token rows' d z = d[k | v] . [Wk ; Wv]: built on first use, refresh() drops it with the rest)
            pk["wkvT"] = ops.transpose(pk["wqkv"][C:])
        kv, zh, zs = st["kv"], st["zh"], st["zs"]
        # out = h + scale * (o . Wc^T + bc)
        ops.wgrad(dout, st["o"], gv("sketch_conv.weight"), gv("sketch_conv.bias"), alpha=self.scale, **acc)
        do = ops.gemm(dout, pk["wcT"], alpha=self.scale)
        ops.wgrad(do, st["a"], gv("sketch_attn.to_out.0.weight"), gv("sketch_attn.to_out.0.bias"), **acc)
        da = ops.gemm(do, pk["woT"])
        # attention: per sample the N image rows are the queries, keys / values its N + T rows of the padded buffer
        dqkv = torch.empty(B * N, 3 * C, device=self.dev, dtype=torch.float16)
        dkv = torch.empty(B * L, 2 * C, device=self.dev, dtype=torch.float16)      # (pad rows: never written, never read)
        K, V = kv[:, :C], kv[:, C:]
        _, delta = ops.attn_bwd_dq_delta(st["q"], K, V, da, st["a"], st["lse"], B, heads, N, NT, L, dh, sc, out=dqkv[:, :C])
        ops.attn_bwd_dkv_strided(st["q"], K, V, da, st["lse"], delta, B, heads, N, NT, L, dh, sc, dkv[:, :C], dkv[:, C:])
        ops.batch_copy(dkv, L, dqkv[:, C:], N, B, N)                 # d[k | v] of the image rows next to their d q
        dkvs = torch.empty(B * T, 2 * C, device=self.dev, dtype=torch.float16)
        ops.batch_copy(dkv[N:], L, dkvs, T, B, T)                    # ... and of the token rows, dense
        ops.wgrad(dqkv[:, :C], zh, gv("sketch_attn.to_q.weight"), **acc)
        for j, leaf in ((0, "sketch_attn.to_k.weight"), (1, "sketch_attn.to_v.weight")):
            ops.wgrad(dqkv[:, (1 + j) * C:(2 + j) * C], zh, gv(leaf), **acc)
            ops.wgrad(dkvs[:, j * C:(1 + j) * C], zs, gv(leaf), **acc)
        dzh = ops.gemm(dqkv, pk["wqkvT"])
        dzs = ops.gemm(dkvs, pk["wkvT"])
        ng = w(f"{n}.sketch_norm.weight")
        ops.layernorm_param_grads(st["h"], dzh, st["sth"], gv("sketch_norm.weight"), gv("sketch_norm.bias"), **acc)
        ops.layernorm_param_grads(st["s"], dzs, st["sts"], gv("sketch_norm.weight"), gv("sketch_norm.bias"), **acc)
        ds = ops.layernorm_bwd(st["s"], dzs, ng, st["sts"])
        ops.wgrad(ds, self.state16.view(B * T, CLIP_DIM), gv("sketch_proj.weight"), gv("sketch_proj.bias"), **acc)
        self.dstate += ops.gemm(ds, pk["wpT"], out_f32=True).view(B, T, CLIP_DIM)
        return ops.layernorm_bwd(st["h"], dzh, ng, st["sth"], residual=dout)
