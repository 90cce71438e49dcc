"""SD-style UNet evaluated with the libskg.so kernels: forward (with feature taps) and
backward-to-input.

Replaces what the reference reaches through ``self.unet(...)`` at modules/pipeline.py:96
(diffusers UNet2DConditionModel -> cuDNN / cuBLAS / xformers kernels), the forward hooks of
modules/latent_predictor.py:47-81 (the nine taps) and the autograd pass triggered at
modules/pipeline.py:159.  Weights use the diffusers state_dict key names.

Data layout in HBM: every activation is fp16, token-major [rows*H*W, C]; rows are
ordered [uncond rows of all samples ; cond rows of all samples] so the backward pass (cond rows
only - the uncond gradient is discarded at modules/pipeline.py:159) works on a contiguous suffix
of every buffer, which is all a Stash keeps of it (a free view).  Weight-pack layouts: packs.py (which packs a net has: HipUNet._pack / _pack_hp here).

Work hoisted out of the per-step loop because it does not depend on the latent:
  * the time-embedding MLP and every ResnetBlock2D.time_emb_proj(silu(temb)) -> one fused bias
    vector per (timestep, resnet), folded into conv1's bias;
  * cross-attention K / V projections of the text embeddings (per prompt).
"""
from __future__ import annotations

import functools
import math
import os
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch

from . import ops
from .config import UNetConfig, up_block_plan
from .packs import (CIN_PAD, COUT_PAD, CTX_PAD, EPS_SEED_LD, _h, _pad_vec, pack_conv, pack_conv_dgrad,      # noqa: F401 (re-exported)
                    pack_conv_up2, pack_conv_up2_dgrad, pack_conv_up2_hilo, pack_conv_wino, pack_ff_block, pack_xattn_kv,
                    pack_xattn_weights)

_GN_FROM_PRODUCER = os.environ.get("SKG_GN_PRODUCER", "1") != "0"      # A/B switches (bench.py on one box)
_GN_CONCAT = os.environ.get("SKG_GN_CONCAT", "1") != "0"
_FF_BLOCK = os.environ.get("SKG_FF_BLOCK", "1") != "0"              # fused feed-forward sub-block at C = 320 (csrc/ffblock.hip)
_XATTN_BLOCK = os.environ.get("SKG_XATTN_BLOCK", "1") != "0"        # fused cross-attention sub-block at C = 320, 8 heads (csrc/xattn.hip)
_FF_KEEP = os.environ.get("SKG_FF_KEEP", "1") != "0"                # ... also in a guided step (stashing launch; 0 = all rows unfused there)
_XATTN_HEADS = (8,) if os.environ.get("SKG_XATTN_D64", "1") == "0" else (8, 5)     # head counts of the fused cross-attention launch at C = 320 (5 x 64: round 5)
# (head width, 16-key score tiles) pairs whose cross-attention over a long prompt (80 < Lp <= 240 key slots) asks for the LDS-resident
# forward (SKG_ATTN_RESIDENT_KV): the pairs that beat the streaming kernel by more than the run-to-run spread at both batch sizes of
# profiles/attn_resident_kv.txt - none did (EXPERIMENTS.md, long prompts), so the default is empty; SKG_RESIDENT_KV=1 routes every
# built pair (A/B runs)
_RESIDENT_KV_BUILT = frozenset({(40, 10), (40, 15), (64, 10), (64, 15), (80, 10), (80, 15), (160, 10)})
_RESIDENT_KV = _RESIDENT_KV_BUILT if os.environ.get("SKG_RESIDENT_KV", "0") == "1" else frozenset()
_XATTN_KEEP = os.environ.get("SKG_XATTN_KEEP", "1") != "0"          # the fused cross-attention launch also in guided steps (stashing launch)
_XATTN_KEEP_HP = os.environ.get("SKG_XATTN_KEEP_HP", "1") != "0"    # ... and in the accuracy mode's guided steps (pairs)
_FF_PROJ = os.environ.get("SKG_FF_PROJ", "1") != "0"                # proj_out + outer residual inside the fused feed-forward launch
_FF_PROJ_HP = os.environ.get("SKG_FF_PROJ_HP", "1") != "0"          # ... in the accuracy mode too (skg_ff_block_f16 with bias_proj on pairs, round 5)
_ATTN_DQ_DELTA = os.environ.get("SKG_ATTN_DQ_DELTA", "1") != "0"    # attention backward: delta inside the dQ launch (round 5)
_RES_SC = os.environ.get("SKG_RES_SC", "1") != "0"                  # conv2 + conv_shortcut of a ResnetBlock as one implicit GEMM (round 5)
# round 6: the ResnetBlock convolutions of the two deepest levels (16 x 16 / 8 x 8 at 64 x 64 latents) by Winograd F(2x2, 3x3) (csrc/wino.hip):
# 0 = off, 1 = conv1, conv2 without a shortcut and the data gradients, 2 (default) = also conv2 of the channel-changing blocks of the
# second-deepest level (shortcut GEMM + Winograd with a residual instead of the folded launch: 0.79-0.87 of its time at 16 x 16, 1.17 at
# 8 x 8 - profiles/r06_wino_bench.txt).  A launch takes the path with >= _WINO_MIN_TILES tile positions (output pixels / 4): at 128 - the
# cond-only backward of the 8 x 8 level - the 16 component GEMMs are 128 rows each and the implicit GEMM is as fast.
_WINO = int(os.environ.get("SKG_WINO", "2"))
_WINO_MIN_TILES = int(os.environ.get("SKG_WINO_MIN_TILES", "256"))  # tile positions (output pixels / 4) a launch needs to take the path
_WINO_GN = os.environ.get("SKG_WINO_GN", "1") != "0"                # the GroupNorm in front writes the Winograd input transform itself
# accuracy mode: Winograd also for the ResnetBlock convolutions of the PAIR zone's small maps (the 16 x 16 level with HP_PLAIN_LEVELS = 1):
# pair output through the output transform, the K-doubled shortcut as a pair GEMM whose result is the residual
_HP_WINO = os.environ.get("SKG_HP_WINO", "0") != "0"


# spatial sizes inside the UNet are (height, width) pairs; every level keeps the latent's aspect ratio (both sides are
# multiples of 2^(levels - 1), so each stride-2 level halves both exactly and each nearest-2x upsample lands on the skip's size)
def _half(sz: Tuple[int, int]) -> Tuple[int, int]:
    return (sz[0] // 2, sz[1] // 2)


def _dbl(sz: Tuple[int, int]) -> Tuple[int, int]:
    return (2 * sz[0], 2 * sz[1])


def _side(sz: Tuple[int, int]):
    """What a tap / residual sample carries as its size: the side s of a square map (the form of square evaluations),
    else (height, width)."""
    return sz[0] if sz[0] == sz[1] else sz


UP2_POLYPHASE = os.environ.get("SKG_UP2_POLY", "1") != "0"      # A/B switch (bench.py on one box)
# accuracy mode: 1 = the upsamplers' K-tripled form ([x_hi | x_lo | x_hi] . [W_hi | W_hi | W_lo]), 0 (default, round 5) = the default
# polyphase launch on x_hi with a pair output: both correction thirds together move eps by 3.6 % of the mode's distance from fp32
# (tools/eps_decompose_up.py) and cost two thirds of the upsamplers' time - the largest single item of the mode's price
HP_UP_TRIPLE = os.environ.get("SKG_HP_UP_TRIPLE", "0") != "0"
# accuracy mode (round 6): GroupNorm OUTPUTS kept as (hi, lo) pairs - the K-doubled operand [n_hi | n_lo] . [W | W] of the matmul that
# consumes them - at the sites whose fp16 rounding carries the most of the mode's remaining eps distance (tools/eps_decompose_sites.py:
# the norm outputs of the LAST up block are 66 % of its variance; conv_norm_out, 18 %, has been a pair since round 4).  Comma-separated
# norm names of the last up block ("<resnet>.norm1" / ".norm2" -> conv1 / conv2, "<attention>.norm" -> proj_in); "" = none (round 5).
# Default = eight of the nine sites (all but norm1 of the first ResnetBlock: the widest operand, 960 channels, for the smallest share),
# chosen together with HP_PLAIN_LEVELS = 1 AT THE REAL BATCH (profiles/r06_eps_real_batch.txt: configs[1]'s 8 samples x 3 timesteps = 48
# rows, ms per 16-row evaluation on one box): round 5's mode rel 5.41e-4 / worst max 1.03e-3 / 18.89 ms; plain 2 + 6 sites + Winograd
# 5.08e-4 / 9.8e-4 / 18.18; plain 1 + 6 sites 4.50e-4 / 8.4e-4 / 19.16; plain 1 + 9 sites 4.18e-4 / 8.1e-4 / 19.66; plain 0 + 9 sites
# 4.14e-4 / 7.7e-4 / 19.88: accuracy costs ~0.5 % of time per 1 % of rel along the whole front - the setting is where the worst row keeps
# ~15 % of north_star's bound (the throughput target has 60 % of headroom, the bound had 2 %).
# ("{last}" = the index of the last up block of the UNet at hand: 3 for SD1.x / SD2.x.)
HP_NORM_PAIRS = tuple(n for n in os.environ.get(
    "SKG_HP_NORM_PAIRS", "up_blocks.{last}.resnets.0.norm2,up_blocks.{last}.resnets.1.norm1,up_blocks.{last}.resnets.1.norm2,"
                         "up_blocks.{last}.resnets.2.norm1,up_blocks.{last}.resnets.2.norm2,up_blocks.{last}.attentions.0.norm,"
                         "up_blocks.{last}.attentions.1.norm,up_blocks.{last}.attentions.2.norm").split(",") if n)
# accuracy mode (round 6): the DEEPEST resolution levels run the default fp16 kernels - tools/eps_decompose_stream.py: of what the pairs
# (residual stream, conv outputs that feed a norm, stream-as-operand) buy, 60 % is bought in the last up block, 25 % in the first down block
# (its skips feed the last up block), 15 % at the 32 x 32 level, ~4 % at the 16 x 16 level and nothing at 8 x 8.  n = number of deepest
# levels (8 x 8, 16 x 16, ...) whose blocks run plain fp16: down_blocks[nb - n ..], mid_block, up_blocks[.. n - 1]; 0 = pairs everywhere.
HP_PLAIN_LEVELS = int(os.environ.get("SKG_HP_PLAIN_LEVELS", "1"))
UP2_SMALL_MAPS = os.environ.get("SKG_UP2_SMALL", "1") != "0"    # A/B: polyphase also where one phase does not fill the chip
UP2_DGRAD = os.environ.get("SKG_UP2_DGRAD", "1") != "0"         # A/B: the upsampler's backward as one 4 x 4 stride-2 convolution


@dataclass
class Stash:
    """Activations kept by a grad-enabled forward for the backward pass: of every tensor exactly the rows the backward
    differentiates, the last rows - first of the evaluation's batch rows (forward sets both before its first launch)."""
    res: Dict[str, dict] = field(default_factory=dict)
    tr: Dict[str, dict] = field(default_factory=dict)
    misc: dict = field(default_factory=dict)
    rows: int = 0          # batch rows of the evaluation
    first: int = 0         # the first differentiated row (forward's diff_from; rows // 2 without one)

    def suffix(self, key: str, v: Optional[torch.Tensor], unit: int) -> Optional[torch.Tensor]:
        """The view of v's last rows - first batch rows.  unit: tensor rows per batch row (HW for activations and per-token
        statistics, 1 for per-image tensors).  Every tensor a forward produces holds a suffix of the batch rows - all of them, the
        cond half of a shared CFG front, the rows a stashing launch kept - and how many is read off the tensor itself, so a wrong
        belief about a launch fails here, under the name `key`, not as a mis-slice in the backward.  None passes through."""
        if v is None:
            return None
        S, (n, rem) = self.rows - self.first, divmod(v.shape[0], unit)
        if rem or not S <= n <= self.rows:
            raise ValueError(f"stash {key}: {v.shape[0]} rows at {unit} per batch row - a suffix of {S} ... {self.rows} batch rows expected")
        return v if n == S else v[(n - S) * unit:]


class _Packs(dict):
    """Weight packs by name.  `lazy[k] = make` registers a pack that is only built (from a host copy of the tensor) the first time it
    is read: the packs of code paths that normally never run - the two-launch fall-back of a declined fused launch (they
    were ~0.5 GB of resident duplicates)."""

    def __init__(self):
        super().__init__()
        self.lazy: Dict[str, Callable[[], torch.Tensor]] = {}

    def __missing__(self, k):
        v = self[k] = self.lazy.pop(k)()         # (KeyError for a name that was never registered)
        return v

    def __contains__(self, k):
        return dict.__contains__(self, k) or k in self.lazy


def _hi(v):
    """The fp16 tensor of a value of either representation (taps, stashes and hi-only operands carry it)."""
    return v.hi if isinstance(v, ops.Pair) else v


def _rows_of(v, m0: int, m1: int):
    if isinstance(v, ops.Pair):
        return ops.Pair(v.hi[m0:m1], v.lo[m0:m1], None if v.full is None else v.full[m0:m1])
    return v[m0:m1]


def _copy_up(src, dst, M1: int):
    """Shared CFG front: the cond rows `src` (M1 of them, the second half of `dst`) -> the uncond rows of dst."""
    if not isinstance(src, ops.Pair):
        ops.batch_copy(src, M1, dst, M1, 1, M1)
    elif src.full is not None and dst.full is not None:
        ops.batch_copy(src.full, M1, dst.full, M1, 1, M1)
    else:
        ops.batch_copy(src.hi, M1, dst.hi, M1, 1, M1)
        ops.batch_copy(src.lo, M1, dst.lo, M1, 1, M1)


def _fresh(like, M: int, C: int):
    """An uninitialised [M, C] value of `like`'s representation."""
    if isinstance(like, ops.Pair):
        return ops.Pair.empty(M, C, like.hi.device)
    return torch.empty(M, C, device=like.device, dtype=torch.float16)


def _produce(fn: str, *args, out=None, residual=None, gn: Optional[Tuple[int, int]] = None, **kw):
    """ops.<fn> (gemm, conv3x3, conv3x3_sc, conv3x3_wino) with `out` / `residual` of either representation: a Pair goes in as
    out= / out_lo= (residual= / residual_lo=), its pair epilogue.  gn = (HW, groups): the GroupNorm partial sums of the output come
    with it.  -> (the output in the representation of `out`, a fresh fp16 tensor without one; the sums or None)."""
    for name, v in (("out", out), ("residual", residual)):
        if isinstance(v, ops.Pair):
            kw[name], kw[name + "_lo"] = v.hi, v.lo
        elif v is not None:
            kw[name] = v
    if gn is not None:
        kw.update({"gn_stats": gn} if fn == "gemm" else {"gn_groups": gn[1]})
    res = getattr(ops, fn)(*args, **kw)
    o, part = res if gn is not None else (res, None)
    return (out if isinstance(out, ops.Pair) else o), part


def per_sample_timesteps(t, rows: int, shared_input: bool = False):
    """What HipUNet.forward makes of its `t`: an int for one timestep shared by all rows (an int, or a sequence / 1-D integer tensor
    of `rows` equal entries), else the list of `rows` ints - a timestep per sample.  ValueError: a length other than `rows`, or
    shared_input (the two halves of the batch are identical) with halves whose timesteps differ row for row."""
    if torch.is_tensor(t):
        if t.dim() == 0:
            return int(t)
        if t.dim() != 1 or t.dtype.is_floating_point or t.dtype == torch.bool:
            raise ValueError(f"timesteps: an int or a 1-D integer tensor of length rows expected, got {tuple(t.shape)} {t.dtype}")
        ts = [int(v) for v in t.tolist()]
    elif isinstance(t, (list, tuple)):
        ts = [int(v) for v in t]
    else:
        return int(t)
    if len(ts) != rows:
        raise ValueError(f"timesteps: {len(ts)} entries for {rows} rows")
    if all(v == ts[0] for v in ts):
        return ts[0]
    if shared_input and (rows % 2 or ts[: rows // 2] != ts[rows // 2:]):
        raise ValueError("shared_input: the two halves of the batch must carry equal timesteps row for row")
    return ts


def _layernorm(v, gamma, beta, **kw):
    """LayerNorm of a value of either representation (a pair is normalised as hi + lo) -> fp16."""
    return ops.layernorm_hilo(v.hi, v.lo, gamma, beta, **kw) if isinstance(v, ops.Pair) else ops.layernorm(v, gamma, beta, **kw)


class _ConcatBuffers:
    """torch.cat((h, skip)) of the up path without copies: the buffer [h | skip] of every up resnet is filled in place - the
    down-path layer that produces a skip writes it straight into the right-hand columns (and keeps using that strided view as its
    own output), the up-path layer that produces h into the left-hand ones.  Buffer u belongs to up block u // (layers + 1); the
    skips are consumed in the reverse order of their production.  A buffer has the representation of its consumer: fp16 in the
    plain zone, else the pair buffer [h_hi | skip_hi | h_lo | skip_lo] - every view handed out then is an ops.Pair inside it."""

    def __init__(self, net: "HipUNet", rows: int, down_only: bool):
        cfg = net.cfg
        lpb1, rev = cfg.layers_per_block + 1, list(reversed(cfg.block_out_channels))
        n = len(rev) * lpb1
        self.ch_h = [rev[0] if u == 0 else (rev[u // lpb1 - 1] if u % lpb1 == 0 else rev[u // lpb1]) for u in range(n)]
        self.pair = [not net._plain_up(u // lpb1) for u in range(n)]
        self.bufs: List[Optional[torch.Tensor]] = [None] * n
        self.skips: list = []                                # every skip produced so far (what down_only returns) ...
        self.parts: List[Optional[ops.GNPartial]] = []       # ... and its GroupNorm partial sums, when its producer left them
        self.rows, self.dev, self.down_only, self.groups = rows, net.dev, down_only, cfg.norm_groups

    def _width(self, u: int) -> int:
        return self.bufs[u].shape[1] // (2 if self.pair[u] else 1)

    def skip_slot(self, ch_s: int, size: Tuple[int, int]):
        """The columns of the concat buffer that will consume the skip produced next (None when down_only: no up path follows);
        the producer's output goes to push()."""
        if self.down_only:
            return None
        u = len(self.bufs) - 1 - len(self.skips)
        ch, ct = self.ch_h[u], self.ch_h[u] + ch_s
        buf = self.bufs[u] = torch.empty(self.rows * size[0] * size[1], (2 if self.pair[u] else 1) * ct, device=self.dev,
                                         dtype=torch.float16)
        return ops.Pair(buf[:, ch:ct], buf[:, ct + ch:]) if self.pair[u] else buf[:, ch:]

    def push(self, skip, part):
        self.skips.append(skip)
        self.parts.append(part)

    def h_slot(self, u: int):
        """The left-hand columns of buffer u: where the up-path layer in front of it writes h."""
        buf, ch, ct = self.bufs[u], self.ch_h[u], self._width(u)
        return ops.Pair(buf[:, :ch], buf[:, ct:ct + ch]) if self.pair[u] else buf[:, :ch]

    def whole(self, u: int):
        buf, ct = self.bufs[u], self._width(u)
        return ops.Pair(buf[:, :ct], buf[:, ct:], buf) if self.pair[u] else buf

    def concat_part(self, u: int, hp):
        """GroupNorm partial sums of buffer u for its consumer's norm1 - hp (of h) and the skip's, regrouped - or None where either
        producer left none or the widths do not allow it."""
        sp = self.parts.pop()
        ch = self.ch_h[u]
        if _GN_CONCAT and hp is not None and sp is not None and ops.gn_concat_ok(ch, self._width(u) - ch, self.groups, hp.groups, sp.groups):
            return (hp, ch, sp)
        return None


class HipUNet:
    def __init__(self, cfg: UNetConfig, state_dict: Dict[str, torch.Tensor], device="cuda",
                 need_backward: bool = True, residual_fp32: bool = False):
        """residual_fp32: opt-in ACCURACY mode that meets north_star's <= 1e-3 max eps deviation from the fp32 reference: the
        residual stream and every conv output that feeds a norm or the residual sum are kept as (hi, lo) pairs of fp16 tensors
        (~22 mantissa bits), see forward().  Where the stream itself is a matmul operand the pair is the K-doubled
        operand (shortcuts, downsamplers, proj_out, conv_out) - EXCEPT the three nearest-2x upsampler convolutions, which read the hi
        part only and write a pair (round 5: SKG_HP_UP_TRIPLE=1 restores their pair operand; the declined-launch fall-back keeps the
        hi-only operand too).  Guided steps work: the pair forward stashes the hi activations and the ordinary backward runs on them."""
        self.cfg = cfg
        self.dev = torch.device(device)
        self.need_backward = need_backward
        self.residual_fp32 = residual_fp32
        self.W: Dict[str, torch.Tensor] = _Packs()
        self.hp_norm_pairs: set = set()
        nb = len(cfg.block_out_channels)
        # the zone: how many of the outermost resolution levels (level of down_blocks.i = i, of mid_block = nb - 1, of up_blocks.i =
        # nb - 1 - i) carry (hi, lo) pairs; the deeper levels - every level in the default mode, the HP_PLAIN_LEVELS deepest in the
        # accuracy mode - run the fp16 kernels
        self.pair_levels = nb - max(0, min(HP_PLAIN_LEVELS, nb - 1)) if residual_fp32 else 0
        self._pack(state_dict)
        if residual_fp32:
            assert all(c % 64 == 0 for c in cfg.block_out_channels), \
                "accuracy mode: the pair epilogue lives in the LDS-DMA kernels (channel counts must be multiples of 64)"
            self._pack_hp(state_dict)
        self._sd_time = {k: v for k, v in state_dict.items()
                         if k.startswith("time_embedding.") or ".time_emb_proj." in k or k.endswith("conv1.bias")}
        self.tbias: Dict[int, Dict[str, torch.Tensor]] = {}
        # the same rows as ONE [T, Cout] table per resnet (row tbias_row[t]): a timestep per sample is one gather per resnet
        self.tbias_tab: Dict[str, torch.Tensor] = {}
        self.tbias_row: Dict[int, int] = {}
        self.ctx: Optional[dict] = None
        self.inject: Optional[Callable] = None      # set by modules.*_guided_attn.SatMixin

    def _hp_plain(self, name: str) -> bool:
        """Does this module (state-dict prefix) run the default fp16 kernels?  Every one in the default mode; in the accuracy mode the
        blocks of the plain zone (HP_PLAIN_LEVELS), nothing outside the blocks (conv_in, conv_norm_out, conv_out)."""
        if not self.residual_fp32:
            return True
        part = name.split(".")
        if part[0] == "down_blocks":
            return self._plain_down(int(part[1]))
        if part[0] == "up_blocks":
            return self._plain_up(int(part[1]))
        return part[0] == "mid_block" and self._plain_up(0)

    def _plain_down(self, i: int) -> bool:
        return i >= self.pair_levels

    def _plain_up(self, i: int) -> bool:
        """up block i - and mid_block, which shares the level of up block 0"""
        return len(self.cfg.block_out_channels) - 1 - i >= self.pair_levels

    # ------------------------------------------------------------------ packing
    def _pack(self, sd):
        W, dev, bw = self.W, self.dev, self.need_backward
        # ResnetBlocks whose conv2 + conv_shortcut run as ONE implicit GEMM (ops.conv3x3_sc): the forward packs of the two separate
        # launches are only read when that launch is declined (an operand >= 2 GiB) - registered lazily, from fp16 host copies
        folded = set()
        if _RES_SC:
            for k, v in sd.items():
                if k.endswith(".conv_shortcut.weight"):
                    r = k[: -len(".conv_shortcut.weight")]
                    if sd[r + ".conv2.weight"].shape[1] % 64 == 0 and v.shape[1] % 64 == 0:
                        folded.add(r)

        def lazy(key, tensor, make):
            host = tensor.detach().to("cpu", torch.float16)
            W.lazy[key] = lambda: make(host)

        for k, v in sd.items():
            r = k.rsplit(".", 2)[0]
            if r in folded and k.endswith(".conv2.weight"):
                lazy(k, v, lambda h: pack_conv(h, dev))
                if bw:
                    W[k + ":T"] = pack_conv_dgrad(v, dev)
                continue
            if r in folded and k.endswith(".conv_shortcut.weight"):
                lazy(k, v, lambda h: _h(h.reshape(h.shape[0], h.shape[1]), dev))
                if bw:
                    W[k + ":T"] = _h(v.reshape(v.shape[0], v.shape[1]).t(), dev)
                continue
            if v.dim() == 4 and v.shape[2] == 3:
                if k == "conv_in.weight":
                    W[k] = pack_conv(v, dev, cin_pad=CIN_PAD)
                    if bw:
                        W[k + ":T"] = pack_conv_dgrad(v, dev, cin_pad=COUT_PAD)
                elif k == "conv_out.weight":
                    W[k] = pack_conv(v, dev, cout_pad=COUT_PAD)
                    if bw:      # backward from eps (backward_eps): d eps arrives in EPS_SEED_LD columns, 4 of them valid
                        W[k + ":T"] = pack_conv_dgrad(v, dev, cout_pad=EPS_SEED_LD)
                else:
                    W[k] = pack_conv(v, dev)
                    if bw:
                        W[k + ":T"] = pack_conv_dgrad(v, dev)
                    if ".upsamplers." in k and UP2_POLYPHASE and v.shape[1] % 64 == 0:
                        W[k + ":pp"] = pack_conv_up2(v, dev)
                        if bw and v.shape[0] % 64 == 0:
                            W[k + ":ppT"] = pack_conv_up2_dgrad(v, dev)
            elif v.dim() == 4:                                  # 1x1 conv
                W[k] = _h(v.reshape(v.shape[0], v.shape[1]), dev)
                if bw:
                    W[k + ":T"] = _h(v.reshape(v.shape[0], v.shape[1]).t(), dev)
            elif v.dim() == 2:
                if ".attn1.to_" in k and not k.endswith("to_out.0.weight"):
                    continue                                    # fused below
                if ".attn2.to_k." in k or ".attn2.to_v." in k:
                    W[k] = _h(v, dev)                            # used once per prompt
                    continue
                if ".time_emb" in k:
                    W[k] = _h(v, dev)
                    continue
                W[k] = _h(v, dev)
                if bw:
                    W[k + ":T"] = _h(v.t(), dev)
            else:
                W[k] = _h(_pad_vec(v, COUT_PAD) if k == "conv_out.bias" else v, dev)
        # conv2 + conv_shortcut as ONE implicit GEMM (ops.conv3x3_sc): [conv2 tap-major pack | W_sc] along K, biases summed
        if _WINO and len(self.cfg.block_out_channels) >= 3:
            nb = len(self.cfg.block_out_channels)
            for blk, deepest in ((f"down_blocks.{nb - 2}.", False), ("up_blocks.1.", False), (f"down_blocks.{nb - 1}.", True),
                                 ("mid_block.", True), ("up_blocks.0.", True)):
                for k, v in sd.items():
                    if k.startswith(blk) and ".resnets." in k and (k.endswith(".conv1.weight") or k.endswith(".conv2.weight")) and v.shape[1] % 64 == 0:
                        if deepest and k.endswith(".conv2.weight") and (k[: -len(".conv2.weight")] + ".conv_shortcut.weight") in sd:
                            continue      # (8 x 8: the folded shortcut launch stays ahead of shortcut GEMM + Winograd)
                        if self._hp_plain(k) or _HP_WINO:      # (accuracy mode: the forward of a pair-zone block takes Winograd only with SKG_HP_WINO)
                            W[k + ":wino"] = pack_conv_wino(v, dev)
                        if bw and v.shape[0] % 64 == 0 and not deepest:      # (the deepest level's cond-only backward stays on the implicit GEMM)
                            W[k + ":winoT"] = pack_conv_wino(v, dev, dgrad=True)
        for r in sorted(folded):
            w2, wsc = sd[r + ".conv2.weight"], sd[r + ".conv_shortcut.weight"]
            wsc = wsc.reshape(wsc.shape[0], wsc.shape[1])
            w2p = w2.permute(0, 2, 3, 1).reshape(w2.shape[0], -1)                   # [Cout][ky][kx][Cin] (pack_conv's order)
            if not self._hp_plain(r):   # (the accuracy mode's pair blocks read only :sc2 - the pair operand [x_hi | x_lo] . [W | W] - and the summed bias)
                W[r + ".conv2.weight:sc2"] = _h(torch.cat([w2p, wsc, wsc], 1), dev)
            else:
                W[r + ".conv2.weight:sc"] = _h(torch.cat([w2p, wsc], 1), dev)
            W[r + ".conv2.bias:sc"] = _h(sd[r + ".conv2.bias"].float() + sd[r + ".conv_shortcut.bias"].float(), dev)
        # FF1 (GEGLU projection): rows interleaved [a a g g] so the GEMM epilogue can gate in registers
        for k in list(sd.keys()):
            if k.endswith(".ff.net.0.proj.weight"):
                idx = ops.geglu_interleave_index(sd[k].shape[0] // 2)
                W[k] = _h(sd[k][idx], dev)
                W[k[:-len("weight")] + "bias"] = _h(sd[k[:-len("weight")] + "bias"][idx], dev)
                if bw:
                    W[k + ":T"] = _h(sd[k][idx].t(), dev)
        # first level (C = 320; SD1.5: 8 heads of 40, SD2.1: 5 heads of 64): norm2 -> to_q -> text attention -> to_out + residual as
        # ONE row-local launch (csrc/xattn.hip); the per-prompt K / V packs are made in prepare_context
        cfg = self.cfg
        heads320 = cfg.num_heads[list(cfg.block_out_channels).index(320)] if 320 in cfg.block_out_channels else None
        for k in list(sd.keys()):
            if k.endswith(".attn2.to_q.weight") and sd[k].shape == (320, 320) and heads320 in _XATTN_HEADS:
                t = k[: -len(".to_q.weight")]
                W[t + ".xpack"] = pack_xattn_weights(sd[k], sd[t + ".to_out.0.weight"], heads320, dev)
        # 64 x 64 level (C = 320): the whole feed-forward sub-block as ONE row-local launch (csrc/ffblock.hip)
        for k in list(sd.keys()):
            if k.endswith(".ff.net.0.proj.weight") and sd[k].shape[1] == 320 and sd[k].shape[0] // 2 <= 1280:
                t = k[: -len(".ff.net.0.proj.weight")]
                # (with Transformer2DModel.proj_out behind it when the block has one of the same width: skg_ff_block_f16 with bias_proj;
                # the plain launch reads the leading chunks of the same tensor)
                tp = t[: -len(".transformer_blocks.0")] if t.endswith(".transformer_blocks.0") else None
                wpj = sd.get(tp + ".proj_out.weight") if tp else None
                wpj = wpj.reshape(wpj.shape[0], -1) if wpj is not None and wpj.numel() == 320 * 320 else None
                packp, W[t + ".ff.bias1"] = pack_ff_block(sd[k], sd[t + ".ff.net.0.proj.bias"], sd[t + ".ff.net.2.weight"], dev, w_proj=wpj)
                nchf = sd[k].shape[0] // 64
                W[t + ".ff.pack"] = packp[:nchf]
                if wpj is not None:
                    W[t + ".ff.packp"] = packp
        for k in list(sd.keys()):
            if k.endswith(".attn1.to_q.weight"):
                p = k[: -len(".to_q.weight")]
                qkv = torch.cat([sd[p + ".to_q.weight"], sd[p + ".to_k.weight"], sd[p + ".to_v.weight"]], 0)
                W[p + ".qkv"] = _h(qkv, dev)
                if bw:
                    W[p + ".qkv:T"] = _h(qkv.t(), dev)

    def _pack_hp(self, sd):
        """Accuracy mode: where the residual stream itself is a matmul operand (conv_shortcut, the resampling
        convolutions, proj_out) the operand is the PAIR [hi | lo] along K and the weight pack is [W | W]."""
        W, dev = self.W, self.dev
        for k, v in sd.items():
            if self._hp_plain(k):       # (a block of the deepest levels: runs the default kernels, HP_PLAIN_LEVELS)
                continue
            if k.endswith(".conv_shortcut.weight") and (k[: -len(".conv_shortcut.weight")] + ".conv2.weight:sc2") in W:
                host = v.detach().to("cpu", torch.float16)          # (fall-back of a declined conv3x3_sc launch only)
                W.lazy[k + ":2"] = lambda h=host: _h(torch.cat([h.reshape(h.shape[0], h.shape[1])] * 2, 1), dev)
            elif k.endswith(".conv_shortcut.weight") or k.endswith(".proj_out.weight"):
                w = v.reshape(v.shape[0], v.shape[1])
                W[k + ":2"] = _h(torch.cat([w, w], 1), dev)
            elif ".downsamplers." in k and k.endswith(".weight") or ".upsamplers." in k and k.endswith(".weight"):
                if ".upsamplers." in k and UP2_POLYPHASE and v.shape[1] % 64 == 0:
                    if getattr(self, "_sd_cpu", None) is None:
                        self._sd_cpu = {}
                    self._sd_cpu[k] = v.detach().to("cpu", torch.float16)      # (source of the 9-tap fall-back pack: _w9x2)
                    if HP_UP_TRIPLE or (k + ":pp") not in W:
                        W[k + ":pp3"] = pack_conv_up2_hilo(v, dev)  # polyphase with (hi, lo) pre-summed weights, K tripled
                    # (else: the default polyphase pack W[k + ":pp"] on x_hi, pair output only)
                else:
                    W[k + ":2"] = pack_conv(torch.cat([v, v], 1), dev)
            elif k == "conv_out.weight":      # its operand - the last normalised activation - reaches eps one to one: a pair too
                W[k + ":2"] = pack_conv(torch.cat([v, v], 1), dev, cout_pad=COUT_PAD)
        # norm outputs as pairs (HP_NORM_PAIRS): the [W | W] pack of the matmul behind each listed norm
        self.hp_norm_pairs = set()
        for name in HP_NORM_PAIRS:
            name = name.replace("{last}", str(len(self.cfg.block_out_channels) - 1))
            r, which = name.rsplit(".", 1)
            if which == "norm" and (r + ".proj_in.weight") in sd:
                w = sd[r + ".proj_in.weight"]
                w = w.reshape(w.shape[0], w.shape[1])
                W[r + ".proj_in.weight:n2"] = _h(torch.cat([w, w], 1), dev)
            elif which == "norm1" and (r + ".conv1.weight") in sd:
                W[r + ".conv1.weight:n2"] = pack_conv(torch.cat([sd[r + ".conv1.weight"]] * 2, 1), dev)
            elif which == "norm2" and (r + ".conv2.weight") in sd:
                w2 = sd[r + ".conv2.weight"]
                w2p = torch.cat([w2, w2], 1).permute(0, 2, 3, 1).reshape(w2.shape[0], -1)      # per tap [W | W]
                if (r + ".conv2.weight:sc2") in W:      # folded shortcut: [conv2 taps on the pair | W_sc | W_sc]
                    wsc = sd[r + ".conv_shortcut.weight"]
                    wsc = wsc.reshape(wsc.shape[0], wsc.shape[1])
                    W[r + ".conv2.weight:n2"] = _h(torch.cat([w2p, wsc, wsc], 1), dev)
                else:
                    W[r + ".conv2.weight:n2"] = _h(w2p, dev)
            elif "SKG_HP_NORM_PAIRS" in os.environ:
                raise ValueError(f"SKG_HP_NORM_PAIRS: {name!r} is not a GroupNorm of this UNet")
            else:
                continue                   # (a default site this architecture does not have: fewer layers per block)
            self.hp_norm_pairs.add(name)

    def _w9x2(self, k: str) -> torch.Tensor:
        """The 9-tap [W | W] pack of an upsampler (accuracy mode), built on first use: only a declined polyphase launch needs it."""
        if k + ":2" not in self.W:
            v = self._sd_cpu[k] if getattr(self, "_sd_cpu", None) is not None else None
            if v is None:
                raise RuntimeError(f"{k}: the polyphase launch was declined and the layer's 9-tap pack is not available")
            self.W[k + ":2"] = pack_conv(torch.cat([v, v], 1), self.dev)
        return self.W[k + ":2"]

    # ------------------------------------------------------------------ hoisted precompute
    def prepare_timesteps(self, timesteps: Sequence[int]):
        """Time-embedding MLP and the per-resnet time projections for every timestep of the schedule
        (diffusers get_timestep_embedding(flip_sin_to_cos=True, shift 0) -> TimestepEmbedding ->
        ResnetBlock2D.time_emb_proj(silu(.))), folded with conv1.bias."""
        cfg, W = self.cfg, self.W
        ts = list(dict.fromkeys(int(t) for t in timesteps if int(t) not in self.tbias))
        if not ts:
            return
        c0 = cfg.block_out_channels[0]
        half = c0 // 2
        expo = -math.log(10000.0) * torch.arange(half, dtype=torch.float32) / half
        emb = torch.tensor(ts, dtype=torch.float32)[:, None] * torch.exp(expo)[None, :]
        emb = torch.cat([torch.cos(emb), torch.sin(emb)], dim=-1)              # host table, fp32
        e = emb.to(self.dev, torch.float16).contiguous()
        e = ops.gemm(e, W["time_embedding.linear_1.weight"], bias=W["time_embedding.linear_1.bias"])
        e = ops.silu(e)
        e = ops.gemm(e, W["time_embedding.linear_2.weight"], bias=W["time_embedding.linear_2.bias"])
        e = ops.silu(e)                                                          # silu(temb), [T, 4*c0]
        out = {t: {} for t in ts}
        for k in W:
            if k.endswith(".time_emb_proj.weight"):
                p = k[: -len(".time_emb_proj.weight")]
                proj = ops.gemm(e, W[k], bias=W[p + ".time_emb_proj.bias"])       # [T, Cout]
                fused = ops.axpby(proj, W[p + ".conv1.bias"].expand(len(ts), -1).contiguous())
                for i, t in enumerate(ts):
                    out[t][p] = fused[i].contiguous()
                self.tbias_tab[p] = torch.cat([self.tbias_tab[p], fused]) if p in self.tbias_tab else fused
        for t in ts:
            self.tbias_row[t] = len(self.tbias_row)
        self.tbias.update(out)

    def prepare_context(self, ehs: torch.Tensor):
        """Cross-attention K / V of the text embeddings, per transformer block.  ehs [rows, L, D] in the
        row order [uncond rows; cond rows]."""
        cfg, W = self.cfg, self.W
        rows, L, D = ehs.shape
        Lp = (L + CTX_PAD - 1) // CTX_PAD * CTX_PAD
        Dp = (D + 31) // 32 * 32
        x = torch.zeros(rows, Lp, Dp, device=self.dev, dtype=torch.float16)
        x[:, :L, :D] = ehs.to(self.dev, torch.float16)
        x = x.reshape(rows * Lp, Dp)
        S = rows // 2
        ctx = dict(L=L, Lp=Lp, rows=rows, blocks={})
        for k in W:
            if k.endswith(".attn2.to_k.weight"):
                p = k[: -len(".to_k.weight")]
                wk, wv = W[k], W[p + ".to_v.weight"]
                if Dp != D:
                    wk = torch.nn.functional.pad(wk, (0, Dp - D)).contiguous()
                    wv = torch.nn.functional.pad(wv, (0, Dp - D)).contiguous()
                Kc = ops.gemm(x, wk)                     # padded token rows are exactly zero (zero input, no bias)
                Vc = ops.gemm(x, wv)
                ctx["blocks"][p] = dict(K=Kc, V=Vc)
                if (p + ".xpack") in W and L <= 80:
                    ctx["blocks"][p]["kvpack"] = pack_xattn_kv(Kc, Vc, rows, Lp, L, W[p + ".xpack"].shape[0])
        self.ctx = ctx

    # ------------------------------------------------------------------ modules, forward
    def _gn_from_producer(self, rows: int, HW: int, C: int) -> bool:
        """GroupNorm inputs of the 64 x 64 / 32 x 32 levels get their statistics from the epilogue of the kernel that
        writes them (ops.gemm / ops.conv3x3 with gn_stats= / gn_groups=): the separate statistics pass - a second read of
        a 10-40 MB tensor - disappears.  Smaller maps keep the one-launch GroupNorm that holds a slice in registers."""
        return _GN_FROM_PRODUCER and HW >= 1024 and ops.gn_fusable(rows * HW, C, HW, self.cfg.norm_groups)

    def _wino_ok(self, key: str, rows: int, sz: Tuple[int, int]) -> bool:
        return key in self.W and rows * sz[0] * sz[1] // 4 >= _WINO_MIN_TILES and not (sz[0] & 1) and not (sz[1] & 1)

    def _conv_wino(self, key: str, x, rows: int, sz: Tuple[int, int], **kw):
        """The 3x3 convolution `key` (a weight name + ':wino' / ':winoT') by Winograd F(2x2, 3x3) when the pack exists and the launch is
        large enough (out= / residual=: fp16 or Pair, see _produce); None when the path does not take it (the caller runs the
        implicit GEMM)."""
        if not self._wino_ok(key, rows, sz):
            return None
        try:
            return _produce("conv3x3_wino", x, self.W[key], rows, *sz, **kw)[0]
        except ops.SkgError as e:      # declined (no room for the slabs in the stream's workspace)
            if e.rc != -2:
                raise
            return None

    def _gn_conv_wino(self, nkey: str, wkey: str, x, rows: int, sz: Tuple[int, int], eps: float, **kw):
        """GroupNorm + SiLU `nkey` and the Winograd convolution `wkey` behind it with the norm writing the convolution's input transform
        (ops.groupnorm_wino: no normalised tensor in memory; fp16 only).  -> (conv output, statistics), or None when either step
        declines (nothing was consumed: the caller runs groupnorm and the convolution as before)."""
        if not _WINO_GN or not self._wino_ok(wkey, rows, sz):
            return None
        W = self.W
        try:
            V, st = ops.groupnorm_wino(x, rows, *sz, self.cfg.norm_groups, eps, W[nkey + ".weight"], W[nkey + ".bias"], True)
            return ops.conv3x3_wino(None, W[wkey], rows, *sz, V=V, **kw), st
        except ops.SkgError as e:
            if e.rc != -2:
                raise
            return None

    def _norm(self, x, rows: int, HW: int, eps: float, name: str, silu: bool, partial=None, pair_out: bool = False):
        """GroupNorm(+SiLU) `name` of x (fp16 or Pair) -> (normalised fp16 tensor, statistics [rows, groups, 2]); partial: the producer's
        epilogue sums.  pair_out, or a norm listed in hp_norm_pairs (pair input only): the output is a pair too - an ops.Pair whose
        .full is the K-doubled operand [hi | lo] of its consumer."""
        args = (rows, HW, self.cfg.norm_groups, eps, self.W[name + ".weight"], self.W[name + ".bias"], silu)
        if not isinstance(x, ops.Pair):
            return ops.groupnorm(x, *args, partial=partial)
        if not (pair_out or name in self.hp_norm_pairs):
            return ops.groupnorm_hilo(x.hi, x.lo, *args, want_stats=True, partial=partial)
        n = _fresh(x, *x.hi.shape)
        _, st = ops.groupnorm_hilo(x.hi, x.lo, *args, out=n.hi, out_lo=n.lo, want_stats=True, partial=partial)
        return n, st

    def _operand(self, v, key: str, suffix: str):
        """(A, B) of the contraction `key` that reads v: a pair is the K-doubled operand [hi | lo] against the [W | W] pack
        `key + suffix` (':2' where the stream is the operand, ':n2' behind a norm with a pair output)."""
        return (self._full_of(v), self.W[key + suffix]) if isinstance(v, ops.Pair) else (v, self.W[key])

    def _shortcut(self, p: str, x, M: int, Cout: int):
        """What conv2 of ResnetBlock p adds as its residual when the shortcut is not folded into its launch: the block input, or
        conv_shortcut of it (x's representation)."""
        if (p + ".conv_shortcut.weight") not in self.W:
            return x
        return _produce("gemm", *self._operand(x, p + ".conv_shortcut.weight", ":2"), out=_fresh(x, M, Cout),
                        bias=self.W[p + ".conv_shortcut.bias"])[0]

    def _res_fwd(self, p, x, rows, sz, tb, stash: Optional[Stash], out=None, xpart=None, want_part=False):
        """x: fp16, or a Pair in the accuracy mode's pair zone - the output (and conv1's, which feeds norm2) has its representation.
        xpart: GroupNorm partial sums of x from its producer (or None).  Returns (out, partial sums of out or None):
        they are produced when want_part is set and the level takes its statistics from the producers.
        `rows` may be the COND rows only (the shared CFG prefix, see forward): the stash keeps the differentiated rows either way."""
        W, pair = self.W, isinstance(x, ops.Pair)
        G, HW, M = self.cfg.norm_groups, sz[0] * sz[1], rows * sz[0] * sz[1]
        k1, k2 = p + ".conv1.weight", p + ".conv2.weight"
        Cout = W[k1].shape[0]
        fuse = self._gn_from_producer(rows, HW, Cout)
        # small maps (no statistics from the producers): conv1 / conv2 by Winograd F(2x2, 3x3) - in the pair zone under _HP_WINO only, and
        # never with the norm in front writing the input transform (ops.groupnorm_wino has no pair input) or for a norm output that is a pair
        wino1 = not fuse and (not pair or _HP_WINO)
        h1 = st1 = part1 = None
        if wino1 and not pair and xpart is None:
            h1, st1 = self._gn_conv_wino(p + ".norm1", k1 + ":wino", x, rows, sz, 1e-5, bias=tb[p]) or (None, None)
        if h1 is None:
            n1, st1 = self._norm(x, rows, HW, 1e-5, p + ".norm1", True, partial=xpart)
            h1o = _fresh(x, M, Cout)
            if wino1 and not isinstance(n1, ops.Pair):
                h1 = self._conv_wino(k1 + ":wino", n1, rows, sz, out=h1o, bias=tb[p])
            if h1 is None:
                h1, part1 = _produce("conv3x3", *self._operand(n1, k1, ":n2"), rows, *sz, out=h1o, bias=tb[p], gn=(HW, G) if fuse else None)
        out = _fresh(x, M, Cout) if out is None else out
        ogn = (HW, G) if want_part and fuse else None
        has_sc = (p + ".conv_shortcut.weight") in W
        # (fp16: also a large map whose consumer folds no sums; a channel-changing block takes shortcut GEMM + Winograd from _WINO = 2 on)
        wino2 = ((wino1 or not (pair or want_part)) and self._wino_ok(k2 + ":wino", rows, sz) and (pair or not has_sc or _WINO >= 2))
        n2 = st2 = sc = opart = None
        done = False
        if wino2 and not pair:
            # Winograd conv2 with the block input - or the shortcut GEMM's output - as its residual
            sc = self._shortcut(p, x, M, Cout)
            got = self._gn_conv_wino(p + ".norm2", k2 + ":wino", h1, rows, sz, 1e-5, out=out, bias=W[p + ".conv2.bias"], residual=sc)
            if got is not None:
                (out, st2), done = got, True
        if not done:
            n2, st2 = self._norm(h1, rows, HW, 1e-5, p + ".norm2", True, partial=part1)
        n2_pair = isinstance(n2, ops.Pair)
        if wino2 and not done and not n2_pair:
            sc = self._shortcut(p, x, M, Cout) if sc is None else sc
            done = self._conv_wino(k2 + ":wino", n2, rows, sz, out=out, bias=W[p + ".conv2.bias"], residual=sc) is not None
        a2 = n2.full if n2_pair else n2
        ksc = k2 + (":sc2" if pair else ":sc")
        if not done and ksc in W:
            # the 1x1 shortcut as K tiles behind conv2's 3x3 walk: one launch, no [M, Cout] round trip of the shortcut output (pair zone:
            # the K-doubled shortcut [x_hi | x_lo] . [W_sc | W_sc]; behind a norm with a pair output the folded pack is ':n2')
            try:
                out, opart = _produce("conv3x3_sc", a2, self._full_of(x) if pair else x, W[k2 + ":n2"] if n2_pair else W[ksc], rows, *sz,
                                      out=out, bias=W[p + ".conv2.bias:sc"], gn=ogn)
                done = True
            except ops.SkgError as e:      # declined (an operand >= 2 GiB): the two launches
                if e.rc != -2:
                    raise
        if not done:
            sc = self._shortcut(p, x, M, Cout) if sc is None else sc
            # (behind a norm with a pair output conv2's own [W | W] taps are the leading columns of its ':n2' pack, made contiguous)
            w2 = W[k2 + ":n2"][:, : 9 * a2.shape[1]].contiguous() if n2_pair else W[k2]
            out, opart = _produce("conv3x3", a2, w2, rows, *sz, out=out, bias=W[p + ".conv2.bias"], residual=sc, gn=ogn)
        if stash is not None:      # (the backward differentiates the fp16 - hi - values in either mode)
            k = lambda name, v, unit=HW: stash.suffix(f"{p}.{name}", v, unit)
            stash.res[p] = dict(x=k("x", _hi(x)), st1=k("st1", st1, 1), h1=k("h1", _hi(h1)), st2=k("st2", st2, 1), sz=sz)
        return out, opart

    def _tr_fwd(self, p, x, rows, sz, heads, stash: Optional[Stash], out=None, xpart=None, want_part=False, shared=False,
                x_full=None, diff_from: Optional[int] = None):
        """x: fp16 or a Pair (the pair zone): p1, p2, p3, pin and the output have its representation, q2 / qkv are fp16.
        shared: x holds the COND rows only (rows // 2 of them) of a CFG-doubled batch whose two halves are identical up
        to here (see forward): everything in front of the first text-dependent operation - GroupNorm, proj_in, the whole
        self-attention, LayerNorm 2, to_q - runs once; p1 and q2 are written into the cond half of full-size buffers and
        copied to the uncond half (x_full: the same for x, filled by the caller).
        diff_from (forward's; None: rows // 2): selects the split / fused stashing launches and the first row they keep."""
        cfg, W, pair = self.cfg, self.W, isinstance(x, ops.Pair)
        HW, M = sz[0] * sz[1], rows * sz[0] * sz[1]
        C = _hi(x).shape[1]
        dh = C // heads
        scale = dh ** -0.5
        t = p + ".transformer_blocks.0"
        keep = stash is not None
        r1 = rows // 2 if shared else rows                    # rows of the text-independent part
        M1, M0 = r1 * HW, (rows // 2 if diff_from is None else diff_from) * HW      # M0: the first stashed row of a stashing launch
        # the split / fused stashing launches: the sampler's even CFG-doubled batches, or any batch with an explicit diff_from
        split = diff_from is not None or rows % 2 == 0
        ln = lambda v, k: _layernorm(v, W[f"{t}.{k}.weight"], W[f"{t}.{k}.bias"], want_stats=True)
        g, gst = self._norm(x, r1, HW, 1e-6, p + ".norm", False, partial=xpart)
        pin, _ = _produce("gemm", *self._operand(g, p + ".proj_in.weight", ":n2"), out=_fresh(x, M1, C), bias=W[p + ".proj_in.bias"])
        a1, st1 = ln(pin, "norm1")
        qkv = ops.gemm(a1, W[t + ".attn1.qkv"])
        # V straight out of the fused projection (row-major; the kernel's LDS transpose read replaces the V^T copy)
        o1, lse1 = ops.attn_fwd(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], r1, heads, HW, HW, HW, dh, scale,
                                want_lse=True, v_rows=True)
        p1_full = _fresh(x, M, C) if shared else None
        p1, _ = _produce("gemm", o1, W[t + ".attn1.to_out.0.weight"], out=_rows_of(p1_full, M1, M) if shared else _fresh(x, M, C),
                         bias=W[t + ".attn1.to_out.0.bias"], residual=pin)
        x_c, p1_c = x, p1                                     # what the backward of the cond rows reads
        if self.inject is not None:
            if shared and getattr(self.inject, "halves_equal", False):
                # the injected K / V are the same for both halves too (checked by the injector): stay shared through it
                p1_full = _fresh(x, M, C)
                p1 = self.inject(t, p1, rows, HW, heads, cond_only=True, out=_rows_of(p1_full, M1, M))
            else:
                if shared:                                    # the injected K / V differ between the halves: diverge here
                    _copy_up(p1, p1_full, M1)
                    x, p1, shared = x_full, p1_full, False
                p1 = self.inject(t, p1, rows, HW, heads)
            p1_c = p1
        cb = self.ctx["blocks"][t + ".attn2"]
        xab = (_XATTN_BLOCK and (not keep or ((_XATTN_KEEP_HP if pair else _XATTN_KEEP) and split)) and "kvpack" in cb
               and heads in _XATTN_HEADS and HW % 128 == 0)
        if xab:
            # norm2 -> to_q -> attention over the text keys -> to_out + residual in ONE row-local launch (skg_xattn_block_f16[_hilo]);
            # the text-dependent part needs both halves, so a shared front ends here
            if shared:
                _copy_up(p1, p1_full, M1)
                x, p1, shared = x_full, p1_full, False
            xargs = (HW, heads, self.ctx["L"], W[t + ".norm2.weight"], W[t + ".norm2.bias"], 1e-5, W[t + ".attn2.xpack"], cb["kvpack"],
                     W[t + ".attn2.to_out.0.bias"], scale)
            if keep:
                # guided step: the same launch also stores what the backward of the cond rows (second half) reads - norm2's
                # statistics, q, the attention output and its lse (skg_xattn_block_f16[_hilo]_keep), for those rows only
                p2, st2, q2_c, o2, lse2 = ops.xattn_block(p1, *xargs, keep_from=M0)
            else:
                p2 = ops.xattn_block(p1, *xargs)
                st2 = q2_c = o2 = lse2 = None                 # (only a stash would read them, and there is none)
        else:
            a2, st2 = ln(p1, "norm2")
            q2_full = torch.empty(M, C, device=self.dev, dtype=torch.float16) if shared else None
            q2 = q2_c = ops.gemm(a2, W[t + ".attn2.to_q.weight"], q2_full[M1:] if shared else None)
            if shared:      # the text-dependent part needs both halves: one copy each into the uncond half
                _copy_up(p1, p1_full, M1)
                ops.batch_copy(q2, M1, q2_full, M1, 1, M1)
                x, p1, q2 = x_full, p1_full, q2_full
            Lp = self.ctx["Lp"]      # a long prompt's keys (encode_tokens: 78 ... 231) stay in LDS where that measured faster
            o2, lse2 = ops.attn_fwd(q2, cb["K"], cb["V"], rows, heads, HW, self.ctx["L"], Lp, dh, scale, want_lse=True, v_rows=True,
                                    resident_kv=80 < Lp <= 240 and (dh, 10 if Lp <= 160 else 15) in _RESIDENT_KV)
            p2, _ = _produce("gemm", o2, W[t + ".attn2.to_out.0.weight"], out=_fresh(x, M, C), bias=W[t + ".attn2.to_out.0.bias"], residual=p1)
        # C = 320: norm3 -> FF1 -> gate -> FF2 + residual in ONE row-local launch (skg_ff_block_f16[_hilo]: the row panel and the output
        # accumulators stay in registers, only weights stream).  In a guided step the same launch also stores what the backward of
        # the cond rows reads: the FF1 output (interleaved pack) and norm3's statistics
        ffb = _FF_BLOCK and (t + ".ff.pack") in W and (not keep or (split and _FF_KEEP))
        ffp = ffb and _FF_PROJ and (not pair or _FF_PROJ_HP) and (t + ".ff.packp") in W and HW % 128 == 0
        gn = (HW, cfg.norm_groups) if want_part and self._gn_from_producer(rows, HW, C) else None
        out = _fresh(x, M, C) if out is None else out
        f = st3 = opart = None
        if ffb:
            ffargs = (W[t + ".norm3.weight"], W[t + ".norm3.bias"], 1e-5, W[t + (".ff.packp" if ffp else ".ff.pack")], W[t + ".ff.bias1"],
                      W[t + ".ff.net.2.bias"])
            if ffp:
                # ... and proj_out + the outer residual behind it in the same launch (skg_ff_block_f16 with bias_proj): the block output
                # p3 never reaches memory (no backward reads it); GroupNorm partial sums of the result when the consumer folds them
                _, st3, f, opart = ops.ff_block_proj(p2, *ffargs, W[p + ".proj_out.bias"], x, out=out, want_stats=keep,
                                                     keep_from=M0 if keep else None, gn=gn)
            elif keep:
                p3, st3, f = ops.ff_block(p2, *ffargs, want_stats=True, keep_from=M0)
            else:
                p3 = ops.ff_block(p2, *ffargs)
        else:
            a3, st3 = ln(p2, "norm3")
            w1, b1 = W[t + ".ff.net.0.proj.weight"], W[t + ".ff.net.0.proj.bias"]
            if not keep and C % 64 == 0:        # no backward will follow: gate inside the GEMM epilogue (half the bytes)
                gg = ops.gemm(a3, w1, bias=b1, geglu=True)
            elif C % 64 == 0 and split:
                # guided step: only the cond half (second half of the rows) is differentiated, so only it needs the pre-activation
                # f: the uncond half takes the fused-GEGLU GEMM (a fifth of the bytes of GEMM + gate kernel), the cond half the
                # same fused epilogue that also stores the pre-activation the gate's backward needs (diff_from = 0: no first part)
                gg = torch.empty(M, 4 * C, device=self.dev, dtype=torch.float16)
                if M0:
                    ops.gemm(a3[:M0], w1, bias=b1, geglu=True, out=gg[:M0])
                _, f = ops.gemm_geglu_keep(a3[M0:], w1, b1, out=gg[M0:])
            else:
                f = ops.gemm(a3, w1, bias=b1)
                gg = ops.geglu(f, interleaved=True)
            p3, _ = _produce("gemm", gg, W[t + ".ff.net.2.weight"], out=_fresh(x, M, C), bias=W[t + ".ff.net.2.bias"], residual=p2)
        if not ffp:
            out, opart = _produce("gemm", *self._operand(p3, p + ".proj_out.weight", ":2"), out=out, bias=W[p + ".proj_out.bias"],
                                  residual=x, gn=gn)
        if keep:
            # the fp16 (hi) tensors the backward reads, each narrowed to the differentiated rows by what it actually holds - all rows,
            # the cond rows of a shared front (x / p1 / q2: what the text-independent part produced, after the injector for p1) or the
            # rows a stashing launch kept - whatever the injector did
            per_row = dict(x=_hi(x_c), pin=_hi(pin), st1=st1, qkv=qkv, o1=o1, p1=_hi(p1_c), st2=st2, q2=q2_c, o2=o2, p2=_hi(p2), st3=st3, f=f)
            per_image = dict(gst=gst, lse1=lse1, lse2=lse2)
            stash.tr[p] = dict({k: stash.suffix(f"{p}.{k}", v, HW) for k, v in per_row.items()},
                               **{k: stash.suffix(f"{p}.{k}", v, 1) for k, v in per_image.items()}, sz=sz, heads=heads)
        return out, opart

    @staticmethod
    def _dup_partial(part):
        """GroupNorm partial sums of the cond rows -> of [uncond rows ; cond rows] (the halves are identical)."""
        if part is None:
            return None
        both = ops.GNPartial.__new__(ops.GNPartial)
        both.rows, both.nch, both.groups = 2 * part.rows, part.nch, part.groups
        both.buf = torch.cat([part.buf, part.buf])
        return both

    def size_multiple(self) -> int:
        """What both latent sides of a non-square map must be multiples of: every stride-2 level halves them exactly and every
        nearest-2x upsample lands on its skip's size (odd sides need diffusers' upsample_size branch)."""
        return 2 ** (len(self.cfg.block_out_channels) - 1)

    def _check_rect(self, sz: Tuple[int, int]):
        f = self.size_multiple()
        if sz[0] % f or sz[1] % f:
            raise NotImplementedError(f"non-square latents {sz}: both sides must be multiples of {f}")

    # ------------------------------------------------------------------ forward
    def _conv_gn(self, x, w, bkey: str, rows: int, sz: Tuple[int, int], mode: int, out, residual=None):
        """A convolution (x, w: see _operand) whose output may leave GroupNorm partial sums behind: -> (out, the sums or None).  out: an
        fp16 view, a Pair (the pair epilogue), or None (a fresh fp16 tensor); the sums come with it where the level of the OUTPUT takes
        its statistics from the producers (_gn_from_producer).  residual: added in the epilogue (a ControlNet trunk's hint)."""
        osz = _half(sz) if mode == ops.CONV_S2 else sz
        gn = (osz[0] * osz[1], self.cfg.norm_groups) if self._gn_from_producer(rows, osz[0] * osz[1], w.shape[0]) else None
        return _produce("conv3x3", x, w, rows, *sz, mode, out=out, bias=self.W[bkey], gn=gn, residual=residual)

    def _add_control(self, dst, feat: torch.Tensor, zero_conv: Tuple[torch.Tensor, torch.Tensor], scale: float):
        """dst += scale * (feat . Wz^T + b): one zero convolution of a ControlNet, scaled by the conditioning scale and added to a skip
        (or to the mid block's output) IN PLACE - one GEMM launch whose residual is its own output, dst being a strided view inside a
        concat buffer or a Pair of them (the pair epilogue; feat stays a plain fp16 operand).  Safe: every epilogue of gemm.hip /
        gemm2.hip / gemm8.hip, the split-K reduce included, reads a residual element in the thread that then writes that element, and
        no thread reads an element another one writes (ControlNet)."""
        Wz, b = zero_conv
        if feat.shape[0] != _hi(dst).shape[0] or Wz.shape != (_hi(dst).shape[1], feat.shape[1]):
            raise ValueError(f"control residual {tuple(feat.shape)} / zero convolution {tuple(Wz.shape)} do not fit the skip "
                             f"{tuple(_hi(dst).shape)}: the ControlNet was built for another UNet config, batch or latent size")
        _produce("gemm", feat, Wz, out=dst, bias=b, residual=dst, alpha=float(scale))

    def _upsample(self, p: str, h, rows: int, sz: Tuple[int, int], out):
        """The nearest-2x upsampler convolution `p` of an up block: h (fp16: the block lies in the plain zone, or a Pair) -> out (the
        `h` columns of the next level's first concat buffer: fp16 inside the plain zone, else a Pair)."""
        W, wk, b = self.W, p + ".weight", self.W[p + ".bias"]
        if not isinstance(out, ops.Pair):
            # polyphase: 16 instead of 36 tap-products per low-res pixel (four launches; one grid on the small maps)
            if (wk + ":pp") in W and (UP2_SMALL_MAPS or (rows * sz[0] * sz[1] // 128) * (h.shape[1] // 160) >= 200):
                return ops.conv_up2(h, W[wk + ":pp"], rows, *sz, out=out, bias=b, W9=W[wk])
            return ops.conv3x3(h, W[wk], rows, *sz, ops.CONV_UP2, out=out, bias=b)
        pair_in = isinstance(h, ops.Pair)      # (leaving the plain zone: h is fp16 and the hi-only launch is the natural one)
        if (not pair_in or not HP_UP_TRIPLE) and (wk + ":pp") in W and (wk + ":pp3") not in W:
            try:
                ops.conv_up2_pairout(_hi(h), W[wk + ":pp"], rows, *sz, out, bias=b)
            except ops.SkgError as e:      # declined (an operand >= 2 GiB): the 9-tap gather form on the SAME hi-only operand
                if e.rc != -2:               # (both routes of the mode must see the same operand; pair output either way)
                    raise
                ops.conv3x3(_hi(h), W[wk], rows, *sz, ops.CONV_UP2, out=out.hi, out_lo=out.lo, bias=b)
        elif not pair_in:
            ops.conv3x3(h, W[wk], rows, *sz, ops.CONV_UP2, out=out.hi, out_lo=out.lo, bias=b)
        elif (wk + ":pp3") in W:      # polyphase, K axis [x_hi | x_lo | x_hi] . [W_hi | W_hi | W_lo]: 12 instead of 18 tap-products
            ops.conv_up2_hilo(self._full_of(h), W[wk + ":pp3"], rows, *sz, out, bias=b, W9x2=lambda: self._w9x2(wk))
        else:
            ops.conv3x3(self._full_of(h), W[wk + ":2"], rows, *sz, ops.CONV_UP2, out=out.hi, out_lo=out.lo, bias=b)
        return out

    def forward(self, x32: torch.Tensor, t, rows: int, H: int, stash: Optional[Stash] = None,
                want_taps: bool = True, want_eps: bool = True, down_only: bool = False, shared_input: bool = False,
                on_taps: Optional[Callable] = None, W: Optional[int] = None, diff_from: Optional[int] = None,
                through_mid: bool = False, hint: Optional[torch.Tensor] = None, control=None):
        """x32: fp16 [rows*H*W, 32] (latent channels zero-padded; W defaults to H).  Returns (eps [rows*H*W, 8] or None,
        taps: list of 9 (tensor [rows*s*s, C], s)) - on a non-square map (tensor [rows*sh*sw, C], (sh, sw)).

        t: one timestep for all rows (an int), or a sequence / 1-D integer tensor of `rows` timesteps, one per sample - the trainers'
        unet(noisy_latents, timesteps, ehs).  The time projection folded into conv1.bias of every ResnetBlock then is a [rows, Cout]
        stack, one gather per resnet, and conv1's epilogue reads a bias row per sample (ops.conv3x3 / conv3x3_wino with a 2-D bias);
        nothing else in the walk depends on t.  Equal entries take the int path.

        shared_input: the caller guarantees that the two halves of x32 are IDENTICAL - the CFG-doubled batch of
        modules/pipeline.py:85, `torch.cat([latents] * 2)`.  The two halves of the evaluation then only differ from the
        first text-dependent operation on (the first cross-attention), so everything in front of it - conv_in, the first
        ResnetBlock, and GroupNorm / proj_in / self-attention / LayerNorm 2 / to_q of the first transformer block, all at
        the full 64 x 64 resolution - is evaluated ONCE on the cond rows and copied to the uncond rows.  Exact in exact
        arithmetic (every kernel's result for a row depends on that row only); bit-identical to the doubled evaluation
        when the half-size launches run the same kernel instantiations, else equal to fp16 rounding noise - another
        summation order of GroupNorm partial sums / K slices (tests/test_gpu_pipeline.py::test_shared_cfg_prefix_is_bit_identical).

        on_taps(taps): called as soon as the ninth tap exists (after the third up block), before the last up block and
        conv_out are launched - the guidance branch (LGP + backward-to-input) depends on nothing later, so the sampler can put
        it on a second stream while this one finishes eps (sampler.HipSampler.fork_guidance).

        diff_from (with a stash): the first row the backward will differentiate - the stash keeps rows diff_from ... rows - 1 where
        it keeps a part only.  None: rows // 2, the cond half of a CFG-doubled batch (or the single row of rows = 1).  0: every row,
        the trainers' batch (backward_eps then differentiates all of them); odd row counts are fine.  An explicit value also selects
        the split / fused stashing launches whatever the parity of rows.  Not with shared_input (ValueError).

        through_mid (with down_only; the walk of a ControlNet trunk, controlnet.HipControlNet): the down path continued through
        mid_block -> (the list of all skips in production order, tensors [rows*sh*sw, C]; the mid block's output).  hint (down_only
        walks): fp16 [rows*H*W, C0], added to conv_in's output in its epilogue - diffusers' `sample = conv_in(sample) + cond`.

        control = (features, zero_convs, scale): the residuals of a ControlNet - features the n + 1 tensors a through_mid walk
        returns (skips, then mid), zero_convs n + 1 pairs (weight [C, C], bias [C]) fp16, the last for the mid block.  Behind
        mid_block every skip k becomes skip_k + scale (F_k Wz_k^T + b_k) and the mid block's output the same with the last pair
        (_add_control: one in-place GEMM each).  The adds wait for mid_block because the last skip is also mid_block's INPUT (one
        buffer; diffusers adds to copies), which the control must not reach.  The producers' GroupNorm partial sums of the skips
        describe them before the add and are dropped: the up path's norm1 takes its own statistics.  Not with a stash or taps (the
        backward would need the trunk's).

        One walk for both modes.  The blocks of the `pair_levels` outermost resolution levels (none in the default mode) carry the
        residual stream as (hi, lo) pairs: the same graph, the same kernels for every contraction, pair-aware epilogues / norms
        (skg_*_hilo), the same GroupNorm statistics from the producers' epilogues and the same shared CFG front; eps then is a pair
        too.  The deeper levels - the plain zone - run the default kernels on fp16 tensors (their pairs buy ~4 % of what the mode's
        pairs buy, tools/eps_decompose_stream.py): the stride-2 convolution that enters the zone reads the pair and writes fp16, the
        upsampler that leaves it reads fp16 and writes a pair; skips produced inside the zone are consumed inside it (the U-Net's
        skips connect equal resolutions).  Taps always carry the fp16 (hi) tensor."""
        if diff_from is not None:
            if shared_input:
                raise ValueError("diff_from: not with shared_input (the shared CFG front keeps the cond half only)")
            if not 0 <= int(diff_from) < rows:
                raise ValueError(f"diff_from = {diff_from}: a row index below rows = {rows} expected")
            diff_from = int(diff_from)
        if through_mid and not down_only:
            raise ValueError("through_mid continues the down_only walk: pass down_only=True with it")
        if hint is not None and not down_only:
            raise ValueError("hint: the input of a ControlNet trunk's walk (down_only=True, through_mid=True)")
        if control is not None and (down_only or stash is not None or want_taps):
            raise ValueError("control: a plain eps evaluation (no down_only, no stash, want_taps=False) - the guidance gradient and "
                             "the taps' consumers would need the ControlNet trunk's backward")
        sz = (H, H if W is None else W)
        cfg, W = self.cfg, self.W
        assert self.ctx is not None and self.ctx["rows"] == rows, "call prepare_context first"
        # every injector (inject.HipInjector, inject.HipClipInjectorTrain) has check_rows: a row count that differs from the batch
        # raises here.  It stays ahead of prepare_timesteps, the first call of this walk that launches kernels
        if self.inject is not None:
            self.inject.check_rows(rows)
        if sz[0] != sz[1]:
            self._check_rect(sz)
        t = per_sample_timesteps(t, rows, shared_input)
        self.prepare_timesteps(sorted(set(t)) if isinstance(t, list) else [t])
        assert not (down_only and self.residual_fp32), "accuracy mode: the whole UNet (with or without a stash, with or without an injector)"
        if stash is not None:
            stash.rows, stash.first = rows, rows // 2 if diff_from is None else diff_from
            stash.misc.update(H=H, W=sz[1])
        if isinstance(t, list):      # a timestep per sample: every resnet's bias rows in row order, one gather per resnet
            idx = torch.tensor([self.tbias_row[v] for v in t], device=self.dev)
            tb = {p: tab.index_select(0, idx) for p, tab in self.tbias_tab.items()}
        else:
            tb = self.tbias[t]
        boc = cfg.block_out_channels
        nb, lpb, lpb1 = len(boc), cfg.layers_per_block, cfg.layers_per_block + 1
        cats = _ConcatBuffers(self, rows, down_only)
        res = self._res_fwd                        # (one body each: the representation of their input - fp16 or Pair - decides)
        tr = self._tr_fwd if diff_from is None else functools.partial(self._tr_fwd, diff_from=diff_from)
        # hp: GroupNorm partial sums of h left behind by the kernel that produced it, whenever the next consumer of h is a
        # GroupNorm of the 64 x 64 / 32 x 32 levels (None otherwise: concatenated inputs, small maps)
        shared = shared_input and rows % 2 == 0 and rows >= 2 and not down_only and nb > 1 and lpb >= 1
        cur = sz
        if shared:
            S1, M1 = rows // 2, (rows // 2) * sz[0] * sz[1]
            slot = cats.skip_slot(boc[0], sz)                      # the skip of conv_in, all rows
            hc = _rows_of(slot, M1, 2 * M1)
            _, hp1 = self._conv_gn(x32[M1:], W["conv_in.weight"], "conv_in.bias", S1, sz, ops.CONV_S1, hc)
            _copy_up(hc, slot, M1)
            cats.push(slot, self._dup_partial(hp1))
            x_full = _fresh(slot, 2 * M1, boc[0])
            p0 = "down_blocks.0.resnets.0"      # (a timestep per sample: the halves' timesteps are equal row for row - the cond rows' stack)
            h1, hp1 = res(p0, hc, S1, cur, {p0: tb[p0][S1:]} if isinstance(t, list) else tb, stash, out=_rows_of(x_full, M1, 2 * M1), xpart=hp1,
                          want_part=True)
            _copy_up(h1, x_full, M1)
            h, hp = tr("down_blocks.0.attentions.0", h1, rows, cur, cfg.num_heads[0], stash, out=cats.skip_slot(boc[0], cur),
                       xpart=hp1, want_part=0 < lpb - 1, shared=True, x_full=x_full)
        else:
            h, hp = self._conv_gn(x32, W["conv_in.weight"], "conv_in.bias", rows, sz, ops.CONV_S1, cats.skip_slot(boc[0], sz),
                                  residual=hint)
        cats.push(h, hp)
        taps_down = []
        for i in range(nb):
            for j in range(lpb):
                if shared and i == 0 and j == 0:
                    continue                                      # done above, once for both halves
                rp, ap = f"down_blocks.{i}.resnets.{j}", f"down_blocks.{i}.attentions.{j}"
                if i < nb - 1:
                    h, hp = res(rp, h, rows, cur, tb, stash, xpart=hp, want_part=True)
                    # the block's last transformer feeds the downsampling conv, the others the next resnet's norm1
                    h, hp = tr(ap, h, rows, cur, cfg.num_heads[i], stash, out=cats.skip_slot(boc[i], cur), xpart=hp,
                               want_part=j < lpb - 1)
                else:
                    h, hp = res(rp, h, rows, cur, tb, stash, out=cats.skip_slot(boc[i], cur), xpart=hp, want_part=True)
                cats.push(h, hp)
            if i < nb - 1:
                # (its output - a skip - has the representation of the next level: entering the plain zone, the pair is the
                # K-doubled operand and the output fp16)
                p = f"down_blocks.{i}.downsamplers.0.conv"
                o = cats.skip_slot(boc[i], _half(cur))
                h, hp = self._conv_gn(*self._operand(h, p + ".weight", ":2"), p + ".bias", rows, cur, ops.CONV_S2, o)
                cur = _half(cur)
                cats.push(h, hp)
            if i < 3:
                taps_down.append((_hi(h), _side(cur)))
        if down_only and not through_mid:
            # modules/sketch_encoder.py:39-98: the forward stops after the down path and returns the per-block
            # tuples of residual samples ((tensor [rows*s*s, C], s), ...) - what SatMixin.set_res_samples consumes
            # (on a non-square map: (tensor [rows*sh*sw, C], (sh, sw)))
            out, k = [], 1
            for i in range(nb):
                n = lpb + (1 if i < nb - 1 else 0)
                lv = lambda i: _side((sz[0] >> i, sz[1] >> i))
                sizes = [lv(i)] * lpb + ([lv(i + 1)] if i < nb - 1 else [])
                out.append(tuple((cats.skips[k + j], sizes[j]) for j in range(n)))
                k += n
            return out
        h, hp = res("mid_block.resnets.0", h, rows, cur, tb, stash, xpart=hp, want_part=True)
        tap_r0 = (_hi(h), _side(cur))
        h, hp = tr("mid_block.attentions.0", h, rows, cur, cfg.num_heads[-1], stash, xpart=hp, want_part=True)
        tap_at = (_hi(h), _side(cur))
        h, _ = res("mid_block.resnets.1", h, rows, cur, tb, stash, out=None if down_only else cats.h_slot(0), xpart=hp)
        if down_only:
            return list(cats.skips), h
        tap_r1 = (_hi(h), _side(cur))
        if control is not None:
            feats, zero_convs, cscale = control
            if len(feats) != len(cats.skips) + 1 or len(zero_convs) != len(feats):
                raise ValueError(f"control: {len(cats.skips) + 1} residuals and zero convolutions expected, got {len(feats)} / {len(zero_convs)}")
            for k, skip in enumerate(cats.skips):
                self._add_control(skip, feats[k], zero_convs[k], cscale)
                cats.parts[k] = None
            self._add_control(h, feats[-1], zero_convs[-1], cscale)
        hp = None
        taps_up = []
        rev_heads = tuple(reversed(cfg.num_heads))
        last_needed = 2 if not want_eps else nb - 1
        for i in range(nb):
            if i > last_needed:
                break
            for j in range(lpb1):
                u = i * lpb1 + j
                rp, ap = f"up_blocks.{i}.resnets.{j}", f"up_blocks.{i}.attentions.{j}"
                # norm1 of a resnet that reads [h | skip]: both halves' producers may have left their sums behind
                # (regrouped where the widths allow, else the norm makes its own pass)
                cpart = cats.concat_part(u, hp)
                # where this layer's output goes: the next concat buffer of the same block, else a fresh tensor
                nxt = cats.h_slot(u + 1) if j < lpb1 - 1 else None
                if i > 0:
                    h, hp = res(rp, cats.whole(u), rows, cur, tb, stash, xpart=cpart, want_part=True)
                    # the transformer's output goes to conv_norm_out (the very last one) or into the next concatenation,
                    # whose GroupNorm regroups its sums with the skip's; the block's last output feeds the upsampling conv
                    keep = (want_eps and i == nb - 1 and j == lpb1 - 1) or j < lpb1 - 1
                    h, hp = tr(ap, h, rows, cur, rev_heads[i], stash, out=nxt, xpart=hp, want_part=keep)
                else:
                    h, hp = res(rp, cats.whole(u), rows, cur, tb, stash, out=nxt, xpart=cpart, want_part=j < lpb1 - 1)
            if i < nb - 1:
                h = self._upsample(f"up_blocks.{i}.upsamplers.0.conv", h, rows, cur, cats.h_slot((i + 1) * lpb1))
                hp = None              # (the next concatenation's widths do not line up with 32 groups per half)
                cur = _dbl(cur)
            if i < 3:
                taps_up.append((_hi(h), _side(cur)))
                if i == 2 and on_taps is not None:
                    on_taps(taps_down + [tap_at, tap_r0, tap_r1] + taps_up)
        eps = None
        HW = cur[0] * cur[1]
        if want_eps:
            # conv_norm_out -> SiLU -> conv_out.  Accuracy mode: both the normalised activation (the K-doubled operand [hi | lo] . [W | W])
            # and eps itself (a (hi, lo) pair in one [M, 2 * 8] buffer, combined in fp32 by the CFG / scheduler kernel) keep fp32
            # accuracy - their fp16 roundings would reach eps one to one (2.8e-4 relative each)
            n, nst = self._norm(h, rows, HW, 1e-5, "conv_norm_out", True, partial=hp, pair_out=True)
            eps, _ = _produce("conv3x3", *self._operand(n, "conv_out.weight", ":2"), rows, *cur, out=_fresh(h, rows * HW, COUT_PAD),
                              bias=W["conv_out.bias"])
            if stash is not None and not isinstance(h, ops.Pair):      # what backward_eps reads (references only: no extra launch)
                stash.misc.update(out_h=stash.suffix("conv_norm_out.h", h, HW), out_st=stash.suffix("conv_norm_out.st", nst, 1))
        taps = taps_down + [tap_at, tap_r0, tap_r1] + taps_up
        return eps, (taps if want_taps else None)

    # ------------------------------------------------------------------ pairs (accuracy mode, residual_fp32)
    @staticmethod
    def _full_of(pv: ops.Pair) -> torch.Tensor:
        """[hi | lo] as ONE operand: the pair's own buffer, or a packed copy when it lives inside a concat buffer."""
        if pv.full is not None:
            return pv.full
        C = pv.hi.shape[1]
        buf = torch.empty(pv.hi.shape[0], 2 * C, device=pv.hi.device, dtype=torch.float16)
        ops.axpby(pv.hi, None, out=buf[:, :C])
        ops.axpby(pv.lo, None, out=buf[:, C:])
        return buf

    # ------------------------------------------------------------------ modules, backward (cond rows)
    def _res_bwd(self, p, dout, S, st: dict):
        """S: number of differentiated rows - the rows every tensor of the stash entry st holds (Stash.suffix)."""
        cfg, W = self.cfg, self.W
        sz = st["sz"]
        HW, G = sz[0] * sz[1], cfg.norm_groups
        x, h1, st1, st2 = st["x"], st["h1"], st["st1"], st["st2"]
        dn2 = self._conv_wino(p + ".conv2.weight:winoT", dout, S, sz)
        if dn2 is None:
            dn2 = ops.conv3x3(dout, W[p + ".conv2.weight:T"], S, *sz)
        dh1 = ops.groupnorm_bwd(h1, dn2, S, HW, G, st2, W[p + ".norm2.weight"], W[p + ".norm2.bias"], True)
        dn1 = self._conv_wino(p + ".conv1.weight:winoT", dh1, S, sz)
        if dn1 is None:
            dn1 = ops.conv3x3(dh1, W[p + ".conv1.weight:T"], S, *sz)
        if (p + ".conv_shortcut.weight") in W:
            sc = ops.gemm(dout, W[p + ".conv_shortcut.weight:T"])
        else:
            sc = dout
        return ops.groupnorm_bwd(x, dn1, S, HW, G, st1, W[p + ".norm1.weight"], W[p + ".norm1.bias"], True,
                                 residual=sc)

    def _tr_bwd(self, p, dout, S, st: dict, inject_bwd: Optional[Callable] = None):
        """S: see _res_bwd.  inject_bwd(block path, d p1) -> d (p1 in front of the injected attention): the backward of the
        injector the stashed forward ran between the self-attention and norm2 (backward_eps)."""
        cfg, W = self.cfg, self.W
        sz, heads = st["sz"], st["heads"]
        HW = sz[0] * sz[1]
        C = dout.shape[1]
        dh = C // heads
        scale = dh ** -0.5
        t = p + ".transformer_blocks.0"
        dp3 = ops.gemm(dout, W[p + ".proj_out.weight:T"])
        dgg = ops.gemm(dp3, W[t + ".ff.net.2.weight:T"])
        df = ops.geglu_bwd(st["f"], dgg, interleaved=True)
        da3 = ops.gemm(df, W[t + ".ff.net.0.proj.weight:T"])
        dp2 = ops.layernorm_bwd(st["p2"], da3, W[t + ".norm3.weight"], st["st3"], residual=dp3)
        # cross-attention: only dQ (K/V come from the constant text embeddings - of every row of the evaluation: the differentiated
        # rows' keys start at row `first`, the one thing the stash did not narrow)
        do2 = ops.gemm(dp2, W[t + ".attn2.to_out.0.weight:T"])
        cb = self.ctx["blocks"][t + ".attn2"]
        L, Lp = self.ctx["L"], self.ctx["Lp"]
        first = self.ctx["rows"] - S
        K2, V2 = cb["K"][first * Lp:], cb["V"][first * Lp:]
        if _ATTN_DQ_DELTA:      # delta = sum_d dO O in the prologue of the dQ launch (one launch and one read of dO fewer)
            dq2, _ = ops.attn_bwd_dq_delta(st["q2"], K2, V2, do2, st["o2"], st["lse2"], S, heads, HW, L, Lp, dh, scale)
        else:
            delta2 = ops.attn_bwd_delta(st["o2"], do2, S, heads, HW, dh)
            dq2 = ops.attn_bwd_dq(st["q2"], K2, V2, do2, st["lse2"], delta2, S, heads, HW, L, Lp, dh, scale)
        da2 = ops.gemm(dq2, W[t + ".attn2.to_q.weight:T"])
        dp1 = ops.layernorm_bwd(st["p1"], da2, W[t + ".norm2.weight"], st["st2"], residual=dp2)
        if inject_bwd is not None:      # the stashed p1 is the injector's output: through it to the self-attention's output
            dp1 = inject_bwd(t, dp1)
        # self-attention
        do1 = ops.gemm(dp1, W[t + ".attn1.to_out.0.weight:T"])
        qkv, o1, lse1 = st["qkv"], st["o1"], st["lse1"]
        Q, K, V = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
        dqkv = torch.empty(S * HW, 3 * C, device=self.dev, dtype=torch.float16)
        if _ATTN_DQ_DELTA:
            _, delta1 = ops.attn_bwd_dq_delta(Q, K, V, do1, o1, lse1, S, heads, HW, HW, HW, dh, scale, out=dqkv[:, :C])
        else:
            delta1 = ops.attn_bwd_delta(o1, do1, S, heads, HW, dh)
            ops.attn_bwd_dq(Q, K, V, do1, lse1, delta1, S, heads, HW, HW, HW, dh, scale, out=dqkv[:, :C])
        ops.attn_bwd_dkv(Q, K, V, do1, lse1, delta1, S, heads, HW, HW, dh, scale, dK=dqkv[:, C:2 * C], dV=dqkv[:, 2 * C:])
        da1 = ops.gemm(dqkv, W[t + ".attn1.qkv:T"])
        dpin = ops.layernorm_bwd(st["pin"], da1, W[t + ".norm1.weight"], st["st1"], residual=dp1)
        dg = ops.gemm(dpin, W[p + ".proj_in.weight:T"])
        return ops.groupnorm_bwd(st["x"], dg, S, HW, cfg.norm_groups, st["gst"], W[p + ".norm.weight"],
                                 W[p + ".norm.bias"], False, residual=dout)

    # ------------------------------------------------------------------ backward
    def backward(self, stash: Stash, tap_grads: Sequence[Optional[torch.Tensor]]) -> torch.Tensor:
        """tap_grads: 9 fp16 tensors [S*s*s, C] (cond rows) in tap order.  Returns d loss / d x for the
        cond rows, fp16 [S*H*W, 8] (first 4 channels valid; H x W: the stashed forward's size)."""
        assert self.need_backward and self.inject is None, "backward with injected attention is not supported"
        return self._backward_chain(stash, tap_grads[8], tap_grads, 2, None, False)

    def backward_eps(self, stash: Stash, d_eps: torch.Tensor, inject_bwd: Optional[Callable] = None) -> Optional[torch.Tensor]:
        """Backward from the UNet's output.  d_eps: fp16 [S*H*W, EPS_SEED_LD] (first 4 channels valid, the rest zero) for the rows
        the stash holds - from stash.first, the stashed forward's diff_from, on (S = rows - first; by default rows // 2: the cond half of a
        CFG-doubled batch, or the single row of a rows = 1 evaluation; 0: every row of a trainer's batch) - of a
        forward(..., stash, want_eps=True).
        conv_out's data gradient, conv_norm_out's GroupNorm + SiLU backward, then every up block, the mid block and the down path.  inject_bwd: see _tr_bwd - the forward ran with an injector, whose parameter
        gradients are the point; the chain then stops in front of down_blocks.0.attentions.0 (nothing trainable lies further
        up) and returns None.  Without an injector: d loss / d x like backward().  All-fp16 mode, square maps, eager."""
        assert self.need_backward, "built with need_backward=False: no :T packs"
        if self.residual_fp32:
            raise NotImplementedError("backward_eps: the accuracy mode (residual_fp32) is not supported")
        assert (self.inject is None) == (inject_bwd is None), "an injected forward needs the injector's backward (and only it)"
        cfg, W = self.cfg, self.W
        sz = (stash.misc["H"], stash.misc.get("W", stash.misc["H"]))
        if sz[0] != sz[1]:
            raise NotImplementedError("backward_eps: square maps only")
        assert "out_h" in stash.misc, "the stashed forward ran without want_eps"
        S = stash.rows - stash.first
        HW = sz[0] * sz[1]
        assert d_eps.shape == (S * HW, EPS_SEED_LD)
        dn = ops.conv3x3(d_eps, W["conv_out.weight:T"], S, *sz)
        dh = ops.groupnorm_bwd(stash.misc["out_h"], dn, S, HW, cfg.norm_groups, stash.misc["out_st"],
                               W["conv_norm_out.weight"], W["conv_norm_out.bias"], True)
        nb = len(cfg.block_out_channels)
        return self._backward_chain(stash, dh, [None] * 9, nb - 1, inject_bwd, inject_bwd is not None)

    def _backward_chain(self, stash: Stash, dh, tap_grads, first_up: int, inject_bwd, stop_early: bool):
        """The reversed graph from the output of up block `first_up` (after its upsampler, if it has one) to the input, on the
        stash's rows - first differentiated rows.  stop_early: return None after down_blocks.0.attentions.0 instead of finishing
        the first ResnetBlock and conv_in."""
        cfg, W = self.cfg, self.W
        S = stash.rows - stash.first
        sz = (stash.misc["H"], stash.misc.get("W", stash.misc["H"]))
        nb = len(cfg.block_out_channels)
        lpb = cfg.layers_per_block

        def add(a, b):
            if a is None:
                return b
            if b is None:
                return a
            return ops.axpby(a, b)

        # skip index bookkeeping: skips = [conv_in] + per down block (lpb resnet outs [+ downsample out])
        n_skips = 1 + sum(lpb + (1 if i < nb - 1 else 0) for i in range(nb))
        gskip: List[Optional[torch.Tensor]] = [None] * n_skips
        # ---- up path, reversed (backward: blocks 2, 1, 0 - block 3 does not feed any tap; backward_eps: from block nb - 1)
        # index of the skip consumed first by up block i: pops from the end
        pop_idx = n_skips
        consumed = {}
        for i in range(nb):
            for j in range(lpb + 1):
                pop_idx -= 1
                consumed[(i, j)] = pop_idx
        cur = sz                                 # spatial size of up block first_up's output (after its upsampler; nb = 4)
        plan = up_block_plan(cfg)
        for i in range(first_up, -1, -1):
            if i < nb - 1:
                # upsampler backward: dgrad at the upsampled size, then 2x2 sum-pool
                p = f"up_blocks.{i}.upsamplers.0.conv"
                if UP2_DGRAD and (p + ".weight:ppT") in W:      # polyphase: one 4 x 4 stride-2 convolution, 16 instead of 36 tap-products
                    dh = ops.conv4x4s2(dh, W[p + ".weight:ppT"], S, *cur, W9T=W[p + ".weight:T"])
                    cur = _half(cur)
                else:
                    du = ops.conv3x3(dh, W[p + ".weight:T"], S, *cur)
                    cur = _half(cur)
                    dh = ops.sumpool2x2(du, S, *cur)
            for j in range(lpb, -1, -1):
                if i > 0:
                    dh = self._tr_bwd(f"up_blocks.{i}.attentions.{j}", dh, S, stash.tr[f"up_blocks.{i}.attentions.{j}"], inject_bwd)
                dcat = self._res_bwd(f"up_blocks.{i}.resnets.{j}", dh, S, stash.res[f"up_blocks.{i}.resnets.{j}"])
                ch = plan[i][j][0]
                k = consumed[(i, j)]
                gskip[k] = add(gskip[k], dcat[:, ch:])
                dh = dcat[:, :ch]
            if 0 < i <= 3:
                dh = add(dh, tap_grads[6 + i - 1])      # output of up block i-1 (after its upsampler)
        # ---- mid
        dh = add(dh, tap_grads[5])
        dh = self._res_bwd("mid_block.resnets.1", dh, S, stash.res["mid_block.resnets.1"])
        dh = add(dh, tap_grads[3])
        dh = self._tr_bwd("mid_block.attentions.0", dh, S, stash.tr["mid_block.attentions.0"], inject_bwd)
        dh = add(dh, tap_grads[4])
        dh = self._res_bwd("mid_block.resnets.0", dh, S, stash.res["mid_block.resnets.0"])
        # ---- down path, reversed
        k = n_skips - 1
        for i in range(nb - 1, -1, -1):
            if i < nb - 1:
                dh = add(dh, gskip[k]); k -= 1
                if i < 3:
                    dh = add(dh, tap_grads[i])
                p = f"down_blocks.{i}.downsamplers.0.conv"
                dh = ops.conv3x3(dh, W[p + ".weight:T"], S, *cur, ops.CONV_S2T)
                cur = _dbl(cur)
            for j in range(lpb - 1, -1, -1):
                dh = add(dh, gskip[k]); k -= 1
                if i < nb - 1:
                    dh = self._tr_bwd(f"down_blocks.{i}.attentions.{j}", dh, S,
                                      stash.tr[f"down_blocks.{i}.attentions.{j}"], inject_bwd)
                    if stop_early and i == 0 and j == 0:
                        return None
                dh = self._res_bwd(f"down_blocks.{i}.resnets.{j}", dh, S, stash.res[f"down_blocks.{i}.resnets.{j}"])
        dh = add(dh, gskip[0])
        return ops.conv3x3(dh, W["conv_in.weight:T"], S, *sz)
