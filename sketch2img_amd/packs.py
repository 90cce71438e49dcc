"""Weight-pack layouts of the libskg.so kernels: how one weight tensor (diffusers state_dict layout) is laid out for the kernel
that reads it.  Which packs a net has is decided in unet.py (HipUNet._pack / _pack_hp); the kernels' side of each layout is
documented in ops.py and csrc/.

Linear / 1x1 conv [N][K]; conv3x3 [Cout][ky][kx][Cin]; each has a second "dgrad" pack (transposed / tap-flipped) for backward."""
from __future__ import annotations

from typing import Iterator, Optional

import torch

CIN_PAD = 64      # latent channels padded to one 64-deep K tile of the LDS-DMA implicit-GEMM conv
COUT_PAD = 8      # conv_out / conv_in-dgrad output channels padded to the 8-channel store granule
CTX_PAD = 8       # text tokens padded to a multiple of 8 (77 -> 80)
EPS_SEED_LD = 32  # columns of the d eps seed of backward_eps: one 32-deep K step of conv_out's data gradient (4 valid channels)


def _h(t: torch.Tensor, dev) -> torch.Tensor:
    return t.detach().to(device=dev, dtype=torch.float16).contiguous()


def _pad_vec(v: torch.Tensor, n: int) -> torch.Tensor:
    return torch.nn.functional.pad(v, (0, n - v.shape[0])) if n > v.shape[0] else v


def pack_conv(w: torch.Tensor, dev, cin_pad: int = 0, cout_pad: int = 0) -> torch.Tensor:
    """[Cout,Cin,3,3] -> [Cout(+pad)][ky][kx][Cin(+pad)] flattened to [Cout, 9*Cin]."""
    co, ci = w.shape[:2]
    p = w.permute(0, 2, 3, 1)
    if cin_pad > ci:
        p = torch.nn.functional.pad(p, (0, cin_pad - ci))
    if cout_pad > co:
        p = torch.nn.functional.pad(p, (0, 0, 0, 0, 0, 0, 0, cout_pad - co))
    return _h(p.reshape(p.shape[0], -1), dev)


def pack_conv_small(w: torch.Tensor, dev) -> torch.Tensor:
    """Pack of a 3x3 convolution with 3 or 16 input channels for ops.conv3x3_small (csrc/condembed.hip): [Cout, 3, 3, 3] ->
    [Cout][16 tap slots][4] (channel 3 and the slots 9 .. 15 zero), [Cout, 16, 3, 3] -> [Cout][10 tap slots][16] (slot 9 zero)."""
    co, ci = w.shape[:2]
    if ci not in (3, 16) or tuple(w.shape[2:]) != (3, 3):
        raise ValueError(f"pack_conv_small: a [Cout, 3 or 16, 3, 3] weight expected, got {tuple(w.shape)}")
    slots, cp = (16, 4) if ci == 3 else (10, 16)
    p = torch.zeros(co, slots, cp, dtype=torch.float32)
    p[:, :9, :ci] = w.detach().float().cpu().permute(0, 2, 3, 1).reshape(co, 9, ci)
    return _h(p.reshape(co, -1), dev)


def pack_conv_wino(w: torch.Tensor, dev, dgrad: bool = False) -> torch.Tensor:
    """Winograd F(2x2, 3x3) weight pack of a 3x3 convolution [Cout, Cin, 3, 3] -> U [Cout, 16 * Cin] fp16: U = G g G^T per (cout, cin),
    formed in fp32 and rounded once; component c = 4 i + j at columns [c Cin, (c + 1) Cin) (ops.conv3x3_wino, csrc/wino.hip).
    dgrad: the pack of the convolution's DATA GRADIENT - itself a 3x3 convolution with the taps flipped and in / out swapped."""
    g = w.detach().to(device=dev, dtype=torch.float32)                   # (formed on the target device, elementwise: no BLAS call at pack time)
    if dgrad:
        g = g.flip(2, 3).transpose(0, 1)

    def G3(a, b, c):                                                     # G = [[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]] applied along one axis
        return a, 0.5 * (a + b + c), 0.5 * (a - b + c), c

    rows = G3(g[:, :, 0, :], g[:, :, 1, :], g[:, :, 2, :])               # G g: 4 x [Cout, Cin, 3]
    U = torch.stack([torch.stack(G3(r[:, :, 0], r[:, :, 1], r[:, :, 2]), 1) for r in rows], 1)      # (G g) G^T: [Cout, 4 (i), 4 (j), Cin]
    return _h(U.reshape(U.shape[0], -1), dev)


def pack_conv_dgrad(w: torch.Tensor, dev, cin_pad: int = 0, cout_pad: int = 0) -> torch.Tensor:
    """dgrad pack: Wd[ci][ky'][kx'][co] = W[co][ci][2-ky'][2-kx'] -> [Cin, 9*Cout].
    ``cin_pad`` pads the OUTPUT rows (the conv's input channels), ``cout_pad`` the contraction."""
    co, ci = w.shape[:2]
    p = w.flip(2, 3).permute(1, 2, 3, 0)
    if cout_pad > co:
        p = torch.nn.functional.pad(p, (0, cout_pad - co))
    if cin_pad > ci:
        p = torch.nn.functional.pad(p, (0, 0, 0, 0, 0, 0, 0, cin_pad - ci))
    return _h(p.reshape(p.shape[0], -1), dev)


def _up2_phase_taps(w: torch.Tensor) -> Iterator[torch.Tensor]:
    """The pre-summed weights of a 3x3 filter [Cout, Cin, 3, 3] (fp32) applied after a nearest 2x upsample, per phase 2a+b a tensor
    [Cout][4 taps][Cin]: output pixel (2i+a, 2j+b) reads low-res rows {i-1, i} (a = 0) or {i, i+1} (a = 1); the filter rows that
    land on one low-res row are summed, the same for columns."""
    for a in (0, 1):
        rws = (w[:, :, 0], w[:, :, 1] + w[:, :, 2]) if a == 0 else (w[:, :, 0] + w[:, :, 1], w[:, :, 2])      # [co, ci, kx]
        for b in (0, 1):
            taps = []
            for r in rws:
                taps += [r[:, :, 0], r[:, :, 1] + r[:, :, 2]] if b == 0 else [r[:, :, 0] + r[:, :, 1], r[:, :, 2]]
            yield torch.stack(taps, 1)                                                                         # [co][tap][ci]


def pack_conv_up2(w: torch.Tensor, dev) -> torch.Tensor:
    """Polyphase pack of a 3x3 filter applied after a nearest 2x upsample (ops.conv_up2): [4 phases 2a+b][Cout][4 taps][Cin],
    the pre-summed weights of _up2_phase_taps (fp32 sums, one fp16 rounding)."""
    co, ci = w.shape[:2]
    return _h(torch.stack([t.reshape(co, 4 * ci) for t in _up2_phase_taps(w.detach().float())], 0), dev)


def pack_conv_up2_hilo(w: torch.Tensor, dev) -> torch.Tensor:
    """Accuracy-mode polyphase pack (ops.conv_up2_hilo): the pre-summed weights of pack_conv_up2 kept as (hi, lo) fp16 pairs,
    per phase and tap [W_hi | W_hi | W_lo] against the operand blocks [x_hi | x_lo | x_hi]: [4][Cout][4 taps][3 Cin]."""
    co, ci = w.shape[:2]
    phases = []
    for t in _up2_phase_taps(w.detach().float()):
        hi = t.half()
        lo = (t - hi.float()).half()
        phases.append(torch.cat([hi, hi, lo], 2).reshape(co, 12 * ci))
    return torch.stack(phases, 0).contiguous().to(dev)


def pack_conv_up2_dgrad(w: torch.Tensor, dev) -> torch.Tensor:
    """Data gradient of the polyphase upsample + conv (ops.conv4x4s2): [Cin][16 taps ky*4+kx][Cout], the transposed pre-summed
    weights of pack_conv_up2.  dX[p] = sum over phases a and taps ty of Wpp[a][ty]^T dY[2 (p - oy(a, ty)) + a] with
    oy(0, .) = (-1, 0), oy(1, .) = (0, +1): rows 2p - 1 .. 2p + 2 of dY, window row ky = 0..3 <-> (a, ty) = (1,1), (0,1), (1,0), (0,0)."""
    w = w.detach().float()
    co, ci = w.shape[:2]

    def split(t, axis):          # 3 filter taps along `axis` -> the four window positions along that axis
        t0, t1, t2 = t.unbind(axis)
        return [t2, t1 + t2, t0 + t1, t0]      # ky = 0: (a=1, ty=1) = w2;  1: (0,1) = w1 + w2;  2: (1,0) = w0 + w1;  3: (0,0) = w0
    taps = []
    for r in split(w, 2):                                        # 4 x [co, ci, kx]
        taps += split(r, 2)                                      # 16 x [co, ci], order ky * 4 + kx
    p = torch.stack(taps, 0)                                     # [16, co, ci]
    return _h(p.permute(2, 0, 1).reshape(ci, 16 * co), dev)


def pack_ff_block(w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, dev, w_proj: Optional[torch.Tensor] = None):
    """Fragment-major pack of a GEGLU feed-forward (diffusers FeedForward: net.0.proj [2F, C] = value rows then gate rows,
    net.2 [C, F]) for skg_ff_block_f16 (csrc/ffblock.hip): every 512-half piece is one MFMA A operand in lane order, so
    the kernel fetches it with one LDS-DMA instruction and reads it with one conflict-free ds_read_b128.
    Chunk c = hidden units 32c .. 32c+31:
      40 W1 pieces (t, ks): t = value 0-15, value 16-31, gate 0-15, gate 16-31; [lane = 16 g + l][i] = W1[row(t, l)][32 ks + 8 g + i]
      20 W2 pieces u:       [lane = 16 g + l][i] = W2[16 u + l][32 c + 16 (i >> 2) + 4 g + (i & 3)]
    (the hidden-unit order of the second product is the accumulator layout of the first).
    w_proj [C, C] (Transformer2DModel.proj_out, skg_ff_block_f16 with bias_proj): five more chunks j behind them whose first 40 pieces are
      (t, ks): [lane = 16 g + l][i] = Wp[16 (4 j + t) + l][32 ks + 16 (i >> 2) + 4 g + (i & 3)]   (the block output's accumulator order)
    and whose last 20 pieces are zeros.
    Returns (pack fp16 [F/32 (+ 5), 60, 512], bias1 fp32 [F/32, 4, 16])."""
    F2, C = w1.shape
    F = F2 // 2
    assert w2.shape == (C, F) and C % 32 == 0 and F % 32 == 0
    nch, KS, NU = F // 32, C // 32, C // 16
    # (host-side packing: the state dict may live on the device after a broadcast)
    w1h, w2h, b1 = w1.detach().to("cpu", torch.float16), w2.detach().to("cpu", torch.float16), b1.detach().cpu()
    rows = torch.stack([w1h[:F].reshape(nch, 2, 16, C), w1h[F:].reshape(nch, 2, 16, C)], 1)     # [c, val|gate, half, l, C]
    rows = rows.reshape(nch, 4, 16, KS, 4, 8)                                                     # [c, t, l, ks, g, i]
    p1 = rows.permute(0, 1, 3, 4, 2, 5).reshape(nch, 4 * KS, 512)                                 # [c, (t, ks), (g, l, i)]
    w2r = w2h.reshape(NU, 16, nch, 2, 4, 4)                                                       # [u, l, c, i_hi, g, i_lo]
    p2 = w2r.permute(2, 0, 4, 1, 3, 5).reshape(nch, NU, 512)                                      # [c, u, (g, l, i_hi, i_lo)]
    pack = torch.cat([p1, p2], 1)
    if w_proj is not None:
        assert w_proj.shape == (C, C) and NU % 4 == 0
        wp = w_proj.detach().to("cpu", torch.float16).reshape(NU, 16, KS, 2, 4, 4)             # [u, l, ks, i_hi, g, i_lo]
        pp = wp.permute(0, 2, 4, 1, 3, 5).reshape(NU // 4, 4 * KS, 512)                        # [j, (t, ks), (g, l, i_hi, i_lo)]
        pack = torch.cat([pack, torch.cat([pp, torch.zeros(NU // 4, NU, 512, dtype=torch.float16)], 1)], 0)
    pack = pack.contiguous().to(dev)
    b1h = b1.to(torch.float16).float()
    bias1 = torch.stack([b1h[:F].reshape(nch, 2, 16), b1h[F:].reshape(nch, 2, 16)], 1).reshape(nch, 4, 16).contiguous().to(dev)
    return pack, bias1


def pack_xattn_weights(wq: torch.Tensor, wo: torch.Tensor, heads: int, dev):
    """Fragment-major pack of attn2.to_q [C, C] and attn2.to_out.0 [C, C] for skg_xattn_block_f16 (csrc/xattn.hip), C = 320; per head h
    the kernel's LDS image in pieces of 512 halves.
    8 heads of 40 (SD1.5; head width padded to 48), 60 pieces:
      30 Wq pieces (t, ks):  [lane = 16 g + l][i] = Wq[40 h + 16 t + l][32 ks + 8 g + i]         (rows 40..47 of the head: zeros)
      Wo image (30 pieces):  20 K = 32 fragments  [lane][i] = Wo[16 u + l][40 h + 16 (i >> 2) + 4 g + (i & 3)]
                             20 K = 16 fragments  [lane][i < 4] = Wo[16 u + l][40 h + 32 + 4 g + i]   (d >= 40: zeros)
    5 heads of 64 (SD2.1), 80 pieces: 40 Wq pieces (t < 4, ks) as above, then 2 x 20 K = 32 fragments
      [s][u]: [lane][i] = Wo[16 u + l][64 h + 32 s + 16 (i >> 2) + 4 g + (i & 3)].
    Returns fp16 [heads, 60 | 80, 512]."""
    C = wq.shape[0]
    dh = C // heads
    assert wq.shape == (C, C) and wo.shape == (C, C) and C == 320 and dh in (40, 64)
    KS, NU = C // 32, C // 16
    DP = 48 if dh == 40 else 64
    NT = DP // 16
    wqh, woh = wq.detach().to("cpu", torch.float16), wo.detach().to("cpu", torch.float16)      # host-side packing
    out = []
    for h in range(heads):
        q = torch.zeros(DP, C, dtype=torch.float16)
        q[:dh] = wqh[h * dh:(h + 1) * dh]
        pq = q.reshape(NT, 16, KS, 4, 8).permute(0, 2, 3, 1, 4).reshape(NT * KS, 512)          # [t, ks][g, l, i]
        o = torch.zeros(C, DP, dtype=torch.float16)
        o[:, :dh] = woh[:, h * dh:(h + 1) * dh]
        o32 = o[:, :32].reshape(NU, 16, 2, 4, 4).permute(0, 3, 1, 2, 4).reshape(-1)             # [u][g, l, i_hi, i_lo]
        if dh == 40:
            tail = o[:, 32:].reshape(NU, 16, 4, 4).permute(0, 2, 1, 3).reshape(-1)              # [u][g, l, i]
        else:
            tail = o[:, 32:].reshape(NU, 16, 2, 4, 4).permute(0, 3, 1, 2, 4).reshape(-1)        # the second K = 32 step: d 32..63
        out.append(torch.cat([pq.reshape(-1), o32, tail]).reshape(-1, 512))
    return torch.stack(out).contiguous().to(dev)


def pack_xattn_kv(K: torch.Tensor, V: torch.Tensor, rows: int, Lp: int, L: int, heads: int) -> torch.Tensor:
    """Fragment-major pack of the text keys / values of every batch row for skg_xattn_block_f16: K, V [rows * Lp, C] (what
    prepare_context hoists per prompt), L <= 80 valid keys per row.  Per (row, head), pieces of 512 halves.
    Head width 40 (16 pieces):
      K image: 5 K = 32 fragments [lane = 16 g + l][i] = K[key 16 kt + l][40 h + 16 (i >> 2) + 4 g + (i & 3)], then 5 K = 16
               fragments [lane][i < 4] = K[key 16 kt + l][40 h + 32 + 4 g + i]                                   (8 pieces)
      V image: (dt, s) K = 32 fragments [lane][i] = V[key 32 s + 16 (i >> 2) + 4 g + (i & 3)][40 h + 16 dt + l], then 3 K = 16
               fragments [lane][i < 4] = V[key 64 + 4 g + i][40 h + 16 dt + l]                                   (8 pieces)
    Head width 64 (20 pieces): K image [s][kt] 2 x 5 K = 32 fragments (d = 64 h + 32 s + ...), V image (dt < 4, s) 8 K = 32 fragments
    then 4 K = 16 fragments (2 pieces); no padding.
    Keys >= L and head columns >= the head width are zeros.  Returns fp16 [rows, heads, 16 | 20, 512] on K's device."""
    C = K.shape[1]
    dh = C // heads
    assert dh in (40, 64) and L <= 80 and K.shape == V.shape == (rows * Lp, C)
    dev = K.device
    DP = 48 if dh == 40 else 64
    NT = DP // 16
    k = torch.zeros(rows, heads, 80, DP, device=dev, dtype=torch.float16)
    v = torch.zeros(rows, heads, 80, DP, device=dev, dtype=torch.float16)
    k[:, :, :L, :dh] = K.reshape(rows, Lp, heads, dh)[:, :L].permute(0, 2, 1, 3)
    v[:, :, :L, :dh] = V.reshape(rows, Lp, heads, dh)[:, :L].permute(0, 2, 1, 3)
    R = rows * heads
    k, v = k.reshape(R, 80, DP), v.reshape(R, 80, DP)
    k32 = k[:, :, :32].reshape(R, 5, 16, 2, 4, 4).permute(0, 1, 4, 2, 3, 5).reshape(R, 5 * 512)      # [kt][g, l, i_hi, i_lo]
    v32 = v[:, :64].reshape(R, 2, 2, 4, 4, NT, 16).permute(0, 5, 1, 3, 6, 2, 4).reshape(R, 2 * NT * 512)   # [dt, s][g, l, i_hi, i_lo]
    v16 = v[:, 64:].reshape(R, 4, 4, NT, 16).permute(0, 3, 1, 4, 2).reshape(R, NT * 256)             # [dt][g, l, i]
    if dh == 64:
        k32b = k[:, :, 32:].reshape(R, 5, 16, 2, 4, 4).permute(0, 1, 4, 2, 3, 5).reshape(R, 5 * 512)
        return torch.cat([k32, k32b, v32, v16], 1).reshape(rows, heads, 20, 512).contiguous()
    k16 = k[:, :, 32:].reshape(R, 5, 16, 4, 4).permute(0, 1, 3, 2, 4).reshape(R, 5 * 256)            # [kt][g, l, i]
    pad_k = torch.zeros(R, 4096 - 5 * 768, device=dev, dtype=torch.float16)
    pad_v = torch.zeros(R, 4096 - 6 * 512 - 3 * 256, device=dev, dtype=torch.float16)
    return torch.cat([k32, k16, pad_k, v32, v16, pad_v], 1).reshape(rows, heads, 16, 512).contiguous()
