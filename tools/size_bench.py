#!/usr/bin/env python3
"""Throughput of the config-2 workload (SD1.5 synthetic weights, LGP sketch guidance on steps 0..25 of 50 DDIM steps, CFG 7.5,
VAE decode to uint8) at square and non-square image sizes, in both UNet modes.  bench.py times 512 x 512 only; this tool
repeats its batch at other sizes and prints one JSON line per (size, mode): images/s, ms per image, ms per megapixel, and the
per-level launch choices that depend on the map's size (fused cross-attention / feed-forward launches at HW % 128 == 0, GroupNorm
sums from the producers, Winograd on even sides) - the "fallback" entries list each fast path a level takes at 512 x 512 and not here.

    python tools/size_bench.py                       (512x512, 768x512, 512x768, 576x320; fast + accuracy mode)
    python tools/size_bench.py --sizes 768x512 --modes fast --steps 3
Sizes are WIDTH x HEIGHT in pixels.  Inputs: seeded N(0, 1) latents and 0.18215 * N(0, 1) sketch targets of the size's
latent shape (synthetic.sketch_targets draws square canvases only)."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def launch_choices(net, rows: int, h: int, w: int):
    """What HipUNet's shape gates pick per resolution level for `rows` UNet rows of an h x w latent, and the fallbacks: every
    fast path that the same level takes at 512 x 512 (64 x 64 latents) and this size does not."""
    from sketch2img_amd import ops, unet as U
    cfg = net.cfg

    def levels(h, w):
        out = []
        for k, C in enumerate(cfg.block_out_channels):
            sz = (h >> k, w >> k)
            HW = sz[0] * sz[1]
            lv = dict(level=k, map=f"{sz[0]}x{sz[1]}", HW=HW, C=C)
            if C == 320:          # the fused cross-attention / feed-forward(+proj_out) launches exist for the 320-channel level
                lv["fused_xattn_ff_proj"] = HW % 128 == 0
            lv["gn_from_producer"] = bool(U._GN_FROM_PRODUCER and HW >= 1024 and ops.gn_fusable(rows * HW, C, HW, cfg.norm_groups))
            lv["winograd"] = rows * HW // 4 >= U._WINO_MIN_TILES and not (sz[0] & 1) and not (sz[1] & 1)
            out.append(lv)
        return out

    what = dict(fused_xattn_ff_proj="fused cross-attention / feed-forward launches -> per-operator launches",
                gn_from_producer="GroupNorm sums from the producers' epilogues -> a separate statistics pass",
                winograd="Winograd ResnetBlock convolutions -> implicit GEMM")
    out = levels(h, w)
    fallback = [f"level {d['level']} ({d['map']}): {what[k]}" for d, d0 in zip(out, levels(64, 64)) for k in what
                if d0.get(k) and not d.get(k)]
    return out, fallback


def run(width: int, height: int, accuracy: bool, samples: int, steps: int, warmup: int, T: int, dev):
    from sketch2img_amd import synthetic
    from sketch2img_amd.config import SD15, SD_VAE, tap_channels
    from sketch2img_amd.lgp import HipLGP
    from sketch2img_amd.modules.pipeline import check_image_size
    from sketch2img_amd.sampler import DDIMTables, HipSampler
    from sketch2img_amd.unet import HipUNet
    from sketch2img_amd.vae import HipVAEDecoder
    check_image_size(height, width)
    h, w = height // 8, width // 8
    net = HipUNet(SD15, synthetic.unet_state_dict(SD15), dev, residual_fp32=accuracy)
    lgp = HipLGP(synthetic.lgp_state_dict(synthetic.lgp_input_dim(SD15)), tap_channels(SD15), dev)
    vae = HipVAEDecoder(SD_VAE, synthetic.vae_decoder_state_dict(SD_VAE), dev)
    net.prepare_context(synthetic.text_embeddings(samples, dim=SD15.cross_attention_dim))
    tab = DDIMTables.make(T)
    net.prepare_timesteps(tab.timesteps.tolist())
    g = torch.Generator().manual_seed(height * 10000 + width)
    lat0 = torch.randn(samples, 4, h, w, generator=g).to(dev)
    target = (0.18215 * torch.randn(samples, 4, h, w, generator=g)).to(dev)
    sampler = HipSampler(net, lgp)

    def one():
        return vae.decode_to_u8(sampler.sample(lat0, target, T, tables=tab))

    for _ in range(warmup):
        one()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = one()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    assert tuple(out.shape) == (samples, height, width, 3)
    levels, fallback = launch_choices(net, 2 * samples, h, w)
    ms_img = 1e3 * dt / samples
    return dict(size=f"{width}x{height}", latents=[h, w], mode="accuracy" if accuracy else "fast", samples=samples,
                ddim_steps=T, images_per_s=samples / dt, ms_per_image=ms_img, ms_per_megapixel=ms_img / (width * height / 1e6),
                fallback=fallback, levels=levels)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512x512,768x512,512x768,576x320", help="comma-separated WIDTHxHEIGHT list")
    ap.add_argument("--modes", default="fast,accuracy")
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ddim-steps", type=int, default=50)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for size in a.sizes.split(","):
        width, height = (int(v) for v in size.lower().split("x"))
        for mode in a.modes.split(","):
            r = run(width, height, mode == "accuracy", a.samples, a.steps, a.warmup, a.ddim_steps, dev)
            print(json.dumps(r), flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
