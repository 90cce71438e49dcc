#!/usr/bin/env python3
"""Which scale the seam between the SatMixin backward and the CLIP vision tower's backward needs (CPU only, oracle only).

d loss / d sketch_state leaves the SatMixin step as fp32 x LOSS_SCALE (2^13) and is cast to fp16 to seed the tower's backward.  This
sweeps an extra power-of-two factor applied at that cast: the fp16-storage emulation (oracle.unet.fp16_storage for the UNet and the
injector, the tower emulation and the seam factor of tests/test_gpu_clip_train.py - one definition, loaded from there - for the ViT) against autograd of
the fp32 oracle, per tower parameter tensor.

    python tools/clip_loss_scale.py [--out profiles/clip_loss_scale.txt]

TINY UNet, 16 x 16 latents, B = 2, timesteps (37, 803).  Towers: the end-to-end test's (hidden 1024, 16 heads, I 256, 1 layer, 17 tokens)
and a deeper, wider one with the real token count (hidden 1024, 16 heads, I 4096, 4 layers, 257 tokens), where the gradient has further to
travel.  The seed of the UNet backward is 2^13 * 2 (eps - noise) / numel with numel = 2048 here and 65536 at SD1.5's 4 x 4 x 64 x 64, so
what factor 2^k does at SD1.5's size is what 2^(k - 5) does here: read the plateau with that shift."""
import argparse
import importlib.util
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import attn_inject as oinj, clip_vision as oclip, ddim as oddim, unet as ounet  # noqa: E402
from sketch2img_amd.sat_train import LOSS_SCALE, add_noise  # noqa: E402

B, TS, SCALE, H = 2, (37, 803), 0.8, 16
TOWERS = {"1 layer, 17 tokens": dict(hidden_size=1024, intermediate_size=256, num_hidden_layers=1, num_attention_heads=16, image_size=56,
                                     patch_size=14),
          "4 layers, 257 tokens": dict(hidden_size=1024, intermediate_size=4096, num_hidden_layers=4, num_attention_heads=16,
                                       image_size=224, patch_size=14)}


def _emulation():
    spec = importlib.util.spec_from_file_location("_clip_train_tests", os.path.join(ROOT, "tests", "test_gpu_clip_train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod._emulated_tokens, mod._SeamFactor


def run(W, sd, ocfg, Wc, bt, emulated_tokens, factor, seam_factor):
    """Tower gradients of the unscaled loss; emulated_tokens = None: the fp32 oracle."""
    emulate = emulated_tokens is not None
    scale = LOSS_SCALE if emulate else 1.0
    pc = {k: v.clone().requires_grad_(True) for k, v in Wc.items()}
    noisy = add_noise(bt["lat"], bt["noise"], TS, bt["acp"])
    with ounet.fp16_storage(emulate):
        st = emulated_tokens(ocfg, pc, bt["px"]) if emulate else oclip.last_hidden_state(ocfg, pc, bt["px"])
        st = seam_factor.apply(st, factor)
        eps = torch.cat([ounet.unet_forward(ounet.TINY, W, noisy[b:b + 1], TS[b], bt["ehs"][b:b + 1],
                                            inject=oinj.make_clip_inject(sd, st[b:b + 1], SCALE))[0] for b in range(B)])
        (torch.nn.functional.mse_loss(eps, bt["noise"]) * scale).backward()
    return {k: pc[k].grad / (scale * factor) for k in pc if pc[k].grad is not None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    emulated_tokens, seam_factor = _emulation()
    from sketch2img_amd.clip_vision_train import SEAM_SCALE
    lines = [f"LOSS_SCALE of the SatMixin trainer: 2^{int(torch.log2(torch.tensor(LOSS_SCALE)))}; swept: the extra factor at the seam "
             f"(SEAM_SCALE of the tower trainer: 2^{int(torch.log2(torch.tensor(SEAM_SCALE)))})",
             "relative L2 distance of the fp16-storage emulation from the fp32 oracle, per tower parameter tensor (d k_proj.bias, zero in "
             "exact arithmetic, left out)"]
    W = ounet.init_weights(ounet.TINY)
    sd = oinj.init_state_dict(ounet.TINY, "clip")
    for name, kw in TOWERS.items():
        ocfg = oclip.CLIPVisionConfig(**kw)
        Wc = oclip.init_weights(ocfg)
        g = torch.Generator().manual_seed(100 + H)
        bt = dict(lat=torch.randn(B, 4, H, H, generator=g), noise=torch.randn(B, 4, H, H, generator=g),
                  ehs=torch.randn(B, 77, ounet.TINY.cross_attention_dim, generator=g).half().float(),
                  px=torch.randn(B, 3, ocfg.image_size, ocfg.image_size, generator=g).half().float(),
                  acp=oddim.make_tables(50).alphas_cumprod)
        ref = run(W, sd, ocfg, Wc, bt, None, 1.0, seam_factor)
        keys = [k for k in ref if not k.endswith("k_proj.bias")]
        for e in (-13, -9, -6, -3, 0, 3, 6, 9, 12, 15, 18, 21):
            gr = run(W, sd, ocfg, Wc, bt, emulated_tokens, 2.0 ** e, seam_factor)
            rel = torch.tensor([float((gr[k] - ref[k]).norm() / ref[k].norm()) for k in keys])
            fin = all(bool(torch.isfinite(v).all()) for v in gr.values())
            worst = keys[int(torch.nan_to_num(rel, nan=float("inf")).argmax())]
            lines.append(f"{name:22s} seam 2^{e:<3d}: max {float(rel.max()):.3e} median {float(rel.median()):.3e} "
                         f"tensors > 1e-2: {int((rel > 1e-2).sum()):3d} of {len(keys)}  finite {fin}  worst {worst}")
            print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
