#!/usr/bin/env python3
"""Which static loss scale the SatMixin trainer needs (CPU only, oracle only): the oracle's fp16-storage emulation - forward and
backward rounded to fp16 at the tensor boundaries the HIP path stores - against the fp32 oracle, per parameter tensor, for a
range of loss scales.  TINY UNet, B = 2, timesteps (37, 803), 257 sketch tokens of N(0, 0.25), latents 32 x 32 and 16 x 16.

    python tools/sat_loss_scale.py [--out profiles/sat_loss_scale.txt]

The seed of the backward is scale * 2 (eps - noise) / numel.  numel is 8192 at the 32 x 32 test size and 65536 at SD1.5's training
size (4 x 4 x 64 x 64), so scale s at SD1.5's size puts the same magnitudes into the backward as s / 8 here: the row
"2^10" is what LOSS_SCALE = 2^13 does at SD1.5's eps scale, the row "2^16" what it would do on a single 32 x 32 sample of a
batch of 1 / 8 - the two ends bracket every batch / size the trainer is used at."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import attn_inject as oinj, ddim as oddim, unet as ounet  # noqa: E402
from sketch2img_amd.sat_train import LOSS_SCALE, add_noise  # noqa: E402

B, TS, SCALE = 2, (37, 803), 0.8


def run(W, sd, bt, emulate, loss_scale):
    p = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    st = bt["state"].clone().requires_grad_(True)
    noisy = add_noise(bt["lat"], bt["noise"], TS, bt["acp"])
    with ounet.fp16_storage(emulate):
        eps = torch.cat([ounet.unet_forward(ounet.TINY, W, noisy[b:b + 1], TS[b], bt["ehs"][b:b + 1],
                                            inject=oinj.make_clip_inject(p, st[b:b + 1], SCALE))[0] for b in range(B)])
        loss = torch.nn.functional.mse_loss(eps, bt["noise"])
        (loss * loss_scale).backward()
    return {k: p[k].grad / loss_scale for k in p}, st.grad / loss_scale


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = [f"LOSS_SCALE of the trainer: 2^{int(torch.log2(torch.tensor(LOSS_SCALE)))}",
             "relative L2 distance of the fp16-storage emulation from the fp32 oracle, per parameter tensor (176) and for d sketch_state"]
    W = ounet.init_weights(ounet.TINY)
    sd = oinj.init_state_dict(ounet.TINY, "clip")
    for h in (32, 16):
        g = torch.Generator().manual_seed(100 + h)
        bt = dict(lat=torch.randn(B, 4, h, h, generator=g), noise=torch.randn(B, 4, h, h, generator=g),
                  ehs=torch.randn(B, 77, ounet.TINY.cross_attention_dim, generator=g).half().float(),
                  state=(0.5 * torch.randn(B, 257, 1024, generator=g)).half().float(), acp=oddim.make_tables(50).alphas_cumprod)
        ref, ref_s = run(W, sd, bt, False, 1.0)
        for e in (0, 7, 10, 13, 16, 19):
            gr, ds = run(W, sd, bt, True, 2.0 ** e)
            rel = torch.tensor([float((gr[k] - ref[k]).norm() / ref[k].norm()) for k in ref])
            fin = all(bool(torch.isfinite(v).all()) for v in gr.values()) and bool(torch.isfinite(ds).all())
            worst = max(ref, key=lambda k: float((gr[k] - ref[k]).norm() / ref[k].norm()))
            lines.append(f"h={h:2d} scale 2^{e:<2d}: max {float(rel.max()):.3e} median {float(rel.median()):.3e} "
                         f"tensors > 1e-2: {int((rel > 1e-2).sum()):3d}  d_state {float((ds - ref_s).norm() / ref_s.norm()):.3e} "
                         f"finite {fin}  worst {worst.split('transformer_blocks_0.')[-1]}")
            print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
