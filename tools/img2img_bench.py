#!/usr/bin/env python3
"""img2img timings (not a gate) -> profiles/img2img.txt.

    python tools/img2img_bench.py [--out profiles/img2img.txt] [--samples 8] [--h 64] [--steps 50] [--strength 0.8] [--windows 3]

SD1.5 synthetic weights, h x h latents, `samples` samples, DDIM, eager launches: HipSampler.sample(init_latents=, start_step=) over the
int(steps * strength) executed steps, once with a mask (one skg_latent_renoise launch at the end of every step) and once without.
Whole sample() calls on a host clock that ends in a synchronise; `windows` alternating windows (mask, no mask, mask, ...) after one
warm-up call of each, the median and [min ... max] of the windows - the spread the difference has to exceed to mean anything.  The
kernel alone (device events around back-to-back launches) is printed next to it."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sketch2img_amd import ops, synthetic  # noqa: E402
from sketch2img_amd.config import SD15  # noqa: E402
from sketch2img_amd.sampler import DDIMTables, HipSampler, start_step  # noqa: E402
from sketch2img_amd.unet import HipUNet  # noqa: E402

DEV = torch.device("cuda:0")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "img2img.txt"))
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--h", type=int, default=64)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--strength", type=float, default=0.8)
    ap.add_argument("--windows", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    S, h, T = args.samples, args.h, args.steps
    k = start_step(T, args.strength)
    n = T - k
    net = HipUNet(SD15, synthetic.unet_state_dict(SD15), DEV)
    net.prepare_context(synthetic.text_embeddings(S, SD15.cross_attention_dim))
    tab = DDIMTables.make(T)
    sampler = HipSampler(net, None)
    init = (0.18215 * 4.0 * synthetic.initial_latents(100, S, h)).to(DEV)
    eps = synthetic.initial_latents(0, S, h).to(DEV)
    mask = torch.zeros(1, 1, h, h)
    mask[..., h // 4: 3 * h // 4, h // 4: 3 * h // 4] = 1.0            # repaint the centre

    def run(m):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = sampler.sample(eps, None, T, tables=tab, init_latents=init, start_step=k, mask=m)
        torch.cuda.synchronize()
        assert len(sampler.last_aux) == n and bool(torch.isfinite(out).all())
        return 1e3 * (time.perf_counter() - t)

    timers = {"mask": lambda: run(mask), "plain": lambda: run(None)}
    for f in timers.values():
        f()
    rows = {key: [] for key in timers}
    for _ in range(args.windows):
        for key, f in timers.items():
            rows[key].append(f())
    stat = {key: (sorted(v)[len(v) // 2], min(v), max(v)) for key, v in rows.items()}
    cell = lambda t: f"{t[0]:.2f} [{t[1]:.2f} ... {t[2]:.2f}]"
    diff = (stat["mask"][0] - stat["plain"][0]) / n
    spread = max(stat[key][2] - stat[key][1] for key in stat) / n

    md, x = mask.to(DEV), eps.clone()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    iters = 200
    ops.latent_renoise(init, eps, 0.6, 0.8, x=x, mask=md)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        ops.latent_renoise(init, eps, 0.6, 0.8, x=x, mask=md)
    b.record()
    torch.cuda.synchronize()
    kern = 1e3 * a.elapsed_time(b) / iters

    lines = [f"# {torch.cuda.get_device_name(0)}; ms per sample() call, median of {args.windows} alternating windows [min ... max]",
             f"# python tools/img2img_bench.py --samples {S} --h {h} --steps {T} --strength {args.strength} --windows {args.windows}",
             f"SD1.5 {h} x {h} latents, {S} samples, DDIM {T} steps, strength {args.strength}: start {k}, {n} executed steps, eager",
             f"  with a mask : {cell(stat['mask'])}  = {stat['mask'][0] / n:.3f} ms per step",
             f"  without     : {cell(stat['plain'])}  = {stat['plain'][0] / n:.3f} ms per step",
             f"  mask - plain: {diff:+.4f} ms per step (largest window spread {spread:.4f} ms per step)",
             f"  skg_latent_renoise alone, masked, [{S}, 4, {h}, {h}]: {kern:.2f} us per launch, back-to-back launches on device events"]
    print("\n".join(lines), flush=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
