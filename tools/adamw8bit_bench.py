#!/usr/bin/env python3
"""8-bit AdamW state timings and the convergence margin (not a gate) -> profiles/adamw8bit.txt.

    python tools/adamw8bit_bench.py [--out profiles/adamw8bit.txt] [--n 300000000] [--windows 5] [--iters 10] [--no-convergence]

1. One flat tensor of n elements (3e8: the ViT-L/14 tower's): skg_adamw8_step (FlatAdamW(state_bits=8)'s launch: block table, codes,
   absmax) and skg_adamw_step on the same masters and gradient, in one process, alternating windows, device events around back-to-back
   launches.  GB/s on the bytes each form has to move per element: 18 (p r/w 8, g 4, two codes r/w 4, p16 2; + 8 per 2048 for the
   absmax) and 30 (m, v r/w 16 instead of the codes).  State bytes of both.
2. The convergence problem of tests/test_gpu_adamw8bit.py (1/2 |p - target|^2, 10 067 elements in four tensors, 200 steps at lr 1e-2):
   final loss of the GPU's 8-bit run, of the numpy checker's 8-bit run (tests/adamw8bit_ref.py), their margin, and the GPU's fp32 run.

Every timing: the median and [min ... max] of `windows` alternating windows after a warm-up of each."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sketch2img_amd import flat_adamw, ops  # noqa: E402
from tools.loss_scaler_bench import alternate, cell, device_ms  # noqa: E402

DEV = torch.device("cuda:0")
CONV = [("a", (5000,)), ("b", (64, 65)), ("c", (900,)), ("d", (7,))]


def opt(shapes, sd, bits, lr, grad_scale):
    return flat_adamw.FlatAdamW(shapes, sd, DEV, lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, schedule=lambda s: 1.0,
                                grad_scale=grad_scale, state_bits=bits)


def convergence():
    from tests import adamw8bit_ref as ref
    g = torch.Generator().manual_seed(6)
    sd = {k: torch.randn(shp, generator=g) for k, shp in CONV}
    st8, st32 = opt(CONV, sd, 8, 1e-2, 1.0), opt(CONV, sd, 32, 1e-2, 1.0)
    gen = torch.Generator().manual_seed(7)
    target = torch.zeros(st8.n)
    for k, (off, shp) in st8.layout.items():
        target[off:off + shp.numel()] = torch.randn(shp.numel(), generator=gen)
    chk = ref.Adam8([st8.w32(k).cpu().numpy() for k, _ in CONV], 1e-2, (0.9, 0.999), 1e-8, 1e-2)
    tnp = [target[st8.layout[k][0]:st8.layout[k][0] + st8.layout[k][1].numel()].numpy() for k, _ in CONV]
    tdev = target.to(DEV)
    loss_dev = lambda st: 0.5 * float(((st.p.double() - tdev.double()) ** 2).sum())
    start = loss_dev(st8)
    for _ in range(200):
        for st in (st8, st32):
            st.step(st.p - tdev, checked=True)
        chk.step([(p - t).astype(np.float32) for p, t in zip(chk.p, tnp)])
    lref = 0.5 * sum(float(((p.astype(np.float64) - t) ** 2).sum()) for p, t in zip(chk.p, tnp))
    l8, l32 = loss_dev(st8), loss_dev(st32)
    return (f"convergence 1/2|p - target|^2, {st8.n_opt} elements, 200 steps, lr 1e-2: start {start:.6e}  GPU 8-bit {l8:.6e}  "
            f"checker 8-bit {lref:.6e}  margin (GPU - checker) / checker {(l8 - lref) / lref:+.3e}  GPU fp32 {l32:.6e}  "
            f"8-bit / fp32 {l8 / l32:.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adamw8bit.txt"))
    ap.add_argument("--n", type=int, default=300000000)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--no-convergence", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    n, W = args.n, args.windows
    lines = [f"# {torch.cuda.get_device_name(0)}; ms, median of {W} alternating windows [min ... max of the windows]",
             f"# python tools/adamw8bit_bench.py --n {n} --windows {W} --iters {args.iters}"]

    def say(s):
        lines.append(s)
        print(s, flush=True)

    st = opt([("w", (n,))], {"w": torch.randn(n)}, 8, 2e-4, 8192.0)
    g = torch.randn(st.n, device=DEV) * 64.0
    p, p16 = st.p.clone(), st.p16.clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    hyper = (2e-4, 0.9, 0.999, 1e-8, 1e-2, 10, 1.0 / 8192)
    step8 = lambda: ops.adamw8_step(st.p, g, st.p16, st.state1, st.state2, st.absmax1, st.absmax2, st.m32, st.v32, st.rows, st.qtab,
                                    *hyper)
    r = alternate({"q8": lambda: device_ms(step8, args.iters),
                   "f32": lambda: device_ms(lambda: ops.adamw_step(p, g, m, v, p16, *hyper), args.iters)}, W)
    rows = st.rows.shape[0]
    say(f"adamw n={n} ({rows} blocks of 2048): skg_adamw8_step {cell(r['q8'])} ({18e-6 * n / r['q8'][0]:.0f} GB/s at 18 B per element)  "
        f"skg_adamw_step {cell(r['f32'])} ({30e-6 * n / r['f32'][0]:.0f} GB/s at 30 B per element)  "
        f"fp32 / 8-bit time x{r['f32'][0] / r['q8'][0]:.3f} (ceiling x{30 / 18:.2f})")
    say(f"state n={n}: 8-bit {st.state_bytes()} bytes (codes {2 * st.state1.numel()}, absmax {8 * rows}, maps + thresholds "
        f"{4 * st.qtab.numel()}; block table {8 * st.rows.numel()} beside it)  fp32 {8 * n} bytes  x{st.state_bytes() / (8 * n):.4f}")
    del st, g, p, p16, m, v
    torch.cuda.empty_cache()
    if not args.no_convergence:
        say(convergence())
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
