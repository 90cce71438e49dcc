#!/usr/bin/env python3
"""Dynamic loss scale timings (not a gate) -> profiles/loss_scaler.txt.

    python tools/loss_scaler_bench.py [--out profiles/loss_scaler.txt] [--sizes 1048576,16777216,300000000] [--windows 5]
                                      [--h 64] [--batch 4] [--iters 5] [--no-step]

1. The verdict over a flat fp32 vector of n floats (2^20, 2^24, 3e8 - the tower's): skg_nonfinite_flag against the static path's
   bool(torch.isfinite(g).all()).  Two figures each: "device" = device events around back-to-back launches (the flag kernel; for torch
   the isfinite + all kernels without the read-back), "verdict" = a host clock from the call to the answer on the host (the flag
   kernel + the 4-byte read-back; torch's bool()).  GB/s = 4 n bytes over the device time.
2. skg_adamw_step_guarded (flag 0) against skg_adamw_step on the same vectors, device events.
3. A SatMixin training step (SD1.5 synthetic weights, h x h latents, batched=True) with scaler= against the static step, whole
   train_step calls on a host clock that ends in a synchronise.

Every figure: `windows` alternating windows (a, b, a, b, ...) after a warm-up of each, the median and [min ... max] of the windows -
the spread a difference has to exceed."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sketch2img_amd import loss_scaler, ops, sat_train, synthetic  # noqa: E402
from sketch2img_amd.config import SD15  # noqa: E402
from sketch2img_amd.sampler import DDIMTables  # noqa: E402
from sketch2img_amd.unet import HipUNet  # noqa: E402

DEV = torch.device("cuda:0")


def device_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def host_ms(fn, iters):
    """fn ends with its answer on the host (or the caller synchronises inside fn)."""
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t) / iters


def alternate(timers, windows):
    """timers: {name: () -> ms}.  -> {name: (median, min, max)} over alternating windows, one warm-up call of each first."""
    for f in timers.values():
        f()
    rows = {k: [] for k in timers}
    for _ in range(windows):
        for k, f in timers.items():
            rows[k].append(f())
    out = {}
    for k, v in rows.items():
        v = sorted(v)
        out[k] = (v[len(v) // 2], v[0], v[-1])
    return out


def cell(t):
    return f"{t[0]:.4f} [{t[1]:.4f} ... {t[2]:.4f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_scaler.txt"))
    ap.add_argument("--sizes", default=f"{1 << 20},{1 << 24},300000000")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--h", type=int, default=64)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--no-step", action="store_true", help="kernels only: skip the SatMixin step")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    W = args.windows
    lines = [f"# {torch.cuda.get_device_name(0)}; ms, median of {W} alternating windows [min ... max of the windows]",
             f"# python tools/loss_scaler_bench.py --sizes {args.sizes} --windows {W} --h {args.h} --batch {args.batch} --iters {args.iters}"]

    def say(s):
        lines.append(s)
        print(s, flush=True)

    for n in [int(s) for s in args.sizes.split(",")]:
        iters = max(5, min(200, (1 << 28) // n))
        g = torch.randn(n, device=DEV) * 64.0
        flag = torch.zeros(1, device=DEV)
        ops.nonfinite_flag(g, flag, reset=True)
        assert float(flag) == 0.0 and bool(torch.isfinite(g).all())
        r = alternate({
            "flag_dev": lambda: device_ms(lambda: ops.nonfinite_flag(g, flag, reset=True), iters),
            "torch_dev": lambda: device_ms(lambda: torch.isfinite(g).all(), iters),
            "flag_host": lambda: host_ms(lambda: (ops.nonfinite_flag(g, flag, reset=True), float(flag)), iters),
            "torch_host": lambda: host_ms(lambda: bool(torch.isfinite(g).all()), iters)}, W)
        say(f"verdict n={n}: skg_nonfinite_flag device {cell(r['flag_dev'])} ({4e-6 * n / r['flag_dev'][0]:.0f} GB/s)  "
            f"torch.isfinite(g).all() device {cell(r['torch_dev'])} ({4e-6 * n / r['torch_dev'][0]:.0f} GB/s)  x{r['torch_dev'][0] / r['flag_dev'][0]:.2f}")
        say(f"verdict n={n}: flag + 4-byte read-back, host {cell(r['flag_host'])}  bool(torch.isfinite(g).all()), host {cell(r['torch_host'])}  "
            f"x{r['torch_host'][0] / r['flag_host'][0]:.2f}")
        p, m, v = torch.randn(n, device=DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        p16 = p.half()
        hyper = (2e-4, 0.9, 0.999, 1e-8, 1e-2, 10, 1.0 / 8192)
        r = alternate({
            "plain": lambda: device_ms(lambda: ops.adamw_step(p, g, m, v, p16, *hyper), iters),
            "guarded": lambda: device_ms(lambda: ops.adamw_step_guarded(p, g, m, v, p16, *hyper, flag), iters)}, W)
        say(f"adamw   n={n}: skg_adamw_step {cell(r['plain'])}  skg_adamw_step_guarded (flag 0) {cell(r['guarded'])}  "
            f"guarded / plain x{r['guarded'][0] / r['plain'][0]:.3f}  ({30e-6 * n / r['plain'][0]:.0f} GB/s at 30 B per element)")
        del g, p, m, v, p16
        torch.cuda.empty_cache()

    if not args.no_step:
        cfg, h, B = SD15, args.h, args.batch
        net = HipUNet(cfg, synthetic.unet_state_dict(cfg), DEV)
        sd = synthetic.satmixin_state_dict(cfg, "clip")
        static = sat_train.HipSatTrainer(cfg, sd, DEV, warmup_steps=0)
        scaled = sat_train.HipSatTrainer(cfg, sd, DEV, warmup_steps=0)
        sc = loss_scaler.DynamicLossScaler(DEV, init_scale=sat_train.LOSS_SCALE)
        lat, noise = synthetic.initial_latents(0, B, h), synthetic.initial_latents(100, B, h)
        ehs, state = synthetic.text_embeddings(B, cfg.cross_attention_dim)[B:], synthetic.sketch_state(0, B)[B:]
        acp = DDIMTables.make(50).alphas_cumprod
        ts = [(37 + 251 * i) % 1000 for i in range(B)]
        step = lambda tr, **kw: sat_train.train_step(tr, net, lat, ehs, state, ts, noise, acp, batched=True, **kw)
        r = alternate({"static": lambda: host_ms(lambda: step(static), args.iters),
                       "scaler": lambda: host_ms(lambda: step(scaled, scaler=sc), args.iters)}, W)
        sc.resolve()
        assert static.step_count == scaled.step_count and sc.scale == sat_train.LOSS_SCALE
        spread = max(r["static"][2] - r["static"][1], r["scaler"][2] - r["scaler"][1])
        say(f"SatMixin step SD1.5 {h} x {h} batch {B} batched, n = {static.n} floats: static {cell(r['static'])}  scaler= {cell(r['scaler'])}  "
            f"scaler - static {r['scaler'][0] - r['static'][0]:+.4f} ms (largest window spread {spread:.4f} ms); "
            f"{static.step_count} steps each, all counted")
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
