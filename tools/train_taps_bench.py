#!/usr/bin/env python3
"""lgp_train.unet_taps on one MI355X: the per-sample loop (B walks of one row) against the batched walk (one walk of B rows with a
timestep per sample, the conv1 epilogues reading a bias row per sample).

Synthetic SD1.5 weights, 64 x 64 latents, B = 4 (train.yaml batch_size: 4), random distinct timesteps.  Both forms run in ONE
process on one box: warm-up of both, then `--repeats` timed runs of each in alternating order (A B A B ...), each run `--iters`
calls between two device synchronisations; the median per call of each form and their ratio are printed and written to --out.
A record, not a gate (EXPERIMENTS.md)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--latent", type=int, default=64)
    ap.add_argument("--iters", type=int, default=5, help="unet_taps calls per timed run")
    ap.add_argument("--repeats", type=int, default=7, help="timed runs per form, alternating")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="text file for the result lines")
    a = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "needs a GPU: a time measured anywhere else says nothing"
    from sketch2img_amd import synthetic
    from sketch2img_amd.config import SD15
    from sketch2img_amd.lgp_train import unet_taps
    from sketch2img_amd.unet import HipUNet
    dev = "cuda:0"
    net = HipUNet(SD15, synthetic.unet_state_dict(SD15), dev, need_backward=False)
    g = torch.Generator().manual_seed(a.seed)
    B, h = a.batch, a.latent
    noisy = torch.randn(B, 4, h, h, generator=g).to(dev)
    ehs = torch.randn(B, 77, SD15.cross_attention_dim, generator=g).half().float()
    ts = torch.randperm(1000, generator=g)[:B].tolist()      # distinct
    net.prepare_timesteps(ts)

    def run(batched: bool, n: int) -> float:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            unet_taps(net, noisy, ts, ehs, batched=batched)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    for _ in range(a.warmup):
        run(False, 1), run(True, 1)
    # same seeded inputs, both forms: the taps agree to fp16 rounding noise (other kernel instantiations, another summation order)
    ta, tb = unet_taps(net, noisy, ts, ehs, batched=False), unet_taps(net, noisy, ts, ehs, batched=True)
    rel = max(float((x.float() - y.float()).norm() / y.float().norm()) for (x, _), (y, _) in zip(tb, ta))
    times = {False: [], True: []}
    for r in range(a.repeats):
        for batched in ((False, True) if r % 2 == 0 else (True, False)):
            times[batched].append(run(batched, a.iters))
    med = {k: statistics.median(v) for k, v in times.items()}
    res = dict(metric="lgp_train.unet_taps, SD1.5 synthetic, ms per call", batch=B, latent=h, timesteps=ts, iters=a.iters, repeats=a.repeats,
               per_sample_ms=round(med[False], 2), batched_ms=round(med[True], 2), ratio_per_sample_over_batched=round(med[False] / med[True], 3),
               per_sample_runs_ms=[round(v, 2) for v in times[False]], batched_runs_ms=[round(v, 2) for v in times[True]],
               worst_tap_rel_batched_vs_per_sample=float(f"{rel:.3e}"), device=torch.cuda.get_device_name(0))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(f"# tools/train_taps_bench.py --batch {B} --latent {h} --iters {a.iters} --repeats {a.repeats}\n{line}\n")


if __name__ == "__main__":
    main()
