#!/usr/bin/env python3
"""SatMixin training step timing (not a gate): SD1.5 synthetic weights, 64 x 64 latents, batch 4 (train.yaml).

    python tools/sat_train_bench.py [--out profiles/sat_train_bench.json] [--h 64] [--batch 4] [--iters 3]

Reports ms per step split into forward (stashing, per sample) / UNet backward / injected backward + weight gradients /
optimizer - device events around work that ends in a synchronise, after a warm-up step; the injected part is the sum of event
pairs around every HipClipInjectorTrain.backward call, the UNet part is the rest of the backward.
Then, on the step's actual (M, N, K) list, skg_wgrad_f16 against the composition it replaces: two ops.transpose +
ops.gemm(out_f32=True), both from the same build, 200 back-to-back calls per window, three alternating windows, the median.
The composition needs M % 32 == 0: its operands are zero-padded copies made OUTSIDE the timed region (in its favour)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sketch2img_amd import ops, sat_train, synthetic  # noqa: E402
from sketch2img_amd.config import SD15  # noqa: E402
from sketch2img_amd.inject import block_dims  # noqa: E402
from sketch2img_amd.sampler import DDIMTables  # noqa: E402
from sketch2img_amd.unet import HipUNet  # noqa: E402


def timed(fn, warmup=2, iters=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def wgrad_shapes(cfg, h, T=257):
    """(M, N, K, count per sample) of every weight gradient of one sample's backward."""
    nb = len(cfg.block_out_channels)
    out = {}
    for path, c, _ in block_dims(cfg):
        part = path.split(".")
        lvl = int(part[1]) if part[0] == "down_blocks" else (nb - 1 - int(part[1]) if part[0] == "up_blocks" else nb - 1)
        N = (h >> lvl) ** 2
        for shp in ((N, c, c), (N, c, c), (N, c, c), (N + T, c, c), (N + T, c, c), (T, c, 1024)):
            out[shp] = out.get(shp, 0) + 1
    return sorted((m, n, k, cnt) for (m, n, k), cnt in out.items())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--h", type=int, default=64)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--iters", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg, h, B = SD15, args.h, args.batch
    net = HipUNet(cfg, synthetic.unet_state_dict(cfg), dev)
    tr = sat_train.HipSatTrainer(cfg, synthetic.satmixin_state_dict(cfg, "clip"), dev, warmup_steps=0)
    lat, noise = synthetic.initial_latents(0, B, h), synthetic.initial_latents(100, B, h)
    ehs = synthetic.text_embeddings(B, cfg.cross_attention_dim)[B:]
    state = synthetic.sketch_state(0, B)[B:]
    acp = DDIMTables.make(50).alphas_cumprod
    ts = [(37 + 251 * i) % 1000 for i in range(B)]
    batch = (lat, noise, ts, ehs, state, acp)

    inj_events = []
    orig = tr.injector.backward

    def timed_backward(path, dout):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = orig(path, dout)
        b.record()
        inj_events.append((a, b))
        return r

    tr.injector.backward = timed_backward
    ev = lambda: torch.cuda.Event(enable_timing=True)
    rows = []
    for it in range(args.iters + 1):                 # iteration 0 is the warm-up
        inj_events.clear()
        e = [ev() for _ in range(4)]
        e[0].record()
        fw = tr.forward_batch(net, *batch)
        e[1].record()
        loss, g, _ = tr.backward_batch(net, fw)
        e[2].record()
        tr.all_reduce(g)
        stepped = tr.step(g)
        e[3].record()
        torch.cuda.synchronize()
        inj = sum(a.elapsed_time(b) for a, b in inj_events)
        bwd = e[1].elapsed_time(e[2])
        rows.append(dict(loss=float(loss), stepped=bool(stepped), forward_ms=e[0].elapsed_time(e[1]), unet_backward_ms=bwd - inj,
                         injected_backward_ms=inj, optimizer_ms=e[2].elapsed_time(e[3]), step_ms=e[0].elapsed_time(e[3])))
        print(json.dumps(rows[-1]), flush=True)
    steady = rows[1:]
    mean = {k: sum(r[k] for r in steady) / len(steady) for k in steady[0] if k.endswith("_ms")}
    res = {"device": torch.cuda.get_device_name(0), "h": h, "batch": B, "loss_scale": sat_train.LOSS_SCALE, "steps": rows,
           "mean_ms": mean, "wgrad": []}
    print(json.dumps({"mean_ms": mean}), flush=True)

    # ---- the weight-gradient kernel against the composition it replaces, on this step's shapes
    g = torch.Generator().manual_seed(0)
    for M, N, K, cnt in wgrad_shapes(cfg, h):
        dY = (0.05 * torch.randn(M, N, generator=g)).half().to(dev)
        X = torch.randn(M, K, generator=g).half().to(dev)
        Mp = (M + 31) // 32 * 32
        dYp, Xp = torch.zeros(Mp, N, device=dev, dtype=torch.float16), torch.zeros(Mp, K, device=dev, dtype=torch.float16)
        dYp[:M], Xp[:M] = dY, X
        dW = torch.zeros(N, K, device=dev)
        f_new = lambda: ops.wgrad(dY, X, dW, accumulate=True)
        f_old = lambda: ops.gemm(ops.transpose(dYp), ops.transpose(Xp), out_f32=True)
        rounds = [(timed(f_new, 5, 200), timed(f_old, 5, 200)) for _ in range(3)]      # alternating, median of three
        t_new, t_old = sorted(r[0] for r in rounds)[1], sorted(r[1] for r in rounds)[1]
        ref = ops.gemm(ops.transpose(dYp), ops.transpose(Xp), out_f32=True)
        new = ops.wgrad(dY, X)
        row = dict(M=M, N=N, K=K, per_sample=cnt, wgrad_us=1e3 * t_new, transpose2_gemm_us=1e3 * t_old,
                   rel_diff=float((new - ref).norm() / ref.norm()))
        res["wgrad"].append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
