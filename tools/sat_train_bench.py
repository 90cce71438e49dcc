#!/usr/bin/env python3
"""SatMixin training step timing (not a gate): SD1.5 synthetic weights, 64 x 64 latents, batch 4 (train.yaml).

    python tools/sat_train_bench.py [--out profiles/sat_train_bench.json] [--h 64] [--batch 4] [--iters 3]
    python tools/sat_train_bench.py --batched [--batches 4,8] [--windows 3] [--iters 3] [--txt profiles/sat_train_batched.txt]

Reports ms per step split into forward (stashing, per sample) / UNet backward / injected backward + weight gradients /
optimizer - device events around work that ends in a synchronise, after a warm-up step; the injected part is the sum of event
pairs around every HipClipInjectorTrain.backward call, the UNet part is the rest of the backward.
Then, on the step's actual (M, N, K) list, skg_wgrad_f16 against the composition it replaces: two ops.transpose +
ops.gemm(out_f32=True), both from the same build, 200 back-to-back calls per window, three alternating windows, the median.
The composition needs M % 32 == 0: its operands are zero-padded copies made OUTSIDE the timed region (in its favour).

--batched: the one-walk mode (batched=True) against the per-sample step - whose launches are the parent commit's, pinned bit for
bit by tests/test_gpu_sat_train.py - in the SAME process: per batch size `windows` alternating windows (per-sample, batched,
per-sample, ...) of `iters` steps each after one warm-up step per mode; per part the median over the windows and their min ... max
spread.  Prints text lines (and appends them to --txt); the weight-gradient comparison is skipped."""
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


def step_parts(tr, net, batch, batched, inj_events):
    """One training step -> its parts in ms (device events; ends in a synchronise)."""
    ev = lambda: torch.cuda.Event(enable_timing=True)
    inj_events.clear()
    e = [ev() for _ in range(4)]
    e[0].record()
    fw = tr.forward_batch(net, *batch, batched=batched)
    e[1].record()
    loss, g, _ = tr.backward_batch(net, fw, batched=batched)
    e[2].record()
    tr.all_reduce(g)
    stepped = tr.step(g)
    e[3].record()
    torch.cuda.synchronize()
    inj = sum(a.elapsed_time(b) for a, b in inj_events)
    bwd = e[1].elapsed_time(e[2])
    return dict(loss=float(loss), stepped=bool(stepped), forward_ms=e[0].elapsed_time(e[1]), unet_backward_ms=bwd - inj,
                injected_backward_ms=inj, optimizer_ms=e[2].elapsed_time(e[3]), step_ms=e[0].elapsed_time(e[3]))


def compare_batched(tr, net, cfg, h, batches, windows, iters, inj_events, txt):
    """Alternating windows of the per-sample and the batched step -> text lines."""
    acp = DDIMTables.make(50).alphas_cumprod
    lines = [f"# {torch.cuda.get_device_name(0)}; SD1.5 synthetic, {h} x {h} latents; ms per step, median of {windows} alternating windows "
             f"of {iters} steps [min ... max of the windows]; per-sample = the parent commit's launches"]
    parts = ("step_ms", "forward_ms", "unet_backward_ms", "injected_backward_ms", "optimizer_ms")
    for B in batches:
        lat, noise = synthetic.initial_latents(0, B, h), synthetic.initial_latents(100, B, h)
        batch = (lat, noise, [(37 + 251 * i) % 1000 for i in range(B)], synthetic.text_embeddings(B, cfg.cross_attention_dim)[B:],
                 synthetic.sketch_state(0, B)[B:], acp)
        win = {False: [], True: []}
        for mode in (False, True):
            step_parts(tr, net, batch, mode, inj_events)                     # warm-up
        for _ in range(windows):
            for mode in (False, True):
                rows = [step_parts(tr, net, batch, mode, inj_events) for _ in range(iters)]
                win[mode].append({k: sum(r[k] for r in rows) / len(rows) for k in parts})
        med = {}
        for mode, name in ((False, "per-sample"), (True, "batched")):
            cells = []
            for k in parts:
                v = sorted(w[k] for w in win[mode])
                med[(mode, k)] = v[len(v) // 2]
                cells.append(f"{k[:-3]} {v[len(v) // 2]:.2f} [{v[0]:.2f} ... {v[-1]:.2f}]")
            lines.append(f"batch {B} {name:10s} " + "  ".join(cells))
        lines.append(f"batch {B} per-sample / batched: " + "  ".join(f"{k[:-3]} x{med[(False, k)] / med[(True, k)]:.2f}" for k in parts))
    for ln in lines:
        print(ln, flush=True)
    if txt:
        with open(txt, "a") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--h", type=int, default=64)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--batched", action="store_true", help="compare batched=True with the per-sample step (see the docstring)")
    ap.add_argument("--batches", default="4,8")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--txt", default=None)
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
    if args.batched:
        compare_batched(tr, net, cfg, h, [int(b) for b in args.batches.split(",")], args.windows, args.iters, inj_events, args.txt)
        return
    rows = []
    for it in range(args.iters + 1):                 # iteration 0 is the warm-up
        rows.append(step_parts(tr, net, batch, False, inj_events))
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
