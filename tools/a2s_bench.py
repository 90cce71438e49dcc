#!/usr/bin/env python3
"""Sketch generator timing (not a gate): ms per picture at 1024 x 1024 and 512 x 512, B = 1 and 4, device events around work that
ends in a synchronise, after a warm-up; the algorithmic flop count of the layer table; for orientation a plain
torch.nn.functional restatement of the network on the same box, if PyTorch's convolutions run there.

    python tools/a2s_bench.py [--out profiles/a2s_bench.json] [--no-torch] [--once H B]

--once H B: one warmed-up forward only (what `rocprofv3 --kernel-trace --stats -- python tools/a2s_bench.py --once 1024 1` traces)."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sketch2img_amd import synthetic  # noqa: E402
from sketch2img_amd.anime2sketch import CH, HipSketchGenerator  # noqa: E402


def flops(H, W):
    """2 x multiply-adds of the 16 layers: a 4 x 4 stride-2 convolution spends 16 Cin per output value, its transpose 4 Cin."""
    px = [(H >> k) * (W >> k) for k in range(9)]
    total = sum(2 * px[k] * CH[k] * 16 * CH[k - 1] for k in range(1, 9))
    shapes = list(synthetic.anime2sketch_param_shapes().values())[16::2][::-1]      # up convolution of level 1 .. 8: (Cin, Cout, 4, 4)
    total += sum(2 * px[k - 1] * shapes[k - 1][1] * 4 * shapes[k - 1][0] for k in range(1, 9))
    return total


def torch_forward(W, x):
    """The same network with torch operators (comparison only; fp16, NCHW)."""
    keys = list(W)
    dn, up = keys[0:16:2], keys[16:32:2][::-1]
    d = [F.conv2d(x, W[dn[0]], W[dn[0][:-6] + "bias"], stride=2, padding=1)]
    for k in range(1, 8):
        y = F.conv2d(F.leaky_relu(d[-1], 0.2), W[dn[k]], W[dn[k][:-6] + "bias"], stride=2, padding=1)
        d.append(F.instance_norm(y) if k < 7 else y)
    u = d[7]
    for k in range(7, -1, -1):
        inp = F.relu(u if k == 7 else torch.cat([d[k], u], 1))
        u = F.conv_transpose2d(inp, W[up[k]], W[up[k][:-6] + "bias"], stride=2, padding=1)
        u = F.instance_norm(u) if k > 0 else torch.tanh(u)
    return u


def timed(fn, warmup=3, iters=10):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--once", nargs=2, type=int, default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    W = synthetic.anime2sketch_state_dict()
    eng = HipSketchGenerator(W, dev)
    if args.once:
        H, B = args.once
        x = synthetic.pictures(0, 1, H, H).expand(B, -1, -1, -1).contiguous().to(dev)
        eng.forward(x)
        torch.cuda.synchronize()
        eng.forward(x)
        torch.cuda.synchronize()
        return
    Wh = {k: v.half().to(dev) for k, v in W.items()}
    res = {"device": torch.cuda.get_device_name(0), "cases": []}
    for H in (1024, 512):
        for B in (1, 4):
            x = synthetic.pictures(0, 1, H, H).expand(B, -1, -1, -1).contiguous().to(dev)
            ms = timed(lambda: eng.forward(x))
            case = {"H": H, "W": H, "B": B, "ms_per_picture": ms / B, "gflop_per_picture": flops(H, H) / 1e9,
                    "tflops": flops(H, H) * B / ms / 1e9}
            if not args.no_torch:
                try:
                    xh = x.half()
                    with torch.no_grad():
                        case["torch_functional_ms_per_picture"] = timed(lambda: torch_forward(Wh, xh)) / B
                except RuntimeError as e:      # PyTorch's convolutions do not run on this box: nothing to compare with
                    case["torch_functional_error"] = str(e).splitlines()[0][:200]
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
