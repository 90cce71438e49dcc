#!/usr/bin/env python3
"""ControlNet timing (not a gate): SD1.5 synthetic weights, 64 x 64 latents (512 x 512 px control picture).

    python tools/controlnet_bench.py [--txt profiles/controlnet.txt] [--h 64] [--samples 1,8] [--steps 10] [--windows 3]

1. Step time, controlled against uncontrolled, for S = 1 and S = 8, eager and hipGraph replay: DDIM, guidance_scale 7.5, all
   steps inside the control's window.  Per configuration `windows` alternating windows (uncontrolled, controlled, ...) of one
   `steps`-step trajectory each after a warm-up trajectory per mode; ms per step = the median window / steps, with the min ... max
   spread.  A window is device events around work that ends in a synchronise.  The uncontrolled launches are the parent commit's
   (pinned bit for bit by the suite), so "uncontrolled" is the parent's step on the same box in the same process.
2. The hint encoder, once per call: the whole of it, and its three pixel-resolution layers through skg_conv3x3_small_f16 against
   the route it replaces - the picture zero-padded to 32 channels (skg_nchw_f32_to_nhwc_f16), the implicit GEMM with Cin = 32 and
   skg_silu_f16 - 200 back-to-back calls per window, three alternating windows, the median.

Prints text lines and appends them to --txt."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sketch2img_amd import ops, synthetic  # noqa: E402
from sketch2img_amd.config import SD15  # noqa: E402
from sketch2img_amd.controlnet import Control, ControlNetModel  # noqa: E402
from sketch2img_amd.packs import pack_conv  # noqa: E402
from sketch2img_amd.sampler import DDIMTables, HipSampler  # noqa: E402
from sketch2img_amd.unet import HipUNet  # noqa: E402

DEV = "cuda:0"


def window(fn, iters=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def alternate(fns, windows, iters=1):
    """{name: [ms per call, one per window]} with the candidates alternating inside every round."""
    for fn in fns.values():      # warm-up: every shape of the timed windows
        fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            out[k].append(window(fn, iters))
    return out


def fmt(v):
    return f"{statistics.median(v):8.3f} ms ({min(v):.3f} ... {max(v):.3f})"


def step_times(net, cnet, h, S, steps, windows, say):
    g = torch.Generator().manual_seed(S)
    ehs = torch.randn(2 * S, 77, SD15.cross_attention_dim, generator=g).half().float()
    net.prepare_context(ehs)
    cnet.prepare_context(ehs)
    lat = torch.randn(S, 4, h, h, generator=g).to(DEV)
    img = torch.rand(1, 3, 8 * h, 8 * h, generator=g).to(DEV)
    control = Control(cnet, cnet.hint_rows(cnet.embed(img), 1, 2 * S), 1.0)
    tab = DDIMTables.make(steps)
    for graphs in (False, True):
        sampler = HipSampler(net, use_graphs=graphs)
        t = alternate({"uncontrolled": lambda: sampler.sample(lat, None, tables=tab),
                       "controlled": lambda: sampler.sample(lat, None, tables=tab, control=control)}, windows)
        u, c = [v / steps for v in t["uncontrolled"]], [v / steps for v in t["controlled"]]
        say(f"step S={S} {'graph' if graphs else 'eager'}: uncontrolled {fmt(u)}  controlled {fmt(c)}  "
            f"ratio {statistics.median(c) / statistics.median(u):.3f}")
        del sampler
        torch.cuda.empty_cache()


def encoder_times(cnet, h, windows, say):
    B, H = 1, 8 * h
    img = torch.rand(B, 3, H, H, generator=torch.Generator().manual_seed(1)).to(DEV)
    say(f"hint encoder, {H} x {H} px, whole (8 layers): {fmt(alternate({'e': lambda: cnet.embed(img)}, windows, 50)['e'])}")
    sd = synthetic.controlnet_state_dict(SD15)
    e = "controlnet_cond_embedding"
    names = ["conv_in", "blocks.0", "blocks.1"]
    small = cnet.embed_layers[:3]
    padded = []
    for n in names:      # the route replaced: input channels zero-padded to 32 for the implicit GEMM
        w = sd[f"{e}.{n}.weight"]
        padded.append((pack_conv(w, DEV, cin_pad=32), sd[f"{e}.{n}.bias"].half().to(DEV)))

    def run_small():
        x, s = img, H
        for wp, b, stride, _ in small:
            x = ops.conv3x3_small(x, wp, B, s, s, stride, bias=b, silu=True)
            s //= stride
        return x

    def run_padded():
        x, s = ops.nchw_to_nhwc(img, 32), H
        for li, (wp, b) in enumerate(padded):
            co = wp.shape[0]
            # (the next layer reads 32 channels: a 16-channel output goes into the left half of a zeroed 32-column buffer)
            y = torch.zeros(B * (s // (2 if li == 2 else 1)) ** 2, 32, device=DEV, dtype=torch.float16) if co < 32 else None
            o = ops.conv3x3(x, wp, B, s, s, ops.CONV_S2 if li == 2 else ops.CONV_S1, out=None if y is None else y[:, :co], bias=b)
            ops.silu(o, out=o)
            x = o if y is None else y
            s //= 2 if li == 2 else 1
        return x

    a, b = run_small().float(), run_padded().float()
    say(f"three pixel-resolution layers: small-channel vs padded route, outputs rel {float((a - b).norm() / b.norm()):.2e}")
    t = alternate({"small": run_small, "padded": run_padded}, windows, 200)
    say(f"three pixel-resolution layers, {H} x {H} px: small-channel {fmt(t['small'])}  padded implicit GEMM {fmt(t['padded'])}  "
        f"ratio {statistics.median(t['small']) / statistics.median(t['padded']):.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--txt", default=None)
    ap.add_argument("--h", type=int, default=64)
    ap.add_argument("--samples", default="1,8")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("controlnet_bench.py measures on the GPU: no device found")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    net = HipUNet(SD15, synthetic.unet_state_dict(SD15), DEV, need_backward=False)
    cnet = ControlNetModel.from_pretrained(None).to(DEV).hip
    say(f"# tools/controlnet_bench.py --h {args.h} --samples {args.samples} --steps {args.steps} --windows {args.windows}: "
        f"SD1.5 synthetic, {args.h} x {args.h} latents, DDIM, guidance_scale 7.5, {torch.cuda.get_device_name(0)}")
    encoder_times(cnet, args.h, args.windows, say)
    for S in (int(s) for s in args.samples.split(",")):
        step_times(net, cnet, args.h, S, args.steps, args.windows, say)
    if args.txt:
        with open(args.txt, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
