#!/usr/bin/env python3
"""CLIP vision tower training step timing (not a gate): ViT-L/14 synthetic weights, batch 4.

    python tools/clip_train_bench.py [--out profiles/clip_train_bench.json] [--batch 4] [--iters 3] [--no-sat]

Reports ms per step split into forward_train / backward / optimizer (AdamW + the refresh of the derived packs, which the next
forward would otherwise pay) - device events around work that ends in a synchronise, after a warm-up step - and, inside it, the
time spent in ops.wgrad, in ops.transpose and in ops.colsum (the embedding fold: skg_colsum_f16's worst shape, B rows by Lp * D
columns) - event pairs around every call, summed.  Next to it the SatMixin step of
tools/sat_train_bench.py (SD1.5 synthetic weights, 64 x 64 latents, the same batch) on the same box: the step the tower's joins."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sketch2img_amd import ops, sat_train, synthetic  # noqa: E402
from sketch2img_amd.clip_vision_train import HipClipTowerTrainer  # noqa: E402
from sketch2img_amd.config import SD15, VIT_L_14  # noqa: E402

ev = lambda: torch.cuda.Event(enable_timing=True)


class Timed:
    """Wraps ops.<name> with an event pair per call."""

    def __init__(self, name):
        self.name, self.orig, self.pairs = name, getattr(ops, name), []

    def __enter__(self):
        def wrapped(*a, **kw):
            e0, e1 = ev(), ev()
            e0.record()
            r = self.orig(*a, **kw)
            e1.record()
            self.pairs.append((e0, e1))
            return r
        setattr(ops, self.name, wrapped)
        return self

    def __exit__(self, *exc):
        setattr(ops, self.name, self.orig)

    def take_ms(self):
        t = sum(a.elapsed_time(b) for a, b in self.pairs)
        self.pairs = []
        return t


def sat_step_ms(dev, B, iters):
    from sketch2img_amd.sampler import DDIMTables
    from sketch2img_amd.unet import HipUNet
    cfg, h = SD15, 64
    net = HipUNet(cfg, synthetic.unet_state_dict(cfg), dev)
    tr = sat_train.HipSatTrainer(cfg, synthetic.satmixin_state_dict(cfg, "clip"), dev, warmup_steps=0)
    lat, noise = synthetic.initial_latents(0, B, h), synthetic.initial_latents(100, B, h)
    ehs = synthetic.text_embeddings(B, cfg.cross_attention_dim)[B:]
    state = synthetic.sketch_state(0, B)[B:]
    acp = DDIMTables.make(50).alphas_cumprod
    ts = [(37 + 251 * i) % 1000 for i in range(B)]
    out = []
    for it in range(iters + 1):
        a, b = ev(), ev()
        a.record()
        sat_train.train_step(tr, net, lat, ehs, state, ts, noise, acp)
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return sum(out[1:]) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--no-sat", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg, B = VIT_L_14, args.batch
    tw = HipClipTowerTrainer(cfg, synthetic.clip_vision_state_dict(cfg), dev, warmup_steps=0)
    g = torch.Generator().manual_seed(0)
    px = torch.randn(B, 3, cfg.image_size, cfg.image_size, generator=g)
    dtok = (1e-2 * torch.randn(B, cfg.num_tokens, cfg.hidden_size, generator=g)).half().to(dev)
    rows = []
    with Timed("wgrad") as tw_wgrad, Timed("transpose") as tw_tr, Timed("colsum") as tw_fold:
        for it in range(args.iters + 1):             # iteration 0 is the warm-up (it also builds the packs)
            e = [ev() for _ in range(4)]
            e[0].record()
            tok, kept = tw.forward_train(px)
            e[1].record()
            gt = tw.new_grad()
            tw.backward(kept, dtok, gt)
            e[2].record()
            stepped = tw.step(gt)
            tw.refresh()
            e[3].record()
            torch.cuda.synchronize()
            rows.append(dict(stepped=bool(stepped), forward_ms=e[0].elapsed_time(e[1]), backward_ms=e[1].elapsed_time(e[2]),
                             optimizer_ms=e[2].elapsed_time(e[3]), step_ms=e[0].elapsed_time(e[3]), wgrad_ms=tw_wgrad.take_ms(),
                             transpose_ms=tw_tr.take_ms(), fold_ms=tw_fold.take_ms()))
            del kept
            print(json.dumps(rows[-1]), flush=True)
    steady = rows[1:]
    mean = {k: sum(r[k] for r in steady) / len(steady) for k in steady[0] if k.endswith("_ms")}
    for k in ("wgrad", "transpose", "fold"):
        mean[k + "_share"] = mean[k + "_ms"] / mean["step_ms"]
    res = {"device": torch.cuda.get_device_name(0), "model": "ViT-L/14", "batch": B, "parameters": tw.n, "steps": rows, "mean_ms": mean}
    if not args.no_sat:
        res["sat_step_ms"] = sat_step_ms(dev, B, 2)
    print(json.dumps({k: v for k, v in res.items() if k != "steps"}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
