"""What evaluating the UNet at round(t) costs under "linspace" timestep spacing (Euler / Euler ancestral, sampler.EulerTables).

diffusers feeds the fractional timestep of the "linspace" spacing to the time embedding; here the sigmas are taken at the fractional
timestep and the UNet runs at the nearest integer one.  This measures, on the CPU oracle's TINY model (seeded synthetic weights, CFG
rows, a model input of the schedule's scale at that timestep), the relative distance of eps at the half-integers of the 7-step
schedule to eps at the two neighbouring integers - and, for scale, the distance between those two neighbours.  CPU only:
    python tools/euler_round_t.py
"""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from oracle import unet as ounet
    cfg = ounet.TINY
    W = ounet.init_weights(cfg)
    g = torch.Generator().manual_seed(41)
    S, h = 2, 16
    ehs = torch.randn(2 * S, 77, cfg.cross_attention_dim, generator=g).half().float()
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float32) ** 2
    acp = torch.cumprod(1.0 - betas, dim=0).double()
    rel = lambda a, b: float((a - b).double().norm() / b.double().norm())
    print("t_frac  |eps(lo) - eps(t)|/|eps(t)|  |eps(hi) - eps(t)|/|eps(t)|  |eps(hi) - eps(lo)|/|eps(lo)|   (round(t) is marked *)")
    worst = 0.0
    for t in (832.5, 499.5, 166.5):
        lo, hi = int(math.floor(t)), int(math.ceil(t))
        sig = 0.5 * (math.sqrt((1 - acp[lo]) / acp[lo]) + math.sqrt((1 - acp[hi]) / acp[hi]))
        x0, e = 0.18215 * 5.0 * torch.randn(S, 4, h, h, generator=g), torch.randn(S, 4, h, h, generator=g)
        xin = ((x0 + sig * e) / math.sqrt(sig * sig + 1.0)).float()
        with torch.no_grad():
            out = {tt: ounet.unet_forward(cfg, W, torch.cat([xin, xin]), tt, ehs)[0] for tt in (lo, t, hi)}
        r = round(t)                                           # half to even, as numpy rounds
        d_lo, d_hi = rel(out[lo], out[t]), rel(out[hi], out[t])
        worst = max(worst, d_lo if r == lo else d_hi)
        print(f"{t:6.1f}  {d_lo:.3e}{'*' if r == lo else ' '}                  {d_hi:.3e}{'*' if r == hi else ' '}"
              f"                  {rel(out[hi], out[lo]):.3e}")
    print(f"largest relative distance of eps(round(t)) to eps(t): {worst:.3e}")


if __name__ == "__main__":
    main()
