#!/usr/bin/env python3
"""Bit fingerprints of the sampling loop: one line per case with the sha256 of the final latents and of the concatenated
last_aux, each case run eager and from captured hipGraphs.  TINY UNet, latents [2, 4, 8, 8], T = 4, fixed seeds, synthetic
weights.  Two commits compute the same trajectories iff their outputs are equal line for line (it uses the public sampler
surface only, so the same file runs on either); eager and graphed lines of one case are equal too.

    python tools/sampler_parity.py > parity.txt
"""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sketch2img_amd import synthetic
from sketch2img_amd.config import TINY, tap_channels
from sketch2img_amd.controlnet import Control, ControlNetModel
from sketch2img_amd.lgp import HipLGP
from sketch2img_amd.sampler import DDIMTables, DPMTables, HipSampler
from sketch2img_amd.unet import HipUNet

DEV, S, H, T = "cuda:0", 2, 8, 4
SDE = "sde-dpmsolver++"


def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def main():
    net = HipUNet(TINY, synthetic.unet_state_dict(TINY), DEV)
    cnet = ControlNetModel.from_pretrained(None, unet_config=TINY).to(DEV).hip
    ehs = synthetic.text_embeddings(S, TINY.cross_attention_dim)
    sd_lgp = synthetic.lgp_state_dict(synthetic.lgp_input_dim(TINY))
    lat, target = rnd(S, 4, H, H, seed=1), 0.18215 * rnd(S, 4, H, H, seed=2)
    init, mask = 0.8 * rnd(S, 4, H, H, seed=3), (rnd(S, 1, H, H, seed=4) > 0).float()
    picture = torch.rand(1, 3, 8 * H, 8 * H, generator=torch.Generator().manual_seed(5)).to(DEV)
    ddim, dpm = DDIMTables.make(T), DPMTables.make(T)

    def control(start, end):
        return lambda: Control(cnet, cnet.hint_rows(cnet.embed(picture), 1, 2 * S), 0.8, start, end)

    # name -> (tables, guided by the LGP, sample() keywords, control factory or None)
    cases = {
        "ddim": (ddim, False, {}, None),
        "ddim eta 0.5": (ddim, False, dict(eta=0.5), None),
        "ddim no cfg": (ddim, False, dict(classifier_free=False), None),
        "ddim guided": (ddim, True, {}, None),
        "dpm 2m": (dpm, False, {}, None),
        "dpm 2m guided": (dpm, True, {}, None),
        "dpm karras": (DPMTables.make(T, use_karras_sigmas=True), False, {}, None),
        "dpm sde": (DPMTables.make(T, algorithm_type=SDE), False, {}, None),
        "img2img start 2": (ddim, False, dict(init_latents=init, start_step=2), None),
        "img2img mask": (ddim, False, dict(init_latents=init, start_step=1, mask=mask), None),
        "control full window": (ddim, False, {}, control(0.0, 1.0)),
        "control window 0.25-0.75": (ddim, False, {}, control(0.25, 0.75)),
    }
    for name, (tab, guided, kw, make_control) in cases.items():
        for graphs in (False, True):
            cf = kw.get("classifier_free", True)
            net.prepare_context(ehs if cf else ehs[S:])
            kw2 = dict(kw)
            if make_control is not None:
                cnet.prepare_context(ehs)
                kw2["control"] = make_control()
            lgp = HipLGP({k: v.clone() for k, v in sd_lgp.items()}, tap_channels(TINY), DEV) if guided else None
            sampler = HipSampler(net, lgp, use_graphs=graphs)
            out = sampler.sample(lat, target if guided else None, T, tables=tab, generator=torch.Generator().manual_seed(7), **kw2)
            aux = [a for a in sampler.last_aux if a is not None]
            torch.cuda.synchronize()
            print(f"{name:26s} {'graphed' if graphs else 'eager  '} latents {sha(out)} aux {sha(torch.cat(aux)) if aux else '-'}",
                  flush=True)


if __name__ == "__main__":
    main()
