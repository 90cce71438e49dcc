#!/usr/bin/env python3
"""Golden vectors of the sketch generator (checked by tests/test_host_anime2sketch.py and tests/test_gpu_anime2sketch.py) from
the reference's own module: loads <reference checkout>/anime2sketch/model.py BY PATH, builds UnetGenerator(3, 1, 8, 64,
InstanceNorm2d(affine=False, track_running_stats=False)) as its create_model() does, loads synthetic.anime2sketch_state_dict()
into it and runs it on synthetic.pictures() on the CPU in fp32.  No arithmetic of this package enters the vectors.

    python tools/gen_golden_anime2sketch.py <reference checkout>

Writes tests/golden/anime2sketch_256.npz, anime2sketch_256x512.npz (y, checksums), anime2sketch_1024_blocks.npz (16 x 16 block
means of y and of the binarised mask) and anime2sketch_meta.json (manifest, per-layer statistics, tolerances).

Tolerances are MEASURED here, without the code under test: the same module with every Conv2d / ConvTranspose2d /
InstanceNorm2d output rounded to fp16 (forward hooks) - the storage the engine uses.  meta["cases"][name] holds
max |y_emu - y_ref| and the relative L2 distance; the tests allow 2 x those.  The binarised mask is compared only where
|1 - y_ref - 0.5| >= band = 2 x the max-abs tolerance; the tool refuses to write a fixture in which more than 5 % of the pixels
fall inside the band."""
import functools
import importlib.util
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sketch2img_amd import synthetic  # noqa: E402  (seeded weight / picture recipe only)

GOLD = os.path.join(ROOT, "tests", "golden")
MAX_BYTES = 750_000
CASES = {"256": (0, 256, 256), "256x512": (1, 256, 512), "1024_blocks": (2, 1024, 1024)}      # name -> (picture index, H, W)
LAYERS = (nn.Conv2d, nn.ConvTranspose2d, nn.InstanceNorm2d)


def load_reference(ref_dir):
    spec = importlib.util.spec_from_file_location("_ref_anime2sketch_model", os.path.join(ref_dir, "anime2sketch", "model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    norm = functools.partial(nn.InstanceNorm2d, affine=False, track_running_stats=False)
    return mod.UnetGenerator(3, 1, 8, 64, norm_layer=norm, use_dropout=False).eval()


def checksums(tensors):
    return np.array([[float(t.double().sum()), float((t.double() ** 2).sum())] for t in tensors], dtype=np.float64)


def block_means(t, n=16):
    return torch.nn.functional.avg_pool2d(t.double(), n)[0, 0].numpy()


def mask_of(y):
    return ((1.0 - y) >= 0.5).float()


def main():
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "anime2sketch", "model.py")):
        sys.exit(__doc__)
    torch.manual_seed(0)
    net = load_reference(sys.argv[1])
    W = synthetic.anime2sketch_state_dict()
    net.load_state_dict(W)      # strict: the 32 keys and shapes must be the reference's
    manifest = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    meta = {"manifest": manifest, "parameters": int(sum(p.numel() for p in net.parameters())), "cases": {},
            "torch": torch.__version__, "weight_seed": synthetic.A2S_WEIGHT_SEED}
    wsum = checksums(W.values())

    for name, (idx, H, Wd) in CASES.items():
        x = synthetic.pictures(idx, 1, H, Wd)
        stats, hooks = [], []
        if name == "256":      # per-layer statistics of the 16 convolution outputs: where to look when the end-to-end test fails
            for n_, m in net.named_modules():
                if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
                    hooks.append(m.register_forward_hook(
                        lambda mod, i, o, n_=n_: stats.append([n_, float(o.mean()), float(o.std()), float(o.abs().max())])))
        with torch.no_grad():
            y = net(x.clone())
        for h in hooks:
            h.remove()
        hooks = [m.register_forward_hook(lambda mod, i, o: o.half().float()) for m in net.modules() if isinstance(m, LAYERS)]
        with torch.no_grad():
            y_emu = net(x.clone())
        for h in hooks:
            h.remove()
        max_abs = float((y_emu - y).abs().max())
        rel_l2 = float((y_emu - y).norm() / y.norm())
        band = 2 * (2 * max_abs)
        dist = ((1.0 - y) - 0.5).abs()
        share = float((dist < band).float().mean())
        flips = float(((mask_of(y_emu) != mask_of(y)) & (dist >= band)).float().mean())
        case = {"picture": idx, "H": H, "W": Wd, "emu_max_abs": max_abs, "emu_rel_l2": rel_l2, "band": band, "band_share": share,
                "emu_flips_off_band": flips, "y_mean": float(y.mean()), "y_std": float(y.std()), "ink_share": float(1 - mask_of(y).mean())}
        if share > 0.05:
            sys.exit(f"{name}: {share:.3f} of the pixels lie within +-{band:.2e} of the threshold (cap 0.05): no fixture written")
        path = os.path.join(GOLD, f"anime2sketch_{name}.npz")
        if name == "1024_blocks":
            yb, mb = block_means(y), block_means(mask_of(y))
            eyb, emb = block_means(y_emu), block_means(mask_of(y_emu))
            case.update(emu_y_blocks_max_abs=float(np.abs(eyb - yb).max()), emu_y_blocks_rel_l2=float(np.linalg.norm(eyb - yb) / np.linalg.norm(yb)),
                        emu_mask_blocks_max_abs=float(np.abs(emb - mb).max()),
                        emu_mask_blocks_rel_l2=float(np.linalg.norm(emb - mb) / np.linalg.norm(mb)))
            np.savez_compressed(path, y_blocks=yb.astype(np.float32), mask_blocks=mb.astype(np.float32), input_checksum=checksums([x]),
                                weight_checksums=wsum)
        else:
            np.savez_compressed(path, y=y.numpy(), input_checksum=checksums([x]), weight_checksums=wsum)
        if stats:
            meta["layers_256"] = stats
        assert os.path.getsize(path) <= MAX_BYTES, (path, os.path.getsize(path))
        meta["cases"][name] = case
        print(name, json.dumps(case))
    with open(os.path.join(GOLD, "anime2sketch_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
