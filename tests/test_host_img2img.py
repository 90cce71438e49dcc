"""CPU tests (-m "not gpu") of img2img and masked repaint: the skg_latent_renoise symbol and its argument checks, start_step and the
schedule levels, the hipGraph cache key, the pipeline's argument validation (before any device work) and the identities of the
CPU reference trajectory (tests/img2img_ref.py) that the GPU tests compare against.  No kernel is launched here."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_latent_renoise_symbol_is_declared_bound_and_exported():
    from sketch2img_amd import _lib
    src = open(os.path.join(ROOT, "include", "skg.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+skg_latent_renoise\s*\(([^;{]*?)\)\s*;", src, flags=re.S)
    assert m, "include/skg.h does not declare skg_latent_renoise"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    letters = "".join("p" if "*" in a else "f" if a.startswith("float") else "i" if a.startswith("int") else "?" for a in args)
    assert letters == "pppipiiffp"
    assert _lib.SIGNATURES["skg_latent_renoise"] == ("i", letters)
    assert _lib.ABI_VERSION == 6 and _lib.lib.skg_abi_version() == 6
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert "skg_latent_renoise" in set(re.findall(r" T (skg_\w+)", nm))


def test_latent_renoise_checks_its_arguments_without_a_gpu():
    """SKG_E_BADARG before any HIP call (the pointers are never dereferenced: 16 stands for 'not NULL')."""
    from sketch2img_amd import _lib
    f = _lib.lib.skg_latent_renoise
    args = lambda init=16, noise=16, mask=None, ms=0, x=16, samples=3, HW=4: (init, noise, mask, ms, x, samples, HW, 0.6, 0.8, None)
    assert f(*args(init=None)) == -1
    assert f(*args(noise=None)) == -1
    assert f(*args(x=None)) == -1
    assert f(*args(samples=0)) == -1
    assert f(*args(HW=0)) == -1
    assert f(*args(HW=-3)) == -1
    assert f(*args(mask=16, ms=2, samples=3)) == -1
    assert f(*args(mask=16, ms=0)) == -1


@pytest.mark.parametrize("T,strength,want", [(50, 0.8, 10), (50, 1.0, 0), (50, 0.5, 25), (3, 0.5, 2), (4, 0.75, 1), (4, 0.25, 3)])
def test_start_step(T, strength, want):
    from sketch2img_amd.sampler import start_step
    assert start_step(T, strength) == want


def test_start_step_refusals():
    from sketch2img_amd.sampler import start_step
    with pytest.raises(ValueError, match="no step"):
        start_step(10, 0.05)
    for bad in (-0.1, 1.1):
        with pytest.raises(ValueError, match=r"The value of strength should in \[0.0, 1.0\] but is"):
            start_step(50, bad)


@pytest.mark.parametrize("kind", ["ddim", "dpm", "dpm_karras"])
def test_levels(kind):
    from sketch2img_amd.sampler import DDIMTables, DPMTables
    T = 10
    tab = DDIMTables.make(T) if kind == "ddim" else DPMTables.make(T, use_karras_sigmas=kind == "dpm_karras")
    lv = [tab.level(j) for j in range(T + 1)]
    assert lv[T] == (1.0, 0.0)
    for j, (a, s) in enumerate(lv):
        assert isinstance(a, float) and isinstance(s, float)
        assert a == float(np.float32(a)) and s == float(np.float32(s)), "fp32 floats"
        if j < T:
            assert abs(a * a + s * s - 1.0) < 1e-6, (j, a, s)
    assert all(lv[j + 1][0] > lv[j][0] for j in range(T)), "a rises strictly along the schedule"
    if kind == "ddim":
        for j, t in enumerate(tab.timesteps.tolist()):
            acp = float(tab.alphas_cumprod[t])
            assert abs(lv[j][0] - acp ** 0.5) < 1e-7 and abs(lv[j][1] - (1 - acp) ** 0.5) < 1e-7
            assert lv[j] == tab.coeffs(t)[:2]                  # the floats the step kernel reads x at
    else:
        for j in range(T):
            al, sg, _ = tab.source(j)
            assert lv[j] == (float(np.float32(al)), float(np.float32(sg)))
            assert lv[j] == tab.coeffs(j, 1)[:2]
        if kind == "dpm":
            assert all(lv[j] == tab.source(j)[:2] for j in range(T))      # the uniform schedule's source is fp32 table values


def test_graph_key_start_and_mask():
    from sketch2img_amd.sampler import DDIMTables, DPMTables, graph_key
    base = dict(shape=(2, 4, 16, 16), unguided=True, guidance_scale=7.5, beta=1.6, share_cfg_prefix=True)
    for tab in (DDIMTables.make(4), DPMTables.make(4, algorithm_type="sde-dpmsolver++")):
        k0 = graph_key(tab, **base)
        assert k0 == graph_key(tab, **base, start_step=0, masked=False)
        assert graph_key(tab, **base, eta=0.0, classifier_free=True) == graph_key(tab, **base, eta=0.0, classifier_free=True,
                                                                                 start_step=0, masked=False) == k0
        assert graph_key(tab, **base, start_step=1) != k0
        assert graph_key(tab, **base, masked=True) != k0
        assert graph_key(tab, **base, start_step=1, masked=True) != graph_key(tab, **base, start_step=1)
        assert graph_key(tab, **base, start_step=1) != graph_key(tab, **base, start_step=2)
        hash(graph_key(tab, **base, start_step=1, masked=True))


@pytest.fixture(scope="module")
def cpu_pipe():
    """A TINY synthetic pipeline without a VAE that never leaves the CPU: touching its UNet engine raises RuntimeError."""
    from modules.pipeline import AntiGradientPipeline
    from sketch2img_amd.config import TINY
    return AntiGradientPipeline.from_pretrained(None, unet_config=TINY)


def test_pipeline_validates_img2img_arguments_before_any_device_work(cpu_pipe):
    """ValueError, not the RuntimeError of a UNet engine that is asked to run on the CPU."""
    from PIL import Image
    call = dict(height=64, width=64, num_inference_steps=4, output_type="latent")
    lat = torch.zeros(1, 4, 8, 8)
    with pytest.raises(ValueError, match="mask_image"):
        cpu_pipe("a", mask_image=torch.ones(1, 1, 64, 64), **call)
    with pytest.raises(ValueError, match="image"):
        cpu_pipe("a", image=torch.zeros(1, 3, 64, 32), **call)                    # pixels of the wrong size
    with pytest.raises(ValueError, match="image"):
        cpu_pipe("a", image=torch.zeros(1, 4, 8, 16), **call)                     # latents of the wrong size
    with pytest.raises(ValueError, match="resize"):
        cpu_pipe("a", image=Image.new("RGB", (32, 64)), **call)                   # PIL: (width, height) = (32, 64)
    with pytest.raises(ValueError, match="VAE"):
        cpu_pipe("a", image=torch.zeros(1, 3, 64, 64), **call)                    # three channels, no VAE to encode them
    with pytest.raises(ValueError, match="VAE"):
        cpu_pipe("a", image=Image.new("RGB", (64, 64)), **call)
    with pytest.raises(ValueError, match=r"strength should in \[0.0, 1.0\]"):
        cpu_pipe("a", image=lat, strength=1.5, **call)
    with pytest.raises(ValueError, match="no step"):
        cpu_pipe("a", image=lat, strength=0.2, **call)                            # int(4 * 0.2) = 0 steps
    with pytest.raises(ValueError, match="mask_image"):
        cpu_pipe("a", image=lat, mask_image=torch.ones(1, 1, 32, 32), **call)     # neither the pixel nor the latent grid
    with pytest.raises(ValueError, match="image"):
        cpu_pipe(["a", "b", "c"], image=torch.zeros(2, 4, 8, 8), **call)          # batch neither 1 nor S
    # what is valid reaches the engine, which refuses the CPU
    for ok in (dict(image=lat), dict(image=lat, strength=1.0), dict(image=lat, mask_image=torch.ones(1, 1, 64, 64)),
               dict(image=lat, mask_image=Image.new("L", (64, 64), 255)), dict(image=lat, latents=torch.zeros(1, 4, 8, 8))):
        with pytest.raises(RuntimeError, match="GPU only"):
            cpu_pipe("a", **ok, **call)


def test_pixel_mask_is_reduced_by_the_block_mean(cpu_pipe):
    """8 x 8 block mean, soft; a latent cell is kept (0) exactly where all of its 64 pixels are 0."""
    from PIL import Image
    m = torch.zeros(1, 1, 64, 64)
    m[0, 0, :8, :8] = 1.0               # cell (0, 0): all ones
    m[0, 0, 8, 15] = 1.0                # cell (1, 1): one pixel of 64
    r = cpu_pipe._prepare_mask(m, 1, 64, 64)
    assert r.shape == (1, 1, 8, 8) and r.dtype == torch.float32
    assert float(r[0, 0, 0, 0]) == 1.0 and float(r[0, 0, 1, 1]) == 1.0 / 64
    keep = torch.ones(8, 8, dtype=torch.bool)
    keep[0, 0] = keep[1, 1] = False
    assert torch.equal(r[0, 0] == 0, keep)
    assert torch.equal(cpu_pipe._prepare_mask(r, 1, 64, 64), r)                   # latent resolution: as given
    pil = cpu_pipe._prepare_mask(Image.fromarray((m[0, 0] * 255).to(torch.uint8).numpy(), "L"), 1, 64, 64)
    assert torch.equal(pil, r)
    img = cpu_pipe._pil_to_tensor(Image.new("RGB", (64, 64), (255, 0, 51)), "RGB", 64, 64, "image")
    assert img.shape == (1, 3, 64, 64) and torch.equal(img[0, :, 0, 0], torch.tensor([1.0, 0.0, 51 / 255], dtype=torch.float32))


def test_sampler_validates_img2img_arguments_before_any_launch():
    from types import SimpleNamespace
    from sketch2img_amd.sampler import HipSampler
    s = HipSampler(SimpleNamespace(dev="cpu", inject=None), None)
    x = torch.zeros(2, 4, 8, 8)
    with pytest.raises(ValueError, match="init_latents"):
        s.sample(x, None, 4, mask=torch.ones(1, 1, 8, 8))
    with pytest.raises(ValueError, match="init_latents"):
        s.sample(x, None, 4, start_step=1)
    with pytest.raises(ValueError, match="start_step"):
        s.sample(x, None, 4, init_latents=x, start_step=4)
    with pytest.raises(ValueError, match="init_latents shape"):
        s.sample(x, None, 4, init_latents=torch.zeros(1, 4, 8, 8), start_step=1)
    with pytest.raises(ValueError, match="mask shape"):
        s.sample(x, None, 4, init_latents=x, start_step=1, mask=torch.ones(2, 4, 8, 8))


@pytest.mark.parametrize("scheduler", ["ddim", "dpm", "dpm_karras"])
def test_reference_identities(scheduler):
    """TINY, 8 x 8, T = 4, start 1, guided by a sketch target: a mask == 1 is the maskless trajectory exactly, a mask == 0 returns
    init exactly, and the maskless trajectory is neither init nor the trajectory with a half mask."""
    from oracle import lgp as olgp, unet as ounet
    from tests.img2img_ref import levels, trajectory
    cfg, h, T, k = ounet.TINY, 8, 4, 1
    g = torch.Generator().manual_seed(5)
    W = ounet.init_weights(cfg)
    sd = olgp.init_state_dict(sum(ounet.tap_channels(cfg)) + 40)
    ehs = torch.randn(2, 77, cfg.cross_attention_dim, generator=g).half().float()
    init, eps = 0.5 * torch.randn(1, 4, h, h, generator=g), torch.randn(1, 4, h, h, generator=g)
    target = 0.18215 * torch.randn(1, 4, h, h, generator=g)
    run = lambda mask: trajectory(cfg, W, ehs, init, eps, T, k, scheduler, mask=mask, lgp_sd=sd, target=target)
    plain = run(None)
    assert torch.isfinite(plain).all() and not torch.equal(plain, init)
    assert torch.equal(run(torch.ones(1, 1, h, h)), plain)
    assert torch.equal(run(torch.zeros(1, 1, h, h)), init)
    half = torch.ones(1, 1, h, h)
    half[..., : h // 2] = 0.0
    out = run(half)
    assert torch.equal(out[..., : h // 2], init[..., : h // 2]) and not torch.equal(out[..., h // 2:], plain[..., h // 2:])
    lv = levels(scheduler, T)
    assert lv[T] == (1.0, 0.0) and all(abs(a * a + s * s - 1) < 1e-6 for a, s in lv[:T])
