"""CPU tests (-m "not gpu") of the sampler options of the reference call: DDIM's eta > 0 coefficients against a float64
restatement, the order in which the initial latents and the per-step noise are drawn from one generator or a list of them,
the pipeline's argument validation (before any device work) and the hipGraph cache key.  No kernel is launched here."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch


def _eta_ref(tab, t, eta):
    """diffusers DDIMScheduler._get_variance / step in float64, from the same fp32 table entries -> (c_dir, sigma)."""
    prev = t - tab.ratio
    a_t = float(tab.alphas_cumprod[t])
    a_p = float(tab.alphas_cumprod[prev]) if prev >= 0 else float(np.float32(tab.final_alpha_cumprod))
    variance = ((1.0 - a_p) / (1.0 - a_t)) * (1.0 - a_t / a_p)
    sigma = eta * math.sqrt(variance)
    return math.sqrt(1.0 - a_p - sigma * sigma), sigma


@pytest.mark.parametrize("steps", [50, 25, 3])
@pytest.mark.parametrize("eta", [0.3, 1.0])
def test_coeffs_eta_vs_float64(steps, eta):
    """Bound 2e-4 relative on sigma and c_dir: 1 - a_t / a_prev loses about 10 bits at the last step (2^-24 * 2^10 = 6e-5), x 3."""
    from sketch2img_amd.sampler import DDIMTables
    tab = DDIMTables.make(steps)
    worst = [0.0, 0.0]
    for t in tab.timesteps.tolist():
        c = tab.coeffs_eta(t, eta)
        assert len(c) == 5 and all(isinstance(v, float) for v in c)
        assert c[:3] == tab.coeffs(t)[:3]
        c_dir, sigma = _eta_ref(tab, t, eta)
        assert sigma > 0 and c_dir > 0
        worst = [max(worst[0], abs(c[4] - sigma) / sigma), max(worst[1], abs(c[3] - c_dir) / c_dir)]
    print(f"[parity] coeffs_eta {steps} steps eta {eta}: worst rel sigma {worst[0]:.3e} c_dir {worst[1]:.3e}")
    assert worst[0] < 2e-4 and worst[1] < 2e-4


def test_coeffs_eta_zero_and_range():
    from sketch2img_amd.sampler import DDIMTables
    tab = DDIMTables.make(50)
    for t in tab.timesteps.tolist():
        assert tab.coeffs_eta(t, 0.0) == tab.coeffs(t) + (0.0,)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            tab.coeffs_eta(501, bad)


@pytest.fixture(scope="module")
def cpu_pipe():
    """A TINY synthetic pipeline that never leaves the CPU: touching its UNet engine raises RuntimeError."""
    from modules.pipeline import AntiGradientPipeline
    from sketch2img_amd.config import TINY
    return AntiGradientPipeline.from_pretrained(None, unet_config=TINY)


def test_draw_order_single_generator(cpu_pipe):
    """The initial latents first, then one [S, 4, h, w] draw per step."""
    from sketch2img_amd.sampler import draw_noise
    S, h, w, T, k = 3, 8, 16, 4, 1234
    g = torch.Generator().manual_seed(k)
    lat = cpu_pipe.prepare_latents(S, 4, 8 * h, 8 * w, torch.float32, "cpu", g)
    zs = [draw_noise(lat.shape, g, "cpu") for _ in range(T)]
    r = torch.Generator().manual_seed(k)
    assert torch.equal(lat, torch.randn((S, 4, h, w), generator=r))
    for z in zs:
        assert z.dtype == torch.float32 and z.is_contiguous()
        assert torch.equal(z, torch.randn((S, 4, h, w), generator=r))
    assert torch.equal(g.get_state(), r.get_state())
    # None: the default generator of the device, for the latents (as before) and for the step noise alike
    torch.manual_seed(9)
    lat = cpu_pipe.prepare_latents(2, 4, 64, 64, torch.float32, "cpu", None)
    z = draw_noise(lat.shape, None, "cpu")
    torch.manual_seed(9)
    assert torch.equal(lat, torch.randn((2, 4, 8, 8), dtype=torch.float32))
    assert torch.equal(z, torch.randn((2, 4, 8, 8), dtype=torch.float32))


def test_draw_order_generator_list(cpu_pipe):
    """Sample s of the latents and of every step's noise is a [1, 4, h, w] draw from generator[s]; a list no longer falls back to
    the unseeded default generator; a list of the wrong length is a ValueError."""
    from sketch2img_amd.sampler import check_generators, draw_noise
    S, h, w, T, k = 3, 8, 8, 3, 77
    seeded = lambda: [torch.Generator().manual_seed(k + s) for s in range(S)]
    gs = seeded()
    lat = cpu_pipe.prepare_latents(S, 4, 8 * h, 8 * w, torch.float32, "cpu", gs)
    zs = [draw_noise(lat.shape, gs, "cpu") for _ in range(T)]
    rs = seeded()
    assert lat.shape == (S, 4, h, w)
    assert torch.equal(lat, torch.cat([torch.randn((1, 4, h, w), generator=r) for r in rs]))
    for z in zs:
        assert torch.equal(z, torch.cat([torch.randn((1, 4, h, w), generator=r) for r in rs]))
    assert torch.equal(lat, cpu_pipe.prepare_latents(S, 4, 8 * h, 8 * w, torch.float32, "cpu", seeded()))
    assert torch.equal(lat, cpu_pipe.prepare_latents(S, 4, 8 * h, 8 * w, torch.float32, "cpu", tuple(seeded())))
    for short in (seeded()[:2], seeded() + seeded()[:1]):
        with pytest.raises(ValueError, match="list of generators of length"):
            cpu_pipe.prepare_latents(S, 4, 8 * h, 8 * w, torch.float32, "cpu", short)
        with pytest.raises(ValueError):
            draw_noise((S, 4, h, w), short, "cpu")
        with pytest.raises(ValueError):
            check_generators(short, S)
    check_generators(None, S)
    check_generators(torch.Generator(), S)


def test_pipeline_validates_before_any_device_work(cpu_pipe):
    """ValueError, not the RuntimeError of a UNet engine that is asked to run on the CPU."""
    call = dict(height=256, width=256, num_inference_steps=2, output_type="latent")
    with pytest.raises(ValueError, match="eta"):
        cpu_pipe("a", eta=2, **call)
    with pytest.raises(ValueError, match="eta"):
        cpu_pipe("a", eta=-0.5, **call)
    with pytest.raises(ValueError, match="sketch_image"):
        cpu_pipe("a", guidance_scale=1.0, sketch_image=torch.zeros(1, 4, 32, 32), **call)
    with pytest.raises(ValueError, match="list of generators of length"):
        cpu_pipe(["a", "b", "c"], generator=[torch.Generator().manual_seed(s) for s in range(2)], **call)
    with pytest.raises(ValueError, match="list of generators of length"):
        cpu_pipe("a", num_images_per_prompt=2, eta=0.5, generator=[torch.Generator()], **call)
    with pytest.raises(ValueError, match="Unexpected latents shape"):
        cpu_pipe("a", eta=0.5, latents=torch.zeros(1, 4, 32, 16), **call)
    # the lifted refusals: what is valid reaches the engine (which refuses the CPU), it is not stopped as unimplemented
    for ok in (dict(eta=0.5), dict(guidance_scale=1.0), dict(guidance_scale=0.0, negative_prompt="x"),
               dict(generator=[torch.Generator().manual_seed(1)])):
        with pytest.raises(RuntimeError, match="GPU only"):
            cpu_pipe("a", **ok, **call)


def test_sampler_validates_before_any_launch():
    from sketch2img_amd.sampler import HipSampler
    s = HipSampler(SimpleNamespace(dev="cpu", inject=None), None)
    x = torch.zeros(2, 4, 8, 8)
    with pytest.raises(ValueError, match="eta"):
        s.sample(x, None, 2, eta=1.5)
    with pytest.raises(ValueError, match="classifier_free"):
        s.sample(x, torch.zeros(2, 4, 8, 8), 2, classifier_free=False)
    with pytest.raises(ValueError, match="list of generators of length"):
        s.sample(x, None, 2, eta=0.5, generator=[torch.Generator()])


def test_graph_key_separates_eta_and_cfg():
    from sketch2img_amd.sampler import DDIMTables, DPMTables, graph_key
    tab = DDIMTables.make(4)
    base = dict(shape=(2, 4, 16, 16), unguided=True, guidance_scale=7.5, beta=1.6, share_cfg_prefix=True)
    k0 = graph_key(tab, **base)
    assert k0 == graph_key(DDIMTables.make(4), **base, eta=0.0, classifier_free=True)
    assert hash(k0) == hash(graph_key(tab, **base))
    assert graph_key(tab, **base, eta=0.5) != k0
    assert graph_key(tab, **base, eta=0.5) != graph_key(tab, **base, eta=0.25)
    assert graph_key(tab, **base, classifier_free=False) != k0
    assert graph_key(tab, **base, eta=0.5, classifier_free=False) != graph_key(tab, **base, eta=0.5)
    assert graph_key(DPMTables.make(4), **base) != k0


def test_eta_entry_point_checks_its_arguments_without_a_gpu():
    """skg_cfg_ddim_eta_step: skg_cfg_ddim_step's preconditions plus z != NULL, all refused before any HIP call."""
    from sketch2img_amd import _lib
    f = _lib.lib.skg_cfg_ddim_eta_step
    args = lambda z=16, ld=8, lo_off=0, vpred=0: (16, 16, ld, lo_off, 16, z, 16, None, 1, 4, 7.5, 0.1, 0.9, 0.2, 0.8, 0.1, vpred, None)
    assert f(*args(z=None)) == -1
    assert f(*args(ld=3)) == -1
    assert f(*args(ld=8, lo_off=8)) == -1        # the lo part needs ld >= lo_off + 4
    assert f(*args(vpred=2)) == -1
    assert _lib.SIGNATURES["skg_cfg_ddim_eta_step"] == ("i", "ppiippppiiffffffip") and _lib.ABI_VERSION == 6
