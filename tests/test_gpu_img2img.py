"""GPU tests (-m gpu) of img2img and masked repaint: skg_latent_renoise against float64 and its bit-exact identities, the sampler's
start index and blend against a hand-written loop of HipSampler.step, the pipeline against the CPU reference trajectory of
tests/img2img_ref.py, the VAE path with its draw order, and hipGraph replay."""
import numpy as np
import pytest
import torch

from tests.util import report

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SDE = "sde-dpmsolver++"


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def soft_mask(B, h, w, seed):
    """Uniform in [0, 1] with an exactly kept (0) top band and an exactly repainted (1) bottom band."""
    m = torch.rand(B, 1, h, w, generator=torch.Generator().manual_seed(seed))
    m[:, :, : max(1, h // 4)] = 0.0
    m[:, :, h - max(1, h // 4):] = 1.0
    return m


# ---------------------------------------------------------------------------------------------------- the kernel
KERNEL_SHAPES = [(1, (9, 9), None), (3, (16, 16), 1), (3, (32, 32), 3), (2, (8, 16), 2)]      # HW = 81, 256, 1024, 128


@pytest.mark.parametrize("S,hw,MS", KERNEL_SHAPES)
def test_latent_renoise_vs_float64(S, hw, MS):
    """a = 0.6, s = 0.8 (their fp32 values).  Element-wise bound 4 * 2^-24 * (|a init| + |s noise| + |x|): three fp32 roundings on
    the way to any output element, one spare.  Without a mask x is not read and its term is left out of the bound."""
    from sketch2img_amd import ops
    h, w = hw
    a, s = float(np.float32(0.6)), float(np.float32(0.8))
    init, noise, x0 = rnd(S, 4, h, w, seed=1), rnd(S, 4, h, w, seed=2), rnd(S, 4, h, w, seed=3)
    r64 = a * init.double() + s * noise.double()
    mag = (a * init.double()).abs() + (s * noise.double()).abs()
    if MS is None:
        got = ops.latent_renoise(init.to(DEV), noise.to(DEV), 0.6, 0.8)
        ref, bound = r64, 4 * 2.0 ** -24 * mag
        x = x0.to(DEV)                                  # a given x is written, not blended
        assert ops.latent_renoise(init.to(DEV), noise.to(DEV), 0.6, 0.8, x=x) is x and torch.equal(x, got)
    else:
        m = soft_mask(MS, h, w, seed=4)
        x = x0.to(DEV)
        got = ops.latent_renoise(init.to(DEV), noise.to(DEV), 0.6, 0.8, x=x, mask=m.to(DEV))
        assert got is x
        ref = m.double() * x0.double() + (1.0 - m.double()) * r64
        bound = 4 * 2.0 ** -24 * (mag + x0.double().abs())
    err = (got.cpu().double() - ref).abs()
    worst = float((err / bound).max())
    print(f"[parity] latent_renoise S={S} HW={h * w} mask_samples={MS}: max err {float(err.max()):.3e}, worst err/bound {worst:.3f}")
    assert got.shape == (S, 4, h, w) and bool((err <= bound).all())


@pytest.mark.parametrize("S,hw,MS", KERNEL_SHAPES)
def test_latent_renoise_identities_are_bit_exact(S, hw, MS):
    from sketch2img_amd import ops
    h, w = hw
    init, noise, x0 = rnd(S, 4, h, w, seed=5).to(DEV), rnd(S, 4, h, w, seed=6).to(DEV), rnd(S, 4, h, w, seed=7).to(DEV)
    plain = ops.latent_renoise(init, noise, 0.6, 0.8)
    assert torch.equal(ops.latent_renoise(init, noise, 1.0, 0.0), init)                     # (a, s) = (1, 0): init
    B = MS or 1
    ones, zeros = torch.ones(B, 1, h, w, device=DEV), torch.zeros(B, 1, h, w, device=DEV)
    x = x0.clone()
    ops.latent_renoise(init, noise, 0.6, 0.8, x=x, mask=ones)
    assert torch.equal(x, x0)                                                               # m = 1: x untouched
    ops.latent_renoise(init, noise, 0.6, 0.8, x=x, mask=zeros)
    assert torch.equal(x, plain)                                                            # m = 0: the NULL-mask output
    x = x0.clone()
    ops.latent_renoise(init, noise, 1.0, 0.0, x=x, mask=zeros)
    assert torch.equal(x, init)
    if MS == S and S > 1:
        # one mask per sample: changing the mask of sample 1 changes sample 1 alone
        m = soft_mask(S, h, w, seed=8).to(DEV)
        xa, xb = x0.clone(), x0.clone()
        ops.latent_renoise(init, noise, 0.6, 0.8, x=xa, mask=m)
        m2 = m.clone()
        m2[1] = 1.0 - m2[1]
        ops.latent_renoise(init, noise, 0.6, 0.8, x=xb, mask=m2)
        same = [torch.equal(xa[i], xb[i]) for i in range(S)]
        assert same == [i != 1 for i in range(S)]
    if MS == 1 and S > 1:
        # one mask for all: the same as that mask repeated per sample
        m = soft_mask(1, h, w, seed=9).to(DEV)
        xa, xb = x0.clone(), x0.clone()
        ops.latent_renoise(init, noise, 0.6, 0.8, x=xa, mask=m)
        ops.latent_renoise(init, noise, 0.6, 0.8, x=xb, mask=m.expand(S, -1, -1, -1).contiguous())
        assert torch.equal(xa, xb)


def test_latent_renoise_refusals():
    from sketch2img_amd import ops
    from sketch2img_amd._lib import SkgError
    init, noise = rnd(3, 4, 4, 4, seed=1).to(DEV), rnd(3, 4, 4, 4, seed=2).to(DEV)
    with pytest.raises(SkgError) as ei:
        ops.latent_renoise(init, noise, 0.6, 0.8, x=init.clone(), mask=torch.ones(2, 1, 4, 4, device=DEV))
    assert ei.value.rc == -1
    with pytest.raises(AssertionError):
        ops.latent_renoise(init, noise, 0.6, 0.8, mask=torch.ones(1, 1, 4, 4, device=DEV))       # a blend needs its x
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- the sampler
@pytest.fixture(scope="module")
def tiny():
    from oracle import lgp as olgp, unet as ounet
    from sketch2img_amd.config import TINY
    from sketch2img_amd.lgp import HipLGP
    from sketch2img_amd.unet import HipUNet
    W = ounet.init_weights(ounet.TINY)
    S = 2
    net = HipUNet(TINY, W, DEV)
    net.prepare_context(torch.randn(2 * S, 77, ounet.TINY.cross_attention_dim, generator=torch.Generator().manual_seed(41)).half().float())
    sd = olgp.init_state_dict(sum(ounet.tap_channels(ounet.TINY)) + 40, seed=12)
    return dict(net=net, S=S, lgp=HipLGP(sd, ounet.tap_channels(ounet.TINY), DEV))


def tables(kind, T):
    from sketch2img_amd.sampler import DDIMTables, DPMTables
    if kind == "ddim":
        return DDIMTables.make(T)
    return DPMTables.make(T, use_karras_sigmas=kind == "dpm_karras", algorithm_type=SDE if kind == "sde" else "dpmsolver++")


def case(S, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return dict(init=(0.8 * torch.randn(S, 4, h, w, generator=g)).to(DEV), eps=torch.randn(S, 4, h, w, generator=g).to(DEV),
                target=(0.18215 * torch.randn(S, 4, h, w, generator=g)).to(DEV))


def hand_loop(net, lgp, tab, c, k, target=None, noise="eps"):
    """The start by ops.latent_renoise, then HipSampler.step by hand for i = k .. T-1 on a fresh sampler."""
    from sketch2img_amd import ops
    from sketch2img_amd.sampler import HipSampler
    s = HipSampler(net, lgp)
    net.prepare_timesteps(tab.timesteps.tolist())
    s.reset_history()
    x = ops.latent_renoise(c["init"], c["eps"], *tab.level(k))
    nz = c["eps"] if noise == "eps" else x.clone()
    auxs = []
    for i in range(k, len(tab.timesteps)):
        x, _, aux = s.step(x, nz, target, tab, i, 7.5, 1.6)
        auxs.append(aux)
    return x, auxs


@pytest.mark.parametrize("kind", ["ddim", "dpm"])
@pytest.mark.parametrize("k,hw", [(1, (16, 16)), (3, (16, 16)), (1, (8, 16))])
def test_sampler_start_step_is_the_hand_loop_bit_for_bit(tiny, kind, k, hw):
    from sketch2img_amd.sampler import HipSampler
    T, S = 4, tiny["S"]
    tab, c = tables(kind, T), case(S, *hw, seed=50 + k)
    want, _ = hand_loop(tiny["net"], None, tab, c, k)
    seen = []
    s = HipSampler(tiny["net"], None)
    got = s.sample(c["eps"], None, T, tables=tab, init_latents=c["init"], start_step=k)
    assert torch.isfinite(got).all() and torch.equal(got, want)
    assert len(s.last_aux) == T - k and all(a is None for a in s.last_aux)
    again = s.sample(c["eps"], None, T, tables=tab, init_latents=c["init"], start_step=k, callback=lambda i, t, x: seen.append((i, t)))
    assert torch.equal(again, want)
    assert seen == [(n, int(tab.timesteps[k + n])) for n in range(T - k)]           # i counts the executed steps from 0
    full = s.sample(c["eps"], None, T, tables=tab)
    assert not torch.equal(full, got)


@pytest.mark.parametrize("kind", ["ddim", "dpm"])
def test_sampler_start_step_with_lgp_reads_eps(tiny, kind):
    """With an LGP and a sketch target: T - k aux entries; at k = 1 the steps i = 1, 2 (i <= T / 2) are guided, at k = 3 none is;
    the guided result is the hand loop with noise = eps bit for bit and is not the hand loop with noise = x_k."""
    from sketch2img_amd.sampler import HipSampler
    T, S = 4, tiny["S"]
    tab, c = tables(kind, T), case(S, 16, 16, seed=60)
    s = HipSampler(tiny["net"], tiny["lgp"])
    got = s.sample(c["eps"], c["target"], T, tables=tab, init_latents=c["init"], start_step=1)
    assert len(s.last_aux) == T - 1 and [a is not None for a in s.last_aux] == [True, True, False]
    want, auxs = hand_loop(tiny["net"], tiny["lgp"], tab, c, 1, target=c["target"])
    assert torch.isfinite(got).all() and torch.equal(got, want)
    assert all(torch.equal(a, b) for a, b in zip(s.last_aux[:2], auxs[:2]))
    other, _ = hand_loop(tiny["net"], tiny["lgp"], tab, c, 1, target=c["target"], noise="x_k")
    d = float((other - got).norm() / got.norm())
    print(f"[parity] {kind}: guidance noise eps vs x_k: relative distance of the results {d:.3e}")
    assert not torch.equal(other, got)
    unguided, _ = hand_loop(tiny["net"], None, tab, c, 1)
    assert not torch.equal(unguided, got)
    late = s.sample(c["eps"], c["target"], T, tables=tab, init_latents=c["init"], start_step=3)
    assert s.last_aux == [None]
    assert torch.equal(late, hand_loop(tiny["net"], None, tab, c, 3)[0])


@pytest.mark.parametrize("kind", ["ddim", "dpm", "dpm_karras"])
def test_sampler_mask_identities(tiny, kind):
    from sketch2img_amd.sampler import HipSampler
    T, S, h, k = 4, tiny["S"], 16, 1
    tab, c = tables(kind, T), case(S, h, h, seed=70)
    s = HipSampler(tiny["net"], None)
    run = lambda m: s.sample(c["eps"], None, T, tables=tab, init_latents=c["init"], start_step=k, mask=m)
    plain = run(None)
    assert torch.equal(run(torch.ones(1, 1, h, h)), plain)
    assert torch.equal(run(torch.ones(S, 1, h, h)), plain)
    assert torch.equal(run(torch.zeros(1, 1, h, h)), c["init"])
    half = torch.ones(1, 1, h, h)
    half[..., : h // 2] = 0.0                                    # the left half is kept
    out = run(half)
    assert torch.isfinite(out).all()
    assert torch.equal(out[..., : h // 2], c["init"][..., : h // 2])
    assert not torch.equal(out[..., h // 2:], c["init"][..., h // 2:])
    assert not torch.equal(out[..., h // 2:], plain[..., h // 2:])  # the repainted half saw the kept one through the UNet


# ---------------------------------------------------------------------------------------------------- the pipeline
@pytest.fixture(scope="module")
def pipe():
    from modules.pipeline import AntiGradientPipeline
    from sketch2img_amd.config import TINY
    return AntiGradientPipeline.from_pretrained(None, unet_config=TINY, torch_dtype=torch.float16).to("cuda")


def scheduler(kind):
    from sketch2img_amd.schedulers import DPMSolverMultistepScheduler
    if kind == "ddim":
        return None
    return DPMSolverMultistepScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", num_train_timesteps=1000,
                                       algorithm_type="dpmsolver++", solver_type="midpoint", lower_order_final=True,
                                       use_karras_sigmas=kind == "dpm_karras")


@pytest.mark.parametrize("kind", ["ddim", "dpm", "dpm_karras"])
def test_pipeline_img2img_with_soft_mask_vs_cpu_reference(pipe, kind):
    """S = 2 prompts, 32 x 32 latents, T = 5, strength 0.6 (start 2), guidance_scale 7.5, image given as latents, a soft mask at
    latent resolution.  Relative L2 < 1e-2 against tests/img2img_ref.py - the bound of the unguided pipeline-vs-oracle tests of this
    trajectory length (tests/test_gpu_sampler_options.py); the blend pulls both sides towards the same init and cannot loosen it.
    The txt2img call from latents = eps is more than 5e-2 away."""
    from oracle import unet as ounet
    from sketch2img_amd.sampler import start_step
    from tests.img2img_ref import trajectory
    h, T, prompts = 32, 5, ["a cat", "a dog on a hill"]
    S = len(prompts)
    assert start_step(T, 0.6) == 2
    init, eps, mask = 0.8 * rnd(S, 4, h, h, seed=80), rnd(S, 4, h, h, seed=81), soft_mask(1, h, h, seed=82)
    call = dict(height=8 * h, width=8 * h, num_inference_steps=T, guidance_scale=7.5, latents=eps, output_type="latent")
    old, pipe.scheduler = pipe.scheduler, scheduler(kind)
    try:
        out = pipe(prompts, image=init, strength=0.6, mask_image=mask, **call).cpu()
        executed = len(pipe.last_aux)
        txt = pipe(prompts, **call).cpu()
        if kind == "ddim":
            # what the feature leaves alone keeps working with an image: no CFG, and a pixel-resolution mask
            nocfg = pipe(prompts, image=init, strength=0.6, **{**call, "guidance_scale": 1.0})
            assert torch.isfinite(nocfg).all() and pipe.unet.hip.ctx["rows"] == S
            big = torch.rand(1, 1, 8 * h, 8 * h, generator=torch.Generator().manual_seed(83))
            small = torch.nn.functional.avg_pool2d(big, 8)
            assert torch.equal(pipe(prompts, image=init, strength=0.6, mask_image=big, **call),
                               pipe(prompts, image=init, strength=0.6, mask_image=small, **call))
    finally:
        pipe.scheduler = old
    assert out.shape == (S, 4, h, h) and torch.isfinite(out).all() and executed == 3
    ehs = pipe._encode_prompt(prompts, "cpu", 1, True, None).half().float()
    ref = trajectory(ounet.TINY, pipe.unet.state_dict(), ehs, init, eps, T, 2, kind, mask=mask, guidance_scale=7.5)
    assert report(f"pipeline img2img + soft mask, {kind}, vs CPU reference", out, ref)[0] < 1e-2
    band = h // 4
    assert torch.equal(out[:, :, :band], init[:, :, :band])                 # m = 0: the original, exactly
    d = float((out - txt).norm() / txt.norm())
    print(f"[parity] {kind}: img2img vs txt2img from the same eps: relative distance {d:.3e}")
    assert d > 5e-2


@pytest.mark.parametrize("S", [1, 2])
def test_pipeline_pixels_through_the_vae_and_draw_order(pipe, S):
    """image = pixels: the posterior noise is the first draw from the generator, eps the second - re-drawn by hand, encoded with
    HipVAEEncoder.encode(.., 0.18215) and passed as image= (4 channels) and latents=, the call is the same bit for bit.  S = 2: a
    generator list, one [1, 4, h, w] draw per sample and purpose; the one picture is broadcast over the samples."""
    from sketch2img_amd import synthetic
    from sketch2img_amd.config import TINY_VAE
    from sketch2img_amd.vae import AutoencoderKL
    px, h = 64, 8
    pixels = synthetic.pictures(3, 1, px, px)
    assert pixels.shape == (1, 3, px, px) and float(pixels.min()) >= -1.0 and float(pixels.max()) <= 1.0
    prompt = "a cat" if S == 1 else ["a cat", "a dog"]
    gens = lambda: torch.Generator().manual_seed(7) if S == 1 else [torch.Generator().manual_seed(7 + s) for s in range(S)]
    call = dict(height=px, width=px, num_inference_steps=4, strength=0.5, output_type="latent")
    old, pipe.vae = pipe.vae, AutoencoderKL(TINY_VAE).to("cuda")
    try:
        g = gens()
        a = pipe(prompt, image=pixels, generator=g, **call)
        r = gens()
        draw = (lambda: torch.randn((1, 4, h, h), generator=r)) if S == 1 else \
            (lambda: torch.cat([torch.randn((1, 4, h, h), generator=q) for q in r]))
        pn, eps = draw(), draw()
        init = pipe.vae._hip_enc.encode(pixels.to(DEV).expand(S, -1, -1, -1), pn, 0.18215)
        b = pipe(prompt, image=init, latents=eps, **call)
        left = lambda q: [x.get_state() for x in (q if isinstance(q, list) else [q])]
        assert all(torch.equal(u, v) for u, v in zip(left(g), left(r))), "the call drew another number of values"
    finally:
        pipe.vae = old
    assert a.shape == (S, 4, h, h) and torch.isfinite(a).all() and torch.equal(a, b)
    assert len(pipe.last_aux) == 2
    if S == 2:
        assert not torch.equal(a[0], a[1])


# ---------------------------------------------------------------------------------------------------- hipGraph replay
@pytest.mark.parametrize("kind", ["ddim", "sde"])
def test_graph_replay_of_masked_img2img_is_bit_identical(tiny, kind):
    """T = 4, start 1, with a mask: replay == eager bit for bit (DDIM eta = 0; the SDE solver from equally seeded generators, which
    end in the same state).  Another init and mask of the same shapes reuse the set; a call without init_latents afterwards
    captures a second set and gives today's output."""
    from sketch2img_amd.sampler import HipSampler
    T, S, h, k = 4, tiny["S"], 16, 1
    tab = tables(kind, T)
    eager, graphed = HipSampler(tiny["net"], None), HipSampler(tiny["net"], None, use_graphs=True)

    def run(sampler, seed, img2img=True):
        c = case(S, h, h, seed=90 + seed)
        gen = torch.Generator().manual_seed(seed)
        kw = dict(init_latents=c["init"], start_step=k, mask=soft_mask(1, h, h, seed=seed)) if img2img else {}
        out = sampler.sample(c["eps"], None, T, tables=tab, generator=gen, **kw).clone()
        return out, gen.get_state(), len(sampler.last_aux)

    outs = {}
    for seed in (1, 2, 1):
        a, sa, na = run(eager, seed)
        b, sb, nb = run(graphed, seed)              # seed 1 first: capture + replay; then replays of the cached set
        assert torch.isfinite(a).all() and torch.equal(a, b), seed
        assert torch.equal(sa, sb), "the graph path drew another number of values than the eager loop"
        assert na == nb == T - k
        assert seed not in outs or torch.equal(outs[seed], a)
        outs[seed] = a
    assert len(graphed._graphs) == 1 and not torch.equal(outs[1], outs[2])
    ent = next(iter(graphed._graphs.values()))
    assert len(ent.graphs) == T - k and ent.init is not None and ent.mask is not None
    a, sa, na = run(eager, 1, img2img=False)
    b, sb, nb = run(graphed, 1, img2img=False)
    assert len(graphed._graphs) == 2 and torch.equal(a, b) and torch.equal(sa, sb) and na == nb == T
    assert not torch.equal(a, outs[1])
