"""GPU tests (-m gpu) of the sampler options of the reference call: the DDIM step with eta > 0 (skg_cfg_ddim_eta_step) against
float64 restatements, sampling without classifier-free guidance (guidance_scale <= 1: the UNet runs the cond rows alone),
generator lists, and both under hipGraph replay.  References are written here or come from the CPU oracle."""
import math

import numpy as np
import pytest
import torch

from tests.util import report

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def nchw(rows_f64, S, HW):
    """[S*HW, 4] NHWC rows -> [S, 4, HW]."""
    return rows_f64.reshape(S, HW, 4).transpose(0, 2, 1)


def eta_step_f64(u, v, x, z, g, coeffs, vpred):
    """The step in float64 numpy from the kernel's own operands (u, v: [S, 4, HW] model outputs; coeffs: the fp32 scalars)."""
    c0, c1, c2, c_dir, sigma = (np.float64(np.float32(c)) for c in coeffs)
    e = u + np.float64(g) * (v - u)
    if vpred:
        e, x0 = c0 * e + c1 * x, c0 * x - c1 * e
    else:
        x0 = (x - c1 * e) / c0
    return c2 * x0 + c_dir * e + sigma * z, e


# ---------------------------------------------------------------------------------------------------- the kernel
S_K, H_K, W_K = 3, 5, 7                     # HW = 35: an odd element count (420), a grid tail
_KCASE = {}


def _kernel_case():
    """Operands shared by the kernel tests (drawn once, never written): fp32 eps for both CFG halves - the pair case splits it into
    hi + lo, the others use its fp16 value - latents and noise."""
    if not _KCASE:
        HW = H_K * W_K
        _KCASE.update(e32=rnd(2 * S_K * HW, 4, seed=1), x=rnd(S_K, 4, H_K, W_K, seed=2), z=rnd(S_K, 4, H_K, W_K, seed=3), HW=HW)
    return _KCASE


def _eps_operand(mode):
    """-> (device view whose first 4 columns are the model output, lo_off, float64 value [2*S*HW, 4])."""
    c = _kernel_case()
    hi = c["e32"].half()
    n = hi.shape[0]
    if mode == "ld8":
        buf = torch.full((n, 8), 3.0, dtype=torch.float16)
        buf[:, :4] = hi
        return buf.to(DEV), 0, hi.double().numpy()
    buf = torch.full((n, 24), 3.0, dtype=torch.float16)
    if mode == "pair":
        lo = (c["e32"] - hi.float()).half()
        buf[:, :4], buf[:, 8:12] = hi, lo
        return buf.to(DEV), 8, (hi.double() + lo.double()).numpy()
    d = buf.to(DEV)
    d[:, 12:16] = hi.to(DEV)
    return d[:, 12:], 0, hi.double().numpy()                          # a column view: ld = 24


@pytest.mark.parametrize("mode", ["ld8", "ld24", "vpred", "pair", "no_eps_out"])
def test_eta_step_kernel_known_answer(mode):
    """skg_cfg_ddim_eta_step vs float64: g = 7.5, N(0, 1) operands, eta = 0.7, the first, a middle and the last step of the 50-step
    table (1 / c0 = 13 at the first).  Bounds: those of test_cfg_ddim_and_guidance_update - max abs 1e-5 on eps_out, 2e-5 on x_prev."""
    from sketch2img_amd import ops
    from sketch2img_amd.sampler import DDIMTables
    c = _kernel_case()
    S, HW = S_K, c["HW"]
    eps, lo_off, e64 = _eps_operand({"vpred": "ld8", "no_eps_out": "ld24"}.get(mode, mode))
    assert eps.stride(0) == (8 if mode in ("ld8", "vpred") else 24)
    u, v = nchw(e64[:S * HW], S, HW), nchw(e64[S * HW:], S, HW)
    x64, z64 = c["x"].double().numpy().reshape(S, 4, HW), c["z"].double().numpy().reshape(S, 4, HW)
    x, z = c["x"].to(DEV), c["z"].to(DEV)
    tab = DDIMTables.make(50)
    for idx in (0, 7, 49):
        co = tab.coeffs_eta(int(tab.timesteps[idx]), 0.7)
        res = ops.cfg_ddim_eta_step(eps[:S * HW], eps[S * HW:], x, z, S, HW, 7.5, co, want_eps=mode != "no_eps_out", lo_off=lo_off,
                                    v_prediction=mode == "vpred")
        xr, er = eta_step_f64(u, v, x64, z64, 7.5, co, mode == "vpred")
        if mode == "no_eps_out":
            assert isinstance(res, torch.Tensor)
            xp = res
        else:
            xp, e = res
            assert report(f"eta step {mode} idx{idx}: eps_out", e.cpu().reshape(S, 4, HW), torch.from_numpy(er))[1] < 1e-5
        assert report(f"eta step {mode} idx{idx}: x_prev", xp.cpu().reshape(S, 4, HW), torch.from_numpy(xr))[1] < 2e-5
        assert co[4] > 0 and float((xp.cpu().reshape(S, 4, HW).double() - torch.from_numpy(xr - np.float64(co[4]) * z64)).abs().max()) > 1e-3


def test_eta_step_kernel_identities():
    from sketch2img_amd import ops
    from sketch2img_amd._lib import SkgError, check, lib
    from sketch2img_amd.sampler import DDIMTables
    c = _kernel_case()
    S, HW = S_K, c["HW"]
    x, z = c["x"].to(DEV), c["z"].to(DEV)
    tab = DDIMTables.make(50)
    t = int(tab.timesteps[7])
    for mode, vp in (("ld8", False), ("ld24", True), ("pair", False)):
        eps, lo_off, _ = _eps_operand(mode)
        eu, ec = eps[:S * HW], eps[S * HW:]
        # sigma = 0: the noise-free step, bit for bit, whatever (finite) z holds
        a = ops.cfg_ddim_step(eu, ec, x, S, HW, 7.5, tab.coeffs(t), want_eps=True, lo_off=lo_off, v_prediction=vp)
        b = ops.cfg_ddim_eta_step(eu, ec, x, z, S, HW, 7.5, tab.coeffs_eta(t, 0.0), want_eps=True, lo_off=lo_off, v_prediction=vp)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), mode
        # no CFG: one tensor as both operands, g = 1 -> eps_out is the fp32 value of the input
        _, e = ops.cfg_ddim_eta_step(eu, eu, x, z, S, HW, 1.0, tab.coeffs_eta(t, 0.7), want_eps=True, lo_off=lo_off)
        val = eu[:, :4].float() + (eu[:, lo_off:lo_off + 4].float() if lo_off else 0.0)
        assert torch.equal(e.reshape(S, 4, HW), val.reshape(S, HW, 4).permute(0, 2, 1)), mode
        _, e = ops.cfg_ddim_step(eu, eu, x, S, HW, 1.0, tab.coeffs(t), want_eps=True, lo_off=lo_off)
        assert torch.equal(e.reshape(S, 4, HW), val.reshape(S, HW, 4).permute(0, 2, 1)), mode
    eps, _, _ = _eps_operand("ld8")
    # z = NULL, through the entry point itself (the wrapper refuses a missing z before it)
    eu, ec, out = eps[:S * HW], eps[S * HW:], torch.empty_like(x)
    with pytest.raises(SkgError) as ei:
        check(lib.skg_cfg_ddim_eta_step(eu.data_ptr(), ec.data_ptr(), eu.stride(0), 0, x.data_ptr(), None, out.data_ptr(), None, S, HW,
                                        7.5, *tab.coeffs_eta(t, 0.7), 0, ops._stream()), "skg_cfg_ddim_eta_step")
    assert ei.value.rc == -1
    with pytest.raises(AssertionError):
        ops.cfg_ddim_eta_step(eu, ec, x, None, S, HW, 7.5, tab.coeffs_eta(t, 0.7))
    narrow = torch.zeros(2 * S * HW, 2, device=DEV, dtype=torch.float16)
    with pytest.raises(SkgError) as ei:
        ops.cfg_ddim_eta_step(narrow[:S * HW], narrow[S * HW:], x, z, S, HW, 7.5, tab.coeffs_eta(t, 0.7))
    assert ei.value.rc == -1
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- the sampler
@pytest.fixture(scope="module")
def tiny():
    from oracle import unet as ounet
    from sketch2img_amd.config import TINY
    from sketch2img_amd.unet import HipUNet
    W = ounet.init_weights(ounet.TINY)
    return dict(W=W, net=HipUNet(TINY, W, DEV))


def test_guided_step_with_eta_takes_its_length_from_the_noised_step(tiny):
    """modules/pipeline.py:104-108,157-161: the guidance update is scaled by ||x - x_prev|| of the scheduler's output, which
    for eta > 0 includes sigma z.  One step, S = 1, 16 x 16 latents, eta = 0.5, the same z with and without the LGP: the difference
    of the two results has norm alpha ||g|| (1e-4) and aux[2] is sqrt(2) ||x - x_prev(unguided)|| (1e-5) - the tolerances of
    test_cfg_ddim_and_guidance_update."""
    from oracle import lgp as olgp, unet as ounet
    from sketch2img_amd.lgp import HipLGP
    from sketch2img_amd.sampler import DDIMTables, HipSampler
    net, h = tiny["net"], 16
    g = torch.Generator().manual_seed(8)
    x = torch.randn(1, 4, h, h, generator=g).to(DEV)
    z = torch.randn(1, 4, h, h, generator=g).to(DEV)
    target = (0.18215 * torch.randn(1, 4, h, h, generator=g)).to(DEV)
    net.prepare_context(torch.randn(2, 77, ounet.TINY.cross_attention_dim, generator=g).half().float())
    sd = olgp.init_state_dict(sum(ounet.tap_channels(ounet.TINY)) + 40, seed=12)
    tab = DDIMTables.make(4)
    guided, aux = HipSampler(net, HipLGP(sd, ounet.tap_channels(ounet.TINY), DEV)).step(x, x, target, tab, 0, 7.5, 1.6, eta=0.5, z=z)[::2]
    plain, aux0 = HipSampler(net, None).step(x, x, None, tab, 0, 7.5, 1.6, eta=0.5, z=z)[::2]
    det = HipSampler(net, None).step(x, x, None, tab, 0, 7.5, 1.6)[0]
    assert aux0 is None and aux is not None
    upd, want = float((guided - plain).double().norm()), float(aux[0, 0].double() * aux[0, 1].double())
    dx = math.sqrt(2.0) * float((x - plain).double().norm())
    dx_det = math.sqrt(2.0) * float((x - det).double().norm())
    print(f"[parity] guided eta step: |update| {upd:.6e} alpha*|g| {want:.6e} rel {abs(upd / want - 1):.2e}; aux[2] {float(aux[0, 2]):.6e} "
          f"sqrt2*|dx| noised {dx:.6e} rel {abs(float(aux[0, 2]) / dx - 1):.2e} (noise-free step: {dx_det:.6e})")
    assert abs(upd / want - 1) < 1e-4
    assert abs(float(aux[0, 2]) / dx - 1) < 1e-5
    assert abs(dx_det / dx - 1) > 1e-3          # (the two lengths differ by far more than the tolerance: the check can tell them apart)


# ---------------------------------------------------------------------------------------------------- the pipeline
@pytest.fixture(scope="module")
def pipe():
    from modules.pipeline import AntiGradientPipeline
    from sketch2img_amd.config import TINY
    return AntiGradientPipeline.from_pretrained(None, unet_config=TINY, torch_dtype=torch.float16).to("cuda")


def _dpm_scheduler():
    from sketch2img_amd.schedulers import DPMSolverMultistepScheduler
    return DPMSolverMultistepScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", num_train_timesteps=1000,
                                       algorithm_type="dpmsolver++", solver_type="midpoint", lower_order_final=True)


def test_pipeline_eta_with_generator_list_vs_oracle(pipe):
    """Two prompts, generator=[g0, g1] on the CPU, eta = 0.6, 3 steps at 32 x 32 latents.  Reference: latents and per-step noise
    re-drawn from equally seeded generators in the documented order (draw_noise), the oracle UNet per step, CFG in fp32, the step
    formula in float64.  Bound 1e-2 relative, as the unguided pipeline-vs-oracle tests of the same trajectory length."""
    from oracle import unet as ounet
    from sketch2img_amd.sampler import DDIMTables
    h, T, eta, prompts = 32, 3, 0.6, ["a cat", "a dog on a hill"]
    S = len(prompts)
    gens = lambda: [torch.Generator().manual_seed(100 + s) for s in range(S)]
    call = dict(negative_prompt="blurry", height=8 * h, width=8 * h, num_inference_steps=T, output_type="latent")
    out = pipe(prompts, eta=eta, generator=gens(), **call).cpu()
    assert out.shape == (S, 4, h, h) and torch.isfinite(out).all()
    assert pipe.unet.hip.ctx["rows"] == 2 * S
    assert torch.equal(out, pipe(prompts, eta=eta, generator=gens(), **call).cpu())       # seeded: reproducible
    # ---- reference
    ehs = pipe._encode_prompt(prompts, "cpu", 1, True, "blurry").half().float()
    W = pipe.unet.state_dict()
    rs = gens()
    draw = lambda: torch.cat([torch.randn((1, 4, h, h), generator=r) for r in rs])
    x = draw()
    lat0 = x.clone()
    tab = DDIMTables.make(T)
    for t in tab.timesteps.tolist():
        with torch.no_grad():
            eps, _ = ounet.unet_forward(ounet.TINY, W, torch.cat([x, x]), t, ehs)
        eu, ec = eps.float().chunk(2)
        e = eu + 7.5 * (ec - eu)
        z = draw()
        prev = t - tab.ratio
        a_t = float(tab.alphas_cumprod[t])
        a_p = float(tab.alphas_cumprod[prev]) if prev >= 0 else float(np.float32(tab.final_alpha_cumprod))
        sigma = eta * math.sqrt((1 - a_p) / (1 - a_t) * (1 - a_t / a_p))
        x0 = (x.double() - math.sqrt(1 - a_t) * e.double()) / math.sqrt(a_t)
        x = (math.sqrt(a_p) * x0 + math.sqrt(1 - a_p - sigma ** 2) * e.double() + sigma * z.double()).float()
    assert report("pipeline eta = 0.6, generator list, vs oracle", out, x)[0] < 1e-2
    # ---- eta = 0 from the same latents is another trajectory, and is today's call
    det = pipe(prompts, eta=0.0, generator=gens(), **call).cpu()
    assert torch.equal(det, pipe(prompts, generator=gens(), **call).cpu())
    assert torch.equal(det, pipe(prompts, latents=lat0, **call).cpu())                      # the list seeded the latents
    d = float((out - det).norm() / det.norm())
    print(f"[parity] pipeline eta = 0.6 vs eta = 0: relative distance {d:.3e}")
    assert d > 5e-2
    # DPM-Solver++ has no eta: the argument is ignored, and no noise is drawn from the generators
    old, pipe.scheduler = pipe.scheduler, _dpm_scheduler()
    try:
        gs = gens()
        a = pipe(prompts, eta=0.6, generator=gs, **call)
        left = [g.get_state() for g in gs]
        gs = gens()
        b = pipe(prompts, generator=gs, **call)
        assert torch.equal(a, b) and all(torch.equal(p, q.get_state()) for p, q in zip(left, gs))
    finally:
        pipe.scheduler = old


@pytest.mark.parametrize("sched", ["ddim", "dpm"])
@pytest.mark.parametrize("S", [1, 3])
def test_pipeline_without_cfg_vs_oracle(pipe, S, sched):
    """guidance_scale = 1.0: the UNet evaluates the S cond rows alone (ctx rows == S), the negative prompt plays no part, and any
    guidance_scale <= 1 is the same call.  Reference: the oracle forward on the cond embeddings + oracle scheduler steps; 1e-2."""
    from oracle import ddim as oddim, dpmsolver as odpm, unet as ounet
    h, T = 32, 3
    prompts = ["a cat", "a dog on a hill", "tree"][:S]
    prompt = prompts[0] if S == 1 else prompts
    lat = rnd(S, 4, h, h, seed=20 + S)
    call = dict(height=8 * h, width=8 * h, num_inference_steps=T, latents=lat, output_type="latent")
    old = pipe.scheduler
    pipe.scheduler = _dpm_scheduler() if sched == "dpm" else None
    try:
        out = pipe(prompt, guidance_scale=1.0, **call).cpu()
        assert pipe.unet.hip.ctx["rows"] == S
        assert torch.equal(out, pipe(prompt, guidance_scale=1.0, negative_prompt="blurry, low quality", **call).cpu())
        assert torch.equal(out, pipe(prompt, guidance_scale=0.5, **call).cpu())
        cfg = pipe(prompt, guidance_scale=7.5, **call).cpu()
        assert pipe.unet.hip.ctx["rows"] == 2 * S and not torch.equal(cfg, out)
    finally:
        pipe.scheduler = old
    ehs = pipe._encode_prompt(prompt, "cpu", 1, False, None).half().float()
    assert ehs.shape[0] == S
    W = pipe.unet.state_dict()
    tab = odpm.make_tables(T) if sched == "dpm" else oddim.make_tables(T)
    state = odpm.DPMState()
    x = lat.clone()
    for i, t in enumerate(tab.timesteps.tolist()):
        with torch.no_grad():
            eps, _ = ounet.unet_forward(ounet.TINY, W, x, t, ehs)
        x = odpm.dpm_step(tab, state, eps, i, x) if sched == "dpm" else oddim.ddim_step(tab, eps, t, x)
    assert report(f"pipeline without CFG, S = {S}, {sched}, vs oracle", out, x)[0] < 1e-2


def test_no_cfg_with_clip_injection_vs_oracle():
    """One cond row through the facade with a one-row CLIP-token state ([h], no zero row in front) against the oracle's injected
    forward; bound as test_injected_attention_vs_oracle at two rows.  A state whose row count differs from the batch raises
    before the forward's first launch."""
    import contextlib
    import io
    from modules.pipeline import AntiGradientPipeline
    from oracle import attn_inject, unet as ounet
    from sketch2img.modules.clip_guided_attn import SatMixin
    from sketch2img_amd.config import TINY
    p = AntiGradientPipeline.from_pretrained(None, unet_config=TINY).to("cuda")
    with contextlib.redirect_stdout(io.StringIO()):
        sat = SatMixin(p.unet)
    sd = attn_inject.init_state_dict(ounet.TINY, "clip")
    sat.load_state_dict(sd)
    sat.to(torch.device("cuda"), dtype=p.unet.dtype)
    g = torch.Generator().manual_seed(6)
    h = 32
    x = torch.randn(1, 4, h, h, generator=g).half().float()
    ehs = torch.randn(1, 77, TINY.cross_attention_dim, generator=g).half().float()
    hid = torch.randn(1, 257, 1024, generator=g).half().float()
    W = p.unet.state_dict()
    sat.set_state(hid.to(DEV))
    sat.set_scale(0.8)
    eps = p.unet(x.to(DEV), 301, ehs).sample.cpu()
    with torch.no_grad():
        ref, _ = ounet.unet_forward(ounet.TINY, W, x, 301, ehs, inject=attn_inject.make_clip_inject(sd, hid, 0.8))
        base, _ = ounet.unet_forward(ounet.TINY, W, x, 301, ehs)
    assert report("inject clip, one cond row, scale 0.8", eps, ref)[0] < 1e-2
    assert (ref - base).abs().max() > 1e-3
    sat.set_state(torch.cat([torch.zeros_like(hid), hid]).to(DEV))       # the CFG layout against a one-row batch
    with pytest.raises(ValueError, match="rows"):
        p.unet(x.to(DEV), 301, ehs)
    # the whole call without CFG, one-row state: runs, and differs from the call without the injector
    sat.set_state(hid.to(DEV))
    call = dict(guidance_scale=1.0, height=8 * h, width=8 * h, num_inference_steps=2, latents=x, output_type="latent")
    a = p("a cat", **call)
    p.unet.hip.inject = None
    b = p("a cat", **call)
    assert torch.isfinite(a).all() and not torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------- hipGraph replay
@pytest.mark.parametrize("eta,classifier_free", [(0.5, True), (0.5, False), (0.0, False)])
def test_graph_replay_with_eta_and_without_cfg_is_bit_identical(tiny, eta, classifier_free):
    """As test_graph_replay_is_bit_identical_to_eager: replay == eager bit for bit, from equally seeded generators (the latents and
    every step's noise come from the one generator).  The warm-up pass of a new set consumes no generator state; a second sample()
    on the cached set with another seed is another trajectory and equals eager for that seed."""
    from oracle import unet as ounet
    from sketch2img_amd.sampler import DDIMTables, HipSampler
    net, h, T, S = tiny["net"], 16, 4, 2
    g = torch.Generator().manual_seed(31)
    net.prepare_context(torch.randn(2 * S if classifier_free else S, 77, ounet.TINY.cross_attention_dim, generator=g).half().float())
    tab = DDIMTables.make(T)
    eager, graphed = HipSampler(net, None), HipSampler(net, None, use_graphs=True)

    def run(sampler, seed):
        gen = torch.Generator().manual_seed(seed)
        x0 = torch.randn(S, 4, h, h, generator=gen)
        out = sampler.sample(x0, None, T, tables=tab, eta=eta, generator=gen, classifier_free=classifier_free).clone()
        return out, gen.get_state()

    outs = {}
    for seed in (1, 2, 1):
        a, sa = run(eager, seed)
        b, sb = run(graphed, seed)            # seed 1 first: capture + replay; then replays of the cached set
        assert torch.isfinite(a).all() and torch.equal(a, b), seed
        assert torch.equal(sa, sb), "the graph path drew another number of values than the eager loop"
        assert seed not in outs or torch.equal(outs[seed], a)
        outs[seed] = a
    assert len(graphed._graphs) == 1 and not torch.equal(outs[1], outs[2])
    assert net.ctx["rows"] == (2 * S if classifier_free else S)
    if eta > 0:
        gen = torch.Generator().manual_seed(1)
        x0 = torch.randn(S, 4, h, h, generator=gen)
        det = graphed.sample(x0, None, T, tables=tab, classifier_free=classifier_free)      # another key: eta = 0
        assert len(graphed._graphs) == 2 and not torch.equal(det, outs[1])


def test_every_option_at_once_replays_as_eager(tiny):
    """Every option through the one step runner in one call: the stochastic Karras DPM-Solver++ with a list of two generators,
    img2img from entry 1 with a per-sample mask, a ControlNet on the window (0.25, 0.75), no sketch target; non-square latents
    [2, 4, 8, 16].  T = 4 is the shortest schedule with a second-order step and with executed steps outside the window at both
    ends (of the 3 executed steps only the middle one is controlled); S = 2 separates the per-sample masks and generators.
    Replay == eager bit for bit; another init, mask and hint of the same shapes replay the same set; the uncontrolled call is a
    second set and equals the uncontrolled eager run."""
    from oracle import unet as ounet
    from sketch2img_amd.config import TINY
    from sketch2img_amd.controlnet import Control, ControlNetModel
    from sketch2img_amd.sampler import DPMTables, HipSampler
    net, S, h, w, T = tiny["net"], 2, 8, 16, 4
    ehs = rnd(2 * S, 77, ounet.TINY.cross_attention_dim, seed=41).half().float()
    cnet = ControlNetModel.from_pretrained(None, unet_config=TINY).to(DEV).hip
    net.prepare_context(ehs)
    cnet.prepare_context(ehs)
    tab = DPMTables.make(T, use_karras_sigmas=True, algorithm_type="sde-dpmsolver++")
    eager, graphed = HipSampler(net), HipSampler(net, use_graphs=True)

    def run(sampler, seed, controlled=True):
        g = torch.Generator().manual_seed(seed)
        eps, init = torch.randn(S, 4, h, w, generator=g), 0.8 * torch.randn(S, 4, h, w, generator=g)
        mask = (torch.rand(S, 1, h, w, generator=g) > 0.5).float()
        assert not torch.equal(mask[0], mask[1])
        control = None
        if controlled:
            hint = cnet.hint_rows(cnet.embed(torch.rand(1, 3, 8 * h, 8 * w, generator=g).to(DEV)), 1, 2 * S)
            control = Control(cnet, hint, 0.8, 0.25, 0.75)
        gens = [torch.Generator().manual_seed(1000 * seed + b) for b in range(S)]
        out = sampler.sample(eps, None, T, tables=tab, generator=gens, init_latents=init, start_step=1, mask=mask, control=control)
        return out.clone(), [gen.get_state() for gen in gens], len(sampler.last_aux)

    outs = []
    for seed in (1, 2):                         # capture + replay, then a replay of the cached set with other buffers
        a, sa, na = run(eager, seed)
        b, sb, nb = run(graphed, seed)
        assert torch.isfinite(a).all() and torch.equal(a, b), seed
        assert all(torch.equal(p, q) for p, q in zip(sa, sb)) and na == nb == T - 1
        assert len(graphed._graphs) == 1
        outs.append(a)
    assert not torch.equal(outs[0], outs[1])
    a, _, _ = run(eager, 1, controlled=False)
    b, _, _ = run(graphed, 1, controlled=False)
    assert len(graphed._graphs) == 2 and torch.equal(a, b) and not torch.equal(a, outs[0])
