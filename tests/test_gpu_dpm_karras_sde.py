"""GPU tests (-m gpu) of DPM-Solver++ 2M with Karras sigmas and of its stochastic variant: the step kernel
skg_cfg_dpmpp2m_sde_step against a float32 composition of its formula and, at d = 0, against skg_cfg_dpmpp2m_step bit for bit;
4-step trajectories on the TINY UNet against the CPU oracle's forward driven by the float64 coefficients of tests/dpm_ref.py;
the draw order of generators; hipGraph replay; one guided run; the pipeline call."""
import math

import numpy as np
import pytest
import torch

from tests.dpm_ref import karras_ref, ode_ref, sde_ref, source_ref
from tests.util import report

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SDE = "sde-dpmsolver++"


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ---------------------------------------------------------------------------------------------------- the kernel
S_K, LD = 2, 8
_KCASE = {}


def _kernel_case(h, w):
    """Operands of one spatial size, drawn once and never written: fp32 model outputs for two steps (both CFG halves; the pair
    layout splits them into hi + lo, the plain one uses their fp16 value), latents, noise."""
    if (h, w) not in _KCASE:
        HW = h * w
        _KCASE[(h, w)] = dict(e32=[rnd(2 * S_K * HW, 4, seed=11 + k) for k in range(2)], x=rnd(S_K, 4, h, w, seed=2),
                              z=[rnd(S_K, 4, h, w, seed=5 + k) for k in range(2)])
    return _KCASE[(h, w)]


def _eps_operand(e32, pair):
    """-> (device buffer [2*S*HW, 8] whose first 4 columns are the model output, lo_off, the fp32 value the kernel combines)."""
    hi = e32.half()
    buf = torch.full((e32.shape[0], LD), 3.0, dtype=torch.float16)
    buf[:, :4] = hi
    if not pair:
        return buf.to(DEV), 0, hi.float()
    lo = (e32 - hi.float()).half()
    buf[:, 4:8] = lo
    return buf.to(DEV), 4, hi.float() + lo.float()


def _nchw(rows, S, h, w):
    return rows.reshape(S, h * w, 4).permute(0, 2, 1).reshape(S, 4, h, w)


@pytest.mark.parametrize("vpred", [0, 1])
@pytest.mark.parametrize("pair", [False, True], ids=["fp16", "pair"])
@pytest.mark.parametrize("h,w", [(8, 8), (5, 9)])
def test_sde_step_kernel_vs_fp32_composition(h, w, pair, vpred):
    """The first two steps of the 25-step Karras SDE schedule (first order, then second order on the first step's x0 history) on
    N(0, 1) operands, g = 7.5: eps_out, x_prev and the x0 history against the formula composed in float32 on the CPU.  Bounds: those
    of test_cfg_dpmpp2m_step_vs_oracle for the deterministic entry on the same kind of operands - max abs 1e-5 on eps_out, 2e-5 on
    x_prev, and on the x0 history 1e-6 relative (max abs 2e-5 for v-prediction).  The first step runs with eps_out, the second without."""
    from sketch2img_amd import ops
    from sketch2img_amd.sampler import DPMTables
    c = _kernel_case(h, w)
    S, HW = S_K, h * w
    tab = DPMTables.make(25, use_karras_sigmas=True, algorithm_type=SDE)
    x = c["x"]
    xg, x0_io, x0_ref, seen = x.to(DEV), torch.zeros(S, 4, h, w, device=DEV), None, 0
    for i in range(2):
        eps, lo_off, val = _eps_operand(c["e32"][i], pair)
        assert eps.stride(0) == LD
        z = c["z"][i]
        order = tab.order(i, seen)
        seen = min(seen + 1, 2)
        assert order == i + 1
        co = tab.coeffs_sde(i, order)
        assert co[5] > 0 and (co[4] != 0) == (order == 2)
        res = ops.cfg_dpmpp2m_sde_step(eps[:S * HW], eps[S * HW:], xg, z.to(DEV), x0_io, S, HW, 7.5, co, want_eps=i == 0, lo_off=lo_off,
                                       v_prediction=bool(vpred))
        al, sg, a, b, cc, d = (torch.tensor(v, dtype=torch.float32) for v in co)
        eu, ec = _nchw(val[:S * HW], S, h, w), _nchw(val[S * HW:], S, h, w)
        e = eu + 7.5 * (ec - eu)
        if vpred:
            x0, e = al * x - sg * e, al * e + sg * x
        else:
            x0 = (x - sg * e) / al
        ref = a * x + b * x0
        if order == 2:
            ref = ref + cc * x0_ref
        ref = ref + d * z
        assert ref.dtype == torch.float32
        tag = f"sde step {h}x{w} {'pair' if pair else 'fp16'} vpred{vpred} order {order}"
        if i == 0:
            xp, eo = res
            assert report(f"{tag}: eps_out", eo.cpu(), e)[1] < 1e-5
        else:
            assert isinstance(res, torch.Tensor)
            xp = res
        assert report(f"{tag}: x_prev", xp.cpu(), ref)[1] < 2e-5
        hist = report(f"{tag}: x0 history", x0_io.cpu(), x0)
        assert hist[1] < 2e-5 if vpred else hist[0] < 1e-6
        assert float((xp.cpu() - (ref - d * z)).abs().max()) > 1e-2          # (the noise term is far above the tolerance)
        x0_ref = x0
        x, xg = ref, ref.to(DEV)


@pytest.mark.parametrize("pair", [False, True], ids=["fp16", "pair"])
def test_sde_step_with_d_zero_is_the_deterministic_step_bit_for_bit(pair):
    """d = 0 and a random finite z: x_prev, the x0 history and eps_out equal skg_cfg_dpmpp2m_step's on the same inputs, first and
    second order (ODE coefficients of the 25-step Karras schedule, the ragged 5 x 9 size), both prediction types; z = NULL is
    refused by the entry point itself."""
    from sketch2img_amd import ops
    from sketch2img_amd._lib import SkgError, check, lib
    from sketch2img_amd.sampler import DPMTables
    h, w = 5, 9
    c = _kernel_case(h, w)
    S, HW = S_K, h * w
    tab = DPMTables.make(25, use_karras_sigmas=True)
    x, z = c["x"].to(DEV), (100.0 * c["z"][0]).to(DEV)
    eps, lo_off, _ = _eps_operand(c["e32"][0], pair)
    eu, ec = eps[:S * HW], eps[S * HW:]
    hist = c["z"][1].to(DEV)                                     # some previous x0
    for order, i in ((1, 0), (2, 3)):
        for vp in (False, True):
            co = tab.coeffs(i, order)
            ha, hb = hist.clone(), hist.clone()
            a = ops.cfg_dpmpp2m_step(eu, ec, x, ha, S, HW, 7.5, co, want_eps=True, lo_off=lo_off, v_prediction=vp)
            b = ops.cfg_dpmpp2m_sde_step(eu, ec, x, z, hb, S, HW, 7.5, co + (0.0,), want_eps=True, lo_off=lo_off, v_prediction=vp)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(ha, hb), (order, vp)
            assert not torch.equal(ha, hist)
    out, x0 = torch.empty_like(x), hist.clone()
    with pytest.raises(SkgError) as ei:
        check(lib.skg_cfg_dpmpp2m_sde_step(eu.data_ptr(), ec.data_ptr(), LD, lo_off, x.data_ptr(), None, x0.data_ptr(), out.data_ptr(), None,
                                           S, HW, 7.5, *tab.coeffs_sde(0, 1), 0, ops._stream()), "skg_cfg_dpmpp2m_sde_step")
    assert ei.value.rc == -1
    with pytest.raises(AssertionError):
        ops.cfg_dpmpp2m_sde_step(eu, ec, x, None, x0, S, HW, 7.5, tab.coeffs_sde(0, 1))
    torch.cuda.synchronize()
    assert torch.equal(x0, hist)


# ---------------------------------------------------------------------------------------------------- trajectories
H_T, T_T = 16, 4


@pytest.fixture(scope="module")
def tiny():
    from oracle import unet as ounet
    from sketch2img_amd.config import TINY
    from sketch2img_amd.unet import HipUNet
    W = ounet.init_weights(ounet.TINY)
    S = 2
    g = torch.Generator().manual_seed(41)
    ehs = torch.randn(2 * S, 77, ounet.TINY.cross_attention_dim, generator=g).half().float()
    x0 = torch.randn(S, 4, H_T, H_T, generator=g)
    zs = [torch.randn(S, 4, H_T, H_T, generator=g) for _ in range(T_T)]
    return dict(W=W, net=HipUNet(TINY, W, DEV), ehs=ehs, x0=x0, zs=zs, S=S, eps_cache={})


def oracle_trajectory(tiny, tab, zs=None):
    """The loop of HipSampler.sample written out: the oracle UNet at the schedule's integer timesteps, CFG in fp32, the update in
    float64 from tests/dpm_ref.py's coefficients (orders 1, 2, 2 and the final x_prev = x0 of the Karras schedule)."""
    from oracle import unet as ounet
    N = len(tab.timesteps)
    sig, ts = karras_ref(N)
    assert np.array_equal(ts, tab.timesteps) and tab.use_karras_sigmas
    src = source_ref(tab, True, N)
    x, x0_before = tiny["x0"].clone(), None
    for i, t in enumerate(ts.tolist()):
        with torch.no_grad():
            eps, _ = ounet.unet_forward(ounet.TINY, tiny["W"], torch.cat([x, x]), t, tiny["ehs"])
        eu, ec = eps.float().chunk(2)
        e = (eu + 7.5 * (ec - eu)).double()
        x0 = (x.double() - src[i][1] * e) / src[i][0]
        order = 1 if i in (0, N - 1) else 2
        if i == N - 1:
            nxt = x0
        elif zs is None:
            a, b, c = ode_ref(src, i, order)
            nxt = a * x.double() + b * x0 + (c * x0_before if order == 2 else 0.0)
        else:
            a, b, c, d = sde_ref(src, i, order)
            nxt = a * x.double() + b * x0 + (c * x0_before if order == 2 else 0.0) + d * zs[i].double()
        x0_before = x0
        x = nxt.float()
    return x


def run_steps(sampler, tab, x0, zs):
    """sampler.sample's eager loop with the noise of every step passed in."""
    sampler.unet.prepare_timesteps(tab.timesteps.tolist())
    sampler.reset_history()
    x = x0.to(DEV)
    for i in range(len(tab.timesteps)):
        x = sampler.step(x, x, None, tab, i, 7.5, 1.6, z=None if zs is None else zs[i].to(DEV))[0]
    return x


def test_karras_ode_trajectory_vs_oracle(tiny):
    """S = 2, 16 x 16 latents, N = 4, Karras spacing, deterministic: < 1e-2 relative, the bound of the project's 3- and 4-step
    dpm++2m comparisons (the same kernels run).  The last step returns its x0."""
    from sketch2img_amd.sampler import DPMTables, HipSampler
    tab = DPMTables.make(T_T, use_karras_sigmas=True)
    tiny["net"].prepare_context(tiny["ehs"])
    sampler = HipSampler(tiny["net"], None)
    out = sampler.sample(tiny["x0"], None, T_T, tables=tab)
    assert torch.isfinite(out).all() and torch.equal(out, sampler._x0_before)
    assert torch.equal(out, run_steps(HipSampler(tiny["net"], None), tab, tiny["x0"], None))
    ref = oracle_trajectory(tiny, tab)
    assert report("Karras dpm++2m, 4 steps, vs oracle", out.cpu(), ref)[0] < 1e-2
    uni = sampler.sample(tiny["x0"], None, T_T, tables=DPMTables.make(T_T))
    assert float((uni - out).norm() / out.norm()) > 1e-2                  # another schedule, another trajectory


def test_karras_sde_trajectory_vs_oracle(tiny):
    """The same with the stochastic solver and a fixed z per step: < 1e-2 relative against the oracle loop with the same z;
    two runs are bit-equal; the last step (d = 0) still returns its x0."""
    from sketch2img_amd.sampler import DPMTables, HipSampler
    tab = DPMTables.make(T_T, use_karras_sigmas=True, algorithm_type=SDE)
    tiny["net"].prepare_context(tiny["ehs"])
    sampler = HipSampler(tiny["net"], None)
    out = run_steps(sampler, tab, tiny["x0"], tiny["zs"])
    assert torch.isfinite(out).all() and torch.equal(out, sampler._x0_before)
    assert torch.equal(out, run_steps(HipSampler(tiny["net"], None), tab, tiny["x0"], tiny["zs"]))
    ref = oracle_trajectory(tiny, tab, tiny["zs"])
    assert report("Karras sde-dpm++2m, 4 steps, vs oracle", out.cpu(), ref)[0] < 1e-2
    ode = run_steps(HipSampler(tiny["net"], None), DPMTables.make(T_T, use_karras_sigmas=True), tiny["x0"], None)
    assert float((ode - out).norm() / out.norm()) > 5e-2


def test_sde_generators_one_draw_per_step_per_sample(tiny):
    """generator=[g0, g1]: sample b's noise is a [1, 4, h, w] draw from its own generator per step - what a run of sample b alone
    draws - so sample() equals, bit for bit, the step loop fed with those draws; each generator has advanced by exactly T draws; a
    single generator draws [S, 4, h, w] per step.  Sample b run alone (other GEMM shapes, same arithmetic) lands on the same
    trajectory within the 1e-2 of the oracle comparisons."""
    from sketch2img_amd.sampler import DPMTables, HipSampler
    S, T = tiny["S"], T_T
    tab = DPMTables.make(T, use_karras_sigmas=True, algorithm_type=SDE)
    tiny["net"].prepare_context(tiny["ehs"])
    gens = lambda: [torch.Generator().manual_seed(300 + b) for b in range(S)]
    gs = gens()
    out = HipSampler(tiny["net"], None).sample(tiny["x0"], None, T, tables=tab, generator=gs)
    rs = gens()
    zs = [torch.cat([torch.randn((1, 4, H_T, H_T), generator=r) for r in rs]) for _ in range(T)]
    assert all(torch.equal(g.get_state(), r.get_state()) for g, r in zip(gs, rs))
    assert torch.equal(out, run_steps(HipSampler(tiny["net"], None), tab, tiny["x0"], zs))
    one = torch.Generator().manual_seed(7)
    out1 = HipSampler(tiny["net"], None).sample(tiny["x0"], None, T, tables=tab, generator=one, eta=0.3)      # (eta is ignored)
    r = torch.Generator().manual_seed(7)
    zs1 = [torch.randn((S, 4, H_T, H_T), generator=r) for _ in range(T)]
    assert torch.equal(one.get_state(), r.get_state())
    assert torch.equal(out1, run_steps(HipSampler(tiny["net"], None), tab, tiny["x0"], zs1)) and not torch.equal(out1, out)
    # sample 1 alone, from its own generator
    b = 1
    tiny["net"].prepare_context(tiny["ehs"][[b, S + b]])
    alone = HipSampler(tiny["net"], None).sample(tiny["x0"][b:b + 1], None, T, tables=tab, generator=[gens()[b]])
    tiny["net"].prepare_context(tiny["ehs"])
    assert report("sde sample 1 of the batch vs run alone", out[b:b + 1].cpu(), alone.cpu())[0] < 1e-2
    assert float((out[0:1] - alone).norm() / alone.norm()) > 0.1


@pytest.mark.parametrize("algo", ["dpmsolver++", SDE])
def test_graph_replay_of_karras_schedules_is_bit_identical(tiny, algo):
    """Replay == eager bit for bit (S = 1, 16 x 16, N = 4), the latents and every step's noise from one generator; the warm-up pass
    of a new set consumes no generator state; a replay of the cached set with another seed equals eager for that seed; the uniform
    / deterministic tables of the same N are other sets."""
    from sketch2img_amd.sampler import DPMTables, HipSampler
    net = tiny["net"]
    net.prepare_context(tiny["ehs"][[0, tiny["S"]]])
    tab = DPMTables.make(T_T, use_karras_sigmas=True, algorithm_type=algo)
    eager, graphed = HipSampler(net, None), HipSampler(net, None, use_graphs=True)

    def run(sampler, seed, tables=tab):
        gen = torch.Generator().manual_seed(seed)
        x0 = torch.randn(1, 4, H_T, H_T, generator=gen)
        return sampler.sample(x0, None, T_T, tables=tables, generator=gen).clone(), gen.get_state()

    outs = {}
    for seed in (1, 2, 1):
        a, sa = run(eager, seed)
        b, sb = run(graphed, seed)
        assert torch.isfinite(a).all() and torch.equal(a, b), seed
        assert torch.equal(sa, sb), "the graph path drew another number of values than the eager loop"
        assert seed not in outs or torch.equal(outs[seed], a)
        outs[seed] = a
    assert len(graphed._graphs) == 1 and not torch.equal(outs[1], outs[2])
    ent = next(iter(graphed._graphs.values()))
    assert (ent.zs is not None and tuple(ent.zs.shape) == (T_T, 1, 4, H_T, H_T)) if algo == SDE else ent.zs is None
    other = DPMTables.make(T_T, algorithm_type=algo)
    a, _ = run(eager, 1, other)
    b, _ = run(graphed, 1, other)
    assert len(graphed._graphs) == 2 and torch.equal(a, b) and not torch.equal(a, outs[1])
    net.prepare_context(tiny["ehs"])


def test_guided_sde_run(tiny):
    """TINY LGP, SDE, Karras, N = 4: finite, the guidance ran on steps 0..2 (i <= T/2), and - one step, the same z with and without
    the LGP - the update length is sqrt(2) ||x - x_prev|| of the NOISED step: aux[2] within 1e-5 and |update| = alpha ||g|| within
    1e-4, the tolerances of the eta > 0 guided test (test_cfg_ddim_and_guidance_update's)."""
    from oracle import lgp as olgp, unet as ounet
    from sketch2img_amd.lgp import HipLGP
    from sketch2img_amd.sampler import DPMTables, HipSampler
    net = tiny["net"]
    net.prepare_context(tiny["ehs"][[0, tiny["S"]]])
    g = torch.Generator().manual_seed(8)
    x = torch.randn(1, 4, H_T, H_T, generator=g).to(DEV)
    z = torch.randn(1, 4, H_T, H_T, generator=g).to(DEV)
    target = (0.18215 * torch.randn(1, 4, H_T, H_T, generator=g)).to(DEV)
    sd = olgp.init_state_dict(sum(ounet.tap_channels(ounet.TINY)) + 40, seed=12)
    lgp = HipLGP(sd, ounet.tap_channels(ounet.TINY), DEV)
    tab = DPMTables.make(T_T, use_karras_sigmas=True, algorithm_type=SDE)
    det_tab = DPMTables.make(T_T, use_karras_sigmas=True)
    net.prepare_timesteps(tab.timesteps.tolist())
    guided, aux = HipSampler(net, lgp).step(x, x, target, tab, 0, 7.5, 1.6, z=z)[::2]
    plain, aux0 = HipSampler(net, None).step(x, x, None, tab, 0, 7.5, 1.6, z=z)[::2]
    det = HipSampler(net, None).step(x, x, None, det_tab, 0, 7.5, 1.6)[0]
    assert aux0 is None and aux is not None
    upd, want = float((guided - plain).double().norm()), float(aux[0, 0].double() * aux[0, 1].double())
    dx = math.sqrt(2.0) * float((x - plain).double().norm())
    dx_det = math.sqrt(2.0) * float((x - det).double().norm())
    print(f"[parity] guided sde step: |update| {upd:.6e} alpha*|g| {want:.6e} rel {abs(upd / want - 1):.2e}; aux[2] {float(aux[0, 2]):.6e} "
          f"sqrt2*|dx| noised {dx:.6e} rel {abs(float(aux[0, 2]) / dx - 1):.2e} (deterministic step: {dx_det:.6e})")
    assert abs(upd / want - 1) < 1e-4
    assert abs(float(aux[0, 2]) / dx - 1) < 1e-5
    assert abs(dx_det / dx - 1) > 1e-3
    sampler = HipSampler(net, lgp)
    out = sampler.sample(x, target, T_T, tables=tab, generator=torch.Generator().manual_seed(3))
    assert torch.isfinite(out).all()
    assert [a is not None for a in sampler.last_aux] == [True, True, True, False]
    assert all(torch.isfinite(a).all() for a in sampler.last_aux[:3])
    net.prepare_context(tiny["ehs"])


# ---------------------------------------------------------------------------------------------------- the pipeline
def test_pipeline_call_with_karras_sde_scheduler():
    """scheduler=DPMSolverMultistepScheduler(use_karras_sigmas=True, algorithm_type="sde-dpmsolver++"), 3 steps, latents out: the
    sampler's result for the same tables, latents and generator, bit for bit - and neither the deterministic Karras call nor the
    uniform SDE call."""
    from modules.pipeline import AntiGradientPipeline
    from sketch2img_amd.config import TINY
    from sketch2img_amd.sampler import DPMTables, HipSampler
    from sketch2img_amd.schedulers import DPMSolverMultistepScheduler
    pipe = AntiGradientPipeline.from_pretrained(None, unet_config=TINY, torch_dtype=torch.float16).to("cuda")
    h, T = 16, 3
    lat = rnd(1, 4, h, h, seed=9)
    call = dict(negative_prompt="blurry", height=8 * h, width=8 * h, num_inference_steps=T, latents=lat, output_type="latent")
    pipe.scheduler = DPMSolverMultistepScheduler(use_karras_sigmas=True, algorithm_type=SDE)
    gen = torch.Generator().manual_seed(5)
    out = pipe("a cat", generator=gen, **call)
    assert out.shape == (1, 4, h, h) and torch.isfinite(out).all()
    tab = pipe._tables(T)
    assert tab.stochastic and tab.use_karras_sigmas and np.array_equal(tab.timesteps, karras_ref(T)[1])
    r = torch.Generator().manual_seed(5)
    ref = HipSampler(pipe.unet.hip, None).sample(lat, None, T, 7.5, 1.6, tables=DPMTables.make(T, use_karras_sigmas=True, algorithm_type=SDE),
                                                 generator=r)
    assert torch.equal(out, ref) and torch.equal(gen.get_state(), r.get_state())
    assert torch.equal(out, pipe("a cat", generator=torch.Generator().manual_seed(5), **call))
    assert not torch.equal(out, pipe("a cat", generator=torch.Generator().manual_seed(6), **call))
    pipe.scheduler = DPMSolverMultistepScheduler(use_karras_sigmas=True)
    ode = pipe("a cat", **call)
    pipe.scheduler = DPMSolverMultistepScheduler(algorithm_type=SDE)
    uni = pipe("a cat", generator=torch.Generator().manual_seed(5), **call)
    pipe.scheduler = DPMSolverMultistepScheduler()
    base = pipe("a cat", **call)
    assert len({tuple(t.flatten().tolist()[:8]) for t in (out, ode, uni, base)}) == 4
