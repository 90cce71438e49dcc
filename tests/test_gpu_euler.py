"""GPU tests (-m gpu) of the Euler and Euler-ancestral samplers: the step kernel skg_cfg_euler_step against the float64 formula on
the operand values it reads, at a derived per-element bound; the operand kernel skg_model_input bit for bit; 4-step trajectories
on the TINY UNet against the CPU oracle's forward driven by the float64 restatement of tests/euler_ref.py; the draw order of
generators; hipGraph replay; one guided step (the guidance length is measured from the scaled model input); v prediction; img2img
and the masked repaint; one ControlNet step; the pipeline call with both scheduler classes."""
import math

import numpy as np
import pytest
import torch

from tests.euler_ref import U32, ancestral_ref, euler_step_ref, schedule_ref
from tests.test_gpu_dpm_karras_sde import H_T, LD, S_K, T_T, _eps_operand, _kernel_case, _nchw, rnd, tiny      # noqa: F401
from tests.util import report

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = 7.5


def make(N, ancestral=False, spacing="leading", off=1, **kw):
    from sketch2img_amd.sampler import EulerTables
    return EulerTables.make(N, timestep_spacing=spacing, steps_offset=off, ancestral=ancestral, **kw)


# ---------------------------------------------------------------------------------------------------- the step kernel
@pytest.mark.parametrize("ancestral", [False, True], ids=["euler", "euler-a"])
@pytest.mark.parametrize("vpred", [0, 1])
@pytest.mark.parametrize("pair", [False, True], ids=["fp16", "pair"])
@pytest.mark.parametrize("h,w", [(8, 8), (5, 9)])
def test_euler_step_kernel_vs_float64(h, w, pair, vpred, ancestral):
    """The first two steps of the 10-step leading schedule, S = 2, ld = 8, g = 7.5, on N(0, 1) model outputs and noise and a state of
    the schedule's size (init_noise_sigma times N(0, 1); the second step starts from the first one's reference).  x_prev and eps_out
    against the formula in float64 on the operand values the kernel reads - the fp16 / pair model outputs, the fp32 state and noise,
    the five fp32 scalars - element by element:
        |x_prev - ref| <= 16 U32 (|x| + sigma (|u| + g (|c| + |u|)) + sigma_up |z|),      |eps_out - d| <= that / sigma.
    Derived, not measured: the update is fewer than sixteen fp32 operations, each one rounding (relative U32) of an intermediate that
    the sum bounds.  The bound can fail: the float64 result of a wrong formula - sigma_next and sigma_down exchanged, and for v
    prediction the coefficients without c_in - is off by more than 100 times the bound on most elements.  The first step runs with
    eps_out, the second without."""
    from sketch2img_amd import ops
    c = _kernel_case(h, w)
    S, HW = S_K, h * w
    tab = make(10, ancestral, v_prediction=bool(vpred))
    sig = schedule_ref(10, "leading", 1)[0]
    x = (float(np.float32(tab.init_noise_sigma)) * c["x"]).float()
    for i in range(2):
        eps, lo_off, _ = _eps_operand(c["e32"][i], pair)
        assert eps.stride(0) == LD
        rows = eps.cpu()
        val = rows[:, :4].double() + (rows[:, 4:8].double() if pair else 0.0)           # what the kernel's operands hold, exactly
        u, cc = _nchw(val[:S * HW], S, h, w), _nchw(val[S * HW:], S, h, w)
        z = c["z"][i]
        co = tab.coeffs(i)
        s, kx, km, dt, up = co
        assert (up > 0) == ancestral and all(v == float(np.float32(v)) for v in co)
        res = ops.cfg_euler_step(eps[:S * HW], eps[S * HW:], x.to(DEV), z.to(DEV) if ancestral else None, S, HW, G, co, want_eps=i == 0,
                                 lo_off=lo_off)
        xd, zd = x.double(), z.double()
        m = u + G * (cc - u)
        x0 = kx * xd + km * m
        d = (xd - x0) / s
        ref = xd + dt * d + up * zd
        bound = 16 * U32 * (xd.abs() + s * (u.abs() + G * (cc.abs() + u.abs())) + up * zd.abs())
        tag = f"{'euler-a' if ancestral else 'euler'} step {i} {h}x{w} {'pair' if pair else 'fp16'} vpred{vpred}"
        xp, eo = res if i == 0 else (res, None)
        err = (xp.cpu().double() - ref).abs()
        print(f"[parity] {tag}: x_prev max err / bound {float((err / bound).max()):.3f} (max err {float(err.max()):.3e})")
        assert bool((err <= bound).all())
        if eo is not None:
            err_d = (eo.cpu().double() - d).abs()
            print(f"[parity] {tag}: eps_out max err / bound {float((err_d / (bound / s)).max()):.3f}")
            assert bool((err_d <= bound / s).all())
        # the bound separates the formula from its neighbours (CPU side, float64 restatement)
        sn = float(sig[i + 1])
        s_up, s_down = ancestral_ref(float(sig[i]), sn)
        right = euler_step_ref(xd, u, cc, zd, G, float(sig[i]), s_down if ancestral else sn, s_up if ancestral else 0.0, bool(vpred))[0]
        assert bool(((right - ref).abs() <= bound).all())                             # (the scalars' fp32 casts lie inside it too)
        wrong = [euler_step_ref(xd, u, cc, zd, G, float(sig[i]), sn if ancestral else s_down, s_up if ancestral else 0.0, bool(vpred))[0]]
        if vpred:
            wrong.append(xd + dt * ((xd - (xd - s * m)) / s) + up * zd)                 # k_x, k_m without c_in
        for wr in wrong:
            far = ((wr - ref).abs() > 100 * bound).double().mean()
            assert float(far) > 0.5, (tag, float(far))
        x = ref.float()


@pytest.mark.parametrize("pair", [False, True], ids=["fp16", "pair"])
def test_sigma_up_zero_is_the_plain_step_bit_for_bit_and_null_z_is_refused(pair):
    """sigma_up = 0 and a random finite z: x_prev and eps_out equal the z = NULL call's on the same inputs (the ragged 5 x 9 size,
    both prediction types, a middle and the last step); z = NULL with sigma_up != 0 is refused by the entry point itself with
    nothing launched."""
    from sketch2img_amd import ops
    from sketch2img_amd._lib import SkgError
    h, w = 5, 9
    c = _kernel_case(h, w)
    S, HW = S_K, h * w
    x, z = (8.0 * c["x"]).to(DEV), (100.0 * c["z"][0]).to(DEV)
    eps, lo_off, _ = _eps_operand(c["e32"][0], pair)
    eu, ec = eps[:S * HW], eps[S * HW:]
    for vp in (False, True):
        tab = make(10, v_prediction=vp)
        for i in (1, 9):
            co = tab.coeffs(i)
            assert co[4] == 0.0
            a = ops.cfg_euler_step(eu, ec, x, None, S, HW, G, co, want_eps=True, lo_off=lo_off)
            b = ops.cfg_euler_step(eu, ec, x, z, S, HW, G, co, want_eps=True, lo_off=lo_off)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.isfinite(a[0]).all(), (vp, i)
            noisy = ops.cfg_euler_step(eu, ec, x, z, S, HW, G, co[:4] + (0.5,), lo_off=lo_off)
            assert not torch.equal(noisy, a[0])
    with pytest.raises(SkgError) as ei:
        ops.cfg_euler_step(eu, ec, x, None, S, HW, G, make(10, True).coeffs(0))
    assert ei.value.rc == -1
    with pytest.raises(AssertionError):
        ops.cfg_euler_step(eu, ec, x, z[:1], S, HW, G, make(10, True).coeffs(0))


# ---------------------------------------------------------------------------------------------------- the operand kernel
@pytest.mark.parametrize("h,w", [(8, 8), (5, 9)])
def test_model_input_kernel(h, w):
    """c_in = 1, dup = 2: ops.nchw_to_nhwc(torch.cat([x, x])) bit for bit, padding columns included (the output buffer is filled with
    another value first).  c_in = 0.068: the fp32 output is the fp32 product exactly and the fp16 operand its rounding; dup = 1 is the
    first half of dup = 2; without the fp32 output the operand is the same."""
    from sketch2img_amd import ops
    from sketch2img_amd.unet import CIN_PAD
    x = (10.0 * rnd(S_K, 4, h, w, seed=21)).to(DEV)
    M = S_K * h * w
    one, none = ops.model_input(x, 1.0, CIN_PAD, dup=2)
    assert none is None and one.shape == (2 * M, CIN_PAD) and one.dtype == torch.float16
    assert torch.equal(one, ops.nchw_to_nhwc(torch.cat([x, x]).contiguous(), CIN_PAD))
    assert float(one[:, 4:].abs().max()) == 0.0
    cin = float(np.float32(0.068))
    two, xs = ops.model_input(x, cin, CIN_PAD, dup=2, want_scaled=True)
    prod = x.cpu() * torch.tensor(cin, dtype=torch.float32)
    assert prod.dtype == torch.float32 and torch.equal(xs.cpu(), prod)
    rows = prod.permute(0, 2, 3, 1).reshape(M, 4).half()
    assert torch.equal(two[:M, :4].cpu(), rows) and torch.equal(two[M:, :4].cpu(), rows) and float(two[:, 4:].abs().max()) == 0.0
    single, xs1 = ops.model_input(x, cin, CIN_PAD, dup=1, want_scaled=True)
    assert single.shape == (M, CIN_PAD) and torch.equal(single, two[:M]) and torch.equal(xs1, xs)
    assert torch.equal(ops.model_input(x, cin, CIN_PAD, dup=2)[0], two)
    assert not torch.equal(two, one)


# ---------------------------------------------------------------------------------------------------- trajectories
def start_of(tab, draw):
    """The trajectory's start as HipSampler.sample makes it: init_noise_sigma times the draw, on the device."""
    from sketch2img_amd import ops
    d = draw.to(DEV).contiguous()
    return ops.latent_renoise(d, d, float(np.float32(tab.init_noise_sigma)), 0.0)


def run_steps(sampler, tab, draw, zs):
    """sampler.sample's eager loop with the noise of every step passed in."""
    sampler.unet.prepare_timesteps(tab.timesteps.tolist())
    x = start_of(tab, draw)
    for i in range(len(tab.timesteps)):
        x = sampler.step(x, x, None, tab, i, G, 1.6, z=None if zs is None else zs[i].to(DEV))[0]
    return x


TRAJ = ("trailing", 0)        # the spacing of the trajectory comparisons: see test_leading_euler_is_ddim_in_other_coordinates


def oracle_trajectory(tiny, N, ancestral, vpred, zs):
    """The reference loop written out on the CPU: the oracle UNet on [x c_in] * 2 at the rounded timestep, CFG in fp32, the update in
    float64 from the restated sigmas."""
    from oracle import unet as ounet
    sig, ts, ins = schedule_ref(N, *TRAJ)
    x = (ins * tiny["x0"].double()).float()
    for i, t in enumerate(ts.tolist()):
        s, sn = float(sig[i]), float(sig[i + 1])
        xin = (x.double() / math.sqrt(s * s + 1.0)).float()
        with torch.no_grad():
            eps, _ = ounet.unet_forward(ounet.TINY, tiny["W"], torch.cat([xin, xin]), t, tiny["ehs"])
        eu, ec = eps.float().chunk(2)
        up, down = ancestral_ref(s, sn) if ancestral else (0.0, sn)
        x = euler_step_ref(x.double(), eu.double(), ec.double(), None if zs is None else zs[i].double(), G, s, down, up, vpred)[0].float()
    return x


@pytest.fixture(scope="module")
def others(tiny):
    """The DDIM and DPM-Solver++ results from the same draw (computed once)."""
    from sketch2img_amd.sampler import DDIMTables, DPMTables, HipSampler
    tiny["net"].prepare_context(tiny["ehs"])
    s = HipSampler(tiny["net"], None)
    return [s.sample(tiny["x0"], None, T_T, tables=tb).clone() for tb in (DDIMTables.make(T_T), DPMTables.make(T_T))]


@pytest.mark.parametrize("kind,vpred", [("euler", False), ("euler-a", False), ("euler", True)], ids=["euler", "euler-a", "euler-v"])
def test_trajectory_vs_oracle(tiny, others, kind, vpred):
    """S = 2, 16 x 16 latents, N = 4, trailing spacing (timesteps 999, 749, 499, 249: the trajectory starts at sigma = 14.6); Euler a
    with a given z per step: < 1e-2 relative against the oracle loop, the bound of the project's other 4-step trajectories; two runs
    are bit-equal; sample() is the step loop; the epsilon results are further than that from the DDIM and the DPM-Solver++ result of
    the same draw, and Euler a from Euler."""
    from sketch2img_amd.sampler import HipSampler
    anc = kind == "euler-a"
    tab = make(T_T, anc, *TRAJ, v_prediction=vpred)
    zs = tiny["zs"] if anc else None
    tiny["net"].prepare_context(tiny["ehs"])
    out = run_steps(HipSampler(tiny["net"], None), tab, tiny["x0"], zs)
    assert torch.isfinite(out).all() and torch.equal(out, run_steps(HipSampler(tiny["net"], None), tab, tiny["x0"], zs))
    if not anc:
        assert torch.equal(out, HipSampler(tiny["net"], None).sample(tiny["x0"], None, T_T, tables=tab))
    ref = oracle_trajectory(tiny, T_T, anc, vpred, zs)
    assert report(f"{kind}{' v' if vpred else ''}, 4 steps, vs oracle", out.cpu(), ref)[0] < 1e-2
    far = lambda a: float((a - out).norm() / out.norm())
    if not vpred:
        assert far(others[0]) > 1e-2 and far(others[1]) > 1e-2
    if anc:
        assert far(run_steps(HipSampler(tiny["net"], None), make(T_T, False, *TRAJ), tiny["x0"], None)) > 1e-2


def test_leading_euler_is_ddim_in_other_coordinates(tiny, others):
    """Why the comparisons above use another spacing.  With "leading" spacing and steps_offset 1 the Euler timesteps are DDIM's, and
    the deterministic Euler step is DDIM's in the coordinates x / sqrt(abar): x + (sigma' - sigma) eps = x0 + sigma' eps, times
    sqrt(abar') is sqrt(abar') x0 + sqrt(1 - abar') eps, and the start sqrt(sigma_0^2 + 1) draw is draw / sqrt(abar_0).  Only the
    last step differs - Euler ends at sigma = 0, DDIM at final_alpha_cumprod = abar_0 - so the two results, computed by different
    kernels on differently scaled states, agree within the 1e-2 of the oracle comparisons (measured: 2.3e-3) without being equal:
    an independent check of the whole sigma-space path.  Euler a does not share this."""
    from sketch2img_amd.sampler import DDIMTables, HipSampler
    tab = make(T_T)
    assert np.array_equal(tab.timesteps, DDIMTables.make(T_T).timesteps)
    tiny["net"].prepare_context(tiny["ehs"])
    out = HipSampler(tiny["net"], None).sample(tiny["x0"], None, T_T, tables=tab)
    rel = report("euler, leading spacing, vs the DDIM result", out.cpu(), others[0].cpu())[0]
    assert 0.0 < rel < 1e-2
    anc = run_steps(HipSampler(tiny["net"], None), make(T_T, True), tiny["x0"], tiny["zs"])
    assert float((anc - others[0]).norm() / others[0].norm()) > 1e-2


def test_no_cfg_run(tiny):
    """classifier_free=False: the S cond rows alone, dup = 1 - the CFG run with g = 1 to the GEMM shapes' rounding."""
    from sketch2img_amd.sampler import HipSampler
    S, tab = tiny["S"], make(T_T)
    tiny["net"].prepare_context(tiny["ehs"][S:])
    alone = HipSampler(tiny["net"], None).sample(tiny["x0"], None, T_T, tables=tab, classifier_free=False)
    tiny["net"].prepare_context(tiny["ehs"])
    both = HipSampler(tiny["net"], None).sample(tiny["x0"], None, T_T, 1.0, tables=tab)
    assert torch.isfinite(alone).all() and report("euler without CFG vs g = 1", alone.cpu(), both.cpu())[0] < 1e-2


def test_ancestral_generators_one_draw_per_step_per_sample(tiny):
    """generator=[g0, g1]: sample b's noise is a [1, 4, h, w] draw from its own generator per executed step, the last one included,
    after the initial latents - sample() equals, bit for bit, the step loop fed with those draws and each generator has advanced by
    exactly T draws; a single generator draws [S, 4, h, w] per step; eta is ignored.  Sample b run alone lands on the batch's
    trajectory within the 1e-2 of the oracle comparisons."""
    from sketch2img_amd.sampler import HipSampler
    S, T = tiny["S"], T_T
    tab = make(T, True)
    tiny["net"].prepare_context(tiny["ehs"])
    gens = lambda: [torch.Generator().manual_seed(300 + b) for b in range(S)]
    gs = gens()
    out = HipSampler(tiny["net"], None).sample(tiny["x0"], None, T, tables=tab, generator=gs)
    rs = gens()
    zs = [torch.cat([torch.randn((1, 4, H_T, H_T), generator=r) for r in rs]) for _ in range(T)]
    assert all(torch.equal(g.get_state(), r.get_state()) for g, r in zip(gs, rs))
    assert torch.equal(out, run_steps(HipSampler(tiny["net"], None), tab, tiny["x0"], zs))
    one = torch.Generator().manual_seed(7)
    out1 = HipSampler(tiny["net"], None).sample(tiny["x0"], None, T, tables=tab, generator=one, eta=0.3)
    r = torch.Generator().manual_seed(7)
    zs1 = [torch.randn((S, 4, H_T, H_T), generator=r) for _ in range(T)]
    assert torch.equal(one.get_state(), r.get_state())
    assert torch.equal(out1, run_steps(HipSampler(tiny["net"], None), tab, tiny["x0"], zs1)) and not torch.equal(out1, out)
    b = 1
    tiny["net"].prepare_context(tiny["ehs"][[b, S + b]])
    alone = HipSampler(tiny["net"], None).sample(tiny["x0"][b:b + 1], None, T, tables=tab, generator=[gens()[b]])
    tiny["net"].prepare_context(tiny["ehs"])
    assert report("euler-a sample 1 of the batch vs run alone", out[b:b + 1].cpu(), alone.cpu())[0] < 1e-2
    assert float((out[0:1] - alone).norm() / alone.norm()) > 0.1


@pytest.mark.parametrize("ancestral", [False, True], ids=["euler", "euler-a"])
def test_graph_replay_is_bit_identical(tiny, ancestral):
    """Replay == eager bit for bit (S = 1, 16 x 16, N = 4), the latents and every step's noise from one generator; the same number
    of values is drawn; one graph set serves every seed; zs is [T, S, 4, h, w] for Euler a only; another spacing is another set."""
    from sketch2img_amd.sampler import HipSampler
    net = tiny["net"]
    net.prepare_context(tiny["ehs"][[0, tiny["S"]]])
    tab = make(T_T, ancestral)
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
    assert (ent.zs is not None and tuple(ent.zs.shape) == (T_T, 1, 4, H_T, H_T)) if ancestral else ent.zs is None
    other = make(T_T, ancestral, "trailing", 0)
    a, _ = run(eager, 1, other)
    b, _ = run(graphed, 1, other)
    assert len(graphed._graphs) == 2 and torch.equal(a, b) and not torch.equal(a, outs[1])
    net.prepare_context(tiny["ehs"])


def test_guided_step_measures_its_length_from_the_scaled_input(tiny):
    """TINY LGP, Euler a, one guided step with a given z: aux[2] is sqrt(2) ||x_hat - x_prev|| with x_hat = c_in x the model input
    and x_prev the unguided step's result, recomputed on the CPU to 1e-5 relative - and not the value with x in place of x_hat,
    which is further than 1e-3 away; |update| = alpha ||g|| within 1e-4.  Then a guided 4-step run: finite, guided on steps 0..2."""
    from oracle import lgp as olgp, unet as ounet
    from sketch2img_amd.lgp import HipLGP
    from sketch2img_amd.sampler import HipSampler
    net = tiny["net"]
    net.prepare_context(tiny["ehs"][[0, tiny["S"]]])
    g = torch.Generator().manual_seed(8)
    draw = torch.randn(1, 4, H_T, H_T, generator=g)
    z = torch.randn(1, 4, H_T, H_T, generator=g).to(DEV)
    target = (0.18215 * torch.randn(1, 4, H_T, H_T, generator=g)).to(DEV)
    sd = olgp.init_state_dict(sum(ounet.tap_channels(ounet.TINY)) + 40, seed=12)
    lgp = HipLGP(sd, ounet.tap_channels(ounet.TINY), DEV)
    tab = make(T_T, True)
    net.prepare_timesteps(tab.timesteps.tolist())
    x = start_of(tab, draw)
    guided, aux = HipSampler(net, lgp).step(x, x, target, tab, 0, G, 1.6, z=z)[::2]
    plain, aux0 = HipSampler(net, None).step(x, x, None, tab, 0, G, 1.6, z=z)[::2]
    assert aux0 is None and aux is not None
    x_hat = x.cpu() * torch.tensor(tab.c_in(0), dtype=torch.float32)
    dx = math.sqrt(2.0) * float((x_hat.double() - plain.cpu().double()).norm())
    dx_x = math.sqrt(2.0) * float((x.cpu().double() - plain.cpu().double()).norm())
    upd, want = float((guided - plain).double().norm()), float(aux[0, 0].double() * aux[0, 1].double())
    print(f"[parity] guided euler-a step: aux[2] {float(aux[0, 2]):.6e} sqrt2*|x_hat - x_prev| {dx:.6e} rel {abs(float(aux[0, 2]) / dx - 1):.2e} "
          f"(with x in place of x_hat: {dx_x:.6e}); |update| {upd:.6e} alpha*|g| {want:.6e} rel {abs(upd / want - 1):.2e}")
    assert abs(float(aux[0, 2]) / dx - 1) < 1e-5
    assert abs(dx_x / dx - 1) > 1e-3
    assert abs(upd / want - 1) < 1e-4
    sampler = HipSampler(net, lgp)
    out = sampler.sample(draw, target, T_T, tables=tab, generator=torch.Generator().manual_seed(3))
    assert torch.isfinite(out).all()
    assert [a is not None for a in sampler.last_aux] == [True, True, True, False]
    assert all(torch.isfinite(a).all() for a in sampler.last_aux[:3])
    net.prepare_context(tiny["ehs"])


@pytest.mark.parametrize("ancestral", [False, True], ids=["euler", "euler-a"])
def test_img2img_and_masked_repaint(tiny, ancestral):
    """strength = 0.5 of N = 4: the trajectory starts at init + sigma_2 eps and runs entries 2 and 3 - sample() is latent_renoise plus
    the step loop, bit for bit, and not the from-noise result.  With a mask the kept cells (m = 0) return init bit for bit and the
    repainted ones do not."""
    from sketch2img_amd import ops
    from sketch2img_amd.sampler import HipSampler, start_step
    net, S = tiny["net"], tiny["S"]
    net.prepare_context(tiny["ehs"])
    tab = make(T_T, ancestral)
    k = start_step(T_T, 0.5)
    assert k == 2
    init, eps = (0.8 * rnd(S, 4, H_T, H_T, seed=61)).to(DEV), tiny["x0"].to(DEV)
    seed = lambda: torch.Generator().manual_seed(17)
    out = HipSampler(net, None).sample(eps, None, T_T, tables=tab, init_latents=init, start_step=k, generator=seed())
    r = seed()
    net.prepare_timesteps(tab.timesteps.tolist())
    x, s = ops.latent_renoise(init, eps, *tab.level(k)), HipSampler(net, None)
    assert tab.level(k) == (1.0, float(np.float32(tab.sigmas[k])))
    for i in range(k, T_T):
        x = s.step(x, eps, None, tab, i, G, 1.6, z=torch.randn(S, 4, H_T, H_T, generator=r).to(DEV) if ancestral else None)[0]
    assert torch.isfinite(out).all() and torch.equal(out, x)
    assert not torch.equal(out, HipSampler(net, None).sample(eps, None, T_T, tables=tab, generator=seed()))
    mask = torch.zeros(1, 1, H_T, H_T)
    mask[..., :, H_T // 2:] = 1.0
    rep = HipSampler(net, None).sample(eps, None, T_T, tables=tab, init_latents=init, start_step=k, mask=mask, generator=seed())
    keep = (mask == 0).expand(S, 4, -1, -1).to(DEV)
    assert torch.isfinite(rep).all() and torch.equal(rep[keep], init[keep]) and not torch.equal(rep[~keep], init[~keep])
    assert not torch.equal(rep[~keep], out[~keep])


def test_one_controlnet_step():
    """The ControlNet trunk reads the scaled operand the UNet reads: one Euler step with a control, S = 1, against the CPU
    restatement of the controlled eps on [c_in x] * 2 and the float64 update, < 1e-2; and not the uncontrolled step."""
    from oracle import unet as ounet
    from sketch2img_amd.config import TINY
    from sketch2img_amd.controlnet import Control, ControlNetModel
    from sketch2img_amd.sampler import HipSampler
    from sketch2img_amd.unet import HipUNet
    from tests import controlnet_ref as cref
    W = ounet.init_weights(ounet.TINY)
    cn = ControlNetModel.from_pretrained(None, unet_config=TINY).to(DEV)
    ehs = rnd(2, 77, TINY.cross_attention_dim, seed=8).half().float()
    net = HipUNet(TINY, W, DEV)
    net.prepare_context(ehs)
    cn.hip.prepare_context(ehs)
    h, tab = 16, make(T_T)
    g = torch.Generator().manual_seed(71)
    img = torch.rand(1, 3, 8 * h, 8 * h, generator=g)
    draw = torch.randn(1, 4, h, h, generator=g)
    x = start_of(tab, draw)
    net.prepare_timesteps(tab.timesteps.tolist())
    cn.hip.prepare_timesteps(tab.timesteps.tolist())
    hint = cn.hip.hint_rows(cn.hip.embed(img.to(DEV)), 1, 2)
    got = HipSampler(net, None).step(x, x, None, tab, 0, G, 1.6, control=Control(cn.hip, hint, 0.8, 0.0, 1.0))[0]
    plain = HipSampler(net, None).step(x, x, None, tab, 0, G, 1.6)[0]
    sig, ts, _ = schedule_ref(T_T, "leading", 1)
    s = float(sig[0])
    xin = (x.cpu().double() / math.sqrt(s * s + 1.0)).float()
    with torch.no_grad():
        eu, ec = cref.controlled_eps(ounet.TINY, W, cn.state_dict(), torch.cat([xin, xin]), int(ts[0]), ehs, img, 0.8).chunk(2)
    ref = euler_step_ref(x.cpu().double(), eu.double(), ec.double(), None, G, s, float(sig[1]), 0.0, False)[0]
    assert report("one controlled euler step vs the restatement", got.cpu(), ref.float())[0] < 1e-2
    assert float((got - plain).norm() / plain.norm()) > 1e-2


# ---------------------------------------------------------------------------------------------------- the pipeline
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "pairs"])
def test_pipeline_call_with_each_scheduler_class(dtype):
    """scheduler=EulerDiscreteScheduler(...) / EulerAncestralDiscreteScheduler(...), 3 steps, latents out, both precision modes: the
    sampler's result for the same tables, latents and generator, bit for bit; reproducible per seed; Euler a differs across seeds
    and Euler does not; the two differ from each other and from the DDIM call; guidance_scale = 1 runs without CFG."""
    from modules.pipeline import AntiGradientPipeline
    from sketch2img_amd.config import TINY, UNetConfig
    from sketch2img_amd.sampler import EulerTables, HipSampler
    from sketch2img_amd.schedulers import EulerAncestralDiscreteScheduler, EulerDiscreteScheduler
    cfg = TINY
    if dtype == torch.float32:            # (the pair epilogue needs channel counts that are multiples of 64)
        cfg = UNetConfig(block_out_channels=(64, 128, 128, 128), cross_attention_dim=64, num_heads=(2, 2, 4, 4), norm_groups=8, sample_size=32)
    pipe = AntiGradientPipeline.from_pretrained(None, unet_config=cfg, torch_dtype=dtype).to("cuda")
    assert (pipe.unet.hip.pair_levels > 0) == (dtype == torch.float32)
    h, T = 16, 3
    lat = rnd(1, 4, h, h, seed=9)
    call = dict(negative_prompt="blurry", height=8 * h, width=8 * h, num_inference_steps=T, latents=lat, output_type="latent")
    seeded = lambda n: torch.Generator().manual_seed(n)
    base = pipe("a cat", **call)
    outs = {}
    for cls, anc in ((EulerDiscreteScheduler, False), (EulerAncestralDiscreteScheduler, True)):
        pipe.scheduler = cls(timestep_spacing="leading", steps_offset=1)
        gen = seeded(5)
        out = pipe("a cat", generator=gen, **call)
        assert out.shape == (1, 4, h, h) and torch.isfinite(out).all()
        tab = pipe._tables(T)
        assert isinstance(tab, EulerTables) and tab.ancestral is anc and tab.key() == make(T, anc).key()
        r = seeded(5)
        ref = HipSampler(pipe.unet.hip, None).sample(lat, None, T, 7.5, 1.6, tables=make(T, anc), generator=r)
        assert torch.equal(out, ref) and torch.equal(gen.get_state(), r.get_state())
        assert torch.equal(out, pipe("a cat", generator=seeded(5), **call))
        assert torch.equal(out, pipe("a cat", generator=seeded(6), **call)) is (not anc)
        nocfg = pipe("a cat", guidance_scale=1.0, generator=seeded(5), **call)
        assert torch.isfinite(nocfg).all() and not torch.equal(nocfg, out)
        outs[anc] = out
    pipe.scheduler = EulerDiscreteScheduler()                                  # diffusers' default spacing: "linspace"
    lin = pipe("a cat", **call)
    assert torch.isfinite(lin).all() and pipe._tables(T).timesteps.tolist() == [999, 500, 0]
    assert len({tuple(t.flatten().tolist()[:8]) for t in (base, outs[False], outs[True], lin)}) == 4
