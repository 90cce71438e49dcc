"""CPU tests (-m "not gpu") of DPM-Solver++ 2M with Karras sigmas and of its stochastic variant (sde-dpmsolver++): the schedule
and both coefficient sets against the float64 restatement of tests/dpm_ref.py (diffusers' sigma-based formulation with
final_sigmas_type="zero"), the scheduler selection of the pipeline, the hipGraph cache key and the new C entry point's argument
checks.  No kernel is launched here."""
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.dpm_ref import U32, karras_ref, ode_ref, orders, sde_ref, source_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------ unchanged defaults
def test_defaults_are_unchanged():
    """(Passes before the feature too: the deterministic uniform path keeps its bits.)"""
    from oracle import dpmsolver as odpm
    from sketch2img_amd.sampler import DPMTables
    for N in (3, 10, 25):
        a, b = DPMTables.make(N), odpm.make_tables(N)
        assert np.array_equal(a.timesteps, b.timesteps) and a.timesteps.dtype == np.int64
        for f in ("alphas_cumprod", "alpha_t", "sigma_t", "lambda_t"):
            assert torch.equal(getattr(a, f), getattr(b, f)), f
        for i, od in enumerate(orders(a)):
            c = a.coeffs(i, od)
            assert len(c) == 5 and c == odpm.step_coeffs(b, i, od)
    assert orders(DPMTables.make(10)) == [1] + [2] * 8 + [1] and orders(DPMTables.make(16)) == [1] + [2] * 15


def test_new_fields_default_to_todays_schedule():
    from sketch2img_amd.sampler import DPMTables
    t = DPMTables.make(10)
    assert t.use_karras_sigmas is False and t.algorithm_type == "dpmsolver++" and t.sigmas is None and not t.stochastic
    e = DPMTables.make(10, use_karras_sigmas=False, algorithm_type="dpmsolver++")
    assert np.array_equal(t.timesteps, e.timesteps) and torch.equal(t.lambda_t, e.lambda_t)
    assert [t.coeffs(i, o) for i, o in enumerate(orders(t))] == [e.coeffs(i, o) for i, o in enumerate(orders(e))]
    with pytest.raises(NotImplementedError):
        DPMTables.make(10, algorithm_type="dpmsolver")


# ------------------------------------------------------------------------------------------ the Karras schedule
def test_karras_known_values():
    from sketch2img_amd.sampler import DPMTables
    t = DPMTables.make(10, use_karras_sigmas=True)
    assert t.timesteps.tolist() == [999, 916, 815, 687, 523, 327, 146, 41, 7, 0] and t.timesteps.dtype == np.int64
    assert abs(t.sigmas[0] - 14.6146) < 1e-4 and abs(t.sigmas[9] - 0.029167) < 1e-6 and t.sigmas[10] == 0.0
    for N in range(2, 31):
        ts = DPMTables.make(N, use_karras_sigmas=True).timesteps
        assert len(set(ts.tolist())) == N, N
    assert DPMTables.make(50, use_karras_sigmas=True).timesteps.tolist()[-6:] == [6, 4, 2, 1, 1, 0]


@pytest.mark.parametrize("N", [1, 2, 10, 25, 50])
def test_karras_schedule_vs_float64(N):
    from sketch2img_amd.sampler import DPMTables
    t = DPMTables.make(N, use_karras_sigmas=True)
    sig, ts = karras_ref(N)
    assert np.array_equal(t.timesteps, ts)
    assert t.sigmas.shape == (N + 1,) and t.sigmas[N] == 0.0
    # the schedule is kept in float64 (a few float64 roundings of a seventh power); what reaches a kernel is cast at the end
    assert np.all(np.abs(t.sigmas[:N] - sig) <= 64 * np.finfo(np.float64).eps * sig)
    assert np.all(np.diff(t.sigmas) < 0)
    if N == 1:
        assert abs(t.sigmas[0] - 14.6146) < 1e-4 and t.timesteps.tolist() == [999]
    # alpha_s / sigma_s as the kernel receives them: one fp32 cast of the float64 value
    src = source_ref(t, True, N)
    for i, od in enumerate(orders(t)):
        al, sg = t.coeffs(i, od)[:2]
        assert al == float(np.float32(al)) and sg == float(np.float32(sg))
        assert abs(al - src[i][0]) <= 1.01 * U32 * src[i][0] and abs(sg - src[i][1]) <= 1.01 * U32 * src[i][1]


@pytest.mark.parametrize("N", [2, 4, 16, 25])
def test_karras_ode_coeffs_vs_float64(N):
    """a, b, c from the sigmas: one fp32 cast of a float64 value (b and c are sums / quotients of O(1) terms without cancellation
    beyond 1 - e^-h, which the implementation may evaluate with expm1: 8 float64 ulps of slack on top of the cast)."""
    from sketch2img_amd.sampler import DPMTables
    t = DPMTables.make(N, use_karras_sigmas=True)
    src = source_ref(t, True, N)
    od = orders(t)
    assert od == ([1] + [2] * (N - 2) + [1] if N > 1 else [1])
    for i in range(N - 1):
        got, want = t.coeffs(i, od[i])[2:], ode_ref(src, i, od[i])
        for g, w in zip(got, want):
            assert abs(g - w) <= 1.01 * U32 * abs(w) + 1e-14, (N, i, got, want)


@pytest.mark.parametrize("N", [1, 4, 10, 16, 25])
@pytest.mark.parametrize("algo", ["dpmsolver++", "sde-dpmsolver++"])
def test_final_step(N, algo):
    """Karras: the last step goes to sigma = 0, is first order and is x_prev = x0 exactly, for N < 15 and N >= 15 alike.
    Uniform: today's rule (first order only below 15 steps), final target t = 0."""
    from sketch2img_amd.sampler import DPMTables
    k = DPMTables.make(N, use_karras_sigmas=True, algorithm_type=algo)
    assert orders(k)[-1] == 1
    assert k.coeffs(N - 1, 1)[2:] == (0.0, 1.0, 0.0)
    assert k.coeffs_sde(N - 1, 1)[2:] == (0.0, 1.0, 0.0, 0.0)
    assert all(math.isfinite(v) for v in k.coeffs(N - 1, 1) + k.coeffs_sde(N - 1, 1))
    u = DPMTables.make(N, algorithm_type=algo)
    assert orders(u)[-1] == (1 if N < 15 else 2)
    assert orders(u) == orders(DPMTables.make(N))
    assert orders(DPMTables.make(N, lower_order_final=False, use_karras_sigmas=True))[-1] == 1


# ------------------------------------------------------------------------------------------ the SDE coefficients
@pytest.mark.parametrize("karras", [False, True])
@pytest.mark.parametrize("N", [4, 16, 25])
def test_sde_marginal_identities(N, karras):
    """x_prev = a x + b x0 + c x0_before + d z keeps the schedule's marginal: with x = alpha_s x0 + sigma_s e and x0_before = x0,
        a alpha_s + b + c = alpha_t          a^2 sigma_s^2 + d^2 = sigma_t^2.
    In the float64 restatement to float64 rounding (1e-13 of the largest term: about ten operations, exp and sqrt among them).  In
    the fp32 scalars the implementation returns, each scalar is ONE cast of a float64 value (relative U32 = 2^-24), so evaluated in
    float64 the first identity is off by at most U32 (|a alpha_s| * 2 + |b| + |c|) and the second by U32 (4 a^2 sigma_s^2 +
    2 d^2) (a product of two cast values carries two casts, a square of a cast value two) - plus the float64 error above."""
    from sketch2img_amd.sampler import DPMTables
    t = DPMTables.make(N, use_karras_sigmas=karras, algorithm_type="sde-dpmsolver++")
    src = source_ref(t, karras, N)
    od = orders(t)
    assert set(od) == {1, 2}
    worst = [0.0, 0.0]
    for i in range(N):
        for order in {od[i], 1} if i > 0 else {1}:                  # (both orders wherever a history exists)
            if karras and i == N - 1:
                if order == 1:
                    assert t.coeffs_sde(i, 1)[5] == 0.0
                continue
            al_t, sg_t = src[i + 1][0], src[i + 1][1]
            a, b, c, d = sde_ref(src, i, order)
            big1, big2 = max(abs(a * src[i][0]), abs(b), abs(c)), max(a * a * src[i][1] ** 2, d * d)
            assert abs(a * src[i][0] + b + c - al_t) < 1e-13 * big1
            assert abs(a * a * src[i][1] ** 2 + d * d - sg_t ** 2) < 1e-13 * big2
            got = t.coeffs_sde(i, order)
            assert len(got) == 6 and all(isinstance(v, float) and v == float(np.float32(v)) for v in got)
            als, sgs, ga, gb, gc, gd = got
            for g, w in zip((als, sgs, ga, gb, gc, gd), (src[i][0], src[i][1], a, b, c, d)):
                assert abs(g - w) <= 1.01 * U32 * abs(w) + 1e-14, (N, karras, i, order, got)
            assert (gc == 0.0) == (order == 1) and gd > 0.0
            e1 = abs(ga * als + gb + gc - al_t)
            e2 = abs(ga * ga * sgs * sgs + gd * gd - sg_t ** 2)
            b1 = U32 * (2 * abs(ga * als) + abs(gb) + abs(gc)) * 1.01 + 1e-13 * big1
            b2 = U32 * (4 * ga * ga * sgs * sgs + 2 * gd * gd) * 1.01 + 1e-13 * big2
            worst = [max(worst[0], e1 / b1), max(worst[1], e2 / b2)]
            assert e1 <= b1 and e2 <= b2, (N, karras, i, order, e1, b1, e2, b2)
    print(f"[parity] sde marginals N {N} karras {karras}: worst error / bound {worst[0]:.3f} {worst[1]:.3f}")


@pytest.mark.parametrize("karras", [False, True])
def test_ode_and_sde_read_the_same_source(karras):
    """Different solvers, one schedule: alpha_s, sigma_s are the same floats.  Under Karras both take (alpha, sigma_hat, lambda) -
    hence h - from DPMTables.source.  On the uniform schedule alpha and sigma_hat are the fp32 table entries at the integer
    timesteps for both; the deterministic coeffs keep the table's fp32 lambda_t (bit-equal to the oracle), the SDE's lambda is
    log alpha - log sigma_hat of the same two entries in float64, which lambda_t equals to the rounding of its three fp32
    operations (two logs, one difference: 3 * 2^-23 of the largest of the three magnitudes)."""
    from sketch2img_amd.sampler import DPMTables
    N = 10
    o = DPMTables.make(N, use_karras_sigmas=karras)
    s = DPMTables.make(N, use_karras_sigmas=karras, algorithm_type="sde-dpmsolver++")
    assert s.stochastic and not o.stochastic and np.array_equal(o.timesteps, s.timesteps)
    src = source_ref(o, karras, N)
    for i, od in enumerate(orders(o)):
        assert o.coeffs(i, od)[:2] == s.coeffs_sde(i, od)[:2]
        assert o.coeffs_sde(i, od) == s.coeffs_sde(i, od) and o.coeffs(i, od) == s.coeffs(i, od)
        for tab in (o, s):
            for j in (i, i + 1):
                got = tab.source(j)
                assert all(g == w or abs(g - w) <= 64 * np.finfo(np.float64).eps * abs(w) for g, w in zip(got, src[j])), (j, got, src[j])
    if not karras:
        for j in range(N + 1):
            t = 0 if j == N else int(o.timesteps[j])
            al, sg, lam = o.source(j)
            assert al == float(o.alpha_t[t]) and sg == float(o.sigma_t[t])
            assert abs(lam - float(o.lambda_t[t])) <= 3 * 2.0 ** -23 * max(abs(math.log(al)), abs(math.log(sg)), abs(lam))


# ------------------------------------------------------------------------------------------ pipeline, graph key, C entry point
def test_pipeline_tables_read_karras_and_algorithm_type():
    from sketch2img_amd.modules.pipeline import AntiGradientPipeline
    from sketch2img_amd.sampler import DPMTables
    from sketch2img_amd.schedulers import DPMSolverMultistepScheduler
    p = AntiGradientPipeline.__new__(AntiGradientPipeline)
    p.scheduler = DPMSolverMultistepScheduler(use_karras_sigmas=True)
    assert p.scheduler.config.use_karras_sigmas is True
    t = p._tables(10)
    assert isinstance(t, DPMTables) and t.use_karras_sigmas and not t.stochastic
    assert t.timesteps.tolist() == [999, 916, 815, 687, 523, 327, 146, 41, 7, 0]
    p.scheduler = DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++")
    t = p._tables(10)
    assert t.stochastic and not t.use_karras_sigmas and np.array_equal(t.timesteps, DPMTables.make(10).timesteps)
    p.scheduler = DPMSolverMultistepScheduler(use_karras_sigmas=True, algorithm_type="sde-dpmsolver++")
    t = p._tables(25)
    assert t.stochastic and t.use_karras_sigmas and len(t.timesteps) == 25
    p.scheduler = DPMSolverMultistepScheduler()
    t = p._tables(10)
    assert not t.stochastic and not t.use_karras_sigmas and t.sigmas is None
    # a diffusers-style object: the options sit in .config
    s = type("DPMSolverMultistepScheduler", (), {})()
    s.config = SimpleNamespace(algorithm_type="sde-dpmsolver++", solver_type="midpoint", use_karras_sigmas=True, final_sigmas_type="zero",
                               use_lu_lambdas=False, euler_at_final=False)
    p.scheduler = s
    assert p._tables(10).stochastic and p._tables(10).use_karras_sigmas
    for bad in (dict(algorithm_type="dpmsolver"), dict(algorithm_type="sde-dpmsolver"), dict(solver_type="heun"),
                dict(algorithm_type="sde-dpmsolver++", solver_type="heun"), dict(thresholding=True),
                dict(use_karras_sigmas=True, thresholding=True), dict(use_lu_lambdas=True)):
        p.scheduler = DPMSolverMultistepScheduler(**bad)
        with pytest.raises(NotImplementedError):
            p._tables(25)


def test_graph_key_separates_spacing_and_algorithm():
    from sketch2img_amd.sampler import DPMTables, graph_key
    base = dict(shape=(1, 4, 16, 16), unguided=True, guidance_scale=7.5, beta=1.6, share_cfg_prefix=True)
    mk = lambda **kw: graph_key(DPMTables.make(4, **kw), **base)
    u, k = mk(), mk(use_karras_sigmas=True)
    us, ks = mk(algorithm_type="sde-dpmsolver++"), mk(use_karras_sigmas=True, algorithm_type="sde-dpmsolver++")
    assert len({u, k, us, ks}) == 4
    assert u == mk() and ks == mk(use_karras_sigmas=True, algorithm_type="sde-dpmsolver++") and hash(ks) == hash(mk(use_karras_sigmas=True, algorithm_type="sde-dpmsolver++"))
    # the per-step sigmas themselves are in the key, not only the flag
    t = DPMTables.make(4, use_karras_sigmas=True)
    t2 = DPMTables.make(4, use_karras_sigmas=True)
    t2.sigmas = t2.sigmas * (1.0 + 1e-6)
    assert graph_key(t, **base) != graph_key(t2, **base)
    assert tuple(float(s) for s in t.sigmas) in graph_key(t, **base)


def test_sampler_validates_generators_for_sde_before_any_launch():
    from sketch2img_amd.sampler import DPMTables, HipSampler, draws_noise
    s = HipSampler(SimpleNamespace(dev="cpu", inject=None), None)
    x = torch.zeros(2, 4, 8, 8)
    tab = DPMTables.make(2, algorithm_type="sde-dpmsolver++")
    with pytest.raises(ValueError, match="list of generators of length"):
        s.sample(x, None, 2, tables=tab, generator=[torch.Generator()])
    assert draws_noise(tab, 0.0) and not draws_noise(DPMTables.make(2), 0.7)


def test_sde_entry_point_is_declared_bound_exported_and_checks_its_arguments():
    """skg_cfg_dpmpp2m_sde_step: skg_cfg_dpmpp2m_step's argument list plus `z` after `x` and `d` after `c`, the same preconditions
    plus z != NULL, all refused (SKG_E_BADARG) before any HIP call; an additive symbol, ABI version 6."""
    import subprocess
    from sketch2img_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "skg.h")).read()
    m = re.search(r"\bint\s+skg_cfg_dpmpp2m_sde_step\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
    assert m is not None
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    letters = "".join("p" if "*" in a else "f" if a.startswith("float") else "i" for a in args)
    assert _lib.SIGNATURES["skg_cfg_dpmpp2m_sde_step"] == ("i", letters)
    det = _lib.SIGNATURES["skg_cfg_dpmpp2m_step"][1]
    assert letters == det[:5] + "p" + det[5:16] + "f" + det[16:] == "ppiipppppiifffffffip"
    assert "const float* z" in args and "float d" in args
    assert re.search(r"#define\s+SKG_ABI_VERSION\s+6\b", hdr) and _lib.ABI_VERSION == 6 and _lib.lib.skg_abi_version() == 6
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r" T skg_cfg_dpmpp2m_sde_step\b", nm)
    f = _lib.lib.skg_cfg_dpmpp2m_sde_step

    def call(x=16, z=16, x0=16, xp=16, ld=8, lo_off=0, samples=1, HW=4, alpha_s=0.5, vpred=0):
        return f(16, 16, ld, lo_off, x, z, x0, xp, None, samples, HW, 7.5, alpha_s, 0.8, 0.5, 0.4, -0.1, 0.3, vpred, None)

    assert call(z=None) == -1 and call(x=None) == -1 and call(x0=None) == -1 and call(xp=None) == -1
    assert call(HW=0) == -1 and call(HW=-3) == -1 and call(samples=0) == -1
    assert call(ld=3) == -1 and call(ld=8, lo_off=8) == -1 and call(lo_off=-1) == -1
    assert call(vpred=2) == -1 and call(alpha_s=0.0) == -1
