"""CPU tests (-m "not gpu") of the Euler and Euler-ancestral samplers: EulerTables against the float64 restatement of
tests/euler_ref.py and against anchor values, the fractional "linspace" timesteps, the ancestral split of sigma_next, the
hipGraph cache key, the scheduler selection of the pipeline with every rejected option, the img2img levels, and the argument
checks of the two C entry points.  No kernel is launched here."""
import dataclasses
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.euler_ref import U32, ancestral_ref, schedule_ref, sd_alphas_cumprod, step_scalars_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-6                                                   # the issue's agreement with the anchors
SPACINGS = [("leading", 1), ("trailing", 0), ("linspace", 0)]


def close(got, want, rel=REL):
    return abs(got - want) <= rel * abs(want)


def printed(got, text):
    """An anchor given with fewer than seven digits: 1e-6 relative on top of half a unit of its last printed digit."""
    want = float(text)
    return abs(got - want) <= REL * abs(want) + 0.5 * 10.0 ** -len(text.split(".")[1])


def make(N, spacing="leading", off=1, **kw):
    from sketch2img_amd.sampler import EulerTables
    return EulerTables.make(N, timestep_spacing=spacing, steps_offset=off, **kw)


# ------------------------------------------------------------------------------------------ the schedule
def test_anchor_values():
    """N = 10, computed from the fp32 alphas_cumprod table."""
    lead, trail, lin = (make(10, sp, off, ancestral=True) for sp, off in SPACINGS)
    assert lead.timesteps.tolist() == list(range(901, 0, -100)) and lead.timesteps.dtype == np.int64
    assert trail.timesteps.tolist() == list(range(999, 98, -100))
    assert lin.timesteps.tolist() == list(range(999, -1, -111))
    for tab, s0, s1 in ((lead, "8.39069", "5.13443"), (trail, "14.6146", "8.30281"), (lin, "14.6146", "7.83989")):
        assert printed(tab.sigmas[0], s0) and printed(tab.sigmas[1], s1)
        assert tab.sigmas.shape == (11,) and tab.sigmas[10] == 0.0 and tab.sigmas.dtype == np.float64
    assert printed(lead.sigmas[9], "0.0413145")
    assert close(lead.init_noise_sigma, 8.450067) and close(trail.init_noise_sigma, 14.614647) and close(lin.init_noise_sigma, 14.614647)
    for tab, (up, down) in ((lead, (4.060922, 3.141865)), (trail, (6.832785, 4.716952))):
        got = tab.sigma_up_down(0)
        assert close(got[0], up) and close(got[1], down)
    k = make(10, use_karras_sigmas=True)
    assert k.timesteps.tolist() == [901, 815, 711, 582, 427, 260, 121, 40, 9, 1]
    assert printed(k.sigmas[1], "5.4777") and k.sigmas[0] == lead.sigmas[0] and close(k.sigmas[9], lead.sigmas[9], 1e-12)
    assert close(k.init_noise_sigma, 8.450067)


@pytest.mark.parametrize("karras", [False, True])
@pytest.mark.parametrize("spacing,off", SPACINGS)
@pytest.mark.parametrize("N", [2, 7, 10, 25, 50])
def test_schedule_vs_float64_restatement(N, spacing, off, karras):
    tab = make(N, spacing, off, use_karras_sigmas=karras)
    sig, its, ins = schedule_ref(N, spacing, off, karras)
    assert np.array_equal(tab.timesteps, its) and tab.timesteps.dtype == np.int64
    assert tab.sigmas.shape == (N + 1,) and tab.sigmas[N] == 0.0
    assert np.all(np.abs(tab.sigmas[:N] - sig[:N]) <= REL * sig[:N])
    assert np.all(np.diff(tab.sigmas) < 0)
    assert close(tab.init_noise_sigma, ins)
    assert torch.equal(tab.alphas_cumprod, sd_alphas_cumprod())
    for i in range(N):
        s = float(sig[i])
        assert close(tab.c_in(i), 1.0 / math.sqrt(s * s + 1.0), 1.01 * U32 + 1e-10)
        assert tab.c_in(i) == float(np.float32(tab.c_in(i)))


def test_linspace_timesteps_are_fractional_and_the_unet_runs_at_the_rounded_ones():
    """N = 7: step 166.5.  The sigmas are the table interpolated at 999, 832.5, 666, 499.5, 333, 166.5, 0 - midway between two
    table entries at the half-integers - and the UNet timesteps their roundings (half to even)."""
    tab = make(7, "linspace", 0)
    acp = sd_alphas_cumprod().double().numpy()
    table = np.sqrt((1 - acp) / acp)
    assert tab.timesteps.tolist() == [999, 832, 666, 500, 333, 166, 0]
    want = [table[999], 0.5 * (table[832] + table[833]), table[666], 0.5 * (table[499] + table[500]), table[333],
            0.5 * (table[166] + table[167]), table[0]]
    assert np.all(np.abs(tab.sigmas[:7] - np.array(want)) <= 1e-12 * np.array(want))
    assert not close(tab.sigmas[1], table[832], 1e-4) and not close(tab.sigmas[1], table[833], 1e-4)
    # the integer spacings sit on the table
    for sp, off in SPACINGS[:2]:
        t = make(7, sp, off)
        assert np.array_equal(t.sigmas[:7], table[t.timesteps])


@pytest.mark.parametrize("karras", [False, True])
@pytest.mark.parametrize("spacing,off", SPACINGS)
def test_ancestral_split_and_step_scalars(spacing, off, karras):
    """sigma_up^2 + sigma_down^2 = sigma_next^2 on every step, both 0 on the last one; the five kernel scalars are one fp32 cast
    of the float64 values of the restatement, for both prediction types; Euler has sigma_up = 0 and dt = sigma_next - sigma."""
    N = 10
    sig = schedule_ref(N, spacing, off, karras)[0]
    for anc in (False, True):
        for vp in (False, True):
            tab = make(N, spacing, off, use_karras_sigmas=karras, ancestral=anc, v_prediction=vp)
            assert tab.noisy(0.0) is anc and tab.noisy(0.7) is anc and tab.has_eta is False and tab.new_history(torch.zeros(1)) is None
            for i in range(N):
                s, to, up = step_scalars_ref(sig, i, anc)
                got = tab.coeffs(i)
                assert all(v == float(np.float32(v)) for v in got) and len(got) == 5
                kx, km = (1.0 / (s * s + 1.0), -s / math.sqrt(s * s + 1.0)) if vp else (1.0, -s)
                for g, w in zip(got, (s, kx, km, to - s, up)):
                    assert g == w == 0.0 or close(g, w, 1.01 * U32 + 1e-10), (i, got)
                if not vp:
                    assert got[1] == 1.0 and got[2] == -got[0]
                if anc:
                    u, d = tab.sigma_up_down(i)
                    sn = float(tab.sigmas[i + 1])
                    assert abs(u * u + d * d - sn * sn) <= 1e-12 * sn * sn
                    assert (u, d) == (0.0, 0.0) if i == N - 1 else (0.0 < u < sn and 0.0 < d < sn)
                    ru, rd = ancestral_ref(float(sig[i]), float(sig[i + 1]))
                    assert (u == ru == 0.0 or close(u, ru)) and (d == rd == 0.0 or close(d, rd))
                else:
                    assert got[4] == 0.0
            assert tab.coeffs(N - 1)[3] == -tab.coeffs(N - 1)[0] and tab.coeffs(N - 1)[4] == 0.0


def test_levels_and_start_step_for_img2img():
    """level(j) = (1, sigma_j) as fp32 floats - the Euler schedulers' add_noise - and (1, 0) at the clean end; sigma(t) stays the
    noise-level factor sqrt(1 - abar_t) at the integer timestep."""
    from sketch2img_amd.sampler import DDIMTables, start_step
    tab = make(10, "linspace", 0, ancestral=True)
    for j in range(10):
        assert tab.level(j) == (1.0, float(np.float32(tab.sigmas[j])))
    assert tab.level(10) == (1.0, 0.0)
    k = start_step(10, 0.5)
    assert k == 5 and tab.level(k)[1] == float(np.float32(tab.sigmas[5]))
    d = DDIMTables.make(10)
    for t in (0, 166, 999):
        assert tab.sigma(t) == d.sigma(t) == float((1 - sd_alphas_cumprod()[t]) ** 0.5)
    assert tab.sigma(999) < 1.0 < tab.sigmas[0]


def test_unknown_spacing_is_refused():
    with pytest.raises(NotImplementedError):
        make(10, "karras", 0)


# ------------------------------------------------------------------------------------------ keys
def test_key_changes_with_every_field():
    from sketch2img_amd.sampler import EulerTables, graph_key
    tab = make(4)
    other = dict(alphas_cumprod=EulerTables.make(4, beta_end=0.02).alphas_cumprod, timesteps=tab.timesteps + 1,
                 sigmas=tab.sigmas * (1.0 + 1e-6), init_noise_sigma=tab.init_noise_sigma + 1.0, ancestral=True, v_prediction=True)
    k0 = tab.key()
    assert k0 == dataclasses.replace(tab).key() == make(4).key() and hash(k0) == hash(make(4).key()) and k0[0] == "EulerTables"
    for f in dataclasses.fields(tab):
        k = dataclasses.replace(tab, **{f.name: other[f.name]}).key()       # (a field added later has no entry: KeyError)
        hash(k)
        assert k != k0, f.name
    base = dict(shape=(1, 4, 16, 16), unguided=True, guidance_scale=7.5, beta=1.6, share_cfg_prefix=True)
    keys = {graph_key(make(4, sp, off, use_karras_sigmas=ka, ancestral=an), **base) for sp, off in SPACINGS for ka in (False, True)
            for an in (False, True)}
    assert len(keys) == 12 and all(v in graph_key(tab, **base) for v in k0)


def test_ddim_and_dpm_keys_are_unchanged():
    """The literal keys of the two existing tables classes for N = 4: the feature adds no field to them."""
    from sketch2img_amd.sampler import DDIMTables, DPMTables, _fingerprint
    d, p = DDIMTables.make(4), DPMTables.make(4, use_karras_sigmas=True, algorithm_type="sde-dpmsolver++")
    fp = _fingerprint(sd_alphas_cumprod())
    assert d.key() == ("DDIMTables", (751, 501, 251, 1), False, float(sd_alphas_cumprod()[0]), 250) + fp
    assert p.key() == ("DPMTables", tuple(int(t) for t in p.timesteps), False, 2, True, True, "sde-dpmsolver++",
                       tuple(float(s) for s in p.sigmas)) + fp
    assert [f.name for f in dataclasses.fields(d)] == ["alphas_cumprod", "final_alpha_cumprod", "timesteps", "ratio", "v_prediction"]
    assert [f.name for f in dataclasses.fields(p)] == ["alphas_cumprod", "alpha_t", "sigma_t", "lambda_t", "timesteps", "lower_order_final",
                                                       "solver_order", "v_prediction", "use_karras_sigmas", "algorithm_type", "sigmas"]
    assert d.scales_input is False and p.scales_input is False and make(4).scales_input is True
    # the Karras DPM schedule still runs between the ends of the full table
    assert DPMTables.make(10, use_karras_sigmas=True).timesteps.tolist() == [999, 916, 815, 687, 523, 327, 146, 41, 7, 0]


# ------------------------------------------------------------------------------------------ the pipeline's scheduler selection
def _pipe():
    from sketch2img_amd.modules.pipeline import AntiGradientPipeline
    return AntiGradientPipeline.__new__(AntiGradientPipeline)


def test_pipeline_tables_for_both_scheduler_classes():
    from sketch2img_amd.sampler import EulerTables
    from sketch2img_amd.schedulers import EulerAncestralDiscreteScheduler, EulerDiscreteScheduler
    p = _pipe()
    p.scheduler = EulerDiscreteScheduler()
    t = p._tables(10)
    assert isinstance(t, EulerTables) and not t.ancestral and not t.v_prediction
    assert t.key() == make(10, "linspace", 0).key()                                  # diffusers' constructor defaults
    p.scheduler = EulerDiscreteScheduler(timestep_spacing="leading", steps_offset=1, use_karras_sigmas=True, prediction_type="v_prediction")
    assert p._tables(10).key() == make(10, "leading", 1, use_karras_sigmas=True, v_prediction=True).key()
    p.scheduler = EulerAncestralDiscreteScheduler(timestep_spacing="trailing")
    t = p._tables(10)
    assert t.ancestral and t.key() == make(10, "trailing", 0, ancestral=True).key()
    p.scheduler = EulerAncestralDiscreteScheduler(timestep_spacing="leading", steps_offset=1, use_karras_sigmas=True)
    assert p._tables(10).key() == make(10, "leading", 1, use_karras_sigmas=True, ancestral=True).key()
    p.scheduler = EulerDiscreteScheduler(beta_end=0.02)
    assert p._tables(10).key() != make(10, "linspace", 0).key()
    # real diffusers objects are recognised by class name; only .config is read
    for name, anc in (("EulerDiscreteScheduler", False), ("EulerAncestralDiscreteScheduler", True)):
        s = type(name, (), {})()
        s.config = SimpleNamespace(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                                   trained_betas=None, prediction_type="epsilon", timestep_spacing="leading", steps_offset=1,
                                   rescale_betas_zero_snr=False)
        p.scheduler = s
        assert p._tables(10).key() == make(10, "leading", 1, ancestral=anc).key()
        s.config = dict(vars(s.config))
        assert p._tables(10).key() == make(10, "leading", 1, ancestral=anc).key()
        # the spacing decides where the trajectory starts and has two plausible defaults: a config that does not state it is refused
        s.config = {k: v for k, v in s.config.items() if k != "timestep_spacing"}
        with pytest.raises(NotImplementedError, match="timestep_spacing"):
            p._tables(10)
    p.scheduler = EulerDiscreteScheduler()
    p.get_noise_level(torch.ones(1, 4, 2, 2), 10)


REJECTED = [dict(beta_schedule="linear"), dict(beta_schedule="squaredcos_cap_v2"), dict(trained_betas=[0.1, 0.2]),
            dict(interpolation_type="log_linear"), dict(sigma_min=0.03), dict(sigma_max=14.0), dict(timestep_type="continuous"),
            dict(rescale_betas_zero_snr=True), dict(use_exponential_sigmas=True), dict(use_beta_sigmas=True),
            dict(final_sigmas_type="sigma_min"), dict(prediction_type="sample"), dict(timestep_spacing="uniform")]


@pytest.mark.parametrize("bad", REJECTED, ids=lambda d: next(iter(d)))
def test_every_rejected_option_raises(bad):
    """Refused by the configuration class and - for an object that carries the option in its .config, as a diffusers scheduler
    does - by the pipeline: never ignored."""
    from sketch2img_amd.schedulers import EulerAncestralDiscreteScheduler, EulerDiscreteScheduler
    p = _pipe()
    for cls in (EulerDiscreteScheduler, EulerAncestralDiscreteScheduler):
        with pytest.raises(NotImplementedError):
            cls(**bad)
        s = type(cls.__name__, (), {})()
        s.config = SimpleNamespace(**dict(vars(cls().config), **bad))
        p.scheduler = s
        with pytest.raises(NotImplementedError):
            p._tables(10)


def test_sampler_validates_generators_for_ancestral_before_any_launch():
    from sketch2img_amd.sampler import HipSampler, draws_noise
    s = HipSampler(SimpleNamespace(dev="cpu", inject=None), None)
    with pytest.raises(ValueError, match="list of generators of length"):
        s.sample(torch.zeros(2, 4, 8, 8), None, 2, tables=make(2, ancestral=True), generator=[torch.Generator()])
    assert draws_noise(make(2, ancestral=True), 0.0) and not draws_noise(make(2), 0.7)


# ------------------------------------------------------------------------------------------ the C entry points
def _declared(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
    assert m is not None, name
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    return args, "".join("p" if "*" in a else "f" if a.startswith("float") else "i" for a in args)


def test_entry_points_are_declared_bound_exported_and_check_their_arguments():
    """skg_model_input and skg_cfg_euler_step: the signature table matches the header, both are exported, ABI version 6 stands,
    and every precondition is refused (SKG_E_BADARG) before any HIP call - z = NULL with sigma_up != 0 among them."""
    import subprocess
    from sketch2img_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "skg.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in ("skg_model_input", "skg_cfg_euler_step"):
        args, letters = _declared(hdr, name)
        assert _lib.SIGNATURES[name] == ("i", letters) and re.search(r" T " + name + r"\b", nm)
    assert "const float* z" in _declared(hdr, "skg_cfg_euler_step")[0] and "float* x_scaled" in _declared(hdr, "skg_model_input")[0]
    assert re.search(r"#define\s+SKG_ABI_VERSION\s+6\b", hdr) and _lib.ABI_VERSION == 6 and _lib.lib.skg_abi_version() == 6
    f = _lib.lib.skg_cfg_euler_step

    def step(eu=16, x=16, z=16, xp=16, ld=8, lo_off=0, samples=1, HW=4, sigma=2.0, up=0.5):
        return f(eu, 16, ld, lo_off, x, z, xp, None, samples, HW, 7.5, sigma, 1.0, -sigma, -0.5, up, None)

    assert step(z=None) == -1 and step(z=None, up=-0.5) == -1 and step(up=-0.5) == -1
    assert step(eu=None) == -1 and step(x=None) == -1 and step(xp=None) == -1
    assert step(HW=0) == -1 and step(HW=-3) == -1 and step(samples=0) == -1 and step(sigma=0.0) == -1
    assert step(ld=3) == -1 and step(ld=8, lo_off=8) == -1 and step(lo_off=-1) == -1
    m = _lib.lib.skg_model_input

    def minput(x=16, y=16, samples=1, C=4, HW=4, Cpad=32, dup=2):
        return m(x, y, None, samples, C, HW, Cpad, dup, 0.5, None)

    assert minput(x=None) == -1 and minput(y=None) == -1 and minput(samples=0) == -1 and minput(HW=0) == -1 and minput(C=0) == -1
    assert minput(Cpad=3) == -1 and minput(dup=0) == -1 and minput(dup=3) == -1
