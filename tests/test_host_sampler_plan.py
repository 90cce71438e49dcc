"""CPU tests (-m "not gpu") of the sampler's structure: every field of the options record and of a scheduler's tables is in the
graph-set key, each scheduler's update() issues the step kernel and coefficients the sampler's type ladder used to pick, and the
step runner gives the eager loop and a graph set's warm-up pass the same control window and blend levels.  No kernel is launched."""
import dataclasses
from types import SimpleNamespace

import numpy as np
import pytest
import torch

STEP_OPS = ("cfg_ddim_step", "cfg_ddim_eta_step", "cfg_dpmpp2m_step", "cfg_dpmpp2m_sde_step")
SDE = "sde-dpmsolver++"


def _control(start=0.25, end=0.75, scale=1.0):
    from sketch2img_amd.controlnet import Control
    return Control(SimpleNamespace(prepare_timesteps=lambda ts: None, ctx=None), torch.zeros(4, 32), scale, start, end)


# ---------------------------------------------------------------------------------------------------------- 1. key completeness
def test_every_plan_field_is_in_the_key():
    """A field without an entry in `other` is a KeyError here: a field added to StepPlan has to come with a second value."""
    from sketch2img_amd.sampler import DDIMTables, StepPlan
    base = dict(guidance_scale=7.5, beta=1.6, eta=0.0, classifier_free=True, start=0, masked=False, share_cfg_prefix=True,
                unguided=True, control=None)
    other = dict(guidance_scale=5.0, beta=1.0, eta=0.5, classifier_free=False, start=1, masked=True, share_cfg_prefix=False,
                 unguided=False, control=_control())
    tab, shape = DDIMTables.make(4), (1, 4, 8, 8)
    k0 = StepPlan(**base).key(tab, shape)
    assert k0 == StepPlan(**base).key(DDIMTables.make(4), shape) and hash(k0) == hash(StepPlan(**base).key(tab, shape))
    keys = {k0}
    for f in dataclasses.fields(StepPlan):
        k = StepPlan(**dict(base, **{f.name: other[f.name]})).key(tab, shape)
        hash(k)
        assert k != k0, f.name
        keys.add(k)
    assert len(keys) == len(base) + 1
    assert StepPlan(**base).key(tab, (1, 4, 8, 16)) != k0
    # the control contributes Control.key(), and nothing when there is none
    kc = StepPlan(**dict(base, control=other["control"])).key(tab, shape)
    assert kc[:len(k0)] == k0 and kc[len(k0):] == other["control"].key()
    assert StepPlan(**dict(base, control=_control(scale=0.5))).key(tab, shape) != kc


def _perturbed_tables():
    """(table, {field: another legal value}, fields that are functions of a covered field) per scheduler."""
    from sketch2img_amd.sampler import DDIMTables, DPMTables
    d, p = DDIMTables.make(4), DPMTables.make(4)
    d2, p2 = DDIMTables.make(4, beta_end=0.02), DPMTables.make(4, beta_end=0.02)       # equal timesteps, other betas
    assert np.array_equal(d.timesteps, d2.timesteps) and np.array_equal(p.timesteps, p2.timesteps)
    yield d, dict(alphas_cumprod=d2.alphas_cumprod, final_alpha_cumprod=1.0, timesteps=d.timesteps + 1, ratio=d.ratio + 1,
                  v_prediction=True), set()
    yield p, dict(alphas_cumprod=p2.alphas_cumprod, timesteps=p.timesteps + 1, lower_order_final=False, solver_order=1,
                  v_prediction=True, use_karras_sigmas=True, algorithm_type=SDE,
                  sigmas=DPMTables.make(4, use_karras_sigmas=True).sigmas), {"alpha_t", "sigma_t", "lambda_t"}


def test_every_table_field_is_in_the_key():
    """Every dataclass field of a tables class either changes key() when it changes, or is listed as computed from alphas_cumprod
    (make() derives alpha_t, sigma_t and lambda_t from it).  A field added later is in neither list: KeyError."""
    for tab, other, derived in _perturbed_tables():
        k0 = tab.key()
        assert k0 == dataclasses.replace(tab).key() and hash(k0) == hash(dataclasses.replace(tab).key())
        assert k0[0] == type(tab).__name__
        for f in dataclasses.fields(tab):
            if f.name in derived:
                continue
            k = dataclasses.replace(tab, **{f.name: other[f.name]}).key()
            hash(k)
            assert k != k0, (type(tab).__name__, f.name)


def test_graph_key_is_the_plan_key():
    from sketch2img_amd.sampler import DDIMTables, DPMTables, StepPlan, draws_noise, graph_key
    for tab in (DDIMTables.make(4), DPMTables.make(4, use_karras_sigmas=True, algorithm_type=SDE)):
        assert graph_key(tab, (2, 4, 8, 8), False, 7.5, 1.6, True, eta=0.5, classifier_free=True, start_step=1, masked=True) == \
            StepPlan(7.5, 1.6, 0.5, True, 1, True, True, False).key(tab, (2, 4, 8, 8))
        assert all(v in graph_key(tab, (2, 4, 8, 8), True, 7.5, 1.6, True) for v in tab.key())
        assert draws_noise(tab, 0.5) is tab.noisy(0.5) is True


# ---------------------------------------------------------------------------------------------------------- 2. dispatch parity
@pytest.fixture
def recorded(monkeypatch):
    """The four step wrappers replaced by recorders of (name, coefficient tuple, tensors by role, g, keywords)."""
    from sketch2img_amd import ops
    calls = []

    def recorder(name):
        def rec(eu, ec, x, *rest, **kw):
            rest = list(rest)
            z = rest.pop(0) if "eta" in name or "sde" in name else None
            x0 = rest.pop(0) if "dpmpp2m" in name else None
            S, hw, g, coeffs, want_eps = rest
            calls.append(SimpleNamespace(name=name, coeffs=coeffs, z=z, x0=x0, g=g, want_eps=want_eps, kw=kw, shape=(S, hw)))
            return torch.zeros_like(x)
        return rec
    for name in STEP_OPS:
        monkeypatch.setattr(ops, name, recorder(name))
    return calls


def _ladder(tab, eta, T):
    """(kernel, coefficients) per step as HipSampler.step chose them by testing the tables' type."""
    from sketch2img_amd.sampler import DPMTables
    out, seen = [], 0
    for i in range(T):
        t = int(tab.timesteps[i])
        if isinstance(tab, DPMTables):
            order = tab.order(i, seen)
            out.append(("cfg_dpmpp2m_sde_step", tab.coeffs_sde(i, order)) if tab.stochastic else ("cfg_dpmpp2m_step", tab.coeffs(i, order)))
            seen = min(seen + 1, tab.solver_order)
        elif eta > 0.0:
            out.append(("cfg_ddim_eta_step", tab.coeffs_eta(t, eta)))
        else:
            out.append(("cfg_ddim_step", tab.coeffs(t)))
    return out


def _drive(tab, eta, T, x):
    history = tab.new_history(x)
    zs = []
    for i in range(T):
        zs.append(torch.full_like(x, float(i + 1)) if tab.noisy(eta) else None)
        out = tab.update(i, x, x, x, zs[-1], history, x.shape[0], 4, 7.5, False, 0, eta)
        assert torch.is_tensor(out)
    return history, zs


@pytest.mark.parametrize("case", ["ddim", "ddim-eta", "dpm", "dpm-karras", "sde", "sde-karras"])
def test_update_issues_the_kernel_and_coefficients_of_the_type_ladder(recorded, case):
    from sketch2img_amd.sampler import DDIMTables, DPMTables
    T, x = 4, torch.zeros(1, 4, 2, 2)
    eta = 0.5 if case == "ddim-eta" else 0.0
    tab = DDIMTables.make(T) if case.startswith("ddim") else \
        DPMTables.make(T, use_karras_sigmas=case.endswith("karras"), algorithm_type=SDE if case.startswith("sde") else "dpmsolver++")
    history, zs = _drive(tab, eta, T, x)
    assert [(c.name, c.coeffs) for c in recorded] == _ladder(tab, eta, T)
    assert tab.noisy(eta) == (case in ("ddim-eta", "sde", "sde-karras"))
    for c, z in zip(recorded, zs):
        assert c.z is z and c.g == 7.5 and c.want_eps is False and c.shape == (1, 4)
        assert c.kw == dict(lo_off=0, v_prediction=False)
        assert (c.x0 is history.x0) if history is not None else c.x0 is None
    if history is None:
        assert case.startswith("ddim")
    else:
        assert history.seen == tab.solver_order == 2 and torch.equal(history.x0, torch.zeros_like(x))


def test_dpm_drops_eta(recorded):
    """DPM-Solver++ with eta = 0.7: the deterministic kernel, no z asked for; sample() hands the steps eta = 0."""
    from sketch2img_amd.sampler import DDIMTables, DPMTables, HipSampler
    tab = DPMTables.make(4)
    assert not tab.has_eta and DDIMTables.make(4).has_eta and not tab.noisy(0.7)
    _drive(tab, 0.7, 4, torch.zeros(1, 4, 2, 2))
    assert [(c.name, c.coeffs, c.z) for c in recorded] == [(n, co, None) for n, co in _ladder(tab, 0.0, 4)]
    s = HipSampler(SimpleNamespace(dev="cpu", inject=None, prepare_timesteps=lambda ts: None), None)
    etas = []
    s.step = lambda x, *a, **kw: (etas.append((kw["eta"], kw["z"])), (x, None, None))[1]
    s.sample(torch.zeros(1, 4, 2, 2), None, 4, tables=tab, eta=0.7, graphs=False)
    assert etas == [(0.0, None)] * 4


def test_step_allocates_a_fresh_history_after_reset(recorded, monkeypatch):
    """step() on a sampler without history makes a zero one of x's shape (DPM-Solver++ only) and the first step is first order;
    reset_history() drops it, so the next step is first order again; a history handed in is advanced instead of the sampler's."""
    from sketch2img_amd import ops
    from sketch2img_amd.sampler import DDIMTables, DPMTables, History, HipSampler
    monkeypatch.setattr(ops, "nchw_to_nhwc", lambda x, pad: x)
    monkeypatch.setattr(ops, "eps_halves", lambda eps, S, hw: (eps, eps, 0))
    net = SimpleNamespace(dev="cpu", inject=None, forward=lambda x32, *a, **kw: (x32, None))
    s, tab, x = HipSampler(net, None), DPMTables.make(4), torch.ones(1, 4, 2, 2)
    assert s._history is None and s._x0_before is None
    s.step(x, x, None, tab, 0, 7.5, 1.6)
    assert s._x0_before is s._history.x0
    s.step(x, x, None, tab, 1, 7.5, 1.6)
    h = s._history
    assert h.seen == 2 and h.x0.shape == x.shape and recorded[0].x0 is h.x0 is recorded[1].x0
    assert [c.coeffs for c in recorded] == [tab.coeffs(0, 1), tab.coeffs(1, 2)]
    s.reset_history()
    assert s._history is None
    s.step(x, x, None, tab, 1, 7.5, 1.6)
    assert recorded[2].coeffs == tab.coeffs(1, 1) and s._history is not h and s._history.seen == 1
    s.step(torch.ones(2, 4, 2, 2), torch.ones(2, 4, 2, 2), None, tab, 1, 7.5, 1.6)      # another shape: a new zero history
    assert recorded[3].coeffs == tab.coeffs(1, 1) and s._history.x0.shape == (2, 4, 2, 2)
    own, mine = s._history, History(torch.zeros_like(x), 1)
    s.step(x, x, None, tab, 1, 7.5, 1.6, history=mine)
    assert recorded[4].coeffs == tab.coeffs(1, 2) and recorded[4].x0 is mine.x0 and mine.seen == 2 and s._history is own
    s.reset_history()
    s.step(x, x, None, DDIMTables.make(4), 0, 7.5, 1.6)
    assert s._history is None and recorded[5].name == "cfg_ddim_step"


# ------------------------------------------------------------------------------------------------- 3. window and blend schedule
def test_eager_loop_and_warm_up_pass_run_the_same_schedule(monkeypatch):
    """start = 1, T = 5, control window (0.25, 0.75), a mask: the control reaches step() exactly on the executed steps n with
    Control.active(n, 4) and every step ends with the blend at tab.level(i + 1) - from sample()'s eager loop and from a GraphSet's
    warm-up pass alike.  The eager loop passes the caller's control and no z; the set passes its own control, history and z slice."""
    from sketch2img_amd import ops
    from sketch2img_amd.sampler import DPMTables, GraphSet, History, HipSampler, StepPlan
    T, start = 5, 1
    tab = DPMTables.make(T, use_karras_sigmas=True, algorithm_type=SDE)
    ctl = _control(0.25, 0.75)
    x = torch.zeros(2, 4, 2, 2)
    init, mask = torch.ones_like(x), torch.ones(2, 1, 2, 2)
    log, extra = [], []

    def step(x, noise, target, tab_, i, g, beta, **kw):
        log.append(["step", i, kw["control"] is not None, g, beta, kw["eta"], kw["classifier_free"]])
        extra.append((kw["control"], kw["z"], kw["history"]))
        return x + 1.0, None, None

    def latent_renoise(init_, noise, a, s, x=None, mask=None):
        if mask is None:
            return a * init_ + s * noise                      # sample()'s start level
        log.append(["blend", (a, s)])
        return x

    monkeypatch.setattr(ops, "latent_renoise", latent_renoise)
    sampler = HipSampler(SimpleNamespace(dev="cpu", inject=None, ctx=None, prepare_timesteps=lambda ts: None), None)
    sampler.step = step
    out = sampler.sample(x, None, T, tables=tab, init_latents=init, start_step=start, mask=mask, control=ctl, graphs=False)
    eager, eager_extra = list(log), list(extra)
    want = []
    for n, i in enumerate(range(start, T)):
        want += [["step", i, ctl.active(n, T - start), 7.5, 1.6, 0.0, True], ["blend", tab.level(i + 1)]]
    assert eager == want and [e[2] for e in eager if e[0] == "step"] == [False, True, True, False]
    assert torch.equal(out, tab.level(start)[0] * init + tab.level(start)[1] * x + (T - start))
    assert all(z is None and h is None and c in (None, ctl) for c, z, h in eager_extra)

    del log[:], extra[:]
    plan = StepPlan(7.5, 1.6, 0.0, True, start, True, True, True, ctl)
    zs = torch.arange(float(T - start)).reshape(-1, 1, 1, 1, 1).expand(-1, *x.shape).contiguous()
    gs = GraphSet(xs=x.clone(), ns=x.clone(), ts=None, init=init.clone(), mask=mask.clone(), zs=zs,
                  control=ctl.with_hint(ctl.hint.clone()), history=History(torch.zeros_like(x)), owner={}, ctx=None, inject=None,
                  per_image=None, scale=None, cnet=ctl.net, cctx=None, graphs=[], auxs=[])
    gs.warm_up(sampler, plan, tab)
    assert log == eager
    for n, (c, z, h) in enumerate(extra):
        assert c in (None, gs.control) and h is gs.history and torch.equal(z, zs[n])
    assert torch.equal(gs.xs, x), "the warm-up pass works on a copy of the latents"
    assert gs.valid_for(sampler, ctl) and not gs.valid_for(sampler, _control())
