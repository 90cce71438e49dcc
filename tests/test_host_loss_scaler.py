"""CPU tests (-m "not gpu") of the dynamic loss scale: loss_scaler.DynamicLossScaler's state machine against torch's own op, its
constructor checks and checkpoint keys, the two C entry points' declarations and argument checks, and that FlatAdamW.step without a
scaler is the step it was."""
import os
import random
import re

import pytest
import torch

from sketch2img_amd import _lib, flat_adamw, loss_scaler, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ["scale", "growth_factor", "backoff_factor", "growth_interval", "_growth_tracker"]


def test_update_rule_matches_torch_amp_update_scale_step_by_step():
    """300 seeded verdicts (a third of them overflows), growth_interval = 3: scale and growth tracker equal
    torch._amp_update_scale_'s on CPU tensors after every one."""
    rnd = random.Random(7)
    seq = [rnd.random() < 1.0 / 3.0 for _ in range(300)]
    assert any(seq) and not all(seq)
    sc = loss_scaler.DynamicLossScaler("cpu", init_scale=2.0 ** 16, growth_interval=3)
    scale, tracker = torch.full((), 2.0 ** 16), torch.zeros((), dtype=torch.int32)
    grew = 0
    for i, found in enumerate(seq):
        before = float(scale)
        torch._amp_update_scale_(scale, tracker, torch.tensor(float(found)), 2.0, 0.5, 3)
        assert sc.update(found) == float(scale), (i, sc.scale, float(scale))
        assert sc.scale == float(scale) and sc.growth_tracker == int(tracker), i
        grew += float(scale) > before
    assert grew > 5                                               # (the sequence exercises growth as well as backoff)
    # the case checked by hand: scale 4, found_inf 1 -> 2, tracker 0
    sc = loss_scaler.DynamicLossScaler("cpu", init_scale=4.0, growth_interval=3)
    sc.update(False)
    assert sc.growth_tracker == 1
    assert sc.update(True) == 2.0 and sc.growth_tracker == 0


def test_defaults_are_torch_grad_scalers():
    ref = torch.amp.GradScaler("cpu", enabled=True)
    sc = loss_scaler.DynamicLossScaler("cpu")
    assert (sc.scale, sc.growth_factor, sc.backoff_factor, sc.growth_interval, sc.growth_tracker) == \
        (65536.0, ref.get_growth_factor(), ref.get_backoff_factor(), ref.get_growth_interval(), 0)
    assert sc.flag.shape == (1,) and sc.flag.dtype == torch.float32 and float(sc.flag) == 0.0
    assert sc.verdict is None and not sc.pending


@pytest.mark.parametrize("kw", [dict(init_scale=3.0), dict(init_scale=0.0), dict(init_scale=-4.0), dict(init_scale=float("inf")),
                                dict(growth_factor=3.0), dict(growth_factor=1.0), dict(growth_factor=0.5),
                                dict(backoff_factor=0.3), dict(backoff_factor=1.0), dict(backoff_factor=2.0),
                                dict(growth_interval=0)])
def test_constructor_refuses_what_is_not_a_power_of_two(kw):
    with pytest.raises(AssertionError):
        loss_scaler.DynamicLossScaler("cpu", **kw)


def test_state_dict_round_trip_uses_torchs_five_keys():
    sc = loss_scaler.DynamicLossScaler("cpu", init_scale=2.0 ** 12, growth_factor=4.0, backoff_factor=0.25, growth_interval=5)
    for found in (False, False, True, False):
        sc.update(found)
    sd = sc.state_dict()
    assert list(sd) == KEYS == list(torch.amp.GradScaler("cpu", enabled=True).state_dict())
    assert sd == {"scale": 2.0 ** 10, "growth_factor": 4.0, "backoff_factor": 0.25, "growth_interval": 5, "_growth_tracker": 1}
    other = loss_scaler.DynamicLossScaler("cpu")
    other.load_state_dict(sd)
    assert other.state_dict() == sd
    for found in (False,) * 4:
        assert other.update(found) == sc.update(found)
    assert other.scale == 2.0 ** 12 and other.growth_tracker == 0
    # a torch GradScaler's own state dict loads as data
    other.load_state_dict(torch.amp.GradScaler("cpu", init_scale=2.0 ** 9, growth_interval=7, enabled=True).state_dict())
    assert (other.scale, other.growth_factor, other.backoff_factor, other.growth_interval) == (512.0, 2.0, 0.5, 7)
    with pytest.raises(AssertionError):
        other.load_state_dict({k: sd[k] for k in KEYS[:4]})
    with pytest.raises(AssertionError):
        other.load_state_dict(dict(sd, scale=3.0))


def test_new_symbols_are_declared_bound_and_check_their_arguments_without_a_gpu():
    src = open(os.path.join(ROOT, "include", "skg.h")).read()
    assert re.search(r"int skg_nonfinite_flag\(const float\* x, size_t n, float\* flag, int reset, void\* stream\);", src)
    assert re.search(r"int skg_adamw_step_guarded\([^;]*const float\* skip_flag, void\* stream\);", src)
    assert re.search(r"#define SKG_ABI_VERSION 6\b", src)
    assert _lib.SIGNATURES["skg_nonfinite_flag"] == ("i", "pzpip")
    assert _lib.SIGNATURES["skg_adamw_step_guarded"] == ("i", _lib.SIGNATURES["skg_adamw_step"][1][:-1] + "pp")
    assert _lib.ABI_VERSION == 6 and _lib.lib.skg_abi_version() == 6
    nf, gs = _lib.lib.skg_nonfinite_flag, _lib.lib.skg_adamw_step_guarded
    assert nf(None, 4, 16, 1, None) == -1 and nf(16, 4, None, 1, None) == -1 and nf(16, 0, 16, 1, None) == -1
    assert nf(18, 4, 16, 0, None) == -1                           # x not 4-byte aligned
    tail = (1e-3, 0.9, 0.999, 1e-8, 1e-2, 1, 1.0)
    assert gs(16, 16, 16, 16, 16, 4, *tail, None, None) == -1     # no flag
    assert gs(None, 16, 16, 16, 16, 4, *tail, 16, None) == -1 and gs(16, None, 16, 16, 16, 4, *tail, 16, None) == -1
    assert gs(16, 16, None, 16, 16, 4, *tail, 16, None) == -1 and gs(16, 16, 16, None, 16, 4, *tail, 16, None) == -1
    assert gs(16, 16, 16, 16, 16, 0, *tail, 16, None) == -1       # n == 0
    assert gs(16, 16, 16, 16, 16, 4, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 0, 1.0, 16, None) == -1      # step 0


SHAPES = [("a.weight", (3, 5)), ("a.bias", (3,))]


def _opt():
    g = torch.Generator().manual_seed(5)
    sd = {k: torch.randn(shp, generator=g) for k, shp in SHAPES}
    return flat_adamw.FlatAdamW(SHAPES, sd, "cpu", lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2,
                                schedule=lambda s: 0.5 ** s, grad_scale=64.0)


def test_step_without_a_scaler_is_the_unguarded_step(monkeypatch):
    st = _opt()
    calls, guarded = [], []
    monkeypatch.setattr(ops, "adamw_step", lambda *a: calls.append(a))
    monkeypatch.setattr(ops, "adamw_step_guarded", lambda *a: guarded.append(a))
    g = st.new_grad()
    assert st.step(g) is True and st.step(g, checked=True) is True and st.step(g, scaler=None) is True
    assert len(calls) == 3 and not guarded and st.step_count == 3
    assert calls[2][5:] == (1e-3 * 0.25, 0.9, 0.999, 1e-8, 1e-2, 3, 1.0 / 64.0)


def test_step_under_a_scaler_is_tentative_until_the_verdict_resolves(monkeypatch):
    """step(scaler=, scale=): the guarded kernel with the scaler's flag, step_count + 1, the LR of step_count and 1 / scale; the
    step count moves when the verdict resolves clean and stays on a hit; one verdict settles two optimizers."""
    a, b = _opt(), _opt()
    calls, guarded = [], []
    monkeypatch.setattr(ops, "adamw_step", lambda *x: calls.append(x))
    monkeypatch.setattr(ops, "adamw_step_guarded", lambda *x: guarded.append(x))
    monkeypatch.setattr(ops, "nonfinite_flag", lambda x, flag, reset=False: (flag.zero_() if reset else None,
                                                                           flag.fill_(1.0) if not torch.isfinite(x).all() else None))
    sc = loss_scaler.DynamicLossScaler("cpu", init_scale=2.0 ** 10, growth_interval=2)
    a.step_count = b.step_count = 2
    ga, gb = a.new_grad(), b.new_grad()
    with pytest.raises(AssertionError):
        a.step(ga, scaler=sc, scale=1024.0)                       # no check() queued
    s = sc.scale
    v = sc.check(ga, gb)
    assert sc.pending and not v.resolved
    with pytest.raises(AssertionError):
        a.step(ga, scaler=sc)                                     # scale= is required
    assert a.step(ga, scaler=sc, scale=s) is v and b.step(gb, scaler=sc, scale=s * 256.0) is v
    with pytest.raises(AssertionError):
        a.step(ga, scaler=sc, scale=s)                            # twice under one verdict
    assert not calls and len(guarded) == 2 and a.step_count == b.step_count == 2 and not v.resolved
    p, gr, m, vv, p16, lr, b1, b2, eps, wd, step, inv, flag = guarded[0]
    assert (lr, step, inv) == (1e-3 * 0.25, 3, 1.0 / 1024.0) and flag is sc.flag
    assert p.data_ptr() == a.p.data_ptr() and gr.data_ptr() == ga.data_ptr() and p.numel() == a.n_opt
    assert guarded[1][11] == 1.0 / (1024.0 * 256.0) and guarded[1][12] is sc.flag
    assert bool(v) is True and v.resolved and a.step_count == b.step_count == 3 and sc.scale == 1024.0 and sc.growth_tracker == 1
    # a hit in the second vector alone: neither counts, the scale halves
    gb[1] = float("nan")
    s = sc.scale
    v = sc.check(ga, gb)
    a.step(ga, scaler=sc, scale=s)
    b.step(gb, scaler=sc, scale=s * 256.0)
    assert guarded[2][10] == 4 and a.step_count == 3
    assert sc.scale == 512.0 and v.resolved and bool(v) is False                 # reading the scale resolved it
    assert a.step_count == b.step_count == 3 and sc.growth_tracker == 0
    # the next check() resolves what is pending
    gb[1] = 0.0
    v1 = sc.check(ga, gb)
    a.step(ga, scaler=sc, scale=512.0)
    v2 = sc.check(ga, gb)
    assert v1.resolved and not v2.resolved and a.step_count == 4 and b.step_count == 3
    assert bool(v2) and sc.scale == 1024.0 and sc.growth_tracker == 0            # two clean verdicts: grown
