"""CPU tests (-m "not gpu") of the SatMixin trainer's host side: parameter layout, checkpoint keys, LR schedule, new symbols."""
import math
import os
import re
from types import SimpleNamespace

import torch

from oracle import attn_inject as oinj, unet as ounet
from sketch2img_amd import sat_train, synthetic
from sketch2img_amd.config import TINY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _trainer(**kw):
    sd = oinj.init_state_dict(ounet.TINY, "clip")
    return sd, sat_train.HipSatTrainer(TINY, sd, "cpu", **kw)


def test_layout_follows_the_manifest():
    man = oinj.state_dict_manifest(ounet.TINY, "clip")
    assert list(sat_train.param_shapes(TINY).items()) == list(man.items())
    assert list(synthetic.satmixin_param_shapes(TINY, "clip").items()) == list(man.items())
    sd, tr = _trainer()
    assert list(tr.layout) == list(man) and len(man) == 176
    end = 0
    for k, (off, shp) in tr.layout.items():
        assert tuple(shp) == tuple(man[k]) and off >= end and off % 8 == 0      # disjoint, 16-byte aligned in the fp16 copy
        end = off + shp.numel()
        assert torch.equal(tr.p[off:end].view(shp), sd[k]) and torch.equal(tr.w16(k).float(), sd[k])
    assert tr.n >= end and tr.p16.dtype == torch.float16 and tr.m.shape == tr.v.shape == tr.p.shape


def test_state_dict_round_trips_through_satmixin():
    from sketch2img_amd.modules.clip_guided_attn import SatMixin
    sd, tr = _trainer()
    out = tr.state_dict()
    assert list(out) == list(sd) and all(out[k].dtype == torch.float32 and torch.equal(out[k], sd[k]) for k in sd)
    mixin = SatMixin(SimpleNamespace(cfg=TINY))
    res = mixin.load_state_dict(out)
    assert not res.missing_keys and not res.unexpected_keys
    back = mixin.state_dict()
    assert all(torch.equal(back[k], sd[k]) for k in sd)


def test_cosine_with_restarts_schedule():
    """Against the closed form of diffusers' cosine_with_restarts (one cycle, 150 warm-up steps) at steps 0, 1, 149, 150,
    mid-cycle and the last one."""
    lr, warm, total = 2e-4, 150, 1150
    _, tr = _trainer(lr=lr, warmup_steps=warm, total_steps=total)
    want = {0: 0.0, 1: lr / 150, 149: lr * 149 / 150, 150: lr,
            650: lr * 0.5 * (1 + math.cos(math.pi * 0.5)), 1149: lr * 0.5 * (1 + math.cos(math.pi * 999 / 1000)), 1150: 0.0}
    for s, v in want.items():
        tr.step_count = s
        assert abs(tr.current_lr() - v) <= 1e-12 + 1e-9 * abs(v), (s, tr.current_lr(), v)
    # two cycles restart at the half-way point
    assert sat_train.cosine_with_restarts(650, 150, 1150, 2) == 1.0
    _, tr0 = _trainer(lr=lr, warmup_steps=0, total_steps=8)
    assert tr0.current_lr() == lr


def test_new_symbols_are_declared_and_bound():
    from sketch2img_amd import _lib
    src = open(os.path.join(ROOT, "include", "skg.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    want = {"skg_wgrad_f16": ("i", "pipiiiifipppp"), "skg_wgrad_scratch_floats": ("z", "iii"),
            "skg_layernorm_param_grads": ("i", "pipiiipfipppp"), "skg_layernorm_param_scratch_floats": ("z", "i"),
            "skg_attn_bwd_dkv": ("i", "pipipipipppipiiiiiiifp")}      # (the strided form, folded into the entry point)
    for name, sig in want.items():
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert _lib.SIGNATURES[name] == sig and hasattr(_lib.lib, name)
    assert _lib.lib.skg_abi_version() == 6
    assert _lib.lib.skg_wgrad_scratch_floats(1281, 64, 128) >= 64 * 128 + 64
    assert _lib.lib.skg_layernorm_param_scratch_floats(128) >= 2 * 128


def test_residual_fp32_net_is_refused():
    import pytest
    _, tr = _trainer()
    net = SimpleNamespace(residual_fp32=True)
    z = torch.zeros(1, 4, 16, 16)
    with pytest.raises(NotImplementedError, match="accuracy mode"):
        tr.loss_and_grads(net, z, z, [1], torch.zeros(1, 77, 64), torch.zeros(1, 257, 1024), torch.ones(1000))
