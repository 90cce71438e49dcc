"""CPU tests (-m "not gpu") of the CLIP tower trainer's host side: flat layout, fused q / k / v views, checkpoint keys, new symbols."""
import os
import re

import torch

from oracle import clip_vision as oclip
from sketch2img_amd import clip_vision_train as cvt
from sketch2img_amd.clip_vision import CLIPVisionModel
from sketch2img_amd.config import TINY_CLIP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _trainer(**kw):
    sd = oclip.init_weights(oclip.TINY_CLIP)
    return sd, cvt.HipClipTowerTrainer(TINY_CLIP, sd, "cpu", **kw)


def test_state_dict_has_the_oracles_keys_and_shapes():
    sd, tr = _trainer()
    out = tr.state_dict()
    shapes = oclip.param_shapes(oclip.TINY_CLIP)
    assert set(out) == set(shapes) and list(out) == list(shapes)
    for k, shp in shapes.items():
        assert tuple(out[k].shape) == tuple(shp) and out[k].dtype == torch.float32 and torch.equal(out[k], sd[k]), k


def test_state_dict_round_trips_through_the_facade():
    """The checkpoint loads into CLIPVisionModel (strict) - with and without transformers 4.x's prefix - and comes back unchanged; the
    facade takes the calls the reference trainer makes on the tower (clip_guided_trainer.py:117,157)."""
    sd, tr = _trainer()
    out = tr.state_dict()
    model = CLIPVisionModel(TINY_CLIP)
    model.load_state_dict(out, strict=True)
    back = model.state_dict()
    assert set(back) == set(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    model.load_state_dict({"vision_model." + k: v for k, v in out.items()}, strict=True)
    assert all(torch.equal(model.state_dict()[k], sd[k]) for k in sd)
    assert model.train() is model and model.requires_grad_(True) is model and model.requires_grad_(False) is model
    params = list(model.parameters())
    assert len(params) == len(sd) and all(any(p is v for v in model.state_dict().values()) for p in params)


def test_layout_is_disjoint_aligned_and_keeps_post_layernorm_out_of_the_optimizer():
    sd, tr = _trainer()
    spans = sorted((off, off + shp.numel(), k) for k, (off, shp) in tr.layout.items())
    end = 0
    for a, b, k in spans:
        assert a >= end and a % 8 == 0, k                      # disjoint; 16-byte aligned in the fp16 copy
        assert tr.w16(k).data_ptr() % 16 == 0, k
        assert torch.equal(tr.p[a:b].view(tr.layout[k][1]), sd[k]) and torch.equal(tr.w16(k).float(), sd[k]), k
        end = b
    assert tr.n >= end and tr.p16.dtype == torch.float16 and tr.m.shape == tr.v.shape == tr.p.shape == (tr.n,)
    for k in tr.layout:
        assert (tr.layout[k][0] >= tr.n_opt) == k.startswith("post_layernorm."), k
    assert tr.n_opt % 8 == 0 and set(tr.layout) == set(oclip.param_shapes(oclip.TINY_CLIP))


def test_fused_qkv_view_splits_into_the_three_projections():
    sd, tr = _trainer()
    D = TINY_CLIP.hidden_size
    g = torch.arange(tr.n, dtype=torch.float32)
    for l in range(TINY_CLIP.num_hidden_layers):
        p = f"encoder.layers.{l}.self_attn"
        gw, gb = tr.grad_view(g, p + ".qkv.weight"), tr.grad_view(g, p + ".qkv.bias")
        assert gw.shape == (3 * D, D) and gb.shape == (3 * D,)
        assert tr.w16(p + ".qkv.weight").data_ptr() % 16 == 0 and tr.w16(p + ".qkv.bias").data_ptr() % 16 == 0
        for i, n in enumerate(("q_proj", "k_proj", "v_proj")):       # the order HipCLIPVision packs the fused operand in
            w, b = tr.grad_view(g, f"{p}.{n}.weight"), tr.grad_view(g, f"{p}.{n}.bias")
            assert w.data_ptr() == gw[i * D:].data_ptr() and torch.equal(w, gw[i * D:(i + 1) * D]), (l, n)
            assert b.data_ptr() == gb[i * D:].data_ptr() and torch.equal(b, gb[i * D:(i + 1) * D]), (l, n)
            assert torch.equal(tr.w16(p + ".qkv.weight")[i * D:(i + 1) * D].float(), sd[f"{p}.{n}.weight"])
            assert torch.equal(tr.w16(p + ".qkv.bias")[i * D:(i + 1) * D].float(), sd[f"{p}.{n}.bias"])


def test_schedule_and_hyperparameters_are_the_sat_trainers():
    from sketch2img_amd import sat_train
    assert cvt.cosine_with_restarts is sat_train.cosine_with_restarts and cvt.LOSS_SCALE == sat_train.LOSS_SCALE
    _, tr = _trainer(lr=2e-4, warmup_steps=150, total_steps=1150)
    for s in (0, 1, 149, 150, 650, 1149, 1150):
        tr.step_count = s
        assert tr.current_lr() == 2e-4 * sat_train.cosine_with_restarts(s, 150, 1150, 1)
    bad = torch.zeros(tr.n)
    bad[7] = float("nan")
    before = (tr.p.clone(), tr.m.clone(), tr.v.clone(), tr.p16.clone())
    tr.step_count = 0
    assert tr.step(bad) is False and tr.step_count == 0                       # refused before any kernel is touched
    assert all(torch.equal(a, b) for a, b in zip(before, (tr.p, tr.m, tr.v, tr.p16)))


def test_new_symbols_are_declared_and_bound():
    from sketch2img_amd import _lib, ops
    src = open(os.path.join(ROOT, "include", "skg.h")).read()
    assert re.search(r"#define\s+SKG_ABI_VERSION\s+6\b", src)
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bskg_quick_gelu_bwd_f16\s*\(", src)
    assert _lib.SIGNATURES["skg_quick_gelu_bwd_f16"] == ("i", "pipipiiip") and hasattr(_lib.lib, "skg_quick_gelu_bwd_f16")
    assert _lib.ABI_VERSION == 6 and _lib.lib.skg_abi_version() == 6
    assert callable(ops.quick_gelu_bwd)
    # the embedding fold runs on skg_colsum_f16 over the [B, Lp * D] view: its scratch is sized per column
    assert _lib.lib.skg_colsum_scratch_floats(264 * 1024) >= 264 * 1024


def test_loss_scale_tool_finds_the_emulation_it_borrows():
    """tools/clip_loss_scale.py sweeps with the tower emulation and the seam factor DEFINED in tests/test_gpu_clip_train.py (one
    definition); renaming either there must fail here, not silently at the next sweep."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_clip_loss_scale_tool", os.path.join(ROOT, "tools", "clip_loss_scale.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    emulated_tokens, seam_factor = tool._emulation()
    assert callable(emulated_tokens) and callable(seam_factor)
