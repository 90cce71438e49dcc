"""CPU tests (-m "not gpu") of ControlNet conditioning: the skg_conv3x3_small_f16 symbol and its argument checks, the weight pack of
the small-channel convolutions, the key manifest and its validation, the config rejections, from_unet, the step window, the
pipeline's argument checks (raised ahead of any device work) and the identities of the CPU restatement (tests/controlnet_ref.py)
the GPU tests compare against.  No kernel is launched here."""
import json
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_conv3x3_small_symbol_is_declared_bound_and_exported():
    from sketch2img_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "skg.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+skg_conv3x3_small_f16\s*\(([^;{]*?)\)\s*;", src, flags=re.S)
    assert m, "include/skg.h does not declare skg_conv3x3_small_f16"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    letters = "".join("p" if "*" in a else "f" if a.startswith("float") else "i" if a.startswith("int") else "?" for a in args)
    assert letters == "pippiiiiiiipip" and _lib.SIGNATURES["skg_conv3x3_small_f16"] == ("i", letters)
    assert _lib.ABI_VERSION == 6 and _lib.lib.skg_abi_version() == 6          # additive: no bump
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert "skg_conv3x3_small_f16" in set(re.findall(r" T (skg_\w+)", nm))


def test_conv3x3_small_checks_its_arguments_without_a_gpu():
    """SKG_E_BADARG before any HIP call (the pointers are never dereferenced: 16 stands for 'not NULL and aligned')."""
    from sketch2img_amd import _lib
    f = _lib.lib.skg_conv3x3_small_f16
    a = lambda X=16, ldx=16, Wp=16, Y=16, ldy=32, B=1, IH=8, IW=8, Cin=16, Cout=32, stride=1, bias=None: \
        (X, ldx, Wp, Y, ldy, B, IH, IW, Cin, Cout, stride, bias, 1, None)
    for bad in (a(X=None), a(Wp=None), a(Y=None), a(B=0), a(IH=0), a(Cin=4), a(Cin=32), a(Cout=8), a(Cout=64), a(stride=3), a(stride=0),
                a(stride=2, IH=7), a(stride=2, IW=6 + 1), a(ldy=16), a(ldy=34), a(ldx=8), a(ldx=20), a(Y=4), a(X=8), a(bias=4),
                a(Cin=3, X=2)):
        assert f(*bad) == -1, bad


def test_pack_conv_small_layout():
    from sketch2img_amd.packs import pack_conv_small
    g = torch.Generator().manual_seed(3)
    for ci, kp, cp in ((3, 64, 4), (16, 160, 16)):
        w = torch.randn(32, ci, 3, 3, generator=g).half().float()
        p = pack_conv_small(w, "cpu").float()
        assert p.shape == (32, kp) and p.dtype == torch.float32
        p = p.reshape(32, kp // cp, cp)
        for ky in range(3):
            for kx in range(3):
                assert torch.equal(p[:, 3 * ky + kx, :ci], w[:, :, ky, kx])
        assert p[:, 9:].abs().sum() == 0 and p[:, :, ci:].abs().sum() == 0      # (tap slots 9 .., padding channels: zero)
    with pytest.raises(ValueError):
        pack_conv_small(torch.zeros(16, 8, 3, 3), "cpu")


# ------------------------------------------------------------------------------------------------------ manifest, validation
def test_key_manifest_sd15():
    from sketch2img_amd import synthetic
    from sketch2img_amd.config import SD15, TINY
    s = synthetic.controlnet_param_shapes(SD15)
    assert synthetic.controlnet_num_residuals(SD15) == 12 and synthetic.controlnet_num_residuals(TINY) == 12
    assert synthetic.controlnet_residual_channels(SD15) == (320, 320, 320, 320, 640, 640, 640, 1280, 1280, 1280, 1280, 1280)
    # diffusers' ControlNetModel.state_dict() layout, SD1.5: the encoder keys are the UNet's own
    u = synthetic.unet_param_shapes(SD15)
    enc = {k: v for k, v in u.items() if k.split(".")[0] in ("conv_in", "time_embedding", "down_blocks", "mid_block")}
    assert all(s[k] == v for k, v in enc.items())
    rest = {k: v for k, v in s.items() if k not in enc}
    assert not any(k.startswith(("up_blocks", "conv_out", "conv_norm_out")) for k in s)
    e = "controlnet_cond_embedding"
    assert rest[e + ".conv_in.weight"] == (16, 3, 3, 3) and rest[e + ".conv_out.weight"] == (320, 256, 3, 3)
    assert [rest[f"{e}.blocks.{i}.weight"] for i in range(6)] == [(16, 16, 3, 3), (32, 16, 3, 3), (32, 32, 3, 3), (96, 32, 3, 3),
                                                                  (96, 96, 3, 3), (256, 96, 3, 3)]
    assert [rest[f"controlnet_down_blocks.{k}.weight"][0] for k in range(12)] == list(synthetic.controlnet_residual_channels(SD15))
    assert rest["controlnet_down_blocks.4.weight"] == (640, 640, 1, 1) and rest["controlnet_mid_block.weight"] == (1280, 1280, 1, 1)
    assert len(rest) == 2 * (8 + 12 + 1)
    # the public SD1.5 ControlNets have 361 279 120 parameters
    import math
    assert sum(math.prod(v) for v in s.values()) == 361_279_120


def _tiny_model():
    from sketch2img_amd.config import TINY
    from sketch2img_amd.controlnet import ControlNetModel
    return ControlNetModel.from_pretrained(None, unet_config=TINY)


def test_synthetic_opt_in_and_facade():
    from sketch2img_amd import synthetic
    from sketch2img_amd.config import TINY
    m = _tiny_model()
    sd = m.state_dict()
    assert list(sd) == list(synthetic.controlnet_param_shapes(TINY))
    assert all(torch.equal(v, v.half().float()) for v in sd.values())
    assert float(sd["controlnet_down_blocks.3.weight"].abs().max()) > 0 and float(sd["controlnet_mid_block.weight"].abs().max()) > 0
    assert m.config.conditioning_embedding_out_channels == (16, 32, 96, 256) and m.config.global_pool_conditions is False
    assert m.device == torch.device("cpu") and m.to("cpu") is m and m.state_dict() is sd
    with pytest.raises(RuntimeError, match="GPU only"):
        m.hip


def test_shape_and_key_validation():
    from sketch2img_amd.config import TINY
    from sketch2img_amd.controlnet import ControlNetModel
    sd = dict(_tiny_model().state_dict())
    bad = dict(sd); del bad["controlnet_down_blocks.11.bias"]
    with pytest.raises(ValueError, match="1 missing keys"):
        ControlNetModel(TINY, bad)
    bad = dict(sd); bad["controlnet_mid_block.weight"] = torch.zeros(64, 64, 1, 1)
    with pytest.raises(ValueError, match="1 shape mismatches"):
        ControlNetModel(TINY, bad)
    bad = dict(sd); bad["up_blocks.0.resnets.0.conv1.bias"] = torch.zeros(128)
    with pytest.raises(ValueError, match="1 unexpected keys"):
        ControlNetModel(TINY, bad)
    ok = dict(sd); ok["controlnet_mid_block.weight"] = sd["controlnet_mid_block.weight"].reshape(128, 128)      # (a linear-form 1x1)
    ControlNetModel(TINY, ok)


def _write_folder(tmp_path, cfg_json, sd):
    torch.save(sd, tmp_path / "diffusion_pytorch_model.bin")
    (tmp_path / "config.json").write_text(json.dumps(cfg_json))
    return str(tmp_path)


TINY_JSON = dict(block_out_channels=[32, 64, 128, 128], cross_attention_dim=64, attention_head_dim=[2, 2, 4, 4], norm_num_groups=8,
                 sample_size=32, layers_per_block=2, down_block_types=["CrossAttnDownBlock2D"] * 3 + ["DownBlock2D"],
                 conditioning_embedding_out_channels=[16, 32, 96, 256], global_pool_conditions=False, class_embed_type=None)


def test_from_pretrained_reads_a_folder(tmp_path):
    from sketch2img_amd.config import TINY
    from sketch2img_amd.controlnet import ControlNetModel
    sd = _tiny_model().state_dict()
    m = ControlNetModel.from_pretrained(_write_folder(tmp_path, TINY_JSON, sd))
    assert m.cfg == TINY and all(torch.equal(m.state_dict()[k], v) for k, v in sd.items())
    with pytest.raises(FileNotFoundError):
        ControlNetModel.from_pretrained(str(tmp_path / "nothing-here"))
    from sketch2img_amd.config import SD15
    with pytest.raises(ValueError, match="unet_config="):
        ControlNetModel.from_pretrained(str(tmp_path), unet_config=SD15)


@pytest.mark.parametrize("field,value,exc", [
    ("global_pool_conditions", True, "global_pool_conditions"),
    ("class_embed_type", "timestep", "class_embed_type"),
    ("conditioning_embedding_out_channels", [16, 32, 96], "four entries"),
    ("conditioning_embedding_out_channels", [16, 32, 96, 256, 512], "four entries"),
    ("conditioning_embedding_out_channels", [8, 32, 96, 256], "hint encoder"),
    ("conditioning_channels", 1, "conditioning_channels"),
    ("act_fn", "gelu", "act_fn"),                                    # (what _config_from_folder rejects for a UNet)
    ("down_block_types", ["DownBlock2D"] * 4, "block types"),
    ("resnet_time_scale_shift", "scale_shift", "resnet_time_scale_shift"),
])
def test_config_rejections(tmp_path, field, value, exc):
    from sketch2img_amd.controlnet import ControlNetModel
    folder = _write_folder(tmp_path, dict(TINY_JSON, **{field: value}), _tiny_model().state_dict())
    with pytest.raises(NotImplementedError, match=exc):
        ControlNetModel.from_pretrained(folder)


def test_from_unet():
    from sketch2img_amd import synthetic
    from sketch2img_amd.config import TINY
    from sketch2img_amd.controlnet import ControlNetModel
    from sketch2img_amd.modules.pipeline import AntiGradientPipeline
    pipe = AntiGradientPipeline.from_pretrained(None, unet_config=TINY)
    m = ControlNetModel.from_unet(pipe.unet)
    sd, usd = m.state_dict(), pipe.unet.state_dict()
    assert list(sd) == list(synthetic.controlnet_param_shapes(TINY))
    for k, v in sd.items():
        if k.startswith(("controlnet_down_blocks", "controlnet_mid_block")):
            assert v.abs().max() == 0, k
        elif k.startswith("controlnet_cond_embedding"):
            assert v.abs().max() > 0, k
        else:
            assert torch.equal(v, usd[k]) and v.data_ptr() != usd[k].data_ptr(), k


@pytest.mark.parametrize("start,end,N,want", [(0.0, 1.0, 3, [1, 1, 1]), (0.0, 0.5, 3, [1, 0, 0]), (0.5, 1.0, 4, [0, 0, 1, 1]),
                                              (0.5, 0.5, 3, [0, 0, 0]), (0.0, 0.0, 3, [0, 0, 0]), (0.25, 0.75, 4, [0, 1, 1, 0])])
def test_step_window_is_diffusers(start, end, N, want):
    from sketch2img_amd.controlnet import Control
    c = Control(None, torch.zeros(4, 32), 1.0, start, end)
    keep = [1.0 - float(i / N < start or (i + 1) / N > end) for i in range(N)]          # diffusers' controlnet_keep
    assert [int(c.active(i, N)) for i in range(N)] == want == [int(k) for k in keep]


def test_graph_key_holds_the_control():
    from sketch2img_amd.controlnet import Control
    a = Control(None, torch.zeros(4, 32), 1.0, 0.0, 1.0).key()
    assert a[0] == "controlled" and a != Control(None, torch.zeros(4, 32), 0.5, 0.0, 1.0).key()
    assert a != Control(None, torch.zeros(4, 32), 1.0, 0.0, 0.5).key() and a != Control(None, torch.zeros(8, 32), 1.0).key()
    assert a == Control(None, torch.ones(4, 32), 1.0).key()


# ------------------------------------------------------------------------------------------------------ __call__'s argument checks
@pytest.fixture(scope="module")
def cpu_pipe():
    """A pipeline that was never moved to a GPU: any device work (the text embeddings' upload, the engine) raises RuntimeError, so
    a ValueError / NotImplementedError proves the check came first."""
    from sketch2img_amd.config import TINY
    from sketch2img_amd.modules.pipeline import AntiGradientPipeline
    return AntiGradientPipeline.from_pretrained(None, unet_config=TINY)


def test_call_refusals_come_before_device_work(cpu_pipe):
    from PIL import Image
    net = _tiny_model()
    img = torch.rand(1, 3, 64, 64)
    kw = dict(height=64, width=64, num_inference_steps=2, output_type="latent")
    with pytest.raises(ValueError, match="needs the `controlnet`"):
        cpu_pipe("p", control_image=img, **kw)
    with pytest.raises(ValueError, match="needs a `control_image`"):
        cpu_pipe("p", controlnet=net, **kw)
    with pytest.raises(NotImplementedError, match="list of ControlNets"):
        cpu_pipe("p", controlnet=[net, net], control_image=[img, img], **kw)
    with pytest.raises(ValueError, match="cannot be combined with a ControlNet"):
        cpu_pipe("p", controlnet=net, control_image=img, sketch_image=torch.zeros(1, 4, 8, 8), **kw)
    with pytest.raises(ValueError, match="has to be 64 x 64"):
        cpu_pipe("p", controlnet=net, control_image=torch.rand(1, 3, 64, 128), **kw)
    with pytest.raises(ValueError, match=r"\[1 or 2, 3, 64, 64\]"):
        cpu_pipe(["p", "q"], controlnet=net, control_image=torch.rand(3, 3, 64, 64), **kw)
    with pytest.raises(ValueError, match="is 32 x 64 px"):
        cpu_pipe("p", controlnet=net, control_image=Image.new("RGB", (32, 64)), **kw)
    with pytest.raises(ValueError, match="control_guidance_start"):
        cpu_pipe("p", controlnet=net, control_image=img, control_guidance_start=0.8, control_guidance_end=0.2, **kw)
    with pytest.raises(ValueError, match="ControlNetModel"):
        cpu_pipe("p", controlnet=object(), control_image=img, **kw)
    from sketch2img_amd.config import SD15
    from sketch2img_amd.controlnet import ControlNetModel
    other = ControlNetModel.__new__(ControlNetModel)
    other.cfg = SD15
    with pytest.raises(ValueError, match="was built for"):
        cpu_pipe("p", controlnet=other, control_image=img, **kw)
    # well-formed arguments get past the checks and stop at the first device work
    with pytest.raises(RuntimeError):
        cpu_pipe("p", controlnet=net, control_image=Image.new("RGB", (64, 64)), **kw)


def test_injector_with_control_is_refused(cpu_pipe):
    from types import SimpleNamespace
    net = _tiny_model()
    cpu_pipe.unet._hip = SimpleNamespace(inject=object())
    try:
        with pytest.raises(NotImplementedError, match="SatMixin injector"):
            cpu_pipe("p", height=64, width=64, controlnet=net, control_image=torch.rand(1, 3, 64, 64))
    finally:
        cpu_pipe.unet._hip = None


def test_forward_keywords_are_refused_off_their_walk():
    """HipUNet.forward's new keywords are checked before anything else (no engine is built: the method is called unbound)."""
    from sketch2img_amd.unet import HipUNet
    with pytest.raises(ValueError, match="through_mid"):
        HipUNet.forward(None, None, 1, 2, 8, through_mid=True)
    with pytest.raises(ValueError, match="hint"):
        HipUNet.forward(None, None, 1, 2, 8, hint=torch.zeros(1))
    with pytest.raises(ValueError, match="control"):
        HipUNet.forward(None, None, 1, 2, 8, control=([], [], 1.0))


# ------------------------------------------------------------------------------------------------------ the restatement
def test_restatement_with_zero_residuals_is_the_oracle():
    from oracle import unet as ounet
    from sketch2img_amd import synthetic
    from sketch2img_amd.config import TINY
    from tests import controlnet_ref as cref
    cfg = ounet.TINY
    W = ounet.init_weights(cfg)
    Wc = synthetic.controlnet_state_dict(TINY)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 4, 8, 16, generator=g)
    ehs = torch.randn(2, 77, cfg.cross_attention_dim, generator=g)
    img = torch.rand(1, 3, 64, 128, generator=g)
    with torch.no_grad():
        ref, _ = ounet.unet_forward(cfg, W, x, 301, ehs)
        hint = cref.cond_embedding(Wc, img).repeat(2, 1, 1, 1)
        res = cref.controlnet_forward(cfg, Wc, x, 301, ehs, hint)
        feats = cref.controlnet_forward(cfg, Wc, x, 301, ehs, hint, zero_convs=False)
        zero = cref.unet_forward_controlled(cfg, W, x, 301, ehs, [torch.zeros_like(r) for r in res], 1.0)
        off = cref.unet_forward_controlled(cfg, W, x, 301, ehs, res, 0.0)
        on = cref.unet_forward_controlled(cfg, W, x, 301, ehs, res, 1.0)
        # with the hint zero and the UNet's own weights the trunk IS the UNet's encoder: its skips are down_only's
        blocks = ounet.unet_forward(cfg, W, x, 301, ehs, down_only=True)
        own = cref.controlnet_forward(cfg, W, x, 301, ehs, torch.zeros_like(hint), zero_convs=False)
    assert torch.equal(zero, ref) and torch.equal(off, ref)
    assert float((on - ref).abs().max()) > 1e-3
    assert len(res) == 13 and [tuple(r.shape) for r in res] == [tuple(f.shape) for f in feats]
    assert hint.shape == (2, 32, 8, 16) and res[-1].shape == (2, 128, 1, 2)
    flat = [s for blk in blocks for s in blk]
    assert len(flat) == 11 and all(torch.equal(a, b) for a, b in zip(flat, own[1:12]))
    # the rounding variant stays one fp16 rounding per layer away
    with torch.no_grad():
        e = float((cref.cond_embedding(Wc, img, round_fp16=True) - hint[:1]).norm() / hint[:1].norm())
    assert 0 < e < 2e-3
