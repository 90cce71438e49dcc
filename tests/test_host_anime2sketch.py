"""Sketch generator (sketch2img_amd/anime2sketch.py), checks that need no GPU: the state_dict surface against the manifest the
reference's own module wrote (tests/golden/anime2sketch_meta.json, tools/gen_golden_anime2sketch.py), the weight packs evaluated
with torch in fp64 against F.conv2d / F.conv_transpose2d, the size rule and the host-side argument checks of the new launchers."""
import json
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.util import GOLDEN, load_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def meta():
    with open(os.path.join(GOLDEN, "anime2sketch_meta.json")) as f:
        return json.load(f)


def checksums(tensors):
    return np.array([[float(t.double().sum()), float((t.double() ** 2).sum())] for t in tensors], dtype=np.float64)


def test_state_dict_manifest_is_the_reference_modules():
    from sketch2img_amd import synthetic
    from sketch2img_amd.anime2sketch import UnetGenerator
    m = meta()
    net = UnetGenerator().eval()
    sd = net.state_dict()
    assert [[k, list(v.shape)] for k, v in sd.items()] == m["manifest"] and len(sd) == 32
    assert sum(p.numel() for p in net.parameters()) == m["parameters"] == 54_405_505
    assert [[k, list(s)] for k, s in synthetic.anime2sketch_param_shapes().items()] == m["manifest"]
    # load_state_dict round trip (strict), and the seeded weights are the ones the golden outputs were computed with
    W = synthetic.anime2sketch_state_dict()
    net.load_state_dict(W)
    assert all(torch.equal(net.state_dict()[k], v) and torch.equal(v, v.half().float()) for k, v in W.items())
    assert np.allclose(checksums(W.values()), load_npz("anime2sketch_256.npz")["weight_checksums"], rtol=1e-12, atol=0)


def test_only_create_models_configuration_is_built():
    import functools
    import torch.nn as nn
    from sketch2img_amd.anime2sketch import UnetGenerator
    UnetGenerator(3, 1, 8, 64, norm_layer=functools.partial(nn.InstanceNorm2d, affine=False, track_running_stats=False), use_dropout=False)
    for args, kw in [((3, 1, 7, 64), {}), ((3, 3, 8, 64), {}), ((3, 1, 8, 64), {"norm_layer": nn.BatchNorm2d}),
                     ((3, 1, 8, 64), {"use_dropout": True}), ((3, 1, 8, 64), {"norm_layer": functools.partial(nn.InstanceNorm2d, affine=True)})]:
        with pytest.raises(NotImplementedError):
            UnetGenerator(*args, **kw)


def test_create_model_strips_the_module_prefix_and_the_alias_package_resolves(tmp_path):
    from anime2sketch.model import create_model
    from sketch2img_amd import anime2sketch as a2s, synthetic
    assert create_model is a2s.create_model
    W = synthetic.anime2sketch_state_dict(seed=5)
    path = str(tmp_path / "netG.pth")
    torch.save({"module." + k: v for k, v in W.items()}, path)
    net = create_model(path)
    assert isinstance(net, a2s.UnetGenerator) and all(torch.equal(net.state_dict()[k], v) for k, v in W.items())
    with pytest.raises(FileNotFoundError):
        create_model(str(tmp_path / "missing.pth"))


def test_synthetic_pictures_match_the_golden_inputs():
    from sketch2img_amd import synthetic
    m = meta()
    for name, c in m["cases"].items():
        x = synthetic.pictures(c["picture"], 1, c["H"], c["W"])
        assert x.shape == (1, 3, c["H"], c["W"]) and float(x.abs().max()) <= 1.0 and torch.equal(x, x.half().float())
        assert np.allclose(checksums([x]), load_npz(f"anime2sketch_{name}.npz")["input_checksum"], rtol=1e-9, atol=0), name
        assert c["band_share"] <= 0.05


def test_transposed_convolution_phase_pack_is_conv_transpose2d():
    """pack_convt evaluated as four 2 x 2-tap stride-1 convolutions over the low-res input (phase (a, b) -> pixels (2i+a, 2j+b))."""
    from sketch2img_amd.anime2sketch import pack_convt
    g = torch.Generator().manual_seed(3)
    for ci, co, ih, iw in [(6, 5, 3, 4), (4, 1, 1, 1), (8, 3, 2, 5)]:
        w = torch.randn(ci, co, 4, 4, generator=g).half().double()
        x = torch.randn(2, ci, ih, iw, generator=g, dtype=torch.float64)
        ref = F.conv_transpose2d(x, w, stride=2, padding=1)
        P = pack_convt(w, cout_pad=8).double()
        assert P.shape == (4, max(co, 8), 4 * ci) and float(P[:, co:].abs().max() if co < 8 else 0) == 0
        out = torch.zeros_like(ref)
        xp = F.pad(x, (1, 1, 1, 1))
        for a in (0, 1):
            for b in (0, 1):
                k = P[2 * a + b, :co].reshape(co, 2, 2, ci).permute(0, 3, 1, 2)      # [co][ty][tx][ci] -> conv2d weight
                full = F.conv2d(xp, k)                                               # windows over rows {i-1, i} at index i, {i, i+1} at i + 1
                out[:, :, a::2, b::2] = full[:, :, a:a + ih, b:b + iw]
        assert float((out - ref).abs().max()) < 1e-12


def test_down_convolution_packs_are_conv2d():
    """pack_conv_down as [Cout][ky*4+kx][Cin] against the unfolded 4 x 4 stride-2 windows; pack_conv_first against the window
    matrix skg_a2s_patch_f16 writes (column (ky*4+kx)*3 + c, 48..63 zero)."""
    from sketch2img_amd.anime2sketch import pack_conv_down, pack_conv_first
    g = torch.Generator().manual_seed(4)
    for ci, co, h, w_ in [(8, 5, 6, 4), (3, 7, 8, 10), (4, 4, 2, 2)]:
        w = torch.randn(co, ci, 4, 4, generator=g).half().double()
        x = torch.randn(2, ci, h, w_, generator=g, dtype=torch.float64)
        ref = F.conv2d(x, w, stride=2, padding=1)
        cols = F.unfold(x, 4, padding=1, stride=2)                                   # [B, ci*16, L], row index c*16 + ky*4 + kx
        win = cols.reshape(2, ci, 16, -1).permute(0, 3, 2, 1).reshape(2, cols.shape[-1], 16 * ci)      # [B, L, tap, c]
        out = (win @ pack_conv_down(w).double().t()).permute(0, 2, 1).reshape(ref.shape)
        assert float((out - ref).abs().max()) < 1e-12
        if ci == 3:
            P = pack_conv_first(w).double()
            assert P.shape == (co, 64) and float(P[:, 48:].abs().max()) == 0
            patch = F.pad(win, (0, 16))                                              # the kernel's [pixels][64] layout
            out = (patch @ P.t()).permute(0, 2, 1).reshape(ref.shape)
            assert float((out - ref).abs().max()) < 1e-12


def test_size_rule():
    from sketch2img_amd.anime2sketch import UnetGenerator, check_size, generate_sketch
    for h, w in [(256, 256), (256, 512), (1024, 768), (1024, 1024)]:
        check_size(h, w)
    net = UnetGenerator()
    for h, w in [(128, 256), (256, 384), (1280, 1024), (255, 256), (512, 2048)]:
        with pytest.raises(ValueError):
            check_size(h, w)
        with pytest.raises(ValueError):
            net(torch.zeros(1, 3, h, w))
    with pytest.raises(ValueError):
        generate_sketch(net, torch.zeros(1, 3, 64, 64), fixed=300)
    with pytest.raises(RuntimeError):      # a valid size on the CPU: there is no CPU path
        net(torch.zeros(1, 3, 256, 256))


def test_product_module_has_no_torch_compute():
    """The generator's arithmetic is libskg.so's: no convolution, matmul, norm or concatenation operator of torch in the module
    (the bicubic resize of generate_sketch is the one exception, imported by name)."""
    src = open(os.path.join(ROOT, "sketch2img_amd", "anime2sketch.py")).read()
    code = "\n".join(l.split("#")[0] for part in src.split('"""')[::2] for l in part.splitlines())      # no docstrings, no comments
    for pat in (r"\bF\.", r"functional\.(?!interpolate)", r"conv\w*d\(", r"matmul", r"einsum", r"instance_norm", r"torch\.cat", r"\bbmm\b",
                r"nn\.(Conv|InstanceNorm|Linear)\w*\(", r" @ ", r"\.mm\("):
        assert not re.search(pat, code), pat
    assert "from torch.nn.functional import interpolate" in src


def test_new_launchers_check_arguments_without_a_gpu():
    """Precondition failures return SKG_E_BADARG before any HIP call."""
    from sketch2img_amd._lib import lib
    ok = dict(X=16, ldx=64, rows=1, HW=4, C=64, eps=1e-5, ident=0, Y0=16, ld0=64, s0=0.2, Y1=16, ld1=128, s1=0.0, scr=None, st=None)

    def inorm(**kw):
        return lib.skg_instnorm_act_f16(*{**ok, **kw}.values())
    assert inorm(X=None) == -1 and inorm(C=96, ldx=96, ld0=96) == -1 and inorm(C=0) == -1 and inorm(ldx=60) == -1 and inorm(ld1=32) == -1
    assert inorm(Y0=None, Y1=None) == -1 and inorm(Y0=8) == -1 and inorm(HW=4096) == -1      # (several slabs need the scratch buffer)
    assert inorm(HW=0) == -1 and inorm(eps=0.0) == -1
    assert lib.skg_instnorm_scratch_floats(2, 262144, 64) == 2 * 256 * 64 * 2 + 2 * 64 * 2 and lib.skg_instnorm_scratch_floats(2, 256, 512) == 0
    assert lib.skg_instnorm_scratch_floats(1, 4096, 512) == 16 * 512 * 2 + 512 * 2 and lib.skg_instnorm_scratch_floats(0, 4, 64) == 0
    convt = lambda **kw: lib.skg_convt4x4s2_f16(*{**dict(X=16, ldx=64, W=16, Y=16, ldy=8, rows=1, IH=1, IW=1, Cin=64, Cout=8, bias=None, epi=1,
                                                        st=None), **kw}.values())
    assert convt(X=None) == -1 and convt(Cin=96, ldx=96) == -1 and convt(Cout=1) == -1 and convt(epi=2) == -1 and convt(ldy=4) == -1
    patch = lambda **kw: lib.skg_a2s_patch_f16(*{**dict(img=16, P=16, ldp=64, B=1, H=256, W=256, st=None), **kw}.values())
    assert patch(img=None) == -1 and patch(H=255) == -1 and patch(ldp=48) == -1 and patch(P=8) == -1 and patch(B=0) == -1
    tail = lambda **kw: lib.skg_a2s_tail(*{**dict(Y=16, ldy=8, y=16, m=None, B=1, H=256, W=256, st=None), **kw}.values())
    assert tail(Y=None) == -1 and tail(y=None) == -1 and tail(W=0) == -1 and tail(ldy=0) == -1
