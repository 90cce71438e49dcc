"""GPU tests (-m gpu) of ControlNet conditioning: the small-channel convolutions of the hint encoder, the whole encoder, the in-place
zero convolution, the trunk, the controlled UNet in both modes, from_unet, the pipeline, hipGraph replay and the refusals.  The
checker is tests/controlnet_ref.py: diffusers' ControlNetModel restated on the CPU from oracle.unet's functions."""
import pytest
import torch
import torch.nn.functional as F

from tests.util import report

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FP16_RND = 6e-4      # one fp16 output rounding, relative Frobenius (tests/test_gpu_kernels.py)


def nhwc(x):   # [B,C,H,W] -> [B*H*W, C]
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


def from_nhwc(y, B, H, W):
    return y.float().cpu().reshape(B, H, W, -1).permute(0, 3, 1, 2)


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def picture(B, H, W, seed):
    return torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------------------ 1. small-channel convolutions
# (B, height, width): the two sizes of the issue, and one launch of a single partly filled workgroup (192 output pixels: the masked tail)
SMALL_SHAPES = [(2, 32, 48), (2, 64, 64), (1, 8, 24)]
SMALL_LAYERS = [(3, 16, 1), (16, 16, 1), (16, 32, 2)]      # (Cin, Cout, stride): conv_in, blocks.0, blocks.1 of the hint encoder


@pytest.mark.parametrize("B,H,W", SMALL_SHAPES)
@pytest.mark.parametrize("ci,co,stride", SMALL_LAYERS)
def test_small_channel_convolutions(B, H, W, ci, co, stride):
    """Each of the three pixel-resolution layers alone against F.conv2d on the fp16-rounded operands, with the SiLU and without."""
    from sketch2img_amd import ops
    from sketch2img_amd.packs import pack_conv_small
    g = torch.Generator().manual_seed(1000 * ci + 10 * H + W)
    x = torch.rand(B, ci, H, W, generator=g) if ci == 3 else torch.randn(B, ci, H, W, generator=g)
    w = (torch.randn(co, ci, 3, 3, generator=g) * (9 * ci) ** -0.5).half()
    b = (0.1 * torch.randn(co, generator=g)).half()
    xd = x.to(DEV) if ci == 3 else nhwc(x.half()).to(DEV)
    ref = F.conv2d(x.half().float(), w.float(), b.float(), stride=stride, padding=1)
    oh, ow = H // stride, W // stride
    for silu in (True, False):
        y = ops.conv3x3_small(xd, pack_conv_small(w, DEV), B, H, W, stride, bias=b.to(DEV), silu=silu)
        assert y.shape == (B * oh * ow, co) and y.dtype == torch.float16
        r, _ = report(f"conv3x3_small {ci}->{co} s{stride} silu={silu} B={B} @{H}x{W}", from_nhwc(y, B, oh, ow), F.silu(ref) if silu else ref)
        assert r < FP16_RND
    # the output may be a column slice of a wider buffer; no bias
    wide = torch.full((B * oh * ow, co + 8), 7.0, device=DEV, dtype=torch.float16)
    ops.conv3x3_small(xd, pack_conv_small(w, DEV), B, H, W, stride, out=wide[:, :co])
    assert report("conv3x3_small strided out, no bias", from_nhwc(wide[:, :co], B, oh, ow), ref - b.float()[None, :, None, None])[0] < FP16_RND
    assert bool((wide[:, co:] == 7.0).all())


# ------------------------------------------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def tiny():
    """TINY UNet (default mode) + synthetic ControlNet, 4 rows of context."""
    from oracle import unet as ounet
    from sketch2img_amd import synthetic
    from sketch2img_amd.config import TINY
    from sketch2img_amd.controlnet import ControlNetModel
    from sketch2img_amd.unet import HipUNet
    W = ounet.init_weights(ounet.TINY)
    cn = ControlNetModel.from_pretrained(None, unet_config=TINY).to(DEV)
    ehs = rnd(4, 77, TINY.cross_attention_dim, seed=8).half().float()
    net = HipUNet(TINY, W, DEV)
    net.prepare_context(ehs)
    cn.hip.prepare_context(ehs)
    assert list(cn.state_dict()) == list(synthetic.controlnet_param_shapes(TINY))
    return dict(cfg=ounet.TINY, W=W, Wc=cn.state_dict(), cn=cn, net=net, ehs=ehs)


def gpu_controlled_eps(net, cnet, x, t, rows, h, w, image, scale, control=True):
    """eps [rows, 4, h, w] of `net` with (or without) the ControlNet engine `cnet` on the picture(s) `image`."""
    from sketch2img_amd import ops
    from sketch2img_amd.unet import CIN_PAD
    x32 = ops.nchw_to_nhwc(x.to(DEV), CIN_PAD)
    kw = {}
    if control:
        hint = cnet.hint_rows(cnet.embed(image.to(DEV)), image.shape[0], rows)
        kw["control"] = (cnet.forward(x32, t, rows, h, w, hint), cnet.zero_convs, scale)
    eps, _ = net.forward(x32, t, rows, h, want_taps=False, W=w, **kw)
    e = eps.hi.float() + eps.lo.float() if isinstance(eps, ops.Pair) else eps
    return from_nhwc(e, rows, h, w)[:, :4]


# ------------------------------------------------------------------------------------------------------ 2. the hint encoder
@pytest.mark.parametrize("B,H,W", [(2, 64, 64), (1, 32, 48)])
def test_hint_encoder_vs_fp32_restatement(tiny, B, H, W):
    """Bound 2 e + 6e-4: e is the distance from fp32 of the restatement that rounds every layer's output to fp16 - computed here,
    on the CPU -, the factor 2 covers the summation order, 6e-4 the last rounding."""
    from tests import controlnet_ref as cref
    img = picture(B, H, W, seed=H + W)
    with torch.no_grad():
        ref = cref.cond_embedding(tiny["Wc"], img)
        e = float((cref.cond_embedding(tiny["Wc"], img, round_fp16=True) - ref).norm() / ref.norm())
    got = tiny["cn"].hip.embed(img)
    assert got.shape == (B * (H // 8) * (W // 8), 32) and got.dtype == torch.float16
    r, _ = report(f"hint encoder B={B} @{H}x{W} (fp16-rounding restatement e = {e:.3e})", from_nhwc(got, B, H // 8, W // 8), ref)
    assert r < 2 * e + FP16_RND


# ------------------------------------------------------------------------------------------------------ 3. in-place zero convolution
@pytest.mark.parametrize("M,C", [(512, 64), (512, 128), (120, 64), (120, 128), (2048, 320), (128, 1280)])
def test_zero_convolution_in_place_is_the_out_of_place_call(M, C):
    """skip += scale (F Wz^T + b) with the GEMM's residual aliasing its output - a strided destination (ldc > C) and a Pair
    destination - bit-equal to the call that writes another tensor.  (2048, 320) and (128, 1280): a skip of the 32 x 32 level of
    SD1.5 and one of its 8 x 8 level, the long-K launch."""
    from sketch2img_amd import ops
    from sketch2img_amd.unet import _produce
    g = torch.Generator().manual_seed(M + C)
    Fk = torch.randn(M, C, generator=g).half().to(DEV)
    Wz = (torch.randn(C, C, generator=g) * C ** -0.5).half().to(DEV)
    b = (0.1 * torch.randn(C, generator=g)).half().to(DEV)
    scale = 0.75
    # fp16, strided: the skip's columns inside a concat buffer [h | skip]
    buf = torch.randn(M, 2 * C, generator=g).half().to(DEV)
    keep = buf.clone()
    want = ops.gemm(Fk, Wz, bias=b, residual=keep[:, C:], alpha=scale)
    ops.gemm(Fk, Wz, out=buf[:, C:], bias=b, residual=buf[:, C:], alpha=scale)
    assert torch.equal(buf[:, C:], want) and torch.equal(buf[:, :C], keep[:, :C])
    ref = keep[:, C:].float() + scale * (Fk.float() @ Wz.float().t() + b.float())
    assert report(f"zero conv in place M={M} C={C}", buf[:, C:].float().cpu(), ref.cpu())[0] < FP16_RND
    # a Pair inside the pair concat buffer [h_hi | skip_hi | h_lo | skip_lo]
    v = torch.randn(M, 2 * C, generator=g)
    pbuf = torch.cat([v.half(), (v - v.half().float()).half()], 1).to(DEV)
    pkeep = pbuf.clone()
    dst = ops.Pair(pbuf[:, C:2 * C], pbuf[:, 3 * C:])
    src = ops.Pair(pkeep[:, C:2 * C], pkeep[:, 3 * C:])
    out = ops.Pair.empty(M, C, DEV)
    _produce("gemm", Fk, Wz, out=out, bias=b, residual=src, alpha=scale)
    _produce("gemm", Fk, Wz, out=dst, bias=b, residual=dst, alpha=scale)
    assert torch.equal(dst.hi, out.hi) and torch.equal(dst.lo, out.lo)
    assert torch.equal(pbuf[:, :C], pkeep[:, :C]) and torch.equal(pbuf[:, 2 * C:3 * C], pkeep[:, 2 * C:3 * C])
    ref = src.hi.double() + src.lo.double() + scale * (Fk.double() @ Wz.double().t() + b.double())
    # (fp32 accumulation over K = C terms - a random walk of 2^-24 steps, doubled - plus the pair's ~2^-22 storage)
    assert report(f"zero conv in place, pair, M={M} C={C}", (dst.hi.double() + dst.lo.double()).cpu(), ref.cpu())[0] < \
        2.0 ** -24 * (4 + 2 * C ** 0.5)


# ------------------------------------------------------------------------------------------------------ 4. the trunk
@pytest.mark.parametrize("h,w", [(16, 16), (8, 24)])
def test_trunk_residuals_vs_restatement(tiny, h, w):
    """TINY, 4 rows: all n + 1 = 13 residuals (the trunk's features through their zero convolutions) < 1e-2 each - the bound the suite
    gives SketchEncoder's samples."""
    from sketch2img_amd import ops
    from sketch2img_amd.unet import CIN_PAD
    from tests import controlnet_ref as cref
    rows, t = 4, 301
    x = rnd(rows, 4, h, w, seed=h * w).half().float()
    img = picture(2, 8 * h, 8 * w, seed=3)
    cnet = tiny["cn"].hip
    hint = cnet.hint_rows(cnet.embed(img.to(DEV)), 2, rows)
    feats = cnet.forward(ops.nchw_to_nhwc(x.to(DEV), CIN_PAD), t, rows, h, w, hint)
    with torch.no_grad():
        href = cref.cond_embedding(tiny["Wc"], img).repeat(2, 1, 1, 1)
        ref = cref.controlnet_forward(tiny["cfg"], tiny["Wc"], x, t, tiny["ehs"], href)
    assert len(feats) == len(ref) == 13 == len(cnet.zero_convs)
    for k, (f, (Wz, b), r) in enumerate(zip(feats, cnet.zero_convs, ref)):
        got = ops.gemm(f, Wz, bias=b)
        assert report(f"controlnet residual {k} @{h}x{w}", from_nhwc(got, rows, r.shape[2], r.shape[3]), r)[0] < 1e-2


# ------------------------------------------------------------------------------------------------------ 5. controlled eps
@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_controlled_eps_tiny(tiny, scale):
    from tests import controlnet_ref as cref
    rows, h, w, t = 4, 16, 16, 501
    x = rnd(rows, 4, h, w, seed=11).half().float()
    img = picture(1, 8 * h, 8 * w, seed=12)
    with torch.no_grad():
        ref = cref.controlled_eps(tiny["cfg"], tiny["W"], tiny["Wc"], x, t, tiny["ehs"], img, scale)
    got = gpu_controlled_eps(tiny["net"], tiny["cn"].hip, x, t, rows, h, w, img, scale)
    plain = gpu_controlled_eps(tiny["net"], None, x, t, rows, h, w, None, scale, control=False)
    assert report(f"controlled eps TINY scale={scale}", got, ref)[0] < 1e-2
    d = float((got - plain).abs().max())
    print(f"[parity] max |eps_ctrl - eps_plain| = {d:.3e}")
    assert d > 1e-3


@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_controlled_eps_accuracy_mode(scale):
    """block_out_channels (64, 128, 128, 128) - the pair epilogue needs multiples of 64 - in the accuracy mode: the skips of the
    pair zone take the control through the pair epilogue (C_lo / residual_lo), the trunk stays fp16.  The mode's 1e-3 bound is a
    statement about the uncontrolled UNet; the distance with an fp16 trunk in front is printed."""
    from oracle import unet as ounet
    from sketch2img_amd.config import UNetConfig
    from sketch2img_amd.controlnet import ControlNetModel
    from sketch2img_amd.unet import HipUNet
    from tests import controlnet_ref as cref
    kw = dict(block_out_channels=(64, 128, 128, 128), cross_attention_dim=64, num_heads=(2, 2, 4, 4), norm_groups=8, sample_size=32)
    cfg, ocfg = UNetConfig(**kw), ounet.UNetConfig(**kw)
    W = ounet.init_weights(ocfg)
    cn = ControlNetModel.from_pretrained(None, unet_config=cfg).to(DEV)
    rows, h, w, t = 4, 16, 16, 501
    ehs = rnd(rows, 77, 64, seed=8).half().float()
    net = HipUNet(cfg, W, DEV, residual_fp32=True)
    assert net.pair_levels > 0
    net.prepare_context(ehs)
    cn.hip.prepare_context(ehs)
    x = rnd(rows, 4, h, w, seed=21).half().float()
    img = picture(1, 8 * h, 8 * w, seed=22)
    with torch.no_grad():
        ref = cref.controlled_eps(ocfg, W, cn.state_dict(), x, t, ehs, img, scale)
        base, _ = ounet.unet_forward(ocfg, W, x, t, ehs)
    got = gpu_controlled_eps(net, cn.hip, x, t, rows, h, w, img, scale)
    plain = gpu_controlled_eps(net, None, x, t, rows, h, w, None, scale, control=False)
    r, m = report(f"controlled eps, accuracy mode, scale={scale}", got, ref)
    rp, mp = report("uncontrolled eps, accuracy mode (the mode's own distance)", plain, base)
    assert r < 1e-2 and float((got - plain).abs().max()) > 1e-3


# ------------------------------------------------------------------------------------------------------ 6. SD1.5
@pytest.fixture(scope="module")
def sd15():
    import os
    from oracle import unet as ounet
    from sketch2img_amd import synthetic
    from sketch2img_amd.config import SD15
    from sketch2img_amd.controlnet import ControlNetModel
    from sketch2img_amd.unet import HipUNet
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    W = synthetic.unet_state_dict(SD15)
    cn = ControlNetModel.from_pretrained(None).to(DEV)
    ehs = rnd(2, 77, 768, seed=8).half().float()
    cn.hip.prepare_context(ehs)
    return dict(cfg=ounet.SD15, W=W, cn=cn, ehs=ehs, HipUNet=HipUNet, SD15=SD15)


def test_controlled_eps_sd15_both_modes(sd15):
    """SD1.5 synthetic at 32 x 32 latents, 2 rows: the smallest map at which the producer-side GroupNorm sums (HW = 1024) and the
    fused C = 320 launches are live - stale sums of a touched skip would show here.  Bounds of test_unet_sd15_non_square_vs_oracle."""
    from tests import controlnet_ref as cref
    rows, h, w, t = 2, 32, 32, 501
    x1 = rnd(1, 4, h, w, seed=64)
    x = torch.cat([x1, x1]).half().float()
    img = picture(1, 8 * h, 8 * w, seed=65)
    with torch.no_grad():
        ref = cref.controlled_eps(sd15["cfg"], sd15["W"], sd15["cn"].state_dict(), x, t, sd15["ehs"], img, 1.0)
    for hp in (False, True):
        net = sd15["HipUNet"](sd15["SD15"], sd15["W"], DEV, residual_fp32=hp)
        net.prepare_context(sd15["ehs"])
        assert net._gn_from_producer(rows, h * w, 320)
        got = gpu_controlled_eps(net, sd15["cn"].hip, x, t, rows, h, w, img, 1.0)
        plain = gpu_controlled_eps(net, None, x, t, rows, h, w, None, 1.0, control=False)
        r, m = report(f"controlled eps sd15 32x32 residual_fp32={hp}", got, ref)
        print(f"[parity] sd15 max |eps_ctrl - eps_plain| = {float((got - plain).abs().max()):.3e}")
        assert r < 2e-3 and m < 3e-3
        assert float((got - plain).abs().max()) > 1e-3
        del net
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------ 7. from_unet
def test_from_unet_changes_nothing(tiny):
    """Zero zero-convolutions: eps is the uncontrolled call's, bit for bit (default mode), although the trunk ran."""
    from sketch2img_amd.controlnet import ControlNetModel
    from types import SimpleNamespace
    from sketch2img_amd.config import TINY
    cn = ControlNetModel.from_unet(SimpleNamespace(cfg=TINY, state_dict=lambda: tiny["W"])).to(DEV)
    cn.hip.prepare_context(tiny["ehs"])
    rows, h, w, t = 4, 16, 16, 301
    x = rnd(rows, 4, h, w, seed=31).half().float()
    img = picture(1, 8 * h, 8 * w, seed=32)
    got = gpu_controlled_eps(tiny["net"], cn.hip, x, t, rows, h, w, img, 1.0)
    plain = gpu_controlled_eps(tiny["net"], None, x, t, rows, h, w, None, 1.0, control=False)
    assert torch.equal(got, plain)


# ------------------------------------------------------------------------------------------------------ 8. the pipeline
@pytest.fixture(scope="module")
def pipe():
    from sketch2img_amd.config import TINY
    from sketch2img_amd.controlnet import ControlNetModel
    from sketch2img_amd.modules.pipeline import AntiGradientPipeline
    p = AntiGradientPipeline.from_pretrained(None, unet_config=TINY, torch_dtype=torch.float16).to("cuda")
    return p, ControlNetModel.from_pretrained(None, unet_config=TINY)


def dpm2m():
    from sketch2img_amd.schedulers import DPMSolverMultistepScheduler
    return DPMSolverMultistepScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", num_train_timesteps=1000,
                                       algorithm_type="dpmsolver++", solver_type="midpoint", lower_order_final=True)


def oracle_loop(cfg, W, Wc, ehs, lat, img, T, kind, scale, g_scale=7.5):
    """The reference's sampling loop (CFG + DDIM / DPM-Solver++ 2M of the oracle) with the twin as the UNet, one sample at a time."""
    from oracle import ddim as oddim, dpmsolver as odpm
    from tests import controlnet_ref as cref
    S = lat.shape[0]
    tab = oddim.make_tables(T) if kind == "ddim" else odpm.make_tables(T)
    outs = []
    for s in range(S):
        e_s = torch.stack([ehs[s], ehs[S + s]])
        x, state = lat[s:s + 1].clone(), odpm.DPMState()
        for i, t in enumerate(tab.timesteps.tolist()):
            with torch.no_grad():
                eu, ec = cref.controlled_eps(cfg, W, Wc, torch.cat([x] * 2), t, e_s, img[s if img.shape[0] > 1 else 0][None], scale).chunk(2)
            e = eu + g_scale * (ec - eu)
            x = oddim.ddim_step(tab, e, t, x) if kind == "ddim" else odpm.dpm_step(tab, state, e, i, x)
        outs.append(x)
    return torch.cat(outs)


@pytest.mark.parametrize("kind", ["ddim", "dpm"])
def test_pipeline_vs_oracle_loop(pipe, kind):
    """TINY, 3 steps, S = 2 prompts, one control picture shared by both: latents < 1e-2 from the oracle loop with the twin."""
    from oracle import unet as ounet
    p, cn = pipe
    h, T, prompts = 16, 3, ["a cat", "a dog on a hill"]
    lat, img = rnd(2, 4, h, h, seed=90), picture(1, 8 * h, 8 * h, seed=91)
    call = dict(height=8 * h, width=8 * h, num_inference_steps=T, guidance_scale=7.5, latents=lat, output_type="latent")
    old, p.scheduler = p.scheduler, None if kind == "ddim" else dpm2m()
    try:
        out = p(prompts, controlnet=cn, control_image=img, controlnet_conditioning_scale=0.8, **call).cpu()
        plain = p(prompts, **call).cpu()
    finally:
        p.scheduler = old
    ehs = p._encode_prompt(prompts, "cpu", 1, True, None).half().float()
    ref = oracle_loop(ounet.TINY, p.unet.state_dict(), cn.state_dict(), ehs, lat, img, T, kind, 0.8)
    assert out.shape == (2, 4, h, h) and torch.isfinite(out).all()
    assert report(f"pipeline + ControlNet, {kind}, vs the oracle loop", out, ref)[0] < 1e-2
    assert float((out - plain).abs().max()) > 1e-2


def test_pipeline_window_pil_img2img_and_no_cfg(pipe):
    from PIL import Image
    import numpy as np
    p, cn = pipe
    h, T = 16, 4
    lat, img = rnd(1, 4, h, h, seed=92), picture(1, 8 * h, 8 * h, seed=93)
    call = dict(height=8 * h, width=8 * h, num_inference_steps=T, latents=lat, output_type="latent")
    ctl = dict(controlnet=cn, control_image=img)
    plain = p("a cat", **call)
    full = p("a cat", **ctl, **call)
    # an empty window (start == end) makes the uncontrolled launches: bit-equal
    assert torch.equal(p("a cat", control_guidance_start=0.5, control_guidance_end=0.5, **ctl, **call), plain)
    assert torch.equal(p("a cat", control_guidance_start=0.0, control_guidance_end=0.0, **ctl, **call), plain)
    half = p("a cat", control_guidance_start=0.0, control_guidance_end=0.5, **ctl, **call)
    assert not torch.equal(half, plain) and not torch.equal(half, full)
    assert torch.equal(p("a cat", control_guidance_start=0.0, control_guidance_end=1.0, controlnet_conditioning_scale=1.0, **ctl, **call), full)
    # a PIL picture is the tensor of its 8-bit values
    u8 = (img[0] * 255).round().clamp(0, 255).to(torch.uint8)
    pil = Image.fromarray(np.ascontiguousarray(u8.permute(1, 2, 0).numpy()))
    assert torch.equal(p("a cat", controlnet=cn, control_image=pil, **call), p("a cat", controlnet=cn, control_image=u8[None].float() / 255, **call))
    # a batch of one picture is broadcast over S; a list of S pictures conditions each sample on its own
    two = p(["a cat", "a dog"], controlnet=cn, control_image=img, **{**call, "latents": torch.cat([lat, lat])})
    other = picture(1, 8 * h, 8 * h, seed=94)
    mix = p(["a cat", "a dog"], controlnet=cn, control_image=torch.cat([img, other]), **{**call, "latents": torch.cat([lat, lat])})
    assert two.shape == (2, 4, h, h) and torch.equal(two[0], mix[0]) and not torch.equal(two[1], mix[1])
    # img2img composes; guidance_scale <= 1 runs the trunk on the S cond rows
    i2i = p("a cat", image=0.8 * rnd(1, 4, h, h, seed=95), strength=0.6, **ctl, **call)
    assert i2i.shape == (1, 4, h, h) and torch.isfinite(i2i).all()
    nocfg = p("a cat", guidance_scale=1.0, **ctl, **call)
    assert torch.isfinite(nocfg).all() and p.unet.hip.ctx["rows"] == 1 and cn.hip.ctx["rows"] == 1
    assert not torch.equal(nocfg, p("a cat", guidance_scale=1.0, **call))


@pytest.mark.parametrize("kind", ["ddim", "dpm"])
def test_graph_replay_is_eager(tiny, kind):
    """use_graphs=True: the captured steps - ControlNet launches included - equal the eager ones bit for bit, again after another
    control picture of the same size (the set's static hint buffer is refilled), and an uncontrolled call on the same sampler keeps
    its own set."""
    from sketch2img_amd.controlnet import Control
    from sketch2img_amd.sampler import DDIMTables, DPMTables, HipSampler
    net, cnet = tiny["net"], tiny["cn"].hip
    S, h, T = 2, 16, 3
    tab = DDIMTables.make(T) if kind == "ddim" else DPMTables.make(T)
    lat = rnd(S, 4, h, h, seed=70).to(DEV)
    hints = [cnet.hint_rows(cnet.embed(picture(1, 8 * h, 8 * h, seed=s).to(DEV)), 1, 2 * S) for s in (71, 72)]
    eager, graphed = HipSampler(net), HipSampler(net, use_graphs=True)
    outs = []
    for hint in hints + hints[:1]:
        c = Control(cnet, hint, 0.8, 0.0, 0.7)            # (the last step lies outside the window)
        a = eager.sample(lat, None, tables=tab, control=c)
        b = graphed.sample(lat, None, tables=tab, control=c)
        assert torch.equal(a, b)
        outs.append(a)
    assert len(graphed._graphs) == 1 and not torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    plain = eager.sample(lat, None, tables=tab)
    assert torch.equal(graphed.sample(lat, None, tables=tab), plain) and len(graphed._graphs) == 2
    assert not torch.equal(plain, outs[0])


def test_refusals(pipe, tiny):
    from sketch2img_amd.controlnet import Control
    from sketch2img_amd.sampler import HipSampler
    p, cn = pipe
    img = picture(1, 128, 128, seed=1)
    kw = dict(height=128, width=128, num_inference_steps=2, output_type="latent")
    with pytest.raises(ValueError, match="go together"):
        p("a cat", control_image=img, **kw)
    with pytest.raises(ValueError, match="go together"):
        p("a cat", controlnet=cn, **kw)
    with pytest.raises(NotImplementedError, match="list of ControlNets"):
        p("a cat", controlnet=[cn], control_image=[img], **kw)
    with pytest.raises(ValueError, match="sketch_image"):
        p("a cat", controlnet=cn, control_image=img, sketch_image=torch.zeros(1, 4, 16, 16), **kw)
    with pytest.raises(ValueError, match="resize it first"):
        p("a cat", controlnet=cn, control_image=picture(1, 64, 128, seed=2), **kw)
    # the sampler refuses the same combinations on its own
    cnet = tiny["cn"].hip
    c = Control(cnet, torch.zeros(4 * 256, 32, device=DEV, dtype=torch.float16))
    lat = rnd(2, 4, 16, 16, seed=3)
    with pytest.raises(ValueError, match="sketch target"):
        HipSampler(tiny["net"]).sample(lat, torch.zeros(2, 4, 16, 16), num_inference_steps=2, control=c)
    tiny["net"].inject = object()
    try:
        with pytest.raises(NotImplementedError, match="SatMixin injector"):
            HipSampler(tiny["net"]).sample(lat, None, num_inference_steps=2, control=c)
    finally:
        tiny["net"].inject = None
    with pytest.raises(ValueError, match="8x the latents"):
        cnet.forward(None, 1, 4, 16, 16, torch.zeros(4 * 64, 32, device=DEV, dtype=torch.float16))
