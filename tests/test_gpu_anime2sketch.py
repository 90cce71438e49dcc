"""Sketch generator on the GPU (-m gpu): the new kernels against torch on the CPU, and the generator end to end against the
outputs of the reference's own module (tests/golden/anime2sketch_*.npz, tools/gen_golden_anime2sketch.py).

End-to-end tolerances are the measured ones of anime2sketch_meta.json: 2 x the distance of the fp16-storage emulation of the
reference (every Conv / ConvTranspose / InstanceNorm output rounded to fp16) from the fp32 reference - the emulation does not
model the MFMA summation order, the fp16 store of tanh's result or statistics taken from rounded outputs."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

from tests.util import GOLDEN, load_npz, report

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CONV_TOL = 5e-4      # test_conv_up2_polyphase / test_conv4x4s2_is_the_dgrad_of_upsample_conv in test_gpu_kernels.py: same kernel bodies


def nhwc(x):
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


def meta():
    with open(os.path.join(GOLDEN, "anime2sketch_meta.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def ops():
    from sketch2img_amd import ops as o
    return o


@pytest.fixture(scope="module")
def net():
    from sketch2img_amd.anime2sketch import UnetGenerator
    return UnetGenerator().eval().to(DEV)      # synthetic.anime2sketch_state_dict(): the weights of the golden vectors


@pytest.mark.parametrize("rows,HW,C", [(2, 4, 512), (1, 4096, 512), (2, 16384, 128), (1, 262144, 64)])
def test_instnorm_two_activated_outputs(ops, rows, HW, C):
    """skg_instnorm_act_f16 vs fp64 on the CPU: LeakyReLU(0.2) into a plain buffer, ReLU into a column slice of a wider one.
    |delta| <= 2^-10 max(1, |ref|): one fp16 ulp of the activated value plus the fp32 statistics' error.  Two runs: same bits."""
    g = torch.Generator().manual_seed(rows * HW + C)
    x = (torch.randn(rows, HW, C, generator=g) * (0.5 + torch.rand(1, 1, C, generator=g)) + 0.5 * torch.randn(rows, 1, C, generator=g)).half()
    xs = torch.zeros(rows * HW, C + 8, dtype=torch.float16, device=DEV)
    xs[:, :C] = x.reshape(-1, C).to(DEV)
    xd = x.double()
    n = (xd - xd.mean(1, keepdim=True)) / (xd.var(1, unbiased=False, keepdim=True) + 1e-5).sqrt()
    refs = [torch.where(n >= 0, n, s * n).reshape(-1, C) for s in (0.2, 0.0)]
    runs = []
    for _ in range(2):
        a = torch.full((rows * HW, C), 7.0, dtype=torch.float16, device=DEV)
        wide = torch.full((rows * HW, 2 * C + 8), 7.0, dtype=torch.float16, device=DEV)
        ops.instnorm_act(xs[:, :C], rows, HW, a, 0.2, wide[:, C:2 * C], 0.0)
        runs.append((a.cpu(), wide.cpu()))
    (a, wide), (a2, wide2) = runs
    assert torch.equal(a, a2) and torch.equal(wide, wide2)
    assert float((wide[:, :C] - 7).abs().max()) == 0 and float((wide[:, 2 * C:] - 7).abs().max()) == 0      # no stray writes
    for name, got, ref in (("leaky", a, refs[0]), ("relu", wide[:, C:2 * C], refs[1])):
        d = (got.double() - ref).abs()
        worst = float((d / ref.abs().clamp_min(1.0)).max())
        print(f"instnorm rows{rows} HW{HW} C{C} {name}: worst |delta| / max(1, |ref|) = {worst:.3e} (bound {2 ** -10:.3e})")
        assert worst <= 2 ** -10
    # one output only, and identity statistics (the activated copies of a convolution output that has no norm): exact
    r = torch.empty(rows * HW, C, dtype=torch.float16, device=DEV)
    ops.instnorm_act(xs[:, :C], rows, HW, None, 1.0, r, 0.0)
    assert torch.equal(r.cpu(), wide[:, C:2 * C])
    ops.instnorm_act(xs[:, :C], rows, HW, r, 0.2, None, 0.0, identity=True)
    xf = x.reshape(-1, C).float()
    assert torch.equal(r.cpu(), torch.where(xf >= 0, xf, 0.2 * xf).half())


def test_first_layer_window_gemm(ops):
    """Conv2d(3, 64, 4, 2, 1) on the picture = skg_a2s_patch_f16 + one K = 64 GEMM, vs F.conv2d on the fp16-rounded operands."""
    from sketch2img_amd.anime2sketch import pack_conv_first
    g = torch.Generator().manual_seed(61)
    for B, H, W in [(2, 64, 96), (1, 256, 256), (3, 2, 2)]:
        x = torch.randn(B, 3, H, W, generator=g).half().float()
        w = (torch.randn(64, 3, 4, 4, generator=g) * 48 ** -0.5).half()
        b = torch.randn(64, generator=g).half()
        M = B * (H // 2) * (W // 2)
        buf = torch.zeros(M, 64 + 16, device=DEV, dtype=torch.float16)
        P = ops.a2s_patch(x.to(DEV))
        ops.gemm(P, pack_conv_first(w, DEV), out=buf[:, 8:72], bias=b.to(DEV))
        ref = nhwc(F.conv2d(x, w.float(), b.float(), stride=2, padding=1))
        e = report(f"first layer {B}x3x{H}x{W}", buf[:, 8:72].float().cpu(), ref)[0]
        stray = float(buf[:, :8].abs().max() + buf[:, 72:].abs().max())
        assert e < CONV_TOL and stray == 0 and float(P[:, 48:].abs().max()) == 0


def test_down_convolution(ops):
    """Conv2d(Cin, Cout, 4, 2, 1) = skg_conv4x4s2_f16 on pack_conv_down, including 2 x 2 -> 1 x 1 maps; output into a strided view."""
    from sketch2img_amd.anime2sketch import pack_conv_down
    g = torch.Generator().manual_seed(62)
    for rows, (ih, iw), cin, cout in [(2, (16, 16), 64, 128), (1, (2, 2), 512, 512), (3, (2, 2), 128, 64), (1, (8, 4), 128, 256),
                                       (2, (2, 4), 512, 512), (1, (64, 64), 64, 128)]:
        x = torch.randn(rows, cin, ih, iw, generator=g).half()
        w = (torch.randn(cout, cin, 4, 4, generator=g) * (16 * cin) ** -0.5).half()
        b = torch.randn(cout, generator=g).half()
        buf = torch.zeros(rows * (ih // 2) * (iw // 2), cout + 16, device=DEV, dtype=torch.float16)
        ops.conv4x4s2(nhwc(x).to(DEV), pack_conv_down(w, DEV), rows, ih, iw, out=buf[:, 8:8 + cout], bias=b.to(DEV))
        ref = nhwc(F.conv2d(x.float(), w.float(), b.float(), stride=2, padding=1))
        e = report(f"down conv rows{rows} {cin}->{cout} @{ih}x{iw}", buf[:, 8:8 + cout].float().cpu(), ref)[0]
        stray = float(buf[:, :8].abs().max() + buf[:, 8 + cout:].abs().max())
        assert e < CONV_TOL and stray == 0


def test_transposed_convolution(ops):
    """ConvTranspose2d(Cin, Cout, 4, 2, 1) = skg_convt4x4s2_f16 on pack_convt: 1 x 1 -> 2 x 2, Cin = 1024 (a concatenation buffer
    read through a view), Cout = 1 (padded to 8) with tanh; output into a strided view."""
    from sketch2img_amd.anime2sketch import pack_convt
    g = torch.Generator().manual_seed(63)
    for rows, (ih, iw), cin, cout, tanh in [(2, (8, 8), 128, 64, False), (2, (1, 1), 512, 512, False), (1, (4, 4), 1024, 512, False),
                                            (1, (2, 4), 1024, 512, False), (1, (32, 32), 128, 1, True), (2, (16, 8), 256, 64, True),
                                            (1, (128, 128), 128, 1, True)]:
        x = torch.randn(rows, cin, ih, iw, generator=g).half()
        w = (torch.randn(cin, cout, 4, 4, generator=g) * (4 * cin) ** -0.5).half()
        b = torch.randn(cout, generator=g).half()
        cp = max(cout, 8)
        bp = torch.zeros(cp, dtype=torch.float16)
        bp[:cout] = b
        xin = torch.zeros(rows * ih * iw, cin + 8, device=DEV, dtype=torch.float16)
        xin[:, :cin] = nhwc(x).to(DEV)
        buf = torch.zeros(rows * 4 * ih * iw, cp + 16, device=DEV, dtype=torch.float16)
        ops.convt4x4s2(xin[:, :cin], pack_convt(w, DEV, cout_pad=8), rows, ih, iw, out=buf[:, 8:8 + cp], bias=bp.to(DEV), tanh=tanh)
        ref = F.conv_transpose2d(x.float(), w.float(), b.float(), stride=2, padding=1)
        ref = nhwc(torch.tanh(ref) if tanh else ref)
        got = buf[:, 8:8 + cout].float().cpu()
        e = report(f"convT rows{rows} {cin}->{cout} @{ih}x{iw} tanh={tanh}", got, ref)[0]
        stray = float(buf[:, :8].abs().max() + buf[:, 8 + cp:].abs().max())
        assert e < CONV_TOL and stray == 0
        if cout < cp:
            assert float(buf[:, 8 + cout:8 + cp].abs().max()) == 0      # zero filters, zero bias: tanh(0)


def test_tail_kernel(ops):
    g = torch.Generator().manual_seed(64)
    B, H, W = 2, 16, 24
    Y = torch.zeros(B * H * W, 8, dtype=torch.float16)
    Y[:, 0] = torch.tanh(torch.randn(B * H * W, generator=g)).half()
    Y[::7, 0] = 0.5      # 1 - 0.5 = 0.5 is NOT below the threshold
    y = torch.empty(B, 1, H, W, device=DEV)
    m = torch.empty(B, 3, H, W, device=DEV)
    ops.a2s_tail(Y.to(DEV), B, H, W, y=y, mask=m)
    ref = Y[:, 0].float().reshape(B, 1, H, W)
    val = 1 - ref
    val[val < 0.5] = 0
    val[val >= 0.5] = 1
    assert torch.equal(y.cpu(), ref) and torch.equal(m.cpu(), val.expand(B, 3, H, W))


@pytest.mark.parametrize("name", ["256", "256x512"])
def test_generator_matches_the_reference_module(net, name):
    from sketch2img_amd import synthetic
    c = meta()["cases"][name]
    ref = torch.from_numpy(load_npz(f"anime2sketch_{name}.npz")["y"])
    x = synthetic.pictures(c["picture"], 1, c["H"], c["W"])
    y = net(x.to(DEV))
    assert y.shape == ref.shape and y.dtype == torch.float32
    r, m = report(f"anime2sketch {name} vs the reference module", y.cpu(), ref)
    print(f"  allowed: max {2 * c['emu_max_abs']:.3e} rel {2 * c['emu_rel_l2']:.3e}")
    assert m <= 2 * c["emu_max_abs"] and r <= 2 * c["emu_rel_l2"]
    # generate_sketch at the picture's own size (no resize): the binarised reference output, off the band around the threshold
    from sketch2img_amd.anime2sketch import generate_sketch
    mask = generate_sketch(net, x.to(DEV), fixed=(c["H"], c["W"])).cpu()
    val = 1 - ref
    keep = ((val - 0.5).abs() >= c["band"]).expand(1, 3, -1, -1)
    want = (val >= 0.5).float().expand(1, 3, -1, -1)
    assert mask.shape == (1, 3, c["H"], c["W"]) and set(mask.unique().tolist()) <= {0.0, 1.0}
    print(f"  mask: {float((mask != want).float().mean()):.2e} of the pixels differ, {float(((mask != want) & keep).float().mean()):.2e} off the band")
    assert torch.equal(mask[keep], want[keep]) and float((~keep).float().mean()) <= 0.05


def test_generator_at_the_trainers_size(net):
    """1024 x 1024 (generate_sketch's `fixed`): 16 x 16 block means of y and of the binarised mask vs the reference module's."""
    from sketch2img_amd import synthetic
    c = meta()["cases"]["1024_blocks"]
    d = load_npz("anime2sketch_1024_blocks.npz")
    x = synthetic.pictures(c["picture"], 1, 1024, 1024).to(DEV)
    y = net(x)
    yb = F.avg_pool2d(y.double().cpu(), 16)[0, 0]
    mb = F.avg_pool2d(net.sketch_mask(x)[:, :1].double().cpu(), 16)[0, 0]
    ry, my = report("anime2sketch 1024 y block means", yb, torch.from_numpy(d["y_blocks"]).double())
    rm, mm = report("anime2sketch 1024 mask block means", mb, torch.from_numpy(d["mask_blocks"]).double())
    print(f"  allowed: y max {2 * c['emu_y_blocks_max_abs']:.3e} rel {2 * c['emu_y_blocks_rel_l2']:.3e}; "
          f"mask max {2 * c['emu_mask_blocks_max_abs']:.3e} rel {2 * c['emu_mask_blocks_rel_l2']:.3e}")
    assert my <= 2 * c["emu_y_blocks_max_abs"] and ry <= 2 * c["emu_y_blocks_rel_l2"]
    assert mm <= 2 * c["emu_mask_blocks_max_abs"] and rm <= 2 * c["emu_mask_blocks_rel_l2"]


def test_batch_equals_single_runs(net):
    from sketch2img_amd import synthetic
    x = synthetic.pictures(5, 2, 256, 512).to(DEV)
    both = net(x).clone()
    assert torch.equal(both[0:1], net(x[0:1])) and torch.equal(both[1:2], net(x[1:2]))
    assert torch.equal(both, net(x))      # and a second run of the batch: same bits
    six = torch.cat([x, x.flip(0), x])    # more pictures than one pass takes
    out = net(six)
    assert torch.equal(out[:2], both) and torch.equal(out[2:4], both.flip(0)) and torch.equal(out[4:], both)


def test_sketch_latents_and_the_pipeline(net):
    """sketch_latents = trainer.py:220 composed by hand, bit for bit; the result drives AntiGradientPipeline(sketch_image=)."""
    from modules.latent_predictor import LatentEdgePredictor
    from modules.pipeline import AntiGradientPipeline
    from sketch2img_amd import synthetic
    from sketch2img_amd.anime2sketch import generate_sketch, sketch_latents
    from sketch2img_amd.config import TINY, TINY_VAE
    from sketch2img_amd.vae import AutoencoderKL
    vae = AutoencoderKL(TINY_VAE).to("cuda")
    x = synthetic.pictures(7, 1, 256, 256).to(DEV)
    lat = sketch_latents(x, net, vae, generator=torch.Generator(device="cuda").manual_seed(11))
    sk = generate_sketch(net, x)      # through 1024 x 1024 and back
    assert sk.shape == x.shape
    by_hand = vae.encode(sk).latent_dist.sample(torch.Generator(device="cuda").manual_seed(11)) * 0.18215
    assert lat.shape == (1, 4, 32, 32) and torch.equal(lat, by_hand) and bool(torch.isfinite(lat).all())
    pipe = AntiGradientPipeline.from_pretrained(None, unet_config=TINY, torch_dtype=torch.float16).to("cuda")
    lgp = LatentEdgePredictor(synthetic.lgp_input_dim(TINY), 4, 9)
    lgp.load_state_dict(synthetic.lgp_state_dict(synthetic.lgp_input_dim(TINY)))
    lgp.to(pipe.unet.device, dtype=pipe.unet.dtype)
    pipe.setup_lgp(lgp)
    start = torch.randn(1, 4, 32, 32, generator=torch.Generator().manual_seed(12))
    out = pipe("a cat", height=256, width=256, num_inference_steps=2, latents=start, sketch_image=lat, output_type="latent")
    assert out.shape == (1, 4, 32, 32) and bool(torch.isfinite(out).all()) and [a is not None for a in pipe.last_aux] == [True, True]
