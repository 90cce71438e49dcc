"""GPU parity tests (-m gpu): every libskg.so kernel, called through the C ABI, against plain PyTorch
fp32 math on the same fp16-rounded inputs.  Tolerances are stated per test; "rel" is the relative
Frobenius error ||got - ref|| / ||ref|| and is dominated by the final fp16 rounding of the output
(2^-11 = 4.9e-4 per element) unless noted."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests.util import rel_err, report

pytestmark = pytest.mark.gpu

FP16_RND = 6e-4      # one fp16 output rounding, relative Frobenius


def dev():
    return torch.device("cuda:0")


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).half()


@pytest.fixture(scope="module")
def ops():
    from sketch2img_amd import ops as o
    return o


# ---------------------------------------------------------------------------------------------- GEMM
@pytest.mark.parametrize("M,N,K", [(300, 320, 64), (1024, 1280, 320), (4099, 64, 512), (65, 8, 32),
                                   (33000, 256, 128), (16384, 640, 640)])
def test_gemm_plain(ops, M, N, K):
    A, B = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5)
    C = ops.gemm(A.to(dev()), B.to(dev()))
    ref = A.float() @ B.float().t()
    r, _ = report(f"gemm {M}x{N}x{K}", C.float(), ref)
    assert r < FP16_RND


def test_gemm_epilogue_and_views(ops):
    M, N, K = 777, 320, 96
    Abig, Bbig = rnd(M, K + 40, seed=3), rnd(N, K + 64, seed=4, scale=0.1)
    bias, res = rnd(N, seed=5), rnd(M, N + 8, seed=6)
    A, B = Abig[:, 8:8 + K], Bbig[:, 32:32 + K]                # column-slice views: lda/ldb > K
    out = torch.zeros(M, N + 16, device=dev(), dtype=torch.float16)
    ops.gemm(Abig.to(dev())[:, 8:8 + K], Bbig.to(dev())[:, 32:32 + K], out=out[:, 8:8 + N],
             bias=bias.to(dev()), residual=res.to(dev())[:, :N], alpha=0.5, relu=True)
    ref = torch.relu(0.5 * (A.float() @ B.float().t() + bias.float()) + res[:, :N].float())
    r, _ = report("gemm epilogue", out[:, 8:8 + N].float(), ref)
    assert r < FP16_RND
    assert out[:, :8].abs().max() == 0 and out[:, 8 + N:].abs().max() == 0      # no stray writes
    o32 = ops.gemm(A.contiguous().to(dev()), B.contiguous().to(dev()), out_f32=True)
    r, _ = report("gemm f32 out", o32, A.float() @ B.float().t())
    assert o32.dtype == torch.float32 and r < 2e-6 * math.sqrt(K) + 1e-6


@pytest.mark.parametrize("M,N,K,tag", [
    (777, 320, 128, "fp16-staged epilogue, ragged rows, strided output"),
    (2048, 5120, 640, "XCD grid 1 x 8 (weight-heavy: every L2 owns one column block)"),
    (4096, 1280, 1280, "three-stage pipeline, exactly 256 tiles"),
    (4096, 1280, 8192, "split-K at exactly 256 tiles"),
    (2048, 1280, 1280, "128 x 64 tile, three stages"),
    (512, 10240, 1280, "256 x 320 tile, two fp16 slabs")])
def test_gemm_residual_free_epilogue_and_launch_variants(ops, M, N, K, tag):
    """No residual -> the fp16-staged epilogue (bias, alpha, ReLU in registers, one rounding) on every launch variant
    the host can pick: result == round(relu(alpha * (A B^T + bias))) up to the fp32 summation order."""
    A, B, bias = rnd(M, K, seed=11), rnd(N, K, seed=12, scale=K ** -0.5), rnd(N, seed=13)
    out = torch.zeros(M, N + 16, device=dev(), dtype=torch.float16)
    ops.gemm(A.to(dev()), B.to(dev()), out=out[:, 8:8 + N], bias=bias.to(dev()), alpha=0.75, relu=True)
    ref = torch.relu(0.75 * (A.float() @ B.float().t() + bias.float()))
    assert report(f"gemm {tag}", out[:, 8:8 + N].float().cpu(), ref)[0] < FP16_RND
    assert out[:, :8].abs().max() == 0 and out[:, 8 + N:].abs().max() == 0      # no stray writes
    res = rnd(M, N, seed=14)
    o2 = ops.gemm(A.to(dev()), B.to(dev()), bias=bias.to(dev()), residual=res.to(dev()))
    assert report(f"gemm +res {tag}", o2.float().cpu(), A.float() @ B.float().t() + bias.float() + res.float())[0] < FP16_RND


@pytest.mark.parametrize("M,K,N", [(4096, 320, 960), (4096, 640, 960), (6144, 320, 448)])
def test_gemm_three_stage_tile_with_two_workgroups_per_cu_is_repeatable(ops, M, K, N):
    """The 128 x 64 three-stage instantiation with more tiles than CUs (two co-resident workgroups, counted vmcnt):
    ten launches each with and without residual, every one of them correct."""
    x, Wt, b, r = rnd(M, K, seed=31), rnd(N, K, seed=32, scale=K ** -0.5), rnd(N, seed=33), rnd(M, N, seed=34)
    d = dev()
    xd, wd, bd, rd = x.to(d), Wt.to(d), b.to(d), r.to(d)
    ref = x.float() @ Wt.float().t() + b.float()
    for _ in range(10):
        assert rel_err(ops.gemm(xd, wd, bias=bd).float().cpu(), ref) < FP16_RND
        assert rel_err(ops.gemm(xd, wd, bias=bd, residual=rd).float().cpu(), ref + r.float()) < FP16_RND


def test_three_stage_pipeline_bitwise_equals_two_stage_under_stress():
    """the three-stage (counted vmcnt) instantiations ship on the hot path.  1000 launches over random
    shapes - 128 x 64 tiles with two co-resident workgroups per CU, 128 x 160 tiles with one - interleaved with
    unrelated kernels: every launch reproduces its case's first output bit for bit, and the outputs equal, bit for bit,
    those of the SAME launches forced through the two-stage pipeline (SKG_NO_NS3=1), whose barrier-per-tile structure
    has no counted wait to get wrong."""
    import os, re, subprocess, sys
    script = os.path.join(os.path.dirname(__file__), "_ns3_stress.py")
    outs = {}
    for tag, env in (("ns3", {}), ("ns2", {"SKG_NO_NS3": "1"})):
        r = subprocess.run([sys.executable, script, "1000"], env=dict(os.environ, **env), capture_output=True, text=True,
                           timeout=900)
        print(r.stdout[-1500:], r.stderr[-1500:])
        assert r.returncode == 0 and "ALL OK" in r.stdout, tag
        outs[tag] = {(a, b): c for a, b, c in re.findall(r"HASH (.*?) v\d+ (m\d) (-?\d+)", r.stdout)}
        if tag == "ns3":
            assert int(re.search(r"three-stage (\d+)", r.stdout).group(1)) >= 30      # the stress really hits NS = 3
    assert outs["ns3"].keys() == outs["ns2"].keys() and len(outs["ns3"]) >= 40
    diff = [k for k in outs["ns3"] if outs["ns3"][k] != outs["ns2"][k]]
    assert not diff, f"three-stage output differs from two-stage: {diff[:5]}"


def test_split_k_deep_ring_bitwise_equals_two_stage(ops):
    """Round 5: split-K launches with at most one workgroup per CU run on the three-stage LDS ring (SPLIT_NS_DEFAULT; SKG_SPLIT_NS is
    read per launch).  Same K slices, same order inside a slice: the fp32 slabs - and so the reduced outputs - must equal the
    two-stage launch's bit for bit (also the four-stage ring the tuning switch reaches), on GEMM and implicit-GEMM shapes of the
    8 x 8 / 16 x 16 levels incl. a ragged last slice; and be right."""
    import os
    d = dev()
    old = os.environ.get("SKG_SPLIT_NS")
    try:
        for (M, N, K, cin) in ((512, 1280, 10240, 0), (1024, 1280, 5120, 0), (512, 1280, 11520, 1280), (1024, 1280, 23040, 2560), (384, 640, 2880 + 64 * 9, 384)):
            conv = cin > 0
            if conv:
                hw = 8
                rows = M // (hw * hw)
                x, w = rnd(M, cin, seed=5).to(d), rnd(N, 9 * cin, seed=6, scale=(9 * cin) ** -0.5).to(d)
            else:
                x, w = rnd(M, K, seed=5).to(d), rnd(N, K, seed=6, scale=K ** -0.5).to(d)
            b, r = rnd(N, seed=7).to(d), rnd(M, N, seed=8).to(d)
            outs = {}
            for ns in ("2", "3", "4"):
                os.environ["SKG_SPLIT_NS"] = ns
                outs[ns] = (ops.conv3x3(x, w, rows, hw, hw, 0, bias=b, residual=r) if conv else ops.gemm(x, w, bias=b, residual=r)).clone()
            torch.cuda.synchronize()
            assert torch.equal(outs["3"], outs["2"]) and torch.equal(outs["4"], outs["2"]), (M, N, K, cin)
            if not conv:
                ref = x.float() @ w.float().t() + b.float() + r.float()
                assert rel_err(outs["3"], ref) < 1.5 * FP16_RND
    finally:
        if old is None:
            os.environ.pop("SKG_SPLIT_NS", None)
        else:
            os.environ["SKG_SPLIT_NS"] = old


def test_gemm_rejects_bad_args(ops):
    from sketch2img_amd._lib import SkgError
    A, B = rnd(16, 24).to(dev()), rnd(8, 24).to(dev())        # K % 32 != 0
    with pytest.raises(SkgError):
        ops.gemm(A, B)


@pytest.mark.parametrize("force,env", [("320", {}), ("160", {}), ("128", {}), ("64", {})])
def test_forced_tiles(force, env):
    """Every tile configuration on small ragged shapes."""
    import os, subprocess, sys
    e = dict(os.environ, SKG_FORCE_BN=force, **env)
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "_tile_check.py")], env=e,
                       capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and "ALL OK" in r.stdout


def test_gemm8_pingpong_320_tile_convolutions(ops):
    """The 256 x 320 ping-pong tile (gemm8.hip) is what the 64 x 64-level 3x3 convolutions run by default: check that
    the dispatcher really takes it for those shapes and that it agrees with F.conv2d (bias, residual, ragged last tile).
    (The withdrawn 256 x 160 form and the persistent gemm4 kernel left the tree: EXPERIMENTS.md, "Where the withdrawn code is".)"""
    from sketch2img_amd._lib import lib
    g = torch.Generator().manual_seed(17)
    for rows, hw, cin, cout, res in [(16, 64, 128, 320, True), (15, 64, 128, 320, False), (16, 64, 320, 320, True)]:
        assert lib.skg_gemm_variant(rows * hw * hw, cout, 9 * cin, cin, 1) == 8320
        x = torch.randn(rows, cin, hw, hw, generator=g).half()
        w = (torch.randn(cout, cin, 3, 3, generator=g) * (9 * cin) ** -0.5).half()
        b = torch.randn(cout, generator=g).half()
        r = torch.randn(rows * hw * hw, cout, generator=g).half().to(dev()) if res else None
        out = ops.conv3x3(x.permute(0, 2, 3, 1).reshape(-1, cin).contiguous().to(dev()),
                          w.permute(0, 2, 3, 1).reshape(cout, -1).contiguous().to(dev()), rows, hw, hw, 0, bias=b.to(dev()), residual=r)
        ref = F.conv2d(x.float().to(dev()), w.float().to(dev()), b.float().to(dev()), padding=1).permute(0, 2, 3, 1).reshape(-1, cout)
        if res:
            ref = ref + r.float()
        e = float((out.float() - ref).norm() / ref.norm())
        print(f"gemm8 conv rows{rows} {cin}->{cout} @{hw}: rel {e:.2e}")
        assert e < 5e-4


def test_conv_up2_polyphase(ops):
    """skg_conv3x3_up2_f16: nearest-2x upsample + 3x3 conv as four 4-tap convolutions over the low-res input (pre-summed taps)
    vs F.interpolate + F.conv2d, and vs the 9-tap UP2 gather form of skg_conv3x3_f16; output into a strided view."""
    from sketch2img_amd.unet import pack_conv, pack_conv_up2
    g = torch.Generator().manual_seed(53)
    for rows, hw, cin, cout in [(2, 16, 64, 160), (3, 8, 128, 320), (16, 32, 640, 640), (2, (8, 24), 64, 320), (5, (40, 24), 128, 160),
                                (1, 64, 512, 512), (1, 128, 512, 512), (1, 64, 256, 256)]:      # last three: VAE decoder (128 x 64 / 128 x 128 tiles)
        ih, iw = hw if isinstance(hw, tuple) else (hw, hw)
        x = torch.randn(rows, cin, ih, iw, generator=g).half()
        w = (torch.randn(cout, cin, 3, 3, generator=g) * (9 * cin) ** -0.5).half()
        b = torch.randn(cout, generator=g).half()
        xs = nhwc(x).to(dev())
        buf = torch.zeros(rows * 4 * ih * iw, cout + 16, device=dev(), dtype=torch.float16)
        ops.conv_up2(xs, pack_conv_up2(w, dev()), rows, ih, iw, out=buf[:, 8:8 + cout], bias=b.to(dev()))
        ref = F.conv2d(F.interpolate(x.float().to(dev()), scale_factor=2.0, mode="nearest"), w.float().to(dev()), b.float().to(dev()),
                       padding=1).permute(0, 2, 3, 1).reshape(-1, cout)
        nine = ops.conv3x3(xs, pack_conv(w, dev()), rows, ih, iw, ops.CONV_UP2, bias=b.to(dev()))
        e = float((buf[:, 8:8 + cout].float() - ref).norm() / ref.norm())
        e9 = float((nine.float() - ref).norm() / ref.norm())
        stray = float(buf[:, :8].abs().max() + buf[:, 8 + cout:].abs().max())
        print(f"conv_up2 polyphase rows{rows} {cin}->{cout} @{ih}x{iw} -> 2x: rel {e:.2e} (9-tap form {e9:.2e}) stray {stray}")
        assert e < 5e-4 and stray == 0


def test_gemm_segmented_output_rows(ops):
    """skg_gemm_f16_rows: one GEMM over all batch rows, product row m stored to row (m // seg) * stride + m % seg of a longer
    per-row buffer (the image tokens' K / V of clip_guided_attn) == one GEMM per batch row into its slot, bit for bit; the
    slots' tails (the sketch tokens' rows) stay untouched; a segment length that is not a multiple of the 128-row tile."""
    g = torch.Generator().manual_seed(91)
    for rows, n_img, L, C in [(8, 9216, 9216 + 264, 320), (3, 1000, 1264, 320), (4, 2304, 2568, 640)]:
        z = torch.randn(rows * n_img, C, generator=g).half().to(dev())
        w = (torch.randn(2 * C, C, generator=g) * C ** -0.5).half().to(dev())
        a = torch.full((rows * L, 2 * C + 8), 7.0, device=dev(), dtype=torch.float16)
        b = a.clone()
        ops.gemm_rows(z, w, a[:, :2 * C], n_img, L)
        for r in range(rows):
            ops.gemm(z[r * n_img:(r + 1) * n_img], w, out=b[r * L:r * L + n_img, :2 * C])
        ref = z[:n_img].float() @ w.float().t()
        e = float((a[:n_img, :2 * C].float() - ref).norm() / ref.norm())
        print(f"gemm_rows rows{rows} seg{n_img} stride{L} C{C}: rel {e:.2e}, equal to the per-row launches: {torch.equal(a, b)}")
        assert e < 4e-4 and torch.equal(a, b)


def test_conv4x4s2_is_the_dgrad_of_upsample_conv(ops):
    """skg_conv4x4s2_f16 with unet.pack_conv_up2_dgrad: the data gradient of nearest-2x upsample + 3x3 conv as ONE 4 x 4
    stride-2 convolution over dY, vs torch autograd of F.interpolate + F.conv2d (fp32), and vs the path it replaces (9-tap
    dgrad at the upsampled size + 2 x 2 sum-pool); split-K and single-launch shapes, output into a strided view."""
    from sketch2img_amd.unet import pack_conv_dgrad, pack_conv_up2_dgrad
    g = torch.Generator().manual_seed(54)
    for rows, hw, cin, cout in [(2, 8, 64, 128), (8, 32, 640, 640), (8, 8, 1280, 1280), (3, 16, 128, 320), (2, (6, 20), 64, 64)]:
        ih, iw = hw if isinstance(hw, tuple) else (hw, hw)
        w = (torch.randn(cout, cin, 3, 3, generator=g) * (9 * cin) ** -0.5).half()
        dy = torch.randn(rows, cout, 2 * ih, 2 * iw, generator=g).half()
        x = torch.zeros(rows, cin, ih, iw, device=dev(), requires_grad=True)
        y = F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), w.float().to(dev()), padding=1)
        ref, = torch.autograd.grad(y, x, dy.float().to(dev()))
        ref = ref.permute(0, 2, 3, 1).reshape(-1, cin)
        dys = nhwc(dy).to(dev())
        buf = torch.zeros(rows * ih * iw, cin + 16, device=dev(), dtype=torch.float16)
        ops.conv4x4s2(dys, pack_conv_up2_dgrad(w, dev()), rows, 2 * ih, 2 * iw, out=buf[:, 8:8 + cin])
        old = ops.sumpool2x2(ops.conv3x3(dys, pack_conv_dgrad(w, dev()), rows, 2 * ih, 2 * iw), rows, ih, iw)
        e = float((buf[:, 8:8 + cin].float() - ref).norm() / ref.norm())
        e9 = float((old.float() - ref).norm() / ref.norm())
        stray = float(buf[:, :8].abs().max() + buf[:, 8 + cin:].abs().max())
        print(f"conv4x4s2 rows{rows} dY {cout}ch @{2 * ih}x{2 * iw} -> dX {cin}ch @{ih}x{iw}: rel {e:.2e} (dgrad + sum-pool {e9:.2e}) stray {stray}")
        assert e < 5e-4 and stray == 0


def test_declined_launches_fall_back_to_the_forms_they_replaced(ops, monkeypatch):
    """SKG_E_UNSUPPORTED from the three LDS-DMA-only entry points (an operand of 2 GiB or more) is not an error of the caller:
    ops.conv_up2 falls back to the 9-tap UP2 gather form, ops.conv4x4s2 to the 9-tap dgrad + 2 x 2 sum-pool, ops.gemm_rows to one
    GEMM per batch row - the entry points return -2 here by substitution, the results are those of the replaced paths; any other
    error code still raises; release_stream drops a side stream's slab and the library's entry."""
    from sketch2img_amd import _lib
    from sketch2img_amd.unet import pack_conv, pack_conv_dgrad, pack_conv_up2, pack_conv_up2_dgrad
    g = torch.Generator().manual_seed(57)
    rows, ih, iw, cin, cout = 2, 16, 16, 64, 160
    x = nhwc(torch.randn(rows, cin, ih, iw, generator=g).half()).to(dev())
    w = (torch.randn(cout, cin, 3, 3, generator=g) * (9 * cin) ** -0.5).half()
    b = torch.randn(cout, generator=g).half().to(dev())
    dy = nhwc(torch.randn(rows, cout, 2 * ih, 2 * iw, generator=g).half()).to(dev())
    z = torch.randn(3 * 1000, 320, generator=g).half().to(dev())
    wz = (torch.randn(640, 320, generator=g) * 320 ** -0.5).half().to(dev())
    nine = ops.conv3x3(x, pack_conv(w, dev()), rows, ih, iw, ops.CONV_UP2, bias=b)
    old = ops.sumpool2x2(ops.conv3x3(dy, pack_conv_dgrad(w, dev()), rows, 2 * ih, 2 * iw), rows, ih, iw)
    seg = torch.full((3 * 1264, 640), 7.0, device=dev(), dtype=torch.float16)
    ops.gemm_rows(z, wz, seg, 1000, 1264)
    for name in ("skg_conv3x3_up2_f16", "skg_conv4x4s2_f16", "skg_gemm_f16_rows"):
        monkeypatch.setattr(ops.lib, name, lambda *a: -2)
    up = ops.conv_up2(x, pack_conv_up2(w, dev()), rows, ih, iw, bias=b, W9=pack_conv(w, dev()))
    dx = ops.conv4x4s2(dy, pack_conv_up2_dgrad(w, dev()), rows, 2 * ih, 2 * iw, W9T=pack_conv_dgrad(w, dev()))
    seg2 = torch.full_like(seg, 7.0)
    ops.gemm_rows(z, wz, seg2, 1000, 1264)
    assert torch.equal(up, nine) and torch.equal(dx, old) and torch.equal(seg, seg2)
    with pytest.raises(_lib.SkgError) as ei:      # without the caller's 9-tap pack there is nothing to fall back to
        ops.conv_up2(x, pack_conv_up2(w, dev()), rows, ih, iw, bias=b)
    assert ei.value.rc == -2
    monkeypatch.setattr(ops.lib, "skg_gemm_f16_rows", lambda *a: -1)
    with pytest.raises(_lib.SkgError) as ei:
        ops.gemm_rows(z, wz, seg2, 1000, 1264)
    assert ei.value.rc == -1
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ops.groupnorm_stats(z, 3, 1000, 32, 1e-5)
        ops.gemm(z, wz)
    side.synchronize()
    key = (side.device.index, side.cuda_stream)
    assert key in ops._workspace
    ops.release_stream(side)
    assert key not in ops._workspace and not any(k[1][1] == side.cuda_stream for k in ops._scratch)
    with torch.cuda.stream(side):      # and the stream is usable again afterwards (a new slab is registered)
        again = ops.gemm(z, wz)
    side.synchronize()
    assert torch.equal(again, ops.gemm(z, wz))
    ops.release_stream(side)


def test_hilo_pair_epilogue_and_norms(ops):
    """Accuracy mode primitives (skg_*_hilo): a GEMM / conv whose output and residual are (hi, lo) fp16 pairs carries
    ~22 mantissa bits (hi + lo vs an fp64 reference of the same fp16 operands: fp32-accumulation error only), hi alone is
    the plain fp16 result; GroupNorm / LayerNorm of a pair equal torch on hi + lo."""
    g = torch.Generator().manual_seed(31)
    for M, N, K, res in [(1024, 320, 640, True), (300, 1280, 320, False), (4096, 640, 1280, True)]:
        a = torch.randn(M, K, generator=g).half().to(dev())
        w = (torch.randn(N, K, generator=g) * K ** -0.5).half().to(dev())
        b = torch.randn(N, generator=g).half().to(dev())
        r32 = torch.randn(M, N, generator=g).to(dev()) if res else None
        rbuf = None
        if res:
            rbuf = torch.empty(M, 2 * N, device=dev(), dtype=torch.float16)
            rbuf[:, :N] = r32.half()
            rbuf[:, N:] = (r32 - rbuf[:, :N].float()).half()
            r32 = rbuf[:, :N].float() + rbuf[:, N:].float()
        out = torch.zeros(M, 2 * N + 8, device=dev(), dtype=torch.float16)
        ops.gemm(a, w, out=out[:, :N], out_lo=out[:, N:2 * N], bias=b, alpha=0.75,
                 residual=rbuf[:, :N] if res else None, residual_lo=rbuf[:, N:] if res else None)
        ref = 0.75 * (a.double() @ w.double().t() + b.double()) + (r32.double() if res else 0)
        got = out[:, :N].double() + out[:, N:2 * N].double()
        e = float((got - ref).norm() / ref.norm())
        e_hi = float((out[:, :N].double() - ref).norm() / ref.norm())
        plain = ops.gemm(a, w, bias=b, alpha=0.75, residual=rbuf[:, :N].contiguous() if res else None)
        print(f"hilo gemm M{M} N{N} K{K} res{int(res)}: pair rel {e:.2e}, hi alone {e_hi:.2e}")
        assert e < 2e-6 and 1e-4 < e_hi < 6e-4 and float(out[:, 2 * N:].abs().max()) == 0
        # hi is the plain fp16 result up to the last bit (the two epilogues apply bias and alpha in a different fp32 order)
        assert float((out[:, :N].float() - plain.float()).abs().max()) <= 2.0 ** -9 * float(plain.float().abs().max())
    # 3x3 conv with a pair as the K-doubled operand ([hi | lo] x [W | W]) and a pair output
    rows, hw, cin, cout = 2, 16, 64, 320
    x32 = torch.randn(rows, cin, hw, hw, generator=g)
    w = (torch.randn(cout, cin, 3, 3, generator=g) * (9 * cin) ** -0.5).half()
    xp = torch.empty(rows * hw * hw, 2 * cin, device=dev(), dtype=torch.float16)
    xn = nhwc(x32).to(dev())
    xp[:, :cin] = xn.half()
    xp[:, cin:] = (xn - xp[:, :cin].float()).half()
    w2 = torch.cat([w, w], 1).permute(0, 2, 3, 1).reshape(cout, -1).contiguous().to(dev())
    o = torch.empty(rows * hw * hw, 2 * cout, device=dev(), dtype=torch.float16)
    ops.conv3x3(xp, w2, rows, hw, hw, 0, out=o[:, :cout], out_lo=o[:, cout:])
    xs = (xp[:, :cin].double() + xp[:, cin:].double()).reshape(rows, hw, hw, cin).permute(0, 3, 1, 2)
    ref = F.conv2d(xs, w.double().to(dev()), padding=1).permute(0, 2, 3, 1).reshape(-1, cout)
    e = float(((o[:, :cout].double() + o[:, cout:].double()) - ref).norm() / ref.norm())
    print(f"hilo conv pair operand + pair output: rel {e:.2e}")
    assert e < 2e-6
    # norms of a pair
    rows, HW, C, G = 2, 256, 320, 32
    v = 3 * torch.randn(rows * HW, C, generator=g).to(dev()) + 1.5
    pr = torch.empty(rows * HW, 2 * C, device=dev(), dtype=torch.float16)
    pr[:, :C] = v.half()
    pr[:, C:] = (v - pr[:, :C].float()).half()
    vs = pr[:, :C].float() + pr[:, C:].float()
    ga, be = (1 + 0.1 * torch.randn(C, generator=g)).half().to(dev()), (0.1 * torch.randn(C, generator=g)).half().to(dev())
    y = ops.groupnorm_hilo(pr[:, :C], pr[:, C:], rows, HW, G, 1e-5, ga, be, True)
    ref = F.silu(F.group_norm(vs.reshape(rows, HW, C).permute(0, 2, 1), G, ga.float(), be.float(), 1e-5)).permute(0, 2, 1).reshape(-1, C)
    e = float((y.float() - ref).norm() / ref.norm())
    y16 = ops.groupnorm(pr[:, :C].contiguous(), rows, HW, G, 1e-5, ga, be, True)[0]
    e16 = float((y16.float() - ref).norm() / ref.norm())
    print(f"hilo groupnorm: rel {e:.2e} (fp16-input kernel on hi alone: {e16:.2e})")
    assert e < 4e-4 and e <= e16 * 1.05
    z = ops.layernorm_hilo(pr[:, :C], pr[:, C:], ga, be)
    refl = F.layer_norm(vs, (C,), ga.float(), be.float(), 1e-5)
    e = float((z.float() - refl).norm() / refl.norm())
    print(f"hilo layernorm: rel {e:.2e}")
    assert e < 4e-4


@pytest.mark.parametrize("kind,rows,H,Cin,Cout,res", [
    ("conv", 16, 64, 320, 320, True),      # 256 x 320 ping-pong tile (gemm8.hip) with the pair epilogue + statistics
    ("conv", 16, 64, 320, 320, False),
    ("conv", 4, 32, 640, 640, True),       # 128 x 160 two-stage tile + statistics
    ("conv", 2, 32, 640, 640, False),      # <= 256 tiles: the three-stage instantiation
    ("conv", 2, 16, 1280, 1280, True),     # split-K: the pair epilogue lives in the reduce kernel, statistics from the stand-alone pass
    ("conv", 2, 8, 1280, 1280, True),
    ("down", 4, 64, 640, 320, False),      # stride 2 on a K-doubled pair operand
    ("gemm", 4, 64, 640, 320, True),       # proj_out: [hi | lo] x [W | W] + pair residual + statistics
    ("gemm", 2, 16, 1280, 1280, True)])
def test_hilo_producers_with_groupnorm_sums(ops, kind, rows, H, Cin, Cout, res):
    """Accuracy mode on every instantiation the default mode uses: pair output (+ pair residual) carries fp32 accuracy
    (hi + lo vs fp64), hi equals the plain launch's fp16 output, the GroupNorm partial sums are those of hi, and
    groupnorm_hilo(partial=) equals torch on hi + lo."""
    d = dev()
    G = 32
    mode = {"conv": ops.CONV_S1, "down": ops.CONV_S2}.get(kind)
    OH = H // 2 if kind == "down" else H
    M, HW = rows * OH * OH, OH * OH
    want_gn = HW % 128 == 0                  # (8 x 8 maps: the one-launch GroupNorm keeps its own statistics)
    x = (rnd(rows * H * H, Cin, seed=1).float() * 0.5).half().to(d)
    b = rnd(Cout, seed=3).to(d)
    rp = None
    if res:
        r32 = torch.randn(M, Cout, generator=torch.Generator().manual_seed(4)).to(d)
        rp = ops.Pair.empty(M, Cout, d)
        rp.hi.copy_(r32.half()); rp.lo.copy_((r32 - rp.hi.float()).half())
    out = ops.Pair.empty(M, Cout, d)
    kw = dict(bias=b, residual=rp.hi if res else None, residual_lo=rp.lo if res else None)
    if kind == "gemm":
        w = (rnd(Cout, Cin, seed=2).float() * Cin ** -0.5).half().to(d)
        part = ops.gemm(x, w, out=out.hi, out_lo=out.lo, gn_stats=(HW, G) if want_gn else None, **kw)
        part = part[1] if want_gn else None
        plain = ops.gemm(x, w, bias=b, residual=rp.hi.contiguous() if res else None)
        ref = x.double() @ w.double().t() + b.double()
    else:
        w4 = (torch.randn(Cout, Cin, 3, 3, generator=torch.Generator().manual_seed(2)) * (9 * Cin) ** -0.5).half()
        w = w4.permute(0, 2, 3, 1).reshape(Cout, -1).contiguous().to(d)
        part = ops.conv3x3(x, w, rows, H, H, mode, out=out.hi, out_lo=out.lo, gn_groups=G if want_gn else None, **kw)
        part = part[1] if want_gn else None
        plain = ops.conv3x3(x, w, rows, H, H, mode, bias=b, residual=rp.hi.contiguous() if res else None)
        xs = x.double().reshape(rows, H, H, Cin).permute(0, 3, 1, 2)
        ref = F.conv2d(xs, w4.double().to(d), padding=1, stride=2 if kind == "down" else 1).permute(0, 2, 3, 1).reshape(M, Cout) + b.double()
    if res:
        ref = ref + rp.hi.double() + rp.lo.double()
    e = float(((out.hi.double() + out.lo.double()) - ref).norm() / ref.norm())
    e_hi = float((out.hi.double() - ref).norm() / ref.norm())
    print(f"hilo {kind} rows{rows} H{H} {Cin}->{Cout} res={res}: pair rel {e:.2e}, hi alone {e_hi:.2e}")
    assert e < 3e-6 and 1e-4 < e_hi < 6e-4
    # hi is the plain launch's output (up to the last bit where the residual's lo part moves a rounding)
    assert float((out.hi.float() - plain.float()).abs().max()) <= 2.0 ** -9 * float(plain.float().abs().max())
    cpg = Cout // G
    ga, be = (1 + 0.2 * rnd(Cout, seed=5).float()).half().to(d), (0.2 * rnd(Cout, seed=6).float()).half().to(d)
    vs = (out.hi.float() + out.lo.float()).reshape(rows, HW, Cout).permute(0, 2, 1)
    nref = F.silu(F.group_norm(vs.double(), G, ga.double(), be.double(), 1e-5)).permute(0, 2, 1).reshape(M, Cout)
    n0, st0 = ops.groupnorm_hilo(out.hi, out.lo, rows, HW, G, 1e-5, ga, be, True, want_stats=True)
    assert float((n0.double() - nref).norm() / nref.norm()) < 4e-4
    # pair OUTPUT of the norm (conv_norm_out in front of conv_out): hi + lo carries fp32 accuracy, hi is the fp16 output
    npair = ops.Pair.empty(M, Cout, d)
    ops.groupnorm_hilo(out.hi, out.lo, rows, HW, G, 1e-5, ga, be, True, out=npair.hi, out_lo=npair.lo, partial=part)
    assert float(((npair.hi.double() + npair.lo.double()) - nref).norm() / nref.norm()) < 3e-5
    assert float((npair.hi.double() - nref).norm() / nref.norm()) < 4e-4
    if want_gn:
        yf = out.hi.float().reshape(rows, HW // 128, 128, G, cpg)
        sref = torch.stack([yf.sum(dim=(2, 4)), (yf * yf).sum(dim=(2, 4))], dim=-1)
        got = part.buf.view(rows, HW // 128, G, 2)
        err = ((got - sref).abs() / (sref.abs().amax(dim=(1, 2), keepdim=True) + 1e-6)).max().item()
        assert err < 2e-5, err
        n1, st1 = ops.groupnorm_hilo(out.hi, out.lo, rows, HW, G, 1e-5, ga, be, True, want_stats=True, partial=part)
        assert float((n1.double() - nref).norm() / nref.norm()) < 4e-4
        assert (st1 - st0).abs().max().item() < 2e-4 * (1 + st0.abs().max().item())


def _as_pair(ops, v32):
    pr = ops.Pair.empty(v32.shape[0], v32.shape[1], v32.device)
    pr.hi.copy_(v32.half())
    pr.lo.copy_((v32 - pr.hi.float()).half())
    return pr


def test_fused_blocks_on_pairs(ops):
    """Accuracy mode: skg_ff_block_f16_hilo / skg_xattn_block_f16_hilo take the residual stream as a (hi, lo) pair and return a
    pair.  Against the unfused pair launches they replace (same rounding points: LayerNorm output, FF1 output, gated value / q,
    probabilities, attention output): hi + lo within 1e-4 relative; the stashed FF1 output and the LayerNorm statistics equal
    the unfused ones; in place == out of place."""
    from sketch2img_amd.unet import pack_ff_block, pack_xattn_kv, pack_xattn_weights
    d = dev()
    C, Fh, M = 320, 1280, 128 * 9 + 48
    g = torch.Generator().manual_seed(51)
    xp = _as_pair(ops, (torch.randn(M, C, generator=g) * 1.5 + 0.3).to(d))
    gam, bet = (1 + 0.2 * rnd(C, seed=52).float()).half().to(d), (0.1 * rnd(C, seed=53).float()).half().to(d)
    w1, b1 = rnd(2 * Fh, C, seed=54, scale=C ** -0.5), rnd(2 * Fh, seed=55, scale=0.1)
    w2, b2 = rnd(C, Fh, seed=56, scale=Fh ** -0.5), rnd(C, seed=57, scale=0.1)
    pack, bias1 = pack_ff_block(w1, b1, w2, d)
    M0 = 128 * 4 + 16
    y, st, pre = ops.ff_block(xp, gam, bet, 1e-5, pack, bias1, b2.to(d), want_stats=True, keep_from=M0)
    idx = ops.geglu_interleave_index(Fh)
    a3, st3 = ops.layernorm_hilo(xp.hi, xp.lo, gam, bet, 1e-5, want_stats=True)
    gg, f = ops.gemm_geglu_keep(a3, w1[idx].contiguous().to(d), b1[idx].contiguous().to(d))
    y3 = ops.Pair.empty(M, C, d)
    ops.gemm(gg, w2.to(d), out=y3.hi, out_lo=y3.lo, bias=b2.to(d), residual=xp.hi, residual_lo=xp.lo)
    s, s3 = y.hi.double() + y.lo.double(), y3.hi.double() + y3.lo.double()
    r = float((s - s3).norm() / s3.norm())
    print(f"[parity] ff_block on a pair vs the unfused pair launches: rel {r:.2e}")
    assert r < 1e-4 and torch.allclose(st, st3, rtol=1e-5, atol=1e-6)
    assert float((pre.float() - f[M0:].float()).norm() / f[M0:].float().norm()) < 1e-4
    assert float(y.lo.abs().max()) > 0 and float((y.hi.float() - s.float()).abs().max()) <= 2.0 ** -10 * float(s.abs().max())
    xin = ops.Pair.empty(M, C, d)
    xin.full.copy_(xp.full)
    ops.ff_block(xin, gam, bet, 1e-5, pack, bias1, b2.to(d), out=xin)
    y0 = ops.ff_block(xp, gam, bet, 1e-5, pack, bias1, b2.to(d))
    assert torch.equal(xin.full, y0.full) and torch.equal(y0.full, y.full)
    # cross-attention block
    for heads in (8, 5):
        _xattn_pair_checks(ops, heads, g, gam, bet)


def _xattn_pair_checks(ops, heads, g, gam, bet):
    from sketch2img_amd.unet import pack_xattn_kv, pack_xattn_weights
    d = dev()
    C = 320
    rows, HW, L, dh, Lp = 3, 512, 77, C // heads, 80
    M = rows * HW
    xp = _as_pair(ops, (torch.randn(M, C, generator=g) * 1.5 - 0.2).to(d))
    wq, wo, bo = rnd(C, C, seed=64, scale=C ** -0.5), rnd(C, C, seed=65, scale=C ** -0.5), rnd(C, seed=66, scale=0.1)
    K, V = rnd(rows * Lp, C, seed=67).to(d), rnd(rows * Lp, C, seed=68).to(d)
    wp, kvp = pack_xattn_weights(wq, wo, heads, d), pack_xattn_kv(K, V, rows, Lp, L, heads)
    y = ops.xattn_block(xp, HW, heads, L, gam, bet, 1e-5, wp, kvp, bo.to(d), dh ** -0.5)
    a2 = ops.layernorm_hilo(xp.hi, xp.lo, gam, bet, 1e-5)
    o2 = ops.attn_fwd(ops.gemm(a2, wq.to(d)), K, V, rows, heads, HW, L, Lp, dh, dh ** -0.5, v_rows=True)
    y4 = ops.Pair.empty(M, C, d)
    ops.gemm(o2, wo.to(d), out=y4.hi, out_lo=y4.lo, bias=bo.to(d), residual=xp.hi, residual_lo=xp.lo)
    s, s4 = y.hi.double() + y.lo.double(), y4.hi.double() + y4.lo.double()
    r = float((s - s4).norm() / s4.norm())
    print(f"[parity] xattn_block ({heads} heads) on a pair vs the unfused pair launches: rel {r:.2e}")
    assert r < 1e-4 and float((y.hi.float() - s.float()).abs().max()) <= 2.0 ** -10 * float(s.abs().max())
    # ... and its stashing form (skg_xattn_block_f16_hilo_keep, guided steps of the accuracy mode): the same pair (to 1 ulp of lo on
    # a few outputs: another instantiation of the same source), and for the rows from keep_from on norm2's statistics, q, the
    # attention output and lse of the unfused pair launches
    kf = 2 * HW
    yk, stk, qk, ok, lsek = ops.xattn_block(xp, HW, heads, L, gam, bet, 1e-5, wp, kvp, bo.to(d), dh ** -0.5, keep_from=kf)
    sk = yk.hi.double() + yk.lo.double()
    rk = float((sk - s).norm() / s.norm())
    a2k, st_ref = ops.layernorm_hilo(xp.hi[kf:], xp.lo[kf:], gam, bet, 1e-5, want_stats=True)
    q_ref = ops.gemm(a2k, wq.to(d))
    o_ref, lse_ref = ops.attn_fwd(q_ref, K[2 * Lp:], V[2 * Lp:], 1, heads, HW, L, Lp, dh, dh ** -0.5, want_lse=True, v_rows=True)
    e_st = float((stk - st_ref.reshape(-1, 2)).abs().max() / st_ref.abs().max())
    e_q, e_o = rel_err(qk, q_ref), rel_err(ok, o_ref)
    e_l = float((lsek.reshape(-1) - lse_ref.reshape(-1)).abs().max())
    print(f"[parity] xattn_block_hilo_keep vs plain pair launch rel {rk:.2e}; stats {e_st:.1e}  q rel {e_q:.1e}  o rel {e_o:.1e}  lse max abs {e_l:.1e}")
    assert rk < 1e-6 and float((yk.hi != y.hi).float().mean()) < 1e-3
    assert e_st < 1e-5 and e_q < 3e-4 and e_o < 6e-4 and e_l < 2e-3
    yk2 = ops.xattn_block(xp, HW, heads, L, gam, bet, 1e-5, wp, kvp, bo.to(d), dh ** -0.5, keep_from=kf)
    assert torch.equal(yk2[0].full, yk.full) and torch.equal(yk2[2], qk)


@pytest.mark.parametrize("rows,ih,cin,cout", [(2, 16, 128, 320), (4, 32, 640, 640), (2, 8, 1280, 1280)])
def test_conv_up2_polyphase_on_pairs(ops, rows, ih, cin, cout):
    """Accuracy mode: nearest-2x upsample + 3x3 conv, polyphase, on a pair input with (hi, lo) pre-summed weights and a pair
    output (skg_conv3x3_up2_f16_hilo; per tap [x_hi | x_lo | x_hi] . [W_hi | W_hi | W_lo]): hi + lo against fp64
    F.interpolate + F.conv2d of the pair's sum carries fp32 accuracy - the pre-summed weights' fp16 rounding (1.4e-4 at kernel
    level, what cost the plain-weight form its eps margin in round 3) is gone; incl. the one-grid form of the small maps."""
    from sketch2img_amd.unet import pack_conv_up2_hilo
    d = dev()
    g = torch.Generator().manual_seed(61)
    x32 = torch.randn(rows * ih * ih, cin, generator=g).to(d)
    xp = _as_pair(ops, x32)
    w = (torch.randn(cout, cin, 3, 3, generator=g) * (9 * cin) ** -0.5).half()
    b = rnd(cout, seed=62).to(d)
    out = ops.Pair.empty(rows * 4 * ih * ih, cout, d)
    ops.conv_up2_hilo(xp.full, pack_conv_up2_hilo(w, d), rows, ih, ih, out, bias=b)
    xs = (xp.hi.double() + xp.lo.double()).reshape(rows, ih, ih, cin).permute(0, 3, 1, 2)
    ref = F.conv2d(F.interpolate(xs, scale_factor=2, mode="nearest"), w.double().to(d), padding=1).permute(0, 2, 3, 1).reshape(-1, cout) + b.double()
    e = float(((out.hi.double() + out.lo.double()) - ref).norm() / ref.norm())
    e_hi = float((out.hi.double() - ref).norm() / ref.norm())
    print(f"[parity] polyphase upsample on a pair rows{rows} {cin}->{cout} @{ih}: pair rel {e:.2e}, hi alone {e_hi:.2e}")
    assert e < 3e-6 and e_hi < 6e-4


def test_cfg_steps_on_a_pair_eps(ops):
    """Accuracy mode: eps arrives as a (hi, lo) pair in one buffer; the CFG + scheduler kernels add the halves in fp32."""
    from sketch2img_amd.sampler import DDIMTables, DPMTables
    d = dev()
    S, hw = 2, 256
    g = torch.Generator().manual_seed(71)
    e32 = torch.randn(2 * S * hw, 8, generator=g).to(d)
    x = torch.randn(S, 4, 16, 16, generator=g).to(d)
    ep = _as_pair(ops, e32)
    eu, ec, off = ops.eps_halves(ep, S, hw)
    assert off == 8
    tab = DDIMTables.make(10)
    t = int(tab.timesteps[3])
    xp, e = ops.cfg_ddim_step(eu, ec, x, S, hw, 7.5, tab.coeffs(t), want_eps=True, lo_off=off)
    es = (ep.hi.float() + ep.lo.float())[:, :4].reshape(2, S, hw, 4).permute(0, 1, 3, 2).reshape(2, S, 4, 16, 16)
    eref = es[0] + 7.5 * (es[1] - es[0])
    c0, c1, c2, c3 = tab.coeffs(t)
    assert torch.allclose(e, eref, rtol=1e-6, atol=1e-6) and torch.allclose(xp, c2 * (x - c1 * eref) / c0 + c3 * eref, rtol=1e-5, atol=1e-5)
    dt = DPMTables.make(10)
    x0 = torch.zeros_like(x)
    xp2, e2 = ops.cfg_dpmpp2m_step(eu, ec, x, x0, S, hw, 7.5, dt.coeffs(0, 1), want_eps=True, lo_off=off)
    assert torch.allclose(e2, eref, rtol=1e-6, atol=1e-6)


def test_split_k_workspace_is_per_stream(ops):
    """the split-K slab used to be ONE process-global pointer.  Since ABI 2 libskg.so keeps one slab per (device,
    stream) and hands it to the kernel as an argument: split-K launches issued alternately on two streams - free to overlap on
    the device - each reproduce the single-stream result bit for bit, and the two streams' slabs are different buffers."""
    g = torch.Generator().manual_seed(41)
    M, N, K = 1024, 1280, 5120                    # 64 tiles -> split-K (fp32 slabs + reduce)
    a = [torch.randn(M, K, generator=g).half().to(dev()) for _ in range(2)]
    w = [(torch.randn(N, K, generator=g) * K ** -0.5).half().to(dev()) for _ in range(2)]
    ref = [ops.gemm(a[i], w[i]).clone() for i in range(2)]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [[], []]
    for rep in range(40):
        for i, st in enumerate(streams):
            with torch.cuda.stream(st):
                outs[i].append(ops.gemm(a[i], w[i]))
    torch.cuda.synchronize()
    for i in range(2):
        assert all(torch.equal(o, ref[i]) for o in outs[i]), f"stream {i}: a split-K result changed under concurrency"
    keys = [(s.device.index, s.cuda_stream) for s in streams]
    assert all(k in ops._workspace for k in keys)
    assert ops._workspace[keys[0]].data_ptr() != ops._workspace[keys[1]].data_ptr()


# ---------------------------------------------------------------------------------------------- conv
def nhwc(x):   # [B,C,H,W] -> [B*H*W, C]
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


def from_nhwc(y, B, H, W):
    return y.reshape(B, H, W, -1).permute(0, 3, 1, 2)


@pytest.mark.parametrize("B,Cin,Cout,H", [(2, 32, 64, 16), (3, 320, 320, 8), (1, 64, 40, 33), (2, 960, 640, 16)])
def test_conv3x3_s1(ops, B, Cin, Cout, H):
    from sketch2img_amd.unet import pack_conv
    x, w, b = rnd(B, Cin, H, H, seed=1), rnd(Cout, Cin, 3, 3, seed=2, scale=(9 * Cin) ** -0.5), rnd(Cout, seed=3)
    res = rnd(B * H * H, Cout, seed=4)
    y = ops.conv3x3(nhwc(x).to(dev()), pack_conv(w, dev()), B, H, H, bias=b.to(dev()), residual=res.to(dev()))
    ref = F.conv2d(x.float(), w.float(), b.float(), padding=1) + from_nhwc(res.float(), B, H, H)
    r, _ = report(f"conv s1 {Cin}->{Cout}@{H}", from_nhwc(y.float().cpu(), B, H, H), ref)
    assert r < FP16_RND


def test_conv3x3_stride2_up2_and_dgrads(ops):
    from sketch2img_amd.unet import pack_conv, pack_conv_dgrad
    B, Ci, Co, H = 2, 64, 96, 16
    x, w = rnd(B, Ci, H, H, seed=1), rnd(Co, Ci, 3, 3, seed=2, scale=(9 * Ci) ** -0.5)
    d = dev()
    # stride 2
    y = ops.conv3x3(nhwc(x).to(d), pack_conv(w, d), B, H, H, ops.CONV_S2)
    ref = F.conv2d(x.float(), w.float(), stride=2, padding=1)
    assert report("conv s2", from_nhwc(y.float().cpu(), B, H // 2, H // 2), ref)[0] < FP16_RND
    # stride 2 with padding (0,1,0,1): the VAE encoder's Downsample2D
    y = ops.conv3x3(nhwc(x).to(d), pack_conv(w, d), B, H, H, ops.CONV_S2A)
    ref = F.conv2d(F.pad(x.float(), (0, 1, 0, 1)), w.float(), stride=2)
    assert report("conv s2 asym", from_nhwc(y.float().cpu(), B, H // 2, H // 2), ref)[0] < FP16_RND
    # nearest-2x upsample fused into the gather
    y = ops.conv3x3(nhwc(x).to(d), pack_conv(w, d), B, H, H, ops.CONV_UP2)
    ref = F.conv2d(F.interpolate(x.float(), scale_factor=2.0, mode="nearest"), w.float(), padding=1)
    assert report("conv up2", from_nhwc(y.float().cpu(), B, 2 * H, 2 * H), ref)[0] < FP16_RND
    # dgrad of stride 1: conv with the flipped / swapped pack
    gy = rnd(B, Co, H, H, seed=7)
    xg = x.float().requires_grad_(True)
    F.conv2d(xg, w.float(), padding=1).backward(gy.float())
    gx = ops.conv3x3(nhwc(gy).to(d), pack_conv_dgrad(w, d), B, H, H, ops.CONV_S1)
    assert report("conv s1 dgrad", from_nhwc(gx.float().cpu(), B, H, H), xg.grad)[0] < FP16_RND
    # dgrad of stride 2 (transposed conv gather)
    gy2 = rnd(B, Co, H // 2, H // 2, seed=8)
    xg = x.float().requires_grad_(True)
    F.conv2d(xg, w.float(), stride=2, padding=1).backward(gy2.float())
    gx = ops.conv3x3(nhwc(gy2).to(d), pack_conv_dgrad(w, d), B, H // 2, H // 2, ops.CONV_S2T)
    assert report("conv s2 dgrad", from_nhwc(gx.float().cpu(), B, H, H), xg.grad)[0] < FP16_RND
    # dgrad of upsample+conv: stride-1 dgrad at 2H then 2x2 sum-pool
    gy3 = rnd(B, Co, 2 * H, 2 * H, seed=9)
    xg = x.float().requires_grad_(True)
    F.conv2d(F.interpolate(xg, scale_factor=2.0, mode="nearest"), w.float(), padding=1).backward(gy3.float())
    gu = ops.conv3x3(nhwc(gy3).to(d), pack_conv_dgrad(w, d), B, 2 * H, 2 * H, ops.CONV_S1)
    gx = ops.sumpool2x2(gu, B, H, H)
    # two fp16 roundings (dgrad output, pooled sum)
    assert report("conv up2 dgrad", from_nhwc(gx.float().cpu(), B, H, H), xg.grad)[0] < 2 * FP16_RND


def test_conv_in_out_padding_paths(ops):
    """conv_in (4 -> C, latent padded to 32 ch) and conv_out (C -> 4, padded to 8) as the UNet uses them."""
    from sketch2img_amd.unet import CIN_PAD, COUT_PAD, pack_conv, pack_conv_dgrad
    B, C, H = 2, 64, 16
    x, w_in, w_out = rnd(B, 4, H, H, seed=1), rnd(C, 4, 3, 3, seed=2, scale=1 / 6), rnd(4, C, 3, 3, seed=3, scale=0.04)
    d = dev()
    x32 = ops.nchw_to_nhwc(x.float().to(d), CIN_PAD)
    h = ops.conv3x3(x32, pack_conv(w_in, d, cin_pad=CIN_PAD), B, H, H)
    ref = F.conv2d(x.float(), w_in.float(), padding=1)
    assert report("conv_in", from_nhwc(h.float().cpu(), B, H, H), ref)[0] < FP16_RND
    e = ops.conv3x3(h, pack_conv(w_out, d, cout_pad=COUT_PAD), B, H, H)
    ref2 = F.conv2d(from_nhwc(h.float().cpu(), B, H, H), w_out.float(), padding=1)
    got = ops.nhwc_to_nchw(e, B, 4, H, H).cpu()
    assert report("conv_out", got, ref2)[0] < FP16_RND
    assert e[:, 4:].abs().max() == 0
    gy = rnd(B, C, H, H, seed=5)
    xg = x.float().requires_grad_(True)
    F.conv2d(xg, w_in.float(), padding=1).backward(gy.float())
    gx = ops.conv3x3(nhwc(gy).to(d), pack_conv_dgrad(w_in, d, cin_pad=COUT_PAD), B, H, H)
    assert report("conv_in dgrad", ops.nhwc_to_nchw(gx, B, 4, H, H).cpu(), xg.grad)[0] < FP16_RND


# ---------------------------------------------------------------------------------------------- norms
@pytest.mark.parametrize("B,C,H,G,silu", [(2, 320, 8, 32, True), (3, 960, 16, 32, True), (2, 64, 64, 8, False),
                                          (1, 2560, 8, 32, True), (2, 1280, 16, 32, True), (2, 2560, 16, 32, False),
                                          (3, 1280, 8, 32, True), (2, 1920, 16, 32, True)])
def test_groupnorm_fwd_bwd(ops, B, C, H, G, silu):
    x = rnd(B, C, H, H, seed=1) + 0.3
    ga, be = (1 + 0.2 * rnd(C, seed=2).float()).half(), (0.2 * rnd(C, seed=3).float()).half()
    d = dev()
    xh = nhwc(x).to(d)
    y, st = ops.groupnorm(xh, B, H * H, G, 1e-5, ga.to(d), be.to(d), silu)
    xr = x.float().requires_grad_(True)
    ref = F.group_norm(xr, G, ga.float(), be.float(), 1e-5)
    if silu:
        ref = F.silu(ref)
    assert report(f"gn fwd C{C}", from_nhwc(y.float().cpu(), B, H, H), ref)[0] < FP16_RND
    dy, res = rnd(B, C, H, H, seed=4), rnd(B, C, H, H, seed=5)
    ref.backward(dy.float())
    dx = ops.groupnorm_bwd(xh, nhwc(dy).to(d), B, H * H, G, st, ga.to(d), be.to(d), silu, residual=nhwc(res).to(d))
    assert report(f"gn bwd C{C}", from_nhwc(dx.float().cpu(), B, H, H), xr.grad + res.float())[0] < 2 * FP16_RND


# (kind, rows, H, Cin, Cout, residual): which kernel's epilogue writes the partial sums is the launcher's choice - the
# cases walk through the v8 256 x 320 tile (64 x 64 level, K >= 1024), the v2 128 x 160 tile with two and with three
# stages, with and without residual (fp16 / fp32 staging slabs), group widths 10 / 20 / 40, and the fall-back pass
# (128 x 64 tile / split-K at the 16 x 16 level)
@pytest.mark.parametrize("kind,rows,H,Cin,Cout,res", [
    ("conv", 16, 64, 320, 320, False), ("conv", 16, 64, 320, 320, True), ("conv", 8, 64, 320, 320, False),
    ("conv", 4, 64, 320, 320, True), ("conv", 16, 32, 640, 640, False), ("conv", 16, 32, 640, 640, True),
    ("conv", 2, 32, 320, 640, True), ("conv", 16, 16, 1280, 1280, True), ("conv", 16, 32, 320, 1280, False),
    ("gemm", 16, 64, 320, 320, True), ("gemm", 16, 32, 640, 640, True), ("gemm", 8, 64, 320, 320, False),
    ("gemm", 2, 32, 640, 640, True), ("up2", 4, 16, 640, 640, False), ("down", 8, 64, 320, 320, False)])
def test_groupnorm_statistics_from_the_producer_epilogue(ops, kind, rows, H, Cin, Cout, res):
    d = dev()
    G = 32
    mode = {"conv": ops.CONV_S1, "up2": ops.CONV_UP2, "down": ops.CONV_S2}.get(kind)
    OH = H * 2 if kind == "up2" else H // 2 if kind == "down" else H
    M, HW = rows * OH * OH, OH * OH
    x = (rnd(rows * H * H, Cin, seed=1).float() * 0.5).half().to(d)
    r = rnd(M, Cout, seed=4).to(d) if res else None
    b = rnd(Cout, seed=3).to(d)
    if kind == "gemm":
        w = (rnd(Cout, Cin, seed=2).float() * Cin ** -0.5).half().to(d)
        y0 = ops.gemm(x, w, bias=b, residual=r)
        y, part = ops.gemm(x, w, bias=b, residual=r, gn_stats=(HW, G))
    else:
        w = (rnd(Cout, 9 * Cin, seed=2).float() * (9 * Cin) ** -0.5).half().to(d)
        y0 = ops.conv3x3(x, w, rows, H, H, mode, bias=b, residual=r)
        y, part = ops.conv3x3(x, w, rows, H, H, mode, bias=b, residual=r, gn_groups=G)
    assert torch.equal(y, y0)                                   # the output itself does not change
    cpg = Cout // G
    yf = y.float().view(rows, HW // 128, 128, G, cpg)
    ref = torch.stack([yf.sum(dim=(2, 4)), (yf * yf).sum(dim=(2, 4))], dim=-1)       # [rows, nch, G, 2]
    got = part.buf.view(rows, HW // 128, G, 2)
    scale = ref.abs().amax(dim=(1, 2), keepdim=True) + 1e-6
    err = ((got - ref).abs() / scale).max().item()
    print(f"gn partial {kind} rows{rows} H{H} {Cin}->{Cout} res={res}: max err / max |sum| {err:.2e}")
    assert err < 2e-5
    ga, be = (1 + 0.2 * rnd(Cout, seed=5).float()).half().to(d), (0.2 * rnd(Cout, seed=6).float()).half().to(d)
    n1, st1 = ops.groupnorm(y, rows, HW, G, 1e-5, ga, be, True, partial=part)
    n0, st0 = ops.groupnorm(y, rows, HW, G, 1e-5, ga, be, True)
    assert (st1 - st0).abs().max().item() < 1e-4 * (1 + st0.abs().max().item())
    assert (n1.float() - n0.float()).abs().max().item() <= 2e-3 * (1 + n0.float().abs().max().item())
    # fixed summation order: a second launch reproduces the partial sums bit for bit
    if kind == "gemm":
        _, part2 = ops.gemm(x, w, bias=b, residual=r, gn_stats=(HW, G))
    else:
        _, part2 = ops.conv3x3(x, w, rows, H, H, mode, bias=b, residual=r, gn_groups=G)
    assert torch.equal(part.buf, part2.buf)


@pytest.mark.parametrize("rows,H,CA,CB", [(4, 64, 320, 320), (4, 32, 640, 640), (2, 32, 320, 320)])
def test_groupnorm_of_a_concatenation_from_two_producers(ops, rows, H, CA, CB):
    """The up path's norm1 reads torch.cat([h, skip]): h and skip are written into one buffer by two producers that each
    leave 32-group partial sums of their own channels; the GroupNorm over the concatenation (32 groups of twice the
    width) regroups them - same result as the stand-alone statistics pass."""
    d = dev()
    G, HW, M = 32, H * H, rows * H * H
    cat = torch.empty(M, CA + CB, device=d, dtype=torch.float16)
    xa, xb = rnd(M, 320, seed=1).to(d), rnd(M, 320, seed=2).to(d)
    wa = (rnd(CA, 320, seed=3).float() * 320 ** -0.5).half().to(d)
    wb = (rnd(CB, 320, seed=4).float() * 320 ** -0.5).half().to(d)
    _, pa = ops.gemm(xa, wa, cat[:, :CA], bias=rnd(CA, seed=5).to(d), gn_stats=(HW, G))
    _, pb = ops.gemm(xb, wb, cat[:, CA:], bias=rnd(CB, seed=6).to(d), residual=rnd(M, CB, seed=7).to(d), gn_stats=(HW, G))
    assert ops.gn_concat_ok(CA, CB, G, pa.groups, pb.groups)
    ga, be = (1 + 0.2 * rnd(CA + CB, seed=8).float()).half().to(d), (0.2 * rnd(CA + CB, seed=9).float()).half().to(d)
    n1, st1 = ops.groupnorm(cat, rows, HW, G, 1e-5, ga, be, True, partial=(pa, CA, pb))
    n0, st0 = ops.groupnorm(cat, rows, HW, G, 1e-5, ga, be, True)
    assert (st1 - st0).abs().max().item() < 1e-4 * (1 + st0.abs().max().item())
    assert (n1.float() - n0.float()).abs().max().item() <= 2e-3 * (1 + n0.float().abs().max().item())
    assert not ops.gn_concat_ok(640, 320, G, 32, 32)              # 960 channels: 30-wide groups straddle the halves
    from sketch2img_amd._lib import SkgError
    with pytest.raises(SkgError):
        bad = torch.empty(M, 960, device=d, dtype=torch.float16)
        ops.groupnorm(bad, rows, HW, G, 1e-5, ga[:960].contiguous(), be[:960].contiguous(), True, partial=(pa, 640, pb))


def test_groupnorm_pair_arms_apply_alone_and_two_producers(ops):
    """The two pair arms of the GroupNorm entry points that no other test calls through ops: skg_groupnorm_apply with X_lo (the
    apply alone on a pair, statistics from groupnorm_stats on the hi part) and skg_groupnorm_from_partial with X_lo and a second
    partial (the concatenation [A | B] on a pair; the partial sums are those of the hi part of each half in the layout the
    producers leave: [sample][128-row chunk][group][sum, sum of squares], two source groups per output group as in the UNet's up
    path).  Smallest shape the kernels take: one image, HW = 128 (one chunk), C = 32, 8 groups.  Against torch's fp32 GroupNorm
    of hi + lo with the bounds of the sibling arms' tests (test_hilo_*: 4e-4 relative, statistics 2e-4)."""
    d = dev()
    rows, HW, C, G, CA, GA = 1, 128, 32, 8, 16, 8
    pr = _as_pair(ops, (3 * torch.randn(rows * HW, C, generator=torch.Generator().manual_seed(11)) + 1.5).to(d))
    vs = pr.hi.float() + pr.lo.float()
    ga, be = (1 + 0.1 * rnd(C, seed=12).float()).half().to(d), (0.1 * rnd(C, seed=13).float()).half().to(d)
    ref = F.silu(F.group_norm(vs.reshape(rows, HW, C).permute(0, 2, 1), G, ga.float(), be.float(), 1e-5)).permute(0, 2, 1).reshape(-1, C)
    st = ops.groupnorm_stats(pr.hi, rows, HW, G, 1e-5)
    y = ops.groupnorm_apply(pr.hi, rows, HW, G, st, ga, be, True, X_lo=pr.lo)
    y16 = ops.groupnorm_apply(pr.hi, rows, HW, G, st, ga, be, True)
    e, e16 = rel_err(y, ref), rel_err(y16, ref)
    print(f"groupnorm_apply on a pair: rel {e:.2e} (hi alone: {e16:.2e})")
    assert e < 4e-4 and e <= e16 * 1.05

    def sums(x, g):
        xf = x.float().reshape(rows, HW // 128, 128, g, x.shape[1] // g)
        return torch.stack([xf.sum(dim=(2, 4)), (xf * xf).sum(dim=(2, 4))], dim=-1).reshape(-1)
    pa, pb = ops.GNPartial(rows, HW, GA, d), ops.GNPartial(rows, HW, GA, d)
    pa.buf.copy_(sums(pr.hi[:, :CA], GA))
    pb.buf.copy_(sums(pr.hi[:, CA:], GA))
    assert ops.gn_concat_ok(CA, C - CA, G, GA, GA)
    n1, st1 = ops.groupnorm_hilo(pr.hi, pr.lo, rows, HW, G, 1e-5, ga, be, True, want_stats=True, partial=(pa, CA, pb))
    n0, st0 = ops.groupnorm_hilo(pr.hi, pr.lo, rows, HW, G, 1e-5, ga, be, True, want_stats=True)
    e1 = rel_err(n1, ref)
    print(f"groupnorm of a pair from two producers' sums: rel {e1:.2e}, statistics max diff {(st1 - st0).abs().max().item():.2e}")
    assert e1 < 4e-4
    assert (st1 - st0).abs().max().item() < 2e-4 * (1 + st0.abs().max().item())


@pytest.mark.parametrize("M,C", [(77, 320), (1024, 1280), (5, 32), (4096, 640)])
def test_layernorm_fwd_bwd(ops, M, C):
    x = rnd(M, C, seed=1) * 2 + 0.5
    ga, be = (1 + 0.2 * rnd(C, seed=2).float()).half(), (0.2 * rnd(C, seed=3).float()).half()
    d = dev()
    y, st = ops.layernorm(x.to(d), ga.to(d), be.to(d), want_stats=True)
    xr = x.float().requires_grad_(True)
    ref = F.layer_norm(xr, (C,), ga.float(), be.float(), 1e-5)
    assert report(f"ln fwd {M}x{C}", y.float().cpu(), ref)[0] < FP16_RND
    dy, res = rnd(M, C, seed=4), rnd(M, C, seed=5)
    ref.backward(dy.float())
    dx = ops.layernorm_bwd(x.to(d), dy.to(d), ga.to(d), st, residual=res.to(d))
    assert report(f"ln bwd {M}x{C}", dx.float().cpu(), xr.grad + res.float())[0] < 2 * FP16_RND


def test_geglu_fwd_bwd(ops):
    M, Fd = 300, 1280
    h = rnd(M, 2 * Fd, seed=1)
    d = dev()
    y = ops.geglu(h.to(d))
    hr = h.float().requires_grad_(True)
    a, g = hr.chunk(2, dim=-1)
    ref = a * F.gelu(g)
    assert report("geglu fwd", y.float().cpu(), ref)[0] < FP16_RND
    dy = rnd(M, Fd, seed=2)
    ref.backward(dy.float())
    dh = ops.geglu_bwd(h.to(d), dy.to(d))
    assert report("geglu bwd", dh.float().cpu(), hr.grad)[0] < FP16_RND


def test_geglu_interleaved_and_fused_gemm(ops):
    """The interleaved FF1 pack: separate kernels and the GEMM-epilogue fusion give diffusers' GEGLU."""
    M, C = 700, 128
    Fd = 4 * C
    x, w, b = rnd(M, C, seed=1), rnd(2 * Fd, C, seed=2, scale=C ** -0.5), rnd(2 * Fd, seed=3)
    d = dev()
    idx = ops.geglu_interleave_index(Fd)
    wp, bp = w[idx].contiguous().to(d), b[idx].contiguous().to(d)
    hr = (x.float() @ w.float().t() + b.float()).requires_grad_(True)
    a, g = hr.chunk(2, dim=-1)
    ref = a * F.gelu(g)
    y_fused = ops.gemm(x.to(d), wp, bias=bp, geglu=True)
    assert y_fused.shape == (M, Fd)
    assert report("gemm+geglu fused", y_fused.float().cpu(), ref)[0] < FP16_RND
    f = ops.gemm(x.to(d), wp, bias=bp)                       # interleaved pre-activation
    assert report("ff1 interleaved", f.float().cpu()[:, torch.argsort(idx)], hr)[0] < FP16_RND
    y = ops.geglu(f, interleaved=True)
    # two roundings here (f stored in fp16) vs one in the fused path
    assert report("geglu interleaved fwd", y.float().cpu(), ref)[0] < 2 * FP16_RND
    dy = rnd(M, Fd, seed=4)
    f16 = f.float().cpu()[:, torch.argsort(idx)].requires_grad_(True)
    a2, g2 = f16.chunk(2, dim=-1)
    (a2 * F.gelu(g2)).backward(dy.float())
    dh = ops.geglu_bwd(f, dy.to(d), interleaved=True)
    assert report("geglu interleaved bwd", dh.float().cpu()[:, torch.argsort(idx)], f16.grad)[0] < FP16_RND
    # small M, long K: the shape class that would take the split-K path without the GEGLU flag
    xs, ws, bs = rnd(128, 1280, seed=5), rnd(2048, 1280, seed=6, scale=1280 ** -0.5), rnd(2048, seed=7)
    i2 = ops.geglu_interleave_index(1024)
    ys = ops.gemm(xs.to(d), ws[i2].contiguous().to(d), bias=bs[i2].contiguous().to(d), geglu=True)
    hs = xs.float() @ ws.float().t() + bs.float()
    assert report("gemm+geglu fused small-M", ys.float().cpu(), hs[:, :1024] * F.gelu(hs[:, 1024:]))[0] < FP16_RND
    from sketch2img_amd._lib import SkgError
    with pytest.raises(SkgError):                            # K % 64 != 0 -> generic kernel -> no fused GEGLU
        ops.gemm(rnd(64, 32).to(d), rnd(16, 32).to(d), geglu=True)
    # the fused gate that also keeps the pre-activation (cond rows of a guided step): both outputs are bit for bit what
    # the two separate launches of the fused epilogue / the plain GEMM give; 128 x 160 and 256 x 320 tile paths
    for Mk, Ck in ((700, 128), (4096, 1280), (8192, 320)):
        xk = rnd(Mk, Ck, seed=8).to(d)
        wk, bk = rnd(8 * Ck, Ck, seed=9, scale=Ck ** -0.5).to(d), rnd(8 * Ck, seed=10).to(d)
        yk, hk = ops.gemm_geglu_keep(xk, wk, bk)
        assert torch.equal(yk, ops.gemm(xk, wk, bias=bk, geglu=True)) and torch.equal(hk, ops.gemm(xk, wk, bias=bk))


def test_data_movement(ops):
    d = dev()
    x = rnd(200, 72, seed=1)
    assert torch.equal(ops.transpose(x.to(d)).cpu(), x.t().contiguous())
    big = rnd(4096 + 64, 320, seed=2)
    assert torch.equal(ops.transpose(big.to(d)).cpu(), big.t().contiguous())
    a, b = rnd(100, 64, seed=3), rnd(100, 96, seed=4)
    out = ops.axpby(a.to(d), b.to(d)[:, 16:80], alpha=1.0, beta=1.0)
    assert report("axpby", out.float().cpu(), a.float() + b[:, 16:80].float())[0] < FP16_RND
    cat = torch.zeros(100, 160, device=d, dtype=torch.float16)
    ops.axpby(a.to(d), out=cat[:, :64]); ops.axpby(b.to(d), out=cat[:, 64:])
    assert torch.equal(cat.cpu(), torch.cat([a, b], 1))
    x4 = rnd(2, 24, 8, 8, seed=5)
    p = ops.sumpool2x2(nhwc(x4).to(d), 2, 4, 4)
    ref = F.avg_pool2d(x4.float(), 2) * 4
    assert report("sumpool", from_nhwc(p.float().cpu(), 2, 4, 4), ref)[0] < FP16_RND
    s = ops.silu(a.to(d))
    assert report("silu", s.float().cpu(), F.silu(a.float()))[0] < FP16_RND
    lat = torch.randn(3, 4, 8, 8)
    n = ops.nchw_to_nhwc(lat.to(d), 32)
    assert n.shape == (3 * 64, 32) and n[:, 4:].abs().max() == 0
    assert torch.equal(ops.nhwc_to_nchw(n, 3, 4, 8, 8).cpu(), lat.half().float())


# ---------------------------------------------------------------------------------------------- attention
def ref_attention(q, k, v, heads, scale):
    B, N, C = q.shape
    dh = C // heads
    qh = q.view(B, N, heads, dh).transpose(1, 2)
    kh = k.view(B, -1, heads, dh).transpose(1, 2)
    vh = v.view(B, -1, heads, dh).transpose(1, 2)
    s = (qh @ kh.transpose(-1, -2)) * scale
    lse = torch.logsumexp(s, dim=-1)
    o = torch.softmax(s, dim=-1) @ vh
    return o.transpose(1, 2).reshape(B, N, C), lse


@pytest.mark.parametrize("dh,heads,Nq,Nkv", [(40, 8, 256, 256), (80, 8, 128, 128), (160, 8, 64, 64), (64, 5, 200, 200),
                                            (16, 2, 72, 72), (32, 2, 1024, 1024), (40, 8, 4096, 4096),
                                            (40, 8, 256, 77), (160, 8, 64, 77), (64, 5, 144, 401), (80, 8, 1000, 77),
                                            (64, 5, 300, 77), (40, 8, 200, 50), (40, 8, 4096, 77),
                                            (40, 8, 3000, 3000), (64, 10, 2560, 2817)])
def test_attention_forward(ops, dh, heads, Nq, Nkv):
    B, C = 2, heads * dh
    kvs = (Nkv + 7) // 8 * 8
    q, k, v = rnd(B, Nq, C, seed=1), rnd(B, Nkv, C, seed=2), rnd(B, Nkv, C, seed=3)
    scale = dh ** -0.5
    d = dev()
    kp = torch.zeros(B, kvs, C, dtype=torch.float16); kp[:, :Nkv] = k
    vp = torch.zeros(B, kvs, C, dtype=torch.float16); vp[:, :Nkv] = v
    Q, K, V = q.reshape(B * Nq, C).to(d), kp.reshape(B * kvs, C).to(d), vp.reshape(B * kvs, C).to(d)
    o, lse = ops.attn_fwd(Q, K, ops.transpose(V), B, heads, Nq, Nkv, kvs, dh, scale, want_lse=True)
    # B = 2 keeps every launch here under the 1024 workgroups QT 3 needs: the streaming kernel at two query tiles per wave (one at d = 160)
    assert ops.attn_fwd_variant(B, heads, Nq, Nkv, kvs, dh) == ((1001, 64) if dh == 160 else (1002, 128))
    ro, rl = ref_attention(q.float(), k.float(), v.float(), heads, scale)
    r, _ = report(f"attn fwd dh{dh} {Nq}x{Nkv}", o.float().cpu().view(B, Nq, C), ro)
    # P is rounded to fp16 before the PV product (like every fp16 flash kernel): ~1e-3 relative
    assert r < 2e-3
    assert report("attn lse", lse.cpu(), rl)[1] < 2e-3
    # V handed over row-major (skg_attn_fwd_rowv: fragments through ds_read_b64_tr_b16): the same products in the same
    # order, so the result is the transposed-copy path's bit for bit
    o2, lse2 = ops.attn_fwd(Q, K, V, B, heads, Nq, Nkv, kvs, dh, scale, want_lse=True, v_rows=True)
    if kvs <= 80 and dh in (40, 64, 80, 160):
        # short key sequences (the 77 text tokens) with row-major V take the LDS-resident kernel (attn_fwd_short_kernel):
        # another kernel, so not bit-equal to the flash kernel - checked against the reference like it, and deterministic
        assert ops.attn_fwd_variant(B, heads, Nq, Nkv, kvs, dh, v_rows=True)[0] == 3005
        assert report(f"attn fwd short-key kernel dh{dh} {Nq}x{Nkv}", o2.float().cpu().view(B, Nq, C), ro)[0] < 2e-3
        assert report("attn lse short-key kernel", lse2.cpu(), rl)[1] < 2e-3
        o3, lse3 = ops.attn_fwd(Q, K, V, B, heads, Nq, Nkv, kvs, dh, scale, want_lse=True, v_rows=True)
        assert torch.equal(o2, o3) and torch.equal(lse2, lse3)
    else:
        # every other shape: the same 4-wave flash kernel as the transposed-copy path (QT 2 also at d = 40, 4096 tokens: 352 workgroups
        # of 192 queries; QT 3 takes 1024 - tests/test_gpu_attention_fwd.py runs it), fed through ds_read_b64_tr_b16.  (The 8-wave
        # formulation of round 4 was measured and withdrawn: EXPERIMENTS.md.)
        assert ops.attn_fwd_variant(B, heads, Nq, Nkv, kvs, dh, v_rows=True) == ops.attn_fwd_variant(B, heads, Nq, Nkv, kvs, dh)
        assert torch.equal(o2, o) and torch.equal(lse2, lse)


@pytest.mark.parametrize("dh,heads,N,Nkv", [(64, 12, 80, 77), (16, 4, 80, 77), (32, 3, 320, 320), (64, 2, 200, 197)])
def test_attention_forward_causal(ops, dh, heads, N, Nkv):
    """skg_attn_fwd_causal (the CLIP text encoder's masked self-attention): key j visible to query i iff j <= i;
    several key tiles, ragged last tile, pad query rows past Nkv ignored."""
    B, C = 2, heads * dh
    q, k, v = rnd(B, N, C, seed=1), rnd(B, N, C, seed=2), rnd(B, N, C, seed=3)
    scale = dh ** -0.5
    d = dev()
    Q, K, V = (t.reshape(B * N, C).to(d) for t in (q, k, v))
    o, lse = ops.attn_fwd(Q, K, ops.transpose(V), B, heads, N, Nkv, N, dh, scale, want_lse=True, causal=True)
    qh, kh, vh = (t.float().view(B, N, heads, dh).transpose(1, 2)[:, :, :Nkv] for t in (q, k, v))
    sc = qh @ kh.transpose(-1, -2) * scale + torch.full((Nkv, Nkv), float("-inf")).triu(1)
    ro = (torch.softmax(sc, -1) @ vh).transpose(1, 2).reshape(B, Nkv, C)
    assert report(f"attn causal dh{dh} {N}", o.float().cpu().view(B, N, C)[:, :Nkv], ro)[0] < 2e-3
    assert report("attn causal lse", lse.cpu()[:, :, :Nkv], torch.logsumexp(sc, -1))[1] < 2e-3
    assert torch.isfinite(o.float()).all()
    with pytest.raises(RuntimeError):
        ops.attn_fwd(Q[:, :40], K[:, :40], ops.transpose(V[:, :40].contiguous()), B, 1, N, Nkv, N, 40, scale, causal=True)


def test_attention_forward_strided_qkv_and_online_rescale(ops):
    """Q/K read as column slices of a fused [M, 3C] buffer; spiked keys force the running max to jump at a
    late tile (the online-softmax rescale branch)."""
    B, heads, dh, N = 2, 8, 40, 320
    C = heads * dh
    qkv = rnd(B * N, 3 * C, seed=1)
    qkv[B * N // 2 + 200, C:2 * C] *= 12.0          # one key with a huge norm, in the 4th kv tile
    qkv[200, C:2 * C] *= -9.0
    d = dev()
    t = qkv.to(d)
    o = ops.attn_fwd(t[:, :C], t[:, C:2 * C], ops.transpose(t[:, 2 * C:]), B, heads, N, N, N, dh, dh ** -0.5)
    q, k, v = (qkv[:, i * C:(i + 1) * C].float().view(B, N, C) for i in range(3))
    ro, _ = ref_attention(q, k, v, heads, dh ** -0.5)
    assert report("attn fwd strided+spike", o.float().cpu().view(B, N, C), ro)[0] < 2e-3
    o2 = ops.attn_fwd(t[:, :C], t[:, C:2 * C], t[:, 2 * C:], B, heads, N, N, N, dh, dh ** -0.5, v_rows=True)
    assert torch.equal(o2, o)                        # V as the third column block of the fused buffer, no transpose


def test_attention_forward_large_map_online_rescale_and_structure(ops):
    """The d = 40 self-attention kernel on a large map, row-major V.  B = 2 makes 256 workgroups of 192 queries, under the 1024 at which
    the launcher takes three query tiles per wave, so this runs attn_fwd_kernel<2, 3, 2> (QT 2: asserted below); the QT 3 instantiation of
    the 64 x 64 level is under tests/test_gpu_attention_fwd.py.  (a) spiked keys in late tiles force the reference maximum to move (the rescale branch); (b) structured probes with
    exact answers: K = 0 makes the softmax uniform, V = one-hot on single keys / single head columns, so every output
    is an exactly known value - a lost k-step, a wrong key <-> k-slot map or a wrong V row permutation shows as an O(1) error."""
    B, heads, dh, N = 2, 8, 40, 3072
    C = heads * dh
    d = dev()
    assert ops.attn_fwd_variant(B, heads, N, N, N, dh, v_rows=True) == (1002, 128)
    qkv = rnd(B * N, 3 * C, seed=1)
    qkv[B * N // 2 + 2900, C:2 * C] *= 12.0          # one key with a huge norm in the 46th kv tile of row 1
    qkv[1700, C:2 * C] *= -9.0
    t = qkv.to(d)
    o = ops.attn_fwd(t[:, :C], t[:, C:2 * C], t[:, 2 * C:], B, heads, N, N, N, dh, dh ** -0.5, v_rows=True)
    q, k, v = (qkv[:, i * C:(i + 1) * C].float().view(B, N, C) for i in range(3))
    ro, _ = ref_attention(q, k, v, heads, dh ** -0.5)
    assert report("attn fwd large map strided + spike", o.float().cpu().view(B, N, C), ro)[0] < 2e-3
    # (b) K = 0: uniform softmax, O[q][c] = mean over keys of V[:, c]
    Q = rnd(B * N, C, seed=2).to(d)
    K0 = torch.zeros(B * N, C, device=d, dtype=torch.float16)
    for key in (0, 5, 17, 31, 36, 63, 64 + 21, N - 1):          # one key carries 1.0 in every column, all others 0
        V = torch.zeros(B * N, C, device=d, dtype=torch.float16)
        V[key] = 1.0
        V[N + key] = 2.0
        o = ops.attn_fwd(Q, K0, V, B, heads, N, N, N, dh, dh ** -0.5, v_rows=True).float().view(B, N, C)
        assert float((o[0] - 1.0 / N).abs().max()) < 1e-6 and float((o[1] - 2.0 / N).abs().max()) < 2e-6, key
    V = torch.zeros(B * N, C, device=d, dtype=torch.float16)      # every key carries its (small-integer) code in one head column
    code = (torch.arange(N) % 61 + 1).half()
    for col in (0, 7, 16, 33, 39):
        V.zero_()
        V.view(B, N, heads, dh)[:, :, :, col] = code.to(d)[None, :, None]
        o = ops.attn_fwd(Q, K0, V, B, heads, N, N, N, dh, dh ** -0.5, v_rows=True).float().view(B, N, heads, dh)
        want = float(code.float().mean())
        assert float((o[..., col] - want).abs().max()) < 2e-2 * want / 31 and float(o[..., [c for c in range(dh) if c != col]].abs().max()) == 0.0, col


@pytest.mark.parametrize("dh,heads", [(40, 8), (64, 5), (160, 8)])
def test_attention_short_keys_structured_probes(ops, dh, heads):
    """ADVICE r3 / VERDICT r4: exact-answer probes for the 77-key cross-attention kernel (attn_fwd_short_kernel) - K = 0 makes the
    softmax uniform over the 77 valid keys (the three padding keys of the 80-row buffer must not count), V = one-hot on single
    keys / a key code in single head columns: a lost key, a padding key that leaks, a wrong key <-> k-slot map or a wrong V
    column shows as an O(1) error."""
    B, Nq, L, Lp = 2, 1024, 77, 80
    C = heads * dh
    d = dev()
    Q = rnd(B * Nq, C, seed=3).to(d)
    K0 = torch.zeros(B * Lp, C, device=d, dtype=torch.float16)
    K0.view(B, Lp, C)[:, L:] = 30.0          # padding rows hold garbage that would win the softmax if a padding key leaked
    for key in (0, 15, 16, 31, 47, 63, 64, 76):
        V = torch.zeros(B * Lp, C, device=d, dtype=torch.float16)
        V.view(B, Lp, C)[:, L:] = 7.0
        V[key] = 1.0
        V[Lp + key] = 2.0
        o = ops.attn_fwd(Q, K0, V, B, heads, Nq, L, Lp, dh, dh ** -0.5, v_rows=True).float().view(B, Nq, C)
        assert float((o[0] - 1.0 / L).abs().max()) < 2e-3 / L and float((o[1] - 2.0 / L).abs().max()) < 4e-3 / L, key
    code = (torch.arange(L) % 13 + 1).half()
    for col in sorted({0, 7, 16, 33, dh - 1}):
        V = torch.zeros(B * Lp, C, device=d, dtype=torch.float16)
        V.view(B, Lp, heads, dh)[:, :L, :, col] = code.to(d)[None, :, None]
        o = ops.attn_fwd(Q, K0, V, B, heads, Nq, L, Lp, dh, dh ** -0.5, v_rows=True).float().view(B, Nq, heads, dh)
        want = float(code.float().mean())
        assert float((o[..., col] - want).abs().max()) < 2e-3 * want, col
        assert float(o[..., [c for c in range(dh) if c != col]].abs().max()) == 0.0, col


@pytest.mark.parametrize("keep", [False, True])
def test_xattn_block_structured_probes(ops, keep):
    """The same probes through the fused cross-attention launch (skg_xattn_block_f16 / _keep): K = 0 -> uniform softmax over the
    77 keys whatever q is; V one-hot or coded; to_out = a cyclic column shift, so that a wrong head <-> column map, a lost
    K = 16 tail step (head columns 32..39) or a wrong Wo fragment shows as an O(1) error at a known place.  x = 0: the
    output IS the attention term."""
    from sketch2img_amd.unet import pack_xattn_kv, pack_xattn_weights
    d = dev()
    C, heads, dh, Lp, L, rows, HW = 320, 8, 40, 80, 77, 2, 1024
    M = rows * HW
    x = torch.zeros(M, C, dtype=torch.float16, device=d)
    gam, bet = torch.ones(C).half().to(d), (0.1 * rnd(C, seed=41).float()).half().to(d)
    wq = rnd(C, C, seed=42, scale=C ** -0.5)
    shift = 3
    wo = torch.zeros(C, C, dtype=torch.float16)
    wo[(torch.arange(C) + shift) % C, torch.arange(C)] = 1.0          # y[:, (c + shift) % C] = o[:, c]
    bo = torch.zeros(C, dtype=torch.float16).to(d)
    wp = pack_xattn_weights(wq, wo, heads, d)
    K0 = torch.zeros(rows * Lp, C, device=d, dtype=torch.float16)

    def run(V):
        kvp = pack_xattn_kv(K0, V, rows, Lp, L, heads)
        if keep:
            return ops.xattn_block(x, HW, heads, L, gam, bet, 1e-5, wp, kvp, bo, dh ** -0.5, keep_from=HW)[0].float().view(rows, HW, C)
        return ops.xattn_block(x, HW, heads, L, gam, bet, 1e-5, wp, kvp, bo, dh ** -0.5).float().view(rows, HW, C)

    for key in (0, 15, 16, 31, 47, 63, 64, 76):
        V = torch.zeros(rows * Lp, C, device=d, dtype=torch.float16)
        V[key] = 1.0
        V[Lp + key] = 2.0
        y = run(V)
        assert float((y[0] - 1.0 / L).abs().max()) < 3e-3 / L and float((y[1] - 2.0 / L).abs().max()) < 6e-3 / L, key
    code = (torch.arange(L) % 13 + 1).half()
    want = float(code.float().mean())
    for col in (0, 7, 16, 31, 32, 39):
        V = torch.zeros(rows * Lp, C, device=d, dtype=torch.float16)
        V.view(rows, Lp, heads, dh)[:, :L, :, col] = code.to(d)[None, :, None]
        y = run(V)
        hot = [(h * dh + col + shift) % C for h in range(heads)]
        cold = [c for c in range(C) if c not in hot]
        assert float((y[..., hot] - want).abs().max()) < 3e-3 * want, col
        assert float(y[..., cold].abs().max()) == 0.0, col


@pytest.mark.parametrize("dh,heads,Nq,Nkv,cross", [(40, 8, 256, 256, False), (80, 8, 64, 64, False),
                                                  (160, 8, 64, 64, False), (16, 2, 16, 16, False),
                                                  (64, 5, 200, 200, False), (32, 2, 1024, 1024, False),
                                                  (40, 8, 128, 77, True), (160, 8, 64, 77, True)])
def test_attention_backward(ops, dh, heads, Nq, Nkv, cross):
    B, C = 2, heads * dh
    kvs = (Nkv + 7) // 8 * 8
    scale = dh ** -0.5
    q, k, v = rnd(B, Nq, C, seed=1), rnd(B, Nkv, C, seed=2), rnd(B, Nkv, C, seed=3)
    do = rnd(B, Nq, C, seed=4)
    qf, kf, vf = (t.float().requires_grad_(True) for t in (q, k, v))
    ro, _ = ref_attention(qf, kf, vf, heads, scale)
    ro.backward(do.float())
    d = dev()
    kp = torch.zeros(B, kvs, C, dtype=torch.float16); kp[:, :Nkv] = k
    vp = torch.zeros(B, kvs, C, dtype=torch.float16); vp[:, :Nkv] = v
    Q, K, V = q.reshape(B * Nq, C).to(d), kp.reshape(B * kvs, C).to(d), vp.reshape(B * kvs, C).to(d)
    dO = do.reshape(B * Nq, C).to(d)
    o, lse = ops.attn_fwd(Q, K, ops.transpose(V), B, heads, Nq, Nkv, kvs, dh, scale, want_lse=True)
    delta = ops.attn_bwd_delta(o, dO, B, heads, Nq, dh)
    dq = ops.attn_bwd_dq(Q, K, V, dO, lse, delta, B, heads, Nq, Nkv, kvs, dh, scale)
    # tolerance: P and dS are rounded to fp16 before their MFMA products, delta uses the fp16 O
    assert report(f"attn dq dh{dh}", dq.float().cpu().view(B, Nq, C), qf.grad)[0] < 4e-3
    # the same with delta formed in the launch's prologue (skg_attn_bwd_dq_delta): delta to fp32 rounding, dq to its own rounding
    dq_f, delta_f = ops.attn_bwd_dq_delta(Q, K, V, dO, o, lse, B, heads, Nq, Nkv, kvs, dh, scale)
    assert float((delta_f - delta).abs().max()) <= 2e-5 * max(1.0, float(delta.abs().max()))
    assert report(f"attn dq with the delta prologue dh{dh}", dq_f.float().cpu().view(B, Nq, C), qf.grad)[0] < 4e-3
    assert rel_err(dq_f, dq) < 5e-4
    if not cross:
        dk, dv = ops.attn_bwd_dkv(Q, K, V, dO, lse, delta, B, heads, Nq, Nkv, dh, scale)
        assert report(f"attn dk dh{dh}", dk.float().cpu().view(B, Nkv, C), kf.grad)[0] < 4e-3
        assert report(f"attn dv dh{dh}", dv.float().cpu().view(B, Nkv, C), vf.grad)[0] < 4e-3


# ---------------------------------------------------------------------------------------------- LGP pieces
def test_lgp_layer0_gather_and_scatter(ops):
    """Re-associated layer 0: bilinear gather of fp32 partial products (+ extras, bias, fp16 round, ReLU)
    vs F.interpolate, and the scatter kernel as its exact adjoint."""
    S, h, H0 = 2, 16, 512
    sizes = [8, 2, 16, 4]
    g = torch.Generator().manual_seed(0)
    d = dev()
    P = [torch.randn(2 * S, H0, s, s, generator=g) for s in sizes]
    Wx, b0 = rnd(H0, 40, seed=1, scale=0.3), rnd(H0, seed=2)
    noise = torch.randn(S, 4, h, h, generator=g)
    sigma = 0.7
    Wfull = torch.zeros(H0, 48, dtype=torch.float16); Wfull[:, 8:] = Wx        # view with ldw > 40
    Z = ops.lgp_layer0_gather([p.permute(0, 2, 3, 1).reshape(-1, H0).contiguous().to(d) for p in P], sizes,
                              Wfull.to(d)[:, 8:], b0.to(d), noise.to(d), sigma, S, h, H0)
    nl = sigma * noise
    e = torch.cat([nl] + [torch.sin(2 * math.pi * nl * 2 ** -l) for l in range(9)], 1).half().float()   # [S,40,h,h]
    e = torch.cat([e, e])                                                            # rows [uncond; cond]
    ref = sum(F.interpolate(p, size=h, mode="bilinear") for p in P)
    ref = ref + torch.einsum("oc,bchw->bohw", Wx.float(), e) + b0.float()[None, :, None, None]
    ref = torch.relu(ref.half().float())
    got = Z.float().cpu().reshape(2 * S, h, h, H0).permute(0, 3, 1, 2)
    assert report("lgp gather", got, ref)[0] < FP16_RND
    # adjoint: <gather_bilinear(P), dZ> == <P, scatter(dZ)>
    dZ = rnd(S * h * h, H0, seed=5)
    for s in (8, 2, 16, 1):
        dP = ops.lgp_layer0_scatter(dZ.to(d), S, h, s, H0)
        pr = torch.randn(S, H0, s, s, generator=g).requires_grad_(True)
        up = F.interpolate(pr, size=h, mode="bilinear")
        up.backward(dZ.float().reshape(S, h, h, H0).permute(0, 3, 1, 2))
        assert report(f"lgp scatter s{s}", dP.float().cpu().reshape(S, s, s, H0).permute(0, 3, 1, 2), pr.grad)[0] < FP16_RND


@pytest.mark.parametrize("S,hw,C", [(3, 64, 256), (2, 1024, 512), (2, 200, 64), (1, 333, 128)])
@pytest.mark.parametrize("train", [True, False])
def test_batchnorm_per_sample_fwd_bwd(ops, train, S, hw, C):
    """BatchNorm1d with one sample's two CFG segments as the batch + backward through the preceding ReLU,
    checked on the SAME post-ReLU activations (so no gate can flip between the two sides).  Shapes: several row
    chunks per sample, the four-rows-in-flight loop and its ragged tail, 8 / 16 / 32 / 64 channel pieces."""
    d = dev()
    x = torch.relu(rnd(2 * S * hw, C, seed=1).float() + 0.2).half()                 # post-ReLU activations
    ga, be = (1 + 0.2 * rnd(C, seed=2).float()).half(), (0.2 * rnd(C, seed=3).float()).half()
    rm, rv = torch.zeros(C), torch.ones(C)
    dy = rnd(2 * S * hw, C, seed=4)
    if train:
        rmd, rvd = rm.clone().to(d), rv.clone().to(d)
        st = ops.bn_stats(x.to(d), S, 2, hw, 1e-5, rmd, rvd)
    else:
        rm, rv = 0.1 * torch.randn(C), 1 + 0.1 * torch.rand(C)
        st = ops.bn_stats_from_running(rm.to(d), rv.to(d), S)
    y = ops.bn_apply(x.to(d), S, 2, hw, st, ga.to(d), be.to(d))
    dx = ops.bn_relu_bwd(x.to(d), dy.to(d), S, 2, hw, st, ga.to(d), train)
    xs = x.float().reshape(2, S, hw, C)
    rm_ref, rv_ref = torch.zeros(C), torch.ones(C)
    for s in range(S):
        pre = xs[:, s].reshape(2 * hw, C).clone().requires_grad_(True)          # treat as pre-activation > 0 or == 0
        act = torch.relu(pre)
        if train:
            ref = F.batch_norm(act, None, None, ga.float(), be.float(), True, 0.1, 1e-5)
            mean, var = act.mean(0), act.var(0, unbiased=True)
            rm_ref = 0.9 * rm_ref + 0.1 * mean.detach(); rv_ref = 0.9 * rv_ref + 0.1 * var.detach()
        else:
            ref = F.batch_norm(act, rm, rv, ga.float(), be.float(), False, 0.1, 1e-5)
        dys = dy.float().reshape(2, S, hw, C)[:, s].reshape(2 * hw, C)
        ref.backward(dys)
        ys = y.float().cpu().reshape(2, S, hw, C)[:, s].reshape(2 * hw, C)
        dxs = dx.float().cpu().reshape(2, S, hw, C)[:, s].reshape(2 * hw, C)
        assert report(f"bn fwd s{s}", ys, ref)[0] < FP16_RND
        gref = pre.grad * (pre > 0)                                                 # relu'(0) = 0 on both sides
        assert report(f"bn+relu bwd s{s}", dxs, gref)[0] < FP16_RND
    if train:
        assert report("bn running_mean", rmd.cpu(), rm_ref)[1] < 1e-5
        assert report("bn running_var", rvd.cpu(), rv_ref)[1] < 1e-5


def test_mse_seed(ops):
    S, h = 2, 8
    hw = h * h
    d = dev()
    out = rnd(2 * S * hw, 8, seed=1)
    tgt = torch.randn(S, 4, h, h)
    dO, loss = ops.lgp_mse_seed(out.to(d), tgt.to(d), S, h, 32, 4096.0)
    oc = out[S * hw:, :4].float().reshape(S, hw, 4).permute(0, 2, 1).reshape(S, 4, h, h)
    for s in range(S):
        assert abs(float(loss[s]) - float(F.mse_loss(oc[s], tgt[s]))) < 1e-5
    ref = 4096.0 * 2 * (oc - tgt) / (4 * hw)
    got = dO[S * hw:, :4].float().cpu().reshape(S, hw, 4).permute(0, 2, 1).reshape(S, 4, h, h)
    assert report("mse seed", got, ref)[0] < FP16_RND
    assert dO[:S * hw].abs().max() == 0 and dO[:, 4:].abs().max() == 0


# ------------------------------------------------------------------------- conv2 + conv_shortcut as one implicit GEMM
@pytest.mark.parametrize("rows,hw,cin,cout,cx,gn", [(16, 64, 320, 320, 640, True), (16, 64, 320, 320, 960, False), (8, 32, 640, 640, 1920, True),
                                                    (8, 32, 640, 640, 320, False), (8, 16, 1280, 1280, 2560, False), (16, 8, 1280, 1280, 2560, False),
                                                    (3, 32, 64, 160, 128, False)])
def test_conv3x3_with_folded_shortcut(ops, rows, hw, cin, cout, cx, gn):
    """skg_conv3x3_sc_f16 (round 5): Y = conv3x3(X) + X2 W_sc^T + bias with the 1x1 shortcut as K tiles behind the 3x3 walk - on the
    256 x 320 ping-pong tile (64 x 64 level), the 128 x 160 tiles, split-K (the small maps) alike - against (a) fp32 torch,
    (b) the two launches it replaces (the shortcut output is no longer rounded to fp16 on the way: rel <= 3e-4), and the GroupNorm
    partial sums of the output against the stand-alone statistics of what was written; bit-repeatable."""
    d = dev()
    g = torch.Generator().manual_seed(5)
    x = torch.randn(rows, cin, hw, hw, generator=g).half()
    x2 = torch.randn(rows * hw * hw, cx, generator=g).half()
    w = (torch.randn(cout, cin, 3, 3, generator=g) * (9 * cin) ** -0.5).half()
    wsc = (torch.randn(cout, cx, generator=g) * cx ** -0.5).half()
    b = (torch.randn(cout, generator=g) * 0.1).half()
    xn = x.permute(0, 2, 3, 1).reshape(-1, cin).contiguous().to(d)
    wp = w.permute(0, 2, 3, 1).reshape(cout, -1).contiguous()
    wcat = torch.cat([wp, wsc], 1).contiguous().to(d)
    G = 32 if cout % 32 == 0 else 8
    if gn:
        y, part = ops.conv3x3_sc(xn, x2.to(d), wcat, rows, hw, hw, bias=b.to(d), gn_groups=G)
    else:
        y = ops.conv3x3_sc(xn, x2.to(d), wcat, rows, hw, hw, bias=b.to(d))
    torch.cuda.synchronize()
    nr = min(rows, 2)
    ref = F.conv2d(x[:nr].float().to(d), w.float().to(d), b.float().to(d), padding=1).permute(0, 2, 3, 1).reshape(-1, cout) \
        + x2[:nr * hw * hw].float().to(d) @ wsc.float().to(d).t()
    r, _ = report(f"conv3x3 + shortcut rows{rows} {cin}->{cout} (+{cx}) @{hw} vs fp32", y[:nr * hw * hw].float().cpu(), ref.cpu())
    assert r < 4e-4
    sc = ops.gemm(x2.to(d), wsc.to(d))
    y2 = ops.conv3x3(xn, wp.to(d), rows, hw, hw, 0, bias=b.to(d), residual=sc)
    assert report("conv3x3 + shortcut vs the two launches", y.float().cpu(), y2.float().cpu())[0] < 4e-4
    y3 = ops.conv3x3_sc(xn, x2.to(d), wcat, rows, hw, hw, bias=b.to(d))
    assert torch.equal(y3, y)
    if gn:
        st = ops.groupnorm_stats(y, rows, hw * hw, G, 1e-5)
        gam, bet = torch.ones(cout).half().to(d), torch.zeros(cout).half().to(d)
        n_ref = ops.groupnorm_apply(y, rows, hw * hw, G, st, gam, bet, False)
        n_par, _ = ops.groupnorm(y, rows, hw * hw, G, 1e-5, gam, bet, False, partial=part)
        assert report("GroupNorm from the fused launch's partial sums", n_par.float().cpu(), n_ref.float().cpu())[0] < 2e-4
    # pair output (accuracy mode): hi + lo carries the fp32 result
    lo = torch.empty_like(y)
    hi = torch.empty_like(y)
    ops.conv3x3_sc(xn, x2.to(d), wcat, rows, hw, hw, out=hi, out_lo=lo, bias=b.to(d))
    rp, _ = report("conv3x3 + shortcut, pair output vs fp32", (hi[:nr * hw * hw].float() + lo[:nr * hw * hw].float()).cpu(), ref.cpu())
    assert rp < 1e-4 and torch.equal(hi, y)


# ------------------------------------------------------------------------------- Winograd F(2x2, 3x3), 16 x 16-level convolutions
@pytest.mark.parametrize("rows,hw,cin,cout", [(16, 16, 1280, 1280), (16, 16, 2560, 1280), (8, 16, 1280, 2560), (16, 16, 640, 1280),
                                              (2, 16, 1920, 1280), (8, 24, 640, 640), (3, 8, 64, 160), (1, 4, 128, 64)])
def test_conv3x3_winograd(ops, rows, hw, cin, cout):
    """skg_conv3x3_wino_f16 (round 6): input transform -> the GEMM kernel's split launch with one K slice per transform component ->
    output transform + epilogue, against (a) fp32 torch, (b) the implicit-GEMM convolution it replaces (the transformed operands carry
    one more fp16 rounding: rel <= 6e-4 of each other), with bias + residual, with a pair output, as the DATA GRADIENT through the dgrad
    pack (vs autograd), bit-repeatable; declined (-2) on an odd map."""
    from sketch2img_amd._lib import SkgError
    from sketch2img_amd.unet import pack_conv, pack_conv_dgrad, pack_conv_wino
    d = dev()
    g = torch.Generator().manual_seed(11)
    x = torch.randn(rows, cin, hw, hw, generator=g).half()
    w = (torch.randn(cout, cin, 3, 3, generator=g) * (9 * cin) ** -0.5).half()
    b = (torch.randn(cout, generator=g) * 0.1).half()
    res = torch.randn(rows * hw * hw, cout, generator=g).half()
    xn = x.permute(0, 2, 3, 1).reshape(-1, cin).contiguous().to(d)
    U = pack_conv_wino(w, d)
    y = ops.conv3x3_wino(xn, U, rows, hw, hw, bias=b.to(d), residual=res.to(d))
    torch.cuda.synchronize()
    nr = min(rows, 2)
    ref = F.conv2d(x[:nr].float().to(d), w.float().to(d), b.float().to(d), padding=1).permute(0, 2, 3, 1).reshape(-1, cout) \
        + res[:nr * hw * hw].float().to(d)
    r, _ = report(f"winograd conv rows{rows} {cin}->{cout} @{hw} vs fp32", y[:nr * hw * hw].float().cpu(), ref.cpu())
    assert r < 6e-4
    y2 = ops.conv3x3(xn, pack_conv(w, d), rows, hw, hw, 0, bias=b.to(d), residual=res.to(d))
    assert report("winograd vs the implicit GEMM", y.float().cpu(), y2.float().cpu())[0] < 6e-4
    assert torch.equal(ops.conv3x3_wino(xn, U, rows, hw, hw, bias=b.to(d), residual=res.to(d)), y)
    # no bias / residual, ReLU, pair output: hi + lo carries the fp32 result of the same arithmetic
    hi, lo = torch.empty_like(y), torch.empty_like(y)
    ops.conv3x3_wino(xn, U, rows, hw, hw, out=hi, out_lo=lo)
    y3 = ops.conv3x3_wino(xn, U, rows, hw, hw, relu=True)
    ref0 = F.conv2d(x[:nr].float().to(d), w.float().to(d), padding=1).permute(0, 2, 3, 1).reshape(-1, cout)
    assert torch.equal(y3, torch.relu(hi)) and report("winograd pair output vs fp32", (hi.float() + lo.float())[:nr * hw * hw].cpu(), ref0.cpu())[0] < 6e-4
    # the data gradient: dX = conv3x3(dY, flipped / transposed weights) = autograd of the forward
    dy = torch.randn(rows, cout, hw, hw, generator=g).half()
    dyn = dy.permute(0, 2, 3, 1).reshape(-1, cout).contiguous().to(d)
    if 64 * (rows * hw * hw // 4) * cin > ops.WORKSPACE_BYTES or cout % 64:      # the gradient's 16 fp32 slabs would not fit the stream's workspace / K tiles:
        with pytest.raises(SkgError) as e:                            # declined, nothing launched (HipUNet then runs the implicit GEMM)
            ops.conv3x3_wino(dyn, pack_conv_wino(w, d, dgrad=True), rows, hw, hw)
        assert e.value.rc == -2
        return
    dx = ops.conv3x3_wino(dyn, pack_conv_wino(w, d, dgrad=True), rows, hw, hw)
    xr = x[:nr].float().to(d).requires_grad_(True)
    F.conv2d(xr, w.float().to(d), padding=1).backward(dy[:nr].float().to(d))
    gref = xr.grad.permute(0, 2, 3, 1).reshape(-1, cin)
    assert report("winograd dgrad vs autograd", dx[:nr * hw * hw].float().cpu(), gref.cpu())[0] < 6e-4
    dx2 = ops.conv3x3(dyn, pack_conv_dgrad(w, d), rows, hw, hw)
    assert report("winograd dgrad vs the implicit-GEMM dgrad", dx.float().cpu(), dx2.float().cpu())[0] < 6e-4
    if hw % 2 == 0 and rows == 1:
        with pytest.raises(SkgError) as e:      # odd map: declined, nothing launched
            ops.conv3x3_wino(xn[: 3 * 3 * 1].contiguous(), U, 1, 3, 3)
        assert e.value.rc == -2


@pytest.mark.parametrize("rows,hw,c,cout", [(16, 16, 1280, 1280), (16, 16, 2560, 1280), (16, 8, 1280, 1280), (3, 8, 64, 160), (2, 16, 1920, 320)])
def test_groupnorm_writes_the_winograd_input_transform(ops, rows, hw, c, cout):
    """skg_groupnorm_wino_fwd: GroupNorm + SiLU of a small map with the normalised slice going to LDS and the Winograd input transform to
    memory - the convolution behind it and the published statistics must equal groupnorm() + conv3x3_wino() BIT FOR BIT; shapes whose
    (row, group) slice does not fit a workgroup (1920 channels: 60 per group) are declined."""
    from sketch2img_amd._lib import SkgError
    from sketch2img_amd.unet import pack_conv_wino
    d = dev()
    g = torch.Generator().manual_seed(13)
    G = 32 if c % 32 == 0 and c >= 256 else 8
    x = (torch.randn(rows * hw * hw, c, generator=g) * 1.5 + 0.3).half().to(d)
    gam, bet = (1 + 0.2 * torch.randn(c, generator=g)).half().to(d), (0.1 * torch.randn(c, generator=g)).half().to(d)
    w = (torch.randn(cout, c, 3, 3, generator=g) * (9 * c) ** -0.5).half()
    U = pack_conv_wino(w, d)
    if (c // G) % 8 != 0:
        with pytest.raises(SkgError) as e:
            ops.groupnorm_wino(x, rows, hw, hw, G, 1e-5, gam, bet, True)
        assert e.value.rc == -2
        return
    n, st = ops.groupnorm(x, rows, hw * hw, G, 1e-5, gam, bet, True)
    ya = ops.conv3x3_wino(n, U, rows, hw, hw)
    V, st2 = ops.groupnorm_wino(x, rows, hw, hw, G, 1e-5, gam, bet, True)
    yb = ops.conv3x3_wino(None, U, rows, hw, hw, V=V)
    torch.cuda.synchronize()
    assert torch.equal(st, st2) and torch.equal(ya, yb)
    ref = F.conv2d(F.silu(F.group_norm(x.float().reshape(rows, hw, hw, c).permute(0, 3, 1, 2), G, gam.float(), bet.float(), 1e-5)),
                   w.float().to(d), padding=1).permute(0, 2, 3, 1).reshape(-1, cout)
    assert report(f"GroupNorm + SiLU + winograd conv rows{rows} {c}->{cout} @{hw} vs fp32", yb.float().cpu(), ref.cpu())[0] < 8e-4


# ---------------------------------------------------------------------------------------------- sampler pointwise
def test_cfg_ddim_and_guidance_update(ops):
    from sketch2img_amd.sampler import DDIMTables
    from oracle import ddim as oddim
    S, h = 3, 16
    hw = h * h
    d = dev()
    g = torch.Generator().manual_seed(0)
    x = torch.randn(S, 4, h, h, generator=g)
    eps = rnd(2 * S * hw, 8, seed=1)
    tab, otab = DDIMTables.make(50), oddim.make_tables(50)
    assert tab.timesteps.tolist() == otab.timesteps.tolist()
    t = int(tab.timesteps[7])
    xp, e = ops.cfg_ddim_step(eps.to(d)[:S * hw], eps.to(d)[S * hw:], x.to(d), S, hw, 7.5, tab.coeffs(t), want_eps=True)
    eu = eps[:S * hw, :4].float().view(S, hw, 4).permute(0, 2, 1).reshape(S, 4, h, h)
    ec = eps[S * hw:, :4].float().view(S, hw, 4).permute(0, 2, 1).reshape(S, 4, h, h)
    er = eu + 7.5 * (ec - eu)
    assert report("cfg eps", e.cpu(), er)[1] < 1e-5
    assert report("ddim step", xp.cpu(), oddim.ddim_step(otab, er, t, x))[1] < 2e-5
    # v-prediction (SD2.1-768): the same CFG-combined tensor read as v; eps_out is the derived epsilon
    c0, c1 = tab.coeffs(t)[:2]
    xpv, ev = ops.cfg_ddim_step(eps.to(d)[:S * hw], eps.to(d)[S * hw:], x.to(d), S, hw, 7.5, tab.coeffs(t), want_eps=True,
                                v_prediction=True)
    assert report("ddim step, v-prediction", xpv.cpu(), oddim.ddim_step(otab, er, t, x, v_prediction=True))[1] < 2e-5
    assert report("derived eps, v-prediction", ev.cpu(), c0 * er + c1 * x)[1] < 1e-5
    grad = rnd(S * hw, 8, seed=2, scale=3.0)
    xprev = xp.clone()
    aux = ops.guidance_update(grad.to(d), x.to(d), xprev, S, hw, 1.6)
    gref = -grad[:, :4].float().view(S, hw, 4).permute(0, 2, 1).reshape(S, 4, h, h)
    for s in range(S):
        num = math.sqrt(2.0) * float((x[s] - xp[s].cpu()).norm())
        alpha = num / float(gref[s].norm()) * 1.6
        assert abs(float(aux[s, 0]) - alpha) / alpha < 1e-5
        assert report(f"guidance update s{s}", xprev[s].cpu(), xp[s].cpu() + alpha * gref[s])[1] < 1e-4


def test_cfg_dpmpp2m_step_vs_oracle(ops):
    """First-order then second-order DPM-Solver++ updates against oracle/dpmsolver.py (fp32 latents)."""
    from oracle import dpmsolver as odpm
    from sketch2img_amd.sampler import DPMTables
    S, h, ld = 2, 16, 8
    hw = h * h
    d = dev()
    tab, otab = DPMTables.make(25), odpm.make_tables(25)
    st = odpm.DPMState()
    x = torch.randn(S, 4, h, h, generator=torch.Generator().manual_seed(1))
    x0_io = torch.zeros(S, 4, h, h, device=d)
    xg, seen = x.to(d), 0
    for i in range(3):
        eps = rnd(2 * S * hw, ld, seed=10 + i)
        eu, ec = eps[:S * hw, :4].float(), eps[S * hw:, :4].float()
        er = (eu + 7.5 * (ec - eu)).reshape(S, hw, 4).permute(0, 2, 1).reshape(S, 4, h, h)
        order = tab.order(i, seen)
        xp, e = ops.cfg_dpmpp2m_step(eps.to(d)[:S * hw], eps.to(d)[S * hw:], xg, x0_io, S, hw, 7.5,
                                     tab.coeffs(i, order), want_eps=True)
        seen = min(seen + 1, 2)
        ref = odpm.dpm_step(otab, st, er, i, x)
        assert st.history[-1] == order
        assert report(f"dpm++ step {i} (order {order}) eps", e.cpu(), er)[1] < 1e-5
        assert report(f"dpm++ step {i} (order {order}) x_prev", xp.cpu(), ref)[1] < 2e-5
        assert report(f"dpm++ step {i} x0 history", x0_io.cpu(), st.x0_before)[0] < 1e-6      # |x0| ~ 450 at t = 999
        x, xg = ref, ref.to(d)
    # v-prediction: two steps (first order, then second order with the x0 history) against the oracle
    st = odpm.DPMState()
    x = torch.randn(S, 4, h, h, generator=torch.Generator().manual_seed(2))
    x0_io = torch.zeros(S, 4, h, h, device=d)
    xg, seen = x.to(d), 0
    for i in range(2):
        eps = rnd(2 * S * hw, ld, seed=20 + i)
        eu, ec = eps[:S * hw, :4].float(), eps[S * hw:, :4].float()
        vr = (eu + 7.5 * (ec - eu)).reshape(S, hw, 4).permute(0, 2, 1).reshape(S, 4, h, h)
        order = tab.order(i, seen)
        xp = ops.cfg_dpmpp2m_step(eps.to(d)[:S * hw], eps.to(d)[S * hw:], xg, x0_io, S, hw, 7.5, tab.coeffs(i, order),
                                  v_prediction=True)
        seen = min(seen + 1, 2)
        ref = odpm.dpm_step(otab, st, vr, i, x, v_prediction=True)
        assert report(f"dpm++ v-prediction step {i} x_prev", xp.cpu(), ref)[1] < 2e-5
        assert report(f"dpm++ v-prediction step {i} x0 history", x0_io.cpu(), st.x0_before)[1] < 2e-5
        x, xg = ref, ref.to(d)


# ------------------------------------------------------------------------------------------------ round-1 additions
def test_softmax_rows_and_quick_gelu(ops):
    x = rnd(300, 4096, seed=1, scale=3.0)
    y = ops.softmax_rows(x.to(dev()))
    ref = torch.softmax(x.float(), dim=-1)
    assert report("softmax rows", y.float().cpu(), ref)[0] < FP16_RND and abs(float(y.float().sum(1).mean()) - 1) < 1e-3
    big = torch.zeros(16, 64, dtype=torch.float16)
    big[:, 3] = 60000.0                                           # near the fp16 maximum: no overflow in the kernel
    z = ops.softmax_rows(big.to(dev())).cpu()
    assert torch.isfinite(z).all() and float(z[:, 3].min()) == 1.0
    h = rnd(777, 256, seed=2, scale=2.0)
    g = ops.quick_gelu(h.to(dev()))
    assert report("quick_gelu", g.float().cpu(), h.float() * torch.sigmoid(1.702 * h.float()))[0] < FP16_RND
    e = ops.gelu(h.to(dev()))
    assert report("gelu", e.float().cpu(), F.gelu(h.float()))[0] < FP16_RND


def test_image_postprocess_and_gaussian_sample(ops):
    S, h = 3, 8
    y = rnd(S * h * h, 8, seed=3, scale=1.5)
    img = ops.image_postprocess(y.to(dev()), S * h * h, 3)
    ref = (y[:, :3].float() / 2 + 0.5).clamp(0, 1)
    assert img.shape == (S * h * h, 3) and report("image postprocess", img.cpu(), ref)[1] < 1e-6
    m = rnd(S * h * h, 8, seed=4)
    m[:, 4:] = m[:, 4:] * 30                                       # exercise the logvar clamp [-30, 20]
    noise = torch.randn(S, 4, h, h, generator=torch.Generator().manual_seed(5))
    z = ops.gaussian_sample(m.to(dev()), S, 4, h * h, noise.to(dev()), 0.18215).reshape(S, 4, h, h)
    mm = m.float().reshape(S, h * h, 8).permute(0, 2, 1).reshape(S, 8, h, h)
    ref = (mm[:, :4] + torch.exp(0.5 * mm[:, 4:].clamp(-30, 20)) * noise) * 0.18215
    assert report("gaussian sample", z.cpu(), ref)[0] < 1e-5
    mode = ops.gaussian_sample(m.to(dev()), S, 4, h * h, None, 1.0).reshape(S, 4, h, h)
    assert report("gaussian mode", mode.cpu(), mm[:, :4])[1] < 1e-6


def test_training_helpers_colsum_bn_param_grads_adamw(ops):
    M, C = 5000, 256
    x, dy = rnd(M, C, seed=6), rnd(M, C, seed=7, scale=0.1)
    cs = ops.colsum(x.to(dev()), 0.5)
    assert report("colsum", cs.cpu(), 0.5 * x.float().sum(0))[0] < 1e-5
    st = ops.bn_stats(x.to(dev()), 1, 1, M)
    dg, db = ops.bn_param_grads(x.to(dev()), dy.to(dev()), st)
    xf = x.float()
    xhat = (xf - xf.mean(0)) / torch.sqrt(xf.var(0, unbiased=False) + 1e-5)
    assert report("bn dgamma", dg.cpu(), (dy.float() * xhat).sum(0))[0] < 1e-4
    assert report("bn dbeta", db.cpu(), dy.float().sum(0))[0] < 1e-5
    n = 10007
    gen = torch.Generator().manual_seed(8)
    p0, g0 = torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 4096
    pt = p0.clone().requires_grad_(True)
    opt = torch.optim.AdamW([pt], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
    p, m, v = p0.clone().to(dev()), torch.zeros(n, device=dev()), torch.zeros(n, device=dev())
    p16 = torch.empty(n, device=dev(), dtype=torch.float16)
    for step in (1, 2, 3):
        pt.grad = g0.clone() / 4096 * step
        opt.step()
        ops.adamw_step(p, (g0 * step).to(dev()), m, v, p16, 1e-3, 0.9, 0.999, 1e-8, 0.05, step, 1.0 / 4096)
    assert report("adamw 3 steps", p.cpu(), pt.detach())[1] < 2e-6
    assert torch.equal(p16.float().cpu(), p.cpu().half().float())
    E = ops.lgp_extra_features(torch.ones(2, 4, 4, 4, device=dev()) * 0.25, 2.0, 2, 2, 4, 64).float().cpu()
    assert E.shape == (32, 64) and float(E[:, 40:].abs().max()) == 0.0
    assert abs(float(E[0, 0]) - 0.5) < 1e-3 and abs(float(E[0, 4]) - math.sin(2 * math.pi * 0.5)) < 2e-3


# ---------------------------------------------------------------------------------------------- fused FF sub-block
@pytest.mark.parametrize("M,Fh", [(4096, 1280), (128 * 5 + 37, 1280), (16, 64), (65536, 1280)])
def test_ff_block_fused(ops, M, Fh):
    """skg_ff_block_f16 (norm3 -> ff.net.0.proj with the GEGLU gate -> ff.net.2 + residual in ONE launch, C = 320) against
    (a) the fp32 definition on the same fp16 inputs: one output rounding + the three internal fp16 roundings the unfused
    path has as well (LayerNorm output, FF1 output, gated value): rel <= 1.5 x FP16_RND on an O(1) residual stream;
    (b) the three-launch path it replaces (skg_layernorm_fwd, skg_gemm_f16 + SKG_EPI_GEGLU, skg_gemm_f16 + residual), which
    rounds at the same points: the two differ only by fp32 summation order, i.e. by rare 1-ulp flips - rel <= 2e-4,
    >= 98 % of the outputs bit-equal (measured 98.9-99.0 %); LayerNorm statistics equal to skg_layernorm_fwd's to 1e-6; in place == out of place."""
    from sketch2img_amd.unet import pack_ff_block
    d = dev()
    C = 320
    x = rnd(M, C, seed=11)
    gam, bet = (1 + 0.2 * rnd(C, seed=12).float()).half(), (0.1 * rnd(C, seed=13).float()).half()
    w1, b1 = rnd(2 * Fh, C, seed=14, scale=C ** -0.5), rnd(2 * Fh, seed=15, scale=0.1)
    w2, b2 = rnd(C, Fh, seed=16, scale=Fh ** -0.5), rnd(C, seed=17, scale=0.1)
    pack, bias1 = pack_ff_block(w1, b1, w2, d)
    xd = x.to(d)
    y, st = ops.ff_block(xd, gam.to(d), bet.to(d), 1e-5, pack, bias1, b2.to(d), want_stats=True)
    torch.cuda.synchronize()
    # (a) fp32 definition
    a = F.layer_norm(x.float(), (C,), gam.float(), bet.float(), 1e-5)
    hid = a @ w1.float().t() + b1.float()
    ref = x.float() + (hid[:, :Fh] * F.gelu(hid[:, Fh:])) @ w2.float().t() + b2.float()
    r, _ = report(f"ff_block M{M} F{Fh} vs fp32", y.float().cpu(), ref)
    assert r < 1.5 * FP16_RND
    # (b) the three launches it replaces
    idx = ops.geglu_interleave_index(Fh)
    a3, st3 = ops.layernorm(xd, gam.to(d), bet.to(d), 1e-5, want_stats=True)
    gg = ops.gemm(a3, w1[idx].contiguous().to(d), bias=b1[idx].contiguous().to(d), geglu=True)
    y3 = ops.gemm(gg, w2.to(d), bias=b2.to(d), residual=xd)
    r3, _ = report(f"ff_block M{M} F{Fh} vs three launches", y.float().cpu(), y3.float().cpu())
    same = float((y == y3).float().mean())
    print(f"[parity] ff_block bit-equal outputs: {same:.5f}")
    assert r3 < 2e-4 and same > 0.98
    assert torch.allclose(st, st3, rtol=1e-5, atol=1e-6)
    y_in = xd.clone()
    ops.ff_block(y_in, gam.to(d), bet.to(d), 1e-5, pack, bias1, b2.to(d), out=y_in)
    assert torch.equal(y_in, y)
    # strided views (the residual stream is sometimes a column slice of a wider buffer)
    wide = torch.zeros(M, 2 * C, device=d, dtype=torch.float16)
    wide[:, C:] = xd
    outw = torch.zeros(M, 2 * C + 8, device=d, dtype=torch.float16)
    ops.ff_block(wide[:, C:], gam.to(d), bet.to(d), 1e-5, pack, bias1, b2.to(d), out=outw[:, 8:8 + C])
    assert torch.equal(outw[:, 8:8 + C], y) and float(outw[:, :8].abs().max()) == 0 and float(outw[:, 8 + C:].abs().max()) == 0


@pytest.mark.parametrize("rows,HW", [(2, 1024), (16, 4096), (3, 256)])
def test_ff_block_with_proj_out(ops, rows, HW):
    """skg_ff_block_proj_f16: the fused feed-forward launch followed by Transformer2DModel.proj_out + the outer residual without the
    block output leaving the registers, against the two launches it replaces (skg_ff_block_f16, then skg_gemm_f16 + residual with
    GroupNorm partial sums - same rounding points: rel <= 3e-4, >= 97 % bit-equal) and against the fp32 definition; the stashing
    form (statistics, FF1 pre-activation of the rows >= keep_from) equals skg_ff_block_f16_keep's; GroupNorm from the partial sums
    equals GroupNorm of the tensor; output into a strided view, R as the output buffer."""
    from sketch2img_amd.unet import pack_ff_block
    d = dev()
    C, Fh, M, G = 320, 1280, rows * HW, 32
    x, R = rnd(M, C, seed=71).to(d), rnd(M, C, seed=72).to(d)
    gam, bet = (1 + 0.2 * rnd(C, seed=73).float()).half().to(d), (0.1 * rnd(C, seed=74).float()).half().to(d)
    w1, b1 = rnd(2 * Fh, C, seed=75, scale=C ** -0.5), rnd(2 * Fh, seed=76, scale=0.1)
    w2, b2 = rnd(C, Fh, seed=77, scale=Fh ** -0.5), rnd(C, seed=78, scale=0.1).to(d)
    wp, bp = rnd(C, C, seed=79, scale=C ** -0.5), rnd(C, seed=80, scale=0.1).to(d)
    pack, bias1 = pack_ff_block(w1, b1, w2, d)
    packp, bias1p = pack_ff_block(w1, b1, w2, d, w_proj=wp)
    assert torch.equal(packp[:Fh // 32], pack) and torch.equal(bias1p, bias1)
    kf = (rows // 2) * HW
    p3, st0, pre0 = ops.ff_block(x, gam, bet, 1e-5, pack, bias1, b2, want_stats=True, keep_from=kf)
    y2, part2 = ops.gemm(p3, wp.to(d), bias=bp, residual=R, gn_stats=(HW, G))
    buf = torch.full((M, C + 16), 7.0, device=d, dtype=torch.float16)
    y, st, pre, part = ops.ff_block_proj(x, gam, bet, 1e-5, packp, bias1, b2, bp, R, out=buf[:, 8:8 + C], want_stats=True, keep_from=kf,
                                         gn=(HW, G))
    e2 = rel_err(y, y2)
    same = float((y == y2).float().mean())
    stray = float((buf[:, :8] - 7).abs().max() + (buf[:, 8 + C:] - 7).abs().max())
    sel = slice(0, min(M, 8192))
    a = F.layer_norm(x.float()[sel], (C,), gam.float(), bet.float(), 1e-5)
    hid = a @ w1.float().to(d).t() + b1.float().to(d)
    p3f = x.float()[sel] + (hid[:, :Fh] * F.gelu(hid[:, Fh:])) @ w2.float().to(d).t() + b2.float()
    ref = R.float()[sel] + p3f @ wp.float().to(d).t() + bp.float()
    e = rel_err(y[sel], ref)
    print(f"[parity] ff_block_proj rows{rows} HW{HW}: rel {e:.2e} vs fp32, {e2:.2e} vs ff_block + gemm (bit-equal {same:.4f}), stray {stray}")
    assert e < 2 * FP16_RND and e2 < 3e-4 and same > 0.97 and stray == 0
    assert torch.equal(st, st0) and torch.equal(pre, pre0)
    gnw, gnb = (1 + 0.1 * rnd(C, seed=81).float()).half().to(d), (0.1 * rnd(C, seed=82).float()).half().to(d)
    ga, _ = ops.groupnorm(y.contiguous(), rows, HW, G, 1e-6, gnw, gnb, False, partial=part)
    gb, _ = ops.groupnorm(y.contiguous(), rows, HW, G, 1e-6, gnw, gnb, False)
    gc, _ = ops.groupnorm(y2, rows, HW, G, 1e-6, gnw, gnb, False, partial=part2)
    print(f"[parity] GroupNorm from the launch's partial sums vs from the tensor: rel {rel_err(ga, gb):.2e}; vs the gemm's partials {rel_err(ga, gc):.2e}")
    assert rel_err(ga, gb) < 1e-3 and rel_err(ga, gc) < 1e-3
    again = R.clone()      # R as the output buffer (the caller's residual slot), no stash, no statistics
    ops.ff_block_proj(x, gam, bet, 1e-5, packp, bias1, b2, bp, again, out=again)
    assert torch.equal(again, y)


@pytest.mark.parametrize("rows,HW", [(2, 1024), (4, 4096)])
def test_ff_block_with_proj_out_pairs(ops, rows, HW):
    """skg_ff_block_proj_f16_hilo (accuracy mode, round 5): pair in, pair out, pair outer residual; proj_out takes the block output as
    the pair it is.  Against the fp32 definition on the fp32 value of the input pairs (hi + lo of the output: rel <= 3e-4 - the
    roundings left are the fp16 MFMA operands inside), against the two launches it replaces (skg_ff_block_f16_hilo, then the
    K-doubled skg_gemm_f16_hilo_gn), the stash against skg_ff_block_f16_hilo's, GroupNorm from the partial sums."""
    from sketch2img_amd.ops import Pair
    from sketch2img_amd.unet import pack_ff_block
    d = dev()
    C, Fh, M, G = 320, 1280, rows * HW, 32

    def pair_of(t32):
        pr = Pair.empty(M, C, d)
        hi = t32.half()
        pr.hi.copy_(hi.to(d)); pr.lo.copy_((t32 - hi.float()).half().to(d))
        return pr

    x32, r32 = rnd(M, C, seed=71).float() * 1.0003, rnd(M, C, seed=72).float() * 0.9997      # (values that need their lo parts)
    X, R = pair_of(x32), pair_of(r32)
    xv, rv = (X.hi.float() + X.lo.float()), (R.hi.float() + R.lo.float())
    gam, bet = (1 + 0.2 * rnd(C, seed=73).float()).half().to(d), (0.1 * rnd(C, seed=74).float()).half().to(d)
    w1, b1 = rnd(2 * Fh, C, seed=75, scale=C ** -0.5), rnd(2 * Fh, seed=76, scale=0.1)
    w2, b2 = rnd(C, Fh, seed=77, scale=Fh ** -0.5), rnd(C, seed=78, scale=0.1).to(d)
    wp, bp = rnd(C, C, seed=79, scale=C ** -0.5), rnd(C, seed=80, scale=0.1).to(d)
    pack, bias1 = pack_ff_block(w1, b1, w2, d)
    packp, _ = pack_ff_block(w1, b1, w2, d, w_proj=wp)
    kf = (rows // 2) * HW
    p3, st0, pre0 = ops.ff_block(X, gam, bet, 1e-5, pack, bias1, b2, want_stats=True, keep_from=kf)
    y2 = Pair.empty(M, C, d)
    w2x = torch.cat([wp, wp], 1).contiguous().to(d)
    _, part2 = ops.gemm(p3.full, w2x, out=y2.hi, out_lo=y2.lo, bias=bp, residual=R.hi, residual_lo=R.lo, gn_stats=(HW, G))
    out = Pair.empty(M, C, d)
    y, st, pre, part = ops.ff_block_proj(X, gam, bet, 1e-5, packp, bias1, b2, bp, R, out=out, want_stats=True, keep_from=kf, gn=(HW, G))
    sel = slice(0, min(M, 8192))
    a = F.layer_norm(xv[sel], (C,), gam.float(), bet.float(), 1e-5)
    hid = a @ w1.float().to(d).t() + b1.float().to(d)
    p3f = xv[sel] + (hid[:, :Fh] * F.gelu(hid[:, Fh:])) @ w2.float().to(d).t() + b2.float()
    ref = rv[sel] + p3f @ wp.float().to(d).t() + bp.float()
    yv, y2v = y.hi.float() + y.lo.float(), y2.hi.float() + y2.lo.float()
    e, e2 = rel_err(yv[sel], ref), rel_err(yv, y2v)
    print(f"[parity] ff_block_proj on pairs rows{rows} HW{HW}: hi + lo rel {e:.2e} vs fp32 (hi alone {rel_err(y.hi[sel], ref):.2e}), "
          f"{e2:.2e} vs ff_block_hilo + K-doubled gemm")
    assert e < 3e-4 and e2 < 2e-4
    assert torch.equal(st, st0) and torch.equal(pre, pre0)
    gnw, gnb = (1 + 0.1 * rnd(C, seed=81).float()).half().to(d), (0.1 * rnd(C, seed=82).float()).half().to(d)
    ga, _ = ops.groupnorm(y.hi.contiguous(), rows, HW, G, 1e-6, gnw, gnb, False, partial=part)
    gb, _ = ops.groupnorm(y.hi.contiguous(), rows, HW, G, 1e-6, gnw, gnb, False)
    assert rel_err(ga, gb) < 1e-3
    y3 = ops.ff_block_proj(X, gam, bet, 1e-5, packp, bias1, b2, bp, R, out=Pair.empty(M, C, d))[0]
    assert torch.equal(y3.hi, y.hi) and torch.equal(y3.lo, y.lo)


def test_ff_block_keep_stores_the_pre_activation(ops):
    """skg_ff_block_f16_keep: the cond rows of a guided step (rows >= keep_from) also get the FF1 output in the interleaved pack
    order - what skg_gemm_f16_geglu_keep writes and skg_geglu_bwd reads.  Same MFMA products and the same fp16 rounding as the
    GEMM path up to fp32 summation order: rel <= 1e-4, >= 98 % bit-equal; the output is unchanged by the extra stores."""
    from sketch2img_amd.unet import pack_ff_block
    d = dev()
    C, Fh, M, M0 = 320, 1280, 128 * 6 + 48, 128 * 3 + 16
    x = rnd(M, C, seed=21)
    gam, bet = (1 + 0.2 * rnd(C, seed=22).float()).half(), (0.1 * rnd(C, seed=23).float()).half()
    w1, b1 = rnd(2 * Fh, C, seed=24, scale=C ** -0.5), rnd(2 * Fh, seed=25, scale=0.1)
    w2, b2 = rnd(C, Fh, seed=26, scale=Fh ** -0.5), rnd(C, seed=27, scale=0.1)
    pack, bias1 = pack_ff_block(w1, b1, w2, d)
    xd = x.to(d)
    y0 = ops.ff_block(xd, gam.to(d), bet.to(d), 1e-5, pack, bias1, b2.to(d))
    y, st, pre = ops.ff_block(xd, gam.to(d), bet.to(d), 1e-5, pack, bias1, b2.to(d), want_stats=True, keep_from=M0)
    assert torch.equal(y, y0) and pre.shape == (M - M0, 2 * Fh)
    idx = ops.geglu_interleave_index(Fh)
    a3 = ops.layernorm(xd[M0:], gam.to(d), bet.to(d), 1e-5)
    _, f = ops.gemm_geglu_keep(a3, w1[idx].contiguous().to(d), b1[idx].contiguous().to(d))
    r, _ = report("ff_block keep vs gemm_geglu_keep", pre.float().cpu(), f.float().cpu())
    same = float((pre == f).float().mean())
    print(f"[parity] ff_block keep bit-equal: {same:.5f}")
    assert r < 1e-4 and same > 0.98
    # and the gate's backward accepts it
    dy = rnd(M - M0, Fh, seed=28).to(d)
    assert rel_err(ops.geglu_bwd(pre, dy, interleaved=True), ops.geglu_bwd(f, dy, interleaved=True)) < 2e-4


# ---------------------------------------------------------------------------------------------- fused cross-attention sub-block
@pytest.mark.parametrize("rows,HW,L,heads", [(2, 1024, 77, 8), (16, 4096, 77, 8), (3, 128, 40, 8), (2, 1024, 77, 5), (4, 9216, 77, 5), (3, 128, 33, 5)])
def test_xattn_block_fused(ops, rows, HW, L, heads):
    """skg_xattn_block_f16 (norm2 -> attn2.to_q -> attention over the text keys -> attn2.to_out + residual in ONE launch,
    C = 320, 8 heads of 40) against (a) the fp32 definition on the same fp16 inputs: the output rounding plus the internal fp16
    roundings the unfused path has too (LayerNorm output, q, scaled q, probabilities, attention output) - rel <= 2 x FP16_RND
    on an O(1) residual stream (heads = 5: the 5 x 64 instantiation of SD2.1's first level, round 5); (b) the four launches it replaces (skg_layernorm_fwd, skg_gemm_f16, skg_attn_fwd_rowv,
    skg_gemm_f16 + residual), which round at the same points: rel <= 3e-4, >= 95 % of the outputs bit-equal; in place == out of place."""
    from sketch2img_amd.unet import pack_xattn_kv, pack_xattn_weights
    d = dev()
    C, Lp = 320, 80
    dh = C // heads
    M = rows * HW
    scale = dh ** -0.5
    x = rnd(M, C, seed=31)
    gam, bet = (1 + 0.2 * rnd(C, seed=32).float()).half(), (0.1 * rnd(C, seed=33).float()).half()
    wq, wo, bo = rnd(C, C, seed=34, scale=C ** -0.5), rnd(C, C, seed=35, scale=C ** -0.5), rnd(C, seed=36, scale=0.1)
    K, V = rnd(rows * Lp, C, seed=37), rnd(rows * Lp, C, seed=38)
    wp = pack_xattn_weights(wq, wo, heads, d)
    kvp = pack_xattn_kv(K.to(d), V.to(d), rows, Lp, L, heads)
    xd = x.to(d)
    y = ops.xattn_block(xd, HW, heads, L, gam.to(d), bet.to(d), 1e-5, wp, kvp, bo.to(d), scale)
    torch.cuda.synchronize()
    # (b) the four launches
    a2 = ops.layernorm(xd, gam.to(d), bet.to(d), 1e-5)
    q2 = ops.gemm(a2, wq.to(d))
    o2 = ops.attn_fwd(q2, K.to(d), V.to(d), rows, heads, HW, L, Lp, dh, scale, v_rows=True)
    y4 = ops.gemm(o2, wo.to(d), bias=bo.to(d), residual=xd)
    r4, _ = report(f"xattn_block rows{rows} HW{HW} L{L} vs four launches", y.float().cpu(), y4.float().cpu())
    same = float((y == y4).float().mean())
    print(f"[parity] xattn_block bit-equal outputs: {same:.5f}")
    # (a) fp32 definition (a subset of the rows at the large size: the CPU reference is the slow part)
    sel = slice(0, min(M, 8192))
    b = (torch.arange(M)[sel] // HW)
    a = F.layer_norm(x.float()[sel], (C,), gam.float(), bet.float(), 1e-5)
    q = (a @ wq.float().t()).reshape(-1, heads, dh)
    Kf = K.float().reshape(rows, Lp, heads, dh)[:, :L][b]            # [m, L, heads, dh]
    Vf = V.float().reshape(rows, Lp, heads, dh)[:, :L][b]
    att = torch.softmax(torch.einsum("mhd,mlhd->mhl", q, Kf) * scale, -1)
    o = torch.einsum("mhl,mlhd->mhd", att, Vf).reshape(-1, C)
    ref = x.float()[sel] + o @ wo.float().t() + bo.float()
    r, _ = report(f"xattn_block rows{rows} HW{HW} L{L} vs fp32", y.float().cpu()[sel], ref)
    assert r < 2 * FP16_RND
    assert r4 < 3e-4 and same > 0.95
    y_in = xd.clone()
    ops.xattn_block(y_in, HW, heads, L, gam.to(d), bet.to(d), 1e-5, wp, kvp, bo.to(d), scale, out=y_in)
    assert torch.equal(y_in, y)
    # (c) the stashing launch (skg_xattn_block_f16_keep): the same output (to 1 ulp on a few outputs), and for the rows of the last images what the
    # backward of the replaced launches reads - norm2's statistics, q, the attention output, lse - against those launches' own
    kf = (rows // 2) * HW
    a2k, st_ref = ops.layernorm(xd[kf:], gam.to(d), bet.to(d), 1e-5, want_stats=True)
    o2k, lse_ref = ops.attn_fwd(q2[kf:], K.to(d)[(rows // 2) * Lp:], V.to(d)[(rows // 2) * Lp:], rows - rows // 2, heads, HW, L, Lp, dh, scale,
                                want_lse=True, v_rows=True)
    yk, stk, qk, ok, lsek = ops.xattn_block(xd, HW, heads, L, gam.to(d), bet.to(d), 1e-5, wp, kvp, bo.to(d), scale, keep_from=kf)
    neq = (yk != y)
    print(f"[parity] xattn_block_keep output vs plain launch: differing {float(neq.float().mean()):.5f} (rows below keep_from {float(neq[:kf].float().mean()):.5f}, "
          f"from it {float(neq[kf:].float().mean()):.5f}), rel {rel_err(yk, y):.2e}, max abs {float((yk.float() - y.float()).abs().max()):.3e}")
    # (another instantiation of the same source: hipcc contracts one fp32 expression differently - 1 ulp of fp16 on ~2e-4 of the outputs,
    # on both sides of keep_from alike; the launch itself is bit-repeatable)
    yk2 = ops.xattn_block(xd, HW, heads, L, gam.to(d), bet.to(d), 1e-5, wp, kvp, bo.to(d), scale, keep_from=kf)[0]
    assert torch.equal(yk2, yk) and float(neq.float().mean()) < 1e-3 and rel_err(yk, y) < 1e-5
    e_st = float((stk - st_ref.reshape(-1, 2)).abs().max() / st_ref.abs().max())
    e_q = rel_err(qk, q2[kf:])
    e_o = rel_err(ok, o2k)
    e_l = float((lsek.reshape(-1) - lse_ref.reshape(-1)).abs().max())
    print(f"[parity] xattn_block_keep rows{rows} HW{HW}: stats {e_st:.1e}  q rel {e_q:.1e} (bit-equal {float((qk == q2[kf:]).float().mean()):.4f})  "
          f"o rel {e_o:.1e}  lse max abs {e_l:.1e}")
    assert e_st < 1e-5 and e_q < 3e-4 and e_o < 6e-4 and e_l < 2e-3
    # ... and the backward launches accept them: dq from the stash of the fused launch == dq from the unfused stash within rounding
    do = rnd(M - kf, C, seed=39).to(d)
    S2 = rows - rows // 2
    Kc, Vc = K.to(d)[(rows // 2) * Lp:], V.to(d)[(rows // 2) * Lp:]
    dq_a = ops.attn_bwd_dq(qk, Kc, Vc, do, lsek, ops.attn_bwd_delta(ok, do, S2, heads, HW, dh), S2, heads, HW, L, Lp, dh, scale)
    dq_b = ops.attn_bwd_dq(q2[kf:], Kc, Vc, do, lse_ref, ops.attn_bwd_delta(o2k, do, S2, heads, HW, dh), S2, heads, HW, L, Lp, dh, scale)
    assert rel_err(dq_a, dq_b) < 2e-3
