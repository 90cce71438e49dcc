"""Exact-integer probes of the matrix-pipe kernels on the device (tests/exact_probes.py has the method, the cases and the references).

Every case asserts the code path it was written for (skg_gemm_variant / skg_gemm_gn_fused) and ZERO mismatching bit patterns over all
samples against a plain torch reference on the CPU.  Run with ``-s`` for one ``EXACT ...`` record line per case (variant number,
element count, mismatch count)."""
import os
import subprocess
import sys

import pytest
import torch

from tests import exact_probes as ep

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from sketch2img_amd import ops as o
    return o


@pytest.fixture(scope="module")
def lib():
    from sketch2img_amd._lib import lib as l_
    return l_


def _cases(table):
    return [pytest.param(c, cls, id=f"{c.name}-{cls}") for c in table for cls in c.classes]


# ------------------------------------------------------------------------------------------------------------ skg_gemm_f16
@pytest.mark.parametrize("case,cls", _cases(ep.GEMM_CASES))
def test_gemm_exact(case, cls):
    ep.run_gemm(case, cls)


@pytest.mark.parametrize("cls", ["small"])
@pytest.mark.parametrize("M,N,K,seg,stride", ep.ROWS_CASES)
def test_gemm_rows_exact(ops, M, N, K, seg, stride, cls):
    """skg_gemm_f16_rows with seg_rows that is no multiple of 128: product row m lands in row (m / seg) * stride + m % seg; the rows
    between the segments and the guard columns keep their fill."""
    name = f"gemm_rows {M}x{N}x{K} seg{seg}/{stride}"
    A = ep.draw_int((M, K), 3, ep.seed_of(name, cls, 0))
    B = ep.draw_int((N, K), 1, ep.seed_of(name, cls, 1))
    bias = ep.draw_int((N,), 8, ep.seed_of(name, cls, 2))
    ep.check_order_free(A.abs(), B.abs(), 8)
    v = ep.epilogue(A.double() @ B.double().t(), bias)
    R = (M // seg - 1) * stride + seg + 5
    want = torch.full((R, N), ep.GUARD, dtype=torch.float16)
    for b in range(M // seg):
        want[b * stride:b * stride + seg] = v[b * seg:(b + 1) * seg].half()
    out = torch.full((R, N + 8), ep.GUARD, device=dev(), dtype=torch.float16)
    Ad, Bd, bd = A.to(dev()), B.to(dev()), bias.to(dev())
    rc = ops.lib.skg_gemm_f16_rows(Ad.data_ptr(), K, Bd.data_ptr(), K, out.data_ptr(), N + 8, M, N, K, bd.data_ptr(), seg, stride, ops._stream())
    assert rc == 0, f"skg_gemm_f16_rows declined or failed: {rc}"      # (ops.gemm_rows would fall back to one GEMM per segment)
    ep.assert_bits_equal(out, want, ep.Layout.matrix(R, N, 64, None, name))
    ep.record(name, cls, "rows", M * N, 0)


@pytest.mark.parametrize("M,N,K", ep.GEGLU_KEEP_CASES)
def test_geglu_keep_pre_activation_exact(ops, M, N, K):
    """The H output of skg_gemm_f16_geglu_keep = A . B^T + bias in the pack's row order (the gated Y is not exact: out of scope)."""
    name = f"geglu_keep H {M}x{N}x{K}"
    A = ep.draw_int((M, K), 3, ep.seed_of(name, "small", 0))
    B = ep.draw_int((N, K), 1, ep.seed_of(name, "small", 1))
    bias = ep.draw_int((N,), 8, ep.seed_of(name, "small", 2))
    ep.check_order_free(A.abs(), B.abs(), 8)
    v = ep.epilogue(A.double() @ B.double().t(), bias)
    pre = torch.full((M, N + 8), ep.GUARD, device=dev(), dtype=torch.float16)
    ops.gemm_geglu_keep(A.to(dev()), B.to(dev()), bias.to(dev()), pre=pre[:, :N])
    ep.assert_bits_equal(pre, v.half(), ep.Layout.matrix(M, N, 64, None, name))
    ep.record(name, "small", "geglu_keep", M * N, 0)


# --------------------------------------------------------------------------------------------------------- skg_conv3x3_f16
@pytest.mark.parametrize("case,cls", _cases(ep.CONV_CASES))
def test_conv3x3_exact(case, cls):
    ep.run_conv(case, cls)


_big_dev = {}


def _big_operands(rows, H, cls):
    from sketch2img_amd.packs import pack_conv
    key = (rows, H, cls)
    if key not in _big_dev:
        _big_dev.clear()                                  # (one draw on the device at a time)
        x, w, acc = ep.big_conv_ref(rows, H, cls)
        _big_dev[key] = (ep.nhwc(x).to(dev()), pack_conv(w, dev()), acc)
    return _big_dev[key]


def _big_params():
    return [pytest.param(rows, H, variant, cls, id=f"rows{rows}@{H}x{H} [{variant}] {cls}")
            for rows, H in ep.BIG_CONV for variant, cls in ep.big_conv_variants(rows, H)]


@pytest.mark.parametrize("rows,H,variant,cls", _big_params())
def test_conv3x3_pingpong_tile_exact(ops, lib, rows, H, variant, cls):
    """The 256 x 320 ping-pong tile (8320) at the 64 x 64 level, 128 -> 320, all samples: whole tiles (14 @ 64 x 64) and ragged
    (15 @ 62 x 62); one reference per (x, w) draw, bias and residual added per variant."""
    d = dev()
    xd, wp, _ = _big_operands(rows, H, cls)
    words = variant.split()
    M, N, K, HW = rows * H * H, ep.BIG_COUT, 9 * ep.BIG_CIN, H * H
    name, bias, res, res_lo, v = ep.big_conv_value(rows, H, variant, cls)
    ops._stream()
    var = lib.skg_gemm_variant(M, N, K, ep.BIG_CIN, 1)
    assert var == 8320, f"{name}: skg_gemm_variant reports {var}"
    lay = ep.Layout(rows, H, H, N, 320, None, f"{name} / {cls}")
    todev = lambda t: None if t is None else t.to(d)      # noqa: E731
    extra = ""
    if "pair" in words:
        buf = torch.full((M, 2 * N), ep.GUARD, device=d, dtype=torch.float16)
        ops.conv3x3(xd, wp, rows, H, H, 0, out=buf[:, :N], out_lo=buf[:, N:], bias=todev(bias), residual=todev(res),
                    residual_lo=todev(res_lo))
        whi, wlo = ep.expected_pair(v)
        ep.assert_bits_equal(buf[:, :N].contiguous(), whi, lay)
        ep.assert_bits_equal(buf[:, N:].contiguous(), wlo, lay)
        extra = f" | lo != 0 on {float((wlo != 0).double().mean()):.2f}"
    else:
        out = torch.full((M, N), ep.GUARD, device=d, dtype=torch.float16)
        want = ep.expected_f16(v, cls)
        if "gn" in words:
            q = lib.skg_gemm_gn_fused(M, N, K, ep.BIG_CIN, 1, HW, ep.BIG_GROUPS)
            assert q == 1, f"{name}: skg_gemm_gn_fused reports {q}"
            _, part = ops.conv3x3(xd, wp, rows, H, H, 0, out=out, bias=todev(bias), gn_groups=ep.BIG_GROUPS)
            sums = ep.gn_sums(want, rows, HW, ep.BIG_GROUPS)
            got = part.buf.view(rows, HW // 128, ep.BIG_GROUPS, 2).double().cpu()
            nb = int((got != sums).sum())
            assert nb == 0, f"{name}: {nb} of {sums.numel()} GroupNorm partial sums differ from the fp64 sums of the fp16 outputs"
            extra = f" | gn fused 1, {sums.numel()} partial sums exact"
        else:
            ops.conv3x3(xd, wp, rows, H, H, 0, out=out, bias=todev(bias), residual=todev(res))
        ep.assert_bits_equal(out, want, lay)
    ep.record(name, cls, var, M * N, 0, extra)


# ----------------------------------------------------------------------------------------------------------------- relatives
CLS2 = ["small", "large"]


@pytest.mark.parametrize("cls", CLS2)
@pytest.mark.parametrize("case", ep.UP2_CASES)
def test_conv_up2_polyphase_exact(ops, case, cls):
    """skg_conv3x3_up2_f16: strided output with guard columns, pair output (pair_in = 0), pair input with a non-zero integer lo half."""
    from sketch2img_amd.packs import pack_conv_up2, pack_conv_up2_hilo
    rows, IH, IW, Cin, Cout = case
    d = dev()
    r = ep.up2_reference(*case, cls)
    M = rows * 4 * IH * IW
    lay = ep.Layout(rows, 2 * IH, 2 * IW, Cout, 160 if Cout % 160 == 0 else 64, None, f"{r['name']} / {cls}")
    xd, Wpp, bias = ep.nhwc(r["x"]).to(d), pack_conv_up2(r["w"], d), r["bias"].to(d)
    out = torch.full((M, Cout + 8), ep.GUARD, device=d, dtype=torch.float16)
    rc = ops.lib.skg_conv3x3_up2_f16(xd.data_ptr(), Cin, Wpp.data_ptr(), out.data_ptr(), None, Cout + 8, rows, IH, IW, Cin, Cout, 0,
                                     bias.data_ptr(), ops._stream())
    assert rc == 0, f"skg_conv3x3_up2_f16: {rc}"
    ep.assert_bits_equal(out, ep.expected_f16(r["v"], cls), lay)
    pr = ops.Pair.empty(M, Cout, d)
    ops.conv_up2_pairout(xd, Wpp, rows, IH, IW, pr, bias=bias)
    whi, wlo = ep.expected_pair(r["v"])
    ep.assert_bits_equal(pr.hi.contiguous(), whi, lay)
    ep.assert_bits_equal(pr.lo.contiguous(), wlo, lay)
    # pair input [x_hi | x_lo] against [W_hi | W_hi | W_lo] (W_lo = 0 for integer weights)
    r2 = ep.up2_reference(*case, cls, pair_in=True)
    assert bool((r2["x_lo"] != 0).any())
    x2 = torch.cat([ep.nhwc(r2["x"]), ep.nhwc(r2["x_lo"])], 1).contiguous().to(d)
    pr2 = ops.Pair.empty(M, Cout, d)
    ops.conv_up2_hilo(x2, pack_conv_up2_hilo(r2["w"], d), rows, IH, IW, pr2, bias=r2["bias"].to(d))
    whi, wlo = ep.expected_pair(r2["v"])
    ep.assert_bits_equal(pr2.hi.contiguous(), whi, lay)
    ep.assert_bits_equal(pr2.lo.contiguous(), wlo, lay)
    ep.record(r["name"], cls, "up2 + pair out + pair in", 5 * M * Cout, 0)


@pytest.mark.parametrize("cls", CLS2)
@pytest.mark.parametrize("case", ep.C4X4_CASES)
def test_conv4x4s2_is_the_exact_dgrad_of_upsample_conv(ops, case, cls):
    from sketch2img_amd.packs import pack_conv_up2_dgrad
    rows, IH, IW, Cin, Cout = case
    r = ep.c4x4_reference(*case, cls)
    M = rows * (IH // 2) * (IW // 2)
    out = torch.full((M, Cout + 8), ep.GUARD, device=dev(), dtype=torch.float16)
    xd, W16 = ep.nhwc(r["x"]).to(dev()), pack_conv_up2_dgrad(r["w"], dev())
    rc = ops.lib.skg_conv4x4s2_f16(xd.data_ptr(), Cin, W16.data_ptr(), out.data_ptr(), Cout + 8, rows, IH, IW, Cin, Cout, None, ops._stream())
    assert rc == 0, f"skg_conv4x4s2_f16: {rc}"
    ep.assert_bits_equal(out, ep.expected_f16(r["v"], cls), ep.Layout(rows, IH // 2, IW // 2, Cout, 64, None, f"{r['name']} / {cls}"))
    ep.record(r["name"], cls, "conv4x4s2", M * Cout, 0)


@pytest.mark.parametrize("cls", CLS2)
@pytest.mark.parametrize("case", ep.CONVT_CASES)
def test_convt4x4s2_exact(ops, case, cls):
    from sketch2img_amd import anime2sketch as a2s
    rows, IH, IW, Cin, Cout = case
    r = ep.convt_reference(*case, cls)
    M = rows * 4 * IH * IW
    out = torch.full((M, Cout), ep.GUARD, device=dev(), dtype=torch.float16)
    ops.convt4x4s2(ep.nhwc(r["x"]).to(dev()), a2s.pack_convt(r["w"], dev()), rows, IH, IW, out=out, bias=r["bias"].to(dev()))
    ep.assert_bits_equal(out, ep.expected_f16(r["v"], cls), ep.Layout(rows, 2 * IH, 2 * IW, Cout, 64, None, f"{r['name']} / {cls}"))
    ep.record(r["name"], cls, "convt4x4s2", M * Cout, 0)


@pytest.mark.parametrize("cls", CLS2)
@pytest.mark.parametrize("case", ep.SC_CASES)
def test_conv3x3_folded_shortcut_exact(ops, lib, case, cls):
    """skg_conv3x3_sc_f16 over all samples: fp16 output, pair output, and (gn cases, small class) the GroupNorm partial sums."""
    from sketch2img_amd.packs import pack_conv
    rows, IH, IW, Cin, Cout, K2, groups = case
    d = dev()
    M = rows * IH * IW
    r = ep.sc_reference(rows, IH, IW, Cin, Cout, K2, cls)
    ops._stream()
    var = lib.skg_gemm_variant(M, Cout, 9 * Cin + K2, Cin, 1)
    lay = ep.Layout(rows, IH, IW, Cout, ep.bn_of(var), None, f"{r['name']} / {cls}")
    xd, x2d, bias = ep.nhwc(r["x"]).to(d), r["x2"].to(d), r["bias"].to(d)
    wcat = torch.cat([pack_conv(r["w"], "cpu"), r["wsc"]], 1).contiguous().to(d)
    out = torch.full((M, Cout + 8), ep.GUARD, device=d, dtype=torch.float16)
    ops.conv3x3_sc(xd, x2d, wcat, rows, IH, IW, out=out[:, :Cout], bias=bias)
    ep.assert_bits_equal(out, ep.expected_f16(r["v"], cls), lay)
    pr = ops.Pair.empty(M, Cout, d)
    ops.conv3x3_sc(xd, x2d, wcat, rows, IH, IW, out=pr.hi, out_lo=pr.lo, bias=bias)
    whi, wlo = ep.expected_pair(r["v"])
    ep.assert_bits_equal(pr.hi.contiguous(), whi, lay)
    ep.assert_bits_equal(pr.lo.contiguous(), wlo, lay)
    extra = ""
    if groups and cls == "small":
        g = ep.sc_reference(rows, IH, IW, Cin, Cout, K2, "gn")
        wcat = torch.cat([pack_conv(g["w"], "cpu"), g["wsc"]], 1).contiguous().to(d)
        y, part = ops.conv3x3_sc(ep.nhwc(g["x"]).to(d), g["x2"].to(d), wcat, rows, IH, IW, bias=g["bias"].to(d), gn_groups=groups)
        want = g["v"].half()
        ep.assert_bits_equal(y, want, lay)
        sums = ep.gn_sums(want, rows, IH * IW, groups)
        nb = int((part.buf.view(rows, IH * IW // 128, groups, 2).double().cpu() != sums).sum())
        assert nb == 0, f"{g['name']}: {nb} of {sums.numel()} GroupNorm partial sums differ"
        extra = f" | {sums.numel()} partial sums exact"
    ep.record(r["name"], cls, var, 3 * M * Cout, 0, extra)


@pytest.mark.parametrize("cls", CLS2)
@pytest.mark.parametrize("case", ep.WINO_CASES)
def test_conv3x3_winograd_exact(ops, case, cls):
    """skg_conv3x3_wino_f16 with weights 4 * integers, both classes: bias + residual, ReLU, pair output with a pair residual, a bias row
    per sample, and the data gradient through the dgrad pack."""
    from sketch2img_amd.packs import pack_conv_wino
    rows, IH, IW, Cin, Cout = case
    d = dev()
    M = rows * IH * IW
    r = ep.wino_reference(*case, cls)
    name = r["name"]
    lay = ep.Layout(rows, IH, IW, Cout, 160 if Cout % 160 == 0 else 128 if Cout % 128 == 0 else 64, (16, Cin // 64), f"{name} / {cls}")
    xd, U = ep.nhwc(r["x"]).to(d), pack_conv_wino(r["w"], d)
    todev = lambda t: None if t is None else t.to(d)      # noqa: E731
    n = 0
    for epi in ("bias res", "relu", "pair pairres bias", "biasrows res"):
        words = epi.split()
        bias, res, res_lo, _ = ep.epi_operands(f"{name} [{epi}]", cls, words, M, Cout, rows)
        b = bias.repeat_interleave(IH * IW, dim=0) if bias is not None and bias.dim() == 2 else bias
        v = ep.epilogue(r["acc"], b, 1.0, res, "relu" in words, cls, res_lo)
        if "pair" in words:
            pr = ops.Pair.empty(M, Cout, d)
            ops.conv3x3_wino(xd, U, rows, IH, IW, out=pr.hi, out_lo=pr.lo, bias=todev(bias), residual=todev(res), residual_lo=todev(res_lo))
            whi, wlo = ep.expected_pair(v)
            ep.assert_bits_equal(pr.hi.contiguous(), whi, lay)
            ep.assert_bits_equal(pr.lo.contiguous(), wlo, lay)
        else:
            y = ops.conv3x3_wino(xd, U, rows, IH, IW, bias=todev(bias), residual=todev(res), relu="relu" in words)
            ep.assert_bits_equal(y, ep.expected_f16(v, cls), lay)
        n += M * Cout
    if Cout % 64 == 0:      # the data gradient (kernel Cin = Cout of the forward): a 3x3 convolution with the flipped, swapped pack
        g = ep.wino_reference(rows, IH, IW, Cin, Cout, cls, dgrad=True)
        y = ops.conv3x3_wino(ep.nhwc(g["x"]).to(d), pack_conv_wino(g["w"], d, dgrad=True), rows, IH, IW)
        ep.assert_bits_equal(y, ep.expected_f16(ep.epilogue(g["acc"], cls=cls), cls), lay)
        n += M * Cout
    ep.record(name, cls, "wino", n, 0)


@pytest.mark.parametrize("cls", CLS2)
@pytest.mark.parametrize("M,N,K", ep.WGRAD_CASES)
def test_wgrad_exact(ops, M, N, K, cls):
    """skg_wgrad_f16: '=' and then '+=', with and without db; dW and db in fp32, exact."""
    r = ep.wgrad_reference(M, N, K, cls)
    dy, x = r["dy"].to(dev()), r["x"].to(dev())
    layW, layb = ep.Layout.matrix(N, K, 64, None, r["name"] + " dW"), ep.Layout.matrix(1, N, 64, None, r["name"] + " db")
    dW = ops.wgrad(dy, x)
    ep.assert_bits_equal(dW, r["dW"].float(), layW)
    ops.wgrad(dy, x, dW=dW, accumulate=True)
    ep.assert_bits_equal(dW, (2 * r["dW"]).float(), layW)
    dW2, db = ops.wgrad(dy, x, want_db=True)
    ep.assert_bits_equal(dW2, r["dW"].float(), layW)
    ep.assert_bits_equal(db.view(1, N), r["db"].float().view(1, N), layb)
    ops.wgrad(dy, x, dW=dW2, db=db, accumulate=True)
    ep.assert_bits_equal(dW2, (2 * r["dW"]).float(), layW)
    ep.assert_bits_equal(db.view(1, N), (2 * r["db"]).float().view(1, N), layb)
    ep.record(r["name"], cls, "wgrad", 4 * N * K + 2 * N, 0)


# ------------------------------------------------------------------------------------------------------- edge sensitivity
@pytest.mark.parametrize("mode", ["S1", "UP2"])
def test_probes_see_the_halo(ops, mode):
    """The kernel output against a MUTANT reference with replicate padding: the mismatch set is non-empty on each of the four borders
    and lies inside the one-pixel border band - every interior pixel matches.  Shows on the device that the probes see halos."""
    case = ep.ConvCase(2, 6, 10, 64, 64, mode, "")
    x, w = ep.conv_operands(case, "small")
    OH, OW = ep.out_size(mode, 6, 10)
    good = ep.nhwc(ep.conv_ref(x.double(), w.double(), mode))
    mutant = ep.nhwc(ep.conv_ref(x.double(), w.double(), mode, pad_mode="replicate"))
    ep.check_fp16_exact(good)
    ep.check_fp16_exact(mutant)
    y = ops.conv3x3(ep.nhwc(x).to(dev()), ep.conv_pack(case, w, dev()), 2, 6, 10, ep.MODE_ID[mode]).cpu()
    ep.assert_bits_equal(y, good.half(), ep.Layout(2, OH, OW, 64, 64, None, case.name))
    diff = (y.double() != mutant).any(dim=1).view(2, OH, OW)
    assert not bool(diff[:, 1:-1, 1:-1].any()), "an interior pixel differs from the replicate-padding mutant"
    for nm, edge in (("top", diff[:, 0, :]), ("bottom", diff[:, -1, :]), ("left", diff[:, :, 0]), ("right", diff[:, :, -1])):
        assert bool(edge.any()), f"the {nm} border does not tell zero padding from replicate padding"
    ep.record(f"halo {mode}", "small", "edge", y.numel(), 0, f" | {int(diff.sum())} border pixels differ from the mutant")


# ------------------------------------------------------------------------------------------- forced tiles / stages / split depth
@pytest.mark.parametrize("what,env", [
    ("tiles", {"SKG_FORCE_BN": "320"}), ("tiles", {"SKG_FORCE_BN": "160"}), ("tiles", {"SKG_FORCE_BN": "128"}), ("tiles", {"SKG_FORCE_BN": "64"}),
    ("tiles", {"SKG_FORCE_BN": "320", "SKG_NO_NS3": "1"}), ("tiles", {"SKG_FORCE_BN": "160", "SKG_NO_NS3": "1"}),
    ("tiles", {"SKG_FORCE_BN": "128", "SKG_NO_NS3": "1"}), ("tiles", {"SKG_FORCE_BN": "64", "SKG_NO_NS3": "1"}),
    ("split", {"SKG_SPLIT_NS": "2"}), ("split", {"SKG_SPLIT_NS": "4"})], ids=lambda v: v if isinstance(v, str) else ",".join(f"{k}={x}" for k, x in v.items()))
def test_exact_probes_under_forced_tiles(what, env):
    """tests/_exact_tile_check.py in a process of its own (the library reads these switches once per process): the same bit-exact
    criterion with the tile width forced, without the three-stage ring, and with two / four stages on the split-K ring."""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "_exact_tile_check.py"), what], env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
