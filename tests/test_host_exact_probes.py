"""Host side of the exact-integer probes (tests/exact_probes.py): the conditions that make the expected bits unambiguous hold for every
(case, seed) of tests/test_gpu_exact_contractions.py, the weight packs of integer weights are integer packs, the transformed /
pre-summed forms reproduce the plain convolution bit for bit, and the comparator sees what the relative Frobenius criterion
(rel < 6e-4) cannot."""
import pytest
import torch
import torch.nn.functional as F

from tests import exact_probes as ep
from tests.util import rel_err

FP16_RND = 6e-4      # the criterion of tests/test_gpu_kernels.py


def test_draw_int_is_fixed_per_seed_and_in_range():
    a, b = ep.draw_int((64, 33), 31, 5), ep.draw_int((64, 33), 31, 5)
    assert torch.equal(a, b) and a.dtype == torch.float16 and float(a.abs().max()) == 31 and torch.equal(a, a.round())
    s = ep.draw_int((4096,), 1, 7, density=0.125, step=4)
    assert set(s.unique().tolist()) == {-4.0, 0.0, 4.0} and 0.05 < float((s != 0).float().mean()) < 0.12
    assert ep.large_amp_w(576) == 15 and ep.large_amp_w(1152) == 7 and ep.large_amp_w(23040) == 1


def test_conditions_hold_for_every_case_and_seed():
    """Order-free exactness, fp16 representability (small), finite rounding (large), exact GroupNorm sums - on the references alone;
    the largest cases by their worst-case bound and a reduced draw (they are asserted in full before each device comparison)."""
    names = list(ep.host_check_all())
    assert len(names) >= sum(len(c.classes) for c in ep.GEMM_CASES + ep.CONV_CASES)
    # up to K = 23040 (the deepest convolution of the UNet) at the class amplitudes
    ep.check_worst_case(23040, 31, ep.large_amp_w(23040), 8 + 4096)
    ep.check_worst_case(23040, 3, 1, 8 + 64)


def test_conditions_reject_what_they_must():
    with pytest.raises(AssertionError):
        ep.check_worst_case(23040, 31, 31)
    with pytest.raises(AssertionError):
        ep.check_fp16_exact(torch.tensor([2049.0], dtype=torch.float64))
    with pytest.raises(AssertionError):
        ep.check_fp16_range(torch.tensor([65520.0], dtype=torch.float64))
    with pytest.raises(AssertionError):
        ep.rne_fp16(torch.tensor([float(2 ** 24 + 1)], dtype=torch.float64))
    with pytest.raises(AssertionError):
        ep.check_order_free(torch.full((1, 4096), 64.0), torch.full((1, 4096), 64.0))


def _is_int_pack(p, bound):
    p = p.float()
    return bool(torch.equal(p, p.round())) and float(p.abs().max()) <= bound <= 2048


def test_packs_of_integer_weights_are_integer_packs():
    from sketch2img_amd import anime2sketch as a2s
    from sketch2img_amd.packs import pack_conv_dgrad, pack_conv_up2, pack_conv_up2_dgrad, pack_conv_wino
    for a in (1, 7, 15):
        w = ep.draw_int((40, 64, 3, 3), a, 11 + a)
        assert _is_int_pack(pack_conv_wino(ep.draw_int((40, 64, 3, 3), a, 3, step=4), "cpu"), 9 * a)
        assert _is_int_pack(pack_conv_wino(ep.draw_int((40, 64, 3, 3), a, 3, step=4), "cpu", dgrad=True), 9 * a)
        assert _is_int_pack(pack_conv_up2(w, "cpu"), 4 * a) and _is_int_pack(pack_conv_up2_dgrad(w, "cpu"), 4 * a)
        assert _is_int_pack(pack_conv_dgrad(w, "cpu"), a)
        w4 = ep.draw_int((64, 40, 4, 4), a, 13 + a)
        assert _is_int_pack(a2s.pack_convt(w4, "cpu"), a) and _is_int_pack(a2s.pack_conv_down(w4, "cpu"), a)
    # a weight that is NOT a multiple of 4 gives a fractional Winograd pack: the step is what makes it integer
    assert not _is_int_pack(pack_conv_wino(ep.draw_int((8, 64, 3, 3), 1, 3), "cpu"), 9)


@pytest.mark.parametrize("cls", ["small", "large"])
@pytest.mark.parametrize("case", ep.WINO_CASES[:3] + ((1, 6, 10, 256, 72),))
def test_winograd_emulation_equals_the_fp64_convolution(case, cls):
    """fp32 emulation of the whole pipeline, fp16(V) and fp16(U) included, against the fp64 convolution: bit for bit."""
    from sketch2img_amd.packs import pack_conv_wino
    for dgrad in (False, True):
        r = ep.wino_reference(*case, cls, dgrad=dgrad)
        y = ep.wino_emulate(r["x"], pack_conv_wino(r["w"], "cpu", dgrad=dgrad))
        assert torch.equal(ep.nhwc(y).double(), r["acc"].double())


def _polyphase(x, Wpp):
    """fp64 emulation of the four 4-tap stride-1 convolutions of skg_conv3x3_up2_f16 / skg_convt4x4s2_f16 over the low-res input:
    phase (a, b) reads rows {i - 1, i} (a = 0) or {i, i + 1} (a = 1), the same for columns; taps row-major over the 2 x 2."""
    Bn, Ci, H, W = x.shape
    Co = Wpp.shape[1]
    xp = F.pad(x, (1, 1, 1, 1))
    out = torch.zeros(Bn, Co, 2 * H, 2 * W, dtype=x.dtype)
    for a in (0, 1):
        for b in (0, 1):
            Wt = Wpp[2 * a + b].to(x.dtype).view(Co, 4, Ci)
            for t, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
                patch = xp[:, :, a + dy:a + dy + H, b + dx:b + dx + W]
                out[:, :, a::2, b::2] += torch.einsum("bchw,oc->bohw", patch, Wt[:, t])
    return out


@pytest.mark.parametrize("cls", ["small", "large"])
def test_presummed_and_transposed_packs_reproduce_the_references(cls):
    """The polyphase pack (pre-summed taps), its data-gradient pack and the transposed-convolution pack, applied in fp64 the way the
    kernels walk them, equal the plain torch references bit for bit: nothing rounds on the way through a pack."""
    from sketch2img_amd import anime2sketch as a2s
    from sketch2img_amd.packs import pack_conv_up2, pack_conv_up2_dgrad
    r = ep.up2_reference(*ep.UP2_CASES[0], cls)
    rows, IH, IW, Cin, Cout = ep.UP2_CASES[0]
    acc = ep.nhwc(_polyphase(r["x"].double(), pack_conv_up2(r["w"], "cpu"))) + r["bias"].double()
    assert torch.equal(acc, r["v"])
    r = ep.c4x4_reference(*ep.C4X4_CASES[0], cls)
    rows, IH, IW, Cin, Cout = ep.C4X4_CASES[0]
    W16 = pack_conv_up2_dgrad(r["w"], "cpu").double().view(Cout, 4, 4, Cin).permute(0, 3, 1, 2)
    assert torch.equal(ep.nhwc(F.conv2d(r["x"].double(), W16, stride=2, padding=1)), r["v"])
    r = ep.convt_reference(*ep.CONVT_CASES[0], cls)
    acc = ep.nhwc(_polyphase(r["x"].double(), a2s.pack_convt(r["w"], "cpu"))) + r["bias"].double()
    assert torch.equal(acc, r["v"])


def test_comparator_reports_location_guards_and_split_structure():
    want = ep.draw_int((300, 72), 64, 1)
    got = torch.full((300, 88), ep.GUARD, dtype=torch.float16)
    got[:, :72] = want
    lay = ep.Layout(3, 10, 10, 72, 64, (4, 9), "probe")
    ep.assert_bits_equal(got, want, lay)
    neg0 = want.clone()
    neg0[want == 0] = -0.0
    ep.assert_bits_equal(neg0, want, lay)                  # the sign of a zero is not a finding
    bad = got.clone()
    bad[257, 70] += 1                                      # sample 2, pixel 57 = (5, 7), channel 70: tile (2, 1)
    with pytest.raises(AssertionError) as e:
        ep.assert_bits_equal(bad, want, lay)
    msg = str(e.value)
    assert "1 of 21600 elements differ" in msg and "(s=2, y=5, x=7, c=70)" in msg and "tile (row 2, col 1)" in msg
    assert "4 K slices of 9 x 64" in msg
    bad = got.clone()
    bad[12, 80] = 0                                        # a guard column
    with pytest.raises(AssertionError) as e:
        ep.assert_bits_equal(bad, want, lay)
    assert "guard elements overwritten" in str(e.value) and "row 12, column 80" in str(e.value)
    nan = got.clone()
    nan[0, 0] = float("nan")
    with pytest.raises(AssertionError):
        ep.assert_bits_equal(nan, want, lay)


# ---- the comparator sees what the Frobenius criterion cannot: mutants of the reference at the 64 x 64-level shape -------------
ROWS, H = ep.BIG_CONV[0]
HW = H * H


def _raises(got, want, lay):
    with pytest.raises(AssertionError) as e:
        ep.assert_bits_equal(got, want, lay)
    return str(e.value)


def test_mutants_the_frobenius_criterion_is_blind_to_small_class():
    x, w, acc = ep.big_conv_ref(ROWS, H, "small")
    Cout, Cin = ep.BIG_COUT, ep.BIG_CIN
    bias = ep.draw_int((ROWS, Cout), 8, 99)
    v = ep.epilogue(acc, bias.repeat_interleave(HW, dim=0))
    want = ep.expected_f16(v, "small")
    lay = ep.Layout(ROWS, H, H, Cout, 64, None, "mutant")
    assert want.numel() > 18e6
    # (a) one missing tap (ky, kx) = (0, 2) at pixel (s, y, x) = (5, 17, 40), in one lane's 8-channel store (channels 16..23): the output
    # there lacks x[s, :, y - 1, x + 1] . w[c, :, 0, 2].  (Over all 320 channels of the pixel the same mutant is 1.4e-3 at this shape.)
    s, y, xx, c0 = 5, 17, 40, 16
    m = (s * H + y) * H + xx
    tap = w[c0:c0 + 8, :, 0, 2].float() @ x[s, :, y - 1, xx + 1].float()
    assert bool((tap != 0).any())
    mut = want.clone()
    mut[m, c0:c0 + 8] = (v[m, c0:c0 + 8] - tap).half()
    assert rel_err(mut, want) < FP16_RND
    msg = _raises(mut, want, lay)
    assert f"(s={s}, y={y}, x={xx}, c={c0 + int((tap != 0).nonzero()[0])})" in msg and f"tile (row {m // 128}, col 0)" in msg
    assert f"{int((tap != 0).sum())} of " in msg
    # (b) the last 64-deep K tile (tap (2, 2), channels 64..127) dropped for the 128 x 64 tile (row 301, col 3)
    ti, tj = 301, 3
    xp = F.pad(x.float(), (1, 1, 1, 1))[:, 64:, 2:, 2:]                       # the (2, 2) tap's pixel for every output pixel
    a_tile = ep.nhwc(xp)[128 * ti:128 * ti + 128]                             # [128, 64]
    part = a_tile @ w[64 * tj:64 * tj + 64, 64:, 2, 2].float().t()
    mut = want.clone()
    mut[128 * ti:128 * ti + 128, 64 * tj:64 * tj + 64] = (v[128 * ti:128 * ti + 128, 64 * tj:64 * tj + 64] - part).half()
    # (a whole tile without 1 / 18 of its K is sqrt(8192 / 18 / 18.35 M) = 5.0e-3 of the norm: this one the Frobenius criterion does
    # see at this shape; it stays blind to it from one 8-channel store down - the comparator names the tile either way)
    r_b = rel_err(mut, want)
    print(f"mutant (b): rel {r_b:.2e}")
    assert 4e-3 < r_b < 6e-3
    mut8 = want.clone()
    mut8[128 * ti + 77, 64 * tj + 8:64 * tj + 16] = mut[128 * ti + 77, 64 * tj + 8:64 * tj + 16]
    assert rel_err(mut8, want) < FP16_RND
    assert f"tile (row {ti}, col {tj})" in _raises(mut8, want, lay)
    msg = _raises(mut, want, lay)
    assert f"in 1 tile(s) of 128 x 64, first [({ti}, {tj})]" in msg
    # (c) the bias row of sample s + 1 on the last pixel of sample s
    s = 8
    m = (s + 1) * HW - 1
    mut = want.clone()
    mut[m] = (acc[m] + bias[s + 1].float()).half()
    assert rel_err(mut, want) < FP16_RND
    msg = _raises(mut, want, lay)
    assert f"(s={s}, y={H - 1}, x={H - 1}, c=" in msg and f"tile (row {m // 128}," in msg


def test_mutant_rounded_before_the_residual_large_class():
    """fp16(fp16(acc + bias) + residual) instead of fp16(acc + bias + residual): about 2.9e-4 in the Frobenius norm - 'one rounding'
    to the old criterion - and a third of all elements to the comparator."""
    x, w, acc = ep.big_conv_ref(ROWS, H, "large")
    Cout = ep.BIG_COUT
    bias = ep.draw_int((Cout,), 8, 98)
    res = ep.draw_int((ROWS * HW, Cout), 2048, 97, step=2)
    v = ep.epilogue(acc, bias, 1.0, res, cls="large")
    want = ep.expected_f16(v, "large")
    mut = ((acc + bias.float()).half().float() + res.float()).half()
    assert rel_err(mut, want) < FP16_RND
    msg = _raises(mut, want, ep.Layout(ROWS, H, H, Cout, 64, None, "mutant"))
    n = int(msg.split(" of ")[0].split()[-1])
    assert n > 0.1 * want.numel()
    # and the pair output of the same value: the lo half is exact and non-zero on about a third of the elements
    hi, lo = ep.expected_pair(v)
    assert torch.equal(hi, want) and torch.equal(hi.double() + lo.double(), v.double())
    assert 0.2 < float((lo != 0).float().mean()) < 0.6
