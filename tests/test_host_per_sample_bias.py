"""CPU tests (-m "not gpu") of the per-sample bias row (SKG_EPI_BIAS_ROWS): the argument checks of the C entry points answer before
any HIP call, ops refuses a bias of the wrong shape before the C call, and HipUNet.forward's timestep argument is validated on
the host.  Pointers are small aligned integers that are never dereferenced; no kernel is launched here."""
import pytest
import torch

BIAS_ROWS = 8


def conv(bias, flags=BIAS_ROWS, mode=0):
    from sketch2img_amd._lib import lib
    # X, ldx, Wp, Y, Y_lo, ldy, rows, IH, IW, Cin, Cout, mode, bias, residual, residual_lo, ldr, alpha, flags, gn_partial, groups, stream
    return lib.skg_conv3x3_f16(16, 64, 16, 16, None, 16, 3, 8, 8, 64, 16, mode, bias, None, None, 0, 1.0, flags, None, 0, None)


def wino(bias, flags=BIAS_ROWS, IH=8):
    from sketch2img_amd._lib import lib
    # X, ldx, U, V, Y, Y_lo, ldy, rows, IH, IW, Cin, Cout, bias, residual, residual_lo, ldr, flags, stream
    return lib.skg_conv3x3_wino_f16(16, 64, 16, 16, 16, None, 16, 3, IH, 8, 64, 16, bias, None, None, 0, flags, None)


def test_flag_value_is_public_and_free():
    """8 next to the public 1, 2, 4; the internal launcher bits start at 0x800."""
    import os
    import re
    from sketch2img_amd import ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "skg.h")).read()
    flags = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (SKG_EPI_\w+) (\d+)u", hdr)}
    assert flags["SKG_EPI_BIAS_ROWS"] == BIAS_ROWS == ops.EPI_BIAS_ROWS
    assert sorted(flags.values()) == [1, 2, 4, 8]


def test_flag_without_bias_is_a_bad_argument():
    assert conv(None) == -1
    assert wino(None) == -1


def test_flag_with_misaligned_bias_is_a_bad_argument():
    assert conv(20) == -1      # 4-byte aligned only
    assert wino(20) == -1


def test_gemm_refuses_the_flag():
    from sketch2img_amd._lib import lib
    # (with the fused GEGLU at K % 64 != 0 the same call without the flag is declined, -2, in front of any launch)
    gemm = lambda flags: lib.skg_gemm_f16(16, 32, 16, 32, 16, None, 16, 256, 16, 32, 16, None, None, 0, 1.0, flags, None, 0, 0, None)
    assert gemm(4) == -2
    assert gemm(4 | BIAS_ROWS) == -1
    assert gemm(BIAS_ROWS) == -1


def test_folded_shortcut_convolution_refuses_the_flag():
    """skg_conv3x3_sc_f16 is conv2 + conv_shortcut: the time bias belongs to conv1.  (Without the flag the same call - an X2 operand of
    2 GiB - is declined, -2, in front of any launch.)"""
    from sketch2img_amd._lib import lib
    sc = lambda flags: lib.skg_conv3x3_sc_f16(16, 320, 16, 1920, 1920, 16, 16, None, 320, 140, 64, 64, 320, 320, 16, flags, None, 0, None)
    assert sc(0) == -2 and sc(1) == -2
    assert sc(BIAS_ROWS) == -1 and sc(BIAS_ROWS | 1) == -1


def test_flag_with_unknown_mode_is_declined_not_refused():
    assert conv(16, mode=9) == -2
    assert conv(16, flags=0, mode=9) == -2


def test_wino_accepts_the_flag_and_still_declines_odd_maps():
    """The flag passes the flag check of skg_conv3x3_wino_f16 (it widened by this bit only): an odd map is declined (-2) behind
    it, any other unknown bit is refused (-1)."""
    assert wino(16, IH=7) == -2
    assert wino(16, flags=BIAS_ROWS | 1, IH=7) == -2
    assert wino(16, flags=BIAS_ROWS | 2, IH=7) == -1
    assert wino(16, flags=16, IH=7) == -1


def test_ops_refuse_a_bias_of_the_wrong_shape_before_the_c_call():
    from sketch2img_amd import ops
    rows, hw, cin, cout = 3, 8, 64, 16
    X = torch.zeros(rows * hw * hw, cin, dtype=torch.float16)
    Wp = torch.zeros(cout, 9 * cin, dtype=torch.float16)
    U = torch.zeros(cout, 16 * cin, dtype=torch.float16)
    z = lambda *shape: torch.zeros(*shape, dtype=torch.float16)
    for bad in (z(rows + 1, cout), z(rows, cout + 8), z(rows, 2 * cout)[:, :cout], z(1, rows, cout)):      # (the third: right shape, not contiguous)
        with pytest.raises(ValueError):
            ops.conv3x3(X, Wp, rows, hw, hw, bias=bad)
        with pytest.raises(ValueError):
            ops.conv3x3_wino(X, U, rows, hw, hw, bias=bad)
    assert ops._bias_rows_flag(torch.zeros(rows, cout).half(), rows, cout) == BIAS_ROWS
    assert ops._bias_rows_flag(torch.zeros(cout).half(), rows, cout) == 0 and ops._bias_rows_flag(None, rows, cout) == 0


def test_forward_timestep_argument():
    """What HipUNet.forward makes of `t` (unet.per_sample_timesteps, the first thing it calls): ints and equal entries take the
    int path, distinct entries the per-sample one; a wrong length and shared_input over unequal halves raise ValueError."""
    from sketch2img_amd.unet import per_sample_timesteps as f
    assert f(801, 3) == 801 and f(torch.tensor(801), 3) == 801
    assert f([5, 5, 5], 3) == 5 and f(torch.tensor([5, 5]), 2) == 5 and f((7,), 1) == 7
    assert f([801, 133, 37], 3) == [801, 133, 37]
    assert f(torch.tensor([801, 133, 37]), 3) == [801, 133, 37]
    assert f([801, 133, 801, 133], 4, shared_input=True) == [801, 133, 801, 133]
    for bad in ([801, 133], torch.tensor([801, 133, 37, 5]), []):
        with pytest.raises(ValueError):
            f(bad, 3)
    with pytest.raises(ValueError):
        f([801, 133, 133, 801], 4, shared_input=True)
    with pytest.raises(ValueError):
        f([801, 133, 37], 3, shared_input=True)
    with pytest.raises(ValueError):
        f(torch.tensor([[801, 133, 37]]), 3)
    with pytest.raises(ValueError):
        f(torch.tensor([801.0, 133.0, 37.0]), 3)
