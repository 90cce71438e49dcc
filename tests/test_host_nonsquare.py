"""Host-side checks of the non-square path (no GPU): the rectangular LGP entry points reject bad arguments before any HIP
call, and the pipeline's image-size rule."""
import ctypes

import pytest

E_BADARG = -1
P = 4096          # a 16-byte aligned host address: never dereferenced, every call below fails its argument checks first


def _taps(*sides):
    from sketch2img_amd._lib import SkgTap
    arr = (SkgTap * len(sides))()
    for i, s in enumerate(sides):
        arr[i].P, arr[i].s = P, s
    return arr


def _gather(arr, h, w, Z=P, Wextra=None, H0=128):
    from sketch2img_amd._lib import lib
    return lib.skg_lgp_layer0_gather(ctypes.addressof(arr), len(arr), Wextra, 0, P, P, 1.0, 1, Z, 2, h, w, H0, None)


def test_rectangular_lgp_entry_points_are_exported():
    from sketch2img_amd import _lib
    for name in ("skg_lgp_layer0_gather", "skg_lgp_layer0_scatter", "skg_lgp_mse_seed", "skg_lgp_extra_features"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)


def test_rectangular_lgp_entry_points_reject_bad_arguments_without_a_gpu():
    from sketch2img_amd._lib import lib
    # gather: sides not multiples of 8, a tap whose width (s * w / h) is not whole, a tap that does not divide h, null output
    assert _gather(_taps(8), 12, 16) == E_BADARG
    assert _gather(_taps(8), 16, 20) == E_BADARG
    assert _gather(_taps(8), 24, 16) == E_BADARG          # tap width 8 * 16 / 24
    assert _gather(_taps(16, 7), 16, 24) == E_BADARG       # 7 does not divide 16
    assert _gather(_taps(8), 16, 24, Z=None) == E_BADARG
    assert _gather(_taps(8), 0, 24) == E_BADARG
    # scatter
    assert lib.skg_lgp_layer0_scatter(P, 128, P, 2, 16, 20, 8, 128, None) == E_BADARG
    assert lib.skg_lgp_layer0_scatter(P, 128, P, 2, 24, 16, 8, 128, None) == E_BADARG
    assert lib.skg_lgp_layer0_scatter(None, 128, P, 2, 16, 24, 8, 128, None) == E_BADARG
    assert lib.skg_lgp_layer0_scatter(P, 128, None, 2, 16, 24, 8, 128, None) == E_BADARG
    # MSE seed
    assert lib.skg_lgp_mse_seed(P, 8, P, P, 32, P, 1, 16, 12, 1.0, None) == E_BADARG
    assert lib.skg_lgp_mse_seed(None, 8, P, P, 32, P, 1, 16, 24, 1.0, None) == E_BADARG
    assert lib.skg_lgp_mse_seed(P, 8, None, P, 32, P, 1, 16, 24, 1.0, None) == E_BADARG
    # extra features
    assert lib.skg_lgp_extra_features(P, 1.0, 1, 2, 20, 16, P, 64, None) == E_BADARG
    assert lib.skg_lgp_extra_features(None, 1.0, 1, 2, 16, 24, P, 64, None) == E_BADARG
    assert lib.skg_lgp_extra_features(P, 1.0, 1, 2, 16, 24, None, 64, None) == E_BADARG


def test_image_size_rule():
    from sketch2img_amd.modules.pipeline import check_image_size
    for hw in ((768, 512), (512, 768), (64, 1024), (1024, 64), (512, 512), (576, 320), (320, 192), (640, 384)):
        check_image_size(*hw)
    for hw in ((520, 512), (512, 520), (1088, 512), (768, 576 + 8), (1024, 1088)):
        with pytest.raises(NotImplementedError):
            check_image_size(*hw)
    for hw in ((250, 256), (256, 250)):
        with pytest.raises(ValueError):
            check_image_size(*hw)
