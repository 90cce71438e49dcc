"""CPU tests (-m "not gpu") of the two places that hold a fact the rest reads: unet.Stash.suffix, which narrows every stashed tensor to
the differentiated rows, and flat_adamw.FlatAdamW.stale, which tells a trainer that its derived packs are out of date."""
import pytest
import torch

from sketch2img_amd import flat_adamw, loss_scaler, ops
from sketch2img_amd.unet import Stash


def _t(rows, cols=3):
    return torch.arange(rows * cols, dtype=torch.float32).reshape(rows, cols)


# ---------------------------------------------------------------------------------------------- Stash.suffix
def test_whole_tensor_is_narrowed_to_a_view_of_the_last_rows():
    st, v = Stash(rows=4, first=2), _t(16)
    out = st.suffix("x", v, 4)
    assert out.shape == (8, 3) and torch.equal(out, v[8:])
    assert out.data_ptr() == v[8].data_ptr() and out.untyped_storage().data_ptr() == v.untyped_storage().data_ptr()
    assert out.is_contiguous()


def test_a_tensor_of_exactly_the_differentiated_rows_comes_back_unchanged():
    st = Stash(rows=4, first=2)
    v = _t(8)                                     # what a stashing launch with keep_from = 2 * 4 returns
    out = st.suffix("f", v, 4)
    assert out.data_ptr() == v.data_ptr() and out.shape == v.shape and torch.equal(out, v)
    assert st.suffix("f", out, 4).data_ptr() == v.data_ptr()      # (narrowing what is narrow already changes nothing)


def test_cond_half_of_a_shared_front():
    """rows = 2 with the default first = rows // 2: the shared front's tensors hold the cond row only, the others both rows."""
    st, HW = Stash(rows=2, first=1), 4
    half, full = _t(HW), _t(2 * HW)
    assert st.suffix("x", half, HW).data_ptr() == half.data_ptr() and st.suffix("x", half, HW).shape == (HW, 3)
    assert torch.equal(st.suffix("p2", full, HW), full[HW:])
    # rows = 6 (three samples, CFG-doubled): the cond half is rows 3 ... 5
    st = Stash(rows=6, first=3)
    assert torch.equal(st.suffix("x", _t(3 * HW), HW), _t(3 * HW)) and torch.equal(st.suffix("x", _t(6 * HW), HW), _t(6 * HW)[3 * HW:])


def test_per_image_tensors_take_unit_one():
    st = Stash(rows=4, first=2)
    gst, lse = _t(4, 2), torch.arange(2 * 5 * 7, dtype=torch.float32).reshape(2, 5, 7)
    assert torch.equal(st.suffix("gst", gst, 1), gst[2:]) and st.suffix("gst", gst, 1).shape == (2, 2)
    out = st.suffix("lse2", lse, 1)
    assert out.data_ptr() == lse.data_ptr() and out.shape == (2, 5, 7)


@pytest.mark.parametrize("first,S", [(1, 2), (0, 3)])
def test_odd_row_counts_and_first_zero(first, S):
    st, HW = Stash(rows=3, first=first), 4
    v = _t(3 * HW)
    out = st.suffix("x", v, HW)
    assert out.shape[0] == S * HW and torch.equal(out, v[first * HW:])
    kept = _t(S * HW)
    assert st.suffix("q2", kept, HW).data_ptr() == kept.data_ptr()
    assert torch.equal(st.suffix("st1", _t(3), 1), _t(3)[first:])
    if first == 0:
        assert out.data_ptr() == v.data_ptr()


def test_a_suffix_longer_than_the_differentiated_rows_is_cut_from_the_front():
    st = Stash(rows=4, first=3)                   # one differentiated row; a tensor that holds the last two
    v = _t(8)
    assert torch.equal(st.suffix("x", v, 4), v[4:])


def test_none_passes_through():
    assert Stash(rows=4, first=2).suffix("st2", None, 4) is None


@pytest.mark.parametrize("n,unit,why", [(10, 4, "no multiple of the unit"), (4, 4, "fewer rows than differentiated"),
                                        (20, 4, "more rows than the evaluation"), (1, 1, "per image: too few"),
                                        (5, 1, "per image: too many")])
def test_raises_with_the_key_in_the_message(n, unit, why):
    st = Stash(rows=4, first=2)
    with pytest.raises(ValueError, match=r"down_blocks\.0\.attentions\.0\.q2"):
        st.suffix("down_blocks.0.attentions.0.q2", _t(n), unit)


# ---------------------------------------------------------------------------------------------- FlatAdamW.stale
SHAPES = [("a.weight", (3, 5)), ("a.bias", (3,))]


def _opt():
    g = torch.Generator().manual_seed(5)
    sd = {k: torch.randn(shp, generator=g) for k, shp in SHAPES}
    return flat_adamw.FlatAdamW(SHAPES, sd, "cpu", lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2,
                                schedule=lambda s: 0.5 ** s, grad_scale=64.0)


def test_stale_is_set_by_a_static_step_that_ran_and_not_by_a_skipped_one(monkeypatch):
    calls = []
    monkeypatch.setattr(ops, "adamw_step", lambda *a: calls.append(a))
    st = _opt()
    assert st.stale is False
    g = st.new_grad()
    g[3] = float("nan")
    assert st.step(g) is False and st.stale is False and not calls          # skipped: the packs are still those of p16
    g[3] = 0.0
    assert st.step(g) is True and st.stale is True and len(calls) == 1
    st.stale = False                                                        # (the trainer clears it before it refreshes)
    assert st.step(g, checked=True) is True and st.stale is True


def test_stale_under_a_scaler_is_set_by_settle_true_only(monkeypatch):
    monkeypatch.setattr(ops, "adamw_step_guarded", lambda *a: None)
    monkeypatch.setattr(ops, "nonfinite_flag", lambda x, flag, reset=False: (flag.zero_() if reset else None,
                                                                           flag.fill_(1.0) if not torch.isfinite(x).all() else None))
    st = _opt()
    st.settle(False)
    assert st.stale is False and st.step_count == 0
    st.settle(True)
    assert st.stale is True and st.step_count == 1
    # the same through a scaler: the guarded step itself marks nothing, the verdict does
    st.stale = False
    sc = loss_scaler.DynamicLossScaler("cpu", init_scale=2.0 ** 10)
    g = st.new_grad()
    g[1] = float("inf")
    v = sc.check(g)
    st.step(g, scaler=sc, scale=sc._scale)
    assert st.stale is False
    assert bool(v) is False and st.stale is False and st.step_count == 1
    g[1] = 0.0
    v = sc.check(g)
    st.step(g, scaler=sc, scale=sc._scale)
    assert st.stale is False
    assert bool(v) is True and st.stale is True and st.step_count == 2
