"""CPU tests (-m "not gpu") of flat_adamw.FlatAdamW on its own: a toy key list, no trainer and no kernel."""
import torch

from sketch2img_amd import flat_adamw, ops

# no element count is a multiple of 8; "frozen" is listed in the middle and must be laid out last
SHAPES = [("a.weight", (3, 5)), ("frozen", (7,)), ("a.bias", (3,)), ("b.weight", (2, 3, 3)), ("b.bias", (1,))]
ORDER = ["a.weight", "a.bias", "b.weight", "b.bias", "frozen"]


def _state(**kw):
    g = torch.Generator().manual_seed(5)
    sd = {k: torch.randn(shp, generator=g) for k, shp in SHAPES}
    args = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, schedule=lambda s: 0.5 ** s, grad_scale=64.0,
                frozen={"frozen"})
    args.update(kw)
    return sd, flat_adamw.FlatAdamW(SHAPES, sd, "cpu", **args)


def test_spans_are_disjoint_aligned_and_frozen_keys_come_last():
    sd, st = _state()
    assert list(st.layout) == ORDER
    end = 0
    for k, (off, shp) in st.layout.items():
        assert off >= end and off % 8 == 0 and shp == sd[k].shape, k
        end = off + shp.numel()
        assert (off >= st.n_opt) == (k == "frozen"), k
        assert torch.equal(st.p[off:end].view(shp), sd[k]) and torch.equal(st.w16(k), sd[k].half()), k
    assert st.n_opt == st.layout["frozen"][0] == 16 + 8 + 24 + 8 and st.n == st.n_opt + 8 >= end
    assert st.p.dtype == st.m.dtype == st.v.dtype == torch.float32 and st.p16.dtype == torch.float16
    assert st.p.shape == st.p16.shape == st.m.shape == st.v.shape == (st.n,)
    assert not st.m.any() and not st.v.any() and st.step_count == 0
    _, plain = _state(frozen=())                                  # nothing frozen: the given order, AdamW on everything
    assert list(plain.layout) == [k for k, _ in SHAPES] and plain.n_opt == plain.n
    bad = dict(sd, **{"a.bias": torch.zeros(4)})
    try:
        flat_adamw.FlatAdamW(SHAPES, bad, "cpu", 1e-3, (0.9, 0.999), 1e-8, 1e-2, lambda s: 1.0, 1.0)
    except AssertionError as e:
        assert "a.bias" in str(e)
    else:
        raise AssertionError("a shape that differs from the state dict's must be refused")


def test_views_alias_the_vectors():
    _, st = _state()
    g = st.new_grad()
    assert g.shape == (st.n,) and g.dtype == torch.float32 and not g.any()
    for i, (k, (off, shp)) in enumerate(st.layout.items()):
        st.w16(k).fill_(i + 1)
        st.w32(k).fill_(-(i + 1))
        st.grad_view(g, k).fill_(10 * (i + 1))
        n = shp.numel()
        assert st.w16(k).shape == st.w32(k).shape == st.grad_view(g, k).shape == shp
        assert (st.p16[off:off + n] == i + 1).all() and (st.p[off:off + n] == -(i + 1)).all() and (g[off:off + n] == 10 * (i + 1)).all()
    pad = torch.ones(st.n, dtype=torch.bool)
    for off, shp in st.layout.values():
        pad[off:off + shp.numel()] = False
    assert not g[pad].any()                                       # the alignment gaps belong to no view


def test_state_dict_returns_clones_in_the_requested_order():
    sd, st = _state()
    out = st.state_dict()
    assert list(out) == ORDER and all(torch.equal(out[k], sd[k]) and out[k].dtype == torch.float32 for k in sd)
    want = ["frozen", "b.bias", "a.weight"]
    out = st.state_dict(want)
    assert list(out) == want
    out["frozen"].zero_()
    assert torch.equal(st.w32("frozen"), sd["frozen"])            # a clone, not a view


def test_step_refuses_a_non_finite_gradient_and_checked_skips_the_test(monkeypatch):
    _, st = _state()
    calls = []
    monkeypatch.setattr(ops, "adamw_step", lambda *a: calls.append(a))
    g = st.new_grad()
    g[3] = float("inf")
    before = [t.clone() for t in (st.p, st.m, st.v, st.p16)]
    assert st.step(g) is False and not calls and st.step_count == 0
    assert all(torch.equal(a, b) for a, b in zip(before, (st.p, st.m, st.v, st.p16)))
    # checked=True: no finiteness test - the same gradient goes to the kernel
    st.step_count = 2
    assert st.current_lr() == 1e-3 * 0.25
    assert st.step(g, checked=True) is True and st.step_count == 3 and len(calls) == 1
    p, gr, m, v, p16, lr, b1, b2, eps, wd, step, inv = calls[0]
    n = st.n_opt                                                  # AdamW on [0, n_opt): views of the vectors' fronts
    for got, vec in ((p, st.p), (gr, g), (m, st.m), (v, st.v), (p16, st.p16)):
        assert got.data_ptr() == vec.data_ptr() and got.numel() == n
    assert (lr, b1, b2, eps, wd, step, inv) == (1e-3 * 0.25, 0.9, 0.999, 1e-8, 1e-2, 3, 1.0 / 64.0)
    g[3] = 0.0
    assert st.step(g) is True and len(calls) == 2 and st.step_count == 4


def test_schedules():
    assert [flat_adamw.constant_with_warmup(s, 4) for s in (0, 1, 4, 9)] == [0.0, 0.25, 1.0, 1.0]
    assert flat_adamw.constant_with_warmup(0, 0) == 1.0
    assert flat_adamw.cosine_with_restarts(0, 150, 1150) == 0.0 and flat_adamw.cosine_with_restarts(150, 150, 1150) == 1.0
    assert flat_adamw.cosine_with_restarts(650, 150, 1150, 2) == 1.0 and flat_adamw.cosine_with_restarts(1150, 150, 1150) == 0.0
