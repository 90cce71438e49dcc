"""CPU tests (-m "not gpu") of the 8-bit AdamW state: the two quantisation maps and their thresholds against the numpy checker
(tests/adamw8bit_ref.py), the checker's round-trip bound, the block-table builder on the mixed layout, the C entry point's declaration
and argument checks, the optimizer state dicts of both modes, and that state_bits = 32 is the optimizer it was."""
import os
import re

import numpy as np
import pytest
import torch

from sketch2img_amd import _lib, flat_adamw, ops
from tests import adamw8bit_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUMEL = {k: int(np.prod(s)) for k, s in ref.MIXED}


def _opt(bits, dev="cpu", **kw):
    g = torch.Generator().manual_seed(3)
    sd = {k: torch.randn(shp, generator=g) for k, shp in ref.MIXED}
    args = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, schedule=lambda s: 1.0, grad_scale=8.0,
                frozen={"frozen"}, state_bits=bits)
    args.update(kw)
    return flat_adamw.FlatAdamW(ref.MIXED, sd, dev, **args)


def test_maps_are_the_definitions_and_the_checkers():
    q1, q2 = (q.numpy() for q in flat_adamw.quant_maps())
    r1, r2 = ref.maps()
    assert q1.dtype == q2.dtype == np.float32 and np.array_equal(q1, r1) and np.array_equal(q2, r2)
    for q in (q1, q2):
        assert q.shape == (256,) and np.all(np.diff(q) > 0)                      # sorted, distinct
    assert q1[0] == np.float32(-0.99296874) and q1[1] == np.float32(-0.9789063) and q1[255] == 1.0
    assert q1[127] == 0.0 and q1[126] == np.float32(-5.5e-7) and q1[128] == np.float32(5.5e-7)
    assert q2[0] == 0.0 and q2[1] == np.float32(3.25e-7) and q2[2] == np.float32(7.75e-7)
    assert q2[254] == np.float32(0.9964844) and q2[255] == 1.0
    assert np.array_equal(q1[:127], -q1[128:255][::-1])                          # the signed map is symmetric below 1
    for i in range(7):                                                            # per-decade counts: [10^(i-7), 10^(i-6))
        lo, hi = 10.0 ** (i - 7), 10.0 ** (i - 6)
        assert int(((q1 > lo) & (q1 < hi)).sum()) == int(((q1 < -lo) & (q1 > -hi)).sum()) == 2 ** i
        assert int(((q2 > lo) & (q2 < hi)).sum()) == 2 ** (i + 1)
    tab = flat_adamw.quant_table(*flat_adamw.quant_maps()).numpy().reshape(4, 256)
    assert np.array_equal(tab[0], r1) and np.array_equal(tab[2], r2)
    assert np.array_equal(tab[1, :255], ref.thresholds(r1)) and np.array_equal(tab[3, :255], ref.thresholds(r2))
    assert np.all(np.diff(tab[1, :255]) > 0) and np.all(np.diff(tab[3, :255]) > 0)
    # the zero codes: 0 quantises to 127 (signed) and 0 (unsigned) under a non-zero absmax too
    assert int((ref.thresholds(r1) < 0).sum()) == ref.ZERO1 == 127 and int((ref.thresholds(r2) < 0).sum()) == ref.ZERO2 == 0


def test_checker_round_trip_stays_within_half_the_top_decades_spacing():
    """|deq(quant(x)) - x| <= 0.9/128 absmax for the signed map (half of 0.9/64, the widest cell spacing), and likewise 0.9/256 for the
    unsigned one; every map value is a fixed point; an all-zero block gives the zero code and absmax 0."""
    q1, q2 = ref.maps()
    rng = np.random.default_rng(0)
    x = (rng.standard_normal(3 * 2048 + 5) * 10.0 ** rng.uniform(-7, 0, 3 * 2048 + 5)).astype(np.float32)
    codes, absmax = ref.quantise(x, q1, ref.ZERO1)
    assert absmax.shape == (4,) and all(absmax[b] == np.abs(x[b * 2048:(b + 1) * 2048]).max() for b in range(4))
    err = np.abs(ref.dequantise(codes, absmax, q1).astype(np.float64) - x)
    assert np.all(err <= 0.9 / 128 * np.repeat(absmax, 2048)[:x.size].astype(np.float64) * (1 + 1e-6))
    codes2, absmax2 = ref.quantise(x * x, q2, ref.ZERO2)
    err2 = np.abs(ref.dequantise(codes2, absmax2, q2).astype(np.float64) - (x * x))
    assert np.all(err2 <= 0.9 / 256 * np.repeat(absmax2, 2048)[:x.size].astype(np.float64) * (1 + 1e-6))
    for q, zero in ((q1, ref.ZERO1), (q2, ref.ZERO2)):
        c, a = ref.quantise(q, q, zero)
        assert a[0] == 1.0 and np.array_equal(c, np.arange(256))
        c, a = ref.quantise(np.zeros(5, np.float32), q, zero)
        assert a[0] == 0.0 and np.all(c == zero)


def test_block_table_on_the_mixed_layout():
    st = _opt(8)
    rows, spans = st.rows.numpy(), st.spans
    assert rows.dtype == np.int64 and rows.shape[1] == 4 and "frozen" not in spans and st.layout["frozen"][0] == st.n_opt
    assert set(spans) == set(NUMEL) - {"frozen"}
    covered = np.zeros(st.n, dtype=np.int32)
    used = {0: np.zeros(st.m32.numel(), np.int32), 1: np.zeros(st.state1.numel(), np.int32)}
    r = 0
    for k, (off, shp) in st.layout.items():
        if k == "frozen":
            continue
        n = shp.numel()
        is8, soff, r0, nr = spans[k]
        assert is8 == (n >= 4096) and r0 == r and nr == -(-n // 2048) and soff % 8 == 0, k     # the small-tensor rule
        for b in range(nr):
            o, ln, so, kind = rows[r]
            assert (o, so, kind) == (off + 2048 * b, soff + 2048 * b, int(is8)), (k, b)        # blocks start at the tensor's first element
            assert ln == min(2048, n - 2048 * b) and o % 8 == 0 and so % 8 == 0                # the last block is short
            assert off <= o and o + ln <= off + n                                              # no straddling
            covered[o:o + ln] += 1
            used[kind][so:so + ln] += 1
            r += 1
    assert r == rows.shape[0] == 2 + 3 + 4 + 5 + 2 + 1 + 1 == st.absmax1.numel() == st.absmax2.numel()
    inside = np.zeros(st.n, dtype=bool)
    for k, (off, shp) in st.layout.items():
        inside[off:off + shp.numel()] = k != "frozen"
    assert np.array_equal(covered == 1, inside) and covered.max() == 1        # every optimised element once; padding and frozen: never
    assert used[0].max() == 1 and used[1].max() == 1
    assert int(used[1].sum()) == 4096 + 4097 + 6149 + 10000 and int(used[0].sum()) == 4095 + 8 + 1
    assert not hasattr(st, "m") and not hasattr(st, "v")
    assert st.state1.dtype == st.state2.dtype == torch.uint8 and bool((st.state1 == 127).all()) and not st.state2.any()
    assert not st.absmax1.any() and not st.absmax2.any() and not st.m32.any() and not st.v32.any()
    # min_8bit_size moves the rule; nothing optimised: arrays stay allocated, no rows
    assert all(s[0] for s in _opt(8, min_8bit_size=1).spans.values())
    assert not any(s[0] for s in _opt(8, min_8bit_size=1 << 20).spans.values())
    none = _opt(8, frozen=set(NUMEL))
    assert none.rows.shape == (0, 4) and none.absmax1.numel() == 1 and none.state1.numel() == 8


def test_symbol_is_declared_bound_and_checks_its_arguments_without_a_gpu():
    src = open(os.path.join(ROOT, "include", "skg.h")).read()
    assert re.search(r"int skg_adamw8_step\(float\* param, const float\* grad, void\* param_f16, unsigned char\* state1,[^;]*"
                     r"const SkgAdamw8Row\* rows, int nrows,[^;]*const float\* skip, void\* stream\);", src)
    assert re.search(r"typedef struct SkgAdamw8Row \{\s*long long off, len, state_off, is8;\s*\} SkgAdamw8Row;", src)
    assert re.search(r"#define SKG_ABI_VERSION 6\b", src)
    assert _lib.SIGNATURES["skg_adamw8_step"] == ("i", "pppppppppp" + "ip" + "fffff" + "if" + "pp")
    assert _lib.ABI_VERSION == 6 and _lib.lib.skg_abi_version() == 6 and hasattr(ops, "adamw8_step")
    fn = _lib.lib.skg_adamw8_step
    ptrs = [64] * 10                   # param, grad, param_f16, state1, state2, absmax1, absmax2, exp_avg32, exp_avg_sq32, rows
    tail = (1e-3, 0.9, 0.999, 1e-8, 1e-2, 1, 1.0)
    for i in range(10):
        if i == 2:
            continue                   # param_f16 is optional
        a = list(ptrs)
        a[i] = None
        assert fn(*a, 4, 64, *tail, None, None) == -1, i
    assert fn(*ptrs, 4, None, *tail, None, None) == -1                         # no maps
    assert fn(*ptrs, -1, 64, *tail, None, None) == -1                          # a negative row count
    assert fn(*ptrs, 4, 64, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 0, 1.0, None, None) == -1      # step 0
    assert fn(*ptrs, 0, 64, *tail, None, None) == 0                            # no rows: nothing to launch


def _fill(st, seed):
    """Distinct non-trivial values in every state buffer (no kernel on the CPU)."""
    g = torch.Generator().manual_seed(seed)
    bufs = (st.m, st.v) if st.state_bits == 32 else (st.state1, st.state2, st.absmax1, st.absmax2, st.m32, st.v32)
    for t in bufs:
        t.copy_(torch.randint(0, 256, t.shape, generator=g).to(t.dtype) if t.dtype == torch.uint8 else torch.rand(t.shape, generator=g))
    st.step_count = 7
    return [t.clone() for t in bufs]


@pytest.mark.parametrize("bits", [32, 8])
def test_optimizer_state_dict_keys_and_round_trip(bits):
    st = _opt(bits)
    _fill(st, 11)
    sd = st.optimizer_state_dict()
    opt_keys = [k for k in st.layout if k != "frozen"]
    assert list(sd) == ["step", "state_bits", "state"] + (["qmap1", "qmap2"] if bits == 8 else [])
    assert sd["step"] == 7 and sd["state_bits"] == bits and list(sd["state"]) == opt_keys
    for k in opt_keys:
        e, shp = sd["state"][k], st.layout[k][1]
        if bits == 8 and NUMEL[k] >= 4096:
            assert list(e) == ["state1", "state2", "absmax1", "absmax2"]
            assert e["state1"].dtype == e["state2"].dtype == torch.uint8 and e["state1"].shape == e["state2"].shape == shp
            assert e["absmax1"].dtype == torch.float32 and e["absmax1"].shape == e["absmax2"].shape == (-(-NUMEL[k] // 2048),)
        else:
            assert list(e) == ["exp_avg", "exp_avg_sq"] and e["exp_avg"].dtype == torch.float32
            assert e["exp_avg"].shape == e["exp_avg_sq"].shape == shp
    if bits == 8:
        assert torch.equal(sd["qmap1"], flat_adamw.quant_maps()[0]) and torch.equal(sd["qmap2"], flat_adamw.quant_maps()[1])
    other = _opt(bits)
    other.load_optimizer_state_dict(sd)
    assert other.step_count == 7
    again = other.optimizer_state_dict()
    for k in opt_keys:
        assert all(torch.equal(again["state"][k][f], sd["state"][k][f]) for f in sd["state"][k]), k
    sd["state"][opt_keys[0]][list(sd["state"][opt_keys[0]])[0]].zero_()          # clones: the optimizer keeps its own
    assert not torch.equal(st.optimizer_state_dict()["state"][opt_keys[0]][list(sd["state"][opt_keys[0]])[0]],
                           sd["state"][opt_keys[0]][list(sd["state"][opt_keys[0]])[0]])


def test_loading_the_other_mode_or_other_keys_raises_and_writes_nothing():
    a32, a8 = _opt(32), _opt(8)
    _fill(a32, 1)
    _fill(a8, 2)
    sd32, sd8 = a32.optimizer_state_dict(), a8.optimizer_state_dict()
    fresh32, fresh8 = _opt(32), _opt(8)
    with pytest.raises(ValueError, match="state_bits = 8 cannot be loaded into state_bits = 32"):
        fresh32.load_optimizer_state_dict(sd8)
    with pytest.raises(ValueError, match="state_bits = 32 cannot be loaded into state_bits = 8"):
        fresh8.load_optimizer_state_dict(sd32)
    missing = dict(sd8, state={k: v for k, v in sd8["state"].items() if k != "b1"})
    with pytest.raises(ValueError, match="other keys.*b1"):
        fresh8.load_optimizer_state_dict(missing)
    with pytest.raises(ValueError, match="w4096.*min_8bit_size = 8192"):                             # same keys, another small-tensor rule
        _opt(8, min_8bit_size=8192).load_optimizer_state_dict(sd8)
    with pytest.raises(ValueError, match="other maps"):
        fresh8.load_optimizer_state_dict(dict(sd8, qmap1=sd8["qmap1"] * 2))
    assert fresh8.step_count == 0 and bool((fresh8.state1 == 127).all()) and not fresh8.absmax1.any() and not fresh8.m32.any()
    assert fresh32.step_count == 0 and not fresh32.m.any() and not fresh32.v.any()


def test_state_bits_32_is_the_optimizer_it_was(monkeypatch):
    st, default = _opt(32), _opt(32)
    args = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, schedule=lambda s: 1.0, grad_scale=8.0, frozen={"frozen"})
    g = torch.Generator().manual_seed(3)
    default = flat_adamw.FlatAdamW(ref.MIXED, {k: torch.randn(shp, generator=g) for k, shp in ref.MIXED}, "cpu", **args)
    assert set(vars(st)) == set(vars(default)) and default.state_bits == 32 and default.min_8bit_size == 4096
    assert st.m.shape == st.v.shape == st.p.shape and not st.m.any() and not st.v.any()
    for name in ("rows", "spans", "state1", "state2", "absmax1", "absmax2", "m32", "v32", "qtab"):
        assert not hasattr(st, name), name
    calls, calls8 = [], []
    monkeypatch.setattr(ops, "adamw_step", lambda *a: calls.append(a))
    monkeypatch.setattr(ops, "adamw8_step", lambda *a: calls8.append(a))
    assert st.step(st.new_grad()) is True and len(calls) == 1 and not calls8
    st8 = _opt(8)
    assert st8.step(st8.new_grad()) is True and len(calls) == 1 and len(calls8) == 1 and st8.step_count == 1 and st8.stale
    p, gr, p16, s1, s2, a1, a2, m32, v32, rows, qtab, lr, b1, b2, eps, wd, step, inv, flag = calls8[0]
    assert p.numel() == gr.numel() == p16.numel() == st8.n_opt and p.data_ptr() == st8.p.data_ptr() and flag is None
    assert (lr, b1, b2, eps, wd, step, inv) == (1e-3, 0.9, 0.999, 1e-8, 1e-2, 1, 1.0 / 8.0) and rows is st8.rows and qtab is st8.qtab
    bad = st8.new_grad()
    bad[5] = float("nan")
    assert st8.step(bad) is False and len(calls8) == 1 and st8.step_count == 1
    with pytest.raises(AssertionError):
        _opt(16)


def test_trainers_take_and_pass_the_two_arguments():
    import inspect
    from sketch2img_amd.clip_vision_train import HipClipTowerTrainer
    from sketch2img_amd.lgp_train import HipLGPTrainer
    from sketch2img_amd.sat_train import HipSatTrainer
    for cls in (flat_adamw.FlatAdamW, HipLGPTrainer, HipSatTrainer, HipClipTowerTrainer):
        sig = inspect.signature(cls.__init__).parameters
        assert sig["state_bits"].default == 32 and sig["min_8bit_size"].default == 4096, cls
