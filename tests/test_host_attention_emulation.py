"""tests/attn_emulation.py checked on the CPU: the inputs of tests/test_gpu_attention_bwd.py and tests/test_gpu_attention_fwd.py are
chosen so that their bounds mean something (rounding noise well under 1e-3), the closed forms of their exact-answer probes are what the
kernels' arithmetic - restated with the kernels' roundings - gives, and every forward case reaches the instantiation of skg_attn_fwd
it is written for (skg_attn_fwd_variant needs no GPU)."""
import math

import pytest
import torch

from tests import attn_emulation as ae

FP16_MIN_NORMAL = 2.0 ** -14


def _variant(c):
    """(code, queries per workgroup) skg_attn_fwd_variant reports for a case: the library loads without a GPU."""
    from sketch2img_amd import ops
    return ops.attn_fwd_variant(c.B, c.heads, c.Nq, c.Nkv, c.kvs, c.dh, causal=bool(c.flags & ae.CAUSAL),
                                v_rows=bool(c.flags & ae.ROWV), resident_kv=bool(c.flags & ae.RESIDENT))


def _denom_fp16(dh, heads, B, Nq, Nkv):
    """The backward tests' forward (row-major V, kv_stride_of): fp16 denominator where the dispatch takes the dh = 40 streaming kernel."""
    from sketch2img_amd import ops
    return ae.fwd_denom_fp16(ops.attn_fwd_variant(B, heads, Nq, Nkv, ae.kv_stride_of(dh, Nkv), dh, v_rows=True)[0], dh)


@pytest.mark.parametrize("dh,heads,B,Nq,Nkv", ae.SHAPES)
def test_rounding_noise_of_the_parity_inputs(dh, heads, B, Nq, Nkv):
    """At every parity shape, dO scaled by 2^-8, 1 and 2^12: the emulation is finite and within 1e-3 of exact arithmetic (measured:
    3.5 - 4.3e-4).  A condition on the inputs - a bound of 2 E is only sharp while E is rounding noise - not a tolerance on a kernel."""
    for e in (-8, 0, 12):
        q, k, v, do = ae.case(dh, heads, B, Nq, Nkv, 2.0 ** e)
        r = ae.emulate(q, k, v, do, heads, dh ** -0.5, denom_fp16=_denom_fp16(dh, heads, B, Nq, Nkv))
        for n in ("dq", "dk", "dv"):
            print(f"[emulation] dh{dh} {Nq}x{Nkv} dO*2^{e} {n}: E={r[n]['E']:.3e} E_row={r[n]['E_row']:.3e}")
            assert bool(torch.isfinite(r[n]["emu"]).all()), (n, e)
            assert r[n]["E"] < 1e-3, (n, e, r[n]["E"])
            assert r[n]["E_row"] >= r[n]["E"] * (1 - 1e-9)      # max row >= rms row: the row metric sees what the whole tensor sees


def test_emulated_forward_is_the_attention():
    """The restated forward against plain fp64 softmax attention: one fp16 rounding of q~, of P and of O apart; lse to 1e-3."""
    dh, heads, B, Nq, Nkv = 40, 4, 2, 129, 77
    q, k, v, _ = ae.case(dh, heads, B, Nq, Nkv)
    for denom in (False, True):
        o, lse = ae.forward(q, k, v, heads, dh ** -0.5, denom_fp16=denom)
        qh, kh, vh = (ae._heads(t, heads) for t in (q, k, v))
        s = qh @ kh.transpose(-1, -2) * dh ** -0.5
        ref = ae._rows(torch.softmax(s, -1) @ vh)
        assert ae.distances(o, ref)[0] < 1e-3
        assert float((lse.double() - torch.logsumexp(s, -1)).abs().max()) < 1e-3


def _normal_or_zero(ds):
    a = ds.double().abs()
    return bool(((a == 0) | (a >= FP16_MIN_NORMAL)).all())


@pytest.mark.parametrize("Nq,Nkv,kvs", ae.PROBE_GEOMETRIES)
@pytest.mark.parametrize("dh,heads", ae.PROBE_CONFIGS)
def test_probe_closed_forms_are_what_the_emulation_gives(dh, heads, Nq, Nkv, kvs):
    """Every probe of test_gpu_attention_bwd.py through the emulated launches, with the analytic lse and delta: the closed form within
    the probes' tolerance, analytic zeros exactly zero, and every dS a normal fp16 number or exactly zero (what fixes PROBE_S)."""
    scale = dh ** -0.5
    Q = ae.probe_q(dh, heads, Nq)
    for qs, _, c, _ in ae.probe_sweep("dv", dh, Nq, Nkv):
        p = ae.probe_dv(dh, heads, Nq, Nkv, qs, c, q=Q)
        dk, dv, ds = ae.bwd_dkv(p["q"], p["k"], p["v"], p["do"], p["lse"], p["delta"], heads, scale)
        ae.probe_check(dv, p["dv"], f"dV probe q*={qs} c={c}")
        ae.probe_check(dk, p["dk"], f"dV probe (dK) q*={qs} c={c}")
        assert float(ds.abs().max()) == 0.0
    for qs, js, c, _ in ae.probe_sweep("dk", dh, Nq, Nkv):
        p = ae.probe_dk(dh, heads, Nq, Nkv, qs, js, c, q=Q)
        dk, _, ds = ae.bwd_dkv(p["q"], p["k"], p["v"], p["do"], p["lse"], p["delta"], heads, scale)
        ae.probe_check(dk, p["dk"], f"dK probe q*={qs} j*={js} c={c}")
        assert _normal_or_zero(ds) and float(ds.abs().max()) > 0
        assert float(dk.double().abs().min()) >= FP16_MIN_NORMAL          # no expected dK element is stored as a subnormal
    for qs, js, c, col in ae.probe_sweep("dq", dh, Nq, Nkv):
        p = ae.probe_dq(dh, heads, Nq, Nkv, qs, js, c, col)
        dq, ds = ae.bwd_dq(p["q"], p["k"], p["v"], p["do"], p["lse"], p["delta"], heads, scale)
        ae.probe_check(dq, p["dq"], f"dQ probe q*={qs} j*={js} c={c} col={col}")
        assert _normal_or_zero(ds) and float(ds.abs().max()) > 0


def test_probe_sweeps_reach_every_position():
    for dh, _ in ae.PROBE_CONFIGS:
        for Nq, Nkv, _ in ae.PROBE_GEOMETRIES:
            for kind in ("dk", "dq"):
                sw = ae.probe_sweep(kind, dh, Nq, Nkv)
                assert {s[0] for s in sw} == set(ae.probe_queries(Nq)) and {s[1] for s in sw} == set(ae.probe_keys(Nkv))
                assert {s[2] for s in sw} == set(ae.probe_cols(dh)) and {s[3] for s in sw} == set(ae.probe_cols(dh))
    assert ae.probe_queries(200) == [0, 15, 16, 31, 47, 63, 64, 127, 128, 199] and ae.probe_keys(77) == [0, 15, 16, 63, 64, 76]
    assert ae.probe_keys(200) == [0, 15, 16, 63, 64, 76, 127, 128, 199]


# ---------------------------------------------------------------------------------------------- forward
# E of the emulation against fp64 per input class, measured over FWD_CASES (profiles/attn_fwd_parity.txt): unit 2.7 - 3.6e-4 (the causal
# cases at the low end: their first rows see few keys), peaked 3.7 - 4.9e-4, selector 7e-6 (dh 16: the other keys weigh 2^-23) - 3.8e-4
E_BAND = {"unit": (2.5e-4, 4.0e-4), "peaked": (3.0e-4, 6.0e-4), "selector": (0.0, 5.0e-4)}


def test_emulated_causal_forward_is_the_masked_attention():
    """forward(causal=True) against a masked fp64 softmax built here (not exact_forward): rounding apart, and the rows behind the last
    key (80 rows, 77 keys) see all 77; exact_forward agrees with the same construction to fp64 rounding."""
    dh, heads, B, N, Nkv = 64, 3, 2, 80, 77
    q, k, v, _ = ae.case(dh, heads, B, N, Nkv)
    qh, kh, vh = (ae._heads(t, heads) for t in (q, k, v))
    s = qh @ kh.transpose(-1, -2) * dh ** -0.5 + torch.full((N, Nkv), float("-inf"), dtype=torch.float64).triu(1)
    ref, ref_lse = ae._rows(torch.softmax(s, -1) @ vh), torch.logsumexp(s, -1)
    oe, le = ae.exact_forward(q, k, v, heads, dh ** -0.5, causal=True)
    assert float((oe - ref).abs().max()) < 1e-13 and float((le - ref_lse).abs().max()) < 1e-13
    assert torch.equal(oe[:, 0], v[:, 0].double())                           # query 0 sees key 0 only
    o, lse = ae.forward(q, k, v, heads, dh ** -0.5, causal=True)
    assert ae.distances(o, ref)[0] < 1e-3 and float((lse.double() - ref_lse).abs().max()) < 1e-3
    assert torch.equal(o[:, 0], v[:, 0])


@pytest.mark.parametrize("name,cls", ae.FWD_PARAMS)
def test_forward_cases_rounding_noise_and_dispatch(name, cls):
    """Every forward case and input class: the library reports the instantiation and the queries per workgroup the case is written
    for; E, E_row and D_lse of the emulation are finite, E lies in its class's band (a condition on the inputs, not a tolerance on a
    kernel); the selector key beats every other by more than 2^8 in the log2 domain, on the fp64 scores."""
    c = ae.FWD_BY_NAME[name]
    assert _variant(c) == (c.variant, c.qpw), f"{name}: skg_attn_fwd_variant reports {_variant(c)}"
    assert not (c.flags & ae.ROWV) or not (c.flags & ae.CAUSAL)
    assert (c.flags & ae.ROWV) or c.kvs % 8 == 0
    _, r = ae.emulate_case(c, cls)
    print(f"[emulation fwd] {name} {cls}: E={r['E']:.3e} E_row={r['E_row']:.3e} D_lse={r['D_lse']:.3e}")
    assert bool(torch.isfinite(r["o_emu"]).all()) and bool(torch.isfinite(r["lse_emu"]).all())
    assert all(math.isfinite(r[x]) for x in ("E", "E_row", "D_lse"))
    lo, hi = E_BAND[cls]
    assert lo < r["E"] < hi, (name, cls, r["E"])
    assert r["E_row"] >= r["E"] * (1 - 1e-9) and r["D_lse"] < 6e-3
    if cls == "selector":
        assert ae.selector_margin(c) > 8.0
        js = ae.selector_keys(c.B, c.Nkv)
        nt = (c.Nkv + 63) // 64
        assert js[0] < 64 and js[1] // 64 == nt // 2 and all(j // 64 == nt - 1 for j in js[2:])


def test_forward_cases_reach_every_product_instantiation():
    """(variant, head width, V row-major) over FWD_CASES, as the library reports them, against the list of what skg_attn_fwd can launch
    without an environment switch: streaming QT 2 at dh 16 / 32 / 40 / 64 / 80 and QT 1 at 160 in both V forms, QT 3 at dh 40 in both,
    causal at 16 / 32 / 64, the short-key kernel at 40 / 64 / 80 / 160, the resident one at NT 10 (40 / 64 / 80 / 160) and NT 15 (40 / 64 /
    80).  The short-key kernel runs query chunks of 64, 192 and 512, the resident one 128 and above."""
    required = ({(1002, d, r) for d in (16, 32, 40, 64, 80) for r in (False, True)} | {(1001, 160, False), (1001, 160, True)} |
                {(1003, 40, False), (1003, 40, True)} | {(2002, 16, False), (2002, 32, False), (2002, 64, False)} |
                {(3005, 40, True), (3005, 64, True), (3005, 80, True), (3005, 160, True)} |
                {(3010, 40, True), (3010, 64, True), (3010, 80, True), (3010, 160, True)} |
                {(3015, 40, True), (3015, 64, True), (3015, 80, True)})
    assert required == ae.FWD_REQUIRED
    reached = {(_variant(c)[0], c.dh, bool(c.flags & ae.ROWV)) for c in ae.FWD_CASES}
    assert required <= reached, required - reached
    chunks = lambda code: {_variant(c)[1] for c in ae.FWD_CASES if c.variant == code}
    assert {64, 192, 512} <= chunks(3005) and {128, 256} <= chunks(3010) and {128, 192} <= chunks(3015)
    for c in ae.FWD_PROBES + ae.FWD_CAUSAL_PROBES:
        assert _variant(c) == (c.variant, c.qpw), c.name
    assert {3005, 3010, 3015, 1001, 1002, 1003} <= {c.variant for c in ae.FWD_PROBES} and 512 in {c.qpw for c in ae.FWD_PROBES}


@pytest.mark.parametrize("g", [g for g in ae.FWD_PROBES + ae.FWD_CAUSAL_PROBES if g.B * g.Nq * g.Nkv <= 2 * 264 * 264],
                         ids=lambda g: g.name)
def test_forward_probe_closed_forms_are_what_the_emulation_gives(g):
    """The forward probes of test_gpu_attention_fwd.py through forward(): the closed form within the probes' tolerance (one fp16 unit in
    the last place), analytic zeros exactly zero, lse within 4 fp32 units of ln n.  (The two large launches share the closed forms.)"""
    scale, causal = g.dh ** -0.5, bool(g.flags & ae.CAUSAL)
    Q = ae.probe_q(g.dh, g.heads, g.Nq, g.B)
    for js, c in ae.probe_fwd_sweep(g.dh, g.Nkv):
        p = ae.probe_fwd_causal(g, js, c, q=Q) if causal else ae.probe_fwd_onehot(g, js, c, q=Q)
        o, lse = ae.forward(p["q"], p["k"], p["v"], g.heads, scale, ae.fwd_denom_fp16(g.variant, g.dh), causal)
        ae.probe_fwd_check(o, lse, p, f"{g.name} j*={js} c={c}")
        assert float(p["o"].abs().max()) > 0
    if not causal:
        for c in ae.probe_cols(g.dh):
            if c < g.dh:
                p = ae.probe_fwd_coded(g, c, q=Q)
                o, lse = ae.forward(p["q"], p["k"], p["v"], g.heads, scale, ae.fwd_denom_fp16(g.variant, g.dh))
                ae.probe_fwd_check(o, lse, p, f"{g.name} coded c={c}")


def test_forward_probe_sweeps_reach_every_position():
    assert ae.probe_fwd_keys(77) == [0, 15, 16, 63, 64, 76] and ae.probe_fwd_keys(200) == [0, 15, 16, 63, 64, 76, 127, 128, 191, 192, 199]
    assert {191, 192, 1536} <= set(ae.probe_fwd_keys(1537))
    for g in ae.FWD_PROBES + ae.FWD_CAUSAL_PROBES:
        sw = ae.probe_fwd_sweep(g.dh, g.Nkv)
        assert [s[0] for s in sw] == ae.probe_fwd_keys(g.Nkv) and {s[1] for s in sw} == {c for c in ae.probe_cols(g.dh) if c < g.dh}
