"""tests/attn_emulation.py checked on the CPU: the inputs of tests/test_gpu_attention_bwd.py are chosen so that its bounds mean
something (rounding noise well under 1e-3), and the closed forms of its exact-answer probes are what the kernels' arithmetic -
restated with the kernels' roundings - gives."""
import pytest
import torch

from tests import attn_emulation as ae

FP16_MIN_NORMAL = 2.0 ** -14


@pytest.mark.parametrize("dh,heads,B,Nq,Nkv", ae.SHAPES)
def test_rounding_noise_of_the_parity_inputs(dh, heads, B, Nq, Nkv):
    """At every parity shape, dO scaled by 2^-8, 1 and 2^12: the emulation is finite and within 1e-3 of exact arithmetic (measured:
    3.5 - 4.3e-4).  A condition on the inputs - a bound of 2 E is only sharp while E is rounding noise - not a tolerance on a kernel."""
    for e in (-8, 0, 12):
        q, k, v, do = ae.case(dh, heads, B, Nq, Nkv, 2.0 ** e)
        r = ae.emulate(q, k, v, do, heads, dh ** -0.5, denom_fp16=(dh == 40 and ae.kv_stride_of(dh, Nkv) > 80))
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
