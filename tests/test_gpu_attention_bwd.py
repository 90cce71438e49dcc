"""The attention backward launches (skg_attn_bwd_delta, skg_attn_bwd_dq with delta and with the delta prologue, skg_attn_bwd_dkv)
on the GPU (-m gpu) against fp64 arithmetic on the same fp16 inputs.

Parity bounds: twice the distance of tests/attn_emulation.py - the launches restated in fp64 with the kernels' own fp16 roundings -
from exact arithmetic, whole tensor (E) and per row (E_row), computed here from the emulation and never from the kernel's result
(factor 2: the convention of tests/test_gpu_sat_train.py).  Shapes: the smallest that reach every tile position (workgroup tile 128
up to dh = 40 and 64 beyond, inner tile 64, a residue of 1 past a tile, key counts that are no multiple of 8).

Exact-answer probes: one-hot / coded operands with closed-form gradients, lse and delta supplied analytically, so that a failure
names the tile and the slot of a backward kernel (a wrong key <-> k-slot map in a transposing LDS read, a lost tile, a ragged-tile
mask off by one).  Operand views: Q / K / V / dQ / dK / dV as column blocks of fused buffers, the way unet.py, inject.py and
clip_vision.py call the kernels, bit-equal to the dense calls; finite garbage in the pad key slots changes no bit."""
import functools

import pytest
import torch

from tests import attn_emulation as ae
from tests.util import report

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from sketch2img_amd import ops as o
    return o


def _pad_kv(x, kvs, fill):
    """[B, Nkv, C] -> device [B * kvs, C], rows Nkv .. kvs - 1 of every batch row = fill."""
    B, Nkv, C = x.shape
    out = torch.full((B, kvs, C), fill, dtype=torch.float16)
    out[:, :Nkv] = x
    return out.reshape(B * kvs, C).to(DEV)


def _valid(buf, B, Nkv, kvs):
    """(valid rows [B, Nkv, C], pad rows) of a [B * kvs, C] device buffer, on the CPU."""
    x = buf.cpu().view(B, kvs, -1)
    return x[:, :Nkv], x[:, Nkv:]


def _dkv(ops, Q, K, V, dO, lse, delta, B, heads, Nq, Nkv, kvs, dh, scale):
    """skg_attn_bwd_dkv into sentinel-filled buffers (the key-stride form; the dense call where kv_stride = Nkv) ->
    valid rows of dK, dV [B, Nkv, C] on the CPU; the pad rows must keep the sentinel."""
    C = heads * dh
    if kvs == Nkv:
        dK, dV = ops.attn_bwd_dkv(Q, K, V, dO, lse, delta, B, heads, Nq, Nkv, dh, scale)
        return dK.cpu().view(B, Nkv, C), dV.cpu().view(B, Nkv, C)
    dK = torch.full((B * kvs, C), ae.OUT_SENTINEL, dtype=torch.float16, device=DEV)
    dV = torch.full((B * kvs, C), ae.OUT_SENTINEL, dtype=torch.float16, device=DEV)
    ops.attn_bwd_dkv_strided(Q, K, V, dO, lse, delta, B, heads, Nq, Nkv, kvs, dh, scale, dK, dV)
    (dk, pk), (dv, pv) = _valid(dK, B, Nkv, kvs), _valid(dV, B, Nkv, kvs)
    assert bool((pk == ae.OUT_SENTINEL).all()) and bool((pv == ae.OUT_SENTINEL).all()), "pad rows of dK / dV were written"
    return dk, dv


# ---------------------------------------------------------------------------------------------- parity against fp64
@functools.lru_cache(maxsize=None)
def _reference(dh, heads, B, Nq, Nkv, e):
    """Inputs, emulation and exact gradients of one case: computed once, shared, never written to."""
    q, k, v, do = ae.case(dh, heads, B, Nq, Nkv, 2.0 ** e)
    from sketch2img_amd import ops
    variant, _ = ops.attn_fwd_variant(B, heads, Nq, Nkv, ae.kv_stride_of(dh, Nkv), dh, v_rows=True)      # the forward _parity runs
    return (q, k, v, do), ae.emulate(q, k, v, do, heads, dh ** -0.5, denom_fp16=ae.fwd_denom_fp16(variant, dh))


def _parity(ops, dh, heads, B, Nq, Nkv, e):
    (q, k, v, do), ref = _reference(dh, heads, B, Nq, Nkv, e)
    C, kvs, scale = heads * dh, ae.kv_stride_of(dh, Nkv), dh ** -0.5
    Q, dO = q.reshape(B * Nq, C).to(DEV), do.reshape(B * Nq, C).to(DEV)
    K, V = _pad_kv(k, kvs, ae.K_PAD), _pad_kv(v, kvs, ae.V_PAD)
    o, lse = ops.attn_fwd(Q, K, V, B, heads, Nq, Nkv, kvs, dh, scale, want_lse=True, v_rows=True)
    delta = ops.attn_bwd_delta(o, dO, B, heads, Nq, dh)
    dq = ops.attn_bwd_dq(Q, K, V, dO, lse, delta, B, heads, Nq, Nkv, kvs, dh, scale)
    dq_f, delta_f = ops.attn_bwd_dq_delta(Q, K, V, dO, o, lse, B, heads, Nq, Nkv, kvs, dh, scale)
    dk, dv = _dkv(ops, Q, K, V, dO, lse, delta, B, heads, Nq, Nkv, kvs, dh, scale)
    assert float((delta_f - delta).abs().max()) <= 2e-5 * max(1.0, float(delta.abs().max()))
    tag = f"dh{dh} h{heads} b{B} {Nq}x{Nkv} dO*2^{e}"
    fails = []
    for name, got, key in (("dq", dq.cpu().view(B, Nq, C), "dq"), ("dq(prologue)", dq_f.cpu().view(B, Nq, C), "dq"),
                           ("dk", dk, "dk"), ("dv", dv, "dv")):
        r = ref[key]
        report(f"attn bwd {name} {tag}", got.float(), r["exact"])
        d, d_row = ae.distances(got, r["exact"])
        print(f"[attn-bwd] {tag} {name}: E={r['E']:.3e} E_row={r['E_row']:.3e} kernel={d:.3e} kernel_row={d_row:.3e} "
              f"ratio={d / r['E']:.3f} ratio_row={d_row / r['E_row']:.3f}")
        if not bool(torch.isfinite(got).all()):
            fails.append(f"{name}: not finite")
        if not d <= 2 * r["E"]:
            fails.append(f"{name}: whole tensor {d:.3e} > 2 x {r['E']:.3e}")
        if not d_row <= 2 * r["E_row"]:
            fails.append(f"{name}: row {d_row:.3e} > 2 x {r['E_row']:.3e}")
    assert not fails, f"{tag}: " + "; ".join(fails)


@pytest.mark.parametrize("dh,heads,B,Nq,Nkv", ae.SHAPES)
def test_backward_parity(ops, dh, heads, B, Nq, Nkv):
    """dQ (both delta forms), dK, dV within 2 E of exact fp64 whole-tensor and 2 E_row per row; the prologue's delta is the stand-alone
    one to fp32 rounding.  Pad key slots hold finite non-zero values; pad rows of dK / dV keep their sentinel."""
    _parity(ops, dh, heads, B, Nq, Nkv, 0)


@pytest.mark.parametrize("e", [-16, -12, -8, 8, 12])
@pytest.mark.parametrize("dh,heads,B,Nq,Nkv", ae.MAGNITUDE_SHAPES)
def test_backward_parity_over_gradient_magnitude(ops, dh, heads, B, Nq, Nkv, e):
    """dO scaled by 2^e: finite and within the same 2 E / 2 E_row.  E is flat (3.5 - 4.3e-4) from 2^-8 up to the trainers' loss scale
    and beyond; at 2^-12 it is ~1e-3 and at 2^-16 ~1e-2: dS underflows fp16 (what LOSS_SCALE = 2^13 exists for) - the kernels must
    lose exactly what the format loses there, no more (profiles/attn_bwd_parity.txt)."""
    _parity(ops, dh, heads, B, Nq, Nkv, e)


# ---------------------------------------------------------------------------------------------- exact-answer probes
def _probe_operands(p, Nkv, kvs):
    B, Nq, C = p["q"].shape
    return (p["q"].reshape(B * Nq, C).to(DEV), _pad_kv(p["k"], kvs, ae.K_PAD), _pad_kv(p["v"], kvs, ae.V_PAD),
            p["do"].reshape(B * Nq, C).to(DEV), p["lse"].to(DEV), p["delta"].to(DEV))


@pytest.mark.parametrize("Nq,Nkv,kvs", ae.PROBE_GEOMETRIES)
@pytest.mark.parametrize("dh,heads", ae.PROBE_CONFIGS)
def test_probe_dv(ops, dh, heads, Nq, Nkv, kvs):
    """K = 0 (P uniform), dO one-hot on (query q*, column c): dV[j][c] = s / Nkv for every valid key, every other column and all of dK
    exactly 0.  Fails on a lost query tile or a wrong query <-> k-slot map in the dO^T read."""
    B, scale = ae.PROBE_B, dh ** -0.5
    Qh = ae.probe_q(dh, heads, Nq)
    for qs, _, c, _ in ae.probe_sweep("dv", dh, Nq, Nkv):
        p = ae.probe_dv(dh, heads, Nq, Nkv, qs, c, q=Qh)
        Q, K, V, dO, lse, delta = _probe_operands(p, Nkv, kvs)
        dk, dv = _dkv(ops, Q, K, V, dO, lse, delta, B, heads, Nq, Nkv, kvs, dh, scale)
        ae.probe_check(dv, p["dv"], f"dV probe dh{dh} {Nq}x{Nkv} q*={qs} c={c}")
        ae.probe_check(dk, p["dk"], f"dV probe (dK) dh{dh} {Nq}x{Nkv} q*={qs} c={c}")


@pytest.mark.parametrize("Nq,Nkv,kvs", ae.PROBE_GEOMETRIES)
@pytest.mark.parametrize("dh,heads", ae.PROBE_CONFIGS)
def test_probe_dk(ops, dh, heads, Nq, Nkv, kvs):
    """K = 0, V one-hot on (key j*, column c), dO one-hot on (query q*, column c): dK[j] = scale (1 / Nkv)(delta_{j j*} - 1 / Nkv) s Q[q*].
    Fails on a wrong Q^T read or a wrong key <-> lane map."""
    B, scale = ae.PROBE_B, dh ** -0.5
    Qh = ae.probe_q(dh, heads, Nq)
    for qs, js, c, _ in ae.probe_sweep("dk", dh, Nq, Nkv):
        p = ae.probe_dk(dh, heads, Nq, Nkv, qs, js, c, q=Qh)
        Q, K, V, dO, lse, delta = _probe_operands(p, Nkv, kvs)
        dk, _ = _dkv(ops, Q, K, V, dO, lse, delta, B, heads, Nq, Nkv, kvs, dh, scale)
        ae.probe_check(dk, p["dk"], f"dK probe dh{dh} {Nq}x{Nkv} q*={qs} j*={js} c={c}")


@pytest.mark.parametrize("Nq,Nkv,kvs", ae.PROBE_GEOMETRIES)
@pytest.mark.parametrize("dh,heads", ae.PROBE_CONFIGS)
def test_probe_dq(ops, dh, heads, Nq, Nkv, kvs):
    """Q = 0 (P uniform whatever K is), K = code_j = j % 13 + 1 in column col, V one-hot on (key j*, column c), dO one-hot on (query q*,
    column c): dQ[q*][col] = scale (s / Nkv)(code_j* - mean code), every other row and column exactly 0.  Fails on a wrong K^T read, a
    lost key tile, or a ragged-tile mask off by one (which moves the mean)."""
    B, scale, C = ae.PROBE_B, dh ** -0.5, heads * dh
    for qs, js, c, col in ae.probe_sweep("dq", dh, Nq, Nkv):
        p = ae.probe_dq(dh, heads, Nq, Nkv, qs, js, c, col)
        Q, K, V, dO, lse, delta = _probe_operands(p, Nkv, kvs)
        dq = ops.attn_bwd_dq(Q, K, V, dO, lse, delta, B, heads, Nq, Nkv, kvs, dh, scale)
        ae.probe_check(dq.cpu().view(B, Nq, C), p["dq"], f"dQ probe dh{dh} {Nq}x{Nkv} q*={qs} j*={js} c={c} col={col}")


# ---------------------------------------------------------------------------------------------- operand views and pad slots
SENT = 3.0


def _inside(t, pad=24, off=8):
    """t as a column view (offset `off`) of a wider sentinel-filled device buffer, and the buffer."""
    buf = torch.full((t.shape[0], t.shape[1] + pad), SENT, dtype=torch.float16, device=DEV)
    buf[:, off:off + t.shape[1]] = t.to(DEV)
    return buf[:, off:off + t.shape[1]], buf


@pytest.mark.parametrize("dh,heads", [(40, 8), (64, 5)])
def test_fused_buffer_views_self_attention(ops, dh, heads):
    """Self-attention the way the UNet and the CLIP tower call it: Q, K, V are the column blocks of one [B N, 3C] buffer, dO and O sit
    inside wider buffers at a column offset, dQ, dK, dV go to the column blocks of one [B N, 3C + 8] buffer.  Bit-equal to the dense
    calls, the 8 trailing columns untouched (at dh = 40 only the d < dh guard of the store loop keeps the last head of dQ out of dK's
    block).  N = 129: kv_stride = 129, two workgroups at dh 40 and three at dh 64, the last ragged by one."""
    B, N, C, scale = 2, 129, heads * dh, dh ** -0.5
    qkv = ae.rnd(B * N, 3 * C, seed=5).to(DEV)
    Q, K, V = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    dO, _ = _inside(ae.rnd(B * N, C, seed=6))
    o_buf = torch.full((B * N, C + 24), SENT, dtype=torch.float16, device=DEV)
    O = o_buf[:, 8:8 + C]
    _, lse = ops.attn_fwd(Q, K, V, B, heads, N, N, N, dh, scale, out=O, want_lse=True, v_rows=True)
    delta = ops.attn_bwd_delta(O, dO, B, heads, N, dh)
    Qc, Kc, Vc, dOc, Oc = (t.contiguous() for t in (Q, K, V, dO, O))
    assert torch.equal(delta, ops.attn_bwd_delta(Oc, dOc, B, heads, N, dh))
    dq_d = ops.attn_bwd_dq(Qc, Kc, Vc, dOc, lse, delta, B, heads, N, N, N, dh, scale)
    dqf_d, deltaf_d = ops.attn_bwd_dq_delta(Qc, Kc, Vc, dOc, Oc, lse, B, heads, N, N, N, dh, scale)
    dk_d, dv_d = ops.attn_bwd_dkv(Qc, Kc, Vc, dOc, lse, delta, B, heads, N, N, dh, scale)
    for prologue in (False, True):
        dqkv = torch.full((B * N, 3 * C + 8), SENT, dtype=torch.float16, device=DEV)
        if prologue:
            _, deltaf = ops.attn_bwd_dq_delta(Q, K, V, dO, O, lse, B, heads, N, N, N, dh, scale, out=dqkv[:, :C])
            assert torch.equal(deltaf, deltaf_d)
        else:
            ops.attn_bwd_dq(Q, K, V, dO, lse, delta, B, heads, N, N, N, dh, scale, out=dqkv[:, :C])
        ops.attn_bwd_dkv_strided(Q, K, V, dO, lse, delta, B, heads, N, N, N, dh, scale, dqkv[:, C:2 * C], dqkv[:, 2 * C:3 * C])
        assert torch.equal(dqkv[:, :C], dqf_d if prologue else dq_d)
        assert torch.equal(dqkv[:, C:2 * C], dk_d) and torch.equal(dqkv[:, 2 * C:3 * C], dv_d)
        assert bool((dqkv[:, 3 * C:] == SENT).all())
    assert float(dq_d.float().abs().max()) > 0 and float(dk_d.float().abs().max()) > 0 and float(dv_d.float().abs().max()) > 0
    assert bool((o_buf[:, :8] == SENT).all()) and bool((o_buf[:, 8 + C:] == SENT).all())


@pytest.mark.parametrize("dh,heads", [(40, 8), (64, 5)])
def test_fused_buffer_views_padded_cross_attention(ops, dh, heads):
    """Cross-shaped and padded: 64 queries, 77 keys in 80 slots.  K, V are the column blocks of one [B 80, 2C] buffer, dK, dV go to the
    column blocks of one [B 80, 2C + 8] buffer, Q, dO, O, dQ sit inside wider buffers.  Bit-equal to the dense calls; the pad rows of
    dK / dV and every column outside the blocks keep their sentinel."""
    B, Nq, Nkv, kvs, C, scale = 2, 64, 77, 80, heads * dh, dh ** -0.5
    kv = ae.rnd(B * kvs, 2 * C, seed=7).to(DEV)
    K, V = kv[:, :C], kv[:, C:]
    Q, _ = _inside(ae.rnd(B * Nq, C, seed=8))
    dO, _ = _inside(ae.rnd(B * Nq, C, seed=9), pad=40, off=16)
    O, _ = _inside(torch.zeros(B * Nq, C, dtype=torch.float16))
    _, lse = ops.attn_fwd(Q, K, V, B, heads, Nq, Nkv, kvs, dh, scale, out=O, want_lse=True, v_rows=True)
    delta = ops.attn_bwd_delta(O, dO, B, heads, Nq, dh)
    Qc, Kc, Vc, dOc, Oc = (t.contiguous() for t in (Q, K, V, dO, O))
    dq_d = ops.attn_bwd_dq(Qc, Kc, Vc, dOc, lse, delta, B, heads, Nq, Nkv, kvs, dh, scale)
    dqf_d, deltaf_d = ops.attn_bwd_dq_delta(Qc, Kc, Vc, dOc, Oc, lse, B, heads, Nq, Nkv, kvs, dh, scale)
    dk_d = torch.full((B * kvs, C), SENT, dtype=torch.float16, device=DEV)
    dv_d = torch.full((B * kvs, C), SENT, dtype=torch.float16, device=DEV)
    ops.attn_bwd_dkv_strided(Qc, Kc, Vc, dOc, lse, delta, B, heads, Nq, Nkv, kvs, dh, scale, dk_d, dv_d)
    dq_buf = torch.full((B * Nq, C + 24), SENT, dtype=torch.float16, device=DEV)
    ops.attn_bwd_dq(Q, K, V, dO, lse, delta, B, heads, Nq, Nkv, kvs, dh, scale, out=dq_buf[:, 8:8 + C])
    assert torch.equal(dq_buf[:, 8:8 + C], dq_d)
    assert bool((dq_buf[:, :8] == SENT).all()) and bool((dq_buf[:, 8 + C:] == SENT).all())
    _, deltaf = ops.attn_bwd_dq_delta(Q, K, V, dO, O, lse, B, heads, Nq, Nkv, kvs, dh, scale, out=dq_buf[:, 8:8 + C])
    assert torch.equal(dq_buf[:, 8:8 + C], dqf_d) and torch.equal(deltaf, deltaf_d)
    dkv = torch.full((B * kvs, 2 * C + 8), SENT, dtype=torch.float16, device=DEV)
    ops.attn_bwd_dkv_strided(Q, K, V, dO, lse, delta, B, heads, Nq, Nkv, kvs, dh, scale, dkv[:, :C], dkv[:, C:2 * C])
    assert torch.equal(dkv[:, :C], dk_d) and torch.equal(dkv[:, C:2 * C], dv_d)
    assert bool((dkv[:, 2 * C:] == SENT).all())
    pad = torch.cat([torch.arange(b * kvs + Nkv, (b + 1) * kvs) for b in range(B)]).to(DEV)
    assert bool((dkv[pad] == SENT).all()) and bool((dk_d[pad] == SENT).all()) and bool((dv_d[pad] == SENT).all())
    rows = torch.cat([torch.arange(b * kvs, b * kvs + Nkv) for b in range(B)]).to(DEV)
    assert bool((dkv[rows][:, :2 * C] != SENT).any(dim=1).all()) and float(dq_d.float().abs().max()) > 0


@pytest.mark.parametrize("dh,heads", ae.PROBE_CONFIGS)
def test_finite_garbage_in_pad_key_slots_changes_no_bit(ops, dh, heads):
    """include/skg.h: key slots Nkv .. kv_stride - 1 are read and must hold finite values.  77 keys in 80 slots, pad rows zero against
    pad rows of 30.0 in K and 65504.0 in V: dQ (both delta forms), delta, dK and dV are bit-equal."""
    B, Nq, Nkv, kvs, C, scale = 2, 129, 77, 80, heads * dh, dh ** -0.5
    q, k, v, do = ae.case(dh, heads, B, Nq, Nkv)
    Q, dO = q.reshape(B * Nq, C).to(DEV), do.reshape(B * Nq, C).to(DEV)
    K0, V0 = _pad_kv(k, kvs, 0.0), _pad_kv(v, kvs, 0.0)
    o, lse = ops.attn_fwd(Q, K0, V0, B, heads, Nq, Nkv, kvs, dh, scale, want_lse=True, v_rows=True)
    delta = ops.attn_bwd_delta(o, dO, B, heads, Nq, dh)
    res = []
    for K, V in ((K0, V0), (_pad_kv(k, kvs, 30.0), _pad_kv(v, kvs, 65504.0))):
        dq = ops.attn_bwd_dq(Q, K, V, dO, lse, delta, B, heads, Nq, Nkv, kvs, dh, scale)
        dq_f, delta_f = ops.attn_bwd_dq_delta(Q, K, V, dO, o, lse, B, heads, Nq, Nkv, kvs, dh, scale)
        dk, dv = _dkv(ops, Q, K, V, dO, lse, delta, B, heads, Nq, Nkv, kvs, dh, scale)
        res.append((dq.cpu(), dq_f.cpu(), delta_f.cpu(), dk, dv))
    for a, b in zip(*res):
        assert bool(torch.isfinite(a.float()).all()) and float(a.float().abs().max()) > 0
        assert torch.equal(a, b)
