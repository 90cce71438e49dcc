"""skg_attn_fwd on the GPU (-m gpu): every instantiation the launcher dispatches to, named through skg_attn_fwd_variant, against fp64
arithmetic on the same fp16 inputs.

Parity bounds: twice the distance of tests/attn_emulation.py - the forward restated in fp64 with the kernels' own fp16 roundings - from
exact arithmetic, whole tensor (E) and per row (E_row), and lse within 2 D_lse + 8 fp32 roundings; computed from the emulation and
never from the kernel's result (factor 2: the convention of tests/test_gpu_sat_train.py and tests/test_gpu_attention_bwd.py).  The
cases (ae.FWD_CASES) are the smallest launches that reach QT 3 at dh = 40, the short-key kernel's query chunks of 64 / 192 / 512, the
LDS-resident kernel at 10 / 15 score tiles and the causal instantiations, each on unit, peaked and selector inputs.  Pad key slots
hold finite garbage; O is a column block of a wider sentinel-filled buffer.

Exact-answer probes: K = 0 with one-hot / coded V, causal and not, whose outputs are closed forms to one fp16 unit in the last place
and whose zeros are exact - a lost tile, a wrong key <-> k-slot map, a ragged-tile or causal mask off by one names its position.
tests/_attn_var_check.py repeats the unit parity and the one-hot probe in child processes under SKG_ATTN_VAR / SKG_NO_ATTN_SHORT (the
library reads the switches once per process)."""
import functools
import os
import subprocess
import sys

import pytest
import torch

from tests import attn_emulation as ae

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LSE_ROUNDINGS = 8 * 2.0 ** -24


@pytest.fixture(scope="module")
def ops():
    from sketch2img_amd import ops as o
    return o


def _ops():
    from sketch2img_amd import ops as o
    return o


def _pad_kv(x, kvs, fill):
    """[B, Nkv, C] -> device [B * kvs, C], rows Nkv .. kvs - 1 of every batch row = fill."""
    B, Nkv, C = x.shape
    out = torch.full((B, kvs, C), fill, dtype=torch.float16)
    out[:, :Nkv] = x
    return out.reshape(B * kvs, C).to(DEV)


def _kw(flags):
    return dict(causal=bool(flags & ae.CAUSAL), v_rows=bool(flags & ae.ROWV), resident_kv=bool(flags & ae.RESIDENT))


def variant_of(ops, c, flags=None):
    return ops.attn_fwd_variant(c.B, c.heads, c.Nq, c.Nkv, c.kvs, c.dh, **_kw(c.flags if flags is None else flags))


def run_forward(ops, c, q, k, v, flags=None, k_fill=ae.K_PAD, v_fill=ae.V_PAD):
    """One skg_attn_fwd call of case / probe geometry c (flags: another V form of the same case): pad key slots filled, O written into
    columns 8 .. 8 + C of a [B Nq, C + 24] sentinel buffer.  -> (O [B, Nq, C] device view, lse [B, heads, Nq], guard columns intact)."""
    flags = c.flags if flags is None else flags
    C = c.heads * c.dh
    Q = q.reshape(c.B * c.Nq, C).to(DEV)
    K, V = _pad_kv(k, c.kvs, k_fill), _pad_kv(v, c.kvs, v_fill)
    buf = torch.full((c.B * c.Nq, C + 24), ae.OUT_SENTINEL, dtype=torch.float16, device=DEV)
    _, lse = ops.attn_fwd(Q, K, V if flags & ae.ROWV else ops.transpose(V), c.B, c.heads, c.Nq, c.Nkv, c.kvs, c.dh, c.dh ** -0.5,
                          out=buf[:, 8:8 + C], want_lse=True, **_kw(flags))
    guard = bool((buf[:, :8] == ae.OUT_SENTINEL).all()) and bool((buf[:, 8 + C:] == ae.OUT_SENTINEL).all())
    return buf[:, 8:8 + C].reshape(c.B, c.Nq, C), lse, guard


def _worst_row(got, ref):
    d = (got.double() - ref).norm(dim=-1)
    i = int(d.argmax())
    return i // got.shape[1], i % got.shape[1]


def parity_fails(ops, c, cls, inputs, r, tag):
    """Runs case c on `inputs`, prints the [attn-fwd] line, -> the list of violated bounds (r: ae.emulate_forward of the inputs)."""
    o, lse, guard = run_forward(ops, c, *inputs)
    o, lse = o.cpu(), lse.cpu()
    d, d_row = ae.distances(o, r["o_exact"])
    d_lse = float((lse.double() - r["lse_exact"]).abs().max())
    lse_bound = 2 * r["D_lse"] + LSE_ROUNDINGS * float(r["lse_exact"].abs().max())
    print(f"[attn-fwd] {tag} {cls} variant={variant_of(ops, c)[0]} qpw={variant_of(ops, c)[1]}: E={r['E']:.3e} E_row={r['E_row']:.3e} "
          f"D_lse={r['D_lse']:.3e} kernel={d:.3e} kernel_row={d_row:.3e} kernel_lse={d_lse:.3e} ratio={d / r['E']:.3f} "
          f"ratio_row={d_row / r['E_row']:.3f} ratio_lse={d_lse / lse_bound * 2:.3f}")
    fails = []
    if not (bool(torch.isfinite(o).all()) and bool(torch.isfinite(lse).all())):
        fails.append("not finite")
    if not d <= 2 * r["E"]:
        fails.append(f"whole tensor {d:.3e} > 2 x {r['E']:.3e}")
    if not d_row <= 2 * r["E_row"]:
        fails.append(f"row {d_row:.3e} > 2 x {r['E_row']:.3e}, worst row (batch row, query) = {_worst_row(o, r['o_exact'])}")
    if not d_lse <= lse_bound:
        i = (lse.double() - r["lse_exact"]).abs().flatten().argmax()
        fails.append(f"lse {d_lse:.3e} > {lse_bound:.3e}, worst (batch row, head, query) = "
                     f"{tuple(int(x) for x in torch.unravel_index(i, lse.shape))}")
    if not guard:
        fails.append("guard columns of the O buffer were written")
    return fails


def onehot_probe(ops, g, expect=None):
    """The one-hot and the coded probe of geometry g over their sweeps (expect: another (variant, qpw) under an environment switch)."""
    assert variant_of(ops, g) == (expect or (g.variant, g.qpw)), f"{g.name}: skg_attn_fwd_variant reports {variant_of(ops, g)}"
    Q = ae.probe_q(g.dh, g.heads, g.Nq, g.B)
    for js, c in ae.probe_fwd_sweep(g.dh, g.Nkv):
        p = ae.probe_fwd_onehot(g, js, c, q=Q)
        o, lse, guard = run_forward(ops, g, p["q"], p["k"], p["v"])
        ae.probe_fwd_check(o, lse, p, f"one-hot probe {g.name} dh{g.dh} {g.Nq}x{g.Nkv} j*={js} c={c}")
        assert guard, f"{g.name}: guard columns written"
    for c in [c for c in ae.probe_cols(g.dh) if c < g.dh][:5 if g.B == ae.PROBE_B else 2]:
        p = ae.probe_fwd_coded(g, c, q=Q)
        o, lse, _ = run_forward(ops, g, p["q"], p["k"], p["v"])
        ae.probe_fwd_check(o, lse, p, f"coded probe {g.name} dh{g.dh} {g.Nq}x{g.Nkv} c={c}")


# ---------------------------------------------------------------------------------------------- parity against fp64
@functools.lru_cache(maxsize=None)
def _reference(name, cls):
    """Inputs, emulation and exact result of one case and class: computed once, shared, never written to."""
    return ae.emulate_case(ae.FWD_BY_NAME[name], cls)


@pytest.mark.parametrize("name,cls", ae.FWD_PARAMS)
def test_forward_parity(ops, name, cls):
    """The case runs the instantiation it names; O and lse are finite, O within 2 E of exact fp64 whole-tensor and 2 E_row per row, lse
    within 2 D_lse + 8 fp32 roundings of max |lse|; the guard columns of the O buffer keep their sentinel."""
    c = ae.FWD_BY_NAME[name]
    assert variant_of(ops, c) == (c.variant, c.qpw), f"{name}: skg_attn_fwd_variant reports {variant_of(ops, c)}"
    inputs, r = _reference(name, cls)
    fails = parity_fails(ops, c, cls, inputs, r, f"{name} dh{c.dh} h{c.heads} b{c.B} {c.Nq}x{c.Nkv}/{c.kvs}")
    assert not fails, f"{name} {cls}: " + "; ".join(fails)


# ---------------------------------------------------------------------------------------------- exact-answer probes
@pytest.mark.parametrize("g", ae.FWD_PROBES, ids=lambda g: g.name)
def test_forward_probes_onehot_and_coded(ops, g):
    """K = 0 (P uniform whatever Q is).  V one-hot on (key j*, column c): O[q][c] = (b + 1) / Nkv for every query, everything else exactly
    0, lse = ln Nkv - fails on a lost or doubled key tile, a pad key that leaks, a wrong key <-> k-slot map in the V read, a workgroup
    that covers the wrong queries.  V = key code in column c: O[q][c] = the mean code - fails on a ragged-tile mask off by one."""
    onehot_probe(ops, g)


@pytest.mark.parametrize("g", ae.FWD_CAUSAL_PROBES, ids=lambda g: g.name)
def test_forward_probes_causal(ops, g):
    """Causal, K = 0, V one-hot on (key j*, column c): O[i][c] = (b + 1) / (i + 1) from query j* on and exactly 0.0 before it,
    lse[i] = ln(i + 1) (ln Nkv behind the last key).  A mask off by one flips an exact zero or moves a denominator."""
    assert variant_of(ops, g) == (g.variant, g.qpw)
    Q = ae.probe_q(g.dh, g.heads, g.Nq, g.B)
    for js, c in ae.probe_fwd_sweep(g.dh, g.Nkv):
        p = ae.probe_fwd_causal(g, js, c, q=Q)
        o, lse, guard = run_forward(ops, g, p["q"], p["k"], p["v"])
        ae.probe_fwd_check(o, lse, p, f"causal probe {g.name} dh{g.dh} {g.Nq}x{g.Nkv} j*={js} c={c}")
        assert guard


# ---------------------------------------------------------------------------------------------- V forms, pad slots, repeatability
BOTH_FORMS = [c.name for c in ae.FWD_CASES if c.flags == ae.ROWV and c.variant // 1000 == 1 and c.kvs % 8 == 0]
FAMILIES = ["rowv40", "rowv64", "qt3_xcd", "short40_q512", "res10_40", "res15_40", "causal64_80"]


def test_case_lists_cover_the_families():
    assert {"qt3_xcd", "qt3_plain", "qt3_wave", "rowv32_t5", "rowv64_t5", "rowv40_t5", "rowv16", "rowv160"} <= set(BOTH_FORMS)
    v = {n: ae.FWD_BY_NAME[n] for n in FAMILIES}
    assert [v[n].variant for n in FAMILIES] == [1002, 1002, 1003, 3005, 3010, 3015, 2002] and v["short40_q512"].qpw == 512
    assert v["causal64_80"].Nq > v["causal64_80"].Nkv and all(v[n].kvs > v[n].Nkv for n in FAMILIES)


@pytest.mark.parametrize("name", BOTH_FORMS)
def test_both_v_forms_agree(ops, name):
    """Where both forms run the streaming kernel - also QT 3 and five key tiles - V^T and row-major V give the same bits: the same
    products in the same order, the fragments through ds_read_b64_tr_b16 instead of from a transposed copy."""
    c = ae.FWD_BY_NAME[name]
    assert variant_of(ops, c, ae.ROWV) == variant_of(ops, c, 0) == (c.variant, c.qpw)
    q, k, v = _reference(name, "unit")[0]
    o_r, lse_r, _ = run_forward(ops, c, q, k, v, flags=ae.ROWV)
    o_t, lse_t, _ = run_forward(ops, c, q, k, v, flags=0)
    assert torch.equal(o_r, o_t) and torch.equal(lse_r, lse_t)
    assert float(o_r.float().abs().max()) > 0


@pytest.mark.parametrize("name", FAMILIES)
def test_pad_slots_change_no_bit_forward(ops, name):
    """include/skg.h: key slots Nkv .. kv_stride - 1 are read and must hold finite values.  Pad rows zero against pad rows of 30.0 in K
    and 65504.0 in V: O and lse are bit-equal, in every kernel family."""
    c = ae.FWD_BY_NAME[name]
    q, k, v = _reference(name, "unit")[0]
    o0, lse0, _ = run_forward(ops, c, q, k, v, k_fill=0.0, v_fill=0.0)
    o1, lse1, _ = run_forward(ops, c, q, k, v, k_fill=30.0, v_fill=65504.0)
    assert bool(torch.isfinite(o1.float()).all()) and float(o0.float().abs().max()) > 0
    assert torch.equal(o0, o1) and torch.equal(lse0, lse1)


@pytest.mark.parametrize("name", FAMILIES)
def test_repeatable(ops, name):
    """The same call twice: identical bits (no launch-order dependence, no uninitialised register or LDS byte that reaches a result)."""
    c = ae.FWD_BY_NAME[name]
    q, k, v = _reference(name, "unit")[0]
    o0, lse0, _ = run_forward(ops, c, q, k, v)
    o1, lse1, _ = run_forward(ops, c, q, k, v)
    assert torch.equal(o0, o1) and torch.equal(lse0, lse1)


# ---------------------------------------------------------------------------------------------- the variants behind the switches
@pytest.mark.parametrize("env", [{"SKG_ATTN_VAR": "7"}, {"SKG_ATTN_VAR": "8"}, {"SKG_ATTN_VAR": "9"}, {"SKG_ATTN_VAR": "12"},
                                 {"SKG_NO_ATTN_SHORT": "1"}], ids=lambda e: "-".join(f"{k}={v}" for k, v in e.items()))
def test_env_variants(env):
    """The instantiations that ship behind SKG_ATTN_VAR (7: two register sets at dh 64, 8: QT 4 at dh 64 row-major, 9: QT 3 on small
    dh 40 launches, 12: QT 2 on large ones) and SKG_NO_ATTN_SHORT (77 keys on the streaming kernel): one child process each, which
    asserts the dispatch through the query and runs the unit parity and the one-hot probe on the dh 40 / 64 cases."""
    e = {k: v for k, v in os.environ.items() if k not in ("SKG_ATTN_VAR", "SKG_NO_ATTN_SHORT")}
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "_attn_var_check.py")], env=dict(e, **env),
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-6000:], r.stderr[-2000:])
    assert r.returncode == 0 and "ALL OK" in r.stdout
