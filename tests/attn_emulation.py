"""The attention forward and backward launches restated in fp64 with fp16 rounding exactly where the kernels round (plain torch, CPU).

Every rounding site below is taken from sketch2img_amd/csrc/attention.hip; where a description elsewhere disagrees with the kernel
source, the source wins.  What the kernels round (everything else is an fp32 MFMA accumulation, restated in fp64):

  forward (attn_fwd_kernel, attn_fwd_short_kernel)
    q~ = fp16(fp32(q) * fp32(scale * log2e))            one fp32 product, one fp16 rounding
    s  = q~ . k                                         log2 domain
    P  = fp16(exp2(s - m))                              into the P.V product; the denominator l sums the UNROUNDED exp2 - except in
                                                        the dh = 40 instantiation of attn_fwd_kernel, where l is a row of the P.V
                                                        MFMA (a ones column of V) and so sums the fp16 P (`denom_fp16`)
    O  = fp16((P . v) / l),  lse = fp32((log2 l + m) ln 2)
    (m: the row maximum in the short-key kernel; attn_fwd_kernel keeps a reference within 2^8 of it.  The emulation uses the
    maximum: another m moves the fp16 grid P is rounded on by less than one binade of the large probabilities.)
  delta (attn_delta_kernel, or the prologue of attn_bwd_dq_kernel):  delta = sum_d dO * O with the fp16 O
  dQ (attn_bwd_dq_kernel)
    P  = exp2(q~ . k - fp32(lse * log2e))               same q~ as the forward; P itself is not rounded here
    dS = fp16(P * (dO . v - delta)),  dQ = fp16((dS . k) * fp32(scale))
  dK / dV (attn_bwd_dkv_kernel)
    k~ = fp16(fp32(k) * fp32(scale * log2e)),  P = exp2(q . k~ - fp32(lse * log2e))         the UNROUNDED q
    dS = fp16(P * (dO . v - delta)),  dK = fp16((dS^T . q) * fp32(scale)),  dV = fp16(fp16(P)^T . dO)

`exact_forward` is softmax(q k^T scale) v in fp64 on the same fp16 inputs, `emulate_forward` the forward's emulation against it (E,
E_row as below, D_lse = max |lse - lse64|); `FWD_CASES` are the smallest launches that reach every instantiation skg_attn_fwd
dispatches to, each with the code skg_attn_fwd_variant must report for it, and three input classes (unit, peaked, selector).
`exact` is the closed form of the gradients of softmax(q k^T scale) v in fp64 on the same fp16 inputs.  `emulate` returns, per
output, the emulation, the exact value, E (whole-tensor relative distance of the emulation from exact) and E_row (max over the rows
of the [batch * N, heads * dh] tensor of ||row difference|| / rms row norm of the exact tensor): the kernels' own rounding noise,
against which the GPU tests bound the kernels (factor 2, the convention of tests/test_gpu_sat_train.py).

The module also holds the inputs the test files share: the parity cases (`SHAPES`, `FWD_CASES`, `case`) and the exact-answer probes
of the backward and of the forward."""
import collections
import math

import numpy as np
import torch

LOG2E32 = np.float32(1.4426950408889634)
LN2 = 0.6931471805599453

# (dh, heads, batch, Nq, Nkv): the smallest shapes that reach every tile position - workgroup tile 128 for dh <= 40 and 64 beyond,
# inner tile 64, residue 1 past a tile; heads * batch % 8 == 0 switches the XCD block map on
SHAPES = [(16, 4, 2, 129, 65), (32, 3, 3, 17, 129), (40, 4, 2, 129, 77), (40, 4, 2, 65, 193), (64, 3, 2, 65, 129),
          (80, 4, 2, 64, 65), (160, 3, 2, 45, 45), (160, 4, 2, 65, 96)]
MAGNITUDE_SHAPES = [(40, 4, 2, 129, 77), (160, 4, 2, 65, 96)]


def kv_stride_of(dh, Nkv):
    """ceil8(Nkv), except the 45-key case (the deepest level of a non-square map), which is dense."""
    return Nkv if (dh, Nkv) == (160, 45) else (Nkv + 7) // 8 * 8


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).half()


def case(dh, heads, B, Nq, Nkv, do_scale=1.0):
    """fp16 q [B, Nq, C], k, v [B, Nkv, C], dO [B, Nq, C] (unit normal, dO times a power of two: exact)."""
    C = heads * dh
    q, k, v = rnd(B, Nq, C, seed=1), rnd(B, Nkv, C, seed=2), rnd(B, Nkv, C, seed=3)
    do = (rnd(B, Nq, C, seed=4).float() * do_scale).half()
    return q, k, v, do


def _r16(x):
    return x.half().double()


def _heads(x, heads):
    B, N, C = x.shape
    return x.double().view(B, N, heads, C // heads).transpose(1, 2)        # [B, heads, N, dh]


def _rows(x):
    B, H, N, dh = x.shape
    return x.transpose(1, 2).reshape(B, N, H * dh)


def _prescale(x, scale):
    """fp16(fp32(x) * fp32(scale * log2e)) as the kernels form q~ / k~."""
    sc = torch.tensor(np.float32(scale) * LOG2E32, dtype=torch.float32)
    return (x.float() * sc).half()


def _nlse(lse):
    """minus lse in the log2 domain the way the backward kernels form it: fp32(-lse * log2e) of the fp32 lse."""
    return (-lse.float() * torch.tensor(LOG2E32)).double()


def forward(q, k, v, heads, scale, denom_fp16=False, causal=False):
    """-> (O fp16 [B, Nq, C], lse fp32 [B, heads, Nq]) as skg_attn_fwd stores them.  causal: key j > query i is masked before the
    maximum (the kernel writes -1e30 over the score: exp2 gives an exact 0)."""
    qt, kh, vh = _heads(_prescale(q, scale), heads), _heads(k, heads), _heads(v, heads)
    s = qt @ kh.transpose(-1, -2)
    if causal:
        s = s.masked_fill(_causal_mask(s.shape[-2], s.shape[-1]), float("-inf"))
    m = s.amax(-1, keepdim=True)
    e = torch.exp2(s - m)
    p16 = _r16(e)
    l = (p16 if denom_fp16 else e).sum(-1, keepdim=True)
    o = _rows((p16 @ vh) / l).half()
    lse = ((torch.log2(l) + m) * LN2).squeeze(-1).float()
    return o, lse


def delta_of(o, do, heads):
    """sum_d dO * O per (batch row, head, query) in fp64 -> [B, heads, Nq]."""
    return (_heads(o, heads) * _heads(do, heads)).sum(-1)


def bwd_dq(q, k, v, do, lse, delta, heads, scale):
    """skg_attn_bwd_dq -> (dQ fp16 [B, Nq, C], dS fp16 [B, heads, Nq, Nkv])."""
    qt, kh, vh, dh_ = _heads(_prescale(q, scale), heads), _heads(k, heads), _heads(v, heads), _heads(do, heads)
    p = torch.exp2(qt @ kh.transpose(-1, -2) + _nlse(lse)[..., None])
    ds = (p * (dh_ @ vh.transpose(-1, -2) - delta.double()[..., None])).half()
    dq = _rows((ds.double() @ kh) * float(np.float32(scale))).half()
    return dq, ds


def bwd_dkv(q, k, v, do, lse, delta, heads, scale):
    """skg_attn_bwd_dkv -> (dK, dV fp16 [B, Nkv, C], dS fp16 [B, heads, Nq, Nkv])."""
    qh, kt, vh, dh_ = _heads(q, heads), _heads(_prescale(k, scale), heads), _heads(v, heads), _heads(do, heads)
    p = torch.exp2(qh @ kt.transpose(-1, -2) + _nlse(lse)[..., None])
    ds = (p * (dh_ @ vh.transpose(-1, -2) - delta.double()[..., None])).half()
    dk = _rows((ds.double().transpose(-1, -2) @ qh) * float(np.float32(scale))).half()
    dv = _rows(_r16(p).transpose(-1, -2) @ dh_).half()
    return dk, dv, ds


def exact(q, k, v, do, heads, scale):
    """fp64 closed form of the gradients of softmax(q k^T scale) v on the same fp16 inputs -> dict of [B, N, C] fp64 tensors."""
    qh, kh, vh, dh_ = (_heads(t, heads) for t in (q, k, v, do))
    p = torch.softmax(qh @ kh.transpose(-1, -2) * scale, dim=-1)
    o = p @ vh
    ds = p * (dh_ @ vh.transpose(-1, -2) - (dh_ * o).sum(-1, keepdim=True))
    return {"dq": _rows(ds @ kh * scale), "dk": _rows(ds.transpose(-1, -2) @ qh * scale), "dv": _rows(p.transpose(-1, -2) @ dh_)}


def distances(got, ref):
    """(whole-tensor ||got - ref|| / ||ref||, max over rows of ||row difference|| / rms row norm of ref), rows of [B * N, C]."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    got, ref = got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1])
    rms = float(ref.pow(2).sum(-1).mean().sqrt())
    return float((got - ref).norm() / ref.norm()), float((got - ref).norm(dim=-1).max()) / rms


def emulate(q, k, v, do, heads, scale, denom_fp16=False):
    """The three launches on one set of inputs.  -> {"dq" | "dk" | "dv": dict(emu=fp16, exact=fp64, E=, E_row=)}, plus "o", "lse",
    "delta" of the emulated forward."""
    o, lse = forward(q, k, v, heads, scale, denom_fp16)
    delta = delta_of(o, do, heads)
    dq, _ = bwd_dq(q, k, v, do, lse, delta, heads, scale)
    dk, dv, _ = bwd_dkv(q, k, v, do, lse, delta, heads, scale)
    ex = exact(q, k, v, do, heads, scale)
    out = {"o": o, "lse": lse, "delta": delta}
    for name, emu in (("dq", dq), ("dk", dk), ("dv", dv)):
        E, E_row = distances(emu, ex[name])
        out[name] = dict(emu=emu, exact=ex[name], E=E, E_row=E_row)
    return out


# ---------------------------------------------------------------------------------------------- exact-answer probes
# One-hot / coded operands whose gradients have a closed form; lse = ln Nkv and delta are supplied analytically, so a wrong answer
# points at the backward kernel.  PROBE_S, the value of the one-hot dO: the smallest dS of any probe is s / Nkv^2 (200 keys: s /
# 40000), which is a normal fp16 number (>= 2^-14) from s = 4 on; 2^12 = LOSS_SCALE / 2 leaves ten binades below and keeps the
# largest (s / 77 = 53) and every stored gradient far inside the range.
PROBE_S = 4096.0
PROBE_CONFIGS = [(40, 8), (64, 5), (160, 8)]           # (dh, heads), B = 2
PROBE_GEOMETRIES = [(200, 77, 80), (77, 200, 208)]     # (Nq, Nkv, kv_stride)
PROBE_B = 2
K_PAD, V_PAD, OUT_SENTINEL = 30.0, 7.0, -5.0
PROBE_TOL = 2e-3


def probe_queries(Nq):
    return sorted({x for x in (0, 15, 16, 31, 47, 63, 64, 127, 128) if x < Nq} | {Nq - 1})


def probe_keys(Nkv):
    return sorted({x for x in (0, 15, 16, 63, 64, 76, 127, 128, 199) if x < Nkv})


def probe_cols(dh):
    return [0, 7, 16, 33, dh - 1]


def probe_q(dh, heads, Nq, B=PROBE_B):
    """The probes' random Q: magnitudes in [0.5, 2), random signs, so that no expected dK element is near the fp16 subnormals."""
    g = torch.Generator().manual_seed(11)
    C = heads * dh
    mag = 0.5 + 1.5 * torch.rand(B, Nq, C, generator=g)
    sign = torch.where(torch.rand(B, Nq, C, generator=g) < 0.5, -1.0, 1.0)
    return (mag * sign).half()


def key_code(Nkv):
    return (torch.arange(Nkv) % 13 + 1).double()


def _one_hot(B, N, heads, dh, row, col, value):
    """[B, N, C] fp16, `value * (b + 1)` at (row, column col of every head) of batch row b."""
    x = torch.zeros(B, N, heads, dh, dtype=torch.float16)
    for b in range(B):
        x[b, row, :, col] = value * (b + 1)
    return x.view(B, N, heads * dh)


def probe_lse(heads, Nq, Nkv):
    return torch.full((PROBE_B, heads, Nq), math.log(Nkv), dtype=torch.float32)


def probe_dv(dh, heads, Nq, Nkv, qs, c, q=None):
    """K = 0 (uniform P), V = 0, dO one-hot (query qs, column c).  dV[j][c] = s / Nkv for every key, every other column 0; dK = 0."""
    q = probe_q(dh, heads, Nq) if q is None else q
    C = heads * dh
    k, v = torch.zeros(PROBE_B, Nkv, C, dtype=torch.float16), torch.zeros(PROBE_B, Nkv, C, dtype=torch.float16)
    do = _one_hot(PROBE_B, Nq, heads, dh, qs, c, PROBE_S)
    delta = torch.zeros(PROBE_B, heads, Nq, dtype=torch.float32)
    want = torch.zeros(PROBE_B, Nkv, heads, dh, dtype=torch.float64)
    for b in range(PROBE_B):
        want[b, :, :, c] = PROBE_S * (b + 1) / Nkv
    return dict(q=q, k=k, v=v, do=do, lse=probe_lse(heads, Nq, Nkv), delta=delta, dv=want.view(PROBE_B, Nkv, C),
                dk=torch.zeros(PROBE_B, Nkv, C, dtype=torch.float64))


def _probe_delta(heads, Nq, Nkv, qs):
    """V one-hot (value 1) and dO one-hot in the same column: O[q][c] = 1 / Nkv for every query, delta[qs] = s / Nkv."""
    delta = torch.zeros(PROBE_B, heads, Nq, dtype=torch.float32)
    for b in range(PROBE_B):
        delta[b, :, qs] = PROBE_S * (b + 1) / Nkv
    return delta


def probe_dk(dh, heads, Nq, Nkv, qs, js, c, q=None):
    """K = 0, V one-hot (key js, column c), dO one-hot (query qs, column c): dK[j] = scale (1 / Nkv)(delta_{j js} - 1 / Nkv) s Q[qs]."""
    q = probe_q(dh, heads, Nq) if q is None else q
    C = heads * dh
    k = torch.zeros(PROBE_B, Nkv, C, dtype=torch.float16)
    v = torch.zeros(PROBE_B, Nkv, heads, dh, dtype=torch.float16)
    v[:, js, :, c] = 1.0
    do = _one_hot(PROBE_B, Nq, heads, dh, qs, c, PROBE_S)
    hot = torch.zeros(Nkv, dtype=torch.float64)
    hot[js] = 1.0
    want = torch.stack([dh ** -0.5 * (PROBE_S * (b + 1) / Nkv) * (hot - 1.0 / Nkv)[:, None] * q[b, qs].double()[None, :]
                        for b in range(PROBE_B)])
    return dict(q=q, k=k, v=v.view(PROBE_B, Nkv, C), do=do, lse=probe_lse(heads, Nq, Nkv), delta=_probe_delta(heads, Nq, Nkv, qs),
                dk=want)


def probe_dq(dh, heads, Nq, Nkv, qs, js, c, col):
    """Q = 0 (uniform P whatever K is), K = code_j in column col, V one-hot (key js, column c), dO one-hot (query qs, column c):
    dQ[qs][col] = scale (s / Nkv)(code_js - mean code), everything else 0."""
    C = heads * dh
    code = key_code(Nkv)
    q = torch.zeros(PROBE_B, Nq, C, dtype=torch.float16)
    k = torch.zeros(PROBE_B, Nkv, heads, dh, dtype=torch.float16)
    k[:, :, :, col] = code.half()[None, :, None]
    v = torch.zeros(PROBE_B, Nkv, heads, dh, dtype=torch.float16)
    v[:, js, :, c] = 1.0
    do = _one_hot(PROBE_B, Nq, heads, dh, qs, c, PROBE_S)
    want = torch.zeros(PROBE_B, Nq, heads, dh, dtype=torch.float64)
    for b in range(PROBE_B):
        want[b, qs, :, col] = dh ** -0.5 * (PROBE_S * (b + 1) / Nkv) * float(code[js] - code.mean())
    return dict(q=q, k=k.view(PROBE_B, Nkv, C), v=v.view(PROBE_B, Nkv, C), do=do, lse=probe_lse(heads, Nq, Nkv),
                delta=_probe_delta(heads, Nq, Nkv, qs), dq=want.view(PROBE_B, Nq, C))


def probe_sweep(kind, dh, Nq, Nkv):
    """The (qs, js, c, col) tuples of one probe: every query position x every key position; the columns cycle so that each of the
    five appears in every role and against queries and keys of different tiles."""
    cols = probe_cols(dh)
    qs_, js_ = probe_queries(Nq), probe_keys(Nkv)
    if kind == "dv":
        return [(qs, None, c, None) for qs in qs_ for c in cols]
    out = []
    for a, qs in enumerate(qs_):
        for b, js in enumerate(js_):
            i = a * len(js_) + b
            out.append((qs, js, cols[i % 5], cols[(i // 5 + 2 * i) % 5]))
    return out


def probe_check(got, want, what, tol=PROBE_TOL):
    """Analytic zeros exactly 0.0; the rest within PROBE_TOL of the expected value (one fp16 rounding of dS, one of the store)."""
    got = got.detach().double()
    want = want.double().to(got.device)
    zero = want == 0
    stray = zero & (got != 0)
    assert not bool(stray.any()), (f"{what}: {int(stray.sum())} analytic zeros are not 0.0, first at {tuple(int(i) for i in stray.nonzero()[0])}: "
                                   f"got {float(got[stray][0])}")
    bad = (got - want).abs() > tol * want.abs()
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} elements off, first at {tuple(int(i) for i in bad.nonzero()[0])}: "
                                 f"got {float(got[bad][0])} want {float(want[bad][0])}")


# ---------------------------------------------------------------------------------------------- forward: parity cases
# skg_attn_fwd picks its instantiation from the size of the launch (attention.hip: attn_fwd_plan), so every case names the code
# skg_attn_fwd_variant must report for it (1000 + QT streaming, 2000 + QT causal, 3000 + NT LDS-resident) and the queries one
# workgroup covers; a case that lands elsewhere is a failed test.
CAUSAL, ROWV, RESIDENT = 1, 2, 4               # include/skg.h SKG_ATTN_*
FwdCase = collections.namedtuple("FwdCase", "name dh heads B Nq Nkv kvs flags classes variant qpw")
_UP, _UPS, _U, _US = ("unit", "peaked"), ("unit", "peaked", "selector"), ("unit",), ("unit", "selector")
FWD_CASES = [FwdCase(*c) for c in [
    # -- streaming kernel, row-major V: the geometry of SHAPES where it stays on this kernel (a residue of 1 past the 128 / 64-query
    #    workgroup, a ragged last key tile), 80 head columns with more than 80 key slots, 257 keys = five key tiles
    ("rowv16", 16, 4, 2, 129, 65, 72, ROWV, _UPS, 1002, 128),
    ("rowv32", 32, 3, 3, 17, 129, 136, ROWV, _UPS, 1002, 128),
    ("rowv40", 40, 4, 2, 65, 193, 200, ROWV, _UPS, 1002, 128),
    ("rowv64", 64, 3, 2, 65, 129, 136, ROWV, _UPS, 1002, 128),            # the 2 | (3 << 2) instantiation (one register set)
    ("rowv80", 80, 4, 2, 65, 129, 136, ROWV, _UPS, 1002, 128),
    ("rowv160", 160, 4, 2, 65, 96, 96, ROWV, _UP, 1001, 64),
    ("rowv32_t5", 32, 3, 2, 129, 257, 264, ROWV, _UPS, 1002, 128),        # DEEP: the two-register-set ring wraps
    ("rowv64_t5", 64, 3, 2, 129, 257, 264, ROWV, _US, 1002, 128),
    ("rowv40_t5", 40, 4, 2, 129, 257, 264, ROWV, _US, 1002, 128),
    # -- streaming kernel, V^T (kv_stride % 8 == 0)
    ("vt16", 16, 4, 2, 129, 65, 72, 0, _UP, 1002, 128),
    ("vt32", 32, 3, 3, 17, 129, 136, 0, _UP, 1002, 128),
    ("vt40_77", 40, 4, 2, 129, 77, 80, 0, _UPS, 1002, 128),               # the ONES path at <= 80 keys
    ("vt40", 40, 4, 2, 65, 193, 200, 0, _UP, 1002, 128),
    ("vt64", 64, 3, 2, 65, 129, 136, 0, _UP, 1002, 128),
    ("vt80", 80, 4, 2, 64, 65, 72, 0, _UPS, 1002, 128),
    ("vt160", 160, 4, 2, 65, 96, 96, 0, _UP, 1001, 64),
    ("vt80_t5", 80, 4, 2, 65, 257, 264, 0, _US, 1002, 128),               # DEEP
    ("vt16_t5", 16, 4, 2, 129, 257, 264, 0, _US, 1002, 128),
    # -- QT 3 (dh 40, >= 1024 workgroups of 192 queries) with no environment variable.  1537 = 8 * 192 + 1: the last workgroup
    #    holds one query; 1585 = 8 * 192 + 49: its wave 1 starts at query 48
    ("qt3_xcd", 40, 8, 16, 1537, 193, 200, ROWV, _US, 1003, 192),         # 128 pairs: XCD block map on
    ("qt3_xcd_vt", 40, 8, 16, 1537, 193, 200, 0, _U, 1003, 192),
    ("qt3_plain", 40, 5, 26, 1537, 129, 136, ROWV, _U, 1003, 192),        # 130 pairs: XCD map off
    ("qt3_wave", 40, 8, 16, 1585, 129, 136, ROWV, _U, 1003, 192),
    # -- short-key kernel (row-major V, <= 80 key slots): query chunks 64, 192 (three tiles per wave, last chunk one query), 512
    ("short40_q64", 40, 4, 2, 129, 77, 80, ROWV, _UPS, 3005, 64),
    ("short40_q192", 40, 8, 16, 1537, 77, 80, ROWV, _US, 3005, 192),
    ("short40_q512", 40, 8, 16, 4097, 77, 80, ROWV, _U, 3005, 512),
    ("short64_q128", 64, 5, 16, 1537, 77, 80, ROWV, _US, 3005, 128),
    ("short80_q128", 80, 4, 16, 2049, 77, 80, ROWV, _U, 3005, 128),
    ("short160_q128", 160, 3, 8, 2817, 77, 80, ROWV, _U, 3005, 128),
    ("short160_k45", 160, 3, 2, 45, 45, 45, ROWV, _UP, 3005, 64),         # <= 64 keys (the short_rows mask), dense, no multiple of 8
    ("short40_k50", 40, 8, 2, 200, 50, 56, ROWV, _UPS, 3005, 64),
    ("short40_k80", 40, 4, 2, 129, 80, 80, ROWV, _UPS, 3005, 64),         # no dead register
    # -- LDS-resident kernel behind the flag: NT 10 (150 keys: tile 9 ragged; 160: none) and NT 15 (231 keys in 232 slots;
    #    200: tile 12 ragged, tiles 13 and 14 dead)
    ("res10_40", 40, 4, 2, 129, 150, 152, ROWV | RESIDENT, _UPS, 3010, 128),
    ("res10_64", 64, 3, 2, 129, 160, 160, ROWV | RESIDENT, _UPS, 3010, 128),
    ("res10_80", 80, 4, 2, 129, 150, 152, ROWV | RESIDENT, _UPS, 3010, 128),
    ("res10_160", 160, 3, 2, 129, 160, 160, ROWV | RESIDENT, _UP, 3010, 128),
    ("res10_40_q256", 40, 8, 16, 2049, 150, 152, ROWV | RESIDENT, _U, 3010, 256),
    ("res15_40", 40, 4, 2, 129, 231, 232, ROWV | RESIDENT, _UPS, 3015, 128),
    ("res15_64", 64, 3, 2, 129, 231, 232, ROWV | RESIDENT, _UPS, 3015, 128),
    ("res15_80", 80, 4, 2, 129, 231, 232, ROWV | RESIDENT, _UPS, 3015, 128),
    ("res15_40_q192", 40, 8, 16, 1537, 200, 200, ROWV | RESIDENT, _U, 3015, 192),
    ("res_160_stream", 160, 3, 2, 65, 231, 232, ROWV | RESIDENT, _UP, 1001, 64),      # does not fit the LDS: runs as without the flag
    # -- causal (V^T): 80 rows / 77 keys (the text encoder), a residue of 1 with two key tiles, 257 keys in 264 rows (five tiles)
    ("causal16_80", 16, 4, 2, 80, 77, 80, CAUSAL, _UP, 2002, 128),
    ("causal32_80", 32, 3, 2, 80, 77, 80, CAUSAL, _UP, 2002, 128),
    ("causal64_80", 64, 3, 2, 80, 77, 80, CAUSAL, _UP, 2002, 128),
    ("causal16_129", 16, 4, 2, 129, 129, 136, CAUSAL, _UP, 2002, 128),
    ("causal32_129", 32, 3, 2, 129, 129, 136, CAUSAL, _UP, 2002, 128),
    ("causal64_129", 64, 3, 2, 129, 129, 136, CAUSAL, _UP, 2002, 128),
    ("causal16_264", 16, 4, 2, 264, 257, 264, CAUSAL, _UP, 2002, 128),
    ("causal32_264", 32, 3, 2, 264, 257, 264, CAUSAL, _UP, 2002, 128),
    ("causal64_264", 64, 3, 2, 264, 257, 264, CAUSAL, _UP, 2002, 128),
]]
FWD_BY_NAME = {c.name: c for c in FWD_CASES}
FWD_PARAMS = [(c.name, cls) for c in FWD_CASES for cls in c.classes]
# every product instantiation of skg_attn_fwd as (variant, dh, V row-major): what the table has to reach
FWD_REQUIRED = ({(1002, d, r) for d in (16, 32, 40, 64, 80) for r in (False, True)} | {(1001, 160, False), (1001, 160, True)} |
                {(1003, 40, False), (1003, 40, True)} | {(2002, d, False) for d in (16, 32, 64)} |
                {(3005, d, True) for d in (40, 64, 80, 160)} | {(3010, d, True) for d in (40, 64, 80, 160)} |
                {(3015, d, True) for d in (40, 64, 80)})
SELECTOR_K, SELECTOR_Q, SELECTOR_COLS = 8.0, 1.0, 8


def fwd_denom_fp16(variant, dh):
    """The denominator sums the fp16 P exactly in the dh = 40 instantiations of attn_fwd_kernel (ONES: l is a row of the P.V MFMA),
    whatever the key count and the V form; the LDS-resident kernel sums the unrounded exp2."""
    return variant // 1000 == 1 and dh == 40


def selector_keys(B, Nkv):
    """The dominant key of every batch row: first key tile for row 0, a middle tile for row 1, the last (ragged) tile for the rest."""
    nt = (Nkv + 63) // 64
    return [3 if b == 0 else min(64 * (nt // 2) + 5, Nkv - 1) if b == 1 else max(Nkv - 2, 64 * (nt - 1)) for b in range(B)]


def fwd_inputs(c, cls):
    """fp16 q [B, Nq, C], k, v [B, Nkv, C] of one case and input class (fixed seeds)."""
    q, k, v, _ = case(c.dh, c.heads, c.B, c.Nq, c.Nkv)
    if cls == "unit":
        return q, k, v
    if cls == "peaked":                         # scores with sigma ~ 4 nat: a few keys dominate (x 4 is exact in fp16)
        return (q.float() * 4.0).half(), k, v
    assert cls == "selector"
    # K = 0 except one key per batch row with 8.0 in the first 8 columns of every head, Q = 1.0 there: that key's score is
    # 64 scale log2e in the log2 domain, every other one exactly 0 - the streaming kernel re-bases its reference maximum at the
    # tile that holds the key (tile 0, a middle one, the last one) and nowhere else
    qs = torch.zeros(c.B, c.Nq, c.heads, c.dh, dtype=torch.float16)
    qs[..., :SELECTOR_COLS] = SELECTOR_Q
    ks = torch.zeros(c.B, c.Nkv, c.heads, c.dh, dtype=torch.float16)
    for b, js in enumerate(selector_keys(c.B, c.Nkv)):
        ks[b, js, :, :SELECTOR_COLS] = SELECTOR_K
    return qs.view(c.B, c.Nq, -1), ks.view(c.B, c.Nkv, -1), v


def _causal_mask(Nq, Nkv):
    return torch.arange(Nkv)[None, :] > torch.arange(Nq)[:, None]


def exact_forward(q, k, v, heads, scale, causal=False):
    """fp64 softmax(q k^T scale) v on the same fp16 inputs -> (O [B, Nq, C], lse [B, heads, Nq])."""
    qh, kh, vh = (_heads(t, heads) for t in (q, k, v))
    s = qh @ kh.transpose(-1, -2) * scale
    if causal:
        s = s.masked_fill(_causal_mask(s.shape[-2], s.shape[-1]), float("-inf"))
    return _rows(torch.softmax(s, dim=-1) @ vh), torch.logsumexp(s, dim=-1)


def emulate_forward(q, k, v, heads, scale, causal=False, denom_fp16=False):
    """-> dict(o_emu fp16, o_exact fp64, E, E_row (`distances`), lse_emu fp32, lse_exact fp64, D_lse = max |lse_emu - lse_exact|)."""
    o, lse = forward(q, k, v, heads, scale, denom_fp16, causal)
    oe, le = exact_forward(q, k, v, heads, scale, causal)
    E, E_row = distances(o, oe)
    return dict(o_emu=o, o_exact=oe, E=E, E_row=E_row, lse_emu=lse, lse_exact=le, D_lse=float((lse.double() - le).abs().max()))


def emulate_case(c, cls):
    q, k, v = fwd_inputs(c, cls)
    return (q, k, v), emulate_forward(q, k, v, c.heads, c.dh ** -0.5, bool(c.flags & CAUSAL), fwd_denom_fp16(c.variant, c.dh))


def selector_margin(c):
    """log2-domain distance of the selector key's score from every other key's, from fp64 scores on the selector inputs (min over rows)."""
    q, k, _ = fwd_inputs(c, "selector")
    s = _heads(q, c.heads) @ _heads(k, c.heads).transpose(-1, -2) * (c.dh ** -0.5 * 1.4426950408889634)
    top = s.topk(2, dim=-1).values
    return float((top[..., 0] - top[..., 1]).min())


# ---------------------------------------------------------------------------------------------- forward: exact-answer probes
# K = 0: every probability is exactly 1, the denominator the exact integer Nkv (causal: i + 1) and the numerator exact in fp32, so a
# stored value is one fp32 reciprocal and one fp16 rounding from the closed form: one fp16 unit in the last place (2^-10 relative);
# lse within 4 fp32 units of ln n.  (name, dh, heads, B, Nq, Nkv, kvs, flags, variant, qpw); batch row b carries (b + 1) x.
FWD_PROBE_TOL = 2.0 ** -10
FwdProbe = collections.namedtuple("FwdProbe", "name dh heads B Nq Nkv kvs flags variant qpw")
FWD_PROBES = [FwdProbe(*g) for g in [
    ("rowv16", 16, 4, 2, 200, 77, 80, ROWV, 1002, 128), ("rowv32", 32, 3, 2, 77, 200, 208, ROWV, 1002, 128),
    ("rowv40", 40, 8, 2, 77, 200, 208, ROWV, 1002, 128), ("vt40", 40, 8, 2, 200, 77, 80, 0, 1002, 128),
    ("rowv64", 64, 5, 2, 77, 200, 208, ROWV, 1002, 128), ("vt64", 64, 5, 2, 200, 77, 80, 0, 1002, 128),
    ("rowv80", 80, 4, 2, 77, 200, 208, ROWV, 1002, 128), ("vt80", 80, 4, 2, 200, 77, 80, 0, 1002, 128),
    ("rowv160", 160, 8, 2, 77, 200, 208, ROWV, 1001, 64), ("vt160", 160, 8, 2, 200, 77, 80, 0, 1001, 64),
    ("qt3", 40, 8, 16, 1537, 1537, 1537, ROWV, 1003, 192),
    ("short40", 40, 8, 2, 200, 77, 80, ROWV, 3005, 64), ("short64", 64, 5, 2, 200, 77, 80, ROWV, 3005, 64),
    ("short80", 80, 4, 2, 200, 77, 80, ROWV, 3005, 64), ("short160", 160, 8, 2, 200, 77, 80, ROWV, 3005, 64),
    ("short40_q512", 40, 8, 16, 4097, 77, 80, ROWV, 3005, 512),
    ("res10_40", 40, 8, 2, 200, 150, 152, ROWV | RESIDENT, 3010, 128), ("res10_160", 160, 8, 2, 200, 150, 152, ROWV | RESIDENT, 3010, 128),
    ("res15_64", 64, 5, 2, 77, 200, 208, ROWV | RESIDENT, 3015, 128), ("res15_80", 80, 4, 2, 200, 231, 232, ROWV | RESIDENT, 3015, 128),
]]
FWD_CAUSAL_PROBES = [FwdProbe(*g) for g in [
    ("causal16", 16, 4, 2, 200, 200, 200, CAUSAL, 2002, 128), ("causal32", 32, 3, 2, 80, 77, 80, CAUSAL, 2002, 128),
    ("causal64", 64, 5, 2, 200, 200, 200, CAUSAL, 2002, 128), ("causal64_264", 64, 3, 2, 264, 257, 264, CAUSAL, 2002, 128),
]]


def probe_fwd_keys(Nkv):
    """probe_keys plus the last key, and the positions around the 192-query / 192-key marks and key 1536 of the QT 3 launch."""
    return sorted(set(probe_keys(Nkv)) | {x for x in (191, 192, 1536) if x < Nkv} | {Nkv - 1})


def probe_fwd_sweep(dh, Nkv):
    """(js, c): every key position once, the columns cycling (each of the five appears: there are at least six key positions)."""
    cols = [c for c in probe_cols(dh) if c < dh]
    return [(js, cols[i % len(cols)]) for i, js in enumerate(probe_fwd_keys(Nkv))]


def _probe_fwd_lse(g, causal=False):
    n = torch.arange(1, g.Nq + 1).clamp(max=g.Nkv).double() if causal else torch.full((g.Nq,), float(g.Nkv), dtype=torch.float64)
    return n.log()[None, None, :].expand(g.B, g.heads, g.Nq)


def probe_fwd_onehot(g, js, c, q=None):
    """K = 0, any Q, V one-hot (key js, column c of every head, value b + 1): O[q][c] = (b + 1) / Nkv for every query, every other
    element exactly 0, lse = ln Nkv."""
    C = g.heads * g.dh
    q = probe_q(g.dh, g.heads, g.Nq, g.B) if q is None else q
    v = _one_hot(g.B, g.Nkv, g.heads, g.dh, js, c, 1.0)
    want = torch.zeros(g.B, g.Nq, g.heads, g.dh, dtype=torch.float64)
    for b in range(g.B):
        want[b, :, :, c] = (b + 1) / g.Nkv
    return dict(q=q, k=torch.zeros(g.B, g.Nkv, C, dtype=torch.float16), v=v, o=want.view(g.B, g.Nq, C), lse=_probe_fwd_lse(g))


def probe_fwd_coded(g, c, q=None):
    """K = 0, V = (b + 1) code_j in column c: O[q][c] = (b + 1) mean code, every other element exactly 0.  A lost or doubled key, or
    a ragged-tile mask off by one, moves the mean."""
    C = g.heads * g.dh
    q = probe_q(g.dh, g.heads, g.Nq, g.B) if q is None else q
    code = key_code(g.Nkv)
    v = torch.zeros(g.B, g.Nkv, g.heads, g.dh, dtype=torch.float16)
    want = torch.zeros(g.B, g.Nq, g.heads, g.dh, dtype=torch.float64)
    for b in range(g.B):
        v[b, :, :, c] = ((b + 1) * code).half()[:, None]
        want[b, :, :, c] = (b + 1) * float(code.mean())
    return dict(q=q, k=torch.zeros(g.B, g.Nkv, C, dtype=torch.float16), v=v.view(g.B, g.Nkv, C), o=want.view(g.B, g.Nq, C),
                lse=_probe_fwd_lse(g))


def probe_fwd_causal(g, js, c, q=None):
    """Causal, K = 0, V one-hot (key js, column c, value b + 1): query i sees keys 0 .. min(i, Nkv - 1), so O[i][c] = (b + 1) / (i + 1)
    for i >= js (/ Nkv from query Nkv on) and exactly 0 for i < js; lse[i] = ln(i + 1).  A mask off by one flips an exact zero."""
    p = probe_fwd_onehot(g, js, c, q)
    n = torch.arange(1, g.Nq + 1).clamp(max=g.Nkv).double()
    want = torch.zeros(g.B, g.Nq, g.heads, g.dh, dtype=torch.float64)
    for b in range(g.B):
        want[b, js:, :, c] = ((b + 1) / n[js:])[:, None]
    p.update(o=want.view(g.B, g.Nq, g.heads * g.dh), lse=_probe_fwd_lse(g, causal=True))
    return p


def probe_fwd_check(o, lse, p, what):
    """O: analytic zeros exactly 0.0, the rest within one fp16 unit in the last place; lse within 4 fp32 units of ln n.  The message
    names the first wrong (batch row, query, column) / (batch row, head, query)."""
    probe_check(o, p["o"], f"{what} O", tol=FWD_PROBE_TOL)
    got = lse.detach().double()
    want, ulp = p["lse"].to(got.device), torch.from_numpy(np.spacing(p["lse"].float().numpy())).double().to(got.device)
    bad = (got - want).abs() > 4 * ulp
    assert not bool(bad.any()), (f"{what} lse: {int(bad.sum())} entries off, first at (b, head, query) = "
                                 f"{tuple(int(i) for i in bad.nonzero()[0])}: got {float(got[bad][0])} want {float(want[bad][0])}")
