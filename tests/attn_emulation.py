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

`exact` is the closed form of the gradients of softmax(q k^T scale) v in fp64 on the same fp16 inputs.  `emulate` returns, per
output, the emulation, the exact value, E (whole-tensor relative distance of the emulation from exact) and E_row (max over the rows
of the [batch * N, heads * dh] tensor of ||row difference|| / rms row norm of the exact tensor): the kernels' own rounding noise,
against which the GPU tests bound the kernels (factor 2, the convention of tests/test_gpu_sat_train.py).

The module also holds the inputs both test files share: the parity cases (`SHAPES`, `case`) and the exact-answer probes."""
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


def forward(q, k, v, heads, scale, denom_fp16=False):
    """-> (O fp16 [B, Nq, C], lse fp32 [B, heads, Nq]) as skg_attn_fwd stores them."""
    qt, kh, vh = _heads(_prescale(q, scale), heads), _heads(k, heads), _heads(v, heads)
    s = qt @ kh.transpose(-1, -2)
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


def probe_q(dh, heads, Nq):
    """The probes' random Q: magnitudes in [0.5, 2), random signs, so that no expected dK element is near the fp16 subnormals."""
    g = torch.Generator().manual_seed(11)
    C = heads * dh
    mag = 0.5 + 1.5 * torch.rand(PROBE_B, Nq, C, generator=g)
    sign = torch.where(torch.rand(PROBE_B, Nq, C, generator=g) < 0.5, -1.0, 1.0)
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


def probe_check(got, want, what):
    """Analytic zeros exactly 0.0; the rest within PROBE_TOL of the expected value (one fp16 rounding of dS, one of the store)."""
    got, want = got.detach().double().cpu(), want.double()
    zero = want == 0
    assert bool((got[zero] == 0).all()), f"{what}: {int((got[zero] != 0).sum())} analytic zeros are not 0.0"
    bad = (got - want).abs() > PROBE_TOL * want.abs()
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} elements off, first at {tuple(int(i) for i in bad.nonzero()[0])}: "
                                 f"got {float(got[bad][0])} want {float(want[bad][0])}")
