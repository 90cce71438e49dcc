"""References, fp32 emulations, bounds and input draws for the normalisation-kernel probes (test_host_norm_probes.py on the CPU,
test_gpu_norm_probes.py on the device).  Plain numpy in float64 / float32: no GPU code, no project kernels.

Layout everywhere: token-major fp16 [rows * HW, C] (NHWC), as the kernels read it.  LayerNorm over [M, C] is the GroupNorm of
(rows = M, HW = 1, groups = 1) with per-channel gamma / beta, so the GroupNorm functions serve both.

Three layers
  * ref_*   fp64, from the fp16 values (pair inputs: hi + lo), returning every intermediate.
  * emu_*   the kernel's FORMULA in fp32 (uncentred s2/n - mean^2 with a clamp where the kernel does that, centred where it is
            centred; a = rstd * gamma, sh = beta - mean * a, y = fma(x, a, sh) where the kernel does that), NOT its thread layout:
            sums run sequentially within a chunk and then sequentially over the chunks - a worse order than any kernel's tree.
  * bounds  built from the reference's own magnitudes; their constants C_M, C_R, K_FWD, K_BWD, C_P are 4 x the largest ratio the
            EMULATION reaches over CASES below (calibrate(); test_host_norm_probes.py checks the recorded numbers against it).
            No tolerance comes from a kernel's output.

Pair inputs on the chunked GroupNorm paths: the kernels take the statistics of the hi part by design (norms.hip, gn_apply_kernel) and
apply them to hi + lo; the reference does the same (`stats_of="hi"`), the small path and LayerNorm use the sum.
"""
from dataclasses import dataclass, field

import numpy as np

U = 2.0 ** -24                    # fp32 unit roundoff
H_RND, H_SUB = 2.0 ** -11, 2.0 ** -25      # one fp16 rounding: normal (relative), subnormal (absolute: half of 2^-24)
SILU_GRAD_MAX = 1.1               # max |silu'| = 1.0998
SENTINEL = 48.0
f32, f64 = np.float32, np.float64

# ---- recorded constants: 4 x the emulation's worst ratio over CASES (python -m tests.norm_probes prints the table they come from;
#      profiles/norm_probes.txt keeps it).  test_host_norm_probes.py fails if calibrate() exceeds them. ----
C_M = 136.0        # mean:  |mean - mean64| <= C_M * U * max(|mean64|, sigma64)
C_R = 180.0       # rstd:  |rstd / rstd64 - 1| <= C_R * U * kappa + 4 U       (kappa -> 1 on the centred paths)
K_FWD = 8.0      # forward outputs: fp32 term K_FWD * U * (|x a| + |mean a| + |beta| + |z64|) + propagated statistics bounds
K_BWD = 84.0      # backward outputs
C_M_IN, C_R_IN = 216.0, 130.0      # instance norm alone: its fp32 sums of x - x[pixel 0] all carry the same low bits, so their roundings do not average out
C_P = 180.0       # producer-epilogue partial sums: |s - s64| <= C_P * U * sum |q|


# ============================================================================================ launcher arithmetic (mirrors)
def gn_chunks(HW):
    """Stage-1 chunks of the chunked GroupNorm paths (norms.hip gn_chunks): ~48 pixels each, at most 128."""
    return max(1, min(128, (HW + 47) // 48))


def gn_lanes(C):
    """Pixel lanes P of the chunked kernels: 256 / (C / 8) while C / 8 <= 256, else 1 (two 256-piece passes)."""
    C8 = C // 8
    return 256 // C8 if C8 <= 256 else 1


def gn_apply_chunks(HW, C):
    return max(1, min(512, HW // (8 * gn_lanes(C))))


def gn_small_ok(C, groups, HW):
    cpg = C // groups
    return cpg % 8 == 0 and cpg // 8 <= 255 and HW * (cpg // 8) <= 2560


def gn_small_np(C, groups, HW):
    n = -(-(HW * (C // groups // 8)) // 256)
    return 2 if n <= 2 else 3 if n <= 3 else 5 if n <= 5 else 10


def gn_path(C, groups, HW, entry="ops.groupnorm"):
    """Which kernels a GroupNorm forward of this shape runs: 'small-NP<k>' (one launch, centred), 'two-launch' (partial + folding
    apply), 'three-launch' (partial, finalize, apply: ops.groupnorm at HW >= 4096)."""
    if entry == "ops.groupnorm" and HW >= 4096:
        return "three-launch"
    return f"small-NP{gn_small_np(C, groups, HW)}" if gn_small_ok(C, groups, HW) else "two-launch"


def gn_bwd_path(C, groups, HW):
    return f"small-NP{gn_small_np(C, groups, HW)}" if gn_small_ok(C, groups, HW) else "chunked"


def has_empty_chunk(HW, nch):
    return -(-HW // nch) * (nch - 1) >= HW


def ln_template(C, pair=False):
    """(NQ pieces per lane, RW rows per wave) of ln_fwd_kernel."""
    if C > 2048 or C % 8:
        raise ValueError("LayerNorm: C % 8 == 0 and C <= 2048")
    return (1, 2 if pair else 4) if C <= 512 else (2, 1 if pair else 2) if C <= 1024 else (4, 1)


def wino_ok(IH, IW, C, groups):
    cpg = C // groups
    return not (IH & 1 or IW & 1 or cpg % 8 or cpg // 8 > 255 or IH * IW * (cpg // 8) > 2560 or IH * IW * cpg * 2 > 64 * 1024)


BN_CHUNKS = 64
IN_SLAB, IN_LANES, IN_CW = 256, 32, 64


def in_slab(HW):
    return IN_SLAB if HW <= 256 * IN_SLAB else -(-(-(-HW // 256)) // IN_LANES) * IN_LANES


def straddling_pieces(C, groups):
    """8-channel pieces whose channels belong to two groups -> [(piece, nlo)]."""
    cpg = C // groups
    out = []
    for piece in range(C // 8):
        nlo = min(8, (piece * 8 // cpg + 1) * cpg - piece * 8)
        if nlo < 8:
            out.append((piece, nlo))
    return out


# ============================================================================================ small fp32 helpers
def seq_sum32(a, axis=-1):
    """Left-to-right fp32 sum (np.cumsum accumulates in order; np.sum would go pairwise)."""
    a = np.asarray(a, dtype=f32)
    return np.take(np.cumsum(a, axis=axis, dtype=f32), -1, axis=axis)


def chunk_sum32(q, per):
    """q [S, L, w] fp32: sequential within chunks of `per` positions along L (x w elements), then sequentially over the chunks."""
    S, L, w = q.shape
    nch = -(-L // per)
    pad = np.zeros((S, nch * per, w), dtype=f32)          # adding +0 is exact
    pad[:, :L] = q
    return seq_sum32(seq_sum32(pad.reshape(S, nch, per * w)))


def fma32(x, a, b):
    return (np.asarray(x, f64) * np.asarray(a, f64) + np.asarray(b, f64)).astype(f32)      # product exact in fp64


def silu64(z):
    return z / (1.0 + np.exp(-z))


def silu_grad64(z):
    s = 1.0 / (1.0 + np.exp(-z))
    return s * (1.0 + z * (1.0 - s))


def silu32(z):
    z = np.asarray(z, f32)
    return (z / (f32(1) + np.exp(-z, dtype=f32))).astype(f32)


def silu_grad32(z):
    z = np.asarray(z, f32)
    s = (f32(1) / (f32(1) + np.exp(-z, dtype=f32))).astype(f32)
    return (s * (f32(1) + z * (f32(1) - s))).astype(f32)


def to16(v):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(v).astype(np.float16)


def _grp(x, rows, HW, G):
    """[rows * HW, C] -> [rows * G, HW, cpg]"""
    C = x.shape[1]
    return np.ascontiguousarray(x.reshape(rows, HW, G, C // G).transpose(0, 2, 1, 3)).reshape(rows * G, HW, C // G)


def _per_channel(s, rows, HW, G, C):
    """[rows, G] -> [rows * HW, C]"""
    return np.repeat(np.repeat(s.reshape(rows, 1, G), C // G, axis=2), HW, axis=1).reshape(rows * HW, C)


# ============================================================================================ fp64 references
def ref_gn_fwd(x16, rows, HW, G, eps, gamma16, beta16, silu, lo16=None, stats_of="sum"):
    x = np.asarray(x16, f64)
    v = x + np.asarray(lo16, f64) if lo16 is not None else x
    C = x.shape[1]
    sv = _grp(v if stats_of == "sum" else x, rows, HW, G).reshape(rows * G, -1)
    mean = sv.mean(axis=1)
    var = ((sv - mean[:, None]) ** 2).mean(axis=1)
    rstd = (var + eps) ** -0.5
    kappa = 1.0 + mean ** 2 / np.maximum(var, 1e-300)
    mc, rc = _per_channel(mean, rows, HW, G, C), _per_channel(rstd, rows, HW, G, C)
    ga, be = np.asarray(gamma16, f64), np.asarray(beta16, f64)
    a = rc * ga
    sh = be - mc * a
    z = (v - mc) * a + be
    y = silu64(z) if silu else z
    sh_ = (rows, G)
    return dict(mean=mean.reshape(sh_), var=var.reshape(sh_), rstd=rstd.reshape(sh_), kappa=kappa.reshape(sh_), sigma=np.sqrt(var).reshape(sh_),
                v=v, a=a, sh=sh, beta=be, z=z, y=y, mean_c=mc, rstd_c=rc, n=HW * (C // G))


def ref_gn_bwd(x16, dy16, rows, HW, G, stats32, gamma16, beta16, silu, res16=None):
    """Backward to the input with the statistics as GIVEN inputs (fp32 [rows, G, 2]: the reference's, rounded, or the forward kernel's)."""
    x, dy = np.asarray(x16, f64), np.asarray(dy16, f64)
    C = x.shape[1]
    st = np.asarray(stats32, f64).reshape(rows, G, 2)
    mc, rc = _per_channel(st[..., 0], rows, HW, G, C), _per_channel(st[..., 1], rows, HW, G, C)
    ga = np.asarray(gamma16, f64)
    be = np.asarray(beta16, f64) if beta16 is not None else np.zeros(C)
    xh = (x - mc) * rc
    z = xh * ga + be
    d = dy * ga * (silu_grad64(z) if silu else 1.0)
    dg, dxg = _grp(d, rows, HW, G).reshape(rows * G, -1), _grp(d * xh, rows, HW, G).reshape(rows * G, -1)
    m1, m2 = dg.mean(axis=1), dxg.mean(axis=1)
    s1, s2 = dg.std(axis=1), dxg.std(axis=1)
    m1c, m2c = _per_channel(m1, rows, HW, G, C), _per_channel(m2, rows, HW, G, C)
    r = np.asarray(res16, f64) if res16 is not None else 0.0
    dx = rc * (d - m1c - xh * m2c) + r
    return dict(m1=m1.reshape(rows, G), m2=m2.reshape(rows, G), sd1=s1.reshape(rows, G), sd2=s2.reshape(rows, G), xh=xh, z=z, d=d, dx=dx,
                mean_c=mc, rstd_c=rc, m1_c=m1c, m2_c=m2c, res=r, x=x, dy=dy, gamma=ga)


def bn_rows(S, segs, seg_rows, g):
    """Row indices of sample g in the order of `rowof` (lgp.hip): segment-major, the S samples interleaved inside a segment."""
    return np.concatenate([(j * S + g) * seg_rows + np.arange(seg_rows) for j in range(segs)])


def ref_bn(x16, S, segs, seg_rows, eps, gamma16, beta16, dy16=None, train=True, stats32=None):
    """Per-sample BatchNorm: statistics [S, C], y, and (dy given) the backward through the preceding ReLU with the statistics
    stats32 [S, C, 2] as given inputs."""
    x = np.asarray(x16, f64)
    C, n = x.shape[1], segs * seg_rows
    ga, be = np.asarray(gamma16, f64), np.asarray(beta16, f64)
    out = dict(mean=np.zeros((S, C)), var=np.zeros((S, C)), y=np.zeros_like(x), n=n)
    if dy16 is not None:
        out.update(dx=np.zeros_like(x), mag=np.zeros_like(x), m1=np.zeros((S, C)), m2=np.zeros((S, C)), sd1=np.zeros((S, C)), sd2=np.zeros((S, C)))
    for g in range(S):
        idx = bn_rows(S, segs, seg_rows, g)
        xs = x[idx]
        out["mean"][g], out["var"][g] = xs.mean(0), xs.var(0)
        out["y"][idx] = (xs - out["mean"][g]) * (out["var"][g] + eps) ** -0.5 * ga + be
        if dy16 is not None:
            st = np.asarray(stats32, f64).reshape(S, C, 2)[g]
            dys = np.asarray(dy16, f64)[idx]
            xh = (xs - st[:, 0]) * st[:, 1]
            m1, m2 = (dys.mean(0), (dys * xh).mean(0)) if train else (np.zeros(C), np.zeros(C))
            out["m1"][g], out["m2"][g], out["sd1"][g], out["sd2"][g] = m1, m2, dys.std(0), (dys * xh).std(0)
            a = ga * st[:, 1]
            out["dx"][idx] = (xs > 0) * a * (dys - m1 - xh * m2)
            out["mag"][idx] = np.abs(a) * (np.abs(dys) + np.abs(m1) + (np.abs(xs) + np.abs(st[:, 0])) * st[:, 1] * np.abs(m2))
    out["rstd"] = (out["var"] + eps) ** -0.5
    out["sigma"] = np.sqrt(out["var"])
    out["kappa"] = 1.0 + out["mean"] ** 2 / np.maximum(out["var"], 1e-300)
    return out


def ref_bn_running(mean, var, n, rm0, rv0):
    """running statistics after the S samples of a call, in sample order (momentum 0.1, unbiased variance)."""
    rm, rv = np.asarray(rm0, f64).copy(), np.asarray(rv0, f64).copy()
    for g in range(mean.shape[0]):
        rm = 0.9 * rm + 0.1 * mean[g]
        rv = 0.9 * rv + 0.1 * var[g] * n / (n - 1)
    return rm, rv


def ref_instnorm(x16, rows, HW, eps, slope):
    """skg_instnorm_act_f16: InstanceNorm2d(affine=False), the normalised value stored in fp16, then act(h) = h if h >= 0 else
    slope * h, stored in fp16.  Returns the fp64 normalised value n and act(n); kappa is that of the data SHIFTED by the sample's
    first pixel, which is what the kernel sums."""
    x = np.asarray(x16, f64).reshape(rows, HW, -1)
    mean, var = x.mean(1), x.var(1)
    rstd = (var + eps) ** -0.5
    nrm = (x - mean[:, None]) * rstd[:, None]
    act = np.where(nrm >= 0, nrm, slope * nrm)
    kap = 1.0 + (mean - x[:, 0]) ** 2 / np.maximum(var, 1e-300)
    C = x.shape[2]
    return dict(mean=mean, var=var, rstd=rstd, sigma=np.sqrt(var), kappa=kap, n=nrm.reshape(rows * HW, C), y=act.reshape(rows * HW, C),
                x=x.reshape(rows * HW, C), mean_c=np.repeat(mean, HW, 0), rstd_c=np.repeat(rstd, HW, 0))


# ============================================================================================ fp32 emulations
def emu_gn_fwd(x16, rows, HW, G, eps, gamma16, beta16, silu, *, centred, per=None, lo16=None, mutant=None, stats32=None):
    """The forward formula in fp32.  centred: gn_small_kernel / gn_small_wino_kernel / ln_fwd_kernel (statistics of hi + lo);
    else the chunked form with `per` pixels per chunk (statistics of hi).  stats32: apply alone on given statistics.
    mutant: one of the deliberate errors of test_host_norm_probes.py."""
    x = np.asarray(x16, f32)
    C, cpg = x.shape[1], x.shape[1] // G
    v = (x + np.asarray(lo16, f32)).astype(f32) if lo16 is not None else x
    inv_n = f32(1.0 / (float(HW) * cpg)) if HW > 1 or G > 1 else None
    epsf = f32(0.0 if mutant == "eps_dropped" else eps)
    raw = None
    if stats32 is not None:
        st = np.asarray(stats32, f32).reshape(rows * G, 2)
        mean, rstd = st[:, 0].copy(), st[:, 1].copy()
    else:
        src = v if centred else x
        if mutant in ("drop_last_pixel", "drop_chunk_last_pixel"):
            src = src.copy().reshape(rows, HW, C)
            src[:, HW - 1 if mutant == "drop_last_pixel" else (per or HW) - 1] = 0
            src = src.reshape(rows * HW, C)
        sg = _grp(src, rows, HW, G)
        if centred and mutant != "uncentred":
            s = chunk_sum32(sg, per or HW)
            mean = (s * inv_n).astype(f32) if inv_n is not None else (s / f32(C)).astype(f32)
            d = (sg - mean[:, None, None]).astype(f32)
            s2 = chunk_sum32((d * d).astype(f32), per or HW)
            raw = (s2 * inv_n).astype(f32) if inv_n is not None else (s2 / f32(C)).astype(f32)
            var = raw
        else:
            inv = inv_n if inv_n is not None else f32(1.0 / C)
            s1 = chunk_sum32(sg, per or HW)
            s2 = chunk_sum32((sg * sg).astype(f32), per or HW)
            mean = (s1 * inv).astype(f32)
            raw = ((s2 * inv).astype(f32) - (mean * mean).astype(f32)).astype(f32)
            var = raw if mutant == "no_clamp" else np.maximum(raw, f32(0))
        with np.errstate(invalid="ignore", divide="ignore"):
            rstd = (f32(1) / np.sqrt((var + epsf).astype(f32))).astype(f32)
    mean2, rstd2 = mean.reshape(rows, G), rstd.reshape(rows, G)
    if mutant == "prev_sample":
        mean2, rstd2 = np.roll(mean2, 1, axis=0), np.roll(rstd2, 1, axis=0)
    mc, rc = _per_channel(mean2, rows, HW, G, C), _per_channel(rstd2, rows, HW, G, C)
    if mutant in ("nlo_off2", "hi_from_lo", "one_store"):
        mc, rc = mc.copy(), rc.copy()
        pieces = straddling_pieces(C, G)
        for piece, nlo in (pieces[:1] if mutant == "one_store" else pieces):
            c0, glo = piece * 8, piece * 8 // cpg
            cols = slice(c0 + nlo - 2, c0 + nlo) if mutant != "hi_from_lo" else slice(c0 + nlo, c0 + 8)
            src_g = glo + 1 if mutant != "hi_from_lo" else glo
            rsel = slice(0, 1) if mutant == "one_store" else slice(None)          # one_store: the first pixel of sample 0 only
            mc[rsel, cols] = _per_channel(mean2, rows, HW, G, C)[rsel, src_g * cpg][:, None]
            rc[rsel, cols] = _per_channel(rstd2, rows, HW, G, C)[rsel, src_g * cpg][:, None]
    ga, be = np.asarray(gamma16, f32), np.asarray(beta16, f32)
    if centred:
        z = ((((v - mc).astype(f32) * rc).astype(f32) * ga).astype(f32) + be).astype(f32)
    else:
        a = (rc * ga).astype(f32)
        sh = (be - (mc * a).astype(f32)).astype(f32)
        z = fma32(v, a, sh)
    with np.errstate(invalid="ignore", over="ignore"):
        y = silu32(z) if silu else z
    return dict(mean=mean2, rstd=rstd2, raw=None if raw is None else raw.reshape(rows, G), y32=y, y16=to16(y),
                lo16=to16(y - to16(y).astype(f32)))


def emu_gn_bwd(x16, dy16, rows, HW, G, stats32, gamma16, beta16, silu, res16=None, per=None, mutant=None):
    x, dy = np.asarray(x16, f32), np.asarray(dy16, f32)
    C, cpg = x.shape[1], x.shape[1] // G
    st = np.asarray(stats32, f32).reshape(rows, G, 2)
    mc, rc = _per_channel(st[..., 0], rows, HW, G, C), _per_channel(st[..., 1], rows, HW, G, C)
    ga = np.asarray(gamma16, f32)
    be = np.asarray(beta16, f32) if beta16 is not None else np.zeros(C, f32)
    xh = ((x - mc).astype(f32) * rc).astype(f32)
    d = dy
    if silu and mutant != "silu_grad_1":
        d = (d * silu_grad32(((xh * ga).astype(f32) + be).astype(f32))).astype(f32)
    d = (d * ga).astype(f32)
    inv_n = f32(1.0 / (float(HW) * cpg)) if HW > 1 or G > 1 else f32(1.0 / C)
    m1 = (chunk_sum32(_grp(d, rows, HW, G), per or HW) * inv_n).astype(f32)
    m2 = (chunk_sum32(_grp((d * (x if mutant == "m2_with_x" else xh)).astype(f32), rows, HW, G), per or HW) * inv_n).astype(f32)
    m1c, m2c = _per_channel(m1.reshape(rows, G), rows, HW, G, C), _per_channel(m2.reshape(rows, G), rows, HW, G, C)
    dx = (rc * ((d - m1c).astype(f32) - (xh * m2c).astype(f32)).astype(f32)).astype(f32)
    if res16 is not None:
        r = np.asarray(res16, f32).copy()
        if mutant == "no_res_last_row":
            r[-1] = 0
        dx = (dx + r).astype(f32)
    return dict(m1=m1.reshape(rows, G), m2=m2.reshape(rows, G), dx32=dx, dx16=to16(dx))


def emu_bn(x16, S, segs, seg_rows, eps, gamma16, beta16, dy16=None, train=True, stats32=None, mutant=None):
    """bn_partial / bn_finalize / bn_apply in fp32: uncentred, 64 row chunks; y = x a + (beta - mean a); the ReLU backward in the
    kernel's coefficient form dx = [x > 0] (dy a - (a m1 - cc mean) - x cc), cc = a rstd m2."""
    x = np.asarray(x16, f32)
    C, n = x.shape[1], segs * seg_rows
    per = -(-n // BN_CHUNKS)
    ga, be = np.asarray(gamma16, f32), np.asarray(beta16, f32)
    out = dict(mean=np.zeros((S, C), f32), rstd=np.zeros((S, C), f32), var=np.zeros((S, C), f32), raw=np.zeros((S, C), f32), y32=np.zeros_like(x))
    if dy16 is not None:
        out["dx32"] = np.zeros_like(x)
    for g in range(S):
        idx = bn_rows(S, segs, seg_rows, g)
        src = bn_rows(S, segs, seg_rows, g) if mutant != "segs_swapped" else np.concatenate([(j * S + g) * seg_rows + np.arange(seg_rows) for j in reversed(range(segs))])
        xs = x[src]
        q = np.ascontiguousarray(xs.T)[:, :, None]                      # [C, n, 1]
        mean = (chunk_sum32(q, per) / f32(n)).astype(f32)
        raw = ((chunk_sum32((q * q).astype(f32), per) / f32(n)).astype(f32) - (mean * mean).astype(f32)).astype(f32)
        var = np.maximum(raw, f32(0))
        rstd = (f32(1) / np.sqrt((var + f32(eps)).astype(f32))).astype(f32)
        out["mean"][g], out["rstd"][g], out["var"][g], out["raw"][g] = mean, rstd, var, raw
        a = (ga * rstd).astype(f32)
        out["y32"][idx] = fma32(xs, a, (be - (mean * a).astype(f32)).astype(f32))
        if dy16 is not None:
            st = np.asarray(stats32, f32).reshape(S, C, 2)[g]
            mu, rs = st[:, 0], st[:, 1]
            dys = np.asarray(dy16, f32)[src]
            if train:
                m1 = (chunk_sum32(np.ascontiguousarray(dys.T)[:, :, None], per) / f32(n)).astype(f32)
                t = ((dys * (xs - mu).astype(f32)).astype(f32) * rs).astype(f32)
                m2 = (chunk_sum32(np.ascontiguousarray(t.T)[:, :, None], per) / f32(n)).astype(f32)
            else:
                m1 = m2 = np.zeros(C, f32)
            a = (ga * rs).astype(f32)
            cc = ((a * rs).astype(f32) * m2).astype(f32)
            cb = ((a * m1).astype(f32) - (cc * mu).astype(f32)).astype(f32)
            out["dx32"][idx] = np.where(xs > 0, (((dys * a).astype(f32) - cb).astype(f32) - (xs * cc).astype(f32)).astype(f32), f32(0))
    out["y16"] = to16(out["y32"])
    if dy16 is not None:
        out["dx16"] = to16(out["dx32"])
    return out


def emu_bn_running(mean32, var32, n, rm0, rv0):
    rm, rv = np.asarray(rm0, f32).copy(), np.asarray(rv0, f32).copy()
    for g in range(mean32.shape[0]):
        rm = (f32(0.9) * rm + f32(0.1) * mean32[g]).astype(f32)
        rv = (f32(0.9) * rv + (f32(0.1) * var32[g]).astype(f32) * (f32(n) / f32(n - 1))).astype(f32)
    return rm, rv


def emu_instnorm(x16, rows, HW, eps, slope):
    """Sums of d = x - x[pixel 0] and d^2 in fp32, sequential over a slab, the slabs folded in fp64 (instnorm_finalize_kernel)."""
    x = np.asarray(x16, f32).reshape(rows, HW, -1)
    C, slab = x.shape[2], in_slab(HW)
    nsl = -(-HW // slab)
    d = (x - x[:, :1]).astype(f32)
    pad = np.zeros((rows, nsl * slab, C), f32)
    pad[:, :HW] = d
    ps = pad.reshape(rows, nsl, slab, C)
    s = seq_sum32(ps, axis=2).astype(f64).sum(1)
    q = seq_sum32((ps * ps).astype(f32), axis=2).astype(f64).sum(1)
    m = s / HW
    var = np.maximum(q / HW - m * m, 0.0)
    mean = (x[:, 0].astype(f64) + m).astype(f32)
    rstd = (1.0 / np.sqrt(var + f64(f32(eps)))).astype(f32)
    nrm = ((x - mean[:, None]).astype(f32) * rstd[:, None]).astype(f32).reshape(rows * HW, C)
    h = to16(nrm).astype(f32)
    return dict(mean=mean, rstd=rstd, n32=nrm, y16=to16(np.where(h >= 0, h, (f32(slope) * h).astype(f32))))


def wino_input_transform(n16, rows, IH, IW):
    """V = B^T d B of F(2x2, 3x3) per 4 x 4 tile (stride 2, zero halo) in the add order of gn_small_wino_kernel: fp32 adds on the
    fp16 activations, one fp16 rounding; component 4 a + b at columns [(4 a + b) C, (4 a + b + 1) C) -> [rows * IH/2 * IW/2, 16 C]."""
    C = n16.shape[1]
    pad = np.zeros((rows, IH + 2, IW + 2, C), f32)
    pad[:, 1:-1, 1:-1] = np.asarray(n16, f32).reshape(rows, IH, IW, C)
    d = [[pad[:, a:a + IH:2, b:b + IW:2] for b in range(4)] for a in range(4)]

    def bt(q0, q1, q2, q3):
        return [(q0 - q2).astype(f32), (q1 + q2).astype(f32), (q2 - q1).astype(f32), (q1 - q3).astype(f32)]
    t = [bt(d[0][b], d[1][b], d[2][b], d[3][b]) for b in range(4)]      # t[b][a']
    V = np.zeros((rows, IH // 2, IW // 2, 16, C), np.float16)
    for a in range(4):
        for b, vv in enumerate(bt(t[0][a], t[1][a], t[2][a], t[3][a])):
            V[..., 4 * a + b, :] = to16(vv)
    return V.reshape(rows * (IH // 2) * (IW // 2), 16 * C)


# ============================================================================================ bounds and comparators
def stat_ratios(mean, rstd, ref, centred):
    """(mean error / (U max(|mean64|, sigma64)), rstd relative error / (U kappa)) - the quantities C_M and C_R scale; kappa -> 1
    when the path is centred."""
    mean, rstd = np.asarray(mean, f64), np.asarray(rstd, f64)
    rm = np.abs(mean - ref["mean"]) / (U * np.maximum(np.abs(ref["mean"]), ref["sigma"]) + 1e-300)
    kap = 1.0 if centred else ref["kappa"]
    rr = np.abs(rstd / ref["rstd"] - 1.0) / (U * kap)
    return rm, rr


def _at(r):
    return tuple(int(v) for v in np.unravel_index(r.argmax(), r.shape))


def mean_bound(ref):
    return C_M * U * np.maximum(np.abs(ref["mean"]), ref["sigma"])


def rstd_bound(ref, centred):
    return C_R * U * (1.0 if centred else ref["kappa"]) + 4 * U


def check_stats(name, mean, rstd, ref, centred):
    """Asserts the statistics bound on every (sample, group); returns the achieved error / bound ratios."""
    mean, rstd = np.asarray(mean, f64).reshape(ref["mean"].shape), np.asarray(rstd, f64).reshape(ref["mean"].shape)
    assert np.isfinite(mean).all() and np.isfinite(rstd).all(), f"{name}: non-finite statistics"
    em = np.abs(mean - ref["mean"]) / mean_bound(ref)
    er = np.abs(rstd / ref["rstd"] - 1.0) / rstd_bound(ref, centred)
    i, j = _at(em), _at(er)
    print(f"[norm-probe] {name}: mean err/bound {em.max():.3f} at {i}, rstd err/bound {er.max():.3f} at {j} (kappa max {ref['kappa'].max():.1f}, "
          f"{'centred' if centred else 'uncentred'})")
    assert em.max() <= 1.0, f"{name}: mean of (sample, group) {i}: {mean[i]!r} vs {ref['mean'][i]!r}, {em.max():.2f} x the bound"
    assert er.max() <= 1.0, f"{name}: rstd of (sample, group) {j}: {rstd[j]!r} vs {ref['rstd'][j]!r}, {er.max():.2f} x the bound"
    return float(em.max()), float(er.max())


def fwd_fp32_term(ref, rows, HW, G, centred, silu, given_stats=False):
    """The fp32 part of the forward output bound per element, WITHOUT K_FWD: (rounding magnitudes, propagated statistics bound)."""
    C = ref["v"].shape[1]
    # |sh| alone would hide the rounding of its own two terms when beta and mean * a cancel, and the centred kernels form
    # (v - mean) * a before adding beta: both terms of sh enter with their own magnitude
    mag = U * (np.abs(ref["v"] * ref["a"]) + np.abs(ref["mean_c"] * ref["a"]) + np.abs(ref["beta"]) +
               np.abs(ref["z"]) + (np.abs(ref["y"]) if silu else 0.0))
    if given_stats:
        prop = 0.0
    else:
        bm = _per_channel(mean_bound(ref), rows, HW, G, C)
        br = _per_channel(np.broadcast_to(rstd_bound(ref, centred), ref["mean"].shape), rows, HW, G, C)
        prop = np.abs(ref["a"]) * bm + np.abs((ref["v"] - ref["mean_c"]) * ref["a"]) * br
    f = SILU_GRAD_MAX if silu else 1.0
    return f * mag, f * prop


def out_bound(y64, fp32_term):
    return H_RND * np.abs(y64) + H_SUB + fp32_term * (1 + H_RND)


def check_out(name, got, y64, fp32_term):
    """Every element: |got - y64| <= one fp16 rounding + the fp32 term.  No element is left out."""
    got = np.asarray(got, f64)
    assert np.isfinite(got).all(), f"{name}: {np.count_nonzero(~np.isfinite(got))} non-finite outputs"
    r = np.abs(got - y64) / out_bound(y64, fp32_term)
    i = _at(r)
    print(f"[norm-probe] {name}: worst element {i}: err/bound {r.max():.3f} ({np.count_nonzero(r > 1)} of {r.size} over)")
    assert r.max() <= 1.0, f"{name}: element {i}: got {got[i]!r}, fp64 {y64[i]!r}, {r.max():.2f} x the bound; {np.count_nonzero(r > 1)} elements over"
    return float(r.max())


def check_gn_fwd(name, y, ref, rows, HW, G, centred, silu, given_stats=False):
    mag, prop = fwd_fp32_term(ref, rows, HW, G, centred, silu, given_stats)
    return check_out(name, y, ref["y"], K_FWD * mag + prop)


def check_lo(name, hi, lo, ref, rows, HW, G, centred, silu):
    """Pair output: hi as any output; lo = fp16(v - hi) against the fp64 v to one lo-rounding (2^-11 |v - hi| + 2^-25) + the fp32 term."""
    mag, prop = fwd_fp32_term(ref, rows, HW, G, centred, silu)
    hi, lo = np.asarray(hi, f64), np.asarray(lo, f64)
    want = ref["y"] - hi
    r = np.abs(lo - want) / (H_RND * np.abs(want) + H_SUB + K_FWD * mag + prop)
    print(f"[norm-probe] {name}: lo half worst err/bound {r.max():.3f}")
    assert r.max() <= 1.0, f"{name}: lo half {r.max():.2f} x the bound at {np.unravel_index(r.argmax(), r.shape)}"
    return float(r.max())


def bwd_fp32_term(rb, rows, HW, G, silu):
    """(rounding magnitudes, propagated bound of the two means m1, m2) of dx = rstd (d - m1 - xhat m2) + residual, without K_BWD.
    xhat = (x - mean) rstd carries U (|x| + |mean|) rstd of its own; it enters through m2 and, with SiLU, through silu'(z)."""
    C = rb["x"].shape[1]
    r = np.abs(rb["rstd_c"])
    exh = (np.abs(rb["x"]) + np.abs(rb["mean_c"])) * r                   # |xhat| with its cancellation undone
    dmag = np.abs(rb["d"]) * (1.0 + (np.abs(rb["z"]) + exh * np.abs(rb["gamma"]) if silu else 0.0))
    mag = U * (r * (dmag + np.abs(rb["m1_c"]) + exh * np.abs(rb["m2_c"])) + np.abs(rb["res"]) + np.abs(rb["dx"]))
    b1 = C_M * U * _per_channel(np.maximum(np.abs(rb["m1"]), rb["sd1"]), rows, HW, G, C)
    b2 = C_M * U * _per_channel(np.maximum(np.abs(rb["m2"]), rb["sd2"]), rows, HW, G, C)
    # the means of dmag / dmag * exh: what the rounding of every summand adds to m1 / m2
    g1 = U * _per_channel(_grp(dmag, rows, HW, G).reshape(rows * G, -1).mean(1).reshape(rows, G), rows, HW, G, C)
    g2 = U * _per_channel(_grp(dmag * exh, rows, HW, G).reshape(rows * G, -1).mean(1).reshape(rows, G), rows, HW, G, C)
    return mag + r * (g1 + np.abs(rb["xh"]) * g2), r * (b1 + np.abs(rb["xh"]) * b2)


def check_gn_bwd(name, dx, rb, rows, HW, G, silu):
    mag, prop = bwd_fp32_term(rb, rows, HW, G, silu)
    return check_out(name, dx, rb["dx"], K_BWD * mag + prop)


def bn_terms(rb, ga, be, x16, S, segs, seg_rows, given_stats=False):
    """BatchNorm apply: the forward fp32 term, per element (rounding magnitudes, propagated statistics bound)."""
    x = np.asarray(x16, f64)
    mag, prop = np.zeros_like(x), np.zeros_like(x)
    for g in range(S):
        idx = bn_rows(S, segs, seg_rows, g)
        a = rb["rstd"][g] * np.asarray(ga, f64)
        sh = np.asarray(be, f64) - rb["mean"][g] * a
        mag[idx] = U * (np.abs(x[idx] * a) + np.abs(rb["mean"][g] * a) + np.abs(np.asarray(be, f64)) + np.abs(rb["y"][idx]))
        if not given_stats:
            bm = C_M * U * np.maximum(np.abs(rb["mean"][g]), rb["sigma"][g])
            br = C_R * U * rb["kappa"][g] + 4 * U
            prop[idx] = np.abs(a) * bm + np.abs((x[idx] - rb["mean"][g]) * a) * br
    return mag, prop


def const_bound(x64, gamma64, beta_act64, eps):
    """Constant groups: |y - act(beta)| <= |gamma| eps^-1/2 C_M U |x| + one fp16 rounding (+ the fp32 rounding of beta's own sum)."""
    return np.abs(gamma64) * eps ** -0.5 * C_M * U * np.abs(x64) * SILU_GRAD_MAX + H_RND * np.abs(beta_act64) + H_SUB + 4 * U * np.abs(beta_act64)


def partial_sums64(y16, rows, HW, G):
    """The producers' layout [rows, HW / 128, G, 2]: (sum, sum of squares) of the fp16 output per (sample, 128-row chunk, group) in fp64,
    and the matching sums of |q| that scale the bound C_P * U * sum |q|."""
    y = np.asarray(y16, f64)
    C = y.shape[1]
    yc = y.reshape(rows, HW // 128, 128, G, C // G)
    return np.stack([yc.sum(axis=(2, 4)), (yc * yc).sum(axis=(2, 4))], -1), np.stack([np.abs(yc).sum(axis=(2, 4)), (yc * yc).sum(axis=(2, 4))], -1)


def emu_partial_sums(y16, rows, HW, G):
    y = np.asarray(y16, f32)
    C = y.shape[1]
    yc = np.ascontiguousarray(y.reshape(rows, HW // 128, 128, G, C // G).transpose(0, 1, 3, 2, 4)).reshape(rows, HW // 128, G, -1)
    return np.stack([seq_sum32(yc), seq_sum32((yc * yc).astype(f32))], -1)


def frob(got, ref64):
    got, ref64 = np.asarray(got, f64), np.asarray(ref64, f64)
    return float(np.linalg.norm(got - ref64) / max(np.linalg.norm(ref64), 1e-300))


# ============================================================================================ input draws
MEANS = (-1.0, 0.35, -0.6, 0.8, 0.1, -0.25, 1.0, -0.85, 0.55)
SCALES = (0.25, 2.0, 1.0, 4.0, 0.5)


def gamma_beta(C, seed):
    r = np.random.default_rng(1000 + seed)
    return to16(1 + 0.2 * r.standard_normal(C)), to16(0.2 * r.standard_normal(C))


def draw_structure(rows, HW, C, G, seed):
    """Every (sample, group) gets its own mean in [-1, 1] and scale in {0.25 .. 4} (kappa <= 17): a statistic read from the wrong
    group, the wrong sample or a stale buffer is an O(1) error in that slice."""
    r = np.random.default_rng(seed)
    k = np.arange(rows * G).reshape(rows, G)
    mu = np.asarray(MEANS)[(3 * k + k // G) % len(MEANS)]
    sc = np.asarray(SCALES)[(k + 2 * (k // G)) % len(SCALES)]
    z = r.standard_normal((rows * HW, C))
    return to16(_per_channel(mu, rows, HW, G, C) + _per_channel(sc, rows, HW, G, C) * z)


def sentinel_pixels(HW, C, per):
    """(pixel, channel) positions of the sentinel draw for the chunked kernels: the last pixel of the map, the last pixel of every
    stage-1 chunk, the first pixel after each 4 P unrolled block of chunk 0, the last channel of the first straddling piece, the
    first channel of the second 256-piece pass."""
    P = gn_lanes(C)
    pos = {(HW - 1, C - 1)}
    for k in range(-(-HW // per)):
        pos.add((min(HW, (k + 1) * per) - 1, (8 * k + 3) % C))
    for j in range(1, 3):
        if 4 * P * j < min(per, HW):
            pos.add((4 * P * j, (8 * j + 5) % C))
    if C > 2048:
        pos.add((min(1, HW - 1), 2048))
    return sorted(pos)


def draw_sentinel(rows, HW, C, G, seed, per):
    x = draw_structure(rows, HW, C, G, seed).reshape(rows, HW, C)
    pos = sentinel_pixels(HW, C, per)
    st = straddling_pieces(C, G)
    if st:
        pos.append((0, st[0][0] * 8 + 7))
    for p, c in pos:
        x[:, p, c] = SENTINEL
    return x.reshape(rows * HW, C), pos


def draw_conditioning(rows, HW, C, ratio, seed):
    """N(mu, 1), mu / sigma = ratio: for the kappa statement only."""
    return to16(ratio + np.random.default_rng(seed).standard_normal((rows * HW, C)))


def as_pair(v64):
    hi = to16(v64)
    return hi, to16(np.asarray(v64, f64) - hi.astype(f64))


def draw_pair(rows, HW, C, G, seed):
    r = np.random.default_rng(seed)
    base = draw_structure(rows, HW, C, G, seed).astype(f64)
    return as_pair(base * (1 + 2.0 ** -9 * r.standard_normal(base.shape)))


def negative_raw_constant(C, G, HW, per, candidates=(48.0, 37.5, 29.0, 21.25, 11.0, 5.5, 3.3, 60.0, 100.0) + tuple(3.1 + 1.7 * k for k in range(60))):
    """A constant for which the emulation's raw s2/n - mean^2 is NEGATIVE in at least one group (the clamp is what keeps rstd finite)."""
    for c in candidates:
        x = np.full((HW, C), c, np.float16)
        e = emu_gn_fwd(x, 1, HW, G, 1e-5, np.ones(C, np.float16), np.zeros(C, np.float16), False, centred=False, per=per)
        if (e["raw"] < 0).any():
            return float(np.float16(c)), float(e["raw"].min())
    raise AssertionError("no candidate constant drives the uncentred variance negative")


# ============================================================================================ the cases
@dataclass(frozen=True)
class GN:
    C: int
    G: int
    HW: int
    rows: int = 3
    draw: str = "structure"          # structure | sentinel | cond<ratio>
    silu: bool = True
    eps: float = 1e-5
    pair: bool = False
    pair_out: bool = False
    entry: str = "ops.groupnorm"     # or "fwd": skg_groupnorm_fwd directly (never the three-launch route)
    note: str = ""

    @property
    def path(self):
        return gn_path(self.C, self.G, self.HW, "fwd" if self.pair else self.entry)

    @property
    def centred(self):
        return self.path.startswith("small")

    @property
    def per(self):
        return -(-self.HW // gn_chunks(self.HW))      # the emulation's chunk: ~48 pixels, on the one-workgroup paths too

    @property
    def id(self):
        return (f"{self.path}-C{self.C}-G{self.G}-HW{self.HW}-r{self.rows}-{self.draw}" + ("-pair" if self.pair else "") +
                ("-pairout" if self.pair_out else "") + ("" if self.silu else "-nosilu") + (f"-eps{self.eps:g}" if self.eps != 1e-5 else "") +
                (f"-{self.note}" if self.note else ""))

    def inputs(self):
        seed = (self.C * 31 + self.G * 7 + self.HW) % 100003
        ga, be = gamma_beta(self.C, seed)
        lo = None
        if self.pair:
            x, lo = draw_pair(self.rows, self.HW, self.C, self.G, seed)
        elif self.draw == "sentinel":
            x, _ = draw_sentinel(self.rows, self.HW, self.C, self.G, seed, self.per or self.HW)
        elif self.draw.startswith("cond"):
            x = draw_conditioning(self.rows, self.HW, self.C, float(self.draw[4:]), seed)
        else:
            x = draw_structure(self.rows, self.HW, self.C, self.G, seed)
        return x, lo, ga, be

    def ref(self, x, lo, ga, be):
        return ref_gn_fwd(x, self.rows, self.HW, self.G, self.eps, ga, be, self.silu, lo16=lo, stats_of="sum" if self.centred else "hi")

    def emu(self, x, lo, ga, be, mutant=None):
        return emu_gn_fwd(x, self.rows, self.HW, self.G, self.eps, ga, be, self.silu, centred=self.centred, per=self.per, lo16=lo, mutant=mutant)


# small path: cpg = 8, 4 groups, 3 rows at both sides of the NP = 2 / 3 / 5 / 10 boundaries (HW * cpg / 8 pieces against 512, 768, 1280,
# 2560), wide groups, pairs.  HW = 2568 is the first map past the small path.
GN_SMALL = [GN(32, 4, hw, silu=bool(i & 1)) for i, hw in enumerate((1, 3, 255, 256, 257, 512, 520, 768, 776, 1280, 1288, 2560))] + [
    GN(160, 4, 64), GN(320, 4, 256, rows=2),
    GN(32, 4, 520, pair=True), GN(32, 4, 2560, pair=True, rows=2), GN(32, 4, 520, pair=True, pair_out=True), GN(32, 4, 2560, pair=True, pair_out=True, rows=2),
    GN(32, 4, 256, eps=1e-3, note="eps"),
]
# two launches.  Corrected against the launchers: (2560, 32, 49) and (4096, 64, 5) have cpg % 8 == 0 and <= 2560 pieces per slice, so
# skg_groupnorm_fwd sends them down the SMALL path; the second fold trip (groups > 32) and the C cap are reached on the chunked path
# by (768, 64, 50) (cpg 12, straddling) and (4096, 64, 328) (328 * 8 pieces > 2560).  (2080, 40, 90) (one pixel lane, 11 apply chunks of 9 pixels) has an empty last apply chunk.
GN_TWO = [
    GN(32, 4, 2568, rows=2, draw="sentinel"), GN(320, 32, 100, draw="sentinel"), GN(960, 32, 50, draw="sentinel"), GN(640, 32, 130, draw="sentinel"),
    GN(32, 8, 128, draw="sentinel"), GN(48, 8, 7, draw="sentinel"), GN(8, 2, 300, draw="sentinel"), GN(2056, 2, 9, rows=2, draw="sentinel"),
    GN(2080, 40, 90, rows=2, draw="sentinel", note="empty-apply-chunk"), GN(2560, 32, 49, rows=2, note="listed-as-two-launch"),
    GN(4096, 64, 5, rows=2, note="listed-as-two-launch"), GN(768, 64, 50, rows=2, draw="sentinel"), GN(4096, 64, 328, rows=2, draw="sentinel"),
    GN(320, 32, 100, pair=True), GN(2560, 32, 49, pair=True, rows=2), GN(640, 32, 130, pair=True, pair_out=True, rows=2),
    GN(320, 32, 100, eps=1e-3, silu=False, note="eps"),
]
GN_THREE = [GN(32, 8, 4096, rows=2, draw="sentinel"), GN(320, 32, 4096, rows=2, draw="sentinel"), GN(16, 2, 6150, rows=2, draw="sentinel", note="128-chunk-cap")]
GN_KAPPA = [GN(c, 32, hw, rows=1, draw=f"cond{r}", silu=False) for (c, hw) in ((320, 4096), (640, 130)) for r in (4, 16, 64)]
GN_FWD = GN_SMALL + GN_TWO + GN_THREE

# backward: (C, G, HW, rows); small path at the four NP boundaries, then the chunked path (the issue's (4096, 64, 5) is a small-path
# shape: (768, 64, 50) and (4096, 64, 328) reach the second trip of the backward fold loop, groups > 16, on the chunked path)
GN_BWD = [(32, 4, 512, 3), (32, 4, 520, 3), (32, 4, 768, 2), (32, 4, 776, 2), (32, 4, 1280, 2), (32, 4, 1288, 2), (32, 4, 2560, 2), (4096, 64, 5, 2),
          (320, 32, 100, 3), (960, 32, 50, 2), (2056, 2, 9, 2), (768, 64, 50, 2), (4096, 64, 328, 1), (32, 8, 4096, 2)]

LN_FWD = [(M, C) for C in (8, 504, 512, 520, 1024, 1032, 2040, 2048) for M in (1, 3, 5, 17)]
LN_PAIR = [(7, 320), (7, 520), (7, 1280)]
BN_CASES = [(3, 1, 5, 8), (2, 3, 37, 64), (2, 2, 129, 512), (1, 1, 300, 2056)]            # (S, segs, seg_rows, C); C is unbounded in skg_bn_*
# instance norm: HW on both sides of the one-slab fork (256 | 257) and of the long-slab fork (65536 | 65537: 288-pixel slabs); C = 64 | 128
IN_CASES = [(2, 1, 64), (2, 256, 64), (2, 257, 128), (1, 65536, 64), (1, 65537, 64)]
PARTIAL_SHAPES = [(2, 128, 32, 8), (2, 128, 64, 8), (2, 128, 80, 8), (100, 128, 320, 32)]      # (rows, HW, C, G) of the producer-epilogue cases
WINO_CASES = [(2, 2, 2, 64, 8), (3, 8, 8, 64, 4), (2, 16, 8, 160, 4), (1, 16, 16, 1280, 32), (2, 4, 6, 320, 8)]


def ln_inputs(M, C, pair=False, ratio=None):
    seed = 7 * M + C
    ga, be = gamma_beta(C, seed)
    if ratio is not None:
        return draw_conditioning(M, 1, C, ratio, seed), None, ga, be
    if pair:
        return (*draw_pair(M, 1, C, 1, seed), ga, be)
    return draw_structure(M, 1, C, 1, seed), None, ga, be


def bn_inputs(S, segs, seg_rows, C, const_channel=True):
    r = np.random.default_rng(S * 1000 + C)
    k = np.arange(S * C).reshape(S, C)
    mu, sc = np.asarray(MEANS)[(3 * k + k // C) % len(MEANS)], np.asarray(SCALES)[(k + k // C) % len(SCALES)]
    x = np.zeros((segs * S * seg_rows, C))
    for g in range(S):
        idx = bn_rows(S, segs, seg_rows, g)
        x[idx] = (np.abs(mu[g] + sc[g] * r.standard_normal((len(idx), C))) + 0.125 * (g + 1)) * (r.random((len(idx), C)) > 0.1)      # post-ReLU-like: >= 0, a tenth of the gates closed
    if const_channel:
        x[:, 5] = 3.3
    ga, be = gamma_beta(C, C)
    return to16(x), ga, be, to16(r.standard_normal(x.shape))


def in_inputs(rows, HW, C):
    r = np.random.default_rng(HW + C)
    k = np.arange(rows * C).reshape(rows, C)
    mu, sc = np.asarray(MEANS)[(3 * k + k // C) % len(MEANS)], np.asarray(SCALES)[(k + k // C) % len(SCALES)]
    return to16(np.repeat(mu, HW, 0) + np.repeat(sc, HW, 0) * r.standard_normal((rows * HW, C)))


def bwd_inputs(rows, HW, C, G):
    seed = C + 3 * HW
    r = np.random.default_rng(seed + 17)
    x = draw_structure(rows, HW, C, G, seed)
    ga, be = gamma_beta(C, seed)
    return x, to16(r.standard_normal(x.shape)), to16(r.standard_normal(x.shape)), ga, be


def ref_stats32(ref):
    return np.stack([ref["mean"], ref["rstd"]], axis=-1).astype(f32)


# ============================================================================================ calibration
@dataclass
class Cal:
    lines: list = field(default_factory=list)
    m: float = 0.0
    r: float = 0.0
    kf: float = 0.0
    kb: float = 0.0
    m_in: float = 0.0
    r_in: float = 0.0
    p: float = 0.0


def _fwd_ratio(y32, ref, mag, prop):
    """largest (|emulation before its fp16 rounding - fp64| - propagated statistics bound) / rounding magnitudes: what K_FWD scales"""
    return float((np.maximum(np.abs(np.asarray(y32, f64) - ref) - prop, 0.0) / np.maximum(mag, 1e-300)).max())


def calibrate(verbose=False, big=True):
    """Runs the emulation over every case of the GPU file and returns the largest ratios (Cal); the recorded constants are 4 x these,
    rounded up.  The forward / backward ratios are taken on the fp32 value BEFORE the fp16 rounding, which the bound carries apart."""
    cal = Cal()

    def stat(tag, n, e_mean, e_rstd, ref, centred):
        rm, rr = stat_ratios(e_mean, e_rstd, ref, centred)
        cal.m, cal.r = max(cal.m, float(rm.max())), max(cal.r, float(rr.max()))
        return f"{tag}: n {n} kappa {float(np.max(ref['kappa'])):.1f} emulation mean {rm.max():.2f} rstd {rr.max():.2f}"

    for c in GN_FWD + GN_KAPPA:
        if not big and c.HW * c.C * c.rows > 400000:
            continue
        x, lo, ga, be = c.inputs()
        ref, e = c.ref(x, lo, ga, be), c.emu(x, lo, ga, be)
        line = stat("gn-fwd " + c.id, ref["n"], e["mean"], e["rstd"], ref, c.centred)
        mag, _ = fwd_fp32_term(ref, c.rows, c.HW, c.G, c.centred, c.silu, given_stats=True)
        ea = emu_gn_fwd(x, c.rows, c.HW, c.G, c.eps, ga, be, c.silu, centred=c.centred, lo16=lo, stats32=ref_stats32(ref))
        k = _fwd_ratio(ea["y32"], ref["y"], mag, 0.0)
        cal.kf = max(cal.kf, k)
        cal.lines.append(line + f" out {k:.2f}")
    for (M, C) in LN_FWD + LN_PAIR:
        x, lo, ga, be = ln_inputs(M, C, pair=(M, C) in LN_PAIR)
        ref, e = ref_gn_fwd(x, M, 1, 1, 1e-5, ga, be, False, lo16=lo), emu_gn_fwd(x, M, 1, 1, 1e-5, ga, be, False, centred=True, lo16=lo)
        line = stat(f"ln-fwd M{M}-C{C}", C, e["mean"], e["rstd"], ref, True)
        mag, _ = fwd_fp32_term(ref, M, 1, 1, True, False, given_stats=True)
        k = _fwd_ratio(emu_gn_fwd(x, M, 1, 1, 1e-5, ga, be, False, centred=True, lo16=lo, stats32=ref_stats32(ref))["y32"], ref["y"], mag, 0.0)
        cal.kf = max(cal.kf, k)
        cal.lines.append(line + f" out {k:.2f}")
        dy, res = to16(np.random.default_rng(M + C).standard_normal(x.shape)), to16(np.random.default_rng(M + C + 1).standard_normal(x.shape))
        st = ref_stats32(ref)
        rb, eb = ref_gn_bwd(x, dy, M, 1, 1, st, ga, None, False, res), emu_gn_bwd(x, dy, M, 1, 1, st, ga, None, False, res)
        mg, _ = bwd_fp32_term(rb, M, 1, 1, False)
        cal.kb = max(cal.kb, _fwd_ratio(eb["dx32"], rb["dx"], mg, 0.0))
    for (C, G, HW, rows) in GN_BWD:
        if not big and HW * C * rows > 400000:
            continue
        x, dy, res, ga, be = bwd_inputs(rows, HW, C, G)
        st = ref_stats32(ref_gn_fwd(x, rows, HW, G, 1e-5, ga, be, True))
        per = -(-HW // gn_chunks(HW))
        for silu in (True, False):
            rb, eb = ref_gn_bwd(x, dy, rows, HW, G, st, ga, be, silu, res), emu_gn_bwd(x, dy, rows, HW, G, st, ga, be, silu, res, per=per)
            mg, _ = bwd_fp32_term(rb, rows, HW, G, silu)
            k = _fwd_ratio(eb["dx32"], rb["dx"], mg, 0.0)      # all of the error against the rounding magnitudes: K_BWD does not lean on C_M
            cal.kb = max(cal.kb, k)
            cal.lines.append(f"gn-bwd {gn_bwd_path(C, G, HW)}-C{C}-G{G}-HW{HW}-silu{int(silu)}: n {HW * C // G} emulation out {k:.2f}")
    for (S, segs, sr, C) in BN_CASES:
        x, ga, be, dy = bn_inputs(S, segs, sr, C, const_channel=False)
        rb = ref_bn(x, S, segs, sr, 1e-5, ga, be)
        e = emu_bn(x, S, segs, sr, 1e-5, ga, be)
        line = stat(f"bn S{S}-segs{segs}-rows{sr}-C{C}", segs * sr, e["mean"], e["rstd"], rb, False)
        mag, _ = bn_terms(rb, ga, be, x, S, segs, sr, given_stats=True)
        st = np.stack([rb["mean"], rb["rstd"]], -1).astype(f32)
        k = 0.0
        for g in range(S):
            idx = bn_rows(S, segs, sr, g)
            a = (np.asarray(ga, f32) * st[g, :, 1]).astype(f32)
            yg = fma32(np.asarray(x, f32)[idx], a, (np.asarray(be, f32) - (st[g, :, 0] * a).astype(f32)).astype(f32))
            k = max(k, _fwd_ratio(yg, rb["y"][idx], mag[idx], 0.0))
        cal.kf = max(cal.kf, k)
        rbb, eb = ref_bn(x, S, segs, sr, 1e-5, ga, be, dy, True, st), emu_bn(x, S, segs, sr, 1e-5, ga, be, dy, True, st)
        kb = _fwd_ratio(eb["dx32"], rbb["dx"], U * (rbb["mag"] + np.abs(rbb["dx"])), 0.0)
        cal.kb = max(cal.kb, kb)
        cal.lines.append(line + f" out {k:.2f} bwd {kb:.2f}")
    for (rows, HW, C) in IN_CASES:
        if not big and HW > 4096:
            continue
        x = in_inputs(rows, HW, C)
        ref, e = ref_instnorm(x, rows, HW, 1e-5, 0.2), emu_instnorm(x, rows, HW, 1e-5, 0.2)
        rm, rr = stat_ratios(e["mean"], e["rstd"], ref, False)
        cal.m_in, cal.r_in = max(cal.m_in, float(rm.max())), max(cal.r_in, float(rr.max()))
        mag, _ = in_terms(ref, HW)
        n32 = ((np.asarray(x, f32) - ref["mean_c"].astype(f32)).astype(f32) * ref["rstd_c"].astype(f32)).astype(f32)
        k = _fwd_ratio(n32, ref["n"], mag, 0.0)
        cal.kf = max(cal.kf, k)
        cal.lines.append(f"instnorm r{rows}-HW{HW}-C{C}: n {HW} kappa {ref['kappa'].max():.1f} emulation mean {rm.max():.2f} rstd {rr.max():.2f} out {k:.2f}")
    for (rows, HW, C, G) in PARTIAL_SHAPES:
        y = draw_structure(rows, HW, C, G, C + G)
        s64, sabs = partial_sums64(y, rows, HW, G)
        k = float((np.abs(emu_partial_sums(y, rows, HW, G) - s64) / (U * sabs)).max())
        cal.p = max(cal.p, k)
        cal.lines.append(f"partial sums rows{rows}-HW{HW}-C{C}-G{G}: {128 * C // G} summands, emulation {k:.2f}")
    if verbose:
        print("\n".join(cal.lines))
    return cal


def bn_bwd_prop(rbb, ga, st, x16, S, segs, seg_rows):
    """propagated bound of m1 = mean(dy), m2 = mean(dy xhat) in dx = [x > 0] a (dy - m1 - xhat m2)"""
    x = np.asarray(x16, f64)
    prop = np.zeros_like(x)
    st = np.asarray(st, f64).reshape(S, -1, 2)
    for g in range(S):
        idx = bn_rows(S, segs, seg_rows, g)
        a = np.abs(np.asarray(ga, f64) * st[g, :, 1])
        b1 = C_M * U * np.maximum(np.abs(rbb["m1"][g]), rbb["sd1"][g])
        exh = (np.abs(x[idx]) + np.abs(st[g, :, 0])) * st[g, :, 1]
        b2 = C_M * U * np.maximum(np.abs(rbb["m2"][g]), rbb["sd2"][g])
        prop[idx] = a * (b1 + exh * b2)
    return prop


def in_terms(ref, HW):
    """instance norm: (rounding magnitudes, propagated statistics bound) of n = (x - mean) rstd"""
    mag = U * ((np.abs(ref["x"]) + np.abs(ref["mean_c"])) * ref["rstd_c"] + np.abs(ref["n"]))
    bm = np.repeat(C_M_IN * U * np.maximum(np.abs(ref["mean"]), ref["sigma"]), HW, 0)
    br = np.repeat(C_R_IN * U * ref["kappa"] + 4 * U, HW, 0)
    return mag, ref["rstd_c"] * bm + np.abs(ref["n"]) * br


def instnorm_out_bound(ref, HW, slope):
    """two fp16 roundings: h = fp16(n), out = fp16(act(h)); act is 1-Lipschitz for |slope| <= 1"""
    mag, prop = in_terms(ref, HW)
    first = H_RND * np.abs(ref["n"]) + H_SUB + (K_FWD * mag + prop) * (1 + H_RND)
    return max(1.0, abs(slope)) * first + H_RND * np.abs(ref["y"]) + H_SUB + 2 * U * np.abs(ref["y"])


if __name__ == "__main__":
    c = calibrate(verbose=True)
    print(f"largest emulation ratios: mean {c.m:.3f} rstd {c.r:.3f} forward {c.kf:.3f} backward {c.kb:.3f} instance norm mean {c.m_in:.3f} rstd {c.r_in:.3f} partial sums {c.p:.3f}")
    print(f"4 x: C_M >= {4 * c.m:.2f} C_R >= {4 * c.r:.2f} K_FWD >= {4 * c.kf:.2f} K_BWD >= {4 * c.kb:.2f}   recorded: {C_M} {C_R} {K_FWD} {K_BWD}")
