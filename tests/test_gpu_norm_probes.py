"""Normalisation kernels (norms.hip, the BatchNorm of lgp.hip, the instance norm of sketchgen.hip) against fp64 references, per
(sample, group) and per element (tests/norm_probes.py: references, the fp32 emulations the tolerances are measured from, bounds,
draws, the case lists).  Every case asserts
  * the statistics bound on the published (mean, rstd),
  * the per-element output bound on ALL elements,
  * that a second launch reproduces outputs and statistics bit for bit (norms.hip: fixed summation orders, no atomics),
  * that the padding columns of the output views (ld > C) keep their pattern.
The path a case takes is derived from the launchers' own conditions (norm_probes.gn_path ...) and is part of the case id."""
import numpy as np
import pytest
import torch

from tests import norm_probes as P

pytestmark = pytest.mark.gpu

PATTERN = 123.5


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from sketch2img_amd import ops as o
    return o


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def N(t):
    return t.detach().cpu().numpy()


def view(M, C, pad=8, src=None):
    """[M, C] view of a [M, C + pad] buffer whose padding columns hold PATTERN; src (numpy) is copied in."""
    buf = torch.full((M, C + pad), PATTERN, device=dev(), dtype=torch.float16)
    if src is not None:
        buf[:, :C] = T(src)
    return buf, buf[:, :C]


def pad_intact(buf, C):
    return bool((buf[:, C:] == PATTERN).all())


def twice(fn):
    """Runs fn twice; every tensor it returns must come back with the same bits."""
    a, b = fn(), fn()
    torch.cuda.synchronize()
    for u, w in zip(a, b):
        if u is not None:
            assert torch.equal(u, w), "a second launch does not reproduce the first bit for bit"
    return a


# ------------------------------------------------------------------------------------------------- GroupNorm forward
@pytest.mark.parametrize("case", P.GN_FWD, ids=lambda c: c.id)
def test_groupnorm_forward(ops, case):
    c = case
    assert c.id.startswith(P.gn_path(c.C, c.G, c.HW, "fwd" if c.pair else "ops.groupnorm"))
    x, lo, ga, be = c.inputs()
    M = c.rows * c.HW
    ref = c.ref(x, lo, ga, be)
    xv = view(M, c.C, 16, x)[1]            # ldx > C on the input as well
    lov = view(M, c.C, 16, lo)[1] if lo is not None else None
    gad, bed = T(ga), T(be)

    def run():
        ob, ov = view(M, c.C, 24)
        lb, lv = view(M, c.C, 24) if c.pair_out else (None, None)
        if c.pair:
            y, st = ops.groupnorm_hilo(xv, lov, c.rows, c.HW, c.G, c.eps, gad, bed, c.silu, out=ov, want_stats=True, out_lo=lv)
        else:
            y, st = ops.groupnorm(xv, c.rows, c.HW, c.G, c.eps, gad, bed, c.silu, out=ov)
        return y, st, ob, lb
    y, st, ob, lb = twice(run)
    assert pad_intact(ob, c.C) and (lb is None or pad_intact(lb, c.C)), "padding columns of the output view were written"
    st = N(st)
    P.check_stats(c.id, st[..., 0], st[..., 1], ref, c.centred)
    P.check_gn_fwd(c.id, N(y).astype(np.float64), ref, c.rows, c.HW, c.G, c.centred, c.silu)
    if c.pair_out:
        P.check_lo(c.id, N(y), N(lb[:, :c.C]), ref, c.rows, c.HW, c.G, c.centred, c.silu)


@pytest.mark.parametrize("C,G,HW,eps", [(320, 32, 100, 1e-5), (320, 32, 100, 1e-3), (32, 4, 256, 1e-5), (32, 8, 4096, 1e-5)],
                         ids=lambda v: str(v))
def test_groupnorm_constant_groups(ops, C, G, HW, eps):
    """var = 0: every second group of every sample is one constant, chosen on the CPU so that the fp32 s2/n - mean^2 of the uncentred
    form is NEGATIVE (only the clamp keeps rstd finite); outputs finite, y = act(beta) to the mean's own error times eps^-1/2."""
    rows, silu = 2, True
    per = -(-HW // P.gn_chunks(HW))
    const, raw = P.negative_raw_constant(C, G, HW, per)
    print(f"[norm-probe] constant {const}: emulated raw variance {raw:.3e} < 0")
    x = P.draw_structure(rows, HW, C, G, 5).reshape(rows, HW, G, C // G)
    x[:, :, ::2] = const
    x = x.reshape(rows * HW, C)
    ga, be = P.gamma_beta(C, 9)
    y, st = twice(lambda: ops.groupnorm(T(x), rows, HW, G, eps, T(ga), T(be), silu))
    y, st = N(y).astype(np.float64), N(st).astype(np.float64)
    assert np.isfinite(y).all() and np.isfinite(st).all()
    g64, b64 = ga.astype(np.float64), P.silu64(be.astype(np.float64))
    err = np.abs(y - b64).reshape(rows, HW, G, C // G)[:, :, ::2]
    bound = np.broadcast_to(P.const_bound(const, g64, b64, eps), (rows * HW, C)).reshape(rows, HW, G, C // G)[:, :, ::2]
    print(f"[norm-probe] constant groups C{C} G{G} HW{HW} eps {eps:g} ({P.gn_path(C, G, HW)}): worst err/bound {(err / bound).max():.3f}")
    assert (err <= bound).all()
    assert (np.abs(st[:, ::2, 0] - const) <= P.C_M * P.U * const).all()
    assert (st[:, ::2, 1] <= eps ** -0.5 * (1 + 8 * P.U)).all() and (st[:, ::2, 1] >= (P.C_M * P.U * const * const * 2 + eps) ** -0.5 * (1 - 8 * P.U)).all()
    # the other groups are ordinary ones
    ref = P.ref_gn_fwd(x, rows, HW, G, eps, ga, be, silu)
    centred = P.gn_small_ok(C, G, HW)
    assert (np.abs(st[:, 1::2, 0] - ref["mean"][:, 1::2]) <= P.mean_bound(ref)[:, 1::2]).all()
    assert (np.abs(st[:, 1::2, 1] / ref["rstd"][:, 1::2] - 1) <= np.broadcast_to(P.rstd_bound(ref, centred), ref["mean"].shape)[:, 1::2]).all()


@pytest.mark.parametrize("C,G,HW,pair", [(320, 32, 100, False), (320, 32, 100, True), (16, 2, 6150, False), (2056, 2, 9, False)], ids=lambda v: str(v))
def test_groupnorm_stats_and_apply_alone(ops, C, G, HW, pair):
    """groupnorm_stats against the reference; groupnorm_apply fed with the REFERENCE's statistics, so an apply error cannot hide
    behind a statistics error."""
    rows, silu = 2, True
    seed = C + HW
    ga, be = P.gamma_beta(C, seed)
    x, lo = P.draw_pair(rows, HW, C, G, seed) if pair else (P.draw_sentinel(rows, HW, C, G, seed, -(-HW // P.gn_chunks(HW)))[0], None)
    ref = P.ref_gn_fwd(x, rows, HW, G, 1e-5, ga, be, silu, lo16=lo, stats_of="hi")
    xb, xv = view(rows * HW, C, 8, x)
    (st,) = twice(lambda: (ops.groupnorm_stats(xv, rows, HW, G, 1e-5),))
    st = N(st)
    P.check_stats(f"groupnorm_stats C{C} G{G} HW{HW}", st[..., 0], st[..., 1], ref, False)
    st_ref = T(P.ref_stats32(ref))
    lov = view(rows * HW, C, 8, lo)[1] if pair else None

    def run():
        ob, ov = view(rows * HW, C, 40)
        return ops.groupnorm_apply(xv, rows, HW, G, st_ref, T(ga), T(be), silu, out=ov, X_lo=lov), ob
    y, ob = twice(run)
    assert pad_intact(ob, C)
    P.check_gn_fwd(f"groupnorm_apply C{C} G{G} HW{HW} pair={pair}", N(y), ref, rows, HW, G, False, silu, given_stats=True)


def _partial(ops, x16, rows, HW, G):
    """GNPartial of the hi part in the producers' layout, synthesised in fp64 and rounded to fp32"""
    p = ops.GNPartial(rows, HW, G, dev())
    p.buf.copy_(T(P.partial_sums64(x16, rows, HW, G)[0].astype(np.float32).reshape(-1)))
    return p


@pytest.mark.parametrize("C,G,pch,pair", [(32, 8, 1, False), (32, 8, 8, False), (32, 8, 9, True), (256, 64, 2, False), (960, 32, 1, False)], ids=lambda v: str(v))
def test_groupnorm_from_partial_one_producer(ops, C, G, pch, pair):
    """The folding apply alone (gn_apply_kernel<FOLD>): 8 lanes stride over pch chunk partials (one trip, exactly one, one and a lane),
    groups = 64 takes the second trip of the 32-group fold loop, cpg 30 straddles."""
    rows, HW, silu = 2, 128 * pch, True
    ga, be = P.gamma_beta(C, C + pch)
    x, lo = P.draw_pair(rows, HW, C, G, pch) if pair else (P.draw_structure(rows, HW, C, G, pch), None)
    ref = P.ref_gn_fwd(x, rows, HW, G, 1e-5, ga, be, silu, lo16=lo, stats_of="hi")
    xv, lov, part = T(x), (T(lo) if pair else None), _partial(ops, x, rows, HW, G)

    def run():
        ob, ov = view(rows * HW, C, 8)
        if pair:
            y, st = ops.groupnorm_hilo(xv, lov, rows, HW, G, 1e-5, T(ga), T(be), silu, out=ov, want_stats=True, partial=part)
        else:
            y, st = ops.groupnorm(xv, rows, HW, G, 1e-5, T(ga), T(be), silu, out=ov, partial=part)
        return y, st, ob
    y, st, ob = twice(run)
    assert pad_intact(ob, C)
    st = N(st)
    name = f"from_partial C{C} G{G} pch{pch} pair={pair}"
    P.check_stats(name, st[..., 0], st[..., 1], ref, False)
    P.check_gn_fwd(name, N(y), ref, rows, HW, G, False, silu)


@pytest.mark.parametrize("C,G,CA,GA,GB", [(32, 4, 16, 4, 4), (32, 4, 16, 2, 4), (512, 64, 256, 64, 64)], ids=lambda v: str(v))
def test_groupnorm_from_partial_two_producers(ops, C, G, CA, GA, GB):
    """[A | B] written by two producers: ratio 2 + 2, ratio 1 + 2, and 64 output groups; the concatenation gn_concat_ok declines raises."""
    from sketch2img_amd._lib import SkgError
    rows, HW, silu = 2, 256, False
    assert ops.gn_concat_ok(CA, C - CA, G, GA, GB)
    ga, be = P.gamma_beta(C, C + GA)
    x = P.draw_structure(rows, HW, C, G, GA)
    ref = P.ref_gn_fwd(x, rows, HW, G, 1e-5, ga, be, silu)
    xv = T(x)
    pa, pb = _partial(ops, x[:, :CA], rows, HW, GA), _partial(ops, x[:, CA:], rows, HW, GB)
    y, st = twice(lambda: ops.groupnorm(xv, rows, HW, G, 1e-5, T(ga), T(be), silu, partial=(pa, CA, pb)))
    st = N(st)
    name = f"from_partial [{CA} | {C - CA}] groups {GA} + {GB} -> {G}"
    P.check_stats(name, st[..., 0], st[..., 1], ref, False)
    P.check_gn_fwd(name, N(y), ref, rows, HW, G, False, silu)
    if C == 32:
        assert not ops.gn_concat_ok(16, 32, 4, 4, 4)                   # 48 channels in 4 groups of 12: CA = 16 is no multiple of 12
        with pytest.raises(SkgError):
            ops.groupnorm(torch.zeros(rows * HW, 48, device=dev(), dtype=torch.float16), rows, HW, 4, 1e-5, T(P.gamma_beta(48, 1)[0]),
                          T(P.gamma_beta(48, 1)[1]), silu, partial=(pa, 16, _partial(ops, np.zeros((rows * HW, 32), np.float16), rows, HW, 4)))


@pytest.mark.parametrize("kind,rows,hw,K,Cout,G", [("gemm", 2, (16, 8), 32, 32, 8), ("gemm", 2, (16, 8), 64, 80, 8), ("gemm", 100, (16, 8), 64, 320, 32),
                                                   ("conv", 2, (16, 8), 64, 64, 8)], ids=lambda v: str(v))
def test_producer_epilogue_sums_then_norm(ops, kind, rows, hw, K, Cout, G):
    """gemm / conv3x3 with gn_stats= / gn_groups= at the smallest shapes gn_fusable takes (and one GEMM wide and deep enough for the
    128 x 160 tile that writes the sums from its own epilogue: 200 tiles, one K step, so no split-K): every (sample, chunk, group) entry against the fp64 sums of the fp16
    output, scaled by ITS OWN sum of |q| - not by the sample's largest sum - then the norm on those sums through the usual bounds."""
    from sketch2img_amd._lib import lib
    IH, IW = hw
    HW, M = IH * IW, rows * IH * IW
    assert ops.gn_fusable(M, Cout, HW, G)
    g = np.random.default_rng(K + Cout)
    # per-group column scales: a small group next to a large one
    colscale = np.repeat(np.asarray(P.SCALES)[np.arange(G) % len(P.SCALES)], Cout // G)
    b = T(P.to16(np.repeat(np.asarray(P.MEANS)[np.arange(G) % len(P.MEANS)], Cout // G)))
    if kind == "gemm":
        xin = T(P.to16(g.standard_normal((M, K))))
        w = T(P.to16(g.standard_normal((Cout, K)) * K ** -0.5 * colscale[:, None]))
        fused = lib.skg_gemm_gn_fused(M, Cout, K, 0, 0, HW, G)
        assert fused == (1 if Cout == 320 else 0), "the case is written for the other source of the sums"
        run = lambda: ops.gemm(xin, w, bias=b, gn_stats=(HW, G))
    else:
        xin = T(P.to16(g.standard_normal((M, K))))
        w = T(P.to16(g.standard_normal((Cout, 9 * K)) * (9 * K) ** -0.5 * colscale[:, None]))
        fused = lib.skg_gemm_gn_fused(M, Cout, 9 * K, K, 1 + ops.CONV_S1, HW, G)
        run = lambda: ops.conv3x3(xin, w, rows, IH, IW, ops.CONV_S1, bias=b, gn_groups=G)
    (y, part), (y2, part2) = run(), run()
    assert torch.equal(y, y2) and torch.equal(part.buf, part2.buf)
    y16 = N(y)
    s64, sabs = P.partial_sums64(y16, rows, HW, G)
    got = N(part.buf).astype(np.float64).reshape(s64.shape)
    r = np.abs(got - s64) / (P.C_P * P.U * sabs + 1e-300)
    print(f"[norm-probe] {kind} {M}x{Cout}x{K} G{G} (sums from the {'epilogue' if fused else 'statistics pass'}): worst partial-sum err/bound {r.max():.3f}")
    assert r.max() <= 1.0, f"partial sum entry {np.unravel_index(r.argmax(), r.shape)}: {r.max():.2f} x the bound"
    ga, be = P.gamma_beta(Cout, Cout)
    ref = P.ref_gn_fwd(y16, rows, HW, G, 1e-5, ga, be, True)
    n1, st1 = twice(lambda: ops.groupnorm(y, rows, HW, G, 1e-5, T(ga), T(be), True, partial=part))
    st1 = N(st1)
    P.check_stats(f"{kind} epilogue sums -> norm", st1[..., 0], st1[..., 1], ref, False)
    P.check_gn_fwd(f"{kind} epilogue sums -> norm", N(n1), ref, rows, HW, G, False, True)


@pytest.mark.parametrize("rows,IH,IW,C,G", P.WINO_CASES, ids=lambda v: str(v))
def test_groupnorm_wino(ops, rows, IH, IW, C, G):
    """skg_groupnorm_wino_fwd: statistics under the centred bound; V bit for bit the input transform (same add order, one fp16 rounding,
    emulated in fp32 on the CPU) of the device's own groupnorm output of the same input."""
    assert P.wino_ok(IH, IW, C, G)
    HW = IH * IW
    x = P.draw_structure(rows, HW, C, G, C + HW)
    ga, be = P.gamma_beta(C, C)
    ref = P.ref_gn_fwd(x, rows, HW, G, 1e-5, ga, be, True)
    xb, xv = view(rows * HW, C, 8, x)
    V, st = twice(lambda: ops.groupnorm_wino(xv, rows, IH, IW, G, 1e-5, T(ga), T(be), True))
    n, st0 = ops.groupnorm(xv, rows, HW, G, 1e-5, T(ga), T(be), True)
    assert torch.equal(st, st0)
    st = N(st)
    P.check_stats(f"groupnorm_wino {rows}x{IH}x{IW}x{C} G{G}", st[..., 0], st[..., 1], ref, True)
    want = P.wino_input_transform(N(n), rows, IH, IW)
    assert np.array_equal(N(V).view(np.uint16), want.view(np.uint16)), \
        f"V differs from the transform of groupnorm's output in {np.count_nonzero(N(V).view(np.uint16) != want.view(np.uint16))} elements"


def test_groupnorm_wino_declines(ops):
    from sketch2img_amd._lib import SkgError
    for (IH, IW, C, G) in [(4, 5, 64, 8), (16, 16, 2048, 8), (64, 64, 64, 8)]:      # odd IW; a 128 KiB slice; > 2560 pieces (this limit binds before the 64 KiB one)
        assert not P.wino_ok(IH, IW, C, G)
        with pytest.raises(SkgError) as e:
            ops.groupnorm_wino(torch.zeros(IH * IW, C, device=dev(), dtype=torch.float16), 1, IH, IW, G, 1e-5, T(P.gamma_beta(C, 1)[0]),
                               T(P.gamma_beta(C, 1)[1]), True)
        assert e.value.rc == -2


# ------------------------------------------------------------------------------------------------- GroupNorm backward
_BWD_REFS = {}


def _bwd_ref(C, G, HW, rows):
    if (C, G, HW, rows) not in _BWD_REFS:
        x, dy, res, ga, be = P.bwd_inputs(rows, HW, C, G)
        _BWD_REFS[(C, G, HW, rows)] = (x, dy, res, ga, be, P.ref_stats32(P.ref_gn_fwd(x, rows, HW, G, 1e-5, ga, be, True)))
    return _BWD_REFS[(C, G, HW, rows)]


@pytest.mark.parametrize("silu,resmode", [(True, "none"), (True, "res"), (False, "res-own-pitch")])
@pytest.mark.parametrize("C,G,HW,rows", P.GN_BWD, ids=lambda v: str(v))
def test_groupnorm_backward(ops, C, G, HW, rows, silu, resmode):
    x, dy, res, ga, be, st = _bwd_ref(C, G, HW, rows)
    M = rows * HW
    r16 = None if resmode == "none" else res
    rb = P.ref_gn_bwd(x, dy, rows, HW, G, st, ga, be, silu, r16)
    xv, dv = view(M, C, 8, x)[1], view(M, C, 16, dy)[1]
    rv = None if r16 is None else (T(res) if resmode == "res" else view(M, C, 32, res)[1])
    std = T(st)

    def run():
        ob, ov = view(M, C, 24)
        return ops.groupnorm_bwd(xv, dv, rows, HW, G, std, T(ga), T(be), silu, residual=rv, out=ov), ob
    dx, ob = twice(run)
    assert pad_intact(ob, C)
    P.check_gn_bwd(f"gn bwd {P.gn_bwd_path(C, G, HW)} C{C} G{G} HW{HW} silu={silu} {resmode}", N(dx), rb, rows, HW, G, silu)


@pytest.mark.parametrize("C,G,HW,rows", [(32, 4, 520, 3), (320, 32, 100, 3), (32, 8, 4096, 2)], ids=lambda v: str(v))
def test_groupnorm_backward_on_the_forward_kernels_statistics(ops, C, G, HW, rows):
    x, dy, res, ga, be, _ = _bwd_ref(C, G, HW, rows)
    _, st = ops.groupnorm(T(x), rows, HW, G, 1e-5, T(ga), T(be), True)
    rb = P.ref_gn_bwd(x, dy, rows, HW, G, N(st), ga, be, True, res)
    (dx,) = twice(lambda: (ops.groupnorm_bwd(T(x), T(dy), rows, HW, G, st, T(ga), T(be), True, residual=T(res)),))
    P.check_gn_bwd(f"gn bwd on forward statistics C{C} G{G} HW{HW}", N(dx), rb, rows, HW, G, True)


# ------------------------------------------------------------------------------------------------- LayerNorm
def _ln_check(ops, M, C, x, lo, ga, be, name):
    ref = P.ref_gn_fwd(x, M, 1, 1, 1e-5, ga, be, False, lo16=lo)
    xv = view(M, C, 8, x)[1]
    lov = view(M, C, 8, lo)[1] if lo is not None else None

    def run():
        ob, ov = view(M, C, 16)
        y, st = (ops.layernorm_hilo(xv, lov, T(ga), T(be), out=ov, want_stats=True) if lo is not None else
                 ops.layernorm(xv, T(ga), T(be), out=ov, want_stats=True))
        return y, st, ob
    y, st, ob = twice(run)
    assert pad_intact(ob, C)
    st = N(st)
    P.check_stats(name, st[:, 0], st[:, 1], ref, True)
    P.check_gn_fwd(name, N(y), ref, M, 1, 1, True, False)
    return ref, st


@pytest.mark.parametrize("M,C", P.LN_FWD, ids=lambda v: str(v))
def test_layernorm_forward(ops, M, C):
    NQ, RW = P.ln_template(C)
    _ln_check(ops, M, C, *P.ln_inputs(M, C), f"ln fwd M{M} C{C} (NQ {NQ}, {RW} rows per wave)")


@pytest.mark.parametrize("M,C", P.LN_PAIR, ids=lambda v: str(v))
def test_layernorm_forward_pair(ops, M, C):
    NQ, RW = P.ln_template(C, pair=True)
    _ln_check(ops, M, C, *P.ln_inputs(M, C, pair=True), f"ln fwd pair M{M} C{C} (NQ {NQ}, {RW} rows per wave)")


def test_layernorm_large_mean_needs_no_kappa_allowance(ops):
    """mu / sigma = 64 (kappa ~ 4100): a centred kernel stays inside the kappa-free bound"""
    for C in (512, 1280):
        ref, _ = _ln_check(ops, 9, C, *P.ln_inputs(9, C, ratio=64.0), f"ln fwd mu/sigma 64 C{C}")
        assert ref["kappa"].min() > 3000


def test_layernorm_rejects_wide_rows(ops):
    from sketch2img_amd._lib import SkgError
    with pytest.raises(ValueError):
        P.ln_template(2056)
    with pytest.raises(SkgError):
        ops.layernorm(torch.zeros(3, 2056, device=dev(), dtype=torch.float16), torch.ones(2056, device=dev(), dtype=torch.float16),
                      torch.zeros(2056, device=dev(), dtype=torch.float16))


@pytest.mark.parametrize("resmode", ["none", "res-own-pitch"])
@pytest.mark.parametrize("M,C", [(M, C) for C in (8, 504, 512, 520, 1024, 1032, 2040, 2048) for M in (5, 17)], ids=lambda v: str(v))
def test_layernorm_backward(ops, M, C, resmode):
    x, _, ga, be = P.ln_inputs(M, C)
    r = np.random.default_rng(M * C)
    dy, res = P.to16(r.standard_normal(x.shape)), (P.to16(r.standard_normal(x.shape)) if resmode != "none" else None)
    st = P.ref_stats32(P.ref_gn_fwd(x, M, 1, 1, 1e-5, ga, be, False)).reshape(M, 2)
    rb = P.ref_gn_bwd(x, dy, M, 1, 1, st, ga, None, False, res)
    xv, dv, rv = view(M, C, 8, x)[1], view(M, C, 16, dy)[1], (view(M, C, 32, res)[1] if res is not None else None)

    def run():
        ob, ov = view(M, C, 24)
        return ops.layernorm_bwd(xv, dv, T(ga), T(st), residual=rv, out=ov), ob
    dx, ob = twice(run)
    assert pad_intact(ob, C)
    P.check_gn_bwd(f"ln bwd M{M} C{C} {resmode}", N(dx), rb, M, 1, 1, False)


def test_layernorm_backward_on_the_forward_kernels_statistics(ops):
    M, C = 17, 1032
    x, _, ga, be = P.ln_inputs(M, C)
    dy = P.to16(np.random.default_rng(3).standard_normal(x.shape))
    _, st = ops.layernorm(T(x), T(ga), T(be), want_stats=True)
    rb = P.ref_gn_bwd(x, dy, M, 1, 1, N(st), ga, None, False, None)
    P.check_gn_bwd("ln bwd on forward statistics", N(ops.layernorm_bwd(T(x), T(dy), T(ga), st)), rb, M, 1, 1, False)


# ------------------------------------------------------------------------------------------------- BatchNorm
@pytest.mark.parametrize("S,segs,seg_rows,C", P.BN_CASES, ids=lambda v: str(v))
def test_batchnorm(ops, S, segs, seg_rows, C):
    """bn_stats (train, with the running-statistics recurrence over the S samples in order), bn_apply, bn_relu_bwd (train and running);
    channel 5 is a constant."""
    x, ga, be, dy = P.bn_inputs(S, segs, seg_rows, C)
    n, M = segs * seg_rows, S * segs * seg_rows
    rb = P.ref_bn(x, S, segs, seg_rows, 1e-5, ga, be)
    r = np.random.default_rng(C)
    rm0, rv0 = (0.1 * r.standard_normal(C)).astype(np.float32), (1 + 0.1 * r.random(C)).astype(np.float32)
    xv = view(M, C, 8, x)[1]

    def stats():
        rm, rv = T(rm0), T(rv0)
        return ops.bn_stats(xv, S, segs, seg_rows, 1e-5, rm, rv), rm, rv
    st, rm, rv = twice(stats)
    stn = N(st).astype(np.float64)
    assert np.isfinite(stn).all()
    live = np.arange(C) != 5
    name = f"bn S{S} segs{segs} rows{seg_rows} C{C}"
    em = np.abs(stn[..., 0] - rb["mean"]) / (P.C_M * P.U * np.maximum(np.abs(rb["mean"]), rb["sigma"]))
    er = (np.abs(stn[..., 1] / rb["rstd"] - 1) / (P.C_R * P.U * rb["kappa"] + 4 * P.U))[:, live]
    print(f"[norm-probe] {name}: mean err/bound {em.max():.3f}, rstd err/bound {er.max():.3f} (kappa max {rb['kappa'][:, live].max():.1f}, uncentred)")
    assert em.max() <= 1 and er.max() <= 1
    # running statistics: S successive batches, momentum 0.1, unbiased variance
    rm64, rv64 = P.ref_bn_running(rb["mean"], rb["var"], n, rm0, rv0)
    w = 0.1 * 0.9 ** np.arange(S - 1, -1, -1)[:, None]
    bm = (w * P.C_M * P.U * np.maximum(np.abs(rb["mean"]), rb["sigma"])).sum(0) + 4 * S * P.U * np.maximum(np.abs(rm64), np.abs(rm0))
    bv = (w * n / (n - 1) * 2 * (P.C_R * P.U * (rb["var"] + rb["mean"] ** 2) + 4 * P.U * rb["var"])).sum(0) + 4 * S * P.U * np.maximum(np.abs(rv64), np.abs(rv0))
    assert (np.abs(N(rm) - rm64) <= bm).all() and (np.abs(N(rv) - rv64) <= bv).all()
    # apply, on the kernel's statistics of the live channels and on the reference's
    for tag, sd in (("own statistics", st), ("reference statistics", T(np.stack([rb["mean"], rb["rstd"]], -1).astype(np.float32)))):
        def run():
            ob, ov = view(M, C, 16)
            return ops.bn_apply(xv, S, segs, seg_rows, sd, T(ga), T(be), out=ov), ob
        y, ob = twice(run)
        assert pad_intact(ob, C)
        mag, prop = P.bn_terms(rb, ga, be, x, S, segs, seg_rows, given_stats=tag.startswith("ref"))
        yl, refl = N(y).astype(np.float64)[:, live], rb["y"][:, live]
        P.check_out(f"{name} apply, {tag}", yl, refl, (P.K_FWD * mag + prop)[:, live])
        if tag == "own statistics":
            cb = P.const_bound(x[:, 5].astype(np.float64), float(ga[5]), float(be[5]), 1e-5) / P.SILU_GRAD_MAX
            assert np.isfinite(N(y)[:, 5]).all() and (np.abs(N(y)[:, 5].astype(np.float64) - float(be[5])) <= cb).all()
    # statistics from the running buffers: mean = running_mean, rstd = (running_var + eps)^-1/2 to rsqrtf's 4 u
    sr_ = N(ops.bn_stats_from_running(T(rm0), T(rv0), S)).astype(np.float64)
    assert sr_.shape == (S, C, 2) and (sr_[..., 0] == rm0).all()
    assert (np.abs(sr_[..., 1] * np.sqrt(rv0.astype(np.float64) + 1e-5) - 1) <= 6 * P.U).all()
    # backward through the preceding ReLU, statistics given
    sref = np.stack([rb["mean"], rb["rstd"]], -1).astype(np.float32)
    for train in (True, False):
        rbb = P.ref_bn(x, S, segs, seg_rows, 1e-5, ga, be, dy, train, sref)
        (dx,) = twice(lambda: (ops.bn_relu_bwd(xv, T(dy), S, segs, seg_rows, T(sref), T(ga), train),))
        term = P.K_BWD * P.U * (rbb["mag"] + np.abs(rbb["dx"])) + P.bn_bwd_prop(rbb, ga, sref, x, S, segs, seg_rows)
        P.check_out(f"{name} relu bwd train={train}", N(dx).astype(np.float64)[:, live], rbb["dx"][:, live], term[:, live])


# ------------------------------------------------------------------------------------------------- instance norm
@pytest.mark.parametrize("rows,HW,C", P.IN_CASES, ids=lambda v: str(v))
def test_instance_norm(ops, rows, HW, C):
    """skg_instnorm_act_f16 on both sides of its launcher's forks: one slab (HW <= 256, one launch) | several (three launches),
    256-pixel slabs | longer ones (HW > 65536); C = 64 | 128 (one | two channel blocks).  Both outputs, slopes (0.2, 0) and (1, 0.2)."""
    slab = P.in_slab(HW)
    nsl = -(-HW // slab)
    x = P.in_inputs(rows, HW, C)
    xv = view(rows * HW, C, 8, x)[1]
    for s0, s1 in ((0.2, 0.0), (1.0, 0.2)):
        def run():
            b0, v0 = view(rows * HW, C, 8)
            b1, v1 = view(rows * HW, C, 24)
            ops.instnorm_act(xv, rows, HW, v0, s0, v1, s1)
            return b0, b1
        b0, b1 = twice(run)
        assert pad_intact(b0, C) and pad_intact(b1, C)
        for buf, slope in ((b0, s0), (b1, s1)):
            ref = P.ref_instnorm(x, rows, HW, 1e-5, slope)
            got = N(buf[:, :C]).astype(np.float64)
            assert np.isfinite(got).all()
            r = np.abs(got - ref["y"]) / P.instnorm_out_bound(ref, HW, slope)
            print(f"[norm-probe] instnorm r{rows} HW{HW} C{C} ({nsl} slab{'s' if nsl > 1 else ''} of {slab}) slope {slope}: worst err/bound {r.max():.3f}")
            assert r.max() <= 1.0, f"element {np.unravel_index(r.argmax(), r.shape)}: {r.max():.2f} x the bound"
    if nsl > 1:      # the statistics are published only on the three-launch route: [rows][C][2] behind the slab partials of the scratch
        nfl = ops.lib.skg_instnorm_scratch_floats(rows, HW, C)
        st = N(ops._scratch_buf(("in", ops._skey(dev()), nfl), nfl, dev())[rows * nsl * C * 2:]).reshape(rows, C, 2).astype(np.float64)
        ref = P.ref_instnorm(x, rows, HW, 1e-5, 0.0)
        em = np.abs(st[..., 0] - ref["mean"]) / (P.C_M_IN * P.U * np.maximum(np.abs(ref["mean"]), ref["sigma"]))
        er = np.abs(st[..., 1] / ref["rstd"] - 1) / (P.C_R_IN * P.U * ref["kappa"] + 4 * P.U)
        print(f"[norm-probe] instnorm r{rows} HW{HW} C{C}: mean err/bound {em.max():.3f}, rstd err/bound {er.max():.3f}")
        assert em.max() <= 1 and er.max() <= 1


# ------------------------------------------------------------------------------------------------- the kappa statement
@pytest.mark.parametrize("case", P.GN_KAPPA, ids=lambda c: c.id)
def test_uncentred_paths_lose_log2_kappa_bits_and_no_more(ops, case):
    """N(mu, 1) with mu / sigma in {4, 16, 64} on the two uncentred forward routes: the kappa-scaled bounds hold; the achieved
    error / (2^-24 kappa) is printed."""
    c = case
    x, lo, ga, be = c.inputs()
    ref = c.ref(x, lo, ga, be)
    y, st = twice(lambda: ops.groupnorm(T(x), c.rows, c.HW, c.G, c.eps, T(ga), T(be), c.silu))
    st = N(st)
    rm, rr = P.stat_ratios(st[..., 0], st[..., 1], ref, False)
    print(f"[norm-probe] kappa statement {c.id}: kappa {ref['kappa'].mean():.0f}, rstd error / (2^-24 kappa) {rr.max():.2f}, mean error / (2^-24 max(|mean|, sigma)) {rm.max():.2f}")
    P.check_stats(c.id, st[..., 0], st[..., 1], ref, False)
    P.check_gn_fwd(c.id, N(y), ref, c.rows, c.HW, c.G, False, c.silu)
