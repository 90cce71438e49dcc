"""The yardstick of test_gpu_norm_probes.py, checked on the CPU: the fp64 references against torch in float64, the fp32 emulation
inside every bound with the recorded constants on every case of the GPU file, the launcher arithmetic the case ids rely on - and the
MUTANTS: deliberate errors of the kind a kernel can have, applied to the emulation's output, each of which the comparators must
reject.  Next to every mutant the relative Frobenius error that tests/test_gpu_kernels.py compares with FP16_RND is printed: the
single-pixel and single-store mutants PASS that criterion, which is why the per-group / per-element comparators exist."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import norm_probes as P

FP16_RND = 6e-4      # the whole-tensor criterion of test_groupnorm_fwd_bwd / test_layernorm_fwd_bwd (twice that backward)


def _nchw(a, rows, HW):
    return torch.from_numpy(np.asarray(a, np.float64)).reshape(rows, HW, -1).permute(0, 2, 1).contiguous()


def _tok(t):
    return t.permute(0, 2, 1).reshape(-1, t.shape[1]).numpy()


# ------------------------------------------------------------------------------------------------- references vs torch, float64
@pytest.mark.parametrize("C,G,HW,silu", [(320, 32, 100, True), (32, 4, 257, False), (48, 8, 7, True)])
def test_groupnorm_reference_is_torch_float64(C, G, HW, silu):
    rows = 3
    x, dy, res, ga, be = P.bwd_inputs(rows, HW, C, G)
    ref = P.ref_gn_fwd(x, rows, HW, G, 1e-5, ga, be, silu)
    xt = _nchw(x, rows, HW).requires_grad_(True)
    y = F.group_norm(xt, G, torch.from_numpy(ga.astype(np.float64)), torch.from_numpy(be.astype(np.float64)), 1e-5)
    y = F.silu(y) if silu else y
    y.backward(_nchw(dy, rows, HW))
    assert np.abs(_tok(y.detach()) - ref["y"]).max() < 1e-12
    xg = x.astype(np.float64).reshape(rows, HW, G, -1)
    assert np.abs(xg.mean(axis=(1, 3)) - ref["mean"]).max() < 1e-12 and np.abs(xg.var(axis=(1, 3)) - ref["var"]).max() < 1e-12
    rb = P.ref_gn_bwd(x, dy, rows, HW, G, np.stack([ref["mean"], ref["rstd"]], -1), ga, be, silu, res)
    assert np.abs(_tok(xt.grad) + res.astype(np.float64) - rb["dx"]).max() < 1e-12 * max(1.0, np.abs(rb["dx"]).max())


def test_layernorm_reference_is_torch_float64():
    M, C = 17, 520
    x, _, ga, be = P.ln_inputs(M, C)
    dy = P.to16(np.random.default_rng(1).standard_normal(x.shape))
    ref = P.ref_gn_fwd(x, M, 1, 1, 1e-5, ga, be, False)
    xt = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    y = F.layer_norm(xt, (C,), torch.from_numpy(ga.astype(np.float64)), torch.from_numpy(be.astype(np.float64)), 1e-5)
    y.backward(torch.from_numpy(dy.astype(np.float64)))
    assert np.abs(y.detach().numpy() - ref["y"]).max() < 1e-12
    rb = P.ref_gn_bwd(x, dy, M, 1, 1, np.stack([ref["mean"], ref["rstd"]], -1), ga, None, False, None)
    assert np.abs(xt.grad.numpy() - rb["dx"]).max() < 1e-12 * max(1.0, np.abs(rb["dx"]).max())


def test_batchnorm_reference_is_torch_float64():
    S, segs, sr, C = 2, 3, 37, 64
    x, ga, be, dy = P.bn_inputs(S, segs, sr, C, const_channel=False)
    rb = P.ref_bn(x, S, segs, sr, 1e-5, ga, be)
    rbb = P.ref_bn(x, S, segs, sr, 1e-5, ga, be, dy, True, np.stack([rb["mean"], rb["rstd"]], -1))
    rm, rv = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
    for g in range(S):
        idx = P.bn_rows(S, segs, sr, g)
        pre = torch.from_numpy(x.astype(np.float64)[idx]).requires_grad_(True)
        y = F.batch_norm(torch.relu(pre), rm, rv, torch.from_numpy(ga.astype(np.float64)), torch.from_numpy(be.astype(np.float64)), True, 0.1, 1e-5)
        y.backward(torch.from_numpy(dy.astype(np.float64)[idx]))
        assert np.abs(y.detach().numpy() - rb["y"][idx]).max() < 1e-12
        assert np.abs(pre.grad.numpy() * (x[idx] > 0) - rbb["dx"][idx]).max() < 1e-12 * max(1.0, np.abs(rbb["dx"]).max())
    rm64, rv64 = P.ref_bn_running(rb["mean"], rb["var"], segs * sr, np.zeros(C), np.ones(C))
    assert np.abs(rm.numpy() - rm64).max() < 1e-12 and np.abs(rv.numpy() - rv64).max() < 1e-12
    # the row order of a sample: segment-major, samples interleaved inside a segment
    assert list(P.bn_rows(2, 2, 3, 1)) == [3, 4, 5, 9, 10, 11]


def test_instance_norm_reference_is_torch_float64():
    rows, HW, C = 2, 257, 64
    x = P.in_inputs(rows, HW, C)
    ref = P.ref_instnorm(x, rows, HW, 1e-5, 0.2)
    y = F.leaky_relu(F.instance_norm(_nchw(x, rows, HW), eps=1e-5), 0.2)
    assert np.abs(_tok(y) - ref["y"]).max() < 1e-12


# ------------------------------------------------------------------------------------------------- launcher arithmetic
def test_case_ids_name_the_path_the_launchers_take():
    assert [P.gn_small_np(32, 4, hw) for hw in (512, 520, 768, 776, 1280, 1288, 2560)] == [2, 3, 3, 5, 5, 10, 10]
    assert P.gn_path(32, 4, 2560) == "small-NP10" and P.gn_path(32, 4, 2568) == "two-launch"
    # two shapes the issue lists under the two-launch path are small-path shapes; the substitutes are not
    assert P.gn_path(2560, 32, 49).startswith("small") and P.gn_path(4096, 64, 5).startswith("small")
    assert P.gn_path(768, 64, 50) == "two-launch" and P.gn_path(4096, 64, 328) == "two-launch" and P.gn_bwd_path(4096, 64, 328) == "chunked"
    assert P.gn_path(320, 32, 4096) == "three-launch" and P.gn_chunks(4096) == 86 and P.gn_chunks(6150) == 128
    assert P.has_empty_chunk(6150, P.gn_chunks(6150))                                  # stage 1 under the 128-chunk cap
    assert P.gn_lanes(2080) == 1 and P.gn_apply_chunks(90, 2080) == 11 and P.has_empty_chunk(90, 11)      # the apply grid
    assert not any(P.has_empty_chunk(hw, P.gn_chunks(hw)) for hw in range(1, 6145))     # below the cap stage 1 has none
    assert P.gn_lanes(320) == 6 and P.gn_lanes(960) == 2 and P.gn_lanes(8) == 256
    assert [p for p, _ in P.straddling_pieces(320, 32)][:3] == [1, 2, 3] and P.straddling_pieces(32, 4) == []
    assert P.ln_template(512) == (1, 4) and P.ln_template(520) == (2, 2) and P.ln_template(1032) == (4, 1) and P.ln_template(512, True) == (1, 2)
    assert P.in_slab(65536) == 256 and P.in_slab(65537) == 288
    paths = {c.path for c in P.GN_FWD}
    assert paths == {"small-NP2", "small-NP3", "small-NP5", "small-NP10", "two-launch", "three-launch"}
    assert all(P.wino_ok(ih, iw, c, g) for (_, ih, iw, c, g) in P.WINO_CASES)


# ------------------------------------------------------------------------------------------------- the emulation inside the bounds
@pytest.fixture(scope="module")
def cal():
    return P.calibrate()


def test_recorded_constants_are_four_times_the_emulations_worst_ratio(cal):
    print("\n".join(cal.lines))
    for name, rec, got in (("C_M", P.C_M, cal.m), ("C_R", P.C_R, cal.r), ("K_FWD", P.K_FWD, cal.kf), ("K_BWD", P.K_BWD, cal.kb),
                           ("C_M_IN", P.C_M_IN, cal.m_in), ("C_R_IN", P.C_R_IN, cal.r_in), ("C_P", P.C_P, cal.p)):
        print(f"{name}: recorded {rec}, 4 x the emulation's worst ratio {4 * got:.2f}")
        assert 4 * got <= rec <= 4 * got * 1.05 + 1, name


@pytest.mark.parametrize("case", P.GN_FWD + P.GN_KAPPA, ids=lambda c: c.id)
def test_emulation_meets_the_forward_bounds(case):
    c = case
    x, lo, ga, be = c.inputs()
    ref, e = c.ref(x, lo, ga, be), c.emu(x, lo, ga, be)
    P.check_stats(c.id, e["mean"], e["rstd"], ref, c.centred)
    P.check_gn_fwd(c.id, e["y16"], ref, c.rows, c.HW, c.G, c.centred, c.silu)
    if c.pair_out:
        P.check_lo(c.id, e["y16"], e["lo16"], ref, c.rows, c.HW, c.G, c.centred, c.silu)
    assert ref["kappa"].max() <= 20 or c.draw.startswith("cond")
    if c.draw == "sentinel":      # losing one sentinel must move the group mean by more than 8 x the bound, else the case proves nothing
        _, pos = P.draw_sentinel(c.rows, c.HW, c.C, c.G, 0, c.per)
        assert len(pos) >= 2
        assert (P.SENTINEL / ref["n"] > 8 * P.mean_bound(ref)).all(), f"{c.id}: 48 / n = {P.SENTINEL / ref['n']:.2e} against 8 x {P.mean_bound(ref).max():.2e}"


@pytest.mark.parametrize("C,G,HW,rows", P.GN_BWD, ids=lambda v: str(v))
def test_emulation_meets_the_backward_bounds(C, G, HW, rows):
    x, dy, res, ga, be = P.bwd_inputs(rows, HW, C, G)
    st = P.ref_stats32(P.ref_gn_fwd(x, rows, HW, G, 1e-5, ga, be, True))
    for silu, r in ((True, None), (True, res), (False, res)):
        rb = P.ref_gn_bwd(x, dy, rows, HW, G, st, ga, be, silu, r)
        eb = P.emu_gn_bwd(x, dy, rows, HW, G, st, ga, be, silu, r, per=-(-HW // P.gn_chunks(HW)))
        P.check_gn_bwd(f"emulation gn bwd C{C} G{G} HW{HW} silu={silu}", eb["dx16"], rb, rows, HW, G, silu)


def test_emulation_meets_the_layernorm_batchnorm_and_instance_norm_bounds():
    for (M, C) in P.LN_FWD + P.LN_PAIR:
        x, lo, ga, be = P.ln_inputs(M, C, pair=(M, C) in P.LN_PAIR)
        ref, e = P.ref_gn_fwd(x, M, 1, 1, 1e-5, ga, be, False, lo16=lo), P.emu_gn_fwd(x, M, 1, 1, 1e-5, ga, be, False, centred=True, lo16=lo)
        P.check_stats(f"ln M{M} C{C}", e["mean"], e["rstd"], ref, True)
        P.check_gn_fwd(f"ln M{M} C{C}", e["y16"], ref, M, 1, 1, True, False)
    for (S, segs, sr, C) in P.BN_CASES:
        x, ga, be, dy = P.bn_inputs(S, segs, sr, C, const_channel=False)
        rb, e = P.ref_bn(x, S, segs, sr, 1e-5, ga, be), P.emu_bn(x, S, segs, sr, 1e-5, ga, be)
        rm, rr = P.stat_ratios(e["mean"], e["rstd"], rb, False)
        assert rm.max() <= P.C_M and (np.abs(e["rstd"] / rb["rstd"] - 1) <= P.C_R * P.U * rb["kappa"] + 4 * P.U).all()
        mag, prop = P.bn_terms(rb, ga, be, x, S, segs, sr)
        P.check_out(f"emulation bn C{C}", e["y16"], rb["y"], P.K_FWD * mag + prop)
    for (rows, HW, C) in P.IN_CASES[:3]:
        x = P.in_inputs(rows, HW, C)
        for slope in (0.2, 0.0, 1.0):
            ref, e = P.ref_instnorm(x, rows, HW, 1e-5, slope), P.emu_instnorm(x, rows, HW, 1e-5, slope)
            assert (np.abs(e["y16"].astype(np.float64) - ref["y"]) <= P.instnorm_out_bound(ref, HW, slope)).all()


def test_a_constant_with_a_negative_raw_variance_exists_and_the_emulation_meets_the_constant_bound():
    C, G, HW, eps = 320, 32, 100, 1e-5
    const, raw = P.negative_raw_constant(C, G, HW, 34)
    assert raw < 0
    x = np.full((HW, C), const, np.float16)
    ga, be = P.gamma_beta(C, 9)
    e = P.emu_gn_fwd(x, 1, HW, G, eps, ga, be, True, centred=False, per=34)
    b64 = P.silu64(be.astype(np.float64))
    assert np.isfinite(e["y16"]).all()
    assert (np.abs(e["y16"].astype(np.float64) - b64) <= P.const_bound(const, ga.astype(np.float64), b64, eps)).all()


# ------------------------------------------------------------------------------------------------- mutants
def _rejected(fn):
    with pytest.raises(AssertionError):
        fn()


def _old(name, got16, ref64, bound=FP16_RND):
    f = P.frob(got16, ref64)
    print(f"[mutant] {name}: relative Frobenius error {f:.2e} against FP16_RND-based bound {bound:.1e} -> the old criterion {'ACCEPTS' if f < bound else 'rejects'} it")
    return f


SMALL = P.GN(320, 32, 100, draw="sentinel")               # cpg 10: straddling pieces, 3 chunks of 34 pixels
BIG = {"drop_last_pixel": P.GN(320, 32, 4096, rows=2, draw="cond0.3"), "one_store": P.GN(320, 32, 4096, rows=2)}             # the 64 x 64 level: where one pixel or one store drowns in the whole-tensor norm


@pytest.mark.parametrize("mutant,stats_only", [("drop_last_pixel", True), ("drop_chunk_last_pixel", True), ("nlo_off2", False),
                                               ("hi_from_lo", False), ("prev_sample", True)])
def test_forward_mutants_are_rejected(mutant, stats_only):
    c = SMALL
    x, lo, ga, be = c.inputs()
    ref, good, bad = c.ref(x, lo, ga, be), c.emu(x, lo, ga, be), c.emu(x, lo, ga, be, mutant=mutant)
    P.check_stats("unmutated", good["mean"], good["rstd"], ref, False)
    P.check_gn_fwd("unmutated", good["y16"], ref, c.rows, c.HW, c.G, False, c.silu)
    _old(f"{mutant} on {c.id}", bad["y16"], ref["y"])
    if stats_only:
        _rejected(lambda: P.check_stats(mutant, bad["mean"], bad["rstd"], ref, False))
    _rejected(lambda: P.check_gn_fwd(mutant, bad["y16"], ref, c.rows, c.HW, c.G, False, c.silu))


@pytest.mark.parametrize("mutant", ["drop_last_pixel", "one_store"])
def test_single_pixel_and_single_store_mutants_pass_the_old_criterion_and_fail_the_new(mutant):
    """One dropped pixel of 4096 in the statistics; one 8-channel store (the first straddling piece of the first pixel) normalised
    with an nlo off by two.  Both stay under FP16_RND = 6e-4 in the whole-tensor norm; both are caught here."""
    c = BIG[mutant]      # N(0.3, 1) as in test_groupnorm_fwd_bwd for the dropped pixel; per-group structure for the wrong-group store
    x, lo, ga, be = c.inputs()
    ref, good, bad = c.ref(x, lo, ga, be), c.emu(x, lo, ga, be), c.emu(x, lo, ga, be, mutant=mutant)
    assert _old(f"unmutated {c.id}", good["y16"], ref["y"]) < FP16_RND
    assert _old(f"{mutant} on {c.id}", bad["y16"], ref["y"]) < FP16_RND
    P.check_stats("unmutated", good["mean"], good["rstd"], ref, False)
    P.check_gn_fwd("unmutated", good["y16"], ref, c.rows, c.HW, c.G, False, c.silu)
    if mutant == "drop_last_pixel":      # ordinary data, no sentinel: the statistics bound alone catches one pixel of 4096
        _rejected(lambda: P.check_stats(mutant, bad["mean"], bad["rstd"], ref, False))
    else:
        _rejected(lambda: P.check_gn_fwd(mutant, bad["y16"], ref, c.rows, c.HW, c.G, False, c.silu))


def test_eps_and_clamp_mutants_are_rejected():
    c = P.GN(320, 32, 100, eps=1e-3, silu=False, note="eps")
    x, lo, ga, be = c.inputs()
    ref, good, bad = c.ref(x, lo, ga, be), c.emu(x, lo, ga, be), c.emu(x, lo, ga, be, mutant="eps_dropped")
    P.check_stats("unmutated", good["mean"], good["rstd"], ref, False)
    _old("eps dropped (eps = 1e-3)", bad["y16"], ref["y"])
    _rejected(lambda: P.check_stats("eps_dropped", bad["mean"], bad["rstd"], ref, False))
    # the clamp: a constant whose raw fp32 variance is below -eps gives rsqrt of a negative number without it
    const, raw = P.negative_raw_constant(320, 32, 100, 34)
    assert raw < -1e-5
    xc = np.full((100, 320), const, np.float16)
    bad = P.emu_gn_fwd(xc, 1, 100, 32, 1e-5, ga, be, False, centred=False, per=34, mutant="no_clamp")
    assert np.isnan(bad["rstd"]).any() and np.isnan(bad["y16"]).any()
    refc = P.ref_gn_fwd(xc, 1, 100, 32, 1e-5, ga, be, False)
    _rejected(lambda: P.check_stats("no_clamp", bad["mean"], bad["rstd"], refc, False))
    _rejected(lambda: P.check_out("no_clamp", bad["y16"], refc["y"], 1.0))


@pytest.mark.parametrize("mutant", ["silu_grad_1", "no_res_last_row", "m2_with_x"])
def test_backward_mutants_are_rejected(mutant):
    C, G, HW, rows = 320, 32, 100, 3
    x, dy, res, ga, be = P.bwd_inputs(rows, HW, C, G)
    st = P.ref_stats32(P.ref_gn_fwd(x, rows, HW, G, 1e-5, ga, be, True))
    rb = P.ref_gn_bwd(x, dy, rows, HW, G, st, ga, be, True, res)
    good, bad = (P.emu_gn_bwd(x, dy, rows, HW, G, st, ga, be, True, res, per=34, mutant=m) for m in (None, mutant))
    P.check_gn_bwd("unmutated", good["dx16"], rb, rows, HW, G, True)
    _old(f"{mutant} (backward)", bad["dx16"], rb["dx"], 2 * FP16_RND)
    _rejected(lambda: P.check_gn_bwd(mutant, bad["dx16"], rb, rows, HW, G, True))


def test_layernorm_mutants_are_rejected():
    M, C = 5, 512
    x, _, ga, be = P.ln_inputs(M, C)
    ref, good = P.ref_gn_fwd(x, M, 1, 1, 1e-5, ga, be, False), P.emu_gn_fwd(x, M, 1, 1, 1e-5, ga, be, False, centred=True)
    P.check_gn_fwd("unmutated", good["y16"], ref, M, 1, 1, True, False)
    unwritten = good["y16"].copy()
    unwritten[M - 1] = 123.5                                  # the pattern the output buffer held before the launch
    _old("LayerNorm row M - 1 not written", unwritten, ref["y"])
    _rejected(lambda: P.check_gn_fwd("row_unwritten", unwritten, ref, M, 1, 1, True, False))
    # uncentred statistics at mu / sigma = 64 need the kappa allowance a centred kernel must not need
    x, _, ga, be = P.ln_inputs(9, C, ratio=64.0)
    ref = P.ref_gn_fwd(x, 9, 1, 1, 1e-5, ga, be, False)
    good, bad = (P.emu_gn_fwd(x, 9, 1, 1, 1e-5, ga, be, False, centred=True, mutant=m) for m in (None, "uncentred"))
    P.check_stats("centred at mu/sigma 64", good["mean"], good["rstd"], ref, True)
    _old("uncentred LayerNorm statistics at mu/sigma 64", bad["y16"], ref["y"])
    _rejected(lambda: P.check_stats("uncentred", bad["mean"], bad["rstd"], ref, True))
    P.check_stats("the same under the kappa-scaled bound", bad["mean"], bad["rstd"], ref, False)


def test_batchnorm_swapped_segments_are_rejected():
    S, segs, sr, C = 2, 2, 129, 512
    x, ga, be, dy = P.bn_inputs(S, segs, sr, C, const_channel=False)
    rb = P.ref_bn(x, S, segs, sr, 1e-5, ga, be)
    mag, prop = P.bn_terms(rb, ga, be, x, S, segs, sr)
    good, bad = (P.emu_bn(x, S, segs, sr, 1e-5, ga, be, mutant=m) for m in (None, "segs_swapped"))
    P.check_out("unmutated", good["y16"], rb["y"], P.K_FWD * mag + prop)
    _old("BatchNorm segments swapped", bad["y16"], rb["y"])
    _rejected(lambda: P.check_out("segs_swapped", bad["y16"], rb["y"], P.K_FWD * mag + prop))


def test_wino_transform_emulation_matches_the_matrix_form():
    rows, IH, IW, C = 2, 4, 6, 16
    n = P.to16(np.random.default_rng(2).standard_normal((rows * IH * IW, C)))
    Bt = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], np.float64)
    pad = np.zeros((rows, IH + 2, IW + 2, C))
    pad[:, 1:-1, 1:-1] = n.astype(np.float64).reshape(rows, IH, IW, C)
    V = P.wino_input_transform(n, rows, IH, IW).astype(np.float64).reshape(rows, IH // 2, IW // 2, 4, 4, C)
    for ti in range(IH // 2):
        for tj in range(IW // 2):
            d = pad[:, 2 * ti:2 * ti + 4, 2 * tj:2 * tj + 4]
            want = np.einsum("ia,rabc,jb->rijc", Bt, d, Bt)
            assert np.abs(V[:, ti, tj] - want).max() <= 2.0 ** -10 * np.abs(want).max()
