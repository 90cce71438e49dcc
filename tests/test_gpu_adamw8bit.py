"""The 8-bit AdamW state on the GPU (-m gpu): skg_adamw8_step against the numpy checker (tests/adamw8bit_ref.py: codes, absmax) and
against skg_adamw_step run on the dequantised old state (masters, fp16 copy, the small tensors' fp32 moments), on the mixed layout of
tests/test_host_adamw8bit.py; FlatAdamW(state_bits=8) under the LGP trainer: first step, scaler, checkpoint, memory, convergence.

Bit equality wherever the arithmetic is the same by construction.  The two exceptions are stated where they are used: codes and absmax
of the random steps (the checker's fused multiply-add goes through float64) and the convergence margin."""
import numpy as np
import pytest
import torch

from tests import adamw8bit_ref as ref
from tests.test_gpu_sat_train import B, DEV, e2e  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

HYPER = dict(lr=1e-3, eps=1e-8, weight_decay=1e-2)
P_PAD, H_PAD, C_PAD, M_PAD = 777.0, 555.0, 0xAB, 333.0           # sentinels in the padding of p, p16, the codes, the small moments


@pytest.fixture(scope="module")
def ops():
    from sketch2img_amd import ops as o
    return o


def _opt(bits=8, betas=(0.9, 0.999), grad_scale=8.0, shapes=ref.MIXED, frozen=("frozen",), seed=3, **kw):
    from sketch2img_amd import flat_adamw
    g = torch.Generator().manual_seed(seed)
    sd = {k: torch.randn(shp, generator=g) for k, shp in shapes}
    return flat_adamw.FlatAdamW(shapes, sd, DEV, betas=betas, schedule=lambda s: 1.0, grad_scale=grad_scale, frozen=set(frozen),
                                state_bits=bits, **dict(HYPER, **kw))


def _inside(st):
    """Boolean masks over the flat vector: elements of optimised tensors, and everything else (padding, frozen keys)."""
    mask = np.zeros(st.n, dtype=bool)
    for k, (off, shp) in st.layout.items():
        mask[off:off + shp.numel()] = off < st.n_opt
    return mask


def _state_masks(st):
    """Boolean masks of the elements of the code arrays and of the compact fp32 arrays that belong to a tensor."""
    c, s = np.zeros(st.state1.numel(), dtype=bool), np.zeros(st.m32.numel(), dtype=bool)
    for k, (is8, so, r0, nr) in st.spans.items():
        (c if is8 else s)[so:so + st.layout[k][1].numel()] = True
    return c, s


def _sentinels(st):
    """Mark everything no row may touch: padding of p / p16 (and the frozen key keeps its values), of the codes, of m32 / v32."""
    pad = torch.from_numpy(~_inside(st)).to(DEV)
    frozen = torch.zeros_like(pad)
    o, shp = st.layout["frozen"]
    frozen[o:o + shp.numel()] = True
    st.p[pad & ~frozen] = P_PAD
    st.p16[pad & ~frozen] = H_PAD
    c, s = (torch.from_numpy(~m).to(DEV) for m in _state_masks(st))
    st.state1[c] = C_PAD
    st.state2[c] = C_PAD
    st.m32[s] = M_PAD
    st.v32[s] = M_PAD


BUFS = ("p", "p16", "state1", "state2", "absmax1", "absmax2", "m32", "v32")


def _snap(st):
    return {n: getattr(st, n).clone() for n in BUFS}


def _same(a, b):
    return [n for n in BUFS if not torch.equal(a[n], b[n])]


def _old_moments(st):
    """The flat fp32 m, v the state stands for, by the checker: q[code] * absmax per block, the small tensors' own values."""
    q1, q2 = ref.maps()
    m, v = np.zeros(st.n_opt, np.float32), np.zeros(st.n_opt, np.float32)
    s1, s2, a1, a2 = (t.cpu().numpy() for t in (st.state1, st.state2, st.absmax1, st.absmax2))
    m32, v32 = st.m32.cpu().numpy(), st.v32.cpu().numpy()
    for k, (is8, so, r0, nr) in st.spans.items():
        off, n = st.layout[k][0], st.layout[k][1].numel()
        if is8:
            m[off:off + n] = ref.dequantise(s1[so:so + n], a1[r0:r0 + nr], q1)
            v[off:off + n] = ref.dequantise(s2[so:so + n], a2[r0:r0 + nr], q2)
        else:
            m[off:off + n], v[off:off + n] = m32[so:so + n], v32[so:so + n]
    return m, v


def _step_and_check(ops, st, g, step, betas, inv_scale, exact, flag=None):
    """One skg_adamw8_step on st against (a) skg_adamw_step on the dequantised old state: p, p16 and the small tensors' m, v bit for bit;
    (b) the checker's quantisation of its own m', v': codes and absmax, bit for bit (exact) or counted.  -> (differing codes, worst
    absmax distance in ulp)."""
    n = st.n_opt
    m0, v0 = _old_moments(st)
    rp, rp16 = st.p[:n].clone(), st.p16[:n].clone()
    rm, rv = torch.from_numpy(m0).to(DEV), torch.from_numpy(v0).to(DEV)
    args = (HYPER["lr"], betas[0], betas[1], HYPER["eps"], HYPER["weight_decay"], step, inv_scale)
    ops.adamw_step(rp, g[:n], rm, rv, rp16, *args)
    ops.adamw8_step(st.p[:n], g[:n], st.p16[:n], st.state1, st.state2, st.absmax1, st.absmax2, st.m32, st.v32, st.rows, st.qtab,
                    *args, flag)
    inside = torch.from_numpy(_inside(st)[:n]).to(DEV)
    assert torch.equal(st.p[:n][inside], rp[inside]) and torch.equal(st.p16[:n][inside], rp16[inside]), step
    q1, q2 = ref.maps()
    gm, gv = ref.moments(g[:n].cpu().numpy(), m0, v0, betas[0], betas[1], inv_scale)
    s1, s2, a1, a2 = (t.cpu().numpy() for t in (st.state1, st.state2, st.absmax1, st.absmax2))
    diff, ulps = 0, 0
    for k, (is8, so, r0, nr) in st.spans.items():
        off, cnt = st.layout[k][0], st.layout[k][1].numel()
        if not is8:                                               # adamw_kernel's arithmetic: skg_adamw_step's bits
            assert torch.equal(st.m32[so:so + cnt], rm[off:off + cnt]) and torch.equal(st.v32[so:so + cnt], rv[off:off + cnt]), (k, step)
            continue
        for got_c, got_a, x, q, zero in ((s1, a1, gm, q1, ref.ZERO1), (s2, a2, gv, q2, ref.ZERO2)):
            c, a = ref.quantise(x[off:off + cnt], q, zero)
            diff += int((got_c[so:so + cnt] != c).sum())
            ulps = max(ulps, int(np.abs(got_a[r0:r0 + nr].view(np.int32).astype(np.int64) - a.view(np.int32)).max()))
    if exact:
        assert diff == 0 and ulps == 0, (step, diff, ulps)
    return diff, ulps


def test_exact_probe_codes_absmax_and_masters_bit_for_bit(ops):
    """beta1 = beta2 = 0.5, inv_scale = 2^-3, gradients = integers in [-1024, 1024] x 2^-k (k = 0 ... 8 per element): every product in
    m' = 0.5 m + 0.5 gi and v' = 0.5 v + (0.5 gi) gi is exact, so a fused and a separate multiply-add round alike and the checker
    states the kernel's m', v' exactly.  Three steps from zero state: codes and absmax equal the checker's bit for bit, p / p16
    equal skg_adamw_step on the dequantised old state; padding, frozen key and the gaps of the state arrays keep their sentinels."""
    st = _opt(betas=(0.5, 0.5))
    _sentinels(st)
    before = _snap(st)
    gen = torch.Generator().manual_seed(1)
    for step in (1, 2, 3):
        ints = torch.randint(-1024, 1025, (st.n,), generator=gen).float()
        g = (ints * torch.exp2(-torch.randint(0, 9, (st.n,), generator=gen).float())).to(DEV)
        _step_and_check(ops, st, g, step, (0.5, 0.5), 2.0 ** -3, exact=True)
    outside = torch.from_numpy(~_inside(st)).to(DEV)
    assert torch.equal(st.p[outside], before["p"][outside]) and torch.equal(st.p16[outside], before["p16"][outside])
    c, s = (torch.from_numpy(~m).to(DEV) for m in _state_masks(st))
    assert bool((st.state1[c] == C_PAD).all()) and bool((st.state2[c] == C_PAD).all())
    assert bool((st.m32[s] == M_PAD).all()) and bool((st.v32[s] == M_PAD).all())
    is8 = st.rows[:, 3] == 1
    assert float(st.absmax1[is8].min()) > 0 and float(st.absmax2[is8].min()) > 0                  # (every block moved)
    assert not st.absmax1[~is8].any() and int(is8.sum()) == 14


@pytest.fixture(scope="module")
def random_run(ops):
    """20 steps at beta = (0.9, 0.999), gradients normal x a per-element scale 10^U(-4, 0) (x the grad scale 8), each step checked from
    the GPU's own previous state."""
    st = _opt()
    _sentinels(st)
    before = _snap(st)
    gen = torch.Generator().manual_seed(2)
    scale = torch.pow(10.0, -4.0 * torch.rand(st.n, generator=gen))
    per_step = []
    for step in range(1, 21):
        g = (torch.randn(st.n, generator=gen) * scale * 8.0).to(DEV)
        g[torch.from_numpy(~_inside(st)).to(DEV)] = float("nan")                  # what no row may read into anything it writes
        per_step.append(_step_and_check(ops, st, g, step, (0.9, 0.999), 1.0 / 8.0, exact=False))
    return st, before, per_step


def test_random_steps_resynced(random_run):
    """p, p16 bit-equal to skg_adamw_step on the dequantised state in every step (asserted inside the run).  Codes: at most 4 of the
    2 n differ from the checker's per step, absmax within 2 ulp - the checker's fma rounds through float64, the kernel's does not.
    Measured on one MI355X: 0 differing codes and 0 ulp in all 20 steps."""
    st, _, per_step = random_run
    print("[adamw8bit] differing codes / absmax ulp per step:", per_step)
    assert len(per_step) == 20
    for step, (diff, ulps) in enumerate(per_step, 1):
        assert diff <= 4 and ulps <= 2, (step, diff, ulps)


def test_small_tensors_padding_and_frozen_rows(random_run):
    """The small tensors' p, p16, m, v were bit-equal to skg_adamw_step in all 20 steps (asserted inside the run) and did move;
    padding elements of p / p16 (their gradient was NaN), the frozen key and the gaps of the state arrays are untouched."""
    st, before, _ = random_run
    for k in ("w4095", "b8", "b1"):
        is8, so, _, _ = st.spans[k]
        n = st.layout[k][1].numel()
        assert not is8 and bool((st.m32[so:so + n] != 0).all()) and bool((st.v32[so:so + n] > 0).all()), k
    outside = torch.from_numpy(~_inside(st)).to(DEV)
    assert torch.equal(st.p[outside], before["p"][outside]) and torch.equal(st.p16[outside], before["p16"][outside])
    assert bool(torch.isfinite(st.p).all())
    c, s = (torch.from_numpy(~m).to(DEV) for m in _state_masks(st))
    assert bool((st.state1[c] == C_PAD).all()) and bool((st.state2[c] == C_PAD).all())
    assert bool((st.m32[s] == M_PAD).all()) and bool((st.v32[s] == M_PAD).all())
    inside = ~outside
    assert not torch.equal(st.p[inside], before["p"][inside])


def test_guard_set_touches_nothing_and_clear_is_the_unguarded_step(ops, random_run):
    """From the state after the random steps (non-trivial codes everywhere): flag 1.0 -> every buffer byte-identical; flag 0 -> every
    buffer identical to the call without a flag."""
    src = random_run[0]
    a, b = _opt(), _opt()
    for st in (a, b):
        for n in BUFS:
            getattr(st, n).copy_(getattr(src, n))
    g = (torch.randn(a.n, generator=torch.Generator().manual_seed(4)) * 8e-2).to(DEV)
    args = (HYPER["lr"], 0.9, 0.999, HYPER["eps"], HYPER["weight_decay"], 21, 1.0 / 8.0)
    call = lambda st, flag: ops.adamw8_step(st.p[:st.n_opt], g[:st.n_opt], st.p16[:st.n_opt], st.state1, st.state2, st.absmax1,
                                            st.absmax2, st.m32, st.v32, st.rows, st.qtab, *args, flag)
    before = _snap(a)
    flag = torch.ones(1, device=DEV)
    call(a, flag)
    assert _same(_snap(a), before) == [] and float(flag) == 1.0
    flag.zero_()
    call(a, flag)
    call(b, None)
    assert _same(_snap(a), _snap(b)) == [] and set(_same(_snap(a), before)) == set(BUFS)


# ---------------------------------------------------------------------------------------------- under the LGP trainer
@pytest.fixture(scope="module")
def lgp_case(e2e):
    """The tiny LGP case of tests/test_gpu_loss_scaler.py: TINY UNet taps, B = 2, 32 x 32."""
    from oracle import ddim as oddim, lgp as olgp, unet as ounet
    h, chans = 32, ounet.tap_channels(ounet.TINY)
    sd = olgp.init_state_dict(sum(chans) + 40, seed=17)
    gen = torch.Generator().manual_seed(9)
    lat, sketch, noise = (torch.randn(B, 4, h, h, generator=gen), 0.2 * torch.randn(B, 4, h, h, generator=gen),
                          torch.randn(B, 4, h, h, generator=gen))
    ehs = torch.randn(B, 77, ounet.TINY.cross_attention_dim, generator=gen).half().float()
    acp = oddim.make_tables(50).alphas_cumprod
    return sd, chans, (e2e["net"], lat, sketch, ehs, [801, 133], noise, acp)


def _lgp(sd, chans, bits):
    from sketch2img_amd.lgp_train import HipLGPTrainer
    return HipLGPTrainer(sd, chans, DEV, warmup_steps=0, state_bits=bits)


def test_first_step_of_the_8bit_trainer_is_the_fp32_trainers(lgp_case):
    """From zero state the dequantised m, v are zero in both, and the update uses the unquantised m', v': one train_step leaves p and
    p16 bit-equal; the 8-bit trainer holds codes for the large weights and fp32 moments for every bias and BatchNorm vector."""
    from sketch2img_amd.lgp_train import train_step
    sd, chans, args = lgp_case
    t32, t8 = _lgp(sd, chans, 32), _lgp(sd, chans, 8)
    p0 = t8.p.clone()
    l32, l8 = train_step(t32, *args), train_step(t8, *args)
    assert float(l32) == float(l8) and t8.step_count == t32.step_count == 1
    assert torch.equal(t32.p, t8.p) and torch.equal(t32.p16, t8.p16) and not torch.equal(t8.p, p0)
    assert not hasattr(t8, "m") and float(t8.absmax1.max()) > 0
    for k, (is8, _, _, _) in t8.spans.items():
        assert is8 == (t8.layout[k][1].numel() >= 4096), k
    assert all(not t8.spans[k][0] for k in t8.spans if k.endswith("bias")) and any(s[0] for s in t8.spans.values())


def test_skipped_step_under_a_scaler_leaves_the_8bit_state_alone(lgp_case):
    """One good step, then a step whose gradient carries an inf (planted where the all-reduce hands it over): codes, absmax, the small
    moments, p, p16 and step_count stay as they were and the scale halves; the next good step runs."""
    from sketch2img_amd import loss_scaler
    from sketch2img_amd.lgp import LOSS_SCALE
    from sketch2img_amd.lgp_train import train_step
    sd, chans, args = lgp_case
    tr = _lgp(sd, chans, 8)
    sc = loss_scaler.DynamicLossScaler(DEV, init_scale=LOSS_SCALE, growth_interval=1000)
    poison = [False]

    def all_reduce(g, bucket_bytes=15 << 20):
        if poison[0]:
            g[5] = float("inf")
        return g
    tr.all_reduce = all_reduce
    _, v = train_step(tr, *args, scaler=sc)
    assert bool(v) is True and tr.step_count == 1
    before = _snap(tr)
    poison[0] = True
    _, v = train_step(tr, *args, scaler=sc)
    assert not v.resolved and bool(v) is False and tr.step_count == 1 and sc.scale == LOSS_SCALE / 2
    assert _same(_snap(tr), before) == []
    poison[0] = False
    _, v = train_step(tr, *args, scaler=sc)
    assert bool(v) is True and tr.step_count == 2 and sc.scale == LOSS_SCALE / 2
    assert set(_same(_snap(tr), before)) >= {"p", "p16", "state1", "state2", "absmax1", "absmax2", "m32", "v32"}


@pytest.mark.parametrize("bits", [32, 8])
def test_checkpoint_round_trip_continues_bit_for_bit(lgp_case, bits):
    """Three steps, optimizer_state_dict() + state_dict() -> a fresh trainer -> load_optimizer_state_dict(): the fourth step of both
    leaves every buffer bit-equal."""
    from sketch2img_amd.lgp_train import train_step
    sd, chans, args = lgp_case
    a = _lgp(sd, chans, bits)
    for _ in range(3):
        train_step(a, *args)
    b = _lgp(a.state_dict(), chans, bits)
    b.load_optimizer_state_dict(a.optimizer_state_dict())
    names = BUFS if bits == 8 else ("p", "p16", "m", "v")
    assert b.step_count == 3 and all(torch.equal(getattr(a, n), getattr(b, n)) for n in names)
    la, lb = train_step(a, *args), train_step(b, *args)
    assert float(la) == float(lb) and a.step_count == b.step_count == 4
    assert [n for n in names if not torch.equal(getattr(a, n), getattr(b, n))] == []
    fresh = _lgp(sd, chans, bits)
    assert not torch.equal(a.p, fresh.p)


def test_state_memory():
    """state_bytes() <= 2 n_opt + 8 rows + 8 (small elements) + the maps (2 x 256 floats); the block table is layout (32 bytes per row)
    and is not state."""
    st, st32 = _opt(8), _opt(32)
    small = sum(st.layout[k][1].numel() for k, s in st.spans.items() if not s[0])
    bound = 2 * st.n_opt + 8 * st.rows.shape[0] + 8 * small + 2 * 256 * 4
    print(f"[adamw8bit] state bytes {st.state_bytes()} (bound {bound}), fp32 state {st32.state_bytes()}, table {st.rows.numel() * 8}")
    assert st.state_bytes() <= bound and st32.state_bytes() == 8 * st32.n


CONV = [("a", (5000,)), ("b", (64, 65)), ("c", (900,)), ("d", (7,))]                 # 10 067 elements, two of them 8-bit


def test_convergence_matches_the_checker():
    """Minimise 1/2 |p - target|^2 with the gradient formed on the device, 200 steps at lr 1e-2: the final loss of the GPU's 8-bit run
    against the numpy checker's 8-bit run of the same problem.  The two part only where a code is decided on a rounding tie (the
    checker's fma goes through float64; its bias corrections come from another powf).  One such code moves one element's m by one cell,
    at most 0.9/64 = 1.4 % of the block's largest m, for one step; the problem is separable and each element is pulled back to its
    own target, so a perturbation decays with beta1 and does not spread.  Bound: 5 % of the checker's loss either way (a few cells'
    worth on EVERY element); measured on one MI355X: GPU 1.099665e3, checker 1.099665e3, margin -8.0e-8 of the loss, the fp32 run
    1.068518e3 (profiles/adamw8bit.txt).  The checker's loss must also have fallen below a quarter of where it started (Adam moves an element about lr per
    step, 2.0 in all, against residuals of standard deviation 1.4: the checker ends at 0.11 of the start)."""
    betas = (0.9, 0.999)
    kw = dict(betas=betas, grad_scale=1.0, shapes=CONV, frozen=(), seed=6, lr=1e-2)
    st8, st32 = _opt(8, **kw), _opt(32, **kw)
    gen = torch.Generator().manual_seed(7)
    target = torch.zeros(st8.n)
    for k, (off, shp) in st8.layout.items():
        target[off:off + shp.numel()] = torch.randn(shp.numel(), generator=gen)
    chk = ref.Adam8([st8.w32(k).cpu().numpy() for k, _ in CONV], 1e-2, betas, HYPER["eps"], HYPER["weight_decay"])
    tnp = [target[st8.layout[k][0]:st8.layout[k][0] + st8.layout[k][1].numel()].numpy() for k, _ in CONV]
    loss_np = lambda: 0.5 * sum(float(((p.astype(np.float64) - t) ** 2).sum()) for p, t in zip(chk.p, tnp))
    tdev = target.to(DEV)
    loss_dev = lambda st: 0.5 * float(((st.p.double() - tdev.double()) ** 2).sum())
    start = loss_dev(st8)
    assert abs(start - loss_np()) <= 1e-9 * start
    for _ in range(200):
        for st in (st8, st32):
            assert st.step(st.p - tdev, checked=True) is True
        chk.step([(p - t).astype(np.float32) for p, t in zip(chk.p, tnp)])
    l8, l32, lref = loss_dev(st8), loss_dev(st32), loss_np()
    print(f"[adamw8bit] convergence: start {start:.6e}, GPU 8-bit {l8:.6e}, checker 8-bit {lref:.6e} "
          f"(margin {(l8 - lref) / lref:+.3e}), GPU fp32 {l32:.6e}")
    assert lref < 0.25 * start and abs(l8 - lref) <= 0.05 * lref
