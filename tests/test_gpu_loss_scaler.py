"""The dynamic loss scale on the GPU (-m gpu): skg_nonfinite_flag, skg_adamw_step_guarded, loss_scaler.DynamicLossScaler under the
three trainers' train_step(scaler=).

Kernel tests are exact (a flag that is 0 or 1, bit equality with skg_adamw_step).  The trainer tests reuse the batch recipe, the
oracle and the bounds of tests/test_gpu_sat_train.py: per gradient tensor twice the relative-L2 distance of the oracle's own
fp16-storage emulation (same inputs, the loss scale in force) from the fp32 oracle, computed here and never taken from the HIP result;
an optimizer step against torch.optim.AdamW fed the HIP gradients within 1e-6 + 1e-5 max|p|.  Overflow cases carry inf / NaN as
values in valid buffers."""
import pytest
import torch

from tests.test_gpu_sat_train import B, DEV, SCALE, TS, _batch, _oracle, _rel, e2e, tiny_sat  # noqa: F401 (fixtures + harness)

pytestmark = pytest.mark.gpu

GRID_ROUND = 4 * 256 * 4096            # floats one grid-stride round of the largest grid covers (4096 blocks x 256 lanes x 16 bytes)
SIZES = [1, 3, 255, 256, 257, 1029, GRID_ROUND + 7]
POISON = {"+inf": 0x7F800000, "-inf": 0xFF800000 - (1 << 32), "quiet NaN": 0x7FC00000, "0x7f800001": 0x7F800001}
# finite and extreme: +-FLT_MAX, the smallest and the largest denormal of either sign, -0.0, 0.0, 1.0
CLEAN = [0x7F7FFFFF, 0xFF7FFFFF - (1 << 32), 0x00000001, 0x807FFFFF - (1 << 32), 0x80000001 - (1 << 32), 0x007FFFFF,
         0x80000000 - (1 << 32), 0x00000000, 0x3F800000]


@pytest.fixture(scope="module")
def ops():
    from sketch2img_amd import ops as o
    return o


def _clean_buffer(n):
    """n + 8 floats cycling through CLEAN, 16-byte aligned."""
    pat = torch.tensor(CLEAN, dtype=torch.int32, device=DEV)
    buf = pat.repeat((n + 8 + len(CLEAN) - 1) // len(CLEAN))[:n + 8].contiguous()
    assert buf.data_ptr() % 16 == 0
    return buf


@pytest.mark.parametrize("n", SIZES)
def test_nonfinite_flag_finds_every_poison_at_every_position_and_alignment(ops, n):
    """x = n floats starting 0, 1, 2, 3 floats into a 16-byte aligned buffer of finite extremes (+-FLT_MAX, denormals, -0.0): the
    flag stays as it was (0, and a sentinel 0.25: 'left alone'); one poisoned element - +-inf, a quiet NaN, the signalling pattern
    0x7f800001 - at the first, the last, the middle element, inside the scalar head, at the first and last element of the 16-byte
    body and inside the scalar tail sets it to exactly 1.0.  The largest n is one grid-stride round of the largest grid plus 7."""
    buf = _clean_buffer(n)
    flag = torch.zeros(1, device=DEV)
    launches = 0
    for off in range(4):
        xi = buf[off:off + n]
        x = xi.view(torch.float32)
        assert x.data_ptr() % 16 == 4 * off and bool(torch.isfinite(x).all())
        flag.fill_(0.25)
        ops.nonfinite_flag(x, flag)
        assert float(flag) == 0.25, (n, off)
        ops.nonfinite_flag(x, flag, reset=True)
        assert float(flag) == 0.0, (n, off)
        head = min((4 - off) & 3, n)
        body_end = head + (n - head) // 4 * 4
        spots = {0, n - 1, n // 2, max(head - 1, 0), min(head, n - 1), max(body_end - 1, 0), min(body_end, n - 1),
                 min(GRID_ROUND + head, n - 1)}
        for pos in sorted(spots):
            keep = int(xi[pos])
            for name, bits in POISON.items():
                xi[pos] = bits
                flag.zero_()
                ops.nonfinite_flag(x, flag)
                launches += 1
                assert float(flag) == 1.0, (n, off, pos, name)
            xi[pos] = keep
        ops.nonfinite_flag(x, flag, reset=True)
        assert float(flag) == 0.0, (n, off)
    assert launches >= 16


def test_nonfinite_flag_accumulates_until_reset(ops):
    """Several vectors OR into one flag: a clean vector after a dirty one leaves the 1.0; reset clears it on the stream; a hit in a
    later vector is kept through clean ones."""
    clean = torch.ones(1029, device=DEV)
    dirty = clean.clone()
    dirty[517] = float("-inf")
    flag = torch.zeros(1, device=DEV)
    ops.nonfinite_flag(dirty, flag, reset=True)
    ops.nonfinite_flag(clean, flag)
    assert float(flag) == 1.0
    ops.nonfinite_flag(clean, flag, reset=True)
    assert float(flag) == 0.0
    ops.nonfinite_flag(clean, flag)
    ops.nonfinite_flag(dirty, flag)
    ops.nonfinite_flag(clean, flag)
    assert float(flag) == 1.0
    ops.nonfinite_flag(dirty, flag, reset=True)                   # reset, then found again in the same call
    assert float(flag) == 1.0


@pytest.mark.parametrize("with_f16", [True, False])
@pytest.mark.parametrize("n", [1, 257, 100003])
def test_guarded_step_is_the_plain_step_or_nothing(ops, n, with_f16):
    """Flag 0: p, m, v and the fp16 copy bit-equal to skg_adamw_step on clones of the same inputs (two steps, so m and v are
    non-zero in the second).  Flag 1.0: all four unchanged, bit for bit."""
    g = torch.Generator().manual_seed(n)
    p = torch.randn(n, generator=g).to(DEV)
    p_init = p.clone()
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    p16 = p.half() if with_f16 else None
    ref = [p.clone(), m.clone(), v.clone(), p16.clone() if with_f16 else None]
    flag = torch.zeros(1, device=DEV)
    hyper = (1e-3, 0.9, 0.999, 1e-8, 0.05)
    for step in (1, 2):
        grad = (torch.randn(n, generator=g) * 4096 * 1e-2).to(DEV)
        ops.adamw_step(ref[0], grad, ref[1], ref[2], ref[3], *hyper, step, 1.0 / 4096)
        ops.adamw_step_guarded(p, grad, m, v, p16, *hyper, step, 1.0 / 4096, flag)
        for a, b in zip((p, m, v, p16), ref):
            assert (a is None and b is None) or torch.equal(a, b), (n, step)
    assert float(ref[1].abs().max()) > 0 and not torch.equal(p, p_init)
    before = [t.clone() for t in (p, m, v)] + [p16.clone() if with_f16 else None]
    flag.fill_(1.0)
    ops.adamw_step_guarded(p, grad, m, v, p16, *hyper, 3, 1.0 / 4096, flag)
    for a, b in zip((p, m, v, p16), before):
        assert (a is None and b is None) or torch.equal(a, b), n
    assert float(flag) == 1.0


# ---------------------------------------------------------------------------------------------- trainers
def _sat(sd, **kw):
    from sketch2img_amd import sat_train
    from sketch2img_amd.config import TINY
    return sat_train.HipSatTrainer(TINY, sd, DEV, lr=2e-4, warmup_steps=0, total_steps=1 << 20, scale=SCALE, **kw)


def _state(*opts):
    return [t.clone() for o in opts for t in (o.p, o.m, o.v, o.p16)]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _capture(trainer, into):
    """Keep the flat gradient of every step: train_step hands it to the trainer's all_reduce (a no-op on one rank)."""
    def all_reduce(g, bucket_bytes=15 << 20):
        into.append(g)
        return g
    trainer.all_reduce = all_reduce


@pytest.mark.parametrize("batched", [False, True])
def test_sat_steps_under_a_scaler_at_loss_scale_equal_the_static_steps(tiny_sat, e2e, batched):
    """TINY UNet, B = 2, 16 x 16 (the batch of test_gpu_sat_train.py), a scaler started at LOSS_SCALE whose growth interval lies
    beyond the test: two train_steps leave masters, m, v and the fp16 copy bit-equal to two static steps, with the same losses and
    d sketch_state.  Nothing waited in between: the verdict is pending after train_step and the step count moves when it resolves."""
    from sketch2img_amd import loss_scaler, sat_train
    bt, net, sd = _batch(16), e2e["net"], tiny_sat["sd"]
    static, dyn = _sat(sd), _sat(sd)
    sc = loss_scaler.DynamicLossScaler(DEV, init_scale=sat_train.LOSS_SCALE, growth_interval=1000)
    args = (net, bt["lat"], bt["ehs"], bt["state"], TS, bt["noise"], bt["acp"])
    for i in range(2):
        l0, stepped, d0 = sat_train.train_step(static, *args, batched=batched)
        l1, v, d1 = sat_train.train_step(dyn, *args, batched=batched, scaler=sc)
        assert stepped is True and not v.resolved and sc.pending and dyn.step_count == i
        assert float(l0) == float(l1) and torch.equal(d0, d1)
    assert bool(v) is True and v.resolved and dyn.step_count == static.step_count == 2
    assert _same(_state(static), _state(dyn))
    assert sc.scale == sat_train.LOSS_SCALE and sc.growth_tracker == 2 and float(sc.flag) == 0.0


@pytest.mark.parametrize("batched", [False, True])
def test_lgp_steps_under_a_scaler_at_loss_scale_equal_the_static_steps(e2e, batched):
    """The LGP trainer at its own LOSS_SCALE (TINY UNet taps, B = 2, 32 x 32): two train_step(scaler=) equal two static ones bit for
    bit - masters, m, v, fp16 copy, BatchNorm running statistics and losses."""
    from oracle import ddim as oddim, lgp as olgp, unet as ounet
    from sketch2img_amd import loss_scaler
    from sketch2img_amd.lgp import LOSS_SCALE
    from sketch2img_amd.lgp_train import HipLGPTrainer, train_step
    h, chans = 32, ounet.tap_channels(ounet.TINY)
    sd = olgp.init_state_dict(sum(chans) + 40, seed=17)
    gen = torch.Generator().manual_seed(9)
    lat, sketch, noise = torch.randn(B, 4, h, h, generator=gen), 0.2 * torch.randn(B, 4, h, h, generator=gen), torch.randn(B, 4, h, h, generator=gen)
    ehs = torch.randn(B, 77, ounet.TINY.cross_attention_dim, generator=gen).half().float()
    acp = oddim.make_tables(50).alphas_cumprod
    static, dyn = HipLGPTrainer(sd, chans, DEV, warmup_steps=0), HipLGPTrainer(sd, chans, DEV, warmup_steps=0)
    sc = loss_scaler.DynamicLossScaler(DEV, init_scale=LOSS_SCALE, growth_interval=1000)
    args = (e2e["net"], lat, sketch, ehs, [801, 133], noise, acp)
    for i in range(2):
        l0 = train_step(static, *args, batched=batched)
        l1, v = train_step(dyn, *args, batched=batched, scaler=sc)
        assert not v.resolved and dyn.step_count == i and float(l0) == float(l1)
    assert bool(v) is True and dyn.step_count == static.step_count == 2 and sc.scale == LOSS_SCALE and sc.growth_tracker == 2
    assert _same(_state(static), _state(dyn))
    a, b = static.state_dict(), dyn.state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


def test_backoff_skips_until_the_backward_is_finite_then_steps_on_good_gradients(tiny_sat, e2e):
    """init_scale = 2^30: the fp16 seed overflows, so the first steps carry inf / NaN gradients.  Repeating train_step on the fixed
    batch, the skipped steps form one unbroken run at the start, leave p, m, v, the fp16 copy and the step count bit-unchanged and
    halve the scale each time.  The first step that runs does so at 2^16 or above (2^10 ... 2^16 is this model's finite window,
    sat_train.py), i.e. after at most 14 skips, and its gradients / the scale in force lie, tensor by tensor, within the bound of
    test_training_gradients_end_to_end: twice the fp16-storage emulation's distance from the fp32 oracle at that same scale.
    Measured on one MI355X: 6 skips, first step at 2^24, worst tensor 5.2e-3 against a largest bound of 1.0e-2."""
    from sketch2img_amd import loss_scaler, sat_train
    bt, net, sd, W = _batch(16), e2e["net"], tiny_sat["sd"], e2e["W"]
    tr = _sat(sd)
    grads = []
    _capture(tr, grads)
    sc = loss_scaler.DynamicLossScaler(DEV, init_scale=2.0 ** 30, growth_interval=1000)
    before = _state(tr)
    scale, skips = 2.0 ** 30, 0
    while True:
        assert sc.scale == scale and skips <= 14, (skips, sc.scale)
        loss, v, dst = sat_train.train_step(tr, net, bt["lat"], bt["ehs"], bt["state"], TS, bt["noise"], bt["acp"], scaler=sc)
        assert not v.resolved and bool(torch.isfinite(loss))
        if bool(v):
            break
        assert not bool(torch.isfinite(grads[-1]).all())
        assert tr.step_count == 0 and _same(before, _state(tr)) and sc.growth_tracker == 0
        skips += 1
        scale *= 0.5
    print(f"[backoff] {skips} skipped steps, first step at scale 2^{int(torch.log2(torch.tensor(scale)))}")
    assert skips >= 1 and scale >= 2.0 ** 16 and sc.scale == scale and sc.growth_tracker == 1
    assert tr.step_count == 1 and not _same(before, _state(tr))
    g = grads[-1]
    assert bool(torch.isfinite(g).all()) and len(grads) == skips + 1
    ref, emu = _oracle(W, sd, bt, False, 1.0), _oracle(W, sd, bt, True, scale)
    fails, worst, worst_b = [], 0.0, 0.0
    for k in tr.layout:
        e, b = _rel(tr.grad_view(g, k).cpu() / scale, ref[1][k]), 2 * _rel(emu[1][k], ref[1][k])
        worst, worst_b = max(worst, e), max(worst_b, b)
        if not e <= b:
            fails.append((k, e, b))
    e, b = _rel(dst.cpu() / scale, ref[2]), 2 * _rel(emu[2], ref[2])
    print(f"[backoff] worst tensor: hip {worst:.3e}, largest bound {worst_b:.3e}; d state hip {e:.3e} bound {b:.3e}")
    assert not fails, fails
    assert e <= b
    # every later step on the fixed batch runs: the skipped steps were one run at the start
    for i in range(2):
        _, v, _ = sat_train.train_step(tr, net, bt["lat"], bt["ehs"], bt["state"], TS, bt["noise"], bt["acp"], scaler=sc)
        assert bool(v) is True and tr.step_count == 2 + i and sc.scale == scale


def test_growth_doubles_the_scale_and_the_next_step_divides_it_out(tiny_sat, e2e):
    """growth_interval = 2, init_scale = 2^10: after two clean steps the scale is 2^11 and the tracker 0.  The third step's update
    equals torch.optim.AdamW's - started from the trainer's p, m, v after two steps, at the trainer's LR - fed that step's HIP
    gradients divided by 2^11 (1e-6 + 1e-5 max|p|, the bound of test_optimizer_step_and_loss_decrease)."""
    from sketch2img_amd import loss_scaler, sat_train
    bt, net, sd = _batch(16), e2e["net"], tiny_sat["sd"]
    tr = _sat(sd)
    grads = []
    _capture(tr, grads)
    sc = loss_scaler.DynamicLossScaler(DEV, init_scale=2.0 ** 10, growth_interval=2)
    step = lambda: sat_train.train_step(tr, net, bt["lat"], bt["ehs"], bt["state"], TS, bt["noise"], bt["acp"], scaler=sc)
    step()
    assert sc.scale == 2.0 ** 10 and sc.growth_tracker == 1
    step()
    assert sc.scale == 2.0 ** 11 and sc.growth_tracker == 0 and tr.step_count == 2
    keys = list(tr.layout)
    p0 = {k: tr.w32(k).cpu().clone().requires_grad_(True) for k in keys}
    opt = torch.optim.AdamW([p0[k] for k in keys], lr=tr.current_lr(), betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    for k in keys:
        opt.state[p0[k]] = dict(step=torch.tensor(2.0), exp_avg=tr.grad_view(tr.m, k).cpu().clone(),
                                exp_avg_sq=tr.grad_view(tr.v, k).cpu().clone())
    _, v, _ = step()
    assert bool(v) is True and tr.step_count == 3 and sc.scale == 2.0 ** 11 and sc.growth_tracker == 1 and len(grads) == 3
    for k in keys:
        p0[k].grad = tr.grad_view(grads[2], k).cpu().clone() / 2.0 ** 11
    opt.step()
    new = tr.state_dict()
    moved = 0.0
    for k in keys:
        assert (new[k].cpu() - p0[k].detach()).abs().max() < 1e-6 + 1e-5 * float(p0[k].detach().abs().max()), k
        assert torch.equal(tr.w16(k).float().cpu(), new[k].cpu().half().float())
        moved = max(moved, float((new[k].cpu() - sd[k]).abs().max()))
    assert moved > 1e-4                                           # (three steps at lr 2e-4 did move the masters)


def test_one_verdict_for_satmixin_and_tower():
    """SatMixin + TINY tower under one scaler at LOSS_SCALE.  The tower built with seam_scale = 2^24: only ITS backward overflows
    (the SatMixin gradient is finite), neither optimizer steps, both step counts stay, the scale halves.  With the default seam
    scale on the same batch both step, and their state equals the static train_step's bit for bit."""
    from oracle import attn_inject as oinj, unet as ounet
    from sketch2img_amd import config, loss_scaler, sat_train
    from sketch2img_amd.clip_vision_train import HipClipTowerTrainer
    from sketch2img_amd.unet import HipUNet
    from tests import test_gpu_clip_train as tc
    from oracle import clip_vision as oclip
    W = ounet.init_weights(ounet.TINY)
    net, sd = HipUNet(config.TINY, W, DEV), oinj.init_state_dict(ounet.TINY, "clip")
    cfg, Wc, bt = config.CLIPVisionConfig(**tc.E2E_CLIP), oclip.init_weights(oclip.CLIPVisionConfig(**tc.E2E_CLIP)), tc._batch(16)
    kw = dict(lr=2e-4, warmup_steps=0, total_steps=1 << 20)
    step = lambda tr, tw, **k: sat_train.train_step(tr, net, bt["lat"], bt["ehs"], None, tc.TS, bt["noise"], bt["acp"], tower=tw,
                                                    pixel_values=bt["px"], **k)
    # only the tower overflows
    tr, tw = _sat(sd), HipClipTowerTrainer(cfg, Wc, DEV, seam_scale=2.0 ** 24, **kw)
    gs, gts = [], []
    _capture(tr, gs)
    _capture(tw, gts)
    sc = loss_scaler.DynamicLossScaler(DEV, init_scale=sat_train.LOSS_SCALE, growth_interval=1000)
    before = _state(tr, tw)
    loss, v, _ = step(tr, tw, scaler=sc)
    assert bool(torch.isfinite(gs[0]).all()) and not bool(torch.isfinite(gts[0]).all())
    assert bool(v) is False and tr.step_count == 0 and tw.step_count == 0 and bool(torch.isfinite(loss))
    assert _same(before, _state(tr, tw)) and sc.scale == sat_train.LOSS_SCALE / 2 and sc.growth_tracker == 0
    # the default seam scale: both step, as the static path does
    tr, tw = _sat(sd), HipClipTowerTrainer(cfg, Wc, DEV, **kw)
    tr0, tw0 = _sat(sd), HipClipTowerTrainer(cfg, Wc, DEV, **kw)
    sc = loss_scaler.DynamicLossScaler(DEV, init_scale=sat_train.LOSS_SCALE, growth_interval=1000)
    l0, stepped, _ = step(tr0, tw0)
    l1, v, _ = step(tr, tw, scaler=sc)
    assert stepped is True and tr.step_count == tw.step_count == 0 and not v.resolved
    assert bool(v) is True and tr.step_count == tw.step_count == 1 and float(l0) == float(l1)
    assert _same(_state(tr0, tw0), _state(tr, tw)) and not _same(before[:4], _state(tr))
    assert sc.scale == sat_train.LOSS_SCALE and sc.growth_tracker == 1
