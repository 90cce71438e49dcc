"""A timestep per sample in ONE UNet walk (HipUNet.forward(x, [t...], rows, h)), the assembled path: the time projection folded
into conv1.bias of every ResnetBlock becomes a [rows, Cout] stack and conv1's epilogue reads a bias row per sample.

The checker is the CPU oracle with a per-row timestep vector (oracle.unet.unet_forward).  The yardstick of every figure is the
SAME figure of the per-sample walks - the existing int-t path, concatenated - measured in the test on the same inputs; the batched
figure may be at most 1.5 x it (the project's margin, tests/test_gpu_pipeline.py _WIDE320_BOUNDS "measured x 1.5": the batch runs other
kernel instantiations, i.e. another summation order - the effect test_shared_cfg_prefix_is_bit_identical documents).

Nets: TINY at 32 x 32 latents and the (320, 64, 128, 128) net of test_wide320_net_fused_stashing_launches_vs_oracle; rows = 3 with
timesteps (801, 133, 37), and 4 rows as two CFG halves with (801, 133, 801, 133).  backward() differentiates the second half of
the rows, so its yardstick walks are the 2-row [uncond; cond] walks of the existing int path, one per cond sample.

Measured on one MI355X (relative Frobenius against the oracle; batched / per-sample walks):
  TINY rows = 3: eps 1.176e-3 / 1.176e-3, taps 6.63e-4 ... 1.565e-3 (worst: tap 7) / the same figures - the batch is bit-identical to
  the concatenated walks on this net; d/dx through the batched stash 2.150e-3 / 2.150e-3;
  wide net, default mode: rows = 3 eps 8.012e-4 / 8.012e-4, 4 rows 8.058e-4 / 8.054e-4, d/dx 1.598e-3 / 1.598e-3;
  wide net, accuracy mode: rows = 3 eps 2.011e-4 / 2.011e-4, 4 rows 2.036e-4 / 2.031e-4, worst tap 1.024e-3 / 1.008e-3 (tap 6),
  d/dx 1.236e-3 / 1.236e-3; shared front against the unshared walk: bit-identical in both modes (rel 0);
  LGP train_step(batched=True): loss 1.87317 against the oracle's 1.87340; unet_taps batched / per-sample loop 6.99e-4 ... 1.686e-3,
  the same figures tap by tap."""
import dataclasses

import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_pipeline import from_nhwc, nhwc16, tiny  # noqa: F401 (fixture)
from tests.util import rel_err, report

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TS3 = (801, 133, 37)
TS4 = (801, 133, 801, 133)
MARGIN = 1.5


def _x32(x):
    from sketch2img_amd import ops
    from sketch2img_amd.unet import CIN_PAD
    return ops.nchw_to_nhwc(x.to(DEV), CIN_PAD)


def _nchw(eps, taps, rows, h):
    from sketch2img_amd import ops
    return ops.nhwc_to_nchw(eps, rows, 4, h, h).cpu(), [from_nhwc(t, rows, s, s) for t, s in taps]


def _batched(net, x, ts, ehs, h, **kw):
    net.prepare_context(ehs)
    return _nchw(*net.forward(_x32(x), list(ts), len(ts), h, **kw), len(ts), h)


def _per_sample(net, x, ts, ehs, h):
    """The existing path: one rows = 1 walk per sample with an int t, concatenated."""
    es, tps = [], []
    for b, t in enumerate(ts):
        net.prepare_context(ehs[b:b + 1])
        e, tp = _nchw(*net.forward(_x32(x[b:b + 1]), int(t), 1, h), 1, h)
        es.append(e); tps.append(tp)
    return torch.cat(es), [torch.cat([tp[i] for tp in tps]) for i in range(9)]


def _compare(tag, batched, walks, ref):
    """[parity] figures of both against the oracle; the batched one within MARGIN x the walks' one, eps and tap by tap."""
    names = ["eps"] + [f"tap{i}" for i in range(9)]
    got_b, got_w, refs = [batched[0]] + batched[1], [walks[0]] + walks[1], [ref[0]] + list(ref[1])
    for n, b, w, r in zip(names, got_b, got_w, refs):
        fb, fw = report(f"{tag} {n}: batched", b, r)[0], report(f"{tag} {n}: per-sample walks", w, r)[0]
        assert fb <= MARGIN * fw, (tag, n, fb, fw)


def _backward_pairs(net, x, ts, ehs, h, tg, S):
    """d/dx of the cond rows from the existing path: one 2-row [uncond; cond] stashing walk per cond sample, int t."""
    from sketch2img_amd import ops
    from sketch2img_amd.unet import Stash
    out = []
    for s in range(S):
        idx = [s, S + s]
        net.prepare_context(ehs[idx])
        stash = Stash()
        net.forward(_x32(x[idx]), int(ts[S + s]), 2, h, stash)
        dx = net.backward(stash, [nhwc16(t[s:s + 1]) for t in tg])
        out.append(ops.nhwc_to_nchw(dx, 1, 4, h, h).cpu())
    return torch.cat(out)


def _oracle(cfg, W, x, ts, ehs, tg=None, S=0):
    from oracle import unet as ounet
    if tg is None:
        with torch.no_grad():
            e, t = ounet.unet_forward(cfg, W, x, torch.tensor(ts), ehs)
        return e, t, None
    xr = x.clone().requires_grad_(True)
    e, t = ounet.unet_forward(cfg, W, xr, torch.tensor(ts), ehs)
    gr = torch.autograd.grad(sum((r[S:] * g).sum() for r, g in zip(t, tg)), xr)[0][S:]
    return e.detach(), [r.detach() for r in t], gr


# ------------------------------------------------------------------------------------------------------ TINY
@pytest.fixture(scope="module")
def tiny_case(tiny):
    """Inputs and oracle results on TINY, computed once: 3 rows at TS3 (forward), 4 rows at TS4 + (37, 501) (backward of rows 2, 3)."""
    h = tiny["h"]
    g = torch.Generator().manual_seed(71)
    x = torch.randn(4, 4, h, h, generator=g).half().float()
    ehs = tiny["ehs"]
    ts_b = (801, 133, 37, 501)
    e3, t3, _ = _oracle(tiny["cfg"], tiny["W"], x[:3], TS3, ehs[:3])
    tg = [torch.randn(2, r.shape[1], r.shape[2], r.shape[3], generator=g).half().float() for r in t3]
    e4, t4, gr = _oracle(tiny["cfg"], tiny["W"], x, ts_b, ehs, tg, 2)
    yield dict(x=x, ehs=ehs, h=h, ref3=(e3, t3), ts_b=ts_b, tg=tg, grad=gr)
    tiny["net"].prepare_context(tiny["ehs"])      # the shared fixture's context, for whoever uses it next


def test_tiny_batched_forward_vs_per_sample_walks(tiny, tiny_case):
    """rows = 3, timesteps (801, 133, 37): eps and the nine taps, batched <= 1.5 x the per-sample walks' figure."""
    c, net = tiny_case, tiny["net"]
    b = _batched(net, c["x"][:3], TS3, c["ehs"][:3], c["h"])
    w = _per_sample(net, c["x"][:3], TS3, c["ehs"][:3], c["h"])
    _compare("tiny rows=3", b, w, c["ref3"])
    # the per-sample rows really differ: the batch at one shared timestep is another result
    one = _batched(net, c["x"][:3], (801, 801, 801), c["ehs"][:3], c["h"])
    assert torch.equal(one[0][0], b[0][0]) and rel_err(one[0][1:], b[0][1:]) > 1e-2


def test_equal_timesteps_take_the_int_path_bit_for_bit(tiny, tiny_case):
    c, net, h = tiny_case, tiny["net"], tiny_case["h"]
    net.prepare_context(c["ehs"][:3])
    x32 = _x32(c["x"][:3])
    e0, t0 = net.forward(x32, 133, 3, h)
    for t in ([133, 133, 133], (133, 133, 133), torch.tensor([133, 133, 133]), torch.tensor(133)):
        e1, t1 = net.forward(x32, t, 3, h)
        assert torch.equal(e0, e1) and all(torch.equal(a[0], b[0]) for a, b in zip(t0, t1))
    # a tensor and a list of distinct timesteps are the same call
    ea, _ = net.forward(x32, list(TS3), 3, h)
    eb, _ = net.forward(x32, torch.tensor(TS3, device=DEV), 3, h)
    assert torch.equal(ea, eb)
    with pytest.raises(ValueError):
        net.forward(x32, [801, 133], 3, h)
    with pytest.raises(ValueError):
        net.forward(x32, list(TS3), 3, h, shared_input=True)


def test_tiny_shared_front_with_per_sample_timesteps(tiny, tiny_case):
    """4 rows = two CFG halves with (801, 133, 801, 133): the shared front gets the half stack - bit-identical to the unshared walk on
    TINY (test_shared_cfg_prefix_is_bit_identical's tolerance for this net); halves with other timesteps are refused."""
    c, net, h = tiny_case, tiny["net"], tiny_case["h"]
    xx = torch.cat([c["x"][:2], c["x"][:2]])
    net.prepare_context(c["ehs"])
    x32 = _x32(xx)
    e0, t0 = net.forward(x32, list(TS4), 4, h)
    e1, t1 = net.forward(x32, list(TS4), 4, h, shared_input=True)
    assert torch.equal(e0, e1) and all(torch.equal(a[0], b[0]) for a, b in zip(t0, t1))
    with pytest.raises(ValueError):
        net.forward(x32, [801, 133, 133, 801], 4, h, shared_input=True)
    # want_taps / want_eps / down_only keep working with a timestep per sample
    _, t2 = net.forward(x32, list(TS4), 4, h, want_eps=False)
    assert all(torch.equal(a[0], b[0]) for a, b in zip(t0, t2))
    blocks = net.forward(x32, list(TS4), 4, h, down_only=True)
    assert torch.equal(blocks[0][-1][0], t0[0][0])      # the first downsampler's output is tap 0


def test_tiny_backward_through_a_per_sample_stash(tiny, tiny_case):
    """Stashing batched forward at (801, 133, 37, 501) + backward(stash, tap gradients of rows 2, 3) against torch.autograd.grad on the
    oracle with the per-row timesteps: <= 1.5 x the d/dx figure of the existing 2-row walks - the stash of a per-sample walk is complete."""
    from sketch2img_amd import ops
    from sketch2img_amd.unet import Stash
    c, net, h = tiny_case, tiny["net"], tiny_case["h"]
    net.prepare_context(c["ehs"])
    stash = Stash()
    net.forward(_x32(c["x"]), list(c["ts_b"]), 4, h, stash)
    dx = ops.nhwc_to_nchw(net.backward(stash, [nhwc16(t) for t in c["tg"]]), 2, 4, h, h).cpu()
    dw = _backward_pairs(net, c["x"], c["ts_b"], c["ehs"], h, c["tg"], 2)
    fb, fw = report("tiny d/dx: batched stash", dx, c["grad"])[0], report("tiny d/dx: per-sample walks", dw, c["grad"])[0]
    assert fb <= MARGIN * fw


def test_public_call_with_a_timestep_tensor(tiny, tiny_case):
    """UNetFacade.__call__(sample, torch.tensor([801, 133]), ehs) - the reference's trainer call - returns forward's eps as .sample and
    fills the hooks; a scalar tensor is handled as before."""
    from sketch2img_amd.modules.latent_predictor import hook_unet
    from sketch2img_amd.modules.pipeline import UNetFacade
    from sketch2img_amd.config import TINY
    c, h = tiny_case, tiny_case["h"]
    un = UNetFacade(TINY, tiny["W"], DEV)
    blocks = hook_unet(un)
    x, ehs = c["x"][:2], c["ehs"][:2]
    out = un(x.to(DEV), torch.tensor([801, 133]), ehs).sample
    eps, taps = _batched(un.hip, x, (801, 133), ehs, h)
    assert out.dtype == torch.float32 and torch.equal(out.cpu(), eps)
    for blk, t in zip(blocks, taps):
        assert torch.equal(blk.output.cpu(), t)
    o1 = un(x.to(DEV), torch.tensor([133]), ehs).sample
    o2 = un(x.to(DEV), 133, ehs).sample
    o3 = un(x.to(DEV), torch.tensor([133, 133]), ehs).sample
    assert torch.equal(o1, o2) and torch.equal(o2, o3) and not torch.equal(o2, out)
    with pytest.raises(ValueError):
        un(x.to(DEV), torch.tensor([801, 133, 37]), ehs)


def test_lgp_train_step_batched(tiny):
    """train_step(..., batched=True) on the inputs of test_lgp_train_step_end_to_end_tiny: the loss within that test's 1 % of the oracle
    loss, one optimizer step; unet_taps(batched=True) against unet_taps(batched=False) tap by tap under the 1.5 x rule (both against
    the oracle's taps)."""
    from oracle import ddim as oddim, lgp as olgp, unet as ounet
    from sketch2img_amd.lgp_train import HipLGPTrainer, add_noise, train_step, unet_taps
    cfg, h, B = tiny["cfg"], 32, 2
    chans = ounet.tap_channels(cfg)
    sd = olgp.init_state_dict(sum(chans) + 40, seed=17)
    gen = torch.Generator().manual_seed(9)
    lat = torch.randn(B, 4, h, h, generator=gen)
    sketch = 0.2 * torch.randn(B, 4, h, h, generator=gen)
    noise = torch.randn(B, 4, h, h, generator=gen)
    ts = [801, 133]
    ehs = tiny["ehs"][:B]
    acp = oddim.make_tables(50).alphas_cumprod
    tr = HipLGPTrainer(sd, chans, DEV, warmup_steps=0)
    loss = train_step(tr, tiny["net"], lat, sketch, ehs, ts, noise, acp, batched=True)
    noisy, nl = add_noise(lat, noise, ts, acp)
    with torch.no_grad():
        _, feats = ounet.unet_forward(cfg, tiny["W"], noisy, torch.tensor(ts), ehs)
    x = torch.cat([F.interpolate(f, size=h, mode="bilinear") for f in feats], 1)
    o = olgp.lgp_forward(sd, x, nl, training=True)
    ref = F.mse_loss(o.reshape(B, h, h, 4).permute(0, 3, 2, 1), sketch)
    print(f"[parity] lgp train_step (batched) loss hip {float(loss):.5f} oracle {float(ref):.5f}")
    assert abs(float(loss) - float(ref)) < 1e-2 * float(ref)
    assert tr.step_count == 1 and int(tr.state_dict()["layers.5.num_batches_tracked"]) == 1
    tb = unet_taps(tiny["net"], noisy.to(DEV), ts, ehs, batched=True)
    tw = unet_taps(tiny["net"], noisy.to(DEV), ts, ehs, batched=False)
    tiny["net"].prepare_context(tiny["ehs"])                    # restore the fixture's context for later tests
    for i, ((a, s), (b, s2), r) in enumerate(zip(tb, tw, feats)):
        assert s == s2 == r.shape[2] and a.shape == b.shape
        fb = report(f"unet_taps tap{i}: batched", from_nhwc(a, B, s, s), r)[0]
        fw = report(f"unet_taps tap{i}: per-sample loop", from_nhwc(b, B, s, s), r)[0]
        assert fb <= MARGIN * fw


# ------------------------------------------------------------------------------------------------------ the wide (320, 64, 128, 128) net
_WIDE = {}


def _wide_case():
    """The net and inputs of test_wide320_net_fused_stashing_launches_vs_oracle with per-row timesteps; the oracle's results once for
    both modes: 4 rows at TS4 with d/dx of the cond rows, and row 2 alone at t = 37 (rows are independent: rows 0, 1 of the 4-row
    result and this one are the 3-row result at TS3)."""
    if not _WIDE:
        from oracle import unet as ounet
        from sketch2img_amd.config import TINY
        rep = dict(block_out_channels=(320, 64, 128, 128), num_heads=(8, 2, 4, 4))
        cfg, ocfg = dataclasses.replace(TINY, **rep), dataclasses.replace(ounet.TINY, **rep)
        W = ounet.init_weights(ocfg)
        S, h = 2, 32
        g = torch.Generator().manual_seed(47)
        x = torch.randn(S, 4, h, h, generator=g)
        xx = torch.cat([x, x]).half().float()
        ehs = torch.randn(2 * S, 77, cfg.cross_attention_dim, generator=g).half().float()
        e2, t2, _ = _oracle(ocfg, W, xx[2:3], TS3[2:], ehs[2:3])
        tg = [torch.randn(S, r.shape[1], r.shape[2], r.shape[3], generator=g).half().float() for r in t2]
        e4, t4, gr = _oracle(ocfg, W, xx, TS4, ehs, tg, S)
        ref3 = (torch.cat([e4[:2], e2]), [torch.cat([a[:2], b]) for a, b in zip(t4, t2)])
        _WIDE.update(cfg=cfg, W=W, S=S, h=h, xx=xx, ehs=ehs, tg=tg, ref3=ref3, ref4=(e4, t4), grad=gr)
    return _WIDE


@pytest.mark.parametrize("residual_fp32", [False, True])
def test_wide320_net_with_per_sample_timesteps(residual_fp32):
    """Default and accuracy mode (residual_fp32=True), each against its own per-sample figures: rows = 3 forward; 4 rows as two CFG
    halves, shared front against the unshared walk (rel < 2e-3, the tolerance where the instantiations differ) and against the oracle;
    stashing forward + backward against autograd on the oracle."""
    from sketch2img_amd import ops
    from sketch2img_amd.unet import HipUNet, Stash
    c = _wide_case()
    S, h = c["S"], c["h"]
    net = HipUNet(c["cfg"], c["W"], DEV, residual_fp32=residual_fp32)
    tag = f"wide320 residual_fp32={residual_fp32}"
    b = _batched(net, c["xx"][:3], TS3, c["ehs"][:3], h)
    w = _per_sample(net, c["xx"][:3], TS3, c["ehs"][:3], h)
    _compare(f"{tag} rows=3", b, w, c["ref3"])
    # 4 rows, two CFG halves
    w4 = _per_sample(net, c["xx"], TS4, c["ehs"], h)
    net.prepare_context(c["ehs"])
    x32 = _x32(c["xx"])
    got = {}
    for shared in (False, True):
        stash = Stash()
        e, tp = _nchw(*net.forward(x32, list(TS4), 4, h, stash, shared_input=shared), 4, h)
        dx = ops.nhwc_to_nchw(net.backward(stash, [nhwc16(t) for t in c["tg"]]), S, 4, h, h).cpu()
        got[shared] = (e, tp, dx)
        _compare(f"{tag} rows=4 shared={shared}", (e, tp), w4, c["ref4"])
    assert report(f"{tag}: eps, shared vs unshared", got[True][0], got[False][0])[0] < 2e-3
    for i, (a, bb) in enumerate(zip(got[True][1], got[False][1])):
        assert report(f"{tag}: tap{i}, shared vs unshared", a, bb)[0] < 2e-3
    dw = _backward_pairs(net, c["xx"], TS4, c["ehs"], h, c["tg"], S)
    fw = report(f"{tag} d/dx: per-sample walks", dw, c["grad"])[0]
    for shared in (False, True):
        fb = report(f"{tag} d/dx: batched stash, shared={shared}", got[shared][2], c["grad"])[0]
        assert fb <= MARGIN * fw
