"""SatMixin (CLIP-token injected attention) training step on the GPU (-m gpu).

Kernel tests compare against fp64 arithmetic on the SAME fp16 inputs with derived bounds (u = 2^-24, the fp32 unit roundoff):
products of two fp16 numbers are exact in fp32, so a sum of M of them in ANY order is off by at most (M - 1) u sum|terms| to first
order; the fold of the split slabs, the multiplication by alpha and the final store / accumulate add a handful of roundings of
the total.  Hence |err| <= c M u alpha (|dY|^T |X|) + u |ref| with c = 2 (M + 3 <= 2 M roundings for M >= 3, and the smallest M
here, 5, leaves a factor > 1 for the matrix pipe's internal order).

Block and end-to-end tests compare against autograd of the fp32 CPU oracle; their bounds are twice the distance of the oracle's
own fp16-storage emulation (same inputs, same loss scale) from the fp32 oracle, computed in the test - never from the HIP result."""

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -24


@pytest.fixture(scope="module")
def ops():
    from sketch2img_amd import ops as o
    return o


def _view(t, pad):
    """t as a column view of a wider device buffer (pitch = width + pad)."""
    buf = torch.full((t.shape[0], t.shape[1] + pad), 3.0, dtype=torch.float16, device=DEV)
    buf[:, 8:8 + t.shape[1]] = t.to(DEV)
    return buf[:, 8:8 + t.shape[1]]


@pytest.mark.parametrize("M,N,K,pad", [(7, 32, 32, 0), (321, 32, 32, 0), (1281, 64, 128, 24), (257, 32, 1024, 0)])
def test_wgrad_matches_fp64_and_is_repeatable(ops, M, N, K, pad):
    """skg_wgrad_f16: '=' with db and alpha = 0.375, then '+=' without db and alpha = 1 on top, then '+=' with db; (1281, 64, 128)
    reads column views (ldy = N + 24, ldx = K + 24).  Bound: module docstring (c = 2).  Two runs give the same bits."""
    g = torch.Generator().manual_seed(M * 7 + N + K)
    dY = (torch.randn(M, N, generator=g) * 0.05).half()
    X = torch.randn(M, K, generator=g).half()
    dYd, Xd = (_view(dY, pad), _view(X, pad)) if pad else (dY.to(DEV), X.to(DEV))
    ref = dY.double().t() @ X.double()
    mag = dY.double().abs().t() @ X.double().abs()
    refb, magb = dY.double().sum(0), dY.double().abs().sum(0)
    runs = []
    for _ in range(2):
        dW, db = ops.wgrad(dYd, Xd, alpha=0.375, want_db=True)
        a = (dW.cpu().clone(), db.cpu().clone())
        ops.wgrad(dYd, Xd, dW=dW, alpha=1.0, accumulate=True)
        b = (dW.cpu().clone(), db.cpu().clone())
        ops.wgrad(dYd, Xd, dW=dW, db=db, alpha=-0.5, accumulate=True)
        c = (dW.cpu().clone(), db.cpu().clone())
        runs.append((a, b, c))
    for x, y in zip(runs[0], runs[1]):
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])
    (a, b, c) = runs[0]
    bound = lambda al, r: 2 * M * U * al * mag + U * r.abs()
    boundb = lambda al, r: 2 * M * U * al * magb + U * r.abs()
    e = (a[0].double() - 0.375 * ref).abs()
    print(f"wgrad {M}x{N}x{K}: max err / bound = {float((e / bound(0.375, 0.375 * ref)).max()):.3f}")
    assert (e <= bound(0.375, 0.375 * ref)).all()
    assert ((a[1].double() - 0.375 * refb).abs() <= boundb(0.375, 0.375 * refb)).all()
    # the accumulating forms: the bounds of the parts add up
    assert ((b[0].double() - 1.375 * ref).abs() <= bound(1.375, 1.375 * ref) + U * (1.375 * ref).abs()).all()
    assert torch.equal(b[1], a[1])                                                          # db = NULL: untouched
    assert ((c[0].double() - 0.875 * ref).abs() <= bound(1.875, 1.375 * ref) + 2 * U * (1.375 * ref).abs()).all()
    assert ((c[1].double() - (-0.125) * refb).abs() <= boundb(0.875, 0.375 * refb) + U * (0.375 * refb).abs()).all()


@pytest.mark.parametrize("C", [32, 128])
@pytest.mark.parametrize("M", [5, 321])
def test_layernorm_param_grads(ops, C, M):
    """skg_layernorm_param_grads, '=' then '+=' (scale 0.5), against fp64 with the kernel's own stored (mean, rstd).  xhat takes two
    fp32 roundings, the product one, the M-term sums M - 1 + the fold's: |err| <= (2 M + 4) u sum|dY xhat| + u |ref| (2 u for '+=')."""
    g = torch.Generator().manual_seed(C + M)
    X = (torch.randn(M, C, generator=g) * 1.5 + 0.3).half().to(DEV)
    dY = (torch.randn(M, C, generator=g) * 0.1).half().to(DEV)
    gamma, beta = torch.ones(C, dtype=torch.float16, device=DEV), torch.zeros(C, dtype=torch.float16, device=DEV)
    _, st = ops.layernorm(X, gamma, beta, want_stats=True)
    s = st.cpu().double()
    xh = (X.cpu().double() - s[:, :1]) * s[:, 1:]
    d = dY.cpu().double()
    rg, mg = (d * xh).sum(0), (d * xh).abs().sum(0)
    rb, mb = d.sum(0), d.abs().sum(0)
    dg, db = ops.layernorm_param_grads(X, dY, st)
    dg2, db2 = ops.layernorm_param_grads(X, dY, st)
    assert torch.equal(dg, dg2) and torch.equal(db, db2)
    k = (2 * M + 4) * U
    assert ((dg.cpu().double() - rg).abs() <= k * mg + U * rg.abs()).all()
    assert ((db.cpu().double() - rb).abs() <= k * mb + U * rb.abs()).all()
    ops.layernorm_param_grads(X, dY, st, dg, db, scale=0.5, accumulate=True)
    assert ((dg.cpu().double() - 1.5 * rg).abs() <= 1.5 * k * mg + 3 * U * rg.abs()).all()
    assert ((db.cpu().double() - 1.5 * rb).abs() <= 1.5 * k * mb + 3 * U * rb.abs()).all()


@pytest.mark.parametrize("dh", [16, 32])
def test_attn_bwd_dkv_with_key_stride(ops, dh):
    """skg_attn_bwd_dkv_strided on the padded [N + T -> multiple of 8] K / V buffer: bit-equal to skg_attn_bwd_dkv on compacted
    copies; the padding rows of dK / dV keep their sentinel."""
    B, heads, Nq, Nkv, L = 2, 2, 64, 321, 328
    C = heads * dh
    g = torch.Generator().manual_seed(dh)
    q = torch.randn(B * Nq, C, generator=g).half().to(DEV)
    kv = torch.randn(B * L, 2 * C, generator=g).half().to(DEV)
    dO = (torch.randn(B * Nq, C, generator=g) * 0.1).half().to(DEV)
    K, V = kv[:, :C], kv[:, C:]
    scale = dh ** -0.5
    o, lse = ops.attn_fwd(q, K, V, B, heads, Nq, Nkv, L, dh, scale, want_lse=True, v_rows=True)
    delta = ops.attn_bwd_delta(o, dO, B, heads, Nq, dh)
    dkv = torch.full((B * L, 2 * C), 7.0, dtype=torch.float16, device=DEV)
    ops.attn_bwd_dkv_strided(q, K, V, dO, lse, delta, B, heads, Nq, Nkv, L, dh, scale, dkv[:, :C], dkv[:, C:])
    rows = torch.cat([torch.arange(b * L, b * L + Nkv) for b in range(B)]).to(DEV)
    Kc, Vc = K[rows].contiguous(), V[rows].contiguous()
    dKc, dVc = ops.attn_bwd_dkv(q, Kc, Vc, dO, lse, delta, B, heads, Nq, Nkv, dh, scale)
    assert torch.equal(dkv[rows][:, :C], dKc) and torch.equal(dkv[rows][:, C:], dVc)
    assert float(dKc.float().abs().max()) > 0
    pad = torch.cat([torch.arange(b * L + Nkv, (b + 1) * L) for b in range(B)]).to(DEV)
    assert bool((dkv[pad] == 7.0).all())


def test_loss_and_seed_against_torch():
    """loss = mean((eps - noise)^2) over the batch, d eps = LOSS_SCALE 2 (eps - noise) / numel in fp16 (4 valid channels, the rest
    zero).  B = 2, h = 8.  Loss: fp32 sum of 512 terms -> 512 u relative; seed: one fp16 rounding (2^-11) of an fp32 value."""
    from sketch2img_amd import sat_train
    B, h = 2, 8
    g = torch.Generator().manual_seed(3)
    eps = torch.zeros(B * h * h, 8, dtype=torch.float16)
    eps[:, :4] = torch.randn(B * h * h, 4, generator=g).half()
    noise = torch.randn(B, 4, h, h, generator=g)
    loss, seed = sat_train.mse_seed(eps.to(DEV), noise.to(DEV), B, h)
    e = eps[:, :4].double().reshape(B, h * h, 4).permute(0, 2, 1).reshape(B, 4, h, h)
    ref = ((e - noise.double()) ** 2).mean()
    assert abs(float(loss) - float(ref)) <= 512 * U * float(ref)
    gref = sat_train.LOSS_SCALE * 2 * (e - noise.double()) / noise.numel()
    got = seed.cpu().double().reshape(B, h * h, -1)
    assert float(got[:, :, 4:].abs().max()) == 0.0
    got4 = got[:, :, :4].permute(0, 2, 1).reshape(B, 4, h, h)
    assert ((got4 - gref).abs() <= 2.0 ** -11 * gref.abs() * (1 + 2.0 ** -10) + 2.0 ** -25).all()


# ---------------------------------------------------------------------------------------------- injected block alone
SCALE = 0.8


def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-300))


@pytest.fixture(scope="module")
def tiny_sat():
    from oracle import attn_inject as oinj, unet as ounet
    from sketch2img_amd import sat_train
    from sketch2img_amd.config import TINY
    sd = oinj.init_state_dict(ounet.TINY, "clip")
    tr = sat_train.HipSatTrainer(TINY, sd, DEV, lr=2e-4, warmup_steps=0, scale=SCALE)
    return dict(sd=sd, tr=tr, cfg=ounet.TINY)


@pytest.mark.parametrize("T", [257, 9])
@pytest.mark.parametrize("N", [16, 256])
@pytest.mark.parametrize("path,C,heads", [("down_blocks.0.attentions.0.transformer_blocks.0", 32, 2),
                                          ("mid_block.attentions.0.transformer_blocks.0", 128, 4)])
def test_injected_block_backward_vs_autograd(tiny_sat, path, C, heads, N, T):
    """HipClipInjectorTrain forward + backward of ONE block against autograd of oracle.attn_inject.make_clip_inject on the same
    fp16-representable inputs: the output, d h, every parameter gradient of the block and d state, per tensor (relative L2).
    Bound per tensor: 2 x the distance of the oracle's fp16-storage emulation from the fp32 oracle (accumulation order, fp16 P / dS
    operands) + 2^-11: one fp16 rounding, for tensors the emulation - fed fp16-exact inputs - happens to leave unrounded
    (d sketch_conv.bias = scale * colsum(d out) is exact there)."""
    from oracle import attn_inject as oinj, unet as ounet
    sd, tr = tiny_sat["sd"], tiny_sat["tr"]
    n = oinj.module_name(path)
    keys = [k for k in sd if k.startswith(n + ".")]
    g = torch.Generator().manual_seed(N * 1000 + T + C)
    h = torch.randn(1, N, C, generator=g).half().float()
    state = (0.5 * torch.randn(1, T, 1024, generator=g)).half().float()
    dout = (0.05 * torch.randn(1, N, C, generator=g)).half().float()

    def run(emulate):
        p = {k: sd[k].clone().requires_grad_(True) for k in keys}
        hh, ss = h.clone().requires_grad_(True), state.clone().requires_grad_(True)
        with ounet.fp16_storage(emulate):
            out = oinj.make_clip_inject(p, ss, SCALE)(path, hh, heads)
            (out * dout).sum().backward()
        return dict({k: p[k].grad for k in keys}, out=out.detach(), dh=hh.grad, dstate=ss.grad)

    ref, emu = run(False), run(True)
    inj = tr.injector
    inj.refresh()
    gflat = torch.zeros(tr.n, device=DEV)
    dstate = torch.zeros(T, 1024, device=DEV)
    inj.begin(state[0].half().to(DEV), gflat, dstate)
    out = inj(path, h[0].half().to(DEV), 1, N, heads)
    dh = inj.backward(path, dout[0].half().to(DEV))
    inj.end()
    got = dict({k: tr.grad_view(gflat, k).cpu().reshape(sd[k].shape) for k in keys}, out=out.float().cpu()[None],
               dh=dh.float().cpu()[None], dstate=dstate.cpu()[None])
    assert len(keys) == 11
    for k in ref:
        e, b = _rel(got[k], ref[k]), 2 * _rel(emu[k], ref[k]) + 2.0 ** -11
        print(f"[block C={C} N={N} T={T}] {k.replace(n + '.', ''):32s} hip {e:.2e}  bound {b:.2e}")
        assert e <= b, (k, e, b)


# ---------------------------------------------------------------------------------------------- end to end
B, TS = 2, (37, 803)


def _batch(h):
    from oracle import ddim as oddim, unet as ounet
    g = torch.Generator().manual_seed(100 + h)
    cfg = ounet.TINY
    return dict(lat=torch.randn(B, 4, h, h, generator=g), noise=torch.randn(B, 4, h, h, generator=g),
                ehs=torch.randn(B, 77, cfg.cross_attention_dim, generator=g).half().float(),
                state=(0.5 * torch.randn(B, 257, 1024, generator=g)).half().float(),       # 257 tokens of N(0, 0.25)
                acp=oddim.make_tables(50).alphas_cumprod)


def _oracle(W, sd, bt, emulate, loss_scale):
    """(loss, {key: grad}, d state) of the oracle UNet with the CLIP injector, by autograd; the emulation multiplies the loss by the
    loss scale so that its gradients round to fp16 at the magnitudes the HIP path stores."""
    from oracle import attn_inject as oinj, unet as ounet
    from sketch2img_amd.sat_train import add_noise
    p = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    st = bt["state"].clone().requires_grad_(True)
    noisy = add_noise(bt["lat"], bt["noise"], TS, bt["acp"])
    with ounet.fp16_storage(emulate):
        eps = torch.cat([ounet.unet_forward(ounet.TINY, W, noisy[b:b + 1], TS[b], bt["ehs"][b:b + 1],
                                            inject=oinj.make_clip_inject(p, st[b:b + 1], SCALE))[0] for b in range(B)])
        loss = torch.nn.functional.mse_loss(eps, bt["noise"])
        (loss * loss_scale).backward()
    return float(loss.detach()), {k: p[k].grad / loss_scale for k in p}, st.grad / loss_scale


@pytest.fixture(scope="module")
def e2e():
    from oracle import unet as ounet
    from sketch2img_amd.config import TINY
    from sketch2img_amd.unet import HipUNet
    W = ounet.init_weights(ounet.TINY)
    return dict(W=W, net=HipUNet(TINY, W, DEV), cache={})


@pytest.mark.parametrize("h", [32, 16])
def test_training_gradients_end_to_end(tiny_sat, e2e, h):
    """TINY UNet, B = 2, timesteps (37, 803), 257 sketch tokens: loss, EVERY one of the 176 parameter gradients per tensor and
    d sketch_state against autograd of the fp32 oracle.  Bound per tensor: twice the relative L2 distance of the fp16-storage
    emulation (loss x LOSS_SCALE = 2^13) from the fp32 oracle on the same inputs - computed here, printed next to the HIP
    figure.  Measured on one MI355X with LOSS_SCALE = 2^13: emulation max 4.5e-3 (32 x 32) / 5.0e-3 (16 x 16) per tensor, so the
    largest bound is 8.9e-3 / 9.9e-3 (bounds differ per tensor, and by a few % with the CPU's BLAS summation order); HIP worst tensor 5.7e-3 / 5.0e-3; d state HIP 1.4e-3 / 1.6e-3 against
    bounds 2.8e-3 / 3.4e-3; loss HIP 1.131303 / oracle 1.131295 (32 x 32).  Loss: 2e-3 relative.  Also: two runs are bit-equal, and grads(B = 2) = the sum of the two single-sample runs
    (same seed: half the loss scale over half the elements) to fp32 rounding."""
    from sketch2img_amd import sat_train
    sd, tr, net, W = tiny_sat["sd"], tiny_sat["tr"], e2e["net"], e2e["W"]
    bt = _batch(h)
    ref = _oracle(W, sd, bt, False, 1.0)
    emu = _oracle(W, sd, bt, True, sat_train.LOSS_SCALE)
    args = (bt["lat"], bt["noise"], TS, bt["ehs"], bt["state"], bt["acp"])
    loss, g, dst = tr.loss_and_grads(net, *args)
    loss2, g2, dst2 = tr.loss_and_grads(net, *args)
    assert torch.equal(g, g2) and torch.equal(dst, dst2) and float(loss) == float(loss2)
    assert bool(torch.isfinite(g).all()) and net.inject is None
    print(f"[sat e2e h={h}] loss hip {float(loss):.6f} oracle {ref[0]:.6f} emulation {emu[0]:.6f}")
    assert abs(float(loss) - ref[0]) <= 2e-3 * ref[0]
    worst, worst_b, fails = 0.0, 0.0, []
    assert len(tr.layout) == 176
    for k in tr.layout:
        got = tr.grad_view(g, k).cpu() / sat_train.LOSS_SCALE
        e, b = _rel(got, ref[1][k]), 2 * _rel(emu[1][k], ref[1][k])
        worst, worst_b = max(worst, e), max(worst_b, b)
        if e > b:
            fails.append((k, e, b))
            print(f"[sat e2e h={h}] OVER {k}: hip {e:.3e} bound {b:.3e}")
    e, b = _rel(dst.cpu() / sat_train.LOSS_SCALE, ref[2]), 2 * _rel(emu[2], ref[2])
    print(f"[sat e2e h={h}] worst tensor: hip {worst:.3e}, largest bound {worst_b:.3e}; d state hip {e:.3e} bound {b:.3e}")
    assert not fails, fails
    assert e <= b
    # the batch is the sum of its samples
    parts = [tr.loss_and_grads(net, bt["lat"][i:i + 1], bt["noise"][i:i + 1], TS[i:i + 1], bt["ehs"][i:i + 1], bt["state"][i:i + 1],
                               bt["acp"], loss_scale=sat_train.LOSS_SCALE / B) for i in range(B)]
    gs = parts[0][1] + parts[1][1]
    assert ((g - gs).abs() <= 2.0 ** -23 * (parts[0][1].abs() + parts[1][1].abs())).all()
    assert torch.equal(dst, torch.cat([parts[0][2], parts[1][2]]))


def test_backward_eps_without_injector_vs_autograd(e2e):
    """HipUNet.backward_eps on a rows = 1 evaluation without an injector: d (eps . seed) / d x through conv_out, conv_norm_out, up
    block 3 and the rest of the chain, against autograd of the fp32 oracle (relative L2 <= 2 x the fp16-storage emulation's)."""
    from oracle import unet as ounet
    from sketch2img_amd import ops
    from sketch2img_amd.unet import CIN_PAD, EPS_SEED_LD, Stash
    net, W, h, t = e2e["net"], e2e["W"], 16, 37
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 4, h, h, generator=g).half().float()
    ehs = torch.randn(1, 77, ounet.TINY.cross_attention_dim, generator=g).half().float()
    dE = torch.randn(1, 4, h, h, generator=g).half().float()

    def run(emulate):
        xg = x.clone().requires_grad_(True)
        with ounet.fp16_storage(emulate):
            (ounet.unet_forward(ounet.TINY, W, xg, t, ehs)[0] * dE).sum().backward()
        return xg.grad

    ref, emu = run(False), run(True)
    net.prepare_context(ehs)
    stash = Stash()
    net.forward(ops.nchw_to_nhwc(x.to(DEV), CIN_PAD), t, 1, h, stash, want_taps=False, want_eps=True)
    seed = torch.zeros(h * h, EPS_SEED_LD, dtype=torch.float16, device=DEV)
    seed[:, :4] = dE[0].reshape(4, h * h).t().half().to(DEV)
    dx = ops.nhwc_to_nchw(net.backward_eps(stash, seed), 1, 4, h, h).cpu()
    e, b = _rel(dx, ref), 2 * _rel(emu, ref)
    print(f"[backward_eps] d x: hip {e:.3e} bound {b:.3e}")
    assert e <= b


def test_backward_with_injector_still_raises(tiny_sat, e2e):
    from sketch2img_amd.unet import Stash
    net = e2e["net"]
    net.inject = tiny_sat["tr"].injector
    try:
        with pytest.raises(AssertionError, match="injected attention is not supported"):
            net.backward(Stash(), [None] * 9)
    finally:
        net.inject = None


# ---------------------------------------------------------------------------------------------- optimizer
def test_optimizer_step_and_loss_decrease(tiny_sat, e2e):
    """One step against torch.optim.AdamW fed the HIP gradients (bound of the LGP trainer's test: 1e-6 + 1e-5 max|p|), fp16 copy
    refreshed; a gradient with one inf is refused and changes nothing; then 8 steps (lr 2e-4, no warm-up) on the fixed batch at
    h = 16 against the fp32 oracle + torch AdamW re-run here: HIP losses monotone, the first within 2e-3 relative of the oracle's,
    falling by at least half the oracle's drop."""
    from oracle import unet as ounet
    from sketch2img_amd import sat_train
    from sketch2img_amd.config import TINY
    sd, net, W = tiny_sat["sd"], e2e["net"], e2e["W"]
    bt = _batch(16)
    args = (bt["lat"], bt["noise"], TS, bt["ehs"], bt["state"], bt["acp"])
    tr = sat_train.HipSatTrainer(TINY, sd, DEV, lr=2e-4, warmup_steps=0, total_steps=1 << 20, scale=SCALE)
    loss, g, _ = tr.loss_and_grads(net, *args)
    keys = list(tr.layout)
    # a non-finite gradient: refused, nothing changes
    bad = g.clone()
    bad[tr.layout[keys[5]][0] + 3] = float("inf")
    before = (tr.p.clone(), tr.m.clone(), tr.v.clone(), tr.p16.clone())
    assert tr.step(bad) is False and tr.step_count == 0
    assert all(torch.equal(a, b) for a, b in zip(before, (tr.p, tr.m, tr.v, tr.p16)))
    # one step vs torch AdamW on the same numbers
    p0 = {k: sd[k].clone().float().requires_grad_(True) for k in keys}
    opt = torch.optim.AdamW([p0[k] for k in keys], lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    for k in keys:
        p0[k].grad = tr.grad_view(g, k).cpu().clone() / sat_train.LOSS_SCALE
    opt.step()
    assert tr.step(g) is True and tr.step_count == 1
    new = tr.state_dict()
    for k in keys:
        assert (new[k].cpu() - p0[k].detach()).abs().max() < 1e-6 + 1e-5 * float(p0[k].detach().abs().max()), k
        assert torch.equal(tr.w16(k).float().cpu(), new[k].cpu().half().float())           # fp16 working copy refreshed
    # 8 steps on the fixed batch: HIP ...
    losses = [float(loss)]
    for _ in range(7):
        l, gg, _ = tr.loss_and_grads(net, *args)
        assert tr.step(gg)
        losses.append(float(l))
    losses.append(float(tr.loss_and_grads(net, *args)[0]))
    # ... and the fp32 oracle with torch AdamW
    po = {k: sd[k].clone().float().requires_grad_(True) for k in keys}
    opt = torch.optim.AdamW([po[k] for k in keys], lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    ref = []
    for i in range(9):
        l, gr, _ = _oracle(W, {k: po[k].detach() for k in keys}, bt, False, 1.0)
        ref.append(l)
        if i < 8:
            for k in keys:
                po[k].grad = gr[k]
            opt.step()
    print("[sat train] hip    losses:", " ".join(f"{v:.5f}" for v in losses))
    print("[sat train] oracle losses:", " ".join(f"{v:.5f}" for v in ref))
    assert all(b < a for a, b in zip(ref, ref[1:]))
    assert all(b < a for a, b in zip(losses, losses[1:]))
    assert abs(losses[0] - ref[0]) <= 2e-3 * ref[0]
    assert losses[0] - losses[-1] >= 0.5 * (ref[0] - ref[-1])
