"""The SatMixin training step on the whole batch in ONE UNet walk (batched=True) on the GPU (-m gpu): HipUNet.forward(diff_from=),
the training injector on B samples, HipSatTrainer / train_step with batched=True.

Bounds are built the way tests/test_gpu_sat_train.py builds them: the reference is autograd of the fp32 CPU oracle, the bound per
tensor is twice the relative-L2 distance of the oracle's own fp16-storage emulation (same inputs, loss x LOSS_SCALE) from that
oracle - computed inside the test, printed next to the HIP figure, never taken from the code under test.  The oracle results of
the end-to-end cases are computed once and shared (read-only) by the tests that need them."""

import pytest
import torch

from tests.test_gpu_sat_train import DEV, SCALE, _rel, e2e, tiny_sat  # noqa: F401 (fixtures + harness)

pytestmark = pytest.mark.gpu

CASES = {"B3_h16": dict(B=3, h=16, ts=(37, 803, 411)), "B2_h32": dict(B=2, h=32, ts=(37, 803)), "B1_h16": dict(B=1, h=16, ts=(803,))}


def _batch(B, h, seed=0):
    """B samples: different latents, noise, prompts (random ehs) and [257, 1024] sketch states."""
    from oracle import ddim as oddim, unet as ounet
    g = torch.Generator().manual_seed(1000 * B + h + seed)
    return dict(lat=torch.randn(B, 4, h, h, generator=g), noise=torch.randn(B, 4, h, h, generator=g),
                ehs=torch.randn(B, 77, ounet.TINY.cross_attention_dim, generator=g).half().float(),
                state=(0.5 * torch.randn(B, 257, 1024, generator=g)).half().float(),
                acp=oddim.make_tables(50).alphas_cumprod)


def _oracle(W, sd, bt, ts, emulate, loss_scale):
    """(loss, {key: grad}, d state) of the oracle UNet with the CLIP injector evaluated sample by sample, by autograd (as
    tests/test_gpu_sat_train.py::_oracle, for any batch)."""
    from oracle import attn_inject as oinj, unet as ounet
    from sketch2img_amd.sat_train import add_noise
    B = len(ts)
    p = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    st = bt["state"].clone().requires_grad_(True)
    noisy = add_noise(bt["lat"], bt["noise"], ts, bt["acp"])
    with ounet.fp16_storage(emulate):
        eps = torch.cat([ounet.unet_forward(ounet.TINY, W, noisy[b:b + 1], ts[b], bt["ehs"][b:b + 1],
                                            inject=oinj.make_clip_inject(p, st[b:b + 1], SCALE))[0] for b in range(B)])
        loss = torch.nn.functional.mse_loss(eps, bt["noise"])
        (loss * loss_scale).backward()
    return float(loss.detach()), {k: p[k].grad / loss_scale for k in p}, st.grad / loss_scale


_SHARED = {}


def _case(name, tiny_sat, e2e):
    """Inputs, the fp32 oracle, the emulation and the per-tensor bounds of an end-to-end case, and the HIP results of the batched
    mode (two runs) - computed once, shared, never modified."""
    if name not in _SHARED:
        from sketch2img_amd import sat_train
        c = CASES[name]
        bt = _batch(c["B"], c["h"])
        ref = _oracle(e2e["W"], tiny_sat["sd"], bt, c["ts"], False, 1.0)
        emu = _oracle(e2e["W"], tiny_sat["sd"], bt, c["ts"], True, sat_train.LOSS_SCALE)
        bound = {k: 2 * _rel(emu[1][k], ref[1][k]) for k in ref[1]}
        bound["d state"] = 2 * _rel(emu[2], ref[2])
        args = (bt["lat"], bt["noise"], c["ts"], bt["ehs"], bt["state"], bt["acp"])
        tr, net = tiny_sat["tr"], e2e["net"]
        runs = [tr.loss_and_grads(net, *args, batched=True) for _ in range(2)]
        _SHARED[name] = dict(c, bt=bt, ref=ref, emu=emu, bound=bound, args=args, runs=runs)
    return _SHARED[name]


# ---------------------------------------------------------------------------------------------- 1. end to end
@pytest.mark.parametrize("name", list(CASES))
def test_batched_gradients_end_to_end(tiny_sat, e2e, name):
    """TINY UNet, B = 3 (odd) at 16 x 16 with timesteps (37, 803, 411), B = 2 at 32 x 32 and B = 1 (the batched form of one sample:
    other launches than the per-sample path's), different prompts and sketch states per sample, ONE UNet walk: the loss (2e-3
    relative), EVERY one of the 176 parameter gradients and d sketch_state against autograd of the fp32 oracle evaluated sample by
    sample; bound per tensor = 2 x the emulation's distance (module docstring).  Two batched runs are bit-equal."""
    from sketch2img_amd import sat_train
    c = _case(name, tiny_sat, e2e)
    tr, net, ref, emu = tiny_sat["tr"], e2e["net"], c["ref"], c["emu"]
    (loss, g, dst), (loss2, g2, dst2) = c["runs"]
    assert torch.equal(g, g2) and torch.equal(dst, dst2) and float(loss) == float(loss2)
    assert bool(torch.isfinite(g).all()) and net.inject is None and dst.shape == (c["B"], 257, 1024)
    print(f"[sat batched {name}] loss hip {float(loss):.6f} oracle {ref[0]:.6f} emulation {emu[0]:.6f}")
    assert abs(float(loss) - ref[0]) <= 2e-3 * ref[0]
    assert len(tr.layout) == 176
    worst, worst_b, fails = 0.0, 0.0, []
    for k in tr.layout:
        e, b = _rel(tr.grad_view(g, k).cpu() / sat_train.LOSS_SCALE, ref[1][k]), c["bound"][k]
        worst, worst_b = max(worst, e), max(worst_b, b)
        if e > b:
            fails.append((k, e, b))
            print(f"[sat batched {name}] OVER {k}: hip {e:.3e} bound {b:.3e}")
    e, b = _rel(dst.cpu() / sat_train.LOSS_SCALE, ref[2]), c["bound"]["d state"]
    print(f"[sat batched {name}] worst tensor: hip {worst:.3e}, largest bound {worst_b:.3e}; d state hip {e:.3e} bound {b:.3e}")
    assert not fails, fails
    assert e <= b


# ---------------------------------------------------------------------------------------------- 2. against the per-sample path
@pytest.mark.parametrize("name", list(CASES))
def test_batched_against_per_sample(tiny_sat, e2e, name):
    """The same inputs through both HIP paths: per tensor the relative L2 between them is at most the sum of their two oracle bounds
    (each path may sit anywhere within its own bound of the oracle; they run different kernel instantiations, so no bit equality)."""
    c = _case(name, tiny_sat, e2e)
    tr, net = tiny_sat["tr"], e2e["net"]
    loss, g, dst = c["runs"][0]
    lp, gp, dp = tr.loss_and_grads(net, *c["args"])
    assert abs(float(loss) - float(lp)) <= 2 * 2e-3 * c["ref"][0]
    worst, fails = (0.0, 1.0, ""), []
    for k in list(tr.layout) + ["d state"]:
        a, b = (dst, dp) if k == "d state" else (tr.grad_view(g, k), tr.grad_view(gp, k))
        e, bd = _rel(a.cpu(), b.cpu()), 2 * c["bound"][k]
        if e / bd > worst[0] / worst[1]:
            worst = (e, bd, k)
        if e > bd:
            fails.append((k, e, bd))
    print(f"[sat batched {name}] batched vs per-sample: loss {float(loss):.6f} / {float(lp):.6f}; worst pair {worst[0]:.3e} bound {worst[1]:.3e} ({worst[2]})")
    assert not fails, fails


# ---------------------------------------------------------------------------------------------- 3. the injected block alone
@pytest.mark.parametrize("T", [257, 9])
@pytest.mark.parametrize("N", [16, 256])
@pytest.mark.parametrize("path,C,heads", [("down_blocks.0.attentions.0.transformer_blocks.0", 32, 2),
                                          ("mid_block.attentions.0.transformer_blocks.0", 128, 4)])
def test_batched_injected_block_vs_autograd(tiny_sat, path, C, heads, N, T):
    """HipClipInjectorTrain on B = 3 samples, forward + backward of ONE block, against autograd of oracle.attn_inject.make_clip_inject
    on the same fp16-representable inputs: the output, d h, the block's 11 parameter gradients and d state per tensor.  N + T = 25,
    265, 273, 513: none a multiple of 8, so every K / V buffer has pad rows.  Bound: 2 x emulation + 2^-11 (one fp16 rounding, for
    tensors the emulation leaves unrounded), as test_injected_block_backward_vs_autograd."""
    from oracle import attn_inject as oinj, unet as ounet
    B = 3
    sd, tr = tiny_sat["sd"], tiny_sat["tr"]
    n = oinj.module_name(path)
    keys = [k for k in sd if k.startswith(n + ".")]
    g = torch.Generator().manual_seed(N * 1000 + T + C + 7)
    h = torch.randn(B, N, C, generator=g).half().float()
    state = (0.5 * torch.randn(B, T, 1024, generator=g)).half().float()
    dout = (0.05 * torch.randn(B, N, C, generator=g)).half().float()

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
    dstate = torch.zeros(B, T, 1024, device=DEV)
    inj.begin(state.half().to(DEV), gflat, dstate)
    inj.check_rows(B)
    out = inj(path, h.half().to(DEV).reshape(B * N, C), B, N, heads)
    L = inj.stash[path]["L"]
    assert L % 8 == 0 and 0 < L - (N + T) < 8
    dh = inj.backward(path, dout.half().to(DEV).reshape(B * N, C))
    inj.end()
    got = dict({k: tr.grad_view(gflat, k).cpu().reshape(sd[k].shape) for k in keys}, out=out.float().cpu().view(B, N, C),
               dh=dh.float().cpu().view(B, N, C), dstate=dstate.cpu())
    assert len(keys) == 11
    for k in ref:
        e, b = _rel(got[k], ref[k]), 2 * _rel(emu[k], ref[k]) + 2.0 ** -11
        print(f"[batched block C={C} N={N} T={T}] {k.replace(n + '.', ''):32s} hip {e:.2e}  bound {b:.2e}")
        assert e <= b, (k, e, b)


# ---------------------------------------------------------------------------------------------- 4. no cross-sample leakage
def test_no_cross_sample_leakage(tiny_sat, e2e, monkeypatch):
    """The B = 3 run with sample 2's latent, noise, timestep, prompt and sketch state replaced: the eps rows of sample 0 and d state[0]
    keep every bit (a wrong kv_stride, row offset or statistics index would mix samples)."""
    from sketch2img_amd import sat_train
    c = _case("B3_h16", tiny_sat, e2e)
    tr, net, bt, hw = tiny_sat["tr"], e2e["net"], c["bt"], c["h"] ** 2
    seen = []
    orig = sat_train.mse_seed
    monkeypatch.setattr(sat_train, "mse_seed", lambda eps, *a, **k: (seen.append(eps.clone()), orig(eps, *a, **k))[1])
    _, _, dst = tr.loss_and_grads(net, *c["args"], batched=True)
    assert torch.equal(dst, c["runs"][0][2])
    other = _batch(3, c["h"], seed=77)
    swap = lambda k: torch.cat([bt[k][:2], other[k][2:]])
    ts = c["ts"][:2] + (640,)
    _, _, dst2 = tr.loss_and_grads(net, swap("lat"), swap("noise"), ts, swap("ehs"), swap("state"), bt["acp"], batched=True)
    eps, eps2 = seen
    assert eps.shape[0] == 3 * hw
    assert torch.equal(eps[:hw], eps2[:hw]) and torch.equal(eps[hw:2 * hw], eps2[hw:2 * hw]) and not torch.equal(eps[2 * hw:], eps2[2 * hw:])
    assert torch.equal(dst[0], dst2[0]) and not torch.equal(dst[2], dst2[2])


# ---------------------------------------------------------------------------------------------- 5. pad rows are dead
def test_kv_pad_rows_are_dead(tiny_sat, e2e):
    """Rows N + T ... L - 1 of every sample in every kept K / V buffer overwritten with 1.0 between the forward and the backward: no
    bit of any gradient or of d state changes (they are masked by Nkv < kv_stride in dQ and dK / dV alike)."""
    c = _case("B3_h16", tiny_sat, e2e)
    tr, net = tiny_sat["tr"], e2e["net"]
    fw = tr.forward_batch(net, *c["args"], batched=True)
    (_, istash, _), = fw["kept"]
    assert len(istash) == 16
    pads = 0
    for st in istash.values():
        kv, N, L = st["kv"], st["N"], st["L"]
        NT = N + 257
        assert kv.shape[0] == 3 * L and L > NT
        for b in range(3):
            assert float(kv[b * L + NT:(b + 1) * L].abs().max()) == 0.0        # zeroed by the forward
            kv[b * L + NT:(b + 1) * L] = 1.0
            pads += L - NT
    assert pads > 0
    loss, g, dst = tr.backward_batch(net, fw, batched=True)
    assert torch.equal(g, c["runs"][0][1]) and torch.equal(dst, c["runs"][0][2]) and float(loss) == float(c["runs"][0][0])


# ---------------------------------------------------------------------------------------------- 6. backward_eps without an injector
@pytest.mark.parametrize("diff_from", [0, 1])
def test_backward_eps_all_rows_without_injector_vs_autograd(e2e, diff_from):
    """HipUNet.backward_eps on a rows = 3 evaluation with a timestep per row and no injector: diff_from = 0 differentiates all three
    rows, diff_from = 1 the last two.  d (eps . seed) / d x of those rows against autograd of the fp32 oracle (relative L2 <= 2 x the
    fp16-storage emulation's, as test_backward_eps_without_injector_vs_autograd)."""
    from oracle import unet as ounet
    from sketch2img_amd import ops
    from sketch2img_amd.unet import CIN_PAD, EPS_SEED_LD, Stash
    net, W, h, rows, ts = e2e["net"], e2e["W"], 16, 3, (37, 803, 411)
    S = rows - diff_from
    g = torch.Generator().manual_seed(11)
    x = torch.randn(rows, 4, h, h, generator=g).half().float()
    ehs = torch.randn(rows, 77, ounet.TINY.cross_attention_dim, generator=g).half().float()
    dE = torch.randn(rows, 4, h, h, generator=g).half().float()

    def run(emulate):
        xg = x.clone().requires_grad_(True)
        with ounet.fp16_storage(emulate):
            eps = ounet.unet_forward(ounet.TINY, W, xg, torch.tensor(ts), ehs)[0]
            (eps[diff_from:] * dE[diff_from:]).sum().backward()
        return xg.grad[diff_from:]

    ref, emu = run(False), run(True)
    net.prepare_context(ehs)
    stash = Stash()
    net.forward(ops.nchw_to_nhwc(x.to(DEV), CIN_PAD), list(ts), rows, h, stash, want_taps=False, want_eps=True, diff_from=diff_from)
    assert stash.first == diff_from
    seed = torch.zeros(S * h * h, EPS_SEED_LD, dtype=torch.float16, device=DEV)
    seed[:, :4] = dE[diff_from:].reshape(S, 4, h * h).transpose(1, 2).reshape(S * h * h, 4).half().to(DEV)
    dx = ops.nhwc_to_nchw(net.backward_eps(stash, seed), S, 4, h, h).cpu()
    e, b = _rel(dx, ref), 2 * _rel(emu, ref)
    print(f"[backward_eps rows=3 diff_from={diff_from}] d x: hip {e:.3e} bound {b:.3e}")
    assert e <= b
    for r in range(S):
        er, br = _rel(dx[r], ref[r]), 2 * _rel(emu[r], ref[r])
        print(f"[backward_eps rows=3 diff_from={diff_from}] row {diff_from + r}: hip {er:.3e} bound {br:.3e}")
        assert er <= br


# ---------------------------------------------------------------------------------------------- 7. the C = 320 block
def test_c320_transformer_block_all_rows_stashed(monkeypatch):
    """SD1.5's down_blocks.0.attentions.0 (C = 320, 8 heads; synthetic weights, rounded to fp16 for both sides) on rows = 3 and a
    16 x 16 map (HW = 256: the fused launches are eligible): _tr_fwd with a stash at diff_from = 0, then _tr_bwd of all three rows,
    against autograd of oracle.unet.transformer2d_forward.  Output and d x: relative L2 <= 2 x the emulation's.  Prints which
    launches ran; every stashing launch must have kept all rows (keep_from = 0)."""
    from oracle import unet as ounet
    from sketch2img_amd import ops, synthetic
    from sketch2img_amd.config import SD15
    from sketch2img_amd.unet import HipUNet, Stash
    p, rows, hh, C, heads = "down_blocks.0.attentions.0", 3, 16, 320, 8
    HW = hh * hh
    W = {k: v.half().float() for k, v in synthetic.unet_state_dict(SD15).items() if k.startswith(p + ".")}
    net = HipUNet(SD15, W, DEV)
    g = torch.Generator().manual_seed(320)
    x = torch.randn(rows, C, hh, hh, generator=g).half().float()
    ehs = torch.randn(rows, 77, SD15.cross_attention_dim, generator=g).half().float()
    dout = (0.05 * torch.randn(rows, C, hh, hh, generator=g)).half().float()

    def run(emulate):
        xg = x.clone().requires_grad_(True)
        with ounet.fp16_storage(emulate):
            out = ounet.transformer2d_forward(ounet.SD15, W, p, xg, ehs, heads)
            (out * dout).sum().backward()
        return out.detach(), xg.grad

    ref, emu = run(False), run(True)
    calls = []
    for name in ("xattn_block", "ff_block_proj", "ff_block", "gemm_geglu_keep"):
        def counted(*a, _f=getattr(ops, name), _n=name, **k):
            calls.append((_n, k.get("keep_from")))
            return _f(*a, **k)
        monkeypatch.setattr(ops, name, counted)
    tok = lambda t: t.permute(0, 2, 3, 1).reshape(rows * HW, C).half().to(DEV).contiguous()
    img = lambda t: t.float().cpu().view(rows, hh, hh, C).permute(0, 3, 1, 2)
    net.prepare_context(ehs)
    stash = Stash(rows=rows, first=0)
    out, _ = net._tr_fwd(p, tok(x), rows, (hh, hh), heads, stash, diff_from=0)
    fused = [c for c in calls if c[0] in ("xattn_block", "ff_block_proj", "ff_block")]
    print(f"[C=320 block rows=3 diff_from=0] launches: {calls} -> {'fused stashing' if fused else 'per-operator'}")
    assert calls and all(kf in (0, None) for _, kf in calls) and all(kf == 0 for _, kf in fused)
    st = stash.tr[p]
    assert st["f"].shape[0] == rows * HW and st["q2"].shape[0] == rows * HW and st["lse2"].shape[0] == rows
    dx = net._tr_bwd(p, tok(dout), rows, st)
    for tag, got, i in (("out", img(out), 0), ("d x", img(dx), 1)):
        e, b = _rel(got, ref[i]), 2 * _rel(emu[i], ref[i])
        print(f"[C=320 block rows=3 diff_from=0] {tag}: hip {e:.3e} bound {b:.3e}")
        assert e <= b, (tag, e, b)


# ---------------------------------------------------------------------------------------------- 8. train_step(batched=True)
def test_train_step_batched_with_the_tower(e2e, monkeypatch):
    """One optimizer step with the CLIP tower attached (TINY UNet, a 1-layer tower of 17 tokens, B = 2): a non-finite entry planted
    in EITHER flat gradient steps neither optimizer; then both step, and the parameters of both are within 1e-6 + 1e-5 max|p| (the
    bound of test_optimizer_step_and_loss_decrease) of torch.optim.AdamW fed the HIP gradients of the batched mode.  The UNet is
    walked once, at rows = B with diff_from = 0."""
    from oracle import attn_inject as oinj, clip_vision as oclip, unet as ounet
    from sketch2img_amd import config, sat_train
    from tests.test_gpu_clip_train import B, E2E_CLIP, TS, _batch as clip_batch, _trainers
    net = e2e["net"]
    ocfg = oclip.CLIPVisionConfig(**E2E_CLIP)
    env = dict(sd=oinj.init_state_dict(ounet.TINY, "clip"), cfg=config.CLIPVisionConfig(**E2E_CLIP), Wc=oclip.init_weights(ocfg))
    bt = clip_batch(16)
    walks = []
    fwd = net.forward
    monkeypatch.setattr(net, "forward", lambda x, t, rows, *a, **k: (walks.append((rows, k.get("diff_from"))), fwd(x, t, rows, *a, **k))[1])
    tr, tw = _trainers(env)
    step = lambda: sat_train.train_step(tr, net, bt["lat"], bt["ehs"], None, TS, bt["noise"], bt["acp"], tower=tw, pixel_values=bt["px"],
                                        batched=True)
    state = lambda: [t.clone() for o in (tr, tw) for t in (o.p, o.m, o.v, o.p16)]
    before = state()
    for victim in (tr, tw):
        def poisoned(g, bucket_bytes=15 << 20):
            g[11] = float("inf")
            return g
        victim.all_reduce = poisoned
        try:
            loss, stepped, _ = step()
        finally:
            del victim.all_reduce
        assert stepped is False and tr.step_count == 0 and tw.step_count == 0 and bool(torch.isfinite(loss))
        assert all(torch.equal(a, b) for a, b in zip(before, state()))
    _, g, gt, _ = sat_train.loss_and_grads_through_tower(tr, tw, net, bt["lat"], bt["noise"], TS, bt["ehs"], bt["px"], bt["acp"], batched=True)
    assert walks == [(B, 0)] * 3
    loss, stepped, dst = step()
    assert stepped is True and tr.step_count == 1 and tw.step_count == 1 and dst.shape[0] == B and net.inject is None
    for trn, grad, scale, init in ((tr, g, sat_train.LOSS_SCALE, env["sd"]), (tw, gt, sat_train.LOSS_SCALE * tw.seam_scale, env["Wc"])):
        keys = [k for k in trn.layout if not k.startswith("post_layernorm.")]
        p0 = {k: init[k].clone().float().requires_grad_(True) for k in keys}
        opt = torch.optim.AdamW([p0[k] for k in keys], lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
        for k in keys:
            p0[k].grad = trn.grad_view(grad, k).cpu().clone().reshape(p0[k].shape) / scale
        opt.step()
        new = trn.state_dict()
        for k in keys:
            assert (new[k].cpu() - p0[k].detach()).abs().max() < 1e-6 + 1e-5 * float(p0[k].detach().abs().max()), k
            assert torch.equal(trn.w16(k).float().cpu().reshape(new[k].shape), new[k].cpu().half().float()), k
