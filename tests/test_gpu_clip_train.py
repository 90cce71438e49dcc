"""CLIP vision tower training on the GPU (-m gpu): quick-GELU backward, the embedding fold, the stashing forward, the ViT backward
against autograd, the seam into the SatMixin step, the optimizer.

Reference gradients: torch autograd through oracle.clip_vision.last_hidden_state in fp32 on the CPU.  Bounds: twice the distance of the
fp16-storage EMULATION below (`_emulated_tokens`: the same forward with x.half().float() at every tensor the HIP path stores in fp16 -
autograd then rounds the gradients at the same places - plus fp16 softmax probabilities and fp16 dS, the operands of the attention
kernels' matrix products, and delta formed from the stored fp16 attention output) from the fp32 oracle.  Never from the HIP result.

Configurations: A = oracle.clip_vision.TINY_CLIP (D 64, 4 heads: d = 16, 17 tokens, Lp 24, 2 layers); B = hidden 128, 2 heads: d = 64,
image 224 / patch 14: 257 tokens, Lp 264 - the real padding and head size at the smallest width with two heads.  Batch 2."""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -24


@pytest.fixture(scope="module")
def ops():
    from sketch2img_amd import ops as o
    return o


def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-300))


# ---------------------------------------------------------------------------------------------- fp16-storage emulation of the tower
def _r(x):
    """Stored in fp16: the value is rounded, and autograd rounds the gradient at the same place."""
    return x.half().float()


class _FlashAttention(torch.autograd.Function):
    """softmax(q k^T scale) v the way the attention kernels store and re-read it.  Forward: the probabilities enter the P.V product as
    fp16, the output O is stored in fp16.  Backward, from the stored tensors as skg_attn_bwd_dq_delta / _dkv do it: delta = rowsum(dO . O)
    with the fp16 O, P recomputed in fp32, dS = P (dO v^T - delta) rounded to fp16 before the dQ / dK products, dV = fp16(P)^T dO.
    (With the stored O, the rows of dS no longer sum to zero exactly - which is all there is to d k_proj.bias, zero in exact
    arithmetic.)  dq / dk / dv are rounded where they are stored: by the _r() of q / k / v outside."""

    @staticmethod
    def forward(ctx, q, k, v, scale):
        p = torch.softmax(q @ k.transpose(-1, -2) * scale, dim=-1)
        o = (p.half().float() @ v).half().float()
        ctx.save_for_backward(q, k, v, p, o)
        ctx.scale = scale
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, p, o = ctx.saved_tensors
        delta = (do * o).sum(-1, keepdim=True)
        ds = (p * (do @ v.transpose(-1, -2) - delta)).half().float()
        return ds @ k * ctx.scale, ds.transpose(-1, -2) @ q * ctx.scale, p.half().float().transpose(-1, -2) @ do, None


class _SeamFactor(torch.autograd.Function):
    """Identity; the gradient is multiplied by the tower's seam scale on its way into the tower, before its fp16 rounding there."""

    @staticmethod
    def forward(ctx, x, factor):
        ctx.factor = factor
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.factor, None


def _emulated_tokens(cfg, W, pixels):
    """oracle.clip_vision.last_hidden_state restated with fp16 storage where HipCLIPVision.forward_train stores fp16."""
    from oracle.clip_vision import quick_gelu
    B = pixels.shape[0]
    D, H = cfg.hidden_size, cfg.num_attention_heads
    d, eps = D // H, cfg.layer_norm_eps
    x = _r(F.conv2d(_r(pixels), W["embeddings.patch_embedding.weight"], stride=cfg.patch_size)).flatten(2).transpose(1, 2)
    pos = W["embeddings.position_embedding.weight"]
    pack = _r(torch.cat([pos[:1] + W["embeddings.class_embedding"][None], pos[1:]]))        # row 0 = class + its position
    x = _r(torch.cat([torch.zeros(B, 1, D), x], dim=1) + pack[None])
    x = _r(F.layer_norm(x, (D,), W["pre_layrnorm.weight"], W["pre_layrnorm.bias"], eps))
    N = x.shape[1]
    for l in range(cfg.num_hidden_layers):
        p = f"encoder.layers.{l}"
        h = _r(F.layer_norm(x, (D,), W[p + ".layer_norm1.weight"], W[p + ".layer_norm1.bias"], eps))
        q, k, v = (_r(F.linear(h, W[f"{p}.self_attn.{n}.weight"], W[f"{p}.self_attn.{n}.bias"])).reshape(B, N, H, d).transpose(1, 2)
                   for n in ("q_proj", "k_proj", "v_proj"))
        a = _r(_FlashAttention.apply(q, k, v, d ** -0.5).transpose(1, 2).reshape(B, N, D))
        x = _r(x + F.linear(a, W[p + ".self_attn.out_proj.weight"], W[p + ".self_attn.out_proj.bias"]))
        h = _r(F.layer_norm(x, (D,), W[p + ".layer_norm2.weight"], W[p + ".layer_norm2.bias"], eps))
        f = _r(F.linear(h, W[p + ".mlp.fc1.weight"], W[p + ".mlp.fc1.bias"]))
        x = _r(x + F.linear(_r(quick_gelu(f)), W[p + ".mlp.fc2.weight"], W[p + ".mlp.fc2.bias"]))
    return x


def _tower_grads(cfg, W, pixels, d_tokens, emulate):
    """{key: d (sum d_tokens . tokens) / d W[key]} by autograd, fp32 CPU."""
    from oracle import clip_vision as oclip
    p = {k: v.clone().requires_grad_(True) for k, v in W.items()}
    tok = _emulated_tokens(cfg, p, pixels) if emulate else oclip.last_hidden_state(cfg, p, pixels)
    (tok * d_tokens).sum().backward()
    return {k: p[k].grad for k in p}


# ---------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("M,C,pad,alias", [(5, 8, 0, False), (264, 136, 0, False), (264, 136, 24, False), (1056, 256, 0, False),
                                           (1056, 256, 0, True)])
def test_quick_gelu_bwd_matches_fp64(ops, M, C, pad, alias):
    """skg_quick_gelu_bwd_f16 against fp64 on the same fp16 inputs; f ~ 3 N(0, 1) reaches both tails of the sigmoid, dY ~ N(0, 1).
    pad: all three operands are column views of wider buffers; alias: out is dY.
    Bound.  With a = 1.702 f the factor g = s (1 + a (1 - s)) has |g| <= 1.0998 < 1.13.  In fp32: the product 1.702 f and the
    exponential's argument scaling carry about (1.5 |a| + 3) u relative into e = exp(-a), which reaches s as s (1 - s) times that and g
    as |1 + a (1 - 2 s)| times that again: under 2 u for every a.  The reciprocal, 1 - s, the two products and the sum inside g and the
    product with dY add one rounding of at most 1.13 each: 6 more.  16 roundoffs of 1.13 |dY| cover both with a factor two to spare.
    Then ONE fp16 rounding of the result (2^-11 relative) or, below the normal range, fp16's smallest subnormal 2^-24:
        |err| <= 2^-11 |ref| + 16 u 1.13 |dY| + 2^-24."""
    g = torch.Generator().manual_seed(M * 31 + C + pad)
    f = (3 * torch.randn(M, C, generator=g)).half()
    dY = torch.randn(M, C, generator=g).half()

    def dev(t):
        if not pad:
            return t.to(DEV).clone()
        buf = torch.full((M, C + pad), 3.0, dtype=torch.float16, device=DEV)
        buf[:, 8:8 + C] = t.to(DEV)
        return buf[:, 8:8 + C]

    fd, dYd = dev(f), dev(dY)
    out = dYd if alias else dev(torch.zeros(M, C).half())
    got = ops.quick_gelu_bwd(fd, dYd, out=out)
    assert got.data_ptr() == out.data_ptr()
    if not alias:
        assert torch.equal(dYd.cpu(), dY) and torch.equal(ops.quick_gelu_bwd(fd, dYd).cpu(), got.cpu())     # out=None allocates
    assert torch.equal(fd.cpu(), f)
    a = 1.702 * f.double()
    s = torch.sigmoid(a)
    ref = dY.double() * s * (1 + a * (1 - s))
    bound = 2.0 ** -11 * ref.abs() + 16 * U * 1.13 * dY.double().abs() + 2.0 ** -24
    e = (got.cpu().double() - ref).abs()
    print(f"quick_gelu_bwd {M}x{C} pad {pad} alias {alias}: max err / bound = {float((e / bound).max()):.3f}")
    assert (e <= bound).all()
    if M * C >= 1000:
        assert float(f.float().min()) < -6 and float(f.float().max()) > 6                 # both tails were exercised


@pytest.mark.parametrize("B", [1, 3])
def test_embedding_fold_matches_fp64_and_is_repeatable(B):
    """dpos[n] = sum over the images of row n of d x0 (configuration B's padding: 257 of 264 rows), fp32 accumulation in ascending
    image order: against an fp64 sum with |err| <= (B - 1) u sum|terms| + u |ref| (B - 1 additions, one final scaling by 1); two
    runs give the same bits."""
    from oracle import clip_vision as oclip
    from sketch2img_amd.clip_vision import HipCLIPVision
    from sketch2img_amd.config import CLIPVisionConfig
    cfg = CLIPVisionConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=2)
    vis = HipCLIPVision(cfg, oclip.init_weights(oclip.CLIPVisionConfig(128, 256, 1, 2)), DEV)
    N, Lp, D = cfg.num_tokens, vis.Lp, cfg.hidden_size
    assert (N, Lp) == (257, 264)
    g = torch.Generator().manual_seed(B)
    dx0 = torch.randn(B * Lp, D, generator=g).half()
    x = dx0.to(DEV)
    a, b = vis.embedding_fold(x, B).clone(), vis.embedding_fold(x, B).clone()
    assert torch.equal(a, b) and a.shape == (N, D) and a.dtype == torch.float32
    terms = dx0.double().view(B, Lp, D)[:, :N]
    ref, mag = terms.sum(0), terms.abs().sum(0)
    e = (a.cpu().double() - ref).abs()
    bound = (B - 1) * U * mag + U * ref.abs()
    print(f"embedding fold B={B}: max err {float(e.max()):.2e}")
    assert (e <= bound).all()


# ---------------------------------------------------------------------------------------------- the tower
def _cfgs(name):
    from oracle import clip_vision as oclip
    from sketch2img_amd import config
    if name == "A":
        return oclip.TINY_CLIP, config.TINY_CLIP
    kw = dict(hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=2, image_size=224, patch_size=14)
    return oclip.CLIPVisionConfig(**kw), config.CLIPVisionConfig(**kw)


@pytest.fixture(scope="module")
def towers():
    """Per configuration: weights, pixels, a seeded fp16-exact d_tokens, the oracle's and the emulation's gradients (computed once,
    shared, left unchanged) and a HipClipTowerTrainer."""
    from oracle import clip_vision as oclip
    from sketch2img_amd.clip_vision_train import HipClipTowerTrainer
    out = {}
    for name in ("A", "B"):
        ocfg, cfg = _cfgs(name)
        W = oclip.init_weights(ocfg)
        g = torch.Generator().manual_seed(7 + len(W))
        px = torch.randn(2, 3, cfg.image_size, cfg.image_size, generator=g).half().float()
        dtok = (0.05 * torch.randn(2, cfg.num_tokens, cfg.hidden_size, generator=g)).half().float()
        out[name] = dict(ocfg=ocfg, cfg=cfg, W=W, px=px, dtok=dtok, ref=_tower_grads(ocfg, W, px, dtok, False),
                         emu=_tower_grads(ocfg, W, px, dtok, True), tr=HipClipTowerTrainer(cfg, W, DEV, lr=2e-4, warmup_steps=0))
    return out


@pytest.mark.parametrize("name", ["A", "B"])
def test_forward_train_equals_last_hidden_state(towers, name):
    """The stashing forward makes the same launches: bit-identical tokens to HipCLIPVision.last_hidden_state on the same weights, and
    within the inference tower's tolerance of the fp32 oracle."""
    from oracle import clip_vision as oclip
    from sketch2img_amd.clip_vision import HipCLIPVision
    t = towers[name]
    tok, kept = t["tr"].forward_train(t["px"])
    want = HipCLIPVision(t["cfg"], t["W"], DEV).last_hidden_state(t["px"])
    assert tok.dtype == torch.float16 and tok.shape == (2, t["cfg"].num_tokens, t["cfg"].hidden_size)
    assert torch.equal(tok, want)
    assert torch.equal(t["tr"].vision.last_hidden_state(t["px"]), want)           # the same object's own inference walk
    assert len(kept["layers"]) == t["cfg"].num_hidden_layers
    for k in ("x1", "s1", "h1", "qkv", "a", "lse", "x2", "s2", "h2", "f", "act"):
        assert k in kept["layers"][0], k
    assert _rel(tok.float().cpu(), oclip.last_hidden_state(t["ocfg"], t["W"], t["px"])) < 5e-3


def test_training_forward_equals_an_inference_tower_built_from_the_checkpoint():
    """Masters that are NOT fp16-exact (as after any optimizer step): the training forward's tokens are bit-identical to those of an
    inference HipCLIPVision packed from the trainer's state_dict() - in particular pack row 0 is fp16(pos32[0] + class32), one rounding
    of the fp32 sum, on both sides."""
    from oracle import clip_vision as oclip
    from sketch2img_amd.clip_vision import HipCLIPVision
    from sketch2img_amd.clip_vision_train import HipClipTowerTrainer
    ocfg, cfg = _cfgs("A")
    g = torch.Generator().manual_seed(3)
    W = {k: v * (1 + 1e-3 * torch.randn(v.shape, generator=g)) for k, v in oclip.init_weights(ocfg).items()}
    assert any(not torch.equal(v.half().float(), v) for v in W.values())
    px = torch.randn(2, 3, cfg.image_size, cfg.image_size, generator=g).half().float()
    tr = HipClipTowerTrainer(cfg, W, DEV)
    tok, _ = tr.forward_train(px)
    ckpt = {k: v.cpu() for k, v in tr.state_dict().items()}                        # what torch.save / torch.load hand back
    assert torch.equal(tok, HipCLIPVision(cfg, ckpt, DEV).last_hidden_state(px))


def _hip_grads(t, kept=None):
    tr = t["tr"]
    if kept is None:
        _, kept = tr.forward_train(t["px"])
    g = tr.new_grad()
    tr.backward(kept, t["dtok"].half().to(DEV), g)
    return g


@pytest.mark.parametrize("name", ["A", "B"])
def test_tower_backward_vs_autograd(towers, name):
    """HipCLIPVision.backward against autograd of the fp32 oracle, loss = sum(d_tokens . tokens), for EVERY parameter tensor of
    oracle.clip_vision.param_shapes: relative L2 <= 2 x the emulation's distance + 2^-11 (one fp16 rounding, for tensors the
    emulation leaves unrounded); post_layernorm.* gets exactly zero; two runs are bit-equal.
    d k_proj.bias is zero in exact arithmetic (a constant added to every key shifts all scores of a row alike), so for it both sides
    of the comparison are rounding noise relative to the oracle's own ~1e-8 noise: the emulation forms delta from the stored fp16
    attention output as the kernels do, which is what makes the rows of dS sum to something other than zero.
    Measured on one MI355X, worst HIP figure / its bound by ratio: A 9.73e-4 / 2.32e-3 (layers.1.q_proj.bias), B 6.81e-4 / 1.84e-3
    (layers.0.q_proj.weight); d k_proj.bias A 3.89e+3 / 8.02e+3, B 2.13e+3 / 3.57e+3."""
    from oracle import clip_vision as oclip
    t = towers[name]
    tr = t["tr"]
    g, g2 = _hip_grads(t), _hip_grads(t)
    assert torch.equal(g, g2) and bool(torch.isfinite(g).all())
    keys = list(oclip.param_shapes(t["ocfg"]))
    assert set(keys) == set(tr.layout)
    fails, worst = [], (0.0, 0.0, "")
    for k in keys:
        got = tr.grad_view(g, k).cpu()
        if k.startswith("post_layernorm."):
            assert float(got.abs().max()) == 0.0 and t["ref"][k] is None
            continue
        e, b = _rel(got, t["ref"][k]), 2 * _rel(t["emu"][k], t["ref"][k]) + 2.0 ** -11
        print(f"[tower {name}] {k:48s} hip {e:.2e}  bound {b:.2e}")
        if e / b > worst[0] / (worst[1] or 1.0):
            worst = (e, b, k)
        if e > b:
            fails.append((k, e, b))
    print(f"[tower {name}] worst pair: hip {worst[0]:.3e} bound {worst[1]:.3e} ({worst[2]})")
    assert not fails, fails


def test_pad_rows_are_inert(towers):
    """Configuration B (7 pad rows per image): with every kept activation's pad rows overwritten by 1.0 before backward, no gradient
    changes by a bit - the zeroed seed and the zeroed dq / dk / dv buffer are all the masking there is."""
    t = towers["B"]
    tr = t["tr"]
    N, Lp = t["cfg"].num_tokens, tr.vision.Lp if tr.vision is not None else 264
    g0 = _hip_grads(t)
    _, kept = tr.forward_train(t["px"])
    touched = 0
    acts = [kept["x0"]] + [v for lay in kept["layers"] for k, v in lay.items() if k not in ("s1", "s2", "lse")]
    for a in acts:
        assert a.dtype == torch.float16 and a.shape[0] == 2 * Lp
        a.view(2, Lp, -1)[:, N:] = 1.0
        touched += 1
    assert touched == 1 + 8 * t["cfg"].num_hidden_layers and Lp - N == 7
    assert torch.equal(_hip_grads(t, kept), g0)


# ---------------------------------------------------------------------------------------------- end to end through the seam
SCALE = 0.8
B, TS = 2, (37, 803)
E2E_CLIP = dict(hidden_size=1024, intermediate_size=256, num_hidden_layers=1, num_attention_heads=16, image_size=56, patch_size=14)


def _batch(h):
    from oracle import ddim as oddim, unet as ounet
    g = torch.Generator().manual_seed(100 + h)
    cfg = ounet.TINY
    return dict(lat=torch.randn(B, 4, h, h, generator=g), noise=torch.randn(B, 4, h, h, generator=g),
                ehs=torch.randn(B, 77, cfg.cross_attention_dim, generator=g).half().float(),
                px=torch.randn(B, 3, 56, 56, generator=g).half().float(),
                acp=oddim.make_tables(50).alphas_cumprod)


def _oracle(W, sd, ocfg, Wc, bt, emulate, loss_scale, seam=1.0):
    """(loss, SatMixin grads, tower grads) of the oracle UNet with the CLIP injector fed by the tower, by autograd; the emulation
    multiplies the loss by the loss scale and the gradient entering the tower by the seam scale, as the HIP path does."""
    from oracle import attn_inject as oinj, clip_vision as oclip, unet as ounet
    from sketch2img_amd.sat_train import add_noise
    p = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    pc = {k: v.clone().requires_grad_(True) for k, v in Wc.items()}
    noisy = add_noise(bt["lat"], bt["noise"], TS, bt["acp"])
    with ounet.fp16_storage(emulate):
        st = _emulated_tokens(ocfg, pc, bt["px"]) if emulate else oclip.last_hidden_state(ocfg, pc, bt["px"])
        st = _SeamFactor.apply(st, seam)
        eps = torch.cat([ounet.unet_forward(ounet.TINY, W, noisy[b:b + 1], TS[b], bt["ehs"][b:b + 1],
                                            inject=oinj.make_clip_inject(p, st[b:b + 1], SCALE))[0] for b in range(B)])
        loss = F.mse_loss(eps, bt["noise"])
        (loss * loss_scale).backward()
    return (float(loss.detach()), {k: p[k].grad / loss_scale for k in p},
            {k: (None if pc[k].grad is None else pc[k].grad / (loss_scale * seam)) for k in pc})


@pytest.fixture(scope="module")
def e2e():
    from oracle import attn_inject as oinj, clip_vision as oclip, unet as ounet
    from sketch2img_amd import config
    from sketch2img_amd.unet import HipUNet
    W = ounet.init_weights(ounet.TINY)
    ocfg = oclip.CLIPVisionConfig(**E2E_CLIP)
    return dict(W=W, net=HipUNet(config.TINY, W, DEV), sd=oinj.init_state_dict(ounet.TINY, "clip"), ocfg=ocfg,
                cfg=config.CLIPVisionConfig(**E2E_CLIP), Wc=oclip.init_weights(ocfg), bt=_batch(16))


def _trainers(e2e):
    from sketch2img_amd import config, sat_train
    from sketch2img_amd.clip_vision_train import HipClipTowerTrainer
    kw = dict(lr=2e-4, warmup_steps=0, total_steps=1 << 20)
    return (sat_train.HipSatTrainer(config.TINY, e2e["sd"], DEV, scale=SCALE, **kw), HipClipTowerTrainer(e2e["cfg"], e2e["Wc"], DEV, **kw))


def test_training_through_the_seam_end_to_end(e2e):
    """TINY UNet, 16 x 16 latents, B = 2, timesteps (37, 803); tower: hidden 1024 (the injector's CLIP_DIM), 16 heads, I 256, 1 layer,
    17 tokens.  Loss within 2e-3 relative of the fp32 oracle's; every SatMixin gradient and every tower gradient (post_layernorm.*:
    exactly zero) within 2 x the emulation's distance (oracle.unet.fp16_storage + the tower emulation above, loss x LOSS_SCALE, the
    gradient x the seam scale where it enters the tower) per tensor; the SatMixin gradients bit-equal to loss_and_grads fed the same tokens as sketch_state."""
    from sketch2img_amd import sat_train
    tr, tw = _trainers(e2e)
    bt, net = e2e["bt"], e2e["net"]
    total = sat_train.LOSS_SCALE * tw.seam_scale
    ref = _oracle(e2e["W"], e2e["sd"], e2e["ocfg"], e2e["Wc"], bt, False, 1.0)
    emu = _oracle(e2e["W"], e2e["sd"], e2e["ocfg"], e2e["Wc"], bt, True, sat_train.LOSS_SCALE, tw.seam_scale)
    args = (net, bt["lat"], bt["noise"], TS, bt["ehs"], bt["px"], bt["acp"])
    loss, g, gt, dst = sat_train.loss_and_grads_through_tower(tr, tw, *args)
    loss2, g2, gt2, dst2 = sat_train.loss_and_grads_through_tower(tr, tw, *args)
    assert torch.equal(g, g2) and torch.equal(gt, gt2) and torch.equal(dst, dst2) and float(loss) == float(loss2)
    assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(gt).all()) and net.inject is None
    # the tower does not disturb the existing path
    tokens, _ = tw.forward_train(bt["px"])
    loss3, g3, dst3 = tr.loss_and_grads(net, bt["lat"], bt["noise"], TS, bt["ehs"], tokens, bt["acp"])
    assert torch.equal(g, g3) and torch.equal(dst, dst3) and float(loss) == float(loss3)
    print(f"[seam e2e] loss hip {float(loss):.6f} oracle {ref[0]:.6f} emulation {emu[0]:.6f}")
    assert abs(float(loss) - ref[0]) <= 2e-3 * ref[0]
    fails = []
    for tag, trn, grad, scale, rg, eg in (("sat", tr, g, sat_train.LOSS_SCALE, ref[1], emu[1]), ("tower", tw, gt, total, ref[2], emu[2])):
        worst = (0.0, 1.0, "")
        for k in rg:
            got = trn.grad_view(grad, k).cpu() / scale
            if rg[k] is None:
                assert k.startswith("post_layernorm.") and float(got.abs().max()) == 0.0
                continue
            e, b = _rel(got, rg[k]), 2 * _rel(eg[k], rg[k])
            if e / max(b, 1e-300) > worst[0] / worst[1]:
                worst = (e, b, k)
            if e > b:
                fails.append((k, e, b))
                print(f"[seam e2e] OVER {k}: hip {e:.3e} bound {b:.3e}")
        print(f"[seam e2e] {tag}: worst pair hip {worst[0]:.3e} bound {worst[1]:.3e} ({worst[2]})")
    assert not fails, fails


def test_optimizers_step_together(e2e):
    """One step of the tower's AdamW against torch.optim.AdamW fed the HIP gradients (1e-6 + 1e-5 max|p|), fp16 copy = the rounded
    masters, post_layernorm.* unchanged; a NaN planted in EITHER flat gradient (at the all-reduce, where train_step holds it) makes
    train_step return stepped = False with both trainers' p, m, v, fp16 copy and step count untouched; then the loss falls over three
    steps on the fixed batch."""
    from sketch2img_amd import sat_train
    tr, tw = _trainers(e2e)
    bt, net = e2e["bt"], e2e["net"]
    Wc = e2e["Wc"]
    step = lambda: sat_train.train_step(tr, net, bt["lat"], bt["ehs"], None, TS, bt["noise"], bt["acp"], tower=tw, pixel_values=bt["px"])
    state = lambda: [t.clone() for o in (tr, tw) for t in (o.p, o.m, o.v, o.p16)]
    before = state()
    for victim in (tr, tw):
        def poisoned(g, bucket_bytes=15 << 20):
            g[11] = float("nan")
            return g
        victim.all_reduce = poisoned
        try:
            loss, stepped, _ = step()
        finally:
            del victim.all_reduce
        assert stepped is False and tr.step_count == 0 and tw.step_count == 0 and bool(torch.isfinite(loss))
        assert all(torch.equal(a, b) for a, b in zip(before, state()))
    # one tower step vs torch AdamW on the same numbers
    _, _, gt, _ = sat_train.loss_and_grads_through_tower(tr, tw, net, bt["lat"], bt["noise"], TS, bt["ehs"], bt["px"], bt["acp"])
    keys = [k for k in tw.layout if not k.startswith("post_layernorm.")]
    p0 = {k: Wc[k].clone().float().requires_grad_(True) for k in keys}
    opt = torch.optim.AdamW([p0[k] for k in keys], lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    for k in keys:
        p0[k].grad = tw.grad_view(gt, k).cpu().clone() / (sat_train.LOSS_SCALE * tw.seam_scale)
    opt.step()
    assert tw.step(gt) is True and tw.step_count == 1
    new = tw.state_dict()
    for k in keys:
        assert (new[k].cpu() - p0[k].detach()).abs().max() < 1e-6 + 1e-5 * float(p0[k].detach().abs().max()), k
        assert torch.equal(tw.w16(k).float().cpu(), new[k].cpu().half().float()), k
    for k in ("post_layernorm.weight", "post_layernorm.bias"):
        assert torch.equal(new[k].cpu(), Wc[k]) and torch.equal(tw.w16(k).float().cpu(), Wc[k])
    # both optimizers on the fixed batch
    tr, tw = _trainers(e2e)
    losses = []
    for i in range(3):
        loss, stepped, _ = step()
        assert stepped is True and tr.step_count == tw.step_count == i + 1
        losses.append(float(loss))
    losses.append(float(step()[0]))
    print("[seam train] losses:", " ".join(f"{v:.5f}" for v in losses))
    assert all(b < a for a, b in zip(losses, losses[1:]))
