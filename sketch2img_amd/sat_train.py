"""One training step of the CLIP-token injected attention (SatMixin) on the libskg.so kernels (reference trainer:
modules/clip_guided_trainer.py:203-236).

    frozen UNet with one SatMixin block per BasicTransformerBlock  ->  every sample noised at its own timestep  ->
    loss = mse(unet(noisy, t, ehs), noise)  ->  backward through the whole UNet into the 16 injected modules  ->
    gradient all-reduce across ranks (DDP, bucket_cap_mb = 15)  ->  AdamW, cosine_with_restarts schedule.

How it runs here by default: one sample at a time (rows = 1) - every sample has its own timestep and the time-embedding bias is folded
into the conv epilogues per launch - with a Stash, so every block takes the unfused stashing launches; the injector is
inject.HipClipInjectorTrain (forward with stash, backward with weight gradients); the backward is HipUNet.backward_eps.  The
gradients of the B samples accumulate (+=) inside one flat fp32 vector; the loss and its seed come from ONE launch over the
whole batch (skg_lgp_mse_train: the same [B*hw, >= 4] / NCHW layouts), so the seed carries 1 / numel of the whole batch.

batched=True (opt-in, every entry point below): the reference's call form - ONE UNet walk at rows = B with a timestep per row
(a bias row per sample in conv1's epilogue), a stash of every row (HipUNet.forward(diff_from=0)), the injector on B token sets
(image rows and token rows as two tensors, K / V gathered per sample into one padded buffer, the attention trio at batch = B, every
weight gradient contracted over all samples' rows) and one backward_eps over all rows.  Same values to rounding, not to the bit.

What differs from the reference, on purpose (as in lgp_train.py): accelerate's fp16 autocast becomes fp16 compute with fp32 master
weights and, by default, a STATIC power-of-two loss scale; the reference's GradScaler is train_step(scaler=) with a
loss_scaler.DynamicLossScaler (one scaler, one verdict for SatMixin and tower).  bitsandbytes' AdamW8bit becomes plain fp32 AdamW
with the same hyper-parameters.

The CLIP vision tower, which the reference trains in the same optimizer (clip_guided_trainer.py:116-119), attaches at the seam:
loss_and_grads returns d loss / d sketch_state, and train_step(tower=, pixel_values=) takes the sketch tokens from
clip_vision_train.HipClipTowerTrainer.forward_train, casts d sketch_state (fp32, x LOSS_SCALE, x the tower's power-of-two seam
scale) to fp16, runs HipCLIPVision.backward from it, all-reduces both flat gradients and steps both optimizers or - when either
gradient is non-finite, the reference's single GradScaler - neither.  Without a tower nothing changes.

Loss scale: gradients of the unscaled loss are 1e-6 ... 1e-5 and underflow fp16 (6 of the 11 parameter kinds off by 30-100 %);
between 2^10 and 2^16 every tensor is within 5e-3 of the fp32 oracle.  LOSS_SCALE = 2^13 sits in the middle of that
plateau: the seed 2^13 * 2 (eps - noise) / numel is 2 (eps - noise) at the TINY test size (numel 8192) and (eps - noise) / 4 at
SD1.5's 4 x 4 x 64 x 64 - both far from fp16's 6e-5 / 65504 limits.

LR schedule - diffusers "cosine_with_restarts", num_cycles = 1 (clip_guided_trainer.py:135-140), for optimizer step s (0-based):
    s < warmup:   lr * s / max(1, warmup)
    otherwise:    p = (s - warmup) / max(1, total - warmup);  lr * 0 if p >= 1 else lr * max(0, (1 + cos(pi * ((cycles * p) mod 1))) / 2)
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import torch

from . import lgp_train, ops
from .clip_text import encode_tokens  # noqa: F401 (re-exported: the trainer's long-prompt encoding, clip_guided_trainer.py:40-66)
from .config import UNetConfig
from .flat_adamw import FlatAdamW, cosine_with_restarts  # noqa: F401 (cosine_with_restarts is re-exported)
from .inject import CLIP_DIM, HipClipInjectorTrain, block_dims, module_name
from .lgp_train import row_groups

LOSS_SCALE = 8192.0        # 2^13, see the module docstring
_LEAVES = ("sketch_proj.weight", "sketch_proj.bias", "sketch_norm.weight", "sketch_norm.bias", "sketch_attn.to_q.weight",
           "sketch_attn.to_k.weight", "sketch_attn.to_v.weight", "sketch_attn.to_out.0.weight", "sketch_attn.to_out.0.bias",
           "sketch_conv.weight", "sketch_conv.bias")


def param_shapes(cfg: UNetConfig) -> "Dict[str, Tuple[int, ...]]":
    """SatMixin.state_dict() keys / shapes of the CLIP variant, in the checkpoint's order."""
    out: Dict[str, Tuple[int, ...]] = {}
    for path, c, _ in block_dims(cfg):
        n = module_name(path)
        for leaf in _LEAVES:
            if leaf == "sketch_proj.weight":
                shp: Tuple[int, ...] = (c, CLIP_DIM)
            elif leaf == "sketch_conv.weight":
                shp = (c, c, 1)
            elif leaf.endswith("bias") or leaf.startswith("sketch_norm"):
                shp = (c,)
            else:
                shp = (c, c)
            out[f"{n}.{leaf}"] = shp
    return out


def mse_seed(eps16: torch.Tensor, noise: torch.Tensor, B: int, h: int, loss_scale: float = LOSS_SCALE):
    """eps16 fp16 [B*h*h, >= 4] (the UNet's output rows of all samples), noise fp32 [B, 4, h, h] ->
    (loss = mean((eps - noise)^2) over the whole batch, d eps = loss_scale * 2 (eps - noise) / numel as fp16
    [B*h*h, EPS_SEED_LD], 4 valid channels, the rest zero)."""
    from .unet import EPS_SEED_LD
    noise = noise.to(eps16.device, torch.float32).contiguous()
    assert noise.shape == (B, 4, h, h) and eps16.shape[0] == B * h * h
    seed, parts = ops.lgp_mse_train(eps16, noise, B, h, EPS_SEED_LD, loss_scale)
    return parts.sum(), seed


def add_noise(latents: torch.Tensor, noise: torch.Tensor, timesteps: Sequence[int], alphas_cumprod: torch.Tensor):
    """DDPMScheduler.add_noise with host-side fp32 scalars per sample."""
    return lgp_train.add_noise(latents, noise, timesteps, alphas_cumprod)[0]


class HipSatTrainer(FlatAdamW):
    def __init__(self, cfg: UNetConfig, state_dict: Dict[str, torch.Tensor], device="cuda", lr: float = 2e-4,
                 betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2, warmup_steps: int = 150,
                 total_steps: int = 10000, num_cycles: int = 1, scale: float = 1.0, state_bits: int = 32,
                 min_8bit_size: int = 4096):
        # state_bits / min_8bit_size: FlatAdamW's (8: block-wise quantised m / v, the reference's AdamW8bit)
        # the master vector is in the checkpoint's key order: state_dict() is the reference's sketch_attn_model.pt
        super().__init__(list(param_shapes(cfg).items()), state_dict, device, lr, betas, eps, weight_decay,
                         lambda s: cosine_with_restarts(s, warmup_steps, total_steps, num_cycles), LOSS_SCALE,
                         state_bits=state_bits, min_8bit_size=min_8bit_size)
        self.cfg = cfg
        self.injector = HipClipInjectorTrain(cfg, self.w16, self.grad_view, self.dev)
        self.injector.set_scale(scale)
        self.stale = True          # (FlatAdamW's flag: the injector's packs are built by the first forward_batch)

    # ------------------------------------------------------------------------------------------ fwd + bwd
    @torch.no_grad()
    def loss_and_grads(self, net, latents: torch.Tensor, noise: torch.Tensor, timesteps: Sequence[int], ehs: torch.Tensor,
                       sketch_state: torch.Tensor, alphas_cumprod: torch.Tensor, loss_scale: float = LOSS_SCALE, batched: bool = False):
        """latents, noise fp32 [B, 4, h, h]; timesteps: B ints; ehs [B, L, D] (L = 77, or 78 ... 231 from encode_tokens); sketch_state [B, T, 1024].
        loss_scale: a power of two (step() divides by LOSS_SCALE: leave the default unless the caller rescales itself).
        Returns (loss, flat fp32 gradient x LOSS_SCALE in the layout of the master vector, d loss / d sketch_state x LOSS_SCALE
        fp32 [B, T, 1024]).
        batched: the whole batch in ONE UNet walk - the reference's unet(noisy_latents, timesteps, encoder_hidden_states) - instead of
        one rows = 1 evaluation per sample: the same values to rounding (other kernel instantiations), B >= 1."""
        fw = self.forward_batch(net, latents, noise, timesteps, ehs, sketch_state, alphas_cumprod, loss_scale, batched=batched)
        return self.backward_batch(net, fw, batched=batched)

    @torch.no_grad()
    def forward_batch(self, net, latents, noise, timesteps, ehs, sketch_state, alphas_cumprod, loss_scale: float = LOSS_SCALE,
                      batched: bool = False):
        """The stashing forward of every row group - the samples one by one - the loss and its seed (the loss is a mean over the
        whole batch, so all forwards come first).  Returns what backward_batch consumes (with the same `batched`).
        batched: one group, the batch - one prepare_context, one stashing forward at rows = B with a timestep per row and
        diff_from = 0 (every row is differentiated), the injector holding all B token sets."""
        from .unet import CIN_PAD, Stash
        if net.residual_fp32:
            raise NotImplementedError("HipSatTrainer: the accuracy mode (residual_fp32) is not supported - build the HipUNet "
                                      "without residual_fp32")
        B, _, h, w = latents.shape
        assert h == w, "square maps only"
        dev = self.dev
        if self.stale:             # an optimizer step ran since the injector's packs were built (FlatAdamW.step / settle)
            self.stale = False
            self.injector.refresh()
        if batched and len(timesteps) != B:
            raise ValueError(f"timesteps: {len(timesteps)} entries for {B} samples")
        noise = noise.to(dev, torch.float32).contiguous()
        noisy = add_noise(latents.to(dev, torch.float32), noise, timesteps, alphas_cumprod)
        state16 = sketch_state.to(dev, torch.float16)
        T = state16.shape[1]
        hw = h * h
        g = self.new_grad()
        dstate = torch.zeros(B, T, CLIP_DIM, device=dev, dtype=torch.float32)
        eps_all = None if batched else torch.empty(B * hw, 8, device=dev, dtype=torch.float16)
        kept = []
        prev = net.inject
        net.inject = self.injector
        try:
            for b0, b1 in row_groups(B, batched):
                net.prepare_context(ehs[b0:b1])
                x32 = ops.nchw_to_nhwc(noisy[b0:b1].contiguous(), CIN_PAD)
                stash = Stash()
                if batched:        # the group is the batch: a timestep per row, 3-D state, every row differentiated
                    self.injector.begin(state16, g, dstate)
                    eps_all, _ = net.forward(x32, [int(t) for t in timesteps], B, h, stash, want_taps=False, want_eps=True, diff_from=0)
                else:              # one sample: its timestep, its 2-D state, its eps rows into the batch buffer
                    self.injector.begin(state16[b0], g, dstate[b0])
                    eps, _ = net.forward(x32, int(timesteps[b0]), 1, h, stash, want_taps=False, want_eps=True)
                    ops.batch_copy(eps, hw, eps_all[b0 * hw:], hw, 1, hw)
                kept.append((stash, self.injector.stash, net.ctx))
            loss, seed = mse_seed(eps_all, noise, B, h, loss_scale)
        finally:
            self.injector.end()
            net.inject = prev
        return dict(loss=loss, seed=seed, kept=kept, g=g, dstate=dstate, state16=state16, hw=hw)

    @torch.no_grad()
    def backward_batch(self, net, fw: dict, batched: bool = False):
        """HipUNet.backward_eps of every row group of forward_batch (same `batched`: the samples one by one, or all rows at once) into
        the flat gradient vector.  -> (loss, g, d sketch_state)."""
        g, dstate, kept, hw = fw["g"], fw["dstate"], fw["kept"], fw["hw"]
        groups = row_groups(len(fw["dstate"]), batched)
        assert len(groups) == len(kept), "backward_batch: the `batched` of the forward_batch that made fw"
        prev, prev_ctx = net.inject, net.ctx
        net.inject = self.injector
        try:
            for i, (b0, b1) in enumerate(groups):
                (stash, istash, ctx), kept[i] = kept[i], None
                net.ctx = ctx                                      # (the cross-attention K / V of this group's prompts)
                if batched:
                    self.injector.begin(fw["state16"], g, dstate)
                else:
                    self.injector.begin(fw["state16"][b0], g, dstate[b0])
                self.injector.stash = istash
                net.backward_eps(stash, fw["seed"][b0 * hw:b1 * hw], inject_bwd=self.injector.backward)
        finally:
            self.injector.end()
            net.inject, net.ctx = prev, prev_ctx
        return fw["loss"], g, dstate


@torch.no_grad()
def loss_and_grads_through_tower(trainer: HipSatTrainer, tower, net, latents, noise, timesteps, ehs, pixel_values, alphas_cumprod,
                                 batched: bool = False, loss_scale: float = LOSS_SCALE):
    """HipSatTrainer.loss_and_grads fed by the tower's stashing forward, then the tower's backward from d sketch_state.
    -> (loss, SatMixin flat gradient x LOSS_SCALE, tower flat gradient x LOSS_SCALE x tower.seam_scale, d sketch_state x LOSS_SCALE);
    loss_scale (a power of two) takes LOSS_SCALE's place in all three."""
    assert pixel_values is not None, "training through the tower needs pixel_values"
    tokens, kept = tower.forward_train(pixel_values)
    loss, g, dstate = trainer.loss_and_grads(net, latents, noise, timesteps, ehs, tokens, alphas_cumprod, loss_scale=loss_scale,
                                             batched=batched)
    gt = tower.new_grad()
    tower.backward(kept, tower.seam(dstate), gt)
    return loss, g, gt, dstate


@torch.no_grad()
def train_step(trainer: HipSatTrainer, net, latents: torch.Tensor, ehs: torch.Tensor, sketch_state: Optional[torch.Tensor],
               timesteps: Sequence[int], noise: torch.Tensor, alphas_cumprod: torch.Tensor, tower=None,
               pixel_values: Optional[torch.Tensor] = None, batched: bool = False, scaler=None):
    """clip_guided_trainer.py:203-236 for one batch: noise the latents, UNet forward / backward per sample, gradient all-reduce
    across ranks, AdamW.  Returns (loss (0-dim tensor), whether the optimizer stepped, d loss / d sketch_state x LOSS_SCALE).

    tower (a clip_vision_train.HipClipTowerTrainer) + pixel_values [B, 3, S, S]: the sketch tokens come from the tower's stashing
    forward (sketch_state is ignored: pass None), d sketch_state goes into the tower's backward, and the two optimizers step
    together or not at all.

    batched: the UNet evaluates the whole batch in one walk (HipSatTrainer.loss_and_grads); everything else is unchanged.

    scaler (a loss_scaler.DynamicLossScaler): the reference's GradScaler in place of the static LOSS_SCALE.  The backward is seeded
    with scaler.scale (reading it resolves the previous step's verdict); after the all-reduce scaler.check(g[, gt]) queues the
    finiteness test of both flat gradients into the scaler's one device flag, and the guarded AdamW steps of both optimizers read that
    flag: both step or neither, and the host waits for nothing.  The second return value is then the verdict object in place of the
    bool - bool(verdict) resolves it - and d sketch_state carries scaler.scale (the tower's gradient scaler.scale x its seam scale,
    which stays a fixed ratio).  The ranks agree without a collective of their own: the verdict is taken after the all-reduce,
    where a non-finite value in any rank's addend has made the sum non-finite on every rank."""
    s = LOSS_SCALE if scaler is None else scaler.scale         # (reading it resolves the previous step's verdict)
    if tower is None:
        loss, g, dstate = trainer.loss_and_grads(net, latents, noise, timesteps, ehs, sketch_state, alphas_cumprod, loss_scale=s,
                                                 batched=batched)
        steps = [(trainer, g, s)]                              # (optimizer, its flat gradient, the scale that gradient carries)
    else:
        loss, g, gt, dstate = loss_and_grads_through_tower(trainer, tower, net, latents, noise, timesteps, ehs, pixel_values,
                                                           alphas_cumprod, batched=batched, loss_scale=s)
        steps = [(trainer, g, s), (tower, gt, s * tower.seam_scale)]
    for opt, grad, _ in steps:
        opt.all_reduce(grad)
    if scaler is not None:
        verdict = scaler.check(*(grad for _, grad, _ in steps))
        for opt, grad, scale in steps:
            opt.step(grad, scaler=scaler, scale=scale)
        return loss, verdict, dstate
    # one GradScaler in the reference: a non-finite gradient in either set skips both.  The verdict is taken here, once per vector
    # (the tower's is ~3e8 floats; the second is not read when the first has failed), and handed down
    stepped = all(bool(torch.isfinite(grad).all()) for _, grad, _ in steps)
    if stepped:
        for opt, grad, _ in steps:
            opt.step(grad, checked=True)
    return loss, stepped, dstate
