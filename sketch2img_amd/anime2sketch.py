"""Sketch generator: the reference's anime2sketch U-Net (anime2sketch/model.py) on the HIP kernels - picture -> sketch -> latent.

``create_model()`` -> ``generate_sketch(net, img)`` -> ``vae.encode(.) * 0.18215`` is where every training target of the
reference's LGP trainer comes from (trainer.py:36-44,115,220), and ``anime2sketch/generate.py`` is the stand-alone tool.

Dataflow (the reference's activations are in-place, so every ``dk`` is read twice: LeakyReLU by the next down convolution, ReLU by
the skip; IN = InstanceNorm2d(affine=False), eps 1e-5)::

    d1 = Conv4x4s2(x)                              3 -> 64     a2s_patch + ONE K = 64 GEMM
    dk = IN(Conv4x4s2(LeakyReLU(d(k-1))))          k = 2..7    skg_conv4x4s2_f16, skg_instnorm_act_f16
    d8 =    Conv4x4s2(LeakyReLU(d7))
    u8 = IN(ConvT4x4s2(ReLU(d8)))                              skg_convt4x4s2_f16
    uk = IN(ConvT4x4s2(ReLU([dk | u(k+1)])))       k = 7..2    the concatenation is a buffer whose halves the norm kernels write
    y  = tanh(ConvT4x4s2(ReLU([d1 | u2])))         128 -> 1

There is no PyTorch compute path: the two bicubic resizes of ``generate_sketch`` are the only torch arithmetic (host plumbing).
"""
from __future__ import annotations

from typing import Dict, Optional

import torch
import torch.nn as nn
from torch.nn.functional import interpolate

from . import ops, synthetic

CH = synthetic.A2S_DOWN                  # channels of the picture and of d1 .. d8
# Pictures per pass through the kernels.  The contract is that a batch equals its pictures run one by one BIT FOR BIT (the reference:
# exactly 0 on the CPU); the GEMM launcher picks its tile and its split-K factor from M = rows * pixels, and with them the order of
# summation, so a pass takes one picture.  Statistics are per picture anyway, and the levels that under-fill the chip (4 x 4 ... 32 x 32)
# are bound by their 8 - 17 MB of weights, not by M.
PICTURES_PER_PASS = 1
LATENT_SCALE = 0.18215


def check_size(H: int, W: int):
    """Eight halvings and an InstanceNorm over more than one value below them: sides are multiples of 256, 256 ... 1024."""
    if H % 256 or W % 256 or not (256 <= H <= 1024 and 256 <= W <= 1024):
        raise ValueError(f"sketch generator: picture sides must be multiples of 256 in 256 ... 1024, got {H} x {W}")


def _h(t: torch.Tensor, dev) -> torch.Tensor:
    return t.detach().to(torch.float16).contiguous().to(dev)


def pack_conv_first(w: torch.Tensor, dev=None) -> torch.Tensor:
    """Conv2d(3, Cout, 4, 2, 1) weight [Cout, 3, 4, 4] -> [Cout, 64]: column (ky*4 + kx)*3 + c, columns 48..63 zero - the
    B operand of the GEMM over ops.a2s_patch's window matrix."""
    co = w.shape[0]
    p = torch.zeros(co, 64, dtype=torch.float32)
    p[:, :48] = w.detach().float().permute(0, 2, 3, 1).reshape(co, 48)
    return _h(p, dev)


def pack_conv_down(w: torch.Tensor, dev=None) -> torch.Tensor:
    """Conv2d(Cin, Cout, 4, 2, 1) weight [Cout, Cin, 4, 4] -> [Cout, 16 taps ky*4+kx, Cin] as [Cout, 16*Cin] (ops.conv4x4s2)."""
    co, ci = w.shape[:2]
    return _h(w.detach().float().permute(0, 2, 3, 1).reshape(co, 16 * ci), dev)


# filter rows (columns) that land on the two low-res rows (columns) of a phase: a = 0 reads {i-1, i}, a = 1 reads {i, i+1}
CONVT_TAPS = ((3, 1), (2, 0))


def pack_convt(w: torch.Tensor, dev=None, cout_pad: int = 0) -> torch.Tensor:
    """ConvTranspose2d(Cin, Cout, 4, 2, 1) weight [Cin, Cout, 4, 4] -> [4 phases 2a+b, Cout, 4 taps, Cin] as [4, Cout, 4*Cin]
    (ops.convt4x4s2); output channels zero-padded to ``cout_pad``."""
    w = w.detach().float()
    ci, co = w.shape[:2]
    phases = []
    for a in (0, 1):
        for b in (0, 1):
            taps = [w[:, :, ky, kx].t() for ky in CONVT_TAPS[a] for kx in CONVT_TAPS[b]]      # 4 x [co, ci]
            phases.append(torch.stack(taps, 1).reshape(co, 4 * ci))
    p = torch.zeros(4, max(co, cout_pad), 4 * ci)
    p[:, :co] = torch.stack(phases, 0)
    return _h(p, dev)


class HipSketchGenerator:
    """The generator's engine: packed weights on the device, per-size activation buffers with the concatenation halves laid out
    once, forward over ``rows`` pictures.  ``state_dict``: the reference's 32 keys."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], device="cuda"):
        self.dev = torch.device(device)
        shapes = synthetic.anime2sketch_param_shapes()
        sd = {k.replace("module.", ""): v for k, v in state_dict.items()}
        if set(sd) != set(shapes) or any(tuple(sd[k].shape) != s for k, s in shapes.items()):
            raise ValueError("HipSketchGenerator: state_dict is not UnetGenerator(3, 1, 8, 64, InstanceNorm2d)'s")
        keys = list(shapes)
        dn, up = keys[0:16:2], keys[16:32:2][::-1]      # weights of the down / up convolution of level 1 .. 8
        self.Wd = [pack_conv_first(sd[dn[0]], self.dev)] + [pack_conv_down(sd[k], self.dev) for k in dn[1:]]
        self.bd = [_h(sd[k[:-6] + "bias"], self.dev) for k in dn]
        self.Wu = [pack_convt(sd[k], self.dev, cout_pad=8) for k in up]
        self.bu = [_h(sd[k[:-6] + "bias"], self.dev) for k in up]
        self.bu[0] = torch.zeros(8, device=self.dev, dtype=torch.float16)      # the single output channel, padded like its filters
        self.bu[0][:1] = _h(sd[up[0][:-6] + "bias"], self.dev)
        self._buf = {}

    def _buffers(self, rows: int, H: int, W: int):
        key = (rows, H, W, torch.cuda.current_stream().cuda_stream)
        if key not in self._buf:
            e = lambda m, c: torch.empty(m, c, device=self.dev, dtype=torch.float16)
            M = [rows * (H >> k) * (W >> k) for k in range(9)]
            b = {"patch": e(M[1], 64), "y": e(M[0], 8), "r8": e(M[8], CH[8])}
            for k in range(1, 9):
                b[f"raw{k}"] = e(M[k], CH[k])                       # convolution output of level k (before the norm)
            for k in range(1, 8):
                b[f"act{k}"] = e(M[k], CH[k])                       # LeakyReLU(dk): operand of the next down convolution
                b[f"cat{k}"] = e(M[k], 2 * CH[k])                   # ReLU([dk | u(k+1)]): operand of the up convolution of level k
                b[f"up{k}"] = e(M[k], CH[k])                        # transposed-convolution output u(k+1) (before the norm)
            self._buf = {key: b}                                    # (one size at a time: a 1024 x 1024 set is ~0.4 GB per picture)
        return self._buf[key]

    @torch.no_grad()
    def tokens(self, img: torch.Tensor) -> torch.Tensor:
        """img float [rows, 3, H, W] -> fp16 [rows*H*W, 8], column 0 = y (the buffer is reused by the next call)."""
        rows, _, H, W = img.shape
        b = self._buffers(rows, H, W)
        sz = [(H >> k, W >> k) for k in range(9)]
        hw = [h * w for h, w in sz]
        ops.a2s_patch(img, out=b["patch"])
        ops.gemm(b["patch"], self.Wd[0], out=b["raw1"], bias=self.bd[0])
        ops.instnorm_act(b["raw1"], rows, hw[1], b["act1"], 0.2, b["cat1"][:, :CH[1]], 0.0, identity=True)
        for k in range(2, 9):
            ops.conv4x4s2(b[f"act{k - 1}"], self.Wd[k - 1], rows, *sz[k - 1], out=b[f"raw{k}"], bias=self.bd[k - 1])
            if k < 8:
                ops.instnorm_act(b[f"raw{k}"], rows, hw[k], b[f"act{k}"], 0.2, b[f"cat{k}"][:, :CH[k]], 0.0)
        ops.instnorm_act(b["raw8"], rows, hw[8], None, 1.0, b["r8"], 0.0, identity=True)
        x = b["r8"]
        for k in range(8, 1, -1):      # the up convolution of level k writes u(k) at the size of level k - 1
            ops.convt4x4s2(x, self.Wu[k - 1], rows, *sz[k], out=b[f"up{k - 1}"], bias=self.bu[k - 1])
            ops.instnorm_act(b[f"up{k - 1}"], rows, hw[k - 1], None, 1.0, b[f"cat{k - 1}"][:, CH[k - 1]:], 0.0)
            x = b[f"cat{k - 1}"]
        return ops.convt4x4s2(x, self.Wu[0], rows, *sz[1], out=b["y"], bias=self.bu[0], tanh=True)

    def forward(self, img: torch.Tensor, want_y: bool = True, want_mask: bool = False):
        """img float [B, 3, H, W] in [-1, 1] -> (y float [B, 1, H, W] or None, mask float [B, 3, H, W] or None); statistics are
        per picture, so a batch equals its pictures run one by one."""
        if img.dim() != 4 or img.shape[1] != 3:
            raise ValueError(f"sketch generator: [B, 3, H, W] pictures expected, got {tuple(img.shape)}")
        check_size(*img.shape[2:])
        if not img.is_cuda:
            raise RuntimeError("sketch2img_amd has no CPU path: move the picture to the GPU")
        img = img.to(self.dev, torch.float32).contiguous()
        B, _, H, W = img.shape
        y = torch.empty(B, 1, H, W, device=self.dev, dtype=torch.float32) if want_y else None
        m = torch.empty(B, 3, H, W, device=self.dev, dtype=torch.float32) if want_mask else None
        for s0 in range(0, B, PICTURES_PER_PASS):
            s1 = min(B, s0 + PICTURES_PER_PASS)
            ops.a2s_tail(self.tokens(img[s0:s1]), s1 - s0, H, W, y=y[s0:s1] if want_y else None, mask=m[s0:s1] if want_mask else None)
        return y, m


class _Slots(nn.Module):
    """``.model`` = a Sequential whose parameter-carrying entries sit where the reference block has them (state_dict keys only;
    nothing is ever run through it)."""

    def __init__(self, entries):
        super().__init__()
        self.model = nn.Sequential(*entries)


class _Holder(nn.Module):
    def __init__(self, wshape, bshape):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(wshape))
        self.bias = nn.Parameter(torch.zeros(bshape))


def _skeleton() -> nn.Module:
    """Module tree with exactly the reference's 32 state_dict keys, built from synthetic.anime2sketch_param_shapes()."""
    shapes = synthetic.anime2sketch_param_shapes()
    keys = list(shapes)
    dn, up = keys[0:16:2], keys[16:32:2][::-1]
    hold = lambda k: _Holder(shapes[k], shapes[k[:-6] + "bias"])
    block = _Slots([nn.Identity(), hold(dn[7]), nn.Identity(), hold(up[7]), nn.Identity()])                      # innermost
    for k in range(6, 0, -1):
        block = _Slots([nn.Identity(), hold(dn[k]), nn.Identity(), block, nn.Identity(), hold(up[k]), nn.Identity()])
    return _Slots([hold(dn[0]), block, nn.Identity(), hold(up[0]), nn.Identity()])                                # outermost


class UnetGenerator(nn.Module):
    """Drop-in for anime2sketch/model.py's UnetGenerator in the one configuration ``create_model`` builds - (3, 1, num_downs 8,
    ngf 64, InstanceNorm2d(affine=False, track_running_stats=False), no dropout).  Same 32 state_dict keys, ``load_state_dict``,
    ``.eval()``, ``.to()``; ``__call__(img)``: float NCHW in [-1, 1] on the GPU -> [B, 1, H, W] float32, on the HIP kernels."""

    def __init__(self, input_nc=3, output_nc=1, num_downs=8, ngf=64, norm_layer=None, use_dropout=False):
        super().__init__()
        fn = getattr(norm_layer, "func", norm_layer)
        kw = dict(getattr(norm_layer, "keywords", None) or {})
        if (input_nc, output_nc, num_downs, ngf) != (3, 1, 8, 64) or use_dropout or fn not in (None, nn.InstanceNorm2d) or \
                kw.get("affine", False) or kw.get("track_running_stats", False):
            raise NotImplementedError("UnetGenerator: only create_model()'s configuration is built - (3, 1, 8, 64), "
                                      "InstanceNorm2d(affine=False, track_running_stats=False), no dropout")
        self.model = _skeleton()
        with torch.no_grad():
            for k, v in synthetic.anime2sketch_state_dict().items():      # seeded stand-in weights until load_state_dict()
                self.state_dict()[k].copy_(v)
        self._hip: Optional[HipSketchGenerator] = None
        self._hip_key = None

    def _engine(self, device) -> HipSketchGenerator:
        ps = list(self.parameters())
        key = (str(device), tuple((int(t._version), t.data_ptr()) for t in ps))
        if self._hip is None or self._hip_key != key:
            self._hip = HipSketchGenerator(self.state_dict(), device)
            self._hip_key = key
        return self._hip

    def _run(self, img, want_y, want_mask):
        if img.dim() == 4:
            check_size(*img.shape[2:])
        if not img.is_cuda:
            raise RuntimeError("sketch2img_amd has no CPU path: move the picture to the GPU")
        return self._engine(img.device).forward(img.float(), want_y, want_mask)

    def forward(self, input):
        return self._run(input, True, False)[0]

    def sketch_mask(self, img):
        """(1 - net(img)) binarised at 0.5 and tiled to three channels (trainer.py:39-42), in the generator's tail kernel."""
        return self._run(img, False, True)[1]


def create_model(path: str = "weights/netG.pth") -> UnetGenerator:
    """anime2sketch/model.py:104-116: the generator with the checkpoint at ``path`` (a local file; nothing is downloaded);
    a ``module.`` prefix (DataParallel checkpoints) is stripped."""
    net = UnetGenerator(3, 1, 8, 64)
    ckpt = torch.load(path, map_location="cpu")
    net.load_state_dict({k.replace("module.", ""): v for k, v in ckpt.items()})
    return net


def _resize(img: torch.Tensor, size) -> torch.Tensor:
    if tuple(img.shape[-2:]) == tuple(size):
        return img
    return interpolate(img, size=tuple(size), mode="bicubic", align_corners=False, antialias=True)


def generate_sketch(sketch_generator, img: torch.Tensor, fixed=1024) -> torch.Tensor:
    """trainer.py:36-44: resize to ``fixed`` x ``fixed`` (bicubic) -> 1 - generator -> binarise at 0.5 -> three channels ->
    resize back.  img float [B, 3, H, W] in [-1, 1] on the GPU; returns float [B, 3, H, W]."""
    size = (fixed, fixed) if isinstance(fixed, int) else tuple(fixed)
    check_size(*size)
    if not hasattr(sketch_generator, "sketch_mask"):
        raise TypeError("generate_sketch: a sketch2img_amd UnetGenerator expected (create_model())")
    return _resize(sketch_generator.sketch_mask(_resize(img.float(), size)), img.shape[-2:])


def sketch_latents(img: torch.Tensor, sketch_generator, vae, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """trainer.py:220: the LGP training target / the pipeline's ``sketch_image`` of a picture."""
    return vae.encode(generate_sketch(sketch_generator, img)).latent_dist.sample(generator) * LATENT_SCALE
