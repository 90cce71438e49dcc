"""Exact-integer probes for the matrix-pipe kernels (GEMM, the 3x3 convolution family, Winograd, the weight gradient).

With small-integer operands every product and every partial sum of a contraction is an integer below 2^24, so fp32 accumulation is
exact in ANY order: on every tile shape, split-K slicing and LDS ring depth the accumulator holds the same integer.  The correct
output is then a known bit pattern and the tolerance is zero.

Two amplitude classes (``draw`` below):
  small  x in [-3, 3], w in [-1, 1] (Winograd: 4 * [-1, 1]), bias in [-8, 8], residual in [-64, 64].  Every named intermediate and
         the result are fp16 numbers: the class tests STRUCTURE (indexing, halos, sample seams, tile edges, K slices, row maps).
  large  x in [-31, 31], w in [-a_w, a_w] with a_w from the K of the case (``large_amp_w``), residual in [-4096, 4096].  v is an
         exact fp32 integer that fp16 cannot hold, the expected output is RNE_fp16(v): the class tests that the epilogue rounds
         exactly ONCE (a stage that rounds before the residual is added changes many elements).  Pair outputs: hi = fp16(v),
         lo = fp16(v - hi).
  gn     x in {-1, 0, 1}, w in {-1, 0, 1} at density 1/8: the small class with outputs so small that the GroupNorm partial sums
         (sum y, sum y^2 per sample, 128-row chunk and group) are exact integers below 2^24 as well.

References are plain torch on the CPU over all samples - fp64, or fp32 where the order-free condition makes fp32 exact too - and never
call a libskg kernel.  The conditions that make the expected bits unambiguous are asserted ON THE REFERENCE, before any comparison
(``check_*``); a failed condition is a failed test, never a skip and never a mask.

This module imports without a GPU; the ``run_*`` functions at the end are the device side, shared by
tests/test_gpu_exact_contractions.py and tests/_exact_tile_check.py.
"""
from __future__ import annotations

import dataclasses
import functools
from dataclasses import dataclass
from typing import Optional, Tuple

import torch
import torch.nn.functional as F

TWO24 = float(1 << 24)
FP16_MAX = 65504.0
GUARD = 7.0                     # what guard columns / rows of strided outputs are filled with beforehand
AMP = {"small": dict(x=3, bias=8, res=64), "large": dict(x=31, bias=8, res=4096), "gn": dict(x=1, bias=8, res=64)}
RES_STEP = {"small": 1, "large": 2, "gn": 1}      # (fp16 holds every integer up to 2048 only: the large residuals are the even ones)
FP64_REF_MACS = 3e9             # references above this many multiply-adds are formed in fp32 (exact under the order-free bound)


# ------------------------------------------------------------------------------------------------------------------ draws
def draw_int(shape, amp: int, seed: int, density: float = 1.0, step: int = 1) -> torch.Tensor:
    """Integers in [-amp, amp] * step as fp16; `density` zeroes entries at random.  One fixed seed per call, no re-draw, no filter."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(-amp, amp + 1, tuple(shape), generator=g, dtype=torch.int32)
    if density < 1.0:
        v = v * (torch.rand(tuple(shape), generator=g) < density).to(torch.int32)
    out = (v * step).to(torch.float16)
    assert torch.equal(out.to(torch.int32), v * step)
    return out


def large_amp_w(K: int) -> int:
    """Weight amplitude of the large class: K * 31 * a_w < 2^24 with room, and |v| (about 5.5 sigma of a sum of K products of
    two uniform integers, sigma = sqrt(K) * 17.9 * 0.6 a_w) below 60000: 15 at K = 576, 7 at K = 1152, 1 from K = 8640."""
    return max(1, min(15, 8640 // K))


def amp_w(cls: str, K: int) -> int:
    return large_amp_w(K) if cls == "large" else 1


def seed_of(name: str, cls: str, what: int) -> int:
    """One fixed seed per (case, class, tensor): a stable hash of the case name (Python's hash() is salted per process)."""
    h = 0
    for ch in f"{name}/{cls}":
        h = (h * 131 + ord(ch)) % 1000003
    return h * 16 + what


# ------------------------------------------------------------------------------------------------------------- conditions
def check_order_free(absA: torch.Tensor, absB: torch.Tensor, extra: float = 0.0) -> float:
    """|A| . |B|^T + |bias| + |residual| < 2^24 per output element (absA [M, K], absB [N, K], fp64): every partial sum of the
    contraction, in any order, is an integer that fp32 holds.  Returns the largest bound."""
    bound = float((absA.double() @ absB.double().t()).max()) + extra
    assert bound < TWO24, f"order-free exactness violated: sum of |products| reaches {bound:.0f} >= 2^24"
    return bound


def check_worst_case(K: int, amp_x: int, amp_w_: int, extra: float = 0.0) -> float:
    """The cheaper worst case of check_order_free for the big cases: K * amp_x * amp_w (+ |bias| + |residual|) < 2^24."""
    bound = float(K) * amp_x * amp_w_ + extra
    assert bound < TWO24, f"worst-case bound {bound:.0f} >= 2^24 (K = {K}, |x| <= {amp_x}, |w| <= {amp_w_})"
    return bound


def check_fp16_exact(v: torch.Tensor, what: str = "reference"):
    """small class: the value is an fp16 number everywhere (v fp64 or fp32)."""
    bad = v.half().to(v.dtype) != v
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} values are not fp16 numbers (max |v| = {float(v.abs().max())})"


def check_fp16_range(v: torch.Tensor, what: str = "reference"):
    """large class: RNE_fp16(v) is finite."""
    m = float(v.abs().max())
    assert m < FP16_MAX, f"{what}: max |v| = {m} does not round to a finite fp16 number"


def rne_fp16(v: torch.Tensor) -> torch.Tensor:
    """Round-to-nearest-even of an exact value to fp16 in ONE rounding: v must be an fp32 number (asserted), the fp32 -> fp16
    conversion is then the only rounding."""
    f = v.float()
    assert torch.equal(f.to(v.dtype), v), "the exact value is not an fp32 number: fp32 accumulation could not hold it"
    return f.half()


def gn_sums(y16: torch.Tensor, rows: int, HW: int, groups: int) -> torch.Tensor:
    """fp64 sum(y), sum(y^2) per (sample, 128-row chunk, group) of the fp16 outputs [rows * HW, C] -> [rows, HW / 128, groups, 2];
    asserts that sum |y| and sum y^2 stay below 2^24, so the fp32 sums are exact in any order."""
    C = y16.shape[1]
    y = y16.double().view(rows, HW // 128, 128, groups, C // groups)
    s_abs, s2 = y.abs().sum(dim=(2, 4)), (y * y).sum(dim=(2, 4))
    assert float(s_abs.max()) < TWO24 and float(s2.max()) < TWO24, \
        f"GroupNorm partial sums are not order-free: max sum|y| = {float(s_abs.max()):.0f}, max sum y^2 = {float(s2.max()):.0f}"
    return torch.stack([y.sum(dim=(2, 4)), s2], dim=-1)


# ------------------------------------------------------------------------------------------------------------ comparator
@dataclass(frozen=True)
class Layout:
    """How the rows of an output matrix map to pixels, and the launch structure the report names.  rows samples of OH x OW pixels,
    C valid columns; bn = tile width of the launch (tiles are 128 rows x bn columns); split = (slices, K tiles of 64 per slice)."""
    rows: int
    OH: int
    OW: int
    C: int
    bn: int = 64
    split: Optional[Tuple[int, int]] = None
    name: str = ""

    @staticmethod
    def matrix(M: int, N: int, bn: int = 64, split=None, name: str = "") -> "Layout":
        return Layout(M, 1, 1, N, bn, split, name)


def _bits(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().cpu().contiguous()
    it = {torch.float16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}[t.dtype]
    return torch.where(t == 0, torch.zeros_like(t), t).view(it)      # (-0 and +0 are the same answer)


def assert_bits_equal(got: torch.Tensor, want: torch.Tensor, layout: Layout, show: int = 6):
    """got [M, ld >= C] (the whole strided buffer: columns >= C are guard columns that must still hold GUARD), want [M, C] of the
    same dtype.  Zero mismatching bit patterns or an AssertionError that gives the number of mismatching elements, the first few
    as (sample, y, x, channel) with got / want, their 128-row x bn tile coordinates and the K-slice structure of a split launch."""
    got, want = got.detach().cpu(), want.detach().cpu()
    M, C = want.shape
    assert got.dtype == want.dtype and got.shape[0] == M and got.shape[1] >= C and C == layout.C, \
        f"{layout.name}: got {tuple(got.shape)} {got.dtype}, want {tuple(want.shape)} {want.dtype}, layout C = {layout.C}"
    msgs = []
    if got.shape[1] > C:
        g = got[:, C:]
        bad = g != GUARD
        if bool(bad.any()):
            m, n = (int(v) for v in bad.nonzero()[0])
            msgs.append(f"{int(bad.sum())} guard elements overwritten, first at row {m}, column {C + n}: {float(g[m, n])}")
    bad = _bits(got[:, :C]) != _bits(want)
    nbad = int(bad.sum())
    if nbad:
        hw = layout.OH * layout.OW
        idx = bad.nonzero()
        lines = []
        for m, n in idx[:show].tolist():
            s, p = divmod(m, hw)
            y, x = divmod(p, layout.OW)
            lines.append(f"  (s={s}, y={y}, x={x}, c={n}) got {float(got[m, n])!r} want {float(want[m, n])!r}  "
                         f"tile (row {m // 128}, col {n // layout.bn})")
        tiles = sorted({(m // 128, n // layout.bn) for m, n in idx.tolist()}) if nbad <= 100000 else None
        head = f"{nbad} of {M * C} elements differ"
        if tiles is not None:
            head += f" in {len(tiles)} tile(s) of 128 x {layout.bn}, first {tiles[:4]}"
        if layout.split:
            head += f"; split-K launch: {layout.split[0]} K slices of {layout.split[1]} x 64"
        msgs.append(head + "\n" + "\n".join(lines))
    assert not msgs, f"{layout.name or 'output'}: " + "; ".join(msgs)


# ------------------------------------------------------------------------------------------------------- layout helpers
def nhwc(x: torch.Tensor) -> torch.Tensor:
    """[B, C, H, W] -> [B * H * W, C]"""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


def epilogue(acc: torch.Tensor, bias=None, alpha: float = 1.0, residual=None, relu: bool = False, cls: str = "small",
             residual_lo=None) -> torch.Tensor:
    """v = relu?(alpha * (acc + bias) + residual (+ residual_lo)) in the dtype of acc (exact), with the class conditions on the
    value in front of the residual (the fp16-staged epilogue may legitimately hold it) and on v."""
    v = acc if bias is None else acc + bias.to(acc.dtype)
    v = v * alpha
    if residual is not None or residual_lo is not None:
        if cls != "large":
            check_fp16_exact(v, "alpha * (acc + bias)")
        if residual is not None:
            v = v + residual.to(acc.dtype)
        if residual_lo is not None:
            v = v + residual_lo.to(acc.dtype)
    if relu:
        v = torch.relu(v)
    if cls == "large":
        check_fp16_range(v)
    else:
        check_fp16_exact(v)
    return v


def expected_f16(v: torch.Tensor, cls: str) -> torch.Tensor:
    return rne_fp16(v) if cls == "large" else v.half()


def expected_pair(v: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """hi = fp16(v), lo = fp16(v - hi); v - hi is exact in fp32 and an fp16 number (asserted)."""
    hi = rne_fp16(v)
    d = v - hi.to(v.dtype)
    check_fp16_exact(d, "v - hi")
    return hi, d.half()


# ------------------------------------------------------------------------------------------------------------ references
CONV_MODES = ("S1", "S2", "UP2", "S2T", "S2A")
MODE_ID = {"S1": 0, "S2": 1, "UP2": 2, "S2T": 3, "S2A": 4}


def out_size(mode: str, IH: int, IW: int) -> Tuple[int, int]:
    if mode in ("UP2", "S2T"):
        return 2 * IH, 2 * IW
    if mode in ("S2", "S2A"):
        return IH // 2, IW // 2
    return IH, IW


def conv_ref(x: torch.Tensor, w: torch.Tensor, mode: str, dgrad: bool = False, pad_mode: str = "zeros") -> torch.Tensor:
    """Plain torch reference, x [B, Cin, IH, IW] and w in torch's layout, same floating dtype.
    forward (dgrad False): w [Cout, Cin, 3, 3].  S1 / S2 / S2A / UP2 as include/skg.h defines the gather modes.
    dgrad: w [Cin, Cout, 3, 3] is the FORWARD weight of the convolution whose data gradient is taken (x is its output gradient):
    S1 -> the gradient of a stride-1 convolution, S2T -> of a stride-2 one.
    pad_mode 'replicate' (S1 / UP2 forward only): the mutant of the edge-sensitivity check."""
    if dgrad:
        if mode == "S1":
            return F.conv_transpose2d(x, w, stride=1, padding=1)
        assert mode == "S2T"
        return F.conv_transpose2d(x, w, stride=2, padding=1, output_padding=1)
    if mode == "UP2":
        x = F.interpolate(x, scale_factor=2.0, mode="nearest")
    if mode in ("S1", "UP2"):
        if pad_mode == "replicate":
            return F.conv2d(F.pad(x, (1, 1, 1, 1), mode="replicate"), w)
        return F.conv2d(x, w, padding=1)
    if mode == "S2":
        return F.conv2d(x, w, stride=2, padding=1)
    if mode == "S2A":
        return F.conv2d(F.pad(x, (0, 1, 0, 1)), w, stride=2)
    raise ValueError(mode)


def ref_dtype(macs: float) -> torch.dtype:
    return torch.float64 if macs <= FP64_REF_MACS else torch.float32


def wino_emulate(x16: torch.Tensor, U16: torch.Tensor) -> torch.Tensor:
    """fp32 emulation of skg_conv3x3_wino_f16 without bias: x16 [B, Cin, H, W] fp16 (even H, W), U16 [Cout, 16 * Cin] fp16 from
    pack_conv_wino -> [B, Cout, H, W] fp32.  V = B^T d B per 4 x 4 input tile (stride 2) rounded to fp16, 16 fp32 GEMMs
    V_c . U_c^T, Y = A^T M A.  Also asserts the order-free condition on |V| . |U|^T summed through |A^T| . |A|."""
    Bn, Ci, H, W = x16.shape
    Co = U16.shape[0]
    xp = F.pad(x16.float(), (1, 1, 1, 1))
    t = xp.unfold(2, 4, 2).unfold(3, 4, 2)                                   # [B, Ci, H/2, W/2, 4, 4]
    Bt = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float32)
    V = torch.einsum("ij,bcyxjk,lk->byxilc", Bt, t, Bt)                     # [B, H/2, W/2, 4, 4, Ci]
    V16 = V.half()
    assert torch.equal(V16.float(), V), "V = B^T d B is not held exactly by fp16"
    Vm = V16.float().reshape(-1, 16, Ci)
    U = U16.float().view(Co, 16, Ci)
    Mc = torch.einsum("mck,nck->mcn", Vm, U)                                 # [Mt, 16, Co]
    bound = float(torch.einsum("mck,nck->mn", Vm.abs().double(), U.abs().double()).max())
    assert bound < TWO24, f"Winograd: sum over the 16 components of |V| . |U|^T reaches {bound:.0f} >= 2^24"
    At = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float32)
    Y = torch.einsum("ai,mijn,bj->mabn", At, Mc.view(-1, 4, 4, Co), At)      # [Mt, 2, 2, Co]
    Y = Y.view(Bn, H // 2, W // 2, 2, 2, Co).permute(0, 5, 1, 3, 2, 4).reshape(Bn, Co, H, W)
    return Y


# ----------------------------------------------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class GemmCase:
    """One skg_gemm_f16 probe.  epi: words of bias alpha relu res f32 slice guard pair pairres gn.  variant: what
    skg_gemm_variant must report (2000 + tile width, + 10000 three stages, 1064 / 1128 generic); split = (slices, K tiles per
    slice) of a split-K launch, for the report; gn = (HW, groups, fused?)."""
    M: int
    N: int
    K: int
    variant: int
    epi: str = ""
    split: Optional[Tuple[int, int]] = None
    gn: Optional[Tuple[int, int, int]] = None
    classes: Tuple[str, ...] = ("small", "large")

    @property
    def name(self) -> str:
        return f"gemm {self.M}x{self.N}x{self.K} [{self.epi or 'plain'}]"

    def has(self, word: str) -> bool:
        return word in self.epi.split()


def _gemm_cases():
    c = []
    # the generic BK = 32 kernel (K % 64 != 0), narrow and wide form
    c += [GemmCase(1, 8, 32, 1064), GemmCase(65, 40, 96, 1064, "bias alpha res"), GemmCase(129, 72, 32, 1064, "bias relu"),
          GemmCase(129, 72, 32, 1064, "f32 guard"), GemmCase(32768, 128, 32, 1128, "bias res")]
    # 128 x 64: ragged M and N; K = 64 (one K tile), 192 (two stages), 256 (three stages)
    for K, var in ((64, 2064), (192, 2064), (256, 12064)):
        for i, M in enumerate((1, 127, 129, 300)):
            for N in (64, 72):
                c.append(GemmCase(M, N, K, var, ("", "bias alpha res", "bias res relu")[(i + N // 72 + K // 64) % 3]))
    # the epilogues on the 128 x 64 tile (three stages) and on the 128 x 160 tile (three stages)
    for (M, N, K, var) in ((300, 72, 256, 12064), (12800, 320, 256, 12160)):
        for epi in ("bias", "alpha", "relu", "res", "f32 bias", "slice bias", "guard bias res", "pair bias", "pair pairres bias alpha",
                    "bias alpha res relu"):
            c.append(GemmCase(M, N, K, var, epi))
    c += [GemmCase(16512, 320, 256, 2160, "bias res"),                       # 128 x 160, two stages (more than 256 tiles)
          GemmCase(12800, 256, 128, 2128, "bias res"),                       # 128 x 128
          GemmCase(7680, 2560, 1024, 2320, "bias res"),                      # 256 x 320 (gemm2), streaming stores (>= 32 MiB)
          GemmCase(7679, 2560, 1024, 2320, "bias alpha"),                    # ... ragged rows
          GemmCase(16384, 1024, 64, 2128, "bias"),                           # streaming stores on a 128-row tile
          GemmCase(256, 512, 128, 2064, "bias res"),                         # XCD re-arrangement (16 tiles, 8 column tiles)
          GemmCase(200, 64, 1024, 2064, "bias alpha res", split=(2, 8)),     # split-K, 128 x 64
          GemmCase(200, 64, 1024, 2064, "pair pairres bias", split=(2, 8)),
          GemmCase(1536, 320, 2048, 12160, "bias res", split=(4, 8)),        # split-K on the deep ring
          GemmCase(1536, 320, 2368, 12160, "bias alpha res relu", split=(4, 10)),      # ... ragged last slice (10, 10, 10, 7)
          GemmCase(1536, 320, 2368, 12160, "pair bias", split=(4, 10)),
          # GroupNorm partial sums: from the epilogue of the 128 x 160 tile (whole tiles, HW = 128 k), and the stand-alone pass
          GemmCase(12800, 320, 256, 12160, "gn bias", gn=(6400, 32, 1), classes=("gn",)),
          GemmCase(12800, 320, 256, 12160, "gn bias res", gn=(1280, 32, 1), classes=("gn",)),
          GemmCase(16512, 320, 256, 2160, "gn bias", gn=(128, 32, 1), classes=("gn",)),
          GemmCase(256, 64, 64, 2064, "gn bias", gn=(128, 8, 0), classes=("gn",)),
          GemmCase(768, 320, 128, 2064, "gn bias res", gn=(384, 32, 0), classes=("gn",))]
    return tuple(c)


GEMM_CASES = _gemm_cases()


def bn_of(variant: int) -> int:
    return variant % 1000


@dataclass(frozen=True)
class ConvCase:
    """One skg_conv3x3_f16 probe: rows samples of IH x IW, Cin -> Cout, gather mode; epi words as GemmCase plus biasrows (a bias
    row per sample) and dgrad (the flipped, in / out-swapped pack: the data gradient of a convolution Cout -> Cin).
    pad = (cin_real, cout_real): conv_in / conv_out channel padding.  variant None: only the family (LDS-DMA vs generic) is
    asserted from Cin."""
    rows: int
    IH: int
    IW: int
    Cin: int
    Cout: int
    mode: str = "S1"
    epi: str = ""
    variant: Optional[int] = None
    split: Optional[Tuple[int, int]] = None
    gn: Optional[Tuple[int, int]] = None             # (groups, fused?)
    pad: Optional[Tuple[int, int]] = None
    classes: Tuple[str, ...] = ("small", "large")

    @property
    def name(self) -> str:
        return f"conv {self.mode} rows{self.rows} {self.IH}x{self.IW} {self.Cin}->{self.Cout} [{self.epi or 'plain'}]"

    def has(self, word: str) -> bool:
        return word in self.epi.split()

    @property
    def K(self) -> int:
        return 9 * self.Cin


def _conv_cases():
    c = []
    epis = ("", "bias", "bias res", "bias alpha res relu", "biasrows")
    maps = {"S1": (3, 6, 10), "S2": (3, 12, 20), "S2A": (3, 12, 20), "UP2": (3, 6, 10), "S2T": (3, 6, 10)}
    i = 0
    for mode in CONV_MODES:
        rows, IH, IW = maps[mode]
        for Cin in (32, 64, 128):
            for Cout in (8, 40, 64, 160, 320):
                c.append(ConvCase(rows, IH, IW, Cin, Cout, mode, ("dgrad " if mode == "S2T" else "") + epis[i % len(epis)]))
                i += 1
    # S1 on odd and tiny maps, samples that share tiles, rows * OH * OW = 128 k +- 1
    for (rows, IH, IW) in ((3, 1, 1), (5, 2, 2), (3, 5, 7), (3, 12, 20), (11, 5, 7), (3, 1, 43), (127, 1, 1)):
        c += [ConvCase(rows, IH, IW, 64, 160, "S1", "bias res"), ConvCase(rows, IH, IW, 32, 40, "S1", "bias")]
    c += [ConvCase(3, 6, 10, 64, 64, "S1", "dgrad bias"), ConvCase(3, 6, 10, 128, 320, "S1", "dgrad"),
          ConvCase(3, 6, 10, 160, 64, "S2T", "dgrad bias"),
          # conv_in (4 latent channels padded to one K tile) and conv_out (4 output channels padded to the 8-channel store)
          ConvCase(3, 6, 10, 64, 320, "S1", "bias", pad=(4, 320)), ConvCase(3, 6, 10, 320, 8, "S1", "bias", pad=(320, 4)),
          # a bias row per sample: tiles inside a sample (HW % 128 == 0), tiles that span samples, fp32 output, pair output
          ConvCase(3, 8, 16, 64, 160, "S1", "biasrows res"), ConvCase(3, 8, 16, 64, 320, "S1", "biasrows f32"),
          ConvCase(3, 8, 16, 64, 160, "S1", "biasrows pair"), ConvCase(3, 6, 10, 64, 160, "S1", "biasrows pair pairres"),
          ConvCase(3, 6, 10, 64, 160, "S1", "biasrows f32"), ConvCase(3, 12, 20, 64, 160, "S2", "biasrows res"),
          ConvCase(3, 6, 10, 64, 160, "UP2", "biasrows pair"), ConvCase(3, 6, 10, 64, 72, "S1", "pair bias"),
          ConvCase(3, 6, 10, 64, 72, "S1", "guard bias res"), ConvCase(3, 12, 20, 64, 160, "S2", "pair pairres bias"),
          # split-K on the deep ring: K = 2304 over four slices of nine K tiles
          ConvCase(6, 16, 16, 256, 320, "S1", "bias res", variant=12160, split=(4, 9)),
          ConvCase(6, 16, 16, 256, 320, "S1", "biasrows pair pairres", variant=12160, split=(4, 9)),
          # GroupNorm partial sums on the 128-row tiles (the 256 x 320 tile: BIG_CONV below)
          ConvCase(2, 16, 16, 64, 320, "S1", "gn bias", gn=(32, 0), classes=("gn",))]
    return tuple(c)


CONV_CASES = _conv_cases()

# the 256 x 320 ping-pong tile (variant 8320) at the 64 x 64 level: (rows, H), whole tiles and ragged
BIG_CONV = ((14, 64), (15, 62))
BIG_CIN, BIG_COUT, BIG_GROUPS = 128, 320, 32
BIG_VARIANTS = ("bias", "bias res", "pair pairres bias", "biasrows", "gn bias")


def conv_operands(case: ConvCase, cls: str):
    """-> (x [B, Cin, IH, IW] fp16, w fp16 in torch layout for conv_ref).  Padded channels are zero."""
    A = AMP[cls]
    dens = 0.125 if cls == "gn" else 1.0
    x = draw_int((case.rows, case.Cin, case.IH, case.IW), A["x"], seed_of(case.name, cls, 0))
    shape = (case.Cin, case.Cout, 3, 3) if case.has("dgrad") else (case.Cout, case.Cin, 3, 3)
    w = draw_int(shape, amp_w(cls, case.K), seed_of(case.name, cls, 1), density=dens)
    if case.pad:
        ci, co = case.pad
        x[:, ci:] = 0
        w[co:] = 0
        w[:, ci:] = 0
    return x, w


def epi_operands(name: str, cls: str, words, M: int, N: int, rows: int = 0):
    """bias / residual / pair residual / alpha of a case from the words of its epilogue string."""
    A = AMP[cls]
    bias = None
    if "biasrows" in words:
        bias = draw_int((rows, N), A["bias"], seed_of(name, cls, 2))
    elif "bias" in words:
        bias = draw_int((N,), A["bias"], seed_of(name, cls, 2))
    res = draw_int((M, N), A["res"] // RES_STEP[cls], seed_of(name, cls, 3), step=RES_STEP[cls]) if ("res" in words or "pairres" in words) else None
    res_lo = draw_int((M, N), 2, seed_of(name, cls, 4)) if "pairres" in words else None
    return bias, res, res_lo, (0.5 if "alpha" in words else 1.0)


@functools.lru_cache(maxsize=4)
def big_conv_ref(rows: int, H: int, cls: str):
    """One reference per (x, w) draw of the 256 x 320-tile cases: -> (x16, w16, acc fp32 [rows * H * H, Cout]); bias and residual are
    added per variant.  fp32 is exact here: the worst-case bound is asserted."""
    name = f"bigconv rows{rows} {H}x{H}"
    x = draw_int((rows, BIG_CIN, H, H), AMP[cls]["x"], seed_of(name, cls, 0))
    aw = amp_w(cls, 9 * BIG_CIN)
    w = draw_int((BIG_COUT, BIG_CIN, 3, 3), aw, seed_of(name, cls, 1), density=0.125 if cls == "gn" else 1.0)
    check_worst_case(9 * BIG_CIN, AMP[cls]["x"], aw, AMP[cls]["bias"] + AMP[cls]["res"] + 2)
    acc = nhwc(F.conv2d(x.float(), w.float(), padding=1))
    return x, w, acc


def big_conv_variants(rows: int, H: int):
    """(variant, class) pairs of the 256 x 320-tile cases: the GroupNorm sums on their own draw, on whole 128-row chunks only."""
    for cls in ("small", "large", "gn"):
        for variant in BIG_VARIANTS:
            if ("gn" in variant.split()) == (cls == "gn") and not (cls == "gn" and (H * H) % 128):
                yield variant, cls


def big_conv_value(rows: int, H: int, variant: str, cls: str):
    """-> (name, bias, residual, residual_lo, v) of one variant on the shared reference (conditions asserted)."""
    name = f"bigconv rows{rows} {H}x{H} [{variant}]"
    acc = big_conv_ref(rows, H, cls)[2]
    bias, res, res_lo, alpha = epi_operands(name, cls, variant.split(), rows * H * H, BIG_COUT, rows)
    b = bias.repeat_interleave(H * H, dim=0) if bias.dim() == 2 else bias
    return name, bias, res, res_lo, epilogue(acc, b, alpha, res, False, cls, res_lo)


def tile_check_cases(what: str):
    """The ragged subset tests/_exact_tile_check.py runs with the tile width forced ("tiles": N % 320 == 0, so that every forced
    width applies) or with another depth of the split-K ring ("split").  The dispatch path is not asserted there (variant 0)."""
    G, C = GemmCase, ConvCase
    if what == "tiles":
        return ([G(777, 320, 128, 0, "bias alpha res relu"), G(513, 640, 256, 0, "pair pairres bias"), G(129, 320, 192, 0, "guard bias res"),
                 G(1000, 640, 1280, 0, "slice bias"), G(300, 320, 256, 0, "f32 bias"),
                 G(256, 320, 128, 0, "gn bias", gn=(128, 32, 0), classes=("gn",))],
                [C(3, 6, 10, 64, 320, "S1", "bias res"), C(3, 6, 10, 64, 320, "S1", "biasrows pair pairres"),
                 C(3, 8, 16, 128, 320, "S1", "biasrows res"), C(3, 12, 20, 64, 320, "S2", "bias alpha res relu"),
                 C(3, 12, 20, 64, 320, "S2A", "bias"), C(3, 6, 10, 64, 320, "UP2", "pair bias"), C(3, 6, 10, 64, 320, "S2T", "dgrad bias"),
                 C(3, 6, 10, 128, 320, "S1", "dgrad"), C(11, 5, 7, 64, 320, "S1", "guard bias res"),
                 C(2, 16, 16, 64, 320, "S1", "gn bias", gn=(32, 0), classes=("gn",))])
    assert what == "split"
    return ([G(200, 64, 1024, 0, "bias alpha res", split=(2, 8)), G(1536, 320, 2048, 0, "bias res", split=(4, 8)),
             G(1536, 320, 2368, 0, "pair pairres bias", split=(4, 10)), G(1500, 320, 2368, 0, "bias alpha res relu", split=(4, 10))],
            [C(6, 16, 16, 256, 320, "S1", "bias res", split=(4, 9)), C(6, 16, 16, 256, 320, "S1", "biasrows pair pairres", split=(4, 9)),
             C(3, 8, 8, 256, 320, "S1", "bias", split=(4, 9))])


# ---------------------------------------------------------------------------------------------------------- device side
def _dev():
    return torch.device("cuda:0")


def record(name: str, cls: str, variant, elems: int, mism: int, extra: str = ""):
    print(f"EXACT {name} | {cls} | variant {variant} | {elems} elements | {mism} mismatches{extra}", flush=True)


def gemm_reference(case: GemmCase, cls: str, A=None, B=None):
    """-> dict of the CPU operands and the exact value v (conditions asserted).  A / B: column-slice parents when given."""
    Acl = AMP[cls]
    M, N, K = case.M, case.N, case.K
    aw = amp_w(cls, K)
    dens = 0.125 if cls == "gn" else 1.0
    A = draw_int((M, K), Acl["x"], seed_of(case.name, cls, 0)) if A is None else A
    B = draw_int((N, K), aw, seed_of(case.name, cls, 1), density=dens) if B is None else B
    words = case.epi.split()
    bias, res, res_lo, alpha = epi_operands(case.name, cls, words, M, N)
    extra = Acl["bias"] + Acl["res"] + 2
    dt = ref_dtype(float(M) * N * K)
    if dt == torch.float64:
        check_order_free(A.abs(), B.abs(), extra)
    else:
        check_worst_case(K, Acl["x"], aw, extra)
    acc = A.to(dt) @ B.to(dt).t()
    v = epilogue(acc, bias, alpha, res, "relu" in words, cls, res_lo)
    return dict(A=A, B=B, bias=bias, res=res, res_lo=res_lo, alpha=alpha, v=v)


def run_gemm(case: GemmCase, cls: str, check_variant: bool = True, bn: Optional[int] = None) -> int:
    """Runs one GEMM probe on the device and compares all of it bit for bit.  Returns the variant number that ran."""
    from sketch2img_amd import ops
    from sketch2img_amd._lib import lib
    d = _dev()
    M, N, K = case.M, case.N, case.K
    words = case.epi.split()
    r = gemm_reference(case, cls)
    A, B, v = r["A"], r["B"], r["v"]
    todev = lambda t: None if t is None else t.to(d)      # noqa: E731
    if "slice" in words:                                  # column-slice views of wider buffers: lda, ldb > K
        Abig = torch.full((M, K + 40), 5.0, dtype=torch.float16)
        Bbig = torch.full((N, K + 64), 5.0, dtype=torch.float16)
        Abig[:, 8:8 + K], Bbig[:, 32:32 + K] = A, B
        Ad, Bd = Abig.to(d)[:, 8:8 + K], Bbig.to(d)[:, 32:32 + K]
    else:
        Ad, Bd = A.to(d), B.to(d)
    res = r["res"]
    resd = None
    if res is not None:                                   # ldr > N
        rb = torch.full((M, N + 8), 3.0, dtype=torch.float16)
        rb[:, :N] = res
        resd = rb.to(d)[:, :N]
    reslo = None
    if r["res_lo"] is not None:
        rb = torch.full((M, N + 8), 3.0, dtype=torch.float16)
        rb[:, :N] = r["res_lo"]
        reslo = rb.to(d)[:, :N]
    ops._stream()                                         # (the shape queries plan with the stream's registered split-K workspace)
    variant = lib.skg_gemm_variant(M, N, K, 0, 0)
    if check_variant:
        assert variant == case.variant, f"{case.name}: skg_gemm_variant reports {variant}, the case is written for {case.variant}"
    lay = Layout.matrix(M, N, bn or bn_of(variant), case.split, f"{case.name} / {cls}")
    f32 = "f32" in words
    ldc = N + 16 if "guard" in words else N
    odt = torch.float32 if f32 else torch.float16
    out = torch.full((M, ldc), GUARD, device=d, dtype=odt)
    kw = dict(bias=todev(r["bias"]), residual=resd, alpha=r["alpha"], relu="relu" in words)
    if "pair" in words:
        buf = torch.full((M, 2 * N), GUARD, device=d, dtype=torch.float16)
        hi, lo = buf[:, :N], buf[:, N:]
        ops.gemm(Ad, Bd, out=hi, out_lo=lo, residual_lo=reslo, **kw)
        whi, wlo = expected_pair(v)
        assert_bits_equal(hi.contiguous(), whi, lay)
        assert_bits_equal(lo.contiguous(), wlo, lay)
        extra = f" | lo != 0 on {float((wlo != 0).double().mean()):.2f}"
    elif case.gn:
        HW, groups, fused = case.gn
        q = lib.skg_gemm_gn_fused(M, N, K, 0, 0, HW, groups)
        if check_variant:
            assert q == fused, f"{case.name}: skg_gemm_gn_fused reports {q}, the case is written for {fused}"
        _, part = ops.gemm(Ad, Bd, out=out[:, :N], gn_stats=(HW, groups), **kw)
        want = expected_f16(v, cls)
        assert_bits_equal(out, want, lay)
        sums = gn_sums(want, M // HW, HW, groups)
        got = part.buf.view(M // HW, HW // 128, groups, 2).double().cpu()
        nb = int((got != sums).sum())
        assert nb == 0, f"{case.name}: {nb} of {sums.numel()} GroupNorm partial sums differ from the fp64 sums of the fp16 outputs"
        extra = f" | gn fused {q}, {sums.numel()} partial sums exact"
    else:
        ops.gemm(Ad, Bd, out=out[:, :N], out_f32=f32, **kw)
        want = v.float() if f32 else expected_f16(v, cls)
        if f32:
            assert torch.equal(want.to(v.dtype), v)
        assert_bits_equal(out, want, lay)
        extra = ""
    record(case.name, cls, variant, M * N, 0, extra)
    return variant


def conv_reference(case: ConvCase, cls: str):
    x, w = conv_operands(case, cls)
    Acl = AMP[cls]
    OH, OW = out_size(case.mode, case.IH, case.IW)
    M = case.rows * OH * OW
    words = case.epi.split()
    bias, res, res_lo, alpha = epi_operands(case.name, cls, words, M, case.Cout, case.rows)
    if case.pad and bias is not None:
        bias[..., case.pad[1]:] = 0
    check_worst_case(case.K, Acl["x"], amp_w(cls, case.K), Acl["bias"] + Acl["res"] + 2)
    acc = nhwc(conv_ref(x.double(), w.double(), case.mode, dgrad="dgrad" in words))
    b = bias
    if bias is not None and bias.dim() == 2:
        b = bias.repeat_interleave(OH * OW, dim=0)
    v = epilogue(acc, b, alpha, res, "relu" in words, cls, res_lo)
    return dict(x=x, w=w, bias=bias, res=res, res_lo=res_lo, alpha=alpha, v=v, OH=OH, OW=OW, M=M)


def conv_pack(case: ConvCase, w: torch.Tensor, dev):
    from sketch2img_amd.packs import pack_conv, pack_conv_dgrad
    if case.pad:      # conv_in / conv_out: the real channels, padded by the pack itself
        ci, co = case.pad
        return pack_conv(w[:co, :ci], dev, cin_pad=case.Cin, cout_pad=case.Cout)
    return pack_conv_dgrad(w, dev) if case.has("dgrad") else pack_conv(w, dev)


def run_conv(case: ConvCase, cls: str, check_variant: bool = True, bn: Optional[int] = None) -> int:
    from sketch2img_amd import ops
    from sketch2img_amd._lib import lib
    d = _dev()
    r = conv_reference(case, cls)
    words = case.epi.split()
    M, N, v = r["M"], case.Cout, r["v"]
    todev = lambda t: None if t is None else t.to(d)      # noqa: E731
    ops._stream()
    mode = MODE_ID[case.mode]
    variant = lib.skg_gemm_variant(M, N, case.K, case.Cin, 1 + mode)
    if check_variant:
        if case.variant is not None:
            assert variant == case.variant, f"{case.name}: skg_gemm_variant reports {variant}, the case is written for {case.variant}"
        else:                                             # Cin = 32: the generic BK = 32 kernel; else the LDS-DMA family
            assert (variant // 1000 == 1) == (case.Cin % 64 != 0), f"{case.name}: variant {variant}"
    lay = Layout(case.rows, r["OH"], r["OW"], N, bn or bn_of(variant), case.split, f"{case.name} / {cls}")
    xd, wp = nhwc(r["x"]).to(d), conv_pack(case, r["w"], d)
    f32 = "f32" in words
    ldc = N + 16 if "guard" in words else N
    kw = dict(bias=todev(r["bias"]), residual=todev(r["res"]), alpha=r["alpha"], relu="relu" in words)
    extra = ""
    if "pair" in words:
        buf = torch.full((M, 2 * N), GUARD, device=d, dtype=torch.float16)
        hi, lo = buf[:, :N], buf[:, N:]
        ops.conv3x3(xd, wp, case.rows, case.IH, case.IW, mode, out=hi, out_lo=lo, residual_lo=todev(r["res_lo"]), **kw)
        whi, wlo = expected_pair(v)
        assert_bits_equal(hi.contiguous(), whi, lay)
        assert_bits_equal(lo.contiguous(), wlo, lay)
        extra = f" | lo != 0 on {float((wlo != 0).double().mean()):.2f}"
    elif f32:
        # (ops.conv3x3 has no fp32-output switch: the C entry point directly)
        out = torch.full((M, ldc), GUARD, device=d, dtype=torch.float32)
        brows = ops._bias_rows_flag(kw["bias"], case.rows, N)
        ops.check(lib.skg_conv3x3_f16(xd.data_ptr(), xd.stride(0), wp.data_ptr(), out.data_ptr(), None, ldc, case.rows, case.IH, case.IW,
                                      case.Cin, N, mode, ops._p(kw["bias"]), ops._p(kw["residual"]), None,
                                      N if kw["residual"] is not None else 0, r["alpha"], ops.EPI_OUT_F32 | brows | (1 if kw["relu"] else 0),
                                      None, 0, ops._stream()), "skg_conv3x3_f16")
        want = v.float()
        assert torch.equal(want.to(v.dtype), v)
        assert_bits_equal(out, want, lay)
    else:
        out = torch.full((M, ldc), GUARD, device=d, dtype=torch.float16)
        want = expected_f16(v, cls)
        if case.gn:
            groups, fused = case.gn
            HW = r["OH"] * r["OW"]
            q = lib.skg_gemm_gn_fused(M, N, case.K, case.Cin, 1 + mode, HW, groups)
            if check_variant:
                assert q == fused, f"{case.name}: skg_gemm_gn_fused reports {q}, the case is written for {fused}"
            _, part = ops.conv3x3(xd, wp, case.rows, case.IH, case.IW, mode, out=out[:, :N], gn_groups=groups, **kw)
            sums = gn_sums(want, case.rows, HW, groups)
            got = part.buf.view(case.rows, HW // 128, groups, 2).double().cpu()
            nb = int((got != sums).sum())
            assert nb == 0, f"{case.name}: {nb} of {sums.numel()} GroupNorm partial sums differ from the fp64 sums of the fp16 outputs"
            extra = f" | gn fused {q}, {sums.numel()} partial sums exact"
        else:
            ops.conv3x3(xd, wp, case.rows, case.IH, case.IW, mode, out=out[:, :N], **kw)
        if case.pad:
            assert not bool(want[:, case.pad[1]:].any())      # the pad columns are written, as zeros
        assert_bits_equal(out, want, lay)
    record(case.name, cls, variant, M * N, 0, extra)
    return variant


# ------------------------------------------------------------------------------------------------- relatives: references
# (rows, IH, IW, Cin, Cout) in the kernel's terms
UP2_CASES = ((2, 6, 10, 64, 160), (3, 8, 8, 128, 320))
C4X4_CASES = ((2, 12, 20, 64, 64), (3, 12, 20, 128, 160))          # K = 16 Cin >= 1024 on few tiles: split-K launches
CONVT_CASES = ((2, 5, 7, 64, 8), (2, 4, 6, 1024, 64), (3, 6, 10, 128, 160))
SC_CASES = ((3, 6, 10, 64, 160, 128, None), (2, 8, 16, 64, 160, 64, 16), (4, 64, 64, 64, 320, 64, 32))      # (..., K2, gn groups)
WINO_CASES = ((3, 8, 8, 64, 160), (1, 4, 4, 128, 64), (2, 6, 10, 64, 128), (2, 16, 16, 1280, 1280))
WGRAD_CASES = ((1, 64, 72), (127, 40, 64), (1281, 320, 64))          # (M, N, K)
ROWS_CASES = ((231, 64, 64, 77, 100), (600, 160, 128, 200, 257))     # (M, N, K, seg_rows, seg_stride)
GEGLU_KEEP_CASES = ((200, 128, 64), (300, 640, 320))


def up2_reference(rows, IH, IW, Cin, Cout, cls, pair_in=False):
    """skg_conv3x3_up2_f16: nearest 2x upsample + 3x3 convolution.  The pre-summed polyphase taps of integer weights are integers
    (up to four taps: |w| <= 4 a_w), so nothing rounds.  pair_in: x = x_hi + x_lo with an integer lo half in [-1, 1]."""
    name = f"up2 rows{rows} {IH}x{IW} {Cin}->{Cout}" + (" pair_in" if pair_in else "")
    A = AMP[cls]
    aw = amp_w(cls, 9 * Cin)
    x = draw_int((rows, Cin, IH, IW), A["x"], seed_of(name, cls, 0))
    x_lo = draw_int((rows, Cin, IH, IW), 1, seed_of(name, cls, 5)) if pair_in else None
    w = draw_int((Cout, Cin, 3, 3), aw, seed_of(name, cls, 1))
    bias = draw_int((Cout,), A["bias"], seed_of(name, cls, 2))
    check_worst_case(9 * Cin, A["x"] + (1 if pair_in else 0), aw, A["bias"])
    xs = x.double() + (x_lo.double() if pair_in else 0)
    v = epilogue(nhwc(conv_ref(xs, w.double(), "UP2")), bias, cls=cls)
    return dict(name=name, x=x, x_lo=x_lo, w=w, bias=bias, v=v)


def c4x4_reference(rows, IH, IW, Cin, Cout, cls):
    """skg_conv4x4s2_f16 with the up2-dgrad pack: the data gradient of upsample + convolution (Cout -> Cin forward channels), by
    autograd.  x is the gradient [rows, Cin, IH, IW] at the upsampled size."""
    name = f"conv4x4s2 rows{rows} {IH}x{IW} {Cin}->{Cout}"
    A = AMP[cls]
    aw = amp_w(cls, 36 * Cin)
    gy = draw_int((rows, Cin, IH, IW), A["x"], seed_of(name, cls, 0))
    w = draw_int((Cin, Cout, 3, 3), aw, seed_of(name, cls, 1))      # forward weight: Cout (low-res input) -> Cin (output) channels
    check_worst_case(36 * Cin, A["x"], aw)
    xr = torch.zeros(rows, Cout, IH // 2, IW // 2, dtype=torch.float64, requires_grad=True)
    conv_ref(xr, w.double(), "UP2").backward(gy.double())
    v = epilogue(nhwc(xr.grad), cls=cls)
    return dict(name=name, x=gy, w=w, v=v)


def convt_reference(rows, IH, IW, Cin, Cout, cls):
    """skg_convt4x4s2_f16 without tanh: ConvTranspose2d(4, stride 2, padding 1)."""
    name = f"convt4x4s2 rows{rows} {IH}x{IW} {Cin}->{Cout}"
    A = AMP[cls]
    aw = amp_w(cls, 4 * Cin)
    x = draw_int((rows, Cin, IH, IW), A["x"], seed_of(name, cls, 0))
    w = draw_int((Cin, Cout, 4, 4), aw, seed_of(name, cls, 1))
    bias = draw_int((Cout,), A["bias"], seed_of(name, cls, 2))
    check_worst_case(4 * Cin, A["x"], aw, A["bias"])
    v = epilogue(nhwc(F.conv_transpose2d(x.double(), w.double(), stride=2, padding=1)), bias, cls=cls)
    return dict(name=name, x=x, w=w, bias=bias, v=v)


def sc_reference(rows, IH, IW, Cin, Cout, K2, cls):
    """skg_conv3x3_sc_f16: conv3x3(X) + X2 . Wsc^T + bias."""
    name = f"conv_sc rows{rows} {IH}x{IW} {Cin}->{Cout} +{K2}"
    A = AMP[cls]
    K = 9 * Cin + K2
    aw = amp_w(cls, K)
    dens = 0.125 if cls == "gn" else 1.0
    x = draw_int((rows, Cin, IH, IW), A["x"], seed_of(name, cls, 0))
    x2 = draw_int((rows * IH * IW, K2), A["x"], seed_of(name, cls, 5))
    w = draw_int((Cout, Cin, 3, 3), aw, seed_of(name, cls, 1), density=dens)
    wsc = draw_int((Cout, K2), aw, seed_of(name, cls, 6), density=dens)
    bias = draw_int((Cout,), A["bias"], seed_of(name, cls, 2))
    check_worst_case(K, A["x"], aw, A["bias"])
    acc = nhwc(conv_ref(x.double(), w.double(), "S1")) + x2.double() @ wsc.double().t()
    return dict(name=name, x=x, x2=x2, w=w, wsc=wsc, bias=bias, v=epilogue(acc, bias, cls=cls))


def wino_reference(rows, IH, IW, Cin, Cout, cls, dgrad=False):
    """skg_conv3x3_wino_f16 with weights 4 * integers: U = G g G^T is an integer pack, V = B^T d B an integer fp16 holds, every
    component product sum an integer - the transforms round nothing and the expected value is that of the plain convolution.
    -> acc (fp64 for the small maps, fp32 under the worst-case bound for the 1280-channel one); the order-free condition on
    |V| . |U|^T of the emulated transforms is asserted by wino_emulate (tests/test_host_exact_probes.py runs it per case)."""
    name = f"wino rows{rows} {IH}x{IW} {Cin}->{Cout}" + (" dgrad" if dgrad else "")
    A = AMP[cls]
    # the weights are 4 * integers, so the class amplitudes are divided by the step where they can be: large |w| <= 4 * (a_w / 4);
    # small stays 4 * [-1, 1] and is thinned out above K = 2304 instead (density 2304 / K: sigma of the sum as at K = 2304), so
    # that the sums stay fp16 numbers (dense they reach 3127 at 1280 -> 1280)
    aw = max(1, amp_w(cls, 9 * Cin) // 4)
    dens = min(1.0, 2304.0 / (9 * Cin)) if cls == "small" else 1.0
    x = draw_int((rows, Cin, IH, IW), A["x"], seed_of(name, cls, 0))
    w = draw_int((Cin, Cout, 3, 3) if dgrad else (Cout, Cin, 3, 3), aw, seed_of(name, cls, 1), density=dens, step=4)
    # |V| <= 4 |x|, |U| <= 9 a_w per (component, channel); the output transform adds 9 of the 16 component sums
    check_worst_case(9 * Cin, 4 * A["x"], 9 * aw, A["bias"] + A["res"])
    dt = ref_dtype(float(rows) * IH * IW * Cout * 9 * Cin)
    acc = nhwc(conv_ref(x.to(dt), w.to(dt), "S1", dgrad=dgrad))
    return dict(name=name, x=x, w=w, acc=acc)


def wgrad_reference(M, N, K, cls):
    """skg_wgrad_f16: dW [N, K] = dY^T . X, db = colsum(dY), fp32 and exact."""
    name = f"wgrad {M}x{N}x{K}"
    A = AMP[cls]
    dy = draw_int((M, N), A["x"], seed_of(name, cls, 0))
    x = draw_int((M, K), A["x"], seed_of(name, cls, 1))
    check_worst_case(M, A["x"], A["x"])
    dW = dy.double().t() @ x.double()
    db = dy.double().sum(0)
    assert float(dW.abs().max()) * 2 < TWO24 and float(db.abs().max()) * 2 < TWO24      # ("=" and then "+=": twice the value)
    return dict(name=name, dy=dy, x=x, dW=dW, db=db)


def host_check_all(big: bool = False):
    """Every condition of every (case, class) of the GPU module, on the references alone.  The largest GEMM / convolution cases are
    reduced to their worst-case bound (gemm_reference / conv_reference do that from the size of the contraction) and, with
    big=False, to their first 256 rows.  Yields the case names it checked."""
    tg, tc = [a + b for a, b in zip(tile_check_cases("tiles"), tile_check_cases("split"))]
    for case in GEMM_CASES + tuple(tg):
        for cls in case.classes:
            c = case
            if float(case.M) * case.N * case.K > 2e8 and not big:      # (a draw of the same distribution, fewer rows)
                Acl = AMP[cls]
                check_worst_case(case.K, Acl["x"], amp_w(cls, case.K), Acl["bias"] + Acl["res"] + 2)
                c = dataclasses.replace(case, M=min(case.M, max(256, case.gn[0] if case.gn else 0)))
            r = gemm_reference(c, cls)
            if c.gn:
                gn_sums(r["v"].half(), c.M // c.gn[0], c.gn[0], c.gn[1])
            yield case.name, cls
    for case in CONV_CASES + tuple(tc):
        for cls in case.classes:
            r = conv_reference(case, cls)
            if case.gn:
                gn_sums(r["v"].half(), case.rows, r["OH"] * r["OW"], case.gn[0])
            yield case.name, cls
    for cls in ("small", "large"):
        for c in UP2_CASES:
            up2_reference(*c, cls)
            up2_reference(*c, cls, pair_in=True)
        for c in C4X4_CASES:
            c4x4_reference(*c, cls)
        for c in CONVT_CASES:
            convt_reference(*c, cls)
        for c in SC_CASES:
            sc_reference(*c[:6], cls)
        for c in WINO_CASES:
            if c[3] <= 128 or big:
                wino_reference(*c, cls)
        for c in WGRAD_CASES:
            wgrad_reference(*c, cls)
        yield "relatives", cls
    for c in SC_CASES:
        if c[6]:
            r = sc_reference(*c[:6], "gn")
            gn_sums(r["v"].half(), c[0], c[1] * c[2], c[6])
    for rows, H in BIG_CONV:      # (three fp32 convolutions of the 64 x 64-level shape: the longest part)
        for variant, cls in big_conv_variants(rows, H):
            if (rows, H) != BIG_CONV[0] and not big:      # (same K and amplitudes as the first shape: the worst-case bound alone)
                check_worst_case(9 * BIG_CIN, AMP[cls]["x"], amp_w(cls, 9 * BIG_CIN), AMP[cls]["bias"] + AMP[cls]["res"] + 2)
                continue
            name, _, _, _, v = big_conv_value(rows, H, variant, cls)
            if cls == "gn":
                gn_sums(v.half(), rows, H * H, BIG_GROUPS)
            yield name, cls
