"""Thin tensor-level wrappers over the C ABI (include/skg.h).

Every function takes torch CUDA tensors only to get at device pointers, strides and the current HIP
stream; all arithmetic happens inside libskg.so.  A 2-D "matrix view" is any tensor with
``stride(1) == 1`` - column slices of wider buffers are passed as (pointer, leading dimension).
"""
from __future__ import annotations

import ctypes
import threading
from typing import List, Optional, Sequence, Tuple

import torch

from ._lib import SkgError, SkgTap, check, lib

EPI_RELU, EPI_OUT_F32, EPI_GEGLU, EPI_BIAS_ROWS = 1, 2, 4, 8
CONV_S1, CONV_S2, CONV_UP2, CONV_S2T, CONV_S2A = 0, 1, 2, 3, 4
ATTN_CAUSAL, ATTN_ROWV, ATTN_RESIDENT_KV = 1, 2, 4


_workspace = {}
_workspace_lock = threading.Lock()      # (two host threads on one stream: allocate + register is one step)
WORKSPACE_BYTES = 128 << 20
_capture_owner = None      # set by private_buffers(): scratch / workspace owned by one hipGraph set


def _stream() -> int:
    """Current HIP stream.  The first launch on a (device, stream) registers that stream's split-K workspace with
    libskg.so (skg_set_workspace keeps one slab per stream: launches on different streams may run concurrently -
    several pipelines in one process, a graph capture stream next to the eager stream - and never share a slab;
    launches on ONE stream are ordered, so they share their stream's slab and scratch buffers)."""
    st = torch.cuda.current_stream()
    key = (st.device.index, st.cuda_stream)
    if key not in _workspace:
        with _workspace_lock:
            if key not in _workspace:
                with torch.cuda.device(st.device):
                    ws = torch.empty(WORKSPACE_BYTES // 4, device=st.device, dtype=torch.float32)
                    check(lib.skg_set_workspace(ws.data_ptr(), WORKSPACE_BYTES, st.cuda_stream), "skg_set_workspace")
                    _workspace[key] = ws
    return st.cuda_stream


def release_stream(stream: "torch.cuda.Stream"):
    """Drop the split-K slab, the library's registry entry and the scratch buffers of a stream that will not launch again (a
    sampler's side stream, a retired graph set): they are otherwise held for the life of the process."""
    key = (stream.device.index, stream.cuda_stream)
    with _workspace_lock:
        if _workspace.pop(key, None) is not None:
            check(lib.skg_set_workspace(None, 0, stream.cuda_stream), "skg_set_workspace")
    # (scratch keys carry (str(device), stream handle): the same handle value - 0, the default stream - exists on every device)
    for k in [k for k in _scratch if isinstance(k, tuple) and len(k) > 1 and isinstance(k[1], tuple) and k[1][1] == stream.cuda_stream
              and str(k[1][0]) == str(stream.device)]:
        _scratch.pop(k, None)


class private_buffers:
    """``with private_buffers(owner):`` inside a ``torch.cuda.graph`` capture - the launches captured in the block use a
    split-K workspace and scratch buffers that belong to `owner` (a dict that keeps them alive) instead of the capture
    stream's shared ones, so two graph sets captured on torch's one capture stream can be replayed concurrently on
    different streams.  The workspace must be allocated BEFORE the capture starts: ``prepare(owner, dev)``."""

    @staticmethod
    def prepare(owner: dict, dev):
        owner["ws"] = torch.empty(WORKSPACE_BYTES // 4, device=dev, dtype=torch.float32)
        owner["scratch"] = {}

    def __init__(self, owner: dict):
        self.owner = owner

    def __enter__(self):
        global _capture_owner
        st = torch.cuda.current_stream()
        self.key = (st.device.index, st.cuda_stream)
        self.prev_owner, _capture_owner = _capture_owner, self.owner
        with _workspace_lock:
            self.prev_ws = _workspace.get(self.key)
            _workspace[self.key] = self.owner["ws"]
            check(lib.skg_set_workspace(self.owner["ws"].data_ptr(), WORKSPACE_BYTES, st.cuda_stream), "skg_set_workspace")
        return self

    def __exit__(self, *exc):
        global _capture_owner
        _capture_owner = self.prev_owner
        with _workspace_lock:
            if self.prev_ws is None:
                del _workspace[self.key]
                check(lib.skg_set_workspace(None, 0, self.key[1]), "skg_set_workspace")
            else:
                _workspace[self.key] = self.prev_ws
                check(lib.skg_set_workspace(self.prev_ws.data_ptr(), WORKSPACE_BYTES, self.key[1]), "skg_set_workspace")


def _skey(dev):
    """Scratch-buffer key part: device + current stream (see _stream)."""
    return (str(dev), torch.cuda.current_stream().cuda_stream)


def _scratch_buf(key, n: int, dev) -> torch.Tensor:
    """fp32 scratch of n floats for `key`: the current stream's, or - inside private_buffers() - the graph set's own."""
    store = _scratch if _capture_owner is None else _capture_owner["scratch"]
    if key not in store:
        store[key] = torch.empty(n, device=dev, dtype=torch.float32)
    return store[key]


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _ld(t: torch.Tensor) -> int:
    assert t.dim() == 2 and (t.stride(1) == 1 or t.shape[1] == 1), "matrix view must be row-major"
    return t.stride(0)


def _f16(*ts):
    for t in ts:
        assert t is None or (t.is_cuda and t.dtype == torch.float16), "fp16 CUDA tensor expected"


class GNPartial:
    """Per (sample, 128-row chunk, group) sum / sum of squares of a producer's output - what `groupnorm(partial=)` folds
    instead of reading the tensor a second time (skg_gemm_f16 / skg_conv3x3_f16 with gn_partial)."""
    __slots__ = ("buf", "nch", "rows", "groups")

    def __init__(self, rows: int, HW: int, groups: int, dev):
        self.rows, self.nch, self.groups = rows, HW // 128, groups
        self.buf = torch.empty(rows * self.nch * groups * 2, device=dev, dtype=torch.float32)


class Pair:
    """Accuracy mode: a tensor kept as (hi, lo) fp16 views with one pitch, value = hi + lo; `full` = the [M, 2C] tensor
    [hi | lo] when the two are its halves (then the pair is directly a K-doubled matmul operand)."""
    __slots__ = ("hi", "lo", "full")

    def __init__(self, hi, lo, full=None):
        self.hi, self.lo, self.full = hi, lo, full

    @staticmethod
    def empty(M: int, C: int, dev) -> "Pair":
        buf = torch.empty(M, 2 * C, device=dev, dtype=torch.float16)
        return Pair(buf[:, :C], buf[:, C:], buf)


def _bias_rows_flag(bias: Optional[torch.Tensor], rows: int, Cout: int) -> int:
    """EPI_BIAS_ROWS for a 2-D bias of a 3x3 convolution - one [Cout] row per sample, [rows, Cout] contiguous - and 0 for the shared
    1-D one.  Any other shape raises ValueError before the C call."""
    if bias is None or bias.dim() == 1:
        return 0
    if bias.dim() != 2 or tuple(bias.shape) != (rows, Cout) or not bias.is_contiguous():
        raise ValueError(f"bias per sample: a contiguous [rows = {rows}, Cout = {Cout}] tensor expected, got {tuple(bias.shape)}")
    return EPI_BIAS_ROWS


def gn_fusable(M: int, N: int, HW: int, groups: int) -> bool:
    """Shapes the `gn_stats=` form of gemm / conv3x3 accepts (whole 128-row chunks per sample, even group width)."""
    return (HW % 128 == 0 and HW // 128 <= 128 and M % HW == 0 and N % groups == 0 and N % 8 == 0 and
            (N // groups) % 2 == 0 and N // groups >= 4 and N <= 4096)


def gn_concat_ok(CA: int, CB: int, groups: int, ga: int, gb: int) -> bool:
    """Can groupnorm(partial=(pa, CA, pb)) regroup the two producers' sums for a [CA | CB]-channel concatenation?"""
    C = CA + CB
    if C % groups or CA % ga or CB % gb:
        return False
    cpg = C // groups
    return CA % cpg == 0 and cpg % (CA // ga) == 0 and cpg % (CB // gb) == 0


def gemm(A: torch.Tensor, B: torch.Tensor, out: Optional[torch.Tensor] = None, *,
         bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
         alpha: float = 1.0, relu: bool = False, out_f32: bool = False, geglu: bool = False, gn_stats=None,
         out_lo: Optional[torch.Tensor] = None, residual_lo: Optional[torch.Tensor] = None):
    """out[m][n] = epi(alpha*(A[m,:] . B[n,:] + bias[n]) + residual[m][n]);  A [M,K], B [N,K].
    geglu=True: B / bias are the interleaved FF1 pack and out is [M, N/2] = a * gelu(g).
    gn_stats=(HW, groups): also returns the GroupNorm partial sums of the output -> (out, GNPartial).
    out_lo / residual_lo (accuracy mode): the output / residual as (hi, lo) pairs of fp16 views with equal pitch."""
    _f16(A, B, bias, residual, out_lo, residual_lo)
    M, K = A.shape
    N = B.shape[0]
    assert B.shape[1] == K
    if out_lo is not None or residual_lo is not None:
        assert out is not None and not (out_f32 or geglu)
        assert out_lo is None or _ld(out_lo) == _ld(out)
        assert residual_lo is None or residual is None or _ld(residual_lo) == _ld(residual)
    elif out is None:
        out = torch.empty(M, N // 2 if geglu else N, device=A.device,
                          dtype=torch.float32 if out_f32 else torch.float16)
    r_any = residual if residual is not None else residual_lo
    flags = (EPI_RELU if relu else 0) | (EPI_OUT_F32 if out_f32 else 0) | (EPI_GEGLU if geglu else 0)
    HW, groups = gn_stats or (0, 0)      # the partial sums of the output (a pair's hi part) come with it
    part = GNPartial(M // HW, HW, groups, A.device) if gn_stats is not None else None
    check(lib.skg_gemm_f16(_p(A), _ld(A), _p(B), _ld(B), _p(out), _p(out_lo), _ld(out), M, N, K, _p(bias),
                           _p(residual), _p(residual_lo), _ld(r_any) if r_any is not None else 0, alpha, flags,
                           _p(part.buf) if part is not None else None, HW, groups, _stream()), "skg_gemm_f16")
    return out if part is None else (out, part)


def gemm_geglu_keep(A: torch.Tensor, B: torch.Tensor, bias: Optional[torch.Tensor] = None, out=None, pre=None):
    """FF1 with the gate fused AND the pre-activation kept: returns (a * gelu(g) [M, N/2], H [M, N] interleaved pack)."""
    _f16(A, B, bias)
    M, K = A.shape
    N = B.shape[0]
    if out is None:
        out = torch.empty(M, N // 2, device=A.device, dtype=torch.float16)
    if pre is None:
        pre = torch.empty(M, N, device=A.device, dtype=torch.float16)
    check(lib.skg_gemm_f16_geglu_keep(_p(A), _ld(A), _p(B), _ld(B), _p(out), _ld(out), _p(pre), _ld(pre), M, N, K,
                                      _p(bias), _stream()), "skg_gemm_f16_geglu_keep")
    return out, pre


def _ff_block(X, gamma, beta, eps, pack, bias1_pack, bias2, bias_proj, R, out, want_stats, keep_from, gn):
    """The skg_ff_block_f16 launch behind ff_block / ff_block_proj -> (out, stats | None, pre | None, GNPartial | None)."""
    pair = isinstance(X, Pair)
    Xh, Xl = (X.hi, X.lo) if pair else (X, None)
    Rh, Rl = (R.hi, R.lo) if pair and R is not None else (R, None)
    _f16(Xh, Xl, gamma, beta, pack, bias2, bias_proj, Rh, Rl)
    M, C = Xh.shape
    assert pack.is_contiguous() and pack.dim() == 3 and pack.shape[1:] == (60, 512) and bias1_pack.dtype == torch.float32
    F = (pack.shape[0] - (0 if bias_proj is None else 5)) * 32
    assert bias_proj is None or bias1_pack.shape[0] * 32 == F
    dev = Xh.device
    if out is None:
        out = Pair.empty(M, C, dev) if pair else torch.empty(M, C, device=dev, dtype=torch.float16)
    Yh, Yl = (out.hi, out.lo) if pair else (out, None)
    assert not pair or (_ld(Xl) == _ld(Xh) and _ld(Yl) == _ld(Yh) and (Rl is None or _ld(Rl) == _ld(Rh)))
    stats = torch.empty(M, 2, device=dev, dtype=torch.float32) if want_stats else None
    pre = None if keep_from is None else torch.empty(M - keep_from, 2 * F, device=dev, dtype=torch.float16)
    HW, groups = gn or (0, 0)
    part = GNPartial(M // HW, HW, groups, dev) if gn is not None else None
    check(lib.skg_ff_block_f16(_p(Xh), _p(Xl), _ld(Xh), _p(Yh), _p(Yl), _ld(Yh), M, C, F, _p(gamma), _p(beta), eps, _p(pack),
                               _p(bias1_pack), _p(bias2), _p(bias_proj), _p(Rh), _p(Rl), _ld(Rh) if Rh is not None else 0, _p(stats),
                               _p(pre), _ld(pre) if pre is not None else 0, keep_from or 0,
                               _p(part.buf) if part is not None else None, HW, groups, _stream()), "skg_ff_block_f16")
    return out, stats, pre, part


def ff_block(X, gamma, beta, eps: float, pack: torch.Tensor, bias1_pack: torch.Tensor, bias2: torch.Tensor,
             out=None, want_stats: bool = False, keep_from: Optional[int] = None):
    """Fused feed-forward sub-block at C = 320: out = X + b2 + W2 . geglu(W1 . LayerNorm(X) + b1) in one launch
    (skg_ff_block_f16; pack / bias1_pack from packs.pack_ff_block).  out may be X.
    keep_from=m0: rows >= m0 also store the FF1 output (interleaved pack, what geglu_bwd reads) -> returned last.
    X (and out) may be ops.Pair objects (accuracy mode)."""
    out, stats, pre, _ = _ff_block(X, gamma, beta, eps, pack, bias1_pack, bias2, None, None, out, want_stats, keep_from, None)
    if keep_from is None:
        return (out, stats) if want_stats else out
    return (out, stats, pre) if want_stats else (out, pre)


def ff_block_proj(X, gamma, beta, eps: float, pack: torch.Tensor, bias1_pack: torch.Tensor, bias2: torch.Tensor, bias_proj: torch.Tensor,
                  R: torch.Tensor, out=None, want_stats: bool = False, keep_from: Optional[int] = None, gn: Optional[Tuple[int, int]] = None):
    """ff_block followed by Transformer2DModel.proj_out and the outer residual in the same launch (skg_ff_block_f16 with bias_proj):
    out = R + bias_proj + W_proj . fp16(X + FF(LayerNorm(X))); pack = packs.pack_ff_block(..., w_proj) (five chunks more).
    gn = (HW, groups): also the GroupNorm partial sums of out.  Returns (out, stats | None, pre | None, GNPartial | None);
    out must not be X (it may be R).  Accuracy mode: X, R and out are pairs."""
    assert bias_proj is not None and R is not None and (out is not None or not isinstance(X, Pair))
    return _ff_block(X, gamma, beta, eps, pack, bias1_pack, bias2, bias_proj, R, out, want_stats, keep_from, gn)


def xattn_block(X, HW: int, heads: int, Nkv: int, gamma, beta, eps: float, wpack: torch.Tensor, kvpack: torch.Tensor,
                bias_out: torch.Tensor, scale: float, out=None, keep_from: Optional[int] = None):
    """Fused cross-attention sub-block at C = 320, 8 heads: out = X + bo + Wo . Attention(Wq . LayerNorm(X), K, V) over the text
    keys of each row's image, in one launch (skg_xattn_block_f16; packs from packs.pack_xattn_weights / pack_xattn_kv).
    X (and out) may be ops.Pair objects (accuracy mode)."""
    pair = isinstance(X, Pair)
    Xh = X.hi if pair else X
    _f16(Xh, gamma, beta, wpack, kvpack, bias_out)
    M, C = Xh.shape
    wp, kp = (60, 16) if heads == 8 else (80, 20)      # pieces per head: 8 x 40 (padded to 48) or 5 x 64
    assert wpack.is_contiguous() and wpack.shape == (heads, wp, 512) and kvpack.is_contiguous() and kvpack.shape == (M // HW, heads, kp, 512)
    if out is None:
        out = Pair.empty(M, C, Xh.device) if pair else torch.empty(M, C, device=Xh.device, dtype=torch.float16)
    Yh, Yl = (out.hi, out.lo) if pair else (out, None)
    assert not pair or (_ld(X.lo) == _ld(Xh) and _ld(Yl) == _ld(Yh))
    st = q = o = lse = None
    if keep_from is not None:      # stashing launch: -> (out, stats, q, o, lse) of the rows >= keep_from
        Mk = M - keep_from
        dev = Xh.device
        st = torch.empty(Mk, 2, device=dev, dtype=torch.float32)
        q = torch.empty(Mk, C, device=dev, dtype=torch.float16)
        o = torch.empty(Mk, C, device=dev, dtype=torch.float16)
        lse = torch.empty(Mk // HW, heads, HW, device=dev, dtype=torch.float32)
    check(lib.skg_xattn_block_f16(_p(Xh), _p(X.lo) if pair else None, _ld(Xh), _p(Yh), _p(Yl), _ld(Yh), M, HW, C, heads, Nkv,
                                  _p(gamma), _p(beta), eps, _p(wpack), _p(kvpack), _p(bias_out), scale, _p(st), _p(q), _p(o), C,
                                  _p(lse), keep_from or 0, _stream()), "skg_xattn_block_f16")
    return out if keep_from is None else (out, st, q, o, lse)


def conv3x3(X: torch.Tensor, Wp: torch.Tensor, rows: int, IH: int, IW: int, mode: int = CONV_S1,
            out: Optional[torch.Tensor] = None, *, bias=None, residual=None, alpha: float = 1.0,
            relu: bool = False, gn_groups: Optional[int] = None, out_lo=None, residual_lo=None):
    """X [rows*IH*IW, Cin] (view), Wp [Cout, 9*Cin] tap-major.  Returns [rows*OH*OW, Cout];
    gn_groups=G: (out, GNPartial) - the GroupNorm partial sums of the output come with it.
    bias: [Cout], or [rows, Cout] - a row per sample (EPI_BIAS_ROWS: output row m adds bias[m // (OH*OW)]).
    out_lo / residual_lo (accuracy mode): see gemm."""
    Cin = X.shape[1]
    Cout = Wp.shape[0]
    brows = _bias_rows_flag(bias, rows, Cout)
    _f16(X, Wp, bias, residual, out_lo, residual_lo)
    assert Wp.shape[1] == 9 * Cin and Wp.is_contiguous() and X.shape[0] == rows * IH * IW
    if mode == CONV_S1:
        OH, OW = IH, IW
    elif mode in (CONV_S2, CONV_S2A):
        OH, OW = IH // 2, IW // 2
    else:
        OH, OW = IH * 2, IW * 2
    if out is None:
        out = torch.empty(rows * OH * OW, Cout, device=X.device, dtype=torch.float16)
    assert out_lo is None or _ld(out_lo) == _ld(out)
    assert residual_lo is None or residual is None or _ld(residual_lo) == _ld(residual)
    r_any = residual if residual is not None else residual_lo
    part = GNPartial(rows, OH * OW, gn_groups, X.device) if gn_groups is not None else None
    check(lib.skg_conv3x3_f16(_p(X), _ld(X), _p(Wp), _p(out), _p(out_lo), _ld(out), rows, IH, IW, Cin, Cout, mode,
                              _p(bias), _p(residual), _p(residual_lo), _ld(r_any) if r_any is not None else 0,
                              alpha, (EPI_RELU if relu else 0) | brows, _p(part.buf) if part is not None else None, gn_groups or 0,
                              _stream()), "skg_conv3x3_f16")
    return out if part is None else (out, part)


def conv3x3_small(X: torch.Tensor, Wp: torch.Tensor, B: int, IH: int, IW: int, stride: int = 1, out: Optional[torch.Tensor] = None, *,
                  bias=None, silu: bool = False):
    """The small-channel 3x3 convolution of the ControlNet hint encoder (skg_conv3x3_small_f16): X the fp32 NCHW picture
    [B, 3, IH, IW] (contiguous, read as it is) or an fp16 [B*IH*IW, 16] view; Wp = packs.pack_conv_small (Cout 16 or 32); stride 1
    or 2 (even IH, IW).  -> fp16 [B*OH*OW, Cout] with bias and, with silu, the SiLU applied in registers."""
    if X.dtype == torch.float32:
        if X.dim() != 4 or tuple(X.shape) != (B, 3, IH, IW) or not X.is_contiguous() or not X.is_cuda:
            raise ValueError(f"conv3x3_small: a contiguous fp32 CUDA picture [{B}, 3, {IH}, {IW}] expected, got {tuple(X.shape)}")
        Cin, ldx = 3, 0
    else:
        _f16(X)
        if X.dim() != 2 or tuple(X.shape) != (B * IH * IW, 16):
            raise ValueError(f"conv3x3_small: an fp16 [{B * IH * IW}, 16] view expected, got {tuple(X.shape)}")
        Cin, ldx = 16, _ld(X)
    _f16(Wp, bias, out)
    Cout = Wp.shape[0]
    if stride not in (1, 2) or (stride == 2 and (IH % 2 or IW % 2)):
        raise ValueError(f"conv3x3_small: stride 1, or 2 on an even map, expected (stride {stride}, {IH} x {IW})")
    assert Wp.is_contiguous() and Wp.shape[1] == (64 if Cin == 3 else 160) and (bias is None or bias.shape == (Cout,))
    M = B * (IH // stride) * (IW // stride)
    if out is None:
        out = torch.empty(M, Cout, device=X.device, dtype=torch.float16)
    assert out.shape == (M, Cout)
    check(lib.skg_conv3x3_small_f16(_p(X), ldx, _p(Wp), _p(out), _ld(out), B, IH, IW, Cin, Cout, stride, _p(bias), int(silu), _stream()),
          "skg_conv3x3_small_f16")
    return out


def conv3x3_sc(X: torch.Tensor, X2: torch.Tensor, Wcat: torch.Tensor, rows: int, IH: int, IW: int, out: Optional[torch.Tensor] = None, *,
               bias=None, relu: bool = False, gn_groups: Optional[int] = None, out_lo=None):
    """conv2 + conv_shortcut of a ResnetBlock as ONE implicit GEMM (skg_conv3x3_sc_f16): X [rows*IH*IW, Cin] the 3x3 input,
    X2 [rows*IH*IW, K2] the block's input (accuracy mode: the pair buffer [x_hi | x_lo]), Wcat [Cout, 9*Cin + K2], bias =
    conv2.bias + conv_shortcut.bias.  Returns out, or (out, GNPartial) with gn_groups.  Raises SkgError(rc = -2) when declined."""
    _f16(X, X2, Wcat, bias, out_lo)
    Cin, K2, Cout = X.shape[1], X2.shape[1], Wcat.shape[0]
    assert Wcat.shape[1] == 9 * Cin + K2 and Wcat.is_contiguous() and X.shape[0] == X2.shape[0] == rows * IH * IW
    if out is None:
        out = torch.empty(rows * IH * IW, Cout, device=X.device, dtype=torch.float16)
    assert out_lo is None or _ld(out_lo) == _ld(out)
    part = GNPartial(rows, IH * IW, gn_groups, X.device) if gn_groups is not None else None
    check(lib.skg_conv3x3_sc_f16(_p(X), _ld(X), _p(X2), _ld(X2), K2, _p(Wcat), _p(out), _p(out_lo), _ld(out), rows, IH, IW, Cin, Cout,
                                 _p(bias), EPI_RELU if relu else 0, _p(part.buf) if part is not None else None,
                                 gn_groups or 0, _stream()), "skg_conv3x3_sc_f16")
    return (out, part) if part is not None else out


def groupnorm_wino(X: torch.Tensor, rows: int, IH: int, IW: int, groups: int, eps: float, gamma, beta, silu: bool):
    """GroupNorm(+SiLU) of a small map straight into the Winograd input transform of its consumer (skg_groupnorm_wino_fwd):
    -> (V [rows*IH/2*IW/2, 16*C] for conv3x3_wino(None, ..., V=V), statistics [rows, groups, 2]).  Raises SkgError(rc = -2) when the
    (row, group) slice does not fit one workgroup (run groupnorm + conv3x3_wino on its output)."""
    _f16(X, gamma, beta)
    C = X.shape[1]
    V = torch.empty(rows * (IH // 2) * (IW // 2), 16 * C, device=X.device, dtype=torch.float16)
    st = torch.empty(rows, groups, 2, device=X.device, dtype=torch.float32)
    check(lib.skg_groupnorm_wino_fwd(_p(X), _ld(X), _p(V), rows, IH, IW, C, groups, eps, _p(gamma), _p(beta), int(silu), _p(st), _stream()),
          "skg_groupnorm_wino_fwd")
    return V, st


def conv3x3_wino(X: Optional[torch.Tensor], U: torch.Tensor, rows: int, IH: int, IW: int, out: Optional[torch.Tensor] = None, *, bias=None,
                 residual=None, relu: bool = False, out_lo=None, residual_lo=None, V: Optional[torch.Tensor] = None):
    """3x3 stride-1 convolution by Winograd F(2x2, 3x3) (skg_conv3x3_wino_f16): X [rows*IH*IW, Cin] (view), U [Cout, 16*Cin] =
    packs.pack_conv_wino(weight).  Returns [rows*IH*IW, Cout].  Raises SkgError(rc = -2) when declined (odd map, Cin % 64, no room for the
    16 fp32 slabs in the stream's workspace): the caller runs conv3x3.  X = None, V = groupnorm_wino(...)[0]: the input transform exists.
    bias: [Cout], or [rows, Cout] - a row per sample, as conv3x3."""
    Cout = U.shape[0]
    brows = _bias_rows_flag(bias, rows, Cout)
    _f16(X, U, bias, residual, out_lo, residual_lo, V)
    Cin = U.shape[1] // 16
    Mt = rows * (IH // 2) * (IW // 2)
    if X is None:
        assert V is not None and V.shape == (Mt, 16 * Cin) and V.is_contiguous() and U.is_contiguous()
        dev_ = V.device
    else:
        assert X.shape[1] == Cin and U.is_contiguous() and X.shape[0] == rows * IH * IW
        dev_ = X.device
        V = torch.empty(Mt, 16 * Cin, device=dev_, dtype=torch.float16)
    if out is None:
        out = torch.empty(rows * IH * IW, Cout, device=dev_, dtype=torch.float16)
    assert out_lo is None or _ld(out_lo) == _ld(out)
    assert residual_lo is None or residual is None or _ld(residual_lo) == _ld(residual)
    r_any = residual if residual is not None else residual_lo
    st = _stream()
    check(lib.skg_conv3x3_wino_f16(_p(X), _ld(X) if X is not None else 0, _p(U), _p(V), _p(out), _p(out_lo), _ld(out), rows, IH, IW, Cin, Cout, _p(bias),
                                   _p(residual), _p(residual_lo), _ld(r_any) if r_any is not None else 0, (EPI_RELU if relu else 0) | brows, st),
          "skg_conv3x3_wino_f16")
    return out


def conv_up2(X: torch.Tensor, Wpp: torch.Tensor, rows: int, IH: int, IW: int, out: Optional[torch.Tensor] = None, *, bias=None, W9=None):
    """Nearest-2x upsample + 3x3 conv, polyphase (four 4-tap convs over the low-res input).  X [rows*IH*IW, Cin] (view),
    Wpp [4, Cout, 4*Cin] (packs.pack_conv_up2).  Returns [rows*2IH*2IW, Cout].  W9: the layer's ordinary 9-tap pack - the
    fall-back when the launch is declined (SKG_E_UNSUPPORTED)."""
    _f16(X, Wpp, bias)
    Cin, Cout = X.shape[1], Wpp.shape[1]
    assert Wpp.shape == (4, Cout, 4 * Cin) and Wpp.is_contiguous() and X.shape[0] == rows * IH * IW
    if out is None:
        out = torch.empty(rows * 4 * IH * IW, Cout, device=X.device, dtype=torch.float16)
    try:
        check(lib.skg_conv3x3_up2_f16(_p(X), _ld(X), _p(Wpp), _p(out), None, _ld(out), rows, IH, IW, Cin, Cout, 0, _p(bias), _stream()),
              "skg_conv3x3_up2_f16")
    except SkgError as e:      # the LDS-DMA kernel declined the launch (an operand >= 2 GiB): the 9-tap gather form, when the caller has its pack
        if e.rc != -2 or W9 is None:
            raise
        return conv3x3(X, W9, rows, IH, IW, CONV_UP2, out=out, bias=bias)
    return out


def conv_up2_hilo(X2: torch.Tensor, Wpp3: torch.Tensor, rows: int, IH: int, IW: int, out: Pair, *, bias=None, W9x2=None):
    """Accuracy mode: conv_up2 on the pair buffer X2 = [x_hi | x_lo] ([rows*IH*IW, 2C]) with (hi, lo) pre-summed weights
    Wpp3 [4, Cout, 4 * 3C] (packs.pack_conv_up2_hilo); the output is the pair `out`.  W9x2 (a callable returning the layer's 9-tap
    [W | W] pack, built on first use): the fall-back when the polyphase launch is declined (an operand >= 2 GiB - the pair
    buffer is twice as wide, so the limit comes at half the batch size of conv_up2's): ADVICE r4."""
    _f16(X2, Wpp3, bias, out.hi, out.lo)
    C, Cout = X2.shape[1] // 2, Wpp3.shape[1]
    assert Wpp3.shape == (4, Cout, 12 * C) and Wpp3.is_contiguous() and X2.shape[0] == rows * IH * IW and _ld(out.hi) == _ld(out.lo)
    try:
        check(lib.skg_conv3x3_up2_f16(_p(X2), _ld(X2), _p(Wpp3), _p(out.hi), _p(out.lo), _ld(out.hi), rows, IH, IW, C, Cout, 1, _p(bias),
                                      _stream()), "skg_conv3x3_up2_f16 (pair input)")
    except SkgError as e:
        if e.rc != -2 or W9x2 is None:
            raise
        conv3x3(X2, W9x2(), rows, IH, IW, CONV_UP2, out=out.hi, bias=bias, out_lo=out.lo)
    return out


def conv_up2_pairout(X: torch.Tensor, Wpp: torch.Tensor, rows: int, IH: int, IW: int, out: Pair, *, bias=None):
    """Accuracy mode, cheaper upsampler (round 5): the default polyphase launch on the hi part X [rows*IH*IW, C] (a view of the
    pair buffer) with the default pack Wpp [4, Cout, 4*C]; only the OUTPUT is a pair.  Raises SkgError(rc = -2) when declined."""
    _f16(X, Wpp, bias, out.hi, out.lo)
    Cin, Cout = X.shape[1], Wpp.shape[1]
    assert Wpp.shape == (4, Cout, 4 * Cin) and Wpp.is_contiguous() and X.shape[0] == rows * IH * IW and _ld(out.hi) == _ld(out.lo)
    check(lib.skg_conv3x3_up2_f16(_p(X), _ld(X), _p(Wpp), _p(out.hi), _p(out.lo), _ld(out.hi), rows, IH, IW, Cin, Cout, 0, _p(bias),
                                  _stream()), "skg_conv3x3_up2_f16 (pair output)")
    return out


def gemm_rows(A: torch.Tensor, B: torch.Tensor, out: torch.Tensor, seg_rows: int, seg_stride: int, *, bias=None):
    """A [M, K] @ B[N, K]^T with product row m stored to row (m // seg_rows) * seg_stride + m % seg_rows of `out`
    (out: [(M // seg_rows) * seg_stride, >= N] view): every batch row's block into its slot of a longer per-row buffer."""
    _f16(A, B, out, bias)
    M, K = A.shape
    N = B.shape[0]
    assert B.shape[1] == K and M % seg_rows == 0 and out.shape[0] >= (M // seg_rows - 1) * seg_stride + seg_rows and out.shape[1] >= N
    try:
        check(lib.skg_gemm_f16_rows(_p(A), _ld(A), _p(B), _ld(B), _p(out), _ld(out), M, N, K, _p(bias), seg_rows, seg_stride, _stream()),
              "skg_gemm_f16_rows")
    except SkgError as e:      # declined: one GEMM per batch row straight into its slot
        if e.rc != -2:
            raise
        for b in range(M // seg_rows):
            gemm(A[b * seg_rows:(b + 1) * seg_rows], B, out=out[b * seg_stride:b * seg_stride + seg_rows, :N], bias=bias)
    return out


def conv4x4s2(X: torch.Tensor, W16: torch.Tensor, rows: int, IH: int, IW: int, out: Optional[torch.Tensor] = None, *, bias=None, W9T=None):
    """4 x 4 stride-2 convolution, padding 1 (the data gradient of conv_up2).  X [rows*IH*IW, Cin] (view), W16 [Cout, 16*Cin]
    (packs.pack_conv_up2_dgrad).  Returns [rows*(IH/2)*(IW/2), Cout]."""
    _f16(X, W16, bias)
    Cin, Cout = X.shape[1], W16.shape[0]
    assert W16.shape == (Cout, 16 * Cin) and W16.is_contiguous() and X.shape[0] == rows * IH * IW
    if out is None:
        out = torch.empty(rows * (IH // 2) * (IW // 2), Cout, device=X.device, dtype=torch.float16)
    try:
        check(lib.skg_conv4x4s2_f16(_p(X), _ld(X), _p(W16), _p(out), _ld(out), rows, IH, IW, Cin, Cout, _p(bias), _stream()),
              "skg_conv4x4s2_f16")
    except SkgError as e:      # declined: the 9-tap dgrad at the upsampled size + 2 x 2 sum-pool it replaced
        if e.rc != -2 or W9T is None or bias is not None:
            raise
        return sumpool2x2(conv3x3(X, W9T, rows, IH, IW, bias=bias), rows, IH // 2, IW // 2, out=out)
    return out


_scratch = {}


def _gn_scratch(rows: int, groups: int, dev) -> torch.Tensor:
    n = lib.skg_groupnorm_scratch_floats(rows, groups)
    return _scratch_buf(("gn", _skey(dev), n), n, dev)


def groupnorm_stats(X, rows, HW, groups, eps, stats=None):
    _f16(X)
    C = X.shape[1]
    if stats is None:
        stats = torch.empty(rows, groups, 2, device=X.device, dtype=torch.float32)
    check(lib.skg_groupnorm_stats(_p(X), _ld(X), rows, HW, C, groups, eps, _p(stats),
                                  _p(_gn_scratch(rows, groups, X.device)), _stream()), "skg_groupnorm_stats")
    return stats


def groupnorm_apply(X, rows, HW, groups, stats, gamma, beta, silu: bool, out=None, X_lo=None):
    """X_lo (accuracy mode): the apply reads the pair X + X_lo (one pitch); stats from groupnorm_stats on the hi part."""
    _f16(X, X_lo, gamma, beta)
    assert X_lo is None or _ld(X_lo) == _ld(X)
    C = X.shape[1]
    if out is None:
        out = torch.empty(X.shape[0], C, device=X.device, dtype=torch.float16)
    check(lib.skg_groupnorm_apply(_p(X), _p(X_lo), _ld(X), _p(out), _ld(out), rows, HW, C, groups, _p(stats), _p(gamma),
                                  _p(beta), int(silu), _stream()), "skg_groupnorm_apply")
    return out


def _groupnorm(X, X_lo, rows, HW, groups, eps, gamma, beta, silu, out, out_lo, partial):
    """The one-launch forms behind groupnorm / groupnorm_hilo -> (out, statistics): from the producers' partial sums (a
    GNPartial, or (GNPartial of A, channels of A, GNPartial of B) for a concatenation [A | B]), else with an own pass."""
    _f16(X, X_lo, gamma, beta, out_lo)
    C = X.shape[1]
    if out is None:
        out = torch.empty(X.shape[0], C, device=X.device, dtype=torch.float16)
    st = torch.empty(rows, groups, 2, device=X.device, dtype=torch.float32)
    if partial is None:
        check(lib.skg_groupnorm_fwd(_p(X), _p(X_lo), _ld(X), _p(out), _p(out_lo), _ld(out), rows, HW, C, groups, eps, _p(gamma),
                                    _p(beta), int(silu), _p(st), _p(_gn_scratch(rows, groups, X.device)), _stream()),
              "skg_groupnorm_fwd")
        return out, st
    pa, CA, pb = partial if isinstance(partial, tuple) else (partial, 0, None)
    assert pa.rows == rows and pa.nch == HW // 128
    assert pa.groups == groups if pb is None else (pb.rows == rows and pb.nch == pa.nch)
    check(lib.skg_groupnorm_from_partial(_p(X), _p(X_lo), _ld(X), _p(out), _p(out_lo), _ld(out), rows, HW, C, CA, groups, eps,
                                         _p(gamma), _p(beta), int(silu), _p(st), _p(pa.buf), pa.groups,
                                         None if pb is None else _p(pb.buf), 0 if pb is None else pb.groups, pa.nch, _stream()),
          "skg_groupnorm_from_partial")
    return out, st


def groupnorm(X, rows, HW, groups, eps, gamma, beta, silu: bool, out=None, partial: Optional[GNPartial] = None):
    """Forward GroupNorm.  partial=: the producer of X already left the chunk sums behind (gemm / conv3x3 with
    gn_stats= / gn_groups=): ONE launch that folds them and applies, X is read once; (GNPartial of A, channels of A, GNPartial
    of B): X = [A | B], each half written by its own producer.
    Otherwise:  Up to 32x32 maps: two launches (chunk partial sums; apply, which folds the partials itself
    and publishes the statistics) - at 64x64 the 86 chunk partials per group make the in-kernel fold dearer than the
    4.7 us finalize launch it replaces, so the three-launch path stays (measured: tools/ew_bench.py)."""
    if partial is None and HW >= 4096:
        st = groupnorm_stats(X, rows, HW, groups, eps)
        return groupnorm_apply(X, rows, HW, groups, st, gamma, beta, silu, out), st
    return _groupnorm(X, None, rows, HW, groups, eps, gamma, beta, silu, out, None, partial)


def groupnorm_hilo(X, X_lo, rows, HW, groups, eps, gamma, beta, silu: bool, out=None, want_stats=False, partial=None, out_lo=None):
    """GroupNorm(+SiLU) of the pair X + X_lo (accuracy mode): statistics from the hi part (the producer's epilogue sums when
    `partial` - a GNPartial, or (GNPartial of A, channels of A, GNPartial of B) for a concatenation - is given, else an own
    pass; small maps: one launch on the pair's sum), apply on the sum.  out_lo: the output as a pair too (pitch of `out`)."""
    assert _ld(X) == _ld(X_lo) and (out_lo is None or (out is not None and _ld(out_lo) == _ld(out)))
    out, st = _groupnorm(X, X_lo, rows, HW, groups, eps, gamma, beta, silu, out, out_lo, partial)
    return (out, st) if want_stats else out


def _layernorm(X, X_lo, gamma, beta, eps, out, want_stats):
    _f16(X, X_lo, gamma, beta)
    M, C = X.shape
    if out is None:
        out = torch.empty(M, C, device=X.device, dtype=torch.float16)
    stats = torch.empty(M, 2, device=X.device, dtype=torch.float32) if want_stats else None
    check(lib.skg_layernorm_fwd(_p(X), _p(X_lo), _ld(X), _p(out), _ld(out), M, C, _p(gamma), _p(beta), eps, _p(stats),
                                _stream()), "skg_layernorm_fwd")
    return (out, stats) if want_stats else out


def layernorm_hilo(X, X_lo, gamma, beta, eps=1e-5, out=None, want_stats=False):
    assert _ld(X) == _ld(X_lo)
    return _layernorm(X, X_lo, gamma, beta, eps, out, want_stats)


def groupnorm_bwd(X, dY, rows, HW, groups, stats, gamma, beta, silu: bool, residual=None, out=None):
    _f16(X, dY, gamma, beta, residual)
    C = X.shape[1]
    if out is None:
        out = torch.empty(X.shape[0], C, device=X.device, dtype=torch.float16)
    check(lib.skg_groupnorm_bwd(_p(X), _ld(X), _p(dY), _ld(dY), _p(out), _ld(out), _p(residual),
                                _ld(residual) if residual is not None else 0, rows, HW, C, groups, _p(stats),
                                _p(gamma), _p(beta), int(silu), _p(_gn_scratch(rows, groups, X.device)),
                                _stream()), "skg_groupnorm_bwd")
    return out


def layernorm(X, gamma, beta, eps=1e-5, out=None, want_stats=False):
    return _layernorm(X, None, gamma, beta, eps, out, want_stats)


def layernorm_bwd(X, dY, gamma, stats, residual=None, out=None):
    _f16(X, dY, gamma, residual)
    M, C = X.shape
    if out is None:
        out = torch.empty(M, C, device=X.device, dtype=torch.float16)
    check(lib.skg_layernorm_bwd(_p(X), _ld(X), _p(dY), _ld(dY), _p(out), _ld(out), _p(residual),
                                _ld(residual) if residual is not None else 0, M, C, _p(gamma), _p(stats),
                                _stream()), "skg_layernorm_bwd")
    return out


def geglu(H, out=None, interleaved: bool = False):
    _f16(H)
    M, F2 = H.shape
    F = F2 // 2
    if out is None:
        out = torch.empty(M, F, device=H.device, dtype=torch.float16)
    check(lib.skg_geglu_fwd(_p(H), _ld(H), _p(out), _ld(out), M, F, int(interleaved), _stream()), "skg_geglu_fwd")
    return out


def geglu_bwd(H, dY, out=None, interleaved: bool = False):
    _f16(H, dY)
    M, F2 = H.shape
    if out is None:
        out = torch.empty(M, F2, device=H.device, dtype=torch.float16)
    check(lib.skg_geglu_bwd(_p(H), _ld(H), _p(dY), _ld(dY), _p(out), _ld(out), M, F2 // 2, int(interleaved),
                            _stream()), "skg_geglu_bwd")
    return out


def geglu_interleave_index(F: int) -> torch.Tensor:
    """Row permutation that turns diffusers' FF1 weight [a rows (F) ; g rows (F)] into the interleaved pack:
    packed row 4t+e is a_{2t+e} for e < 2 and g_{2t+e-2} for e >= 2."""
    r = torch.arange(2 * F)
    t, e = r // 4, r % 4
    return torch.where(e < 2, 2 * t + e, F + 2 * t + (e - 2))


def transpose(X, out=None):
    _f16(X)
    M, C = X.shape
    if out is None:
        out = torch.empty(C, M, device=X.device, dtype=torch.float16)
    check(lib.skg_transpose_f16(_p(X), _ld(X), _p(out), _ld(out), M, C, _stream()), "skg_transpose_f16")
    return out


def axpby(A, B=None, out=None, alpha=1.0, beta=1.0):
    _f16(A, B)
    M, C = A.shape
    if out is None:
        out = torch.empty(M, C, device=A.device, dtype=torch.float16)
    check(lib.skg_axpby_f16(_p(A), _ld(A), _p(B), _ld(B) if B is not None else 0, _p(out), _ld(out), M, C,
                            alpha, beta, _stream()), "skg_axpby_f16")
    return out


def batch_copy(X, in_batch_rows, out, out_batch_rows, batches, rows_per_batch):
    """out[b*out_batch_rows + r] = X[b*in_batch_rows + r] for r < rows_per_batch."""
    _f16(X, out)
    check(lib.skg_batch_copy_f16(_p(X), _ld(X), in_batch_rows, _p(out), _ld(out), out_batch_rows, batches,
                                 rows_per_batch, X.shape[1], _stream()), "skg_batch_copy_f16")
    return out


def silu(X, out=None):
    _f16(X)
    M, C = X.shape
    if out is None:
        out = torch.empty(M, C, device=X.device, dtype=torch.float16)
    check(lib.skg_silu_f16(_p(X), _ld(X), _p(out), _ld(out), M, C, _stream()), "skg_silu_f16")
    return out


def quick_gelu(X, out=None):
    _f16(X)
    M, C = X.shape
    if out is None:
        out = torch.empty(M, C, device=X.device, dtype=torch.float16)
    check(lib.skg_quick_gelu_f16(_p(X), _ld(X), _p(out), _ld(out), M, C, _stream()), "skg_quick_gelu_f16")
    return out


def quick_gelu_bwd(F, dY, out=None):
    """d loss / d F of Y = quick_gelu(F) from dY; out may be dY itself."""
    _f16(F, dY, out)
    M, C = F.shape
    assert dY.shape == (M, C)
    if out is None:
        out = torch.empty(M, C, device=F.device, dtype=torch.float16)
    check(lib.skg_quick_gelu_bwd_f16(_p(F), _ld(F), _p(dY), _ld(dY), _p(out), _ld(out), M, C, _stream()),
          "skg_quick_gelu_bwd_f16")
    return out


def gelu(X, out=None):
    _f16(X)
    M, C = X.shape
    if out is None:
        out = torch.empty(M, C, device=X.device, dtype=torch.float16)
    check(lib.skg_gelu_f16(_p(X), _ld(X), _p(out), _ld(out), M, C, _stream()), "skg_gelu_f16")
    return out


def sumpool2x2(X, rows, H, W, out=None):
    """X [rows*2H*2W, C] -> [rows*H*W, C]."""
    _f16(X)
    C = X.shape[1]
    if out is None:
        out = torch.empty(rows * H * W, C, device=X.device, dtype=torch.float16)
    check(lib.skg_sumpool2x2_f16(_p(X), _ld(X), _p(out), _ld(out), rows, H, W, C, _stream()),
          "skg_sumpool2x2_f16")
    return out


def nchw_to_nhwc(X: torch.Tensor, Cpad: int, out=None):
    """float32 [rows, C, H, W] -> fp16 [rows*H*W, Cpad]."""
    assert X.is_cuda and X.dtype == torch.float32 and X.is_contiguous()
    rows, C, H, W = X.shape
    if out is None:
        out = torch.empty(rows * H * W, Cpad, device=X.device, dtype=torch.float16)
    check(lib.skg_nchw_f32_to_nhwc_f16(_p(X), _p(out), rows, C, H * W, Cpad, _stream()),
          "skg_nchw_f32_to_nhwc_f16")
    return out


def nhwc_to_nchw(X, rows: int, C: int, H: int, W: int):
    if isinstance(X, Pair):      # accuracy mode: hi + lo in fp32
        return nhwc_to_nchw(X.hi, rows, C, H, W) + nhwc_to_nchw(X.lo, rows, C, H, W)
    _f16(X)
    out = torch.empty(rows, C, H, W, device=X.device, dtype=torch.float32)
    check(lib.skg_nhwc_f16_to_nchw_f32(_p(X), _ld(X), _p(out), rows, C, H * W, _stream()),
          "skg_nhwc_f16_to_nchw_f32")
    return out


def attn_fwd(Q, K, Vt, batch, heads, Nq, Nkv, kv_stride, dh, scale, out=None, want_lse=False, causal=False,
             v_rows=False, resident_kv=False):
    """v_rows=True: `Vt` is the row-major V ([batch*kv_stride, heads*dh] view, any row pitch) instead of its transpose.
    resident_kv=True (needs v_rows): SKG_ATTN_RESIDENT_KV, the LDS-resident kernel for 81 ... 240 key slots where it is built -
    a hint, every other call runs as without it."""
    _f16(Q, K, Vt)
    assert not (causal and v_rows) and (v_rows or not resident_kv)
    if out is None:
        out = torch.empty(batch * Nq, heads * dh, device=Q.device, dtype=torch.float16)
    lse = torch.empty(batch, heads, Nq, device=Q.device, dtype=torch.float32) if want_lse else None
    check(lib.skg_attn_fwd(_p(Q), _ld(Q), _p(K), _ld(K), _p(Vt), _ld(Vt), _p(out), _ld(out), _p(lse), batch,
                           heads, Nq, Nkv, kv_stride, dh, scale, (ATTN_CAUSAL if causal else 0) | (ATTN_ROWV if v_rows else 0) | (ATTN_RESIDENT_KV if resident_kv else 0),
                           _stream()), "skg_attn_fwd")
    return (out, lse) if want_lse else out


def attn_fwd_variant(batch, heads, Nq, Nkv, kv_stride, dh, causal=False, v_rows=False, resident_kv=False):
    """skg_attn_fwd_variant: (instantiation code, queries per workgroup) of the attn_fwd call with these arguments - 1000 + QT the
    streaming kernel, 2000 + QT causal, 3000 + NT the LDS-resident kernel.  No launch, no GPU; raises SkgError where attn_fwd would."""
    qpw = ctypes.c_int(0)
    flags = (ATTN_CAUSAL if causal else 0) | (ATTN_ROWV if v_rows else 0) | (ATTN_RESIDENT_KV if resident_kv else 0)
    code = lib.skg_attn_fwd_variant(batch, heads, Nq, Nkv, kv_stride, dh, flags, ctypes.addressof(qpw))
    if code < 0:
        check(code, "skg_attn_fwd_variant")
    return code, qpw.value


def attn_bwd_delta(O, dO, batch, heads, Nq, dh):
    _f16(O, dO)
    delta = torch.empty(batch, heads, Nq, device=O.device, dtype=torch.float32)
    check(lib.skg_attn_bwd_delta(_p(O), _ld(O), _p(dO), _ld(dO), _p(delta), batch, heads, Nq, dh, _stream()),
          "skg_attn_bwd_delta")
    return delta


def attn_bwd_dq(Q, K, V, dO, lse, delta, batch, heads, Nq, Nkv, kv_stride, dh, scale, out=None):
    _f16(Q, K, V, dO)
    if out is None:
        out = torch.empty(batch * Nq, heads * dh, device=Q.device, dtype=torch.float16)
    check(lib.skg_attn_bwd_dq(_p(Q), _ld(Q), _p(K), _ld(K), _p(V), _ld(V), _p(dO), _ld(dO), None, 0,
                              _p(lse), _p(delta), None, _p(out), _ld(out), batch, heads, Nq, Nkv, kv_stride, dh,
                              scale, _stream()), "skg_attn_bwd_dq")
    return out


def attn_bwd_dq_delta(Q, K, V, dO, O, lse, batch, heads, Nq, Nkv, kv_stride, dh, scale, out=None):
    """attn_bwd_delta + attn_bwd_dq in one launch (skg_attn_bwd_dq without delta) -> (dQ, delta)."""
    _f16(Q, K, V, dO, O)
    if out is None:
        out = torch.empty(batch * Nq, heads * dh, device=Q.device, dtype=torch.float16)
    delta = torch.empty(batch, heads, Nq, device=Q.device, dtype=torch.float32)
    check(lib.skg_attn_bwd_dq(_p(Q), _ld(Q), _p(K), _ld(K), _p(V), _ld(V), _p(dO), _ld(dO), _p(O), _ld(O), _p(lse), None, _p(delta),
                              _p(out), _ld(out), batch, heads, Nq, Nkv, kv_stride, dh, scale, _stream()), "skg_attn_bwd_dq (delta prologue)")
    return out, delta


def attn_bwd_dkv(Q, K, V, dO, lse, delta, batch, heads, Nq, Nkv, dh, scale, dK=None, dV=None):
    _f16(Q, K, V, dO)
    if dK is None:
        dK = torch.empty(batch * Nkv, heads * dh, device=Q.device, dtype=torch.float16)
    if dV is None:
        dV = torch.empty(batch * Nkv, heads * dh, device=Q.device, dtype=torch.float16)
    check(lib.skg_attn_bwd_dkv(_p(Q), _ld(Q), _p(K), _ld(K), _p(V), _ld(V), _p(dO), _ld(dO),
                               _p(lse), _p(delta), _p(dK), _ld(dK), _p(dV), _ld(dV), batch,
                               heads, Nq, Nkv, Nkv, dh, scale, _stream()), "skg_attn_bwd_dkv")
    return dK, dV


def attn_bwd_dkv_strided(Q, K, V, dO, lse, delta, batch, heads, Nq, Nkv, kv_stride, dh, scale, dK, dV):
    """attn_bwd_dkv on a padded K / V buffer: rows of batch row b start at b * kv_stride; rows Nkv .. kv_stride - 1 of
    dK / dV (views of [batch * kv_stride, >= heads * dh] buffers) are left untouched."""
    _f16(Q, K, V, dO, dK, dV)
    assert kv_stride >= Nkv and dK.shape[0] >= (batch - 1) * kv_stride + Nkv and dV.shape[0] >= (batch - 1) * kv_stride + Nkv
    assert K.shape[0] >= (batch - 1) * kv_stride + Nkv and V.shape[0] >= (batch - 1) * kv_stride + Nkv
    check(lib.skg_attn_bwd_dkv(_p(Q), _ld(Q), _p(K), _ld(K), _p(V), _ld(V), _p(dO), _ld(dO),
                               _p(lse), _p(delta), _p(dK), _ld(dK), _p(dV), _ld(dV), batch,
                               heads, Nq, Nkv, kv_stride, dh, scale, _stream()), "skg_attn_bwd_dkv (strided)")
    return dK, dV


# ---- LGP --------------------------------------------------------------------------------------------
def lgp_layer0_gather(P: Sequence[torch.Tensor], sizes: Sequence[int], Wextra, bias0, noise, sigma: float,
                      samples: int, h: int, H0: int, out=None, rows: Optional[int] = None, w: Optional[int] = None):
    """rows defaults to 2*samples ([uncond ; cond] blocks of the sampler); the trainer passes rows = samples.
    w: the grid's width when it is not square (sizes are the taps' heights, a tap of height s is s * w // h wide)."""
    rows = 2 * samples if rows is None else rows
    wd = h if w is None else w
    arr = (SkgTap * len(P))()
    for i, (t, s) in enumerate(zip(P, sizes)):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.shape == (rows * s * (s * wd // h), H0)
        arr[i].P, arr[i].s = t.data_ptr(), s
    if out is None:
        out = torch.empty(rows * h * wd, H0, device=noise.device, dtype=torch.float16)
    check(lib.skg_lgp_layer0_gather(ctypes.addressof(arr), len(P), _p(Wextra), _ld(Wextra) if Wextra is not None else 0, _p(bias0),
                                    _p(noise), sigma, samples, _p(out), rows, h, wd, H0, _stream()), "skg_lgp_layer0_gather")
    return out


def lgp_layer0_scatter(dZ, rows, h, s, H0, w: Optional[int] = None):
    """-> dP [rows * s * sw, H0] of the tap of height s (sw = s * w // h, w defaults to h)."""
    _f16(dZ)
    if s == h and dZ.stride(0) == H0:          # the adjoint of an identity resize: no copy
        return dZ
    wd = h if w is None else w
    out = torch.empty(rows * s * (s * wd // h), H0, device=dZ.device, dtype=torch.float16)
    check(lib.skg_lgp_layer0_scatter(_p(dZ), _ld(dZ), _p(out), rows, h, wd, s, H0, _stream()), "skg_lgp_layer0_scatter")
    return out


def _bn_scratch(samples, C, dev):
    n = lib.skg_bn_scratch_floats(samples, C)
    return _scratch_buf(("bn", _skey(dev), n), n, dev)


def bn_stats(X, samples, segs, seg_rows, eps=1e-5, running_mean=None, running_var=None):
    _f16(X)
    C = X.shape[1]
    stats = torch.empty(samples, C, 2, device=X.device, dtype=torch.float32)
    check(lib.skg_bn_stats(_p(X), _ld(X), samples, segs, seg_rows, C, eps, _p(stats),
                           _p(_bn_scratch(samples, C, X.device)), _p(running_mean), _p(running_var), _stream()),
          "skg_bn_stats")
    return stats


def bn_stats_from_running(running_mean, running_var, samples, eps=1e-5):
    C = running_mean.numel()
    stats = torch.empty(samples, C, 2, device=running_mean.device, dtype=torch.float32)
    check(lib.skg_bn_stats_from_running(_p(running_mean), _p(running_var), samples, C, eps, _p(stats), _stream()),
          "skg_bn_stats_from_running")
    return stats


def bn_apply(X, samples, segs, seg_rows, stats, gamma, beta, out=None):
    _f16(X, gamma, beta)
    C = X.shape[1]
    if out is None:
        out = torch.empty(X.shape[0], C, device=X.device, dtype=torch.float16)
    check(lib.skg_bn_apply(_p(X), _ld(X), _p(out), _ld(out), samples, segs, seg_rows, C, _p(stats), _p(gamma),
                           _p(beta), _stream()), "skg_bn_apply")
    return out


def bn_relu_bwd(X, dY, samples, segs, seg_rows, stats, gamma, train: bool, out=None):
    _f16(X, dY, gamma)
    C = X.shape[1]
    if out is None:
        out = torch.empty(X.shape[0], C, device=X.device, dtype=torch.float16)
    check(lib.skg_bn_relu_bwd(_p(X), _ld(X), _p(dY), _ld(dY), _p(out), _ld(out), samples, segs, seg_rows, C,
                              _p(stats), _p(gamma), int(train), _p(_bn_scratch(samples, C, X.device)), _stream()),
          "skg_bn_relu_bwd")
    return out


def lgp_mse_seed(out16, target, samples, h, ldd, loss_scale, w: Optional[int] = None):
    _f16(out16)
    wd = h if w is None else w
    dOut = torch.empty(2 * samples * h * wd, ldd, device=out16.device, dtype=torch.float16)
    loss = torch.empty(samples, device=out16.device, dtype=torch.float32)
    check(lib.skg_lgp_mse_seed(_p(out16), _ld(out16), _p(target), _p(dOut), ldd, _p(loss), samples, h, wd,
                               loss_scale, _stream()), "skg_lgp_mse_seed")
    return dOut, loss


# ---- LGP training ------------------------------------------------------------------------------------
def colsum(X, scale: float = 1.0):
    _f16(X)
    M, C = X.shape
    out = torch.empty(C, device=X.device, dtype=torch.float32)
    scr = _scratch_buf(("colsum", _skey(X.device), C), lib.skg_colsum_scratch_floats(C), X.device)
    check(lib.skg_colsum_f16(_p(X), _ld(X), M, C, scale, _p(out), _p(scr), _stream()), "skg_colsum_f16")
    return out


def bn_param_grads(X, dY, stats, scale: float = 1.0):
    """(dgamma, dbeta) of one BatchNorm1d batch = all rows of X; stats [1, C, 2] from bn_stats(samples=1)."""
    _f16(X, dY)
    M, C = X.shape
    dg = torch.empty(C, device=X.device, dtype=torch.float32)
    db = torch.empty(C, device=X.device, dtype=torch.float32)
    check(lib.skg_bn_param_grads(_p(X), _ld(X), _p(dY), _ld(dY), M, C, _p(stats), scale, _p(dg), _p(db),
                                 _p(_bn_scratch(1, C, X.device)), _stream()), "skg_bn_param_grads")
    return dg, db


def lgp_extra_features(noise, sigma: float, samples: int, rows: int, h: int, ld: int = 64, w: Optional[int] = None):
    wd = h if w is None else w
    out = torch.empty(rows * h * wd, ld, device=noise.device, dtype=torch.float16)
    check(lib.skg_lgp_extra_features(_p(noise), sigma, samples, rows, h, wd, _p(out), ld, _stream()),
          "skg_lgp_extra_features")
    return out


def lgp_mse_train(out16, target, samples, h, ldd, loss_scale):
    _f16(out16)
    dOut = torch.empty(samples * h * h, ldd, device=out16.device, dtype=torch.float16)
    parts = torch.empty(samples, device=out16.device, dtype=torch.float32)
    check(lib.skg_lgp_mse_train(_p(out16), _ld(out16), _p(target), _p(dOut), ldd, _p(parts), samples, h, loss_scale,
                                _stream()), "skg_lgp_mse_train")
    return dOut, parts


def adamw_step(param, grad, exp_avg, exp_avg_sq, param_f16, lr, beta1, beta2, eps, weight_decay, step: int,
               inv_grad_scale: float = 1.0):
    n = param.numel()
    assert param.dtype == grad.dtype == exp_avg.dtype == exp_avg_sq.dtype == torch.float32 and grad.numel() == n
    check(lib.skg_adamw_step(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), _p(param_f16), n, lr, beta1, beta2,
                             eps, weight_decay, step, inv_grad_scale, _stream()), "skg_adamw_step")


def adamw_step_guarded(param, grad, exp_avg, exp_avg_sq, param_f16, lr, beta1, beta2, eps, weight_decay, step: int,
                       inv_grad_scale: float, skip_flag):
    """adamw_step behind a one-float device flag (nonfinite_flag's): non-zero -> nothing is touched, zero -> adamw_step's bits."""
    n = param.numel()
    assert param.dtype == grad.dtype == exp_avg.dtype == exp_avg_sq.dtype == skip_flag.dtype == torch.float32
    assert grad.numel() == n and skip_flag.numel() == 1
    check(lib.skg_adamw_step_guarded(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), _p(param_f16), n, lr, beta1, beta2,
                                     eps, weight_decay, step, inv_grad_scale, _p(skip_flag), _stream()), "skg_adamw_step_guarded")


def adamw8_step(param, grad, param_f16, state1, state2, absmax1, absmax2, exp_avg32, exp_avg_sq32, rows, qtab, lr, beta1, beta2,
                eps, weight_decay, step: int, inv_grad_scale: float = 1.0, skip_flag=None):
    """One AdamW step on block-wise quantised 8-bit moments (skg_adamw8_step; flat_adamw.FlatAdamW builds every operand): rows is
    the int64 [R, 4] block table (offset, length <= 2048, state offset, 8-bit or fp32), state1 / state2 the uint8 codes, absmax1 /
    absmax2 one float per row, exp_avg32 / exp_avg_sq32 the compact fp32 moments of the small tensors, qtab the 4 x 256 maps and
    thresholds.  skip_flag (nonfinite_flag's float): non-zero -> nothing is touched."""
    n, R = param.numel(), rows.shape[0]
    assert param.dtype == grad.dtype == absmax1.dtype == absmax2.dtype == exp_avg32.dtype == exp_avg_sq32.dtype == torch.float32
    assert qtab.dtype == torch.float32 and qtab.numel() == 1024 and qtab.is_contiguous() and grad.numel() == n
    assert state1.dtype == state2.dtype == torch.uint8 and state1.numel() == state2.numel()
    assert rows.dtype == torch.int64 and rows.dim() == 2 and rows.shape[1] == 4 and rows.is_contiguous()
    assert absmax1.numel() == absmax2.numel() == max(R, 1) and exp_avg32.numel() == exp_avg_sq32.numel()
    assert param_f16 is None or (param_f16.dtype == torch.float16 and param_f16.numel() == n)
    assert skip_flag is None or (skip_flag.dtype == torch.float32 and skip_flag.numel() == 1)
    check(lib.skg_adamw8_step(_p(param), _p(grad), _p(param_f16), _p(state1), _p(state2), _p(absmax1), _p(absmax2), _p(exp_avg32),
                              _p(exp_avg_sq32), _p(rows), R, _p(qtab), lr, beta1, beta2, eps, weight_decay, step, inv_grad_scale,
                              _p(skip_flag), _stream()), "skg_adamw8_step")


def nonfinite_flag(x, flag, reset: bool = False):
    """flag (one fp32 element on x's device) = 1.0 if the dense fp32 tensor x holds an inf or a NaN, else untouched; reset zeroes
    it first.  Queued on the current stream: nothing waits."""
    assert x.dtype == flag.dtype == torch.float32 and x.is_contiguous() and flag.numel() == 1 and x.numel() > 0
    check(lib.skg_nonfinite_flag(_p(x), x.numel(), _p(flag), int(bool(reset)), _stream()), "skg_nonfinite_flag")


# ---- injected-attention training (sat_train.py) ---------------------------------------------------------
def wgrad(dY, X, dW=None, db=None, alpha: float = 1.0, accumulate: bool = False, want_db: bool = False):
    """dW [N, K] fp32 = or += alpha * dY^T . X (dY [M, N], X [M, K]: fp16 row-major views, contraction over the rows) and,
    when db is given or want_db is set, db [N] fp32 = or += alpha * colsum(dY) in the same pass (skg_wgrad_f16: no
    transposed copies, fixed-order reduction).  dW / db must be dense; returns dW or (dW, db)."""
    _f16(dY, X)
    M, N = dY.shape
    K = X.shape[1]
    assert X.shape[0] == M
    if dW is None:
        assert not accumulate
        dW = torch.empty(N, K, device=dY.device, dtype=torch.float32)
    if db is None and want_db:
        assert not accumulate
        db = torch.empty(N, device=dY.device, dtype=torch.float32)
    assert dW.dtype == torch.float32 and dW.is_contiguous() and dW.numel() == N * K
    assert db is None or (db.dtype == torch.float32 and db.is_contiguous() and db.numel() == N)
    n = lib.skg_wgrad_scratch_floats(M, N, K)
    scr = _scratch_buf(("wgrad", _skey(dY.device), n), n, dY.device)
    check(lib.skg_wgrad_f16(_p(dY), _ld(dY), _p(X), _ld(X), M, N, K, alpha, int(accumulate), _p(dW), _p(db), _p(scr),
                            _stream()), "skg_wgrad_f16")
    return dW if db is None else (dW, db)


def layernorm_param_grads(X, dY, stats, dgamma=None, dbeta=None, scale: float = 1.0, accumulate: bool = False):
    """(dgamma, dbeta) [C] fp32 = or += scale * (sum_rows dY * xhat, sum_rows dY); stats [M, 2] from layernorm(want_stats=True)."""
    _f16(X, dY)
    M, C = X.shape
    assert dY.shape == (M, C) and stats.dtype == torch.float32 and stats.is_contiguous() and stats.numel() == 2 * M
    if dgamma is None:
        assert not accumulate
        dgamma = torch.empty(C, device=X.device, dtype=torch.float32)
        dbeta = torch.empty(C, device=X.device, dtype=torch.float32)
    for t in (dgamma, dbeta):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == C
    n = lib.skg_layernorm_param_scratch_floats(C)
    scr = _scratch_buf(("lnp", _skey(X.device), n), n, X.device)
    check(lib.skg_layernorm_param_grads(_p(X), _ld(X), _p(dY), _ld(dY), M, C, _p(stats), scale, int(accumulate),
                                        _p(dgamma), _p(dbeta), _p(scr), _stream()), "skg_layernorm_param_grads")
    return dgamma, dbeta


# ---- sampler ------------------------------------------------------------------------------------------
def softmax_rows(X, out=None):
    """Row softmax of fp16 scores (fp32 arithmetic); in place when out is X."""
    _f16(X)
    M, N = X.shape
    if out is None:
        out = torch.empty(M, N, device=X.device, dtype=torch.float16)
    check(lib.skg_softmax_rows_f16(_p(X), _ld(X), _p(out), _ld(out), M, N, _stream()), "skg_softmax_rows_f16")
    return out


def image_postprocess(X, pixels: int, C: int, scale: float = 0.5, shift: float = 0.5):
    """fp16 NHWC rows (first C channels of pitch ld) -> float [pixels, C] = clamp(x*scale + shift, 0, 1)."""
    _f16(X)
    out = torch.empty(pixels, C, device=X.device, dtype=torch.float32)
    check(lib.skg_image_postprocess(_p(X), _ld(X), _p(out), pixels, C, scale, shift, _stream()),
          "skg_image_postprocess")
    return out


def image_to_u8(X, pixels: int, C: int, scale: float = 0.5, shift: float = 0.5):
    """fp16 NHWC rows -> uint8 [pixels, C] = rint(clamp(x*scale + shift, 0, 1) * 255) (numpy_to_pil's quantisation)."""
    _f16(X)
    out = torch.empty(pixels, C, device=X.device, dtype=torch.uint8)
    check(lib.skg_image_to_u8(_p(X), _ld(X), _p(out), pixels, C, scale, shift, _stream()), "skg_image_to_u8")
    return out


def gaussian_sample(moments, samples: int, L: int, HW: int, noise=None, scale: float = 1.0):
    """(mean + exp(0.5*clamp(logvar))*noise)*scale from fp16 NHWC moments [samples*HW, >=2L] -> float [samples, L, HW]."""
    _f16(moments)
    out = torch.empty(samples, L, HW, device=moments.device, dtype=torch.float32)
    check(lib.skg_gaussian_sample(_p(moments), _ld(moments), _p(noise), _p(out), samples, L, HW, scale, _stream()),
          "skg_gaussian_sample")
    return out


def eps_halves(eps, samples, HW):
    """(uncond rows, cond rows, pair offset) of the UNet's eps for cfg_*_step: fp16 [2 S HW, >= 4], or - accuracy mode - a
    Pair whose lo part sits a fixed number of columns to the right of the hi part in the same buffer."""
    if isinstance(eps, Pair):
        off = (eps.lo.data_ptr() - eps.hi.data_ptr()) // 2
        assert _ld(eps.hi) == _ld(eps.lo) and 0 < off <= _ld(eps.hi) - 4
        return eps.hi[:samples * HW], eps.hi[samples * HW:], off
    return eps[:samples * HW], eps[samples * HW:], 0


def cfg_ddim_step(eps_u, eps_c, x, samples, HW, g, coeffs: Tuple[float, float, float, float],
                  want_eps=False, lo_off: int = 0, v_prediction: bool = False):
    """lo_off != 0: eps_u / eps_c are the hi parts of pairs whose lo parts sit lo_off columns to the right (eps_halves).
    v_prediction: the model output is v (eps = c0 v + c1 x, x0 = c0 x - c1 v); the returned eps is the derived one."""
    _f16(eps_u, eps_c)
    x_prev = torch.empty_like(x)
    eps_out = torch.empty_like(x) if want_eps else None
    c0, c1, c2, c3 = coeffs
    check(lib.skg_cfg_ddim_step(_p(eps_u), _p(eps_c), _ld(eps_u), lo_off, _p(x), _p(x_prev), _p(eps_out), samples, HW,
                                g, c0, c1, c2, c3, int(bool(v_prediction)), _stream()), "skg_cfg_ddim_step")
    return (x_prev, eps_out) if want_eps else x_prev


def cfg_ddim_eta_step(eps_u, eps_c, x, z, samples, HW, g, coeffs: Tuple[float, float, float, float, float],
                      want_eps=False, lo_off: int = 0, v_prediction: bool = False):
    """cfg_ddim_step with DDIM's noise term: coeffs = DDIMTables.coeffs_eta(t, eta) = (c0, c1, c2, c_dir, sigma),
    x_prev = c2 x0 + c_dir eps + sigma z.  z: N(0, 1) drawn by the caller, fp32 and contiguous in x's shape."""
    _f16(eps_u, eps_c)
    assert z is not None and z.is_cuda and z.dtype == torch.float32 and z.is_contiguous() and z.shape == x.shape, \
        "z: contiguous fp32 CUDA tensor of the latents' shape"
    x_prev = torch.empty_like(x)
    eps_out = torch.empty_like(x) if want_eps else None
    c0, c1, c2, c_dir, sigma = coeffs
    check(lib.skg_cfg_ddim_eta_step(_p(eps_u), _p(eps_c), _ld(eps_u), lo_off, _p(x), _p(z), _p(x_prev), _p(eps_out), samples, HW,
                                    g, c0, c1, c2, c_dir, sigma, int(bool(v_prediction)), _stream()), "skg_cfg_ddim_eta_step")
    return (x_prev, eps_out) if want_eps else x_prev


def cfg_dpmpp2m_step(eps_u, eps_c, x, x0_io, samples, HW, g, coeffs: Tuple[float, float, float, float, float],
                     want_eps=False, lo_off: int = 0, v_prediction: bool = False):
    """coeffs = (alpha_s, sigma_s, a, b, c); x0_io is updated in place (previous x0 in, this step's x0 out)."""
    _f16(eps_u, eps_c)
    x_prev = torch.empty_like(x)
    eps_out = torch.empty_like(x) if want_eps else None
    al, sg, a, b, c = coeffs
    check(lib.skg_cfg_dpmpp2m_step(_p(eps_u), _p(eps_c), _ld(eps_u), lo_off, _p(x), _p(x0_io), _p(x_prev), _p(eps_out),
                                   samples, HW, g, al, sg, a, b, c, int(bool(v_prediction)), _stream()), "skg_cfg_dpmpp2m_step")
    return (x_prev, eps_out) if want_eps else x_prev


def cfg_dpmpp2m_sde_step(eps_u, eps_c, x, z, x0_io, samples, HW, g, coeffs: Tuple[float, float, float, float, float, float],
                         want_eps=False, lo_off: int = 0, v_prediction: bool = False):
    """cfg_dpmpp2m_step with the stochastic solver's noise term: coeffs = DPMTables.coeffs_sde(i, order) = (alpha_s, sigma_s, a, b,
    c, d), x_prev = a x + b x0 + c x0_before + d z.  z: N(0, 1) drawn by the caller, fp32 and contiguous in x's shape."""
    _f16(eps_u, eps_c)
    assert z is not None and z.is_cuda and z.dtype == torch.float32 and z.is_contiguous() and z.shape == x.shape, \
        "z: contiguous fp32 CUDA tensor of the latents' shape"
    x_prev = torch.empty_like(x)
    eps_out = torch.empty_like(x) if want_eps else None
    al, sg, a, b, c, d = coeffs
    check(lib.skg_cfg_dpmpp2m_sde_step(_p(eps_u), _p(eps_c), _ld(eps_u), lo_off, _p(x), _p(z), _p(x0_io), _p(x_prev), _p(eps_out),
                                       samples, HW, g, al, sg, a, b, c, d, int(bool(v_prediction)), _stream()),
          "skg_cfg_dpmpp2m_sde_step")
    return (x_prev, eps_out) if want_eps else x_prev


def model_input(x: torch.Tensor, c_in: float, Cpad: int, dup: int = 1, want_scaled: bool = False):
    """The UNet operand of a sigma-space step: float32 [S, C, H, W] -> fp16 [dup*S*H*W, Cpad] = half(c_in * x), dup = 2 stacking the
    CFG twin, and - want_scaled - the fp32 product [S, C, H, W] itself.  Returns (operand, scaled or None)."""
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 4 and dup in (1, 2)
    S, C, H, W = x.shape
    out = torch.empty(dup * S * H * W, Cpad, device=x.device, dtype=torch.float16)
    scaled = torch.empty_like(x) if want_scaled else None
    check(lib.skg_model_input(_p(x), _p(out), _p(scaled), S, C, H * W, Cpad, dup, c_in, _stream()), "skg_model_input")
    return out, scaled


def cfg_euler_step(eps_u, eps_c, x, z, samples, HW, g, coeffs: Tuple[float, float, float, float, float], want_eps=False,
                   lo_off: int = 0):
    """CFG combine + one Euler (z None) or Euler-ancestral step: coeffs = EulerTables.coeffs(i) = (sigma, k_x, k_m, dt, sigma_up),
    x0 = k_x x + k_m m, d = (x - x0)/sigma, x_prev = x + dt d + sigma_up z.  z: N(0, 1) drawn by the caller, fp32 and contiguous in
    x's shape; the prediction type is in k_x and k_m.  The returned eps is d."""
    _f16(eps_u, eps_c)
    assert z is None or (z.is_cuda and z.dtype == torch.float32 and z.is_contiguous() and z.shape == x.shape), \
        "z: contiguous fp32 CUDA tensor of the latents' shape"
    x_prev = torch.empty_like(x)
    eps_out = torch.empty_like(x) if want_eps else None
    sigma, k_x, k_m, dt, sigma_up = coeffs
    check(lib.skg_cfg_euler_step(_p(eps_u), _p(eps_c), _ld(eps_u), lo_off, _p(x), _p(z), _p(x_prev), _p(eps_out), samples, HW, g,
                                 sigma, k_x, k_m, dt, sigma_up, _stream()), "skg_cfg_euler_step")
    return (x_prev, eps_out) if want_eps else x_prev


def guidance_update(grad, x_in, x_prev, samples, HW, beta):
    """In place: x_prev += alpha * (-grad).  Returns aux [samples,4] = (alpha, ||g||, sqrt2*||dx||, 0)."""
    _f16(grad)
    aux = torch.empty(samples, 4, device=grad.device, dtype=torch.float32)
    check(lib.skg_guidance_update(_p(grad), _ld(grad), _p(x_in), _p(x_prev), _p(aux), samples, HW, beta,
                                  _stream()), "skg_guidance_update")
    return aux


def latent_renoise(init, noise, a: float, s: float, x=None, mask=None):
    """r = a*init + s*noise on fp32 latents [S, 4, h, w] (scheduler.add_noise at the schedule level (a, s)).  Without a mask: x = r,
    x allocated when None.  With a mask - fp32 [1 or S, 1, h, w], 1 = repaint, 0 = keep - x is updated in place:
    x = m*x + (1 - m)*r.  Returns x."""
    chk = lambda t, what: (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(), f"{what}: contiguous fp32 CUDA tensor")
    for t, what in ((init, "init"), (noise, "noise")):
        ok, msg = chk(t, what)
        assert ok and t.dim() == 4 and t.shape[1] == 4 and t.shape == init.shape, msg + " [S, 4, h, w]"
    S, _, h, w = init.shape
    if x is None:
        assert mask is None, "latent_renoise: the masked blend updates x in place and needs it"
        x = torch.empty_like(init)
    ok, msg = chk(x, "x")
    assert ok and x.shape == init.shape, msg + " of init's shape"
    ms = 0
    if mask is not None:
        ok, msg = chk(mask, "mask")
        assert ok and mask.dim() == 4 and tuple(mask.shape[1:]) == (1, h, w), msg + f" [1 or S, 1, {h}, {w}], got {tuple(mask.shape)}"
        ms = mask.shape[0]
    check(lib.skg_latent_renoise(_p(init), _p(noise), _p(mask), ms, _p(x), S, h * w, a, s, _stream()), "skg_latent_renoise")
    return x


# ---- sketch generator (anime2sketch.py) ------------------------------------------------------------------------------------
CONVT_EPI_NONE, CONVT_EPI_TANH = 0, 1


def instnorm_act(X: torch.Tensor, rows: int, HW: int, out0: Optional[torch.Tensor] = None, slope0: float = 1.0,
                 out1: Optional[torch.Tensor] = None, slope1: float = 0.0, *, eps: float = 1e-5, identity: bool = False):
    """InstanceNorm2d(affine=False) of X [rows*HW, C] (view) with up to two activated outputs (views, e.g. the skip half of a
    concatenation buffer): out_k = act_k(norm(X)), act(v) = v if v >= 0 else slope * v.  identity=True: no statistics."""
    _f16(X, out0, out1)
    C = X.shape[1]
    assert X.shape[0] == rows * HW and all(o is None or o.shape == X.shape for o in (out0, out1))
    n = 0 if identity else lib.skg_instnorm_scratch_floats(rows, HW, C)
    scratch = _scratch_buf(("in", _skey(X.device), n), n, X.device) if n else None
    check(lib.skg_instnorm_act_f16(_p(X), _ld(X), rows, HW, C, eps, int(identity), _p(out0), _ld(out0) if out0 is not None else 0, slope0,
                                   _p(out1), _ld(out1) if out1 is not None else 0, slope1, _p(scratch), _stream()), "skg_instnorm_act_f16")
    return out0, out1


def convt4x4s2(X: torch.Tensor, Wpp: torch.Tensor, rows: int, IH: int, IW: int, out: Optional[torch.Tensor] = None, *, bias=None,
               tanh: bool = False):
    """ConvTranspose2d(4, stride 2, padding 1), polyphase.  X [rows*IH*IW, Cin] (view), Wpp [4, Cout, 4*Cin]
    (anime2sketch.pack_convt).  Returns [rows*2IH*2IW, Cout]; tanh=True applies tanh to it."""
    _f16(X, Wpp, bias, out)
    Cin, Cout = X.shape[1], Wpp.shape[1]
    assert Wpp.shape == (4, Cout, 4 * Cin) and Wpp.is_contiguous() and X.shape[0] == rows * IH * IW
    if out is None:
        out = torch.empty(rows * 4 * IH * IW, Cout, device=X.device, dtype=torch.float16)
    assert out.shape == (rows * 4 * IH * IW, Cout)
    check(lib.skg_convt4x4s2_f16(_p(X), _ld(X), _p(Wpp), _p(out), _ld(out), rows, IH, IW, Cin, Cout, _p(bias),
                                 CONVT_EPI_TANH if tanh else CONVT_EPI_NONE, _stream()), "skg_convt4x4s2_f16")
    return out


def a2s_patch(img: torch.Tensor, out: Optional[torch.Tensor] = None):
    """float32 [B, 3, H, W] -> fp16 [B*(H/2)*(W/2), 64]: the 4 x 4 stride-2 windows (column (ky*4+kx)*3 + c, 48..63 zero)."""
    assert img.is_cuda and img.dtype == torch.float32 and img.is_contiguous() and img.shape[1] == 3
    B, _, H, W = img.shape
    if out is None:
        out = torch.empty(B * (H // 2) * (W // 2), 64, device=img.device, dtype=torch.float16)
    _f16(out)
    assert out.shape == (B * (H // 2) * (W // 2), 64)
    check(lib.skg_a2s_patch_f16(_p(img), _p(out), _ld(out), B, H, W, _stream()), "skg_a2s_patch_f16")
    return out


def a2s_tail(Y: torch.Tensor, B: int, H: int, W: int, y: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None):
    """Column 0 of Y [B*H*W, >= 1] (fp16) -> y float [B, 1, H, W] and / or mask float [B, 3, H, W] = (1 - y >= 0.5), whichever is given."""
    _f16(Y)
    assert Y.shape[0] == B * H * W and (y is not None or mask is not None)
    for t, c in ((y, 1), (mask, 3)):
        assert t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.shape == (B, c, H, W))
    check(lib.skg_a2s_tail(_p(Y), Y.stride(0), _p(y), _p(mask), B, H, W, _stream()), "skg_a2s_tail")
    return y, mask
