"""numpy restatement of the 8-bit AdamW state (block-wise dynamic quantisation after Dettmers et al., "8-bit Optimizers via Block-wise
Quantization", as DESIGN.md section 15 fixes it), shared by tests/test_host_adamw8bit.py and tests/test_gpu_adamw8bit.py.  Written from
that definition, independent of sketch2img_amd.flat_adamw and of the kernel: the checker of both files.  bitsandbytes itself is not
involved anywhere."""
import numpy as np

BLOCK = 2048
ZERO1, ZERO2 = 127, 0
f32 = np.float32


def maps():
    """-> (signed [256], unsigned [256]) fp32, ascending.  Decade i = 0 ... 6: the midpoints of k equal-width cells on [0.1, 1] times
    10^(i - 6); k = 2^i and both signs (signed), k = 2^(i + 1) (unsigned); plus 0 and 1.  Each value is
    (0.1 + 0.9 * (j + 0.5) / k) / 10^(6 - i), evaluated in this order in float64, rounded once to fp32."""
    def pos(shift):
        out = []
        for i in range(7):
            k = 1 << (i + shift)
            out += [(0.1 + 0.9 * (j + 0.5) / k) / 10.0 ** (6 - i) for j in range(k)]
        return out
    s = pos(0)
    signed = np.sort(np.array([-x for x in s] + [0.0] + s + [1.0], dtype=np.float64)).astype(f32)
    unsigned = np.sort(np.array([0.0] + pos(1) + [1.0], dtype=np.float64)).astype(f32)
    return signed, unsigned


def thresholds(q):
    """mid[j] = 0.5f * (q[j] + q[j + 1]), j = 0 ... 254, in fp32."""
    return (f32(0.5) * (q[:-1] + q[1:])).astype(f32)


def quantise(s, q, zero):
    """One tensor's fp32 values (flat) -> (codes uint8 [n], absmax fp32 [blocks]): per block of at most 2048 elements counted from
    the first, a = max |s| exact; a == 0 -> the zero code; else x = s / a (correctly rounded fp32), code = #{ j : mid[j] < x }."""
    s = np.ascontiguousarray(s, dtype=f32).reshape(-1)
    mid = thresholds(q)
    codes = np.empty(s.size, dtype=np.uint8)
    absmax = np.empty((s.size + BLOCK - 1) // BLOCK, dtype=f32)
    for b in range(absmax.size):
        blk = s[b * BLOCK:(b + 1) * BLOCK]
        a = np.max(np.abs(blk))
        absmax[b] = a
        if a == 0:
            codes[b * BLOCK:(b + 1) * BLOCK] = zero
        else:
            x = (blk / a).astype(f32)
            codes[b * BLOCK:(b + 1) * BLOCK] = np.searchsorted(mid, x, side="left")       # = #{ j : mid[j] < x }
    return codes, absmax


def dequantise(codes, absmax, q):
    """s = q[code] * absmax of the element's block: one fp32 multiply."""
    codes = np.asarray(codes).reshape(-1)
    return (q[codes] * np.repeat(absmax, BLOCK)[:codes.size]).astype(f32)


def _fma(a, b, c):
    """fp32 fma through float64: the product of two fp32 is exact there; the sum is rounded to 53 bits and then to 24 (off from a true
    fma only on a double-rounding tie)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def moments(g, m, v, b1, b2, inv_scale, fused=True):
    """m', v' of one AdamW step on fp32 arrays: gi = g * inv_scale; m' = b1 m + (1 - b1) gi; v' = b2 v + ((1 - b2) gi) gi, every
    operation in fp32, the outer multiply-add fused (the kernel's form) or not."""
    b1, b2 = f32(b1), f32(b2)
    gi = (np.asarray(g, f32) * f32(inv_scale)).astype(f32)
    t1 = ((f32(1) - b1) * gi).astype(f32)
    t2 = (gi * ((f32(1) - b2) * gi).astype(f32)).astype(f32)
    if fused:
        return _fma(b1, m, t1), _fma(b2, v, t2)
    return ((b1 * m).astype(f32) + t1).astype(f32), ((b2 * v).astype(f32) + t2).astype(f32)


def update(p, m1, v1, lr, b1, b2, eps, wd, step):
    """The new master weights from the FRESH fp32 moments: p (1 - lr wd) - (lr (m' / bc1)) / (sqrt(v' / bc2) + eps) in fp32."""
    lr, eps, wd = f32(lr), f32(eps), f32(wd)
    bc1 = f32(1) - np.power(f32(b1), f32(step), dtype=f32)
    bc2 = f32(1) - np.power(f32(b2), f32(step), dtype=f32)
    decay = _fma(-lr, wd, f32(1))
    upd = ((lr * (m1 / bc1).astype(f32)).astype(f32) / (np.sqrt((v1 / bc2).astype(f32)).astype(f32) + eps).astype(f32)).astype(f32)
    return _fma(decay, p, -upd)


class Adam8:
    """AdamW with 8-bit state over a list of flat fp32 tensors; tensors below min_8bit_size keep fp32 moments."""

    def __init__(self, params, lr, betas, eps, wd, min_8bit_size=4096):
        self.q1, self.q2 = maps()
        self.p = [np.array(x, dtype=f32).reshape(-1) for x in params]
        self.hyper = (lr, betas[0], betas[1], eps, wd)
        self.step_count = 0
        self.is8 = [x.size >= min_8bit_size for x in self.p]
        self.state = [(quantise(np.zeros_like(x), self.q1, ZERO1), quantise(np.zeros_like(x), self.q2, ZERO2)) if e
                      else (np.zeros_like(x), np.zeros_like(x)) for x, e in zip(self.p, self.is8)]

    def old_moments(self, i):
        a, b = self.state[i]
        return (dequantise(*a, self.q1), dequantise(*b, self.q2)) if self.is8[i] else (a, b)

    def step(self, grads, inv_scale=1.0):
        lr, b1, b2, eps, wd = self.hyper
        self.step_count += 1
        for i, g in enumerate(grads):
            m, v = self.old_moments(i)
            m1, v1 = moments(g, m, v, b1, b2, inv_scale)
            self.p[i] = update(self.p[i], m1, v1, lr, b1, b2, eps, wd, self.step_count)
            self.state[i] = (quantise(m1, self.q1, ZERO1), quantise(v1, self.q2, ZERO2)) if self.is8[i] else (m1, v1)


# the mixed layout both test files use: at, just above and well above min_8bit_size = 4096, a short last block (5, 1808 and 1
# elements), a tensor one element short of 8-bit, sizes that leave 7, 4 and 3 padding elements behind them, and a frozen key listed
# in the middle (laid out last, no rows)
MIXED = [("w4096", (64, 64)), ("w4097", (4097,)), ("frozen", (2050,)), ("w6149", (3 * 2048 + 5,)), ("w10000", (100, 100)),
         ("w4095", (4095,)), ("b8", (8,)), ("b1", (1,))]
