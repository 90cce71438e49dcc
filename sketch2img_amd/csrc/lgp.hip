// LGP (Latent Gradient/Edge Predictor) kernels: re-associated layer 0 (bilinear gather of per-tap
// partial products + noise-level / sinusoid channels), its adjoint, per-sample train-mode
// BatchNorm1d (stats / apply / backward through the preceding ReLU) and the MSE seed gradient.
//
// Row layout of every LGP activation: row = (j * S + s) * hw + pixel with j = CFG half (0 = uncond,
// 1 = cond), s = sample, pixel = y * w + x on the h x w grid.  A tap of height s has width s * w / h (every tap sits at
// the same power-of-two scale on both axes).  One BatchNorm "batch" is one sample's two CFG rows
// (2*hw LGP rows): the reference only runs B = 1, so statistics are per sample.
#include "common.h"

namespace {

constexpr int BN_CHUNKS = 64;
constexpr int MAX_TAPS = 12;
constexpr int NEXTRA = 40;   // 4 noise-level channels + 9 * 4 sinusoid channels

struct TapArgs {
  const float* P[MAX_TAPS];
  int s[MAX_TAPS];
  int n;
};

__device__ __forceinline__ void bil_coord(int d, int s, int h, int& i0, int& i1, float& w1) {
  const float scale = (float)s / (float)h;
  float src = ((float)d + 0.5f) * scale - 0.5f;
  if (src < 0.f) src = 0.f;
  i0 = (int)src;
  if (i0 > s - 1) i0 = s - 1;
  i1 = i0 + (i0 < s - 1 ? 1 : 0);
  w1 = src - (float)i0;
}

// one 128-thread half-block per output pixel, 4 channels per thread (H0 == 512)
__global__ __launch_bounds__(256) void lgp_gather_kernel(const TapArgs taps, const half_t* __restrict__ Wx, int ldw,
                                                         const half_t* __restrict__ bias0,
                                                         const float* __restrict__ noise, float sigma, int S,
                                                         half_t* __restrict__ Z, int rows, int h, int w, int H0) {
  __shared__ float e_s[2][NEXTRA];
  const int hw = h * w;
  const int half_id = threadIdx.x >> 7;
  const int tl = threadIdx.x & 127;
  const size_t pix = (size_t)blockIdx.x * 2 + half_id;   // over rows*hw
  const bool ok = pix < (size_t)rows * hw;
  const int row = ok ? (int)(pix / hw) : 0;
  const int pp = ok ? (int)(pix - (size_t)row * hw) : 0;
  const int y = pp / w, x = pp - y * w;
  const int smp = row % S;
  if (tl < NEXTRA) {
    const int c = tl < 4 ? tl : (tl - 4) & 3;
    const float nl = sigma * noise[((size_t)smp * 4 + c) * hw + pp];
    float v = nl;
    if (tl >= 4) {
      const int l = (tl - 4) >> 2;
      v = sinf((6.283185307179586f * nl) * exp2f(-(float)l));
    }
    e_s[half_id][tl] = (float)(half_t)v;    // the reference casts the concatenated input to fp16
  }
  __syncthreads();
  if (!ok) return;
  for (int c0 = tl * 4; c0 < H0; c0 += 512) {
    float4_t acc = {0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < taps.n; ++i) {
      const int s = taps.s[i], sw = s * w / h;
      const float* P = taps.P[i] + (size_t)row * s * sw * H0 + c0;
      if (s == h) {
        acc += *reinterpret_cast<const float4_t*>(P + (size_t)pp * H0);
      } else {
        int y0, y1, x0, x1;
        float wy, wx;
        bil_coord(y, s, h, y0, y1, wy);
        bil_coord(x, sw, w, x0, x1, wx);
        const float4_t v00 = *reinterpret_cast<const float4_t*>(P + (size_t)(y0 * sw + x0) * H0);
        const float4_t v01 = *reinterpret_cast<const float4_t*>(P + (size_t)(y0 * sw + x1) * H0);
        const float4_t v10 = *reinterpret_cast<const float4_t*>(P + (size_t)(y1 * sw + x0) * H0);
        const float4_t v11 = *reinterpret_cast<const float4_t*>(P + (size_t)(y1 * sw + x1) * H0);
        acc += (1.f - wy) * ((1.f - wx) * v00 + wx * v01) + wy * ((1.f - wx) * v10 + wx * v11);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const half_t* wr = Wx + (size_t)(c0 + j) * ldw;
      float d = 0.f;
#pragma unroll
      for (int k = 0; k < NEXTRA; k += 8) {
        const half8_t wv = ld_half8(wr + k);
#pragma unroll
        for (int q = 0; q < 8; ++q) d += (float)wv[q] * e_s[half_id][k + q];
      }
      acc[j] += d + (float)bias0[c0 + j];
    }
    half4_t o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (half_t)fmaxf((float)(half_t)acc[j], 0.f);
    st_half4(Z + pix * H0 + c0, o);
  }
}

// Tiled variant (h % 8 == 0, H0 % 128 == 0): one workgroup = an 8x8 output tile x 128 channels of one row.  For every
// tap the source window of the tile (<= 8x8 native pixels; 3x3 for an 8x-upsampled tap) is staged ONCE in LDS and
// every thread interpolates from there: the per-pixel kernel above re-read four 2 KB corner rows per tap and output
// pixel from L2 (73 KB per output pixel, ~8 TB/s of L2 traffic for 589 us at 64x64); here the taps cost ~5 KB per
// output pixel.  thread = (output pixel = tid / 4, 32-channel group = tid % 4).
constexpr int GT = 8, GC = 128, GPITCH = GC + 4;
__global__ __launch_bounds__(256) void lgp_gather_tiled_kernel(const TapArgs taps, const half_t* __restrict__ Wx, int ldw,
                                                               const half_t* __restrict__ bias0,
                                                               const float* __restrict__ noise, float sigma, int S,
                                                               half_t* __restrict__ Z, int rows, int h, int w, int H0) {
  __shared__ __attribute__((aligned(16))) float patch[GT * GT * GPITCH];
  __shared__ float e_s[GT * GT][NEXTRA];
  const int hw = h * w;
  const int tiles = w / GT;
  const int ty = blockIdx.x / tiles, tx = blockIdx.x - ty * tiles;
  const int row = blockIdx.y, cbase = blockIdx.z * GC;
  const int tid = threadIdx.x;
  const int pix = tid >> 2, cg = tid & 3;
  const int py = pix >> 3, px = pix & 7;
  const int oy = ty * GT + py, ox = tx * GT + px;
  const int smp = row % S;
  for (int i = tid; Wx != nullptr && i < GT * GT * NEXTRA; i += 256) {
    const int p = i / NEXTRA, tl = i - p * NEXTRA;
    const int pp = (ty * GT + (p >> 3)) * w + tx * GT + (p & 7);
    const int c = tl < 4 ? tl : (tl - 4) & 3;
    const float nl = sigma * noise[((size_t)smp * 4 + c) * hw + pp];
    float v = nl;
    if (tl >= 4) v = sinf((6.283185307179586f * nl) * exp2f(-(float)((tl - 4) >> 2)));
    e_s[p][tl] = (float)(half_t)v;          // the reference casts the concatenated input to fp16
  }
  float4_t acc[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) acc[q] = float4_t{0.f, 0.f, 0.f, 0.f};
  for (int i = 0; i < taps.n; ++i) {
    const int s = taps.s[i], sw = s * w / h;
    int sy0, sx0, nrow, ncol;
    if (s == h) {
      sy0 = ty * GT; sx0 = tx * GT; nrow = ncol = GT;
    } else {
      int a0, a1, b0, b1;
      float wt;
      bil_coord(ty * GT, s, h, a0, a1, wt);
      bil_coord(ty * GT + GT - 1, s, h, b0, b1, wt);
      sy0 = a0; nrow = b1 - a0 + 1;
      bil_coord(tx * GT, sw, w, a0, a1, wt);
      bil_coord(tx * GT + GT - 1, sw, w, b0, b1, wt);
      sx0 = a0; ncol = b1 - a0 + 1;
    }
    __syncthreads();                                   // the previous tap's window has been consumed
    const float* P = taps.P[i] + (size_t)row * s * sw * H0 + cbase;
    for (int idx = tid; idx < nrow * ncol * (GC / 4); idx += 256) {
      const int sp = idx / (GC / 4), q = idx - sp * (GC / 4);
      const int sy = sp / ncol, sx = sp - sy * ncol;
      *reinterpret_cast<float4_t*>(&patch[sp * GPITCH + q * 4]) =
          *reinterpret_cast<const float4_t*>(P + (size_t)((sy0 + sy) * sw + sx0 + sx) * H0 + q * 4);
    }
    __syncthreads();
    const float* pc = patch + cg * 32;
    if (s == h) {
      const float* a = pc + (py * GT + px) * GPITCH;
#pragma unroll
      for (int q = 0; q < 8; ++q) acc[q] += *reinterpret_cast<const float4_t*>(a + q * 4);
    } else {
      int y0, y1, x0, x1;
      float wy, wx;
      bil_coord(oy, s, h, y0, y1, wy);
      bil_coord(ox, sw, w, x0, x1, wx);
      const float* p00 = pc + ((y0 - sy0) * ncol + (x0 - sx0)) * GPITCH;
      const float* p01 = pc + ((y0 - sy0) * ncol + (x1 - sx0)) * GPITCH;
      const float* p10 = pc + ((y1 - sy0) * ncol + (x0 - sx0)) * GPITCH;
      const float* p11 = pc + ((y1 - sy0) * ncol + (x1 - sx0)) * GPITCH;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const float4_t v00 = *reinterpret_cast<const float4_t*>(p00 + q * 4);
        const float4_t v01 = *reinterpret_cast<const float4_t*>(p01 + q * 4);
        const float4_t v10 = *reinterpret_cast<const float4_t*>(p10 + q * 4);
        const float4_t v11 = *reinterpret_cast<const float4_t*>(p11 + q * 4);
        acc[q] += (1.f - wy) * ((1.f - wx) * v00 + wx * v01) + wy * ((1.f - wx) * v10 + wx * v11);
      }
    }
  }
  const size_t orow = (size_t)row * hw + (size_t)oy * w + ox;
  half_t* zo = Z + orow * H0 + cbase + cg * 32;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    half4_t o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = cbase + cg * 32 + q * 4 + j;
      float d = 0.f;
      if (Wx != nullptr) {       // (callers normally pass the 40 extra channels as one more s == h tap instead)
        const half_t* wr = Wx + (size_t)c * ldw;
#pragma unroll
        for (int k = 0; k < NEXTRA; k += 8) {
          const half8_t wv = ld_half8(wr + k);
#pragma unroll
          for (int u = 0; u < 8; ++u) d += (float)wv[u] * e_s[pix][k + u];
        }
      }
      const float v = acc[q][j] + d + (float)bias0[c];
      o[j] = (half_t)fmaxf((float)(half_t)v, 0.f);
    }
    st_half4(zo + q * 4, o);
  }
}

// adjoint of the bilinear resize for one tap: one block per native pixel; thread = (8-channel piece, window lane):
// 16-byte loads, the window ROWS are dealt round-robin to the 256 / (H0/8) window lanes and folded in LDS.  The
// bilinear weight is separable: the row / column factors of the (<= 3f)^2 window are computed once per block into LDS,
// so the inner loop is a multiply, a test and a load + 8 FMAs (the first version redid both coordinate computations and
// an integer division for every window pixel: ~40 VALU per 16-byte load, and two thirds of the window has zero weight).
__global__ __launch_bounds__(256) void lgp_scatter_kernel(const half_t* __restrict__ dZ, int lddz,
                                                          half_t* __restrict__ dP, int rows, int h, int w, int s,
                                                          int H0) {
  __shared__ float red[256][9];
  __shared__ float cys[256], cxs[256];
  const int sw = s * w / h;
  const int ss = s * sw;
  const int row = blockIdx.x / ss;
  const int np = blockIdx.x - row * ss;
  const int py = np / sw, px = np - py * sw;
  const int f = h / s;
  const int ylo = max(0, f * py - f), yhi = min(h - 1, f * py + 2 * f - 1);
  const int xlo = max(0, f * px - f), xhi = min(w - 1, f * px + 2 * f - 1);
  const int wy_n = yhi - ylo + 1, wx_n = xhi - xlo + 1;
  const bool tab = wy_n <= 256 && wx_n <= 256;            // (always, for the resolutions of the pipeline)
  auto coef = [&](int v, int p, int n, int d) {          // weight of native index p (of n) at output index v (of d)
    int v0, v1;
    float wt;
    bil_coord(v, n, d, v0, v1, wt);
    return (v0 == p ? 1.f - wt : 0.f) + (v1 == p ? wt : 0.f);
  };
  if (tab) {
    for (int i = threadIdx.x; i < wy_n; i += 256) cys[i] = coef(ylo + i, py, s, h);
    for (int i = threadIdx.x; i < wx_n; i += 256) cxs[i] = coef(xlo + i, px, sw, w);
    __syncthreads();
  }
  const int C8 = H0 >> 3;
  for (int pb = 0; pb < C8; pb += 256) {
    const int npc = min(256, C8 - pb);
    const int WL = 256 / npc;
    const int piece = threadIdx.x % npc, wl = threadIdx.x / npc;
    const int c0 = (pb + piece) * 8;
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (wl < WL) {
      for (int yy = wl; yy < wy_n; yy += WL) {
        const float cy = tab ? cys[yy] : coef(ylo + yy, py, s, h);
        if (cy == 0.f) continue;
        const half_t* src = dZ + ((size_t)row * h * w + (size_t)(ylo + yy) * w + xlo) * lddz + c0;
        for (int xx = 0; xx < wx_n; ++xx) {
          const float wt = cy * (tab ? cxs[xx] : coef(xlo + xx, px, sw, w));
          if (wt == 0.f) continue;
          const half8_t v = ld_half8(src + (size_t)xx * lddz);
#pragma unroll
          for (int j = 0; j < 8; ++j) a[j] += wt * (float)v[j];
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) red[threadIdx.x][j] = a[j];
    __syncthreads();
    if (threadIdx.x < npc) {
      half8_t o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float t = 0.f;
        for (int l = 0; l < WL; ++l) t += red[l * npc + threadIdx.x][j];
        o[j] = (half_t)t;
      }
      st_half8(dP + ((size_t)row * ss + np) * H0 + c0, o);
    }
  }
}

// ---- BatchNorm1d, statistics over one sample's rows -------------------------------------------
// KIND 0: (sum x, sum x^2);  KIND 1: (sum dy, sum dy*xhat)
template <int KIND>
__global__ __launch_bounds__(256) void bn_partial_kernel(const half_t* __restrict__ X, int ldx,
                                                         const half_t* __restrict__ dY, int lddy, int S, int segs,
                                                         int seg_rows, int C, const float* __restrict__ stats,
                                                         float* __restrict__ partial) {
  // thread = (8-channel piece, row lane): 16-byte loads, two rows in flight per iteration, fixed-order LDS fold
  __shared__ float red[256][17];
  const int g = blockIdx.y, chunk = blockIdx.x;
  const int n = segs * seg_rows;
  const int per = (n + BN_CHUNKS - 1) / BN_CHUNKS;
  const int i0 = chunk * per, i1 = min(n, i0 + per);
  const int C8 = C >> 3;
  for (int pb = 0; pb < C8; pb += 256) {               // C <= 2048: one pass
    const int npc = min(256, C8 - pb);                   // pieces in this pass
    const int RL = 256 / npc;                            // row lanes
    const int piece = threadIdx.x % npc, rl = threadIdx.x / npc;
    const int c0 = (pb + piece) * 8;
    float s1[8], s2[8], mu[8], rs[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { s1[j] = 0.f; s2[j] = 0.f; mu[j] = 0.f; rs[j] = 0.f; }
    if (rl < RL) {
      if (KIND == 1) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          mu[j] = stats[((size_t)g * C + c0 + j) * 2];
          rs[j] = stats[((size_t)g * C + c0 + j) * 2 + 1];
        }
      }
      auto rowof = [&](int i) {
        const int jseg = i / seg_rows, ii = i - jseg * seg_rows;
        return ((size_t)jseg * S + g) * seg_rows + ii;
      };
      auto accum = [&](const half8_t& xv, const half8_t& dv) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if (KIND == 0) {
            const float a = (float)xv[j];
            s1[j] += a; s2[j] += a * a;
          } else {
            const float d = (float)dv[j];
            s1[j] += d; s2[j] += d * ((float)xv[j] - mu[j]) * rs[j];
          }
        }
      };
      int i = i0 + rl;
      for (; i + RL < i1; i += 2 * RL) {
        const size_t ra = rowof(i), rb = rowof(i + RL);
        const half8_t xa = ld_half8(X + ra * ldx + c0), xb = ld_half8(X + rb * ldx + c0);
        const half8_t da = KIND == 1 ? ld_half8(dY + ra * lddy + c0) : zero_half8();
        const half8_t db = KIND == 1 ? ld_half8(dY + rb * lddy + c0) : zero_half8();
        accum(xa, da);
        accum(xb, db);
      }
      for (; i < i1; i += RL) {
        const size_t r = rowof(i);
        accum(ld_half8(X + r * ldx + c0), KIND == 1 ? ld_half8(dY + r * lddy + c0) : zero_half8());
      }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) { red[threadIdx.x][j] = s1[j]; red[threadIdx.x][8 + j] = s2[j]; }
    __syncthreads();
    if (threadIdx.x < npc) {
      float* o = partial + (((size_t)g * BN_CHUNKS + chunk) * C + c0) * 2;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float t1 = 0.f, t2 = 0.f;
        for (int l = 0; l < RL; ++l) { t1 += red[l * npc + threadIdx.x][j]; t2 += red[l * npc + threadIdx.x][8 + j]; }
        o[2 * j] = t1; o[2 * j + 1] = t2;
      }
    }
  }
}

// fold chunks, one (channel, sample) per thread; KIND 0 -> (mean, rstd), KIND 1 -> (m1, m2).  var_out (KIND 0, optional)
// receives the biased variance for the running-statistics update.
template <int KIND>
__global__ void bn_finalize_kernel(const float* __restrict__ partial, int S, int C, int n, float eps,
                                   float* __restrict__ out, float* __restrict__ var_out) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  const int g = blockIdx.y;
  if (c >= C) return;
  float s1 = 0.f, s2 = 0.f;
  for (int k = 0; k < BN_CHUNKS; ++k) {
    const float* q = partial + (((size_t)g * BN_CHUNKS + k) * C + c) * 2;
    s1 += q[0]; s2 += q[1];
  }
  if (KIND == 0) {
    const float mean = s1 / n;
    const float var = fmaxf(s2 / n - mean * mean, 0.f);
    out[((size_t)g * C + c) * 2] = mean;
    out[((size_t)g * C + c) * 2 + 1] = rsqrtf(var + eps);
    if (var_out) var_out[(size_t)g * C + c] = var;
  } else {
    out[((size_t)g * C + c) * 2] = s1 / n;
    out[((size_t)g * C + c) * 2 + 1] = s2 / n;
  }
}

// running statistics: the S samples of a call are S successive BatchNorm batches (momentum 0.1, unbiased variance),
// applied in sample order exactly like S separate module calls
__global__ void bn_running_kernel(const float* __restrict__ stats, const float* __restrict__ var, int S, int C, int n,
                                  float* __restrict__ running_mean, float* __restrict__ running_var) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float rm = running_mean[c], rv = running_var[c];
  for (int g = 0; g < S; ++g) {
    rm = 0.9f * rm + 0.1f * stats[((size_t)g * C + c) * 2];
    rv = 0.9f * rv + 0.1f * var[(size_t)g * C + c] * ((float)n / (float)(n - 1));
  }
  running_mean[c] = rm;
  running_var[c] = rv;
}

__global__ void bn_from_running_kernel(const float* __restrict__ rm, const float* __restrict__ rv, int S, int C,
                                       float eps, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= S * C) return;
  const int c = i % C;
  out[(size_t)i * 2] = rm[c];
  out[(size_t)i * 2 + 1] = rsqrtf(rv[c] + eps);
}

// MODE 0: y = (x-mean)*rstd*gamma+beta.   MODE 1: dx = [x>0] * gamma*rstd*(dy - m1 - xhat*m2)
// Workgroup = (row chunk, sample), thread = fixed 8-channel piece x strided rows (the decomposition of bn_partial_kernel):
// the per-channel coefficients are loop-invariant registers -  y = x*a + sh,  dx = [x>0] * (dy*a - b - x*c)  - and four
// rows are in flight per thread.  (The first version re-read 128 bytes of statistics per 16 bytes of x through the
// vector-memory path, which capped it at 1.3 TB/s.)
// row chunks per sample: >= 8 rows per thread and chunk, <= 512 chunks
inline int bn_apply_chunks(int n, int C) {
  const int C8 = C >> 3, RL = C8 >= 256 ? 1 : 256 / C8;
  int c = n / (8 * RL);
  return c < 1 ? 1 : (c > 512 ? 512 : c);
}
template <int MODE>
__global__ __launch_bounds__(256) void bn_apply_kernel(const half_t* __restrict__ X, int ldx,
                                                       const half_t* __restrict__ dY, int lddy,
                                                       half_t* __restrict__ Y, int ldy, int S, int segs, int seg_rows,
                                                       int C, const float* __restrict__ stats,
                                                       const float* __restrict__ sums,
                                                       const half_t* __restrict__ gamma,
                                                       const half_t* __restrict__ beta, int train) {
  const int g = blockIdx.y, chunk = blockIdx.x;
  const int n = segs * seg_rows;
  const int per = (n + (int)gridDim.x - 1) / (int)gridDim.x;
  const int i0 = chunk * per, i1 = min(n, i0 + per);
  const int C8 = C >> 3;
  auto rowof = [&](int i) {
    const int jseg = i / seg_rows, ii = i - jseg * seg_rows;
    return ((size_t)jseg * S + g) * seg_rows + ii;
  };
  for (int pb = 0; pb < C8; pb += 256) {
    const int npc = min(256, C8 - pb);
    const int RL = 256 / npc;
    const int piece = threadIdx.x % npc, rl = threadIdx.x / npc;
    if (rl >= RL) continue;
    const int c0 = (pb + piece) * 8;
    float ca[8], cb[8], cc[8];
    {
      const half8_t gv = ld_half8(gamma + c0);
      const half8_t bv = MODE == 0 ? ld_half8(beta + c0) : zero_half8();
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float mean = stats[((size_t)g * C + c0 + j) * 2], rstd = stats[((size_t)g * C + c0 + j) * 2 + 1];
        const float a = (float)gv[j] * rstd;
        ca[j] = a;
        if (MODE == 0) {
          cb[j] = (float)bv[j] - mean * a;
          cc[j] = 0.f;
        } else {
          const float m1 = train ? sums[((size_t)g * C + c0 + j) * 2] : 0.f;
          const float m2 = train ? sums[((size_t)g * C + c0 + j) * 2 + 1] : 0.f;
          cc[j] = a * rstd * m2;                       // dx = [x>0] * (a*dy - a*m1 - a*rstd*m2*(x - mean))
          cb[j] = a * m1 - cc[j] * mean;
        }
      }
    }
    auto apply = [&](const half8_t& xv, const half8_t& dv) {
      half8_t o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float x = (float)xv[j];
        if (MODE == 0) o[j] = (half_t)(x * ca[j] + cb[j]);
        else o[j] = x > 0.f ? (half_t)((float)dv[j] * ca[j] - cb[j] - x * cc[j]) : (half_t)0.f;
      }
      return o;
    };
    int i = i0 + rl;
    for (; i + 3 * RL < i1; i += 4 * RL) {
      size_t r[4];
      half8_t xv[4], dv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        r[u] = rowof(i + u * RL);
        xv[u] = ld_half8(X + r[u] * ldx + c0);
        dv[u] = MODE == 1 ? ld_half8(dY + r[u] * lddy + c0) : zero_half8();
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) st_half8(Y + r[u] * ldy + c0, apply(xv[u], dv[u]));
    }
    for (; i < i1; i += RL) {
      const size_t r = rowof(i);
      st_half8(Y + r * ldy + c0, apply(ld_half8(X + r * ldx + c0), MODE == 1 ? ld_half8(dY + r * lddy + c0) : zero_half8()));
    }
  }
}

// one block per sample: loss, and the seed gradient for the cond row.  dOut has been zero-filled by the launcher
// (uncond rows and the padding columns stay zero); this kernel only writes the 4 real channels of the cond rows,
// one pixel (8 bytes) per thread and iteration.
__global__ __launch_bounds__(256) void mse_seed_kernel(const half_t* __restrict__ out, int ldo,
                                                       const float* __restrict__ target, half_t* __restrict__ dOut,
                                                       int ldd, float* __restrict__ loss, int S, int hw,
                                                       float loss_scale) {
  __shared__ float red[8];
  const int s = blockIdx.x;
  const float k = loss_scale * 2.f / (4.f * hw);
  float acc = 0.f;
  for (int p = threadIdx.x; p < hw; p += 256) {
    const size_t crow = ((size_t)S + s) * hw + p;
    const half4_t o = ld_half4(out + crow * ldo);
    half4_t gq;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float d = (float)o[c] - target[((size_t)s * 4 + c) * hw + p];
      acc += d * d;
      gq[c] = (half_t)(k * d);
    }
    st_half4(dOut + crow * ldd, gq);
  }
  acc = block_sum<256>(acc, red);
  if (threadIdx.x == 0 && loss) loss[s] = acc / (4.f * hw);
}

// ---- training-only kernels (LGP weight gradients + AdamW: SURVEY 8f row 4, trainer.py:208-252) --------------------
// column sums of a [M][C] fp16 matrix (bias gradients): block (x = 8-channel piece, y = row chunk) -> partial[chunk][C]
constexpr int CS_CHUNKS = 32;
__global__ __launch_bounds__(256) void colsum_partial_kernel(const half_t* __restrict__ X, int ldx, int M, int C,
                                                             float* __restrict__ partial) {
  __shared__ float red[256][8];
  const int c0 = blockIdx.x * 8, chunk = blockIdx.y;
  const int per = (M + CS_CHUNKS - 1) / CS_CHUNKS;
  const int r0 = chunk * per, r1 = min(M, r0 + per);
  float a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int r = r0 + threadIdx.x; r < r1; r += 256) {
    const half8_t v = ld_half8(X + (size_t)r * ldx + c0);
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] += (float)v[j];
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) red[threadIdx.x][j] = a[j];
  __syncthreads();
  if (threadIdx.x < 8) {          // fixed-order fold: deterministic
    float t = 0.f;
    for (int i = 0; i < 256; ++i) t += red[i][threadIdx.x];
    partial[(size_t)chunk * C + c0 + threadIdx.x] = t;
  }
}
__global__ void colsum_final_kernel(const float* __restrict__ partial, int C, float scale, float* __restrict__ out) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float t = 0.f;
  for (int k = 0; k < CS_CHUNKS; ++k) t += partial[(size_t)k * C + c];
  out[c] = t * scale;
}

// (d gamma, d beta) = (sum dy*xhat, sum dy) * scale from the folded chunk partials of bn_partial_kernel<1>
__global__ void bn_param_grads_kernel(const float* __restrict__ partial, int C, float scale,
                                      float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float s1 = 0.f, s2 = 0.f;
  for (int k = 0; k < BN_CHUNKS; ++k) {
    const float* q = partial + ((size_t)k * C + c) * 2;
    s1 += q[0]; s2 += q[1];
  }
  dbeta[c] = s1 * scale;
  dgamma[c] = s2 * scale;
}

// the 40 extra input channels of layer 0 (noise level + 36 sinusoids), fp16-rounded like the reference's cast:
// E [rows*hw][ld] with columns >= 40 zero.  Same arithmetic as lgp_gather_kernel.
__global__ __launch_bounds__(256) void lgp_extra_kernel(const float* __restrict__ noise, float sigma, int S, int rows,
                                                        int hw, half_t* __restrict__ E, int ld) {
  const size_t total = (size_t)rows * hw * ld;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t pix = i / ld;
    const int tl = (int)(i - pix * ld);
    float v = 0.f;
    if (tl < NEXTRA) {
      const int row = (int)(pix / hw), pp = (int)(pix - (size_t)row * hw);
      const int smp = row % S;
      const int c = tl < 4 ? tl : (tl - 4) & 3;
      const float nl = sigma * noise[((size_t)smp * 4 + c) * hw + pp];
      v = nl;
      if (tl >= 4) v = sinf((6.283185307179586f * nl) * exp2f(-(float)((tl - 4) >> 2)));
    }
    E[i] = (half_t)v;
  }
}

// training loss: one scalar MSE over all samples; dOut = loss_scale * 2 (out - target) / (S*4*hw) on every row
__global__ __launch_bounds__(256) void mse_train_kernel(const half_t* __restrict__ out, int ldo,
                                                        const float* __restrict__ target, half_t* __restrict__ dOut,
                                                        int ldd, float* __restrict__ loss_part, int S, int h,
                                                        float loss_scale) {
  __shared__ float red[8];
  const int s = blockIdx.x;
  const int hw = h * h;
  const float n = 4.f * hw * S;
  const float k = loss_scale * 2.f / n;
  float acc = 0.f;
  for (int p = threadIdx.x; p < hw; p += 256) {
    const size_t row = (size_t)s * hw + p;
    const half4_t o = ld_half4(out + row * ldo);
    half4_t gq;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float d = (float)o[c] - target[((size_t)s * 4 + c) * hw + p];
      acc += d * d;
      gq[c] = (half_t)(k * d);
    }
    st_half4(dOut + row * ldd, gq);
  }
  acc = block_sum<256>(acc, red);
  if (threadIdx.x == 0) loss_part[s] = acc / n;       // the caller sums the S partials (fixed order)
}

// The hyper-parameters of one AdamW step as the kernels take them (bc1 / bc2: the bias corrections 1 - beta^step).
struct AdamwArgs {
  float lr, b1, b2, eps, wd, bc1, bc2, inv_scale;
};

// One element of AdamW (decoupled weight decay): m, v in -> m', v' out, returns the new master weight.  The body of adamw_kernel
// and of adamw8_kernel: every multiply-add that is fused is written as an fma and nothing else may be contracted, so the rounding
// does not depend on the kernel the compiler inlines it into (the five fused forms are the ones adamw_kernel always had).
__device__ __forceinline__ float adamw_update(float pi, float g, float& m, float& v, const AdamwArgs& a) {
#pragma clang fp contract(off)
  const float gi = g * a.inv_scale;
  const float mi = __builtin_fmaf(a.b1, m, (1.f - a.b1) * gi);
  const float vi = __builtin_fmaf(a.b2, v, gi * ((1.f - a.b2) * gi));
  m = mi;
  v = vi;
  const float decay = __builtin_fmaf(-a.lr, a.wd, 1.f);
  const float upd = (a.lr * (mi / a.bc1)) / (sqrtf(vi / a.bc2) + a.eps);
  return __builtin_fmaf(decay, pi, -upd);
}

// AdamW, fp32 master weights + fp16 working copy; g is the loss-scaled gradient.
// GUARDED: *skip (the loss scaler's verdict, written earlier on the stream by nonfinite_flag_kernel) != 0 -> nothing is touched;
// otherwise the same body, so the two instantiations contract alike and agree to the bit.
template <bool GUARDED>
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                    float* __restrict__ m, float* __restrict__ v,
                                                    half_t* __restrict__ p16, size_t n, const AdamwArgs a,
                                                    const float* __restrict__ skip) {
  if (GUARDED && *skip != 0.f) return;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    float mi = m[i], vi = v[i];
    const float w = adamw_update(p[i], g[i], mi, vi, a);
    m[i] = mi;
    v[i] = vi;
    p[i] = w;
    if (p16) p16[i] = (half_t)w;
  }
}

// ---- 8-bit AdamW state (block-wise dynamic quantisation: DESIGN.md section 15) ---------------------------------------
// qtab: 4 x 256 floats - the signed map (m), its 255 thresholds mid[j] = 0.5f * (q[j] + q[j + 1]) (+ one unused slot), the
// unsigned map (v), its thresholds; built once on the host, copied to LDS as they are.
// A quantisation block is at most 2048 elements = 256 lanes x 8.
constexpr int Q8_ZERO1 = 127, Q8_ZERO2 = 0;

// code = #{ j : mid[j] < x }, mid ascending, 255 entries: 8 halvings, every index read lies in [0, 254] whatever x is (NaN: 0)
__device__ __forceinline__ unsigned q8_code(const float* mid, float x) {
  unsigned lo = 0;
#pragma unroll
  for (unsigned s = 128; s > 0; s >>= 1)
    if (mid[lo + s - 1] < x) lo += s;
  return lo;
}

__device__ __forceinline__ float q8_div(float s, float a) {
#pragma clang fp contract(off)
  return s / a;                          // correctly rounded (hipcc's default for fp32 division)
}

// One 256-thread workgroup per row of the block table (grid-strided), 8 consecutive elements per lane.  A row is
// (offset into p / g / p16, length <= 2048, offset into the state arrays, 8-bit or fp32), four int64: at most 2048 elements of ONE
// tensor, so the lanes beyond `len` touch nothing - not the padding between tensors either.  8-bit rows: dequantise m, v
// (q[code] * absmax), adamw_update, write p / p16 from the fresh fp32 m', v', then the block's new absmax (wave shuffle + a 4-entry
// LDS exchange, double-buffered over the rows so that one barrier per row suffices) and the new codes.  fp32 rows (tensors below
// min_8bit_size): adamw_kernel's arithmetic on the compact m32 / v32 arrays.  All stores are vector stores from the lanes.
__global__ __launch_bounds__(256) void adamw8_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                     half_t* __restrict__ p16, unsigned char* __restrict__ c1,
                                                     unsigned char* __restrict__ c2, float* __restrict__ am1,
                                                     float* __restrict__ am2, float* __restrict__ m32,
                                                     float* __restrict__ v32, const long long* __restrict__ rows, int nrows,
                                                     const float* __restrict__ qtab, const AdamwArgs a,
                                                     const float* __restrict__ skip) {
  __shared__ float sq[1024];
  __shared__ float red[2][2][4];
  if (skip && *skip != 0.f) return;
  for (int i = threadIdx.x; i < 1024; i += 256) sq[i] = qtab[i];
  __syncthreads();
  const float* q1 = sq;
  const float* mid1 = sq + 256;
  const float* q2 = sq + 512;
  const float* mid2 = sq + 768;
  const int lane8 = threadIdx.x * 8, wave = threadIdx.x >> 6;
  int par = 0;
  for (int r = blockIdx.x; r < nrows; r += gridDim.x) {
    const long long off = rows[4 * (size_t)r] + lane8, len = rows[4 * (size_t)r + 1];
    const long long soff = rows[4 * (size_t)r + 2] + lane8;
    const bool is8 = rows[4 * (size_t)r + 3] != 0;
    const long long left = len - lane8;
    const int nv = left >= 8 ? 8 : (left > 0 ? (int)left : 0);      // this lane's elements: 8, or the row's short tail, or none
    const bool full = nv == 8;
    float gi[8], pi[8], mi[8], vi[8];
    unsigned char k1[8], k2[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) gi[e] = pi[e] = mi[e] = vi[e] = 0.f, k1[e] = k2[e] = 0;
    if (full) {
      const float4 g0 = *reinterpret_cast<const float4*>(g + off), g1 = *reinterpret_cast<const float4*>(g + off + 4);
      const float4 p0 = *reinterpret_cast<const float4*>(p + off), p1 = *reinterpret_cast<const float4*>(p + off + 4);
      gi[0] = g0.x, gi[1] = g0.y, gi[2] = g0.z, gi[3] = g0.w, gi[4] = g1.x, gi[5] = g1.y, gi[6] = g1.z, gi[7] = g1.w;
      pi[0] = p0.x, pi[1] = p0.y, pi[2] = p0.z, pi[3] = p0.w, pi[4] = p1.x, pi[5] = p1.y, pi[6] = p1.z, pi[7] = p1.w;
      if (is8) {
        const uint2 u1 = *reinterpret_cast<const uint2*>(c1 + soff), u2 = *reinterpret_cast<const uint2*>(c2 + soff);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          k1[e] = (unsigned char)(u1.x >> (8 * e)), k1[4 + e] = (unsigned char)(u1.y >> (8 * e));
          k2[e] = (unsigned char)(u2.x >> (8 * e)), k2[4 + e] = (unsigned char)(u2.y >> (8 * e));
        }
      } else {
        const float4 m0 = *reinterpret_cast<const float4*>(m32 + soff), m1 = *reinterpret_cast<const float4*>(m32 + soff + 4);
        const float4 v0 = *reinterpret_cast<const float4*>(v32 + soff), v1 = *reinterpret_cast<const float4*>(v32 + soff + 4);
        mi[0] = m0.x, mi[1] = m0.y, mi[2] = m0.z, mi[3] = m0.w, mi[4] = m1.x, mi[5] = m1.y, mi[6] = m1.z, mi[7] = m1.w;
        vi[0] = v0.x, vi[1] = v0.y, vi[2] = v0.z, vi[3] = v0.w, vi[4] = v1.x, vi[5] = v1.y, vi[6] = v1.z, vi[7] = v1.w;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (e < nv) {
          gi[e] = g[off + e];
          pi[e] = p[off + e];
          if (is8) k1[e] = c1[soff + e], k2[e] = c2[soff + e];
          else mi[e] = m32[soff + e], vi[e] = v32[soff + e];
        }
    }
    if (is8) {
      const float a1 = am1[r], a2 = am2[r];
#pragma unroll
      for (int e = 0; e < 8; ++e) mi[e] = q1[k1[e]] * a1, vi[e] = q2[k2[e]] * a2;
    }
    float w[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) w[e] = adamw_update(pi[e], gi[e], mi[e], vi[e], a);
    if (full) {
      *reinterpret_cast<float4*>(p + off) = make_float4(w[0], w[1], w[2], w[3]);
      *reinterpret_cast<float4*>(p + off + 4) = make_float4(w[4], w[5], w[6], w[7]);
      if (p16) {
        half8_t h;
#pragma unroll
        for (int e = 0; e < 8; ++e) h[e] = (half_t)w[e];
        st_half8(p16 + off, h);
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (e < nv) {
          p[off + e] = w[e];
          if (p16) p16[off + e] = (half_t)w[e];
        }
    }
    if (!is8) {                          // (block-uniform: the barrier below is reached by all lanes or by none)
      if (full) {
        *reinterpret_cast<float4*>(m32 + soff) = make_float4(mi[0], mi[1], mi[2], mi[3]);
        *reinterpret_cast<float4*>(m32 + soff + 4) = make_float4(mi[4], mi[5], mi[6], mi[7]);
        *reinterpret_cast<float4*>(v32 + soff) = make_float4(vi[0], vi[1], vi[2], vi[3]);
        *reinterpret_cast<float4*>(v32 + soff + 4) = make_float4(vi[4], vi[5], vi[6], vi[7]);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (e < nv) m32[soff + e] = mi[e], v32[soff + e] = vi[e];
      }
      continue;
    }
    // the block's new absmax, exact: lanes without elements contribute 0 (the update of an all-zero element was discarded)
    float x1 = 0.f, x2 = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (e < nv) x1 = fmaxf(x1, fabsf(mi[e])), x2 = fmaxf(x2, fabsf(vi[e]));
    x1 = wave_max(x1);
    x2 = wave_max(x2);
    if ((threadIdx.x & 63) == 0) red[par][0][wave] = x1, red[par][1][wave] = x2;
    __syncthreads();
    const float n1 = fmaxf(fmaxf(red[par][0][0], red[par][0][1]), fmaxf(red[par][0][2], red[par][0][3]));
    const float n2 = fmaxf(fmaxf(red[par][1][0], red[par][1][1]), fmaxf(red[par][1][2], red[par][1][3]));
    if (threadIdx.x == 0) am1[r] = n1, am2[r] = n2;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      k1[e] = (unsigned char)(n1 == 0.f ? Q8_ZERO1 : q8_code(mid1, q8_div(mi[e], n1)));
      k2[e] = (unsigned char)(n2 == 0.f ? Q8_ZERO2 : q8_code(mid2, q8_div(vi[e], n2)));
    }
    if (full) {
      uint2 u1 = make_uint2(0, 0), u2 = make_uint2(0, 0);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        u1.x |= (unsigned)k1[e] << (8 * e), u1.y |= (unsigned)k1[4 + e] << (8 * e);
        u2.x |= (unsigned)k2[e] << (8 * e), u2.y |= (unsigned)k2[4 + e] << (8 * e);
      }
      *reinterpret_cast<uint2*>(c1 + soff) = u1;
      *reinterpret_cast<uint2*>(c2 + soff) = u2;
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (e < nv) c1[soff + e] = k1[e], c2[soff + e] = k2[e];
    }
    par ^= 1;                            // (only where a barrier was passed: two 8-bit rows in a row never share a buffer)
  }
}

// ±inf / NaN: exponent bits all ones
__device__ __forceinline__ unsigned nonfinite_bits(unsigned u) { return (u & 0x7f800000u) == 0x7f800000u; }
__device__ __forceinline__ unsigned nonfinite_bits(const uint4& u) {
  return nonfinite_bits(u.x) | nonfinite_bits(u.y) | nonfinite_bits(u.z) | nonfinite_bits(u.w);
}

// *flag = 1.0f when any of x[0, n) is non-finite, untouched otherwise (several vectors OR into one flag).  x is 4-byte aligned:
// `head` (0 ... 3) scalars up to the first 16-byte boundary, nvec 16-byte loads (grid-stride, four in flight per lane), then the
// scalar tail; head and tail belong to block 0.  A wave with a hit stores 1.0f from its first lane: every writer stores the same
// value, so the stores need no order among themselves.
__global__ __launch_bounds__(256) void nonfinite_flag_kernel(const unsigned* __restrict__ x, size_t n, size_t head,
                                                             size_t nvec, float* __restrict__ flag) {
  const uint4* __restrict__ xv = reinterpret_cast<const uint4*>(x + head);
  const size_t stride = (size_t)gridDim.x * 256;
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  unsigned bad = 0;
  for (; i + 3 * stride < nvec; i += 4 * stride) {
    const uint4 a = xv[i], b = xv[i + stride], c = xv[i + 2 * stride], d = xv[i + 3 * stride];
    bad |= nonfinite_bits(a) | nonfinite_bits(b) | nonfinite_bits(c) | nonfinite_bits(d);
  }
  for (; i < nvec; i += stride) bad |= nonfinite_bits(xv[i]);
  if (blockIdx.x == 0) {
    const size_t body_end = head + 4 * nvec;
    if (threadIdx.x < head) bad |= nonfinite_bits(x[threadIdx.x]);
    if (threadIdx.x >= 64 && body_end + (threadIdx.x - 64) < n) bad |= nonfinite_bits(x[body_end + (threadIdx.x - 64)]);
  }
  const unsigned long long hits = __ballot(bad != 0);
  if (hits != 0 && (threadIdx.x & 63) == 0) *flag = 1.0f;
}

inline int ew_grid(size_t total_items) {
  size_t b = (total_items + 255) / 256;
  if (b > 4096) b = 4096;
  if (b < 1) b = 1;
  return (int)b;
}

}  // namespace

// a tap of height s on the h x w grid: s divides h and the tap's width s * w / h divides w (the same scale on both axes)
static inline bool tap_fits(int s, int h, int w) {
  return s > 0 && h % s == 0 && ((long long)s * w) % h == 0 && w % (int)((long long)s * w / h) == 0;
}

// a square grid passes w = h; a rectangular one has 8-multiple sides (same kernels, same arithmetic)
static inline bool grid_ok(int h, int w) { return h == w || (h % GT == 0 && w % GT == 0); }

extern "C" int skg_lgp_layer0_gather(const SkgLgpTap* taps, int ntaps, const void* Wextra, int ldw, const void* bias0,
                                     const float* noise, float sigma, int samples, void* Z, int rows, int h, int w, int H0,
                                     void* stream) {
  SKG_REQUIRE(grid_ok(h, w));
  SKG_REQUIRE(taps && ntaps > 0 && ntaps <= MAX_TAPS && bias0 && noise && Z && rows > 0 && h > 0 && w > 0);
  SKG_REQUIRE(H0 % 4 == 0 && skg_aligned(Z, 8) && samples > 0 && rows % samples == 0);
  SKG_REQUIRE(Wextra ? (ldw % 8 == 0 && skg_aligned(Wextra, 16)) : (h % GT == 0 && w % GT == 0 && H0 % GC == 0));
  TapArgs a{};
  a.n = ntaps;
  for (int i = 0; i < ntaps; ++i) {
    SKG_REQUIRE(taps[i].P && tap_fits(taps[i].s, h, w) && skg_aligned(taps[i].P, 16));
    a.P[i] = taps[i].P;
    a.s[i] = taps[i].s;
  }
  if (h % GT == 0 && w % GT == 0 && H0 % GC == 0) {
    hipLaunchKernelGGL(lgp_gather_tiled_kernel, dim3((h / GT) * (w / GT), rows, H0 / GC), dim3(256), 0,
                       (hipStream_t)stream, a, (const half_t*)Wextra, ldw, (const half_t*)bias0, noise, sigma, samples,
                       (half_t*)Z, rows, h, w, H0);
    SKG_CHECK_LAUNCH("skg_lgp_layer0_gather");
    return SKG_OK;
  }
  const size_t pixels = (size_t)rows * h * w;
  hipLaunchKernelGGL(lgp_gather_kernel, dim3((unsigned)((pixels + 1) / 2)), dim3(256), 0, (hipStream_t)stream, a,
                     (const half_t*)Wextra, ldw, (const half_t*)bias0, noise, sigma, samples, (half_t*)Z, rows, h, w, H0);
  SKG_CHECK_LAUNCH("skg_lgp_layer0_gather");
  return SKG_OK;
}

extern "C" int skg_lgp_layer0_scatter(const void* dZ, int lddz, void* dP, int rows, int h, int w, int s, int H0,
                                      void* stream) {
  SKG_REQUIRE(grid_ok(h, w) && dZ && dP && rows > 0 && h > 0 && w > 0 && tap_fits(s, h, w) && H0 % 8 == 0 && lddz % 8 == 0 &&
              skg_aligned(dZ, 16) && skg_aligned(dP, 16));
  hipLaunchKernelGGL(lgp_scatter_kernel, dim3(rows * s * (s * w / h)), dim3(256), 0, (hipStream_t)stream,
                     (const half_t*)dZ, lddz, (half_t*)dP, rows, h, w, s, H0);
  SKG_CHECK_LAUNCH("skg_lgp_layer0_scatter");
  return SKG_OK;
}

extern "C" int skg_lgp_mse_seed(const void* out, int ldo, const float* target, void* dOut, int ldd, float* loss,
                                int samples, int h, int w, float loss_scale, void* stream) {
  SKG_REQUIRE(grid_ok(h, w) && out && target && dOut && samples > 0 && h > 0 && w > 0 && ldo >= 4 && ldd >= 4 && ldo % 4 == 0 &&
              ldd % 4 == 0);
  SKG_REQUIRE(skg_aligned(out, 8) && skg_aligned(dOut, 8));
  if (hipMemsetAsync(dOut, 0, (size_t)2 * samples * h * w * ldd * sizeof(half_t), (hipStream_t)stream) != hipSuccess)
    return SKG_E_LAUNCH;
  hipLaunchKernelGGL(mse_seed_kernel, dim3(samples), dim3(256), 0, (hipStream_t)stream, (const half_t*)out, ldo,
                     target, (half_t*)dOut, ldd, loss, samples, h * w, loss_scale);
  SKG_CHECK_LAUNCH("skg_lgp_mse_seed");
  return SKG_OK;
}

extern "C" int skg_lgp_extra_features(const float* noise, float sigma, int samples, int rows, int h, int w, void* E,
                                      int ld, void* stream) {
  SKG_REQUIRE(grid_ok(h, w) && noise && E && samples > 0 && rows > 0 && rows % samples == 0 && h > 0 && w > 0 && ld >= NEXTRA);
  hipLaunchKernelGGL(lgp_extra_kernel, dim3(ew_grid((size_t)rows * h * w * ld)), dim3(256), 0, (hipStream_t)stream,
                     noise, sigma, samples, rows, h * w, (half_t*)E, ld);
  SKG_CHECK_LAUNCH("skg_lgp_extra_features");
  return SKG_OK;
}

extern "C" size_t skg_bn_scratch_floats(int samples, int C) {
  return (size_t)samples * BN_CHUNKS * C * 2 + (size_t)samples * C * 2;
}

extern "C" int skg_bn_stats(const void* X, int ldx, int samples, int segs, int seg_rows, int C, float eps,
                            float* stats, float* scratch, float* running_mean, float* running_var, void* stream) {
  SKG_REQUIRE(X && stats && scratch && samples > 0 && segs > 0 && seg_rows > 0 && C % 8 == 0 && ldx % 8 == 0 &&
              skg_aligned(X, 16));
  SKG_REQUIRE((running_mean == nullptr) == (running_var == nullptr));
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL((bn_partial_kernel<0>), dim3(BN_CHUNKS, samples), dim3(256), 0, st, (const half_t*)X, ldx,
                     (const half_t*)nullptr, 0, samples, segs, seg_rows, C, (const float*)nullptr, scratch);
  float* var = scratch + (size_t)samples * BN_CHUNKS * C * 2;      // [samples][C] (the "sums" area of the backward)
  hipLaunchKernelGGL((bn_finalize_kernel<0>), dim3(skg_cdiv(C, 128), samples), dim3(128), 0, st, scratch, samples, C,
                     segs * seg_rows, eps, stats, running_mean ? var : (float*)nullptr);
  if (running_mean)
    hipLaunchKernelGGL(bn_running_kernel, dim3(skg_cdiv(C, 128)), dim3(128), 0, st, stats, var, samples, C,
                       segs * seg_rows, running_mean, running_var);
  SKG_CHECK_LAUNCH("skg_bn_stats");
  return SKG_OK;
}

extern "C" int skg_bn_stats_from_running(const float* running_mean, const float* running_var, int samples, int C,
                                         float eps, float* stats, void* stream) {
  SKG_REQUIRE(running_mean && running_var && stats && samples > 0 && C > 0);
  hipLaunchKernelGGL(bn_from_running_kernel, dim3(skg_cdiv(samples * C, 256)), dim3(256), 0, (hipStream_t)stream,
                     running_mean, running_var, samples, C, eps, stats);
  SKG_CHECK_LAUNCH("skg_bn_stats_from_running");
  return SKG_OK;
}

extern "C" int skg_bn_apply(const void* X, int ldx, void* Y, int ldy, int samples, int segs, int seg_rows, int C,
                            const float* stats, const void* gamma, const void* beta, void* stream) {
  SKG_REQUIRE(X && Y && stats && gamma && beta && samples > 0 && C % 8 == 0 && ldx % 8 == 0 && ldy % 8 == 0);
  SKG_REQUIRE(skg_aligned(X, 16) && skg_aligned(Y, 16) && skg_aligned(gamma, 16) && skg_aligned(beta, 16));
  SKG_REQUIRE(segs > 0 && seg_rows > 0);
  hipLaunchKernelGGL((bn_apply_kernel<0>), dim3(bn_apply_chunks(segs * seg_rows, C), samples), dim3(256), 0, (hipStream_t)stream,
                     (const half_t*)X, ldx, (const half_t*)nullptr, 0, (half_t*)Y, ldy, samples, segs, seg_rows, C,
                     stats, (const float*)nullptr, (const half_t*)gamma, (const half_t*)beta, 1);
  SKG_CHECK_LAUNCH("skg_bn_apply");
  return SKG_OK;
}

extern "C" int skg_bn_relu_bwd(const void* X, int ldx, const void* dY, int lddy, void* dX, int lddx, int samples,
                               int segs, int seg_rows, int C, const float* stats, const void* gamma,
                               int train_mode, float* scratch, void* stream) {
  SKG_REQUIRE(X && dY && dX && stats && gamma && scratch && samples > 0 && C % 8 == 0);
  SKG_REQUIRE(ldx % 8 == 0 && lddy % 8 == 0 && lddx % 8 == 0 && skg_aligned(X, 16) && skg_aligned(dY, 16) &&
              skg_aligned(dX, 16) && skg_aligned(gamma, 16));
  hipStream_t st = (hipStream_t)stream;
  float* sums = scratch + (size_t)samples * BN_CHUNKS * C * 2;
  if (train_mode) {
    hipLaunchKernelGGL((bn_partial_kernel<1>), dim3(BN_CHUNKS, samples), dim3(256), 0, st, (const half_t*)X, ldx,
                       (const half_t*)dY, lddy, samples, segs, seg_rows, C, stats, scratch);
    hipLaunchKernelGGL((bn_finalize_kernel<1>), dim3(skg_cdiv(C, 128), samples), dim3(128), 0, st, scratch, samples, C,
                       segs * seg_rows, 0.f, sums, (float*)nullptr);
  }
  hipLaunchKernelGGL((bn_apply_kernel<1>), dim3(bn_apply_chunks(segs * seg_rows, C), samples), dim3(256), 0, st, (const half_t*)X, ldx,
                     (const half_t*)dY, lddy, (half_t*)dX, lddx, samples, segs, seg_rows, C, stats, sums,
                     (const half_t*)gamma, (const half_t*)nullptr, train_mode);
  SKG_CHECK_LAUNCH("skg_bn_relu_bwd");
  return SKG_OK;
}

// ---- training entry points ----------------------------------------------------------------------------------------
extern "C" size_t skg_colsum_scratch_floats(int C) { return (size_t)CS_CHUNKS * C; }

extern "C" int skg_colsum_f16(const void* X, int ldx, int M, int C, float scale, float* out, float* scratch,
                              void* stream) {
  SKG_REQUIRE(X && out && scratch && M > 0 && C > 0 && C % 8 == 0 && ldx % 8 == 0 && ldx >= C && skg_aligned(X, 16));
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(colsum_partial_kernel, dim3(C / 8, CS_CHUNKS), dim3(256), 0, st, (const half_t*)X, ldx, M, C,
                     scratch);
  hipLaunchKernelGGL(colsum_final_kernel, dim3(skg_cdiv(C, 128)), dim3(128), 0, st, scratch, C, scale, out);
  SKG_CHECK_LAUNCH("skg_colsum_f16");
  return SKG_OK;
}

extern "C" int skg_bn_param_grads(const void* X, int ldx, const void* dY, int lddy, int rows, int C,
                                  const float* stats, float scale, float* dgamma, float* dbeta, float* scratch,
                                  void* stream) {
  SKG_REQUIRE(X && dY && stats && dgamma && dbeta && scratch && rows > 0 && C % 8 == 0 && ldx % 8 == 0 && lddy % 8 == 0 &&
              skg_aligned(X, 16) && skg_aligned(dY, 16));
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL((bn_partial_kernel<1>), dim3(BN_CHUNKS, 1), dim3(256), 0, st, (const half_t*)X, ldx,
                     (const half_t*)dY, lddy, 1, 1, rows, C, stats, scratch);
  hipLaunchKernelGGL(bn_param_grads_kernel, dim3(skg_cdiv(C, 128)), dim3(128), 0, st, scratch, C, scale, dgamma, dbeta);
  SKG_CHECK_LAUNCH("skg_bn_param_grads");
  return SKG_OK;
}

extern "C" int skg_lgp_mse_train(const void* out, int ldo, const float* target, void* dOut, int ldd,
                                 float* loss_parts, int samples, int h, float loss_scale, void* stream) {
  SKG_REQUIRE(out && target && dOut && loss_parts && samples > 0 && h > 0 && ldo >= 4 && ldd >= 4 && ldo % 4 == 0 &&
              ldd % 4 == 0 && skg_aligned(out, 8) && skg_aligned(dOut, 8));
  if (hipMemsetAsync(dOut, 0, (size_t)samples * h * h * ldd * sizeof(half_t), (hipStream_t)stream) != hipSuccess)
    return SKG_E_LAUNCH;
  hipLaunchKernelGGL(mse_train_kernel, dim3(samples), dim3(256), 0, (hipStream_t)stream, (const half_t*)out, ldo,
                     target, (half_t*)dOut, ldd, loss_parts, samples, h, loss_scale);
  SKG_CHECK_LAUNCH("skg_lgp_mse_train");
  return SKG_OK;
}

extern "C" int skg_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* param_f16,
                              size_t n, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                              float inv_grad_scale, void* stream) {
  SKG_REQUIRE(param && grad && exp_avg && exp_avg_sq && n > 0 && step >= 1 && lr >= 0.f);
  const float bc1 = 1.f - powf(beta1, (float)step), bc2 = 1.f - powf(beta2, (float)step);
  hipLaunchKernelGGL(adamw_kernel<false>, dim3(ew_grid(n)), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg,
                     exp_avg_sq, (half_t*)param_f16, n, AdamwArgs{lr, beta1, beta2, eps, weight_decay, bc1, bc2, inv_grad_scale},
                     (const float*)nullptr);
  SKG_CHECK_LAUNCH("skg_adamw_step");
  return SKG_OK;
}

extern "C" int skg_adamw_step_guarded(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* param_f16,
                                      size_t n, float lr, float beta1, float beta2, float eps, float weight_decay,
                                      int step, float inv_grad_scale, const float* skip_flag, void* stream) {
  SKG_REQUIRE(param && grad && exp_avg && exp_avg_sq && skip_flag && n > 0 && step >= 1 && lr >= 0.f);
  const float bc1 = 1.f - powf(beta1, (float)step), bc2 = 1.f - powf(beta2, (float)step);
  hipLaunchKernelGGL(adamw_kernel<true>, dim3(ew_grid(n)), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg,
                     exp_avg_sq, (half_t*)param_f16, n, AdamwArgs{lr, beta1, beta2, eps, weight_decay, bc1, bc2, inv_grad_scale},
                     skip_flag);
  SKG_CHECK_LAUNCH("skg_adamw_step_guarded");
  return SKG_OK;
}

extern "C" int skg_adamw8_step(float* param, const float* grad, void* param_f16, unsigned char* state1, unsigned char* state2,
                               float* absmax1, float* absmax2, float* exp_avg32, float* exp_avg_sq32, const SkgAdamw8Row* rows,
                               int nrows, const float* qtab, float lr, float beta1, float beta2, float eps, float weight_decay,
                               int step, float inv_grad_scale, const float* skip, void* stream) {
  SKG_REQUIRE(param && grad && state1 && state2 && absmax1 && absmax2 && exp_avg32 && exp_avg_sq32 && rows && qtab);
  SKG_REQUIRE(nrows >= 0 && step >= 1 && lr >= 0.f);
  SKG_REQUIRE(skg_aligned(param, 16) && skg_aligned(grad, 16) && skg_aligned(param_f16, 16) && skg_aligned(state1, 8) &&
              skg_aligned(state2, 8) && skg_aligned(exp_avg32, 16) && skg_aligned(exp_avg_sq32, 16) && skg_aligned(rows, 8));
  if (nrows == 0) return SKG_OK;
  static_assert(sizeof(SkgAdamw8Row) == 4 * sizeof(long long), "a table row is four int64");
  const float bc1 = 1.f - powf(beta1, (float)step), bc2 = 1.f - powf(beta2, (float)step);
  // 2048 workgroups: more than are resident at once (the chip takes them in as others finish; a grid of exactly the resident ones
  // measured the same), each walks its share of the rows
  hipLaunchKernelGGL(adamw8_kernel, dim3(nrows < 2048 ? nrows : 2048), dim3(256), 0, (hipStream_t)stream, param, grad,
                     (half_t*)param_f16, state1, state2, absmax1, absmax2, exp_avg32, exp_avg_sq32, (const long long*)rows,
                     nrows, qtab, AdamwArgs{lr, beta1, beta2, eps, weight_decay, bc1, bc2, inv_grad_scale}, skip);
  SKG_CHECK_LAUNCH("skg_adamw8_step");
  return SKG_OK;
}

extern "C" int skg_nonfinite_flag(const float* x, size_t n, float* flag, int reset, void* stream) {
  SKG_REQUIRE(x && flag && n > 0 && skg_aligned(x, 4) && skg_aligned(flag, 4));
  if (reset && hipMemsetAsync(flag, 0, sizeof(float), (hipStream_t)stream) != hipSuccess) return SKG_E_LAUNCH;
  size_t head = (4 - (((uintptr_t)x >> 2) & 3)) & 3;          // floats up to the first 16-byte boundary
  if (head > n) head = n;
  const size_t nvec = (n - head) / 4;
  hipLaunchKernelGGL(nonfinite_flag_kernel, dim3(ew_grid(nvec)), dim3(256), 0, (hipStream_t)stream, (const unsigned*)x, n,
                     head, nvec, flag);
  SKG_CHECK_LAUNCH("skg_nonfinite_flag");
  return SKG_OK;
}
