// Sketch generator (anime2sketch U-Net, sketch2img_amd/anime2sketch.py): the pieces the GEMM / conv library does not have.
//   * InstanceNorm2d(affine = False) on NHWC fp16 with up to two activated outputs (LeakyReLU into the next down convolution's
//     operand, ReLU into the skip half of the concatenation buffer the up convolution reads)
//   * ConvTranspose2d(4, stride 2, padding 1) = the polyphase launch of skg_conv3x3_up2_f16 on an un-summed phase pack (+ tanh)
//   * the first layer's operand: float NCHW picture -> fp16 [pixels][4 x 4 x 3 window, padded to 64] for ONE K = 64 GEMM
//   * the tail of generate_sketch: y -> float NCHW, 1 - y binarised at 0.5 and tiled to three channels
#include "common.h"

namespace {

constexpr int IN_THREADS = 256;
constexpr int IN_CW = 64;          // channels of one workgroup: 8 octets x 32 pixel lanes
constexpr int IN_LANES = IN_THREADS / (IN_CW / 8);
constexpr int IN_SLAB = 256;       // pixels of one (sample, slab) workgroup; a map of one slab is ONE launch (statistics + apply)

enum { IN_FUSED = 0, IN_PARTIAL = 1, IN_APPLY = 2, IN_IDENTITY = 3 };

struct InParams {
  const half_t* X; int ldx;
  int HW, C, slab, nslab;
  float eps;
  half_t* Y0; int ldy0; float slope0;
  half_t* Y1; int ldy1; float slope1;
  float* partial;      // [rows][nslab][C][2]: sum and sum of squares of (x - x[pixel 0]) over the slab
  float* stats;        // [rows][C][2]: mean, 1 / sqrt(var + eps)
};

// slab length of a map: 256 pixels up to 256 slabs, longer slabs (whole pixel-lane rounds) beyond - never more than 256 partials to fold
inline int in_slab(int HW) {
  return HW <= 256 * IN_SLAB ? IN_SLAB : skg_cdiv(skg_cdiv(HW, 256), IN_LANES) * IN_LANES;
}

__device__ __forceinline__ half8_t act8(const float* v, float slope) {
  half8_t o;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float h = (float)(half_t)v[e];      // the normalised value in its fp16 storage, then the activation
    o[e] = (half_t)(h >= 0.f ? h : slope * h);
  }
  return o;
}

// Workgroup (slab, 64-channel block, sample); thread t owns the eight channels of octet t % 8 and walks the pixels t / 8, + 32, ...
// of its slab.  Sums are taken relative to the sample's first pixel (per channel) so that E[d^2] - E[d]^2 does not cancel for
// channels whose mean is large against their spread.  Every order of summation is fixed: thread-sequential over pixels, then over
// the 32 pixel lanes in LDS, then over the slabs (instnorm_finalize_kernel) - two runs give the same bits.
template <int MODE>
__global__ __launch_bounds__(IN_THREADS) void instnorm_kernel(InParams p) {
  __shared__ float red[IN_LANES * IN_CW * 2];
  __shared__ float s_mean[IN_CW], s_rstd[IN_CW];
  const int t = threadIdx.x, cg = t & 7, pl = t >> 3;
  const int slab = blockIdx.x, c0 = blockIdx.y * IN_CW, row = blockIdx.z;
  const int p0 = slab * p.slab, p1 = min(p.HW, p0 + p.slab);
  const half_t* Xr = p.X + (size_t)row * p.HW * p.ldx + c0 + cg * 8;
  float mean[8], rstd[8];

  if (MODE == IN_FUSED || MODE == IN_PARTIAL) {
    const half8_t sh = ld_half8(Xr);
    float s[8], q[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] = q[e] = 0.f;
    for (int px = p0 + pl; px < p1; px += IN_LANES) {
      const half8_t v = ld_half8(Xr + (size_t)px * p.ldx);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float d = (float)v[e] - (float)sh[e];
        s[e] += d;
        q[e] = fmaf(d, d, q[e]);
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      red[(pl * IN_CW + cg * 8 + e) * 2] = s[e];
      red[(pl * IN_CW + cg * 8 + e) * 2 + 1] = q[e];
    }
    __syncthreads();
    if (t < IN_CW) {
      float ss = 0.f, qq = 0.f;
      for (int l = 0; l < IN_LANES; ++l) {
        ss += red[(l * IN_CW + t) * 2];
        qq += red[(l * IN_CW + t) * 2 + 1];
      }
      if (MODE == IN_PARTIAL) {
        float* o = p.partial + (((size_t)row * p.nslab + slab) * p.C + c0 + t) * 2;
        o[0] = ss;
        o[1] = qq;
      } else {
        const double n = (double)p.HW, m = (double)ss / n, var = fmax((double)qq / n - m * m, 0.0);
        s_mean[t] = (float)((double)(float)p.X[(size_t)row * p.HW * p.ldx + c0 + t] + m);
        s_rstd[t] = (float)(1.0 / sqrt(var + (double)p.eps));
      }
    }
    if (MODE == IN_PARTIAL) return;
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 8; ++e) { mean[e] = s_mean[cg * 8 + e]; rstd[e] = s_rstd[cg * 8 + e]; }
  } else if (MODE == IN_APPLY) {
    const float* st = p.stats + ((size_t)row * p.C + c0 + cg * 8) * 2;
#pragma unroll
    for (int e = 0; e < 8; ++e) { mean[e] = st[2 * e]; rstd[e] = st[2 * e + 1]; }
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) { mean[e] = 0.f; rstd[e] = 1.f; }
  }
  for (int px = p0 + pl; px < p1; px += IN_LANES) {
    const half8_t v = ld_half8(Xr + (size_t)px * p.ldx);
    float n[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) n[e] = ((float)v[e] - mean[e]) * rstd[e];
    const size_t m = (size_t)row * p.HW + px;
    if (p.Y0) st_half8(p.Y0 + m * p.ldy0 + c0 + cg * 8, act8(n, p.slope0));
    if (p.Y1) st_half8(p.Y1 + m * p.ldy1 + c0 + cg * 8, act8(n, p.slope1));
  }
}

// slab partials -> (mean, rstd) per (sample, channel): workgroup (64-channel block, sample), four threads per channel take every
// fourth slab in fp64, then one thread adds the four in order
__global__ __launch_bounds__(IN_THREADS) void instnorm_finalize_kernel(InParams p) {
  __shared__ double red[4 * IN_CW * 2];
  const int t = threadIdx.x, c = t & (IN_CW - 1), part = t >> 6;
  const int c0 = blockIdx.x * IN_CW, row = blockIdx.y;
  double ss = 0.0, qq = 0.0;
  const float* o = p.partial + ((size_t)row * p.nslab * p.C + c0 + c) * 2;
  for (int sl = part; sl < p.nslab; sl += 4) {
    ss += (double)o[(size_t)sl * p.C * 2];
    qq += (double)o[(size_t)sl * p.C * 2 + 1];
  }
  red[(part * IN_CW + c) * 2] = ss;
  red[(part * IN_CW + c) * 2 + 1] = qq;
  __syncthreads();
  if (t < IN_CW) {
    ss = qq = 0.0;
    for (int q4 = 0; q4 < 4; ++q4) {
      ss += red[(q4 * IN_CW + t) * 2];
      qq += red[(q4 * IN_CW + t) * 2 + 1];
    }
    const double n = (double)p.HW, m = ss / n, var = fmax(qq / n - m * m, 0.0);
    float* st = p.stats + ((size_t)row * p.C + c0 + t) * 2;
    st[0] = (float)((double)(float)p.X[(size_t)row * p.HW * p.ldx + c0 + t] + m);
    st[1] = (float)(1.0 / sqrt(var + (double)p.eps));
  }
}

// in-place tanh over the Cout columns of Y [M][ldy] (eight columns per thread)
__global__ __launch_bounds__(256) void tanh_rows_kernel(half_t* Y, int ldy, size_t M, int octets) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * octets) return;
  half_t* y = Y + (i / octets) * ldy + (i % octets) * 8;
  half8_t v = ld_half8(y);
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = (half_t)tanhf((float)v[e]);
  st_half8(y, v);
}

// P[(b, oy, ox)][(ky * 4 + kx) * 3 + c] = img[b][c][2 oy - 1 + ky][2 ox - 1 + kx] (0 outside the picture), columns 48..63 = 0
__global__ __launch_bounds__(256) void patch_kernel(const float* img, half_t* P, int ldp, int B, int H, int W) {
  const int OH = H >> 1, OW = W >> 1;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t M = (size_t)B * OH * OW;
  if (i >= M * 8) return;
  const size_t m = i >> 3;
  const int oct = (int)(i & 7);
  const int ox = (int)(m % OW), oy = (int)((m / OW) % OH), b = (int)(m / ((size_t)OW * OH));
  half8_t v = zero_half8();
  if (oct < 6) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int col = oct * 8 + e, tap = col / 3, c = col - tap * 3;
      const int iy = 2 * oy - 1 + (tap >> 2), ix = 2 * ox - 1 + (tap & 3);
      if (iy >= 0 && iy < H && ix >= 0 && ix < W) v[e] = (half_t)img[(((size_t)b * 3 + c) * H + iy) * W + ix];
    }
  }
  st_half8(P + m * ldp + oct * 8, v);
}

// y = Y[:, 0] -> y_out [B][1][H][W] (float) and / or mask [B][3][H][W] = (1 - y < 0.5 ? 0 : 1) on all three channels
__global__ __launch_bounds__(256) void tail_kernel(const half_t* Y, int ldy, float* y_out, float* mask, int B, size_t HW) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)B * HW) return;
  const float y = (float)Y[i * ldy];
  if (y_out) y_out[i] = y;
  if (mask) {
    const float v = (1.f - y) < 0.5f ? 0.f : 1.f;
    const size_t b = i / HW, px = i - b * HW;
    float* o = mask + b * 3 * HW + px;
    o[0] = v; o[HW] = v; o[2 * HW] = v;
  }
}

}  // namespace

extern "C" size_t skg_instnorm_scratch_floats(int rows, int HW, int C) {
  if (rows <= 0 || HW <= 0 || C <= 0) return 0;
  const int nslab = skg_cdiv(HW, in_slab(HW));
  return nslab == 1 ? 0 : (size_t)rows * nslab * C * 2 + (size_t)rows * C * 2;
}

extern "C" int skg_instnorm_act_f16(const void* X, int ldx, int rows, int HW, int C, float eps, int identity, void* Y0, int ldy0,
                                    float slope0, void* Y1, int ldy1, float slope1, float* scratch, void* stream) {
  SKG_REQUIRE(X && rows > 0 && rows <= 65535 && HW > 0 && C > 0 && C % IN_CW == 0 && C / IN_CW <= 65535 && (Y0 || Y1) && eps > 0.f);
  SKG_REQUIRE(ldx % 8 == 0 && ldx >= C && skg_aligned(X, 16));
  SKG_REQUIRE(!Y0 || (ldy0 % 8 == 0 && ldy0 >= C && skg_aligned(Y0, 16)));
  SKG_REQUIRE(!Y1 || (ldy1 % 8 == 0 && ldy1 >= C && skg_aligned(Y1, 16)));
  InParams p{};
  p.slab = in_slab(HW);
  p.nslab = skg_cdiv(HW, p.slab);
  SKG_REQUIRE(identity || p.nslab == 1 || (scratch && skg_aligned(scratch, 4)));
  p.X = (const half_t*)X; p.ldx = ldx; p.HW = HW; p.C = C; p.eps = eps;
  p.Y0 = (half_t*)Y0; p.ldy0 = ldy0; p.slope0 = slope0;
  p.Y1 = (half_t*)Y1; p.ldy1 = ldy1; p.slope1 = slope1;
  p.partial = scratch;
  p.stats = scratch ? scratch + (size_t)rows * p.nslab * C * 2 : nullptr;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(p.nslab, C / IN_CW, rows), block(IN_THREADS);
  if (identity) {
    hipLaunchKernelGGL(instnorm_kernel<IN_IDENTITY>, grid, block, 0, st, p);
  } else if (p.nslab == 1) {
    hipLaunchKernelGGL(instnorm_kernel<IN_FUSED>, grid, block, 0, st, p);
  } else {
    hipLaunchKernelGGL(instnorm_kernel<IN_PARTIAL>, grid, block, 0, st, p);
    hipLaunchKernelGGL(instnorm_finalize_kernel, dim3(C / IN_CW, rows), block, 0, st, p);
    hipLaunchKernelGGL(instnorm_kernel<IN_APPLY>, grid, block, 0, st, p);
  }
  SKG_CHECK_LAUNCH("skg_instnorm_act_f16");
  return SKG_OK;
}

extern "C" int skg_convt4x4s2_f16(const void* X, int ldx, const void* Wpp, void* Y, int ldy, int rows, int IH, int IW, int Cin,
                                  int Cout, const void* bias, int epilogue, void* stream) {
  SKG_REQUIRE(epilogue == SKG_CONVT_EPI_NONE || epilogue == SKG_CONVT_EPI_TANH);
  const int rc = skg_conv3x3_up2_f16(X, ldx, Wpp, Y, nullptr, ldy, rows, IH, IW, Cin, Cout, 0, bias, stream);
  if (rc != SKG_OK || epilogue == SKG_CONVT_EPI_NONE) return rc;
  const size_t M = (size_t)rows * 4 * IH * IW, n = M * (Cout / 8);
  hipLaunchKernelGGL(tanh_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (half_t*)Y, ldy, M, Cout / 8);
  SKG_CHECK_LAUNCH("skg_convt4x4s2_f16 (tanh)");
  return SKG_OK;
}

extern "C" int skg_a2s_patch_f16(const float* img, void* P, int ldp, int B, int H, int W, void* stream) {
  SKG_REQUIRE(img && P && B > 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0 && ldp % 8 == 0 && ldp >= 64 && skg_aligned(P, 16) &&
              skg_aligned(img, 4));
  const size_t n = (size_t)B * (H / 2) * (W / 2) * 8;
  SKG_REQUIRE((n + 255) / 256 < 0x7fffffffull);
  hipLaunchKernelGGL(patch_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, img, (half_t*)P, ldp, B, H, W);
  SKG_CHECK_LAUNCH("skg_a2s_patch_f16");
  return SKG_OK;
}

extern "C" int skg_a2s_tail(const void* Y, int ldy, float* y_out, float* mask, int B, int H, int W, void* stream) {
  SKG_REQUIRE(Y && (y_out || mask) && B > 0 && H > 0 && W > 0 && ldy >= 1 && skg_aligned(Y, 2));
  const size_t n = (size_t)B * H * W;
  SKG_REQUIRE((n + 255) / 256 < 0x7fffffffull);
  hipLaunchKernelGGL(tail_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const half_t*)Y, ldy, y_out, mask, B,
                     (size_t)H * W);
  SKG_CHECK_LAUNCH("skg_a2s_tail");
  return SKG_OK;
}
