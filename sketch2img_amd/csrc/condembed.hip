// Small-channel 3x3 convolutions of the ControlNet hint encoder (diffusers ControlNetConditioningEmbedding) for gfx950.
//
// The encoder's first three layers run at the full PIXEL resolution with 3 and 16 input channels (3 -> 16, 16 -> 16, 16 -> 32 at
// stride 2).  The implicit GEMM of gemm.hip wants Cin % 32 == 0: padding the picture to 32 channels at 512 x 512 is ten times the
// bytes the layer needs to read.  These layers get a direct form of their own:
//
//   Y[(b, oy, ox)][n] = act(bias[n] + sum_{ky, kx, c} X[b][s oy + ky - 1][s ox + kx - 1][c] * W[n][ky][kx][c]),   s = 1 or 2
//
// as MFMAs with NO LDS and no staging: the K axis is (tap, channel) with the channel contiguous, so the 8 K values a lane feeds to
// a 16x16x32 f16 MFMA are 16 contiguous bytes of ONE input pixel (Cin = 16: K slice ks = taps 2 ks, 2 ks + 1; ten tap slots, the
// tenth has zero weights) or two taps of the fp32 NCHW picture packed as 4 channels each (Cin = 3: K = 16 tap slots x 4 = 64, two
// slices; the picture is read as it is, no conversion pass).  Lane (l16, g) loads the operand of pixel l16 directly from global
// memory - the 16 lanes of a group read 16 neighbouring pixels, 32 contiguous bytes each pair of groups: whole 512-byte runs - and
// the weights (at most [32][160] fp16 = 10 KB) live in registers for the life of the wave.  The MFMA is issued "swapped" as in
// gemm.hip (weights as A, activations as B), so a lane's four accumulators are four consecutive output channels of one pixel:
// bias and SiLU are applied in registers and the store is 8 bytes, 512 contiguous bytes per instruction and 16 pixels.
// A wave owns 64 consecutive output pixels (four 16-pixel tiles, their loads independent of each other); a workgroup 256.
#include "common.h"

namespace {

constexpr int TILES = 4;                 // 16-pixel tiles per wave
constexpr int WG_PIX = 4 * TILES * 16;   // output pixels per 256-thread workgroup

struct SmallConvParams {
  const void* X;        // CIN16: fp16 [B*IH*IW][ldx]; else fp32 [B][3][IH][IW]
  const half_t* Wp;     // [Cout][KP] fp16, packs.pack_conv_small
  const half_t* bias;   // [Cout] or null
  half_t* Y;            // [B*OH*OW][ldy]
  int ldx, ldy, B, IH, IW, OH, OW, stride, silu;
  long M;               // B*OH*OW
};

// CIN16: 16 fp16 NHWC input channels (KS = 5 K slices of two taps), else the 3-channel fp32 NCHW picture (KS = 2 slices of
// eight 4-channel tap slots).  NT: 16-channel output tiles (Cout = 16 NT).
template <bool CIN16, int NT>
__global__ __launch_bounds__(256) void conv3x3_small_kernel(const SmallConvParams p) {
  constexpr int KS = CIN16 ? 5 : 2;
  constexpr int KP = KS * 32;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, l16 = lane & 15;

  half8_t wf[KS][NT];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks)
#pragma unroll
    for (int j = 0; j < NT; ++j) wf[ks][j] = ld_half8(p.Wp + (size_t)(j * 16 + l16) * KP + ks * 32 + g * 8);

  const long mw = (long)blockIdx.x * WG_PIX + wave * (TILES * 16);
  float4_t acc[TILES][NT];
#pragma unroll
  for (int t = 0; t < TILES; ++t) {
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[t][j] = float4_t{0.f, 0.f, 0.f, 0.f};
    const long m = mw + t * 16 + l16;
    const bool mok = m < p.M;
    const long mm = mok ? m : 0;
    const int ohw = p.OH * p.OW;
    const int b = (int)(mm / ohw);
    const int r = (int)(mm - (long)b * ohw);
    const int oy = r / p.OW, ox = r - oy * p.OW;
    const int y0 = oy * p.stride - 1, x0 = ox * p.stride - 1;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      half8_t xf = zero_half8();
      if constexpr (CIN16) {
        const int tap = 2 * ks + (g >> 1);
        const int ky = tap / 3, kx = tap - 3 * ky;
        const int iy = y0 + ky, ix = x0 + kx;
        if (mok && tap < 9 && iy >= 0 && iy < p.IH && ix >= 0 && ix < p.IW)
          xf = ld_half8(reinterpret_cast<const half_t*>(p.X) + ((size_t)b * p.IH * p.IW + (size_t)iy * p.IW + ix) * p.ldx + (g & 1) * 8);
      } else {
        const float* const img = reinterpret_cast<const float*>(p.X) + (size_t)b * 3 * p.IH * p.IW;
        const size_t plane = (size_t)p.IH * p.IW;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const int tap = ks * 8 + 2 * g + q;
          const int ky = tap / 3, kx = tap - 3 * ky;
          const int iy = y0 + ky, ix = x0 + kx;
          if (mok && tap < 9 && iy >= 0 && iy < p.IH && ix >= 0 && ix < p.IW) {
            const float* const px = img + (size_t)iy * p.IW + ix;
            xf[q * 4 + 0] = (half_t)px[0];
            xf[q * 4 + 1] = (half_t)px[plane];
            xf[q * 4 + 2] = (half_t)px[2 * plane];
          }
        }
      }
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[ks][j], xf, acc[t][j], 0, 0, 0);
    }
  }

  // ---- epilogue: lane holds Y[m = .. + l16][n = 16 j + 4 g .. + 3] ------------------------------------------------------
#pragma unroll
  for (int t = 0; t < TILES; ++t) {
    const long m = mw + t * 16 + l16;
    if (m >= p.M) continue;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int n = j * 16 + g * 4;
      float4_t v = acc[t][j];
      if (p.bias) {
        const half4_t bz = ld_half4(p.bias + n);
        v[0] += (float)bz[0]; v[1] += (float)bz[1]; v[2] += (float)bz[2]; v[3] += (float)bz[3];
      }
      if (p.silu) {
        v[0] = silu_f(v[0]); v[1] = silu_f(v[1]); v[2] = silu_f(v[2]); v[3] = silu_f(v[3]);
      }
      const half4_t o = {(half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3]};
      st_half4(p.Y + (size_t)m * p.ldy + n, o);
    }
  }
}

}  // namespace

extern "C" int skg_conv3x3_small_f16(const void* X, int ldx, const void* Wp, void* Y, int ldy, int B, int IH, int IW, int Cin, int Cout,
                                     int stride, const void* bias, int silu, void* stream) {
  SKG_REQUIRE(X && Wp && Y && B > 0 && IH > 0 && IW > 0 && (Cin == 3 || Cin == 16) && (Cout == 16 || Cout == 32));
  SKG_REQUIRE(stride == 1 || (stride == 2 && IH % 2 == 0 && IW % 2 == 0));
  SKG_REQUIRE(ldy % 4 == 0 && ldy >= Cout && skg_aligned(Y, 8) && skg_aligned(Wp, 16) && (!bias || skg_aligned(bias, 8)));
  SKG_REQUIRE(Cin == 3 ? skg_aligned(X, 4) : (ldx % 8 == 0 && ldx >= 16 && skg_aligned(X, 16)));
  SmallConvParams p{};
  p.X = X; p.Wp = (const half_t*)Wp; p.bias = (const half_t*)bias; p.Y = (half_t*)Y;
  p.ldx = ldx; p.ldy = ldy; p.B = B; p.IH = IH; p.IW = IW; p.OH = IH / stride; p.OW = IW / stride; p.stride = stride; p.silu = silu ? 1 : 0;
  p.M = (long)B * p.OH * p.OW;
  const long blocks = (p.M + WG_PIX - 1) / WG_PIX;
  SKG_REQUIRE(blocks < 0x7fffffffl && (long)p.OH * p.OW < 0x7fffffffl);
  const dim3 grid((unsigned)blocks), blk(256);
  hipStream_t st = (hipStream_t)stream;
  if (Cin == 16 && Cout == 16) hipLaunchKernelGGL((conv3x3_small_kernel<true, 1>), grid, blk, 0, st, p);
  else if (Cin == 16) hipLaunchKernelGGL((conv3x3_small_kernel<true, 2>), grid, blk, 0, st, p);
  else if (Cout == 16) hipLaunchKernelGGL((conv3x3_small_kernel<false, 1>), grid, blk, 0, st, p);
  else hipLaunchKernelGGL((conv3x3_small_kernel<false, 2>), grid, blk, 0, st, p);
  SKG_CHECK_LAUNCH("skg_conv3x3_small_f16");
  return SKG_OK;
}
