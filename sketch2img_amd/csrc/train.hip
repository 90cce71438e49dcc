// Weight-gradient kernels of the injected-attention (SatMixin) training step (sketch2img_amd/sat_train.py).
//
// skg_wgrad_f16:  dW[N][K] (fp32) = or += alpha * dY^T . X, optionally db[N] = or += alpha * colsum(dY) in the same pass.
//   dY [M][ldy], X [M][ldx] are fp16 ROW-major (column views of wider buffers are fine); the contraction runs over the M rows.
//   Neither operand is transposed in memory: a workgroup stages 64-row tiles of both in LDS as they are and every MFMA fragment
//   - dY^T rows as the A operand, X^T columns as the B operand - comes out of them through the gfx950 LDS transpose read
//   (ds_read_b64_tr_b16), the way the attention backward reads Q^T / dO^T.  Both operands use the SAME k-slot <-> row map
//   (slot (g, i) of 32-row step s = row 32 s + 16 (i >> 2) + 4 g + (i & 3)), which is all the MFMA needs.
//   Tiling: a workgroup (4 waves) owns a 32 (n) x 64 (k) tile of dW and one contiguous range of 64-row tiles of M; wave w owns
//   k columns 16 w .. 16 w + 15 and both 16-row n sub-tiles (two fp32 accumulators).  The outputs are tiny (C x C ... C x 1024)
//   and M is long, so M is split over blockIdx.z; every split writes its fp32 slab [split][N][K] (and [split][N] for db) to the
//   caller's scratch and a second launch folds the slabs in ascending split order, applies alpha and stores or accumulates.
//   No floating-point atomics anywhere: the result is bit-repeatable.
//   LDS image: pitches 48 (dY) and 80 (X) halves, both = 16 (mod 32): conflict-free for the transposed read (8 rows x 32 bytes
//   per 32-lane half land on distinct banks) and every lane address is a multiple of 8 bytes (the transposed read returns wrong
//   data off that alignment).  Rows behind M and columns behind N / K are ZERO-filled in LDS, never masked: the transposed read
//   needs every lane of the wave active.
//
// skg_layernorm_param_grads:  dgamma[c] = or += sum_rows dY * xhat, dbeta[c] = or += sum_rows dY from X, dY and the stored
//   (mean, rstd) of skg_layernorm_fwd; two stages (row chunks -> fixed-order fold), fp32 out.
#include "common.h"

namespace {

typedef __fp16 fp16x4_t __attribute__((__vector_size__(4 * sizeof(__fp16))));
__device__ __forceinline__ half4_t tr_read4(const half_t* p) {
  const fp16x4_t r = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fp16x4_t*)(p));
  return __builtin_bit_cast(half4_t, r);
}
// fragment of 16 columns (16 u ..) x the 32 rows of step s out of a row-major tile [64][VP]; base = tile + (4 g + (l16 >> 2)) VP + 4 (l16 & 3)
template <int VP>
__device__ __forceinline__ half8_t tfrag_rows(const half_t* base, int u, int s) {
  const half4_t lo = tr_read4(base + (32 * s) * VP + 16 * u), hi = tr_read4(base + (32 * s + 16) * VP + 16 * u);
  half8_t f = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return f;
}

constexpr int WG_TN = 32, WG_TK = 64, WG_TM = 64;
constexpr int WG_YP = WG_TN + 16, WG_XP = WG_TK + 16;
constexpr int WG_MAX_SPLITS = 64;

// m-tiles per split and number of splits: enough workgroups to fill the chip, never more than WG_MAX_SPLITS slabs
inline void wgrad_plan(int M, int N, int K, int* per, int* splits) {
  const int tiles = skg_cdiv(N, WG_TN) * skg_cdiv(K, WG_TK);
  const int mt = skg_cdiv(M, WG_TM);
  int want = skg_cdiv(512, tiles);
  if (want > WG_MAX_SPLITS) want = WG_MAX_SPLITS;
  if (want > mt) want = mt;
  if (want < 1) want = 1;
  *per = skg_cdiv(mt, want);
  *splits = skg_cdiv(mt, *per);
}

__global__ __launch_bounds__(256) void wgrad_partial_kernel(const half_t* __restrict__ dY, int ldy, const half_t* __restrict__ X, int ldx,
                                                            int M, int N, int K, int per, float* __restrict__ slab,
                                                            float* __restrict__ bslab) {
  __shared__ __attribute__((aligned(16))) half_t Ys[WG_TM * WG_YP];
  __shared__ __attribute__((aligned(16))) half_t Xs[WG_TM * WG_XP];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l16 = lane & 15, g = lane >> 4;
  const int k0 = blockIdx.x * WG_TK, n0 = blockIdx.y * WG_TN, split = blockIdx.z;
  const int mt0 = split * per, mt1 = min((M + WG_TM - 1) / WG_TM, mt0 + per);
  // staging: dY tile 64 x 32 = 256 pieces of 8 halves (one per thread), X tile 64 x 64 = 512 pieces (two per thread)
  const int yr = threadIdx.x >> 2, yc = (threadIdx.x & 3) * 8;
  const int xr = threadIdx.x >> 3, xc = (threadIdx.x & 7) * 8;      // rows xr and xr + 32
  const bool yok = n0 + yc < N, xok = k0 + xc < K;                  // N, K are multiples of 8: a piece is inside or outside
  const int tlane = (4 * g + (l16 >> 2));
  const half_t* ybase = Ys + tlane * WG_YP + 4 * (l16 & 3);
  const half_t* xbase = Xs + tlane * WG_XP + 4 * (l16 & 3);
  float4_t acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;                                                  // threads 0 .. 31 of the k-tile-0 workgroups: colsum of dY
  for (int mt = mt0; mt < mt1; ++mt) {
    const int m0 = mt * WG_TM;
    half8_t yv = zero_half8(), xv0 = zero_half8(), xv1 = zero_half8();
    if (yok && m0 + yr < M) yv = ld_half8(dY + (size_t)(m0 + yr) * ldy + n0 + yc);
    if (xok && m0 + xr < M) xv0 = ld_half8(X + (size_t)(m0 + xr) * ldx + k0 + xc);
    if (xok && m0 + xr + 32 < M) xv1 = ld_half8(X + (size_t)(m0 + xr + 32) * ldx + k0 + xc);
    __syncthreads();                                                 // the previous tile's reads are done
    st_half8(Ys + yr * WG_YP + yc, yv);
    st_half8(Xs + xr * WG_XP + xc, xv0);
    st_half8(Xs + (xr + 32) * WG_XP + xc, xv1);
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const half8_t b = tfrag_rows<WG_XP>(xbase, wave, s);
      const half8_t a0 = tfrag_rows<WG_YP>(ybase, 0, s), a1 = tfrag_rows<WG_YP>(ybase, 1, s);
      acc0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, b, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, b, acc1, 0, 0, 0);
    }
    if (bslab && blockIdx.x == 0 && threadIdx.x < WG_TN) {           // rows in ascending order: fixed summation order
      for (int r = 0; r < WG_TM; ++r) bsum += (float)Ys[r * WG_YP + threadIdx.x];
    }
  }
  // C layout: lane (l16, g) holds rows 4 g + r (n) of column l16 (k)
  const int k = k0 + 16 * wave + l16;
  if (k < K) {
    float* out = slab + (size_t)split * N * K;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int na = n0 + 4 * g + r, nb = na + 16;
      if (na < N) out[(size_t)na * K + k] = acc0[r];
      if (nb < N) out[(size_t)nb * K + k] = acc1[r];
    }
  }
  if (bslab && blockIdx.x == 0 && threadIdx.x < WG_TN && n0 + (int)threadIdx.x < N)
    bslab[(size_t)split * N + n0 + threadIdx.x] = bsum;
}

// out[i] = (accumulate ? out[i] : 0) + alpha * sum_{s ascending} slab[s][i]
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ slab, size_t n, int splits, float alpha,
                                                           int accumulate, float* __restrict__ out) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    float t = 0.f;
    for (int s = 0; s < splits; ++s) t += slab[(size_t)s * n + i];
    t *= alpha;
    out[i] = accumulate ? out[i] + t : t;
  }
}

// ---- LayerNorm parameter gradients ------------------------------------------------------------------------------------------
constexpr int LNP_CHUNKS = 32;
__global__ __launch_bounds__(256) void ln_param_partial_kernel(const half_t* __restrict__ X, int ldx, const half_t* __restrict__ dY,
                                                               int lddy, int M, int C, const float* __restrict__ stats,
                                                               float* __restrict__ partial) {
  __shared__ float red[256][16];
  const int c0 = blockIdx.x * 8, chunk = blockIdx.y;
  const int per = (M + LNP_CHUNKS - 1) / LNP_CHUNKS;
  const int r0 = chunk * per, r1 = min(M, r0 + per);
  float ag[8] = {0, 0, 0, 0, 0, 0, 0, 0}, ab[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int r = r0 + threadIdx.x; r < r1; r += 256) {
    const half8_t x = ld_half8(X + (size_t)r * ldx + c0), d = ld_half8(dY + (size_t)r * lddy + c0);
    const float mean = stats[(size_t)r * 2], rstd = stats[(size_t)r * 2 + 1];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      ag[j] += (float)d[j] * (((float)x[j] - mean) * rstd);
      ab[j] += (float)d[j];
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) { red[threadIdx.x][j] = ag[j]; red[threadIdx.x][8 + j] = ab[j]; }
  __syncthreads();
  if (threadIdx.x < 16) {          // fixed-order fold: deterministic
    float t = 0.f;
    for (int i = 0; i < 256; ++i) t += red[i][threadIdx.x];
    // partial[chunk][0 = gamma, 1 = beta][C]
    partial[((size_t)chunk * 2 + (threadIdx.x >> 3)) * C + c0 + (threadIdx.x & 7)] = t;
  }
}
__global__ void ln_param_final_kernel(const float* __restrict__ partial, int C, float scale, int accumulate,
                                      float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float s1 = 0.f, s2 = 0.f;
  for (int k = 0; k < LNP_CHUNKS; ++k) {
    s1 += partial[((size_t)k * 2) * C + c];
    s2 += partial[((size_t)k * 2 + 1) * C + c];
  }
  s1 *= scale; s2 *= scale;
  dgamma[c] = accumulate ? dgamma[c] + s1 : s1;
  dbeta[c] = accumulate ? dbeta[c] + s2 : s2;
}

}  // namespace

extern "C" size_t skg_wgrad_scratch_floats(int M, int N, int K) {
  if (M < 1 || N < 1 || K < 1) return 0;
  int per, splits;
  wgrad_plan(M, N, K, &per, &splits);
  return (size_t)splits * ((size_t)N * K + N);
}

extern "C" int skg_wgrad_f16(const void* dY, int ldy, const void* X, int ldx, int M, int N, int K, float alpha, int accumulate,
                             float* dW, float* db, float* scratch, void* stream) {
  SKG_REQUIRE(dY && X && dW && scratch && M >= 1 && N >= 8 && K >= 8 && N % 8 == 0 && K % 8 == 0);
  SKG_REQUIRE(ldy % 8 == 0 && ldx % 8 == 0 && ldy >= N && ldx >= K && skg_aligned(dY, 16) && skg_aligned(X, 16));
  SKG_REQUIRE(skg_aligned(dW, 4) && skg_aligned(scratch, 4) && (!db || skg_aligned(db, 4)));
  int per, splits;
  wgrad_plan(M, N, K, &per, &splits);
  hipStream_t st = (hipStream_t)stream;
  float* bslab = db ? scratch + (size_t)splits * N * K : nullptr;
  hipLaunchKernelGGL(wgrad_partial_kernel, dim3(skg_cdiv(K, WG_TK), skg_cdiv(N, WG_TN), splits), dim3(256), 0, st,
                     (const half_t*)dY, ldy, (const half_t*)X, ldx, M, N, K, per, scratch, bslab);
  const size_t n = (size_t)N * K;
  size_t blocks = (n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, st, scratch, n, splits, alpha, accumulate, dW);
  if (db)
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(skg_cdiv(N, 256)), dim3(256), 0, st, bslab, (size_t)N, splits, alpha, accumulate, db);
  SKG_CHECK_LAUNCH("skg_wgrad_f16");
  return SKG_OK;
}

extern "C" size_t skg_layernorm_param_scratch_floats(int C) { return (size_t)LNP_CHUNKS * 2 * (C > 0 ? C : 0); }

extern "C" int skg_layernorm_param_grads(const void* X, int ldx, const void* dY, int lddy, int M, int C, const float* stats,
                                         float scale, int accumulate, float* dgamma, float* dbeta, float* scratch, void* stream) {
  SKG_REQUIRE(X && dY && stats && dgamma && dbeta && scratch && M >= 1 && C >= 8 && C % 8 == 0);
  SKG_REQUIRE(ldx % 8 == 0 && lddy % 8 == 0 && ldx >= C && lddy >= C && skg_aligned(X, 16) && skg_aligned(dY, 16));
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ln_param_partial_kernel, dim3(C / 8, LNP_CHUNKS), dim3(256), 0, st, (const half_t*)X, ldx, (const half_t*)dY,
                     lddy, M, C, stats, scratch);
  hipLaunchKernelGGL(ln_param_final_kernel, dim3(skg_cdiv(C, 128)), dim3(128), 0, st, scratch, C, scale, accumulate, dgamma, dbeta);
  SKG_CHECK_LAUNCH("skg_layernorm_param_grads");
  return SKG_OK;
}
