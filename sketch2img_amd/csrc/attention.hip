// Flash-style fused attention for gfx950, fp16 in / fp32 accumulate: forward, dQ and dK/dV.
//
// Formulation ("swapped" products, so every softmax statistic is lane-local or a 2-step shuffle):
// a wave owns 16 query rows and computes S^T = K Q^T with 16x16x32 f16 MFMAs, K rows as the A
// operand (from LDS) and the wave's Q rows as the B operand (registers, loaded once).  In the MFMA
// C layout lane (q = lane & 15, g = lane >> 4) then holds S^T[kv = 16 t + 4 g + r][q] in register r of
// tile t: all 16 scores a lane holds belong to ONE query, so max / sum are in-lane plus two xor
// shuffles (16, 32), and the online-softmax rescale factor is a per-lane scalar.
// For the second product O^T = V^T P^T the probabilities are used straight from those registers as
// the B operand: element i of lane (q, g) is declared to be k-slot (g, i) <-> key
// 32 s + 16 (i >> 2) + 4 g + (i & 3); the MFMA only needs A and B to agree on the k <-> key map, so
// the A operand (V^T rows = head-dim index) is read with the same map: two ds_read_b64_tr_b16 per fragment out of
// the ROW-MAJOR V tile (SKG_ATTN_ROWV; tfrag_rows below), or two 8-byte reads out of a tile stored transposed
// when the caller hands over V^T (no SKG_ATTN_ROWV).  No P round trip through LDS, no cross-lane transposes.
// The backward kernels read K^T, Q^T and dO^T fragments the same way from the row tiles they stage anyway, so
// nothing on the UNet path needs skg_transpose_f16 any more.
//
// Block = 4 waves = 64 query rows (forward, dQ) or 64 key rows (dK/dV); KV / Q tiles of 64 rows are
// staged in LDS.  Pitches: row tiles [64][32 KS + 16] (ds_read_b128 is served in four NON-contiguous 16-lane groups,
// MI355X_MICROARCH.md section LDS: a pitch of 16 or 48 mod 64 halves puts each group on 16 distinct 16-byte slots; the
// round-1 pitch 32 KS + 8 was 2-way conflicted - SQ_LDS_BANK_CONFLICT = 42 % of SQ_LDS_IDX_ACTIVE), transposed tiles
// [d][72] read with ds_read_b64 pairs (two 32-lane groups: conflict-free at 72).
#include "common.h"
#include <stdlib.h>
#include <type_traits>

namespace {

struct AttnParams {
  const half_t* Q; int ldq;
  const half_t* K; int ldk;
  const half_t* V; int ldv;       // row-major V (backward)
  const half_t* Vt; int ldvt;     // forward: V^T (skg_attn_fwd, also causal) or the row-major V and its pitch (SKG_ATTN_ROWV)
  const half_t* dO; int lddo;
  half_t* O; int ldo;             // fwd: O; dq: dQ; dkv: dK
  half_t* O2; int ldo2;           // dkv: dV
  float* lse;                     // [batch][heads][Nq]
  const float* delta;             // [batch][heads][Nq]
  const half_t* Of; int ldof;     // dq with the delta prologue (skg_attn_bwd_dq without delta): the forward's O, and where delta is also stored
  float* delta_out;
  int batch, heads, Nq, Nkv, kv_stride, dh;
  float scale;
  int nx;                         // workgroups per (batch row, head): launches are 1-D, nx * heads * batch
};

// Workgroup -> (tile, head, batch row).  Workgroup b runs on XCD b % 8 and every XCD has its own L2, so all nx
// workgroups of one (row, head) - which stream the same K / V (or Q / dO) panels - are placed on ONE XCD: pair
// = 8 * (slot / nx) + xcd.  With the plain x-fastest 3-D grid the 32 query tiles of a head were spread over all 8
// XCDs and each L2 fetched the panel again (rocprofv3 FETCH_SIZE: 428 MB per forward launch at 64x64, 2.5 x the
// algorithmic bytes).  Falls back to the plain order when heads * batch is not a multiple of 8.
struct BlkMap { int bx, h, b; };
__device__ __forceinline__ BlkMap attn_block_map(const AttnParams& p) {
  const int lid = blockIdx.x, nx = p.nx;
  const int pairs = p.heads * p.batch;
  int pair, bx;
  if ((pairs & 7) == 0) {
    const int xcd = lid & 7, slot = lid >> 3;
    const int grp = slot / nx;
    pair = grp * 8 + xcd;
    bx = slot - grp * nx;
  } else {
    pair = lid / nx;
    bx = lid - pair * nx;
  }
  const int b = pair / p.heads;
  return {bx, pair - b * p.heads, b};
}

constexpr float NEG_BIG = -1.0e30f;

#ifdef SKG_PHASES
// profiling build only (make phases; tools/attn_phases.py): per-wave cycle sums of the forward kernel's phases
__device__ unsigned long long g_attn_phase[1 << 16][8];
#define ATT_T(x) const unsigned long long x = __builtin_readcyclecounter()
#define ATT_ACC(i, a, b) att_acc[i] += (b) - (a)
#else
#define ATT_T(x) do { } while (0)
#define ATT_ACC(i, a, b) do { } while (0)
#endif

// max of three without the canonicalising v_max_f32 x, x, x that fmaxf() puts in front of every MFMA result (the
// compiler cannot prove an MFMA output is not a signalling NaN): 16 scores reduce in 8 VALU instead of 31
__device__ __forceinline__ float max3f(float a, float b, float c) {
  float r;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;
constexpr int TP = 72;   // pitch (halves) of the transposed tiles [d][64 + 8]

// A-operand fragment of a transposed tile for k-step s: head-dim row (16 u + l16), keys by the map above
__device__ __forceinline__ half8_t tfrag(const half_t* tile, int u, int s, int l16, int g) {
  const half_t* p = tile + (u * 16 + l16) * TP + 32 * s + 4 * g;
  const half4_t lo = ld_half4(p), hi = ld_half4(p + 16);
  half8_t f = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return f;
}
// The same fragment out of a ROW-MAJOR tile [key][VP] through the gfx950 transpose read: in a 16-lane group lane i hands
// in the address of 4 contiguous halves - row i >> 2, columns 4 (i & 3) .. + 3 of a [4][16] block - and receives column
// i of that block, rows 0 .. 3 (tools/ubench/tr_probe.hip).  Group g of fragment (u, s) takes the block of keys
// 32 s + 16 hh + 4 g .. + 3 x head-dim columns 16 u .. + 15, hh = 0 / 1: exactly the k <-> key map above, so V (and K, Q,
// dO in the backward kernels) needs no transposed copy in HBM.  `base` = tile + (4 g + (l16 >> 2)) * VP + 4 (l16 & 3).
// Banks: 8 key rows x 32 bytes per 32-lane group are conflict-free when VP = 16 (mod 32) halves.
typedef __fp16 fp16x4_t __attribute__((__vector_size__(4 * sizeof(__fp16))));
__device__ __forceinline__ half4_t tr_read(const half_t* p) {
  const fp16x4_t r = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fp16x4_t*)(p));
  return __builtin_bit_cast(half4_t, r);
}
template <int VP>
__device__ __forceinline__ half8_t tfrag_rows(const half_t* base, int u, int s) {
  const half4_t lo = tr_read(base + (32 * s) * VP + 16 * u), hi = tr_read(base + (32 * s + 16) * VP + 16 * u);
  half8_t f = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return f;
}
constexpr int vrow_pitch(int nd) { return nd * 16 + ((nd & 1) ? 0 : 16); }      // = 16 (mod 32) halves, >= 16 nd
// pack score-layout registers (4 tiles x 4) into the two B-operand fragments
__device__ __forceinline__ void pack_p(const float4_t (&s)[4], half8_t (&pb)[2]) {
#pragma unroll
  for (int k2 = 0; k2 < 2; ++k2)
#pragma unroll
    for (int i = 0; i < 8; ++i) pb[k2][i] = (half_t)s[2 * k2 + (i >> 2)][i & 3];
}

// register staging of [64][dh] row tiles (global -> VGPR now, VGPR -> LDS later)
template <int KS>
struct RowRegs { half8_t v[KS]; };               // 64 * KS*4 pieces / 256 threads

template <int KS>
__device__ __forceinline__ void rows_store(const RowRegs<KS>& r, half_t* __restrict__ dst) {
  constexpr int KP = KS * 32 + 16;      // pitch = 16 or 48 (mod 64) halves: conflict-free for the 4 x 16-lane groups of ds_read_b128 (+ 8 is 2-way)
  constexpr int PPR = KS * 4;
#pragma unroll
  for (int q = 0; q < KS; ++q) {
    const int pi = threadIdx.x + q * 256;
    const int row = pi / PPR, pc = (pi - row * PPR) * 8;
    st_half8(dst + row * KP + pc, r.v[q]);
  }
}
// -------------------------------------------------------------------------------------------------
// register staging of one K tile ([64][dh] rows) and one V tile (transposed [dh][64], or row-major [64][VP] with VROW)
// per workgroup.  ONES (d = 40): the first padding row of V^T / column dh of the row-major tile is 1.0, so row dh of
// O^T = V^T P^T accumulates the softmax denominator sum_k p[k] on the matrix pipe instead of the VALU.
template <int KS, int ND>
struct KVRegs {
  static constexpr int NK = KS;                 // 64 * KS*4 pieces / 256 threads
  static constexpr int NV = (ND + 1) / 2;       // ND*16*8 pieces / 256 threads
  half8_t k[NK], v[NV];
};

template <int KS, int ND, bool VROW = false>
__device__ __forceinline__ void kv_store(const KVRegs<KS, ND>& r, half_t* __restrict__ Ks, half_t* __restrict__ Vs) {
  constexpr int KP = KS * 32 + 16;      // pitch = 16 or 48 (mod 64) halves: conflict-free for the 4 x 16-lane groups of ds_read_b128 (+ 8 is 2-way)
  constexpr int PPR = KS * 4;
#pragma unroll
  for (int q = 0; q < KVRegs<KS, ND>::NK; ++q) {
    const int pi = threadIdx.x + q * 256;
    const int row = pi / PPR, pc = (pi - row * PPR) * 8;
    st_half8(Ks + row * KP + pc, r.k[q]);
  }
#pragma unroll
  for (int q = 0; q < KVRegs<KS, ND>::NV; ++q) {
    const int pi = threadIdx.x + q * 256;
    if constexpr (VROW) {      // row-major V tile [64][VP]: 2 ND pieces per key row (a dense image when VP = 16 ND)
      constexpr int VP = vrow_pitch(ND);
      if (pi < ND * 128) st_half8(Vs + (pi / (2 * ND)) * VP + (pi % (2 * ND)) * 8, r.v[q]);
    } else {
      if (pi < ND * 128) st_half8(Vs + (pi >> 3) * TP + (pi & 7) * 8, r.v[q]);
    }
  }
}

// The same prefetch through buffer descriptors: every per-lane source offset is loop-invariant (row / column inside the
// tile, or an out-of-range constant for the zero-padded head-dim columns / rows), the tile position is a wave-uniform
// soffset and the descriptor's range check supplies the zeros behind the last key row - a prefetch is 2 * (KS + NV)
// instructions instead of ~15 VALU + 8 SALU per load of compare / select / zero-fill / exec masking (the round-2 counters:
// 140 VALU instructions per tile and wave of which only 32 + 16 + 20 are the softmax; VALU time ~ MFMA time at d = 40).
constexpr unsigned ATT_OOB = 0x80000000u;
template <int KS, int ND>
struct KVSrc {
  __amdgpu_buffer_rsrc_t rk, rv;
  unsigned ko[KVRegs<KS, ND>::NK], vo[KVRegs<KS, ND>::NV];
  int vcol[KVRegs<KS, ND>::NV];            // first key column of the lane's piece (ragged last tile only)
  unsigned ones;                           // bit q: piece q of this lane is the all-ones row (ONES)
};
template <int KS, int ND, bool ONES, bool VROW = false>
__device__ __forceinline__ KVSrc<KS, ND> kv_src(const half_t* Kb, int ldk, const half_t* Vb, int ldvt, int kvlim, int dh) {
  KVSrc<KS, ND> s;
  // K: rows of THIS batch row only (the next row's keys start right behind: the size is what cuts them off)
  s.rk = __builtin_amdgcn_make_buffer_rsrc((void*)Kb, 0, (unsigned)(((size_t)(kvlim - 1) * ldk + dh) * 2), 0x00020000);
  s.rv = __builtin_amdgcn_make_buffer_rsrc((void*)Vb, 0, (unsigned)((VROW ? (size_t)(kvlim - 1) * ldvt + dh
                                                                           : (size_t)(dh - 1) * ldvt + kvlim) * 2), 0x00020000);
  constexpr int PPR = KS * 4;
  s.ones = 0;
#pragma unroll
  for (int q = 0; q < KVRegs<KS, ND>::NK; ++q) {
    const int pi = threadIdx.x + q * 256;
    const int row = pi / PPR, pc = (pi - row * PPR) * 8;
    s.ko[q] = pc < dh ? (unsigned)(row * ldk + pc) * 2u : ATT_OOB;
  }
#pragma unroll
  for (int q = 0; q < KVRegs<KS, ND>::NV; ++q) {
    const int pi = threadIdx.x + q * 256;
    if constexpr (VROW) {      // ldvt is V's row pitch here; rows behind the last key read as zero by the range check
      const int row = pi / (2 * ND), pc = (pi % (2 * ND)) * 8;
      s.vo[q] = (pi < ND * 128 && pc < dh) ? (unsigned)(row * ldvt + pc) * 2u : ATT_OOB;
      s.vcol[q] = 0;
      if (ONES && pi < ND * 128 && pc == dh) s.ones |= 1u << q;      // column dh of every key row = 1.0
    } else {
      const int d = pi >> 3, pc = (pi & 7) * 8;
      s.vo[q] = (pi < ND * 128 && d < dh) ? (unsigned)(d * ldvt + pc) * 2u : ATT_OOB;
      s.vcol[q] = pc;
      if (ONES && d == dh) s.ones |= 1u << q;
    }
  }
  return s;
}
__device__ __forceinline__ half8_t buf_half8(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
  typedef unsigned u4 __attribute__((ext_vector_type(4)));
  const u4 v = __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0);
  return __builtin_bit_cast(half8_t, v);
}
template <int KS, int ND, bool ONES, bool VROW = false>
__device__ __forceinline__ void kv_load_buf(KVRegs<KS, ND>& r, const KVSrc<KS, ND>& s, int kv0, int ldk, int kvlim,
                                            int ldv = 0) {
  const unsigned sk = (unsigned)kv0 * (unsigned)ldk * 2u, sv = VROW ? (unsigned)kv0 * (unsigned)ldv * 2u : (unsigned)kv0 * 2u;
#pragma unroll
  for (int q = 0; q < KVRegs<KS, ND>::NK; ++q) r.k[q] = buf_half8(s.rk, s.ko[q], sk);
  if (VROW || kv0 + 64 <= kvlim) {         // wave-uniform
#pragma unroll
    for (int q = 0; q < KVRegs<KS, ND>::NV; ++q) r.v[q] = buf_half8(s.rv, s.vo[q], sv);
  } else {                                 // ragged last tile: key columns behind this batch row's keys read as zero
#pragma unroll
    for (int q = 0; q < KVRegs<KS, ND>::NV; ++q) r.v[q] = buf_half8(s.rv, kv0 + s.vcol[q] < kvlim ? s.vo[q] : ATT_OOB, sv);
  }
  if (ONES) {
    const half_t one = (half_t)1.f, zr = (half_t)0.f;
#pragma unroll
    for (int q = 0; q < KVRegs<KS, ND>::NV; ++q)
      if ((s.ones >> q) & 1u) r.v[q] = VROW ? half8_t{one, zr, zr, zr, zr, zr, zr, zr} : half8_t{one, one, one, one, one, one, one, one};
  }
}

// The backward kernels' row / transposed tiles through the same descriptors (see KVSrc)
template <int KS>
struct RowSrc { __amdgpu_buffer_rsrc_t r; unsigned o[KS]; };
template <int KS>
__device__ __forceinline__ RowSrc<KS> row_src(const half_t* src, int ld, int rlim, int dh) {
  RowSrc<KS> s;
  s.r = __builtin_amdgcn_make_buffer_rsrc((void*)src, 0, (unsigned)(((size_t)(rlim - 1) * ld + dh) * 2), 0x00020000);
  constexpr int PPR = KS * 4;
#pragma unroll
  for (int q = 0; q < KS; ++q) {
    const int pi = threadIdx.x + q * 256;
    const int row = pi / PPR, pc = (pi - row * PPR) * 8;
    s.o[q] = pc < dh ? (unsigned)(row * ld + pc) * 2u : ATT_OOB;
  }
  return s;
}
template <int KS>
__device__ __forceinline__ void rows_load_buf(RowRegs<KS>& r, const RowSrc<KS>& s, int ld, int r0) {
  const unsigned so = (unsigned)r0 * (unsigned)ld * 2u;
#pragma unroll
  for (int q = 0; q < KS; ++q) r.v[q] = buf_half8(s.r, s.o[q], so);
}
// Forward.  Per 64-key tile: issue the global loads of the NEXT tile into registers, run S^T = K Q^T,
// online softmax and O^T += V^T P^T on the current LDS tile, then (barrier) spill the prefetched
// registers into LDS: the HBM/L2 latency of tile t+1 hides under the MFMA + VALU work of tile t.
// Softmax arithmetic is kept to ~6 VALU per score: raw v_exp_f32 (arguments are <= 0, no range fix-up),
// scale folded into one FMA, masking only on a ragged last tile.
// CAUSAL (the CLIP text encoder, modules/pipeline.py:55-57 -> transformers CLIPTextModel): key j is visible to
// query i only when j <= i; a separate instantiation so the UNet's kernels carry no extra test.
// VAR (experiments / per-shape tuning): bit 0 = request every fragment of a tile up front (PRE), bit 1 = one register
// prefetch set instead of two (frees 16 VGPRs), bits 2-3 = waves per SIMD the register allocation is bounded for (0 = default)
template <int KS, int ND, int QT, bool CAUSAL = false, int VAR = 0, bool VROW = false>
__global__ __launch_bounds__(256, ((VAR >> 2) ? (VAR >> 2) : KS >= 5 ? 1 : (KS == 2 && ND == 3 && !CAUSAL && QT == 2) ? 4 : 2)) void attn_fwd_kernel(const AttnParams p) {
  // QT query tiles of 16 per wave: a workgroup covers 64 * QT queries, so every K / V^T fragment read from LDS
  // (and every byte of K/V streamed from L2) is used by QT MFMAs instead of one.
  constexpr int KP = KS * 32 + 16;      // pitch = 16 or 48 (mod 64) halves: conflict-free for the 4 x 16-lane groups of ds_read_b128 (+ 8 is 2-way)
  constexpr int VP = vrow_pitch(ND);    // VROW: p.Vt / p.ldvt are the ROW-MAJOR V and its pitch; the tile is kept [64][VP] and read transposing
  constexpr int KSZ = 64 * KP, VSZ = VROW ? 64 * VP : ND * 16 * TP;
  __shared__ __attribute__((aligned(16))) half_t lds[2 * (KSZ + VSZ)];      // two (K, V^T) stages
  half_t* const Ks0 = lds;
  half_t* const Vs0 = lds + KSZ;
  half_t* const Ks1 = lds + KSZ + VSZ;
  half_t* const Vs1 = lds + 2 * KSZ + VSZ;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l16 = lane & 15, g = lane >> 4;
  const BlkMap bm = attn_block_map(p);
  const int b = bm.b, h = bm.h;
  const int dh = p.dh;
  int q[QT];
  bool qok[QT];
  half8_t qf[QT][KS];
#pragma unroll
  for (int i = 0; i < QT; ++i) {
    q[i] = bm.bx * (64 * QT) + (wave * QT + i) * 16 + l16;
    qok[i] = q[i] < p.Nq;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int c = 32 * ks + 8 * g;
      qf[i][ks] = (qok[i] && c < dh) ? ld_half8(p.Q + (size_t)(b * p.Nq + q[i]) * p.ldq + h * dh + c) : zero_half8();
    }
  }
  // Q is pre-multiplied by scale * log2(e) (one fp16 rounding, the size of Q's own) and MINUS the reference maximum
  // rides in as the C operand of the first QK^T MFMA, so a score leaves the matrix pipe as  s*sc - m  and the softmax
  // is exp2 + max + pack per score: no FMA, no cross-lane traffic.  The reference m only has to stay within 2^8 of the
  // true running maximum (p <= 256 is exact enough in fp16, O and the denominator share the reference), so it moves
  // when a tile beats it by more than 8 (rare after the first tile) instead of on every new maximum.
  const float sc = p.scale * LOG2E;
#pragma unroll
  for (int i = 0; i < QT; ++i)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int j = 0; j < 8; ++j) qf[i][ks][j] = (half_t)((float)qf[i][ks][j] * sc);
  float4_t o[QT][ND];
  float4_t nm[QT];                  // minus the reference maximum (log2 domain), replicated: the MFMA C operand
  float l[QT];
#pragma unroll
  for (int i = 0; i < QT; ++i) {
    nm[i] = float4_t{0.f, 0.f, 0.f, 0.f}; l[i] = 0.f;
#pragma unroll
    for (int u = 0; u < ND; ++u) o[i][u] = float4_t{0.f, 0.f, 0.f, 0.f};
  }
  constexpr float REF_SLACK = 8.f;
  // (measured: requesting all fragments of a tile up front costs 14 VGPRs = the third wave per SIMD: 710 -> 767 us at
  // d = 40; the compiler's read-as-you-go order with three resident waves is faster.  Kept for experiments.)
  constexpr bool PRE = (VAR & 1) && KS <= 2 && 4 * KS * QT >= 2 * ND;
  constexpr int VREADS = 2;                                   // LDS instructions per V^T fragment (two ds_read_b64)
  // <2, 3> is dispatched for d = 40 only: 8 spare rows in the 48-row V^T tile -> the denominator comes out of the
  // PV MFMA (row 40 of O^T) and the 16 adds per tile and query tile leave the VALU, which bounds this head size
  constexpr bool ONES = (KS == 2 && ND == 3);

  const half_t* Kb = p.K + (size_t)b * p.kv_stride * p.ldk + h * dh;
  const half_t* Vb = VROW ? p.Vt + (size_t)b * p.kv_stride * p.ldvt + h * dh
                          : p.Vt + (size_t)h * dh * p.ldvt + (size_t)b * p.kv_stride;
  const int vlane = (4 * g + (l16 >> 2)) * VP + 4 * (l16 & 3);      // VROW: the lane's corner of every [4][16] block
  const int nt = (p.Nkv + 63) / 64;

#ifdef SKG_PHASES
  unsigned long long att_acc[6] = {0, 0, 0, 0, 0, 0};
#endif
  // one 64-key tile: S^T = K Q^T - m, online softmax, O^T += V^T P^T   (for the wave's QT query tiles)
  auto tile = [&](const half_t* __restrict__ Ks, const half_t* __restrict__ Vs, int kv0) {
    ATT_T(ta);
    float4_t s[QT][4];
    half8_t vf[ND][2];
    if constexpr (PRE) {
      // hipcc emits "2 ds_read -> s_waitcnt -> 4 MFMA" per 16 keys, i.e. one exposed LDS latency per group and the
      // V^T reads after the softmax.  Here every K fragment of the tile is requested up front and the V^T fragments
      // are requested under the QK^T MFMAs, so they land while the matrix pipe and then the softmax VALU work.
      half8_t kf[4][KS];
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) kf[t][ks] = ld_half8(Ks + (16 * t + l16) * KP + 32 * ks + 8 * g);
#pragma unroll
      for (int u = 0; u < ND; ++u)
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2) vf[u][k2] = VROW ? tfrag_rows<VP>(Vs + vlane, u, k2) : tfrag(Vs, u, k2, l16, g);
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
          for (int i = 0; i < QT; ++i)
            s[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[t][ks], qf[i][ks], ks == 0 ? nm[i] : s[i][t], 0, 0, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, 4 * KS, 0);            // all K fragment reads
#pragma unroll
      for (int r = 0; r < 2 * ND; ++r) {                                  // V^T reads woven under the first MFMAs
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, VREADS, 0);
      }
      __builtin_amdgcn_sched_group_barrier(0x008, 4 * KS * QT - 2 * ND, 0);
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const half8_t kf = ld_half8(Ks + (16 * t + l16) * KP + 32 * ks + 8 * g);
#pragma unroll
          for (int i = 0; i < QT; ++i)
            s[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf[i][ks], ks == 0 ? nm[i] : s[i][t], 0, 0, 0);
        }
      }
    }
    ATT_T(tb);
    ATT_ACC(0, ta, tb);                   // K fragment reads + QK^T MFMA issue
    const bool first = kv0 == 0;          // the reference starts at 0: the first tile always re-bases it
    half8_t pb[QT][2];
#pragma unroll
    for (int i = 0; i < QT; ++i) {
      if (CAUSAL || kv0 + 64 > p.Nkv) {          // ragged last tile only (wave-uniform)
        // key = kv0 + 4g + (16t + r): compare the compile-time part against per-lane limits computed in here, so
        // the full tiles carry no index arithmetic
        int lim = p.Nkv - kv0 - 4 * g;
        int qlim = CAUSAL ? q[i] - kv0 - 4 * g : 0;
        asm volatile("" : "+v"(lim), "+v"(qlim));      // keeps the 16 compares inside this (rare) branch
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (16 * t + r >= lim || (CAUSAL && 16 * t + r > qlim)) s[i][t][r] = NEG_BIG;
      }
      const float m0 = max3f(s[i][0][0], s[i][0][1], s[i][0][2]);
      const float m1 = max3f(s[i][0][3], s[i][1][0], s[i][1][1]);
      const float m2 = max3f(s[i][1][2], s[i][1][3], s[i][2][0]);
      const float m3 = max3f(s[i][2][1], s[i][2][2], s[i][2][3]);
      const float m4 = max3f(s[i][3][0], s[i][3][1], s[i][3][2]);
      float mx = max3f(max3f(m0, m1, m2), max3f(m3, m4, s[i][3][3]), m0);
      if (__builtin_amdgcn_ballot_w64(first || mx > REF_SLACK) != 0) {      // wave-uniform, rare after tile 0
        mx = max3f(mx, __shfl_xor(mx, 16, 64), mx);
        mx = max3f(mx, __shfl_xor(mx, 32, 64), mx);                         // the query's maximum over the tile
        const float delta = (first || mx > REF_SLACK) ? mx : 0.f;
        const float alpha = first ? 1.f : __builtin_amdgcn_exp2f(-delta);   // (o, l are still zero in tile 0)
        nm[i] -= delta;
        if (!ONES) l[i] *= alpha;
#pragma unroll
        for (int u = 0; u < ND; ++u) o[i][u] *= alpha;
#pragma unroll
        for (int t = 0; t < 4; ++t) s[i][t] -= delta;
      }
      float ps = 0.f;
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float e = __builtin_amdgcn_exp2f(s[i][t][r]);
          s[i][t][r] = e;
          if (!ONES) ps += e;
        }
      if (!ONES) l[i] += ps;
      pack_p(s[i], pb[i]);
    }
    ATT_T(tc);
    ATT_ACC(1, tb, tc);                   // wait for the scores + softmax VALU
#pragma unroll
    for (int u = 0; u < ND; ++u)
#pragma unroll
      for (int k2 = 0; k2 < 2; ++k2) {
        if constexpr (!PRE) vf[u][k2] = VROW ? tfrag_rows<VP>(Vs + vlane, u, k2) : tfrag(Vs, u, k2, l16, g);
#pragma unroll
        for (int i = 0; i < QT; ++i) o[i][u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf[u][k2], pb[i][k2], o[i][u], 0, 0, 0);
      }
    ATT_T(td);
    ATT_ACC(2, tc, td);                   // V^T fragment reads + PV MFMA issue
  };

  // Two LDS stages (+ two register sets when they fit): tile t computes from stage t&1 while tile t+1 sits in
  // registers on its way to the other stage and tile t+2 is in flight from L2/HBM, ONE barrier per tile.
  // Invariant at the top of the (unrolled-by-2) loop, t even: stage 0 = tile t, r0 = tile t+1, r1 = tile t+2.
  constexpr bool DEEP = KS < 5 && !(KS == 2 && ND == 3) && !(VAR & 2);      // d = 160: a second register set would not fit 2 waves / SIMD; d = 40: four waves / SIMD instead
  const KVSrc<KS, ND> src = kv_src<KS, ND, ONES, VROW>(Kb, p.ldk, Vb, p.ldvt, p.kv_stride, dh);
  KVRegs<KS, ND> r0;
  kv_load_buf<KS, ND, ONES, VROW>(r0, src, 0, p.ldk, p.kv_stride, p.ldvt);
  kv_store<KS, ND, VROW>(r0, Ks0, Vs0);
  if (nt > 1) kv_load_buf<KS, ND, ONES, VROW>(r0, src, 64, p.ldk, p.kv_stride, p.ldvt);
  if constexpr (DEEP) {
    KVRegs<KS, ND> r1;
    if (nt > 2) kv_load_buf<KS, ND, ONES, VROW>(r1, src, 128, p.ldk, p.kv_stride, p.ldvt);
    __syncthreads();
    for (int t0 = 0; t0 < nt; t0 += 2) {
      tile(Ks0, Vs0, t0 * 64);
      if (t0 + 1 < nt) kv_store<KS, ND, VROW>(r0, Ks1, Vs1);
      if (t0 + 3 < nt) kv_load_buf<KS, ND, ONES, VROW>(r0, src, (t0 + 3) * 64, p.ldk, p.kv_stride, p.ldvt);
      __syncthreads();
      if (t0 + 1 < nt) {
        tile(Ks1, Vs1, (t0 + 1) * 64);
        if (t0 + 2 < nt) kv_store<KS, ND, VROW>(r1, Ks0, Vs0);
        if (t0 + 4 < nt) kv_load_buf<KS, ND, ONES, VROW>(r1, src, (t0 + 4) * 64, p.ldk, p.kv_stride, p.ldvt);
        __syncthreads();
      }
    }
  } else {
    // one register set: r0 = tile t+1 while tile t computes (prefetch distance one tile)
    __syncthreads();
    ATT_T(tl0);
    for (int t0 = 0; t0 < nt; t0 += 2) {
      tile(Ks0, Vs0, t0 * 64);
      ATT_T(t1);
      if (t0 + 1 < nt) kv_store<KS, ND, VROW>(r0, Ks1, Vs1);
      ATT_T(t2);
      __syncthreads();
      ATT_T(t3);
      ATT_ACC(3, t1, t2);                 // staging the next tile (waits for its global loads)
      ATT_ACC(4, t2, t3);                 // barrier
      if (t0 + 1 < nt) {
        if (t0 + 2 < nt) kv_load_buf<KS, ND, ONES, VROW>(r0, src, (t0 + 2) * 64, p.ldk, p.kv_stride, p.ldvt);
        tile(Ks1, Vs1, (t0 + 1) * 64);
        ATT_T(t4);
        if (t0 + 2 < nt) kv_store<KS, ND, VROW>(r0, Ks0, Vs0);
        if (t0 + 3 < nt) kv_load_buf<KS, ND, ONES, VROW>(r0, src, (t0 + 3) * 64, p.ldk, p.kv_stride, p.ldvt);
        ATT_T(t5);
        __syncthreads();
        ATT_T(t6);
        ATT_ACC(3, t4, t5);
        ATT_ACC(4, t5, t6);
      }
    }
    ATT_T(tl1);
    ATT_ACC(5, tl0, tl1);                 // whole loop
#ifdef SKG_PHASES
    if (lane == 0 && blockIdx.x < (1 << 14)) {
      for (int j = 0; j < 6; ++j) g_attn_phase[blockIdx.x * 4 + wave][j] = att_acc[j];
      g_attn_phase[blockIdx.x * 4 + wave][6] = nt;
    }
#endif
  }
#pragma unroll
  for (int i = 0; i < QT; ++i) {
    float li;
    if (ONES) {      // denominator = row dh = 40 of O^T: tile 2, row 8 -> lanes g == 2, element 0
      li = __shfl(o[i][ND - 1][0], 32 + l16, 64);
    } else {
      li = l[i];
      li += __shfl_xor(li, 16, 64);
      li += __shfl_xor(li, 32, 64);
    }
    const float inv = 1.f / li;
    if (qok[i]) {
      half_t* orow = p.O + (size_t)(b * p.Nq + q[i]) * p.ldo + h * dh;
#pragma unroll
      for (int u = 0; u < ND; ++u) {
        const int d = 16 * u + 4 * g;
        if (d < dh) {
          half4_t v = {(half_t)(o[i][u][0] * inv), (half_t)(o[i][u][1] * inv), (half_t)(o[i][u][2] * inv),
                       (half_t)(o[i][u][3] * inv)};
          st_half4(orow + d, v);
        }
      }
      if (p.lse && g == 0) p.lse[((size_t)b * p.heads + h) * p.Nq + q[i]] = (log2f(li) - nm[i][0]) * LN2;
    }
  }
}

// ---- forward for SHORT key sequences (cross-attention over the 77 text tokens: modules/pipeline.py:96 -> diffusers
// CrossAttention with encoder_hidden_states) -------------------------------------------------------------------------------
// Round 2 ran these through the flash kernel above: two 64-key tiles of which the second holds 13 keys, a prologue / epilogue
// per 128 queries that never amortises, 45 us at 64x64 for 14 us of HBM time (128-142 TFLOP/s).
// With <= 80 keys there is nothing to stream and nothing "online": K [80][d] and V [96][d] of one (row, head) are staged in
// LDS ONCE per workgroup (25 KB at d = 40: four workgroups per CU), every wave then walks 16-query tiles: Q fragments
// straight from global memory (the next tile's loads in flight while this one computes), S^T = K Q^T in 5 x KS MFMAs, one
// plain softmax over the wave's 20 scores per lane (the maximum is exact: no running reference), O^T = V^T P^T with the
// probabilities as the B operand out of the accumulator registers, normalise, store.  What is left is one read of Q and one
// write of O: the kernel is HBM-bound.
//
// Long prompts (clip_text.encode_tokens: 75-token windows, 78 ... 231 keys; SKG_ATTN_RESIDENT_KV): K and V of one (row, head) still
// fit in LDS, so NT - the number of 16-key score tiles - is a template parameter: 5 (<= 80 keys, the kernel as it always was, the
// same instruction stream), 10 (<= 160) and 15 (<= 240).  The LDS image 2 (16 NT KP + 32 NSV VP) bytes bounds the workgroups per
// CU (163 840 bytes): NT = 10: d = 40 40 960 (4), d = 64 51 200 (3), d = 80 61 440 (2), d = 160 112 640 (1); NT = 15: 62 976 (2),
// 79 360 (2), 94 720 (1), d = 160 174 592 - does not fit, not built.  A lane holds 4 NT scores of one query, so the softmax stays
// in-lane plus two shuffles; any tile may be ragged or dead (Lp is a multiple of 8, not of 16: 231 keys -> 232 slots).
// Measured (profiles/attn_resident_kv.txt): unlike at 77 keys this does NOT beat the streaming kernel - every 16-query tile of a wave
// reads the whole K / V image from LDS (54 KB at d = 40, 231 keys) where attn_fwd_kernel shares each fragment between 2-3 query
// tiles, at 1-2 waves per SIMD instead of 3-4 - so unet.py does not ask for it; it stays built and tested behind the flag.
constexpr int short_min_blocks(int KS, int NT) { return NT > 5 ? (KS >= 5 || (KS >= 3 && NT > 10) ? 1 : 2) : (KS >= 5 ? 2 : (KS >= 3 ? 3 : 4)); }
template <int KS, int ND, int NT = 5>
__global__ __launch_bounds__(256, short_min_blocks(KS, NT)) void attn_fwd_short_kernel(const AttnParams p, int qchunk) {
  // NT 16-key score tiles: kv_stride <= 16 NT
  constexpr int NSV = (NT + 1) / 2;     // 32-key k-steps of the PV product (odd NT: the last half step is zero rows)
  constexpr int KP = KS * 32 + 16;
  constexpr int VP = vrow_pitch(ND);
  __shared__ __attribute__((aligned(16))) half_t Ks[16 * NT * KP];
  __shared__ __attribute__((aligned(16))) half_t Vs[32 * NSV * VP];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l16 = lane & 15, g = lane >> 4;
  const BlkMap bm = attn_block_map(p);
  const int b = bm.b, h = bm.h, dh = p.dh;
  const half_t* Kb = p.K + (size_t)b * p.kv_stride * p.ldk + h * dh;
  const half_t* Vb = p.Vt + (size_t)b * p.kv_stride * p.ldvt + h * dh;
  // ---- stage K [80][KP] and V [96][VP]: rows behind the last key and head-dim columns behind dh are zero
  for (int pi = threadIdx.x; pi < 16 * NT * (KS * 4); pi += 256) {
    const int row = pi / (KS * 4), pc = (pi - row * (KS * 4)) * 8;
    st_half8(Ks + row * KP + pc, (row < p.Nkv && pc < dh) ? ld_half8(Kb + (size_t)row * p.ldk + pc) : zero_half8());
  }
  for (int pi = threadIdx.x; pi < 32 * NSV * (2 * ND); pi += 256) {
    const int row = pi / (2 * ND), pc = (pi - row * (2 * ND)) * 8;
    st_half8(Vs + row * VP + pc, (row < p.Nkv && pc < dh) ? ld_half8(Vb + (size_t)row * p.ldvt + pc) : zero_half8());
  }
  __syncthreads();
  const int vlane = (4 * g + (l16 >> 2)) * VP + 4 * (l16 & 3);
  const float sc = p.scale * LOG2E;
  // keys this lane holds in score tile t, register r: 16 t + 4 g + r.  77 text tokens: only the last tile is ragged
  // (three registers of the g = 3 lanes); fewer than 65 keys (tests, other callers) take the general mask
  // NT > 5 (any key count up to 16 NT): tile rag = Nkv / 16 is the ragged one, the tiles behind it are dead as a whole - four
  // lane masks and wave-uniform tile tests (a mask per (tile, register) is 120 SGPRs at NT = 15: they spilled)
  const int rag = NT == 5 ? NT - 1 : p.Nkv >> 4;
  bool dead[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) dead[r] = 16 * rag + 4 * g + r >= p.Nkv;
  const bool short_rows = p.Nkv <= 16 * (NT - 1);        // wave-uniform
  const int klim = p.Nkv - 4 * g;
  const int q_begin = bm.bx * qchunk, q_end = min(p.Nq, q_begin + qchunk);
  const size_t rowbase = (size_t)b * p.Nq;
  auto load_q = [&](half8_t (&dst)[KS], int q0) {          // rows behind q_end read row q_end - 1 (not stored)
    const int q = min(q0 + l16, q_end - 1);
    const half_t* src = p.Q + (rowbase + q) * p.ldq + h * dh + 8 * g;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) dst[ks] = (32 * ks + 8 * g < dh) ? ld_half8(src + 32 * ks) : zero_half8();
  };
  half8_t qn[KS];
  int q0 = q_begin + wave * 16;
  if (q0 < q_end) load_q(qn, q0);
  for (; q0 < q_end; q0 += 64) {
    half8_t qf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int j = 0; j < 8; ++j) qf[ks][j] = (half_t)((float)qn[ks][j] * sc);
    if (q0 + 64 < q_end) load_q(qn, q0 + 64);               // in flight under this tile's work
    // (the accumulators start from an opaque zero REGISTER, the operands of an accumulator-starting MFMA stay live past
    // it, and the k-steps of one accumulator are separated by the other tiles' MFMAs - the treatment xattn.hip got after its
    // first build lost half an accumulator; tools/ubench/mfma_fresh_overlap.hip could not make the pattern fail in isolation,
    // profiles/r04_mfma_fresh_overlap.txt, so this is belt and braces)
    float4_t s[NT];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const half8_t kf = ld_half8(Ks + (16 * t + l16) * KP + 32 * ks + 8 * g);
        if (ks == 0) {
          float4_t z = {0.f, 0.f, 0.f, 0.f};
          asm volatile("" : "+v"(z));
          s[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf[ks], z, 0, 0, 0);
          asm volatile("" ::"v"(kf), "v"(qf[ks]));
        } else {
          s[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf[ks], s[t], 0, 0, 0);
        }
      }
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (NT == 5 && dead[r]) s[NT - 1][r] = NEG_BIG;
    if (NT == 5 && short_rows) {
#pragma unroll
      for (int t = 0; t < NT - 1; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (16 * t + r >= klim) s[t][r] = NEG_BIG;
    }
    if (NT > 5) {      // key 16 t + 4 g + r >= Nkv, every tile
      int ragl = rag;      // (opaque: the 2 NT tile tests are redone per query tile instead of living in SGPRs across the loop)
      asm volatile("" : "+s"(ragl));
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        if (t == ragl) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (dead[r]) s[t][r] = NEG_BIG;
        } else if (t > ragl) {
          s[t] = float4_t{NEG_BIG, NEG_BIG, NEG_BIG, NEG_BIG};
        }
      }
    }
    // the lane's maximum over its 4 NT scores: the first two by themselves, then two more per v_max3
    float mx = max3f(s[0][0], s[0][1], s[0][2]);
#pragma unroll
    for (int j = 3; j + 1 < 4 * NT; j += 2) mx = max3f(mx, s[j >> 2][j & 3], s[(j + 1) >> 2][(j + 1) & 3]);
    mx = max3f(mx, s[NT - 1][3], mx);
    mx = max3f(mx, __shfl_xor(mx, 16, 64), mx);
    mx = max3f(mx, __shfl_xor(mx, 32, 64), mx);
    float li = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = __builtin_amdgcn_exp2f(s[t][r] - mx);
        s[t][r] = e;
        li += e;
      }
    li += __shfl_xor(li, 16, 64);
    li += __shfl_xor(li, 32, 64);
    // B-operand fragments of P^T: element i of k-step sv <-> key 32 sv + 16 (i >> 2) + 4 g + (i & 3)
    half8_t pb[NSV];
#pragma unroll
    for (int sv = 0; sv < NSV; ++sv)
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int t = 2 * sv + (i >> 2);
        pb[sv][i] = t < NT ? (half_t)s[t][i & 3] : (half_t)0.f;
      }
    float4_t o[ND];
#pragma unroll
    for (int sv = 0; sv < NSV; ++sv)
#pragma unroll
      for (int u = 0; u < ND; ++u) {
        const half8_t vfr = tfrag_rows<VP>(Vs + vlane, u, sv);
        if (sv == 0) {
          float4_t z = {0.f, 0.f, 0.f, 0.f};
          asm volatile("" : "+v"(z));
          o[u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vfr, pb[sv], z, 0, 0, 0);
          asm volatile("" ::"v"(vfr), "v"(pb[sv]));
        } else {
          o[u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vfr, pb[sv], o[u], 0, 0, 0);
        }
      }
    const int q = q0 + l16;
    if (q < q_end) {
      const float inv = 1.f / li;
      half_t* orow = p.O + (rowbase + q) * p.ldo + h * dh;
#pragma unroll
      for (int u = 0; u < ND; ++u) {
        const int d = 16 * u + 4 * g;
        if (d < dh) {
          half4_t v = {(half_t)(o[u][0] * inv), (half_t)(o[u][1] * inv), (half_t)(o[u][2] * inv), (half_t)(o[u][3] * inv)};
          st_half4(orow + d, v);
        }
      }
      if (p.lse && g == 0) p.lse[((size_t)b * p.heads + h) * p.Nq + q] = (log2f(li) + mx) * LN2;
    }
  }
}

// dQ: per 64-query block, loop over key tiles.  dS^T = P^T o (dP^T - delta);  dQ^T += K^T dS^T.
template <int KS, int ND, int QT>
__global__ __launch_bounds__(256, 2) void attn_bwd_dq_kernel(const AttnParams p) {
  // QT query tiles of 16 per wave (64 * QT queries per workgroup): each K / V / K^T fragment read feeds QT MFMAs
  constexpr int KP = KS * 32 + 16;      // pitch = 16 or 48 (mod 64) halves: conflict-free for the 4 x 16-lane groups of ds_read_b128 (+ 8 is 2-way)
  __shared__ __attribute__((aligned(16))) half_t Ks[64 * KP];
  __shared__ __attribute__((aligned(16))) half_t Vr[64 * KP];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l16 = lane & 15, g = lane >> 4;
  const BlkMap bm = attn_block_map(p);
  const int b = bm.b, h = bm.h;
  const int dh = p.dh;
  int q[QT];
  bool qok[QT];
  half8_t qf[QT][KS], dof[QT][KS];
  float4_t nlse[QT], ndl[QT];
  float4_t dq[QT][ND];
#pragma unroll
  for (int i = 0; i < QT; ++i) {
    q[i] = bm.bx * (64 * QT) + (wave * QT + i) * 16 + l16;
    qok[i] = q[i] < p.Nq;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int c = 32 * ks + 8 * g;
      const bool ok = qok[i] && c < dh;
      qf[i][ks] = ok ? ld_half8(p.Q + (size_t)(b * p.Nq + q[i]) * p.ldq + h * dh + c) : zero_half8();
      dof[i][ks] = ok ? ld_half8(p.dO + (size_t)(b * p.Nq + q[i]) * p.lddo + h * dh + c) : zero_half8();
    }
    const size_t sidx = ((size_t)b * p.heads + h) * p.Nq + (qok[i] ? q[i] : 0);
    // minus lse (log2 domain) and minus delta ride in as the C operands of the S and dP MFMAs (see the forward)
    float dl;
    if (p.Of) {      // (launch-uniform) delta = sum_c O dO of this query from the dO fragments already in registers: the four lanes of a
                     // query hold 8 channels of every 32 each; the sum also goes to delta_out for the dK / dV launch
      float sm = 0.f;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const int c = 32 * ks + 8 * g;
        if (qok[i] && c < dh) {
          const half8_t of = ld_half8(p.Of + (size_t)(b * p.Nq + q[i]) * p.ldof + h * dh + c);
#pragma unroll
          for (int j = 0; j < 8; ++j) sm += (float)of[j] * (float)dof[i][ks][j];
        }
      }
      sm += __shfl_xor(sm, 16, 64);
      sm += __shfl_xor(sm, 32, 64);
      if (g == 0 && qok[i]) p.delta_out[sidx] = sm;
      dl = sm;
    } else {
      dl = qok[i] ? p.delta[sidx] : 0.f;
    }
    const float nl = qok[i] ? -p.lse[sidx] * LOG2E : NEG_BIG, nd = qok[i] ? -dl : 0.f;
    nlse[i] = float4_t{nl, nl, nl, nl};
    ndl[i] = float4_t{nd, nd, nd, nd};
#pragma unroll
    for (int u = 0; u < ND; ++u) dq[i][u] = float4_t{0.f, 0.f, 0.f, 0.f};
  }
  const float sc = p.scale * LOG2E;
#pragma unroll
  for (int i = 0; i < QT; ++i)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int j = 0; j < 8; ++j) qf[i][ks][j] = (half_t)((float)qf[i][ks][j] * sc);   // same rounding as the forward

  const half_t* Kb = p.K + (size_t)b * p.kv_stride * p.ldk + h * dh;
  const half_t* Vb = p.V + (size_t)b * p.kv_stride * p.ldv + h * dh;
  const int nt = (p.Nkv + 63) / 64;
  // register prefetch: the two tiles of key block t+1 are loaded while block t computes.  K^T fragments (the A operand
  // of dQ^T += K^T dS^T) come out of the SAME row-major K tile through the LDS transpose read (tfrag_rows).
  RowRegs<KS> rk, rv;
  const RowSrc<KS> sk = row_src<KS>(Kb, p.ldk, p.kv_stride, dh), sv = row_src<KS>(Vb, p.ldv, p.kv_stride, dh);
  const int tlane = (4 * g + (l16 >> 2)) * KP + 4 * (l16 & 3);
  rows_load_buf<KS>(rk, sk, p.ldk, 0);
  rows_load_buf<KS>(rv, sv, p.ldv, 0);
  for (int t0 = 0; t0 < nt; ++t0) {
    const int kv0 = t0 * 64;
    __syncthreads();                     // everyone is done reading the previous block
    rows_store<KS>(rk, Ks);
    rows_store<KS>(rv, Vr);
    __syncthreads();
    if (t0 + 1 < nt) {
      rows_load_buf<KS>(rk, sk, p.ldk, kv0 + 64);
      rows_load_buf<KS>(rv, sv, p.ldv, kv0 + 64);
    }
    float4_t s[QT][4], dp[QT][4];      // s = S*sc - lse,  dp = dP - delta  straight out of the matrix pipe
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const int off = (16 * t + l16) * KP + 32 * ks + 8 * g;
        const half8_t kfr = ld_half8(Ks + off), vfr = ld_half8(Vr + off);
#pragma unroll
        for (int i = 0; i < QT; ++i) {
          s[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kfr, qf[i][ks], ks == 0 ? nlse[i] : s[i][t], 0, 0, 0);
          dp[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vfr, dof[i][ks], ks == 0 ? ndl[i] : dp[i][t], 0, 0, 0);
        }
      }
    }
    half8_t sb[QT][2];
#pragma unroll
    for (int i = 0; i < QT; ++i) {
      if (kv0 + 64 > p.Nkv) {          // ragged last block only (wave-uniform)
        const int lim = p.Nkv - kv0 - 4 * g;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (16 * t + r >= lim) s[i][t][r] = NEG_BIG;
      }
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) s[i][t][r] = __builtin_amdgcn_exp2f(s[i][t][r]) * dp[i][t][r];
      pack_p(s[i], sb[i]);
    }
#pragma unroll
    for (int u = 0; u < ND; ++u)
#pragma unroll
      for (int k2 = 0; k2 < 2; ++k2) {
        const half8_t ktf = tfrag_rows<KP>(Ks + tlane, u, k2);
#pragma unroll
        for (int i = 0; i < QT; ++i) dq[i][u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ktf, sb[i][k2], dq[i][u], 0, 0, 0);
      }
  }
#pragma unroll
  for (int i = 0; i < QT; ++i) {
    if (!qok[i]) continue;
    half_t* orow = p.O + (size_t)(b * p.Nq + q[i]) * p.ldo + h * dh;
#pragma unroll
    for (int u = 0; u < ND; ++u) {
      const int d = 16 * u + 4 * g;
      if (d < dh) {
        half4_t v = {(half_t)(dq[i][u][0] * p.scale), (half_t)(dq[i][u][1] * p.scale), (half_t)(dq[i][u][2] * p.scale),
                     (half_t)(dq[i][u][3] * p.scale)};
        st_half4(orow + d, v);
      }
    }
  }
}

// dK/dV: per 64-key block (lane column = key), loop over query tiles.
//   S = Q K^T (rows q), P = exp(S*scale - lse[q]), dP = dO V^T, dS = P o (dP - delta[q])
//   dV^T += dO^T P,   dK^T += Q^T dS      (A operands = transposed tiles, B = registers)
template <int KS, int ND, int KT>
__global__ __launch_bounds__(256, (KS >= 5 ? 1 : 2)) void attn_bwd_dkv_kernel(const AttnParams p) {
  // KT key tiles of 16 per wave: a workgroup owns 64 * KT keys, so every Q / dO / Q^T / dO^T fragment read from LDS
  // (and every byte of those panels streamed from L2) feeds KT MFMAs instead of one (same idea as QT in the forward).
  constexpr int KP = KS * 32 + 16;      // pitch = 16 or 48 (mod 64) halves: conflict-free for the 4 x 16-lane groups of ds_read_b128 (+ 8 is 2-way)
  __shared__ __attribute__((aligned(16))) half_t Qs[64 * KP];
  __shared__ __attribute__((aligned(16))) half_t Ds[64 * KP];
  __shared__ __attribute__((aligned(16))) float lse_s[64], del_s[64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l16 = lane & 15, g = lane >> 4;
  const BlkMap bm = attn_block_map(p);
  const int b = bm.b, h = bm.h;
  const int dh = p.dh;
  int kv[KT];
  bool kok[KT];
  half8_t kf[KT][KS], vf[KT][KS];
#pragma unroll
  for (int i = 0; i < KT; ++i) {
    kv[i] = bm.bx * (64 * KT) + (wave * KT + i) * 16 + l16;
    kok[i] = kv[i] < p.Nkv;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int c = 32 * ks + 8 * g;
      const bool ok = kok[i] && c < dh;
      kf[i][ks] = ok ? ld_half8(p.K + (size_t)(b * p.kv_stride + kv[i]) * p.ldk + h * dh + c) : zero_half8();
      vf[i][ks] = ok ? ld_half8(p.V + (size_t)(b * p.kv_stride + kv[i]) * p.ldv + h * dh + c) : zero_half8();
    }
  }
  const float sc = p.scale * LOG2E;
#pragma unroll
  for (int i = 0; i < KT; ++i)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int j = 0; j < 8; ++j) kf[i][ks][j] = (half_t)((float)kf[i][ks][j] * sc);   // S*sc out of the matrix pipe
  float4_t dk[KT][ND], dv[KT][ND];
#pragma unroll
  for (int i = 0; i < KT; ++i)
#pragma unroll
    for (int u = 0; u < ND; ++u) {
      dk[i][u] = float4_t{0.f, 0.f, 0.f, 0.f};
      dv[i][u] = float4_t{0.f, 0.f, 0.f, 0.f};
    }
  const half_t* Qb = p.Q + (size_t)b * p.Nq * p.ldq + h * dh;
  const half_t* Db = p.dO + (size_t)b * p.Nq * p.lddo + h * dh;
  const size_t sbase = ((size_t)b * p.heads + h) * p.Nq;
  const int nt = (p.Nq + 63) / 64;
  // register prefetch of query block t+1 (Q, dO row tiles, lse, delta) under block t's math; the Q^T / dO^T fragments
  // of dK^T += Q^T dS, dV^T += dO^T P are read from the same row tiles through the LDS transpose read
  RowRegs<KS> rq, rd;
  float r_lse = 0.f, r_del = 0.f;
  const RowSrc<KS> sq = row_src<KS>(Qb, p.ldq, p.Nq, dh), sd = row_src<KS>(Db, p.lddo, p.Nq, dh);
  const int tlane = (4 * g + (l16 >> 2)) * KP + 4 * (l16 & 3);
  auto prefetch = [&](int q0) {
    rows_load_buf<KS>(rq, sq, p.ldq, q0);
    rows_load_buf<KS>(rd, sd, p.lddo, q0);
    if (threadIdx.x < 64) {
      const int qq = q0 + threadIdx.x;
      r_lse = qq < p.Nq ? -p.lse[sbase + qq] * LOG2E : NEG_BIG;      // stored NEGATED: they are MFMA C operands
      r_del = qq < p.Nq ? -p.delta[sbase + qq] : 0.f;
    }
  };
  prefetch(0);
  for (int t0 = 0; t0 < nt; ++t0) {
    const int q0 = t0 * 64;
    __syncthreads();
    rows_store<KS>(rq, Qs);
    rows_store<KS>(rd, Ds);
    if (threadIdx.x < 64) { lse_s[threadIdx.x] = r_lse; del_s[threadIdx.x] = r_del; }
    __syncthreads();
    if (t0 + 1 < nt) prefetch(q0 + 64);
    float4_t s[KT][4], dp[KT][4];      // s = S*sc - lse[q],  dp = dP - delta[q]  (rows 16t + 4g + r are queries)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const float4_t nl = *reinterpret_cast<const float4_t*>(lse_s + 16 * t + 4 * g);
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const int off = (16 * t + l16) * KP + 32 * ks + 8 * g;
        const half8_t qfr = ld_half8(Qs + off), dfr = ld_half8(Ds + off);
#pragma unroll
        for (int i = 0; i < KT; ++i) {
          s[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(qfr, kf[i][ks], ks == 0 ? nl : s[i][t], 0, 0, 0);
          dp[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(dfr, vf[i][ks], ks == 0 ? float4_t{0.f, 0.f, 0.f, 0.f} : dp[i][t], 0, 0, 0);
        }
      }
    }
    half8_t pb[KT][2], sb[KT][2];
#pragma unroll
    for (int i = 0; i < KT; ++i) {
      float4_t ds[4];
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float pr = __builtin_amdgcn_exp2f(s[i][t][r]);
          s[i][t][r] = pr;
          ds[t][r] = pr * (dp[i][t][r] + del_s[16 * t + 4 * g + r]);
        }
      pack_p(s[i], pb[i]);
      pack_p(ds, sb[i]);
    }
#pragma unroll
    for (int u = 0; u < ND; ++u)
#pragma unroll
      for (int k2 = 0; k2 < 2; ++k2) {
        const half8_t dtf = tfrag_rows<KP>(Ds + tlane, u, k2), qtf = tfrag_rows<KP>(Qs + tlane, u, k2);
#pragma unroll
        for (int i = 0; i < KT; ++i) {
          dv[i][u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(dtf, pb[i][k2], dv[i][u], 0, 0, 0);
          dk[i][u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(qtf, sb[i][k2], dk[i][u], 0, 0, 0);
        }
      }
  }
#pragma unroll
  for (int i = 0; i < KT; ++i) {
    if (!kok[i]) continue;
    half_t* krow = p.O + (size_t)(b * p.kv_stride + kv[i]) * p.ldo + h * dh;
    half_t* vrow = p.O2 + (size_t)(b * p.kv_stride + kv[i]) * p.ldo2 + h * dh;
#pragma unroll
    for (int u = 0; u < ND; ++u) {
      const int d = 16 * u + 4 * g;
      if (d < dh) {
        half4_t a = {(half_t)(dk[i][u][0] * p.scale), (half_t)(dk[i][u][1] * p.scale),
                     (half_t)(dk[i][u][2] * p.scale), (half_t)(dk[i][u][3] * p.scale)};
        half4_t c = {(half_t)dv[i][u][0], (half_t)dv[i][u][1], (half_t)dv[i][u][2], (half_t)dv[i][u][3]};
        st_half4(krow + d, a);
        st_half4(vrow + d, c);
      }
    }
  }
}

// delta[b][h][q] = sum_d dO[q][h*dh+d] * O[q][h*dh+d]; one 16-lane group per (row, head)
__global__ __launch_bounds__(256) void attn_delta_kernel(const half_t* __restrict__ O, int ldo,
                                                         const half_t* __restrict__ dO, int lddo,
                                                         float* __restrict__ delta, int batch, int heads, int Nq,
                                                         int dh) {
  const size_t total = (size_t)batch * Nq * heads;
  const size_t item = ((size_t)blockIdx.x * 256 + threadIdx.x) >> 4;
  const int sub = threadIdx.x & 15;
  float s = 0.f;
  if (item < total) {
    const int h = (int)(item % heads);
    const size_t row = item / heads;   // b*Nq + q
    for (int c = sub * 8; c < dh; c += 128) {
      const half8_t a = ld_half8(O + row * ldo + h * dh + c);
      const half8_t d = ld_half8(dO + row * lddo + h * dh + c);
#pragma unroll
      for (int j = 0; j < 8; ++j) s += (float)a[j] * (float)d[j];
    }
  }
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (item < total && sub == 0) {
    const int h = (int)(item % heads);
    const size_t row = item / heads;
    const size_t b = row / Nq, q = row - b * Nq;
    delta[(b * heads + h) * Nq + q] = s;
  }
}

// d = 40 / d = 64 forward: how many 16-query tiles a wave carries (QT) against how many waves a SIMD holds.
// Every K / V fragment a wave reads from LDS feeds QT MFMAs, and at QT = 2 the 16 resident waves of a CU move 56 KB through the
// LDS per 448 MFMA cycles - half the LDS pipe's time, which the probes of round 4 priced at 135 of 632 us at d = 40.  More tiles
// per wave trade that traffic for occupancy (the register budget): measured on one box (profiles/r04_attn_qt_variants.txt)
//   d = 40:  QT 2, 4 waves / SIMD 529 us;  QT 3, 3 waves / SIMD (165 VGPRs) 514-520 us;  QT 4, 2 waves / SIMD 554-562 us
//   d = 64:  QT 2, 3 waves / SIMD 1053 us at 9 480 tokens;  QT 4, 2 waves / SIMD (256 VGPRs) 1001-1006 us there, but
//            218 against 209 us at 2 568 tokens and 71 against 57 us at 840 (too few workgroups of 256 queries)
// End to end (same box, alternating): config 2 + 0.3 % / + 0.1 % with QT 3 at d = 40; config 5 - 0.4 % / + 0.0 % with QT 4 at d = 64.
// So QT 3 runs d = 40 where the launch has >= 1024 workgroups of 192 queries, d = 64 stays at QT 2 with ONE register prefetch
// set (152 VGPRs = three waves per SIMD instead of two: + 8...15 %).  SKG_ATTN_VAR: 12 = QT 2 everywhere (round 3's
// dispatch), 9 / 8 = QT 3 at d = 40 / QT 4 at d = 64 whatever the size, 7 = the two-set form at d = 64 (tools/attn_var_bench.py).
inline int attn_var() {
  static const int v = getenv("SKG_ATTN_VAR") ? atoi(getenv("SKG_ATTN_VAR")) : 0;
  return v;
}
inline bool attn_no_short() {
  static const bool v = getenv("SKG_NO_ATTN_SHORT") != nullptr;        // A/B switch
  return v;
}

// The streaming kernel of a plan (below) with QT query tiles per wave: two (128 queries per workgroup) except at d = 160
// (register budget), three / four at d = 40 / 64 where the plan says so
template <bool VROW>
static int attn_fwd_launch_stream(const AttnParams& p, int QT, bool two_sets, dim3 grid, hipStream_t st) {
  switch (p.dh) {
    case 16: hipLaunchKernelGGL((attn_fwd_kernel<1, 1, 2, false, 0, VROW>), grid, dim3(256), 0, st, p); break;
    case 32: hipLaunchKernelGGL((attn_fwd_kernel<1, 2, 2, false, 0, VROW>), grid, dim3(256), 0, st, p); break;
    case 40:
      if (QT == 3) hipLaunchKernelGGL((attn_fwd_kernel<2, 3, 3, false, 2 | (3 << 2), VROW>), grid, dim3(256), 0, st, p);
      else hipLaunchKernelGGL((attn_fwd_kernel<2, 3, 2, false, 0, VROW>), grid, dim3(256), 0, st, p);
      break;
    case 64:
      if constexpr (VROW) {      // (the transposed-V form of this instantiation spills 5 registers: row-major V only)
        if (QT == 4) {
          hipLaunchKernelGGL((attn_fwd_kernel<2, 4, 4, false, 2 | (2 << 2), VROW>), grid, dim3(256), 0, st, p);
          break;
        }
      }
      if (two_sets) hipLaunchKernelGGL((attn_fwd_kernel<2, 4, 2, false, 0, VROW>), grid, dim3(256), 0, st, p);
      else hipLaunchKernelGGL((attn_fwd_kernel<2, 4, 2, false, 2 | (3 << 2), VROW>), grid, dim3(256), 0, st, p);
      break;
    case 80: hipLaunchKernelGGL((attn_fwd_kernel<3, 5, 2, false, 0, VROW>), grid, dim3(256), 0, st, p); break;
    case 160: hipLaunchKernelGGL((attn_fwd_kernel<5, 10, 1, false, 0, VROW>), grid, dim3(256), 0, st, p); break;
    default: return SKG_E_UNSUPPORTED;
  }
  return SKG_OK;
}

// kv8: kv_stride % 8 == 0 - only the transposed V^T operand needs it (16-byte loads along the key axis start at b * kv_stride).
// Row-major K / V rows are addressed row by row (buffer descriptors sized to this batch row's keys, or explicit key < Nkv
// tests), so the forms that read V row-major take any kv_stride: the self-attention of a non-square map has HW keys per
// image, e.g. 5 x 9 = 45 at the deepest level of 320 x 576 px.
inline bool common_ok(int batch, int heads, int Nq, int Nkv, int kv_stride, int dh, bool kv8 = true) {
  return batch > 0 && heads > 0 && Nq > 0 && Nkv > 0 && kv_stride >= Nkv && (!kv8 || kv_stride % 8 == 0) && dh % 8 == 0;
}

// THE dispatch rule of skg_attn_fwd: which instantiation a call runs and how many queries one workgroup of it covers.  The
// launcher switches on the plan and skg_attn_fwd_variant reports it, so the two cannot disagree.
//   code  1000 + QT  attn_fwd_kernel with QT query tiles per wave       2000 + QT  its causal instantiation
//         3000 + NT  attn_fwd_short_kernel with NT 16-key score tiles
//         negative   SKG_E_*: what skg_attn_fwd returns for these arguments once its pointers and pitches pass
//   qpw   queries per workgroup: 64 QT, or the short-key kernel's query chunk
//   two_sets  d = 64, QT 2: two register prefetch sets (SKG_ATTN_VAR = 7) instead of the shipped one
struct AttnFwdPlan { int code, qpw; bool two_sets; };
AttnFwdPlan attn_fwd_plan(int batch, int heads, int Nq, int Nkv, int kv_stride, int dh, unsigned flags) {
  const bool causal = flags & SKG_ATTN_CAUSAL, vrow = flags & SKG_ATTN_ROWV, resident = flags & SKG_ATTN_RESIDENT_KV;
  if ((flags & ~(SKG_ATTN_CAUSAL | SKG_ATTN_ROWV | SKG_ATTN_RESIDENT_KV)) || (causal && vrow) || (resident && !vrow) ||
      !common_ok(batch, heads, Nq, Nkv, kv_stride, dh, !vrow))
    return {SKG_E_BADARG, 0, false};
  const long pairs = (long)heads * batch;
  const bool short_dh = dh == 40 || dh == 64 || dh == 80 || dh == 160;
  // queries per workgroup of the short-key kernel: ~1024+ workgroups where the launch has them, a multiple of 64
  long qch = (pairs * Nq / 1024 + 63) / 64 * 64;
  qch = qch > 512 ? 512 : qch;
  // short key sequences (the 77 text tokens of every cross-attention): the LDS-resident kernel, HBM-bound; at least 64 queries
  if (vrow && !causal && kv_stride <= 80 && !attn_no_short() && short_dh) return {3005, (int)(qch < 64 ? 64 : qch), false};
  // SKG_ATTN_RESIDENT_KV (a hint: cross-attention over a long prompt's 81 ... 240 keys): the same kernel with 10 / 15 score tiles
  // where K and V of one (row, head) fit the 160 KB of LDS - not d = 160 above 160 keys; everything else runs as without the flag.
  // One staging pass of up to 240 K / V rows per workgroup: at least 128 queries behind it where the launch has them
  const int rtiles = kv_stride <= 160 ? 10 : 15;
  if (resident && kv_stride > 80 && kv_stride <= 240 && !attn_no_short() && short_dh && (dh != 160 || rtiles == 10))
    return {3000 + rtiles, (int)(qch < 128 ? 128 : qch), false};
  if (causal) {
    if (dh == 160) return {SKG_E_BADARG, 0, false};
    if (dh != 16 && dh != 32 && dh != 64) return {SKG_E_UNSUPPORTED, 0, false};
    return {2002, 128, false};
  }
  const int var = attn_var();
  switch (dh) {
    case 16: case 32: case 80: return {1002, 128, false};
    case 160: return {1001, 64, false};
    case 40:      // QT 3 where the launch has >= 1024 workgroups of 192 queries (the measurements above attn_var)
      if (var == 9 || (var == 0 && skg_cdiv(Nq, 192) * pairs >= 1024)) return {1003, 192, false};
      return {1002, 128, false};
    case 64:      // QT 4: opt-in, row-major V (+ 5 % on the kernel alone at 9 480 tokens, nothing end to end on config 5)
      if (vrow && var == 8) return {1004, 256, false};
      return {1002, 128, var == 7};
    default: return {SKG_E_UNSUPPORTED, 0, false};
  }
}

}  // namespace

extern "C" int skg_attn_fwd_variant(int batch, int heads, int Nq, int Nkv, int kv_stride, int dh, unsigned flags,
                                    int* queries_per_workgroup) {
  const AttnFwdPlan plan = attn_fwd_plan(batch, heads, Nq, Nkv, kv_stride, dh, flags);
  if (plan.code >= 0 && queries_per_workgroup) *queries_per_workgroup = plan.qpw;
  return plan.code;
}

// SKG_ATTN_ROWV: V handed over ROW-MAJOR ([batch * kv_stride][ldvt], e.g. the third column block of a fused QKV projection) - the
// kernel reads its fragments through the LDS transpose read, no V^T copy is needed; SKG_ATTN_CAUSAL: key j <= query i only
extern "C" int skg_attn_fwd(const void* Q, int ldq, const void* K, int ldk, const void* Vt, int ldvt, void* O,
                            int ldo, float* lse, int batch, int heads, int Nq, int Nkv, int kv_stride, int dh,
                            float scale, unsigned flags, void* stream) {
  // (the plan refuses what the flags and the shape rule out - the same SKG_E_BADARG the pointer and pitch checks give)
  SKG_REQUIRE(Q && K && Vt && O);
  SKG_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldvt % 8 == 0 && ldo % 4 == 0);
  SKG_REQUIRE(skg_aligned(Q, 16) && skg_aligned(K, 16) && skg_aligned(Vt, 16) && skg_aligned(O, 8));
  const AttnFwdPlan plan = attn_fwd_plan(batch, heads, Nq, Nkv, kv_stride, dh, flags);
  if (plan.code < 0) return plan.code;
  AttnParams p{};
  p.Q = (const half_t*)Q; p.ldq = ldq; p.K = (const half_t*)K; p.ldk = ldk; p.Vt = (const half_t*)Vt; p.ldvt = ldvt;
  p.O = (half_t*)O; p.ldo = ldo; p.lse = lse;
  p.batch = batch; p.heads = heads; p.Nq = Nq; p.Nkv = Nkv; p.kv_stride = kv_stride; p.dh = dh; p.scale = scale;
  hipStream_t st = (hipStream_t)stream;
  p.nx = skg_cdiv(Nq, plan.qpw);
  const dim3 grid((unsigned)p.nx * heads * batch);
  const int qch = plan.qpw;
  switch (plan.code) {
    case 3005:
      switch (dh) {
        case 40: hipLaunchKernelGGL((attn_fwd_short_kernel<2, 3>), grid, dim3(256), 0, st, p, qch); break;
        case 64: hipLaunchKernelGGL((attn_fwd_short_kernel<2, 4>), grid, dim3(256), 0, st, p, qch); break;
        case 80: hipLaunchKernelGGL((attn_fwd_short_kernel<3, 5>), grid, dim3(256), 0, st, p, qch); break;
        default: hipLaunchKernelGGL((attn_fwd_short_kernel<5, 10>), grid, dim3(256), 0, st, p, qch); break;
      }
      SKG_CHECK_LAUNCH("skg_attn_fwd (short keys)");
      return SKG_OK;
    case 3010:
      switch (dh) {
        case 40: hipLaunchKernelGGL((attn_fwd_short_kernel<2, 3, 10>), grid, dim3(256), 0, st, p, qch); break;
        case 64: hipLaunchKernelGGL((attn_fwd_short_kernel<2, 4, 10>), grid, dim3(256), 0, st, p, qch); break;
        case 80: hipLaunchKernelGGL((attn_fwd_short_kernel<3, 5, 10>), grid, dim3(256), 0, st, p, qch); break;
        default: hipLaunchKernelGGL((attn_fwd_short_kernel<5, 10, 10>), grid, dim3(256), 0, st, p, qch); break;
      }
      SKG_CHECK_LAUNCH("skg_attn_fwd (resident keys)");
      return SKG_OK;
    case 3015:
      switch (dh) {
        case 40: hipLaunchKernelGGL((attn_fwd_short_kernel<2, 3, 15>), grid, dim3(256), 0, st, p, qch); break;
        case 64: hipLaunchKernelGGL((attn_fwd_short_kernel<2, 4, 15>), grid, dim3(256), 0, st, p, qch); break;
        default: hipLaunchKernelGGL((attn_fwd_short_kernel<3, 5, 15>), grid, dim3(256), 0, st, p, qch); break;
      }
      SKG_CHECK_LAUNCH("skg_attn_fwd (resident keys)");
      return SKG_OK;
    case 2002:
      switch (dh) {
        case 16: hipLaunchKernelGGL((attn_fwd_kernel<1, 1, 2, true>), grid, dim3(256), 0, st, p); break;
        case 32: hipLaunchKernelGGL((attn_fwd_kernel<1, 2, 2, true>), grid, dim3(256), 0, st, p); break;
        default: hipLaunchKernelGGL((attn_fwd_kernel<2, 4, 2, true>), grid, dim3(256), 0, st, p); break;
      }
      break;
    default: {      // 1000 + QT
      const int rc = (flags & SKG_ATTN_ROWV) ? attn_fwd_launch_stream<true>(p, plan.code - 1000, plan.two_sets, grid, st)
                                             : attn_fwd_launch_stream<false>(p, plan.code - 1000, plan.two_sets, grid, st);
      if (rc != SKG_OK) return rc;
    }
  }
  SKG_CHECK_LAUNCH("skg_attn_fwd");
  return SKG_OK;
}

extern "C" int skg_attn_bwd_delta(const void* O, int ldo, const void* dO, int lddo, float* delta, int batch,
                                  int heads, int Nq, int dh, void* stream) {
  SKG_REQUIRE(O && dO && delta && batch > 0 && heads > 0 && Nq > 0 && dh % 8 == 0 && ldo % 8 == 0 && lddo % 8 == 0);
  SKG_REQUIRE(skg_aligned(O, 16) && skg_aligned(dO, 16));
  const size_t total = (size_t)batch * Nq * heads;
  hipLaunchKernelGGL(attn_delta_kernel, dim3((unsigned)((total * 16 + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, (const half_t*)O, ldo, (const half_t*)dO, lddo, delta, batch, heads, Nq, dh);
  SKG_CHECK_LAUNCH("skg_attn_bwd_delta");
  return SKG_OK;
}

// delta == NULL: skg_attn_bwd_delta in the prologue (round 5) - delta[b][h][q] = sum_d dO O is formed from the dO fragments the launch
// loads anyway and O, used, and stored to delta_out for the dK / dV launch that follows: one launch and one read of dO fewer per
// attention.  With delta given, O / ldo / delta_out are not looked at.
extern "C" int skg_attn_bwd_dq(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, const void* dO, int lddo,
                               const void* O, int ldo, const float* lse, const float* delta, float* delta_out, void* dQ, int lddq,
                               int batch, int heads, int Nq, int Nkv, int kv_stride, int dh, float scale, void* stream) {
  if (delta) { O = nullptr; ldo = 0; delta_out = nullptr; }
  SKG_REQUIRE(Q && K && V && dO && lse && (delta || (O && delta_out)) && dQ && common_ok(batch, heads, Nq, Nkv, kv_stride, dh, false));
  SKG_REQUIRE(!O || (ldo % 8 == 0 && skg_aligned(O, 16)));
  SKG_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && lddo % 8 == 0 && lddq % 4 == 0);
  SKG_REQUIRE(skg_aligned(Q, 16) && skg_aligned(K, 16) && skg_aligned(V, 16) && skg_aligned(dO, 16) && skg_aligned(dQ, 8));
  AttnParams p{};
  p.Q = (const half_t*)Q; p.ldq = ldq; p.K = (const half_t*)K; p.ldk = ldk; p.V = (const half_t*)V; p.ldv = ldv;
  p.dO = (const half_t*)dO; p.lddo = lddo;
  p.lse = const_cast<float*>(lse); p.delta = delta; p.O = (half_t*)dQ; p.ldo = lddq;
  p.Of = (const half_t*)O; p.ldof = ldo; p.delta_out = delta_out;
  p.batch = batch; p.heads = heads; p.Nq = Nq; p.Nkv = Nkv; p.kv_stride = kv_stride; p.dh = dh; p.scale = scale;
  hipStream_t st = (hipStream_t)stream;
  p.nx = skg_cdiv(Nq, dh <= 40 ? 128 : 64);         // query tiles per wave: 2 up to d = 40, 1 beyond
  dim3 grid((unsigned)p.nx * heads * batch);
  switch (dh) {
    case 16: hipLaunchKernelGGL((attn_bwd_dq_kernel<1, 1, 2>), grid, dim3(256), 0, st, p); break;
    case 32: hipLaunchKernelGGL((attn_bwd_dq_kernel<1, 2, 2>), grid, dim3(256), 0, st, p); break;
    case 40: hipLaunchKernelGGL((attn_bwd_dq_kernel<2, 3, 2>), grid, dim3(256), 0, st, p); break;
    case 64: hipLaunchKernelGGL((attn_bwd_dq_kernel<2, 4, 1>), grid, dim3(256), 0, st, p); break;
    case 80: hipLaunchKernelGGL((attn_bwd_dq_kernel<3, 5, 1>), grid, dim3(256), 0, st, p); break;
    case 160: hipLaunchKernelGGL((attn_bwd_dq_kernel<5, 10, 1>), grid, dim3(256), 0, st, p); break;
    default: return SKG_E_UNSUPPORTED;
  }
  SKG_CHECK_LAUNCH("skg_attn_bwd_dq");
  return SKG_OK;
}

// K, V, dK, dV rows of batch row b start at b * kv_stride (>= Nkv: a padded K / V buffer; dense: kv_stride = Nkv); rows
// Nkv .. kv_stride - 1 of dK / dV are not written
extern "C" int skg_attn_bwd_dkv(const void* Q, int ldq, const void* K, int ldk,
                                const void* V, int ldv, const void* dO, int lddo,
                                const float* lse, const float* delta, void* dK, int lddk, void* dV, int lddv,
                                int batch, int heads, int Nq, int Nkv, int kv_stride, int dh, float scale, void* stream) {
  SKG_REQUIRE(Q && K && V && dO && lse && delta && dK && dV && common_ok(batch, heads, Nq, Nkv, kv_stride, dh, false));
  SKG_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && lddo % 8 == 0 && lddk % 4 == 0 && lddv % 4 == 0);
  SKG_REQUIRE(skg_aligned(Q, 16) && skg_aligned(K, 16) && skg_aligned(V, 16) &&
              skg_aligned(dO, 16) && skg_aligned(dK, 8) && skg_aligned(dV, 8));
  AttnParams p{};
  p.Q = (const half_t*)Q; p.ldq = ldq; p.K = (const half_t*)K; p.ldk = ldk;
  p.V = (const half_t*)V; p.ldv = ldv; p.dO = (const half_t*)dO; p.lddo = lddo;
  p.lse = const_cast<float*>(lse); p.delta = delta; p.O = (half_t*)dK; p.ldo = lddk;
  p.O2 = (half_t*)dV; p.ldo2 = lddv;
  p.batch = batch; p.heads = heads; p.Nq = Nq; p.Nkv = Nkv; p.kv_stride = kv_stride; p.dh = dh; p.scale = scale;
  hipStream_t st = (hipStream_t)stream;
  p.nx = skg_cdiv(Nkv, dh <= 40 ? 128 : 64);        // key tiles per wave: 2 up to d = 40, 1 beyond (register budget)
  dim3 grid((unsigned)p.nx * heads * batch);
  switch (dh) {
    case 16: hipLaunchKernelGGL((attn_bwd_dkv_kernel<1, 1, 2>), grid, dim3(256), 0, st, p); break;
    case 32: hipLaunchKernelGGL((attn_bwd_dkv_kernel<1, 2, 2>), grid, dim3(256), 0, st, p); break;
    case 40: hipLaunchKernelGGL((attn_bwd_dkv_kernel<2, 3, 2>), grid, dim3(256), 0, st, p); break;
    case 64: hipLaunchKernelGGL((attn_bwd_dkv_kernel<2, 4, 1>), grid, dim3(256), 0, st, p); break;
    case 80: hipLaunchKernelGGL((attn_bwd_dkv_kernel<3, 5, 1>), grid, dim3(256), 0, st, p); break;
    case 160: hipLaunchKernelGGL((attn_bwd_dkv_kernel<5, 10, 1>), grid, dim3(256), 0, st, p); break;
    default: return SKG_E_UNSUPPORTED;
  }
  SKG_CHECK_LAUNCH("skg_attn_bwd_dkv");
  return SKG_OK;
}

#ifdef SKG_PHASES
extern "C" int skg_debug_attn_phases(void* host_out, int nwaves) {      // not part of the ABI: profiling builds only
  return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_attn_phase), (size_t)nwaves * 8 * sizeof(unsigned long long));
}
#endif
