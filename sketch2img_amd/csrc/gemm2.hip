// v2 fp16 MFMA GEMM / 3x3 implicit-GEMM convolution for gfx950: LDS-DMA staged, swizzled, double buffered.
//
//   C[m][n] = epi(alpha * (sum_k A[m][k] * B[n][k] + bias[n]) + residual[m][n])
// (SKG_EPI_BIAS_ROWS, convolutions: bias[m / (OH * OW)][n].  A tile that lies inside one sample - OH * OW % BM == 0, the 64x64 to
// 16x16 levels - offsets the bias pointer once per workgroup, a scalar, in front of the slice load; a launch whose tiles can span
// samples runs the BROWS instantiations, whose epilogue looks the bias row up per output row)
//
// Block tile 128 x BN x 64 (BN = 160 | 128 | 64), 4 waves as 2(M) x 2(N), wave tile 64 x BN/2 out of
// 16x16x32 f16 MFMAs (weights as the A operand so each lane owns 4 consecutive output channels).
//
// HBM/L2 -> LDS goes through `buffer_load_dwordx4 ... lds` (LDS-DMA, 16 B per lane, no VGPR round trip, no
// ds_write pass).  The DMA writes the LDS image lane-linearly (wave-uniform base + lane * 16 B), so one
// wave instruction fills 8 tile rows x 128 B and the LDS tile is an UNPADDED row-major [rows][64] image.
// Read back row-major, the 16 rows of an MFMA fragment would sit on two 16-byte slots (8-way conflict);
// instead piece p of row r is stored at slot p ^ ((r >> 1) & 7).  The permutation is applied to the
// per-lane SOURCE offset (lanes of a row still cover the same 128-byte line, so coalescing is unchanged)
// and to the ds_read_b128 address: the 16 rows of a fragment then land on 16 distinct slots of the
// 256-byte bank row (SQ_LDS_BANK_CONFLICT = 0 measured).
//
// Address generation is kept off the VALU (the first version spent 3.5 VALU instructions per MFMA on it):
// every operand row has ONE precomputed 32-bit byte offset (voffset) into a buffer descriptor; the K-tile
// position - filter tap and channel offset for a conv - is a wave-uniform SGPR (soffset).  Padding, masked
// rows and N/M edges use the descriptor's bounds check: an out-of-range voffset returns zeros, so a lane
// "predicates" its load with one v_cndmask on a precomputed 9-bit tap-validity mask.  The conv descriptor's
// base is shifted back by one row + one pixel so that tap offsets are non-negative.
//
// Pipeline: two LDS stages, ONE barrier per 64-deep K tile, loop unrolled by the stage parity so that every
// LDS address is base + immediate.  The DMA for tile k+1 is issued right after the barrier and lands while
// the 2 x (MT x NT) MFMAs of tile k run (and while the CU's second resident workgroup computes).
// All LDS lives in ONE __shared__ object: with two, hipcc drains the in-flight DMA before every ds_read.
//
// Workgroup ids are remapped so that each XCD (private 4 MiB L2, workgroup b -> XCD b % 8) owns a
// contiguous range of tiles, n fastest: the tiles that share an activation row panel hit the same L2.
#include "gemm_params.h"
#include <stdlib.h>

namespace {

constexpr int BK = 64;
constexpr unsigned OOB = 0x80000000u;     // voffset that fails the descriptor's range check -> zeros

typedef __attribute__((address_space(3))) void* lds_ptr_t;

__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t rsrc, half_t* lds_wave_base, unsigned voff,
                                      unsigned soff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_ptr_t)lds_wave_base, 16, voff, soff, 0, 0);
}

// Tile configurations: <BM, BN, WGM, WGN> = block tile and wave grid.
//   128 x {160,128,64}, 2 x 2 waves (wave tile 64 x BN/2), 2 workgroups per CU   - the general case
//   256 x 320,          2 x 4 waves (wave tile 128 x 80),  1 workgroup per CU    - 64x64-resolution layers:
//     half the L2->LDS bytes per output, the activation panel of an N = 320 layer is read exactly once
// ---- issue-order plan for one stage of the main loop (see `compute`) ---------------------------------------------
template <int MASK, int N>
__device__ __forceinline__ void sgb() {
  if constexpr (N > 0) __builtin_amdgcn_sched_group_barrier(MASK, N, 0);
}
constexpr int SGB_MFMA = 0x008, SGB_VMEM = 0x010, SGB_DSREAD = 0x100;
// one group of NT MFMAs; after each of the first R an LDS fragment read is issued, after each of the next V one
// LDS-DMA instruction of the NEXT stage
template <int NT, int R, int V>
__device__ __forceinline__ void sched_group() {
  if constexpr (NT > 0) {
    sgb<SGB_MFMA, 1>();
    if constexpr (R > 0) {
      sgb<SGB_DSREAD, 1>();
      sched_group<NT - 1, R - 1, V>();
    } else if constexpr (V > 0) {
      sgb<SGB_VMEM, 1>();
      sched_group<NT - 1, 0, V - 1>();
    } else {
      sgb<SGB_MFMA, NT - 1>();
    }
  }
}
// fragment reads: NT+1 up front, then RPG per group until all 2*(MT+NT) are issued
template <int MT, int NT>
constexpr int plan_initial() { return NT + 1; }
template <int MT, int NT>
constexpr int plan_reads(int g) {
  const int rpg = NT < 3 ? NT : 3;
  const int left = 2 * (MT + NT) - (NT + 1) - g * rpg;
  return left < 0 ? 0 : (left < rpg ? left : rpg);
}
// LDS-DMA instructions woven into group g: the MFMA slots its fragment reads leave free, until all nd are placed
template <int MT, int NT>
constexpr int plan_vmem(int g, int nd) {
  int left = nd;
  for (int h = 0; h <= g; ++h) {
    const int v = (NT - plan_reads<MT, NT>(h)) < left ? (NT - plan_reads<MT, NT>(h)) : left;
    if (h == g) return v;
    left -= v;
  }
  return 0;
}
template <int MT, int NT, int G, int VLEFT>
__device__ __forceinline__ void sched_groups() {
  if constexpr (G < 2 * MT) {
    constexpr int R = plan_reads<MT, NT>(G);
    constexpr int V = (NT - R) < VLEFT ? (NT - R) : VLEFT;
    sched_group<NT, R, V>();
    sched_groups<MT, NT, G + 1, VLEFT - V>();
  } else {
    static_assert(VLEFT == 0, "not every DMA instruction found a slot");
  }
}
template <int MT, int NT, int ND>
__device__ __forceinline__ void sched_plan() {
  static_assert(plan_reads<MT, NT>(MT - 1) <= NT, "more woven reads than MFMAs in a group");
  sgb<SGB_DSREAD, plan_initial<MT, NT>()>();
  sched_groups<MT, NT, 0, ND>();
}
// Workgroup barrier that orders LDS traffic only.  __syncthreads() is fence + barrier and hipcc lowers the fence to
// s_waitcnt vmcnt(0): in the epilogue that parks every wave until its global STORES are acknowledged (measured with
// the phase stamps below: ~3.7 us per 64-row slab, the largest single item of a short-K tile).
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// ---- optional phase stamps (make PHASES=1; tools/gemm_phases.py): per workgroup s_memtime at tile start, before the
// K loop, after it, after the first epilogue slab and at tile end, plus HW_ID / XCC_ID of wave 0 -------------------
#ifdef SKG_PHASES
__device__ unsigned long long g_phase[1 << 15][16];
#define SKG_PH(i) do { if (tid == 0 && vb < (1 << 15)) g_phase[vb][i] = __builtin_readcyclecounter(); } while (0)
#else
#define SKG_PH(i) do { } while (0)
#endif

// the epilogue of a split-K launch on 4 summed outputs (row m, columns n .. n + 3)
__device__ __forceinline__ void splitk_epilogue(const GemmParams& p, float4_t v, size_t m, int n) {
  if (p.bias) {
    const half4_t b = ld_half4(p.bias + (p.bias_pitch ? (m / (size_t)p.gn_hw) * (size_t)p.bias_pitch : 0) + n);      // (the sample's bias row)
    v[0] += (float)b[0]; v[1] += (float)b[1]; v[2] += (float)b[2]; v[3] += (float)b[3];
  }
  v *= p.alpha;
  if (p.res) {
    const half4_t r = ld_half4(p.res + m * p.ldr + n);
    v[0] += (float)r[0]; v[1] += (float)r[1]; v[2] += (float)r[2]; v[3] += (float)r[3];
  }
  if (p.res_lo) {      // accuracy mode: pair residual
    const half4_t r = ld_half4(p.res_lo + m * p.ldr + n);
    v[0] += (float)r[0]; v[1] += (float)r[1]; v[2] += (float)r[2]; v[3] += (float)r[3];
  }
  if (p.flags & SKG_EPI_RELU) {
    v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f);
  }
  if (p.flags & SKG_EPI_OUT_F32) {
    *reinterpret_cast<float4_t*>(reinterpret_cast<float*>(p.C) + m * p.ldc + n) = v;
  } else {
    half4_t o = {(half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3]};
    st_half4(reinterpret_cast<half_t*>(p.C) + m * p.ldc + n, o);
    if (p.c_lo) {      // accuracy mode: pair output, lo = fp16(v - hi)
      half4_t l = {(half_t)(v[0] - (float)o[0]), (half_t)(v[1] - (float)o[1]), (half_t)(v[2] - (float)o[2]), (half_t)(v[3] - (float)o[3])};
      st_half4(p.c_lo + m * p.ldc + n, l);
    }
  }
}

// NS = pipeline stages.  2: two workgroups per CU cover each other's DMA waits.  3: for launches with at most ONE
// workgroup per CU (<= 256 tiles) nothing else is resident, so the lone workgroup keeps two K tiles in flight instead
// (110 KB of LDS) and waits with a counted vmcnt.
// GNS: the instantiation whose epilogue also writes the GroupNorm partial sums of the output (launched only when asked
// for - its 25 extra epilogue registers and code cost the plain launches 0.3 % of a batch when they shared one kernel)
// HILO: the accuracy-mode instantiation (skg_*_hilo): the fp32-staged epilogue also adds p.res_lo and stores
// lo = fp16(v - fp16(v)) to p.c_lo, whatever the launch (an own instantiation: the plain kernels stay as tuned)
// BROWS: the instantiations for a bias row per sample (p.bias_pitch) on tiles that can span samples (launch_cfg: SKG_FLAG_BIAS_PER_ROW):
// always the fp32-staged epilogue, whose second phase owns ONE output row per thread and adds that row's bias row there (the slice in
// LDS stays zero), or the direct stores with a per-row lookup.  The plain instantiations only ever see tiles inside one sample.
template <int BM, int BN, int WGM, int WGN, int MODE, int NS, bool GNS, bool HILO, bool BROWS = false>
__device__ __forceinline__ void gemm2_body(const GemmParams& p, int tiles_n, int nwg, unsigned a_bytes, unsigned b_bytes,
                                           unsigned a_shift, int kt_per_split, float* __restrict__ ws) {
  constexpr int NW = WGM * WGN;       // waves
  constexpr int NTHR = NW * 64;
  constexpr int WM = BM / WGM;        // wave tile rows (64 or 128)
  constexpr int WN = BN / WGN;        // wave tile columns
  constexpr int NT = WN / 16;         // 5, 4 or 2
  constexpr int MT = WM / 16;         // 4 or 8
  constexpr int ACH = BM / 8 / NW;    // A 8-row chunks per wave (4)
  constexpr int BCH = BN / 8 / NW;    // B 8-row chunks per wave (5, 4, 2)
  static_assert(BM % (8 * NW) == 0 && BN % (8 * NW) == 0 && WM % 16 == 0 && WN % 16 == 0, "tile shape");
  constexpr int STAGE = (BM + BN) * BK;               // halves per stage: A tile then B tile
  constexpr bool AFFINE = (MODE == MODE_DIRECT || MODE == MODE_S1 || MODE == MODE_S2 || MODE == MODE_S2A);
  __shared__ __attribute__((aligned(16))) half_t smem[NS * STAGE + 2 * BN];     // the stages + the tile's fp32 bias slice

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WGN, wn = wave - wm * WGN;
  const int g = lane >> 4, l16 = lane & 15;

  // descriptors: A is based `a_shift` bytes BEFORE p.A (conv: one row + one pixel) so tap offsets are >= 0
  const __amdgpu_buffer_rsrc_t rA =
      __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)p.A - a_shift), 0, a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rB = __builtin_amdgcn_make_buffer_rsrc((void*)p.B, 0, b_bytes, 0x00020000);
  // second A operand (the folded 1x1 shortcut, MODE_S1 only): plain row-major rows, no halo
  const __amdgpu_buffer_rsrc_t rA2 = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(p.A2 ? p.A2 : p.A), 0, p.A2 ? ((unsigned)(p.M - 1) * (unsigned)p.lda2 + (unsigned)p.K2) * 2u : 0u, 0x00020000);
  const int KT1 = (MODE == MODE_S1 && p.K2) ? (p.K - p.K2) / BK : (1 << 30);      // first K tile of the second operand

  // Persistent workgroups: the grid holds at most one resident wave of workgroups; each walks tiles
  // vb = blockIdx.x, blockIdx.x + gridDim.x, ...  A workgroup's s_endpgm waits for all of its stores to be
  // acknowledged; inside the loop the stores of tile i simply drain under the main loop of tile i+1.
  // (gridDim.x is a multiple of 8 whenever it is smaller than nwg, so vb keeps the workgroup's XCD.)
  for (int vb = blockIdx.x; vb < nwg; vb += gridDim.x) {
  if (vb != (int)blockIdx.x) lds_barrier();        // previous tile's epilogue reads of the LDS staging area
  SKG_PH(0);
#ifdef SKG_PHASES
  if (tid == 0 && vb < (1 << 15)) {
    g_phase[vb][6] = __builtin_amdgcn_s_getreg((31 << 11) | 4);      // HW_ID
    g_phase[vb][7] = __builtin_amdgcn_s_getreg((31 << 11) | 20);     // XCC_ID
    g_phase[vb][5] = __builtin_amdgcn_s_getreg((31 << 11) | 6);      // LDS_ALLOC
  }
#endif
  // ---- XCD-aware tile assignment (bijective) ------------------------------------------------------
  int lid;
  {
    const int bid = vb;
    const int xcd = bid & 7, idx = bid >> 3;
    const int q = nwg >> 3, r = nwg & 7;
    lid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  // split-K: workgroups [s * ntiles, (s+1) * ntiles) own K tiles [s * kt_per_split, ...) and write fp32 slab s
  const int ntiles = ws ? nwg / ((p.K / BK + kt_per_split - 1) / kt_per_split) : nwg;
  const int split = lid / ntiles;
  lid -= split * ntiles;
  // polyphase upsample: phase 2a + b of this tile (p.up2 = 1 + phase: one launch per phase; 5: all four phases in this
  // launch, tiles [ph * ntiles / 4, (ph + 1) * ntiles / 4) - the small maps, where one phase does not fill the chip)
  int ph = p.up2 ? p.up2 - 1 : 0;
  if (p.up2 == 5) {
    const int per = ntiles >> 2;
    ph = lid / per;
    lid -= ph * per;
  }
  int tile_m = lid / tiles_n;
  int tile_n = lid - tile_m * tiles_n;
  // Weight-heavy launches (16x16 / 8x8 levels: W = 30-60 MB, A = 10-20 MB): with the plain order every XCD walks all
  // column panels, so each of the 8 L2s pulls the WHOLE weight matrix through the fabric.  The host then picks an
  // gm x gn arrangement of the XCDs over the tile grid (flags bits 20-23 = gn; only when everything divides evenly):
  // XCD (xm, xn) owns row block xm and column block xn, fabric traffic ~ gn * A + gm * W.
  // Split-K launches: a K slice spans G = 8 / splits XCDs (flags bits 24-27, 0 = all 8) and the arrangement is made
  // inside that group - `lid` is already the index inside the slice.
  if (const int gn = (p.flags >> 20) & 0xf) {
    const int G = ((p.flags >> 24) & 0xf) ? (int)((p.flags >> 24) & 0xf) : 8;
    const int per = ntiles / G, tmb = (ntiles / tiles_n) / (G / gn), tnb = tiles_n / gn;
    const int xr = lid / per, r = lid - xr * per;
    const int xm = xr / gn, xn = xr - xm * gn;
    const int rm = r / tnb;
    tile_m = xm * tmb + rm;
    tile_n = xn * tnb + (r - rm * tnb);
  }
  const int m0 = tile_m * BM, n0 = tile_n * BN;

  // ---- per-lane DMA source description ---------------------------------------------------------------
  const int lr = lane >> 3;           // row within an 8-row chunk
  const int lq = lane & 7;            // LDS slot this lane fills
  unsigned a_voff[ACH];               // byte offset of (row, logical piece) at tap (0,0) / k = 0, or OOB
  unsigned a_mask[ACH];               // S1/S2: bit t set <=> tap t reads a pixel inside the image
  int a_oy[ACH], a_ox[ACH];           // UP2/S2T only
  unsigned a_img[ACH];                // UP2/S2T: byte offset of the image + piece
  int smp0 = 0;                       // conv: the sample of this lane's first row (lane 0 of a wave: of a row in the tile's first 32)
#pragma unroll
  for (int j = 0; j < ACH; ++j) {
    const int r = (j * NW + wave) * 8 + lr;
    const unsigned pk = (unsigned)(lq ^ ((r >> 1) & 7)) * 16u;      // byte offset of the logical piece
    const int m = m0 + r;
    const bool ok = m < p.M;
    const int mm = ok ? m : 0;
    a_mask[j] = 0; a_oy[j] = a_ox[j] = 0; a_img[j] = 0;
    if (MODE == MODE_DIRECT) {
      a_voff[j] = ok ? (unsigned)mm * (unsigned)p.lda * 2u + pk : OOB;
    } else {
      const int ohw = p.OH * p.OW;
      const int b = mm / ohw;
      if (j == 0) smp0 = b;
      const int rr = mm - b * ohw;
      const int oy = rr / p.OW, ox = rr - oy * p.OW;
      const unsigned img = (unsigned)b * (unsigned)(p.IH * p.IW);
      if (MODE == MODE_S1 || MODE == MODE_S2 || MODE == MODE_S2A) {
        // centre pixel of output (oy, ox): stride 1 / stride 2 with padding 1 / stride 2 with padding (0,1,0,1)
        const int cy = MODE == MODE_S1 ? oy : 2 * oy + (MODE == MODE_S2A), cx = MODE == MODE_S1 ? ox : 2 * ox + (MODE == MODE_S2A);
        // with the shifted base, tap (ky,kx) of this row is at voff + ((ky*IW + kx)*lda + c0)*2
        a_voff[j] = ok ? ((img + (unsigned)(cy * p.IW + cx)) * (unsigned)p.lda) * 2u + pk : OOB;
        unsigned mk = 0;
        if (MODE == MODE_S2 && p.ntaps == 16) {      // 4 x 4 stride-2 window, rows 2 oy - 1 .. 2 oy + 2 (skg_conv4x4s2_f16)
#pragma unroll
          for (int t = 0; t < 16; ++t) {
            const int iy = cy + (t >> 2) - 1, ix = cx + (t & 3) - 1;
            if (ok && iy >= 0 && iy < p.IH && ix >= 0 && ix < p.IW) mk |= 1u << t;
          }
        } else {
#pragma unroll
          for (int t = 0; t < 9; ++t) {
            const int iy = cy + t / 3 - 1, ix = cx + t % 3 - 1;
            if (ok && iy >= 0 && iy < p.IH && ix >= 0 && ix < p.IW) mk |= 1u << t;
          }
        }
        a_mask[j] = mk;
      } else {
        a_voff[j] = ok ? 0u : OOB;
        a_oy[j] = oy; a_ox[j] = ox;
        a_img[j] = img * (unsigned)p.lda * 2u + pk + a_shift;
      }
    }
  }
  unsigned b_voff[BCH];
#pragma unroll
  for (int j = 0; j < BCH; ++j) {
    const int r = (j * NW + wave) * 8 + lr;
    const unsigned pk = (unsigned)(lq ^ ((r >> 1) & 7)) * 16u;
    const int n = n0 + r;
    b_voff[j] = n < p.N ? ((unsigned)n + (p.up2 == 5 ? (unsigned)(ph * p.N) : 0u)) * (unsigned)p.ldb * 2u + pk : OOB;
  }

  // LDS-DMA of K tile kt into stage `buf`, split into the per-step address part (`dma_prepare`: SALU + a few VALU
  // selects) and the individual instructions (`dma_one`, d = 0 .. ACH+BCH-1) so that the main loop can place each
  // instruction between MFMAs.  !live: every lane out of range -> zero fill, no memory traffic.
  const bool tap_minor = (p.flags & 0x1000u) != 0;
  struct DmaStep { unsigned va[ACH]; unsigned vb[BCH]; unsigned soa, sob; bool second; };
  auto dma_prepare = [&](int kt, bool live) {
    DmaStep d;
    d.second = false;
    if (MODE == MODE_S1 && kt >= KT1) {      // (wave-uniform) the shortcut operand: row m of A2, channels (kt - KT1) * 64 ..
      d.second = true;
#pragma unroll
      for (int j = 0; j < ACH; ++j) {
        const int r = (j * NW + wave) * 8 + lr;
        const unsigned pk = (unsigned)(lq ^ ((r >> 1) & 7)) * 16u;
        d.va[j] = (live && m0 + r < p.M) ? (unsigned)(m0 + r) * (unsigned)p.lda2 * 2u + pk : OOB;
      }
#pragma unroll
      for (int j = 0; j < BCH; ++j) d.vb[j] = live ? b_voff[j] : OOB;
      d.soa = (unsigned)(kt - KT1) * (BK * 2u);
      d.sob = (unsigned)kt * (BK * 2u);          // the weight row is [9 taps x Cin | K2]: position kt * 64 either way
      return d;
    }
    const int k0 = kt * BK;
    unsigned soff = (unsigned)k0 * 2u;
    int tap = 0, ky = 0, kx = 0, c0 = 0;
    unsigned kb = (unsigned)k0;            // position of this K tile in a weight row
    if (MODE != MODE_DIRECT) {
      // K order of the implicit GEMM: channel block outermost, the 9 taps innermost (the weight pack stays
      // [Cout][tap][Cin]; only the walk changes).  A tile then re-reads the SAME 64-channel slice of its ~3 input rows
      // for nine consecutive K steps - 32 KB per workgroup instead of the whole 3-row halo of all channels - so the
      // slices of all workgroups of an XCD fit its 4 MB L2 (tap-major order: 2.5 x the algorithmic bytes fetched
      // from beyond L2, rocprofv3 FETCH_SIZE).
      int ti;                              // position in the tap walk = position in the weight pack
      if (tap_minor) {
        const int nt = p.ntaps ? p.ntaps : 9;
        const int cb = kt / nt;
        ti = kt - cb * nt;
        c0 = cb * BK;
      } else {
        ti = k0 / p.Cin;
        c0 = k0 - ti * p.Cin;
      }
      kb = (unsigned)(ti * p.Cin + c0);
      if (MODE == MODE_S2 && p.ntaps == 16) {      // 4 x 4 window
        tap = ti;
        ky = ti >> 2;
        kx = ti & 3;
      } else {
        // polyphase launches walk a 2 x 2 subset of the stride-1 taps: rows {a, a + 1}, columns {b, b + 1} of the 3 x 3 ids
        const unsigned tapmap = p.up2 == 5 ? (unsigned)((ph >> 1) * 3 + (ph & 1)) * 0x1111u + 0x4310u : p.tapmap;
        tap = p.ntaps ? (int)((tapmap >> (4 * ti)) & 0xfu) : ti;
        ky = tap / 3;
        kx = tap - ky * 3;
      }
      const int ca = (p.a_wrap && c0 >= p.a_wrap) ? c0 - p.a_wrap : c0;      // (accuracy-mode polyphase: the x_hi block is read twice)
      soff = (unsigned)((ky * p.IW + kx) * p.lda + ca) * 2u;
    }
#pragma unroll
    for (int j = 0; j < ACH; ++j) {
      unsigned v;
      if (MODE == MODE_DIRECT) {
        v = a_voff[j];
      } else if (AFFINE) {
        v = (a_mask[j] >> tap) & 1u ? a_voff[j] : OOB;
      } else {
        const int ty = a_oy[j] + ky - 1, tx = a_ox[j] + kx - 1;
        bool ok = a_voff[j] != OOB;
        int iy, ix;
        if (MODE == MODE_UP2) {
          ok = ok && ty >= 0 && ty < p.OH && tx >= 0 && tx < p.OW;
          iy = ty >> 1; ix = tx >> 1;
        } else {   // MODE_S2T
          ok = ok && ty >= 0 && tx >= 0 && !(ty & 1) && !(tx & 1);
          iy = ty >> 1; ix = tx >> 1;
          ok = ok && iy < p.IH && ix < p.IW;
        }
        v = ok ? a_img[j] + (unsigned)((iy * p.IW + ix) * p.lda) * 2u : OOB;
      }
      d.va[j] = live ? v : OOB;
    }
#pragma unroll
    for (int j = 0; j < BCH; ++j) d.vb[j] = live ? b_voff[j] : OOB;
    d.soa = AFFINE ? soff : (unsigned)c0 * 2u;     // gather modes carry the pixel in voffset
    d.sob = kb * 2u;
    return d;
  };
  auto dma_one = [&](const DmaStep& d, int buf, int i) {     // buf, i: compile-time constants at every call site
    if (i < ACH) dma16(d.second ? rA2 : rA, &smem[buf * STAGE + (i * NW + wave) * 8 * BK], d.va[i], d.soa);
    else dma16(rB, &smem[buf * STAGE + BM * BK + ((i - ACH) * NW + wave) * 8 * BK], d.vb[i - ACH], d.sob);
  };

  float4_t acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = float4_t{0.f, 0.f, 0.f, 0.f};

  // fragment read addresses (halves) inside a stage for k-step 0 / 1; slot = piece ^ ((row >> 1) & 7)
  int a_ad[MT][2], b_ad[NT][2];
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int row = wm * WM + i * 16 + l16;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) a_ad[i][ks] = row * BK + (((ks * 4 + g) ^ ((row >> 1) & 7)) << 3);
  }
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int row = wn * WN + j * 16 + l16;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) b_ad[j][ks] = BM * BK + row * BK + (((ks * 4 + g) ^ ((row >> 1) & 7)) << 3);
  }

  // One pipeline step = the LDS-DMA of the next K tile + 2 k-steps x MT row groups of NT MFMAs on the current one, as
  // ONE basic block whose issue order is pinned with sched_group_barrier.  Two things hipcc does not do by itself:
  //  * a buffer_load...lds occupies its wave for ~100 cycles (the texture path takes 64 B/clk per CU), so issuing the
  //    9 DMA instructions of a stage back to back ahead of the MFMAs costs ~a third of the step; woven one by one
  //    between MFMAs they run under the matrix pipe;
  //  * hipcc keeps ONE x-fragment register set and emits ds_read -> s_waitcnt lgkmcnt(0) -> NT MFMAs per group,
  //    exposing the LDS latency 2*MT times per stage.  All fragment reads are issued at least one group (NT*16
  //    cycles) ahead of their first use.
  // LDS reads and LDS-DMA writes keep their program order, so the source below emits them in exactly the order
  // the plan wants (reads of group g, then the DMA instructions of group g); the MFMAs are free to move and the
  // plan drops them in between.  The DMA is unconditional (out of range on the last step: zero fill into the idle
  // stage) to keep the block whole.
  constexpr int ND = ACH + BCH;
  auto step = [&](int knext, int ibuf, int cbuf, int KT_) {
    const DmaStep d = dma_prepare(knext, knext < KT_);
    const half_t* sb = &smem[cbuf * STAGE];
    if constexpr (MT >= 8) {      // 160 accumulator registers: no room to pre-load every fragment
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        half8_t xf[MT], wf[NT];
#pragma unroll
        for (int i = 0; i < MT; ++i) xf[i] = ld_half8(sb + a_ad[i][ks]);
#pragma unroll
        for (int j = 0; j < NT; ++j) wf[j] = ld_half8(sb + b_ad[j][ks]);
        if (ks == 1) {
#pragma unroll
          for (int i = 0; i < ND; ++i) dma_one(d, ibuf, i);
        }
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int j = 0; j < NT; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[j], xf[i], acc[i][j], 0, 0, 0);
      }
      return;
    }
    half8_t xf[2][MT], wf[2][NT];
    auto rd = [&](int idx) {     // fragment reads in order of first use: w[0][*], x[0][*], w[1][*], x[1][*]
      if (idx < NT) wf[0][idx] = ld_half8(sb + b_ad[idx][0]);
      else if (idx < NT + MT) xf[0][idx - NT] = ld_half8(sb + a_ad[idx - NT][0]);
      else if (idx < 2 * NT + MT) wf[1][idx - NT - MT] = ld_half8(sb + b_ad[idx - NT - MT][1]);
      else xf[1][idx - 2 * NT - MT] = ld_half8(sb + a_ad[idx - 2 * NT - MT][1]);
    };
    int ri = 0, di = 0;          // compile-time after unrolling
#pragma unroll
    for (int r = 0; r < plan_initial<MT, NT>(); ++r) rd(ri++);
#pragma unroll
    for (int gq = 0; gq < 2 * MT; ++gq) {
#pragma unroll
      for (int r = 0; r < plan_reads<MT, NT>(gq); ++r) rd(ri++);
#pragma unroll
      for (int v = 0; v < plan_vmem<MT, NT>(gq, ND); ++v) dma_one(d, ibuf, di++);
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[ks][j], xf[ks][i], acc[i][j], 0, 0, 0);
    sched_plan<MT, NT, ND>();
  };

  const int kt_begin = split * kt_per_split;
  const int KT = min(p.K / BK, kt_begin + kt_per_split);
  // the tile's bias slice is fetched now and parked in a register until the epilogue puts it into LDS
  float bias_r = 0.f;
  if constexpr (!BROWS) {
    // (a bias row per sample: the whole tile lies inside one sample, the one the DMA description above already found for the
    // rows of lane 0 - a scalar; bias_pitch = 0: the shared row)
    const half_t* bias_t = p.bias;
    if constexpr (MODE != MODE_DIRECT) bias_t += __builtin_amdgcn_readfirstlane(smp0) * p.bias_pitch;
    bias_r = (tid < BN && p.bias && n0 + tid < p.N) ? (float)bias_t[n0 + tid] : 0.f;
  }
  SKG_PH(1);
  {
    const DmaStep d0 = dma_prepare(kt_begin, true);
#pragma unroll
    for (int i = 0; i < ND; ++i) dma_one(d0, 0, i);
  }
  if constexpr (NS == 2) {
    for (int kt = kt_begin; kt < KT; kt += 2) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      lds_barrier();
      step(kt + 1, 1, 0, KT);
      if (kt + 1 < KT) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        lds_barrier();
        step(kt + 2, 0, 1, KT);
      }
    }
  } else {
    static_assert(NS >= 3 && (NS - 2) * ND <= 63, "counted wait");
#pragma unroll
    for (int s = 1; s < NS - 1; ++s) {
      const DmaStep d1 = dma_prepare(kt_begin + s, kt_begin + s < KT);
#pragma unroll
      for (int i = 0; i < ND; ++i) dma_one(d1, s, i);
    }
    // every step issues exactly ND DMA instructions per thread (dead ones are out-of-range zero fills) and loads
    // retire in order, so "at most (NS-2)*ND outstanding" == the K tile about to be computed has landed.  The counting
    // starts from a drained queue (the bias load and the first NS-1 tiles), so that only DMA loads are ever counted.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    for (int kt = kt_begin; kt < KT; kt += NS) {
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        if (kt + s < KT) {
          asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NS - 2) * ND) : "memory");
          lds_barrier();
          step(kt + s + NS - 1, (s + NS - 1) % NS, s, KT);
        }
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the last steps' zero-fill DMA must not land in the staging area

  SKG_PH(2);
#ifdef SKG_PHASES
  if ((tid & 63) == 0 && vb < (1 << 15)) g_phase[vb][12 + (tid >> 6)] = __builtin_readcyclecounter();
#endif
  // ---- epilogue: lane holds C[m = .. + l16][n = .. + 4g .. 4g+3] -----------------------------------
  // Outputs that cannot stay in the 32 MB of L2 anyway are stored non-temporally: a write-allocated 336 MB FF1 output
  // otherwise evicts the activation panel and the weights every other workgroup is still streaming (N = 2560, K = 320:
  // 185 vs 239 us); small outputs stay cacheable for the consumer kernel.
  const bool stream_out = p.flags & 0x800u;
  const bool relu = p.flags & SKG_EPI_RELU;
  const bool f32out = p.flags & SKG_EPI_OUT_F32;
  if (ws) {   // split-K partial: raw fp32 accumulators, epilogue happens in splitk_reduce_kernel
    float* slab = ws + (size_t)split * p.M * p.N;
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const int m = m0 + wm * WM + i * 16 + l16;
      if (m >= p.M) continue;
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int n = n0 + wn * WN + j * 16 + g * 4;
        if (n < p.N) {
          *reinterpret_cast<float4_t*>(slab + (size_t)m * p.N + n) = acc[i][j];
        }
      }
    }
    continue;
  }
  const bool staged = HILO ||      // (launcher-checked alignment)
                      (!f32out && (p.ldc % 8 == 0) && ((reinterpret_cast<uintptr_t>(p.C) & 15) == 0) &&
                       (!p.res || ((p.ldr % 8 == 0) && (reinterpret_cast<uintptr_t>(p.res) & 15) == 0)));
  // GroupNorm statistics of this tile's OUTPUT (launcher-checked: 128 x 160 tile, whole tiles, groups do not straddle the
  // tile, staged epilogue): phase 2 of either staged path keeps, per 16-byte piece it stores, sum(y) and sum(y^2) of the
  // four fp16 pairs (v_dot2: two values per instruction, no conversions; a pair never straddles a group because the
  // group width is even); gn_fold() reduces them over the tile's rows in a fixed order (bitwise reproducible).
  constexpr bool gn = GNS;
  constexpr int GNP = (BN / 8) / (NTHR / 64);       // pieces per thread and row (5 for the 128 x 160 tile)
  float gs[GNP][4][2];
#pragma unroll
  for (int k = 0; k < GNP; ++k)
#pragma unroll
    for (int q = 0; q < 4; ++q) gs[k][q][0] = gs[k][q][1] = 0.f;
  auto gn_acc = [&](int k, const half8_t& y) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    const h2 one = {(_Float16)1.f, (_Float16)1.f};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const h2 v = {y[2 * q], y[2 * q + 1]};
      gs[k][q][0] = __builtin_amdgcn_fdot2(v, one, gs[k][q][0], false);
      gs[k][q][1] = __builtin_amdgcn_fdot2(v, v, gs[k][q][1], false);
    }
  };
  auto gn_fold = [&]() {
    if constexpr (BM == 128 && NTHR == 256 && BN == 160) {
      // thread (er = tid / 4, tq = tid % 4): the four row lanes of a 16-lane DPP row that share tq are summed in registers
      // (rotations by 4 and 8), so 64 threads write and the LDS fold walks 16 slots instead of 64
      float* const red = reinterpret_cast<float*>(smem);                  // [16 slots][4 tq][GNP * 8]: 10 KB of the dead stages
      float* const csum = red + 64 * GNP * 8;                             // [BN]: (column pair, quantity) totals
#pragma unroll
      for (int k = 0; k < GNP; ++k)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int z = 0; z < 2; ++z) gs[k][q][z] = dpp_add<0x124>(dpp_add<0x128>(gs[k][q][z]));
      lds_barrier();                                                      // phase-2 reads of the staging slab are done
      if ((tid & 15) < 4) {
        float* const dst = red + ((tid >> 4) * 4 + (tid & 3)) * (GNP * 8);
#pragma unroll
        for (int k = 0; k < GNP; ++k) {
          *reinterpret_cast<float4_t*>(dst + k * 8) = float4_t{gs[k][0][0], gs[k][0][1], gs[k][1][0], gs[k][1][1]};
          *reinterpret_cast<float4_t*>(dst + k * 8 + 4) = float4_t{gs[k][2][0], gs[k][2][1], gs[k][3][0], gs[k][3][1]};
        }
      }
      lds_barrier();
      if (tid < BN) {      // column pair cp = (8 tq + 32 k) / 2 + q
        const int cp = tid >> 1, qq = tid & 1;
        const int off = ((cp & 15) >> 2) * (GNP * 8) + (cp >> 4) * 8 + (cp & 3) * 2 + qq;
        float t = 0.f;
#pragma unroll
        for (int sl2 = 0; sl2 < 16; ++sl2) t += red[sl2 * 4 * (GNP * 8) + off];
        csum[tid] = t;
      }
      lds_barrier();
      const int cpg = p.N / p.gn_groups, ngr = BN / cpg;
      if (tid < 2 * ngr) {
        const int gi = tid >> 1, qq = tid & 1;
        float t = 0.f;
        for (int c = 0; c < (cpg >> 1); ++c) t += csum[(gi * (cpg >> 1) + c) * 2 + qq];
        const int nch = p.gn_hw >> 7, b = m0 / p.gn_hw, chunk = (m0 - b * p.gn_hw) >> 7;
        p.gn_partial[(((size_t)b * nch + chunk) * p.gn_groups + n0 / cpg + gi) * 2 + qq] = t;
      }
    }
  };
  if (staged && !p.res && !HILO && !BROWS) {
    // No residual: bias, alpha and ReLU are applied in registers and the value is rounded to fp16 (its final rounding;
    // for the fused GEGLU the same rounding the unfused path and the reference apply to the FF1 output) BEFORE it
    // goes through LDS - half the staging bytes, all 128 rows in one slab, every wave writes at once, two barriers
    // instead of four; phase 2 is then a plain 16-byte LDS read + 16-byte store per piece.
    constexpr int OPH = BN + 8;                // staging pitch (halves)
    constexpr int HROWS = 128;
    constexpr int HSLABS = BM / HROWS;
    constexpr int PPR = BN / 8;
    constexpr int TPR2 = NTHR / 64;            // threads per staged row (4 or 8): 64-byte runs per row and store
    constexpr int IT2 = PPR / TPR2;            // instruction (32-byte runs - two threads per row - store at half the rate)
    constexpr int RPT = HROWS / 64;            // rows per thread: er, er + 64
    static_assert(HROWS * OPH * 2 <= 2 * STAGE * 2 && NTHR % 64 == 0 && PPR % TPR2 == 0, "fp16 staging slab");
    half_t* const hst = smem;
    float* const bias_s = reinterpret_cast<float*>(smem + NS * STAGE);
    const int er = tid / TPR2, ec = (tid % TPR2) * 8;
    const bool geglu = p.flags & SKG_EPI_GEGLU;
    if (tid < BN) bias_s[tid] = bias_r;
    half_t* const crow0 = reinterpret_cast<half_t*>(p.C) + (size_t)(m0 + er) * p.ldc + n0 + ec;
#pragma unroll
    for (int sl = 0; sl < HSLABS; ++sl) {
      lds_barrier();
      if (sl == 0) SKG_PH(8);
      if (WM < HROWS || wm == sl) {
        // (a lone wave issues one VALU instruction per ~8 cycles - tools/ubench/valu_rate.hip - so this block is
        // priced by its instruction count: one packed FMA per two values, ReLU behind a REAL branch; written as a
        // select hipcc emits 2 x 80 v_max_f32 for every launch)
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          const float4_t b4 = *reinterpret_cast<const float4_t*>(&bias_s[wn * WN + j * 16 + g * 4]) * p.alpha;
#pragma unroll
          for (int i = 0; i < MT; ++i) acc[i][j] = acc[i][j] * p.alpha + b4;
        }
        if (relu) {
          asm volatile("" ::: "memory");           // not if-convertible
#pragma unroll
          for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
              for (int e = 0; e < 4; ++e) acc[i][j][e] = fmaxf(acc[i][j][e], 0.f);
        }
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
          for (int i = 0; i < MT; ++i) {
            const float4_t v = acc[i][j];
            const half4_t h = {(half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3]};
            const int row = (WM < HROWS ? wm * WM : 0) + i * 16 + l16;
            *reinterpret_cast<half4_t*>(&hst[row * OPH + wn * WN + j * 16 + g * 4]) = h;
          }
      }
      if (sl == 0) SKG_PH(9);
      lds_barrier();
      if (sl == 0) { SKG_PH(10); SKG_PH(11); SKG_PH(3); }
      if (geglu && TPR2 >= 8) {
        // eight threads per row: 8-byte outputs already form 64-byte runs (the 256 x 320 tile)
#pragma unroll
        for (int hr = 0; hr < RPT; ++hr) {
          if (m0 + sl * HROWS + hr * 64 + er >= p.M) continue;
          const half_t* const srow = hst + (hr * 64 + er) * OPH + ec;
          half_t* const crow = reinterpret_cast<half_t*>(p.C) + (size_t)(m0 + sl * HROWS + hr * 64 + er) * p.ldc + ((n0 + ec) >> 1);
#pragma unroll
          for (int k = 0; k < IT2; ++k) {
            if (n0 + ec + k * TPR2 * 8 >= p.N) continue;
            const half8_t a = ld_half8(srow + k * TPR2 * 8);
            half4_t y = {(half_t)((float)a[0] * gelu_fast_f((float)a[2])), (half_t)((float)a[1] * gelu_fast_f((float)a[3])),
                         (half_t)((float)a[4] * gelu_fast_f((float)a[6])), (half_t)((float)a[5] * gelu_fast_f((float)a[7]))};
            half4_t* dst4 = reinterpret_cast<half4_t*>(crow + k * TPR2 * 4);
            if (stream_out) asm volatile("global_store_dwordx2 %0, %1, off nt\n\ts_nop 1" ::"v"(dst4), "v"(y) : "memory");
            else *dst4 = y;
            if (p.aux) {      // the pre-activation too (what the backward of the gate needs)
              half8_t* h8 = reinterpret_cast<half8_t*>(p.aux + (size_t)(m0 + sl * HROWS + hr * 64 + er) * p.ldaux + n0 + ec + k * TPR2 * 8);
              asm volatile("global_store_dwordx4 %0, %1, off nt\n\ts_nop 1" ::"v"(h8), "v"(a) : "memory");
            }
          }
        }
        continue;
      }
      if (geglu) {
        // interleaved FF1 pack: 16 staged columns [a0 a1 g0 g1 | a2 a3 g2 g3] x 2 -> 8 outputs a * gelu(g) = ONE
        // 16-byte store; consecutive lanes take consecutive 16-byte pieces of an output row (whole-row runs - the
        // 8-byte-per-thread form left 32-byte runs per row and instruction, which store at half the rate)
        constexpr int QPR = PPR / 2;               // 16-byte output pieces per tile row
        static_assert(HROWS * QPR % NTHR == 0, "GEGLU piece loop");
#pragma unroll
        for (int k = 0; k < HROWS * QPR / NTHR; ++k) {
          const int pi = tid + k * NTHR;
          const int row = pi / QPR, pp = pi - row * QPR;
          if (m0 + sl * HROWS + row >= p.M || n0 + pp * 16 >= p.N) continue;
          const half8_t a = ld_half8(hst + row * OPH + pp * 16), b = ld_half8(hst + row * OPH + pp * 16 + 8);
          half8_t y = {(half_t)((float)a[0] * gelu_fast_f((float)a[2])), (half_t)((float)a[1] * gelu_fast_f((float)a[3])),
                       (half_t)((float)a[4] * gelu_fast_f((float)a[6])), (half_t)((float)a[5] * gelu_fast_f((float)a[7])),
                       (half_t)((float)b[0] * gelu_fast_f((float)b[2])), (half_t)((float)b[1] * gelu_fast_f((float)b[3])),
                       (half_t)((float)b[4] * gelu_fast_f((float)b[6])), (half_t)((float)b[5] * gelu_fast_f((float)b[7]))};
          half8_t* dst8 = reinterpret_cast<half8_t*>(reinterpret_cast<half_t*>(p.C) + (size_t)(m0 + sl * HROWS + row) * p.ldc +
                                                     (n0 >> 1) + pp * 8);
          if (stream_out) asm volatile("global_store_dwordx4 %0, %1, off nt\n\ts_nop 1" ::"v"(dst8), "v"(y) : "memory");
          else *dst8 = y;
          if (p.aux) {        // the pre-activation too (what the backward of the gate needs): 32 contiguous bytes
            half_t* const hrow = p.aux + (size_t)(m0 + sl * HROWS + row) * p.ldaux + n0 + pp * 16;
            asm volatile("global_store_dwordx4 %0, %1, off nt\n\ts_nop 1" ::"v"(hrow), "v"(a) : "memory");
            asm volatile("global_store_dwordx4 %0, %1, off nt\n\ts_nop 1" ::"v"(hrow + 8), "v"(b) : "memory");
          }
        }
        continue;
      }
#pragma unroll
      for (int hr = 0; hr < RPT; ++hr) {
        if (m0 + sl * HROWS + hr * 64 + er >= p.M) continue;
        const half_t* const srow = hst + (hr * 64 + er) * OPH + ec;
        half_t* crow = crow0 + (size_t)(sl * HROWS + hr * 64) * p.ldc;
        if (p.up2) {      // polyphase upsample: low-res pixel (i, j) of image b -> high-res pixel (2 i + a, 2 j + b)
          const int m = m0 + sl * HROWS + hr * 64 + er, hw = p.OH * p.OW;
          const int img = m / hw, rr = m - img * hw, i = rr / p.OW, j = rr - i * p.OW;
          const size_t r = (size_t)img * 4 * hw + (size_t)(2 * i + (ph >> 1)) * (2 * p.OW) + 2 * j + (ph & 1);
          crow = reinterpret_cast<half_t*>(p.C) + r * p.ldc + n0 + ec;
        } else if (p.seg_rows) {      // segmented output rows: batch row b's block goes to rows [b * seg_stride, b * seg_stride + seg_rows)
          const int m = m0 + sl * HROWS + hr * 64 + er, b = m / p.seg_rows;
          crow = reinterpret_cast<half_t*>(p.C) + ((size_t)b * p.seg_stride + (m - b * p.seg_rows)) * p.ldc + n0 + ec;
        }
        half8_t hv[IT2];
#pragma unroll
        for (int k = 0; k < IT2; ++k) hv[k] = ld_half8(srow + k * TPR2 * 8);
        if constexpr (IT2 == GNP) {
          if (gn) {
#pragma unroll
            for (int k = 0; k < IT2; ++k) gn_acc(k, hv[k]);
          }
        }
#pragma unroll
        for (int k = 0; k < IT2; ++k) {
          if (n0 + ec + k * TPR2 * 8 >= p.N) continue;
          half8_t* dst8 = reinterpret_cast<half8_t*>(crow + k * TPR2 * 8);
          if (stream_out) asm volatile("global_store_dwordx4 %0, %1, off nt\n\ts_nop 1" ::"v"(dst8), "v"(hv[k]) : "memory");
          else *dst8 = hv[k];
        }
      }
    }
    if (gn) gn_fold();
    SKG_PH(4);
    continue;
  }
  if (staged) {
    // The raw fp32 accumulators go through LDS (the pipeline stages are dead now), 64 tile rows at a time:
    // phase 1 is branch-free register -> LDS traffic; phase 2 walks whole output rows with 16-byte residual
    // loads / 16-byte stores (full 320-byte lines instead of 8-byte fragments of 16 different rows), applies
    // bias, alpha, residual and ReLU in fp32 and rounds to fp16 once.
    constexpr int OPF = BN + 4;                // staging pitch (floats)
    constexpr int SROWS = 64;
    constexpr int SLABS = BM / SROWS;
    static_assert(SROWS * OPF * 4 <= 2 * STAGE * 2, "staging slab must fit in the pipeline stages");
    constexpr int PPR = BN / 8;                // 8-column pieces per tile row
    constexpr int TPR = NTHR / SROWS;          // threads per staged row (4 or 8): a thread keeps ONE row of the slab
    constexpr int ITER = PPR / TPR;            // and walks pieces ec/8 + k * TPR of it (5, 4 or 2 of them)
    static_assert(NTHR % SROWS == 0 && PPR % TPR == 0, "piece loop must have a compile-time trip count");
    float* const stg = reinterpret_cast<float*>(smem);
    float* const bias_s = reinterpret_cast<float*>(smem + NS * STAGE);     // own area behind the stages
    const int er = tid / TPR, ec = (tid % TPR) * 8;
    if (tid < BN) bias_s[tid] = bias_r;        // visible after the first barrier below
    // all residual loads of the tile are issued before the first store: vmcnt retires in order, so a load issued
    // behind a store could not be waited for without waiting for the store's acknowledgement too
    constexpr bool RES_UP_FRONT = SLABS * ITER <= 10;
    half8_t rv[SLABS][ITER];
    const half_t* const rrow0 = p.res ? p.res + (size_t)(m0 + er) * p.ldr + n0 + ec : nullptr;
    auto load_res = [&](int sl) {
      const bool rowok = p.res && m0 + sl * SROWS + er < p.M;
#pragma unroll
      for (int k = 0; k < ITER; ++k)
        rv[sl][k] = (rowok && n0 + ec + k * TPR * 8 < p.N)
                        ? ld_half8(rrow0 + (size_t)sl * SROWS * p.ldr + k * TPR * 8) : zero_half8();
    };
    if (RES_UP_FRONT) {
#pragma unroll
      for (int sl = 0; sl < SLABS; ++sl) load_res(sl);
    }
    half_t* const crow0 = reinterpret_cast<half_t*>(p.C) + (size_t)(m0 + er) * p.ldc + n0 + ec;
#pragma unroll
    for (int sl = 0; sl < SLABS; ++sl) {
      if (sl == 1) SKG_PH(11);
      lds_barrier();                           // stage reads (slab 0) / previous slab's reads are done
      if (sl == 1) SKG_PH(3);
      if (sl == 0) SKG_PH(8);
      if (wm == (sl * SROWS) / WM) {           // the bias joins the accumulators on their way into the staging slab
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          const float4_t b4 = *reinterpret_cast<const float4_t*>(&bias_s[wn * WN + j * 16 + g * 4]);
#pragma unroll
          for (int ii = 0; ii < SROWS / 16; ++ii) {
            const int i = ((sl * SROWS) % WM) / 16 + ii;
            *reinterpret_cast<float4_t*>(&stg[(ii * 16 + l16) * OPF + wn * WN + j * 16 + g * 4]) = acc[i][j] + b4;
          }
        }
      }
      if (sl == 0) SKG_PH(9);
      lds_barrier();
      if (sl == 0) SKG_PH(10);
      if (!RES_UP_FRONT) load_res(sl);
      if (m0 + sl * SROWS + er < p.M) {
        const float* const srow = stg + er * OPF + ec;
        half_t* crow = crow0 + (size_t)sl * SROWS * p.ldc;
        size_t lo_row = (size_t)(m0 + er + sl * SROWS);
        if constexpr (HILO) {
          if (p.up2) {      // polyphase upsample: low-res pixel (i, j) of image b -> high-res pixel (2 i + a, 2 j + b)
            const int m = m0 + sl * SROWS + er, hw = p.OH * p.OW;
            const int img = m / hw, rr = m - img * hw, i = rr / p.OW, j = rr - i * p.OW;
            lo_row = (size_t)img * 4 * hw + (size_t)(2 * i + (ph >> 1)) * (2 * p.OW) + 2 * j + (ph & 1);
            crow = reinterpret_cast<half_t*>(p.C) + lo_row * p.ldc + n0 + ec;
          }
        }
        float4_t v0[ITER], v1[ITER];
#pragma unroll
        for (int k = 0; k < ITER; ++k) {
          v0[k] = *reinterpret_cast<const float4_t*>(srow + k * TPR * 8);
          v1[k] = *reinterpret_cast<const float4_t*>(srow + k * TPR * 8 + 4);
        }
        {
#pragma unroll
          for (int k = 0; k < ITER; ++k) {
            if (n0 + ec + k * TPR * 8 >= p.N) continue;
            float v[8] = {v0[k][0], v0[k][1], v0[k][2], v0[k][3], v1[k][0], v1[k][1], v1[k][2], v1[k][3]};
            half8_t o;
            if constexpr (BROWS) {      // this thread's row reads its sample's bias row
              const half_t* const brow = p.bias + (size_t)((m0 + sl * SROWS + er) / p.gn_hw) * p.bias_pitch + n0 + ec + k * TPR * 8;
              const half4_t b0 = ld_half4(brow), b1 = ld_half4(brow + 4);
              const float bb[8] = {(float)b0[0], (float)b0[1], (float)b0[2], (float)b0[3], (float)b1[0], (float)b1[1], (float)b1[2], (float)b1[3]};
              if (HILO || p.res) {      // as this epilogue without the flag: (acc + b) * alpha + residual
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = (v[e] + bb[e]) * p.alpha + (float)rv[sl][k][e];
              } else {                  // as the fp16-staged epilogue a launch without residual takes without the flag: acc * alpha + (b * alpha)
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                  const float ba = bb[e] * p.alpha;
                  v[e] = __builtin_fmaf(v[e], p.alpha, ba);
                }
              }
            } else {
#pragma unroll
              for (int e = 0; e < 8; ++e) v[e] = v[e] * p.alpha + (float)rv[sl][k][e];
            }
            if constexpr (HILO) {
              if (p.res_lo) {
                const half8_t rl = ld_half8(p.res_lo + (size_t)(m0 + er + sl * SROWS) * p.ldr + n0 + ec + k * TPR * 8);
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] += (float)rl[e];
              }
            }
            if (relu) {
              asm volatile("" ::: "memory");       // a real (wave-uniform) branch instead of 8 selects per piece
#pragma unroll
              for (int e = 0; e < 8; ++e) v[e] = fmaxf(v[e], 0.f);
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (half_t)v[e];
            if constexpr (ITER == GNP) {
              if (gn) gn_acc(k, o);
            }
            if constexpr (HILO) {
              if (p.c_lo) {
                half8_t lo;
#pragma unroll
                for (int e = 0; e < 8; ++e) lo[e] = (half_t)(v[e] - (float)o[e]);
                st_half8(p.c_lo + lo_row * p.ldc + n0 + ec + k * TPR * 8, lo);
              }
            }
            half8_t* dst8 = reinterpret_cast<half8_t*>(crow + k * TPR * 8);
#ifdef SKG_PHASES
            if (p.flags & 0x4000u) { if (o[0] == (half_t)12345.f) *dst8 = o; continue; }   // probe: epilogue without stores
#endif
            // (inline asm: hipcc merges an if/else pair of builtin stores into ONE plain store and drops the hint.
            //  The s_nop behind every asm store is the gfx9 "VMEM store of more than 8 bytes, then a VALU write of its
            //  data registers" wait states (two on gfx940+): hipcc's hazard recognizer does not look inside an asm block, and it is free
            //  to reuse the registers in the very next instruction - seen with the GEGLU pre-activation store, whose
            //  first 8 bytes came out as the next store's address.)
            if (stream_out) asm volatile("global_store_dwordx4 %0, %1, off nt\n\ts_nop 1" ::"v"(dst8), "v"(o) : "memory");
            else *dst8 = o;
          }
        }
      }
    }
    if (gn) gn_fold();
    SKG_PH(4);
    continue;
  }
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int m = m0 + wm * WM + i * 16 + l16;
    if (m >= p.M) continue;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int n = n0 + wn * WN + j * 16 + g * 4;
      if (n >= p.N) continue;
      float4_t v = acc[i][j];
      if (p.bias) {      // (BROWS: the row's own bias row; the plain instantiations never get here with a bias row per sample - launch_cfg)
        const half4_t b = ld_half4(p.bias + (BROWS ? (size_t)(m / p.gn_hw) * p.bias_pitch : 0) + n);
        v[0] += (float)b[0]; v[1] += (float)b[1]; v[2] += (float)b[2]; v[3] += (float)b[3];
      }
      v *= p.alpha;
      if (p.res) {
        const half4_t r = ld_half4(p.res + (size_t)m * p.ldr + n);
        v[0] += (float)r[0]; v[1] += (float)r[1]; v[2] += (float)r[2]; v[3] += (float)r[3];
      }
      if (relu) {
        v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f);
      }
      if (f32out) {
        *reinterpret_cast<float4_t*>(reinterpret_cast<float*>(p.C) + (size_t)m * p.ldc + n) = v;
      } else {
        half4_t o = {(half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3]};
        st_half4(reinterpret_cast<half_t*>(p.C) + (size_t)m * p.ldc + n, o);
      }
    }
  }
  }   // persistent tile loop
}

template <int BM, int BN, int WGM, int WGN, int MODE, int NS = 2, bool GNS = false, bool HILO = false, bool BROWS = false>
__global__ __launch_bounds__(WGM * WGN * 64, (NS * (BM + BN) * BK * 2 + 8 * BN <= 80 * 1024) ? 2 : 1) void gemm2_kernel(const GemmParams p, int tiles_n, int nwg,
                                                                  unsigned a_bytes, unsigned b_bytes,
                                                                  unsigned a_shift, int kt_per_split,
                                                                  float* __restrict__ ws) {
  gemm2_body<BM, BN, WGM, WGN, MODE, NS, GNS, HILO, BROWS>(p, tiles_n, nwg, a_bytes, b_bytes, a_shift, kt_per_split, ws);
}

// out = epi(sum_s slab[s]) for a split-K launch; 4 outputs per thread
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const GemmParams p, const float* __restrict__ ws,
                                                            int splits) {
  const int N4 = p.N >> 2;
  const size_t total = (size_t)p.M * N4;
  const size_t slab = (size_t)p.M * p.N;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t m = i / N4;
    const int n = (int)(i - m * N4) * 4;
    float4_t v = *reinterpret_cast<const float4_t*>(ws + m * p.N + n);
    for (int s = 1; s < splits; ++s) v += *reinterpret_cast<const float4_t*>(ws + s * slab + m * p.N + n);
    splitk_epilogue(p, v, m, n);
  }
}


// Tuning values of the split-K policy (SKG_SPLIT_TARGET, SKG_MAX_SPLITS, SKG_SPLIT_NS), ONE helper for launch_cfg, pick_splits and
// skg_gemm2_tile_n: validated, read once per process.
struct SplitTuning { int target, smax, ns; };
inline SplitTuning read_split_tuning() {
  auto geti = [](const char* n, int dflt) { const char* e = getenv(n); return e ? atoi(e) : dflt; };
  SplitTuning t{geti("SKG_SPLIT_TARGET", 512), geti("SKG_MAX_SPLITS", 8), geti("SKG_SPLIT_NS", 3 /* SPLIT_NS_DEFAULT */)};
  t.target = t.target < 1 ? 1 : t.target > 4096 ? 4096 : t.target;      // workgroups a split launch aims at
  t.smax = t.smax < 1 ? 1 : t.smax > 64 ? 64 : t.smax;                   // cap of the split factor
  t.ns = t.ns <= 2 ? 2 : t.ns >= 4 ? 4 : 3;                              // LDS stages of a split launch with <= 256 workgroups
  return t;
}
inline SplitTuning split_tuning() {
  static const SplitTuning t = read_split_tuning();
  return t;
}

// number of K splits for a launch of `nwg` 128-row tiles over KT K-tiles (1 = no split)
inline int pick_splits(long nwg, int KT, size_t slab_bytes, const float* ws, size_t ws_bytes) {
  // nwg == 256 is ONE workgroup per CU: nothing overlaps its DMA waits.  Two K halves per CU (16x16-level convs,
  // K >= 8192: 720 -> 990 TFLOP/s) beat the three-stage single workgroup (870) there; below that the fp32 slabs +
  // reduce pass cost more than they hide and the launch takes the three-stage kernel instead
  if (!ws || nwg > 256 || KT < (nwg == 256 ? 128 : 16)) return 1;
  const SplitTuning tune = split_tuning();
  int s = (int)((tune.target + nwg - 1) / nwg);
  if (s > tune.smax) s = tune.smax;
  while (s > 1 && KT / s < 8) --s;
  while (s > 1 && (size_t)s * slab_bytes > ws_bytes) --s;
  return s;
}

// bytes of the A / B operands reachable through their descriptors (must stay below 2^31 for the OOB trick)
inline bool operand_bytes(const GemmParams& p, int mode, unsigned long long& a, unsigned long long& b,
                          unsigned long long& shift) {
  b = ((unsigned long long)((p.up2 == 5 ? 4 : 1) * p.N - 1) * p.ldb + p.K) * 2ull;
  if (mode == MODE_DIRECT) {
    shift = 0;
    a = ((unsigned long long)(p.M - 1) * p.lda + p.K) * 2ull;
  } else {
    const unsigned long long rows = (unsigned long long)p.M / ((unsigned long long)p.OH * p.OW);
    shift = (unsigned long long)(p.IW + 1) * p.lda * 2ull;
    a = rows * p.IH * p.IW * p.lda * 2ull + shift + (unsigned long long)(2 * p.IW + 2) * p.lda * 2ull;
  }
  return a < 0x7fffffffull && b < 0x7fffffffull;
}

inline bool eligible(const GemmParams& p, int mode) {
  if (p.K % BK != 0 || p.M < 1) return false;
  if (mode != MODE_DIRECT && p.Cin % BK != 0) return false;
  unsigned long long a, b, s;
  return operand_bytes(p, mode, a, b, s);
}

struct TileCfg { int bm, bn; };

// 256 x 320 (8 waves) when it still puts a workgroup on (almost) every CU; else the widest 128-row tile that
// divides N and gives >= ~0.8 workgroups per CU; else 128 x 64 (with split-K if a workspace is set)
inline TileCfg pick_tile(int M, int N, int K) {
  static const char* force = getenv("SKG_FORCE_BN");          // tuning / ablation only
  if (force) {
    const int bn = atoi(force);
    if (bn == 320 && N % 320 == 0) return {256, 320};
    if ((bn == 160 || bn == 128 || bn == 64) && (N % bn == 0 || bn == 64)) return {128, bn};
  }
  // with the pinned issue order the 4-wave 128 x 160 tile matches or beats the 8-wave tile on every N = 320 layer
  // (conv 320->320 @ 64x64: 122 vs 139 us); the wide tile still wins (+7 %) when there are many column tiles of a
  // long K loop to share each activation panel (FF1 of the 16x16 level: N = 10240, K = 1280)
  if (K >= 1024 && N >= 2560 && N % 320 == 0 && (long)skg_cdiv(M, 256) * (N / 320) >= 240) return {256, 320};
  const long tm = skg_cdiv(M, 128);
  if (N % 160 == 0 && tm * (N / 160) >= 200) return {128, 160};
  // few row tiles but a long K loop (the 8x8-resolution convolutions): the wide tile + split-K moves 40 % fewer
  // operand bytes per flop than 128 x 64 + split-K (conv 2560->1280 @ 8x8: 68 vs 86 us)
  if (N % 160 == 0 && K >= 2048 && tm * (N / 160) >= 24) return {128, 160};
  if (N % 128 == 0 && tm * (N / 128) >= 200) return {128, 128};
  return {128, 64};
}

// Grid size.  The kernel body is a tile loop (vb += gridDim.x), so any grid <= nwg is valid; measured on MI355X
// a one-resident-wave persistent grid (512 / 256 workgroups) is 5-30 % SLOWER than one workgroup per tile
// (dispatch of the next workgroup overlaps the tail of the previous one better than the in-kernel loop does
// with a 2-stage pipeline), so the launch uses nwg.  SKG_PERSISTENT=1 switches for experiments.
inline int persistent_grid(int nwg, int nthr) {
  static const bool on = getenv("SKG_PERSISTENT") != nullptr;
  if (!on) return nwg;
  const int resident = (nthr > 256 ? 1 : 2) * 256;
  return nwg < resident ? nwg : resident;
}

constexpr size_t STREAM_OUT_BYTES = (size_t)32 << 20;      // the aggregate L2 (8 x 4 MB)
static_assert(true, "");                                 // (SPLIT_NS default = 3: read_split_tuning, LDS stages of a split-K launch with <= 256 workgroups)

// GroupNorm statistics in the epilogue: the plain 128 x 160 instantiations (two or three stages, no split-K) with the
// staged epilogue, whole tiles, 128-row chunks that stay inside one sample and groups that stay inside one tile
inline bool gn_fusable(const GemmParams& p, int mode) {
  if (!p.gn_partial || p.gn_groups <= 0 || p.gn_hw <= 0 || !eligible(p, mode)) return false;
  if (p.flags & (SKG_EPI_OUT_F32 | SKG_EPI_GEGLU)) return false;
  const bool hilo = p.c_lo || p.res_lo;      // accuracy mode: 128-row tiles only (launch_mode)
  TileCfg t = pick_tile(p.M, p.N, p.K);
  if (hilo && t.bm == 256) t = TileCfg{128, 160};
  if (t.bm != 128 || t.bn != 160) return false;
  if (p.M % 128 != 0 || p.N % 160 != 0 || p.gn_hw % 128 != 0 || p.M % p.gn_hw != 0 || p.N % p.gn_groups != 0) return false;
  const int cpg = p.N / p.gn_groups;
  if ((cpg & 1) || 160 % cpg != 0) return false;
  if (p.ldc % 8 != 0 || (reinterpret_cast<uintptr_t>(p.C) & 15) != 0) return false;
  if (p.res && (p.ldr % 8 != 0 || (reinterpret_cast<uintptr_t>(p.res) & 15) != 0)) return false;
  const long ntiles = (long)(p.M / 128) * (p.N / 160);
  return pick_splits(ntiles, p.K / BK, (size_t)p.M * p.N * 4, p.ws, p.ws_bytes) == 1;
}

template <int BM, int BN, int WGM, int WGN, int MODE>
void launch_cfg(const GemmParams& p_in, hipStream_t st) {
  GemmParams p = p_in;
  const size_t out_bytes = (size_t)p.M * ((p.flags & SKG_EPI_GEGLU) ? p.N / 2 : p.N) * ((p.flags & SKG_EPI_OUT_F32) ? 4 : 2);
  static const bool tap_major = getenv("SKG_TAP_MAJOR") != nullptr;        // A/B switch for the K order (tools/gemm_bench.py)
  if (MODE != MODE_DIRECT && !tap_major) p.flags |= 0x1000u;
  static const char* smb = getenv("SKG_STREAM_MB");          // tuning only
  if (out_bytes >= (smb ? (size_t)atoi(smb) << 20 : STREAM_OUT_BYTES)) p.flags |= 0x800u;
  const int tiles_n = skg_cdiv(p.N, BN);
  const int ntiles = skg_cdiv(p.M, BM) * tiles_n * (p.up2 == 5 ? 4 : 1);      // (5: the four polyphase launches in one grid)
  unsigned long long a, b, s;
  operand_bytes(p, MODE, a, b, s);
  const int KT = p.K / BK;
  // (the split-K reduce kernel has the plain epilogue only: fused-GEGLU launches never split)
  int splits = (BM == 128 && !(p.flags & SKG_EPI_GEGLU) && !p.up2 && !p.seg_rows) ? pick_splits(ntiles, KT, (size_t)p.M * p.N * 4, p.ws, p.ws_bytes) : 1;
  if (p.wino) splits = p.wino;      // Winograd GEMM step: one K slice per transform component (skg_gemm2_try_launch checked the preconditions)
  constexpr int NTHR = WGM * WGN * 64;
  if (BM == 128 && BN == 160 && splits == 1 && gn_fusable(p, MODE)) p.flags |= SKG_FLAG_GN_STATS;
  // a bias row per sample: the plain instantiations place the tile's sample once per workgroup in front of their staged epilogues;
  // tiles that can span samples (or a launch that would take the direct stores: fp32 output, an unaligned output or residual) run the BROWS instantiations (launch_mode: BM = 128)
  if (p.bias_pitch && (p.gn_hw % BM != 0 || (p.flags & SKG_EPI_OUT_F32) || p.ldc % 8 != 0 || !skg_aligned(p.C, 16) || (p.res && (p.ldr % 8 != 0 || !skg_aligned(p.res, 16)))))
    p.flags |= SKG_FLAG_BIAS_PER_ROW;
  // XCDs per K slice: all 8 without split-K; 8 / ns when the slices line up with XCD boundaries
  const int ns_eff = splits > 1 ? skg_cdiv(KT, skg_cdiv(KT, splits)) : 1;
  const int G = (8 % ns_eff == 0) ? 8 / ns_eff : 0;
  if (G >= 2 && ntiles % G == 0 && p.up2 != 5) {
    static const bool off = getenv("SKG_NO_XGRID") != nullptr;        // A/B switch (tools/gemm_bench.py)
    const int tiles_m = ntiles / tiles_n;
    const double a_mb = (double)p.M * (MODE == MODE_DIRECT ? p.K : p.Cin) * 2.0, w_mb = (double)p.N * p.K * 2.0;
    int best = 1;
    double cost = a_mb + G * w_mb;
    for (int gn = 2; gn <= G; gn *= 2) {
      if (tiles_n % gn != 0 || tiles_m % (G / gn) != 0) continue;
      const double c = gn * a_mb + (G / gn) * w_mb;
      if (c < 0.9 * cost) { cost = c; best = gn; }
    }
    static const char* force_gn = getenv("SKG_XGRID_GN");      // tuning (tools/gemm_fetch.sh): force the column blocks of the XCD arrangement
    if (force_gn) {
      const int gn = atoi(force_gn);
      best = (gn >= 1 && gn <= G && G % gn == 0 && tiles_n % gn == 0 && tiles_m % (G / gn) == 0) ? gn : 1;
    }
    if (!off && best > 1) p.flags |= ((unsigned)best << 20) | ((unsigned)(G == 8 ? 0 : G) << 24);
  }
  if (splits > 1) {
    const int per = skg_cdiv(KT, splits);
    const int ns = skg_cdiv(KT, per);            // every split non-empty
    // at most one workgroup per CU anyway: a deeper LDS ring (three / four stages, 110 / 147 KB) keeps two / three operand tiles of
    // its K slice in flight where the two-stage kernel waits out one DMA latency per step (SKG_SPLIT_NS: tuning)
    bool deep = false;
    if constexpr (BM == 128 && BN == 160 && (MODE == MODE_DIRECT || MODE == MODE_S1)) {
      const int sns = split_tuning().ns;
      if (ntiles * ns <= 256 && per >= 4 && sns >= 3) {
        deep = true;
        if (sns >= 4)
          hipLaunchKernelGGL((gemm2_kernel<BM, BN, WGM, WGN, MODE, 4, false, false>), dim3(ntiles * ns), dim3(NTHR), 0, st, p, tiles_n, ntiles * ns,
                             (unsigned)a, (unsigned)b, (unsigned)s, per, p.ws);
        else
          hipLaunchKernelGGL((gemm2_kernel<BM, BN, WGM, WGN, MODE, 3, false, false>), dim3(ntiles * ns), dim3(NTHR), 0, st, p, tiles_n, ntiles * ns,
                             (unsigned)a, (unsigned)b, (unsigned)s, per, p.ws);
      }
    }
    if (!deep)
      hipLaunchKernelGGL((gemm2_kernel<BM, BN, WGM, WGN, MODE>), dim3(persistent_grid(ntiles * ns, NTHR)), dim3(NTHR),
                         0, st, p, tiles_n, ntiles * ns, (unsigned)a, (unsigned)b, (unsigned)s, per, p.ws);
    if (p.wino) return;      // (the slabs are transform components, not partial sums: the caller's output transform follows)
    size_t blocks = ((size_t)p.M * (p.N / 4) + 255) / 256;
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)(blocks > 2048 ? 2048 : blocks)), dim3(256), 0, st, p,
                       (const float*)p.ws, ns);
    return;
  }
  // accuracy mode (p.c_lo / p.res_lo): the same decision tree on the instantiations with the hi / lo epilogue (split-K launches
  // above: the slabs are raw accumulators, the pair epilogue is splitk_reduce_kernel's)
  const bool hilo = p.c_lo || p.res_lo;
  constexpr bool HILO_OK = BM == 128 && (MODE == MODE_DIRECT || MODE == MODE_S1 || MODE == MODE_S2 || MODE == MODE_UP2);
  const bool gns = (p.flags & SKG_FLAG_GN_STATS) != 0;
  if constexpr (BM == 128 && MODE != MODE_DIRECT) {      // (two stages, no statistics: gn_fusable wants whole 128-row chunks per sample)
    if (p.flags & SKG_FLAG_BIAS_PER_ROW) {
      if constexpr (HILO_OK) {
        if (hilo) {
          hipLaunchKernelGGL((gemm2_kernel<BM, BN, WGM, WGN, MODE, 2, false, true, true>), dim3(ntiles), dim3(NTHR), 0, st, p, tiles_n, ntiles,
                             (unsigned)a, (unsigned)b, (unsigned)s, KT, (float*)nullptr);
          return;
        }
      }
      hipLaunchKernelGGL((gemm2_kernel<BM, BN, WGM, WGN, MODE, 2, false, false, true>), dim3(ntiles), dim3(NTHR), 0, st, p, tiles_n, ntiles,
                         (unsigned)a, (unsigned)b, (unsigned)s, KT, (float*)nullptr);
      return;
    }
  }
#define G2_LAUNCH(NS_, GNS_, HILO_)                                                                                            \
  hipLaunchKernelGGL((gemm2_kernel<BM, BN, WGM, WGN, MODE, NS_, GNS_, HILO_>), dim3(ntiles), dim3(NTHR), 0, st, p, tiles_n, ntiles, \
                     (unsigned)a, (unsigned)b, (unsigned)s, KT, (float*)nullptr)
  // three stages: the 128 x 160 tile when the launch has at most one workgroup per CU anyway (110 KB of LDS), the
  // 128 x 64 tile always (74 KB: two workgroups per CU still fit)
  if constexpr (BM == 128 && (BN == 160 || BN == 64) && (MODE == MODE_DIRECT || MODE == MODE_S1)) {
    static const bool off = getenv("SKG_NO_NS3") != nullptr;        // A/B switch (tools/gemm_bench.py)
    if (!off && KT >= 4 && (BN == 64 || ntiles <= 256)) {
      if constexpr (BN == 160) {
        if (gns) {
          if (hilo) G2_LAUNCH(3, true, true); else G2_LAUNCH(3, true, false);
          return;
        }
      }
      if (hilo) G2_LAUNCH(3, false, true); else G2_LAUNCH(3, false, false);
      return;
    }
  }
#ifdef SKG_PHASES
  static const char* solo = getenv("SKG_SOLO");      // probe: pad the LDS request so that ONE workgroup fits per CU
  if (solo) {
    hipLaunchKernelGGL((gemm2_kernel<BM, BN, WGM, WGN, MODE>), dim3(ntiles), dim3(NTHR), 48 * 1024, st,
                       p, tiles_n, ntiles, (unsigned)a, (unsigned)b, (unsigned)s, KT, (float*)nullptr);
    return;
  }
#endif
  if constexpr (HILO_OK) {
    if (hilo) {
      if constexpr (BN == 160 && MODE != MODE_UP2) {
        if (gns) { G2_LAUNCH(2, true, true); return; }
      }
      G2_LAUNCH(2, false, true);
      return;
    }
  }
  if constexpr (BM == 128 && BN == 160) {
    if (gns) { G2_LAUNCH(2, true, false); return; }
  }
#undef G2_LAUNCH
  hipLaunchKernelGGL((gemm2_kernel<BM, BN, WGM, WGN, MODE>), dim3(persistent_grid(ntiles, NTHR)), dim3(NTHR), 0, st,
                     p, tiles_n, ntiles, (unsigned)a, (unsigned)b, (unsigned)s, KT, (float*)nullptr);
}

template <int MODE>
void launch_mode(const GemmParams& p, hipStream_t st) {
  TileCfg t = pick_tile(p.M, p.N, p.K);
  if (t.bm == 256 && (p.c_lo || p.res_lo || p.up2 || p.seg_rows || p.bias_pitch)) t = TileCfg{128, 160};      // (hi / lo epilogue, polyphase row map, a bias row per sample: 128-row tiles)
  if (p.wino) t = p.N % 160 == 0 ? TileCfg{128, 160} : p.N % 128 == 0 ? TileCfg{128, 128} : TileCfg{128, 64};      // 16 slices of 128-row tiles
  if (t.bm == 256) launch_cfg<256, 320, 2, 4, MODE>(p, st);
  else if (t.bn == 160) {
    launch_cfg<128, 160, 2, 2, MODE>(p, st);
  }
  else if (t.bn == 128) launch_cfg<128, 128, 2, 2, MODE>(p, st);
  else launch_cfg<128, 64, 2, 2, MODE>(p, st);
}

}  // namespace

// tile width of the instantiation a plain (no fused GEGLU) launch of this shape runs, + 10000 when it is the
// three-stage one (bench.py / tools spell the rocprofv3 kernel name from this)
int skg_gemm2_tile_n(int M, int N, int K, int Cin, int mode, size_t ws_bytes) {
  if (K % BK != 0 || M < 1 || (mode != MODE_DIRECT && Cin % BK != 0)) return 0;
  const TileCfg t = pick_tile(M, N, K);
  const int KT = K / BK;
  const long ntiles = (long)skg_cdiv(M, t.bm) * skg_cdiv(N, t.bn);
  const int splits = t.bm == 128 ? pick_splits(ntiles, KT, (size_t)M * N * 4, ws_bytes ? (const float*)1 : nullptr, ws_bytes) : 1;
  bool three = t.bm == 128 && (t.bn == 160 || t.bn == 64) && (mode == MODE_DIRECT || mode == MODE_S1) &&
               !getenv("SKG_NO_NS3") && KT >= 4 && (t.bn == 64 || ntiles <= 256) && splits == 1;
  if (splits > 1 && t.bm == 128 && t.bn == 160 && (mode == MODE_DIRECT || mode == MODE_S1)) {      // split launch on the deep ring (launch_cfg)
    const int per = skg_cdiv(KT, splits), ns = skg_cdiv(KT, per);
    three = ntiles * ns <= 256 && per >= 4 && split_tuning().ns >= 3;      // (a tuning value of 4 is reported as three stages too)
  }
  return t.bn + (three ? 10000 : 0);
}

bool skg_gemm2_fuses_gn(const GemmParams& p, int mode) { return gn_fusable(p, mode); }

void skg_splitk_reduce_launch(const GemmParams& p, const float* ws, int splits, hipStream_t st) {
  size_t blocks = ((size_t)p.M * (p.N / 4) + 255) / 256;
  hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)(blocks > 2048 ? 2048 : blocks)), dim3(256), 0, st, p, ws, splits);
}

bool skg_gemm2_try_launch(const GemmParams& p, int mode, hipStream_t st) {
  if (!eligible(p, mode)) return false;
  if (p.wino &&      // Winograd GEMM step: whole K tiles per component, its slabs fit the stream's workspace, plain launch otherwise
      (mode != MODE_DIRECT || p.wino != 16 || (p.K / BK) % 16 != 0 || !p.ws || (size_t)16 * p.M * p.N * 4 > p.ws_bytes || p.gn_partial ||
       p.seg_rows || p.up2 || p.aux || (p.flags & (SKG_EPI_GEGLU | SKG_EPI_OUT_F32))))
    return false;
  if (p.seg_rows &&               // segmented output rows: the plain fp16-staged epilogue, no split-K slabs
      (mode != MODE_DIRECT || p.res || p.gn_partial || p.c_lo || p.res_lo || p.aux || (p.flags & (SKG_EPI_GEGLU | SKG_EPI_OUT_F32)) ||
       p.ldc % 8 != 0 || (reinterpret_cast<uintptr_t>(p.C) & 15) != 0))
    return false;
  if ((p.ntaps || p.up2) &&      // polyphase: stride-1 walk (4 x 4 window: stride 2), the plain fp16-staged epilogue (no residual / statistics) or the pair one
      ((p.ntaps == 16 ? (mode != MODE_S2 || p.up2 || p.c_lo) : mode != MODE_S1) || p.res || p.gn_partial || p.res_lo || (p.flags & (SKG_EPI_GEGLU | SKG_EPI_OUT_F32)) ||
       p.ldc % 8 != 0 || (reinterpret_cast<uintptr_t>(p.C) & 15) != 0 || p.M % (p.OH * p.OW) != 0))
    return false;
  if ((p.c_lo || p.res_lo) &&
      ((p.flags & (SKG_EPI_GEGLU | SKG_EPI_OUT_F32)) || p.aux || p.ldc % 8 != 0 ||
       (mode != MODE_DIRECT && mode != MODE_S1 && mode != MODE_S2 && mode != MODE_UP2) || (mode == MODE_UP2 && p.gn_partial) ||
       (reinterpret_cast<uintptr_t>(p.C) & 15) != 0 || (p.c_lo && (reinterpret_cast<uintptr_t>(p.c_lo) & 15) != 0) ||
       ((p.res || p.res_lo) && p.ldr % 8 != 0) || (p.res && (reinterpret_cast<uintptr_t>(p.res) & 15) != 0) ||
       (p.res_lo && (reinterpret_cast<uintptr_t>(p.res_lo) & 15) != 0)))
    return false;
  if ((p.flags & SKG_EPI_GEGLU) && ((p.flags & SKG_EPI_OUT_F32) || p.res || p.ldc % 8 != 0 ||
                                     (reinterpret_cast<uintptr_t>(p.C) & 15) != 0))
    return false;
  switch (mode) {
    case MODE_DIRECT: launch_mode<MODE_DIRECT>(p, st); break;
    case MODE_S1: launch_mode<MODE_S1>(p, st); break;
    case MODE_S2: launch_mode<MODE_S2>(p, st); break;
    case MODE_UP2: launch_mode<MODE_UP2>(p, st); break;
    case MODE_S2T: launch_mode<MODE_S2T>(p, st); break;
    case MODE_S2A: launch_mode<MODE_S2A>(p, st); break;
    default: return false;
  }
  return true;
}

#ifdef SKG_PHASES
extern "C" int skg_debug_phases(void* host_out, int nblocks) {      // not part of the ABI: profiling builds only
  return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_phase), (size_t)nblocks * 16 * sizeof(unsigned long long));
}
#endif
