/* skg.h - C ABI of libskg.so: MI355X (gfx950) kernels for the sketch-guided diffusion
 * sampler hot path (Mikubill/sketch2img).
 *
 * The reference is 100 % Python and has no FFI of its own; every "kernel" on its hot path is
 * reached through third-party Python packages (diffusers -> torch/cuDNN/cuBLAS, xformers).  Each
 * entry point below therefore cites the reference CALL SITE (file:line under the reference
 * repo root) whose third-party kernels it replaces.  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - all pointers are DEVICE pointers unless noted; the caller owns every buffer (the library
 *     never allocates or frees), `stream` is a hipStream_t passed as void* (0 = null stream);
 *   - activations are fp16, token-major / NHWC: a tensor of `rows` images of H x W pixels and C
 *     channels is the row-major matrix [rows*H*W][C] with an explicit leading dimension (in
 *     elements) where a slice of a wider buffer may be passed;
 *   - weights are fp16 [N][K] row-major ("out x in", K contiguous), see each function;
 *   - return value: 0 = launched, negative = SKG_E_* (nothing launched).  No exceptions.
 */
#ifndef SKG_H_
#define SKG_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SKG_OK 0
#define SKG_E_BADARG (-1)    /* shape/alignment precondition violated */
#define SKG_E_UNSUPPORTED (-2)
#define SKG_E_LAUNCH (-3)    /* hipGetLastError() != hipSuccess after the launch */

#define SKG_ABI_VERSION 6
int skg_abi_version(void);
/* Human-readable text of the last SKG_E_LAUNCH on this thread ("" if none). */
const char* skg_last_error(void);

/* ---- epilogue flags shared by skg_gemm_f16 / skg_conv3x3_f16 ---------------------------------- */
#define SKG_EPI_RELU 1u      /* max(.,0) applied last */
#define SKG_EPI_OUT_F32 2u   /* C is float* instead of fp16 */
#define SKG_EPI_GEGLU 4u     /* skg_gemm_f16 only: B / bias rows are the interleaved FF1 pack (groups of four output
                              * columns [a a g g]); C is [M][N/2] = a * gelu(g).  No residual, fp16 out, K % 64 == 0
                              * (else SKG_E_UNSUPPORTED).  Fuses diffusers GEGLU into ff.net.0.proj. */
#define SKG_EPI_BIAS_ROWS 8u /* skg_conv3x3_f16 (every mode) / skg_conv3x3_wino_f16 only: bias is fp16 [rows][Cout] (pitch Cout), one row
                              * per SAMPLE - output row m reads bias[m / (OH * OW)][n].  Needs bias != NULL (else SKG_E_BADARG;
                              * skg_gemm_f16: SKG_E_BADARG).  The time-embedding projection of a ResnetBlock folded into conv1.bias
                              * when every sample of the batch has its own timestep (the trainers' unet(noisy_latents, timesteps,
                              * ehs) at modules/pipeline.py:96 with a [B] timestep tensor). */

/* C[m][n] = epi( alpha * (sum_k A[m][k] * B[n][k] + bias[n]) + residual[m][n] )
 * (convolutions with SKG_EPI_BIAS_ROWS: bias[m / (OH * OW)][n] in place of bias[n])
 * A fp16 [M][K] (lda), B fp16 [N][K] (ldb), C fp16|fp32 [M][N] (ldc), bias fp16 [N] or NULL,
 * residual fp16 [M][N] (ldr) or NULL.  Requires K % 32 == 0, N % 8 == 0, lda/ldb % 8 == 0,
 * ldc/ldr % 4 == 0, 16-byte aligned A/B, 8-byte aligned C/residual/bias.
 * Replaces: every nn.Linear / 1x1 Conv2d the UNet evaluates at modules/pipeline.py:96
 * (diffusers proj_in/proj_out, to_q/k/v, to_out, ff.net, conv_shortcut -> cuBLAS/cuDNN), their
 * backward-to-input GEMMs triggered at modules/pipeline.py:159, the LGP's Linear layers at
 * modules/latent_predictor.py:45 and Conv1d(k=1) at modules/clip_guided_attn.py:124.
 * C_lo / residual_lo (either may be NULL): the lo half of an output / residual PAIR - the accuracy mode below.
 * gn_partial != NULL: the launch also leaves the GroupNorm partial sums of its output behind (HW = rows of C per sample,
 * `groups` groups over the N columns) - "GroupNorm whose statistics pass is done by the PRODUCER" below; else HW = groups = 0. */
int skg_gemm_f16(const void* A, int lda, const void* B, int ldb, void* C, void* C_lo, int ldc, int M, int N, int K,
                 const void* bias, const void* residual, const void* residual_lo, int ldr, float alpha, unsigned flags,
                 float* gn_partial, int HW, int groups, void* stream);

/* Optional split-K workspace for skg_gemm_f16 / skg_conv3x3_f16 launches on `stream` of the CURRENT device: a caller-owned
 * device buffer (>= 1 MiB, 16-byte aligned, fp32 partial slabs) that must stay valid until replaced.  With it, launches that
 * would put fewer than one workgroup on every CU (the 8x8 / 16x16-resolution layers) split their K loop over several
 * workgroups per tile and a second tiny kernel sums the slabs and applies the epilogue.  One slab per stream: launches on
 * one stream are ordered and share theirs, launches on different streams never do (the registry is mutex-protected and
 * the pointer reaches the kernel as an argument).  ws = NULL removes the stream's entry. */
int skg_set_workspace(void* ws, size_t bytes, void* stream);

/* Which kernel instantiation skg_gemm_f16 (mode 0, Cin ignored) / skg_conv3x3_f16 (mode = 1 + SKG_CONV_*)
 * run for this shape: 2000 + BN for the LDS-DMA kernel (gemm2_kernel<BN,MODE>), 1000 + BN for the generic one;
 * lets a profiler attribute a launch to the kernel instantiation that ran (bench.py roofline).  (A convolution with SKG_EPI_BIAS_ROWS
 * runs the same kernel family, with two exceptions this query does not see: the LDS-DMA kernel runs such a launch on its 128-row tiles
 * only - where it reports 2320 the launch runs 128 x 160 - and the 256 x 320 ping-pong tile (8320) is taken only when OH * OW % 256 == 0;
 * tiles that can span samples - OH * OW % 128 != 0 - and fp32 outputs take the two-stage per-row instantiations.) */
int skg_gemm_variant(int M, int N, int K, int Cin, int mode);

/* 3x3 convolution, padding 1, as implicit GEMM over NHWC fp16.
 *   mode SKG_CONV_S1      stride 1                         out (OH,OW) = in (IH,IW)
 *   mode SKG_CONV_S2      stride 2                         out = in / 2
 *   mode SKG_CONV_UP2     nearest 2x upsample then stride 1  out = 2 * in
 *   mode SKG_CONV_S2T     transpose of S2 (its dgrad)      out = 2 * in
 *   mode SKG_CONV_S2A     stride 2, padding (0,1,0,1): bottom/right only (the VAE encoder's Downsample2D)  out = in / 2
 * X fp16 [rows*IH*IW][Cin] (ldx), Wp fp16 [Cout][3][3][Cin] (tap-major, Cin contiguous),
 * Y [rows*OH*OW][Cout] (ldy).  IH, IW are the INPUT sizes.  Requires Cin % 32 == 0, Cout % 8 == 0.
 * bias / residual / alpha / flags, Y_lo / residual_lo and gn_partial / groups (HW = OH * OW) as skg_gemm_f16.  For a dgrad pass
 * Wp is the flipped, in/out-swapped pack (see sketch2img_amd/weights.py).
 * Replaces: ResnetBlock2D conv1/conv2, Downsample2D, Upsample2D, conv_in/conv_out (cuDNN) at
 * modules/pipeline.py:96 and their dgrad at modules/pipeline.py:159. */
#define SKG_CONV_S1 0
#define SKG_CONV_S2 1
#define SKG_CONV_UP2 2
#define SKG_CONV_S2T 3
#define SKG_CONV_S2A 4
int skg_conv3x3_f16(const void* X, int ldx, const void* Wp, void* Y, void* Y_lo, int ldy, int rows, int IH, int IW,
                    int Cin, int Cout, int mode, const void* bias, const void* residual, const void* residual_lo, int ldr,
                    float alpha, unsigned flags, float* gn_partial, int groups, void* stream);

/* ---- GroupNorm (+SiLU), NHWC fp16 -------------------------------------------------------------
 * stats: per (row, group) mean and rstd (float2 [rows][groups]) over HW x (C/groups) values.
 *   `partial` is scratch of skg_groupnorm_scratch_floats(rows, groups) floats.
 * apply: y = act((x-mean)*rstd*gamma+beta), act = SiLU if silu != 0.
 * bwd:   dx = GN'(SiLU'(dy)) + residual (residual may be NULL); needs x and the saved stats.
 * Replaces: torch group_norm + silu (ResnetBlock2D.norm1/2 + nonlinearity, Transformer2DModel.norm,
 * conv_norm_out) at modules/pipeline.py:96; backward at :159. */
size_t skg_groupnorm_scratch_floats(int rows, int groups);
int skg_groupnorm_stats(const void* X, int ldx, int rows, int HW, int C, int groups, float eps,
                        float* stats, float* partial, void* stream);
/* stats + apply in two launches (the apply kernel folds the chunk partials itself and publishes `stats` for a later
 * skg_groupnorm_bwd): what the UNet / VAE forward use.  X_lo != NULL (accuracy mode, below): GroupNorm of the pair X + X_lo (one
 * pitch; own statistics pass over the hi part; small maps: one launch on the pair's sum), and then Y_lo != NULL: the output is a
 * pair too (pitch ldy; conv_norm_out in front of conv_out, whose operand rounding would reach eps one to one). */
int skg_groupnorm_fwd(const void* X, const void* X_lo, int ldx, void* Y, void* Y_lo, int ldy, int rows, int HW, int C, int groups,
                      float eps, const void* gamma, const void* beta, int silu, float* stats, float* partial, void* stream);
/* GroupNorm whose statistics pass is done by the PRODUCER of X.  skg_gemm_f16 / skg_conv3x3_f16 with gn_partial != NULL
 * additionally leave, per (sample b, 128-row chunk c, group g), sum(y) and sum(y^2) of the fp16 outputs (the hi part of a pair)
 * in gn_partial[((b * (HW / 128) + c) * groups + g) * 2 + {0, 1}] (HW = rows of C per sample, a multiple of 128; fp16 output, no
 * fused GEGLU, 16-byte aligned C, ldc % 8 == 0).  The sums come out of the kernel's own epilogue when the tile that runs
 * can produce them (256 x 320 and 128 x 160 tiles, whole tiles, groups inside a tile - every 64 x 64 / 32 x 32-level
 * layer of the UNet), otherwise from the stand-alone statistics pass: the result is the same either way, in a fixed
 * summation order.  skg_groupnorm_from_partial folds `nch` chunks per (sample, group), publishes (mean, rstd) to `stats`
 * and applies - X is read once instead of twice.  Same replaced reference calls as skg_groupnorm_fwd. */
/* 1 when a gn_partial launch of this shape gets its partial sums from the kernel's own epilogue (mode as in
 * skg_gemm_variant: 0 = GEMM, 1 + SKG_CONV_*), 0 when the stand-alone statistics pass follows. */
int skg_gemm_gn_fused(int M, int N, int K, int Cin, int mode, int HW, int groups);
/* partialB != NULL: the same for a CONCATENATION X = [A (CA channels) | B (C - CA channels)] whose halves were written by two
 * producers (the skip connection of the UNet's up path and the layer in front of it): partialA / partialB hold groupsA / groupsB
 * groups per chunk over each half's own channels; the concatenation's group width must be a multiple of both source
 * widths and CA a multiple of it (320 + 320, 640 + 640 channels: two source groups per output group), otherwise
 * SKG_E_UNSUPPORTED (nothing launched: run skg_groupnorm_fwd).  Replaces: the GroupNorm on torch.cat([h, skip]) in
 * diffusers' CrossAttnUpBlock2D / UpBlock2D resnets (modules/pipeline.py:96).  partialB == NULL: one producer, CA and groupsB
 * unused (pass 0) and groupsA = groups.  X_lo / Y_lo as skg_groupnorm_fwd. */
int skg_groupnorm_from_partial(const void* X, const void* X_lo, int ldx, void* Y, void* Y_lo, int ldy, int rows, int HW, int C,
                               int CA, int groups, float eps, const void* gamma, const void* beta, int silu, float* stats,
                               const float* partialA, int groupsA, const float* partialB, int groupsB, int nch, void* stream);
/* C[(m / seg_rows) * seg_stride + m % seg_rows][n] = sum_k A[m][k] * B[n][k] + bias[n]: a GEMM over all batch rows whose output rows
 * land in per-batch-row slots of a longer buffer - clip_guided_attn concatenates [N image tokens ; 257 sketch tokens] per batch
 * row (modules/clip_guided_attn.py:111-119), so the image tokens' K / V of row b belong at rows [b L, b L + N) of the K / V
 * buffer; one launch instead of one per batch row.  M % seg_rows == 0, K % 64 == 0, C 16-byte aligned, ldc % 8 == 0. */
int skg_gemm_f16_rows(const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N, int K,
                      const void* bias, int seg_rows, int seg_stride, void* stream);
/* Nearest-neighbour 2x upsample followed by a 3x3 convolution (diffusers Upsample2D: the up path of the UNet at
 * modules/pipeline.py:96, the VAE decoder at :118), POLYPHASE: out (2i+a, 2j+b) = sum over the 2 x 2 low-resolution pixels the
 * nine taps land on, with the taps that land on one pixel pre-summed - four 4-tap stride-1 convolutions over the low-res
 * input, 16 tap-products per input pixel instead of 36 (skg_conv3x3_f16 with SKG_CONV_UP2 is the 9-tap form, same result up
 * to the fp16 rounding of the summed weights).  X [rows*IH*IW, Cin] (ldx), Y [rows*2IH*2IW, Cout] (ldy), Wpp: packed
 * [4 phases 2a+b][Cout][4 taps][Cin] (sketch2img_amd.unet.pack_conv_up2).  Cin % 64 == 0.
 * Accuracy mode.  Y_lo != NULL, pair_in == 0 (round 5, what the mode runs): the launch on the hi part of the stream (ldx >= Cin)
 * with the output written as the pair Y + Y_lo - drops the x_lo and W_lo correction thirds of the pair_in form (each ~1 % of the
 * mode's eps distance, together two thirds of its time).  pair_in != 0 (needs Y_lo): X is the pair buffer [x_hi | x_lo], 2 Cin
 * channels per pixel, with (hi, lo) pre-summed weights: per tap [x_hi | x_lo | x_hi] . [W_hi | W_hi | W_lo], Wpp = Wpp3
 * [4 phases][Cout][4 taps][3 Cin] (sketch2img_amd.unet.pack_conv_up2_hilo). */
int skg_conv3x3_up2_f16(const void* X, int ldx, const void* Wpp, void* Y, void* Y_lo, int ldy, int rows, int IH, int IW, int Cin,
                        int Cout, int pair_in, const void* bias, void* stream);
/* conv2 + conv_shortcut of a ResnetBlock whose channel count changes, as ONE implicit GEMM (round 5; diffusers ResnetBlock2D:
 * output = conv2(.) + conv_shortcut(x), under modules/pipeline.py:96): the 1x1 shortcut is a tenth "tap" without halo -
 *   Y[m][n] = sum_{tap, c} X[pixel(m) + tap][c] * Wcat[n][tap * Cin + c] + sum_{c2 < K2} X2[m][c2] * Wcat[n][9 * Cin + c2] + bias[n]
 * X [rows*IH*IW][ldx >= Cin] the 3x3 input (stride 1), X2 [rows*IH*IW][ldx2 >= K2] the block's input x, Wcat [Cout][9*Cin + K2]
 * (conv2's tap-major pack followed by the shortcut weight; bias = conv2.bias + conv_shortcut.bias).  Y_lo != NULL (accuracy mode):
 * pair output, and X2 / K2 are the pair buffer [x_hi | x_lo] / 2 * Cin_x against [W_sc | W_sc].  gn_partial != NULL: the GroupNorm
 * partial sums of the output as skg_conv3x3_f16 writes them.  Removes one GEMM launch, its M x Cout output write and the
 * residual read of conv2's epilogue per such block (14 per SD1.5 evaluation).  Cin % 64 == 0, K2 % 64 == 0.  Returns
 * SKG_E_UNSUPPORTED (nothing launched: run conv2 and the shortcut GEMM as two launches) when X2 spans 2 GiB or more. */
int skg_conv3x3_sc_f16(const void* X, int ldx, const void* X2, int ldx2, int K2, const void* Wcat, void* Y, void* Y_lo, int ldy,
                       int rows, int IH, int IW, int Cin, int Cout, const void* bias, unsigned flags, float* gn_partial, int groups,
                       void* stream);
/* 3x3 stride-1 convolution (padding 1) by Winograd F(2x2, 3x3) - the 16 x 16-level ResnetBlock convolutions of the UNet evaluated at
 * modules/pipeline.py:96 and their data gradients inside torch.autograd.grad at modules/pipeline.py:159 (diffusers ResnetBlock2D conv1 /
 * conv2 -> cuDNN).  2.25 x fewer MFMA flops and 4 x more workgroups than the implicit GEMM on maps that under-fill the chip:
 *   V = B^T d B per 4 x 4 input tile (stride 2)  ->  16 GEMMs V_c [Mt][Cin] . U_c^T, Mt = rows * IH/2 * IW/2 (ONE split launch of the
 *   GEMM kernel, fp32 slabs in the stream's workspace)  ->  Y = A^T M A + bias (+ residual) per 2 x 2 output tile.
 * X [rows*IH*IW][ldx >= Cin] fp16; U [Cout][16 * Cin] fp16 = G g G^T per (cout, cin), component c = 4 i + j at columns [c Cin, (c + 1) Cin)
 * (unet.pack_conv_wino); V: caller-owned scratch of skg_conv3x3_wino_v_bytes() bytes; Y [rows*IH*IW][ldy] (+ Y_lo: pair output);
 * flags: SKG_EPI_RELU and SKG_EPI_BIAS_ROWS only.  Needs IH, IW even, Cin % 64 == 0, Cout % 8 == 0 and a registered workspace of >= 64 * Mt * Cout bytes
 * (skg_set_workspace); otherwise SKG_E_UNSUPPORTED (nothing launched: run skg_conv3x3_f16).  U and V carry one more fp16 rounding than
 * the implicit GEMM's operands (tools/eps_winograd.py prices it: default-mode eps rel 1.07e-3 -> 1.09e-3).
 * X == NULL: V already holds the input transform (skg_groupnorm_wino_fwd wrote it). */
size_t skg_conv3x3_wino_v_bytes(int rows, int IH, int IW, int Cin);
int skg_conv3x3_wino_f16(const void* X, int ldx, const void* U, void* V, void* Y, void* Y_lo, int ldy, int rows, int IH, int IW,
                         int Cin, int Cout, const void* bias, const void* residual, const void* residual_lo, int ldr, unsigned flags,
                         void* stream);
/* GroupNorm(+SiLU) of a small map whose consumer is skg_conv3x3_wino_f16: statistics published to `stats` as skg_groupnorm_fwd does,
 * and instead of the normalised tensor its Winograd input transform V [rows*IH/2*IW/2][16*C] (the fp16-rounded activations transformed:
 * bit-identical to skg_groupnorm_fwd + the convolution's own input transform; one launch and one [M, C] round trip less).  One workgroup
 * per (row, group) holds the slice in registers / LDS: C / groups a multiple of 8, IH * IW * C / groups / 8 <= 2560, even maps - else
 * SKG_E_UNSUPPORTED (nothing launched).  Same replaced reference calls as skg_groupnorm_fwd (ResnetBlock2D.norm1 / norm2). */
int skg_groupnorm_wino_fwd(const void* X, int ldx, void* V, int rows, int IH, int IW, int C, int groups, float eps,
                           const void* gamma, const void* beta, int silu, float* stats, void* stream);
/* Data gradient of the polyphase upsample + convolution above (the autograd backward of diffusers Upsample2D inside
 * torch.autograd.grad at modules/pipeline.py:159): ONE 4 x 4 stride-2 convolution, padding 1, over the gradient at the upsampled
 * size.  X [rows*IH*IW, Cin] (ldx; IH, IW even), Y [rows*(IH/2)*(IW/2), Cout] (ldy), W16 [Cout][16 taps ky*4+kx][Cin]
 * (sketch2img_amd.unet.pack_conv_up2_dgrad: the transposed pre-summed polyphase weights).  16 tap-products per output pixel
 * where the 9-tap dgrad at the upsampled size + 2 x 2 sum-pool spends 36.  Cin % 64 == 0. */
int skg_conv4x4s2_f16(const void* X, int ldx, const void* W16, void* Y, int ldy, int rows, int IH, int IW, int Cin,
                      int Cout, const void* bias, void* stream);

/* ---- accuracy mode ("residual_fp32"): tensors as (hi, lo) PAIRS of fp16, value = hi + lo (~22 mantissa bits) -------
 * north_star asks for <= 1e-3 max latent-eps deviation from the fp32 reference (modules/pipeline.py:96 in fp32 on CPU);
 * with every stored tensor in fp16 - what the reference's own GPU path does (app.py:34) - an evaluation is 1.5e-3 away,
 * 1.0e-3 of it from the fp16 residual stream.  HipUNet(residual_fp32=True) keeps the residual stream and the conv outputs
 * that feed a norm or the residual sum as pairs: the producer's epilogue writes hi = fp16(v) and lo = fp16(v - hi), adds a
 * residual pair in fp32; norms read hi + lo; where the stream itself is a matmul operand the pair is the operand
 * ([hi | lo] along K against [W | W]).  skg_gemm_f16 / skg_conv3x3_f16 take the second output / residual pointer (same leading
 * dimensions); with either of them: fp16 output only, K % 64 == 0 (Cin % 64 == 0), ldc % 8 == 0 (ldr % 8 == 0), all four 16-byte
 * aligned.  The norms take X_lo: the reference's GroupNorm / LayerNorm layers (diffusers ResnetBlock2D / Transformer2DModel /
 * BasicTransformerBlock under modules/pipeline.py:96) evaluated on the fp32-accurate stream. */

/* apply alone (statistics [rows][groups][2] from skg_groupnorm_stats - on the hi part of a pair X + X_lo, X_lo != NULL) */
int skg_groupnorm_apply(const void* X, const void* X_lo, int ldx, void* Y, int ldy, int rows, int HW, int C, int groups,
                        const float* stats, const void* gamma, const void* beta, int silu, void* stream);
int skg_groupnorm_bwd(const void* X, int ldx, const void* dY, int lddy, void* dX, int lddx,
                      const void* residual, int ldr, int rows, int HW, int C, int groups,
                      const float* stats, const void* gamma, const void* beta, int silu,
                      float* partial, void* stream);

/* ---- LayerNorm over the last dim, fp16 [M][C] ------------------------------------------------
 * fwd also writes float2 (mean, rstd) per row to `stats` if non-NULL; X_lo != NULL: LayerNorm of the pair X + X_lo.
 * bwd: dX = LN'(dY) + residual.  Requires C % 8 == 0, C <= 2048.
 * Replaces: BasicTransformerBlock.norm1/2/3 and sketch_norm (modules/clip_guided_attn.py:113). */
int skg_layernorm_fwd(const void* X, const void* X_lo, int ldx, void* Y, int ldy, int M, int C, const void* gamma,
                      const void* beta, float eps, float* stats, void* stream);
int skg_layernorm_bwd(const void* X, int ldx, const void* dY, int lddy, void* dX, int lddx,
                      const void* residual, int ldr, int M, int C, const void* gamma,
                      const float* stats, void* stream);

/* skg_gemm_f16 with SKG_EPI_GEGLU that ALSO stores the pre-activation: Y [M][N/2] = a * gelu(g) and H [M][N] = A B^T + bias
 * in the interleaved pack order (what skg_geglu_bwd takes as its saved H).  One launch instead of GEMM + skg_geglu_fwd
 * for the rows whose gate will be differentiated (the cond rows of a guided step).  K % 64 == 0, N % 16 == 0. */
int skg_gemm_f16_geglu_keep(const void* A, int lda, const void* B, int ldb, void* Y, int ldy, void* H, int ldh,
                            int M, int N, int K, const void* bias, void* stream);

/* ---- Row-local fused feed-forward sub-block (round 3) -----------------------------------
 * Y [M][C] = X + b2 + W2 . geglu(W1 . LayerNorm(X; gamma, beta, eps) + b1)   - ONE launch instead of skg_layernorm_fwd,
 * skg_gemm_f16 with SKG_EPI_GEGLU and skg_gemm_f16 with a residual; the [M][F] gated tensor never exists in memory.
 * C == 320 (the 64 x 64 level of SD1.5, the 96 x 96 level of SD2.1), F = hidden width (1280), F % 32 == 0, F <= 1280.
 * Wpack: fp16 [F/32][60][512] "fragment-major" pack of W1 [2F][C] (diffusers order: value rows, then gate rows) and
 * W2 [C][F]: chunk c holds the 32 hidden units 32c..32c+31 as 40 W1 pieces (tile t = val 0-15, val 16-31, gate 0-15,
 * gate 16-31; k-step ks; piece [lane = 16 g + l][8] = W1[row(t, l)][32 ks + 8 g ..]) then 20 W2 pieces (output tile u;
 * piece [lane][i] = W2[16 u + l][32 c + 16 (i >> 2) + 4 g + (i & 3)]); bias1_pack: fp32 [F/32][4][16] in W1-tile order
 * (sketch2img_amd.unet.pack_ff_block builds both).  stats (optional): float2 (mean, rstd) per row, as skg_layernorm_fwd.
 * Y may alias X.  Same roundings as the three-launch path (fp16 LayerNorm output, fp16 FF1 output before the gate,
 * fp16 gated value, one fp16 rounding of the residual sum).
 * Replaces: BasicTransformerBlock.norm3 / ff (GEGLU) / residual add ([diffusers] attention.py), reached from
 * modules/pipeline.py:96.
 * H != NULL: ALSO store the FF1 output H = fp16(W1 . LayerNorm(X) + b1) of rows >= keep_from to H [M - keep_from][2F]
 * (row m -> H row m - keep_from) in the interleaved pack order skg_geglu_bwd takes as its saved H (what
 * skg_gemm_f16_geglu_keep writes): the cond rows of a guided step, whose gate is differentiated.  keep_from % 16 == 0,
 * ldh % 8 == 0.
 * bias_proj != NULL: followed by Transformer2DModel.proj_out + the transformer's outer residual in the same launch ([diffusers]
 * attention.py Transformer2DModel.forward: `hidden_states = self.proj_out(hidden_states); output = hidden_states + residual`):
 *   Y = R + bias_proj + W_proj . fp16(X + FF(LayerNorm(X)))
 * Wpack holds five more chunks behind the F / 32 feed-forward ones (sketch2img_amd.unet.pack_ff_block(..., w_proj)); the block
 * output never reaches memory (its backward does not read it).  Then gn_partial != NULL: also the GroupNorm partial sums of Y,
 * fp32 [M / HW][HW / 128][groups][2], the layout skg_gemm_f16 leaves (HW % 128 == 0, groups <= 32).  Y must not alias X; it may
 * alias R.
 * X_lo and Y_lo != NULL (accuracy mode; both or neither): PAIR input X + X_lo (pitch ldx) and PAIR output Y + Y_lo (pitch ldy) -
 * LayerNorm reads the sum, the residual sum is formed in fp32 and stored as hi = fp16(v), lo = fp16(v - hi).  With bias_proj
 * (round 5) the outer residual is the pair R + R_lo (pitch ldr) and proj_out takes the block output as the pair it is,
 * W_proj . hi + W_proj . lo on the same weight fragments (the K-doubled [p3_hi | p3_lo] . [W | W] GEMM of the unfused
 * accuracy-mode path, without its second weight read and without the [M, 2C] round trip of p3); gn_partial: the GroupNorm partial
 * sums of Y's hi part. */
int skg_ff_block_f16(const void* X, const void* X_lo, int ldx, void* Y, void* Y_lo, int ldy, int M, int C, int F,
                     const void* gamma, const void* beta, float eps, const void* Wpack, const float* bias1_pack,
                     const void* bias2, const void* bias_proj, const void* R, const void* R_lo, int ldr, float* stats,
                     void* H, int ldh, int keep_from, float* gn_partial, int HW, int groups, void* stream);

/* ---- Row-local fused cross-attention sub-block (round 3; VERDICT r2 next #2, first half) ---------------------------
 * Y [M][C] = X + bo + Wo . Attention(Q = Wq . LayerNorm(X; gamma, beta, eps), K, V) over the Nkv <= 80 text keys of the row's
 * image - ONE launch instead of skg_layernorm_fwd, skg_gemm_f16 (attn2.to_q), skg_attn_fwd with SKG_ATTN_ROWV (77 keys) and skg_gemm_f16 with a
 * residual (attn2.to_out); q, the attention output and the normalised rows never exist in memory.
 * C == 320, heads == 8 (head width 40: the 64 x 64 level of SD1.5); rows [b * HW, (b + 1) * HW) belong to image b, HW % 128 == 0,
 * M % HW == 0; scale = head_width^-0.5.
 * Wpack: fp16 [heads][60][512], KVpack: fp16 [M / HW][heads][16][512] - fragment-major images of Wq / Wo and of the per-image
 * text keys / values (layouts: sketch2img_amd.unet.pack_xattn_weights / pack_xattn_kv, which build them; KVpack once per prompt).
 * Same rounding points as the four-launch path (fp16 LayerNorm output, fp16 q, fp16 scaled q, fp16 probabilities, fp16
 * attention output, one fp16 rounding of the residual sum).  Y may alias X.  No LSE / q / o outputs: for rows nobody
 * differentiates (unguided evaluations, the uncond half of guided ones).
 * Replaces: BasicTransformerBlock.norm2 / attn2 / residual add ([diffusers] attention.py; the op order of
 * modules/clip_guided_attn.py:127-152), reached from modules/pipeline.py:96.
 * Q != NULL: the stashing launch of a guided evaluation (as H of skg_ff_block_f16): rows >= keep_from - a multiple of HW, i.e.
 * whole images: the cond half - ALSO store what the backward of the four replaced launches reads: stats fp32 [M - keep_from][2] =
 * norm2's (mean, rstd) per row, Q / O fp16 [M - keep_from][ldk] = the attn2.to_q output and the attention output (head h in
 * columns 40 h .. 40 h + 39), lse fp32 [(M - keep_from) / HW][heads][HW] in skg_attn_fwd's convention.  Feeds skg_attn_bwd_delta /
 * skg_attn_bwd_dq / skg_layernorm_bwd unchanged.
 * X_lo and Y_lo != NULL (accuracy mode; both or neither): PAIR input X + X_lo (pitch ldx), PAIR output Y + Y_lo (pitch ldy); with
 * Q (round 5) the stash as above. */
int skg_xattn_block_f16(const void* X, const void* X_lo, int ldx, void* Y, void* Y_lo, int ldy, int M, int HW, int C, int heads,
                        int Nkv, const void* gamma, const void* beta, float eps, const void* Wpack, const void* KVpack,
                        const void* bias_out, float scale, float* stats, void* Q, void* O, int ldk, float* lse, int keep_from,
                        void* stream);

/* ---- GEGLU: Y[m][j] = a_j * gelu(g_j),  H fp16 [M][2F] -----------------------------------------------
 * interleaved == 0: H = [a (F columns) | g (F columns)] (diffusers' chunk(2));  interleaved == 1: groups of four
 * columns [a_2t a_2t+1 g_2t g_2t+1] (the pack SKG_EPI_GEGLU uses).  bwd writes dH [M][2F] in the same layout from
 * dY [M][F] and the saved H.  F % 8 == 0.
 * Replaces: diffusers GEGLU (ff.net.0) inside BasicTransformerBlock. */
int skg_geglu_fwd(const void* H, int ldh, void* Y, int ldy, int M, int F, int interleaved, void* stream);
int skg_geglu_bwd(const void* H, int ldh, const void* dY, int lddy, void* dH, int lddh, int M,
                  int F, int interleaved, void* stream);

/* ---- fused multi-head attention (flash style), fp16 --------------------------------------------
 * Q [batch*Nq][..] (ldq), K [batch*kv_stride][..] (ldk), head h occupies columns
 * [h*dh, (h+1)*dh).  Vt is V transposed: Vt[h*dh + d][b*kv_stride + j] (ldvt).  Only the first
 * Nkv of each batch row's kv_stride key slots are valid.  O [batch*Nq][..] (ldo).
 * lse (float [batch][heads][Nq], natural-log-sum-exp of the scaled scores) may be NULL.
 * dh in {16, 32, 40, 64, 80, 160}; kv_stride % 8 == 0 (the V^T operand; SKG_ATTN_ROWV takes any kv_stride).
 * Pad key slots (all four attention entry points): the slots Nkv .. kv_stride - 1 of every batch row ARE READ - skg_attn_fwd and
 * skg_attn_bwd_dq stage whole 64-key tiles of up to kv_stride rows and only mask the scores - and must hold FINITE values (zeros, or
 * whatever finite numbers a projection of padded token rows left there); the results do not depend on them, bit for bit
 * (tests/test_gpu_attention_bwd.py).  An Inf or NaN there reaches the output as 0 * Inf.  K and V (V^T: every row) must therefore
 * have batch * kv_stride readable rows (columns) for skg_attn_fwd and skg_attn_bwd_dq; skg_attn_bwd_dkv touches only the first Nkv
 * rows of every batch row of K, V, dK and dV.
 * Replaces: xformers memory_efficient_attention (enabled at app.py:43) / diffusers
 * CrossAttention baddbmm+softmax+bmm for attn1, attn2 and the injected sketch_attn
 * (modules/clip_guided_attn.py:114, modules/sketch_guided_attn.py:127).
 * flags (SKG_ATTN_ROWV and SKG_ATTN_CAUSAL exclude each other: SKG_E_BADARG):
 *   SKG_ATTN_ROWV    Vt / ldvt are V handed over ROW-MAJOR: V [batch*kv_stride][ldv], head h at columns h*dh.. (e.g. the third
 *                    column block of a fused QKV projection, ldv = 3C).  The kernel reads its V fragments through the gfx950 LDS
 *                    transpose read (ds_read_b64_tr_b16), so no transposed copy of V is written.
 *   SKG_ATTN_CAUSAL  key j of a batch row is visible to query i only when j <= i (self-attention, Nq rows and kv_stride key
 *                    slots per batch row).  dh in {16, 32, 64}.  Replaces: the masked self-attention of transformers'
 *                    CLIPTextModel, which the reference calls through StableDiffusionPipeline._encode_prompt
 *                    (modules/pipeline.py:55-57).
 *   SKG_ATTN_RESIDENT_KV  (only with SKG_ATTN_ROWV, otherwise SKG_E_BADARG) a hint for cross-attention over 81 ... 240 key slots
 *                    (long prompts: clip_text.encode_tokens): K and V of one (batch row, head) are staged in LDS once per workgroup
 *                    and the softmax is a plain one with the exact maximum, as for kv_stride <= 80 - instead of the streaming
 *                    kernel.  Served: dh 40 / 64 / 80 up to kv_stride 240, dh 160 up to 160; every other call (kv_stride <= 80
 *                    or > 240, other head widths, SKG_NO_ATTN_SHORT set) runs exactly as without the flag.  The results differ
 *                    from the streaming kernel's in the last bits, which is why self-attention callers with 81 ... 240 keys
 *                    (small or non-square maps) do not get it implicitly. */
#define SKG_ATTN_CAUSAL 1u
#define SKG_ATTN_ROWV 2u
#define SKG_ATTN_RESIDENT_KV 4u
int skg_attn_fwd(const void* Q, int ldq, const void* K, int ldk, const void* Vt, int ldvt,
                 void* O, int ldo, float* lse, int batch, int heads, int Nq, int Nkv,
                 int kv_stride, int dh, float scale, unsigned flags, void* stream);
/* Which kernel instantiation skg_attn_fwd runs for these arguments (it takes its decision from the same function): 1000 + QT for the
 * streaming kernel (attn_fwd_kernel with QT 16-query tiles per wave: 2, 1 at dh = 160, 3 at dh = 40 on launches of >= 1024
 * workgroups, 4 only behind SKG_ATTN_VAR), 2000 + QT for its SKG_ATTN_CAUSAL instantiation, 3000 + NT for the LDS-resident kernel
 * (attn_fwd_short_kernel with NT 16-key score tiles: 5 up to 80 key slots with SKG_ATTN_ROWV, 10 / 15 behind SKG_ATTN_RESIDENT_KV).
 * Negative: the SKG_E_* skg_attn_fwd returns for this
 * shape and these flags once its pointers and pitches pass.  *queries_per_workgroup (may be NULL; written only on success) = 64 QT,
 * or the resident kernel's query chunk.  Needs no GPU and no buffers; honours the SKG_ATTN_VAR / SKG_NO_ATTN_SHORT switches, which
 * the library reads once per process.  Lets a test name the instantiation it was written for (tests/attn_emulation.py FWD_CASES).
 * Additive entry point (SKG_ABI_VERSION unchanged). */
int skg_attn_fwd_variant(int batch, int heads, int Nq, int Nkv, int kv_stride, int dh, unsigned flags, int* queries_per_workgroup);
/* backward.  delta[b][h][q] = sum_d dO*O (skg_attn_bwd_delta).  All operands row-major like their primals (Q, dO
 * [batch*Nq][..], K, V [batch*kv_stride][..]); the transposed fragments the dQ / dK / dV products need (K^T, Q^T, dO^T)
 * are read from the row tiles in LDS through ds_read_b64_tr_b16 - no transposed copies in HBM.  Outputs row-major.
 * Replaces: torch autograd through xformers memory_efficient_attention / CrossAttention, triggered by
 * torch.autograd.grad at modules/pipeline.py:159. */
int skg_attn_bwd_delta(const void* O, int ldo, const void* dO, int lddo, float* delta, int batch,
                       int heads, int Nq, int dh, void* stream);
/* dq.  delta given: O / ldo / delta_out are not looked at.  delta == NULL (round 5): skg_attn_bwd_delta in the prologue - O
 * [batch*Nq][ldo] is the forward's output; delta is formed from the dO fragments the launch loads anyway, used, and stored to
 * delta_out [batch][heads][Nq] for the skg_attn_bwd_dkv launch that follows (summation order differs from skg_attn_bwd_delta's:
 * equal to fp32 rounding, not bit for bit). */
int skg_attn_bwd_dq(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, const void* dO, int lddo,
                    const void* O, int ldo, const float* lse, const float* delta, float* delta_out, void* dQ, int lddq,
                    int batch, int heads, int Nq, int Nkv, int kv_stride, int dh, float scale, void* stream);
/* dK, dV.  K, V, dK, dV rows of batch row b start at b * kv_stride (kv_stride >= Nkv; dense buffers: kv_stride = Nkv; a padded
 * K / V buffer such as the injected attention's [N image tokens ; T sketch tokens -> multiple of 8]: same kernel, same grid).
 * Rows Nkv .. kv_stride - 1 of dK / dV are left untouched. */
int skg_attn_bwd_dkv(const void* Q, int ldq, const void* K, int ldk,
                     const void* V, int ldv, const void* dO, int lddo,
                     const float* lse, const float* delta, void* dK, int lddk, void* dV, int lddv,
                     int batch, int heads, int Nq, int Nkv, int kv_stride, int dh, float scale, void* stream);

/* ---- data movement -----------------------------------------------------------------------------*/
/* Out[c][m] = In[m][c], fp16, In [M][C] (ldi), Out [C][M] (ldo).  C % 8 == 0, M % 8 == 0. */
int skg_transpose_f16(const void* In, int ldi, void* Out, int ldo, int M, int C, void* stream);
/* Y[m][c] = alpha*A[m][c] + beta*B[m][c] (B may be NULL); fp16, C % 8 == 0.  Used for channel
 * concat (copy into a slice), skip-gradient accumulation and slicing. */
int skg_axpby_f16(const void* A, int lda, const void* B, int ldb, void* Y, int ldy, int M, int C,
                  float alpha, float beta, void* stream);
/* Out[b*out_batch_rows + r][:] = In[b*in_batch_rows + r][:] for b < batches, r < rows_per_batch (fp16, C % 8 == 0).
 * Moves the N image tokens of every batch row into / out of the [N + 257 (+pad)]-token buffer of the
 * injected self-attention, i.e. the torch.cat(..., dim=1) and [:, :N] slice of
 * modules/clip_guided_attn.py:113,119. */
int skg_batch_copy_f16(const void* In, int ldi, int in_batch_rows, void* Out, int ldo, int out_batch_rows,
                       int batches, int rows_per_batch, int C, void* stream);
/* Y = silu(X), fp16 [M][C], C % 8 == 0.  Used once per timestep for the time-embedding MLP
 * (diffusers TimestepEmbedding / ResnetBlock2D.time_emb_proj input), off the per-step path. */
int skg_silu_f16(const void* X, int ldx, void* Y, int ldy, int M, int C, void* stream);
/* Y = X * sigmoid(1.702 X): transformers' "quick_gelu", the MLP activation of the CLIP vision tower that
 * modules/clip_guided_inf.py:49-54,103 runs to produce the sketch tokens. */
int skg_quick_gelu_f16(const void* X, int ldx, void* Y, int ldy, int M, int C, void* stream);
/* Its backward: out = dY * s * (1 + 1.702 F (1 - s)) with s = sigmoid(1.702 F), F = the activation's INPUT (the fc1 output);
 * fp32 arithmetic, fp16 [M][C] views with their own row pitches, C % 8 == 0; out may alias dY.  The MLP step of the CLIP
 * vision tower's backward (modules/clip_guided_trainer.py:116-119 trains the tower).  Additive: same ABI version. */
int skg_quick_gelu_bwd_f16(const void* F, int ldf, const void* dY, int lddy, void* out, int ldo, int M, int C, void* stream);
/* Y = X/2 (1 + erf(X / sqrt 2)): exact "gelu", the MLP activation of the OpenCLIP text encoder that SD 2.x
 * checkpoints carry (transformers CLIPTextModel with hidden_act = "gelu"; modules/pipeline.py:55-57). */
int skg_gelu_f16(const void* X, int ldx, void* Y, int ldy, int M, int C, void* stream);
/* adjoint of nearest 2x upsample: Y[b][y][x][c] = sum of the 2x2 block of X.  X [rows*2H*2W][C]. */
int skg_sumpool2x2_f16(const void* X, int ldx, void* Y, int ldy, int rows, int H, int W, int C,
                       void* stream);
/* NCHW float [rows][C][HW]  ->  NHWC fp16 [rows*HW][Cpad] (channels >= C zero-filled) and back
 * (the inverse reads the first C channels of fp16 [rows*HW][ldx] into float NCHW). */
int skg_nchw_f32_to_nhwc_f16(const float* X, void* Y, int rows, int C, int HW, int Cpad, void* stream);
int skg_nhwc_f16_to_nchw_f32(const void* X, int ldx, float* Y, int rows, int C, int HW, void* stream);

/* ---- LGP (Latent Gradient/Edge Predictor) pieces ------------------------------------------------
 * Layer 0 is re-associated with the bilinear resize: per tap i the caller runs
 * skg_gemm_f16(F_i, W0[:, off_i:off_i+C_i]) -> P_i fp32 [rows*s_i*s_i][H0] at the tap's NATIVE
 * size; skg_lgp_layer0_gather then forms, for every output pixel of the h x w grid,
 *   z = relu( fp16( sum_i bilinear_i(P_i) + W0[:, E:E+40] . fp16(e) + b0 ) )
 * with e = [nl(4), sin(2 pi nl 2^-l) l=0..8 (36)], nl = sigma * noise  (fp32, then fp16 cast, as
 * modules/latent_predictor.py:39-43).  Output Z fp16 [rows*h*w][H0], pixel order (y, x), pixel = y*w + x.
 * w == h: the square grid, any h.  w != h: h, w multiples of 8, and a tap of height s has width s*w/h (the same power-of-two scale
 * on both axes): P [rows*s*(s*w/h)][H0], noise / target float NCHW [samples][4][h][w].
 * `taps` is a HOST array of ntaps (<= 12) SkgLgpTap; rows = 2*samples in the row layout
 * [uncond rows of all samples; cond rows of all samples].  Replaces F.interpolate x9 + cat + cast + layer 0 of
 * modules/pipeline.py:146-153 / modules/latent_predictor.py:42-45. */
typedef struct {
  const float* P;   /* fp32 [rows*s*(s*w/h)][H0] */
  int s;            /* native height */
  int pad_;
} SkgLgpTap;
/* Wextra may be NULL (h % 8 == 0 and H0 % 128 == 0 required): the caller then supplies the product of the 40 extra
 * channels (skg_lgp_extra_features x W0[:, E:], an fp32 GEMM) as one more tap with s == h - the matrix pipe does the
 * 40-wide dot products instead of 160 cached vector loads per thread. */
int skg_lgp_layer0_gather(const SkgLgpTap* taps, int ntaps, const void* Wextra, int ldw,
                          const void* bias0, const float* noise, float sigma, int samples,
                          void* Z, int rows, int h, int w, int H0, void* stream);
/* adjoint of the bilinear part for ONE tap: dP [rows*s*(s*w/h)][H0] fp16 from dZ [rows*h*w][H0] fp16. */
int skg_lgp_layer0_scatter(const void* dZ, int lddz, void* dP, int rows, int h, int w, int s, int H0,
                           void* stream);
/* train-mode BatchNorm1d whose "batch" is ONE sample's LGP rows (the reference only runs B = 1:
 * SURVEY Q1/Q3).  Row layout of X: row = (j*samples + s)*seg_rows + i, j = 0..segs-1 (segs = 2 CFG
 * halves, seg_rows = h*h).  X is the post-ReLU activation fp16 [samples*segs*seg_rows][C].
 * stats float [samples][C][2] = (mean, rstd), biased variance.  If running_mean/var != NULL
 * (float [C]) they receive the momentum-0.1 / unbiased-variance update once per sample, in sample
 * order (= the side effect of `samples` consecutive reference calls).
 * apply:    Y = fp16((x-mean)*rstd*gamma+beta).
 * relu_bwd: dX = [x>0] * gamma*rstd*(dY - mean_s(dY) - xhat*mean_s(dY*xhat))  - BatchNorm backward
 *           including the statistic terms, then the ReLU that precedes the BN in
 *           modules/latent_predictor.py:15-27 (x is post-ReLU so relu'(.) = [x>0]).  With
 *           train_mode == 0 the statistic terms are dropped (eval-mode BN: stats from running).
 * scratch: skg_bn_scratch_floats(samples, C) floats. */
size_t skg_bn_scratch_floats(int samples, int C);
int skg_bn_stats(const void* X, int ldx, int samples, int segs, int seg_rows, int C, float eps,
                 float* stats, float* scratch, float* running_mean, float* running_var,
                 void* stream);
int skg_bn_stats_from_running(const float* running_mean, const float* running_var, int samples,
                              int C, float eps, float* stats, void* stream);
int skg_bn_apply(const void* X, int ldx, void* Y, int ldy, int samples, int segs, int seg_rows,
                 int C, const float* stats, const void* gamma, const void* beta, void* stream);
int skg_bn_relu_bwd(const void* X, int ldx, const void* dY, int lddy, void* dX, int lddx,
                    int samples, int segs, int seg_rows, int C, const float* stats,
                    const void* gamma, int train_mode, float* scratch, void* stream);
/* MSE seed: for the cond rows, dOut = loss_scale * 2*(out - target)/(n) with n = 4*h*w, zero for the
 * uncond rows; also writes loss (float[samples]).  out fp16 [2*samples*h*w][ldo] (uncond block then
 * cond block, (y,x) pixel order), first 4 columns valid; target float NCHW [samples][4][h][w] (w != h: multiples of 8).  dOut fp16 [..][ldd],
 * columns >= 4 zeroed up to ldd.  Mirrors modules/pipeline.py:155-157. */
int skg_lgp_mse_seed(const void* out, int ldo, const float* target, void* dOut, int ldd,
                     float* loss, int samples, int h, int w, float loss_scale, void* stream);

/* ---- LGP training (trainer.py:208-252: forward taps -> LGP -> MSE -> backward with weight gradients -> optimizer) --
 * The reference trains with accelerate fp16 autocast + bitsandbytes AdamW8bit; here: fp16 compute with a static loss
 * scale, fp32 master weights, plain AdamW (8-bit moments: skg_adamw8_step below).  Weight gradients are GEMMs on transposed operands (skg_transpose_f16 +
 * skg_gemm_f16 with SKG_EPI_OUT_F32); these are the remaining pieces. */
/* out[c] = scale * sum_m X[m][c]  (bias gradients).  scratch: skg_colsum_scratch_floats(C) floats. */
size_t skg_colsum_scratch_floats(int C);
int skg_colsum_f16(const void* X, int ldx, int M, int C, float scale, float* out, float* scratch, void* stream);
/* BatchNorm1d parameter gradients over `rows` rows of ONE batch: dgamma[c] = scale * sum dY*xhat, dbeta[c] = scale *
 * sum dY, xhat from stats (mean, rstd)[C] of skg_bn_stats(samples = 1).  scratch: skg_bn_scratch_floats(1, C). */
int skg_bn_param_grads(const void* X, int ldx, const void* dY, int lddy, int rows, int C, const float* stats,
                       float scale, float* dgamma, float* dbeta, float* scratch, void* stream);
/* The 40 extra input channels of LGP layer 0 (noise level x4, sin(2 pi nl 2^-l) x36; modules/latent_predictor.py:39-41),
 * fp16, E [rows*h*w][ld] with columns >= 40 zeroed: the operand of the layer-0 weight gradient for those columns (w != h:
 * multiples of 8). */
int skg_lgp_extra_features(const float* noise, float sigma, int samples, int rows, int h, int w, void* E, int ld,
                           void* stream);
/* Training loss (trainer.py:240): mean((out - target)^2) over samples*4*h*h; dOut = loss_scale * d loss / d out
 * (fp16 [samples*h*h][ldd], columns >= 4 zero); loss_parts[s] = this sample's share of the mean (sum them). */
int skg_lgp_mse_train(const void* out, int ldo, const float* target, void* dOut, int ldd, float* loss_parts,
                      int samples, int h, float loss_scale, void* stream);
/* One AdamW step on a flat fp32 parameter vector (decoupled weight decay, bias correction for `step` >= 1); grad is
 * multiplied by inv_grad_scale first; param_f16 (optional) receives the fp16 working copy. */
int skg_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* param_f16, size_t n,
                   float lr, float beta1, float beta2, float eps, float weight_decay, int step, float inv_grad_scale,
                   void* stream);
/* ---- dynamic loss scale (sketch2img_amd/loss_scaler.py: the reference's GradScaler) ----------------------
 * *flag = 1.0f if any of x[0, n) is +-inf or NaN (exponent bits all ones); otherwise *flag is left alone, so several vectors
 * OR into one flag.  reset != 0 zeroes *flag first, on the stream.  x: any 4-byte aligned pointer, n >= 1; one pass, no
 * host synchronisation. */
int skg_nonfinite_flag(const float* x, size_t n, float* flag, int reset, void* stream);
/* skg_adamw_step that reads *skip_flag (device memory, e.g. skg_nonfinite_flag's) once: non-zero -> param, exp_avg,
 * exp_avg_sq and param_f16 are left untouched; zero -> the same bits as skg_adamw_step. */
int skg_adamw_step_guarded(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* param_f16, size_t n,
                           float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                           float inv_grad_scale, const float* skip_flag, void* stream);

/* ---- 8-bit AdamW state (sketch2img_amd/flat_adamw.py state_bits = 8; the reference's bitsandbytes AdamW8bit, restated from
 * Dettmers et al., "8-bit Optimizers via Block-wise Quantization": DESIGN.md section 15) -----------------
 * One row of the block table: `len` <= 2048 consecutive elements of ONE tensor, starting `off` elements into param / grad /
 * param_f16 and `state_off` elements into the state arrays - state1 / state2 when is8 != 0, exp_avg32 / exp_avg_sq32 when
 * is8 == 0 (a tensor below min_8bit_size keeps fp32 moments).  off and state_off are multiples of 8. */
typedef struct SkgAdamw8Row {
  long long off, len, state_off, is8;
} SkgAdamw8Row;
/* One AdamW step (skg_adamw_step's arithmetic on fp32 values) over `nrows` table rows in one launch.  8-bit rows: exp_avg =
 * qmap1[state1] * absmax1[row], exp_avg_sq = qmap2[state2] * absmax2[row] are dequantised, updated, param / param_f16
 * (optional) written from the fresh fp32 moments, then absmax := max |.| over the row and code := #{ j : mid[j] < x / absmax }
 * (the zero code where absmax == 0).  qtab (device, 1024 floats): qmap1[256], its thresholds mid1[j] = 0.5f * (q[j] + q[j + 1])
 * in [0, 255) and one unused float, qmap2[256], mid2 likewise.  absmax1 / absmax2: one float per table row.  skip (optional,
 * device): non-zero -> nothing is touched (skg_adamw_step_guarded's flag).  nrows == 0: nothing to do. */
int skg_adamw8_step(float* param, const float* grad, void* param_f16, unsigned char* state1, unsigned char* state2,
                    float* absmax1, float* absmax2, float* exp_avg32, float* exp_avg_sq32, const SkgAdamw8Row* rows, int nrows,
                    const float* qtab, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                    float inv_grad_scale, const float* skip, void* stream);

/* ---- sampler elementwise -------------------------------------------------------------------------
 * CFG combine + DDIM step (eta = 0) on float NCHW latents:
 *   eps = eps_u + g*(eps_c - eps_u);  x0 = (x - c1*eps)/c0;  x_prev = c2*x0 + c3*eps
 * eps_u / eps_c are fp16 NHWC [HW][ld] rows of the UNet output (first 4 channels); lo_off != 0 (accuracy mode): eps is a
 * (hi, lo) pair whose lo part sits lo_off columns to the right in the same rows (0 = plain fp16).
 * vpred = 1 (scheduler config prediction_type "v_prediction", the public SD2.1-768 checkpoint): the UNet output is v;
 *   v = v_u + g*(v_c - v_u);  eps = c0*v + c1*x;  x0 = c0*x - c1*v;  x_prev as above (eps_out receives the derived eps).
 * Replaces modules/pipeline.py:99-104 (CFG + scheduler.step). */
int skg_cfg_ddim_step(const void* eps_u, const void* eps_c, int ld, int lo_off, const float* x, float* x_prev,
                      float* eps_out, int samples, int HW, float g, float c0, float c1, float c2,
                      float c3, int vpred, void* stream);
/* The same step with DDIM's noise term (eta > 0; diffusers DDIMScheduler.step(eta=, generator=)):
 *   x_prev = c2*x0 + c_dir*eps + sigma*z,   sigma = eta * sqrt((1-a_prev)/(1-a_t) * (1 - a_t/a_prev)),  c_dir = sqrt(1 - a_prev - sigma^2)
 * z: caller-drawn N(0, 1), float NCHW like x (required).  eps, x0, the pair offset, vpred and eps_out as above; the five
 * scalars are host-side fp32 table arithmetic (sketch2img_amd/sampler.py DDIMTables.coeffs_eta). */
int skg_cfg_ddim_eta_step(const void* eps_u, const void* eps_c, int ld, int lo_off, const float* x, const float* z,
                          float* x_prev, float* eps_out, int samples, int HW, float g, float c0, float c1,
                          float c2, float c_dir, float sigma, int vpred, void* stream);
/* ---- VAE decoder helpers (modules/pipeline.py:118 decode_latents; third-party AutoencoderKL.decode) -------------
 * Row softmax y[m][:] = softmax(x[m][:]) of fp16 scores, fp32 arithmetic: the decoder's single-head mid attention
 * (AttentionBlock: softmax(q k^T / sqrt(C)) v over HW tokens) is GEMM -> this -> GEMM.  N % 8 == 0. */
int skg_softmax_rows_f16(const void* x, int ldx, void* y, int ldy, int M, int N, void* stream);
/* decode_latents tail: out[px][c] = clamp(x[px][c]*scale + shift, 0, 1), fp16 NHWC (row pitch ld) -> float NHWC
 * (the (B, H, W, 3) array the pipeline converts to PIL; scale 0.5, shift 0.5). */
int skg_image_postprocess(const void* x, int ld, float* out, size_t pixels, int C, float scale, float shift,
                          void* stream);

/* The same tail fused with numpy_to_pil's quantisation (modules/pipeline.py:125 -> diffusers numpy_to_pil:
 * (images * 255).round().astype("uint8")): out[px][c] = rint(clamp(x*scale + shift, 0, 1) * 255), uint8 NHWC
 * [pixels][C] - the (S, 512, 512, 3) payload a rank contributes to the final gather of decoded images. */
int skg_image_to_u8(const void* x, int ld, void* out, size_t pixels, int C, float scale, float shift, void* stream);

/* VAE encoder tail (app.py:109: vae.encode(img).latent_dist.sample() * 0.18215): from the fp16 NHWC moments
 * [samples*HW][ld] = (mean[0..L), logvar[L..2L)) to float NCHW [samples][L][HW]:
 *   out = (mean + exp(0.5 * clamp(logvar, -30, 20)) * noise) * scale;   noise NULL -> the mode (mean * scale).
 * noise is a caller-drawn standard normal tensor in the output layout (the reference draws it from torch's RNG). */
int skg_gaussian_sample(const void* moments, int ld, const float* noise, float* out, int samples, int L, int HW,
                        float scale, void* stream);

/* CFG combine + one DPM-Solver++ (2M, midpoint) update - the scheduler app.py:13-25 configures - on float NCHW latents:
 *   eps = eps_u + g*(eps_c - eps_u);  x0 = (x - sigma_s*eps)/alpha_s;  x_prev = a*x + b*x0 + c*x0_before
 * x0_io [samples][4][HW] float: the previous step's x0 on entry (not read when c == 0: first-order step), this
 * step's x0 on exit.  The five scalars are host-side fp32 table arithmetic (sketch2img_amd/sampler.py DPMTables).
 * vpred = 1: the UNet output is v: x0 = alpha_s*x - sigma_s*v (eps_out: alpha_s*v + sigma_s*x).
 * Replaces modules/pipeline.py:99-104 when the pipeline was built with DPMSolverMultistepScheduler. */
int skg_cfg_dpmpp2m_step(const void* eps_u, const void* eps_c, int ld, int lo_off, const float* x, float* x0_io,
                         float* x_prev, float* eps_out, int samples, int HW, float g, float alpha_s,
                         float sigma_s, float a, float b, float c, int vpred, void* stream);
/* The same update with the noise term of the stochastic solver (scheduler config algorithm_type "sde-dpmsolver++"):
 *   x_prev = a*x + b*x0 + c*x0_before + d*z
 * with  h = lambda_t - lambda_s,  a = (sigma_t/sigma_s)*exp(-h),  b = alpha_t*(1 - exp(-2h))  [second order: * (1 + 0.5/r0)],
 * c = 0  [second order: -0.5*alpha_t*(1 - exp(-2h))/r0],  d = sigma_t*sqrt(1 - exp(-2h))  (DPMTables.coeffs_sde).
 * z: caller-drawn N(0, 1), float NCHW like x (required).  The three products are summed as skg_cfg_dpmpp2m_step sums them and
 * d*z is added on top as a rounded product: d = 0 gives that entry point's result bit for bit.  Additive entry point
 * (SKG_ABI_VERSION unchanged). */
int skg_cfg_dpmpp2m_sde_step(const void* eps_u, const void* eps_c, int ld, int lo_off, const float* x, const float* z,
                             float* x0_io, float* x_prev, float* eps_out, int samples, int HW, float g, float alpha_s,
                             float sigma_s, float a, float b, float c, float d, int vpred, void* stream);
/* ---- sigma-space samplers: Euler and Euler ancestral (diffusers EulerDiscreteScheduler / EulerAncestralDiscreteScheduler).  The
 * trajectory is x = x0 + sigma*eps with sigma up to 14.6 and the UNet reads x / sqrt(sigma^2 + 1).  Additive entry points
 * (SKG_ABI_VERSION unchanged).
 *
 * The UNet operand of one step - modules/pipeline.py:85-86, torch.cat([latents] * 2) and scheduler.scale_model_input, plus the
 * layout change of skg_nchw_f32_to_nhwc_f16 - in one launch.  x: float NCHW [samples][C][HW].
 *   y         fp16 NHWC [dup*samples*HW][Cpad], dup 1 or 2 (the second copy is the CFG twin): half(c_in * x), the fp32 product
 *             rounded once; columns C..Cpad-1 zero, as skg_nchw_f32_to_nhwc_f16 writes them (c_in = 1 gives its output bit for bit);
 *   x_scaled  NULL, or float NCHW [samples][C][HW] = c_in * x: latent_model_input, the `latents_prev` the guidance update
 *             measures its length from (modules/pipeline.py:109, :160). */
int skg_model_input(const float* x, void* y, float* x_scaled, int samples, int C, int HW, int Cpad, int dup, float c_in,
                    void* stream);
/* CFG combine + one Euler / Euler-ancestral update - modules/pipeline.py:99-104 with one of the two schedulers - on float NCHW
 * latents, eps operands and lo_off as in skg_cfg_ddim_step (the pair's halves are summed in fp32):
 *   m = eps_u + g*(eps_c - eps_u);  x0 = k_x*x + k_m*m;  d = (x - x0)/sigma;  x_prev = x + dt*d + sigma_up*z
 * epsilon prediction: k_x = 1, k_m = -sigma; v prediction: k_x = 1/(sigma^2 + 1), k_m = -sigma/sqrt(sigma^2 + 1).
 * Euler: dt = sigma_next - sigma, sigma_up = 0, z NULL.  Ancestral: sigma_up = sqrt(sigma_next^2 (sigma^2 - sigma_next^2)/sigma^2),
 * dt = sqrt(sigma_next^2 - sigma_up^2) - sigma, z a caller-drawn N(0, 1) float NCHW like x; the last step (sigma_next = 0) has
 * sigma_up = 0 and dt = -sigma: x_prev = x0.  The scalars are float64 host arithmetic cast once (sampler.py EulerTables.coeffs).
 * eps_out (nullable) receives d.  z NULL with sigma_up != 0 is SKG_E_BADARG, nothing launched; every product is rounded before
 * its sum, so sigma_up = 0 with a finite z gives the z = NULL result bit for bit. */
int skg_cfg_euler_step(const void* eps_u, const void* eps_c, int ld, int lo_off, const float* x, const float* z, float* x_prev,
                       float* eps_out, int samples, int HW, float g, float sigma, float k_x, float k_m, float dt, float sigma_up,
                       void* stream);
/* guidance update, modules/pipeline.py:159-161, per sample s:
 *   g = -grad[s] (fp16 NHWC [HW][ld], first 4 ch);  alpha = sqrt(2)*||x_in - x_prev|| / ||g|| * beta
 *   x_prev += alpha * g.   aux float [samples][4] receives (alpha, ||g||, ||x_in-x_prev||*sqrt2, 0). */
int skg_guidance_update(const void* grad, int ld, const float* x_in, float* x_prev, float* aux,
                        int samples, int HW, float beta, void* stream);
/* img2img start and masked repaint (diffusers' scheduler.add_noise and the legacy inpainting blend) on float NCHW latents
 * [samples][4][HW]:   r = a*init + s*noise   with (a, s) the schedule level (DDIMTables.level / DPMTables.level).
 *   mask NULL:  x = r.
 *   mask:       float [mask_samples][HW], one channel for the four, mask_samples 1 (one mask for every sample) or `samples`;
 *               x = m*x + (1 - m)*r in place (1 = repaint, 0 = keep the original).
 * Every product is rounded before its sum: m = 1 leaves x as it is, m = 0 gives the mask-free r, (a, s) = (1, 0) gives init,
 * each bit for bit.  Any HW (16-byte accesses when HW % 4 == 0 and the operands are 16-byte aligned).  Additive entry point
 * (SKG_ABI_VERSION unchanged). */
int skg_latent_renoise(const float* init, const float* noise, const float* mask, int mask_samples, float* x, int samples,
                       int HW, float a, float s, void* stream);

/* Box calibration (bench.py `config.box_mfma_tflops`; no reference call site - measurement infrastructure): one launch of
 * SKG_BOX_PROBE_WORKGROUPS workgroups x 8 waves, each wave `iters` rounds of 40 register-resident 16x16x32 fp16 MFMAs on
 * pseudo-random operands = SKG_BOX_PROBE_WORKGROUPS * 8 * iters * 40 * 16384 flop.  out: float [SKG_BOX_PROBE_WORKGROUPS * 512]
 * (the accumulator sums: only there so that the loop is not removed).  Time it with events on `stream`. */
#define SKG_BOX_PROBE_WORKGROUPS 512
int skg_box_probe_mfma(float* out, int iters, void* stream);

/* ---- sketch generator: the anime2sketch U-Net (anime2sketch/model.py UnetGenerator(3, 1, 8, 64, InstanceNorm2d), called by
 * generate_sketch at trainer.py:36-44 and pic2sketch at anime2sketch/generate.py:7-15) ---------------------------------------
 * Additive entry points (SKG_ABI_VERSION unchanged).  The down convolutions are skg_conv4x4s2_f16 on the [Cout][16 taps][Cin]
 * pack of the Conv2d weight; the first one (3 input channels) is skg_a2s_patch_f16 + ONE skg_gemm_f16 with K = 64.
 *
 * InstanceNorm2d(C, affine = False, track_running_stats = False) over NHWC fp16 with up to two activated outputs - replaces
 * nn.InstanceNorm2d followed by the in-place nn.LeakyReLU(0.2) of the next block, the in-place nn.ReLU in front of the up
 * convolution and the torch.cat of the skip connection:
 *   n = (x - mean) / sqrt(var + eps) per (row, channel) over HW, biased variance, statistics in fp32 / fp64 of the fp16 values;
 *   Yk[m][c] = act_k(fp16(n)),  act_k(v) = v >= 0 ? v : slope_k * v   (slope 0.2: LeakyReLU, 0: ReLU, 1: none)
 * X [rows*HW][ldx >= C]; Y0 / Y1 [rows*HW][ldy_k >= C], each may be a column slice of a wider buffer (the skip half of the
 * concatenation the up convolution reads) and either may be NULL.  identity != 0: no statistics, n = x (the two activated
 * copies of a convolution output that has no norm).  C % 64 == 0; all pointers 16-byte aligned, ld % 8 == 0.
 * Workgroups take (slab of pixels, 64 channels, sample).  HW <= 256: one launch (statistics + apply); larger maps: per-slab partial
 * sums (256 pixels per slab, longer slabs beyond 65536 pixels: at most 256 of them) into `scratch`, a fold in slab order to
 * (mean, rstd) per (sample, channel), then the apply launch.  scratch: skg_instnorm_scratch_floats(rows, HW, C) floats,
 * caller-owned; may be NULL when that is 0 or identity.  No atomics: two runs give identical bits. */
size_t skg_instnorm_scratch_floats(int rows, int HW, int C);
int skg_instnorm_act_f16(const void* X, int ldx, int rows, int HW, int C, float eps, int identity, void* Y0, int ldy0,
                         float slope0, void* Y1, int ldy1, float slope1, float* scratch, void* stream);
/* nn.ConvTranspose2d(Cin, Cout, kernel_size = 4, stride = 2, padding = 1) (the upconv of every UnetSkipConnectionBlock),
 * POLYPHASE on the kernel of skg_conv3x3_up2_f16: output pixel (2i+a, 2j+b) reads low-res rows {i-1, i} with filter rows (3, 1)
 * for a = 0, {i, i+1} with (2, 0) for a = 1, the same for columns.  X [rows*IH*IW][ldx >= Cin] (the [skip | up] concatenation
 * buffer: Cin up to 1024), Y [rows*2IH*2IW][ldy >= Cout], Wpp [4 phases 2a+b][Cout][4 taps][Cin]
 * (sketch2img_amd.anime2sketch.pack_convt: no pre-summing).  Cin % 64 == 0, Cout % 8 == 0 (a single output channel is padded
 * with zero filters).  epilogue SKG_CONVT_EPI_TANH: tanh over the Cout columns of Y (the nn.Tanh of the outermost block), a
 * second launch over the stored fp16 values.  Returns SKG_E_UNSUPPORTED, nothing launched, when an operand spans 2 GiB or more. */
#define SKG_CONVT_EPI_NONE 0
#define SKG_CONVT_EPI_TANH 1
int skg_convt4x4s2_f16(const void* X, int ldx, const void* Wpp, void* Y, int ldy, int rows, int IH, int IW, int Cin, int Cout,
                       const void* bias, int epilogue, void* stream);
/* Operand of the first down convolution (nn.Conv2d(3, 64, 4, 2, 1) on the picture): img float [B][3][H][W] (H, W even) ->
 * P [B*(H/2)*(W/2)][ldp >= 64] fp16, P[(b, oy, ox)][(ky*4 + kx)*3 + c] = img[b][c][2oy-1+ky][2ox-1+kx] (0 outside), columns 48..63
 * zero: the layer is then skg_gemm_f16 with K = 64 against sketch2img_amd.anime2sketch.pack_conv_first.  Replaces the float ->
 * NHWC conversion and a 64-channel zero padding of the picture. */
int skg_a2s_patch_f16(const float* img, void* P, int ldp, int B, int H, int W, void* stream);
/* Tail of the generator and of generate_sketch (trainer.py:39-42): y = column 0 of Y [B*H*W][ldy] (fp16, after tanh) ->
 * y_out float [B][1][H][W] and / or mask float [B][3][H][W] = (1 - y < 0.5 ? 0 : 1) tiled to three channels.  Either may be NULL. */
int skg_a2s_tail(const void* Y, int ldy, float* y_out, float* mask, int B, int H, int W, void* stream);

/* ---- injected-attention (SatMixin) training: weight gradients (csrc/train.hip) -------------------------------------------*/
/* dW[N][K] (fp32, dense) = or += alpha * dY^T . X;  db[N] (may be NULL) = or += alpha * column sums of dY, same pass.
 * dY [M][ldy], X [M][ldx] fp16 row-major (ldy >= N, ldx >= K: column views are fine), contraction over the M >= 1 rows (tail
 * rows masked).  N % 8 == 0, K % 8 == 0, ldy % 8 == 0, ldx % 8 == 0, operands 16-byte aligned.  accumulate != 0: +=.
 * M is split over workgroups into fp32 slabs in `scratch` (skg_wgrad_scratch_floats(M, N, K) floats) that a second launch
 * folds in a fixed order: no atomics, bit-repeatable. */
size_t skg_wgrad_scratch_floats(int M, int N, int K);
int skg_wgrad_f16(const void* dY, int ldy, const void* X, int ldx, int M, int N, int K, float alpha, int accumulate,
                  float* dW, float* db, float* scratch, void* stream);
/* dgamma[c] = or += scale * sum_rows dY[r][c] * (X[r][c] - mean[r]) * rstd[r];  dbeta[c] = or += scale * sum_rows dY[r][c].
 * stats [M][2] = (mean, rstd) as skg_layernorm_fwd stores them.  C % 8 == 0; scratch: skg_layernorm_param_scratch_floats(C)
 * floats.  Two stages, fixed order. */
size_t skg_layernorm_param_scratch_floats(int C);
int skg_layernorm_param_grads(const void* X, int ldx, const void* dY, int lddy, int M, int C, const float* stats, float scale,
                              int accumulate, float* dgamma, float* dbeta, float* scratch, void* stream);

/* ---- ControlNet hint encoder: the small-channel 3x3 convolutions (csrc/condembed.hip) ---------------------------------------
 * Additive entry point (SKG_ABI_VERSION unchanged).  The first three layers of diffusers' ControlNetConditioningEmbedding run at
 * the pixel resolution with 3 and 16 input channels, which skg_conv3x3_f16 (Cin % 32 == 0) does not take:
 *   Y[(b, oy, ox)][n] = act(bias[n] + sum_{ky,kx,c} X[b][stride*oy + ky - 1][stride*ox + kx - 1][c] * W[n][ky][kx][c])   (0 outside)
 * Cin == 3:  X is the picture as it is, float [B][3][IH][IW] (ldx ignored), rounded to fp16 on the way into the MFMA;
 *            Wp [Cout][64] fp16, Wp[n][(3 ky + kx) * 4 + c], every other column zero.
 * Cin == 16: X fp16 [B*IH*IW][ldx >= 16] (ldx % 8 == 0, 16-byte aligned); Wp [Cout][160] fp16, Wp[n][(3 ky + kx) * 16 + c],
 *            columns 144 .. 159 zero.       (sketch2img_amd.packs.pack_conv_small makes both.)
 * Cout 16 or 32; stride 1, or 2 with even IH and IW (OH = IH / stride); Y fp16 [B*OH*OW][ldy >= Cout], ldy % 4 == 0, 8-byte
 * aligned; bias [Cout] fp16 or NULL; silu != 0: act = SiLU, else the identity.  fp32 accumulation, one rounding. */
int skg_conv3x3_small_f16(const void* X, int ldx, const void* Wp, void* Y, int ldy, int B, int IH, int IW, int Cin, int Cout,
                          int stride, const void* bias, int silu, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SKG_H_ */
