/* egaze_hip.h -- C ABI of libegaze_hip.so (gfx950 / MI355X only).
 *
 * The drop-in boundary of the SP / AT / LF hot path of hyf015/egocentric-gaze-prediction.  The reference has no
 * FFI layer of its own: its hot path is the set of torch.nn ops that models/model_SP.py, models/LSTMnet.py,
 * models/late_fusion.py and floss.py execute.  Each entry point below replaces one of those
 * op instances (forward and backward); the reference-side binding is the ctypes table in
 * egocentric-gaze-prediction_amd/_lib.py (INTEGRATION.md shows how a maintainer wires it into the reference).
 *
 * Conventions
 *   - device pointers only (fp32 unless stated); no allocation and no synchronisation inside: the caller passes
 *     workspaces (sizes from the *_ws_bytes / *_rows / *_elems queries) and a hipStream_t; work is stream-ordered.
 *   - activations are NHWC ([B][H][W][C]); network inputs (first conv) are NCHW as the reference's DataLoader
 *     yields them; 1-channel maps are identical in both layouts; weights keep the reference layout (Cout,Cin,3,3).
 *   - every function returns 0 on success or a non-zero hipError_t-style code; egz_last_error() returns the message
 *     of the calling thread's last failure (the Python shim raises EgazeHipError / RuntimeError, matching the
 *     reference's exception-based error behaviour, e.g. utils.py:151-152, extractLSTMw.py:111).
 *   - reentrant per stream; one process per GPU (no cross-device state).
 */
#ifndef EGAZE_HIP_H
#define EGAZE_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* hipStream_t;

const char* egz_version(void);
const char* egz_last_error(void);

/* ---- nn.Conv2d(Cin, Cout, 3, padding=1): utils.py:70 (encoders), models/model_SP.py:10,13-29 (fusion Conv3d
 *      k=(1,3,3) == the same 3x3 conv on each stream; decoder), models/late_fusion.py:10-12.
 *      Implicit GEMM on v_mfma_f32_32x32x2_f32.  Weights are re-packed on the device first:
 *      fwd  : wp[tap][Cout_pad][Cin_pad]         dgrad: wp[8-tap][Cin_pad][Cout_pad]   (pad = round up to 32, zeros;
 *      one reduction-index-contiguous row per output channel of the GEMM -- private layout, may change) */
size_t egz_pack_w3x3_elems(int C, int K, int kind /* 0: fwd / dgrad, 1: ups_fwd / ups_dgrad */);
int egz_pack_w3x3_fwd(const float* w, float* wp, int C, int K, hipStream_t stream);
int egz_pack_w3x3_dgrad(const float* w, float* wp, int C, int K, hipStream_t stream);
/* nn.Upsample(scale_factor=2) followed by the conv (models/model_SP.py:16-17,20-21,24-25,27-28): per output phase the
 * 3x3 taps collapse to 2x2 pre-summed taps on the low-res input (4/9 of the MACs); ups_dgrad is its transpose. */
int egz_pack_w3x3_ups_fwd(const float* w, float* wp, int C, int K, hipStream_t stream);
int egz_pack_w3x3_ups_dgrad(const float* w, float* wp, int C, int K, hipStream_t stream);
/* rows of the BatchNorm statistic partials written by the stats epilogue: stat_partial is [rows][2][K] fp64 */
int egz_conv3x3_stat_rows(int B, int H, int W, int K, int flags);
/* y[B][H][W][K] = conv3x3(x) + bias.  H, W are OUTPUT dims.  flags: bit0 = x is [B][H/2][W/2][C] and is nearest-x2
 * upsampled on the fly (nn.Upsample(scale_factor=2), models/model_SP.py:16,20,24,27); bit1 (with bit0) = use the
 * phase-decomposed form (weights from egz_pack_w3x3_ups_fwd); bits 4-5 epilogue: 0 bias,
 * 1 bias+ReLU, 2 bias + per-channel (sum, sumsq) partials for train-mode BatchNorm; 0x100 / 0x200 / 0x400 force the
 * 128x64 / 128x128 / 64x64 tile (same flags must be given to egz_conv3x3_stat_rows).  Called with dgrad-packed weights (and K = Cin) it computes the data gradient. */
int egz_conv3x3_fwd(const float* x, const float* wp, const float* bias, float* y, double* stat_partial, int B, int H,
                    int W, int C, int K, int flags, hipStream_t stream);
/* data gradient of [upsample x2 -> conv] w.r.t. the low-res input: dy [B][H][W][K] -> dx [B][H/2][W/2][C] */
int egz_conv3x3_ups_dgrad(const float* dy, const float* wp, float* dx, int B, int H, int W, int C, int K, int flags,
                          hipStream_t stream);
/* Error-compensated split-half variant for the wide layers (Cout % 128 == 0, Cin % 32 == 0): operands as hi + lo in a
 * 16-bit type, a*b ~= hi*hi + hi*lo + lo*hi accumulated in fp32 on v_mfma_f32_32x32x16_{f16,bf16} (16x the exact-f32
 * MFMA rate, 3 instructions per product).  dtype 1 = f16 x3 (weights pre-scaled 2^10; err ~3e-7 = fp32 class),
 * 2 = bf16 x3 (fp32 exponent range, err ~5e-6; used for gradients).  kind: 0 fwd, 1 dgrad, 2 ups_fwd, 3 ups_dgrad.
 * egz_conv3x3_fwd_split: flags as egz_conv3x3_fwd (bits 0-1, 4-5) plus bit2 = the 16-tap data gradient of an
 * upsampled conv (then C / K are the GEMM's reduction / output channel counts). */
int egz_pack_w3x3_split(const float* w, void* wp, int C, int K, int kind, int dtype, hipStream_t stream);
/* Optional tile schedule of egz_conv3x3_fwd_split (flags bit 14 = 0x4000): tiles beyond the last full round of resident
 * blocks are run split-K through `workspace` (raw partial accumulators) and reduced in a fixed order;
 * egz_conv3x3_fwd_split_ws_bytes gives the workspace size (0 without the flag: workspace may then be NULL). */
size_t egz_conv3x3_fwd_split_ws_bytes(int B, int H, int W, int C, int K, int flags);
int egz_conv3x3_fwd_split(const float* x, const void* wp, const float* bias, float* y, double* stat_partial, int B,
                          int H, int W, int C, int K, int flags, int dtype, void* workspace, size_t ws_bytes,
                          const unsigned int* x_absmax, unsigned int* absmax_out, hipStream_t stream);
/* absmax_out (optional; bias + ReLU epilogue, forward forms): receives max |y| in the egz_absmax layout -- the f16 x3
 * scaling of the convolution that consumes y (per-block partials from the epilogue + one fold launch, no extra pass over y
 * for launches of at most 16384 blocks).
 * Streamed-weight form of the plain split-half conv (csrc/conv3x3_igemm_x3s.hip): the weights are packed in MFMA
 * fragment order (kind 4 = forward, 5 = data gradient of the same nn.Conv2d: utils.py:66, models/model_SP.py:13-29) and go
 * L2 -> registers, the activation halo goes through LDS.  egz_conv3x3_streamed_ok: 1 when a geometry is covered
 * (C = reduction channels % 32 == 0, K = GEMM columns % 64 == 0).  mode 0 = plain conv; mode 1 = data gradient of
 * [nn.Upsample(x2) -> nn.Conv2d] (models/model_SP.py:17-18,22-23,25-26,28-29) w.r.t. the low-res input, x = hi-res dy,
 * kind-6 packing; mode 2 = the FORWARD of [nn.Upsample(x2) -> nn.Conv2d] as four 2 x 2-tap phase convolutions over the
 * low-res input (x = [B][H/2][W/2][C], y = [B][H][W][K], H x W passed = the hi-res output, kind-7 packing =
 * [phase][channel block][pre-summed tap], f16 x3 only, epi 0 / 1, K % 64 == 0).  epi: 0 bias, 1 bias + ReLU, 2 bias + BN partials (egz_conv3x3_streamed_stat_rows rows), 3 = data gradient
 * masked by mask_src > 0 with per-channel sums and per-tile abs-max (see below). */
int egz_conv3x3_streamed_ok(int B, int H, int W, int C, int K, int mode);
/* rows of stat_partial ([rows][2][K] doubles) of an epi 2 / epi 5 launch of egz_conv3x3_fwd_streamed (mode 0) */
int egz_conv3x3_streamed_stat_rows(int B, int H, int W, int C, int K);
int egz_pack_w3x3_split_frag(const float* w, void* wq, int C, int K, int kind, int dtype, hipStream_t stream);
/* Every fragment-ordered packing an optimizer step made stale in ONE launch (no reference counterpart: the reference's
 * Conv2d reads its fp32 weights directly, utils.py:70; this is the repack after optim.Adam.step, SP.py:137).  table: n rows of
 * 8 x int64 in DEVICE memory [w, wq, C, K, kind 4..7, dtype 1 f16 / 2 bf16, first block, unused]; first block = running sum of
 * egz_pack_w3x3_frag_blocks(C, K) over the preceding rows, total_blocks = the sum over all rows.  Bit-identical to n calls of
 * egz_pack_w3x3_split_frag. */
int egz_pack_w3x3_frag_blocks(int C, int K);
int egz_pack_w3x3_frag_batch(const long long* table, int n, int total_blocks, hipStream_t stream);
int egz_conv3x3_fwd_streamed(const float* x, const void* wq, const float* bias, float* y, double* stat_partial, int B,
                             int H, int W, int C, int K, int epi, int dtype, int mode, const unsigned int* x_absmax,
                             const float* mask_src, unsigned int* absmax_out, const float* bn_coef, float* minmax_out,
                             hipStream_t stream);
/* dtype | 0x10 (with dtype 1, f16 split halves; the wide tiles K % 32 == 0 of modes 0 and 1): TWO MFMA products per MAC instead of
 * three -- x_hi w_hi + x_hi w_lo: the x operand (the halo image that goes through LDS; dy in a data gradient) enters with its f16 hi
 * half only, rounded to nearest from the fp32 value or from hi + lo of a pre-split pair, the packed weights keep their 22 bits.
 * Meant for the data gradients (autograd of utils.py:70, models/model_SP.py:13-29): the result moves by ~2e-4 relative L2
 * (tests/test_hip_ops.py::test_backward_two_products).  Honoured by the narrow (late-fusion) kernel for epi 0 and 5 too; ignored by
 * egz_conv3x3_fwd_streamed_splitk, which stays on three products. */
/* Deferred BatchNorm (narrow geometry, epi 0 / 1 / 2): with bn_coef != NULL, x is the PRE-BatchNorm conv output of the block
 * below and bn_coef that BatchNorm's 4 x C coefficient rows; relu(x * scale + shift) is applied while the halo is staged, so
 * the normalised tensor of late_fusion.py:11-12 is never materialised (x_absmax = its max, from egz_bn_finalize_deferred).
 * minmax_out (epi 2, narrow geometry): [egz_conv3x3_streamed_stat_rows][2][K] per-channel max / min of y. */
/* epi 5 (mode 0, no bias; the narrow geometry C, K <= 32 with H and W multiples of 16, or K % 64 == 0): data gradient w.r.t. the
 * output of a train-mode [BatchNorm2d -> ReLU] (late_fusion.py:10-12; the conv -> BN -> ReLU -> conv pairs of the VGG
 * encoders, utils.py:64-76) that ALSO accumulates that BatchNorm's backward sums: mask_src =
 * the layer's pre-BN conv output (layout of y), bn_coef = 4 rows of K floats (batch mean, 1/std, scale, shift);
 * stat_partial receives egz_conv3x3_streamed_stat_rows rows of (sum dz, sum dz * xhat) with dz = (mask_src * scale + shift > 0) ? y : 0,
 * the `sums` argument of egz_bn_relu_pool_bwd.
 * epi 1 (bias + ReLU) with absmax_out != NULL (K % 64 == 0, at most 16384 tiles): absmax_out receives max |y|, folded.
 * Split-K form of a plain egz_conv3x3_fwd_streamed launch for small pixel counts (batch-1 inference as in
 * run_spatialstream.py:85-138 / AT.py:216, the 14 x 14 layers at the reference's default --batch_size_sp 8): the channel
 * blocks of a tile are divided over nsplit blocks (raw partial sums in the workspace, nsplit x B x H x W x K floats) and a
 * fix-up launch sums them in split order and applies the epilogue (epi 0 / 1 / 2).  egz_conv3x3_streamed_splits recommends
 * the split count; 1 = use egz_conv3x3_fwd_streamed.  K % 128 == 0, C % 32 == 0. */
int egz_conv3x3_streamed_splits(int B, int H, int W, int C, int K);
int egz_conv3x3_fwd_streamed_splitk_stat_rows(int B, int H, int W);   /* rows of stat_partial for epi 2 (one per 32 pixels) */
size_t egz_conv3x3_fwd_streamed_splitk_ws_bytes(int B, int H, int W, int K, int nsplit);
int egz_conv3x3_fwd_streamed_splitk(const float* x, const void* wq, const float* bias, float* y, double* stat_partial, int B,
                                    int H, int W, int C, int K, int epi, int dtype, const unsigned int* x_absmax,
                                    void* workspace, size_t ws_bytes, int nsplit, unsigned int* absmax_out,
                                    hipStream_t stream);
/* helpers of the epi = 3 (ReLU mask + bias-gradient sums + abs-max) form of egz_conv3x3_fwd_streamed, which folds the
 * nn.ReLU backward of a decoder layer (models/model_SP.py:13-29) into the data gradient of the layer above it */
int egz_colsum_f64(const double* part, int rows, int cols, int ncols_out, float* out, void* workspace, size_t ws_bytes,
                   hipStream_t stream);
/* dw (K,C,3,3) = sum_pixels dy (x) x   (autograd of the same conv; loss.backward() at SP.py:136, LF.py:99) */
size_t egz_conv3x3_wgrad_ws_bytes(int B, int H, int W, int C, int K, int flags);
int egz_conv3x3_wgrad(const float* x, const float* dy, float* dw, int B, int H, int W, int C, int K, int flags,
                      void* workspace, size_t ws_bytes, const unsigned int* dy_absmax, const unsigned int* x_absmax,
                      const float* x_bn, hipStream_t stream);
/* flags (both entry points; the size query reads only those that choose the kernel):
 *   1        the conv input was the nearest-x2 upsampling of x ([B][H/2][W/2][C]; H, W even)
 *   0x2000   split-half arithmetic on the 16-bit MFMA path where a split-half kernel covers the geometry and both operands
 *            are below 4 GiB (else exact f32): bf16 x3 when dy_absmax is NULL, f16 x3 with dy scaled by its abs-max when it is
 *            given; x_absmax (optional, f16 x3 only): max |x|, x is scaled the same way
 *   0x8000 / 0x10000   x / dy holds pre-split pairs (see egz_conv3x3_wgrad_presplit_ok below)
 *   0x20000  with 0x2000 and dy_absmax (f16 split halves; wide kernels: C and K multiples of 32 / 64): TWO MFMA products
 *            per MAC -- x_hi dy_hi + x_hi dy_lo: x enters with 11 significant bits, rounded to nearest (from the fp32 value, or
 *            from hi + lo of a pre-split pair), dy keeps 22; dw moves by ~2e-4 relative L2.  Also on the narrow (late-fusion)
 *            kernels; ignored by the bf16 and exact-f32 launches.
 *   A/B benchmarking: 0x100 per-tap kernel on 64 tiles where it would take 128, 0x800 force the per-tap kernel, 0x1000 the
 *            folded 9-tap form of an upsampled conv in place of its phase form, 0x4000 K = 4 / 8 on the narrow kernel keep
 *            the nine-tile form */
/* x_bn (optional): x is the PRE-BatchNorm conv output of the block below and x_bn that BatchNorm's 4 x C coefficient rows;
 * relu(x * scale + shift) is applied while x is staged (deferred BatchNorm, late_fusion.py:11-12), x_absmax = the max of the
 * normalised values.  Only where egz_conv3x3_wgrad_narrow_ok(B, H, W, C, K) (C, K <= 32, W % 16 == 0, flags 0x2000). */
int egz_conv3x3_wgrad_narrow_ok(int B, int H, int W, int C, int K);
/* Pre-split activations (round 5; the x operand of the encoder convolutions, utils.py:64-76).  The [BatchNorm -> ReLU (-> pool)]
 * pass that writes a block output can store it as f16 hi / lo PAIRS instead of fp32 -- per 4-channel quad the 16 bytes
 * [4 hi halves | 4 lo halves] of (value * 2^s), s from the tensor's exact abs-max, the very pair the split-half kernels
 * would form while staging the fp32 value (same footprint, bit-identical products).  Consumers: egz_conv3x3_fwd_streamed with
 * mode | 0x100 (mode 0, dtype 1, epi 2, K % 64 == 0, C % 32 == 0, x_absmax = the abs-max the pairs were scaled with) and
 * egz_conv3x3_wgrad with flags | 0x8000 where egz_conv3x3_wgrad_presplit_ok(B, H, W, C, K) (C, K multiples of 64, the
 * split-half 9-tap kernel's geometry; flags 0x2000, dy_absmax and x_absmax given, plain conv).  Producer chain:
 * egz_conv3x3_fwd_streamed(epi 2, K % 64 == 0, K <= 512, minmax_out = 1024 zero-filled uints: 1024 / (2 K) sets of order-preserving
 * images of the per-channel max of y and of -y) -> egz_bn_finalize_bound -> egz_bn_relu_pool_fwd_presplit. */
int egz_conv3x3_wgrad_presplit_ok(int B, int H, int W, int C, int K);

/* ---- first conv of a stack, small Cin, NCHW input: Conv2d(3,64) / Conv2d(20,64) (utils.py:70 at SP.py:53, inputs
 *      per data/STdatas.py:50-73) and Conv2d(2,32) (models/late_fusion.py:10).  K in {64, 32}. */
int egz_conv_first_stat_rows(int B, int H, int W);
int egz_conv_first_stat_rows_for(int B, int H, int W, int C, int K);   /* rows of stat_partial egz_conv_first_fwd writes for C -> K
                                                                        * (C <= 3: the direct kernel, one row per block) */
int egz_conv_first_fwd(const float* x_nchw, const float* w, const float* bias, float* y_nhwc, double* stat_partial,
                       int B, int H, int W, int C, int K, float* minmax_out, unsigned int* minmax_ordered, hipStream_t stream);
/* minmax_out (optional; C <= 3 with stat_partial): [rows][2][K] per-channel max / min of y, rows as
 * stat_partial -- input of egz_bn_finalize_deferred.  minmax_ordered (optional, same conditions): 1024 zero-filled uints (the first 2 K are written), the
 * atomic-max form egz_bn_finalize_bound reads (see egz_conv3x3_wgrad_presplit_ok). */
size_t egz_conv_first_wgrad_ws_bytes(int B, int H, int W, int C);
int egz_conv_first_wgrad(const float* x_nchw, const float* dy_nhwc, float* dw, int B, int H, int W, int C, int K,
                         void* workspace, size_t ws_bytes, hipStream_t stream);

/* ---- nn.BatchNorm2d (train: batch statistics + running-stat update with unbiased variance; eval: affine) fused with
 *      the nn.ReLU and optional nn.MaxPool2d(2,2) that follow it (utils.py:68,72; models/model_SP.py:12,45-47;
 *      models/late_fusion.py:10-12).  mean/invstd/scale/shift are [K] outputs kept for the backward pass. */
size_t egz_bn_ws_bytes(int K);
int egz_bn_finalize(const double* stat_partial, int rows, int K, double count, const float* gamma, const float* beta,
                    float* running_mean, float* running_var, float momentum, float eps, float* mean_out,
                    float* invstd_out, float* scale, float* shift, long long* num_batches_tracked, void* workspace,
                    size_t ws_bytes, hipStream_t stream);
/* The same for a BatchNorm whose output is never materialised -- the convolution above it applies relu(y * scale + shift) while
 * staging y (egz_conv3x3_fwd_streamed bn_coef; late_fusion.py:11-12).  minmax: [mm_rows][2][K] per-channel max / min rows of y
 * from the producing conv; absmax_out (egz_absmax layout) receives the exact max of the normalised + ReLU'd values, the f16
 * split scale of that convolution.  K in {16, 32, 64}; one launch, no workspace. */
int egz_bn_finalize_deferred(const double* stat_partial, int rows, int K, double count, const float* gamma, const float* beta,
                             float* running_mean, float* running_var, float momentum, float eps, float* mean_out,
                             float* invstd_out, float* scale, float* shift, long long* num_batches_tracked,
                             const float* minmax, int mm_rows, unsigned int* absmax_out, hipStream_t stream);
/* egz_bn_finalize that also bounds the block output: minmax as written by egz_conv3x3_fwd_streamed on the 64- / 128-column tiles
 * (1024 uints), absmax_out (egz_absmax layout, zero-filled by the caller) receives the EXACT max of relu(y * scale + shift)
 * (the map is monotonic in y per channel).  K % 64 == 0. */
int egz_bn_finalize_bound(const double* stat_partial, int rows, int K, double count, const float* gamma, const float* beta,
                          float* running_mean, float* running_var, float momentum, float eps, float* mean_out,
                          float* invstd_out, float* scale, float* shift, long long* num_batches_tracked, void* workspace,
                          size_t ws_bytes, const unsigned int* minmax, unsigned int* absmax_out, hipStream_t stream);
int egz_bn_eval_coeffs(int K, const float* gamma, const float* beta, const float* running_mean,
                       const float* running_var, float eps, float* scale, float* shift, hipStream_t stream);
/* egz_bn_relu_pool_fwd with the output stored pre-split (see egz_conv3x3_wgrad_presplit_ok): absmax is an INPUT, the exact max of
 * the output from egz_bn_finalize_bound. */
int egz_bn_relu_pool_fwd_presplit(const float* y, const float* scale, const float* shift, float* out, int B, int H, int W,
                                  int K, int pool, const unsigned int* absmax, hipStream_t stream);
int egz_bn_relu_pool_fwd(const float* y, const float* scale, const float* shift, float* out, int B, int H, int W,
                         int K, int pool, unsigned int* absmax, hipStream_t stream);   /* absmax: optional, max |out| */
size_t egz_bn_relu_pool_bwd_ws_bytes(int K);
int egz_bn_relu_pool_bwd(const float* y, const float* dout, const float* scale, const float* shift, const float* mean,
                         const float* invstd, float* dy, float* dgamma, float* dbeta, int B, int H, int W, int K,
                         int pool, void* workspace, size_t ws_bytes, unsigned int* absmax, const double* sums,
                         int sums_rows, hipStream_t stream);
/* The same with dy stored PRE-SPLIT (f16 hi / lo pairs; see egz_conv3x3_wgrad_presplit_ok): scaled by a BOUND of max |dy| that the
 * finalize step derives before the apply pass runs from y_minmax (the 1024 uints of egz_conv3x3_fwd_streamed's minmax_out for y),
 * dout_absmax (max |dout|, egz_absmax layout: egz_conv3x3_fwd_streamed's absmax_out of the data gradient that produced dout)
 * and the two per-channel sums; the bound is left in `absmax` (zero-filled by the caller) and is dy's abs-max for its consumers
 * (egz_conv3x3_fwd_streamed mode | 0x100 with epi 0 / 5, egz_conv3x3_wgrad flags | 0x10000).  K % 64 == 0, K <= 512. */
int egz_bn_relu_pool_bwd_presplit(const float* y, const float* dout, const float* scale, const float* shift, const float* mean,
                                  const float* invstd, float* dy, float* dgamma, float* dbeta, int B, int H, int W, int K,
                                  int pool, void* workspace, size_t ws_bytes, unsigned int* absmax, const double* sums,
                                  int sums_rows, const unsigned int* y_minmax, const unsigned int* dout_absmax,
                                  hipStream_t stream);
/* Backward of a FIRST block [Conv2d(C -> K, 3x3) -> BatchNorm2d(train) -> ReLU] with C <= 3 and K = 32 (late_fusion.py:10-12)
 * or 64 (the RGB encoder, utils.py:70 at SP.py:53; the network input needs no data gradient): dgamma / dbeta and dw (K, C, 3, 3) in one pass
 * over y (pre-BN conv output, NHWC) and dout, x = the block input [B][C][H][W]; the gradient w.r.t. the conv output is never
 * stored.  sums / sums_rows as for egz_bn_relu_pool_bwd. */
size_t egz_bn_bwd_first_wgrad_ws_bytes(int C, int K);
int egz_bn_bwd_first_wgrad(const float* y, const float* dout, const float* scale, const float* shift, const float* mean,
                           const float* invstd, const float* x, float* dw, float* dgamma, float* dbeta, int B, int H, int W,
                           int C, int K, void* workspace, size_t ws_bytes, const double* sums, int sums_rows,
                           hipStream_t stream);
/* sums (optional, pool = 0): [sums_rows][2][K] partial rows of (sum dz, sum dz * xhat) produced together with dout by
 * egz_conv3x3_fwd_streamed epi 5 -- the reduce pass over y and dout is skipped.
 * `absmax` of the three gradient producers (egz_bn_relu_pool_bwd, egz_pairmax_bwd, egz_relu_bwd_bias; optional): a buffer of
 * egz_absmax_elems() uints that the CALLER ZERO-FILLS before the producing call (true for every `absmax` / `absmax_out`
 * argument of this header except egz_absmax's, which zero-fills its own).  Layout: 32 slots, one per 128-byte line, each the
 * bit pattern of a non-negative float; a producing block folds its maximum into one slot with at most one device-scope atomic
 * max (max is exact and order independent: deterministic), a consumer (`x_absmax`, `dy_absmax`, `a_absmax` arguments) takes
 * the maximum of the slots at the top of its kernel -- no fold launch between producer and consumer.  It is the scale source
 * of the f16 x3 split-half forward / data / weight gradients; egz_absmax computes it for a bare tensor (n % 4 == 0). */
int egz_absmax_elems(void);
int egz_absmax(const float* x, long n, unsigned int* absmax, hipStream_t stream);

/* ---- nn.MaxPool3d((2,1,1)) over the depth-2 stack == element-wise max of the two streams (model_SP.py:11,43);
 *      y2 = [2][n] (stream s, then t), the first stream wins ties like torch's pooling scan. */
int egz_pairmax_fwd(const float* y2, float* z, long n, hipStream_t stream);
int egz_pairmax_bwd(const float* y2, const float* dz, float* dy2, long n, unsigned int* absmax, hipStream_t stream);
/* per-channel (sum, sumsq) partials of an NHWC tensor, in the conv-epilogue format ([rows][2][K] fp64) */
int egz_channel_stats_rows(void);
int egz_channel_stats(const float* x, long rows, int K, double* stat_partial, hipStream_t stream);

/* ---- nn.ReLU backward (decoder, models/model_SP.py:13-29), optionally fused with the conv bias gradient;
 *      nn.Upsample(scale_factor=2) backward (2x2 sum); column sums; NCHW <-> NHWC transposes. */
int egz_relu_bwd(const float* out, const float* dout, float* dy, long n, hipStream_t stream);
size_t egz_relu_bwd_bias_ws_bytes(int K);
int egz_relu_bwd_bias(const float* out, const float* dout, float* dy, float* db, long rows, int K, void* workspace,
                      size_t ws_bytes, unsigned int* absmax, hipStream_t stream);
int egz_upsample2x_bwd(const float* dxu, float* dx, int B, int H, int W, int C, hipStream_t stream);
int egz_colsum(const float* x, long rows, int K, float* out, void* workspace, size_t ws_bytes, hipStream_t stream);
int egz_nchw_to_nhwc(const float* in, float* out, int B, int C, int H, int W, hipStream_t stream);
/* the same transpose with the channel dimension zero-padded to Cp (the 20-channel flow stack -> 32 channels so that the
 * temporal encoder's first conv, SP.py:53, runs on the split-half kernels) */
int egz_nchw_to_nhwc_pad(const float* in, float* out, int B, int C, int H, int W, int Cp, hipStream_t stream);
int egz_nhwc_to_nchw(const float* in, float* out, int B, int C, int H, int W, hipStream_t stream);
/* stream-ordered device copy of n floats / zero fill of `bytes` bytes: torch.cat of the two encoder maps
 * (models/model_SP.py:39) when they do not already share a buffer; optimizer.zero_grad() (SP.py:138) */
int egz_copy(const float* src, float* dst, long n, hipStream_t stream);
int egz_fill_zero(void* dst, size_t bytes, hipStream_t stream);

/* ---- nn.Conv2d(C, 1, 1) + nn.Sigmoid head (models/model_SP.py:30,32,49; models/late_fusion.py:13,15,22) */
int egz_conv1x1_sigmoid_fwd(const float* x, const float* w, const float* bias, float* out, float* logits, long M,
                            int C, hipStream_t stream);
size_t egz_conv1x1_sigmoid_bwd_ws_bytes(int C);
int egz_conv1x1_sigmoid_bwd(const float* x, const float* w, const float* out, const float* dout, float* dx, float* dw,
                            float* db, long M, int C, void* workspace, size_t ws_bytes, hipStream_t stream);
/* The same with the ReLU backward of the block below folded in, for `Conv2d 3x3 -> ReLU -> Conv2d 1x1 -> Sigmoid`
 * (models/model_SP.py:28-32): x is that block's post-ReLU output, dx = (x > 0) ? dlogit * w : 0.  mstat: fp64 partial rows
 * [egz_conv1x1_sigmoid_bwd_rows(M, C)][C] whose column sums (egz_colsum_f64) are the 3x3 conv's bias gradient; absmax: an
 * egz_absmax_elems() buffer, slot 0 = max |dx| on return.  Replaces the autograd ReLU-backward pass between the two convs. */
int egz_conv1x1_sigmoid_bwd_rows(long M, int C);
int egz_conv1x1_sigmoid_bwd_masked(const float* x, const float* w, const float* out, const float* dout, float* dx, float* dw,
                                   float* db, double* mstat, unsigned int* absmax, long M, int C, void* workspace,
                                   size_t ws_bytes, hipStream_t stream);

/* ---- floss.forward / build_weight_from_target (floss.py:9-41): W = width / (||p - centroid(argmax set)|| + 1),
 *      F.binary_cross_entropy(input, target, W) with torch's -100 log clamp, mean reduction.  weighted = 0 gives
 *      torch.nn.BCELoss() (SP.py:103-106).  Backward follows aten: w*(x-t)/max((1-x)x, 1e-12)/N.
 *      nn.MSELoss (AT.py:83,138) likewise.  loss_out / grad_out are device scalars. */
size_t egz_loss_ws_bytes(int B);
int egz_floss_fwd(const float* inp, const float* target, float* weights_out, float* loss_out, int B, int H, int W,
                  int weighted, void* workspace, size_t ws_bytes, hipStream_t stream);
int egz_floss_bwd(const float* inp, const float* target, const float* weights, const float* grad_out, float* dinp,
                  long n, hipStream_t stream);
/* nn.MSELoss (AT.py:83); tanh_b != 0: the target is tanh(b), i.e. `criterion(pred, tanh(target))` of AT.py:138 in one pass */
int egz_mse_fwd(const float* a, const float* b, float* loss_out, long n, void* workspace, size_t ws_bytes, int tanh_b,
                hipStream_t stream);
int egz_mse_bwd(const float* a, const float* b, const float* grad_out, float* da, long n, int tanh_b, hipStream_t stream);
/* nn.MSELoss + its gradient for a unit seed in ONE single-block launch, n <= 4096 (AT.py:138-141 on one (1, 1, 512) sample);
 * bit-identical to egz_mse_fwd + egz_mse_bwd(grad_out = 1).  ring (optional): the loss is also parked in ring[counter[0] % ring_n]. */
int egz_mse_fwd_grad(const float* a, const float* b, float* loss_out, float* da, long n, int tanh_b, float* ring, int ring_n,
                     const int* counter, hipStream_t stream);

/* ---- AT: nn.LSTM(512,512,2) + nn.Linear + tanh (models/LSTMnet.py:18-37) from a strided f32-MFMA GEMM and fused
 *      cell kernels.  egz_gemm: C[M][N] (row stride ldc) = op(A) op(B) (+C if flags&1) (+bias[n]) (ReLU if flags&2),
 *      op(A)(m,k) = A[m*sam + k*sak], op(B)(k,n) = B[k*sbk + n*sbn].  Gate order i,f,g,o. */
int egz_gemm(const float* A, const float* B, float* C, const float* bias, int M, int N, int K, long sam, long sak,
             long sbk, long sbn, long ldc, int flags, hipStream_t stream);
/* count <= 8 products of ONE shape and stride set in one launch (blockIdx.z picks the operands): the weight-gradient products
 * dgates^T [x | h_prev] of nn.LSTM's backward (models/LSTMnet.py:18 under autograd).  A, B, C: HOST arrays of `count` device
 * pointers; flags bit 0 = accumulate; no bias, no ReLU.  Outside egz_gemm's fast-path geometry: `count` egz_gemm calls. */
int egz_gemm_batched(const float* const* A, const float* const* B, float* const* C, int count, int M, int N, int K, long sam,
                     long sak, long sbk, long sbn, long ldc, int flags, hipStream_t stream);
int egz_lstm_cell_fwd(const float* gates, const float* c_prev, float* h_out, float* c_out, float* act, int B, int Hd,
                      hipStream_t stream);
int egz_lstm_cell_bwd(const float* act, const float* c, const float* c_prev, const float* dh, const float* dc_in,
                      float* dgates, float* dc_prev, int B, int Hd, hipStream_t stream);
/* nn.LSTM(H, H, num_layers = L) as a wavefront over (layer, step) (models/LSTMnet.py:18,26-35: self.lstm(input, hidden)): launch
 * s runs step s - l of every layer l, T + L - 1 dependent launches instead of T x L, the upper layers' input projections reduced
 * in the same launch (K = 2H).  w_ih / w_hh / bsum: HOST arrays of L device pointers ([4H][H], [4H][H], [4H] = b_ih + b_hh;
 * w_ih[0] / bsum[0] unused: gx0 [T][B][4H] = x W_ih0^T + b_ih0 + b_hh0 for every step); h0, c0, hn, cn: [L][B][H];
 * hs: [L][T + 1][B][H] (slot 0 of a layer = a copy of its h0, slots 1 .. T = the outputs); cs: [L][T][B][H]; acts: [L][T][B][4H]
 * or null.  1 <= L <= 4, H % 256 == 0. */
int egz_lstm_wave_fwd(const float* gx0, const float* const* w_ih, const float* const* w_hh, const float* const* bsum,
                      const float* h0, const float* c0, float* hs, float* cs, float* acts, float* hn, float* cn, int L, int T,
                      int B, int H, hipStream_t stream);
/* The same forward recurrence for the AT network's own geometry (L = 2, H = 512, B <= 32) as ONE persistent, weight-stationary
 * launch: each of 128 x ceil(B / 16) blocks keeps its 16 x 1536 weights in registers for the whole sequence and the blocks hand
 * h_t to each other inside the launch (write-through stores + arrival counters, csrc/lstm_seq.hip).  Outputs as
 * egz_lstm_wave_fwd; inputs differ in two places: gx0 = x W_ih0^T WITHOUT bias, and b_ih / b_hh = HOST arrays of L device pointers
 * to the module's own bias vectors ([4H] each), summed inside the kernel.  `sync`: egz_lstm_persist_sync_words() uints of device
 * scratch (its counters are zeroed by the call); after the launch word [1024] is 0, or 1 + s when a block gave up waiting in
 * global step s (0.5 s of wall clock without progress; outputs then NaN from that step on).  The LAST 32 words of the scratch are
 * sticky: a call writes them only on such a time-out (word 0: forward launches, word 1: backward launches; atomic max of 1 + s) and
 * never clears them -- zero the scratch once when allocating it, keep it across calls, read the two words wherever the host
 * synchronises anyway.  Any other geometry (or T * B beyond the 32-bit offsets of this form): returns hipErrorNotSupported (801)
 * and launches nothing -- call egz_lstm_wave_fwd. */
int egz_lstm_persist_sync_words(void);
int egz_lstm_persist_fwd(const float* gx0, const float* const* w_ih, const float* const* w_hh, const float* const* b_ih,
                         const float* const* b_hh, const float* h0, const float* c0, float* hs, float* cs, float* acts, float* hn,
                         float* cn, unsigned int* sync, int L, int T, int B, int H, hipStream_t stream);
/* Its backward through time (autograd of the same call): T + 2 L - 1 launches of uniform K = 4H blocks; the gradient a lower layer
 * receives from the layer above (dgates_above,t W_ih_above) is formed by blocks of its own one launch ahead of the cell backward
 * that consumes it and parked in dhin.  dh_top: [T][B][H] or null; dhn, dcn: [L][B][H] or null; w_hh_t / w_ih_t: HOST arrays of L
 * device pointers to the TRANSPOSED weights [H][4H] (w_ih_t[0] unused); dgates: [L][T][B][4H] out; dh0, dc0: [L][B][H] out;
 * dhin: [L - 1][T][B][H] scratch (may be null at L = 1). */
int egz_lstm_wave_bwd(const float* dh_top, const float* dhn, const float* dcn, const float* acts, const float* cs,
                      const float* c0, const float* const* w_hh_t, const float* const* w_ih_t, float* dgates, float* dh0,
                      float* dc0, float* dhin, int L, int T, int B, int H, hipStream_t stream);
/* egz_lstm_wave_bwd for the AT network's own geometry (L = 2, H = 512, B <= 32) as ONE persistent launch: 64 x ceil(B / 8) blocks,
 * each keeping 8 units x 2048 of W_hh_l1^T, W_ih_l1^T, W_hh_l0^T in registers; the dgates of a step are handed over inside the
 * launch (csrc/lstm_seq.hip, lstm_persist_bwd_kernel).  Inputs and outputs as egz_lstm_wave_bwd without dhin, except: w_hh / w_ih
 * are the weights AS THE MODULE HOLDS THEM ([4H][H]; HOST arrays of L device pointers, w_ih[0] unused) -- no transposed copies --
 * and the launch also forms the bias gradients: db = HOST array of 2 L device pointers (b_ih_l0, b_hh_l0, b_ih_l1, b_hh_l1: [4H]
 * each = the sum of dgates_l over steps and batch rows; null entries skipped; db may be null).  `sync` as in
 * egz_lstm_persist_fwd.  Any other geometry: hipErrorNotSupported, nothing launched. */
int egz_lstm_persist_bwd(const float* dh_top, const float* dhn, const float* dcn, const float* acts, const float* cs,
                         const float* c0, const float* const* w_hh, const float* const* w_ih, float* dgates, float* dh0,
                         float* dc0, float* const* db, unsigned int* sync, int L, int T, int B, int H, hipStream_t stream);
/* The same network at T = 1, B = 1 -- the reference's own stepping (AT.py:127-145 training loop, AT.py:246 inference): the
 * whole step in ONE call (L + 1 launches forward, 2L + 1 backward; csrc/lstm_b1.hip).  params / grads: HOST arrays of
 * 4L + 2 device pointers in state-dict order (w_ih, w_hh, b_ih, b_hh per layer, lin.weight [N][H], lin.bias [N]); a null
 * grads entry skips that gradient.  inp [C] raw (tanh applied inside, saved to xt); h0, c0, hn, cn [L][H]; acts [L][4H]
 * (null in no-grad runs); out [N] after ReLU.  No gradient w.r.t. inp / h0 / c0 (the loop detaches them, AT.py:143). */
size_t egz_lstm_b1_ws_bytes(int L, int C, int H, int N);
int egz_lstm_b1_fwd(const void* const* params, int L, const float* inp, const float* h0, const float* c0, float* xt,
                    float* acts, float* hn, float* cn, float* out, int C, int H, int N, hipStream_t stream);
int egz_lstm_b1_bwd(const void* const* params, void* const* grads, int L, const float* dout, const float* dhn,
                    const float* dcn, const float* xt, const float* acts, const float* h0, const float* c0,
                    const float* hn, const float* cn, const float* out, int C, int H, int N, void* workspace,
                    size_t ws_bytes, hipStream_t stream);
int egz_tanh_fwd(const float* x, float* y, long n, hipStream_t stream);
int egz_tanh_bwd(const float* y, const float* dy, float* dx, long n, hipStream_t stream);
int egz_add(const float* a, const float* b, float* out, long n, hipStream_t stream);

/* ---- torch.optim.Adam step (defaults as configured at SP.py:110-113, AT.py:84, LF.py:77) over one flat buffer;
 *      grad_scale multiplies the gradient first (1/world_size after the RCCL sum all-reduce).
 *      nonfinite: device word (may be null; zeroed by its owner).  An element whose scaled gradient is NaN / inf is skipped (p, m, v
 *      keep their values) and bit 0 of *nonfinite is set -- torch.optim.Adam would write NaN into the weights there; every finite
 *      gradient gives torch's bits. */
int egz_adam_step(float* p, const float* g, float* m, float* v, long n, double lr, double beta1, double beta2,
                  double eps, int step, double grad_scale, unsigned int* nonfinite, hipStream_t stream);
/* the same step with the counter of COMPLETED steps on the device (applies step step[0] + 1, then increments step[0]): for
 * optimizer steps inside a captured hipGraph, where a replay cannot receive a new host scalar.  step -> TWO ints {completed
 * steps, reserved (0)} */
int egz_adam_step_dev(float* p, const float* g, float* m, float* v, long n, double lr, double beta1, double beta2,
                      double eps, int* step, double grad_scale, unsigned int* nonfinite, hipStream_t stream);

/* utils.computeAAEAUC (utils.py:96-140) per sample on the device: res (B,6) doubles = (AAE deg, fp = #{z > z[gp]}, gaze row,
 * gaze col, centroid row, centroid col); gw = the 2R+1 weights of scipy's gaussian kernel (sigma 14, R = 56),
 * dist = 112 / tan(pi/6).  224 x 224 maps only, like the reference.  Called by LF.trainLate / SP.testSP every batch
 * (LF.py:92-94, SP.py:170-174) instead of a device-to-host copy of both maps + 148 ms of scipy per 32 frames. */
int egz_aae_auc(const float* out, const float* gt, int B, int H, int W, const double* gw, int R, double dist,
                double* res, hipStream_t stream);

/* Dataset preparation (data/dataset_preprocessing.py, misc/gazedataset_gt.py): N ground-truth gaze maps rendered from N impulse
 * positions pos (N, 2) = (row, col) in [0, H) x [0, W): scipy.ndimage.gaussian_filter of the impulse (gw = the 2R + 1 weights
 * of scipy's 1-D kernel, R < min(H, W), 'reflect'), min-max normalised times 255, then OpenCV's INTER_AREA resize to oh x ow
 * from host-built tables (x / y: entries [ofs[d], ofs[d + 1]) of (source index, float32 alpha), nx / ny entries in all).
 * mode 0: double source and accumulation, out_u8 = round-half-even with saturation; mode 1: truncated uint8 source, float
 * accumulation.  out_f64 (nullable): (N, oh, ow) resized maps; out_full (nullable): (N, H, W) normalised maps.  fp64, no FMA
 * contraction: bit-identical with scipy + numpy at full resolution. */
int egz_gaze_gt_maps(const int* pos, int N, int H, int W, const double* gw, int R, const int* xofs, const int* xsi,
                     const float* xalpha, int nx, const int* yofs, const int* ysi, const float* yalpha, int ny, int mode,
                     int oh, int ow, unsigned char* out_u8, double* out_f64, double* out_full, hipStream_t stream);

/* Feature visualisation (vis_features.py, csrc/vis_overlay.hip).  OpenCV's INTER_LINEAR resize of N 8-bit images (C = 1 or 3,
 * planar (C, H, W) or interleaved (H, W, C)) from host-built 11-bit tables (hipops.linear_table): xofs[dw] clamped source
 * columns, xalpha[2 dw]; yofs[dh] unclamped source rows, yalpha[2 dh].  Integer arithmetic only, bit-identical with OpenCV's
 * fixed-point path.  The overlay chain resizes M maps (h x w) to H x W with the same tables, looks each value up in a 256 x 3 BGR
 * table and blends it over frame frame_index[m] of the (F, 3, H, W) BGR planes as rint(fl64(h * 0.3) + fl64(i * 0.5)) into
 * (M, H, W, 3) BGR bytes.  cell_argmax: per (H, W) byte map, the row-major index of the first maximal exact sum over the
 * (H / cell) x (W / cell) cells. */
int egz_resize_linear_u8(const unsigned char* src, int N, int C, int sh, int sw, int dh, int dw, int interleaved,
                         const int* xofs, const short* xalpha, const int* yofs, const short* yalpha, unsigned char* dst,
                         hipStream_t stream);
int egz_heatmap_overlay(const unsigned char* maps, int M, int h, int w, const int* frame_index, const unsigned char* frames,
                        int F, int H, int W, const unsigned char* lut, const int* xofs, const short* xalpha, const int* yofs,
                        const short* yalpha, unsigned char* out, hipStream_t stream);
int egz_cell_argmax_u8(const unsigned char* gt, int N, int H, int W, int cell, int* out, hipStream_t stream);

/* The AT -> LF hand-over on the device and the gaze marker of an overlay (predict.py, csrc/late_input.hip).
 * late_input: sp (B, H, W) and at (B, h, w) are fp32 maps, or uint8 planes where sp_u8 / at_u8 is non-zero.  An fp32 value is
 * quantised as q = trunc(fl32(255 x)) -- (255 * x).to(uint8) for x in [0, 1]; NaN or x < 0 gives 0 and 255 x >= 256 gives 255,
 * and *status (device, zero-filled by the caller) gets bit 0 (NaN) or bit 1 (out of range).  The AT plane is quantised at h x w
 * and resized to H x W with egz_resize_linear_u8's arithmetic and tables (all four null when (h, w) == (H, W): no resize).
 * fused (B, 2, H, W) fp32: channel 0 the AT plane, channel 1 the SP plane, every value (float)u8 / 255.f -- bit-identical
 * with egz_late_gather of the same planes; planes (B, 2, H, W) uint8, optional (null: not written), the same two planes.
 * fused stays below 4 GiB.  No allocation, no synchronisation.
 * late_store: the same two planes of n samples, quantised and resized by the same code, written into planes of late_pool
 * (P, H, W) uint8: dst (n, 3) int64 on the device names the planes that take sample i's SP plane, AT plane and ground truth;
 * -1 skips a plane (its map is then neither read nor flagged).  gt_pool (Q, H, W) uint8 and gt_src (n,) int64 go together:
 * plane dst[i, 2] takes a copy of plane gt_src[i] of gt_pool; both null: the third column of dst is not read.  A row with a
 * number outside [-1, P) in dst or outside [0, Q) in gt_src is never dereferenced, writes none of its planes and raises bit 2
 * of *status; bits 0 and 1 as late_input's.  The planes named in one call must be distinct.  No fp32 output.
 * draw_ring: images (M, H, W, 3) uint8 in place; pixel (y, x) of image m takes (c0, c1, c2) iff
 * r_in^2 <= (y - centers[2m])^2 + (x - centers[2m + 1])^2 <= r_out^2 (integers); centres may lie outside the image. */
int egz_late_input(const void* sp, int sp_u8, const void* at, int at_u8, int B, int H, int W, int h, int w, const int* xofs,
                   const short* xalpha, const int* yofs, const short* yalpha, float* fused, unsigned char* planes, int* status,
                   hipStream_t stream);
int egz_late_store(const void* sp, int sp_u8, const void* at, int at_u8, int n, int H, int W, int h, int w, const int* xofs,
                   const short* xalpha, const int* yofs, const short* yalpha, unsigned char* late_pool, long P, const long* dst,
                   const unsigned char* gt_pool, long Q, const long* gt_src, int* status, hipStream_t stream);
int egz_draw_ring(unsigned char* images, int M, int H, int W, const int* centers, int r_in, int r_out, int c0, int c1, int c2,
                  hipStream_t stream);

/* Baseline JPEG decode of N streams in one call (data/STdatas.STDataset(decode='gpu'), csrc/jpeg_decode.hip): stream i is
 * data[offsets[i], offsets[i + 1]) and is decoded into the channels[i] (1 or 3) uint8 planes of H x W starting at plane
 * planes[i] of out (out_planes planes in all), bit-identical with libjpeg-turbo's default decode (cv2.imread): BGR for colour,
 * the Y plane for a grayscale request of a colour file, replicated planes for a colour request of a grayscale file.
 * status[i]: 0 ok, 1 corrupt data in the scan (decoded with libjpeg's zero padding), 2 unsupported, 3 size differs from
 * H x W, 4 a file libjpeg refuses (bad header or table, no scan; cv2.imread returns None).  2 / 3 / 4 write nothing.  n3 = number of streams with channels 3,
 * ws = egz_jpeg_decode_ws_bytes(N, H, W, n3) bytes.  stages: 2 = full decode, 1 = header + entropy decode only (timing). */
size_t egz_jpeg_decode_ws_bytes(int N, int H, int W, int n3);
int egz_jpeg_decode(const unsigned char* data, long data_len, const long* offsets, const int* channels, const long* planes,
                    int N, int H, int W, unsigned char* out, long out_planes, int* status, void* ws, size_t ws_bytes,
                    int n3, int stages, hipStream_t stream);

/* Baseline JPEG encode of N images of one geometry (csrc/jpeg_encode.hip): images is uint8 (N, H, W) for C = 1 or interleaved
 * BGR (N, H, W, 3) for C = 3 (written as YCbCr 4:2:0); every file is byte-identical with libjpeg-turbo's default encoder at
 * that quality (Pillow's Image.save, cv2.imwrite): sequential Huffman, Annex K tables, no restart markers.  quality 1 .. 100,
 * subsampling 420 (the only one built; 444 / 422 are refused), 1 <= H, W <= 4096, N <= 65535.
 * egz_jpeg_encode transforms, entropy-codes into the workspace (egz_jpeg_encode_ws_bytes(N, H, W, C) bytes) and writes the
 * length every file needs to needed[N]; stages: 4 = all of that, 1 / 2 / 3 = stop after the transform / the bit-position
 * scan / the bit packing (timing; needed is not written).  egz_jpeg_encode_write, given the same workspace and geometry,
 * writes file i to out[slot_off[i], slot_off[i] + lengths[i]) with lengths[i] the length it needs and status[i] 0 -- or,
 * where lengths[i] > slot_cap[i] or the slot leaves out's out_bytes, writes nothing of it and sets status[i] 1. */
size_t egz_jpeg_encode_ws_bytes(int N, int H, int W, int C);
int egz_jpeg_encode(const unsigned char* images, int N, int H, int W, int C, int quality, int subsampling, void* ws,
                    size_t ws_bytes, long* needed, int stages, hipStream_t stream);
int egz_jpeg_encode_write(const void* ws, size_t ws_bytes, int N, int H, int W, int C, unsigned char* out, long out_bytes,
                          const long* slot_off, const long* slot_cap, long* lengths, int* status, hipStream_t stream);

/* The planes jpeg_decode gives for jpeg_encode's files, without the files (csrc/jpeg_roundtrip.hip): src is N grey planes of
 * H x W uint8, quality 1 .. 100, 1 <= H, W <= 4096, any N >= 1.  Per 8x8 block: FDCT, quantisation by the table
 * jpge::setup builds for that quality, dequantisation, IDCT, range limit -- bit-identical with egz_jpeg_encode followed by
 * egz_jpeg_decode, whose entropy coding is lossless.  Plane i is written to plane planes[i] of dst (dst_planes planes of
 * H x W; planes null: i).  status[i]: 0 ok, 1 planes[i] outside [0, dst_planes) -- nothing of that plane is written.  A
 * destination plane may be its own source plane (in place); any other overlap of src with a written plane is undefined.
 * One launch, no workspace, no host synchronisation. */
int egz_jpeg_roundtrip(const unsigned char* src, long N, int H, int W, int quality, const long* planes, unsigned char* dst,
                       long dst_planes, int* status, hipStream_t stream);

/* torch.cat((f, g), dim=1) of two one-channel maps, the late-fusion stack's input (models/late_fusion.py:19):
 * f, g [B][1][H][W] -> out [B][2][H][W]; 16-byte copies when HW % 4 == 0 and the pointers are 16-byte aligned, 4-byte ones otherwise. */
int egz_cat2_planes(const float* f, const float* g, float* out, int B, long HW, hipStream_t stream);
/* Input pipeline on the device (data/STdatas.py:50-68, data/lateDataset.py:22-33): uint8 planes [...][C][plane] ->
 * (u8 / 255 - mean[c]) / std[c] in fp32, the reference's three correctly-rounded operations (bit-exact). */
int egz_u8_normalize(const unsigned char* src, float* dst, long n, long plane, int C, const float* mean,
                     const float* std, hipStream_t stream);
/* A batch gathered from a pool of decoded planes that stays on the device (data/resident.py, csrc/batch_gather.hip).  pool
 * (P, H, W) uint8; table (N, 22) int64 plane numbers per sample -- column 0 the first of 3 consecutive BGR planes, 1 .. 20 the
 * flow planes (x_t, y_t, x_{t-1}, y_{t-1}, ...), 21 the ground truth; idx (B,) int64 sample numbers; mean / std 24 floats each.
 * Outputs, each optional (null: not produced, nothing written): image (B,3,H,W), flow (B,20,H,W), gt (B,1,H,W) fp32 =
 * (u8 / 255 - mean) / std, bit-identical with egz_u8_normalize of the gathered bytes; flow_nhwc32 (B,H,W,32), bit-identical
 * with egz_nchw_to_nhwc_pad of flow (channels 20 .. 31 zero), together with absmax (egz_absmax layout, zero-filled by the
 * caller: receives max |flow|); raw (B,24,H,W) uint8, the gathered bytes, of which the fields in raw_fields (bit 0 image, 1
 * flow, 2 gt) are written.  H * W % 4 == 0; pool offsets are 64-bit.  A sample number or a table entry of a field in use that is
 * out of range is not dereferenced: that sample is skipped and *status (device, zero-filled by the caller) gets bit 0 (idx)
 * or bit 1 (table). */
int egz_resident_gather(const unsigned char* pool, long P, const long* table, long N, const long* idx, int B, int H, int W,
                        const float* mean, const float* std, float* image, float* flow, float* gt, float* flow_nhwc32,
                        unsigned int* absmax, unsigned char* raw, int raw_fields, int* status, hipStream_t stream);
/* egz_resident_gather with data augmentation in the same launch.  Per sample: a horizontal flip and an
 * integer translation (dy, dx) applied alike to the colour frame, the flow planes and the ground truth -- out(y, x) =
 * F(y - dy, x - dx), F the flipped frame; colour and flow replicate the edge, the ground truth is 0 outside the frame; an x-flow
 * plane (table columns 1, 3, ..., 19) becomes 255 - byte under a flip -- and on the colour frame alone v = min(max(gain * (u8 /
 * 255) + bias, 0), 1) before the normalisation, each operation rounded once.  raw carries the geometric step only.  The
 * parameters are drawn on the device from a hash of (seed, epoch, idx[b]) -- flip with probability flip_thr / 2^32 (0 <= flip_thr
 * <= 2^32), dy, dx in -max_shift .. max_shift (0 <= max_shift <= 32767), gain in 1 +- contrast, bias in +- brightness (both
 * amplitudes in [0, 1)) -- unless params_in (device, (B, 5) int32 rows flip, dy, dx, float bits of gain, float bits of bias) is
 * non-null: then its rows are used.  params_out (device, same layout, optional) receives the parameters used.  flip 0, dy = dx =
 * 0, gain 1, bias 0 reproduce egz_resident_gather bit for bit.  W % 4 == 0 and H * W < 2^31.  *status: bits 0 and 1 as above;
 * bit 2 = an explicit row with flip outside {0, 1}, |dy| or |dx| above 32767 or a non-finite gain / bias: the sample was skipped. */
int egz_resident_gather_aug(const unsigned char* pool, long P, const long* table, long N, const long* idx, int B, int H, int W,
                            const float* mean, const float* std, float* image, float* flow, float* gt, float* flow_nhwc32,
                            unsigned int* absmax, unsigned char* raw, int raw_fields, int* status, unsigned long long seed,
                            unsigned long long epoch, unsigned long long flip_thr, int max_shift, float contrast,
                            float brightness, const int* params_in, int* params_out, hipStream_t stream);
/* egz_resident_gather_aug with a magnification g and a rotation theta about the frame's centre c = ((W - 1) / 2, (H - 1) / 2)
 * in the same launch: p_out = c + d + g R(theta) (F(p_src) - c), F the flip and d = (dx, dy) the shift
 * above; theta in radians, positive turning the picture from +x towards +y (y down).  Every output pixel takes its source
 * coordinate in 1/256 pixel from a Q16 inverse matrix -- fp32 polynomial sine and cosine and a correctly rounded 1 / g, each
 * operation rounded once, then integers only -- and the bilinear mix of the four neighbouring bytes of every plane: colour and
 * flow replicate the edge, the ground truth is 0 outside the frame, and the vector of a flow pair (table columns 1 + 2 k, 2 +
 * 2 k) about byte 127.5 is turned and scaled by the forward matrix and clamped to 0 .. 255.  The draw adds two words of the same
 * hash: g in 1 +- scale (0 <= scale <= 0.5), theta in +- rotate_rad (0 <= rotate_rad <= float32(pi / 4)); the other five
 * parameters of a (seed, epoch, sample) are those of egz_resident_gather_aug.  params_in / params_out are (B, 7) int32 on the
 * device: flip, dy, dx, bits(gain), bits(bias), bits(g), bits(theta).  g = 1 and theta = 0 reproduce egz_resident_gather_aug bit
 * for bit.  W % 4 == 0 and H * W < 2^31.  *status: bits 0 .. 2 as above; bit 3 = an explicit row with g outside [0.5, 1.5],
 * |theta| above float32(pi / 4) or a non-finite g / theta: the sample was skipped. */
int egz_resident_gather_affine(const unsigned char* pool, long P, const long* table, long N, const long* idx, int B, int H,
                               int W, const float* mean, const float* std, float* image, float* flow, float* gt,
                               float* flow_nhwc32, unsigned int* absmax, unsigned char* raw, int raw_fields, int* status,
                               unsigned long long seed, unsigned long long epoch, unsigned long long flip_thr, int max_shift,
                               float contrast, float brightness, const int* params_in, int* params_out, float scale,
                               float rotate_rad, hipStream_t stream);
/* A late-fusion batch gathered from such a pool (data/late_resident.py, csrc/batch_gather.hip).  pool (P, H, W) uint8; table
 * (N, 3) int64 plane numbers per sample -- column 0 the SP prediction, 1 the AT map, 2 the ground truth; idx (B,) int64 sample
 * numbers.  Outputs, each optional (null: not produced, nothing written): fused (B,2,H,W) fp32, channel 0 the AT map and
 * channel 1 the SP prediction (the tensor egz_cat2_planes builds for models/late_fusion.py); gt (B,1,H,W) fp32; raw (B,3,H,W)
 * uint8, the gathered bytes in table order.  Every fp32 value is (float)u8 / 255.f, the correctly rounded division:
 * bit-identical with egz_u8_normalize(mean 0, std 1) of the gathered bytes.  H * W % 4 == 0; pool offsets are 64-bit.  A sample
 * number, or a table entry of an output asked for, that is out of range is not dereferenced: that sample is skipped and
 * *status (device, zero-filled by the caller) gets bit 0 (idx) or bit 1 (table). */
int egz_late_gather(const unsigned char* pool, long P, const long* table, long N, const long* idx, int B, int H, int W,
                    float* fused, float* gt, unsigned char* raw, int* status, hipStream_t stream);
/* One step of the AT module's LSTM loops fetched from a pool of the extracted fixation vectors that stays on the device
 * (data/lstm_resident.py, csrc/lstm_pool.hip).  pool (rows, width) fp32; in_row / tgt_row (n_steps,) int32 pool rows and reset
 * (n_steps,) uint8: the step plan; cursor: two ints on the device, {next step, step being run}.  With k = cursor[0], 0 <= k <
 * n_steps and both rows of step k inside the pool: inp[0 .. width) = pool[in_row[k]], tgt[0 .. width) = pool[tgt_row[k]],
 * state[0 .. state_n) = 0 if reset[k] != 0 and state is not null, then cursor[1] = k and cursor[0] = k + 1 -- a later launch of
 * the same stream can address per-step output off cursor + 1 (egz_mse_fwd_grad's counter).  Otherwise nothing is dereferenced
 * with the index that failed, nothing is written and the cursor stays: *status (device, zero-filled by the caller once; a sticky
 * OR) gets bit 0 (cursor outside the plan) or bit 1 (a plan row outside the pool).  One single-block launch; 1 <= width <= 4096
 * (egz_mse_fwd_grad's limit), rows >= 1, n_steps >= 1, state_n >= 0, every pointer but state required: anything else returns an
 * error and launches nothing. */
int egz_lstm_pool_fetch(const float* pool, long rows, int width, const int* in_row, const int* tgt_row,
                        const unsigned char* reset, long n_steps, int* cursor, float* inp, float* tgt, float* state,
                        long state_n, unsigned int* status, hipStream_t stream);
/* The SP -> AT hand-over written into such a pool on the device (extractLSTMw.extractw(into=...), csrc/lstm_pool.hip): for
 * every sample b of an encoder forward, the vector the file path stores in fix_<name>.pth.tar.  feat (B, H, W, C) fp32
 * channels-last, H == W; gt_pool (Q, H cell, W cell) uint8 and gt_src (B,) int64: sample b's ground truth is plane gt_src[b];
 * pool (rows, C) fp32 and dst (B,) int64: the row that takes sample b's vector, -1 skips the sample (nothing of it is read).
 * Gaze cell = the first arg-max of avg_pool2d(u8 / 255, cell) as ATen's CPU kernel computes it: per cell s = 0.f, s += (float)u
 * / 255.f over its cell x cell bytes in row-major order, s / (float)(cell cell); on equal scores the lower cell.  Window =
 * extractLSTMw.var_window(gaze cell, size) (both coordinates clipped with H); pool[dst[b]][c] = the window mean of channel c
 * with egz_window_mean's arithmetic.  cells (B,) int32, optional (null: not written): the flat gaze cell of every stored
 * sample.  A gt_src[b] outside [0, Q) or a dst[b] outside [-1, rows) is never turned into an address: that sample writes
 * nothing and *status (device, zero-filled by the caller; a sticky OR) gets bit 0.  1 <= B <= 65535, 1 <= H == W <= 1024,
 * 1 <= cell <= 256, 1 <= size <= H, C, Q, rows >= 1, every pointer but cells required: anything else returns an error and
 * launches nothing.  The rows named in one call must be distinct.  No allocation, no synchronisation. */
int egz_lstm_store(const float* feat, int B, int H, int W, int C, const unsigned char* gt_pool, long Q, const long* gt_src,
                   int cell, int size, float* pool, long rows, const long* dst, int* cells, unsigned int* status,
                   hipStream_t stream);
/* AT extraction glue (AT.py:25-39,58-66,229; extractLSTMw.py:81-90): chn_weight = mean of the size x size window of the
 * channels-last (B,H,W,C) feature map around gaze_point / cell; weighted map = min-max normalised sum_c feat * w. */
int egz_crop_mean(const float* feat, const int* gp, float* out, int B, int H, int W, int C, int size, int cell,
                  hipStream_t stream);
/* extractLSTMw.crop_feature_var (extractLSTMw.py:46-58) + mean: explicit window {y0, y1, x0, x1} per sample */
int egz_window_mean(const float* feat, const int* win, float* out, int B, int H, int W, int C, hipStream_t stream);
/* AT.crop_align_feature + mean (AT.py:41-56,229; extractLSTMw.py:32-44, `--align`): the mean of a window of the bilinearly
 * x16-upsampled map is a linear functional of the map -- out[b][c] = sum_p wmap[b][p] * feat[b][p][c] */
int egz_pixel_weighted_sum(const float* feat, const float* wmap, float* out, int B, int HW, int C, hipStream_t stream);
/* AT.get_weighted (AT.py:58-66): channel-weighted sum, (x - min) / max(x - min) per map, HW <= 4096.  A NaN sum makes the whole
 * map NaN, as torch.min / torch.max propagate it */
int egz_weighted_minmax(const float* feat, const float* w, float* out, int B, int HW, int C, hipStream_t stream);

/* Config-1 glue (run_spatialstream.py:99-104,130-136): centre of mass of the uint8-quantised gaze map exactly as
 * scipy.ndimage.center_of_mass((map * 255).astype(uint8)) computes it (com (B,2) doubles, gp = floor(com) (B,2) int32, q8
 * optional (B,H,W) uint8 image), and nn.functional.interpolate(mode='bilinear', scale_factor=scale) of (B,h,w) maps with either
 * align_corners convention (False: run_spatialstream.py:136; True: upsample_bilinear at AT.py:47, extractLSTMw.py:33); sample b
 * of the result starts at dst + b * dst_bstride floats. */
int egz_u8_center_of_mass(const float* map, int B, int H, int W, double* com, int* gp, unsigned char* q8, hipStream_t stream);
int egz_bilinear_up(const float* src, float* dst, int B, int h, int w, int scale, int align_corners, long dst_bstride,
                    hipStream_t stream);

/* Dual TV-L1 optical flow (csrc/flow_tvl1.hip; DESIGN.md "TV-L1 optical flow"; data/extract_flow.py): the flow_x / flow_y images
 * of the temporal stream from a run of grey frames.  A batch of N pairs is a run of F = N + 1 planes, pair i = planes i, i + 1;
 * images are 16 .. 2048 pixels per side; a shape or parameter outside its range returns an error and launches nothing.
 *   egz_bgr_to_gray_u8  BGR bytes, interleaved (N, H, W, 3) or planar (N, 3, H, W), -> (N, H, W) by OpenCV's 8-bit rule
 *                       (4899 R + 9617 G + 1868 B + 8192) >> 14.
 *   egz_flow_gauss      separable Gaussian, replicated border, of uint8 (src_u8) or float planes; gw: 2 R + 1 float taps on the
 *                       device (scipy.ndimage's); tmp, dst: planes x H x W floats each, distinct.
 *   egz_flow_resample   Keys bicubic (a = -0.5), position and taps clamped: dst(i, j) = scale * src((i + .5) hs / hd - .5, ..).
 *   egz_flow_grad       central differences, replicated border.
 *   egz_tvl1_warp       img: N + 1 planes; i1x, i1y: gradient of planes 1 .. N; u: state (u1, u2 read); consts (4, N, H, W)
 *                       = gx, gy, gx^2 + gy^2, I1w - gx u1 - gy u2 - I0 with I1, its gradient sampled at x + u.
 *   egz_tvl1_iterate    `iterations` inner iterations on the state (6, N, H, W) = u1 u2 p11 p12 p21 p22 read from a, k per
 *                       launch: 1 = one streaming launch per iteration, 2 / 3 / 4 / 6 / 8 = overlapped tiles in LDS, 0 =
 *                       egz_tvl1_default_k(); every k gives the same bits.  The result is in a if ceil(iterations / k) is even,
 *                       else in b; the other buffer is overwritten.
 *   egz_flow_to_u8      v > bound -> 255, v < -bound -> 0, else rint(255 (v + bound) / (2 bound)) in double, half to even.
 *   egz_tvl1_flow       the whole chain on (F, H, W) grey bytes -> u1, u2 (F - 1, H, W) floats; gw0 / gw1: presmoothing /
 *                       pyramid taps; ws: egz_tvl1_flow_ws_bytes(F, H, W, nscales, zfactor) bytes (0 = arguments out of range). */
int egz_tvl1_default_k(void);
int egz_bgr_to_gray_u8(const unsigned char* src, int N, int H, int W, int planar, unsigned char* dst, hipStream_t stream);
int egz_flow_gauss(const void* src, int src_u8, int planes, int H, int W, const float* gw, int R, float* tmp, float* dst,
                   hipStream_t stream);
int egz_flow_resample(const float* src, int planes, int hs, int ws, float* dst, int hd, int wd, float scale, hipStream_t stream);
int egz_flow_grad(const float* img, int planes, int H, int W, float* gx, float* gy, hipStream_t stream);
int egz_tvl1_warp(const float* img, const float* i1x, const float* i1y, const float* u, float* consts, int N, int H, int W,
                  hipStream_t stream);
int egz_tvl1_iterate(float* a, float* b, const float* consts, int N, int H, int W, int iterations, int k, double tau,
                     double lambda, double theta, hipStream_t stream);
int egz_flow_to_u8(const float* v, long n, double bound, unsigned char* out, hipStream_t stream);
size_t egz_tvl1_flow_ws_bytes(int F, int H, int W, int nscales, double zfactor);
int egz_tvl1_flow(const unsigned char* frames, int F, int H, int W, const float* gw0, int R0, const float* gw1, int R1,
                  double tau, double lambda, double theta, int nscales, double zfactor, int warps, int iterations, int k,
                  void* ws, size_t ws_bytes, float* u1, float* u2, hipStream_t stream);

/* ---- measurement aid (bench.py): sustained v_mfma_f32_32x32x16_f16 rate of this chip on the given operand bits; frag =
 *      16 x 64 x 16 bytes, out = blocks x 256 floats; executes blocks x 4 x iters x 8 MFMAs of 32768 flop. */
int egz_mfma_probe(const void* frag, float* out, int blocks, int iters, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* EGAZE_HIP_H */
