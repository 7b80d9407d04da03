/*
 * idiff_hip.h -- C ABI of libidiff_hip.so, the gfx950 (MI355X) kernels behind the
 * manifold_dimension hot path of GBATZOLIS/ID-diff.
 *
 * Conventions
 *   - Every pointer is a DEVICE pointer (HBM) unless named h_*; the library never
 *     allocates, frees or synchronises: the caller owns all buffers and passes the
 *     hipStream_t (as void*) the work is enqueued on.  Re-entrant.  The only process-level state is
 *     (a) which devices already carry the per-kernel dynamic-LDS attribute (one bit per device
 *     ordinal, set on first use on that device) and (b) the debug switches of idiff_set_option(),
 *     read from the environment once when the library is loaded -- never on a launch path.
 *   - Return value: 0 on success, otherwise a hipError_t (launch failure) or
 *     IDIFF_EINVAL (1001) for an argument the kernels cannot take; idiff_last_error()
 *     gives a thread-local message.
 *   - "Replaces" names the reference interface (file:line under GBATZOLIS/ID-diff)
 *     that the entry point stands in for.
 *   - Buffers.  What a scratch buffer or workspace holds on entry is unspecified: every word a kernel reads from it has been
 *     written by the same call (a kernel before it, or a memset on the stream).  Its size is exactly what the query beside the
 *     entry point returns (idiff_*_scratch_doubles, idiff_*_workspace_bytes, or the count stated in the comment); nothing is
 *     written beyond it.  What it holds on return is unspecified too, unless the comment says otherwise.  Every element of
 *     every output is written on a return of 0, whatever the call computes for it (a refused query, a failed solve), unless
 *     the comment names the elements that are not; an operand that is "only read" comes back bit for bit.
 *     tests/test_hip_buffer_contract.py holds the fp64 / neighbour-search / graph launchers to this.
 */
#ifndef IDIFF_HIP_H
#define IDIFF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IDIFF_EINVAL 1001
#define IDIFF_ABI_VERSION 1

int idiff_abi_version(void);
const char *idiff_last_error(void);
/* First 16 hex digits of the sha256 over the sources the library was built from (csrc/build.sh); the Python binding
 * compares it with the tree and refuses a stale libidiff_hip.so. */
const char *idiff_source_stamp(void);
/* "" for the product library.  A diagnostic / A-B build (csrc/build.sh with IDIFF_VARIANT=<name> IDIFF_VARIANT_FLAGS=...: timing-only
 * kernels, stamped kernels, lifted scratch limit) reports its extra compile flags here, is written to libidiff_hip.<name>.so only,
 * and the Python binding loads it only when IDIFF_LIB_VARIANT=<name> asks for it -- never from the production path. */
const char *idiff_variant_flags(void);

/* Debug / A-B switches, named like the environment variables that initialise them at load time:
 * IDIFF_NO_WINOGRAD (3x3 convs on the implicit GEMM), IDIFF_NO_COLSTATS, IDIFF_NO_PIPE, IDIFF_SCALAR_EPILOGUE,
 * IDIFF_TRIDIAG_ONESTAGE (per-column Householder instead of the two-stage band reduction),
 * IDIFF_UFD_ROWS, IDIFF_CHASE_WAVEFRONT (bulge chasing one launch per wavefront instead of the persistent systolic kernel),
 * IDIFF_CHASE_SPIN_LIMIT (polls before a waiting node of the systolic chase gives up; default 2^24), IDIFF_FAKE_CU_COUNT
 * (CU count used when sizing the systolic chase; tests), IDIFF_SBR_SYNC (band reduction waits for and names every launch on
 * stderr: a fault then names its kernel),
 * IDIFF_NO_SPLIT (contractions of idiff_gemm_f32 / idiff_conv2d_nhwc_f32 on the fp32 matrix cores instead of the
 * split-precision products described there),
 * IDIFF_NO_WINO43 (3x3 convolutions on the F(2x2,3x3) kernel instead of F(4x4,3x3)), IDIFF_NO_WINO43H (F(4x4,3x3) with its
 * contractions on the fp32 matrix cores instead of fp16 pairs), IDIFF_NO_FUSED_ATTN (idiff_attention256_ok and idiff_attention_heads_ok answer 0), IDIFF_NO_WINO1D (idiff_conv2d_wino1d_ok answers 0),
 * IDIFF_NO_FUSED_GN (idiff_conv2d_wino1d_gn_ok answers 0: the GroupNorm behind a row-wise convolution stays a launch of its own), IDIFF_NO_FUSED_GN_LOAD
 * (idiff_conv2d_wino1d_normload_ok answers 0: the GroupNorm in front of a row-wise convolution stays a pass of its own),
 * IDIFF_NO_FUSED_GN_LOAD_2SRC (idiff_conv2d_wino1d_normload_2src_ok answers 0: the GroupNorm of cat[x1, x2] in front of a row-wise
 * convolution stays a pass of its own), IDIFF_NO_FUSED_GN_FIR (idiff_upfirdn2d_gn_ok answers 0: the GroupNorm in front of the FIR
 * resampling of an up / down block stays a pass of its own), IDIFF_NO_PAIRS (idiff_gemm_pairs_ok answers 0: the 1x1
 * projections behind a GroupNorm stay on idiff_gemm_f32's six-product form), IDIFF_NO_2SRC_PITCH (idiff_gemm_2src_ld_ok answers 0: the
 * shortcut of cat[h, skip] with sources of different widths stays two contractions), IDIFF_NO_FUSED_RES_UP (idiff_conv2d_wino1d_resup_ok
 * answers 0: the shortcut of an up block is upsampled by a pass of its own), IDIFF_PAIRS_MIN_TILES (tests: the number of 128 x 128
 * tiles from which idiff_gemm_pairs_ok answers 1; default 256).
 * Returns the previous value, -1 for an unknown name.  No reference counterpart. */
int idiff_set_option(const char *name, int value);

/* The same switch for launches made from the CALLING host thread only (every launcher reads its switches on the thread that
 * calls it); set = 0 removes the override and the process-wide value applies again.  Used by the fail-soft re-solve of a
 * failed eigensolve, so that selecting a slower solver form for ONE launch cannot change what another host thread launches
 * in the meantime.  Returns 0, -1 for an unknown name.  No reference counterpart. */
int idiff_set_thread_option(const char *name, int value, int set);

/* ------------------------------------------------------------------ native ops (op/) */

/* Replaces the pybind entry `upfirdn2d(input, kernel, up_x, up_y, down_x, down_y, pad_x0, pad_x1,
 * pad_y0, pad_y1)` of op/upfirdn2d.cpp:12-19 (host op op/upfirdn2d_kernel.cu:209-369).
 * x is [major, in_h, in_w, minor] fp32 contiguous, k is [kh, kw] fp32 (NOT flipped: the op is a true
 * convolution, the kernel flips), out is [major, out_h, out_w, minor] with
 * out_h = (in_h*up_y + pad_y0 + pad_y1 - kh)/down_y + 1 (op/upfirdn2d_kernel.cu:237-240).
 * minor = 1 is the NCHW view the reference uses (op/upfirdn2d.py:99); minor = C serves NHWC activations.
 * major = 0 (an empty batch) launches nothing and accepts null pointers. */
int idiff_upfirdn2d_f32(const float *x, const float *k, float *out, int major, int in_h, int in_w, int minor,
                        int kh, int kw, int up_x, int up_y, int down_x, int down_y, int pad_x0, int pad_x1,
                        int pad_y0, int pad_y1, void *stream);

/* The kernel idiff_upfirdn2d_f32 would launch for these arguments (same admission code, same thread options such as
 * IDIFF_UFD_ROWS; x and out are only inspected for 16-byte alignment): "planes_fir4", "planes_rowslide", "planes_down2",
 * "planes_whole<0>" / "<1>" / "<-1>", "planes_lds", "nhwc_up2_block", "nhwc_rows<0>" / "<1>" / "<-1>", "nhwc_vec4",
 * "generic", or "none" when major == 0 (nothing to launch).  NULL for arguments the launcher refuses (idiff_last_error says
 * why).  Launches nothing; no reference counterpart. */
const char *idiff_upfirdn2d_route(const void *x, const void *out, int major, int in_h, int in_w, int minor, int kh, int kw,
                                  int up_x, int up_y, int down_x, int down_y, int pad_x0, int pad_x1, int pad_y0, int pad_y1);

/* idiff_upfirdn2d_f32 on act(a x + b): x is the RAW input of a GroupNorm over [major = images, in_h, in_w, minor = channels], coef
 * [major, minor, 2] floats (a, b) per (image, channel) from idiff_groupnorm_coef_f32, 16-byte aligned; act: IDIFF_ACT_SILU or
 * IDIFF_ACT_NONE.  The norm is applied to every sample as it is loaded (one fma, the pass's own SiLU); taps outside the image are exact
 * zeros, never act(b); the normalised tensor is never written.  Served where idiff_upfirdn2d_f32 takes "nhwc_up2_block" (up 2, 4x4
 * taps, pads (2, 1)) or "nhwc_rows<0>" with down 2 and 4x4 taps (minor % 4 == 0: the score networks' FIR x2 / :2), by kernels of its
 * own (a thread slides a 3 x 3 window along its row / forms a 2 x 2 output block, so that a sample's SiLU is evaluated 3 / 2.25 times
 * and not 9 / 4); every other geometry or activation, and a null or misaligned coef, is refused with an error and nothing launched.
 *   idiff_upfirdn2d_gn_ok   1 where the launcher serves these arguments AND the form was measured faster than the pass plus the plain
 *                           kernel (up: maps of 64 pixels and more, down: of 256 and more); 0 otherwise and under
 *                           IDIFF_NO_FUSED_GN_FIR.  Launches nothing.
 * No reference counterpart. */
int idiff_upfirdn2d_gn_f32(const float *x, const float *k, const float *coef, int act, float *out, int major, int in_h, int in_w,
                           int minor, int kh, int kw, int up_x, int up_y, int down_x, int down_y, int pad_x0, int pad_x1, int pad_y0,
                           int pad_y1, void *stream);
int idiff_upfirdn2d_gn_ok(const void *x, const void *coef, int act, const void *out, int major, int in_h, int in_w, int minor, int kh,
                          int kw, int up_x, int up_y, int down_x, int down_y, int pad_x0, int pad_x1, int pad_y0, int pad_y1);

/* Replaces `fused_bias_act(input, bias, refer, act, grad, alpha, scale)` of op/fused_bias_act.cpp:11-17
 * (kernel op/fused_bias_act_kernel.cu:18-49).  out[i] = f(x[i] + b[(i/step_b) % size_b]) * scale with
 * act*10+grad in {10,11: identity; 12,32: 0; 30: x>0?x:x*alpha; 31: ref>0?x:x*alpha}.  b may be NULL
 * (size_b = 0), ref may be NULL unless grad = 1. */
int idiff_fused_bias_act_f32(const float *x, const float *b, const float *ref, float *out, int64_t n,
                             int step_b, int size_b, int act, int grad, float alpha, float scale, void *stream);

/* The other two dtypes of the reference's native-op dispatch (AT_DISPATCH_FLOATING_TYPES_AND_HALF: op/upfirdn2d_kernel.cu:311,
 * op/fused_bias_act_kernel.cu:79).  Same arguments and geometry as the _f32 entry points; the FIR kernel / bias / ref tensors carry
 * the input's dtype, as the reference's `data_ptr<scalar_t>()` calls require.  f16 pointers are IEEE binary16 (torch.float16).
 *   upfirdn2d:      f16 = fp32 products and accumulation, rounded once to half (the CPU path's arithmetic, op/upfirdn2d.py:159-200;
 *                   the reference's CUDA kernels round per tap in one of two ways depending on the kernel chosen); f64 = fp64
 *                   products and accumulation (its tiled kernels form fp32 products under an fp64 accumulator, .cu:115-116,198).
 *   fused_bias_act: the reference kernel's scalar_t arithmetic operation by operation: alpha and scale are converted to the
 *                   tensor's dtype first (.cu:19), then x = r(x + b), y = x > 0 ? x : r(x * alpha), out = r(y * scale) with r =
 *                   rounding to the dtype. */
int idiff_upfirdn2d_f16(const void *x, const void *k, void *out, int major, int in_h, int in_w, int minor, int kh, int kw,
                        int up_x, int up_y, int down_x, int down_y, int pad_x0, int pad_x1, int pad_y0, int pad_y1, void *stream);
int idiff_upfirdn2d_f64(const double *x, const double *k, double *out, int major, int in_h, int in_w, int minor, int kh, int kw,
                        int up_x, int up_y, int down_x, int down_y, int pad_x0, int pad_x1, int pad_y0, int pad_y1, void *stream);
int idiff_fused_bias_act_f16(const void *x, const void *b, const void *ref, void *out, int64_t n, int step_b, int size_b,
                             int act, int grad, float alpha, float scale, void *stream);
int idiff_fused_bias_act_f64(const double *x, const double *b, const double *ref, double *out, int64_t n, int step_b,
                             int size_b, int act, int grad, float alpha, float scale, void *stream);

/* ------------------------------------------------------------------ dense contractions (fp32 in, fp32 out) */

/* Activation codes shared by the epilogues below. */
#define IDIFF_ACT_NONE 0
#define IDIFF_ACT_SILU 1
#define IDIFF_ACT_ELU 2
#define IDIFF_ACT_RELU 3
#define IDIFF_ACT_LRELU 4 /* slope 0.2, models/layers.py:36 */

/* Epilogue applied by idiff_gemm_f32 / idiff_conv2d_nhwc_f32 to every accumulator element (m, n):
 *   v = acc + bias[n] + rowbias[(m / rows_per_group) * ld_rowbias + n]
 *   v = act(v)
 *   v = (v + residual[m * ld_residual + n]) * out_scale          (residual optional)
 *   v = v * rowscale[m / rows_per_group]                          (optional, e.g. -1/std[b]: models/utils.py:266-267)
 *   out[m * ldc + n] = v
 * NULL pointers drop the corresponding term.  This is what lets one launch produce
 * `Conv_0(h) + Dense_0(act(temb))[:, :, None, None]` (models/layerspp.py:256-259) or
 * `(x + Conv_1(h)) / sqrt(2)` (:262-273) without extra passes over HBM. */
typedef struct idiff_epilogue {
  const float *bias;      /* [N] or NULL */
  const float *rowbias;   /* [M / rows_per_group, ld_rowbias] or NULL */
  int64_t ld_rowbias;
  int rows_per_group;     /* e.g. H*W for a per-sample time-embedding bias */
  int act;                /* IDIFF_ACT_* */
  const float *residual;  /* [M, ld_residual] or NULL */
  int64_t ld_residual;
  float out_scale;        /* 1.0f for none */
  const float *rowscale;  /* [M / rows_per_group] or NULL */
  double *colstats;       /* NULL, or [tiles_m, N, 2] fp64: per row-tile column sums (sum, sum of squares) of the stored
                             values, so that the GroupNorm consuming the output needs no statistics pass of its own; only
                             valid when idiff_gemm_colstats_split / idiff_conv2d_colstats_split returns > 0 */
} idiff_epilogue;

/* Batched C[b] = epilogue(A[b] (M x K, row-major, lda) * Bt[b]^T (Bt is N x K, row-major, ldb)).
 * Replaces torch.nn.Linear (models/fcn.py:18-28), NIN / 1x1 conv contractions (models/layers.py:555-564),
 * and the two attention einsums of models/layerspp.py:82-86.  fp32 operands and results.  Arithmetic of the fast path
 * (16-byte aligned K-contiguous operands below 4 GiB): every operand element is cut EXACTLY into three bf16 pieces
 * (8 + 8 + 8 mantissa bits) and a product is formed as the six partial products of weight >= 2^-16 on
 * v_mfma_f32_32x32x16_bf16 with fp32 accumulation; what is left out is < 2^-23 of the product, the size of one fp32
 * rounding (1.7e-7 against an fp64 contraction where the k-ordered fp32 fma chain of v_mfma_f32_32x32x2_f32 gives
 * 2.0e-7).  IDIFF_NO_SPLIT selects that fp32 chain; operands the fast path does not take always use it.
 * Non-finite operands: the cut forms x - hi(x), so a +-inf element turns into NaN in its lower pieces and every output that
 * element reaches is NaN, where the fp32 chain would give +-inf (or NaN against a zero).  Non-finite stays non-finite -- the
 * drivers refuse a score matrix with any non-finite entry either way -- but inf vs NaN is not preserved on this path.
 * batch strides are in elements; a stride of 0 broadcasts that operand.  The epilogue pointers are
 * shared by all batch entries. */
int idiff_gemm_f32(const float *A, int64_t lda, int64_t strideA, const float *Bt, int64_t ldb, int64_t strideB,
                   float *C, int64_t ldc, int64_t strideC, int M, int N, int K, int batch,
                   const idiff_epilogue *ep, void *stream);

/* The batched contraction of idiff_gemm_f32, C[b] = epilogue(A[b] (M x K) * Bt[b]^T (Bt is N x K)), with every fp32 operand element
 * as a PAIR of fp16 values (hi = fp16(v), lo = fp16(v - hi): 22 significand bits) and a product as lo*hi + hi*lo + hi*hi on
 * v_mfma_f32_32x32x16_f16 with fp32 accumulation -- three matrix instructions where idiff_gemm_f32's exact bf16 cut needs six, and
 * the matrix pipes are what that form runs out of (1.36-1.64x faster on the q / k / v projections of models/layerspp.py:66-98 at
 * BASELINE sizes, scripts/gemm_pairs_probe.py).  fp16 has a 5-bit exponent, so the CALLER vouches for the ranges: one operand is an
 * ACTIVATION, used as it is, and must be of order one -- |x| < 65504 (beyond: +-inf, the outputs NaN), and an element below 0.25
 * carries an absolute error of 2^-25 instead of a relative 2^-22: the output of a GroupNorm is the intended operand; the other is
 * a WEIGHT (Bt, or A when weight_is_a != 0 -- V^T = Wv n^T of the attention block), multiplied by w_scale[0], the power of two that
 * idiff_gemm_pairs_scale_f32 computes once per weight (max |w| -> [2^11, 2^12)), the sums by w_scale[1] = 1 / w_scale[0], exactly.
 * w_scale is a DEVICE pointer to those two floats.  Measured against an fp64 contraction of the same fp32 operands: 1.0e-7 where the
 * six-product form gives 1.3e-7 (a GroupNorm's output x N(0, 1/K) weights; tests/test_hip_ops.py).  idiff_gemm_pairs_ok: 1 when the
 * shape is served (N > 64, K % 4 == 0, at least 256 tiles of 128 x 128 over the batch; 0 under IDIFF_NO_PAIRS / IDIFF_NO_SPLIT /
 * IDIFF_NO_PIPE).  Operands 16-byte aligned, row pitches and batch strides multiples of 4, one batch slice inside 4 GiB.  Same
 * epilogue, same column-statistics layout as idiff_gemm_f32 (idiff_gemm_colstats_split; unbatched only). */
int idiff_gemm_pairs_ok(int M, int N, int K, int batch);
int idiff_gemm_pairs_scale_f32(const float *w, int64_t ldw, int rows, int K, float *w_scale, void *stream);
int idiff_gemm_pairs_f32(const float *A, int64_t lda, int64_t strideA, const float *Bt, int64_t ldb, int64_t strideB,
                         const float *w_scale, int weight_is_a, const float *act_scale, float *C, int64_t ldc, int64_t strideC,
                         int M, int N, int K, int batch, const idiff_epilogue *ep, void *stream);

/* The activation operand of the pair form when it is NOT a GroupNorm's output: act_scale (NULL above = 1) is a device pointer to
 * {s, 1 / s}, s the power of two the activation is multiplied by before its cut, so that its ROOT MEAN SQUARE lands in [0.71, 1.41):
 * the pair then carries 22 bits relative to the tensor's own scale whatever that scale is (elements below rms / 4: absolute error
 * 2^-25 rms), and the range bound becomes max |x| < 65504 rms.  idiff_pairs_act_scale_f32 derives it on the device from the per-tile
 * column sums (sum, sum of squares) that the contraction(s) producing the tensor -- or the two tensors of a concatenation -- left for
 * the GroupNorm that reads them as well (idiff_epilogue.colstats: [B, nsplit, C, 2] fp64); `out`: 8 floats, {s, 1 / s} in front.
 * idiff_gemm_pairs_2src_f32: the two-source contraction of idiff_gemm_2src_f32 ([A1 | A2], the shortcut of a residual block on
 * torch.cat([h, skip]), models/ncsnpp.py:376-385) on pairs, one act_scale for both sources.  K1 % 32 == 0. */
int idiff_pairs_act_scale_f32(const double *ws1, int nsplit1, int C1, const double *ws2, int nsplit2, int C2, int B, int HW, float *out,
                              void *stream);
int idiff_gemm_pairs_2src_f32(const float *A1, const float *A2, int64_t lda, int K1, const float *act_scale, const float *Bt, int64_t ldb,
                              const float *w_scale, float *C, int64_t ldc, int M, int N, int K, const idiff_epilogue *ep, void *stream);

/* The same contraction with A given as two row-major matrices of equal row pitch, A = [A1 (M x K1) | A2 (M x (K - K1))]:
 * the 1x1 shortcut of a residual block whose input is torch.cat([h, skip], dim=1) (models/ncsnpp.py:376-385 with
 * layerspp.py:271-274) without materialising the concatenation or an intermediate partial product.  K1 % 32 == 0. */
int idiff_gemm_2src_f32(const float *A1, const float *A2, int64_t lda, int K1, const float *Bt, int64_t ldb, float *C,
                        int64_t ldc, int M, int N, int K, const idiff_epilogue *ep, void *stream);
/* The same with a row pitch per source, A1 (M x K1) at lda1 and A2 (M x (K - K1)) at lda2: cat[h, skip] of two tensors of different
 * channel counts (256 + 128 in the up path of the flagship network), which otherwise takes two contractions and a partial product
 * written and read back through the residual term.  K1 % 32 == 0, (K - K1) % 4 == 0; each source inside one buffer descriptor, or the
 * rows are cut in two on the host (both sources shifted).  idiff_gemm_2src_f32 is this call with lda2 = lda1.
 *   idiff_gemm_2src_ld_ok   1 where the executor should take this form for sources of K1 and K2 columns; 0 under IDIFF_NO_2SRC_PITCH
 *                           (A/B runs: the two-contraction path returns) and IDIFF_NO_PIPE.  Launches nothing. */
int idiff_gemm_2src_ld_ok(int K1, int K2);
int idiff_gemm_2src_ld_f32(const float *A1, int64_t lda1, const float *A2, int64_t lda2, int K1, const float *Bt, int64_t ldb, float *C,
                           int64_t ldc, int M, int N, int K, const idiff_epilogue *ep, void *stream);

/* 2-D convolution, NHWC activations: x [B, H, W, Cin] (Cin % 4 == 0), weights packed as
 * wt [Cout, KH, KW, Cin] (= the reference's [Cout, Cin, KH, KW] nn.Conv2d weight permuted once at load),
 * out [B, OH, OW, Cout] with OH = (H + pad_lo + pad_hi - KH)/stride + 1 (pad_lo on top/left, pad_hi on
 * bottom/right: the non-FIR Downsample pads (0, 1), models/layerspp.py:153-155).  Implicit GEMM with M = B*OH*OW,
 * N = Cout, K = KH*KW*Cin on the same MFMA core as idiff_gemm_f32; zero padding.
 * Replaces F.conv2d behind ddpm_conv3x3 / ddpm_conv1x1 (models/layers.py:100-132) and the stride-2 VALID
 * conv of conv_downsample_2d (models/up_or_down_sampling.py:178).  rows_per_group in the epilogue counts
 * OUTPUT pixels (OH*OW for a per-sample bias). */
int idiff_conv2d_nhwc_f32(const float *x, const float *wt, float *out, int B, int H, int W, int Cin, int Cout,
                          int KH, int KW, int stride, int pad_lo, int pad_hi, const idiff_epilogue *ep, void *stream);

/* Which kernel and which form of its tail idiff_gemm_f32 (pairs = 0) / idiff_gemm_pairs_f32 (pairs != 0) / idiff_conv2d_nhwc_f32 would
 * launch for these arguments: the launchers and these queries call the same chooser (csrc/igemm.hip: igemm_choose) under the same thread
 * options; pointers are only inspected for null and for 16-byte alignment.  "<family> <tile> <arithmetic> <epilogue form>":
 *   family     "pipe" (pipelined, buffer-addressed operands), "direct-vec" / "direct-scalar" (the general kernel with 16-byte / 4-byte
 *              operand loads), "narrow" (conv3x3 to <= 4 channels on the vector ALUs; tile "c<Cout>")
 *   tile       rows x columns of a workgroup: "128x128", "128x64", "128x32", "64x64"
 *   arithmetic "split" (three bf16 pieces, six products), "fp32", "fp32-1buf" (fp32, single LDS buffer), "pairs" (fp16 pairs)
 *   epilogue   "buf-block" (C and residual through buffer descriptors, group terms folded per 32-row block: rows_per_group % 32 == 0),
 *              "buf-row" (the same with the group terms per row), "vec64" (16-byte accesses through 64-bit addresses: C or the residual
 *              beyond 0xE0000000 bytes, or a tile's rows spanning 0x0FFFFFF0 bytes), "scalar" (one element at a time: an operand of the
 *              tail that is not 16-byte aligned, N / ldc / a pitch not a multiple of 4, IDIFF_SCALAR_EPILOGUE; always for "direct-*");
 *              "narrow": "row" / "elem" (rowscale folded per image row / applied per element) or "none" (no rowscale)
 * idiff_gemm_2src_f32 / idiff_gemm_pairs_2src_f32 take the route of the one-source call with A = A1.  A problem cut in two on the host
 * (an operand beyond 4 GiB) reports its first half.  "none" when there is nothing to launch (an empty problem), NULL for arguments the
 * launcher refuses (idiff_last_error says why).  Launches nothing; no reference counterpart. */
const char *idiff_gemm_route(const void *A, int64_t lda, int64_t strideA, const void *Bt, int64_t ldb, int64_t strideB, const void *C,
                             int64_t ldc, int64_t strideC, int M, int N, int K, int batch, const idiff_epilogue *ep, int pairs);
const char *idiff_conv2d_route(const void *x, const void *wt, const void *out, int B, int H, int W, int Cin, int Cout, int KH, int KW,
                               int stride, int pad_lo, int pad_hi, const idiff_epilogue *ep);

/* Fused GroupNorm statistics: when `rows_per_sample` consecutive output rows form one sample, these return the number of
 * workgroup row-tiles per sample (`nsplit`: epilogue.colstats is then laid out [samples, nsplit, N, 2]) or 0 when the
 * fused statistics are unavailable for the problem (general kernel, operands beyond 4 GiB, tiles straddling samples).  The rule is the
 * launchers' own: "the pipelined kernel takes this shape" (csrc/igemm.hip: pipe_serves_linear / pipe_serves_conv, which the front ends
 * of idiff_gemm_f32 / idiff_conv2d_nhwc_f32 ask too, adding pointer alignment and batch strides) and whole tiles of the chooser's tile
 * (igemm_tile) per sample.  nsplit > 0 therefore implies that a call with 16-byte aligned operands takes tiles of rows_per_sample /
 * nsplit rows; the launchers accept some calls these decline (samples of 96 rows in tiles of 64). */
int idiff_gemm_colstats_split(int M, int N, int K, int64_t lda, int64_t ldb, int rows_per_sample);
int idiff_conv2d_colstats_split(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad_lo,
                                int pad_hi);

/* The same 3x3 / stride 1 / pad 1 convolution (ddpm_conv3x3, models/layers.py:100-116; conv3x3 of
 * models/layerspp.py) by Winograd F(2x2, 3x3): 2.25x fewer multiplications than the implicit GEMM, still fp32
 * throughout (results agree with idiff_conv2d_nhwc_f32 to fp32 rounding, not bit for bit).
 *   idiff_conv2d_winograd_ok       1 when the geometry is served (H, W even, Cin % 8 == 0, Cout % 64 == 0), else 0.
 *   idiff_winograd_weight_floats   size of the transformed filter bank u (16 * Cin * Cout floats).
 *   idiff_winograd_pack_f32        wt [Cout, 3, 3, Cin] (the panel idiff_conv2d_nhwc_f32 takes) -> u, once per layer.
 *   idiff_conv2d_winograd_f32      x [B, H, W, Cin] -> out [B, H, W, Cout], epilogue as above (rows_per_group counts
 *                                  output pixels).
 *   idiff_conv2d_winograd_colstats_split   nsplit of epilogue.colstats ([samples, nsplit, Cout, 2]) or 0 when the
 *                                  fused statistics are unavailable (fewer than 64 output tiles per sample). */
int idiff_conv2d_winograd_ok(int B, int H, int W, int Cin, int Cout);
int64_t idiff_winograd_weight_floats(int Cin, int Cout);
int idiff_winograd_pack_f32(const float *wt, float *u, int Cin, int Cout, void *stream);
int idiff_conv2d_winograd_f32(const float *x, const float *u, float *out, int B, int H, int W, int Cin, int Cout,
                              const idiff_epilogue *ep, void *stream);
int idiff_conv2d_winograd_colstats_split(int B, int H, int W, int Cin, int Cout);
/* F(4x4, 3x3): the same convolution with 36 multiplications per 4x4 output tile (2.25 per output; the F(2x2, 3x3) form above
 * spends 4), interpolation points 0, +-2/3, +-3/2, infinity, all arithmetic fp32 on v_mfma_f32_32x32x2_f32 (csrc/winograd43.hip).
 * Per layer 0.8-1.4e-6 against an fp64 convolution where the 2x2 form gives 3-9e-7; measured on the whole nf = 128 NCSN++ before
 * the kernel was written (scripts/f43_emulation.py): rel_err(S) 3.3e-6 against an fp64 network, singular values within 1.4e-5.
 *   idiff_conv2d_winograd43_ok      1 when served: H % 4 == 0, W % 4 == 0, Cin % 8 == 0, Cout % 64 == 0, every tensor within one
 *                                   buffer descriptor (4 GiB), and neither IDIFF_NO_WINOGRAD nor IDIFF_NO_WINO43 set.
 *   idiff_winograd43_weight_floats  size of the transformed filter bank (36 * Cin * Cout floats).
 *   idiff_winograd43_pack_f32       wt [Cout, 3, 3, Cin] -> U = G g G^T (fp64, rounded once), once per layer.
 *   idiff_conv2d_winograd43_f32     x [B, H, W, Cin] -> out [B, H, W, Cout] with the epilogue of idiff_conv2d_nhwc_f32; a per-row-group
 *                                   bias / scale only per image (rows_per_group = H * W).
 *   idiff_conv2d_winograd43_colstats_split   nsplit of epilogue.colstats ([samples, nsplit, Cout, 2]) or 0 when the statistics cannot
 *                                   be produced (a workgroup covers 32 tiles of 4x4 pixels: whole workgroups per sample, or whole
 *                                   samples per workgroup).
 * Replaces F.conv2d behind ddpm_conv3x3 (models/layers.py:119-132) like the 2x2 form. */
int idiff_conv2d_winograd43_ok(int B, int H, int W, int Cin, int Cout);
int idiff_conv2d_winograd43_colstats_split(int B, int H, int W, int Cin, int Cout);
int64_t idiff_winograd43_weight_floats(int Cin, int Cout);
int idiff_winograd43_pack_f32(const float *wt, float *u, int Cin, int Cout, void *stream);
int idiff_conv2d_winograd43_f32(const float *x, const float *u, float *out, int B, int H, int W, int Cin, int Cout,
                                const idiff_epilogue *ep, void *stream);
/* F(4x4, 3x3) with the 36 contractions on the fp16 matrix cores (v_mfma_f32_32x32x16_f16), each fp32 operand as a PAIR of fp16
 * values hi = fp16(v), lo = fp16(v - hi) and three of the four partial products kept (hi hi + hi lo + lo hi, fp32 accumulation);
 * transforms in fp32 as above.  The filter bank is scaled by a power of two at pack time (undone exactly on the outputs) so that its
 * low parts are normal fp16 numbers; the transformed input is used as is and must stay below 65504 in magnitude (activations below
 * ~2000): beyond that the outputs are NaN.  Same parity bars as the fp32 form; measured (scripts/f43_emulation.py, whole network)
 * per layer 8.0e-7 and rel_err(S) 3.33e-6 where the fp32 contraction gives 7.8e-7 and 3.27e-6.
 *   idiff_conv2d_winograd43h_ok     1 when served: the fp32 form's conditions, Cin % 16 == 0, 32 <= Cin <= 1024, and none of
 *                                   IDIFF_NO_WINOGRAD / IDIFF_NO_WINO43 / IDIFF_NO_WINO43H set.
 *   idiff_winograd43h_weight_floats size of the bank in floats (36 * Cin * Cout for the fp16 pairs + 4 of header).
 *   idiff_winograd43h_pack_f32      wt [Cout, 3, 3, Cin] -> the scaled pairs of U = G g G^T (fp64, rounded once to fp32, then cut).
 *   idiff_conv2d_winograd43h_f32    as idiff_conv2d_winograd43_f32; colstats geometry: idiff_conv2d_winograd43_colstats_split. */
int idiff_conv2d_winograd43h_ok(int B, int H, int W, int Cin, int Cout);
int64_t idiff_winograd43h_weight_floats(int Cin, int Cout);
int idiff_winograd43h_pack_f32(const float *wt, float *u, int Cin, int Cout, void *stream);
int idiff_conv2d_winograd43h_f32(const float *x, const float *u, float *out, int B, int H, int W, int Cin, int Cout,
                                 const idiff_epilogue *ep, void *stream);

/* The same 3x3 / stride 1 / pad 1 convolution (replaces F.conv2d behind ddpm_conv3x3, models/layers.py:100-132, as the entries above)
 * by Winograd's F(4, 3) along the image rows only -- the three filter rows stay a direct sum: 4.5 multiplications per output instead of
 * 2.25, on fp16 pairs as idiff_conv2d_winograd43h_f32 (same cut, same three partial products, fp32 accumulation; one 6-point transform
 * instead of two: gain 5.4 instead of 29.3, the input may reach |x| ~ 12,000 before a pair overflows to NaN).  Twice the matrix work for
 * half the operand traffic per output: a workgroup of 512 output pixels x 64 channels reads 18 instead of 36 transformed filter slots
 * per K step and every input pixel once instead of 2.25 times, which is what bounds the 2-D form on gfx950 (csrc/wino1d.hip).
 *   idiff_conv2d_wino1d_ok             1 when served: W in {4, 8, 16, 32, 64}, H % 4 == 0 with 512 / W a multiple or a divisor of H (a workgroup takes
 *                                      whole images or a whole part of one), Cin % 16 == 0, 32 <= Cin <= 1024, Cout % 64 == 0, every tensor
 *                                      within one buffer descriptor; 0 under IDIFF_NO_WINOGRAD / IDIFF_NO_WINO43H / IDIFF_NO_WINO1D.
 *   idiff_conv2d_wino1d_colstats_split nsplit of epilogue.colstats ([samples, nsplit, Cout, 2]): H * W / 512 for maps above 512 pixels, else 1
 *                                      (0 under IDIFF_NO_COLSTATS or when the geometry is not served).
 *   idiff_wino1d_weight_floats         size of the bank in floats (18 * Cin * Cout for the fp16 pairs + 4 of header).
 *   idiff_wino1d_pack_f32              wt [Cout, 3, 3, Cin] -> the scaled pairs of U[i][ky] = (G g[ky])[i] (fp64, rounded once to fp32, then cut).
 *   idiff_conv2d_wino1d_f32            x [B, H, W, Cin] -> out [B, H, W, Cout] with the epilogue of idiff_conv2d_nhwc_f32. */
int idiff_conv2d_wino1d_ok(int B, int H, int W, int Cin, int Cout);
int idiff_conv2d_wino1d_colstats_split(int B, int H, int W, int Cin, int Cout);
int64_t idiff_wino1d_weight_floats(int Cin, int Cout);
int idiff_wino1d_pack_f32(const float *wt, float *u, int Cin, int Cout, void *stream);
int idiff_conv2d_wino1d_f32(const float *x, const float *u, float *out, int B, int H, int W, int Cin, int Cout,
                            const idiff_epilogue *ep, void *stream);
/* The same convolution with the GroupNorm (+ activation) that reads its output applied in the kernel's tail, for maps of at most 256
 * pixels (Conv_0 -> GroupNorm_1 -> act of a residual block, models/layerspp.py:256-262): a workgroup finishes 256 consecutive pixels x 64
 * channels at a time, which are whole images and whole groups, so mean and variance of every (image, group) are formed on chip -- the mean
 * first, then the sum of squares about it, both in fp64 -- and
 *     out = act(((conv + bias + rowbias) - mean) * rstd * gamma[c] + beta[c])
 * is stored instead of the convolution's output, which never reaches memory: one launch and one pass over the activations less.
 *   idiff_conv2d_wino1d_gn_ok   1 when idiff_conv2d_wino1d_ok and W <= 16, H * W divides 256, groups divides Cout and Cout / groups
 *                               divides 64; 0 otherwise and under IDIFF_NO_FUSED_GN.
 *   idiff_conv2d_wino1d_gn_f32  epilogue: bias and the per-image rowbias only (rows_per_group = H * W); a residual, colstats, an
 *                               activation or a scale in front of the norm are refused (IDIFF_EINVAL, nothing launched), as is a geometry
 *                               the query does not admit.  gamma, beta: [Cout], 16-byte aligned; act: IDIFF_ACT_*. */
int idiff_conv2d_wino1d_gn_ok(int B, int H, int W, int Cin, int Cout, int groups);
int idiff_conv2d_wino1d_gn_f32(const float *x, const float *u, float *out, int B, int H, int W, int Cin, int Cout,
                               const idiff_epilogue *ep, int groups, const float *gamma, const float *beta, float eps, int act,
                               void *stream);
/* The same convolution with the GroupNorm (+ SiLU) in FRONT of it applied by the kernel's loader, for rows of 32 pixels: a workgroup (16
 * rows) holds rows of one image, the statistics are complete before it starts (the producers' column sums), so the norm is one affine pair
 * per (image, input channel) -- idiff_groupnorm_coef_f32 -- and
 *     out = epilogue(conv(pad0(act(a[b][c] * x + b[b][c]))))
 * with the padding zero AFTER the norm: the normalised tensor is never written or read.
 *   idiff_conv2d_wino1d_normload_ok   1 where this form is served (W = 32, H % 16 == 0, Cin % 16 == 0, 16 <= Cin <= 1024, Cout % 64 == 0) and
 *                                     routed (measured faster than the pass: Cout <= 128, csrc/wino1d.hip); 0 under IDIFF_NO_FUSED_GN_LOAD, IDIFF_NO_PAIRS and the switches of idiff_conv2d_wino1d_ok.
 *   idiff_conv2d_wino1d_normload_f32  coef: [B, Cin, 2] floats (a, b), 16-byte aligned; act: IDIFF_ACT_SILU or IDIFF_ACT_NONE; the epilogue
 *                                     of idiff_conv2d_wino1d_f32.  Whether the normalised input stays inside the fp16 pairs' range is the
 *                                     caller's to decide from the GroupNorm's gamma / beta (the tensor in memory is the raw one). */
int idiff_conv2d_wino1d_normload_ok(int B, int H, int W, int Cin, int Cout);
int idiff_conv2d_wino1d_normload_f32(const float *x, const float *u, float *out, int B, int H, int W, int Cin, int Cout,
                                     const idiff_epilogue *ep, const float *coef, int act, void *stream);
/* The same with the convolution's input cat[x1, x2] along the channels read from its two sources, x1 [B, H * W, C1] and x2 [B, H * W, C2], each
 * with its own row pitch: input channels [0, C1) come from x1 and [C1, C1 + C2) from x2 (GroupNorm_0 of cat[h, skip] in a residual block of the
 * up path: neither the concatenated nor the normalised tensor is written).  The filter bank is the one packed over Cin = C1 + C2 and coef is
 * [B, C1 + C2, 2], indexed by the concatenated channel (idiff_groupnorm_coef_f32 with both sources' column sums).
 *   idiff_conv2d_wino1d_normload_2src_ok   1 where this form is served (C1 % 16 == 0, C2 % 16 == 0, both > 0, and the one-source form's
 *                                          conditions on Cin = C1 + C2) and routed (measured faster than the pass + convolution: Cout <= 128,
 *                                          csrc/wino1d.hip); 0 under IDIFF_NO_FUSED_GN_LOAD_2SRC, IDIFF_NO_PAIRS and the switches of
 *                                          idiff_conv2d_wino1d_ok.  IDIFF_NO_FUSED_GN_LOAD does not bear on it.
 *   idiff_conv2d_wino1d_normload_2src_f32  x1, x2: 16-byte aligned, each inside one buffer descriptor; the rest as
 *                                          idiff_conv2d_wino1d_normload_f32.  Anything else is refused (IDIFF_EINVAL, nothing launched). */
int idiff_conv2d_wino1d_normload_2src_ok(int B, int H, int W, int C1, int C2, int Cout);
int idiff_conv2d_wino1d_normload_2src_f32(const float *x1, int C1, const float *x2, int C2, const float *u, float *out, int B, int H, int W,
                                          int Cout, const idiff_epilogue *ep, const float *coef, int act, void *stream);

/* The plain form with its residual given at HALF the resolution: lo [B, (H/2) * (W/2), Cout] (pitch Cout, 16-byte aligned) is upsampled x2 in
 * the tail by the FIR whose 16 polyphase weights are taps[a][b][u][v] (host memory; passed on as kernel arguments): output pixel
 * (2 i + a, 2 j + b) receives sum over u, v of lo[i - 1 + a + u][j - 1 + b + v] * taps[a][b][u][v], samples outside lo counting as zero --
 * upfirdn2d with up = 2, a 4 x 4 kernel and pads (2, 1), i.e. the shortcut of an up block (W_s . x before the upsampling) without the
 * resampler's pass and without the full-resolution shortcut.  ep->residual must be NULL; everything else of the epilogue as in the plain form.
 *   idiff_conv2d_wino1d_resup_ok   1 where this form is served: idiff_conv2d_wino1d_ok, W in {8, 16, 32}, H even; 0 under
 *                                  IDIFF_NO_FUSED_RES_UP.
 *   idiff_conv2d_wino1d_resup_f32  anything else is refused (IDIFF_EINVAL, nothing launched). */
int idiff_conv2d_wino1d_resup_ok(int B, int H, int W, int Cin, int Cout);
int idiff_conv2d_wino1d_resup_f32(const float *x, const float *u, float *out, int B, int H, int W, int Cin, int Cout, const idiff_epilogue *ep,
                                  const float *lo, const float *taps, void *stream);

/* ------------------------------------------------------------------ normalisation / pointwise (HBM-bound) */

/* GroupNorm statistics over NHWC x [B, HW, C] with G groups: stats[b, g] = {mean, rstd}, biased variance,
 * rstd = 1/sqrt(var + eps) (torch.nn.GroupNorm as used at models/layerspp.py:219,231).  fp64 accumulation.
 * `x2`/`C2` describe an optional second source whose channels are appended to x's (the skip tensor of
 * torch.cat([h, hs.pop()], 1), models/ncsnpp.py:324) so the concatenation is never materialised for the norm
 * (a group may straddle the two sources: 256 + 128 channels in 32 groups of 12).  workspace: >= B * nsplit * (C + C2) * 2 doubles, nsplit as
 * returned by idiff_groupnorm_nsplit. */
int idiff_groupnorm_nsplit(int B, int HW, int C);
int idiff_groupnorm_stats_f32(const float *x, int C, const float *x2, int C2, int B, int HW, int G, float eps,
                              double *workspace, float *stats, void *stream);
/* Same statistics from the per-tile column sums a producing contraction wrote through epilogue.colstats (one workspace
 * per source tensor, [B, nsplit_i, C_i, 2] fp64); ws2 may be NULL.  No pass over the activations. */
int idiff_groupnorm_finalize_f32(const double *ws1, int nsplit1, int C1, const double *ws2, int nsplit2, int C2, int B,
                                 int HW, int G, float eps, float *stats, void *stream);
/* y[b, p, c] = act(n * (1 + mod[b, c]) + mod[b, Ctot + c]) with n = (x - mean) * rstd * gamma[c] + beta[c]; writes the
 * channel-concatenated output [B, HW, Ctot = C+C2].  mod ([B, ld_mod], scale then shift halves) is the scale-shift
 * conditioning of models/BeatGANsblocks.py:258-332 (`h * (1 + scale) + shift` after the norm); NULL skips it. */
int idiff_groupnorm_apply_f32(const float *x, int C, const float *x2, int C2, int B, int HW, int G,
                              const float *stats, const float *gamma, const float *beta, const float *mod,
                              int64_t ld_mod, int act, float *y, void *stream);
/* idiff_groupnorm_finalize_f32 + idiff_groupnorm_apply_f32 in one launch: the statistics are taken from the producers'
 * column sums (same arithmetic, same result) inside the apply kernel.  C + C2 <= 1024, B <= 65535. */
int idiff_groupnorm_apply_colstats_f32(const float *x, int C, const float *x2, int C2, int B, int HW, int G,
                                       const double *ws1, int nsplit1, const double *ws2, int nsplit2, float eps,
                                       const float *gamma, const float *beta, const float *mod, int64_t ld_mod,
                                       int act, float *y, void *stream);
/* The kernel idiff_groupnorm_apply_f32 / idiff_groupnorm_apply_colstats_f32 would launch for these arguments (same admission code; the
 * pointers are only inspected for null and 16-byte alignment): "rows" (a thread per float4 channel column, grid.y = sample: C + C2 <= 1024
 * and B <= 65535) or "flat" (one grid-stride loop over all float4s; never with column sums).  NULL for arguments the launcher refuses
 * (idiff_last_error says why).  Launches nothing; no reference counterpart. */
const char *idiff_groupnorm_apply_route(const void *x, int C, const void *x2, int C2, int B, int HW, int G, const void *stats,
                                        const void *gamma, const void *beta, const void *y);
const char *idiff_groupnorm_apply_colstats_route(const void *x, int C, const void *x2, int C2, int B, int HW, int G,
                                                 const double *ws1, int nsplit1, const double *ws2, int nsplit2,
                                                 const void *gamma, const void *beta, const void *y);
/* The same GroupNorm as one affine pair per (sample, channel) for a consumer that applies it itself (idiff_conv2d_wino1d_normload_f32):
 * coef [B, C1 + C2, 2] = (a, b) with a = rstd * gamma[c], b = beta[c] - mean * rstd * gamma[c], so that a * x + b is the norm of x.
 * Statistics from the producers' column sums as idiff_groupnorm_finalize_f32 forms them; the pair is formed in fp64 and rounded once. */
int idiff_groupnorm_coef_f32(const double *ws1, int nsplit1, int C1, const double *ws2, int nsplit2, int C2, int B, int HW, int G,
                             float eps, const float *gamma, const float *beta, float *coef, void *stream);

/* Row softmax of x [rows, cols] scaled by `scale` before the exponent (layerspp.py:82-84). In place allowed. */
int idiff_softmax_rows_f32(const float *x, float *y, int64_t rows, int cols, float scale, void *stream);
/* The kernel idiff_softmax_rows_f32 would launch (same admission code; x and y are only inspected for null and 16-byte alignment):
 * "vec<1>" / "vec<2>" / "vec<4>" (16-byte accesses, v_exp_f32: cols a multiple of 4 up to 256 / 512 / 1024, aligned pointers, scale > 0),
 * else the general kernel's branch "regs" (cols <= 1024, the row in registers) or "stream" (three passes over the row); "none" when
 * rows == 0 (nothing to launch).  NULL for arguments the launcher refuses.  Launches nothing; no reference counterpart. */
const char *idiff_softmax_rows_route(const void *x, const void *y, int64_t rows, int cols, float scale);

/* Single-head self-attention over 256 tokens in ONE launch, the [256, 256] logits never leaving the chip (models/layerspp.py:75-91:
 * w = einsum(q, k) * C^-1/2 -> softmax -> einsum(w, v); models/BeatGANsblocks.py:466-491, one head):
 *     out[b, i, :] = sum_j softmax_j(q[b, i] . k[b, j] * scale) v[b, j, :]  (+ bias_v)
 * qk: [B * 256, ld_qk] with q in columns [0, C) and k in [C, 2 C) (the stacked projection the executors already make); vt: V^T as
 * [B, C, 256] (idiff_gemm_*'s weight-times-activation form); out: [B * 256, C].  Both contractions run on fp16 PAIRS (22
 * significand bits, 3 products, fp32 accumulation -- idiff_gemm_pairs_f32's arithmetic), the softmax in fp32.  s_qk / s_v: DEVICE
 * pointers to {s, 1 / s}, the power of two q and k / v are multiplied by before their cut (the caller derives them once per weight:
 * the projections' inputs are GroupNorm outputs); s |q|, s |k|, s |v| must stay below 65504 -- beyond it the outputs are NaN,
 * never finite-and-wrong.  idiff_attention256_ok: 1 for tokens == 256 and C in {128, 256}, 0 otherwise and under
 * IDIFF_NO_FUSED_ATTN / IDIFF_NO_PAIRS / IDIFF_NO_SPLIT (the callers then run the three-launch form on idiff_gemm_f32).
 * All pointers 16-byte aligned, ld_qk a multiple of 4. */
int idiff_attention256_ok(int B, int tokens, int C);
int idiff_attention256_f32(const float *qk, int64_t ld_qk, const float *vt, const float *bias_v, const float *s_qk, const float *s_v,
                           float *out, int B, int tokens, int C, float scale, void *stream);

/* Multi-head self-attention in ONE launch with the keys streamed, the logits never leaving the chip (models/BeatGANsblocks.py:466-526:
 * QKVAttentionLegacy and QKVAttention; the head ORDER of the qkv projection is the caller's row permutation of its weight):
 *     out[b, i, h D + c] = sum_j softmax_j(q_h[b, i] . k_h[b, j] * scale) v_h[b, j, c]  (+ bias_v[h D + c])
 * Head-contiguous operands, C = H D: qk [B * tokens, ld_qk] with q of head h in columns [h D, (h + 1) D) and k of head h in
 * [C + h D, C + (h + 1) D); vt: V^T as [B, C, tokens], row h D + c; out [B * tokens, C].  Arithmetic and s_qk / s_v as
 * idiff_attention256_f32 (fp16 pairs, three products, fp32 accumulation, fp32 softmax); the softmax runs over chunks of 64 keys with a
 * running maximum and sum per query.  s |q|, s |k|, s |v| beyond 65504 give non-finite outputs, never finite-and-wrong.
 * idiff_attention_heads_ok: 1 for D in {32, 64, 128}, H >= 1 with H D <= 1024, tokens a multiple of 64 in [64, 4096], B H <= 2^20;
 * 0 otherwise and under IDIFF_NO_FUSED_ATTN / IDIFF_NO_PAIRS / IDIFF_NO_SPLIT (the callers then run the three-launch form per head).
 * The entry point refuses every other shape and launches nothing.  All pointers 16-byte aligned, ld_qk >= 2 C and a multiple of 4. */
int idiff_attention_heads_ok(int B, int tokens, int H, int D);
int idiff_attention_heads_f32(const float *qk, int64_t ld_qk, const float *vt, const float *bias_v, const float *s_qk, const float *s_v,
                              float *out, int B, int tokens, int H, int D, float scale, void *stream);

/* The kernel instantiation idiff_attention256_f32 / idiff_attention_heads_f32 would launch (the same admission code; the pointers are only
 * inspected for null and 16-byte alignment): "attention256<128>" / "attention256<256>"; "heads<D,NW>" with D in {32, 64, 128} and NW = 8
 * waves of 16 queries where tokens is a multiple of 128, else 4; "none" when B == 0 (nothing to launch).  NULL for arguments the launcher
 * refuses (idiff_last_error says why).  Launches nothing; no reference counterpart. */
const char *idiff_attention256_route(const void *qk, int64_t ld_qk, const void *vt, const void *bias_v, const void *s_qk, const void *s_v,
                                     const void *out, int B, int tokens, int C);
const char *idiff_attention_heads_route(const void *qk, int64_t ld_qk, const void *vt, const void *bias_v, const void *s_qk, const void *s_v,
                                        const void *out, int B, int tokens, int H, int D);

/* y = act(a * alpha + beta_const) elementwise; covers `2*x - 1` (models/ncsnpp.py:264-266), SiLU/ELU of the
 * time embedding, and -out/std when `rowscale` ([n / inner]) is given: y = act(...) * rowscale[i / inner]. */
int idiff_affine_act_f32(const float *a, float *y, int64_t n, float alpha, float beta_const, int act,
                         const float *rowscale, int64_t inner, void *stream);
/* The kernel idiff_affine_act_f32 would launch (same admission code): "vec4" (n and inner multiples of 4, a and y 16-byte aligned) or
 * "scalar"; "none" when n == 0.  NULL for arguments the launcher refuses.  The same for idiff_add_scale_f32 (a, b, y aligned, n % 4 == 0)
 * and idiff_concat_cols_f32 (Ca and Cb multiples of 4, a, b, out aligned; "none" when rows == 0).  They launch nothing; no reference
 * counterpart. */
const char *idiff_affine_act_route(const void *a, const void *y, int64_t n, const void *rowscale, int64_t inner);
const char *idiff_add_scale_route(const void *a, const void *b, const void *y, int64_t n);
const char *idiff_concat_cols_route(const void *a, int Ca, const void *b, int Cb, const void *out, int64_t rows);
/* y = (a + b) * scale (skip-rescale adds, models/ncsnpp.py:303-307). */
int idiff_add_scale_f32(const float *a, const float *b, float *y, int64_t n, float scale, void *stream);
/* Gaussian Fourier features: out[b] = [sin(2*pi*t[b]*W), cos(2*pi*t[b]*W)] (models/layerspp.py:39-41). */
int idiff_fourier_embed_f32(const float *t, const float *W, float *out, int B, int half, void *stream);
/* Sinusoidal timestep embedding, dim even.  mode 0: DDPM (models/layers.py:524-538, [sin, cos], log(max)/(half-1));
 * mode 1: guided-diffusion / BeatGANs (models/BeatGANs_nn.py:107-125, [cos, sin], log(max)/half). */
int idiff_positional_embed_f32(const float *t, float *out, int B, int dim, float max_positions, int mode, void *stream);
/* out[r, :] = cat(a[r, :Ca], b[r, :Cb]) for r < rows (channel concat of NHWC tensors / fcn's cat([x, t])). */
int idiff_concat_cols_f32(const float *a, int Ca, const float *b, int Cb, float *out, int64_t rows, void *stream);
/* Layout changes at the model boundary: NCHW [B, C, HW] <-> NHWC [B, HW, Cpad] (zero-filled pad channels),
 * with an optional affine on the way in (alpha * x + beta) and a per-sample scale on the way out. */
int idiff_nchw_to_nhwc_f32(const float *x, float *y, int B, int C, int HW, int Cpad, float alpha, float beta,
                           void *stream);
int idiff_nhwc_to_nchw_f32(const float *x, float *y, int B, int C, int HW, int Cpad, const float *rowscale,
                           void *stream);
/* Perturbation of one data point into `rows` noisy copies (dim_reduction.py:178-182):
 * out[r, :] = mean_coeff[r] * x[:] + std[r] * z[r, :]; mean_coeff NULL means 1 (VE SDE, sde_lib.py:346). */
int idiff_perturb_f32(const float *x, const float *z, const float *std_, const float *mean_coeff, float *out,
                      int64_t rows, int64_t D, void *stream);
/* Same perturbation with the Gaussian draw generated in the kernel (replaces `z = torch.randn_like(batch)` of
 * dim_reduction.py:181): Philox4x32-10 keyed by `seed`, counter = position of the element in the point's logical
 * [total_rows, D] noise matrix (row0 = first row of this launch), Box-Muller.  The draw for an element does not depend on
 * how rows are cut into launches.  D % 4 == 0.  z_out (optional, [rows, D]) receives the N(0,1) values for tests. */
int idiff_perturb_randn_f32(const float *x, const float *std_, const float *mean_coeff, float *out, int64_t rows,
                            int64_t D, int64_t row0, uint64_t seed, float *z_out, void *stream);
/* Nearest x2 upsample / 2x2 mean downsample of NHWC tensors (naive_upsample_2d / naive_downsample_2d,
 * models/up_or_down_sampling.py:59-69; BeatGANs Upsample/Downsample, models/BeatGANsblocks.py:335-396). */
int idiff_resample2x_nhwc_f32(const float *x, float *y, int B, int H, int W, int C, int up, void *stream);

/* ------------------------------------------------------------------ spectrum of the centred score matrix */

/* Replaces `scores - scores.mean(0)` + `torch.linalg.svd(...)` of dim_reduction.py:193-198 for a batch of P
 * score matrices S[p] (M x D fp32, row-major, contiguous): D singular values per matrix, descending; for M < D the
 * reference's min(M, D) values are the leading M of them (the rest are zeros up to rounding).  Method: fp64 column means -> fp64 Gram of the centred columns on v_mfma_f64_16x16x4 ->
 * tridiagonalisation (fp64, idiff_symtridiag_f64) -> Sturm bisection -> sqrt.  Products of fp32 inputs are exact in
 * fp64, so the squared condition number costs nothing at the 1e-4 tolerance.
 * workspace: idiff_spectrum_workspace_bytes(P, M, D) bytes; sv: [P, D] fp32.
 * `eig_out` (optional, [P, D] fp64) receives the Gram eigenvalues (ascending) for diagnosis. */
int64_t idiff_spectrum_workspace_bytes(int P, int M, int D);
int idiff_spectrum_f32(const float *S, int P, int M, int D, void *workspace, int64_t workspace_bytes, float *sv,
                       double *eig_out, void *stream);
/* The stages, exported for the parity tests and the profiler. */
/* scratch: P * 32 * D doubles (deterministic two-stage column sums). */
int idiff_colmean_f64(const float *S, int P, int M, int D, double *mean, double *scratch, void *stream);
int idiff_centered_gram_f64(const float *S, const double *mean, int P, int M, int D, double *G, void *stream);
/* Row-sharded single point (one point's rows spread over the ranks): the upper triangle of the
 * centred Gram for rows [row0, row1) only (tile-aligned: multiples of 64, or D), so that block b can be all-reduced
 * while block b + 1 is computed; idiff_symmetrize_upper_f64 mirrors the reduced upper triangle afterwards.  G is
 * [D][D] fp64 and should be zeroed first (the part left of a block's diagonal tile is not written). */
int idiff_centered_gram_rows_f64(const float *S, const double *mean, int M, int D, int row0, int row1, double *G,
                                 void *stream);
int idiff_symmetrize_upper_f64(double *G, int D, void *stream);
/* G [P][D][D] symmetric (both triangles), overwritten -> diag/offdiag [P][D] of a similar tridiagonal matrix.
 * D <= 128: one workgroup per matrix in LDS.  Larger D: two-stage -- blocked reduction to a band of half-width 32
 * (CholeskyQR2 + Householder-reconstruction panels, compact-WY rank-64 trailing updates on v_mfma_f64_16x16x4) and
 * bulge chasing on the compact band; if the panels' annihilation residual exceeds 1e-11 ||G||_F the outputs are NaN
 * (never a silently wrong spectrum; IDIFF_TRIDIAG_ONESTAGE selects the unblocked Householder sweep instead).
 * scratch: idiff_symtridiag_scratch_doubles(D) doubles (shared by the P matrices, which are processed in turn). */
int64_t idiff_symtridiag_scratch_doubles(int D);
/* stage 1 alone (D > 128): on return the first D * idiff_symband_ld() doubles of scratch hold the lower band,
 * band[j * ld + k] = B[j + k][j], k <= 32 (the rest of a column is bulge room, zero: the kernel that extracts the band writes it,
 * and the two zero columns behind the band, whatever the scratch held). */
int idiff_symband_ld(void);
int idiff_symband_f64(double *G, int D, double *scratch, void *stream);
int idiff_symtridiag_f64(double *G, int P, int D, double *diag, double *offdiag, double *scratch, void *stream);
/* Which path idiff_symtridiag_f64 takes for a D x D matrix on the current device: 0 LDS-resident (D <= 128), 1 two-stage
 * with the single-launch systolic bulge chase, 2 two-stage with the wavefront chase (the systolic kernel's
 * ceil(D / 32) mutually waiting workgroups exceed HALF of what the device can hold resident -- asked of the
 * runtime per device -- or IDIFF_CHASE_WAVEFRONT is set), 3 one-stage sweep (IDIFF_TRIDIAG_ONESTAGE). */
int idiff_symtridiag_plan(int D);
/* diag, offdiag [P][D] -> eig [P][D] ascending.  offdiag[p][i] couples rows i and i + 1, so offdiag[p][D - 1] is the unused entry:
 * idiff_symtridiag_f64 writes 0 there on every path, idiff_tridiag_eigvals_f64 never reads it (any value, a NaN too, changes nothing).
 * A NaN or Inf in any entry that IS read turns the matrix's D eigenvalues into NaN. */
int idiff_tridiag_eigvals_f64(const double *diag, const double *offdiag, int P, int D, double *eig, void *stream);

/* The tangent side of the spectrum: T [D, k] row-major with orthonormal columns spanning the invariant subspace of the k SMALLEST
 * eigenvalues of the symmetric positive semi-definite G [D, D] (both triangles), ritz [k] the Ritz values of G on it (ascending,
 * column i of T belongs to ritz[i]) and resid [1] = |G T - T diag(ritz)|_F, evaluated from the T that is returned.  At small t
 * the score vectors span the normal space, so for k = the point's intrinsic dimension T is the estimated tangent space (the
 * `v` the reference's torch.linalg.svd returns and drops, dim_reduction.py:197) and its orthogonal complement the normal space.
 * Method: Cholesky of G + eps I, eps = 8 D 2^-53 max_i G_ii (blocked, trailing updates on v_mfma_f64_16x16x4), four steps of
 * inverse subspace iteration from a fixed Philox block (the same result on every call), each followed by CholeskyQR2, then
 * Rayleigh-Ritz with a cyclic Jacobi eigensolver of the k x k projection.  The contraction per step is lambda_k / lambda_k+1:
 * the gap the ID rule detects.  G is only read (the factor lives in the scratch).  A non-positive pivot -- G not positive
 * semi-definite to rounding, or a start block that lost rank -- and a NaN in G turn T, ritz and resid into NaN; no input can hang
 * the call.  Needs 1 <= k <= 128 and k < D (IDIFF_EINVAL otherwise, as for null pointers; nothing is launched).  scratch:
 * idiff_sym_lowvecs_scratch_doubles(D, k) doubles (0 for arguments the call refuses).  No host synchronisation. */
int64_t idiff_sym_lowvecs_scratch_doubles(int D, int k);
int idiff_sym_lowvecs_f64(double *G, int D, int k, double *T, double *ritz, double *resid, double *scratch, void *stream);

/* The other end of the spectrum: the k LARGEST eigenpairs of a symmetric fp64 matrix K [N, N] (both triangles) that may be
 * indefinite -- the centred geodesic kernel of Isomap.  V [N, k] row-major with orthonormal columns, ritz [k] descending (column i
 * of V belongs to ritz[i]), resid [1] = |K V - V diag(ritz)|_F evaluated from the V that is returned.  Method: block subspace
 * iteration on p columns (k <= p <= 128, p < N) with a Chebyshev filter: `sweeps` times a polynomial of degree `degree` in K that
 * stays within [-1, 1] on [lo, hi] and equals 1 at `top`, every step Y <- alpha K X + beta X + gamma Z on v_mfma_f64_16x16x4 with K
 * read once, each sweep followed by a shifted CholeskyQR3; then Rayleigh-Ritz (cyclic Jacobi) on the p columns, of which the k
 * largest pairs are returned.  The caller, who has the eigenvalues, sets lo = lambda_min, hi = lambda_(p+1), top = lambda_1 and
 * bounds the degree (python: _lib.topvecs_plan): all loops are fixed, nothing waits.  K is only read.  A NaN in K and a failed
 * p x p factorisation turn V, ritz and resid into NaN.  Needs 1 <= k <= 64, k < N <= 2^20, lo < hi <= top finite, 1 <= degree <= 64,
 * degree * sweeps <= 4096 (IDIFF_EINVAL otherwise, as for null pointers; nothing is launched).  scratch:
 * idiff_sym_topvecs_scratch_doubles(N, k, p) doubles (0 for arguments the call refuses).  No host synchronisation. */
int64_t idiff_sym_topvecs_scratch_doubles(int N, int k, int p);
int idiff_sym_topvecs_f64(const double *K, int N, int k, int p, double lo, double hi, double top, int degree, int sweeps, double *V,
                          double *ritz, double *resid, double *scratch, void *stream);

/* ------------------------------------------------------------------ exact k nearest neighbours */

/* Replaces `NearestNeighbors(n_neighbors=k+1, algorithm='ball_tree').fit(X).kneighbors(X)` of mle.py:19-20 / :47-48 /
 * :80-81 (without the self column).  X is [N, D] fp32, row-major, contiguous.  For every row i: the k nearest OTHER rows
 * (self excluded by index), by ascending Euclidean distance, equal distances by lower index; dist [N, k] fp64 holds
 * sqrt(sum_d (x_id - x_jd)^2) evaluated in fp64 from the fp32 inputs, idx [N, k] the row indices.  Exact: candidates from
 * an fp32 pass on v_mfma_f32_32x32x2_f32 (centred data, K' = min(N - 1, k + 16) per row), refined in fp64, with a bound
 * on the fp32 pass's error deciding per row whether the candidates are provably enough; rows where they are not are done
 * again by fp64 brute force, and *n_exact_rows (device int) receives their count.  Needs 2 <= N, 1 <= D, 1 <= k <= 64,
 * k <= N - 1 (IDIFF_EINVAL otherwise).  workspace: idiff_knn_workspace_bytes(N, D, k) bytes, 256-byte aligned (0 for
 * arguments the call refuses). */
int64_t idiff_knn_workspace_bytes(int N, int D, int k);
int idiff_knn_f32(const float *X, int N, int D, int k, void *workspace, int64_t workspace_bytes, double *dist, int64_t *idx,
                  int *n_exact_rows, void *stream);

/* ------------------------------------------------------------------ geodesic distances (Isomap) */

/* The three device stages of `Isomap(n_neighbors, n_components).fit(X).reconstruction_error()` of isomap.py:56-58 between
 * the neighbour search and the eigenvalues, all fp64, row-major, contiguous.  Each launches on `stream`, does not
 * synchronise and does not allocate.  Needs 1 <= N <= 2^20 and non-null pointers (IDIFF_EINVAL otherwise, nothing launched).
 *
 * knn_graph: dist, idx [N, k] as idiff_knn_f32 writes them (0 <= k <= N - 1; both may be null only for k = 0) -> G [N, N]
 * with G[i, i] = 0, G[i, j] = the distance where j is among i's neighbours or i among j's (the smaller where both),
 * +inf elsewhere: the graph scipy.sparse.csgraph.shortest_path(directed=False) reads from sklearn's kneighbors_graph.
 * Deterministic (no atomics); an index outside [0, N) is dropped.
 *
 * apsp: all-pairs shortest paths in place, blocked Floyd-Warshall on tiles of idiff_apsp_tile() = 64 (3 launches per
 * diagonal tile; any N, no padding asked of the caller).  G holds non-negative weights, 0 on the diagonal and +inf for
 * "no edge", no NaN; an unreachable pair stays +inf and the diagonal stays 0 exactly.  2 N^3 fp64 operations.
 *
 * double_center: D [N, N] (symmetric, only read) -> K = -1/2 J (D o D) J, J = I - 1 1^T / N, and *fro2 = ||K||_F^2 (device
 * scalar).  scratch: idiff_double_center_scratch_doubles(N) doubles (0 for an N the call refuses); on return its first N hold
 * the row (= column) means of D o D and scratch[2 N] their grand mean.  Fixed summation trees: the same bits on every launch. */
int idiff_apsp_tile(void);
int idiff_knn_graph_f64(const double *dist, const int64_t *idx, int N, int k, double *G, void *stream);
int idiff_apsp_f64(double *G, int N, void *stream);
int64_t idiff_double_center_scratch_doubles(int N);
int idiff_double_center_f64(const double *D, int N, double *K, double *fro2, double *scratch, void *stream);

/* Points that were not in the fit (sklearn.manifold.Isomap.transform), fp64 results, row-major, contiguous, no host
 * synchronisation, no allocation.
 *
 * knn_cross: for every row of Xq [M, D] the k nearest rows of X [N, D] (both fp32) by fp64 brute force: dist [M, k] =
 * sqrt(sum_d (q_d - x_d)^2) evaluated in fp64 from the fp32 inputs, ascending, equal distances by lower index; idx [M, k] the
 * rows of X.  No row is excluded.  Needs 1 <= M, 1 <= N <= 2^20, 1 <= D, 1 <= k <= 64, k <= N.  workspace:
 * idiff_knn_cross_workspace_bytes(M, N) bytes, 8-byte aligned (0 for arguments the call refuses).
 *
 * isomap_project: dist, idx [M, k] as knn_cross writes them, D [N, N] the fitted geodesic matrix, A [N, c] the eigenvectors
 * divided by sqrt(eigenvalue), colmean [N] and grand [1] (device) the column means and the grand mean of -1/2 D o D over the fit
 * -> Z [M, c] with g_ij = min_n (dist[i, n] + D[idx[i, n], j]), g'_ij = -1/2 g_ij^2 and
 * Z[i, :] = sum_j (g'_ij - colmean_j - mean_j g'_ij + grand) A[j, :], in one launch: the [M, N] geodesic matrix is never
 * written (the columns j are walked once per 8 components: one pass for c <= 8).
 * Fixed summation trees: the same bits on every launch.  An index outside [0, N) is dropped.  Needs 1 <= M, 1 <= N <= 2^20,
 * 1 <= k <= 64, 1 <= c <= 64.  scratch: idiff_isomap_project_scratch_doubles(c) doubles (0 for a c the call refuses). */
int64_t idiff_knn_cross_workspace_bytes(int M, int N);
int idiff_knn_cross_f64(const float *Xq, int M, const float *X, int N, int D, int k, void *workspace, int64_t workspace_bytes,
                        double *dist, int64_t *idx, void *stream);
int64_t idiff_isomap_project_scratch_doubles(int c);
int idiff_isomap_project_f64(const double *dist, const int64_t *idx, int M, int k, const double *D, int N, const double *A, int c,
                             const double *colmean, const double *grand, double *Z, double *scratch, void *stream);

/* A disconnected neighbourhood graph joined the way scikit-learn joins it (sklearn.utils.graph._fix_connected_components,
 * mode="distance"): between every two components one edge, the closest pair of points.  No host synchronisation, no allocation;
 * IDIFF_EINVAL and nothing launched for arguments outside what is stated.
 *
 * component_labels: D [N, N] a shortest-path matrix (symmetric pattern of finite entries, finite diagonal), 1 <= N <= 2^20 ->
 * labels [N] in 0 .. C - 1, numbered in the order of each component's smallest vertex (scipy's connected_components numbers
 * them so), and *count = C (device scalar).  scratch: N int32.
 *
 * component_bridges: X [N, D] fp32, labels [N] with every value of 0 .. C - 1 present, 2 <= C <= 1024 -> for i = 1 .. C - 1 and
 * j < i, at position i (i - 1) / 2 + j: bi = the point a of component i and bj = the point b of component j with the smallest
 * sqrt(sum_d (a_d - b_d)^2), evaluated in fp64 from the fp32 coordinates (fused multiply-adds in ascending d), bw that distance.
 * Equal distances: the smallest a, then the smallest b, whatever the launch order (two passes of unsigned 64-bit atomic
 * minima; no floating-point atomics).  A label outside 0 .. C - 1 is dropped, never an address; a pair of components without
 * points comes back as (-1, -1, +inf).  workspace: idiff_component_bridges_workspace_bytes(C) bytes, 8-byte aligned (0 for a
 * C the call refuses).
 *
 * minplus: C = min(C, A (x) B) in the (min, +) semiring, A [m, p], B [p, n], C [m, n] fp64 with row pitches lda, ldb, ldc (in
 * doubles, at least the row lengths), 1 <= m, n, p <= 2^20; C may not overlap A or B.  The device function of phases 2 and 3 of
 * apsp over every pivot tile of p.  Non-negative entries or +inf, no NaN.  2 m n p fp64 operations.
 *
 * symmetrize_min: G = min(G, G^T) in place, G [N, N]: the tile pass that ends knn_graph. */
int idiff_component_labels_f64(const double *D, int N, int32_t *labels, int32_t *count, int32_t *scratch, void *stream);
int64_t idiff_component_bridges_workspace_bytes(int C);
int idiff_component_bridges_f64(const float *X, int N, int D, const int32_t *labels, int C, void *workspace, int64_t workspace_bytes,
                                int64_t *bi, int64_t *bj, double *bw, void *stream);
int idiff_minplus_f64(const double *A, int64_t lda, const double *B, int64_t ldb, double *C, int64_t ldc, int m, int n, int p,
                      void *stream);
int idiff_symmetrize_min_f64(double *G, int N, void *stream);

/* ------------------------------------------------------------------ image manifolds of known dimension */

/* The two fixed image manifolds of lightning_data_modules/SyntheticDataset.py:81-183, one workgroup per image, out
 * [N, S, S] fp32 (16-byte aligned).  Both need S a multiple of 4 in [4, 64], 1 <= K <= 1024 and N * S * S < 2^31
 * (IDIFF_EINVAL otherwise, nothing launched; N = 0 is a no-op).  The tables are the caller's: the kernels index pixels
 * only, so a rectangle or centre outside the image cannot make them leave `out`, but the Python wrapper refuses one.
 *
 * squares: rects [K, 3] int32 = (row0, col0, side) of square k, coef [N, K] fp32.  out[n, p] = sum_k coef[n, k] [p in rect_k]
 * as a sequential fp32 chain in ascending k from +0: bit-equal to FixedSquaresManifold for coef = fl32 of its draws.
 *
 * gaussians: centres [K, 2] int32 = (row, column), std [N, K] fp64.  v[i, j] = sum_k exp(d_k ((i - row_k)^2 + (j - col_k)^2))
 * / (sqrt(2 pi) std_k), d_k = -1 / (2 std_k^2), accumulated in fp64 and rounded once to fp32; out = (v - min v) / (max v - min v)
 * in fp32 with a correctly rounded division (FixedGaussiansManifold works in fp32 throughout: equal within
 * (K + 4) 2^-24 max / (max - min), not bit for bit). */
int idiff_render_squares_f32(const float *coef, const int *rects, float *out, int N, int K, int S, void *stream);
int idiff_render_gaussians_f32(const double *std, const int *centres, float *out, int N, int K, int S, void *stream);

/* ------------------------------------------------------------------ exact score of a noised union of k-spheres */

/* The mixture of J uniform distributions on R_j S^{k_j} inside span Q_j (Q_j [n, p_j] orthonormal, p_j = k_j + 1), convolved with
 * N(0, sigma^2 I): out[b, :] = mult[b] (-x_b + sum_j w_j (R_j A_j / r_j) Q_j Q_j^T x_b), i.e. mult[b] sigma[b]^2 times the score
 * (csrc/ksphere_union.hip has the formulas; models/ksphere_union_exact.py: reference_score restates them in numpy).  One launch, x
 * read once, out written once, every operation between the two in fp64, one rounding to fp32.
 *
 * x, out [B, n] fp32; Qcat [n, P] fp64 row-major = [Q_0 | ... | Q_{J-1}]; sigma [B] fp32; mult [B] fp32 or NULL (= 1); all device
 * pointers.  comp is a HOST table [J, 4] of doubles (first column off_j, columns p_j, radius R_j, log pi_j): the frames must tile
 * [0, P) in order.  A row in which a component with kappa_j = r_j R_j / sigma^2 < max(32, p_j^2 / 16) cannot be shown to have
 * weight exactly 0 in fp64, or that has no component above that threshold, is REFUSED: written as NaN, and *refused (device int32,
 * zeroed by the caller) is incremented.
 *
 * idiff_ksphere_union_ok (host only, nothing launched) = 1 where the launch is served: 1 <= J <= 8, J <= P <= 128 J (the launch also
 * checks p_j <= 128 and p_j <= n), and, Qcat being kept in LDS beside at least two waves' tiles, with Pst = 16 ceil(P / 16) + 2 and
 * n4 = 4 ceil(n / 4):   8 n Pst + 384 + 2 (128 Pst + 64 n4 + 4224) <= 163840 bytes. */
int idiff_ksphere_union_ok(int n, int J, int P);
int idiff_ksphere_union_score_f32(const float *x, const double *Qcat, const double *comp, const float *sigma, const float *mult,
                                  float *out, int *refused, int B, int n, int J, int P, void *stream);

/* ------------------------------------------------------------------ local PCA: per-point spectrum and tangent basis */

/* Fukunaga-Olsen's estimator in its original, per-point form (the reference reaches it through R's pcaLocalDimEst; no reference
 * counterpart in code).  Query q has a centre row centre[q] and k neighbour rows idx[q, :] of X [N, D] fp32 (row-major, contiguous);
 * with m = k + 1 rows in the neighbourhood (the centre and its neighbours), y_j = x_j - x_centre formed in fp64 before any product,
 * G = Y Y^T (m x m, v_mfma_f64_16x16x4_f64, D streamed through LDS in chunks of idiff_local_pca_chunk() columns) and
 * B = J G J / (m - 1), J = I - 1 1^T / m, whose non-zero eigenvalues are those of the neighbourhood's sample covariance.  One
 * workgroup per query solves B by cyclic Jacobi in LDS; nothing [m, D] or [D, D] is written to HBM.  One launch, no host
 * synchronisation, no allocation, no workspace.
 *
 * eig [Q, r] fp64, r = min(k, D): the r largest eigenvalues, descending, clamped at 0 (the others are zero by construction).
 * basis [Q, n_vec, D] fp64 (NULL allowed only for n_vec = 0; 0 <= n_vec <= r): row v = Y^T J u_v / sqrt((m - 1) lambda_v), the unit
 * eigenvector of the covariance, its component of largest magnitude positive (lowest index on ties); a row whose eigenvalue is
 * <= m 2^-52 lambda_1, and every row when lambda_1 = 0, is NaN.
 * status [Q] int32: 0 converged; 1 the sweep cap was reached with the off-diagonal norm above m 2^-52 ||B||_F (the results are
 * what the last sweep left); 2 an index of the query lies outside [0, N): THE KERNEL CHECKS every index before it reads a row of X,
 * so the caller need not; such a query's eig and basis rows are NaN; 3 ||B||_F is not finite (a NaN or Inf among the query's rows, or
 * an overflow): no sweep is run and eig and basis are NaN or Inf as they fall, never a spectrum to read a dimension from.
 *
 * Needs 1 <= N, 1 <= D, 2 <= k <= 64, 0 <= n_vec <= min(k, D), 0 <= Q and non-null pointers (IDIFF_EINVAL otherwise, nothing
 * launched; Q = 0 is a no-op).  idiff_local_pca_ok (host only) = 1 where the sizes are served.  centre [Q] and idx [Q, k] are
 * int64, as idiff_knn_f32 writes them. */
int idiff_local_pca_ok(int N, int D, int k, int n_vec);
int idiff_local_pca_chunk(void);
int idiff_local_pca_f64(const float *X, int N, int D, const int64_t *centre, const int64_t *idx, int Q, int k, int n_vec,
                        double *eig, double *basis, int *status, void *stream);

/* ------------------------------------------------------------------ simplex skewness: per-point ID across neighbourhood sizes */

/* Expected Simplex Skewness with d = 1 (Johnsson, Soneson and Fontes 2015; the reference's R package has it as essLocalDimEst; no
 * reference counterpart in code).  Query q has a centre row centre[q] and k neighbour rows idx[q, :] of X [N, D] fp32 (row-major,
 * contiguous), the neighbours in ascending distance as idiff_knn_f32 writes them, so that the neighbourhood of size k' <= k is the
 * centre and the first k' columns.  y_j = x_j - x_centre is formed in fp64 before any product and G = Y Y^T over the m = k + 1 rows
 * on v_mfma_f64_16x16x4_f64, D streamed through LDS in chunks, exactly as idiff_local_pca_f64 does.  Then, for every scale
 * k' = scales[s] with m' = k' + 1, on the leading m' x m' block of G: B = J G J, J = I - 1 1^T / m' (the Gram matrix of the rows
 * centred on their own mean: B_ij = G_ij - (r_i + r_j) + g with the block's row means r and grand mean g summed in a fixed order), and
 * over all pairs i < j < m'
 *     ess[q, s, 0] = sum sqrt(max(0, B_ii B_jj - B_ij^2)) / W     the weighted mean of |sin| of the angle between two centred rows
 *     ess[q, s, 1] = sum |B_ij| / W                               the weighted mean of |cos|
 *     ess[q, s, 2] = W = sum sqrt(B_ii) sqrt(B_jj)                the weight sum
 * One workgroup per query, one launch, no atomics, no host synchronisation, no allocation, no workspace; nothing [m, D] or [m, m]
 * is written to HBM.  The bits of ess[q, s, :] depend on the query's first scales[s] + 1 rows alone: not on k, not on the other
 * scales of the list, not on Q or on the other queries of the launch.
 *
 * scales: HOST array of S neighbourhood sizes, strictly ascending, 2 <= scales[s] <= k (read before the launch, not kept).
 * ess [Q, S, 3] fp64.  status [Q] int32: 0 served; 2 an index of the query lies outside [0, N): THE KERNEL CHECKS every index before
 * it reads a row of X, so the caller need not; the query's ess is NaN; 3 a value of the query's k + 1 rows is not finite (or |y_j|^2
 * overflows): ess is NaN at every scale; 4 at least one scale has W = 0 exactly (its rows are identical): that scale's two means are
 * NaN and its W is 0, the other scales are served.
 *
 * Needs 1 <= N, 1 <= D, 2 <= k <= 64, 1 <= S <= 16, 0 <= Q, the scales as above and non-null pointers (IDIFF_EINVAL otherwise,
 * nothing launched; Q = 0 is a no-op).  idiff_simplex_skewness_ok (host only) = 1 where the sizes are served.  centre [Q] and
 * idx [Q, k] are int64, as idiff_knn_f32 writes them. */
int idiff_simplex_skewness_ok(int N, int D, int k, int S);
int idiff_simplex_skewness_f64(const float *X, int N, int D, const int64_t *centre, const int64_t *idx, int Q, int k,
                               const int *scales, int S, double *ess, int *status, void *stream);

/* ------------------------------------------------------------------ score of the empirical distribution of a point cloud */

/* The N points x_i of a cloud, each with weight 1 / N, convolved with N(0, sigma^2 I) -- exact for any finite data set, no training:
 *   w_bi = softmax_i(-|x_b - x_i|^2 / (2 sigma_b^2)),   out[b, :] = mult[b] (sum_i w_bi x_i - x_b),   ess[b] = 1 / sum_i w_bi^2
 * i.e. mult[b] sigma[b]^2 times the score, and the effective number of points the row's estimate rests on.  The cloud is passed
 * centred (_lib.empirical_pack): c [D] its fp64 column mean, Y [N, D4] fp64 row-major with D4 = 4 ceil(D / 4) and zero padding,
 * y_i = x_i - c, and h [N] = |y_i|^2 / 2.  The kernel forms q_b = x_b - c in fp64, the logits (q_b . y_i - h_i) / sigma_b^2 and both
 * products on v_mfma_f64_16x16x4_f64 with a streamed softmax (csrc/empirical_score.hip); logits and weights stay in registers, there
 * is no [B, N] buffer and no workspace, and the result is rounded to fp32 once.  One launch, no atomics: the same inputs give the same
 * bits, and a row's result does not depend on which other rows are in the launch.
 *
 * x, out [B, D] fp32; sigma [B] fp32; mult [B] fp32 or NULL (= 1); ess [B] fp32 or NULL; all device pointers, Y 16-byte aligned.
 * A row whose x is not finite or whose sigma is not a positive finite number is written as NaN (out and ess); no other row is
 * affected.  IDIFF_EINVAL before any device call for a null pointer (mult and ess excepted), B < 0, N < 1, D < 1 or a shape
 * idiff_empirical_score_ok (host only) denies: it serves 1 <= D <= 192 (a wave keeps its [16, D] fp64 output and its q tile in
 * registers) and 1 <= N < 2^31 - 32.  B = 0 is a no-op. */
int idiff_empirical_score_ok(int64_t N, int D);
int idiff_empirical_score_f32(const float *x, const double *Y, const double *h, const double *c, const float *sigma, const float *mult,
                              float *out, float *ess, int B, int64_t N, int D, void *stream);

/* The Jacobian of that score in closed form, no sampling: with d_i = x_i - x_b, w_bi as above and m_b = sum_i w_bi d_i,
 *   I + sigma_b^2 grad s(x_b)  =  C[b]  :=  sum_i w_bi (d_i - m_b)(d_i - m_b)^T / sigma_b^2
 * the softmax-weighted covariance of the cloud seen from x_b in units of sigma_b^2: eigenvalues near 1 along the tangent, near 0 along
 * the normal.  A query is a (point, sigma) pair; a launch mixes points and bandwidths freely.  X [N, D] is the RAW fp32 cloud (not the
 * fp64 pack): d = (double)x_i - (double)x_b is one rounding and does not depend on the cloud's offset.  One workgroup per query, two
 * passes over the cloud in one launch (the largest logit; then every logit recomputed by the same instructions, w = exp(l - max), no
 * rescaling), sum w d d^T on v_mfma_f64_16x16x4_f64 over the 16 x 16 blocks of the upper triangle, mirrored at the store: C[b] is
 * symmetric to the bit (csrc/empirical_jacobian.hip).  No atomics, no workspace: the same inputs give the same bits, and a query's
 * result does not depend on which other queries share its launch.
 *
 * x [B, D], sigma [B] fp32; C [B, D, D] fp64, both triangles; mean [B, D] fp64 = sum_i w_bi d_i; ess [B] fp32 = 1 / sum_i w_bi^2; all
 * device pointers, all required.  A query whose x is not finite or whose sigma is not a positive finite number is written as NaN in
 * all three outputs; no other query is affected.  IDIFF_EINVAL before any device call for a null or misaligned pointer, B < 0, N < 1,
 * D < 1 or a shape idiff_empirical_jacobian_ok (host only) denies: it serves 1 <= D <= 192 (the four waves of a workgroup keep the 78
 * upper blocks of C in registers) and 1 <= N < 2^31 - 32.  B = 0 is a no-op. */
int idiff_empirical_jacobian_ok(int64_t N, int D);
int idiff_empirical_jacobian_f64(const float *x, const float *X, const float *sigma, double *C, double *mean, float *ess,
                                 int B, int64_t N, int D, void *stream);

/* FLIPD of the same empirical distribution (Kamkari et al. 2024; LIDL of Tempczyk et al. 2022 through the Fokker-Planck equation):
 * D + sigma^2 (tr grad s + |s|^2) of the score s above, which for a cloud is the softmax-weighted mean of squared distances
 *   flipd[p, j] = sum_i w_i r_i^2 / sigma_j^2,   r_i^2 = |x_i - x_p|^2,   w = softmax_i(-r_i^2 / (2 sigma_j^2)),   ess[p, j] = 1 / sum_i w_i^2
 * a real-valued local dimension per (query, bandwidth).  Nothing of width D is kept per query, so D only streams: any 1 <= D <= 65536
 * is served.  The cloud is read as _lib.empirical_pack makes it (Y, h, c as for idiff_empirical_score_f32); q = x - c is formed in
 * fp64 and r^2 = max(0, |q|^2 + 2 h_i - 2 q . y_i) with the product on v_mfma_f64_16x16x4_f64, q and Y staged through LDS in chunks of
 * 32 columns (csrc/empirical_flipd.hip).  All S bandwidths share one r^2 tile and one running minimum per query.
 *
 * x [P, D] fp32; sigmas [S] fp32, 1 <= S <= 32; exclude [P] int32 or NULL: the cloud row left out of query p's softmax (leave-one-out
 * when the query is a cloud point), any value outside [0, N) excluding nothing; flipd [P, S] fp64; ess [P, S] fp32.  N is cut into
 * `splits` contiguous ranges of ceil(N / splits) points across workgroups; their partials (r^2 min, sum e, sum e^2, sum e r^2) go to
 * `workspace` (idiff_empirical_flipd_workspace_doubles(P, S, splits) = 4 P S splits doubles, `workspace_doubles` what the caller
 * has) and a second small launch merges them in range order, an empty range as the neutral element.  No atomics: the same inputs and
 * the same `splits` give the same bits.  idiff_empirical_flipd_splits (host only, launches nothing) is the default: two workgroups a
 * CU when P / 64 alone gives fewer than 256, never a range below 64 points, 1 when the queries fill the card.
 *
 * A query row that is not finite is NaN in its row of both outputs, a sigma that is not positive and finite in its column; a query
 * with no admissible point (N = 1 and that point excluded) is NaN.  Nonzero (idiff_last_error says why) before any launch for a null
 * or misaligned pointer, N < 1, D < 1, S < 1, a shape idiff_empirical_flipd_ok denies, splits outside 1 .. 65535 or a workspace that
 * is too small.  P = 0 is a no-op.  No host synchronisation. */
int idiff_empirical_flipd_ok(int64_t N, int D, int S);
int64_t idiff_empirical_flipd_workspace_doubles(int64_t P, int S, int splits);
int idiff_empirical_flipd_splits(int64_t P, int64_t N, int D);
int idiff_empirical_flipd_f64(const float *x, const double *Y, const double *h, const double *c, const float *sigmas, const int *exclude,
                              double *flipd, float *ess, double *workspace, int64_t workspace_doubles, int64_t P, int64_t N, int D, int S,
                              int splits, void *stream);

/* ------------------------------------------------------------------ training the fcn score network (csrc/fcn_train.hip) */

/* The two contractions the backward pass of a Linear + ELU layer needs beside idiff_gemm_f32, on v_mfma_f32_32x32x2_f32 (a k-ordered
 * chain of fp32 fmas: |C - exact| <= K 2^-24 sum_k |a_k b_k|).  No split of K, no atomics, no workspace: the same bits on every run.
 *
 *   gemm_nn:  C[M, N] = (A[M, K] . Bm[K, N]) (*) g(P),  A rows K-contiguous (lda), Bm rows N-contiguous (ldb) -- an nn.Linear weight
 *             [out, in] as it lies gives the data gradient dH = dA . W.  P [M, N] (ldp) or NULL: the ELU OUTPUT the gradient flows
 *             back through, g(a) = a > 0 ? 1 : a + 1 (= ELU' written in terms of the output), applied as one fma.
 *   gemm_tn:  C[M, N] = At[K, M]^T . Bm[K, N], both operands with K as the row index (lda, ldb): dW = dA^T . H with the batch as K.
 *             colsum [M] or NULL: sum_k At[k, m] added in the order k = 0, 1, ... (the bias gradient).
 *
 * Any M, N, K >= 1.  Matrices 16-byte aligned, leading dimensions multiples of 4 floats and at least the row length; IDIFF_EINVAL
 * before any device call otherwise, with a message that starts "gemm_nn: " / "gemm_tn: ".  *_ok (host only): 1 for the sizes served. */
int idiff_gemm_nn_ok(int M, int N, int K);
int idiff_gemm_nn_f32(const float *A, int64_t lda, const float *Bm, int64_t ldb, float *C, int64_t ldc, const float *P, int64_t ldp,
                      int M, int N, int K, void *stream);
int idiff_gemm_tn_ok(int M, int N, int K);
int idiff_gemm_tn_f32(const float *At, int64_t lda, const float *Bm, int64_t ldb, float *C, int64_t ldc, float *colsum,
                      int M, int N, int K, void *stream);

/* Doubles of workspace the two fixed-order reductions below take (per-workgroup partials, indexed by workgroup). */
#define IDIFF_REDUCE_WS_DOUBLES 1024

/* Denoising score matching loss of losses.py:164-188 and its gradient with respect to the network output.  With score = -out / std both
 * weightings are  mean_b weight[b] r_b,  r_b = reduce_d (z - out)^2:  weight NULL (= 1) or [B] (g(t)^2 / std^2 under likelihood
 * weighting), reduce = mean_d (reduce_mean != 0) or (1/2) sum_d.  G [B, D] (row pitch ldg >= D floats) or NULL = s weight[b] (out - z), s = 2 / (B D) or 1 / B;
 * *loss (device float) = the loss, summed in fp64 over fixed ranges in a fixed order and rounded once.  ws: IDIFF_REDUCE_WS_DOUBLES
 * doubles.  G is evaluated in fp64 and rounded once.  Two launches. */
int idiff_dsm_loss_grad_f32(const float *out, const float *z, const float *weight, float *G, int64_t ldg, float *loss, double *ws,
                            int B, int D, int reduce_mean, void *stream);

/* *sumsq (device double) = sum_i x[i]^2 in fp64, fixed ranges, fixed order (two launches); ws as above. */
int idiff_grad_sumsq_f32(const float *x, int64_t n, double *ws, double *sumsq, void *stream);

/* One torch.optim.Adam step (L2 weight_decay added to the gradient, bias corrections with `step` >= 1 the number of this step,
 * denom = sqrt(v) / sqrt(1 - beta2^step) + eps, step size lr / (1 - beta1^step)) over ONE flat parameter buffer, behind
 * torch.nn.utils.clip_grad_norm_: with sumsq (device double, from idiff_grad_sumsq_f32) the gradient is first multiplied by
 * min(1, max_norm / (sqrt(*sumsq) + 1e-6)), read on the device; sumsq NULL: no clipping.  Evaluated in fp64 from the fp32 state, each
 * of theta, m, v rounded once.  grad is not modified. */
int idiff_adam_step_f32(float *theta, const float *grad, float *m, float *v, int64_t n, const double *sumsq, double max_norm, double lr,
                        double beta1, double beta2, double eps, double weight_decay, int64_t step, void *stream);

/* The network's input rows for a training batch: h[b, :D] = mean_coeff[b] x[b, :] + std[b] z[b, :] (mean_coeff NULL = 1),
 * h[b, D] = label[b], h[b, D + 1 : kpad] = 0; x, z [B, D], h [B, kpad]. */
int idiff_fcn_train_input_f32(const float *x, const float *z, const float *std_, const float *mean_coeff, const float *label, float *h,
                              int64_t B, int D, int kpad, void *stream);

/* One update of a predictor or corrector of the sampler over the state rows [B, D] (sampling.py):
 *     mean_out = a x + b score_scale s,      x_out = mean_out + c z
 * evaluated in fp64 from the fp32 inputs, x_out from the unrounded mean, each output rounded to fp32 once.  Row pitches in floats, each
 * >= D.  x_out may be x (in place); mean_out may be NULL.
 * Noise: z given = explicit noise [B, D]; z NULL = drawn here, Philox4x32-10 keyed by `seed` with counter ((row0 + r) D4 + col) >> 2,
 * D4 = D rounded up to 4: element (r, col) has the bits idiff_perturb_randn_f32 writes to z_out for a [rows, D4] matrix and the same
 * seed and row0, however rows are cut into launches.  With c == 0 and no noise_norm nothing is drawn and z is not read.
 * Langevin form: noise_norm (device double, from idiff_sampler_noise_norm_f32) given = the kernel uses a = 1,
 * b = lang_scale (*noise_norm)^2 score_scale, c = sqrt(2 lang_scale (*noise_norm)^2) and ignores the a, b, c passed.
 * label_col >= 0 (D <= label_col < ldo): label_value is also written into that column of every row of x_out (the time feature of the
 * fcn's padded input rows).  16-byte accesses when every pointer is 16-byte aligned and every pitch a multiple of 4; any D and pitch
 * otherwise.  No atomics, no workspace.  B == 0 returns 0. */
int idiff_sampler_step_f32(const float *x, int64_t ldx, const float *s, int64_t lds, const float *z, int64_t ldz, float *x_out, int64_t ldo,
                           float *mean_out, int64_t ldm, int64_t B, int D, double a, double b, double c, const double *noise_norm,
                           double lang_scale, double score_scale, uint64_t seed, int64_t row0, int label_col, float label_value,
                           void *stream);

/* *out (device double) = mean_r sqrt(sum_col z[r, col]^2) over the explicit z [B, D] (pitch ldz), or, z NULL, over the generated stream
 * of (seed, row0, B, D) above -- no noise buffer exists on that path.  fp64, fixed order: per-row sums, rows added in index order
 * (two launches); ws: IDIFF_REDUCE_WS_DOUBLES doubles. */
int idiff_sampler_noise_norm_f32(const float *z, int64_t ldz, int64_t B, int D, uint64_t seed, int64_t row0, double *ws, double *out,
                                 void *stream);

/* ------------------------------------------------------------------ Jacobian of the fcn score network (csrc/fcn_jacobian.hip) */

/* Forward-mode propagation of a point's D input directions through Linear + ELU layers: D tangent rows per point.  g(a) = a > 0 ? 1 :
 * a + 1 is ELU' written in terms of the ELU OUTPUT a (as idiff_gemm_nn_f32 has it); here it belongs to a (point, column) pair and is
 * broadcast over the point's rows.
 *
 *   jvp_seed:   T[p][i, n] = W1[n, i] g(act[p, n]),  i < D, n < N.  W1 [N, ldw] is the first Linear's weight as it lies; its columns from
 *               D on (the time column, the pads) are never read.  act [P, ld_act]; T [P][D, ldt] with point stride strideT.  One fp32
 *               multiply per element after the one rounding of a + 1: bit-equal to fl(W1 fl(a + 1)).
 *   jvp_layer:  C[p][r, n] = (sum_k A[p][r, k] W[n, k]) g(act[p, n]).  A [P][R, lda] with point stride strideA, W [N, ldw] K-contiguous (an
 *               nn.Linear weight as it lies), act [P, ld_act] or NULL (no factor: the output layer), C [P][R, ldc] with point stride
 *               strideC.  On v_mfma_f32_32x32x2_f32, a k-ordered chain of fp32 fmas:
 *               |C - exact| <= g (K + 2) 2^-24 sum_k |a_k w_k| + 2 2^-24 |exact| (the roundings of a + 1 and of the multiply).  No split of
 *               K, no atomics, no workspace: the same bits on every run, and a point's bits do not depend on the other points of the launch.
 *               Pads of C (columns N .. ldc) and rows from R on are not written.
 *
 * Any P >= 0 (P = 0 is a no-op) and R, D, N, K >= 1.  Pointers 16-byte aligned; leading dimensions and point strides multiples of 4 floats,
 * leading dimensions at least the row length; IDIFF_EINVAL before any device call otherwise, with a message that starts "jvp_seed: " /
 * "jvp_layer: ".  idiff_jvp_layer_ok (host only): 1 for the sizes served. */
int idiff_jvp_layer_ok(int R, int N, int K);
int idiff_jvp_seed_f32(const float *W1, int64_t ldw, const float *act, int64_t ld_act, float *T, int64_t ldt, int64_t strideT, int P, int D,
                       int N, void *stream);
int idiff_jvp_layer_f32(const float *A, int64_t lda, int64_t strideA, const float *W, int64_t ldw, const float *act, int64_t ld_act,
                        float *C, int64_t ldc, int64_t strideC, int P, int R, int N, int K, void *stream);

/* ------------------------------------------------------------------ probability-flow ODE: adaptive Runge-Kutta (csrc/ode.hip) */

/* The arithmetic over the batch of one adaptive Runge-Kutta step whose step-size control runs on the host (ode.py).  State y [B, W]
 * doubles, W = D + aug (aug = 1: column D carries log p); stage derivatives K [7][B, W] doubles, stage j at K + j strideK; pitches in
 * elements.  fp64 throughout, every output rounded once, sums over stages in index order with one fma per term, reductions over fixed
 * ranges in a fixed order, no atomics: the same arguments give the same bits.  B == 0 (P == 0) returns 0 without a launch; a bad size,
 * pitch or alignment returns IDIFF_EINVAL before any device call, with a message that starts with the kernel's name.
 *
 *   rk_stage   v = y + sum_{j < ns} c[j] K_j, 0 <= ns <= 6, c a HOST array (h a_sj, or h b_j for the solution).  y_out (or NULL) = v;
 *              x32[r, c < D] = fl32(v[r, c]) and x32[r, D] = label_value: the padded first-layer input rows [B, ldx >= D + 1] of the
 *              network.  Columns of x32 beyond D are never written.  y_out may be y.
 *              |v - exact| <= (ns + 1) 2^-53 (|y| + sum_j |c_j K_j|), the fp32 rows 2^-24 |v| more.
 *   rk_error   *out (device double) = sum_{r, c} ((sum_{j < 7} e[j] K_j[r, c]) / (atol + rtol max(|y[r, c]|, |y_new[r, c]|)))^2, e a HOST
 *              array (h E_j).  Two launches; ws: IDIFF_REDUCE_WS_DOUBLES doubles.
 *   flow_rhs   Ks[r, c < D] = a x32[r, c] + b v[r, c] (x32, v fp32); with aug: Ks[r, D] = a D + b q_r, where q_r = q[r] (device doubles:
 *              the exact trace) or, q NULL, sum_c eps[r, c] u[r, c] over fp32 rows (Hutchinson: u the vector-Jacobian product of eps), one
 *              fixed-order sum per row.  Pass q, or eps and u.
 *   jvp_trace  tr[p] = sum_{i < D} sum_{n < N} T[p][i, n] Wout[i, n]: the trace of the network Jacobian from the tangent rows T [P][D, ldt]
 *              (point stride strideT) in front of the output layer Wout [D, ldw].  One workgroup per point.  T and Wout 16-byte aligned,
 *              ldt, ldw, strideT multiples of 4 floats, ldt and ldw at least N rounded up to 4 (those columns are read, not used).
 *
 * rk_stage and flow_rhs move 16 bytes per access when the double pointers are 16-byte aligned and their pitches even. */
int idiff_rk_stage_f64(const double *y, int64_t ldy, const double *K, int64_t ldk, int64_t strideK, const double *c, int ns, double *y_out,
                       int64_t ldyo, float *x32, int64_t ldx, int64_t B, int D, int aug, float label_value, void *stream);
int idiff_rk_error_f64(const double *K, int64_t ldk, int64_t strideK, const double *e, const double *y, int64_t ldy, const double *y_new,
                       int64_t ldyn, int64_t B, int W, double atol, double rtol, double *ws, double *out, void *stream);
int idiff_flow_rhs_f64(const float *x32, int64_t ldx, const float *v, int64_t ldv, double a, double b, double *Ks, int64_t ldk, int64_t B,
                       int D, int aug, const float *eps, int64_t lde, const float *u, int64_t ldu, const double *q, void *stream);
int idiff_jvp_trace_f64(const float *T, int64_t ldt, int64_t strideT, const float *Wout, int64_t ldw, double *tr, int P, int D, int N,
                        void *stream);

/* ------------------------------------------------------------------ Stein divergence from sampled score rows (csrc/stein.hip)
 * The score rows s_i = s(y + sigma z_i), z_i ~ N(0, I), that the sampled ID path evaluates hold the divergence of the score smoothed
 * over the sampling ball: E[z . s(y + sigma z)] = sigma tr grad (s * N(0, sigma^2 I))(y) (Stein's identity), so FLIPD needs no JVP of
 * the network.  For P points of M rows each:
 *   rows[p, i] = (a', q),   a' = sum_c z_ic (s_ic - mean_pc),   q = sum_c z_ic^2                      [P, M, 2] fp64
 *   sums[p]    = (sum a', sum a'^2, sum q, sum q^2, sum a' q) over the M rows                          [P, 5] fp64
 * S fp32: row i of point p at S + p stride_s + i lds (lds >= D; stride_s >= (M - 1) lds + D when P > 1); mean [P, D] fp64 (the column
 * means, idiff_colmean_f64).  Noise: Z fp32, addressed as S with ldz / stride_z; or Z NULL and seeds [P] uint64 on the device, D % 4 == 0:
 * the element (row0 + i, c) of the Philox stream idiff_perturb_randn_f32 draws for that seed in a matrix of width D, the same bits,
 * never written anywhere.  row0 only indexes that stream: the M rows given are rows row0 .. row0 + M - 1 of the point's noise matrix.
 *
 * One wave per row, 16-byte loads where the pointer, pitch and point stride allow, every product an fp64 fma of converted fp32
 * values, a fixed order that depends on D alone: a row's (a', q) is the same bits whatever P, M, row0 or the source of the same z.
 * The sums: one workgroup a point, fixed order.  No atomics, no workspace.  A row with a non-finite value in S, Z or the mean is NaN
 * in both of its values, and so are its point's sums; other points are not touched.
 *
 * Nonzero (idiff_last_error starts "stein_rows: ") before any launch for a null or misaligned pointer (S, Z 4 bytes; mean, seeds,
 * rows, sums 8), neither Z nor seeds, Z NULL with D % 4 != 0, M < 1, D < 1, a shape idiff_stein_rows_ok (host only) denies (M < 2^31,
 * D <= 2^30), P outside 0 .. 65535, a negative row0 or a pitch below D.  P = 0 is a no-op.  No host synchronisation. */
int idiff_stein_rows_ok(int64_t M, int64_t D);
int idiff_stein_rows_f64(const float *S, int64_t lds, int64_t stride_s, const double *mean, const float *Z, int64_t ldz, int64_t stride_z,
                         const uint64_t *seeds, int64_t row0, double *rows, double *sums, int64_t P, int64_t M, int64_t D, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* IDIFF_HIP_H */
