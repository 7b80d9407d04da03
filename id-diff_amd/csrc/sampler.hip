// Sampling from a score model (sampling.py): the one update every predictor and corrector of the reference reduces to when all rows of
// a step share one time,
//
//   x_mean = a x + b s,      x_new = x_mean + c z,      z ~ N(0, I)
//
// with s the score (or the raw network output: b then carries -1 / std) and (a, b, c) three scalars the host knows before the loop
// starts.  The Langevin corrector is the exception: its step size (snr mean_r |z_r|)^2 2 alpha depends on the noise just drawn, so
// the kernel reads that mean as a device double (idiff_sampler_noise_norm_f32) and forms b and c itself -- nothing comes back to the host.
//
// Arithmetic: fp32 in, a, b, c doubles by value; m = a x + b s and y = m + c z in fp64, y from the unrounded m, each output rounded to
// fp32 once (as idiff_adam_step_f32).  Noise: a given z is read; a null z is drawn here, Philox4x32-10 keyed by `seed`, counter
// ((row0 + r) D4 + c) >> 2 with D4 = D rounded up to 4, Box-Muller as rng.hip -- element (r, c) is the bit pattern
// idiff_perturb_randn_f32 writes to z_out for a [rows, D4] matrix, however the rows are cut into launches.
//
// One lane owns four consecutive columns of one row: 16-byte loads and stores where every pointer and pitch allows it (VEC) and the
// four columns lie inside D, scalar accesses otherwise.  No atomics, no workspace: the same arguments give the same bits.
#include "common.h"
#include "philox.h"
#include <math.h>

namespace {
using namespace idiff;

constexpr int RED_THREADS = 256;

// the four normals of the 4-column group whose counter is ctr (rng.hip: perturb_randn_kernel)
__device__ __forceinline__ float4 normals4(uint64_t ctr, uint32_t k0, uint32_t k1) {
  const u4 rnd = philox4x32_10({(uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u}, k0, k1);
  const float r0 = sqrtf(-2.0f * logf(u01(rnd.x))), r1 = sqrtf(-2.0f * logf(u01(rnd.z)));
  float s0, c0, s1, c1;
  sincosf(6.2831853071795864f * u01(rnd.y), &s0, &c0);
  sincosf(6.2831853071795864f * u01(rnd.w), &s1, &c1);
  return make_float4(r0 * c0, r0 * s0, r1 * c1, r1 * s1);
}

struct StepP {
  const float *x, *s, *z;
  float *x_out, *mean_out;
  const double *noise_norm;
  int64_t ldx, lds, ldz, ldo, ldm, B, row0;
  int D, label_col;
  double a, b, c, lang_scale, score_scale;
  float label_value;
  uint32_t k0, k1;
};

// `n` columns (1 .. 4) of a row starting at p; the whole 16 bytes at once when the caller knows they are there and aligned
template <bool VEC> __device__ __forceinline__ float4 load_cols(const float *p, int n) {
  if (VEC && n == 4) return *reinterpret_cast<const float4 *>(p);
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  v.x = p[0];
  if (n > 1) v.y = p[1];
  if (n > 2) v.z = p[2];
  if (n > 3) v.w = p[3];
  return v;
}

template <bool VEC> __device__ __forceinline__ void store_cols(float *p, float4 v, int n) {
  if (VEC && n == 4) {
    *reinterpret_cast<float4 *>(p) = v;
    return;
  }
  p[0] = v.x;
  if (n > 1) p[1] = v.y;
  if (n > 2) p[2] = v.z;
  if (n > 3) p[3] = v.w;
}

// (no __restrict__: x_out may be x)
template <bool VEC> __global__ void __launch_bounds__(256) step_kernel(StepP p) {
  double a = p.a, b = p.b * p.score_scale, c = p.c;
  if (p.noise_norm) {
    const double nn = *p.noise_norm, base = p.lang_scale * nn * nn;
    a = 1.0;
    b = base * p.score_scale;
    c = sqrt(2.0 * base);
  }
  const bool noisy = p.noise_norm != nullptr || p.c != 0.0;
  const int64_t G = (p.D + 3) >> 2, D4 = G * 4, total = p.B * G;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = g / G;
    const int col = (int)(g - r * G) * 4;
    const int n = p.D - col < 4 ? p.D - col : 4;
    const float4 xv = load_cols<VEC>(p.x + r * p.ldx + col, n);
    const float4 sv = load_cols<VEC>(p.s + r * p.lds + col, n);
    double m0 = a * (double)xv.x + b * (double)sv.x, m1 = a * (double)xv.y + b * (double)sv.y;
    double m2 = a * (double)xv.z + b * (double)sv.z, m3 = a * (double)xv.w + b * (double)sv.w;
    if (p.mean_out) store_cols<VEC>(p.mean_out + r * p.ldm + col, make_float4((float)m0, (float)m1, (float)m2, (float)m3), n);
    if (noisy) {
      const float4 zv = p.z ? load_cols<VEC>(p.z + r * p.ldz + col, n)
                            : normals4((uint64_t)((p.row0 + r) * D4 + col) >> 2, p.k0, p.k1);
      m0 += c * (double)zv.x; m1 += c * (double)zv.y; m2 += c * (double)zv.z; m3 += c * (double)zv.w;
    }
    float *dst = p.x_out + r * p.ldo;
    store_cols<VEC>(dst + col, make_float4((float)m0, (float)m1, (float)m2, (float)m3), n);
    if (p.label_col >= 0 && col == 0) dst[p.label_col] = p.label_value;
  }
}

// ---- mean_r |z_r| in fp64, fixed order.  Workgroup w owns the rows [w per, (w + 1) per): per row the 256 lanes add their strided share
// of the squares, a tree whose shape does not depend on the data folds them, lane 0 adds the roots in row order; partial w goes to ws[w].
__device__ __forceinline__ double block_sum(double v, double *sh) {
  __syncthreads();                       // the previous row's sh[0] has been read by lane 0
  sh[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int s = RED_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  return sh[0];
}

__global__ void __launch_bounds__(RED_THREADS)
row_norm_partial_kernel(const float *__restrict__ z, int64_t ldz, int64_t B, int D, int64_t row0, uint32_t k0, uint32_t k1, int64_t per,
                        double *__restrict__ ws) {
  __shared__ double sh[RED_THREADS];
  const int64_t lo = (int64_t)blockIdx.x * per, hi = lo + per < B ? lo + per : B;
  const int G = (D + 3) >> 2;
  const int64_t D4 = (int64_t)G * 4;
  double part = 0.0;
  for (int64_t r = lo; r < hi; ++r) {
    double acc = 0.0;
    for (int g = threadIdx.x; g < G; g += RED_THREADS) {
      const int col = g * 4, n = D - col < 4 ? D - col : 4;
      const float4 zv = z ? load_cols<false>(z + r * ldz + col, n) : normals4((uint64_t)((row0 + r) * D4 + col) >> 2, k0, k1);
      acc += (double)zv.x * (double)zv.x;
      if (n > 1) acc += (double)zv.y * (double)zv.y;
      if (n > 2) acc += (double)zv.z * (double)zv.z;
      if (n > 3) acc += (double)zv.w * (double)zv.w;
    }
    const double tot = block_sum(acc, sh);
    if (threadIdx.x == 0) part += sqrt(tot);
  }
  if (threadIdx.x == 0) ws[blockIdx.x] = part;
}

__global__ void __launch_bounds__(RED_THREADS) row_norm_final_kernel(const double *__restrict__ ws, int n, double scale, double *__restrict__ out) {
  __shared__ double sh[RED_THREADS];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += RED_THREADS) acc += ws[i];
  const double tot = block_sum(acc, sh);
  if (threadIdx.x == 0) *out = scale * tot;
}

}  // namespace

IDIFF_API int idiff_sampler_step_f32(const float *x, int64_t ldx, const float *s, int64_t lds, const float *z, int64_t ldz, float *x_out,
                                     int64_t ldo, float *mean_out, int64_t ldm, int64_t B, int D, double a, double b, double c,
                                     const double *noise_norm, double lang_scale, double score_scale, uint64_t seed, int64_t row0,
                                     int label_col, float label_value, void *stream) {
  if (B < 0 || D <= 0 || row0 < 0) return fail("sampler_step: B = %lld, D = %d, row0 = %lld: needs B >= 0, D >= 1, row0 >= 0", (long long)B, D, (long long)row0);
  if (!x || !s || !x_out) return fail("sampler_step: null pointer");
  if (ldx < D || lds < D || ldo < D || (z && ldz < D) || (mean_out && ldm < D))
    return fail("sampler_step: a row pitch is shorter than a row of %d (x %lld, s %lld, z %lld, x_out %lld, mean_out %lld)", D, (long long)ldx,
                (long long)lds, (long long)ldz, (long long)ldo, (long long)ldm);
  if (((uintptr_t)x & 3) || ((uintptr_t)s & 3) || ((uintptr_t)z & 3) || ((uintptr_t)x_out & 3) || ((uintptr_t)mean_out & 3) ||
      ((uintptr_t)noise_norm & 7))
    return fail("sampler_step: x, s, z, x_out and mean_out must be 4-byte aligned, the noise norm 8-byte");
  if (label_col >= 0 && (label_col < D || label_col >= ldo))
    return fail("sampler_step: label_col = %d must lie in the pad columns [%d, %lld) of x_out", label_col, D, (long long)ldo);
  if (B == 0) return 0;
  StepP p = {x, s, z, x_out, mean_out, noise_norm, ldx, lds, ldz, ldo, ldm, B, row0, D, label_col < 0 ? -1 : label_col,
             a, b, c, lang_scale, score_scale, label_value, (uint32_t)seed, (uint32_t)(seed >> 32)};
  const bool vec = !(((uintptr_t)x | (uintptr_t)s | (uintptr_t)z | (uintptr_t)x_out | (uintptr_t)mean_out) & 15) &&
                   !((ldx | lds | ldo | (z ? ldz : 0) | (mean_out ? ldm : 0)) & 3);
  const int grid = streaming_grid(B * (int64_t)((D + 3) / 4), 256);
  if (vec)
    hipLaunchKernelGGL(step_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
  else
    hipLaunchKernelGGL(step_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
  return launch_status("sampler_step");
}

IDIFF_API int idiff_sampler_noise_norm_f32(const float *z, int64_t ldz, int64_t B, int D, uint64_t seed, int64_t row0, double *ws,
                                           double *out, void *stream) {
  if (B < 1 || D <= 0 || row0 < 0) return fail("sampler_noise_norm: B = %lld, D = %d, row0 = %lld: needs B >= 1, D >= 1, row0 >= 0", (long long)B, D, (long long)row0);
  if (!ws || !out) return fail("sampler_noise_norm: null pointer");
  if (z && ldz < D) return fail("sampler_noise_norm: ldz = %lld is shorter than a row of %d", (long long)ldz, D);
  if (((uintptr_t)z & 3) || ((uintptr_t)ws & 7) || ((uintptr_t)out & 7))
    return fail("sampler_noise_norm: z must be 4-byte aligned, the workspace and the result 8-byte");
  const int64_t nb = B < IDIFF_REDUCE_WS_DOUBLES ? B : IDIFF_REDUCE_WS_DOUBLES, per = ceil_div64(B, nb);
  const int blocks = (int)ceil_div64(B, per);
  hipLaunchKernelGGL(row_norm_partial_kernel, dim3(blocks), dim3(RED_THREADS), 0, (hipStream_t)stream, z, ldz, B, D, row0, (uint32_t)seed,
                     (uint32_t)(seed >> 32), per, ws);
  hipLaunchKernelGGL(row_norm_final_kernel, dim3(1), dim3(RED_THREADS), 0, (hipStream_t)stream, (const double *)ws, blocks, 1.0 / (double)B, out);
  return launch_status("sampler_noise_norm");
}
