// The paper's two image manifolds of known dimension, rendered one workgroup per image (the reference paints them with
// Python loops over pixels, lightning_data_modules/SyntheticDataset.py:81-183, FixedSquaresManifold / FixedGaussiansManifold).
//
//   squares     out[n, p] = sum_k coef[n, k] [p in rect_k]: a sequential fp32 chain in ascending k that starts from +0.
//               This IS the reference's arithmetic (`img[i, j] += c` on an fp32 image: c rounded to fp32, one fp32 add per
//               square that covers the pixel), so the images are bit-equal to it.  A square that misses the pixel adds
//               +0.0f, which changes no fp32 value (x + 0 = x for every x but -0, and a chain that starts at +0 never
//               holds -0 under round-to-nearest), so the loop is branch-free.
//   gaussians   v[i, j] = sum_k exp(d_k (i - cx_k)^2) exp(d_k (j - cy_k)^2) / (sqrt(2 pi) std_k), d_k = -1 / (2 std_k^2),
//               accumulated in fp64 from the separable factors (2 S exponentials per Gaussian, not S^2), which live in LDS
//               for GK Gaussians at a time; rounded ONCE to fp32; the image's minimum and maximum by a workgroup reduction;
//               then (v - min) / (max - min) in fp32 as the reference does (:160-163): one rounding for the numerator, one
//               for the denominator, one for the correctly rounded division (hipcc's default for `/` on floats; this
//               library is built without fast-math).
//
// Each lane owns quads of 4 consecutive pixels of a row (S % 4 == 0) and stores them with one 16-byte store.
#include "common.h"

#include <math.h>

using namespace idiff;

namespace {

constexpr int TPB = 256;           // lanes per workgroup
constexpr int S_MAX = 64;          // largest image side
constexpr int K_MAX = 1024;        // most squares / Gaussians per image
constexpr int QPL = S_MAX * S_MAX / 4 / TPB;   // quads per lane at the largest side (4)
constexpr int GK = 16;             // Gaussians whose factors are in LDS at a time (2 * GK * S_MAX doubles = 16 KB)

__global__ void __launch_bounds__(TPB)
render_squares_kernel(const float *__restrict__ coef, const int *__restrict__ rects, float *__restrict__ out, int K, int S) {
  __shared__ int4 sq[K_MAX];       // {row0, col0, side, bits of the coefficient}: one 16-byte LDS read per square
  const int n = blockIdx.x, tid = threadIdx.x;
  for (int k = tid; k < K; k += TPB)
    sq[k] = make_int4(rects[3 * k], rects[3 * k + 1], rects[3 * k + 2], __float_as_int(coef[(int64_t)n * K + k]));
  __syncthreads();
  const int qrow = S / 4, Q = S * qrow;
  float *img = out + (int64_t)n * S * S;
  for (int q = tid; q < Q; q += TPB) {
    const int row = q / qrow, col = (q - row * qrow) * 4;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int k = 0; k < K; ++k) {
      const int4 r = sq[k];
      const float c = __int_as_float(r.w);
      const unsigned side = (unsigned)r.z, dc = (unsigned)(col - r.y);
      const bool in_row = (unsigned)(row - r.x) < side;
      a0 += (in_row && dc < side) ? c : 0.f;
      a1 += (in_row && dc + 1u < side) ? c : 0.f;
      a2 += (in_row && dc + 2u < side) ? c : 0.f;
      a3 += (in_row && dc + 3u < side) ? c : 0.f;
    }
    *reinterpret_cast<float4 *>(img + 4 * q) = make_float4(a0, a1, a2, a3);
  }
}

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

__global__ void __launch_bounds__(TPB)
render_gaussians_kernel(const double *__restrict__ std_, const int *__restrict__ centres, float *__restrict__ out, int K, int S) {
  __shared__ double fx[GK][S_MAX];   // exp(d_k (i - cx_k)^2) / (sqrt(2 pi) std_k), by row i
  __shared__ __attribute__((aligned(16))) double fy[GK][S_MAX];   // exp(d_k (j - cy_k)^2), by column j (read two at a time)
  __shared__ float red[2][TPB / 64];
  const int n = blockIdx.x, tid = threadIdx.x;
  const int qrow = S / 4, Q = S * qrow;
  double acc[QPL][4];
#pragma unroll
  for (int m = 0; m < QPL; ++m)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[m][j] = 0.0;

  for (int k0 = 0; k0 < K; k0 += GK) {
    const int kc = min(GK, K - k0);
    __syncthreads();                 // the previous chunk's factors have been read
    for (int e = tid; e < kc * 2 * S; e += TPB) {
      const int kk = e / (2 * S), r = e - kk * 2 * S, axis = r >= S ? 1 : 0, i = r - axis * S;
      const double sd = std_[(int64_t)n * K + k0 + kk];
      const double d = -1.0 / (2.0 * (sd * sd));
      const double t = (double)(i - centres[2 * (k0 + kk) + axis]);
      const double v = exp(d * (t * t));
      if (axis == 0) fx[kk][i] = v * (1.0 / (2.5066282746310002 * sd));   // sqrt(2 pi) as np.sqrt(2 * np.pi) rounds it
      else fy[kk][i] = v;
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < QPL; ++m) {
      const int q = tid + m * TPB;
      if (q < Q) {
        const int row = q / qrow, col = (q - row * qrow) * 4;
        for (int kk = 0; kk < kc; ++kk) {
          const double a = fx[kk][row];
          const double2 b0 = *reinterpret_cast<const double2 *>(&fy[kk][col]);
          const double2 b1 = *reinterpret_cast<const double2 *>(&fy[kk][col + 2]);
          acc[m][0] = fma(a, b0.x, acc[m][0]);
          acc[m][1] = fma(a, b0.y, acc[m][1]);
          acc[m][2] = fma(a, b1.x, acc[m][2]);
          acc[m][3] = fma(a, b1.y, acc[m][3]);
        }
      }
    }
  }

  // one rounding to fp32, then the image's extremes
  float v[QPL][4];
  float lo = INFINITY, hi = -INFINITY;
#pragma unroll
  for (int m = 0; m < QPL; ++m) {
    const bool live = tid + m * TPB < Q;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[m][j] = (float)acc[m][j];
      if (live) { lo = fminf(lo, v[m][j]); hi = fmaxf(hi, v[m][j]); }
    }
  }
  lo = wave_min(lo); hi = wave_max(hi);
  if ((tid & 63) == 0) { red[0][tid >> 6] = lo; red[1][tid >> 6] = hi; }
  __syncthreads();
  lo = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
  hi = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
  const float den = hi - lo;
  float *img = out + (int64_t)n * S * S;
#pragma unroll
  for (int m = 0; m < QPL; ++m) {
    const int q = tid + m * TPB;
    if (q < Q)
      *reinterpret_cast<float4 *>(img + 4 * q) =
          make_float4((v[m][0] - lo) / den, (v[m][1] - lo) / den, (v[m][2] - lo) / den, (v[m][3] - lo) / den);
  }
}

// what both entry points admit; 0 = launch, 1 = nothing to do, IDIFF_EINVAL = refused (nothing launched)
int admit(const char *what, const void *in, const void *table, const void *out, int N, int K, int S) {
  if (N < 0) return fail("%s: N = %d", what, N);
  if (S < 4 || S > S_MAX || S % 4 != 0) return fail("%s: the image side must be a multiple of 4 in [4, %d] (got %d)", what, S_MAX, S);
  if (K < 1 || K > K_MAX) return fail("%s: K must be in [1, %d] (got %d)", what, K_MAX, K);
  if ((int64_t)N * S * S >= ((int64_t)1 << 31)) return fail("%s: N * S * S = %lld is not below 2^31", what, (long long)N * S * S);
  if (N == 0) return 1;
  if (!in || !table || !out) return fail("%s: null pointer", what);
  if ((uintptr_t)out & 15) return fail("%s: out must be 16-byte aligned", what);
  return 0;
}

}  // namespace

IDIFF_API int idiff_render_squares_f32(const float *coef, const int *rects, float *out, int N, int K, int S, void *stream) {
  const int a = admit("render_squares", coef, rects, out, N, K, S);
  if (a) return a == 1 ? 0 : a;
  if (((uintptr_t)coef & 3) || ((uintptr_t)rects & 3)) return fail("render_squares: coef and rects must be 4-byte aligned");
  hipLaunchKernelGGL(render_squares_kernel, dim3(N), dim3(TPB), 0, (hipStream_t)stream, coef, rects, out, K, S);
  return launch_status("render_squares");
}

IDIFF_API int idiff_render_gaussians_f32(const double *std_, const int *centres, float *out, int N, int K, int S, void *stream) {
  const int a = admit("render_gaussians", std_, centres, out, N, K, S);
  if (a) return a == 1 ? 0 : a;
  if (((uintptr_t)std_ & 7) || ((uintptr_t)centres & 3)) return fail("render_gaussians: std must be 8-byte and centres 4-byte aligned");
  hipLaunchKernelGGL(render_gaussians_kernel, dim3(N), dim3(TPB), 0, (hipStream_t)stream, std_, centres, out, K, S);
  return launch_status("render_gaussians");
}
