// Stein divergence from the rows the sampled ID path has already paid for (stein.py): the score rows s_i = s(y + sigma z_i) of a point,
// z_i ~ N(0, I), hold the divergence of the score smoothed over the sampling ball,
//
//   E[z . s(y + sigma z)] = sigma tr grad (s * N(0, sigma^2 I))(y)            (Stein's identity; Ramani, Blu and Unser 2008)
//
// so FLIPD, D + sigma^2 (tr grad s + |s|^2), needs no JVP of the network.  Per row i of point p this file forms, in fp64,
//
//   a'_i = sum_c z_ic (s_ic - mean_c),     q_i = sum_c z_ic^2
//
// (mean the fp64 column mean of the point's rows, idiff_colmean_f64; q_i, whose expectation D is known, is the control variate) and per
// point the five sums  sum a', sum a'^2, sum q, sum q^2, sum a' q  the host turns into the reading and its error bar.
//
// NOISE: read from Z, or -- Z null, D % 4 == 0 -- drawn here: Philox4x32-10 keyed by the point's seed, counter ((row0 + i) D + c) >> 2,
// Box-Muller as rng.hip, i.e. the bit pattern idiff_perturb_randn_f32 drew for element (row0 + i, c) when it perturbed the row.  Z is
// never written.
//
// ROWS: one wave owns one row.  Lane l takes the 4-column groups l, l + 64, ... of it, one 16-byte load of S (and of Z) each where the
// pointer and both pitches allow it, scalar loads of the same elements otherwise; the columns of a group are added in order, the
// lanes' partials by a butterfly.  The order depends on D alone: a row's (a', q) is the same bits whatever P, M or row0 split it was
// computed under, and whichever noise source supplied the same z.  Every product is an fp64 fma of converted fp32 values.  A row
// whose a' or q is not finite (a non-finite value in S, Z or the mean: inf - inf, 0 inf and inf all end there, and finite fp32 inputs
// cannot overflow fp64) is NaN in both.
//
// SUMS: one workgroup per point, thread t adds rows t, t + 256, ... in order, then a tree over the 256 partials.  No atomics, no
// workspace: the same inputs give the same bits.  A point with a NaN row has NaN sums; no other point reads it.
#include "common.h"
#include "philox.h"
#include <math.h>

namespace {
using namespace idiff;

constexpr int WAVES = 4;
constexpr int THREADS = 64 * WAVES;
constexpr int64_t P_MAX = 65535;                 // gridDim.y
constexpr int64_t M_MAX = 2147483647;
constexpr int64_t D_MAX = 1 << 30;

// the four normals of the 4-column group whose counter is ctr (rng.hip: perturb_randn_kernel)
__device__ __forceinline__ float4 normals4(uint64_t ctr, uint32_t k0, uint32_t k1) {
  const u4 rnd = philox4x32_10({(uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u}, k0, k1);
  const float r0 = sqrtf(-2.0f * logf(u01(rnd.x))), r1 = sqrtf(-2.0f * logf(u01(rnd.z)));
  float s0, c0, s1, c1;
  sincosf(6.2831853071795864f * u01(rnd.y), &s0, &c0);
  sincosf(6.2831853071795864f * u01(rnd.w), &s1, &c1);
  return make_float4(r0 * c0, r0 * s0, r1 * c1, r1 * s1);
}

// `n` columns (1 .. 4) of a row starting at p, zeros behind them; the whole 16 bytes at once where the caller knows they are aligned
__device__ __forceinline__ float4 load_cols(const float *p, int n, bool vec) {
  if (vec && n == 4) return *reinterpret_cast<const float4 *>(p);
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  v.x = p[0];
  if (n > 1) v.y = p[1];
  if (n > 2) v.z = p[2];
  if (n > 3) v.w = p[3];
  return v;
}

struct SteinP {
  const float *S, *Z;
  const double *mean;
  const uint64_t *seeds;
  double *rows;
  int64_t lds, stride_s, ldz, stride_z, row0, M, D;
  int vec_s, vec_z;
};

__global__ void __launch_bounds__(THREADS) stein_rows_kernel(const SteinP p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t r = (int64_t)blockIdx.x * WAVES + wave, pt = blockIdx.y;
  if (r >= p.M) return;                                              // wave-uniform; no barrier below
  const float *srow = p.S + pt * p.stride_s + r * p.lds;
  const float *zrow = p.Z ? p.Z + pt * p.stride_z + r * p.ldz : nullptr;
  const double *mean = p.mean + pt * p.D;
  uint32_t k0 = 0, k1 = 0;
  if (!zrow) {
    const uint64_t seed = p.seeds[pt];
    k0 = (uint32_t)seed;
    k1 = (uint32_t)(seed >> 32);
  }
  const int64_t e0 = (p.row0 + r) * p.D, groups = (p.D + 3) >> 2;
  double a = 0.0, q = 0.0;
  for (int64_t g = lane; g < groups; g += 64) {
    const int64_t c = 4 * g;
    const int n = p.D - c < 4 ? (int)(p.D - c) : 4;
    const float4 s = load_cols(srow + c, n, p.vec_s);
    const float4 z = zrow ? load_cols(zrow + c, n, p.vec_z) : normals4((uint64_t)(e0 + c) >> 2, k0, k1);
    const double m0 = mean[c], m1 = n > 1 ? mean[c + 1] : 0.0, m2 = n > 2 ? mean[c + 2] : 0.0, m3 = n > 3 ? mean[c + 3] : 0.0;
    const double z0 = z.x, z1 = z.y, z2 = z.z, z3 = z.w;             // the columns behind D: z = 0, s = 0, mean = 0 add nothing
    a = fma(z0, (double)s.x - m0, a);
    a = fma(z1, (double)s.y - m1, a);
    a = fma(z2, (double)s.z - m2, a);
    a = fma(z3, (double)s.w - m3, a);
    q = fma(z0, z0, q);
    q = fma(z1, z1, q);
    q = fma(z2, z2, q);
    q = fma(z3, z3, q);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    a += __shfl_xor(a, off, 64);
    q += __shfl_xor(q, off, 64);
  }
  if (lane == 0) {
    if (!(fabs(a) < INFINITY) || !(fabs(q) < INFINITY)) a = q = __longlong_as_double(0x7ff8000000000000ll);
    double *out = p.rows + (pt * p.M + r) * 2;
    out[0] = a;
    out[1] = q;
  }
}

// sums[p] = (sum a', sum a'^2, sum q, sum q^2, sum a' q) over the M rows of point p, in a fixed order
__global__ void __launch_bounds__(THREADS) stein_sums_kernel(const double *__restrict__ rows, double *__restrict__ sums, int64_t M) {
  __shared__ double part[5][THREADS];
  const int tid = threadIdx.x;
  const double *mine = rows + (int64_t)blockIdx.x * M * 2;
  double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t i = tid; i < M; i += THREADS) {
    const double a = mine[2 * i], q = mine[2 * i + 1];
    v[0] += a;
    v[1] = fma(a, a, v[1]);
    v[2] += q;
    v[3] = fma(q, q, v[3]);
    v[4] = fma(a, q, v[4]);
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) part[k][tid] = v[k];
  __syncthreads();
  for (int half = THREADS / 2; half >= 1; half >>= 1) {
    if (tid < half) {
#pragma unroll
      for (int k = 0; k < 5; ++k) part[k][tid] += part[k][tid + half];
    }
    __syncthreads();
  }
  if (tid < 5) sums[(int64_t)blockIdx.x * 5 + tid] = part[tid][0];
}

}  // namespace

IDIFF_API int idiff_stein_rows_ok(int64_t M, int64_t D) { return M >= 1 && M <= M_MAX && D >= 1 && D <= D_MAX ? 1 : 0; }

IDIFF_API int idiff_stein_rows_f64(const float *S, int64_t lds, int64_t stride_s, const double *mean, const float *Z, int64_t ldz,
                                   int64_t stride_z, const uint64_t *seeds, int64_t row0, double *rows, double *sums, int64_t P,
                                   int64_t M, int64_t D, void *stream) {
  if (P < 0 || P > P_MAX) return fail("stein_rows: P = %lld, must be 0 .. %lld", (long long)P, (long long)P_MAX);
  if (M < 1 || D < 1) return fail("stein_rows: M = %lld, D = %lld", (long long)M, (long long)D);
  if (!idiff_stein_rows_ok(M, D))
    return fail("stein_rows: M = %lld, D = %lld: served are M <= %lld and D <= %lld (ask idiff_stein_rows_ok)", (long long)M,
                (long long)D, (long long)M_MAX, (long long)D_MAX);
  if (row0 < 0 || row0 > ((int64_t)1 << 62) / D - M)
    return fail("stein_rows: row0 = %lld: negative, or (row0 + M) D leaves 62 bits", (long long)row0);
  if (!S || !mean || !rows || !sums) return fail("stein_rows: null pointer");
  if (!Z && !seeds) return fail("stein_rows: neither Z nor seeds: the noise must come from somewhere");
  if (!Z && D % 4 != 0)
    return fail("stein_rows: D = %lld is no multiple of 4: the in-kernel Philox stream draws 4-column groups, pass Z", (long long)D);
  if (lds < D || (P > 1 && stride_s < (M - 1) * lds + D))
    return fail("stein_rows: S pitch %lld, point stride %lld for rows of %lld floats, %lld rows a point", (long long)lds,
                (long long)stride_s, (long long)D, (long long)M);
  if (Z && (ldz < D || (P > 1 && stride_z < (M - 1) * ldz + D)))
    return fail("stein_rows: Z pitch %lld, point stride %lld for rows of %lld floats, %lld rows a point", (long long)ldz,
                (long long)stride_z, (long long)D, (long long)M);
  if (((uintptr_t)S & 3) || ((uintptr_t)Z & 3) || ((uintptr_t)mean & 7) || ((uintptr_t)seeds & 7) || ((uintptr_t)rows & 7) ||
      ((uintptr_t)sums & 7))
    return fail("stein_rows: S and Z must be 4-byte aligned, mean, seeds, rows and sums 8-byte aligned");
  if (P == 0) return 0;
  SteinP p = {S, Z, mean, Z ? nullptr : seeds, rows, lds, stride_s, Z ? ldz : 0, Z ? stride_z : 0, row0, M, D,
              !((uintptr_t)S & 15) && lds % 4 == 0 && stride_s % 4 == 0, Z && !((uintptr_t)Z & 15) && ldz % 4 == 0 && stride_z % 4 == 0};
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(stein_rows_kernel, dim3((unsigned)ceil_div64(M, WAVES), (unsigned)P), dim3(THREADS), 0, st, p);
  if (int rc = launch_status("stein_rows")) return rc;
  hipLaunchKernelGGL(stein_sums_kernel, dim3((unsigned)P), dim3(THREADS), 0, st, rows, sums, M);
  return launch_status("stein_rows sums");
}
