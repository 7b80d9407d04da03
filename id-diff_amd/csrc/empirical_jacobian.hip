// Jacobian of the empirical score (csrc/empirical_score.hip) in closed form: with d_i = x_i - x, w = softmax_i(-|d_i|^2 / (2 sigma^2)) and
// m = sum_i w_i d_i (= score sigma^2),
//
//   I + sigma^2 grad s(x)  =  C(x, sigma)  :=  sum_i w_i (d_i - m)(d_i - m)^T / sigma^2
//
// the softmax-weighted covariance of the cloud seen from x, in units of sigma^2.  Tangent directions have eigenvalue near 1, normal
// directions near 0; the Monte-Carlo score matrix of the driver estimates |1 - eig(C)|, this kernel gives C itself.
//
// One workgroup (four waves) per query (point, sigma), two passes over the RAW fp32 cloud in one launch, fp64 from the first difference:
//   pass 1  the largest logit -|d_i|^2 / (2 sigma^2) (the nearest point);
//   pass 2  every logit again BY THE SAME CODE (tile_logit: the same fma chain over the same LDS tile), w_i = exp(l_i - max) <= 1 with
//           the nearest point at exactly 1, so nothing is ever rescaled; sum w, sum w^2, sum w d and M = sum w d d^T.
// A tile of TN = 32 points is staged in LDS as fp64 d (rows past N and the columns from D to DP = 16 NB are zeros).  M runs on
// v_mfma_f64_16x16x4_f64 (lane l supplies A[l & 15][l >> 4] and B[l >> 4][l & 15], register r of lane l is C[(l >> 4) + 4 r][l & 15]):
// for the 16 x 16 block (a, b) and the k step of points 4 r .. 4 r + 3, lane l reads tile[4 r + (l >> 4)][16 a + (l & 15)], scales it by
// the point's weight in a register (the A operand) and reads tile[4 r + (l >> 4)][16 b + (l & 15)] unscaled (the B operand): both
// operands come from LDS by the same address pattern.  Only the NB (NB + 1) / 2 blocks a <= b are accumulated; block t (row-major over
// a <= b) belongs to wave t % 4, accumulator t / 4 of that wave: at D = 192 that is 78 blocks, 20 a wave, 160 VGPRs.  The lower
// triangle -- of a diagonal block too, whose two halves the matrix core rounds differently -- is the mirror of the upper at the store,
// so C is symmetric to the bit.  The row pitch is 16 (mod 32) doubles: the two rows x 16 columns a 32-lane group of ds_read_b64
// touches fall on 64 distinct banks.
//
// A tile whose 32 weights are all exactly 0.0 (exp underflowed) is skipped; none is skipped on a threshold.  Every sum has one fixed
// order, there are no atomics and no workspace: the same inputs give the same bits, whatever else is in the launch.
#include "common.h"

#include <math.h>

using namespace idiff;

namespace {

typedef double doublex4 __attribute__((ext_vector_type(4)));

constexpr int TN = 32;               // points of the cloud per tile
constexpr int WAVES = 4;
constexpr int THREADS = 64 * WAVES;
constexpr int NB_MAX = 12;           // 16-column blocks of a row of C
constexpr int D_MAX = 16 * NB_MAX;
constexpr int64_t N_MAX = 2147483647 - TN;

struct JacParams {
  const float *x, *X, *sigma; double *C, *mean; float *ess;
  int N, D;
};

__device__ __forceinline__ doublex4 mfma(double a, double b, doublex4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

template <int NB>
__global__ void __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(NB <= 8 ? 2 : 1, NB <= 8 ? 2 : 1)))
empirical_jacobian_kernel(const JacParams p) {
  constexpr int DP = 16 * NB, PITCH = (NB & 1) ? DP : DP + 16;
  constexpr int T = NB * (NB + 1) / 2, J = (T + WAVES - 1) / WAVES;
  constexpr int UF = 2 * NB;         // floats of a tile per thread: TN DP / THREADS
  __shared__ __attribute__((aligned(16))) double ds[TN * PITCH];
  __shared__ double xs[DP], ms[DP], ws[TN], red[2 * TN];
  const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int D = p.D, N = p.N;
  const int64_t q = blockIdx.x, total = (int64_t)N * D;

  for (int e = tid; e < TN * PITCH; e += THREADS) ds[e] = 0.0;    // the columns from D on are never written again

  // ---- the query; one that is not finite, or whose sigma is not positive and finite, is computed as the origin at sigma 1 and
  // written as NaN
  float sg = p.sigma[q];
  float xv = 0.f;
  if (tid < D) xv = p.x[q * D + tid];
  const int bad = __syncthreads_or(!(sg > 0.f && sg < INFINITY) || !(fabsf(xv) < INFINITY));
  if (bad) sg = 1.f;
  if (tid < DP) xs[tid] = bad ? 0.0 : (double)xv;
  const double s2 = (double)sg * (double)sg, inv2 = 0.5 / s2;

  // ---- the tile loader: float e = tid + THREADS u of the [TN, D] tile, which is contiguous in X
  // (its row e / D as a float product: e + 1/2 is never within 1 / (2 D) of a multiple of D, far above the rounding)
  const float rD = 1.f / (float)D;
  float pre[UF];
  auto fetch = [&](int n0) {
#pragma unroll
    for (int u = 0; u < UF; ++u) {
      const int e = tid + THREADS * u;
      const int64_t g = (int64_t)n0 * D + e;
      pre[u] = (e < TN * D && g < total) ? p.X[g] : 0.f;
    }
  };
  auto stage = [&](int n0) {
#pragma unroll
    for (int u = 0; u < UF; ++u) {
      const int e = tid + THREADS * u;
      if (e < TN * D) {
        const int r = (int)(((float)e + 0.5f) * rD), c = e - r * D;
        ds[r * PITCH + c] = (int64_t)n0 * D + e < total ? (double)pre[u] - xs[c] : 0.0;   // a row past N: zeros, weight exactly 0
      }
    }
  };
  // the logit of point tid >> 3 of the tile, the same value in the eight lanes that share it: the one code both passes run
  const int pt = tid >> 3, g8 = tid & 7;
  auto tile_logit = [&](int n0) {
    const double *row = ds + pt * PITCH + g8;
    double sq = 0.0;
#pragma unroll
    for (int s = 0; s < UF; ++s) sq = fma(row[8 * s], row[8 * s], sq);
    sq += __shfl_xor(sq, 1, 64);
    sq += __shfl_xor(sq, 2, 64);
    sq += __shfl_xor(sq, 4, 64);
    return n0 + pt < N ? -(sq * inv2) : -INFINITY;
  };

  // ---- pass 1: the largest logit
  double lmax = -INFINITY;
  fetch(0);
  for (int n0 = 0; n0 < N; n0 += TN) {
    __syncthreads();                                              // everyone is done with the previous tile (and xs is written)
    stage(n0);
    __syncthreads();
    if (n0 + TN < N) fetch(n0 + TN);
    lmax = fmax(lmax, tile_logit(n0));
  }
#pragma unroll
  for (int o = 8; o < 64; o <<= 1) lmax = fmax(lmax, __shfl_xor(lmax, o, 64));
  if (lane == 0) red[wave] = lmax;
  __syncthreads();
  lmax = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));

  // ---- the blocks of this wave: t = wave + 4 j, row-major over a <= b
  int off[J];                                                     // 16 a | 16 b << 16, wave-uniform
#pragma unroll
  for (int j = 0; j < J; ++j) {
    int a = 0, rem = wave + WAVES * j;
    while (a < NB - 1 && rem >= NB - a) { rem -= NB - a; ++a; }
    off[j] = 16 * a | 16 * (a + rem) << 16;                       // b past NB where t >= T: never used
  }
  doublex4 acc[J];
#pragma unroll
  for (int j = 0; j < J; ++j) acc[j] = doublex4{0.0, 0.0, 0.0, 0.0};
  double sw = 0.0, sw2 = 0.0, md = 0.0;                           // of point pt (lanes g8 == 0); of column tid

  // ---- pass 2
  fetch(0);
  for (int n0 = 0; n0 < N; n0 += TN) {
    __syncthreads();
    stage(n0);
    __syncthreads();
    if (n0 + TN < N) fetch(n0 + TN);
    const double lg = tile_logit(n0);
    const double w = lg == -INFINITY ? 0.0 : exp(lg - lmax);
    if (g8 == 0) {
      ws[pt] = w;
      sw += w;
      sw2 = fma(w, w, sw2);
    }
    if (!__syncthreads_or(w != 0.0)) continue;                    // workgroup-uniform: every weight of the tile is exactly 0

    if (tid < DP) {
#pragma unroll 8
      for (int i = 0; i < TN; ++i) md = fma(ws[i], ds[i * PITCH + tid], md);
    }
#pragma unroll 2
    for (int r = 0; r < TN / 4; ++r) {                            // (unrolled further, the tile's reads are all hoisted and spill)
      const double wv = ws[4 * r + l4];
      const double *row = ds + (4 * r + l4) * PITCH + l15;
#pragma unroll
      for (int j = 0; j < J; ++j)
        if (wave + WAVES * j < T) acc[j] = mfma(wv * row[off[j] & 0xffff], row[off[j] >> 16], acc[j]);
    }
  }

  // ---- sum w and sum w^2 in the order of the tile's points; mean = sum w d / sum w
  __syncthreads();
  if (g8 == 0) {
    red[pt] = sw;
    red[TN + pt] = sw2;
  }
  __syncthreads();
  double tot = 0.0, tot2 = 0.0;
#pragma unroll 8
  for (int i = 0; i < TN; ++i) {
    tot += red[i];
    tot2 += red[TN + i];
  }
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  if (tid < DP) {
    const double m = md / tot;
    ms[tid] = m;
    if (tid < D) p.mean[q * D + tid] = bad ? nan : m;
  }
  if (tid == 0) p.ess[q] = bad ? __int_as_float(0x7fc00000) : (float)(tot * tot / tot2);
  __syncthreads();

  // ---- C = (M / sum w - m m^T) / sigma^2: the upper triangle as accumulated, the lower as its mirror
  double *Cq = p.C + q * D * D;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    if (wave + WAVES * j >= T) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int oa = off[j] & 0xffff, ob = off[j] >> 16, i = oa + l4 + 4 * r, k = ob + l15;
      if (i >= D || k >= D || (oa == ob && i > k)) continue;
      const double v = bad ? nan : (acc[j][r] / tot - ms[i] * ms[k]) / s2;
      Cq[(int64_t)i * D + k] = v;
      if (i != k) Cq[(int64_t)k * D + i] = v;
    }
  }
}

template <int NB> void launch(const JacParams &p, int B, hipStream_t stream) {
  hipLaunchKernelGGL(empirical_jacobian_kernel<NB>, dim3((unsigned)B), dim3(THREADS), 0, stream, p);
}

}  // namespace

IDIFF_API int idiff_empirical_jacobian_ok(int64_t N, int D) { return N >= 1 && N <= N_MAX && D >= 1 && D <= D_MAX ? 1 : 0; }

IDIFF_API int idiff_empirical_jacobian_f64(const float *x, const float *X, const float *sigma, double *C, double *mean, float *ess,
                                           int B, int64_t N, int D, void *stream) {
  if (B < 0) return fail("empirical_jacobian: B = %d", B);
  if (N < 1 || D < 1) return fail("empirical_jacobian: N = %lld, D = %d", (long long)N, D);
  if (!idiff_empirical_jacobian_ok(N, D))
    return fail("empirical_jacobian: N = %lld, D = %d: a workgroup keeps the upper triangle of a query's fp64 C in registers and "
                "serves D <= %d, N <= %lld (ask idiff_empirical_jacobian_ok)", (long long)N, D, D_MAX, (long long)N_MAX);
  if (!x || !X || !sigma || !C || !mean || !ess) return fail("empirical_jacobian: null pointer");
  if (((uintptr_t)x & 3) || ((uintptr_t)X & 3) || ((uintptr_t)sigma & 3) || ((uintptr_t)ess & 3) || ((uintptr_t)C & 7) ||
      ((uintptr_t)mean & 7))
    return fail("empirical_jacobian: x, X, sigma and ess must be 4-byte aligned, C and mean 8-byte aligned");
  if (B == 0) return 0;
  JacParams p = {x, X, sigma, C, mean, ess, (int)N, D};
  hipStream_t s = (hipStream_t)stream;
  switch (ceil_div(D, 16)) {
    case 1: launch<1>(p, B, s); break;
    case 2: launch<2>(p, B, s); break;
    case 3: launch<3>(p, B, s); break;
    case 4: launch<4>(p, B, s); break;
    case 5: launch<5>(p, B, s); break;
    case 6: launch<6>(p, B, s); break;
    case 7: launch<7>(p, B, s); break;
    case 8: launch<8>(p, B, s); break;
    case 9: launch<9>(p, B, s); break;
    case 10: launch<10>(p, B, s); break;
    case 11: launch<11>(p, B, s); break;
    default: launch<12>(p, B, s); break;
  }
  return launch_status("empirical_jacobian");
}
