// Score of the empirical distribution of a point cloud convolved with N(0, sigma^2 I) (models/empirical_exact.py), one launch, fp64 from
// the first difference to the single final rounding.  It is attention with the cloud as keys and values:
//
//   w_i(x)  = softmax_i(-|x - x_i|^2 / (2 sigma^2))
//   out     = mult (sum_i w_i x_i - x),      ess = 1 / sum_i w_i^2
//
// in the centred, expanded form: c the fp64 column mean of the cloud, y_i = x_i - c, h_i = |y_i|^2 / 2 (packed once, _lib.empirical_pack),
// q = x - c formed in fp64 before any product, logit l_i = (q . y_i - h_i) / sigma^2 (|q|^2 is common to all i and drops out), and
// out = mult (sum_i w_i y_i / sum_i w_i - q).  The centring makes the result independent of the cloud's offset.
//
// A wave owns 16 rows of x and streams the whole cloud past them, 32 points a step, with a running maximum, a running sum of w and
// of w^2 and the [16 x D] fp64 accumulator in registers (8 D / 16 VGPRs a lane: that, with q held the same way, sets the cap D <= 192).
// Logits and weights never leave the registers: no [B, N] buffer exists.  Both products run on v_mfma_f64_16x16x4_f64 (lane l supplies
// A[l & 15][l >> 4] and B[l >> 4][l & 15], register r of lane l is C[(l >> 4) + 4 r][l & 15]):
//   S^T [16 points, 16 rows] = Y [16 points, D] q^T [D, 16 rows]        (A from the LDS tile, B = the lane's q registers)
//   O   [16 rows, 16 cols]  += W [16 rows, 4 points] Y [4 points, 16 cols]
// S is computed TRANSPOSED so that register r of lane l holds the logit of row l & 15 against point (l >> 4) + 4 r: exactly the A operand
// of k step r of the second product.  The weights go from one product to the other without touching LDS.
//
// The four waves of a workgroup share the tile of the cloud in LDS, rows PITCH = 16 NB + 2 doubles apart: PITCH / 2 is odd, so the
// 16 x 2 doubles a half wave reads for the first product (16 points, 2 adjacent k) fall on 32 distinct bank pairs; the second product
// reads 2 points x 16 adjacent columns, two rows 4 banks apart, a two-way conflict that costs 2 LDS cycles per product of 64.  The
// next tile is fetched from memory into registers while the current one is computed on.
#include "common.h"

#include <math.h>

using namespace idiff;

namespace {

typedef double doublex4 __attribute__((ext_vector_type(4)));

constexpr int ROWS = 16;             // rows of x per wave
constexpr int TN = 32;               // points of the cloud per step
constexpr int WAVES = 4;
constexpr int THREADS = 64 * WAVES;
constexpr int NB_MAX = 12;           // 16-column blocks of the output a wave holds in registers
constexpr int D_MAX = 16 * NB_MAX;
constexpr int64_t N_MAX = 2147483647 - TN;

struct EmpParams {
  const float *x; const double *Y, *h, *c; const float *sigma, *mult; float *out, *ess;
  int B, N, D, D4;                   // D4: D rounded up to 4, the row pitch of Y
};

__device__ __forceinline__ doublex4 mfma(double a, double b, doublex4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// over the four lanes (l, l ^ 16, l ^ 32, l ^ 48) that share a row of x
__device__ __forceinline__ double row_max(double v) {
  v = fmax(v, __shfl_xor(v, 16, 64));
  return fmax(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ double row_sum(double v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}

template <int NB>
__global__ void __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(NB <= 6 ? 2 : 1, NB <= 6 ? 2 : 1)))
empirical_score_kernel(const EmpParams p) {
  constexpr int PITCH = 16 * NB + 2, KS = 4 * NB;
  __shared__ __attribute__((aligned(16))) double ys[TN * PITCH];
  __shared__ double hs[TN];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
  const int D = p.D, D4 = p.D4, half = D4 >> 1, N = p.N;
  const int64_t row0 = ((int64_t)blockIdx.x * WAVES + wave) * ROWS;

  for (int e = tid; e < TN * PITCH; e += THREADS) ys[e] = 0.0;   // the columns from D4 on are never written again

  // ---- q = x - c for the lane's row (l15) and its k (4 s + l4); a row that is not finite, or whose sigma is not positive and finite,
  // is computed as a row of zeros at sigma 1 and written as NaN
  const int64_t myrow = row0 + l15;
  const bool inb = myrow < p.B;
  float sg = inb ? p.sigma[myrow] : 1.f;
  int bad = (sg > 0.f && sg < INFINITY) ? 0 : 1;
  double q[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const int k = 4 * s + l4;
    const bool in = inb && k < D;
    const float xv = in ? p.x[myrow * D + k] : 0.f;
    if (!(fabsf(xv) < INFINITY)) bad = 1;
    q[s] = in ? (double)xv - p.c[k] : 0.0;
  }
  bad |= __shfl_xor(bad, 16, 64);
  bad |= __shfl_xor(bad, 32, 64);
  if (bad) {
    sg = 1.f;
#pragma unroll
    for (int s = 0; s < KS; ++s) q[s] = 0.0;
  }
  const double inv = 1.0 / ((double)sg * (double)sg);

  // ---- the tile loader: double2 e = tid + THREADS u of the [TN, D4 / 2] tile (TN D4 / 2 <= THREADS NB)
  // (its row e / half as a float product: e + 1/2 is never within 1 / (2 half) of a multiple of half, far above the rounding)
  const float rhalf = 1.f / (float)half;
  auto tile_row = [&](int u) { return (int)(((float)(tid + THREADS * u) + 0.5f) * rhalf); };
  double2 pre[NB];
  double hpre = INFINITY;
  auto fetch = [&](int n0) {
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      const int r = tile_row(u), c2 = tid + THREADS * u - r * half;
      pre[u] = make_double2(0.0, 0.0);                            // a row past N: zeros (its h is +inf: weight exactly 0)
      if (r < TN && n0 + r < N) pre[u] = *reinterpret_cast<const double2 *>(p.Y + (int64_t)(n0 + r) * D4 + 2 * c2);
    }
    if (tid < TN) hpre = n0 + tid < N ? p.h[n0 + tid] : INFINITY;
  };

  double m = -INFINITY, sw = 0.0, sw2 = 0.0;                      // of row l15: running maximum; this lane's share of the sums
  doublex4 acc[NB];
#pragma unroll
  for (int u = 0; u < NB; ++u) acc[u] = doublex4{0.0, 0.0, 0.0, 0.0};

  fetch(0);
  for (int n0 = 0; n0 < N; n0 += TN) {
    __syncthreads();                                              // everyone is done with the previous tile
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      const int r = tile_row(u), c2 = tid + THREADS * u - r * half;
      if (r < TN) *reinterpret_cast<double2 *>(ys + r * PITCH + 2 * c2) = pre[u];
    }
    if (tid < TN) hs[tid] = hpre;
    __syncthreads();
    if (n0 + TN < N) fetch(n0 + TN);

    // ---- logits, transposed: st[sub][r] = q_{l15} . y_{16 sub + l4 + 4 r}
    doublex4 st[2] = {doublex4{0.0, 0.0, 0.0, 0.0}, doublex4{0.0, 0.0, 0.0, 0.0}};
    const double *ya = ys + l15 * PITCH + l4;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      st[0] = mfma(ya[4 * s], q[s], st[0]);
      st[1] = mfma(ya[16 * PITCH + 4 * s], q[s], st[1]);
    }
    double lg[2][4], top = -INFINITY;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        lg[sub][r] = (st[sub][r] - hs[16 * sub + l4 + 4 * r]) * inv;
        top = fmax(top, lg[sub][r]);
      }
    const double mnew = fmax(m, row_max(top));
    const double alpha = m == mnew ? 1.0 : exp(m - mnew);         // the first tile: m = -inf, mnew finite, alpha = 0
    m = mnew;
    double ws = 0.0, ws2 = 0.0;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double w = lg[sub][r] == -INFINITY ? 0.0 : exp(lg[sub][r] - mnew);
        lg[sub][r] = w;
        ws += w;
        ws2 = fma(w, w, ws2);
      }
    sw = fma(sw, alpha, ws);
    sw2 = fma(sw2, alpha * alpha, ws2);
    if (__any(alpha != 1.0)) {                                    // wave-uniform; a factor of 1 changes no bit
      double ar[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) ar[r] = __shfl(alpha, l4 + 4 * r, 64);   // the accumulator's rows are l4 + 4 r
#pragma unroll
      for (int u = 0; u < NB; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[u][r] *= ar[r];
    }

    // ---- O += W Y: k step r of block sub takes the points 16 sub + 4 r + (0 .. 3), whose weights are register r of the four lanes
    const double *yb = ys + l4 * PITCH + l15;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int u = 0; u < NB; ++u) acc[u] = mfma(lg[sub][r], yb[(16 * sub + 4 * r) * PITCH + 16 * u], acc[u]);
  }

  // ---- out = mult (O / sum w - q), rounded once; ess = (sum w)^2 / sum w^2
  sw = row_sum(sw);
  sw2 = row_sum(sw2);
  if (l4 == 0 && inb && p.ess) p.ess[myrow] = bad ? __int_as_float(0x7fc00000) : (float)(sw * sw / sw2);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = l4 + 4 * r;
    const double tot = __shfl(sw, row, 64);
    const int badr = __shfl(bad, row, 64);
    const int64_t g = row0 + row;
    if (g >= p.B) continue;
    const double mu = p.mult ? (double)p.mult[g] : 1.0;
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      const int col = 16 * u + l15;
      if (col < D) {
        const double qv = (double)p.x[g * D + col] - p.c[col];
        p.out[g * D + col] = badr ? __int_as_float(0x7fc00000) : (float)(mu * (acc[u][r] / tot - qv));
      }
    }
  }
}

template <int NB> void launch(const EmpParams &p, hipStream_t stream) {
  const int64_t tiles = ceil_div64(p.B, ROWS);
  hipLaunchKernelGGL(empirical_score_kernel<NB>, dim3((unsigned)ceil_div64(tiles, WAVES)), dim3(THREADS), 0, stream, p);
}

}  // namespace

IDIFF_API int idiff_empirical_score_ok(int64_t N, int D) { return N >= 1 && N <= N_MAX && D >= 1 && D <= D_MAX ? 1 : 0; }

IDIFF_API int idiff_empirical_score_f32(const float *x, const double *Y, const double *h, const double *c, const float *sigma,
                                        const float *mult, float *out, float *ess, int B, int64_t N, int D, void *stream) {
  if (B < 0) return fail("empirical_score: B = %d", B);
  if (N < 1 || D < 1) return fail("empirical_score: N = %lld, D = %d", (long long)N, D);
  if (!idiff_empirical_score_ok(N, D))
    return fail("empirical_score: N = %lld, D = %d: the kernel keeps a row's fp64 output in registers and serves D <= %d, N <= %lld "
                "(ask idiff_empirical_score_ok)", (long long)N, D, D_MAX, (long long)N_MAX);
  if (!x || !Y || !h || !c || !sigma || !out) return fail("empirical_score: null pointer");
  if (((uintptr_t)x & 3) || ((uintptr_t)out & 3) || ((uintptr_t)sigma & 3) || ((uintptr_t)mult & 3) || ((uintptr_t)ess & 3) ||
      ((uintptr_t)Y & 15) || ((uintptr_t)h & 7) || ((uintptr_t)c & 7))
    return fail("empirical_score: x, sigma, mult, out and ess must be 4-byte aligned, h and c 8-byte aligned, Y 16-byte aligned");
  if (B == 0) return 0;
  EmpParams p = {x, Y, h, c, sigma, mult, out, ess, B, (int)N, D, (D + 3) / 4 * 4};
  hipStream_t s = (hipStream_t)stream;
  switch (ceil_div(D, 16)) {
    case 1: launch<1>(p, s); break;
    case 2: launch<2>(p, s); break;
    case 3: launch<3>(p, s); break;
    case 4: launch<4>(p, s); break;
    case 5: launch<5>(p, s); break;
    case 6: launch<6>(p, s); break;
    case 7: launch<7>(p, s); break;
    case 8: launch<8>(p, s); break;
    case 9: launch<9>(p, s); break;
    case 10: launch<10>(p, s); break;
    case 11: launch<11>(p, s); break;
    default: launch<12>(p, s); break;
  }
  return launch_status("empirical_score");
}
