// FLIPD of the empirical distribution of a point cloud (Kamkari et al. 2024; the Fokker-Planck form of LIDL, Tempczyk et al. 2022):
// with rho_sigma the cloud convolved with N(0, sigma^2 I) and s its score, D + sigma^2 (tr grad s + |s|^2) in closed form,
//
//   flipd(x, sigma) = sum_i w_i r_i^2 / sigma^2,   r_i^2 = |x_i - x|^2,   w = softmax_i(-r_i^2 / (2 sigma^2)),   ess = 1 / sum_i w_i^2
//
// a softmax-weighted mean of squared distances: one scalar per (query, sigma), nothing of width D kept per query, so D only streams
// and there is no cap on it.  All S bandwidths are served from one r^2 tile: the largest logit is at the nearest point for every sigma.
//
// ARITHMETIC: the centred, expanded route of csrc/empirical_score.hip, chosen over direct differences on the vector units because
// the distance contraction then runs on v_mfma_f64_16x16x4_f64 with a 16 x 64 register tile per wave (an LDS operand feeds 16 or 64
// products instead of one), and the centring keeps the cancellation independent of the cloud's offset.  The cloud is read as
// _lib.empirical_pack makes it (c the fp64 column mean, y_i = x_i - c padded to D4 columns, h_i = |y_i|^2 / 2), q = x - c is formed in
// fp64 before any product, and r_i^2 = max(0, |q|^2 + 2 h_i - 2 q . y_i).  The price is an ABSOLUTE error of (D + 8) u (|q| + Ymax)^2 on
// r^2 where direct differences have a relative one; tests/empirical_flipd_cases.py derives the bound from it.
//
// A workgroup of four waves owns 64 queries (16 a wave) and one contiguous range of the cloud (blockIdx.y of `splits`).  q and Y go
// through LDS in chunks of DC = 32 columns (zero-padded), rows PITCH = DC + 2 doubles apart (PITCH / 2 odd: the 16 rows x 2 adjacent k a
// half wave reads fall on 32 distinct bank pairs); the next chunk is fetched into registers while the current one is multiplied.  Only
// the [16 queries x 64 points] accumulators live in registers: lane l supplies A[l & 15][l >> 4] = y and B[l >> 4][l & 15] = q, register
// r of lane l is the product of point (l >> 4) + 4 r with query l & 15.
//
// SOFTMAX: per query the running minimum m of r^2; per (query, sigma) the sums of e, e^2 and e r^2 with e = exp(-(r^2 - m) / 2 sigma^2)
// (taken as exactly 0 below an argument of -700: 1e-304 of the nearest point's weight).  The four lanes that share a query share out
// the bandwidths (lane group l >> 4 takes sigma (l >> 4) + 4 j); the tile's r^2 go through the LDS the operands have left, so that
// each of the four sees all 64 points, in point order.  When the minimum moves the sums are rescaled by
// exp(-(m_old - m_new) / 2 sigma^2); a factor that underflows is 0, and the first tile (m_old = inf, sums 0) takes the factor 0
// without evaluating inf - inf.
//
// SPLIT OF N: the partial (m, sum e, sum e^2, sum e r^2) of every (query, sigma, range) goes to the workspace, and a second small launch
// merges the ranges in range order.  A range that is empty, or whose only point is the excluded one, leaves (inf, 0, 0, 0), which the
// merge skips.  No atomics: the same inputs and the same `splits` give the same bits.
#include "common.h"

#include <math.h>

using namespace idiff;

namespace {

typedef double doublex4 __attribute__((ext_vector_type(4)));

constexpr int ROWS = 16;             // queries per wave
constexpr int WAVES = 4;
constexpr int QR = ROWS * WAVES;     // queries per workgroup
constexpr int TN = 64;               // points of the cloud per tile
constexpr int DC = 32;               // columns per chunk
constexpr int PITCH = DC + 2;
constexpr int RP = TN + 1;           // pitch of a query's row of r^2 in LDS
static_assert(WAVES * ROWS * RP <= (TN + QR) * PITCH, "the r^2 slices reuse the operand tiles");
constexpr int THREADS = 64 * WAVES;
constexpr int S_MAX = 32;
constexpr int D_MAX = 65536;
constexpr int64_t N_MAX = 2147483647 - TN;
constexpr int SPLITS_MAX = 65535;    // gridDim.y
constexpr int CUS = 256;
constexpr double E_FLOOR = -700.0;   // exp of an argument below this is taken as 0

struct FlipdParams {
  const float *x; const double *Y, *h, *c; const float *sigmas; const int *exclude; double *ws;
  int P, N, D, D4, S, splits, per;   // per: points of a range, ceil(N / splits)
};

__device__ __forceinline__ doublex4 mfma(double a, double b, doublex4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// over the four lanes (l, l ^ 16, l ^ 32, l ^ 48) that share a query
__device__ __forceinline__ double row_min(double v) {
  v = fmin(v, __shfl_xor(v, 16, 64));
  return fmin(v, __shfl_xor(v, 32, 64));
}

template <int SL>
__global__ void __launch_bounds__(THREADS) empirical_flipd_partial_kernel(const FlipdParams p) {
  __shared__ __attribute__((aligned(16))) double smem[(TN + QR) * PITCH];
  double *const ys = smem, *const qs = smem + TN * PITCH;         // and, between two tiles, the r^2 slices of the four waves
  __shared__ double hs[TN], qqs[QR];
  __shared__ int bads[QR];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
  const int D = p.D, D4 = p.D4, S = p.S;
  const int64_t row0 = (int64_t)blockIdx.x * QR;
  const int split = blockIdx.y;
  const int64_t lo = (int64_t)split * p.per;
  const int nb = (int)(lo < p.N ? lo : p.N), ne = (int)(lo + p.per < p.N ? lo + p.per : p.N);
  const int myrow_l = ROWS * wave + l15;                          // this lane's query, within the workgroup
  const int64_t myrow = row0 + myrow_l;
  const double inf = INFINITY, nan = __longlong_as_double(0x7ff8000000000000ll);

  // ---- this lane's bandwidths: sigma l4 + 4 j; one that is not positive and finite is computed at 1 (the merge writes NaN)
  double inv2[SL];
#pragma unroll
  for (int j = 0; j < SL; ++j) {
    const int s = l4 + 4 * j;
    const float sg = s < S ? p.sigmas[s] : 1.f;
    const double sd = (sg > 0.f && sg < INFINITY) ? (double)sg : 1.0;
    inv2[j] = 0.5 / (sd * sd);
  }
  double m = inf, se[SL], see[SL], ser[SL];
#pragma unroll
  for (int j = 0; j < SL; ++j) se[j] = see[j] = ser[j] = 0.0;

  const int ntiles = (ne - nb + TN - 1) / TN, nchunks = (D + DC - 1) / DC;
  if (ntiles > 0) {
    if (tid < QR) bads[tid] = 0;
    const int excl = (p.exclude && myrow < p.P) ? p.exclude[myrow] : -1;

    // ---- the loaders.  q: thread t takes query t >> 2 of the workgroup, columns 8 (t & 3) .. + 7 of the chunk; Y: double2
    // e = t + THREADS u of the [TN, DC / 2] chunk
    const int qrow = tid >> 2, qk = 8 * (tid & 3);
    const int64_t grow = row0 + qrow;
    const bool rin = grow < p.P;
    double2 ypre[4];
    float xpre[8];
    double cpre[8], hpre = inf, qq = 0.0;
    int mybad = 0;
    auto fetch = [&](int n0, int k0, bool with_h) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = tid + THREADS * u, r = e >> 4, col = k0 + 2 * (e & 15);
        ypre[u] = make_double2(0.0, 0.0);                         // a row past the range or a column past D4: zeros
        if (n0 + r < ne && col < D4) ypre[u] = *reinterpret_cast<const double2 *>(p.Y + (int64_t)(n0 + r) * D4 + col);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int k = k0 + qk + u;
        const bool in = rin && k < D;
        xpre[u] = in ? p.x[grow * D + k] : 0.f;
        cpre[u] = in ? p.c[k] : 0.0;
      }
      if (with_h && tid < TN) hpre = n0 + tid < ne ? p.h[n0 + tid] : inf;   // a row past the range: r^2 = inf, no weight
    };

    fetch(nb, 0, true);
    for (int tile = 0; tile < ntiles; ++tile) {
      const int n0 = nb + tile * TN;
      doublex4 st[4];
#pragma unroll
      for (int b = 0; b < 4; ++b) st[b] = doublex4{0.0, 0.0, 0.0, 0.0};
      for (int ch = 0; ch < nchunks; ++ch) {
        __syncthreads();                                          // everyone is done with the previous chunk
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int e = tid + THREADS * u;
          *reinterpret_cast<double2 *>(ys + (e >> 4) * PITCH + 2 * (e & 15)) = ypre[u];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const bool fin = fabsf(xpre[u]) < INFINITY;
          if (!fin) mybad = 1;
          const double qv = fin ? (double)xpre[u] - cpre[u] : 0.0;
          qs[qrow * PITCH + qk + u] = qv;
          if (tile == 0) qq = fma(qv, qv, qq);
        }
        if (ch == 0 && tid < TN) hs[tid] = hpre;
        __syncthreads();
        if (ch + 1 < nchunks) fetch(n0, DC * (ch + 1), false);
        else if (tile + 1 < ntiles) fetch(n0 + TN, 0, true);

        const double *qa = qs + myrow_l * PITCH + l4, *ya = ys + l15 * PITCH + l4;
#pragma unroll
        for (int s = 0; s < DC / 4; ++s) {
          const double bq = qa[4 * s];
#pragma unroll
          for (int b = 0; b < 4; ++b) st[b] = mfma(ya[16 * b * PITCH + 4 * s], bq, st[b]);
        }
      }
      if (tile == 0) {                                            // |q|^2 of every query of the workgroup, and whether it is finite
        qq += __shfl_xor(qq, 1, 64);
        qq += __shfl_xor(qq, 2, 64);
        if ((tid & 3) == 0) qqs[qrow] = qq;
        if (mybad) bads[qrow] = 1;
        __syncthreads();
      }
      const double myqq = qqs[myrow_l];

      // ---- r^2 of the tile's 64 points against this lane's query: register r of block b is point 16 b + l4 + 4 r.  They go to the
      // wave's [16 queries, 64 points] slice of LDS (the operand tiles are done with), where every lane of a query reads them all
      __syncthreads();
      double *mine = smem + wave * (ROWS * RP) + l15 * RP, tmin = inf;
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = 16 * b + l4 + 4 * r;
          double v = fmax(0.0, fma(-2.0, st[b][r], myqq + 2.0 * hs[i]));
          if (n0 + i >= ne || n0 + i == excl) v = inf;
          mine[i] = v;
          tmin = fmin(tmin, v);
        }
      __syncthreads();
      const double mnew = fmin(m, row_min(tmin));
      if (mnew < m) {                                             // the minimum moved: rescale (from m = inf the sums are 0)
#pragma unroll
        for (int j = 0; j < SL; ++j) {
          const double a = m == inf ? 0.0 : exp(-(m - mnew) * inv2[j]);
          se[j] *= a;
          see[j] *= a * a;
          ser[j] *= a;
        }
        m = mnew;
      }
      if (m < inf) {
#pragma unroll 2
        for (int i = 0; i < TN; ++i) {                            // in point order
          const double v = mine[i];
#pragma unroll
          for (int j = 0; j < SL; ++j) {
            const double a = -(v - m) * inv2[j];                  // v = inf: -inf, no weight
            if (a >= E_FLOOR) {
              const double e = exp(a);
              se[j] += e;
              see[j] = fma(e, e, see[j]);
              ser[j] = fma(e, v, ser[j]);
            }
          }
        }
      }
    }
    __syncthreads();
    if (bads[myrow_l]) m = nan;                                   // a query that is not finite: the merge writes NaN
  }

  if (myrow < p.P) {
#pragma unroll
    for (int j = 0; j < SL; ++j) {
      const int s = l4 + 4 * j;
      if (s < S) {
        double *w = p.ws + ((myrow * S + s) * p.splits + split) * 4;
        w[0] = m;
        w[1] = se[j];
        w[2] = see[j];
        w[3] = ser[j];
      }
    }
  }
}

// One thread per (query, sigma): the ranges in order.
__global__ void __launch_bounds__(THREADS) empirical_flipd_merge_kernel(const double *ws, const float *sigmas, double *flipd, float *ess,
                                                                       int64_t PS, int S, int splits) {
  const int64_t g = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (g >= PS) return;
  const float sg = sigmas[g % S];
  const bool ok = sg > 0.f && sg < INFINITY;
  const double sd = ok ? (double)sg : 1.0, s2 = sd * sd, inv2 = 0.5 / s2, inf = INFINITY;
  double m = inf, a = 0.0, b = 0.0, c = 0.0;
  bool bad = !ok;
  for (int k = 0; k < splits; ++k) {
    const double *w = ws + (g * splits + k) * 4;
    const double mk = w[0];
    if (mk != mk) bad = true;
    else if (mk < inf) {                                          // (an empty range is the neutral element)
      if (mk < m) {
        const double f = m == inf ? 0.0 : exp(-(m - mk) * inv2);
        a = fma(a, f, w[1]);
        b = fma(b, f * f, w[2]);
        c = fma(c, f, w[3]);
        m = mk;
      } else {
        const double f = exp(-(mk - m) * inv2);
        a = fma(w[1], f, a);
        b = fma(w[2], f * f, b);
        c = fma(w[3], f, c);
      }
    }
  }
  if (bad || !(a > 0.0)) {                                        // no admissible point: NaN
    flipd[g] = __longlong_as_double(0x7ff8000000000000ll);
    ess[g] = __int_as_float(0x7fc00000);
  } else {
    flipd[g] = c / (s2 * a);
    ess[g] = (float)(a * a / b);
  }
}

template <int SL> void launch(const FlipdParams &p, hipStream_t stream) {
  hipLaunchKernelGGL(empirical_flipd_partial_kernel<SL>, dim3((unsigned)ceil_div64(p.P, QR), (unsigned)p.splits), dim3(THREADS), 0, stream, p);
}

}  // namespace

IDIFF_API int idiff_empirical_flipd_ok(int64_t N, int D, int S) {
  return N >= 1 && N <= N_MAX && D >= 1 && D <= D_MAX && S >= 1 && S <= S_MAX ? 1 : 0;
}

IDIFF_API int64_t idiff_empirical_flipd_workspace_doubles(int64_t P, int S, int splits) {
  return P < 0 || S < 1 || splits < 1 ? 0 : 4 * P * S * splits;
}

// Two workgroups a CU when the queries alone give fewer, never a range shorter than one tile; 1 when the queries fill the card.
IDIFF_API int idiff_empirical_flipd_splits(int64_t P, int64_t N, int D) {
  (void)D;
  if (P < 1 || N < 1) return 1;
  const int64_t blocks = ceil_div64(P, QR);
  if (blocks >= CUS) return 1;
  int64_t s = ceil_div64(2 * CUS, blocks);
  const int64_t tiles = ceil_div64(N, TN);
  if (s > tiles) s = tiles;
  if (s > SPLITS_MAX) s = SPLITS_MAX;
  return (int)s;
}

IDIFF_API int idiff_empirical_flipd_f64(const float *x, const double *Y, const double *h, const double *c, const float *sigmas,
                                        const int *exclude, double *flipd, float *ess, double *workspace, int64_t workspace_doubles,
                                        int64_t P, int64_t N, int D, int S, int splits, void *stream) {
  if (P < 0 || P > 2147483647) return fail("empirical_flipd: P = %lld", (long long)P);
  if (N < 1 || D < 1 || S < 1) return fail("empirical_flipd: N = %lld, D = %d, S = %d", (long long)N, D, S);
  if (!idiff_empirical_flipd_ok(N, D, S))
    return fail("empirical_flipd: N = %lld, D = %d, S = %d: served are N <= %lld, D <= %d and S <= %d bandwidths a call "
                "(ask idiff_empirical_flipd_ok)", (long long)N, D, S, (long long)N_MAX, D_MAX, S_MAX);
  if (splits < 1 || splits > SPLITS_MAX) return fail("empirical_flipd: splits = %d, must be 1 .. %d", splits, SPLITS_MAX);
  const int64_t need = idiff_empirical_flipd_workspace_doubles(P, S, splits);
  if (workspace_doubles < need)
    return fail("empirical_flipd: workspace of %lld doubles, P = %lld, S = %d and splits = %d need %lld "
                "(idiff_empirical_flipd_workspace_doubles)", (long long)workspace_doubles, (long long)P, S, splits, (long long)need);
  if (!x || !Y || !h || !c || !sigmas || !flipd || !ess || (!workspace && need)) return fail("empirical_flipd: null pointer");
  if (((uintptr_t)x & 3) || ((uintptr_t)sigmas & 3) || ((uintptr_t)exclude & 3) || ((uintptr_t)ess & 3) || ((uintptr_t)Y & 15) ||
      ((uintptr_t)h & 7) || ((uintptr_t)c & 7) || ((uintptr_t)flipd & 7) || ((uintptr_t)workspace & 7))
    return fail("empirical_flipd: x, sigmas, exclude and ess must be 4-byte aligned, h, c, flipd and the workspace 8-byte aligned, "
                "Y 16-byte aligned");
  if (P == 0) return 0;
  FlipdParams p = {x, Y, h, c, sigmas, exclude, workspace, (int)P, (int)N, D, (D + 3) / 4 * 4, S, splits, (int)ceil_div64(N, splits)};
  hipStream_t s = (hipStream_t)stream;
  switch (ceil_div(S, 4)) {
    case 1: launch<1>(p, s); break;
    case 2: launch<2>(p, s); break;
    case 3: launch<3>(p, s); break;
    case 4: launch<4>(p, s); break;
    case 5: launch<5>(p, s); break;
    case 6: launch<6>(p, s); break;
    case 7: launch<7>(p, s); break;
    default: launch<8>(p, s); break;
  }
  if (int rc = launch_status("empirical_flipd")) return rc;
  const int64_t PS = P * S;
  hipLaunchKernelGGL(empirical_flipd_merge_kernel, dim3((unsigned)ceil_div64(PS, THREADS)), dim3(THREADS), 0, s, workspace, sigmas, flipd,
                     ess, PS, S, splits);
  return launch_status("empirical_flipd merge");
}
