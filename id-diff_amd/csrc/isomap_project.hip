// Out-of-sample side of Isomap (what sklearn.manifold.Isomap.transform does for points that were not in the fit): the exact
// nearest fitted points of every query, and the projection of the queries onto the fitted embedding in one launch.  All fp64,
// plain VALU code.
//
//   idiff_knn_cross_f64        for every row of Xq [M, D] the k nearest rows of X [N, D] (both fp32) by fp64 brute force, in the style
//                              of the exact pass of knn.hip: a workgroup takes queries b, b + G, ...; one wave per candidate row
//                              (lanes over D, the sum of squared differences of the fp32 coordinates in fp64) fills the workgroup's N
//                              doubles of workspace, then k rounds of a lexicographic (distance, index) minimum pick the answer:
//                              ascending, equal distances by lower index.  No row is excluded (a query that is a fitted point finds
//                              itself at distance 0).
//   idiff_isomap_project_f64   Z [M, c] from the queries' neighbours (dist, idx [M, kn]), the fitted geodesic matrix D [N, N], A [N, c]
//                              = eigenvectors / sqrt(eigenvalue), and the column means colmean [N] and grand mean of -1/2 D o D:
//                                g_ij = min_n (dist[i, n] + D[idx[i, n], j]),   g'_ij = -1/2 g_ij^2
//                                Z[i, :] = sum_j (g'_ij - colmean_j - mean_j g'_ij + grand) A[j, :]
//                              in one launch.  One wave per query, four queries per workgroup (neighbouring queries gather neighbouring rows of D:
//                              they meet in L2).  A lane walks the columns j = lane, lane + 64, ... accumulating sum_j g'_ij A[j, :]
//                              and sum_j g'_ij, the wave adds them in a butterfly, and the three centring terms come at the end
//                              from sum_j colmean_j A[j, :] and sum_j A[j, :], which one launch computes first (scratch).  The
//                              [M, N] matrix of geodesic distances is never written; a wave walks the columns once per 8
//                              components (once in all for c <= 8, 8 times at c = 64, forming g'_ij again each time).  Every sum is a fixed tree: the same bits
//                              on every launch.  An index outside [0, N) is dropped, never an address.
#include "common.h"

#include <math.h>

using namespace idiff;

namespace {

constexpr int K_MAX = 64;          // most neighbours per query (both entry points)
constexpr int C_MAX = 64;          // most components
constexpr int CT = 8;              // components a wave accumulates per walk over the columns
constexpr int QPB = 4;             // queries per workgroup of the projection: one per wave
constexpr int CROSS_GRID = 256;    // workgroups of the neighbour search (each owns N doubles of workspace)
constexpr int N_LIMIT = 1 << 20;

__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ double block_sum(double v, double *red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ __forceinline__ bool key_less(double da, int ia, double db, int ib) { return da < db || (da == db && ia < ib); }

__global__ void __launch_bounds__(256)
knn_cross_kernel(const float *__restrict__ Xq, const float *__restrict__ X, int M, int N, int D, int k, double *__restrict__ scr,
                 double *__restrict__ dist, int64_t *__restrict__ idx) {
  __shared__ double red_d[4];
  __shared__ int red_i[4];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  double *sd = scr + (int64_t)blockIdx.x * N;
  for (int q = blockIdx.x; q < M; q += gridDim.x) {
    for (int j = w; j < N; j += 4) {
      double acc = 0.0;
      for (int d = lane; d < D; d += 64) {
        const double diff = (double)Xq[(int64_t)q * D + d] - (double)X[(int64_t)j * D + d];
        acc += diff * diff;
      }
      acc = wave_sum(acc);
      if (lane == 0) sd[j] = acc;
    }
    __syncthreads();
    double pd = -INFINITY;
    int pi = -1;
    for (int r = 0; r < k; ++r) {
      double bestd = INFINITY;
      int besti = 0x7fffffff;
      for (int e = t; e < N; e += 256) {
        const double d = sd[e];
        if (key_less(pd, pi, d, e) && key_less(d, e, bestd, besti)) { bestd = d; besti = e; }
      }
      for (int o = 32; o > 0; o >>= 1) {
        const double od = __shfl_xor(bestd, o);
        const int oj = __shfl_xor(besti, o);
        if (key_less(od, oj, bestd, besti)) { bestd = od; besti = oj; }
      }
      if (lane == 0) { red_d[w] = bestd; red_i[w] = besti; }
      __syncthreads();
      bestd = red_d[0];
      besti = red_i[0];
      for (int v = 1; v < 4; ++v)
        if (key_less(red_d[v], red_i[v], bestd, besti)) { bestd = red_d[v]; besti = red_i[v]; }
      if (t == 0) {
        dist[(int64_t)q * k + r] = sqrt(bestd);
        idx[(int64_t)q * k + r] = besti;
      }
      pd = bestd;
      pi = besti;
      __syncthreads();                                // red_* reused by the next round, sd by the next query
    }
  }
}

// sums[cc] = sum_j colmean_j A[j, cc],  sums[c + cc] = sum_j A[j, cc]: one workgroup per component
__global__ void __launch_bounds__(256)
project_sums_kernel(const double *__restrict__ A, const double *__restrict__ colmean, int N, int c, double *__restrict__ sums) {
  __shared__ double red[4];
  const int cc = blockIdx.x;
  double ca = 0.0, sa = 0.0;
  for (int j = threadIdx.x; j < N; j += 256) {
    const double a = A[(int64_t)j * c + cc];
    ca += colmean[j] * a;
    sa += a;
  }
  ca = block_sum(ca, red);
  sa = block_sum(sa, red);
  if (threadIdx.x == 0) { sums[cc] = ca; sums[c + cc] = sa; }
}

__global__ void __launch_bounds__(256)
project_kernel(const double *__restrict__ dist, const int64_t *__restrict__ idx, int M, int kn, const double *__restrict__ D, int N,
               const double *__restrict__ A, int c, const double *__restrict__ sums, const double *__restrict__ grand,
               double *__restrict__ Z) {
  __shared__ double nd[QPB][K_MAX];
  __shared__ int ni[QPB][K_MAX];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int q = QPB * (int)blockIdx.x + w;
  if (q < M && lane < kn) {
    const int64_t j = idx[(int64_t)q * kn + lane];
    ni[w][lane] = (j >= 0 && j < N) ? (int)j : -1;       // an index outside the fit is dropped, never an address
    nd[w][lane] = dist[(int64_t)q * kn + lane];
  }
  __syncthreads();
  if (q >= M) return;
  const double gm = grand[0];
  for (int c0 = 0; c0 < c; c0 += CT) {
    double acc[CT], s0 = 0.0;
#pragma unroll
    for (int t = 0; t < CT; ++t) acc[t] = 0.0;
    for (int j = lane; j < N; j += 64) {
      double g = INFINITY;
      for (int n = 0; n < kn; ++n) {
        const int r = ni[w][n];
        if (r >= 0) g = fmin(g, nd[w][n] + D[(int64_t)r * N + j]);
      }
      const double gp = -0.5 * g * g;
      s0 += gp;
#pragma unroll
      for (int t = 0; t < CT; ++t)
        if (c0 + t < c) acc[t] += gp * A[(int64_t)j * c + c0 + t];
    }
    s0 = wave_sum(s0);
#pragma unroll
    for (int t = 0; t < CT; ++t) {
      const double s1 = wave_sum(acc[t]);
      if (lane == 0 && c0 + t < c) Z[(int64_t)q * c + c0 + t] = (s1 - sums[c0 + t]) + (gm - s0 / N) * sums[c + c0 + t];
    }
  }
}

}  // namespace

IDIFF_API int64_t idiff_knn_cross_workspace_bytes(int M, int N) {
  if (M < 1 || N < 1 || N > N_LIMIT) return 0;
  return (int64_t)(M < CROSS_GRID ? M : CROSS_GRID) * N * 8;
}

IDIFF_API int idiff_knn_cross_f64(const float *Xq, int M, const float *X, int N, int D, int k, void *workspace, int64_t workspace_bytes,
                                  double *dist, int64_t *idx, void *stream) {
  if (M < 1) return fail("knn_cross: M = %d, need at least 1 query", M);
  if (N < 1) return fail("knn_cross: N = %d, need at least 1 point", N);
  if (N > N_LIMIT) return fail("knn_cross: N = %d above %d", N, N_LIMIT);
  if (D < 1) return fail("knn_cross: D = %d, need at least 1 dimension", D);
  if (k < 1 || k > K_MAX) return fail("knn_cross: k = %d outside 1..%d", k, K_MAX);
  if (k > N) return fail("knn_cross: k = %d but only N = %d points", k, N);
  if (!Xq || !X || !workspace || !dist || !idx) return fail("knn_cross: null pointer");
  if ((int64_t)N * D > ((int64_t)1 << 40) || (int64_t)M * D > ((int64_t)1 << 40)) return fail("knn_cross: N * D too large");
  const int64_t need = idiff_knn_cross_workspace_bytes(M, N);
  if (workspace_bytes < need)
    return fail("knn_cross: workspace of %lld bytes, need %lld (idiff_knn_cross_workspace_bytes)", (long long)workspace_bytes, (long long)need);
  if (((uintptr_t)workspace & 7) != 0) return fail("knn_cross: workspace must be 8-byte aligned");
  const int G = M < CROSS_GRID ? M : CROSS_GRID;
  hipLaunchKernelGGL(knn_cross_kernel, dim3(G), dim3(256), 0, (hipStream_t)stream, Xq, X, M, N, D, k, (double *)workspace, dist, idx);
  return launch_status("knn_cross");
}

IDIFF_API int64_t idiff_isomap_project_scratch_doubles(int c) { return c < 1 || c > C_MAX ? 0 : 2 * (int64_t)c; }

IDIFF_API int idiff_isomap_project_f64(const double *dist, const int64_t *idx, int M, int k, const double *D, int N, const double *A, int c,
                                       const double *colmean, const double *grand, double *Z, double *scratch, void *stream) {
  if (M < 1) return fail("isomap_project: M = %d, need at least 1 query", M);
  if (N < 1) return fail("isomap_project: N = %d, need at least 1 point", N);
  if (N > N_LIMIT) return fail("isomap_project: N = %d above %d", N, N_LIMIT);
  if (k < 1 || k > K_MAX) return fail("isomap_project: k = %d neighbours outside 1..%d", k, K_MAX);
  if (c < 1 || c > C_MAX) return fail("isomap_project: %d components outside 1..%d", c, C_MAX);
  if (!dist || !idx || !D || !A || !colmean || !grand || !Z || !scratch) return fail("isomap_project: null pointer");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(project_sums_kernel, dim3(c), dim3(256), 0, st, A, colmean, N, c, scratch);
  hipLaunchKernelGGL(project_kernel, dim3(ceil_div(M, QPB)), dim3(256), 0, st, dist, idx, M, k, D, N, A, c, scratch, grand, Z);
  return launch_status("isomap_project");
}
