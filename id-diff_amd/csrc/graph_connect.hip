// The connected components of a neighbourhood graph and the edges scikit-learn joins them with
// (sklearn.utils.graph._fix_connected_components, mode="distance": between every two components the closest pair of points).
//
//   idiff_component_labels_f64   labels [N] (int32) and their number C (device scalar) from the finite pattern of a shortest-path
//                                matrix D [N, N]: two vertices share a component exactly when their distance is finite, so a
//                                component is named by its smallest vertex, the first column of the row with a finite entry
//                                (one wave per row; it stops at the diagonal, which is finite).  One workgroup then numbers the
//                                components 0 .. C - 1 in the order of those smallest vertices (a ballot scan over the roots) and
//                                hands every vertex the number of its root.
//   idiff_component_bridges_f64  for every pair of components i > j the pair of points (a in i, b in j) of smallest Euclidean
//                                distance, by fp64 brute force from the fp32 coordinates: a workgroup owns a 32 x 32 tile of
//                                (a, b) pairs, each lane 2 x 2 of them, the coordinates staged through LDS 32 at a time; a tile
//                                with no pair to look at (no a of a later component than b) ends before any arithmetic.  The
//                                minimum per pair of components is taken in two passes of the SAME kernel, so the same bits
//                                twice: pass 0 an unsigned 64-bit atomic minimum of the squared distance (non-negative doubles
//                                order as their bit patterns), pass 1 an atomic minimum of the key (a << 32 | b) among the pairs
//                                that equal it.  The result does not depend on the launch order: exact ties go to the smallest
//                                a, then the smallest b, which is numpy's argmin over X[idx_i] x X[idx_j] (row-major, ranks by
//                                ascending vertex index).  No floating-point atomics.
#include "common.h"

#include <math.h>

using namespace idiff;

namespace {

constexpr int N_LIMIT = 1 << 20;
constexpr int C_LIMIT = 1024;      // most components (523,776 pairs of them)
constexpr int BT = 32;             // tile of the bridge search: 32 x 32 pairs of points
constexpr int DC = 32;             // coordinates staged per step
typedef unsigned long long u64;
constexpr u64 INF_BITS = 0x7ff0000000000000ull;
constexpr u64 NO_KEY = ~0ull;

// ------------------------------------------------------------------------------------------------ labels
__global__ void __launch_bounds__(256) first_reachable_kernel(const double *__restrict__ D, int N, int *__restrict__ first) {
  const int lane = threadIdx.x & 63;
  const int i = 4 * (int)blockIdx.x + (threadIdx.x >> 6);
  if (i >= N) return;                                   // the whole wave
  int f = i;
  for (int j0 = 0; j0 <= i; j0 += 64) {
    const int j = j0 + lane;
    const bool fin = j <= i && isfinite(D[(int64_t)i * N + j]);
    const u64 m = __ballot(fin);
    if (m) {
      f = j0 + __ffsll((long long)m) - 1;
      break;
    }
  }
  if (lane == 0) first[i] = f;                          // 0 <= f <= i
}

// one workgroup.  first[i] in [0, i]; a root is a vertex with first[i] == i
__global__ void __launch_bounds__(256) compact_labels_kernel(const int *__restrict__ first, int N, int *labels, int *__restrict__ count) {
  __shared__ int wsum[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int base = 0;
  for (int i0 = 0; i0 < N; i0 += 256) {
    const int i = i0 + threadIdx.x;
    const bool root = i < N && first[i] == i;
    const u64 m = __ballot(root);
    const int before = __popcll(m & ((1ull << lane) - 1));
    __syncthreads();                                    // the previous round's wsum has been read
    if (lane == 0) wsum[w] = __popcll(m);
    __syncthreads();
    int off = base;
    for (int v = 0; v < w; ++v) off += wsum[v];
    if (root) labels[i] = off + before;
    base += (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
  }
  __syncthreads();                                      // the roots' labels are written
  for (int i = threadIdx.x; i < N; i += 256) {
    const int f = first[i];
    if (f != i && f >= 0 && f < i) labels[i] = labels[f];
  }
  if (threadIdx.x == 0) count[0] = base;
}

// ------------------------------------------------------------------------------------------------ bridges
__global__ void __launch_bounds__(256) bridges_init_kernel(u64 *__restrict__ best, u64 *__restrict__ key, int B) {
  for (int e = blockIdx.x * 256 + threadIdx.x; e < B; e += gridDim.x * 256) {
    best[e] = INF_BITS;
    key[e] = NO_KEY;
  }
}

// tile (blockIdx.y, blockIdx.x) of the pairs (a, b).  pass 0: best[pair of components] = min of the squared distance;
// pass 1: key = min of (a << 32 | b) among the pairs whose squared distance is that minimum
__global__ void __launch_bounds__(256)
bridges_kernel(const float *__restrict__ X, int N, int D, const int *__restrict__ labels, int C, u64 *best, u64 *key, int pass) {
  __shared__ float xa[BT][DC + 1], xb[BT][DC + 1];
  __shared__ int la[BT], lb[BT];
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
  const int a0 = blockIdx.y * BT, b0 = blockIdx.x * BT;
  if (t < BT) {
    const int a = a0 + t;
    const int l = a < N ? labels[a] : -1;
    la[t] = (l >= 0 && l < C) ? l : -1;                 // a label outside 0 .. C - 1 is dropped, never an address
  } else if (t < 2 * BT) {
    const int b = b0 + t - BT;
    const int l = b < N ? labels[b] : -1;
    lb[t - BT] = (l >= 0 && l < C) ? l : -1;
  }
  __syncthreads();
  bool want[2][2];
  int any = 0;
  for (int r = 0; r < 2; ++r)
    for (int c = 0; c < 2; ++c) {
      want[r][c] = lb[tx + 16 * c] >= 0 && la[ty + 16 * r] > lb[tx + 16 * c];
      any |= want[r][c];
    }
  if (!__syncthreads_or(any)) return;                   // the whole workgroup
  double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
  for (int d0 = 0; d0 < D; d0 += DC) {
    if (d0 > 0) __syncthreads();
    for (int e = t; e < BT * DC; e += 256) {
      const int r = e / DC, d = d0 + e % DC;
      xa[r][e % DC] = (a0 + r < N && d < D) ? X[(int64_t)(a0 + r) * D + d] : 0.f;
      xb[r][e % DC] = (b0 + r < N && d < D) ? X[(int64_t)(b0 + r) * D + d] : 0.f;
    }
    __syncthreads();
    const int dn = min(DC, D - d0);
    for (int d = 0; d < dn; ++d) {
      const double p0 = xa[ty][d], p1 = xa[ty + 16][d], q0 = xb[tx][d], q1 = xb[tx + 16][d];
      const double e00 = p0 - q0, e01 = p0 - q1, e10 = p1 - q0, e11 = p1 - q1;
      acc[0][0] = fma(e00, e00, acc[0][0]);
      acc[0][1] = fma(e01, e01, acc[0][1]);
      acc[1][0] = fma(e10, e10, acc[1][0]);
      acc[1][1] = fma(e11, e11, acc[1][1]);
    }
  }
  for (int r = 0; r < 2; ++r)
    for (int c = 0; c < 2; ++c) {
      if (!want[r][c]) continue;
      const int i = la[ty + 16 * r], j = lb[tx + 16 * c];                 // 0 <= j < i < C
      const int pair = i * (i - 1) / 2 + j;
      const u64 bits = (u64)__double_as_longlong(acc[r][c]);
      if (pass == 0) {
        if (bits < best[pair]) atomicMin(&best[pair], bits);              // the plain read only spares atomics: best never grows
      } else if (bits == best[pair]) {
        atomicMin(&key[pair], ((u64)(a0 + ty + 16 * r) << 32) | (u64)(b0 + tx + 16 * c));
      }
    }
}

__global__ void __launch_bounds__(256)
bridges_finish_kernel(const u64 *__restrict__ best, const u64 *__restrict__ key, int B, int64_t *__restrict__ bi, int64_t *__restrict__ bj,
                      double *__restrict__ bw) {
  for (int e = blockIdx.x * 256 + threadIdx.x; e < B; e += gridDim.x * 256) {
    const u64 k = key[e];
    const bool have = k != NO_KEY;                      // a component number no vertex carries leaves its pairs empty
    bi[e] = have ? (int64_t)(k >> 32) : -1;
    bj[e] = have ? (int64_t)(k & 0xffffffffull) : -1;
    bw[e] = have ? sqrt(__longlong_as_double((long long)best[e])) : INFINITY;
  }
}

}  // namespace

IDIFF_API int idiff_component_labels_f64(const double *D, int N, int32_t *labels, int32_t *count, int32_t *scratch, void *stream) {
  if (N < 1) return fail("component_labels: N = %d, need at least 1 vertex", N);
  if (N > N_LIMIT) return fail("component_labels: N = %d above %d", N, N_LIMIT);
  if (!D || !labels || !count || !scratch) return fail("component_labels: null pointer");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(first_reachable_kernel, dim3(ceil_div(N, 4)), dim3(256), 0, st, D, N, scratch);
  hipLaunchKernelGGL(compact_labels_kernel, dim3(1), dim3(256), 0, st, scratch, N, labels, count);
  return launch_status("component_labels");
}

IDIFF_API int64_t idiff_component_bridges_workspace_bytes(int C) {
  return C < 2 || C > C_LIMIT ? 0 : 16 * ((int64_t)C * (C - 1) / 2);
}

IDIFF_API int idiff_component_bridges_f64(const float *X, int N, int D, const int32_t *labels, int C, void *workspace,
                                          int64_t workspace_bytes, int64_t *bi, int64_t *bj, double *bw, void *stream) {
  if (N < 1) return fail("component_bridges: N = %d, need at least 1 point", N);
  if (N > N_LIMIT) return fail("component_bridges: N = %d above %d", N, N_LIMIT);
  if (D < 1) return fail("component_bridges: D = %d, need at least 1 coordinate", D);
  if (C < 2) return fail("component_bridges: C = %d components, need at least 2", C);
  if (C > C_LIMIT) return fail("component_bridges: C = %d components above %d", C, C_LIMIT);
  if (C > N) return fail("component_bridges: C = %d components of N = %d points", C, N);
  if (!X || !labels || !bi || !bj || !bw || !workspace) return fail("component_bridges: null pointer");
  if (((uintptr_t)workspace & 7) != 0) return fail("component_bridges: workspace must be 8-byte aligned");
  const int B = C * (C - 1) / 2;
  if (workspace_bytes < 16 * (int64_t)B)
    return fail("component_bridges: workspace of %lld bytes, need %lld", (long long)workspace_bytes, (long long)(16 * (int64_t)B));
  hipStream_t st = (hipStream_t)stream;
  u64 *best = (u64 *)workspace, *key = best + B;
  const int nt = ceil_div(N, BT);
  hipLaunchKernelGGL(bridges_init_kernel, dim3(streaming_grid(B, 256)), dim3(256), 0, st, best, key, B);
  for (int pass = 0; pass < 2; ++pass)
    hipLaunchKernelGGL(bridges_kernel, dim3(nt, nt), dim3(256), 0, st, X, N, D, labels, C, best, key, pass);
  hipLaunchKernelGGL(bridges_finish_kernel, dim3(streaming_grid(B, 256)), dim3(256), 0, st, best, key, B, bi, bj, bw);
  return launch_status("component_bridges");
}
