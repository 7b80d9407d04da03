// Geodesic distances of a neighbourhood graph and the centred kernel Isomap takes its eigenvalues from (the pieces of
// sklearn.manifold.Isomap that isomap.py of the reference goes through: kneighbors_graph -> shortest_path -> KernelCenterer).
// All fp64, plain VALU code: the (min, +) semiring has no matrix-core form.
//
//   idiff_knn_graph_f64      dense weighted graph G [N, N] of a kNN result: fill (0 on the diagonal, +inf elsewhere), one store
//                            per neighbour (the columns of one row are distinct, rows do not overlap: no conflicts, no
//                            atomics), then G = min(G, G^T) by pairs of 32 x 32 tiles, each pair owned by one workgroup.
//   idiff_apsp_f64           blocked Floyd-Warshall in place, tile T = 64.  Round b (one per diagonal tile), three launches:
//                              1. the diagonal tile (b, b): the scalar recurrence over its <= 64 pivots, in LDS, one workgroup;
//                              2. the tiles of row b and of column b:  C = min(C, D (x) C) resp. min(C, C (x) D), D the closed
//                                 diagonal tile.  Because D is closed (D (x) D = D, zero diagonal) the product with the tile
//                                 AS IT WAS equals the pivot-by-pivot recurrence on it, so both operands are snapshots in LDS
//                                 and the tile is written once;
//                              3. every other tile (I, J):  C = min(C, A (x) B), A = (I, b), B = (b, J).
//                            Phases 2 and 3 are one device function.  A 256-lane workgroup owns a 64 x 64 tile of C, lane
//                            (ty, tx) the rows 4 ty .. 4 ty + 3 and the columns {2 tx, 2 tx + 1, 32 + 2 tx, 33 + 2 tx}: per
//                            pivot 4 + 4 doubles from LDS feed 16 adds and 16 mins.  A sits row-major with a pitch of 66
//                            doubles (the 4 rows one wave reads at a time fall into different banks; the rest of the wave
//                            reads the same address), B row-major with pitch 64 (16 lanes x 16 bytes = one 256-byte line).
//                            Entries outside the matrix are +inf in LDS, so the edge tiles need no second code path, and
//                            are neither loaded from nor stored to G.
//   idiff_minplus_f64        C = min(C, A (x) B) for rectangular A [m, p], B [p, n]: the device function of phases 2 and 3 over every
//                            pivot tile of p, one workgroup per tile of C (the repair of a disconnected graph, isomap.py).
//   idiff_symmetrize_min_f64 G = min(G, G^T), the tile pass of knn_graph on its own.
//   idiff_double_center_f64  K = -1/2 J (D o D) J from the row means and the grand mean of D o D (D is symmetric, so the
//                            column means are the row means), and ||K||_F^2 from one partial sum per row: every sum is a
//                            fixed tree, the result does not depend on the launch.
//
// +inf is the only special value: the inputs hold no negative number and no NaN, so inf + x = inf and min() keeps an
// unreachable pair at +inf; the diagonal stays min(0, non-negative) = 0.
#include "common.h"

#include <math.h>

using namespace idiff;

namespace {

constexpr int T = 64;              // tile of the blocked Floyd-Warshall (idiff_apsp_tile)
constexpr int LDA = T + 2;         // LDS pitch of the A operand, doubles
constexpr int ST = 32;             // tile of the symmetrisation
constexpr int N_MAX = 1 << 20;     // the grids index tiles in 16 bits

__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// sum over the workgroup's 256 lanes, the same tree for every launch; red: 4 doubles of LDS
__device__ __forceinline__ double block_sum(double v, double *red) {
  v = wave_sum(v);
  __syncthreads();                                      // a previous use of red is over
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// ------------------------------------------------------------------------------------------------ graph
__global__ void __launch_bounds__(256) graph_fill_kernel(double *__restrict__ G, int N) {
  const int64_t total = (int64_t)N * N;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256)
    G[e] = (e / N == e % N) ? 0.0 : INFINITY;
}

__global__ void __launch_bounds__(256)
graph_edges_kernel(const double *__restrict__ dist, const int64_t *__restrict__ idx, int N, int k, double *__restrict__ G) {
  const int64_t total = (int64_t)N * k;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t i = e / k, j = idx[e];
    if (j >= 0 && j < N && j != i) G[i * N + j] = dist[e];      // an index outside the matrix is dropped, never an address
  }
}

// workgroup (bx <= by): the tiles (bx, by) and (by, bx), both read into LDS, both written with the minimum
__global__ void __launch_bounds__(256) graph_symmetrize_kernel(double *__restrict__ G, int N) {
  __shared__ double a[ST][ST + 1], b[ST][ST + 1];
  const int bx = blockIdx.x, by = blockIdx.y;
  if (bx > by) return;
  const int c = threadIdx.x & 31, r0 = threadIdx.x >> 5;
  for (int r = r0; r < ST; r += 8) {
    const int ia = bx * ST + r, ja = by * ST + c;         // tile (bx, by)
    const int ib = by * ST + r, jb = bx * ST + c;         // tile (by, bx)
    a[r][c] = (ia < N && ja < N) ? G[(int64_t)ia * N + ja] : INFINITY;
    b[r][c] = (ib < N && jb < N) ? G[(int64_t)ib * N + jb] : INFINITY;
  }
  __syncthreads();
  for (int r = r0; r < ST; r += 8) {
    const int ia = bx * ST + r, ja = by * ST + c;
    const int ib = by * ST + r, jb = bx * ST + c;
    if (ia < N && ja < N) G[(int64_t)ia * N + ja] = fmin(a[r][c], b[c][r]);
    if (bx != by && ib < N && jb < N) G[(int64_t)ib * N + jb] = fmin(b[r][c], a[c][r]);
  }
}

// ------------------------------------------------------------------------------------------------ shortest paths
// the tile (ti, tj) of the rows x cols matrix M (row pitch ldm) into LDS (row pitch `ld`), +inf outside the matrix
__device__ __forceinline__ void load_tile(const double *M, int rows, int cols, int64_t ldm, int ti, int tj, double *s, int ld) {
  for (int e = threadIdx.x; e < T * T; e += 256) {
    const int r = e >> 6, c = e & 63;
    const int i = ti * T + r, j = tj * T + c;
    s[r * ld + c] = (i < rows && j < cols) ? M[(int64_t)i * ldm + j] : INFINITY;
  }
}

// phase 1: the diagonal tile.  Each lane keeps its 16 entries in registers; per pivot it reads the pivot's column and row
// entries from LDS, and the tile is written back between two barriers (no lane reads what another is writing).
__global__ void __launch_bounds__(256) apsp_diag_kernel(double *__restrict__ G, int N, int b) {
  __shared__ double s[T * T];
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
  load_tile(G, N, N, N, b, b, s, T);
  __syncthreads();
  double acc[4][4];
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) acc[r][c] = s[(4 * ty + r) * T + 4 * tx + c];
  const int kmax = min(T, N - b * T);
  for (int k = 0; k < kmax; ++k) {
    double a[4], bb[4];
    for (int r = 0; r < 4; ++r) a[r] = s[(4 * ty + r) * T + k];
    for (int c = 0; c < 4; ++c) bb[c] = s[k * T + 4 * tx + c];
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) acc[r][c] = fmin(acc[r][c], a[r] + bb[c]);
    __syncthreads();                                    // every lane has read pivot k
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) s[(4 * ty + r) * T + 4 * tx + c] = acc[r][c];
    __syncthreads();
  }
  for (int r = 0; r < 4; ++r) {
    const int i = b * T + 4 * ty + r;
    for (int c = 0; c < 4; ++c) {
      const int j = b * T + 4 * tx + c;
      if (i < N && j < N) G[(int64_t)i * N + j] = acc[r][c];
    }
  }
}

// C (I, J) = min(C, A (I, kb) (x) B (kb, J)) over the pivot tiles kb0 <= kb < kb1, with C [m, n], A [m, p] and B [p, n] of row pitches
// ldc, lda, ldb; As: T x LDA doubles, Bs: T x T doubles.  The tile C may be one of the operands when there is one pivot tile (phase 2 of
// the Floyd-Warshall: A = B = C = G): both are complete in LDS before the first store.
__device__ __forceinline__ void minplus_tile(double *C, int64_t ldc, int m, int n, const double *A, int64_t lda, const double *B,
                                             int64_t ldb, int p, int I, int J, int kb0, int kb1, double *As, double *Bs) {
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
  const int i0 = I * T + 4 * ty, j0 = J * T + 2 * tx;
  double acc[4][4];
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) {
      const int i = i0 + r, j = j0 + (c & 1) + 32 * (c >> 1);
      acc[r][c] = (i < m && j < n) ? C[(int64_t)i * ldc + j] : INFINITY;
    }
  const double *ap = As + 4 * ty * LDA, *bp = Bs + 2 * tx;
  for (int kb = kb0; kb < kb1; ++kb) {
    if (kb > kb0) __syncthreads();                      // every lane is through with the previous pivot tile
    load_tile(A, m, p, lda, I, kb, As, LDA);
    load_tile(B, p, n, ldb, kb, J, Bs, T);
    __syncthreads();
    // two pivots per step, every LDS read 16 bytes wide (LDA and T are even, the bases 16-byte aligned); an odd pivot count
    // runs one pivot into the +inf padding, which changes nothing
    const int kmax = min(T, p - kb * T);
#pragma unroll 4
    for (int k = 0; k < kmax; k += 2) {
      double2 a[4], b0[2], b1[2];
      for (int r = 0; r < 4; ++r) a[r] = *reinterpret_cast<const double2 *>(ap + r * LDA + k);
      for (int h = 0; h < 2; ++h) {
        b0[h] = *reinterpret_cast<const double2 *>(bp + k * T + 32 * h);
        b1[h] = *reinterpret_cast<const double2 *>(bp + (k + 1) * T + 32 * h);
      }
      for (int r = 0; r < 4; ++r)
        for (int h = 0; h < 2; ++h) {
          acc[r][2 * h] = fmin(acc[r][2 * h], a[r].x + b0[h].x);
          acc[r][2 * h + 1] = fmin(acc[r][2 * h + 1], a[r].x + b0[h].y);
        }
      for (int r = 0; r < 4; ++r)
        for (int h = 0; h < 2; ++h) {
          acc[r][2 * h] = fmin(acc[r][2 * h], a[r].y + b1[h].x);
          acc[r][2 * h + 1] = fmin(acc[r][2 * h + 1], a[r].y + b1[h].y);
        }
    }
  }
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) {
      const int i = i0 + r, j = j0 + (c & 1) + 32 * (c >> 1);
      if (i < m && j < n) C[(int64_t)i * ldc + j] = acc[r][c];
    }
}

// phase 2: blockIdx.y = 0 the tile (b, x) of row b, 1 the tile (x, b) of column b
__global__ void __launch_bounds__(256) apsp_cross_kernel(double *G, int N, int b) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int x = blockIdx.x;
  if (x == b) return;
  if (blockIdx.y == 0) minplus_tile(G, N, N, N, G, N, G, N, N, b, x, b, b + 1, smem, smem + T * LDA);
  else minplus_tile(G, N, N, N, G, N, G, N, N, x, b, b, b + 1, smem, smem + T * LDA);
}

// phase 3: the tile (y, x), neither in row b nor in column b
__global__ void __launch_bounds__(256) apsp_rest_kernel(double *G, int N, int b) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int I = blockIdx.y, J = blockIdx.x;
  if (I == b || J == b) return;
  minplus_tile(G, N, N, N, G, N, G, N, N, I, J, b, b + 1, smem, smem + T * LDA);
}

// the rectangular product: the tile (y, x) of C over every pivot tile of p
__global__ void __launch_bounds__(256)
minplus_kernel(const double *__restrict__ A, int64_t lda, const double *__restrict__ B, int64_t ldb, double *__restrict__ C, int64_t ldc,
               int m, int n, int p) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  minplus_tile(C, ldc, m, n, A, lda, B, ldb, p, blockIdx.y, blockIdx.x, 0, (p + T - 1) / T, smem, smem + T * LDA);
}

// ------------------------------------------------------------------------------------------------ centring
// one workgroup per row: mean of the squares
__global__ void __launch_bounds__(256) center_rowmean_kernel(const double *__restrict__ D, int N, double *__restrict__ rowmean) {
  __shared__ double red[4];
  const int i = blockIdx.x;
  double acc = 0.0;
  for (int j = threadIdx.x; j < N; j += 256) {
    const double d = D[(int64_t)i * N + j];
    acc += d * d;
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) rowmean[i] = acc / N;
}

// one workgroup: out[0] = scale * sum of v[0 .. n)
__global__ void __launch_bounds__(256) center_reduce_kernel(const double *__restrict__ v, int n, double scale, double *__restrict__ out) {
  __shared__ double red[4];
  double acc = 0.0;
  for (int j = threadIdx.x; j < n; j += 256) acc += v[j];
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) out[0] = acc * scale;
}

// one workgroup per row: the row of K and the sum of its squares
__global__ void __launch_bounds__(256)
center_apply_kernel(const double *__restrict__ D, int N, const double *__restrict__ rowmean, const double *__restrict__ grand,
                    double *__restrict__ K, double *__restrict__ rowsq) {
  __shared__ double red[4];
  const int i = blockIdx.x;
  const double ri = rowmean[i], g = grand[0];
  double acc = 0.0;
  for (int j = threadIdx.x; j < N; j += 256) {
    const double d = D[(int64_t)i * N + j];
    const double v = -0.5 * (((d * d - ri) - rowmean[j]) + g);
    K[(int64_t)i * N + j] = v;
    acc += v * v;
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) rowsq[i] = acc;
}

}  // namespace

IDIFF_API int idiff_apsp_tile(void) { return T; }

IDIFF_API int idiff_knn_graph_f64(const double *dist, const int64_t *idx, int N, int k, double *G, void *stream) {
  if (N < 1) return fail("knn_graph: N = %d, need at least 1 point", N);
  if (N > N_MAX) return fail("knn_graph: N = %d above %d", N, N_MAX);
  if (k < 0) return fail("knn_graph: k = %d is negative", k);
  if (k > N - 1) return fail("knn_graph: k = %d but only N - 1 = %d other points", k, N - 1);
  if (!G || (k > 0 && (!dist || !idx))) return fail("knn_graph: null pointer");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(graph_fill_kernel, dim3(streaming_grid((int64_t)N * N, 256)), dim3(256), 0, st, G, N);
  if (k > 0)
    hipLaunchKernelGGL(graph_edges_kernel, dim3(streaming_grid((int64_t)N * k, 256)), dim3(256), 0, st, dist, idx, N, k, G);
  const int nt = ceil_div(N, ST);
  hipLaunchKernelGGL(graph_symmetrize_kernel, dim3(nt, nt), dim3(256), 0, st, G, N);
  return launch_status("knn_graph");
}

constexpr int APSP_LDS = (T * LDA + T * T) * (int)sizeof(double);   // 66,560 bytes: two workgroups per CU

// the three kernels that take APSP_LDS bytes of dynamic LDS, allowed it once per device
static int allow_tile_lds(const char *what) {
  static AttrGuard guard;
  const void *fns[3] = {reinterpret_cast<const void *>(apsp_cross_kernel), reinterpret_cast<const void *>(apsp_rest_kernel),
                        reinterpret_cast<const void *>(minplus_kernel)};
  return set_dynamic_lds_once(guard, fns, 3, APSP_LDS, what);
}

IDIFF_API int idiff_apsp_f64(double *G, int N, void *stream) {
  if (N < 1) return fail("apsp: N = %d, need at least 1 vertex", N);
  if (N > N_MAX) return fail("apsp: N = %d above %d", N, N_MAX);
  if (!G) return fail("apsp: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (int rc = allow_tile_lds("apsp")) return rc;
  const int nt = ceil_div(N, T);
  for (int b = 0; b < nt; ++b) {
    hipLaunchKernelGGL(apsp_diag_kernel, dim3(1), dim3(256), 0, st, G, N, b);
    hipLaunchKernelGGL(apsp_cross_kernel, dim3(nt, 2), dim3(256), APSP_LDS, st, G, N, b);
    hipLaunchKernelGGL(apsp_rest_kernel, dim3(nt, nt), dim3(256), APSP_LDS, st, G, N, b);
  }
  return launch_status("apsp");
}

static bool overlap(const double *a, int64_t na, const double *b, int64_t nb) { return a < b + nb && b < a + na; }

IDIFF_API int idiff_minplus_f64(const double *A, int64_t lda, const double *B, int64_t ldb, double *C, int64_t ldc, int m, int n, int p,
                                void *stream) {
  if (m < 1 || n < 1 || p < 1) return fail("minplus: m = %d, n = %d, p = %d, need at least 1 each", m, n, p);
  if (m > N_MAX || n > N_MAX || p > N_MAX) return fail("minplus: m = %d, n = %d, p = %d above %d", m, n, p, N_MAX);
  if (!A || !B || !C) return fail("minplus: null pointer");
  if (lda < p || ldb < n || ldc < n || lda > N_MAX || ldb > N_MAX || ldc > N_MAX)
    return fail("minplus: row pitches %lld, %lld, %lld for rows of %d, %d, %d entries", (long long)lda, (long long)ldb, (long long)ldc, p, n, n);
  const int64_t na = (int64_t)(m - 1) * lda + p, nb = (int64_t)(p - 1) * ldb + n, nc = (int64_t)(m - 1) * ldc + n;
  if (overlap(C, nc, A, na) || overlap(C, nc, B, nb)) return fail("minplus: C overlaps an operand");
  hipStream_t st = (hipStream_t)stream;
  if (int rc = allow_tile_lds("minplus")) return rc;
  hipLaunchKernelGGL(minplus_kernel, dim3(ceil_div(n, T), ceil_div(m, T)), dim3(256), APSP_LDS, st, A, lda, B, ldb, C, ldc, m, n, p);
  return launch_status("minplus");
}

IDIFF_API int idiff_symmetrize_min_f64(double *G, int N, void *stream) {
  if (N < 1) return fail("symmetrize_min: N = %d, need at least 1 vertex", N);
  if (N > N_MAX) return fail("symmetrize_min: N = %d above %d", N, N_MAX);
  if (!G) return fail("symmetrize_min: null pointer");
  const int nt = ceil_div(N, ST);
  hipLaunchKernelGGL(graph_symmetrize_kernel, dim3(nt, nt), dim3(256), 0, (hipStream_t)stream, G, N);
  return launch_status("symmetrize_min");
}

IDIFF_API int64_t idiff_double_center_scratch_doubles(int N) { return N < 1 || N > N_MAX ? 0 : 2 * (int64_t)N + 1; }

IDIFF_API int idiff_double_center_f64(const double *D, int N, double *K, double *fro2, double *scratch, void *stream) {
  if (N < 1) return fail("double_center: N = %d, need at least 1 point", N);
  if (N > N_MAX) return fail("double_center: N = %d above %d", N, N_MAX);
  if (!D || !K || !fro2 || !scratch) return fail("double_center: null pointer");
  hipStream_t st = (hipStream_t)stream;
  double *rowmean = scratch, *rowsq = scratch + N, *grand = scratch + 2 * (int64_t)N;
  hipLaunchKernelGGL(center_rowmean_kernel, dim3(N), dim3(256), 0, st, D, N, rowmean);
  hipLaunchKernelGGL(center_reduce_kernel, dim3(1), dim3(256), 0, st, rowmean, N, 1.0 / N, grand);
  hipLaunchKernelGGL(center_apply_kernel, dim3(N), dim3(256), 0, st, D, N, rowmean, grand, K, rowsq);
  hipLaunchKernelGGL(center_reduce_kernel, dim3(1), dim3(256), 0, st, rowsq, N, 1.0, fro2);
  return launch_status("double_center");
}
