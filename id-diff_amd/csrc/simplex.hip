// Expected Simplex Skewness with d = 1 (Johnsson, Soneson and Fontes 2015; R intrinsicDimension::essLocalDimEst): for every query
// and every neighbourhood size k' of a list, the weighted mean of |sin| and of |cos| of the angle between all pairs of the
// mean-centred rows of the neighbourhood {centre, its k' nearest neighbours} of X [N, D] (fp32).  One workgroup per query,
// everything between the fp32 rows and the results in fp64, no intermediate in HBM.
//
//   1. gather   y_j = x_j - x_c in fp64 BEFORE any product, D streamed through LDS in chunks of DC columns, rows m .. mp - 1
//               (m = k + 1, mp = 16 ceil(m / 16)) zero -- as csrc/lpca.hip does
//   2. Gram     G = Y Y^T (mp x mp) on v_mfma_f64_16x16x4_f64: the upper 16 x 16 tiles dealt round-robin to the four waves,
//               accumulated over all chunks in registers, written once to LDS with their mirror images -- as csrc/lpca.hip does
//   3. tail     per scale s, m' = scales[s] + 1: the neighbours come in ascending distance, so the neighbourhood of size k' is the
//               leading m' x m' block of G.  Row means r_i and grand mean g of that block summed in a fixed order,
//               B_ij = G_ij - (r_i + r_j) + g  (= J G J, the Gram matrix of the rows centred on THEIR mean), never stored: the
//               clamped diagonal and its roots are kept, an off-diagonal entry is formed where its pair is summed
//   4. pairs    over i < j < m':  area = sum sqrt(max(0, B_ii B_jj - B_ij^2)),  dot = sum |B_ij|,  w = sum sqrt(B_ii) sqrt(B_jj);
//               element e = i m' + j of the block goes to thread e mod 256, which adds its elements in ascending e; the 256 partial
//               sums meet in a fixed tree.  ess_a = area / w, ess_b = dot / w: one division each.
//
// Steps 1-2 are restated here, not shared with lpca_kernel: a common device function would change what lpca.hip compiles to.
//
// What a (query, scale) produces depends on m' and on the rows alone: G_ij is accumulated in the same order whatever k is (the
// tile an entry belongs to and the chunk order are functions of i, j and D), the tail reads the leading block only, and the
// assignment of pairs to threads and the reduction tree depend on m' only.  No atomics.
//
// Index safety: every row index (centre and neighbours) is compared with [0, N) before any row of X is read; a query with an
// index outside gets status 2, NaN results, and reads nothing of X.
#include "common.h"

#include <math.h>

using namespace idiff;

namespace {

typedef double doublex4 __attribute__((ext_vector_type(4)));

constexpr int DC = 64;            // columns of X per chunk (lpca.hip's; _lib.LOCAL_PCA_CHUNK is the tests' handle on both)
constexpr int YP = DC + 2;        // LDS pitch of a gathered row, in doubles: 132 dwords = 4 (mod 64), so the 32 lanes of a
                                  // ds_read_b64 group (16 rows x 2 consecutive columns) hit 64 distinct banks
constexpr int K_MAX = 64;
constexpr int MP_MAX = 80;        // 16 ceil((K_MAX + 1) / 16)
constexpr int S_MAX = 16;
constexpr int MAX_OWN = 4;        // upper tiles per wave: ceil(15 / 4) at mp = 80

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

struct Args {
  const float *X;
  const int64_t *centre, *idx;
  double *ess;
  int *status;
  int N, D, k, S;
  int scales[S_MAX];
};

// LDS of one workgroup, in doubles from the start of the dynamic segment: the gathered chunk, the centre's chunk, G
__host__ __device__ inline int mp_of(int k) { return 16 * ((k + 1 + 15) / 16); }
__host__ __device__ inline int lds_doubles(int k) {
  const int mp = mp_of(k);
  return mp * YP + DC + mp * (mp + 1);
}

// rows j < m of the chunk [d0, d0 + DC): y_j = x_j - x_c in fp64, zero beyond D; rows m .. mp - 1 stay zero
__device__ __forceinline__ void gather_chunk(const Args &a, const int64_t *rows, int m, int d0, double *Y, double *xc) {
  const int tid = threadIdx.x;
  if (tid < DC) xc[tid] = d0 + tid < a.D ? (double)a.X[rows[0] * a.D + d0 + tid] : 0.0;
  __syncthreads();
  for (int e = tid; e < m * DC; e += 256) {
    const int j = e / DC, c = e % DC;
    Y[j * YP + c] = d0 + c < a.D ? (double)a.X[rows[j] * a.D + d0 + c] - xc[c] : 0.0;
  }
  __syncthreads();
}

__device__ __forceinline__ void refuse_query(const Args &a, int64_t q, int code) {
  for (int e = threadIdx.x; e < a.S * 3; e += 256) a.ess[q * a.S * 3 + e] = quiet_nan();
  if (threadIdx.x == 0) a.status[q] = code;
}

__global__ void __launch_bounds__(256) simplex_kernel(Args a) {
  extern __shared__ double lds[];
  __shared__ double red[3][256], rmean[MP_MAX], diag[MP_MAX], nrm[MP_MAX];
  __shared__ int64_t rows[MP_MAX];
  __shared__ int bad;
  const int tid = threadIdx.x, l = tid & 63, w = tid >> 6;
  const int64_t q = blockIdx.x;
  const int m = a.k + 1, mp = mp_of(a.k), ld = mp + 1, T = mp / 16;
  double *Y = lds, *xc = Y + mp * YP, *H = xc + DC;

  // ---- the row indices, checked before anything of X is read
  if (tid == 0) bad = 0;
  __syncthreads();
  if (tid < m) {
    const int64_t i = tid == 0 ? a.centre[q] : a.idx[q * a.k + tid - 1];
    if (i < 0 || i >= a.N) bad = 1;
    rows[tid] = i;
  }
  for (int e = tid; e < (mp - m) * YP; e += 256) Y[m * YP + e] = 0.0;      // the padding rows, once
  __syncthreads();
  if (bad) { refuse_query(a, q, 2); return; }

  // ---- Gram: wave w owns the upper tiles p = w, w + 4, ... of the T (T + 1) / 2
  int ta[MAX_OWN], tb[MAX_OWN];
  const int ntiles = T * (T + 1) / 2;
#pragma unroll
  for (int j = 0; j < MAX_OWN; ++j) {
    int p = w + 4 * j, ra = 0;
    if (p >= ntiles) p = 0;
    while (p >= T - ra) { p -= T - ra; ++ra; }
    ta[j] = ra; tb[j] = ra + p;
  }
  doublex4 acc[MAX_OWN] = {};
  for (int d0 = 0; d0 < a.D; d0 += DC) {
    gather_chunk(a, rows, m, d0, Y, xc);
#pragma unroll
    for (int j = 0; j < MAX_OWN; ++j) {
      if (w + 4 * j >= ntiles) continue;
      // lane l feeds row l & 15 of both operands at column (l >> 4) + 4 s of each block of 16 (the k order of the reduction is
      // free as long as both operands take the same one)
      const double *ya = Y + (16 * ta[j] + (l & 15)) * YP + (l >> 4), *yb = Y + (16 * tb[j] + (l & 15)) * YP + (l >> 4);
#pragma unroll
      for (int s = 0; s < DC / 4; ++s) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ya[4 * s], yb[4 * s], acc[j], 0, 0, 0);
    }
    __syncthreads();                                   // the next chunk overwrites Y
  }
#pragma unroll
  for (int j = 0; j < MAX_OWN; ++j) {
    if (w + 4 * j >= ntiles) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {                      // accumulator register r of lane l: C[(l >> 4) + 4 r][l & 15]
      const int row = 16 * ta[j] + (l >> 4) + 4 * r, col = 16 * tb[j] + (l & 15);
      H[row * ld + col] = acc[j][r];
      if (ta[j] != tb[j]) H[col * ld + row] = acc[j][r];
    }
  }
  __syncthreads();

  // ---- a NaN or Inf among the rows (or an overflow of |y_j|^2) shows on the diagonal of G: G_jj = sum_c y_jc^2
  if (tid < m) {
    const double d = H[tid * ld + tid];
    if (!(d - d == 0.0)) bad = 1;
  }
  __syncthreads();
  if (bad) { refuse_query(a, q, 3); return; }

  // ---- the tail, scale by scale on the leading mm x mm block of G
  int degenerate = 0;                                  // thread 0's
  for (int s = 0; s < a.S; ++s) {
    const int mm = a.scales[s] + 1;
    if (tid < mm) {
      double t = 0.0;
      for (int j = 0; j < mm; ++j) t += H[tid * ld + j];
      rmean[tid] = t / mm;
    }
    __syncthreads();
    double grand = 0.0;
    for (int j = 0; j < mm; ++j) grand += rmean[j];
    grand /= mm;
    if (tid < mm) {
      const double d = H[tid * ld + tid] - (rmean[tid] + rmean[tid]) + grand;
      diag[tid] = d > 0.0 ? d : 0.0;
      nrm[tid] = d > 0.0 ? sqrt(d) : 0.0;
    }
    __syncthreads();
    double area = 0.0, dot = 0.0, wsum = 0.0;
    for (int e = tid; e < mm * mm; e += 256) {
      const int i = e / mm, j = e % mm;
      if (i >= j) continue;
      const double b = H[i * ld + j] - (rmean[i] + rmean[j]) + grand;
      const double a2 = diag[i] * diag[j] - b * b;
      area += a2 > 0.0 ? sqrt(a2) : 0.0;
      dot += fabs(b);
      wsum += nrm[i] * nrm[j];
    }
    red[0][tid] = area; red[1][tid] = dot; red[2][tid] = wsum;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
      if (tid < h) { red[0][tid] += red[0][tid + h]; red[1][tid] += red[1][tid + h]; red[2][tid] += red[2][tid + h]; }
      __syncthreads();
    }
    if (tid == 0) {
      const double ws = red[2][0];
      double *out = a.ess + (q * a.S + s) * 3;
      if (ws == 0.0) degenerate = 1;                   // identical points: no angle to read
      out[0] = ws == 0.0 ? quiet_nan() : red[0][0] / ws;
      out[1] = ws == 0.0 ? quiet_nan() : red[1][0] / ws;
      out[2] = ws;
    }
    __syncthreads();                                   // the next scale overwrites rmean, diag, nrm and red
  }
  if (tid == 0) a.status[q] = degenerate ? 4 : 0;
}

const char *refusal(int N, int D, int k, int S) {
  static thread_local char buf[160];
  if (N < 1) { snprintf(buf, sizeof buf, "N = %d, need at least 1 row", N); return buf; }
  if (D < 1) { snprintf(buf, sizeof buf, "D = %d, need at least 1 dimension", D); return buf; }
  if (k < 2 || k > K_MAX) { snprintf(buf, sizeof buf, "k = %d outside 2..%d", k, K_MAX); return buf; }
  if (S < 1 || S > S_MAX) { snprintf(buf, sizeof buf, "S = %d scales outside 1..%d", S, S_MAX); return buf; }
  if ((int64_t)N * D > ((int64_t)1 << 40)) { snprintf(buf, sizeof buf, "N * D too large"); return buf; }
  return nullptr;
}

}  // namespace

IDIFF_API int idiff_simplex_skewness_ok(int N, int D, int k, int S) { return refusal(N, D, k, S) ? 0 : 1; }

IDIFF_API int idiff_simplex_skewness_f64(const float *X, int N, int D, const int64_t *centre, const int64_t *idx, int Q, int k,
                                         const int *scales, int S, double *ess, int *status, void *stream) {
  if (const char *why = refusal(N, D, k, S)) return fail("simplex_skewness: %s", why);
  if (Q < 0) return fail("simplex_skewness: Q = %d, need at least 0 queries", Q);
  if (!X || !centre || !idx || !scales || !ess || !status) return fail("simplex_skewness: null pointer");
  Args a{X, centre, idx, ess, status, N, D, k, S, {}};
  for (int s = 0; s < S; ++s) {
    if (scales[s] < 2 || scales[s] > k) return fail("simplex_skewness: scales[%d] = %d outside 2..k = %d", s, scales[s], k);
    if (s > 0 && scales[s] <= scales[s - 1])
      return fail("simplex_skewness: scales must ascend strictly, scales[%d] = %d after %d", s, scales[s], scales[s - 1]);
    a.scales[s] = scales[s];
  }
  if (Q == 0) return 0;
  static AttrGuard guard;
  const void *fn = reinterpret_cast<const void *>(simplex_kernel);
  if (int rc = set_dynamic_lds_once(guard, &fn, 1, lds_doubles(K_MAX) * 8, "simplex_skewness")) return rc;
  hipLaunchKernelGGL(simplex_kernel, dim3((unsigned)Q), dim3(256), lds_doubles(k) * 8, (hipStream_t)stream, a);
  return launch_status("simplex_skewness");
}
