// Local PCA (Fukunaga-Olsen in its original, per-point form): for every query the spectrum -- and, when asked, the leading
// eigenvectors -- of the sample covariance of a neighbourhood of m = k + 1 rows of X [N, D] (fp32): the centre row and its k
// neighbours.  One workgroup per query, everything between the fp32 rows and the results in fp64, no intermediate in HBM.
//
//   1. gather   y_j = x_j - x_c in fp64 BEFORE any product (the result does not depend on where the data sit relative to the
//               origin), D streamed through LDS in chunks of DC columns, rows m .. mp - 1 (mp = 16 ceil(m / 16)) zero
//   2. Gram     G = Y Y^T (mp x mp) on v_mfma_f64_16x16x4_f64: the upper 16 x 16 tiles dealt round-robin to the four waves,
//               accumulated over all chunks in registers, written once to LDS with their mirror images
//   3. centre   B = J G J / (m - 1), J = I - 1 1^T / m, as (G_ij - (r_i + r_j) + g) / (m - 1) with the row means r and the grand
//               mean g summed in a fixed order.  B's non-zero eigenvalues are those of the neighbourhood's sample covariance;
//               the D x D covariance is never formed (m <= 65 keeps B in LDS at any D)
//   4. Jacobi   cyclic, with the round-robin ordering of orth_shared.h's jacobi_kernel (n / 2 disjoint rotations per round,
//               n - 1 rounds per sweep), B and -- only when vectors are asked for -- the accumulated rotations W in LDS; stops
//               when the off-diagonal norm is at most m 2^-52 ||B||_F, or after SWEEP_CAP sweeps (status 1); a B that is not
//               finite (NaN or Inf among the rows, or an overflow) is status 3, its results NaN or Inf as they fall
//   5. vectors  row v = Y^T J u_v / sqrt((m - 1) lambda_v): a second pass over the gathered rows, NaN where lambda_v <= m 2^-52
//               lambda_1 (never guessed), then the sign that makes the component of largest magnitude positive
//
// The rotation code is restated here, not shared with jacobi_kernel: that kernel sums partial Grams from HBM, keeps W in HBM,
// stops on another rule and sorts ascending into a matrix for X <- X M; a common device function would change what lowvecs.hip
// and topvecs.hip compile to.
//
// Index safety: every row index (centre and neighbours) is compared with [0, N) before any row of X is read; a query with an
// index outside gets status 2, NaN results, and reads nothing of X.
#include "common.h"

#include <math.h>

using namespace idiff;

namespace {

typedef double doublex4 __attribute__((ext_vector_type(4)));

constexpr int DC = 64;            // columns of X per chunk
constexpr int YP = DC + 2;        // LDS pitch of a gathered row, in doubles: 132 dwords = 4 (mod 64), so the 32 lanes of a
                                  // ds_read_b64 group (16 rows x 2 consecutive columns) hit 64 distinct banks
constexpr int K_MAX = 64;
constexpr int MP_MAX = 80;        // 16 ceil((K_MAX + 1) / 16)
constexpr int SWEEP_CAP = 30;
constexpr int MAX_OWN = 4;        // upper tiles per wave: ceil(15 / 4) at mp = 80
constexpr double EPS52 = 2.220446049250313e-16;   // 2^-52

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

struct Args {
  const float *X;
  const int64_t *centre, *idx;
  double *eig, *basis;
  int *status;
  int N, D, k, n_vec, r;
};

// LDS of one workgroup, in doubles from the start of the dynamic segment
__host__ __device__ inline int mp_of(int k) { return 16 * ((k + 1 + 15) / 16); }
__host__ __device__ inline int lds_doubles(int k, int n_vec) {
  const int mp = mp_of(k);
  return mp * YP + DC + mp * (mp + 1) * (n_vec > 0 ? 2 : 1);
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

__global__ void __launch_bounds__(256) lpca_kernel(Args a) {
  extern __shared__ double lds[];
  __shared__ double red[256], rc[MP_MAX / 2 + 1], rs[MP_MAX / 2 + 1], lam[MP_MAX], rmean[MP_MAX], best_abs[K_MAX];
  __shared__ int64_t rows[MP_MAX];
  __shared__ int rp[MP_MAX / 2 + 1], rq[MP_MAX / 2 + 1], perm[MP_MAX], best_neg[K_MAX], bad, converged;
  const int tid = threadIdx.x, l = tid & 63, w = tid >> 6;
  const int64_t q = blockIdx.x;
  const int m = a.k + 1, mp = mp_of(a.k), ld = mp + 1, T = mp / 16;
  double *Y = lds, *xc = Y + mp * YP, *H = xc + DC, *W = a.n_vec > 0 ? H + mp * ld : nullptr;

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
  if (bad) {
    for (int e = tid; e < a.r; e += 256) a.eig[q * a.r + e] = quiet_nan();
    for (int64_t e = tid; e < (int64_t)a.n_vec * a.D; e += 256) a.basis[q * a.n_vec * a.D + e] = quiet_nan();
    if (tid == 0) a.status[q] = 2;
    return;
  }

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

  // ---- double centring, in place
  if (tid < m) {
    double s = 0.0;
    for (int j = 0; j < m; ++j) s += H[tid * ld + j];
    rmean[tid] = s / m;
  }
  __syncthreads();
  double grand = 0.0;
  for (int j = 0; j < m; ++j) grand += rmean[j];
  grand /= m;
  for (int e = tid; e < m * m; e += 256) {
    const int i = e / m, j = e % m;
    H[i * ld + j] = (H[i * ld + j] - (rmean[i] + rmean[j]) + grand) / (m - 1);
    if (W) W[i * ld + j] = i == j ? 1.0 : 0.0;
  }
  if (tid == 0) converged = 0;
  __syncthreads();

  // ---- cyclic Jacobi
  const int n = m + (m & 1), npairs = n / 2;
  double tot = 0.0;
  for (int sweep = 0; sweep <= SWEEP_CAP; ++sweep) {
    double all = 0.0, off = 0.0;
    for (int e = tid; e < m * m; e += 256) {
      const double v = H[(e / m) * ld + e % m];
      all += v * v;
      if (e / m != e % m) off += v * v;
    }
    if (sweep == 0) {
      red[tid] = all;
      __syncthreads();
      for (int s = 128; s > 0; s >>= 1) { if (tid < s) red[tid] += red[tid + s]; __syncthreads(); }
      tot = red[0];
      __syncthreads();
    }
    red[tid] = off;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) { if (tid < s) red[tid] += red[tid + s]; __syncthreads(); }
    off = red[0];
    __syncthreads();
    const double thr = (double)m * EPS52;
    if (!(off > thr * thr * tot)) {                    // converged -- or not finite (a NaN or Inf in the rows): no further sweep
      if (tid == 0) converged = tot - tot == 0.0 ? 1 : 2;
      break;
    }
    if (sweep == SWEEP_CAP) break;
    for (int r = 0; r < n - 1; ++r) {
      if (tid < npairs) {
        const int ia = tid == 0 ? n - 1 : (r + tid) % (n - 1), ib = tid == 0 ? r : (r - tid + n - 1) % (n - 1);
        const int p = ia < ib ? ia : ib, qq = ia < ib ? ib : ia;
        double c = 1.0, s = 0.0;
        const double hpq = qq < m ? H[p * ld + qq] : 0.0;
        if (hpq != 0.0) {
          const double th = (H[qq * ld + qq] - H[p * ld + p]) / (2.0 * hpq);
          const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
          c = 1.0 / sqrt(t * t + 1.0);
          s = t * c;
        }
        rp[tid] = (qq < m && s != 0.0) ? p : -1; rq[tid] = qq; rc[tid] = c; rs[tid] = s;
      }
      __syncthreads();
      for (int e = tid; e < npairs * m; e += 256) {    // H <- H J, W <- W J: columns p, q of every row
        const int pi = e / m, row = e % m, p = rp[pi], qq = rq[pi];
        if (p < 0) continue;
        const double c = rc[pi], s = rs[pi];
        const double hp = H[row * ld + p], hq = H[row * ld + qq];
        H[row * ld + p] = c * hp - s * hq; H[row * ld + qq] = s * hp + c * hq;
        if (W) {
          const double wp = W[row * ld + p], wq = W[row * ld + qq];
          W[row * ld + p] = c * wp - s * wq; W[row * ld + qq] = s * wp + c * wq;
        }
      }
      __syncthreads();
      for (int e = tid; e < npairs * m; e += 256) {    // H <- J^T H: rows p, q of every column; the rotated pair itself is exactly 0
        const int pi = e / m, col = e % m, p = rp[pi], qq = rq[pi];
        if (p < 0) continue;
        const double c = rc[pi], s = rs[pi];
        const double hp = H[p * ld + col], hq = H[qq * ld + col];
        H[p * ld + col] = col == qq ? 0.0 : c * hp - s * hq;
        H[qq * ld + col] = col == p ? 0.0 : s * hp + c * hq;
      }
      __syncthreads();
    }
  }
  __syncthreads();

  // ---- eigenvalues, descending (equal values by lower index), clamped at 0
  if (tid < m) lam[tid] = H[tid * ld + tid];
  __syncthreads();
  if (tid < m) {
    int rk = 0;
    for (int j = 0; j < m; ++j) rk += (lam[j] > lam[tid]) || (!(lam[tid] > lam[j]) && j < tid);
    if (rk > m - 1) rk = m - 1;
    perm[rk] = tid;
    if (rk < a.r) a.eig[q * a.r + rk] = lam[tid] > 0.0 ? lam[tid] : (lam[tid] == lam[tid] ? 0.0 : lam[tid]);
  }
  if (tid == 0) a.status[q] = converged == 1 ? 0 : converged == 2 ? 3 : 1;
  if (a.n_vec == 0) return;
  __syncthreads();

  // ---- vectors: the coefficients C[j][v] = (J u_v)_j / sqrt((m - 1) lambda_v) over the finished B (every thread has read its lam)
  double *C = H;
  const double lam1 = lam[perm[0]];
  __syncthreads();
  if (tid < a.n_vec) {
    const int col = perm[tid];
    const double lv = lam[col];
    const bool ok = lam1 > 0.0 && lv > (double)m * EPS52 * lam1;
    double mean = 0.0;
    for (int j = 0; j < m; ++j) mean += W[j * ld + col];
    mean /= m;
    const double scale = ok ? 1.0 / sqrt((double)(m - 1) * lv) : quiet_nan();
    for (int j = 0; j < m; ++j) C[j * a.n_vec + tid] = (W[j * ld + col] - mean) * scale;
    best_abs[tid] = -1.0; best_neg[tid] = 0;
  }
  __syncthreads();
  double *out = a.basis + q * a.n_vec * a.D;
  for (int d0 = 0; d0 < a.D; d0 += DC) {
    gather_chunk(a, rows, m, d0, Y, xc);
    for (int v = w; v < a.n_vec; v += 4) {             // wave w: vectors w, w + 4, ...; lane = column of the chunk
      double s = 0.0;
      for (int j = 0; j < m; ++j) s += C[j * a.n_vec + v] * Y[j * YP + l];
      const int d = d0 + l;
      if (d < a.D) out[(int64_t)v * a.D + d] = s;
      // the component of largest magnitude, lowest index on ties: over the lanes, then against the chunks before
      double ba = d < a.D ? fabs(s) : -1.0;
      int bi = d, bn = s < 0.0;
      for (int o = 32; o > 0; o >>= 1) {
        const double oa = __shfl_xor(ba, o);
        const int oi = __shfl_xor(bi, o), on = __shfl_xor(bn, o);
        if (oa > ba || (oa == ba && oi < bi)) { ba = oa; bi = oi; bn = on; }
      }
      if (l == 0 && ba > best_abs[v]) { best_abs[v] = ba; best_neg[v] = bn; }      // a later chunk wins only if strictly larger
    }
    __syncthreads();
  }
  __threadfence();
  __syncthreads();
  for (int v = 0; v < a.n_vec; ++v) {
    if (!best_neg[v]) continue;
    for (int d = tid; d < a.D; d += 256) out[(int64_t)v * a.D + d] = -out[(int64_t)v * a.D + d];
  }
}

const char *refusal(int N, int D, int k, int n_vec) {
  static thread_local char buf[160];
  if (N < 1) { snprintf(buf, sizeof buf, "N = %d, need at least 1 row", N); return buf; }
  if (D < 1) { snprintf(buf, sizeof buf, "D = %d, need at least 1 dimension", D); return buf; }
  if (k < 2 || k > K_MAX) { snprintf(buf, sizeof buf, "k = %d outside 2..%d", k, K_MAX); return buf; }
  const int r = k < D ? k : D;
  if (n_vec < 0 || n_vec > r) { snprintf(buf, sizeof buf, "n_vec = %d outside 0..min(k, D) = %d", n_vec, r); return buf; }
  if ((int64_t)N * D > ((int64_t)1 << 40)) { snprintf(buf, sizeof buf, "N * D too large"); return buf; }
  return nullptr;
}

}  // namespace

IDIFF_API int idiff_local_pca_ok(int N, int D, int k, int n_vec) { return refusal(N, D, k, n_vec) ? 0 : 1; }

IDIFF_API int idiff_local_pca_chunk(void) { return DC; }

IDIFF_API int idiff_local_pca_f64(const float *X, int N, int D, const int64_t *centre, const int64_t *idx, int Q, int k, int n_vec,
                                  double *eig, double *basis, int *status, void *stream) {
  if (const char *why = refusal(N, D, k, n_vec)) return fail("local_pca: %s", why);
  if (Q < 0) return fail("local_pca: Q = %d, need at least 0 queries", Q);
  if (!X || !centre || !idx || !eig || !status || (n_vec > 0 && !basis)) return fail("local_pca: null pointer");
  if (Q == 0) return 0;
  Args a{X, centre, idx, eig, basis, status, N, D, k, n_vec, k < D ? k : D};
  static AttrGuard guard;
  const void *fn = reinterpret_cast<const void *>(lpca_kernel);
  if (int rc = set_dynamic_lds_once(guard, &fn, 1, lds_doubles(K_MAX, 1) * 8, "local_pca")) return rc;
  hipLaunchKernelGGL(lpca_kernel, dim3((unsigned)Q), dim3(256), lds_doubles(k, n_vec) * 8, (hipStream_t)stream, a);
  return launch_status("local_pca");
}
