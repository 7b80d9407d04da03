// The k LARGEST eigenpairs of a symmetric fp64 matrix K [N, N] that may be indefinite (the centred geodesic kernel of Isomap:
// its most negative eigenvalue is 0.7-19 % of the largest in magnitude on the fixtures), where lowvecs.hip serves the smallest ones of a positive semi-definite
// matrix.  Block subspace iteration with a Chebyshev filter on p = k + oversampling <= 128 columns:
//
//   X <- orth(X0)                               the fixed Philox block of lowvecs.hip
//   `sweeps` times:  X <- orth(C_m(K) X)        C_m the Chebyshev polynomial of degree m = `degree` mapped so that [lo, hi] =
//                                               [lambda_min, lambda_p+1] goes to [-1, 1] (where |C_m| <= 1) and scaled so that
//                                               C_m(top) = 1, top = lambda_1: the three-term recurrence
//                                                 Y_1 = (s_1 / e) (K - c) X,   Y_j+1 = (2 s_j+1 / e) (K - c) Y_j - s_j s_j+1 Y_j-1,
//                                                 c = (hi + lo) / 2, e = (hi - lo) / 2, s_1 = e / (top - c), s_j+1 = 1 / (2 / s_1 - s_j)
//                                               every step one launch of  Y <- alpha K X + beta X + gamma Z  on
//                                               v_mfma_f64_16x16x4_f64 (gemm_gt_kernel of orth_shared.h with the StoreAxpby
//                                               epilogue), K read once, Y written over Z
//   H = X^T K X = W diag(ritz) W^T              Rayleigh-Ritz on the p columns (cyclic Jacobi, one workgroup); the k largest taken
//   V = X W[:, top k],  resid = |K V - V diag(ritz)|_F   (K V evaluated afresh from the V that is returned)
//
// Interval, degree and sweeps come from the caller, who has the eigenvalues (python: _lib.topvecs_plan): the loops here have fixed
// bounds, there is no convergence test and the host never waits.  The interval starts at lambda_min, so a negative eigenvalue of
// large magnitude is damped like the rest of the unwanted spectrum (plain power iteration would converge to it).  The degree is
// the caller's to bound: C_m(top) / C_m(lambda_k) is how far column k falls below column 1 in one sweep, and what falls below
// 2^-53 of it is lost.
//
// orth is a shifted CholeskyQR3: the p x p Gram matrix on the matrix cores, its Cholesky factor and inverse in LDS (orth_shared.h),
// the first of the three passes with s = 11 (N p + p (p + 1)) 2^-53 trace(G) added to the diagonal, which keeps a block whose
// condition number is far beyond the 10^8 that plain CholeskyQR bears factorable (the plan lets the block's last column fall up to
// 10^10 below its first in a sweep); the two passes after it then bring |X^T X - I| to rounding.
//
// K is only read.  A NaN in K reaches every Gram matrix; it and a non-positive pivot poison V, ritz and resid with NaN -- never a
// silently wrong basis.
#include "common.h"
#include "philox.h"

#include <math.h>

namespace {
using namespace idiff;

#include "orth_shared.h"

constexpr int TOP_MAX = 64;        // most eigenpairs returned
constexpr int N_LIMIT = 1 << 20;
constexpr int DEGREE_MAX = 64;
constexpr int PRODUCTS_MAX = 4096; // degree * sweeps the call accepts (the plan of _lib.topvecs_plan stops at 1000)

__global__ void clear_ctl_kernel(double *__restrict__ ctl) {
  if (threadIdx.x < 8) ctl[threadIdx.x] = 0.0;
}

// the shift of the first CholeskyQR pass: coef * trace(sum of the partial Grams) onto the diagonal of the first partial
__global__ void __launch_bounds__(KMAX) gram_shift_kernel(double *__restrict__ P, int nch, int p, double coef) {
  __shared__ double red[KMAX];
  const int i = threadIdx.x;
  double d = 0.0;
  if (i < p)
    for (int ch = 0; ch < nch; ++ch) d += P[(int64_t)ch * p * p + i * p + i];
  red[i] = d;
  __syncthreads();
  for (int s = KMAX / 2; s > 0; s >>= 1) { if (i < s) red[i] += red[i + s]; __syncthreads(); }
  if (i < p) P[i * p + i] += coef * red[0];
}

// ritz = the k largest of the p eigenvalues jacobi_kernel left ascending in ritz_p, descending (apply_right_kernel takes the
// eigenvectors in the same order)
__global__ void top_ritz_kernel(const double *__restrict__ ritz_p, double *__restrict__ ritz, int p, int k) {
  if ((int)threadIdx.x < k) ritz[threadIdx.x] = ritz_p[p - 1 - threadIdx.x];
}

struct Layout { int64_t A, B, P, M, Wt, ritz_p, ctl, total; int nch; };
Layout layout(int N, int p) {
  Layout o;
  o.nch = ceil_div(N, CH);
  o.A = 0;
  o.B = o.A + (int64_t)N * p;
  o.P = o.B + (int64_t)N * p;
  o.M = o.P + (int64_t)o.nch * p * p;
  o.Wt = o.M + (int64_t)p * p;
  o.ritz_p = o.Wt + (int64_t)p * p;
  o.ctl = o.ritz_p + KMAX;
  o.total = o.ctl + 8;
  return o;
}

const char *refuse(int N, int k, int p) {
  static thread_local char msg[160];
  msg[0] = 0;
  if (k < 1 || k > TOP_MAX) snprintf(msg, sizeof(msg), "k must be in [1, %d] (got %d)", TOP_MAX, k);
  else if (N > N_LIMIT) snprintf(msg, sizeof(msg), "N = %d above %d", N, N_LIMIT);
  else if (k >= N) snprintf(msg, sizeof(msg), "k must be below N (got k = %d, N = %d)", k, N);
  else if (p < k || p > KMAX || p >= N) snprintf(msg, sizeof(msg), "block width p = %d outside [k, min(%d, N - 1)] (k = %d, N = %d)", p, KMAX, k, N);
  return msg[0] ? msg : nullptr;
}

}  // namespace

IDIFF_API int64_t idiff_sym_topvecs_scratch_doubles(int N, int k, int p) {
  if (refuse(N, k, p)) return 0;
  return layout(N, p).total;
}

IDIFF_API int idiff_sym_topvecs_f64(const double *K, int N, int k, int p, double lo, double hi, double top, int degree, int sweeps,
                                    double *V, double *ritz, double *resid, double *scratch, void *stream) {
  using namespace idiff;
  if (const char *why = refuse(N, k, p)) return fail("sym_topvecs: %s", why);
  if (!K || !V || !ritz || !resid || !scratch) return fail("sym_topvecs: null pointer");
  if (!(lo < hi && hi <= top) || !isfinite(lo) || !isfinite(top))
    return fail("sym_topvecs: the filter interval needs lo < hi <= top, all finite (got %g, %g, %g)", lo, hi, top);
  if (degree < 1 || degree > DEGREE_MAX || sweeps < 1 || (int64_t)degree * sweeps > PRODUCTS_MAX)
    return fail("sym_topvecs: degree %d (1..%d) x sweeps %d outside 1..%d matrix products", degree, DEGREE_MAX, sweeps, PRODUCTS_MAX);
  hipStream_t st = (hipStream_t)stream;
  const Layout o = layout(N, p);
  double *cur = scratch + o.A, *oth = scratch + o.B, *P = scratch + o.P, *M = scratch + o.M, *Wt = scratch + o.Wt,
         *ritz_p = scratch + o.ritz_p, *ctl = scratch + o.ctl;
  const size_t small_lds = ((size_t)p * (p + 1) + p) * sizeof(double);
  {
    static AttrGuard guard;
    const void *fns[2] = {reinterpret_cast<const void *>(chol_inv_kernel), reinterpret_cast<const void *>(jacobi_kernel)};
    if (int rc = set_dynamic_lds_once(guard, fns, 2, (int)(((size_t)KMAX * (KMAX + 1) + KMAX) * sizeof(double)), "sym_topvecs")) return rc;
  }
  const double shift = 11.0 * ((double)N * p + (double)p * (p + 1)) * 0x1p-53;
  auto orth = [&]() {                                 // shifted CholeskyQR3: cur -> oth -> cur -> oth, then the names are swapped
    for (int pass = 0; pass < 3; ++pass) {
      launch_xty(cur, cur, N, p, P, o.nch, st);
      if (pass == 0) hipLaunchKernelGGL(gram_shift_kernel, dim3(1), dim3(KMAX), 0, st, P, o.nch, p, shift);
      hipLaunchKernelGGL(chol_inv_kernel, dim3(1), dim3(256), small_lds, st, P, o.nch, p, M, ctl);
      hipLaunchKernelGGL(apply_right_kernel, dim3(ceil_div(N, AR_ROWS)), dim3(256), 0, st, cur, M, oth, N, p, p, 0, ctl, 0);
      double *t = cur; cur = oth; oth = t;
    }
  };

  hipLaunchKernelGGL(clear_ctl_kernel, dim3(1), dim3(64), 0, st, ctl);
  hipLaunchKernelGGL(init_x0_kernel, dim3(streaming_grid(ceil_div64((int64_t)N * p, 4), 256)), dim3(256), 0, st, cur, (int64_t)N * p);
  orth();
  const double c = 0.5 * (hi + lo), e = 0.5 * (hi - lo), s1 = e / (top - c);
  for (int sw = 0; sw < sweeps; ++sw) {
    double s = s1;
    launch_gemm_gt(K, cur, N, p, StoreAxpby{cur, nullptr, oth, s / e, -c * s / e, 0.0}, st);
    double *prev = cur, *now = oth;
    for (int j = 2; j <= degree; ++j) {
      const double sn = 1.0 / (2.0 / s1 - s);
      launch_gemm_gt(K, now, N, p, StoreAxpby{now, prev, prev, 2.0 * sn / e, -2.0 * sn * c / e, -s * sn}, st);
      double *t = prev; prev = now; now = t;
      s = sn;
    }
    cur = now; oth = prev;
    orth();
  }

  // ---- Rayleigh-Ritz on the p columns, the k largest pairs, and the residual of what is returned
  launch_gemm_gt(K, cur, N, p, oth, st);
  launch_xty(cur, oth, N, p, P, o.nch, st);
  hipLaunchKernelGGL(jacobi_kernel, dim3(1), dim3(256), small_lds, st, P, o.nch, p, Wt, M, ritz_p, ctl);
  hipLaunchKernelGGL(apply_right_kernel, dim3(ceil_div(N, AR_ROWS)), dim3(256), 0, st, cur, M, V, N, p, k, 1, ctl, 1);
  hipLaunchKernelGGL(top_ritz_kernel, dim3(1), dim3(64), 0, st, ritz_p, ritz, p, k);
  launch_gemm_gt(K, V, N, k, oth, st);
  hipLaunchKernelGGL(resid_kernel, dim3(1), dim3(256), 0, st, oth, V, ritz, N, k, resid, ctl);
  return launch_status("sym_topvecs");
}
