// Invariant subspace of the k smallest eigenvalues of a symmetric positive semi-definite fp64 matrix G [D, D] (the centred
// Gram matrix of the score vectors): the estimated tangent space of the data manifold at the point, where the spectrum
// path (spectrum.hip / sbr.hip) yields the eigenvalues alone.  The reference keeps `v` of torch.linalg.svd for this
// (dim_reduction.py:197); here k is the intrinsic dimension, 10-100 of 1024-12288, so only that side is computed:
//
//   L L^T = G + eps I                         blocked right-looking Cholesky, panels of 32, trailing update on
//                                             v_mfma_f64_16x16x4_f64 (lower tiles only); eps = 8 D 2^-53 max_i G_ii keeps a
//                                             rank-deficient G factorable and moves no eigenvector
//   X <- orth(L^-T L^-1 X), 4 times           inverse subspace iteration from a fixed Philox block X0: the eigenvalue gap at k
//                                             is what the ID rule detects, so the contraction per step is lambda_k / lambda_k+1;
//                                             orth = CholeskyQR2 (k x k Gram on the matrix cores, Cholesky + inverse in LDS)
//   H = X^T G X,  H = W diag(ritz) W^T        Rayleigh-Ritz: cyclic Jacobi in one workgroup, H in LDS
//   T = X W,  resid = |G T - T diag(ritz)|_F  (G T evaluated afresh from the T that is returned)
//
// G is only read: the factor lives in the scratch.  A non-positive pivot (of G + eps I or of a k x k Gram) and a NaN in G
// poison T, ritz and resid with NaN -- never a silently wrong basis.  Every loop has a fixed bound: nothing can hang.
// All launches go to the caller's stream; the host never waits.
#include "common.h"
#include "philox.h"

namespace {
using namespace idiff;

#include "orth_shared.h"

constexpr int NB = 32;         // Cholesky panel width = row block of the triangular solves
constexpr int STRIP = 64;      // rows one workgroup of a triangular-solve step updates
constexpr int ITERS = 4;

// ctl[0] = eps (the diagonal shift), ctl[1] = 0, or NaN once any stage has failed (added to every output at the end)
__global__ void __launch_bounds__(256) prepare_kernel(const double *__restrict__ G, int D, double *__restrict__ ctl) {
  __shared__ double red[256];
  __shared__ int bad[256];
  double m = 0.0;
  int b = 0;
  for (int i = threadIdx.x; i < D; i += 256) {
    const double v = G[(int64_t)i * D + i];
    b |= !(v == v);
    m = v > m ? v : m;
  }
  red[threadIdx.x] = m; bad[threadIdx.x] = b;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      red[threadIdx.x] = red[threadIdx.x + s] > red[threadIdx.x] ? red[threadIdx.x + s] : red[threadIdx.x];
      bad[threadIdx.x] |= bad[threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    ctl[0] = bad[0] ? quiet_nan() : 8.0 * (double)D * 0x1p-53 * red[0];
    ctl[1] = 0.0;
  }
}

// L = tril(G) + eps I (the strict upper triangle of L is zero and stays zero)
__global__ void __launch_bounds__(256) copy_lower_kernel(const double *__restrict__ G, double *__restrict__ L, int D,
                                                         const double *__restrict__ ctl) {
  const double eps = ctl[0];
  const int64_t n = (int64_t)D * D;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    const int64_t r = e / D, c = e - r * D;
    L[e] = c < r ? G[e] : (c == r ? G[e] + eps : 0.0);
  }
}

__global__ void __launch_bounds__(256) potrf_diag_kernel(double *__restrict__ L, int D, int j0, int nb, double *__restrict__ ctl) {
  __shared__ double A[NB * (NB + 1)];
  for (int e = threadIdx.x; e < nb * nb; e += 256) {
    const int r = e / nb, c = e % nb;
    A[r * (NB + 1) + c] = L[(int64_t)(j0 + r) * D + j0 + c];
  }
  chol_lds(A, NB + 1, nb, ctl);
  for (int e = threadIdx.x; e < nb * nb; e += 256) {
    const int r = e / nb, c = e % nb;
    if (c <= r) L[(int64_t)(j0 + r) * D + j0 + c] = A[r * (NB + 1) + c];
  }
}

// L21 = A21 L11^-T for the rows below a full panel: one row per lane, in registers; L11 is read from LDS by all lanes alike
__global__ void __launch_bounds__(256) trsm_panel_kernel(double *__restrict__ L, int D, int j0) {
  __shared__ double A[NB * (NB + 1)];
  for (int e = threadIdx.x; e < NB * NB; e += 256) A[(e / NB) * (NB + 1) + e % NB] = L[(int64_t)(j0 + e / NB) * D + j0 + e % NB];
  __syncthreads();
  const int64_t i = (int64_t)j0 + NB + (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= D) return;
  double *row = L + i * D + j0;
  double x[NB];
#pragma unroll
  for (int c = 0; c < NB; ++c) x[c] = row[c];
#pragma unroll
  for (int c = 0; c < NB; ++c) {
    double s = x[c];
#pragma unroll
    for (int m = 0; m < c; ++m) s -= x[m] * A[c * (NB + 1) + m];
    x[c] = s / A[c * (NB + 1) + c];
  }
#pragma unroll
  for (int c = 0; c < NB; ++c) row[c] = x[c];
}

// A22 -= L21 L21^T on the matrix cores, tiles of 64 x 64 on and below the diagonal; wave w owns the 32 x 32 quadrant
// (w >> 1, w & 1) as 2 x 2 instruction tiles.  Only entries with column <= row are stored.
__global__ void __launch_bounds__(256) syrk_kernel(double *__restrict__ L, int D, int j0) {
  if (blockIdx.y > blockIdx.x) return;
  const int base = j0 + NB, w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int r0 = base + 64 * (int)blockIdx.x + 32 * (w >> 1), c0 = base + 64 * (int)blockIdx.y + 32 * (w & 1);
  if (r0 >= D || c0 >= D || c0 > r0 + 31) return;
  const double *pa[2], *pb[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int ra = r0 + 16 * q + (l & 15), rb = c0 + 16 * q + (l & 15);
    pa[q] = L + (int64_t)(ra < D ? ra : D - 1) * D + j0 + 4 * (l >> 4);
    pb[q] = L + (int64_t)(rb < D ? rb : D - 1) * D + j0 + 4 * (l >> 4);
  }
  doublex4 acc[2][2] = {};
#pragma unroll
  for (int kk = 0; kk < NB; kk += 16)
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      double a[2], b[2];
#pragma unroll
      for (int q = 0; q < 2; ++q) { a[q] = pa[q][kk + s]; b[q] = pb[q][kk + s]; }
#pragma unroll
      for (int qa = 0; qa < 2; ++qa)
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) acc[qa][qb] = mfma(a[qa], b[qb], acc[qa][qb]);
    }
#pragma unroll
  for (int qa = 0; qa < 2; ++qa)
#pragma unroll
    for (int qb = 0; qb < 2; ++qb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = r0 + 16 * qa + (l >> 4) + 4 * r, col = c0 + 16 * qb + (l & 15);
        if (row < D && col <= row) L[(int64_t)row * D + col] -= acc[qa][qb][r];
      }
}

// One block step of L Y = X (FWD) or L^T Y = X (backward) with k right-hand sides.  Every workgroup solves the diagonal
// block [b0, b0 + nb) itself, in LDS (a few thousand multiply-adds); workgroup 0 writes those rows of Y; workgroup g
// subtracts the block's contribution from its strip of the rows of X that are still to come (below the block going
// forward, above it going backward).  Y is another buffer than X: no workgroup reads what another one writes.
template <bool FWD>
__global__ void __launch_bounds__(256) tri_solve_kernel(const double *__restrict__ L, int D, int k, double *__restrict__ X,
                                                        double *__restrict__ Y, int b0, int nb) {
  __shared__ double Lbb[NB * (NB + 1)];
  __shared__ double Yb[NB * KMAX];
  __shared__ double strip[STRIP * (NB + 1)];
  for (int e = threadIdx.x; e < nb * nb; e += 256) Lbb[(e / nb) * (NB + 1) + e % nb] = L[(int64_t)(b0 + e / nb) * D + b0 + e % nb];
  for (int e = threadIdx.x; e < nb * k; e += 256) Yb[(e / k) * KMAX + e % k] = X[(int64_t)b0 * k + e];
  const int i0 = FWD ? b0 + nb + STRIP * (int)blockIdx.x : STRIP * (int)blockIdx.x;
  const int iend = FWD ? D : b0;
  const int nr = iend - i0 < STRIP ? iend - i0 : STRIP;        // <= 0: this workgroup has no strip (the last block's only one)
  if (FWD) {
    for (int e = threadIdx.x; e < nr * nb; e += 256) strip[(e / nb) * (NB + 1) + e % nb] = L[(int64_t)(i0 + e / nb) * D + b0 + e % nb];
  } else {
    for (int e = threadIdx.x; e < nr * nb; e += 256) strip[(e % nr) * (NB + 1) + e / nr] = L[(int64_t)(b0 + e / nr) * D + i0 + e % nr];
  }
  __syncthreads();
  const int c = threadIdx.x;
  if (c < k) {
    if (FWD) {
      for (int r = 0; r < nb; ++r) {
        double s = Yb[r * KMAX + c];
        for (int m = 0; m < r; ++m) s -= Lbb[r * (NB + 1) + m] * Yb[m * KMAX + c];
        Yb[r * KMAX + c] = s / Lbb[r * (NB + 1) + r];
      }
    } else {
      for (int r = nb - 1; r >= 0; --r) {
        double s = Yb[r * KMAX + c];
        for (int m = r + 1; m < nb; ++m) s -= Lbb[m * (NB + 1) + r] * Yb[m * KMAX + c];
        Yb[r * KMAX + c] = s / Lbb[r * (NB + 1) + r];
      }
    }
  }
  __syncthreads();
  if (blockIdx.x == 0)
    for (int e = threadIdx.x; e < nb * k; e += 256) Y[(int64_t)b0 * k + e] = Yb[(e / k) * KMAX + e % k];
  for (int e = threadIdx.x; e < nr * k; e += 256) {
    const int r = e / k, cc = e % k;
    double s = 0.0;
    for (int m = 0; m < nb; ++m) s += strip[r * (NB + 1) + m] * Yb[m * KMAX + cc];
    X[(int64_t)(i0 + r) * k + cc] -= s;
  }
}

struct Layout { int64_t L, X, Y, P, M, Wt, ctl, total; int nch; };
Layout layout(int D, int k) {
  Layout o;
  o.nch = ceil_div(D, CH);
  o.L = 0;
  o.X = o.L + (int64_t)D * D;
  o.Y = o.X + (int64_t)D * k;
  o.P = o.Y + (int64_t)D * k;
  o.M = o.P + (int64_t)o.nch * k * k;
  o.Wt = o.M + (int64_t)k * k;
  o.ctl = o.Wt + (int64_t)k * k;
  o.total = o.ctl + 8;
  return o;
}

}  // namespace

IDIFF_API int64_t idiff_sym_lowvecs_scratch_doubles(int D, int k) {
  if (k < 1 || k > KMAX || k >= D) return 0;
  return layout(D, k).total;
}

IDIFF_API int idiff_sym_lowvecs_f64(double *G, int D, int k, double *T, double *ritz, double *resid, double *scratch, void *stream) {
  using namespace idiff;
  if (k < 1 || k > KMAX) return fail("sym_lowvecs: k must be in [1, %d] (got %d)", KMAX, k);
  if (k >= D) return fail("sym_lowvecs: k must be below D (got k = %d, D = %d)", k, D);
  if (!G || !T || !ritz || !resid || !scratch) return fail("sym_lowvecs: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const Layout o = layout(D, k);
  double *L = scratch + o.L, *X = scratch + o.X, *Y = scratch + o.Y, *P = scratch + o.P, *M = scratch + o.M, *Wt = scratch + o.Wt,
         *ctl = scratch + o.ctl;
  const size_t small_lds = ((size_t)k * (k + 1) + k) * sizeof(double);
  {
    static AttrGuard guard;
    const void *fns[2] = {reinterpret_cast<const void *>(chol_inv_kernel), reinterpret_cast<const void *>(jacobi_kernel)};
    if (int rc = set_dynamic_lds_once(guard, fns, 2, (int)(((size_t)KMAX * (KMAX + 1) + KMAX) * sizeof(double)), "sym_lowvecs")) return rc;
  }

  // ---- L L^T = G + eps I
  hipLaunchKernelGGL(prepare_kernel, dim3(1), dim3(256), 0, st, G, D, ctl);
  hipLaunchKernelGGL(copy_lower_kernel, dim3(streaming_grid((int64_t)D * D, 256)), dim3(256), 0, st, G, L, D, ctl);
  for (int j0 = 0; j0 < D; j0 += NB) {
    const int nb = D - j0 < NB ? D - j0 : NB;
    hipLaunchKernelGGL(potrf_diag_kernel, dim3(1), dim3(256), 0, st, L, D, j0, nb, ctl);
    const int below = D - j0 - NB;
    if (below <= 0) break;
    hipLaunchKernelGGL(trsm_panel_kernel, dim3(ceil_div(below, 256)), dim3(256), 0, st, L, D, j0);
    const int nt = ceil_div(below, 64);
    hipLaunchKernelGGL(syrk_kernel, dim3(nt, nt), dim3(256), 0, st, L, D, j0);
  }

  // ---- inverse subspace iteration
  hipLaunchKernelGGL(init_x0_kernel, dim3(streaming_grid(ceil_div64((int64_t)D * k, 4), 256)), dim3(256), 0, st, X, (int64_t)D * k);
  const int nblk = ceil_div(D, NB);
  for (int it = 0; it < ITERS; ++it) {
    for (int b = 0; b < nblk; ++b) {              // L Y = X
      const int b0 = b * NB, nb = D - b0 < NB ? D - b0 : NB, rest = D - b0 - nb;
      hipLaunchKernelGGL(tri_solve_kernel<true>, dim3(rest > 0 ? ceil_div(rest, STRIP) : 1), dim3(256), 0, st, L, D, k, X, Y, b0, nb);
    }
    for (int b = nblk - 1; b >= 0; --b) {         // L^T X = Y
      const int b0 = b * NB, nb = D - b0 < NB ? D - b0 : NB;
      hipLaunchKernelGGL(tri_solve_kernel<false>, dim3(b0 > 0 ? ceil_div(b0, STRIP) : 1), dim3(256), 0, st, L, D, k, Y, X, b0, nb);
    }
    for (int pass = 0; pass < 2; ++pass) {        // CholeskyQR2: X -> Y -> X
      double *src = pass == 0 ? X : Y, *dst = pass == 0 ? Y : X;
      launch_xty(src, src, D, k, P, o.nch, st);
      hipLaunchKernelGGL(chol_inv_kernel, dim3(1), dim3(256), small_lds, st, P, o.nch, k, M, ctl);
      hipLaunchKernelGGL(apply_right_kernel, dim3(ceil_div(D, AR_ROWS)), dim3(256), 0, st, src, M, dst, D, k, k, 0, ctl, 0);
    }
  }

  // ---- Rayleigh-Ritz and the residual of what is returned
  launch_gemm_gt(G, X, D, k, Y, st);
  launch_xty(X, Y, D, k, P, o.nch, st);
  hipLaunchKernelGGL(jacobi_kernel, dim3(1), dim3(256), small_lds, st, P, o.nch, k, Wt, M, ritz, ctl);
  hipLaunchKernelGGL(apply_right_kernel, dim3(ceil_div(D, AR_ROWS)), dim3(256), 0, st, X, M, T, D, k, k, 0, ctl, 1);
  launch_gemm_gt(G, T, D, k, Y, st);
  hipLaunchKernelGGL(resid_kernel, dim3(1), dim3(256), 0, st, Y, T, ritz, D, k, resid, ctl);
  return launch_status("sym_lowvecs");
}
