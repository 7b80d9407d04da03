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

typedef double doublex4 __attribute__((ext_vector_type(4)));

constexpr int NB = 32;         // Cholesky panel width = row block of the triangular solves
constexpr int KMAX = 128;      // widest basis (k x (k + 1) doubles of LDS in the one-workgroup kernels: 129 KB)
constexpr int CH = 256;        // rows of X per partial sum of X^T Y
constexpr int STRIP = 64;      // rows one workgroup of a triangular-solve step updates
constexpr int AR_ROWS = 16;    // rows one workgroup of X <- X M holds in LDS
constexpr int ITERS = 4;
constexpr int JACOBI_SWEEPS = 40;
constexpr uint64_t X0_SEED = 0x1D1FF7A26E27ull;

// v_mfma_f64_16x16x4_f64: lane l supplies A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]; accumulator register r of
// lane l is C[(l >> 4) + 4 r][l & 15].  The k order of a reduction is free: a lane feeds FOUR consecutive k of its row to four
// consecutive instructions (both operands permuted alike), so its loads of a row-major operand are 32 contiguous bytes.
__device__ __forceinline__ doublex4 mfma(double a, double b, doublex4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

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

// Cholesky of an n x n block (lower triangle) held in LDS with row pitch `ld`, by the whole workgroup; a pivot that is not
// positive becomes NaN (which then spreads over everything it touches) and raises the flag.
__device__ void chol_lds(double *A, int ld, int n, double *__restrict__ ctl) {
  for (int j = 0; j < n; ++j) {
    __syncthreads();
    const double p = A[j * ld + j];
    const double d = p > 0.0 ? sqrt(p) : quiet_nan();
    __syncthreads();
    if (threadIdx.x == 0) {
      A[j * ld + j] = d;
      if (!(p > 0.0)) ctl[1] = quiet_nan();
    }
    for (int i = j + 1 + threadIdx.x; i < n; i += blockDim.x) A[i * ld + j] /= d;
    __syncthreads();
    const int m = n - j - 1;                 // trailing block: rows / columns j + 1 .. n - 1, lower part
    for (int e = threadIdx.x; e < m * m; e += blockDim.x) {
      const int i = j + 1 + e / m, c = j + 1 + e % m;
      if (c <= i) A[i * ld + c] -= A[i * ld + j] * A[c * ld + j];
    }
  }
  __syncthreads();
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

// X0: standard normals from Philox4x32-10 (counter = index of the group of four elements), the same block on every call
__global__ void __launch_bounds__(256) init_x0_kernel(double *__restrict__ X, int64_t n) {
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; 4 * g < n; g += (int64_t)gridDim.x * 256) {
    const u4 rnd = philox4x32_10({(uint32_t)g, (uint32_t)(g >> 32), 0u, 0u}, (uint32_t)X0_SEED, (uint32_t)(X0_SEED >> 32));
    const float r0 = sqrtf(-2.0f * logf(u01(rnd.x))), r1 = sqrtf(-2.0f * logf(u01(rnd.z)));
    float s0, c0, s1, c1;
    sincosf(6.2831853071795864f * u01(rnd.y), &s0, &c0);
    sincosf(6.2831853071795864f * u01(rnd.w), &s1, &c1);
    const double z[4] = {(double)(r0 * c0), (double)(r0 * s0), (double)(r1 * c1), (double)(r1 * s1)};
    for (int i = 0; i < 4; ++i)
      if (4 * g + i < n) X[4 * g + i] = z[i];
  }
}

// P[ch] = X[rows of chunk ch]^T Y[same rows]  (k x k), on the matrix cores: wave -> 16 columns of X (rows of the product) x all
// NT * 16 columns of Y.  The chunks are summed afterwards in a fixed order (deterministic, no atomics).
template <int NT>
__global__ void __launch_bounds__(256) xty_partial_kernel(const double *__restrict__ X, const double *__restrict__ Y, int D, int k,
                                                          double *__restrict__ P) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, ab = 4 * (int)blockIdx.y + w;
  if (16 * ab >= k) return;
  const int r0 = CH * (int)blockIdx.x, rend = r0 + CH < D ? r0 + CH : D;
  const int acol = 16 * ab + (l & 15) < k ? 16 * ab + (l & 15) : k - 1;
  int bcol[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) bcol[t] = 16 * t + (l & 15) < k ? 16 * t + (l & 15) : k - 1;
  doublex4 acc[NT] = {};
  for (int rr = r0; rr < rend; rr += 16)
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int r = rr + 4 * (l >> 4) + s;
      const bool valid = r < rend;
      const int64_t off = (int64_t)(valid ? r : r0) * k;
      const double a = valid ? X[off + acol] : 0.0;
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = mfma(a, Y[off + bcol[t]], acc[t]);
    }
  double *out = P + (int64_t)blockIdx.x * k * k;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * ab + (l >> 4) + 4 * r, col = 16 * t + (l & 15);
      if (row < k && col < k) out[row * k + col] = acc[t][r];
    }
}

// Y = G T on the matrix cores: wave -> 16 rows of G x all NT * 16 columns of T, the whole of D in steps of 16
template <int NT>
__global__ void __launch_bounds__(256) gemm_gt_kernel(const double *__restrict__ G, const double *__restrict__ T, int D, int k,
                                                      double *__restrict__ Y) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int row0 = 16 * (4 * (int)blockIdx.x + w);
  if (row0 >= D) return;
  const int arow = row0 + (l & 15) < D ? row0 + (l & 15) : D - 1;
  const double *ga = G + (int64_t)arow * D;
  int bcol[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) bcol[t] = 16 * t + (l & 15) < k ? 16 * t + (l & 15) : k - 1;
  doublex4 acc[NT] = {};
  for (int kk = 0; kk < D; kk += 16)
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int kidx = kk + 4 * (l >> 4) + s;
      const bool valid = kidx < D;
      const int kc = valid ? kidx : 0;
      const double a = valid ? ga[kc] : 0.0;
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = mfma(a, T[(int64_t)kc * k + bcol[t]], acc[t]);
    }
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = row0 + (l >> 4) + 4 * r, col = 16 * t + (l & 15);
      if (row < D && col < k) Y[(int64_t)row * k + col] = acc[t][r];
    }
}

// CholeskyQR, the k x k part, one workgroup: W = sum of the partial Grams (lower triangle), W = C C^T in LDS, then
// M = C^-T (upper triangular, [k, k] row-major) so that X M has orthonormal columns.  Column j of C^-1 is one lane's
// forward substitution, kept in the unused upper triangle of the LDS array: A[j][i] = (C^-1)[i][j] = M[j][i].
__global__ void __launch_bounds__(256) chol_inv_kernel(const double *__restrict__ P, int nch, int k, double *__restrict__ M,
                                                       double *__restrict__ ctl) {
  extern __shared__ double lds[];
  const int ld = k + 1;
  double *A = lds, *invd = lds + k * ld;
  for (int e = threadIdx.x; e < k * k; e += 256) {
    double s = 0.0;
    for (int ch = 0; ch < nch; ++ch) s += P[(int64_t)ch * k * k + e];
    A[(e / k) * ld + e % k] = s;
  }
  chol_lds(A, ld, k, ctl);
  const int j = threadIdx.x;
  if (j < k) {
    invd[j] = 1.0 / A[j * ld + j];
    for (int i = j + 1; i < k; ++i) {
      double s = A[i * ld + j] * invd[j];
      for (int m = j + 1; m < i; ++m) s += A[i * ld + m] * A[j * ld + m];
      A[j * ld + i] = -s / A[i * ld + i];
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < k * k; e += 256) {
    const int a = e / k, b = e % k;
    M[e] = a < b ? A[a * ld + b] : (a == b ? invd[a] : 0.0);
  }
}

// Out = In M (+ the failure flag when `poison`): In, Out [D, k], M [k, k]
__global__ void __launch_bounds__(256) apply_right_kernel(const double *__restrict__ In, const double *__restrict__ M,
                                                          double *__restrict__ Out, int D, int k, const double *__restrict__ ctl,
                                                          int poison) {
  __shared__ double rows[AR_ROWS * KMAX];
  const int r0 = AR_ROWS * (int)blockIdx.x, nr = D - r0 < AR_ROWS ? D - r0 : AR_ROWS;
  for (int e = threadIdx.x; e < nr * k; e += 256) rows[(e / k) * KMAX + e % k] = In[(int64_t)r0 * k + e];
  __syncthreads();
  const double add = poison ? ctl[1] : 0.0;
  for (int e = threadIdx.x; e < nr * k; e += 256) {
    const int r = e / k, c = e % k;
    double s = 0.0;
    for (int m = 0; m < k; ++m) s += rows[r * KMAX + m] * M[m * k + c];
    Out[(int64_t)r0 * k + e] = s + add;
  }
}

// Rayleigh-Ritz, the k x k part, one workgroup: H = sym(sum of the partials of X^T (G X)) in LDS, cyclic Jacobi with the
// round-robin ordering (k / 2 disjoint rotations per round, k - 1 rounds per sweep), eigenvectors accumulated in `Wt`
// (global, k x k); then the eigenvalues ascending into ritz and the eigenvectors, in that order, into the columns of M.
__global__ void __launch_bounds__(256) jacobi_kernel(const double *__restrict__ P, int nch, int k, double *__restrict__ Wt,
                                                     double *__restrict__ M, double *__restrict__ ritz, double *__restrict__ ctl) {
  extern __shared__ double lds[];
  __shared__ double red[256], rc[KMAX / 2], rs[KMAX / 2], lam[KMAX];
  __shared__ int rp[KMAX / 2], rq[KMAX / 2], rank[KMAX], anynan;
  const int ld = k + 1, tid = threadIdx.x;
  double *H = lds;
  for (int e = tid; e < k * k; e += 256) {
    const int a = e / k, b = e % k;
    double s = 0.0, st = 0.0;
    for (int ch = 0; ch < nch; ++ch) { s += P[(int64_t)ch * k * k + a * k + b]; st += P[(int64_t)ch * k * k + b * k + a]; }
    H[a * ld + b] = 0.5 * (s + st);
    Wt[e] = a == b ? 1.0 : 0.0;
  }
  __syncthreads();
  const int n = k + (k & 1), npairs = n / 2;
  double tot = 0.0;
  for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
    double all = 0.0, off = 0.0;
    for (int e = tid; e < k * k; e += 256) {
      const double v = H[(e / k) * ld + e % k];
      all += v * v;
      if (e / k != e % k) off += v * v;
    }
    red[tid] = sweep == 0 ? all : off;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) { if (tid < s) red[tid] += red[tid + s]; __syncthreads(); }
    const double first = red[0];
    __syncthreads();
    if (sweep == 0) {
      tot = first;
      red[tid] = off;
      __syncthreads();
      for (int s = 128; s > 0; s >>= 1) { if (tid < s) red[tid] += red[tid + s]; __syncthreads(); }
      off = red[0];
      __syncthreads();
    } else {
      off = first;
    }
    if (!(off > 1e-34 * tot)) break;              // converged -- or NaN: either way no further sweep
    for (int r = 0; r < n - 1; ++r) {
      if (tid < npairs) {
        const int a = tid == 0 ? n - 1 : (r + tid) % (n - 1), b = tid == 0 ? r : (r - tid + n - 1) % (n - 1);
        const int p = a < b ? a : b, q = a < b ? b : a;
        double c = 1.0, s = 0.0;
        const double hpq = q < k ? H[p * ld + q] : 0.0;
        if (hpq != 0.0) {
          const double th = (H[q * ld + q] - H[p * ld + p]) / (2.0 * hpq);
          const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
          c = 1.0 / sqrt(t * t + 1.0);
          s = t * c;
        }
        rp[tid] = q < k ? p : -1; rq[tid] = q; rc[tid] = c; rs[tid] = s;
      }
      __syncthreads();
      for (int e = tid; e < npairs * k; e += 256) {            // H <- H J, W <- W J: columns p, q of every row
        const int pi = e / k, row = e % k, p = rp[pi], q = rq[pi];
        if (p < 0) continue;
        const double c = rc[pi], s = rs[pi];
        const double hp = H[row * ld + p], hq = H[row * ld + q];
        H[row * ld + p] = c * hp - s * hq; H[row * ld + q] = s * hp + c * hq;
        const double wp = Wt[row * k + p], wq = Wt[row * k + q];
        Wt[row * k + p] = c * wp - s * wq; Wt[row * k + q] = s * wp + c * wq;
      }
      __syncthreads();
      for (int e = tid; e < npairs * k; e += 256) {            // H <- J^T H: rows p, q of every column
        const int pi = e / k, col = e % k, p = rp[pi], q = rq[pi];
        if (p < 0) continue;
        const double c = rc[pi], s = rs[pi];
        const double hp = H[p * ld + col], hq = H[q * ld + col];
        H[p * ld + col] = c * hp - s * hq; H[q * ld + col] = s * hp + c * hq;
      }
      __syncthreads();
      if (tid < npairs && rp[tid] >= 0 && rs[tid] != 0.0) { H[rp[tid] * ld + rq[tid]] = 0.0; H[rq[tid] * ld + rp[tid]] = 0.0; }
      __syncthreads();
    }
  }
  if (tid == 0) anynan = 0;
  __syncthreads();
  if (tid < k) {
    lam[tid] = H[tid * ld + tid];
    if (!(lam[tid] == lam[tid])) anynan = 1;
  }
  __syncthreads();
  if (tid < k) {
    int rk = 0;
    for (int j = 0; j < k; ++j) rk += (lam[j] < lam[tid]) || (!(lam[tid] < lam[j]) && j < tid);
    rank[tid] = rk < k ? rk : k - 1;
    ritz[rank[tid]] = lam[tid];
  }
  if (tid == 0 && anynan) ctl[1] = quiet_nan();
  __syncthreads();
  for (int e = tid; e < k * k; e += 256) M[(e / k) * k + rank[e % k]] = Wt[e];
}

// resid = |Y - T diag(ritz)|_F + flag, ritz += flag; one workgroup, a fixed summation order
__global__ void __launch_bounds__(256) resid_kernel(const double *__restrict__ Y, const double *__restrict__ T, double *__restrict__ ritz,
                                                    int D, int k, double *__restrict__ resid, const double *__restrict__ ctl) {
  __shared__ double red[256], lam[KMAX];
  if ((int)threadIdx.x < k) lam[threadIdx.x] = ritz[threadIdx.x];
  __syncthreads();
  double s = 0.0;
  const int64_t n = (int64_t)D * k;
  for (int64_t e = threadIdx.x; e < n; e += 256) {
    const double d = Y[e] - T[e] * lam[e % k];
    s += d * d;
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) { if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h]; __syncthreads(); }
  const double flag = ctl[1];
  if (threadIdx.x == 0) resid[0] = sqrt(red[0]) + flag;
  if ((int)threadIdx.x < k) ritz[threadIdx.x] = lam[threadIdx.x] + flag;
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

int tiles_of(int k) { const int t = ceil_div(k, 16); return t <= 1 ? 1 : t <= 2 ? 2 : t <= 4 ? 4 : 8; }

void launch_xty(const double *X, const double *Y, int D, int k, double *P, int nch, hipStream_t st) {
  const dim3 grid(nch, ceil_div(ceil_div(k, 16), 4));
  switch (tiles_of(k)) {
    case 1: hipLaunchKernelGGL(xty_partial_kernel<1>, grid, dim3(256), 0, st, X, Y, D, k, P); break;
    case 2: hipLaunchKernelGGL(xty_partial_kernel<2>, grid, dim3(256), 0, st, X, Y, D, k, P); break;
    case 4: hipLaunchKernelGGL(xty_partial_kernel<4>, grid, dim3(256), 0, st, X, Y, D, k, P); break;
    default: hipLaunchKernelGGL(xty_partial_kernel<8>, grid, dim3(256), 0, st, X, Y, D, k, P); break;
  }
}

void launch_gemm_gt(const double *G, const double *T, int D, int k, double *Y, hipStream_t st) {
  const dim3 grid(ceil_div(D, 64));
  switch (tiles_of(k)) {
    case 1: hipLaunchKernelGGL(gemm_gt_kernel<1>, grid, dim3(256), 0, st, G, T, D, k, Y); break;
    case 2: hipLaunchKernelGGL(gemm_gt_kernel<2>, grid, dim3(256), 0, st, G, T, D, k, Y); break;
    case 4: hipLaunchKernelGGL(gemm_gt_kernel<4>, grid, dim3(256), 0, st, G, T, D, k, Y); break;
    default: hipLaunchKernelGGL(gemm_gt_kernel<8>, grid, dim3(256), 0, st, G, T, D, k, Y); break;
  }
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
      hipLaunchKernelGGL(apply_right_kernel, dim3(ceil_div(D, AR_ROWS)), dim3(256), 0, st, src, M, dst, D, k, ctl, 0);
    }
  }

  // ---- Rayleigh-Ritz and the residual of what is returned
  launch_gemm_gt(G, X, D, k, Y, st);
  launch_xty(X, Y, D, k, P, o.nch, st);
  hipLaunchKernelGGL(jacobi_kernel, dim3(1), dim3(256), small_lds, st, P, o.nch, k, Wt, M, ritz, ctl);
  hipLaunchKernelGGL(apply_right_kernel, dim3(ceil_div(D, AR_ROWS)), dim3(256), 0, st, X, M, T, D, k, ctl, 1);
  launch_gemm_gt(G, T, D, k, Y, st);
  hipLaunchKernelGGL(resid_kernel, dim3(1), dim3(256), 0, st, Y, T, ritz, D, k, resid, ctl);
  return launch_status("sym_lowvecs");
}
