// The one-workgroup and tall-skinny pieces that the two eigenvector routines share (lowvecs.hip: smallest eigenpairs of a positive
// semi-definite matrix; topvecs.hip: largest eigenpairs of an indefinite one), all fp64: the v_mfma_f64_16x16x4_f64 products
// X^T Y and G T, CholeskyQR's k x k Cholesky + inverse in LDS, the cyclic Jacobi Rayleigh-Ritz solver, X <- X M, the residual of
// the returned pairs and the fixed Philox start block.  Widest basis: KMAX = 128 columns.  Include inside the file's anonymous
// namespace, after common.h and philox.h and `using namespace idiff`.
#pragma once

typedef double doublex4 __attribute__((ext_vector_type(4)));

constexpr int KMAX = 128;      // widest basis (k x (k + 1) doubles of LDS in the one-workgroup kernels: 129 KB)
constexpr int CH = 256;        // rows of X per partial sum of X^T Y
constexpr int AR_ROWS = 16;    // rows one workgroup of X <- X M holds in LDS
constexpr int JACOBI_SWEEPS = 40;
constexpr uint64_t X0_SEED = 0x1D1FF7A26E27ull;

// v_mfma_f64_16x16x4_f64: lane l supplies A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]; accumulator register r of
// lane l is C[(l >> 4) + 4 r][l & 15].  The k order of a reduction is free: a lane feeds FOUR consecutive k of its row to four
// consecutive instructions (both operands permuted alike), so its loads of a row-major operand are 32 contiguous bytes.
__device__ __forceinline__ doublex4 mfma(double a, double b, doublex4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

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

// What becomes of element o = row * k + col of the product G T: stored as it is ...
struct StoreProduct {
  double *Y;
  __device__ __forceinline__ void operator()(int64_t o, double acc) const { Y[o] = acc; }
};
// ... or combined into one step of a three-term recurrence, Y = alpha G T + beta T + gamma Z.  Z is read only where gamma != 0 and
// only at the element this lane then writes, so Y may be Z (never T, which other lanes are still reading).
struct StoreAxpby {
  const double *T, *Z;
  double *Y;
  double alpha, beta, gamma;
  __device__ __forceinline__ void operator()(int64_t o, double acc) const {
    double v = alpha * acc + beta * T[o];
    if (gamma != 0.0) v += gamma * Z[o];
    Y[o] = v;
  }
};

// epi(G T) on the matrix cores: wave -> 16 rows of G x all NT * 16 columns of T, the whole of D in steps of 16
template <int NT, class Epi>
__global__ void __launch_bounds__(256) gemm_gt_kernel(const double *__restrict__ G, const double *__restrict__ T, int D, int k, Epi epi) {
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
      if (row < D && col < k) epi((int64_t)row * k + col, acc[t][r]);
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

// Out = In M[:, columns] (+ the failure flag when `poison`): In [D, k], M [k, k], Out [D, kout] with column c of Out from column c of M,
// or, when `reverse`, from column k - 1 - c (the LAST kout columns of M in descending order)
__global__ void __launch_bounds__(256) apply_right_kernel(const double *__restrict__ In, const double *__restrict__ M,
                                                          double *__restrict__ Out, int D, int k, int kout, int reverse,
                                                          const double *__restrict__ ctl, int poison) {
  __shared__ double rows[AR_ROWS * KMAX];
  const int r0 = AR_ROWS * (int)blockIdx.x, nr = D - r0 < AR_ROWS ? D - r0 : AR_ROWS;
  for (int e = threadIdx.x; e < nr * k; e += 256) rows[(e / k) * KMAX + e % k] = In[(int64_t)r0 * k + e];
  __syncthreads();
  const double add = poison ? ctl[1] : 0.0;
  for (int e = threadIdx.x; e < nr * kout; e += 256) {
    const int r = e / kout, c = e % kout, mc = reverse ? k - 1 - c : c;
    double s = 0.0;
    for (int m = 0; m < k; ++m) s += rows[r * KMAX + m] * M[m * k + mc];
    Out[(int64_t)r0 * kout + e] = s + add;
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

template <class Epi>
void launch_gemm_gt(const double *G, const double *T, int D, int k, Epi epi, hipStream_t st) {
  const dim3 grid(ceil_div(D, 64));
  switch (tiles_of(k)) {
    case 1: hipLaunchKernelGGL((gemm_gt_kernel<1, Epi>), grid, dim3(256), 0, st, G, T, D, k, epi); break;
    case 2: hipLaunchKernelGGL((gemm_gt_kernel<2, Epi>), grid, dim3(256), 0, st, G, T, D, k, epi); break;
    case 4: hipLaunchKernelGGL((gemm_gt_kernel<4, Epi>), grid, dim3(256), 0, st, G, T, D, k, epi); break;
    default: hipLaunchKernelGGL((gemm_gt_kernel<8, Epi>), grid, dim3(256), 0, st, G, T, D, k, epi); break;
  }
}

void launch_gemm_gt(const double *G, const double *T, int D, int k, double *Y, hipStream_t st) {
  launch_gemm_gt(G, T, D, k, StoreProduct{Y}, st);
}
