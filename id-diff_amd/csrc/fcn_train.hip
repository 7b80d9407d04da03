// Training of the fcn score network (models/fcn.py): the kernels the backward pass and the optimiser need beside idiff_gemm_f32.
//
//   gemm_nn   C[M, N] = (A[M, K] . Bm[K, N]) (*) g(P)     data gradient: A = dL/dA_l, Bm = the weight as it lies ([out, in], `in`
//                                                          contiguous), P = the ELU output of the layer below, g(a) = a > 0 ? 1 : a + 1
//   gemm_tn   C[M, N] = At[K, M]^T . Bm[K, N]              weight gradient: At = dL/dA_l, Bm = the layer's input, K = the batch;
//             colsum[M] = sum_k At[k, m]                   the bias gradient from the tile the kernel has in LDS anyway
//   dsm_loss_grad, grad_sumsq, adam_step, fcn_train_input  streaming kernels around them
//
// Both contractions run on v_mfma_f32_32x32x2_f32: a k-ordered chain of fp32 fmas, one rounding per product, so the result is
// within K 2^-24 sum_k |a_k b_k| of the exact one whatever the tile order.  One workgroup of four waves owns a 64 x 64 tile of C
// and walks K in steps of 32; each wave owns one 32 x 32 accumulator (the instruction's dependent latency equals its issue interval,
// one accumulator keeps the matrix core busy).  Both operands lie in LDS K-MAJOR -- tile[k][m] and tile[k][n] -- which is the
// instruction's own lane map (lane l: A[m = l & 31][k = l >> 5], B[k = l >> 5][n = l & 31]): a wave's operand read is two runs of 32
// consecutive floats, and with a pitch of 96 floats (= 32 mod 64 banks) the two runs fall on disjoint banks.  The operands that
// are stored with the tile's long side contiguous (Bm in both kernels, At in gemm_tn) go to LDS as they come, 16 bytes per lane; only
// gemm_nn's A, which is K-contiguous, is transposed on its way in (lanes of a wave hold consecutive rows, so the four scalar LDS
// writes of a lane's float4 are conflict-free).  The next K step's global loads are issued before the current step's MFMAs.
//
// K is never split across workgroups and nothing is accumulated in memory: no atomics, no workspace, the same bits on every run.
// The reductions (loss, squared gradient norm) are two launches each: per-workgroup fp64 partials over FIXED element ranges into a
// caller-supplied workspace indexed by workgroup, then one workgroup that adds them in index order.
#include "common.h"
#include <math.h>

namespace {
using namespace idiff;

typedef float floatx16 __attribute__((ext_vector_type(16)));

constexpr int BM = 64, BN = 64, BK = 32, THREADS = 256, PITCH = 96;
constexpr int RED_THREADS = 256;
constexpr int RED_MAX_BLOCKS = IDIFF_REDUCE_WS_DOUBLES;

struct GemmP {
  const float *A, *B, *P;
  float *C, *colsum;
  int64_t lda, ldb, ldc, ldp;
  int M, N, K;
};

// 16 bytes of row `row` (valid: row < rows) at column c .. c + 3 of a matrix whose rows hold `cols` floats; zero outside
__device__ __forceinline__ float4 load4(const float *base, int64_t ld, int row, int rows, int c, int cols) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (row < rows) {
    const float *src = base + (int64_t)row * ld + c;
    if (c + 3 < cols) {
      v = *reinterpret_cast<const float4 *>(src);
    } else {
      if (c < cols) v.x = src[0];
      if (c + 1 < cols) v.y = src[1];
      if (c + 2 < cols) v.z = src[2];
    }
  }
  return v;
}

template <bool TN> __global__ void __launch_bounds__(THREADS) gemm_kernel(GemmP p) {
  __shared__ __attribute__((aligned(16))) float As[BK * PITCH];
  __shared__ __attribute__((aligned(16))) float Bs[BK * PITCH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
  const bool do_colsum = TN && p.colsum && blockIdx.x == 0 && tid < BM;
  float cs = 0.f;
  floatx16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float4 ra[2], rb[2];

  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int idx = tid + THREADS * i;
      const int k = idx >> 4, c = (idx & 15) * 4;          // rows of 64 floats = 16 float4
      rb[i] = load4(p.B, p.ldb, k0 + k, p.K, n0 + c, p.N);
      if (TN) {
        ra[i] = load4(p.A, p.lda, k0 + k, p.K, m0 + c, p.M);
      } else {
        const int m = idx & 63, k4 = (idx >> 6) * 4;       // a wave: 64 consecutive rows, one float4 of k each
        ra[i] = load4(p.A, p.lda, m0 + m, p.M, k0 + k4, p.K);
      }
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int idx = tid + THREADS * i;
      const int k = idx >> 4, c = (idx & 15) * 4;
      *reinterpret_cast<float4 *>(&Bs[k * PITCH + c]) = rb[i];
      if (TN) {
        *reinterpret_cast<float4 *>(&As[k * PITCH + c]) = ra[i];
      } else {
        const int m = idx & 63, k4 = (idx >> 6) * 4;
        As[(k4 + 0) * PITCH + m] = ra[i].x;
        As[(k4 + 1) * PITCH + m] = ra[i].y;
        As[(k4 + 2) * PITCH + m] = ra[i].z;
        As[(k4 + 3) * PITCH + m] = ra[i].w;
      }
    }
  };

  fetch(0);
  const float *ap = As + (lane >> 5) * PITCH + wm + (lane & 31);
  const float *bp = Bs + (lane >> 5) * PITCH + wn + (lane & 31);
  for (int k0 = 0; k0 < p.K; k0 += BK) {
    stage();
    __syncthreads();
    if (k0 + BK < p.K) fetch(k0 + BK);
#pragma unroll
    for (int kk = 0; kk < BK; kk += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[kk * PITCH], bp[kk * PITCH], acc, 0, 0, 0);
    if (do_colsum) {
      // rows k >= K of the tile are zero: adding them changes nothing, and the order k = 0, 1, ... is the same on every run
#pragma unroll
      for (int k = 0; k < BK; ++k) cs += As[k * PITCH + tid];
    }
    __syncthreads();
  }

  if (do_colsum && m0 + tid < p.M) p.colsum[m0 + tid] = cs;
  const int col = n0 + wn + (lane & 31);
  if (col >= p.N) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    if (row >= p.M) continue;
    float v = acc[r];
    if (!TN && p.P) {
      const float a = p.P[(int64_t)row * p.ldp + col];
      if (!(a > 0.f)) v = fmaf(v, a, v);                  // v (a + 1) in one rounding
    }
    p.C[(int64_t)row * p.ldc + col] = v;
  }
}

// ---- fixed-order reductions: workgroup b owns the elements [b * per, (b + 1) * per), a lane adds its strided share in fp64, the 256
// lane sums are folded by a tree whose shape does not depend on the data; partial b goes to ws[b]
__device__ __forceinline__ double block_sum(double v, double *sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int s = RED_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  return sh[0];
}

__global__ void __launch_bounds__(RED_THREADS)
dsm_partial_kernel(const float *__restrict__ out, const float *__restrict__ z, const float *__restrict__ w, float *__restrict__ G,
                   int64_t total, int D, int64_t ldg, int64_t per, double s, double *__restrict__ ws) {
  __shared__ double sh[RED_THREADS];
  const int64_t lo = (int64_t)blockIdx.x * per, hi = lo + per < total ? lo + per : total;
  double acc = 0.0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += RED_THREADS) {
    const int64_t b = i / D;
    const double om = w ? (double)w[b] : 1.0;
    const double d = (double)out[i] - (double)z[i];
    acc += om * d * d;
    if (G) G[b * ldg + (i - b * D)] = (float)(s * om * d);
  }
  const double tot = block_sum(acc, sh);
  if (threadIdx.x == 0) ws[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(RED_THREADS)
sumsq_partial_kernel(const float *__restrict__ x, int64_t total, int64_t per, double *__restrict__ ws) {
  __shared__ double sh[RED_THREADS];
  const int64_t lo = (int64_t)blockIdx.x * per, hi = lo + per < total ? lo + per : total;
  double acc = 0.0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += RED_THREADS) {
    const double v = (double)x[i];
    acc += v * v;
  }
  const double tot = block_sum(acc, sh);
  if (threadIdx.x == 0) ws[blockIdx.x] = tot;
}

// one workgroup: scale * sum_b ws[b], b in index order per lane, the same tree; as a float (the loss) or a double (the squared norm)
__global__ void __launch_bounds__(RED_THREADS)
reduce_final_kernel(const double *__restrict__ ws, int n, double scale, float *__restrict__ out_f, double *__restrict__ out_d) {
  __shared__ double sh[RED_THREADS];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += RED_THREADS) acc += ws[i];
  const double tot = block_sum(acc, sh);
  if (threadIdx.x == 0) {
    if (out_f) *out_f = (float)(scale * tot);
    if (out_d) *out_d = scale * tot;
  }
}

inline void reduction_grid(int64_t total, int *blocks, int64_t *per) {
  int64_t nb = ceil_div64(total, 4 * RED_THREADS);
  if (nb > RED_MAX_BLOCKS) nb = RED_MAX_BLOCKS;
  if (nb < 1) nb = 1;
  *per = ceil_div64(total, nb);
  *blocks = (int)ceil_div64(total, *per);
}

struct AdamP {
  float *theta, *m, *v;
  const float *grad;
  const double *sumsq;
  int64_t n;
  double max_norm, step_size, beta1, beta2, eps, weight_decay, inv_sqrt_bc2;
};

// torch.optim.Adam (L2 weight decay, no amsgrad) behind clip_grad_norm_, evaluated in fp64 from the fp32 state and rounded once per
// output: m, v and theta are each within one fp32 rounding of the exact update of the state they were given
__global__ void __launch_bounds__(256) adam_kernel(AdamP p) {
  double coef = 1.0;
  if (p.sumsq) {
    const double c = p.max_norm / (sqrt(*p.sumsq) + 1e-6);
    coef = c < 1.0 ? c : 1.0;
  }
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < p.n; i += (int64_t)gridDim.x * blockDim.x) {
    const double th = (double)p.theta[i];
    const double g = (double)p.grad[i] * coef + p.weight_decay * th;
    const double m0 = (double)p.m[i];
    const double m = m0 + (1.0 - p.beta1) * (g - m0);
    const double v = p.beta2 * (double)p.v[i] + (1.0 - p.beta2) * g * g;
    const double denom = sqrt(v) * p.inv_sqrt_bc2 + p.eps;
    p.m[i] = (float)m;
    p.v[i] = (float)v;
    p.theta[i] = (float)(th - p.step_size * (m / denom));
  }
}

// h[b, :D] = mean_coeff[b] x[b, :] + std[b] z[b, :], h[b, D] = label[b], h[b, D + 1 : kpad] = 0: the network's input row
__global__ void __launch_bounds__(256)
train_input_kernel(const float *__restrict__ x, const float *__restrict__ z, const float *__restrict__ std_,
                   const float *__restrict__ mean_coeff, const float *__restrict__ label, float *__restrict__ h, int64_t B, int D,
                   int kpad) {
  const int64_t total = B * kpad;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / kpad;
    const int c = (int)(i - b * kpad);
    float v = 0.f;
    if (c < D) {
      const float mc = mean_coeff ? mean_coeff[b] : 1.0f;
      v = fmaf(std_[b], z[b * D + c], mc * x[b * D + c]);
    } else if (c == D) {
      v = label[b];
    }
    h[i] = v;
  }
}

int check_gemm(const char *who, const void *A, int64_t lda, int64_t a_row, const void *B, int64_t ldb, const void *C, int64_t ldc,
               const void *P, int64_t ldp, const void *colsum, int M, int N, int K) {
  if (M < 1 || N < 1 || K < 1) return fail("%s: M = %d, N = %d, K = %d: every size must be positive", who, M, N, K);
  if (!A || !B || !C) return fail("%s: null pointer", who);
  if (((uintptr_t)A & 15) || ((uintptr_t)B & 15) || ((uintptr_t)C & 15) || ((uintptr_t)P & 15) || ((uintptr_t)colsum & 3))
    return fail("%s: the matrices must be 16-byte aligned (the column sums 4-byte)", who);
  if (lda < a_row || ldb < N || ldc < N || (P && ldp < N))
    return fail("%s: a leading dimension is shorter than its row (lda %lld, ldb %lld, ldc %lld, ldp %lld)", who, (long long)lda,
                (long long)ldb, (long long)ldc, (long long)ldp);
  if ((lda & 3) || (ldb & 3) || (ldc & 3) || (P && (ldp & 3)))
    return fail("%s: leading dimensions must be multiples of 4 floats (16-byte rows)", who);
  if (ceil_div(M, BM) > 65535) return fail("%s: M = %d exceeds the grid (at most %d rows)", who, M, 65535 * BM);
  return 0;
}

}  // namespace

IDIFF_API int idiff_gemm_nn_ok(int M, int N, int K) { return M >= 1 && N >= 1 && K >= 1 && ceil_div(M, BM) <= 65535 ? 1 : 0; }
IDIFF_API int idiff_gemm_tn_ok(int M, int N, int K) { return idiff_gemm_nn_ok(M, N, K); }

IDIFF_API int idiff_gemm_nn_f32(const float *A, int64_t lda, const float *Bm, int64_t ldb, float *C, int64_t ldc, const float *P,
                                int64_t ldp, int M, int N, int K, void *stream) {
  if (int rc = check_gemm("gemm_nn", A, lda, K, Bm, ldb, C, ldc, P, ldp, nullptr, M, N, K)) return rc;
  GemmP p = {A, Bm, P, C, nullptr, lda, ldb, ldc, ldp, M, N, K};
  hipLaunchKernelGGL(gemm_kernel<false>, dim3(ceil_div(N, BN), ceil_div(M, BM)), dim3(THREADS), 0, (hipStream_t)stream, p);
  return launch_status("gemm_nn");
}

IDIFF_API int idiff_gemm_tn_f32(const float *At, int64_t lda, const float *Bm, int64_t ldb, float *C, int64_t ldc, float *colsum,
                                int M, int N, int K, void *stream) {
  if (int rc = check_gemm("gemm_tn", At, lda, M, Bm, ldb, C, ldc, nullptr, 0, colsum, M, N, K)) return rc;
  GemmP p = {At, Bm, nullptr, C, colsum, lda, ldb, ldc, 0, M, N, K};
  hipLaunchKernelGGL(gemm_kernel<true>, dim3(ceil_div(N, BN), ceil_div(M, BM)), dim3(THREADS), 0, (hipStream_t)stream, p);
  return launch_status("gemm_tn");
}

IDIFF_API int idiff_dsm_loss_grad_f32(const float *out, const float *z, const float *weight, float *G, int64_t ldg, float *loss,
                                      double *ws, int B, int D, int reduce_mean, void *stream) {
  if (B < 1 || D < 1) return fail("dsm_loss_grad: B = %d, D = %d: both must be positive", B, D);
  if (!out || !z || !loss || !ws) return fail("dsm_loss_grad: null pointer");
  if (G && ldg < D) return fail("dsm_loss_grad: ldg = %lld is shorter than a row of %d", (long long)ldg, D);
  if (((uintptr_t)out & 3) || ((uintptr_t)z & 3) || ((uintptr_t)weight & 3) || ((uintptr_t)G & 3) || ((uintptr_t)loss & 3) ||
      ((uintptr_t)ws & 7))
    return fail("dsm_loss_grad: out, z, weight, G and loss must be 4-byte aligned, the workspace 8-byte");
  const int64_t total = (int64_t)B * D;
  // reduce_mean: mean_b mean_d; otherwise mean_b (1/2) sum_d (losses.py: reduce_op)
  const double s = reduce_mean ? 2.0 / ((double)B * D) : 1.0 / (double)B;
  const double loss_scale = reduce_mean ? 1.0 / ((double)B * D) : 0.5 / (double)B;
  int blocks;
  int64_t per;
  reduction_grid(total, &blocks, &per);
  hipLaunchKernelGGL(dsm_partial_kernel, dim3(blocks), dim3(RED_THREADS), 0, (hipStream_t)stream, out, z, weight, G, total, D, ldg, per, s, ws);
  hipLaunchKernelGGL(reduce_final_kernel, dim3(1), dim3(RED_THREADS), 0, (hipStream_t)stream, (const double *)ws, blocks, loss_scale,
                     loss, (double *)nullptr);
  return launch_status("dsm_loss_grad");
}

IDIFF_API int idiff_grad_sumsq_f32(const float *x, int64_t n, double *ws, double *sumsq, void *stream) {
  if (n < 1) return fail("grad_sumsq: n = %lld must be positive", (long long)n);
  if (!x || !ws || !sumsq) return fail("grad_sumsq: null pointer");
  if (((uintptr_t)x & 3) || ((uintptr_t)ws & 7) || ((uintptr_t)sumsq & 7))
    return fail("grad_sumsq: x must be 4-byte aligned, the workspace and the result 8-byte");
  int blocks;
  int64_t per;
  reduction_grid(n, &blocks, &per);
  hipLaunchKernelGGL(sumsq_partial_kernel, dim3(blocks), dim3(RED_THREADS), 0, (hipStream_t)stream, x, n, per, ws);
  hipLaunchKernelGGL(reduce_final_kernel, dim3(1), dim3(RED_THREADS), 0, (hipStream_t)stream, (const double *)ws, blocks, 1.0,
                     (float *)nullptr, sumsq);
  return launch_status("grad_sumsq");
}

IDIFF_API int idiff_adam_step_f32(float *theta, const float *grad, float *m, float *v, int64_t n, const double *sumsq, double max_norm,
                                  double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step, void *stream) {
  if (n < 1) return fail("adam_step: n = %lld must be positive", (long long)n);
  if (step < 1) return fail("adam_step: step = %lld: the first step is 1", (long long)step);
  if (!theta || !grad || !m || !v) return fail("adam_step: null pointer");
  if (((uintptr_t)theta & 3) || ((uintptr_t)grad & 3) || ((uintptr_t)m & 3) || ((uintptr_t)v & 3) || ((uintptr_t)sumsq & 7))
    return fail("adam_step: theta, grad, m and v must be 4-byte aligned, the squared norm 8-byte");
  if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) || !(lr >= 0.0) || !(weight_decay >= 0.0))
    return fail("adam_step: lr %g, betas (%g, %g), eps %g, weight_decay %g outside torch.optim.Adam's ranges", lr, beta1, beta2, eps,
                weight_decay);
  if (sumsq && !(max_norm > 0.0)) return fail("adam_step: max_norm = %g with a squared norm given (pass none to disable clipping)", max_norm);
  const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
  AdamP p = {theta, m, v, grad, sumsq, n, max_norm, lr / bc1, beta1, beta2, eps, weight_decay, 1.0 / sqrt(bc2)};
  hipLaunchKernelGGL(adam_kernel, dim3(streaming_grid(n, 256)), dim3(256), 0, (hipStream_t)stream, p);
  return launch_status("adam_step");
}

IDIFF_API int idiff_fcn_train_input_f32(const float *x, const float *z, const float *std_, const float *mean_coeff, const float *label,
                                        float *h, int64_t B, int D, int kpad, void *stream) {
  if (B < 1 || D < 1 || kpad <= D) return fail("fcn_train_input: B = %lld, D = %d, kpad = %d (needs kpad > D >= 1)", (long long)B, D, kpad);
  if (!x || !z || !std_ || !label || !h) return fail("fcn_train_input: null pointer");
  if (((uintptr_t)x & 3) || ((uintptr_t)z & 3) || ((uintptr_t)std_ & 3) || ((uintptr_t)mean_coeff & 3) || ((uintptr_t)label & 3) ||
      ((uintptr_t)h & 3))
    return fail("fcn_train_input: pointers must be 4-byte aligned");
  hipLaunchKernelGGL(train_input_kernel, dim3(streaming_grid(B * kpad, 256)), dim3(256), 0, (hipStream_t)stream, x, z, std_, mean_coeff,
                     label, h, B, D, kpad);
  return launch_status("fcn_train_input");
}
