// The probability-flow ODE of a score model (ode.py, likelihood.py): the arithmetic over the batch of an adaptive Runge-Kutta step whose
// step-size control stays on the host.  The state y is [B, W] doubles, W = D + aug (aug = 1: the last column carries log p), the seven
// stage derivatives K are [7][B, W] doubles, the network reads the first D columns of a stage's argument as fp32 rows [B, kpad] with the
// time label in column D.
//
//   rk_stage    v = y + sum_{j < ns} c_j K_j  (the host passes c_j = h a_sj, or h b_j for the solution); v optionally becomes the new
//               state; fl32(v[:, :D]) and the label always go to the network's input rows.  The pad columns beyond the label are not written.
//   rk_error    sum_{r, c} ((sum_{j < 7} e_j K_j[r, c]) / (atol + rtol max(|y|, |y_new|)))^2 as one device double, e_j = h E_j
//   flow_rhs    K_s[r, c < D] = a x32[r, c] + b v[r, c];  with aug  K_s[r, D] = a D + b q[r],  q[r] = sum_c eps[r, c] u[r, c] (Hutchinson)
//               or a given device vector (the exact trace)
//   jvp_trace   tr[p] = sum_{i < D} sum_n T[p][i, n] W_out[i, n]: the trace of the network Jacobian from the tangent rows in front of the
//               output layer
//
// Arithmetic: fp64 throughout, fp32 inputs widened exactly, every output rounded once.  Sums over j run in index order with one fma per
// term; the reductions add fixed ranges in a fixed order (a lane's strided share, then a tree whose shape does not depend on the data), no
// atomics: the same arguments give the same bits.  rk_stage and flow_rhs move two doubles (16 bytes) per access where every pointer is
// 16-byte aligned and every pitch even, one otherwise.
#include "common.h"

namespace {
using namespace idiff;

constexpr int RED_THREADS = 256;
constexpr int MAX_STAGES = 7;

struct Coef {
  double c[MAX_STAGES];
};

// ---------------------------------------------------------------------------------------------- rk_stage
struct StageP {
  const double *y, *K;
  double *y_out;
  float *x32;
  int64_t ldy, ldk, strideK, ldyo, ldx, B;
  int D, W, ns;
  float label_value;
  Coef c;
};

template <bool VEC> __global__ void __launch_bounds__(256) stage_kernel(StageP p) {
  const int64_t G = (p.W + 1) >> 1, total = p.B * G;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = g / G;
    const int col = (int)(g - r * G) * 2;
    const bool two = col + 1 < p.W;
    double s0 = 0.0, s1 = 0.0;
    const double *k = p.K + r * p.ldk + col;
#pragma unroll
    for (int j = 0; j < MAX_STAGES - 1; ++j) {
      if (j < p.ns) {
        if (VEC && two) {
          const double2 kv = *reinterpret_cast<const double2 *>(k + j * p.strideK);
          s0 = fma(p.c.c[j], kv.x, s0);
          s1 = fma(p.c.c[j], kv.y, s1);
        } else {
          s0 = fma(p.c.c[j], k[j * p.strideK], s0);
          if (two) s1 = fma(p.c.c[j], k[j * p.strideK + 1], s1);
        }
      }
    }
    const double *yr = p.y + r * p.ldy + col;
    double v0, v1 = 0.0;
    if (VEC && two) {
      const double2 yv = *reinterpret_cast<const double2 *>(yr);
      v0 = yv.x + s0;
      v1 = yv.y + s1;
    } else {
      v0 = yr[0] + s0;
      if (two) v1 = yr[1] + s1;
    }
    if (p.y_out) {
      double *yo = p.y_out + r * p.ldyo + col;
      if (VEC && two) {
        *reinterpret_cast<double2 *>(yo) = make_double2(v0, v1);
      } else {
        yo[0] = v0;
        if (two) yo[1] = v1;
      }
    }
    float *xr = p.x32 + r * p.ldx;
    if (col < p.D) xr[col] = (float)v0;
    if (two && col + 1 < p.D) xr[col + 1] = (float)v1;
    if (col == 0) xr[p.D] = p.label_value;
  }
}

// ---------------------------------------------------------------------------------------------- fixed-order reductions
__device__ __forceinline__ double block_sum(double v, double *sh) {
  __syncthreads();                       // the previous use's sh[0] has been read
  sh[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int s = RED_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  return sh[0];
}

struct ErrorP {
  const double *K, *y, *y_new;
  double *ws;
  int64_t ldk, strideK, ldy, ldyn, total, per;
  int W;
  double atol, rtol;
  Coef e;
};

// workgroup b owns the elements [b per, (b + 1) per) of the B W elements in row-major order
__global__ void __launch_bounds__(RED_THREADS) error_partial_kernel(ErrorP p) {
  __shared__ double sh[RED_THREADS];
  const int64_t lo = (int64_t)blockIdx.x * p.per, hi = lo + p.per < p.total ? lo + p.per : p.total;
  double acc = 0.0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += RED_THREADS) {
    const int64_t r = i / p.W;
    const int c = (int)(i - r * p.W);
    const double *k = p.K + r * p.ldk + c;
    double err = 0.0;
#pragma unroll
    for (int j = 0; j < MAX_STAGES; ++j) err = fma(p.e.c[j], k[j * p.strideK], err);
    const double a = fabs(p.y[r * p.ldy + c]), b = fabs(p.y_new[r * p.ldyn + c]);
    const double q = err / (p.atol + p.rtol * fmax(a, b));
    acc = fma(q, q, acc);
  }
  const double tot = block_sum(acc, sh);
  if (threadIdx.x == 0) p.ws[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(RED_THREADS) error_final_kernel(const double *__restrict__ ws, int n, double *__restrict__ out) {
  __shared__ double sh[RED_THREADS];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += RED_THREADS) acc += ws[i];
  const double tot = block_sum(acc, sh);
  if (threadIdx.x == 0) *out = tot;
}

// ---------------------------------------------------------------------------------------------- flow_rhs
struct RhsP {
  const float *x32, *v, *eps, *u;
  const double *q;
  double *Ks;
  int64_t ldx, ldv, lde, ldu, ldk, B;
  int D, aug;
  double a, b;
};

// one wave per row: a lane owns the column pairs lane, lane + 64, ...; the Hutchinson sum adds a lane's products in that order and folds
// the 64 lane sums by a fixed shuffle tree
template <bool VEC> __global__ void __launch_bounds__(256) rhs_kernel(RhsP p) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= p.B) return;                   // whole waves leave; there is no barrier below
  const float *xr = p.x32 + r * p.ldx, *vr = p.v + r * p.ldv;
  double *kr = p.Ks + r * p.ldk;
  const bool hutch = p.aug && !p.q;
  const float *er = hutch ? p.eps + r * p.lde : nullptr, *ur = hutch ? p.u + r * p.ldu : nullptr;
  double acc = 0.0;
  for (int col = lane * 2; col < p.D; col += 128) {
    const bool two = col + 1 < p.D;
    const double k0 = fma(p.a, (double)xr[col], p.b * (double)vr[col]);
    const double k1 = two ? fma(p.a, (double)xr[col + 1], p.b * (double)vr[col + 1]) : 0.0;
    if (VEC && two) {
      *reinterpret_cast<double2 *>(kr + col) = make_double2(k0, k1);
    } else {
      kr[col] = k0;
      if (two) kr[col + 1] = k1;
    }
    if (hutch) {
      acc = fma((double)er[col], (double)ur[col], acc);
      if (two) acc = fma((double)er[col + 1], (double)ur[col + 1], acc);
    }
  }
  if (!p.aug) return;
  if (hutch) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) acc += __shfl_down(acc, s, 64);
  }
  if (lane == 0) kr[p.D] = fma(p.b, hutch ? acc : p.q[r], p.a * (double)p.D);
}

// ---------------------------------------------------------------------------------------------- jvp_trace
// one workgroup per point: a lane owns the 4-column groups lane, lane + 256, ... of the point's [D, N] tangent rows
__global__ void __launch_bounds__(RED_THREADS)
trace_kernel(const float *__restrict__ T, int64_t ldt, int64_t strideT, const float *__restrict__ Wo, int64_t ldw, double *__restrict__ tr,
             int D, int N) {
  __shared__ double sh[RED_THREADS];
  const float *Tp = T + (int64_t)blockIdx.x * strideT;
  const int G = (N + 3) >> 2, total = D * G;
  double acc = 0.0;
  for (int g = threadIdx.x; g < total; g += RED_THREADS) {
    const int i = g / G, n = (g - i * G) * 4, cnt = N - n < 4 ? N - n : 4;
    const float4 tv = *reinterpret_cast<const float4 *>(Tp + (int64_t)i * ldt + n);
    const float4 wv = *reinterpret_cast<const float4 *>(Wo + (int64_t)i * ldw + n);
    acc = fma((double)tv.x, (double)wv.x, acc);
    if (cnt > 1) acc = fma((double)tv.y, (double)wv.y, acc);
    if (cnt > 2) acc = fma((double)tv.z, (double)wv.z, acc);
    if (cnt > 3) acc = fma((double)tv.w, (double)wv.w, acc);
  }
  const double tot = block_sum(acc, sh);
  if (threadIdx.x == 0) tr[blockIdx.x] = tot;
}

bool even_pitches(int64_t a, int64_t b, int64_t c) { return !((a | b | c) & 1); }

}  // namespace

IDIFF_API int idiff_rk_stage_f64(const double *y, int64_t ldy, const double *K, int64_t ldk, int64_t strideK, const double *c, int ns,
                                 double *y_out, int64_t ldyo, float *x32, int64_t ldx, int64_t B, int D, int aug, float label_value,
                                 void *stream) {
  if (B < 0 || D < 1 || aug < 0 || aug > 1) return fail("rk_stage: B = %lld, D = %d, aug = %d: needs B >= 0, D >= 1, aug 0 or 1", (long long)B, D, aug);
  if (ns < 0 || ns > MAX_STAGES - 1) return fail("rk_stage: ns = %d stages (0 .. %d served)", ns, MAX_STAGES - 1);
  if (!y || !K || !x32 || (ns > 0 && !c)) return fail("rk_stage: null pointer");
  const int W = D + aug;
  if (ldy < W || ldk < W || (y_out && ldyo < W)) return fail("rk_stage: a row pitch is shorter than a row of %d doubles (y %lld, K %lld, y_out %lld)", W, (long long)ldy, (long long)ldk, (long long)ldyo);
  if (ldx < D + 1) return fail("rk_stage: ldx = %lld leaves no column %d for the time label", (long long)ldx, D);
  if (ns > 1 && strideK < (B - 1) * ldk + W) return fail("rk_stage: strideK = %lld is shorter than a stage of %lld rows", (long long)strideK, (long long)B);
  if (((uintptr_t)y & 7) || ((uintptr_t)K & 7) || ((uintptr_t)y_out & 7) || ((uintptr_t)x32 & 3))
    return fail("rk_stage: y, K and y_out must be 8-byte aligned, x32 4-byte");
  if (B == 0) return 0;
  StageP p = {y, K, y_out, x32, ldy, ldk, strideK, ldyo, ldx, B, D, W, ns, label_value, {}};
  for (int j = 0; j < ns; ++j) p.c.c[j] = c[j];
  const bool vec = !(((uintptr_t)y | (uintptr_t)K | (uintptr_t)y_out) & 15) && even_pitches(ldy, ldk, strideK) && !(ldyo & 1);
  const int grid = streaming_grid(B * (int64_t)((W + 1) / 2), 256);
  if (vec)
    hipLaunchKernelGGL(stage_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
  else
    hipLaunchKernelGGL(stage_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
  return launch_status("rk_stage");
}

IDIFF_API int idiff_rk_error_f64(const double *K, int64_t ldk, int64_t strideK, const double *e, const double *y, int64_t ldy,
                                 const double *y_new, int64_t ldyn, int64_t B, int W, double atol, double rtol, double *ws, double *out,
                                 void *stream) {
  if (B < 0 || W < 1) return fail("rk_error: B = %lld, W = %d: needs B >= 0, W >= 1", (long long)B, W);
  if (!K || !e || !y || !y_new || !ws || !out) return fail("rk_error: null pointer");
  if (ldk < W || ldy < W || ldyn < W) return fail("rk_error: a row pitch is shorter than a row of %d doubles (K %lld, y %lld, y_new %lld)", W, (long long)ldk, (long long)ldy, (long long)ldyn);
  if (strideK < (B - 1) * ldk + W) return fail("rk_error: strideK = %lld is shorter than a stage of %lld rows", (long long)strideK, (long long)B);
  if (((uintptr_t)K & 7) || ((uintptr_t)y & 7) || ((uintptr_t)y_new & 7) || ((uintptr_t)ws & 7) || ((uintptr_t)out & 7))
    return fail("rk_error: every pointer must be 8-byte aligned");
  if (!(atol >= 0.0) || !(rtol >= 0.0)) return fail("rk_error: atol = %g, rtol = %g must not be negative", atol, rtol);
  if (B == 0) return 0;
  const int64_t total = B * (int64_t)W;
  int64_t nb = ceil_div64(total, 4 * RED_THREADS);
  if (nb > IDIFF_REDUCE_WS_DOUBLES) nb = IDIFF_REDUCE_WS_DOUBLES;
  const int64_t per = ceil_div64(total, nb);
  const int blocks = (int)ceil_div64(total, per);
  ErrorP p = {K, y, y_new, ws, ldk, strideK, ldy, ldyn, total, per, W, atol, rtol, {}};
  for (int j = 0; j < MAX_STAGES; ++j) p.e.c[j] = e[j];
  hipLaunchKernelGGL(error_partial_kernel, dim3(blocks), dim3(RED_THREADS), 0, (hipStream_t)stream, p);
  hipLaunchKernelGGL(error_final_kernel, dim3(1), dim3(RED_THREADS), 0, (hipStream_t)stream, (const double *)ws, blocks, out);
  return launch_status("rk_error");
}

IDIFF_API int idiff_flow_rhs_f64(const float *x32, int64_t ldx, const float *v, int64_t ldv, double a, double b, double *Ks, int64_t ldk,
                                 int64_t B, int D, int aug, const float *eps, int64_t lde, const float *u, int64_t ldu, const double *q,
                                 void *stream) {
  if (B < 0 || D < 1 || aug < 0 || aug > 1) return fail("flow_rhs: B = %lld, D = %d, aug = %d: needs B >= 0, D >= 1, aug 0 or 1", (long long)B, D, aug);
  if (!x32 || !v || !Ks) return fail("flow_rhs: null pointer");
  if (aug && !q && (!eps || !u)) return fail("flow_rhs: aug = 1 needs q, or eps and u");
  if (aug && q && (eps || u)) return fail("flow_rhs: pass q, or eps and u, not both");
  if (ldx < D || ldv < D || ldk < D + aug || (eps && lde < D) || (u && ldu < D))
    return fail("flow_rhs: a row pitch is shorter than its row (x32 %lld, v %lld, K %lld, eps %lld, u %lld; D = %d)", (long long)ldx,
                (long long)ldv, (long long)ldk, (long long)lde, (long long)ldu, D);
  if (((uintptr_t)x32 & 3) || ((uintptr_t)v & 3) || ((uintptr_t)eps & 3) || ((uintptr_t)u & 3) || ((uintptr_t)Ks & 7) || ((uintptr_t)q & 7))
    return fail("flow_rhs: x32, v, eps and u must be 4-byte aligned, K and q 8-byte");
  if (ceil_div64(B, 4) > 2147483647LL) return fail("flow_rhs: B = %lld exceeds the grid", (long long)B);
  if (B == 0) return 0;
  RhsP p = {x32, v, aug && !q ? eps : nullptr, aug && !q ? u : nullptr, aug ? q : nullptr, Ks, ldx, ldv, lde, ldu, ldk, B, D, aug, a, b};
  const int grid = (int)ceil_div64(B, 4);
  if (!((uintptr_t)Ks & 15) && !(ldk & 1))
    hipLaunchKernelGGL(rhs_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
  else
    hipLaunchKernelGGL(rhs_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
  return launch_status("flow_rhs");
}

IDIFF_API int idiff_jvp_trace_f64(const float *T, int64_t ldt, int64_t strideT, const float *Wout, int64_t ldw, double *tr, int P, int D,
                                  int N, void *stream) {
  if (P < 0 || D < 1 || N < 1) return fail("jvp_trace: P = %d, D = %d, N = %d: needs P >= 0, D >= 1, N >= 1", P, D, N);
  if (!T || !Wout || !tr) return fail("jvp_trace: null pointer");
  if (((uintptr_t)T & 15) || ((uintptr_t)Wout & 15) || ((uintptr_t)tr & 7)) return fail("jvp_trace: T and Wout must be 16-byte aligned, tr 8-byte");
  const int64_t N4 = ((int64_t)N + 3) / 4 * 4;
  if ((ldt & 3) || (ldw & 3) || (strideT & 3) || ldt < N4 || ldw < N4)
    return fail("jvp_trace: ldt = %lld, ldw = %lld, strideT = %lld must be multiples of 4 floats and the pitches at least %lld", (long long)ldt,
                (long long)ldw, (long long)strideT, (long long)N4);
  if (P > 1 && strideT < (int64_t)(D - 1) * ldt + N4) return fail("jvp_trace: strideT = %lld is shorter than a point of %d rows", (long long)strideT, D);
  if ((int64_t)D * (N4 / 4) > 2147483647LL) return fail("jvp_trace: D = %d, N = %d exceeds the index range", D, N);
  if (P == 0) return 0;
  hipLaunchKernelGGL(trace_kernel, dim3(P), dim3(RED_THREADS), 0, (hipStream_t)stream, T, ldt, strideT, Wout, ldw, tr, D, N);
  return launch_status("jvp_trace");
}
