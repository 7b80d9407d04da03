// Jacobian of the fcn score network (models/fcn.py) in forward mode: the D input directions of a point are pushed through the layers as D
// tangent rows.  With a_l[p] the ELU output of layer l at point p and g(a) = a > 0 ? 1 : a + 1 (ELU' written in the output, as gemm_nn has it)
//
//   jvp_seed    T[p][i, n] = W1[n, i] g(a_1[p, n])                          the first layer: the tangent of input i is column i of W1
//   jvp_layer   C[p][r, n] = (sum_k A[p][r, k] W[n, k]) g(a_l[p, n])        every further layer; act = NULL (no factor) for the output layer
//
// The factor belongs to a (point, column) pair and is the same for all rows of a point, so a workgroup's row tile never leaves its point
// (grid = column tiles x row tiles x points): g is one vector per tile, read once and applied to the accumulators in registers.
//
// jvp_layer runs on v_mfma_f32_32x32x2_f32 like csrc/fcn_train.hip: a k-ordered chain of fp32 fmas, one rounding per product, K never split,
// no atomics, no workspace -- the same bits on every run, and a point's bits do not depend on the other points of the launch.  One workgroup
// of four waves owns a 128 x 128 tile of one point's C (a point has D <= 128 tangent rows in every config of the paper: one row tile, and the
// weight panel is read once per point); each wave owns 64 x 64 of it as 2 x 2 accumulators of 32 x 32 and walks K in steps of 32.  Both
// operands are K-contiguous in memory and K-MAJOR in LDS (tile[k][m], the instruction's lane map: lane l holds A[m = l & 31][k = l >> 5]), so
// both are transposed on their way in: eight lanes read one row's 128 bytes of the K step as float4, and each lane writes its four floats to
// four LDS rows.  With a pitch of 129 floats (4 * 129 = 4 mod 32 banks) the 32 lanes of a write group -- four rows m, eight k quads -- fall on
// 32 different banks; a wave's operand read is two runs of 32 consecutive floats.  The next K step's global loads are issued before the
// current step's MFMAs.
//
// jvp_seed is a transposed copy with a factor: a workgroup stages a 64 (n) x 64 (i) tile of W1 through LDS once (read as float4 along i, the
// contiguous side), keeps its 16 elements per lane in registers, and walks the points, one fp32 multiply and one float4 store along n each.
#include "common.h"

namespace {
using namespace idiff;

typedef float floatx16 __attribute__((ext_vector_type(16)));

constexpr int BM = 128, BN = 128, BK = 32, THREADS = 256, PITCH = 129;
constexpr int ST = 64, SPITCH = 65;           // jvp_seed: tile edge and its LDS pitch
constexpr int GRID_Z = 65535;

struct LayerP {
  const float *A, *W, *act;
  float *C;
  int64_t lda, strideA, ldw, ld_act, ldc, strideC;
  int R, N, K;
};

struct SeedP {
  const float *W1, *act;
  float *T;
  int64_t ldw, ld_act, ldt, strideT;
  int P, D, N;
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

__device__ __forceinline__ float elu_slope(float a) { return a > 0.f ? 1.f : a + 1.f; }

__global__ void __launch_bounds__(THREADS) jvp_layer_kernel(LayerP p) {
  __shared__ __attribute__((aligned(16))) float As[BK * PITCH];
  __shared__ __attribute__((aligned(16))) float Ws[BK * PITCH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  const int wm = (wave & 1) * 64, wn = (wave >> 1) * 64;
  const float *A = p.A + (int64_t)blockIdx.z * p.strideA;
  float *C = p.C + (int64_t)blockIdx.z * p.strideC;
  floatx16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  float4 ra[4], rw[4];

  // a tile is 128 rows of 8 float4: lane idx & 7 takes the k quad, idx >> 3 the row
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int idx = tid + THREADS * i;
      const int m = idx >> 3, k4 = (idx & 7) * 4;
      ra[i] = load4(A, p.lda, m0 + m, p.R, k0 + k4, p.K);
      rw[i] = load4(p.W, p.ldw, n0 + m, p.N, k0 + k4, p.K);
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int idx = tid + THREADS * i;
      const int m = idx >> 3, k4 = (idx & 7) * 4;
      As[(k4 + 0) * PITCH + m] = ra[i].x;
      As[(k4 + 1) * PITCH + m] = ra[i].y;
      As[(k4 + 2) * PITCH + m] = ra[i].z;
      As[(k4 + 3) * PITCH + m] = ra[i].w;
      Ws[(k4 + 0) * PITCH + m] = rw[i].x;
      Ws[(k4 + 1) * PITCH + m] = rw[i].y;
      Ws[(k4 + 2) * PITCH + m] = rw[i].z;
      Ws[(k4 + 3) * PITCH + m] = rw[i].w;
    }
  };

  fetch(0);
  const float *ap = As + (lane >> 5) * PITCH + wm + (lane & 31);
  const float *wp = Ws + (lane >> 5) * PITCH + wn + (lane & 31);
  for (int k0 = 0; k0 < p.K; k0 += BK) {
    stage();
    __syncthreads();
    if (k0 + BK < p.K) fetch(k0 + BK);
#pragma unroll
    for (int kk = 0; kk < BK; kk += 2) {
      const float a0 = ap[kk * PITCH], a1 = ap[kk * PITCH + 32];
      const float w0 = wp[kk * PITCH], w1 = wp[kk * PITCH + 32];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, w0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, w1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, w0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, w1, acc[1][1], 0, 0, 0);
    }
    __syncthreads();
  }

#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int col = n0 + wn + 32 * j + (lane & 31);
    if (col >= p.N) continue;
    // the tile's factor: one value per column of this point, whatever the row
    const float g = p.act ? elu_slope(p.act[(int64_t)blockIdx.z * p.ld_act + col]) : 1.f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (row >= p.R) continue;
        const float v = acc[i][j][r];
        C[(int64_t)row * p.ldc + col] = p.act ? v * g : v;
      }
    }
  }
}

__global__ void __launch_bounds__(THREADS) jvp_seed_kernel(SeedP p) {
  __shared__ float s[ST * SPITCH];                       // s[i][n]
  const int tid = threadIdx.x;
  const int n0 = blockIdx.x * ST, i0 = blockIdx.y * ST;
  // W1[n0 + n, i0 + 4 q .. + 3] -> s[4 q + j][n]: 64 rows n of 16 float4; columns i >= D (the time column, the pads) are never read
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int idx = tid + THREADS * it;
    const int n = idx >> 4, q4 = (idx & 15) * 4;
    const float4 v = load4(p.W1, p.ldw, n0 + n, p.N, i0 + q4, p.D);
    s[(q4 + 0) * SPITCH + n] = v.x;
    s[(q4 + 1) * SPITCH + n] = v.y;
    s[(q4 + 2) * SPITCH + n] = v.z;
    s[(q4 + 3) * SPITCH + n] = v.w;
  }
  __syncthreads();
  // a lane keeps four quads (rows i = tid >> 4 + 16 e, columns n4 .. n4 + 3) for every point
  const int n4 = (tid & 15) * 4, ib = tid >> 4;
  float w[4][4];
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int c = 0; c < 4; ++c) w[e][c] = s[(ib + 16 * e) * SPITCH + n4 + c];
  const int col = n0 + n4;
  if (col >= p.N) return;
  const bool whole = col + 3 < p.N;
  for (int pt = blockIdx.z; pt < p.P; pt += gridDim.z) {
    const float *a = p.act + (int64_t)pt * p.ld_act + col;
    float g[4] = {1.f, 1.f, 1.f, 1.f};
    if (whole) {
      const float4 v = *reinterpret_cast<const float4 *>(a);
      g[0] = elu_slope(v.x); g[1] = elu_slope(v.y); g[2] = elu_slope(v.z); g[3] = elu_slope(v.w);
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c)
        if (col + c < p.N) g[c] = elu_slope(a[c]);
    }
    float *T = p.T + (int64_t)pt * p.strideT;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int i = i0 + ib + 16 * e;
      if (i >= p.D) continue;
      float *dst = T + (int64_t)i * p.ldt + col;
      if (whole) {
        *reinterpret_cast<float4 *>(dst) = make_float4(w[e][0] * g[0], w[e][1] * g[1], w[e][2] * g[2], w[e][3] * g[3]);
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c)
          if (col + c < p.N) dst[c] = w[e][c] * g[c];
      }
    }
  }
}

bool aligned16(const void *ptr) { return ((uintptr_t)ptr & 15) == 0; }

}  // namespace

IDIFF_API int idiff_jvp_layer_ok(int R, int N, int K) {
  return R >= 1 && N >= 1 && K >= 1 && ceil_div(R, BM) <= 65535 ? 1 : 0;
}

IDIFF_API int idiff_jvp_seed_f32(const float *W1, int64_t ldw, const float *act, int64_t ld_act, float *T, int64_t ldt, int64_t strideT,
                                 int P, int D, int N, void *stream) {
  if (P < 0 || D < 1 || N < 1) return fail("jvp_seed: P = %d, D = %d, N = %d: needs P >= 0 and D, N >= 1", P, D, N);
  if (!W1 || !act || !T) return fail("jvp_seed: null pointer");
  if (!aligned16(W1) || !aligned16(act) || !aligned16(T)) return fail("jvp_seed: W1, act and T must be 16-byte aligned");
  if ((ldw & 3) || (ld_act & 3) || (ldt & 3) || (strideT & 3))
    return fail("jvp_seed: leading dimensions and the point stride must be multiples of 4 floats (ldw %lld, ld_act %lld, ldt %lld, strideT %lld)",
                (long long)ldw, (long long)ld_act, (long long)ldt, (long long)strideT);
  if (ldw < D || ld_act < N || ldt < N)
    return fail("jvp_seed: a leading dimension is shorter than its row (ldw %lld < D %d, ld_act %lld or ldt %lld < N %d)", (long long)ldw, D,
                (long long)ld_act, (long long)ldt, N);
  if (P > 1 && strideT < (int64_t)(D - 1) * ldt + N)
    return fail("jvp_seed: strideT = %lld is shorter than one point's [%d, %lld] block", (long long)strideT, D, (long long)ldt);
  if (ceil_div(D, ST) > 65535) return fail("jvp_seed: D = %d exceeds the grid (at most %d input directions)", D, 65535 * ST);
  if (P == 0) return 0;
  SeedP p = {W1, act, T, ldw, ld_act, ldt, strideT, P, D, N};
  const int64_t tiles = (int64_t)ceil_div(N, ST) * ceil_div(D, ST);
  // enough workgroups to fill the chip; the rest of the points are a loop over one staged tile
  int64_t pz = ceil_div64(2048, tiles);
  if (pz > P) pz = P;
  if (pz > GRID_Z) pz = GRID_Z;
  hipLaunchKernelGGL(jvp_seed_kernel, dim3(ceil_div(N, ST), ceil_div(D, ST), (unsigned)pz), dim3(THREADS), 0, (hipStream_t)stream, p);
  return launch_status("jvp_seed");
}

IDIFF_API int idiff_jvp_layer_f32(const float *A, int64_t lda, int64_t strideA, const float *W, int64_t ldw, const float *act,
                                  int64_t ld_act, float *C, int64_t ldc, int64_t strideC, int P, int R, int N, int K, void *stream) {
  if (P < 0 || R < 1 || N < 1 || K < 1) return fail("jvp_layer: P = %d, R = %d, N = %d, K = %d: needs P >= 0 and R, N, K >= 1", P, R, N, K);
  if (!A || !W || !C) return fail("jvp_layer: null pointer");
  if (!aligned16(A) || !aligned16(W) || !aligned16(C) || !aligned16(act)) return fail("jvp_layer: A, W, act and C must be 16-byte aligned");
  if ((lda & 3) || (ldw & 3) || (ldc & 3) || (strideA & 3) || (strideC & 3) || (act && (ld_act & 3)))
    return fail("jvp_layer: leading dimensions and point strides must be multiples of 4 floats (lda %lld, ldw %lld, ldc %lld, ld_act %lld, "
                "strideA %lld, strideC %lld)", (long long)lda, (long long)ldw, (long long)ldc, (long long)ld_act, (long long)strideA,
                (long long)strideC);
  if (lda < K || ldw < K || ldc < N || (act && ld_act < N))
    return fail("jvp_layer: a leading dimension is shorter than its row (lda %lld, ldw %lld < K %d, or ldc %lld, ld_act %lld < N %d)",
                (long long)lda, (long long)ldw, K, (long long)ldc, (long long)ld_act, N);
  if (strideA < 0 || (P > 1 && strideC < (int64_t)(R - 1) * ldc + N))
    return fail("jvp_layer: strideA = %lld is negative or strideC = %lld is shorter than one point's [%d, %lld] block", (long long)strideA,
                (long long)strideC, R, (long long)ldc);
  if (!idiff_jvp_layer_ok(R, N, K)) return fail("jvp_layer: R = %d exceeds the grid (at most %d rows a point)", R, 65535 * BM);
  if (P == 0) return 0;
  for (int p0 = 0; p0 < P; p0 += GRID_Z) {
    const int np = P - p0 < GRID_Z ? P - p0 : GRID_Z;
    LayerP p = {A + (int64_t)p0 * strideA, W, act ? act + (int64_t)p0 * ld_act : nullptr, C + (int64_t)p0 * strideC,
                lda, strideA, ldw, ld_act, ldc, strideC, R, N, K};
    hipLaunchKernelGGL(jvp_layer_kernel, dim3(ceil_div(N, BN), ceil_div(R, BM), np), dim3(THREADS), 0, (hipStream_t)stream, p);
  }
  return launch_status("jvp_layer");
}
