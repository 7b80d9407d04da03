// Exact score of a noised union of k-spheres (models/ksphere_union_exact.py), one launch, fp64 from the projection to the final rounding.
//
// Component j: radius R_j, orthonormal frame Q_j [n, p_j] (columns off_j .. off_j + p_j of Qcat [n, P]), weight pi_j.  For a row x at noise
// level sigma, with a_j = Q_j^T x, r_j = |a_j|, kappa_j = r_j R_j / sigma^2, nu_j = p_j / 2 - 1 and the Hankel series
// H_nu(kappa) = sum_{m < 64} (-1)^m prod_{i <= m} (4 nu^2 - (2 i - 1)^2) / (m! (8 kappa)^m):
//
//   E_j  = log pi_j + lgamma(p_j / 2) - R_j^2 / (2 sigma^2) + nu_j log(2 / kappa_j) + kappa_j - log(2 pi kappa_j) / 2 + log H_nu_j(kappa_j)
//   w    = softmax_j(E_j),   A_j = H_{nu_j + 1}(kappa_j) / H_nu_j(kappa_j)
//   out  = mult (-x + sum_j w_j (R_j A_j / r_j) Q_j a_j)
//
// The series is used where kappa_j >= kmin_j = max(32, p_j^2 / 16) only.  A component below that is never guessed: it is bounded by
// U_j = log pi_j + kappa_j - R_j^2 / (2 sigma^2) >= E_j, and where U_j < max(exact E) - 800 its weight is exactly 0 in fp64.  A row with
// no exact component, or with a bounded one that is not that far down, is REFUSED: written as NaN and counted.
//
// One wave owns 16 rows at a time.  Qcat lives in LDS (one copy per workgroup, rows `Pst` doubles apart, Pst = 2 mod 16, which keeps
// the 16 x 2 doubles a half wave reads for either operand shape on 32 distinct bank pairs); the wave's x tile, its a tile and the per-row
// scalars live in LDS areas of its own, so a wave never waits for another one after the frames are loaded: while one wave waits for HBM the
// others of the CU compute.  Both products run on v_mfma_f64_16x16x4_f64 (lane l supplies A[l & 15][l >> 4] and B[l >> 4][l & 15], register
// r of lane l is C[(l >> 4) + 4 r][l & 15]):
//   a [16, P]   = x [16, n] Qcat [n, P]          (x converted to fp64 on the way into the A operand)
//   y [16, n]   = (g a) [16, P] Qcat^T [P, n]    (g_j = w_j R_j A_j / r_j per row and component, applied to the a tile in LDS)
// The 2 J series of a row are spread over lanes (row, component, nu / nu + 1): 64 lanes are busy at J = 2.  x is read once (coalesced,
// through the wave's LDS tile) and out written once (from the same tile).
#include "common.h"

#include <math.h>

using namespace idiff;

namespace {

typedef double doublex4 __attribute__((ext_vector_type(4)));

constexpr int J_MAX = 8;             // components
constexpr int P_MAX = 128;           // widest frame (k + 1)
constexpr int ROWS = 16;             // rows of x per wave tile
constexpr int CB = 4;                // 16-column blocks of the output a wave accumulates at a time (16 accumulator registers each)
constexpr int WAVES_MAX = 8;
constexpr int TERMS = 63;            // terms of the Hankel series after the leading 1
constexpr int LDS_MAX = 160 * 1024;  // LDS of a CU
constexpr int SMALL = 4 * ROWS * J_MAX + ROWS;   // doubles per wave: kappa -> g, r, (E | A) pairs, the refusal flag

struct Comp { int off, p; double R, lp, c0, nu, kmin; };

struct UnionParams {
  const float *x; const double *Q; const float *sigma; const float *mult; float *out; int *refused;
  int B, n, J, P;
  int n4, P16, Pst;       // n rounded up to 4; P rounded up to 16; row pitch of the frames and of the a tile in LDS
  int waves, vec, tiles;  // waves per workgroup; 16-byte accesses to x / out; 16-row tiles
  int wave_bytes;
  Comp comp[J_MAX];
};

inline int round_up(int a, int b) { return (a + b - 1) / b * b; }
inline int frame_pitch(int P) { return round_up(P, 16) + 2; }
inline int wave_bytes_of(int n, int P) { return (ROWS * frame_pitch(P) + SMALL) * 8 + ROWS * round_up(n, 4) * 4; }
inline int64_t shared_bytes_of(int n, int P) { return (int64_t)n * frame_pitch(P) * 8 + J_MAX * (5 * 8 + 2 * 4); }
// waves that fit beside the frames (0: the shape is refused)
inline int waves_of(int n, int P) {
  const int64_t left = LDS_MAX - shared_bytes_of(n, P);
  if (left <= 0) return 0;
  const int64_t w = left / wave_bytes_of(n, P);
  return (int)(w > WAVES_MAX ? WAVES_MAX : w);
}

__device__ __forceinline__ doublex4 mfma(double a, double b, doublex4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// LDS handed from lane to lane of ONE wave: its ds instructions complete in order, the compiler may not move them across this point
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ double hankel(double nu, double kappa) {
  const double mu = 4.0 * nu * nu, inv = 1.0 / (8.0 * kappa);
  double term = 1.0, sum = 1.0;
#pragma unroll
  for (int m = 1; m <= TERMS; ++m) {
    const double odd = (double)((2 * m - 1) * (2 * m - 1));
    term *= (odd - mu) * (inv * (1.0 / m));
    sum += term;
  }
  return sum;
}

constexpr int KU = 4;                // k steps whose operands are read from LDS before the first of their products is issued

// KU steps of NB products each: all operands first (one exposed LDS latency per KU * NB products), then the products in k order
template <int NB, int KU_>
__device__ __forceinline__ void project_steps(doublex4 (&acc)[NB], const float *x_lane, const double *q, int k0, int n, int Pst, int l4) {
  double a[KU_], b[KU_][NB];
#pragma unroll
  for (int s = 0; s < KU_; ++s) {
    const int k = k0 + 4 * s + l4;
    const int qrow = k < n ? k : n - 1;                            // past n the x operand is zero
    a[s] = (double)x_lane[k];
#pragma unroll
    for (int u = 0; u < NB; ++u) b[s][u] = q[qrow * Pst + u * 16];
  }
#pragma unroll
  for (int s = 0; s < KU_; ++s)
#pragma unroll
    for (int u = 0; u < NB; ++u) acc[u] = mfma(a[s], b[s][u], acc[u]);
}

// NB 16-column blocks of a = x Qcat for the wave's 16 rows: q and a_out point at this lane's column of the first block
template <int NB>
__device__ __forceinline__ void project(const float *xs, const double *q, double *a_out, int n, int n4, int Pst, int l15, int l4) {
  doublex4 acc[NB];
#pragma unroll
  for (int u = 0; u < NB; ++u) acc[u] = doublex4{0.0, 0.0, 0.0, 0.0};
  const float *x_lane = xs + l15 * n4;
  int k0 = 0;
  for (; k0 + 4 * KU <= n4; k0 += 4 * KU) project_steps<NB, KU>(acc, x_lane, q, k0, n, Pst, l4);
  for (; k0 < n4; k0 += 4) project_steps<NB, 1>(acc, x_lane, q, k0, n, Pst, l4);
#pragma unroll
  for (int u = 0; u < NB; ++u)
#pragma unroll
    for (int r = 0; r < 4; ++r) a_out[(l4 + 4 * r) * Pst + u * 16] = acc[u][r];
}

template <int NB, int KU_>
__device__ __forceinline__ void back_steps(doublex4 (&acc)[NB], const double *a_lane, const double *const (&q)[NB], int k0) {
  double a[KU_], b[KU_][NB];
#pragma unroll
  for (int s = 0; s < KU_; ++s) {
    a[s] = a_lane[k0 + 4 * s];
#pragma unroll
    for (int u = 0; u < NB; ++u) b[s][u] = q[u][k0 + 4 * s];
  }
#pragma unroll
  for (int s = 0; s < KU_; ++s)
#pragma unroll
    for (int u = 0; u < NB; ++u) acc[u] = mfma(a[s], b[s][u], acc[u]);
}

// NB 16-column blocks, from block c0, of y = (g a) Qcat^T and out = mult (-x + y), rounded once, into the x tile
template <int NB>
__device__ __forceinline__ void back_project(const double *as, const double *qs, float *xs, int c0, int n, int n4, int P16, int Pst, int l15,
                                             int l4, const double (&mrow)[4], const bool (&brow)[4]) {
  doublex4 acc[NB];
  const double *q[NB];
#pragma unroll
  for (int u = 0; u < NB; ++u) {
    acc[u] = doublex4{0.0, 0.0, 0.0, 0.0};
    const int i = (c0 + u) * 16 + l15;
    q[u] = qs + (i < n ? i : n - 1) * Pst + l4;                    // columns past n are computed and dropped
  }
  const double *a_lane = as + l15 * Pst + l4;
  int k0 = 0;                                                      // P16 / 4 steps: a multiple of KU = 4
  for (; k0 + 4 * KU <= P16; k0 += 4 * KU) back_steps<NB, KU>(acc, a_lane, q, k0);
  for (; k0 < P16; k0 += 4) back_steps<NB, 1>(acc, a_lane, q, k0);
#pragma unroll
  for (int u = 0; u < NB; ++u) {
    const int col = (c0 + u) * 16 + l15;
    if (col < n) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int at = (l4 + 4 * r) * n4 + col;
        const double v = mrow[r] * (acc[u][r] - (double)xs[at]);
        xs[at] = brow[r] ? __int_as_float(0x7fc00000) : (float)v;
      }
    }
  }
}

__global__ void __launch_bounds__(64 * WAVES_MAX)
ksphere_union_kernel(const UnionParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = p.n, n4 = p.n4, P = p.P, P16 = p.P16, Pst = p.Pst, J = p.J;
  double *qs = reinterpret_cast<double *>(smem);                 // [n][Pst]
  double *cd = qs + (int64_t)n * Pst;                            // [J_MAX][5]: R, log pi, c0, nu, kmin
  int *ci = reinterpret_cast<int *>(cd + J_MAX * 5);             // [J_MAX][2]: off, p
  unsigned char *mine = reinterpret_cast<unsigned char *>(ci + J_MAX * 2) + (int64_t)wave * p.wave_bytes;
  double *as = reinterpret_cast<double *>(mine);                 // [ROWS][Pst]
  double *kap = as + ROWS * Pst;                                 // [ROWS][J_MAX]   kappa, then g
  double *rr = kap + ROWS * J_MAX;                               // [ROWS][J_MAX]   r
  double *hh = rr + ROWS * J_MAX;                                // [ROWS][J_MAX][2]   (E or U, A)
  double *fl = hh + ROWS * J_MAX * 2;                            // [ROWS]   1 = refused
  float *xs = reinterpret_cast<float *>(fl + ROWS);              // [ROWS][n4]

  for (int e = tid; e < n * Pst; e += blockDim.x) {
    const int i = e / Pst, c = e - i * Pst;
    qs[e] = c < P ? p.Q[(int64_t)i * P + c] : 0.0;
  }
#pragma unroll
  for (int j = 0; j < J_MAX; ++j)
    if (tid == j) {
      cd[j * 5 + 0] = p.comp[j].R; cd[j * 5 + 1] = p.comp[j].lp; cd[j * 5 + 2] = p.comp[j].c0; cd[j * 5 + 3] = p.comp[j].nu;
      cd[j * 5 + 4] = p.comp[j].kmin;
      ci[j * 2] = p.comp[j].off; ci[j * 2 + 1] = p.comp[j].p;
    }
  __syncthreads();

  const int l15 = lane & 15, l4 = lane >> 4;
  const int nblk_p = P16 / 16, nblk_n = (n + 15) / 16;
  int refused = 0;

  for (int tile = blockIdx.x * p.waves + wave; tile < p.tiles; tile += gridDim.x * p.waves) {
    const int row0 = tile * ROWS;
    const int valid = p.B - row0 < ROWS ? p.B - row0 : ROWS;
    const float *gx = p.x + (int64_t)row0 * n;
    float *go = p.out + (int64_t)row0 * n;

    // ---- 1. the tile of x into LDS (rows past the batch and columns past n: zero)
    if (p.vec) {                                                 // n % 4 == 0: n4 == n, 16 bytes never straddle a row
      for (int e = lane * 4; e < ROWS * n; e += 256) {
        const int row = e / n;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row < valid) v = *reinterpret_cast<const float4 *>(gx + e);
        *reinterpret_cast<float4 *>(xs + e) = v;
      }
    } else {
      for (int e = lane; e < ROWS * n4; e += 64) {
        const int row = e / n4, col = e - row * n4;
        xs[e] = (row < valid && col < n) ? gx[row * n + col] : 0.f;
      }
    }
    wave_lds_sync();

    // ---- 2. a = x Qcat
    for (int c0 = 0; c0 < nblk_p; c0 += CB) {
      const double *q = qs + c0 * 16 + l15;
      double *a_out = as + c0 * 16 + l15;
      switch (nblk_p - c0) {                                       // wave-uniform: the loops inside carry no branch
        case 1: project<1>(xs, q, a_out, n, n4, Pst, l15, l4); break;
        case 2: project<2>(xs, q, a_out, n, n4, Pst, l15, l4); break;
        case 3: project<3>(xs, q, a_out, n, n4, Pst, l15, l4); break;
        default: project<CB>(xs, q, a_out, n, n4, Pst, l15, l4); break;
      }
    }
    wave_lds_sync();

    // ---- 3. r and kappa, one lane per (row, component)
    for (int idx = lane; idx < ROWS * J; idx += 64) {
      const int row = idx & 15, j = idx >> 4;
      const int off = ci[j * 2], pj = ci[j * 2 + 1];
      double s = 0.0;
      for (int c = 0; c < pj; ++c) {
        const double v = as[row * Pst + off + c];
        s = fma(v, v, s);
      }
      const double r = sqrt(s);
      const double sg = row < valid ? (double)p.sigma[row0 + row] : 1.0;
      kap[row * J_MAX + j] = r * cd[j * 5 + 0] / (sg * sg);
      rr[row * J_MAX + j] = r;
    }
    wave_lds_sync();

    // ---- 4. the two series of every (row, component): lane bit 4 selects nu or nu + 1
    for (int idx = lane; idx < (2 * ROWS * J + 63) / 64 * 64; idx += 64) {
      const int row = idx & 15, s = (idx >> 4) & 1, j = idx >> 5;
      const int jj = j < J ? j : J - 1;                          // every lane takes part in the exchange below
      const double kappa = kap[row * J_MAX + jj];
      const double nu = cd[jj * 5 + 3];
      const double H = hankel(nu + (double)s, kappa);
      const double Hother = __shfl_xor(H, 16, 64);
      if (j < J) {
        if (s == 0) {
          const double sg = row < valid ? (double)p.sigma[row0 + row] : 1.0;
          const double R = cd[j * 5 + 0];
          const double half = R * R / (2.0 * (sg * sg));
          double e;
          if (kappa >= cd[j * 5 + 4])
            e = cd[j * 5 + 2] - half + nu * log(2.0 / kappa) + kappa - 0.5 * log(6.283185307179586 * kappa) + log(H);
          else
            e = cd[j * 5 + 1] + kappa - half;                    // the bound U
          hh[(row * J_MAX + j) * 2] = e;
        } else {
          hh[(row * J_MAX + j) * 2 + 1] = H / Hother;            // H_{nu + 1} / H_nu
        }
      }
    }
    wave_lds_sync();

    // ---- 5. weights, refusal and g, one lane per row
    if (lane < ROWS) {
      const int row = lane;
      double top = -INFINITY;
      bool any = false;
      for (int j = 0; j < J; ++j)
        if (kap[row * J_MAX + j] >= cd[j * 5 + 4]) {
          top = fmax(top, hh[(row * J_MAX + j) * 2]);
          any = true;
        }
      bool bad = !any;
      double Z = 0.0;
      for (int j = 0; j < J; ++j) {
        const double e = hh[(row * J_MAX + j) * 2];
        if (kap[row * J_MAX + j] >= cd[j * 5 + 4]) Z += exp(e - top);
        else if (!(e < top - 800.0)) bad = true;
      }
      for (int j = 0; j < J; ++j) {
        double g = 0.0;
        if (kap[row * J_MAX + j] >= cd[j * 5 + 4])
          g = exp(hh[(row * J_MAX + j) * 2] - top) / Z * cd[j * 5 + 0] * hh[(row * J_MAX + j) * 2 + 1] / rr[row * J_MAX + j];
        kap[row * J_MAX + j] = g;
      }
      fl[row] = bad ? 1.0 : 0.0;
      if (bad && row < valid) ++refused;
    }
    wave_lds_sync();

    // ---- 6. a <- g a
    for (int j = 0; j < J; ++j) {
      const int off = ci[j * 2], pj = ci[j * 2 + 1];
      for (int e = lane; e < ROWS * pj; e += 64) {
        const int row = e & 15, c = e >> 4;
        as[row * Pst + off + c] *= kap[row * J_MAX + j];
      }
    }
    wave_lds_sync();

    // ---- 7. y = (g a) Qcat^T and out = mult (-x + y), rounded once, into the x tile
    double mrow[4];
    bool brow[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = l4 + 4 * r;
      mrow[r] = row < valid ? (p.mult ? (double)p.mult[row0 + row] : 1.0) : 0.0;
      brow[r] = fl[row] != 0.0;
    }
    for (int c0 = 0; c0 < nblk_n; c0 += CB) {
      switch (nblk_n - c0) {
        case 1: back_project<1>(as, qs, xs, c0, n, n4, P16, Pst, l15, l4, mrow, brow); break;
        case 2: back_project<2>(as, qs, xs, c0, n, n4, P16, Pst, l15, l4, mrow, brow); break;
        case 3: back_project<3>(as, qs, xs, c0, n, n4, P16, Pst, l15, l4, mrow, brow); break;
        default: back_project<CB>(as, qs, xs, c0, n, n4, P16, Pst, l15, l4, mrow, brow); break;
      }
    }
    wave_lds_sync();

    // ---- 8. the tile of out
    if (p.vec) {
      for (int e = lane * 4; e < valid * n; e += 256) *reinterpret_cast<float4 *>(go + e) = *reinterpret_cast<const float4 *>(xs + e);
    } else {
      for (int e = lane; e < valid * n4; e += 64) {
        const int row = e / n4, col = e - row * n4;
        if (col < n) go[row * n + col] = xs[e];
      }
    }
    wave_lds_sync();                                             // before the next tile overwrites the areas
  }
  if (refused) atomicAdd(p.refused, refused);
}

int shape_status(int n, int J, int P) {
  if (J < 1 || J > J_MAX) return fail("ksphere_union: %d components (1 to %d)", J, J_MAX);
  if (P < J || P > J * P_MAX) return fail("ksphere_union: %d frame columns for %d components of at most %d each", P, J, P_MAX);
  if (n < 1) return fail("ksphere_union: n = %d", n);
  if (shared_bytes_of(n, P) >= LDS_MAX || waves_of(n, P) < 2)
    return fail("ksphere_union: n = %d, P = %d: the frames and two waves' tiles do not fit the LDS (ask idiff_ksphere_union_ok)", n, P);
  return 0;
}

}  // namespace

IDIFF_API int idiff_ksphere_union_ok(int n, int J, int P) {
  if (J < 1 || J > J_MAX || P < J || P > J * P_MAX || n < 1) return 0;
  return shared_bytes_of(n, P) < LDS_MAX && waves_of(n, P) >= 2 ? 1 : 0;
}

IDIFF_API int idiff_ksphere_union_score_f32(const float *x, const double *Qcat, const double *comp, const float *sigma, const float *mult,
                                            float *out, int *refused, int B, int n, int J, int P, void *stream) {
  if (B < 0) return fail("ksphere_union: B = %d", B);
  if (int rc = shape_status(n, J, P)) return rc;
  if (!comp) return fail("ksphere_union: null component table");
  UnionParams p = {};
  int next = 0;
  for (int j = 0; j < J; ++j) {
    const double off = comp[4 * j], pj = comp[4 * j + 1], R = comp[4 * j + 2], lp = comp[4 * j + 3];
    if (off != (double)next || !(pj >= 1 && pj <= P_MAX) || pj != (double)(int)pj || next + (int)pj > P)
      return fail("ksphere_union: component %d: columns [%g, %g + %g) -- the frames must tile [0, %d) in order, 1 to %d columns each",
                  j, off, off, pj, P, P_MAX);
    if (pj > n) return fail("ksphere_union: component %d: a frame of %g columns in R^%d", j, pj, n);
    if (!(R > 0.0) || !(R < INFINITY) || !(lp <= 0.0) || !(lp > -INFINITY))
      return fail("ksphere_union: component %d: radius %g, log weight %g", j, R, lp);
    Comp &c = p.comp[j];
    c.off = next; c.p = (int)pj; c.R = R; c.lp = lp;
    c.c0 = lp + lgamma(0.5 * pj);
    c.nu = 0.5 * pj - 1.0;
    c.kmin = pj * pj / 16.0 > 32.0 ? pj * pj / 16.0 : 32.0;
    next += (int)pj;
  }
  if (next != P) return fail("ksphere_union: the components hold %d columns, P = %d", next, P);
  if (B == 0) return 0;
  if (!x || !Qcat || !sigma || !out || !refused) return fail("ksphere_union: null pointer");
  if (((uintptr_t)x & 3) || ((uintptr_t)out & 3) || ((uintptr_t)sigma & 3) || ((uintptr_t)mult & 3) || ((uintptr_t)refused & 3) ||
      ((uintptr_t)Qcat & 7))
    return fail("ksphere_union: x, sigma, mult, out and refused must be 4-byte aligned, Qcat 8-byte aligned");
  p.x = x; p.Q = Qcat; p.sigma = sigma; p.mult = mult; p.out = out; p.refused = refused;
  p.B = B; p.n = n; p.J = J; p.P = P;
  p.n4 = round_up(n, 4); p.P16 = round_up(P, 16); p.Pst = frame_pitch(P);
  p.waves = waves_of(n, P);
  p.vec = (n % 4 == 0 && !((uintptr_t)x & 15) && !((uintptr_t)out & 15)) ? 1 : 0;
  p.tiles = ceil_div(B, ROWS);
  p.wave_bytes = wave_bytes_of(n, P);
  const int lds = (int)(shared_bytes_of(n, P) + (int64_t)p.waves * p.wave_bytes);
  static AttrGuard guard;
  const void *fn = reinterpret_cast<const void *>(ksphere_union_kernel);
  if (int rc = set_dynamic_lds_once(guard, &fn, 1, LDS_MAX, "ksphere_union")) return rc;
  int grid = ceil_div(p.tiles, p.waves);
  if (grid > 256) grid = 256;                                    // one workgroup per CU: each loads the frames once
  hipLaunchKernelGGL(ksphere_union_kernel, dim3(grid), dim3(64 * p.waves), lds, (hipStream_t)stream, p);
  return launch_status("ksphere_union");
}
