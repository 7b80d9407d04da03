// Exact k-nearest neighbours of every row of a point set X [N, D] among the other rows (the kneighbors(X) call of
// mle.py:19-20 / :47-48 / :80-81 of the reference, there on sklearn's CPU ball tree).
//
//   1. centre      c_i = fl32(x_i - mean) (fp64 mean, idiff_colmean_f64), zero-padded to [Np, Dp]; n_i = fl32(||c_i||^2)
//                  and a_i = ||c_i|| from an fp64 sum of the fp32 c_i
//   2. tiles       128 query rows x 128 candidate columns per step: g_ij = c_i . c_j on v_mfma_f32_32x32x2_f32, the
//                  approximate squared distance A_ij = (n_i + n_j) - 2 g_ij, and per row a list of the K' = min(N-1, k+16)
//                  smallest A_ij seen so far (one compare against the list's maximum rejects almost every entry).  When
//                  N / 128 row blocks are too few workgroups for the CUs the columns are split over S workgroups per
//                  row block, each with a list of its own.
//   3. refine      per row: the K' smallest of the S lists, their squared distances again in fp64 from the fp32 X
//                  (sum_d (x_id - x_jd)^2), sorted by (distance, index); the first k are the answer if the margin
//                  test below passes.
//   4. exact pass  rows that fail it are done again by fp64 brute force over all N (one workgroup per row).
//
// Margin (u = 2^-24; s = a_i + a_j).  Every row left out of the candidate set has A_ij >= B, B the K'-th smallest A of
// the row: it was rejected or evicted against a list maximum that never grows, and the S-way merge keeps the K'
// smallest.  The fp32 pass errs by at most
//   centring     c_i - c_j = (x_i - x_j) + e, ||e|| <= u s (1 + u); with ||c_i - c_j|| <= s,
//                | ||c_i - c_j||^2 - ||x_i - x_j||^2 | <= ||e|| (2 s + ||e||) <= 2.01 u s^2
//   norms        n_i, n_j rounded once each: u (n_i + n_j) <= u s^2
//   dot product  MFMA accumulation is a k-ordered fmaf chain; every 32-deep K tile starts from zero and is added to
//                a running fp32 sum, so |g - c_i . c_j| <= gamma a_i a_j <= gamma s^2 / 4 with
//                gamma = 1.01 (32 + T + 4) u, T = Dp / 32 tiles (instead of Dp u for one long chain)
//   combination  two roundings of values <= 2 s^2: 4 u s^2
// so |A_ij - ||x_i - x_j||^2| <= E_i = (gamma / 2 + 80 u) (a_i + a_max)^2 for every j (a_max = max_j a_j, rounded up;
// the 80 u holds the terms above with room, and covers the fp64 rounding of the refined sums, < Dp 2^-53 s^2).
// If the refined k-th squared distance r_k < B - E_i, every row outside the candidates is strictly farther than r_k,
// so the k smallest (distance, index) pairs of the candidates are the k smallest of all N.  Otherwise (or for inputs
// whose norms are large against the neighbour gaps, such as tight clusters far from the mean) the row takes step 4.
// n_exact_rows counts those rows.
#include "common.h"

#include <math.h>

using namespace idiff;

namespace {

typedef float floatx16 __attribute__((ext_vector_type(16)));

constexpr int BM = 128;            // query rows per workgroup
constexpr int BN = 128;            // candidate columns per step
constexpr int KT = 32;             // K depth staged per iteration (and the length of one fmaf chain, see the margin)
constexpr int LDA = KT + 1;        // LDS pitch of a staged row: the 32 rows of an operand fragment hit 32 banks
constexpr int TS = BN + 1;         // LDS pitch of the distance tile
constexpr int KP_MAX = 64 + 16;    // longest candidate list (k <= 64)
constexpr int MAX_SPLITS = 8;
constexpr int EXACT_GRID = 256;    // workgroups of the brute-force pass (each owns N doubles + N ints of workspace)
constexpr int STAGE_BYTES = 2 * BM * LDA * 4;
constexpr int TILE_BYTES = BM * TS * 4;
constexpr int UNION_BYTES = TILE_BYTES > STAGE_BYTES ? TILE_BYTES : STAGE_BYTES;
constexpr double U32 = 5.9604644775390625e-08;   // 2^-24

inline int64_t align256(int64_t b) { return (b + 255) & ~(int64_t)255; }

struct Plan {
  int Np, Dp, KP, S, tiles_per_split, ntiles;
  int64_t off_mean, off_colscr, off_xc, off_nrm, off_arow, off_amax, off_cd, off_ci, off_flag, off_rkd, off_rki, off_sd,
      off_si, total;
};

int cu_count() {
  int dev = 0, c = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 256;
  if (hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || c <= 0) return 256;
  return c;
}

Plan make_plan(int N, int D, int k) {
  Plan p;
  p.Np = ceil_div(N, BM) * BM;
  p.Dp = ceil_div(D, KT) * KT;
  p.KP = N - 1 < k + 16 ? N - 1 : k + 16;
  const int nrb = p.Np / BM;
  p.ntiles = nrb;
  // one workgroup per CU (the lists and the distance tile take most of the LDS): choose the split count whose grid
  // fills the last round of workgroups best, fewest splits among equals
  const int cus = cu_count();
  int best = 1;
  double best_eff = 0.0;
  for (int s = 1; s <= MAX_SPLITS && s <= nrb; ++s) {
    const int64_t blocks = (int64_t)nrb * s;
    const double eff = (double)blocks / (double)(ceil_div64(blocks, cus) * cus);
    if (eff > best_eff + 1e-9) { best_eff = eff; best = s; }
  }
  p.tiles_per_split = ceil_div(nrb, best);
  p.S = ceil_div(nrb, p.tiles_per_split);
  int64_t o = 0;
  auto take = [&](int64_t bytes) { int64_t at = o; o += align256(bytes); return at; };
  p.off_mean = take((int64_t)D * 8);
  p.off_colscr = take((int64_t)32 * D * 8);
  p.off_xc = take((int64_t)p.Np * p.Dp * 4);
  p.off_nrm = take((int64_t)p.Np * 4);
  p.off_arow = take((int64_t)p.Np * 8);
  p.off_amax = take(4);
  p.off_cd = take((int64_t)p.S * N * p.KP * 4);
  p.off_ci = take((int64_t)p.S * N * p.KP * 4);
  p.off_flag = take((int64_t)N * 4);
  p.off_rkd = take((int64_t)N * 8);
  p.off_rki = take((int64_t)N * 4);
  const int G = N < EXACT_GRID ? N : EXACT_GRID;
  p.off_sd = take((int64_t)G * N * 8);
  p.off_si = take((int64_t)G * N * 4);
  p.total = o;
  return p;
}

__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// lexicographic (distance, index) order: ties of distance go to the lower index
template <typename T>
__device__ __forceinline__ bool key_less(T da, int ia, T db, int ib) { return da < db || (da == db && ia < ib); }

// ------------------------------------------------------------------------------------------------ 1. centre
// one wave per (padded) row
__global__ void __launch_bounds__(256)
knn_center_kernel(const float *__restrict__ X, const double *__restrict__ mean, int N, int D, int Dp,
                  float *__restrict__ Xc, float *__restrict__ nrm, double *__restrict__ arow, unsigned *__restrict__ amax_bits) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);     // < Np (Np is a multiple of 128, the grid is Np / 4)
  double acc = 0.0;
  for (int d = lane; d < Dp; d += 64) {
    float c = 0.f;
    if (i < N && d < D) c = (float)((double)X[(int64_t)i * D + d] - mean[d]);
    Xc[(int64_t)i * Dp + d] = c;
    acc += (double)c * (double)c;
  }
  acc = wave_sum(acc);
  if (lane == 0) {
    nrm[i] = (float)acc;
    const double a = sqrt(acc);
    arow[i] = a;
    float af = (float)a;
    if ((double)af < a) af = nextafterf(af, INFINITY);   // rounded up: a_max may only overstate the bound
    atomicMax(amax_bits, __float_as_uint(af));          // non-negative floats order like their bit patterns
  }
}

// ------------------------------------------------------------------------------------------------ 2. tiles
// Workgroup (rb, s): query rows rb*128 .. +127 against the column tiles of split s.  Wave w computes the 64 x 64 quadrant
// (w>>1, w&1) of each 128 x 128 tile as 2 x 2 v_mfma_f32_32x32x2_f32 tiles (lane l feeds A[i = l&31][k = l>>5] and
// B[k = l>>5][j = l&31]; C/D col = l&31, row = (r&3) + 8 (r>>2) + 4 (l>>5)).  The next K tile is loaded into registers
// while the current one is multiplied.  Threads 0..127 own one query row each for the selection; a row's list lives in
// LDS entry-major (entry e of thread t at e * 128 + t: the 128 owners read 128 consecutive words).
__global__ void __launch_bounds__(256)
knn_tiles_kernel(const float *__restrict__ Xc, const float *__restrict__ nrm, int N, int Dp, int KP, int tiles_per_split,
                 int ntiles, float *__restrict__ cand_d, int *__restrict__ cand_i) {
  extern __shared__ float smem[];
  float *As = smem;
  float *Bs = smem + BM * LDA;
  float *Ts = smem;                                   // the distance tile reuses the staging area after the K loop
  float *Ld = smem + UNION_BYTES / 4;
  int *Li = reinterpret_cast<int *>(Ld + BM * KP);
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int wr = (w >> 1) * 64, wc = (w & 1) * 64;
  const int row0 = blockIdx.x * BM, s = blockIdx.y;
  const int my_i = row0 + t;
  const int nk = Dp / KT;
  int cnt = 0, maxpos = 0;
  float thr = INFINITY;
  const int ct_end = min(ntiles, (s + 1) * tiles_per_split);
  for (int ct = s * tiles_per_split; ct < ct_end; ++ct) {
    const int col0 = ct * BN;
    floatx16 master[2][2];
    for (int x = 0; x < 2; ++x)
      for (int y = 0; y < 2; ++y)
        for (int r = 0; r < 16; ++r) master[x][y][r] = 0.f;
    float4 ra[4], rb[4];
    auto load = [&](int k0) {
      for (int q = 0; q < 4; ++q) {
        const int e = t + 256 * q, r = e >> 3, c4 = e & 7;
        ra[q] = *reinterpret_cast<const float4 *>(Xc + (int64_t)(row0 + r) * Dp + k0 + c4 * 4);
        rb[q] = *reinterpret_cast<const float4 *>(Xc + (int64_t)(col0 + r) * Dp + k0 + c4 * 4);
      }
    };
    load(0);
    for (int kt = 0; kt < nk; ++kt) {
      __syncthreads();                                // previous readers of As / Bs / Ts are done
      for (int q = 0; q < 4; ++q) {
        const int e = t + 256 * q, r = e >> 3, c4 = e & 7;
        float *a = As + r * LDA + c4 * 4, *b = Bs + r * LDA + c4 * 4;
        a[0] = ra[q].x; a[1] = ra[q].y; a[2] = ra[q].z; a[3] = ra[q].w;
        b[0] = rb[q].x; b[1] = rb[q].y; b[2] = rb[q].z; b[3] = rb[q].w;
      }
      __syncthreads();
      if (kt + 1 < nk) load((kt + 1) * KT);
      floatx16 acc[2][2];
      for (int x = 0; x < 2; ++x)
        for (int y = 0; y < 2; ++y)
          for (int r = 0; r < 16; ++r) acc[x][y][r] = 0.f;
#pragma unroll
      for (int kk = 0; kk < KT / 2; ++kk) {
        const int kc = 2 * kk + (lane >> 5);
        const float a0 = As[(wr + (lane & 31)) * LDA + kc], a1 = As[(wr + 32 + (lane & 31)) * LDA + kc];
        const float b0 = Bs[(wc + (lane & 31)) * LDA + kc], b1 = Bs[(wc + 32 + (lane & 31)) * LDA + kc];
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
      }
      for (int x = 0; x < 2; ++x)
        for (int y = 0; y < 2; ++y) master[x][y] += acc[x][y];
    }
    __syncthreads();                                  // every wave is done with As / Bs: Ts overwrites them
    for (int x = 0; x < 2; ++x)
      for (int y = 0; y < 2; ++y) {
        const int col = wc + 32 * y + (lane & 31);
        const float nj = nrm[col0 + col];
        for (int r = 0; r < 16; ++r) {
          const int row = wr + 32 * x + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
          Ts[row * TS + col] = (nrm[row0 + row] + nj) - 2.f * master[x][y][r];
        }
      }
    __syncthreads();
    if (t < BM && my_i < N) {
      const int cmax = min(BN, N - col0);
      for (int c = 0; c < cmax; ++c) {
        const int j = col0 + c;
        const float v = Ts[t * TS + c];
        if (j == my_i) continue;
        if (cnt < KP) {
          Ld[cnt * BM + t] = v;
          Li[cnt * BM + t] = j;
          ++cnt;
          if (cnt < KP) continue;
        } else if (v < thr) {
          Ld[maxpos * BM + t] = v;
          Li[maxpos * BM + t] = j;
        } else {
          continue;
        }
        // the list is full and changed: find its new maximum (the rejection threshold never grows)
        thr = Ld[t];
        maxpos = 0;
        for (int e = 1; e < KP; ++e) {
          const float q = Ld[e * BM + t];
          if (q > thr) { thr = q; maxpos = e; }
        }
      }
    }
  }
  if (t < BM && my_i < N) {
    const int64_t base = ((int64_t)s * N + my_i) * KP;
    for (int e = 0; e < KP; ++e) {
      cand_d[base + e] = e < cnt ? Ld[e * BM + t] : INFINITY;
      cand_i[base + e] = e < cnt ? Li[e * BM + t] : -1;
    }
  }
}

// ------------------------------------------------------------------------------------------------ 3. refine
// one workgroup per row
__global__ void __launch_bounds__(256)
knn_refine_kernel(const float *__restrict__ X, int N, int D, int k, int KP, int S, const float *__restrict__ cand_d,
                  const int *__restrict__ cand_i, const double *__restrict__ arow, const unsigned *__restrict__ amax_bits,
                  double err_coef, double *__restrict__ dist, int64_t *__restrict__ idx, int *__restrict__ n_exact,
                  int *__restrict__ flag_rows, double *__restrict__ rk_d, int *__restrict__ rk_i) {
  __shared__ float md[MAX_SPLITS * KP_MAX];
  __shared__ int mi[MAX_SPLITS * KP_MAX];
  __shared__ float kapp[KP_MAX];
  __shared__ int ki[KP_MAX];
  __shared__ double kd[KP_MAX];
  __shared__ double od[KP_MAX];
  __shared__ int oi[KP_MAX];
  __shared__ int pass;
  const int i = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int M = S * KP;
  for (int e = t; e < M; e += 256) {
    const int sp = e / KP, q = e - sp * KP;
    const int64_t src = ((int64_t)sp * N + i) * KP + q;
    const int j = cand_i[src];
    md[e] = j < 0 ? INFINITY : cand_d[src];
    mi[e] = j < 0 ? 0x7fffffff : j;
  }
  __syncthreads();
  // the K' smallest approximate entries of the S lists (ranks by counting; the keys of valid entries are distinct and
  // at least K' of them are valid, so ranks 0 .. K'-1 are written once each)
  for (int e = t; e < M; e += 256) {
    int r = 0;
    for (int f = 0; f < M; ++f) r += key_less(md[f], mi[f], md[e], mi[e]);
    if (r < KP) { kapp[r] = md[e]; ki[r] = mi[e]; }
  }
  __syncthreads();
  for (int c = w; c < KP; c += 4) {
    const int j = (unsigned)ki[c] < (unsigned)N ? ki[c] : i;   // always true for finite inputs; never an address outside X
    double acc = 0.0;
    for (int d = lane; d < D; d += 64) {
      const double diff = (double)X[(int64_t)i * D + d] - (double)X[(int64_t)j * D + d];
      acc += diff * diff;
    }
    acc = wave_sum(acc);
    if (lane == 0) kd[c] = acc;
  }
  __syncthreads();
  for (int c = t; c < KP; c += 256) {
    int r = 0;
    for (int f = 0; f < KP; ++f) r += key_less(kd[f], ki[f], kd[c], ki[c]);
    od[r] = kd[c];
    oi[r] = ki[c];
  }
  __syncthreads();
  if (t == 0) {
    const double rk = od[k - 1];
    const double amax = (double)__uint_as_float(*amax_bits);
    const double s = arow[i] + amax;
    const double B = (double)kapp[KP - 1];
    int ok = (KP == N - 1) || (rk < B - err_coef * s * s);
    if (!ok) {
      const int pos = atomicAdd(n_exact, 1);
      flag_rows[pos] = i;
      rk_d[i] = rk;
      rk_i[i] = oi[k - 1];
    }
    pass = ok;
  }
  __syncthreads();
  if (pass && t < k) {
    dist[(int64_t)i * k + t] = sqrt(od[t]);
    idx[(int64_t)i * k + t] = oi[t];
  }
}

// ------------------------------------------------------------------------------------------------ 4. exact pass
// Workgroup b takes flagged rows b, b + G, ...: the fp64 squared distance to every other row (one wave per column, lanes
// over D), those whose (distance, index) key is not above the refined k-th candidate's are gathered in this workgroup's
// N-entry workspace (the true k nearest are among them), and k rounds of a lexicographic minimum pick the answer.
__global__ void __launch_bounds__(256)
knn_exact_kernel(const float *__restrict__ X, int N, int D, int k, const int *__restrict__ n_exact,
                 const int *__restrict__ flag_rows, const double *__restrict__ rk_d, const int *__restrict__ rk_i,
                 double *__restrict__ scr_d, int *__restrict__ scr_i, double *__restrict__ dist, int64_t *__restrict__ idx) {
  __shared__ int cnt;
  __shared__ double red_d[4];
  __shared__ int red_i[4];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int nrows = *n_exact;
  double *sd = scr_d + (int64_t)blockIdx.x * N;
  int *si = scr_i + (int64_t)blockIdx.x * N;
  for (int r = blockIdx.x; r < nrows; r += gridDim.x) {
    const int i = flag_rows[r];
    const double bd = rk_d[i];
    const int bi = rk_i[i];
    if (t == 0) cnt = 0;
    __syncthreads();
    for (int j = w; j < N; j += 4) {
      if (j == i) continue;
      double acc = 0.0;
      for (int d = lane; d < D; d += 64) {
        const double diff = (double)X[(int64_t)i * D + d] - (double)X[(int64_t)j * D + d];
        acc += diff * diff;
      }
      acc = wave_sum(acc);
      if (lane == 0 && !key_less(bd, bi, acc, j)) {
        const int p = atomicAdd(&cnt, 1);
        sd[p] = acc;
        si[p] = j;
      }
    }
    __syncthreads();
    const int m = cnt;
    double pd = -INFINITY;
    int pi = -1;
    for (int q = 0; q < k; ++q) {
      double bestd = INFINITY;
      int besti = 0x7fffffff;
      for (int e = t; e < m; e += 256) {
        const double d = sd[e];
        const int j = si[e];
        if (key_less(pd, pi, d, j) && key_less(d, j, bestd, besti)) { bestd = d; besti = j; }
      }
      for (int o = 32; o > 0; o >>= 1) {
        const double od = __shfl_xor(bestd, o);
        const int oj = __shfl_xor(besti, o);
        if (key_less(od, oj, bestd, besti)) { bestd = od; besti = oj; }
      }
      if (lane == 0) { red_d[w] = bestd; red_i[w] = besti; }
      __syncthreads();
      bestd = red_d[0];
      besti = red_i[0];
      for (int v = 1; v < 4; ++v)
        if (key_less(red_d[v], red_i[v], bestd, besti)) { bestd = red_d[v]; besti = red_i[v]; }
      if (t == 0) {
        dist[(int64_t)i * k + q] = sqrt(bestd);
        idx[(int64_t)i * k + q] = besti;
      }
      pd = bestd;
      pi = besti;
      __syncthreads();                                // red_* reused by the next round
    }
  }
}

}  // namespace

IDIFF_API int64_t idiff_knn_workspace_bytes(int N, int D, int k) {
  if (N < 2 || D < 1 || k < 1 || k > 64 || k > N - 1) return 0;
  return make_plan(N, D, k).total;
}

IDIFF_API int idiff_knn_f32(const float *X, int N, int D, int k, void *workspace, int64_t workspace_bytes, double *dist,
                            int64_t *idx, int *n_exact_rows, void *stream) {
  if (N < 2) return fail("knn: N = %d, need at least 2 points", N);
  if (D < 1) return fail("knn: D = %d, need at least 1 dimension", D);
  if (k < 1 || k > 64) return fail("knn: k = %d outside 1..64", k);
  if (k > N - 1) return fail("knn: k = %d but only N - 1 = %d other points", k, N - 1);
  if (!X || !workspace || !dist || !idx || !n_exact_rows) return fail("knn: null pointer");
  if ((int64_t)N * D > ((int64_t)1 << 40)) return fail("knn: N * D too large");
  const Plan p = make_plan(N, D, k);
  if (workspace_bytes < p.total)
    return fail("knn: workspace of %lld bytes, need %lld (idiff_knn_workspace_bytes)", (long long)workspace_bytes,
                (long long)p.total);
  if (((uintptr_t)workspace & 255) != 0) return fail("knn: workspace must be 256-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  char *ws = (char *)workspace;
  double *mean = (double *)(ws + p.off_mean);
  float *Xc = (float *)(ws + p.off_xc);
  float *nrm = (float *)(ws + p.off_nrm);
  double *arow = (double *)(ws + p.off_arow);
  unsigned *amax = (unsigned *)(ws + p.off_amax);
  float *cd = (float *)(ws + p.off_cd);
  int *ci = (int *)(ws + p.off_ci);
  int *flag = (int *)(ws + p.off_flag);
  double *rkd = (double *)(ws + p.off_rkd);
  int *rki = (int *)(ws + p.off_rki);
  double *sd = (double *)(ws + p.off_sd);
  int *si = (int *)(ws + p.off_si);

  static AttrGuard guard;
  const void *fn = reinterpret_cast<const void *>(knn_tiles_kernel);
  const int lds_max = UNION_BYTES + BM * KP_MAX * 8;
  if (int rc = set_dynamic_lds_once(guard, &fn, 1, lds_max, "knn")) return rc;

  if (int rc = idiff_colmean_f64(X, 1, N, D, mean, (double *)(ws + p.off_colscr), stream)) return rc;
  hipError_t e = hipMemsetAsync(amax, 0, sizeof(unsigned), st);
  if (e == hipSuccess) e = hipMemsetAsync(n_exact_rows, 0, sizeof(int), st);
  if (e != hipSuccess) { set_error("knn: hipMemsetAsync: %s", hipGetErrorString(e)); return (int)e; }
  hipLaunchKernelGGL(knn_center_kernel, dim3(p.Np / 4), dim3(256), 0, st, X, mean, N, D, p.Dp, Xc, nrm, arow, amax);
  const int lds = UNION_BYTES + BM * p.KP * 8;
  hipLaunchKernelGGL(knn_tiles_kernel, dim3(p.Np / BM, p.S), dim3(256), lds, st, Xc, nrm, N, p.Dp, p.KP, p.tiles_per_split,
                     p.ntiles, cd, ci);
  const int T = p.Dp / KT;
  const double gamma = 1.01 * (KT + T + 4) * U32;
  hipLaunchKernelGGL(knn_refine_kernel, dim3(N), dim3(256), 0, st, X, N, D, k, p.KP, p.S, cd, ci, arow, amax,
                     gamma / 2 + 80 * U32, dist, idx, n_exact_rows, flag, rkd, rki);
  const int G = N < EXACT_GRID ? N : EXACT_GRID;
  hipLaunchKernelGGL(knn_exact_kernel, dim3(G), dim3(256), 0, st, X, N, D, k, n_exact_rows, flag, rkd, rki, sd, si, dist, idx);
  return launch_status("knn");
}
