// What the four 3x3 Winograd files (winograd.hip, winograd43.hip, winograd43h.hip, wino1d.hip) share IN FRONT of their convolution
// kernels: the six interpolation points and their G, the filter-bank packer of the two fp16-pair forms, the validation of a call and the
// fill of the kernel arguments.  Host code and run-once pack kernels only; the kernel-argument structs stay in their files, each with its
// own field order (a common base would move kernarg offsets), and are filled here by field NAME.
#pragma once
#include "common.h"

namespace {

// Interpolation points 0, +-a, +-b, infinity with a b = 1 (reciprocal pairs keep the transforms balanced): a = 2/3, b = 3/2.
// (scripts/f43_emulation.py on the whole network: rel_err(S) 3.3e-6 for this set, 4.9e-6 for 1/2, 2 -- whose constants are all
// dyadic -- and 7.0e-6 for Lavin's 1, 2.)  The transforms use these fp32 constants; G is evaluated in fp64 from the same a, b.
constexpr double F4_A = 2.0 / 3.0, F4_B = 1.5;
constexpr float F4_a = (float)F4_A, F4_b = (float)F4_B, F4_a2 = (float)(F4_A * F4_A), F4_b2 = (float)(F4_B * F4_B),
                F4_a3 = (float)(F4_A * F4_A * F4_A), F4_b3 = (float)(F4_B * F4_B * F4_B), F4_ab2 = (float)(F4_A * F4_A + F4_B * F4_B);

// G of the points 0, +-a, +-b, infinity in fp64.  Row of point p: (1, p, p^2) / N(p), N(p) = prod over the other finite points (p - q);
// N(0) = a^2 b^2, N(+-a) = 2 a^2 (a^2 - b^2), N(+-b) = 2 b^2 (b^2 - a^2); the point at infinity picks g[2]
__device__ __forceinline__ void wino_G(const double a, const double b, double (&G)[6][3]) {
  const double na = 1.0 / (2.0 * a * a * (a * a - b * b)), nb = 1.0 / (2.0 * b * b * (b * b - a * a)), n0 = 1.0 / (a * a * b * b);
  const double rows[6][3] = {{n0, 0.0, 0.0}, {na, a * na, a * a * na}, {na, -a * na, a * a * na}, {nb, b * nb, b * b * nb}, {nb, -b * nb, b * b * nb},
                             {0.0, 0.0, 1.0}};
  for (int i = 0; i < 6; ++i)
    for (int k = 0; k < 3; ++k) G[i][k] = rows[i][k];
}

// a0 b0 + a1 b1 + a2 b2 in fp64 with its roundings written out: product UNFUSED (0 or 1) is rounded on its own, the other of the first two
// is fused onto it and the third onto their sum.  Left to the compiler's contraction the one expression came out as UNFUSED = 0 in
// winograd43_pack_kernel and as 1 in the pair packers (an fp32 ulp apart in 7e-5 of a bank's values): each bank keeps the form it had.
template <int UNFUSED>
__device__ __forceinline__ double wino_dot3(double a0, double b0, double a1, double b1, double a2, double b2) {
  return fma(a2, b2, UNFUSED == 0 ? fma(a1, b1, a0 * b0) : fma(a0, b0, a1 * b1));
}

// ---------------------------------------------------------------- filter banks of fp16 pairs (winograd43h.hip: 36 slots, wino1d.hip: 18)
// [Cin/16][Cout/64][NSLOT][2 planes (hi, lo)][64 cout][16 cin] fp16 + 4 floats of header (the factor that undoes the scaling first)
constexpr int PAIR_KC = 16;
constexpr int PAIR_COUT = 64;
constexpr int PAIR_PLANE_BYTES = PAIR_COUT * PAIR_KC * 2;           // 2048
constexpr int PAIR_SLOT_BYTES = 2 * PAIR_PLANE_BYTES;               // 4096: one slot of one (step, cout tile)

// the NSLOT weight-domain values of one (cin, cout) pair in fp64: f4_u_of_pair, r1_u_of_pair
template <int NSLOT> using PairU = void (*)(const float *wt, int Cin, int cin, int cout, double (&U)[NSLOT]);

// pass 1: max |U| over the layer (bits of a non-negative float order like unsigned integers; the word was zeroed by the launcher)
template <int NSLOT, PairU<NSLOT> U_OF_PAIR>
__global__ void pair_absmax_kernel(const float *wt, unsigned int *absmax_bits, int Cin, int Cout) {
  const int64_t total = (int64_t)Cin * Cout;
  float m = 0.f;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    double U[NSLOT];
    U_OF_PAIR(wt, Cin, (int)(idx % Cin), (int)(idx / Cin), U);
    for (int k = 0; k < NSLOT; ++k) m = fmaxf(m, fabsf((float)U[k]));
  }
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0 && m > 0.f) atomicMax(absmax_bits, __float_as_uint(m));
}

// pass 2: the pairs.  The scale 2^k brings max |U| into [2^11, 2^12); header[0] receives 2^-k.
template <int NSLOT, PairU<NSLOT> U_OF_PAIR>
__global__ void pair_pack_kernel(const float *wt, _Float16 *u, float *header, int Cin, int Cout) {
  const float amax = __uint_as_float(*reinterpret_cast<const unsigned int *>(header + 1));
  int e = 0;
  if (amax > 0.f && isfinite(amax)) { (void)frexpf(amax, &e); }          // amax = f 2^e, f in [0.5, 1)
  const int k = (amax > 0.f && isfinite(amax)) ? 12 - e : 0;
  const double scale = ldexp(1.0, k);
  const int64_t total = (int64_t)Cin * Cout;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int cin = (int)(idx % Cin), cout = (int)(idx / Cin);
    double U[NSLOT];
    U_OF_PAIR(wt, Cin, cin, cout, U);
    const int s = cin / PAIR_KC, c16 = cin % PAIR_KC, nt = cout / PAIR_COUT, co = cout % PAIR_COUT;
    _Float16 *dst = u + ((int64_t)(s * (Cout / PAIR_COUT) + nt) * NSLOT) * (PAIR_SLOT_BYTES / 2) + co * PAIR_KC + c16;
    for (int q = 0; q < NSLOT; ++q) {
      const float v = (float)(U[q] * scale);                                   // rounded once to fp32, as the fp32 kernel's U, then cut
      const _Float16 hi = (_Float16)v;
      const _Float16 lo = (_Float16)(v - (float)hi);
      dst[(int64_t)q * (PAIR_SLOT_BYTES / 2)] = hi;
      dst[(int64_t)q * (PAIR_SLOT_BYTES / 2) + PAIR_PLANE_BYTES / 2] = lo;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) header[0] = (float)ldexp(1.0, -k);
}

// idiff_winograd43h_pack_f32 / idiff_wino1d_pack_f32: u receives NSLOT * Cin * Cout floats of pairs and the header behind them
template <int NSLOT, PairU<NSLOT> U_OF_PAIR>
int pair_bank_pack(const char *name, const float *wt, float *u, int Cin, int Cout, void *stream) {
  using namespace idiff;
  if (Cin <= 0 || Cout <= 0 || Cin % PAIR_KC || Cout % PAIR_COUT)
    return fail("%s: Cin must be a multiple of %d and Cout of %d (got %d, %d)", name, PAIR_KC, PAIR_COUT, Cin, Cout);
  if (!wt || !u) return fail("%s: null pointer", name);
  if ((uintptr_t)u & 15) return fail("%s: u must be 16-byte aligned", name);
  const int64_t total = (int64_t)Cin * Cout;
  float *header = u + (int64_t)NSLOT * Cin * Cout;
  hipError_t e = hipMemsetAsync(header, 0, 16, (hipStream_t)stream);
  if (e != hipSuccess) return fail("%s: hipMemsetAsync: %s", name, hipGetErrorString(e));
  hipLaunchKernelGGL((pair_absmax_kernel<NSLOT, U_OF_PAIR>), dim3(streaming_grid(total, 256)), dim3(256), 0, (hipStream_t)stream, wt,
                     reinterpret_cast<unsigned int *>(header + 1), Cin, Cout);
  hipLaunchKernelGGL((pair_pack_kernel<NSLOT, U_OF_PAIR>), dim3(streaming_grid(total, 256)), dim3(256), 0, (hipStream_t)stream, wt,
                     reinterpret_cast<_Float16 *>(u), header, Cin, Cout);
  return launch_status(name);
}

// ---------------------------------------------------------------- validation of a convolution call (after the form's own geometry check)
// what every form asks of its operands: no null pointer, 16-byte alignment, a residual, bias and per-group bias the tail can read 16 bytes
// at a time
inline int wino_check_operands(const char *name, const float *x, const float *u, const float *out, const idiff_epilogue *ep, int Cout) {
  using namespace idiff;
  if (!x || !u || !out) return fail("%s: null pointer", name);
  if (((uintptr_t)x & 15) || ((uintptr_t)u & 15) || ((uintptr_t)out & 15)) return fail("%s: x, u and out must be 16-byte aligned", name);
  if (ep && ep->residual && (((uintptr_t)ep->residual & 15) || ep->ld_residual % 4 || ep->ld_residual < Cout || ep->ld_residual > 0x7fffffff / 4))
    return fail("%s: residual must be 16-byte aligned with a row pitch >= Cout that is a multiple of 4", name);
  // every tail reads bias and the per-group bias four channels at a time; there is no scalar form to fall back to
  if (ep && ep->bias && ((uintptr_t)ep->bias & 15)) return fail("%s: bias must be 16-byte aligned", name);
  if (ep && ep->rowbias && (((uintptr_t)ep->rowbias & 15) || ep->ld_rowbias % 4))
    return fail("%s: rowbias must be 16-byte aligned with a row pitch that is a multiple of 4", name);
  return 0;
}

inline int64_t wino_residual_bytes(const idiff_epilogue *ep, int B, int H, int W) {
  return (ep && ep->residual) ? (int64_t)B * H * W * ep->ld_residual * 4 : 0;
}

// the forms that serve per-image row groups only and one buffer descriptor (`limit` bytes) per tensor: winograd43, winograd43h, wino1d
inline int wino_check_call(const char *name, const float *x, const float *u, const float *out, const idiff_epilogue *ep, int B, int H, int W,
                           int Cout, int64_t limit, int64_t &res_bytes) {
  using namespace idiff;
  if (int rc = wino_check_operands(name, x, u, out, ep, Cout)) return rc;
  if (ep && (ep->rowbias || ep->rowscale) && ep->rows_per_group != H * W)
    return fail("%s: per-row-group bias / scale only per image (rows_per_group = H * W = %d, got %d)", name, H * W, ep->rows_per_group);
  res_bytes = wino_residual_bytes(ep, B, H, W);
  if (res_bytes >= limit) return fail("%s: residual beyond one buffer descriptor", name);
  return 0;
}

// ---------------------------------------------------------------- kernel arguments, by field name
template <class P> auto wino_fill_consts(P &p, int) -> decltype((void)p.c_nb2) {
  p.c_nb2 = -F4_b2; p.c_na2 = -F4_a2; p.c_nab2 = -F4_ab2; p.c_a = F4_a; p.c_b = F4_b;
}
template <class P> void wino_fill_consts(P &, long) {}      // WinoParams: F(2x2, 3x3) has no such constants

// Pointers, dimensions, byte extents (u_floats: the bank without a header), epilogue, the 6-point transforms' constants where the struct has
// them, and the output-channel tiles: ngroup of them are scheduled together (tile_n innermost inside a group):
// `ngroup_pairs ? two : all` (see the callers for which and why)
template <class P>
void wino_fill(P &p, const float *x, const float *u, float *out, int B, int H, int W, int Cin, int Cout, int64_t u_floats, int64_t res_bytes,
               const idiff_epilogue *ep, int cout_tile, bool ngroup_pairs) {
  p.x = x; p.u = u; p.out = out; p.B = B; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout;
  p.x_bytes = (uint32_t)((int64_t)B * H * W * Cin * 4); p.u_bytes = (uint32_t)(u_floats * 4);
  p.out_bytes = (uint32_t)((int64_t)B * H * W * Cout * 4); p.res_bytes = (uint32_t)res_bytes;
  idiff::set_epilogue(p, ep);
  wino_fill_consts(p, 0);
  p.tiles_n = Cout / cout_tile;
  p.ngroup = (ngroup_pairs && p.tiles_n > 2 && p.tiles_n % 2 == 0) ? 2 : p.tiles_n;
}

// the tile grid of WinoParams / Wino43Params: output tiles of edge x edge pixels, wg_tiles of them per workgroup
template <class P> void wino_fill_tiles(P &p, int edge, int wg_tiles) {
  p.tiles_x = p.W / edge; p.tiles_y = p.H / edge; p.tiles_per_img = p.tiles_x * p.tiles_y; p.total_tiles = p.B * p.tiles_per_img;
  p.tx_shift = p.tpi_shift = -1;
  if ((p.tiles_x & (p.tiles_x - 1)) == 0 && (p.tiles_per_img & (p.tiles_per_img - 1)) == 0) {
    p.tx_shift = __builtin_ctz((unsigned)p.tiles_x); p.tpi_shift = __builtin_ctz((unsigned)p.tiles_per_img);
  }
  p.tiles_m = idiff::ceil_div(p.total_tiles, wg_tiles);
}

}  // namespace
