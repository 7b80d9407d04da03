// 3x3 / stride 1 / pad 1 convolutions of the score networks by Winograd's minimal filtering F(2x2, 3x3) on the
// fp32 matrix cores of gfx950: 16 multiplications per 2x2 output tile and (cin, cout) pair instead of 36, i.e.
// 2.25x fewer MFMA flops than the implicit GEMM of igemm.hip, all of it still exact-fp32 arithmetic
// (v_mfma_f32_32x32x2_f32; the transforms only add, subtract and halve).
//
//   Y = A^T [ (G g G^T) (.) (B^T d B) ] A        d: 4x4 input patch at (2ty-1, 2tx-1), Y: 2x2 outputs at (2ty, 2tx)
//
//   U = G g G^T is packed once per layer (idiff_winograd_pack_f32) as [Cin/8][Cout/64][16 slots][64 cout][8 cin].
//   V = B^T d B is formed by the loader on its way from HBM/L2 to LDS and never written to memory.
//   M_p = V_p U_p^T for the 16 positions p = (i, j) are 16 independent [tiles x Cin] x [Cin x Cout] contractions; a
//   workgroup owns 64 tiles x 64 output channels of ALL 16 of them, so the inverse transform A^T M A is local to the
//   workgroup and M never leaves the CU either.  Position (i, j) lives in slot 4j + i (LDS and packed U alike).
//
// Cost model this kernel is built on (measured with in-kernel stamps and PMC): a SIMD's time is
//   64 cycles x (fp32 MFMAs) + ~6.5 cycles x (every other instruction its waves issue) -- fp32 MFMAs run on the
//   same fp32 lanes as the VALU and nothing overlaps them -- so the design minimises non-MFMA instructions per MFMA.
//
// Workgroup (WG_TILES = 32): 256 threads = 4 waves = the 4 rows i of the 4x4 transform domain, 32 tiles x 64 channels,
//   64 KB of LDS, 216 registers -> TWO workgroups per CU, each one's prologue and tail running under the other's K loop
//   (WG_TILES = 64, 8 waves with 2 tile halves and one workgroup per CU, also builds: 2-4 % slower, 10 % on 4x4 maps, but
//   half as many workgroups stream each filter slab).  A wave holds
//   4 positions (i, 0..3) x [32 tiles x 64 channels] = 8 MFMA tiles = 128 accumulators, and per 8-channel step issues
//   32 MFMAs from 4 sixteen-byte LDS reads of V and 8 sixteen-byte global loads of U (each lane half feeds four
//   consecutive channels to four successive MFMAs, the order of the k-reduction being free; one V fragment serves both
//   32-channel halves).
// K loop: 8 input channels per step, two LDS stages of V (16 slots x [64 tiles][8] + 32 bytes of padding per slot), one
//   barrier per step, V loads two steps ahead in registers.  U never touches LDS: the packed slab is laid out so that the
//   32 channels x 32 bytes a half wave needs for one MFMA operand are contiguous, and each lane loads its own fragments
//   (8 x 16 bytes per step) straight into the registers the MFMAs read, re-requesting a position's pair for the next
//   step as soon as that position's MFMAs have issued (4 + 4 LDS writes and 8 LDS reads per wave-step fewer than the
//   staged form: +4 %).  The allocation is what the tail's exchange needs (64 KB at 32 tiles).
// Loader: every thread owns row r of the 4x4 patch of one (tile, 4-channel quad) unit -- tiles x 2 x 4 threads.  The four
//   rows of a unit are the four lanes of a DPP quad: column mixing is local (16 VALU), row mixing is one v_fmac_f32_dpp per value (quad_perm:[2,2,1,1], signs
//   -1,+1,-1,-1; row 3 comes out negated and the packed U carries the same sign).  Per-step address offsets ride in the
//   buffer instructions' scalar offset.  Half of the waves transform at the start of a step, the other half at the end,
//   so that the matrix pipe of a SIMD always has some wave's MFMAs.
// LDS rows are 32 bytes (8 channels); the two 16-byte halves of row r are swapped when bit 3 of r is set (in LDS for V,
//   in the packed slab for U), which makes the ds_read_b128 of a 32-row MFMA operand conflict-free, and the V slot pitch
//   of 520 floats makes the four rows' ds_write_b128 conflict-free (lane groups per instruction: MI355X_MICROARCH.md section LDS).
// Tail: each wave mixes its row over j (z_ib), the four rows meet in LDS ([4 rows][tiles][2][64 cout], over the dead
//   stage buffers), and every thread finishes float4 runs of 4 channels: Y[0][b] = z0b + z1b + z2b,
//   Y[1][b] = z1b - z2b - z3b, fused epilogue (bias, per-sample bias, activation, residual, scales, optional per-tile
//   column statistics), 16-byte stores -- the one-dword-per-lane store tail of the first version was store-issue bound
//   (29.8k of 131k cycles per workgroup at Cin = 128).
#include "wino_host.h"
#include <stdlib.h>
#include <type_traits>

namespace {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef unsigned int uintx4 __attribute__((ext_vector_type(4)));

constexpr int WG_TILES = 32;                      // 32: two workgroups per CU (see the header); 64 also builds
constexpr int THREADS = WG_TILES * 8;
constexpr int NWAVES = THREADS / 64;
constexpr int WG_COUT = 64;
constexpr int KC = 8;
constexpr int NPOS = 16;
constexpr int OPER_FLOATS = NPOS * 64 * KC;       // one operand of one stage in HBM order: 8192 floats = 32 KB
constexpr int V_SLOT = WG_TILES * KC + 8;         // LDS floats per position slot of V (see above); = 8 mod 32
constexpr int V_FLOATS = NPOS * V_SLOT;           // 8320
constexpr int STAGE_FLOATS = V_FLOATS;            // U never touches LDS
constexpr int TAIL_FLOATS = 4 * WG_TILES * 2 * 64;     // the tail's exchange: [4 rows][tiles][2][64 cout]
constexpr size_t LDS_BYTES = sizeof(float) * (size_t)(2 * STAGE_FLOATS > TAIL_FLOATS ? 2 * STAGE_FLOATS : TAIL_FLOATS);   // 64 KB
constexpr int64_t X_LIMIT = 0xFFFF0000ll;          // one buffer descriptor, with room for the invalid-pixel bias
constexpr int PEEL_MIN_WORKGROUPS = 4 * 512;      // four rounds of 2 workgroups on each of 256 CUs
constexpr uint32_t INVALID_PIXEL = 0xFFFF8000u;    // beyond any valid extent (the scalar step offset is not range-checked)

struct WinoParams {
  const float *x;
  const float *u;
  float *out;
  int B, H, W, Cin, Cout;
  int tiles_x, tiles_y, tiles_per_img, total_tiles;
  int tx_shift, tpi_shift;        // log2 of tiles_x / tiles_per_img when both are powers of two, else -1 (division)
  int tiles_m, tiles_n, ngroup;   // ngroup: output-channel tiles scheduled together (tile_n innermost inside a group)
  uint32_t x_bytes, u_bytes, out_bytes, res_bytes;
  idiff_epilogue ep;
  int has_ep;
};

__device__ __forceinline__ float4 f4sub(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
__device__ __forceinline__ float4 f4add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// tile index -> (image, tile row, tile column); the maps of the score networks are powers of two, where this is two
// shifts and two masks instead of two ~20-instruction integer divisions
__device__ __forceinline__ void split_tile(const WinoParams &p, int T, int &img, int &ty, int &tx) {
  if (p.tx_shift >= 0) {
    img = T >> p.tpi_shift;
    const int rem = T & (p.tiles_per_img - 1);
    ty = rem >> p.tx_shift; tx = rem & (p.tiles_x - 1);
  } else {
    img = T / p.tiles_per_img;
    const int rem = T - img * p.tiles_per_img;
    ty = rem / p.tiles_x; tx = rem - ty * p.tiles_x;
  }
}

// ---------------------------------------------------------------- tail
// acc[2 j + h] = M at position (wi, j) for this wave's 32 tiles x cout half h, in the 32x32 accumulator layout.
__device__ __forceinline__ void wino_tail(const WinoParams &p, const floatx16 *acc, float *lds, const int tile0, const int n0,
                                          const int tile_m, const int tid, const int lane, const int wave, const int wi, const int tb) {
  // This thread finishes 4 channels (n .. n+3) of tiles 2g and 2g+1: output pixels (2ty + a, 2tx + b).  Everything here
  // is VALU work that no MFMA hides (a wave's non-MFMA VALU instructions were split about evenly between the K loop and
  // prologue + tail at Cin = 256), so the tail is written to issue as few of them as it can: 32-bit byte offsets into
  // buffer descriptors of `out` and `residual` (one VGPR per tile; the four pixels of a tile differ by wave-uniform
  // amounts that ride in the scalar offset), bias + per-sample bias and out_scale x per-sample scale folded once per
  // tile, an out-of-range offset instead of a predicate for tiles beyond the end.  Every epilogue operand that comes
  // from memory is requested BEFORE the transform-domain exchange, so its latency hides under it (the residual read
  // issued at its point of use cost 0.3 ms of a 3.1 ms launch).
  const idiff_epilogue &ep = p.ep;
  const bool has_ep = p.has_ep != 0;
  const bool want_stats = has_ep && ep.colstats != nullptr;
  const int cq = tid & 15, g = tid >> 4;
  const int n = n0 + 4 * cq;
  const bool per_image = ep.rows_per_group == p.H * p.W;   // the usual per-sample bias / scale: group = image
  const bool grouped = has_ep && !per_image && (ep.rowbias || ep.rowscale);   // any other row group: cold path below
  const bool has_res = has_ep && ep.residual != nullptr;
  const bool scaled = has_ep && (ep.out_scale != 1.f || ep.rowscale != nullptr);
  const int act = has_ep ? ep.act : (int)IDIFF_ACT_NONE;
  const __amdgpu_buffer_rsrc_t rO = __builtin_amdgcn_make_buffer_rsrc((void *)p.out, 0, (int)p.out_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rR = __builtin_amdgcn_make_buffer_rsrc((void *)ep.residual, 0, (int)p.res_bytes, 0x00020000);
  const int ld_res = (int)ep.ld_residual;
  int m00[2];                  // row of `out` of pixel (0, 0) of the tile
  uint32_t ooff[2];            // its byte offset (+ this thread's channels), INVALID_PIXEL beyond the last tile
  float4 badd[2], res[2][4];
  float sc[2];
  {
    int T = tile0 + 2 * g, img, ty, tx;
    split_tile(p, T, img, ty, tx);
    float4 bias = make_float4(0.f, 0.f, 0.f, 0.f);
    if (has_ep && ep.bias) bias = *reinterpret_cast<const float4 *>(ep.bias + n);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const bool ok = T < p.total_tiles;
      m00[t] = (img * p.H + 2 * ty) * p.W + 2 * tx;
      ooff[t] = ok ? ((uint32_t)m00[t] * (uint32_t)p.Cout + (uint32_t)n) * 4u : INVALID_PIXEL;
      badd[t] = bias;
      sc[t] = has_ep ? ep.out_scale : 1.f;
      if (has_ep && per_image && ok) {
        if (ep.rowbias) badd[t] = f4add(bias, *reinterpret_cast<const float4 *>(ep.rowbias + (int64_t)img * ep.ld_rowbias + n));
        if (ep.rowscale) sc[t] *= ep.rowscale[img];
      }
      if (has_res) {
        const uint32_t roff = ok ? ((uint32_t)m00[t] * (uint32_t)ld_res + (uint32_t)n) * 4u : INVALID_PIXEL;
#pragma unroll
        for (int ab = 0; ab < 4; ++ab)
          res[t][ab] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rR, (int)roff, ((ab >> 1) * p.W + (ab & 1)) * ld_res * 4, 0));
      }
      ++T;
      if (++tx == p.tiles_x) { tx = 0; if (++ty == p.tiles_y) { ty = 0; ++img; } }
    }
  }

  // z_ib for this wave's row i: z_i0 = m_i0 + m_i1 + m_i2, z_i1 = m_i1 - m_i2 - m_i3 -> LDS [i][tile][b][cout]
  {
    float *zp = lds + ((wi * WG_TILES + tb * 32 + 4 * (lane >> 5)) * 2) * 64 + (lane & 31);
#pragma unroll
    for (int ch = 0; ch < 2; ++ch)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const float m0 = acc[ch][reg], m1 = acc[2 + ch][reg], m2 = acc[4 + ch][reg], m3 = acc[6 + ch][reg];
        const int trow = (reg & 3) + 8 * (reg >> 2);        // + 4 * (lane >> 5): row of the 32x32 accumulator tile
        zp[(trow * 2) * 64 + ch * 32] = m0 + m1 + m2;
        zp[(trow * 2 + 1) * 64 + ch * 32] = m1 - m2 - m3;
      }
  }
  __syncthreads();

  double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int t = 0; t < 2; ++t) {
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const float *zr = lds + ((2 * g + t) * 2 + b) * 64 + 4 * cq;
      const float4 z0 = *reinterpret_cast<const float4 *>(zr);
      const float4 z1 = *reinterpret_cast<const float4 *>(zr + 1 * WG_TILES * 2 * 64);
      const float4 z2 = *reinterpret_cast<const float4 *>(zr + 2 * WG_TILES * 2 * 64);
      const float4 z3 = *reinterpret_cast<const float4 *>(zr + 3 * WG_TILES * 2 * 64);
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        float v[4];
        if (a == 0) { v[0] = z0.x + z1.x + z2.x; v[1] = z0.y + z1.y + z2.y; v[2] = z0.z + z1.z + z2.z; v[3] = z0.w + z1.w + z2.w; }
        else { v[0] = z1.x - z2.x - z3.x; v[1] = z1.y - z2.y - z3.y; v[2] = z1.z - z2.z - z3.z; v[3] = z1.w - z2.w - z3.w; }
        v[0] += badd[t].x; v[1] += badd[t].y; v[2] += badd[t].z; v[3] += badd[t].w;
        float rsv = 1.f;
        if (grouped) {
          const int64_t grp = ((int64_t)m00[t] + a * p.W + b) / ep.rows_per_group;
          if (ep.rowbias) {
            const float4 rbv = *reinterpret_cast<const float4 *>(ep.rowbias + grp * ep.ld_rowbias + n);
            v[0] += rbv.x; v[1] += rbv.y; v[2] += rbv.z; v[3] += rbv.w;
          }
          if (ep.rowscale) rsv = ep.rowscale[grp];
        }
        if (act != IDIFF_ACT_NONE) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = idiff::act_apply(v[e], act);
        }
        if (has_res) {
          const float4 r4 = res[t][2 * a + b];
          v[0] += r4.x; v[1] += r4.y; v[2] += r4.z; v[3] += r4.w;
        }
        if (scaled) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] *= sc[t];
          if (grouped) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] *= rsv;
          }
        }
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(uintx4, make_float4(v[0], v[1], v[2], v[3])), rO, (int)ooff[t],
                                               (a * p.W + b) * p.Cout * 4, 0);
        if (want_stats) {
#pragma unroll
          for (int e = 0; e < 4; ++e) { s1[e] += (double)v[e]; s2[e] += (double)v[e] * (double)v[e]; }
        }
      }
    }
  }
  if (want_stats && p.tiles_per_img < WG_TILES) {
    // Maps smaller than a workgroup (8x8: 16 tiles, 4x4: 4 tiles per sample): the workgroup holds WG_TILES / tiles_per_img
    // whole samples and writes one slot per (sample, channel), layout [B][1][Cout][2].  A thread's two tiles lie in one
    // sample (tiles_per_img is even); the 16 (tile pair, 4-channel) partial sums of the workgroup meet in LDS and
    // 64 x samples threads add up the tile pairs of their sample in a fixed order.
    __syncthreads();                                          // every z has been read: the area is free again
    double *red = reinterpret_cast<double *>(lds);           // [16 tile pairs][64 channels][2]
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      red[((g * WG_COUT) + 4 * cq + e) * 2] = s1[e];
      red[((g * WG_COUT) + 4 * cq + e) * 2 + 1] = s2[e];
    }
    __syncthreads();
    const int pairs = p.tiles_per_img >> 1, samples = WG_TILES / p.tiles_per_img;
    for (int o = tid; o < samples * WG_COUT; o += THREADS) {
      const int smp = o / WG_COUT, ch = o - smp * WG_COUT;
      const int64_t img = (int64_t)tile_m * samples + smp;
      if (img >= p.B) continue;
      double a = 0.0, b = 0.0;
      for (int k = 0; k < pairs; ++k) { a += red[((smp * pairs + k) * WG_COUT + ch) * 2]; b += red[((smp * pairs + k) * WG_COUT + ch) * 2 + 1]; }
      double *dst = ep.colstats + (img * p.Cout + n0 + ch) * 2;
      dst[0] = a; dst[1] = b;
    }
  } else if (want_stats) {
    // lanes l, l+16, l+32, l+48 hold the same four channels; then one slot per (wave, channel)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      s1[e] += __shfl_xor(s1[e], 16, 64); s1[e] += __shfl_xor(s1[e], 32, 64);
      s2[e] += __shfl_xor(s2[e], 16, 64); s2[e] += __shfl_xor(s2[e], 32, 64);
    }
    __syncthreads();                                          // every z has been read: the area is free again
    double *red = reinterpret_cast<double *>(lds);           // [NWAVES][64][2]
    if (lane < 16) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        red[((wave * WG_COUT) + 4 * cq + e) * 2] = s1[e];
        red[((wave * WG_COUT) + 4 * cq + e) * 2 + 1] = s2[e];
      }
    }
    __syncthreads();
    if (tid < WG_COUT) {
      double a = 0.0, b = 0.0;
#pragma unroll
      for (int w = 0; w < NWAVES; ++w) { a += red[(w * WG_COUT + tid) * 2]; b += red[(w * WG_COUT + tid) * 2 + 1]; }
      double *dst = ep.colstats + ((int64_t)tile_m * p.Cout + n0 + tid) * 2;
      dst[0] = a; dst[1] = b;
    }
  }
}

// PEEL: step 0 is peeled and its MFMAs take C = 0 as an inline constant, so no accumulator is initialised (1-3 % on the
// large maps); launches of only a few rounds of workgroups (the 4x4 maps) measured 7 % faster with the plain loop.
template <bool PEEL>
__global__ void __launch_bounds__(THREADS, 2)   // two waves per SIMD (256 VGPRs): two 256-thread workgroups per CU
winograd_kernel(const WinoParams p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];

  const int nwg = p.tiles_m * p.tiles_n;
  int bid = blockIdx.x;
  {
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, local = bid >> 3;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + local;
  }
  // groups of `ngroup` output-channel tiles: inside a group tile_n is innermost (the workgroups of an XCD share the input
  // patches of a run of tile_m and stream only ngroup filter slabs), the groups follow one another
  const int per_group = p.tiles_m * p.ngroup;
  const int grp = bid / per_group, in_grp = bid - grp * per_group;
  const int tile_n = grp * p.ngroup + in_grp % p.ngroup, tile_m = in_grp / p.ngroup;
  const int tile0 = tile_m * WG_TILES, n0 = tile_n * WG_COUT;
  const int tid = threadIdx.x, lane = tid & 63;
  // the wave index in an SGPR: roles, operand halves and buffer descriptors stay provably wave-uniform (no waterfall
  // loops around the buffer loads, scalar branches)
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wi = wave & 3, tb = wave >> 2;   // transform-domain row, 32-tile half

  const __amdgpu_buffer_rsrc_t rX = __builtin_amdgcn_make_buffer_rsrc((void *)p.x, 0, (int)p.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rU = __builtin_amdgcn_make_buffer_rsrc((void *)p.u, 0, (int)p.u_bytes, 0x00020000);

  // ---------------------------------------------------------------- loader state
  const bool early = wave < NWAVES / 2;    // waves w and w+4 share a SIMD: one transforms while the other feeds the matrix pipe
  uint32_t v_src[4], u_src[4];
  int v_dst;
  float sgn;
  {
    const int r = tid & 3, q = (tid >> 2) & 1, tl = tid >> 3;
    const int T = tile0 + tl;
    const bool tv = T < p.total_tiles;
    const int TT = tv ? T : 0;
    int img, ty, tx;
    split_tile(p, TT, img, ty, tx);
    const int y = 2 * ty - 1 + r, x0 = 2 * tx - 1;
    const bool yok = tv && y >= 0 && y < p.H;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int xx = x0 + j;
      v_src[j] = (yok && xx >= 0 && xx < p.W) ? (uint32_t)(((img * p.H + y) * p.W + xx) * p.Cin + q * 4) * 4u : INVALID_PIXEL;
    }
    v_dst = r * V_SLOT + tl * KC + 4 * (q ^ ((tl >> 3) & 1));
    sgn = (r == 1) ? 1.f : -1.f;
    // U fragments go straight from the slab to the MFMA operand registers of the lane that uses them (32 channels x 32
    // bytes contiguous per half wave): no LDS round trip for the filter bank
    const int fr_ = lane & 31, fh_ = lane >> 5;
#pragma unroll
    for (int j = 0; j < 4; ++j) u_src[j] = (uint32_t)(((4 * j + wi) * 64 + fr_) * 32 + 16 * (fh_ ^ ((fr_ >> 3) & 1)));
  }

  float4 ldv[4], bfr[4][2];
  const int nsteps = p.Cin / KC;
  int f_step = 0;
  // the per-step offsets are wave-uniform: they ride in the buffer instruction's scalar offset (not part of the range
  // check of a raw buffer, so an out-of-range pixel stays out of range) instead of costing a VALU add per load
  auto fetch = [&]() {
    const int choff = min(f_step, nsteps - 1) * (KC * 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) ldv[j] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rX, (int)v_src[j], choff, 0));
    ++f_step;
  };

  auto stage = [&](int buf) {
    float *Vd = lds + buf * STAGE_FLOATS + v_dst;
    float4 c[4];
    c[0] = f4sub(ldv[0], ldv[2]); c[1] = f4add(ldv[1], ldv[2]); c[2] = f4sub(ldv[2], ldv[1]); c[3] = f4sub(ldv[1], ldv[3]);
    // c += sgn * quad_perm[2,2,1,1](c), the permute folded into the fma's DPP operand (hipcc keeps v_mov_b32_dpp + v_fmac
    // apart).  s_nop 1: a VALU write of a VGPR needs two wait states before a DPP read of it, and the hazard
    // recogniser does not look inside inline asm.
#define IDIFF_QFMA(x) "v_fmac_f32_dpp " x ", " x ", %16 quad_perm:[2,2,1,1] row_mask:0xf bank_mask:0xf bound_ctrl:1\n"
    asm volatile("s_nop 1\n" IDIFF_QFMA("%0") IDIFF_QFMA("%1") IDIFF_QFMA("%2") IDIFF_QFMA("%3") IDIFF_QFMA("%4") IDIFF_QFMA("%5")
                 IDIFF_QFMA("%6") IDIFF_QFMA("%7") IDIFF_QFMA("%8") IDIFF_QFMA("%9") IDIFF_QFMA("%10") IDIFF_QFMA("%11")
                 IDIFF_QFMA("%12") IDIFF_QFMA("%13") IDIFF_QFMA("%14") IDIFF_QFMA("%15")
                 : "+v"(c[0].x), "+v"(c[0].y), "+v"(c[0].z), "+v"(c[0].w), "+v"(c[1].x), "+v"(c[1].y), "+v"(c[1].z), "+v"(c[1].w),
                   "+v"(c[2].x), "+v"(c[2].y), "+v"(c[2].z), "+v"(c[2].w), "+v"(c[3].x), "+v"(c[3].y), "+v"(c[3].z), "+v"(c[3].w)
                 : "v"(sgn));
#undef IDIFF_QFMA
#pragma unroll
    for (int j = 0; j < 4; ++j) *reinterpret_cast<float4 *>(Vd + j * 4 * V_SLOT) = c[j];
  };

  floatx16 acc[8];   // [j][channel half]; PEEL: first written by the MFMAs of step 0 (the 2 x 128 v_mov_b32 of an explicit
                     // initialisation were 11 % of a wave's non-MFMA VALU work)

  const int fr = lane & 31, fh = lane >> 5;
  const int frag = fr * KC + 4 * (fh ^ ((fr >> 3) & 1));
  const int a_frag = wi * V_SLOT + tb * 32 * KC + frag;       // slot of position (wi, j): 4j + wi

  auto load_b = [&](int j, int step) {
    const int slab = (step * p.tiles_n + tile_n) * (OPER_FLOATS * 4);
    bfr[j][0] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rU, (int)u_src[j], slab, 0));
    bfr[j][1] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rU, (int)u_src[j] + 32 * 32, slab, 0));
  };
  // The four positions of a step one after the other, their V fragments through TWO registers sets in rotation: the fragment
  // of position j + 2 is read from LDS right after the eight MFMAs of position j have been issued, so the eight MFMAs of
  // position j + 1 (512 cycles) cover its latency.  (Before, the compiler interleaved positions 0 / 1 and then read the
  // fragments of positions 2 and 3 each immediately in front of its use: two exposed LDS round trips per step.)
  auto mfma8 = [&](int j, const float4 a, auto first) {
    const float4 b0 = bfr[j][0], b1 = bfr[j][1];
    if constexpr (decltype(first)::value) {
      const floatx16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      acc[2 * j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b0.x, zero, 0, 0, 0);
      acc[2 * j + 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b1.x, zero, 0, 0, 0);
    } else {
      acc[2 * j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b0.x, acc[2 * j], 0, 0, 0);
      acc[2 * j + 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b1.x, acc[2 * j + 1], 0, 0, 0);
    }
    acc[2 * j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b0.y, acc[2 * j], 0, 0, 0);
    acc[2 * j + 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b1.y, acc[2 * j + 1], 0, 0, 0);
    acc[2 * j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b0.z, acc[2 * j], 0, 0, 0);
    acc[2 * j + 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b1.z, acc[2 * j + 1], 0, 0, 0);
    acc[2 * j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b0.w, acc[2 * j], 0, 0, 0);
    acc[2 * j + 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b1.w, acc[2 * j + 1], 0, 0, 0);
  };
  auto compute = [&](int buf, int s, auto first, auto before_last) {
    const float *S = lds + buf * STAGE_FLOATS + a_frag;
    const int snext = min(s + 1, nsteps - 1);
    float4 f0 = *reinterpret_cast<const float4 *>(S), f1 = *reinterpret_cast<const float4 *>(S + 4 * V_SLOT);
    __builtin_amdgcn_sched_barrier(0);
    mfma8(0, f0, first);
    // the registers are free once these MFMAs have read them; the last step re-requests its own slab (clamped, not
    // skipped: no branch per position, and the scalar offset of a raw buffer is not range-checked, so it must stay valid)
    load_b(0, snext);
    f0 = *reinterpret_cast<const float4 *>(S + 8 * V_SLOT);
    __builtin_amdgcn_sched_barrier(0);
    mfma8(1, f1, first);
    load_b(1, snext);
    f1 = *reinterpret_cast<const float4 *>(S + 12 * V_SLOT);
    __builtin_amdgcn_sched_barrier(0);
    mfma8(2, f0, first);
    load_b(2, snext);
    __builtin_amdgcn_sched_barrier(0);
    before_last();                      // the late role writes its stage HERE: its LDS writes then land under eight MFMAs
    __builtin_amdgcn_sched_barrier(0);  // instead of in front of the barrier
    mfma8(3, f1, first);
    load_b(3, snext);
  };
  // The role is a compile-time constant of the loop a wave runs, and writing the next stage / requesting the one after are
  // unconditional (the last two steps re-request the last stage and write a stage nobody reads): the compiler's wait counts
  // are static, and with `if (early)` / `if (s + 2 < nsteps)` inside one shared loop the paths merged into `s_waitcnt
  // vmcnt(1) / vmcnt(0)` in front of the input transform -- an early wave waited for the filter loads of the CURRENT step
  // (issued at the end of the previous one) before starting the work that is meant to cover them.
  auto step = [&](int s, auto first, auto is_early) {
    const int buf = s & 1;
    if constexpr (decltype(is_early)::value) {
      stage(buf ^ 1); fetch();
      compute(buf, s, first, [] {});
    } else {
      compute(buf, s, first, [&] { stage(buf ^ 1); fetch(); });
    }
    __syncthreads();
  };

#pragma unroll
  for (int j = 0; j < 4; ++j) load_b(j, 0);
  fetch();
  stage(0);
  fetch();
  __syncthreads();

  auto run = [&](auto is_early) {
    if constexpr (PEEL) {
      step(0, std::true_type(), is_early);
      for (int s = 1; s < nsteps; ++s) step(s, std::false_type(), is_early);
    } else {
      for (int s = 0; s < nsteps; ++s) step(s, std::false_type(), is_early);
    }
  };
  if constexpr (!PEEL) {
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
  }
  if (early) run(std::true_type()); else run(std::false_type());

  wino_tail(p, acc, lds, tile0, n0, tile_m, tid, lane, wave, wi, tb);
}

// U = G g G^T in fp64, rounded once; g[ky][kx] = wt[cout][ky][kx][cin] (the K-contiguous panel of the direct kernel).
__global__ void winograd_pack_kernel(const float *wt, float *u, int Cin, int Cout) {
  const int64_t total = (int64_t)Cin * Cout;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int cin = (int)(idx % Cin), cout = (int)(idx / Cin);
    double g[3][3];
    for (int ky = 0; ky < 3; ++ky)
      for (int kx = 0; kx < 3; ++kx) g[ky][kx] = (double)wt[((int64_t)cout * 9 + ky * 3 + kx) * Cin + cin];
    double gg[4][3];   // G g
    for (int kx = 0; kx < 3; ++kx) {
      gg[0][kx] = g[0][kx];
      gg[1][kx] = 0.5 * (g[0][kx] + g[1][kx] + g[2][kx]);
      gg[2][kx] = 0.5 * (g[0][kx] - g[1][kx] + g[2][kx]);
      gg[3][kx] = g[2][kx];
    }
    const int s = cin / KC, c8 = cin % KC, nt = cout / WG_COUT, co = cout % WG_COUT;
    const int slot = 4 * ((c8 >> 2) ^ ((co >> 3) & 1)) + (c8 & 3);
    float *dst = u + ((int64_t)(s * (Cout / WG_COUT) + nt) * NPOS * 64 + co) * KC + slot;
    for (int i = 0; i < 4; ++i) {
      const double r0 = gg[i][0], r1 = gg[i][1], r2 = gg[i][2];
      const double v[4] = {r0, 0.5 * (r0 + r1 + r2), 0.5 * (r0 - r1 + r2), r2};
      const double sign = i == 3 ? -1.0 : 1.0;     // the kernel's input transform produces row 3 negated
      for (int j = 0; j < 4; ++j) dst[(int64_t)(j * 4 + i) * 64 * KC] = (float)(sign * v[j]);
    }
  }
}

bool geometry_ok(int B, int H, int W, int Cin, int Cout) {
  if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return false;
  if (H % 2 || W % 2 || Cin % KC || Cout % WG_COUT) return false;
  if ((int64_t)Cin * 4 > 0x7000) return false;                               // channel offset must stay below the invalid-pixel bias
  if ((int64_t)16 * Cin * Cout * 4 >= X_LIMIT) return false;
  if ((int64_t)B * (H / 2) * (W / 2) > 0x7fffffff / 4) return false;
  return true;
}

}  // namespace

IDIFF_API int idiff_conv2d_winograd_ok(int B, int H, int W, int Cin, int Cout) {
  if (idiff::option(idiff::OPT_NO_WINOGRAD)) return 0;
  return geometry_ok(B, H, W, Cin, Cout) ? 1 : 0;
}

IDIFF_API int idiff_conv2d_winograd_colstats_split(int B, int H, int W, int Cin, int Cout) {
  if (!idiff_conv2d_winograd_ok(B, H, W, Cin, Cout) || idiff::option(idiff::OPT_NO_COLSTATS)) return 0;
  if ((int64_t)B * H * W * (Cin > Cout ? Cin : Cout) * 4 >= X_LIMIT) return 0;
  const int tpi = (H / 2) * (W / 2);
  if (tpi % WG_TILES == 0) return tpi / WG_TILES;
  // maps smaller than a workgroup's 32 tiles (8x8, 4x4): whole samples per workgroup, one slot per sample
  return (tpi >= 2 && tpi % 2 == 0 && WG_TILES % tpi == 0) ? 1 : 0;
}

IDIFF_API int64_t idiff_winograd_weight_floats(int Cin, int Cout) { return (int64_t)16 * Cin * Cout; }

IDIFF_API int idiff_winograd_pack_f32(const float *wt, float *u, int Cin, int Cout, void *stream) {
  using namespace idiff;
  if (Cin <= 0 || Cout <= 0 || Cin % KC || Cout % WG_COUT)
    return fail("winograd_pack: Cin must be a multiple of %d and Cout of %d (got %d, %d)", KC, WG_COUT, Cin, Cout);
  if (!wt || !u) return fail("winograd_pack: null pointer");
  const int64_t total = (int64_t)Cin * Cout;
  hipLaunchKernelGGL(winograd_pack_kernel, dim3(streaming_grid(total, 256)), dim3(256), 0, (hipStream_t)stream, wt, u, Cin, Cout);
  return launch_status("winograd_pack");
}

IDIFF_API int idiff_conv2d_winograd_f32(const float *x, const float *u, float *out, int B, int H, int W, int Cin, int Cout,
                                        const idiff_epilogue *ep, void *stream) {
  using namespace idiff;
  if (B == 0) return 0;
  if (!geometry_ok(B, H, W, Cin, Cout))
    return fail("conv2d_winograd: geometry B=%d H=%d W=%d Cin=%d Cout=%d not supported (ask idiff_conv2d_winograd_ok)", B, H, W, Cin, Cout);
  if (int rc = wino_check_operands("conv2d_winograd", x, u, out, ep, Cout)) return rc;
  const int64_t x_bytes = (int64_t)B * H * W * Cin * 4, out_bytes = (int64_t)B * H * W * Cout * 4, res_bytes = wino_residual_bytes(ep, B, H, W);
  // the kernel addresses x, out and residual through one buffer descriptor each (32-bit byte offsets)
  if (x_bytes >= X_LIMIT || out_bytes >= X_LIMIT || res_bytes >= X_LIMIT) {
    if (ep && ep->colstats) return fail("conv2d_winograd: colstats is not available for inputs beyond one buffer descriptor");
    if (B < 2) return fail("conv2d_winograd: a single image exceeds one buffer descriptor");
    const int64_t cut = host_cut_row(B, H * W, ep);
    if (!cut) return fail("conv2d_winograd: cannot split the batch inside an epilogue row group");
    return run_cut((int64_t)B * H * W, cut, ep, false, [&](int64_t r0, int64_t r1, const idiff_epilogue *e) {
      return idiff_conv2d_winograd_f32(x + r0 * Cin, u, out + r0 * Cout, (int)((r1 - r0) / (H * W)), H, W, Cin, Cout, e, stream);
    });
  }
  WinoParams p = {};
  // two output-channel tiles per scheduling group: the workgroups of an XCD then stream two filter slabs instead of
  // four (1.5-3 % on the Cout = 256 layers; the slabs of four tiles plus the live input lines overflow the 4 MB L2)
  wino_fill(p, x, u, out, B, H, W, Cin, Cout, (int64_t)16 * Cin * Cout, res_bytes, ep, WG_COUT, true);
  wino_fill_tiles(p, 2, WG_TILES);
  if (ep && ep->colstats && p.tiles_per_img % WG_TILES && !(p.tiles_per_img >= 2 && p.tiles_per_img % 2 == 0 && WG_TILES % p.tiles_per_img == 0))
    return fail("conv2d_winograd: colstats needs whole workgroups per sample or whole samples per workgroup "
                "(ask idiff_conv2d_winograd_colstats_split)");
  const void *fns[2] = {reinterpret_cast<const void *>(winograd_kernel<false>), reinterpret_cast<const void *>(winograd_kernel<true>)};
  {
    static AttrGuard guard;
    if (int rc = set_dynamic_lds_once(guard, fns, 2, (int)LDS_BYTES, "conv2d_winograd")) return rc;
  }
  const int nwg = p.tiles_m * p.tiles_n;
  if (nwg >= PEEL_MIN_WORKGROUPS)
    hipLaunchKernelGGL(winograd_kernel<true>, dim3(nwg), dim3(THREADS), LDS_BYTES, (hipStream_t)stream, p);
  else
    hipLaunchKernelGGL(winograd_kernel<false>, dim3(nwg), dim3(THREADS), LDS_BYTES, (hipStream_t)stream, p);
  return launch_status("conv2d_winograd");
}
