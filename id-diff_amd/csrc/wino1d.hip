// 3x3 / stride 1 / pad 1 convolutions by Winograd's F(4, 3) ALONG THE IMAGE ROWS ONLY -- the three filter rows stay a direct sum -- with
// the 18 contractions per 1 x 4 output tile on the fp16 matrix cores of gfx950 (fp16 pairs, as winograd43h.hip).
//
// Why a second pair kernel.  winograd43h_kernel (F(4x4, 3x3): 2.25 multiplications per output) is not bound by its matrix instructions
// (22 % of the SIMD cycles) but by what its workgroup has to bring in per K step: 36 positions x 64 channels of U (147 KB) for 512 output
// pixels, because 36 accumulators per tile and channel leave room for no more pixels in the register file, plus 6 x 6 patches that repeat
// their neighbours' pixels -- 2,040 - 2,230 128-byte lines from L2 per workgroup and step, at the 16 TB/s the L2 -> L1 path delivers chip-wide
// (profiles/r05_wino43h_l1_requests.txt: the time follows the line count).  Transforming along x only costs twice the matrix work
// (4.5 multiplications per output) and HALF the lines: six positions x three filter rows of U are 74 KB per step, shared by all 512 pixels
// of the workgroup, and the input is read as whole image rows -- every pixel once per step, no horizontal halo at all, one halo row above or
// below the block.  The matrix cores have the room: 108 instructions per wave and step are 3,456 cycles of a step that took 9,300.
//
//   out[r][4t + a] = sum_i A^T[a][i] sum_ky ( V[r + ky - 1][t][i] . U[i][ky] ),   V[r][t][.] = B^T x[r][4t - 1 .. 4t + 4],   U[.][ky] = G g[ky][.]
//   (same points 0, +-2/3, +-3/2, inf and the same B^T, G, A^T as winograd43_shared.h, used in one dimension: the transform's gain is
//   5.4 where the 2-D form has 29.3, so |x| may reach 12,000 before a pair overflows, and the rounding of the transform enters once)
//
// Workgroup: 256 threads = 4 waves, ONE PER SIMD (up to 512 registers each), 512 output pixels x 64 output channels:
//   RB = 512 / W whole image rows (W = 64: eight rows, 32: half a 32 x 32 image, 16: two images, 8: eight, 4: thirty-two), 128 row-tiles of 1 x 4 pixels, six positions each.
//   Wave (h, ph): output channels 32 h .. 32 h + 31, positions 3 ph .. 3 ph + 2, all four groups of 32 row-tiles: 12 accumulator tiles of
//   32 x 32 = 192 registers.  Every U fragment (position, filter row, channel half: 2 KB of pairs) is loaded by exactly one wave, straight from
//   L2 into registers, three (position, filter row) combinations ahead.
// K step: 16 input channels.  Per wave and step nine combinations (position, filter row) x four groups x three matrix instructions
//   (hi hi, hi lo, lo hi); the V operand of (group, filter row ky) is the stage's rows 4 g + ky - 1 .. 4 g + ky + 2: the same LDS image read at a
//   row's distance, no copy per filter row.  Rows that lie outside the image of an output row (a block of small maps holds several images) are
//   read from an all-zero entry instead.  The step is written as 108 GAPS -- one matrix instruction, a hand-dealt slice of the other work, a
//   scheduling fence (see step()): one wave per SIMD issues in order, and nothing else hides behind the matrix instructions.
// Loader: lane lm = tid % 8 holds the channel PAIR 2 lm, 2 lm + 1 (8-byte loads; eight consecutive lanes read the 64 contiguous bytes of a
//   pixel), segment set tid / 8: four row-tiles = 16 pixels + the neighbour left and right of one image row (W = 32: half a row, W = 16: a row,
//   W = 8: two rows) -- 36 registers that hold the NEXT step's pixels while this step is contracted; threads tid / 8 < 2 W / 4 additionally one
//   row-tile (six pixels) of the halo row above or below the block.  A row-tile's staging is 13 groups of <= 5 vector instructions: t = B^T d
//   for both channels (12 plain fmas each), then per position one dword of hi parts (v_cvt_pk_f16_f32 of the two channels: no lane exchange)
//   and one of lo parts (v - hi by v_fma_mix_f32, exact), two positions of a plane per ds_write2st64_b32, then the requests for the step after next.
// Stage (LDS): [6 positions][(RB + 2) W / 4 + 1 entries, rounded up to eight][64 B], entry = (row slot, tile), the last one all zero; entry e lives
//   in slot r1_slot(e) (pairs of every second group of four swapped: the four loader threads of a write pass then fall on four bank quarters),
//   its four 16-byte pieces (plane, channel half) at piece ^ ((slot >> 2) & 3): a ds_read_b128 of 32 consecutive entries is conflict-free from
//   any even first entry (checked by enumeration over the instruction's lane groups).  Two stages, 64 KB apart (the other stage: one XOR).
// U (global): [Cin/16][Cout/64][18 slots = position * 3 + filter row][2 planes][64 cout][16 cin] fp16 + 4 floats of header (the factor that
//   undoes the power-of-two scaling first).
// Tail: two rounds (groups {0, 1}, {2, 3}); every wave parks its three positions' accumulators as they are ([64 row-tiles][6 positions][64
//   channels] fp32), and thread (4 channels, 16 consecutive pixels) forms A^T m from six 16-byte reads per row-tile, applies the epilogue of
//   idiff_conv2d_nhwc_f32 -- its switches as compile-time constants -- and stores 16 bytes per pixel.
// Measured (profiles/r05_wino1d_*.txt, HISTORY_r05.md 5): 1.03 - 1.23x winograd43h_kernel by shape, matrix cores 52 % busy, 1,120 lines from L2 per
// workgroup and step.
#include "wino_host.h"
#include <stdlib.h>
#include <type_traits>

namespace {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef unsigned int uintx4 __attribute__((ext_vector_type(4)));
typedef _Float16 halfx8 __attribute__((ext_vector_type(8)));
typedef float f2 __attribute__((ext_vector_type(2)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
// LDS by its 32-bit address: the K loop keeps complete addresses in registers (stage, entry, piece; positions are immediate offsets), so no
// instruction re-adds the allocation's base per access
typedef __attribute__((address_space(3))) char r1_lds_char;
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wint-to-pointer-cast"           // (the host pass sees 64-bit pointers; LDS pointers of the device pass are 32 bits wide)
typedef __attribute__((address_space(3))) halfx8 r1_lds_halfx8;
typedef __attribute__((address_space(3))) uint32_t r1_lds_u32;
__device__ __forceinline__ halfx8 r1_lds_read16(uint32_t at) { return *(const r1_lds_halfx8 *)at; }
__device__ __forceinline__ void r1_lds_write4(uint32_t at, uint32_t v) { *(r1_lds_u32 *)at = v; }
#pragma clang diagnostic pop

constexpr int R1_THREADS = 256;
constexpr int R1_COUT = PAIR_COUT;                                  // 64, 16: the bank is pair_bank_pack's (wino_host.h)
constexpr int R1_KC = PAIR_KC;
constexpr int R1_PIXELS = 512;                                     // output pixels of a workgroup
constexpr int R1_RT = R1_PIXELS / 4;                               // its row-tiles
constexpr int R1_NSLOT = 18;                                       // (position, filter row)
constexpr int R1_SLOT_BYTES = PAIR_SLOT_BYTES;                     // 4096
constexpr int R1_PLANE_BYTES = PAIR_PLANE_BYTES;                   // 2048
constexpr int R1_Z_BYTES = R1_RT * 4 * R1_COUT * 4;                // the tail's exchange: 131,072
constexpr size_t R1_LDS_BYTES = R1_Z_BYTES;
constexpr uint32_t R1_STAGE_STRIDE = 0x10000;                      // the two stages 64 KB apart: the other stage is one XOR away
constexpr uint32_t R1_INVALID = 0xFFFF8000u;                       // beyond any valid extent (the scalar offset is not range-checked)
constexpr int64_t R1_X_LIMIT = 0xFFFF0000ll;
constexpr int R1_BRING = 3;                                        // combinations of U requested ahead (register sets of 8)
static_assert(9 % R1_BRING == 0, "the ring of U registers must divide the nine combinations of a step");
constexpr int R1_STORE_AUX = 0;                                    // cache policy bits of the output stores: nt, sc1 and both with sc0 all
                                                                   // measured within noise of the default (profiles/r05_wino1d_loop_experiments.txt)

// Where entry e of a stage lives: the entries of every second group of four trade places in pairs.  The 32 lanes of one pass of a ds_write_b32
// are four loader threads' dwords of the entries e, e + 4, e + 8, e + 12 (32 bytes each); at e * 64 they would fall on two of the four
// 32-byte quarters of the 128 bytes the banks span (a two-way conflict on every stage write, SQ_LDS_BANK_CONFLICT = 24 % of the LDS cycles);
// the trade alternates the entries' parity and the four land on four quarters.  A fragment read covers both members of every pair, so its
// conflict-free pattern is unchanged.
__device__ __forceinline__ int r1_slot(int e) { return e ^ ((e >> 2) & 1); }

template <int W> struct R1Geo {
  static constexpr int TPR = W / 4;                                // row-tiles per image row
  static constexpr int RB = R1_PIXELS / W;                         // image rows per workgroup
  static constexpr int EZ = (RB + 2) * TPR;                        // stage entries: row slot 0 = the row above the block, RB + 1 = the row below, then the zero entry
  static constexpr int E = (EZ + 1 + 7) & ~7;                      // (whole groups of eight: r1_slot() stays inside)
  static constexpr int POS_BYTES = E * 64;
  static constexpr int STAGE_BYTES = 6 * POS_BYTES;
  static_assert(RB * TPR == R1_RT, "128 row-tiles per workgroup");
  static_assert(STAGE_BYTES <= R1_STAGE_STRIDE, "a stage inside its half of the LDS allocation");
  static_assert(5 * POS_BYTES < 65536, "positions are reached by the LDS instructions' immediate offset");
  static_assert(POS_BYTES % 256 == 0, "two positions of one entry: one ds_write2st64_b32");
};

struct Wino1dParams {
  const float *x;
  const float *u;
  float *out;
  int B, H, W, Cin, Cout;
  int rows_total, blocks_m, tiles_n, ngroup;
  uint32_t x_bytes, u_bytes, out_bytes, res_bytes;
  idiff_epilogue ep;
  int has_ep;
  const float *gn_gamma, *gn_beta;                 // the fused GroupNorm of wino1d_gn_kernel: [Cout] each, groups of gn_cpg channels
  int gn_cpg, gn_act;
  float gn_eps;
  const float *nl_coef;                            // wino1d_nl_kernel: [B][Cin][2] = (a, b) of the GroupNorm in FRONT of this convolution, x -> act(a x + b)
  uint32_t nl_bytes;
  float c_nb2, c_na2, c_nab2, c_a, c_b;            // the transform's constants as kernel arguments (SGPR operands of plain fmas)
  const float *x2;                                 // wino1d_nl2_kernel: input channels [c1, Cin) come from x2 [B, H W, Cin - c1], [0, c1) from x [B, H W, c1]
  uint32_t x2_bytes;
  int c1;
  int res_up2;                                     // wino1d_kernel<8|16|32>: ep.residual is the LOW-resolution residual [B, (H/2)(W/2), Cout] (pitch Cout,
  float up_w[16];                                  // res_bytes its extent), upsampled x2 in the tail by the polyphase weights up_w[phase y][phase x][u][v]
#ifdef IDIFF_W1D_STAMP
  uint64_t *stamps;                                // diagnostic build (scripts/wino1d_stamps.py): 8 ticks of 100 MHz per workgroup
#endif
};

// GN: the tail of wino1d_gn_kernel (GroupNorm + activation of the output inside the workgroup) instead of the epilogue's switches
// NL: the loader of wino1d_nl_kernel (0: none): the GroupNorm that PRODUCES the input, as one affine pair per (image, channel), (NL = 2:) + SiLU,
//     applied to the pixel registers in front of B^T d; W = 32 only (a block is half an image: one image's coefficients per workgroup)
// S2: the loader of wino1d_nl2_kernel: the input is cat[x, x2] along the channels, never written -- a K step (16 channels) lies in ONE source
//     (c1 % 16 == 0), so the source of a step is a wave-uniform choice of descriptor, channel offset and pitch; everything else is the NL kernel
template <int W, bool GN, int NL = 0, bool S2 = false>
__device__ __forceinline__ void r1_body(const Wino1dParams &p) {
  static_assert(NL == 0 || (W == 32 && !GN), "the norm in the loader: 32-pixel rows, the plain tail");
  static_assert(!S2 || NL != 0, "two sources: only with the norm in the loader");
  using G = R1Geo<W>;
  constexpr int TPR = G::TPR, RB = G::RB, POS = G::POS_BYTES, BRING = R1_BRING;
  extern __shared__ __attribute__((aligned(16))) float lds[];
#ifdef IDIFF_W1D_STAMP
  uint64_t st[8];
#define IDIFF_W1D_T(k) { __builtin_amdgcn_sched_barrier(0); st[k] = __builtin_amdgcn_s_memrealtime(); __builtin_amdgcn_sched_barrier(0); }
#else
#define IDIFF_W1D_T(k)
#endif
  IDIFF_W1D_T(0)
  char *const ldsb = reinterpret_cast<char *>(lds);
  const uint32_t lds0 = (uint32_t)(uintptr_t)(r1_lds_char *)ldsb;   // the allocation's LDS address
  const int nwg = p.blocks_m * p.tiles_n;
  int bid = blockIdx.x;
  {   // consecutive workgroups of the launch order land on different XCDs: give every XCD a contiguous range of the (row block, cout tile) order
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, local = bid >> 3;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + local;
  }
  const int per_group = p.blocks_m * p.ngroup;
  const int grp = bid / per_group, in_grp = bid - grp * per_group;
  const int tile_n = grp * p.ngroup + in_grp % p.ngroup, tile_m = in_grp / p.ngroup;
  const int row0 = tile_m * RB, n0 = tile_n * R1_COUT;            // first global image row (sample * H + y) of the block
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wh = wave & 1, ph = wave >> 1;

  const __amdgpu_buffer_rsrc_t rU = __builtin_amdgcn_make_buffer_rsrc((void *)p.u, 0, (int)p.u_bytes, 0x00020000);
  const uint32_t cin4 = (uint32_t)(S2 ? p.c1 : p.Cin) * 4u;        // bytes per pixel (S2: of the first source)
  const int roww = W * (int)cin4;                                  // bytes per image row
  const int nsteps = p.Cin / R1_KC;

  // ---------------------------------------------------------------- loader: thread = (channel pair, row segment)
  // Lane lm holds channels 2 lm and 2 lm + 1 (8-byte loads: eight consecutive lanes read the 64 contiguous bytes of a pixel), so the two halves of
  // every stage dword are in ONE lane and a value pair costs 2 conversions + 2 mixed fmas -- no exchange with a neighbouring lane, no selects.
  // Segment set lk: W = 64 / 32: a quarter / half of a row (16 pixels and their two neighbours), W = 16: row lk, W = 8 / 4: two / four whole rows -- four
  // row-tiles and 16 pixels (+ the neighbours left and right) per thread and step; lk < 2 W / 4 additionally one row-tile of a halo row.
  constexpr int TS = TPR < 4 ? TPR : 4;                            // row-tiles per segment
  constexpr int NSEG = 4 / TS;                                     // row segments of a thread
  constexpr int NPX = 4 * TS + 2;                                  // its pixels, the one to the left and the one to the right included
  const int lm = tid & 7, lk = tid >> 3;
  // base one pixel to the LEFT: offset v + j * cin4 is the segment's pixel j - 1 ... (the range check covers the vector offset only)
  const __amdgpu_buffer_rsrc_t rXm = __builtin_amdgcn_make_buffer_rsrc((void *)(p.x - (S2 ? p.c1 : p.Cin)), 0, (int)(p.x_bytes + cin4), 0x00020000);
  uint32_t v_main, v_halo;
  // S2: the second source's pitch, descriptor (the same construction, its own extent) and per-lane offsets (pixel index * pitch + lm * 8:
  // equal to the first source's only where c1 = Cin - c1), and the first K step that reads it
  const uint32_t cin4b = S2 ? (uint32_t)(p.Cin - p.c1) * 4u : 0u;
  const int n1 = S2 ? p.c1 / R1_KC : 0;
  const __amdgpu_buffer_rsrc_t rXm2 =
      __builtin_amdgcn_make_buffer_rsrc((void *)(S2 ? p.x2 - (p.Cin - p.c1) : p.x), 0, S2 ? (int)(p.x2_bytes + cin4b) : 0, 0x00020000);
  uint32_t v_main2 = R1_INVALID, v_halo2 = R1_INVALID;
  bool m_l, m_r, h_c0, h_c5;
  int e_halo;
  {
#ifdef IDIFF_W1D_DIAG_SAME_X       // timing-only build: every workgroup reads the first block's pixels (L2 hits instead of HBM misses)
    const int rho = (W >= 32 ? lk / (W / 16) : NSEG * lk);
#else
    const int rho = row0 + (W >= 32 ? lk / (W / 16) : NSEG * lk);
#endif
    const int xf = W >= 32 ? 16 * (lk % (W / 16)) : 0;            // first pixel of my first tile
    v_main = rho < p.rows_total ? (uint32_t)rho * (uint32_t)roww + (uint32_t)xf * cin4 + (uint32_t)lm * 8u : R1_INVALID;
    m_l = xf > 0; m_r = xf + 4 * TS < W;                           // the neighbours are pixels of the row (else the zero padding)
    const bool part = lk < 2 * TPR, top = lk < TPR;
    const int tx = top ? lk : lk - TPR;
    const int hr = top ? row0 - 1 : row0 + RB;                     // the halo row: inside the same image as the block's first / last row?
    const bool valid = part && (top ? (row0 % p.H != 0) : ((row0 + RB) % p.H != 0 && row0 + RB < p.rows_total));
    v_halo = valid ? (uint32_t)hr * (uint32_t)roww + (uint32_t)(4 * tx) * cin4 + (uint32_t)lm * 8u : R1_INVALID;
    h_c0 = tx > 0; h_c5 = tx + 1 < TPR;
    if constexpr (S2) {
      if (rho < p.rows_total) v_main2 = (uint32_t)rho * (uint32_t)W * cin4b + (uint32_t)xf * cin4b + (uint32_t)lm * 8u;
      if (valid) v_halo2 = (uint32_t)hr * (uint32_t)W * cin4b + (uint32_t)(4 * tx) * cin4b + (uint32_t)lm * 8u;
    }
    e_halo = part ? (top ? tx : (RB + 1) * TPR + tx) : G::EZ;      // threads without a halo tile transform zeros into the zero entry
  }
  // does any lane of this wave hold a halo tile that is inside the image?  (W = 32: wave 0 the row above, wave 1 the row below; else wave 0 both)
  const bool halo_wave = __builtin_amdgcn_readfirstlane((int)__builtin_amdgcn_ballot_w64(v_halo != R1_INVALID)) != 0
                         || __builtin_amdgcn_readfirstlane((int)(__builtin_amdgcn_ballot_w64(v_halo != R1_INVALID) >> 32)) != 0;
  const int e_main0 = TPR + 4 * lk;                                // my four row-tiles' entries: consecutive
  f2 px[NSEG][NPX];                                                // (channel 2 lm, channel 2 lm + 1) per pixel
  f2 hp[6];
#pragma unroll
  for (int g = 0; g < NSEG; ++g)
#pragma unroll
    for (int j = 0; j < NPX; ++j) px[g][j] = f2{0.f, 0.f};
  uint32_t invalid_s = R1_INVALID;
  // pixels [j0, j1] of segment g for K step `step` (clamped: the last stages request their own step again, nobody reads it)
  // S2: the (clamped) step's source, chosen by the wave-uniform `second` (scalar selects; one vector select for the lane's offset): the clamp
  // stays inside the second source, whose last step is the convolution's last
  auto fetch_px = [&](int g, int j0, int j1, int step) __attribute__((always_inline)) {
    if constexpr (S2) {
      const int st = min(step, nsteps - 1);
      const bool second = st >= n1;
      const int choff = (second ? st - n1 : st) * (R1_KC * 4);
      const int pitch = (int)(second ? cin4b : cin4);
      const uint32_t vm = second ? v_main2 : v_main;
      asm volatile("" : "+s"(invalid_s));
#pragma unroll
      for (int j = j0; j <= j1; ++j) {
        const uint32_t vo = j == 0 ? (m_l ? vm : invalid_s) : (j == NPX - 1 ? (m_r ? vm : invalid_s) : vm);
        px[g][j] = __builtin_bit_cast(f2, __builtin_amdgcn_raw_buffer_load_b64(second ? rXm2 : rXm, (int)vo, choff + j * pitch, 0));
      }
      return;
    }
    const int choff = min(step, nsteps - 1) * (R1_KC * 4);
    asm volatile("" : "+s"(invalid_s));
#pragma unroll
    for (int j = j0; j <= j1; ++j) {
      if (W < 32 && (j == 0 || j == NPX - 1)) continue;            // always the padding
      const uint32_t vo = j == 0 ? (m_l ? v_main : invalid_s) : (j == NPX - 1 ? (m_r ? v_main : invalid_s) : v_main);
      px[g][j] = __builtin_bit_cast(f2, __builtin_amdgcn_raw_buffer_load_b64(rXm, (int)vo, choff + g * roww + j * (int)cin4, 0));
    }
  };
  auto fetch_hp = [&](int j0, int j1, int step) __attribute__((always_inline)) {
    if constexpr (S2) {
      const int st = min(step, nsteps - 1);
      const bool second = st >= n1;
      const int choff = (second ? st - n1 : st) * (R1_KC * 4);
      const int pitch = (int)(second ? cin4b : cin4);
      const uint32_t vh = second ? v_halo2 : v_halo;
      asm volatile("" : "+s"(invalid_s));
#pragma unroll
      for (int j = j0; j <= j1; ++j) {
        const uint32_t vo = j == 0 ? (h_c0 ? vh : invalid_s) : (j == 5 ? (h_c5 ? vh : invalid_s) : vh);
        hp[j] = __builtin_bit_cast(f2, __builtin_amdgcn_raw_buffer_load_b64(second ? rXm2 : rXm, (int)vo, choff + j * pitch, 0));
      }
      return;
    }
    const int choff = min(step, nsteps - 1) * (R1_KC * 4);
    asm volatile("" : "+s"(invalid_s));
#pragma unroll
    for (int j = j0; j <= j1; ++j) {
      const uint32_t vo = j == 0 ? (h_c0 ? v_halo : invalid_s) : (j == 5 ? (h_c5 ? v_halo : invalid_s) : v_halo);
      hp[j] = __builtin_bit_cast(f2, __builtin_amdgcn_raw_buffer_load_b64(rXm, (int)vo, choff + j * (int)cin4, 0));
    }
  };
  // where my hi dword of row-tile i (4: the halo tile) goes in stage 0, position 0 (LDS address); the lo dword: bit 5 flipped; stage 1: bit 16
  uint32_t wtab[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int e = r1_slot(i < 4 ? e_main0 + i : e_halo);
    wtab[i] = lds0 + (uint32_t)(e * 64 + (((lm >> 2) ^ ((e >> 2) & 3)) << 4) + (lm & 3) * 4);
  }
  const float k_nb2 = p.c_nb2, k_na2 = p.c_na2, k_nab2 = p.c_nab2, k_a = p.c_a, k_b = p.c_b;
#ifdef IDIFF_W1D_DIAG_NO_VWRITE
  uint32_t diag_sink = 0;
#endif
  // The staging of ONE row-tile (two channels) in 13 groups of at most five vector instructions, the units the K loop deals over its gaps:
  //   0 - 4   t = B^T d for both channels (12 operations each, the arithmetic of winograd43_shared.h's f4_bt)
  //   5 - 10  position grp - 5: the two channels' values -> one dword of hi parts, one of lo parts (v - hi in one mixed-precision fma each), stored
  //   11, 12  the pixels no later tile reads are requested for K step `next`
  float t_pe[2], t_po[2], t_re[2], t_ro[2], t_s04[2], t_s15[2], tv[2][6];
  uint32_t w_hi = 0, w_lo = 0, p_hi = 0, p_lo = 0;
  auto tile_group = [&](auto ii, auto gg, uint32_t wbase, int next) __attribute__((always_inline)) {
    constexpr int i = decltype(ii)::value, grp = decltype(gg)::value;
    constexpr int sg = i < 4 ? i / TS : 0, t = i < 4 ? i % TS : 0;
    auto d = [&](int c, int j) __attribute__((always_inline)) { return i < 4 ? px[sg][4 * t + j][c] : hp[j][c]; };
    auto head = [&](int c, int part) __attribute__((always_inline)) {          // the twelve operations of channel c in five parts
      if (part == 0) { t_pe[c] = fmaf(k_nb2, d(c, 2), d(c, 4)); t_po[c] = fmaf(k_nb2, d(c, 1), d(c, 3)); t_re[c] = fmaf(k_na2, d(c, 2), d(c, 4)); }
      if (part == 1) { t_ro[c] = fmaf(k_na2, d(c, 1), d(c, 3)); t_s04[c] = d(c, 0) + d(c, 4); t_s15[c] = d(c, 1) + d(c, 5); }
      if (part == 2) { tv[c][0] = fmaf(k_nab2, d(c, 2), t_s04[c]); tv[c][5] = fmaf(k_nab2, d(c, 3), t_s15[c]); }
      if (part == 3) { tv[c][1] = fmaf(k_a, t_po[c], t_pe[c]); tv[c][2] = fmaf(-k_a, t_po[c], t_pe[c]); }
      if (part == 4) { tv[c][3] = fmaf(k_b, t_ro[c], t_re[c]); tv[c][4] = fmaf(-k_b, t_ro[c], t_re[c]); }
    };
    if (grp == 0) { w_hi = wtab[i] ^ wbase; w_lo = w_hi ^ 32u; head(0, 0); head(0, 1); }     // (wbase: 0 or the stage stride)
    if (grp == 1) { head(0, 2); head(0, 3); }
    if (grp == 2) { head(0, 4); head(1, 0); }
    if (grp == 3) { head(1, 1); head(1, 2); }
    if (grp == 4) { head(1, 3); head(1, 4); }
    if (grp >= 5 && grp <= 10) {
      // positions in pairs (0, 1), (2, 3), (4, 5): the first group of a pair cuts its position, the second cuts the other and stores both -- two
      // dwords of one plane at one base and a distance that is a multiple of 256 bytes go out as ONE ds_write2st64_b32
      constexpr int pos = grp >= 5 && grp <= 10 ? grp - 5 : 0;
      const f2 vv = {tv[0][pos], tv[1][pos]};
      const uint32_t xh = __builtin_bit_cast(uint32_t, __builtin_convertvector(vv, h2));
      f2 rest;                                                      // v - hi in one mixed-precision instruction per channel (exact)
      asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(rest.x) : "v"(xh), "v"(vv.x));
      asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(rest.y) : "v"(xh), "v"(vv.y));
      const uint32_t xl = __builtin_bit_cast(uint32_t, __builtin_convertvector(rest, h2));
      if ((pos & 1) == 0) { p_hi = xh; p_lo = xl; }
      else {
#ifdef IDIFF_W1D_DIAG_NO_VWRITE    // timing-only build: the pairs are summed into one register instead of written
        diag_sink += xh + xl + p_hi + p_lo;
#else
        r1_lds_write4(w_hi + (pos - 1) * POS, p_hi); r1_lds_write4(w_hi + pos * POS, xh);
        r1_lds_write4(w_lo + (pos - 1) * POS, p_lo); r1_lds_write4(w_lo + pos * POS, xl);
#endif
      }
    }
#ifdef IDIFF_W1D_DIAG_NO_XLOAD     // timing-only build: the input is loaded for the first two steps only
    if (next <= 1)
#endif
    if (grp >= 11) {
      if (i < 4) {
        constexpr int j0 = 4 * t, j1 = t == TS - 1 ? 4 * t + 5 : 4 * t + 3, mid = (j0 + j1) / 2;
        if (grp == 11) fetch_px(sg, j0, mid, next); else fetch_px(sg, mid + 1, j1, next);
      } else {
        if (grp == 11) fetch_hp(0, 2, next); else fetch_hp(3, 5, next);
      }
    }
  };
  // all of one tile at once (the first step's stage, before the loop)
  auto tile_all = [&](auto ii, uint32_t wbase, int next) __attribute__((always_inline)) {
    tile_group(ii, std::integral_constant<int, 0>(), wbase, next); tile_group(ii, std::integral_constant<int, 1>(), wbase, next);
    tile_group(ii, std::integral_constant<int, 2>(), wbase, next); tile_group(ii, std::integral_constant<int, 3>(), wbase, next);
    tile_group(ii, std::integral_constant<int, 4>(), wbase, next); tile_group(ii, std::integral_constant<int, 5>(), wbase, next);
    tile_group(ii, std::integral_constant<int, 6>(), wbase, next); tile_group(ii, std::integral_constant<int, 7>(), wbase, next);
    tile_group(ii, std::integral_constant<int, 8>(), wbase, next); tile_group(ii, std::integral_constant<int, 9>(), wbase, next);
    tile_group(ii, std::integral_constant<int, 10>(), wbase, next); tile_group(ii, std::integral_constant<int, 11>(), wbase, next);
    tile_group(ii, std::integral_constant<int, 12>(), wbase, next);
    __builtin_amdgcn_sched_barrier(0);
  };

  // ---------------------------------------------------------------- NL: act(a x + b) on the pixel registers
  // The block's rows belong to ONE image (H % RB == 0, checked by the launcher), so a K step needs 16 (a, b) pairs, and lane lm the two of its
  // channel pair: one 16-byte load per lane and step.  Every pixel register is rewritten in place exactly once between its arrival and the
  // staging of the first row-tile that reads it (a tile's pixels 4, 5 are the next tile's 0, 1: row-tile 0 owns six pixels, the others four),
  // in UNITS of one transcendental each (a pixel = two channels = four units), the K loop deals one unit to a gap:
  //   0  z = a x + b (both channels), e0 = 2^(-log2(e) z0)     1  e1, 1 + e (both)     2  1 / (1 + e0)     3  1 / (1 + e1), x = z / (1 + e)
  // act_apply's SiLU (v_exp_f32, v_rcp_f32) on the same argument.  The padding is zero AFTER the norm (silu(b) != 0): the neighbour pixels of
  // the row's first and last segment and of the halo row's first and last tile -- loaded as zeros from beyond the descriptor -- are set to
  // zero again by unit 3; rows outside the image are never staged (the fragments read the zero entry, which no unit touches).
  const __amdgpu_buffer_rsrc_t rC = __builtin_amdgcn_make_buffer_rsrc((void *)p.nl_coef, 0, NL != 0 ? (int)p.nl_bytes : 0, 0x00020000);
  const uint32_t c_lane = ((uint32_t)(row0 / p.H) * (uint32_t)p.Cin + 2u * (uint32_t)lm) * 8u;
  float4 kn = make_float4(0.f, 0.f, 0.f, 0.f);                    // the pairs requested for the step after the one in ka, kb
  float ka[2] = {0.f, 0.f}, kb[2] = {0.f, 0.f}, az[2] = {0.f, 0.f}, ae[2] = {0.f, 0.f};
  auto fetch_coef = [&](int step) __attribute__((always_inline)) {
    kn = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rC, (int)c_lane, min(step, nsteps - 1) * (R1_KC * 8), 0));
  };
  auto take_coef = [&]() __attribute__((always_inline)) { ka[0] = kn.x; kb[0] = kn.y; ka[1] = kn.z; kb[1] = kn.w; };
  constexpr int NL_UNITS = 4 * (NPX + 6), NL_MAIN = 4 * NPX;       // 96 units, the halo tile's six pixels last
  auto act_unit = [&](auto uu) __attribute__((always_inline)) {
    constexpr int u = decltype(uu)::value, pi = u >> 2, q = u & 3;
    f2 &d = pi < NPX ? px[0][pi < NPX ? pi : 0] : hp[pi >= NPX ? pi - NPX : 0];
    const bool keep = pi == 0 ? m_l : pi == NPX - 1 ? m_r : pi == NPX ? h_c0 : pi == NPX + 5 ? h_c5 : true;
    constexpr bool edge = pi == 0 || pi == NPX - 1 || pi == NPX || pi == NPX + 5;
    if (NL == 1) {
      if (q == 0) {
        d.x = fmaf(ka[0], d.x, kb[0]); d.y = fmaf(ka[1], d.y, kb[1]);
        if (edge) { d.x = keep ? d.x : 0.f; d.y = keep ? d.y : 0.f; }
      }
    } else {
      if (q == 0) {
        az[0] = fmaf(ka[0], d.x, kb[0]); az[1] = fmaf(ka[1], d.y, kb[1]);
        ae[0] = __builtin_amdgcn_exp2f(az[0] * -1.44269504088896340736f); ae[1] = az[1] * -1.44269504088896340736f;
      }
      if (q == 1) { ae[1] = __builtin_amdgcn_exp2f(ae[1]); ae[0] += 1.0f; ae[1] += 1.0f; }
      if (q == 2) ae[0] = __builtin_amdgcn_rcpf(ae[0]);
      if (q == 3) {
        ae[1] = __builtin_amdgcn_rcpf(ae[1]);
        d.x = az[0] * ae[0]; d.y = az[1] * ae[1];
        if (edge) { d.x = keep ? d.x : 0.f; d.y = keep ? d.y : 0.f; }
      }
    }
  };
  // units [U0, U1) at once (before the loop); the halo tile's only in the waves that hold one
  auto act_range = [&](auto u0, auto u1) __attribute__((always_inline)) {
    constexpr int U0 = decltype(u0)::value, U1 = decltype(u1)::value;
    auto each = [&](auto self, auto uu) __attribute__((always_inline)) {
      constexpr int u = decltype(uu)::value;
      if constexpr (u < U1) {
        if (u < NL_MAIN) act_unit(uu); else if (halo_wave) act_unit(uu);
        self(self, std::integral_constant<int, u + 1>());
      }
    };
    each(each, std::integral_constant<int, U0>());
    __builtin_amdgcn_sched_barrier(0);
  };

  // ---------------------------------------------------------------- contraction
  floatx16 acc[4][3];
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[g][i][r] = 0.f;
  const int fr = lane & 31, fh = lane >> 5;
  // V fragment of (group g, filter row ky): the entry of row-tile 32 g + fr one row up / at / one row down, or the zero entry where that row
  // is outside the output row's image; piece fh of plane 0, plane 1 lies at the address with bit 5 flipped
  uint32_t ra[4][3];                                  // LDS addresses (plane 0; plane 1: bit 5 flipped) in the stage being read: toggled to the other stage after every step
  {
    const int y0 = row0 % p.H;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int m = 32 * g + fr, r = m / TPR, tx = m % TPR;
      const int y = (y0 + r) % p.H;
      const bool inside = row0 + r < p.rows_total;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const bool ok = inside && (ky == 1 || (ky == 0 ? y > 0 : y + 1 < p.H));
        const int e = r1_slot(ok ? (r + ky) * TPR + tx : G::EZ);
        ra[g][ky] = lds0 + (uint32_t)(ph * 3 * POS + e * 64 + ((fh ^ ((e >> 2) & 3)) << 4));
      }
    }
  }
  const uint32_t u_lane = (uint32_t)((wh * 32 + fr) * (R1_KC * 2) + fh * 16);
  halfx8 bh[BRING], bl[BRING];
  auto load_b = [&](int c, int step) __attribute__((always_inline)) {
    const int soff = ((step * p.tiles_n + tile_n) * R1_NSLOT + 9 * ph + c) * R1_SLOT_BYTES;     // slot = (3 ph + c / 3) * 3 + c % 3
    bh[c % BRING] = __builtin_bit_cast(halfx8, __builtin_amdgcn_raw_buffer_load_b128(rU, (int)u_lane, soff, 0));
    bl[c % BRING] = __builtin_bit_cast(halfx8, __builtin_amdgcn_raw_buffer_load_b128(rU, (int)u_lane + R1_PLANE_BYTES, soff, 0));
  };
  // A step: nine combinations c = (position 3 ph + c / 3, filter row c % 3), each twelve matrix instructions on four V fragments read one
  // combination ahead and a U fragment requested BRING ahead.  One wave per SIMD issues in order: vector work placed behind the matrix
  // instructions would start when the last of them has been issued.  So the step is written as 108 GAPS -- one matrix instruction, then at
  // most ~five other instructions that fit in the 32 cycles it runs, then a scheduling fence -- and everything else is dealt over them by hand:
  //   gaps 1, 2, 6, 9 of a combination: two LDS reads each of the NEXT combination's V fragments (plane 0 first: its products come first)
  //   gap 4: the two U loads
  //   gaps 0, 3, 5, 7, 8, 10, 11 (and 1, 2, 6, 9 of the last combination): the next staging group -- 4 x 13 for my row-tiles, then 13 for the halo tile.
  auto step = [&](int s, auto last) __attribute__((always_inline)) {
    constexpr bool LAST = decltype(last)::value;
    const uint32_t wbase = (s & 1) ? 0u : R1_STAGE_STRIDE;         // the stage being written: the one not read
    halfx8 ah[2][4], al[2][4];
    auto rd_hi = [&](int c, int g) __attribute__((always_inline)) { ah[c & 1][g] = r1_lds_read16(ra[g][c % 3] + (c / 3) * POS); };
    auto rd_lo = [&](int c, int g) __attribute__((always_inline)) { al[c & 1][g] = r1_lds_read16((ra[g][c % 3] ^ 32u) + (c / 3) * POS); };
#pragma unroll
    for (int g = 0; g < 4; ++g) { rd_hi(0, g); rd_lo(0, g); }
    auto slice = [&](auto cc, auto kk) __attribute__((always_inline)) {
      constexpr int c = decltype(cc)::value, k = decltype(kk)::value;
      if (c + 1 < 9) {
        if (k == 1) { rd_hi(c + 1, 0); rd_hi(c + 1, 1); }
        if (k == 2) { rd_hi(c + 1, 2); rd_hi(c + 1, 3); }
        if (k == 6) { rd_lo(c + 1, 0); rd_lo(c + 1, 1); }
        if (k == 9) { rd_lo(c + 1, 2); rd_lo(c + 1, 3); }
      }
      if (k == 4) {
#ifdef IDIFF_W1D_DIAG_NO_BLOAD     // timing-only build: U is loaded for the first step only
        if (s == 0) { if (c + BRING < 9) load_b(c + BRING, s); }
#else
        if (c + BRING < 9) load_b(c + BRING, s); else if (!LAST) load_b(c + BRING - 9, s + 1);
#endif
      }
#ifndef IDIFF_W1D_DIAG_NO_STAGE    // timing-only build: no transform, no stage writes, no input loads after the prologue
      if (!LAST) {
        // the staging slot of this gap: 7 per combination, 11 in the last one
        constexpr int idx7 = k == 0 ? 0 : k == 3 ? 1 : k == 5 ? 2 : k == 7 ? 3 : k == 8 ? 4 : k == 10 ? 5 : k == 11 ? 6 : -1;
        constexpr int idx11 = k < 4 ? k : (k == 4 ? -1 : k - 1);
        constexpr int slot = c < 8 ? (idx7 < 0 ? -1 : 7 * c + idx7) : (idx11 < 0 ? -1 : 56 + idx11);
        if (slot >= 0 && slot < 52)
          tile_group(std::integral_constant<int, (slot >= 0 && slot < 52 ? slot / 13 : 0)>(), std::integral_constant<int, (slot >= 0 ? slot % 13 : 0)>(), wbase, s + 2);
        // the halo tile: only in the waves that hold one (a wave-uniform branch; the others' gaps stay empty)
        if (slot >= 52 && slot < 65 && halo_wave)
          tile_group(std::integral_constant<int, 4>(), std::integral_constant<int, (slot >= 52 ? slot - 52 : 0)>(), wbase, s + 2);
      }
#endif
      if constexpr (NL != 0) {
        // The norm's units, one per gap at most, 96 over the 108: unit u in gap (81 + 9 u / 8) mod 108.  Row-tile 0's pixels (units 0 .. 23: gaps
        // 81 .. 106) are those of the step after next, requested in gaps 19 .. 44 of this step and staged from gap 0 of the next; row-tiles
        // 1, 2, 3 (gaps 0 .. 16, 18 .. 34, 36 .. 52) and the halo tile (54 .. 79) are done before their staging begins in gaps 23, 46, 68, 91
        // and after their request, 57 gaps and more earlier.  The pairs change between the halo tile's last unit and row-tile 0's first.
        if (!LAST) {
          constexpr int gi = 12 * c + k, rel = (gi + 108 - 81) % 108, u = (rel * 8 + 8) / 9;
          if constexpr (u < NL_UNITS && (u * 9) / 8 == rel) {
            if (u < NL_MAIN) act_unit(std::integral_constant<int, u>()); else if (halo_wave) act_unit(std::integral_constant<int, u>());
          }
          if (gi == 40) fetch_coef(s + 2);
          if (gi == 80) take_coef();
        }
      }
    };
    auto combo = [&](auto cc) __attribute__((always_inline)) {
      constexpr int c = decltype(cc)::value;
      constexpr int pi = c / 3;
      const halfx8 yh = bh[c % BRING], yl = bl[c % BRING];
      auto gap = [&](auto kk) __attribute__((always_inline)) {
        constexpr int k = decltype(kk)::value, g = k & 3, pr = k >> 2;       // products: plane 0 x plane 0, plane 0 x plane 1, plane 1 x plane 0
#ifdef IDIFF_W1D_DIAG_NO_MFMA      // timing-only build: the operands are consumed by one vector instruction instead
        acc[g][pi][0] += (float)(pr == 2 ? al[c & 1][g] : ah[c & 1][g])[0] + (float)(pr == 1 ? yl : yh)[0];
#else
        acc[g][pi] = __builtin_amdgcn_mfma_f32_32x32x16_f16(pr == 2 ? al[c & 1][g] : ah[c & 1][g], pr == 1 ? yl : yh, acc[g][pi], 0, 0, 0);
#endif
        slice(cc, kk);
        __builtin_amdgcn_sched_barrier(0);
      };
      gap(std::integral_constant<int, 0>()); gap(std::integral_constant<int, 1>()); gap(std::integral_constant<int, 2>());
      gap(std::integral_constant<int, 3>()); gap(std::integral_constant<int, 4>()); gap(std::integral_constant<int, 5>());
      gap(std::integral_constant<int, 6>()); gap(std::integral_constant<int, 7>()); gap(std::integral_constant<int, 8>());
      gap(std::integral_constant<int, 9>()); gap(std::integral_constant<int, 10>()); gap(std::integral_constant<int, 11>());
    };
    __builtin_amdgcn_sched_barrier(0);
    combo(std::integral_constant<int, 0>()); combo(std::integral_constant<int, 1>()); combo(std::integral_constant<int, 2>());
    combo(std::integral_constant<int, 3>()); combo(std::integral_constant<int, 4>()); combo(std::integral_constant<int, 5>());
    combo(std::integral_constant<int, 6>()); combo(std::integral_constant<int, 7>()); combo(std::integral_constant<int, 8>());
#ifndef IDIFF_W1D_DIAG_NO_BARRIER  // timing-only build (a race by construction): what the step barrier and the waves' skew at it cost
    __syncthreads();
#endif
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) ra[g][ky] ^= R1_STAGE_STRIDE;
  };

  // the zero entry of both stages
  if (tid < 192) {
    const int b = tid / 96, rem = tid - 96 * b;
    *reinterpret_cast<uint32_t *>(ldsb + b * R1_STAGE_STRIDE + (rem >> 4) * POS + r1_slot(G::EZ) * 64 + (rem & 15) * 4) = 0u;
  }
#pragma unroll
  for (int c = 0; c < BRING; ++c) load_b(c, 0);
#pragma unroll
  for (int g = 0; g < NSEG; ++g) fetch_px(g, 0, NPX - 1, 0);
  fetch_hp(0, 5, 0);
#ifdef IDIFF_W1D_STAMP
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
  IDIFF_W1D_T(1)                                     // first operands arrived
  if constexpr (NL != 0) {
    fetch_coef(0); take_coef();
    act_range(std::integral_constant<int, 0>(), std::integral_constant<int, NL_UNITS>());
  }
  tile_all(std::integral_constant<int, 0>(), 0u, 1); tile_all(std::integral_constant<int, 1>(), 0u, 1); tile_all(std::integral_constant<int, 2>(), 0u, 1);
  tile_all(std::integral_constant<int, 3>(), 0u, 1);
  if (halo_wave) tile_all(std::integral_constant<int, 4>(), 0u, 1);
  if constexpr (NL != 0) {   // row-tile 0's pixels of step 1, which the loop's first step stages from its first gap on
    fetch_coef(1); take_coef();
    act_range(std::integral_constant<int, 0>(), std::integral_constant<int, 24>());
  }
  __syncthreads();
  IDIFF_W1D_T(2)
  if (NL == 0 || nsteps > 1) {                        // at least two steps (Cin >= 32, checked by the launcher); the NL kernel also takes one
    int s = 0;
    do step(s, std::false_type()); while (++s + 1 < nsteps);
  }
  step(nsteps - 1, std::true_type());
  IDIFF_W1D_T(3)
#ifdef IDIFF_W1D_DIAG_NO_VWRITE
  if (diag_sink == 12345u) ldsb[tid] = 1;
#endif

  // ---------------------------------------------------------------- tail
  // Two rounds, groups {0, 1} then {2, 3} (64 row-tiles each).  A wave PARKS its three positions' accumulators as they stand --
  // zr[row-tile][position][cout], 98,304 B -- and after a barrier thread (4 channels, 4 row-tiles = 16 consecutive pixels) reads the six
  // positions of a row-tile (six 16-byte reads), forms A^T m, applies the epilogue and stores 16 bytes per pixel.  (The first form had each
  // wave mix its positions into four partial outputs, park half and read - add - write the other half on top of the partner's: a third more
  // LDS writes, at 64 B per clock, and 128 dependent LDS round trips per lane: 72.4 -> 69.9 ms per forward with this one.)
  const float descale = p.u[(int64_t)R1_NSLOT * p.Cin * p.Cout];
  const idiff_epilogue &ep = p.ep;
  const bool has_ep = p.has_ep != 0;
  // accumulator register `reg` of lane l is row-tile (reg & 3) + 8 (reg >> 2) + 4 (l >> 5) of its group, cout wh * 32 + (l & 31)
  float *zbase = lds + (size_t)(4 * (lane >> 5)) * 6 * R1_COUT + (size_t)(3 * ph) * R1_COUT + wh * 32 + (lane & 31);
  auto park = [&](auto grp) __attribute__((always_inline)) {
    constexpr int GI = decltype(grp)::value;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      float *zp = zbase + (size_t)(32 * (GI & 1) + (reg & 3) + 8 * (reg >> 2)) * 6 * R1_COUT;
      zp[0] = acc[GI][0][reg]; zp[R1_COUT] = acc[GI][1][reg]; zp[2 * R1_COUT] = acc[GI][2][reg];
    }
  };
  using I0 = std::integral_constant<int, 0>; using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2>; using I3 = std::integral_constant<int, 3>;
  // the finishing thread: channels n .. n + 3 of row-tiles 64 round + 4 tl .. + 3: 16 consecutive pixels of one sample
  const int cq = tid & 15, tl = tid >> 4;
  const int n = n0 + 4 * cq;
#ifdef IDIFF_W1D_DIAG_PLAIN_EP      // timing-only build: the epilogue's switches as compile-time constants (bias only)
  const bool has_res = false, scaled = false, want_stats = false;
  const int act = (int)IDIFF_ACT_NONE;
#else
  const bool has_res = has_ep && ep.residual != nullptr;
  const bool scaled = has_ep && (ep.out_scale != 1.f || ep.rowscale != nullptr);
  const int act = has_ep ? ep.act : (int)IDIFF_ACT_NONE;
  const bool want_stats = has_ep && ep.colstats != nullptr;
#endif
  const __amdgpu_buffer_rsrc_t rO = __builtin_amdgcn_make_buffer_rsrc((void *)p.out, 0, (int)p.out_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rR = __builtin_amdgcn_make_buffer_rsrc((void *)ep.residual, 0, (int)p.res_bytes, 0x00020000);
  const int ld_res = (int)ep.ld_residual;
  float4 bias4 = make_float4(0.f, 0.f, 0.f, 0.f);
  if (has_ep && ep.bias) bias4 = *reinterpret_cast<const float4 *>(ep.bias + n);
  // (the last step ended with a barrier: nobody reads the stages any more)
  if constexpr (GN) {
    // The fused GroupNorm (GN): a round is 256 consecutive pixels = whole images (H W divides 256, checked by the launcher) and the tile's 64
    // channels are whole groups, so every (image, group) the norm needs is inside this round of this workgroup.  The thread keeps its 16 pixels
    // x 4 channels of descale * A^T m + bias + rowbias in registers (the residual's 64 are free: no residual here), and the sets are reduced
    // twice -- the sum for the mean, then the sum of squares about that mean over the same registers (no cancellation whatever the channels'
    // offset), both in fp64 as the column sums are: the thread's 16 pixels; the group's channels in neighbouring lanes (cq = lane & 15); the
    // image's thread rows tl = 4 wave + (lane >> 4): two lane exchanges inside the wave, and for images of 128 / 256 pixels (two / four waves)
    // one exchange through the LDS the parked accumulators leave free.  Every lane of a set adds the same values in the same order, so all
    // of them normalise with the same bits.  Then y = act((v - mean) * (rstd * gamma) + beta), gn_apply_rows_kernel's expression, and the
    // same 16-byte stores.  Samples beyond B in a partial last block are computed on zeros and their stores dropped (ooff: R1_INVALID).
    const int gn_cpg = p.gn_cpg;
    const int gn_span = (p.H * W) >> 4;                               // thread rows per image: 1, 2, 4 (one wave), 8, 16
    double *const gn_red = reinterpret_cast<double *>(ldsb + 6 * R1_RT / 2 * R1_COUT * 4);        // behind a round's parked accumulators (98,304 B)
    static_assert(6 * R1_RT / 2 * R1_COUT * 4 + 2 * 4 * 16 * 4 * 8 <= R1_Z_BYTES, "the statistics' exchange inside the allocation");
    // t[0 .. N - 1] summed over the lanes of my (image, group); N = 1: one group per thread (gn_cpg >= 4), N = 4: a value per channel (gn_cpg 1, 2)
    auto gn_reduce = [&](auto n_c, double *t, int pass) __attribute__((always_inline)) {
      constexpr int N = decltype(n_c)::value;
      if (N == 1) { for (int o = 1; o < (gn_cpg >> 2); o <<= 1) t[0] += __shfl_xor(t[0], o, 64); }
      else if (gn_cpg == 2) { t[0] += t[1]; t[1] = t[0]; t[2] += t[3]; t[3] = t[2]; }
      if (gn_span >= 2) {
#pragma unroll
        for (int e = 0; e < N; ++e) t[e] += __shfl_xor(t[e], 16, 64);
      }
      if (gn_span >= 4) {
#pragma unroll
        for (int e = 0; e < N; ++e) t[e] += __shfl_xor(t[e], 32, 64);
      }
      if (gn_span >= 8) {                                              // (uniform over the workgroup: H is a kernel argument)
        double *area = gn_red + pass * (4 * 16 * 4);                   // one area per pass: the next pass writes while this one is still read
        if (lane < 16) {
#pragma unroll
          for (int e = 0; e < N; ++e) area[(wave * 16 + lane) * 4 + e] = t[e];
        }
        __syncthreads();
        const int nw = gn_span >> 2, w0 = wave & ~(nw - 1);            // the image's waves
#pragma unroll
        for (int e = 0; e < N; ++e) {
          double a = area[(w0 * 16 + cq) * 4 + e];
          for (int k = 1; k < nw; ++k) a += area[((w0 + k) * 16 + cq) * 4 + e];
          t[e] = a;
        }
      }
    };
    auto finish_gn = [&](auto round_c, auto act_c, auto n_c) __attribute__((always_inline)) {
      constexpr int RND = decltype(round_c)::value, ACT = decltype(act_c)::value, N = decltype(n_c)::value;
      const uint32_t pxl = (uint32_t)(4 * (64 * RND + 4 * tl));
      const int orow = row0 + (int)(pxl / W);
      const bool ook = orow < p.rows_total;
      const uint32_t px0 = (uint32_t)row0 * (uint32_t)W + pxl;
      const uint32_t ooff = ook ? (px0 * (uint32_t)p.Cout + (uint32_t)n) * 4u : R1_INVALID;
      float4 badd = bias4;
      if (has_ep && ook && ep.rowbias) {
        const float4 rb = *reinterpret_cast<const float4 *>(ep.rowbias + (int64_t)(orow / p.H) * ep.ld_rowbias + n);
        badd.x += rb.x; badd.y += rb.y; badd.z += rb.z; badd.w += rb.w;
      }
      float v[16][4];
      double s[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float *zr = lds + (size_t)(4 * tl + j) * 6 * R1_COUT + 4 * cq;
        float4 z[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) z[i] = *reinterpret_cast<const float4 *>(zr + i * R1_COUT);
#define IDIFF_R1_AT(cmp, e, b)                                                                               \
        {                                                                                                      \
          const float s12 = z[1].cmp + z[2].cmp, d12 = z[1].cmp - z[2].cmp, s34 = z[3].cmp + z[4].cmp, d34 = z[3].cmp - z[4].cmp; \
          v[4 * j + 0][e] = fmaf(z[0].cmp + (s12 + s34), descale, b);                                           \
          v[4 * j + 1][e] = fmaf(fmaf(F4_b, d34, F4_a * d12), descale, b);                                      \
          v[4 * j + 2][e] = fmaf(fmaf(F4_b2, s34, F4_a2 * s12), descale, b);                                    \
          v[4 * j + 3][e] = fmaf(fmaf(F4_b3, d34, fmaf(F4_a3, d12, z[5].cmp)), descale, b);                     \
        }
        IDIFF_R1_AT(x, 0, badd.x) IDIFF_R1_AT(y, 1, badd.y) IDIFF_R1_AT(z, 2, badd.z) IDIFF_R1_AT(w, 3, badd.w)
#undef IDIFF_R1_AT
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int e = 0; e < 4; ++e) s[e] += (double)v[4 * j + a][e];
      }
      const double inv_n = 1.0 / (double)(gn_cpg * p.H * W);
      double mean[4], q[4] = {0.0, 0.0, 0.0, 0.0};
      if (N == 1) s[0] = (s[0] + s[1]) + (s[2] + s[3]);
      gn_reduce(n_c, s, 0);
#pragma unroll
      for (int e = 0; e < 4; ++e) mean[e] = s[e < N ? e : 0] * inv_n;
#pragma unroll
      for (int i = 0; i < 16; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) { const double d = (double)v[i][e] - mean[e]; q[e] = fma(d, d, q[e]); }
      if (N == 1) q[0] = (q[0] + q[1]) + (q[2] + q[3]);
      gn_reduce(n_c, q, 1);
      const float4 ga = *reinterpret_cast<const float4 *>(p.gn_gamma + n), be = *reinterpret_cast<const float4 *>(p.gn_beta + n);
      const float gam[4] = {ga.x, ga.y, ga.z, ga.w}, bet[4] = {be.x, be.y, be.z, be.w};
      float mu[4], sc[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (e < N) sc[e] = (float)(1.0 / sqrt(q[e] * inv_n + (double)p.gn_eps)); else sc[e] = sc[0];
        mu[e] = (float)mean[e];
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) sc[e] *= gam[e];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        float y[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = idiff::act_apply((v[i][e] - mu[e]) * sc[e] + bet[e], ACT < 0 ? p.gn_act : ACT);
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(uintx4, make_float4(y[0], y[1], y[2], y[3])), rO, (int)ooff, i * p.Cout * 4,
                                               R1_STORE_AUX);
      }
    };
    auto finish_gn_round = [&](auto round_c) __attribute__((always_inline)) {
      using ASilu = std::integral_constant<int, (int)IDIFF_ACT_SILU>; using AAny = std::integral_constant<int, -1>;
      using N1 = std::integral_constant<int, 1>; using N4 = std::integral_constant<int, 4>;
      auto by_n = [&](auto a) __attribute__((always_inline)) { if (gn_cpg >= 4) finish_gn(round_c, a, N1()); else finish_gn(round_c, a, N4()); };
      if (p.gn_act == (int)IDIFF_ACT_SILU) by_n(ASilu()); else by_n(AAny());
    };
    park(I0()); park(I1());
    __syncthreads();
    IDIFF_W1D_T(4)
    finish_gn_round(I0());
    __syncthreads();
    park(I2()); park(I3());
    __syncthreads();
    finish_gn_round(I1());
    IDIFF_W1D_T(5)
  } else {   // the plain kernel's tail, as it was (not indented: the lines are the ones wino1d_kernel always had)
  // the residual's 16 pixels of a round are requested one phase ahead (round 0: before the first park, round 1: behind round 0's outputs) and
  // arrive behind the parks and barriers
  // The up2 state of the residual (p.res_up2, wino1d_kernel<8|16|32> alone): ep.residual is the residual at HALF the resolution and the thread
  // forms its 16 pixels' values itself -- the FIR x2 of upfirdn2d_nhwc_up2_block, output (2 i + a, 2 j + b) = sum over u, v of
  // lo[i - 1 + a + u][j - 1 + b + v] * up_w[a][b][u][v] in that kernel's tap order -- from the window its run of pixels needs: UR low-resolution
  // rows x UC columns (one image row or half of one: 2 x 10; W = 8, two image rows: 3 x 6), requested where the plain state requests its 16
  // pixels and held in the same registers.  A window entry outside the low-resolution image (row -1 or H/2, column -1 or W/2), or of a row
  // beyond rows_total, is R1_INVALID: the descriptor's range check returns the zero the FIR's padding is, never a neighbouring row's or image's
  // value.  Every offset is the range-checked VECTOR offset (the scalar one is not checked).
  constexpr bool UP2 = NL == 0 && (W == 8 || W == 16 || W == 32);
  constexpr int UR = W == 8 ? 3 : 2, UC = W == 8 ? 6 : 10;
  const bool res_up2 = UP2 && p.res_up2 != 0;
  float4 res[UP2 ? UR * UC : 16];
  auto request_res = [&](int rnd) __attribute__((always_inline)) {
    const uint32_t pxl = (uint32_t)(4 * (64 * rnd + 4 * tl));
    const bool ook = row0 + (int)(pxl / W) < p.rows_total;
    const uint32_t roff = ook ? (((uint32_t)row0 * (uint32_t)W + pxl) * (uint32_t)ld_res + (uint32_t)n) * 4u : R1_INVALID;
#pragma unroll
    for (int i = 0; i < 16; ++i) res[i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rR, (int)roff, i * ld_res * 4, 0));
  };
  auto request_up2 = [&](int rnd) __attribute__((always_inline)) {
    const int pxl = 4 * (64 * rnd + 4 * tl);
    const int orow = row0 + pxl / W;                               // image * H + y; W = 8: y is even (the run is rows y and y + 1)
    const bool ook = orow < p.rows_total;
    const int img = orow / p.H, y = orow - img * p.H;
    const int hl = p.H >> 1;
    constexpr int WL = W / 2;
    const int r0 = (y - 1) >> 1, c0 = ((pxl % W) >> 1) - 1;        // the window's first row and column: -1 at the image's top / left edge
#pragma unroll
    for (int k = 0; k < UC; ++k)                                   // column by column: the first pixels' entries arrive first
#pragma unroll
      for (int u = 0; u < UR; ++u) {
        const int r = r0 + u, c = c0 + k;
        const bool ok = ook && (unsigned)r < (unsigned)hl && (unsigned)c < (unsigned)WL;
        const uint32_t off = ok ? ((uint32_t)((img * hl + r) * WL + c) * (uint32_t)p.Cout + (uint32_t)n) * 4u : R1_INVALID;
        res[u * UC + k] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rR, (int)off, 0, 0));
      }
  };
  // pixel i of the run from the window; uw[row of the run][b][u][v]: the phase a of the run's row(s) is chosen by finish
  auto up2_res = [&](int i, const float (&uw)[2][8]) __attribute__((always_inline)) {
    const int xr = W == 8 ? (i & 7) : i, rr = W == 8 ? (i >> 3) : 0;
    const int b = xr & 1, k0 = (xr >> 1) + b;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int v = 0; v < 2; ++v) {
        const float wt = uw[rr][(b * 2 + u) * 2 + v];
        const float4 sv = res[(rr + u) * UC + k0 + v];
        acc.x += sv.x * wt; acc.y += sv.y * wt; acc.z += sv.z * wt; acc.w += sv.w * wt;
      }
    return acc;
  };
  double s1[2][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}}, s2[2][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
  // One round's 16 pixels with the epilogue's switches as COMPILE-TIME constants: tested at run time inside the loop every pixel became a chain
  // of scalar branches between its LDS reads and its store and nothing of one pixel overlapped the next -- 9.6 us per workgroup where the
  // constant form took 1.7 (profiles/r05_wino1d_stamps.txt).  ACT < 0: the activation by its run-time code.
  auto finish = [&](auto round_c, auto act_c, auto res_c, auto scaled_c, auto stats_c) __attribute__((always_inline)) {
    constexpr int RND = decltype(round_c)::value, ACT = decltype(act_c)::value;
    constexpr int RESK = decltype(res_c)::value;                               // the residual: 0 none, 1 plain, 2 up2
    constexpr bool RES = RESK != 0, SCALED = decltype(scaled_c)::value, STATS = decltype(stats_c)::value;
    // row-tile m of the block is its pixels 4 m .. 4 m + 3 in row-major order
    const uint32_t pxl = (uint32_t)(4 * (64 * RND + 4 * tl));                  // my first pixel, counted from the block's first
    const int orow = row0 + (int)(pxl / W);
    const bool ook = orow < p.rows_total;
    const uint32_t px0 = (uint32_t)row0 * (uint32_t)W + pxl;
    const uint32_t ooff = ook ? (px0 * (uint32_t)p.Cout + (uint32_t)n) * 4u : R1_INVALID;
    float4 badd = bias4;
    float sc = has_ep ? ep.out_scale : 1.f;
    if (has_ep && ook) {
      const int img = orow / p.H;
      if (ep.rowbias) {
        const float4 rb = *reinterpret_cast<const float4 *>(ep.rowbias + (int64_t)img * ep.ld_rowbias + n);
        badd.x += rb.x; badd.y += rb.y; badd.z += rb.z; badd.w += rb.w;
      }
      if (ep.rowscale) sc *= ep.rowscale[img];
    }
    float uw[2][8];                                    // up2: the weights of the run's row(s); H is even, so orow's parity is y's
    if (RESK == 2) {
#pragma unroll
      for (int t = 0; t < 8; ++t) { uw[0][t] = (W != 8 && (orow & 1)) ? p.up_w[8 + t] : p.up_w[t]; uw[1][t] = p.up_w[8 + t]; }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {                      // row-tile 4 tl + j of the round
      const float *zr = lds + (size_t)(4 * tl + j) * 6 * R1_COUT + 4 * cq;
      float4 z[6];
#pragma unroll
      for (int i = 0; i < 6; ++i) z[i] = *reinterpret_cast<const float4 *>(zr + i * R1_COUT);
      float y[4][4];
#define IDIFF_R1_AT(cmp, e)                                                                                  \
      {                                                                                                      \
        const float s12 = z[1].cmp + z[2].cmp, d12 = z[1].cmp - z[2].cmp, s34 = z[3].cmp + z[4].cmp, d34 = z[3].cmp - z[4].cmp; \
        y[0][e] = z[0].cmp + (s12 + s34);                                                                     \
        y[1][e] = fmaf(F4_b, d34, F4_a * d12);                                                                \
        y[2][e] = fmaf(F4_b2, s34, F4_a2 * s12);                                                              \
        y[3][e] = fmaf(F4_b3, d34, fmaf(F4_a3, d12, z[5].cmp));                                               \
      }
      IDIFF_R1_AT(x, 0) IDIFF_R1_AT(y, 1) IDIFF_R1_AT(z, 2) IDIFF_R1_AT(w, 3)
#undef IDIFF_R1_AT
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        y[a][0] = fmaf(y[a][0], descale, badd.x); y[a][1] = fmaf(y[a][1], descale, badd.y);
        y[a][2] = fmaf(y[a][2], descale, badd.z); y[a][3] = fmaf(y[a][3], descale, badd.w);
        if (ACT != (int)IDIFF_ACT_NONE) {
#pragma unroll
          for (int e = 0; e < 4; ++e) y[a][e] = idiff::act_apply(y[a][e], ACT < 0 ? act : ACT);
        }
        if (RES) { const float4 r = RESK == 2 ? up2_res(4 * j + a, uw) : res[4 * j + a]; y[a][0] += r.x; y[a][1] += r.y; y[a][2] += r.z; y[a][3] += r.w; }
        if (SCALED) {
#pragma unroll
          for (int e = 0; e < 4; ++e) y[a][e] *= sc;
        }
        if (STATS) {
#pragma unroll
          for (int e = 0; e < 4; ++e) { s1[RND][e] += (double)y[a][e]; s2[RND][e] += (double)y[a][e] * (double)y[a][e]; }
        }
#ifdef IDIFF_W1D_DIAG_NO_STORE     // timing-only build: one store per thread and round instead of 16
        if (4 * j + a == 15)
#endif
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(uintx4, make_float4(y[a][0], y[a][1], y[a][2], y[a][3])), rO, (int)ooff,
                                               (4 * j + a) * p.Cout * 4, R1_STORE_AUX);
      }
    }
  };
  auto finish_round = [&](auto round_c) __attribute__((always_inline)) {
    using T = std::true_type; using F = std::false_type;
    using ANone = std::integral_constant<int, (int)IDIFF_ACT_NONE>; using AAny = std::integral_constant<int, -1>;
    auto by_stats = [&](auto a, auto r, auto sc_) __attribute__((always_inline)) { if (want_stats) finish(round_c, a, r, sc_, T()); else finish(round_c, a, r, sc_, F()); };
    auto by_scale = [&](auto a, auto r) __attribute__((always_inline)) { if (scaled) by_stats(a, r, T()); else by_stats(a, r, F()); };
    auto by_res = [&](auto a) __attribute__((always_inline)) {
      if constexpr (UP2) { if (res_up2) { by_scale(a, I2()); return; } }
      if (has_res) by_scale(a, I1()); else by_scale(a, I0());
    };
    if (act == (int)IDIFF_ACT_NONE) by_res(ANone()); else by_res(AAny());
  };
  auto request = [&](int rnd) __attribute__((always_inline)) {
    if constexpr (UP2) { if (res_up2) { request_up2(rnd); return; } }
    request_res(rnd);
  };
  if (has_res) request(0);
  park(I0()); park(I1());
  __syncthreads();
  IDIFF_W1D_T(4)
  finish_round(I0());
  if (has_res) request(1);
  __syncthreads();
  park(I2()); park(I3());
  __syncthreads();
  finish_round(I1());
  IDIFF_W1D_T(5)
  if (want_stats) {
    // per-sample (or per-block, where a sample spans several blocks) column sums for the GroupNorm that reads this output: thread sums ->
    // [32 thread rows = (round, tl)][64 channels] in LDS -> one thread per (slot, channel)
    __syncthreads();
    double *red = reinterpret_cast<double *>(lds);
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        red[(((16 * r + tl) * R1_COUT) + 4 * cq + e) * 2] = s1[r][e];
        red[(((16 * r + tl) * R1_COUT) + 4 * cq + e) * 2 + 1] = s2[r][e];
      }
    __syncthreads();
    const int slots = RB > p.H ? RB / p.H : 1;                     // samples per block
    const int per = 32 / slots;                                    // thread rows per sample
    for (int o = tid; o < slots * R1_COUT; o += R1_THREADS) {
      const int smp = o / R1_COUT, ch = o - smp * R1_COUT;
      const int64_t slot = (int64_t)tile_m * slots + smp;           // sample, or (sample, split) = block
      if (slots > 1 && slot >= p.B) continue;
      double a = 0.0, b = 0.0;
      for (int k = 0; k < per; ++k) { a += red[((smp * per + k) * R1_COUT + ch) * 2]; b += red[((smp * per + k) * R1_COUT + ch) * 2 + 1]; }
      double *dst = ep.colstats + (slot * p.Cout + n0 + ch) * 2;
      dst[0] = a; dst[1] = b;
    }
  }
  }
#ifdef IDIFF_W1D_STAMP
  IDIFF_W1D_T(6)
  if (tid == 0 && p.stamps) {
    uint64_t *q = p.stamps + 8 * (int64_t)blockIdx.x;
    for (int k = 0; k < 7; ++k) q[k] = st[k];
    q[7] = __builtin_amdgcn_s_getreg(((8 - 1) << 11) | (0 << 6) | 4) ;   // HW_ID low byte: wave / SIMD / pipe ... (bits 8..11: CU)
  }
#endif
#undef IDIFF_W1D_T
}

template <int W>
__global__ void __launch_bounds__(R1_THREADS)
wino1d_kernel(const Wino1dParams p) { r1_body<W, false>(p); }

// the same convolution with the GroupNorm (+ activation) that reads its output applied in the tail: maps of at most 256 pixels
template <int W>
__global__ void __launch_bounds__(R1_THREADS)
wino1d_gn_kernel(const Wino1dParams p) { r1_body<W, true>(p); }

// the same convolution of act(a x + b), (a, b) per (image, input channel): the GroupNorm (+ SiLU: NL = 2) in front of it, applied by the loader
template <int NL>
__global__ void __launch_bounds__(R1_THREADS)
wino1d_nl_kernel(const Wino1dParams p) { r1_body<32, false, NL>(p); }

// the same with the input cat[x, x2] read from its two sources (GroupNorm_0 of a residual block on the up path: the concatenation is never made)
template <int NL>
__global__ void __launch_bounds__(R1_THREADS)
wino1d_nl2_kernel(const Wino1dParams p) { r1_body<32, false, NL, true>(p); }

// U[i][ky] = sum_kx G[i][kx] g[ky][kx] in fp64 for one (cin, cout) pair
__device__ __forceinline__ void r1_u_of_pair(const float *wt, int Cin, int cin, int cout, double (&U)[18]) {
  double Gm[6][3];
  wino_G(F4_A, F4_B, Gm);
  for (int ky = 0; ky < 3; ++ky) {
    double g[3];
    for (int kx = 0; kx < 3; ++kx) g[kx] = (double)wt[((int64_t)cout * 9 + ky * 3 + kx) * Cin + cin];
    for (int i = 0; i < 6; ++i) U[3 * i + ky] = Gm[i][0] * g[0] + Gm[i][1] * g[1] + Gm[i][2] * g[2];
  }
}

bool r1_geometry_ok(int B, int H, int W, int Cin, int Cout, int min_cin = 2 * R1_KC) {
  if (B <= 0 || H <= 0 || Cin <= 0 || Cout <= 0) return false;
  if (W != 4 && W != 8 && W != 16 && W != 32 && W != 64) return false;
  const int RB = R1_PIXELS / W;
  if (H % 4 || (RB % H != 0 && H % RB != 0)) return false;                     // a block is whole images or a whole part of one
  if (Cin % R1_KC || Cin < min_cin || Cin > 1024 || Cout % R1_COUT) return false;
  if ((int64_t)R1_NSLOT * Cin * Cout * 4 >= R1_X_LIMIT) return false;
  if ((int64_t)B * H * W * (Cin > Cout ? Cin : Cout) * 4 >= R1_X_LIMIT - 0x4000) return false;   // one buffer descriptor per tensor
  return true;
}

// one AttrGuard per kernel: the static lives in the instantiation
template <void (*KERNEL)(const Wino1dParams)>
int r1_launch(const Wino1dParams &p, const char *name, hipStream_t stream) {
  static idiff::AttrGuard guard;
  const void *fn = reinterpret_cast<const void *>(KERNEL);
  if (int rc = idiff::set_dynamic_lds_once(guard, &fn, 1, (int)R1_LDS_BYTES, name)) return rc;
  hipLaunchKernelGGL(KERNEL, dim3(p.blocks_m * p.tiles_n), dim3(R1_THREADS), R1_LDS_BYTES, stream, p);
  return idiff::launch_status(name);
}

// the fused GroupNorm's own conditions (the convolution's: r1_geometry_ok): a tail round of 256 pixels holds whole images, a tile of 64
// channels whole groups; the kernel is built for the rows of 4, 8 and 16 pixels such maps have in the networks
bool r1_gn_geometry_ok(int H, int W, int Cout, int groups) {
  if (W > 16 || H * W > 256 || 256 % (H * W)) return false;
  if (groups <= 0 || Cout % groups) return false;
  return R1_COUT % (Cout / groups) == 0;
}

// the norm in the loader: rows of 32 pixels and blocks (16 rows) that never straddle two images; one K step is enough for this kernel
bool r1_nl_geometry_ok(int B, int H, int W, int Cin, int Cout) {
  return W == 32 && H % (R1_PIXELS / 32) == 0 && r1_geometry_ok(B, H, W, Cin, Cout, R1_KC);
}
}  // namespace

IDIFF_API int idiff_conv2d_wino1d_ok(int B, int H, int W, int Cin, int Cout) {
  using namespace idiff;
  if (option(OPT_NO_WINOGRAD) || option(OPT_NO_WINO43H) || option(OPT_NO_WINO1D)) return 0;
  return r1_geometry_ok(B, H, W, Cin, Cout) ? 1 : 0;
}

// nsplit of epilogue.colstats ([samples, nsplit, Cout, 2]) or 0 when the statistics cannot be produced
IDIFF_API int idiff_conv2d_wino1d_colstats_split(int B, int H, int W, int Cin, int Cout) {
  if (!idiff_conv2d_wino1d_ok(B, H, W, Cin, Cout) || idiff::option(idiff::OPT_NO_COLSTATS)) return 0;
  const int RB = R1_PIXELS / W;
  return H > RB ? H / RB : 1;
}

IDIFF_API int64_t idiff_wino1d_weight_floats(int Cin, int Cout) { return (int64_t)R1_NSLOT * Cin * Cout + 4; }

IDIFF_API int idiff_wino1d_pack_f32(const float *wt, float *u, int Cin, int Cout, void *stream) {
  return pair_bank_pack<R1_NSLOT, r1_u_of_pair>("wino1d_pack", wt, u, Cin, Cout, stream);
}

namespace {
struct R1GroupNorm { int groups; const float *gamma, *beta; float eps; int act; };
struct R1NormLoad { const float *coef; int act; const float *x2; int c1; };       // x2 != nullptr: two sources, x [.., c1] and x2 [.., Cin - c1]
struct R1ResUp { const float *lo; const float *taps; };                            // the residual at half the resolution and its 16 polyphase weights (host)

// the up2 residual's own conditions (the convolution's: r1_geometry_ok): the rows the tail's up2 state is built for, whole 2 x 2 blocks
bool r1_resup_geometry_ok(int H, int W) { return (W == 8 || W == 16 || W == 32) && H % 2 == 0; }

// the four entry points: gn == nullptr and nl == nullptr is idiff_conv2d_wino1d_f32
int r1_run(const float *x, const float *u, float *out, int B, int H, int W, int Cin, int Cout, const idiff_epilogue *ep, const R1GroupNorm *gn,
           const R1NormLoad *nl, void *stream, const R1ResUp *ru = nullptr) {
  using namespace idiff;
  if (B == 0) return 0;
  if (ru) {
    // nothing is launched unless the plain tail of wino1d_kernel<8|16|32> finishes this call and the request is its only residual (the entry
    // point has neither the fused GroupNorm's nor the loader norm's arguments: those combinations cannot be expressed)
    if (option(OPT_NO_FUSED_RES_UP)) return fail("conv2d_wino1d_resup: switched off (IDIFF_NO_FUSED_RES_UP): ask idiff_conv2d_wino1d_resup_ok");
    if (!r1_resup_geometry_ok(H, W))
      return fail("conv2d_wino1d_resup: H=%d W=%d not served: W in {8, 16, 32}, H even (ask idiff_conv2d_wino1d_resup_ok)", H, W);
    if (!ru->lo || ((uintptr_t)ru->lo & 15) || !ru->taps) return fail("conv2d_wino1d_resup: the low-resolution residual (16-byte aligned) and its 16 weights are required");
    if (ep && ep->residual) return fail("conv2d_wino1d_resup: the epilogue already carries a residual");
  }
  const bool two = nl && nl->x2;
  if (nl && (nl->x2 || nl->c1 != Cin)) {
    // two sources: whole K steps from each, each inside one buffer descriptor of its own
    const int C1 = nl->c1, C2 = Cin - nl->c1;
    if (C1 <= 0 || C2 <= 0 || C1 % R1_KC || C2 % R1_KC)
      return fail("conv2d_wino1d_normload_2src: C1 = %d and C2 = %d must be positive multiples of %d (a K step reads one source)", C1, C2, R1_KC);
    if (B > 0 && H > 0 && W > 0 && (int64_t)B * H * W * (C1 > C2 ? C1 : C2) * 4 >= R1_X_LIMIT - 0x4000)
      return fail("conv2d_wino1d_normload_2src: a source of B=%d H=%d W=%d C=%d is beyond one buffer descriptor", B, H, W, C1 > C2 ? C1 : C2);
    if (!nl->x2 || ((uintptr_t)nl->x2 & 15)) return fail("conv2d_wino1d_normload_2src: x2 is required, 16-byte aligned");
  }
  if (nl) {
    // nothing is launched unless a block's rows are one image's (one set of coefficients per workgroup)
    if (!r1_nl_geometry_ok(B, H, W, Cin, Cout))
      return fail("conv2d_wino1d_normload: geometry B=%d H=%d W=%d Cin=%d Cout=%d not supported: W = 32, H %% 16 == 0, Cin %% 16 == 0, "
                  "Cout %% 64 == 0", B, H, W, Cin, Cout);
    if (!nl->coef || ((uintptr_t)nl->coef & 15)) return fail("conv2d_wino1d_normload: the coefficients [B, Cin, 2] are required, 16-byte aligned");
    if (nl->act != IDIFF_ACT_NONE && nl->act != IDIFF_ACT_SILU)
      return fail("conv2d_wino1d_normload: the loader applies SiLU or no activation (code %d)", nl->act);
  } else if (!r1_geometry_ok(B, H, W, Cin, Cout))
    return fail("conv2d_wino1d: geometry B=%d H=%d W=%d Cin=%d Cout=%d not supported (ask idiff_conv2d_wino1d_ok)", B, H, W, Cin, Cout);
  int64_t res_bytes = 0;
  if (int rc = wino_check_call("conv2d_wino1d", x, u, out, ep, B, H, W, Cout, R1_X_LIMIT, res_bytes)) return rc;
  // (the loader forms serve a single K step, which the plain kernel and with it the query do not: the column sums are the tail's and do not
  // depend on Cin, so such a call is asked about as one of two steps)
  if (ep && ep->colstats && idiff_conv2d_wino1d_colstats_split(B, H, W, nl && Cin < 2 * R1_KC ? 2 * R1_KC : Cin, Cout) <= 0)
    return fail("conv2d_wino1d: colstats are switched off (IDIFF_NO_COLSTATS): ask idiff_conv2d_wino1d_colstats_split");
  if (gn) {
    // nothing is launched unless the tail can finish every (image, group) inside one round of one workgroup and store act(GN(.)) alone
    if (!r1_gn_geometry_ok(H, W, Cout, gn->groups))
      return fail("conv2d_wino1d_gn: H * W = %d must divide 256 (rows of at most 16 pixels) and Cout / groups = %d / %d must divide 64 "
                  "(ask idiff_conv2d_wino1d_gn_ok)", H * W, Cout, gn->groups);
    if (!gn->gamma || !gn->beta || (((uintptr_t)gn->gamma | (uintptr_t)gn->beta) & 15))
      return fail("conv2d_wino1d_gn: gamma and beta are required, 16-byte aligned");
    if (gn->act < IDIFF_ACT_NONE || gn->act > IDIFF_ACT_LRELU) return fail("conv2d_wino1d_gn: unknown activation code %d", gn->act);
    if (ep && ep->residual) return fail("conv2d_wino1d_gn: a residual cannot be combined with the fused GroupNorm (its registers hold the image)");
    if (ep && ep->colstats) return fail("conv2d_wino1d_gn: colstats together with the fused GroupNorm: the convolution's own output is never stored");
    if (ep && (ep->act != IDIFF_ACT_NONE || ep->out_scale != 1.f || ep->rowscale))
      return fail("conv2d_wino1d_gn: the epilogue in front of the fused GroupNorm is bias + per-image bias only (no activation, no scale)");
    if (ep && ep->rows_per_group != H * W)
      return fail("conv2d_wino1d_gn: rows_per_group must be H * W = %d (got %d)", H * W, ep->rows_per_group);
  }
  Wino1dParams p = {};
  // all cout tiles of a row block next to each other in the launch order (same XCD, same K step at about the same time: the block's pixels come
  // from HBM once): 1.49x -> 1.39x algorithmic bytes over a forward at equal time (pairs of tiles: 73.0 ms, all four: 72.9, one: 74.1)
  wino_fill(p, x, u, out, B, H, W, Cin, Cout, (int64_t)R1_NSLOT * Cin * Cout, res_bytes, ep, R1_COUT, false);
  p.rows_total = B * H;
  p.blocks_m = ceil_div(p.rows_total, R1_PIXELS / W);
  if (ru) {
    // the low-resolution residual in the residual's place: pitch Cout, a quarter of the output's extent (inside one descriptor with it)
    p.has_ep = 1; p.ep.residual = ru->lo; p.ep.ld_residual = Cout;
    p.res_bytes = (uint32_t)((int64_t)B * (H / 2) * (W / 2) * Cout * 4);
    p.res_up2 = 1;
    for (int t = 0; t < 16; ++t) p.up_w[t] = ru->taps[t];
  }
#ifdef IDIFF_W1D_STAMP
  { const char *e = getenv("IDIFF_W1D_STAMP_PTR"); p.stamps = e ? reinterpret_cast<uint64_t *>(strtoull(e, nullptr, 0)) : nullptr; }
#endif
  if (nl) {
    p.nl_coef = nl->coef; p.nl_bytes = (uint32_t)((int64_t)B * Cin * 8);
    if (two) {
      p.x2 = nl->x2; p.c1 = nl->c1;
      p.x_bytes = (uint32_t)((int64_t)B * H * W * nl->c1 * 4); p.x2_bytes = (uint32_t)((int64_t)B * H * W * (Cin - nl->c1) * 4);
    }
    const bool silu = nl->act == IDIFF_ACT_SILU;
    const hipStream_t s = (hipStream_t)stream;
    return two ? (silu ? r1_launch<wino1d_nl2_kernel<2>>(p, "conv2d_wino1d_normload_2src", s)
                       : r1_launch<wino1d_nl2_kernel<1>>(p, "conv2d_wino1d_normload_2src", s))
               : (silu ? r1_launch<wino1d_nl_kernel<2>>(p, "conv2d_wino1d_normload", s) : r1_launch<wino1d_nl_kernel<1>>(p, "conv2d_wino1d_normload", s));
  }
  if (gn) {
    p.gn_gamma = gn->gamma; p.gn_beta = gn->beta; p.gn_cpg = Cout / gn->groups; p.gn_act = gn->act; p.gn_eps = gn->eps;
    switch (W) {
      case 4: return r1_launch<wino1d_gn_kernel<4>>(p, "conv2d_wino1d_gn", (hipStream_t)stream);
      case 8: return r1_launch<wino1d_gn_kernel<8>>(p, "conv2d_wino1d_gn", (hipStream_t)stream);
      default: return r1_launch<wino1d_gn_kernel<16>>(p, "conv2d_wino1d_gn", (hipStream_t)stream);       // (r1_gn_geometry_ok: W <= 16)
    }
  }
  switch (W) {
    case 4: return r1_launch<wino1d_kernel<4>>(p, "conv2d_wino1d", (hipStream_t)stream);
    case 8: return r1_launch<wino1d_kernel<8>>(p, "conv2d_wino1d", (hipStream_t)stream);
    case 16: return r1_launch<wino1d_kernel<16>>(p, "conv2d_wino1d", (hipStream_t)stream);
    case 64: return r1_launch<wino1d_kernel<64>>(p, "conv2d_wino1d", (hipStream_t)stream);
    default: return r1_launch<wino1d_kernel<32>>(p, "conv2d_wino1d", (hipStream_t)stream);
  }
}
}  // namespace

IDIFF_API int idiff_conv2d_wino1d_f32(const float *x, const float *u, float *out, int B, int H, int W, int Cin, int Cout,
                                      const idiff_epilogue *ep, void *stream) {
  return r1_run(x, u, out, B, H, W, Cin, Cout, ep, nullptr, nullptr, stream);
}

// The x2 FIR of an up block's shortcut inside Conv_1's tail (scripts/shortcut_shape_ab.py, profiles/shortcut_shape_ab.txt).
// IDIFF_NO_FUSED_RES_UP answers no.
IDIFF_API int idiff_conv2d_wino1d_resup_ok(int B, int H, int W, int Cin, int Cout) {
  if (!idiff_conv2d_wino1d_ok(B, H, W, Cin, Cout) || idiff::option(idiff::OPT_NO_FUSED_RES_UP)) return 0;
  return r1_resup_geometry_ok(H, W) ? 1 : 0;
}

IDIFF_API int idiff_conv2d_wino1d_resup_f32(const float *x, const float *u, float *out, int B, int H, int W, int Cin, int Cout,
                                            const idiff_epilogue *ep, const float *lo, const float *taps, void *stream) {
  const R1ResUp ru = {lo, taps};
  return r1_run(x, u, out, B, H, W, Cin, Cout, ep, nullptr, nullptr, stream, &ru);
}

IDIFF_API int idiff_conv2d_wino1d_gn_ok(int B, int H, int W, int Cin, int Cout, int groups) {
  if (!idiff_conv2d_wino1d_ok(B, H, W, Cin, Cout) || idiff::option(idiff::OPT_NO_FUSED_GN)) return 0;
  return r1_gn_geometry_ok(H, W, Cout, groups) ? 1 : 0;
}

IDIFF_API int idiff_conv2d_wino1d_gn_f32(const float *x, const float *u, float *out, int B, int H, int W, int Cin, int Cout,
                                         const idiff_epilogue *ep, int groups, const float *gamma, const float *beta, float eps, int act,
                                         void *stream) {
  const R1GroupNorm gn = {groups, gamma, beta, eps, act};
  return r1_run(x, u, out, B, H, W, Cin, Cout, ep, &gn, nullptr, stream);
}

// Routed: where the loader's norm was MEASURED faster than the pass in front of the convolution (scripts/normload_shape_ab.py,
// profiles/normload_shape_ab.txt, B = 2240, 32 x 32, median us of {groupnorm_apply_colstats + conv2d_wino1d} against {coefficients + this}):
//   128 -> 128   453 + 1203 = 1656   against   8 + 1422 = 1430   (-13.7 %)
//   256 -> 128   909 + 2077 = 2985   against  16 + 2512 = 2527   (-15.3 %)
//   384 -> 128  1390 + 2997 = 4387   against  23 + 3684 = 3707   (-15.5 %)
//   256 -> 256   917 + 4129 = 5046   against  16 + 4961 = 4977   (-1.4 %: inside the repetitions' spread -- not routed)
// The K loop is 18 - 23 % slower with the norm's 96 units in it, whatever the class; the pass it replaces costs the same per input channel
// while the loop's time grows with the cout tiles that stage the same input: one or two tiles win, four do not.
// In config 3 one source only ever brings 128 -> 128 here: the 256 -> 128 and 384 -> 128 classes are GroupNorm_0 of cat[h, skip] on the up
// path and reach the loader through the two-source form (idiff_conv2d_wino1d_normload_2src_ok, at the end of this file).
IDIFF_API int idiff_conv2d_wino1d_normload_ok(int B, int H, int W, int Cin, int Cout) {
  using namespace idiff;
  if (option(OPT_NO_WINOGRAD) || option(OPT_NO_WINO43H) || option(OPT_NO_WINO1D) || option(OPT_NO_PAIRS) || option(OPT_NO_FUSED_GN_LOAD)) return 0;
  if (!r1_nl_geometry_ok(B, H, W, Cin, Cout)) return 0;
  return Cout / R1_COUT <= 2 ? 1 : 0;
}

IDIFF_API int idiff_conv2d_wino1d_normload_f32(const float *x, const float *u, float *out, int B, int H, int W, int Cin, int Cout,
                                               const idiff_epilogue *ep, const float *coef, int act, void *stream) {
  const R1NormLoad nl = {coef, act, nullptr, Cin};
  return r1_run(x, u, out, B, H, W, Cin, Cout, ep, nullptr, &nl, stream);
}

// The two-source form: GroupNorm_0 of cat[h, skip] in the level-0 blocks of config 3's up path -- the 256 -> 128 and 384 -> 128 classes of the
// table above reach the loader only through it (one source never has them there).  Routed class by class as the one-source form is
// (scripts/normload_shape_ab.py, profiles/normload2_shape_ab.txt: {two-source groupnorm_apply_colstats + conv2d_wino1d on the concatenated
// output} against {coefficients + this}, B = 2240, 32 x 32, median us):
//   128 + 128 -> 128   929 + 2081 = 3010   against  16 + 2607 = 2623   (-12.8 %, spread 190)
//   256 + 128 -> 128  1371 + 2994 = 4366   against  23 + 3720 = 3743   (-14.3 %, spread 133)
// both beyond the repetitions' spread: at most two cout tiles are routed, as for one source (four were never a gain there).
// IDIFF_NO_FUSED_GN_LOAD_2SRC answers no, IDIFF_NO_FUSED_GN_LOAD does not bear on it.
IDIFF_API int idiff_conv2d_wino1d_normload_2src_ok(int B, int H, int W, int C1, int C2, int Cout) {
  using namespace idiff;
  if (option(OPT_NO_WINOGRAD) || option(OPT_NO_WINO43H) || option(OPT_NO_WINO1D) || option(OPT_NO_PAIRS) || option(OPT_NO_FUSED_GN_LOAD_2SRC)) return 0;
  if (C1 <= 0 || C2 <= 0 || C1 % R1_KC || C2 % R1_KC || !r1_nl_geometry_ok(B, H, W, C1 + C2, Cout)) return 0;
  return Cout / R1_COUT <= 2 ? 1 : 0;
}

IDIFF_API int idiff_conv2d_wino1d_normload_2src_f32(const float *x1, int C1, const float *x2, int C2, const float *u, float *out, int B, int H,
                                                    int W, int Cout, const idiff_epilogue *ep, const float *coef, int act, void *stream) {
  if (C1 <= 0 || C2 <= 0)
    return idiff::fail("conv2d_wino1d_normload_2src: C1 = %d and C2 = %d must be positive multiples of %d (a K step reads one source)", C1, C2, R1_KC);
  const R1NormLoad nl = {coef, act, x2, C1};
  return r1_run(x1, u, out, B, H, W, C1 + C2, Cout, ep, nullptr, &nl, stream);
}
