// Shared host/device helpers for libidiff_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>

#include "../../include/idiff_hip.h"

#define IDIFF_API extern "C" __attribute__((visibility("default")))

namespace idiff {

void set_error(const char *fmt, ...);

inline int fail(const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  set_error("%s", buf);
  return IDIFF_EINVAL;
}

// Every launcher ends with this: reports a launch-time error without synchronising.
inline int launch_status(const char *what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: %s", what, hipGetErrorString(e));
    return (int)e;
  }
  return 0;
}

// ---- process-level debug switches (A/B experiments, parity tests).  Read from the environment ONCE, when the library
// is loaded (no getenv on any launch path); idiff_set_option() flips them afterwards.
enum Option { OPT_NO_WINOGRAD, OPT_NO_COLSTATS, OPT_NO_PIPE, OPT_SCALAR_EPILOGUE, OPT_TRIDIAG_ONESTAGE,
              OPT_UFD_ROWS, OPT_CHASE_WAVEFRONT, OPT_GRAM_SMALL_TILES, OPT_CHASE_SPIN_LIMIT, OPT_FAKE_CU_COUNT,
              OPT_SBR_SYNC, OPT_NO_SPLIT, OPT_NO_WINO43, OPT_NO_WINO43H, OPT_NO_PAIRS, OPT_PAIRS_MIN_TILES, OPT_NO_FUSED_ATTN, OPT_NO_WINO1D, OPT_NO_FUSED_GN, OPT_NO_FUSED_GN_LOAD, OPT_NO_FUSED_GN_LOAD_2SRC, OPT_NO_FUSED_GN_FIR, OPT_NO_2SRC_PITCH, OPT_NO_FUSED_RES_UP, OPT_COUNT };
bool option(Option o);
int option_value(Option o);   // the integer behind a switch (IDIFF_PAIRS_MIN_TILES: a tile count)

// hipFuncSetAttribute is per DEVICE: one bit per device ordinal, so a process that drives several GPUs sets the
// attribute on each of them (a process-wide `static bool` would leave the second device at the 64 KB default).
struct AttrGuard { unsigned long long done_mask = 0; };
int set_dynamic_lds_once(AttrGuard &g, const void *const *fns, int n_fns, int bytes, const char *what);

// conv_narrow.hip: 3x3 / stride 1 / pad 1 convolution to <= 4 output channels on the vector ALUs (the image heads)
bool conv3x3_narrow_ok(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad_lo, int pad_hi,
                       const idiff_epilogue *ep);
int conv3x3_narrow(const float *x, const float *wt, float *out, int B, int H, int W, int Cin, int Cout,
                   const idiff_epilogue *ep, hipStream_t stream);

// Every launcher's "the caller's epilogue, or none" into its kernel arguments (P has the fields ep and has_ep): without one the kernels
// read has_ep alone; the neutral values (no pointers, one row per group, scale 1) are there for the host code that reads p.ep regardless.
template <class P> inline void set_epilogue(P &p, const idiff_epilogue *ep) {
  p.has_ep = ep ? 1 : 0;
  p.ep = ep ? *ep : idiff_epilogue{};
  if (!ep) p.ep.out_scale = 1.f;
  if (p.ep.rows_per_group <= 0) p.ep.rows_per_group = 1;
}

// ---- the host cut.  The fast kernels address an operand through one 32-bit-offset buffer descriptor (< 4 GiB).  Rows are independent,
// so a larger problem runs as two row ranges (igemm.hip: matrices and NHWC convolutions; winograd.hip), each cut again if it must be.
// The epilogue of the range that starts at row m0, which must be a multiple of rows_per_group:
inline idiff_epilogue shift_epilogue(const idiff_epilogue &ep, int64_t m0) {
  idiff_epilogue e = ep;
  const int64_t g0 = m0 / (ep.rows_per_group > 0 ? ep.rows_per_group : 1);
  if (e.rowbias) e.rowbias += g0 * ep.ld_rowbias;
  if (e.residual) e.residual += m0 * ep.ld_residual;
  if (e.rowscale) e.rowscale += g0;
  return e;
}
// The row to cut `units` units of `unit_rows` rows at (a matrix: rows of 1; a convolution: images of OH * OW), or 0: there is none, and
// the caller falls back or refuses.  Matrices are cut at the last whole row group below the middle, images after the middle one or not
// at all.
inline int64_t host_cut_row(int64_t units, int64_t unit_rows, const idiff_epilogue *ep) {
  const int64_t rpg = (ep && ep->rows_per_group > 0) ? ep->rows_per_group : 1;
  const int64_t half = units / 2 * unit_rows;
  return unit_rows == 1 ? half / rpg * rpg : half % rpg ? 0 : half;
}
// run(r0, r1, ep) for the rows [0, cut) and [cut, rows), each with its epilogue (first_only: a route query, which reports the first range)
template <class Run> inline int run_cut(int64_t rows, int64_t cut, const idiff_epilogue *ep, bool first_only, Run run) {
  if (int rc = run((int64_t)0, cut, ep)) return rc;
  if (first_only) return 0;
  idiff_epilogue hi;
  if (ep) hi = shift_epilogue(*ep, cut);
  return run(cut, rows, ep ? &hi : nullptr);
}

static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
static inline int64_t ceil_div64(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Memory-bound grids: enough workgroups to fill 256 CUs x 8 without paying for a huge grid.
static inline int streaming_grid(int64_t work_items, int block) {
  int64_t g = ceil_div64(work_items, block);
  const int64_t cap = 256 * 8;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}

__device__ __forceinline__ float act_apply(float v, int act) {
  switch (act) {
    // v_exp_f32 / v_rcp_f32 (1-2 ulp each) instead of libm's expf and an IEEE division: 4 instructions, not ~25, which
    // is what kept the GroupNorm-apply pass below the HBM rate.  __expf(-v) is exp2(fl(-v log2 e)): the rounded product puts 1.2 |v| u into
    // the exponent, so the error grows with |v|: |error| <= u |silu(v)| (6 + 1.5 |v|), u = 2^-24 (4.5e-7 |silu(v)| at |v| = 1, 2.1e-6 at
    // |v| = 20; derived in tests/norm_act_cases.py, measured in tests/test_hip_norm_act_routes.py), inside the 2e-5 parity bar
    case IDIFF_ACT_SILU: return v * __frcp_rn(1.0f + __expf(-v));
    case IDIFF_ACT_ELU: return v > 0.f ? v : (expf(v) - 1.0f);  // exp(x)-1 as ATen's elu does
    case IDIFF_ACT_RELU: return v > 0.f ? v : 0.f;
    case IDIFF_ACT_LRELU: return v > 0.f ? v : 0.2f * v;
    default: return v;
  }
}

}  // namespace idiff
