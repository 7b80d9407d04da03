// Philox4x32-10 (Salmon et al., SC'11) and the uniform it feeds to Box-Muller: shared by the noise of the score matrices
// (rng.hip) and the start block of the subspace iteration (lowvecs.hip).
#pragma once
#include "common.h"

namespace idiff {

struct u4 { uint32_t x, y, z, w; };

__device__ __forceinline__ u4 philox4x32_10(u4 ctr, uint32_t k0, uint32_t k1) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(M0, ctr.x), lo0 = M0 * ctr.x;
    const uint32_t hi1 = __umulhi(M1, ctr.z), lo1 = M1 * ctr.z;
    ctr = {hi1 ^ ctr.y ^ k0, lo1, hi0 ^ ctr.w ^ k1, lo0};
    k0 += W0; k1 += W1;
  }
  return ctr;
}

__device__ __forceinline__ float u01(uint32_t v) {   // (0, 1]: never feeds log(0)
  return ((float)(v >> 8) + 1.0f) * (1.0f / 16777216.0f);
}

}  // namespace idiff
