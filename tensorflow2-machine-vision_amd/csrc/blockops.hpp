// Block- and wave-level building blocks shared by csrc/detect.hip, csrc/match.hip and
// csrc/evalmap.hip: the order-preserving float key, the LDS bitonic sort and the wave-wide
// integer maximum.  One definition each.
#pragma once
#include "common.hpp"

namespace edet {

typedef unsigned long long u64;

// fp32 -> uint32 whose unsigned order is the DESCENDING float order (an ascending sort of the
// keys then yields logit descending), and back
__device__ __forceinline__ uint32_t desc_bits(float v) {
  const uint32_t u = __float_as_uint(v);
  return ~(u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u));
}
__device__ __forceinline__ float desc_float(uint32_t k) {
  k = ~k;
  return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu));
}

// ascending bitonic sort of P (a power of two) keys in LDS by the whole block
template <typename K>
__device__ __forceinline__ void bitonic_sort(K* k, int P) {
  for (int kk = 2; kk <= P; kk <<= 1) {
    for (int j = kk >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < (P >> 1); t += blockDim.x) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
        const K a = k[i], b = k[l];
        if ((a > b) == ((i & kk) == 0)) { k[i] = b; k[l] = a; }
      }
      __syncthreads();
    }
  }
}

template <int CTRL>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false);
}
// Max of an unsigned word over the wave, result in every lane: four DPP steps within the 16-lane
// rows and the two row swaps of gfx950, all VALU (the shuffle form is six ds_bpermute round trips)
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
  v = max(v, dpp_u32<0xB1>(v));   // quad_perm [1,0,3,2]: lane ^ 1
  v = max(v, dpp_u32<0x4E>(v));   // quad_perm [2,3,0,1]: lane ^ 2
  v = max(v, dpp_u32<0x141>(v));  // row_half_mirror: the other quad of the 8-lane half
  v = max(v, dpp_u32<0x140>(v));  // row_mirror: the other half of the row
  const auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);
  v = max(r[0], r[1]);
  const auto h = __builtin_amdgcn_permlane32_swap(v, v, false, false);
  return max(h[0], h[1]);
}
// Max of a 64-bit key over the wave as two word reductions: the largest high word, then the
// largest low word among the lanes that hold it (a 64-bit compare-and-select per step cost three
// times the instructions; measured)
__device__ __forceinline__ u64 wave_max_u64(u64 v) {
  const uint32_t hi = (uint32_t)(v >> 32), top = wave_max_u32(hi);
  return ((u64)top << 32) | wave_max_u32(hi == top ? (uint32_t)v : 0u);
}

}  // namespace edet
