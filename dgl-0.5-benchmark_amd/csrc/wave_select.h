// wave_select.h -- (key, position) pairs and the wave-wide sorting network that the selection kernels share: weighted sampling and
// select_topk over CSR rows (sample.hip), top-k over the row segments of a batched graph (segtopk.hip).
#pragma once
#include "common.h"

namespace mgx {

// A candidate is ONE 64-bit number: the key as order-preserving bits above the position inside the row (or segment), so that pairs
// compare as (key, position) -- equal keys fall to the lower position -- and all-ones (kNoPair) sorts after every real pair, +inf keys
// included.  (Rows and segments are taken to be shorter than 2^32 - 1.)
constexpr uint64_t kNoPair = ~0ull;

__device__ __forceinline__ uint64_t pack_pair(float key, uint64_t rel_pos) {
  const uint32_t b = __float_as_uint(key);
  return ((uint64_t)(b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u)) << 32) | (rel_pos & 0xFFFFFFFFull);
}

// v of the 64 lanes in ascending lane order (bitonic network, 21 compare-exchanges over ds_bpermute)
__device__ __forceinline__ uint64_t wave_sort(uint64_t v, int lane) {
#pragma unroll
  for (int k = 2; k <= kWave; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      const uint64_t o = __shfl_xor(v, j, kWave);
      const bool keep_min = ((lane & j) == 0) == ((lane & k) == 0);
      v = keep_min ? (o < v ? o : v) : (o > v ? o : v);
    }
  }
  return v;
}
// the last 6 steps alone: sorts a bitonic sequence
__device__ __forceinline__ uint64_t wave_bitonic_merge(uint64_t v, int lane) {
#pragma unroll
  for (int j = kWave >> 1; j > 0; j >>= 1) {
    const uint64_t o = __shfl_xor(v, j, kWave);
    v = ((lane & j) == 0) ? (o < v ? o : v) : (o > v ? o : v);
  }
  return v;
}

}  // namespace mgx
