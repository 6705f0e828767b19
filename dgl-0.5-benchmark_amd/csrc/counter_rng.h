// counter_rng.h -- the counter-based random numbers of the samplers (sample.hip, edgefind.hip): pure functions of their arguments, so
// a sample never depends on the launch geometry or on the index width of the graph.
#pragma once
#include <stdint.h>

namespace mgx {

__device__ __forceinline__ uint64_t mix64(uint64_t x) {  // splitmix64 finaliser
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// ---- negative sampling (mgx_negative_sample) -----------------------------------------------------------------------------------
// Try t (0 <= t < max_tries <= kNegMaxTries) of draw (e, j) -- positive edge e, j < k -- proposes the destination
//
//     c  = (e * k + j) * 64 + t                     (64 = kNegMaxTries: a counter of its own for every try of every draw)
//     r  = mix64(rng_seed ^ mix64(c))               (all arithmetic modulo 2^64, >> is a logical shift)
//     v' = ((r >> 32) * num_dst_nodes) >> 32        (num_dst_nodes < 2^31: the product stays below 2^63)
//
// which is floor(u * num_dst_nodes) for u = the upper 32 bits of r as a fraction.  A host restatement needs nothing beyond wrapping
// int64 multiplication and addition and a shift followed by a mask (mi355x_graph/sampling.py: _mix64_t, negative_candidates).
constexpr int kNegMaxTries = 64;

__device__ __forceinline__ int64_t negative_candidate(uint64_t rng_seed, int64_t draw, int t, int64_t num_dst_nodes) {
  const uint64_t c = (uint64_t)draw * (uint64_t)kNegMaxTries + (uint64_t)t;
  const uint64_t r = mix64(rng_seed ^ mix64(c));
  return (int64_t)(((r >> 32) * (uint64_t)num_dst_nodes) >> 32);
}

}  // namespace mgx
