// knn_stream.h -- the candidate streaming knn.hip and ballquery.hip share: which segment holds a row (and its number, from which the
// query-set k-NN takes the rows of the OTHER matrix's segment), one 64-candidate x 32-column tile
// staged into LDS, and the direct-form distance terms of that tile for a wave's four queries.  One 256-thread workgroup takes 16 queries,
// four per wave; a tile is stored column-major with a row of 65 floats: the transposing stores are at most 2-way conflicted, lane j then
// reads candidate j at consecutive addresses and that ONE LDS read feeds four queries.  The query's own coordinates come from
// wave-uniform addresses (scalar loads).
#pragma once
#include "common.h"

namespace mgx {

constexpr int kKnnQueries = 16;  // query rows per workgroup
constexpr int kKnnPerWave = kKnnQueries / kWavesPerBlock;
constexpr int kKnnCols = 32;     // columns staged per pass
constexpr int kKnnTileLd = kWave + 1;

// The segment of `row`: the last s with offsets[s] <= row, clamped to the N rows there are.  A row no segment holds: beg = end = 0.
// Returns the segment's number s, -1 for a row no segment holds.
__device__ __forceinline__ int64_t knn_segment_of(int64_t S, const int64_t* __restrict__ offsets, int64_t N, int64_t row, int64_t& beg,
                                                  int64_t& end) {
  beg = end = 0;
  if (row < 0 || row >= N) return -1;
  int64_t lo = 0, hi = S + 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (offsets[mid] > row) hi = mid; else lo = mid + 1;
  }
  if (lo >= 1 && lo <= S) {
    beg = offsets[lo - 1];
    end = offsets[lo];
  }
  end = end < N ? end : N;
  beg = beg < 0 ? 0 : beg;
  if (!(beg <= row && row < end)) {
    beg = end = 0;
    return -1;
  }
  return lo - 1;
}

// Rows [beg, end) of segment s of a matrix of N rows, clamped to the rows there are; s < 0 or nothing left: beg = end = 0.
__device__ __forceinline__ void knn_segment_rows(const int64_t* __restrict__ offsets, int64_t N, int64_t s, int64_t& beg, int64_t& end) {
  beg = end = 0;
  if (s < 0) return;
  beg = offsets[s];
  end = offsets[s + 1];
  end = end < N ? end : N;
  beg = beg < 0 ? 0 : beg;
  if (beg >= end) beg = end = 0;
}

// tile[c][r] = x[c0 + r, d0 + c] for r < rows (0 beyond), c < dc <= kKnnCols.  The caller puts a barrier on either side.
__device__ __forceinline__ void knn_stage_tile(float* __restrict__ tile, const float* __restrict__ x, int64_t ld, int64_t c0, int rows, int d0,
                                               int dc, int tid) {
  if (dc == kKnnCols) {
    const int c = tid & (kKnnCols - 1);
#pragma unroll
    for (int r = tid / kKnnCols; r < kWave; r += kBlock / kKnnCols)
      tile[c * kKnnTileLd + r] = r < rows ? x[(c0 + r) * ld + d0 + c] : 0.f;
  } else {
    for (int e = tid; e < kWave * dc; e += kBlock) {
      const int r = e / dc, c = e - r * dc;
      tile[c * kKnnTileLd + r] = r < rows ? x[(c0 + r) * ld + d0 + c] : 0.f;
    }
  }
}

// acc[q] += sum_c (xq[q][d0 + c] - tile[c][lane])^2 over c ascending, one fma per term
__device__ __forceinline__ void knn_tile_terms(const float* __restrict__ tile, int lane, int d0, int dc, const float* (&xq)[kKnnPerWave],
                                               float (&acc)[kKnnPerWave]) {
#pragma unroll 8
  for (int c = 0; c < dc; ++c) {
    const float v = tile[c * kKnnTileLd + lane];
#pragma unroll
    for (int q = 0; q < kKnnPerWave; ++q) {
      const float diff = xq[q][d0 + c] - v;
      acc[q] = __builtin_fmaf(diff, diff, acc[q]);
    }
  }
}

}  // namespace mgx
