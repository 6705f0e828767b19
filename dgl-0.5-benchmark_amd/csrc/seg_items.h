// seg_items.h -- work items INSIDE row segments, found on the device (segmm.hip, segmha.hip).
// An item is a run of at most `unit` rows of one segment, from offsets[r] + i * unit on, so nothing straddles two segments.  Nothing about
// the segment lengths is known on the host: seg_items_kernel (one workgroup, any R) turns offsets into the scanned per-segment item counts
// table[R + 1]; a main grid of the host-known bound ceil(n / unit) + R items finds the segment of an item by binary search in the table
// (seg_item) and leaves when it is beyond table[R].  A segment whose offsets do not lie in 0 <= beg <= end <= n gets no item.
#pragma once
#include "common.h"

namespace mgx {

// table[r] = number of items of the segments before r, table[R] = all items; one workgroup of kBlock threads, R in rounds of kBlock
static __global__ __launch_bounds__(kBlock) void seg_items_kernel(int64_t R, int64_t n, const int64_t* __restrict__ offsets, int64_t unit,
                                                                  int64_t* __restrict__ table) {
  __shared__ int64_t scan[kBlock];
  __shared__ int64_t carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int64_t base = 0; base < R; base += kBlock) {
    const int64_t r = base + threadIdx.x;
    int64_t cnt = 0;
    if (r < R) {
      const int64_t beg = offsets[r], end = offsets[r + 1];
      if (beg >= 0 && end > beg && end <= n) cnt = (end - beg + unit - 1) / unit;
    }
    scan[threadIdx.x] = cnt;
    __syncthreads();
    for (int off = 1; off < kBlock; off <<= 1) {
      const int64_t add = (int)threadIdx.x >= off ? scan[threadIdx.x - off] : 0;
      __syncthreads();
      scan[threadIdx.x] += add;
      __syncthreads();
    }
    if (r < R) table[r] = carry + scan[threadIdx.x] - cnt;
    __syncthreads();
    if (threadIdx.x == 0) carry += scan[kBlock - 1];
    __syncthreads();
  }
  if (threadIdx.x == 0) table[R] = carry;
}

// item -> (segment, first row, rows); false beyond the last item
__device__ __forceinline__ bool seg_item(const int64_t* __restrict__ table, const int64_t* __restrict__ offsets, int64_t R, int64_t item,
                                         int64_t unit, int64_t& seg, int64_t& beg, int64_t& cnt) {
  if (item >= table[R]) return false;
  int64_t lo = 1, hi = R;  // the smallest j with table[j] > item (empty segments repeat an entry)
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (table[mid] > item) hi = mid; else lo = mid + 1;
  }
  seg = lo - 1;
  beg = offsets[seg] + (item - table[seg]) * unit;
  const int64_t left = offsets[seg + 1] - beg;
  cnt = left < unit ? left : unit;
  return true;
}

}  // namespace mgx
