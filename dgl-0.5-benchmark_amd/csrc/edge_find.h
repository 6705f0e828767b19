// edge_find.h -- "is column c in row r, and under which edge id": the one scan behind mgx_edge_lookup and the existence checks of
// mgx_negative_sample (edgefind.hip).
//
// formats.hip sorts stably by row only, so a row is in edge-id order, not in column order: there is nothing to bisect and a lookup is a
// scan of the row.  A query owns an aligned group of kFindLanes consecutive lanes of a wave (four queries per wave): the group strides
// the row, lane s reading positions beg + s, beg + s + 16, ... -- adjacent lanes read adjacent indices -- and keeps the lowest edge id
// among its matches; four xor-shuffles inside the group give every lane the minimum.  No atomics and no early exit: the result does
// not depend on the order inside the row, and every loop is bounded by the row length.
#pragma once
#include "common.h"

namespace mgx {

constexpr int kFindLanes = 16;                      // lanes per query
constexpr int kFindPerBlock = kBlock / kFindLanes;  // queries per workgroup
constexpr int64_t kNoEdge = INT64_MAX;              // what a group without a match reduces to

// Lowest edge id among the positions p of [beg, end) with indices[p] == col (eids[p], or p when eids is NULL), kNoEdge without one;
// the same value in all kFindLanes lanes of the group.  EVERY lane of the group must call it (the shuffles read the whole group); a
// group with nothing to look up passes beg == end.  `sub` is the lane's number inside its group.
template <typename Idx>
__device__ __forceinline__ int64_t group_find_edge(const Idx* indices, const Idx* eids, int64_t beg, int64_t end, int64_t col, int sub) {
  int64_t best = kNoEdge;
  for (int64_t p = beg + sub; p < end; p += kFindLanes) {
    if ((int64_t)indices[p] != col) continue;
    const int64_t id = eids ? (int64_t)eids[p] : p;
    best = id < best ? id : best;
  }
#pragma unroll
  for (int off = kFindLanes >> 1; off > 0; off >>= 1) {
    const int64_t o = __shfl_xor(best, off, kWave);
    best = o < best ? o : best;
  }
  return best;
}

}  // namespace mgx
