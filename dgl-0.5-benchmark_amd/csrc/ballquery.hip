// ballquery.hip -- fixed-radius neighbour query of chosen centre rows inside the contiguous row segments of a batch of point clouds
// (gfx950 / MI355X): the PointNet++ "ball query", the grouping step after fps.hip.  Distances and selection in ONE walk: no [M, n]
// distance matrix is written.
//
//   query q, centre row c = centers[q], inside the segment that holds c:
//   index[q, :]  the first K rows j in ASCENDING ROW ORDER (not the nearest) with d(c, j) = sum_c' (x[c,c'] - x[j,c'])^2 <= radius2 --
//                fp32, c' ascending, one fma per term, the direct form of knn.hip; a NaN d is outside the ball
//   count[q]     how many were found, at most K
//   ranks >= count[q] hold index[q, 0] with pad_first (every query then has K entries: the PointNet++ convention), else -1
//   count[q] == 0 (a NaN centre, c = -1, c in no segment): every rank is -1.  Every element is written: no memset.
//
// The streaming is knn.hip's (knn_stream.h): one 256-thread workgroup takes 16 queries, four per wave, each query's segment found by the
// same binary search, and the rows of the union of their segments pass through LDS 64 candidates by 32 columns at a time.  Selection is
// a ballot of "inside the ball" and a prefix popcount: that IS the hit's rank in ascending row order.  A full query takes part no
// more, and the workgroup stops streaming once all 16 are full: every wave posts "my four are full" in LDS and all read the four flags
// after the barrier at the top of the next chunk, so the decision is workgroup-uniform (there are barriers inside the loop).
// Nothing is read on the host and the launch depends on M only: capture-safe.  No atomics: reruns are bitwise equal.
#include "knn_stream.h"

namespace mgx {

constexpr int kBallMaxK = kWave;  // one rank per lane when padding
constexpr int kBallMaxD = 256;

__global__ __launch_bounds__(kBlock) void segment_ball_query_kernel(int64_t S, const int64_t* __restrict__ offsets, int64_t N, int D, int64_t ld,
                                                                    const float* __restrict__ x, int64_t M,
                                                                    const int64_t* __restrict__ centers, float radius2, int K, int pad_first,
                                                                    int64_t* __restrict__ index, int32_t* __restrict__ count) {
  __shared__ float tile[kKnnCols * kKnnTileLd];
  __shared__ int64_t sbeg[kKnnQueries], send[kKnnQueries], srow[kKnnQueries];
  __shared__ int wfull[kWavesPerBlock];
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int w = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int64_t q0 = (int64_t)blockIdx.x * kKnnQueries;
  if (tid < kKnnQueries) {  // the segment of the centre of query q0 + tid; no query, no centre or a centre no segment holds: beg = end = 0
    const int64_t q = q0 + tid;
    const int64_t row = q < M ? centers[q] : -1;
    int64_t beg, end;
    knn_segment_of(S, offsets, N, row, beg, end);
    sbeg[tid] = beg;
    send[tid] = end;
    srow[tid] = beg < end ? row : 0;
  }
  if (tid < kWavesPerBlock) wfull[tid] = 0;
  __syncthreads();
  int64_t lo = N, hi = 0;  // the rows the workgroup streams
#pragma unroll
  for (int q = 0; q < kKnnQueries; ++q) {
    const int64_t b = sbeg[q], e = send[q];
    if (b < e) {
      lo = b < lo ? b : lo;
      hi = e > hi ? e : hi;
    }
  }
  int64_t qbeg[kKnnPerWave], qend[kKnnPerWave], first[kKnnPerWave];
  const float* xq[kKnnPerWave];
  int cnt[kKnnPerWave];
#pragma unroll
  for (int q = 0; q < kKnnPerWave; ++q) {
    qbeg[q] = sbeg[w * kKnnPerWave + q];
    qend[q] = send[w * kKnnPerWave + q];
    xq[q] = x + srow[w * kKnnPerWave + q] * ld;
    cnt[q] = 0;
    first[q] = -1;
  }
  for (int64_t c0 = lo; c0 < hi; c0 += kWave) {
    __syncthreads();  // the flags of the chunk before are posted (and its last tile has been read)
    if (wfull[0] & wfull[1] & wfull[2] & wfull[3]) break;  // workgroup-uniform
    const int rows = hi - c0 < kWave ? (int)(hi - c0) : kWave;
    bool mine = false;  // wave-uniform: a query of this wave that is not full and whose segment meets the chunk
#pragma unroll
    for (int q = 0; q < kKnnPerWave; ++q) mine = mine || (cnt[q] < K && c0 < qend[q] && c0 + kWave > qbeg[q]);
    float acc[kKnnPerWave];
#pragma unroll
    for (int q = 0; q < kKnnPerWave; ++q) acc[q] = 0.f;
    for (int d0 = 0; d0 < D; d0 += kKnnCols) {
      const int dc = D - d0 < kKnnCols ? D - d0 : kKnnCols;
      if (d0) __syncthreads();  // the previous tile has been read
      knn_stage_tile(tile, x, ld, c0, rows, d0, dc, tid);
      __syncthreads();
      if (!mine) continue;
      knn_tile_terms(tile, lane, d0, dc, xq, acc);
    }
    bool full = true;  // wave-uniform: a query past its segment's end can find nothing more
    const int64_t g = c0 + lane;
#pragma unroll
    for (int q = 0; q < kKnnPerWave; ++q) {
      if (mine && cnt[q] < K) {
        const bool in = g >= qbeg[q] && g < qend[q] && acc[q] <= radius2;  // a NaN distance compares false
        const uint64_t hit = __ballot(in);
        if (hit) {
          const int rank = cnt[q] + __popcll(hit & ((uint64_t(1) << lane) - 1));
          const int64_t qi = q0 + w * kKnnPerWave + q;
          if (in && rank < K) index[qi * K + rank] = g;
          if (cnt[q] == 0) first[q] = c0 + __builtin_ctzll(hit);
          const int total = cnt[q] + __popcll(hit);
          cnt[q] = total < K ? total : K;
        }
      }
      full = full && (cnt[q] >= K || c0 + kWave >= qend[q]);
    }
    if (lane == 0) wfull[w] = full;
  }
  if (lane < K) {
#pragma unroll
    for (int q = 0; q < kKnnPerWave; ++q) {
      const int64_t qi = q0 + w * kKnnPerWave + q;
      if (qi >= M) continue;
      if (lane >= cnt[q]) index[qi * K + lane] = pad_first ? first[q] : -1;  // first is -1 when nothing was found
    }
  }
  if (lane < kKnnPerWave) {
    const int64_t qi = q0 + w * kKnnPerWave + lane;
    int c = cnt[0];
#pragma unroll
    for (int q = 1; q < kKnnPerWave; ++q) c = lane == q ? cnt[q] : c;
    if (qi < M) count[qi] = c;
  }
}

static bool ball_shape_ok(int64_t K, int64_t D) { return K >= 1 && K <= kBallMaxK && D >= 1 && D <= kBallMaxD; }

}  // namespace mgx

extern "C" int32_t mgx_segment_ball_query_supported(int64_t K, int64_t D) { return mgx::ball_shape_ok(K, D); }

extern "C" int32_t mgx_segment_ball_query(int64_t num_segments, const int64_t* offsets, int64_t N, int64_t D, int64_t ld, const float* x, int64_t M,
                                          const int64_t* centers, float radius2, int64_t K, int32_t pad_first, int64_t* index, int32_t* count,
                                          void* stream) {
  using namespace mgx;
  MGX_ENTER();
  const char* who = "mgx_segment_ball_query";
  MGX_CHECK_ARG(num_segments >= 0 && N >= 0 && M >= 0, "%s: negative num_segments, N or M", who);
  MGX_CHECK_ARG(D >= 1 && ld >= D, "%s: needs D >= 1 and a row stride of at least D (got D = %lld, ld = %lld)", who, (long long)D, (long long)ld);
  MGX_CHECK_ARG(K >= 1, "%s: K must be at least 1, got %lld", who, (long long)K);
  if (!ball_shape_ok(K, D)) MGX_UNSUPPORTED("%s: K = %lld beyond %d or D = %lld beyond %d", who, (long long)K, kBallMaxK, (long long)D, kBallMaxD);
  const int64_t lim = int64_t(1) << 31;
  if (N >= lim || num_segments >= lim || ld >= lim || N * ld >= lim / 2 || M >= lim)
    MGX_UNSUPPORTED("%s: needs N and num_segments and M below 2^31 and x below 4 GiB (got N = %lld, num_segments = %lld, ld = %lld, "
                    "M = %lld)", who, (long long)N, (long long)num_segments, (long long)ld, (long long)M);
  if (M == 0) return MGX_OK;
  MGX_CHECK_ARG(offsets && centers && index && count && (x || N == 0), "%s: offsets / x / centers / index / count is NULL", who);
  const dim3 grid((unsigned)((M + kKnnQueries - 1) / kKnnQueries));
  hipLaunchKernelGGL(segment_ball_query_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, num_segments, offsets, N, (int)D, ld, x, M, centers,
                     radius2, (int)K, (int)pad_first, index, count);
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}
