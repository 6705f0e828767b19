// knn.hip -- k nearest neighbours inside the contiguous row segments of a batch of point clouds (gfx950 / MI355X): dgl.knn_graph /
// segmented_knn_graph and the graph dgl.nn.EdgeConv models rebuild before every layer.  Distances and selection in ONE walk: no
// [n, n] distance matrix is written.
//
//   distance   d(i, j) = sum_c (x[i,c] - x[j,c])^2 over c ascending, one fp32 fma per term: the DIRECT difference form (the expansion
//              |x_i|^2 + |x_j|^2 - 2 x_i.x_j cancels for clouds far from the origin).  Every j of i's segment, i itself included.
//   order      (d, j) ascending: equal distances keep the lower row first, a NaN distance is the greatest key (one canonical NaN, so
//              NaNs tie).  The pair is pack_pair(d, j - offsets[s]) of wave_select.h, compared as one 64-bit integer.
//   outputs    index int64 [N, k]: global row numbers; dist fp32 [N, k] (optional).  A segment shorter than k: ranks >= len hold index
//              -1 and dist +inf.  Every element is written: no memset.
//
// One 256-thread workgroup takes 16 consecutive query rows, four per wave.  The candidates of the union of their segments (a contiguous
// row range: segments are consecutive) stream through LDS 64 rows at a time and 32 columns per pass, stored column-major with a row of
// 65 floats: the transposing stores are at most 2-way conflicted, lane j then reads candidate j at consecutive addresses and that ONE LDS
// read feeds four queries.  The query's own coordinates come from wave-uniform addresses (scalar loads).  A candidate outside a query's
// own segment is kNoPair.  Each query keeps its 64 best pairs one per lane, ascending; a chunk in which no lane beats the current k-th is
// skipped on a ballot; up to 8 lanes that do (the common case past a segment's first chunks: about k / i candidates of chunk i) are inserted
// one at a time -- a ballot against the sorted best gives the place, the lanes above it shift up by one -- else wave_sort +
// wave_bitonic_merge as in the wave form of segtopk.hip.  Only ranks below k are exact in either path: a skipped chunk may have held ranks
// k .. 63.  A wave whose four segments do not meet the chunk skips the arithmetic (never the barriers).
// Nothing is read on the host and the launch depends on N only: capture-safe.  No atomics: reruns are bitwise equal.
// The segment search, the tile staging and the distance terms are knn_stream.h, shared with ballquery.hip.
//
// The same kernel answers a query set y [M, D] from a reference set x [N, D] (mgx_segment_knn_query: PyG's knn(x, y, k, batch_x,
// batch_y), the neighbour step of PointNet++'s feature propagation): the queries and their offsets are operands of their own, query
// segment s is answered from reference segment s, and the self k-NN above passes x and offsets twice.  Segments are consecutive in both
// matrices, so the union of the reference segments of 16 consecutive queries is still one contiguous row range.  Optional third
// output, the interpolation weights of the ranks: weight = (1 / (d + eps)) / sum over the valid ranks, 0 at a padded rank; the sum is a
// butterfly over the wave -- a balanced tree over the ranks padded with zeros to 64 -- so it does not depend on k and is deterministic.
#include "knn_stream.h"
#include "wave_select.h"

namespace mgx {

constexpr int kKnnMaxK = kWave;  // one rank per lane
constexpr int kKnnMaxD = 256;
constexpr int kKnnInsertMax = 8;  // candidates of a chunk under the current k-th that are inserted one by one; more: sort and merge

// Operands: the references x [N, ld] in S segments (offsets), the queries y [M, ldq] in S segments (q_offsets).  The self k-NN is y = x,
// q_offsets = offsets.  weight (optional): the normalised inverse-distance weights of the ranks, see mgx_segment_knn_query.
__global__ __launch_bounds__(kBlock) void segment_knn_kernel(int64_t S, const int64_t* __restrict__ offsets, int64_t N, int64_t ld,
                                                             const float* __restrict__ x, const int64_t* __restrict__ q_offsets, int64_t M,
                                                             int64_t ldq, const float* __restrict__ y, int D, int k, float eps,
                                                             int64_t* __restrict__ index, float* __restrict__ dist,
                                                             float* __restrict__ weight) {
  __shared__ float tile[kKnnCols * kKnnTileLd];
  __shared__ int64_t sbeg[kKnnQueries], send[kKnnQueries];
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int w = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int64_t q0 = (int64_t)blockIdx.x * kKnnQueries;
  if (tid < kKnnQueries) {  // the reference rows of the segment that holds query row q0 + tid; a row no segment holds: k ranks of padding
    int64_t beg, end;
    const int64_t s = knn_segment_of(S, q_offsets, M, q0 + tid, beg, end);
    knn_segment_rows(offsets, N, s, beg, end);
    sbeg[tid] = beg;
    send[tid] = end;
  }
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
  int64_t qbeg[kKnnPerWave], qend[kKnnPerWave], wlo = N, whi = 0;  // ... and the rows this wave has a use for
  const float* xq[kKnnPerWave];
  uint64_t best[kKnnPerWave];
#pragma unroll
  for (int q = 0; q < kKnnPerWave; ++q) {
    qbeg[q] = sbeg[w * kKnnPerWave + q];
    qend[q] = send[w * kKnnPerWave + q];
    if (qbeg[q] < qend[q]) {
      wlo = qbeg[q] < wlo ? qbeg[q] : wlo;
      whi = qend[q] > whi ? qend[q] : whi;
    }
    const int64_t row = q0 + w * kKnnPerWave + q;
    xq[q] = y + (row < M ? row : M - 1) * ldq;
    best[q] = kNoPair;
  }
  for (int64_t c0 = lo; c0 < hi; c0 += kWave) {
    const int rows = hi - c0 < kWave ? (int)(hi - c0) : kWave;
    const bool mine = c0 < whi && c0 + kWave > wlo;  // wave-uniform
    float acc[kKnnPerWave];
#pragma unroll
    for (int q = 0; q < kKnnPerWave; ++q) acc[q] = 0.f;
    for (int d0 = 0; d0 < D; d0 += kKnnCols) {
      const int dc = D - d0 < kKnnCols ? D - d0 : kKnnCols;
      __syncthreads();  // the previous tile has been read
      knn_stage_tile(tile, x, ld, c0, rows, d0, dc, tid);
      __syncthreads();
      if (!mine) continue;
      knn_tile_terms(tile, lane, d0, dc, xq, acc);
    }
    if (!mine) continue;
    const int64_t g = c0 + lane;
#pragma unroll
    for (int q = 0; q < kKnnPerWave; ++q) {
      float d = acc[q];
      if (d != d) d = __uint_as_float(0x7FC00000u);  // every NaN is the one positive NaN: above +inf, ties by row
      const uint64_t cand = (g >= qbeg[q] && g < qend[q]) ? pack_pair(d, (uint64_t)(g - qbeg[q])) : kNoPair;
      const uint64_t kth = __shfl(best[q], k - 1, kWave);
      uint64_t pass = __ballot(cand < kth);
      if (pass == 0) continue;  // nothing in this chunk beats the current k-th
      if (__popcll(pass) <= kKnnInsertMax) {  // a few: each goes to its place among the sorted best, the lanes above move up by one
        do {
          const int l = __builtin_ctzll(pass);  // wave-uniform
          const uint64_t v = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(cand >> 32), l) << 32) |
                             (uint32_t)__builtin_amdgcn_readlane((int)(cand & 0xFFFFFFFFull), l);
          const int pos = __popcll(__ballot(best[q] < v));  // pairs are distinct; best is ascending: lanes 0 .. pos-1 stay
          const uint64_t up = __shfl_up(best[q], 1, kWave);
          best[q] = lane < pos ? best[q] : (lane == pos ? v : up);
          pass &= pass - 1;
        } while (pass);
        continue;
      }
      const uint64_t sorted = wave_sort(cand, lane);
      const uint64_t rev = __shfl(sorted, kWave - 1 - lane, kWave);
      best[q] = wave_bitonic_merge(rev < best[q] ? rev : best[q], lane);  // the 64 smallest of both, as a bitonic sequence, sorted
    }
  }
  if (lane < k) {
#pragma unroll
    for (int q = 0; q < kKnnPerWave; ++q) {
      const int64_t row = q0 + w * kKnnPerWave + q;
      if (row >= M) continue;
      const uint64_t p = best[q];
      const uint32_t b = (uint32_t)(p >> 32);
      index[row * k + lane] = p == kNoPair ? (int64_t)-1 : qbeg[q] + (int64_t)(p & 0xFFFFFFFFull);
      if (dist) dist[row * k + lane] = p == kNoPair ? __uint_as_float(0x7F800000u) : __uint_as_float((b >> 31) ? b ^ 0x80000000u : ~b);
    }
  }
  if (weight) {  // 1 / (d + eps) of the valid ranks over their sum: a balanced tree over the ranks, rank r and rank r ^ 1 first
#pragma unroll
    for (int q = 0; q < kKnnPerWave; ++q) {
      const int64_t row = q0 + w * kKnnPerWave + q;
      if (row >= M) continue;  // wave-uniform
      const uint64_t p = best[q];
      const uint32_t b = (uint32_t)(p >> 32);
      const bool valid = lane < k && p != kNoPair;
      const float inv = valid ? 1.f / (__uint_as_float((b >> 31) ? b ^ 0x80000000u : ~b) + eps) : 0.f;
      float sum = inv;
#pragma unroll
      for (int o = 1; o < kWave; o <<= 1) sum += __shfl_xor(sum, o, kWave);
      if (lane < k) weight[row * k + lane] = valid ? inv / sum : 0.f;
    }
  }
}

static bool knn_shape_ok(int64_t k, int64_t D) { return k >= 1 && k <= kKnnMaxK && D >= 1 && D <= kKnnMaxD; }

}  // namespace mgx

extern "C" int32_t mgx_segment_knn_supported(int64_t k, int64_t D) { return mgx::knn_shape_ok(k, D); }

// The checks and the launch of both entry points.
static int32_t knn_launch(const char* who, int64_t S, const int64_t* offsets, int64_t N, int64_t ld, const float* x, const int64_t* q_offsets,
                          int64_t M, int64_t ldq, const float* y, int64_t D, int64_t k, float eps, int64_t* index, float* dist, float* weight,
                          void* stream) {
  using namespace mgx;
  MGX_CHECK_ARG(S >= 0 && N >= 0 && M >= 0, "%s: negative num_segments, N or M", who);
  MGX_CHECK_ARG(D >= 1 && ld >= D && ldq >= D, "%s: needs D >= 1 and a row stride of at least D (got D = %lld, ld = %lld, ldq = %lld)", who,
                (long long)D, (long long)ld, (long long)ldq);
  MGX_CHECK_ARG(k >= 1, "%s: k must be at least 1, got %lld", who, (long long)k);
  if (!knn_shape_ok(k, D)) MGX_UNSUPPORTED("%s: k = %lld beyond %d or D = %lld beyond %d", who, (long long)k, kKnnMaxK, (long long)D, kKnnMaxD);
  const int64_t lim = int64_t(1) << 31;
  if (N >= lim || M >= lim || S >= lim || ld >= lim || ldq >= lim || N * ld >= lim / 2 || M * ldq >= lim / 2)
    MGX_UNSUPPORTED("%s: needs N, M and num_segments below 2^31 and each matrix below 4 GiB (got N = %lld, M = %lld, num_segments = %lld, "
                    "ld = %lld, ldq = %lld)", who, (long long)N, (long long)M, (long long)S, (long long)ld, (long long)ldq);
  if (M == 0) return MGX_OK;
  MGX_CHECK_ARG(offsets && q_offsets && y && index && (x || N == 0), "%s: offsets / x / index is NULL", who);
  const dim3 grid((unsigned)((M + kKnnQueries - 1) / kKnnQueries));
  hipLaunchKernelGGL(segment_knn_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, S, offsets, N, ld, x, q_offsets, M, ldq, y, (int)D, (int)k,
                     eps, index, dist, weight);
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}

extern "C" int32_t mgx_segment_knn(int64_t num_segments, const int64_t* offsets, int64_t N, int64_t D, int64_t ld, const float* x, int64_t k,
                                   int64_t* index, float* dist, void* stream) {
  MGX_ENTER();
  return knn_launch("mgx_segment_knn", num_segments, offsets, N, ld, x, offsets, N, ld, x, D, k, 0.f, index, dist, nullptr, stream);
}

extern "C" int32_t mgx_segment_knn_query_supported(int64_t k, int64_t D) { return mgx::knn_shape_ok(k, D); }

extern "C" int32_t mgx_segment_knn_query(int64_t num_segments, const int64_t* offsets, int64_t N, int64_t ld, const float* x,
                                         const int64_t* q_offsets, int64_t M, int64_t ldq, const float* y, int64_t D, int64_t k, float eps,
                                         int64_t* index, float* dist, float* weight, void* stream) {
  MGX_ENTER();
  return knn_launch("mgx_segment_knn_query", num_segments, offsets, N, ld, x, q_offsets, M, ldq, y, D, k, eps, index, dist, weight, stream);
}
