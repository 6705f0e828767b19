// segtopk.hip -- top-k over the contiguous row segments of a batched graph (gfx950 / MI355X): dgl.topk_nodes / topk_edges and the
// selection behind dgl.nn.SortPooling.  Everything is a copy: outputs are input bits, every check can be bitwise.
//
//   order      that of torch.sort(key, stable=True, descending=...) on the CPU, per segment: NaN is the greatest key (first when
//              descending, last when ascending; a NaN with the sign bit set is a NaN), -0.0 == +0.0, equal keys keep the lower row
//              first in BOTH directions.  A key becomes order-preserving bits above the row's position inside the segment
//              (wave_select.h), after NaN and zero are canonicalised and -- descending -- the sign is flipped: comparing the 64-bit
//              pairs as integers IS that order.  The values written are the untouched input bits.
//   row mode   key = column `sortby`; values[s, j, :] = the whole row of rank j, index[s, j] = its row number inside the segment
//   col mode   every column ranked on its own; values[s, j, c], index[s, j, c]
//   padding    a segment shorter than k: ranks j >= len hold zero values and index -1
//   slot       int32 [N] (row mode) / [N, D] (column mode): the flat output rank s*k + j of a selected row (element), -1 otherwise; all
//              of it is written here, and the backward is the gather d_feat[i] = slot[i] >= 0 ? d_values[slot[i]] : 0.
//
// A PROBLEM is a segment (row mode) or a (segment, column) pair (column mode); problems are independent.
//   k <= 64          one wave per problem: lane i holds the i-th best pair; the segment is merged into them 64 candidates at a time
//                    (wave_sort + wave_bitonic_merge), a chunk in which nothing beats the current k-th is skipped on a ballot.  Four
//                    chunks of keys are loaded ahead of the merges.
//   64 < k <= 1024   one 256-thread workgroup per problem and 2048 pairs of LDS (16 KB): the lower half holds the best 1024 so far,
//                    sorted; the next chunk of up to 1024 candidates is bitonic-sorted in the upper half, compare-exchanged against the
//                    reversed lower half and the lower half bitonic-merged.  A chunk with nothing under the current k-th is skipped;
//                    a segment of <= 1024 rows is one sort (over the next power of two).
// Both: the walk writes slot = -1 for every row (element) it reads; after a fence the owners of the k ranks overwrite the selected ones,
// so no address is raced for and nothing is memset.  The epilogue copies selected rows with lanes along D.  Nothing is read on the host
// and the launch depends on (S, D, k, mode) only: capture-safe.  No atomics: reruns are bitwise equal.
//
// Column mode reads its keys with the row stride (lane i reads row i of one column): the four waves of a workgroup -- and the
// neighbouring workgroups -- take adjacent columns of one segment, so the lines are shared through L1 / L2, but nothing is staged.
// Limitation (as segattn.hip): one wave or workgroup walks a problem whatever its length.
#include "wave_select.h"

namespace mgx {

constexpr int kTopkWaveMax = kWave;  // k <= 64: the wave form
constexpr int kTopkMax = 1024;       // k <= 1024: the workgroup form
constexpr int kTopkChunk = 1024;
constexpr int kTopkLoadAhead = 4;    // wave form: chunks of 64 keys loaded before they are merged

struct TopkArgs {
  int64_t problems;        // S (row mode) or S * D (column mode)
  const int64_t* offsets;  // [S + 1]
  int64_t N, D, ld;
  const uint32_t* feat;    // [N, ld] fp32, moved as bits
  int k, sortby, descending;
  uint32_t* values;        // [S, k, D]
  int64_t* index;          // [S, k] | [S, k, D]
  int32_t* slot;           // [N] | [N, D]
};

__device__ __forceinline__ uint64_t topk_pair(uint32_t bits, uint64_t pos, int descending) {
  if ((bits & 0x7FFFFFFFu) > 0x7F800000u) bits = 0x7FC00000u;  // every NaN is the one positive NaN: above +inf
  if ((bits & 0x7FFFFFFFu) == 0u) bits = 0u;                   // -0 and +0 are one key
  if (descending) bits ^= 0x80000000u;
  return pack_pair(__uint_as_float(bits), pos);
}

// what a problem walks: its segment (clamped to the N rows there are), the key column, the stride of its slot entries
template <bool COL>
struct TopkProblem {
  int64_t seg, beg, len, col;
  const uint32_t* keys;  // key of row i of the segment: keys[i * ld]
  int32_t* slot;         // slot of row i (row mode) or of element (i, col): slot[i * slot_ld]
  int64_t slot_ld;
  __device__ __forceinline__ TopkProblem(const TopkArgs& a, int64_t prob) {
    seg = COL ? prob / a.D : prob;
    col = COL ? prob % a.D : a.sortby;
    int64_t end = a.offsets[seg + 1];
    beg = a.offsets[seg];
    end = end < a.N ? end : a.N;
    beg = beg < 0 ? 0 : (beg < end ? beg : end);
    len = end - beg;
    keys = a.feat + beg * a.ld + col;
    slot_ld = COL ? a.D : 1;
    slot = a.slot + beg * slot_ld + (COL ? col : 0);
  }
};

// The k ranks of one problem from its sorted pairs `best` (LDS, ascending; kNoPair past the segment's length), by the T threads (a
// multiple of 64) that walked it, g = 0 .. T-1.
template <bool COL>
__device__ __forceinline__ void topk_write(const TopkArgs& a, const TopkProblem<COL>& p, const uint64_t* best, int g, int T) {
  const int k = a.k;
  const int64_t D = a.D;
  const int n_sel = p.len < k ? (int)p.len : k;
  const int64_t o = p.seg * k;  // flat rank of rank 0
  for (int j = g; j < k; j += T) {
    int64_t idx = -1;
    uint32_t v = 0u;
    if (j < n_sel) {
      idx = (int64_t)(best[j] & 0xFFFFFFFFull);
      p.slot[idx * p.slot_ld] = (int32_t)(o + j);
      if (COL) v = p.keys[idx * a.ld];
    }
    if (COL) {
      a.values[(o + j) * D + p.col] = v;
      a.index[(o + j) * D + p.col] = idx;
    } else {
      a.index[o + j] = idx;
    }
  }
  if (!COL) {  // a wave per rank, lanes along the row
    const int lane = g & (kWave - 1);
    for (int j = g / kWave; j < k; j += T / kWave) {
      const bool sel = j < n_sel;
      const uint32_t* src = a.feat + (p.beg + (sel ? (int64_t)(best[j] & 0xFFFFFFFFull) : 0)) * a.ld;
      uint32_t* dst = a.values + (o + j) * D;
      for (int64_t c = lane; c < D; c += kWave) dst[c] = sel ? src[c] : 0u;
    }
  }
}

// ---------------------------------------------------------------------------------------------- k <= 64: a wave per problem
template <bool COL>
__global__ __launch_bounds__(kBlock) void seg_topk_wave_kernel(const TopkArgs a) {
  __shared__ uint64_t sbest[kWavesPerBlock][kWave];
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
  const int64_t prob = (int64_t)blockIdx.x * kWavesPerBlock + w;
  if (prob >= a.problems) return;  // the whole wave leaves; no workgroup barrier below
  const TopkProblem<COL> p(a, prob);
  uint64_t best = kNoPair;
  for (int64_t c = 0; c < p.len; c += kTopkLoadAhead * kWave) {
    uint64_t cand[kTopkLoadAhead];
#pragma unroll
    for (int u = 0; u < kTopkLoadAhead; ++u) {
      const int64_t i = c + u * kWave + lane;
      cand[u] = kNoPair;
      if (i < p.len) {
        cand[u] = topk_pair(p.keys[i * a.ld], (uint64_t)i, a.descending);
        p.slot[i * p.slot_ld] = -1;
      }
    }
#pragma unroll
    for (int u = 0; u < kTopkLoadAhead; ++u) {
      const uint64_t kth = __shfl(best, a.k - 1, kWave);
      if (__ballot(cand[u] < kth) == 0) continue;  // nothing in this chunk beats the current k-th (a chunk past the end included)
      const uint64_t sorted = wave_sort(cand[u], lane);
      const uint64_t rev = __shfl(sorted, kWave - 1 - lane, kWave);
      best = wave_bitonic_merge(rev < best ? rev : best, lane);  // the 64 smallest of both, as a bitonic sequence, sorted
    }
  }
  sbest[w][lane] = best;
  __threadfence();  // the -1 slots are in memory before a selected one is overwritten (by another lane)
  __builtin_amdgcn_wave_barrier();
  topk_write<COL>(a, p, sbest[w], lane, kWave);
}

// ---------------------------------------------------------------------------------------------- 64 < k <= 1024: a workgroup per problem
// buf[0 .. n) ascending, n a power of two >= 2, by the whole workgroup; ends on a barrier
__device__ __forceinline__ void block_bitonic(uint64_t* buf, int n, int first_k, int tid) {
  for (int k2 = first_k; k2 <= n; k2 <<= 1) {
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < n / 2; t += kBlock) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
        const bool up = (i & k2) == 0;  // the last stage (k2 == n > i) is ascending throughout
        const uint64_t x = buf[i], y = buf[l];
        if ((x > y) == up) { buf[i] = y; buf[l] = x; }
      }
      __syncthreads();
    }
  }
}

static __device__ __forceinline__ int pow2_at_least(int64_t n) {
  int p = 2;
  while (p < n) p <<= 1;
  return p;
}

template <bool COL>
__global__ __launch_bounds__(kBlock) void seg_topk_block_kernel(const TopkArgs a) {
  __shared__ uint64_t buf[2 * kTopkChunk];  // [0, 1024): the best so far, sorted; [1024, 2048): the chunk being merged in
  const int tid = threadIdx.x;
  const TopkProblem<COL> p(a, (int64_t)blockIdx.x);
  for (int i = tid; i < kTopkChunk; i += kBlock) {  // the first chunk is sorted where it stays
    uint64_t pair = kNoPair;
    if (i < p.len) {
      pair = topk_pair(p.keys[(int64_t)i * a.ld], (uint64_t)i, a.descending);
      p.slot[(int64_t)i * p.slot_ld] = -1;
    }
    buf[i] = pair;
  }
  __syncthreads();
  block_bitonic(buf, pow2_at_least(p.len < kTopkChunk ? p.len : kTopkChunk), 2, tid);
  for (int64_t c = kTopkChunk; c < p.len; c += kTopkChunk) {
    const uint64_t kth = buf[a.k - 1];
    int any = 0;
    for (int u = tid; u < kTopkChunk; u += kBlock) {
      const int64_t i = c + u;
      uint64_t pair = kNoPair;
      if (i < p.len) {
        pair = topk_pair(p.keys[i * a.ld], (uint64_t)i, a.descending);
        p.slot[i * p.slot_ld] = -1;
      }
      buf[kTopkChunk + u] = pair;
      any |= pair < kth;
    }
    if (!__syncthreads_or(any)) continue;  // nothing in this chunk beats the current k-th
    const int64_t left = p.len - c;
    block_bitonic(buf + kTopkChunk, pow2_at_least(left < kTopkChunk ? left : kTopkChunk), 2, tid);  // the rest of the half is kNoPair
    for (int i = tid; i < kTopkChunk; i += kBlock) {
      const uint64_t x = buf[i], y = buf[2 * kTopkChunk - 1 - i];
      buf[i] = y < x ? y : x;  // the 1024 smallest of both halves, a bitonic sequence
    }
    __syncthreads();
    block_bitonic(buf, kTopkChunk, kTopkChunk, tid);  // the merge steps alone
  }
  __threadfence();  // the -1 slots are in memory before a selected one is overwritten (by another thread)
  __syncthreads();
  topk_write<COL>(a, p, buf, tid, kBlock);
}

// ---------------------------------------------------------------------------------------------- backward: a gather
// CL lanes along the columns (a power of two, at most 64), 256 / CL rows per workgroup; every element of d_feat is written once
template <bool COL>
__global__ __launch_bounds__(kBlock) void seg_topk_bwd_kernel(int64_t N, int64_t D, int CL, const int32_t* __restrict__ slot,
                                                              const uint32_t* __restrict__ dv, uint32_t* __restrict__ df) {
  const int64_t row = (int64_t)blockIdx.x * (kBlock / CL) + threadIdx.x / CL;
  if (row >= N) return;
  const int32_t row_slot = COL ? -1 : slot[row];
  for (int64_t c = threadIdx.x % CL; c < D; c += CL) {
    const int32_t sl = COL ? slot[row * D + c] : row_slot;
    df[row * D + c] = sl >= 0 ? dv[(int64_t)sl * D + c] : 0u;
  }
}

static bool topk_shape_ok(int64_t k, int64_t D, int32_t mode) { return k >= 1 && k <= kTopkMax && D >= 1 && (mode == 0 || mode == 1); }

}  // namespace mgx

extern "C" int32_t mgx_segment_topk_supported(int64_t k, int64_t D, int32_t mode) { return mgx::topk_shape_ok(k, D, mode); }

extern "C" int32_t mgx_segment_topk_fwd(int64_t num_segments, const int64_t* offsets, int64_t N, int64_t D, int64_t ld, const float* feat,
                                        int64_t k, int32_t mode, int64_t sortby, int32_t descending, float* values, int64_t* index,
                                        int32_t* slot, void* stream) {
  using namespace mgx;
  MGX_ENTER();
  const char* who = "mgx_segment_topk_fwd";
  MGX_CHECK_ARG(num_segments >= 0 && N >= 0, "%s: negative num_segments or N", who);
  MGX_CHECK_ARG(D >= 1 && ld >= D, "%s: needs D >= 1 and a row stride of at least D (got D = %lld, ld = %lld)", who, (long long)D, (long long)ld);
  MGX_CHECK_ARG(k >= 1, "%s: k must be at least 1, got %lld", who, (long long)k);
  MGX_CHECK_ARG(mode == 0 || mode == 1, "%s: mode must be 0 (rows by one column) or 1 (every column on its own), got %d", who, (int)mode);
  MGX_CHECK_ARG(mode == 1 || (sortby >= 0 && sortby < D), "%s: sortby must be in [0, %lld), got %lld", who, (long long)D, (long long)sortby);
  if (k > kTopkMax) MGX_UNSUPPORTED("%s: k = %lld beyond %d", who, (long long)k, kTopkMax);
  const int64_t lim = int64_t(1) << 31;
  if (N >= lim || num_segments >= lim || D >= lim || num_segments * k >= lim || (mode == 1 && num_segments * D >= lim))
    MGX_UNSUPPORTED("%s: needs N, num_segments * k and the number of (segment, column) problems below 2^31 (got N = %lld, num_segments = "
                    "%lld, k = %lld, D = %lld)", who, (long long)N, (long long)num_segments, (long long)k, (long long)D);
  const int64_t problems = mode == 1 ? num_segments * D : num_segments;
  if (num_segments == 0) return MGX_OK;
  MGX_CHECK_ARG(offsets && values && index, "%s: offsets / values / index is NULL", who);
  MGX_CHECK_ARG(N == 0 || (feat && slot), "%s: feat / slot is NULL", who);
  TopkArgs a;
  a.problems = problems; a.offsets = offsets;
  a.N = N; a.D = D; a.ld = ld;
  a.feat = reinterpret_cast<const uint32_t*>(feat);
  a.k = (int)k; a.sortby = (int)sortby; a.descending = descending != 0;
  a.values = reinterpret_cast<uint32_t*>(values); a.index = index; a.slot = slot;
  hipStream_t s = (hipStream_t)stream;
  if (k <= kTopkWaveMax) {
    const dim3 grid((unsigned)((problems + kWavesPerBlock - 1) / kWavesPerBlock));
    if (mode == 1) hipLaunchKernelGGL(seg_topk_wave_kernel<true>, grid, dim3(kBlock), 0, s, a);
    else hipLaunchKernelGGL(seg_topk_wave_kernel<false>, grid, dim3(kBlock), 0, s, a);
  } else {
    const dim3 grid((unsigned)problems);
    if (mode == 1) hipLaunchKernelGGL(seg_topk_block_kernel<true>, grid, dim3(kBlock), 0, s, a);
    else hipLaunchKernelGGL(seg_topk_block_kernel<false>, grid, dim3(kBlock), 0, s, a);
  }
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}

extern "C" int32_t mgx_segment_topk_bwd(int64_t N, int64_t D, int32_t mode, const int32_t* slot, const float* d_values, float* d_feat,
                                        void* stream) {
  using namespace mgx;
  MGX_ENTER();
  const char* who = "mgx_segment_topk_bwd";
  MGX_CHECK_ARG(N >= 0 && D >= 1, "%s: needs N >= 0 and D >= 1 (got %lld, %lld)", who, (long long)N, (long long)D);
  MGX_CHECK_ARG(mode == 0 || mode == 1, "%s: mode must be 0 or 1, got %d", who, (int)mode);
  if (N >= (int64_t(1) << 31) || D >= (int64_t(1) << 31)) MGX_UNSUPPORTED("%s: N = %lld or D = %lld beyond 2^31", who, (long long)N, (long long)D);
  if (N == 0) return MGX_OK;
  MGX_CHECK_ARG(slot && d_feat, "%s: slot / d_feat is NULL", who);  // d_values may be NULL: no segment, every slot is -1
  int cl = 1;
  while (cl < D && cl < kWave) cl <<= 1;
  const int rows_per_block = kBlock / cl;
  const dim3 grid((unsigned)((N + rows_per_block - 1) / rows_per_block));
  const uint32_t* dv = reinterpret_cast<const uint32_t*>(d_values);
  uint32_t* df = reinterpret_cast<uint32_t*>(d_feat);
  if (mode == 1) hipLaunchKernelGGL(seg_topk_bwd_kernel<true>, grid, dim3(kBlock), 0, (hipStream_t)stream, N, D, cl, slot, dv, df);
  else hipLaunchKernelGGL(seg_topk_bwd_kernel<false>, grid, dim3(kBlock), 0, (hipStream_t)stream, N, D, cl, slot, dv, df);
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}
