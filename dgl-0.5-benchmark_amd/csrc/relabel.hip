// relabel.hip -- global node ids -> the local ids of a sampled block / an induced subgraph, on the device (integer work only).
//
// Replaces the torch index arithmetic behind dgl.to_block (reddit/ns-sage-dgl.py:132-141, one call per layer and step) and
// g.subgraph(nodes) (dgl_cluster_sampler.py:99, one call per cluster batch).
//
// Both share one scheme: a look-up table lut[num_nodes] of int32, -1 = "not in the output", filled by hipMemsetAsync inside the entry
// point (no state survives a call), and for a block a bitmap of the sources that are not destinations.  A block's sources must come
// out as [dst_nodes..., the other sources in ASCENDING global id] -- what torch.unique gives the composition -- and a bitmap walked
// word by word, bit by bit, IS that order: no sort, no hash probing, the same result on every run.
//
//   mgx_to_block        scatter (lut[dst_nodes[i]] = i by atomicCAS: a lost swap is a duplicate) -> mark (every edge: its destination
//                       must be in the table, its source sets a bit when it is not) -> rank (popcount per word, exclusive scan over the
//                       words) -> emit (the owner of a word walks its bits: src_nodes, lut) -> apply (l_src, l_dst in the requested
//                       width, and the in-CSR row pointer by boundary detection when the edges arrive grouped by destination)
//   mgx_node_subgraph_* scatter, then a wave per selected row of the parent's in-CSR: count the in-edges whose source is selected too,
//                       and -- after the caller's cumsum -- write them in CSR order (ballot + prefix popcount, no atomics)
//   mgx_frontier_exclude_*  the same count / cumsum / fill protocol over a sampled frontier (edges grouped by seed): drop the edges whose
//                       id is in a short ascending list -- the seed edges of a link-prediction batch and their reverses
//   mgx_compact_nodes   mark (every id sets its bit) -> rank -> emit -> apply: the distinct ids ascending and each entry's position among
//                       them, what sort + unique + inverse give (dgl.compact_graphs, g.edge_subgraph, the pair graphs of an edge batch)
//
// Every phase is its own launch on the caller's stream: what one phase wrote is read by the next only across a kernel boundary, never
// through a hand-off between workgroups of one launch.  The scan over the bitmap words is ONE workgroup of 1024 threads striding over
// the words (1024 words = 65 536 nodes per round, the running total carried in a register): 38 k words for a products-sized graph are
// 37 rounds, and one launch is cheaper than the partials / scan-of-partials / add-back triple at every size met here.
//
// Every id read from a caller's array is checked against [0, num_nodes) before it indexes anything; a bad id sets an error bit in
// `result` and the thread skips.  The only atomics are the CAS of the scatter, the OR of the bitmap and the OR of the error bits.
#include "common.h"

namespace mgx {

constexpr int kRankBlock = 1024;  // the one workgroup of the word scan
constexpr int kMaxGrid = 2048;    // grid-stride launches: at most this many workgroups

enum { kErrDuplicate = 1, kErrDstMissing = 2, kErrRange = 4, kErrUnsorted = 8, kRowsNotByEid = 16 };

static inline dim3 stride_grid(int64_t n) {
  int64_t b = (n + kBlock - 1) / kBlock;
  if (b < 1) b = 1;
  return dim3((unsigned)(b < kMaxGrid ? b : kMaxGrid));
}

__device__ __forceinline__ void flag_error(int64_t* flags, int bit) { atomicOr((unsigned long long*)flags, (unsigned long long)bit); }
__device__ __forceinline__ bool in_range(int64_t v, int64_t n) { return (uint64_t)v < (uint64_t)n; }

// lut[nodes[i]] = i; `copy` (or NULL) receives nodes[0..n) unchanged (the head of a block's source list)
__global__ __launch_bounds__(kBlock) void relabel_scatter_kernel(const int64_t* nodes, int64_t n, int64_t num_nodes, int32_t* lut,
                                                                 int64_t* copy, int64_t* flags) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const int64_t v = nodes[i];
    if (copy) copy[i] = v;
    if (!in_range(v, num_nodes)) { flag_error(flags, kErrRange); continue; }
    if (atomicCAS(&lut[v], -1, (int32_t)i) != -1) flag_error(flags, kErrDuplicate);
  }
}

__global__ __launch_bounds__(kBlock) void block_mark_kernel(const int64_t* src, const int64_t* dst, int64_t nnz, int64_t num_nodes,
                                                            const int32_t* lut, unsigned long long* bits, int64_t* flags) {
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < nnz; e += (int64_t)gridDim.x * kBlock) {
    const int64_t d = dst[e], s = src[e];
    if (!in_range(d, num_nodes)) flag_error(flags, kErrRange);
    else if (lut[d] < 0) flag_error(flags, kErrDstMissing);
    if (!in_range(s, num_nodes)) { flag_error(flags, kErrRange); continue; }
    if (lut[s] >= 0) continue;
    const unsigned long long m = 1ull << (s & 63);
    // the plain read may be stale and then only costs the atomic it was meant to save (one source repeated by every edge)
    if (!(bits[s >> 6] & m)) atomicOr(&bits[s >> 6], m);
  }
}

// word_rank[w] = set bits in the words before w; *num_src = num_dst + all set bits.  ONE workgroup.
__global__ __launch_bounds__(kRankBlock) void block_rank_kernel(const unsigned long long* bits, int64_t words, int32_t* word_rank,
                                                                int64_t num_dst, int64_t* num_src) {
  __shared__ int32_t wave_total[kRankBlock / kWave];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  int32_t carry = 0;  // the same number in every thread
  for (int64_t base = 0; base < words; base += kRankBlock) {
    const int64_t w = base + threadIdx.x;
    const int32_t c = w < words ? __popcll(bits[w]) : 0;
    int32_t incl = c;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
      const int32_t t = __shfl_up(incl, off, kWave);
      if (lane >= off) incl += t;
    }
    if (lane == kWave - 1) wave_total[wave] = incl;
    __syncthreads();
    int32_t before = 0, all = 0;
#pragma unroll
    for (int i = 0; i < kRankBlock / kWave; ++i) {
      const int32_t t = wave_total[i];
      before += i < wave ? t : 0;
      all += t;
    }
    if (w < words) word_rank[w] = carry + before + incl - c;
    carry += all;
    __syncthreads();  // wave_total is rewritten by the next round
  }
  if (threadIdx.x == 0) *num_src = num_dst + (int64_t)carry;
}

// the owner of a word walks its bits in ascending order: the sources that are no destinations, by ascending global id
__global__ __launch_bounds__(kBlock) void block_emit_kernel(const unsigned long long* bits, int64_t words, const int32_t* word_rank,
                                                            int64_t num_dst, int64_t capacity, int32_t* lut, int64_t* src_nodes) {
  for (int64_t w = (int64_t)blockIdx.x * kBlock + threadIdx.x; w < words; w += (int64_t)gridDim.x * kBlock) {
    unsigned long long m = bits[w];
    int64_t r = num_dst + (int64_t)word_rank[w];
    for (; m && r < capacity; m &= m - 1, ++r) {  // r < capacity always holds (one bit per distinct in-range source); checked all the same
      const int64_t node = w * 64 + __builtin_ctzll(m);
      src_nodes[r] = node;
      lut[node] = (int32_t)r;
    }
  }
}

// l_src / l_dst of every edge; with `indptr` the row pointer of the in-CSR: the thread of edge e fills indptr[k] = e for every row k in
// (row of edge e - 1, row of edge e], the first edge the rows up to its own, the last edge the rows after its own as well.
template <typename Out>
__global__ __launch_bounds__(kBlock) void block_apply_kernel(const int64_t* src, const int64_t* dst, int64_t nnz, int64_t num_nodes,
                                                             int64_t num_dst, const int32_t* lut, Out* l_src, Out* l_dst, Out* indptr,
                                                             int64_t* flags) {
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < nnz; e += (int64_t)gridDim.x * kBlock) {
    const int64_t s = src[e], d = dst[e];
    const int64_t ls = in_range(s, num_nodes) ? (int64_t)lut[s] : -1;
    int64_t ld = in_range(d, num_nodes) ? (int64_t)lut[d] : -1;
    if (ld >= num_dst) ld = -1;  // a source that is no destination: the mark phase has reported it
    l_src[e] = (Out)(ls < 0 ? 0 : ls);
    l_dst[e] = (Out)(ld < 0 ? 0 : ld);
    if (!indptr || ld < 0) continue;
    int64_t prev = -1;  // row of the edge before; rows (prev, ld] begin at e
    if (e > 0) {
      const int64_t dp = dst[e - 1];
      prev = in_range(dp, num_nodes) ? (int64_t)lut[dp] : -1;
      if (prev < 0 || prev >= num_dst) continue;  // reported by the mark phase
      if (ld < prev) { flag_error(flags, kErrUnsorted); continue; }
    }
    for (int64_t k = prev + 1; k <= ld; ++k) indptr[k] = (Out)e;
    if (e == nnz - 1)
      for (int64_t k = ld + 1; k <= num_dst; ++k) indptr[k] = (Out)nnz;
  }
}

// ---- induced subgraph: one wave per selected row of the parent's in-CSR ------------------------------------------------------
template <typename Idx>
__global__ __launch_bounds__(kBlock) void subgraph_count_kernel(const Idx* indptr, const Idx* indices, const Idx* eids, int64_t num_nodes,
                                                                const int64_t* sel, int64_t num_sel, const int32_t* lut, int64_t* counts,
                                                                int64_t* flags) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t i = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (i >= num_sel) return;
  const int64_t v = sel[i];
  int64_t cnt = 0;
  bool bad = false, unordered = false;
  if (in_range(v, num_nodes)) {  // else: reported by the scatter
    const int64_t beg = (int64_t)indptr[v], end = (int64_t)indptr[v + 1];
    for (int64_t c = beg; c < end; c += kWave) {
      const int64_t p = c + lane;
      bool keep = false;
      if (p < end) {
        const int64_t u = (int64_t)indices[p];
        if (in_range(u, num_nodes)) keep = lut[u] >= 0; else bad = true;
        if (eids && p > beg) unordered |= eids[p] < eids[p - 1];
      }
      cnt += __popcll(__ballot(keep));
    }
  }
  const bool any_bad = __ballot(bad) != 0, any_unordered = __ballot(unordered) != 0;
  if (lane == 0) {
    counts[i] = cnt;
    if (any_bad) flag_error(flags, kErrRange);
    if (any_unordered) flag_error(flags, kRowsNotByEid);
  }
}

template <typename Idx, typename Out>
__global__ __launch_bounds__(kBlock) void subgraph_fill_kernel(const Idx* indptr, const Idx* indices, const Idx* eids, int64_t num_nodes,
                                                               const int64_t* sel, int64_t num_sel, const int32_t* lut,
                                                               const int64_t* offsets, Out* l_src, Out* l_dst, int64_t* parent_eid) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t i = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (i >= num_sel) return;
  const int64_t v = sel[i];
  if (!in_range(v, num_nodes)) return;
  int64_t o = offsets[i];
  const int64_t stop = offsets[i + 1];  // never past the room the caller left for this row
  const int64_t beg = (int64_t)indptr[v], end = (int64_t)indptr[v + 1];
  for (int64_t c = beg; c < end; c += kWave) {
    const int64_t p = c + lane;
    int32_t local = -1;
    if (p < end) {
      const int64_t u = (int64_t)indices[p];
      if (in_range(u, num_nodes)) local = lut[u];
    }
    const uint64_t mask = __ballot(local >= 0);
    const int64_t at = o + __popcll(mask & ((1ull << lane) - 1ull));
    if (local >= 0 && at < stop) {
      l_src[at] = (Out)local;
      l_dst[at] = (Out)i;
      parent_eid[at] = eids ? (int64_t)eids[p] : p;
    }
    o += __popcll(mask);
  }
}

// ---- seed-edge exclusion: one wave per seed of a sampled frontier ------------------------------------------------------------
// x in the ascending list a[0..n)?  At most 64 halvings; the list (the edge ids of one batch and their reverses, a few thousand) stays
// in cache, where a bitmap over all E edges would have to be cleared for every batch.
__device__ __forceinline__ bool in_sorted_list(const int64_t* a, int64_t n, int64_t x) {
  int64_t lo = 0, hi = n;
  for (int it = 0; it < 64 && lo < hi; ++it) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo < n && a[lo] == x;
}

template <typename Idx>
__global__ __launch_bounds__(kBlock) void frontier_exclude_count_kernel(int64_t num_seeds, const int64_t* offsets, const Idx* eid,
                                                                        int64_t num_excl, const int64_t* excl, int64_t* counts) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t i = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (i >= num_seeds) return;
  const int64_t beg = offsets[i], end = offsets[i + 1];
  int64_t cnt = 0;
  for (int64_t c = beg; c < end; c += kWave) {
    const int64_t p = c + lane;
    const bool keep = p < end && !in_sorted_list(excl, num_excl, (int64_t)eid[p]);
    cnt += __popcll(__ballot(keep));
  }
  if (lane == 0) counts[i] = cnt;
}

// the kept edges of seed i, in their order, at [new_offsets[i], new_offsets[i + 1]) -- never past it
template <typename Idx>
__global__ __launch_bounds__(kBlock) void frontier_exclude_fill_kernel(int64_t num_seeds, const int64_t* offsets, const Idx* eid,
                                                                       int64_t num_excl, const int64_t* excl, const Idx* src,
                                                                       const int64_t* new_offsets, Idx* out_src, Idx* out_eid) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t i = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (i >= num_seeds) return;
  const int64_t beg = offsets[i], end = offsets[i + 1];
  int64_t o = new_offsets[i];
  const int64_t stop = new_offsets[i + 1];
  for (int64_t c = beg; c < end; c += kWave) {
    const int64_t p = c + lane;
    Idx id = 0;
    bool keep = false;
    if (p < end) {
      id = eid[p];
      keep = !in_sorted_list(excl, num_excl, (int64_t)id);
    }
    const uint64_t mask = __ballot(keep);
    const int64_t at = o + __popcll(mask & ((1ull << lane) - 1ull));
    if (keep && at < stop) {
      out_src[at] = src[p];
      out_eid[at] = id;
    }
    o += __popcll(mask);
  }
}

// ---- compaction: the distinct ids of a list in ascending order, and where each entry of the list went --------------------------
__global__ __launch_bounds__(kBlock) void compact_mark_kernel(const int64_t* ids, int64_t n, int64_t num_nodes, unsigned long long* bits,
                                                              int64_t* flags) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const int64_t v = ids[i];
    if (!in_range(v, num_nodes)) { flag_error(flags, kErrRange); continue; }
    const unsigned long long m = 1ull << (v & 63);
    if (!(bits[v >> 6] & m)) atomicOr(&bits[v >> 6], m);  // a stale plain read only costs the atomic it was meant to save
  }
}

// lut is read only at marked nodes, and block_emit_kernel has written every one of them
template <typename Out>
__global__ __launch_bounds__(kBlock) void compact_apply_kernel(const int64_t* ids, int64_t n, int64_t num_nodes, const int32_t* lut,
                                                               Out* local) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const int64_t v = ids[i];
    local[i] = in_range(v, num_nodes) ? (Out)lut[v] : (Out)0;  // out of range: reported by the mark phase
  }
}

// workspace of mgx_to_block: lut int32[num_nodes] | bits uint64[words] | word_rank int32[words]
static inline int64_t bitmap_words(int64_t num_nodes) { return (num_nodes + 63) / 64; }
static inline int64_t lut_bytes(int64_t num_nodes) { return round_up(num_nodes * 4, 16); }

}  // namespace mgx

extern "C" int64_t mgx_to_block_workspace(int64_t num_nodes, int64_t nnz) {
  using namespace mgx;
  if (num_nodes < 0 || nnz < 0) return -1;
  const int64_t words = bitmap_words(num_nodes);
  return lut_bytes(num_nodes) + words * 8 + round_up(words * 4, 16) + 16;
}

extern "C" int32_t mgx_to_block(int64_t num_nodes, int64_t num_dst, const int64_t* dst_nodes, int64_t nnz, const int64_t* src,
                                const int64_t* dst, int32_t dst_sorted, int32_t out_bits, void* workspace, int64_t* src_nodes,
                                void* l_src, void* l_dst, void* indptr, int64_t* result, void* stream) {
  using namespace mgx;
  MGX_ENTER();
  MGX_CHECK_ARG(num_nodes >= 0 && num_dst >= 0 && nnz >= 0, "mgx_to_block: negative size");
  MGX_CHECK_ARG(out_bits == 32 || out_bits == 64, "mgx_to_block: out_bits must be 32 or 64, got %d", out_bits);
  MGX_CHECK_ARG(num_dst + nnz < (int64_t(1) << 31), "mgx_to_block: num_dst + nnz must be below 2^31");
  MGX_CHECK_ARG(result != nullptr, "mgx_to_block: result is NULL");
  MGX_CHECK_ARG(num_nodes == 0 || workspace, "mgx_to_block: workspace is NULL");
  MGX_CHECK_ARG(num_dst == 0 || (dst_nodes && src_nodes), "mgx_to_block: NULL pointer (dst_nodes, src_nodes)");
  MGX_CHECK_ARG(nnz == 0 || (src && dst && l_src && l_dst), "mgx_to_block: NULL pointer (src, dst, l_src, l_dst)");
  MGX_CHECK_ARG(nnz == 0 || num_nodes == 0 || src_nodes, "mgx_to_block: src_nodes is NULL");
  MGX_CHECK_ARG(!dst_sorted || indptr, "mgx_to_block: indptr is NULL with dst_sorted");
  hipStream_t s = (hipStream_t)stream;
  const int64_t words = bitmap_words(num_nodes);
  int32_t* lut = (int32_t*)workspace;
  unsigned long long* bits = (unsigned long long*)((char*)workspace + lut_bytes(num_nodes));
  int32_t* word_rank = (int32_t*)((char*)bits + words * 8);
  int64_t* flags = result + 1;
  MGX_CHECK_HIP(hipMemsetAsync(result, 0, 2 * sizeof(int64_t), s));
  if (num_nodes > 0) {
    MGX_CHECK_HIP(hipMemsetAsync(lut, 0xFF, (size_t)num_nodes * 4, s));
    MGX_CHECK_HIP(hipMemsetAsync(bits, 0, (size_t)words * 8, s));
  }
  if (num_dst > 0)
    hipLaunchKernelGGL(relabel_scatter_kernel, stride_grid(num_dst), dim3(kBlock), 0, s, dst_nodes, num_dst, num_nodes, lut, src_nodes,
                       flags);
  if (nnz > 0)
    hipLaunchKernelGGL(block_mark_kernel, stride_grid(nnz), dim3(kBlock), 0, s, src, dst, nnz, num_nodes, lut, bits, flags);
  hipLaunchKernelGGL(block_rank_kernel, dim3(1), dim3(kRankBlock), 0, s, bits, nnz > 0 ? words : 0, word_rank, num_dst, result);
  if (nnz > 0) {
    const int64_t capacity = num_dst + (nnz < num_nodes ? nnz : num_nodes);
    hipLaunchKernelGGL(block_emit_kernel, stride_grid(words), dim3(kBlock), 0, s, bits, words, word_rank, num_dst, capacity, lut,
                       src_nodes);
    if (out_bits == 32)
      hipLaunchKernelGGL((block_apply_kernel<int32_t>), stride_grid(nnz), dim3(kBlock), 0, s, src, dst, nnz, num_nodes, num_dst, lut,
                         (int32_t*)l_src, (int32_t*)l_dst, dst_sorted ? (int32_t*)indptr : nullptr, flags);
    else
      hipLaunchKernelGGL((block_apply_kernel<int64_t>), stride_grid(nnz), dim3(kBlock), 0, s, src, dst, nnz, num_nodes, num_dst, lut,
                         (int64_t*)l_src, (int64_t*)l_dst, dst_sorted ? (int64_t*)indptr : nullptr, flags);
  } else if (dst_sorted) {  // no edge: every row is empty
    MGX_CHECK_HIP(hipMemsetAsync(indptr, 0, (size_t)(num_dst + 1) * (out_bits / 8), s));
  }
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}

extern "C" int64_t mgx_node_subgraph_workspace(int64_t num_nodes) {
  using namespace mgx;
  if (num_nodes < 0) return -1;
  return lut_bytes(num_nodes) + 16;
}

namespace mgx {
static int32_t check_subgraph_args(const char* who, const mgx_csr* csr, int64_t num_sel, const int64_t* sel_nodes, const void* workspace) {
  MGX_CHECK_ARG(csr != nullptr, "%s: csr is NULL", who);
  MGX_CHECK_ARG(csr->idx_bits == 32 || csr->idx_bits == 64, "%s: idx_bits must be 32 or 64", who);
  MGX_CHECK_ARG(num_sel >= 0 && csr->num_rows >= 0 && csr->nnz >= 0, "%s: negative size", who);
  MGX_CHECK_ARG(csr->num_rows == csr->num_cols, "%s: the parent must have one node set (num_rows == num_cols)", who);
  MGX_CHECK_ARG(num_sel < (int64_t(1) << 31), "%s: num_sel must be below 2^31", who);
  MGX_CHECK_ARG(num_sel == 0 || (sel_nodes && csr->indptr), "%s: NULL pointer (sel_nodes, indptr)", who);
  MGX_CHECK_ARG(csr->num_rows == 0 || workspace, "%s: workspace is NULL", who);
  MGX_CHECK_ARG(csr->nnz == 0 || csr->indices, "%s: indices is NULL", who);
  return MGX_OK;
}
static inline dim3 row_wave_grid(int64_t rows) { return dim3((unsigned)((rows + kWavesPerBlock - 1) / kWavesPerBlock)); }
}  // namespace mgx

extern "C" int32_t mgx_node_subgraph_count(const mgx_csr* csr, int64_t num_sel, const int64_t* sel_nodes, void* workspace,
                                           int64_t* counts, int64_t* result, void* stream) {
  using namespace mgx;
  MGX_ENTER();
  if (int32_t st = check_subgraph_args("mgx_node_subgraph_count", csr, num_sel, sel_nodes, workspace)) return st;
  MGX_CHECK_ARG(result != nullptr, "mgx_node_subgraph_count: result is NULL");
  MGX_CHECK_ARG(num_sel == 0 || counts, "mgx_node_subgraph_count: counts is NULL");
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = csr->num_rows;
  int32_t* lut = (int32_t*)workspace;
  MGX_CHECK_HIP(hipMemsetAsync(result, 0, sizeof(int64_t), s));
  if (n > 0) MGX_CHECK_HIP(hipMemsetAsync(lut, 0xFF, (size_t)n * 4, s));
  if (num_sel == 0) return MGX_OK;
  hipLaunchKernelGGL(relabel_scatter_kernel, stride_grid(num_sel), dim3(kBlock), 0, s, sel_nodes, num_sel, n, lut, (int64_t*)nullptr,
                     result);
  if (csr->idx_bits == 32)
    hipLaunchKernelGGL((subgraph_count_kernel<int32_t>), row_wave_grid(num_sel), dim3(kBlock), 0, s, (const int32_t*)csr->indptr,
                       (const int32_t*)csr->indices, (const int32_t*)csr->eids, n, sel_nodes, num_sel, lut, counts, result);
  else
    hipLaunchKernelGGL((subgraph_count_kernel<int64_t>), row_wave_grid(num_sel), dim3(kBlock), 0, s, (const int64_t*)csr->indptr,
                       (const int64_t*)csr->indices, (const int64_t*)csr->eids, n, sel_nodes, num_sel, lut, counts, result);
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}

namespace mgx {
template <typename Idx>
static void launch_subgraph_fill(const mgx_csr* csr, int64_t num_sel, const int64_t* sel, const int32_t* lut, const int64_t* offsets,
                                 int32_t out_bits, void* l_src, void* l_dst, int64_t* parent_eid, hipStream_t s) {
  const Idx* indptr = (const Idx*)csr->indptr;
  const Idx* indices = (const Idx*)csr->indices;
  const Idx* eids = (const Idx*)csr->eids;
  if (out_bits == 32)
    hipLaunchKernelGGL((subgraph_fill_kernel<Idx, int32_t>), row_wave_grid(num_sel), dim3(kBlock), 0, s, indptr, indices, eids,
                       csr->num_rows, sel, num_sel, lut, offsets, (int32_t*)l_src, (int32_t*)l_dst, parent_eid);
  else
    hipLaunchKernelGGL((subgraph_fill_kernel<Idx, int64_t>), row_wave_grid(num_sel), dim3(kBlock), 0, s, indptr, indices, eids,
                       csr->num_rows, sel, num_sel, lut, offsets, (int64_t*)l_src, (int64_t*)l_dst, parent_eid);
}
}  // namespace mgx

extern "C" int32_t mgx_node_subgraph_fill(const mgx_csr* csr, int64_t num_sel, const int64_t* sel_nodes, const void* workspace,
                                          const int64_t* offsets, int32_t out_bits, void* l_src, void* l_dst, int64_t* parent_eid,
                                          void* stream) {
  using namespace mgx;
  MGX_ENTER();
  if (int32_t st = check_subgraph_args("mgx_node_subgraph_fill", csr, num_sel, sel_nodes, workspace)) return st;
  MGX_CHECK_ARG(out_bits == 32 || out_bits == 64, "mgx_node_subgraph_fill: out_bits must be 32 or 64, got %d", out_bits);
  if (num_sel == 0 || csr->nnz == 0) return MGX_OK;
  MGX_CHECK_ARG(offsets && l_src && l_dst && parent_eid, "mgx_node_subgraph_fill: NULL pointer (offsets, l_src, l_dst, parent_eid)");
  hipStream_t s = (hipStream_t)stream;
  if (csr->idx_bits == 32)
    launch_subgraph_fill<int32_t>(csr, num_sel, sel_nodes, (const int32_t*)workspace, offsets, out_bits, l_src, l_dst, parent_eid, s);
  else
    launch_subgraph_fill<int64_t>(csr, num_sel, sel_nodes, (const int32_t*)workspace, offsets, out_bits, l_src, l_dst, parent_eid, s);
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}

namespace mgx {
static int32_t check_frontier_args(const char* who, int64_t num_seeds, const int64_t* offsets, const void* eid, int32_t idx_bits,
                                   int64_t num_excl, const int64_t* excl_sorted) {
  MGX_CHECK_ARG(num_seeds >= 0 && num_excl >= 0, "%s: negative size", who);
  MGX_CHECK_ARG(idx_bits == 32 || idx_bits == 64, "%s: idx_bits must be 32 or 64, got %d", who, idx_bits);
  MGX_CHECK_ARG(num_seeds < (int64_t(1) << 31), "%s: num_seeds must be below 2^31", who);
  MGX_CHECK_ARG(num_seeds == 0 || (offsets && eid), "%s: NULL pointer (offsets, eid)", who);
  MGX_CHECK_ARG(num_excl == 0 || excl_sorted, "%s: excl_sorted is NULL", who);
  return MGX_OK;
}
}  // namespace mgx

extern "C" int32_t mgx_frontier_exclude_count(int64_t num_seeds, const int64_t* offsets, const void* eid, int32_t idx_bits,
                                              int64_t num_excl, const int64_t* excl_sorted, int64_t* counts, void* stream) {
  using namespace mgx;
  MGX_ENTER();
  if (int32_t st = check_frontier_args("mgx_frontier_exclude_count", num_seeds, offsets, eid, idx_bits, num_excl, excl_sorted)) return st;
  MGX_CHECK_ARG(num_seeds == 0 || counts, "mgx_frontier_exclude_count: counts is NULL");
  if (num_seeds == 0) return MGX_OK;
  hipStream_t s = (hipStream_t)stream;
  if (idx_bits == 32)
    hipLaunchKernelGGL((frontier_exclude_count_kernel<int32_t>), row_wave_grid(num_seeds), dim3(kBlock), 0, s, num_seeds, offsets,
                       (const int32_t*)eid, num_excl, excl_sorted, counts);
  else
    hipLaunchKernelGGL((frontier_exclude_count_kernel<int64_t>), row_wave_grid(num_seeds), dim3(kBlock), 0, s, num_seeds, offsets,
                       (const int64_t*)eid, num_excl, excl_sorted, counts);
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}

extern "C" int32_t mgx_frontier_exclude_fill(int64_t num_seeds, const int64_t* offsets, const void* eid, int32_t idx_bits,
                                             int64_t num_excl, const int64_t* excl_sorted, const void* src, const int64_t* new_offsets,
                                             void* out_src, void* out_eid, void* stream) {
  using namespace mgx;
  MGX_ENTER();
  if (int32_t st = check_frontier_args("mgx_frontier_exclude_fill", num_seeds, offsets, eid, idx_bits, num_excl, excl_sorted)) return st;
  MGX_CHECK_ARG(num_seeds == 0 || (src && new_offsets && out_src && out_eid),
                "mgx_frontier_exclude_fill: NULL pointer (src, new_offsets, out_src, out_eid)");
  if (num_seeds == 0) return MGX_OK;
  hipStream_t s = (hipStream_t)stream;
  if (idx_bits == 32)
    hipLaunchKernelGGL((frontier_exclude_fill_kernel<int32_t>), row_wave_grid(num_seeds), dim3(kBlock), 0, s, num_seeds, offsets,
                       (const int32_t*)eid, num_excl, excl_sorted, (const int32_t*)src, new_offsets, (int32_t*)out_src,
                       (int32_t*)out_eid);
  else
    hipLaunchKernelGGL((frontier_exclude_fill_kernel<int64_t>), row_wave_grid(num_seeds), dim3(kBlock), 0, s, num_seeds, offsets,
                       (const int64_t*)eid, num_excl, excl_sorted, (const int64_t*)src, new_offsets, (int64_t*)out_src,
                       (int64_t*)out_eid);
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}

extern "C" int64_t mgx_compact_nodes_workspace(int64_t num_nodes, int64_t n) { return mgx_to_block_workspace(num_nodes, n); }

extern "C" int32_t mgx_compact_nodes(int64_t num_nodes, int64_t n, const int64_t* ids, int32_t out_bits, void* workspace, int64_t* nodes,
                                     void* local, int64_t* result, void* stream) {
  using namespace mgx;
  MGX_ENTER();
  MGX_CHECK_ARG(num_nodes >= 0 && n >= 0, "mgx_compact_nodes: negative size");
  MGX_CHECK_ARG(out_bits == 32 || out_bits == 64, "mgx_compact_nodes: out_bits must be 32 or 64, got %d", out_bits);
  MGX_CHECK_ARG(n < (int64_t(1) << 31), "mgx_compact_nodes: n must be below 2^31");
  MGX_CHECK_ARG(result != nullptr, "mgx_compact_nodes: result is NULL");
  MGX_CHECK_ARG(num_nodes == 0 || workspace, "mgx_compact_nodes: workspace is NULL");
  MGX_CHECK_ARG(n == 0 || (ids && local), "mgx_compact_nodes: NULL pointer (ids, local)");
  MGX_CHECK_ARG(n == 0 || num_nodes == 0 || nodes, "mgx_compact_nodes: nodes is NULL");
  hipStream_t s = (hipStream_t)stream;
  const int64_t words = bitmap_words(num_nodes);
  int32_t* lut = (int32_t*)workspace;
  unsigned long long* bits = (unsigned long long*)((char*)workspace + lut_bytes(num_nodes));
  int32_t* word_rank = (int32_t*)((char*)bits + words * 8);
  int64_t* flags = result + 1;
  MGX_CHECK_HIP(hipMemsetAsync(result, 0, 2 * sizeof(int64_t), s));
  if (n == 0) return MGX_OK;
  if (words > 0) MGX_CHECK_HIP(hipMemsetAsync(bits, 0, (size_t)words * 8, s));
  hipLaunchKernelGGL(compact_mark_kernel, stride_grid(n), dim3(kBlock), 0, s, ids, n, num_nodes, bits, flags);
  hipLaunchKernelGGL(block_rank_kernel, dim3(1), dim3(kRankBlock), 0, s, bits, words, word_rank, (int64_t)0, result);
  if (words > 0)
    hipLaunchKernelGGL(block_emit_kernel, stride_grid(words), dim3(kBlock), 0, s, bits, words, word_rank, (int64_t)0,
                       n < num_nodes ? n : num_nodes, lut, nodes);
  if (out_bits == 32)
    hipLaunchKernelGGL((compact_apply_kernel<int32_t>), stride_grid(n), dim3(kBlock), 0, s, ids, n, num_nodes, lut, (int32_t*)local);
  else
    hipLaunchKernelGGL((compact_apply_kernel<int64_t>), stride_grid(n), dim3(kBlock), 0, s, ids, n, num_nodes, lut, (int64_t*)local);
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}
