// edgefind.hip -- edge lookup and negative sampling on the device: the integer work that turns a batch of EDGES into a link-prediction
// training step (dgl.dataloading.EdgeDataLoader, dgl.dataloading.negative_sampler.Uniform, g.edge_ids / g.has_edges_between).
//
//   mgx_edge_lookup      (row, col) -> the lowest edge id of that pair, -1 without one.  A group of 16 lanes per query scans the row
//                        (edge_find.h says why a scan); replaces a sort of one key per edge of the WHOLE graph on every call.
//   mgx_negative_sample  k uniform destinations per positive edge, proposals that are edges of the graph (exclude_existing) or self
//                        loops rejected and redrawn -- at most max_tries times: a node adjacent to everything ends with -1 in its slots
//                        and a count in `result`, never with a loop that does not end.  A group of 16 lanes per draw; the existence
//                        check is the scan of mgx_edge_lookup.  Every proposal is a function of (rng_seed, draw, try) alone
//                        (counter_rng.h holds the formula), so the in-CSR form, the out-CSR form, both index widths and the host
//                        restatement agree bit for bit.
//
// Every id read from a caller's array is checked before it indexes anything; a bad id sets error bit 4 and its slot gets -1.  The only
// atomics are the OR of the error bits and the count of failed draws (an integer sum: the same on every run).
#include "common.h"
#include "counter_rng.h"
#include "edge_find.h"

namespace mgx {

enum { kFindErrRange = 4 };
enum { kNegExcludeExisting = 1, kNegExcludeSelfLoops = 2 };

__device__ __forceinline__ bool id_in_range(int64_t v, int64_t n) { return (uint64_t)v < (uint64_t)n; }

static inline dim3 find_grid(int64_t groups) { return dim3((unsigned)((groups + kFindPerBlock - 1) / kFindPerBlock)); }

template <typename Idx>
__global__ __launch_bounds__(kBlock) void edge_lookup_kernel(const Idx* indptr, const Idx* indices, const Idx* eids, int64_t num_rows,
                                                             int64_t num_cols, int64_t num_q, const int64_t* row_ids,
                                                             const int64_t* col_ids, int64_t* out_eid, int64_t* flags) {
  const int sub = threadIdx.x & (kFindLanes - 1);
  const int64_t q = (int64_t)blockIdx.x * kFindPerBlock + (threadIdx.x / kFindLanes);
  const bool live = q < num_q;  // no early return: the shuffles of group_find_edge want whole groups, and waves stay converged
  int64_t beg = 0, end = 0, col = 0;
  bool ok = false;
  if (live) {
    const int64_t row = row_ids[q];
    col = col_ids[q];
    ok = id_in_range(row, num_rows) && id_in_range(col, num_cols);
    if (ok) {
      beg = (int64_t)indptr[row];
      end = (int64_t)indptr[row + 1];
    }
  }
  const int64_t found = group_find_edge(indices, eids, beg, end, col, sub);
  if (live && sub == 0) {
    out_eid[q] = (ok && found != kNoEdge) ? found : -1;
    if (!ok) atomicOr((unsigned long long*)flags, (unsigned long long)kFindErrRange);
  }
}

// `indptr` NULL: no existence check (exclude_existing off).  rows_are_sources: the CSR is the out-CSR and the row scanned is the
// positive edge's source -- the same row for all k * max_tries checks of that edge -- else the in-CSR, scanned at the proposal.
template <typename Idx>
__global__ __launch_bounds__(kBlock) void negative_sample_kernel(const Idx* indptr, const Idx* indices, int64_t num_src_nodes,
                                                                 int rows_are_sources, int64_t num_pos, const int64_t* pos_src, int k,
                                                                 int64_t num_dst_nodes, int flags, int max_tries, uint64_t rng_seed,
                                                                 int64_t* out_dst, int64_t* result) {
  const int sub = threadIdx.x & (kFindLanes - 1);
  const int64_t d = (int64_t)blockIdx.x * kFindPerBlock + (threadIdx.x / kFindLanes);  // draw (e, j) = e * k + j
  const bool live = d < num_pos * k;
  int64_t u = 0;
  bool bad = false;
  if (live) {
    u = pos_src[d / k];
    bad = indptr != nullptr && !id_in_range(u, num_src_nodes);  // without a CSR u indexes nothing: it is only compared
  }
  bool open = live && !bad;
  int64_t pick = -1;
  for (int t = 0; t < max_tries; ++t) {  // bounded: max_tries <= kNegMaxTries, checked by the entry point
    if (__ballot(open) == 0) break;      // wave-uniform
    const int64_t cand = negative_candidate(rng_seed, d, t, num_dst_nodes);
    const bool rejected = (flags & kNegExcludeSelfLoops) && cand == u;
    int64_t beg = 0, end = 0;
    const int64_t col = rows_are_sources ? cand : u;
    if (open && !rejected && indptr) {
      const int64_t row = rows_are_sources ? u : cand;  // cand < num_dst_nodes <= the CSR's node count (entry point)
      beg = (int64_t)indptr[row];
      end = (int64_t)indptr[row + 1];
    }
    const int64_t found = group_find_edge(indices, (const Idx*)nullptr, beg, end, col, sub);
    if (open && !rejected && found == kNoEdge) {
      pick = cand;
      open = false;
    }
  }
  if (live && sub == 0) {
    out_dst[d] = pick;
    if (bad) atomicOr((unsigned long long*)(result + 1), (unsigned long long)kFindErrRange);
    else if (pick < 0) atomicAdd((unsigned long long*)result, 1ull);
  }
}

static int32_t check_find_csr(const char* who, const mgx_csr* csr) {
  MGX_CHECK_ARG(csr->idx_bits == 32 || csr->idx_bits == 64, "%s: idx_bits must be 32 or 64", who);
  MGX_CHECK_ARG(csr->num_rows >= 0 && csr->num_cols >= 0 && csr->nnz >= 0, "%s: negative size", who);
  MGX_CHECK_ARG(csr->indptr != nullptr, "%s: indptr is NULL", who);
  MGX_CHECK_ARG(csr->nnz == 0 || csr->indices, "%s: indices is NULL", who);
  return MGX_OK;
}

}  // namespace mgx

extern "C" int32_t mgx_edge_lookup(const mgx_csr* csr, int64_t num_q, const int64_t* row_ids, const int64_t* col_ids, int64_t* out_eid,
                                   int64_t* result, void* stream) {
  using namespace mgx;
  MGX_ENTER();
  MGX_CHECK_ARG(csr != nullptr, "mgx_edge_lookup: csr is NULL");
  MGX_CHECK_ARG(num_q >= 0, "mgx_edge_lookup: negative num_q");
  MGX_CHECK_ARG(num_q < (int64_t(1) << 34), "mgx_edge_lookup: num_q must be below 2^34");
  if (int32_t st = check_find_csr("mgx_edge_lookup", csr)) return st;
  MGX_CHECK_ARG(result != nullptr, "mgx_edge_lookup: result is NULL");
  MGX_CHECK_ARG(num_q == 0 || (row_ids && col_ids && out_eid), "mgx_edge_lookup: NULL pointer (row_ids, col_ids, out_eid)");
  hipStream_t s = (hipStream_t)stream;
  MGX_CHECK_HIP(hipMemsetAsync(result, 0, sizeof(int64_t), s));
  if (num_q == 0) return MGX_OK;
  if (csr->idx_bits == 32)
    hipLaunchKernelGGL((edge_lookup_kernel<int32_t>), find_grid(num_q), dim3(kBlock), 0, s, (const int32_t*)csr->indptr,
                       (const int32_t*)csr->indices, (const int32_t*)csr->eids, csr->num_rows, csr->num_cols, num_q, row_ids, col_ids,
                       out_eid, result);
  else
    hipLaunchKernelGGL((edge_lookup_kernel<int64_t>), find_grid(num_q), dim3(kBlock), 0, s, (const int64_t*)csr->indptr,
                       (const int64_t*)csr->indices, (const int64_t*)csr->eids, csr->num_rows, csr->num_cols, num_q, row_ids, col_ids,
                       out_eid, result);
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}

extern "C" int32_t mgx_negative_sample(const mgx_csr* csr, int32_t rows_are_sources, int64_t num_pos, const int64_t* pos_src, int32_t k,
                                       int64_t num_dst_nodes, int32_t flags, int32_t max_tries, uint64_t rng_seed, int64_t* out_dst,
                                       int64_t* result, void* stream) {
  using namespace mgx;
  MGX_ENTER();
  MGX_CHECK_ARG(num_pos >= 0 && num_dst_nodes >= 0, "mgx_negative_sample: negative size");
  MGX_CHECK_ARG(k >= 1, "mgx_negative_sample: k must be at least 1, got %d", k);
  MGX_CHECK_ARG(max_tries >= 1 && max_tries <= kNegMaxTries, "mgx_negative_sample: max_tries must be in [1, %d], got %d", kNegMaxTries,
                max_tries);
  MGX_CHECK_ARG((flags & ~(kNegExcludeExisting | kNegExcludeSelfLoops)) == 0, "mgx_negative_sample: unknown flag bits in %d", flags);
  MGX_CHECK_ARG(num_dst_nodes < (int64_t(1) << 31), "mgx_negative_sample: num_dst_nodes must be below 2^31");
  MGX_CHECK_ARG(num_pos < (int64_t(1) << 34) / k, "mgx_negative_sample: num_pos * k must be below 2^34");
  const bool existing = (flags & kNegExcludeExisting) != 0;
  MGX_CHECK_ARG(!existing || csr != nullptr, "mgx_negative_sample: csr is NULL with exclude_existing");
  MGX_CHECK_ARG(existing || csr == nullptr, "mgx_negative_sample: csr must be NULL without exclude_existing");
  int64_t num_src_nodes = 0;
  if (csr) {
    if (int32_t st = check_find_csr("mgx_negative_sample", csr)) return st;
    num_src_nodes = rows_are_sources ? csr->num_rows : csr->num_cols;
    MGX_CHECK_ARG(num_dst_nodes <= (rows_are_sources ? csr->num_cols : csr->num_rows),
                  "mgx_negative_sample: num_dst_nodes exceeds the graph's destination nodes");
  }
  MGX_CHECK_ARG(result != nullptr, "mgx_negative_sample: result is NULL");
  MGX_CHECK_ARG(num_pos == 0 || (pos_src && out_dst), "mgx_negative_sample: NULL pointer (pos_src, out_dst)");
  MGX_CHECK_ARG(num_pos == 0 || num_dst_nodes >= 1, "mgx_negative_sample: no destination node to draw from");
  hipStream_t s = (hipStream_t)stream;
  MGX_CHECK_HIP(hipMemsetAsync(result, 0, 2 * sizeof(int64_t), s));
  if (num_pos == 0) return MGX_OK;
  const dim3 grid = find_grid(num_pos * k);
  if (csr && csr->idx_bits == 32)
    hipLaunchKernelGGL((negative_sample_kernel<int32_t>), grid, dim3(kBlock), 0, s, (const int32_t*)csr->indptr,
                       (const int32_t*)csr->indices, num_src_nodes, rows_are_sources, num_pos, pos_src, k, num_dst_nodes, flags,
                       max_tries, rng_seed, out_dst, result);
  else
    hipLaunchKernelGGL((negative_sample_kernel<int64_t>), grid, dim3(kBlock), 0, s, csr ? (const int64_t*)csr->indptr : nullptr,
                       csr ? (const int64_t*)csr->indices : nullptr, num_src_nodes, rows_are_sources, num_pos, pos_src, k,
                       num_dst_nodes, flags, max_tries, rng_seed, out_dst, result);
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}
