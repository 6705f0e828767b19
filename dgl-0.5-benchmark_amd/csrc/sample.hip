// sample.hip -- uniform neighbor sampling without replacement on the device.
//
// Replaces what dgl.dataloading.MultiLayerNeighborSampler / dgl.sampling.sample_neighbors do in CPU worker
// processes for end_to_end/sampling/node-classification/reddit/ns-sage-dgl.py:132-141: for every seed
// (destination node) keep all in-edges when in-degree <= fanout, else draw `fanout` distinct in-edges
// uniformly.  One thread per seed runs Floyd's subset-sampling algorithm over CSR positions with a
// counter-based generator (no state, reproducible for a given rng_seed), sorts the <= 64 picks so the
// block keeps CSR order, and writes source ids and edge ids at the caller-computed offsets.  Integer work,
// no atomics; the caller sizes the outputs from min(in_degree, fanout).
//
// The other modes of dgl.sampling.sample_neighbors (ogbn-product/ns-gat/ns-gat-dgl.py:22-42 samples with replace=True) and
// dgl.sampling.select_topk give a WAVE to every seed (the kernels after sample_neighbors_kernel):
//   weighted, without replacement   Efraimidis-Spirakis keys -log(u) / w; the wave keeps the `fanout` smallest (key, position) pairs,
//                                   one per lane, sorted, and merges the row into them 64 edges at a time (bitonic sort + merge)
//   select_topk                     the same selection with key = -weight (or +weight, ascending)
//   with replacement                lane j < fanout owns draw j: floor(r * deg) when uniform, else the inverse CDF over the row --
//                                   a running sum in row order, fp32 inside a chunk of 64 and fp64 across chunks
// Every random number is a function of (rng_seed, seed slot, draw or CSR position), never of the launch geometry.
#include "common.h"
#include "counter_rng.h"  // mix64
#include "wave_select.h"

namespace mgx {

constexpr int kMaxFanout = 64;

template <typename Idx>
__global__ __launch_bounds__(kBlock) void sample_neighbors_kernel(const Idx* indptr, const Idx* indices, const Idx* eids,
                                                                  const Idx* seeds, int64_t num_seeds, int fanout,
                                                                  uint64_t rng_seed, const int64_t* out_offsets,
                                                                  Idx* out_src, Idx* out_eid) {
  const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (s >= num_seeds) return;
  const int64_t v = (int64_t)seeds[s];
  const int64_t beg = (int64_t)indptr[v];
  const int64_t deg = (int64_t)indptr[v + 1] - beg;
  int64_t o = out_offsets[s];
  if (deg <= fanout) {
    for (int64_t p = beg; p < beg + deg; ++p, ++o) {
      out_src[o] = indices[p];
      out_eid[o] = eids ? eids[p] : (Idx)p;
    }
    return;
  }
  int64_t pick[kMaxFanout];
  int n = 0;
  for (int64_t j = deg - fanout; j < deg; ++j) {  // Floyd: a uniform `fanout`-subset of [0, deg)
    const uint64_t r = mix64(rng_seed ^ mix64((uint64_t)s * 0x100000001B3ull + (uint64_t)(j - (deg - fanout))));
    int64_t t = (int64_t)(((unsigned __int128)r * (uint64_t)(j + 1)) >> 64);  // uniform in [0, j]
    bool seen = false;
    for (int i = 0; i < n; ++i) seen |= pick[i] == t;
    if (seen) t = j;
    int i = n++;  // insertion keeps the picks ascending (CSR order)
    while (i > 0 && pick[i - 1] > t) { pick[i] = pick[i - 1]; --i; }
    pick[i] = t;
  }
  for (int i = 0; i < n; ++i, ++o) {
    const int64_t p = beg + pick[i];
    out_src[o] = indices[p];
    out_eid[o] = eids ? eids[p] : (Idx)p;
  }
}


// ---- one wave per seed: weighted / with-replacement sampling, top-k ----------------------------------------------------------
// (key, position) pairs, kNoPair, wave_sort and wave_bitonic_merge: wave_select.h, shared with segtopk.hip.

// Inclusive scan of w over the lanes IN LANE ORDER, fl(fl(w0 + w1) + w2) ...: a lane of weight 0 repeats its predecessor's sum bit for
// bit and the sums never decrease, which a tree-shaped scan does not promise under rounding -- the inverse CDF below depends on both
// ("first position whose running sum exceeds t" must not be a zero-weight edge).  `total` = the sum at lane 63, wave-uniform.
__device__ __forceinline__ float wave_scan_in_order(float w, int lane, float& total) {
  float acc = 0.f, incl = 0.f;
#pragma unroll
  for (int i = 0; i < kWave; ++i) {
    acc += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w), i));
    incl = lane == i ? acc : incl;
  }
  total = acc;
  return incl;
}

__device__ __forceinline__ bool weight_invalid(float w) { return !(w >= 0.f) || w == INFINITY; }  // negative, NaN, infinite

// picks (row-relative positions, kNoPair in the lanes without one) -> sorted by position and written at the seed's offsets; never
// past the room the caller left for this seed
template <typename Idx>
__device__ __forceinline__ void write_picks(uint64_t pick, int lane, int64_t beg, const Idx* indices, const Idx* eids, int64_t o,
                                            int64_t room, Idx* out_src, Idx* out_eid) {
  const int n = __popcll(__ballot(pick != kNoPair));
  pick = wave_sort(pick, lane);
  if (lane < n && lane < room) {
    const int64_t p = beg + (int64_t)pick;
    out_src[o + lane] = indices[p];
    out_eid[o + lane] = eids ? eids[p] : (Idx)p;
  }
}

template <typename Idx>
__global__ __launch_bounds__(kBlock) void sample_count_positive_kernel(const Idx* indptr, const Idx* eids, const Idx* seeds,
                                                                       int64_t num_seeds, const float* prob, int64_t* out_counts,
                                                                       int32_t* out_invalid) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t s = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (s >= num_seeds) return;
  const int64_t v = (int64_t)seeds[s];
  const int64_t beg = (int64_t)indptr[v], end = (int64_t)indptr[v + 1];
  int64_t cnt = 0;
  bool bad = false;
  for (int64_t c = beg; c < end; c += kWave) {
    const int64_t p = c + lane;
    float w = 0.f;
    if (p < end) w = prob[eids ? (int64_t)eids[p] : p];
    cnt += __popcll(__ballot(w > 0.f));
    bad |= weight_invalid(w);
  }
  const bool any_bad = __ballot(bad) != 0;
  if (lane == 0) {
    out_counts[s] = cnt;
    if (any_bad) *out_invalid = 1;  // every writer stores the same value
  }
}

// Weighted sampling without replacement (kTopk = false: candidates are the edges of weight > 0, key = -log(u) / w) and select_topk
// (kTopk = true: every edge, key = -weight or +weight).  Lane i holds the i-th smallest pair seen so far.
template <typename Idx, bool kTopk>
__global__ __launch_bounds__(kBlock) void select_smallest_kernel(const Idx* indptr, const Idx* indices, const Idx* eids,
                                                                 const Idx* seeds, int64_t num_seeds, int k, const float* weight,
                                                                 int ascending, uint64_t rng_seed, const int64_t* out_offsets,
                                                                 Idx* out_src, Idx* out_eid) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t s = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (s >= num_seeds) return;
  const int64_t o = out_offsets[s], room = out_offsets[s + 1] - o;
  if (room <= 0) return;
  const int64_t v = (int64_t)seeds[s];
  const int64_t beg = (int64_t)indptr[v], end = (int64_t)indptr[v + 1];
  uint64_t best = kNoPair;
  for (int64_t c = beg; c < end; c += kWave) {
    const int64_t p = c + lane;
    uint64_t cand = kNoPair;
    if (p < end) {
      const float w = weight[eids ? (int64_t)eids[p] : p];
      if (kTopk) {
        cand = pack_pair((ascending ? w : -w) + 0.f, (uint64_t)(p - beg));  // + 0: -0 and +0 are one key
      } else if (w > 0.f) {
        const uint64_t r = mix64(rng_seed ^ mix64((uint64_t)s * 0x100000001B3ull ^ mix64((uint64_t)p)));
        const double u = ((double)(r >> 12) + 0.5) * 0x1p-52;  // strictly inside (0, 1)
        cand = pack_pair((float)(-log(u) / (double)w), (uint64_t)(p - beg));
      }
    }
    const uint64_t kth = __shfl(best, k - 1, kWave);
    if (__ballot(cand < kth) == 0) continue;  // nothing in this chunk beats the current k-th
    cand = wave_sort(cand, lane);
    const uint64_t rev = __shfl(cand, kWave - 1 - lane, kWave);
    best = wave_bitonic_merge(rev < best ? rev : best, lane);  // the 64 smallest of both, as a bitonic sequence, sorted
  }
  const uint64_t pick = (lane < k && best != kNoPair) ? (best & 0xFFFFFFFFull) : kNoPair;
  write_picks(pick, lane, beg, indices, eids, o, room, out_src, out_eid);
}

// Sampling with replacement: `fanout` independent draws per seed, lane j owns draw j.
template <typename Idx, bool kWeighted>
__global__ __launch_bounds__(kBlock) void sample_replace_kernel(const Idx* indptr, const Idx* indices, const Idx* eids,
                                                                const Idx* seeds, int64_t num_seeds, int fanout, const float* prob,
                                                                uint64_t rng_seed, const int64_t* out_offsets, Idx* out_src,
                                                                Idx* out_eid) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t s = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (s >= num_seeds) return;
  const int64_t o = out_offsets[s], room = out_offsets[s + 1] - o;
  if (room <= 0) return;
  const int64_t v = (int64_t)seeds[s];
  const int64_t beg = (int64_t)indptr[v], end = (int64_t)indptr[v + 1];
  if (end <= beg) return;
  const uint64_t r = mix64(rng_seed ^ mix64((uint64_t)s * 0x100000001B3ull + (uint64_t)lane));
  uint64_t pick = kNoPair;
  if (!kWeighted) {
    if (lane < fanout) pick = (uint64_t)(((unsigned __int128)r * (uint64_t)(end - beg)) >> 64);  // floor(r * deg), r in [0, 1)
  } else {
    // sweep 1: the row total W -- the same sums in the same order as sweep 2, so that sweep 2 ends on W exactly
    double W = 0.0;
    int64_t last = -1;  // last position of weight > 0: where a target that rounding pushed to >= W lands
    for (int64_t c = beg; c < end; c += kWave) {
      const int64_t p = c + lane;
      float w = 0.f, tot;
      if (p < end) w = prob[eids ? (int64_t)eids[p] : p];
      if (weight_invalid(w)) w = 0.f;  // the caller raises on these (mgx_sample_count_positive); here they only must not be picked
      wave_scan_in_order(w, lane, tot);
      W += (double)tot;
      const uint64_t pos_mask = __ballot(w > 0.f);
      if (pos_mask) last = (c - beg) + (kWave - 1 - __clzll(pos_mask));
    }
    if (last < 0) return;
    const double t = (double)(r >> 11) * 0x1p-53 * W;
    bool open = lane < fanout;
    double base = 0.0;
    for (int64_t c = beg; c < end && __ballot(open) != 0; c += kWave) {
      const int64_t p = c + lane;
      float w = 0.f, tot;
      if (p < end) w = prob[eids ? (int64_t)eids[p] : p];
      if (weight_invalid(w)) w = 0.f;
      const float incl = wave_scan_in_order(w, lane, tot);
      const double chunk_end = base + (double)tot;
      int lo = 0, hi = kWave - 1;  // first lane whose running sum exceeds t: the sums do not decrease along the lanes
#pragma unroll
      for (int it = 0; it < 6; ++it) {
        const int mid = (lo + hi) >> 1;
        const bool above = base + (double)__shfl(incl, mid, kWave) > t;
        hi = above ? mid : hi;
        lo = above ? lo : mid + 1;
      }
      if (open && chunk_end > t) {
        const int64_t q = (c - beg) + (lo < kWave ? lo : kWave - 1);
        pick = (uint64_t)(q < last ? q : last);
        open = false;
      }
      base = chunk_end;
    }
    if (open) pick = (uint64_t)last;
  }
  write_picks(pick, lane, beg, indices, eids, o, room, out_src, out_eid);
}

}  // namespace mgx

extern "C" int32_t mgx_sample_neighbors(const mgx_csr* csr, int64_t num_seeds, const void* seeds, int32_t fanout,
                                        uint64_t rng_seed, const int64_t* out_offsets, void* out_src, void* out_eid,
                                        void* stream) {
  using namespace mgx;
  MGX_ENTER();
  MGX_CHECK_ARG(csr != nullptr, "mgx_sample_neighbors: csr is NULL");
  MGX_CHECK_ARG(csr->idx_bits == 32 || csr->idx_bits == 64, "mgx_sample_neighbors: idx_bits must be 32 or 64");
  MGX_CHECK_ARG(num_seeds >= 0, "mgx_sample_neighbors: negative num_seeds");
  MGX_CHECK_ARG(fanout >= 1 && fanout <= kMaxFanout, "mgx_sample_neighbors: fanout must be in [1, %d], got %d", kMaxFanout, fanout);
  if (num_seeds == 0) return MGX_OK;
  MGX_CHECK_ARG(csr->indptr && seeds && out_offsets, "mgx_sample_neighbors: NULL pointer");
  MGX_CHECK_ARG(csr->nnz == 0 || (csr->indices && out_src && out_eid), "mgx_sample_neighbors: NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  dim3 grid((unsigned)((num_seeds + kBlock - 1) / kBlock));
  if (csr->idx_bits == 32)
    hipLaunchKernelGGL((sample_neighbors_kernel<int32_t>), grid, dim3(kBlock), 0, s, (const int32_t*)csr->indptr,
                       (const int32_t*)csr->indices, (const int32_t*)csr->eids, (const int32_t*)seeds, num_seeds, fanout,
                       rng_seed, out_offsets, (int32_t*)out_src, (int32_t*)out_eid);
  else
    hipLaunchKernelGGL((sample_neighbors_kernel<int64_t>), grid, dim3(kBlock), 0, s, (const int64_t*)csr->indptr,
                       (const int64_t*)csr->indices, (const int64_t*)csr->eids, (const int64_t*)seeds, num_seeds, fanout,
                       rng_seed, out_offsets, (int64_t*)out_src, (int64_t*)out_eid);
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}

namespace mgx {
// one wave per seed
static inline dim3 seed_wave_grid(int64_t num_seeds) { return dim3((unsigned)((num_seeds + kWavesPerBlock - 1) / kWavesPerBlock)); }
}  // namespace mgx

extern "C" int32_t mgx_sample_count_positive(const mgx_csr* csr, int64_t num_seeds, const void* seeds, const float* prob,
                                             int64_t* out_counts, int32_t* out_invalid, void* stream) {
  using namespace mgx;
  MGX_ENTER();
  MGX_CHECK_ARG(csr != nullptr, "mgx_sample_count_positive: csr is NULL");
  MGX_CHECK_ARG(csr->idx_bits == 32 || csr->idx_bits == 64, "mgx_sample_count_positive: idx_bits must be 32 or 64");
  MGX_CHECK_ARG(num_seeds >= 0, "mgx_sample_count_positive: negative num_seeds");
  if (num_seeds == 0) return MGX_OK;
  MGX_CHECK_ARG(csr->indptr && seeds && out_counts && out_invalid, "mgx_sample_count_positive: NULL pointer");
  MGX_CHECK_ARG(csr->nnz == 0 || prob, "mgx_sample_count_positive: prob is NULL");
  hipStream_t s = (hipStream_t)stream;
  if (csr->idx_bits == 32)
    hipLaunchKernelGGL((sample_count_positive_kernel<int32_t>), seed_wave_grid(num_seeds), dim3(kBlock), 0, s,
                       (const int32_t*)csr->indptr, (const int32_t*)csr->eids, (const int32_t*)seeds, num_seeds, prob, out_counts,
                       out_invalid);
  else
    hipLaunchKernelGGL((sample_count_positive_kernel<int64_t>), seed_wave_grid(num_seeds), dim3(kBlock), 0, s,
                       (const int64_t*)csr->indptr, (const int64_t*)csr->eids, (const int64_t*)seeds, num_seeds, prob, out_counts,
                       out_invalid);
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}

namespace mgx {
template <typename Idx>
static void launch_sample_weighted(const mgx_csr* csr, int64_t num_seeds, const void* seeds, int fanout, const float* prob, bool replace,
                                   uint64_t rng_seed, const int64_t* out_offsets, void* out_src, void* out_eid, hipStream_t s) {
  const Idx* indptr = (const Idx*)csr->indptr;
  const Idx* indices = (const Idx*)csr->indices;
  const Idx* eids = (const Idx*)csr->eids;
  const dim3 grid = seed_wave_grid(num_seeds);
  if (!replace)
    hipLaunchKernelGGL((select_smallest_kernel<Idx, false>), grid, dim3(kBlock), 0, s, indptr, indices, eids, (const Idx*)seeds,
                       num_seeds, fanout, prob, 1, rng_seed, out_offsets, (Idx*)out_src, (Idx*)out_eid);
  else if (prob)
    hipLaunchKernelGGL((sample_replace_kernel<Idx, true>), grid, dim3(kBlock), 0, s, indptr, indices, eids, (const Idx*)seeds,
                       num_seeds, fanout, prob, rng_seed, out_offsets, (Idx*)out_src, (Idx*)out_eid);
  else
    hipLaunchKernelGGL((sample_replace_kernel<Idx, false>), grid, dim3(kBlock), 0, s, indptr, indices, eids, (const Idx*)seeds,
                       num_seeds, fanout, prob, rng_seed, out_offsets, (Idx*)out_src, (Idx*)out_eid);
}
}  // namespace mgx

extern "C" int32_t mgx_sample_neighbors_weighted(const mgx_csr* csr, int64_t num_seeds, const void* seeds, int32_t fanout,
                                                 const float* prob, int32_t replace, uint64_t rng_seed, const int64_t* out_offsets,
                                                 void* out_src, void* out_eid, void* stream) {
  using namespace mgx;
  MGX_ENTER();
  MGX_CHECK_ARG(csr != nullptr, "mgx_sample_neighbors_weighted: csr is NULL");
  MGX_CHECK_ARG(csr->idx_bits == 32 || csr->idx_bits == 64, "mgx_sample_neighbors_weighted: idx_bits must be 32 or 64");
  MGX_CHECK_ARG(num_seeds >= 0, "mgx_sample_neighbors_weighted: negative num_seeds");
  MGX_CHECK_ARG(fanout >= 1 && fanout <= kMaxFanout, "mgx_sample_neighbors_weighted: fanout must be in [1, %d], got %d", kMaxFanout,
                fanout);
  MGX_CHECK_ARG(prob || replace, "mgx_sample_neighbors_weighted: prob is NULL without replace (uniform sampling without replacement "
                                 "is mgx_sample_neighbors)");
  if (num_seeds == 0) return MGX_OK;
  MGX_CHECK_ARG(csr->indptr && seeds && out_offsets, "mgx_sample_neighbors_weighted: NULL pointer");
  MGX_CHECK_ARG(csr->nnz == 0 || (csr->indices && out_src && out_eid), "mgx_sample_neighbors_weighted: NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  if (csr->idx_bits == 32)
    launch_sample_weighted<int32_t>(csr, num_seeds, seeds, fanout, prob, replace != 0, rng_seed, out_offsets, out_src, out_eid, s);
  else
    launch_sample_weighted<int64_t>(csr, num_seeds, seeds, fanout, prob, replace != 0, rng_seed, out_offsets, out_src, out_eid, s);
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}

extern "C" int32_t mgx_select_topk(const mgx_csr* csr, int64_t num_seeds, const void* seeds, int32_t k, const float* weight,
                                   int32_t ascending, const int64_t* out_offsets, void* out_src, void* out_eid, void* stream) {
  using namespace mgx;
  MGX_ENTER();
  MGX_CHECK_ARG(csr != nullptr, "mgx_select_topk: csr is NULL");
  MGX_CHECK_ARG(csr->idx_bits == 32 || csr->idx_bits == 64, "mgx_select_topk: idx_bits must be 32 or 64");
  MGX_CHECK_ARG(num_seeds >= 0, "mgx_select_topk: negative num_seeds");
  MGX_CHECK_ARG(k >= 1 && k <= kMaxFanout, "mgx_select_topk: k must be in [1, %d], got %d", kMaxFanout, k);
  if (num_seeds == 0) return MGX_OK;
  MGX_CHECK_ARG(csr->indptr && seeds && out_offsets, "mgx_select_topk: NULL pointer");
  MGX_CHECK_ARG(csr->nnz == 0 || (csr->indices && out_src && out_eid), "mgx_select_topk: NULL pointer");
  MGX_CHECK_ARG(csr->nnz == 0 || weight, "mgx_select_topk: weight is NULL");
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid = seed_wave_grid(num_seeds);
  if (csr->idx_bits == 32)
    hipLaunchKernelGGL((select_smallest_kernel<int32_t, true>), grid, dim3(kBlock), 0, s, (const int32_t*)csr->indptr,
                       (const int32_t*)csr->indices, (const int32_t*)csr->eids, (const int32_t*)seeds, num_seeds, k, weight,
                       ascending, 0ull, out_offsets, (int32_t*)out_src, (int32_t*)out_eid);
  else
    hipLaunchKernelGGL((select_smallest_kernel<int64_t, true>), grid, dim3(kBlock), 0, s, (const int64_t*)csr->indptr,
                       (const int64_t*)csr->indices, (const int64_t*)csr->eids, (const int64_t*)seeds, num_seeds, k, weight,
                       ascending, 0ull, out_offsets, (int64_t*)out_src, (int64_t*)out_eid);
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}
