// spgemm.hip -- sparse x sparse product C = A B of two CSR operands on the device (ops.spgemm, dgl.adj_product_graph,
// dgl.metapath_reachable_graph): row-wise Gustavson with the accumulator of a row in LDS, in three steps.
//
//   bound   ub[i] = sum over the entries (i, k) of A of len(B_k), the products of row i, by a 16-lane group per row; the rows are
//           sorted (stably, rocPRIM) by class -- empty, <= 32, <= T1, <= T2, above T2 -- so that every later launch has workgroups
//           of like work.  The host reads the five class sizes (read 1 of 2).
//   count   the distinct columns of every row.  Classes 1 - 3 insert the columns into an open-addressing hash set in LDS (atomicCAS on
//           32-bit keys; 2 x the class bound slots, so it is never more than half full): a 16-lane group with 64 slots, a wave with
//           2 T1, a workgroup with 2 T2.  Rows above T2 walk their products once per window of W columns over a bitmap in LDS.
//           The caller scans the counts and reads nnz(C) (read 2 of 2).
//   fill    the same walk again; the table is sorted where it lies (bitonic, the empty key is the largest), which leaves the sorted
//           columns in its first half and the empty key in its second half; values are then added into the slot of every product,
//           found by binary search (hash classes) or by its offset in the window.
//
// Sums are deterministic.  A's entries of a row are walked one after the other and B's row across the lanes, so two products meet
// in one slot at the same time only when B's row holds a column twice (a multigraph).  Every lane proposes its lane id with an
// integer LDS atomicMin on the slot's owner word -- the emptied second half of the table -- the lowest lane adds and releases the
// slot, the others try again: additions happen in (A position, B position) order whatever the timing.  No floating-point atomic.
//
//   grad    d wa[(i,k)] = sum_{(k,j) in B} wb d wc[(i,j)] and d wb[(k,j)] = sum_{(i,k) in A} wa d wc[(i,j)] from one kernel: a
//           16-lane group per entry walks a row of the other operand (B, or A^T), finds (i, j) by binary search in C's sorted row and
//           adds across the lanes in a fixed order.
#include <cstring>
#include <rocprim/rocprim.hpp>

#include "common.h"

namespace mgx {
namespace {

constexpr uint32_t kEmpty = 0xffffffffu;  // no key / no owner: larger than every column (mgx_spgemm_supported keeps m below it)
constexpr int kSmall = 32;                // class 1: at most this many products, 64 slots, a 16-lane group
constexpr int kSmallGroup = 16;
constexpr int kHeadWords = 8;             // int64 words at the head of the workspace: class_start[6], error bits, spare

template <typename Idx>
struct SpOperands {
  const Idx *a_ptr, *a_idx, *a_eid, *b_ptr, *b_idx, *b_eid;
  const float *wa, *wb;  // by edge id, NULL = ones
  int64_t k, m;          // rows and columns of B
};

template <int GROUP>
__device__ __forceinline__ void group_sync() {
  if (GROUP > kWave) {
    __syncthreads();
  } else {  // the group is inside one wave: LDS operations of a wave complete in order, the compiler must not move them
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

// x of any lane of the group, after a group_sync
template <int GROUP>
__device__ __forceinline__ bool group_any(bool x) {
  if (GROUP > kWave) return __syncthreads_or(x);
  group_sync<GROUP>();
  const uint64_t b = __ballot(x);
  if (GROUP == kWave) return b != 0;
  const int base = (threadIdx.x & (kWave - 1)) & ~(GROUP - 1);
  return ((b >> base) & ((1ull << (GROUP % kWave)) - 1ull)) != 0;
}

// The products of row i: A's entries one after the other, B's row across the GROUP lanes.  Every lane of the group calls
// f(column, wa * wb, valid) together, so f may synchronise the group.  Entries that point outside B are skipped (mgx_spgemm_bound
// reports them in the error bits).
template <typename Idx, int GROUP, bool VALUES, typename F>
__device__ __forceinline__ void walk_products(const SpOperands<Idx>& o, int64_t i, int lane, F&& f) {
  const int64_t a0 = (int64_t)o.a_ptr[i], a1 = (int64_t)o.a_ptr[i + 1];
  for (int64_t p = a0; p < a1; ++p) {
    const int64_t kk = (int64_t)o.a_idx[p];
    if ((uint64_t)kk >= (uint64_t)o.k) continue;
    float av = 1.f;
    if (VALUES && o.wa) av = o.wa[o.a_eid ? (int64_t)o.a_eid[p] : p];
    const int64_t b0 = (int64_t)o.b_ptr[kk], b1 = (int64_t)o.b_ptr[kk + 1];
    for (int64_t q0 = b0; q0 < b1; q0 += GROUP) {
      const int64_t q = q0 + lane;
      const int64_t col = q < b1 ? (int64_t)o.b_idx[q] : -1;
      const bool valid = (uint64_t)col < (uint64_t)o.m;
      float v = 0.f;
      if (VALUES && valid) v = av * (o.wb ? o.wb[o.b_eid ? (int64_t)o.b_eid[q] : q] : 1.f);
      f((uint32_t)col, v, valid);
    }
  }
}

// acc[s] += v for every pending lane of the group, lanes that meet in one slot in lane order: the lowest proposes itself with an
// integer atomicMin, adds, and releases the slot; the others go round again.  owner[] is kEmpty between calls.
template <int GROUP>
__device__ __forceinline__ void add_in_lane_order(float* acc, uint32_t* owner, int s, float v, bool pending, uint32_t lane) {
  do {
    if (pending) atomicMin(&owner[s], lane);
    group_sync<GROUP>();
    if (pending && owner[s] == lane) {
      acc[s] += v;
      owner[s] = kEmpty;
      pending = false;
    }
  } while (group_any<GROUP>(pending));
}

// keys[0 .. table) ascending (table a power of two), by the GROUP lanes; the empty key ends up behind every column
template <int GROUP>
__device__ __forceinline__ void bitonic_sort(uint32_t* keys, int table, int lane) {
  for (int k = 2; k <= table; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = lane; t < (table >> 1); t += GROUP) {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
        const uint32_t x = keys[lo], y = keys[hi];
        if ((x > y) == ((lo & k) == 0)) {
          keys[lo] = y;
          keys[hi] = x;
        }
      }
      group_sync<GROUP>();
    }
  }
}

// Classes 1 - 3: one GROUP of lanes per row of `rows`, a hash set of `table` keys per group (and table / 2 sums when FILL writes
// values).  Words per group in LDS: table + (values ? table / 2 : 0) + 1.
template <typename Idx, int GROUP, bool FILL>
__global__ __launch_bounds__(kBlock) void spgemm_hash_kernel(SpOperands<Idx> o, const int32_t* rows, int64_t n_list, int table,
                                                             int shift, int64_t* counts, const int64_t* offsets, Idx* c_idx, float* wc) {
  extern __shared__ uint32_t lds[];
  const int g = threadIdx.x / GROUP, lane = threadIdx.x % GROUP;
  const int64_t li = (int64_t)blockIdx.x * (kBlock / GROUP) + g;
  if (li >= n_list) return;  // a whole group; GROUP = kBlock has one row per workgroup and a grid of n_list
  const bool values = FILL && wc != nullptr;
  uint32_t* keys = lds + (size_t)g * (table + (values ? table / 2 : 0) + 1);
  uint32_t* tail = keys + table;  // count: the counter; fill: the sums
  const int64_t i = rows[li];
  for (int t = lane; t < table; t += GROUP) keys[t] = kEmpty;
  if (lane == 0) tail[0] = 0u;
  group_sync<GROUP>();
  walk_products<Idx, GROUP, false>(o, i, lane, [&](uint32_t col, float, bool valid) {
    if (!valid) return;
    uint32_t h = (col * 2654435761u) >> shift;
    for (int probe = 0; probe < table; ++probe) {  // at most half full: ends long before the bound
      const uint32_t old = atomicCAS(&keys[h], kEmpty, col);
      if (old == kEmpty || old == col) return;
      h = (h + 1) & (uint32_t)(table - 1);
    }
  });
  group_sync<GROUP>();
  if (!FILL) {
    int c = 0;
    for (int t = lane; t < table; t += GROUP) c += keys[t] != kEmpty;
    if (c) atomicAdd(&tail[0], (uint32_t)c);
    group_sync<GROUP>();
    if (lane == 0) counts[i] = (int64_t)tail[0];
    return;
  }
  bitonic_sort<GROUP>(keys, table, lane);
  const int64_t off = offsets[i];
  int cnt = (int)(offsets[i + 1] - off);
  if (cnt > table / 2) cnt = table / 2;
  for (int t = lane; t < cnt; t += GROUP) c_idx[off + t] = (Idx)keys[t];
  if (!values) return;
  float* acc = reinterpret_cast<float*>(tail);
  uint32_t* owner = keys + table / 2;  // the emptied half of the table: kEmpty everywhere
  for (int t = lane; t < table / 2; t += GROUP) acc[t] = 0.f;
  group_sync<GROUP>();
  walk_products<Idx, GROUP, true>(o, i, lane, [&](uint32_t col, float v, bool valid) {
    int lo = 0, hi = cnt;
    while (valid && lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (keys[mid] < col) lo = mid + 1; else hi = mid;
    }
    valid = valid && lo < cnt && keys[lo] == col;
    add_in_lane_order<GROUP>(acc, owner, valid ? lo : 0, v, valid, (uint32_t)lane);
  });
  group_sync<GROUP>();
  for (int t = lane; t < cnt; t += GROUP) wc[off + t] = acc[t];
}

// Class 4: a workgroup per row, the columns in windows of W: a bitmap of W bits, its word ranks and -- FILL with values -- W sums
// and W owner words in LDS.  The row's products are walked once per window (twice where values are added).
// LDS words: W / 32 + 256 + 4 + (values ? 2 W : 0).
template <typename Idx, bool FILL>
__global__ __launch_bounds__(kBlock) void spgemm_window_kernel(SpOperands<Idx> o, const int32_t* rows, int W, int64_t* counts,
                                                               const int64_t* offsets, Idx* c_idx, float* wc) {
  extern __shared__ uint32_t lds[];
  const int tid = threadIdx.x, nwords = W >> 5;  // nwords <= kBlock
  const bool values = FILL && wc != nullptr;
  uint32_t* bits = lds;
  uint32_t* pref = bits + nwords;  // [kBlock] words set before word t
  uint32_t* wsum = pref + kBlock;  // [4]
  float* acc = reinterpret_cast<float*>(wsum + 4);
  uint32_t* owner = wsum + 4 + W;
  const int64_t i = rows[blockIdx.x];
  int64_t base = FILL ? offsets[i] : 0, total = 0;
  for (int64_t w0 = 0; w0 < o.m; w0 += W) {
    for (int t = tid; t < nwords; t += kBlock) bits[t] = 0u;
    if (values)
      for (int t = tid; t < W; t += kBlock) {
        acc[t] = 0.f;
        owner[t] = kEmpty;
      }
    __syncthreads();
    walk_products<Idx, kBlock, false>(o, i, tid, [&](uint32_t col, float, bool valid) {
      const int64_t d = (int64_t)col - w0;
      if (valid && d >= 0 && d < W) atomicOr(&bits[d >> 5], 1u << (d & 31));
    });
    __syncthreads();
    const int mine = tid < nwords ? __popc(bits[tid]) : 0;
    int inc = mine;
    for (int d = 1; d < kWave; d <<= 1) {
      const int up = __shfl_up(inc, d, kWave);
      if ((tid & (kWave - 1)) >= d) inc += up;
    }
    if ((tid & (kWave - 1)) == kWave - 1) wsum[tid / kWave] = (uint32_t)inc;
    __syncthreads();
    int before = 0, cntw = 0;
    for (int w = 0; w < kWavesPerBlock; ++w) {
      if (w < tid / kWave) before += (int)wsum[w];
      cntw += (int)wsum[w];
    }
    pref[tid] = (uint32_t)(before + inc - mine);
    __syncthreads();
    if (FILL && cntw) {
      for (int t = tid; t < nwords; t += kBlock) {
        int64_t at = base + pref[t];
        for (uint32_t wd = bits[t]; wd; wd &= wd - 1) c_idx[at++] = (Idx)(w0 + t * 32 + (__ffs(wd) - 1));
      }
      if (values) {
        walk_products<Idx, kBlock, true>(o, i, tid, [&](uint32_t col, float v, bool valid) {
          const int64_t d = (int64_t)col - w0;
          const bool in = valid && d >= 0 && d < W;
          add_in_lane_order<kBlock>(acc, owner, in ? (int)d : 0, v, in, (uint32_t)tid);
        });
        __syncthreads();
        for (int t = tid; t < nwords; t += kBlock) {
          int64_t at = base + pref[t];
          for (uint32_t wd = bits[t]; wd; wd &= wd - 1) wc[at++] = acc[t * 32 + (__ffs(wd) - 1)];
        }
      }
    }
    base += cntw;
    total += cntw;
    __syncthreads();
  }
  if (!FILL && tid == 0) counts[i] = total;
}

// ---- bound: products per row, classes, row lists
__global__ __launch_bounds__(kBlock) void spgemm_iota_kernel(int32_t* iota, int64_t n, int64_t* head) {
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t < kHeadWords) head[t] = 0;
  for (int64_t r = t; r < n; r += (int64_t)gridDim.x * kBlock) iota[r] = (int32_t)r;
}

template <typename Idx>
__global__ __launch_bounds__(kBlock) void spgemm_bound_kernel(const Idx* a_ptr, const Idx* a_idx, const Idx* b_ptr, int64_t n, int64_t k,
                                                              int64_t t1, int64_t t2, int32_t* cls, int64_t* err) {
  const int64_t i = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / kSmallGroup;
  const int lane = threadIdx.x % kSmallGroup;
  if (i >= n) return;
  int64_t ub = 0;
  bool bad = false;
  for (int64_t p = (int64_t)a_ptr[i] + lane; p < (int64_t)a_ptr[i + 1]; p += kSmallGroup) {
    const int64_t kk = (int64_t)a_idx[p];
    if ((uint64_t)kk >= (uint64_t)k) bad = true;
    else ub += (int64_t)b_ptr[kk + 1] - (int64_t)b_ptr[kk];
  }
  for (int d = kSmallGroup / 2; d > 0; d >>= 1) ub += __shfl_xor(ub, d, kWave);
  if (bad) atomicOr((unsigned long long*)err, 1ull);
  if (lane == 0) cls[i] = ub == 0 ? 0 : ub <= kSmall ? 1 : ub <= t1 ? 2 : ub <= t2 ? 3 : 4;
}

template <typename Idx>
__global__ __launch_bounds__(kBlock) void spgemm_check_cols_kernel(const Idx* idx, int64_t nnz, int64_t m, int64_t* err) {
  bool bad = false;
  for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < nnz; p += (int64_t)gridDim.x * kBlock)
    bad |= (uint64_t)(int64_t)idx[p] >= (uint64_t)m;
  if (bad) atomicOr((unsigned long long*)err, 2ull);
}

__global__ void spgemm_class_start_kernel(const int32_t* sorted_cls, int64_t n, int64_t* class_start) {
  const int c = threadIdx.x;  // 0 .. 5: the first position whose class is >= c
  if (c > 5) return;
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (sorted_cls[mid] < c) lo = mid + 1; else hi = mid;
  }
  class_start[c] = lo;
}

__global__ __launch_bounds__(kBlock) void spgemm_zero_rows_kernel(const int32_t* rows, int64_t n_list, int64_t* counts) {
  for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < n_list; r += (int64_t)gridDim.x * kBlock) counts[rows[r]] = 0;
}

// ---- grad: mode 0 = d wa (x = A, y = B), mode 1 = d wb (x = B, y = A^T)
template <typename Idx>
__global__ __launch_bounds__(kBlock) void spgemm_grad_kernel(const Idx* x_ptr, const Idx* x_idx, const Idx* x_eid, int64_t x_rows,
                                                             int64_t x_nnz, const Idx* y_ptr, const Idx* y_idx, const Idx* y_eid,
                                                             int64_t y_rows, const float* wy, const Idx* c_ptr, const Idx* c_idx,
                                                             int64_t c_rows, const float* d_wc, float* d_wx, int mode) {
  const int64_t p = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / kSmallGroup;
  const int lane = threadIdx.x % kSmallGroup;
  if (p >= x_nnz) return;
  int64_t lo = 0, hi = x_rows;  // x_ptr[lo] <= p < x_ptr[hi]
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)x_ptr[mid] <= p) lo = mid; else hi = mid;
  }
  const int64_t r = lo, c = (int64_t)x_idx[p], yr = mode ? r : c;
  float sum = 0.f;
  if ((uint64_t)yr < (uint64_t)y_rows) {
    for (int64_t q = (int64_t)y_ptr[yr] + lane; q < (int64_t)y_ptr[yr + 1]; q += kSmallGroup) {
      const int64_t t = (int64_t)y_idx[q], crow = mode ? t : r, ccol = mode ? c : t;
      if ((uint64_t)crow >= (uint64_t)c_rows) continue;
      int64_t l = (int64_t)c_ptr[crow], h = (int64_t)c_ptr[crow + 1];
      const int64_t end = h;
      while (l < h) {
        const int64_t mid = (l + h) >> 1;
        if ((int64_t)c_idx[mid] < ccol) l = mid + 1; else h = mid;
      }
      if (l < end && (int64_t)c_idx[l] == ccol) sum += (wy ? wy[y_eid ? (int64_t)y_eid[q] : q] : 1.f) * d_wc[l];
    }
  }
  sum = lanes_sum<kSmallGroup>(sum);
  if (lane == 0) d_wx[x_eid ? (int64_t)x_eid[p] : p] = sum;
}

inline size_t align256(size_t x) { return (x + 255) / 256 * 256; }
inline unsigned grid_for(int64_t n) {
  int64_t b = (n + kBlock - 1) / kBlock;
  return (unsigned)(b < 1 ? 1 : b > 256 * 32 ? 256 * 32 : b);
}

hipError_t sort_temp_bytes(int64_t n, size_t* bytes) {
  *bytes = 0;
  return rocprim::radix_sort_pairs<rocprim::default_config, const int32_t*, int32_t*, const int32_t*, int32_t*>(
      nullptr, *bytes, nullptr, nullptr, nullptr, nullptr, (size_t)n, 0, 3, nullptr, false);
}

struct Workspace {
  int64_t* head;
  int32_t *cls, *sorted_cls, *iota, *rows;
  void* temp;
  Workspace(void* ws, int64_t n) {
    const size_t arr = align256(sizeof(int32_t) * (size_t)n);
    char* p = (char*)ws;
    head = (int64_t*)p;
    p += align256(sizeof(int64_t) * kHeadWords);
    cls = (int32_t*)p;
    sorted_cls = (int32_t*)(p + arr);
    iota = (int32_t*)(p + 2 * arr);
    rows = (int32_t*)(p + 3 * arr);
    temp = p + 4 * arr;
  }
};

bool pow2(int64_t x) { return x > 0 && (x & (x - 1)) == 0; }

int32_t check_operands(const char* who, const mgx_csr* a, const mgx_csr* b) {
  MGX_CHECK_ARG(a && b, "%s: NULL operand", who);
  if (!mgx_spgemm_supported(a, b)) MGX_UNSUPPORTED("%s: operands outside mgx_spgemm_supported", who);
  MGX_CHECK_ARG(a->indptr && b->indptr && (a->nnz == 0 || a->indices) && (b->nnz == 0 || b->indices), "%s: NULL pointer", who);
  return MGX_OK;
}

int32_t check_constants(const char* who, int64_t t1, int64_t t2, int64_t w) {
  MGX_CHECK_ARG(pow2(t1) && pow2(t2) && t1 >= 2 * kSmall && t1 <= 1024 && t2 > t1 && t2 <= 4096,
                "%s: T1 and T2 must be powers of two with 64 <= T1 <= 1024 and T1 < T2 <= 4096, got %lld and %lld", who, (long long)t1,
                (long long)t2);
  MGX_CHECK_ARG(w >= 32 && w <= 7168 && w % 32 == 0, "%s: W must be a multiple of 32 in 32 .. 7168, got %lld", who, (long long)w);
  return MGX_OK;
}

template <typename Idx>
SpOperands<Idx> operands(const mgx_csr* a, const mgx_csr* b, const float* wa, const float* wb) {
  SpOperands<Idx> o;
  o.a_ptr = (const Idx*)a->indptr, o.a_idx = (const Idx*)a->indices, o.a_eid = (const Idx*)a->eids;
  o.b_ptr = (const Idx*)b->indptr, o.b_idx = (const Idx*)b->indices, o.b_eid = (const Idx*)b->eids;
  o.wa = wa, o.wb = wb, o.k = b->num_rows, o.m = b->num_cols;
  return o;
}

// the launches of count (FILL = false) or fill over the four classes with rows
template <typename Idx, bool FILL>
int32_t run_classes(const mgx_csr* a, const mgx_csr* b, const float* wa, const float* wb, int64_t t1, int64_t t2, int64_t w,
                    const int64_t* class_start, void* workspace, int64_t* counts, const int64_t* offsets, Idx* c_idx, float* wc,
                    hipStream_t s) {
  const Workspace ws(workspace, a->num_rows);
  const SpOperands<Idx> o = operands<Idx>(a, b, wa, wb);
  const bool values = FILL && wc != nullptr;
  const int64_t tables[4] = {0, 2 * kSmall, 2 * t1, 2 * t2};
  for (int c = 1; c <= 4; ++c) {
    const int64_t n_list = class_start[c + 1] - class_start[c];
    if (n_list <= 0) continue;
    const int32_t* rows = ws.rows + class_start[c];
    if (c == 4) {
      const size_t lds = sizeof(uint32_t) * (size_t)(w / 32 + kBlock + 4 + (values ? 2 * w : 0));
      hipLaunchKernelGGL((spgemm_window_kernel<Idx, FILL>), dim3((unsigned)n_list), dim3(kBlock), lds, s, o, rows, (int)w, counts, offsets,
                         c_idx, wc);
    } else {
      const int table = (int)tables[c], shift = 32 - ilog2_ceil(table);
      const int group = c == 1 ? kSmallGroup : c == 2 ? kWave : kBlock;
      const size_t lds = sizeof(uint32_t) * (size_t)(kBlock / group) * (size_t)(table + (values ? table / 2 : 0) + 1);
      const dim3 grid((unsigned)((n_list + kBlock / group - 1) / (kBlock / group)));
      if (c == 1)
        hipLaunchKernelGGL((spgemm_hash_kernel<Idx, kSmallGroup, FILL>), grid, dim3(kBlock), lds, s, o, rows, n_list, table, shift, counts,
                           offsets, c_idx, wc);
      else if (c == 2)
        hipLaunchKernelGGL((spgemm_hash_kernel<Idx, kWave, FILL>), grid, dim3(kBlock), lds, s, o, rows, n_list, table, shift, counts,
                           offsets, c_idx, wc);
      else
        hipLaunchKernelGGL((spgemm_hash_kernel<Idx, kBlock, FILL>), grid, dim3(kBlock), lds, s, o, rows, n_list, table, shift, counts,
                           offsets, c_idx, wc);
    }
    MGX_CHECK_LAUNCH();
  }
  return MGX_OK;
}

int32_t check_class_start(const char* who, const int64_t* cs, int64_t n) {
  MGX_CHECK_ARG(cs != nullptr, "%s: class_start is NULL", who);
  MGX_CHECK_ARG(cs[0] == 0 && cs[5] == n, "%s: class_start does not cover the %lld rows", who, (long long)n);
  for (int c = 0; c < 5; ++c) MGX_CHECK_ARG(cs[c] <= cs[c + 1], "%s: class_start descends", who);
  return MGX_OK;
}

template <typename Idx>
int32_t bound_impl(const mgx_csr* a, const mgx_csr* b, int64_t t1, int64_t t2, void* workspace, hipStream_t s) {
  const int64_t n = a->num_rows;
  const Workspace ws(workspace, n);
  size_t temp = 0;
  MGX_CHECK_HIP(sort_temp_bytes(n, &temp));
  hipLaunchKernelGGL(spgemm_iota_kernel, dim3(grid_for(n)), dim3(kBlock), 0, s, ws.iota, n, ws.head);
  MGX_CHECK_LAUNCH();
  hipLaunchKernelGGL((spgemm_bound_kernel<Idx>), dim3((unsigned)((n * kSmallGroup + kBlock - 1) / kBlock)), dim3(kBlock), 0, s,
                     (const Idx*)a->indptr, (const Idx*)a->indices, (const Idx*)b->indptr, n, b->num_rows, t1, t2, ws.cls, ws.head + 6);
  MGX_CHECK_LAUNCH();
  if (b->nnz > 0) {
    hipLaunchKernelGGL((spgemm_check_cols_kernel<Idx>), dim3(grid_for(b->nnz)), dim3(kBlock), 0, s, (const Idx*)b->indices, b->nnz,
                       b->num_cols, ws.head + 6);
    MGX_CHECK_LAUNCH();
  }
  MGX_CHECK_HIP((rocprim::radix_sort_pairs<rocprim::default_config, const int32_t*, int32_t*, const int32_t*, int32_t*>(
      ws.temp, temp, ws.cls, ws.sorted_cls, (const int32_t*)ws.iota, ws.rows, (size_t)n, 0, 3, s, false)));
  hipLaunchKernelGGL(spgemm_class_start_kernel, dim3(1), dim3(kWave), 0, s, (const int32_t*)ws.sorted_cls, n, ws.head);
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}

template <typename Idx>
int32_t grad_impl(const mgx_csr* x, const mgx_csr* y, int32_t mode, const float* wy, const mgx_csr* c, const float* d_wc, float* d_wx,
                  hipStream_t s) {
  hipLaunchKernelGGL((spgemm_grad_kernel<Idx>), dim3((unsigned)((x->nnz * kSmallGroup + kBlock - 1) / kBlock)), dim3(kBlock), 0, s,
                     (const Idx*)x->indptr, (const Idx*)x->indices, (const Idx*)x->eids, x->num_rows, x->nnz, (const Idx*)y->indptr,
                     (const Idx*)y->indices, (const Idx*)y->eids, y->num_rows, wy, (const Idx*)c->indptr, (const Idx*)c->indices,
                     c->num_rows, d_wc, d_wx, (int)mode);
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}

}  // namespace
}  // namespace mgx

extern "C" int32_t mgx_spgemm_supported(const mgx_csr* a, const mgx_csr* b) {
  if (!a || !b || a->idx_bits != b->idx_bits || (a->idx_bits != 32 && a->idx_bits != 64)) return 0;
  if (a->num_rows < 0 || a->num_cols < 0 || b->num_cols < 0 || a->nnz < 0 || b->nnz < 0 || a->num_cols != b->num_rows) return 0;
  const int64_t lim = int64_t(1) << 31;  // 32-bit keys in LDS and 32-bit row lists; 16 lanes per row / entry within a 32-bit grid
  if (b->num_cols >= lim - 1 || a->num_rows >= lim / 16 || a->nnz >= lim / 16 || b->nnz >= lim / 16) return 0;
  return 1;
}

extern "C" int64_t mgx_spgemm_workspace(int64_t n_rows) {
  using namespace mgx;
  MGX_ENTER();
  if (n_rows < 0) return -1;
  size_t temp = 0;
  if (n_rows > 0 && sort_temp_bytes(n_rows, &temp) != hipSuccess) {
    set_error("mgx_spgemm_workspace: rocPRIM size query failed");
    return -1;
  }
  return (int64_t)(align256(sizeof(int64_t) * kHeadWords) + 4 * align256(sizeof(int32_t) * (size_t)n_rows) + temp);
}

extern "C" int32_t mgx_spgemm_bound(const mgx_csr* a, const mgx_csr* b, int64_t t1, int64_t t2, void* workspace, void* stream) {
  using namespace mgx;
  MGX_ENTER();
  if (int32_t st = check_operands("mgx_spgemm_bound", a, b)) return st;
  if (int32_t st = check_constants("mgx_spgemm_bound", t1, t2, 32)) return st;
  MGX_CHECK_ARG(workspace != nullptr && a->num_rows > 0, "mgx_spgemm_bound: NULL workspace or no rows");
  return a->idx_bits == 32 ? bound_impl<int32_t>(a, b, t1, t2, workspace, (hipStream_t)stream)
                           : bound_impl<int64_t>(a, b, t1, t2, workspace, (hipStream_t)stream);
}

extern "C" int32_t mgx_spgemm_count(const mgx_csr* a, const mgx_csr* b, int64_t t1, int64_t t2, int64_t w, const int64_t* class_start,
                                    void* workspace, int64_t* counts, void* stream) {
  using namespace mgx;
  MGX_ENTER();
  if (int32_t st = check_operands("mgx_spgemm_count", a, b)) return st;
  if (int32_t st = check_constants("mgx_spgemm_count", t1, t2, w)) return st;
  if (int32_t st = check_class_start("mgx_spgemm_count", class_start, a->num_rows)) return st;
  MGX_CHECK_ARG(workspace && counts, "mgx_spgemm_count: NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  if (class_start[1] > 0) {
    hipLaunchKernelGGL(spgemm_zero_rows_kernel, dim3(grid_for(class_start[1])), dim3(kBlock), 0, s,
                       (const int32_t*)Workspace(workspace, a->num_rows).rows, class_start[1], counts);
    MGX_CHECK_LAUNCH();
  }
  return a->idx_bits == 32
             ? run_classes<int32_t, false>(a, b, nullptr, nullptr, t1, t2, w, class_start, workspace, counts, nullptr, nullptr, nullptr, s)
             : run_classes<int64_t, false>(a, b, nullptr, nullptr, t1, t2, w, class_start, workspace, counts, nullptr, nullptr, nullptr, s);
}

extern "C" int32_t mgx_spgemm_fill(const mgx_csr* a, const mgx_csr* b, const float* wa, const float* wb, int64_t t1, int64_t t2, int64_t w,
                                   const int64_t* class_start, void* workspace, const int64_t* offsets, void* c_indices, float* wc,
                                   void* stream) {
  using namespace mgx;
  MGX_ENTER();
  if (int32_t st = check_operands("mgx_spgemm_fill", a, b)) return st;
  if (int32_t st = check_constants("mgx_spgemm_fill", t1, t2, w)) return st;
  if (int32_t st = check_class_start("mgx_spgemm_fill", class_start, a->num_rows)) return st;
  MGX_CHECK_ARG(workspace && offsets && c_indices, "mgx_spgemm_fill: NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  return a->idx_bits == 32 ? run_classes<int32_t, true>(a, b, wa, wb, t1, t2, w, class_start, workspace, nullptr, offsets,
                                                        (int32_t*)c_indices, wc, s)
                           : run_classes<int64_t, true>(a, b, wa, wb, t1, t2, w, class_start, workspace, nullptr, offsets,
                                                        (int64_t*)c_indices, wc, s);
}

extern "C" int32_t mgx_spgemm_grad(const mgx_csr* x, const mgx_csr* y, int32_t mode, const float* wy, const mgx_csr* c, const float* d_wc,
                                   float* d_wx, void* stream) {
  using namespace mgx;
  MGX_ENTER();
  MGX_CHECK_ARG(x && y && c && (mode == 0 || mode == 1), "mgx_spgemm_grad: NULL operand or mode not 0 / 1");
  MGX_CHECK_ARG(x->idx_bits == y->idx_bits && x->idx_bits == c->idx_bits && (x->idx_bits == 32 || x->idx_bits == 64),
                "mgx_spgemm_grad: idx_bits must be 32 or 64 and the same everywhere");
  MGX_CHECK_ARG(mode == 0 ? (y->num_rows == x->num_cols && c->num_rows == x->num_rows && c->num_cols == y->num_cols)
                          : (y->num_rows == x->num_rows && c->num_rows == y->num_cols && c->num_cols == x->num_cols),
                "mgx_spgemm_grad: the shapes of x, y and c do not fit mode %d", (int)mode);
  if (x->nnz >= (int64_t(1) << 31) / 16) MGX_UNSUPPORTED("mgx_spgemm_grad: too many entries");
  if (x->nnz == 0) return MGX_OK;
  MGX_CHECK_ARG(x->indptr && x->indices && y->indptr && c->indptr && (y->nnz == 0 || y->indices) && (c->nnz == 0 || (c->indices && d_wc)) && d_wx,
                "mgx_spgemm_grad: NULL pointer");
  return x->idx_bits == 32 ? grad_impl<int32_t>(x, y, mode, wy, c, d_wc, d_wx, (hipStream_t)stream)
                           : grad_impl<int64_t>(x, y, mode, wy, c, d_wc, d_wx, (hipStream_t)stream);
}
