// plan_walk.h -- the walk skeleton the two attention families (gatfused.hip with gat_tile.inc, dotattn.hip) share: the work items
// of an mgx_spmm_plan as kernel arguments, a block's stretch of them and one item's (row, edge range), the slot convention of a
// split (hub) row, the two kernels that merge a hub row's chunks in slot order, and the plan's argument checks.
// What stays with each family: its edge loop and lane-group merge, its NaN rule and its statistics layout (dotattn.hip).
// The row walks with 16-byte lanes (gine.hip, multiagg.hip) also take their supported set and argument checks from here (row_walk_*).
#pragma once
#include <math.h>

#include "common.h"

namespace mgx {

// ---------------------------------------------------------------------------------------------- the plan as kernel arguments
struct PlanItems {  // 32-bit graphs only, as both families require
  const int32_t* indptr;
  const int32_t* indices;
  const int32_t* item_row;  // plan (all NULL: one item per row)
  const int32_t* item_beg;
  const int32_t* item_end;
  const int32_t* item_node;
  int64_t n_items;
  XcdRanges xcd;    // item stretch of every XCD (edge balanced when the plan says so)
  int64_t nblocks;  // grid size
  int rpb;          // work items per workgroup
};

constexpr int kPlanRowsPerBlock = 16;  // work items per workgroup: the g-SpMM's measured choice (spmm.hip)

static inline void plan_items_fill(PlanItems& p, const mgx_csr* csr, const mgx_spmm_plan* plan, int rpb) {
  memset(&p, 0, sizeof(p));
  p.indptr = (const int32_t*)csr->indptr; p.indices = (const int32_t*)csr->indices;
  p.n_items = csr->num_rows;
  if (plan) {
    p.item_row = plan->item_row; p.item_beg = (const int32_t*)plan->item_beg; p.item_end = (const int32_t*)plan->item_end;
    p.item_node = plan->item_node; p.n_items = plan->num_items;
  }
  p.rpb = rpb;
  p.nblocks = xcd_ranges(plan, p.n_items, p.rpb, p.xcd);
}

// a malformed plan (NULL plan: nothing to check); the last checks of gat_check and dot_check
static inline int32_t plan_check(const mgx_csr* csr, const mgx_spmm_plan* plan, const char* who) {
  if (plan) {
    MGX_CHECK_ARG(plan->item_row && plan->item_beg && plan->item_end && plan->item_node && plan->num_items >= csr->num_rows,
                  "%s: malformed plan", who);
    MGX_CHECK_ARG(plan->num_slots == 0 || (plan->hub_row && plan->hub_slot_ptr), "%s: plan has split rows but no hub tables", who);
  }
  return MGX_OK;
}

// This block's items [first, stop): its XCD's stretch from the block's own group of rpb items on.  Wave w takes items
// first + w, first + w + 4, ... of the group: `for (int r = wave; r < p.rpb; r += kWavesPerBlock)`, leaving at `stop`.
__device__ __forceinline__ void plan_block_items(const PlanItems& p, int64_t& first, int64_t& stop) {
  xcd_stretch(p.xcd, first, stop);
  first += (int64_t)(blockIdx.x / kXcds) * p.rpb;
}

struct PlanItem {
  int64_t row, irow;  // row: the node whose edges these are; irow: the same, or for a chunk of a hub row its slot (plan_slot)
  int32_t beg, end;   // CSR positions
};
__device__ __forceinline__ PlanItem plan_item(const PlanItems& p, int64_t item) {
  PlanItem it;
  if (p.item_row) {
    it.irow = p.item_row[item];
    it.row = p.item_node[item];
    it.beg = p.item_beg[item];
    it.end = p.item_end[item];
  } else {
    it.irow = it.row = item;
    it.beg = p.indptr[item];
    it.end = p.indptr[item + 1];
  }
  return it;
}

// A chunk of a hub row carries irow = -(slot + 1) < 0: it writes its partial result to row `slot` of the workspace instead of the
// output, and hub_rows_sum / hub_online_merge combine the slots hub_slot_ptr gives the row, in slot order (the tile plans' tile_item
// follows the same convention).
__device__ __forceinline__ int64_t plan_slot(int64_t irow) { return -(irow + 1); }

// edges in flight per lane group of G lanes: four, fewer when the wave holds many groups
template <int G>
struct LaneUnroll {
  static constexpr int NB = kWave / G;
  static constexpr int value = NB >= 16 ? 1 : (NB >= 8 ? 2 : 4);
};

// max that keeps a NaN (fmaxf drops it): a NaN logit must reach the row's result
__device__ __forceinline__ float nan_max(float a, float b) { return (a > b || a != a) ? a : b; }

// a lane's 16 bytes of a row product (dotattn.hip, segattn.hip); lanes_sum<LPH> completes the head's dot product
__device__ __forceinline__ float dot4(const v4f& a, const v4f& b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }

// ---------------------------------------------------------------------------------------------- row walks with 16-byte lanes
// What gine.hip and multiagg.hip share on the host side: G lanes of 16 bytes cover a row of D floats, the supported set and its checks.
static inline int row_walk_lanes(int D) {  // the smallest power of two G with 4 G >= D
  int G = 1;
  while (G * 4 < D) G <<= 1;
  return G;
}

static inline bool row_walk_width_ok(int64_t D) { return D >= 4 && D % 4 == 0 && D <= 256; }

// gathered rows are addressed by 32-bit byte offsets: every [nodes, D] and [nnz, D] matrix stays below 4 GiB
static inline bool row_walk_size_ok(const mgx_csr* csr, int64_t D) {
  int64_t most = csr->num_rows > csr->num_cols ? csr->num_rows : csr->num_cols;
  if (csr->nnz > most) most = csr->nnz;
  return csr->nnz < (int64_t(1) << 31) && most * D * 4 < (int64_t(1) << 32);
}

static inline bool row_walk_supported(const mgx_csr* csr, int64_t D) {
  return csr && csr->idx_bits == 32 && csr->nnz > 0 && row_walk_width_ok(D) && row_walk_size_ok(csr, D);
}

static inline int32_t row_walk_check(const mgx_csr* csr, const mgx_spmm_plan* plan, int64_t D, const char* who) {
  MGX_CHECK_ARG(csr != nullptr, "%s: csr is NULL", who);
  MGX_CHECK_ARG(csr->idx_bits == 32 || csr->idx_bits == 64, "%s: idx_bits must be 32 or 64 (got %d)", who, csr->idx_bits);
  MGX_CHECK_ARG(D >= 4 && D % 4 == 0, "%s: D must be a positive multiple of 4 (got %lld)", who, (long long)D);
  MGX_CHECK_ARG(csr->indptr && (csr->indices || csr->nnz <= 0), "%s: indptr / indices is NULL", who);
  const int32_t st = plan_check(csr, plan, who);  // argument errors first, then what is outside the supported set
  if (st != MGX_OK) return st;
  if (csr->idx_bits != 32) MGX_UNSUPPORTED("%s: 32-bit graph indices only (got %d)", who, csr->idx_bits);
  if (!row_walk_width_ok(D)) MGX_UNSUPPORTED("%s: needs D <= 256 (got %lld)", who, (long long)D);
  if (csr->nnz <= 0) MGX_UNSUPPORTED("%s: graph without edges", who);
  if (!row_walk_size_ok(csr, D)) MGX_UNSUPPORTED("%s: operands beyond 32-bit byte offsets", who);
  return MGX_OK;
}

static inline bool row_aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }

// ---------------------------------------------------------------------------------------------- hub rows
static inline dim3 hub_grid(const mgx_spmm_plan* plan) {  // one wave per hub row
  return dim3((unsigned)((plan->num_hubs + kWavesPerBlock - 1) / kWavesPerBlock));
}

// out[hub_row[h], k] = sum over the hub's slots, in slot order, of partial[slot, k]   (no atomics: deterministic)
static __global__ __launch_bounds__(kBlock) void hub_rows_sum_kernel(const int32_t* hub_row, const int32_t* hub_slot_ptr, int64_t n_hubs,
                                                                     int L, const float* partial, float* out) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t h = (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
  if (h >= n_hubs) return;
  const int64_t row = hub_row[h];
  const int s0 = hub_slot_ptr[h], s1 = hub_slot_ptr[h + 1];
  for (int k = lane; k < L; k += kWave) {
    float acc = 0.f;
    for (int s = s0; s < s1; ++s) acc += partial[(int64_t)s * L + k];
    out[row * L + k] = acc;
  }
}

static inline void hub_rows_sum(const mgx_spmm_plan* plan, int L, const float* partial, float* out, hipStream_t s) {
  hipLaunchKernelGGL(hub_rows_sum_kernel, hub_grid(plan), dim3(kBlock), 0, s, plan->hub_row, plan->hub_slot_ptr, plan->num_hubs, L, partial,
                     out);
}

// Online softmax of a hub row: each chunk leaves (running max m_c, sum s_c) per head in pstat [slot, 2H] and an accumulator
// relative to m_c in partial [slot, D]; merged in slot order: m = max m_c, s = sum s_c e^(m_c - m), out = sum acc_c e^(m_c - m) / s.
// The row's statistics go to stat [row, H, 4]: (er, m, 1/s, 0) with `er` (GAT), (m, 1/s, 0, 0) without (dot product).
// KEEP_NAN is the family's rule for a NaN logit, the one its gather kernels apply -- the two give different statistics for such a
// row and the backward reads them, so they are NOT one rule:
//   false (GAT):         fmaxf drops a NaN maximum, a chunk counts when m_c > -inf, 1/s = 0 unless s > 0   -> m finite, 1/s = 0
//   true  (dot product): nan_max keeps it, a chunk counts unless m_c == -inf, 1/s = 0 only for s == 0      -> m = 1/s = NaN
template <bool KEEP_NAN>
__global__ __launch_bounds__(kBlock) void hub_online_merge_kernel(const int32_t* hub_row, const int32_t* hub_slot_ptr, int64_t n_hubs, int H,
                                                                  int F, const float* er, const float* partial, const float* pstat,
                                                                  float* out, float* stat) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t hb = (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
  if (hb >= n_hubs) return;
  const int64_t row = hub_row[hb];
  const int s0 = hub_slot_ptr[hb], s1 = hub_slot_ptr[hb + 1];
  const int D = H * F;
  for (int k = lane; k < D; k += kWave) {
    const int h = k / F;
    float m = -INFINITY;
    for (int s = s0; s < s1; ++s) {
      const float mc = pstat[(int64_t)s * 2 * H + h];
      m = KEEP_NAN ? nan_max(m, mc) : fmaxf(m, mc);
    }
    float sum = 0.f, acc = 0.f;
    for (int s = s0; s < s1; ++s) {
      const float mc = pstat[(int64_t)s * 2 * H + h];
      if (KEEP_NAN ? !(mc == -INFINITY) : mc > -INFINITY) {
        const float fct = __expf(mc - m);
        sum += pstat[(int64_t)s * 2 * H + H + h] * fct;
        acc += partial[(int64_t)s * D + k] * fct;
      }
    }
    float is, ms;
    if (KEEP_NAN) {
      is = sum == 0.f ? 0.f : 1.f / sum;
      ms = m == -INFINITY ? 0.f : m;
    } else {
      is = sum > 0.f ? 1.f / sum : 0.f;
      ms = m > -INFINITY ? m : 0.f;
    }
    out[row * D + k] = acc * is;
    if (k % F == 0) {
      v4f st;
      if (er) { st.x = er[row * H + h]; st.y = ms; st.z = is; }
      else { st.x = ms; st.y = is; st.z = 0.f; }
      st.w = 0.f;
      *reinterpret_cast<v4f*>(stat + (row * H + h) * 4) = st;
    }
  }
}

template <bool KEEP_NAN>
static void hub_online_merge(const mgx_spmm_plan* plan, int H, int F, const float* er, const float* partial, const float* pstat, float* out,
                             float* stat, hipStream_t s) {
  hipLaunchKernelGGL(hub_online_merge_kernel<KEEP_NAN>, hub_grid(plan), dim3(kBlock), 0, s, plan->hub_row, plan->hub_slot_ptr,
                     plan->num_hubs, H, F, er, partial, pstat, out, stat);
}

}  // namespace mgx
