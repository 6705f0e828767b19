// spmm_rel.hip -- multi-relation g-SpMM: all R relations of an [nnz, R] edge-weight matrix in ONE walk of the graph.
//
// The edge-weighted relational layer of main_dgl_proteins_rgcn_for.py:46-60 runs update_all(u_mul_e, mean) once per relation with an
// [E, 1] weight column: R launches that re-read the same index and re-gather the same source rows, each fetching its weight by edge id
// out of a strided column.  Here:
//
//   forward   out[v, r, d] = dst_scale[v] * SUM | MEAN_{p in row v} W[p, r] * src_scale[u_p] * X[u_p, d]
//   reverse   dX[u, d]     = src_scale[u] * SUM_{p in row u} SUM_r W[p, r] * dst_scale[v_p] * dZ[v_p, r, d]      (on the transposed CSR)
//
// W is [nnz, R] in the CSR's own POSITION order (the caller permutes the edge-id ordered matrix once: mgx_gather_rows with idx = eids), so
// an edge's R weights are one contiguous 4R-byte read that streams along the row; offsets into W are 64-bit ([79.1 M, 8] fp32 is 2.53 GB).
//
// Schedule: a wave per work item (a row, or a chunk of a split row: mgx_spmm_plan).  A feature row of D columns is covered by G = D / VEC
// lanes (VEC = min(D, 4) floats each), the wave's 64 / G lane groups take the item's edges round-robin, and every lane keeps ALL relations of
// its columns: R x VEC accumulators (at most 64 registers) whatever D is.  The index, the weights and the gathered row are read once per
// edge.  At the end the lane groups are summed by an xor butterfly (a fixed tree) and group 0 writes the R rows.  No atomics; the order of
// additions is a function of (graph, plan, R, D) only, so two runs give the same bits.  Split rows go through the plan's partial slots and
// a fix-up pass in slot order, as in spmm.hip.
#include "common.h"

namespace mgx {
namespace {

constexpr int kRelItemsPerBlock = 16;  // as spmm.hip's kItemsPerBlock: a tight window of the schedule per XCD
constexpr int kRelMaxR = 16;

template <typename Idx>
struct RelArgs {
  const Idx* indptr;
  const Idx* indices;
  const float* w;       // [nnz, R], position order
  const float* g;       // gathered matrix: X [num_cols, D] (row stride ldg) or dZ [num_cols, R * D]
  const float* gscale;  // optional factor per gathered row
  const float* rscale;  // optional factor per output row
  float* out;           // [num_rows, R * D] (forward) or [num_rows, D] (reverse)
  const int32_t* item_row;  // optional schedule, as SpmmFastArgs
  const Idx* item_beg;
  const Idx* item_end;
  float* partial;
  int64_t n_items;
  int64_t nblocks;  // multiple of kXcds
  int64_t ldg;
  int R, D;
  int glog;   // log2(G), G = lanes per feature row
  int mean;
  int wvec;   // W rows are whole, 16-byte aligned float4s (R % 4 == 0)
};

template <int RP>
__device__ __forceinline__ void load_weights(const float* __restrict__ w, int64_t q, int R, int wvec, float (&out)[RP]) {
  const float* row = w + q * (int64_t)R;  // 64-bit offset
  if constexpr (RP >= 4) {
    if (wvec) {
#pragma unroll
      for (int r = 0; r < RP; r += 4) {
        v4f t = (v4f)(0.f);
        if (r < R) t = *reinterpret_cast<const v4f*>(row + r);
        out[r] = t.x; out[r + 1] = t.y; out[r + 2] = t.z; out[r + 3] = t.w;
      }
      return;
    }
  }
#pragma unroll
  for (int r = 0; r < RP; ++r) out[r] = r < R ? row[r] : 0.f;
}

template <int RP, int VEC, bool REVERSE>
struct RelUnroll {
  // edges in flight per lane group: bounded by the registers the gathered values take (forward: VEC, reverse: RP * VEC per edge)
  static constexpr int value = REVERSE ? (RP * VEC >= 64 ? 1 : (RP * VEC >= 32 ? 2 : 4)) : (RP * VEC >= 64 ? 2 : 4);
};

template <typename Idx>
__device__ __forceinline__ bool rel_item(const RelArgs<Idx>& a, int64_t item, int64_t& row, int64_t& beg, int64_t& end) {
  if (item >= a.n_items) return false;
  if (a.item_row) {
    row = (int64_t)a.item_row[item];
    beg = (int64_t)a.item_beg[item];
    end = (int64_t)a.item_end[item];
  } else {
    row = item;
    beg = (int64_t)a.indptr[item];
    end = (int64_t)a.indptr[item + 1];
  }
  return true;
}

// ---- forward: R * VEC accumulators per lane -------------------------------------------------------------------------------------------
template <typename Idx, int VEC, int RP>
__global__ __launch_bounds__(kBlock) void spmm_rel_fwd_kernel(const RelArgs<Idx> a) {
  typedef typename VecT<VEC>::type V;
  constexpr int U = RelUnroll<RP, VEC, false>::value;
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int G = 1 << a.glog, NB = kWave >> a.glog;
  const int sub = lane >> a.glog;
  const int f = (lane & (G - 1)) * VEC;
  const int R = a.R;
  const int64_t out_len = (int64_t)R * a.D;
  const int64_t item_base = xcd_remap(blockIdx.x, a.nblocks) * kRelItemsPerBlock;

  for (int it = wave; it < kRelItemsPerBlock; it += kWavesPerBlock) {
    int64_t row = 0, beg = 0, end = 0;
    if (!rel_item(a, item_base + it, row, beg, end)) break;  // wave-uniform
    V acc[RP];
#pragma unroll
    for (int r = 0; r < RP; ++r) acc[r] = (V)(0.f);
    for (int64_t p = beg + sub; p < end; p += (int64_t)NB * U) {
      float s[U];
      V val[U];
      float w[U][RP];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        // positions past the item's end are clamped onto its last edge and weighted 0: every address stays inside the row
        const int64_t q0 = p + (int64_t)u * NB;
        const bool ok = q0 < end;
        const int64_t q = ok ? q0 : end - 1;
        const int64_t nbr = (int64_t)a.indices[q];
        s[u] = ok ? (a.gscale ? a.gscale[nbr] : 1.f) : 0.f;
        val[u] = *reinterpret_cast<const V*>(a.g + nbr * a.ldg + f);
        load_weights<RP>(a.w, q, R, a.wvec, w[u]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const V xs = val[u] * s[u];
#pragma unroll
        for (int r = 0; r < RP; ++r) acc[r] += xs * w[u][r];
      }
    }
    for (int off = G; off < kWave; off <<= 1) {  // lane groups summed by a fixed tree
#pragma unroll
      for (int r = 0; r < RP; ++r) acc[r] += vec_shfl_xor<VEC>(acc[r], off);
    }
    if (sub == 0) {
      if (row >= 0) {
        float scale = a.rscale ? a.rscale[row] : 1.f;
        const int64_t deg = end - beg;
        const float fdeg = (float)(deg > 1 ? deg : 1);
        float* o = a.out + row * out_len + f;
#pragma unroll
        for (int r = 0; r < RP; ++r) {
          if (r < R) {
            V v = acc[r];
            if (a.mean) v = v / fdeg;
            if (a.rscale) v = v * scale;
            *reinterpret_cast<V*>(o + (int64_t)r * a.D) = v;
          }
        }
      } else {  // chunk of a split row: mean / scale are applied by the fix-up pass
        float* o = a.partial + (-(row + 1)) * out_len + f;
#pragma unroll
        for (int r = 0; r < RP; ++r)
          if (r < R) *reinterpret_cast<V*>(o + (int64_t)r * a.D) = acc[r];
      }
    }
  }
}

// ---- reverse: gathers [R * D] rows of dZ, contracts over r in registers ---------------------------------------------------------------
template <typename Idx, int VEC, int RP>
__global__ __launch_bounds__(kBlock) void spmm_rel_grad_kernel(const RelArgs<Idx> a) {
  typedef typename VecT<VEC>::type V;
  constexpr int U = RelUnroll<RP, VEC, true>::value;
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int G = 1 << a.glog, NB = kWave >> a.glog;
  const int sub = lane >> a.glog;
  const int f = (lane & (G - 1)) * VEC;
  const int R = a.R;
  const int64_t item_base = xcd_remap(blockIdx.x, a.nblocks) * kRelItemsPerBlock;

  for (int it = wave; it < kRelItemsPerBlock; it += kWavesPerBlock) {
    int64_t row = 0, beg = 0, end = 0;
    if (!rel_item(a, item_base + it, row, beg, end)) break;  // wave-uniform
    V acc = (V)(0.f);
    for (int64_t p = beg + sub; p < end; p += (int64_t)NB * U) {
      float s[U];
      V val[U][RP];
      float w[U][RP];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t q0 = p + (int64_t)u * NB;
        const bool ok = q0 < end;
        const int64_t q = ok ? q0 : end - 1;  // clamped and weighted 0, as in the forward
        const int64_t nbr = (int64_t)a.indices[q];
        s[u] = ok ? (a.gscale ? a.gscale[nbr] : 1.f) : 0.f;
        const float* grow = a.g + nbr * a.ldg + f;
#pragma unroll
        for (int r = 0; r < RP; ++r) {
          val[u][r] = (V)(0.f);
          if (r < R) val[u][r] = *reinterpret_cast<const V*>(grow + (int64_t)r * a.D);
        }
        load_weights<RP>(a.w, q, R, a.wvec, w[u]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int r = 0; r < RP; ++r) acc += val[u][r] * (w[u][r] * s[u]);
      }
    }
    for (int off = G; off < kWave; off <<= 1) acc += vec_shfl_xor<VEC>(acc, off);
    if (sub == 0) {
      if (row >= 0) {
        if (a.rscale) acc = acc * a.rscale[row];
        *reinterpret_cast<V*>(a.out + row * (int64_t)a.D + f) = acc;
      } else {
        *reinterpret_cast<V*>(a.partial + (-(row + 1)) * (int64_t)a.D + f) = acc;
      }
    }
  }
}

// Partial slots of every split row added in slot order, then the mean / row-scale epilogue.  One wave per split row.
template <typename Idx>
__global__ __launch_bounds__(kBlock) void spmm_rel_fixup_kernel(const Idx* indptr, const int32_t* hub_row, const int32_t* hub_slot_ptr,
                                                                int64_t num_hubs, const float* partial, const float* rscale, float* out,
                                                                int64_t len, int mean) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t h = (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
  if (h >= num_hubs) return;
  const int64_t row = hub_row[h];
  const int s0 = hub_slot_ptr[h], s1 = hub_slot_ptr[h + 1];
  for (int64_t k = lane; k < len; k += kWave) {
    float acc = 0.f;
    for (int s = s0; s < s1; ++s) acc += partial[(int64_t)s * len + k];
    if (mean) {
      const int64_t deg = (int64_t)indptr[row + 1] - (int64_t)indptr[row];
      acc = acc / (float)(deg > 1 ? deg : 1);
    }
    if (rscale) acc *= rscale[row];
    out[row * len + k] = acc;
  }
}

template <typename Idx, int VEC, bool REVERSE>
static void launch_rel_rp(const RelArgs<Idx>& a, hipStream_t s) {
  const dim3 grid((unsigned)a.nblocks), block(kBlock);
#define MGX_REL_CASE(RP_)                                                                               \
  if (REVERSE) hipLaunchKernelGGL((spmm_rel_grad_kernel<Idx, VEC, RP_>), grid, block, 0, s, a);       \
  else hipLaunchKernelGGL((spmm_rel_fwd_kernel<Idx, VEC, RP_>), grid, block, 0, s, a)
  if (a.R <= 1) { MGX_REL_CASE(1); }
  else if (a.R <= 2) { MGX_REL_CASE(2); }
  else if (a.R <= 4) { MGX_REL_CASE(4); }
  else if (a.R <= 8) { MGX_REL_CASE(8); }
  else { MGX_REL_CASE(16); }
#undef MGX_REL_CASE
}

static bool rel_width_supported(int64_t D) { return D >= 1 && D <= 128 && (D & (D - 1)) == 0; }

template <typename Idx, bool REVERSE>
static int32_t spmm_rel_impl(const char* name, const mgx_csr* csr, const mgx_spmm_plan* plan, int mean, int64_t R, int64_t D, const float* w,
                             const float* g, int64_t ldg, const float* gscale, const float* rscale, float* out, float* partial_ws,
                             hipStream_t s) {
  const int64_t n_rows = csr->num_rows;
  if (n_rows == 0) return MGX_OK;
  RelArgs<Idx> a;
  a.indptr = (const Idx*)csr->indptr; a.indices = (const Idx*)csr->indices; a.w = w; a.g = g; a.gscale = gscale; a.rscale = rscale;
  a.out = out; a.item_row = nullptr; a.item_beg = nullptr; a.item_end = nullptr; a.partial = nullptr; a.n_items = n_rows;
  a.ldg = ldg; a.R = (int)R; a.D = (int)D; a.mean = mean;
  a.wvec = (R % 4 == 0 && (uintptr_t)w % 16 == 0) ? 1 : 0;
  if (plan) {
    MGX_CHECK_ARG(!plan->rest, "%s: two-part plans are for the copy_u / copy_e kernels", name);
    MGX_CHECK_ARG(plan->num_items >= n_rows && plan->item_row && plan->item_beg && plan->item_end, "%s: malformed plan", name);
    MGX_CHECK_ARG(plan->num_slots == 0 || (partial_ws && plan->hub_row && plan->hub_slot_ptr),
                  "%s: plan has split rows but no partial workspace / hub tables", name);
    MGX_CHECK_ARG(n_rows < (int64_t(1) << 31), "%s: plans need fewer than 2^31 rows", name);
    a.item_row = plan->item_row; a.item_beg = (const Idx*)plan->item_beg; a.item_end = (const Idx*)plan->item_end;
    a.partial = partial_ws; a.n_items = plan->num_items;
  }
  a.nblocks = round_up((a.n_items + kRelItemsPerBlock - 1) / kRelItemsPerBlock, kXcds);
  MGX_CHECK_ARG(a.nblocks < (int64_t(1) << 31), "%s: too many work items (%lld)", name, (long long)a.n_items);
  const int vec = D >= 4 ? 4 : (int)D;
  a.glog = ilog2_ceil(D / vec);
  note_spmm_kernel(REVERSE ? "rel_grad" : "rel");
  if (vec == 4) launch_rel_rp<Idx, 4, REVERSE>(a, s);
  else if (vec == 2) launch_rel_rp<Idx, 2, REVERSE>(a, s);
  else launch_rel_rp<Idx, 1, REVERSE>(a, s);
  MGX_CHECK_LAUNCH();
  if (plan && plan->num_hubs > 0) {
    hipLaunchKernelGGL((spmm_rel_fixup_kernel<Idx>), dim3((unsigned)((plan->num_hubs + kWavesPerBlock - 1) / kWavesPerBlock)), dim3(kBlock), 0,
                       s, a.indptr, plan->hub_row, plan->hub_slot_ptr, plan->num_hubs, (const float*)partial_ws, rscale, out,
                       REVERSE ? D : R * D, mean);
    MGX_CHECK_LAUNCH();
  }
  return MGX_OK;
}

// the checks both entry points share; MGX_OK = go on
static int32_t rel_check(const char* name, const mgx_csr* csr, int64_t R, int64_t D, const float* w, const float* g, const float* out,
                         int64_t ldg, int64_t g_len) {
  MGX_CHECK_ARG(csr != nullptr, "%s: csr is NULL", name);
  MGX_CHECK_ARG(csr->idx_bits == 32 || csr->idx_bits == 64, "%s: idx_bits must be 32 or 64, got %d", name, csr->idx_bits);
  MGX_CHECK_ARG(csr->num_rows >= 0 && csr->num_cols >= 0 && csr->nnz >= 0, "%s: negative sizes", name);
  MGX_CHECK_ARG(R >= 1 && D >= 1, "%s: R and D must be positive, got %lld and %lld", name, (long long)R, (long long)D);
  MGX_CHECK_ARG(csr->num_rows == 0 || csr->indptr != nullptr, "%s: indptr is NULL", name);
  MGX_CHECK_ARG(csr->nnz == 0 || (csr->indices != nullptr && w != nullptr && g != nullptr), "%s: indices / w / gathered matrix is NULL", name);
  MGX_CHECK_ARG(out != nullptr || csr->num_rows == 0, "%s: out is NULL", name);
  MGX_CHECK_ARG(ldg >= g_len, "%s: row stride %lld below the row length %lld", name, (long long)ldg, (long long)g_len);
  if (R > kRelMaxR || !rel_width_supported(D))
    MGX_UNSUPPORTED("%s: 1 <= R <= 16 and D a power of two up to 128, got R = %lld, D = %lld", name, (long long)R, (long long)D);
  if (D >= 4 && ((uintptr_t)g % 16 != 0 || (uintptr_t)out % 16 != 0 || ldg % 4 != 0))
    MGX_UNSUPPORTED("%s: 16-byte aligned operands and a row stride that is a multiple of 4", name);
  if (D == 2 && ((uintptr_t)g % 8 != 0 || (uintptr_t)out % 8 != 0 || ldg % 2 != 0))
    MGX_UNSUPPORTED("%s: 8-byte aligned operands and an even row stride", name);
  return MGX_OK;
}

}  // namespace
}  // namespace mgx

extern "C" int32_t mgx_spmm_rel(const mgx_csr* csr, const mgx_spmm_plan* plan, int32_t reduce, int64_t R, int64_t D, const float* w,
                                const float* x, int64_t x_stride, const float* src_scale, const float* dst_scale, float* out,
                                float* partial_ws, void* stream) {
  using namespace mgx;
  MGX_ENTER();
  MGX_CHECK_ARG(reduce == MGX_REDUCE_SUM || reduce == MGX_REDUCE_MEAN, "mgx_spmm_rel: SUM or MEAN only, got %d", reduce);
  const int32_t st = rel_check("mgx_spmm_rel", csr, R, D, w, x, out, x_stride, D);
  if (st != MGX_OK) return st;
  const int mean = reduce == MGX_REDUCE_MEAN;
  if (csr->idx_bits == 32)
    return spmm_rel_impl<int32_t, false>("mgx_spmm_rel", csr, plan, mean, R, D, w, x, x_stride, src_scale, dst_scale, out, partial_ws,
                                         (hipStream_t)stream);
  return spmm_rel_impl<int64_t, false>("mgx_spmm_rel", csr, plan, mean, R, D, w, x, x_stride, src_scale, dst_scale, out, partial_ws,
                                       (hipStream_t)stream);
}

extern "C" int32_t mgx_spmm_rel_grad(const mgx_csr* csr, const mgx_spmm_plan* plan, int64_t R, int64_t D, const float* w, const float* dz,
                                     const float* dst_scale, const float* src_scale, float* dx, float* partial_ws, void* stream) {
  using namespace mgx;
  MGX_ENTER();
  const int32_t st = rel_check("mgx_spmm_rel_grad", csr, R, D, w, dz, dx, R * D, R * D);
  if (st != MGX_OK) return st;
  if (csr->idx_bits == 32)
    return spmm_rel_impl<int32_t, true>("mgx_spmm_rel_grad", csr, plan, 0, R, D, w, dz, R * D, dst_scale, src_scale, dx, partial_ws,
                                        (hipStream_t)stream);
  return spmm_rel_impl<int64_t, true>("mgx_spmm_rel_grad", csr, plan, 0, R, D, w, dz, R * D, dst_scale, src_scale, dx, partial_ws,
                                      (hipStream_t)stream);
}
