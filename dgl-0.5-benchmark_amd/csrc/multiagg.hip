// multiagg.hip -- sum / mean / var / std / max / min of the same messages in ONE walk, and all their gradients in one (gfx950 / MI355X).
//
// Replaces the mailbox UDF of Principal Neighbourhood Aggregation (upstream's dgl.nn.PNAConv: mean, max, min and std of one
// message per edge) and what it costs through the generic operators -- five g-SpMM walks forward and five backward, over an [E, D]
// message tensor when the edges carry features:
//
//   m_e = x[u(e),:] (+ w[e,:])            w by EDGE ID, optional;  d = in-degree of v
//   S1 = sum_e m_e   S2 = sum_e m_e^2     sum = S1, mean = S1 / d, msq = S2 / d, var = relu(msq - mean^2) (a NaN stays), std = sqrt(var + eps)
//   max / min / arg_max / arg_min         mgx_spmm_csr's rule: storage order, strict compare, a NaN never wins, the arg is an edge id
//
//   forward   multi_agg_kernel<G, MM, SQ>  ONE walk of the in-CSR, laid out as gine_kernel<G, false> (gine.hip): per lane S1, S2, the
//                                          running max / min and the CSR POSITION of each winner.  Lane groups take interleaved edges,
//                                          so they are merged on (value, position): the larger value, on equal values the smaller
//                                          position -- which is the first edge in storage order.  Positions become edge ids at the end.
//   hub rows  every chunk leaves (S1, S2, max, pos, min, pos) in its slot; multi_agg_hub_kernel merges a row's slots in slot order
//             with the same compare and runs the same epilogue (divide, relu, sqrt, stores).
//   backward  multi_agg_bwd_kernel<G, MM>  ONE walk of the out-CSR, laid out as gine_kernel<G, true>: holds x[u], gathers per edge the
//                                          destination's rows A[v], B[v] (and g_max, arg_max, g_min, arg_min), w[eid];
//                                          d m_e = A[v] + B[v] m_e + g_max[v] 1[arg_max[v] == e] + g_min[v] 1[arg_min[v] == e],
//                                          d w[e] = d m_e (one store per edge), d x[u] = sum_e d m_e (hub sources: slots, hub_rows_sum).
// The per-destination rows are SEPARATE [N_dst, D] matrices: one 32-bit byte offset per edge serves all of them, the args are the
// forward's own outputs, and a call without max / min gathers two rows instead of six.
// No atomics; lane groups in a fixed order, hub chunks in slot order: a rerun is bitwise equal.
#include "plan_walk.h"

namespace mgx {

typedef int v4i __attribute__((ext_vector_type(4)));

struct MultiAggArgs {
  PlanItems plan;
  const int32_t* eids;  // [nnz] or NULL (= positions)
  int D;
  const float* x;       // [sources, D]
  const float* w;       // [nnz, D] by edge id, or NULL
  // ---- forward
  float *o_sum, *o_mean, *o_var, *o_std, *o_max, *o_min;  // each [rows, D] with row stride ld, or NULL
  int64_t ld;
  int32_t *arg_max, *arg_min;  // [rows, D] dense, or NULL
  float* stats;                // [rows, 2, D]: mean, var (when var or std is requested)
  float eps;
  // ---- backward (rows = sources)
  const float *A, *B;          // [destinations, D]; B may be NULL
  const float *g_max, *g_min;  // [destinations, D] or NULL
  const int32_t *a_max, *a_min;
  float* dx;                   // [rows, D] or NULL
  float* dw;                   // [nnz, D] by edge id, or NULL
  float* partial;              // FWD: [slots, 6, D]; BWD: [slots, D]
};

// (value, position) order of the winners of two disjoint sets of edges: the larger value; equal values: the smaller position
#define MGX_TAKE(cmp, c) \
  if (ov.c cmp v.c || (ov.c == v.c && op.c < p.c)) { v.c = ov.c; p.c = op.c; }
__device__ __forceinline__ void take_max(v4f& v, v4i& p, const v4f ov, const v4i op) {
  MGX_TAKE(>, x) MGX_TAKE(>, y) MGX_TAKE(>, z) MGX_TAKE(>, w)
}
__device__ __forceinline__ void take_min(v4f& v, v4i& p, const v4f ov, const v4i op) {
  MGX_TAKE(<, x) MGX_TAKE(<, y) MGX_TAKE(<, z) MGX_TAKE(<, w)
}
#undef MGX_TAKE
__device__ __forceinline__ v4i shfl_xor_i4(v4i v, int mask) {
  v4i r;
  r.x = __shfl_xor(v.x, mask, kWave); r.y = __shfl_xor(v.y, mask, kWave);
  r.z = __shfl_xor(v.z, mask, kWave); r.w = __shfl_xor(v.w, mask, kWave);
  return r;
}
__device__ __forceinline__ float relu_keep_nan(float t) { return (t > 0.f || t != t) ? t : 0.f; }

// the row epilogue of a lane's four columns: d = the row's in-degree
template <bool MM, bool SQ>
__device__ __forceinline__ void multi_agg_store(const MultiAggArgs& a, int64_t row, int f, int32_t d, v4f s1, v4f s2, v4f mx, v4i pmx,
                                                v4f mn, v4i pmn) {
  const int D = a.D;
  const bool none = d <= 0;  // a destination without in-edges: 0 everywhere, arg -1
  const float fd = (float)d;
  const int64_t at = row * a.ld + f;
  v4f mean = s1 / fd;
  if (none) { s1 = (v4f)(0.f); mean = (v4f)(0.f); }
  if (a.o_sum) *reinterpret_cast<v4f*>(a.o_sum + at) = s1;
  if (a.o_mean) *reinterpret_cast<v4f*>(a.o_mean + at) = mean;
  if (SQ) {
    const v4f t = s2 / fd - mean * mean;
    v4f var, sd;
    var.x = relu_keep_nan(t.x); var.y = relu_keep_nan(t.y); var.z = relu_keep_nan(t.z); var.w = relu_keep_nan(t.w);
    if (none) var = (v4f)(0.f);
    sd.x = sqrtf(var.x + a.eps); sd.y = sqrtf(var.y + a.eps); sd.z = sqrtf(var.z + a.eps); sd.w = sqrtf(var.w + a.eps);
    if (none) sd = (v4f)(0.f);
    *reinterpret_cast<v4f*>(a.stats + row * 2 * (int64_t)D + f) = mean;
    *reinterpret_cast<v4f*>(a.stats + row * 2 * (int64_t)D + D + f) = var;
    if (a.o_var) *reinterpret_cast<v4f*>(a.o_var + at) = var;
    if (a.o_std) *reinterpret_cast<v4f*>(a.o_std + at) = sd;
  }
  if (MM) {
    if (none) { mx = (v4f)(0.f); mn = (v4f)(0.f); }
    if (a.eids) {  // positions -> edge ids
      pmx.x = pmx.x < 0 ? -1 : a.eids[pmx.x]; pmx.y = pmx.y < 0 ? -1 : a.eids[pmx.y];
      pmx.z = pmx.z < 0 ? -1 : a.eids[pmx.z]; pmx.w = pmx.w < 0 ? -1 : a.eids[pmx.w];
      pmn.x = pmn.x < 0 ? -1 : a.eids[pmn.x]; pmn.y = pmn.y < 0 ? -1 : a.eids[pmn.y];
      pmn.z = pmn.z < 0 ? -1 : a.eids[pmn.z]; pmn.w = pmn.w < 0 ? -1 : a.eids[pmn.w];
    }
    if (a.o_max) *reinterpret_cast<v4f*>(a.o_max + at) = mx;
    if (a.o_min) *reinterpret_cast<v4f*>(a.o_min + at) = mn;
    if (a.arg_max) *reinterpret_cast<v4i*>(a.arg_max + row * (int64_t)D + f) = pmx;
    if (a.arg_min) *reinterpret_cast<v4i*>(a.arg_min + row * (int64_t)D + f) = pmn;
  }
}

// G lanes cover one row of D floats (16 bytes each); gathers x[indices[p]] and, with w, w[eid(p)].  MM: max / min are wanted; SQ: S2 is.
template <int G, bool MM, bool SQ>
__global__ __launch_bounds__(kBlock) void multi_agg_kernel(const MultiAggArgs a) {
  constexpr int NB = kWave / G;
  constexpr int U = LaneUnroll<G>::value;
  constexpr int STEP = NB * U;
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int sub = lane / G, l = lane % G;
  const int D = a.D;
  const int f = l * 4;
  const bool fact = f < D;
  const uint32_t f4 = fact ? (uint32_t)f * 4u : 0u;  // idle feature lanes re-read the row start, never stored
  const uint32_t rbytes = (uint32_t)D * 4u;
  const char* __restrict__ gn = reinterpret_cast<const char*>(a.x);  // gathered by node id
  const char* __restrict__ gw = reinterpret_cast<const char*>(a.w);  // gathered by edge id (may be NULL)
  int64_t item_base, item_stop;
  plan_block_items(a.plan, item_base, item_stop);

  for (int r = wave; r < a.plan.rpb; r += kWavesPerBlock) {
    const int64_t item = item_base + r;
    if (item >= item_stop) break;
    const PlanItem it = plan_item(a.plan, item);
    const int64_t row = it.row, irow = it.irow;
    const int32_t beg = it.beg, end = it.end;
    v4f s1 = (v4f)(0.f), s2 = (v4f)(0.f);
    v4f mx = (v4f)(-INFINITY), mn = (v4f)(INFINITY);
    v4i pmx = (v4i)(-1), pmn = (v4i)(-1);

    for (int32_t cbase = beg; cbase < end; cbase += kWave) {
      const int32_t p = cbase + lane;
      uint32_t noff = 0, woff = 0;
      if (p < end) {
        const uint32_t nid = (uint32_t)__builtin_nontemporal_load(&a.plan.indices[p]);
        noff = nid * rbytes;
        if (gw) woff = (a.eids ? (uint32_t)__builtin_nontemporal_load(&a.eids[p]) : (uint32_t)p) * rbytes;
      }
      const int cnt = (end - cbase) < kWave ? (end - cbase) : kWave;
      for (int j = 0; j < cnt; j += STEP) {
        v4f vn[U], vw[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int jdx = j + u * NB + sub;
          const int bi = (jdx < cnt ? jdx : 0) * 4;  // lanes past the end re-read edge 0 of the chunk (valid memory), never counted
          vn[u] = *reinterpret_cast<const v4f*>(gn + (uint32_t)__builtin_amdgcn_ds_bpermute(bi, (int)noff) + f4);
          if (gw) vw[u] = *reinterpret_cast<const v4f*>(gw + (uint32_t)__builtin_amdgcn_ds_bpermute(bi, (int)woff) + f4);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int jdx = j + u * NB + sub;
          if (jdx < cnt) {
            const v4f m = gw ? vn[u] + vw[u] : vn[u];
            s1 += m;
            if (SQ) s2 += m * m;
            if (MM) {  // a lane meets its edges in storage order: the strict compare keeps the first of equal values; a NaN compares false
              const int pos = cbase + jdx;
              if (m.x > mx.x) { mx.x = m.x; pmx.x = pos; }
              if (m.y > mx.y) { mx.y = m.y; pmx.y = pos; }
              if (m.z > mx.z) { mx.z = m.z; pmx.z = pos; }
              if (m.w > mx.w) { mx.w = m.w; pmx.w = pos; }
              if (m.x < mn.x) { mn.x = m.x; pmn.x = pos; }
              if (m.y < mn.y) { mn.y = m.y; pmn.y = pos; }
              if (m.z < mn.z) { mn.z = m.z; pmn.z = pos; }
              if (m.w < mn.w) { mn.w = m.w; pmn.w = pos; }
            }
          }
        }
      }
    }
    // ---- combine the lane groups in a fixed order
#pragma unroll
    for (int off = G; off < kWave; off <<= 1) {
      s1 += vec_shfl_xor<4>(s1, off);
      if (SQ) s2 += vec_shfl_xor<4>(s2, off);
      if (MM) {
        const v4f ox = vec_shfl_xor<4>(mx, off), on = vec_shfl_xor<4>(mn, off);
        const v4i opx = shfl_xor_i4(pmx, off), opn = shfl_xor_i4(pmn, off);
        take_max(mx, pmx, ox, opx);
        take_min(mn, pmn, on, opn);
      }
    }
    if (!fact || sub != 0) continue;
    if (irow >= 0) {
      multi_agg_store<MM, SQ>(a, row, f, a.plan.indptr[row + 1] - a.plan.indptr[row], s1, s2, mx, pmx, mn, pmn);
    } else {  // a chunk of a hub row: its slot
      float* slot = a.partial + plan_slot(irow) * 6 * (int64_t)D + f;
      *reinterpret_cast<v4f*>(slot) = s1;
      if (SQ) *reinterpret_cast<v4f*>(slot + D) = s2;
      if (MM) {
        *reinterpret_cast<v4f*>(slot + 2 * D) = mx;
        *reinterpret_cast<v4i*>(slot + 3 * D) = pmx;
        *reinterpret_cast<v4f*>(slot + 4 * D) = mn;
        *reinterpret_cast<v4i*>(slot + 5 * D) = pmn;
      }
    }
  }
}

// one wave per hub row, a lane per four columns: the row's slots in slot order, then the epilogue
template <bool MM, bool SQ>
__global__ __launch_bounds__(kBlock) void multi_agg_hub_kernel(const MultiAggArgs a, const int32_t* hub_row, const int32_t* hub_slot_ptr,
                                                               int64_t n_hubs) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t h = (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
  const int D = a.D, f = lane * 4;
  if (h >= n_hubs || f >= D) return;
  const int64_t row = hub_row[h];
  const int s0 = hub_slot_ptr[h], s_end = hub_slot_ptr[h + 1];
  v4f s1 = (v4f)(0.f), s2 = (v4f)(0.f);
  v4f mx = (v4f)(-INFINITY), mn = (v4f)(INFINITY);
  v4i pmx = (v4i)(-1), pmn = (v4i)(-1);
  for (int s = s0; s < s_end; ++s) {
    const float* slot = a.partial + (int64_t)s * 6 * D + f;
    s1 += *reinterpret_cast<const v4f*>(slot);
    if (SQ) s2 += *reinterpret_cast<const v4f*>(slot + D);
    if (MM) {
      const v4f ox = *reinterpret_cast<const v4f*>(slot + 2 * D), on = *reinterpret_cast<const v4f*>(slot + 4 * D);
      const v4i opx = *reinterpret_cast<const v4i*>(slot + 3 * D), opn = *reinterpret_cast<const v4i*>(slot + 5 * D);
      take_max(mx, pmx, ox, opx);
      take_min(mn, pmn, on, opn);
    }
  }
  multi_agg_store<MM, SQ>(a, row, f, a.plan.indptr[row + 1] - a.plan.indptr[row], s1, s2, mx, pmx, mn, pmn);
}

// edges in flight per lane group in the backward: six gathered rows and w per edge with max / min, so half of the forward's
template <int G, bool MM>
struct BwdUnroll {
  static constexpr int U = LaneUnroll<G>::value;
  static constexpr int value = MM ? (U > 2 ? 2 : U) : U;
};

// rows = sources.  Holds x[row]; gathers A, B (and g_max, arg_max, g_min, arg_min) of indices[p] and w[eid].
template <int G, bool MM>
__global__ __launch_bounds__(kBlock) void multi_agg_bwd_kernel(const MultiAggArgs a) {
  constexpr int NB = kWave / G;
  constexpr int U = BwdUnroll<G, MM>::value;
  constexpr int STEP = NB * U;
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int sub = lane / G, l = lane % G;
  const int D = a.D;
  const int f = l * 4;
  const bool fact = f < D;
  const uint32_t f4 = fact ? (uint32_t)f * 4u : 0u;
  const uint32_t rbytes = (uint32_t)D * 4u;
  const char* __restrict__ gA = reinterpret_cast<const char*>(a.A);
  const char* __restrict__ gB = reinterpret_cast<const char*>(a.B);
  const char* __restrict__ gw = reinterpret_cast<const char*>(a.w);
  const char* __restrict__ ggx = reinterpret_cast<const char*>(a.g_max);
  const char* __restrict__ ggn = reinterpret_cast<const char*>(a.g_min);
  const char* __restrict__ gax = reinterpret_cast<const char*>(a.a_max);
  const char* __restrict__ gan = reinterpret_cast<const char*>(a.a_min);
  char* __restrict__ gdw = reinterpret_cast<char*>(a.dw);
  const bool need_m = gB != nullptr, has_w = need_m && gw != nullptr;
  int64_t item_base, item_stop;
  plan_block_items(a.plan, item_base, item_stop);

  for (int r = wave; r < a.plan.rpb; r += kWavesPerBlock) {
    const int64_t item = item_base + r;
    if (item >= item_stop) break;
    const PlanItem it = plan_item(a.plan, item);
    const int64_t row = it.row, irow = it.irow;
    const int32_t beg = it.beg, end = it.end;
    v4f xr = (v4f)(0.f);
    if (need_m && fact) xr = *reinterpret_cast<const v4f*>(a.x + row * D + f);
    v4f acc = (v4f)(0.f);

    for (int32_t cbase = beg; cbase < end; cbase += kWave) {
      const int32_t p = cbase + lane;
      uint32_t noff = 0;
      int eid = 0;
      if (p < end) {
        noff = (uint32_t)__builtin_nontemporal_load(&a.plan.indices[p]) * rbytes;
        eid = a.eids ? __builtin_nontemporal_load(&a.eids[p]) : p;
      }
      const int cnt = (end - cbase) < kWave ? (end - cbase) : kWave;
      for (int j = 0; j < cnt; j += STEP) {
        v4f vA[U], vB[U], vw[U], vgx[U], vgn[U];
        v4i vax[U], van[U];
        int ve[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int jdx = j + u * NB + sub;
          const int bi = (jdx < cnt ? jdx : 0) * 4;  // lanes past the end re-read edge 0 of the chunk (valid memory), never added or stored
          const uint32_t vo = (uint32_t)__builtin_amdgcn_ds_bpermute(bi, (int)noff) + f4;
          ve[u] = __builtin_amdgcn_ds_bpermute(bi, eid);
          vA[u] = *reinterpret_cast<const v4f*>(gA + vo);
          if (need_m) vB[u] = *reinterpret_cast<const v4f*>(gB + vo);
          if (has_w) vw[u] = *reinterpret_cast<const v4f*>(gw + (uint32_t)ve[u] * rbytes + f4);
          if (MM) {
            if (ggx) { vgx[u] = *reinterpret_cast<const v4f*>(ggx + vo); vax[u] = *reinterpret_cast<const v4i*>(gax + vo); }
            if (ggn) { vgn[u] = *reinterpret_cast<const v4f*>(ggn + vo); van[u] = *reinterpret_cast<const v4i*>(gan + vo); }
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const bool live = j + u * NB + sub < cnt;
          v4f dm = vA[u];
          if (need_m) dm += vB[u] * (has_w ? xr + vw[u] : xr);
          if (MM) {  // a select, not a product: the gradient of a column reaches its one winner and nothing else
            const int e = ve[u];
            if (ggx) {
              dm.x += vax[u].x == e ? vgx[u].x : 0.f; dm.y += vax[u].y == e ? vgx[u].y : 0.f;
              dm.z += vax[u].z == e ? vgx[u].z : 0.f; dm.w += vax[u].w == e ? vgx[u].w : 0.f;
            }
            if (ggn) {
              dm.x += van[u].x == e ? vgn[u].x : 0.f; dm.y += van[u].y == e ? vgn[u].y : 0.f;
              dm.z += van[u].z == e ? vgn[u].z : 0.f; dm.w += van[u].w == e ? vgn[u].w : 0.f;
            }
          }
          if (live && fact && gdw) *reinterpret_cast<v4f*>(gdw + (uint32_t)ve[u] * rbytes + f4) = dm;
          if (live) acc += dm;
        }
      }
    }
#pragma unroll
    for (int off = G; off < kWave; off <<= 1) acc += vec_shfl_xor<4>(acc, off);
    if (fact && sub == 0 && a.dx)
      *reinterpret_cast<v4f*>(irow >= 0 ? a.dx + row * (int64_t)D + f : a.partial + plan_slot(irow) * (int64_t)D + f) = acc;
  }
}

template <bool MM, bool SQ>
static bool multi_agg_launch(const MultiAggArgs& a, hipStream_t s) {
  const dim3 grid((unsigned)a.plan.nblocks), block(kBlock);
  switch (row_walk_lanes(a.D)) {
#define MGX_MAGG_G(g) case g: hipLaunchKernelGGL((multi_agg_kernel<g, MM, SQ>), grid, block, 0, s, a); return true;
    MGX_MAGG_G(1) MGX_MAGG_G(2) MGX_MAGG_G(4) MGX_MAGG_G(8) MGX_MAGG_G(16) MGX_MAGG_G(32) MGX_MAGG_G(64)
#undef MGX_MAGG_G
    default: return false;
  }
}

template <bool MM>
static bool multi_agg_bwd_launch(const MultiAggArgs& a, hipStream_t s) {
  const dim3 grid((unsigned)a.plan.nblocks), block(kBlock);
  switch (row_walk_lanes(a.D)) {
#define MGX_MAGG_G(g) case g: hipLaunchKernelGGL((multi_agg_bwd_kernel<g, MM>), grid, block, 0, s, a); return true;
    MGX_MAGG_G(1) MGX_MAGG_G(2) MGX_MAGG_G(4) MGX_MAGG_G(8) MGX_MAGG_G(16) MGX_MAGG_G(32) MGX_MAGG_G(64)
#undef MGX_MAGG_G
    default: return false;
  }
}

template <bool MM, bool SQ>
static bool multi_agg_fwd_run(const MultiAggArgs& a, const mgx_spmm_plan* plan, bool hubs, hipStream_t s) {
  if (!multi_agg_launch<MM, SQ>(a, s)) return false;
  if (hubs)
    hipLaunchKernelGGL((multi_agg_hub_kernel<MM, SQ>), hub_grid(plan), dim3(kBlock), 0, s, a, plan->hub_row, plan->hub_slot_ptr,
                       plan->num_hubs);
  return true;
}

}  // namespace mgx

extern "C" int32_t mgx_multi_agg_supported(const mgx_csr* csr, int64_t D) {
  using namespace mgx;
  return row_walk_supported(csr, D);
}

extern "C" int64_t mgx_multi_agg_workspace(const mgx_spmm_plan* plan, int64_t D) {
  return (plan ? plan->num_slots : 0) * 6 * D * (int64_t)sizeof(float);  // [slots, 6, D]: S1, S2, max, its position, min, its position
}

extern "C" int32_t mgx_multi_agg_fwd(const mgx_csr* csc, const mgx_spmm_plan* plan, int64_t D, const float* x, const float* w, float eps,
                                     float* o_sum, float* o_mean, float* o_var, float* o_std, float* o_max, float* o_min, int64_t out_ld,
                                     int32_t* arg_max, int32_t* arg_min, float* stats, void* workspace, void* stream) {
  using namespace mgx;
  MGX_ENTER();
  int32_t st = row_walk_check(csc, plan, D, "mgx_multi_agg_fwd");
  if (st != MGX_OK) return st;
  MGX_CHECK_ARG(x && (o_sum || o_mean || o_var || o_std || o_max || o_min), "mgx_multi_agg_fwd: NULL pointer (x, or no aggregate at all)");
  const bool sq = o_var || o_std, mm = o_max || o_min;
  MGX_CHECK_ARG(!sq || stats, "mgx_multi_agg_fwd: NULL pointer (var / std need the statistics buffer)");
  MGX_CHECK_ARG((!arg_max || o_max) && (!arg_min || o_min), "mgx_multi_agg_fwd: an arg without its aggregate");
  MGX_CHECK_ARG(out_ld >= D && out_ld % 4 == 0, "mgx_multi_agg_fwd: out_ld must be a multiple of 4 and at least D (got %lld)", (long long)out_ld);
  MGX_CHECK_ARG(!sq || (eps > 0.f && isfinite(eps)), "mgx_multi_agg_fwd: eps must be positive and finite");
  MGX_CHECK_ARG(row_aligned16(x) && row_aligned16(w) && row_aligned16(o_sum) && row_aligned16(o_mean) && row_aligned16(o_var) && row_aligned16(o_std) && row_aligned16(o_max) && row_aligned16(o_min) &&
                    row_aligned16(arg_max) && row_aligned16(arg_min) && row_aligned16(stats),
                "mgx_multi_agg_fwd: x, w, the aggregates, the args and the statistics must be 16-byte aligned");
  const bool hubs = plan && plan->num_slots > 0;
  MGX_CHECK_ARG(!hubs || (workspace && row_aligned16(workspace)), "mgx_multi_agg_fwd: plan has split rows but no 16-byte aligned workspace");
  hipStream_t s = (hipStream_t)stream;
  MultiAggArgs a;
  memset(&a, 0, sizeof(a));
  plan_items_fill(a.plan, csc, plan, kPlanRowsPerBlock);
  a.eids = (const int32_t*)csc->eids;
  a.D = (int)D;
  a.x = x; a.w = w; a.eps = eps;
  a.o_sum = o_sum; a.o_mean = o_mean; a.o_var = o_var; a.o_std = o_std; a.o_max = o_max; a.o_min = o_min;
  a.ld = out_ld; a.arg_max = arg_max; a.arg_min = arg_min; a.stats = stats;
  a.partial = (float*)workspace;
  const bool ok = mm ? (sq ? multi_agg_fwd_run<true, true>(a, plan, hubs, s) : multi_agg_fwd_run<true, false>(a, plan, hubs, s))
                     : (sq ? multi_agg_fwd_run<false, true>(a, plan, hubs, s) : multi_agg_fwd_run<false, false>(a, plan, hubs, s));
  if (!ok) MGX_UNSUPPORTED("mgx_multi_agg_fwd: unsupported width");
  MGX_CHECK_LAUNCH();
  note_spmm_kernel("multi_agg_fwd");
  return MGX_OK;
}

extern "C" int32_t mgx_multi_agg_bwd(const mgx_csr* csr, const mgx_spmm_plan* plan, int64_t D, const float* x, const float* w, const float* A,
                                     const float* B, const float* g_max, const int32_t* arg_max, const float* g_min, const int32_t* arg_min,
                                     float* d_x, float* d_w, void* workspace, void* stream) {
  using namespace mgx;
  MGX_ENTER();
  int32_t st = row_walk_check(csr, plan, D, "mgx_multi_agg_bwd");
  if (st != MGX_OK) return st;
  MGX_CHECK_ARG(x && A, "mgx_multi_agg_bwd: NULL pointer");
  MGX_CHECK_ARG((g_max != nullptr) == (arg_max != nullptr) && (g_min != nullptr) == (arg_min != nullptr),
                "mgx_multi_agg_bwd: NULL pointer (g_max / g_min come with their args)");
  MGX_CHECK_ARG(row_aligned16(x) && row_aligned16(w) && row_aligned16(A) && row_aligned16(B) && row_aligned16(g_max) && row_aligned16(arg_max) && row_aligned16(g_min) && row_aligned16(arg_min) && row_aligned16(d_x) &&
                    row_aligned16(d_w),
                "mgx_multi_agg_bwd: x, w, the destination rows and the gradients must be 16-byte aligned");
  const bool hubs = d_x && plan && plan->num_slots > 0;
  MGX_CHECK_ARG(!hubs || (workspace && row_aligned16(workspace)), "mgx_multi_agg_bwd: plan has split rows but no 16-byte aligned workspace");
  if (!d_x && !d_w) return MGX_OK;
  hipStream_t s = (hipStream_t)stream;
  MultiAggArgs a;
  memset(&a, 0, sizeof(a));
  plan_items_fill(a.plan, csr, plan, kPlanRowsPerBlock);
  a.eids = (const int32_t*)csr->eids;
  a.D = (int)D;
  a.x = x; a.w = w; a.A = A; a.B = B;
  a.g_max = g_max; a.a_max = arg_max; a.g_min = g_min; a.a_min = arg_min;
  a.dx = d_x; a.dw = d_w;
  a.partial = (float*)workspace;
  const bool ok = (g_max || g_min) ? multi_agg_bwd_launch<true>(a, s) : multi_agg_bwd_launch<false>(a, s);
  if (!ok) MGX_UNSUPPORTED("mgx_multi_agg_bwd: unsupported width");
  MGX_CHECK_LAUNCH();
  if (hubs) {
    hub_rows_sum(plan, (int)D, a.partial, d_x, s);
    MGX_CHECK_LAUNCH();
  }
  note_spmm_kernel("multi_agg_bwd");
  return MGX_OK;
}
