// gine.hip -- sum aggregation of relu(x_u + w_e) messages with no E-sized temporary (gfx950 / MI355X).
//
// Replaces what a Python UDF message `s * relu(src.x + edge.w)` reduced with fn.sum runs (main_dgl_molhiv_gcn.py:37-52,
// main_dgl_ppa_gcn.py:44-51; with s = 1 upstream's dgl.nn.GINEConv) -- two per-edge gathers, add / relu / mul over [E, D] tensors,
// a copy_e / sum g-SpMM -- and its backward:
//
//   out[v,:] = sum_{e: u -> v} s[e] * relu(x[u,:] + w[e,:])          w, s by EDGE ID; s NULL = 1; a row without in-edges is 0
//
//   forward   gine_kernel<G, false>  ONE walk of the in-CSR: gathers x[indices[p]] and w[eid(p)], eid(p) = eids[p] (p when eids is NULL)
//   backward  gine_kernel<G, true>   ONE walk of the out-CSR (rows = sources; every edge is met exactly once there):
//                                    m = s[e] * 1[x[u] + w[e] > 0] * d out[v],  d w[e] = m (one store per edge),  d x[u] = sum_e m
// The mask is recomputed: fp32 x + w is one rounding, so both walks see the same sign; nothing but x, w and s is kept between them.
// relu'(0) = 0.  A NaN in x[u,c] + w[e,c] reaches out[v,c] (the select below keeps it; fmaxf would drop it) and no other element.
//
// Laid out like dot_attn_kernel (dotattn.hip): one wave per work item of the mgx_spmm_plan (plan_walk.h: items, hub slots, hub merge),
// G lanes ALONG the row with 16-byte accesses (lanes past D / 4 of a group idle when D / 4 is no power of two), 64 / G edges per
// wave-instruction, source and edge ids and scales loaded 64 at a time ahead of the row gathers and handed out by ds_bpermute as
// 32-bit byte offsets.  Lane groups are merged in a fixed order, hub chunks in slot order: no atomics, a rerun is bitwise equal.
#include "plan_walk.h"

namespace mgx {

struct GineArgs {
  PlanItems plan;
  const int32_t* eids;  // [nnz] or NULL (= positions)
  int D;
  const float* x;       // [sources, D]
  const float* w;       // [nnz, D] by edge id
  const float* scale;   // [nnz] by edge id, or NULL
  const float* dout;    // BWD: [destinations, D]
  float* o;             // FWD: out [rows, D]; BWD: d x [rows, D] or NULL
  float* dw;            // BWD: [nnz, D] by edge id, or NULL
  float* partial;       // [slots, D]
};

// G lanes cover one row of D floats (16 bytes each).  FWD gathers x[indices[p]] and w[eid]; BWD holds x[row] and gathers
// d out[indices[p]] and w[eid].
template <int G, bool BWD>
__global__ __launch_bounds__(kBlock) void gine_kernel(const GineArgs a) {
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
  const char* __restrict__ gn = reinterpret_cast<const char*>(BWD ? a.dout : a.x);  // gathered by node id
  const char* __restrict__ gw = reinterpret_cast<const char*>(a.w);                 // gathered by edge id
  char* __restrict__ gdw = reinterpret_cast<char*>(a.dw);
  int64_t item_base, item_stop;
  plan_block_items(a.plan, item_base, item_stop);

  for (int r = wave; r < a.plan.rpb; r += kWavesPerBlock) {
    const int64_t item = item_base + r;
    if (item >= item_stop) break;
    const PlanItem it = plan_item(a.plan, item);
    const int64_t row = it.row, irow = it.irow;
    const int32_t beg = it.beg, end = it.end;
    v4f xr = (v4f)(0.f);  // BWD: x[u], loaded once per work item
    if (BWD && fact) xr = *reinterpret_cast<const v4f*>(a.x + row * D + f);
    v4f acc = (v4f)(0.f);

    for (int32_t cbase = beg; cbase < end; cbase += kWave) {
      const int32_t p = cbase + lane;
      uint32_t noff = 0, woff = 0;
      float sc = 1.f;
      if (p < end) {
        const uint32_t nid = (uint32_t)__builtin_nontemporal_load(&a.plan.indices[p]);
        const uint32_t eid = a.eids ? (uint32_t)__builtin_nontemporal_load(&a.eids[p]) : (uint32_t)p;
        noff = nid * rbytes;
        woff = eid * rbytes;
        if (a.scale) sc = a.scale[eid];
      }
      const int cnt = (end - cbase) < kWave ? (end - cbase) : kWave;
      for (int j = 0; j < cnt; j += STEP) {
        v4f vn[U], vw[U];
        float vs[U];
        uint32_t wo[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int jdx = j + u * NB + sub;
          const int bi = (jdx < cnt ? jdx : 0) * 4;  // lanes past the end re-read edge 0 of the chunk (valid memory), never added or stored
          wo[u] = (uint32_t)__builtin_amdgcn_ds_bpermute(bi, (int)woff) + f4;
          vn[u] = *reinterpret_cast<const v4f*>(gn + (uint32_t)__builtin_amdgcn_ds_bpermute(bi, (int)noff) + f4);
          vw[u] = *reinterpret_cast<const v4f*>(gw + wo[u]);
          vs[u] = __int_as_float(__builtin_amdgcn_ds_bpermute(bi, __float_as_int(sc)));
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const bool live = j + u * NB + sub < cnt;
          const v4f t = (BWD ? xr : vn[u]) + vw[u];
          v4f m;
          if (BWD) {  // relu'(0) = 0; a NaN compares false
            m.x = t.x > 0.f ? vs[u] * vn[u].x : 0.f;
            m.y = t.y > 0.f ? vs[u] * vn[u].y : 0.f;
            m.z = t.z > 0.f ? vs[u] * vn[u].z : 0.f;
            m.w = t.w > 0.f ? vs[u] * vn[u].w : 0.f;
            if (live && fact && gdw) *reinterpret_cast<v4f*>(gdw + wo[u]) = m;
          } else {    // relu that keeps a NaN
            m.x = vs[u] * ((t.x > 0.f || t.x != t.x) ? t.x : 0.f);
            m.y = vs[u] * ((t.y > 0.f || t.y != t.y) ? t.y : 0.f);
            m.z = vs[u] * ((t.z > 0.f || t.z != t.z) ? t.z : 0.f);
            m.w = vs[u] * ((t.w > 0.f || t.w != t.w) ? t.w : 0.f);
          }
          if (live) acc += m;
        }
      }
    }
    // ---- combine the lane groups in a fixed order, write the row (or the partial slot of a hub chunk)
#pragma unroll
    for (int off = G; off < kWave; off <<= 1) acc += vec_shfl_xor<4>(acc, off);
    if (fact && sub == 0 && a.o)
      *reinterpret_cast<v4f*>(irow >= 0 ? a.o + row * (int64_t)D + f : a.partial + plan_slot(irow) * (int64_t)D + f) = acc;
  }
}

template <bool BWD>
static bool gine_launch(const GineArgs& a, hipStream_t s) {
  const dim3 grid((unsigned)a.plan.nblocks), block(kBlock);
  switch (row_walk_lanes(a.D)) {
#define MGX_GINE_G(g) case g: hipLaunchKernelGGL((gine_kernel<g, BWD>), grid, block, 0, s, a); return true;
    MGX_GINE_G(1) MGX_GINE_G(2) MGX_GINE_G(4) MGX_GINE_G(8) MGX_GINE_G(16) MGX_GINE_G(32) MGX_GINE_G(64)
#undef MGX_GINE_G
    default: return false;
  }
}

static void gine_fill(GineArgs& a, const mgx_csr* csr, const mgx_spmm_plan* plan, int64_t D, const float* x, const float* w,
                      const float* scale, void* workspace) {
  memset(&a, 0, sizeof(a));
  plan_items_fill(a.plan, csr, plan, kPlanRowsPerBlock);
  a.eids = (const int32_t*)csr->eids;
  a.D = (int)D;
  a.x = x; a.w = w; a.scale = scale;
  a.partial = (float*)workspace;
}

}  // namespace mgx

extern "C" int32_t mgx_gine_supported(const mgx_csr* csr, int64_t D) {
  using namespace mgx;
  return row_walk_supported(csr, D);
}

extern "C" int64_t mgx_gine_workspace(const mgx_spmm_plan* plan, int64_t D) {
  return (plan ? plan->num_slots : 0) * D * (int64_t)sizeof(float);  // [slots, D] partial rows of out (forward) or d x (backward)
}

extern "C" int32_t mgx_gine_fwd(const mgx_csr* csc, const mgx_spmm_plan* plan, int64_t D, const float* x, const float* w, const float* scale,
                                float* out, void* workspace, void* stream) {
  using namespace mgx;
  MGX_ENTER();
  int32_t st = row_walk_check(csc, plan, D, "mgx_gine_fwd");
  if (st != MGX_OK) return st;
  MGX_CHECK_ARG(x && w && out, "mgx_gine_fwd: NULL pointer");
  MGX_CHECK_ARG(row_aligned16(x) && row_aligned16(w) && row_aligned16(out), "mgx_gine_fwd: x, w and out must be 16-byte aligned");
  const bool hubs = plan && plan->num_slots > 0;
  MGX_CHECK_ARG(!hubs || (workspace && row_aligned16(workspace)), "mgx_gine_fwd: plan has split rows but no 16-byte aligned workspace");
  hipStream_t s = (hipStream_t)stream;
  GineArgs a;
  gine_fill(a, csc, plan, D, x, w, scale, workspace);
  a.o = out;
  if (!gine_launch<false>(a, s)) MGX_UNSUPPORTED("mgx_gine_fwd: unsupported width");
  MGX_CHECK_LAUNCH();
  if (hubs) {
    hub_rows_sum(plan, (int)D, a.partial, out, s);
    MGX_CHECK_LAUNCH();
  }
  note_spmm_kernel("gine_fwd");
  return MGX_OK;
}

extern "C" int32_t mgx_gine_bwd(const mgx_csr* csr, const mgx_spmm_plan* plan, int64_t D, const float* x, const float* w, const float* scale,
                                const float* d_out, float* d_x, float* d_w, void* workspace, void* stream) {
  using namespace mgx;
  MGX_ENTER();
  int32_t st = row_walk_check(csr, plan, D, "mgx_gine_bwd");
  if (st != MGX_OK) return st;
  MGX_CHECK_ARG(x && w && d_out, "mgx_gine_bwd: NULL pointer");
  MGX_CHECK_ARG(row_aligned16(x) && row_aligned16(w) && row_aligned16(d_out) && row_aligned16(d_x) && row_aligned16(d_w),
                "mgx_gine_bwd: x, w, d_out and the gradients must be 16-byte aligned");
  const bool hubs = d_x && plan && plan->num_slots > 0;
  MGX_CHECK_ARG(!hubs || (workspace && row_aligned16(workspace)), "mgx_gine_bwd: plan has split rows but no 16-byte aligned workspace");
  if (!d_x && !d_w) return MGX_OK;
  hipStream_t s = (hipStream_t)stream;
  GineArgs a;
  gine_fill(a, csr, plan, D, x, w, scale, workspace);
  a.dout = d_out; a.o = d_x; a.dw = d_w;
  if (!gine_launch<true>(a, s)) MGX_UNSUPPORTED("mgx_gine_bwd: unsupported width");
  MGX_CHECK_LAUNCH();
  if (hubs) {
    hub_rows_sum(plan, (int)D, a.partial, d_x, s);
    MGX_CHECK_LAUNCH();
  }
  note_spmm_kernel("gine_bwd");
  return MGX_OK;
}
