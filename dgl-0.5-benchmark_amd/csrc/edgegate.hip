// edgegate.hip -- edge-gated aggregation (ResGatedGCN, upstream's dgl.nn.GatedGCNConv) with one E-sized tensor each way (gfx950 / MI355X).
//
// Replaces the composition u_add_v -> add -> sigmoid -> u_mul_e / sum -> copy_e / sum -> divide (five [E, F] tensors forward) and its
// backward:
//
//   e_hat[e,:] = (s[u,:] + d[v,:]) + c[e,:]          e: u -> v; c and e_hat by EDGE ID
//   sig        = 1 / (1 + exp(-e_hat))               gate_sigmoid below, the ONE expression all three walks use
//   den[v,:]   = sum_e sig,   h[v,:] = (sum_e sig * b[u,:]) / (den[v,:] + eps)       a row without in-edges: h = den = 0
//
//   forward     edge_gate_fwd_kernel<G>          ONE walk of the in-CSR: holds d[v], gathers s[u], b[u], c[eid], stores e_hat[eid] once,
//                                                keeps the numerator and the denominator in registers, divides in the row epilogue
//   backward 1  edge_gate_bwd_dst_kernel<G, DH>  in-CSR again (rows = destinations): gn = d_h / (den + eps), gd = -gn * h per row,
//                                                t = (gn * b[u] + gd) * sig * (1 - sig) + d_e_hat[eid];  d_c[eid] = t,  d_d[v] = sum_e t;
//                                                leaves gn [N_dst, F].  DH = false (no d_h): t = d_e_hat[eid], nothing else is read
//   backward 2  edge_gate_bwd_src_kernel<G, NB>  out-CSR (rows = sources; every edge is met once): d_s[u] = sum_e d_c[eid],
//                                                d_b[u] = sum_e sig * gn[v].  NB = false (d_b not wanted): e_hat and gn are not read
// sig is recomputed from the stored e_hat bits, so the three walks agree on it; nothing of size E exists but e_hat and d_c, nothing of
// size N but den and gn.
//
// Laid out like gine_kernel (gine.hip): one wave per work item of the mgx_spmm_plan (plan_walk.h), G lanes ALONG the row with 16-byte
// accesses, 64 / G edges per wave-instruction, node and edge ids loaded 64 ahead and handed out by ds_bpermute as 32-bit byte offsets.
// A chunk of a split (hub) row leaves BOTH its sums in its slot, [slots, 2, F]; edge_gate_hub_kernel adds them in slot order and only
// then divides (a quotient per chunk would not sum to the row's).  Lane groups merge in a fixed order: no atomics, a rerun is bitwise equal.
#include "plan_walk.h"

namespace mgx {

struct EdgeGateArgs {
  PlanItems plan;
  const int32_t* eids;  // [nnz] or NULL (= positions)
  int D;
  float eps;
  const float* b;       // [sources, D]
  const float* s;       // [sources, D]
  const float* d;       // [destinations, D]
  const float* c;       // [nnz, D] by edge id
  float* e_hat;         // [nnz, D] by edge id: written forward, read backward
  float* h;             // [destinations, D]: written forward, read backward
  float* den;           // [destinations, D]: written forward, read backward
  const float* dh;      // BWD: [destinations, D] or NULL
  const float* de;      // BWD dst: d e_hat [nnz, D] by edge id, or NULL
  float* gn;            // BWD dst writes, BWD src gathers: [destinations, D]
  float* dc;            // BWD dst writes (or NULL), BWD src reads: [nnz, D] by edge id
  float* o0;            // BWD dst: d d [rows, D] or NULL;  BWD src: d s [rows, D] or NULL
  float* o1;            // BWD src: d b [rows, D] or NULL
  float* partial;       // FWD: [slots, 2, D] (numerator, denominator); BWD dst: [slots, D]; BWD src: [slots, 2, D] (d s, d b)
};

__device__ __forceinline__ float gate_sigmoid1(float x) { return 1.f / (1.f + __expf(-x)); }
__device__ __forceinline__ v4f gate_sigmoid(const v4f x) {
  v4f r;
  r.x = gate_sigmoid1(x.x); r.y = gate_sigmoid1(x.y); r.z = gate_sigmoid1(x.z); r.w = gate_sigmoid1(x.w);
  return r;
}

// the lane geometry every walk below starts from
#define MGX_GATE_LANES                                                                                          \
  constexpr int NB_ = kWave / G;                                                                                \
  constexpr int U = LaneUnroll<G>::value;                                                                       \
  constexpr int STEP = NB_ * U;                                                                                 \
  const int lane = threadIdx.x & (kWave - 1);                                                                   \
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);                                         \
  const int sub = lane / G, l = lane % G;                                                                       \
  const int D = a.D;                                                                                            \
  const int f = l * 4;                                                                                          \
  const bool fact = f < D;                                                                                      \
  const uint32_t f4 = fact ? (uint32_t)f * 4u : 0u; /* idle feature lanes re-read the row start, never stored */ \
  const uint32_t rbytes = (uint32_t)D * 4u;                                                                     \
  int64_t item_base, item_stop;                                                                                 \
  plan_block_items(a.plan, item_base, item_stop)

// node and edge byte offsets of the 64 positions from cbase on, one per lane
#define MGX_GATE_IDS                                                                                                     \
  const int32_t p = cbase + lane;                                                                                        \
  uint32_t noff = 0, eoff = 0;                                                                                           \
  if (p < end) {                                                                                                         \
    noff = (uint32_t)__builtin_nontemporal_load(&a.plan.indices[p]) * rbytes;                                            \
    eoff = (a.eids ? (uint32_t)__builtin_nontemporal_load(&a.eids[p]) : (uint32_t)p) * rbytes;                           \
  }                                                                                                                      \
  const int cnt = (end - cbase) < kWave ? (end - cbase) : kWave

// edge j + u * NB_ + sub of the chunk: its offsets; lanes past the end re-read edge 0 of the chunk (valid memory), never added or stored
#define MGX_GATE_EDGE(u)                                                                       \
  const int jdx = j + (u) * NB_ + sub;                                                         \
  const int bi = (jdx < cnt ? jdx : 0) * 4;                                                    \
  const uint32_t no = (uint32_t)__builtin_amdgcn_ds_bpermute(bi, (int)noff) + f4;              \
  eo[u] = (uint32_t)__builtin_amdgcn_ds_bpermute(bi, (int)eoff) + f4

template <int G>
__device__ __forceinline__ v4f groups_sum(v4f acc) {
#pragma unroll
  for (int off = G; off < kWave; off <<= 1) acc += vec_shfl_xor<4>(acc, off);
  return acc;
}

// ---------------------------------------------------------------------------------------------- forward
template <int G>
__global__ __launch_bounds__(kBlock) void edge_gate_fwd_kernel(const EdgeGateArgs a) {
  MGX_GATE_LANES;
  const char* __restrict__ gb = reinterpret_cast<const char*>(a.b);
  const char* __restrict__ gs = reinterpret_cast<const char*>(a.s);
  const char* __restrict__ gc = reinterpret_cast<const char*>(a.c);
  char* __restrict__ ge = reinterpret_cast<char*>(a.e_hat);

  for (int r = wave; r < a.plan.rpb; r += kWavesPerBlock) {
    const int64_t item = item_base + r;
    if (item >= item_stop) break;
    const PlanItem it = plan_item(a.plan, item);
    const int64_t row = it.row, irow = it.irow;
    const int32_t beg = it.beg, end = it.end;
    v4f dr = (v4f)(0.f);  // d[v], loaded once per work item
    if (fact) dr = *reinterpret_cast<const v4f*>(a.d + row * D + f);
    v4f num = (v4f)(0.f), den = (v4f)(0.f);

    for (int32_t cbase = beg; cbase < end; cbase += kWave) {
      MGX_GATE_IDS;
      for (int j = 0; j < cnt; j += STEP) {
        v4f vs[U], vb[U], vc[U];
        uint32_t eo[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          MGX_GATE_EDGE(u);
          vs[u] = *reinterpret_cast<const v4f*>(gs + no);
          vb[u] = *reinterpret_cast<const v4f*>(gb + no);
          vc[u] = *reinterpret_cast<const v4f*>(gc + eo[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const bool live = j + u * NB_ + sub < cnt;
          const v4f eh = (vs[u] + dr) + vc[u];
          if (live && fact) *reinterpret_cast<v4f*>(ge + eo[u]) = eh;
          const v4f sig = gate_sigmoid(eh);
          if (live) { num += sig * vb[u]; den += sig; }
        }
      }
    }
    num = groups_sum<G>(num);
    den = groups_sum<G>(den);
    if (fact && sub == 0) {
      if (irow >= 0) {  // a whole row: divide here; no in-edges: exactly 0, also with eps = 0
        *reinterpret_cast<v4f*>(a.h + row * (int64_t)D + f) = end > beg ? num / (den + a.eps) : (v4f)(0.f);
        *reinterpret_cast<v4f*>(a.den + row * (int64_t)D + f) = den;
      } else {          // a chunk of a hub row: both sums to the slot, the division waits for the merge
        float* slot = a.partial + plan_slot(irow) * 2 * (int64_t)D + f;
        *reinterpret_cast<v4f*>(slot) = num;
        *reinterpret_cast<v4f*>(slot + D) = den;
      }
    }
  }
}

// A hub row's slots [slot, 2, D] added in slot order.  DIV (forward): h = num / (den + eps) and den; else (backward 2) the two sums to
// o0 / o1, either of which may be NULL.
template <bool DIV>
__global__ __launch_bounds__(kBlock) void edge_gate_hub_kernel(const EdgeGateArgs a, const int32_t* hub_row, const int32_t* hub_slot_ptr,
                                                               int64_t n_hubs) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t hb = (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
  const int D = a.D, f = lane * 4;
  if (hb >= n_hubs || f >= D) return;
  const int64_t row = hub_row[hb];
  const int s0 = hub_slot_ptr[hb], s_end = hub_slot_ptr[hb + 1];
  v4f p0 = (v4f)(0.f), p1 = (v4f)(0.f);
  for (int s = s0; s < s_end; ++s) {
    const float* slot = a.partial + (int64_t)s * 2 * D + f;
    p0 += *reinterpret_cast<const v4f*>(slot);
    p1 += *reinterpret_cast<const v4f*>(slot + D);
  }
  if (DIV) {
    *reinterpret_cast<v4f*>(a.h + row * D + f) = p0 / (p1 + a.eps);
    *reinterpret_cast<v4f*>(a.den + row * D + f) = p1;
  } else {
    if (a.o0) *reinterpret_cast<v4f*>(a.o0 + row * D + f) = p0;
    if (a.o1) *reinterpret_cast<v4f*>(a.o1 + row * D + f) = p1;
  }
}

// ---------------------------------------------------------------------------------------------- backward 1: in-CSR, rows = destinations
template <int G, bool DH>
__global__ __launch_bounds__(kBlock) void edge_gate_bwd_dst_kernel(const EdgeGateArgs a) {
  MGX_GATE_LANES;
  const char* __restrict__ gb = reinterpret_cast<const char*>(a.b);
  const char* __restrict__ ge = reinterpret_cast<const char*>(a.e_hat);
  const char* __restrict__ gde = reinterpret_cast<const char*>(a.de);
  char* __restrict__ gdc = reinterpret_cast<char*>(a.dc);

  for (int r = wave; r < a.plan.rpb; r += kWavesPerBlock) {
    const int64_t item = item_base + r;
    if (item >= item_stop) break;
    const PlanItem it = plan_item(a.plan, item);
    const int64_t row = it.row, irow = it.irow;
    const int32_t beg = it.beg, end = it.end;
    v4f gn = (v4f)(0.f), gd = (v4f)(0.f);
    if (DH && fact && end > beg) {
      const int64_t at = row * D + f;
      gn = *reinterpret_cast<const v4f*>(a.dh + at) / (*reinterpret_cast<const v4f*>(a.den + at) + a.eps);
      gd = -gn * *reinterpret_cast<const v4f*>(a.h + at);
    }
    // gn[v] for backward 2: written by the item that holds the row's first edge (a row without in-edges: 0, read by nobody)
    if (DH && fact && sub == 0 && beg == a.plan.indptr[row]) *reinterpret_cast<v4f*>(a.gn + row * D + f) = gn;
    v4f acc = (v4f)(0.f);

    for (int32_t cbase = beg; cbase < end; cbase += kWave) {
      MGX_GATE_IDS;
      for (int j = 0; j < cnt; j += STEP) {
        v4f vb[U], ve[U], vd[U];
        uint32_t eo[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          MGX_GATE_EDGE(u);
          if (DH) {
            vb[u] = *reinterpret_cast<const v4f*>(gb + no);
            ve[u] = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(ge + eo[u]));
          }
          vd[u] = gde ? __builtin_nontemporal_load(reinterpret_cast<const v4f*>(gde + eo[u])) : (v4f)(0.f);
          (void)no;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const bool live = j + u * NB_ + sub < cnt;
          v4f t = vd[u];
          if (DH) {
            const v4f sig = gate_sigmoid(ve[u]);
            t = (gn * vb[u] + gd) * sig * (1.f - sig) + vd[u];
          }
          if (live && fact && gdc) *reinterpret_cast<v4f*>(gdc + eo[u]) = t;
          if (live) acc += t;
        }
      }
    }
    if (a.o0) {
      acc = groups_sum<G>(acc);
      if (fact && sub == 0)
        *reinterpret_cast<v4f*>(irow >= 0 ? a.o0 + row * (int64_t)D + f : a.partial + plan_slot(irow) * (int64_t)D + f) = acc;
    }
  }
}

// ---------------------------------------------------------------------------------------------- backward 2: out-CSR, rows = sources
template <int G, bool NEED_B>
__global__ __launch_bounds__(kBlock) void edge_gate_bwd_src_kernel(const EdgeGateArgs a) {
  MGX_GATE_LANES;
  const char* __restrict__ ggn = reinterpret_cast<const char*>(a.gn);
  const char* __restrict__ ge = reinterpret_cast<const char*>(a.e_hat);
  const char* __restrict__ gdc = reinterpret_cast<const char*>(a.dc);

  for (int r = wave; r < a.plan.rpb; r += kWavesPerBlock) {
    const int64_t item = item_base + r;
    if (item >= item_stop) break;
    const PlanItem it = plan_item(a.plan, item);
    const int64_t row = it.row, irow = it.irow;
    const int32_t beg = it.beg, end = it.end;
    v4f accs = (v4f)(0.f), accb = (v4f)(0.f);

    for (int32_t cbase = beg; cbase < end; cbase += kWave) {
      MGX_GATE_IDS;
      for (int j = 0; j < cnt; j += STEP) {
        v4f vt[U], ve[U], vg[U];
        uint32_t eo[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          MGX_GATE_EDGE(u);
          vt[u] = gdc ? __builtin_nontemporal_load(reinterpret_cast<const v4f*>(gdc + eo[u])) : (v4f)(0.f);
          if (NEED_B) {
            ve[u] = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(ge + eo[u]));
            vg[u] = *reinterpret_cast<const v4f*>(ggn + no);
          }
          (void)no;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (j + u * NB_ + sub < cnt) {
            accs += vt[u];
            if (NEED_B) accb += gate_sigmoid(ve[u]) * vg[u];
          }
        }
      }
    }
    accs = groups_sum<G>(accs);
    if (NEED_B) accb = groups_sum<G>(accb);
    if (fact && sub == 0) {
      if (irow >= 0) {
        if (a.o0) *reinterpret_cast<v4f*>(a.o0 + row * (int64_t)D + f) = accs;
        if (NEED_B) *reinterpret_cast<v4f*>(a.o1 + row * (int64_t)D + f) = accb;
      } else {
        float* slot = a.partial + plan_slot(irow) * 2 * (int64_t)D + f;
        *reinterpret_cast<v4f*>(slot) = accs;
        *reinterpret_cast<v4f*>(slot + D) = accb;
      }
    }
  }
}

#undef MGX_GATE_LANES
#undef MGX_GATE_IDS
#undef MGX_GATE_EDGE

#define MGX_GATE_LAUNCH(kernel)                                                                                  \
  row_walk_dispatch(a.D, [&](auto g) {                                                                           \
    hipLaunchKernelGGL((kernel), dim3((unsigned)a.plan.nblocks), dim3(kBlock), 0, s, a);                         \
    return true;                                                                                                 \
  })

static void edge_gate_fill(EdgeGateArgs& a, const mgx_csr* csr, const mgx_spmm_plan* plan, int64_t D, float eps, void* workspace) {
  memset(&a, 0, sizeof(a));
  plan_items_fill(a.plan, csr, plan, kPlanRowsPerBlock);
  a.eids = (const int32_t*)csr->eids;
  a.D = (int)D;
  a.eps = eps;
  a.partial = (float*)workspace;
}

static inline bool gate_eps_ok(float eps) { return eps >= 0.f && isfinite(eps); }

}  // namespace mgx

extern "C" int32_t mgx_edge_gate_supported(const mgx_csr* csr, int64_t D) {
  using namespace mgx;
  return row_walk_supported(csr, D);
}

extern "C" int64_t mgx_edge_gate_workspace(const mgx_spmm_plan* plan, int64_t D) {
  return (plan ? plan->num_slots : 0) * 2 * D * (int64_t)sizeof(float);  // [slots, 2, D]: two partial sums per chunk of a split row
}

extern "C" int32_t mgx_edge_gate_fwd(const mgx_csr* csc, const mgx_spmm_plan* plan, int64_t D, const float* b, const float* s_, const float* d,
                                     const float* c, float eps, float* h, float* e_hat, float* den, void* workspace, void* stream) {
  using namespace mgx;
  MGX_ENTER();
  int32_t st = row_walk_check(csc, plan, D, "mgx_edge_gate_fwd");
  if (st != MGX_OK) return st;
  MGX_CHECK_ARG(b && s_ && d && c && h && e_hat && den, "mgx_edge_gate_fwd: NULL pointer");
  MGX_CHECK_ARG(gate_eps_ok(eps), "mgx_edge_gate_fwd: eps must be finite and >= 0");
  MGX_CHECK_ARG(row_aligned16(b) && row_aligned16(s_) && row_aligned16(d) && row_aligned16(c) && row_aligned16(h) && row_aligned16(e_hat) &&
                    row_aligned16(den),
                "mgx_edge_gate_fwd: the operands and the results must be 16-byte aligned");
  const bool hubs = plan && plan->num_slots > 0;
  MGX_CHECK_ARG(!hubs || (workspace && row_aligned16(workspace)), "mgx_edge_gate_fwd: plan has split rows but no 16-byte aligned workspace");
  hipStream_t s = (hipStream_t)stream;
  EdgeGateArgs a;
  edge_gate_fill(a, csc, plan, D, eps, workspace);
  a.b = b; a.s = s_; a.d = d; a.c = c;
  a.h = h; a.e_hat = e_hat; a.den = den;
  if (!MGX_GATE_LAUNCH(edge_gate_fwd_kernel<decltype(g)::value>)) MGX_UNSUPPORTED("mgx_edge_gate_fwd: unsupported width");
  st = walk_launched(false, plan, (int)D, nullptr, nullptr, s);
  if (st != MGX_OK) return st;
  if (hubs) {
    hipLaunchKernelGGL(edge_gate_hub_kernel<true>, hub_grid(plan), dim3(kBlock), 0, s, a, plan->hub_row, plan->hub_slot_ptr, plan->num_hubs);
    MGX_CHECK_LAUNCH();
  }
  note_spmm_kernel("edge_gate_fwd");
  return MGX_OK;
}

extern "C" int32_t mgx_edge_gate_bwd_dst(const mgx_csr* csc, const mgx_spmm_plan* plan, int64_t D, const float* b, const float* e_hat,
                                         const float* h, const float* den, float eps, const float* d_h, const float* d_e_hat, float* gn,
                                         float* d_c, float* d_d, void* workspace, void* stream) {
  using namespace mgx;
  MGX_ENTER();
  int32_t st = row_walk_check(csc, plan, D, "mgx_edge_gate_bwd_dst");
  if (st != MGX_OK) return st;
  MGX_CHECK_ARG(d_h || d_e_hat, "mgx_edge_gate_bwd_dst: NULL pointer (neither d_h nor d_e_hat)");
  MGX_CHECK_ARG(!d_h || (b && e_hat && h && den && gn), "mgx_edge_gate_bwd_dst: NULL pointer (d_h needs b, e_hat, h, den and gn)");
  MGX_CHECK_ARG(gate_eps_ok(eps), "mgx_edge_gate_bwd_dst: eps must be finite and >= 0");
  MGX_CHECK_ARG(row_aligned16(b) && row_aligned16(e_hat) && row_aligned16(h) && row_aligned16(den) && row_aligned16(d_h) &&
                    row_aligned16(d_e_hat) && row_aligned16(gn) && row_aligned16(d_c) && row_aligned16(d_d),
                "mgx_edge_gate_bwd_dst: the operands and the gradients must be 16-byte aligned");
  const bool hubs = d_d && plan && plan->num_slots > 0;
  MGX_CHECK_ARG(!hubs || (workspace && row_aligned16(workspace)), "mgx_edge_gate_bwd_dst: plan has split rows but no 16-byte aligned workspace");
  if (!d_c && !d_d && !d_h) return MGX_OK;  // (with d_h, gn is still owed to backward 2)
  hipStream_t s = (hipStream_t)stream;
  EdgeGateArgs a;
  edge_gate_fill(a, csc, plan, D, eps, workspace);
  a.b = b; a.e_hat = const_cast<float*>(e_hat); a.h = const_cast<float*>(h); a.den = const_cast<float*>(den);
  a.dh = d_h; a.de = d_e_hat; a.gn = gn; a.dc = d_c; a.o0 = d_d;
  const bool ok = d_h ? MGX_GATE_LAUNCH((edge_gate_bwd_dst_kernel<decltype(g)::value, true>))
                      : MGX_GATE_LAUNCH((edge_gate_bwd_dst_kernel<decltype(g)::value, false>));
  if (!ok) MGX_UNSUPPORTED("mgx_edge_gate_bwd_dst: unsupported width");
  st = walk_launched(hubs, plan, (int)D, a.partial, d_d, s);
  if (st != MGX_OK) return st;
  note_spmm_kernel("edge_gate_bwd_dst");
  return MGX_OK;
}

extern "C" int32_t mgx_edge_gate_bwd_src(const mgx_csr* csr, const mgx_spmm_plan* plan, int64_t D, const float* e_hat, const float* gn,
                                         const float* d_c, float* d_s, float* d_b, void* workspace, void* stream) {
  using namespace mgx;
  MGX_ENTER();
  int32_t st = row_walk_check(csr, plan, D, "mgx_edge_gate_bwd_src");
  if (st != MGX_OK) return st;
  MGX_CHECK_ARG(!d_s || d_c, "mgx_edge_gate_bwd_src: NULL pointer (d_s needs d_c)");
  MGX_CHECK_ARG(!d_b || (e_hat && gn), "mgx_edge_gate_bwd_src: NULL pointer (d_b needs e_hat and gn)");
  MGX_CHECK_ARG(row_aligned16(e_hat) && row_aligned16(gn) && row_aligned16(d_c) && row_aligned16(d_s) && row_aligned16(d_b),
                "mgx_edge_gate_bwd_src: the operands and the gradients must be 16-byte aligned");
  const bool hubs = plan && plan->num_slots > 0;
  MGX_CHECK_ARG(!hubs || (workspace && row_aligned16(workspace)), "mgx_edge_gate_bwd_src: plan has split rows but no 16-byte aligned workspace");
  if (!d_s && !d_b) return MGX_OK;
  hipStream_t s = (hipStream_t)stream;
  EdgeGateArgs a;
  edge_gate_fill(a, csr, plan, D, 0.f, workspace);
  a.e_hat = const_cast<float*>(e_hat); a.gn = const_cast<float*>(gn);
  a.dc = d_s ? const_cast<float*>(d_c) : nullptr;  // not read when d_s is not wanted
  a.o0 = d_s; a.o1 = d_b;
  const bool ok = d_b ? MGX_GATE_LAUNCH((edge_gate_bwd_src_kernel<decltype(g)::value, true>))
                      : MGX_GATE_LAUNCH((edge_gate_bwd_src_kernel<decltype(g)::value, false>));
  if (!ok) MGX_UNSUPPORTED("mgx_edge_gate_bwd_src: unsupported width");
  st = walk_launched(false, plan, (int)D, nullptr, nullptr, s);
  if (st != MGX_OK) return st;
  if (hubs) {
    hipLaunchKernelGGL(edge_gate_hub_kernel<false>, hub_grid(plan), dim3(kBlock), 0, s, a, plan->hub_row, plan->hub_slot_ptr, plan->num_hubs);
    MGX_CHECK_LAUNCH();
  }
  note_spmm_kernel("edge_gate_bwd_src");
  return MGX_OK;
}
