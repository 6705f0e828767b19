// dotattn.hip -- scaled dot-product attention over a graph without any E-sized tensor (gfx950 / MI355X).
//
// Replaces the three operators a dgl.nn.DotGatConv runs between its projection and its result -- apply_edges(fn.u_dot_v) ->
// edge_softmax -> update_all(fn.u_mul_e, fn.sum) -- and their backward:
//
//   z[e,h]     = scale * <q[v,h,:], k[u,h,:]>                        e: u -> v, scale applied once, after the sum
//   a[e,h]     = exp(z[e,h] - m[v,h]) / s[v,h]                       m, s: max and sum over the in-edges of v
//   out[v,h,:] = sum_e a[e,h] v[u,h,:]
//
//   forward   dot_attn_kernel<FWD>      ONE walk of the in-CSR with an online softmax (running m and s per head, the accumulator
//                                       rescaled when m grows); writes out and stat[v,h] = (m, 1/s, ., .)
//   backward  dot_attn_kernel<BWD_DST>  walks the in-CSR again (gathers k[u], v[u]): t[v,h] = <out[v,h,:], d out[v,h,:]> into stat,
//                                       a rebuilt from (q, k, stat), dp = <v[u,h,:], d out[v,h,:]>, ds = a (dp - t) scale,
//                                       d q[v] = sum_e ds k[u]
//             dot_attn_kernel<BWD_SRC>  walks the out-CSR (gathers q[v], d out[v], stat[v]): d k[u] = sum_e ds q[v], d v[u] = sum_e a d out[v]
// using  sum_e a dp = <out, d out>  (out IS that weighted sum), so the softmax backward needs no pass of its own: the flash-attention
// backward, row by row.
//
// Laid out like gat_fused_kernel (gatfused.hip): one wave per work item of the mgx_spmm_plan, lanes ALONG the H*F row with 16-byte
// loads, 64/G neighbour rows per wave-instruction, ids handed out by ds_bpermute as 32-bit byte offsets; hub rows are split by the
// plan and merged in slot order (no atomics: deterministic).  The walk skeleton -- the plan's items as kernel arguments, a block's
// stretch and an item's (row, edge range), the hub-slot convention, the two hub merge kernels -- is plan_walk.h, shared with
// gatfused.hip; the edge loop, the NaN rule (nan_max: a NaN logit reaches the row's result) and the (m, 1/s, t) statistics are this
// family's own.  Every matrix operand of the caller has a row stride, so q, k and v may be column blocks of one projection.
// KV_SAME: k and v are one array -- the row is gathered once.
#include <math.h>

#include "plan_walk.h"

namespace mgx {

enum { DOT_FWD = 0, DOT_BWD_DST = 1, DOT_BWD_SRC = 2 };

struct DotArgs {
  PlanItems plan;
  int H, D;
  float scale;
  const float* q;      // [num_dst, q_ld]
  const float* k;      // [num_src, k_ld]
  const float* v;      // [num_src, v_ld]
  int q_ld, k_ld, v_ld;
  const float* out;    // BWD_DST: out [num_dst, D]
  const float* dout;   // BWD_*: d out [num_dst, D]
  const float* stat;   // [num_dst, H, 4] = (m, 1/s, t, .)
  float* stat_w;
  float* o1;           // FWD: out; BWD_DST: d q; BWD_SRC: d k      [rows, D]
  float* o2;           // BWD_SRC: d v (may be NULL)
  float* partial;      // [slots, D]
  float* partial2;     // BWD_SRC: [slots, D] of d v; FWD: [slots, 2H] chunk statistics (m_c, s_c)
};

// t[v,h] = <out[v,h,:], d out[v,h,:]> into stat[v,h,2] -- only when d q is not wanted but d k is (BWD_DST writes it otherwise)
__global__ __launch_bounds__(kBlock) void dot_attn_t_kernel(int64_t rows, int H, int F, const float* out, const float* dout, float* stat) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= rows * H) return;
  const float* o = out + i * F;
  const float* d = dout + i * F;
  float t = 0.f;
  for (int f = 0; f < F; ++f) t += o[f] * d[f];
  stat[i * 4 + 2] = t;
}

// ---------------------------------------------------------------------------------------------- the gather kernels
// G lanes cover one H*F row (16 bytes each; the lanes past D / 4 of a row whose lane count is no power of two idle);
// LPH = F / 4 lanes share a head.
template <int G, int LPH, int MODE, bool KV_SAME>
__global__ __launch_bounds__(kBlock) void dot_attn_kernel(const DotArgs a) {
  constexpr int NB = kWave / G;
  constexpr int U = LaneUnroll<G>::value;
  constexpr int STEP = NB * U;
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int sub = lane / G, l = lane % G;
  const int D = a.D, H = a.H;
  const int f = l * 4;
  const bool fact = f < D;
  const int head = fact ? l / LPH : 0;
  const uint32_t f4 = fact ? (uint32_t)f * 4u : 0u;  // idle feature lanes re-read the row start, never stored
  const bool lead = fact && sub == 0 && (l % LPH) == 0;
  // gathered operands: A = k (FWD, BWD_DST) / q (BWD_SRC), B = v (FWD, BWD_DST) / d out (BWD_SRC); BWD_SRC also gathers stat
  const char* __restrict__ ga = reinterpret_cast<const char*>(MODE == DOT_BWD_SRC ? a.q : a.k);
  const char* __restrict__ gb = reinterpret_cast<const char*>(MODE == DOT_BWD_SRC ? a.dout : a.v);
  const char* __restrict__ gs = reinterpret_cast<const char*>(a.stat);
  const uint32_t abytes = (uint32_t)(MODE == DOT_BWD_SRC ? a.q_ld : a.k_ld) * 4u;
  const uint32_t bbytes = (uint32_t)(MODE == DOT_BWD_SRC ? D : a.v_ld) * 4u;
  const uint32_t sbytes = (uint32_t)H * 16u;
  const uint32_t h16 = (uint32_t)head * 16u;
  const float scale = a.scale;
  int64_t item_base, item_stop;
  plan_block_items(a.plan, item_base, item_stop);

  for (int r = wave; r < a.plan.rpb; r += kWavesPerBlock) {
    const int64_t item = item_base + r;
    if (item >= item_stop) break;
    const PlanItem it = plan_item(a.plan, item);
    const int64_t row = it.row, irow = it.irow;
    const int32_t beg = it.beg, end = it.end;
    // ---- row constants (idle lanes hold zeros and take part in the lane swaps)
    v4f ra = (v4f)(0.f), rb = (v4f)(0.f);  // FWD: q[v], -; BWD_DST: q[v], d out[v]; BWD_SRC: k[u], v[u]
    float c_m = 0.f, c_is = 0.f, c_t = 0.f;
    if (fact) {
      if (MODE == DOT_BWD_SRC) {
        ra = *reinterpret_cast<const v4f*>(a.k + row * a.k_ld + f);
        rb = *reinterpret_cast<const v4f*>(a.v + row * a.v_ld + f);
      } else {
        ra = *reinterpret_cast<const v4f*>(a.q + row * a.q_ld + f);
      }
    }
    if (MODE == DOT_BWD_DST) {
      v4f ov = (v4f)(0.f);
      if (fact) {
        rb = *reinterpret_cast<const v4f*>(a.dout + row * D + f);
        ov = *reinterpret_cast<const v4f*>(a.out + row * D + f);
      }
      const v4f st = *reinterpret_cast<const v4f*>(a.stat + (row * H + head) * 4);
      c_m = st.x; c_is = st.y;
      c_t = lanes_sum<LPH>(dot4(rb, ov));
      if (lead) a.stat_w[(row * H + head) * 4 + 2] = c_t;  // every chunk of a hub row writes the same value
    }
    float run_m = -INFINITY, run_s = 0.f;  // FWD: online softmax state of this lane's head (per lane group)
    v4f acc = (v4f)(0.f), acc2 = (v4f)(0.f);

    for (int32_t cbase = beg; cbase < end; cbase += kWave) {
      const int32_t p = cbase + lane;
      uint32_t aoff = 0, boff = 0, soff = 0;
      if (p < end) {
        const uint32_t gid = (uint32_t)__builtin_nontemporal_load(&a.plan.indices[p]);
        aoff = gid * abytes;
        boff = gid * bbytes;
        soff = gid * sbytes;
      }
      const int cnt = (end - cbase) < kWave ? (end - cbase) : kWave;
      for (int j = 0; j < cnt; j += STEP) {
        v4f va[U], vb[U], sm[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int jdx = j + u * NB + sub;
          const int bi = (jdx < cnt ? jdx : 0) * 4;  // lanes past the end re-read edge 0 (valid memory), weight zeroed below
          va[u] = *reinterpret_cast<const v4f*>(ga + (uint32_t)__builtin_amdgcn_ds_bpermute(bi, (int)aoff) + f4);
          if (MODE == DOT_BWD_SRC || !KV_SAME) vb[u] = *reinterpret_cast<const v4f*>(gb + (uint32_t)__builtin_amdgcn_ds_bpermute(bi, (int)boff) + f4);
          else vb[u] = va[u];
          if (MODE == DOT_BWD_SRC) sm[u] = *reinterpret_cast<const v4f*>(gs + (uint32_t)__builtin_amdgcn_ds_bpermute(bi, (int)soff) + h16);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const bool live = j + u * NB + sub < cnt;
          const float z = lanes_sum<LPH>(dot4(ra, va[u])) * scale;
          if (MODE == DOT_FWD) {
            const float mn = live ? nan_max(run_m, z) : run_m;
            const float rescale = run_m == -INFINITY ? 0.f : __expf(run_m - mn);  // 1 while the maximum stands
            const float pe = (!live || mn == -INFINITY) ? 0.f : __expf(z - mn);   // mn = -inf: only masked logits (-inf) so far
            run_s = run_s * rescale + pe;
            acc = acc * rescale + vb[u] * pe;
            run_m = mn;
          } else {
            const float mm = MODE == DOT_BWD_DST ? c_m : sm[u].x;
            const float is = MODE == DOT_BWD_DST ? c_is : sm[u].y;
            const float tt = MODE == DOT_BWD_DST ? c_t : sm[u].z;
            const float av = live ? __expf(z - mm) * is : 0.f;
            const float dp = lanes_sum<LPH>(dot4(rb, vb[u]));
            const float ds = live ? av * (dp - tt) * scale : 0.f;
            acc += va[u] * ds;                                 // d q += ds k[u] / d k += ds q[v]
            if (MODE == DOT_BWD_SRC) acc2 += vb[u] * av;       // d v += a d out[v]
          }
        }
      }
    }
    // ---- combine the lane groups, write the row (or the partial slot of a hub chunk)
    if (MODE == DOT_FWD) {
#pragma unroll
      for (int off = G; off < kWave; off <<= 1) {
        const float mo = __shfl_xor(run_m, off, kWave), so = __shfl_xor(run_s, off, kWave);
        const v4f ao = vec_shfl_xor<4>(acc, off);
        const float mn = nan_max(run_m, mo);
        const float f1 = run_m == -INFINITY ? 0.f : __expf(run_m - mn), f2 = mo == -INFINITY ? 0.f : __expf(mo - mn);
        run_s = run_s * f1 + so * f2;
        acc = acc * f1 + ao * f2;
        run_m = mn;
      }
      if (irow >= 0) {
        const float is = run_s == 0.f ? 0.f : 1.f / run_s;  // rows without in-edges aggregate to 0
        acc = acc * is;
        if (lead) {
          v4f st;
          st.x = run_m == -INFINITY ? 0.f : run_m;
          st.y = is;
          st.z = 0.f;
          st.w = 0.f;
          *reinterpret_cast<v4f*>(a.stat_w + (row * H + head) * 4) = st;
        }
      } else if (lead) {  // hub chunk: statistics travel with the unnormalised partial row
        const int64_t slot = plan_slot(irow);
        a.partial2[slot * 2 * H + head] = run_m;
        a.partial2[slot * 2 * H + H + head] = run_s;
      }
    } else {
#pragma unroll
      for (int off = G; off < kWave; off <<= 1) {
        acc += vec_shfl_xor<4>(acc, off);
        if (MODE == DOT_BWD_SRC) acc2 += vec_shfl_xor<4>(acc2, off);
      }
    }
    if (fact && sub == 0) {
      const int64_t slot = plan_slot(irow);
      if (a.o1) *reinterpret_cast<v4f*>(irow >= 0 ? a.o1 + row * (int64_t)D + f : a.partial + slot * (int64_t)D + f) = acc;
      if (MODE == DOT_BWD_SRC && a.o2) *reinterpret_cast<v4f*>(irow >= 0 ? a.o2 + row * (int64_t)D + f : a.partial2 + slot * (int64_t)D + f) = acc2;
    }
  }
}

template <int G, int LPH, int MODE>
static void dot_launch_kv(const DotArgs& a, bool kv_same, hipStream_t s) {
  const dim3 grid((unsigned)a.plan.nblocks), block(kBlock);
  if (MODE != DOT_BWD_SRC && kv_same) hipLaunchKernelGGL((dot_attn_kernel<G, LPH, MODE, true>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((dot_attn_kernel<G, LPH, MODE, false>), grid, block, 0, s, a);
}

template <int G, int MODE>
static bool dot_launch_lph(const DotArgs& a, int lph, bool kv_same, hipStream_t s) {
  switch (lph) {
#define MGX_DOT_LPH(L) case L: if (L <= G) { dot_launch_kv<G, (L <= G ? L : G), MODE>(a, kv_same, s); return true; } return false;
    MGX_DOT_LPH(1) MGX_DOT_LPH(2) MGX_DOT_LPH(4) MGX_DOT_LPH(8) MGX_DOT_LPH(16)
#undef MGX_DOT_LPH
    default: return false;
  }
}

template <int MODE>
static bool dot_launch(const DotArgs& a, int F, bool kv_same, hipStream_t s) {
  int G = 1;
  while (G * 4 < a.D) G <<= 1;
  const int lph = F / 4;
  switch (G) {
    case 1: return dot_launch_lph<1, MODE>(a, lph, kv_same, s);
    case 2: return dot_launch_lph<2, MODE>(a, lph, kv_same, s);
    case 4: return dot_launch_lph<4, MODE>(a, lph, kv_same, s);
    case 8: return dot_launch_lph<8, MODE>(a, lph, kv_same, s);
    case 16: return dot_launch_lph<16, MODE>(a, lph, kv_same, s);
    case 32: return dot_launch_lph<32, MODE>(a, lph, kv_same, s);
    case 64: return dot_launch_lph<64, MODE>(a, lph, kv_same, s);
    default: return false;
  }
}

static bool dot_shape_ok(int64_t H, int64_t F) {
  return (F == 4 || F == 8 || F == 16 || F == 32 || F == 64) && H >= 1 && H * F <= 256;
}

// the kernels address gathered rows by 32-bit byte offsets: a dense [rows, H*F] operand and the [rows, H, 4] statistics stay below 4 GiB
static bool dot_size_ok(const mgx_csr* csr, int64_t H, int64_t F) {
  const int64_t rows = csr->num_rows > csr->num_cols ? csr->num_rows : csr->num_cols;
  const int64_t per = H * (F * 4 > 16 ? F * 4 : 16);
  return csr->nnz < (int64_t(1) << 31) && rows * per < (int64_t(1) << 32);
}

// a matrix operand: 16-byte aligned base, row stride a multiple of 4 floats and at least D
static bool dot_operand_ok(const float* p, int64_t ld, int64_t D) {
  return p && (uintptr_t)p % 16 == 0 && ld % 4 == 0 && ld >= D;
}
// ... and rows * stride below 4 GiB (32-bit byte offsets); a wider stride is not an error: the caller passes a dense copy or composes
static bool dot_stride_fits(int64_t ld, int64_t rows) { return rows * ld * 4 < (int64_t(1) << 32); }

static int32_t dot_check(const mgx_csr* csr, const mgx_spmm_plan* plan, int64_t H, int64_t F, const char* who) {
  MGX_CHECK_ARG(csr != nullptr, "%s: csr is NULL", who);
  MGX_CHECK_ARG(csr->idx_bits == 32 || csr->idx_bits == 64, "%s: idx_bits must be 32 or 64 (got %d)", who, csr->idx_bits);
  if (csr->idx_bits != 32) MGX_UNSUPPORTED("%s: 32-bit graph indices only (got %d)", who, csr->idx_bits);
  MGX_CHECK_ARG(H >= 1 && F >= 1, "%s: H and F must be positive (got H = %lld, F = %lld)", who, (long long)H, (long long)F);
  if (!dot_shape_ok(H, F))
    MGX_UNSUPPORTED("%s: needs F in {4, 8, 16, 32, 64} and H*F <= 256 (got H = %lld, F = %lld)", who, (long long)H, (long long)F);
  if (csr->nnz <= 0) MGX_UNSUPPORTED("%s: graph without edges", who);
  if (!dot_size_ok(csr, H, F)) MGX_UNSUPPORTED("%s: operands beyond 32-bit byte offsets", who);
  MGX_CHECK_ARG(csr->indptr && csr->indices, "%s: indptr / indices is NULL", who);
  return plan_check(csr, plan, who);
}

static void dot_fill(DotArgs& a, const mgx_csr* csr, const mgx_spmm_plan* plan, int64_t H, int64_t F, float scale) {
  memset(&a, 0, sizeof(a));
  plan_items_fill(a.plan, csr, plan, kPlanRowsPerBlock);
  a.H = (int)H; a.D = (int)(H * F);
  a.scale = scale;
}

}  // namespace mgx

extern "C" int32_t mgx_dot_attention_supported(const mgx_csr* csr, int64_t H, int64_t F) {
  using namespace mgx;
  return csr && csr->idx_bits == 32 && csr->nnz > 0 && dot_shape_ok(H, F) && dot_size_ok(csr, H, F);
}

extern "C" int64_t mgx_dot_attention_workspace(const mgx_spmm_plan* plan, int64_t H, int64_t F) {
  const int64_t slots = plan ? plan->num_slots : 0;
  // forward: [slots, D] partial rows + [slots, 2H] chunk statistics; backward: [slots, D] of d q, or two [slots, D] of d k and d v
  return slots * (2 * H * F + 2 * H) * (int64_t)sizeof(float);
}

extern "C" int32_t mgx_dot_attention_fwd(const mgx_csr* csr, const mgx_spmm_plan* plan, int64_t H, int64_t F, const float* q, int64_t q_ld,
                                         const float* k, int64_t k_ld, const float* v, int64_t v_ld, float scale, float* out, float* stat,
                                         void* workspace, void* stream) {
  using namespace mgx;
  MGX_ENTER();
  int32_t st = dot_check(csr, plan, H, F, "mgx_dot_attention_fwd");
  if (st != MGX_OK) return st;
  const int64_t D = H * F;
  MGX_CHECK_ARG(q && k && v && out && stat, "mgx_dot_attention_fwd: NULL pointer");
  MGX_CHECK_ARG(dot_operand_ok(q, q_ld, D) && dot_operand_ok(k, k_ld, D) && dot_operand_ok(v, v_ld, D),
                "mgx_dot_attention_fwd: q / k / v need a 16-byte aligned base and a row stride that is a multiple of 4 and at least H*F "
                "(strides %lld / %lld / %lld, H*F = %lld)", (long long)q_ld, (long long)k_ld, (long long)v_ld, (long long)D);
  if (!dot_stride_fits(q_ld, csr->num_rows) || !dot_stride_fits(k_ld, csr->num_cols) || !dot_stride_fits(v_ld, csr->num_cols))
    MGX_UNSUPPORTED("mgx_dot_attention_fwd: rows * row stride of q / k / v beyond 32-bit byte offsets (strides %lld / %lld / %lld)",
                    (long long)q_ld, (long long)k_ld, (long long)v_ld);
  MGX_CHECK_ARG((uintptr_t)out % 16 == 0 && (uintptr_t)stat % 16 == 0, "mgx_dot_attention_fwd: out and stat must be 16-byte aligned");
  const bool hubs = plan && plan->num_slots > 0;
  MGX_CHECK_ARG(!hubs || workspace, "mgx_dot_attention_fwd: plan has split rows but no workspace");
  hipStream_t s = (hipStream_t)stream;
  DotArgs a;
  dot_fill(a, csr, plan, H, F, scale);
  a.q = q; a.k = k; a.v = v; a.q_ld = (int)q_ld; a.k_ld = (int)k_ld; a.v_ld = (int)v_ld;
  a.stat = stat; a.stat_w = stat; a.o1 = out;
  float* ws = (float*)workspace;
  a.partial = ws;
  a.partial2 = hubs ? ws + plan->num_slots * D : nullptr;
  if (!dot_launch<DOT_FWD>(a, (int)F, k == v && k_ld == v_ld, s)) MGX_UNSUPPORTED("mgx_dot_attention_fwd: unsupported head layout");
  MGX_CHECK_LAUNCH();
  if (hubs) {
    hub_online_merge<true>(plan, (int)H, (int)F, nullptr, a.partial, a.partial2, out, stat, s);
    MGX_CHECK_LAUNCH();
  }
  note_spmm_kernel("dot_attn_fwd");
  return MGX_OK;
}

extern "C" int32_t mgx_dot_attention_bwd(const mgx_csr* csc, const mgx_spmm_plan* csc_plan, const mgx_csr* csr, const mgx_spmm_plan* csr_plan,
                                         int64_t H, int64_t F, const float* q, int64_t q_ld, const float* k, int64_t k_ld, const float* v,
                                         int64_t v_ld, float scale, const float* out, const float* d_out, float* stat, float* dq, float* dk,
                                         float* dv, void* workspace, void* stream) {
  using namespace mgx;
  MGX_ENTER();
  int32_t st = dot_check(csc, csc_plan, H, F, "mgx_dot_attention_bwd");
  if (st != MGX_OK) return st;
  st = dot_check(csr, csr_plan, H, F, "mgx_dot_attention_bwd");
  if (st != MGX_OK) return st;
  MGX_CHECK_ARG(csc->num_rows == csr->num_cols && csc->num_cols == csr->num_rows && csc->nnz == csr->nnz,
                "mgx_dot_attention_bwd: the two CSRs are not transposes of each other");
  const int64_t D = H * F;
  MGX_CHECK_ARG(q && k && v && out && d_out && stat, "mgx_dot_attention_bwd: NULL pointer");
  MGX_CHECK_ARG(dot_operand_ok(q, q_ld, D) && dot_operand_ok(k, k_ld, D) && dot_operand_ok(v, v_ld, D),
                "mgx_dot_attention_bwd: q / k / v need a 16-byte aligned base and a row stride that is a multiple of 4 and at least H*F "
                "(strides %lld / %lld / %lld, H*F = %lld)", (long long)q_ld, (long long)k_ld, (long long)v_ld, (long long)D);
  if (!dot_stride_fits(q_ld, csc->num_rows) || !dot_stride_fits(k_ld, csc->num_cols) || !dot_stride_fits(v_ld, csc->num_cols))
    MGX_UNSUPPORTED("mgx_dot_attention_bwd: rows * row stride of q / k / v beyond 32-bit byte offsets (strides %lld / %lld / %lld)",
                    (long long)q_ld, (long long)k_ld, (long long)v_ld);
  MGX_CHECK_ARG((uintptr_t)out % 16 == 0 && (uintptr_t)d_out % 16 == 0 && (uintptr_t)stat % 16 == 0 && (uintptr_t)dq % 16 == 0 &&
                (uintptr_t)dk % 16 == 0 && (uintptr_t)dv % 16 == 0,
                "mgx_dot_attention_bwd: out, d_out, stat and the gradients must be 16-byte aligned");
  const bool hubs_dst = csc_plan && csc_plan->num_slots > 0, hubs_src = csr_plan && csr_plan->num_slots > 0;
  MGX_CHECK_ARG(!((hubs_dst && dq) || (hubs_src && (dk || dv))) || workspace, "mgx_dot_attention_bwd: plan has split rows but no workspace");
  hipStream_t s = (hipStream_t)stream;
  if (dq) {  // destination side: t[v,h] into stat, d q
    DotArgs a;
    dot_fill(a, csc, csc_plan, H, F, scale);
    a.q = q; a.k = k; a.v = v; a.q_ld = (int)q_ld; a.k_ld = (int)k_ld; a.v_ld = (int)v_ld;
    a.out = out; a.dout = d_out; a.stat = stat; a.stat_w = stat; a.o1 = dq;
    a.partial = (float*)workspace;
    if (!dot_launch<DOT_BWD_DST>(a, (int)F, k == v && k_ld == v_ld, s)) MGX_UNSUPPORTED("mgx_dot_attention_bwd: unsupported head layout");
    MGX_CHECK_LAUNCH();
    if (hubs_dst) {
      hub_rows_sum(csc_plan, (int)D, a.partial, dq, s);
      MGX_CHECK_LAUNCH();
    }
    note_spmm_kernel("dot_attn_bwd_dst");
  } else if (dk) {  // d k needs t of every destination
    const int64_t n = csc->num_rows * H;
    hipLaunchKernelGGL(dot_attn_t_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, csc->num_rows, (int)H, (int)F, out,
                       d_out, stat);
    MGX_CHECK_LAUNCH();
  }
  if (dk || dv) {  // source side (same stream: after t was written)
    float* ws = (float*)workspace;
    DotArgs a;
    dot_fill(a, csr, csr_plan, H, F, scale);
    a.q = q; a.k = k; a.v = v; a.q_ld = (int)q_ld; a.k_ld = (int)k_ld; a.v_ld = (int)v_ld;
    a.dout = d_out; a.stat = stat; a.o1 = dk; a.o2 = dv;
    a.partial = ws;
    a.partial2 = hubs_src ? ws + csr_plan->num_slots * D : nullptr;
    if (!dot_launch<DOT_BWD_SRC>(a, (int)F, false, s)) MGX_UNSUPPORTED("mgx_dot_attention_bwd: unsupported head layout");
    MGX_CHECK_LAUNCH();
    if (hubs_src) {
      if (dk) hub_rows_sum(csr_plan, (int)D, a.partial, dk, s);
      if (dv) hub_rows_sum(csr_plan, (int)D, a.partial2, dv, s);
      MGX_CHECK_LAUNCH();
    }
    note_spmm_kernel("dot_attn_bwd_src");
  }
  return MGX_OK;
}
