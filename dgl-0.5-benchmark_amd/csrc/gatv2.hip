// gatv2.hip -- GATv2 attention over a graph without any E-sized tensor (gfx950 / MI355X).
//
// Replaces the operators a dgl.nn.GATv2Conv runs between its projections and its result -- apply_edges(fn.u_add_v) -> leaky_relu ->
// (e * attn).sum(-1) -> edge_softmax -> update_all(fn.u_mul_e, fn.sum) -- and their backward.  The non-linearity comes BEFORE the
// reduction over features, so the composition materialises an [E, H, F] tensor each way; here nothing of size E exists:
//
//   s[e,h,f]   = fs[u,h,f] + fd[v,h,f]                                e: u -> v
//   z[e,h]     = sum_f attn[h,f] * lrelu(s[e,h,f])
//   a[e,h]     = exp(z[e,h] - m[v,h]) / S[v,h]                        m, S: max and sum over the in-edges of v
//   out[v,h,:] = sum_e a[e,h] fs[u,h,:]                               fs[u] is gathered once: key and value
//
//   forward   gatv2_kernel<FWD>      ONE walk of the in-CSR with an online softmax (running m and S per head, the accumulator rescaled
//                                    when m grows); writes out and stat[v,h] = (m, 1/S, ., .)
//   backward  gatv2_kernel<BWD_DST>  walks the in-CSR again (gathers fs[u]): t[v,h] = <out[v,h,:], d out[v,h,:]> into stat, a rebuilt
//                                    from (fs, fd, attn, stat), dp = <fs[u,h,:], d out[v,h,:]>, dz = a (dp - t),
//                                    d fd[v] = sum_e dz attn lrelu'(s),  d attn[h,f] = sum over ALL edges of dz lrelu(s)
//             gatv2_kernel<BWD_SRC>  walks the out-CSR (gathers fd[v], d out[v], stat[v]):
//                                    d fs[u] = sum_e (dz attn lrelu'(s) + a d out[v])      -- one accumulator, one output
// with  sum_e a dp = <out, d out>, as in dotattn.hip.  lrelu'(x) = 1 for x > 0, negative_slope otherwise (F.leaky_relu's backward).
//
// The walk skeleton is dotattn.hip's, through plan_walk.h: one wave per work item of the mgx_spmm_plan, lanes ALONG the H*F row with
// 16-byte loads, LPH = F / 4 lanes per head, ids handed out by ds_bpermute as 32-bit byte offsets, hub rows split by the plan and
// merged in slot order, the nan_max rule and the (m, 1/S, t) statistics.  This family's own: the score (a leaky_relu inside the
// feature sum, so the row constant is a whole feature row and not a scalar per head), the edge loop, and d attn -- a reduction over
// the whole graph: every wave keeps its sum in registers across all its items (a hub chunk is just more summands), the workgroup
// adds its waves through LDS in wave order and writes ONE [D] partial, and gatv2_dattn_finish_kernel adds the workgroups' partials
// in a fixed order (16 slices of the block list, added in slice order, as segment_xty_finish_kernel does).  No atomics.
#include <math.h>

#include "plan_walk.h"

namespace mgx {

enum { V2_FWD = 0, V2_BWD_DST = 1, V2_BWD_SRC = 2 };

struct GatV2Args {
  PlanItems plan;
  int H, D;
  float slope;
  const float* fs;     // [num_src, fs_ld]
  const float* fd;     // [num_dst, fd_ld]
  const float* attn;   // [H, F] dense
  int fs_ld, fd_ld;
  const float* out;    // BWD_DST: out [num_dst, D]
  const float* dout;   // BWD_*: d out [num_dst, D]
  const float* stat;   // [num_dst, H, 4] = (m, 1/S, t, .)
  float* stat_w;
  float* o1;           // FWD: out; BWD_DST: d fd (may be NULL); BWD_SRC: d fs      [rows, D]
  float* partial;      // [slots, D]
  float* pstat;        // FWD: [slots, 2H] chunk statistics (m_c, S_c)
  float* dattn_part;   // BWD_DST: [workgroups, D] partial sums of d attn (NULL: not wanted)
};

// t[v,h] = <out[v,h,:], d out[v,h,:]> into stat[v,h,2] -- only when neither d fd nor d attn is wanted but d fs is (BWD_DST writes it otherwise)
__global__ __launch_bounds__(kBlock) void gatv2_t_kernel(int64_t rows, int H, int F, const float* out, const float* dout, float* stat) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= rows * H) return;
  const float* o = out + i * F;
  const float* d = dout + i * F;
  float t = 0.f;
  for (int f = 0; f < F; ++f) t += o[f] * d[f];
  stat[i * 4 + 2] = t;
}

// d attn[e] = the workgroups' partials added in a fixed order: thread (e, sl) adds slice sl of the block list, the 16 slices are added
// in slice order.  16 elements per workgroup.
__global__ __launch_bounds__(kBlock) void gatv2_dattn_finish_kernel(int64_t nblocks, int D, const float* __restrict__ part,
                                                                    float* __restrict__ out) {
  __shared__ float red[16][17];
  const int c = threadIdx.x % 16, sl = threadIdx.x / 16;
  const int e = blockIdx.x * 16 + c;
  const int64_t per = (nblocks + 15) / 16;
  float s = 0.f;
  if (e < D) {
    const int64_t lo = sl * per, hi = lo + per < nblocks ? lo + per : nblocks;
#pragma unroll 4
    for (int64_t w = lo; w < hi; ++w) s += part[w * D + e];
  }
  red[sl][c] = s;
  __syncthreads();
  if (sl == 0 && e < D) {
    float sum = 0.f;
    for (int i = 0; i < 16; ++i) sum += red[i][c];
    out[e] = sum;
  }
}

__device__ __forceinline__ v4f lrelu4(const v4f& s, float slope) {
  v4f r;
  r.x = s.x > 0.f ? s.x : s.x * slope; r.y = s.y > 0.f ? s.y : s.y * slope;
  r.z = s.z > 0.f ? s.z : s.z * slope; r.w = s.w > 0.f ? s.w : s.w * slope;
  return r;
}
// attn * lrelu'(s)
__device__ __forceinline__ v4f lrelu_grad4(const v4f& s, const v4f& at, float slope) {
  v4f r;
  r.x = s.x > 0.f ? at.x : at.x * slope; r.y = s.y > 0.f ? at.y : at.y * slope;
  r.z = s.z > 0.f ? at.z : at.z * slope; r.w = s.w > 0.f ? at.w : at.w * slope;
  return r;
}

// ---------------------------------------------------------------------------------------------- the gather kernels
// G lanes cover one H*F row (16 bytes each; the lanes past D / 4 of a row whose lane count is no power of two idle with attn = 0);
// LPH = F / 4 lanes share a head.
template <int G, int LPH, int MODE>
__global__ __launch_bounds__(kBlock) void gatv2_kernel(const GatV2Args a) {
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
  // gathered per edge: fs[u] (FWD, BWD_DST) / fd[v], d out[v], stat[v] (BWD_SRC)
  const char* __restrict__ ga = reinterpret_cast<const char*>(MODE == V2_BWD_SRC ? a.fd : a.fs);
  const char* __restrict__ gb = reinterpret_cast<const char*>(a.dout);
  const char* __restrict__ gs = reinterpret_cast<const char*>(a.stat);
  const uint32_t abytes = (uint32_t)(MODE == V2_BWD_SRC ? a.fd_ld : a.fs_ld) * 4u;
  const uint32_t bbytes = (uint32_t)D * 4u;
  const uint32_t sbytes = (uint32_t)H * 16u;
  const uint32_t h16 = (uint32_t)head * 16u;
  const float slope = a.slope;
  const v4f at = fact ? *reinterpret_cast<const v4f*>(a.attn + f) : (v4f)(0.f);  // once per wave; 0 in idle lanes: their scores are 0
  v4f dat = (v4f)(0.f);  // BWD_DST: this lane's share of d attn, over all the items of the wave
  int64_t item_base, item_stop;
  plan_block_items(a.plan, item_base, item_stop);

  for (int r = wave; r < a.plan.rpb; r += kWavesPerBlock) {
    const int64_t item = item_base + r;
    if (item >= item_stop) break;
    const PlanItem it = plan_item(a.plan, item);
    const int64_t row = it.row, irow = it.irow;
    const int32_t beg = it.beg, end = it.end;
    // ---- row constants (idle lanes hold zeros and take part in the lane swaps)
    v4f rc = (v4f)(0.f), rb = (v4f)(0.f);  // rc: fd[v] (FWD, BWD_DST) / fs[u] (BWD_SRC); rb: d out[v] (BWD_DST)
    float c_m = 0.f, c_is = 0.f, c_t = 0.f;
    if (fact) rc = *reinterpret_cast<const v4f*>(MODE == V2_BWD_SRC ? a.fs + row * a.fs_ld + f : a.fd + row * a.fd_ld + f);
    if (MODE == V2_BWD_DST) {
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
    v4f acc = (v4f)(0.f);

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
          if (MODE == V2_BWD_SRC) {
            vb[u] = *reinterpret_cast<const v4f*>(gb + (uint32_t)__builtin_amdgcn_ds_bpermute(bi, (int)boff) + f4);
            sm[u] = *reinterpret_cast<const v4f*>(gs + (uint32_t)__builtin_amdgcn_ds_bpermute(bi, (int)soff) + h16);
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const bool live = j + u * NB + sub < cnt;
          const v4f s = va[u] + rc;  // fs[u] + fd[v] either way round
          const v4f lr = lrelu4(s, slope);
          const float z = lanes_sum<LPH>(dot4(at, lr));
          if (MODE == V2_FWD) {
            const float mn = live ? nan_max(run_m, z) : run_m;
            const float rescale = run_m == -INFINITY ? 0.f : __expf(run_m - mn);  // 1 while the maximum stands
            const float pe = (!live || mn == -INFINITY) ? 0.f : __expf(z - mn);   // mn = -inf: only masked logits (-inf) so far
            run_s = run_s * rescale + pe;
            acc = acc * rescale + va[u] * pe;
            run_m = mn;
          } else {
            const float mm = MODE == V2_BWD_DST ? c_m : sm[u].x;
            const float is = MODE == V2_BWD_DST ? c_is : sm[u].y;
            const float tt = MODE == V2_BWD_DST ? c_t : sm[u].z;
            const float av = live ? __expf(z - mm) * is : 0.f;
            // dp = <fs[u], d out[v]>: the gathered row against the row constant, whichever side is which
            const float dp = lanes_sum<LPH>(MODE == V2_BWD_DST ? dot4(rb, va[u]) : dot4(vb[u], rc));
            const float dz = live ? av * (dp - tt) : 0.f;
            acc += lrelu_grad4(s, at, slope) * dz;              // d fd[v] / d fs[u] += dz attn lrelu'(s)
            if (MODE == V2_BWD_DST) dat += lr * dz;             // d attn += dz lrelu(s)
            if (MODE == V2_BWD_SRC) acc += vb[u] * av;          // d fs[u] += a d out[v]
          }
        }
      }
    }
    // ---- combine the lane groups, write the row (or the partial slot of a hub chunk)
    if (MODE == V2_FWD) {
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
        // divided, not multiplied by 1/S: under uniform attention the row is then the correctly rounded mean of its neighbours
        if (run_s != 0.f) acc = acc / run_s;
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
        a.pstat[slot * 2 * H + head] = run_m;
        a.pstat[slot * 2 * H + H + head] = run_s;
      }
    } else {
#pragma unroll
      for (int off = G; off < kWave; off <<= 1) acc += vec_shfl_xor<4>(acc, off);
    }
    if (fact && sub == 0 && a.o1) {
      const int64_t slot = plan_slot(irow);
      *reinterpret_cast<v4f*>(irow >= 0 ? a.o1 + row * (int64_t)D + f : a.partial + slot * (int64_t)D + f) = acc;
    }
  }
  // ---- d attn of this workgroup: lane groups by swaps, then the four waves through LDS in wave order (every wave arrives here)
  if (MODE == V2_BWD_DST) {
    if (a.dattn_part) {
      __shared__ v4f red[kWavesPerBlock][G];
#pragma unroll
      for (int off = G; off < kWave; off <<= 1) dat += vec_shfl_xor<4>(dat, off);
      if (sub == 0) red[wave][l] = dat;
      __syncthreads();
      if (wave == 0 && sub == 0 && fact) {
        v4f sum = red[0][l];
#pragma unroll
        for (int w = 1; w < kWavesPerBlock; ++w) sum += red[w][l];
        *reinterpret_cast<v4f*>(a.dattn_part + (int64_t)blockIdx.x * D + f) = sum;
      }
    }
  }
}

template <int G, int MODE>
static bool gatv2_launch_lph(const GatV2Args& a, int lph, hipStream_t s) {
  const dim3 grid((unsigned)a.plan.nblocks), block(kBlock);
  switch (lph) {
#define MGX_V2_LPH(L) \
  case L: if (L <= G) { hipLaunchKernelGGL((gatv2_kernel<G, (L <= G ? L : G), MODE>), grid, block, 0, s, a); return true; } return false;
    MGX_V2_LPH(1) MGX_V2_LPH(2) MGX_V2_LPH(4) MGX_V2_LPH(8) MGX_V2_LPH(16)
#undef MGX_V2_LPH
    default: return false;
  }
}

template <int MODE>
static bool gatv2_launch(const GatV2Args& a, int F, hipStream_t s) {
  return row_walk_dispatch(a.D, [&](auto g) { return gatv2_launch_lph<decltype(g)::value, MODE>(a, F / 4, s); });
}

// ---------------------------------------------------------------------------------------------- supported set and checks (dotattn.hip's)
static bool gatv2_shape_ok(int64_t H, int64_t F) {
  return (F == 4 || F == 8 || F == 16 || F == 32 || F == 64) && H >= 1 && H * F <= 256;
}

// the kernels address gathered rows by 32-bit byte offsets: a dense [rows, H*F] operand and the [rows, H, 4] statistics stay below 4 GiB
static bool gatv2_size_ok(const mgx_csr* csr, int64_t H, int64_t F) {
  const int64_t rows = csr->num_rows > csr->num_cols ? csr->num_rows : csr->num_cols;
  const int64_t per = H * (F * 4 > 16 ? F * 4 : 16);
  return csr->nnz < (int64_t(1) << 31) && rows * per < (int64_t(1) << 32);
}

// a matrix operand: 16-byte aligned base, row stride a multiple of 4 floats and at least D
static bool gatv2_operand_ok(const float* p, int64_t ld, int64_t D) { return p && row_aligned16(p) && ld % 4 == 0 && ld >= D; }
// ... and rows * stride below 4 GiB (32-bit byte offsets); a wider stride is not an error: the caller passes a dense copy or composes
static bool gatv2_stride_fits(int64_t ld, int64_t rows) { return rows * ld * 4 < (int64_t(1) << 32); }

static int32_t gatv2_check(const mgx_csr* csr, const mgx_spmm_plan* plan, int64_t H, int64_t F, const char* who) {
  MGX_CHECK_ARG(csr != nullptr, "%s: csr is NULL", who);
  MGX_CHECK_ARG(csr->idx_bits == 32 || csr->idx_bits == 64, "%s: idx_bits must be 32 or 64 (got %d)", who, csr->idx_bits);
  if (csr->idx_bits != 32) MGX_UNSUPPORTED("%s: 32-bit graph indices only (got %d)", who, csr->idx_bits);
  MGX_CHECK_ARG(H >= 1 && F >= 1, "%s: H and F must be positive (got H = %lld, F = %lld)", who, (long long)H, (long long)F);
  if (!gatv2_shape_ok(H, F))
    MGX_UNSUPPORTED("%s: needs F in {4, 8, 16, 32, 64} and H*F <= 256 (got H = %lld, F = %lld)", who, (long long)H, (long long)F);
  if (csr->nnz <= 0) MGX_UNSUPPORTED("%s: graph without edges", who);
  if (!gatv2_size_ok(csr, H, F)) MGX_UNSUPPORTED("%s: operands beyond 32-bit byte offsets", who);
  MGX_CHECK_ARG(csr->indptr && csr->indices, "%s: indptr / indices is NULL", who);
  return plan_check(csr, plan, who);
}

// fs / fd / attn of either entry point
static int32_t gatv2_operands_check(const mgx_csr* csc, int64_t D, const float* fs, int64_t fs_ld, const float* fd, int64_t fd_ld,
                                    const float* attn, const char* who) {
  MGX_CHECK_ARG(gatv2_operand_ok(fs, fs_ld, D) && gatv2_operand_ok(fd, fd_ld, D),
                "%s: fs / fd need a 16-byte aligned base and a row stride that is a multiple of 4 and at least H*F "
                "(strides %lld / %lld, H*F = %lld)", who, (long long)fs_ld, (long long)fd_ld, (long long)D);
  MGX_CHECK_ARG(row_aligned16(attn), "%s: attn must be 16-byte aligned", who);
  if (!gatv2_stride_fits(fs_ld, csc->num_cols) || !gatv2_stride_fits(fd_ld, csc->num_rows))
    MGX_UNSUPPORTED("%s: rows * row stride of fs / fd beyond 32-bit byte offsets (strides %lld / %lld)", who, (long long)fs_ld,
                    (long long)fd_ld);
  return MGX_OK;
}

static void gatv2_fill(GatV2Args& a, const mgx_csr* csr, const mgx_spmm_plan* plan, int64_t H, int64_t F, float slope, const float* fs,
                       int64_t fs_ld, const float* fd, int64_t fd_ld, const float* attn) {
  memset(&a, 0, sizeof(a));
  plan_items_fill(a.plan, csr, plan, kPlanRowsPerBlock);
  a.H = (int)H; a.D = (int)(H * F);
  a.slope = slope;
  a.fs = fs; a.fd = fd; a.attn = attn; a.fs_ld = (int)fs_ld; a.fd_ld = (int)fd_ld;
}

// floats of the hub part of a workspace: [slots, D] partial rows + [slots, 2H] chunk statistics, kept a multiple of 16 bytes
static int64_t gatv2_hub_floats(const mgx_spmm_plan* plan, int64_t H, int64_t F) {
  const int64_t slots = plan ? plan->num_slots : 0;
  return round_up(slots * (H * F + 2 * H), 4);
}

}  // namespace mgx

extern "C" int32_t mgx_gatv2_supported(const mgx_csr* csr, int64_t H, int64_t F) {
  using namespace mgx;
  return csr && csr->idx_bits == 32 && csr->nnz > 0 && gatv2_shape_ok(H, F) && gatv2_size_ok(csr, H, F);
}

extern "C" int64_t mgx_gatv2_workspace(const mgx_spmm_plan* plan, const mgx_csr* csr, int64_t H, int64_t F) {
  using namespace mgx;
  if (!csr || H < 1 || F < 1) return 0;
  // the hub slots (forward: partial rows + chunk statistics; backward: one [slots, D] per walk), then the [workgroups, D] partials of d attn
  PlanItems p;
  plan_items_fill(p, csr, plan, kPlanRowsPerBlock);
  return (gatv2_hub_floats(plan, H, F) + p.nblocks * H * F) * (int64_t)sizeof(float);
}

extern "C" int32_t mgx_gatv2_fwd(const mgx_csr* csr, const mgx_spmm_plan* plan, int64_t H, int64_t F, const float* fs, int64_t fs_ld,
                                 const float* fd, int64_t fd_ld, const float* attn, float negative_slope, float* out, float* stat,
                                 void* workspace, void* stream) {
  using namespace mgx;
  MGX_ENTER();
  int32_t st = gatv2_check(csr, plan, H, F, "mgx_gatv2_fwd");
  if (st != MGX_OK) return st;
  const int64_t D = H * F;
  MGX_CHECK_ARG(fs && fd && attn && out && stat, "mgx_gatv2_fwd: NULL pointer");
  st = gatv2_operands_check(csr, D, fs, fs_ld, fd, fd_ld, attn, "mgx_gatv2_fwd");
  if (st != MGX_OK) return st;
  MGX_CHECK_ARG(row_aligned16(out) && row_aligned16(stat), "mgx_gatv2_fwd: out and stat must be 16-byte aligned");
  const bool hubs = plan && plan->num_slots > 0;
  MGX_CHECK_ARG(!hubs || workspace, "mgx_gatv2_fwd: plan has split rows but no workspace");
  hipStream_t s = (hipStream_t)stream;
  GatV2Args a;
  gatv2_fill(a, csr, plan, H, F, negative_slope, fs, fs_ld, fd, fd_ld, attn);
  a.stat = stat; a.stat_w = stat; a.o1 = out;
  float* ws = (float*)workspace;
  a.partial = ws;
  a.pstat = hubs ? ws + plan->num_slots * D : nullptr;
  if (!gatv2_launch<V2_FWD>(a, (int)F, s)) MGX_UNSUPPORTED("mgx_gatv2_fwd: unsupported head layout");
  MGX_CHECK_LAUNCH();
  if (hubs) {
    hub_online_merge<true>(plan, (int)H, (int)F, nullptr, a.partial, a.pstat, out, stat, s);
    MGX_CHECK_LAUNCH();
  }
  note_spmm_kernel("gatv2_fwd");
  return MGX_OK;
}

extern "C" int32_t mgx_gatv2_bwd(const mgx_csr* csc, const mgx_spmm_plan* csc_plan, const mgx_csr* csr, const mgx_spmm_plan* csr_plan,
                                 int64_t H, int64_t F, const float* fs, int64_t fs_ld, const float* fd, int64_t fd_ld, const float* attn,
                                 float negative_slope, const float* out, const float* d_out, float* stat, float* d_fs, float* d_fd,
                                 float* d_attn, void* workspace, void* stream) {
  using namespace mgx;
  MGX_ENTER();
  int32_t st = gatv2_check(csc, csc_plan, H, F, "mgx_gatv2_bwd");
  if (st != MGX_OK) return st;
  st = gatv2_check(csr, csr_plan, H, F, "mgx_gatv2_bwd");
  if (st != MGX_OK) return st;
  MGX_CHECK_ARG(csc->num_rows == csr->num_cols && csc->num_cols == csr->num_rows && csc->nnz == csr->nnz,
                "mgx_gatv2_bwd: the two CSRs are not transposes of each other");
  const int64_t D = H * F;
  MGX_CHECK_ARG(fs && fd && attn && out && d_out && stat, "mgx_gatv2_bwd: NULL pointer");
  st = gatv2_operands_check(csc, D, fs, fs_ld, fd, fd_ld, attn, "mgx_gatv2_bwd");
  if (st != MGX_OK) return st;
  MGX_CHECK_ARG(row_aligned16(out) && row_aligned16(d_out) && row_aligned16(stat) && row_aligned16(d_fs) && row_aligned16(d_fd) &&
                row_aligned16(d_attn) && row_aligned16(workspace),
                "mgx_gatv2_bwd: out, d_out, stat, the gradients and the workspace must be 16-byte aligned");
  const bool hubs_dst = csc_plan && csc_plan->num_slots > 0, hubs_src = csr_plan && csr_plan->num_slots > 0;
  MGX_CHECK_ARG(!(d_attn || (hubs_dst && d_fd) || (hubs_src && d_fs)) || workspace,
                "mgx_gatv2_bwd: d_attn or a plan with split rows needs the workspace");
  hipStream_t s = (hipStream_t)stream;
  float* ws = (float*)workspace;
  if (d_fd || d_attn) {  // destination side: t[v,h] into stat, d fd, the workgroups' partials of d attn
    GatV2Args a;
    gatv2_fill(a, csc, csc_plan, H, F, negative_slope, fs, fs_ld, fd, fd_ld, attn);
    a.out = out; a.dout = d_out; a.stat = stat; a.stat_w = stat; a.o1 = d_fd;
    a.partial = ws;
    a.dattn_part = d_attn ? ws + gatv2_hub_floats(csc_plan, H, F) : nullptr;
    if (!gatv2_launch<V2_BWD_DST>(a, (int)F, s)) MGX_UNSUPPORTED("mgx_gatv2_bwd: unsupported head layout");
    st = walk_launched(hubs_dst && d_fd, csc_plan, (int)D, a.partial, d_fd, s);
    if (st != MGX_OK) return st;
    if (d_attn) {
      hipLaunchKernelGGL(gatv2_dattn_finish_kernel, dim3((unsigned)((D + 15) / 16)), dim3(kBlock), 0, s, a.plan.nblocks, (int)D,
                         a.dattn_part, d_attn);
      MGX_CHECK_LAUNCH();
    }
    note_spmm_kernel("gatv2_bwd_dst");
  } else if (d_fs) {  // d fs needs t of every destination
    const int64_t n = csc->num_rows * H;
    hipLaunchKernelGGL(gatv2_t_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, csc->num_rows, (int)H, (int)F, out,
                       d_out, stat);
    MGX_CHECK_LAUNCH();
  }
  if (d_fs) {  // source side (same stream: after t was written and the destination side's hub slots were merged)
    GatV2Args a;
    gatv2_fill(a, csr, csr_plan, H, F, negative_slope, fs, fs_ld, fd, fd_ld, attn);
    a.dout = d_out; a.stat = stat; a.o1 = d_fs;
    a.partial = ws;
    if (!gatv2_launch<V2_BWD_SRC>(a, (int)F, s)) MGX_UNSUPPORTED("mgx_gatv2_bwd: unsupported head layout");
    st = walk_launched(hubs_src, csr_plan, (int)D, a.partial, d_fs, s);
    if (st != MGX_OK) return st;
    note_spmm_kernel("gatv2_bwd_src");
  }
  return MGX_OK;
}
