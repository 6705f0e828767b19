// segattn.hip -- graph readout over the contiguous row segments of a batched graph (gfx950 / MI355X): the per-column segment softmax
// (dgl.softmax_nodes / softmax_edges) and the fused attention readout of dgl.nn.GlobalAttentionPooling and dgl.nn.Set2Set.
//
//   segment softmax     out[i,c] = exp(x[i,c] - m[g,c]) / s[g,c]                     m, s: max and sum over the rows of segment g
//                       d x      = out * (d out - sum_{j in g} out[j,c] d out[j,c])
//   segment attention   z[i,h]     = logits[i,h]                                     gate mode  (GlobalAttentionPooling)
//                       z[i,h]     = scale * <feat[i,h,:], query[g,h,:]>             query mode (Set2Set), scale applied once, after the sum
//                       a[i,h]     = exp(z[i,h] - m[g,h]) / s[g,h]
//                       out[g,h,:] = sum_{i in g} a[i,h] feat[i,h,:]
//     forward   seg_attn_kernel<FWD>  ONE walk of the segment with an online softmax (running m and s per head, the accumulator rescaled
//                                     when m grows); writes out and stat[g,h] = (m, 1/s)
//     backward  seg_attn_kernel<BWD>  ONE walk: t[g,h] = <out[g,h,:], d out[g,h,:]>, a rebuilt from stat, dp = <feat[i,h,:], d out[g,h,:]>,
//                                     dz = a (dp - t);  gate: d logits = dz, d feat[i] = a d out[g];
//                                     query: d feat[i] = a d out[g] + dz scale query[g], d query[g] = scale sum_i dz feat[i]
//   (sum_i a dp = <out, d out>: the flash-attention backward of dotattn.hip, over rows that need no gather.)
//
// Laid out like dot_attn_kernel (dotattn.hip): one wave per segment, G lanes ALONG the H*F row with 16-byte loads, 64/G rows per
// wave-instruction, LaneUnroll<G> rows in flight per lane group; the lane groups' (m, s, accumulator) are merged by an online-softmax
// merge in a fixed order when the segment ends.  The segment's query, d out, out and stat rows live in registers, d query is accumulated
// in registers and stored once.  No atomics, no N-sized temporary: reruns are bitwise equal.  Nothing here reads offsets on the host, so
// every entry point can be captured in a HIP graph.
//
// Shapes of the fused pair (mgx_segment_attention_supported): F % 4 == 0, H*F <= 256, feat_ld % 4 == 0 and >= H*F; one head takes any such
// F (its lanes_sum spans the whole lane group, idle lanes hold zeros), several heads need F in {4, 8, 16, 32, 64} (lanes_sum<F/4>).
// The segment softmax takes any D >= 1.
//
// Edge rules (the dot family's):
//   an empty segment            out = 0, stat = (0, 0), every gradient 0
//   a -inf logit                weight 0
//   only -inf logits            like an empty segment: out = 0 (not NaN), every gradient 0
//   a NaN logit                 that (segment, head) -- that (segment, column) of the softmax -- is NaN; every other one is untouched
//
// Limitation: a segment is walked by ONE wave whatever its length (as mgx_segment_reduce does): a batch of a few very long segments has
// little parallelism.  Splitting long segments over workgroups is not done here.
#include <math.h>

#include "plan_walk.h"

namespace mgx {

// ---------------------------------------------------------------------------------------------- segment softmax
// One wave per segment; CL lanes along the columns (a power of two, at most 64), 64/CL lanes along the rows.  Pass 1: online (m, s) per
// lane, merged over the row lanes in a fixed order; pass 2: the values.  Columns beyond CL are taken in turns.
template <bool BWD>
__global__ __launch_bounds__(kBlock) void seg_softmax_kernel(int64_t S, const int64_t* __restrict__ offsets, int D, int CL,
                                                             const float* __restrict__ x,   // FWD: logits; BWD: out
                                                             const float* __restrict__ dy,  // BWD: d out
                                                             float* __restrict__ y) {       // FWD: out; BWD: d x
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t seg = (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
  if (seg >= S) return;
  const int RL = kWave / CL, rl = lane / CL, cl = lane % CL;
  const int64_t beg = offsets[seg], end = offsets[seg + 1];
  for (int c0 = 0; c0 < D; c0 += CL) {
    const int c = c0 + cl;
    const bool cact = c < D;
    if (!BWD) {
      float m = -INFINITY, s = 0.f;
      if (cact)
        for (int64_t r = beg + rl; r < end; r += RL) {
          const float z = x[r * D + c];
          const float mn = nan_max(m, z);
          s = s * (m == -INFINITY ? 0.f : __expf(m - mn)) + (mn == -INFINITY ? 0.f : __expf(z - mn));
          m = mn;
        }
      for (int off = CL; off < kWave; off <<= 1) {
        const float mo = __shfl_xor(m, off, kWave), so = __shfl_xor(s, off, kWave);
        const float mn = nan_max(m, mo);
        s = s * (m == -INFINITY ? 0.f : __expf(m - mn)) + so * (mo == -INFINITY ? 0.f : __expf(mo - mn));
        m = mn;
      }
      const float is = s == 0.f ? 0.f : 1.f / s;
      if (cact)
        for (int64_t r = beg + rl; r < end; r += RL) y[r * D + c] = m == -INFINITY ? 0.f : __expf(x[r * D + c] - m) * is;
    } else {
      float t = 0.f;
      if (cact)
        for (int64_t r = beg + rl; r < end; r += RL) t += x[r * D + c] * dy[r * D + c];
      for (int off = CL; off < kWave; off <<= 1) t += __shfl_xor(t, off, kWave);
      if (cact)
        for (int64_t r = beg + rl; r < end; r += RL) y[r * D + c] = x[r * D + c] * (dy[r * D + c] - t);
    }
  }
}

static int32_t seg_softmax_check(int64_t S, const int64_t* offsets, int64_t D, const char* who) {
  MGX_CHECK_ARG(S >= 0 && D >= 1, "%s: needs num_segments >= 0 and D >= 1 (got %lld, %lld)", who, (long long)S, (long long)D);
  MGX_CHECK_ARG(S == 0 || offsets != nullptr, "%s: offsets is NULL", who);
  if (D >= (int64_t(1) << 31)) MGX_UNSUPPORTED("%s: D = %lld beyond 32 bits", who, (long long)D);
  return MGX_OK;
}

static int seg_softmax_cl(int64_t D) {
  int cl = 1;
  while (cl < D && cl < kWave) cl <<= 1;
  return cl;
}

static dim3 seg_grid(int64_t S) { return dim3((unsigned)((S + kWavesPerBlock - 1) / kWavesPerBlock)); }

// ---------------------------------------------------------------------------------------------- segment attention
enum { SEG_FWD = 0, SEG_BWD = 1 };

struct SegAttnArgs {
  int64_t S;
  const int64_t* offsets;  // [S + 1]
  int H, D;
  float scale;
  const float* feat;       // [N, feat_ld]
  int64_t feat_ld;
  const float* logits;     // gate mode: [N, H]
  const float* query;      // query mode: [S, D]
  const float* out;        // BWD: out [S, D]
  const float* dout;       // BWD: d out [S, D]
  const float* stat;       // BWD: [S, H, 2] = (m, 1/s)
  float* o_out;            // FWD
  float* o_stat;           // FWD
  float* d_feat;           // BWD, each may be NULL: [N, D]
  float* d_logits;         //                        [N, H]
  float* d_query;          //                        [S, D]
};

// G lanes cover one H*F row (16 bytes each; the lanes past D / 4 of a row whose lane count is no power of two hold zeros and store
// nothing); LPH lanes share a head: F / 4 with several heads, all G with one (then F / 4 need not be a power of two).
template <int G, int LPH, int MODE, bool QUERY>
__global__ __launch_bounds__(kBlock) void seg_attn_kernel(const SegAttnArgs a) {
  constexpr int NB = kWave / G;
  constexpr int U = LaneUnroll<G>::value;
  constexpr int STEP = NB * U;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t seg = (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
  if (seg >= a.S) return;  // the whole wave leaves
  const int sub = lane / G, l = lane % G;
  const int D = a.D, H = a.H;
  const int f = l * 4;
  const bool fact = f < D;
  const int head = fact ? l / LPH : 0;
  const int fo = fact ? f : 0;                      // idle feature lanes re-read the row start; the value is zeroed, never stored
  const bool hlead = fact && (l % LPH) == 0;        // one lane per (row, head)
  const int64_t beg = a.offsets[seg], end = a.offsets[seg + 1];
  const float scale = a.scale;
  // ---- segment constants (idle lanes hold zeros and take part in the lane sums)
  v4f rq = (v4f)(0.f), rd = (v4f)(0.f);
  float c_m = 0.f, c_is = 0.f, c_t = 0.f;
  if (QUERY && fact) rq = *reinterpret_cast<const v4f*>(a.query + seg * D + f);
  if (MODE == SEG_BWD) {
    v4f ov = (v4f)(0.f);
    if (fact) {
      rd = *reinterpret_cast<const v4f*>(a.dout + seg * D + f);
      ov = *reinterpret_cast<const v4f*>(a.out + seg * D + f);
    }
    c_m = a.stat[(seg * H + head) * 2];
    c_is = a.stat[(seg * H + head) * 2 + 1];
    c_t = lanes_sum<LPH>(dot4(rd, ov));
  }
  float run_m = -INFINITY, run_s = 0.f;  // FWD: online softmax state of this lane's head (per lane group)
  v4f acc = (v4f)(0.f);                  // FWD: sum a feat (relative to run_m); BWD query mode: sum dz feat

  for (int64_t j = beg; j < end; j += STEP) {
    v4f x[U];
    float zl[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t r = j + u * NB + sub;
      const int64_t rr = r < end ? r : beg;  // lanes past the end re-read the segment's first row (valid memory), weight zeroed below
      x[u] = *reinterpret_cast<const v4f*>(a.feat + rr * a.feat_ld + fo);
      if (!fact) x[u] = (v4f)(0.f);
      zl[u] = QUERY ? 0.f : a.logits[rr * H + head];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t r = j + u * NB + sub;
      const bool live = r < end;
      const float z = QUERY ? lanes_sum<LPH>(dot4(rq, x[u])) * scale : zl[u];
      if (MODE == SEG_FWD) {
        const float mn = live ? nan_max(run_m, z) : run_m;
        const float rescale = run_m == -INFINITY ? 0.f : __expf(run_m - mn);  // 1 while the maximum stands
        const float pe = (!live || mn == -INFINITY) ? 0.f : __expf(z - mn);   // mn = -inf: only masked logits (-inf) so far
        run_s = run_s * rescale + pe;
        acc = acc * rescale + x[u] * pe;
        run_m = mn;
      } else {
        const float av = live ? __expf(z - c_m) * c_is : 0.f;
        const float dp = lanes_sum<LPH>(dot4(rd, x[u]));
        const float dz = live ? av * (dp - c_t) : 0.f;
        if (QUERY) acc += x[u] * dz;
        if (live) {
          if (a.d_feat && fact) {
            v4f g = rd * av;
            if (QUERY) g += rq * (dz * scale);
            *reinterpret_cast<v4f*>(a.d_feat + r * D + f) = g;
          }
          if (!QUERY && a.d_logits && hlead) a.d_logits[r * H + head] = dz;
        }
      }
    }
  }
  // ---- combine the lane groups in a fixed order, write the segment's row
  if (MODE == SEG_FWD) {
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
    const float is = run_s == 0.f ? 0.f : 1.f / run_s;  // empty or fully masked segments read out 0
    if (fact && sub == 0) *reinterpret_cast<v4f*>(a.o_out + seg * D + f) = acc * is;
    if (hlead && sub == 0) {
      a.o_stat[(seg * H + head) * 2] = run_m == -INFINITY ? 0.f : run_m;
      a.o_stat[(seg * H + head) * 2 + 1] = is;
    }
  } else if (QUERY && a.d_query) {
#pragma unroll
    for (int off = G; off < kWave; off <<= 1) acc += vec_shfl_xor<4>(acc, off);
    if (fact && sub == 0) *reinterpret_cast<v4f*>(a.d_query + seg * D + f) = acc * scale;
  }
}

template <int G, int LPH, int MODE>
static void seg_launch_mode(const SegAttnArgs& a, hipStream_t s) {
  const dim3 grid = seg_grid(a.S), block(kBlock);
  if (a.query) hipLaunchKernelGGL((seg_attn_kernel<G, LPH, MODE, true>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((seg_attn_kernel<G, LPH, MODE, false>), grid, block, 0, s, a);
}

// lph: the lanes of one head -- G for a single head, F / 4 < G otherwise
template <int G, int MODE>
static bool seg_launch_lph(const SegAttnArgs& a, int lph, hipStream_t s) {
  if (lph == G) { seg_launch_mode<G, G, MODE>(a, s); return true; }
  switch (lph) {
#define MGX_SEG_LPH(L) case L: if (L < G) { seg_launch_mode<G, (L < G ? L : G), MODE>(a, s); return true; } return false;
    MGX_SEG_LPH(1) MGX_SEG_LPH(2) MGX_SEG_LPH(4) MGX_SEG_LPH(8) MGX_SEG_LPH(16)
#undef MGX_SEG_LPH
    default: return false;
  }
}

template <int MODE>
static bool seg_launch(const SegAttnArgs& a, int F, hipStream_t s) {
  int G = 1;
  while (G * 4 < a.D) G <<= 1;
  const int lph = a.H == 1 ? G : F / 4;
  switch (G) {
    case 1: return seg_launch_lph<1, MODE>(a, lph, s);
    case 2: return seg_launch_lph<2, MODE>(a, lph, s);
    case 4: return seg_launch_lph<4, MODE>(a, lph, s);
    case 8: return seg_launch_lph<8, MODE>(a, lph, s);
    case 16: return seg_launch_lph<16, MODE>(a, lph, s);
    case 32: return seg_launch_lph<32, MODE>(a, lph, s);
    case 64: return seg_launch_lph<64, MODE>(a, lph, s);
    default: return false;
  }
}

static bool seg_shape_ok(int64_t H, int64_t F, int64_t feat_ld) {
  if (H < 1 || F < 4 || F % 4 != 0 || H * F > 256 || feat_ld % 4 != 0 || feat_ld < H * F) return false;
  return H == 1 || F == 4 || F == 8 || F == 16 || F == 32 || F == 64;
}

static bool aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }

// the checks the two directions share; fills what they share of the arguments
static int32_t seg_attn_check(SegAttnArgs& a, int64_t S, const int64_t* offsets, int64_t H, int64_t F, const float* feat, int64_t feat_ld,
                              const float* logits, const float* query, float scale, const char* who) {
  MGX_CHECK_ARG(S >= 0, "%s: negative num_segments", who);
  MGX_CHECK_ARG(H >= 1 && F >= 1, "%s: H and F must be positive (got H = %lld, F = %lld)", who, (long long)H, (long long)F);
  MGX_CHECK_ARG((logits != nullptr) != (query != nullptr), "%s: exactly one of logits (gate mode) and query (query mode) must be given, got %s",
                who, logits ? "both" : "neither");
  if (!seg_shape_ok(H, F, feat_ld))
    MGX_UNSUPPORTED("%s: needs F %% 4 == 0, H*F <= 256, a row stride that is a multiple of 4 and at least H*F, and F in {4, 8, 16, 32, 64} "
                    "with several heads (got H = %lld, F = %lld, feat_ld = %lld)", who, (long long)H, (long long)F, (long long)feat_ld);
  MGX_CHECK_ARG(S == 0 || offsets != nullptr, "%s: offsets is NULL", who);
  MGX_CHECK_ARG(S == 0 || feat != nullptr, "%s: feat is NULL", who);
  MGX_CHECK_ARG(aligned16(feat) && aligned16(query), "%s: feat and query must be 16-byte aligned", who);
  memset(&a, 0, sizeof(a));
  a.S = S; a.offsets = offsets;
  a.H = (int)H; a.D = (int)(H * F);
  a.scale = query ? scale : 1.f;
  a.feat = feat; a.feat_ld = feat_ld;
  a.logits = logits; a.query = query;
  return MGX_OK;
}

}  // namespace mgx

extern "C" int32_t mgx_segment_softmax_fwd(int64_t num_segments, const int64_t* offsets, int64_t D, const float* x, float* out, void* stream) {
  using namespace mgx;
  MGX_ENTER();
  int32_t st = seg_softmax_check(num_segments, offsets, D, "mgx_segment_softmax_fwd");
  if (st != MGX_OK) return st;
  if (num_segments == 0) return MGX_OK;
  MGX_CHECK_ARG(x && out, "mgx_segment_softmax_fwd: NULL pointer");
  hipLaunchKernelGGL(seg_softmax_kernel<false>, seg_grid(num_segments), dim3(kBlock), 0, (hipStream_t)stream, num_segments, offsets, (int)D,
                     seg_softmax_cl(D), x, (const float*)nullptr, out);
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}

extern "C" int32_t mgx_segment_softmax_bwd(int64_t num_segments, const int64_t* offsets, int64_t D, const float* out, const float* d_out,
                                           float* d_x, void* stream) {
  using namespace mgx;
  MGX_ENTER();
  int32_t st = seg_softmax_check(num_segments, offsets, D, "mgx_segment_softmax_bwd");
  if (st != MGX_OK) return st;
  if (num_segments == 0) return MGX_OK;
  MGX_CHECK_ARG(out && d_out && d_x, "mgx_segment_softmax_bwd: NULL pointer");
  hipLaunchKernelGGL(seg_softmax_kernel<true>, seg_grid(num_segments), dim3(kBlock), 0, (hipStream_t)stream, num_segments, offsets, (int)D,
                     seg_softmax_cl(D), out, d_out, d_x);
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}

extern "C" int32_t mgx_segment_attention_supported(int64_t H, int64_t F, int64_t feat_ld) { return mgx::seg_shape_ok(H, F, feat_ld); }

extern "C" int32_t mgx_segment_attention_fwd(int64_t num_segments, const int64_t* offsets, int64_t H, int64_t F, const float* feat,
                                             int64_t feat_ld, const float* logits, const float* query, float scale, float* out, float* stat,
                                             void* stream) {
  using namespace mgx;
  MGX_ENTER();
  SegAttnArgs a;
  int32_t st = seg_attn_check(a, num_segments, offsets, H, F, feat, feat_ld, logits, query, scale, "mgx_segment_attention_fwd");
  if (st != MGX_OK) return st;
  if (num_segments == 0) return MGX_OK;
  MGX_CHECK_ARG(out && stat, "mgx_segment_attention_fwd: out / stat is NULL");
  MGX_CHECK_ARG(aligned16(out), "mgx_segment_attention_fwd: out must be 16-byte aligned");
  a.o_out = out; a.o_stat = stat;
  if (!seg_launch<SEG_FWD>(a, (int)F, (hipStream_t)stream)) MGX_UNSUPPORTED("mgx_segment_attention_fwd: unsupported head layout");
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}

extern "C" int32_t mgx_segment_attention_bwd(int64_t num_segments, const int64_t* offsets, int64_t H, int64_t F, const float* feat,
                                             int64_t feat_ld, const float* logits, const float* query, float scale, const float* out,
                                             const float* d_out, const float* stat, float* d_feat, float* d_logits, float* d_query,
                                             void* stream) {
  using namespace mgx;
  MGX_ENTER();
  SegAttnArgs a;
  int32_t st = seg_attn_check(a, num_segments, offsets, H, F, feat, feat_ld, logits, query, scale, "mgx_segment_attention_bwd");
  if (st != MGX_OK) return st;
  MGX_CHECK_ARG(!(d_logits && query) && !(d_query && logits), "mgx_segment_attention_bwd: d_logits belongs to gate mode, d_query to query mode");
  if (num_segments == 0 || !(d_feat || d_logits || d_query)) return MGX_OK;
  MGX_CHECK_ARG(out && d_out && stat, "mgx_segment_attention_bwd: out / d_out / stat is NULL");
  MGX_CHECK_ARG(aligned16(out) && aligned16(d_out) && aligned16(d_feat) && aligned16(d_query),
                "mgx_segment_attention_bwd: out, d_out, d_feat and d_query must be 16-byte aligned");
  a.out = out; a.dout = d_out; a.stat = stat;
  a.d_feat = d_feat; a.d_logits = d_logits; a.d_query = d_query;
  if (!seg_launch<SEG_BWD>(a, (int)F, (hipStream_t)stream)) MGX_UNSUPPORTED("mgx_segment_attention_bwd: unsupported head layout");
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}
