// segmha.hip -- dense multi-head attention INSIDE every row segment (gfx950 / MI355X, wave64, fp32 MFMA 16x16x4): the attention of
// dgl.nn.SetTransformerEncoder / SetTransformerDecoder and of a GraphGPS-style global attention layer over a batch of graphs.
//   mgx_segment_mha_fwd   out[i,h,:] = sum_{j in kv-segment g} a[i,j,h] v[j,h,:],  a[i,:,h] = softmax_j(scale <q[i,h,:], k[j,h,:]>)  for the
//                         query rows i of query-segment g; lse[i,h] = m + log(s) of that softmax
//   mgx_segment_mha_bwd   d_q, d_k, d_v from q, k, v, out, lse, d_out
// Two offset arrays of S + 1 entries give the query and the key/value segments (the same array twice: self-attention); segment g of the
// queries meets segment g of the keys and nothing else.  No padded tensor, no n^2 tensor, no edge list, no atomics.
// OUT OF SCOPE: an additive attention bias (Graphormer), masks other than the segment structure, attention-weight dropout inside the
// kernel, fp16 / bf16.
//
// ONE BODY, THREE MODES.  Every kernel has OWN rows, held in registers, and WALKED rows, staged through LDS 64 at a time:
//   forward    own = queries (q),          walked = keys (k, v)
//   d_q        own = queries (q, d_out),   walked = keys (k, v)
//   d_k, d_v   own = keys (k, v),          walked = queries (q, d_out)
// WORK ITEMS (seg_items.h).  An item is a run of 16 * W own rows inside one segment, W = waves of the workgroup; the grid is the host-known
// bound (ceil(N_own / (16 W)) + S) * H, a workgroup finds (segment, head) on the device and leaves beyond the table's end: nothing is read
// back, every entry point can be captured.  W is chosen on the host from N_own / S, the only thing it knows: 2 waves (32 rows) up to an
// average of 32 rows per segment -- a batch of molecules of about 25 nodes does not pay for a 64-row tile it cannot fill --, else 4.
// ONE WAVE OWNS 16 ROWS OF ONE HEAD; the waves of a workgroup share the staged tiles.  LDS holds two stages of both walked operands
// (2 x 2 x 64 x 64 floats = 64 KB at F = 64): the global loads of stage t + 1 are issued into registers before the MFMAs of stage t and
// stored after them, one barrier per stage.  Rows of a stage are padded by 4 floats (F < 64) or rotated by their row number in units of
// 16 bytes (F = 64, where padding would not fit): both the 16-byte row reads and the dword column reads below are free of bank conflicts.
// BOTH GEMMS TRANSPOSED, so that nothing crosses lanes between them.  Lane (c = lane % 16, qq = lane / 16):
//   S^T = walked x own^T:  A = walked tile [16 rows x 4 f] (one ds_read_b128 = four k-steps), B = own rows (registers, loaded once).  The
//        lane gets S^T[walked 4 qq + r][own c], r = 0..3: every value of a lane belongs to ONE own row.
//   forward: the running max / sum of own row c is an in-lane reduction and two xor-shuffles over qq (the sum stays per lane until the
//        end); the rescale factor is in the lane that needs it.  Walked rows past the segment's end get weight 0 (a select, not a product).
//   acc^T = walked^T x P^T:  A = walked[row 4 qq + r][column 16 ct + c] (dword LDS reads, the rows of a 16-row tile in the order 4 qq + r),
//        B = the register the lane already holds.  The accumulators are acc^T[column 4 qq + r][own c]: four consecutive columns of one row,
//        one 16-byte store per row and column tile.
//   backward: p = exp(scale s - lse), dP^T = walked2 x own2^T the same way, dS = p (dP - D) with D[i,h] = <out[i,h,:], d_out[i,h,:]> from a
//        pre-pass; d_q = scale dS K (per query tile), d_k = scale dS^T Q and d_v = P^T dO (per key tile) -- two kernels, fixed summation
//        order, reruns bitwise equal.
// EDGE RULES.  A query whose key segment is empty gets out = 0, lse = 0, d_q = 0; keys whose query segment is empty get d_k = d_v = 0; every
// row of out, lse, d_q, d_k, d_v is written (lengths that add up to the row counts).  Own rows past the end of an item are computed on the
// item's last row and not stored.  A NaN stays inside its (segment, head).  exp and log are the accurate library forms.
#include "common.h"
#include "seg_items.h"

namespace mgx {

constexpr int kMhaStage = 64;  // walked rows per stage
enum { kMhaFwd = 0, kMhaBwdQ = 1, kMhaBwdKV = 2 };

static bool mha_shape_ok(int64_t H, int64_t F) { return H >= 1 && F >= 4 && F <= 64 && F % 4 == 0; }
static bool mha_ld_ok(int64_t H, int64_t F, int64_t ld) { return ld >= H * F && ld % 4 == 0; }

// FJ = column tiles of 16 (F padded with zeros to 16 FJ)
template <int FJ>
struct MhaLds {
  static constexpr int kStride = FJ == 4 ? 64 : 16 * FJ + 4;
  static constexpr int kTile = kMhaStage * kStride;  // floats of one staged operand
  __device__ static __forceinline__ int at(int row, int col) {
    if (FJ == 4) return row * 64 + ((((col >> 2) + row) & 15) << 2) + (col & 3);
    return row * kStride + col;
  }
};

// D[i,h] = <out[i,h,:], d_out[i,h,:]>, one thread per (row, head), the columns in order
__global__ __launch_bounds__(kBlock) void mha_rowdot_kernel(int64_t rows_heads, int F, const float* __restrict__ out,
                                                            const float* __restrict__ d_out, float* __restrict__ D) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= rows_heads) return;
  const v4f* __restrict__ a = reinterpret_cast<const v4f*>(out + i * F);
  const v4f* __restrict__ b = reinterpret_cast<const v4f*>(d_out + i * F);
  float s = 0.f;
  for (int f = 0; f < F / 4; ++f) {
    const v4f x = a[f], y = b[f];
    s += x.x * y.x;
    s += x.y * y.y;
    s += x.z * y.z;
    s += x.w * y.w;
  }
  D[i] = s;
}

// own1 / own2: the operands of the own rows (q | q, d_out | k, v); walk1 / walk2: those of the walked rows (k, v | k, v | q, d_out).
// stat_lse / stat_D: [N_queries, H].  res1 / res2: out, - | d_q, - | d_k, d_v ([N_own, H, F], contiguous; NULL: not stored).
template <int MODE, int FJ, int W>
__global__ __launch_bounds__(64 * W) void segment_mha_kernel(
    int64_t S, int H, int F, const int64_t* __restrict__ own_off, const int64_t* __restrict__ walk_off, const int64_t* __restrict__ table,
    int64_t n_walk, const float* __restrict__ own1, int64_t ld_own1, const float* __restrict__ own2, int64_t ld_own2,
    const float* __restrict__ walk1, int64_t ld_walk1, const float* __restrict__ walk2, int64_t ld_walk2, float scale,
    float* __restrict__ stat_lse, const float* __restrict__ stat_D, float* __restrict__ res1, float* __restrict__ res2) {
  using L = MhaLds<FJ>;
  constexpr int NT = 64 * W, G = 4 * FJ;          // threads; float4 groups of a staged row
  constexpr int NLD = kMhaStage * G / NT;         // float4 per thread, operand and stage
  __shared__ float lds[2][2][L::kTile];           // [stage][operand]
  const int h = blockIdx.x % H;
  int64_t seg, obeg, ocnt;
  if (!seg_item(table, own_off, S, blockIdx.x / H, 16 * W, seg, obeg, ocnt)) return;
  int64_t wbeg = walk_off[seg], wend = walk_off[seg + 1];
  if (!(wbeg >= 0 && wend >= wbeg && wend <= n_walk)) wend = wbeg = 0;  // (a bad segment: as an empty one)
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int c = lane % 16, qq = lane / 16;
  const bool active = 16 * wave < ocnt;  // wave-uniform: a wave without rows only stages
  // ---- own rows: lane (c, qq) holds row c's columns 16 j + 4 qq .. + 3 (k-step (j, t) of S^T = column 16 j + 4 qq + t of both operands)
  int64_t orow = obeg + 16 * wave + c;
  if (orow > obeg + ocnt - 1) orow = obeg + ocnt - 1;
  float r1[FJ][4], r2[FJ][4];
#pragma unroll
  for (int j = 0; j < FJ; ++j) {
    const int col = 16 * j + 4 * qq;
    const bool ok = col < F;
    const v4f a = ok ? *reinterpret_cast<const v4f*>(own1 + orow * ld_own1 + h * F + col) : (v4f)(0.f);
    r1[j][0] = a.x; r1[j][1] = a.y; r1[j][2] = a.z; r1[j][3] = a.w;
    if (MODE != kMhaFwd) {
      const v4f b = ok ? *reinterpret_cast<const v4f*>(own2 + orow * ld_own2 + h * F + col) : (v4f)(0.f);
      r2[j][0] = b.x; r2[j][1] = b.y; r2[j][2] = b.z; r2[j][3] = b.w;
    }
  }
  float own_lse = 0.f, own_D = 0.f;
  if (MODE == kMhaBwdQ) {
    own_lse = stat_lse[orow * H + h];
    own_D = stat_D[orow * H + h];
  }
  v4f acc1[FJ], acc2[FJ];
#pragma unroll
  for (int ct = 0; ct < FJ; ++ct) acc1[ct] = acc2[ct] = (v4f)(0.f);
  float m_run = -INFINITY, l_run = 0.f;  // forward: running max of own row c (all its lanes agree), this lane's share of the sum

  // ---- staging: thread tid moves the float4 groups tid, tid + NT, ... of the 64 x G groups of a stage, both operands
  v4f pre[2][NLD];
  auto fetch = [&](int64_t w0) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int e = tid + i * NT, row = e / G, g = e - row * G;
      const int64_t wr = w0 + row;
      const bool ok = wr < wend && 4 * g < F;
      pre[0][i] = ok ? *reinterpret_cast<const v4f*>(walk1 + wr * ld_walk1 + h * F + 4 * g) : (v4f)(0.f);
      pre[1][i] = ok ? *reinterpret_cast<const v4f*>(walk2 + wr * ld_walk2 + h * F + 4 * g) : (v4f)(0.f);
    }
  };
  auto put = [&](int st) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int e = tid + i * NT, row = e / G, g = e - row * G;
      *reinterpret_cast<v4f*>(&lds[st][0][L::at(row, 4 * g)]) = pre[0][i];
      *reinterpret_cast<v4f*>(&lds[st][1][L::at(row, 4 * g)]) = pre[1][i];
    }
  };
  // S^T tile kt of a staged operand against own registers: element r = <walked row 16 kt + 4 qq + r, own row c>
  auto dots = [&](const float* __restrict__ tile, const float (&own)[FJ][4], int kt) {
    v4f s = (v4f)(0.f);
#pragma unroll
    for (int j = 0; j < FJ; ++j) {
      const v4f a = *reinterpret_cast<const v4f*>(&tile[L::at(16 * kt + c, 16 * j + 4 * qq)]);
#pragma unroll
      for (int t = 0; t < 4; ++t) s = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], own[j][t], s, 0, 0, 0);
    }
    return s;
  };
  // acc^T += tile^T (rows 16 kt ..) x P^T: k-step r pairs the walked row 16 kt + 4 qq + r with p[r]
  auto accumulate = [&](v4f (&acc)[FJ], const float* __restrict__ tile, const v4f& p, int kt) {
#pragma unroll
    for (int ct = 0; ct < FJ; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(tile[L::at(16 * kt + 4 * qq + r, 16 * ct + c)], p[r], acc[ct], 0, 0, 0);
  };

  if (wend > wbeg) {
    fetch(wbeg);
    put(0);
    __syncthreads();
  }
  int st = 0;
  for (int64_t w0 = wbeg; w0 < wend; w0 += kMhaStage, st ^= 1) {
    const bool more = w0 + kMhaStage < wend;
    if (more) fetch(w0 + kMhaStage);  // in flight under this stage's MFMAs
    if (active) {
      const float* __restrict__ t1 = lds[st][0];
      const float* __restrict__ t2 = lds[st][1];
      const int64_t left = wend - w0;
      const int tiles = left >= kMhaStage ? kMhaStage / 16 : (int)((left + 15) >> 4);  // wave-uniform
      if (MODE == kMhaFwd) {
        v4f x[4];
        float tmax = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
          x[kt] = (v4f)(-INFINITY);
          if (kt < tiles) {
            const v4f s = dots(t1, r1, kt);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              x[kt][r] = 16 * kt + 4 * qq + r < left ? s[r] * scale : -INFINITY;
              tmax = fmaxf(tmax, x[kt][r]);
            }
          }
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 16, kWave));
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, kWave));
        const float m_new = fmaxf(m_run, tmax);
        const float m_use = m_new == -INFINITY ? 0.f : m_new;
        const float alpha = expf(m_run - m_use);
        float sum = 0.f;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            x[kt][r] = 16 * kt + 4 * qq + r < left ? expf(x[kt][r] - m_use) : 0.f;
            sum += x[kt][r];
          }
        l_run = l_run * alpha + sum;
        m_run = m_new;
#pragma unroll
        for (int ct = 0; ct < FJ; ++ct) acc1[ct] *= alpha;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
          if (kt < tiles) accumulate(acc1, t2, x[kt], kt);
      } else {
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
          if (kt >= tiles) continue;
          float lse[4], D[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            if (MODE == kMhaBwdQ) {
              lse[r] = own_lse;
              D[r] = own_D;
            } else {  // the statistics of the walked QUERY rows (a row past the end: the last one, its weight is 0)
              int64_t wr = w0 + 16 * kt + 4 * qq + r;
              if (wr > wend - 1) wr = wend - 1;
              lse[r] = stat_lse[wr * H + h];
              D[r] = stat_D[wr * H + h];
            }
          }
          const v4f s = dots(t1, r1, kt);
          const v4f dp = dots(t2, r2, kt);
          v4f p, ds;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const bool ok = 16 * kt + 4 * qq + r < left;
            p[r] = ok ? expf(s[r] * scale - lse[r]) : 0.f;
            ds[r] = ok ? p[r] * (dp[r] - D[r]) : 0.f;
          }
          accumulate(acc1, t1, ds, kt);
          if (MODE == kMhaBwdKV) accumulate(acc2, t2, p, kt);
        }
      }
    }
    if (more) put(st ^ 1);  // (read last in the stage before this one: every wave has passed that stage's barrier)
    __syncthreads();
  }
  if (!active) return;

  // ---- epilogue: accumulator element r of column tile ct = column 16 ct + 4 qq + r of own row c
  const bool mine = 16 * wave + c < ocnt;
  float div = 1.f, mul = scale;
  if (MODE == kMhaFwd) {
    float l = l_run;
    l += __shfl_xor(l, 16, kWave);
    l += __shfl_xor(l, 32, kWave);
    div = l;
    if (mine && qq == 0) stat_lse[orow * H + h] = l == 0.f ? 0.f : m_run + logf(l);
  }
  if (!mine) return;
#pragma unroll
  for (int ct = 0; ct < FJ; ++ct) {
    const int col = 16 * ct + 4 * qq;
    if (col >= F) continue;
    const int64_t at = (orow * H + h) * F + col;
    if (MODE == kMhaFwd) {
      *reinterpret_cast<v4f*>(res1 + at) = div == 0.f ? (v4f)(0.f) : acc1[ct] / div;
    } else {
      if (res1) *reinterpret_cast<v4f*>(res1 + at) = acc1[ct] * mul;
      if (MODE == kMhaBwdKV && res2) *reinterpret_cast<v4f*>(res2 + at) = acc2[ct];
    }
  }
}

static int mha_waves(int64_t n_own, int64_t S) { return n_own > 32 * S ? 4 : 2; }
static int64_t mha_items(int64_t n_own, int64_t S, int W) { return (n_own + 16 * W - 1) / (16 * W) + S; }
static int64_t mha_table_bytes(int64_t S) { return round_up((S + 1) * (int64_t)sizeof(int64_t), 256); }

template <int MODE, int FJ>
static void launch_mha_w(int W, unsigned blocks, hipStream_t s, int64_t S, int H, int F, const int64_t* own_off, const int64_t* walk_off,
                         const int64_t* table, int64_t n_walk, const float* own1, int64_t ld_own1, const float* own2, int64_t ld_own2,
                         const float* walk1, int64_t ld_walk1, const float* walk2, int64_t ld_walk2, float scale, float* stat_lse,
                         const float* stat_D, float* res1, float* res2) {
  if (W == 2)
    hipLaunchKernelGGL((segment_mha_kernel<MODE, FJ, 2>), dim3(blocks), dim3(128), 0, s, S, H, F, own_off, walk_off, table, n_walk, own1,
                       ld_own1, own2, ld_own2, walk1, ld_walk1, walk2, ld_walk2, scale, stat_lse, stat_D, res1, res2);
  else
    hipLaunchKernelGGL((segment_mha_kernel<MODE, FJ, 4>), dim3(blocks), dim3(256), 0, s, S, H, F, own_off, walk_off, table, n_walk, own1,
                       ld_own1, own2, ld_own2, walk1, ld_walk1, walk2, ld_walk2, scale, stat_lse, stat_D, res1, res2);
}

// the scan of the own side's items, then the main grid
template <int MODE>
static int32_t launch_mha(hipStream_t s, int64_t S, int64_t H, int64_t F, int64_t n_own, int64_t n_walk, const int64_t* own_off,
                          const int64_t* walk_off, int64_t* table, const float* own1, int64_t ld_own1, const float* own2, int64_t ld_own2,
                          const float* walk1, int64_t ld_walk1, const float* walk2, int64_t ld_walk2, float scale, float* stat_lse,
                          const float* stat_D, float* res1, float* res2) {
  const int W = mha_waves(n_own, S);
  const int64_t blocks = mha_items(n_own, S, W) * H;
  if (blocks >= (int64_t(1) << 31)) MGX_UNSUPPORTED("mgx_segment_mha: (rows / 32 + segments) x heads must stay below 2^31");
  hipLaunchKernelGGL(seg_items_kernel, dim3(1), dim3(kBlock), 0, s, S, n_own, own_off, (int64_t)(16 * W), table);
  MGX_CHECK_LAUNCH();
#define MGX_MHA(FJ_)                                                                                                                   \
  launch_mha_w<MODE, FJ_>(W, (unsigned)blocks, s, S, (int)H, (int)F, own_off, walk_off, table, n_walk, own1, ld_own1, own2, ld_own2, walk1, \
                          ld_walk1, walk2, ld_walk2, scale, stat_lse, stat_D, res1, res2)
  switch ((F + 15) / 16) {
    case 1: MGX_MHA(1); break;
    case 2: MGX_MHA(2); break;
    case 3: MGX_MHA(3); break;
    default: MGX_MHA(4); break;
  }
#undef MGX_MHA
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}

static int32_t mha_check(const char* who, int64_t S, int64_t Nq, int64_t Nk, int64_t H, int64_t F, int64_t ld_q, int64_t ld_k, int64_t ld_v,
                         const void* q, const void* k, const void* v) {
  MGX_CHECK_ARG(S >= 0 && Nq >= 0 && Nk >= 0 && H >= 1 && F >= 1, "%s: bad sizes (S %lld, Nq %lld, Nk %lld, H %lld, F %lld)", who,
                (long long)S, (long long)Nq, (long long)Nk, (long long)H, (long long)F);
  if (!mha_shape_ok(H, F)) MGX_UNSUPPORTED("%s: needs F %% 4 == 0 and 4 <= F <= 64, got F = %lld", who, (long long)F);
  if (!mha_ld_ok(H, F, ld_q) || !mha_ld_ok(H, F, ld_k) || !mha_ld_ok(H, F, ld_v))
    MGX_UNSUPPORTED("%s: row strides must be multiples of 4 floats and at least H x F (got %lld, %lld, %lld)", who, (long long)ld_q,
                    (long long)ld_k, (long long)ld_v);
  if ((uintptr_t)q % 16 || (uintptr_t)k % 16 || (uintptr_t)v % 16) MGX_UNSUPPORTED("%s: q, k and v must be 16-byte aligned", who);
  const int64_t ld = ld_q > ld_k ? (ld_q > ld_v ? ld_q : ld_v) : (ld_k > ld_v ? ld_k : ld_v);
  if ((Nq > Nk ? Nq : Nk) >= (int64_t(1) << 30) / ld) MGX_UNSUPPORTED("%s: rows x row stride must stay below 2^30", who);
  return MGX_OK;
}

}  // namespace mgx

extern "C" int32_t mgx_segment_mha_supported(int64_t H, int64_t F, int64_t ld_q, int64_t ld_kv) {
  using namespace mgx;
  return mha_shape_ok(H, F) && mha_ld_ok(H, F, ld_q) && mha_ld_ok(H, F, ld_kv) ? 1 : 0;
}

extern "C" int64_t mgx_segment_mha_workspace(int64_t Nq, int64_t Nk, int64_t S, int64_t H) {
  using namespace mgx;
  if (Nq < 0 || Nk < 0 || S < 0 || H < 1) return -1;
  return mha_table_bytes(S) + round_up(Nq * H * (int64_t)sizeof(float), 256);  // one item table at a time, then D [Nq, H]
}

extern "C" int32_t mgx_segment_mha_fwd(int64_t S, const int64_t* q_offsets, const int64_t* kv_offsets, int64_t Nq, int64_t Nk, int64_t H,
                                       int64_t F, const float* q, int64_t ld_q, const float* k, int64_t ld_k, const float* v, int64_t ld_v,
                                       float scale, float* out, float* lse, void* workspace, void* stream) {
  using namespace mgx;
  MGX_ENTER();
  if (int32_t st = mha_check("mgx_segment_mha_fwd", S, Nq, Nk, H, F, ld_q, ld_k, ld_v, q, k, v)) return st;
  if (Nq == 0 || S == 0) return MGX_OK;
  MGX_CHECK_ARG(q_offsets && kv_offsets && q && out && lse && workspace && (Nk == 0 || (k && v)), "mgx_segment_mha_fwd: NULL pointer");
  MGX_CHECK_ARG((uintptr_t)out % 16 == 0, "mgx_segment_mha_fwd: out must be 16-byte aligned");
  return launch_mha<kMhaFwd>((hipStream_t)stream, S, H, F, Nq, Nk, q_offsets, kv_offsets, (int64_t*)workspace, q, ld_q, nullptr, 0, k, ld_k,
                             v, ld_v, scale, lse, nullptr, out, nullptr);
}

extern "C" int32_t mgx_segment_mha_bwd(int64_t S, const int64_t* q_offsets, const int64_t* kv_offsets, int64_t Nq, int64_t Nk, int64_t H,
                                       int64_t F, const float* q, int64_t ld_q, const float* k, int64_t ld_k, const float* v, int64_t ld_v,
                                       float scale, const float* out, const float* lse, const float* d_out, float* d_q, float* d_k,
                                       float* d_v, void* workspace, void* stream) {
  using namespace mgx;
  MGX_ENTER();
  if (int32_t st = mha_check("mgx_segment_mha_bwd", S, Nq, Nk, H, F, ld_q, ld_k, ld_v, q, k, v)) return st;
  if (S == 0 || (Nq == 0 && Nk == 0) || (!d_q && !d_k && !d_v)) return MGX_OK;
  MGX_CHECK_ARG(q_offsets && kv_offsets && workspace && (Nq == 0 || (q && out && lse && d_out)) && (Nk == 0 || (k && v)),
                "mgx_segment_mha_bwd: NULL pointer");
  MGX_CHECK_ARG((uintptr_t)out % 16 == 0 && (uintptr_t)d_out % 16 == 0 && (uintptr_t)d_q % 16 == 0 && (uintptr_t)d_k % 16 == 0 &&
                    (uintptr_t)d_v % 16 == 0, "mgx_segment_mha_bwd: out, d_out and the gradients must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  int64_t* table = (int64_t*)workspace;
  float* D = (float*)((char*)workspace + mha_table_bytes(S));
  const int64_t HF = H * F;
  if (Nq > 0) {
    hipLaunchKernelGGL(mha_rowdot_kernel, dim3((unsigned)((Nq * H + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, Nq * H, (int)F, out, d_out, D);
    MGX_CHECK_LAUNCH();
  }
  if (d_q && Nq > 0)
    if (int32_t st = launch_mha<kMhaBwdQ>(s, S, H, F, Nq, Nk, q_offsets, kv_offsets, table, q, ld_q, d_out, HF, k, ld_k, v, ld_v, scale,
                                          const_cast<float*>(lse), D, d_q, nullptr))
      return st;
  if ((d_k || d_v) && Nk > 0)  // (the table is rebuilt from the key offsets: stream order keeps the two uses apart)
    if (int32_t st = launch_mha<kMhaBwdKV>(s, S, H, F, Nk, Nq, kv_offsets, q_offsets, table, k, ld_k, v, ld_v, q, ld_q, d_out, HF, scale,
                                           const_cast<float*>(lse), D, d_k, d_v))
      return st;
  return MGX_OK;
}
