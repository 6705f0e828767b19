// cfconv.hip -- SchNet's continuous-filter convolution (dgl.nn.CFConv) with no E-sized tensor forward (gfx950 / MI355X, wave64, fp32 MFMA 16x16x4).
//   mgx_edge_filter_sum   out[row(p), f] (+)= Q[indices[p], f] * ssp(ssp(a_p w1^T + b1) w2^T + b2)[f]   over the positions p of a CSR
//   mgx_edge_filter_grad  h1, d pre2, d pre1 (and, in rbf mode, the expansion a) per edge, for the weight and bias gradients
// a_p is ef[eid(p), :K], or exp(-gamma (ef[eid(p)] - centers[k])^2) formed in registers; ssp(t) = max(t, 0) + log1p(exp(-|t|)) - ln 2.
// The forward walks the in-CSR with Q = x; d x is the SAME call on the out-CSR with Q = d out (divided by the in-degree for mean).
//
// WORK ITEM.  `item` consecutive CSR positions (a multiple of 16), one WAVE; the waves of a persistent grid take items round robin and an
// item's tiles of 16 positions in order, so a row's sum runs on in registers from tile to tile.
// A TILE.  Stage 1, [16, K] x [K, F]: lane (c, q) supplies a[c][4 s + q] for k-step s (K padded with zeros to a multiple of 4), straight
// from the ef row or from the expansion; w1 sits in LDS as fragments [s / 4][column tile][lane][s % 4], one ds_read_b128 per four k-steps.
// Bias and ssp in the accumulators (element r of column tile nt in lane (c, q) = row 4 q + r, column 16 nt + c).  The [16, F] result
// goes through a per-wave strip [16][64 + 4], 64 columns at a time, to come back as the A operand of stage 2 (lane (c, q) reads
// h1[c][16 g + 4 q .. + 3], one ds_read_b128 per four k-steps: the k index is relabelled, A and B alike, as lstm_agg.hip does).  Stage 2,
// [16, F] x [F, F] against w2, bias, ssp; times the gathered Q rows.  The next tile's ef values and the ids of the tile after it are
// requested before the current tile's MFMAs.
// w2 IN LDS.  lstm_agg.hip's fragment: (g, nt) holds for lane (c, q) w2[16 nt + c][16 g + 4 q .. + 3] at word q * 68 + 4 c.  The gradient
// kernel reads the SAME copy the other way for d h1 = d pre2 w2: lane (c, q) takes word (c / 4) * 68 + 4 (4 q + w) + c % 4, and the pad of 4
// words per q block puts the 64 lanes on 64 banks.  At F = K = 128: 64 KB (w1) + 68 KB (w2) + 17 KB (strips) of the 160 KB.
// ROW SUMS.  The message tile goes to the strip, 64 columns at a time; lane = column walks its 16 positions in order.  A row wholly inside
// the item is stored (divided by its length for mean); the leading / trailing row that continues in a neighbour item is stored as
// part[item][0 | 1][.]; edge_filter_rows_finish_kernel, one wave per item boundary, adds the partials of a straddling row in item order
// (nnconv.hip's scheme).  No atomics; a row without positions is not written (the caller passes zeros).
// GRADIENT.  One launch over the in-CSR recomputes both stages and forms d pre2 = x[u] g[v] sigmoid(pre2), d h1 = d pre2 w2 (d pre2 through
// the strip as the A operand), d pre1 = d h1 sigmoid(pre1).  h1 and d pre2 are stored by position, d pre1 by edge id -- or, in rbf mode, by
// position beside the recomputed expansion; the caller reduces them with mgx_xty / mgx_column_sum.
#include "common.h"

namespace mgx {

constexpr int kCfWaves = kBlock / kWave;
constexpr int kCfQ = 68;               // words of one q block of a w2 fragment: 64 + 4 of padding
constexpr int kCfFrag = 4 * kCfQ;      // words of a w2 fragment
constexpr int kCfLd = 68;              // row stride of a strip: 64 columns + 4; rows 4 q + r land on banks 16 q + 4 r + c
constexpr int kCfPartLd = 128;         // part[item][2][128]
constexpr int kCfMaxItem = 4096;
constexpr int kCfLdsMax = 160 * 1024;

struct CfArgs {
  const int32_t *indptr, *indices, *eids, *rowpos;
  int nrows, nnz, item, nitems;
  int F, K, K4, rbf, mean;   // K4 = k-steps of stage 1
  const float *Q, *G, *ef, *w1, *b1, *w2, *b2, *cen;
  int64_t ldq, ldg, ldef, ldo;
  float gamma;
  float *out, *part, *h1, *dp2, *dp1, *aexp;
};

// the row of position p: the largest r < nrows with indptr[r] <= p (0 <= p < nnz)
__device__ __forceinline__ int cf_row_of(const int32_t* __restrict__ indptr, int nrows, int p) {
  int lo = 0, hi = nrows;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (indptr[mid] <= p) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ float cf_ssp(float t) { return fmaxf(t, 0.f) + log1pf(expf(-fabsf(t))) - 0.69314718055994530942f; }
__device__ __forceinline__ float cf_sigmoid(float t) { return 1.f / (1.f + expf(-t)); }

template <int FT>
__device__ __forceinline__ int cf_w1_words(int K) { return ((K + 15) / 16) * FT * 256; }

// w1 [F, K], w2 [F, F] (nn.Linear layout) -> the fragments described above; centers -> cen[128], zeros past K
template <int FT>
__device__ __forceinline__ void cf_stage_weights(const CfArgs& a, float* W1l, float* W2l, float* cenl) {
  constexpr int F = 16 * FT;
  const int K = a.K;
  for (int e = threadIdx.x; e < cf_w1_words<FT>(K); e += kBlock) W1l[e] = 0.f;
  __syncthreads();
  for (int e = threadIdx.x; e < F * K; e += kBlock) {
    const int f = e / K, k = e - f * K, s = k >> 2;
    W1l[(((s >> 2) * FT + (f >> 4)) * 64 + (k & 3) * 16 + (f & 15)) * 4 + (s & 3)] = a.w1[e];
  }
  for (int e = threadIdx.x; e < F * F; e += kBlock) {
    const int n = e / F, k = e % F;
    W2l[((k >> 4) * FT + (n >> 4)) * kCfFrag + ((k & 15) >> 2) * kCfQ + (n & 15) * 4 + (k & 3)] = a.w2[e];
  }
  for (int e = threadIdx.x; e < 128; e += kBlock) cenl[e] = (a.rbf && e < K) ? a.cen[e] : 0.f;
  __syncthreads();
}

// ids of the tile at position tp: the edge id of position tp + c (the A operand's row of this lane) and the gathered rows of positions
// tp + 4 q + r (the accumulator's rows); -1 past the item's end
__device__ __forceinline__ void cf_ids(const CfArgs& a, int tp, int pend, int c, int q, int& e, int (&u)[4]) {
  const int p = tp + c;
  e = p < pend ? (a.eids ? a.eids[p] : p) : -1;
#pragma unroll
  for (int r = 0; r < 4; ++r) u[r] = tp + 4 * q + r < pend ? a.indices[tp + 4 * q + r] : -1;
}

// the raw edge values of this lane's A row: ef[e, 4 s + q], or the distance in v[0]
template <int KQ>
__device__ __forceinline__ void cf_load_a(const CfArgs& a, int e, int q, float (&v)[KQ]) {
  if (a.rbf) {
    v[0] = e >= 0 ? a.ef[(int64_t)e * a.ldef] : 0.f;
    return;
  }
  const float* row = a.ef + (int64_t)(e >= 0 ? e : 0) * a.ldef;
#pragma unroll
  for (int s = 0; s < KQ; ++s) v[s] = (e >= 0 && 4 * s + q < a.K) ? row[4 * s + q] : 0.f;
}

// raw values -> the A operand (the expansion in rbf mode); zeros for k >= K
template <int KQ>
__device__ __forceinline__ void cf_expand(const CfArgs& a, const float* cenl, int q, float (&v)[KQ]) {
  if (!a.rbf) return;
  const float d = v[0];
#pragma unroll
  for (int s = 0; s < KQ; ++s) {
    const float t = d - cenl[(4 * s + q) & 127];
    v[s] = 4 * s + q < a.K ? expf(-a.gamma * (t * t)) : 0.f;
  }
}

// acc[nt] = a w1^T for the 16 rows of the tile
template <int FT, int KQ>
__device__ __forceinline__ void cf_stage1(const CfArgs& a, const float* W1l, int lo, const float (&av)[KQ], v4f (&acc)[FT]) {
#pragma unroll
  for (int nt = 0; nt < FT; ++nt) acc[nt] = (v4f)(0.f);
#pragma unroll
  for (int g = 0; g < KQ / 4; ++g) {
    if (4 * g >= a.K4) break;  // wave-uniform
#pragma unroll
    for (int nt = 0; nt < FT; ++nt) {
      const v4f b = *reinterpret_cast<const v4f*>(&W1l[((g * FT + nt) * 64 + lo) * 4]);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (4 * g + i < a.K4) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[4 * g + i], b[i], acc[nt], 0, 0, 0);
    }
  }
}

// columns 64 h .. of a [16, F] tile in the accumulator layout -> the wave's strip
template <int FT>
__device__ __forceinline__ void cf_to_strip(float* strip, int h, int c, int q, const v4f (&v)[FT]) {
  __builtin_amdgcn_wave_barrier();  // every lane has read what the strip held
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (4 * h + j < FT) {
#pragma unroll
      for (int r = 0; r < 4; ++r) strip[(4 * q + r) * kCfLd + 16 * j + c] = v[4 * h + j < FT ? 4 * h + j : 0][r];
    }
  __builtin_amdgcn_wave_barrier();
}

// acc[nt] = h1 w2^T, h1 handed over through the strip 64 columns at a time
template <int FT>
__device__ __forceinline__ void cf_stage2(const float* W2l, float* strip, int lo, int c, int q, const v4f (&h1)[FT], v4f (&acc)[FT]) {
#pragma unroll
  for (int nt = 0; nt < FT; ++nt) acc[nt] = (v4f)(0.f);
  const float* Wf = W2l + lo + q * kCfQ + 4 * c;
#pragma unroll
  for (int h = 0; h < (FT + 3) / 4; ++h) {
    cf_to_strip<FT>(strip, h, c, q, h1);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (4 * h + j < FT) {
        const v4f av = *reinterpret_cast<const v4f*>(&strip[c * kCfLd + 16 * j + 4 * q + lo]);
#pragma unroll
        for (int nt = 0; nt < FT; ++nt) {
          const v4f b = *reinterpret_cast<const v4f*>(&Wf[((4 * h + j) * FT + nt) * kCfFrag]);
#pragma unroll
          for (int w = 0; w < 4; ++w) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[w], b[w], acc[nt], 0, 0, 0);
        }
      }
  }
}

template <int FT>
__device__ __forceinline__ void cf_gather(const float* __restrict__ Q, int64_t ld, const int (&u)[4], int c, float (&x)[FT][4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int nt = 0; nt < FT; ++nt) x[nt][r] = u[r] >= 0 ? Q[(int64_t)u[r] * ld + 16 * nt + c] : 0.f;
}

template <int FT>
__device__ __forceinline__ void cf_bias(const float* b, int c, float (&v)[FT]) {
#pragma unroll
  for (int nt = 0; nt < FT; ++nt) v[nt] = b ? b[16 * nt + c] : 0.f;
}

// FT = column tiles of 16, KQ = k-steps of stage 1 held in registers (16: K <= 64, 32: K <= 128)
template <int FT, int KQ>
__global__ __launch_bounds__(kBlock) void edge_filter_sum_kernel(const CfArgs a) {
  constexpr int NH = (FT + 3) / 4;
  extern __shared__ __attribute__((aligned(16))) float cf_lds[];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int c = lane & 15, q = lane >> 4;
  float* W1l = cf_lds;
  float* W2l = W1l + cf_w1_words<FT>(a.K);
  float* cenl = W2l + FT * FT * kCfFrag;
  float* strip = cenl + 128 + wave * 16 * kCfLd;
  cf_stage_weights<FT>(a, W1l, W2l, cenl);
  float b1v[FT], b2v[FT];
  cf_bias<FT>(a.b1, c, b1v);
  cf_bias<FT>(a.b2, c, b2v);

  for (int it = blockIdx.x * kCfWaves + wave; it < a.nitems; it += gridDim.x * kCfWaves) {
    const int p0 = it * a.item, pend = p0 + a.item < a.nnz ? p0 + a.item : a.nnz;
    // the row walk's state (wave-uniform): the row of the next position and its ends
    int row = __builtin_amdgcn_readfirstlane(cf_row_of(a.indptr, a.nrows, p0));
    int rb = a.indptr[row], re = a.indptr[row + 1];
    float rs[NH];
#pragma unroll
    for (int h = 0; h < NH; ++h) rs[h] = 0.f;
    auto flush = [&](int h, int r_, int rb_, int re_, float s) {
      const int col = 64 * h + lane;
      if (col >= 16 * FT) return;
      if (rb_ >= p0 && re_ <= pend)
        a.out[(int64_t)r_ * a.ldo + col] = a.mean ? s / (float)(re_ - rb_) : s;
      else
        a.part[((int64_t)it * 2 + (rb_ < p0 ? 0 : 1)) * kCfPartLd + col] = s;
    };

    int e1, u0[4], u1[4], e2, u2[4];
    float av[KQ], an[KQ];
    cf_ids(a, p0, pend, c, q, e1, u0);
    cf_load_a<KQ>(a, e1, q, av);
    cf_ids(a, p0 + 16, pend, c, q, e1, u1);
    for (int tp = p0; tp < pend; tp += 16) {
      float xg[FT][4];
      cf_gather<FT>(a.Q, a.ldq, u0, c, xg);  // used after stage 2
      cf_load_a<KQ>(a, e1, q, an);           // tile + 1, in flight under the MFMAs below
      cf_ids(a, tp + 32, pend, c, q, e2, u2);
      int lo = lane;  // the weights stay in LDS: an offset the compiler cannot prove loop-invariant keeps the fragments out of registers
      asm volatile("" : "+v"(lo));
      cf_expand<KQ>(a, cenl, q, av);
      v4f h1[FT], f2[FT];
      cf_stage1<FT, KQ>(a, W1l, lo, av, h1);
#pragma unroll
      for (int nt = 0; nt < FT; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) h1[nt][r] = cf_ssp(h1[nt][r] + b1v[nt]);
      cf_stage2<FT>(W2l, strip, lo - lane, c, q, h1, f2);
#pragma unroll
      for (int nt = 0; nt < FT; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) f2[nt][r] = xg[nt][r] * cf_ssp(f2[nt][r] + b2v[nt]);
      // ---- the row sums: lane = column, the tile's positions in order
      const int n = pend - tp < 16 ? pend - tp : 16;
      int row1 = row, rb1 = rb, re1 = re;
#pragma unroll
      for (int h = 0; h < NH; ++h) {
        cf_to_strip<FT>(strip, h, c, q, f2);
        row1 = row; rb1 = rb; re1 = re;
        for (int j = 0; j < n; ++j) {
          while (tp + j >= re1) {  // the row is over; rows without positions are passed by
            if (re1 > rb1) { flush(h, row1, rb1, re1, rs[h]); rs[h] = 0.f; }
            ++row1; rb1 = re1; re1 = a.indptr[row1 + 1];
          }
          rs[h] += strip[j * kCfLd + lane];
        }
      }
      row = row1; rb = rb1; re = re1;
#pragma unroll
      for (int s = 0; s < KQ; ++s) av[s] = an[s];
#pragma unroll
      for (int r = 0; r < 4; ++r) { u0[r] = u1[r]; u1[r] = u2[r]; }
      e1 = e2;
    }
#pragma unroll
    for (int h = 0; h < NH; ++h) flush(h, row, rb, re, rs[h]);  // the row of the item's last position
  }
}

// One wave per item boundary j (position j * item): the row that straddles it, if this is the first boundary inside that row, is the sum
// of its trailing partial in the item it starts in and the leading partials of the items after, in item order.
__global__ __launch_bounds__(kBlock) void edge_filter_rows_finish_kernel(const int32_t* __restrict__ indptr, int nrows, int nitems, int item,
                                                                         int N, int mean, const float* __restrict__ part,
                                                                         float* __restrict__ out, int64_t ldo) {
  const int j = blockIdx.x * kWavesPerBlock + threadIdx.x / kWave + 1;
  if (j >= nitems) return;
  const int p = j * item;
  const int r = cf_row_of(indptr, nrows, p);
  const int rb = indptr[r], re = indptr[r + 1];
  const int t0 = rb / item;
  if (rb >= p || t0 + 1 != j) return;
  const int t1 = (re - 1) / item;
  for (int n = threadIdx.x & (kWave - 1); n < N; n += kWave) {
    float s = part[((int64_t)t0 * 2 + 1) * kCfPartLd + n];
    for (int t = t0 + 1; t <= t1; ++t) s += part[(int64_t)t * 2 * kCfPartLd + n];
    out[(int64_t)r * ldo + n] = mean ? s / (float)(re - rb) : s;
  }
}

template <int FT, int KQ>
__global__ __launch_bounds__(kBlock) void edge_filter_grad_kernel(const CfArgs a) {
  constexpr int F = 16 * FT;
  extern __shared__ __attribute__((aligned(16))) float cf_lds[];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int c = lane & 15, q = lane >> 4;
  float* W1l = cf_lds;
  float* W2l = W1l + cf_w1_words<FT>(a.K);
  float* cenl = W2l + FT * FT * kCfFrag;
  float* strip = cenl + 128 + wave * 16 * kCfLd;
  cf_stage_weights<FT>(a, W1l, W2l, cenl);
  float b1v[FT], b2v[FT];
  cf_bias<FT>(a.b1, c, b1v);
  cf_bias<FT>(a.b2, c, b2v);

  for (int it = blockIdx.x * kCfWaves + wave; it < a.nitems; it += gridDim.x * kCfWaves) {
    const int p0 = it * a.item, pend = p0 + a.item < a.nnz ? p0 + a.item : a.nnz;
    int e0, e1, u0[4], u1[4], e2, u2[4];
    float av[KQ], an[KQ];
    cf_ids(a, p0, pend, c, q, e0, u0);
    cf_load_a<KQ>(a, e0, q, av);
    cf_ids(a, p0 + 16, pend, c, q, e1, u1);
    for (int tp = p0; tp < pend; tp += 16) {
      float xg[FT][4];
      {
        int v[4];
        float gg[FT][4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = tp + 4 * q + r < pend ? a.rowpos[tp + 4 * q + r] : -1;
        cf_gather<FT>(a.Q, a.ldq, u0, c, xg);
        cf_gather<FT>(a.G, a.ldg, v, c, gg);
#pragma unroll
        for (int nt = 0; nt < FT; ++nt)
#pragma unroll
          for (int r = 0; r < 4; ++r) xg[nt][r] *= gg[nt][r];
      }
      cf_load_a<KQ>(a, e1, q, an);
      cf_ids(a, tp + 32, pend, c, q, e2, u2);
      int lo = lane;
      asm volatile("" : "+v"(lo));
      cf_expand<KQ>(a, cenl, q, av);
      if (a.rbf && e0 >= 0) {  // the expansion by position, for d w1 = d pre1^T a
        float* dst = a.aexp + (int64_t)(tp + c) * a.K;
#pragma unroll
        for (int s = 0; s < KQ; ++s)
          if (4 * s + q < a.K) dst[4 * s + q] = av[s];
      }
      v4f h1[FT], s1[FT], d2[FT], d1[FT];
      cf_stage1<FT, KQ>(a, W1l, lo, av, h1);
#pragma unroll
      for (int nt = 0; nt < FT; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float t = h1[nt][r] + b1v[nt];
          h1[nt][r] = cf_ssp(t);
          s1[nt][r] = cf_sigmoid(t);
        }
      cf_stage2<FT>(W2l, strip, lo - lane, c, q, h1, d2);
#pragma unroll
      for (int nt = 0; nt < FT; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) d2[nt][r] = xg[nt][r] * cf_sigmoid(d2[nt][r] + b2v[nt]);
      // d h1 = d pre2 w2: the reduction runs over the columns of d pre2, k-step (j, w) gives lane q the column 64 h + 16 j + 4 q + w
#pragma unroll
      for (int kt = 0; kt < FT; ++kt) d1[kt] = (v4f)(0.f);
      const float* Wb = W2l + (lo - lane) + (c / 4) * kCfQ + 16 * q + c % 4;
#pragma unroll
      for (int h = 0; h < (FT + 3) / 4; ++h) {
        cf_to_strip<FT>(strip, h, c, q, d2);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (4 * h + j < FT) {
            const v4f dv = *reinterpret_cast<const v4f*>(&strip[c * kCfLd + 16 * j + 4 * q + (lo - lane)]);
#pragma unroll
            for (int w = 0; w < 4; ++w)
#pragma unroll
              for (int kt = 0; kt < FT; ++kt)
                d1[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(dv[w], Wb[(kt * FT + 4 * h + j) * kCfFrag + 4 * w], d1[kt], 0, 0, 0);
          }
      }
      // ---- stores: row 4 q + r of the tile, columns 16 nt + c
      int er[4];  // where d pre1 goes: the edge id, or the position in rbf mode
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int p = tp + 4 * q + r;
        er[r] = p >= pend ? -1 : (a.rbf || !a.eids) ? p : a.eids[p];
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (er[r] < 0) continue;
        const int64_t p = tp + 4 * q + r;
#pragma unroll
        for (int nt = 0; nt < FT; ++nt) {
          a.h1[p * F + 16 * nt + c] = h1[nt][r];
          a.dp2[p * F + 16 * nt + c] = d2[nt][r];
          a.dp1[(int64_t)er[r] * F + 16 * nt + c] = d1[nt][r] * s1[nt][r];
        }
      }
#pragma unroll
      for (int s = 0; s < KQ; ++s) av[s] = an[s];
#pragma unroll
      for (int r = 0; r < 4; ++r) { u0[r] = u1[r]; u1[r] = u2[r]; }
      e0 = e1; e1 = e2;
    }
  }
}

static bool cf_shape_ok(int64_t F, int64_t K) { return F >= 16 && F <= 128 && F % 16 == 0 && K >= 1 && K <= 128; }
static bool cf_item_ok(int64_t item) { return item >= 16 && item <= kCfMaxItem && item % 16 == 0; }
static size_t cf_lds_bytes(int64_t F, int64_t K) {
  const int64_t FT = F / 16;
  return (size_t)(((K + 15) / 16) * FT * 256 + FT * FT * kCfFrag + 128 + kCfWaves * 16 * kCfLd) * sizeof(float);
}

// a persistent grid: as many workgroups as a CU's LDS holds (four at most) per CU, an item per wave at least
static int cf_grid(int64_t nitems, size_t lds) {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) n = 256;
    cus = n;
  }
  int per = (int)(kCfLdsMax / lds);
  per = per < 1 ? 1 : per > 4 ? 4 : per;
  const int64_t want = (nitems + kCfWaves - 1) / kCfWaves;
  return (int)(want < (int64_t)cus * per ? want : (int64_t)cus * per);
}

template <typename Kn>
static int32_t cf_launch(Kn kernel, const CfArgs& a, size_t lds, hipStream_t s) {
  MGX_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kernel, dim3((unsigned)cf_grid(a.nitems, lds)), dim3(kBlock), lds, s, a);
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}

template <int FT>
static int32_t cf_launch_ft(bool grad, const CfArgs& a, size_t lds, hipStream_t s) {
  if (a.K <= 64) return grad ? cf_launch(edge_filter_grad_kernel<FT, 16>, a, lds, s) : cf_launch(edge_filter_sum_kernel<FT, 16>, a, lds, s);
  return grad ? cf_launch(edge_filter_grad_kernel<FT, 32>, a, lds, s) : cf_launch(edge_filter_sum_kernel<FT, 32>, a, lds, s);
}

static int32_t cf_dispatch(bool grad, const CfArgs& a, hipStream_t s) {
  const size_t lds = cf_lds_bytes(a.F, a.K);
  switch (a.F / 16) {
    case 1: return cf_launch_ft<1>(grad, a, lds, s);
    case 2: return cf_launch_ft<2>(grad, a, lds, s);
    case 3: return cf_launch_ft<3>(grad, a, lds, s);
    case 4: return cf_launch_ft<4>(grad, a, lds, s);
    case 5: return cf_launch_ft<5>(grad, a, lds, s);
    case 6: return cf_launch_ft<6>(grad, a, lds, s);
    case 7: return cf_launch_ft<7>(grad, a, lds, s);
    default: return cf_launch_ft<8>(grad, a, lds, s);
  }
}

static int32_t cf_fill(CfArgs& a, const mgx_csr* csr, int64_t F, int64_t K, const float* Q, int64_t ldq, const float* ef, int64_t ldef,
                       const float* w1, const float* b1, const float* w2, const float* b2, const float* centers, float gamma,
                       int64_t item_edges, const char* who) {
  MGX_CHECK_ARG(csr && csr->num_rows >= 0 && csr->num_cols >= 0 && csr->nnz >= 0, "%s: bad CSR", who);
  MGX_CHECK_ARG(csr->nnz == 0 || (csr->indptr && csr->indices), "%s: CSR without indptr / indices", who);
  if (csr->idx_bits != 32) MGX_UNSUPPORTED("%s: needs 32-bit graph indices", who);
  if (csr->nnz == 0) MGX_UNSUPPORTED("%s: needs at least one edge", who);
  if (!cf_shape_ok(F, K)) MGX_UNSUPPORTED("%s: needs F a multiple of 16 in 16 .. 128 and 1 <= K <= 128 (got %lld, %lld)", who, (long long)F, (long long)K);
  const int64_t lim = int64_t(1) << 30;
  if (csr->nnz >= lim / 128 * 16 || csr->num_rows >= lim || csr->num_cols >= lim) MGX_UNSUPPORTED("%s: needs fewer than 2^27 edges and 2^30 rows", who);
  MGX_CHECK_ARG(Q && ef && w1 && w2, "%s: NULL pointer", who);
  MGX_CHECK_ARG(cf_item_ok(item_edges), "%s: item_edges must be a multiple of 16 in 16 .. %d, got %lld", who, kCfMaxItem, (long long)item_edges);
  MGX_CHECK_ARG(ldq >= F && (centers ? ldef >= 1 : ldef >= K), "%s: leading dimensions smaller than the operands", who);
  memset(&a, 0, sizeof(a));
  a.indptr = (const int32_t*)csr->indptr; a.indices = (const int32_t*)csr->indices; a.eids = (const int32_t*)csr->eids;
  a.nrows = (int)csr->num_rows; a.nnz = (int)csr->nnz; a.item = (int)item_edges; a.nitems = (int)((csr->nnz + item_edges - 1) / item_edges);
  a.F = (int)F; a.K = (int)K; a.K4 = (int)((K + 3) / 4); a.rbf = centers ? 1 : 0;
  a.Q = Q; a.ldq = ldq; a.ef = ef; a.ldef = ldef; a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2; a.cen = centers; a.gamma = gamma;
  return MGX_OK;
}

}  // namespace mgx

extern "C" int32_t mgx_edge_filter_supported(const mgx_csr* csr, int64_t F, int64_t K) {
  using namespace mgx;
  const int64_t lim = int64_t(1) << 30;
  return (csr && csr->idx_bits == 32 && csr->nnz > 0 && cf_shape_ok(F, K) && csr->nnz < lim / 128 * 16 && csr->num_rows < lim && csr->num_cols < lim) ? 1 : 0;
}

extern "C" int64_t mgx_edge_filter_workspace(int64_t nnz, int64_t item_edges) {
  using namespace mgx;
  if (nnz < 0 || !cf_item_ok(item_edges)) return -1;
  return (nnz + item_edges - 1) / item_edges * 2 * kCfPartLd * (int64_t)sizeof(float);
}

extern "C" int32_t mgx_edge_filter_sum(const mgx_csr* csr, int64_t F, int64_t K, const float* Q, int64_t ldq, const float* ef, int64_t ldef,
                                       const float* w1, const float* b1, const float* w2, const float* b2, const float* centers, float gamma,
                                       int32_t mean, float* out, int64_t ldo, int64_t item_edges, void* workspace, void* stream) {
  using namespace mgx;
  MGX_ENTER();
  CfArgs a;
  const int32_t st = cf_fill(a, csr, F, K, Q, ldq, ef, ldef, w1, b1, w2, b2, centers, gamma, item_edges, "mgx_edge_filter_sum");
  if (st != MGX_OK) return st;
  MGX_CHECK_ARG(out && workspace && ldo >= F, "mgx_edge_filter_sum: out or workspace missing, or ldo < F");
  a.out = out; a.ldo = ldo; a.part = (float*)workspace; a.mean = mean ? 1 : 0;
  hipStream_t s = (hipStream_t)stream;
  const int32_t r = cf_dispatch(false, a, s);
  if (r != MGX_OK) return r;
  if (a.nitems > 1) {
    hipLaunchKernelGGL(edge_filter_rows_finish_kernel, dim3((unsigned)((a.nitems - 1 + kWavesPerBlock - 1) / kWavesPerBlock)), dim3(kBlock), 0, s,
                       a.indptr, a.nrows, a.nitems, a.item, a.F, a.mean, (const float*)a.part, out, ldo);
    MGX_CHECK_LAUNCH();
  }
  note_spmm_kernel("edge_filter_sum");
  return MGX_OK;
}

extern "C" int32_t mgx_edge_filter_grad(const mgx_csr* csc, const int32_t* row_of_position, int64_t F, int64_t K, const float* x, int64_t ldx,
                                        const float* g, int64_t ldg, const float* ef, int64_t ldef, const float* w1, const float* b1,
                                        const float* w2, const float* b2, const float* centers, float gamma, float* h1, float* d_pre2,
                                        float* d_pre1, float* expansion, int64_t item_edges, void* stream) {
  using namespace mgx;
  MGX_ENTER();
  CfArgs a;
  const int32_t st = cf_fill(a, csc, F, K, x, ldx, ef, ldef, w1, b1, w2, b2, centers, gamma, item_edges, "mgx_edge_filter_grad");
  if (st != MGX_OK) return st;
  MGX_CHECK_ARG(row_of_position && g && h1 && d_pre2 && d_pre1 && ldg >= F, "mgx_edge_filter_grad: NULL pointer, or ldg < F");
  MGX_CHECK_ARG((centers == nullptr) == (expansion == nullptr), "mgx_edge_filter_grad: the expansion goes with centers");
  a.rowpos = row_of_position; a.G = g; a.ldg = ldg; a.h1 = h1; a.dp2 = d_pre2; a.dp1 = d_pre1; a.aexp = expansion;
  const int32_t r = cf_dispatch(true, a, (hipStream_t)stream);
  if (r != MGX_OK) return r;
  note_spmm_kernel("edge_filter_grad");
  return MGX_OK;
}
