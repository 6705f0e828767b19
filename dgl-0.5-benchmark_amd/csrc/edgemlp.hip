// edgemlp.hip -- a one- or two-layer MLP on every edge under a max or a sum (PointNet++ set abstraction, dgl.nn.PointNetConv) with no
// E-sized tensor forward (gfx950 / MI355X, wave64, fp32 MFMA 16x16x4).
//   mgx_edge_mlp_reduce  out[row(p), f] = max | sum over the positions p of a row of e_L[p, f],
//                        e_0 = relu(u[indices[p]] - v[row(p)]),  e_l = relu(e_{l-1} W_l^T + b_l),  l = 1 .. L,  L = 1 | 2
//   mgx_edge_mlp_grad    e_{l-1} and d pre_l per position and d e_0 per edge, for the weight, bias and node gradients
// cfconv.hip's conventions: a WORK ITEM is `item` consecutive CSR positions (a multiple of 16) walked by one WAVE in tiles of 16, the waves
// of a persistent grid take items round robin; weights sit in LDS as MFMA fragments; a per-wave strip [16][64 + 4] turns an accumulator
// tile back into an A operand; a row that straddles items leaves partials that edge_mlp_rows_finish_kernel merges in item order.
// THE A OPERAND OF LAYER 1.  Lane (c, q) holds row c of the tile, columns 16 g + 4 q .. + 3 of every 16-column group g: one 16-byte load
// of the u row and one of the v row per group, subtract and ReLU in registers -- e_0 never exists in memory.  The k index is relabelled, A
// and B alike: k-step (g, w) pairs column 16 g + 4 q + w of lane q with the same column of the weights.  The rows of tile + 1 and the ids of
// tile + 2 are requested before the current tile's MFMAs.
// WEIGHTS IN LDS.  One layout for every layer, W [N, K] in nn.Linear's: fragment (g, nt) holds for lane (c, q) W[16 nt + c][16 g + 4 q .. + 3]
// at word q * 68 + 4 c (one ds_read_b128 per four k-steps).  The gradient reads the SAME copy the other way for d e_{l-1} = d pre_l W_l:
// lane (c, q) takes word (c / 4) * 68 + 4 (4 q + w) + c % 4; the pad of 4 words per q block puts the 64 lanes on 64 banks.
// SLABS.  The LAST layer's output columns are split into slabs of at most 128: 128-128-256 needs 64 K words of W_1 and W_2, 192 KB; with a
// slab it is 68 + 68 + 17 KB of the 160 KB.  Forward: the slab is the grid's second dimension, a workgroup recomputes the cheap first GEMM
// for its slab.  Gradient: one grid, the slabs in turn inside the kernel (the last layer's fragments are staged again per slab); a wave
// meets the same items in every turn and adds its own partial d e_{L-1} of the turn before through `acc`, so no other wave's data is read.
// REDUCE.  The e_L tile goes to the strip, 64 columns at a time; lane = column walks its 16 positions in order.  Max keeps a value and the
// position of its FIRST maximum (strict > in position order; the finish kernel's merge is strict > in item order).  No atomics: reruns
// are bitwise equal.  A row without positions is not written (the caller passes zeros).
#include "common.h"

namespace mgx {

constexpr int kEmWaves = kBlock / kWave;
constexpr int kEmQ = 68;               // words of one q block of a fragment: 64 + 4 of padding
constexpr int kEmFrag = 4 * kEmQ;      // words of a fragment
constexpr int kEmLd = 68;              // row stride of a strip: 64 columns + 4
constexpr int kEmSlab = 128;           // columns of the last layer one workgroup holds
constexpr int kEmPartLd = 256;         // part[item][2][256]
constexpr int kEmMaxItem = 4096;
constexpr int kEmLdsMax = 160 * 1024;

struct EmArgs {
  const int32_t *indptr, *indices, *eids, *rowpos;
  int nrows, nnz, item, nitems;
  int H0, H1, HL, sum;   // H1: the hidden width (two layers only)
  const float *u, *v, *w1, *b1, *w2, *b2, *G;
  int64_t ldu, ldv, ldo, ldg;
  float *out, *part;
  int32_t *arg, *parg;
  const int32_t* argin;
  float *e0, *de0, *e1, *dp1, *dpl, *acc;
};

// the row of position p: the largest r < nrows with indptr[r] <= p (0 <= p < nnz)
__device__ __forceinline__ int em_row_of(const int32_t* __restrict__ indptr, int nrows, int p) {
  int lo = 0, hi = nrows;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (indptr[mid] <= p) lo = mid; else hi = mid;
  }
  return lo;
}

// rows n0 .. n0 + 16 NT of W [., K] -> the fragments described above (the pad words are never read)
__device__ __forceinline__ void em_stage(const float* __restrict__ W, int K, int n0, int NT, float* Wl) {
  for (int e = threadIdx.x; e < 16 * NT * K; e += kBlock) {
    const int n = e / K, k = e - n * K;
    Wl[((k >> 4) * NT + (n >> 4)) * kEmFrag + ((k & 15) >> 2) * kEmQ + (n & 15) * 4 + (k & 3)] = W[(int64_t)(n0 + n) * K + k];
  }
}

template <int MT>
__device__ __forceinline__ void em_bias(const float* b, int n0, int NT, int c, float (&v)[MT]) {
#pragma unroll
  for (int nt = 0; nt < MT; ++nt) v[nt] = (b && nt < NT) ? b[n0 + 16 * nt + c] : 0.f;
}

// this lane's A row of the tile at tp: the source and the destination of position tp + c; -1 past the item's end
__device__ __forceinline__ void em_ids(const EmArgs& a, int tp, int pend, int c, int& s, int& d) {
  const int p = tp + c;
  s = p < pend ? a.indices[p] : -1;
  d = p < pend ? a.rowpos[p] : -1;
}

// columns 16 g + 4 q .. + 3 of row i of X for the KT groups; zeros for i < 0 and past KT
template <int MT>
__device__ __forceinline__ void em_load(const float* __restrict__ X, int64_t ld, int i, int KT, int q, v4f (&x)[MT]) {
  const float* row = X + (int64_t)(i >= 0 ? i : 0) * ld + 4 * q;
#pragma unroll
  for (int g = 0; g < MT; ++g) x[g] = (i >= 0 && g < KT) ? *reinterpret_cast<const v4f*>(row + 16 * g) : (v4f)(0.f);
}

// acc[nt] = A W^T for the tile, A from registers (the layout of em_load), nt < NT
template <int MT>
__device__ __forceinline__ void em_gemm_regs(const float* Wl, int KT, int NT, int c, int q, const v4f (&av)[MT], v4f (&acc)[MT]) {
#pragma unroll
  for (int nt = 0; nt < MT; ++nt) acc[nt] = (v4f)(0.f);
  const float* Wf = Wl + q * kEmQ + 4 * c;
#pragma unroll
  for (int g = 0; g < MT; ++g)
    if (g < KT) {  // wave-uniform
#pragma unroll
      for (int nt = 0; nt < MT; ++nt)
        if (nt < NT) {
          const v4f b = *reinterpret_cast<const v4f*>(&Wf[(g * NT + nt) * kEmFrag]);
#pragma unroll
          for (int w = 0; w < 4; ++w) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[g][w], b[w], acc[nt], 0, 0, 0);
        }
    }
}

// columns 64 h .. of a [16, 16 NT] tile in the accumulator layout (element r of tile nt in lane (c, q) = row 4 q + r, column 16 nt + c)
// -> the wave's strip
template <int MT>
__device__ __forceinline__ void em_to_strip(float* strip, int h, int NT, int c, int q, const v4f (&v)[MT]) {
  __builtin_amdgcn_wave_barrier();  // every lane has read what the strip held
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (4 * h + j < MT && 4 * h + j < NT) {
#pragma unroll
      for (int r = 0; r < 4; ++r) strip[(4 * q + r) * kEmLd + 16 * j + c] = v[4 * h + j < MT ? 4 * h + j : 0][r];
    }
  __builtin_amdgcn_wave_barrier();
}

// acc[nt] = h W^T, h [16, 16 KT] handed over through the strip 64 columns at a time
template <int MT>
__device__ __forceinline__ void em_gemm_strip(const float* Wl, float* strip, int KT, int NT, int c, int q, const v4f (&h)[MT], v4f (&acc)[MT]) {
#pragma unroll
  for (int nt = 0; nt < MT; ++nt) acc[nt] = (v4f)(0.f);
  const float* Wf = Wl + q * kEmQ + 4 * c;
#pragma unroll
  for (int hh = 0; hh < (MT + 3) / 4; ++hh)
    if (4 * hh < KT) {
      em_to_strip<MT>(strip, hh, KT, c, q, h);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (4 * hh + j < MT && 4 * hh + j < KT) {
          const v4f av = *reinterpret_cast<const v4f*>(&strip[c * kEmLd + 16 * j + 4 * q]);
#pragma unroll
          for (int nt = 0; nt < MT; ++nt)
            if (nt < NT) {
              const v4f b = *reinterpret_cast<const v4f*>(&Wf[((4 * hh + j) * NT + nt) * kEmFrag]);
#pragma unroll
              for (int w = 0; w < 4; ++w) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[w], b[w], acc[nt], 0, 0, 0);
            }
        }
    }
}

// acc[kt] = d W for kt < KT, d [16, 16 NT] through the strip: the reduction runs over the columns of d, k-step (j, w) gives lane q the
// column 64 hh + 16 j + 4 q + w
template <int MT>
__device__ __forceinline__ void em_gemm_back(const float* Wl, float* strip, int KT, int NT, int c, int q, const v4f (&d)[MT], v4f (&acc)[MT]) {
#pragma unroll
  for (int kt = 0; kt < MT; ++kt) acc[kt] = (v4f)(0.f);
  const float* Wb = Wl + (c >> 2) * kEmQ + 16 * q + (c & 3);
#pragma unroll
  for (int hh = 0; hh < (MT + 3) / 4; ++hh)
    if (4 * hh < NT) {
      em_to_strip<MT>(strip, hh, NT, c, q, d);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (4 * hh + j < MT && 4 * hh + j < NT) {
          const v4f dv = *reinterpret_cast<const v4f*>(&strip[c * kEmLd + 16 * j + 4 * q]);
#pragma unroll
          for (int w = 0; w < 4; ++w)
#pragma unroll
            for (int kt = 0; kt < MT; ++kt)
              if (kt < KT) acc[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(dv[w], Wb[(kt * NT + 4 * hh + j) * kEmFrag + 4 * w], acc[kt], 0, 0, 0);
        }
    }
}

template <int MT>
__device__ __forceinline__ void em_bias_relu(const float (&b)[MT], v4f (&v)[MT]) {
#pragma unroll
  for (int nt = 0; nt < MT; ++nt)
#pragma unroll
    for (int r = 0; r < 4; ++r) v[nt][r] = fmaxf(v[nt][r] + b[nt], 0.f);
}

// MT = column tiles of 16 held in registers per stage (the widest of H0, H1 and the slab), L = layers
template <int MT, int L>
__global__ __launch_bounds__(kBlock) void edge_mlp_reduce_kernel(const EmArgs a) {
  constexpr int NH = (MT + 3) / 4;
  extern __shared__ __attribute__((aligned(16))) float em_lds[];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int c = lane & 15, q = lane >> 4;
  const int n0 = blockIdx.y * kEmSlab;
  const int NTs = (a.HL - n0 < kEmSlab ? a.HL - n0 : kEmSlab) >> 4;  // column tiles of this slab
  const int KT0 = a.H0 >> 4, NT1 = L == 2 ? a.H1 >> 4 : NTs;
  float* W1l = em_lds;
  float* W2l = W1l + KT0 * NT1 * kEmFrag;
  float* strip0 = W2l + (L == 2 ? NT1 * NTs * kEmFrag : 0) + wave * 16 * kEmLd;
  em_stage(a.w1, a.H0, L == 2 ? 0 : n0, NT1, W1l);
  if (L == 2) em_stage(a.w2, a.H1, n0, NTs, W2l);
  __syncthreads();
  float b1v[MT], b2v[MT];
  em_bias<MT>(a.b1, L == 2 ? 0 : n0, NT1, c, b1v);
  em_bias<MT>(L == 2 ? a.b2 : nullptr, n0, NTs, c, b2v);
  const float init = a.sum ? 0.f : -INFINITY;

  for (int it = blockIdx.x * kEmWaves + wave; it < a.nitems; it += gridDim.x * kEmWaves) {
    const int p0 = it * a.item, pend = p0 + a.item < a.nnz ? p0 + a.item : a.nnz;
    // the row walk's state (wave-uniform): the row of the next position and its ends
    int row = __builtin_amdgcn_readfirstlane(em_row_of(a.indptr, a.nrows, p0));
    int rb = a.indptr[row], re = a.indptr[row + 1];
    float rs[NH];
    int ra[NH];
#pragma unroll
    for (int h = 0; h < NH; ++h) { rs[h] = init; ra[h] = -1; }
    auto flush = [&](int h, int r_, int rb_, int re_, float s, int ar) {
      const int col = 64 * h + lane;
      if (col >= 16 * NTs) return;
      if (rb_ >= p0 && re_ <= pend) {
        a.out[(int64_t)r_ * a.ldo + n0 + col] = s;
        if (!a.sum) a.arg[(int64_t)r_ * a.HL + n0 + col] = ar;
      } else {
        const int64_t at = ((int64_t)it * 2 + (rb_ < p0 ? 0 : 1)) * kEmPartLd + n0 + col;
        a.part[at] = s;
        if (!a.sum) a.parg[at] = ar;
      }
    };

    int s1, d1;
    v4f xu[MT], xv[MT], av[MT];
    em_ids(a, p0, pend, c, s1, d1);
    em_load<MT>(a.u, a.ldu, s1, KT0, q, xu);
    em_load<MT>(a.v, a.ldv, d1, KT0, q, xv);
    em_ids(a, p0 + 16, pend, c, s1, d1);
    for (int tp = p0; tp < pend; tp += 16) {
#pragma unroll
      for (int g = 0; g < MT; ++g)
#pragma unroll
        for (int w = 0; w < 4; ++w) av[g][w] = fmaxf(xu[g][w] - xv[g][w], 0.f);
      em_load<MT>(a.u, a.ldu, s1, KT0, q, xu);  // tile + 1, in flight under the MFMAs below
      em_load<MT>(a.v, a.ldv, d1, KT0, q, xv);
      em_ids(a, tp + 32, pend, c, s1, d1);
      int lo = 0;  // the weights stay in LDS: an offset the compiler cannot prove loop-invariant keeps the fragments out of registers
      asm volatile("" : "+v"(lo));
      float* strip = strip0 + lo;
      v4f h1[MT], f[MT];
      em_gemm_regs<MT>(W1l + lo, KT0, NT1, c, q, av, h1);
      em_bias_relu<MT>(b1v, h1);
      if (L == 2) {
        em_gemm_strip<MT>(W2l + lo, strip, NT1, NTs, c, q, h1, f);
        em_bias_relu<MT>(b2v, f);
      }
      const v4f (&eL)[MT] = L == 2 ? f : h1;
      // ---- the row reduce: lane = column, the tile's positions in order
      const int n = pend - tp < 16 ? pend - tp : 16;
      int row1 = row, rb1 = rb, re1 = re;
#pragma unroll
      for (int h = 0; h < NH; ++h)
        if (4 * h < NTs) {
          em_to_strip<MT>(strip, h, NTs, c, q, eL);
          row1 = row; rb1 = rb; re1 = re;
          for (int j = 0; j < n; ++j) {
            while (tp + j >= re1) {  // the row is over; rows without positions are passed by
              if (re1 > rb1) { flush(h, row1, rb1, re1, rs[h], ra[h]); rs[h] = init; ra[h] = -1; }
              ++row1; rb1 = re1; re1 = a.indptr[row1 + 1];
            }
            const float x = strip[j * kEmLd + lane];
            if (a.sum) rs[h] += x;
            else if (x > rs[h]) { rs[h] = x; ra[h] = tp + j; }
          }
        }
      row = row1; rb = rb1; re = re1;
    }
#pragma unroll
    for (int h = 0; h < NH; ++h) flush(h, row, rb, re, rs[h], ra[h]);  // the row of the item's last position
  }
}

// One wave per item boundary j (position j * item): the row that straddles it, if this is the first boundary inside that row, is merged
// from its trailing partial in the item it starts in and the leading partials of the items after, in item order.
__global__ __launch_bounds__(kBlock) void edge_mlp_rows_finish_kernel(const int32_t* __restrict__ indptr, int nrows, int nitems, int item, int N,
                                                                      int sum, const float* __restrict__ part, const int32_t* __restrict__ parg,
                                                                      float* __restrict__ out, int64_t ldo, int32_t* __restrict__ arg) {
  const int j = blockIdx.x * kWavesPerBlock + threadIdx.x / kWave + 1;
  if (j >= nitems) return;
  const int p = j * item;
  const int r = em_row_of(indptr, nrows, p);
  const int rb = indptr[r], re = indptr[r + 1];
  const int t0 = rb / item;
  if (rb >= p || t0 + 1 != j) return;
  const int t1 = (re - 1) / item;
  for (int n = threadIdx.x & (kWave - 1); n < N; n += kWave) {
    int64_t at = ((int64_t)t0 * 2 + 1) * kEmPartLd + n;
    float s = part[at];
    int ar = sum ? 0 : parg[at];
    for (int t = t0 + 1; t <= t1; ++t) {
      at = (int64_t)t * 2 * kEmPartLd + n;
      const float x = part[at];
      if (sum) s += x;
      else if (x > s) { s = x; ar = parg[at]; }
    }
    out[(int64_t)r * ldo + n] = s;
    if (!sum) arg[(int64_t)r * N + n] = ar;
  }
}

template <int MT, int L>
__global__ __launch_bounds__(kBlock) void edge_mlp_grad_kernel(const EmArgs a) {
  constexpr bool kAhead = !(MT == 8 && L == 2);  // the widest form has no registers for the rows of tile + 1: it requests the ids only
  extern __shared__ __attribute__((aligned(16))) float em_lds[];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int c = lane & 15, q = lane >> 4;
  const int nslab = (a.HL + kEmSlab - 1) / kEmSlab;
  const int KT0 = a.H0 >> 4, NTmax = (a.HL < kEmSlab ? a.HL : kEmSlab) >> 4;
  float* W1l = em_lds;
  float* W2l = W1l + KT0 * (L == 2 ? a.H1 >> 4 : NTmax) * kEmFrag;
  float* strip0 = W2l + (L == 2 ? (a.H1 >> 4) * NTmax * kEmFrag : 0) + wave * 16 * kEmLd;

  for (int slab = 0; slab < nslab; ++slab) {
    const int n0 = slab * kEmSlab;
    const int NTs = (a.HL - n0 < kEmSlab ? a.HL - n0 : kEmSlab) >> 4;
    const int NT1 = L == 2 ? a.H1 >> 4 : NTs;
    const int KTl = L == 2 ? NT1 : KT0;  // 16-column groups of the last layer's input
    const bool last = slab + 1 == nslab;
    if (slab) __syncthreads();  // every wave is through with the fragments of the slab before
    if (L == 2) {
      if (slab == 0) em_stage(a.w1, a.H0, 0, NT1, W1l);
      em_stage(a.w2, a.H1, n0, NTs, W2l);
    } else {
      em_stage(a.w1, a.H0, n0, NTs, W1l);
    }
    __syncthreads();
    float b1v[MT], b2v[MT];
    em_bias<MT>(a.b1, L == 2 ? 0 : n0, NT1, c, b1v);
    em_bias<MT>(L == 2 ? a.b2 : nullptr, n0, NTs, c, b2v);

    for (int it = blockIdx.x * kEmWaves + wave; it < a.nitems; it += gridDim.x * kEmWaves) {
      const int p0 = it * a.item, pend = p0 + a.item < a.nnz ? p0 + a.item : a.nnz;
      int s1, d1;
      v4f xu[MT], xv[MT], av[MT];
      em_ids(a, p0, pend, c, s1, d1);
      if (kAhead) {
        em_load<MT>(a.u, a.ldu, s1, KT0, q, xu);
        em_load<MT>(a.v, a.ldv, d1, KT0, q, xv);
        em_ids(a, p0 + 16, pend, c, s1, d1);
      }
      for (int tp = p0; tp < pend; tp += 16) {
        if (!kAhead) {
          em_load<MT>(a.u, a.ldu, s1, KT0, q, xu);
          em_load<MT>(a.v, a.ldv, d1, KT0, q, xv);
          em_ids(a, tp + 16, pend, c, s1, d1);
        }
#pragma unroll
        for (int g = 0; g < MT; ++g)
#pragma unroll
          for (int w = 0; w < 4; ++w) av[g][w] = fmaxf(xu[g][w] - xv[g][w], 0.f);
        if (kAhead) {
          em_load<MT>(a.u, a.ldu, s1, KT0, q, xu);
          em_load<MT>(a.v, a.ldv, d1, KT0, q, xv);
          em_ids(a, tp + 32, pend, c, s1, d1);
        }
        int lo = 0;
        asm volatile("" : "+v"(lo));
        float* strip = strip0 + lo;
        // ---- the stages again, as the forward formed them
        v4f h1[MT], dl[MT], dprev[MT];
        em_gemm_regs<MT>(W1l + lo, KT0, NT1, c, q, av, h1);
        em_bias_relu<MT>(b1v, h1);
        if (L == 2) {
          em_gemm_strip<MT>(W2l + lo, strip, NT1, NTs, c, q, h1, dl);
          em_bias_relu<MT>(b2v, dl);
        }
        // ---- d pre_L of this slab: rows 4 q + r of the tile, columns n0 + 16 nt + c
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int p = tp + 4 * q + r;
          const int64_t rw = p < pend ? a.rowpos[p] : -1;
#pragma unroll
          for (int nt = 0; nt < MT; ++nt) {
            float d = 0.f;
            if (nt < NTs && rw >= 0) {
              const int col = n0 + 16 * nt + c;
              const float e = L == 2 ? dl[nt][r] : h1[nt][r];
              if (e > 0.f && (a.sum || a.argin[rw * a.HL + col] == p)) d = a.G[rw * a.ldg + col];
              a.dpl[(int64_t)p * a.HL + col] = d;
            }
            dl[nt][r] = d;
          }
        }
        em_gemm_back<MT>((L == 2 ? W2l : W1l) + lo, strip, KTl, NTs, c, q, dl, dprev);
        if (nslab > 1) {  // the sum over the slabs, in slab order
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int p = tp + 4 * q + r;
            if (p >= pend) continue;
#pragma unroll
            for (int kt = 0; kt < MT; ++kt)
              if (kt < KTl) {
                float* at = a.acc + (int64_t)p * (16 * KTl) + 16 * kt + c;
                if (slab) dprev[kt][r] += *at;
                if (!last) *at = dprev[kt][r];
              }
          }
        }
        if (!last) continue;
        if (L == 2) {  // d pre_1 = d e_1 where e_1 > 0; e_1 and d pre_1 by position for d W_2, d W_1 and d b_1
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int64_t p = tp + 4 * q + r;
#pragma unroll
            for (int kt = 0; kt < MT; ++kt) {
              const float d = h1[kt][r] > 0.f ? dprev[kt][r] : 0.f;
              dl[kt][r] = d;
              if (kt < NT1 && p < pend) {
                a.e1[p * a.H1 + 16 * kt + c] = h1[kt][r];
                a.dp1[p * a.H1 + 16 * kt + c] = d;
              }
            }
          }
          em_gemm_back<MT>(W1l + lo, strip, KT0, NT1, c, q, dl, dprev);
        }
        // ---- d e_0 = d . where e_0 > 0, through the strip into the A layout: row c, 16-byte stores; d e_0 by edge id, e_0 by position
        const int pc = tp + c;
        const int64_t eid = pc >= pend ? -1 : a.eids ? a.eids[pc] : pc;
#pragma unroll
        for (int hh = 0; hh < (MT + 3) / 4; ++hh)
          if (4 * hh < KT0) {
            em_to_strip<MT>(strip, hh, KT0, c, q, dprev);
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (4 * hh + j < MT && 4 * hh + j < KT0) {
                constexpr int kLast = MT - 1;
                const int g = 4 * hh + j < MT ? 4 * hh + j : kLast;
                v4f d = *reinterpret_cast<const v4f*>(&strip[c * kEmLd + 16 * j + 4 * q]);
#pragma unroll
                for (int w = 0; w < 4; ++w) d[w] = av[g][w] > 0.f ? d[w] : 0.f;
                if (eid >= 0) {
                  *reinterpret_cast<v4f*>(&a.de0[eid * a.H0 + 16 * g + 4 * q]) = d;
                  *reinterpret_cast<v4f*>(&a.e0[(int64_t)pc * a.H0 + 16 * g + 4 * q]) = av[g];
                }
              }
          }
      }
    }
  }
}

static bool em_shape_ok(int64_t L, int64_t H0, int64_t H1, int64_t HL) {
  auto w = [](int64_t h, int64_t top) { return h >= 16 && h <= top && h % 16 == 0; };
  return (L == 1 || L == 2) && w(H0, 128) && w(HL, 256) && (L == 1 || w(H1, 128));
}
static bool em_item_ok(int64_t item) { return item >= 16 && item <= kEmMaxItem && item % 16 == 0; }
static bool em_csr_ok(const mgx_csr* csr) {
  const int64_t lim = int64_t(1) << 30;
  return csr && csr->idx_bits == 32 && csr->nnz > 0 && csr->nnz < lim / 128 * 16 && csr->num_rows < lim && csr->num_cols < lim;
}
static size_t em_lds_bytes(const EmArgs& a, int L) {
  const int64_t KT0 = a.H0 / 16, NTs = (a.HL < kEmSlab ? a.HL : kEmSlab) / 16, NT1 = L == 2 ? a.H1 / 16 : NTs;
  return (size_t)((KT0 * NT1 + (L == 2 ? NT1 * NTs : 0)) * kEmFrag + kEmWaves * 16 * kEmLd) * sizeof(float);
}

// a persistent grid: as many workgroups as a CU's LDS holds (four at most) per CU, an item per wave at least
static int em_grid(int64_t nitems, size_t lds) {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) n = 256;
    cus = n;
  }
  int per = (int)(kEmLdsMax / lds);
  per = per < 1 ? 1 : per > 4 ? 4 : per;
  const int64_t want = (nitems + kEmWaves - 1) / kEmWaves;
  return (int)(want < (int64_t)cus * per ? want : (int64_t)cus * per);
}

template <typename Kn>
static int32_t em_launch(Kn kernel, const EmArgs& a, size_t lds, int slabs, hipStream_t s) {
  MGX_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kernel, dim3((unsigned)em_grid(a.nitems, lds), (unsigned)slabs), dim3(kBlock), lds, s, a);
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}

template <int MT>
static int32_t em_launch_mt(bool grad, int L, const EmArgs& a, size_t lds, int slabs, hipStream_t s) {
  if (L == 2) return grad ? em_launch(edge_mlp_grad_kernel<MT, 2>, a, lds, 1, s) : em_launch(edge_mlp_reduce_kernel<MT, 2>, a, lds, slabs, s);
  return grad ? em_launch(edge_mlp_grad_kernel<MT, 1>, a, lds, 1, s) : em_launch(edge_mlp_reduce_kernel<MT, 1>, a, lds, slabs, s);
}

static int32_t em_dispatch(bool grad, int L, const EmArgs& a, hipStream_t s) {
  const size_t lds = em_lds_bytes(a, L);
  const int slabs = (a.HL + kEmSlab - 1) / kEmSlab;
  int widest = a.HL < kEmSlab ? a.HL : kEmSlab;
  widest = a.H0 > widest ? a.H0 : widest;
  widest = L == 2 && a.H1 > widest ? a.H1 : widest;
  if (widest <= 32) return em_launch_mt<2>(grad, L, a, lds, slabs, s);
  if (widest <= 64) return em_launch_mt<4>(grad, L, a, lds, slabs, s);
  return em_launch_mt<8>(grad, L, a, lds, slabs, s);
}

static int32_t em_fill(EmArgs& a, const mgx_csr* csc, const int32_t* rowpos, int64_t L, int64_t H0, int64_t H1, int64_t HL, const float* u,
                       int64_t ldu, const float* v, int64_t ldv, const float* w1, const float* b1, const float* w2, const float* b2,
                       int64_t item_edges, const char* who) {
  MGX_CHECK_ARG(csc && csc->num_rows >= 0 && csc->num_cols >= 0 && csc->nnz >= 0, "%s: bad CSR", who);
  MGX_CHECK_ARG(csc->nnz == 0 || (csc->indptr && csc->indices), "%s: CSR without indptr / indices", who);
  if (!em_csr_ok(csc)) MGX_UNSUPPORTED("%s: needs 32-bit graph indices, at least one edge, fewer than 2^27 edges and 2^30 rows", who);
  if (!em_shape_ok(L, H0, H1, HL))
    MGX_UNSUPPORTED("%s: needs 1 or 2 layers, the input and hidden widths multiples of 16 in 16 .. 128 and the output width one in 16 .. 256 "
                    "(got %lld: %lld, %lld, %lld)", who, (long long)L, (long long)H0, (long long)H1, (long long)HL);
  MGX_CHECK_ARG(rowpos && u && v && w1 && (L == 1 || w2), "%s: NULL pointer", who);
  MGX_CHECK_ARG(em_item_ok(item_edges), "%s: item_edges must be a multiple of 16 in 16 .. %d, got %lld", who, kEmMaxItem, (long long)item_edges);
  MGX_CHECK_ARG(ldu >= H0 && ldv >= H0 && ldu % 4 == 0 && ldv % 4 == 0 && (uintptr_t)u % 16 == 0 && (uintptr_t)v % 16 == 0,
                "%s: u and v need rows of at least H0 floats, row strides that are multiples of 4 floats and 16-byte aligned bases", who);
  memset(&a, 0, sizeof(a));
  a.indptr = (const int32_t*)csc->indptr; a.indices = (const int32_t*)csc->indices; a.eids = (const int32_t*)csc->eids; a.rowpos = rowpos;
  a.nrows = (int)csc->num_rows; a.nnz = (int)csc->nnz; a.item = (int)item_edges; a.nitems = (int)((csc->nnz + item_edges - 1) / item_edges);
  a.H0 = (int)H0; a.H1 = (int)(L == 2 ? H1 : HL); a.HL = (int)HL;
  a.u = u; a.ldu = ldu; a.v = v; a.ldv = ldv; a.w1 = w1; a.b1 = b1; a.w2 = L == 2 ? w2 : nullptr; a.b2 = L == 2 ? b2 : nullptr;
  return MGX_OK;
}

}  // namespace mgx

extern "C" int32_t mgx_edge_mlp_supported(const mgx_csr* csc, int64_t layers, int64_t H0, int64_t H1, int64_t HL) {
  return (mgx::em_csr_ok(csc) && mgx::em_shape_ok(layers, H0, H1, HL)) ? 1 : 0;
}

extern "C" int64_t mgx_edge_mlp_workspace(int64_t nnz, int64_t item_edges) {
  using namespace mgx;
  if (nnz < 0 || !em_item_ok(item_edges)) return -1;
  return (nnz + item_edges - 1) / item_edges * 2 * kEmPartLd * (int64_t)(sizeof(float) + sizeof(int32_t));
}

extern "C" int32_t mgx_edge_mlp_reduce(const mgx_csr* csc, const int32_t* row_of_position, int64_t layers, int64_t H0, int64_t H1, int64_t HL,
                                       const float* u, int64_t ldu, const float* v, int64_t ldv, const float* w1, const float* b1,
                                       const float* w2, const float* b2, int32_t sum, float* out, int64_t ldo, int32_t* arg, int64_t item_edges,
                                       void* workspace, void* stream) {
  using namespace mgx;
  MGX_ENTER();
  EmArgs a;
  const int32_t st = em_fill(a, csc, row_of_position, layers, H0, H1, HL, u, ldu, v, ldv, w1, b1, w2, b2, item_edges, "mgx_edge_mlp_reduce");
  if (st != MGX_OK) return st;
  MGX_CHECK_ARG(out && workspace && ldo >= HL && (sum || arg), "mgx_edge_mlp_reduce: out, workspace or (for max) arg missing, or ldo < HL");
  a.out = out; a.ldo = ldo; a.arg = arg; a.sum = sum ? 1 : 0;
  a.part = (float*)workspace; a.parg = (int32_t*)workspace + (int64_t)a.nitems * 2 * kEmPartLd;
  hipStream_t s = (hipStream_t)stream;
  const int32_t r = em_dispatch(false, (int)layers, a, s);
  if (r != MGX_OK) return r;
  if (a.nitems > 1) {
    hipLaunchKernelGGL(edge_mlp_rows_finish_kernel, dim3((unsigned)((a.nitems - 1 + kWavesPerBlock - 1) / kWavesPerBlock)), dim3(kBlock), 0, s,
                       a.indptr, a.nrows, a.nitems, a.item, a.HL, a.sum, (const float*)a.part, (const int32_t*)a.parg, out, ldo, arg);
    MGX_CHECK_LAUNCH();
  }
  note_spmm_kernel("edge_mlp_reduce");
  return MGX_OK;
}

extern "C" int32_t mgx_edge_mlp_grad(const mgx_csr* csc, const int32_t* row_of_position, int64_t layers, int64_t H0, int64_t H1, int64_t HL,
                                     const float* u, int64_t ldu, const float* v, int64_t ldv, const float* w1, const float* b1, const float* w2,
                                     const float* b2, int32_t sum, const float* g, int64_t ldg, const int32_t* arg, float* e0, float* d_e0,
                                     float* e1, float* d_pre1, float* d_preL, float* acc, int64_t item_edges, void* stream) {
  using namespace mgx;
  MGX_ENTER();
  EmArgs a;
  const int32_t st = em_fill(a, csc, row_of_position, layers, H0, H1, HL, u, ldu, v, ldv, w1, b1, w2, b2, item_edges, "mgx_edge_mlp_grad");
  if (st != MGX_OK) return st;
  MGX_CHECK_ARG(g && e0 && d_e0 && d_preL && ldg >= HL && (sum || arg), "mgx_edge_mlp_grad: NULL pointer, or ldg < HL");
  MGX_CHECK_ARG(layers == 1 || (e1 && d_pre1), "mgx_edge_mlp_grad: two layers need e1 and d_pre1");
  MGX_CHECK_ARG(HL <= kEmSlab || acc, "mgx_edge_mlp_grad: an output wider than %d needs acc", kEmSlab);
  a.sum = sum ? 1 : 0; a.G = g; a.ldg = ldg; a.argin = arg; a.e0 = e0; a.de0 = d_e0; a.e1 = e1; a.dp1 = d_pre1; a.dpl = d_preL; a.acc = acc;
  const int32_t r = em_dispatch(true, (int)layers, a, (hipStream_t)stream);
  if (r != MGX_OK) return r;
  note_spmm_kernel("edge_mlp_grad");
  return MGX_OK;
}
