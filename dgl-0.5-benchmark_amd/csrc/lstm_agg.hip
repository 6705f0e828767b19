// lstm_agg.hip -- the "lstm" aggregator of dgl.nn.SAGEConv as one recurrent row walk each way (gfx950 / MI355X, wave64, fp32 MFMA 16x16x4).
//   mgx_lstm_agg_fwd   out[v] = the last h of an LSTM run over the in-edges of v in storage order, from h = c = 0
//   mgx_lstm_agg_bwd   dG[e] = the gradient of the pre-activation gates of edge e's step, given d out
// The input projection is NOT here: the caller hands in P[u] = W_ih x_u + b_ih + b_hh, one row per SOURCE NODE, so nothing is projected
// per edge.  P's columns are gate-interleaved, column 4 j + gate (gate = i, f, g, o): one 16-byte load brings the four gates of a hidden
// unit, and dG is written in the same layout.
//
// TILES.  Rows are taken 16 at a time from `order`, the destination rows by descending in-degree (a stable sort, built by the caller
// once per graph).  A wave owns a tile and runs max-degree steps; a row whose degree is at most t keeps its state -- in a sorted tile
// those rows are a suffix.  Waves take tiles round robin, so the longest tiles start first (a persistent grid, four waves a workgroup).
// A STEP.  The [16, 4H] accumulator starts as the gathered rows P[indices[indptr[r] + t]] and gets h W_hh^T added by H / 4 x 4H / 16
// MFMAs; accumulator tile 4 jt + gate, lane (c, q), element r is gate `gate` of hidden unit 16 jt + c of tile row 4 q + r, so the four
// gates of a unit meet in one lane and c stays in registers in that layout.  The new h goes through a per-wave LDS strip [16][H + 4] to
// come back as the A operand (lane (c, q) reads h[c][16 ks + 4 q .. + 3], one ds_read_b128 per four k-steps: the k index is relabelled,
// A and B alike).  The ids of step t + 2 and the P rows of step t + 1 are requested before the MFMAs of step t.
// W_hh IN LDS.  Staged once per workgroup as B fragments: fragment (ks, nt) holds, for lane (c, q), W_hh[gate H + 16 jt + c][16 ks + 4 q
// .. + 3] (nt = 4 jt + gate) at word q * 68 + 4 c: the forward reads it 16 bytes a lane, and the backward reads the SAME copy the other
// way for dh_prev = dG W_hh -- lane (c, q) takes word (c / 4) * 68 + 4 (4 q + w) + c % 4, and the pad of 4 words per q block puts the 64
// lanes on 64 banks.  69.6 KB at H = 64.
// BACKWARD.  The same tiles from the last position to the first, dh and dc in registers.  The gates are recomputed from P[u] and the
// saved state before the step (h_prev as the A operand straight from memory, c_prev in the accumulator layout), dG is stored by edge
// id and also laid into a per-wave strip [16][4H + 4] to be the A operand of dh_prev = dG W_hh.  The next step's rows are requested
// before that second product.  No atomics in either kernel: a rerun gives the same bits.
#include "common.h"

namespace mgx {

constexpr int kLaWaves = kBlock / kWave;
constexpr int kLaQ = 68;              // words of one q block of a W fragment: 64 + 4 of padding
constexpr int kLaFrag = 4 * kLaQ;     // words of a fragment

struct LaArgs {
  const int32_t *indptr, *indices, *eids, *order;
  int nrows, ntiles;
  const float *P, *W, *hprev_in, *cprev_in, *dout;
  int64_t ldp, ldd;
  float *out, *hprev, *cprev, *dG;
};

__device__ __forceinline__ float la_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// W_hh [4H, H] -> the fragments described above
template <int HT>
__device__ __forceinline__ void la_stage_w(float* Wl, const float* __restrict__ W) {
  constexpr int H = 16 * HT, NT = 4 * HT;
  for (int e = threadIdx.x; e < 4 * H * H; e += kBlock) {
    const int n = e / H, k = e % H;
    const int gate = n / H, j = n % H, nt = 4 * (j / 16) + gate;
    Wl[((k / 16) * NT + nt) * kLaFrag + ((k % 16) / 4) * kLaQ + (j % 16) * 4 + k % 4] = W[e];
  }
}

// the tile's rows in the accumulator layout (rows 4 q + r) and its length; rows past the end have degree 0 and row -1
__device__ __forceinline__ int la_tile_rows(const LaArgs& a, int tile, int q, int (&row)[4], int (&base)[4], int (&deg)[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = tile * 16 + 4 * q + r;
    row[r] = i < a.nrows ? a.order[i] : -1;
    base[r] = row[r] >= 0 ? a.indptr[row[r]] : 0;
    deg[r] = row[r] >= 0 ? a.indptr[row[r] + 1] - base[r] : 0;
  }
  const int first = a.order[tile * 16];  // the longest row of a sorted tile
  return __builtin_amdgcn_readfirstlane(a.indptr[first + 1] - a.indptr[first]);
}

template <int HT, bool SAVE>
__global__ __launch_bounds__(kBlock) void lstm_agg_fwd_kernel(const LaArgs a) {
  constexpr int H = 16 * HT, NT = 4 * HT, LDH = H + 4;
  extern __shared__ __attribute__((aligned(16))) float la_lds[];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int c = lane & 15, q = lane >> 4;
  float* Wl = la_lds;
  float* hs = la_lds + HT * NT * kLaFrag + wave * 16 * LDH;
  la_stage_w<HT>(Wl, a.W);
  __syncthreads();

  for (int tile = blockIdx.x * kLaWaves + wave; tile < a.ntiles; tile += gridDim.x * kLaWaves) {
    int row[4], base[4], deg[4];
    const int L = la_tile_rows(a, tile, q, row, base, deg);
    float cs[HT][4], hv[HT][4];
#pragma unroll
    for (int jt = 0; jt < HT; ++jt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        cs[jt][r] = hv[jt][r] = 0.f;
        hs[(4 * q + r) * LDH + 16 * jt + c] = 0.f;
      }
    // ids of a step (source node, edge id) and its P rows; a row that is over reads nothing
    auto load_ids = [&](int t, int (&u)[4], int (&e)[4]) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool on = t < deg[r];
        u[r] = on ? a.indices[base[r] + t] : -1;
        e[r] = !SAVE || !on ? -1 : a.eids ? a.eids[base[r] + t] : base[r] + t;
      }
    };
    auto load_rows = [&](const int (&u)[4], v4f (&p)[HT][4]) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int jt = 0; jt < HT; ++jt)
          p[jt][r] = u[r] >= 0 ? *reinterpret_cast<const v4f*>(a.P + (int64_t)u[r] * a.ldp + 64 * jt + 4 * c) : (v4f)(0.f);
    };
    int u1[4], e1[4], u2[4], e2[4], e0[4];
    v4f pn[HT][4];
    load_ids(0, u1, e1);
    load_rows(u1, pn);
#pragma unroll
    for (int r = 0; r < 4; ++r) e0[r] = e1[r];
    load_ids(1, u1, e1);

    for (int t = 0; t < L; ++t) {
      v4f acc[NT];
#pragma unroll
      for (int jt = 0; jt < HT; ++jt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          acc[4 * jt + g][0] = pn[jt][0][g]; acc[4 * jt + g][1] = pn[jt][1][g];
          acc[4 * jt + g][2] = pn[jt][2][g]; acc[4 * jt + g][3] = pn[jt][3][g];
        }
      load_rows(u1, pn);        // step t + 1, in flight under the MFMAs below
      load_ids(t + 2, u2, e2);
      if (SAVE) {               // the state BEFORE position t, by edge id
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (e0[r] >= 0) {
#pragma unroll
            for (int jt = 0; jt < HT; ++jt) {
              a.hprev[(int64_t)e0[r] * H + 16 * jt + c] = hv[jt][r];
              a.cprev[(int64_t)e0[r] * H + 16 * jt + c] = cs[jt][r];
            }
          }
      }
      int lo = 0;  // W stays in LDS: an offset the compiler cannot prove loop-invariant keeps the fragments out of registers
      asm volatile("" : "+v"(lo));
      const float* Wf = Wl + lo + q * kLaQ + 4 * c;
#pragma unroll
      for (int ks = 0; ks < HT; ++ks) {
        const v4f av = *reinterpret_cast<const v4f*>(&hs[c * LDH + 16 * ks + 4 * q + lo]);
#pragma unroll
        for (int g4 = 0; g4 < HT; ++g4) {
          v4f b[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) b[i] = *reinterpret_cast<const v4f*>(&Wf[(ks * NT + 4 * g4 + i) * kLaFrag]);
#pragma unroll
          for (int w = 0; w < 4; ++w)
#pragma unroll
            for (int i = 0; i < 4; ++i)
              acc[4 * g4 + i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[w], b[i][w], acc[4 * g4 + i], 0, 0, 0);
        }
      }
      __builtin_amdgcn_wave_barrier();  // every lane has read the strip before it is written again
#pragma unroll
      for (int jt = 0; jt < HT; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float ig = la_sigmoid(acc[4 * jt][r]), fg = la_sigmoid(acc[4 * jt + 1][r]);
          const float gg = tanhf(acc[4 * jt + 2][r]), og = la_sigmoid(acc[4 * jt + 3][r]);
          const float cn = fg * cs[jt][r] + ig * gg;
          const float hn = og * tanhf(cn);
          if (t < deg[r]) { cs[jt][r] = cn; hv[jt][r] = hn; }
          hs[(4 * q + r) * LDH + 16 * jt + c] = hv[jt][r];
        }
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int r = 0; r < 4; ++r) { e0[r] = e1[r]; u1[r] = u2[r]; e1[r] = e2[r]; }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (row[r] >= 0) {
#pragma unroll
        for (int jt = 0; jt < HT; ++jt) a.out[(int64_t)row[r] * H + 16 * jt + c] = hv[jt][r];
      }
  }
}

template <int HT>
__global__ __launch_bounds__(kBlock) void lstm_agg_bwd_kernel(const LaArgs a) {
  constexpr int H = 16 * HT, NT = 4 * HT, LDD = 4 * H + 4;
  extern __shared__ __attribute__((aligned(16))) float la_lds[];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int c = lane & 15, q = lane >> 4;
  float* Wl = la_lds;
  float* ds = la_lds + HT * NT * kLaFrag + wave * 16 * LDD;
  la_stage_w<HT>(Wl, a.W);
  __syncthreads();

  for (int tile = blockIdx.x * kLaWaves + wave; tile < a.ntiles; tile += gridDim.x * kLaWaves) {
    int row[4], base[4], deg[4];
    const int L = la_tile_rows(a, tile, q, row, base, deg);
    // the A operand's row of this lane: tile row c
    const int ia = tile * 16 + c;
    const int rowA = ia < a.nrows ? a.order[ia] : -1;
    const int baseA = rowA >= 0 ? a.indptr[rowA] : 0;
    const int degA = rowA >= 0 ? a.indptr[rowA + 1] - baseA : 0;
    float dh[HT][4], dc[HT][4];
#pragma unroll
    for (int jt = 0; jt < HT; ++jt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        dh[jt][r] = row[r] >= 0 ? a.dout[(int64_t)row[r] * a.ldd + 16 * jt + c] : 0.f;
        dc[jt][r] = 0.f;
      }
    auto load_ids = [&](int t, int (&u)[4], int (&e)[4], int& ea) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool on = t >= 0 && t < deg[r];
        u[r] = on ? a.indices[base[r] + t] : -1;
        e[r] = !on ? -1 : a.eids ? a.eids[base[r] + t] : base[r] + t;
      }
      ea = !(t >= 0 && t < degA) ? -1 : a.eids ? a.eids[baseA + t] : baseA + t;
    };
    auto load_rows = [&](const int (&u)[4], const int (&e)[4], int ea, v4f (&p)[HT][4], v4f (&ha)[HT], float (&cp)[HT][4]) {
#pragma unroll
      for (int jt = 0; jt < HT; ++jt) {
        ha[jt] = ea >= 0 ? *reinterpret_cast<const v4f*>(a.hprev_in + (int64_t)ea * H + 16 * jt + 4 * q) : (v4f)(0.f);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          p[jt][r] = u[r] >= 0 ? *reinterpret_cast<const v4f*>(a.P + (int64_t)u[r] * a.ldp + 64 * jt + 4 * c) : (v4f)(0.f);
          cp[jt][r] = e[r] >= 0 ? a.cprev_in[(int64_t)e[r] * H + 16 * jt + c] : 0.f;
        }
      }
    };
    int u0[4], e0[4], ea0, u1[4], e1[4], ea1;
    v4f pn[HT][4], ha[HT];
    float cp[HT][4];
    load_ids(L - 1, u0, e0, ea0);
    load_rows(u0, e0, ea0, pn, ha, cp);
    load_ids(L - 2, u1, e1, ea1);

    for (int t = L - 1; t >= 0; --t) {
      v4f acc[NT];
#pragma unroll
      for (int jt = 0; jt < HT; ++jt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          acc[4 * jt + g][0] = pn[jt][0][g]; acc[4 * jt + g][1] = pn[jt][1][g];
          acc[4 * jt + g][2] = pn[jt][2][g]; acc[4 * jt + g][3] = pn[jt][3][g];
        }
      int lo = 0;
      asm volatile("" : "+v"(lo));
      const float* Wf = Wl + lo + q * kLaQ + 4 * c;
#pragma unroll
      for (int ks = 0; ks < HT; ++ks)
#pragma unroll
        for (int g4 = 0; g4 < HT; ++g4) {
          v4f b[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) b[i] = *reinterpret_cast<const v4f*>(&Wf[(ks * NT + 4 * g4 + i) * kLaFrag]);
#pragma unroll
          for (int w = 0; w < 4; ++w)
#pragma unroll
            for (int i = 0; i < 4; ++i)
              acc[4 * g4 + i] = __builtin_amdgcn_mfma_f32_16x16x4f32(ha[ks][w], b[i][w], acc[4 * g4 + i], 0, 0, 0);
        }
      __builtin_amdgcn_wave_barrier();  // the strip's readers of the step before are done
#pragma unroll
      for (int jt = 0; jt < HT; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool on = e0[r] >= 0;
          const float ig = la_sigmoid(acc[4 * jt][r]), fg = la_sigmoid(acc[4 * jt + 1][r]);
          const float gg = tanhf(acc[4 * jt + 2][r]), og = la_sigmoid(acc[4 * jt + 3][r]);
          const float tc = tanhf(fg * cp[jt][r] + ig * gg);
          const float dct = dc[jt][r] + dh[jt][r] * og * (1.f - tc * tc);
          v4f d;
          d[0] = on ? dct * gg * ig * (1.f - ig) : 0.f;
          d[1] = on ? dct * cp[jt][r] * fg * (1.f - fg) : 0.f;
          d[2] = on ? dct * ig * (1.f - gg * gg) : 0.f;
          d[3] = on ? dh[jt][r] * tc * og * (1.f - og) : 0.f;
          if (on) {
            *reinterpret_cast<v4f*>(a.dG + (int64_t)e0[r] * (4 * H) + 64 * jt + 4 * c) = d;
            dc[jt][r] = dct * fg;
          }
#pragma unroll
          for (int g = 0; g < 4; ++g) ds[(4 * q + r) * LDD + (4 * jt + g) * 16 + c] = d[g];
        }
      __builtin_amdgcn_wave_barrier();
      bool on[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) { on[r] = e0[r] >= 0; u0[r] = u1[r]; e0[r] = e1[r]; }
      ea0 = ea1;
      load_rows(u0, e0, ea0, pn, ha, cp);  // step t - 1, in flight under the second product
      load_ids(t - 2, u1, e1, ea1);
      // dh_prev = dG W_hh: k runs over the gate columns, k-step (nt, w) gives lane q the column 16 nt + 4 q + w
      v4f acc2[HT];
#pragma unroll
      for (int jt = 0; jt < HT; ++jt) acc2[jt] = (v4f)(0.f);
      const float* Wb = Wl + lo + (c / 4) * kLaQ + 16 * q + c % 4;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const v4f av = *reinterpret_cast<const v4f*>(&ds[c * LDD + 16 * nt + 4 * q + lo]);
#pragma unroll
        for (int w = 0; w < 4; ++w)
#pragma unroll
          for (int jt = 0; jt < HT; ++jt)
            acc2[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[w], Wb[(jt * NT + nt) * kLaFrag + 4 * w], acc2[jt], 0, 0, 0);
      }
#pragma unroll
      for (int jt = 0; jt < HT; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (on[r]) dh[jt][r] = acc2[jt][r];
    }
  }
}

static bool la_shape_ok(int64_t H) { return H >= 16 && H <= 64 && H % 16 == 0; }
static size_t la_lds_bytes(int64_t H, bool bwd) {
  return (size_t)((H / 16) * (H / 4) * kLaFrag + kLaWaves * 16 * ((bwd ? 4 * H : H) + 4)) * sizeof(float);
}

// a persistent grid: a workgroup per CU at most (W_hh and the strips leave room for one), four tiles a workgroup at least
static int la_grid(int ntiles) {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) n = 256;
    cus = n;
  }
  const int want = (ntiles + kLaWaves - 1) / kLaWaves;
  return want < cus ? want : cus;
}

template <typename K>
static int32_t la_launch(K kernel, const LaArgs& a, size_t lds, hipStream_t s) {
  MGX_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kernel, dim3((unsigned)la_grid(a.ntiles)), dim3(kBlock), lds, s, a);
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}

static int32_t la_fill(LaArgs& a, const mgx_csr* csc, const int32_t* order, int64_t H, const float* P, int64_t ldp, const float* w_hh, const char* who) {
  MGX_CHECK_ARG(csc && csc->num_rows >= 0 && csc->num_cols >= 0 && csc->nnz >= 0, "%s: bad CSR", who);
  if (csc->idx_bits != 32) MGX_UNSUPPORTED("%s: needs 32-bit graph indices", who);
  if (!la_shape_ok(H)) MGX_UNSUPPORTED("%s: needs H a multiple of 16 in 16 .. 64, got %lld", who, (long long)H);
  if (csc->nnz >= (int64_t(1) << 30) || csc->num_rows >= (int64_t(1) << 30)) MGX_UNSUPPORTED("%s: needs fewer than 2^30 edges and rows", who);
  MGX_CHECK_ARG(csc->num_rows == 0 || (csc->indptr && order), "%s: rows without indptr / order", who);
  MGX_CHECK_ARG(csc->nnz == 0 || csc->indices, "%s: edges without indices", who);
  MGX_CHECK_ARG(P && w_hh, "%s: NULL pointer", who);
  MGX_CHECK_ARG(ldp >= 4 * H && ldp % 4 == 0 && ((uintptr_t)P & 15) == 0, "%s: P needs 16-byte aligned rows of at least 4H floats", who);
  memset(&a, 0, sizeof(a));
  a.indptr = (const int32_t*)csc->indptr; a.indices = (const int32_t*)csc->indices; a.eids = (const int32_t*)csc->eids; a.order = order;
  a.nrows = (int)csc->num_rows; a.ntiles = (int)((csc->num_rows + 15) / 16);
  a.P = P; a.ldp = ldp; a.W = w_hh;
  return MGX_OK;
}

}  // namespace mgx

extern "C" int32_t mgx_lstm_agg_supported(const mgx_csr* csc, int64_t H) {
  using namespace mgx;
  return (csc && csc->idx_bits == 32 && la_shape_ok(H) && csc->nnz < (int64_t(1) << 30) && csc->num_rows < (int64_t(1) << 30)
          && csc->num_cols < (int64_t(1) << 30)) ? 1 : 0;
}

extern "C" int32_t mgx_lstm_agg_fwd(const mgx_csr* csc, const int32_t* order, int64_t H, const float* P, int64_t ldp, const float* w_hh,
                                    float* out, float* h_prev, float* c_prev, void* stream) {
  using namespace mgx;
  MGX_ENTER();
  LaArgs a;
  const int32_t st = la_fill(a, csc, order, H, P, ldp, w_hh, "mgx_lstm_agg_fwd");
  if (st != MGX_OK) return st;
  MGX_CHECK_ARG(out && (h_prev == nullptr) == (c_prev == nullptr), "mgx_lstm_agg_fwd: out missing, or only one of h_prev / c_prev");
  if (a.ntiles == 0) return MGX_OK;
  a.out = out; a.hprev = h_prev; a.cprev = c_prev;
  hipStream_t s = (hipStream_t)stream;
  const size_t lds = la_lds_bytes(H, false);
  int32_t r;
  if (h_prev) {
    r = H == 16 ? la_launch(lstm_agg_fwd_kernel<1, true>, a, lds, s) : H == 32 ? la_launch(lstm_agg_fwd_kernel<2, true>, a, lds, s)
      : H == 48 ? la_launch(lstm_agg_fwd_kernel<3, true>, a, lds, s) : la_launch(lstm_agg_fwd_kernel<4, true>, a, lds, s);
  } else {
    r = H == 16 ? la_launch(lstm_agg_fwd_kernel<1, false>, a, lds, s) : H == 32 ? la_launch(lstm_agg_fwd_kernel<2, false>, a, lds, s)
      : H == 48 ? la_launch(lstm_agg_fwd_kernel<3, false>, a, lds, s) : la_launch(lstm_agg_fwd_kernel<4, false>, a, lds, s);
  }
  if (r != MGX_OK) return r;
  note_spmm_kernel("lstm_agg_fwd");
  return MGX_OK;
}

extern "C" int32_t mgx_lstm_agg_bwd(const mgx_csr* csc, const int32_t* order, int64_t H, const float* P, int64_t ldp, const float* w_hh,
                                    const float* h_prev, const float* c_prev, const float* d_out, int64_t ldd, float* dG, void* stream) {
  using namespace mgx;
  MGX_ENTER();
  LaArgs a;
  const int32_t st = la_fill(a, csc, order, H, P, ldp, w_hh, "mgx_lstm_agg_bwd");
  if (st != MGX_OK) return st;
  if (a.ntiles == 0 || csc->nnz == 0) return MGX_OK;
  MGX_CHECK_ARG(h_prev && c_prev && d_out && dG, "mgx_lstm_agg_bwd: NULL pointer");
  MGX_CHECK_ARG(ldd >= H && ((uintptr_t)h_prev & 15) == 0 && ((uintptr_t)dG & 15) == 0, "mgx_lstm_agg_bwd: h_prev and dG must be 16-byte aligned, ldd >= H");
  a.hprev_in = h_prev; a.cprev_in = c_prev; a.dout = d_out; a.ldd = ldd; a.dG = dG;
  hipStream_t s = (hipStream_t)stream;
  const size_t lds = la_lds_bytes(H, true);
  const int32_t r = H == 16 ? la_launch(lstm_agg_bwd_kernel<1>, a, lds, s) : H == 32 ? la_launch(lstm_agg_bwd_kernel<2>, a, lds, s)
                  : H == 48 ? la_launch(lstm_agg_bwd_kernel<3>, a, lds, s) : la_launch(lstm_agg_bwd_kernel<4>, a, lds, s);
  if (r != MGX_OK) return r;
  note_spmm_kernel("lstm_agg_bwd");
  return MGX_OK;
}
