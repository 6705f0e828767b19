// nnconv.hip -- edge-conditioned convolution (dgl.nn.NNConv, the MPNN layer) without an [E, I*O] tensor (gfx950 / MI355X, wave64, fp32 MFMA 16x16x4).
//   mgx_edge_bilinear         out[row(p), n] (+)= sum_a sum_b P[ia(p), a] * Q[ib(p), b] * W[a, b, n]   over the positions p of a CSR
//   mgx_edge_bilinear_grad_w  dW[k, i, o] = sum_e h[e, k] * x[src(e), i] * g[dst(e), o],  k = DH: the bias block (h = 1)
// Per edge the layer is (h_e (x) x_u) Theta: a GEMM with E rows and inner dimension DH * I whose A operand is an outer product of two
// gathered rows.  It is formed in registers, never in memory.  One kernel serves the forward (P = h by edge id, Q = x[src], rows summed
// per destination), d x (the out-CSR, Q = d out[dst], W read with i and o exchanged) and d h (P = x[src], Q = d out[dst], one output row
// per edge id); they differ in the index modes, the three strides of W, the implicit last a (P = 1: the bias) and the epilogue.
//
// WORK ITEM.  `item` consecutive CSR positions (a multiple of 16, at most 256), one workgroup of 8 waves; wave w takes the 16-position
// tiles w and w + 8.  Lane (c, q) of a tile keeps Q[ib, 4 j + q], j < 4 KCQ, in registers for the whole item and forms P[ia, a] * Q[..]
// once per a and chunk of 16 b; those products feed every column tile (B / 4 multiplies against B / 4 * MT MFMAs).  P is read one dword
// per lane and a, an a ahead of its use -- any alignment of P is taken.
// W THROUGH LDS.  W is streamed in stages of one a and CPS chunks of 16 b (all of B, or half of it at 128 x 128): 32 KB at most, two
// buffers, staged in the order the lanes read it ([chunk][column tile][lane][4 b]: one ds_read_b128 per chunk and column tile, segmm.hip's
// labelling, four consecutive columns of a group of 64 in one lane).  The next stage's global loads are issued before the current
// stage's MFMAs and written to the other buffer after them; one barrier per stage.  The stager walks W along the stride that is 1.
// EPILOGUES.  Store: row p goes to output row eid(p).  Row sum: the item's tile goes to LDS, 64 columns at a time (over the W buffers);
// the rows of the item are found by binary search of indptr, wave w sums rows r0 + w, r0 + w + 8, .. in position order; a row wholly
// inside the item is stored (divided by its length for mean), the leading / trailing row that continues in a neighbour item is stored
// as part[item][0 | 1][.].  edge_bilinear_rows_finish_kernel, one wave per item boundary, adds the partials of a straddling row in item
// order.  No atomics; a row without positions is not written (the caller passes zeros).
//
// WEIGHT GRADIENT.  MFMA rows are i, columns o, the reduction runs over edges (xty.hip's orientation).  A workgroup takes (edge chunk,
// group of 8 units); a unit is (k, 64 x 64 block of [I, O]), one per wave, k = DH (the bias) last.  The chunk's gathered x[src] and
// g[dst] rows are staged in LDS 32 edges at a time and shared by the 8 waves; each wave keeps its block's sum in accumulators over the
// whole chunk and forms h[e, k] * x[u, i] on the fly.  Each (chunk, unit) writes a partial; the finish kernel adds them in chunk order,
// 16 slices of the chunk list per element, the slices in slice order.  The chunk count depends on E alone.
#include "common.h"

namespace mgx {

constexpr int kEbBlock = 512;
constexpr int kEbWaves = kEbBlock / kWave;
constexpr int kEbTiles = 2;        // tiles of 16 positions per wave: items of at most 16 * 8 * 2 = 256 positions
constexpr int kEbMaxItem = 16 * kEbWaves * kEbTiles;
constexpr int kEbBuf = 8192;       // floats of one W stage; two of them = the [256, 64] tile of the row-sum epilogue
constexpr int kEbPartLd = 128;     // part[item][2][128]
constexpr int kGwEdges = 32;       // edges per LDS stage of the weight gradient
constexpr int kGwLd = 144;         // row stride of the staged x / g rows: 144 % 64 == 16, the four edge rows of a step on different banks
constexpr int kGwMaxChunks = 32;
constexpr int kGwMinChunk = 256;

// the row of position p: the largest r < nrows with indptr[r] <= p (0 <= p < nnz)
__device__ __forceinline__ int eb_row_of(const int32_t* __restrict__ indptr, int nrows, int p) {
  int lo = 0, hi = nrows;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (indptr[mid] <= p) lo = mid; else hi = mid;
  }
  return lo;
}

struct EbArgs {
  const int32_t *indptr, *indices, *eids;
  int nrows, nnz, item;
  int A, B, N, KC, has_one;  // KC = chunks of 16 b
  const float *P, *Q, *W, *W1;
  int64_t ldp, ldq, sa, sb, sn, sb1, sn1, ldo;
  int p_mode, q_mode, mean;
  float *out, *part;
};

__device__ __forceinline__ int eb_index(const EbArgs& a, int mode, int p) {
  if (mode == MGX_EB_BY_EDGE) return a.eids ? a.eids[p] : p;
  if (mode == MGX_EB_BY_COL) return a.indices[p];
  return eb_row_of(a.indptr, a.nrows, p);
}

// MT = column tiles of 16 (4 or 8), KCQ = chunks of 16 b held in registers (4 or 8)
template <int MT, int KCQ, bool ROWSUM>
__global__ __launch_bounds__(kEbBlock) void edge_bilinear_kernel(const EbArgs a) {
  constexpr int CPS = KCQ < 32 / MT ? KCQ : 32 / MT;  // chunks per stage
  constexpr int NH = KCQ / CPS;                       // stages per a
  constexpr int SE = CPS * 16 * MT * 16 / kEbBlock;   // staged floats per thread
  __shared__ __attribute__((aligned(16))) float lds[2 * kEbBuf];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int c = lane % 16, q = lane / 16;
  const int p0 = blockIdx.x * a.item;
  const int pend = p0 + a.item < a.nnz ? p0 + a.item : a.nnz;
  const int cnt = pend - p0;
  const int AT = a.A + a.has_one;
  const bool nfast = a.sn == 1;

  // ---- this lane's edge of each tile: its P row and its Q row slice
  bool live[kEbTiles];
  const float* prow[kEbTiles];
  float qv[kEbTiles][4 * KCQ];
#pragma unroll
  for (int j = 0; j < kEbTiles; ++j) {
    const int t16 = 16 * (wave + kEbWaves * j);
    live[j] = t16 < cnt;  // wave-uniform
    const int p = p0 + t16 + c;
    const bool ok = p < pend;
    prow[j] = ok ? a.P + (int64_t)eb_index(a, a.p_mode, p) * a.ldp : nullptr;
    const float* qrow = ok ? a.Q + (int64_t)eb_index(a, a.q_mode, p) * a.ldq : nullptr;
#pragma unroll
    for (int s = 0; s < 4 * KCQ; ++s) qv[j][s] = (ok && 4 * s + q < a.B) ? qrow[4 * s + q] : 0.f;
  }
  auto load_p = [&](float (&v)[kEbTiles], int a_) {
#pragma unroll
    for (int j = 0; j < kEbTiles; ++j) v[j] = !prow[j] ? 0.f : a_ < a.A ? prow[j][a_] : 1.f;
  };
  // ---- the stager: element e of stage (a_, h_) is W[a_][b][n], (b, n) walked along the stride that is 1
  auto split = [&](int e, int& bl, int& n) {
    if (nfast) { n = e % (MT * 16); bl = e / (MT * 16); } else { bl = e % (CPS * 16); n = e / (CPS * 16); }
  };
  auto fetch = [&](float (&v)[SE], int a_, int h_) {
    const bool one = a_ >= a.A;
    const float* __restrict__ base = one ? a.W1 : a.W + a_ * a.sa;
    const int64_t sb = one ? a.sb1 : a.sb, sn = one ? a.sn1 : a.sn;
#pragma unroll
    for (int i = 0; i < SE; ++i) {
      int bl, n;
      split(tid + kEbBlock * i, bl, n);
      const int b = h_ * CPS * 16 + bl;
      v[i] = (b < a.B && n < a.N) ? base[b * sb + n * sn] : 0.f;
    }
  };
  // element (chunk jj, tile mt, lane (c, q), component t) = W[b = 16 jj + 4 t + q][n = 64 (mt / 4) + 4 c + mt % 4]
  auto put = [&](float* buf, const float (&v)[SE]) {
#pragma unroll
    for (int i = 0; i < SE; ++i) {
      int bl, n;
      split(tid + kEbBlock * i, bl, n);
      const int jj = bl >> 4, w = bl & 15, mt = 4 * (n >> 6) + (n & 3);
      buf[((jj * MT + mt) * 64 + 16 * (w & 3) + ((n & 63) >> 2)) * 4 + (w >> 2)] = v[i];
    }
  };

  v4f acc[kEbTiles][MT];
#pragma unroll
  for (int j = 0; j < kEbTiles; ++j)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[j][mt] = (v4f)(0.f);
  float st[SE], pv[kEbTiles], pn[kEbTiles];
  fetch(st, 0, 0);
  put(lds, st);
  load_p(pv, 0);
  __syncthreads();
  int cur = 0;
  for (int a_ = 0; a_ < AT; ++a_) {
    load_p(pn, a_ + 1 < AT ? a_ + 1 : a_);
#pragma unroll
    for (int hh = 0; hh < NH; ++hh) {
      const int na = hh + 1 < NH ? a_ : a_ + 1, nh = hh + 1 < NH ? hh + 1 : 0;
      const bool more = na < AT;
      if (more) fetch(st, na, nh);  // in flight under the MFMAs below
      const float* Wl = lds + cur * kEbBuf;
      int lo = lane;  // W stays in LDS: an address the compiler cannot prove loop-invariant keeps the fragments out of registers
      asm volatile("" : "+v"(lo));
#pragma unroll
      for (int jj = 0; jj < CPS; ++jj) {
        const int jc = hh * CPS + jj;
        if (jc < a.KC) {  // wave-uniform
          float pr[kEbTiles][4];
#pragma unroll
          for (int j = 0; j < kEbTiles; ++j)
#pragma unroll
            for (int t = 0; t < 4; ++t) pr[j][t] = pv[j] * qv[j][4 * jc + t];
#pragma unroll
          for (int g = 0; g < MT / 4; ++g) {
            v4f b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) b[i] = *reinterpret_cast<const v4f*>(&Wl[((jj * MT + 4 * g + i) * 64 + lo) * 4]);
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                acc[0][4 * g + i] = __builtin_amdgcn_mfma_f32_16x16x4f32(pr[0][t], b[i][t], acc[0][4 * g + i], 0, 0, 0);
                if (live[1]) acc[1][4 * g + i] = __builtin_amdgcn_mfma_f32_16x16x4f32(pr[1][t], b[i][t], acc[1][4 * g + i], 0, 0, 0);
              }
          }
        }
      }
      if (more) put(lds + (cur ^ 1) * kEbBuf, st);
      __syncthreads();  // the other buffer is whole, and nobody reads this one any more
      cur ^= 1;
    }
#pragma unroll
    for (int j = 0; j < kEbTiles; ++j) pv[j] = pn[j];
  }

  // accumulator element r of tile 4 g + i = result[position 4 q + r of the tile][64 g + 4 c + i]
  if (!ROWSUM) {
#pragma unroll
    for (int j = 0; j < kEbTiles; ++j) {
      if (!live[j]) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int p = p0 + 16 * (wave + kEbWaves * j) + 4 * q + r;
        if (p >= pend) continue;
        float* dst = a.out + (int64_t)(a.eids ? a.eids[p] : p) * a.ldo;
#pragma unroll
        for (int g = 0; g < MT / 4; ++g)
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (64 * g + 4 * c + i < a.N) dst[64 * g + 4 * c + i] = acc[j][4 * g + i][r];
      }
    }
    return;
  }
  const int r0 = eb_row_of(a.indptr, a.nrows, p0), r1 = eb_row_of(a.indptr, a.nrows, pend - 1);
  const int col = tid & 63;
#pragma unroll
  for (int g = 0; g < MT / 4; ++g) {
    if (64 * g >= a.N) break;
    if (g > 0) __syncthreads();  // the walk over the group before is done
#pragma unroll
    for (int j = 0; j < kEbTiles; ++j)
      if (live[j])
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          v4f o; o.x = acc[j][4 * g + 0][r]; o.y = acc[j][4 * g + 1][r]; o.z = acc[j][4 * g + 2][r]; o.w = acc[j][4 * g + 3][r];
          *reinterpret_cast<v4f*>(&lds[(16 * (wave + kEbWaves * j) + 4 * q + r) * 64 + 4 * c]) = o;
        }
    __syncthreads();
    const int n = 64 * g + col;
    for (int r = r0 + wave; r <= r1; r += kEbWaves) {
      const int rb = a.indptr[r], re = a.indptr[r + 1];
      const int lo = rb > p0 ? rb : p0, hi = re < pend ? re : pend;
      if (lo >= hi || n >= a.N) continue;
      float s = 0.f;
      for (int p = lo; p < hi; ++p) s += lds[(p - p0) * 64 + col];
      if (rb >= p0 && re <= pend)
        a.out[(int64_t)r * a.ldo + n] = a.mean ? s / (float)(re - rb) : s;
      else
        a.part[((int64_t)blockIdx.x * 2 + (rb < p0 ? 0 : 1)) * kEbPartLd + n] = s;
    }
  }
}

// One wave per item boundary j (position j * item): the row that straddles it, if this is the first boundary inside that row, is the sum
// of its trailing partial in the item it starts in and the leading partials of the items after, in item order.
__global__ __launch_bounds__(kBlock) void edge_bilinear_rows_finish_kernel(const int32_t* __restrict__ indptr, int nrows, int nitems, int item,
                                                                           int N, int mean, const float* __restrict__ part,
                                                                           float* __restrict__ out, int64_t ldo) {
  const int j = blockIdx.x * kWavesPerBlock + threadIdx.x / kWave + 1;
  if (j >= nitems) return;
  const int p = j * item;
  const int r = eb_row_of(indptr, nrows, p);
  const int rb = indptr[r], re = indptr[r + 1];
  const int t0 = rb / item;
  if (rb >= p || t0 + 1 != j) return;
  const int t1 = (re - 1) / item;
  for (int n = threadIdx.x & (kWave - 1); n < N; n += kWave) {
    float s = part[((int64_t)t0 * 2 + 1) * kEbPartLd + n];
    for (int t = t0 + 1; t <= t1; ++t) s += part[(int64_t)t * 2 * kEbPartLd + n];
    out[(int64_t)r * ldo + n] = mean ? s / (float)(re - rb) : s;
  }
}

// ---- weight gradient
struct GwArgs {
  const int32_t *indptr, *indices, *eids;
  int nrows, nnz, chunk;
  int DH, KT, I, O, IB, OB;  // KT = DH + (bias ? 1 : 0) values of k; IB x OB blocks of 64 x 64
  const float *h, *x, *g;
  int64_t ldh, ldx, ldg;
  float* part;
};

template <int IT, int JT>
__global__ __launch_bounds__(kEbBlock) void edge_bilinear_grad_w_kernel(const GwArgs a) {
  __shared__ float xs[kGwEdges * kGwLd], gs[kGwEdges * kGwLd], hs[kEbWaves][kGwEdges];
  __shared__ int src_s[kGwEdges], dst_s[kGwEdges], eid_s[kGwEdges];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int c = lane % 16, q = lane / 16;
  const int e0 = blockIdx.x * a.chunk, e1 = e0 + a.chunk < a.nnz ? e0 + a.chunk : a.nnz;
  const int units = a.KT * a.IB * a.OB, per_k = a.IB * a.OB;
  const int u = blockIdx.y * kEbWaves + wave;
  const bool valid = u < units;
  const int k = u / per_k, ib = (u - k * per_k) / a.OB, ob = u - k * per_k - ib * a.OB;
  const int Ip = (a.I + 15) & ~15, Op = (a.O + 15) & ~15;
  v4f acc[IT][JT];
#pragma unroll
  for (int i = 0; i < IT; ++i)
#pragma unroll
    for (int j = 0; j < JT; ++j) acc[i][j] = (v4f)(0.f);
  for (int s0 = e0; s0 < e1; s0 += kGwEdges) {
    __syncthreads();  // the stage before has been read
    if (tid < kGwEdges) {
      const int p = s0 + tid;
      const bool ok = p < e1;
      src_s[tid] = ok ? a.indices[p] : -1;
      dst_s[tid] = ok ? eb_row_of(a.indptr, a.nrows, p) : -1;
      eid_s[tid] = ok ? (a.eids ? a.eids[p] : p) : -1;
    }
    __syncthreads();
    for (int e = tid; e < kGwEdges * Ip; e += kEbBlock) {
      const int r = e / Ip, i = e - r * Ip;
      xs[r * kGwLd + i] = (src_s[r] >= 0 && i < a.I) ? a.x[(int64_t)src_s[r] * a.ldx + i] : 0.f;
    }
    for (int e = tid; e < kGwEdges * Op; e += kEbBlock) {
      const int r = e / Op, o = e - r * Op;
      gs[r * kGwLd + o] = (dst_s[r] >= 0 && o < a.O) ? a.g[(int64_t)dst_s[r] * a.ldg + o] : 0.f;
    }
    if (tid < kEbWaves * kGwEdges) {
      const int w = tid / kGwEdges, e = tid % kGwEdges;
      const int uw = blockIdx.y * kEbWaves + w, kw = uw / per_k;
      hs[w][e] = (uw >= units || eid_s[e] < 0) ? 0.f : kw < a.DH ? a.h[(int64_t)eid_s[e] * a.ldh + kw] : 1.f;
    }
    __syncthreads();
    if (valid) {
      // columns of a 64-wide block beyond the padded width hold stale values: they reach only accumulator elements that are not stored
#pragma unroll
      for (int s = 0; s < kGwEdges / 4; ++s) {
        const int e = 4 * s + q;
        const float hv = hs[wave][e];
        float av[IT], bv[JT];
#pragma unroll
        for (int i = 0; i < IT; ++i) av[i] = hv * xs[e * kGwLd + 64 * ib + 16 * i + c];
#pragma unroll
        for (int j = 0; j < JT; ++j) bv[j] = gs[e * kGwLd + 64 * ob + 16 * j + c];
#pragma unroll
        for (int i = 0; i < IT; ++i)
#pragma unroll
          for (int j = 0; j < JT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[j], acc[i][j], 0, 0, 0);
      }
    }
  }
  if (!valid) return;
  // accumulator element r of tile (i, j) in lane (c, q) = the sum for (64 ib + 16 i + 4 q + r, 64 ob + 16 j + c)
  float* __restrict__ p = a.part + ((int64_t)blockIdx.x * a.KT + k) * a.I * a.O;
#pragma unroll
  for (int i = 0; i < IT; ++i)
#pragma unroll
    for (int j = 0; j < JT; ++j) {
      const int o = 64 * ob + 16 * j + c;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ii = 64 * ib + 16 * i + 4 * q + r;
        if (ii < a.I && o < a.O) p[ii * a.O + o] = acc[i][j][r];
      }
    }
}

// d Theta / d B element e = the partials of the chunks added in chunk order: thread (e, sl) adds slice sl of the chunk list, the 16
// slices are added in slice order.  16 elements per workgroup.
__global__ __launch_bounds__(kBlock) void edge_bilinear_grad_w_finish_kernel(int64_t tile, int64_t theta, int chunks, const float* __restrict__ part,
                                                                             float* __restrict__ d_theta, float* __restrict__ d_bias) {
  __shared__ float red[16][17];
  const int64_t e = (int64_t)blockIdx.x * 16 + threadIdx.x % 16;
  const int sl = threadIdx.x / 16;
  const int per = (chunks + 15) / 16;
  float s = 0.f;
  if (e < tile) {
    const int lo = sl * per, hi = lo + per < chunks ? lo + per : chunks;
    for (int w = lo; w < hi; ++w) s += part[w * tile + e];
  }
  red[sl][threadIdx.x % 16] = s;
  __syncthreads();
  if (sl == 0 && e < tile) {
    float sum = 0.f;
    for (int i = 0; i < 16; ++i) sum += red[i][threadIdx.x % 16];
    if (e < theta) d_theta[e] = sum; else d_bias[e - theta] = sum;
  }
}

static bool eb_shape_ok(int64_t DH, int64_t I, int64_t O) { return DH >= 1 && I >= 1 && I <= 128 && O >= 1 && O <= 128; }
static int64_t eb_items(int64_t nnz, int64_t item) { return (nnz + item - 1) / item; }
static int64_t gw_chunk(int64_t nnz) {
  const int64_t chunk = round_up((nnz + kGwMaxChunks - 1) / kGwMaxChunks, kGwEdges);
  return chunk < kGwMinChunk ? kGwMinChunk : chunk;
}

template <int MT, int KCQ>
static void eb_launch(const EbArgs& a, bool rowsum, unsigned blocks, hipStream_t s) {
  if (rowsum)
    hipLaunchKernelGGL((edge_bilinear_kernel<MT, KCQ, true>), dim3(blocks), dim3(kEbBlock), 0, s, a);
  else
    hipLaunchKernelGGL((edge_bilinear_kernel<MT, KCQ, false>), dim3(blocks), dim3(kEbBlock), 0, s, a);
}

template <int IT>
static bool gw_launch(int jt, const GwArgs& a, dim3 grid, hipStream_t s) {
  switch (jt) {
    case 1: hipLaunchKernelGGL((edge_bilinear_grad_w_kernel<IT, 1>), grid, dim3(kEbBlock), 0, s, a); return true;
    case 2: hipLaunchKernelGGL((edge_bilinear_grad_w_kernel<IT, 2>), grid, dim3(kEbBlock), 0, s, a); return true;
    case 4: hipLaunchKernelGGL((edge_bilinear_grad_w_kernel<IT, 4>), grid, dim3(kEbBlock), 0, s, a); return true;
  }
  return false;
}
static int gw_tiles(int64_t w) { return w <= 16 ? 1 : w <= 32 ? 2 : 4; }

static int32_t eb_csr_check(const mgx_csr* csr, const char* who) {
  MGX_CHECK_ARG(csr && csr->num_rows >= 0 && csr->num_cols >= 0 && csr->nnz >= 0, "%s: bad CSR", who);
  MGX_CHECK_ARG(csr->nnz == 0 || (csr->indptr && csr->indices), "%s: CSR without indptr / indices", who);
  if (csr->idx_bits != 32) MGX_UNSUPPORTED("%s: needs 32-bit graph indices", who);
  if (csr->nnz == 0) MGX_UNSUPPORTED("%s: needs at least one edge", who);
  if (csr->nnz >= (int64_t(1) << 30) || csr->num_rows >= (int64_t(1) << 30)) MGX_UNSUPPORTED("%s: needs fewer than 2^30 edges and rows", who);
  return MGX_OK;
}

}  // namespace mgx

extern "C" int32_t mgx_edge_bilinear_supported(const mgx_csr* csr, int64_t DH, int64_t I, int64_t O) {
  using namespace mgx;
  if (!csr || csr->idx_bits != 32 || csr->nnz <= 0 || !eb_shape_ok(DH, I, O)) return 0;
  const int64_t rows = csr->num_rows > csr->num_cols ? csr->num_rows : csr->num_cols;
  const int64_t lim = int64_t(1) << 30;  // operands within 32-bit byte offsets
  return (csr->nnz < lim / DH && rows < lim / 128 && DH * I * O < lim) ? 1 : 0;
}

extern "C" int64_t mgx_edge_bilinear_workspace(int64_t nnz, int64_t DH, int64_t I, int64_t O, int64_t item_edges, int32_t grad_w) {
  using namespace mgx;
  if (nnz < 0 || !eb_shape_ok(DH, I, O) || item_edges < 16 || item_edges > kEbMaxItem || item_edges % 16) return -1;
  if (!grad_w) return eb_items(nnz, item_edges) * 2 * kEbPartLd * (int64_t)sizeof(float);
  return eb_items(nnz, gw_chunk(nnz)) * (DH + 1) * I * O * (int64_t)sizeof(float);
}

extern "C" int32_t mgx_edge_bilinear(const mgx_csr* csr, int64_t A, int64_t B, int64_t N, const float* P, int64_t ldp, int32_t p_index,
                                     const float* Q, int64_t ldq, int32_t q_index, const float* W, int64_t w_sa, int64_t w_sb, int64_t w_sn,
                                     const float* W_one, int64_t one_sb, int64_t one_sn, int32_t epilogue, float* out, int64_t ldo,
                                     int64_t item_edges, void* workspace, void* stream) {
  using namespace mgx;
  MGX_ENTER();
  int32_t st = eb_csr_check(csr, "mgx_edge_bilinear");
  if (st != MGX_OK) return st;
  MGX_CHECK_ARG(A >= 1 && B >= 1 && N >= 1, "mgx_edge_bilinear: bad sizes (A %lld, B %lld, N %lld)", (long long)A, (long long)B, (long long)N);
  MGX_CHECK_ARG(P && Q && W && out, "mgx_edge_bilinear: NULL pointer");
  MGX_CHECK_ARG(p_index >= MGX_EB_BY_EDGE && p_index <= MGX_EB_BY_ROW && q_index >= MGX_EB_BY_EDGE && q_index <= MGX_EB_BY_ROW,
                "mgx_edge_bilinear: unknown index mode");
  MGX_CHECK_ARG(epilogue >= MGX_EB_STORE_BY_EDGE && epilogue <= MGX_EB_ROW_MEAN, "mgx_edge_bilinear: unknown epilogue");
  MGX_CHECK_ARG(item_edges >= 16 && item_edges <= kEbMaxItem && item_edges % 16 == 0,
                "mgx_edge_bilinear: item_edges must be a multiple of 16 in 16 .. %d, got %lld", kEbMaxItem, (long long)item_edges);
  MGX_CHECK_ARG(ldp >= A && ldq >= B && ldo >= N, "mgx_edge_bilinear: leading dimensions smaller than the operands");
  const bool rowsum = epilogue != MGX_EB_STORE_BY_EDGE;
  MGX_CHECK_ARG(!rowsum || workspace, "mgx_edge_bilinear: the row-sum epilogue needs its workspace");
  if (B > 128 || (rowsum && N > 128)) MGX_UNSUPPORTED("mgx_edge_bilinear: needs B <= 128 and, for a row sum, N <= 128 (got %lld, %lld)", (long long)B, (long long)N);
  hipStream_t s = (hipStream_t)stream;
  EbArgs a;
  memset(&a, 0, sizeof(a));
  a.indptr = (const int32_t*)csr->indptr; a.indices = (const int32_t*)csr->indices; a.eids = (const int32_t*)csr->eids;
  a.nrows = (int)csr->num_rows; a.nnz = (int)csr->nnz; a.item = (int)item_edges;
  a.A = (int)A; a.B = (int)B; a.KC = (int)((B + 15) / 16); a.has_one = W_one ? 1 : 0;
  a.P = P; a.Q = Q; a.W1 = W_one;
  a.ldp = ldp; a.ldq = ldq; a.sa = w_sa; a.sb = w_sb; a.sn = w_sn; a.sb1 = one_sb; a.sn1 = one_sn; a.ldo = ldo;
  a.p_mode = p_index; a.q_mode = q_index; a.mean = epilogue == MGX_EB_ROW_MEAN;
  a.part = (float*)workspace;
  const int64_t nitems = eb_items(csr->nnz, item_edges);
  for (int64_t n0 = 0; n0 < N; n0 += 128) {  // wider than 128 columns: the store epilogue only (d h with DH > 128)
    a.N = (int)(N - n0 < 128 ? N - n0 : 128);
    a.W = W + n0 * w_sn;
    a.out = out + n0;
    const bool wide = a.N > 64;
    if (a.KC <= 4) { if (wide) eb_launch<8, 4>(a, rowsum, (unsigned)nitems, s); else eb_launch<4, 4>(a, rowsum, (unsigned)nitems, s); }
    else { if (wide) eb_launch<8, 8>(a, rowsum, (unsigned)nitems, s); else eb_launch<4, 8>(a, rowsum, (unsigned)nitems, s); }
    MGX_CHECK_LAUNCH();
  }
  if (rowsum && nitems > 1) {
    hipLaunchKernelGGL(edge_bilinear_rows_finish_kernel, dim3((unsigned)((nitems - 1 + kWavesPerBlock - 1) / kWavesPerBlock)), dim3(kBlock), 0, s,
                       a.indptr, a.nrows, (int)nitems, a.item, (int)N, a.mean, (const float*)a.part, out, ldo);
    MGX_CHECK_LAUNCH();
  }
  note_spmm_kernel(rowsum ? "edge_bilinear_rows" : "edge_bilinear_edges");
  return MGX_OK;
}

extern "C" int32_t mgx_edge_bilinear_grad_w(const mgx_csr* csr, int64_t DH, int64_t I, int64_t O, const float* h, int64_t ldh, const float* x,
                                            int64_t ldx, const float* g, int64_t ldg, float* d_theta, float* d_bias, void* workspace,
                                            void* stream) {
  using namespace mgx;
  MGX_ENTER();
  int32_t st = eb_csr_check(csr, "mgx_edge_bilinear_grad_w");
  if (st != MGX_OK) return st;
  MGX_CHECK_ARG(DH >= 1 && I >= 1 && O >= 1, "mgx_edge_bilinear_grad_w: bad sizes (DH %lld, I %lld, O %lld)", (long long)DH, (long long)I, (long long)O);
  MGX_CHECK_ARG(h && x && g && d_theta && workspace, "mgx_edge_bilinear_grad_w: NULL pointer");
  MGX_CHECK_ARG(ldh >= DH && ldx >= I && ldg >= O, "mgx_edge_bilinear_grad_w: leading dimensions smaller than the operands");
  if (!eb_shape_ok(DH, I, O)) MGX_UNSUPPORTED("mgx_edge_bilinear_grad_w: needs I, O <= 128 (got %lld, %lld)", (long long)I, (long long)O);
  hipStream_t s = (hipStream_t)stream;
  GwArgs a;
  memset(&a, 0, sizeof(a));
  a.indptr = (const int32_t*)csr->indptr; a.indices = (const int32_t*)csr->indices; a.eids = (const int32_t*)csr->eids;
  a.nrows = (int)csr->num_rows; a.nnz = (int)csr->nnz; a.chunk = (int)gw_chunk(csr->nnz);
  a.DH = (int)DH; a.KT = (int)DH + (d_bias ? 1 : 0); a.I = (int)I; a.O = (int)O; a.IB = (int)((I + 63) / 64); a.OB = (int)((O + 63) / 64);
  a.h = h; a.x = x; a.g = g; a.ldh = ldh; a.ldx = ldx; a.ldg = ldg;
  a.part = (float*)workspace;
  const int chunks = (int)eb_items(csr->nnz, a.chunk);
  const int units = a.KT * a.IB * a.OB;
  const dim3 grid((unsigned)chunks, (unsigned)((units + kEbWaves - 1) / kEbWaves));
  const int it = gw_tiles(I), jt = gw_tiles(O);
  const bool ok = it == 1 ? gw_launch<1>(jt, a, grid, s) : it == 2 ? gw_launch<2>(jt, a, grid, s) : gw_launch<4>(jt, a, grid, s);
  MGX_CHECK_ARG(ok, "mgx_edge_bilinear_grad_w: no kernel for this block");
  MGX_CHECK_LAUNCH();
  const int64_t tile = (int64_t)a.KT * I * O;
  hipLaunchKernelGGL(edge_bilinear_grad_w_finish_kernel, dim3((unsigned)((tile + 15) / 16)), dim3(kBlock), 0, s, tile, DH * I * O, chunks,
                     (const float*)a.part, d_theta, d_bias);
  MGX_CHECK_LAUNCH();
  note_spmm_kernel("edge_bilinear_grad_w");
  return MGX_OK;
}
