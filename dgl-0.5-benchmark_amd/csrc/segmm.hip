// segmm.hip -- typed linear layers: one weight matrix per row SEGMENT (gfx950 / MI355X, wave64, fp32 MFMA 16x16x4).
//   mgx_segment_mm         C[c_rows[p]] = A[a_rows[p]] x B[seg(p)]           positions offsets[r] .. offsets[r + 1] - 1 use B[r]
//   mgx_segment_mm_grad_b  dB[r] = sum_{p in segment r} A[a_rows[p]]^T dC[c_rows[p]]
// dgl.ops.segment_mm / gather_mm, TypedLinear and the per-edge-type RelGraphConv of DGL >= 0.8: R = tens to hundreds of [K, M] weights over
// millions of rows.  The input gradient is mgx_segment_mm itself with b_transposed.  No atomics, fixed summation order.
//
// WORK ITEMS.  The unit of work is a run of rows INSIDE one segment -- at most `unit` rows from offsets[r] + i * unit on -- so nothing ever
// straddles two weights.  Nothing about the segment lengths is known on the host: seg_items_kernel (seg_items.h; one workgroup, any R) turns offsets
// into the scanned per-segment item counts table[R + 1]; the main grid has the host-known bound ceil(n / unit) + R, a workgroup (a wave in
// the gradient) finds its segment by binary search in the table and leaves when it is beyond table[R].  The launch depends on n, R, K, M only.
// A segment whose offsets do not lie in 0 <= beg <= end <= n gets no item.
//
// FORWARD.  A workgroup of 8 waves stages B[r] once per item in LDS in the order the lanes read it (rows_gemm's labelling: chunk of 16 k,
// column tile, lane, component; zero-padded to K_pad x M_pad), read from global memory in rows -- 16 bytes per lane where B allows it.  Wave w
// takes the item's 16-row tiles w, w + 8, ...  Unlike rows_gemm the K dimension is a RUN-TIME loop, in groups of 64 k (16 registers per lane):
// the (tile, group) pairs of a wave form one stream, and the registers of the pair after the current one are loaded before the current
// pair's MFMAs issue -- the next tile's first group behind the last group of this one, its row-list entry fetched a tile earlier still.
// One instantiation per number of column tiles and operand form (8 in all) serves every K.  Column tiles inside a group of 64 columns are
// relabelled so that a lane holds four consecutive columns in four accumulators: one float4 store per row and group.
//   float4 form: lane (c, q) loads A[row0 + c][64 kg + 16 jj + 4 q .. + 3]; dword form (K % 4 != 0 or A not 16-byte aligned by rows): lane (c, q)
//   loads A[row0 + c][64 kg + 4 s + q].  B is staged to pair with either.
//
// WEIGHT GRADIENT.  The MFMA's i is the k index, j the m index, and its reduction runs over the rows of the segment (xty.hip's orientation:
// operands straight from global memory, no LDS).  An item is a row chunk of one segment walked by ONE wave, which holds a 64 x 64 block of
// the [K, M] sum in accumulators (wider sums: one launch per block) and writes it as the item's partial; the finish kernel adds the
// partials of a segment in item order -- 16 slices of the item list per element, the slices in slice order -- and writes zeros for a
// segment without rows.  (xty.hip's walk is tied to its grid-stride row order and has neither segment bounds nor two row lists, so the
// body is restated here in the segment form rather than shared.)
#include "common.h"
#include "seg_items.h"

namespace mgx {

constexpr int kSegLdsFloats = 16384;  // 64 KB: K_pad x M_pad of one B[r]
constexpr int kSegBlock = 512;        // 8 waves share one stage of B[r]
constexpr int kSegWaves = kSegBlock / kWave;
constexpr int kSegXtyItems = 2048;    // the weight gradient aims at this many row chunks (partial tiles) ...
constexpr int kSegXtyMinRows = 256;   // ... of at least this many rows

static inline int64_t seg_pad(int64_t x, int64_t m) { return (x + m - 1) / m * m; }
static bool seg_shape_ok(int64_t K, int64_t M) { return K >= 1 && M >= 1 && M <= 256 && seg_pad(K, 16) * seg_pad(M, 64) <= kSegLdsFloats; }

// rows per chunk of the weight gradient: a multiple of 16; large tiles get fewer, longer chunks (the partials are K x M floats each)
static int64_t seg_xty_chunk(int64_t n, int64_t K, int64_t M) {
  const int64_t items = K * M > 4096 ? kSegXtyItems / 2 : kSegXtyItems;
  int64_t chunk = seg_pad((n + items - 1) / items, 16);
  return chunk < kSegXtyMinRows ? kSegXtyMinRows : chunk;
}

// MT = column tiles of 16 (a multiple of 4: groups of 64 columns), KC = chunks of 16 k (run time)
template <int MT, bool V4>
__global__ __launch_bounds__(kSegBlock, MT <= 8 ? 4 : 2) void segment_mm_kernel(
    int64_t R, int K, int M, int KC, const float* __restrict__ A, int64_t lda, const int64_t* __restrict__ a_rows, const float* __restrict__ B,
    int b_transposed, const int64_t* __restrict__ offsets, const int64_t* __restrict__ table, int64_t item_rows, float* __restrict__ C,
    int64_t ldc, const int64_t* __restrict__ c_rows) {
  __shared__ float Bl[kSegLdsFloats];
  int64_t seg, beg, cnt;
  if (!seg_item(table, offsets, R, blockIdx.x, item_rows, seg, beg, cnt)) return;
  // ---- stage B[seg]: element (chunk jj, tile mt, lane (c, q), component t) = B[k][m] with k = 16 jj + (V4 ? 4 q + t : 4 t + q) and
  // m = 64 (mt / 4) + 4 c + mt % 4, stored [jj][mt][lane][t]: one ds_read_b128 per (chunk, tile) in the MFMA loop
  const float* __restrict__ Bb = B + seg * (int64_t)K * M;
  auto dest = [&](int k, int m) {
    const int jj = k >> 4, w = k & 15;
    const int q = V4 ? w >> 2 : w & 3, t = V4 ? w & 3 : w >> 2;
    const int mt = 4 * (m >> 6) + (m & 3), c = (m & 63) >> 2;
    return ((jj * MT + mt) * 64 + 16 * q + c) * 4 + t;
  };
  {
    // walked in B's own row order (m fastest, or k fastest when transposed), padding included: consecutive threads read consecutive floats
    const int inner = b_transposed ? K : M, outer = b_transposed ? M : K;
    const int innerP = b_transposed ? KC * 16 : MT * 16, outerP = b_transposed ? MT * 16 : KC * 16;
    if (inner % 4 == 0 && (uintptr_t)B % 16 == 0) {
      const int iv = innerP / 4;
      for (int e = threadIdx.x; e < iv * outerP; e += kSegBlock) {
        const int o = e / iv, i0 = (e - o * iv) * 4;
        v4f v = (v4f)(0.f);
        if (o < outer && i0 < inner) v = *reinterpret_cast<const v4f*>(Bb + (int64_t)o * inner + i0);
#pragma unroll
        for (int t = 0; t < 4; ++t) Bl[b_transposed ? dest(i0 + t, o) : dest(o, i0 + t)] = v[t];
      }
    } else {
      for (int e = threadIdx.x; e < innerP * outerP; e += kSegBlock) {
        const int o = e / innerP, i = e - o * innerP;
        const float v = (o < outer && i < inner) ? Bb[(int64_t)o * inner + i] : 0.f;
        Bl[b_transposed ? dest(i, o) : dest(o, i)] = v;
      }
    }
  }
  __syncthreads();

  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int c = lane % 16, q = lane / 16;
  const int ntiles = (int)((cnt + 15) >> 4);
  if (wave >= ntiles) return;
  const int KG = (KC + 3) >> 2;  // groups of 64 k
  const int64_t last = beg + cnt - 1;
  // this lane's source row of the item's tile t; a position beyond the item reads the item's last row instead (row i of A only reaches
  // row i of C, which is not stored)
  auto src_of = [&](int t) {
    int64_t p = beg + 16 * (int64_t)t + c;
    if (p > last) p = last;
    return a_rows ? a_rows[p] : p;
  };
  // group kg of a row: a[4 jj + t] pairs with component t of chunk 4 kg + jj of the stage
  auto load_group = [&](float (&a)[16], int64_t src, int kg) {
    const float* __restrict__ ap = A + src * lda + 64 * kg;
    if (V4) {
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const int k0 = 16 * jj + 4 * q;
        const v4f v = (64 * kg + k0 < K) ? *reinterpret_cast<const v4f*>(ap + k0) : (v4f)(0.f);
        a[4 * jj + 0] = v.x; a[4 * jj + 1] = v.y; a[4 * jj + 2] = v.z; a[4 * jj + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int s = 0; s < 16; ++s) a[s] = (64 * kg + 4 * s + q < K) ? ap[4 * s + q] : 0.f;
    }
  };
  const bool cvec = ldc % 4 == 0 && (uintptr_t)C % 16 == 0 && M % 4 == 0;
  float cur[16], nxt[16];
  int64_t s_cur = src_of(wave), s_nxt = src_of(wave + kSegWaves);
  load_group(cur, s_cur, 0);
  for (int t = wave; t < ntiles; t += kSegWaves) {
    // the list entry of the tile after next and where this tile's rows go, BEFORE the operand loads of the next pair are issued: loads
    // return in order
    const int64_t s_after = src_of(t + 2 * kSegWaves);
    int64_t to[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t p = beg + 16 * (int64_t)t + 4 * q + r;
      to[r] = p > last ? (int64_t)-1 : c_rows ? c_rows[p] : p;
    }
    v4f acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] = (v4f)(0.f);
    for (int kg = 0; kg < KG; ++kg) {
      if (kg + 1 < KG) load_group(nxt, s_cur, kg + 1); else load_group(nxt, s_nxt, 0);
      // B stays in LDS: an address the compiler cannot prove loop-invariant keeps it from hoisting the fragments into registers
      int lo = lane;
      asm volatile("" : "+v"(lo));
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const int jg = 4 * kg + jj;
        if (jg < KC) {  // wave-uniform
#pragma unroll
          for (int g = 0; g < MT / 4; ++g) {
            v4f b[4];  // four column tiles of this chunk, then four INDEPENDENT accumulators between two uses of the same one
#pragma unroll
            for (int i = 0; i < 4; ++i) b[i] = *reinterpret_cast<const v4f*>(&Bl[((jg * MT + 4 * g + i) * 64 + lo) * 4]);
#pragma unroll
            for (int tt = 0; tt < 4; ++tt)
#pragma unroll
              for (int i = 0; i < 4; ++i)
                acc[4 * g + i] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur[4 * jj + tt], b[i][tt], acc[4 * g + i], 0, 0, 0);
          }
        }
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) cur[i] = nxt[i];
    }
    s_cur = s_nxt;
    s_nxt = s_after;
    // accumulator element r of tile 4 g + i = C[row 4 q + r of the tile][64 g + 4 c + i]
#pragma unroll
    for (int g = 0; g < MT / 4; ++g) {
      const int m0 = 64 * g + 4 * c;
      if (m0 >= M) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (to[r] < 0) continue;
        float* dst = C + to[r] * ldc + m0;
        if (cvec) {
          v4f o; o.x = acc[4 * g + 0][r]; o.y = acc[4 * g + 1][r]; o.z = acc[4 * g + 2][r]; o.w = acc[4 * g + 3][r];
          *reinterpret_cast<v4f*>(dst) = o;
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (m0 + i < M) dst[i] = acc[4 * g + i][r];
        }
      }
    }
  }
}

// ---- weight gradient: one wave per row chunk, a (<= 64) x (<= 64) block of A^T dC in IT x JT accumulators of 16 x 16.
// AV / DV: the operand arrives as one float4 per lane and row (lane c holds columns 4 c .. 4 c + 3, i.e. index c of FOUR tiles: tile t
// stands for the columns 4 x + t), else as IT / JT dwords (tile i = columns 16 i ..).  Kw, Mw: the widths of this block.
template <int IT, bool AV, int JT, bool DV>
__global__ __launch_bounds__(kBlock) void segment_xty_kernel(int64_t R, int Kw, int Mw, const float* __restrict__ A, int64_t lda,
                                                             const int64_t* __restrict__ a_rows, const float* __restrict__ D, int64_t ldd,
                                                             const int64_t* __restrict__ d_rows, const int64_t* __restrict__ offsets,
                                                             const int64_t* __restrict__ table, int64_t chunk, int64_t max_items,
                                                             float* __restrict__ part, int ldp, int64_t tile) {
  static_assert((!AV || IT == 4) && (!DV || JT == 4), "a float4 operand is four tiles");
  const int lane = threadIdx.x & (kWave - 1);
  const int c = lane % 16, q = lane / 16;
  const int64_t item = (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
  int64_t seg, beg, cnt;
  // (max_items: the partials the workspace holds -- offsets that are not ascending could ask for more)
  if (item >= max_items || !seg_item(table, offsets, R, item, chunk, seg, beg, cnt)) return;
  const int64_t end = beg + cnt;
  v4f acc[IT][JT];
#pragma unroll
  for (int i = 0; i < IT; ++i)
#pragma unroll
    for (int j = 0; j < JT; ++j) acc[i][j] = (v4f)(0.f);
  // row indices fit 32 bits (the entry points check n * ld < 2^30); -1: a position beyond the chunk, nothing read, zeros multiplied
  auto row_at = [&](const int64_t* __restrict__ list, int64_t p) { return p < end ? (int)(list ? list[p] : p) : -1; };
  int na[4], nd[4];  // the lists a step ahead: an operand address never waits for its list entry
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    na[s] = row_at(a_rows, beg + 4 * s + q);
    nd[s] = row_at(d_rows, beg + 4 * s + q);
  }
  for (int64_t r0 = beg; r0 < end; r0 += 16) {
    int ia[4], id[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      ia[s] = na[s];
      id[s] = nd[s];
      na[s] = row_at(a_rows, r0 + 16 + 4 * s + q);
      nd[s] = row_at(d_rows, r0 + 16 + 4 * s + q);
    }
    float a[4][IT], b[4][JT];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const bool ok = ia[s] >= 0;
      if (AV) {
        const v4f v = (ok && 4 * c < Kw) ? *reinterpret_cast<const v4f*>(A + (int64_t)ia[s] * lda + 4 * c) : (v4f)(0.f);
        a[s][0] = v.x; a[s][1] = v.y; a[s][2] = v.z; a[s][3] = v.w;
      } else {
#pragma unroll
        for (int i = 0; i < IT; ++i) a[s][i] = (ok && 16 * i + c < Kw) ? A[(int64_t)ia[s] * lda + 16 * i + c] : 0.f;
      }
      if (DV) {
        const v4f v = (ok && 4 * c < Mw) ? *reinterpret_cast<const v4f*>(D + (int64_t)id[s] * ldd + 4 * c) : (v4f)(0.f);
        b[s][0] = v.x; b[s][1] = v.y; b[s][2] = v.z; b[s][3] = v.w;
      } else {
#pragma unroll
        for (int j = 0; j < JT; ++j) b[s][j] = (ok && 16 * j + c < Mw) ? D[(int64_t)id[s] * ldd + 16 * j + c] : 0.f;
      }
    }
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int i = 0; i < IT; ++i)
#pragma unroll
        for (int j = 0; j < JT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s][i], b[s][j], acc[i][j], 0, 0, 0);
  }
  // accumulator element r of tile (i, j) in lane (c, q) is the sum for (k, m) = the real columns behind (tile i, index 4 q + r) / (tile j, index c)
  float* __restrict__ p = part + item * tile;
#pragma unroll
  for (int i = 0; i < IT; ++i)
#pragma unroll
    for (int j = 0; j < JT; ++j) {
      const int m = DV ? 4 * c + j : 16 * j + c;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int k = AV ? 4 * (4 * q + r) + i : 16 * i + 4 * q + r;
        if (k < Kw && m < Mw) p[k * ldp + m] = acc[i][j][r];
      }
    }
}

// dB[r][e] = the partials of segment r's items added in item order: thread (e, sl) adds slice sl of the item list, the 16 slices are
// added in slice order.  A segment without items gets zeros.  16 elements per workgroup, blockIdx.x over R x ceil(tile / 16).
__global__ __launch_bounds__(kBlock) void segment_xty_finish_kernel(int64_t tile, int64_t blocks_per_seg, int64_t max_items,
                                                                    const int64_t* __restrict__ table, const float* __restrict__ part,
                                                                    float* __restrict__ out) {
  __shared__ float red[16][17];
  const int64_t seg = blockIdx.x / blocks_per_seg;
  const int64_t e = (blockIdx.x - seg * blocks_per_seg) * 16 + threadIdx.x % 16;
  const int sl = threadIdx.x / 16;
  const int64_t first = table[seg] < max_items ? table[seg] : max_items;
  const int64_t items = (table[seg + 1] < max_items ? table[seg + 1] : max_items) - first;
  const int64_t per = (items + 15) / 16;
  float s = 0.f;
  if (e < tile) {
    const int64_t lo = sl * per, hi = lo + per < items ? lo + per : items;
    const float* __restrict__ p = part + first * tile + e;
#pragma unroll 4
    for (int64_t w = lo; w < hi; ++w) s += p[w * tile];
  }
  red[sl][threadIdx.x % 16] = s;
  __syncthreads();
  if (sl == 0 && e < tile) {
    float sum = 0.f;
    for (int i = 0; i < 16; ++i) sum += red[i][threadIdx.x % 16];
    out[seg * tile + e] = sum;
  }
}

template <int IT, bool AV>
static bool launch_seg_xty_d(int jt, bool dv, dim3 grid, hipStream_t s, int64_t R, int Kw, int Mw, const float* A, int64_t lda,
                             const int64_t* a_rows, const float* D, int64_t ldd, const int64_t* d_rows, const int64_t* offsets,
                             const int64_t* table, int64_t chunk, int64_t max_items, float* part, int ldp, int64_t tile) {
#define MGX_SEGX(JT_, DV_)                                                                                                               \
  if (jt == JT_ && dv == DV_) {                                                                                                          \
    hipLaunchKernelGGL((segment_xty_kernel<IT, AV, JT_, DV_>), grid, dim3(kBlock), 0, s, R, Kw, Mw, A, lda, a_rows, D, ldd, d_rows,       \
                       offsets, table, chunk, max_items, part, ldp, tile);                                                              \
    return true;                                                                                                                         \
  }
  MGX_SEGX(1, false) MGX_SEGX(2, false) MGX_SEGX(4, false) MGX_SEGX(4, true)
#undef MGX_SEGX
  return false;
}

// the form of one operand block of `w` columns: (tiles, float4 loads)
static void seg_xty_form(int w, bool vec_ok, int& tiles, bool& vec) {
  vec = vec_ok && w > 32 && w % 4 == 0;
  tiles = w <= 16 ? 1 : w <= 32 ? 2 : 4;
}

template <int MT>
static void launch_segment_mm(bool v4, unsigned blocks, hipStream_t s, int64_t R, int K, int M, int KC, const float* a, int64_t lda,
                              const int64_t* a_rows, const float* b, int bt, const int64_t* offsets, const int64_t* table, int64_t item_rows,
                              float* c, int64_t ldc, const int64_t* c_rows) {
  if (v4)
    hipLaunchKernelGGL((segment_mm_kernel<MT, true>), dim3(blocks), dim3(kSegBlock), 0, s, R, K, M, KC, a, lda, a_rows, b, bt, offsets, table,
                       item_rows, c, ldc, c_rows);
  else
    hipLaunchKernelGGL((segment_mm_kernel<MT, false>), dim3(blocks), dim3(kSegBlock), 0, s, R, K, M, KC, a, lda, a_rows, b, bt, offsets, table,
                       item_rows, c, ldc, c_rows);
}

}  // namespace mgx

extern "C" int32_t mgx_segment_mm_supported(int64_t K, int64_t M) { return mgx::seg_shape_ok(K, M) ? 1 : 0; }

extern "C" int64_t mgx_segment_mm_workspace(int64_t n, int64_t R, int64_t K, int64_t M, int32_t grad_b) {
  using namespace mgx;
  if (n < 0 || R < 0 || !seg_shape_ok(K, M)) return -1;
  const int64_t table = seg_pad((R + 1) * (int64_t)sizeof(int64_t), 256);
  if (!grad_b) return table;
  const int64_t items = (n + seg_xty_chunk(n, K, M) - 1) / seg_xty_chunk(n, K, M) + R;
  return table + items * K * M * (int64_t)sizeof(float);
}

extern "C" int32_t mgx_segment_mm(int64_t n, int64_t R, int64_t K, int64_t M, const float* a, int64_t lda, const int64_t* a_rows,
                                  const float* b, int32_t b_transposed, const int64_t* offsets, float* c, int64_t ldc, const int64_t* c_rows,
                                  int64_t item_rows, void* workspace, void* stream) {
  using namespace mgx;
  MGX_ENTER();
  MGX_CHECK_ARG(n >= 0 && R >= 0 && K >= 1 && M >= 1, "mgx_segment_mm: bad sizes (n %lld, R %lld, K %lld, M %lld)", (long long)n,
                (long long)R, (long long)K, (long long)M);
  MGX_CHECK_ARG(n > 0 || (!a_rows && !c_rows), "mgx_segment_mm: a row list without rows");
  MGX_CHECK_ARG(item_rows >= 16 && item_rows % 16 == 0, "mgx_segment_mm: item_rows must be a positive multiple of 16, got %lld", (long long)item_rows);
  if (!seg_shape_ok(K, M))
    MGX_UNSUPPORTED("mgx_segment_mm: needs M <= 256 and K x M padded to 16 x 64 within %d floats (got %lld x %lld)", kSegLdsFloats, (long long)K, (long long)M);
  if (n == 0 || R == 0) return MGX_OK;
  MGX_CHECK_ARG(a && b && c && offsets && workspace, "mgx_segment_mm: NULL pointer");
  MGX_CHECK_ARG(lda >= K && ldc >= M, "mgx_segment_mm: leading dimensions smaller than the operands");
  MGX_CHECK_ARG(n < (int64_t(1) << 30) / (lda > ldc ? lda : ldc), "mgx_segment_mm: n x max(lda, ldc) must stay below 2^30");
  hipStream_t s = (hipStream_t)stream;
  int64_t* table = (int64_t*)workspace;
  hipLaunchKernelGGL(seg_items_kernel, dim3(1), dim3(kBlock), 0, s, R, n, offsets, item_rows, table);
  MGX_CHECK_LAUNCH();
  const bool v4 = K % 4 == 0 && lda % 4 == 0 && (uintptr_t)a % 16 == 0;
  const int KC = (int)((K + 15) / 16);
  const unsigned blocks = (unsigned)((n + item_rows - 1) / item_rows + R);
  switch ((M + 63) / 64) {
    case 1: launch_segment_mm<4>(v4, blocks, s, R, (int)K, (int)M, KC, a, lda, a_rows, b, b_transposed, offsets, table, item_rows, c, ldc, c_rows); break;
    case 2: launch_segment_mm<8>(v4, blocks, s, R, (int)K, (int)M, KC, a, lda, a_rows, b, b_transposed, offsets, table, item_rows, c, ldc, c_rows); break;
    case 3: launch_segment_mm<12>(v4, blocks, s, R, (int)K, (int)M, KC, a, lda, a_rows, b, b_transposed, offsets, table, item_rows, c, ldc, c_rows); break;
    default: launch_segment_mm<16>(v4, blocks, s, R, (int)K, (int)M, KC, a, lda, a_rows, b, b_transposed, offsets, table, item_rows, c, ldc, c_rows); break;
  }
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}

extern "C" int32_t mgx_segment_mm_grad_b(int64_t n, int64_t R, int64_t K, int64_t M, const float* a, int64_t lda, const int64_t* a_rows,
                                         const float* dc, int64_t lddc, const int64_t* c_rows, const int64_t* offsets, float* db,
                                         void* workspace, void* stream) {
  using namespace mgx;
  MGX_ENTER();
  MGX_CHECK_ARG(n >= 0 && R >= 0 && K >= 1 && M >= 1, "mgx_segment_mm_grad_b: bad sizes (n %lld, R %lld, K %lld, M %lld)", (long long)n,
                (long long)R, (long long)K, (long long)M);
  MGX_CHECK_ARG(n > 0 || (!a_rows && !c_rows), "mgx_segment_mm_grad_b: a row list without rows");
  if (!seg_shape_ok(K, M))
    MGX_UNSUPPORTED("mgx_segment_mm_grad_b: needs M <= 256 and K x M padded to 16 x 64 within %d floats (got %lld x %lld)", kSegLdsFloats, (long long)K, (long long)M);
  if (n == 0 || R == 0) return MGX_OK;
  MGX_CHECK_ARG(a && dc && db && offsets && workspace, "mgx_segment_mm_grad_b: NULL pointer");
  MGX_CHECK_ARG(lda >= K && lddc >= M, "mgx_segment_mm_grad_b: leading dimensions smaller than the operands");
  MGX_CHECK_ARG(n < (int64_t(1) << 30) / (lda > lddc ? lda : lddc), "mgx_segment_mm_grad_b: n x max(lda, lddc) must stay below 2^30");
  hipStream_t s = (hipStream_t)stream;
  int64_t* table = (int64_t*)workspace;
  float* part = (float*)((char*)workspace + seg_pad((R + 1) * (int64_t)sizeof(int64_t), 256));
  const int64_t chunk = seg_xty_chunk(n, K, M), tile = K * M;
  hipLaunchKernelGGL(seg_items_kernel, dim3(1), dim3(kBlock), 0, s, R, n, offsets, chunk, table);
  MGX_CHECK_LAUNCH();
  const int64_t waves = (n + chunk - 1) / chunk + R;
  const dim3 grid((unsigned)((waves + kWavesPerBlock - 1) / kWavesPerBlock));
  const bool a_vec = lda % 4 == 0 && (uintptr_t)a % 16 == 0, d_vec = lddc % 4 == 0 && (uintptr_t)dc % 16 == 0;
  for (int64_t k0 = 0; k0 < K; k0 += 64)
    for (int64_t m0 = 0; m0 < M; m0 += 64) {
      const int Kw = (int)(K - k0 < 64 ? K - k0 : 64), Mw = (int)(M - m0 < 64 ? M - m0 : 64);
      int it, jt;
      bool av, dv, ok = false;
      seg_xty_form(Kw, a_vec, it, av);
      seg_xty_form(Mw, d_vec, jt, dv);
#define MGX_SEGX_A(IT_, AV_)                                                                                                             \
  if (!ok && it == IT_ && av == AV_)                                                                                                     \
    ok = launch_seg_xty_d<IT_, AV_>(jt, dv, grid, s, R, Kw, Mw, a + k0, lda, a_rows, dc + m0, lddc, c_rows, offsets, table, chunk,        \
                                    waves, part + k0 * M + m0, (int)M, tile);
      MGX_SEGX_A(1, false) MGX_SEGX_A(2, false) MGX_SEGX_A(4, false) MGX_SEGX_A(4, true)
#undef MGX_SEGX_A
      MGX_CHECK_ARG(ok, "mgx_segment_mm_grad_b: no kernel for this block");
      MGX_CHECK_LAUNCH();
    }
  const int64_t blocks_per_seg = (tile + 15) / 16;
  if (R * blocks_per_seg >= (int64_t(1) << 31)) MGX_UNSUPPORTED("mgx_segment_mm_grad_b: R x K x M / 16 must stay below 2^31");
  hipLaunchKernelGGL(segment_xty_finish_kernel, dim3((unsigned)(R * blocks_per_seg)), dim3(kBlock), 0, s, tile, blocks_per_seg, waves,
                     (const int64_t*)table, (const float*)part, db);
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}
