// xty.hip -- C[M, K] = A^T B for A [n, M], B [n, K] row-major with n in the millions and M, K <= 64 / 128 (one tile; up to
// 256 x 1024 as a grid of such tiles in one launch): the weight
// gradient dW = dY^T X of the dense layer that follows every aggregation (SAGEConv's fc_self / fc_neigh,
// main_dgl_product_sage.py:31-33,64).  rocBLAS / hipBLASLt run these tall-skinny reductions (K-dim = 2.45 M) at 0.5-1.0 ms;
// the operands only need to be streamed once (1.6 GB at 64 x 100), so the bound is HBM.
//
// fp32 MFMA 16x16x4: the "k" of the instruction runs over data rows.  Lane l supplies A[row0 + l/16][m0 + l%16] and
// B[row0 + l/16][k0 + l%16] -- both row-major, i.e. operands are loaded straight from global memory in the layout the
// instruction wants, no LDS staging and no transpose; a wave keeps the whole (M/16) x (K/16) grid of 16x16 accumulators
// (<= 4 x 8 x 4 = 128 VGPRs) and walks 16 rows per trip.  Every wave writes its partial tile; a second launch adds the
// partials in wave order (deterministic, no atomics).
//
// What is here:
//   xty_walk_dword<MT, KT>               the row walk with dword loads: loads, MFMAs and the partial-tile store; the body of
//     xty_partial_kernel<MT, KT>           one tile, any stride and alignment
//     xty_partial_grid_kernel              outputs wider than one tile, blockIdx.y = a 64 x 128 tile
//   xty_partial_v4_kernel                the walk with 16-byte loads for the operand(s) that allow it, column sums, a row list or a
//                                        position map; a __global__ body of its own
//   xty_masked_partial_kernel            the masked one-pass form (two waves per partition, a register ring)
//   xty_sum_partials, xty_sum_column     the ONE order in which partial tiles resp. partial column sums are added: every finish
//                                        kernel (plain, grid, column sums, masked) is index arithmetic around them
//   xty_col                              the real column behind (tile, index) of an operand cut into float4 groups + dword tiles
#include "common.h"

namespace mgx {

constexpr int kXtyWaves = 2048;  // most partial tiles (workspace size); fewer for shorter inputs, see xty_waves()

// One partial tile (<= 32 KB written, then read back) per wave: keep >= 256 rows per wave so that the tiles stay a small
// part of the traffic, between 256 waves (one per CU) and kXtyWaves; a multiple of 64 for the finish kernel's 16 slices.
static int xty_waves(int64_t n) {
  int64_t w = (n / 256 + 63) / 64 * 64;
  if (w < 256) w = 256;
  if (w > kXtyWaves) w = kXtyWaves;
  return (int)w;
}

// The walk with dword loads: any stride and alignment, no column sums, no list.  Wave gw = blockIdx.x's wave takes rows gw * 16 .. + 15,
// then on by all the waves of gridDim.x, and writes the gw-th partial tile [MT*16][KT*16] behind part.  Shared by the dword kernels
// and the grid of tiles.  (It is xty_partial_v4_kernel<0, MT, 0, KT, 0> with part_sum = b_rows = NULL -- the same loads, the same MFMAs
// in the same order, the same partial layout -- and exists beside it because that kernel keeps its register counts only as a
// __global__ body, see docs/LOG_xty_body.md.)
template <int MT, int KT>
__device__ __forceinline__ void xty_walk_dword(int64_t n, int M, int K, const float* __restrict__ A, int64_t lda,
                                               const float* __restrict__ B, int64_t ldb, float* __restrict__ part) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t gw = (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
  const int c = lane % 16, q = lane / 16;
  v4f acc[MT][KT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < KT; ++j) acc[i][j] = (v4f)(0.f);
  bool am[MT], bm[KT];
#pragma unroll
  for (int i = 0; i < MT; ++i) am[i] = i * 16 + c < M;
#pragma unroll
  for (int j = 0; j < KT; ++j) bm[j] = j * 16 + c < K;
  const int64_t stride = (int64_t)gridDim.x * kWavesPerBlock * 16;
  for (int64_t r0 = gw * 16; r0 < n; r0 += stride) {
    float a[4][MT], b[4][KT];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int64_t row = r0 + s * 4 + q;
      const bool ok = row < n;
#pragma unroll
      for (int i = 0; i < MT; ++i) a[s][i] = (ok && am[i]) ? A[row * lda + i * 16 + c] : 0.f;
#pragma unroll
      for (int j = 0; j < KT; ++j) b[s][j] = (ok && bm[j]) ? B[row * ldb + j * 16 + c] : 0.f;
    }
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < KT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s][i], b[s][j], acc[i][j], 0, 0, 0);
  }
  // D[4*(lane/16) + r][lane%16] of every tile -> partial [MT*16][KT*16]
  float* p = part + gw * (int64_t)(MT * 16) * (KT * 16);
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < KT; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) p[(i * 16 + 4 * q + r) * (KT * 16) + j * 16 + c] = acc[i][j][r];
}

template <int MT, int KT>
__global__ __launch_bounds__(kBlock) void xty_partial_kernel(int64_t n, int M, int K, const float* __restrict__ A, int64_t lda,
                                                             const float* __restrict__ B, int64_t ldb, float* __restrict__ part) {
  xty_walk_dword<MT, KT>(n, M, K, A, lda, B, ldb, part);
}

// The same walk with 16-BYTE operand loads.  The MFMA wants lane (c, q) to supply A[row + q][m = c] of a 16-column
// tile -- a dword per lane, i.e. 256 bytes per load instruction for 16 rows.  But which 16 columns form a "tile" is only a labelling of the
// OUTPUT: a lane that loads the float4 A[row][4c .. 4c+3] holds one column of FOUR tiles (tile t = component t, its 16 columns are
// 4c + t), so a 64-column operand arrives in one 16-byte load per lane and row, and the epilogue writes accumulator (tile t, index c) to
// column 4c + t.  Per operand: VG groups of 64 columns by float4 loads (VG * 4 tiles) + ST tiles of 16 columns by dword loads for the
// remainder (K = 72 = one group + one tile) or for an operand whose row stride is not a multiple of 4 floats (the 47-column output
// gradient).  Same accumulators, same partial layout, same finish kernel; fp32 MFMA, sums in another (fixed) order.
// ROWS (mgx_xty_rows): row r of B is B[b_rows[r]] -- the loss rows of an [N, 2K] layer buffer against their compact output gradient;
// int64[n], in range (not checked).  Same rows per wave, same MFMAs in the same order as ROWS = false on a gathered copy: same bits.
// A row beyond n reads no list entry.
// ROWS = kXtyAPos (mgx_xty_colsum_pos): the reduction runs over all n rows of B, but A exists on some of them only: row r pairs
// A[b_rows[r]] with B[r], and b_rows[r] < 0 stands for a ZERO row of A, which is neither read nor multiplied (B[r] is not read either).
// Adding the products of a zero row leaves an accumulator as it is, so the bits are those of ROWS = 0 on A scattered into a zero
// [n, M] matrix -- same rows per wave, same place of every row in its MFMA; a step of four rows without any row of A is skipped.
// (For FINITE B: an Inf or NaN in a row of B that meets a zero row of A gives NaN in that product and is not even read here.)
constexpr int kXtyBRows = 1, kXtyAPos = 2;

// the real column behind (tile j, index x) of an operand cut into vg float4 groups of 64 columns, then dword tiles of 16
__device__ __forceinline__ constexpr int xty_col(int vg, int j, int x) {
  return j < vg * 4 ? (j / 4) * 64 + 4 * x + j % 4 : vg * 64 + (j - vg * 4) * 16 + x;
}

template <int AVG, int AST, int BVG, int BST, int ROWS>
__global__ __launch_bounds__(kBlock) void xty_partial_v4_kernel(int64_t n, int M, int K, int mt16, int kt16, const float* __restrict__ A,
                                                                int64_t lda, const float* __restrict__ B, int64_t ldb,
                                                                float* __restrict__ part, float* __restrict__ part_sum,
                                                                const int64_t* __restrict__ b_rows) {
  // part_sum (may be NULL): the COLUMN SUMS of A as well -- the bias gradient that goes with this weight gradient -- as the product with
  // one more B column of ones: four MFMAs per 16 rows instead of another pass over A (mgx_column_sum: 0.08 - 0.11 ms at N = 2.45 M)
  constexpr int AT = AVG * 4 + AST, BT = BVG * 4 + BST;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t gw = (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
  const int c = lane % 16, q = lane / 16;
  v4f acc[AT][BT];
  v4f accs[AT > 0 ? AT : 1];
#pragma unroll
  for (int i = 0; i < AT; ++i) {
    accs[i] = (v4f)(0.f);
#pragma unroll
    for (int j = 0; j < BT; ++j) acc[i][j] = (v4f)(0.f);
  }
  const float one = c == 0 ? 1.f : 0.f;  // B column 0 of the extra tile is all ones, the other fifteen zero
  const int64_t stride = (int64_t)gridDim.x * kWavesPerBlock * 16;
  // kXtyAPos: the operand addresses hang on the map, so a tile's four entries are fetched a tile ahead (one round trip per tile, not two)
  int64_t ahead[4] = {-1, -1, -1, -1};
  auto pos_of = [&](int64_t r, int s) { return r + s * 4 + q < n ? b_rows[r + s * 4 + q] : (int64_t)-1; };
  if (ROWS == kXtyAPos) {
#pragma unroll
    for (int s = 0; s < 4; ++s) ahead[s] = pos_of(gw * 16, s);
  }
  for (int64_t r0 = gw * 16; r0 < n; r0 += stride) {
    float a[4][AT > 0 ? AT : 1], b[4][BT > 0 ? BT : 1];
    bool live[4] = {true, true, true, true};  // kXtyAPos, wave-uniform: some row of this step has a row of A
    int64_t here[4] = {0, 0, 0, 0};
    if (ROWS == kXtyAPos) {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        here[s] = ahead[s];
        ahead[s] = pos_of(r0 + stride, s);
      }
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int64_t row = r0 + s * 4 + q;
      const int64_t listed = ROWS == kXtyAPos ? here[s] : ROWS ? (row < n ? b_rows[row] : 0) : row;
      const bool ok = row < n && (ROWS != kXtyAPos || listed >= 0);
      const int64_t brow = ROWS == kXtyBRows ? listed : row, arow = ROWS == kXtyAPos ? listed : row;
      if (ROWS == kXtyAPos) live[s] = __ballot(ok) != 0;
#pragma unroll
      for (int g = 0; g < AVG; ++g) {
        const v4f v = (ok && g * 64 + 4 * c + 3 < M) ? *reinterpret_cast<const v4f*>(A + arow * lda + g * 64 + 4 * c) : (v4f)(0.f);
        a[s][g * 4 + 0] = v.x; a[s][g * 4 + 1] = v.y; a[s][g * 4 + 2] = v.z; a[s][g * 4 + 3] = v.w;
      }
#pragma unroll
      for (int i = 0; i < AST; ++i) a[s][AVG * 4 + i] = (ok && AVG * 64 + i * 16 + c < M) ? A[arow * lda + AVG * 64 + i * 16 + c] : 0.f;
#pragma unroll
      for (int g = 0; g < BVG; ++g) {
        const v4f v = (ok && g * 64 + 4 * c + 3 < K) ? *reinterpret_cast<const v4f*>(B + brow * ldb + g * 64 + 4 * c) : (v4f)(0.f);
        b[s][g * 4 + 0] = v.x; b[s][g * 4 + 1] = v.y; b[s][g * 4 + 2] = v.z; b[s][g * 4 + 3] = v.w;
      }
#pragma unroll
      for (int j = 0; j < BST; ++j) b[s][BVG * 4 + j] = (ok && BVG * 64 + j * 16 + c < K) ? B[brow * ldb + BVG * 64 + j * 16 + c] : 0.f;
    }
#pragma unroll
    for (int s = 0; s < 4; ++s)
      if (ROWS != kXtyAPos || live[s]) {
#pragma unroll
        for (int i = 0; i < AT; ++i)
#pragma unroll
          for (int j = 0; j < BT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s][i], b[s][j], acc[i][j], 0, 0, 0);
      }
    if (part_sum) {
#pragma unroll
      for (int s = 0; s < 4; ++s)
        if (ROWS != kXtyAPos || live[s]) {
#pragma unroll
          for (int i = 0; i < AT; ++i) accs[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s][i], (r0 + s * 4 + q < n) ? one : 0.f, accs[i], 0, 0, 0);
        }
    }
  }
  if (part_sum && c == 0) {  // lane (0, q) holds the sums of the real columns behind (tile i, index 4 q + r): one [mt16] vector per wave
#pragma unroll
    for (int i = 0; i < AT; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = xty_col(AVG, i, 4 * q + r);
        if (m < mt16) part_sum[gw * (int64_t)mt16 + m] = accs[i][r];
      }
  }
  // accumulator element r of tile (i, j) in lane (c, q) is C[m][k] with m / k the REAL columns behind (tile i, index 4q + r) / (tile j, index c)
  float* p = part + gw * (int64_t)mt16 * kt16;
#pragma unroll
  for (int i = 0; i < AT; ++i)
#pragma unroll
    for (int j = 0; j < BT; ++j) {
      const int k = xty_col(BVG, j, c);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = xty_col(AVG, i, 4 * q + r);
        if (m < mt16 && k < kt16) p[m * kt16 + k] = acc[i][j][r];
      }
    }
}

// Outputs wider than one 64 x 128 tile (arxiv's 256 x 512, GAT's 128 x 602, the stacked 64 x 200 of the one-GEMM SAGE layer):
// ONE launch, blockIdx.y = output tile.  The waves of different tiles walk the same data rows at the same time, so an operand
// row is read from HBM once and from L2 by the other tiles, and 4 waves per SIMD are resident -- against one launch per tile,
// each streaming both operands again with less than one wave per SIMD.  About kXtyGridTotal waves in all (4 per SIMD at 128
// VGPRs) shared evenly by the tiles; partials per (tile, wave).
constexpr int kXtyGridTotal = 4096;
constexpr int kXtyTileM = 64, kXtyTileK = 128;

__global__ __launch_bounds__(kBlock) void xty_partial_grid_kernel(int64_t n, int M, int K, int tiles_k, const float* __restrict__ A,
                                                                  int64_t lda, const float* __restrict__ B, int64_t ldb,
                                                                  float* __restrict__ part) {
  const int tile = blockIdx.y;
  const int m0 = (tile / tiles_k) * kXtyTileM, k0 = (tile % tiles_k) * kXtyTileK;
  const int Mt = M - m0 < kXtyTileM ? M - m0 : kXtyTileM, Kt = K - k0 < kXtyTileK ? K - k0 : kXtyTileK;
  const int64_t wpt = (int64_t)gridDim.x * kWavesPerBlock;  // waves per tile
  xty_walk_dword<kXtyTileM / 16, kXtyTileK / 16>(n, Mt, Kt, A + m0, lda, B + k0, ldb, part + (int64_t)tile * wpt * (kXtyTileM * kXtyTileK));
}

template <int AVG, int AST>
static bool launch_xty_v4_b(int bvg, int bst, int waves, int64_t n, int M, int K, int mt16, int kt16, const float* A, int64_t lda,
                            const float* B, int64_t ldb, float* part, float* part_sum, hipStream_t s, const int64_t* b_rows, int mode) {
#define MGX_XTY4(G, T, ROWS) if (bvg == G && bst == T) { hipLaunchKernelGGL((xty_partial_v4_kernel<AVG, AST, G, T, ROWS>), dim3(waves / kWavesPerBlock), dim3(kBlock), 0, s, n, M, K, mt16, kt16, A, lda, B, ldb, part, part_sum, b_rows); return true; }
  if (b_rows) {  // the list forms that are built: a dword-loaded A (the 47-column output gradient) against 128 or 64 float4 columns
    if constexpr (AVG == 0 && AST == 3) {
      if (mode == kXtyAPos) { MGX_XTY4(2, 0, kXtyAPos) MGX_XTY4(1, 0, kXtyAPos) }
      else { MGX_XTY4(2, 0, kXtyBRows) MGX_XTY4(1, 0, kXtyBRows) }
    }
    return false;
  }
  MGX_XTY4(2, 0, 0) MGX_XTY4(1, 0, 0) MGX_XTY4(1, 1, 0) MGX_XTY4(1, 2, 0) MGX_XTY4(1, 3, 0) MGX_XTY4(1, 4, 0)
#undef MGX_XTY4
  return false;
}

// 16-byte loads for the operand(s) that allow it; false = use the dword kernels above
static bool launch_xty_v4(int mt, int kt, int waves, int64_t n, int M, int K, const float* A, int64_t lda, const float* B, int64_t ldb,
                          float* part, float* part_sum, hipStream_t s, const int64_t* b_rows, int mode) {
  const bool bvec = ldb % 4 == 0 && (uintptr_t)B % 16 == 0 && K % 4 == 0 && K >= 64;
  if (!bvec) return false;
  const int bvg = K >= 128 ? 2 : 1, bst = (K - bvg * 64 + 15) / 16;
  const bool avec = lda % 4 == 0 && (uintptr_t)A % 16 == 0 && M == 64 && !b_rows;
  const int mt16 = mt * 16, kt16 = kt * 16;
  if (avec) return launch_xty_v4_b<1, 0>(bvg, bst, waves, n, M, K, mt16, kt16, A, lda, B, ldb, part, part_sum, s, b_rows, mode);
  switch (mt) {
    case 1: return launch_xty_v4_b<0, 1>(bvg, bst, waves, n, M, K, mt16, kt16, A, lda, B, ldb, part, part_sum, s, b_rows, mode);
    case 2: return launch_xty_v4_b<0, 2>(bvg, bst, waves, n, M, K, mt16, kt16, A, lda, B, ldb, part, part_sum, s, b_rows, mode);
    case 3: return launch_xty_v4_b<0, 3>(bvg, bst, waves, n, M, K, mt16, kt16, A, lda, B, ldb, part, part_sum, s, b_rows, mode);
    default: return launch_xty_v4_b<0, 4>(bvg, bst, waves, n, M, K, mt16, kt16, A, lda, B, ldb, part, part_sum, s, b_rows, mode);
  }
}

template <int MT>
static bool launch_xty_kt(int kt, int waves, int64_t n, int M, int K, const float* A, int64_t lda, const float* B, int64_t ldb,
                          float* part, hipStream_t s) {
  switch (kt) {
#define MGX_XTY(J) case J: hipLaunchKernelGGL((xty_partial_kernel<MT, J>), dim3(waves / kWavesPerBlock), dim3(kBlock), 0, s, n, M, K, A, lda, B, ldb, part); return true;
    MGX_XTY(1) MGX_XTY(2) MGX_XTY(3) MGX_XTY(4) MGX_XTY(5) MGX_XTY(6) MGX_XTY(7) MGX_XTY(8)
#undef MGX_XTY
    default: return false;
  }
}

// One output element's sum over the partial list, by the 16 threads that share threadIdx.x % 16: thread (e, sl) adds slice sl of the
// list in four running sums, the slices are added in slice order.  at(): the element in partial 0, asked for a live element only (an
// address worked out before the test is carried through the sum: four more VGPRs in xty_finish_kernel); the total comes back in the
// sl == 0 threads of a live element.  Every thread of the workgroup calls this (one __syncthreads()).
template <class At>
__device__ __forceinline__ float xty_sum_partials(At at, int64_t tile, int waves, bool live, float (*red)[17]) {
  const int e = threadIdx.x % 16, sl = threadIdx.x / 16;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (live) {
    const float* __restrict__ p = at();
    const int per = waves / 16;
    for (int w = sl * per; w < (sl + 1) * per; w += 4) {
      s0 += p[w * tile];
      s1 += p[(w + 1) * tile];
      s2 += p[(w + 2) * tile];
      s3 += p[(w + 3) * tile];
    }
  }
  red[sl][e] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  float s = 0.f;
  if (sl == 0 && live)
    for (int i = 0; i < 16; ++i) s += red[i][e];
  return s;
}

// One column's sum over the [waves][ld] partial vectors by one wave: lanes stride the list, then a butterfly.  p: the column in vector 0.
__device__ __forceinline__ float xty_sum_column(const float* __restrict__ p, int ld, int waves) {
  float s = 0.f;
  for (int w = threadIdx.x % kWave; w < waves; w += kWave) s += p[(int64_t)w * ld];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, kWave);
  return s;
}

// 16 output elements per workgroup, over M * K
__global__ __launch_bounds__(kBlock) void xty_finish_kernel(int M, int K, int ldm /* KT*16 */, int tile /* MT*16*KT*16 */, int waves,
                                                            const float* __restrict__ part, float* __restrict__ out, int64_t ldc) {
  __shared__ float red[16][17];
  const int idx = blockIdx.x * 16 + threadIdx.x % 16;
  const bool live = idx < M * K;
  const float s = xty_sum_partials([&] { return part + (int64_t)(idx / K) * ldm + idx % K; }, tile, waves, live, red);
  if (threadIdx.x < 16 && live) out[(int64_t)(idx / K) * ldc + idx % K] = s;
}

// blockIdx.y = tile; blockIdx.x over the 64 x 128 elements of a tile, 16 per workgroup
__global__ __launch_bounds__(kBlock) void xty_finish_grid_kernel(int M, int K, int tiles_k, int wpt, const float* __restrict__ part,
                                                                 float* __restrict__ out, int64_t ldc) {
  __shared__ float red[16][17];
  constexpr int tsz = kXtyTileM * kXtyTileK;
  const int tile = blockIdx.y;
  const int m0 = (tile / tiles_k) * kXtyTileM, k0 = (tile % tiles_k) * kXtyTileK;
  const int idx = blockIdx.x * 16 + threadIdx.x % 16;
  const int m = idx / kXtyTileK, k = idx % kXtyTileK;
  const bool live = m0 + m < M && k0 + k < K;
  const float s = xty_sum_partials([&] { return part + (int64_t)tile * wpt * tsz + idx; }, tsz, wpt, live, red);
  if (threadIdx.x < 16 && live) out[(int64_t)(m0 + m) * ldc + k0 + k] = s;
}

// column sums: the [waves][mt16] partial vectors, one wave per output column
__global__ __launch_bounds__(kBlock) void xty_colsum_finish_kernel(int M, int mt16, int waves, const float* __restrict__ part_sum,
                                                                   float* __restrict__ colsum) {
  const int m = blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
  if (m >= M) return;
  const float s = xty_sum_column(part_sum + m, mt16, waves);
  if (threadIdx.x % kWave == 0) colsum[m] = s;
}

// mgx_xty_colsum_masked: relu_dropout_bwd_kernel + xty_partial_v4_kernel<1, 0, ...> per 128-column block of B + the column sums in ONE
// pass.  dZ[r][4c + t] = bit t of mask[r * 16 + c] ? dy[r][4c + t] * scale : 0.f is formed in registers from the float2 a lane loads anyway
// and never stored.  The bits are those of the composition by construction: partition gw of xty_waves(n) walks the rows the composition's
// wave gw walks, a 16 x 16 accumulator (A component i, B tile j) sees the same MFMAs in the same order (steps in row order, s = 0 .. 3
// inside a step), B's tiles are cut as the composition's launches cut them (per block of 128 columns: float4 groups of 64, then dword
// tiles of 16), and the partials are added by the finish kernels' own code.  Which physical wave holds which accumulator is free:
// TWO waves per partition split A's four components (h = 0: x, y; h = 1: z, w), so both carry 2 x BT + 2 tiles -- the same MFMA count --
// and run the same code; each reads all of B, the later one from L1 / L2 (same workgroup, same rows at the same time).
// Operands live in a ring of the step's four 4-row slices: slice s of the NEXT step is loaded right after the MFMAs of slice s, so a load has
// three slices of MFMAs (>= 1 us) to land while the registers of one step, not two, are held.
// VG0 / ST0: float4 groups / dword tiles of block 0 (columns 0 .. 127), VG1 / ST1: of block 1 (columns 128 ..).
template <int VG0, int ST0, int VG1, int ST1>
__global__ __launch_bounds__(kBlock) void xty_masked_partial_kernel(int64_t n, int K, int waves, const float* __restrict__ dy, int64_t lddy,
                                                                    const uint8_t* __restrict__ mask, float scale,
                                                                    const float* __restrict__ B, int64_t ldb, float* __restrict__ part,
                                                                    float* __restrict__ part_sum) {
  constexpr int NG = VG0 + VG1, NS = ST0 + ST1, BT = NG * 4 + NS;
  constexpr int kDword0 = VG0 * 64, kDword1 = 128 + VG1 * 64;  // first dword-tile column of either block
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int h = wave & 1;                                                         // which two components of A's float4
  const int64_t gw = (int64_t)blockIdx.x * (kWavesPerBlock / 2) + (wave >> 1);  // the partition: the composition's wave number
  const int c = lane % 16, q = lane / 16;
  v4f acc[2][BT];
  v4f accs[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    accs[i] = (v4f)(0.f);
#pragma unroll
    for (int j = 0; j < BT; ++j) acc[i][j] = (v4f)(0.f);
  }
  const float one = c == 0 ? 1.f : 0.f;
  const int64_t stride = (int64_t)waves * 16;
  v2f ra[4];                         // the ring: dy[row][4c + 2h .. + 1], its mask byte, B's float4 groups and dword tiles, per slice
  uint32_t rm[4];
  v4f rg[4][NG > 0 ? NG : 1];
  float rs[4][NS > 0 ? NS : 1];
  // Every load is issued unconditionally from a clamped address, and what a row >= n (the tail of the last step, the step after a wave's
  // last) or a column >= K brought is replaced by zero where the slice is CONSUMED: no branch and no use of the loaded registers sits
  // between a load and the MFMAs it feeds three slices later, so the wait before them leaves the younger loads in flight.
  auto fetch = [&](int64_t r0, int s) {
    const int64_t row = r0 + s * 4 + q;
    const int64_t rc = row < n ? row : n - 1;
    ra[s] = *reinterpret_cast<const v2f*>(dy + rc * lddy + 4 * c + 2 * h);
    rm[s] = mask[rc * 16 + c];
    const float* b = B + rc * ldb;
#pragma unroll
    for (int g = 0; g < NG; ++g) rg[s][g] = *reinterpret_cast<const v4f*>(b + (g < VG0 ? g * 64 : 128 + (g - VG0) * 64) + 4 * c);
#pragma unroll
    for (int t = 0; t < NS; ++t) {
      const int col = (t < ST0 ? kDword0 + t * 16 : kDword1 + (t - ST0) * 16) + c;
      rs[s][t] = b[col < K ? col : K - 1];
    }
    // keeps the loads HERE: without a barrier the compiler turns "loaded in step i, carried round the loop, used in step i + 1" into a
    // load at the use (a phi of loads becomes the load of a phi), and the ring into load-wait-multiply
    asm volatile("" ::: "memory");
  };
  if (gw * 16 < n) {
#pragma unroll
    for (int s = 0; s < 4; ++s) fetch(gw * 16, s);
  }
  for (int64_t r0 = gw * 16; r0 < n; r0 += stride) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const bool ok = r0 + s * 4 + q < n;
      const uint32_t m = ok ? rm[s] >> (2 * h) : 0u;
      float a[2];
      a[0] = (m & 1) ? ra[s].x * scale : 0.f;  // a select, as relu_dropout_bwd_kernel writes it: nothing behind a cleared bit is multiplied
      a[1] = (m & 2) ? ra[s].y * scale : 0.f;
      float b[BT];
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        const v4f v = ok ? rg[s][g] : (v4f)(0.f);
        b[g * 4 + 0] = v.x; b[g * 4 + 1] = v.y; b[g * 4 + 2] = v.z; b[g * 4 + 3] = v.w;
      }
#pragma unroll
      for (int t = 0; t < NS; ++t) {
        const int col = (t < ST0 ? kDword0 + t * 16 : kDword1 + (t - ST0) * 16) + c;
        b[NG * 4 + t] = (ok & (col < K)) ? rs[s][t] : 0.f;
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < BT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
      const float ones = ok ? one : 0.f;
#pragma unroll
      for (int i = 0; i < 2; ++i) accs[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], ones, accs[i], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);  // the slice's MFMAs, THEN its refill: the scheduler would gather all four refills at the loop's end
      fetch(r0 + stride, s);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  // accumulator element r of (component i, tile j) in lane (c, q) is C[m][k], m = 4 (4q + r) + 2h + i; partial [64][K] + sums [64] per partition
  float* p = part + gw * (int64_t)64 * K;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int mrow = 4 * (4 * q + r) + 2 * h + i;
      if (c == 0) part_sum[gw * 64 + mrow] = accs[i][r];
#pragma unroll
      for (int j = 0; j < BT; ++j) {
        int k;
        if (j < NG * 4) {
          const int g = j / 4;
          k = (g < VG0 ? g * 64 : 128 + (g - VG0) * 64) + 4 * c + (j % 4);
        } else {
          const int t = j - NG * 4;
          k = (t < ST0 ? kDword0 + t * 16 : kDword1 + (t - ST0) * 16) + c;
        }
        if (k < K) p[mrow * K + k] = acc[i][j][r];
      }
    }
}

// One finish launch for out [64, K] and colsum [64]: the element workgroups are xty_finish_kernel's, the last 16 workgroups
// xty_colsum_finish_kernel's (one wave per column).
__global__ __launch_bounds__(kBlock) void xty_masked_finish_kernel(int K, int waves, const float* __restrict__ part,
                                                                   const float* __restrict__ part_sum, float* __restrict__ out, int64_t ldc,
                                                                   float* __restrict__ colsum) {
  __shared__ float red[16][17];
  const int elem_blocks = 64 * K / 16;
  if ((int)blockIdx.x >= elem_blocks) {
    const int m = ((int)blockIdx.x - elem_blocks) * kWavesPerBlock + threadIdx.x / kWave;
    const float s = xty_sum_column(part_sum + m, 64, waves);
    if (threadIdx.x % kWave == 0) colsum[m] = s;
    return;
  }
  const int idx = blockIdx.x * 16 + threadIdx.x % 16;  // over 64 * K, a multiple of 16
  const float s = xty_sum_partials([&] { return part + idx; }, 64 * K, waves, true, red);
  if (threadIdx.x < 16) out[(int64_t)(idx / K) * ldc + idx % K] = s;
}

}  // namespace mgx

extern "C" int64_t mgx_xty_workspace(int64_t M, int64_t K) {
  const int64_t mt = (M + 15) / 16, kt = (K + 15) / 16;
  if (M < 1 || K < 1) return -1;
  if (mt > 4 || kt > 8) {  // several 64 x 128 tiles in one launch
    if (M > 256 || K > 1024) return -1;
    return (int64_t)mgx::kXtyGridTotal * mgx::kXtyTileM * mgx::kXtyTileK * (int64_t)sizeof(float);  // tiles x waves-per-tile <= this many
  }
  return (int64_t)mgx::kXtyWaves * (mt * 16 * kt * 16 + mt * 16) * (int64_t)sizeof(float);  // partial tiles + partial column sums
}

static int32_t xty_impl(int64_t n, int64_t M, int64_t K, const float* a, int64_t lda, const float* b, int64_t ldb, float* out, int64_t ldc,
                        float* colsum, void* workspace, void* stream, const int64_t* b_rows = nullptr, int mode = 0) {
  using namespace mgx;
  MGX_ENTER();
  MGX_CHECK_ARG(n >= 0 && M >= 1 && K >= 1, "mgx_xty: bad sizes");
  const int mt = (int)((M + 15) / 16), kt = (int)((K + 15) / 16);
  if (M > 256 || K > 1024) MGX_UNSUPPORTED("mgx_xty: needs M <= 256 and K <= 1024 (got %lld x %lld)", (long long)M, (long long)K);
  MGX_CHECK_ARG(out != nullptr, "mgx_xty: out is NULL");
  MGX_CHECK_ARG(lda >= M && ldb >= K && ldc >= K, "mgx_xty: leading dimensions smaller than the tile (lda %lld, ldb %lld, ldc %lld)",
                (long long)lda, (long long)ldb, (long long)ldc);
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) {
    MGX_CHECK_HIP(hipMemset2DAsync(out, (size_t)ldc * sizeof(float), 0, (size_t)K * sizeof(float), (size_t)M, s));
    if (colsum) MGX_CHECK_HIP(hipMemsetAsync(colsum, 0, (size_t)M * sizeof(float), s));
    return MGX_OK;
  }
  MGX_CHECK_ARG(a && b && workspace, "mgx_xty: NULL pointer");
  float* part = (float*)workspace;
  if (b_rows && (mt > 4 || kt > 8)) MGX_UNSUPPORTED("mgx_xty_rows: one 64 x 128 tile only");
  if (mt > 4 || kt > 8) {
    if (colsum) MGX_UNSUPPORTED("mgx_xty_colsum: one 64 x 128 tile only");
    const int tiles_m = (int)((M + kXtyTileM - 1) / kXtyTileM), tiles_k = (int)((K + kXtyTileK - 1) / kXtyTileK);
    // waves per tile: an even share of kXtyGridTotal, a multiple of 64 (the finish kernel's 16 slices x 4), at least 64 and at
    // most what gives every wave 256 rows
    int wpt = kXtyGridTotal / (tiles_m * tiles_k) / 64 * 64;
    const int64_t by_rows = n / 128 / 64 * 64;  // >= 128 rows per wave: short inputs (a batch of small graphs) take few waves
    if (wpt > by_rows) wpt = (int)by_rows;
    if (wpt < 64) wpt = 64;
    hipLaunchKernelGGL(xty_partial_grid_kernel, dim3(wpt / kWavesPerBlock, tiles_m * tiles_k), dim3(kBlock), 0, s, n, (int)M,
                       (int)K, tiles_k, a, lda, b, ldb, part);
    MGX_CHECK_LAUNCH();
    hipLaunchKernelGGL(xty_finish_grid_kernel, dim3(kXtyTileM * kXtyTileK / 16, tiles_m * tiles_k), dim3(kBlock), 0, s, (int)M, (int)K,
                       tiles_k, wpt, (const float*)part, out, ldc);
    MGX_CHECK_LAUNCH();
    return MGX_OK;
  }
  const int waves = xty_waves(n);
  float* part_sum = colsum ? part + (int64_t)kXtyWaves * mt * 16 * kt * 16 : nullptr;
  bool ok = launch_xty_v4(mt, kt, waves, n, (int)M, (int)K, a, lda, b, ldb, part, part_sum, s, b_rows, mode);
  if (!ok && b_rows) MGX_UNSUPPORTED("mgx_xty_rows: no row-list kernel for %lld x %lld", (long long)M, (long long)K);
  if (!ok && colsum) MGX_UNSUPPORTED("mgx_xty_colsum: needs the 16-byte-load form (B: K %% 4 == 0, K >= 64, aligned)");
  if (!ok) switch (mt) {
    case 1: ok = launch_xty_kt<1>(kt, waves, n, (int)M, (int)K, a, lda, b, ldb, part, s); break;
    case 2: ok = launch_xty_kt<2>(kt, waves, n, (int)M, (int)K, a, lda, b, ldb, part, s); break;
    case 3: ok = launch_xty_kt<3>(kt, waves, n, (int)M, (int)K, a, lda, b, ldb, part, s); break;
    default: ok = launch_xty_kt<4>(kt, waves, n, (int)M, (int)K, a, lda, b, ldb, part, s); break;
  }
  MGX_CHECK_ARG(ok, "mgx_xty: no kernel for this tile shape");
  MGX_CHECK_LAUNCH();
  hipLaunchKernelGGL(xty_finish_kernel, dim3((unsigned)((M * K + 15) / 16)), dim3(kBlock), 0, s, (int)M, (int)K, kt * 16,
                     mt * 16 * kt * 16, waves, (const float*)part, out, ldc);
  MGX_CHECK_LAUNCH();
  if (colsum) {
    hipLaunchKernelGGL(xty_colsum_finish_kernel, dim3((unsigned)((M + kWavesPerBlock - 1) / kWavesPerBlock)), dim3(kBlock), 0, s, (int)M,
                       mt * 16, waves, (const float*)part_sum, colsum);
    MGX_CHECK_LAUNCH();
  }
  return MGX_OK;
}

// b_rows with mode kXtyBRows: the row list of b; with kXtyAPos: the position map of a.  A NULL list is the plain form.
extern "C" int32_t mgx_xty(int64_t n, int64_t M, int64_t K, const float* a, int64_t lda, const float* b, int64_t ldb, float* out,
                           int64_t ldc, void* workspace, void* stream) {
  return xty_impl(n, M, K, a, lda, b, ldb, out, ldc, nullptr, workspace, stream);
}

extern "C" int32_t mgx_xty_colsum(int64_t n, int64_t M, int64_t K, const float* a, int64_t lda, const float* b, int64_t ldb, float* out,
                                  int64_t ldc, float* colsum, void* workspace, void* stream) {
  return xty_impl(n, M, K, a, lda, b, ldb, out, ldc, colsum, workspace, stream);
}

extern "C" int32_t mgx_xty_rows(int64_t n, int64_t M, int64_t K, const float* a, int64_t lda, const float* b, int64_t ldb,
                                const int64_t* b_rows, float* out, int64_t ldc, void* workspace, void* stream) {
  return xty_impl(n, M, K, a, lda, b, ldb, out, ldc, nullptr, workspace, stream, b_rows, mgx::kXtyBRows);
}

extern "C" int32_t mgx_xty_colsum_rows(int64_t n, int64_t M, int64_t K, const float* a, int64_t lda, const float* b, int64_t ldb,
                                       const int64_t* b_rows, float* out, int64_t ldc, float* colsum, void* workspace, void* stream) {
  return xty_impl(n, M, K, a, lda, b, ldb, out, ldc, colsum, workspace, stream, b_rows, mgx::kXtyBRows);
}

extern "C" int32_t mgx_xty_colsum_pos(int64_t n, int64_t M, int64_t K, const float* a, int64_t lda, const int64_t* a_pos, const float* b,
                                      int64_t ldb, float* out, int64_t ldc, float* colsum, void* workspace, void* stream) {
  return xty_impl(n, M, K, a, lda, b, ldb, out, ldc, colsum, workspace, stream, a_pos, mgx::kXtyAPos);
}

extern "C" int64_t mgx_xty_masked_workspace(int64_t K) {
  if (K < 64 || K > 256 || K % 4) return -1;
  return (int64_t)mgx::kXtyWaves * (64 * K + 64) * (int64_t)sizeof(float);  // a [64, K] partial tile + 64 column sums per partition
}

extern "C" int32_t mgx_xty_colsum_masked(int64_t n, int64_t K, const float* dy, int64_t lddy, const uint8_t* mask, float p, const float* b,
                                         int64_t ldb, float* out, int64_t ldc, float* colsum, void* workspace, void* stream) {
  using namespace mgx;
  MGX_ENTER();
  MGX_CHECK_ARG(n >= 0 && K >= 1, "mgx_xty_colsum_masked: bad sizes");
  MGX_CHECK_ARG(p >= 0.f && p < 1.f, "mgx_xty_colsum_masked: p must be in [0, 1)");
  if (K < 64 || K > 256 || K % 4) MGX_UNSUPPORTED("mgx_xty_colsum_masked: needs 64 <= K <= 256, K %% 4 == 0 (got %lld)", (long long)K);
  MGX_CHECK_ARG(out && colsum, "mgx_xty_colsum_masked: out or colsum is NULL");
  MGX_CHECK_ARG(lddy >= 64 && ldb >= K && ldc >= K, "mgx_xty_colsum_masked: leading dimensions smaller than the tile (lddy %lld, ldb %lld, ldc %lld)",
                (long long)lddy, (long long)ldb, (long long)ldc);
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) {
    MGX_CHECK_HIP(hipMemset2DAsync(out, (size_t)ldc * sizeof(float), 0, (size_t)K * sizeof(float), 64, s));
    MGX_CHECK_HIP(hipMemsetAsync(colsum, 0, 64 * sizeof(float), s));
    return MGX_OK;
  }
  MGX_CHECK_ARG(dy && mask && b && workspace, "mgx_xty_colsum_masked: NULL pointer");
  if (lddy % 4 || (uintptr_t)dy % 16 || ldb % 4 || (uintptr_t)b % 16)
    MGX_UNSUPPORTED("mgx_xty_colsum_masked: needs the 16-byte-load form of both operands (row strides %% 4 == 0, 16-byte aligned)");
  // the tiles of either 128-column block as mgx_xty_colsum cuts them (launch_xty_v4): float4 groups of 64 columns, dword tiles of 16 for the rest
  const int64_t k0 = K < 128 ? K : 128, k1 = K - k0;
  if (k1 > 0 && k1 < 64) MGX_UNSUPPORTED("mgx_xty_colsum_masked: a second block of %lld columns has no 16-byte-load form", (long long)k1);
  const int vg0 = k0 >= 128 ? 2 : 1, st0 = (int)((k0 - vg0 * 64 + 15) / 16);
  const int vg1 = k1 >= 128 ? 2 : k1 >= 64 ? 1 : 0, st1 = (int)((k1 - vg1 * 64 + 15) / 16);
  const int waves = xty_waves(n);
  float* part = (float*)workspace;
  float* part_sum = part + (int64_t)kXtyWaves * 64 * K;
  const float scale = 1.f / (1.f - p);
  bool ok = false;
#define MGX_XTYM(A, B, C, D)                                                                                                             \
  if (vg0 == A && st0 == B && vg1 == C && st1 == D) {                                                                                    \
    hipLaunchKernelGGL((xty_masked_partial_kernel<A, B, C, D>), dim3(waves / (kWavesPerBlock / 2)), dim3(kBlock), 0, s, n, (int)K, waves, \
                       dy, lddy, mask, scale, b, ldb, part, part_sum);                                                                   \
    ok = true;                                                                                                                           \
  }
  MGX_XTYM(1, 0, 0, 0) MGX_XTYM(1, 1, 0, 0) MGX_XTYM(2, 0, 0, 0) MGX_XTYM(2, 0, 1, 1) MGX_XTYM(2, 0, 2, 0)
#undef MGX_XTYM
  if (!ok) MGX_UNSUPPORTED("mgx_xty_colsum_masked: no kernel for K = %lld (built: 64, 68 .. 80, 128, 196 .. 208, 256)", (long long)K);
  MGX_CHECK_LAUNCH();
  hipLaunchKernelGGL(xty_masked_finish_kernel, dim3((unsigned)(64 * K / 16 + 64 / kWavesPerBlock)), dim3(kBlock), 0, s, (int)K, waves,
                     (const float*)part, (const float*)part_sum, out, ldc, colsum);
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}
