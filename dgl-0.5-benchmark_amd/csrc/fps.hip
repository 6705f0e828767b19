// fps.hip -- farthest point sampling inside the contiguous row segments of a batch of point clouds (gfx950 / MI355X):
// dgl.geometry.farthest_point_sampler, the centre selection of a PointNet++ set-abstraction level.  The whole serial chain of a cloud
// runs inside ONE workgroup of ONE launch: in torch every selected point is a gather, a distance, a minimum and an argmax launch.
//
//   per segment (len rows from row beg):  mind[j] = +inf;  cur = start ? start[s] : 0 (outside [0, len): 0)
//   for t = 0 .. min(m, len) - 1:         index[s, t] = beg + cur;  dist[s, t] = mind[cur]  (rank 0: +inf);  cur is selected for good
//                                         every unselected j:  d = sum_c (x[cur,c] - x[j,c])^2  (fp32, c ascending, one fma per term, the
//                                         direct form of knn.hip);  if (d < mind[j]) mind[j] = d  -- a NaN d changes nothing
//                                         cur = the unselected row of greatest mind, the lowest row on ties
//   ranks t >= len:                       index -1, dist 0.  Every element is written: no memset.
// So the selected rows are distinct; duplicates are taken in row order once everything else is at distance 0; a row with a NaN
// coordinate keeps mind = +inf, is selected right after the start (the lowest such row first) and, as cur, changes no mind.
//
// One workgroup per segment.  The segment's coordinates are staged into LDS once, point-major with an ODD row stride (D | 1): thread
// tid owns points tid, tid + T, ... (P of them, mind in registers), so the lanes of a wave read one column of 64 consecutive points at
// conflict-free addresses, and the current point's coordinates come from a workgroup-uniform address (a broadcast).  With D == 3 the
// thread's own coordinates stay in registers as well and the step reads LDS for the current point only.
// mind = -1 marks a row that is no candidate (selected, or past the segment's end): no distance is below it.  The arg-max is one
// 64-bit key per thread, built once from the greatest mind of its points: the bits of mind (non-negative, so they order as integers)
// in the high word, the complemented row in the low word (the lowest row wins a tie), 0 when no candidate is left.  Keys are reduced
// inside the wave with DPP row moves and four lane reads, one key per wave goes through a double-buffered LDS slot, and every wave
// reduces the slots again: ONE barrier per selected point (slot b is rewritten two steps later, after the barrier of the step
// between).  The workgroup shapes below were measured: docs/LOG_fps.md.
// Nothing is read on the host; the launch depends on num_segments, D and max_len only: capture-safe.  No atomics.
#include "common.h"

namespace mgx {

constexpr int kFpsMaxD = 64;
constexpr int kFpsSmallLds = 4096;    // floats: 16 KiB, many workgroups per CU (batches of small clouds)
constexpr int kFpsMidLds = 8192;      // 32 KiB
constexpr int kFpsBigLds = 38912;     // 152 KiB of the 160 KiB a workgroup may declare; the rest is the key slots
constexpr int kFpsMaxWaves = 16;

__host__ __device__ constexpr int fps_ld(int D) { return D | 1; }

// The configurations (threads T, points per thread P, LDS floats): the first one that holds max_len points of D floats is taken.
struct FpsConfig { int T, P, lds; };
constexpr int kFpsNumConfigs = 5;
constexpr FpsConfig kFpsConfigs[kFpsNumConfigs] = {{256, 1, kFpsSmallLds}, {512, 2, kFpsMidLds}, {512, 8, kFpsBigLds}, {1024, 8, kFpsBigLds},
                                                       {1024, 16, kFpsBigLds}};

static int fps_config(int64_t D, int64_t max_len) {
  if (D < 1 || D > kFpsMaxD || max_len < 0) return -1;
  for (int i = 0; i < kFpsNumConfigs; ++i)
    if (max_len <= (int64_t)kFpsConfigs[i].T * kFpsConfigs[i].P && max_len * fps_ld((int)D) <= kFpsConfigs[i].lds) return i;
  return -1;
}

template <int CTRL>
__device__ __forceinline__ uint64_t dpp_max64(uint64_t k) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)k, CTRL, 0xf, 0xf, true);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(k >> 32), CTRL, 0xf, 0xf, true);
  const uint64_t o = ((uint64_t)hi << 32) | lo;
  return o > k ? o : k;
}
// the greatest key of every 16-lane DPP row, in all of its lanes: VALU moves, no LDS pipe
__device__ __forceinline__ uint64_t row_max64(uint64_t k) {
  k = dpp_max64<0xB1>(k);   // quad_perm [1, 0, 3, 2]
  k = dpp_max64<0x4E>(k);   // quad_perm [2, 3, 0, 1]
  k = dpp_max64<0x141>(k);  // row_half_mirror
  k = dpp_max64<0x140>(k);  // row_mirror
  return k;
}
__device__ __forceinline__ uint64_t read_lane64(uint64_t k, int l) {
  return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(k >> 32), l) << 32) |
         (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)k, l);
}

// DC: D when the thread's own coordinates live in registers (3), 0: they are read from LDS every step.
template <int T, int P, int LDS, int DC>
__global__ __launch_bounds__(T) void segment_fps_kernel(const int64_t* __restrict__ offsets, int64_t N, int D, int64_t ld,
                                                        const float* __restrict__ x, int m, int max_len,
                                                        const int64_t* __restrict__ start, int64_t* __restrict__ index,
                                                        float* __restrict__ dist) {
  constexpr int kWaves = T / kWave;
  static_assert(kWaves <= kFpsMaxWaves && kWaves <= 16, "one DPP row reduces the wave keys");
  __shared__ float xs[LDS];
  __shared__ uint64_t slot[2][kFpsMaxWaves];
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int w = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int64_t s = blockIdx.x;
  if (DC) D = DC;
  const int ldp = fps_ld(D);
  int64_t beg = offsets[s], end = offsets[s + 1];
  beg = beg < 0 ? 0 : (beg > N ? N : beg);
  end = end < beg ? beg : (end > N ? N : end);
  int cap = T * P < LDS / ldp ? T * P : LDS / ldp;   // a segment longer than max_len (a caller error) is cut to what was provided for
  cap = max_len < cap ? max_len : cap;
  const int len = end - beg < cap ? (int)(end - beg) : cap;
  const int mm = m < len ? m : len;
  int64_t* __restrict__ oi = index + s * (int64_t)m;
  float* __restrict__ od = dist ? dist + s * (int64_t)m : nullptr;
  for (int t = mm + tid; t < m; t += T) {
    oi[t] = -1;
    if (od) od[t] = 0.f;
  }
  if (mm == 0) return;  // workgroup-uniform
  const float* __restrict__ xb = x + beg * ld;
  for (int e = tid; e < len * D; e += T) {
    const int r = e / D, c = e - r * D;
    xs[r * ldp + c] = xb[(int64_t)r * ld + c];
  }
  __syncthreads();
  float mind[P], own[P][DC ? DC : 1];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int j = tid + p * T;
    mind[p] = j < len ? __uint_as_float(0x7F800000u) : -1.f;  // -1: not a candidate (past the end; later: selected) -- no d is below it
    if (DC) {
#pragma unroll
      for (int c = 0; c < DC; ++c) own[p][c] = j < len ? xs[j * ldp + c] : 0.f;
    }
  }
  int cur = 0;
  if (start) {
    const int64_t st = start[s];
    cur = st >= 0 && st < len ? (int)st : 0;
  }
  uint32_t curd = 0x7F800000u;
  for (int t = 0;; ++t) {
    if (tid == 0) {
      oi[t] = beg + cur;
      if (od) od[t] = __uint_as_float(curd);
    }
    if (t == mm - 1) break;
    float bestd = -1.f;  // the thread's greatest mind and its lowest row: rows ascend with p and only a greater mind replaces
    int bestj = 0;
    const float* __restrict__ xc = xs + cur * ldp;  // workgroup-uniform
    if (DC) {
      float cc[DC ? DC : 1];
#pragma unroll
      for (int c = 0; c < DC; ++c) cc[c] = xc[c];
#pragma unroll
      for (int p = 0; p < P; ++p) {
        const int j = tid + p * T;
        float d = 0.f;
#pragma unroll
        for (int c = 0; c < DC; ++c) {
          const float diff = cc[c] - own[p][c];
          d = __builtin_fmaf(diff, diff, d);
        }
        if (j == cur) mind[p] = -1.f;  // selected: out of every later step
        if (d < mind[p]) mind[p] = d;  // false for a NaN d and for mind = -1
        if (mind[p] > bestd) {
          bestd = mind[p];
          bestj = j;
        }
      }
    } else {
      float acc[P];
#pragma unroll
      for (int p = 0; p < P; ++p) acc[p] = 0.f;
      for (int c = 0; c < D; ++c) {
        const float v = xc[c];
#pragma unroll
        for (int p = 0; p < P; ++p) {
          const int j = tid + p * T;
          const float diff = v - xs[(j < len ? j : 0) * ldp + c];
          acc[p] = __builtin_fmaf(diff, diff, acc[p]);
        }
      }
#pragma unroll
      for (int p = 0; p < P; ++p) {
        const int j = tid + p * T;
        if (j == cur) mind[p] = -1.f;
        if (acc[p] < mind[p]) mind[p] = acc[p];
        if (mind[p] > bestd) {
          bestd = mind[p];
          bestj = j;
        }
      }
    }
    uint64_t best = bestd >= 0.f ? ((uint64_t)__float_as_uint(bestd) << 32) | (uint32_t)~(uint32_t)bestj : 0;
    best = row_max64(best);
    uint64_t wk = read_lane64(best, 0);
    const uint64_t k1 = read_lane64(best, 16), k2 = read_lane64(best, 32), k3 = read_lane64(best, 48);
    wk = k1 > wk ? k1 : wk;
    wk = k2 > wk ? k2 : wk;
    wk = k3 > wk ? k3 : wk;
    if (kWaves > 1) {
      const int b = t & 1;
      if (lane == 0) slot[b][w] = wk;
      __syncthreads();
      wk = read_lane64(row_max64(lane < kWaves ? slot[b][lane] : 0), 0);
    }
    // mm <= len rows are selected in all, so before the last one an unselected row is left and wk != 0
    cur = (int)~(uint32_t)wk;
    cur = cur >= 0 && cur < len ? cur : 0;  // never taken; keeps every address inside the staged rows whatever happens
    curd = (uint32_t)(wk >> 32);
  }
}

template <int CFG>
static void fps_launch(int64_t S, const int64_t* offsets, int64_t N, int D, int64_t ld, const float* x, int m, int max_len,
                       const int64_t* start, int64_t* index, float* dist, hipStream_t stream) {
  constexpr FpsConfig c = kFpsConfigs[CFG];
  if (D == 3)
    hipLaunchKernelGGL((segment_fps_kernel<c.T, c.P, c.lds, 3>), dim3((unsigned)S), dim3(c.T), 0, stream, offsets, N, D, ld, x, m, max_len, start,
                       index, dist);
  else
    hipLaunchKernelGGL((segment_fps_kernel<c.T, c.P, c.lds, 0>), dim3((unsigned)S), dim3(c.T), 0, stream, offsets, N, D, ld, x, m, max_len, start,
                       index, dist);
}

}  // namespace mgx

extern "C" int32_t mgx_segment_fps_supported(int64_t D, int64_t max_len) { return mgx::fps_config(D, max_len) >= 0; }

extern "C" int32_t mgx_segment_fps(int64_t num_segments, const int64_t* offsets, int64_t N, int64_t D, int64_t ld, const float* x, int64_t m,
                                   int64_t max_len, const int64_t* start, int64_t* index, float* dist, void* stream) {
  using namespace mgx;
  MGX_ENTER();
  const char* who = "mgx_segment_fps";
  MGX_CHECK_ARG(num_segments >= 0 && N >= 0, "%s: negative num_segments or N", who);
  MGX_CHECK_ARG(D >= 1 && ld >= D, "%s: needs D >= 1 and a row stride of at least D (got D = %lld, ld = %lld)", who, (long long)D, (long long)ld);
  MGX_CHECK_ARG(m >= 1, "%s: m must be at least 1, got %lld", who, (long long)m);
  MGX_CHECK_ARG(max_len >= 0, "%s: negative max_len", who);
  const int cfg = fps_config(D, max_len);
  if (cfg < 0)
    MGX_UNSUPPORTED("%s: D = %lld beyond %d, or max_len = %lld points of D floats beyond %d points / %d KiB of LDS", who, (long long)D, kFpsMaxD,
                    (long long)max_len, kFpsConfigs[kFpsNumConfigs - 1].T * kFpsConfigs[kFpsNumConfigs - 1].P, kFpsBigLds / 256);
  const int64_t lim = int64_t(1) << 31;
  if (N >= lim || num_segments >= lim || ld >= lim || N * ld >= lim / 2 || m >= lim || num_segments * m >= lim)
    MGX_UNSUPPORTED("%s: needs N, num_segments and num_segments * m below 2^31 and x below 4 GiB (got N = %lld, num_segments = %lld, ld = %lld, "
                    "m = %lld)", who, (long long)N, (long long)num_segments, (long long)ld, (long long)m);
  if (num_segments == 0) return MGX_OK;
  MGX_CHECK_ARG(offsets && index && (x || N == 0), "%s: offsets / x / index is NULL", who);
  hipStream_t st = (hipStream_t)stream;
  switch (cfg) {
    case 0: fps_launch<0>(num_segments, offsets, N, (int)D, ld, x, (int)m, (int)max_len, start, index, dist, st); break;
    case 1: fps_launch<1>(num_segments, offsets, N, (int)D, ld, x, (int)m, (int)max_len, start, index, dist, st); break;
    case 2: fps_launch<2>(num_segments, offsets, N, (int)D, ld, x, (int)m, (int)max_len, start, index, dist, st); break;
    case 3: fps_launch<3>(num_segments, offsets, N, (int)D, ld, x, (int)m, (int)max_len, start, index, dist, st); break;
    default: fps_launch<4>(num_segments, offsets, N, (int)D, ld, x, (int)m, (int)max_len, start, index, dist, st); break;
  }
  MGX_CHECK_LAUNCH();
  return MGX_OK;
}
