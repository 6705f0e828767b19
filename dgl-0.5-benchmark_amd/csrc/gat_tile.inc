// gat_tile.inc -- the three fused GAT walks (gatfused.hip) as LDS-staged TILE kernels for one-head layers of up to 16 columns on
// graphs with dense neighbourhoods (main_dgl_reddit_gat.py:31-55 on reddit: 492 in-edges per node, hidden 16, one head).
// Included by gatfused.hip (same kernels' arithmetic, same per-node statistics, same hub fix-up kernels); the walk is
// spmm_tile.hip's narrow form: 8-wave workgroups, wave 0 gathers the tile's staged sources chunk by chunk into LDS with LDS-DMA
// -- a 64-byte row AND its small per-node record (el: 4 bytes; the source walk: (er, m, 1/s, t): 16 bytes) per source --, waves
// 1-7 walk their streams of LDS slots (four lanes per row, sixteen rows per wave-instruction), sources used once in the tile
// follow as a direct list.  A source that the row kernels fetch from L2 once per EDGE (one request each: they are request bound,
// DESIGN 4.4d) is fetched once per TILE here.

namespace mgx {

struct GatTileArgs {
  const int32_t* tile_chunk_ptr;
  const int32_t* chunk_ids;
  const int32_t* lds_off;
  const uint16_t* lds_cnt;
  const uint32_t* lds_stream;
  const uint32_t* lds_stream16;  // DROP: 16-bit entries, slot | rank << 8
  const int32_t* dir_off;
  const int32_t* dir_cnt;
  const int32_t* dir_stream;
  const int32_t* tile_item;
  const int32_t* tile_node;
  const float* zero_row;
  int num_tiles, tiles_per_xcd;
  int D;              // columns of the gathered rows (= F): 4, 8, 12 or 16
  int gat_ld;         // floats between consecutive rows of `gat`
  int small_ld;       // floats between consecutive nodes of `small`
  const float* gat;   // gathered rows: feat (FWD, BWD_DST), d out (BWD_SRC)
  const float* small; // gathered record: el[u] (FWD, BWD_DST), nstat[v] = (er, m, 1/s, t) (BWD_SRC)
  const float* er;    // FWD: [num_dst]
  const float* nstat; // BWD_DST: [num_dst, 4]
  float* nstat_w;     // FWD: (er, m, 1/s, 0); BWD_DST: t
  const float* rowa;  // row-constant operand [*, D]: d out[v] (BWD_DST), feat[u] (BWD_SRC)
  const float* rowb;  // BWD_DST: out[v]
  const float* el_row;  // BWD_SRC: el[u]
  float* out;         // FWD: out; BWD_SRC: d feat   [rows, D]
  float* out_h;       // BWD_DST: d er; BWD_SRC: d el   [rows]
  float* partial;     // [slots, D]
  float* partial_h;   // FWD: [slots, 2] (m, s); backward: [slots]
  float slope, keep_scale;
  uint32_t drop_below;
  uint64_t seed;
};

template <int MODE, bool DROP>
struct GatTileGeo {
  static constexpr int G = 4, NBG = 16, NC = 7;
  static constexpr int CS = 256;                                // slots per chunk (255 + the zero slot)
  static constexpr int CHB = CS * 64;                           // 16 KiB of rows per chunk
  static constexpr int PER = CHB / 1024;                        // row DMAs per chunk
  static constexpr int SMB = MODE == GAT_BWD_SRC ? 16 : 4;      // bytes of the small record
  static constexpr int SMCH = CS * SMB;                         // records of a chunk: 1 KiB / 4 KiB
  static constexpr int WS = 16;                                 // supersteps per window of the slot stream
  static constexpr int WB = DROP ? 2048 : 1024;                 // bytes of a window: 1-byte entries, or 2-byte (slot, rank) entries
  static constexpr int WSD = 4;                                 // supersteps per 1-KiB window of the direct stream
  static constexpr int kSmallOff = 2 * CHB;                     // [2 chunks][2 x records][3 x 1 KiB ids][7 x 2 windows]
  static constexpr int kIdsOff = kSmallOff + 2 * SMCH;
  static constexpr int kStreamOff = kIdsOff + 3 * 1024;
  static constexpr int kLdsBytes = kStreamOff + NC * 2 * WB;
};

// attn_drop: one bit per (seed, destination, source, rank among the parallel edges of that pair).  The row kernels key it by edge
// id; a tile walk does not know the ids of its entries (a 4-byte stream per edge), but it knows both endpoints -- the source of a
// staged entry is the chunk's id table in LDS -- and the plan gives it the edge's rank among parallel edges (by edge id, so both
// CSRs of a graph agree) in the second byte of the DROP stream's entries / bits 24-30 of a direct id.  A key per edge all the same;
// the two forms' masks differ, so a layer takes one form for all three of its walks (sparse.py: _gat_tile_plans).
__device__ __forceinline__ float gat_pair_keep(uint64_t seed, int dst, int src, uint32_t rank, uint32_t drop_below, float keep_scale) {
  return gat_hash(seed, (uint32_t)src, (uint32_t)dst + rank * 0x9E3779B1u) >= drop_below ? keep_scale : 0.f;
}

// dpp_mov<CTRL> below: x of the lane quad_perm names inside this lane's quad (four consecutive lanes = the lane group of one row);
// CTRL = a | b << 2 | c << 4 | d << 6: 0xB1 swaps neighbours, 0x4E swaps pairs, 0x00 / 0x55 / 0xAA / 0xFF broadcast lane 0 / 1 / 2 / 3.

template <int MODE, int NACC, bool DROP>
__global__ __launch_bounds__(512, 4) void gat_tile_kernel(const GatTileArgs a) {
  typedef GatTileGeo<MODE, DROP> Geo;
  constexpr int G = Geo::G, NBG = Geo::NBG, NC = Geo::NC, SMB = Geo::SMB;
  __shared__ __attribute__((aligned(1024))) char ring[Geo::kLdsBytes];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & (kWave - 1);
  const int tile = (int)(blockIdx.x % kXcds) * a.tiles_per_xcd + (int)(blockIdx.x / kXcds);
  if (tile >= a.num_tiles) return;
  const int cbeg = a.tile_chunk_ptr[tile];
  const int n = a.tile_chunk_ptr[tile + 1] - cbeg;
  const int g = lane >> 2, l = lane & (G - 1);
  const int col = l * 4;
  const bool cvalid = col < a.D;
  const uint32_t rowbytes = (uint32_t)a.gat_ld * 4u;
  const uint32_t smallbytes = (uint32_t)a.small_ld * 4u;

  if (wave == 0) {  // ---- the loader wave
    const char* zrow = reinterpret_cast<const char*>(a.zero_row) + l * 16;
    const char* zsmall = reinterpret_cast<const char*>(a.zero_row);
    const char* xcol = reinterpret_cast<const char*>(a.gat + col);
    const char* sbase = reinterpret_cast<const char*>(a.small);
    auto issue_ids = [&](int k) {  // ids ring of 3: the ids of chunk k stay readable while the consumers work on it (attn_drop keys)
      __builtin_amdgcn_global_load_lds((gbl_ptr_t)(a.chunk_ids + (int64_t)(cbeg + k) * Geo::CS + lane * 4),
                                       (lds_ptr_t)(ring + Geo::kIdsOff + (k % 3) * 1024), 16, 0, 0);
    };
    auto issue_rows = [&](int k) {  // chunk k: 16 row DMAs (16 slots each) + 4 record DMAs (64 slots each)
      const int* idl = reinterpret_cast<const int*>(ring + Geo::kIdsOff + (k % 3) * 1024);
      char* dst = ring + (k & 1) * Geo::CHB;
      char* sdst = ring + Geo::kSmallOff + (k & 1) * Geo::SMCH;
      int idv[Geo::PER], ids[4];
#pragma unroll
      for (int i = 0; i < Geo::PER; ++i) idv[i] = idl[i * NBG + g];
#pragma unroll
      for (int i = 0; i < 4; ++i) ids[i] = idl[i * 64 + lane];
#pragma unroll
      for (int i = 0; i < Geo::PER; ++i) {
        const bool live = idv[i] >= 0 && cvalid;
        const char* src = live ? xcol + (uint32_t)idv[i] * rowbytes : zrow;
        __builtin_amdgcn_global_load_lds((gbl_ptr_t)src, (lds_ptr_t)(dst + i * 1024), 16, 0, 0);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const char* src = ids[i] >= 0 ? sbase + (uint32_t)ids[i] * smallbytes : zsmall;
        // (literal sizes: the host pass of hipcc rejects a template-dependent 16 here)
        if (Geo::SMB == 16) __builtin_amdgcn_global_load_lds((gbl_ptr_t)src, (lds_ptr_t)(sdst + i * 1024), 16, 0, 0);
        else __builtin_amdgcn_global_load_lds((gbl_ptr_t)src, (lds_ptr_t)(sdst + i * 256), 4, 0, 0);
      }
    };
    if (n > 0) {
      issue_ids(0);
      wait_vmcnt<0>();
      issue_rows(0);
      if (n > 1) issue_ids(1);
    }
    for (int c = 0; c < n; ++c) {
      wait_vmcnt<0>();               // chunk c and the ids of chunk c + 1 have landed
      __builtin_amdgcn_s_barrier();  // ... and every consumer has finished chunk c - 1
      asm volatile("" ::: "memory");
      if (c + 1 < n) issue_rows(c + 1);
      if (c + 2 < n) issue_ids(c + 2);
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // the consumers' barrier between their two parts
    return;
  }

  // ---- consumer waves: row constants and accumulators of this lane group's NACC rows
  const int cw = wave - 1;
  int item[NACC], node[NACC];
  v4f acc[NACC], ra[NACC];
  float rm[NACC], rs[NACC], hacc[NACC], c0[NACC], c1[NACC], c2[NACC], c3[NACC];
#pragma unroll
  for (int j = 0; j < NACC; ++j) {
    const int64_t pos = (int64_t)tile * (NC * NACC * NBG) + (cw * NACC + j) * NBG + g;
    item[j] = a.tile_item[pos];
    node[j] = item[j] == kNoItem ? 0 : a.tile_node[pos];
    acc[j] = (v4f)(0.f);
    ra[j] = (v4f)(0.f);
    rm[j] = -INFINITY;
    rs[j] = 0.f;
    hacc[j] = 0.f;
    c0[j] = c1[j] = c2[j] = c3[j] = 0.f;
    const bool have = item[j] != kNoItem;
    if (MODE == GAT_FWD && have) c0[j] = a.er[node[j]];
    if (MODE == GAT_BWD_DST && have) {
      const v4f st = *reinterpret_cast<const v4f*>(a.nstat + (int64_t)node[j] * 4);
      c0[j] = st.x; c1[j] = st.y; c2[j] = st.z;
      v4f ov = (v4f)(0.f);
      if (cvalid) {
        ra[j] = *reinterpret_cast<const v4f*>(a.rowa + (int64_t)node[j] * a.D + col);
        ov = *reinterpret_cast<const v4f*>(a.rowb + (int64_t)node[j] * a.D + col);
      }
      float t = ra[j].x * ov.x + ra[j].y * ov.y + ra[j].z * ov.z + ra[j].w * ov.w;
      t += __shfl_xor(t, 1, kWave);  // the four lanes of a group share `have`
      t += __shfl_xor(t, 2, kWave);
      c3[j] = t;
      if (l == 0) a.nstat_w[(int64_t)node[j] * 4 + 3] = t;  // every chunk of a hub row writes the same value
    }
    if (MODE == GAT_BWD_SRC && have) {
      if (cvalid) ra[j] = *reinterpret_cast<const v4f*>(a.rowa + (int64_t)node[j] * a.D + col);
      c0[j] = a.el_row[node[j]];
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the row constants are in registers before the first stream DMA is counted

  // A superstep is four entries of row j, and the row's lane group is one DPP quad: lane l does the SCALAR work of entry l alone
  // (its logit, its exp, its mask bit: once per entry instead of once per lane and entry), the weights travel through quad_perm
  // broadcasts folded into the multiply-adds, maxima / sums / dot products through quad_perm swaps.  v: the four gathered rows
  // (every lane: its 16 bytes of each); sm: the record of THIS lane's entry; live, other: of this lane's entry.
  auto combine = [&](int j, const v4f (&v)[4], const v4f& sm, bool live, int other, uint32_t rank) {
    float keep = 1.f;
    if (DROP) keep = MODE == GAT_BWD_SRC ? gat_pair_keep(a.seed, other, node[j], rank, a.drop_below, a.keep_scale)
                                         : gat_pair_keep(a.seed, node[j], other, rank, a.drop_below, a.keep_scale);
    const float t = c0[j] + sm.x;
    const float z = t > 0.f ? t : t * a.slope;
    if (MODE == GAT_FWD) {
      float m4 = live ? z : -INFINITY;
      m4 = fmaxf(m4, dpp_mov<0xB1>(m4));
      m4 = fmaxf(m4, dpp_mov<0x4E>(m4));
      const float mx = fmaxf(rm[j], m4);
      const float resc = rm[j] > -INFINITY ? __expf(rm[j] - mx) : 0.f;
      const float pe = live && mx > -INFINITY ? __expf(z - mx) : 0.f;  // mx = -inf: only masked logits (-inf) so far
      float ps = pe + dpp_mov<0xB1>(pe);
      ps += dpp_mov<0x4E>(ps);
      const float pw = pe * keep;
      v4f pa = v[0] * dpp_mov<0x00>(pw);  // explicit fused multiply-adds (the library is built with -ffp-contract=off)
      pa = __builtin_elementwise_fma(v[1], (v4f)(dpp_mov<0x55>(pw)), pa);
      pa = __builtin_elementwise_fma(v[2], (v4f)(dpp_mov<0xAA>(pw)), pa);
      pa = __builtin_elementwise_fma(v[3], (v4f)(dpp_mov<0xFF>(pw)), pa);
      rs[j] = __builtin_fmaf(rs[j], resc, ps);
      acc[j] = __builtin_elementwise_fma(acc[j], (v4f)(resc), pa);
      rm[j] = mx;
    } else {
      const float mm = MODE == GAT_BWD_DST ? c1[j] : sm.y;
      const float is = MODE == GAT_BWD_DST ? c2[j] : sm.z;
      const float tt = MODE == GAT_BWD_DST ? c3[j] : sm.w;
      const float av = live ? __expf(z - mm) * is : 0.f;
      float d[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        d[u] = __builtin_fmaf(v[u].w, ra[j].w, __builtin_fmaf(v[u].z, ra[j].z, __builtin_fmaf(v[u].y, ra[j].y, v[u].x * ra[j].x)));
        d[u] += dpp_mov<0xB1>(d[u]);
        d[u] += dpp_mov<0x4E>(d[u]);
      }
      float dot = d[0];  // this lane's entry
      dot = l == 1 ? d[1] : dot;
      dot = l == 2 ? d[2] : dot;
      dot = l == 3 ? d[3] : dot;
      hacc[j] += av * (dot * keep - tt) * (t > 0.f ? 1.f : a.slope);  // summed over the quad in the epilogue
      if (MODE == GAT_BWD_SRC) {
        const float w = av * keep;
        acc[j] = __builtin_elementwise_fma(v[0], (v4f)(dpp_mov<0x00>(w)), acc[j]);
        acc[j] = __builtin_elementwise_fma(v[1], (v4f)(dpp_mov<0x55>(w)), acc[j]);
        acc[j] = __builtin_elementwise_fma(v[2], (v4f)(dpp_mov<0xAA>(w)), acc[j]);
        acc[j] = __builtin_elementwise_fma(v[3], (v4f)(dpp_mov<0xFF>(w)), acc[j]);
      }
    }
  };

  if (n > 0) {  // ---- staged part: 1-KiB windows (16 supersteps) of the slot stream in a private 2-window ring, as spmm_tile.hip
    const auto* cnt = as_const(reinterpret_cast<const v4u*>(a.lds_cnt));
    int64_t k = (int64_t)cbeg * NC + cw;
    // per superstep and lane group: 4 bytes of slots (one word), or with DROP 8 bytes of (slot, rank) entries (two words)
    const int64_t soff = as_const(a.lds_off)[(int64_t)tile * NC + cw];
    const uint32_t* gs = DROP ? a.lds_stream16 + soff * (NBG * 2) + lane * 4 : a.lds_stream + soff * NBG + lane * 4;
    char* swin = ring + Geo::kStreamOff + cw * (2 * Geo::WB);
    auto dma = [&](int wi) {
      __builtin_amdgcn_global_load_lds((gbl_ptr_t)(gs + (int64_t)wi * (Geo::WB / 4)), (lds_ptr_t)(swin + (wi & 1) * Geo::WB), 16, 0, 0);
      if (DROP) __builtin_amdgcn_global_load_lds((gbl_ptr_t)(gs + (int64_t)wi * (Geo::WB / 4) + 256),
                                                 (lds_ptr_t)(swin + (wi & 1) * Geo::WB + 1024), 16, 0, 0);
    };
    dma(0);
    dma(1);
    wait_vmcnt<0>();
    int ss = 0;
    int landed = 2 * Geo::WS;
    int issue_at = Geo::WS, nextw = 2;
    auto word = [&](int i) -> v2u {  // .x: the four slots; .y (DROP): the four ranks
      const char* wp = swin + ((i / Geo::WS) & 1) * Geo::WB + (i % Geo::WS) * (Geo::WB / Geo::WS) + g * (DROP ? 8 : 4);
      v2u w;
      if (DROP) {
        const v2u e = *reinterpret_cast<const v2u*>(wp);  // four 16-bit entries: slot | rank << 8
        w.x = (e.x & 0xffu) | ((e.x >> 8) & 0xff00u) | ((e.y & 0xffu) << 16) | ((e.y << 8) & 0xff000000u);
        w.y = ((e.x >> 8) & 0xffu) | ((e.x >> 16) & 0xff00u) | ((e.y << 8) & 0xff0000u) | (e.y & 0xff000000u);
      } else {
        w.x = *reinterpret_cast<const uint32_t*>(wp);
        w.y = 0u;
      }
      return w;
    };
    auto prepare = [&](int lo, int hi) {  // the words of supersteps lo .. hi are about to be read
      if (hi >= landed) {
        wait_vmcnt<0>();
        landed = nextw * Geo::WS;
      }
      if (lo >= issue_at) {
        dma(nextw);
        ++nextw;
        issue_at += Geo::WS;
      }
    };
    v2u w0 = word(0), w1 = word(1);
    for (int c = 0; c < n; ++c) {
      const v4u cq = cnt[2 * k];
      const uint32_t cnts[4] = {cq.x, cq.y, cq.z, cq.w};
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      const char* rows = ring + (c & 1) * Geo::CHB + l * 16;
      const char* recs = ring + Geo::kSmallOff + (c & 1) * Geo::SMCH;
      const char* idl = ring + Geo::kIdsOff + (c % 3) * 1024;
      auto step = [&](int j, const v2u& w) {
        v4f v[4], sm = (v4f)(0.f);
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const v4f*>(rows + (((w.x >> (8 * u)) & 0xffu) << 6));
        const uint32_t slot = (w.x >> (8 * l)) & 0xffu;  // this lane's entry
        if (SMB == 16) sm = *reinterpret_cast<const v4f*>(recs + (slot << 4));
        else sm.x = *reinterpret_cast<const float*>(recs + (slot << 2));
        const int other = DROP ? *reinterpret_cast<const int*>(idl + (slot << 2)) : 0;
        combine(j, v, sm, slot != (uint32_t)(Geo::CS - 1), other, (w.y >> (8 * l)) & 0xffu);
      };
#pragma unroll
      for (int j = 0; j < NACC; ++j) {
        const int nss = (int)((cnts[j >> 1] >> ((j & 1) * 16)) & 0xffffu);
        int s = 0;
        for (; s + 2 <= nss; s += 2) {
          prepare(ss + 2, ss + 3);
          const v2u n0 = word(ss + 2), n1 = word(ss + 3);
          step(j, w0);
          step(j, w1);
          w0 = n0;
          w1 = n1;
          ss += 2;
        }
        if (s < nss) {
          prepare(ss + 2, ss + 2);
          const v2u n1 = word(ss + 2);
          step(j, w0);
          w0 = w1;
          w1 = n1;
          ss += 1;
        }
      }
      k += NC;
    }
  }

  // ---- direct part: sources used once in the tile, gathered from global memory; 1-KiB windows of ids (4 supersteps, ring of 4)
  // live where the chunks were
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  {
    const int64_t k = (int64_t)tile * NC + cw;
    const int so = as_const(a.dir_off)[k], se = as_const(a.dir_off)[k + 1];
    if (se > so) {
      const auto* dcnt = as_const(reinterpret_cast<const v4u*>(a.dir_cnt)) + k * 4;
      const v4u c0q = dcnt[0];
      const uint32_t cnts[4] = {c0q.x, c0q.y, c0q.z, c0q.w};
      const v4i* gd = reinterpret_cast<const v4i*>(a.dir_stream) + (int64_t)so * NBG + lane;
      char* dwin = ring + cw * 4096;
      auto dma = [&](int wi) {
        __builtin_amdgcn_global_load_lds((gbl_ptr_t)(gd + (int64_t)wi * 64), (lds_ptr_t)(dwin + (wi & 3) * 1024), 16, 0, 0);
      };
      dma(0);
      dma(1);
      wait_vmcnt<1>();
      dma(2);
      int ss = 0, ready = Geo::WSD;
      auto ids = [&](int i) -> v4i { return *reinterpret_cast<const v4i*>(dwin + (i % (4 * Geo::WSD)) * (NBG * 16) + g * 16); };
      auto open_window = [&](int upto) {
        if (upto >= ready) {
          wait_vmcnt<1>();
          dma(ready / Geo::WSD + 2);
          ready += Geo::WSD;
        }
      };
      const char* xb = reinterpret_cast<const char*>(a.gat) + (size_t)(cvalid ? col : 0) * 4u;
      const char* zb = reinterpret_cast<const char*>(a.zero_row) + (size_t)(cvalid ? col : 0) * 4u;
      const char* sb = reinterpret_cast<const char*>(a.small);
      auto step = [&](int j, const v4i& id4) {  // an id: bits 0-23 the source, bits 24-30 its rank among parallel edges, -1 = padding
        v4f v[4], sm = (v4f)(0.f);
#pragma unroll
        for (int u = 0; u < 4; ++u)  // padding gathers the zero row: its weight is 0, and 0 x a NaN or inf of source 0 would be NaN
          v[u] = *reinterpret_cast<const v4f*>(id4[u] >= 0 ? xb + ((uint32_t)id4[u] & 0xFFFFFFu) * rowbytes : zb);
        int mine = id4[0];  // this lane's entry
        mine = l == 1 ? id4[1] : mine;
        mine = l == 2 ? id4[2] : mine;
        mine = l == 3 ? id4[3] : mine;
        const uint32_t id = mine >= 0 ? (uint32_t)mine & 0xFFFFFFu : 0u;
        if (SMB == 16) sm = *reinterpret_cast<const v4f*>(sb + id * smallbytes);
        else sm.x = *reinterpret_cast<const float*>(sb + id * smallbytes);
        if (!cvalid) {
#pragma unroll
          for (int u = 0; u < 4; ++u) v[u] = (v4f)(0.f);
        }
        combine(j, v, sm, mine >= 0, (int)id, ((uint32_t)mine >> 24) & 0x7fu);
      };
      v4i i0 = ids(0), i1 = ids(1);
#pragma unroll
      for (int j = 0; j < NACC; ++j) {
        const int nss = (int)cnts[j];
        int s = 0;
        for (; s + 2 <= nss; s += 2) {
          open_window(ss + 3);
          const v4i n0 = ids(ss + 2), n1 = ids(ss + 3);
          step(j, i0);
          step(j, i1);
          i0 = n0;
          i1 = n1;
          ss += 2;
        }
        if (s < nss) {
          open_window(ss + 2);
          const v4i n1 = ids(ss + 2);
          step(j, i0);
          i0 = i1;
          i1 = n1;
          ss += 1;
        }
      }
    }
  }

  // ---- epilogue: one row (or the partial slot of a hub chunk) per lane group and j
#pragma unroll
  for (int j = 0; j < NACC; ++j) {
    if (item[j] == kNoItem) continue;
    const bool whole = item[j] >= 0;
    const int64_t row = node[j], slot = plan_slot(item[j]);
    if (MODE == GAT_FWD) {
      if (whole) {
        const float is = rs[j] > 0.f ? 1.f / rs[j] : 0.f;  // rows without in-edges aggregate to 0
        if (cvalid) *reinterpret_cast<v4f*>(a.out + row * a.D + col) = acc[j] * is;
        if (l == 0) {
          v4f st;
          st.x = c0[j];
          st.y = rm[j] > -INFINITY ? rm[j] : 0.f;
          st.z = is;
          st.w = 0.f;
          *reinterpret_cast<v4f*>(a.nstat_w + row * 4) = st;
        }
      } else {
        if (cvalid) *reinterpret_cast<v4f*>(a.partial + slot * a.D + col) = acc[j];
        if (l == 0) {
          a.partial_h[slot * 2] = rm[j];
          a.partial_h[slot * 2 + 1] = rs[j];
        }
      }
    } else {
      if (MODE == GAT_BWD_SRC && cvalid) *reinterpret_cast<v4f*>((whole ? a.out + row * a.D : a.partial + slot * a.D) + col) = acc[j];
      float hs = hacc[j] + dpp_mov<0xB1>(hacc[j]);  // every lane accumulated the terms of its own entries
      hs += dpp_mov<0x4E>(hs);
      if (l == 0) *(whole ? a.out_h + row : a.partial_h + slot) = hs;
    }
  }
}

static bool gat_tile_shape_ok(const mgx_tile_plan* tp, int64_t H, int64_t F) {
  return tp && H == 1 && F >= 4 && F <= 16 && F % 4 == 0 && tp->lanes_log2 == 2 && tp->consumers == 7 && tp->loaders == 1 &&
         (tp->nacc == 3 || tp->nacc == 4) && tp->tile_node != nullptr;
}

static void gat_tile_fill(GatTileArgs& a, const mgx_tile_plan* tp, int64_t F, float slope, float p, uint64_t seed) {
  memset(&a, 0, sizeof(a));
  a.tile_chunk_ptr = tp->tile_chunk_ptr; a.chunk_ids = tp->chunk_ids; a.lds_off = tp->lds_off; a.lds_cnt = tp->lds_cnt;
  a.lds_stream = tp->lds_stream; a.lds_stream16 = tp->lds_stream16; a.dir_off = tp->dir_off; a.dir_cnt = tp->dir_cnt;
  a.dir_stream = tp->dir_stream; a.tile_item = tp->tile_item; a.tile_node = tp->tile_node;
  a.zero_row = tp->zero_row;
  a.num_tiles = (int)tp->num_tiles;
  a.tiles_per_xcd = (int)((tp->num_tiles + kXcds - 1) / kXcds);
  a.D = (int)F; a.gat_ld = (int)F; a.small_ld = 1;
  a.slope = slope; a.seed = seed;
  a.keep_scale = 1.f / (1.f - p);
  double thr = (double)p * 4294967296.0;
  a.drop_below = thr >= 4294967295.0 ? 4294967295u : (uint32_t)thr;
}

template <int MODE>
static bool gat_tile_launch(const GatTileArgs& a, int nacc, bool drop, hipStream_t s) {
  const dim3 grid((unsigned)(a.tiles_per_xcd * kXcds)), block(512);
#define MGX_GAT_TILE(NACC_)                                                                                  \
  if (nacc == NACC_) {                                                                                        \
    if (drop) hipLaunchKernelGGL((gat_tile_kernel<MODE, NACC_, true>), grid, block, 0, s, a);                 \
    else hipLaunchKernelGGL((gat_tile_kernel<MODE, NACC_, false>), grid, block, 0, s, a);                     \
    return true;                                                                                              \
  }
  MGX_GAT_TILE(3)
  MGX_GAT_TILE(4)
#undef MGX_GAT_TILE
  return false;
}

}  // namespace mgx
