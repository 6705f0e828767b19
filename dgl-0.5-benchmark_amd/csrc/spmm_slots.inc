// spmm_slots.inc -- included by spmm.hip inside namespace mgx (uses its SpmmFastArgs, plan stretches and hub fix-up).
//
// copy_u / sum|mean over a gathered matrix of 64 columns whose rows are MOSTLY ZERO -- dropout(relu(.)) outputs, the input of every hidden
// GraphSAGE layer (main_dgl_product_sage.py:93-96): 20-25 % non-zero on the benchmark model.  The wave-per-item kernel moves whole
// 256-byte rows from L2 to the CUs at ~15 TB/s and is bound by exactly that (docs/LOG_r05.md section 5); here a source row travels as ONE
// 128-byte SLOT -- one cache line per edge instead of two:
//
//   slot = 8 x { meta, v0, v1, v2 } (16 bytes per lane of the 8 lanes that fetch it)
//   meta = c0 | c1 << 8 | c2 << 16 | flag << 24     c = column of the value, 64 = none (value 0.0f)
//   the row's non-zeros in increasing (component, lane) order of the 16-lane x float4 layout, three per lane; up to 24 per row.
//   A row with more than 24 non-zeros has flag = 255 in EVERY lane: the kernel gathers the dense row instead (0.9 % of the rows at
//   25 % density).  Exact: values are moved, never rounded.
//
// Accumulation: a lane group of 8 lanes owns a 64-float accumulator row in LDS; every lane adds its three values at their columns by
// plain read - add - write (three reads, then three writes: the columns of one source row are distinct, lane groups own different
// accumulator rows, and a wave's LDS operations execute in order, so no two updates of one address overlap) -- NOT ds_add_f32, which
// runs 12 x slower here (14.8 ms against 1.2 ms, profiles/r05_sparse_row_bound.txt).  The eight accumulator rows are summed per output
// column in the epilogue.  Fixed summation order => bitwise reproducible for a given graph and input.
//
// Schedule: spmm_rowwave32_kernel's (plan items, per-XCD stretches, ids as byte offsets through ds_bpermute, the next item's ids
// prefetched, 8 U source rows per step and two steps in flight per wave).

constexpr int kSlotAccStride = 72;  // floats per lane-group accumulator row: bank = (8 g + c) % 64

template <int U, bool PP>
__global__ __launch_bounds__(kBlock) void spmm_slots_kernel(const SpmmFastArgs<int32_t> a, const char* __restrict__ slots) {
  __shared__ float acc_all[kWavesPerBlock][8][kSlotAccStride];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int grp = lane >> 3, gi = lane & 7;
  float* accw = &acc_all[wave][0][0];
  float* accg = accw + grp * kSlotAccStride;
  for (int i = lane; i < 8 * kSlotAccStride; i += kWave) accw[i] = 0.f;
  int64_t item_base, item_stop;
  xcd_stretch(a.xcd, item_base, item_stop);
  item_base += (int64_t)(blockIdx.x / kXcds) * a.rpb;
  int r = wave;
  if (r >= a.rpb || item_base + r >= item_stop) return;
  const uint32_t laneoff = (uint32_t)gi * 16u;

  auto load_meta = [&](int64_t item, int64_t& row, int32_t& beg, int32_t& end) {
    if (a.item_row) {
      row = (int64_t)a.item_row[item];
      beg = a.item_beg[item];
      end = a.item_end[item];
    } else {
      row = item;
      beg = a.indptr[item];
      end = a.indptr[item + 1];
    }
  };
  auto load_ids = [&](int32_t base, int32_t end) -> uint32_t {
    const int32_t q = base + lane;
    return q < end ? (uint32_t)__builtin_nontemporal_load(&a.indices[q]) * (uint32_t)kSlotBytes : 0u;
  };

  // the gathers of one step: 8 U edges from edge k of the current 64-edge chunk on, one 16-byte piece of a slot per lane
  auto issue = [&](int k, int cnt, uint32_t goff, v4f (&val)[U], uint32_t (&roff)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int e = k + u * 8 + grp;
      roff[u] = (uint32_t)__builtin_amdgcn_ds_bpermute((e < cnt ? e : 0) * 4, (int)goff);
      val[u] = *reinterpret_cast<const v4f*>(slots + roff[u] + laneoff);
    }
  };
  auto consume = [&](int k, int cnt, const v4f (&val)[U], const uint32_t (&roff)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (k + u * 8 + grp < cnt) {
        const uint32_t meta = (uint32_t)__float_as_int(val[u].x);
        if ((meta >> 24) != 255u) {
          const uint32_t c0 = meta & 0xffu, c1 = (meta >> 8) & 0xffu, c2 = (meta >> 16) & 0xffu;
          const float a0 = accg[c0], a1 = accg[c1], a2 = accg[c2];  // (column 64 = the padding element of the accumulator row)
          if (c0 < 64u) accg[c0] = a0 + val[u].y;
          if (c1 < 64u) accg[c1] = a1 + val[u].z;
          if (c2 < 64u) accg[c2] = a2 + val[u].w;
        } else {  // more than 24 non-zeros: the dense row, 8 columns per lane
          const uint32_t srow = roff[u] / (uint32_t)kSlotBytes;
          const float* dr = a.src + (size_t)srow * (size_t)a.lds + gi * 8;
          v4f d0 = *reinterpret_cast<const v4f*>(dr), d1 = *reinterpret_cast<const v4f*>(dr + 4);
          if (a.src_scale) {  // the slots carry pre-scaled values (mgx_rows_slots_pack's row_scale); the dense row does not
            const float sc = a.src_scale[srow];
            d0 *= sc;
            d1 *= sc;
          }
          v4f* ar = reinterpret_cast<v4f*>(accg + gi * 8);
          ar[0] += d0;
          ar[1] += d1;
        }
      }
    }
  };

  int64_t row;
  int32_t beg, end;
  load_meta(item_base + r, row, beg, end);
  uint32_t goff = load_ids(beg, end);
  for (;;) {
    const int rn = r + kWavesPerBlock;
    const bool has_next = rn < a.rpb && item_base + rn < item_stop;
    int64_t nrow = 0;
    int32_t nbeg = 0, nend = 0;
    uint32_t ngoff = 0;
    if (has_next) {
      load_meta(item_base + rn, nrow, nbeg, nend);
      ngoff = load_ids(nbeg, nend);
    }
    // out += result: the row to add to is requested before the item's gathers (spmm_rowwave32_kernel's reason)
    float prior = 0.f;
    if (a.accum && row >= 0) prior = a.out[row * (int64_t)a.ldo + lane];
    for (int32_t cbase = beg; cbase < end; cbase += kWave) {
      if (cbase != beg) goff = load_ids(cbase, end);
      const int cnt = (end - cbase) < kWave ? (end - cbase) : kWave;
      // two buffers in ping-pong: the gathers of step k + 1 are in flight while step k's values are added (the LDS pipe and the
      // vector-memory pipe are different units; without this the gathers wait for every read - add - write chain)
      v4f va[U], vb[U];
      uint32_t ra[U], rb[U];
      if (PP) {
        issue(0, cnt, goff, va, ra);
        int k = 0;
        for (;;) {
          if (k + 8 * U >= cnt) { consume(k, cnt, va, ra); break; }
          issue(k + 8 * U, cnt, goff, vb, rb);
          consume(k, cnt, va, ra);
          k += 8 * U;
          if (k + 8 * U >= cnt) { consume(k, cnt, vb, rb); break; }
          issue(k + 8 * U, cnt, goff, va, ra);
          consume(k, cnt, vb, rb);
          k += 8 * U;
        }
      } else {
        for (int k = 0; k < cnt; k += 8 * U) {
          issue(k, cnt, goff, va, ra);
          consume(k, cnt, va, ra);
        }
      }
    }
    float res = 0.f;
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      res += accw[g * kSlotAccStride + lane];
      accw[g * kSlotAccStride + lane] = 0.f;
    }
    if (row >= 0) {
      if (a.mean) {
        const int deg = end - beg;
        res = res / (float)(deg > 1 ? deg : 1);
      }
      if (a.dst_scale) res = res * a.dst_scale[row];
      if (a.accum) res += prior;
      __builtin_nontemporal_store(res, a.out + row * (int64_t)a.ldo + lane);
    } else {
      a.partial[(-(row + 1)) * (int64_t)64 + lane] = res;
    }
    if (!has_next) break;
    r = rn;
    row = nrow; beg = nbeg; end = nend;
    goff = ngoff;
  }
}

// mgx_spmm_copy_u_slots_init: the INIT launch of spmm_rowwave32_kernel<4, 16, ...> (plain copy_u sum whose initial value comes from a compact
// matrix, `out` write-only) for a gathered matrix most of whose ROWS are zero (d neigh / deg of a loss taken on 8 % of the nodes).  The
// slots are the PROBE: the lane that holds an edge's id fetches the first meta word of that source's slot -- one line per edge -- and the
// row is LIVE iff that word carries the flag 255 or a column below 64 (slot_pack_rows4 fills group 0 first: exactly "the row has a
// non-zero").  A live row is gathered whole from the dense matrix, zeros included, whether its slot holds values or the flag; a dead
// edge costs its probe and nothing else.
//
// The sum has the dense INIT launch's bits, which fixes the order of additions: that kernel keeps one float4 accumulator per lane group
// (16 lanes, four groups), edge e of an item (counted from the item's first edge) is added to group e % 4's in increasing e, group 0's
// starts from the initial value, and the result is (A0 + A1) + (A2 + A3) through the xor-shuffle tree.  Here lane group s walks the
// LIVE edges among e = s, s + 4, s + 8, ... of a 64-edge chunk in increasing e, four per step -- its own bits of the chunk's live ballot,
// lowest first -- so every accumulator receives the addends of the dense launch in the dense launch's order, minus the rows that are
// all zero.  Such a row's addend is +0.0f in every column.  x + (+0.0f) is x for every x but -0.0f, and an accumulator that is -0.0f at
// the end of an item leaves the result unchanged too: A1 .. A3 start from +0.0f and a sum that started from +0.0f is never -0.0f, so
// A0 = -0.0f and A0 = +0.0f give the same (A0 + A1).  Edges are never moved between lane groups (that is spmm_rowwave32_kernel's
// MASKED form, another sum).
//
// Schedule: the bounds and map entries of all of a wave's items are fetched at once, one item per lane.  The items then are one stream of
// 64-edge chunks with three of them open -- the ids of chunk c + 2 and the probes of chunk c + 1 are requested before the gathers of
// chunk c and consumed after them, so neither round trip is paid per chunk or per item.  With 8 % live rows a lane group has 1.3 live
// edges per chunk, so one step of four gathers per group covers a chunk (more than four live among a group's sixteen: 0.7 % of the
// groups) and one value buffer is enough: 42 VGPRs, 8 waves per SIMD.  (Two buffers in ping-pong as in spmm_rowwave32_kernel: 78 VGPRs,
// 6 waves, 1.54 ms against 1.51 ms for the whole call on the products graph -- docs/LOG_head_probe.md.)  Every gather is unconditional:
// a lane group with no live edge left reads the matrix's first 16 bytes (one hot line for all such lanes of the wave) and the value is
// dropped where it is consumed, so the wait counts stay exact.  No LDS.
__device__ __forceinline__ bool slot_meta_live(uint32_t meta) { return (meta >> 24) == 255u || (meta & 0xffu) < 64u; }

__global__ __launch_bounds__(kBlock) void spmm_probe_init_kernel(const SpmmFastArgs<int32_t> a, const char* __restrict__ slots) {
  constexpr int G = 16, U = 4;
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int sub = lane / G;
  const uint32_t f4 = (uint32_t)(lane % G) * 16u;
  int64_t item_base, item_stop;
  xcd_stretch(a.xcd, item_base, item_stop);
  item_base += (int64_t)(blockIdx.x / kXcds) * a.rpb + wave;  // this wave's items: item_base + kWavesPerBlock * i
  const uint32_t rowbytes = (uint32_t)a.lds * 4u;
  const char* __restrict__ srcb = reinterpret_cast<const char*>(a.src);

  // The wave's items all at once, item i in lane i (at most 64: launch_spmm_slots keeps rpb <= 64 * kWavesPerBlock): one round trip for the
  // bounds of all of them and one for their map entries, instead of that chain per item.
  int32_t rowv = 0, begv = 0, endv = 0, iposv = -1;
  {
    const int r = wave + kWavesPerBlock * lane;
    const int64_t item = item_base + (int64_t)kWavesPerBlock * lane;
    if (r < a.rpb && item < item_stop) {
      if (a.item_row) {
        rowv = a.item_row[item];
        begv = a.item_beg[item];
        endv = a.item_end[item];
        if (rowv >= 0) iposv = (int32_t)a.init_pos[rowv];  // (a chunk of a split row starts from zero: its row's value enters in the fix-up)
      } else {
        begv = a.indptr[item];
        endv = a.indptr[item + 1];
        iposv = (int32_t)a.init_pos[item];
      }
    }
  }
  const int n_mine = __popcll(__ballot(wave + kWavesPerBlock * lane < a.rpb && item_base + (int64_t)kWavesPerBlock * lane < item_stop));
  if (n_mine == 0) return;

  struct Chunk {  // 64 edges [cbase, min(cbase + 64, end)) of the wave's item i (an item without edges: one empty chunk)
    int i;
    bool ok;
    int32_t beg, end, cbase;
  };
  auto open_item = [&](Chunk& c) {
    c.ok = c.i < n_mine;
    c.beg = 0; c.end = 0;
    if (c.ok) {
      c.beg = __builtin_amdgcn_readlane(begv, c.i);
      c.end = __builtin_amdgcn_readlane(endv, c.i);
    }
    c.cbase = c.beg;
  };
  auto next_chunk = [&](Chunk& c) {
    if (!c.ok) return;
    if (c.cbase + kWave < c.end) {
      c.cbase += kWave;
    } else {
      c.i += 1;
      open_item(c);
    }
  };
  auto load_ids = [&](const Chunk& c) -> uint32_t {  // lane j: source row of edge cbase + j (0 past the end)
    const int32_t q = c.cbase + lane;
    return (c.ok && q < c.end) ? (uint32_t)__builtin_nontemporal_load(&a.indices[q]) : 0u;
  };
  auto probe = [&](uint32_t gid) -> uint32_t {  // unconditional: a lane past the end reads slot 0
    return *reinterpret_cast<const uint32_t*>(slots + gid * (uint32_t)kSlotBytes);
  };
  // one step of a lane group: its next four live edges, lowest first; `m` = the group's live edges still to gather, bit 4 t = edge 4 t + sub
  auto issue_step = [&](uint64_t& m, uint32_t goff, v4f (&val)[U], uint32_t& has) {
    has = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool h = m != 0;
      const int e = h ? (int)__builtin_ctzll(m) + sub : 0;
      m &= m - 1;
      const uint32_t g = (uint32_t)__builtin_amdgcn_ds_bpermute(e * 4, (int)goff);
      val[u] = *reinterpret_cast<const v4f*>(srcb + (h ? g + f4 : 0u));
      has |= (h ? 1u : 0u) << u;
    }
  };
  auto consume_step = [&](const v4f (&val)[U], uint32_t has, v4f& acc) {
#pragma unroll
    for (int u = 0; u < U; ++u) acc += ((has >> u) & 1u) ? val[u] : (v4f)(0.f);
  };

  Chunk c0;
  c0.i = 0;
  open_item(c0);
  uint32_t g0 = load_ids(c0);
  Chunk c1 = c0;
  next_chunk(c1);
  uint32_t g1 = load_ids(c1);
  bool live0 = c0.cbase + lane < c0.end && slot_meta_live(probe(g0));
  Chunk c2 = c1;
  v4f acc = (v4f)(0.f);
  for (;;) {
    next_chunk(c2);
    const uint32_t g2 = load_ids(c2);
    const uint32_t p1 = probe(g1);
    // the initial value is requested before the item's gathers, as lane group 0's accumulator (spmm_rowwave32_kernel's reason)
    if (c0.cbase == c0.beg) {
      const int32_t ipos = __builtin_amdgcn_readlane(iposv, c0.i);
      acc = (v4f)(0.f);
      if (ipos >= 0 && sub == 0)
        acc = *reinterpret_cast<const v4f*>(reinterpret_cast<const char*>(a.init) + ((uint32_t)ipos * ((uint32_t)a.ldi * 4u) + f4));
    }
    const uint64_t lb = __ballot(live0);
    if (lb != 0) {  // (a chunk without a live source adds nothing)
      const uint32_t goff = g0 * rowbytes;
      uint64_t m = (lb >> sub) & 0x1111111111111111ull;
      do {
        v4f val[U];
        uint32_t has;
        issue_step(m, goff, val, has);
        consume_step(val, has, acc);
      } while (__ballot(m != 0) != 0);
    }
    if (c0.cbase + kWave >= c0.end) {  // the item's last chunk
#pragma unroll
      for (int off = G; off < kWave; off <<= 1) acc += vec_shfl_xor<4>(acc, off);
      if (sub == 0) {
        const int64_t row = a.item_row ? (int64_t)__builtin_amdgcn_readlane(rowv, c0.i) : item_base + (int64_t)kWavesPerBlock * c0.i;
        if (row >= 0) __builtin_nontemporal_store(acc, reinterpret_cast<v4f*>(a.out + row * (int64_t)a.ldo + (f4 >> 2)));
        else *reinterpret_cast<v4f*>(a.partial + (-(row + 1)) * (int64_t)64 + (f4 >> 2)) = acc;
      }
    }
    if (!c1.ok) break;
    live0 = c1.cbase + lane < c1.end && slot_meta_live(p1);
    c0 = c1;
    c1 = c2;
    g0 = g1;
    g1 = g2;
  }
}

// SHORT work items (the head of a two-part plan: direct rows of at most 32 edges): one item per LANE GROUP of 8 lanes, 8 items per wave at
// a time (spmm_rowgroup32_kernel's reason: a wave per 3-edge row is one dependent chain per row).  The group's 8 lanes fetch the 8 pieces
// of one slot per edge, U edges in flight, and add into the group's own accumulator row, which IS the item's result: no cross-group sum.
template <int U>
__global__ __launch_bounds__(kBlock) void spmm_slots_short_kernel(const SpmmFastArgs<int32_t> a, const char* __restrict__ slots) {
  __shared__ float acc_all[kWavesPerBlock][8][kSlotAccStride];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int grp = lane >> 3, gi = lane & 7;
  float* accw = &acc_all[wave][0][0];
  float* accg = accw + grp * kSlotAccStride;
  for (int i = lane; i < 8 * kSlotAccStride; i += kWave) accw[i] = 0.f;
  int64_t item_base, item_stop;
  xcd_stretch(a.xcd, item_base, item_stop);
  item_base += (int64_t)(blockIdx.x / kXcds) * a.rpb;
  const uint32_t laneoff = (uint32_t)gi * 16u;
  const int gbase = grp * 8;

  auto load_meta = [&](int r, bool& ok, int64_t& row, int32_t& beg, int32_t& end) {
    const int64_t item = item_base + r;
    ok = r < a.rpb && item < item_stop;
    row = 0; beg = 0; end = 0;
    if (ok) {
      if (a.item_row) {
        row = (int64_t)a.item_row[item];
        beg = a.item_beg[item];
        end = a.item_end[item];
      } else {
        row = item;
        beg = a.indptr[item];
        end = a.indptr[item + 1];
      }
    }
  };
  auto load_ids = [&](int32_t base, int32_t end) -> uint32_t {  // lane gi of the group: byte offset of the slot of neighbour base + gi
    const int32_t q = base + gi;
    return q < end ? (uint32_t)__builtin_nontemporal_load(&a.indices[q]) * (uint32_t)kSlotBytes : 0u;
  };

  int r = wave * 8 + grp;  // this group's item inside the workgroup's stretch; batches of kWavesPerBlock * 8 items
  bool ok;
  int64_t row;
  int32_t beg, end;
  load_meta(r, ok, row, beg, end);
  uint32_t goff = load_ids(beg, end);
  for (;;) {
    const int rn = r + kWavesPerBlock * 8;
    const bool more = __builtin_amdgcn_readfirstlane(rn - grp) < a.rpb && item_base + (rn - grp) < item_stop;  // wave-uniform
    bool nok = false;
    int64_t nrow = 0;
    int32_t nbeg = 0, nend = 0;
    uint32_t ngoff = 0;
    if (more) {
      load_meta(rn, nok, nrow, nbeg, nend);
      ngoff = load_ids(nbeg, nend);
    }
    v4f prior0 = (v4f)(0.f), prior1 = (v4f)(0.f);
    if (a.accum && ok && row >= 0) {
      const float* op = a.out + row * (int64_t)a.ldo + gi * 8;
      prior0 = *reinterpret_cast<const v4f*>(op);
      prior1 = *reinterpret_cast<const v4f*>(op + 4);
    }
    int32_t cbase = beg;
    for (;;) {  // chunks of 8 edges; wave-uniform trip count (the longest item of the batch), per-group predicates inside
      const int cnt = (end - cbase) < 8 ? (end - cbase) : 8;
      for (int k = 0; k < 8; k += U) {
        if (__builtin_amdgcn_ballot_w64(k < cnt) == 0) break;
        v4f val[U];
        uint32_t roff[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const bool live = k + u < cnt;
          roff[u] = (uint32_t)__builtin_amdgcn_ds_bpermute((gbase + (live ? k + u : 0)) * 4, (int)goff);
          val[u] = (v4f)(0.f);
          if (live) val[u] = *reinterpret_cast<const v4f*>(slots + roff[u] + laneoff);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (k + u < cnt) {
            const uint32_t meta = (uint32_t)__float_as_int(val[u].x);
            if ((meta >> 24) != 255u) {
              const uint32_t c0 = meta & 0xffu, c1 = (meta >> 8) & 0xffu, c2 = (meta >> 16) & 0xffu;
              const float a0 = accg[c0], a1 = accg[c1], a2 = accg[c2];
              if (c0 < 64u) accg[c0] = a0 + val[u].y;
              if (c1 < 64u) accg[c1] = a1 + val[u].z;
              if (c2 < 64u) accg[c2] = a2 + val[u].w;
            } else {
              const uint32_t srow = roff[u] / (uint32_t)kSlotBytes;
              const float* dr = a.src + (size_t)srow * (size_t)a.lds + gi * 8;
              v4f d0 = *reinterpret_cast<const v4f*>(dr), d1 = *reinterpret_cast<const v4f*>(dr + 4);
              if (a.src_scale) {
                const float sc = a.src_scale[srow];
                d0 *= sc;
                d1 *= sc;
              }
              v4f* ar = reinterpret_cast<v4f*>(accg + gi * 8);
              ar[0] += d0;
              ar[1] += d1;
            }
          }
        }
      }
      cbase += 8;
      if (__builtin_amdgcn_ballot_w64(cbase < end) == 0) break;
      goff = load_ids(cbase, end);
    }
    {  // the group's accumulator row is the item's result: lane gi owns columns 8 gi .. 8 gi + 7
      v4f* ar = reinterpret_cast<v4f*>(accg + gi * 8);
      v4f r0 = ar[0], r1 = ar[1];
      ar[0] = (v4f)(0.f);
      ar[1] = (v4f)(0.f);
      if (gi == 0) accg[64] = 0.f;
      if (ok) {
        if (row >= 0) {
          if (a.mean) {
            const int deg = end - beg;
            r0 = r0 / (float)(deg > 1 ? deg : 1);
            r1 = r1 / (float)(deg > 1 ? deg : 1);
          }
          if (a.dst_scale) {
            const float ds = a.dst_scale[row];
            r0 *= ds;
            r1 *= ds;
          }
          if (a.accum) {
            r0 += prior0;
            r1 += prior1;
          }
          float* op = a.out + row * (int64_t)a.ldo + gi * 8;
          __builtin_nontemporal_store(r0, reinterpret_cast<v4f*>(op));
          __builtin_nontemporal_store(r1, reinterpret_cast<v4f*>(op + 4));
        } else {
          float* pp = a.partial + (-(row + 1)) * (int64_t)64 + gi * 8;
          *reinterpret_cast<v4f*>(pp) = r0;
          *reinterpret_cast<v4f*>(pp + 4) = r1;
        }
      }
    }
    if (!more) break;
    r = rn;
    ok = nok; row = nrow; beg = nbeg; end = nend; goff = ngoff;
  }
}

// x [n, 64] (row stride ld floats) -> slots [n, 32 x u32].  16 lanes x float4 per row, four rows per wave-instruction; a row's slot is
// assembled in LDS (byte writes for the columns) and leaves as one coalesced 128-byte store (slots.h).  *overflow += rows with more than
// 24 non-zeros.
__global__ __launch_bounds__(kBlock) void rows_slots_pack_kernel(int64_t n, const float* __restrict__ x, int64_t ld, const float* __restrict__ row_scale,
                                                                 uint32_t* __restrict__ slots, unsigned long long* __restrict__ overflow) {
  __shared__ uint32_t stage_all[kWavesPerBlock][4 * 32];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int sub = lane >> 4, l = lane & 15;
  const int64_t rows_per_pass = (int64_t)gridDim.x * kWavesPerBlock * 4;
  unsigned long long over_rows = 0;
  for (int64_t base = ((int64_t)blockIdx.x * kWavesPerBlock + wave) * 4; base < n; base += rows_per_pass) {
    const int64_t r = base + sub;
    v4f v = (v4f)(0.f);
    if (r < n) {
      v = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(x + r * ld + l * 4));
      if (row_scale) v *= row_scale[r];  // (a zero stays a zero; a non-zero times a factor that underflows to zero is dropped like one)
    }
    const bool over = slot_pack_rows4(v, sub, l, stage_all[wave], r < n ? slots + r * 32 : nullptr);
    over_rows += (unsigned long long)__popcll(__ballot(over && l == 0 && r < n));
  }
  if (overflow && lane == 0 && over_rows) atomicAdd(overflow, over_rows);
}

// the slots of the listed rows only (mgx_rows_slots_pack_rows): what rows_slots_pack_kernel writes for them, byte for byte; four listed rows
// per wave-instruction, a row id outside [0, n) is skipped
__global__ __launch_bounds__(kBlock) void rows_slots_pack_rows_kernel(int64_t n, int64_t nrows, const int64_t* __restrict__ rows, const float* __restrict__ x,
                                                                      int64_t ld, uint32_t* __restrict__ slots) {
  __shared__ uint32_t stage_all[kWavesPerBlock][4 * 32];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int sub = lane >> 4, l = lane & 15;
  const int64_t rows_per_pass = (int64_t)gridDim.x * kWavesPerBlock * 4;
  for (int64_t base = ((int64_t)blockIdx.x * kWavesPerBlock + wave) * 4; base < nrows; base += rows_per_pass) {
    int64_t r = -1;
    if (base + sub < nrows) r = rows[base + sub];
    const bool ok = r >= 0 && r < n;
    v4f v = (v4f)(0.f);
    if (ok) v = *reinterpret_cast<const v4f*>(x + r * ld + l * 4);
    slot_pack_rows4(v, sub, l, stage_all[wave], ok ? slots + r * 32 : nullptr);
  }
}

static bool spmm_slots_eligible(const SpmmFastArgs<int32_t>& a) {
  return a.D == 64 && a.lds % 4 == 0 && a.ldo >= 64 && !a.src_bits && !a.ragged &&
         a.src_rows * (int64_t)kSlotBytes < (int64_t(1) << 32) && a.src_rows * (int64_t)a.lds * 4 < (int64_t(1) << 32) &&
         (uintptr_t)a.src % 16 == 0;
}

// the items of `a` on the slot kernels: a whole schedule or the `rest` part of a two-part plan (a wave per item), or its head of short
// items (a.short_rows: a lane group per item)
static void launch_spmm_slots(SpmmFastArgs<int32_t> a, const void* slots, hipStream_t s) {
  if (a.init_pos) {  // mgx_spmm_copy_u_slots_init (its entry point checked; short items never come here: they carry no src_scale)
    static_assert(kItemsPerBlock <= 64 * kWavesPerBlock, "spmm_probe_init_kernel holds a wave's items one per lane");
    a.rpb = kItemsPerBlock;
    const dim3 grid((unsigned)xcd_ranges(a.plan, a.n_items, a.rpb, a.xcd));
    note_spmm_kernel("slots");
    hipLaunchKernelGGL(spmm_probe_init_kernel, grid, dim3(kBlock), 0, s, a, (const char*)slots);
    return;
  }
  if (a.short_rows) {
    a.rpb = 2 * kWavesPerBlock * 8;  // two batches per wave: the second's ids travel under the first's gathers
    const dim3 grid((unsigned)xcd_ranges(a.plan, a.n_items, a.rpb, a.xcd));
    note_spmm_kernel("slots");
    hipLaunchKernelGGL((spmm_slots_short_kernel<4>), grid, dim3(kBlock), 0, s, a, (const char*)slots);
    return;
  }
  a.rpb = kItemsPerBlock;
  const dim3 grid((unsigned)xcd_ranges(a.plan, a.n_items, a.rpb, a.xcd));
  note_spmm_kernel("slots");
  // 16 source rows per wave and step, two steps in flight (measured on the products graph, D = 64, 21 % non-zero, whole call incl. the
  // 0.34 ms lane-group part: U = 1 2.04 / 1.65 with ping-pong, U = 2 1.70 / 1.49, U = 3 - / 1.99, U = 4 1.55 / 1.93, U = 8 2.05 ms;
  // dense rows 2.15 ms -- experiments/exp_slots_tune.py)
  hipLaunchKernelGGL((spmm_slots_kernel<2, true>), grid, dim3(kBlock), 0, s, a, (const char*)slots);
}
