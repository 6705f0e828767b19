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
// matrix, `out` write-only) over slots -- for a gathered matrix most of whose ROWS are zero (d neigh / deg of a loss taken on 8 % of the
// nodes): an empty slot is one line per edge instead of the dense row's two and adds nothing.
//
// The sum has the dense INIT launch's bits, which fixes the order of additions: that kernel keeps four accumulators, edge e of an item
// (counted from the item's first edge) is added to accumulator e % 4 in increasing e, accumulator 0 starts from the initial value, and
// the result is (A0 + A1) + (A2 + A3).  Here the four accumulators are four LDS rows of the wave.  Lane group g of a step holds edge
// k + 8 u + g (k a multiple of 16), so groups g and g + 4 feed accumulator g & 3: the lower half of the wave adds first, then the upper
// half (a wave's LDS operations execute in order), u ascending.  An empty slot adds nothing -- eight empty slots skip the whole path,
// tested wave-uniformly --; a slot with values adds them at their columns by read - add - write; a flagged slot (more than 24
// non-zeros) adds the dense row.  A skipped addend is an exact +0.0f, so the result is the dense launch's bit for bit wherever no
// element of the operands is -0.0f, and equal as a number otherwise (only the sign of an exactly-zero result can differ).
//
// Schedule: spmm_slots_kernel's (two steps of 16 slots in ping-pong); the dense rows of a step's flagged slots are read where they are
// added, both halves' at once.  (Requesting them one step ahead -- a third stage, 108 - 138 VGPRs at U = 2, 70 at U = 1 -- was
// measured on the products graph with 8 % dense rows and lost to this form and to the dense launch: docs/LOG_head_slots.md.)
template <int U>
__global__ __launch_bounds__(kBlock) void spmm_slots_init_kernel(const SpmmFastArgs<int32_t> a, const char* __restrict__ slots) {
  __shared__ __attribute__((aligned(16))) float acc_all[kWavesPerBlock][4][kSlotAccStride];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int grp = lane >> 3, gi = lane & 7;
  float* accw = &acc_all[wave][0][0];
  float* accg = accw + (grp & 3) * kSlotAccStride;
  for (int i = lane; i < 4 * kSlotAccStride; i += kWave) accw[i] = 0.f;
  int64_t item_base, item_stop;
  xcd_stretch(a.xcd, item_base, item_stop);
  item_base += (int64_t)(blockIdx.x / kXcds) * a.rpb;
  int r = wave;
  if (r >= a.rpb || item_base + r >= item_stop) return;
  const uint32_t laneoff = (uint32_t)gi * 16u;
  const char* __restrict__ srcb = reinterpret_cast<const char*>(a.src);
  const uint32_t rowbytes = (uint32_t)a.lds * 4u;

  auto load_meta = [&](int64_t item, int64_t& row, int32_t& beg, int32_t& end, int32_t& ipos) {
    if (a.item_row) {
      row = (int64_t)a.item_row[item];
      beg = a.item_beg[item];
      end = a.item_end[item];
    } else {
      row = item;
      beg = a.indptr[item];
      end = a.indptr[item + 1];
    }
    ipos = row >= 0 ? (int32_t)a.init_pos[row] : -1;  // (a chunk of a split row starts from zero: its row's value enters in the fix-up)
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
      const bool live = k + u * 8 + grp < cnt;
      const uint32_t meta = (uint32_t)__float_as_int(val[u].x);
      const uint32_t c0 = meta & 0xffu, c1 = (meta >> 8) & 0xffu, c2 = (meta >> 16) & 0xffu;
      const bool dense = live && (meta >> 24) == 255u;
      const bool valued = live && !dense && c0 < 64u;  // (a lane's values fill c0 first)
      const uint64_t busy = __ballot(dense || valued);
      if (busy == 0) continue;  // eight empty slots: nothing to add
      v4f d0 = (v4f)(0.f), d1 = (v4f)(0.f);
      if (dense) {  // more than 24 non-zeros: the dense row, 8 columns per lane
        const char* dr = srcb + ((roff[u] / (uint32_t)kSlotBytes) * rowbytes + (uint32_t)gi * 32u);
        d0 = *reinterpret_cast<const v4f*>(dr);
        d1 = *reinterpret_cast<const v4f*>(dr + 16);
      }
#pragma unroll
      for (int half = 0; half < 2; ++half) {  // groups g before groups g + 4: the order of the additions to accumulator g & 3
        if (((busy >> (32 * half)) & 0xffffffffull) == 0) continue;
        if ((grp >> 2) == half) {
          if (valued) {
            const float a0 = accg[c0], a1 = accg[c1], a2 = accg[c2];  // (column 64 = the padding element of the accumulator row)
            accg[c0] = a0 + val[u].y;
            if (c1 < 64u) accg[c1] = a1 + val[u].z;
            if (c2 < 64u) accg[c2] = a2 + val[u].w;
          } else if (dense) {
            v4f* ar = reinterpret_cast<v4f*>(accg + gi * 8);
            ar[0] += d0;
            ar[1] += d1;
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
      }
    }
  };

  int64_t row;
  int32_t beg, end, ipos;
  load_meta(item_base + r, row, beg, end, ipos);
  uint32_t goff = load_ids(beg, end);
  for (;;) {
    // the initial value is requested before anything else of the item and enters accumulator 0 behind the first step's gathers
    float iv = 0.f;
    if (ipos >= 0) iv = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(a.init) + ((uint32_t)ipos * ((uint32_t)a.ldi * 4u) + (uint32_t)lane * 4u));
    const int rn = r + kWavesPerBlock;
    const bool has_next = rn < a.rpb && item_base + rn < item_stop;
    int64_t nrow = 0;
    int32_t nbeg = 0, nend = 0, nipos = -1;
    uint32_t ngoff = 0;
    if (has_next) {
      load_meta(item_base + rn, nrow, nbeg, nend, nipos);
      ngoff = load_ids(nbeg, nend);
    }
    for (int32_t cbase = beg; cbase < end; cbase += kWave) {
      if (cbase != beg) goff = load_ids(cbase, end);
      const int cnt = (end - cbase) < kWave ? (end - cbase) : kWave;
      v4f va[U], vb[U];
      uint32_t ra[U], rb[U];
      issue(0, cnt, goff, va, ra);
      if (cbase == beg) accw[lane] = iv;
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
    }
    float A[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      A[j] = accw[j * kSlotAccStride + lane];
      accw[j * kSlotAccStride + lane] = 0.f;
    }
    if (end <= beg) A[0] = iv;  // no edge: the initial value never reached the accumulator
    const float res = (A[0] + A[1]) + (A[2] + A[3]);
    if (row >= 0) __builtin_nontemporal_store(res, a.out + row * (int64_t)a.ldo + lane);
    else a.partial[(-(row + 1)) * (int64_t)64 + lane] = res;
    if (!has_next) break;
    r = rn;
    row = nrow; beg = nbeg; end = nend; ipos = nipos;
    goff = ngoff;
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
    a.rpb = kItemsPerBlock;
    const dim3 grid((unsigned)xcd_ranges(a.plan, a.n_items, a.rpb, a.xcd));
    note_spmm_kernel("slots");
    hipLaunchKernelGGL((spmm_slots_init_kernel<2>), grid, dim3(kBlock), 0, s, a, (const char*)slots);
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
