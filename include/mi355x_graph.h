/*
 * mi355x_graph.h -- C ABI of the MI355X (gfx950 / CDNA4) sparse message-passing library.
 *
 * This is the drop-in boundary for the one hot path of dglai/dgl-0.5-benchmark:
 * what DGLGraph.update_all(builtin, builtin) / apply_edges(builtin) / dgl.ops.gspmm /
 * dgl.ops.gsddmm / edge_softmax execute.  The reference itself is pure Python; the seam it
 * crosses is DGL v0.6.x's FFI pair
 *     _CAPI_DGLKernelSpMM (graph, op, reduce_op, U, E, V, ArgU, ArgE)
 *     _CAPI_DGLKernelSDDMM(graph, op, lhs, rhs, out, lhs_target, rhs_target)
 * (UPSTREAM src/array/kernel.cc, called from python/dgl/sparse.py::_gspmm/_gsddmm), reached
 * from the reference at
 *     kernel/dgl-new.py:20,39
 *     end_to_end/full_graph/node_classification/main_dgl_product_sage.py:62
 *     end_to_end/full_graph/node_classification/main_dgl_reddit_gat.py:10,31-55
 *     end_to_end/full_graph/node_classification/main_dgl_proteins_rgcn_for.py:52
 *     end_to_end/full_graph/graph_classification/main_dgl_molhiv_gcn.py:41-52,75
 * Each entry point below names the reference interface it replaces.
 *
 * Conventions (same as the upstream seam):
 *   - every pointer is a DEVICE pointer unless the name ends in `_host`; the CALLER allocates
 *     every output / arg-index / workspace buffer, the library never allocates or frees;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); all work is enqueued
 *     on it and the call returns without synchronising;
 *   - graph index arrays are int32 or int64 (`idx_bits`); element offsets are 64-bit inside;
 *   - features are dense row-major fp32 (`MGX_F32`), `*_len` = elements per row;
 *   - broadcasting ((N,H,F) op (E,H,1)) is expressed by optional device tables
 *     `*_off[out_len]` mapping an output element to the operand element (NULL = identity),
 *     the formulation of DGL's BcastOff;
 *   - every function returns MGX_OK (0) or an error code; mgx_last_error() gives the text
 *     (thread-local).  Nothing aborts the process.
 *
 * No torch types, no C++ types: plain pointers and sizes, bindable from ctypes / cgo / JNI.
 */
#ifndef MI355X_GRAPH_H_
#define MI355X_GRAPH_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  MGX_OK = 0,
  MGX_ERR_INVALID_ARGUMENT = 1,
  MGX_ERR_UNSUPPORTED = 2,
  MGX_ERR_HIP = 3
} mgx_status;

/* binary ops of kernel/utils.py:8-16 (binary_op_dict) */
typedef enum {
  MGX_OP_ADD = 0, MGX_OP_SUB = 1, MGX_OP_MUL = 2, MGX_OP_DIV = 3,
  MGX_OP_COPY_LHS = 4, MGX_OP_COPY_RHS = 5, MGX_OP_DOT = 6
} mgx_op;

/* reducers selectable with kernel/dgl-new.py:51 --spmm-reduce */
typedef enum { MGX_REDUCE_SUM = 0, MGX_REDUCE_MAX = 1, MGX_REDUCE_MIN = 2, MGX_REDUCE_MEAN = 3 } mgx_reduce;

/* flags of mgx_spmm_csr / mgx_spmm_copy_u_strided */
enum {
  MGX_SPMM_ACCUMULATE = 1, /* out += result (SUM / MEAN only) */
  MGX_SPMM_SHORT_ROWS = 2  /* the caller vouches that the work items (plan items, or rows without a plan) are SHORT AND EVEN: for every
                              batch of B = 64 / G consecutive items (G = lanes per feature row = next power of two >= D / 4) the longest is
                              not much above the batch mean.  copy_lhs / copy_rhs with SUM | MEAN then take the kernel that gives every
                              item a lane group of its own (2 - 3.5x on rows of ~3 edges); without the flag, or on skewed items, a wave per
                              item.  Items above 32 edges are taken by the whole wave inside that kernel, one after the other: keep them
                              (rows above 32 edges, the chunks of split rows) out of the way in the plan's `rest` part (mgx_spmm_plan),
                              or do not set the flag.  A hint: results are the same either way (other fp32 summation order). */
};

/* SDDMM operand targets (lhs_target / rhs_target of dgl.ops.gsddmm) */
typedef enum { MGX_TARGET_U = 0, MGX_TARGET_E = 1, MGX_TARGET_V = 2 } mgx_target;

/* A CSR view.  For message passing this is the IN-CSR ("CSC"): one row per destination node,
 * indices[p] = source node, eids[p] = id of the edge in the original COO (NULL = identity). */
typedef struct mgx_csr {
  int64_t num_rows;
  int64_t num_cols;
  int64_t nnz;
  const void* indptr;   /* [num_rows + 1] */
  const void* indices;  /* [nnz] */
  const void* eids;     /* [nnz] or NULL */
  int32_t idx_bits;     /* 32 or 64 */
  int32_t reserved;
} mgx_csr;

/* Optional execution schedule of a CSR for the summing g-SpMM (built once per graph, like the CSR
 * itself; mi355x_graph/schedule.py builds it).  Work items replace the natural row order:
 *   - items are walked in array order, 64 per workgroup, each XCD (own L2) taking a contiguous
 *     range -- a locality-aware order (rows of one community adjacent) turns gathers into L2 hits;
 *   - rows longer than the split threshold appear as several items (edge ranges) whose partial
 *     sums go to `partial_ws` slots and are combined in slot order by a fix-up launch, so a hub
 *     row never serialises on one wavefront and the result stays deterministic.
 * Every row must be covered exactly once (one direct item, or >= 2 slot items + a hub entry). */
typedef struct mgx_spmm_plan {
  int64_t num_items;
  const int32_t* item_row;  /* [num_items] >= 0: row written directly; < 0: partial slot -(v+1) */
  const void* item_beg;     /* [num_items] first edge position (graph index width) */
  const void* item_end;     /* [num_items] one past the last edge position */
  int64_t num_hubs;
  const int32_t* hub_row;       /* [num_hubs] rows that were split */
  const int32_t* hub_slot_ptr;  /* [num_hubs+1] slots of hub h are [ptr[h], ptr[h+1]) */
  int64_t num_slots;            /* partial_ws holds num_slots * out_len floats */
  const int32_t* slot_item;     /* [num_slots] index of the work item that owns each partial slot */
  const int32_t* item_node;     /* [num_items] the row of EVERY item (direct or split); used by mgx_sddmm_csr */
  /* Optional (HOST values): items [xcd_item_start[x], xcd_item_start[x+1]) are walked by XCD x.  Each XCD (own L2) gets a
   * CONTIGUOUS stretch of the schedule; equal item counts leave the XCDs unequal WORK on skewed graphs (R-MAT: 151 % vs 0.1 %
   * of the mean edge count), so the builder cuts the schedule at equal EDGE counts.  All zero: equal item counts.
   * xcd_item_start_dev: the same nine numbers in device memory (kernels read their two from there: a by-value array indexed
   * by blockIdx costs scalar registers and, through them, resident workgroups). */
  int64_t xcd_item_start[9];
  const int64_t* xcd_item_start_dev;
  /* Optional second part (NULL: this plan is the whole schedule).  With `rest`, THIS plan holds only short direct items (item_row >= 0,
   * at most 32 edges, no slots or hubs) and `rest` holds every other item with the hub tables; together they cover each row once.
   * Accepted by mgx_spmm_csr / mgx_spmm_copy_u_strided with MGX_SPMM_SHORT_ROWS for copy_lhs / copy_rhs with SUM | MEAN only: the short
   * items run on the lane-group kernel, `rest` on the wave-per-item kernel (partial_ws: rest->num_slots * out_len floats).  A hub row
   * of 13 k edges is 52 consecutive 256-edge chunks; walked by the lane-group kernel they would be one wave's serial tail. */
  const struct mgx_spmm_plan* rest;
} mgx_spmm_plan;

/* Device-side construction of the plan tables (hub-row splitting over an optional row order; NULL = natural order).
 *   ws      = mgx_spmm_plan_workspace(num_rows) bytes, passed UNCHANGED from _count to _fill (it carries the scans);
 *   _count  writes {num_items, num_hubs, num_slots} to `totals` (device int64[3]); the caller reads them, allocates
 *           item_row/item_node [num_items] (int32), item_beg/item_end [num_items] (graph index width),
 *           hub_row [num_hubs], hub_slot_ptr [num_hubs+1], slot_item [num_slots] (int32) and calls
 *   _fill   with the same csr / split / row_order.
 * The locality-aware row order itself is computed by the host layer (mi355x_graph/schedule.py). */
int64_t mgx_spmm_plan_workspace(int64_t num_rows);
int32_t mgx_spmm_plan_count(const mgx_csr* csr, int64_t split, const void* row_order, int64_t* totals,
                            void* workspace, int64_t workspace_bytes, void* stream);
int32_t mgx_spmm_plan_fill(const mgx_csr* csr, int64_t split, const void* row_order,
                           int32_t* item_row, void* item_beg, void* item_end, int32_t* item_node,
                           int32_t* hub_row, int32_t* hub_slot_ptr, int32_t* slot_item,
                           void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ misc */
const char* mgx_last_error(void);
/* ABI version, bumped on any signature change. */
int32_t mgx_abi_version(void);
/* Name of the kernel family the calling thread's last g-SpMM entry point launched ("rowwave32", "rowgroup32", "rowwave", "fast",
 * "generic", "tile"; "" before the first call): which of the schedules a CSR / width was routed to -- for tests and tuning. */
const char* mgx_last_spmm_kernel(void);
/* Fills *num_cus / *lds_bytes of the current HIP device; MGX_ERR_HIP when no GPU is usable. */
int32_t mgx_device_info(int32_t* num_cus, int32_t* lds_bytes_per_cu, char* arch_name, int32_t arch_name_len);

/* ------------------------------------------------------------------ g-SpMM
 * Replaces _CAPI_DGLKernelSpMM as reached by dgl.ops.gspmm (kernel/dgl-new.py:20) and
 * update_all(fn.copy_src, fn.mean) (main_dgl_product_sage.py:62), update_all(fn.u_mul_e, fn.sum)
 * (GATConv, main_dgl_reddit_gat.py:10; main_dgl_proteins_rgcn_for.py:52), update_all(udf, fn.sum)
 * -> copy_e/sum (main_dgl_molhiv_gcn.py:46).
 *
 *   out[v,k] = dst_scale[v] * REDUCE_{p in row v} op( src_scale[u] * U[u, u_off[k]], E[eid(p), e_off[k]] )
 *
 * op: ADD, MUL, COPY_LHS, COPY_RHS (callers rewrite SUB/DIV as ADD(-E)/MUL(1/E), as DGL does).
 * reduce: SUM, MEAN (sum / max(in_degree,1), the divide DGL performs after the kernel),
 *         MAX / MIN (empty rows give 0; arg_u/arg_e receive the winning source node / edge id,
 *         -1 for empty rows).  MAX / MIN walk a row in CSR storage order with a strict compare (> / <) that starts
 *         from the identity -inf / +inf: of several equal extrema the FIRST in storage order wins (for a CSR built
 *         stably from COO, the smallest edge id; +0.0 and -0.0 are equal), and the backward routes the whole gradient
 *         through that one arg.  A NaN term never wins.  A non-empty row whose terms never beat the identity -- all
 *         NaN, all -inf under MAX, all +inf under MIN -- gives the identity with arg_u = arg_e = -1.
 * src_scale / dst_scale: optional per-node fp32 factors (NULL = 1); used for the fused backward
 * of `mean` and for symmetric-norm GCN layers.  Only with SUM/MEAN.
 * arg_u/arg_e: same index width as the graph, [num_rows*out_len], may be NULL.
 * NULL offset table: identity when the operand row has out_len elements, otherwise head-wise
 * broadcast k -> k / (out_len / len)  (the (N,H,F) x (E,H,1) pattern of GATConv).
 * Deterministic: no atomics, fixed summation order for a given graph (and plan). */
int32_t mgx_spmm_csr(const mgx_csr* csr, const mgx_spmm_plan* plan /* may be NULL */,
                     int32_t op, int32_t reduce,
                     const float* ufeat, const float* efeat,
                     int64_t u_len, int64_t e_len, int64_t out_len,
                     const int64_t* u_off, const int64_t* e_off,
                     const float* src_scale, const float* dst_scale,
                     float* out, void* arg_u, void* arg_e,
                     float* partial_ws /* [plan->num_slots * out_len] or NULL */,
                     int32_t flags /* MGX_SPMM_ACCUMULATE: out += result (SUM/MEAN only) */, void* stream);

/* Row-sparse gathered matrix (round 2).  The gradient of a loss taken on a subset of the nodes (ogbn-products trains on 8 %,
 * main_dgl_product_sage.py:105-106) is zero in every other row, so the backward aggregation of the last layer gathers rows that
 * are 92 % zeros.  mgx_row_nonzero_bits flags the non-zero rows of x [n, D] (bit r of a ceil(n / 32)-word bitmap, n padded to 64
 * rows); mgx_spmm_copy_u_masked is mgx_spmm_csr(COPY_LHS, SUM | MEAN) that skips gathers of rows whose bit is clear -- the same
 * sum, fewer terms (exact: the skipped terms are zeros).  32-bit indices, D % 4 == 0, operands below 4 GiB, else
 * MGX_ERR_UNSUPPORTED (call mgx_spmm_csr).  plan / partial_ws / flags as for mgx_spmm_csr. */
int32_t mgx_row_nonzero_bits(int64_t n, int64_t D, const float* x, uint32_t* bits /* [2 * ceil(n / 64)] */, void* stream);
int32_t mgx_spmm_copy_u_masked(const mgx_csr* csr, const mgx_spmm_plan* plan /* may be NULL */, int32_t reduce,
                               const float* ufeat, int64_t D, const uint32_t* src_bits, const float* dst_scale /* may be NULL */,
                               float* out, float* partial_ws, int32_t flags, void* stream);

/* copy_u / sum | mean with STRIDED rows (round 2): ufeat rows are u_stride floats apart, out rows out_stride floats apart
 * (both >= D).  Lets the aggregation read and write column blocks of wider matrices in place -- SAGEConv
 * (main_dgl_product_sage.py:61-64) feeds `fc_self(h) + fc_neigh(neigh)`; with h and neigh as the two halves of one [N, 2 D]
 * matrix that is ONE GEMM against the stacked weights instead of two, and the backward aggregation accumulates straight
 * into the h-half of the gradient.  32-bit indices, D and both strides multiples of 4, 16-byte aligned pointers, gathered
 * matrix below 4 GiB; otherwise MGX_ERR_UNSUPPORTED (make the operands dense and call mgx_spmm_csr).  plan / partial_ws / flags
 * as for mgx_spmm_csr. */
int32_t mgx_spmm_copy_u_strided(const mgx_csr* csr, const mgx_spmm_plan* plan /* may be NULL */, int32_t reduce,
                                const float* ufeat, int64_t D, int64_t u_stride, const float* dst_scale /* may be NULL */,
                                float* out, int64_t out_stride, float* partial_ws, int32_t flags, void* stream);

/* mgx_spmm_copy_u_strided with MGX_SPMM_ACCUMULATE semantics whose INITIAL VALUE comes from a compact matrix instead of from `out`:
 *     out[v, :] = (init_pos[v] >= 0 ? init[init_pos[v], :] : +0.0f) + SUM_{u -> v} ufeat[u, :]
 * The backward of a layer whose loss reads R of N rows (main_dgl_product_sage.py:105-106) has d self as a compact [R, D] matrix; the
 * accumulating launch wanted it scattered into a zero-filled [N, D] first -- a fill, a copy and a read of N rows of which 92 % are the
 * zeros just written.  Here `out` is WRITE-ONLY and every row of it is written (rows without in-edges with their initial value); the
 * value enters the arithmetic exactly where the accumulated value enters in mgx_spmm_copy_u_strided -- a row outside the list goes
 * through the same add with +0.0f, so a sum of -0.0f still ends as +0.0f -- and the result is bit for bit that of
 *     zeros [N, D]; rows listed by init_pos copied from init; mgx_spmm_copy_u_strided(..., MGX_SPMM_ACCUMULATE)
 * on the same graph and plan (two-part plans and split rows included: a split row's value enters in the fix-up).
 *   init      fp32 [R, D] (R = init_rows), rows init_stride floats apart (a multiple of 4, >= D), 16-byte aligned; NULL only with R = 0
 *   init_pos  int64 [num_rows]: the row of `init` a destination row starts from, or -1.  The entries MUST be -1 or in [0, R): the
 *             kernels follow them unchecked (an entry outside is a read outside `init`).  Two rows may name the same row of `init`.
 * reduce = MGX_REDUCE_SUM, dst_scale = NULL, int32 graph, D and the three strides multiples of 4, 16-byte aligned pointers, gathered
 * and initial matrix below 4 GiB each; anything else (MEAN, a dst_scale, D = 62, an int64 graph) returns MGX_ERR_UNSUPPORTED and the caller keeps the
 * sequence above.  flags: MGX_SPMM_SHORT_ROWS only (accumulation is implied).  plan / partial_ws as for mgx_spmm_csr.
 * Deterministic: no atomics.  Purely additive: mgx_abi_version() stays 35. */
int32_t mgx_spmm_copy_u_strided_init(const mgx_csr* csr, const mgx_spmm_plan* plan /* may be NULL */, int32_t reduce, const float* ufeat,
                                     int64_t D, int64_t u_stride, const float* dst_scale /* must be NULL */, const float* init,
                                     int64_t init_rows /* R */, int64_t init_stride, const int64_t* init_pos, float* out,
                                     int64_t out_stride, float* partial_ws, int32_t flags, void* stream);

/* copy_u / sum | mean of a CONSTANT matrix of exactly 100 columns (round 5; csrc/spmm_tail.inc) -- the layer-1 aggregation of
 * ogbn-products' input features (main_dgl_product_sage.py:61-62), the largest launch of the epoch.  The row kernel's time is the number of
 * cache-line requests per edge, and a 400-byte row costs a fourth (4.125 on average) for its last 16 bytes.  The features never change, so
 * they are laid out ONCE as
 *     block_a    [num_cols, 96]  columns 0 .. 95, compact: 384-byte rows = three lines each (128-byte aligned)
 *     edge_tail  [nnz, 4]        edge_tail[p] = x[indices[p], 96 .. 99] for every stored position p of the CSR (mgx_edge_tail_fill)
 * and the lane that streams position p's id reads edge_tail[p] in the same coalesced pass: three gathered lines per edge + a 16-byte
 * stream.  out: [num_rows, 100] (row stride out_stride), columns 0 .. 95 bit-identical to mgx_spmm_copy_u_strided of x, 96 .. 99 equal
 * to fp32 rounding (another order of additions).  The tail belongs to ONE CSR (its position order) and ONE x.
 * int32 graphs, one schedule (no two-part plan, no MGX_SPMM_SHORT_ROWS), block_a below 4 GiB; otherwise MGX_ERR_UNSUPPORTED. */
int32_t mgx_edge_tail_fill(const mgx_csr* csr, const float* x /* [num_cols, 100] */, int64_t x_stride, float* edge_tail /* [nnz, 4] */,
                           void* stream);
int32_t mgx_spmm_copy_u_edge_tail(const mgx_csr* csr, const mgx_spmm_plan* plan /* may be NULL */, int32_t reduce, const float* block_a,
                                  const float* edge_tail, const float* dst_scale /* may be NULL */, float* out, int64_t out_stride,
                                  float* partial_ws, int32_t flags, void* stream);

/* copy_u / sum | mean over MOSTLY-ZERO rows of exactly 64 columns (round 5; csrc/spmm_slots.inc) -- the input of a hidden GraphSAGE
 * layer is dropout(relu(.)) (main_dgl_product_sage.py:93-96; 20-25 % non-zero on the benchmark model), and the wave-per-item g-SpMM is
 * bound by the bytes of the gathered rows (L2 -> CU).  mgx_rows_slots_pack turns x [n, 64] into one 128-BYTE SLOT per row:
 *     8 x { meta, v0, v1, v2 } (uint32, float, float, float), meta = c0 | c1 << 8 | c2 << 16 | flag << 24
 *     the row's non-zero values in increasing order of (column % 4) * 16 + column / 4 -- the (component, lane) order of a 16-lane x float4
 *     read --, three per group, c = their columns, 64 = no value (the value word is 0); at most 24 per row; a row with MORE has
 *     flag = 255 in all eight metas (columns 64, values 0): the consumer reads the dense row instead.  *overflow_rows (device, may be
 *     NULL) += the number of such rows.
 *     row_scale (may be NULL): the slots hold row_scale[r] * x[r, :] (the dense matrix is left as it is).
 * mgx_spmm_copy_u_slots is mgx_spmm_copy_u_strided with the slots beside the dense matrix (same rows: slots = pack(ufeat, src_scale)):
 * every work item gathers ONE cache line per edge and adds its values at their columns -- per lane group of 8 lanes a 64-float
 * accumulator row in LDS, updated by plain read - add - write in a fixed order; a wave per item (a whole schedule, the `rest` part of a
 * two-part plan: the eight rows are summed at the end) or a lane group per item (MGX_SPMM_SHORT_ROWS, the head of a two-part plan).
 *     out[v] (+)= dst_scale[v] * SUM | MEAN_{u -> v} src_scale[u] * ufeat[u, :]
 * src_scale (may be NULL) must be the row_scale the slots were packed with: the kernel applies it only to the rows it reads from ufeat
 * (those above 24 non-zeros).  The reversed aggregation of a mean layer is of this form: A^T (D^-1 dy) with dy the gradient behind a
 * relu + dropout.  Exact (values are moved, never rounded; the products by row_scale are the ones the dense kernels form); the order of
 * additions inside a row differs from the dense kernels', so results agree to fp32 rounding, not bit for bit.  products-shaped graph,
 * D = 64, 21 % non-zero: 2.15 -> 1.49 ms per call.
 * int32 graphs, 16-byte aligned operands below 4 GiB (and fewer than 2^25 source rows); otherwise MGX_ERR_UNSUPPORTED. */
int32_t mgx_rows_slots_pack(int64_t n, int64_t D /* 64 */, const float* x, int64_t x_stride, const float* row_scale /* [n] or NULL */,
                            void* slots /* [n, 128 bytes] */, int64_t* overflow_rows /* device, may be NULL */, void* stream);
int32_t mgx_spmm_copy_u_slots(const mgx_csr* csr, const mgx_spmm_plan* plan /* may be NULL */, int32_t reduce, const float* ufeat,
                              int64_t D /* 64 */, int64_t u_stride, const void* slots, const float* src_scale /* may be NULL */,
                              const float* dst_scale /* may be NULL */, float* out, int64_t out_stride, float* partial_ws, int32_t flags,
                              void* stream);

/* mgx_spmm_copy_u_slots_init is mgx_spmm_copy_u_strided_init with the slots beside the dense matrix (slots = pack(ufeat), no factor),
 * for a gathered matrix most of whose ROWS are zero -- d neigh / deg of a loss taken on 8 % of the nodes:
 *     out[v] = (init[init_pos[v]] where init_pos[v] >= 0, else +0.0f) + SUM_{u -> v} ufeat[u, :]          (`out` is write-only)
 * A wave-per-item work item uses the slots as a per-edge PROBE: it fetches the first word of every source row's slot (one line per
 * edge) and gathers the dense row of `ufeat` for the rows whose slot holds a value or the flag; a row whose slot is empty costs its
 * probe only.  The additions per output element are made in the order of the dense call -- four accumulators, edge e of an item to
 * accumulator e % 4, the initial value first in accumulator 0, (A0 + A1) + (A2 + A3); a live row is added whole -- and a skipped
 * addend is an exact +0.0f, so the result is that of mgx_spmm_copy_u_strided_init on the same graph and plan
 *     bit for bit wherever no element of `ufeat` and `init` is -0.0f;
 *     equal as numbers otherwise (mgx_rows_slots_pack drops a -0.0f, so a row of nothing but zeros of either sign is skipped): only the
 *     sign of an exactly-zero result can differ.
 * The short items of a two-part plan (MGX_SPMM_SHORT_ROWS) read the dense rows, as in mgx_spmm_copy_u_slots without a factor.
 * reduce = MGX_REDUCE_SUM, dst_scale = NULL, int32 graph, D = 64, fewer than 2^25 source rows, and the alignment / stride / size
 * conditions of the two entries it combines; anything else returns MGX_ERR_UNSUPPORTED before a launch.
 * mgx_rows_slots_pack_rows writes the slots of the listed rows only -- rows int64 [num_listed], distinct, in [0, n) (an id outside is
 * skipped) -- byte for byte what mgx_rows_slots_pack writes for them; every other slot is left as it is.
 * Deterministic: no atomics.  Purely additive: mgx_abi_version() stays 35. */
int32_t mgx_rows_slots_pack_rows(int64_t n, int64_t D /* 64 */, const float* x, int64_t x_stride, const int64_t* rows, int64_t num_listed,
                                 void* slots /* [n, 128 bytes] */, void* stream);
int32_t mgx_spmm_copy_u_slots_init(const mgx_csr* csr, const mgx_spmm_plan* plan /* may be NULL */, int32_t reduce, const float* ufeat,
                                   int64_t D /* 64 */, int64_t u_stride, const void* slots, const float* dst_scale /* must be NULL */,
                                   const float* init, int64_t init_rows /* R */, int64_t init_stride, const int64_t* init_pos, float* out,
                                   int64_t out_stride, float* partial_ws, int32_t flags, void* stream);

/* LDS-staged copy_u / sum | mean for DENSE neighbourhoods (round 3; csrc/spmm_tile.hip).  On graphs with hundreds of in-edges
 * per node (reddit, proteins: kernel/dgl-new.py:61; main_dgl_reddit_sage.py:73-80) destination rows scheduled next to each other
 * share most of their sources; a TILE of consumers * nacc * 4 work items of the schedule is aggregated by one workgroup of
 * consumers + loaders = 16 waves (one per CU) or 8 waves (two per CU) that gathers each of the tile's re-used sources ONCE from L2 into LDS (chunks of 127 rows x 64 columns, LDS-DMA,
 * 4-deep ring, `loaders` loader waves) and serves every edge into it from LDS; sources used once in the tile are gathered
 * directly.  The tables below replace the graph arrays inside the kernel (built once per CSR by the host layer,
 * mi355x_graph/tileplan.py; all device memory, caller-owned):
 *   tile_chunk_ptr [num_tiles+1]            chunks of tile t are [ptr[t], ptr[t+1])
 *   chunk_ids      [num_chunks*128]         source row of every LDS slot, -1 = all-zero row (slot 127 always)
 *   lds_off        [num_tiles*consumers+1]  first superstep of the stream of (tile, consumer wave): its chunks, then rows j
 *   lds_cnt        [num_chunks*consumers*16] uint16 supersteps (4 steps each) of (chunk, wave, accumulator j < nacc)
 *   lds_stream     [(lds_steps+128)*4]       per superstep and lane group one dword = the LDS slots of its four steps
 *                                           (127 = zero row); 128 supersteps of padding behind the end (prefetch)
 *   dir_off        [num_tiles*consumers+1]  the same for the direct part; dir_cnt int32 [num_tiles*consumers*16];
 *   dir_stream     [(dir_steps+128)*16]      per superstep and lane group four source ids, -1 = padding
 *   tile_item      [num_tiles*R]            item_row of the work item at every (wave, j, lane group), INT32_MIN = none
 *   zero_row       [64] floats of zeros
 *   tile_order     [num_tiles] or NULL: the tile each dispatch slot runs (the builder puts an XCD's longest tiles first)
 * Work items are those of `plan` (hub rows stay split: partial_ws / fix-up as for mgx_spmm_csr; plan may be NULL when the tile
 * plan was built over natural rows).  32-bit indices, D and both strides multiples of 4, 16-byte aligned operands, gathered
 * matrix below 4 GiB; otherwise MGX_ERR_UNSUPPORTED (call mgx_spmm_csr).  Deterministic: no atomics. */
typedef struct mgx_tile_plan {
  int64_t num_tiles, num_chunks, lds_steps, dir_steps; /* steps: supersteps without the padding */
  int32_t consumers, nacc, loaders, lanes_log2; /* lanes per row: 0 | 4 = 16 lanes (64-column passes), 3 = 8 (32), 2 = 4 (16): narrow rows,
                                                    256 slots per chunk, consumers = 7, loaders = 1 */
  const int32_t* tile_chunk_ptr;
  const int32_t* chunk_ids;
  const int32_t* lds_off;
  const uint16_t* lds_cnt;
  const uint32_t* lds_stream;
  const int32_t* dir_off;
  const int32_t* dir_cnt;
  const int32_t* dir_stream;
  const int32_t* tile_item;
  const float* zero_row;
  const int32_t* tile_order; /* optional [num_tiles]: dispatch slot -> tile; slots [x * ceil(T/8), ...) run on XCD x in order */
  const int32_t* tile_node; /* optional [num_tiles*R]: the NODE of the item at every position (hub chunks: their row); mgx_gat_tile_* */
  const uint32_t* lds_stream16; /* optional, mgx_gat_tile_* with drop_p > 0: lds_stream with 16-bit entries, slot | rank << 8, rank = the
                                   edge's rank among the parallel edges of its (row, source) pair by edge id, mod 128; such a plan's
                                   dir_stream carries the rank in bits 24-30 of every source id (sources < 2^24) */
} mgx_tile_plan;
int32_t mgx_spmm_tile_copy_u(const mgx_csr* csr, const mgx_spmm_plan* plan /* may be NULL */, const mgx_tile_plan* tile_plan,
                             int32_t reduce, const float* ufeat, int64_t D, int64_t u_stride, const float* dst_scale /* may be NULL */,
                             float* out, int64_t out_stride, float* partial_ws, int32_t flags, void* stream);

/* Multi-relation g-SpMM (csrc/spmm_rel.hip): ALL R relations of an edge-weight matrix in one walk of the graph -- the edge-weighted
 * relational layer of main_dgl_proteins_rgcn_for.py:46-60, which the reference runs as R update_all(fn.u_mul_e, fn.mean) calls with
 * [E, 1] weight columns.
 *
 *   mgx_spmm_rel       out[v, r, d] = dst_scale[v] * SUM | MEAN_{p in row v} w[p, r] * src_scale[u_p] * x[u_p, d]      r < R, d < D
 *   mgx_spmm_rel_grad  dx[u, d]     = src_scale[u] * SUM_{p in row u} SUM_r w[p, r] * dst_scale[v_p] * dz[v_p, r, d]
 *
 * w: [nnz, R] fp32 in the POSITION order of the CSR passed (NOT by edge id: permute once with mgx_gather_rows(idx = csr->eids, D = R));
 * csr->eids is not read.  x: [num_cols, D] rows x_stride floats apart; out: [num_rows, R * D] dense.  MEAN divides by max(in_degree, 1),
 * empty rows give 0.  mgx_spmm_rel_grad is the gradient with respect to x: `csr` is the TRANSPOSED CSR (rows = source nodes u, indices =
 * destination nodes v_p) with w in THAT CSR's position order, dz: [num_cols, R * D] dense, dx: [num_rows, D] dense; the 1 / deg of a MEAN
 * forward goes into dst_scale.  src_scale / dst_scale: optional per-node factors (NULL = 1), indexed by source / destination node in both
 * entries.  plan / partial_ws as for mgx_spmm_csr (one schedule, no `rest` part; partial_ws: plan->num_slots * R * D floats forward,
 * plan->num_slots * D reverse).  int32 and int64 graphs; offsets into w are 64-bit.  Deterministic: no atomics, fixed summation order
 * for a given graph, plan, R and D.  1 <= R <= 16 and D in {1, 2, 4, ..., 128}, operands of D >= 4 16-byte aligned with x_stride % 4
 * == 0 (D = 2: 8 bytes, even stride); otherwise MGX_ERR_UNSUPPORTED (call mgx_spmm_csr per relation, or with the (N, 1, D) x (E, R, 1)
 * broadcast).  mgx_last_spmm_kernel(): "rel" / "rel_grad". */
int32_t mgx_spmm_rel(const mgx_csr* csr, const mgx_spmm_plan* plan /* may be NULL */, int32_t reduce, int64_t R, int64_t D,
                     const float* w, const float* x, int64_t x_stride, const float* src_scale, const float* dst_scale, float* out,
                     float* partial_ws, void* stream);
int32_t mgx_spmm_rel_grad(const mgx_csr* csr, const mgx_spmm_plan* plan /* may be NULL */, int64_t R, int64_t D, const float* w,
                          const float* dz, const float* dst_scale, const float* src_scale, float* dx, float* partial_ws, void* stream);

/* ------------------------------------------------------------------ g-SDDMM
 * Replaces _CAPI_DGLKernelSDDMM as reached by dgl.ops.gsddmm (kernel/dgl-new.py:39),
 * apply_edges(fn.u_add_v) inside GATConv (main_dgl_reddit_gat.py:10) and fn.u_dot_v
 * (link_prediction/gcmc_dgl/model.py:342).
 *
 *   out[e,k] = op( L[t_l(e), l_off[k]], R[t_r(e), r_off[k]] ),   e = edge id
 *   DOT: out[e,k] = sum_{j<reduce_size} L[.., l_off[k]*reduce_size+j] * R[.., r_off[k]*reduce_size+j]
 *
 * COO form: src/dst are [nnz] in edge-id order. */
int32_t mgx_sddmm_coo(int64_t num_src, int64_t num_dst, int64_t nnz,
                      const void* src, const void* dst, int32_t idx_bits,
                      int32_t op, const float* lhs, const float* rhs,
                      int32_t lhs_target, int32_t rhs_target,
                      int64_t l_len, int64_t r_len, int64_t out_len, int64_t reduce_size,
                      const int64_t* l_off, const int64_t* r_off,
                      float* out, void* stream);

/* The same walk over an edge list kept in ANOTHER order than the edge ids (round 5): src / dst give the q-th WALKED edge, perm[q] its
 * edge id = the output row.  For graphs that hold an in-CSR beside (or instead of) their COO: walked in the CSR's order -- sorted by
 * destination -- one operand row of consecutive edges is the same row and the other has the g-SpMM's locality, whole output rows are
 * scattered by edge id.  int32 ids, element-wise op (no DOT) on u / v operands [rows, feat_len] below 4 GiB each, else
 * MGX_ERR_UNSUPPORTED (call mgx_sddmm_coo / mgx_sddmm_csr).  Same values as mgx_sddmm_coo bit for bit. */
int32_t mgx_sddmm_coo_perm(int64_t num_src, int64_t num_dst, int64_t nnz, const void* src, const void* dst, const void* perm,
                           int32_t idx_bits, int32_t op, const float* lhs, const float* rhs, int32_t lhs_target, int32_t rhs_target,
                           int64_t feat_len, float* out, void* stream);
/* CSR form (graphs restricted to formats(['csr','csc']), main_dgl_product_sage.py:158): walks
 * the in-CSR, t(e)=V is the row, t(e)=U is indices[p], output still addressed by edge id. */
int32_t mgx_sddmm_csr(const mgx_csr* csr, const mgx_spmm_plan* plan /* may be NULL */,
                      int32_t op, const float* lhs, const float* rhs,
                      int32_t lhs_target, int32_t rhs_target,
                      int64_t l_len, int64_t r_len, int64_t out_len, int64_t reduce_size,
                      const int64_t* l_off, const int64_t* r_off,
                      float* out, void* stream);

/* ------------------------------------------------------------------ edge softmax
 * Replaces dgl.nn.functional.edge_softmax(graph, logits) (norm_by='dst') as called by GATConv
 * (main_dgl_reddit_gat.py:31-55).  DGL 0.6 runs 2 SpMM + 2 SDDMM + exp; here one fused
 * row-segmented kernel.  z, a, da, dz: [nnz, H] addressed by edge id.
 *   With a plan, split (hub) rows are handled as chunks (statistics, combine, normalise) and `ws` must
 *   hold (plan->num_slots + plan->num_hubs) * 2 * H floats; without a plan ws may be NULL.
 *   fwd: a[e,h]  = exp(z[e,h]-max_v) / sum_{e'->v} exp(z[e',h]-max_v)
 *   bwd: dz[e,h] = a*da - a * sum_{e'->v}(a*da)                                            */
int32_t mgx_edge_softmax_fwd(const mgx_csr* csr, const mgx_spmm_plan* plan /* may be NULL */, int64_t H,
                             const float* z, float* a, float* ws, void* stream);
int32_t mgx_edge_softmax_bwd(const mgx_csr* csr, const mgx_spmm_plan* plan /* may be NULL */, int64_t H,
                             const float* a, const float* da, float* dz, float* ws, void* stream);

/* GAT attention with the logits fused in (GATConv, main_dgl_reddit_gat.py:31-55):
 *   fwd: a[e,h]  = softmax_{e->v}( leaky_relu(el[u(e),h] + er[v(e),h], negative_slope) )
 *        = apply_edges(fn.u_add_v) -> leaky_relu -> edge_softmax in ONE launch; the [nnz, H] logits are never written.
 *   bwd: de[e,h] = (a*da - a*sum_{e'->v}(a*da)) * leaky_relu'(el[u]+er[v])   (gradient w.r.t. the pre-activation sum;
 *        the caller reduces it over out-edges / in-edges with copy_e g-SpMMs to get d el / d er).
 * el: [num_cols, H], er: [num_rows, H]; a, da, de: [nnz, H] by edge id.  plan / ws as for mgx_edge_softmax_*. */
int32_t mgx_gat_attention_fwd(const mgx_csr* csr, const mgx_spmm_plan* plan /* may be NULL */, int64_t H,
                              const float* el, const float* er, float negative_slope, float* a, float* ws, void* stream);
int32_t mgx_gat_attention_bwd(const mgx_csr* csr, const mgx_spmm_plan* plan /* may be NULL */, int64_t H,
                              const float* el, const float* er, float negative_slope,
                              const float* a, const float* da, float* de, float* ws, void* stream);

/* One GAT layer's message passing with NO E-sized tensor (GATConv between its projection and its bias,
 * main_dgl_reddit_gat.py:10,31-55: apply_edges(fn.u_add_v) -> leaky_relu -> edge_softmax -> attn_drop ->
 * update_all(fn.u_mul_e, fn.sum)):
 *   fwd: out[v,h,:] = sum_{e:(u->v)} keep(e,h)/(1-p) * a[e,h] * feat[u,h,:],  a = softmax_{e->v}(leaky_relu(el[u,h] + er[v,h]))
 *        nstat[v,h,0..3] = (er, row max, 1 / row sum, -) is what the backward rebuilds a[e,h] from; `a` is never written.
 *   bwd: d_er[v,h], then d_feat[u,h,:] and d_el[u,h] (both or neither); `csc` is the in-CSR the forward ran on, `csr` its
 *        transpose (rows = source nodes) whose eids map to the in-CSR's edge ids (NULL eids = positions) so that both walks
 *        regenerate the same dropout bit for an edge; nstat[.,.,3] receives t = <out, d_out> per head.
 * feat [num_cols, H*F], el [num_cols, H], er [num_rows, H], out / d_out [num_rows, H*F], nstat [num_rows, H, 4], 16-byte
 * aligned; F in {4, 8, ..., 256} with H*F <= 256, or ONE head of any width 4 < F <= 256 (e.g. a 41-class output layer: rows moved
 * in dword-aligned 16-byte windows); 32-bit indices (else MGX_ERR_UNSUPPORTED: callers fall back to mgx_gat_attention_* +
 * mgx_spmm_csr).  keep(e,h) = hash(seed, edge id e, head h) >= p * 2^32 (counter based; drop_p = 0: no mask), e = eids[q] of
 * CSR position q, or q itself when eids is NULL; the hash is a 32-bit mixer of the two key words (gat_hash in csrc/gatfused.hip).
 * workspace: max over the plans passed of mgx_gat_fused_workspace(plan, H, F) bytes (NULL when no plan splits rows).
 * pack_ws (may be NULL): mgx_gat_fused_pack_workspace(num_src, num_dst, H, F) bytes of scratch; when given and the layer is
 *   narrow enough that a node's feature row and its per-head attention terms fit the row's 128-byte lines (one head of
 *   16 or 41 features: yes; 8 x 16: no, the function returns 0), the gathered operands are first packed into rows
 *   [feat | el] (forward, backward destination walk) and [d_out | er, m, 1/s, t] (backward source walk), so that an edge
 *   costs one L2 request instead of two -- these walks are bound by requests, not bytes.  Same results bit for bit.
 * attn_l (may be NULL; round 3): when el IS (feat * attn_l).sum(-1) -- GATConv's own definition -- pass attn_l [H, F] as well:
 *   layers whose rows are not packed (several heads, H*F >= 64: the 8 x 16 layers) then form el[u,h] from the gathered feature
 *   row inside the kernels (4 multiply-adds and a lane swap or two per edge) instead of gathering it -- one L2 request per edge
 *   less; the `el` array is then only differentiated (d_el), not read.  Pass the same attn_l to the backward.
 * Deterministic: no atomics, hub partial sums combined in slot order. */
int64_t mgx_gat_fused_workspace(const mgx_spmm_plan* plan /* may be NULL */, int64_t H, int64_t F);
int64_t mgx_gat_fused_pack_workspace(int64_t num_src, int64_t num_dst, int64_t H, int64_t F);
int32_t mgx_gat_fused_fwd(const mgx_csr* csr, const mgx_spmm_plan* plan /* may be NULL */, int64_t H, int64_t F,
                          const float* feat, const float* el, const float* attn_l /* [H, F] or NULL */, const float* er,
                          float negative_slope, float drop_p, uint64_t seed, float* out, float* nstat, void* workspace,
                          void* pack_ws, void* stream);
int32_t mgx_gat_fused_bwd(const mgx_csr* csc, const mgx_spmm_plan* csc_plan /* may be NULL */, const mgx_csr* csr,
                          const mgx_spmm_plan* csr_plan /* may be NULL */, int64_t H, int64_t F, const float* feat,
                          const float* el, const float* attn_l /* [H, F] or NULL: as passed to the forward */, float negative_slope,
                          float drop_p, uint64_t seed, const float* out, const float* d_out, float* nstat,
                          float* d_feat /* may be NULL with d_el */, float* d_el, float* d_er, void* workspace, void* pack_ws,
                          void* stream);

/* The same three walks over a TILE plan (csrc/gat_tile.inc): one head of 4, 8, 12 or 16 columns on a graph with dense
 * neighbourhoods (main_dgl_reddit_gat.py on reddit).  `tile_plan`: 4 lanes per row (lanes_log2 = 2), 7 + 1 waves, nacc 3 or 4, with
 * tile_node; `plan`: the tile plan's base plan (its hub tables; workspace = mgx_gat_fused_workspace(plan, 1, F)).  Same arguments,
 * results and statistics as mgx_gat_fused_fwd / _bwd, another fp32 summation order (deterministic for a given plan).  attn_drop:
 * the mask bit of an edge is a function of (seed, destination, source, rank among parallel edges) here -- of (seed, edge id) in
 * the row kernels --: use the tile form for all three walks of a layer or for none when drop_p > 0; it needs lds_stream16 in both
 * plans.  Sources below 2^24 (the direct stream's ids are masked to 24 bits).  Other shapes: MGX_ERR_UNSUPPORTED. */
int32_t mgx_gat_tile_fwd(const mgx_csr* csr, const mgx_spmm_plan* plan, const mgx_tile_plan* tile_plan, int64_t H, int64_t F,
                         const float* feat, const float* el, const float* er, float negative_slope, float drop_p, uint64_t seed,
                         float* out, float* nstat, void* workspace, void* pack_ws, void* stream);
int32_t mgx_gat_tile_bwd(const mgx_csr* csc, const mgx_spmm_plan* csc_plan, const mgx_tile_plan* csc_tile_plan, const mgx_csr* csr,
                         const mgx_spmm_plan* csr_plan, const mgx_tile_plan* csr_tile_plan, int64_t H, int64_t F, const float* feat,
                         const float* el, float negative_slope, float drop_p, uint64_t seed, const float* out, const float* d_out,
                         float* nstat, float* d_feat /* may be NULL with d_el */, float* d_el, float* d_er, void* workspace,
                         void* pack_ws, void* stream);

/* Scaled dot-product attention over a graph with NO E-sized tensor (dgl.nn.DotGatConv between its projection and its result:
 * apply_edges(fn.u_dot_v) -> edge_softmax -> update_all(fn.u_mul_e, fn.sum); csrc/dotattn.hip):
 *   z[e,h]     = scale * sum_f q[dst(e),h,f] * k[src(e),h,f]          (scale applied once, after the sum)
 *   a[e,h]     = exp(z[e,h] - m[v,h]) / s[v,h],   m, s = max and sum over the in-edges of v = dst(e)
 *   out[v,h,:] = sum_{e: u->v} a[e,h] * v[u,h,:]                      (exactly 0 for a destination without in-edges)
 *   fwd: writes out and stat[v,h,0..3] = (m, 1/s, -, -), from which the backward rebuilds a[e,h]; `a` is never written.
 *   bwd: with t[v,h] = <out[v,h,:], d_out[v,h,:]> (written to stat[v,h,2]), dp[e,h] = <v[u,h,:], d_out[v,h,:]> and
 *        ds = a * (dp - t) * scale:   dq[v] = sum_e ds * k[u],   dk[u] = sum_e ds * q[v],   dv[u] = sum_e a * d_out[v].
 *        `csc` is the in-CSR the forward ran on, `csr` its transpose (rows = source nodes).  dq, dk, dv may each be NULL.
 * q [num_rows, q_ld], k [num_cols, k_ld], v [num_cols, v_ld]: the first H*F floats of a row are the operand; every row stride is
 * a multiple of 4 floats, at least H*F, with a 16-byte aligned base -- so q, k and v may be column blocks of one [N, 3*H*F]
 * projection.  k == v with k_ld == v_ld: the row is gathered once.  out, d_out, dq [num_rows, H*F], dk, dv [num_cols, H*F],
 * stat [num_rows, H, 4]: dense, 16-byte aligned, allocated by the caller.
 * Supported (mgx_dot_attention_supported; everything else is MGX_ERR_UNSUPPORTED and the caller composes mgx_sddmm_*,
 * mgx_edge_softmax_* and mgx_spmm_csr): F in {4, 8, 16, 32, 64}, H >= 1, H*F <= 256, 32-bit indices, nnz > 0, and
 * max(num_rows, num_cols) * H * max(4 F, 16) below 4 GiB (32-bit byte offsets: the dense operands and stat).  A strided q, k or v
 * whose rows * row stride * 4 reaches 4 GiB is MGX_ERR_UNSUPPORTED too: pass a dense copy.
 * workspace: max over the plans passed of mgx_dot_attention_workspace(plan, H, F) bytes (NULL when no plan splits rows).
 * mgx_last_spmm_kernel(): "dot_attn_fwd" / "dot_attn_bwd_dst" / "dot_attn_bwd_src" after the respective launch.
 * Deterministic: no atomics, hub partial sums combined in slot order.  Purely additive: mgx_abi_version() stays 35. */
int32_t mgx_dot_attention_supported(const mgx_csr* csr, int64_t H, int64_t F);
int64_t mgx_dot_attention_workspace(const mgx_spmm_plan* plan /* may be NULL */, int64_t H, int64_t F);
int32_t mgx_dot_attention_fwd(const mgx_csr* csr, const mgx_spmm_plan* plan /* may be NULL */, int64_t H, int64_t F,
                              const float* q, int64_t q_ld, const float* k, int64_t k_ld, const float* v, int64_t v_ld,
                              float scale, float* out, float* stat, void* workspace, void* stream);
int32_t mgx_dot_attention_bwd(const mgx_csr* csc, const mgx_spmm_plan* csc_plan /* may be NULL */, const mgx_csr* csr,
                              const mgx_spmm_plan* csr_plan /* may be NULL */, int64_t H, int64_t F, const float* q, int64_t q_ld,
                              const float* k, int64_t k_ld, const float* v, int64_t v_ld, float scale, const float* out,
                              const float* d_out, float* stat, float* dq, float* dk, float* dv, void* workspace, void* stream);

/* Sum aggregation of relu(x_u + w_e) messages with NO E-sized temporary (the UDF message of main_dgl_molhiv_gcn.py:37-52 and
 * main_dgl_ppa_gcn.py:44-51 reduced with fn.sum; with scale = NULL upstream's dgl.nn.GINEConv; csrc/gine.hip):
 *   out[v,:] = sum_{e: u->v} s[e] * relu(x[u,:] + w[e,:])             (exactly 0 for a destination without in-edges)
 *   fwd: ONE walk of the in-CSR `csc`; w and s are indexed by EDGE ID: position p of the CSR reads w[eid(p)], s[eid(p)] with
 *        eid(p) = csc->eids[p], or p when eids is NULL.  scale NULL means s = 1.  Nothing of size E is written or kept.
 *   bwd: ONE walk of the transpose `csr` (rows = source nodes, its eids the same edge ids), where every edge is met exactly once:
 *        m[e,:] = s[e] * 1[x[u,:] + w[e,:] > 0] * d_out[v,:],   d_w[e,:] = m[e,:] (written exactly once per edge),
 *        d_x[u,:] = sum_{e: u->...} m[e,:] (exactly 0 for a source without out-edges).  d_x and d_w may each be NULL; s gets no gradient.
 *        The mask is recomputed from x and w (x[u,:] is loaded once per work item): fp32 x + w is one rounding, its sign is exact, so
 *        forward and backward agree on it.  relu'(0) = 0.
 * A NaN in x[u,c] + w[e,c] makes out[v,c] NaN and leaves every other (row, column) bitwise untouched; gradients at such an element
 * are unspecified.  +inf passes through.
 * x [csc->num_cols, D], w [nnz, D], scale [nnz], out [csc->num_rows, D]; d_out [csr->num_cols, D], d_x [csr->num_rows, D],
 * d_w [nnz, D]: fp32, dense, 16-byte aligned, allocated by the caller.
 * Supported (mgx_gine_supported): D % 4 == 0 and 4 <= D <= 256 (one pass of a wave; wider rows are NOT taken), 32-bit indices,
 * nnz > 0, and max(num_rows, num_cols, nnz) * D * 4 below 4 GiB -- gathered rows, w and d_w included, are addressed by 32-bit byte
 * offsets, so a graph whose nnz * D * 4 reaches 4 GiB is refused rather than addressed with 64-bit offsets.
 * Errors: a D that is not a positive multiple of 4, NULL or misaligned operands and a malformed plan are MGX_ERR_INVALID_ARGUMENT;
 * D > 256, 64-bit indices, nnz == 0 and operands of 4 GiB are MGX_ERR_UNSUPPORTED (the caller composes mgx_sddmm_* and mgx_spmm_csr).
 * The argument checks of the graph, D and the plan come before the supported-set checks: a malformed plan on an empty graph is an argument error.
 * plan: the CSR's mgx_spmm_plan or NULL (one work item per row); workspace: mgx_gine_workspace(plan, D) bytes (NULL when the plan
 * splits no row; the backward needs it only for d_x).  Nothing is read back to the host: every entry point can be captured in a graph.
 * mgx_last_spmm_kernel(): "gine_fwd" / "gine_bwd" after the respective launch.
 * Deterministic: no atomics, lane groups merged in a fixed order, hub partial sums combined in slot order -- the result is a function
 * of the arguments only.  Purely additive: mgx_abi_version() stays 35. */
int32_t mgx_gine_supported(const mgx_csr* csr, int64_t D);
int64_t mgx_gine_workspace(const mgx_spmm_plan* plan /* may be NULL */, int64_t D);
int32_t mgx_gine_fwd(const mgx_csr* csc, const mgx_spmm_plan* plan /* may be NULL */, int64_t D, const float* x /* [num_cols, D] */,
                     const float* w /* [nnz, D] by edge id */, const float* scale /* [nnz] by edge id, or NULL */,
                     float* out /* [num_rows, D] */, void* workspace, void* stream);
int32_t mgx_gine_bwd(const mgx_csr* csr /* transpose: rows = sources */, const mgx_spmm_plan* plan /* may be NULL */, int64_t D,
                     const float* x, const float* w, const float* scale, const float* d_out /* [csr->num_cols, D] */,
                     float* d_x /* or NULL */, float* d_w /* or NULL */, void* workspace, void* stream);

/* Several aggregates of the SAME messages in one walk (Principal Neighbourhood Aggregation, upstream's dgl.nn.PNAConv: the mailbox
 * UDF that takes mean, max, min and std of one message per edge; csrc/multiagg.hip):
 *   m_e = x[u(e),:] + w[e,:]  (w by EDGE ID as in mgx_gine_*: position p reads w[eid(p)]; w NULL: m_e = x[u(e),:]),  d = in-degree of v
 *   S1 = sum_e m_e,  S2 = sum_e m_e^2;   sum = S1,  mean = S1 / d,  msq = S2 / d,
 *   var = relu(msq - mean * mean) (a NaN stays a NaN),  std = sqrt(var + eps)
 *   max, min, arg_max, arg_min: exactly mgx_spmm_csr's MAX / MIN rule above -- storage order, strict compare from -inf / +inf, the first
 *   of equal extrema wins, a NaN never wins, a row that never beats the identity gives the identity with arg -1; the arg is the EDGE ID
 *   of the winner, int32.  A destination with d == 0 gives 0 in every aggregate, std included, with arg -1.
 *   fwd: ONE walk of the in-CSR `csc`.  One pointer per aggregate, NULL = not wanted (at least one is); each names a [num_rows, D] block
 *        whose rows are out_ld floats apart (out_ld % 4 == 0, >= D), so the aggregates can land in one [num_rows, A, D] tensor.
 *        arg_max / arg_min: [num_rows, D] int32, dense, optional, only with their aggregate.  When o_var or o_std is given, `stats`
 *        [num_rows, 2, D] receives (mean, var) for the backward and eps must be positive and finite; the backward mask 1[var > 0] is
 *        read from these stored bits, never recomputed.  Lane groups of a wave take interleaved edges and are merged on (value, CSR
 *        position): the larger (smaller) value, on equal values the smaller position, which is the storage-order rule; the chunks of a
 *        split row are merged in slot order by the same compare.
 *   bwd: ONE walk of the transpose `csr` (rows = source nodes, its eids the same edge ids), where every edge is met exactly once.
 *        The caller forms the per-destination rows (N-sized, elementwise) from the upstream gradients and `stats`:
 *          gv = (g_var + g_std / (2 std)) * 1[var > 0],   A = g_sum + g_mean / d - 2 gv mean / d,   B = 2 gv / d
 *        and the walk computes, per column,
 *          d m_e = A[v] + B[v] * m_e + g_max[v] * 1[arg_max[v] == e] + g_min[v] * 1[arg_min[v] == e]
 *          d_w[e,:] = d m_e (written exactly once per edge),   d_x[u,:] = sum_{e: u->...} d m_e (0 for a source without out-edges).
 *        A is required; B NULL means 0 (m_e is then not formed: x and w are not read); g_max / g_min come with their args or are NULL.
 *        The rows are SEPARATE dense [csr->num_cols, D] matrices: one 32-bit byte offset per edge addresses all of them.
 *        d_x and d_w may each be NULL.
 * All operands fp32 (args int32), 16-byte aligned, allocated by the caller.
 * Supported (mgx_multi_agg_supported), the set of mgx_gine_supported: D % 4 == 0 and 4 <= D <= 256, 32-bit indices, nnz > 0, and
 * max(num_rows, num_cols, nnz) * D * 4 below 4 GiB (every gathered matrix is addressed by 32-bit byte offsets).
 * Errors: a D that is not a positive multiple of 4, NULL or misaligned operands, a bad out_ld or eps and a malformed plan are
 * MGX_ERR_INVALID_ARGUMENT; D > 256, 64-bit indices, nnz == 0 and operands of 4 GiB are MGX_ERR_UNSUPPORTED (the caller composes
 * mgx_spmm_csr and mgx_sddmm_*).  The argument checks of the graph, D and the plan come before the supported-set checks.
 * plan: the CSR's mgx_spmm_plan or NULL; workspace: mgx_multi_agg_workspace(plan, D) bytes -- [slots, 6, D] (S1, S2, max, its
 * position, min, its position) forward, [slots, D] of it backward (needed only for d_x); NULL when the plan splits no row.
 * Nothing is read back to the host: every entry point can be captured in a graph.
 * mgx_last_spmm_kernel(): "multi_agg_fwd" / "multi_agg_bwd" after the respective launch.
 * Deterministic: no atomics, lane groups merged in a fixed order, hub chunks in slot order.  Purely additive: mgx_abi_version() stays 35. */
int32_t mgx_multi_agg_supported(const mgx_csr* csr, int64_t D);
int64_t mgx_multi_agg_workspace(const mgx_spmm_plan* plan /* may be NULL */, int64_t D);
int32_t mgx_multi_agg_fwd(const mgx_csr* csc, const mgx_spmm_plan* plan /* may be NULL */, int64_t D, const float* x /* [num_cols, D] */,
                          const float* w /* [nnz, D] by edge id, or NULL */, float eps, float* o_sum, float* o_mean, float* o_var,
                          float* o_std, float* o_max, float* o_min, int64_t out_ld, int32_t* arg_max, int32_t* arg_min,
                          float* stats /* [num_rows, 2, D] with o_var / o_std */, void* workspace, void* stream);
int32_t mgx_multi_agg_bwd(const mgx_csr* csr /* transpose: rows = sources */, const mgx_spmm_plan* plan /* may be NULL */, int64_t D,
                          const float* x, const float* w /* or NULL */, const float* A, const float* B /* or NULL */,
                          const float* g_max, const int32_t* arg_max, const float* g_min, const int32_t* arg_min,
                          float* d_x /* or NULL */, float* d_w /* or NULL */, void* workspace, void* stream);

/* ------------------------------------------------------------------ GAT attention terms
 * el[n,h] = sum_f feat[n,h,f] * attn[h,f] -- GATConv's `(feat * attn_l).sum(-1)` (main_dgl_reddit_gat.py:10, UPSTREAM
 * dgl.nn.pytorch.GATConv.forward), one pass; attn_b/out_b (may be NULL) apply a second attention vector to the same
 * feat in that pass (full-graph GAT: el and er share feat).  Needs H*F <= 256 and F <= 64 or F in {128, 256}
 * (else MGX_ERR_UNSUPPORTED).  Backward: d_feat = d_out_a*attn_a (+ d_out_b*attn_b) written once (d_feat may be NULL),
 * d_attn = column sums of d_out*feat, two-stage in fixed order; workspace of mgx_head_dot_bwd_workspace(H, F) bytes. */
int32_t mgx_head_dot_fwd(int64_t n, int64_t H, int64_t F, const float* feat, const float* attn_a,
                         const float* attn_b, float* out_a, float* out_b, void* stream);
int64_t mgx_head_dot_bwd_workspace(int64_t H, int64_t F);
int32_t mgx_head_dot_bwd(int64_t n, int64_t H, int64_t F, const float* feat, const float* attn_a,
                         const float* attn_b, const float* d_out_a, const float* d_out_b, float* d_feat,
                         float* d_attn_a, float* d_attn_b, void* workspace, void* stream);

/* ------------------------------------------------------------------ segment reduce
 * Replaces dgl.nn.AvgPooling / dgl.ops.segment_reduce (main_dgl_molhiv_gcn.py:75,93).
 * offsets: int64 [num_segments+1] (cumsum of batch_num_nodes).  reduce: SUM, MEAN, MAX, MIN.
 * arg (int64 [num_segments*D], MAX/MIN only) may be NULL. */
int32_t mgx_segment_reduce(int64_t num_segments, const int64_t* offsets, int64_t D, int32_t reduce,
                           const float* x, float* out, int64_t* arg, void* stream);

/* Column sum out[c] = sum_r x[r, c] of a row-major [n, C] matrix, C <= 256: the single-segment case of the readout
 * above (a segment of millions of rows has no row parallelism), used for the bias gradient of the dense layer that
 * follows every aggregation (`nn.Linear` in SAGEConv, main_dgl_product_sage.py:31-33).  Two stages in fixed order
 * (deterministic); workspace of mgx_column_sum_workspace(C) bytes. */
int64_t mgx_column_sum_workspace(int64_t C);
int32_t mgx_column_sum(int64_t n, int64_t C, const float* x, float* out, void* workspace, void* stream);

/* Two column reductions in one pass over a row-major [n, C] matrix (C <= 256): mode 0 -> (sum a, sum a*a), mode 1 ->
 * (sum a, sum a*b) -- the statistics of BatchNorm1d over the node dimension (main_dgl_arxiv_sage.py:70-77) forward and
 * backward; modes 2 / 3 are the same sums taken relative to the first row p of the squared / second operand, mode 2 ->
 * (sum (a-p), sum (a-p)^2) with p = a[0,:], mode 3 -> (sum a, sum a*(b-p)) with p = b[0,:], which keeps the variance
 * accurate when |mean| >> std; workspace of 2 * mgx_column_sum_workspace(C) bytes.  mgx_column_affine: out[r,c] = a[r,c]*A[c] + b[r,c]*B[c] +
 * Cc[c] (b/B may be NULL), C % 4 == 0, 16-byte aligned: the normalisation and its input gradient. */
int32_t mgx_column_pair_sums(int64_t n, int64_t C, int32_t mode, const float* a, const float* b, float* out0, float* out1,
                             void* workspace, void* stream);
int32_t mgx_column_affine(int64_t n, int64_t C, const float* a, const float* b, const float* A, const float* B, const float* Cc,
                          float* out, void* stream);

/* out[M, K] = a^T b for a [n, M] (row stride lda floats), b [n, K] (row stride ldb), out row stride ldc, n in the hundreds of
 * thousands to millions: the weight gradient dW = dY^T X of the dense layer after an aggregation
 * (main_dgl_product_sage.py:31-33,64).  M <= 64 and K <= 128: one tile, operands streamed once.  Up to M <= 256, K <= 1024
 * (round 2): the grid of 64 x 128 tiles in ONE launch, the tiles' waves walking the same rows together so that operand rows
 * are shared through L2 (else MGX_ERR_UNSUPPORTED).  fp32 MFMA, per-wave partial tiles added in fixed order
 * (deterministic); workspace of mgx_xty_workspace(M, K) bytes (-1 if the shape is unsupported). */
int64_t mgx_xty_workspace(int64_t M, int64_t K);
int32_t mgx_xty(int64_t n, int64_t M, int64_t K, const float* a, int64_t lda, const float* b, int64_t ldb, float* out, int64_t ldc,
                void* workspace, void* stream);
/* mgx_xty that also returns the column sums of a (colsum [M]; the bias gradient beside the weight gradient) from the same pass over a,
 * as the product with one more column of ones.  One 64 x 128 tile, b read with 16-byte loads (K % 4 == 0, K >= 64, ldb % 4 == 0,
 * 16-byte aligned), else MGX_ERR_UNSUPPORTED (mgx_xty + mgx_column_sum).  Same workspace. */
int32_t mgx_xty_colsum(int64_t n, int64_t M, int64_t K, const float* a, int64_t lda, const float* b, int64_t ldb, float* out, int64_t ldc,
                       float* colsum, void* workspace, void* stream);
/* mgx_xty / mgx_xty_colsum over a ROW LIST of b: row r of the reduction pairs a[r] (compact, n rows) with b[b_rows[r]] -- the weight
 * gradient of a layer whose output gradient exists on n listed rows only, read from the layer's [N, 2K] input buffer in place.  The same
 * rows per wave and the same MFMAs in the same order as the calls above on a gathered copy of b: the same bits.  b_rows: int64[n] on the
 * device; every entry must lie in [0, rows of b) -- NOT checked on the device.  b_rows == NULL: the calls above.  Built for a of
 * 33 .. 48 columns read by dword loads (the 47-class gradient) and b of 64 or 128 columns read by float4 loads (ldb % 4 == 0, 16-byte
 * aligned); else MGX_ERR_UNSUPPORTED (gather b and use the calls above).  Same workspace. */
int32_t mgx_xty_rows(int64_t n, int64_t M, int64_t K, const float* a, int64_t lda, const float* b, int64_t ldb, const int64_t* b_rows,
                     float* out, int64_t ldc, void* workspace, void* stream);
int32_t mgx_xty_colsum_rows(int64_t n, int64_t M, int64_t K, const float* a, int64_t lda, const float* b, int64_t ldb,
                            const int64_t* b_rows, float* out, int64_t ldc, float* colsum, void* workspace, void* stream);
/* mgx_xty_colsum for an a that is ZERO outside some rows and stored without them: row r of the reduction (over all n rows of b) pairs
 * a[a_pos[r]] with b[r]; a_pos[r] < 0 says that row r of a is zero -- neither it nor b[r] is read, and steps of four rows without any
 * row of a issue no MFMA.  a_pos: int64[n] on the device, every entry < rows of a -- NOT checked on the device.  Bit for bit the result
 * of mgx_xty_colsum on a scattered into a zero [n, M] matrix (same rows per wave, every row at the same place of its MFMA; the products
 * of a zero row leave an accumulator unchanged -- for finite b: 0 x Inf / NaN would be NaN there and is skipped here), which is what keeps a training run on the bits of the layer over all rows.  colsum may
 * be NULL.  Built for the shapes of mgx_xty_rows; else MGX_ERR_UNSUPPORTED.  a_pos == NULL: mgx_xty_colsum.  Same workspace. */
int32_t mgx_xty_colsum_pos(int64_t n, int64_t M, int64_t K, const float* a, int64_t lda, const int64_t* a_pos, const float* b,
                           int64_t ldb, float* out, int64_t ldc, float* colsum, void* workspace, void* stream);
/* mgx_xty_colsum of dZ [n, 64] against b [n, K] where dZ is the gradient behind relu + dropout and is never stored: dZ[r][j] =
 * dy[r][j] * (1 / (1 - p)) where bit j % 4 of mask[r * 16 + j / 4] is set, else 0.f (a select: an Inf or NaN behind a cleared bit does
 * not reach a sum) -- mask as mgx_relu_dropout_fwd / mgx_rows_gemm_relu_dropout write it for 64 columns, uint8 [n * 16].  One pass over
 * dy, mask and b and one finish launch instead of mgx_relu_dropout_bwd + one mgx_xty(_colsum) per 128 columns of b.  Bit for bit the
 * result of that composition (out[:, k0 : k0 + 128] = mgx_xty of b's column block k0 = 0, 128; colsum from the first): the same row
 * partitions, the same MFMAs in the same order per accumulator, the same order of the partial sums.  64 <= K <= 256, K % 4 == 0; dy
 * and b 16-byte aligned with row strides % 4 == 0; built for K = 64, 68 .. 80, 128, 196 .. 208 and 256, else MGX_ERR_UNSUPPORTED
 * (nothing is launched).  Workspace of mgx_xty_masked_workspace(K) bytes (-1 outside 64 .. 256 or K % 4 != 0). */
int64_t mgx_xty_masked_workspace(int64_t K);
int32_t mgx_xty_colsum_masked(int64_t n, int64_t K, const float* dy, int64_t lddy, const uint8_t* mask, float p, const float* b,
                              int64_t ldb, float* out, int64_t ldc, float* colsum, void* workspace, void* stream);

/* C[n, M] = A[n, K] x B (+ bias[M]) for A with millions of rows and small K, M -- the dense projections either side of an aggregation
 * (SAGEConv's fc_self / fc_neigh on [h | mean_agg(h)], main_dgl_product_sage.py:23-24,64, and the input gradient d[h | neigh] = dY x W).
 * B: [K, M] row-major with ldb, or -- b_transposed -- [M, K] (torch.nn.Linear's weight layout).  row_scale (may be NULL): C[r, m] is
 * multiplied by row_scale[r] for the columns m >= scale_from (the 1 / deg of fn.mean's backward on the `neigh` half).  fp32 MFMA, fixed
 * summation order.  K x M padded to 16 must fit a 64 KB stage and be one of the built shapes, else MGX_ERR_UNSUPPORTED (use a GEMM). */
int32_t mgx_rows_gemm(int64_t n, int64_t K, int64_t M, const float* a, int64_t lda, const float* b, int64_t ldb, int32_t b_transposed,
                      const float* bias /* [M] or NULL */, const float* row_scale /* [n] or NULL */, int64_t scale_from, float* c,
                      int64_t ldc, float* c2 /* NULL, or the matrix that receives the columns split_col .. M - 1 (as its columns 0 ..) */,
                      int64_t ldc2, int64_t split_col /* a multiple of 4 */, void* stream);
/* mgx_rows_gemm with row lists (int64[n] on the device, either may be NULL; both NULL: mgx_rows_gemm).
 *   a_rows:  row r of the product reads a[a_rows[r]]; c (and c2) stay compact [n, .] -- the projection of n listed rows of a tall matrix.
 *   c2_rows: row r of the SECOND output is stored at c2[c2_rows[r]]; c stays compact and no other row of c2 is written -- the scatter
 *            of one half of a gradient into a matrix the caller zeroed.  row_scale is indexed by r in both forms.
 * PRECONDITIONS, not checked on the device: every entry lies inside the matrix it indexes, and the entries of c2_rows are distinct (two
 * rows stored at one place would race).  The same MFMAs in the same order as mgx_rows_gemm on a gathered copy: the same bits.
 * Built for: a_rows with K = 113 .. 128 in the float4 form (K % 4 == 0, lda % 4 == 0, a 16-byte aligned) and M <= 64; c2_rows with
 * K = 37 .. 48 in the dword form and 65 <= M <= 128.  Everything else: MGX_ERR_UNSUPPORTED (gather / scatter around mgx_rows_gemm). */
int32_t mgx_rows_gemm_rows(int64_t n, int64_t K, int64_t M, const float* a, int64_t lda, const int64_t* a_rows, const float* b, int64_t ldb,
                           int32_t b_transposed, const float* bias, const float* row_scale, int64_t scale_from, float* c, int64_t ldc,
                           float* c2, int64_t ldc2, int64_t split_col, const int64_t* c2_rows, void* stream);
/* 1 when mgx_rows_gemm has a kernel for these sizes (lda: A's row stride in floats), else 0. */
int32_t mgx_rows_gemm_supported(int64_t K, int64_t M, int64_t lda);
/* Rows that one sweep of mgx_rows_gemm's grid covers on the current device for these sizes (relu_dropout != 0: of
 * mgx_rows_gemm_relu_dropout's): every workgroup that is resident at once, 16 rows per wave.  A wave of a longer matrix walks its
 * tiles this far apart.  0 when there is no kernel. */
int64_t mgx_rows_gemm_sweep_rows(int64_t K, int64_t M, int64_t lda, int32_t relu_dropout);
/* The same product followed by relu and inverted dropout (main_dgl_product_sage.py:93-95) in the epilogue: y[r, :] (row stride ldy) and the
 * 4 mask bits per float4 exactly as mgx_relu_dropout_fwd_strided(p, seed, offset) would produce them from the stored product -- which is
 * never written.  M % 4 == 0, y 16-byte aligned, ldy % 4 == 0; mask: [n * M / 4] bytes.
 * slots (optional, M == 64 only): the rows of y as 128-byte slots as well, byte for byte what mgx_rows_slots_pack(y) would write (the
 * epilogue holds a row exactly as that pass reads it), *overflow_rows (device, may be NULL) += rows with more than 24 non-zeros -- the
 * next layer's aggregation (mgx_spmm_copy_u_slots) then needs no pack pass. */
int32_t mgx_rows_gemm_relu_dropout(int64_t n, int64_t K, int64_t M, const float* a, int64_t lda, const float* b, int64_t ldb,
                                   int32_t b_transposed, const float* bias /* [M] or NULL */, float p, uint64_t seed, uint64_t offset,
                                   float* y, int64_t ldy, uint8_t* mask, void* slots /* [n, 128 bytes] or NULL */,
                                   int64_t* overflow_rows /* or NULL */, void* stream);

/* y = dropout_p(relu(x)) in one pass (inverted dropout: kept values scaled by 1/(1-p)); the activation between two
 * aggregations (main_dgl_product_sage.py:93-95).  n elements, n % 4 == 0, 16-byte aligned; mask: n/4 bytes, 4 bits per
 * float4 = (x > 0 AND kept), all that backward needs: dx = mask ? dy/(1-p) : 0.  Random bits are a counter-based function
 * of (seed, offset + element index): the caller advances `offset` by n between calls.
 * The stream: float4 number i of the dense tensor draws r0 = splitmix64(seed ^ ((offset + i) * 2)) and r1 = splitmix64(seed ^
 * ((offset + i) * 2 + 1)), modulo 2^64; x, y, z, w are kept when (uint32)r0, r0 >> 32, (uint32)r1, r1 >> 32 are >= uint32(p * 2^32).
 * NaN rule: "x > 0" is evaluated as !(x <= 0), so a NaN is never turned into a clean zero.  At a kept position it gives NaN with
 * its mask bit SET (backward passes dy/(1-p) there); at a dropped position 0 with a clear bit.  Finite and infinite inputs are not
 * affected.  mgx_rows_gemm_relu_dropout follows the same rule, and what derives sparsity from y (mgx_rows_slots_pack*,
 * mgx_row_nonzero_bits, mgx_rows_pack_count) tests != 0, which counts a NaN as a value. */
int32_t mgx_relu_dropout_fwd(int64_t n, const float* x, float p, uint64_t seed, uint64_t offset, float* y, uint8_t* mask,
                             void* stream);
int32_t mgx_relu_dropout_bwd(int64_t n, const float* dy, const uint8_t* mask, float p, float* dx, void* stream);
/* Row-strided forms (round 2): [rows, cols] views whose rows are *_stride floats apart (cols, strides % 4 == 0); the mask
 * stays dense and equals the dense call's for the same (seed, offset). */
int32_t mgx_relu_dropout_fwd_strided(int64_t rows, int64_t cols, const float* x, int64_t x_stride, float p, uint64_t seed,
                                     uint64_t offset, float* y, int64_t y_stride, uint8_t* mask, void* stream);
int32_t mgx_relu_dropout_bwd_strided(int64_t rows, int64_t cols, const float* dy, int64_t dy_stride, const uint8_t* mask, float p,
                                     float* dx, int64_t dx_stride, void* stream);
/* mgx_relu_dropout_bwd_strided for rows of exactly 64 columns that ALSO writes the result's rows, times row_scale[r] when given, as
 * 128-byte slots (mgx_rows_slots_pack's format, byte for byte what that pass would write from row_scale * dx): the gradient behind
 * relu + dropout is as sparse as the activation, and the reversed aggregation that follows gathers the slots (mgx_spmm_copy_u_slots). */
int32_t mgx_relu_dropout_bwd_slots(int64_t rows, const float* dy, int64_t dy_stride, const uint8_t* mask, float p, float* dx,
                                   int64_t dx_stride, const float* row_scale /* [rows] or NULL */, void* slots /* [rows, 128 bytes] */,
                                   int64_t* overflow_rows /* device, may be NULL */, void* stream);
/* Forward whose offset into the random stream is read from device memory when the launch RUNS (offset = *counter *
 * 0x9E3779B97F4A7C15 mod 2^63): captured in a HIP graph next to an increment of the counter, every replay draws a new mask. */
int32_t mgx_relu_dropout_fwd_counter(int64_t rows, int64_t cols, const float* x, int64_t x_stride, float p, uint64_t seed,
                                     const uint64_t* counter, float* y, int64_t y_stride, uint8_t* mask, void* stream);

/* ------------------------------------------------------------------ graph readout: segment softmax, segment attention
 * (csrc/segattn.hip).  Segments are the contiguous row slices of a batched graph: offsets int64 [num_segments+1] on the device
 * (the array mgx_segment_reduce takes), offsets[num_segments] = number of rows.  Nothing is read back to the host: every entry
 * point can be captured in a HIP graph.  All operands fp32.
 *
 * Segment softmax (dgl.softmax_nodes / softmax_edges), per column, any D >= 1, one launch each way:
 *   out[i,c] = exp(x[i,c] - m[g,c]) / s[g,c]          m, s = max and sum over the rows of segment g
 *   d_x      = out * (d_out - sum_{j in g} out[j,c] * d_out[j,c])
 *
 * Segment attention (dgl.nn.GlobalAttentionPooling, dgl.nn.Set2Set), one launch each way, no N-sized temporary:
 *   gate mode  (logits given):  z[i,h] = logits[i,h]                                      (scale ignored)
 *   query mode (query given):   z[i,h] = scale * sum_f feat[i,h,f] * query[g,h,f]         (scale applied once, after the sum)
 *   a[i,h] = exp(z[i,h] - m[g,h]) / s[g,h];   out[g,h,:] = sum_{i in g} a[i,h] * feat[i,h,:]
 *   fwd: writes out [S, H*F] and stat [S, H, 2] = (m, 1/s), from which the backward rebuilds a; `a` is never written.
 *   bwd: t[g,h] = <out[g,h,:], d_out[g,h,:]>, dp[i,h] = <feat[i,h,:], d_out[g,h,:]>, dz = a * (dp - t);
 *        gate:  d_logits = dz, d_feat[i] = a * d_out[g];
 *        query: d_feat[i] = a * d_out[g] + dz * scale * query[g], d_query[g] = scale * sum_i dz * feat[i].
 *        d_feat [N, H*F], d_logits [N, H] (gate mode), d_query [S, H*F] (query mode) may each be NULL.
 * Exactly one of logits [N, H] and query [S, H*F] is non-NULL (else MGX_ERR_INVALID_ARGUMENT).  feat [N, feat_ld]: the first H*F
 * floats of a row are the operand, so feat may be a column block of a wider matrix.  feat, query, out, d_out, d_feat, d_query:
 * 16-byte aligned; everything but feat dense.
 * Supported (mgx_segment_attention_supported; everything else is MGX_ERR_UNSUPPORTED and the caller composes mgx_segment_reduce
 * and mgx_gather_rows): F % 4 == 0, H*F <= 256, feat_ld % 4 == 0 and >= H*F; H == 1: any such F; H > 1: F in {4, 8, 16, 32, 64}.
 * Edge rules: an empty segment gives out = 0, stat = (0, 0) and zero gradients; a -inf logit has weight 0; a segment whose logits
 * are all -inf behaves like an empty one (out = 0, not NaN); a NaN logit makes that (segment, head) NaN -- for the softmax that
 * (segment, column) -- and leaves every other one untouched.
 * One wave walks one segment whatever its length (as in mgx_segment_reduce): a few very long segments have little parallelism.
 * Deterministic: no atomics, lane groups merged in a fixed order.  Purely additive: mgx_abi_version() stays 35. */
int32_t mgx_segment_softmax_fwd(int64_t num_segments, const int64_t* offsets, int64_t D, const float* x, float* out, void* stream);
int32_t mgx_segment_softmax_bwd(int64_t num_segments, const int64_t* offsets, int64_t D, const float* out, const float* d_out,
                                float* d_x, void* stream);
int32_t mgx_segment_attention_supported(int64_t H, int64_t F, int64_t feat_ld);
int32_t mgx_segment_attention_fwd(int64_t num_segments, const int64_t* offsets, int64_t H, int64_t F, const float* feat,
                                  int64_t feat_ld, const float* logits /* [N, H] or NULL */, const float* query /* [S, H*F] or NULL */,
                                  float scale, float* out, float* stat, void* stream);
int32_t mgx_segment_attention_bwd(int64_t num_segments, const int64_t* offsets, int64_t H, int64_t F, const float* feat,
                                  int64_t feat_ld, const float* logits, const float* query, float scale, const float* out,
                                  const float* d_out, const float* stat, float* d_feat, float* d_logits, float* d_query,
                                  void* stream);

/* ------------------------------------------------------------------ graph readout: segment top-k (csrc/segtopk.hip)
 * dgl.topk_nodes / topk_edges and the selection of dgl.nn.SortPooling over the segments described above (offsets int64
 * [num_segments+1] on the device; segment s = rows offsets[s] .. offsets[s+1]).  feat [N, ld] fp32, the first D floats of a row are the
 * operand (ld >= D, no alignment asked).  Everything is a copy: outputs hold input BITS.
 *
 * Order inside a segment = torch.sort(key, stable=True, descending=...) on the CPU: NaN is the greatest key (first when descending,
 * last when ascending; a NaN with the sign bit set is a NaN too), -0.0 == +0.0, equal keys keep the lower row first in both
 * directions.
 *   mode 0 (rows):    key = column `sortby` in [0, D);  values[s, j, :] = the whole row of rank j,  index[s, j] = its row number
 *                     INSIDE the segment (int64);  values [S, k, D], index [S, k], slot [N]
 *   mode 1 (columns): every column ranked on its own (`sortby` ignored);  values[s, j, c], index[s, j, c];
 *                     values [S, k, D], index [S, k, D], slot [N, D]
 * A segment shorter than k: ranks j >= len hold zero values and index -1.
 * slot (int32) is the inverse map: the flat output rank s*k + j of a selected row (mode 0) or element (mode 1), -1 for one not
 * selected.  The forward writes every output element and all of slot: no memset is needed.
 *   bwd: d_feat[i, c] = slot >= 0 ? d_values[slot, c] : 0 with slot = slot[i] (mode 0) or slot[i, c] (mode 1); d_values [S*k, D] and
 *        d_feat [N, D] dense.  A pure gather that writes every element of d_feat once, one launch.
 * Supported (mgx_segment_topk_supported(k, D, mode); everything else is MGX_ERR_UNSUPPORTED and the caller composes sorts and
 * gathers): 1 <= k <= 1024, any D >= 1, segments shorter than 2^32 - 1, N < 2^31, num_segments * k < 2^31 (mode 1: num_segments * D
 * < 2^31).  k <= 64: one wave per segment (mode 1: per segment and column); larger k: one 256-thread workgroup with 16 KB of LDS.
 * One wave / workgroup walks a segment whatever its length.  Nothing is read back to the host: capture-safe.
 * Deterministic: no atomics.  Purely additive: mgx_abi_version() stays 35. */
int32_t mgx_segment_topk_supported(int64_t k, int64_t D, int32_t mode);
int32_t mgx_segment_topk_fwd(int64_t num_segments, const int64_t* offsets, int64_t N, int64_t D, int64_t ld, const float* feat, int64_t k,
                             int32_t mode, int64_t sortby, int32_t descending, float* values, int64_t* index, int32_t* slot,
                             void* stream);
int32_t mgx_segment_topk_bwd(int64_t N, int64_t D, int32_t mode, const int32_t* slot, const float* d_values, float* d_feat,
                             void* stream);

/* ------------------------------------------------------------------ point clouds: segment k nearest neighbours (csrc/knn.hip)
 * dgl.knn_graph / segmented_knn_graph over the segments described above: for every row i of x [N, ld] fp32 (the first D floats of a
 * row are the point, ld >= D, no alignment asked) the k rows j of i's own segment, i included, with the smallest
 *   d(i, j) = sum_c (x[i,c] - x[j,c])^2      (fp32, c ascending, one fma per term; the direct difference form)
 * ordered by (d, j) ascending: equal distances keep the lower row first, a NaN distance is the greatest key and NaNs tie.
 *   index int64 [N, k]: global row numbers in x;  dist fp32 [N, k] or NULL: the distances of those ranks.
 * A segment shorter than k: ranks >= len hold index -1 and dist +inf; so does every rank of a row that no segment holds.  Every
 * output element is written: no memset is needed.  Distances and selection are one launch: no [n, n] matrix exists.
 * Supported (mgx_segment_knn_supported(k, D); everything else is MGX_ERR_UNSUPPORTED before a launch and the caller composes a
 * sort): 1 <= k <= 64, 1 <= D <= 256, N and num_segments < 2^31, N * ld * 4 bytes < 4 GiB.  One 256-thread workgroup per 16 query
 * rows streams the rows of their segments through LDS.  Nothing is read back to the host and the launch depends on N only:
 * capture-safe.  Deterministic: no atomics.  Purely additive: mgx_abi_version() stays 35. */
int32_t mgx_segment_knn_supported(int64_t k, int64_t D);
int32_t mgx_segment_knn(int64_t num_segments, const int64_t* offsets, int64_t N, int64_t D, int64_t ld, const float* x, int64_t k,
                        int64_t* index, float* dist /* may be NULL */, void* stream);

/* The same search from a query set into a reference set (PyG's knn(x, y, k, batch_x, batch_y), the neighbour step of PointNet++'s
 * feature propagation): references x [N, ld] in num_segments segments given by offsets, queries y [M, ldq] in the SAME number of
 * segments given by q_offsets (num_segments + 1 entries each).  Query row q of query segment s gets the k rows j of reference segment
 * s = [offsets[s], offsets[s+1]) with the smallest d(q, j) = sum_c (y[q,c] - x[j,c])^2, by the arithmetic and the order above; index
 * holds global rows of x.  Ranks at or beyond the reference segment's length hold index -1 and dist +inf, and so does every rank of a
 * query row that no query segment holds.  mgx_segment_knn is the case y = x, q_offsets = offsets: one kernel serves both.
 *   weight fp32 [M, k] or NULL: weight[q, r] = (1 / (dist[q, r] + eps)) / sum_r' (1 / (dist[q, r'] + eps)) over the valid ranks r',
 *   the normalised inverse squared-distance weights of knn_interpolate; a padded rank gets 0, a query without a valid rank k zeros; a
 *   NaN distance makes the sum, and so every valid rank's weight of that query, NaN.  The terms are fp32 with a true division each;
 *   the sum is a balanced binary tree over the ranks padded with zeros to 64 -- (t0 + t1) + (t2 + t3), then pairs of those, ... -- so
 *   it is deterministic and the same whatever k.
 * Every output element is written.  Supported (mgx_segment_knn_query_supported(k, D); everything else is MGX_ERR_UNSUPPORTED before a
 * launch): 1 <= k <= 64, 1 <= D <= 256, N, M and num_segments < 2^31, N * ld and M * ldq * 4 bytes < 4 GiB.  One launch whose grid
 * depends on M only; a workgroup's 16 consecutive query rows stream the union of their reference segments, one contiguous row
 * range.  Nothing is read back to the host, no atomics: capture-safe, reruns are bitwise equal.  Purely additive:
 * mgx_abi_version() stays 35. */
int32_t mgx_segment_knn_query_supported(int64_t k, int64_t D);
int32_t mgx_segment_knn_query(int64_t num_segments, const int64_t* offsets, int64_t N, int64_t ld, const float* x,
                              const int64_t* q_offsets, int64_t M, int64_t ldq, const float* y, int64_t D, int64_t k, float eps,
                              int64_t* index /* [M, k] */, float* dist /* [M, k] or NULL */, float* weight /* [M, k] or NULL */,
                              void* stream);

/* ------------------------------------------------------------------ point clouds: farthest point sampling (csrc/fps.hip)
 * dgl.geometry.farthest_point_sampler over the segments described above (x [N, ld] fp32, the first D floats of a row are the point).
 * Per segment of length len starting at row beg:
 *   mind[j] = +inf for every row j;  cur = start ? start[s] : 0, a value outside [0, len) is taken as 0
 *   for t = 0 .. min(m, len) - 1:
 *     index[s, t] = beg + cur;  dist[s, t] = mind[cur]  (rank 0 therefore has dist = +inf);  cur is selected and never chosen again
 *     for every unselected j:  d = sum_c (x[cur,c] - x[j,c])^2  (fp32, c ascending, one fma per term: the direct form of the k-NN);
 *                              if (d < mind[j]) mind[j] = d  -- a NaN d leaves mind[j] unchanged
 *     cur = the unselected row with the greatest mind, the lowest row on ties
 *   ranks t >= len: index = -1, dist = 0.
 *   index int64 [S, m]: global row numbers in x;  dist fp32 [S, m] or NULL.  Every output element is written: no memset is needed.
 * Consequences: the min(m, len) selected rows are distinct; duplicate points are taken in row order once everything else is at
 * distance 0; a row with a NaN coordinate keeps mind = +inf, so it is selected right after the start (the lowest such row first), and
 * once it is cur it changes no mind.
 * max_len: an upper bound of the segment lengths, a HOST argument (like `total` elsewhere) that chooses the kernel's shape.  A segment
 * that is longer on the device is a caller error the library cannot see: the kernel clamps it to its first max_len rows and reads or
 * writes nothing out of bounds.
 * Supported (mgx_segment_fps_supported(D, max_len); everything else is MGX_ERR_UNSUPPORTED before a launch and the caller composes
 * the loop): 1 <= D <= 64 and max_len points of (D | 1) floats within 152 KiB of LDS and 16 384 points of registers:
 *   max_len <= min(16384, 38912 / (D | 1)):  D = 1: 16 384;  D = 2, 3: 12 970;  D = 4: 7 782;  D = 64: 598
 * and N, num_segments, num_segments * m < 2^31, N * ld * 4 bytes < 4 GiB.  One workgroup per segment, one launch, the whole chain
 * on chip (coordinates in LDS, mind in registers, one barrier per selected point); the workgroup is 256 threads x 1 point
 * (max_len * (D | 1) <= 4096 floats), 512 x 2 (<= 8192 floats), 512 x 8, 1024 x 8 or 1024 x 16 (docs/LOG_fps.md has the
 * measurements behind these).  Nothing is read back to the host and the launch depends on num_segments, D and max_len only: capture-safe.  Deterministic: no atomics.  Purely additive: mgx_abi_version() stays 35. */
int32_t mgx_segment_fps_supported(int64_t D, int64_t max_len);
int32_t mgx_segment_fps(int64_t num_segments, const int64_t* offsets, int64_t N, int64_t D, int64_t ld, const float* x, int64_t m,
                        int64_t max_len, const int64_t* start /* [S] or NULL */, int64_t* index /* [S, m] */,
                        float* dist /* [S, m] or NULL */, void* stream);

/* ------------------------------------------------------------------ point clouds: fixed-radius ball query (csrc/ballquery.hip)
 * The PointNet++ grouping step: for query q with centre row c = centers[q] (a global row of x, -1 = none), inside the segment that
 * holds c, index[q, :] holds the FIRST K rows j in ascending row order (not the nearest) with
 *   d(c, j) = sum_c' (x[c,c'] - x[j,c'])^2 <= radius2     (the fp32 direct form above; a NaN d is outside the ball)
 * and count[q] how many were found, at most K.  Ranks >= count[q] hold index[q, 0] when pad_first is set (the PointNet++ convention:
 * every query then has exactly K entries), otherwise -1.  count[q] == 0 -- a NaN centre, c = -1, c in no segment -- leaves every
 * rank -1.  index int64 [M, K], count int32 [M]; every element is written.
 * Supported (mgx_segment_ball_query_supported(K, D); everything else is MGX_ERR_UNSUPPORTED before a launch): 1 <= K <= 64,
 * 1 <= D <= 256, N, num_segments and M < 2^31, N * ld * 4 bytes < 4 GiB.  The streaming of the k-NN (one 256-thread workgroup per 16
 * queries, csrc/knn_stream.h); selection is a ballot and a prefix popcount, and a workgroup stops once its 16 queries are full.
 * Nothing is read back to the host and the launch depends on M only: capture-safe.  Deterministic: no atomics.  Purely additive:
 * mgx_abi_version() stays 35. */
int32_t mgx_segment_ball_query_supported(int64_t K, int64_t D);
int32_t mgx_segment_ball_query(int64_t num_segments, const int64_t* offsets, int64_t N, int64_t D, int64_t ld, const float* x, int64_t M,
                               const int64_t* centers /* [M] */, float radius2, int64_t K, int32_t pad_first,
                               int64_t* index /* [M, K] */, int32_t* count /* [M] */, void* stream);

/* ------------------------------------------------------------------ formats (integer, bit-exact)
 * Replace the lazy COO->CSR/CSC construction behind g.formats(...)/first kernel call
 * (main_dgl_product_sage.py:158, kernel/dgl-new.py:63) and g.in_degrees()
 * (main_dgl_molhiv_gcn.py:41).
 *
 * mgx_coo_to_csr: stable sort of the COO by `row` (edge-id order kept inside a row).
 *   For the in-CSR pass row = dst, col = src.  Outputs indptr[num_rows+1], indices[nnz],
 *   eids[nnz] in the same index width.  `workspace` of mgx_coo_to_csr_workspace() bytes. */
int64_t mgx_coo_to_csr_workspace(int64_t num_rows, int64_t nnz, int32_t idx_bits);
int32_t mgx_coo_to_csr(int64_t num_rows, int64_t nnz, const void* row, const void* col, int32_t idx_bits,
                       void* indptr, void* indices, void* eids,
                       void* workspace, int64_t workspace_bytes, void* stream);
/* Transpose of a CSR (the out-CSR from the in-CSR or back; UPSTREAM aten::CSRTranspose behind g.formats / the reversed
 * graph of every SpMM backward): rows of the result = columns of `csr`, entries of a row in EDGE-ID order -- bit-identical
 * to mgx_coo_to_csr on the graph's COO, so both formats address the same edge tensors and reduce in the same order.
 * csr->eids must be a permutation of [0, nnz) or NULL (= positions).  Outputs indptr_t[num_cols+1], indices_t[nnz],
 * eids_t[nnz]; workspace of mgx_csr_transpose_workspace() bytes. */
int64_t mgx_csr_transpose_workspace(int64_t num_cols, int64_t nnz, int32_t idx_bits);
int32_t mgx_csr_transpose(const mgx_csr* csr, void* indptr_t, void* indices_t, void* eids_t,
                          void* workspace, int64_t workspace_bytes, void* stream);
/* in_degrees / out_degrees from a CSR: deg[v] = indptr[v+1]-indptr[v] (graph index width). */
int32_t mgx_csr_degrees(int64_t num_rows, const void* indptr, int32_t idx_bits, void* deg, void* stream);
/* inv_deg[v] = 1 / max(deg,1) as fp32 (the factor of fn.mean and of its backward). */
int32_t mgx_csr_inv_degrees(int64_t num_rows, const void* indptr, int32_t idx_bits, float* inv_deg, void* stream);

/* Host-side (CPU pointers, no GPU needed) stable COO->CSR used when a graph is prepared on the
 * CPU before .to(device) (main_dgl_product_sage.py:158 does formats() before to()). */
int32_t mgx_coo_to_csr_host(int64_t num_rows, int64_t nnz, const void* row_host, const void* col_host,
                            int32_t idx_bits, void* indptr_host, void* indices_host, void* eids_host);

/* ------------------------------------------------------------------ halo exchange helpers (multi-GPU)
 * New capability (the reference is single-GPU): pack boundary rows for the RCCL all_to_all and
 * add received gradient rows back into their owners.
 *   gather_rows:      out[i,:]      = x[idx[i],:]
 *   scatter_add_rows: x[idx[i],:]  += in[i,:]   (idx sorted & unique per call => no atomics) */
int32_t mgx_gather_rows(int64_t n, const void* idx, int32_t idx_bits, int64_t D,
                        const float* x, float* out, void* stream);
/* The same gather over row-strided operands (round 4): x rows x_stride floats apart, out rows out_stride floats apart (both >= D,
 * multiples of 4, 16-byte aligned pointers; else MGX_ERR_UNSUPPORTED) -- packs the boundary rows straight out of a column block of a
 * wider matrix (the left half of the one-GEMM SAGE layer's [h | neigh] buffer). */
int32_t mgx_gather_rows_strided(int64_t n, const void* idx, int32_t idx_bits, int64_t D, const float* x, int64_t x_stride,
                                float* out, int64_t out_stride, void* stream);
int32_t mgx_scatter_add_rows(int64_t n, const void* idx, int32_t idx_bits, int64_t D,
                             const float* in, float* x, void* stream);

/* Halo rows as bitmaps + packed values (round 5, csrc/rowpack.hip): the exchange of relu + dropout outputs, ~75 % exact zeros
 * (main_dgl_product_sage.py:93-96), moves a 64-bit mask per 64 columns + the non-zero values forward and the values under the SAME
 * mask back.  masks: [n, mgx_rows_mask_words(D)] uint64; bit (c * G + l) of a block's word = column 64 * block + 4 l + c, G = min(16,
 * pow2 >= D / 4); a row's values are stored in increasing bit order, block after block, from offsets[i] on (the caller's exclusive
 * scan of `counts`).  idx: row ids of x (NULL = identity).  D % 4 == 0, D <= 256, strides multiples of 4, 16-byte aligned, else
 * MGX_ERR_UNSUPPORTED.  Values are moved, never rounded: unpack(pack(x)) == x bit for bit. */
int64_t mgx_rows_mask_words(int64_t D);
int32_t mgx_rows_pack_count(int64_t n, const void* idx, int32_t idx_bits, int64_t D, const float* x, int64_t x_stride,
                            uint64_t* masks, int32_t* counts /* [n] non-zeros per row */, void* stream);
int32_t mgx_rows_mask_count(int64_t n, int64_t D, const uint64_t* masks, int32_t* counts, void* stream);
int32_t mgx_rows_pack_values(int64_t n, const void* idx, int32_t idx_bits, int64_t D, const float* x, int64_t x_stride,
                             const uint64_t* masks, const int64_t* offsets /* [n] */, float* values, void* stream);
int32_t mgx_rows_unpack(int64_t n, int64_t D, const uint64_t* masks, const int64_t* offsets, const float* values,
                        float* out /* [n, D] rows out_stride apart; zeros where the mask is clear */, int64_t out_stride, void* stream);
/* out[v, :] += sum over the entries p = positions[q], q in [indptr[v], indptr[v+1]), of the packed row p (int32 CSR over the n output rows;
 * entries added in CSR order: deterministic): the returned halo-row gradients added into their owners without a dense intermediate.
 * `values` holds fewer than 2^32 floats (offsets are used as 32-bit numbers on the D <= 64 path). */
int32_t mgx_rows_unpack_add_csr(int64_t n, const int32_t* indptr, const int32_t* positions, int64_t D, const uint64_t* masks,
                                const int64_t* offsets, const float* values, float* out, int64_t out_stride, void* stream);

/* ------------------------------------------------------------------ neighbor sampling
 * Replaces the CPU-side sampling of dgl.dataloading.MultiLayerNeighborSampler / dgl.sampling.sample_neighbors
 * (end_to_end/sampling/node-classification/reddit/ns-sage-dgl.py:132-141): for every seed v (a row of the in-CSR)
 * keep all in-edges when in_degree(v) <= fanout, else `fanout` distinct in-edges drawn uniformly (Floyd's
 * algorithm, counter-based generator: the same rng_seed gives the same sample).  The caller computes
 * out_offsets = exclusive cumsum of min(in_degree, fanout) ([num_seeds+1], int64) and allocates out_src / out_eid
 * (graph index width, out_offsets[num_seeds] entries).  Picks of one seed are written in CSR order.
 * fanout in [1, 64]. */
int32_t mgx_sample_neighbors(const mgx_csr* csr, int64_t num_seeds, const void* seeds, int32_t fanout,
                             uint64_t rng_seed, const int64_t* out_offsets, void* out_src, void* out_eid,
                             void* stream);

/* The other modes of dgl.sampling.sample_neighbors -- prob=, replace=True (ogbn-product/ns-gat/ns-gat-dgl.py:22-42) -- and
 * dgl.sampling.select_topk: one wave per seed (csrc/sample.hip).  Purely additive entry points: no existing signature or behaviour
 * changed with them, so mgx_abi_version() stays 35.
 *
 * Common to the three entry points below: `csr` is the in-CSR (or the out-CSR for edge_dir="out"; the seeds are its rows), `prob` /
 * `weight` is fp32 with one value per EDGE ID -- the kernels read prob[eids[p]] for CSR position p, prob[p] only when csr->eids is
 * NULL.  Output order is that of mgx_sample_neighbors: grouped by seed in seed order, CSR positions non-decreasing inside a seed.
 * out_offsets is [num_seeds + 1] int64 (exclusive cumsum of the per-seed counts given below, computed by the caller, who allocates
 * out_src / out_eid with out_offsets[num_seeds] entries of the graph's index width); a kernel never writes more than
 * out_offsets[s + 1] - out_offsets[s] entries for seed s.  fanout / k in [1, 64]; rows shorter than 2^32 - 1 edges.
 *
 * mgx_sample_count_positive: out_counts[s] = number of in-edges of seed s with prob > 0.  *out_invalid (device int32, zeroed by the
 *   caller) is set to 1 when an in-edge of any seed has a negative, NaN or infinite weight; the caller reads it together with the
 *   output size and raises.  Weights of edges of other nodes are not looked at. */
int32_t mgx_sample_count_positive(const mgx_csr* csr, int64_t num_seeds, const void* seeds, const float* prob,
                                  int64_t* out_counts /* [num_seeds] */, int32_t* out_invalid /* [1] */, void* stream);
/* mgx_sample_neighbors_weighted:
 *   prob != NULL, replace == 0   successive weighted sampling without replacement (draw proportionally to weight, remove, repeat) as
 *       Efraimidis-Spirakis keys: key = -log(u) / w, u strictly inside (0, 1) from (rng_seed, seed slot, CSR position); the `fanout`
 *       smallest (key, position) pairs among the edges of weight > 0.  count(s) = min(fanout, positive-weight in-edges), all distinct.
 *   replace != 0   `fanout` independent draws, lane j of the seed's wave owns draw j: position floor(r * deg) when prob == NULL
 *       (count = fanout when deg > 0, else 0); else the inverse CDF over the row -- the first position whose inclusive running sum,
 *       taken in row order (fp32 inside a chunk of 64, fp64 across chunks), is strictly greater than u * W, which is never an edge
 *       of weight 0; a target that rounding pushed to >= W lands on the last positive-weight edge (count = fanout when the seed has
 *       a positive-weight in-edge, else 0).  Duplicates are written as duplicates.
 *   prob == NULL, replace == 0 is mgx_sample_neighbors and an error here.
 *   The same rng_seed gives the same sample, for either index width.  A weight of 0 is never picked; negative / NaN / infinite
 *   weights are treated as 0 here and reported by mgx_sample_count_positive. */
int32_t mgx_sample_neighbors_weighted(const mgx_csr* csr, int64_t num_seeds, const void* seeds, int32_t fanout, const float* prob,
                                      int32_t replace, uint64_t rng_seed, const int64_t* out_offsets, void* out_src, void* out_eid,
                                      void* stream);
/* mgx_select_topk: for every seed the k in-edges of largest weight (ascending != 0: smallest), all of them when in_degree <= k
 *   (count = min(k, in_degree)); equal weights go to the lower CSR position.  Deterministic: the selection of
 *   mgx_sample_neighbors_weighted with key = -weight (or +weight). */
int32_t mgx_select_topk(const mgx_csr* csr, int64_t num_seeds, const void* seeds, int32_t k, const float* weight, int32_t ascending,
                        const int64_t* out_offsets, void* out_src, void* out_eid, void* stream);

/* ------------------------------------------------------------------ sampled blocks and induced subgraphs (csrc/relabel.hip)
 * What follows the sampler on every step: global node ids -> the local ids of a bipartite block (dgl.to_block) or of a node-induced
 * subgraph (g.subgraph).  Integer kernels over a look-up table int32[num_nodes] (-1 = not in the output) that the entry point fills
 * itself (hipMemsetAsync): nothing is kept between calls.  Every id read from a caller's array is checked against [0, num_nodes)
 * before it indexes anything; a bad id sets an error bit and is skipped.  Purely additive: mgx_abi_version() stays 35.
 *
 * mgx_to_block: dst_nodes[num_dst], src[nnz], dst[nnz] are int64 global ids (what the sampler returns).  Writes
 *   src_nodes   int64, capacity num_dst + min(nnz, num_nodes): dst_nodes, then every other source in ASCENDING global id (the order
 *               a sort + unique gives; here from a bitmap of the nodes, walked word by word)
 *   l_src/l_dst [nnz] the edges in local ids, 32- or 64-bit by `out_bits`
 *   indptr      [num_dst + 1] in the same width, only when dst_sorted != 0 (the caller promises that the edges arrive grouped by
 *               destination in dst_nodes order): the row pointer of the in-CSR whose indices are l_src.  May be NULL otherwise.
 *   result      device int64[2]: {num_src, error bits}; error bits: 1 a node twice in dst_nodes, 2 an edge destination that is not in
 *               dst_nodes, 4 an id outside [0, num_nodes), 8 dst_sorted promised but l_dst decreases somewhere.  With an error bit
 *               set the other outputs are unspecified (nothing is written out of bounds).
 *   workspace   mgx_to_block_workspace(num_nodes, nnz) bytes (-1: bad arguments).  num_dst + nnz < 2^31. */
int64_t mgx_to_block_workspace(int64_t num_nodes, int64_t nnz);
int32_t mgx_to_block(int64_t num_nodes, int64_t num_dst, const int64_t* dst_nodes, int64_t nnz, const int64_t* src, const int64_t* dst,
                     int32_t dst_sorted, int32_t out_bits, void* workspace, int64_t* src_nodes, void* l_src, void* l_dst,
                     void* indptr /* may be NULL without dst_sorted */, int64_t* result /* [2] */, void* stream);
/* Node-induced subgraph over the parent's in-CSR `csr` (num_rows == num_cols, either index width): sel_nodes[num_sel] int64, the
 * selected nodes; node sel_nodes[i] becomes i.
 *   _count  fills the look-up table in `workspace` (mgx_node_subgraph_workspace(num_nodes) bytes) and writes counts[i] (int64) = the
 *           in-edges of sel_nodes[i] whose source is selected too.  result: device int64[1] of error bits -- 1 a node twice in
 *           sel_nodes, 4 an id outside [0, num_rows), 16 (no error) the edge ids inside some selected row do not ascend.
 *   The caller takes offsets = exclusive cumsum of counts ([num_sel + 1], int64), reads offsets[num_sel] and the error bits, allocates
 *   l_src / l_dst (out_bits wide) and parent_eid (int64) with offsets[num_sel] entries and calls
 *   _fill   with the same csr / sel_nodes / workspace (unchanged since _count): row i's kept edges go to [offsets[i], offsets[i+1]) in
 *           CSR order -- local source, local destination i, parent edge id (eids[p], or p without eids); never past offsets[i+1].
 * Ballot + prefix popcount inside a row, no atomics: deterministic. */
int64_t mgx_node_subgraph_workspace(int64_t num_nodes);
int32_t mgx_node_subgraph_count(const mgx_csr* csr, int64_t num_sel, const int64_t* sel_nodes, void* workspace, int64_t* counts,
                                int64_t* result /* [1] */, void* stream);
int32_t mgx_node_subgraph_fill(const mgx_csr* csr, int64_t num_sel, const int64_t* sel_nodes, const void* workspace,
                               const int64_t* offsets, int32_t out_bits, void* l_src, void* l_dst, int64_t* parent_eid, void* stream);

/* ------------------------------------------------------------------ link-prediction minibatches (csrc/edgefind.hip, csrc/relabel.hip)
 * What turns a batch of EDGES into a training step (dgl.dataloading.EdgeDataLoader, dgl.dataloading.negative_sampler,
 * end_to_end/sampling/link-prediction/): which edge joins a pair of nodes, k negative destinations per positive edge, the batch's own
 * edges (and their reverses) taken out of the sampled neighbourhoods, and the compaction of the batch's endpoints.  Integer kernels;
 * every id read from a caller's array is checked before it indexes anything.  Purely additive: mgx_abi_version() stays 35.
 *
 * mgx_edge_lookup: `csr` is the in-CSR (rows = destinations, indices = sources) or the out-CSR, the caller passing row_ids / col_ids
 *   (int64, [num_q]) in the matching order.  out_eid[q] = the LOWEST edge id among the positions p of row row_ids[q] with
 *   indices[p] == col_ids[q] -- eids[p], or p when csr->eids is NULL -- and -1 when there is none.  A minimum over all matches: nothing
 *   is assumed about the order inside a row (rows are in edge-id order, not column order, so a lookup is a scan of one row: 16 lanes
 *   per query, coalesced loads, a shuffle reduction, no atomics -- deterministic).  result: device int64[1] of error bits; 4 = a row id
 *   outside [0, num_rows) or a column id outside [0, num_cols): that query gets -1.  num_q < 2^34. */
int32_t mgx_edge_lookup(const mgx_csr* csr, int64_t num_q, const int64_t* row_ids, const int64_t* col_ids,
                        int64_t* out_eid /* [num_q] */, int64_t* result /* [1] error bits */, void* stream);
/* mgx_negative_sample: draw (e, j), e < num_pos, j < k, belongs to positive edge e with source u = pos_src[e] and proposes a
 *   destination uniform on [0, num_dst_nodes), num_dst_nodes < 2^31.  flags: bit 1 (exclude_existing) rejects v' when (u, v') is an edge
 *   of the graph, bit 2 (exclude_self_loops) rejects v' == u.  Try t of the draw uses
 *       r = mix64(rng_seed ^ mix64((e * k + j) * 64 + t)),   v' = ((r >> 32) * num_dst_nodes) >> 32
 *   (mix64: the splitmix64 finaliser; csrc/counter_rng.h), a function of (rng_seed, e, j, t) alone -- never of the launch geometry, the
 *   index width or the form of the CSR.  out_dst[e * k + j] = the first accepted of at most max_tries tries, -1 when all were rejected;
 *   max_tries in [1, 64]: there is no unbounded rejection loop, a source adjacent to every node fails its draws and ends.
 *   csr: NULL exactly when exclude_existing is off.  rows_are_sources != 0: the out-CSR, all k * max_tries checks of one positive edge
 *   scan the row of u; else the in-CSR, scanned at row v'.  Both give the same output.
 *   result: device int64[2] = {failed draws, error bits}; 4 = a source outside the graph (its slots get -1 and are not counted). */
int32_t mgx_negative_sample(const mgx_csr* csr /* NULL iff no exclude_existing */, int32_t rows_are_sources, int64_t num_pos,
                            const int64_t* pos_src, int32_t k, int64_t num_dst_nodes, int32_t flags, int32_t max_tries, uint64_t rng_seed,
                            int64_t* out_dst /* [num_pos * k] */, int64_t* result /* [2] */, void* stream);
/* Seed-edge exclusion.  A frontier is what the samplers return: edges grouped by seed, seed s owning [offsets[s], offsets[s + 1])
 * ([num_seeds + 1] int64) of `src` / `eid` (idx_bits wide).  An edge is dropped when its edge id occurs in excl_sorted[num_excl]
 * (int64, ASCENDING; a few thousand ids, searched by bisection -- no bitmap over all edges to clear per batch).  DGL's semantics:
 * sample first, then remove, so a seed may end with fewer than `fanout` edges.
 *   _count  counts[s] (int64) = the kept edges of seed s.  The caller takes new_offsets = exclusive cumsum ([num_seeds + 1]), reads
 *           new_offsets[num_seeds] once, allocates out_src / out_eid (idx_bits wide) and calls
 *   _fill   with the same arguments: the kept edges of seed s in their order at [new_offsets[s], new_offsets[s + 1]), never past it.
 * Ballot + prefix popcount inside a seed, no atomics: deterministic. */
int32_t mgx_frontier_exclude_count(int64_t num_seeds, const int64_t* offsets, const void* eid, int32_t idx_bits, int64_t num_excl,
                                   const int64_t* excl_sorted, int64_t* counts /* [num_seeds] */, void* stream);
int32_t mgx_frontier_exclude_fill(int64_t num_seeds, const int64_t* offsets, const void* eid, int32_t idx_bits, int64_t num_excl,
                                  const int64_t* excl_sorted, const void* src, const int64_t* new_offsets, void* out_src, void* out_eid,
                                  void* stream);
/* mgx_compact_nodes: ids[n] (int64, values in [0, num_nodes), repeats allowed, n < 2^31) -> nodes = the distinct ids in ASCENDING order
 *   (int64, capacity min(n, num_nodes)) and local[i] = the position of ids[i] in nodes (out_bits wide): what sort + unique + inverse
 *   give, from the node bitmap of mgx_to_block walked word by word -- no sort.  result: device int64[2] = {number of distinct ids,
 *   error bits}; 4 = an id out of range (skipped; its local entry is 0).  workspace: mgx_compact_nodes_workspace(num_nodes, n) bytes
 *   (-1: bad arguments). */
int64_t mgx_compact_nodes_workspace(int64_t num_nodes, int64_t n);
int32_t mgx_compact_nodes(int64_t num_nodes, int64_t n, const int64_t* ids, int32_t out_bits, void* workspace,
                          int64_t* nodes /* capacity min(n, num_nodes) */, void* local /* [n] */, int64_t* result /* [2] */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI355X_GRAPH_H_ */
