"""Settings of the host layer.

USER switches are environment variables, read where they are used; the complete list is the table in README.md ("Switches"):
    MGX_LIB_PATH  MGX_DATA_ROOT  MGX_CACHE_DIR  MGX_SCHEDULE  MGX_TILE  MGX_GAT_TILE  MGX_GAT_FUSED  MGX_TORCH_OPS  MGX_SDDMM_WALK
    MGX_SPARSE_HALO  MGX_ACCELERATE_LINEAR  MGX_SAGE_SPARSE_LAST  MGX_SAGE_HEAD_ROWS  MGX_SAGE_HEAD_SLOTS  MGX_XTY_MASKED  MGX_SAGE_L1_PROJECT_FIRST  MGX_PLAIN_MODEL  MGX_HOST_THREADS
(+ the bench / test hooks MGX_DIST_BACKEND, MGX_BENCH_SHARE_GPU, MGX_BENCH_TUNABLEOP, MGX_BENCH_STEP_TIMES, MGX_DATASET_SCALE).

Everything below is NOT a user switch: module attributes with fixed defaults that choose between a fused form and the composition it
stands for (both kept: the composition is the fallback for shapes the fused kernel does not take, and the tests compare the two), or
hold a measured constant.  Tests flip them with monkeypatch.setattr(config, ...).  Variants that were measured and lost (per-slot LDS
flags, shrinking tail tiles, the tile kernel's direct part as its own launch, longest-tile-first dispatch, 8 waves per SIMD, the own-matrix
backward, ...) are not switches any more: their code is gone, their numbers are in docs/LOG_r0*.md.
"""

# ---- SAGEConv forms (ops.py, dist.py, full_graph.py)
SAGE_FUSED_LAYER = True    # a mean-aggregator layer as ONE autograd node (ops.SageMeanLayerFn / SageMeanCatFn)
SAGE_CAT = True            # ... over an [h | neigh] buffer: one GEMM per layer (ops.CatBuffer)
SAGE_STATIC_CAT = True     # an unmodified input tensor stays resident in that buffer (identity + version counter)
SAGE_FUSED_ADD = True      # fc_self(h) + fc_neigh(neigh) as two GEMMs, the second accumulating (ops.linear_sum)
SAGE_FUSED_ACT = True      # relu + dropout in the layer GEMM's epilogue (mgx_rows_gemm_relu_dropout)
SAGE_PROJECT_FIRST = True  # project before aggregating when that moves fewer columns (reddit: 602 -> 16)
SAGE_HEAD_ROWS = True      # the last layer's dense work on the loss rows only (ops.SageMeanCatHeadFn; MGX_SAGE_HEAD_ROWS=0 turns it off)
SAGE_HEAD_INIT = True      # ... its reversed aggregation started from the compact d self (mgx_spmm_copy_u_strided_init), d neigh / deg scattered into
                           # one [N, K] matrix kept zero elsewhere between steps (ops._head_dn): no zero fill, no copy of d self into one
SAGE_HEAD_SLOTS = True     # ... and, on a graph of PACKED_GATHER_MIN_NNZ edges with K = 64, gathering that matrix behind its 128-byte slots kept beside it: an
                           # empty slot's first word per zero row, the dense row otherwise (mgx_spmm_copy_u_slots_init, same bits; MGX_SAGE_HEAD_SLOTS=0 turns it off)
SAGE_HEAD_SLOTS_MIN_NNZ = 12_000_000  # ... from this many edges on (or PACKED_GATHER_MIN_NNZ where that is lower): products shape x 0.1 / 0.2 / 0.3 / 0.5 / 1,
                           # dense call 0.225 / 0.412 / 0.635 / 1.091 / 2.289 ms, this call 0.162 / 0.291 / 0.445 / 0.731 / 1.506 ms (docs/LOG_head_probe.md);
                           # not measured below 12 M edges
ROWS_GEMM = True           # mgx_rows_gemm for the projections of a layer over >= 65 536 rows (else the library GEMM)
LINEAR_XTY = True          # tall-skinny weight gradients by mgx_xty (else the library GEMM)
XTY_COLSUM = True          # ... with the bias gradient from the same pass (mgx_xty_colsum)
XTY_MASKED = True          # ... and, behind relu + dropout where d z is needed for nothing else, the mask applied on load: d z is never
                           # stored (mgx_xty_colsum_masked, same bits; MGX_XTY_MASKED=0 restores relu_dropout_bwd + xty)

# ---- GAT (nn.py, sparse.py)
GAT_AGG_FIRST = True       # aggregate before projecting when in_feats < heads * out_feats
GAT_PACK = True            # one packed gather operand per node for the fused walks (mgx_gat_fused_pack_workspace); False: separate arrays

# ---- dot-product attention (ops.dot_attention, nn.DotGatConv)
DOT_ATTENTION_FUSED = True  # the fused walks of csrc/dotattn.hip; False: u_dot_v -> edge_softmax -> u_mul_e/sum through the existing operators
# ---- relu(x_u + w_e) messages summed per destination (ops.gine_sum, nn.GINEConv, graph_classification.py --fused-message)
GINE_FUSED = True  # the fused walks of csrc/gine.hip; False: gather -> add -> relu -> mul -> copy_e/sum through the existing operators
# ---- sum / mean / var / std / max / min of the same messages at once (ops.multi_aggregate, nn.PNAConv, graph_classification.py --model pna)
MULTI_AGG_FUSED = True  # the fused walks of csrc/multiagg.hip; False: one g-SpMM per aggregate through the existing operators
# ONE of sum / mean / max / min without edge features is a single g-SpMM as a composition; the fused form walks the graph once as well
# and has the longer host path.  pna_bench.py, forward + backward, fused / composed per call (docs/LOG_pna.md):
#   sum, mean   lose 0.75 - 0.81x at D = 64 on all four batches (3 090 ... 110 036 edges) and at D = 256 up to 73 600 edges; win 1.07x /
#               1.14x only on the 2048-graph batch at D = 256 -- given up: a single sum or mean always takes the g-SpMM
#   max, min    D = 64: lose 0.92x (88 against 81 us) at 3 090 and 13 266 edges, win 1.2 - 1.4x at 73 600 and 110 036; D = 256: win
#               everywhere (1.4 - 5.2x).  Widths between 64 and 256 were not measured: the gate covers the measured losing region only.
MULTI_AGG_SINGLE_SUM_FUSED = False  # a single sum or mean without w: the fused walk (True) or the g-SpMM
MULTI_AGG_SINGLE_MIN_EDGES = 16384  # a single max or min without w, D <= MULTI_AGG_SINGLE_MAX_D, fewer edges than this: the g-SpMM
MULTI_AGG_SINGLE_MAX_D = 64

# ---- graph readout (ops.segment_attention, nn.GlobalAttentionPooling, nn.Set2Set)
SEGMENT_ATTENTION_FUSED = True  # the fused pair of csrc/segattn.hip; False: segment max -> gather -> exp -> segment sum -> gather -> multiply -> segment sum

# ---- segment top-k (ops.segment_topk, readout.topk_nodes / topk_edges, nn.SortPooling)
SEGMENT_TOPK_FUSED = True  # csrc/segtopk.hip, one launch each way; False: two stable sorts and gathers in torch operators

# ---- point clouds (ops.segment_knn, transform.knn_graph / segmented_knn_graph, nn.EdgeConv; ops.segment_fps, ops.segment_ball_query,
#      transform.fixed_radius_block, nn.PointNetConv)
KNN_FUSED = True       # csrc/knn.hip: distances and selection in one launch; False: a stable sort of direct-form distances per segment in torch operators
KNN_QUERY_FUSED = True  # ops.segment_knn_query (queries into a reference set; transform.knn_block, nn.FeaturePropagation) through the same
                        # kernel, weights included; False: the same composition per segment
EDGECONV_FUSED = True  # EdgeConv without batch norm as theta GEMM over nodes -> copy_u / max -> + x (phi - theta)^T: no E-sized tensor; False:
                       # u_sub_v -> the two Linears over edges -> copy_e / max
FPS_FUSED = True         # csrc/fps.hip: the whole sampling chain of a cloud in one workgroup of one launch; False: the same loop in torch operators
BALL_QUERY_FUSED = True  # csrc/ballquery.hip: distances and first-K selection in one launch; False: per-segment distances and a cumsum in torch operators
POINTNETCONV_FUSED = True  # PointNetConv with one layer and no batch norm as a GEMM over the points -> copy_u / max -> relu(. - centre term): no
                           # E-sized tensor; False: u_sub_v -> relu -> copy_e / max

# ---- sampled blocks and induced subgraphs (sampling.to_block, sampling.node_subgraph)
DEVICE_BLOCKS = True    # the relabelling kernels of csrc/relabel.hip; False: look-up table -> unique -> gathers -> bincount + cumsum in torch ops
DEVICE_SUBGRAPH = True  # a wave per selected row of a materialised in-CSR (csrc/relabel.hip); False: the look-up table gathered at both ends of every parent edge

# ---- link-prediction minibatches (linkpred.py, sampling.exclude_frontier_edges, DGLGraph.has_edges_between)
DEVICE_LINKPRED = True  # edge lookup, negative sampling (csrc/edgefind.hip), seed-edge exclusion and compaction (csrc/relabel.hip); False: the
                        # torch compositions of the same semantics -- the same result bit for bit, the negatives' random stream included

# ---- schedules (schedule.py, tileplan.py)
PLAN_BUILDER = "device"    # "device" (mgx_spmm_plan_count / _fill) | "torch" | "host": the same tables three ways (tests compare them)
HUB_SPLIT = 256            # rows longer than this become several work items (256 measured best on MI355X; 1024: +5..10 %)
LP_ROUNDS = 8              # label-propagation rounds of the locality order
CLUSTER_MIN_NNZ = 4_000_000   # smaller graphs keep their natural row order
TILE_HUB_SPLIT = 2048      # hub threshold of the tile kernel's work items
TILE_CONFIG = {4: (7, 6, 1, 3), 3: (7, 3, 1, 3), 2: (7, 3, 1, 2)}   # lanes_log2 -> (consumers, nacc, loaders, tau)
GAT_TILE_CONFIG = (7, 3, 1, 2)
TILE_MIN_WIDTH = 4         # rows of 4 .. 20 columns take the 16-column tile pass, 24 .. 44 the 32-column one, wider the 64-column one
TILE_VALIDATE = True       # check every tile plan's tables on the device before a kernel may walk them (a dozen reductions per plan)
SHORT_ROWS_IMBALANCE = 6.0    # two-part plans: sum over batches of max(len) * B may exceed the short edges by at most this factor

# ---- row-sparse gradients, wide rows (sparse.py)
SPARSE_GRAD = False        # skip all-zero rows of a gradient in the reversed aggregation (measured: no gain on dense gradients)
SPARSE_GRAD_MIN_NNZ = 2_000_000
WIDE_PAD = True            # rows wider than 256 columns on dense graphs: line-padded passes
WIDE_PAD_MIN_NNZ = 1 << 20

# ---- mostly-zero rows as 128-byte slots (ops._packed_rows, csrc/spmm_slots.inc)
PACKED_GATHER = True       # the forward aggregation of a [N, 64] relu + dropout output gathers one 128-byte slot per edge instead of the 256-byte row
PACKED_GATHER_MIN_NNZ = 20_000_000   # products shape x 0.1 / 0.2 / 0.3 / 0.5 / 1 (12 .. 124 M edges): dense 0.21 / 0.39 / 0.59 / 1.02 / 2.13 ms, slots +
                                     # pack pass 0.21 / 0.36 / 0.53 / 0.82 / 1.62 ms: small operands sit in L2 / MALL, where whole rows are cheap
PACKED_GATHER_PROBE = True          # dgl.ops.gspmm / update_all(copy_u, sum | mean) of an UNTAGGED [N, 64] operand on such a graph: pack it and let the overflow count decide
PACKED_GATHER_MAX_OVERFLOW = 0.10    # share of rows with more than 24 non-zeros (read from the dense matrix) above which the dense kernels are used

# ---- a constant 100-column input as [N, 96] + its last four columns along the edge list (ops._edge_tail_operands, csrc/spmm_tail.inc)
EDGE_TAIL = True           # products layer 1: 4.74 -> 4.09 ms per aggregation, for 16 bytes per edge (2 GB) + the [N, 96] copy, laid out once
EDGE_TAIL_MIN_NNZ = 20_000_000
