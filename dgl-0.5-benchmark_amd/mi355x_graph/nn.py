"""dgl.nn.pytorch modules used by the benchmark scripts, written against this backend's ops:
  GATConv    main_dgl_reddit_gat.py:10,31-55 (u_add_v SDDMM + fused edge_softmax + u_mul_e/sum SpMM)
  DotGatConv dgl.nn.pytorch.DotGatConv (u_dot_v SDDMM + edge_softmax + u_mul_e/sum SpMM, fused: ops.dot_attention)
  GINEConv   dgl.nn.pytorch.GINEConv (sum of relu(h_u + e_uv) messages, fused: ops.gine_sum)
  PNAConv    dgl.nn.pytorch.PNAConv (mean / max / min / std ... of one message per edge, fused: ops.multi_aggregate)
  SAGEConv   main_dgl_arxiv_sage_nn.py:9,27-34
  GraphConv  main_dgl_enzymes_gcn_nn.py:12,29-36
  AvgPooling / SumPooling / MaxPooling   main_dgl_molhiv_gcn.py:75,93
  GlobalAttentionPooling / Set2Set / WeightAndSum   dgl.nn.pytorch.glob (attention readouts, fused: ops.segment_attention)
  SortPooling   dgl.nn.pytorch.glob (the DGCNN readout: ops.segment_topk)
  KNNGraph / SegmentedKNNGraph   dgl.nn.pytorch.factory (ops.segment_knn);  EdgeConv   dgl.nn.pytorch.conv (point clouds)
  FarthestPointSampler   dgl.geometry.pytorch (ops.segment_fps);  FixedRadiusNNGraph   the PointNet++ grouping (ops.segment_ball_query);  PointNetConv   its message
  FeaturePropagation   the PointNet++ decoder level (ops.segment_knn_query + u_mul_e / sum: transform.knn_interpolate)
Parameter names, shapes and initialisation follow DGL v0.6.x so state_dicts and the scripts'
reset_parameters() calls (main_dgl_reddit_gat.py:57-59) line up.
"""
import math
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from ._lib import DGLError
from . import function as fn
from . import config
from . import ops
from .utils import expand_as_pair


def _has_zero_in_degree(graph):
    index = getattr(graph, "_index", None)
    if index is not None and hasattr(index, "has_zero_in_degree"):
        return index.has_zero_in_degree()
    return bool((graph.in_degrees() == 0).any())


class Linear(nn.Linear):
    """torch.nn.Linear (same parameters, init and state_dict) whose bias gradient runs in the library's column-sum kernel."""

    def forward(self, input):
        return ops.linear(input, self.weight, self.bias)


class BatchNorm1d(nn.BatchNorm1d):
    """torch.nn.BatchNorm1d (same parameters, buffers and state_dict) over node features [N, C]: in training mode the
    statistics, the normalisation and their gradients run in the library's column kernels (PyTorch's channels-last
    batch-norm kernels need 0.6-0.9 ms for [169 k, 256]; the data is 173 MB).  Evaluation mode, C > 256 or C % 4 != 0 and
    non-2-D inputs take the PyTorch path."""

    def forward(self, input):
        use_batch = self.training or not self.track_running_stats
        if not use_batch or not ops.batch_norm_supported(input):
            return super(BatchNorm1d, self).forward(input)
        y, mean, var = ops.BatchNormFn.apply(input, self.weight, self.bias, self.eps)
        if self.training and self.track_running_stats:
            with torch.no_grad():
                self.num_batches_tracked.add_(1)
                m = self.momentum if self.momentum is not None else 1.0 / float(self.num_batches_tracked)
                n = input.shape[0]
                self.running_mean.mul_(1 - m).add_(mean, alpha=m)
                self.running_var.mul_(1 - m).add_(var, alpha=m * n / (n - 1))
        return y


class Identity(nn.Module):
    def forward(self, x):
        return x


class GATConv(nn.Module):
    def __init__(self, in_feats, out_feats, num_heads, feat_drop=0., attn_drop=0., negative_slope=0.2,
                 residual=False, activation=None, allow_zero_in_degree=False, bias=True):
        super(GATConv, self).__init__()
        self._num_heads = num_heads
        self._in_src_feats, self._in_dst_feats = expand_as_pair(in_feats)
        self._out_feats = out_feats
        self._allow_zero_in_degree = allow_zero_in_degree
        if isinstance(in_feats, tuple):
            self.fc_src = Linear(self._in_src_feats, out_feats * num_heads, bias=False)
            self.fc_dst = Linear(self._in_dst_feats, out_feats * num_heads, bias=False)
        else:
            self.fc = Linear(self._in_src_feats, out_feats * num_heads, bias=False)
        self.attn_l = nn.Parameter(torch.FloatTensor(size=(1, num_heads, out_feats)))
        self.attn_r = nn.Parameter(torch.FloatTensor(size=(1, num_heads, out_feats)))
        self.feat_drop = nn.Dropout(feat_drop)
        self.attn_drop = nn.Dropout(attn_drop)
        self.leaky_relu = nn.LeakyReLU(negative_slope)
        if bias:
            self.bias = nn.Parameter(torch.FloatTensor(size=(num_heads * out_feats,)))
        else:
            self.register_buffer("bias", None)
        if residual:
            if self._in_dst_feats != out_feats:
                self.res_fc = Linear(self._in_dst_feats, num_heads * out_feats, bias=False)
            else:
                self.res_fc = Identity()
        else:
            self.register_buffer("res_fc", None)
        self.reset_parameters()
        self.activation = activation

    def reset_parameters(self):
        gain = nn.init.calculate_gain("relu")
        if hasattr(self, "fc"):
            nn.init.xavier_normal_(self.fc.weight, gain=gain)
        else:
            nn.init.xavier_normal_(self.fc_src.weight, gain=gain)
            nn.init.xavier_normal_(self.fc_dst.weight, gain=gain)
        nn.init.xavier_normal_(self.attn_l, gain=gain)
        nn.init.xavier_normal_(self.attn_r, gain=gain)
        if self.bias is not None:
            nn.init.constant_(self.bias, 0)
        if isinstance(self.res_fc, nn.Linear):
            nn.init.xavier_normal_(self.res_fc.weight, gain=gain)

    def set_allow_zero_in_degree(self, set_value):
        self._allow_zero_in_degree = set_value

    def _aggregate_first(self, graph, feat, get_attention):
        """One-head layers that WIDEN (in < out, e.g. 16 hidden -> 41 classes): aggregate the input rows, project afterwards.
        Taken when the fused block exists for the input width and it saves a 16-column gather pass; config.GAT_AGG_FIRST = False: never."""
        if (self._num_heads != 1 or isinstance(feat, tuple) or get_attention or not hasattr(self, "fc") or not torch.is_tensor(feat)
                or feat.dim() != 2 or not config.GAT_AGG_FIRST):
            return False
        k, f = self._in_src_feats, self._out_feats
        if k % 4 != 0 or (k + 15) // 16 >= (f + 15) // 16:
            return False
        if self.training and self.attn_drop.p > 0.0 and feat.is_cuda and ops.capture_path():
            return False  # frozen mask under capture: see forward
        return ops.gat_fused_supported(graph, feat.view(feat.shape[0], 1, k))

    def _forward_on_partition(self, graph, feat):
        """A partition of the graph (dist.DistGraph): every owned node has all its in-edges here, its remote in-neighbours'
        rows travel ONCE per layer -- the layer's input or its projection, whichever is narrower (reddit: 602 -> 16: the 16 projected
        columns) -- through the halo exchange (autograd adds the halo rows' gradients back into their owners), and the layer then
        runs on the local block graph [owned | halo] -> owned exactly as on a sampled block."""
        h = self.feat_drop(feat)
        blk = graph._block
        if self._in_src_feats <= self._num_heads * self._out_feats:
            return self.forward(blk, graph.halo_exchange(h), _dropped=True)
        proj = graph.halo_exchange(self.fc(h))                      # [n_own + n_halo, H * F]
        return self.forward(blk, h, _projected=proj)

    def forward(self, graph, feat, get_attention=False, _dropped=False, _projected=None):
        if hasattr(graph, "halo_exchange") and _projected is None and not _dropped:
            if isinstance(feat, tuple) or get_attention or not hasattr(self, "fc"):
                raise DGLError("GATConv on a partitioned graph takes one feature tensor of the owned nodes (no attention output)")
            return self._forward_on_partition(graph, feat)
        with graph.local_scope():
            if not self._allow_zero_in_degree:
                if _has_zero_in_degree(graph):
                    raise DGLError(
                        "There are 0-in-degree nodes in the graph, output for those nodes will be invalid. "
                        "This is harmful for some applications, causing silent performance regression. "
                        "Adding self-loop on the input graph by calling `g = dgl.add_self_loop(g)` will resolve "
                        "the issue. Setting ``allow_zero_in_degree`` to be `True` when constructing this module "
                        "will suppress the check and let the code run.")
            if _projected is None and self._aggregate_first(graph, feat, get_attention):
                # ONE head: a[e] is a scalar, so sum_e a[e] (h[u] W^T) = (sum_e a[e] h[u]) W^T and el = h (W^T attn_l): the
                # fused block runs at the INPUT width and the projection follows it (reddit GAT's 16 -> 41 output layer:
                # three gather walks at 64-byte rows instead of 164-byte ones).  Same function, other fp32 summation order.
                h = feat if _dropped else self.feat_drop(feat)
                w = self.fc.weight                                    # [F, in]
                v = torch.cat([self.attn_l.view(1, -1), self.attn_r.view(1, -1)], 0) @ w  # [2, in]
                lr = h @ v.t()                                        # [N, 2]: el, er
                n_dst = graph.number_of_dst_nodes()
                el, er = lr[:, 0:1].unsqueeze(-1), lr[:n_dst, 1:2].unsqueeze(-1)
                agg = ops.gat_fused(graph, h.view(h.shape[0], 1, -1), el.contiguous(), er.contiguous(),
                                    self.leaky_relu.negative_slope, self.attn_drop.p, self.training)
                rst = (agg.view(n_dst, -1) @ w.t()).view(n_dst, 1, self._out_feats)
                if self.res_fc is not None:
                    rst = rst + self.res_fc(h[:n_dst]).view(n_dst, -1, self._out_feats)
                if self.bias is not None:
                    rst = ops.bias_add(rst, self.bias)
                if self.activation:
                    rst = self.activation(rst)
                return rst
            if _projected is not None:  # a partition: `feat` = the owned rows after feat_drop, `_projected` = fc of [owned | halo]
                h_dst = feat
                feat_src = _projected.view(-1, self._num_heads, self._out_feats)
                feat_dst = feat_src[:graph.number_of_dst_nodes()]
            elif isinstance(feat, tuple):
                h_src = self.feat_drop(feat[0])
                h_dst = self.feat_drop(feat[1])
                if not hasattr(self, "fc_src"):
                    feat_src = self.fc(h_src).view(-1, self._num_heads, self._out_feats)
                    feat_dst = self.fc(h_dst).view(-1, self._num_heads, self._out_feats)
                else:
                    feat_src = self.fc_src(h_src).view(-1, self._num_heads, self._out_feats)
                    feat_dst = self.fc_dst(h_dst).view(-1, self._num_heads, self._out_feats)
            else:
                h_src = h_dst = feat if _dropped else self.feat_drop(feat)
                feat_src = feat_dst = self.fc(h_src).view(-1, self._num_heads, self._out_feats)
                if graph.is_block:
                    feat_dst = feat_src[:graph.number_of_dst_nodes()]
                    h_dst = h_dst[:graph.number_of_dst_nodes()]
            if ops.head_dot_supported(feat_src):  # one pass over feat instead of product + last-dim reduction
                if feat_dst is feat_src:
                    el, er = ops.head_dot(feat_src, self.attn_l, self.attn_r)
                else:
                    el, er = ops.head_dot(feat_src, self.attn_l), ops.head_dot(feat_dst, self.attn_r)
                el, er = el.unsqueeze(-1), er.unsqueeze(-1)
            else:
                el = (feat_src * self.attn_l).sum(dim=-1).unsqueeze(-1)
                er = (feat_dst * self.attn_r).sum(dim=-1).unsqueeze(-1)
            rst = None
            # Under HIP-graph capture the fused block's attn_drop seed would be a frozen launch argument -- every replay the
            # same mask -- so a dropping layer takes the unfused path there (nn.Dropout is capture-safe); ADVICE r02.
            frozen_mask = self.training and self.attn_drop.p > 0.0 and feat_src.is_cuda and ops.capture_path()
            if not get_attention and not frozen_mask and ops.gat_fused_supported(graph, feat_src):
                # the whole block u_add_v -> leaky_relu -> edge_softmax -> attn_drop -> u_mul_e/sum without any E x H tensor
                rst = ops.gat_fused(graph, feat_src, el, er, self.leaky_relu.negative_slope, self.attn_drop.p, self.training,
                                    attn_l=self.attn_l)  # el = (feat_src * attn_l).sum(-1), whichever branch above formed it
            # e and a are internal to the module: keep them in in-CSR (destination-major) edge order so that
            # u_add_v, edge_softmax and u_mul_e/sum stream them instead of gathering by edge id
            cidx, perm = graph._index.canonical() if rst is None else (None, None)
            if rst is not None:
                pass
            elif int(el.shape[1]) <= 64:  # fused u_add_v -> leaky_relu -> edge_softmax: the logits are never materialised
                a = self.attn_drop(ops.gat_attention(cidx, el, er, self.leaky_relu.negative_slope))
            else:
                e = self.leaky_relu(ops.gsddmm(cidx, "add", el, er, "u", "v"))
                a = self.attn_drop(ops.edge_softmax(cidx, e))
            if rst is None:
                rst = ops.gspmm(cidx, "mul", "sum", feat_src, a)
            if self.res_fc is not None:
                resval = self.res_fc(h_dst).view(h_dst.shape[0], -1, self._out_feats)
                rst = rst + resval
            if self.bias is not None:
                rst = ops.bias_add(rst, self.bias)
            if self.activation:
                rst = self.activation(rst)
            if get_attention:
                if perm is not None:  # back to the caller's edge-id order
                    a_user = torch.empty_like(a)
                    a_user[perm.long()] = a
                    a = a_user
                return rst, a
            return rst


class DotGatConv(nn.Module):
    """dgl.nn.pytorch.DotGatConv: scaled dot-product attention over the in-edges, h'_v = sum_{u->v} softmax_u(<W h_v, W h_u> / sqrt(F)) W h_u
    per head, with ONE bias-free projection `fc` for both roles.  The block between the projection and the result is
    ops.dot_attention (csrc/dotattn.hip when it takes the shape); get_attention=True runs the operators one by one and also returns
    the attention [E, H, 1] in edge-id order."""

    def __init__(self, in_feats, out_feats, num_heads, allow_zero_in_degree=False):
        super(DotGatConv, self).__init__()
        self._in_src_feats, self._in_dst_feats = expand_as_pair(in_feats)
        self._out_feats = out_feats
        self._num_heads = num_heads
        self._allow_zero_in_degree = allow_zero_in_degree
        self.fc = Linear(self._in_src_feats, out_feats * num_heads, bias=False)  # a pair of inputs shares it, as in DGL

    def set_allow_zero_in_degree(self, set_value):
        self._allow_zero_in_degree = set_value

    def forward(self, graph, feat, get_attention=False):
        with graph.local_scope():
            if not self._allow_zero_in_degree:
                if _has_zero_in_degree(graph):
                    raise DGLError(
                        "There are 0-in-degree nodes in the graph, output for those nodes will be invalid. "
                        "This is harmful for some applications, causing silent performance regression. "
                        "Adding self-loop on the input graph by calling `g = dgl.add_self_loop(g)` will resolve "
                        "the issue. Setting ``allow_zero_in_degree`` to be `True` when constructing this module "
                        "will suppress the check and let the code run.")
            if isinstance(feat, tuple):
                feat_src = self.fc(feat[0]).view(-1, self._num_heads, self._out_feats)
                feat_dst = self.fc(feat[1]).view(-1, self._num_heads, self._out_feats)
            else:
                feat_src = feat_dst = self.fc(feat).view(-1, self._num_heads, self._out_feats)
                if graph.is_block:
                    feat_dst = feat_src[:graph.number_of_dst_nodes()]
            scale = float(self._out_feats) ** -0.5
            if not get_attention:  # q, k and v are one tensor here: k and v are gathered once, autograd sums the three gradients
                return ops.dot_attention(graph, feat_dst, feat_src, feat_src, scale)
            a = ops.edge_softmax(graph, ops.gsddmm(graph, "dot", feat_src, feat_dst, "u", "v") * scale)
            return ops.gspmm(graph, "mul", "sum", feat_src, a), a


class SAGEConv(nn.Module):
    def __init__(self, in_feats, out_feats, aggregator_type, feat_drop=0., bias=True, norm=None, activation=None):
        super(SAGEConv, self).__init__()
        if aggregator_type not in ("mean", "gcn", "pool"):
            raise DGLError("Unsupported aggregator type %r on this backend (mean, gcn, pool)" % (aggregator_type,))
        self._in_src_feats, self._in_dst_feats = expand_as_pair(in_feats)
        self._out_feats = out_feats
        self._aggre_type = aggregator_type
        self.norm = norm
        self.feat_drop = nn.Dropout(feat_drop)
        self.activation = activation
        if aggregator_type == "pool":
            self.fc_pool = Linear(self._in_src_feats, self._in_src_feats)
        if aggregator_type != "gcn":
            self.fc_self = Linear(self._in_dst_feats, out_feats, bias=bias)
        self.fc_neigh = Linear(self._in_src_feats, out_feats, bias=bias)
        self.reset_parameters()

    def reset_parameters(self):
        gain = nn.init.calculate_gain("relu")
        if self._aggre_type == "pool":
            nn.init.xavier_uniform_(self.fc_pool.weight, gain=gain)
        if self._aggre_type != "gcn":
            nn.init.xavier_uniform_(self.fc_self.weight, gain=gain)
        nn.init.xavier_uniform_(self.fc_neigh.weight, gain=gain)

    def forward(self, graph, feat):
        with graph.local_scope():
            if isinstance(feat, tuple):
                feat_src = self.feat_drop(feat[0])
                feat_dst = self.feat_drop(feat[1])
            else:
                feat_src = feat_dst = self.feat_drop(feat)
                if graph.is_block:
                    feat_dst = feat_src[:graph.number_of_dst_nodes()]
            h_self = feat_dst
            if graph.number_of_edges() == 0:
                graph.dstdata["neigh"] = torch.zeros(feat_dst.shape[0], self._in_src_feats).to(feat_dst)
            # aggregate after the projection when that moves fewer bytes (DGL's lin_before_mp)
            lin_before_mp = self._in_src_feats > self._out_feats
            if self._aggre_type == "mean":
                graph.srcdata["h"] = self.fc_neigh(feat_src) if lin_before_mp else feat_src
                graph.update_all(fn.copy_src("h", "m"), fn.mean("m", "neigh"))
                h_neigh = graph.dstdata["neigh"]
                if not lin_before_mp:
                    h_neigh = self.fc_neigh(h_neigh)
            elif self._aggre_type == "gcn":
                graph.srcdata["h"] = feat_src
                graph.dstdata["h"] = feat_dst
                graph.update_all(fn.copy_src("h", "m"), fn.sum("m", "neigh"))
                degs = graph.in_degrees().to(feat_dst)
                h_neigh = (graph.dstdata["neigh"] + graph.dstdata["h"]) / (degs.unsqueeze(-1) + 1)
                h_neigh = self.fc_neigh(h_neigh)
            else:  # pool
                graph.srcdata["h"] = F.relu(self.fc_pool(feat_src))
                graph.update_all(fn.copy_src("h", "m"), fn.max("m", "neigh"))
                h_neigh = self.fc_neigh(graph.dstdata["neigh"])
            rst = h_neigh if self._aggre_type == "gcn" else self.fc_self(h_self) + h_neigh
            if self.activation is not None:
                rst = self.activation(rst)
            if self.norm is not None:
                rst = self.norm(rst)
            return rst


class RelGraphConv(nn.Module):
    """Edge-weighted relational graph convolution, the layer of main_dgl_proteins_rgcn_for.py:14-60 (every pair of connected nodes
    carries an edge of every relation, each with a prior weight):

        h_v = act( sum_r (mean_{e: u -> v} w[e, r] * x_u) W_r  +  skip(x_v) ),  then dropout.

    Parameters are the script's -- `_rel_fcs`, R matrices [in, out] with kaiming_uniform_(a = sqrt(5)), and `_skip` = Linear(in, out)
    -- so a state_dict moves across.  The R aggregations are ONE ops.rel_gspmm over the graph, and the R products with their sum are one
    GEMM [N, R * in] x [R * in, out] against the stacked `_rel_fcs` (the sum over relations is the GEMM's K dimension)."""

    def __init__(self, in_feats, out_feats, num_relations, activation=None, dropout=0.):
        super(RelGraphConv, self).__init__()
        self._num_relations, self._in_feats, self._out_feats = num_relations, in_feats, out_feats
        self._rel_fcs = nn.ParameterList([nn.Parameter(torch.empty(in_feats, out_feats)) for _ in range(num_relations)])
        self._skip = nn.Linear(in_feats, out_feats, bias=True)
        self._activation = activation
        self._dropout = nn.Dropout(dropout)
        self.reset_parameters()

    def reset_parameters(self):
        for rel_fc in self._rel_fcs:
            nn.init.kaiming_uniform_(rel_fc, a=math.sqrt(5))
        self._skip.reset_parameters()

    def forward(self, g, node_feats, edge_weights):
        """edge_weights: an [E, R] matrix in edge-id order, or the script's list of R [E, 1] columns."""
        w = ops.rel_weight_matrix(g, edge_weights)
        if w.shape[1] != self._num_relations:
            raise DGLError("RelGraphConv: %d relations, got edge weights of %d" % (self._num_relations, w.shape[1]))
        agg = ops.rel_gspmm(g, node_feats, w, "mean")                          # [N_dst, R, in]
        stacked = torch.cat(list(self._rel_fcs), 0)                            # [R * in, out]
        h_dst = node_feats[:agg.shape[0]]
        h = torch.matmul(agg.reshape(agg.shape[0], -1), stacked) + self._skip(h_dst)
        if self._activation:
            h = self._activation(h)
        return self._dropout(h)


class GraphConv(nn.Module):
    def __init__(self, in_feats, out_feats, norm="both", weight=True, bias=True, activation=None,
                 allow_zero_in_degree=False):
        super(GraphConv, self).__init__()
        if norm not in ("none", "both", "right"):
            raise DGLError('Invalid norm value. Must be either "none", "both" or "right". But got "%s".' % norm)
        self._in_feats, self._out_feats, self._norm = in_feats, out_feats, norm
        self._allow_zero_in_degree = allow_zero_in_degree
        if weight:
            self.weight = nn.Parameter(torch.Tensor(in_feats, out_feats))
        else:
            self.register_parameter("weight", None)
        if bias:
            self.bias = nn.Parameter(torch.Tensor(out_feats))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()
        self._activation = activation

    def reset_parameters(self):
        if self.weight is not None:
            nn.init.xavier_uniform_(self.weight)
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    def set_allow_zero_in_degree(self, set_value):
        self._allow_zero_in_degree = set_value

    def forward(self, graph, feat, weight=None):
        with graph.local_scope():
            if not self._allow_zero_in_degree and _has_zero_in_degree(graph):
                raise DGLError("There are 0-in-degree nodes in the graph, output for those nodes will be invalid. "
                               "Adding self-loop on the input graph by calling `g = dgl.add_self_loop(g)` will "
                               "resolve the issue. Setting ``allow_zero_in_degree`` to be `True` when constructing "
                               "this module will suppress the check and let the code run.")
            feat_src, feat_dst = expand_as_pair(feat, graph)
            if self._norm == "both":
                degs = graph.out_degrees().to(feat_src).clamp(min=1)
                norm = torch.pow(degs, -0.5)
                feat_src = feat_src * norm.view((-1,) + (1,) * (feat_src.dim() - 1))
            if weight is not None and self.weight is not None:
                raise DGLError("External weight is provided while at the same time the module has defined its own "
                               "weight parameter. Please create the module with flag weight=False.")
            weight = self.weight if weight is None else weight
            if self._in_feats > self._out_feats:
                if weight is not None:
                    feat_src = torch.matmul(feat_src, weight)
                graph.srcdata["h"] = feat_src
                graph.update_all(fn.copy_src(src="h", out="m"), fn.sum(msg="m", out="h"))
                rst = graph.dstdata["h"]
            else:
                graph.srcdata["h"] = feat_src
                graph.update_all(fn.copy_src(src="h", out="m"), fn.sum(msg="m", out="h"))
                rst = graph.dstdata["h"]
                if weight is not None:
                    rst = torch.matmul(rst, weight)
            if self._norm != "none":
                degs = graph.in_degrees().to(feat_dst).clamp(min=1)
                norm = torch.pow(degs, -0.5) if self._norm == "both" else 1.0 / degs
                rst = rst * norm.view((-1,) + (1,) * (feat_dst.dim() - 1))
            if self.bias is not None:
                rst = ops.bias_add(rst, self.bias)
            if self._activation is not None:
                rst = self._activation(rst)
            return rst


class GINConv(nn.Module):
    """dgl.nn.pytorch.GINConv (UPSTREAM): h_v = f((1 + eps) h_v + AGG_{u->v} h_u), AGG = sum | mean | max -- a builtin
    copy_u aggregation (one g-SpMM) followed by `apply_func`.  BASELINE.json names "5-layer GIN on ogbg-molhiv" for the
    batched many-small-graphs path; the reference's own molhiv script is the GCN of graph_classification.py."""

    def __init__(self, apply_func=None, aggregator_type="sum", init_eps=0, learn_eps=False):
        super(GINConv, self).__init__()
        if aggregator_type not in ("sum", "max", "mean"):
            raise KeyError("Aggregator type {} not recognized.".format(aggregator_type))
        self.apply_func = apply_func
        self._reducer = getattr(fn, aggregator_type)
        if learn_eps:
            self.eps = nn.Parameter(torch.FloatTensor([init_eps]))
        else:
            self.register_buffer("eps", torch.FloatTensor([init_eps]))

    def forward(self, graph, feat, edge_weight=None):
        with graph.local_scope():
            feat_src, feat_dst = expand_as_pair(feat, graph)
            graph.srcdata["h"] = feat_src
            if edge_weight is not None:
                graph.edata["_edge_weight"] = edge_weight
                graph.update_all(fn.u_mul_e("h", "_edge_weight", "m"), self._reducer("m", "neigh"))
            else:
                graph.update_all(fn.copy_u("h", "m"), self._reducer("m", "neigh"))
            rst = (1 + self.eps) * feat_dst + graph.dstdata["neigh"]
            if self.apply_func is not None:
                rst = self.apply_func(rst)
            return rst


class GINEConv(nn.Module):
    """dgl.nn.pytorch.GINEConv (UPSTREAM): h_v = f((1 + eps) h_v + sum_{u->v} relu(h_u + e_uv)) -- GIN with edge features of the node
    width.  The aggregation is ops.gine_sum (csrc/gine.hip when it takes the shape: no [E, D] message tensor), then `apply_func`."""

    def __init__(self, apply_func=None, init_eps=0, learn_eps=False):
        super(GINEConv, self).__init__()
        self.apply_func = apply_func
        if learn_eps:
            self.eps = nn.Parameter(torch.FloatTensor([init_eps]))
        else:
            self.register_buffer("eps", torch.FloatTensor([init_eps]))

    def forward(self, graph, node_feat, edge_feat):
        feat_src, feat_dst = expand_as_pair(node_feat, graph)
        rst = (1 + self.eps) * feat_dst + ops.gine_sum(graph, feat_src, edge_feat)
        if self.apply_func is not None:
            rst = self.apply_func(rst)
        return rst


class PNAConvTower(nn.Module):
    """The parameters of one tower of PNAConv (UPSTREAM dgl.nn.pytorch.conv.pnaconv.PNAConvTower: M, U, batchnorm, dropout).  The
    arithmetic is PNAConv.forward's: all towers share one aggregation call."""

    def __init__(self, in_size, out_size, n_agg, n_scalers, dropout=0., edge_feat_size=0):
        super(PNAConvTower, self).__init__()
        self.M = nn.Linear(2 * in_size + edge_feat_size, in_size)
        self.U = nn.Linear((n_agg * n_scalers + 1) * in_size, out_size)
        self.dropout = nn.Dropout(dropout)
        self.batchnorm = BatchNorm1d(out_size)


class PNAConv(nn.Module):
    """dgl.nn.pytorch.PNAConv (UPSTREAM): Principal Neighbourhood Aggregation.  Per tower t (a column block of the features)

        msg_e = M_t [h_u ; h_v ; a_e],   agg = [AGG(msg) for AGG in aggregators],   h_neigh = [scaler(agg, d) for scaler in scalers]
        h_t   = dropout(batchnorm(U_t [h_v ; h_neigh] / sqrt(nodes in v's graph)))

    then mixing_layer = Linear + LeakyReLU over the towers' concatenation and the residual when in_size == out_size.
    aggregators out of sum, mean, max, min, var, std (std = sqrt(var + 1e-30), var = relu(E[m^2] - E[m]^2) as upstream);
    scalers out of identity, amplification (* log(d + 1) / delta), attenuation (* delta / log(d + 1), 0 where d == 0).
    A node without in-edges has h_neigh = 0, as the mailbox UDF leaves it.

    M is never applied per edge: with M.weight = [W_src | W_dst | W_e] by columns, a = h W_src^T and b = h W_dst^T + bias per NODE
    and c = a_e W_e^T per edge give msg_e = a_u + b_v + c_e; all towers are column blocks of one matrix, so ONE
    ops.multi_aggregate(g, a, aggregators, w=c) serves the layer (csrc/multiagg.hip: one walk forward, one backward), and b_v is
    added afterwards: to mean / max / min as it is, d times to sum, not at all to var / std.  Without edge features no tensor of E rows
    exists.

    Knowingly different from upstream: moment3 / moment4 / moment5 are not offered; `delta` must be positive; on a block (or a pair of
    inputs) the destination rows are used for h_v and the graph-size normalisation counts destination nodes (upstream takes
    homogeneous graphs only); ties of max / min route their gradient to the first edge in storage order, where the mailbox's
    torch.max picks an index of its own."""

    AGGREGATORS = ("sum", "mean", "max", "min", "var", "std")
    SCALERS = ("identity", "amplification", "attenuation")

    def __init__(self, in_size, out_size, aggregators, scalers, delta, dropout=0., num_towers=1, edge_feat_size=0, residual=True):
        super(PNAConv, self).__init__()
        aggregators, scalers = tuple(aggregators), tuple(scalers)
        if not aggregators or any(a not in self.AGGREGATORS for a in aggregators) or len(set(aggregators)) != len(aggregators):
            raise DGLError("PNAConv: aggregators must be distinct names out of %s, got %r" % (", ".join(self.AGGREGATORS), aggregators))
        if not scalers or any(s not in self.SCALERS for s in scalers):
            raise DGLError("PNAConv: scalers must be names out of %s, got %r" % (", ".join(self.SCALERS), scalers))
        if in_size % num_towers or out_size % num_towers:
            raise DGLError("PNAConv: in_size %d and out_size %d must be divisible by num_towers %d" % (in_size, out_size, num_towers))
        if not float(delta) > 0:
            raise DGLError("PNAConv: delta must be positive, got %r" % (delta,))
        self.in_size, self.out_size, self.num_towers = in_size, out_size, num_towers
        self.tower_in_size, self.tower_out_size = in_size // num_towers, out_size // num_towers
        self.aggregators, self.scalers, self.delta = aggregators, scalers, float(delta)
        self.edge_feat_size = edge_feat_size
        self.residual = residual and in_size == out_size
        self.towers = nn.ModuleList([PNAConvTower(self.tower_in_size, self.tower_out_size, len(aggregators), len(scalers), dropout,
                                                  edge_feat_size) for _ in range(num_towers)])
        self.mixing_layer = nn.Sequential(nn.Linear(out_size, out_size), nn.LeakyReLU())

    def _graph_size_norm(self, graph, n_dst, like):
        counts = graph.batch_num_nodes() if not getattr(graph, "is_block", False) else None
        if counts is None or int(counts.shape[0]) == 1:
            return like.new_full((1, 1), 1.0 / math.sqrt(max(n_dst, 1)))
        counts = counts.to(like.device)
        return torch.repeat_interleave(counts.to(like.dtype).rsqrt(), counts, output_size=n_dst).unsqueeze(-1)

    def forward(self, graph, node_feat, edge_feat=None):
        feat_src, feat_dst = expand_as_pair(node_feat, graph)
        T, tin = self.num_towers, self.tower_in_size
        if (edge_feat is not None) != (self.edge_feat_size > 0):
            raise DGLError("PNAConv: edge_feat is %s but edge_feat_size is %d" % ("given" if edge_feat is not None else "missing", self.edge_feat_size))
        n_dst = feat_dst.shape[0]
        a, b = [], []
        for t, tower in enumerate(self.towers):  # per NODE: the source and destination parts of M
            Wm = tower.M.weight
            a.append(F.linear(feat_src[:, t * tin:(t + 1) * tin], Wm[:, :tin]))
            b.append(F.linear(feat_dst[:, t * tin:(t + 1) * tin], Wm[:, tin:2 * tin], tower.M.bias))
        a, b = (torch.cat(p, dim=1) if T > 1 else p[0] for p in (a, b))
        c = None
        if edge_feat is not None:                # per edge: one [E, in_size] product for all towers
            c = F.linear(edge_feat, torch.cat([tower.M.weight[:, 2 * tin:] for tower in self.towers], dim=0))
        agg = ops.multi_aggregate(graph, a, self.aggregators, w=c)   # [n_dst, A, in_size]
        deg = graph.in_degrees().to(agg.dtype).view(-1, 1)
        some = (deg > 0).to(agg.dtype)
        shift = {"mean": some, "max": some, "min": some, "sum": deg}  # what b_v adds: nothing to var / std, nothing without in-edges
        agg = agg + torch.stack([b * shift[n] if n in shift else torch.zeros_like(b) for n in self.aggregators], dim=1)
        logd = torch.log(deg + 1)
        scale = {"identity": None, "amplification": logd / self.delta,
                 "attenuation": torch.where(deg > 0, self.delta / logd.clamp(min=1e-30), torch.zeros_like(logd))}
        snorm = self._graph_size_norm(graph, n_dst, agg)
        outs = []
        for t, tower in enumerate(self.towers):
            h = agg[:, :, t * tin:(t + 1) * tin].reshape(n_dst, -1)
            h = torch.cat([h if scale[s] is None else h * scale[s] for s in self.scalers], dim=1)
            h = tower.U(torch.cat([feat_dst[:, t * tin:(t + 1) * tin], h], dim=1)) * snorm
            outs.append(tower.dropout(tower.batchnorm(h)))
        h_out = self.mixing_layer(torch.cat(outs, dim=1) if T > 1 else outs[0])
        if self.residual:
            h_out = h_out + feat_dst
        return h_out


def _hetero_aggregate(name):
    if callable(name):
        return name
    if name == "stack":
        return lambda xs, dsttype: torch.stack(xs, dim=1) if xs else None
    fns = {"sum": lambda t: t.sum(0), "mean": lambda t: t.mean(0), "max": lambda t: t.max(0)[0], "min": lambda t: t.min(0)[0]}
    if name not in fns:
        raise DGLError('Invalid cross type aggregator. Must be one of "sum", "max", "min", "mean" or "stack". But got "%s"' % name)
    return lambda xs, dsttype: fns[name](torch.stack(xs, dim=0)) if xs else None


class HeteroGraphConv(nn.Module):
    """dglnn.HeteroGraphConv (gcmc_dgl/model.py:205): one sub-module per relation, each run on the relation's own
    graph view (its own in-CSR and execution plan), results combined per destination type by `aggregate`."""

    def __init__(self, mods, aggregate="sum"):
        super(HeteroGraphConv, self).__init__()
        self.mods = nn.ModuleDict(mods)
        for _, v in self.mods.items():  # isolated destinations are expected inside a single relation
            set_allow = getattr(v, "set_allow_zero_in_degree", None)
            if callable(set_allow):
                set_allow(True)
        self.agg_fn = _hetero_aggregate(aggregate)

    def forward(self, g, inputs, mod_args=None, mod_kwargs=None):
        mod_args = mod_args or {}
        mod_kwargs = mod_kwargs or {}
        outputs = {nty: [] for nty in g.dsttypes}
        if isinstance(inputs, tuple):
            src_inputs, dst_inputs = inputs
        elif g.is_block:
            src_inputs = inputs
            dst_inputs = {k: v[:g.number_of_dst_nodes(k)] for k, v in inputs.items()}
        else:
            src_inputs = dst_inputs = inputs
        for stype, etype, dtype in g.canonical_etypes:
            rel_graph = g[stype, etype, dtype]
            if rel_graph.number_of_edges() == 0:
                continue
            if stype not in src_inputs or dtype not in dst_inputs:
                continue
            dstdata = self.mods[etype](rel_graph, (src_inputs[stype], dst_inputs[dtype]), *mod_args.get(etype, ()),
                                       **mod_kwargs.get(etype, {}))
            outputs[dtype].append(dstdata)
        rsts = {}
        for nty, alist in outputs.items():
            if len(alist) != 0:
                rsts[nty] = self.agg_fn(alist, nty)
        return rsts


class _Pooling(nn.Module):
    _op = "sum"

    def forward(self, graph, feat):
        return ops.segment_reduce(graph.batch_num_nodes(), feat, self._op, total=graph.number_of_nodes())


class SumPooling(_Pooling):
    _op = "sum"


class AvgPooling(_Pooling):
    """Per-graph mean of node features (main_dgl_molhiv_gcn.py:75,93)."""
    _op = "mean"


class MaxPooling(_Pooling):
    _op = "max"


class GlobalAttentionPooling(nn.Module):
    """dgl.nn.GlobalAttentionPooling: r_g = sum_{i in g} softmax_g(gate_nn(x))_i * feat_nn(x_i) -> [B, D].  The softmax over the graph's
    nodes and the weighted sum are ONE ops.segment_attention call in gate mode (csrc/segattn.hip; H = 1)."""

    def __init__(self, gate_nn, feat_nn=None):
        super(GlobalAttentionPooling, self).__init__()
        self.gate_nn = gate_nn
        self.feat_nn = feat_nn

    def forward(self, graph, feat):
        gate = self.gate_nn(feat)
        if gate.shape[-1] != 1:
            raise DGLError("The output of gate_nn should have size 1 at the last axis.")
        feat = self.feat_nn(feat) if self.feat_nn is not None else feat
        n = graph.number_of_nodes()
        out = ops.segment_attention(graph.batch_num_nodes(), feat.reshape(n, 1, -1), logits=gate.reshape(n, 1), total=n)
        return out.view(out.shape[0], -1)


class Set2Set(nn.Module):
    """dgl.nn.Set2Set (Vinyals et al., Order Matters): n_iters rounds of  q_t = LSTM(q*_{t-1});  a = softmax_g(<x_i, q_t>);
    r_t = sum_i a_i x_i;  q*_t = [q_t, r_t]  ->  [B, 2 * input_dim].  Parameters are DGL's: an nn.LSTM(2 * input_dim, input_dim, n_layers)
    named `lstm`.  Every round's softmax-weighted sum is ONE ops.segment_attention call in query mode (csrc/segattn.hip).  The LSTM sees a
    sequence of length one per round, so its step is written out over the nn.LSTM parameters (two GEMMs and the gate arithmetic per
    layer -- nn.LSTM's own formulas): plain tensor operators, which a HIP-graph capture of the training step records like any others."""

    def __init__(self, input_dim, n_iters, n_layers):
        super(Set2Set, self).__init__()
        self.input_dim = input_dim
        self.output_dim = 2 * input_dim
        self.n_iters = n_iters
        self.n_layers = n_layers
        self.lstm = nn.LSTM(self.output_dim, self.input_dim, n_layers)
        # _lstm_step writes the step out over this module's parameters and holds only for the options used here (DGL's): biases, no
        # projection, one direction, no dropout between layers -- building self.lstm otherwise means changing _lstm_step with it
        assert self.lstm.bias and self.lstm.proj_size == 0 and not self.lstm.bidirectional and self.lstm.dropout == 0
        self.reset_parameters()

    def reset_parameters(self):
        self.lstm.reset_parameters()

    def _lstm_step(self, x, h, c):
        """One time step of self.lstm: x [B, in], h / c lists of [B, input_dim] per layer -> (top layer's h, new h, new c)."""
        hs, cs = [], []
        for k in range(self.n_layers):
            gates = (F.linear(x, getattr(self.lstm, "weight_ih_l%d" % k), getattr(self.lstm, "bias_ih_l%d" % k))
                     + F.linear(h[k], getattr(self.lstm, "weight_hh_l%d" % k), getattr(self.lstm, "bias_hh_l%d" % k)))
            i, f, g, o = gates.chunk(4, dim=1)
            ck = torch.sigmoid(f) * c[k] + torch.sigmoid(i) * torch.tanh(g)
            x = torch.sigmoid(o) * torch.tanh(ck)
            hs.append(x)
            cs.append(ck)
        return x, hs, cs

    def forward(self, graph, feat):
        B, n = graph.batch_size, graph.number_of_nodes()
        seglen = graph.batch_num_nodes()
        feat3 = feat.reshape(n, 1, self.input_dim)
        h = [feat.new_zeros((B, self.input_dim)) for _ in range(self.n_layers)]
        c = [feat.new_zeros((B, self.input_dim)) for _ in range(self.n_layers)]
        q_star = feat.new_zeros((B, self.output_dim))
        for _ in range(self.n_iters):
            q, h, c = self._lstm_step(q_star, h, c)
            readout = ops.segment_attention(seglen, feat3, query=q.view(B, 1, self.input_dim), scale=1.0, total=n)
            q_star = torch.cat([q, readout.view(B, self.input_dim)], dim=-1)
        return q_star

    def extra_repr(self):
        return "n_iters={n_iters}".format(**self.__dict__)


class SortPooling(nn.Module):
    """dgl.nn.SortPooling (Zhang et al., An End-to-End Deep Learning Architecture for Graph Classification): every node's features sorted
    ascending, the k nodes of every graph with the largest last feature in descending order, flattened -> [B, k * D]; graphs with fewer
    than k nodes are padded with zeros.  The selection is ONE ops.segment_topk call (csrc/segtopk.hip, sortby = -1); the per-node
    feature sort stays a torch operator (feat.sort(dim=-1))."""

    def __init__(self, k):
        super(SortPooling, self).__init__()
        self.k = k

    def forward(self, graph, feat):
        feat, _ = feat.sort(dim=-1)
        values, _ = ops.segment_topk(graph.batch_num_nodes(), feat, self.k, sortby=-1, descending=True, total=graph.number_of_nodes())
        return values.view(values.shape[0], -1)

    def extra_repr(self):
        return "k={k}".format(**self.__dict__)


class KNNGraph(nn.Module):
    """dgl.nn.KNNGraph: points [N, D] (one set) or [B, n, D] (B sets, node b * n + i) -> the graph in which every node's predecessors
    are its k nearest points (transform.knn_graph: ops.segment_knn, whose index is the in-CSR).  No parameters."""

    def __init__(self, k):
        super(KNNGraph, self).__init__()
        self.k = k

    def forward(self, x):
        from .transform import knn_graph
        return knn_graph(x, self.k)

    def extra_repr(self):
        return "k={k}".format(**self.__dict__)


class SegmentedKNNGraph(nn.Module):
    """dgl.nn.SegmentedKNNGraph: points [N, D] in consecutive sets of segs[0], segs[1], ... points (transform.segmented_knn_graph)."""

    def __init__(self, k):
        super(SegmentedKNNGraph, self).__init__()
        self.k = k

    def forward(self, x, segs):
        from .transform import segmented_knn_graph
        return segmented_knn_graph(x, self.k, segs)

    def extra_repr(self):
        return "k={k}".format(**self.__dict__)


class FarthestPointSampler(nn.Module):
    """dgl.geometry.FarthestPointSampler (dgl.geometry.pytorch in DGL 0.5): pos [B, n, C] -> int64 [B, npoints], the sampled points'
    numbers inside each cloud, the start of every cloud drawn at random (transform.farthest_point_sampler: ops.segment_fps).  No
    parameters."""

    def __init__(self, npoints):
        super(FarthestPointSampler, self).__init__()
        self.npoints = npoints

    def forward(self, pos):
        from .transform import farthest_point_sampler
        return farthest_point_sampler(pos, self.npoints)

    def extra_repr(self):
        return "npoints={npoints}".format(**self.__dict__)


class FixedRadiusNNGraph(nn.Module):
    """The PointNet++ grouping: points [N, D] in consecutive sets of segs[0], segs[1], ... points and centres int64 [M] (rows of the
    points) -> the block whose destination i is centre i and whose predecessors are the first max_neighbors points within radius of
    it (transform.fixed_radius_block: ops.segment_ball_query, whose padded index is the in-CSR).  No parameters."""

    def __init__(self, radius, max_neighbors):
        super(FixedRadiusNNGraph, self).__init__()
        self.radius, self.max_neighbors = radius, max_neighbors

    def forward(self, pos, centers, segs):
        from .transform import fixed_radius_block
        return fixed_radius_block(pos, centers, self.radius, self.max_neighbors, segs)

    def extra_repr(self):
        return "radius={radius}, max_neighbors={max_neighbors}".format(**self.__dict__)


class EdgeConv(nn.Module):
    """dgl.nn.EdgeConv (Wang et al., Dynamic Graph CNN for Learning on Point Clouds), by upstream's documented formula:
        out_i = max_{j -> i} [ theta(x_j - x_i) + phi(x_i) ]     per column; 0 for a node without in-edges
    with theta, phi = Linear(in_feat, out_feat).  Without batch norm (config.EDGECONV_FUSED) the bracket is
    x_j Theta^T + [x_i (Phi - Theta)^T + b_theta + b_phi], whose second part does not depend on j: a GEMM over the NODES, the
    copy_u / max g-SpMM (gradient through its arg) and a second node GEMM -- no tensor of E rows exists in either direction.  With
    batch_norm=True, or with the switch off, the literal composition: u_sub_v g-SDDMM, the two Linears, BatchNorm1d over the edges,
    copy_e / max."""

    def __init__(self, in_feat, out_feat, batch_norm=False, allow_zero_in_degree=False):
        super(EdgeConv, self).__init__()
        self.batch_norm = batch_norm
        self._allow_zero_in_degree = allow_zero_in_degree
        self.theta = Linear(in_feat, out_feat)
        self.phi = Linear(in_feat, out_feat)
        if batch_norm:
            self.bn = BatchNorm1d(out_feat)

    def set_allow_zero_in_degree(self, set_value):
        self._allow_zero_in_degree = set_value

    def forward(self, g, feat):
        with g.local_scope():
            zero_deg = _has_zero_in_degree(g)
            if zero_deg and not self._allow_zero_in_degree:
                raise DGLError("There are 0-in-degree nodes in the graph, output for those nodes will be invalid. "
                               "Adding self-loop on the input graph by calling `g = dgl.add_self_loop(g)` will "
                               "resolve the issue. Setting ``allow_zero_in_degree`` to be `True` when constructing "
                               "this module will suppress the check and let the code run.")
            h_src, h_dst = expand_as_pair(feat, g)
            if not self.batch_norm and config.EDGECONV_FUSED:
                g.srcdata["y"] = F.linear(h_src, self.theta.weight)
                g.update_all(fn.copy_u("y", "m"), fn.max("m", "m"))
                rst = g.dstdata["m"] + ops.linear(h_dst, self.phi.weight - self.theta.weight, self.theta.bias + self.phi.bias)
            else:
                g.srcdata["x"], g.dstdata["x"] = h_src, h_dst
                g.apply_edges(fn.u_sub_v("x", "x", "theta"))
                g.edata["theta"] = self.theta(g.edata["theta"])
                g.dstdata["phi"] = self.phi(h_dst)
                g.apply_edges(fn.e_add_v("theta", "phi", "e"))
                e = g.edata["e"]
                g.edata["e"] = self.bn(e) if self.batch_norm else e
                g.update_all(fn.copy_e("e", "m"), fn.max("m", "x"))
                rst = g.dstdata["x"]
            if zero_deg:
                has = (g.in_degrees() > 0).view((-1,) + (1,) * (rst.dim() - 1))
                rst = torch.where(has, rst, rst.new_zeros(()))
            return rst


class PointNetConv(nn.Module):
    """The PointNet++ set-abstraction message (Qi et al., PointNet++: Deep Hierarchical Feature Learning on Point Sets in a Metric Space)
    over a block such as transform.fixed_radius_block builds:
        out_i = max_{j -> i} MLP([h_j | pos_j - pos_i])     per column; 0 for a node without in-edges
    with MLP = Linear(in_feats + pos_dim, sizes[0]) -> ReLU -> Linear(sizes[0], sizes[1]) -> ReLU ... (a ReLU after every layer, a
    BatchNorm1d over the edges before it with batch_norm=True).  in_feats = 0: positions only (the first level).  Positions come from
    srcdata["pos"] / dstdata["pos"] of the block unless given.
    The first Linear is pulled to the nodes as EdgeConv's is: W [h_j | pos_j - pos_i] + b = (W_h h_j + W_p pos_j) - (W_p pos_i - b).
    With one layer and no batch norm (config.POINTNETCONV_FUSED) the ReLU commutes with the max, so the layer is a GEMM over the N
    points, the copy_u / max g-SpMM (gradient through its arg) and M-row arithmetic: no tensor of E rows exists in either direction.
    With more layers or batch norm: the u_sub_v g-SDDMM of the two node projections, the remaining Linears over the edges, copy_e / max.
    The repeated first point of a padded ball changes nothing under the max."""

    def __init__(self, in_feats, sizes, batch_norm=False, pos_dim=3, allow_zero_in_degree=False):
        super(PointNetConv, self).__init__()
        sizes = [int(v) for v in sizes]
        if in_feats < 0 or pos_dim < 1 or not sizes or min(sizes) < 1:
            raise DGLError("PointNetConv: needs in_feats >= 0, pos_dim >= 1 and at least one layer size >= 1, got %r, %r, %r" % (in_feats, pos_dim, sizes))
        self.in_feats, self.pos_dim, self.sizes, self.batch_norm = in_feats, pos_dim, sizes, batch_norm
        self._allow_zero_in_degree = allow_zero_in_degree
        self.layers = nn.ModuleList([Linear(a, b) for a, b in zip([in_feats + pos_dim] + sizes[:-1], sizes)])
        if batch_norm:
            self.bns = nn.ModuleList([BatchNorm1d(b) for b in sizes])

    def set_allow_zero_in_degree(self, set_value):
        self._allow_zero_in_degree = set_value

    def forward(self, g, feat=None, pos=None):
        with g.local_scope():
            zero_deg = _has_zero_in_degree(g)
            if zero_deg and not self._allow_zero_in_degree:
                raise DGLError("There are 0-in-degree nodes in the graph, output for those nodes will be invalid. "
                               "Setting ``allow_zero_in_degree`` to be `True` when constructing this module will suppress the check "
                               "and let the code run.")
            pos_src, pos_dst = (g.srcdata["pos"], g.dstdata["pos"]) if pos is None else expand_as_pair(pos, g)
            if (feat is None) != (self.in_feats == 0):
                raise DGLError("PointNetConv: in_feats = %d %s source features" % (self.in_feats, "needs" if feat is None else "takes no"))
            if pos_src.shape[1] != self.pos_dim or (feat is not None and feat.shape[1] != self.in_feats):
                raise DGLError("PointNetConv: expected positions [*, %d] and features [*, %d]" % (self.pos_dim, self.in_feats))
            first = self.layers[0]
            w_pos = first.weight[:, self.in_feats:]
            u = F.linear(pos_src if feat is None else torch.cat([feat, pos_src], 1), first.weight)   # W_h h_j + W_p pos_j: over the N points
            v = F.linear(pos_dst, w_pos) - first.bias                                               # W_p pos_i - b: over the M centres
            if len(self.layers) == 1 and not self.batch_norm and config.POINTNETCONV_FUSED:
                g.srcdata["u"] = u
                g.update_all(fn.copy_u("u", "m"), fn.max("m", "m"))
                rst = F.relu(g.dstdata["m"] - v)
            else:
                g.srcdata["u"], g.dstdata["v"] = u, v
                g.apply_edges(fn.u_sub_v("u", "v", "e"))
                e = g.edata["e"]
                for i, layer in enumerate(self.layers):
                    if i:
                        e = layer(e)
                    e = F.relu(self.bns[i](e) if self.batch_norm else e)
                g.edata["e"] = e
                g.update_all(fn.copy_e("e", "m"), fn.max("m", "m"))
                rst = g.dstdata["m"]
            if zero_deg:
                has = (g.in_degrees() > 0).view((-1,) + (1,) * (rst.dim() - 1))
                rst = torch.where(has, rst, rst.new_zeros(()))
            return rst


class FeaturePropagation(nn.Module):
    """The PointNet++ feature-propagation level (PointNet2FP of DGL's example; PyG's knn_interpolate + MLP): the features of a coarse
    level are carried up to the M points of a finer one,
        h_q = sum_r w[q, r] feat[index[q, r]]     over the k nearest coarse points of q's own cloud, w the normalised 1 / (d^2 + eps)
    (transform.knn_interpolate: ops.segment_knn_query, whose index is the in-CSR, and the u_mul_e / sum g-SpMM), concatenated with the
    finer level's own `skip` features when skip_feats > 0, then Linear -> (BatchNorm1d) -> ReLU per entry of `sizes` over the M
    points.  The gradient reaches feat, skip and the parameters; the interpolation weights are constants."""

    def __init__(self, in_feats, skip_feats, sizes, batch_norm=False, k=3):
        super(FeaturePropagation, self).__init__()
        sizes = [int(v) for v in sizes]
        if in_feats < 1 or skip_feats < 0 or not sizes or min(sizes) < 1 or isinstance(k, bool) or not isinstance(k, int) or k < 1:
            raise DGLError("FeaturePropagation: needs in_feats >= 1, skip_feats >= 0, at least one layer size >= 1 and an integer k >= 1, "
                           "got %r, %r, %r, %r" % (in_feats, skip_feats, sizes, k))
        self.in_feats, self.skip_feats, self.sizes, self.batch_norm, self.k = in_feats, skip_feats, sizes, batch_norm, k
        self.layers = nn.ModuleList([Linear(a, b) for a, b in zip([in_feats + skip_feats] + sizes[:-1], sizes)])
        if batch_norm:
            self.bns = nn.ModuleList([BatchNorm1d(b) for b in sizes])

    def forward(self, feat, pos_src, pos_dst, segs_src, segs_dst, skip=None):
        """feat [N, in_feats] on the coarse points pos_src [N, D]; pos_dst [M, D] the finer points, skip [M, skip_feats] their own
        features; segs_src / segs_dst the clouds' lengths in either level (Python lists) -> [M, sizes[-1]]"""
        from .transform import knn_interpolate
        if (skip is None) != (self.skip_feats == 0):
            raise DGLError("FeaturePropagation: skip_feats = %d %s skip features" % (self.skip_feats, "needs" if skip is None else "takes no"))
        if feat.dim() != 2 or feat.shape[1] != self.in_feats or (skip is not None and (skip.dim() != 2 or skip.shape[1] != self.skip_feats
                                                                                       or skip.shape[0] != pos_dst.shape[0])):
            raise DGLError("FeaturePropagation: expected features [*, %d] and skip features [%d, %d]"
                           % (self.in_feats, pos_dst.shape[0], self.skip_feats))
        h = knn_interpolate(feat, pos_src, pos_dst, segs_src, segs_dst, self.k)
        if skip is not None:
            h = torch.cat([h, skip], 1)
        for i, layer in enumerate(self.layers):
            h = layer(h)
            h = F.relu(self.bns[i](h) if self.batch_norm else h)
        return h

    def extra_repr(self):
        return "in_feats={in_feats}, skip_feats={skip_feats}, sizes={sizes}, k={k}".format(**self.__dict__)


class WeightAndSum(nn.Module):
    """dgl.nn.WeightAndSum: per-node weights sigmoid(Linear(in_feats, 1)) (named `atom_weighting`), then the weighted sum_nodes."""

    def __init__(self, in_feats):
        super(WeightAndSum, self).__init__()
        self.in_feats = in_feats
        self.atom_weighting = nn.Sequential(nn.Linear(in_feats, 1), nn.Sigmoid())

    def forward(self, g, feats):
        return ops.segment_reduce(g.batch_num_nodes(), feats * self.atom_weighting(feats), "sum", total=g.number_of_nodes())
