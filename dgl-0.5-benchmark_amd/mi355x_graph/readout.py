"""Graph-level readout functions of DGL 0.5 (python/dgl/readout.py) over a batched graph: readout / sum / mean / max / softmax /
broadcast for nodes and for edges.  A graph of the batch is a contiguous slice of rows (batch_num_nodes() / batch_num_edges()), so every
function is one segment operator of ops.py: segment_reduce (csrc/segment.hip), segment_softmax (csrc/segattn.hip) or a row gather.  An
unbatched graph is one segment.  The layers built on them are in nn.py (GlobalAttentionPooling, Set2Set, WeightAndSum); the fused
attention readout those layers use is ops.segment_attention.  topk_nodes / topk_edges select rows: ops.segment_topk (csrc/segtopk.hip),
which nn.SortPooling is built on."""
from ._lib import DGLError
from . import ops

__all__ = ["readout_nodes", "sum_nodes", "mean_nodes", "max_nodes", "softmax_nodes", "broadcast_nodes", "topk_nodes",
           "readout_edges", "sum_edges", "mean_edges", "max_edges", "softmax_edges", "broadcast_edges", "topk_edges"]

_READOUT_OPS = ("sum", "mean", "max", "min")


def _rows(graph, kind, type_):
    """(segment lengths, frame, row count) of the nodes or the edges of `graph`."""
    if kind == "nodes":
        return graph.batch_num_nodes(type_), graph.ndata, graph.number_of_nodes()
    return graph.batch_num_edges(type_), graph.edata, graph.number_of_edges()


def _readout(graph, kind, feat, weight, op, type_):
    if op not in _READOUT_OPS:
        raise DGLError("Unsupported readout op %r: expected one of %s" % (op, ", ".join(_READOUT_OPS)))
    seglen, frame, total = _rows(graph, kind, type_)
    x = frame[feat]
    if weight is not None:
        x = x * frame[weight]
    return ops.segment_reduce(seglen, x, op, total=total)


def _softmax(graph, kind, feat, type_):
    seglen, frame, total = _rows(graph, kind, type_)
    return ops.segment_softmax(seglen, frame[feat], total=total)


def _broadcast(graph, kind, graph_feat, type_):
    seglen, _, total = _rows(graph, kind, type_)
    if graph_feat.shape[0] != seglen.shape[0]:
        if seglen.shape[0] == 1 and graph_feat.dim() >= 1:  # DGL: a feature without the batch dimension on an unbatched graph
            graph_feat = graph_feat.unsqueeze(0)
        else:
            raise DGLError("broadcast_%s: the graph feature has %d rows, the batch has %d graphs"
                           % (kind, graph_feat.shape[0], seglen.shape[0]))
    return ops.segment_broadcast(seglen, graph_feat, total)


def _topk(graph, kind, feat, k, descending, sortby, type_):
    seglen, frame, total = _rows(graph, kind, type_)
    return ops.segment_topk(seglen, frame[feat], k, sortby=sortby, descending=descending, total=total)


# ---- nodes
def readout_nodes(graph, feat, weight=None, *, op="sum", ntype=None):
    """Per-graph `op` (sum, mean, max, min) of the node feature `feat`, multiplied by the node feature `weight` first: [B, ...]."""
    return _readout(graph, "nodes", feat, weight, op, ntype)


def sum_nodes(graph, feat, weight=None, *, ntype=None):
    return _readout(graph, "nodes", feat, weight, "sum", ntype)


def mean_nodes(graph, feat, weight=None, *, ntype=None):
    return _readout(graph, "nodes", feat, weight, "mean", ntype)


def max_nodes(graph, feat, weight=None, *, ntype=None):
    return _readout(graph, "nodes", feat, weight, "max", ntype)


def softmax_nodes(graph, feat, *, ntype=None):
    """Softmax of the node feature `feat` over the nodes of every graph, per column: [N, ...]."""
    return _softmax(graph, "nodes", feat, ntype)


def broadcast_nodes(graph, graph_feat, *, ntype=None):
    """Row g of `graph_feat` [B, ...] repeated for every node of graph g: [N, ...]."""
    return _broadcast(graph, "nodes", graph_feat, ntype)


def topk_nodes(graph, feat, k, *, descending=True, sortby=None, ntype=None):
    """The k first nodes of every graph by the node feature `feat` [N, D] (dgl.topk_nodes): (values [B, k, D], index).  With `sortby` (a
    column; negative counts from the last) whole rows are ordered by that column and index is [B, k]; without, every column is ordered on
    its own and index is [B, k, D].  The order is a stable sort's (ties keep the lower node first, NaN is the greatest value); a graph
    with fewer than k nodes is padded with zero rows, whose index is -1 (DGL leaves it unspecified)."""
    return _topk(graph, "nodes", feat, k, descending, sortby, ntype)


# ---- edges
def readout_edges(graph, feat, weight=None, *, op="sum", etype=None):
    """Per-graph `op` (sum, mean, max, min) of the edge feature `feat`, multiplied by the edge feature `weight` first: [B, ...]."""
    return _readout(graph, "edges", feat, weight, op, etype)


def sum_edges(graph, feat, weight=None, *, etype=None):
    return _readout(graph, "edges", feat, weight, "sum", etype)


def mean_edges(graph, feat, weight=None, *, etype=None):
    return _readout(graph, "edges", feat, weight, "mean", etype)


def max_edges(graph, feat, weight=None, *, etype=None):
    return _readout(graph, "edges", feat, weight, "max", etype)


def softmax_edges(graph, feat, *, etype=None):
    """Softmax of the edge feature `feat` over the edges of every graph, per column: [E, ...]."""
    return _softmax(graph, "edges", feat, etype)


def broadcast_edges(graph, graph_feat, *, etype=None):
    """Row g of `graph_feat` [B, ...] repeated for every edge of graph g: [E, ...]."""
    return _broadcast(graph, "edges", graph_feat, etype)


def topk_edges(graph, feat, k, *, descending=True, sortby=None, etype=None):
    """topk_nodes over the edges of every graph by the edge feature `feat` (dgl.topk_edges)."""
    return _topk(graph, "edges", feat, k, descending, sortby, etype)
