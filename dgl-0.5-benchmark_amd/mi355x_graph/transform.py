"""Integer graph transforms used by the benchmark scripts (bit-exact index work, torch integer ops):
  dgl.to_bidirected   main_dgl_arxiv_sage.py:162      dgl.add_self_loop  main_dgl_reddit_gat.py:136
  dgl.from_networkx   main_dgl_citation_sage.py:190   dgl.batch          GraphDataLoader, main_dgl_molhiv_gcn.py:163
They run on whatever device holds the index tensors (the scripts call them on the CPU before .to()).
"""
import torch

from ._lib import DGLError
from .graph import DGLGraph, GraphIndex, graph


def to_bidirected(g, copy_ndata=False, readonly=None):
    """Union of the edges and their reverses with duplicates removed; result edges sorted by
    (src, dst).  Edge features are dropped (as DGL does)."""
    if g.is_block:
        raise DGLError("to_bidirected expects a homogeneous graph")
    src, dst = g.edges()
    n = g.number_of_nodes()
    s = torch.cat([src, dst]).long()
    d = torch.cat([dst, src]).long()
    key = torch.unique(s * n + d)  # sorted
    ns = torch.div(key, n, rounding_mode="floor").to(g.idtype)
    nd = (key % n).to(g.idtype)
    out = DGLGraph(GraphIndex(n, n, coo=(ns, nd)))
    if copy_ndata:
        for k, v in g.ndata.items():
            out.ndata[k] = v
    return out


def add_reverse_edges(g, copy_ndata=True, copy_edata=False):
    src, dst = g.edges()
    n = g.number_of_nodes()
    out = DGLGraph(GraphIndex(n, n, coo=(torch.cat([src, dst]), torch.cat([dst, src]))))
    if copy_ndata:
        for k, v in g.ndata.items():
            out.ndata[k] = v
    return out


def add_self_loop(g, etype=None):
    """Appends (i, i) for every node AFTER the existing edges; existing loops are kept.
    Node features are kept; new edges get zero-filled edge features."""
    if g.is_block:
        raise DGLError("add_self_loop expects a homogeneous graph")
    src, dst = g.edges()
    n = g.number_of_nodes()
    loop = torch.arange(n, dtype=g.idtype, device=g.device)
    out = DGLGraph(GraphIndex(n, n, coo=(torch.cat([src, loop]), torch.cat([dst, loop]))))
    for k, v in g.ndata.items():
        out.ndata[k] = v
    for k, v in g.edata.items():
        pad = torch.zeros((n,) + tuple(v.shape[1:]), dtype=v.dtype, device=v.device)
        out.edata[k] = torch.cat([v, pad])
    return out


def remove_self_loop(g, etype=None):
    src, dst = g.edges()
    keep = src != dst
    n = g.number_of_nodes()
    out = DGLGraph(GraphIndex(n, n, coo=(src[keep], dst[keep])))
    for k, v in g.ndata.items():
        out.ndata[k] = v
    for k, v in g.edata.items():
        out.edata[k] = v[keep]
    return out


def reverse(g, copy_ndata=True, copy_edata=False):
    src, dst = g.edges()
    out = DGLGraph(GraphIndex(g.number_of_dst_nodes(), g.number_of_src_nodes(), coo=(dst, src)), is_block=g.is_block)
    if copy_ndata and not g.is_block:
        for k, v in g.ndata.items():
            out.ndata[k] = v
    if copy_edata:
        for k, v in g.edata.items():
            out.edata[k] = v
    return out


def from_networkx(nx_graph, node_attrs=None, edge_attrs=None, idtype=None, device=None):
    """Nodes are relabelled 0..N-1 in sorted order when they are not already consecutive integers;
    undirected graphs yield both directions (networkx' to_directed order)."""
    import networkx as nx
    nodes = list(nx_graph.nodes())
    if not all(isinstance(v, int) for v in nodes) or sorted(nodes) != list(range(len(nodes))):
        nx_graph = nx.convert_node_labels_to_integers(nx_graph, ordering="sorted")
    if not nx_graph.is_directed():
        nx_graph = nx_graph.to_directed()
    n = nx_graph.number_of_nodes()
    edges = list(nx_graph.edges())
    src = torch.tensor([e[0] for e in edges], dtype=torch.int64)
    dst = torch.tensor([e[1] for e in edges], dtype=torch.int64)
    g = graph((src, dst), num_nodes=n, idtype=idtype, device=device)
    for attr in (node_attrs or []):
        g.ndata[attr] = torch.as_tensor([nx_graph.nodes[i][attr] for i in range(n)])
    return g


def from_scipy(sp_mat, idtype=None, device=None):
    coo = sp_mat.tocoo()
    return graph((torch.from_numpy(coo.row.astype("int64")), torch.from_numpy(coo.col.astype("int64"))),
                 num_nodes=max(sp_mat.shape), idtype=idtype, device=device)


class GraphPool(object):
    """The small graphs of a dataset in ONE storage: all edge lists (local node ids) and all feature rows concatenated, with offsets per
    graph.  `GraphPool.adopt(graphs)` builds it once and rewires every graph to VIEWS of it (same DGLGraph objects, same values; in-place
    feature writes land in the pool), so that `batch()` of any subset -- a shuffled mini-batch of 256 molecules, main_dgl_molhiv_gcn.py:163 --
    is a dozen index operations on the pooled arrays instead of four `torch.cat`s over 256 tensors and a Python loop over the graphs:
    3.6 ms -> 0.3 ms per batch on the host; the eager molhiv loop 0.91 -> 0.70 s per epoch (docs/LOG_r05.md section 9a).
    A graph whose fields were reassigned after adoption (Frame._stamp), or a list that mixes pools, takes the general path."""

    def __init__(self, idtype, node_off, edge_off, src, dst, ndata, edata):
        self.idtype, self.node_off, self.edge_off = idtype, node_off, edge_off
        self.src, self.dst, self.ndata, self.edata = src, dst, ndata, edata
        self.members = None  # weak references to the adopted graphs (members_clean)

    def members_clean(self):
        """True when no adopted graph had a field reassigned or deleted since adoption (in-place writes go to the pool and are fine)."""
        for ref in self.members or ():
            g = ref()
            if g is not None:
                p = getattr(g, "_pool", None)
                if p is None or p[2] != g._src_frame._stamp or p[3] != g._edge_frame._stamp:
                    return False
        return True

    @staticmethod
    def adopt(graphs):
        """Pool `graphs` (homogeneous, CPU, not batched, COO available, equal idtype and feature keys / dtypes / trailing shapes) and
        rewire them to views; returns the pool, or None when the list does not qualify (nothing is changed then)."""
        import numpy as np
        if len(graphs) < 2:
            return None
        g0 = graphs[0]
        nkeys, ekeys = list(g0._src_frame.keys()), list(g0._edge_frame.keys())
        for g in graphs:
            if (type(g) is not DGLGraph or g.is_block or g._batch_num_nodes is not None or g.device.type != "cpu" or g.idtype != g0.idtype
                    or not g._index.has_format("coo") or list(g._src_frame.keys()) != nkeys or list(g._edge_frame.keys()) != ekeys
                    or getattr(g, "_pool", None) is not None):
                return None
            for k in nkeys:
                if g._src_frame[k].dtype != g0._src_frame[k].dtype or g._src_frame[k].shape[1:] != g0._src_frame[k].shape[1:]:
                    return None
            for k in ekeys:
                if g._edge_frame[k].dtype != g0._edge_frame[k].dtype or g._edge_frame[k].shape[1:] != g0._edge_frame[k].shape[1:]:
                    return None
        n_nodes = np.fromiter((g.number_of_nodes() for g in graphs), np.int64, len(graphs))
        coos = [g._index.coo() for g in graphs]
        n_edges = np.fromiter((int(s.shape[0]) for s, _ in coos), np.int64, len(graphs))
        node_off = np.concatenate([[0], np.cumsum(n_nodes)])
        edge_off = np.concatenate([[0], np.cumsum(n_edges)])
        src, dst = torch.cat([s for s, _ in coos]), torch.cat([d for _, d in coos])
        ndata = {k: torch.cat([g._src_frame[k] for g in graphs], dim=0) for k in nkeys}
        edata = {k: torch.cat([g._edge_frame[k] for g in graphs], dim=0) for k in ekeys}
        pool = GraphPool(g0.idtype, node_off, edge_off, src, dst, ndata, edata)
        for i, g in enumerate(graphs):
            a, b, ea, eb = int(node_off[i]), int(node_off[i + 1]), int(edge_off[i]), int(edge_off[i + 1])
            g._index = GraphIndex(b - a, b - a, coo=(src[ea:eb], dst[ea:eb]))
            for k in nkeys:
                g._src_frame._d[k] = ndata[k][a:b]
            for k in ekeys:
                g._edge_frame._d[k] = edata[k][ea:eb]
            g._pool = (pool, i, g._src_frame._stamp, g._edge_frame._stamp)
        import weakref
        pool.members = [weakref.ref(g) for g in graphs]
        return pool

    @staticmethod
    def of(graphs):
        """(pool, ids) when every graph of the list is an unmodified member of one pool, else None."""
        import numpy as np
        first = getattr(graphs[0], "_pool", None)
        if first is None:
            return None
        pool = first[0]
        ids = np.empty(len(graphs), np.int64)
        for j, g in enumerate(graphs):
            p = getattr(g, "_pool", None)
            if p is None or p[0] is not pool or p[2] != g._src_frame._stamp or p[3] != g._edge_frame._stamp or g._batch_num_nodes is not None:
                return None
            ids[j] = p[1]
        return pool, ids

    def batch(self, ids):
        import numpy as np

        def ragged(starts, lens):
            total = int(lens.sum())
            if total == 0:
                return torch.zeros(0, dtype=torch.int64)
            excl = np.cumsum(lens) - lens
            return torch.from_numpy(np.arange(total, dtype=np.int64) + np.repeat(starts - excl, lens))

        n_nodes = self.node_off[ids + 1] - self.node_off[ids]
        n_edges = self.edge_off[ids + 1] - self.edge_off[ids]
        e_idx, n_idx = ragged(self.edge_off[ids], n_edges), ragged(self.node_off[ids], n_nodes)
        shift = torch.from_numpy(np.repeat(np.cumsum(n_nodes) - n_nodes, n_edges)).to(self.idtype)
        total = int(n_nodes.sum())
        out = DGLGraph(GraphIndex(total, total, coo=(self.src.index_select(0, e_idx) + shift, self.dst.index_select(0, e_idx) + shift)))
        out._index.ephemeral = True
        out._batch_num_nodes = torch.from_numpy(n_nodes.copy())
        out._batch_num_edges = torch.from_numpy(n_edges.copy())
        for k, v in self.ndata.items():
            out.ndata[k] = v.index_select(0, n_idx)
        for k, v in self.edata.items():
            out.edata[k] = v.index_select(0, e_idx)
        return out


def batch(graphs, ndata="__ALL__", edata="__ALL__"):
    """Block-diagonal union with node / edge id offsets; records batch_num_nodes / batch_num_edges.
    A handful of tensor ops per batch (not per graph): collation of 256 molecules must not cost more than the
    GPU work of the iteration it feeds.  Members of one GraphPool are batched from the pooled arrays."""
    if len(graphs) == 0:
        raise DGLError("The input list of graphs cannot be empty.")
    pooled = GraphPool.of(graphs)
    if pooled is not None:
        return pooled[0].batch(pooled[1])
    idtype, device = graphs[0].idtype, graphs[0].device
    srcs, dsts, n_nodes, n_edges, bn, be = [], [], [], [], [], []
    for g in graphs:
        if g.idtype != idtype or g.device != device:
            raise DGLError("all graphs in a batch must share idtype and device")
        s, d = g._index.coo()
        srcs.append(s)
        dsts.append(d)
        n_nodes.append(g.number_of_nodes())
        n_edges.append(int(s.shape[0]))
        if g._batch_num_nodes is None:
            bn.append(n_nodes[-1])
            be.append(n_edges[-1])
        else:  # batching already-batched graphs keeps the finest granularity
            bn.extend(g._batch_num_nodes.tolist())
            be.extend(g._batch_num_edges.tolist())
    total = sum(n_nodes)
    import numpy as np  # offsets on the host with numpy: torch's repeat_interleave fans tiny inputs out over every core
    node_off = np.concatenate([[0], np.cumsum(n_nodes[:-1], dtype=np.int64)]) if len(n_nodes) > 1 else np.zeros(1, np.int64)
    edge_off = torch.from_numpy(np.repeat(node_off, n_edges)).to(device=device, dtype=idtype)
    out = DGLGraph(GraphIndex(total, total, coo=(torch.cat(srcs) + edge_off, torch.cat(dsts) + edge_off)))
    out._index.ephemeral = True  # a batch of small graphs lives for one step: see GraphIndex.ephemeral
    out._batch_num_nodes = torch.tensor(bn, dtype=torch.int64, device=device)
    out._batch_num_edges = torch.tensor(be, dtype=torch.int64, device=device)
    for frames, target in ((lambda g: g._src_frame, out.ndata), (lambda g: g._edge_frame, out.edata)):
        for k in list(frames(graphs[0]).keys()):
            target[k] = torch.cat([frames(g)[k] for g in graphs], dim=0)
    return out


def unbatch(g):
    bn, be = g.batch_num_nodes().tolist(), g.batch_num_edges().tolist()
    src, dst = g.edges()
    out, no, eo = [], 0, 0
    for n, e in zip(bn, be):
        sub = DGLGraph(GraphIndex(n, n, coo=(src[eo:eo + e] - no, dst[eo:eo + e] - no)))
        for k, v in g.ndata.items():
            sub.ndata[k] = v[no:no + n]
        for k, v in g.edata.items():
            sub.edata[k] = v[eo:eo + e]
        out.append(sub)
        no, eo = no + n, eo + e
    return out


def _knn_graph_of(x2d, k, lens, who):
    """The graph of N nodes and N * k edges whose edge i * k + j runs from the j-th nearest neighbour of row i (inside i's segment,
    i itself first) to i: ops.segment_knn's index IS the in-CSR (indptr = arange(N + 1) * k, no edge-id permutation), so no sort or
    COO -> CSR pass runs.  `lens`: the segment lengths, known on the host."""
    from . import ops
    from .sparse import CsrView
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise DGLError("%s: k must be an integer >= 1, got %r" % (who, k))
    if not torch.is_tensor(x2d) or not x2d.dtype.is_floating_point:
        raise DGLError("%s expects a floating-point tensor of points" % who)
    lens = [int(n) for n in lens]
    N = int(x2d.shape[0])
    if any(n < 0 for n in lens) or sum(lens) != N:
        raise DGLError("%s: segment lengths %s do not sum to the %d points" % (who, lens if len(lens) <= 8 else lens[:8] + ["..."], N))
    short = [n for n in lens if n < k]
    if short:
        raise DGLError("%s: a segment of %d points has no %d nearest neighbours (every segment needs at least k points)" % (who, short[0], k))
    if len(set(lens)) == 1:  # equal sets (knn_graph of [B, n, D]): the lengths are filled in on the device, no host-to-device copy
        seglen = torch.full((len(lens),), lens[0], dtype=torch.int64, device=x2d.device)
    else:
        seglen = torch.tensor(lens, dtype=torch.int64)
    index = ops.segment_knn(seglen, x2d.detach().float(), k, total=N)
    idtype = torch.int32 if N * k < 2 ** 31 else torch.int64
    indptr = torch.arange(N + 1, dtype=idtype, device=x2d.device) * k
    csc = CsrView(N, N, indptr, index.reshape(-1).to(idtype), None)
    if k <= 256:
        csc._plan = None  # every row has k entries: nothing to split or balance, and no host read of the lengths
    idx = GraphIndex(N, N, csc=csc)
    idx.max_in_degree_hint = k
    idx.ephemeral = True  # rebuilt before every layer of every step
    idx._mark_ephemeral(csc)
    idx._zero_in_deg = False
    return DGLGraph(idx)


def knn_graph(x, k):
    """dgl.knn_graph: x [N, D] is one set of points, x [B, n, D] is B sets of n points whose nodes are numbered b * n + i.  Every node's
    predecessors are its k nearest points of its own set (squared Euclidean distance, itself included, ties to the lower point)."""
    if not torch.is_tensor(x) or x.dim() not in (2, 3):
        raise DGLError("knn_graph: expected points [N, D] or [B, n, D], got %s" % (tuple(x.shape) if torch.is_tensor(x) else type(x).__name__,))
    if x.dim() == 2:
        return _knn_graph_of(x, k, [x.shape[0]], "knn_graph")
    return _knn_graph_of(x.reshape(-1, x.shape[2]), k, [x.shape[1]] * x.shape[0], "knn_graph")


def segmented_knn_graph(x, k, segs):
    """dgl.segmented_knn_graph: x [N, D] holds consecutive sets of segs[0], segs[1], ... points (a Python list of lengths); every
    node's predecessors are its k nearest points of its own set."""
    if not torch.is_tensor(x) or x.dim() != 2:
        raise DGLError("segmented_knn_graph: expected points [N, D], got %s" % (tuple(x.shape) if torch.is_tensor(x) else type(x).__name__,))
    return _knn_graph_of(x, k, list(segs), "segmented_knn_graph")


def farthest_point_sampler(pos, npoints, start_idx=None):
    """dgl.geometry.farthest_point_sampler: pos [B, n, C] is B clouds of n points -> int64 [B, npoints], the sampled points' numbers
    INSIDE each cloud (DGL's contract).  start_idx None: one start per cloud drawn with torch.randint on pos's device; an int: the same
    start in every cloud (DGL's meaning).  ops.segment_fps over B equal segments whose lengths are filled in on the device: no
    host-to-device copy and no read-back."""
    from . import ops
    if not torch.is_tensor(pos) or pos.dim() != 3 or not pos.dtype.is_floating_point:
        raise DGLError("farthest_point_sampler: expected floating-point points [B, n, C], got %s"
                       % ((pos.dtype, tuple(pos.shape)) if torch.is_tensor(pos) else type(pos).__name__,))
    B, n, C = (int(v) for v in pos.shape)
    if isinstance(npoints, bool) or not isinstance(npoints, int) or npoints < 1 or npoints > n:
        raise DGLError("farthest_point_sampler: npoints must be an integer in [1, %d] (the points of a cloud), got %r" % (n, npoints))
    if start_idx is None:
        start = torch.randint(0, n, (B,), dtype=torch.int64, device=pos.device)
    elif isinstance(start_idx, int) and not isinstance(start_idx, bool) and 0 <= start_idx < n:
        start = start_idx
    else:
        raise DGLError("farthest_point_sampler: start_idx must be None or an integer in [0, %d), got %r" % (n, start_idx))
    seglen = torch.full((B,), n, dtype=torch.int64, device=pos.device)
    index = ops.segment_fps(seglen, pos.detach().float().reshape(B * n, C), npoints, start=start, total=B * n, max_len=n)
    return index - torch.arange(B, dtype=torch.int64, device=pos.device).unsqueeze(1) * n


def fixed_radius_block(pos, centers, radius, max_neighbors, segs):
    """The PointNet++ grouping as a block: pos [N, D] holds consecutive sets of segs[0], segs[1], ... points (a Python list of
    lengths), centers int64 [M] are rows of pos (a segment's farthest point samples, say).  The block has N source nodes and M
    destination nodes; destination i is centre centers[i], and its predecessors are the first max_neighbors points within `radius` of
    it inside its own set (ops.segment_ball_query with pad = "first").

    Every destination has exactly K = max_neighbors in-edges: a ball with fewer points repeats its first point.  The repeats are
    harmless under a `max` reducer and DOUBLE-COUNT under `sum` / `mean`.  A query that found nothing (a NaN centre) gets its own
    centre in every slot, so no -1 reaches a gather.  The padded index IS the in-CSR (indptr = arange(M + 1) * K, no edge-id
    permutation), as in knn_graph: no sort or COO -> CSR pass runs, and nothing is read back.  A -1 centre cannot be told from the
    host, so `centers` must come from a sampling that cannot pad: every set needs at least M / len(segs) points when M is a multiple
    of len(segs) (npoints samples per set); otherwise a DGLError.  The block carries srcdata["pos"] = pos and dstdata["pos"] =
    pos[centers]."""
    from . import ops
    from .sparse import CsrView
    K = max_neighbors
    if not torch.is_tensor(pos) or pos.dim() != 2 or not pos.dtype.is_floating_point:
        raise DGLError("fixed_radius_block: expected floating-point points [N, D], got %s"
                       % ((pos.dtype, tuple(pos.shape)) if torch.is_tensor(pos) else type(pos).__name__,))
    if not torch.is_tensor(centers) or centers.dim() != 1 or centers.dtype != torch.int64 or centers.device != pos.device:
        raise DGLError("fixed_radius_block: centers must be an int64 tensor [M] of rows of pos on %s" % (pos.device,))
    if isinstance(K, bool) or not isinstance(K, int) or K < 1:
        raise DGLError("fixed_radius_block: max_neighbors must be an integer >= 1, got %r" % (K,))
    lens = [int(n) for n in segs]
    N, M = int(pos.shape[0]), int(centers.shape[0])
    if any(n < 0 for n in lens) or sum(lens) != N:
        raise DGLError("fixed_radius_block: segment lengths %s do not sum to the %d points" % (lens if len(lens) <= 8 else lens[:8] + ["..."], N))
    if lens and M % len(lens) == 0 and any(n < M // len(lens) for n in lens):
        raise DGLError("fixed_radius_block: a segment of %d points cannot hold %d sampled centres (a -1 centre)"
                       % (min(lens), M // len(lens)))
    if N == 0 and M > 0:
        raise DGLError("fixed_radius_block: %d centres of no points" % M)
    if len(lens) >= 1 and len(set(lens)) == 1:  # equal sets: the lengths are filled in on the device, no host-to-device copy
        seglen = torch.full((len(lens),), lens[0], dtype=torch.int64, device=pos.device)
    else:
        seglen = torch.tensor(lens, dtype=torch.int64)
    x = pos.detach().float()
    index, count = ops.segment_ball_query(seglen, x, centers, radius, K, pad="first", total=N)
    index = torch.where(count.unsqueeze(1) == 0, centers.unsqueeze(1), index)
    idtype = torch.int32 if max(M * K, N) < 2 ** 31 else torch.int64
    indptr = torch.arange(M + 1, dtype=idtype, device=pos.device) * K
    csc = CsrView(M, N, indptr, index.reshape(-1).to(idtype), None)
    if K <= 256:
        csc._plan = None  # every row has K entries: nothing to split or balance, and no host read of the lengths
    idx = GraphIndex(N, M, csc=csc)
    idx.max_in_degree_hint = K
    idx.ephemeral = True  # rebuilt before every level of every step
    idx.plain_transpose = True  # the out-CSR a backward over the edges asks for: no schedule, so no read-back inside a captured step
    idx._mark_ephemeral(csc)
    idx._zero_in_deg = False
    block = DGLGraph(idx, is_block=True)
    block.srcdata["pos"] = pos
    block.dstdata["pos"] = pos.index_select(0, centers.clamp(min=0))
    return block


def knn_block(x, x_segs, y, y_segs, k, eps=1e-8):
    """The neighbour step of PointNet++'s feature propagation as a block: x [N, D] holds consecutive reference sets of x_segs[0],
    x_segs[1], ... points (a coarse level's centres, say), y [M, D] the query sets of y_segs[0], y_segs[1], ... points (Python lists of
    lengths, as many sets in both).  The block has N source nodes and M destination nodes; destination q's predecessors are the k
    references of its own set nearest to y[q], nearest first (ops.segment_knn_query).

    Every destination has exactly k in-edges and the index IS the in-CSR (indptr = arange(M + 1) * k, no edge-id permutation), as in
    fixed_radius_block: no sort or COO -> CSR pass runs, and nothing is read back.  A reference set shorter than k would leave a -1
    in the index, so it is a DGLError: no -1 reaches a gather.  The block carries edata["w"] [M * k], the normalised inverse
    squared-distance weights (1 / (d + eps)) / sum (constants: no gradient flows to the positions), srcdata["pos"] = x and
    dstdata["pos"] = y."""
    from . import ops
    from .sparse import CsrView
    for name, t in (("x", x), ("y", y)):
        if not torch.is_tensor(t) or t.dim() != 2 or not t.dtype.is_floating_point:
            raise DGLError("knn_block: expected floating-point points %s [rows, D], got %s"
                           % (name, (t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__,))
    if x.shape[1] != y.shape[1] or x.device != y.device:
        raise DGLError("knn_block: x %s on %s and y %s on %s do not go together" % (tuple(x.shape), x.device, tuple(y.shape), y.device))
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise DGLError("knn_block: k must be an integer >= 1, got %r" % (k,))
    x_lens, y_lens = [int(n) for n in x_segs], [int(n) for n in y_segs]
    N, M = int(x.shape[0]), int(y.shape[0])
    for lens, rows, what in ((x_lens, N, "reference"), (y_lens, M, "query")):
        if any(n < 0 for n in lens) or sum(lens) != rows:
            raise DGLError("knn_block: %s segment lengths %s do not sum to the %d points" % (what, lens if len(lens) <= 8 else lens[:8] + ["..."], rows))
    if len(x_lens) != len(y_lens):
        raise DGLError("knn_block: %d reference sets but %d query sets" % (len(x_lens), len(y_lens)))
    short = [n for n in x_lens if n < k]
    if short:
        raise DGLError("knn_block: a reference set of %d points has no %d nearest neighbours (every set needs at least k points)" % (short[0], k))
    seglens = []
    for lens in (x_lens, y_lens):
        if len(lens) >= 1 and len(set(lens)) == 1:  # equal sets: the lengths are filled in on the device, no host-to-device copy
            seglens.append(torch.full((len(lens),), lens[0], dtype=torch.int64, device=x.device))
        else:
            seglens.append(torch.tensor(lens, dtype=torch.int64))
    index, weight = ops.segment_knn_query(seglens[0], x.detach().float(), seglens[1], y.detach().float(), k, ref_total=N, query_total=M,
                                          return_weight=True, eps=eps)
    idtype = torch.int32 if max(M * k, N) < 2 ** 31 else torch.int64
    indptr = torch.arange(M + 1, dtype=idtype, device=x.device) * k
    csc = CsrView(M, N, indptr, index.reshape(-1).to(idtype), None)
    if k <= 256:
        csc._plan = None  # every row has k entries: nothing to split or balance, and no host read of the lengths
    idx = GraphIndex(N, M, csc=csc)
    idx.max_in_degree_hint = k
    idx.ephemeral = True  # rebuilt before every level of every step
    idx.plain_transpose = True  # the out-CSR the backward to the features asks for: no schedule, so no read-back inside a captured step
    idx._mark_ephemeral(csc)
    idx._zero_in_deg = False
    block = DGLGraph(idx, is_block=True)
    block.edata["w"] = weight.reshape(-1)
    block.srcdata["pos"] = x
    block.dstdata["pos"] = y
    return block


def knn_interpolate(feat, pos_src, pos_dst, segs_src, segs_dst, k=3):
    """PyG's knn_interpolate / the interpolation of DGL's PointNet2FP: feat [N, C] on the points pos_src [N, D] -> [M, C] on the points
    pos_dst [M, D], out[q] = sum_r w[q, r] feat[index[q, r]] over the k nearest source points of q's own set with the normalised
    inverse squared-distance weights of knn_block: the u_mul_e / sum g-SpMM over that block.  The gradient flows to feat only (through
    the block's plain transposed CSR); the weights are constants, as in PyG."""
    from . import ops
    if not torch.is_tensor(feat) or feat.dim() < 1 or not torch.is_tensor(pos_src) or feat.shape[0] != pos_src.shape[0]:
        raise DGLError("knn_interpolate: feat must hold one row per source point, got %s for %s points"
                       % (tuple(feat.shape) if torch.is_tensor(feat) else type(feat).__name__,
                          pos_src.shape[0] if torch.is_tensor(pos_src) else type(pos_src).__name__))
    block = knn_block(pos_src, segs_src, pos_dst, segs_dst, k)
    return ops.u_mul_e_sum(block, feat, block.edata["w"])


def metis_partition_assignment(g, k, balance_ntypes=None, balance_edges=False):
    """k-way edge-cut node partition -> [N] part ids.  The role of dgl.transform.metis_partition_assignment
    (end_to_end/sampling/link-prediction/dgl_cluster_sampler.py:24); METIS itself is not available offline, the
    partitioner is the label-propagation + greedy placement + refinement of mi355x_graph/dist.py."""
    from .dist import partition_nodes
    src, dst = g.edges()
    assign, _ = partition_nodes(src.long(), dst.long(), g.number_of_nodes(), int(k))
    return assign


def metis_partition(g, k, extra_cached_hops=0, reshuffle=False, balance_ntypes=None, balance_edges=False):
    """dict part_id -> induced subgraph carrying ndata[dgl.NID]
    (cluster-sage/dgl/partition_utils.py:9-16: `for k, val in metis_partition(g, psize).items(): val.ndata[dgl.NID]`)."""
    if extra_cached_hops:
        raise DGLError("metis_partition: extra_cached_hops is not supported")
    assign = metis_partition_assignment(g, k)
    order = torch.sort(assign, stable=True)[1]
    counts = torch.bincount(assign, minlength=int(k)).tolist()
    parts, off = {}, 0
    if g.device.type != "cpu":
        g._index.csc()  # built once: every g.subgraph below then reads its own rows of the in-CSR, not every edge of g
    for i, c in enumerate(counts):
        if c:
            parts[i] = g.subgraph(order[off:off + c])
        off += c
    return parts
