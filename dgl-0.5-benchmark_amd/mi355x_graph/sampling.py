"""Neighbor sampling and message-flow blocks (the callers on the other side of the hot
path -- bipartite "block" graphs on which the same g-SpMM / g-SDDMM kernels run with N_src != N_dst).

  dgl.dataloading.MultiLayerNeighborSampler(fanouts), NodeDataLoader(g, nids, sampler, batch_size=...)
      end_to_end/sampling/node-classification/reddit/ns-sage-dgl.py:132-141,159-165 (training),
      :67-75 (full-neighbour inference with fanout None)
  dgl.to_block, dgl.sampling.sample_neighbors, g.subgraph(mask)   reddit/load_graph.py:45-51

  dgl.sampling.sample_neighbors(g, seeds, fanout, replace=True), dgl.in_subgraph
      end_to_end/sampling/node-classification/ogbn-product/ns-gat/ns-gat-dgl.py:22-42 (a hand-written NeighborSampler)

Sampling is index work done where the graph lives (the reference samples in CPU worker processes; sampling next to
the features on the GPU removes the host round trip): HIP kernels (csrc/sample.hip) for device graphs and fanout <= 64,
torch integer ops of the same semantics otherwise.  Semantics follow DGL's sample_neighbors: over the in-edges of each
seed (edge_dir="out": the out-edges), uniformly or proportionally to a non-negative edge weight (`prob`, an edge of
weight 0 is never picked), without replacement (a row with no more than `fanout` eligible edges keeps them all) or with
(`fanout` independent draws for every row that has an eligible edge; duplicates stay, as multi-edges); select_topk is
the deterministic sibling.  Every mode returns its edges grouped by seed in seed order, CSR positions non-decreasing
inside a seed.  Destination nodes of a block are a prefix of its source nodes (block.srcdata[NID][:num_dst] ==
block.dstdata[NID]).  The relabelling that follows -- to_block, g.subgraph(nodes) -- runs on the device too (csrc/relabel.hip),
next to the torch compositions it is compared with (config.DEVICE_BLOCKS, config.DEVICE_SUBGRAPH).
"""
import math

import torch

from . import config
from ._lib import DGLError
from .graph import DGLGraph, GraphIndex

NID = "_ID"
EID = "_ID"


DEVICE_MAX_FANOUT = 64  # fanout / k the HIP kernels take (include/mi355x_graph.h); above it the torch formulation runs
DEVICE_MAX_BLOCK_IDS = 2 ** 31  # mgx_to_block keeps local ids in 32 bits: destinations + edges below this, else the torch formulation


def _rng_seed(generator):
    if generator is None or generator.device.type == "cpu":
        return int(torch.randint(0, 2 ** 62, (1,), generator=generator).item())
    return int(torch.randint(0, 2 ** 62, (1,), generator=generator, device=generator.device).item())


def _rand(n, dev, generator):
    """n fp64 numbers in [0, 1) on `dev`, drawn from `generator` on whichever device it lives."""
    if generator is not None and generator.device != torch.device(dev):
        return torch.rand(n, generator=generator, dtype=torch.float64, device=generator.device).to(dev)
    return torch.rand(n, device=dev, generator=generator, dtype=torch.float64)


def _edge_weights(g, idx, w, what):
    """`w` (the name of an edge feature or a tensor) -> a contiguous fp32 vector with one weight per edge id, where the graph lives."""
    if isinstance(w, str):
        if not isinstance(g, DGLGraph) or w not in g.edata:
            raise DGLError("%s: the graph has no edge feature %r" % (what, w))
        w = g.edata[w]
    w = torch.as_tensor(w)
    if w.dim() != 1 or w.shape[0] != idx.num_edges() or not (w.is_floating_point()):
        raise DGLError("%s: expected one floating-point weight per edge (%d), got a tensor of shape %s, %s"
                       % (what, idx.num_edges(), tuple(w.shape), w.dtype))
    return w.detach().to(device=idx.device, dtype=torch.float32).contiguous()


def _candidates(view, nodes):
    """Every stored edge of the rows `nodes` of `view`, row after row: (CSR positions, seed slot of each, first candidate of each
    slot, row lengths)."""
    dev = view.device
    indptr = view.indptr.long()
    beg = indptr[nodes]
    deg = indptr[nodes + 1] - beg
    total = int(deg.sum().item())
    seg = torch.repeat_interleave(torch.arange(nodes.shape[0], device=dev), deg, output_size=total)
    first = torch.cumsum(deg, 0) - deg
    pos = torch.arange(total, device=dev) - first[seg] + beg[seg]
    return pos, seg, first, deg


def _smallest_per_segment(key, seg, first, k, eligible=None):
    """Candidate numbers of the k smallest keys of every segment (equal keys: the earlier candidate), in candidate order."""
    order = torch.argsort(key, stable=True)
    order = order[torch.argsort(seg[order], stable=True)]  # by segment, by key inside a segment, by position among equal keys
    rank = torch.arange(key.shape[0], device=key.device) - first[seg[order]]
    keep = rank < k
    if eligible is not None:  # ineligible candidates carry +inf keys: they sort after every eligible one of their segment
        keep &= eligible[order]
    return torch.sort(order[keep])[0]


def _sample_torch(view, nodes, fanout, w, replace, generator):
    """sample_neighbors in torch ops (CPU graphs, fanout above the device limit); `w`: per-edge-id weights or None.
    Returns (CSR positions, seed slot of each pick)."""
    dev = view.device
    pos, seg, first, deg = _candidates(view, nodes)
    total = pos.shape[0]
    eligible = None
    if w is not None:
        wc = w[pos if view.eids is None else view.eids[pos].long()]
        if bool((~(wc >= 0) | torch.isinf(wc)).any()):
            raise DGLError("sample_neighbors: edge weights must be finite and non-negative")
        eligible = wc > 0
    if total == 0:
        return pos, seg
    if fanout is None or fanout < 0:  # every (eligible) edge
        return (pos, seg) if eligible is None else (pos[eligible], seg[eligible])
    if not replace:
        u = 1.0 - _rand(total, dev, generator)  # (0, 1]
        if w is None:
            key = u
        else:  # Efraimidis-Spirakis: the k smallest -log(u) / w are k successive draws proportional to w without replacement
            key = torch.where(eligible, -torch.log(u) / wc.double(), torch.full_like(u, float("inf")))
        keep = _smallest_per_segment(key, seg, first, fanout, eligible)
        return pos[keep], seg[keep]
    n_seeds = nodes.shape[0]
    ar = torch.arange(total, device=dev)
    if w is None:
        active = torch.nonzero(deg > 0).flatten()
    else:
        # last eligible candidate of every slot: where a target that rounding pushed to the row total (or past it) lands
        last = torch.full((n_seeds,), -1, dtype=torch.int64, device=dev)
        last.scatter_reduce_(0, seg[eligible], ar[eligible], "amax", include_self=True)
        active = torch.nonzero(last >= 0).flatten()
    slot = torch.repeat_interleave(active, fanout)  # slot of every draw, `fanout` draws per slot that has an eligible edge
    u = _rand(slot.shape[0], dev, generator)
    if w is None:
        pick = first[slot] + torch.minimum((u * deg[slot].double()).long(), deg[slot] - 1)
    else:
        # inverse CDF: one running sum over all candidates (fp64; a weight of 0 repeats its predecessor's sum bit for bit), each
        # slot's stretch of it starts at `start`; the first candidate whose inclusive sum is strictly above start + u * W
        csum = torch.cumsum(wc.double(), 0)
        start = torch.where(first > 0, csum[torch.clamp(first - 1, min=0)], torch.zeros((), dtype=torch.float64, device=dev))
        row_total = csum[torch.clamp(first + deg - 1, min=0)] - start
        target = start[slot] + u * row_total[slot]
        pick = torch.minimum(torch.searchsorted(csum, target, right=True), last[slot])
    pick = torch.sort(pick)[0]  # candidate numbers grow with the slot, then with the CSR position: one sort gives the output order
    return pos[pick], seg[pick]


def _triple(view, nodes, pos, seg, edge_dir):
    picked = view.indices[pos].long()
    seeds = nodes[seg]
    eid = pos if view.eids is None else view.eids[pos].long()
    return (picked, seeds, eid) if edge_dir == "in" else (seeds, picked, eid)


def _view(idx, edge_dir, what):
    if edge_dir not in ("in", "out"):
        raise DGLError("%s: edge_dir must be 'in' or 'out', got %r" % (what, edge_dir))
    return idx.csc() if edge_dir == "in" else idx.csr()


def _sample_modes(g, idx, nodes, fanout, edge_dir, prob, replace, generator, want_counts=False):
    """Every mode but the uniform in-edge one without replacement: prob=, replace=True, edge_dir='out'.  Returns (src, dst, eid) and the
    edges per seed (None unless `want_counts`)."""
    view = _view(idx, edge_dir, "sample_neighbors")
    dev = view.device
    nodes = torch.as_tensor(nodes, device=dev).long()
    w = None if prob is None else _edge_weights(g, idx, prob, "sample_neighbors")
    if nodes.is_cuda and fanout is not None and 1 <= fanout <= DEVICE_MAX_FANOUT:
        from . import sparse
        backend = sparse.backend_for(view.indptr)
        seeds = nodes.to(view.indptr.dtype)
        if w is None and not replace:  # uniform without replacement over the out-CSR: the kernel of the in-edge path
            picked, eid, counts = backend.sample_neighbors(view, seeds, fanout, _rng_seed(generator))
        else:
            picked, eid, counts = backend.sample_neighbors_modes(view, seeds, fanout, w, replace, _rng_seed(generator))
        seeds = torch.repeat_interleave(nodes, counts, output_size=picked.shape[0])
        return ((picked.long(), seeds, eid.long()) if edge_dir == "in" else (seeds, picked.long(), eid.long())), counts
    pos, seg = _sample_torch(view, nodes, fanout, w, replace, generator)
    return _triple(view, nodes, pos, seg, edge_dir), (torch.bincount(seg, minlength=nodes.shape[0]) if want_counts else None)


def select_topk(g, k, weight, nodes=None, edge_dir="in", ascending=False):
    """(src, dst, eid) in GLOBAL ids of the `k` in-edges (edge_dir="out": out-edges) of largest `weight` -- smallest with
    `ascending` -- of every node, or of every node of `nodes`; all of them where the degree is <= k (k None / -1: everywhere).
    `weight`: the name of an edge feature or one value per edge id.  Equal weights go to the lower CSR position; the output
    order is that of sample_neighbors."""
    idx = g._index if isinstance(g, DGLGraph) else g
    view = _view(idx, edge_dir, "select_topk")
    dev = view.device
    nodes = torch.arange(view.num_rows, device=dev) if nodes is None else torch.as_tensor(nodes, device=dev).long()
    w = _edge_weights(g, idx, weight, "select_topk")
    if nodes.is_cuda and k is not None and 1 <= k <= DEVICE_MAX_FANOUT:
        from . import sparse
        picked, eid, counts = sparse.backend_for(view.indptr).select_topk(view, nodes.to(view.indptr.dtype), k, w, ascending)
        seeds = torch.repeat_interleave(nodes, counts, output_size=picked.shape[0])
        return (picked.long(), seeds, eid.long()) if edge_dir == "in" else (seeds, picked.long(), eid.long())
    pos, seg, first, deg = _candidates(view, nodes)
    if pos.shape[0] and k is not None and k >= 0:
        wc = w[pos if view.eids is None else view.eids[pos].long()] + 0.0  # + 0: -0 and +0 are one key, as in the kernel
        keep = _smallest_per_segment(wc if ascending else -wc, seg, first, k)
        pos, seg = pos[keep], seg[keep]
    return _triple(view, nodes, pos, seg, edge_dir)


def in_subgraph(g, nodes):
    """Every in-edge of `nodes` as (src, dst, eid) in GLOBAL ids (ns-gat-dgl.py:34 builds its last frontier with it)."""
    return sample_neighbors(g, nodes, None)


def sample_neighbors(g, nodes, fanout, edge_dir="in", prob=None, replace=False, generator=None):
    """Returns (src, dst, eid) of the sampled in-edges (edge_dir="out": out-edges) of `nodes` in GLOBAL ids.
    prob: the name of an edge feature or one non-negative weight per edge id; replace: draw with replacement."""
    return _sample_frontier(g, nodes, fanout, edge_dir, prob, replace, generator)[0]


def _sample_frontier(g, nodes, fanout, edge_dir="in", prob=None, replace=False, generator=None, want_counts=False):
    """sample_neighbors, and with it the edges per seed (int64 [len(nodes)]; None unless `want_counts`): the frontier as the rows of a
    CSR over the seeds, which is what the seed-edge exclusion of a link-prediction batch walks."""
    idx = g._index if isinstance(g, DGLGraph) else g
    if edge_dir != "in" or prob is not None or replace:
        return _sample_modes(g, idx, nodes, fanout, edge_dir, prob, replace, generator, want_counts)
    csc = idx.csc()
    dev = csc.device
    nodes = torch.as_tensor(nodes, device=dev).long()
    if nodes.is_cuda and fanout is not None and 1 <= fanout <= 64:
        # device path: mgx_sample_neighbors (one thread per seed, Floyd's algorithm); the torch formulation below
        # sorts every candidate edge (12 M for a 25 k-node reddit frontier) and is kept for CPU graphs
        from . import sparse
        rng_seed = int(torch.randint(0, 2 ** 62, (1,), generator=generator).item()) if (generator is None or generator.device.type == "cpu") \
            else int(torch.randint(0, 2 ** 62, (1,), generator=generator, device=generator.device).item())
        src, eid, counts = sparse.backend_for(csc.indptr).sample_neighbors(csc, nodes.to(csc.indptr.dtype), fanout, rng_seed)
        dst = torch.repeat_interleave(nodes, counts)
        return (src.long(), dst, eid.long()), counts
    indptr = csc.indptr.long()
    beg = indptr[nodes]
    deg = indptr[nodes + 1] - beg
    total = int(deg.sum().item())
    if total == 0:
        z = torch.zeros(0, dtype=torch.int64, device=dev)
        return (z, z, z), deg
    seg = torch.repeat_interleave(torch.arange(nodes.shape[0], device=dev), deg)
    first = torch.cumsum(deg, 0) - deg
    pos = torch.arange(total, device=dev) - first[seg] + beg[seg]  # CSR positions of every candidate edge
    if fanout is not None and fanout >= 0 and bool((deg > fanout).any()):
        key = torch.rand(total, device=dev, generator=generator, dtype=torch.float64)
        order = torch.argsort(seg.double() + key * 0.999999)  # random order inside each seed's segment
        rank = torch.arange(total, device=dev) - first[seg[order]]
        keep = order[rank < fanout]
        keep, _ = torch.sort(keep)  # keep CSR order: deterministic block layout for a given draw
        pos, seg = pos[keep], seg[keep]
    src = csc.indices[pos].long()
    dst = nodes[seg]
    eid = pos if csc.eids is None else csc.eids[pos].long()
    return (src, dst, eid), (torch.bincount(seg, minlength=nodes.shape[0]) if want_counts else None)


def exclude_frontier_edges(frontier, counts, seeds, excl):
    """(src, dst, eid) of a frontier -- edges grouped by seed, counts[i] of them for seeds[i] -- without the edges whose id is in
    `excl` (int64 on the frontier's device, ASCENDING).  DGL's semantics: sample first, then remove (a seed may end with fewer than `fanout` edges).  Kept edges keep their
    order, so the result is again grouped by seed in seed order.  On the device with config.DEVICE_LINKPRED the count / cumsum / fill
    kernels of csrc/relabel.hip (a bisection per edge in the sorted list), else the same in torch ops."""
    src, dst, eid = frontier
    if src.is_cuda and config.DEVICE_LINKPRED:
        from . import sparse
        backend = sparse.backend_for(src)
        offsets = backend._sample_offsets(counts.long())
        src, eid, kept = backend.frontier_exclude(offsets, src.contiguous(), eid.contiguous(), excl.contiguous())
        return src, torch.repeat_interleave(seeds, kept, output_size=src.shape[0]), eid
    if excl.numel() == 0 or eid.numel() == 0:
        return src, dst, eid
    pos = torch.searchsorted(excl, eid).clamp(max=excl.shape[0] - 1)
    keep = excl[pos] != eid
    return src[keep], dst[keep], eid[keep]


def to_block(g_or_edges, dst_nodes, num_nodes=None, idtype=torch.int64, dst_sorted=False, max_in_degree=None):
    """Bipartite block: dst = `dst_nodes` (kept in order), src = dst_nodes followed by the other sources.
    `g_or_edges` is (src, dst[, eid]) in global ids."""
    src, dst = g_or_edges[0].long(), g_or_edges[1].long()
    eid = g_or_edges[2] if len(g_or_edges) > 2 else None
    dev = src.device
    dst_nodes = torch.as_tensor(dst_nodes, device=dev).long()
    if num_nodes is None:
        num_nodes = int(max(src.max().item() if src.numel() else 0, dst_nodes.max().item() if dst_nodes.numel() else 0)) + 1
    indptr = None
    if src.is_cuda and config.DEVICE_BLOCKS and dst_nodes.shape[0] + src.shape[0] < DEVICE_MAX_BLOCK_IDS:
        # device path: mgx_to_block (csrc/relabel.hip) -- a bitmap gives the ascending order of the other sources without a sort, the
        # in-CSR's row pointer comes from the same pass as the local ids; one host read.  The composition below is kept for CPU graphs
        from . import sparse
        dst_nodes = dst_nodes.contiguous()
        src_nodes, l_src, l_dst, indptr = sparse.backend_for(src).to_block(int(num_nodes), dst_nodes, src.contiguous(), dst.contiguous(),
                                                                           dst_sorted, idtype)
    else:
        lut = torch.full((num_nodes,), -1, dtype=torch.int64, device=dev)
        lut[dst_nodes] = torch.arange(dst_nodes.shape[0], device=dev)
        if int((lut[dst] < 0).sum().item()):
            raise DGLError("to_block: every edge destination must be one of dst_nodes")
        uniq = torch.unique(src)
        extra = uniq[lut[uniq] < 0]
        lut[extra] = dst_nodes.shape[0] + torch.arange(extra.shape[0], device=dev)
        src_nodes = torch.cat([dst_nodes, extra])
        l_src, l_dst = lut[src].to(idtype).contiguous(), lut[dst].to(idtype).contiguous()
    csc = None
    if dst_sorted:  # edges arrive grouped by destination in dst_nodes order: the in-CSR is a cumsum away (no sort)
        from .sparse import CsrView
        if indptr is None:
            indptr = torch.zeros(dst_nodes.shape[0] + 1, dtype=torch.int64, device=dev)
            torch.cumsum(torch.bincount(l_dst.long(), minlength=dst_nodes.shape[0]), 0, out=indptr[1:])
        csc = CsrView(dst_nodes.shape[0], src_nodes.shape[0], indptr.to(idtype), l_src, None)
        csc.dst_is_src_prefix = True
        if max_in_degree is not None and max_in_degree <= 256:
            csc._plan = None  # no row can need splitting and the block is tiny: skip the schedule (and its host syncs)
    block = DGLGraph(GraphIndex(src_nodes.shape[0], dst_nodes.shape[0], coo=(l_src, l_dst), csc=csc), is_block=True)
    block._index.dst_is_src_prefix = True
    block._index.max_in_degree_hint = max_in_degree
    block._index.ephemeral = True  # one training step: kernel forms from host-known numbers, no analysis of the row lengths
    if csc is not None:
        block._index._mark_ephemeral(csc)
    block.srcdata[NID] = src_nodes
    block.dstdata[NID] = dst_nodes
    if eid is not None:
        block.edata[EID] = eid
    return block


class MultiLayerNeighborSampler(object):
    """fanouts[i] = neighbours sampled for layer i (None / -1: all neighbours)."""

    def __init__(self, fanouts, replace=False, return_eids=False, prob=None):
        self.fanouts = list(fanouts)
        self.replace, self.prob = bool(replace), prob

    def sample_blocks(self, g, seed_nodes, exclude_eids=None, generator=None):
        """exclude_eids: edge ids taken out of every layer's frontier before the block is built (the seed edges of a link-prediction
        batch and their reverses: sampling them back in would leak the label)."""
        blocks = []
        seeds = torch.as_tensor(seed_nodes, device=g.device).long()
        n = g.number_of_nodes()
        if exclude_eids is not None:
            exclude_eids = torch.sort(torch.as_tensor(exclude_eids, device=g.device).long().reshape(-1))[0]
        for fanout in reversed(self.fanouts):
            frontier, counts = _sample_frontier(g, seeds, fanout, prob=self.prob, replace=self.replace, generator=generator,
                                                want_counts=exclude_eids is not None)
            # sample_neighbors returns edges grouped by seed in seed order (CSR positions sorted inside a seed); dropping edges keeps
            # that, so the dst-sorted in-CSR below comes from the counts after the exclusion
            if exclude_eids is not None:
                frontier = exclude_frontier_edges(frontier, counts, seeds, exclude_eids)
            block = to_block(frontier, seeds, num_nodes=n, idtype=g.idtype, dst_sorted=True,
                             max_in_degree=fanout if (fanout is not None and fanout >= 0) else None)
            seeds = block.srcdata[NID]
            blocks.insert(0, block)
        return blocks


class MultiLayerFullNeighborSampler(MultiLayerNeighborSampler):
    def __init__(self, n_layers, return_eids=False):
        super(MultiLayerFullNeighborSampler, self).__init__([None] * n_layers)


class NodeDataLoader(object):
    """Iterates (input_nodes, output_nodes, blocks) over mini-batches of seed nodes."""

    def __init__(self, g, nids, block_sampler, device=None, batch_size=1, shuffle=False, drop_last=False,
                 num_workers=0, **kwargs):
        self.g, self.sampler = g, block_sampler
        self.nids = torch.as_tensor(nids).long()
        if self.nids.dtype == torch.bool:
            self.nids = torch.nonzero(self.nids).flatten()
        self.batch_size, self.shuffle, self.drop_last = int(batch_size), shuffle, drop_last
        self.device = device  # num_workers is accepted and ignored: sampling runs where the graph lives

    def __len__(self):
        n = self.nids.shape[0]
        return n // self.batch_size if self.drop_last else math.ceil(n / self.batch_size)

    def __iter__(self):
        nids = self.nids
        if self.shuffle:
            nids = nids[torch.randperm(nids.shape[0])]
        nids = nids.to(self.g.device)
        for i in range(len(self)):
            seeds = nids[i * self.batch_size:(i + 1) * self.batch_size]
            blocks = self.sampler.sample_blocks(self.g, seeds)
            if self.device is not None:
                blocks = [b.to(self.device) for b in blocks]
            yield blocks[0].srcdata[NID], blocks[-1].dstdata[NID], blocks


def _node_subgraph_device(g, parent_csc, nodes):
    """node_subgraph over the parent's materialised in-CSR (mgx_node_subgraph_count / _fill, csrc/relabel.hip): only the rows of the
    selected nodes are read, not every edge of the parent.  Same result as the composition in node_subgraph."""
    from . import sparse
    n_sel = nodes.shape[0]
    l_src, l_dst, parent_eid, offsets, rows_by_eid = sparse.backend_for(nodes).node_subgraph(parent_csc, nodes, g.idtype)
    sorted_eid, order = torch.sort(parent_eid)  # the kept edges only; edge order of the subgraph: ascending parent edge id
    csc = None
    if rows_by_eid:
        # the kernel's row-by-row order IS the subgraph's in-CSR (what a stable sort of its COO by destination gives): hand it over
        # and save the first aggregation that sort.  eids: CSR position -> new edge id, the inverse of `order`
        inv = torch.empty_like(order)
        inv[order] = torch.arange(order.shape[0], device=order.device)
        csc = sparse.CsrView(n_sel, n_sel, offsets.to(g.idtype), l_src, inv.to(g.idtype))
    sub = DGLGraph(GraphIndex(n_sel, n_sel, coo=(l_src[order], l_dst[order]), csc=csc))
    sub._index.ephemeral = True  # a cluster / mini-batch subgraph: see GraphIndex.ephemeral
    if csc is not None:
        sub._index._mark_ephemeral(csc)
    for k, v in g.ndata.items():
        sub.ndata[k] = v[nodes.to(v.device)]
    for k, v in g.edata.items():
        sub.edata[k] = v[sorted_eid.to(v.device)]
    sub.ndata[NID] = nodes
    sub.edata[EID] = sorted_eid
    return sub


def node_subgraph(g, nodes):
    """g.subgraph(nodes | mask): induced subgraph with relabelled nodes; node features are sliced."""
    dev = g.device
    if isinstance(nodes, dict):  # {ntype: ids} of a graph with one node type (dgl_cluster_sampler.py:99)
        if len(nodes) != 1:
            raise DGLError("subgraph: a homogeneous graph takes the nodes of exactly one type")
        nodes = next(iter(nodes.values()))
    nodes = torch.as_tensor(nodes, device=dev)
    if nodes.dtype == torch.bool:
        nodes = torch.nonzero(nodes).flatten()
    nodes = nodes.long()
    n = g.number_of_nodes()
    parent_csc = g._index._csc if g._index._csc is not None else g._index._hidden_csc
    if nodes.is_cuda and config.DEVICE_SUBGRAPH and parent_csc is not None and not g.is_block:
        return _node_subgraph_device(g, parent_csc, nodes.contiguous())
    lut = torch.full((n,), -1, dtype=torch.int64, device=dev)
    lut[nodes] = torch.arange(nodes.shape[0], device=dev)
    src, dst = g.edges()
    ls, ld = lut[src.long()], lut[dst.long()]
    keep = (ls >= 0) & (ld >= 0)
    sub = DGLGraph(GraphIndex(nodes.shape[0], nodes.shape[0], coo=(ls[keep].to(g.idtype).contiguous(), ld[keep].to(g.idtype).contiguous())))
    sub._index.ephemeral = True  # a cluster / mini-batch subgraph: see GraphIndex.ephemeral
    for k, v in g.ndata.items():
        sub.ndata[k] = v[nodes.to(v.device)]
    for k, v in g.edata.items():
        sub.edata[k] = v[keep.to(v.device)]
    sub.ndata[NID] = nodes
    sub.edata[EID] = torch.nonzero(keep).flatten()
    return sub
