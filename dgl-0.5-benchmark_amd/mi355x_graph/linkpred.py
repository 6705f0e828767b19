"""Link-prediction minibatches: what turns a batch of EDGES into a training step, where the graph lives.

  dgl.dataloading.EdgeDataLoader, dgl.dataloading.negative_sampler.Uniform     end_to_end/sampling/link-prediction/
  g.edge_ids, g.has_edges_between, g.edge_subgraph, dgl.compact_graphs          (cluster_gcn_dgl.py:133-144 builds its negatives by hand)

Every piece has two forms that give the same result bit for bit -- config.DEVICE_LINKPRED chooses, CPU graphs always take the second:
  edge lookup        mgx_edge_lookup: 16 lanes scan one row of the in-CSR          | one sorted key per edge of the graph + searchsorted
  negative sampling  mgx_negative_sample: a lane group per draw, bounded redraws   | the same counter-based stream in int64 tensor arithmetic
  seed-edge removal  mgx_frontier_exclude_* (sampling.exclude_frontier_edges)      | searchsorted + a boolean mask
  compaction         mgx_compact_nodes: node bitmap walked word by word            | torch.unique(return_inverse=True)

The negatives' random stream (csrc/counter_rng.h): try t of draw (e, j) -- positive edge e of the batch, j < k -- proposes
    c = (e * k + j) * 64 + t,   r = mix64(rng_seed ^ mix64(c)),   v' = ((r >> 32) * num_dst_nodes) >> 32
mix64 the splitmix64 finaliser, all arithmetic modulo 2^64.  The first of at most max_tries proposals that is not rejected is taken;
a draw whose proposals were all rejected FAILS (its pair is dropped) -- there is no unbounded rejection loop.
"""
import math

import torch

from . import config
from ._lib import DGLError
from .graph import DGLGraph, GraphIndex
from .sampling import NID, EID, _rng_seed

NEG_MAX_TRIES = 64  # kNegMaxTries of csrc/counter_rng.h: the counter leaves 64 tries to a draw
NEG_EXCLUDE_EXISTING, NEG_EXCLUDE_SELF_LOOPS = 1, 2
DEVICE_MAX_COMPACT = 2 ** 31  # mgx_compact_nodes keeps positions in 32 bits


# ---------------------------------------------------------------------------------------------------------------- the random stream
def _s64(x):
    """A 64-bit pattern as the Python int of the same bits read as signed (what an int64 tensor holds)."""
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >> 63 else x


def _lsr(x, s):
    """Logical shift right of an int64 tensor: the arithmetic shift, then a mask over the sign copies."""
    return (x >> s) & ((1 << (64 - s)) - 1)


def _mix64_t(x):
    """mix64 of csrc/counter_rng.h on an int64 tensor (addition and multiplication wrap)."""
    x = x + _s64(0x9E3779B97F4A7C15)
    x = (x ^ _lsr(x, 30)) * _s64(0xBF58476D1CE4E5B9)
    x = (x ^ _lsr(x, 27)) * _s64(0x94D049BB133111EB)
    return x ^ _lsr(x, 31)


def negative_candidates(rng_seed, draws, t, num_dst_nodes):
    """The destination that try `t` of every draw in `draws` (int64 tensor of e * k + j) proposes."""
    r = _mix64_t(_mix64_t(draws * NEG_MAX_TRIES + int(t)) ^ _s64(int(rng_seed)))
    return (_lsr(r, 32) * int(num_dst_nodes)) >> 32


# ---------------------------------------------------------------------------------------------------------------- edge lookup
class _SortedEdges(object):
    """The composition's index: one key src * N + dst per edge, sorted stably, so that the first entry of a run of equal keys is the
    LOWEST edge id of that pair."""

    def __init__(self, idx):
        src, dst = idx.coo()
        self.n = max(idx.num_dst, 1)
        self.key, self.order = torch.sort(src.long() * self.n + dst.long(), stable=True)

    def lookup(self, u, v):
        q = u * self.n + v
        if self.key.numel() == 0:
            return torch.full_like(q, -1)
        pos = torch.searchsorted(self.key, q).clamp(max=self.key.shape[0] - 1)
        return torch.where(self.key[pos] == q, self.order[pos], torch.full_like(q, -1))


def _pair_tensors(g, u, v, what):
    dev = g.device
    u, v = torch.as_tensor(u, device=dev).long().reshape(-1), torch.as_tensor(v, device=dev).long().reshape(-1)
    if u.shape != v.shape:
        raise DGLError("%s: u and v must have the same length, got %d and %d" % (what, u.shape[0], v.shape[0]))
    return u.contiguous(), v.contiguous()


def edge_lookup(g, u, v, what="edge_ids"):
    """int64 [n]: the lowest edge id of every pair (u[i], v[i]), -1 where the graph has no such edge.  DGLError on an id out of range."""
    idx = g._index
    u, v = _pair_tensors(g, u, v, what)
    if u.is_cuda and config.DEVICE_LINKPRED:
        from . import sparse
        # rows of the in-CSR are destinations: the row of v is scanned for the column u
        eid, result = sparse.backend_for(u).edge_lookup(idx.csc(), v, u)
        if int(result[0].item()) & 4:
            raise DGLError("%s: a node id is out of range" % what)
        return eid
    if u.numel() and (int(torch.min(torch.min(u), torch.min(v))) < 0 or int(u.max()) >= idx.num_src or int(v.max()) >= idx.num_dst):
        raise DGLError("%s: a node id is out of range" % what)
    return _SortedEdges(idx).lookup(u, v)


def edge_ids(g, u, v, return_uv=False):
    """g.edge_ids(u, v): one edge id per pair, the lowest among parallel edges."""
    if return_uv:
        raise DGLError("edge_ids: return_uv=True is not supported")
    eid = edge_lookup(g, u, v, "edge_ids")
    missing = torch.nonzero(eid < 0).flatten()
    if missing.numel():
        i = int(missing[0])
        u, v = _pair_tensors(g, u, v, "edge_ids")
        raise DGLError("edge_ids: no edge between %d and %d (pair %d)" % (int(u[i]), int(v[i]), i))
    return eid.to(g.idtype)


# ---------------------------------------------------------------------------------------------------------------- negative sampling
def negative_destinations(idx, pos_src, k, flags, max_tries, rng_seed, form=None):
    """(dst int64 [len(pos_src) * k], failed draws): draw (e, j) at e * k + j, -1 where every try was rejected.
    flags: NEG_EXCLUDE_EXISTING | NEG_EXCLUDE_SELF_LOOPS.  form: "out" / "in" forces the CSR the device form checks existence in.  The
    default is the in-CSR, scanned at the proposal -- a uniformly drawn node, so an average row -- unless only the out-CSR is
    materialised: there all tries of a positive edge scan the row of its source, and the source of an edge is a hub more often than
    not (measured 2.4 - 2.6 times slower on the reddit- and products-shaped graphs, docs/LOG_linkpred.md)."""
    k, max_tries = int(k), int(max_tries)
    if k < 1:
        raise DGLError("negative sampling: k must be at least 1, got %d" % k)
    if not 1 <= max_tries <= NEG_MAX_TRIES:
        raise DGLError("negative sampling: max_tries must be in [1, %d], got %d" % (NEG_MAX_TRIES, max_tries))
    num_dst = idx.num_dst
    if num_dst >= 2 ** 31:
        raise DGLError("negative sampling: the graph must have fewer than 2^31 destination nodes")
    pos_src = pos_src.long().contiguous()
    dev = pos_src.device
    total = pos_src.shape[0] * k
    if total == 0:
        return torch.zeros(0, dtype=torch.int64, device=dev), 0
    if num_dst < 1:
        raise DGLError("negative sampling: the graph has no destination node")
    if pos_src.is_cuda and config.DEVICE_LINKPRED:
        from . import sparse
        csr, by_source = None, False
        if flags & NEG_EXCLUDE_EXISTING:
            have_in = idx._csc is not None or idx._hidden_csc is not None
            have_out = idx._csr is not None or idx._hidden_csr is not None
            by_source = (have_out and not have_in) if form is None else form == "out"
            csr = idx.csr() if by_source else idx.csc()
        dst, result = sparse.backend_for(pos_src).negative_sample(csr, by_source, pos_src, k, num_dst, flags, max_tries, rng_seed)
        failed, err = result.tolist()
        if err & 4:
            raise DGLError("negative sampling: a source node id is out of range")
        return dst, int(failed)
    edges = None
    if flags & NEG_EXCLUDE_EXISTING:
        if int(pos_src.min()) < 0 or int(pos_src.max()) >= idx.num_src:
            raise DGLError("negative sampling: a source node id is out of range")
        edges = _SortedEdges(idx)
    src = pos_src.repeat_interleave(k)
    dst = torch.full((total,), -1, dtype=torch.int64, device=dev)
    open_draws = torch.arange(total, device=dev)
    for t in range(max_tries):  # bounded, like the kernel's loop
        if open_draws.numel() == 0:
            break
        cand = negative_candidates(rng_seed, open_draws, t, num_dst)
        u = src[open_draws]
        rejected = torch.zeros_like(cand, dtype=torch.bool)
        if flags & NEG_EXCLUDE_SELF_LOOPS:
            rejected |= cand == u
        if edges is not None:
            rejected |= edges.lookup(u, cand) >= 0
        dst[open_draws[~rejected]] = cand[~rejected]
        open_draws = open_draws[rejected]
    return dst, int(open_draws.numel())


class Uniform(object):
    """dgl.dataloading.negative_sampler.Uniform(k): k negative destinations, uniform over the nodes, for the source of every edge of the
    batch.  exclude_existing rejects a destination that the source has an edge to, exclude_self_loops the source itself; a rejected
    proposal is redrawn at most max_tries - 1 times (a design constant, not a tuned one: a draw fails with probability
    (deg(u) / N) ** max_tries), then the pair is dropped -- `last_failed` counts them.  The same generator state gives the same negatives
    on every device and in both forms."""

    def __init__(self, k, exclude_existing=False, exclude_self_loops=False, max_tries=16):
        self.k, self.max_tries = int(k), int(max_tries)
        if self.k < 1:
            raise DGLError("negative_sampler.Uniform: k must be at least 1, got %d" % self.k)
        if not 1 <= self.max_tries <= NEG_MAX_TRIES:
            raise DGLError("negative_sampler.Uniform: max_tries must be in [1, %d], got %d" % (NEG_MAX_TRIES, self.max_tries))
        self.flags = (NEG_EXCLUDE_EXISTING if exclude_existing else 0) | (NEG_EXCLUDE_SELF_LOOPS if exclude_self_loops else 0)
        self.last_failed = 0

    def __call__(self, g, eids, generator=None):
        u = g.find_edges(eids)[0].long()
        dst, failed = negative_destinations(g._index, u, self.k, self.flags, self.max_tries, _rng_seed(generator))
        src = u.repeat_interleave(self.k)
        self.last_failed = failed
        if failed:
            keep = dst >= 0
            src, dst = src[keep], dst[keep]
        return src.to(g.idtype), dst.to(g.idtype)


# ---------------------------------------------------------------------------------------------------------------- compaction
def compact_nodes(num_nodes, ids, idtype=torch.int64):
    """(nodes, local): the distinct values of `ids` in ascending order (int64) and the position of every entry among them (`idtype`)."""
    ids = ids.long().contiguous()
    if ids.is_cuda and config.DEVICE_LINKPRED and ids.shape[0] < DEVICE_MAX_COMPACT:
        from . import sparse
        return sparse.backend_for(ids).compact_nodes(int(num_nodes), ids, idtype)
    if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= num_nodes):
        raise DGLError("compact_nodes: a node id is outside [0, %d)" % num_nodes)
    nodes, local = torch.unique(ids, return_inverse=True)
    return nodes, local.to(idtype)


def _local_graph(num_nodes, l_src, l_dst):
    g = DGLGraph(GraphIndex(num_nodes, num_nodes, coo=(l_src.contiguous(), l_dst.contiguous())))
    g._index.ephemeral = True  # a mini-batch graph: see GraphIndex.ephemeral
    return g


def edge_subgraph(g, eids, preserve_nodes=False):
    """g.edge_subgraph(eids): the edges `eids` in the order given; the nodes are their endpoints by ascending global id -- all nodes of
    `g` with preserve_nodes.  edata[EID] = eids, ndata[NID] = the global ids; features are sliced as g.subgraph does."""
    if g.is_block:
        raise DGLError("edge_subgraph: not defined on a block")
    eids = torch.as_tensor(eids, device=g.device)
    if eids.dtype == torch.bool:
        eids = torch.nonzero(eids).flatten()
    eids = eids.long().reshape(-1)
    u, v = g.find_edges(eids)
    n = g.number_of_nodes()
    if preserve_nodes:
        nodes = torch.arange(n, device=g.device)
        sub = _local_graph(n, u, v)
    else:
        nodes, local = compact_nodes(n, torch.cat([u.long(), v.long()]), g.idtype)
        sub = _local_graph(nodes.shape[0], local[:u.shape[0]], local[u.shape[0]:])
    for k, x in g.ndata.items():
        sub.ndata[k] = x if preserve_nodes else x[nodes.to(x.device)]
    for k, x in g.edata.items():
        sub.edata[k] = x[eids.to(x.device)]
    sub.ndata[NID] = nodes
    sub.edata[EID] = eids
    return sub


def compact_graphs(graphs, always_preserve=None):
    """dgl.compact_graphs: graphs over one node set -> the same edges over the nodes that any of them uses (as an endpoint of an edge),
    plus `always_preserve`.  The kept nodes are numbered by ASCENDING global id (DGL leaves the order unspecified); ndata[NID] of every
    returned graph holds them, node features are sliced, edge features carried over.  A single graph in, a single graph out."""
    single = isinstance(graphs, DGLGraph)
    graphs = [graphs] if single else list(graphs)
    if not graphs:
        return []
    n, dev, idtype = graphs[0].number_of_nodes(), graphs[0].device, graphs[0].idtype
    for g in graphs:
        if g.is_block or g.number_of_nodes() != n:
            raise DGLError("compact_graphs: the graphs must be homogeneous graphs over the same %d nodes" % n)
    ends = [t.long() for g in graphs for t in g.edges()]
    if always_preserve is not None:
        ends.append(torch.as_tensor(always_preserve, device=dev).long().reshape(-1))
    nodes, local = compact_nodes(n, torch.cat(ends), idtype)
    out, at = [], 0
    for g in graphs:
        m = g.number_of_edges()
        c = _local_graph(nodes.shape[0], local[at:at + m], local[at + m:at + 2 * m])
        at += 2 * m
        for k, x in g.ndata.items():
            c.ndata[k] = x[nodes.to(x.device)]
        for k, x in g.edata.items():
            c.edata[k] = x
        c.ndata[NID] = nodes
        out.append(c)
    return out[0] if single else out


# ---------------------------------------------------------------------------------------------------------------- the loader
class EdgeDataLoader(object):
    """Iterates (input_nodes, pair_graph, blocks) -- with a negative sampler (input_nodes, pair_graph, neg_graph, blocks) -- over
    mini-batches of edge ids.  pair_graph holds the batch's edges and neg_graph the negative pairs, both over the batch's compacted
    endpoints (ascending global id, ndata[NID]); blocks[-1].dstdata[NID] equals pair_graph.ndata[NID], so the model's output rows are
    the pair graphs' nodes and a score is pair_graph.apply_edges(fn.u_dot_v(...)).

    exclude: None | "self" (the batch's edge ids are taken out of every sampled frontier) | "reverse_id" (and reverse_eids[batch]).
    g_sampling: the graph the neighbourhoods are sampled from (default g; its edge ids must be g's for `exclude` to mean anything).
    generator: draws the shuffle, the neighbour samples and the negatives; num_workers is accepted and ignored (sampling runs where the
    graph lives)."""

    def __init__(self, g, eids, block_sampler, device=None, batch_size=1, shuffle=False, drop_last=False, exclude=None,
                 reverse_eids=None, negative_sampler=None, g_sampling=None, generator=None, num_workers=0):
        if exclude not in (None, "self", "reverse_id"):
            raise DGLError("EdgeDataLoader: exclude must be None, 'self' or 'reverse_id', got %r" % (exclude,))
        if exclude == "reverse_id" and reverse_eids is None:
            raise DGLError("EdgeDataLoader: exclude='reverse_id' needs reverse_eids")
        self.g, self.sampler, self.g_sampling = g, block_sampler, (g if g_sampling is None else g_sampling)
        self.eids = torch.as_tensor(eids)
        if self.eids.dtype == torch.bool:
            self.eids = torch.nonzero(self.eids).flatten()
        self.eids = self.eids.long().reshape(-1)
        self.batch_size, self.shuffle, self.drop_last = int(batch_size), shuffle, drop_last
        self.device, self.exclude, self.negative_sampler, self.generator = device, exclude, negative_sampler, generator
        self.reverse_eids = None if reverse_eids is None else torch.as_tensor(reverse_eids).long().to(g.device)

    def __len__(self):
        n = self.eids.shape[0]
        return n // self.batch_size if self.drop_last else math.ceil(n / self.batch_size)

    def _batch(self, batch):
        g, gen = self.g, self.generator
        u, v = g.find_edges(batch)
        ends = [u.long(), v.long()]
        if self.negative_sampler is not None:
            nu, nv = self.negative_sampler(g, batch, generator=gen)
            ends += [nu.long(), nv.long()]
        nodes, local = compact_nodes(g.number_of_nodes(), torch.cat(ends), g.idtype)
        b = batch.shape[0]
        pair = _local_graph(nodes.shape[0], local[:b], local[b:2 * b])
        pair.ndata[NID] = nodes
        pair.edata[EID] = batch
        graphs = [pair]
        if self.negative_sampler is not None:
            m = nu.shape[0]
            neg = _local_graph(nodes.shape[0], local[2 * b:2 * b + m], local[2 * b + m:])
            neg.ndata[NID] = nodes
            graphs.append(neg)
        excl = None
        if self.exclude == "self":
            excl = batch
        elif self.exclude == "reverse_id":
            excl = torch.cat([batch, self.reverse_eids[batch]])
        blocks = self.sampler.sample_blocks(self.g_sampling, nodes, exclude_eids=excl, generator=gen)
        if self.device is not None:
            graphs = [x.to(self.device) for x in graphs]
            blocks = [x.to(self.device) for x in blocks]
        return tuple([blocks[0].srcdata[NID]] + graphs + [blocks])

    def __iter__(self):
        eids, gen = self.eids, self.generator
        if self.shuffle:
            perm = torch.randperm(eids.shape[0], generator=gen, device="cpu" if gen is None else gen.device)
            eids = eids[perm.to(eids.device)]
        eids = eids.to(self.g.device)
        for i in range(len(self)):
            yield self._batch(eids[i * self.batch_size:(i + 1) * self.batch_size])
