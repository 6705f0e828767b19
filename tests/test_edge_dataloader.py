"""dgl.dataloading.EdgeDataLoader and what it is made of: seed-edge exclusion (mgx_frontier_exclude_*), compaction (mgx_compact_nodes),
g.edge_subgraph, dgl.compact_graphs -- each against a plain-Python restatement, the device form against the torch form bit for bit.
"""
import ctypes
import os
import sys

import pytest
import torch

import mi355x_graph as mg
from mi355x_graph import _lib, config, linkpred, sampling, sparse
from mi355x_graph.sampling import NID, EID

import dgl
from dgl.dataloading import EdgeDataLoader, MultiLayerNeighborSampler
from dgl.dataloading.negative_sampler import Uniform

from test_edge_lookup import build_case

DEV = "cuda:0"
IDTYPES = [torch.int32, torch.int64]
K = 2
LOADER_SEED = 3  # chosen on the CPU: with exclude=None some block of the epoch samples a seed edge or its reverse back in


def bidirected_graph(dev, idtype=torch.int64):
    """About 200 nodes, 600 random pairs stored in both directions: the reverse of edge e is (e + E / 2) % E."""
    gen = torch.Generator().manual_seed(21)
    s, d = torch.randint(0, 200, (600,), generator=gen), torch.randint(0, 200, (600,), generator=gen)
    g = mg.graph((torch.cat([s, d]).to(idtype), torch.cat([d, s]).to(idtype)), num_nodes=200).to(dev)
    E = g.number_of_edges()
    return g, (torch.arange(E) + E // 2) % E


def run_epoch(dev, exclude, idtype=torch.int64, negatives=True):
    g, reverse = bidirected_graph(dev, idtype)
    gen = torch.Generator().manual_seed(LOADER_SEED)
    eids = torch.randperm(g.number_of_edges(), generator=torch.Generator().manual_seed(1))[:100]
    loader = EdgeDataLoader(g, eids, MultiLayerNeighborSampler([3, 3]), batch_size=32, shuffle=True, exclude=exclude,
                            reverse_eids=reverse if exclude == "reverse_id" else None,
                            negative_sampler=Uniform(K) if negatives else None, generator=gen, num_workers=4)
    assert len(loader) == 4
    return g, reverse.to(dev), list(loader)


def batch_tensors(batch):
    """Every id tensor of one batch, in a fixed order."""
    input_nodes, pair, neg, blocks = batch
    out = [input_nodes, pair.ndata[NID], pair.edata[EID], neg.ndata[NID], *pair.edges(), *neg.edges()]
    for b in blocks:
        csc = b._index.csc()
        out += [b.srcdata[NID], b.dstdata[NID], b.edata[EID], *b.edges(), csc.indptr, csc.indices]
    return out


def check_epoch(g, reverse, batches, exclude):
    leaked, seen = 0, []
    for input_nodes, pair, neg, blocks in batches:
        batch = pair.edata[EID]
        seen.append(batch)
        nodes = pair.ndata[NID]
        assert torch.equal(blocks[-1].dstdata[NID], nodes) and torch.equal(blocks[0].srcdata[NID], input_nodes)
        assert torch.equal(nodes, torch.unique(nodes)) and torch.equal(neg.ndata[NID], nodes)  # ascending, distinct
        u, v = g.find_edges(batch)
        pu, pv = pair.edges()
        assert pu.dtype == g.idtype and torch.equal(nodes[pu.long()], u.long()) and torch.equal(nodes[pv.long()], v.long())
        nu, nv = neg.edges()
        assert torch.equal(nodes[nu.long()], u.long().repeat_interleave(K))
        assert neg.number_of_nodes() == pair.number_of_nodes() == nodes.shape[0]
        assert bool(torch.isin(nodes, torch.cat([u.long(), v.long(), nodes[nv.long()]])).all())  # nothing but the endpoints
        banned = torch.cat([batch, reverse[batch]])
        for b in blocks:
            hit = int(torch.isin(b.edata[EID], banned).sum())
            leaked += hit
            if exclude == "reverse_id":
                assert hit == 0
            elif exclude == "self":
                assert int(torch.isin(b.edata[EID], batch).sum()) == 0
            # the edges are real edges of g, and the dst-sorted in-CSR the block carries is the one its COO gives
            ls, ld = b.edges()
            gs, gd = g.find_edges(b.edata[EID])
            assert torch.equal(b.srcdata[NID][ls.long()], gs.long()) and torch.equal(b.dstdata[NID][ld.long()], gd.long())
            csc = b._index.csc()
            order = torch.argsort(ld.long(), stable=True)
            indptr = torch.zeros(b.number_of_dst_nodes() + 1, dtype=torch.int64, device=ld.device)
            torch.cumsum(torch.bincount(ld.long(), minlength=b.number_of_dst_nodes()), 0, out=indptr[1:])
            assert torch.equal(csc.indptr.long(), indptr) and torch.equal(csc.indices, ls[order])
            assert csc.eids is None and torch.equal(order, torch.arange(order.shape[0], device=order.device))
            assert csc.indptr.dtype == g.idtype
    assert torch.cat(seen).unique().numel() == 100
    if exclude is None:
        assert leaked > 0, "the seed gives the exclusion test nothing to exclude"


# ---- plain-Python references
def reference_exclude(src, eid, counts, excl):
    excl = set(excl)
    out_s, out_e, out_c, at = [], [], [], 0
    for c in counts:
        kept = [(s, e) for s, e in zip(src[at:at + c], eid[at:at + c]) if e not in excl]
        out_s += [s for s, _ in kept]
        out_e += [e for _, e in kept]
        out_c.append(len(kept))
        at += c
    return out_s, out_e, out_c


def exclusion_cases(dev, idtype=torch.int64):
    """Full-neighbour frontier over the graph of test_edge_lookup (rows of 0 / 1 / 15 .. 17 / 63 .. 65 / 1000 edges: the last spans 16
    waves' worth of one seed) and the exclude lists of the issue."""
    g, _, _ = build_case(idtype, True)
    g = g.to(dev)
    seeds = torch.tensor([8, 0, 1, 5, 6, 7, 3, 100, 2, 4], device=dev)
    (src, dst, eid), counts = sampling._sample_frontier(g, seeds, None, want_counts=True)
    off = [0] + torch.cumsum(counts, 0).tolist()
    e = eid.tolist()
    row8, row6 = e[off[0]:off[1]], e[off[4]:off[5]]
    cases = {
        "every edge of the 1000-row": row8,
        "every edge of one seed and none of the others": row6,
        "empty list": [],
        "ids at both ends of the list": [min(e), max(e)],
        "every other edge": e[::2],
        "ids that are not in the frontier": [10 ** 9, -5],
        "everything": e,
    }
    return g, seeds, (src, dst, eid), counts, cases


def check_exclusion(dev):
    g, seeds, frontier, counts, cases = exclusion_cases(dev)
    src, dst, eid = frontier
    for name, excl in cases.items():
        want_s, want_e, want_c = reference_exclude(src.tolist(), eid.tolist(), counts.tolist(), excl)
        excl_t = torch.sort(torch.tensor(excl, dtype=torch.int64, device=dev))[0]
        s, d, e = sampling.exclude_frontier_edges(frontier, counts, seeds, excl_t)
        assert s.tolist() == want_s and e.tolist() == want_e, name
        assert d.tolist() == torch.repeat_interleave(seeds.cpu(), torch.tensor(want_c)).tolist(), name


def reference_compact(ids):
    nodes = sorted(set(ids))
    where = {v: i for i, v in enumerate(nodes)}
    return nodes, [where[v] for v in ids]


COMPACT_CASES = [(1, 1), (1, 7), (64, 64), (65, 300), (130, 65), (100000, 5000), (70000, 200000)]  # (num_nodes, len(ids))


def check_compact(dev, idtype):
    gen = torch.Generator().manual_seed(8)
    for num_nodes, n in COMPACT_CASES:
        ids = torch.randint(0, num_nodes, (n,), generator=gen)
        ids[0], ids[-1] = num_nodes - 1, 0
        nodes, local = linkpred.compact_nodes(num_nodes, ids.to(dev), idtype)
        want_nodes, want_local = reference_compact(ids.tolist())
        assert nodes.dtype == torch.int64 and local.dtype == idtype
        assert nodes.tolist() == want_nodes and local.tolist() == want_local
    nodes, local = linkpred.compact_nodes(10, torch.zeros(0, dtype=torch.int64, device=dev), idtype)
    assert nodes.shape == (0,) and local.shape == (0,)
    for bad in ([0, 10], [-1, 3]):
        with pytest.raises(mg.DGLError, match="outside"):
            linkpred.compact_nodes(10, torch.tensor(bad, device=dev), idtype)


def check_subgraphs(dev, idtype):
    g, _ = bidirected_graph(dev, idtype)
    n, E = g.number_of_nodes(), g.number_of_edges()
    g.ndata["x"] = torch.arange(n, device=dev).float() * 2
    g.edata["w"] = torch.arange(E, device=dev).float() + 0.5
    s, d = [t.tolist() for t in g.edges()]
    eids = [7, 3, 700, 3, 1199, 0]
    want_nodes, want_local = reference_compact([s[e] for e in eids] + [d[e] for e in eids])
    sub = g.edge_subgraph(torch.tensor(eids, device=dev))
    assert sub.ndata[NID].tolist() == want_nodes and sub.edata[EID].tolist() == eids
    u, v = sub.edges()
    assert u.dtype == idtype and u.tolist() == want_local[:6] and v.tolist() == want_local[6:]
    assert sub.ndata["x"].tolist() == [2.0 * x for x in want_nodes] and sub.edata["w"].tolist() == [e + 0.5 for e in eids]
    mask = torch.zeros(E, dtype=torch.bool, device=dev)
    mask[[5, 9]] = True
    assert g.edge_subgraph(mask).edata[EID].tolist() == [5, 9]
    keep = g.edge_subgraph(eids, preserve_nodes=True)
    assert keep.number_of_nodes() == n and keep.ndata[NID].tolist() == list(range(n))
    assert keep.edges()[0].tolist() == [s[e] for e in eids] and keep.edges()[1].tolist() == [d[e] for e in eids]
    assert torch.equal(keep.ndata["x"], g.ndata["x"]) and keep.edata[EID].tolist() == eids
    for bad in ([E], [-1]):
        with pytest.raises(mg.DGLError):
            g.edge_subgraph(bad)
    # compact_graphs: two graphs over the same nodes, with and without always_preserve
    a, b = g.edge_subgraph([1, 2, 3], preserve_nodes=True), g.edge_subgraph([900, 2], preserve_nodes=True)
    ends = [t.tolist() for x in (a, b) for t in x.edges()]
    for extra in (None, [199, 0, 199]):
        want_nodes, want_local = reference_compact(sum(ends, []) + (extra or []))
        ca, cb = dgl.compact_graphs([a, b], always_preserve=None if extra is None else torch.tensor(extra, device=dev))
        for c in (ca, cb):
            assert c.ndata[NID].tolist() == want_nodes and c.number_of_nodes() == len(want_nodes)
            assert c.ndata["x"].tolist() == [2.0 * x for x in want_nodes]
        assert ca.edges()[0].tolist() == want_local[0:3] and ca.edges()[1].tolist() == want_local[3:6]
        assert cb.edges()[0].tolist() == want_local[6:8] and cb.edges()[1].tolist() == want_local[8:10]
        assert cb.edata[EID].tolist() == [900, 2] and ca.edges()[0].dtype == idtype
    single = dgl.compact_graphs(a)
    assert isinstance(single, mg.DGLGraph) and single.ndata[NID].tolist() == reference_compact(ends[0] + ends[1])[0]
    with pytest.raises(mg.DGLError):
        dgl.compact_graphs([a, b], always_preserve=torch.tensor([n], device=dev))
    with pytest.raises(mg.DGLError, match="same"):
        dgl.compact_graphs([a, ca])


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_frontier_and_compact_reject_bad_arguments():
    """Through ctypes, no GPU needed: the argument checks come before any HIP call."""
    L = _lib.lib()
    buf = (ctypes.c_int64 * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.mgx_frontier_exclude_count(-1, p, p, 64, 0, p, p, None) == 1 and b"negative size" in L.mgx_last_error()
    assert L.mgx_frontier_exclude_count(1, p, p, 64, -1, p, p, None) == 1 and b"negative size" in L.mgx_last_error()
    assert L.mgx_frontier_exclude_count(1, p, p, 16, 0, p, p, None) == 1 and b"idx_bits must be 32 or 64, got 16" in L.mgx_last_error()
    assert L.mgx_frontier_exclude_count(1, None, p, 64, 0, p, p, None) == 1 and b"NULL pointer" in L.mgx_last_error()
    assert L.mgx_frontier_exclude_count(1, p, p, 64, 2, None, p, None) == 1 and b"excl_sorted is NULL" in L.mgx_last_error()
    assert L.mgx_frontier_exclude_count(1, p, p, 64, 0, None, None, None) == 1 and b"counts is NULL" in L.mgx_last_error()
    assert L.mgx_frontier_exclude_fill(1, p, p, 32, 0, None, None, p, p, p, None) == 1 and b"NULL pointer" in L.mgx_last_error()
    assert L.mgx_frontier_exclude_fill(1, p, p, 8, 0, None, p, p, p, p, None) == 1 and b"idx_bits" in L.mgx_last_error()
    assert L.mgx_compact_nodes_workspace(-1, 0) == -1 and L.mgx_compact_nodes_workspace(10, -1) == -1
    assert L.mgx_compact_nodes_workspace(130, 5) >= 130 * 4 + 3 * 8 + 3 * 4
    assert L.mgx_compact_nodes(-1, 0, p, 64, p, p, p, p, None) == 1 and b"negative size" in L.mgx_last_error()
    assert L.mgx_compact_nodes(4, 2, p, 16, p, p, p, p, None) == 1 and b"out_bits must be 32 or 64, got 16" in L.mgx_last_error()
    assert L.mgx_compact_nodes(4, 2 ** 31, p, 64, p, p, p, p, None) == 1 and b"below 2^31" in L.mgx_last_error()
    assert L.mgx_compact_nodes(4, 2, p, 64, p, p, p, None, None) == 1 and b"result is NULL" in L.mgx_last_error()
    assert L.mgx_compact_nodes(4, 2, p, 64, None, p, p, p, None) == 1 and b"workspace is NULL" in L.mgx_last_error()
    assert L.mgx_compact_nodes(4, 2, None, 64, p, p, p, p, None) == 1 and b"NULL pointer" in L.mgx_last_error()
    assert L.mgx_compact_nodes(4, 2, p, 64, p, None, p, p, None) == 1 and b"nodes is NULL" in L.mgx_last_error()


def test_loader_arguments():
    g, reverse = bidirected_graph("cpu")
    sampler = MultiLayerNeighborSampler([3, 3])
    with pytest.raises(mg.DGLError, match="reverse_eids"):
        EdgeDataLoader(g, torch.arange(10), sampler, exclude="reverse_id")
    with pytest.raises(mg.DGLError, match="exclude must be"):
        EdgeDataLoader(g, torch.arange(10), sampler, exclude="reverse_types")
    loader = EdgeDataLoader(g, torch.arange(10), sampler, batch_size=4, drop_last=True)
    assert len(loader) == 2
    for batch in loader:  # without a negative sampler: three items
        input_nodes, pair, blocks = batch
        assert pair.number_of_edges() == 4 and torch.equal(blocks[-1].dstdata[NID], pair.ndata[NID])
    assert torch.equal(pair.edata[EID], torch.arange(4, 8))


@pytest.mark.parametrize("exclude", [None, "self", "reverse_id"])
def test_loader_invariants_cpu(exclude, monkeypatch):
    for name in ("frontier_exclude", "compact_nodes", "negative_sample"):
        monkeypatch.setattr(sparse.HipBackend, name, lambda *a, **k: pytest.fail("the device path ran on CPU tensors"))
    g, reverse, batches = run_epoch("cpu", exclude)
    check_epoch(g, reverse, batches, exclude)


def test_exclusion_keeps_the_sampled_edges_cpu():
    """Sample first, then remove: with the same generator the excluded epoch's last block is the plain epoch's minus the banned edges.
    (The first batch only: the layer below it has other seeds, draws another amount from the generator, and the epochs part ways.)"""
    _, reverse, plain = run_epoch("cpu", None)
    _, _, excl = run_epoch("cpu", "reverse_id")
    for a, b in zip(plain[:1], excl[:1]):
        batch = a[1].edata[EID]
        assert torch.equal(batch, b[1].edata[EID])
        banned = torch.cat([batch, reverse[batch]])
        top_a, top_b = a[3][-1], b[3][-1]  # the last block's seeds are the same in both epochs
        assert torch.equal(top_a.edata[EID][~torch.isin(top_a.edata[EID], banned)], top_b.edata[EID])


def test_frontier_exclusion_cpu():
    check_exclusion("cpu")


@pytest.mark.parametrize("idtype", IDTYPES)
def test_compact_nodes_cpu(idtype):
    check_compact("cpu", idtype)


@pytest.mark.parametrize("idtype", IDTYPES)
def test_edge_subgraph_and_compact_graphs_cpu(idtype):
    check_subgraphs("cpu", idtype)


# ---------------------------------------------------------------------------------------------------------------- GPU
def spy_on(monkeypatch, name):
    calls = []
    real = getattr(sparse.HipBackend, name)

    def spy(self, *a, **k):
        calls.append(name)
        return real(self, *a, **k)
    monkeypatch.setattr(sparse.HipBackend, name, spy)
    return calls


@pytest.mark.gpu
def test_frontier_exclusion_gpu(monkeypatch):
    calls = spy_on(monkeypatch, "frontier_exclude")
    monkeypatch.setattr(config, "DEVICE_LINKPRED", True)
    check_exclusion(DEV)
    assert len(calls) == 7
    monkeypatch.setattr(config, "DEVICE_LINKPRED", False)
    check_exclusion(DEV)
    assert len(calls) == 7
    # the 32-bit instantiation, through the backend: the same frontier in int32
    g, seeds, (src, dst, eid), counts, cases = exclusion_cases(DEV)
    backend = sparse.backend_for(src)
    offsets = backend._sample_offsets(counts)
    for name, excl in cases.items():
        excl_t = torch.sort(torch.tensor(excl, dtype=torch.int64, device=DEV))[0]
        s, e, c = backend.frontier_exclude(offsets, src.int(), eid.int(), excl_t)
        want = reference_exclude(src.tolist(), eid.tolist(), counts.tolist(), excl)
        assert s.dtype == torch.int32 and (s.tolist(), e.tolist(), c.tolist()) == want, name


@pytest.mark.gpu
@pytest.mark.parametrize("idtype", IDTYPES)
def test_compact_nodes_gpu(idtype, monkeypatch):
    calls = spy_on(monkeypatch, "compact_nodes")
    monkeypatch.setattr(config, "DEVICE_LINKPRED", True)
    check_compact(DEV, idtype)
    assert len(calls) == len(COMPACT_CASES) + 3
    monkeypatch.setattr(config, "DEVICE_LINKPRED", False)
    check_compact(DEV, idtype)
    assert len(calls) == len(COMPACT_CASES) + 3


@pytest.mark.gpu
@pytest.mark.parametrize("idtype", IDTYPES)
def test_edge_subgraph_and_compact_graphs_gpu(idtype, monkeypatch):
    for flag in (True, False):
        monkeypatch.setattr(config, "DEVICE_LINKPRED", flag)
        check_subgraphs(DEV, idtype)


@pytest.mark.gpu
@pytest.mark.parametrize("idtype", IDTYPES)
@pytest.mark.parametrize("exclude", [None, "reverse_id"])
def test_loader_epoch_on_equals_off_gpu(exclude, idtype, monkeypatch):
    compact_calls, neg_calls = spy_on(monkeypatch, "compact_nodes"), spy_on(monkeypatch, "negative_sample")
    excl_calls = spy_on(monkeypatch, "frontier_exclude")
    monkeypatch.setattr(config, "DEVICE_LINKPRED", True)
    g, reverse, on = run_epoch(DEV, exclude, idtype)
    check_epoch(g, reverse, on, exclude)
    assert len(excl_calls) == (8 if exclude else 0), "two layers, four batches"
    assert len(compact_calls) == 4 and len(neg_calls) == 4
    monkeypatch.setattr(config, "DEVICE_LINKPRED", False)
    _, _, off = run_epoch(DEV, exclude, idtype)
    assert len(excl_calls) == (8 if exclude else 0) and len(compact_calls) == 4 and len(neg_calls) == 4
    assert len(on) == len(off) == 4
    for a, b in zip(on, off):
        ta, tb = batch_tensors(a), batch_tensors(b)
        assert len(ta) == len(tb) and all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(ta, tb))
    if idtype == torch.int64:
        # and the first batch equals the CPU epoch's: the negatives' stream does not depend on the device (later batches differ: the
        # CPU sampler draws another amount from the generator)
        _, _, cpu = run_epoch("cpu", exclude, idtype)
        for a, c in zip(on[:1], cpu[:1]):
            assert torch.equal(a[1].edata[EID].cpu(), c[1].edata[EID]) and torch.equal(a[2].edges()[1].cpu(), c[2].edges()[1])


@pytest.mark.gpu
def test_linkpred_model_trains_gpu():
    """20 steps of the sampling_linkpred.py model: a finite loss, and a gradient that is not zero on every parameter."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dgl-0.5-benchmark_amd"))
    import sampling_linkpred as slp
    import torch.nn.functional as F
    torch.manual_seed(0)
    g, reverse = bidirected_graph(DEV, torch.int32)
    feats = torch.randn(g.number_of_nodes(), 24, device=DEV)
    gen = torch.Generator().manual_seed(2)
    loader = slp.make_loader(g, torch.arange(g.number_of_edges() // 2), reverse.to(DEV), [3, 3], 32, K, exclude="reverse_id",
                             exclude_existing=True, generator=gen)
    model = slp.SAGE(24, 16, 16, 2, F.relu, 0.0).to(DEV)
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    steps = 0
    while steps < 20:  # an epoch has 19 batches
        for batch in loader:
            loss = slp.train_step(model, opt, feats, batch)
            assert bool(torch.isfinite(loss))
            for name, prm in model.named_parameters():
                assert prm.grad is not None and bool(torch.isfinite(prm.grad).all()) and float(prm.grad.abs().sum()) > 0, name
            steps += 1
            if steps == 20:
                break
