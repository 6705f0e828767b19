"""to_block on the device (csrc/relabel.hip: mgx_to_block) against the torch composition it stands for.

The two forms must give the SAME block, bit for bit: the same source list (destinations first, then the other sources by ascending global
id), the same local COO in the graph's id type, the same dst-sorted in-CSR.  Every GPU case builds the block twice -- config.DEVICE_BLOCKS
on, then off -- and compares with torch.equal; a spy on HipBackend.to_block makes sure the first one did run the kernels.
"""
import ctypes

import pytest
import torch

import mi355x_graph as mg
from mi355x_graph import _lib, config, sampling, sparse
from mi355x_graph.sampling import NID, EID

from test_sampling import make_graph

NAMES = ["mgx_to_block_workspace", "mgx_to_block", "mgx_node_subgraph_workspace", "mgx_node_subgraph_count", "mgx_node_subgraph_fill"]
DEV = "cuda:0"
IDTYPES = [torch.int32, torch.int64]


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_entry_points_declared_and_exported():
    header = open(_lib.HEADER_PATH).read()
    L = _lib.lib()
    for name in NAMES:
        assert name + "(" in header
        assert name in _lib.SIGNATURES
        assert getattr(L, name) is not None
    assert L.mgx_abi_version() == 35


def test_config_switches_exist():
    assert isinstance(config.DEVICE_BLOCKS, bool) and isinstance(config.DEVICE_SUBGRAPH, bool)


def test_to_block_rejects_bad_arguments():
    """Through ctypes, no GPU needed: the argument checks come before any HIP call."""
    L = _lib.lib()
    buf = (ctypes.c_int64 * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.mgx_to_block_workspace(-1, 0) == -1 and L.mgx_to_block_workspace(10, -1) == -1
    assert L.mgx_to_block_workspace(130, 5) >= 130 * 4 + 3 * 8 + 3 * 4
    assert L.mgx_to_block(-1, 0, None, 0, None, None, 0, 64, p, p, p, p, p, p, None) == 1
    assert b"negative size" in L.mgx_last_error()
    assert L.mgx_to_block(4, 0, None, -2, None, None, 0, 64, p, p, p, p, p, p, None) == 1
    assert b"negative size" in L.mgx_last_error()
    assert L.mgx_to_block(4, 1, p, 1, p, p, 0, 16, p, p, p, p, p, p, None) == 1
    assert b"out_bits must be 32 or 64, got 16" in L.mgx_last_error()
    assert L.mgx_to_block(4, 2 ** 30, p, 2 ** 30, p, p, 0, 64, p, p, p, p, p, p, None) == 1
    assert b"below 2^31" in L.mgx_last_error()
    assert L.mgx_to_block(4, 1, p, 1, p, p, 0, 64, p, p, p, p, p, None, None) == 1
    assert b"result is NULL" in L.mgx_last_error()
    assert L.mgx_to_block(4, 1, p, 1, p, p, 0, 64, None, p, p, p, p, p, None) == 1
    assert b"workspace is NULL" in L.mgx_last_error()
    assert L.mgx_to_block(4, 1, None, 1, p, p, 0, 64, p, p, p, p, p, p, None) == 1
    assert b"NULL pointer" in L.mgx_last_error()
    assert L.mgx_to_block(4, 1, p, 1, p, None, 0, 64, p, p, p, p, p, p, None) == 1
    assert b"NULL pointer" in L.mgx_last_error()
    assert L.mgx_to_block(4, 1, p, 1, p, p, 1, 64, p, p, p, p, None, p, None) == 1
    assert b"indptr is NULL with dst_sorted" in L.mgx_last_error()


def reference_block(num_nodes, dst_nodes, src, dst):
    """The block's tables in plain Python: (src_nodes, l_src, l_dst, indptr of the dst-sorted in-CSR)."""
    dst_nodes, src, dst = dst_nodes.tolist(), src.tolist(), dst.tolist()
    local = {v: i for i, v in enumerate(dst_nodes)}
    for v in sorted(set(src) - set(dst_nodes)):
        local[v] = len(local)
    src_nodes = sorted(local, key=local.get)
    l_dst = [local[v] for v in dst]
    indptr = [0] * (len(dst_nodes) + 1)
    for x in l_dst:
        indptr[x + 1] += 1
    for k in range(len(dst_nodes)):
        indptr[k + 1] += indptr[k]
    return src_nodes, [local[v] for v in src], l_dst, indptr


def make_case(num_nodes, seed, sorted_edges=True, max_deg=4):
    """dst_nodes: about half of the nodes in random order, never node 0 or the last node once there are three; edges grouped by
    destination (0 .. max_deg per row, so empty rows occur), sources drawn from all nodes, node 0 and the last node among them."""
    gen = torch.Generator().manual_seed(seed)
    if num_nodes >= 3:
        pool = torch.randperm(num_nodes - 2, generator=gen) + 1
        dst_nodes = pool[:max(1, (num_nodes - 2) // 2)]
    else:
        dst_nodes = torch.randperm(num_nodes, generator=gen)
    deg = torch.randint(0, max_deg + 1, (dst_nodes.shape[0],), generator=gen)
    deg[0] = max(int(deg[0]), 2)
    dst = torch.repeat_interleave(dst_nodes, deg)
    src = torch.randint(0, num_nodes, (dst.shape[0],), generator=gen)
    src[0], src[1] = 0, num_nodes - 1
    if not sorted_edges:
        perm = torch.randperm(dst.shape[0], generator=gen)
        src, dst = src[perm], dst[perm]
    return dst_nodes, src, dst, torch.arange(dst.shape[0]) * 3 + 1


@pytest.mark.parametrize("idtype", IDTYPES)
def test_cpu_tensors_take_the_torch_form(idtype, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the device path ran on CPU tensors")
    monkeypatch.setattr(sparse.HipBackend, "to_block", boom)
    for n in (1, 65, 130):
        dst_nodes, src, dst, eid = make_case(n, seed=n)
        for flag in (True, False):
            monkeypatch.setattr(config, "DEVICE_BLOCKS", flag)
            b = sampling.to_block((src, dst, eid), dst_nodes, num_nodes=n, idtype=idtype, dst_sorted=True, max_in_degree=4)
            ref = reference_block(n, dst_nodes, src, dst)
            assert b.srcdata[NID].tolist() == ref[0] and b.srcdata[NID].dtype == torch.int64
            assert torch.equal(b.dstdata[NID], dst_nodes) and torch.equal(b.edata[EID], eid)
            u, v = b.edges()
            assert u.dtype == idtype and u.tolist() == ref[1] and v.tolist() == ref[2]
            csc = b._index.csc()
            assert csc.indptr.tolist() == ref[3] and csc.indices.tolist() == ref[1] and csc.eids is None


# ---------------------------------------------------------------------------------------------------------------- GPU
class Spy(object):
    """Counts the calls of HipBackend.to_block that go through."""

    def __init__(self, monkeypatch):
        self.calls = 0
        inner = sparse.HipBackend.to_block

        def to_block(backend, *a, **k):
            self.calls += 1
            return inner(backend, *a, **k)
        monkeypatch.setattr(sparse.HipBackend, "to_block", to_block)


def same_block(a, b, dst_sorted):
    assert a.number_of_src_nodes() == b.number_of_src_nodes() and a.number_of_dst_nodes() == b.number_of_dst_nodes()
    for x, y in ((a.srcdata[NID], b.srcdata[NID]), (a.dstdata[NID], b.dstdata[NID]), (a.edges()[0], b.edges()[0]),
                 (a.edges()[1], b.edges()[1])):
        assert x.dtype == y.dtype and x.device == y.device and torch.equal(x, y)
    assert (EID in a.edata) == (EID in b.edata)
    if EID in a.edata:
        assert torch.equal(a.edata[EID], b.edata[EID])
    ia, ib = a._index, b._index
    assert (ia.dst_is_src_prefix, ia.max_in_degree_hint, ia.ephemeral) == (ib.dst_is_src_prefix, ib.max_in_degree_hint, ib.ephemeral)
    assert (ia._csc is None) == (ib._csc is None) == (not dst_sorted)
    if dst_sorted:
        ca, cb = ia._csc, ib._csc
        assert ca.indptr.dtype == cb.indptr.dtype and torch.equal(ca.indptr, cb.indptr)
        assert ca.indices.dtype == cb.indices.dtype and torch.equal(ca.indices, cb.indices)
        assert ca.eids is None and cb.eids is None
        assert (ca.num_rows, ca.num_cols, ca.dst_is_src_prefix, ca.short_hint) == (cb.num_rows, cb.num_cols, cb.dst_is_src_prefix, cb.short_hint)
        assert (ca._plan is None) == (cb._plan is None)


def both_forms(monkeypatch, edges, dst_nodes, spy=None, **kw):
    """The block by the kernels and by the torch composition, compared; returns the first."""
    spy = spy or Spy(monkeypatch)
    before = spy.calls
    edges = tuple(t.to(DEV) for t in edges)
    dst_nodes = dst_nodes.to(DEV)
    monkeypatch.setattr(config, "DEVICE_BLOCKS", True)
    a = sampling.to_block(edges, dst_nodes, **kw)
    assert spy.calls == before + 1
    monkeypatch.setattr(config, "DEVICE_BLOCKS", False)
    b = sampling.to_block(edges, dst_nodes, **kw)
    assert spy.calls == before + 1
    same_block(a, b, kw.get("dst_sorted", False))
    return a


@pytest.mark.gpu
@pytest.mark.parametrize("idtype", IDTYPES)
@pytest.mark.parametrize("num_nodes", [1, 63, 64, 65, 130, 3000])
def test_sizes_around_the_bitmap_words(num_nodes, idtype, monkeypatch):
    spy = Spy(monkeypatch)
    dst_nodes, src, dst, eid = make_case(num_nodes, seed=num_nodes)
    a = both_forms(monkeypatch, (src, dst, eid), dst_nodes, spy, num_nodes=num_nodes, idtype=idtype, dst_sorted=True, max_in_degree=4)
    ref = reference_block(num_nodes, dst_nodes, src, dst)
    assert a.srcdata[NID].tolist() == ref[0] and a._index._csc.indptr.tolist() == ref[3]
    if num_nodes >= 3:  # node 0 and the last node are sources and no destinations: the first and the last of the other sources
        assert a.srcdata[NID][dst_nodes.shape[0]].item() == 0 and a.srcdata[NID][-1].item() == num_nodes - 1
    both_forms(monkeypatch, (src, dst), dst_nodes, spy, num_nodes=num_nodes, idtype=idtype)
    dst_nodes, src, dst, eid = make_case(num_nodes, seed=num_nodes + 1, sorted_edges=False)
    both_forms(monkeypatch, (src, dst, eid), dst_nodes, spy, num_nodes=num_nodes, idtype=idtype, dst_sorted=False)
    both_forms(monkeypatch, (src, dst, eid), dst_nodes, spy, num_nodes=None, idtype=idtype)  # the max().item() fallback


@pytest.mark.gpu
@pytest.mark.parametrize("idtype", IDTYPES)
def test_scan_over_more_than_three_rounds_of_words(idtype, monkeypatch):
    """The word scan is one workgroup of 1024 threads: 200 000 nodes are 3 125 words, four rounds, the last one partial."""
    n = 200_000
    gen = torch.Generator().manual_seed(5)
    dst_nodes = torch.randperm(n - 2, generator=gen)[:700] + 1
    dst = torch.repeat_interleave(dst_nodes, 6)
    src = torch.randint(0, n, (dst.shape[0],), generator=gen)
    src[:4] = torch.tensor([0, n - 1, 65_536, 131_071])
    a = both_forms(monkeypatch, (src, dst), dst_nodes, num_nodes=n, idtype=idtype, dst_sorted=True, max_in_degree=6)
    other = a.srcdata[NID][700:]
    assert bool((other[1:] > other[:-1]).all()) and other[0].item() == 0 and other[-1].item() == n - 1


@pytest.mark.gpu
@pytest.mark.parametrize("idtype", IDTYPES)
def test_degenerate_blocks(idtype, monkeypatch):
    spy = Spy(monkeypatch)
    z = torch.zeros(0, dtype=torch.int64)
    kw = dict(num_nodes=130, idtype=idtype)
    both_forms(monkeypatch, (z, z), torch.tensor([5, 129, 0]), spy, dst_sorted=True, max_in_degree=3, **kw)  # no edge: all rows empty
    both_forms(monkeypatch, (z, z), torch.tensor([5, 129, 0]), spy, **kw)
    both_forms(monkeypatch, (z, z, z), z, spy, dst_sorted=True, **kw)  # no destination, no edge
    both_forms(monkeypatch, (z, z), z, spy, num_nodes=1, idtype=idtype, dst_sorted=True)
    dst_nodes = torch.tensor([64, 3, 127, 63, 128])
    dst = torch.tensor([64, 64, 3, 127, 127, 127, 128])
    inside = torch.tensor([3, 128, 64, 64, 63, 127, 3])  # every source is a destination
    a = both_forms(monkeypatch, (inside, dst), dst_nodes, spy, dst_sorted=True, max_in_degree=3, **kw)
    assert a.number_of_src_nodes() == 5
    outside = torch.tensor([129, 0, 1, 62, 65, 126, 2])  # no source is one
    a = both_forms(monkeypatch, (outside, dst), dst_nodes, spy, dst_sorted=True, max_in_degree=3, **kw)
    assert a.srcdata[NID].tolist() == [64, 3, 127, 63, 128, 0, 1, 2, 62, 65, 126, 129]
    for node in (129, 64):  # one source repeated by every edge: not a destination, a destination
        many = torch.repeat_interleave(dst_nodes, 300)
        a = both_forms(monkeypatch, (torch.full_like(many, node), many), dst_nodes, spy, dst_sorted=True, max_in_degree=300, **kw)
        assert a.number_of_src_nodes() == (6 if node == 129 else 5) and a._index._csc._plan is False


@pytest.mark.gpu
@pytest.mark.parametrize("idtype", IDTYPES)
def test_empty_rows_first_middle_last(idtype, monkeypatch):
    spy = Spy(monkeypatch)
    dst_nodes = torch.tensor([9, 8, 100, 7, 6, 5, 64, 4, 3])
    for rows in ([2, 2, 5, 5, 5, 6], [0, 8], [4], [8, 8], [0, 1, 2, 3, 4, 5, 6, 7, 8], [3, 3, 3, 7]):
        dst = dst_nodes[torch.tensor(rows)]
        src = torch.arange(dst.shape[0]) * 17 % 129
        a = both_forms(monkeypatch, (src, dst), dst_nodes, spy, num_nodes=129, idtype=idtype, dst_sorted=True, max_in_degree=9)
        assert a._index._csc.indptr.tolist() == [sum(1 for r in rows if r < k) for k in range(10)]


@pytest.mark.gpu
@pytest.mark.parametrize("idtype", IDTYPES)
@pytest.mark.parametrize("fanout", [5, 64])
def test_real_sampler_output(fanout, idtype, monkeypatch):
    g, s, d = make_graph(n=3000, m=40000, device=DEV)
    seeds = torch.randperm(3000, generator=torch.Generator().manual_seed(1))[:500]
    frontier = sampling.sample_neighbors(g, seeds.to(DEV), fanout, generator=torch.Generator().manual_seed(2))
    spy = Spy(monkeypatch)
    a = both_forms(monkeypatch, frontier, seeds, spy, num_nodes=3000, idtype=idtype, dst_sorted=True, max_in_degree=fanout)
    assert torch.equal(a.srcdata[NID][a.edges()[0].long()], frontier[0]) and torch.equal(a.dstdata[NID][a.edges()[1].long()], frontier[1])
    perm = torch.randperm(frontier[0].shape[0], generator=torch.Generator().manual_seed(3)).to(DEV)
    both_forms(monkeypatch, tuple(t[perm] for t in frontier), seeds, spy, num_nodes=3000, idtype=idtype, dst_sorted=False)


@pytest.mark.gpu
def test_each_error_bit_raises_and_the_device_goes_on(monkeypatch):
    monkeypatch.setattr(config, "DEVICE_BLOCKS", True)
    n = 130
    dst_nodes, src, dst, eid = (t.to(DEV) for t in make_case(n, seed=9))
    good = reference_block(n, dst_nodes.cpu(), src.cpu(), dst.cpu())

    def put(t, i, v):
        t = t.clone()
        t[i] = v
        return t

    def check_good():
        b = sampling.to_block((src, dst, eid), dst_nodes, num_nodes=n, idtype=torch.int32, dst_sorted=True, max_in_degree=4)
        assert b.srcdata[NID].tolist() == good[0] and b.edges()[0].tolist() == good[1] and b.edges()[1].tolist() == good[2]
        assert b._index._csc.indptr.tolist() == good[3]

    check_good()
    bad_calls = [
        ("outside", (put(src, 3, n), dst), dst_nodes, True),
        ("outside", (put(src, 0, -1), dst), dst_nodes, True),
        ("outside", (src, put(dst, 5, n)), dst_nodes, False),
        ("outside", (src, put(dst, 5, -1)), dst_nodes, True),
        ("outside", (src, dst), put(dst_nodes, 2, -1), True),
        ("outside", (src, dst), put(dst_nodes, dst_nodes.shape[0] - 1, n), False),
        ("more than once", (src, dst), torch.cat([dst_nodes, dst_nodes[4:5]]), False),
        ("every edge destination must be one of dst_nodes", (src, put(dst, 1, 0)), dst_nodes, True),
        ("every edge destination must be one of dst_nodes", (put(src, 1, 129), put(dst, 1, 129)), dst_nodes, True),
        ("not grouped by destination", (src, torch.flip(dst, [0])), dst_nodes, True),  # rows in dst_nodes order, edges in the opposite one
    ]
    for text, edges, nodes, dst_sorted in bad_calls:
        for idtype in IDTYPES:
            with pytest.raises(mg.DGLError, match=text):
                sampling.to_block(edges, nodes, num_nodes=n, idtype=idtype, dst_sorted=dst_sorted)
        check_good()


@pytest.mark.gpu
@pytest.mark.parametrize("idtype", IDTYPES)
def test_sample_blocks_identical_in_both_forms(idtype, monkeypatch):
    g, s, d = make_graph(n=3000, m=40000, device=DEV)
    g = g.int() if idtype == torch.int32 else g.long()
    sampler = sampling.MultiLayerNeighborSampler([5, 10])
    seeds = torch.arange(100, 400)
    spy = Spy(monkeypatch)
    monkeypatch.setattr(config, "DEVICE_BLOCKS", True)
    a = sampler.sample_blocks(g, seeds, generator=torch.Generator().manual_seed(4))
    assert spy.calls == 2
    monkeypatch.setattr(config, "DEVICE_BLOCKS", False)
    b = sampler.sample_blocks(g, seeds, generator=torch.Generator().manual_seed(4))
    assert spy.calls == 2 and len(a) == len(b) == 2
    for x, y in zip(a, b):
        assert x.idtype == idtype
        same_block(x, y, True)
