"""Edge lookup (csrc/edgefind.hip: mgx_edge_lookup) behind g.edge_ids / g.has_edges_between, against a dict built in Python.

The kernel gives every query a group of 16 lanes (kFindLanes of csrc/edge_find.h) that strides one row of the in-CSR, so the graph has
in-rows of length 0, 1, 15 / 16 / 17 (one below, at and above the group width), 63 / 64 / 65 (the wavefront) and one of 1000; multi-edges,
self loops, and -- in the `shuffled` variant -- edge ids assigned to the CSR positions by a random permutation, so that the lowest id of
a multi-edge is NOT the first match in its row: the kernel has to take a minimum, not the first hit.  The `positional` variant has no
edge-id array at all (eids NULL: the edge id is the CSR position), what a graph renumbered in in-CSR order looks like.
"""
import ctypes

import pytest
import torch

import mi355x_graph as mg
from mi355x_graph import _lib, config, linkpred, sparse

NAMES = ["mgx_edge_lookup", "mgx_negative_sample", "mgx_frontier_exclude_count", "mgx_frontier_exclude_fill",
         "mgx_compact_nodes_workspace", "mgx_compact_nodes"]
DEV = "cuda:0"
IDTYPES = [torch.int32, torch.int64]
N = 300
ROW_LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 1000]  # rows 0 .. 8; the other rows get 0 .. 6 edges


def build_case(idtype, shuffled):
    """(graph, {(u, v): lowest edge id}, multi-edge pairs).  The graph is built straight from its in-CSR."""
    gen = torch.Generator().manual_seed(5)
    deg = torch.randint(0, 7, (N,), generator=gen)
    deg[:len(ROW_LENGTHS)] = torch.tensor(ROW_LENGTHS)
    indptr = torch.zeros(N + 1, dtype=torch.int64)
    torch.cumsum(deg, 0, out=indptr[1:])
    E = int(indptr[-1])
    indices = torch.randint(0, N, (E,), generator=gen)
    for v in range(N):  # self loops on every seventh node that has an in-edge, and a triple edge in the rows that have room
        b, e = int(indptr[v]), int(indptr[v + 1])
        if v % 7 == 0 and e > b:
            indices[b] = v
        if e - b >= 4:
            indices[e - 1] = indices[e - 3] = indices[b + 1]
    eids = torch.randperm(E, generator=gen) if shuffled else None
    table, seen = {}, {}
    rows = torch.repeat_interleave(torch.arange(N), deg).tolist()
    for p, (u, v) in enumerate(zip(indices.tolist(), rows)):
        e = int(eids[p]) if shuffled else p
        seen[(u, v)] = seen.get((u, v), 0) + 1
        table[(u, v)] = min(table.get((u, v), e), e)
    multi = [k for k, c in seen.items() if c > 1]
    csc = sparse.CsrView(N, N, indptr.to(idtype), indices.to(idtype), None if eids is None else eids.to(idtype))
    if shuffled:  # the case has teeth: some multi-edge's lowest id is not at its first position in the row
        first_hit = {}
        for p, (u, v) in enumerate(zip(indices.tolist(), rows)):
            first_hit.setdefault((u, v), int(eids[p]))
        assert any(first_hit[k] != table[k] for k in multi)
    return mg.DGLGraph(mg.GraphIndex(N, N, csc=csc)), table, multi


def queries(table, multi):
    gen = torch.Generator().manual_seed(6)
    present = list(table)
    absent = []
    while len(absent) < 500:
        u, v = torch.randint(0, N, (2,), generator=gen).tolist()
        if (u, v) not in table:
            absent.append((u, v))
    q = present + multi + absent + present[:40] + absent[:40]  # the tail: duplicate queries
    perm = torch.randperm(len(q), generator=gen).tolist()
    return [q[i] for i in perm]


def check_lookup(g, table, multi):
    q = queries(table, multi)
    u, v = torch.tensor([a for a, _ in q], device=g.device), torch.tensor([b for _, b in q], device=g.device)
    want = [table.get(p, -1) for p in q]
    assert linkpred.edge_lookup(g, u, v).tolist() == want
    assert g.has_edges_between(u, v).tolist() == [w >= 0 for w in want]
    assert g.has_edges_between(u, v).dtype == torch.bool
    hit = [i for i, w in enumerate(want) if w >= 0]
    got = g.edge_ids(u[hit], v[hit])
    assert got.dtype == g.idtype and got.tolist() == [want[i] for i in hit]
    empty = torch.zeros(0, dtype=torch.int64, device=g.device)
    assert g.edge_ids(empty, empty).shape == (0,) and g.has_edges_between(empty, empty).shape == (0,)
    miss = next(i for i, w in enumerate(want) if w < 0)
    with pytest.raises(mg.DGLError, match="no edge between %d and %d" % q[miss]):
        g.edge_ids(u[[hit[0], miss]], v[[hit[0], miss]])
    with pytest.raises(mg.DGLError, match="not supported"):
        g.edge_ids(u[:1], v[:1], return_uv=True)
    for bad_u, bad_v in [([N], [0]), ([0], [N]), ([-1], [0]), ([0], [-1])]:
        with pytest.raises(mg.DGLError, match="out of range"):
            g.edge_ids(bad_u, bad_v)
        with pytest.raises(mg.DGLError, match="out of range"):
            g.has_edges_between(bad_u, bad_v)


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_entry_points_declared_and_exported():
    header = open(_lib.HEADER_PATH).read()
    L = _lib.lib()
    for name in NAMES:
        assert name + "(" in header
        assert name in _lib.SIGNATURES
        assert getattr(L, name) is not None
    assert L.mgx_abi_version() == 35
    assert isinstance(config.DEVICE_LINKPRED, bool)


def test_edge_lookup_rejects_bad_arguments():
    """Through ctypes, no GPU needed: the argument checks come before any HIP call."""
    L = _lib.lib()
    buf = (ctypes.c_int64 * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = _lib.MgxCsr(4, 4, 2, p, p, None, 64, 0)
    assert L.mgx_edge_lookup(None, 1, p, p, p, p, None) == 1
    assert b"csr is NULL" in L.mgx_last_error()
    assert L.mgx_edge_lookup(ctypes.byref(ok), -1, p, p, p, p, None) == 1
    assert b"negative num_q" in L.mgx_last_error()
    assert L.mgx_edge_lookup(ctypes.byref(_lib.MgxCsr(4, 4, 2, p, p, None, 16, 0)), 1, p, p, p, p, None) == 1
    assert b"idx_bits must be 32 or 64" in L.mgx_last_error()
    assert L.mgx_edge_lookup(ctypes.byref(_lib.MgxCsr(-4, 4, 2, p, p, None, 64, 0)), 1, p, p, p, p, None) == 1
    assert b"negative size" in L.mgx_last_error()
    assert L.mgx_edge_lookup(ctypes.byref(_lib.MgxCsr(4, 4, 2, None, p, None, 64, 0)), 1, p, p, p, p, None) == 1
    assert b"indptr is NULL" in L.mgx_last_error()
    assert L.mgx_edge_lookup(ctypes.byref(_lib.MgxCsr(4, 4, 2, p, None, None, 64, 0)), 1, p, p, p, p, None) == 1
    assert b"indices is NULL" in L.mgx_last_error()
    assert L.mgx_edge_lookup(ctypes.byref(ok), 1, p, p, p, None, None) == 1
    assert b"result is NULL" in L.mgx_last_error()
    for args in [(None, p, p), (p, None, p), (p, p, None)]:
        assert L.mgx_edge_lookup(ctypes.byref(ok), 1, args[0], args[1], args[2], p, None) == 1
        assert b"NULL pointer" in L.mgx_last_error()


@pytest.mark.parametrize("shuffled", [True, False], ids=["shuffled", "positional"])
@pytest.mark.parametrize("idtype", IDTYPES)
def test_edge_ids_cpu(idtype, shuffled, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the device path ran on CPU tensors")
    monkeypatch.setattr(sparse.HipBackend, "edge_lookup", boom)
    g, table, multi = build_case(idtype, shuffled)
    for flag in (True, False):
        monkeypatch.setattr(config, "DEVICE_LINKPRED", flag)
        check_lookup(g, table, multi)


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("shuffled", [True, False], ids=["shuffled", "positional"])
@pytest.mark.parametrize("idtype", IDTYPES)
def test_edge_ids_gpu(idtype, shuffled, monkeypatch):
    g, table, multi = build_case(idtype, shuffled)
    g = g.to(DEV)
    assert (g._index.csc().eids is None) == (not shuffled)
    calls = []
    real = sparse.HipBackend.edge_lookup

    def spy(self, *a, **k):
        calls.append(1)
        return real(self, *a, **k)
    monkeypatch.setattr(sparse.HipBackend, "edge_lookup", spy)
    monkeypatch.setattr(config, "DEVICE_LINKPRED", True)
    check_lookup(g, table, multi)
    assert calls, "the kernel did not run"
    n_on = len(calls)
    q = queries(table, multi)
    u, v = torch.tensor([a for a, _ in q], device=DEV), torch.tensor([b for _, b in q], device=DEV)
    on = (g.has_edges_between(u, v), linkpred.edge_lookup(g, u, v))
    n_on2 = len(calls)
    assert n_on2 == n_on + 2
    monkeypatch.setattr(config, "DEVICE_LINKPRED", False)
    off = (g.has_edges_between(u, v), linkpred.edge_lookup(g, u, v))
    assert len(calls) == n_on2, "the composition must not call the kernel"
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])
    check_lookup(g, table, multi)  # the composition on device tensors


@pytest.mark.gpu
def test_lookup_over_the_out_csr_gpu():
    """The same entry point over the out-CSR, ids passed in the matching order (rows = sources)."""
    g, table, multi = build_case(torch.int64, True)
    g = g.to(DEV)
    q = queries(table, multi)
    u, v = torch.tensor([a for a, _ in q], device=DEV), torch.tensor([b for _, b in q], device=DEV)
    eid, result = sparse.backend_for(u).edge_lookup(g._index.csr(), u, v)
    assert int(result[0]) == 0 and eid.tolist() == [table.get(p, -1) for p in q]
