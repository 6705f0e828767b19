"""g.subgraph(nodes) on the device (csrc/relabel.hip: mgx_node_subgraph_count / _fill) against the torch composition it stands for.

With the parent's in-CSR materialised the kernels read the rows of the selected nodes only; the subgraph must come out exactly as the
composition gives it -- edges by ascending parent edge id, features sliced -- and carries its own in-CSR, equal to the one a GraphIndex
would build from its COO.
"""
import ctypes

import pytest
import torch

import mi355x_graph as mg
from mi355x_graph import _lib, config, sparse
from mi355x_graph.graph import DGLGraph, GraphIndex
from mi355x_graph.sampling import NID, EID

DEV = "cuda:0"
N = 300
HUB = 7  # a row of 250 in-edges: four wave-widths, the last one partial


def edge_lists():
    """Random edges among nodes 0 .. 289, a hub row, self loops; nodes 290 .. 299 touch only nodes below 290."""
    gen = torch.Generator().manual_seed(3)
    src = [torch.randint(0, 290, (1500,), generator=gen), torch.randint(0, 290, (250,), generator=gen), torch.tensor([5, 7, 288]),
           torch.arange(290, 300), torch.randint(0, 290, (10,), generator=gen)]
    dst = [torch.randint(0, 290, (1500,), generator=gen), torch.full((250,), HUB), torch.tensor([5, 7, 288]),
           torch.randint(0, 290, (10,), generator=gen), torch.arange(290, 300)]
    src, dst = torch.cat(src), torch.cat(dst)
    perm = torch.randperm(src.shape[0], generator=gen)
    return src[perm], dst[perm]


def parent(device, idtype, presorted, with_csc=True):
    """presorted: the edges arrive sorted by destination and the in-CSR has no edge-id array (positions are edge ids)."""
    src, dst = edge_lists()
    n_e = src.shape[0]
    if presorted:
        order = torch.sort(dst, stable=True)[1]
        src, dst = src[order], dst[order]
        indptr = torch.zeros(N + 1, dtype=torch.int64)
        torch.cumsum(torch.bincount(dst, minlength=N), 0, out=indptr[1:])
        s, d = src.to(device=device, dtype=idtype), dst.to(device=device, dtype=idtype)
        csc = sparse.CsrView(N, N, indptr.to(device=device, dtype=idtype), s, None) if with_csc else None
        g = DGLGraph(GraphIndex(N, N, coo=(s, d), csc=csc))
    else:
        g = mg.graph((src, dst), num_nodes=N).to(device)
        g = g.int() if idtype == torch.int32 else g.long()
        if with_csc:
            assert g._index.csc().eids is not None
    g.ndata["x"] = (torch.arange(N * 3, dtype=torch.float32).reshape(N, 3) * 0.5).to(device)
    g.edata["w"] = (torch.arange(n_e, dtype=torch.float32) + 0.25).to(device)
    return g


def selections(device):
    mask = torch.zeros(N, dtype=torch.bool)
    mask[torch.randperm(N, generator=torch.Generator().manual_seed(8))[:120]] = True
    mask[HUB] = True
    return {
        "none": torch.zeros(0, dtype=torch.int64),
        "all": torch.arange(N),
        "self loop": torch.tensor([5]),
        "every second, descending": torch.arange(N - 1, -1, -2),
        "mask": mask.to(device),
        "dict": {"_N": torch.randperm(N, generator=torch.Generator().manual_seed(9))[:200].to(device)},
        "rows keep no edge": torch.tensor([291, 295, 299]),
        "int32 ids": torch.tensor([HUB, 3, 250, 11], dtype=torch.int32),
    }


def same_subgraph(a, b):
    assert a.number_of_nodes() == b.number_of_nodes() and a.number_of_edges() == b.number_of_edges()
    pairs = [(a.edges()[0], b.edges()[0]), (a.edges()[1], b.edges()[1]), (a.ndata[NID], b.ndata[NID]), (a.edata[EID], b.edata[EID]),
             (a.ndata["x"], b.ndata["x"]), (a.edata["w"], b.edata["w"])]
    for x, y in pairs:
        assert x.dtype == y.dtype and x.device == y.device and torch.equal(x, y)
    assert a._index.ephemeral and b._index.ephemeral


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_subgraph_entry_points_reject_bad_arguments():
    """Through ctypes, no GPU needed: the argument checks come before any HIP call."""
    L = _lib.lib()
    buf = (ctypes.c_int64 * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.mgx_node_subgraph_workspace(-1) == -1 and L.mgx_node_subgraph_workspace(300) >= 1200
    ok = _lib.MgxCsr(4, 4, 0, p, None, None, 32, 0)
    assert L.mgx_node_subgraph_count(None, 1, p, p, p, p, None) == 1
    assert b"mgx_node_subgraph_count: csr is NULL" in L.mgx_last_error()
    assert L.mgx_node_subgraph_fill(None, 1, p, p, p, 32, p, p, p, None) == 1
    assert b"mgx_node_subgraph_fill: csr is NULL" in L.mgx_last_error()
    assert L.mgx_node_subgraph_count(ctypes.byref(_lib.MgxCsr(4, 4, 0, p, None, None, 16, 0)), 1, p, p, p, p, None) == 1
    assert b"idx_bits must be 32 or 64" in L.mgx_last_error()
    assert L.mgx_node_subgraph_count(ctypes.byref(_lib.MgxCsr(4, 5, 0, p, None, None, 32, 0)), 1, p, p, p, p, None) == 1
    assert b"num_rows == num_cols" in L.mgx_last_error()
    assert L.mgx_node_subgraph_count(ctypes.byref(ok), -1, p, p, p, p, None) == 1
    assert b"negative size" in L.mgx_last_error()
    assert L.mgx_node_subgraph_count(ctypes.byref(ok), 1, None, p, p, p, None) == 1
    assert b"NULL pointer" in L.mgx_last_error()
    assert L.mgx_node_subgraph_count(ctypes.byref(ok), 1, p, None, p, p, None) == 1
    assert b"workspace is NULL" in L.mgx_last_error()
    assert L.mgx_node_subgraph_count(ctypes.byref(ok), 1, p, p, p, None, None) == 1
    assert b"result is NULL" in L.mgx_last_error()
    assert L.mgx_node_subgraph_count(ctypes.byref(ok), 1, p, p, None, p, None) == 1
    assert b"counts is NULL" in L.mgx_last_error()
    assert L.mgx_node_subgraph_fill(ctypes.byref(ok), 1, p, p, p, 8, p, p, p, None) == 1
    assert b"out_bits must be 32 or 64, got 8" in L.mgx_last_error()
    some = _lib.MgxCsr(4, 4, 3, p, p, None, 64, 0)
    assert L.mgx_node_subgraph_fill(ctypes.byref(some), 1, p, p, None, 64, p, p, p, None) == 1
    assert b"NULL pointer" in L.mgx_last_error()
    assert L.mgx_node_subgraph_fill(ctypes.byref(some), 1, p, p, p, 64, p, p, None, None) == 1
    assert b"NULL pointer" in L.mgx_last_error()


@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
def test_cpu_graphs_take_the_torch_form(idtype, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the device path ran on a CPU graph")
    monkeypatch.setattr(sparse.HipBackend, "node_subgraph", boom)
    monkeypatch.setattr(config, "DEVICE_SUBGRAPH", True)
    g = parent("cpu", idtype, presorted=False)
    src, dst = (t.long() for t in g.edges())
    for name, sel in selections("cpu").items():
        sub = g.subgraph(sel)
        nodes = next(iter(sel.values())) if isinstance(sel, dict) else sel
        nodes = torch.nonzero(nodes).flatten() if nodes.dtype == torch.bool else nodes.long()
        local = {v: i for i, v in enumerate(nodes.tolist())}
        kept = [e for e in range(src.shape[0]) if src[e].item() in local and dst[e].item() in local]
        assert sub.edata[EID].tolist() == kept and torch.equal(sub.ndata[NID], nodes), name
        assert sub.edges()[0].tolist() == [local[src[e].item()] for e in kept] and sub.edges()[0].dtype == idtype
        assert sub.edges()[1].tolist() == [local[dst[e].item()] for e in kept]
        assert torch.equal(sub.ndata["x"], g.ndata["x"][nodes]) and torch.equal(sub.edata["w"], g.edata["w"][torch.tensor(kept, dtype=torch.int64)])
        assert sub._index._csc is None


# ---------------------------------------------------------------------------------------------------------------- GPU
class Spy(object):
    """Counts the calls of HipBackend.node_subgraph that go through."""

    def __init__(self, monkeypatch):
        self.calls = 0
        inner = sparse.HipBackend.node_subgraph

        def node_subgraph(backend, *a, **k):
            self.calls += 1
            return inner(backend, *a, **k)
        monkeypatch.setattr(sparse.HipBackend, "node_subgraph", node_subgraph)


@pytest.mark.gpu
@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("presorted", [False, True])
def test_selections_in_both_forms(presorted, idtype, monkeypatch):
    spy = Spy(monkeypatch)
    g = parent(DEV, idtype, presorted)
    assert (g._index._csc.eids is None) == presorted
    for name, sel in selections(DEV).items():
        monkeypatch.setattr(config, "DEVICE_SUBGRAPH", True)
        before = spy.calls
        a = g.subgraph(sel)
        assert spy.calls == before + 1, name
        monkeypatch.setattr(config, "DEVICE_SUBGRAPH", False)
        b = g.subgraph(sel)
        assert spy.calls == before + 1, name
        same_subgraph(a, b)
        assert a.idtype == idtype and b._index._csc is None
        if name == "all":
            assert a.number_of_edges() == g.number_of_edges()
        if name == "self loop":
            assert a.number_of_edges() == 1
        if name == "rows keep no edge":
            assert a.number_of_edges() == 0
        # the in-CSR handed over with the subgraph: the one its COO alone would give
        mine = a._index._csc
        assert mine is not None and a._index.format_status()["created"] == ["coo", "csc"]
        if a.number_of_nodes():
            ref = GraphIndex(a.number_of_nodes(), a.number_of_nodes(), coo=a._index._coo).csc()
            for x, y in ((mine.indptr, ref.indptr), (mine.indices, ref.indices), (mine.eids, ref.eids)):
                assert x.dtype == y.dtype and torch.equal(x, y), name
            assert (mine.num_rows, mine.num_cols) == (ref.num_rows, ref.num_cols)
        else:
            assert mine.indptr.tolist() == [0] and mine.nnz == 0


@pytest.mark.gpu
def test_duplicates_and_ids_out_of_range_raise(monkeypatch):
    monkeypatch.setattr(config, "DEVICE_SUBGRAPH", True)
    g = parent(DEV, torch.int32, presorted=False)
    good = g.subgraph(torch.tensor([HUB, 3, 250]))
    for sel, text in (([3, 9, 3], "more than once"), ([1, N], "outside"), ([-1, 4], "outside"), ([N, N], "outside")):
        with pytest.raises(mg.DGLError, match=text):
            g.subgraph(torch.tensor(sel))
        same_subgraph(g.subgraph(torch.tensor([HUB, 3, 250])), good)  # the device goes on


@pytest.mark.gpu
@pytest.mark.parametrize("presorted", [False, True])
def test_without_an_in_csr_the_torch_form_runs(presorted, monkeypatch):
    spy = Spy(monkeypatch)
    monkeypatch.setattr(config, "DEVICE_SUBGRAPH", True)
    L = _lib.lib()
    g = parent(DEV, torch.int64, presorted, with_csc=False)
    status = g._index.format_status()
    assert status["created"] == ["coo"]
    sel = torch.arange(N - 1, -1, -2)
    stale = L.mgx_last_error()
    a = g.subgraph(sel)
    assert spy.calls == 0 and g._index.format_status() == status and g._index._hidden_csc is None
    assert L.mgx_last_error() == stale and a._index._csc is None
    g._index.csc()
    b = g.subgraph(sel)
    assert spy.calls == 1
    same_subgraph(a, b)
