"""Sparse x sparse product: ops.spgemm (csrc/spgemm.hip), dgl.adj_product_graph and dgl.metapath_reachable_graph against one dense
fp64 restatement in plain torch: index_put(accumulate=True) of the weights into dense A and B, A @ B; the pattern is that of the same
product with every weight 1, so that cancelled sums stay in; gradients by fp64 autograd of sum(wc * g).

The device operands are built from config.SPGEMM_*: rows of A with 0, 1, 31, 32, 33, T1 - 1, T1, T1 + 1, T2, T2 + 1 and 3 T2 + 32
products, reached by pointing few entries of A at rows of B of chosen lengths -- the smallest shapes at which a class switch, a table
wrap, a window edge (m = W + 37) or a colliding slot can lose or double a product.  Integer weights make every fp32 sum exact: results
must be torch.equal.  Random weights: per element |got - ref| <= (T + 4) * 2^-24 * sum |terms|, T the number of terms of that element
and sum |terms| the restatement run on absolute values (the running-sum bound of tests/test_segment_mm.py: any summation order)."""
import functools

import pytest
import torch

import dgl
import mi355x_graph as mg
from mi355x_graph import config, ops, sparse

DEV = "cuda:0"
T1, T2, W = config.SPGEMM_T1, config.SPGEMM_T2, config.SPGEMM_W
M = W + 37


@functools.lru_cache(maxsize=None)
def operands():
    """(src_a, dst_a, n, src_b, dst_b, k): edge lists in a random edge-id order"""
    gen = torch.Generator().manual_seed(5)
    distinct = lambda count: torch.randperm(M - 1, generator=gen)[:count]
    b_rows = [torch.empty(0, dtype=torch.long),          # 0: empty, referred to by A
              torch.tensor([M - 1]),                      # 1: the last column
              distinct(31), distinct(32), distinct(T1 - 1),   # 2, 3, 4
              distinct(T2),                               # 5: no two products alike
              torch.tensor([5, 5]),                       # 6: a column held twice
              torch.full((T2,), 7)]                       # 7: every product on one column
    a_rows = [[], [0], [1], [2], [3], [3, 1], [4], [4, 1], [4, 6], [5], [5, 1], [5, 5, 7, 0, 3], [7], [1, 1], [6, 6, 2]]
    a_rows = a_rows + [[], [2, 0]]  # products: 0 0 1 31 32 33 T1-1 T1 T1+1 T2 T2+1 3T2+32 T2 2 35 0 31
    pairs = []
    for rows in (a_rows, b_rows):
        src = torch.repeat_interleave(torch.arange(len(rows)), torch.tensor([len(r) for r in rows]))
        dst = torch.cat([torch.as_tensor(r, dtype=torch.long) for r in rows])
        order = torch.randperm(len(src), generator=gen)
        pairs += [src[order], dst[order], len(rows)]
    return tuple(pairs)


def graphs(dev, idtype):
    src_a, dst_a, n, src_b, dst_b, k = operands()
    return (mg.create_block((src_a, dst_a), n, k, idtype=idtype, device=dev), mg.create_block((src_b, dst_b), k, M, idtype=idtype, device=dev))


@functools.lru_cache(maxsize=None)
def weights(integer):
    gen = torch.Generator().manual_seed(9)
    draw = (lambda n: torch.randint(-2, 3, (n,), generator=gen).float()) if integer else (lambda n: torch.randn(n, generator=gen))
    ea, eb = len(operands()[0]), len(operands()[3])
    return draw(ea), draw(eb), draw(ea * eb)  # the last: g, cut to nnz(C)


def restate(src_a, dst_a, n, src_b, dst_b, k, m, wa, wb, g=None):
    """(indptr, indices, wc, d wa, d wb) in fp64; None weights are ones"""
    ones = lambda w, e: torch.ones(len(e), dtype=torch.float64) if w is None else w.detach().double().cpu().requires_grad_(True)
    wa, wb = ones(wa, src_a), ones(wb, src_b)
    dense = lambda rows, cols, w, shape: torch.zeros(shape, dtype=torch.float64).index_put((rows, cols), w, accumulate=True)
    pattern = dense(src_a, dst_a, torch.ones_like(wa), (n, k)) @ dense(src_b, dst_b, torch.ones_like(wb), (k, m)) > 0
    wc = (dense(src_a, dst_a, wa, (n, k)) @ dense(src_b, dst_b, wb, (k, m)))[pattern]
    indptr = torch.cat([torch.zeros(1, dtype=torch.long), pattern.sum(1).cumsum(0)])
    grads = {}
    if g is not None and wc.requires_grad:
        asked = [w for w in (wa, wb) if w.requires_grad]
        grads = dict(zip(map(id, asked), torch.autograd.grad((wc * g[:len(wc)].double()).sum(), asked)))
    return indptr, pattern.nonzero()[:, 1], wc.detach(), grads.get(id(wa)), grads.get(id(wb))


@functools.lru_cache(maxsize=None)
def reference(mode, integer=True):
    wa, wb, g = weights(integer)
    wa, wb = (wa if mode != "pattern" else None), (wb if mode == "weighted" else None)
    return restate(*operands(), M, wa, wb, g)


def on_device(mode, integer=True):
    wa, wb, g = weights(integer)
    return (wa.to(DEV) if mode != "pattern" else None), (wb.to(DEV) if mode == "weighted" else None), g.to(DEV)


def structure(gc):
    c = gc._index.csr()
    assert c.eids is None  # edge id = CSR position
    return c.indptr.cpu().long(), c.indices.cpu().long()


@pytest.mark.gpu
@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("mode", ["weighted", "wa_only", "pattern"])
def test_structure_and_exact_values(idtype, mode):
    ga, gb = graphs(DEV, idtype)
    wa, wb, _ = on_device(mode)
    indptr, indices, wc_ref, _, _ = reference(mode)
    gc, wc = ops.spgemm(ga, gb, wa, wb)
    assert gc.idtype == idtype and (gc.number_of_src_nodes(), gc.number_of_dst_nodes()) == (ga.number_of_src_nodes(), M)
    got_ptr, got_idx = structure(gc)
    assert torch.equal(got_ptr, indptr) and torch.equal(got_idx, indices)
    assert (wc is None) if mode == "pattern" else torch.equal(wc.cpu().double(), wc_ref)
    gc2, wc2 = ops.spgemm(ga, gb, wa, wb)
    assert torch.equal(structure(gc2)[1], got_idx) and (wc is None or torch.equal(wc2, wc))


@pytest.mark.gpu
@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("integer", [True, False])
def test_gradients(idtype, integer):
    ga, gb = graphs(DEV, idtype)
    wa, wb, g = on_device("weighted", integer)
    wa, wb = wa.requires_grad_(True), wb.requires_grad_(True)
    _, _, wc_ref, d_wa, d_wb = reference("weighted", integer)
    _, wc = ops.spgemm(ga, gb, wa, wb)
    got = torch.autograd.grad((wc * g[:len(wc)]).sum(), (wa, wb))
    if integer:
        assert torch.equal(got[0].cpu().double(), d_wa) and torch.equal(got[1].cpu().double(), d_wb)
        return
    w_abs = tuple(w.abs() for w in weights(False))
    ones = tuple(torch.ones_like(w) for w in weights(False))
    mags, terms = restate(*operands(), M, *w_abs), restate(*operands(), M, *ones)
    for what, x, ref, mag, t in (("wc", wc, wc_ref, mags[2], terms[2]), ("d wa", got[0], d_wa, mags[3], terms[3]), ("d wb", got[1], d_wb, mags[4], terms[4])):
        err, bound = (x.detach().cpu().double() - ref).abs(), (t + 4) * 2.0 ** -24 * mag
        print("%s: largest error %.3g, of its bound %.3g" % (what, err.max(), (err / bound.clamp(min=1e-300)).max()))
        assert bool((err <= bound).all()), what


def rejected(ga, gb, wa, wb):
    """{label: operands} the operator must reject, each one edit of the accepted call"""
    src_a, dst_a, n, _, _, k = operands()
    other = torch.int64 if ga.idtype == torch.int32 else torch.int32
    return {"inner": (ga, mg.create_block((src_a, dst_a), n, k, idtype=ga.idtype, device=ga.device), wa, wb),
            "idtype": (ga, graphs(ga.device, other)[1], wa, wb),
            "device": (ga, graphs("cpu", ga.idtype)[1], wa, None),
            "double": (ga, gb, wa.double(), wb),
            "2d": (ga, gb, wa, wb.view(-1, 1)),
            "length": (ga, gb, wa[:-1], wb),
            "no_graph": (ga, None, wa, wb)}


@pytest.mark.gpu
def test_the_predicate_names_the_path(monkeypatch):
    ga, gb = graphs(DEV, torch.int32)
    wa, wb, _ = on_device("weighted")
    backend, calls = type(sparse.backend_for(wa)), []
    inner = backend.spgemm
    monkeypatch.setattr(backend, "spgemm", lambda self, *a: calls.append(1) or inner(self, *a))
    assert ops.spgemm_fused(ga, gb, wa, wb) is True
    gc, wc = ops.spgemm(ga, gb, wa, wb)
    assert len(calls) == 1
    monkeypatch.setattr(config, "SPGEMM_FUSED", False)
    assert ops.spgemm_fused(ga, gb, wa, wb) is False
    gc2, wc2 = ops.spgemm(ga, gb, wa, wb)
    assert len(calls) == 1
    assert all(torch.equal(x, y) for x, y in zip(structure(gc) + (wc,), structure(gc2) + (wc2,)))
    monkeypatch.setattr(config, "SPGEMM_FUSED", True)
    for label, args in rejected(ga, gb, wa, wb).items():
        assert ops.spgemm_fused(*args) is False, label
        with pytest.raises(mg.DGLError, match="spgemm:"):
            ops.spgemm(*args)


# ---- no GPU
SRC = torch.tensor([0, 0, 1, 2, 0, 4, 5, 3])
DST = torch.tensor([1, 2, 2, 0, 1, 5, 4, 3])


@pytest.fixture
def cpu_backend():
    was = mg.enable_cpu_backend(True)
    yield
    mg.enable_cpu_backend(was)


def test_composed_path_and_rejections_on_the_cpu(cpu_backend):
    g = mg.graph((SRC, DST), num_nodes=6)
    wa, wb = torch.arange(1.0, 9.0), torch.arange(2.0, 10.0)
    indptr, indices, wc_ref, _, _ = restate(SRC, DST, 6, SRC, DST, 6, 6, wa, wb)
    gc, wc = ops.spgemm(g, g, wa, wb)
    assert ops.spgemm_fused(g, g, wa, wb) is False
    got_ptr, got_idx = structure(gc)
    assert torch.equal(got_ptr, indptr) and torch.equal(got_idx, indices) and torch.equal(wc.double(), wc_ref)
    assert ops.spgemm(g, g)[1] is None
    for label, args in {"double": (g, g, wa.double(), wb), "length": (g, g, wa, wb[:-1]), "no_graph": (None, g, wa, wb),
                        "inner": (g, mg.graph((SRC, DST), num_nodes=7), wa, wb), "idtype": (g, g.int(), wa, wb)}.items():
        assert ops.spgemm_fused(*args) is False, label
        with pytest.raises(mg.DGLError, match="spgemm:"):
            ops.spgemm(*args)


def test_adj_product_graph_carries_gradient_and_node_data(cpu_backend):
    assert {"spgemm", "spgemm_fused"} <= set(ops.__all__) and dgl.adj_product_graph is mg.transform.adj_product_graph
    A, B = mg.graph((SRC, DST), num_nodes=6), mg.graph((DST, SRC), num_nodes=6)
    A.edata["w"], B.edata["w"] = torch.arange(1.0, 9.0).requires_grad_(True), torch.arange(2.0, 10.0).requires_grad_(True)
    A.ndata["x"] = torch.arange(6.0)
    C = dgl.adj_product_graph(A, B, "w")
    g = torch.arange(1.0, C.number_of_edges() + 1)
    _, _, wc_ref, d_wa, d_wb = restate(SRC, DST, 6, DST, SRC, 6, 6, A.edata["w"], B.edata["w"], g)
    assert torch.equal(C.edata["w"].double(), wc_ref) and torch.equal(C.ndata["x"], A.ndata["x"]) and not C.is_block
    (C.edata["w"] * g).sum().backward()
    assert torch.equal(A.edata["w"].grad.double(), d_wa) and torch.equal(B.edata["w"].grad.double(), d_wb)
    U = dgl.bipartite((SRC[:5], DST[:5]), "user", "rates", "item", num_nodes=(3, 4))
    V = dgl.bipartite((DST[:5], SRC[:5]), "item", "rated", "tag", num_nodes=(4, 3))
    U.edata["w"], V.edata["w"] = torch.ones(5), torch.ones(5)
    U.nodes["user"].data["x"], V.nodes["tag"].data["y"] = torch.arange(3.0), torch.arange(3.0) + 7
    P = dgl.adj_product_graph(U, V, "w", etype="tagged")
    assert P.canonical_etypes == [("user", "tagged", "tag")] and torch.equal(P.nodes["user"].data["x"], torch.arange(3.0))
    assert torch.equal(P.nodes["tag"].data["y"], torch.arange(3.0) + 7)


def test_metapath_reachable_graph_is_the_boolean_chain(cpu_backend):
    rel = {("a", "ab", "b"): (torch.tensor([0, 0, 1, 2]), torch.tensor([0, 3, 1, 1])),
           ("b", "bc", "c"): (torch.tensor([0, 1, 1, 3, 3]), torch.tensor([1, 0, 0, 1, 1])),
           ("c", "ca", "a"): (torch.tensor([0, 1]), torch.tensor([2, 0]))}
    sizes = {"a": 3, "b": 4, "c": 2}
    g = dgl.heterograph(rel, sizes)
    g.nodes["a"].data["x"] = torch.arange(3.0)
    dense = lambda c: torch.zeros(sizes[c[0]], sizes[c[2]]).index_put(rel[c], torch.ones(1), accumulate=True)
    for path in (["ab", "bc", "ca"], ["ab", "bc"], ["bc"]):
        cets = [g.to_canonical_etype(e) for e in path]
        want = functools.reduce(torch.matmul, [dense(c) for c in cets]) > 0
        out = dgl.metapath_reachable_graph(g, path)
        src, dst = (out if path[0] == "ab" and path[-1] == "ca" else out[out.canonical_etypes[0]]).edges()
        assert torch.equal(torch.stack([src, dst], 1).long(), want.nonzero()), path
    assert torch.equal(dgl.metapath_reachable_graph(g, ["ab", "bc", "ca"]).ndata["x"], torch.arange(3.0))
