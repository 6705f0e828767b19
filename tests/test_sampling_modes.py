"""sample_neighbors with prob= / replace=True / edge_dir="out", select_topk, in_subgraph and the samplers over them.

Every check runs on CPU tensors (the torch formulation of mi355x_graph/sampling.py) and, marked gpu, on cuda:0 (the wave-per-seed
kernels of csrc/sample.hip) with an int32 and an int64 graph, which must pick the same positions.

The fixture graph has one destination node per in-degree of DEGS -- below, at and above the fanouts, at the 64 and 128 chunk
edges of the kernels, a remainder chunk, many chunks -- and its edge list is shuffled, so that edge ids are NOT CSR positions:
a kernel that reads prob[position] instead of prob[eid] fails every weighted check.

Statistical bounds are binomial 6 sigma (count of a Bernoulli(p) event over n independent trials: mean n p, variance n p (1 - p)),
derived, not measured; with the fixed generator seeds the tests are deterministic."""
import ctypes
import itertools
import math

import pytest
import torch

import mi355x_graph as mg
from mi355x_graph import _lib, sampling
from mi355x_graph.datasets import synthetic_edges

DEGS = [0, 1, 2, 7, 8, 9, 63, 64, 65, 127, 128, 129, 200, 1000]  # node i has in-degree DEGS[i]
N_OTHER = 1500
N = len(DEGS) + N_OTHER
ALL_ZERO, THREE_POS, D200, D1000 = DEGS.index(9), DEGS.index(65), DEGS.index(200), DEGS.index(1000)
FANOUTS = (1, 8, 64)
# every hub, two sources (no in-edges), not in id order
SEEDS = torch.tensor([12, 0, 5, 13, 3, 20, 7, 1, 9, 2, 11, 4, 6, 8, 10, 100])
_cache = {}


def fixture_edges():
    """(src, dst, weights) in edge-id order, built once."""
    if "edges" not in _cache:
        gen = torch.Generator().manual_seed(20260)
        dst = torch.repeat_interleave(torch.arange(len(DEGS)), torch.tensor(DEGS))
        src = torch.randint(len(DEGS), N, (dst.numel(),), generator=gen)
        perm = torch.randperm(dst.numel(), generator=gen)  # edge ids are not CSR positions
        src, dst = src[perm].contiguous(), dst[perm].contiguous()
        E = dst.numel()
        w = 0.5 + 1.5 * torch.rand(E, generator=gen)
        w[torch.rand(E, generator=gen) < 0.25] = 0.0
        w[dst == ALL_ZERO] = 0.0
        e65 = torch.nonzero(dst == THREE_POS).flatten()
        w[e65] = 0.0
        w[e65[[4, 31, 64]]] = torch.tensor([0.7, 1.9, 1.1])
        assert int((w[dst == D200] > 0).sum()) > 100 and int((w[dst == D200] == 0).sum()) > 20
        _cache["edges"] = (src, dst, w)
    return _cache["edges"]


def fixture_graph(dev, idtype=torch.int64, reverse=False):
    s, d, w = fixture_edges()
    if reverse:
        s, d = d, s
    g = mg.graph((s.to(dev).to(idtype), d.to(dev).to(idtype)), num_nodes=N)
    g.edata["w"] = w.to(dev)
    return g


def csr_positions(g, eid, edge_dir="in"):
    """CSR position of every returned edge id."""
    view = g._index.csc() if edge_dir == "in" else g._index.csr()
    E = view.nnz
    if view.eids is None:
        return eid
    inv = torch.empty(E, dtype=torch.int64, device=eid.device)
    inv[view.eids.long()] = torch.arange(E, device=eid.device)
    return inv[eid]


MODES = {  # name -> (edge_dir, weighted, replace)
    "weighted": ("in", True, False),
    "replace": ("in", False, True),
    "weighted_replace": ("in", True, True),
    "out": ("out", False, False),
    "out_weighted": ("out", True, False),
    "out_weighted_replace": ("out", True, True),
}


def run_structure(dev, idtype, mode, fanout):
    edge_dir, weighted, replace = MODES[mode]
    s, d, w = [t.to(dev) for t in fixture_edges()]
    g = fixture_graph(dev, idtype, reverse=edge_dir == "out")  # reversed: the hubs' OUT-degrees are DEGS
    if edge_dir == "out":
        s, d = d, s
    seeds = SEEDS.to(dev)
    call = lambda: sampling.sample_neighbors(g, seeds, fanout, edge_dir=edge_dir, prob="w" if weighted else None, replace=replace,
                                             generator=torch.Generator().manual_seed(100 + fanout))
    src, dst, eid = call()
    assert src.dtype == dst.dtype == eid.dtype == torch.int64
    # every edge exists by edge id, has a positive weight when weighted
    assert torch.equal(s[eid], src) and torch.equal(d[eid], dst)
    if weighted:
        assert bool((w[eid] > 0).all())
    # counts per seed, grouped by seed in seed order
    seed_end = d if edge_dir == "in" else s
    eligible = torch.bincount(seed_end[w > 0] if weighted else seed_end, minlength=N)[seeds]
    expect = (eligible > 0).long() * fanout if replace else torch.clamp(eligible, max=fanout)
    seg = torch.repeat_interleave(torch.arange(seeds.numel(), device=dev), expect)
    got_seed = dst if edge_dir == "in" else src
    assert got_seed.numel() == seg.numel() and torch.equal(got_seed, seeds[seg])
    by_seed = dict(zip(seeds.tolist(), expect.tolist()))
    assert by_seed[0] == 0 and by_seed[20] == 0 and by_seed[100] == 0  # no edges at all
    if weighted:
        assert by_seed[ALL_ZERO] == 0 and by_seed[THREE_POS] == (fanout if replace else min(3, fanout))
    # CSR positions non-decreasing inside a seed; distinct without replacement
    pos = csr_positions(g, eid, edge_dir)
    same = seg[1:] == seg[:-1]
    step = (pos[1:] - pos[:-1])[same]
    assert bool((step >= 0).all())
    if not replace:
        assert bool((step > 0).all()) and eid.unique().numel() == eid.numel()
    # the same generator state gives the same sample
    assert torch.equal(call()[2], eid)
    return pos


@pytest.mark.parametrize("fanout", FANOUTS)
@pytest.mark.parametrize("mode", sorted(MODES))
def test_structure_cpu(mode, fanout):
    run_structure("cpu", torch.int64, mode, fanout)


@pytest.mark.gpu
@pytest.mark.parametrize("fanout", FANOUTS)
@pytest.mark.parametrize("mode", sorted(MODES))
def test_structure_gpu(mode, fanout):
    p32 = run_structure("cuda:0", torch.int32, mode, fanout)
    p64 = run_structure("cuda:0", torch.int64, mode, fanout)
    assert torch.equal(p32, p64)  # the index width does not change the sample


def test_fanout_above_device_limit_and_all_edges():
    """fanout > 64 (the torch formulation on any device) and fanout None with weights."""
    g = fixture_graph("cpu")
    s, d, w = fixture_edges()
    src, dst, eid = sampling.sample_neighbors(g, SEEDS, 100, prob="w", generator=torch.Generator().manual_seed(1))
    pos_cnt = torch.bincount(d[w > 0], minlength=N)
    assert torch.equal(torch.bincount(dst, minlength=N)[SEEDS], torch.clamp(pos_cnt[SEEDS], max=100))
    assert bool((w[eid] > 0).all()) and eid.unique().numel() == eid.numel()
    src, dst, eid = sampling.sample_neighbors(g, SEEDS, None, prob="w")
    assert torch.equal(torch.bincount(dst, minlength=N)[SEEDS], pos_cnt[SEEDS]) and bool((w[eid] > 0).all())
    with pytest.raises(mg.DGLError):
        sampling.sample_neighbors(g, SEEDS, 3, edge_dir="sideways")


# ---- select_topk


def topk_sets(got, E):
    src, dst, eid = got
    out = {}
    for v, e in zip(dst.tolist(), eid.tolist()):
        out.setdefault(v, []).append(e)
    return out


def run_topk(dev, idtype):
    s, d, _ = fixture_edges()
    E = d.numel()
    wt = torch.randperm(E, generator=torch.Generator().manual_seed(5)).float()  # distinct weights
    g = fixture_graph(dev, idtype)
    g.edata["score"] = wt.to(dev)
    in_edges = {v: torch.nonzero(d == v).flatten() for v in range(len(DEGS))}
    positions = []
    for k, ascending, nodes in itertools.product(FANOUTS, (False, True), (None, torch.tensor([13, 3, 500, 8, 0, 12]))):
        src, dst, eid = sampling.select_topk(g, k, "score", nodes=None if nodes is None else nodes.to(dev), ascending=ascending)
        sd, dd = s.to(dev), d.to(dev)
        assert torch.equal(sd[eid], src) and torch.equal(dd[eid], dst)
        got = topk_sets((src, dst, eid), E)
        want_nodes = range(N) if nodes is None else nodes.tolist()
        assert set(got) == {v for v in want_nodes if v < len(DEGS) and DEGS[v] > 0}
        assert dst.tolist() == [v for v in want_nodes if v < len(DEGS) for _ in range(min(k, DEGS[v]))]  # seed order, counts
        for v, e in got.items():
            ie = in_edges[v]
            ref = ie[torch.topk(wt[ie], min(k, ie.numel()), largest=not ascending).indices]
            assert sorted(e) == sorted(ref.tolist()), (k, ascending, v)
        pos = csr_positions(g, eid)
        same = dst[1:] == dst[:-1]
        assert bool(((pos[1:] - pos[:-1])[same] > 0).all())
        positions.append(pos)
    # all weights equal: the k lowest CSR positions of every row
    csc = g._index.csc()
    for k in FANOUTS:
        src, dst, eid = sampling.select_topk(g, k, torch.full((E,), 2.5), ascending=False)
        want = [csc.eids[int(csc.indptr[v]):int(csc.indptr[v]) + min(k, DEGS[v])].long() for v in range(len(DEGS))]
        assert torch.equal(eid, torch.cat(want))
        positions.append(csr_positions(g, eid))
    return positions


def test_select_topk_exact_cpu():
    run_topk("cpu", torch.int64)


@pytest.mark.gpu
def test_select_topk_exact_gpu():
    p32, p64 = run_topk("cuda:0", torch.int32), run_topk("cuda:0", torch.int64)
    assert all(torch.equal(a, b) for a, b in zip(p32, p64))


# ---- distributions


def check_binomial(count, p, n):
    """|count_i - n p_i| < 6 sqrt(n p_i (1 - p_i)) for every i; p_i == 0 must give exactly 0."""
    count, p = count.double().cpu(), p.double().cpu()
    assert bool((count[p == 0] == 0).all())
    dev = (count - n * p).abs()
    bound = 6 * torch.sqrt(n * p * (1 - p))
    worst = float((dev[p > 0] / bound[p > 0]).max())
    print("largest deviation: %.2f of the 6-sigma bound" % worst)
    assert bool((dev[p > 0] < bound[p > 0]).all())


def run_distribution_replace(dev, idtype):
    s, d, w = fixture_edges()
    g = fixture_graph(dev, idtype)
    ie = torch.nonzero(d == D200).flatten()
    seeds = torch.full((4000,), D200, device=dev)
    out = []
    for prob, p in (("w", w[ie].double() / w[ie].double().sum()), (None, torch.full((200,), 1 / 200.0, dtype=torch.float64))):
        _, dst, eid = sampling.sample_neighbors(g, seeds, 8, prob=prob, replace=True, generator=torch.Generator().manual_seed(7))
        count = torch.bincount(eid, minlength=d.numel()).cpu()
        assert int(count.sum()) == 32000 and int(count[ie].sum()) == 32000 and dst.numel() == 32000
        check_binomial(count[ie], p, 32000)
        out.append(eid)
    return out


def test_distribution_with_replacement_cpu():
    run_distribution_replace("cpu", torch.int64)


@pytest.mark.gpu
def test_distribution_with_replacement_gpu():
    a, b = run_distribution_replace("cuda:0", torch.int32), run_distribution_replace("cuda:0", torch.int64)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def inclusion_probabilities(w, k):
    """P(edge i among k successive draws proportional to w without replacement), by enumeration of the ordered draws."""
    n = len(w)
    pi = [0.0] * n
    for order in itertools.permutations(range(n), k):
        p, rest = 1.0, sum(w)
        for i in order:
            p *= w[i] / rest
            rest -= w[i]
        for i in order:
            pi[i] += p
    return pi


def run_distribution_no_replace(dev, idtype):
    s, d, w = fixture_edges()
    g = fixture_graph(dev, idtype)
    out = []
    # fanout 1: one draw proportional to the weight
    ie = torch.nonzero(d == D200).flatten()
    n = 16000
    _, _, eid = sampling.sample_neighbors(g, torch.full((n,), D200, device=dev), 1, prob="w", generator=torch.Generator().manual_seed(8))
    count = torch.bincount(eid, minlength=d.numel()).cpu()
    assert int(count[ie].sum()) == n and eid.numel() == n
    check_binomial(count[ie], w[ie].double() / w[ie].double().sum(), n)
    out.append(eid)
    # fanout 3 of 5 edges: inclusion probabilities of successive sampling (60 ordered draws)
    w5 = [1.0, 2.0, 3.0, 4.0, 0.5]
    perm = torch.tensor([3, 0, 4, 2, 1])  # edge ids shuffled against the weights' order
    g5 = mg.graph((torch.arange(1, 6)[perm].to(dev).to(idtype), torch.zeros(5, dtype=idtype, device=dev)), num_nodes=6)
    w_by_eid = torch.tensor(w5)[perm]
    pi = inclusion_probabilities(w_by_eid.tolist(), 3)
    assert abs(sum(pi) - 3) < 1e-12
    n = 20000
    _, _, eid = sampling.sample_neighbors(g5, torch.zeros(n, dtype=torch.int64, device=dev), 3, prob=w_by_eid.to(dev),
                                          generator=torch.Generator().manual_seed(9))
    count = torch.bincount(eid, minlength=5).cpu()
    assert int(count.sum()) == 3 * n
    check_binomial(count, torch.tensor(pi), n)
    out.append(eid)
    # fanout 10 of 1000 equal weights: every edge is included with probability 10 / 1000 (a biased multi-chunk merge is not)
    ie = torch.nonzero(d == D1000).flatten()
    n = 3000
    _, _, eid = sampling.sample_neighbors(g, torch.full((n,), D1000, device=dev), 10, prob=torch.ones(d.numel(), device=dev),
                                          generator=torch.Generator().manual_seed(10))
    count = torch.bincount(eid, minlength=d.numel()).cpu()
    assert int(count[ie].sum()) == 10 * n and eid.numel() == 10 * n
    check_binomial(count[ie], torch.full((1000,), 0.01, dtype=torch.float64), n)
    out.append(eid)
    return out


def test_distribution_without_replacement_cpu():
    run_distribution_no_replace("cpu", torch.int64)


@pytest.mark.gpu
def test_distribution_without_replacement_gpu():
    a, b = run_distribution_no_replace("cuda:0", torch.int32), run_distribution_no_replace("cuda:0", torch.int64)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---- validation


def run_validation(dev, idtype):
    s, d, w = fixture_edges()
    g = fixture_graph(dev, idtype)
    seeds = torch.tensor([3, 12, 8], device=dev)
    on_seed = int(torch.nonzero(d == 12).flatten()[17])
    off_seed = int(torch.nonzero(d == 13).flatten()[5])
    for bad in (-1.0, float("nan")):
        for replace in (False, True):
            wb = w.clone()
            wb[off_seed] = bad  # not an in-edge of a seed: not looked at
            sampling.sample_neighbors(g, seeds, 8, prob=wb.to(dev), replace=replace)
            wb[on_seed] = bad
            with pytest.raises(mg.DGLError):
                sampling.sample_neighbors(g, seeds, 8, prob=wb.to(dev), replace=replace)
    with pytest.raises(mg.DGLError):
        sampling.sample_neighbors(g, seeds, 8, prob=w[:-1].to(dev))
    with pytest.raises(mg.DGLError):
        sampling.sample_neighbors(g, seeds, 8, prob="no_such_feature")
    with pytest.raises(mg.DGLError):
        sampling.select_topk(g, 8, w[:-1].to(dev))
    # fp64 / fp16 weights are converted on the host
    a = sampling.sample_neighbors(g, seeds, 8, prob=w.to(dev), generator=torch.Generator().manual_seed(3))[2]
    b = sampling.sample_neighbors(g, seeds, 8, prob=w.double().to(dev), generator=torch.Generator().manual_seed(3))[2]
    assert torch.equal(a, b)
    c = sampling.sample_neighbors(g, seeds, 8, prob=w.half().to(dev), generator=torch.Generator().manual_seed(3))[2]
    assert bool((w.to(dev)[c] > 0).all())


def test_validation_cpu():
    run_validation("cpu", torch.int64)


@pytest.mark.gpu
def test_validation_gpu():
    run_validation("cuda:0", torch.int32)
    run_validation("cuda:0", torch.int64)


def test_entry_points_reject_bad_arguments():
    """Through ctypes, no GPU needed: the argument checks come before any launch."""
    L = _lib.lib()
    csr = _lib.MgxCsr(1, 1, 0, None, None, None, 32, 0)
    assert L.mgx_sample_neighbors_weighted(None, 1, None, 8, None, 1, 0, None, None, None, None) == 1
    assert b"csr is NULL" in L.mgx_last_error()
    assert L.mgx_sample_neighbors_weighted(ctypes.byref(csr), 1, None, 65, None, 1, 0, None, None, None, None) == 1
    assert b"fanout must be in [1, 64], got 65" in L.mgx_last_error()
    assert L.mgx_sample_neighbors_weighted(ctypes.byref(csr), 1, None, 0, None, 1, 0, None, None, None, None) == 1
    assert L.mgx_sample_neighbors_weighted(ctypes.byref(csr), 1, None, 8, None, 0, 0, None, None, None, None) == 1
    assert b"prob is NULL" in L.mgx_last_error()
    assert L.mgx_select_topk(None, 1, None, 8, None, 0, None, None, None, None) == 1
    assert b"csr is NULL" in L.mgx_last_error()
    assert L.mgx_select_topk(ctypes.byref(csr), 1, None, 65, None, 0, None, None, None, None) == 1
    assert b"k must be in [1, 64], got 65" in L.mgx_last_error()
    assert L.mgx_sample_count_positive(None, 1, None, None, None, None, None) == 1
    assert b"csr is NULL" in L.mgx_last_error()
    with pytest.raises(mg.DGLError):
        _lib.check(1)


# ---- samplers and the dgl spellings


def loader_graph(dev):
    s, d = synthetic_edges(3000, 40000, 300, seed=11, symmetric=True)
    g = mg.graph((s.to(dev), d.to(dev)), num_nodes=3000)
    w = torch.rand(s.numel(), generator=torch.Generator().manual_seed(2))
    w[w < 0.3] = 0.0
    g.edata["w"] = w.to(dev)
    return g, s.to(dev), d.to(dev), w.to(dev)


def run_samplers(dev):
    g, s, d, w = loader_graph(dev)
    deg = torch.bincount(d, minlength=3000)
    blocks_replace = None
    for kwargs in ({"replace": True}, {"prob": "w"}):
        sampler = sampling.MultiLayerNeighborSampler([5, 10], **kwargs)
        loader = sampling.NodeDataLoader(g, torch.arange(600), sampler, batch_size=300, shuffle=False)
        seen = 0
        for inp, out, blocks in loader:
            b0, b1 = blocks
            seen += out.numel()
            assert torch.equal(b0.dstdata[sampling.NID], b1.srcdata[sampling.NID])    # layers chain
            assert torch.equal(b1.srcdata[sampling.NID][:out.numel()], out)           # destinations are a prefix of sources
            assert torch.equal(b0.srcdata[sampling.NID], inp)
            for b, fanout in ((b0, 5), (b1, 10)):
                ls, ld = b.edges()
                e = b.edata[sampling.EID]
                assert torch.equal(s[e], b.srcdata[sampling.NID][ls.long()]) and torch.equal(d[e], b.dstdata[sampling.NID][ld.long()])
                indeg = torch.bincount(ld.long(), minlength=b.number_of_dst_nodes())
                if "replace" in kwargs:  # every destination with an in-edge gets exactly `fanout`, duplicates included
                    assert torch.equal(indeg, (deg[b.dstdata[sampling.NID]] > 0).long() * fanout)
                else:
                    assert int(indeg.max()) <= fanout and bool((w[e] > 0).all()) and e.unique().numel() == e.numel()
            if "replace" in kwargs:
                blocks_replace = blocks
        assert seen == 600
    return blocks_replace


def test_samplers_and_aliases_cpu():
    run_samplers("cpu")
    import dgl
    assert dgl.sampling.select_topk is sampling.select_topk and dgl.sampling.sample_neighbors is sampling.sample_neighbors
    assert dgl.dataloading.sample_neighbors is sampling.sample_neighbors and dgl.in_subgraph is sampling.in_subgraph
    g = fixture_graph("cpu")
    s, d, w = fixture_edges()
    src, dst, eid = dgl.in_subgraph(g, SEEDS)
    ref = sampling.sample_neighbors(g, SEEDS, None)
    assert all(torch.equal(a, b) for a, b in zip((src, dst, eid), ref)) and eid.numel() == sum(DEGS)
    a = dgl.dataloading.sample_neighbors(g, SEEDS, 8, replace=True, generator=torch.Generator().manual_seed(4))
    b = sampling.sample_neighbors(g, SEEDS, 8, replace=True, generator=torch.Generator().manual_seed(4))
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    a, b = dgl.sampling.select_topk(g, 8, "w"), sampling.select_topk(g, 8, w)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.gpu
def test_samplers_and_block_spmm_gpu():
    from mi355x_graph import ops
    dev = "cuda:0"
    blocks = run_samplers(dev)
    # mean over a block with multi-edges: a duplicate counts twice.  Both sides are fp32 sums of at most 10 terms of U[0, 1).
    b = blocks[1].int()
    x = torch.rand(b.number_of_src_nodes(), 32, device=dev)
    ls, ld = [t.long() for t in b.edges()]
    assert int(torch.unique(torch.stack([ls, ld]), dim=1).shape[1]) < ls.numel()  # there ARE duplicates
    nd = b.number_of_dst_nodes()
    cnt = torch.bincount(ld, minlength=nd).clamp(min=1).float()[:, None]
    ref = torch.zeros(nd, 32, device=dev).index_add(0, ld, x[ls]) / cnt
    got = ops.gspmm(b, "copy_lhs", "mean", x, None)
    err = float(((got - ref).abs() / ref.abs().clamp(min=1e-6)).max())
    print("gspmm(copy_lhs, mean) on a replace=True block: relative error %.2e" % err)
    assert err < 1e-5
    g = fixture_graph(dev, torch.int32)
    a = sampling.in_subgraph(g, SEEDS.to(dev))
    assert a[2].numel() == sum(DEGS)
    assert math.isfinite(float(got.sum()))
