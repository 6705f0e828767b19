"""ops.lstm_aggregate (csrc/lstm_agg.hip) and SAGEConv(aggregator_type="lstm") against one fp64 restatement in plain torch: a Python loop
over rows and positions with nn.LSTM's documented formulas (gate order i, f, g, o), the positions of a row in the storage order of the
in-CSR the graph holds; gradients by fp64 autograd of sum(out * up).

The bound is measured, not derived (a 70-step recurrence): the same restatement runs in fp32 on the CPU and every tensor may be off by
|got - ref64| <= 4 * max|ref32 - ref64| + 1e-6 -- the factor 4 for a different summation order inside the 64-term products and the
device's exp and tanh being a few ulp off libm.  The tests print the ratio max|got - ref64| / max|ref32 - ref64| (docs/LOG_lstm_agg.md has
the observed ones).  The weights are drawn as nn.LSTM draws them and x ~ randn, so no gate saturates and a lost, doubled or reordered
step moves the result by orders of magnitude more than rounding.

Device shape: a block of 50 source and 37 destination rows -- two full tiles of 16 and one of 5 -- with in-degrees 0, 1, 2, 15, 16, 17, 33
and 70 scattered over the row ids, shuffled edge ids, a row that reads one source twice, and the only empty row in a tile with rows of
15 (sorted by degree the last tile is 15, 15, 2, 1, 0)."""
import functools

import pytest
import torch

import dgl
import mi355x_graph as mg
from mi355x_graph import config, ops, sparse

DEV = "cuda:0"
N_SRC, N_DST = 50, 37
NAMES = ("out", "d x", "d w_ih", "d w_hh", "d b_ih", "d b_hh")
CASES = [(16, 16, True), (48, 48, True), (64, 64, True), (64, 20, True), (48, 48, False)]  # H, D, biases


@functools.lru_cache(maxsize=None)
def block_edges():
    gen = torch.Generator().manual_seed(11)
    degrees = torch.tensor([70, 33, 33] + [17] * 9 + [16] * 11 + [15] * 11 + [2, 1, 0])[torch.randperm(N_DST, generator=gen)]
    assert degrees.numel() == N_DST
    dst = torch.repeat_interleave(torch.arange(N_DST), degrees)
    src = torch.randint(0, N_SRC, (dst.numel(),), generator=gen)
    src[dst == int((degrees == 2).nonzero())] = 7  # one row reads the same source twice
    shuffle = torch.randperm(dst.numel(), generator=gen)
    return src[shuffle], dst[shuffle]


@functools.lru_cache(maxsize=None)
def operands(n_src, n_dst, H, D, biases):
    """(x, w_ih, w_hh[, b_ih, b_hh]), up: fp32 on the host"""
    torch.manual_seed(H + D)
    lstm = torch.nn.LSTM(D, H, bias=biases, batch_first=True)
    gen = torch.Generator().manual_seed(3)
    x, up = torch.randn(n_src, D, generator=gen), torch.randn(n_dst, H, generator=gen)
    return (x,) + tuple(p.detach() for p in lstm.parameters()), up


def restate(csc, given, up, dtype):
    """[out, d x, d w_ih, d w_hh(, d b_ih, d b_hh)] in `dtype` on the host"""
    indptr, indices = csc.indptr.cpu().tolist(), csc.indices.cpu().tolist()
    leaves = [t.detach().cpu().to(dtype).requires_grad_() for t in given]
    x, w_ih, w_hh = leaves[:3]
    bias = leaves[3] + leaves[4] if len(leaves) == 5 else 0
    rows = []
    for v in range(len(indptr) - 1):
        h = c = torch.zeros(w_hh.shape[1], dtype=dtype)
        for p in range(indptr[v], indptr[v + 1]):
            i, f, g, o = (w_ih @ x[indices[p]] + w_hh @ h + bias).chunk(4)
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
            h = torch.sigmoid(o) * torch.tanh(c)
        rows.append(h)
    out = torch.stack(rows)
    (out * up.to(dtype)).sum().backward()
    return [out.detach()] + [t.grad for t in leaves]


def run(g, given, up):
    """the operator forward and backward on the device of `given`"""
    leaves = [t.clone().requires_grad_() for t in given]
    out = ops.lstm_aggregate(g, *leaves)
    (out * up).sum().backward()
    return [out.detach()] + [t.grad for t in leaves]


def check(got, ref64, ref32, label):
    for name, a, b, c in zip(NAMES, got, ref64, ref32):
        err, unit = float((a.cpu().double() - b).abs().max()), float((c.double() - b).abs().max())
        print("%s %s: err %.3e, fp32 restatement %.3e, ratio %.2f" % (label, name, err, unit, err / max(unit, 1e-30)))
        assert a.dtype == torch.float32 and a.shape == b.shape
        assert err <= 4 * unit + 1e-6, (label, name, err, unit)


@functools.lru_cache(maxsize=None)
def device_case(H, D, biases):
    """(graph, operands on the device, up, fp64 restatement, fp32 restatement, the fused results of two runs)"""
    g = mg.create_block(block_edges(), N_SRC, N_DST, idtype=torch.int32, device=DEV)
    given, up = operands(N_SRC, N_DST, H, D, biases)
    on_dev, up_dev = tuple(t.to(DEV) for t in given), up.to(DEV)
    refs = [restate(g._index.csc(), given, up, dtype) for dtype in (torch.float64, torch.float32)]
    return g, on_dev, up_dev, refs[0], refs[1], [run(g, on_dev, up_dev) for _ in range(2)]


@pytest.mark.gpu
@pytest.mark.parametrize("H,D,biases", CASES)
def test_fused_values_and_gradients(H, D, biases):
    g, given, _, ref64, ref32, runs = device_case(H, D, biases)
    assert ops.lstm_aggregate_fused(g, *given) is True
    check(runs[0], ref64, ref32, "H %d D %d%s" % (H, D, "" if biases else " no bias"))
    empty = (g.in_degrees() == 0).cpu()
    assert int(empty.sum()) == 1 and not runs[0][0].cpu()[empty].any()


@pytest.mark.gpu
@pytest.mark.parametrize("H,D,biases", CASES)
def test_a_rerun_is_bitwise_equal(H, D, biases):
    first, second = device_case(H, D, biases)[5]
    for name, a, b in zip(NAMES, first, second):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name


def rejected(g, x, w_ih, w_hh, *b):
    return {"w_hh_shape": (g, x, w_ih, w_hh[:, :-1]) + b, "x_3d": (g, x.unsqueeze(1), w_ih, w_hh) + b,
            "x_rows": (g, x[:-1], w_ih, w_hh) + b, "no_graph": (None, x, w_ih, w_hh) + b}


def check_rejected(g, given):
    for label, args in rejected(g, *given).items():
        assert ops.lstm_aggregate_fused(*args) is False, label
        with pytest.raises(mg.DGLError, match="^lstm_aggregate:"):
            ops.lstm_aggregate(*args)


@pytest.mark.gpu
def test_the_predicate_names_the_path(monkeypatch):
    g, given, up, ref64, ref32, runs = device_case(16, 16, True)
    backend, calls = type(sparse.backend_for(given[0])), []
    inner = backend.lstm_agg_fwd
    monkeypatch.setattr(backend, "lstm_agg_fwd", lambda self, *a: calls.append(1) or inner(self, *a))
    assert ops.lstm_aggregate_fused(g, *given) is True
    assert torch.equal(ops.lstm_aggregate(g, *given), runs[0][0]) and len(calls) == 1
    monkeypatch.setattr(config, "LSTM_AGG_FUSED", False)
    assert ops.lstm_aggregate_fused(g, *given) is False
    check(run(g, given, up), ref64, ref32, "composed")
    assert len(calls) == 1
    monkeypatch.setattr(config, "LSTM_AGG_FUSED", True)
    wide, _ = operands(N_SRC, N_DST, 80, 16, True)
    for label, other in (("H = 80", tuple(t.to(DEV) for t in wide)), ("float64", tuple(t.double() for t in given))):
        assert ops.lstm_aggregate_fused(g, *other) is False, label
        assert ops.lstm_aggregate(g, *other).shape == (N_DST, other[2].shape[1])
    assert len(calls) == 1
    check_rejected(g, given)


# ---- no GPU
SRC = torch.tensor([0, 1, 2, 3, 4, 0, 1, 2])
DST = torch.tensor([1, 2, 3, 0, 0, 2, 2, 1])


@pytest.fixture
def cpu_backend():
    was = mg.enable_cpu_backend(True)
    yield
    mg.enable_cpu_backend(was)


def test_composed_path_and_rejections_on_the_cpu(cpu_backend):
    g = mg.create_block((SRC, DST), 5, 4)  # row 3 of the destinations has one in-edge, none is empty but ...
    given, up = operands(5, 5, 4, 6, True)
    g5 = mg.graph((SRC, DST), num_nodes=5)  # ... here row 4 is
    for graph, rows in ((g, 4), (g5, 5)):
        refs = [restate(graph._index.csc(), given, up[:rows], dtype) for dtype in (torch.float64, torch.float32)]
        assert ops.lstm_aggregate_fused(graph, *given) is False
        check(run(graph, given, up[:rows]), refs[0], refs[1], "cpu %d rows" % rows)
    assert not ops.lstm_aggregate(g5, *given)[4].any()
    check_rejected(g5, given)


def test_sage_conv_lstm_layer(cpu_backend):
    torch.manual_seed(0)
    conv = dgl.nn.SAGEConv(6, 4, "lstm")
    assert sorted(conv.state_dict()) == sorted(["lstm.weight_ih_l0", "lstm.weight_hh_l0", "lstm.bias_ih_l0", "lstm.bias_hh_l0",
                                                "fc_self.weight", "fc_self.bias", "fc_neigh.weight", "fc_neigh.bias"])
    assert tuple(conv.lstm.weight_ih_l0.shape) == (24, 6) and tuple(conv.lstm.weight_hh_l0.shape) == (24, 6)
    g = mg.create_block((SRC, DST), 5, 4)
    x = torch.randn(5, 6)
    out = conv(g, x)
    given = (x,) + tuple(p.detach() for p in conv.lstm.parameters())
    neigh = restate(g._index.csc(), given, torch.zeros(4, 6), torch.float64)[0]
    want = conv.fc_self(x[:4]).double() + neigh @ conv.fc_neigh.weight.double().t() + conv.fc_neigh.bias.double()
    assert torch.allclose(out.double(), want, rtol=1e-5, atol=1e-6)
    out.sum().backward()
    assert all(p.grad is not None and bool(p.grad.abs().sum() > 0) for p in conv.parameters())
    with pytest.raises(mg.DGLError, match="mean, gcn, pool, lstm"):
        dgl.nn.SAGEConv(6, 4, "median")
