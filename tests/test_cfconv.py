"""Continuous-filter convolution: ops.edge_filter_sum (csrc/cfconv.hip) and nn.CFConv against one plain-torch restatement (gather, two
linears, F.softplus - ln 2, multiply, index_add), gradients by autograd of sum(out * up).

The bound is measured, not derived (exp and log1p sit between the sums): the restatement runs in fp64 and in fp32 on the CPU and every
tensor may be off by |got - ref64| <= 4 * max|ref32 - ref64| + 1e-6 -- tests/test_lstm_aggregate.py's rule, the factor 4 for a different
summation order and the device's exp and log being a few ulp off libm.  The tests print the ratios (docs/LOG_cfconv.md has the observed
ones).  Operands are randn and the weights nn.Linear's draws: a lost or doubled edge moves a result by orders of magnitude more.

Graph: in-degrees 0, 1, 15, 16, 17, U - 1, U, U + 1, 3 U + 5, 0 with U = config.CFCONV_ITEM_EDGES -- tile and item boundaries inside and
between rows, a row over four items -- sources over all nodes, one source read twice in a row, shuffled edge ids; and one edge on two nodes."""
import copy
import functools
import math

import pytest
import torch

import dgl
import mi355x_graph as mg
from mi355x_graph import config, nn as mnn, ops, sparse
import oracle_backend

DEV = "cuda:0"
U = config.CFCONV_ITEM_EDGES
DEGREES = {"boundaries": [0, 1, 15, 16, 17, U - 1, U, U + 1, 3 * U + 5, 0], "one_edge": [0, 1]}
NAMES = ("out", "d x", "d w1", "d b1", "d w2", "d b2")
SHAPES = [(16, 5), (48, 20), (64, 50), (128, 64), (128, 128)]


@functools.lru_cache(maxsize=None)
def edges(kind):
    gen = torch.Generator().manual_seed(11)
    deg = torch.tensor(DEGREES[kind])
    dst = torch.repeat_interleave(torch.arange(len(deg)), deg)
    src = torch.randint(0, len(deg), (len(dst),), generator=gen)
    src[1:3] = 0  # the row of 15 reads one source twice in a row
    order = torch.randperm(len(dst), generator=gen)
    return src[order], dst[order], len(deg)


def graph(kind, dev, idtype=torch.int32):
    src, dst, n = edges(kind)
    g = mg.graph((src, dst), num_nodes=n)
    return (g.int() if idtype == torch.int32 else g.long()).to(dev)


@functools.lru_cache(maxsize=None)
def operands(kind, F, K, mode, biases=True, scale=1.0):
    """(x, ef, w1, b1, w2, b2), rbf, up: fp32 on the host"""
    src, dst, n = edges(kind)
    torch.manual_seed(F + 3 * K)
    l1, l2 = torch.nn.Linear(K, F, bias=biases), torch.nn.Linear(F, F, bias=biases)
    gen = torch.Generator().manual_seed(3)
    x, up = torch.randn(n, F, generator=gen), torch.randn(n, F, generator=gen)
    rbf = (torch.arange(K) * (5.0 / K), K / 5.0) if mode == "rbf" else None
    ef = 5 * torch.rand(len(src), generator=gen) if rbf else scale * torch.randn(len(src), K, generator=gen)
    return (x, ef) + tuple(None if p is None else p.detach() for p in (l1.weight, l1.bias, l2.weight, l2.bias)), rbf, up


def restate(kind, given, rbf, up, reduce, dtype):
    src, dst, n = edges(kind)
    x, ef, w1, b1, w2, b2 = (None if t is None else t.detach().cpu().to(dtype).requires_grad_() for t in given)
    a = ef if rbf is None else torch.exp(-rbf[1] * (ef.view(-1, 1) - rbf[0].to(dtype).view(1, -1)) ** 2)
    lin, ssp = torch.nn.functional.linear, lambda t: torch.nn.functional.softplus(t) - math.log(2)
    out = torch.zeros(n, x.shape[1], dtype=dtype).index_add(0, dst, x[src] * ssp(lin(ssp(lin(a, w1, b1)), w2, b2)))
    if reduce == "mean":
        out = out / torch.bincount(dst, minlength=n).clamp(min=1).to(dtype).view(-1, 1)
    (out * up.to(dtype)).sum().backward()
    return [out.detach()] + [None if t is None else t.grad for t in (x, w1, b1, w2, b2)]


@functools.lru_cache(maxsize=None)
def references(kind, F, K, mode, reduce, biases=True, scale=1.0):
    given, rbf, up = operands(kind, F, K, mode, biases, scale)
    return [restate(kind, given, rbf, up, reduce, dtype) for dtype in (torch.float64, torch.float32)]


def run(g, given, rbf, up, reduce, dev):
    x, ef, w1, b1, w2, b2 = (None if t is None else t.clone().to(dev) for t in given)
    leaves = [t.requires_grad_() for t in (x, w1, b1, w2, b2) if t is not None]
    rbf = None if rbf is None else (rbf[0].to(dev), rbf[1])
    out = ops.edge_filter_sum(g, x, ef, w1, b1, w2, b2, rbf, reduce)
    (out * up.to(dev)).sum().backward()
    assert ef.grad is None
    return [out.detach()] + [None if t is None else t.grad for t in (x, w1, b1, w2, b2)]


def check(got, ref64, ref32, label):
    for name, a, b, c in zip(NAMES, got, ref64, ref32):
        if b is None:
            assert a is None
            continue
        err, unit = float((a.cpu().double() - b).abs().max()), float((c.double() - b).abs().max())
        print("%s %s: err %.3e, fp32 restatement %.3e, ratio %.2f" % (label, name, err, unit, err / max(unit, 1e-30)))
        assert a.dtype == torch.float32 and a.shape == b.shape and bool(torch.isfinite(a).all())
        assert err <= 4 * unit + 1e-6, (label, name, err, unit)


def case(kind, F, K, mode, reduce, dev, biases=True, scale=1.0, idtype=torch.int32, fused=True):
    g = graph(kind, dev, idtype)
    given, rbf, up = operands(kind, F, K, mode, biases, scale)
    on_dev = [None if t is None else t.to(dev) for t in given]
    assert ops.edge_filter_sum_fused(g, *on_dev, rbf=None if rbf is None else (rbf[0].to(dev), rbf[1]), reduce=reduce) is fused
    got = run(g, given, rbf, up, reduce, dev)
    check(got, *references(kind, F, K, mode, reduce, biases, scale), "%s F %d K %d %s %s" % (kind, F, K, mode, reduce))
    assert not got[0].cpu()[torch.tensor(DEGREES[kind]) == 0].any()  # rows without in-edges: exactly 0
    return g, got


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["tensor", "rbf"])
@pytest.mark.parametrize("reduce", ["sum", "mean"])
@pytest.mark.parametrize("F,K", SHAPES)
def test_values_and_gradients(F, K, reduce, mode):
    case("boundaries", F, K, mode, reduce, DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,F,K,biases,scale", [("boundaries", 48, 20, False, 1.0), ("one_edge", 16, 5, True, 1.0), ("boundaries", 64, 50, True, 40.0)],
                         ids=["no_biases", "one_edge", "wide_range"])
def test_no_biases_one_edge_and_wide_range(kind, F, K, biases, scale):
    if scale > 1:  # both pre-activations cross +-20: softplus's threshold and the -ln 2 floor
        (x, ef, w1, b1, w2, b2), _, _ = operands(kind, F, K, "tensor", biases, scale)
        pre1 = ef @ w1.t() + b1
        pre2 = (torch.nn.functional.softplus(pre1) - math.log(2)) @ w2.t() + b2
        assert all(float(p.min()) < -20 and float(p.max()) > 20 for p in (pre1, pre2))
    g, got = case(kind, F, K, "tensor", "sum", DEV, biases, scale)
    given, rbf, up = operands(kind, F, K, "tensor", biases, scale)
    again = run(g, given, rbf, up, "sum", DEV)
    assert all(a is b is None or torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got, again))  # a rerun: the same bits


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["fused", "F=24", "F=144", "int64", "config"])
def test_fallbacks_and_the_predicate(which, monkeypatch):
    backend, calls = type(sparse.backend_for(torch.zeros(1, device=DEV))), []
    inner = backend.edge_filter_sum
    monkeypatch.setattr(backend, "edge_filter_sum", lambda self, *a: calls.append(1) or inner(self, *a))
    if which == "config":
        monkeypatch.setattr(config, "CFCONV_FUSED", False)
    F = {"F=24": 24, "F=144": 144}.get(which, 16)
    g = graph("boundaries", DEV, torch.int64 if which == "int64" else torch.int32)
    given, rbf, _ = operands("boundaries", F, 5, "rbf")
    with torch.no_grad():
        ops.edge_filter_sum(g, *(t.to(DEV) for t in given), rbf=(rbf[0].to(DEV), rbf[1]))
    assert len(calls) == (1 if which == "fused" else 0)
    case("boundaries", F, 5, "rbf", "mean", DEV, idtype=torch.int64 if which == "int64" else torch.int32, fused=which == "fused")


def layer_results(conv, kind, feats, efeats, up, dtype, dev):
    """[out, the gradients of the layer's parameters]: the layer itself, or (dev None) its restatement in `dtype` on the host"""
    src, dst, n = edges(kind)
    conv = conv if dev else copy.deepcopy(conv).cpu().to(dtype)
    conv.zero_grad()
    if dev:
        out = conv(graph(kind, dev), feats.to(dev), efeats.to(dev))
    else:
        a = efeats.to(dtype)
        if conv._gamma is not None:
            a = torch.exp(-conv._gamma * (a.view(-1, 1) - conv.centers.to(dtype).view(1, -1)) ** 2)
        m = conv.project_node(feats.to(dtype))[src] * conv.project_edge(a)
        out = conv.project_out(torch.zeros(n, m.shape[1], dtype=dtype).index_add(0, dst, m))
    (out * up.to(out)).sum().backward()
    return [out.detach()] + [p.grad for p in conv.parameters()]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["tensor", "rbf"])
def test_cfconv_layer(mode):
    torch.manual_seed(1)
    conv = dgl.nn.CFConv(12, 20, 32, 8, rbf=(0.0, 5.0, 0.25) if mode == "rbf" else None)
    src, dst, n = edges("boundaries")
    feats, up = torch.randn(n, 12), torch.randn(n, 8)
    efeats = 5 * torch.rand(len(src)) if mode == "rbf" else torch.randn(len(src), 20)
    ref64, ref32 = (layer_results(conv, "boundaries", feats, efeats, up, dtype, None) for dtype in (torch.float64, torch.float32))
    got = layer_results(conv.to(DEV), "boundaries", feats, efeats, up, None, DEV)
    names = ["out"] + ["d " + k for k, _ in conv.named_parameters()]
    assert names[1:] == ["d project_edge.0.weight", "d project_edge.0.bias", "d project_edge.2.weight", "d project_edge.2.bias",
                         "d project_node.weight", "d project_node.bias", "d project_out.0.weight", "d project_out.0.bias"]
    for name, a, b, c in zip(names, got, ref64, ref32):
        err, unit = float((a.cpu().double() - b).abs().max()), float((c.double() - b).abs().max())
        print("layer %s %s: err %.3e, fp32 restatement %.3e, ratio %.2f" % (mode, name, err, unit, err / max(unit, 1e-30)))
        assert err <= 4 * unit + 1e-6, (name, err, unit)


# ---- no GPU
@pytest.fixture
def checker():
    oracle_backend.install()
    yield
    oracle_backend.uninstall()


@pytest.mark.parametrize("mode", ["tensor", "rbf"])
@pytest.mark.parametrize("reduce", ["sum", "mean"])
def test_composition_on_the_cpu(checker, reduce, mode):
    case("boundaries", 7, 5, mode, reduce, "cpu", fused=False)


def test_rejected_operands_and_names(checker):
    g = graph("boundaries", "cpu")
    (x, ef, w1, b1, w2, b2), _, _ = operands("boundaries", 16, 5, "tensor")
    cen = torch.arange(5.0)
    rejected = {"x_3d": (g, x.unsqueeze(1), ef, w1, b1, w2, b2), "ef_rows": (g, x, ef[:-1], w1, b1, w2, b2), "w2_shape": (g, x, ef, w1, b1, w2[:, :-1], b2),
                "float64": (g, x.double(), ef, w1, b1, w2, b2), "reduce": (g, x, ef, w1, b1, w2, b2, None, "max"), "bias": (g, x, ef, w1, b1[:-1], w2, b2),
                "rbf_form": (g, x, ef[:, 0], w1, b1, w2, b2, (cen,)), "rbf_count": (g, x, ef[:, 0], w1, b1, w2, b2, (cen[:-1], 1.0)),
                "no_graph": (None, x, ef, w1, b1, w2, b2)}
    for label, args in rejected.items():
        assert ops.edge_filter_sum_fused(*args) is False, label
        with pytest.raises(mg.DGLError, match="edge_filter_sum"):
            ops.edge_filter_sum(*args)
    assert {"edge_filter_sum", "edge_filter_sum_fused"} <= set(ops.__all__) and config.CFCONV_FUSED is True and U % 16 == 0
    assert dgl.nn.CFConv is mnn.CFConv and dgl.nn.pytorch.conv.CFConv is mnn.CFConv
