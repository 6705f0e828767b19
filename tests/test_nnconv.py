"""Edge-conditioned convolution: ops.edge_bilinear (csrc/nnconv.hip), nn.NNConv and graph_classification.MPNN against one fp64
restatement in plain torch: W_e = h @ Theta + B, m_e = x[src] W_e, index_add by destination, gradients by fp64 autograd of sum(out * g).

Bound of the random-value tests, per element: |got - ref| <= (T + 4) * 2^-24 * sum |terms|, T the number of terms of that element's sum
((DH + 1) * I per in-edge for out, (DH + 1) * O per out-edge for d x, I * O for d h, E for d Theta and d B) and sum |terms| the
restatement run on absolute values.  It is the fp32 running-sum bound of tests/test_segment_mm.py, which holds for every summation
order, with two more units for the rounding of the product h * x formed on the fly and of the mean's division.  The integer tests make
every fp32 sum exact: results must be torch.equal to the fp64 ones, so one lost or doubled edge at a tile, item or row boundary shows."""
import functools
import os
import sys

import pytest
import torch

import mi355x_graph as mg
from mi355x_graph import config, nn as mnn, ops
import oracle_backend

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dgl-0.5-benchmark_amd")
DEV = "cuda:0"
U = config.NNCONV_ITEM_EDGES
DEGREES = {"boundaries": [0, 1, 15, 16, 17, U - 1, U, U + 1, 3 * U + 5, 0], "one_edge": [0, 1]}
SHAPES = [(7, 5, 3), (16, 32, 1), (64, 64, 8), (128, 128, 2), (16, 16, 130)]


@functools.lru_cache(maxsize=None)
def edges(kind):
    """(src, dst, n): the in-degrees of DEGREES[kind], sources drawn over all nodes, edge ids in a random order"""
    gen = torch.Generator().manual_seed(11)
    deg = torch.tensor(DEGREES[kind])
    dst = torch.repeat_interleave(torch.arange(len(deg)), deg)
    order = torch.randperm(len(dst), generator=gen)
    return torch.randint(0, len(deg), (len(dst),), generator=gen)[order], dst[order], len(deg)


def graph(kind, dev, idtype=torch.int32):
    src, dst, n = edges(kind)
    g = mg.graph((src, dst), num_nodes=n)
    return (g.int() if idtype == torch.int32 else g.long()).to(dev)


@functools.lru_cache(maxsize=None)
def operands(kind, I, O, DH, integer, n_src=None):
    src, dst, n = edges(kind)
    gen = torch.Generator().manual_seed(I + 3 * O + 7 * DH)
    draw = (lambda *s: torch.randint(-2, 3, s, generator=gen).float()) if integer else (lambda *s: torch.randn(*s, generator=gen))
    return draw(n_src or n, I), draw(len(src), DH), draw(DH, I, O), draw(I, O), draw(n, O)


def restate(src, dst, n_dst, x, h, theta, bias, g, reduce):
    """(out, d x, d h, d theta, d bias) in fp64"""
    x, h, theta, bias = (t.detach().double().cpu().requires_grad_(True) for t in (x, h, theta, bias))
    DH, I, O = theta.shape
    w_e = (h @ theta.reshape(DH, I * O) + bias.reshape(1, I * O)).view(-1, I, O)
    out = torch.zeros(n_dst, O, dtype=torch.float64).index_add(0, dst, torch.einsum("ei,eio->eo", x[src], w_e))
    if reduce == "mean":
        out = out / torch.bincount(dst, minlength=n_dst).clamp(min=1).double().view(-1, 1)
    return (out.detach(),) + torch.autograd.grad((out * g.double().cpu()).sum(), (x, h, theta, bias))


@functools.lru_cache(maxsize=None)
def reference(kind, I, O, DH, integer, reduce, with_bias):
    """(values, magnitudes, term counts) of the five results for the shared operands of a case"""
    src, dst, n = edges(kind)
    x, h, theta, bias, g = operands(kind, I, O, DH, integer)
    if not with_bias:
        bias = torch.zeros_like(bias)
    ref = restate(src, dst, n, x, h, theta, bias, g, reduce)
    mag = restate(src, dst, n, x.abs(), h.abs(), theta.abs(), bias.abs(), g.abs(), reduce)
    E = len(src)
    terms = (torch.bincount(dst, minlength=n).double().view(-1, 1) * (DH + 1) * I,
             torch.bincount(src, minlength=n).double().view(-1, 1) * (DH + 1) * O, I * O, E, E)
    return ref, mag, terms


def run(g, x, h, theta, bias, up, reduce, dev, h_grad=True):
    x, theta = (t.clone().to(dev).requires_grad_(True) for t in (x, theta))
    h = h.clone().to(dev).requires_grad_(h_grad)
    bias = None if bias is None else bias.clone().to(dev).requires_grad_(True)
    out = ops.edge_bilinear(g, x, h, theta, bias, reduce)
    (out * up.to(dev)).sum().backward()
    return out, x.grad, h.grad, theta.grad, None if bias is None else bias.grad


def check(got, ref, mag, terms, integer=False):
    for name, x, want, m, t in zip(("out", "d x", "d h", "d theta", "d bias"), got, ref, mag, terms):
        if x is None:
            continue
        if integer:
            assert float(m.max()) < 2 ** 24 and torch.equal(x.detach().double().cpu(), want), name
            continue
        err, bound = (x.detach().double().cpu() - want).abs(), (t + 4) * 2.0 ** -24 * m
        print("%s: max error %.3g, max of the bound %.3g" % (name, float(err.max()), float(bound.max())))
        assert bool((err <= bound).all()), name


def case(kind, I, O, DH, integer, reduce, with_bias, dev, idtype=torch.int32, fused=True):
    g = graph(kind, dev, idtype)
    x, h, theta, bias, up = operands(kind, I, O, DH, integer)
    bias = bias if with_bias else None
    on_dev = [None if t is None else t.to(dev) for t in (x, h, theta, bias)]
    assert ops.edge_bilinear_fused(g, *on_dev, reduce=reduce) is fused
    got = run(g, x, h, theta, bias, up, reduce, dev)
    check(got, *reference(kind, I, O, DH, integer, reduce, with_bias), integer=integer)
    return g, got


@pytest.mark.gpu
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("reduce", ["sum", "mean"])
@pytest.mark.parametrize("I,O,DH", SHAPES)
def test_values_and_gradients(I, O, DH, reduce, with_bias):
    case("boundaries", I, O, DH, False, reduce, with_bias, DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("I,O,DH", [(16, 16, 3), (64, 64, 8)])
@pytest.mark.parametrize("kind", ["boundaries", "one_edge"])
def test_exact_structure(kind, I, O, DH):
    g, got = case(kind, I, O, DH, True, "sum", True, DEV)
    x, h, theta, bias, up = operands(kind, I, O, DH, True)
    again = run(g, x, h, theta, bias, up, "sum", DEV)
    assert all(torch.equal(a, b) for a, b in zip(got, again))                      # fixed summation order: the same bits


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["column_block", "odd_offset", "block", "no_d_h"])
def test_layouts_and_selective_gradients(layout):
    I, O, DH = 16, 24, 5
    src, dst, n = edges("boundaries")
    n_src = n + 4 if layout == "block" else n
    x, h, theta, bias, up = operands("boundaries", I, O, DH, True, n_src=n_src)
    g = mg.create_block((src, dst), n_src, n, idtype=torch.int32, device=DEV) if layout == "block" else graph("boundaries", DEV)
    xd, hd = x.to(DEV), h.to(DEV)
    if layout == "column_block":
        xd = torch.zeros(n_src, I + 8, device=DEV)[:, 4:4 + I].copy_(x)
    if layout == "odd_offset":                                                      # h is read a dword at a time: taken where it lies
        hd = torch.zeros(len(src) * DH + 1, device=DEV)[1:].view(len(src), DH).copy_(h)
        assert hd.data_ptr() % 16 == 4
    assert ops.edge_bilinear_fused(g, xd, hd, theta.to(DEV), bias.to(DEV)) is True
    xd, hd = xd.requires_grad_(True), hd.requires_grad_(layout != "no_d_h")
    th, b = theta.to(DEV).requires_grad_(True), bias.to(DEV).requires_grad_(True)
    out = ops.edge_bilinear(g, xd, hd, th, b)
    assert tuple(out.shape) == (n, O)
    (out * up.to(DEV)).sum().backward()
    assert (hd.grad is None) == (layout == "no_d_h")
    ref = restate(src, dst, n, x, h, theta, bias, up, "sum")
    for got, want in zip((out, xd.grad, hd.grad, th.grad, b.grad), ref):
        assert got is None or torch.equal(got.double().cpu(), want)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["I=129", "int64", "config"])
def test_fallbacks_on_the_device(which, monkeypatch):
    if which == "config":
        monkeypatch.setattr(config, "NNCONV_FUSED", False)
    I = 129 if which == "I=129" else 16
    case("boundaries", I, 16, 3, False, "mean", True, DEV, idtype=torch.int64 if which == "int64" else torch.int32, fused=False)


@pytest.fixture
def checker():
    oracle_backend.install()
    yield
    oracle_backend.uninstall()


@pytest.mark.parametrize("reduce", ["sum", "mean"])
def test_composition_and_its_gradients_on_the_cpu(checker, reduce):
    case("boundaries", 7, 5, 3, False, reduce, True, "cpu", fused=False)


@pytest.mark.parametrize("edge_net", ["sequential", "linear", "other"])
@pytest.mark.parametrize("aggr", ["sum", "mean", "max"])
def test_nnconv_layer_equals_dgl_restated(checker, edge_net, aggr):
    I, O, D = 6, 4, 3
    src, dst, n = edges("boundaries")
    torch.manual_seed(5)
    last = torch.nn.Linear(8, I * O)
    net = {"sequential": torch.nn.Sequential(torch.nn.Linear(D, 8), torch.nn.ReLU(), last), "linear": torch.nn.Linear(D, I * O),
           "other": torch.nn.Sequential(torch.nn.Linear(D, I * O), torch.nn.Tanh())}[edge_net]
    conv = mnn.NNConv(I, O, net, aggr, residual=True, bias=True)
    assert {k.split(".")[0] for k in conv.state_dict()} == {"edge_func", "bias", "res_fc"} and "res_fc.weight" in conv.state_dict()
    assert (conv._last_linear() is None) == (edge_net == "other")
    with torch.no_grad():
        conv.bias.add_(0.1 * torch.randn(O))
    feat, efeat = torch.randn(n, I), torch.randn(len(src), D)
    out = conv(graph("boundaries", "cpu"), feat, efeat)
    with torch.no_grad():
        ref64 = conv.double()
        w = ref64.edge_func(efeat.double()).view(-1, I, O)
        m = feat.double()[src].unsqueeze(-1) * w                                    # u_mul_e: [E, I, O]
        idx = dst.view(-1, 1, 1).expand_as(m)
        zero = torch.zeros(n, I, O, dtype=torch.float64)
        red = {"sum": lambda: zero.index_add(0, dst, m), "mean": lambda: zero.scatter_reduce(0, idx, m, "mean", include_self=False),
               "max": lambda: zero.scatter_reduce(0, idx, m, "amax", include_self=False)}[aggr]()
        want = red.sum(1) + ref64.res_fc(feat.double()) + ref64.bias
    err = float((out.detach().double() - want).abs().max())
    assert err <= 1e-5 * float(want.abs().max()), err                               # ~100 fp32 roundings of values of order 1
    import dgl.nn.pytorch as dglnn
    assert dglnn.NNConv is mnn.NNConv and dglnn.conv.NNConv is mnn.NNConv and config.NNCONV_FUSED is True


@pytest.mark.gpu
def test_mpnn_model_fused_on_and_off(monkeypatch):
    """Three optimiser steps from one seed with the kernels on and off.  A loss is a mean of B terms, each behind sums of about
    T = steps * (DH + 1) * I * deg terms (deg <= 6); test 1's bound for such a sum is (T + 4) * 2^-24 relative to its magnitudes.  The two paths
    differ by at most twice that per forward, the update of step s feeds it back s times, and magnitudes exceed values by the
    cancellation of the model (taken as 2^4): tolerance 2 * 3 * 2^4 * (T + 4) * 2^-24 of the loss."""
    sys.path.insert(0, PKG)
    import graph_classification as gc
    losses = []
    for fused in (True, False):
        monkeypatch.setattr(config, "NNCONV_FUSED", fused)
        losses.append(gc.mpnn_smoke_losses(steps=3, device=DEV, seed=4))
    T = gc.MPNN.STEPS * (gc.MPNN.EDGE_HIDDEN + 1) * 16 * 6                  # width 16, at most 6 bonds per atom
    tol = 2 * 3 * 2 ** 4 * (T + 4) * 2.0 ** -24
    print("fused %r, composed %r, tolerance %.3g (relative)" % (losses[0], losses[1], tol))
    assert all(abs(a - b) <= tol * abs(b) for a, b in zip(*losses))
