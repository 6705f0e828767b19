"""ops.edge_mlp_reduce (csrc/edgemlp.hip) and the 2- and 3-layer nn.PointNetConv against one plain-torch restatement: gather, subtract,
ReLU, (Linear, ReLU) per layer, then the reduce on the [row, position] layout -- index_add for sum, for max torch.argmax over the positions
(its documented rule: the FIRST maximal value) and a gather, so the gradient goes through that position only.

Graph: in-degrees 0, 1, 15, 16, 17, U - 1, U, U + 1, 3 U + 5, 0 with U = config.EDGE_MLP_ITEM_EDGES patched to 32 -- empty rows, tile and
item boundaries inside and between rows, a row over four items -- shuffled edge ids; the last edge of every row of two or more repeats the
row's first source, so every such row has tied maxima.
Exact cases: small integers and sparse weights, every intermediate of the fp64 restatement below 2^24 (asserted on it alone), so fp32 sums
in any order are exact and the results must be bit-equal.  Float cases: tests/test_cfconv.py's rule, |got - ref64| <= 4 * max|ref32 - ref64|
+ 1e-6 per tensor; under max only `out` is compared (a near-tie may pick another arg in fp32)."""
import functools

import pytest
import torch

import dgl
import mi355x_graph as mg
from mi355x_graph import config, ops, sparse
import oracle_backend
import test_ball_query as tbq

DEV = "cuda:0"
U = 32
DEGREES = [0, 1, 15, 16, 17, U - 1, U, U + 1, 3 * U + 5, 0]
WIDTHS = [(16, (16,)), (32, (16, 48)), (64, (64, 128)), (128, (128, 256))]  # the last: two slabs of the output columns


@pytest.fixture(autouse=True)
def short_items(monkeypatch):
    monkeypatch.setattr(config, "EDGE_MLP_ITEM_EDGES", U)


@functools.lru_cache(maxsize=None)
def edges():
    gen = torch.Generator().manual_seed(11)
    deg = torch.tensor(DEGREES)
    dst = torch.repeat_interleave(torch.arange(len(deg)), deg)
    src = torch.randint(0, len(deg), (len(dst),), generator=gen)
    ends = torch.cumsum(deg, 0)
    for first, end in zip((ends - deg).tolist(), ends.tolist()):
        if end - first >= 2:
            src[end - 1] = src[first]
    order = torch.randperm(len(dst), generator=gen)  # (a stable sort by destination keeps a row's order)
    return src[order], dst[order], len(deg)


def graph(dev, idtype=torch.int32):
    src, dst, n = edges()
    g = mg.graph((src, dst), num_nodes=n)
    return (g.int() if idtype == torch.int32 else g.long()).to(dev)


@functools.lru_cache(maxsize=None)
def data(H0, hidden, exact):
    """u, v, weights, biases (None at H0 = 16), upstream gradient: fp32 on the host"""
    n, gen = len(DEGREES), torch.Generator().manual_seed(H0 + sum(hidden))
    if exact:
        ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=gen).float()
        draw, weight = lambda *shape: ri(-2, 2, *shape), lambda o, i: ri(-1, 1, o, i) * (torch.rand(o, i, generator=gen) < 0.2)
    else:
        draw, weight = lambda *shape: torch.randn(shape, generator=gen), lambda o, i: torch.randn(o, i, generator=gen) / i ** 0.5
    ws = [weight(o, i) for i, o in zip((H0,) + hidden[:-1], hidden)]
    bs = [None if H0 == 16 else draw(o) for o in hidden]
    return draw(n, H0), draw(n, H0), ws, bs, draw(n, hidden[-1])


def restate(case, reduce, dtype, g):
    """([out, d u, d v, d W.., d b..], the largest magnitude met) in `dtype` on the host, over the graph's in-CSR order"""
    csc = g._index.csc()
    indptr, col = csc.indptr.cpu().long(), csc.indices.cpu().long()
    u, v, ws, bs, up = case
    u, v = (t.clone().to(dtype).requires_grad_() for t in (u, v))
    ws, bs = [w.clone().to(dtype).requires_grad_() for w in ws], [None if b is None else b.clone().to(dtype).requires_grad_() for b in bs]
    deg = indptr[1:] - indptr[:-1]
    row = torch.repeat_interleave(torch.arange(len(deg)), deg)
    seen = [torch.relu(u[col] - v[row])]
    for w, b in zip(ws, bs):
        seen.append(torch.relu(torch.nn.functional.linear(seen[-1], w, b)))
    e = seen[-1]
    if reduce == "sum":
        out = torch.zeros(len(deg), e.shape[1], dtype=dtype).index_add(0, row, e)
    else:
        pad = torch.full((len(deg), int(deg.max()), e.shape[1]), -float("inf"), dtype=dtype)
        pad = pad.index_put((row, torch.arange(len(row)) - indptr[row]), e)
        out = torch.where((deg > 0).view(-1, 1), pad.gather(1, pad.detach().argmax(1, keepdim=True))[:, 0], pad.new_zeros(()))
    (out * up.to(dtype)).sum().backward()
    res = [out.detach()] + [None if t is None else t.grad for t in [u, v] + ws + bs]
    return res, max(float(t.detach().abs().max()) for t in seen + res if t is not None)


def run(g, case, reduce, dev, u_view=None):
    u, v, ws, bs, up = case
    u, v = (t.clone().to(dev).requires_grad_() for t in (u, v))
    ws, bs = [w.clone().to(dev).requires_grad_() for w in ws], [None if b is None else b.clone().to(dev).requires_grad_() for b in bs]
    out = ops.edge_mlp_reduce(g, u if u_view is None else u_view(u), v, ws, bs, reduce)
    (out * up.to(dev)).sum().backward()
    return [out.detach().cpu()] + [None if t is None else t.grad.cpu() for t in [u, v] + ws + bs]


def same_bits(xs, ys):
    return all(a is b is None or (a.dtype == torch.float32 and torch.equal(a.double(), b.double())) for a, b in zip(xs, ys))


@pytest.mark.gpu
@pytest.mark.parametrize("reduce", ["max", "sum"])
@pytest.mark.parametrize("H0,hidden", WIDTHS)
def test_integer_data_bit_equal_to_fp64(H0, hidden, reduce):
    g, case = graph(DEV), data(H0, hidden, True)
    ref, peak = restate(case, reduce, torch.float64, g)
    assert peak < 2 ** 24 and bool((ref[0] > 0).any()) and all(t is None or bool(t.any()) for t in ref)
    assert ops.edge_mlp_reduce_fused(g, *(t.to(DEV) for t in case[:2]), [w.to(DEV) for w in case[2]], None, reduce) is True
    got = run(g, case, reduce, DEV)
    for i, (a, b) in enumerate(zip(got, ref)):
        assert a is b is None or torch.equal(a.double(), b), (i, float((a.double() - b).abs().max()))
    assert same_bits(got, run(g, case, reduce, DEV))  # a rerun: the same bits


@pytest.mark.gpu
@pytest.mark.parametrize("reduce", ["max", "sum"])
@pytest.mark.parametrize("H0,hidden", WIDTHS)
def test_float_data_within_the_fp32_restatements_error(H0, hidden, reduce):
    g, case = graph(DEV), data(H0, hidden, False)
    (ref64, _), (ref32, _) = (restate(case, reduce, dtype, g) for dtype in (torch.float64, torch.float32))
    got = run(g, case, reduce, DEV)
    assert not got[0][torch.tensor(DEGREES) == 0].any()  # rows without in-edges: exactly 0
    for i, (a, b, c) in enumerate(list(zip(got, ref64, ref32))[:1 if reduce == "max" else None]):
        if b is not None:
            err, unit = float((a.double() - b).abs().max()), float((c.double() - b).abs().max())
            print("%s %s %s tensor %d: err %.3e, fp32 restatement %.3e" % (H0, hidden, reduce, i, err, unit))
            assert a.dtype == torch.float32 and bool(torch.isfinite(a).all()) and err <= 4 * unit + 1e-6, (i, err, unit)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["fused", "H0=24", "HL=272", "int64", "config", "offset"])
def test_path_and_fallbacks(which, monkeypatch):
    backend, calls = type(sparse.backend_for(torch.zeros(1, device=DEV))), []
    inner = backend.edge_mlp_reduce
    monkeypatch.setattr(backend, "edge_mlp_reduce", lambda self, *a: calls.append(1) or inner(self, *a))
    H0, hidden = {"H0=24": (24, (16,)), "HL=272": (32, (16, 272))}.get(which, (32, (16, 48)))
    g, case = graph(DEV, torch.int64 if which == "int64" else torch.int32), data(H0, hidden, True)
    offset = (lambda u: torch.cat([u.new_zeros(1), u.flatten()])[1:].view_as(u)) if which == "offset" else None  # 4 bytes into its storage
    u, v = (t.to(DEV) for t in case[:2])
    with monkeypatch.context() as m:
        if which == "config":
            m.setattr(config, "EDGE_MLP_FUSED", False)
        fused = ops.edge_mlp_reduce_fused(g, u if offset is None else offset(u), v, [w.to(DEV) for w in case[2]], None, "max")
        got = run(g, case, "max", DEV, offset)
    assert fused is (which == "fused") and len(calls) == (1 if fused else 0)
    monkeypatch.setattr(config, "EDGE_MLP_FUSED", False)
    assert same_bits(got, run(g, case, "max", DEV)) and len(calls) == (1 if fused else 0)  # the composition: the same values


@pytest.mark.gpu
@pytest.mark.parametrize("in_feats,sizes", [(5, (16, 32)), (0, (16, 16, 32))])
def test_pointnetconv_layers_take_the_fused_path(in_feats, sizes, monkeypatch):
    backend, calls = type(sparse.backend_for(torch.zeros(1, device=DEV))), []
    inner = backend.edge_mlp_reduce
    monkeypatch.setattr(backend, "edge_mlp_reduce", lambda self, *a: calls.append(1) or inner(self, *a))
    pos = tbq.conv_block_host()[0]
    gen = torch.Generator().manual_seed(in_feats)
    ri = lambda *shape: torch.randint(-2, 3, shape, generator=gen).float()
    h = ri(pos.shape[0], in_feats) if in_feats else None
    params = [t for i, o in zip((in_feats + 3,) + sizes[:-1], sizes) for t in (ri(o, i) * (torch.rand(o, i, generator=gen) < 0.3), ri(o))]
    w = ri(len(tbq.CONV_LENS) * tbq.CONV_PER, sizes[-1])
    on = tbq.conv_run(in_feats, sizes, h, pos, params, w, DEV, True, monkeypatch)
    assert len(calls) == 1
    off = tbq.conv_run(in_feats, sizes, h, pos, params, w, DEV, False, monkeypatch)
    assert len(calls) == 1 and bool((on[0] > 0).any()) and same_bits([on[0]] + on[1], [off[0]] + off[1])


# ---- no GPU
@pytest.fixture
def checker():
    oracle_backend.install()
    yield
    oracle_backend.uninstall()


@pytest.mark.parametrize("reduce", ["max", "sum"])
def test_composition_on_the_cpu(checker, reduce):
    g, case = graph("cpu"), data(7, (5, 3), True)
    assert ops.edge_mlp_reduce_fused(g, case[0], case[1], case[2], case[3], reduce) is False
    ref, peak = restate(case, reduce, torch.float64, g)
    assert peak < 2 ** 24 and same_bits(run(g, case, reduce, "cpu"), ref)


def test_rejected_operands_and_names(checker):
    g, (u, v, ws, bs, _) = graph("cpu"), data(7, (5, 3), True)
    for args in ((g, u, v[:, :-1], ws, bs), (g, u, v, [ws[0], ws[1][:, :-1]], bs), (g, u, v, [], []), (g, u, v, ws, bs, "mean"), (g, u, v, ws, bs[:1])):
        assert ops.edge_mlp_reduce_fused(*args) is False
        with pytest.raises(mg.DGLError, match="edge_mlp_reduce"):
            ops.edge_mlp_reduce(*args)
    assert {"edge_mlp_reduce", "edge_mlp_reduce_fused"} <= set(dgl.ops.__all__) and config.EDGE_MLP_ITEM_EDGES == U
