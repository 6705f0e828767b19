"""Typed linear layers: ops.segment_mm / ops.gather_mm (csrc/segmm.hip), nn.TypedLinear and nn.TypedRelGraphConv against one fp64
restatement -- a loop over the weight matrices in plain torch.

Bound of the random-value tests, per element: |got - ref| <= (T + 2) * 2^-24 * sum |terms|, T the number of terms of that element's sum
(K for out, M per use of a row for d a, the segment length for d b): the fp32 running-sum bound, which holds for every summation order.
The integer tests (values in -3 .. 3) make every fp32 sum exact: the results must be torch.equal to the fp64 ones, so one lost or doubled
row at a tile, item or segment boundary shows."""
import pytest
import torch

import mi355x_graph as mg
from mi355x_graph import config, nn as mnn, ops, sparse
import oracle_backend

DEV = "cuda:0"
IR = config.SEGMENT_MM_ITEM_ROWS
LENS = [0, 1, 15, 16, 17, IR - 1, IR, IR + 1, 3 * IR + 5, 0]
SRC = torch.tensor([0, 1, 2, 3, 4, 0, 1, 2])
DST = torch.tensor([1, 2, 3, 4, 0, 2, 2, 1])
ETYPE = torch.tensor([2, 0, 1, 2, 2, 0, 1, 0])


def reference(a, b, types, src, g):
    """(out, d a, d b) in fp64 of out[i] = a[src[i]] b[types[i]] and the loss sum(out * g): one matmul per weight matrix"""
    a, b, g, types, src = a.detach().double().cpu(), b.detach().double().cpu(), g.double().cpu(), types.cpu(), src.cpu()
    out, da, db = torch.zeros(types.shape[0], b.shape[2], dtype=torch.float64), torch.zeros_like(a), torch.zeros_like(b)
    for r in range(b.shape[0]):
        rows = (types == r).nonzero().view(-1)
        x = a[src[rows]]
        out[rows] = x @ b[r]
        da.index_add_(0, src[rows], g[rows] @ b[r].t())
        db[r] = x.t() @ g[rows]
    return out, da, db


def operands(lens, K, M, integer, seed=0, rows_a=None):
    gen = torch.Generator().manual_seed(seed)
    n = sum(lens)
    draw = (lambda *s: torch.randint(-3, 4, s, generator=gen).float()) if integer else (lambda *s: torch.randn(*s, generator=gen))
    return draw(rows_a or n, K), draw(len(lens), K, M), draw(n, M), torch.repeat_interleave(torch.arange(len(lens)), torch.tensor(lens))


def check(got, a, b, types, src, g, integer):
    """got = (out, d a, d b) of the operator against the restatement: exact for integers, else the running-sum bound"""
    ref = reference(a, b, types, src, g)
    if integer:
        for x, want in zip(got, ref):
            assert torch.equal(x.detach().double().cpu(), want)
        return
    mag = reference(a.abs(), b.abs(), types, src, g.abs())
    uses = torch.bincount(src, minlength=a.shape[0]).double().view(-1, 1)
    terms = (a.shape[1], b.shape[2] * uses, torch.bincount(types, minlength=b.shape[0]).double().view(-1, 1, 1))
    for name, x, want, m, t in zip(("out", "d a", "d b"), got, ref, mag, terms):
        err, bound = (x.detach().double().cpu() - want).abs(), (t + 2) * 2.0 ** -24 * m
        print("%s: max error %.3g, max of the bound %.3g" % (name, float(err.max()), float(bound.max())))
        assert bool((err <= bound).all()), name


def run(fn, a, b, g, dev):
    a, b = a.clone().to(dev).requires_grad_(True), b.clone().to(dev).requires_grad_(True)  # (fresh leaves on the host as well)
    out = fn(a, b)
    (out * g.to(dev)).sum().backward()
    return out, a.grad, b.grad


@pytest.mark.gpu
@pytest.mark.parametrize("K,M", [(7, 5), (16, 16), (64, 64), (100, 47), (256, 64), (64, 256)])
def test_segment_mm_values_and_gradients(K, M):
    a, b, g, types = operands(LENS, K, M, False)
    seglen = torch.tensor(LENS, device=DEV)
    assert ops.segment_mm_fused(a.to(DEV), b.to(DEV), seglen, total=a.shape[0]) is True
    check(run(lambda x, w: ops.segment_mm(x, w, seglen), a, b, g, DEV), a, b, types, torch.arange(a.shape[0]), g, False)


@pytest.mark.gpu
@pytest.mark.parametrize("lens", [LENS, [1]], ids=["boundaries", "one_row"])
def test_segment_mm_exact_structure(lens):
    a, b, g, types = operands(lens, 16, 16, True)
    seglen = torch.tensor(lens, device=DEV)
    assert ops.segment_mm_fused(a.to(DEV), b.to(DEV), seglen) is True
    got = run(lambda x, w: ops.segment_mm(x, w, seglen), a, b, g, DEV)
    check(got, a, b, types, torch.arange(a.shape[0]), g, True)
    again = run(lambda x, w: ops.segment_mm(x, w, seglen), a, b, g, DEV)
    assert all(torch.equal(x, y) for x, y in zip(got, again))                      # fixed summation order: the same bits


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["column_block", "odd_offset", "host_seglen"])
def test_segment_mm_layouts(layout):
    K, M = 16, 24
    a, b, g, types = operands(LENS, K, M, True)
    n = a.shape[0]
    seglen = torch.tensor(LENS, device="cpu" if layout == "host_seglen" else DEV)
    if layout == "column_block":
        view = torch.zeros(n, K + 8, device=DEV)[:, 4:4 + K]
    elif layout == "odd_offset":
        view = torch.zeros(n * K + 1, device=DEV)[1:].view(n, K)
        assert view.data_ptr() % 16 == 4
    else:
        view = torch.zeros(n, K, device=DEV)
    view.copy_(a)
    assert ops.segment_mm_fused(view, b.to(DEV), seglen) is (layout != "odd_offset")
    x, w = view.requires_grad_(True), b.to(DEV).requires_grad_(True)
    out = ops.segment_mm(x, w, seglen)
    d_a, d_b = torch.autograd.grad((out * g.to(DEV)).sum(), (x, w))
    check((out, d_a, d_b), a, b, types, torch.arange(n), g, True)


@pytest.mark.gpu
@pytest.mark.parametrize("with_idx_a", [False, True])
@pytest.mark.parametrize("integer", [False, True])
def test_gather_mm(with_idx_a, integer):
    n, R, K, M = 70, 5, 12, 20
    gen = torch.Generator().manual_seed(3)
    idx_b = torch.tensor([0, 2, 4])[torch.randint(0, 3, (n,), generator=gen)]         # unsorted; types 1 and 3 are absent
    idx_a = torch.randint(0, 20, (n,), generator=gen) if with_idx_a else None          # 70 reads of 20 rows: repeats
    a, b, g, _ = operands([n] + [0] * (R - 1), K, M, integer, rows_a=20 if with_idx_a else n)
    dev_a = None if idx_a is None else idx_a.to(DEV)
    assert ops.gather_mm_fused(a.to(DEV), b.to(DEV), idx_b.to(DEV), dev_a) is True
    got = run(lambda x, w: ops.gather_mm(x, w, idx_b.to(DEV), dev_a), a, b, g, DEV)
    check(got, a, b, idx_b, torch.arange(n) if idx_a is None else idx_a, g, integer)


@pytest.mark.gpu
@pytest.mark.parametrize("K,M,switch,fused", [(64, 64, True, True), (64, 64, False, False), (256, 128, True, False)])
def test_the_predicate_names_the_path(monkeypatch, K, M, switch, fused):
    lens = [5, 0, 40]
    a, b, g, types = operands(lens, K, M, True)
    backend, calls = type(sparse.backend_for(torch.zeros(1, device=DEV))), []
    inner = backend.segment_mm
    monkeypatch.setattr(backend, "segment_mm", lambda self, *args, **kw: calls.append(1) or inner(self, *args, **kw))
    monkeypatch.setattr(config, "SEGMENT_MM", switch)
    seglen = torch.tensor(lens, device=DEV)
    assert ops.segment_mm_fused(a.to(DEV), b.to(DEV), seglen, total=45) is fused
    out = ops.segment_mm(a.to(DEV), b.to(DEV), seglen, total=45)
    assert len(calls) == (1 if fused else 0)
    assert torch.equal(out.double().cpu(), reference(a, b, types, torch.arange(45), g)[0])


def layer_case(dev, block):
    """(graph, feat, etypes, norm) of the 5-node, 8-edge graph with R = 3; as a block its destination nodes are the first three"""
    gen = torch.Generator().manual_seed(5)
    dst = DST % 3 if block else DST
    g = (mg.create_block((SRC, dst), 5, 3, idtype=torch.int32, device=dev) if block
         else mg.graph((SRC, DST), num_nodes=5).int().to(dev))
    return g, dst, torch.randn(5, 4, generator=gen).to(dev), ETYPE.to(dev), torch.rand(8, 1, generator=gen).to(dev)


def close(got, want):
    # a few dozen fp32 roundings (2^-24 each) of O(1) values stay far below 1e-5; a wrong type, edge, norm or weight is an O(1) error
    return torch.allclose(got.detach().double().cpu(), want.detach(), rtol=1e-4, atol=1e-5)


def check_layers(dev, block):
    g, dst, feat, etypes, norm = layer_case(dev, block)
    for regularizer in (None, "basis"):
        torch.manual_seed(7)
        lin = mnn.TypedLinear(4, 6, 3, regularizer, 2 if regularizer else None).to(dev)
        conv = mnn.TypedRelGraphConv(4, 6, 3, regularizer, 2 if regularizer else None, activation=torch.tanh).to(dev)
        for module, sorted_types in ((lin, False), (lin, True), (conv, False)):
            module.zero_grad()
            twin = {k: v.detach().double().cpu().requires_grad_(True) for k, v in module.named_parameters()}
            x, types = feat.double().cpu(), (etypes.sort().values if sorted_types else etypes).cpu()
            x8 = torch.cat([x, x])[:8]                                             # TypedLinear: eight typed rows
            prefix = "linear_r." if module is conv else ""
            w = twin[prefix + "W"]
            if regularizer:
                w = (twin[prefix + "coeff"] @ w.view(2, -1)).view(3, 4, 6)
            if module is lin:
                got = lin(x8.float().to(dev), types.to(dev), sorted_by_type=sorted_types)
                want = torch.einsum("ik,ikm->im", x8, w[types])
            else:
                got = conv(g, feat, etypes, norm=norm)
                m = torch.einsum("ik,ikm->im", x[SRC], w[types]) * norm.double().cpu()
                want = torch.zeros(3 if block else 5, 6, dtype=torch.float64).index_add(0, dst, m) + twin["h_bias"]
                want = torch.tanh(want + x[:want.shape[0]] @ twin["loop_weight"])
            assert close(got, want)
            got.sin().sum().backward()
            want.sin().sum().backward()
            for k, v in module.named_parameters():
                assert close(v.grad, twin[k].grad), k


@pytest.mark.gpu
@pytest.mark.parametrize("block", [False, True])
def test_typed_layers_on_the_device(block):
    check_layers(DEV, block)


# ----------------------------------------------------------------------------- CPU: operand checks, the composed path
@pytest.fixture
def checker():
    oracle_backend.install()
    yield
    oracle_backend.uninstall()


def test_rejected_operands_raise_and_the_predicates_say_false(checker):
    a, b, g, types = operands([3, 0, 4], 4, 6, True)
    seglen, idx_b = torch.tensor([3, 0, 4]), torch.tensor([2, 0, 0, 2, 2, 0, 2])
    bad_segment = dict(dtype=(a.double(), b, seglen), a_rank=(a[0], b, seglen), b_rank=(a, b[0], seglen), inner=(a, b[:, :3], seglen),
                       length_sum=(a, b, torch.tensor([3, 0, 3])), seglen_float=(a, b, seglen.float()), seglen_count=(a, b, seglen[:2]),
                       device=(a, torch.empty(3, 4, 6, device="meta"), seglen))
    for label, args in bad_segment.items():
        with pytest.raises(mg.DGLError, match="segment_mm"):
            ops.segment_mm(*args)
        assert ops.segment_mm_fused(*args) is False, label
    bad_gather = dict(dtype=(a, b.double(), idx_b), inner=(a, b[:, :3], idx_b), id_high=(a, b, idx_b + 1), id_negative=(a, b, idx_b - 1),
                      id_count=(a, b, idx_b[:6]), id_float=(a, b, idx_b.float()), idx_a_range=(a, b, idx_b, idx_b + 5),
                      device=(a, b, torch.empty(7, dtype=torch.int64, device="meta")))
    for label, args in bad_gather.items():
        with pytest.raises(mg.DGLError, match="gather_mm"):
            ops.gather_mm(*args)
        assert ops.gather_mm_fused(*args) is False, label
    with pytest.raises(mg.DGLError, match="TypedLinear"):
        mnn.TypedLinear(4, 6, 3, "bdd", 2)
    assert ops.segment_mm_fused(a, b, seglen) is False and ops.gather_mm_fused(a, b, idx_b) is False
    check(run(lambda x, w: ops.segment_mm(x, w, seglen), a, b, g, "cpu"), a, b, types, torch.arange(7), g, True)
    src = torch.tensor([6, 0, 0, 3, 1, 1, 2])
    check(run(lambda x, w: ops.gather_mm(x, w, idx_b, src), a, b, g, "cpu"), a, b, idx_b, src, g, True)


def test_typed_layers_compose_on_the_cpu(checker):
    check_layers("cpu", False)
