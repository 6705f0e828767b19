"""Segment k nearest neighbours: csrc/knn.hip (mgx_segment_knn), ops.segment_knn / segment_knn_fused, transform.knn_graph /
segmented_knn_graph, nn.KNNGraph / SegmentedKNNGraph / EdgeConv, point_cloud.py.

The reference everywhere is the restatement below, a Python loop over the segments and never the code under test:

    d64 = ((s[:, None] - s[None]) ** 2).sum(-1) in fp64;  torch.sort(d64, dim=1, stable=True);  index -1 / dist +inf past a segment's end

  exact   integer coordinates in [-3, 3]: every distance is an integer below 2^24, exact in fp32 in any order -- torch.equal on the
          index (ties are everywhere, so "equal distances keep the lower row" is what is tested), bit equality on dist
  float   normal / row-scaled / a cluster at 1000 + 1e-3 randn (where the expansion |x|^2 + |y|^2 - 2xy fails): for every query and rank
          |d64(i, got[i, j]) - d64_sorted[i, j]| <= (D + 2) 2^-23 d64_sorted[i, j], dist within (D + 2) 2^-24 relative of d64 -- each
          squared difference carries at most 3 roundings, the sum of D non-negative terms D - 1 more, and two distances are compared
  EdgeConv  fused form, composed form and an fp64 restatement: exactly equal (output and every gradient) on integer data; float data
          within (in_feat + 3) 2^-24 A forward and (T + 8) 2^-23 A for the gradients (magnitude A, term count T, as
          tests/test_broadcast_grad.py), where the reference's top-two gap exceeds twice the forward bound so the arg cannot differ."""
import ctypes
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import mi355x_graph as mg
import mi355x_graph.nn  # noqa: F401
from mi355x_graph import _lib, config, ops
import oracle_backend

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dgl-0.5-benchmark_amd")
DEV = "cuda:0"
INF = float("inf")


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ----------------------------------------------------------------------------- the restatement (a loop over segments, never the code under test)
class Restated(object):
    """d64: per segment the fp64 distance matrix; order / sorted: its stable sort.  index(k) / dist(k): the padded outputs."""

    def __init__(self, lens, x):
        x = x.detach().cpu().double()
        self.lens, self.N = [int(n) for n in lens], int(x.shape[0])
        self.d64, self.order, self.sorted = [], [], []
        o = 0
        for n in self.lens:
            s = x[o:o + n]
            d = torch.cat([((s[q:q + 64, None] - s[None]) ** 2).sum(-1) for q in range(0, n, 64)]) if n else torch.zeros(0, 0, dtype=torch.float64)
            srt = torch.sort(d, dim=1, stable=True)
            self.d64.append(d)
            self.order.append(srt.indices)
            self.sorted.append(srt.values)
            o += n
        assert o == self.N

    def index(self, k):
        out = torch.full((self.N, k), -1, dtype=torch.int64)
        o = 0
        for n, order in zip(self.lens, self.order):
            out[o:o + n, :min(k, n)] = order[:, :k] + o
            o += n
        return out

    def dist(self, k):
        out = torch.full((self.N, k), INF, dtype=torch.float64)
        o = 0
        for n, srt in zip(self.lens, self.sorted):
            out[o:o + n, :min(k, n)] = srt[:, :k]
            o += n
        return out


LENS = (0, 1, 15, 16, 17, 19, 20, 21, 63, 64, 65, 0, 127, 300)   # empty; below, at and above k; the 16-row tile; the 64-candidate chunk; several chunks
KS = (1, 2, 20, 63, 64)
DS = (1, 3, 4, 64, 67, 256)
FLOAT_LENS = (20, 21, 64, 65, 127, 300)


@functools.lru_cache(maxsize=None)
def int_points(lens, D, seed=0):
    return torch.randint(-3, 4, (sum(lens), D), generator=torch.Generator().manual_seed(1000 * D + seed)).float()


@functools.lru_cache(maxsize=None)
def int_case(lens, D):
    x = int_points(lens, D)
    return x, Restated(lens, x)


@functools.lru_cache(maxsize=None)
def nan_case():
    """one point with a NaN coordinate (in the segment of 65) and the segment of 17 NaN only"""
    x = int_points(LENS, 4, seed=1).clone()
    ends = np.cumsum(LENS)
    s65, s17 = LENS.index(65), LENS.index(17)
    x[ends[s65] - 30, 2] = float("nan")
    x[ends[s17] - 17:ends[s17]] = float("nan")
    return x, Restated(LENS, x)


def check_exact(got_index, got_dist, ref, k, what=""):
    assert got_index.dtype == torch.int64 and tuple(got_index.shape) == (ref.N, k), what
    assert torch.equal(got_index.cpu(), ref.index(k)), what
    if got_dist is not None:
        want = ref.dist(k)
        got = got_dist.cpu()
        assert got.dtype == torch.float32 and not got_dist.requires_grad, what
        assert torch.equal(torch.isnan(got), torch.isnan(want)), what   # a NaN distance is a NaN (whatever its bits), in the same places
        assert torch.equal(bits(got.nan_to_num(nan=-1.0)), bits(want.float().nan_to_num(nan=-1.0))), what


def knn(lens, x, k, device, return_dist=True, seglen_dtype=torch.int64):
    return ops.segment_knn(torch.tensor(lens, dtype=seglen_dtype).to(device), x.to(device), k, total=int(x.shape[0]), return_dist=return_dist)


def launches(monkeypatch):
    rec = []
    monkeypatch.setattr(mg.sparse, "PROFILE", rec)
    return rec


# ----------------------------------------------------------------------------- float cases
@functools.lru_cache(maxsize=None)
def float_case(D, kind):
    gen = torch.Generator().manual_seed(7 * D + len(kind))
    N = sum(FLOAT_LENS)
    x = torch.randn(N, D, generator=gen)
    if kind == "scaled":
        x = x * torch.exp(4 * torch.randn(N, 1, generator=gen))
    elif kind == "cluster":
        x = 1000 + 1e-3 * x
    else:
        assert kind == "normal"
    return x, Restated(FLOAT_LENS, x)


def check_float(got_index, got_dist, ref, k, D, what=""):
    index, dist = got_index.cpu(), got_dist.cpu().double()
    o, worst = 0, 0.0
    for n, d64, srt in zip(ref.lens, ref.d64, ref.sorted):
        idx = index[o:o + n]
        assert bool(((idx >= o) & (idx < o + n)).all()), what                         # inside the query's own segment (n >= k here)
        assert bool((idx.sort(dim=1).values.diff(dim=1) > 0).all()), what             # no index twice in a row
        at = d64.gather(1, idx - o)                                                   # fp64 distance of what was returned
        want = srt[:, :k]
        err, bound = (at - want).abs(), (D + 2) * 2.0 ** -23 * want
        assert bool((err <= bound).all()), "%s: rank distance off by %g of the bound" % (what, float((err / bound.clamp(min=1e-300)).max()))
        worst = max(worst, float((err / bound.clamp(min=1e-300)).max()))
        derr, dbound = (dist[o:o + n] - at).abs(), (D + 2) * 2.0 ** -24 * at
        assert bool((derr <= dbound).all()), "%s: dist off by %g of the bound" % (what, float((derr / dbound.clamp(min=1e-300)).max()))
        o += n
    print("knn float %s: worst rank-distance error / bound %.3f" % (what, worst))


# ----------------------------------------------------------------------------- CPU: checker backend and the OpenMP backend
@pytest.fixture(params=["checker", "openmp"])
def cpu_backend_on(request):
    if request.param == "checker":
        oracle_backend.install()
        yield request.param
        oracle_backend.uninstall()
    else:
        was = mg.enable_cpu_backend(True)
        try:
            yield request.param
        finally:
            mg.enable_cpu_backend(was)


@pytest.mark.parametrize("D", DS)
def test_composition_matches_the_restatement_exactly(cpu_backend_on, D):
    x, ref = int_case(LENS, D)
    assert not ops.segment_knn_fused(torch.tensor(LENS), x, 20)
    for k in KS:
        index, dist = knn(LENS, x, k, "cpu", seglen_dtype=torch.int32 if k % 2 else torch.int64)
        check_exact(index, dist, ref, k, (D, k))
        only = knn(LENS, x, k, "cpu", return_dist=False)
        assert torch.is_tensor(only) and torch.equal(only, index)


def test_composition_nan_and_strided(cpu_backend_on):
    x, ref = nan_case()
    for k in (2, 20):
        check_exact(*knn(LENS, x, k, "cpu"), ref, k, k)
    wide = int_points(LENS, 9)
    block = wide[:, 2:6]
    assert not block.is_contiguous()
    check_exact(*knn(LENS, block, 20, "cpu"), Restated(LENS, block), 20)


@pytest.mark.parametrize("kind", ["normal", "scaled", "cluster"])
def test_composition_float_cases(cpu_backend_on, kind):
    for D in (1, 3, 64, 128):
        x, ref = float_case(D, kind)
        index, dist = knn(FLOAT_LENS, x, 20, "cpu")
        check_float(index, dist, ref, 20, D, "composition %s D=%d" % (kind, D))


def test_no_rows_no_segments_and_argument_errors(cpu_backend_on):
    index, dist = ops.segment_knn(torch.zeros(0, dtype=torch.int64), torch.zeros(0, 3), 4, return_dist=True)
    assert tuple(index.shape) == (0, 4) and tuple(dist.shape) == (0, 4)
    index = ops.segment_knn(torch.tensor([0, 0]), torch.zeros(0, 3), 4)
    assert tuple(index.shape) == (0, 4)
    x = int_points((5, 7), 3)
    for bad in (lambda: ops.segment_knn(torch.tensor([5, 7]), x, 0),
                lambda: ops.segment_knn(torch.tensor([5, 7]), x, True),
                lambda: ops.segment_knn(torch.tensor([5, 7]), x, 2.0),
                lambda: ops.segment_knn(torch.tensor([5, 6]), x, 2),
                lambda: ops.segment_knn(torch.tensor([5, 7]), x.double(), 2),
                lambda: ops.segment_knn(torch.tensor([5, 7]), x[:, 0], 2),
                lambda: ops.segment_knn([5, 7], x, 2)):
        with pytest.raises(mg.DGLError):
            bad()


def test_without_a_cpu_backend_cpu_tensors_fail_loudly(monkeypatch):
    monkeypatch.delitem(mg.sparse._BACKENDS, "cpu", raising=False)
    with pytest.raises(mg.DGLError, match="MI355X"):
        ops.segment_knn(torch.tensor([5, 7]), int_points((5, 7), 3), 2)


def test_abi_argument_checks():
    L = _lib.lib()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("mgx_segment_knn_supported", "mgx_segment_knn"):
        assert hasattr(handle, name) and name in _lib.SIGNATURES
    assert L.mgx_abi_version() == 35
    for (k, D), want in (((1, 1), 1), ((64, 256), 1), ((20, 3), 1), ((65, 3), 0), ((20, 257), 0), ((0, 3), 0), ((20, 0), 0), ((-1, 3), 0)):
        assert L.mgx_segment_knn_supported(k, D) == want, (k, D)
    host = (ctypes.c_float * 64)()                                             # never dereferenced: every call below fails a check first
    p = ctypes.c_void_p(ctypes.addressof(host))

    def call(S=2, offsets=p, N=8, D=4, ld=4, x=p, k=2, index=p, dist=p):
        return L.mgx_segment_knn(S, offsets, N, D, ld, x, k, index, dist, None)

    assert call(k=0) == 1 and b"k must be at least 1" in L.mgx_last_error()
    with pytest.raises(mg.DGLError, match="k must be at least 1"):
        _lib.check(1)
    assert call(k=-3) == 1 and call(S=-1) == 1 and call(N=-1) == 1 and call(D=0) == 1
    assert call(ld=3) == 1 and b"row stride" in L.mgx_last_error()
    assert call(k=65) == _lib.ERR_UNSUPPORTED and call(D=257, ld=257) == _lib.ERR_UNSUPPORTED
    assert call(N=2 ** 31) == _lib.ERR_UNSUPPORTED and call(N=2 ** 28, ld=4) == _lib.ERR_UNSUPPORTED   # 2^31 rows; 4 GiB of x
    assert call(offsets=None) == 1 and call(x=None) == 1 and call(index=None) == 1 and b"offsets / x / index is NULL" in L.mgx_last_error()
    assert call(N=0, offsets=None, x=None, index=None, dist=None) == 0          # no rows: nothing to do


# ----------------------------------------------------------------------------- graph builders
def check_builders(device):
    import dgl
    x = int_points((72,), 4).to(device)
    ref = Restated([24, 24, 24], x)
    k, N = 5, 72
    g3 = dgl.knn_graph(x.view(3, 24, 4), k)
    gs = dgl.segmented_knn_graph(x, k, [24, 24, 24])
    gl = dgl.nn.KNNGraph(k)(x.view(3, 24, 4))
    gm = dgl.nn.SegmentedKNNGraph(k)(x, [24, 24, 24])
    want = (ref.index(k).flatten(), torch.arange(N).repeat_interleave(k))
    for g in (g3, gs, gl, gm):
        assert g.number_of_nodes() == N and g.number_of_edges() == N * k and g.idtype == torch.int32
        assert g._index.format_status() == {"created": ["csc"], "not created": ["coo", "csr"]}     # the in-CSR, without a conversion
        assert g._index.csc().eids is None and g._index.max_in_degree_hint == k
        assert torch.equal(g.in_degrees().cpu().long(), torch.full((N,), k))
        src, dst = g.edges()
        assert torch.equal(src.cpu().long(), want[0]) and torch.equal(dst.cpu().long(), want[1])
    one = dgl.knn_graph(x, 3)                                                   # [N, D]: one segment
    assert torch.equal(one.edges()[0].cpu().long(), Restated([72], x).index(3).flatten())
    ragged = dgl.segmented_knn_graph(x, 4, [10, 40, 22])
    assert torch.equal(ragged.edges()[0].cpu().long(), Restated([10, 40, 22], x).index(4).flatten())
    for bad in (lambda: dgl.segmented_knn_graph(x, 11, [10, 40, 22]), lambda: dgl.knn_graph(x.view(3, 24, 4), 25),
                lambda: dgl.segmented_knn_graph(x, 4, [10, 40]), lambda: dgl.knn_graph(x, 0), lambda: dgl.knn_graph(x[0], 1)):
        with pytest.raises(mg.DGLError):
            bad()


def test_graph_builders(cpu_backend_on):
    check_builders("cpu")


# ----------------------------------------------------------------------------- EdgeConv
class HostGraph(object):
    def __init__(self, src, dst, n_src, n_dst):
        self.src, self.dst, self.n_src, self.n_dst = src.long(), dst.long(), n_src, n_dst


@functools.lru_cache(maxsize=None)
def conv_graphs():
    """(name -> HostGraph): the k-NN graph of 3 segments of about 30 points (k = 6), a hand-made graph whose node 5 has neither in- nor
    out-edges, a block of 7 destination nodes over 12 source nodes"""
    lens = (29, 30, 33)
    ref = Restated(lens, int_points(lens, 3, seed=5))
    N = sum(lens)
    knn_g = HostGraph(ref.index(6).flatten(), torch.arange(N).repeat_interleave(6), N, N)
    hs = torch.tensor([0, 1, 2, 3, 4, 6, 7, 0, 2, 4, 6, 1, 3, 7, 0, 1])
    hd = torch.tensor([1, 2, 3, 4, 6, 7, 0, 2, 4, 7, 0, 3, 7, 1, 0, 1])
    bs = torch.tensor([0, 7, 8, 11, 1, 2, 9, 3, 10, 4, 5, 6, 11, 8])
    bd = torch.tensor([0, 0, 0, 0, 1, 1, 1, 2, 2, 3, 4, 4, 4, 6])              # destination 5 has no in-edge
    return {"knn": knn_g, "hand": HostGraph(hs, hd, 8, 8), "block": HostGraph(bs, bd, 12, 7)}


def build_graph(name, device):
    import dgl
    h = conv_graphs()[name]
    if name == "knn":
        lens = (29, 30, 33)
        g = dgl.segmented_knn_graph(int_points(lens, 3, seed=5).to(device), 6, list(lens))
        assert torch.equal(g.edges()[0].cpu().long(), h.src)
        return g
    if name == "block":
        return dgl.create_block((h.src, h.dst), num_src_nodes=h.n_src, num_dst_nodes=h.n_dst).int().to(device)
    return dgl.graph((h.src, h.dst), num_nodes=h.n_src).int().to(device)


def conv_restated(h, x, params, w, batch_norm=None):
    """fp64: (out, grads of sum(out * w) w.r.t. x, theta.weight, theta.bias, phi.weight, phi.bias, edge values e, first-wins arg)"""
    x = x.double().clone().requires_grad_(True)
    tw, tb, pw, pb = [p.double().clone().requires_grad_(True) for p in params]
    xs, xd = x, x[:h.n_dst]
    e = (xs[h.src] - xd[h.dst]) @ tw.t() + tb + xd[h.dst] @ pw.t() + pb
    if batch_norm is not None:
        gamma, beta, eps = batch_norm
        mu, var = e.mean(0), e.var(0, unbiased=False)
        e = (e - mu) / torch.sqrt(var + eps) * gamma.double() + beta.double()
    rows, args = [], []
    for v in range(h.n_dst):
        ids = (h.dst == v).nonzero().flatten()
        if ids.numel() == 0:
            rows.append(torch.zeros(e.shape[1], dtype=torch.float64))
            args.append(torch.full((e.shape[1],), -1))
            continue
        a = e[ids].detach().argmax(0)                                           # the first maximal value (torch.argmax's documented tie rule)
        rows.append(e[ids].gather(0, a.unsqueeze(0))[0])
        args.append(ids[a])
    out = torch.stack(rows)
    grads = torch.autograd.grad((out * w.double()).sum(), [x, tw, tb, pw, pb], allow_unused=True)
    return out.detach(), [torch.zeros_like(p) if g is None else g for g, p in zip(grads, (x, tw, tb, pw, pb))], e.detach(), torch.stack(args)


def conv_run(name, in_feat, x, params, w, device, fused, monkeypatch, batch_norm=False):
    monkeypatch.setattr(config, "EDGECONV_FUSED", fused)
    g = build_graph(name, device)
    conv = mg.nn.EdgeConv(in_feat, 8, batch_norm=batch_norm, allow_zero_in_degree=True).to(device)
    with torch.no_grad():
        for p, v in zip((conv.theta.weight, conv.theta.bias, conv.phi.weight, conv.phi.bias), params):
            p.copy_(v)
    xx = x.to(device).requires_grad_(True)
    h = conv_graphs()[name]
    out = conv(g, (xx, xx[:h.n_dst]) if name == "block" else xx)
    grads = torch.autograd.grad(out, [xx, conv.theta.weight, conv.theta.bias, conv.phi.weight, conv.phi.bias], w.to(device))
    return out.detach().cpu(), [t.cpu() for t in grads], conv


def int_conv_inputs(name, in_feat):
    h = conv_graphs()[name]
    gen = torch.Generator().manual_seed(in_feat + len(name))
    ri = lambda *shape: torch.randint(-2, 3, shape, generator=gen).float()
    x = int_points((29, 30, 33), 3, seed=5) if (name == "knn" and in_feat == 3) else ri(h.n_src, in_feat)
    return x, (ri(8, in_feat), ri(8), ri(8, in_feat), ri(8)), ri(h.n_dst, 8)


def check_conv_exact(device, monkeypatch):
    for name in ("knn", "hand", "block"):
        for in_feat in (3, 64):
            h = conv_graphs()[name]
            x, params, w = int_conv_inputs(name, in_feat)
            ref_out, ref_grads, _, _ = conv_restated(h, x, params, w)
            for fused in (True, False):
                out, grads, _ = conv_run(name, in_feat, x, params, w, device, fused, monkeypatch)
                what = (name, in_feat, fused)
                assert torch.equal(out.double(), ref_out), what
                for got, want in zip(grads, ref_grads):
                    assert torch.equal(got.double(), want), what
            if name != "knn":                                                   # the node without in-edges: 0, and no gradient to its x
                lone = 5
                assert bool((ref_out[lone] == 0).all()) and bool((out[lone] == 0).all())
                if name == "hand":
                    assert bool((grads[0][lone] == 0).all())


def test_edgeconv_integer_data_all_forms_equal(cpu_backend_on, monkeypatch):
    check_conv_exact("cpu", monkeypatch)


@functools.lru_cache(maxsize=None)
def float_conv_case(name, in_feat):
    """inputs, the fp64 reference, magnitudes A and the gap condition asserted on the reference alone"""
    h = conv_graphs()[name]
    gen = torch.Generator().manual_seed(40 + in_feat + len(name))
    rn = lambda *shape: torch.randn(shape, generator=gen)
    x, params, w = rn(h.n_src, in_feat), (rn(8, in_feat) / in_feat ** 0.5, rn(8), rn(8, in_feat) / in_feat ** 0.5, rn(8)), rn(h.n_dst, 8)
    out, grads, e, arg = conv_restated(h, x, params, w)
    # magnitudes: the same expression with every sub an add over absolute values, the arg held fixed
    ax = x.double().abs().requires_grad_(True)
    atw, atb, apw, apb = [p.double().abs().requires_grad_(True) for p in params]
    ae = (ax[h.src] + ax[:h.n_dst][h.dst]) @ atw.t() + atb + ax[:h.n_dst][h.dst] @ apw.t() + apb
    live = arg >= 0
    A_sel = torch.where(live, ae.gather(0, arg.clamp(min=0)), torch.zeros((), dtype=torch.float64))
    A_grads = torch.autograd.grad((A_sel * w.double().abs()).sum(), [ax, atw, atb, apw, apb])
    A_out = torch.zeros(h.n_dst, 8, dtype=torch.float64)                        # the largest over the row's edges
    for v in range(h.n_dst):
        ids = (h.dst == v).nonzero().flatten()
        if ids.numel():
            A_out[v] = ae[ids].detach().max(0).values
    fwd_bound = (in_feat + 3) * 2.0 ** -24 * A_out
    for v in range(h.n_dst):                                                    # the top-two gap exceeds twice the bound: the arg cannot differ
        ids = (h.dst == v).nonzero().flatten()
        if ids.numel() >= 2:
            top = e[ids].topk(2, dim=0).values
            assert bool((top[0] - top[1] > 2 * fwd_bound[v]).all()), "seed gives a near-tie in row %d: pick another" % v
    out_deg = torch.bincount(h.src, minlength=h.n_src).max().item()
    T = [8 * (out_deg + 2), 2 * h.n_dst, h.n_dst, h.n_dst, h.n_dst]
    return x, params, w, out, grads, fwd_bound, [a.detach() for a in A_grads], T


def check_conv_float(device, monkeypatch):
    for name in ("knn", "hand", "block"):
        for in_feat in (3, 64):
            x, params, w, ref_out, ref_grads, fwd_bound, A_grads, T = float_conv_case(name, in_feat)
            for fused in (True, False):
                out, grads, _ = conv_run(name, in_feat, x, params, w, device, fused, monkeypatch)
                what = (name, in_feat, fused)
                err = (out.double() - ref_out).abs()
                assert bool((err <= fwd_bound).all()), "%s: forward %g of the bound" % (what, float((err / fwd_bound.clamp(min=1e-300)).max()))
                for got, want, A, t in zip(grads, ref_grads, A_grads, T):
                    gerr, gbound = (got.double() - want).abs(), (t + 8) * 2.0 ** -23 * A
                    assert bool((gerr <= gbound).all()), "%s: gradient %g of the bound" % (what, float((gerr / gbound.clamp(min=1e-300)).max()))


def test_edgeconv_float_data_within_the_bounds(cpu_backend_on, monkeypatch):
    check_conv_float("cpu", monkeypatch)


def check_conv_batch_norm(device, monkeypatch):
    """batch_norm=True runs the composition whatever the switch says.  Bound: the pre-norm e carries at most de = (in_feat + 3) eps A_e;
    with E edges the mean adds (E + 8) eps max|e|, so e - mu is off by at most 2 D_f, D_f = max_e de + (E + 8) eps max|e|; the variance by
    4 D_f sigma (mean |e - mu| <= sigma), sigma by a relative 2 D_f / sigma (4 D_f / sigma is allowed) plus (E + 8) eps of summation; the
    affine step and the final rounding 4 eps (|y| + |beta|).  The max over a row's edges errs by at most the largest bound among them."""
    eps = 2.0 ** -24
    for name, in_feat in (("knn", 3), ("hand", 64)):
        h = conv_graphs()[name]
        x, params, w = float_conv_case(name, in_feat)[:3]
        gen = torch.Generator().manual_seed(3)
        gamma, beta = torch.rand(8, generator=gen) + 0.5, torch.randn(8, generator=gen)
        for fused in (True, False):
            monkeypatch.setattr(config, "EDGECONV_FUSED", fused)
            g = build_graph(name, device)
            conv = mg.nn.EdgeConv(in_feat, 8, batch_norm=True, allow_zero_in_degree=True).to(device).train()
            with torch.no_grad():
                for p, v in zip((conv.theta.weight, conv.theta.bias, conv.phi.weight, conv.phi.bias, conv.bn.weight, conv.bn.bias),
                                params + (gamma, beta)):
                    p.copy_(v)
            out = conv(g, x.to(device)).detach().cpu().double()
            ref_out, _, y, _ = conv_restated(h, x, params, w, batch_norm=(gamma, beta, conv.bn.eps))
            _, _, e, _ = conv_restated(h, x, params, w)
            ax = x.double().abs()
            ae = (ax[h.src] + ax[h.dst]) @ params[0].double().abs().t() + params[1].double().abs() + ax[h.dst] @ params[2].double().abs().t() \
                + params[3].double().abs()
            E = e.shape[0]
            Df = ((in_feat + 3) * eps * ae).max(0).values + (E + 8) * eps * e.abs().max(0).values
            sigma = torch.sqrt(e.var(0, unbiased=False) + conv.bn.eps)
            yb = gamma.double() / sigma * 2 * Df + (y - beta.double()).abs() * (4 * Df / sigma + (E + 8) * eps) + 4 * eps * (y.abs() + beta.double().abs())
            bound = torch.zeros_like(ref_out)
            for v in range(h.n_dst):
                ids = (h.dst == v).nonzero().flatten()
                if ids.numel():
                    bound[v] = yb[ids].max(0).values
            err = (out - ref_out).abs()
            assert bool((err <= bound).all()), "%s: batch-norm forward %g of the bound" % ((name, in_feat, fused), float((err / bound.clamp(min=1e-300)).max()))


def test_edgeconv_batch_norm_matches_the_restatement(cpu_backend_on, monkeypatch):
    check_conv_batch_norm("cpu", monkeypatch)


def test_edgeconv_zero_in_degree_raises_unless_allowed(cpu_backend_on):
    g = build_graph("hand", "cpu")
    with pytest.raises(mg.DGLError, match="0-in-degree"):
        mg.nn.EdgeConv(3, 8)(g, torch.zeros(8, 3))
    import dgl
    assert dgl.nn.EdgeConv is mg.nn.EdgeConv and dgl.nn.pytorch.conv.EdgeConv is mg.nn.EdgeConv
    assert dgl.nn.pytorch.factory.KNNGraph is mg.nn.KNNGraph and dgl.nn.pytorch.factory.SegmentedKNNGraph is mg.nn.SegmentedKNNGraph
    assert dgl.transform.knn_graph is dgl.knn_graph and dgl.transform.segmented_knn_graph is dgl.segmented_knn_graph
    conv = mg.nn.EdgeConv(3, 8)
    assert sorted(n for n, _ in conv.named_parameters()) == ["phi.bias", "phi.weight", "theta.bias", "theta.weight"]


# ----------------------------------------------------------------------------- the script
def test_script_model_trains_one_tiny_epoch_on_the_cpu():
    """point_cloud.py's own parser, model and epoch loop on the OpenMP backend (the script's main() asks for a device)"""
    sys.path.insert(0, PKG)
    import point_cloud as pc
    from mi355x_graph.datasets import POINT_SHAPES, shapes_like
    args = pc.make_parser().parse_args([])
    assert (args.points, args.batch, args.k) == (1024, 32, 20)
    xyz, label = shapes_like(4, 32, seed=2)
    assert tuple(xyz.shape) == (4, 32, 3) and xyz.dtype == torch.float32 and label.dtype == torch.int64
    assert torch.equal(xyz, shapes_like(4, 32, seed=2)[0])                       # seeded
    was = mg.enable_cpu_backend(True)                                            # (the checker backend has no arg for the max readout's backward)
    try:
        torch.manual_seed(0)
        model = pc.DGCNN(4, len(POINT_SHAPES))
        assert [tuple(c.theta.weight.shape) for c in model.convs] == [(64, 3), (64, 64), (128, 64), (256, 128)]
        loss = pc.train_epoch(model, torch.device("cpu"), xyz, label, 4, torch.optim.Adam(model.parameters(), lr=1e-3))
        assert np.isfinite(loss)
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    finally:
        mg.enable_cpu_backend(was)


# ----------------------------------------------------------------------------- GPU: the kernel against the restatement
@pytest.mark.gpu
@pytest.mark.parametrize("D", DS)
def test_kernel_matches_the_restatement_exactly(monkeypatch, D):
    x, ref = int_case(LENS, D)
    for k in KS:
        seglen_dtype = torch.int32 if k % 2 else torch.int64
        assert ops.segment_knn_fused(torch.tensor(LENS, dtype=seglen_dtype).to(DEV), x.to(DEV), k)
        rec = launches(monkeypatch)
        index, dist = knn(LENS, x, k, DEV, seglen_dtype=seglen_dtype)
        assert [r["kernel"] for r in rec] == ["segment_knn"]                    # one launch, nothing else from the library
        check_exact(index, dist, ref, k, (D, k))
        again_index, again_dist = knn(LENS, x, k, DEV, seglen_dtype=seglen_dtype)     # reruns give identical bits
        assert torch.equal(index, again_index) and torch.equal(bits(dist), bits(again_dist))
        only = knn(LENS, x, k, DEV, return_dist=False)                          # dist = NULL
        assert torch.is_tensor(only) and torch.equal(only, index)


@pytest.mark.gpu
def test_kernel_nan_strided_and_single_segment(monkeypatch):
    x, ref = nan_case()
    for k in (2, 20, 64):
        check_exact(*knn(LENS, x, k, DEV), ref, k, ("nan", k))
    wide = int_points(LENS, 100).to(DEV)
    block = wide[:, 10:77]                                                      # D = 67, row stride 100, base 40 bytes into a row
    assert not block.is_contiguous()
    rec = launches(monkeypatch)
    got = knn(LENS, block, 20, DEV)
    assert [r["kernel"] for r in rec] == ["segment_knn"]
    check_exact(*got, Restated(LENS, block), 20, "strided")
    odd = wide[:, ::2]                                                          # a column stride of 2: copied, same result
    check_exact(*knn(LENS, odd, 20, DEV), Restated(LENS, odd), 20, "column stride")
    one = int_points((1000,), 3)
    check_exact(*knn([1000], one, 64, DEV), Restated([1000], one), 64, "one segment")
    check_exact(*knn([0, 0, 1000, 0], one, 7, DEV), Restated([0, 0, 1000, 0], one), 7, "empty segments around")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["normal", "scaled", "cluster"])
def test_kernel_float_cases(kind):
    for D in (1, 3, 64, 128):
        x, ref = float_case(D, kind)
        assert ops.segment_knn_fused(torch.tensor(FLOAT_LENS).to(DEV), x.to(DEV), 20)
        index, dist = knn(FLOAT_LENS, x, 20, DEV)
        check_float(index, dist, ref, 20, D, "kernel %s D=%d" % (kind, D))


@pytest.mark.gpu
def test_outside_the_kernels_set_takes_the_composition(monkeypatch):
    seglen = torch.tensor(LENS).to(DEV)
    x, ref = int_case(LENS, 4)
    assert ops.segment_knn_fused(seglen, x.to(DEV), 64) and not ops.segment_knn_fused(seglen, x.to(DEV), 65)
    rec = launches(monkeypatch)
    check_exact(*knn(LENS, x, 65, DEV), ref, 65, "k = 65")
    lens = (20, 70, 33)
    wide, wref = int_case(lens, 257)
    assert ops.segment_knn_fused(torch.tensor(lens).to(DEV), wide[:, :256].to(DEV), 20)
    assert not ops.segment_knn_fused(torch.tensor(lens).to(DEV), wide.to(DEV), 20)
    check_exact(*knn(lens, wide, 20, DEV), wref, 20, "D = 257")
    monkeypatch.setattr(config, "KNN_FUSED", False)
    assert not ops.segment_knn_fused(seglen, x.to(DEV), 20)
    check_exact(*knn(LENS, x, 20, DEV), ref, 20, "switch off")
    assert not any(r["kernel"] == "segment_knn" for r in rec)


@pytest.mark.gpu
def test_captured_in_a_hip_graph():
    """the capture idiom of tests/test_segment_topk.py: warm-up and capture on ONE side stream, then replay with new points in the static
    input -- the operator reads nothing back to the host"""
    lens = LENS
    N = sum(lens)
    seglen = torch.tensor(lens).to(DEV)
    static = int_points(lens, 4).to(DEV).clone()
    outs = {}

    def step():
        outs["got"] = ops.segment_knn(seglen, static, 20, total=N, return_dist=True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), ops.warming_up_for_capture():
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        step()
    new = int_points(lens, 4, seed=9)
    static.copy_(new.to(DEV))
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    index, dist = outs["got"]
    eager_index, eager_dist = knn(lens, new, 20, DEV)
    assert torch.equal(index, eager_index) and torch.equal(bits(dist), bits(eager_dist))
    check_exact(index, dist, Restated(lens, new), 20)


@pytest.mark.gpu
def test_graph_builders_on_the_device():
    check_builders(DEV)


@pytest.mark.gpu
def test_edgeconv_on_the_device_integer_data(monkeypatch):
    check_conv_exact(DEV, monkeypatch)


@pytest.mark.gpu
def test_edgeconv_on_the_device_float_data(monkeypatch):
    check_conv_float(DEV, monkeypatch)


@pytest.mark.gpu
def test_edgeconv_on_the_device_batch_norm(monkeypatch):
    check_conv_batch_norm(DEV, monkeypatch)


@functools.lru_cache(maxsize=None)
def _script(*args):
    """(losses printed per epoch, whole output) of one run of the script"""
    env = dict(os.environ, PYTHONPATH=PKG)
    cmd = [sys.executable, os.path.join(PKG, "point_cloud.py"), "--clouds", "4", "--batch", "4", "--points", "32", "--k", "4", "--dropout", "0",
           "--no-shuffle"] + list(args)
    res = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert res.returncode == 0, res.stdout[-3000:]
    losses = [float(v) for v in re.findall(r"epoch \d+ loss (\S+)", res.stdout)]
    return losses, res.stdout


@pytest.mark.gpu
def test_script_trains_to_a_finite_decreasing_loss():
    """five epochs of one step each on the same 4 clouds of 32 points, k = 4"""
    losses, text = _script("--epochs", "5")
    assert len(losses) == 5 and all(np.isfinite(v) for v in losses), text[-2000:]
    assert losses[-1] < losses[0], text[-2000:]
