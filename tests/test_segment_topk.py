"""Segment top-k: csrc/segtopk.hip (mgx_segment_topk_*), ops.segment_topk / segment_topk_fused, readout.topk_nodes / topk_edges,
nn.SortPooling, graph_classification.py --readout sortpool.

Everything is a copy, so every comparison is exact: torch.equal on indices, int32 bit views of values and gradients (NaN and -0.0 are
compared as bits).  The reference everywhere is the restatement below, a Python loop over the segments, never the code under test:

    order = torch.sort(key, stable=True, descending=...) on the CPU; the first min(k, len) of it; zero values and index -1 past them
    d feat = zeros.index_put_(selected rows or elements, d values)

  CPU   the composition behind the operator (checker backend and the OpenMP backend), topk_nodes / topk_edges, SortPooling, argument
        errors, the C ABI's argument checks, one tiny epoch of the script's model with --readout sortpool
  GPU   the kernels: both forms (k <= 64: a wave, k <= 1024: a workgroup) over empty / short / chunk-sized / long segments, both modes,
        both directions, ties, specials (+-0, +-inf, NaN, a NaN with the sign bit set, a segment of NaN only), strided operands, int32 and
        int64 lengths, the backward gather, reruns, HIP-graph capture, the script under --hipgraph."""
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


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ----------------------------------------------------------------------------- the restatement (a loop over segments, never the code under test)
class Restated(object):
    def __init__(self, lens, feat, k, sortby, descending, dout=None):
        feat = feat.detach().cpu()
        feat = feat if feat.dim() == 2 else feat.unsqueeze(1)
        N, D = feat.shape
        S = len(lens)
        columns = sortby is None
        self.values = torch.zeros(S, k, D)
        self.index = torch.full((S, k, D) if columns else (S, k), -1, dtype=torch.int64)
        self.d_feat = torch.zeros(N, D)
        dout = None if dout is None else dout.detach().cpu()
        o = 0
        for s, n in enumerate(int(v) for v in lens):
            x = feat[o:o + n]
            m = min(k, n)
            if n and columns:
                order = torch.sort(x, dim=0, stable=True, descending=descending).indices[:m]     # [m, D], every column on its own
                self.values[s, :m] = x.gather(0, order)
                self.index[s, :m] = order
                if dout is not None:
                    self.d_feat[o:o + n].index_put_((order, torch.arange(D).expand(m, D)), dout[s, :m])
            elif n:
                order = torch.sort(x[:, sortby], stable=True, descending=descending).indices[:m]
                self.values[s, :m] = x[order]
                self.index[s, :m] = order
                if dout is not None:
                    self.d_feat[o:o + n].index_put_((order,), dout[s, :m])
            o += n
        assert o == N


LENS = [0, 1, 2, 3, 15, 16, 17, 63, 64, 65, 0, 257, 1000, 1023, 1024, 1025, 2049, 5000, 0]   # zeros first, inside and last; below, at and
CPU_LENS = (0, 1, 5, 0, 17, 1, 40, 0)                                                        # above a wave step and a 1024 chunk; several chunks
NEG_NAN = torch.tensor([-4194303], dtype=torch.int32).view(torch.float32)                    # 0xFFC00001: a NaN with the sign bit set
SPECIALS = torch.cat([torch.tensor([0.0, -0.0, float("inf"), -float("inf"), float("nan")]), NEG_NAN])


@functools.lru_cache(maxsize=None)
def operand(lens_key, D, kind, seed=0):
    """[N, D] values of one kind, computed once and shared (never modified)"""
    lens = list(lens_key)
    N = sum(lens)
    gen = torch.Generator().manual_seed(100 * D + seed + len(kind))
    if kind == "normal":
        return torch.randn(N, D, generator=gen)
    if kind == "ties":
        return torch.randint(0, 4, (N, D), generator=gen).float()
    if kind == "equal":
        return torch.full((N, D), 1.5)
    assert kind == "specials"
    x = torch.randn(N, D, generator=gen)
    pick = torch.rand(N, D, generator=gen) < 0.3                                          # scattered through every segment, long and short
    x = torch.where(pick, SPECIALS[torch.randint(0, 6, (N, D), generator=gen)], x)
    ends = np.cumsum(lens)
    for s in [i for i, n in enumerate(lens) if n in (17, 40, 257)]:                       # segments of NaN only, both signs
        x[ends[s] - lens[s]:ends[s]] = torch.where(torch.rand(lens[s], D, generator=gen) < 0.5, NEG_NAN, torch.tensor(float("nan")))
    return x


def run(lens, feat, k, sortby, descending, dout, device, seglen_dtype=torch.int64):
    """forward + backward of ops.segment_topk on `device`: (values, index, d feat)"""
    f = feat.to(device).requires_grad_(True)
    values, index = ops.segment_topk(torch.tensor(lens, dtype=seglen_dtype).to(device), f, k, sortby=sortby, descending=descending,
                                     total=int(feat.shape[0]))
    assert values.requires_grad and not index.requires_grad and index.dtype == torch.int64
    d_feat, = torch.autograd.grad(values, f, dout.to(device))
    return values.detach(), index, d_feat


def check(got, ref, what=""):
    values, index, d_feat = got
    assert tuple(values.shape) == tuple(ref.values.shape) and tuple(index.shape) == tuple(ref.index.shape), what
    assert torch.equal(index.cpu(), ref.index), what
    assert torch.equal(bits(values), bits(ref.values)), what
    assert torch.equal(bits(d_feat), bits(ref.d_feat.view(d_feat.shape))), what


def launches(monkeypatch):
    rec = []
    monkeypatch.setattr(mg.sparse, "PROFILE", rec)
    return rec


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


@pytest.mark.parametrize("kind", ["normal", "ties", "equal", "specials"])
def test_composition_and_its_gradient_match_the_restatement(cpu_backend_on, kind):
    for D in (1, 4, 20):
        feat = operand(CPU_LENS, D, kind)
        for k in (1, 3, 16, 64):
            dout = torch.randn(len(CPU_LENS), k, D, generator=torch.Generator().manual_seed(k))
            for sortby in (0, D - 1, -1, None):
                for descending in (True, False):
                    assert not ops.segment_topk_fused(torch.tensor(CPU_LENS), feat, k, sortby=sortby, descending=descending)
                    got = run(CPU_LENS, feat, k, sortby, descending, dout, "cpu")
                    check(got, Restated(CPU_LENS, feat, k, sortby, descending, dout), (kind, D, k, sortby, descending))
    # a 1-D feature is one column; host lengths need no `total`; int32 lengths
    x = operand(CPU_LENS, 1, kind).view(-1)
    values, index = ops.segment_topk(torch.tensor(CPU_LENS, dtype=torch.int32), x, 4, sortby=0)
    ref = Restated(CPU_LENS, x, 4, 0, True)
    assert tuple(values.shape) == (len(CPU_LENS), 4, 1) and torch.equal(index, ref.index) and torch.equal(bits(values), bits(ref.values))
    assert "segment_topk" in ops.__all__ and "segment_topk_fused" in ops.__all__


def test_no_segments_and_no_rows(cpu_backend_on):
    values, index = ops.segment_topk(torch.zeros(3, dtype=torch.int64), torch.zeros(0, 4), 2)
    assert tuple(values.shape) == (3, 2, 4) and torch.all(values == 0) and tuple(index.shape) == (3, 2, 4) and torch.all(index == -1)
    values, index = ops.segment_topk(torch.zeros(0, dtype=torch.int64), torch.zeros(0, 4), 2, sortby=1)
    assert tuple(values.shape) == (0, 2, 4) and tuple(index.shape) == (0, 2)


def small_graphs(sizes, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for n in sizes:
        e = int(rng.integers(1, 3 * n + 1))
        out.append(mg.graph((torch.from_numpy(rng.integers(0, n, e)), torch.from_numpy(rng.integers(0, n, e))), num_nodes=n))
    return out


def test_topk_nodes_and_edges_on_a_batch_of_five_graphs(cpu_backend_on):
    import dgl
    graphs = small_graphs([3, 1, 7, 4, 9])
    bg = dgl.batch(graphs)
    nn_, ne_ = [g.number_of_nodes() for g in graphs], [g.number_of_edges() for g in graphs]
    gen = torch.Generator().manual_seed(2)
    bg.ndata["h"] = torch.randint(0, 5, (sum(nn_), 6), generator=gen).float()
    bg.edata["h"] = torch.randn(sum(ne_), 3, generator=gen)
    for k in (2, 5):
        for descending in (True, False):
            values, index = dgl.topk_nodes(bg, "h", k, descending=descending)
            ref = Restated(nn_, bg.ndata["h"], k, None, descending)
            assert tuple(values.shape) == (5, k, 6) and tuple(index.shape) == (5, k, 6)
            assert torch.equal(values, ref.values) and torch.equal(index, ref.index)
            values, index = dgl.topk_nodes(bg, "h", k, descending=descending, sortby=-1)
            ref = Restated(nn_, bg.ndata["h"], k, 5, descending)
            assert tuple(values.shape) == (5, k, 6) and tuple(index.shape) == (5, k)
            assert torch.equal(values, ref.values) and torch.equal(index, ref.index)
            values, index = dgl.topk_edges(bg, "h", k, descending=descending, sortby=1)
            ref = Restated(ne_, bg.edata["h"], k, 1, descending)
            assert torch.equal(values, ref.values) and torch.equal(index, ref.index)
            values, index = dgl.topk_edges(bg, "h", k, descending=descending)
            ref = Restated(ne_, bg.edata["h"], k, None, descending)
            assert tuple(index.shape) == (5, k, 3) and torch.equal(values, ref.values) and torch.equal(index, ref.index)
    g = graphs[2]                                                                         # an unbatched graph is one segment
    g.ndata["h"] = bg.ndata["h"][4:11]
    values, index = dgl.topk_nodes(g, "h", 3, sortby=0)
    ref = Restated([7], g.ndata["h"], 3, 0, True)
    assert tuple(values.shape) == (1, 3, 6) and torch.equal(values, ref.values) and torch.equal(index, ref.index)
    for name in ("topk_nodes", "topk_edges"):
        assert name in mg.readout.__all__ and getattr(dgl, name) is getattr(mg.readout, name) is getattr(mg, name)


def test_sort_pooling_values_and_gradient(cpu_backend_on):
    import dgl
    import dgl.nn.pytorch as dglnn
    lens = [3, 1, 7, 4, 9]
    bg = dgl.batch(small_graphs(lens, seed=3))
    feat = torch.randn(24, 6, generator=torch.Generator().manual_seed(4)).requires_grad_(True)
    k = 5
    pool = dglnn.SortPooling(k)
    assert dglnn.glob.SortPooling is mg.nn.SortPooling and dgl.nn.SortPooling is mg.nn.SortPooling and not list(pool.parameters())
    out = pool(bg, feat)
    assert tuple(out.shape) == (5, k * 6)
    up = torch.randn(5, k * 6, generator=torch.Generator().manual_seed(5))
    got_grad, = torch.autograd.grad(out, feat, up)
    twin = feat.detach().clone().requires_grad_(True)
    want = torch.zeros(5, k, 6)
    o = 0
    for s, n in enumerate(lens):                                                          # the loop: sort every node's features, order the
        x = twin[o:o + n].sort(dim=-1).values                                             # graph's nodes by the last one, keep k, pad
        order = torch.sort(x[:, -1], stable=True, descending=True).indices[:k]
        want = want.index_put((torch.tensor(s), torch.arange(len(order))), x[order])
        o += n
    assert torch.equal(bits(out), bits(want.view(5, k * 6)))
    want_grad, = torch.autograd.grad(want.view(5, k * 6), twin, up)
    assert torch.equal(bits(got_grad), bits(want_grad))


def test_argument_errors_raise_dglerror(cpu_backend_on):
    seglen, feat = torch.tensor(CPU_LENS), operand(CPU_LENS, 4, "normal")
    with pytest.raises(mg.DGLError, match="float32"):
        ops.segment_topk(seglen, feat.double(), 2)
    with pytest.raises(mg.DGLError, match=r"\[N\] or \[N, D\]"):
        ops.segment_topk(seglen, feat.view(64, 2, 2), 2)
    with pytest.raises(mg.DGLError, match=r"\[N\] or \[N, D\]"):
        ops.segment_topk(seglen, [1.0, 2.0], 2)
    for k in (0, -1, 2.5, True):
        with pytest.raises(mg.DGLError, match="k must be an integer >= 1"):
            ops.segment_topk(seglen, feat, k)
    for sortby in (4, -5, 1.0):
        with pytest.raises(mg.DGLError, match=r"sortby must be None or a column in \[-4, 4\)"):
            ops.segment_topk(seglen, feat, 2, sortby=sortby)
    with pytest.raises(mg.DGLError, match="63 rows"):
        ops.segment_topk(seglen, feat[:63], 2)
    with pytest.raises(mg.DGLError, match="1-D tensor"):
        ops.segment_topk(list(CPU_LENS), feat, 2)
    with pytest.raises(mg.DGLError, match="different devices"):
        ops.segment_topk(torch.empty(len(CPU_LENS), dtype=torch.int64, device="meta"), feat, 2)
    assert config.SEGMENT_TOPK_FUSED in (True, False)


def test_without_a_cpu_backend_cpu_tensors_fail_loudly(monkeypatch):
    monkeypatch.delitem(mg.sparse._BACKENDS, "cpu", raising=False)
    with pytest.raises(mg.DGLError, match="MI355X"):
        ops.segment_topk(torch.tensor(CPU_LENS), operand(CPU_LENS, 4, "normal"), 2)


def test_abi_argument_checks():
    L = _lib.lib()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("mgx_segment_topk_supported", "mgx_segment_topk_fwd", "mgx_segment_topk_bwd"):
        assert hasattr(handle, name) and name in _lib.SIGNATURES
    assert L.mgx_abi_version() == 35
    for (k, D, mode), want in (((1, 1, 0), 1), ((64, 7, 1), 1), ((65, 100, 0), 1), ((1024, 1, 1), 1), ((1025, 4, 0), 0), ((0, 4, 0), 0),
                               ((4, 0, 1), 0), ((4, 4, 2), 0), ((4, 4, -1), 0)):
        assert L.mgx_segment_topk_supported(k, D, mode) == want, (k, D, mode)
    host = (ctypes.c_float * 64)()                                             # never dereferenced: every call below fails a check first
    p = ctypes.c_void_p(ctypes.addressof(host))

    def fwd(S=2, offsets=p, N=8, D=4, ld=4, feat=p, k=2, mode=0, sortby=0, values=p, index=p, slot=p):
        return L.mgx_segment_topk_fwd(S, offsets, N, D, ld, feat, k, mode, sortby, 1, values, index, slot, None)

    assert fwd(k=0) == 1 and b"k must be at least 1" in L.mgx_last_error()
    with pytest.raises(mg.DGLError, match="k must be at least 1"):
        _lib.check(1)
    assert fwd(k=-3) == 1 and fwd(S=-1) == 1 and fwd(N=-1) == 1 and fwd(D=0) == 1
    assert fwd(ld=3) == 1 and b"row stride" in L.mgx_last_error()
    assert fwd(mode=2) == 1 and b"mode" in L.mgx_last_error()
    assert fwd(sortby=4) == 1 and fwd(sortby=-1) == 1 and b"sortby" in L.mgx_last_error()
    assert fwd(k=1025) == _lib.ERR_UNSUPPORTED and fwd(k=1025, mode=1) == _lib.ERR_UNSUPPORTED
    assert fwd(N=2 ** 31) == _lib.ERR_UNSUPPORTED and fwd(S=2 ** 21, k=1024) == _lib.ERR_UNSUPPORTED
    assert fwd(offsets=None) == 1 and fwd(values=None) == 1 and fwd(index=None) == 1
    assert fwd(feat=None) == 1 and fwd(slot=None) == 1 and b"feat / slot is NULL" in L.mgx_last_error()
    assert fwd(S=0, offsets=None, feat=None, values=None, index=None, slot=None) == 0   # no segments: nothing to do
    bwd = L.mgx_segment_topk_bwd
    assert bwd(8, 0, 0, p, p, p, None) == 1 and bwd(-1, 4, 0, p, p, p, None) == 1 and bwd(8, 4, 2, p, p, p, None) == 1
    assert bwd(8, 4, 0, None, p, p, None) == 1 and bwd(8, 4, 1, p, p, None, None) == 1 and b"slot / d_feat is NULL" in L.mgx_last_error()
    assert bwd(2 ** 31, 4, 0, p, p, p, None) == _lib.ERR_UNSUPPORTED
    assert bwd(0, 4, 0, None, None, None, None) == 0                                        # no rows: nothing to do


def test_script_model_with_the_sortpool_readout_trains_one_tiny_epoch():
    """graph_classification.py's own parser, model and epoch loop on the checker backend (the script's main() asks for a device)"""
    sys.path.insert(0, PKG)
    import graph_classification as gc
    from dgl.dataloading import GraphDataLoader
    from mi355x_graph.datasets import molhiv_like
    args = gc.make_parser().parse_args(["--readout", "sortpool"])
    assert args.sortpool_k == 30 and gc.make_parser().parse_args(["--readout", "sortpool", "--sortpool-k", "7"]).sortpool_k == 7
    layer, width = gc.make_readout("sortpool", 16)
    assert isinstance(layer, mg.nn.SortPooling) and layer.k == 30 and width == 30 * 16
    oracle_backend.install()
    try:
        torch.manual_seed(0)
        for net in (gc.GCN, gc.GIN):
            model = net(16, 1, 2, 0.0, readout="sortpool", sortpool_k=7)
            assert tuple(model.graph_pred_fc.weight.shape) == (1, 7 * 16)
            loader = GraphDataLoader(molhiv_like(24, seed=3), batch_size=8, shuffle=False)
            loss = gc.train_epoch(model, torch.device("cpu"), loader, torch.optim.Adam(model.parameters(), lr=1e-3), torch.nn.BCEWithLogitsLoss())
            assert np.isfinite(loss)
            assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    finally:
        oracle_backend.uninstall()


# ----------------------------------------------------------------------------- GPU: the kernels against the restatement
#        k     D   sortby descending kind
CASES = [(1, 1, 0, True, "normal"),
         (1, 4, None, False, "ties"),
         (2, 20, -1, True, "specials"),
         (2, 1, None, True, "specials"),
         (3, 64, 63, False, "normal"),
         (3, 100, None, True, "ties"),
         (16, 4, 0, True, "equal"),
         (16, 20, None, False, "specials"),
         (63, 64, -1, False, "ties"),
         (63, 4, None, True, "normal"),
         (64, 100, 99, True, "specials"),
         (64, 20, None, True, "equal"),
         (64, 64, None, False, "specials"),
         (65, 1, -1, False, "specials"),
         (65, 64, None, False, "normal"),
         (128, 20, 0, True, "ties"),
         (128, 4, None, True, "specials"),
         (1000, 64, 0, False, "specials"),
         (1000, 1, None, True, "ties"),
         (1024, 100, -1, True, "normal"),
         (1024, 20, None, False, "equal"),
         (1024, 4, 3, True, "ties"),
         (1024, 1, 0, False, "specials")]


@functools.lru_cache(maxsize=None)
def gpu_case(k, D, sortby, descending, kind, lens_key=tuple(LENS)):
    feat = operand(lens_key, D, kind)
    dout = torch.randn(len(lens_key), k, D, generator=torch.Generator().manual_seed(k + D))
    return feat, dout, Restated(lens_key, feat, k, sortby, descending, dout)


@pytest.mark.gpu
@pytest.mark.parametrize("k,D,sortby,descending,kind", CASES)
def test_kernels_match_the_restatement(monkeypatch, k, D, sortby, descending, kind):
    feat, dout, ref = gpu_case(k, D, sortby, descending, kind)
    seglen_dtype = torch.int32 if (k + D) % 2 else torch.int64
    assert ops.segment_topk_fused(torch.tensor(LENS, dtype=seglen_dtype).to(DEV), feat.to(DEV), k, sortby=sortby, descending=descending)
    rec = launches(monkeypatch)
    got = run(LENS, feat, k, sortby, descending, dout, DEV, seglen_dtype)
    assert [r["kernel"] for r in rec] == ["seg_topk_fwd", "seg_topk_bwd"]       # one launch each way, nothing else from the library
    check(got, ref)
    if kind == "equal":                                                         # all keys equal: the rows in their own order
        index = got[1].cpu()
        for s, n in enumerate(LENS):
            m = min(k, n)
            want = torch.arange(m).view((m,) + (1,) * (index.dim() - 2)).expand(index[s, :m].shape)
            assert torch.equal(index[s, :m], want) and torch.all(index[s, m:] == -1)
    again = run(LENS, feat, k, sortby, descending, dout, DEV, seglen_dtype)     # reruns give identical bits
    for a, b in zip(got, again):
        assert torch.equal(bits(a) if a.dtype == torch.float32 else a.cpu(), bits(b) if b.dtype == torch.float32 else b.cpu())


@pytest.mark.gpu
def test_zero_length_segments_last_and_a_single_segment():
    lens = LENS[1:12] + [0, 0]
    for k, sortby in ((30, -1), (200, None)):
        feat = operand(tuple(lens), 20, "specials")
        dout = torch.randn(len(lens), k, 20, generator=torch.Generator().manual_seed(k))
        check(run(lens, feat, k, sortby, True, dout, DEV), Restated(lens, feat, k, sortby, True, dout), (k, sortby))
    feat = operand((3000,), 4, "ties")
    for k in (8, 100):
        dout = torch.randn(1, k, 4, generator=torch.Generator().manual_seed(k))
        check(run([3000], feat, k, 1, False, dout, DEV), Restated([3000], feat, k, 1, False, dout), k)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ties", "specials"])
def test_k_above_1024_takes_the_composition(monkeypatch, kind):
    feat, dout, ref = gpu_case(1025, 4, None if kind == "ties" else -1, kind == "ties", kind)
    seglen = torch.tensor(LENS).to(DEV)
    assert not ops.segment_topk_fused(seglen, feat.to(DEV), 1025, sortby=None if kind == "ties" else -1)
    assert ops.segment_topk_fused(seglen, feat.to(DEV), 1024, sortby=None if kind == "ties" else -1)
    rec = launches(monkeypatch)
    check(run(LENS, feat, 1025, None if kind == "ties" else -1, kind == "ties", dout, DEV), ref)
    assert not any(r["kernel"].startswith("seg_topk") for r in rec)


@pytest.mark.gpu
def test_switch_off_takes_the_composition_with_the_same_bits(monkeypatch):
    feat, dout, ref = gpu_case(64, 64, None, False, "specials")
    monkeypatch.setattr(config, "SEGMENT_TOPK_FUSED", False)
    assert not ops.segment_topk_fused(torch.tensor(LENS).to(DEV), feat.to(DEV), 64)
    rec = launches(monkeypatch)
    check(run(LENS, feat, 64, None, False, dout, DEV), ref)
    assert not any(r["kernel"].startswith("seg_topk") for r in rec)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [30, 200])
def test_strided_operand_equals_the_contiguous_one(monkeypatch, k):
    wide = operand(tuple(LENS), 100, "specials").to(DEV)
    block = wide[:, 10:74]                                                      # D = 64, row stride 100, base 40 bytes into a row
    dense = block.contiguous()
    assert not block.is_contiguous()
    dout = torch.randn(len(LENS), k, 64, generator=torch.Generator().manual_seed(k))
    for sortby in (5, None):
        ref = Restated(LENS, dense, k, sortby, True, dout)
        rec = launches(monkeypatch)
        got = run(LENS, block, k, sortby, True, dout, DEV)
        assert [r["kernel"] for r in rec] == ["seg_topk_fwd", "seg_topk_bwd"]
        check(got, ref)
        check(run(LENS, dense, k, sortby, True, dout, DEV), ref)
    odd = wide.t()[10:74].t()[:, ::2]                                           # a column stride of 2: copied, same result
    dout = torch.randn(len(LENS), k, 32, generator=torch.Generator().manual_seed(k))
    check(run(LENS, odd, k, 3, False, dout, DEV), Restated(LENS, odd.contiguous(), k, 3, False, dout))


@pytest.mark.gpu
def test_forward_and_backward_captured_in_a_hip_graph():
    """the capture idiom of tests/test_graphed_batches.py / GraphedBatchTrainer: warm-up and capture on ONE side stream, then replay with
    new feature values in the static input -- the operator reads nothing back to the host"""
    lens = LENS[:14]
    N = sum(lens)
    seglen = torch.tensor(lens).to(DEV)
    static = operand(tuple(lens), 20, "normal").to(DEV).requires_grad_(True)
    outs = {}

    def step():
        static.grad = None
        for name, k, sortby in (("rows", 30, -1), ("columns", 100, None)):
            values, index = ops.segment_topk(seglen, static, k, sortby=sortby, total=N)
            values.backward(outs.setdefault("up_" + name, torch.randn(values.shape, device=DEV)))
            outs[name] = (values, index)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), ops.warming_up_for_capture():
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    static.grad = None
    with torch.cuda.graph(graph, stream=side):
        step()
    new = operand(tuple(lens), 20, "specials")
    with torch.no_grad():
        static.copy_(new.to(DEV))
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    want_grad = torch.zeros(N, 20)
    for name, k, sortby in (("rows", 30, -1), ("columns", 100, None)):
        ref = Restated(lens, new, k, sortby, True, outs["up_" + name])
        values, index = outs[name]
        assert torch.equal(index.cpu(), ref.index) and torch.equal(bits(values), bits(ref.values))
        want_grad = want_grad + ref.d_feat                                      # a sum of two exact gradients: one fp32 addition per element
    assert torch.equal(bits(static.grad), bits(want_grad))


def _forty_graphs(width, seed=0):
    import dgl
    from mi355x_graph.datasets import molhiv_like
    data = molhiv_like(40, seed=17)
    bg = dgl.batch([data[i][0] for i in range(40)])
    gen = torch.Generator().manual_seed(seed)
    return bg, torch.randn(bg.number_of_nodes(), width, generator=gen)


@pytest.mark.gpu
def test_layers_on_the_device(monkeypatch):
    import dgl
    bg, feat = _forty_graphs(16)
    lens = [int(v) for v in bg.batch_num_nodes()]
    dbg = bg.to(DEV)
    dbg.ndata["h"] = feat.to(DEV)
    rec = launches(monkeypatch)
    values, index = dgl.topk_nodes(dbg, "h", 10, sortby=2)
    assert [r["kernel"] for r in rec] == ["seg_topk_fwd"]
    ref = Restated(lens, feat, 10, 2, True)
    assert torch.equal(index.cpu(), ref.index) and torch.equal(bits(values), bits(ref.values))
    x = feat.to(DEV).requires_grad_(True)
    up = torch.randn(40, 10 * 16, generator=torch.Generator().manual_seed(1))
    out = mg.nn.SortPooling(10)(dbg, x)
    got_grad, = torch.autograd.grad(out, x, up.to(DEV))
    twin = feat.clone().requires_grad_(True)
    srt = twin.sort(dim=-1).values
    sref = Restated(lens, srt, 10, 15, True)
    want = torch.zeros(40, 10, 16)
    o = 0
    for s, n in enumerate(lens):
        m = min(10, n)
        want = want.index_put((torch.tensor(s), torch.arange(m)), srt[o + sref.index[s, :m]])
        o += n
    want_grad, = torch.autograd.grad(want.view(40, 160), twin, up)
    assert torch.equal(bits(out), bits(want.view(40, 160))) and torch.equal(bits(got_grad), bits(want_grad))


@functools.lru_cache(maxsize=None)
def _script(*args):
    """(loss printed for epoch 1, whole output) of one run of the script"""
    env = dict(os.environ, MGX_DATASET_SCALE="0.01", PYTHONPATH=PKG)
    cmd = [sys.executable, os.path.join(PKG, "graph_classification.py"), "--num_graphs", "320", "--batch_size", "64", "--epochs", "1",
           "--emb_dim", "64", "--num_layers", "2"] + list(args)
    res = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert res.returncode == 0, res.stdout[-3000:]
    m = re.search(r"epoch 1 loss (\S+)", res.stdout)
    assert m, res.stdout[-3000:]
    return m.group(1), res.stdout


@pytest.mark.gpu
def test_script_sortpool_readout_under_hipgraph_trains_to_a_finite_loss():
    """five batches of 64 molecules, padded to one static shape and replayed: the [B, k * D] readout is captured as it is"""
    loss, text = _script("--readout", "sortpool", "--hipgraph")
    assert np.isfinite(float(loss)), text[-2000:]
    replayed = re.search(r"(\d+) steps replayed", text)
    assert replayed and int(replayed.group(1)) >= 5, text[-2000:]
