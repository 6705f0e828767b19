"""Query-set k nearest neighbours: csrc/knn.hip (mgx_segment_knn_query), ops.segment_knn_query / segment_knn_query_fused,
transform.knn_block / knn_interpolate, nn.FeaturePropagation, pointnet2_seg.py.

The reference everywhere is the restatement below, a Python loop over the segments and never the code under test:

    d64 = ((y_s[:, None] - x_s[None]) ** 2).sum(-1) in fp64;  torch.sort(d64, dim=1, stable=True);  index -1 / dist +inf past the
    reference segment's end;  w64 = (1 / (d + eps)) / sum over the valid ranks, 0 at a padded rank, in fp64 (eps is the float the C ABI
    takes: float32(1e-8))

  exact   integer coordinates in [-3, 3]: every distance is an integer below 2^24, exact in fp32 in any order -- torch.equal on the
          index (ties are everywhere, so "equal distances keep the lower row" is what is tested), bit equality on dist; each weight
          carries at most k + 3 roundings (d + eps, the reciprocal, at most k - 1 of the sum, the division; eps itself), doubled in
          case the division is by reciprocal: within (k + 3) 2^-23 relative of w64; padded weights exactly 0
  float   normal / row-scaled / a cluster at 1000 + 1e-3 randn: the bounds tests/test_knn.py derives -- for every query and rank
          |d64(q, got[q, r]) - d64_sorted[q, r]| <= (D + 2) 2^-23 d64_sorted[q, r], dist within (D + 2) 2^-24 relative of d64
  interpolation   against the dense fp64 W64 @ f.  Integer coordinates (the index is exact): forward within (2k + 8) 2^-24 max|f| over
          the query's k neighbours (the weights sum to 1), the gradient to feat within (T + 8) 2^-23 A as tests/test_broadcast_grad.py
          (T the most edges leaving one source, A the sum of |w| |g|).  Float coordinates: only queries whose reference gap between
          ranks k - 1 and k exceeds twice the distance bound are compared (at most 5 %% left out, asserted on the restatement alone); the
          fp32 distances then move every weight by another 2 (D + 2) 2^-24 relative, which both bounds gain
  layer   FeaturePropagation against its fp64 restatement: the interpolation bound pushed through every Linear with absolute values
          (e_out = e_in |W|^T + (n + 3) 2^-24 (|h| |W|^T + |b|)); gradients within (T + 8) 2^-23 A with A from the same expression over
          absolute values (the ReLU masks held) and T the sum of every summation length on the path; the inputs are picked so that no
          pre-activation of the reference lies within twice its bound of 0 (asserted), so no mask can differ"""
import ctypes
import functools
import math
import os
import re
import subprocess
import sys

import pytest
import torch

import mi355x_graph as mg
import mi355x_graph.nn  # noqa: F401
from mi355x_graph import _lib, config, ops, sparse
import oracle_backend

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dgl-0.5-benchmark_amd")
DEV = "cuda:0"
INF = float("inf")
NAN = float("nan")
EPS = 1e-8
EPS32 = float(torch.tensor(EPS, dtype=torch.float32))


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ----------------------------------------------------------------------------- the restatement (a loop over segments, never the code under test)
class Restated(object):
    """d64: per segment the fp64 distance matrix [queries, references]; order / sorted: its stable sort.  index(k) / dist(k) /
    weight(k): the padded outputs."""

    def __init__(self, ref_lens, x, query_lens, y):
        x, y = x.detach().cpu().double(), y.detach().cpu().double()
        self.ref_lens, self.query_lens = [int(n) for n in ref_lens], [int(n) for n in query_lens]
        assert len(self.ref_lens) == len(self.query_lens)
        self.N, self.M = int(x.shape[0]), int(y.shape[0])
        self.d64, self.order, self.sorted = [], [], []
        o = p = 0
        for n, m in zip(self.ref_lens, self.query_lens):
            xs, ys = x[o:o + n], y[p:p + m]
            d = torch.cat([((ys[q:q + 16, None] - xs[None]) ** 2).sum(-1) for q in range(0, m, 16)]) if m else torch.zeros(0, n, dtype=torch.float64)
            srt = torch.sort(d, dim=1, stable=True)
            self.d64.append(d)
            self.order.append(srt.indices)
            self.sorted.append(srt.values)
            o, p = o + n, p + m
        assert o == self.N and p == self.M

    def _padded(self, k, fill, dtype, pick):
        out = torch.full((self.M, k), fill, dtype=dtype)
        o = p = 0
        for s, (n, m) in enumerate(zip(self.ref_lens, self.query_lens)):
            out[p:p + m, :min(k, n)] = pick(s, o)[:, :k]
            o, p = o + n, p + m
        return out

    def index(self, k):
        return self._padded(k, -1, torch.int64, lambda s, o: self.order[s] + o)

    def dist(self, k):
        return self._padded(k, INF, torch.float64, lambda s, o: self.sorted[s])

    def weight(self, k, eps=EPS32):
        valid, zero = self.index(k) >= 0, torch.zeros((), dtype=torch.float64)
        inv = torch.where(valid, 1.0 / (self.dist(k) + eps), zero)
        return torch.where(valid, inv / inv.sum(1, keepdim=True), zero)

    def dense(self, k):
        """W64 [M, N]: the interpolation as a matrix"""
        index, w = self.index(k), self.weight(k)
        assert int(index.min()) >= 0
        return torch.zeros(self.M, self.N, dtype=torch.float64).index_put_((torch.arange(self.M).repeat_interleave(k), index.flatten()),
                                                                        w.flatten(), accumulate=True)


REF_LENS = (0, 1, 2, 3, 4, 63, 64, 65, 130, 300)     # empty; below, at and above k; one and several 64-row chunks
QUERY_LENS = (5, 0, 17, 16, 1, 33, 15, 64, 3, 40)    # queries over nothing; nothing over references; 16-row tiles that straddle segments
KS = (1, 3, 8, 64)
DS = (1, 3, 4, 33, 64, 256)
FLOAT_REF_LENS = (20, 21, 64, 65, 130, 300)
FLOAT_QUERY_LENS = (5, 17, 16, 33, 15, 64)


@functools.lru_cache(maxsize=None)
def int_points(lens, D, seed=0):
    return torch.randint(-3, 4, (sum(lens), D), generator=torch.Generator().manual_seed(1000 * D + seed)).float()


@functools.lru_cache(maxsize=None)
def int_case(D):
    x, y = int_points(REF_LENS, D), int_points(QUERY_LENS, D, seed=1)
    return x, y, Restated(REF_LENS, x, QUERY_LENS, y)


@functools.lru_cache(maxsize=None)
def nan_case():
    """one NaN reference row (in the segment of 4: a rank below k = 8 there, beyond k = 3) and one NaN query row (over the segment of 65)"""
    x, y = int_points(REF_LENS, 4, seed=2).clone(), int_points(QUERY_LENS, 4, seed=3).clone()
    x[sum(REF_LENS[:4]) + 1, 2] = NAN
    y[sum(QUERY_LENS[:7]) + 20, 0] = NAN
    return x, y, Restated(REF_LENS, x, QUERY_LENS, y)


def check_exact(got, ref, k, what=""):
    got_index, got_dist, got_weight = got
    assert got_index.dtype == torch.int64 and tuple(got_index.shape) == (ref.M, k), what
    want_index = ref.index(k)
    assert torch.equal(got_index.cpu(), want_index), what
    if got_dist is not None:
        want, d = ref.dist(k), got_dist.cpu()
        assert d.dtype == torch.float32 and not got_dist.requires_grad and tuple(d.shape) == (ref.M, k), what
        assert torch.equal(torch.isnan(d), torch.isnan(want)), what           # a NaN distance is a NaN (whatever its bits), in the same places
        assert torch.equal(bits(d.nan_to_num(nan=-1.0)), bits(want.float().nan_to_num(nan=-1.0))), what
    if got_weight is not None:
        want, w = ref.weight(k), got_weight.cpu()
        assert w.dtype == torch.float32 and not got_weight.requires_grad and tuple(w.shape) == (ref.M, k), what
        valid = want_index >= 0
        assert bool((w[~valid] == 0).all()), what                               # padded ranks: exactly 0
        assert torch.equal(torch.isnan(w), torch.isnan(want)), what             # NaN where the definition says so, and nowhere else
        fin = valid & ~torch.isnan(want)
        err, bound = (w.double() - want).abs()[fin], (k + 3) * 2.0 ** -23 * want[fin]
        assert bool((err <= bound).all()), "%s: weight off by %g of the bound" % (what, float((err / bound.clamp(min=1e-300)).max()))


def query(ref_lens, x, query_lens, y, k, device, return_dist=True, return_weight=True, seglen_dtype=torch.int64, eps=EPS):
    return ops.segment_knn_query(torch.tensor(ref_lens, dtype=seglen_dtype).to(device), x.to(device),
                                 torch.tensor(query_lens, dtype=seglen_dtype).to(device), y.to(device), k, ref_total=int(x.shape[0]),
                                 query_total=int(y.shape[0]), return_dist=return_dist, return_weight=return_weight, eps=eps)


def fused(ref_lens, x, query_lens, y, k, device=DEV):
    return ops.segment_knn_query_fused(torch.tensor(ref_lens).to(device), x.to(device), torch.tensor(query_lens).to(device), y.to(device), k)


def leaf(t, device):
    """a fresh leaf on the device (the cached case tensors stay as they are)"""
    return t.to(device).clone().requires_grad_(True)


def launches(monkeypatch):
    rec = []
    monkeypatch.setattr(mg.sparse, "PROFILE", rec)
    return rec


# ----------------------------------------------------------------------------- float cases
@functools.lru_cache(maxsize=None)
def float_case(D, kind):
    gen = torch.Generator().manual_seed(11 * D + len(kind))
    N, M = sum(FLOAT_REF_LENS), sum(FLOAT_QUERY_LENS)
    x, y = torch.randn(N, D, generator=gen), torch.randn(M, D, generator=gen)
    if kind == "scaled":
        x, y = x * torch.exp(4 * torch.randn(N, 1, generator=gen)), y * torch.exp(4 * torch.randn(M, 1, generator=gen))
    elif kind == "cluster":
        x, y = 1000 + 1e-3 * x, 1000 + 1e-3 * y
    else:
        assert kind == "normal"
    return x, y, Restated(FLOAT_REF_LENS, x, FLOAT_QUERY_LENS, y)


def check_float(got_index, got_dist, ref, k, D, what=""):
    index, dist = got_index.cpu(), got_dist.cpu().double()
    o = p = 0
    worst = 0.0
    for n, m, d64, srt in zip(ref.ref_lens, ref.query_lens, ref.d64, ref.sorted):
        idx = index[p:p + m]
        assert bool(((idx >= o) & (idx < o + n)).all()), what                         # inside the query's own reference segment (n >= k here)
        assert bool((idx.sort(dim=1).values.diff(dim=1) > 0).all()), what             # no index twice in a row
        at = d64.gather(1, idx - o)                                                   # fp64 distance of what was returned
        want = srt[:, :k]
        err, bound = (at - want).abs(), (D + 2) * 2.0 ** -23 * want
        assert bool((err <= bound).all()), "%s: rank distance off by %g of the bound" % (what, float((err / bound.clamp(min=1e-300)).max()))
        worst = max(worst, float((err / bound.clamp(min=1e-300)).max()))
        derr, dbound = (dist[p:p + m] - at).abs(), (D + 2) * 2.0 ** -24 * at
        assert bool((derr <= dbound).all()), "%s: dist off by %g of the bound" % (what, float((derr / dbound.clamp(min=1e-300)).max()))
        o, p = o + n, p + m
    print("knn query float %s: worst rank-distance error / bound %.3f" % (what, worst))


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


def test_restatement_by_hand():
    x = torch.tensor([[0.], [2.], [5.], [1.]])
    y = torch.tensor([[1.], [4.], [0.]])
    ref = Restated([3, 1], x, [2, 1], y)
    assert ref.index(2).tolist() == [[0, 1], [2, 1], [3, -1]]                    # 1 is as far from 0 as from 2: the lower row first
    assert ref.dist(2).tolist() == [[1., 1.], [1., 4.], [1., INF]]
    w = ref.weight(2, eps=0.0)
    assert torch.allclose(w, torch.tensor([[0.5, 0.5], [0.8, 0.2], [1.0, 0.0]], dtype=torch.float64), atol=1e-15)
    assert torch.allclose(ref.dense(1), torch.tensor([[1., 0, 0, 0], [0, 0, 1., 0], [0, 0, 0, 1.]], dtype=torch.float64))


@pytest.mark.parametrize("D", DS)
def test_composition_matches_the_restatement_exactly(cpu_backend_on, D):
    x, y, ref = int_case(D)
    assert not fused(REF_LENS, x, QUERY_LENS, y, 3, "cpu")
    for k in KS:
        got = query(REF_LENS, x, QUERY_LENS, y, k, "cpu", seglen_dtype=torch.int32 if k % 2 else torch.int64)
        check_exact(got, ref, k, (D, k))
    only = query(REF_LENS, x, QUERY_LENS, y, 3, "cpu", return_dist=False, return_weight=False)
    assert torch.is_tensor(only) and torch.equal(only, ref.index(3))
    index, weight = query(REF_LENS, x, QUERY_LENS, y, 3, "cpu", return_dist=False)
    check_exact((index, None, weight), ref, 3, "index and weight")


def test_composition_nan_strided_and_self(cpu_backend_on):
    x, y, ref = nan_case()
    for k in (3, 8):
        check_exact(query(REF_LENS, x, QUERY_LENS, y, k, "cpu"), ref, k, ("nan", k))
    assert bool(torch.isnan(ref.weight(8)).any()) and bool(torch.isnan(ref.dist(8)).any())
    wide_x, wide_y = int_points(REF_LENS, 9), int_points(QUERY_LENS, 7, seed=1)
    bx, by = wide_x[:, 2:6], wide_y[:, 1:5]
    assert not bx.is_contiguous() and not by.is_contiguous()
    check_exact(query(REF_LENS, bx, QUERY_LENS, by, 8, "cpu"), Restated(REF_LENS, bx, QUERY_LENS, by), 8, "strided")
    x = int_points(REF_LENS, 3)
    index, dist = query(REF_LENS, x, REF_LENS, x, 8, "cpu", return_weight=False)
    self_index, self_dist = ops.segment_knn(torch.tensor(REF_LENS), x, 8, return_dist=True)
    assert torch.equal(index, self_index) and torch.equal(bits(dist), bits(self_dist))


@pytest.mark.parametrize("kind", ["normal", "scaled", "cluster"])
def test_composition_float_cases(cpu_backend_on, kind):
    for D in (1, 3, 64, 128):
        x, y, ref = float_case(D, kind)
        index, dist, _ = query(FLOAT_REF_LENS, x, FLOAT_QUERY_LENS, y, 20, "cpu")
        check_float(index, dist, ref, 20, D, "composition %s D=%d" % (kind, D))


def test_no_rows_no_segments_and_argument_errors(cpu_backend_on):
    none = torch.zeros(0, dtype=torch.int64)
    index, dist, weight = ops.segment_knn_query(none, torch.zeros(0, 3), none, torch.zeros(0, 3), 4, return_dist=True, return_weight=True)
    assert tuple(index.shape) == (0, 4) and tuple(dist.shape) == (0, 4) and tuple(weight.shape) == (0, 4)
    index, dist, weight = ops.segment_knn_query(torch.tensor([0, 0]), torch.zeros(0, 3), torch.tensor([2, 1]), torch.ones(3, 3), 2,
                                                return_dist=True, return_weight=True)                   # queries over nothing: all padding
    assert torch.equal(index, torch.full((3, 2), -1)) and bool((dist == INF).all()) and bool((weight == 0).all())
    x, y = int_points((5, 7), 3), int_points((2, 3), 3, seed=1)
    r, q = torch.tensor([5, 7]), torch.tensor([2, 3])
    for bad in (lambda: ops.segment_knn_query(r, x, q, y, 0), lambda: ops.segment_knn_query(r, x, q, y, True),
                lambda: ops.segment_knn_query(r, x, q, y, 2.0), lambda: ops.segment_knn_query(torch.tensor([5, 6]), x, q, y, 2),
                lambda: ops.segment_knn_query(r, x, torch.tensor([2, 2]), y, 2), lambda: ops.segment_knn_query(r, x, torch.tensor([2, 2, 1]), y, 2),
                lambda: ops.segment_knn_query(r, x.double(), q, y, 2), lambda: ops.segment_knn_query(r, x, q, y.double(), 2),
                lambda: ops.segment_knn_query(r, x[:, 0], q, y, 2), lambda: ops.segment_knn_query(r, x, q, y[:, :2], 2),
                lambda: ops.segment_knn_query([5, 7], x, q, y, 2), lambda: ops.segment_knn_query(r, x, q, y, 2, eps=-1.0),
                lambda: ops.segment_knn_query(r, x, q, y, 2, eps=NAN), lambda: ops.segment_knn_query(r, x, q, y, 2, eps="1")):
        with pytest.raises(mg.DGLError):
            bad()


def test_without_a_cpu_backend_cpu_tensors_fail_loudly(monkeypatch):
    monkeypatch.delitem(mg.sparse._BACKENDS, "cpu", raising=False)
    with pytest.raises(mg.DGLError, match="MI355X"):
        ops.segment_knn_query(torch.tensor([5, 7]), int_points((5, 7), 3), torch.tensor([2, 3]), int_points((2, 3), 3), 2)


def test_abi_argument_checks():
    L = _lib.lib()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("mgx_segment_knn_query_supported", "mgx_segment_knn_query"):
        assert hasattr(handle, name) and name in _lib.SIGNATURES
    assert L.mgx_abi_version() == 35
    assert config.KNN_QUERY_FUSED is True
    for (k, D), want in (((1, 1), 1), ((64, 256), 1), ((3, 3), 1), ((65, 3), 0), ((3, 257), 0), ((0, 3), 0), ((3, 0), 0), ((-1, 3), 0)):
        assert L.mgx_segment_knn_query_supported(k, D) == want, (k, D)
    host = (ctypes.c_float * 64)()                                             # never dereferenced: every call below fails a check first
    p = ctypes.c_void_p(ctypes.addressof(host))

    def call(S=2, offsets=p, N=8, ld=4, x=p, q_offsets=p, M=6, ldq=4, y=p, D=4, k=2, eps=1e-8, index=p, dist=p, weight=p):
        return L.mgx_segment_knn_query(S, offsets, N, ld, x, q_offsets, M, ldq, y, D, k, eps, index, dist, weight, None)

    assert call(k=0) == 1 and b"k must be at least 1" in L.mgx_last_error()
    assert call(k=-3) == 1 and call(S=-1) == 1 and call(N=-1) == 1 and call(M=-1) == 1 and call(D=0) == 1
    assert call(ld=3) == 1 and b"row stride" in L.mgx_last_error()
    assert call(ldq=3) == 1 and b"row stride" in L.mgx_last_error()
    assert call(k=65) == _lib.ERR_UNSUPPORTED and call(D=257, ld=257, ldq=257) == _lib.ERR_UNSUPPORTED
    assert call(N=2 ** 31) == _lib.ERR_UNSUPPORTED and call(M=2 ** 31) == _lib.ERR_UNSUPPORTED and call(S=2 ** 31) == _lib.ERR_UNSUPPORTED
    assert call(N=2 ** 28) == _lib.ERR_UNSUPPORTED and call(M=2 ** 28) == _lib.ERR_UNSUPPORTED          # 4 GiB of x; of y
    for null in ("offsets", "x", "q_offsets", "y", "index"):
        assert call(**{null: None}) == 1 and b"is NULL" in L.mgx_last_error(), null
    assert call(M=0, offsets=None, x=None, q_offsets=None, y=None, index=None, dist=None, weight=None) == 0   # no queries: nothing to do


# ----------------------------------------------------------------------------- the block builder and the interpolation
BLOCK_REF, BLOCK_QUERY, BLOCK_K = (8, 5, 20), (12, 0, 30), 3


def check_block(device):
    import dgl
    import dgl.geometry
    x, y = int_points(BLOCK_REF, 3, seed=6), int_points(BLOCK_QUERY, 3, seed=7)
    ref = Restated(BLOCK_REF, x, BLOCK_QUERY, y)
    N, M, k = ref.N, ref.M, BLOCK_K
    block = dgl.geometry.knn_block(x.to(device), list(BLOCK_REF), y.to(device), list(BLOCK_QUERY), k)
    assert block.is_block and block.number_of_src_nodes() == N and block.number_of_dst_nodes() == M
    assert block.number_of_edges() == M * k and block.idtype == torch.int32
    assert block._index.format_status() == {"created": ["csc"], "not created": ["coo", "csr"]}         # the in-CSR, without a conversion
    csc = block._index.csc()
    assert torch.equal(csc.indptr.cpu().long(), torch.arange(M + 1) * k) and csc.eids is None
    assert block._index.max_in_degree_hint == k and block._index.plain_transpose
    assert torch.equal(csc.indices.cpu().long().view(-1, k), ref.index(k))
    w = block.edata["w"]
    assert tuple(w.shape) == (M * k,) and not w.requires_grad
    check_exact((ref.index(k), None, w.view(M, k)), ref, k, "edata w")
    assert torch.equal(block.srcdata["pos"].cpu(), x) and torch.equal(block.dstdata["pos"].cpu(), y)
    for bad in (lambda: dgl.geometry.knn_block(x, [8, 5, 20], y, [12, 0, 30], 6),                     # a reference set of 5 has no 6 neighbours
                lambda: dgl.geometry.knn_block(x, [8, 5, 19], y, [12, 0, 30], 3),
                lambda: dgl.geometry.knn_block(x, [8, 5, 20], y, [12, 30], 3),
                lambda: dgl.geometry.knn_block(x, [8, 5, 20], y, [12, 1, 30], 3),
                lambda: dgl.geometry.knn_block(x, [8, 5, 20], y, [12, 0, 30], 0),
                lambda: dgl.geometry.knn_block(x, [8, 5, 20], y[:, :2], [12, 0, 30], 3),
                lambda: dgl.geometry.knn_block(x.long(), [8, 5, 20], y, [12, 0, 30], 3),
                lambda: dgl.geometry.knn_block(x[:, 0], [8, 5, 20], y, [12, 0, 30], 3),
                lambda: dgl.geometry.knn_interpolate(torch.zeros(5, 2), x, y, [8, 5, 20], [12, 0, 30])):
        with pytest.raises(mg.DGLError):
            bad()


def test_block_builder(cpu_backend_on):
    check_block("cpu")


INTERP_REF, INTERP_QUERY = (40, 72), (100, 33)


@functools.lru_cache(maxsize=None)
def interp_case(kind, C):
    """(x, y, restatement, feat, upstream g, kept queries, extra weight roundings in units of 2^-24)"""
    gen = torch.Generator().manual_seed(50 + C + len(kind))
    k, D = BLOCK_K, 3
    if kind == "integer":
        x, y = int_points(INTERP_REF, D, seed=8), int_points(INTERP_QUERY, D, seed=9)
    else:
        x, y = torch.randn(sum(INTERP_REF), D, generator=gen), torch.randn(sum(INTERP_QUERY), D, generator=gen)
    ref = Restated(INTERP_REF, x, INTERP_QUERY, y)
    feat, g = torch.randn(ref.N, C, generator=gen), torch.randn(ref.M, C, generator=gen)
    if kind == "integer":
        return x, y, ref, feat, g, torch.ones(ref.M, dtype=torch.bool), 0
    srt = torch.cat([s[:, :k + 1] for s in ref.sorted])
    keep = srt[:, k] - srt[:, k - 1] > 2 * (D + 2) * 2.0 ** -23 * srt[:, k]      # the k-th and the (k + 1)-th cannot change places
    return x, y, ref, feat, g * keep.unsqueeze(1), keep, 2 * (D + 2)


def test_float_interpolation_inputs_meet_the_cap():
    for C in (5, 64):
        keep = interp_case("float", C)[5]
        assert float((~keep).float().mean()) <= 0.05


def check_interpolate(device, kind):
    import dgl.geometry
    k = BLOCK_K
    for C in (5, 64):
        x, y, ref, feat, g, keep, extra = interp_case(kind, C)
        W = ref.dense(k)
        f, xx, yy = leaf(feat, device), leaf(x, device), leaf(y, device)
        out = dgl.geometry.knn_interpolate(f, xx, yy, list(INTERP_REF), list(INTERP_QUERY), k)
        assert tuple(out.shape) == (ref.M, C)
        out.backward(g.to(device))
        assert xx.grad is None and yy.grad is None                               # the weights are constants: the gradient flows to feat only
        want = W @ feat.double()
        top = feat.double().abs()[ref.index(k)].max(1).values                    # max |f| over the query's neighbours, per column
        err, bound = (out.detach().cpu().double() - want).abs()[keep], ((2 * k + 8 + extra) * 2.0 ** -24 * top)[keep]
        assert bool((err <= bound).all()), "%s C=%d: forward %g of the bound" % (kind, C, float((err / bound.clamp(min=1e-300)).max()))
        gwant, A = W.t() @ g.double(), W.abs().t() @ g.double().abs()
        T = int(torch.bincount(ref.index(k).flatten(), minlength=ref.N).max())
        gerr, gbound = (f.grad.cpu().double() - gwant).abs(), (T + 8 + extra / 2) * 2.0 ** -23 * A
        assert bool((gerr <= gbound).all()), "%s C=%d: gradient %g of the bound" % (kind, C, float((gerr / gbound.clamp(min=1e-300)).max()))
        print("knn_interpolate %s C=%d on %s: forward %.3f, gradient %.3f of the bound" % (
            kind, C, device, float((err / bound.clamp(min=1e-300)).max()), float((gerr / gbound.clamp(min=1e-300)).max())))


@pytest.mark.parametrize("kind", ["integer", "float"])
def test_interpolate_against_the_dense_restatement(cpu_backend_on, kind):
    check_interpolate("cpu", kind)


# ----------------------------------------------------------------------------- FeaturePropagation
LAYER_IN, LAYER_SKIP, LAYER_SIZES = 5, 4, (16, 8)


@functools.lru_cache(maxsize=None)
def layer_case(kind, skip_feats):
    """inputs, the fp64 reference (output, gradients), the forward bound and the gradients' magnitudes A and term count T"""
    k, u = BLOCK_K, 2.0 ** -24
    x, y, ref, feat, _, keep, extra = interp_case(kind, LAYER_IN)
    gen = torch.Generator().manual_seed(70 + skip_feats + len(kind))
    rn = lambda *shape: torch.randn(shape, generator=gen)
    skip = rn(ref.M, skip_feats) if skip_feats else None
    widths = [LAYER_IN + skip_feats] + list(LAYER_SIZES)
    params = [(rn(b, a) / a ** 0.5, rn(b)) for a, b in zip(widths[:-1], widths[1:])]
    g = rn(ref.M, LAYER_SIZES[-1]) * keep.unsqueeze(1)
    W = ref.dense(k)

    def run(absolute, masks):
        mag = (lambda t: t.double().abs()) if absolute else (lambda t: t.double())
        leaves = [mag(feat).requires_grad_(True)] + ([mag(skip).requires_grad_(True)] if skip is not None else [])
        leaves += [mag(t).requires_grad_(True) for wb in params for t in wb]
        h = (W.abs() if absolute else W) @ leaves[0]
        if skip is not None:
            h = torch.cat([h, leaves[1]], 1)
        pres, hs = [], [h]
        for i in range(len(params)):
            w, b = leaves[len(leaves) - 2 * len(params) + 2 * i], leaves[len(leaves) - 2 * len(params) + 2 * i + 1]
            pre = h @ w.t() + b
            pres.append(pre)
            h = pre * masks[i] if masks is not None else torch.relu(pre)
            hs.append(h)
        grads = torch.autograd.grad((h * mag(g)).sum(), leaves)
        return h.detach(), [p.detach() for p in pres], [t.detach() for t in hs], list(grads)

    out, pres, hs, grads = run(False, None)
    masks = [(p > 0).double() for p in pres]
    _, _, _, A = run(True, masks)
    # the forward bound: the interpolation's, pushed through every Linear with absolute values
    top = feat.double().abs()[ref.index(k)].max(1).values
    e = (2 * k + 8 + extra) * u * top
    if skip is not None:
        e = torch.cat([e, torch.zeros(ref.M, skip_feats, dtype=torch.float64)], 1)
    for i, (w, b) in enumerate(params):
        n = w.shape[1]
        e = e @ w.double().abs().t() + (n + 3) * u * ((hs[i].abs() + e) @ w.double().abs().t() + b.double().abs())
        assert bool((pres[i].abs()[keep] > 2 * e[keep]).all()), "a pre-activation of layer %d lies within its bound of 0: pick another seed" % i
    T = sum(widths) + ref.M + int(torch.bincount(ref.index(k).flatten(), minlength=ref.N).max()) + extra // 2
    return x, y, feat, skip, params, g, out, grads, e, A, T, keep


def check_layer(device, kind):
    for skip_feats in (LAYER_SKIP, 0):
        x, y, feat, skip, params, g, ref_out, ref_grads, fwd_bound, A, T, keep = layer_case(kind, skip_feats)
        layer = mg.nn.FeaturePropagation(LAYER_IN, skip_feats, LAYER_SIZES, k=BLOCK_K).to(device)
        assert [tuple(l.weight.shape) for l in layer.layers] == [(16, LAYER_IN + skip_feats), (8, 16)]
        with torch.no_grad():
            for l, (w, b) in zip(layer.layers, params):
                l.weight.copy_(w)
                l.bias.copy_(b)
        f = leaf(feat, device)
        s = leaf(skip, device) if skip is not None else None
        out = layer(f, x.to(device), y.to(device), list(INTERP_REF), list(INTERP_QUERY), s)
        leaves = [f] + ([s] if s is not None else []) + [t for l in layer.layers for t in (l.weight, l.bias)]
        grads = torch.autograd.grad(out, leaves, g.to(device))
        err = (out.detach().cpu().double() - ref_out).abs()[keep]
        assert bool((err <= fwd_bound[keep]).all()), "%s skip=%d: forward %g of the bound" % (
            kind, skip_feats, float((err / fwd_bound[keep].clamp(min=1e-300)).max()))
        for got, want, a in zip(grads, ref_grads, A):
            gerr, gbound = (got.cpu().double() - want).abs(), (T + 8) * 2.0 ** -23 * a
            assert bool((gerr <= gbound).all()), "%s skip=%d: gradient %g of the bound" % (
                kind, skip_feats, float((gerr / gbound.clamp(min=1e-300)).max()))


@pytest.mark.parametrize("kind", ["integer", "float"])
def test_feature_propagation_against_the_restatement(cpu_backend_on, kind):
    check_layer("cpu", kind)


def test_feature_propagation_arguments_and_names(cpu_backend_on):
    import dgl
    import dgl.geometry
    assert dgl.nn.FeaturePropagation is mg.nn.FeaturePropagation and dgl.geometry.knn_block is mg.transform.knn_block
    assert dgl.geometry.knn_interpolate is mg.transform.knn_interpolate
    layer = mg.nn.FeaturePropagation(5, 4, (16, 8), batch_norm=True)
    assert sorted(n for n, _ in layer.named_parameters()) == ["bns.0.bias", "bns.0.weight", "bns.1.bias", "bns.1.weight", "layers.0.bias",
                                                              "layers.0.weight", "layers.1.bias", "layers.1.weight"]
    x, y = int_points(INTERP_REF, 3, seed=8), int_points(INTERP_QUERY, 3, seed=9)
    out = layer(torch.randn(112, 5), x, y, list(INTERP_REF), list(INTERP_QUERY), torch.randn(133, 4))
    assert tuple(out.shape) == (133, 8) and bool(torch.isfinite(out).all()) and bool((out >= 0).all())
    for bad in (lambda: mg.nn.FeaturePropagation(0, 4, (8,)), lambda: mg.nn.FeaturePropagation(5, -1, (8,)),
                lambda: mg.nn.FeaturePropagation(5, 4, ()), lambda: mg.nn.FeaturePropagation(5, 4, (8,), k=0),
                lambda: layer(torch.randn(112, 5), x, y, list(INTERP_REF), list(INTERP_QUERY)),                   # skip features missing
                lambda: layer(torch.randn(112, 6), x, y, list(INTERP_REF), list(INTERP_QUERY), torch.randn(133, 4)),
                lambda: mg.nn.FeaturePropagation(5, 0, (8,))(torch.randn(112, 5), x, y, list(INTERP_REF), list(INTERP_QUERY), torch.randn(133, 4))):
        with pytest.raises(mg.DGLError):
            bad()


# ----------------------------------------------------------------------------- the script
TINY = ["--clouds", "4", "--batch", "4", "--points", "64", "--npoints", "16", "8", "--radius", "0.4", "0.8", "--neighbors", "8", "8"]


def test_script_model_trains_one_tiny_epoch_on_the_cpu():
    """pointnet2_seg.py's own parser, model and epoch loop on the OpenMP backend (the script's main() asks for a device)"""
    sys.path.insert(0, PKG)
    import pointnet2_seg as ps
    from mi355x_graph.datasets import POINT_SHAPES, shape_scenes_like
    args = ps.make_parser().parse_args([])
    assert (args.points, args.batch, args.npoints, args.radius, args.neighbors, args.k) == (1024, 32, [512, 128], [0.2, 0.4], [32, 64], 3)
    args = ps.make_parser().parse_args(TINY)
    xyz, label = shape_scenes_like(4, 64, seed=2)
    assert tuple(xyz.shape) == (4, 64, 3) and xyz.dtype == torch.float32 and tuple(label.shape) == (4, 64) and label.dtype == torch.int64
    assert torch.equal(xyz, shape_scenes_like(4, 64, seed=2)[0]) and torch.equal(label, shape_scenes_like(4, 64, seed=2)[1])   # seeded
    assert all(1 <= len(set(row.tolist())) <= 3 for row in label) and int(label.min()) >= 0 and int(label.max()) < len(POINT_SHAPES)
    was = mg.enable_cpu_backend(True)
    try:
        torch.manual_seed(0)
        model = ps.PointNet2Seg(len(POINT_SHAPES), args.npoints, args.radius, args.neighbors)
        assert [tuple(l.weight.shape) for up in model.ups for l in up.layers] == [(256, 384), (128, 256), (128, 131), (128, 128)]
        model.eval()
        assert tuple(model(xyz).shape) == (4 * 64, len(POINT_SHAPES))
        loss = ps.train_epoch(model, torch.device("cpu"), xyz, label, 4, torch.optim.Adam(model.parameters(), lr=1e-3))
        assert math.isfinite(loss)
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    finally:
        mg.enable_cpu_backend(was)


# ----------------------------------------------------------------------------- GPU: the kernel against the restatement
@pytest.mark.gpu
@pytest.mark.parametrize("D", DS)
def test_kernel_matches_the_restatement_exactly(monkeypatch, D):
    x, y, ref = int_case(D)
    for k in KS:
        seglen_dtype = torch.int32 if k % 2 else torch.int64
        assert fused(REF_LENS, x, QUERY_LENS, y, k)
        rec = launches(monkeypatch)
        got = query(REF_LENS, x, QUERY_LENS, y, k, DEV, seglen_dtype=seglen_dtype)
        assert [r["kernel"] for r in rec] == ["segment_knn_query"]              # one launch, nothing else from the library
        check_exact(got, ref, k, (D, k))
        again = query(REF_LENS, x, QUERY_LENS, y, k, DEV, seglen_dtype=seglen_dtype)   # reruns give identical bits
        assert torch.equal(got[0], again[0]) and torch.equal(bits(got[1]), bits(again[1])) and torch.equal(bits(got[2]), bits(again[2]))
        only = query(REF_LENS, x, QUERY_LENS, y, k, DEV, return_dist=False, return_weight=False)   # dist = weight = NULL
        assert torch.is_tensor(only) and torch.equal(only, got[0])
        index, weight = query(REF_LENS, x, QUERY_LENS, y, k, DEV, return_dist=False)              # dist = NULL alone
        assert torch.equal(index, got[0]) and torch.equal(bits(weight), bits(got[2]))


@pytest.mark.gpu
def test_kernel_nan_strided_and_other_eps(monkeypatch):
    x, y, ref = nan_case()
    for k in (3, 8, 64):
        check_exact(query(REF_LENS, x, QUERY_LENS, y, k, DEV), ref, k, ("nan", k))
    wide_x, wide_y = int_points(REF_LENS, 100).to(DEV), int_points(QUERY_LENS, 70, seed=1).to(DEV)
    bx, by = wide_x[:, 10:43], wide_y[:, 5:38]                                  # D = 33, row strides 100 and 70, bases inside a row
    assert not bx.is_contiguous() and not by.is_contiguous()
    rec = launches(monkeypatch)
    got = query(REF_LENS, bx, QUERY_LENS, by, 8, DEV)
    assert [r["kernel"] for r in rec] == ["segment_knn_query"]
    check_exact(got, Restated(REF_LENS, bx, QUERY_LENS, by), 8, "strided")
    ox, oy = wide_x[:, ::2], wide_y[:, :50]                                      # a column stride of 2: copied, same result
    check_exact(query(REF_LENS, ox, QUERY_LENS, oy, 8, DEV), Restated(REF_LENS, ox, QUERY_LENS, oy), 8, "column stride")
    x, y, ref = int_case(3)
    index, dist, weight = query(REF_LENS, x, QUERY_LENS, y, 3, DEV, eps=0.5)
    want, valid = ref.weight(3, eps=0.5), ref.index(3) >= 0
    err = (weight.cpu().double() - want).abs()
    assert bool((err <= 6 * 2.0 ** -23 * want).all()) and bool((weight.cpu()[~valid] == 0).all())
    one_x, one_y = int_points((1000,), 3), int_points((70,), 3, seed=1)
    check_exact(query([1000], one_x, [70], one_y, 64, DEV), Restated([1000], one_x, [70], one_y), 64, "one segment")
    check_exact(query([0, 0, 1000, 0], one_x, [0, 3, 67, 0], one_y, 7, DEV), Restated([0, 0, 1000, 0], one_x, [0, 3, 67, 0], one_y), 7,
                "empty segments around")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["normal", "scaled", "cluster"])
def test_kernel_float_cases(kind):
    for D in (1, 3, 64, 128):
        x, y, ref = float_case(D, kind)
        assert fused(FLOAT_REF_LENS, x, FLOAT_QUERY_LENS, y, 20)
        index, dist, weight = query(FLOAT_REF_LENS, x, FLOAT_QUERY_LENS, y, 20, DEV)
        check_float(index, dist, ref, 20, D, "kernel %s D=%d" % (kind, D))
        assert bool(((weight.sum(1) - 1).abs() <= 23 * 2.0 ** -23).all())      # k + 3 roundings a weight: the weights of a query sum to 1


@pytest.mark.gpu
def test_self_case_equals_segment_knn():
    for D, k in ((3, 8), (4, 64), (33, 1)):
        x = int_points(REF_LENS, D)
        seglen = torch.tensor(REF_LENS).to(DEV)
        index, dist = query(REF_LENS, x, REF_LENS, x, k, DEV, return_weight=False)
        self_index, self_dist = ops.segment_knn(seglen, x.to(DEV), k, total=int(x.shape[0]), return_dist=True)
        assert torch.equal(index, self_index) and torch.equal(bits(dist), bits(self_dist)), (D, k)
    x = float_case(3, "normal")[0]
    index, dist = query(FLOAT_REF_LENS, x, FLOAT_REF_LENS, x, 20, DEV, return_weight=False)
    self_index, self_dist = ops.segment_knn(torch.tensor(FLOAT_REF_LENS).to(DEV), x.to(DEV), 20, return_dist=True)
    assert torch.equal(index, self_index) and torch.equal(bits(dist), bits(self_dist))


@pytest.mark.gpu
def test_outside_the_kernels_set_takes_the_composition(monkeypatch):
    x, y, ref = int_case(4)
    assert fused(REF_LENS, x, QUERY_LENS, y, 64) and not fused(REF_LENS, x, QUERY_LENS, y, 65)
    rec = launches(monkeypatch)
    check_exact(query(REF_LENS, x, QUERY_LENS, y, 65, DEV), ref, 65, "k = 65")
    ref_lens, query_lens = (20, 70, 33), (9, 40, 17)
    wx, wy = int_points(ref_lens, 257), int_points(query_lens, 257, seed=1)
    assert fused(ref_lens, wx[:, :256], query_lens, wy[:, :256], 8) and not fused(ref_lens, wx, query_lens, wy, 8)
    check_exact(query(ref_lens, wx, query_lens, wy, 8, DEV), Restated(ref_lens, wx, query_lens, wy), 8, "D = 257")
    monkeypatch.setattr(config, "KNN_QUERY_FUSED", False)
    assert not fused(REF_LENS, x, QUERY_LENS, y, 3)
    check_exact(query(REF_LENS, x, QUERY_LENS, y, 3, DEV), ref, 3, "switch off")
    assert not any(r["kernel"] == "segment_knn_query" for r in rec)


@pytest.mark.gpu
def test_captured_in_a_hip_graph():
    """the capture idiom of tests/test_knn.py: warm-up and capture on ONE side stream, then replay with new points in the static
    inputs -- the operator reads nothing back to the host"""
    N, M = sum(REF_LENS), sum(QUERY_LENS)
    ref_seglen, query_seglen = torch.tensor(REF_LENS).to(DEV), torch.tensor(QUERY_LENS).to(DEV)
    static_x, static_y = int_points(REF_LENS, 4).to(DEV).clone(), int_points(QUERY_LENS, 4, seed=1).to(DEV).clone()
    outs = {}

    def step():
        outs["got"] = ops.segment_knn_query(ref_seglen, static_x, query_seglen, static_y, 8, ref_total=N, query_total=M, return_dist=True,
                                            return_weight=True)

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
    new_x, new_y = int_points(REF_LENS, 4, seed=9), int_points(QUERY_LENS, 4, seed=10)
    static_x.copy_(new_x.to(DEV))
    static_y.copy_(new_y.to(DEV))
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    got = outs["got"]
    eager = query(REF_LENS, new_x, QUERY_LENS, new_y, 8, DEV)
    assert torch.equal(got[0], eager[0]) and torch.equal(bits(got[1]), bits(eager[1])) and torch.equal(bits(got[2]), bits(eager[2]))
    check_exact(got, Restated(REF_LENS, new_x, QUERY_LENS, new_y), 8)


@pytest.mark.gpu
def test_block_builder_on_the_device_launches_no_sort(monkeypatch):
    import dgl.geometry
    check_block(DEV)
    x, y = int_points(INTERP_REF, 3, seed=8).to(DEV), int_points(INTERP_QUERY, 3, seed=9).to(DEV)
    feat = torch.randn(sum(INTERP_REF), 8, generator=torch.Generator().manual_seed(0)).to(DEV)
    ref = Restated(INTERP_REF, x, INTERP_QUERY, y)
    want = ref.dense(BLOCK_K) @ feat.cpu().double()
    bound = (2 * BLOCK_K + 8) * 2.0 ** -24 * feat.cpu().double().abs()[ref.index(BLOCK_K)].max(1).values
    torch.cuda.synchronize()

    def never(*args, **kwargs):
        raise AssertionError("the block builder sorted or converted a format")

    for owner, name in ((torch, "sort"), (torch, "argsort"), (torch.Tensor, "sort"), (torch.Tensor, "argsort"), (sparse, "coo_to_csr"),
                        (sparse, "csr_transpose")):
        monkeypatch.setattr(owner, name, never)
    rec = launches(monkeypatch)
    block = dgl.geometry.knn_block(x, list(INTERP_REF), y, list(INTERP_QUERY), BLOCK_K)
    assert [r["kernel"] for r in rec] == ["segment_knn_query"]                  # the index IS the in-CSR
    out = ops.u_mul_e_sum(block, feat, block.edata["w"])                         # ... and the forward needs no other format
    assert block._index.format_status() == {"created": ["csc"], "not created": ["coo", "csr"]}
    assert bool(((out.cpu().double() - want).abs() <= bound).all())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["integer", "float"])
def test_interpolate_on_the_device(kind):
    check_interpolate(DEV, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["integer", "float"])
def test_feature_propagation_on_the_device(kind):
    check_layer(DEV, kind)


@functools.lru_cache(maxsize=None)
def _script(*args):
    """(losses printed per epoch, whole output) of one run of the script"""
    env = dict(os.environ, PYTHONPATH=PKG)
    cmd = [sys.executable, os.path.join(PKG, "pointnet2_seg.py")] + TINY + ["--dropout", "0", "--no-shuffle"] + list(args)
    res = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert res.returncode == 0, res.stdout[-3000:]
    losses = [float(v) for v in re.findall(r"epoch \d+ loss (\S+)", res.stdout)]
    return losses, res.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["eager", "hipgraph"])
def test_script_trains_to_a_finite_decreasing_loss(mode):
    """five epochs of one step each on the same 4 clouds of 64 points; with --hipgraph the captured step is replayed"""
    losses, text = _script("--epochs", "5", *(["--hipgraph"] if mode == "hipgraph" else []))
    assert len(losses) == 5 and all(math.isfinite(v) for v in losses), text[-2000:]
    assert losses[-1] < losses[0], text[-2000:]
    if mode == "hipgraph":
        assert "hipgraph: 5 steps replayed" in text, text[-2000:]
