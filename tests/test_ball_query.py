"""Fixed-radius ball query: csrc/ballquery.hip (mgx_segment_ball_query), ops.segment_ball_query / segment_ball_query_fused,
transform.fixed_radius_block, nn.FixedRadiusNNGraph.

The reference everywhere is the restatement below, a Python loop over the queries in fp64 -- never the composed form and never the kernel:

    the segment that holds centre c;  d64 = ((x[c] - seg) ** 2).sum(-1);  the first K rows with d64 <= radius2 in row order (NaN: outside);
    count = how many;  ranks past count: index[q, 0] (pad "first") or -1;  nothing found: -1 everywhere

radius2 = float32(radius) * float32(radius), the operator's documented threshold, computed here the same way.

  exact   integer coordinates in [-3, 3]: every distance is an integer below 2^24, exact in fp32 in any order -- torch.equal on index
          and count, for both pads
  float   normal / row-scaled / a cluster at 1000 + 1e-3 randn: the test picks the radius and a seed for which NO reference d64 lies within
          (D + 2) 2^-23 relative of radius2 (asserted on the reference alone, on the CPU) -- fp32's direct form is within (D + 2) 2^-24
          relative of d64, so no decision can differ -- and then requires torch.equal."""
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
from mi355x_graph import _lib, config, ops
import mi355x_graph.function as fn
import oracle_backend

DEV = "cuda:0"
NAN = float("nan")


def radius2_of(radius):
    r = torch.tensor(float(radius), dtype=torch.float32)
    return float(r * r)


# ----------------------------------------------------------------------------- the restatement (a loop over queries, never the code under test)
def restated(lens, x, centers, radius, K, pad_first):
    x = x.detach().cpu().double()
    r2 = radius2_of(radius)
    ends = [0]
    for n in lens:
        ends.append(ends[-1] + n)
    M = len(centers)
    index = torch.full((M, K), -1, dtype=torch.int64)
    count = torch.zeros(M, dtype=torch.int32)
    for q, c in enumerate(int(v) for v in centers):
        seg = [s for s in range(len(lens)) if ends[s] <= c < ends[s + 1]]
        if not seg:
            continue
        beg, end = ends[seg[0]], ends[seg[0] + 1]
        d = ((x[c] - x[beg:end]) ** 2).sum(-1)
        hits = (d <= r2).nonzero().flatten()[:K] + beg
        count[q] = len(hits)
        index[q, :len(hits)] = hits
        if pad_first and len(hits):
            index[q, len(hits):] = hits[0]
    return index, count


LENS = (0, 1, 15, 16, 17, 63, 64, 65, 0, 127, 300)
RADIUS2 = (0, 1, 4, 9.5, 1e9)
KS = (1, 2, 16, 63, 64)
DS = (1, 3, 4, 64, 67, 256)
FLOAT_LENS = (20, 21, 64, 65, 127, 300)


@functools.lru_cache(maxsize=None)
def int_points(lens, D, seed=0):
    return torch.randint(-3, 4, (sum(lens), D), generator=torch.Generator().manual_seed(1000 * D + seed)).float()


def starts_of(lens):
    return [0] + torch.tensor(lens).cumsum(0).tolist()[:-1]


@functools.lru_cache(maxsize=None)
def all_rows_shuffled(lens, seed=0):
    """every row as a centre, in a random order: centres of different segments inside one 16-query tile"""
    return torch.randperm(sum(lens), generator=torch.Generator().manual_seed(seed))


def ball(lens, x, centers, radius, K, device, pad="first", seglen_dtype=torch.int64):
    return ops.segment_ball_query(torch.tensor(lens, dtype=seglen_dtype).to(device), x.to(device), centers.to(device), radius, K, pad=pad,
                                  total=int(x.shape[0]))


def check(lens, x, centers, radius, K, device, what="", seglen_dtype=torch.int64):
    for pad in ("first", None):
        index, count = ball(lens, x, centers, radius, K, device, pad, seglen_dtype)
        want_index, want_count = restated(lens, x, centers, radius, K, pad == "first")
        assert index.dtype == torch.int64 and tuple(index.shape) == (len(centers), K) and count.dtype == torch.int32, what
        assert not index.requires_grad and not count.requires_grad
        assert torch.equal(count.cpu(), want_count), (what, pad)
        assert torch.equal(index.cpu(), want_index), (what, pad)


def launches(monkeypatch):
    rec = []
    monkeypatch.setattr(mg.sparse, "PROFILE", rec)
    return rec


def exact_cases(device, D, check_fused=None):
    x = int_points(LENS, D)
    centers = all_rows_shuffled(LENS)[:150]                                     # M = 150: not a multiple of 16
    for i, K in enumerate(KS):
        for j, r2 in enumerate(RADIUS2):
            if check_fused:
                check_fused(LENS, x, centers, math.sqrt(r2), K)
            check(LENS, x, centers, math.sqrt(r2), K, device, (D, K, r2), torch.int32 if (i + j) % 2 else torch.int64)


def centre_cases(device):
    x = int_points(LENS, 3)
    N = sum(LENS)
    # farthest point samples as centres (the -1 padding of the short segments included)
    fps = ops.segment_fps(torch.tensor(LENS).to(device), x.to(device), 20, total=N).cpu().flatten()
    assert bool((fps == -1).any())
    check(LENS, x, fps, 2.0, 16, device, "fps centres")
    # unsorted with duplicates, -1 and rows no segment holds
    centers = torch.tensor([400, 3, 3, 700, -1, 17, 400, 0, N - 1, 35, -1, 3, 140, N, N + 5, -7, 250, 251, 249])
    check(LENS, x, centers, 2.0, 16, device, "unsorted, duplicates, -1")
    check(LENS, x, all_rows_shuffled(LENS, 1), 1.5, 5, device, "every row")
    check(LENS, x, torch.zeros(0, dtype=torch.int64), 1.0, 4, device, "M = 0")
    check(LENS, x, torch.tensor([N - 1]), 1.0, 4, device, "M = 1")
    # the early stop: K = 1 within a huge radius is the segment's FIRST row, not the nearest
    last = starts_of(LENS)[-1]
    centers = torch.arange(last, last + 300)
    check(LENS, x, centers, math.sqrt(1e9), 1, device, "early stop")
    index, count = ball(LENS, x, centers, math.sqrt(1e9), 1, device)
    assert bool((index.cpu() == last).all()) and bool((count.cpu() == 1).all())
    # a NaN centre finds nothing (itself included) and is in nobody's ball
    y = x.clone()
    y[last + 7, 1] = NAN
    y[starts_of(LENS)[6]:starts_of(LENS)[6] + 64] = NAN                        # the segment of 64 NaN only
    centers = torch.cat([torch.arange(last, last + 20), torch.arange(starts_of(LENS)[6] - 3, starts_of(LENS)[6] + 70)])
    check(LENS, y, centers, 3.0, 16, device, "nan")
    index, count = ball(LENS, y, centers, 3.0, 16, device)
    assert int(count[7]) == 0 and bool((index[7] == -1).all()) and not bool((index == last + 7).any())
    # a row-strided x
    wide = int_points(LENS, 100).to(device)
    block = wide[:, 10:77]                                                      # D = 67, row stride 100
    assert not block.is_contiguous()
    check(LENS, block, all_rows_shuffled(LENS, 2)[:100], 22.0, 16, device, "strided")


# ----------------------------------------------------------------------------- float cases
@functools.lru_cache(maxsize=None)
def float_case(D, kind):
    """(x, centers, radius): the first seed whose reference has no d64 within (D + 2) 2^-23 relative of radius2 (the reference alone)"""
    N = sum(FLOAT_LENS)
    ends = [0] + torch.tensor(FLOAT_LENS).cumsum(0).tolist()
    for seed in range(50):
        gen = torch.Generator().manual_seed(100 * seed + 7 * D + len(kind))
        x = torch.randn(N, D, generator=gen)
        if kind == "scaled":
            x = x * torch.exp(4 * torch.randn(N, 1, generator=gen))
        elif kind == "cluster":
            x = 1000 + 1e-3 * x
        else:
            assert kind == "normal"
        centers = torch.randperm(N, generator=gen)[:200]
        x64 = x.double()
        d64 = torch.cat([((x64[c] - x64[b:e]) ** 2).sum(-1) for c in centers.tolist() for b, e in zip(ends[:-1], ends[1:]) if b <= c < e])
        radius = float((1.003 * d64.median()).sqrt())                           # about half of every segment is inside
        r2 = radius2_of(radius)
        if bool(((d64 - r2).abs() > (D + 2) * 2.0 ** -23 * r2).all()):
            return x, centers, radius
    raise AssertionError("no seed with a clear margin")


def float_cases(device, kind):
    for D in (1, 3, 64, 128):
        x, centers, radius = float_case(D, kind)
        for K in (8, 64):
            check(FLOAT_LENS, x, centers, radius, K, device, "%s D=%d K=%d" % (kind, D, K))


# ----------------------------------------------------------------------------- CPU: the composed form under the checker backend
@pytest.fixture
def cpu_backend_on():
    oracle_backend.install()
    yield
    oracle_backend.uninstall()


def test_restatement_by_hand():
    x = torch.tensor([[0.], [1.], [2.], [9.], [0.], [3.], [1.]])
    index, count = restated([4, 3], x, [1, 3, 6, -1], 1.0, 3, True)
    assert index.tolist() == [[0, 1, 2], [3, 3, 3], [4, 6, 4], [-1, -1, -1]] and count.tolist() == [3, 1, 2, 0]
    index, count = restated([4, 3], x, [1, 3, 6, -1], 1.0, 2, False)
    assert index.tolist() == [[0, 1], [3, -1], [4, 6], [-1, -1]] and count.tolist() == [2, 1, 2, 0]         # the first K, not the nearest


@pytest.mark.parametrize("D", DS)
def test_composition_matches_the_restatement_exactly(cpu_backend_on, D):
    def composed(lens, x, centers, radius, K):
        assert not ops.segment_ball_query_fused(torch.tensor(lens), x, centers, radius, K)
    exact_cases("cpu", D, composed)


def test_composition_centres(cpu_backend_on):
    centre_cases("cpu")


@pytest.mark.parametrize("kind", ["normal", "scaled", "cluster"])
def test_composition_float_cases(cpu_backend_on, kind):
    float_cases("cpu", kind)


def test_argument_errors(cpu_backend_on):
    x = int_points((5, 7), 3)
    seglen, c = torch.tensor([5, 7]), torch.tensor([0, 6])
    index, count = ops.segment_ball_query(torch.zeros(0, dtype=torch.int64), torch.zeros(0, 3), torch.tensor([0, -1]), 1.0, 4)
    assert torch.equal(index, torch.full((2, 4), -1)) and count.tolist() == [0, 0]
    for bad in (lambda: ops.segment_ball_query(seglen, x, c, 1.0, 0), lambda: ops.segment_ball_query(seglen, x, c, 1.0, True),
                lambda: ops.segment_ball_query(seglen, x, c, 1.0, 2.0), lambda: ops.segment_ball_query(seglen, x, c, -1.0, 2),
                lambda: ops.segment_ball_query(seglen, x, c, NAN, 2), lambda: ops.segment_ball_query(seglen, x, c, "1", 2),
                lambda: ops.segment_ball_query(seglen, x, c.int(), 1.0, 2), lambda: ops.segment_ball_query(seglen, x, [0, 6], 1.0, 2),
                lambda: ops.segment_ball_query(seglen, x, c.view(1, 2), 1.0, 2), lambda: ops.segment_ball_query(seglen, x, c, 1.0, 2, pad="last"),
                lambda: ops.segment_ball_query(torch.tensor([5, 6]), x, c, 1.0, 2), lambda: ops.segment_ball_query(seglen, x.double(), c, 1.0, 2),
                lambda: ops.segment_ball_query(seglen, x[:, 0], c, 1.0, 2), lambda: ops.segment_ball_query([5, 7], x, c, 1.0, 2)):
        with pytest.raises(mg.DGLError):
            bad()


def test_without_a_cpu_backend_cpu_tensors_fail_loudly(monkeypatch):
    monkeypatch.delitem(mg.sparse._BACKENDS, "cpu", raising=False)
    with pytest.raises(mg.DGLError, match="MI355X"):
        ops.segment_ball_query(torch.tensor([5, 7]), int_points((5, 7), 3), torch.tensor([0]), 1.0, 2)


def test_abi_argument_checks():
    L = _lib.lib()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("mgx_segment_ball_query_supported", "mgx_segment_ball_query"):
        assert hasattr(handle, name) and name in _lib.SIGNATURES
    assert L.mgx_abi_version() == 35
    assert config.BALL_QUERY_FUSED is True
    for (K, D), want in (((1, 1), 1), ((64, 256), 1), ((32, 3), 1), ((65, 3), 0), ((32, 257), 0), ((0, 3), 0), ((32, 0), 0), ((-1, 3), 0)):
        assert L.mgx_segment_ball_query_supported(K, D) == want, (K, D)
    host = (ctypes.c_float * 64)()                                             # never dereferenced: every call below fails a check first
    p = ctypes.c_void_p(ctypes.addressof(host))

    def call(S=2, offsets=p, N=8, D=4, ld=4, x=p, M=3, centers=p, radius2=1.0, K=2, pad=1, index=p, count=p):
        return L.mgx_segment_ball_query(S, offsets, N, D, ld, x, M, centers, radius2, K, pad, index, count, None)

    assert call(K=0) == 1 and b"K must be at least 1" in L.mgx_last_error()
    assert call(K=-3) == 1 and call(S=-1) == 1 and call(N=-1) == 1 and call(M=-1) == 1 and call(D=0) == 1
    assert call(ld=3) == 1 and b"row stride" in L.mgx_last_error()
    assert call(K=65) == _lib.ERR_UNSUPPORTED and call(D=257, ld=257) == _lib.ERR_UNSUPPORTED
    assert call(N=2 ** 31) == _lib.ERR_UNSUPPORTED and call(N=2 ** 28, ld=4) == _lib.ERR_UNSUPPORTED and call(M=2 ** 31) == _lib.ERR_UNSUPPORTED
    for null in ("offsets", "x", "centers", "index", "count"):
        assert call(**{null: None}) == 1 and b"is NULL" in L.mgx_last_error(), null
    assert call(M=0, offsets=None, x=None, centers=None, index=None, count=None) == 0                 # no queries: nothing to do


# ----------------------------------------------------------------------------- the block builder
def check_block(device):
    import dgl
    import dgl.geometry
    lens = (40, 0, 72)
    N, K, per = sum(lens), 8, 10
    x = int_points(lens, 3, seed=6)
    pos = x.to(device)
    centers = ops.segment_fps(torch.tensor([40, 72]).to(device), pos, per, total=N).flatten()
    want_index, want_count = restated(lens, x, centers.cpu(), 1.5, K, True)
    for block in (dgl.geometry.fixed_radius_block(pos, centers, 1.5, K, list(lens)), mg.nn.FixedRadiusNNGraph(1.5, K)(pos, centers, list(lens))):
        assert block.is_block and block.number_of_src_nodes() == N and block.number_of_dst_nodes() == 2 * per
        assert block.number_of_edges() == 2 * per * K and block.idtype == torch.int32
        csc = block._index.csc()
        assert torch.equal(csc.indptr.cpu().long(), torch.arange(2 * per + 1) * K) and csc.eids is None
        assert block._index.max_in_degree_hint == K
        assert torch.equal(csc.indices.cpu().long().view(-1, K), want_index) and int(csc.indices.min()) >= 0
        assert torch.equal(block.srcdata["pos"].cpu(), x) and torch.equal(block.dstdata["pos"].cpu(), x[centers.cpu()])
        # copy_u / max over the block against the restatement
        feat = torch.randn(N, 5, generator=torch.Generator().manual_seed(1)).to(device)
        block.srcdata["h"] = feat
        block.update_all(fn.copy_u("h", "m"), fn.max("m", "o"))
        assert torch.equal(block.dstdata["o"].cpu(), feat.cpu()[want_index].max(1).values)
    # count == 0 (a NaN centre): its own row in every slot, no -1 reaches a gather
    y = x.clone()
    lone = int(centers[3])
    y[lone, 0] = NAN
    block = dgl.geometry.fixed_radius_block(y.to(device), centers, 1.5, K, list(lens))
    got = block._index.csc().indices.cpu().long().view(-1, K)
    ref_index, ref_count = restated(lens, y, centers.cpu(), 1.5, K, True)
    assert int(ref_count[3]) == 0 and bool((got[3] == lone).all()) and int(got.min()) >= 0
    keep = ref_count > 0
    assert torch.equal(got[keep], ref_index[keep])
    for bad in (lambda: dgl.geometry.fixed_radius_block(pos, centers, 1.5, K, [40, 71]),
                lambda: dgl.geometry.fixed_radius_block(pos, centers, 1.5, 0, list(lens)),
                lambda: dgl.geometry.fixed_radius_block(pos, centers.int(), 1.5, K, list(lens)),
                lambda: dgl.geometry.fixed_radius_block(pos, centers, -1.0, K, list(lens)),
                lambda: dgl.geometry.fixed_radius_block(pos[:, 0], centers, 1.5, K, list(lens)),
                lambda: dgl.geometry.fixed_radius_block(pos, centers[:18], 1.5, K, [5, 35, 72])):   # 6 samples of a 5-point set: a -1 centre
        with pytest.raises(mg.DGLError):
            bad()


def test_block_builder(cpu_backend_on):
    check_block("cpu")


# ----------------------------------------------------------------------------- GPU: the kernel against the restatement
def fused_one_launch(monkeypatch):
    def check_fused(lens, x, centers, radius, K):
        assert ops.segment_ball_query_fused(torch.tensor(lens).to(DEV), x.to(DEV), centers.to(DEV), radius, K)
        rec = launches(monkeypatch)
        index, count = ball(lens, x, centers, radius, K, DEV)
        assert [r["kernel"] for r in rec] == ["segment_ball_query"]             # one launch, nothing else from the library
        again_index, again_count = ball(lens, x, centers, radius, K, DEV)      # reruns give identical results
        assert torch.equal(index, again_index) and torch.equal(count, again_count)
    return check_fused


@pytest.mark.gpu
@pytest.mark.parametrize("D", DS)
def test_kernel_matches_the_restatement_exactly(monkeypatch, D):
    exact_cases(DEV, D, fused_one_launch(monkeypatch))


@pytest.mark.gpu
def test_kernel_centres():
    centre_cases(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["normal", "scaled", "cluster"])
def test_kernel_float_cases(kind):
    x, centers, radius = float_case(3, kind)
    assert ops.segment_ball_query_fused(torch.tensor(FLOAT_LENS).to(DEV), x.to(DEV), centers.to(DEV), radius, 8)
    float_cases(DEV, kind)


@pytest.mark.gpu
def test_outside_the_kernels_set_takes_the_composition(monkeypatch):
    rec = launches(monkeypatch)
    x = int_points(LENS, 4)
    centers = all_rows_shuffled(LENS)[:100]
    seglen = torch.tensor(LENS).to(DEV)
    assert ops.segment_ball_query_fused(seglen, x.to(DEV), centers.to(DEV), 2.0, 64)
    assert not ops.segment_ball_query_fused(seglen, x.to(DEV), centers.to(DEV), 2.0, 65)
    check(LENS, x, centers, 2.0, 65, DEV, "K = 65")
    lens = (20, 70, 33)
    wide = int_points(lens, 257)
    c = all_rows_shuffled(lens)[:50]
    assert ops.segment_ball_query_fused(torch.tensor(lens).to(DEV), wide[:, :256].to(DEV), c.to(DEV), 20.0, 8)
    assert not ops.segment_ball_query_fused(torch.tensor(lens).to(DEV), wide.to(DEV), c.to(DEV), 20.0, 8)
    check(lens, wide, c, 33.0, 8, DEV, "D = 257")
    monkeypatch.setattr(config, "BALL_QUERY_FUSED", False)
    assert not ops.segment_ball_query_fused(seglen, x.to(DEV), centers.to(DEV), 2.0, 16)
    check(LENS, x, centers, 2.0, 16, DEV, "switch off")
    assert not any(r["kernel"] == "segment_ball_query" for r in rec)


@pytest.mark.gpu
def test_captured_in_a_hip_graph():
    """the capture idiom of tests/test_knn.py on ONE side stream: sampling and grouping captured together, replayed on new points"""
    lens = (64, 300, 127)
    N = sum(lens)
    seglen = torch.tensor(lens).to(DEV)
    static = int_points(lens, 3).to(DEV).clone()
    outs = {}

    def step():
        centers = ops.segment_fps(seglen, static, 32, total=N, max_len=300).flatten()
        outs["got"] = (centers,) + ops.segment_ball_query(seglen, static, centers, 2.0, 16, total=N)

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
    new = int_points(lens, 3, seed=9)
    static.copy_(new.to(DEV))
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    centers, index, count = outs["got"]
    want_index, want_count = restated(lens, new, centers.cpu(), 2.0, 16, True)
    assert torch.equal(index.cpu(), want_index) and torch.equal(count.cpu(), want_count)


@pytest.mark.gpu
def test_block_builder_on_the_device(monkeypatch):
    check_block(DEV)


# ----------------------------------------------------------------------------- PointNetConv over the block
CONV_LENS, CONV_PER, CONV_K, CONV_RADIUS = (40, 72), 10, 8, 1.5


@functools.lru_cache(maxsize=None)
def conv_block_host():
    """(pos, centers, src [M, K] padded as the block holds it) from the restatements alone"""
    import test_fps
    pos = int_points(CONV_LENS, 3, seed=6)
    centers = test_fps.restated(CONV_LENS, pos, CONV_PER)[0].flatten()
    src, _ = restated(CONV_LENS, pos, centers, CONV_RADIUS, CONV_K, True)
    assert int(src.min()) >= 0 and bool((src[:, 1:] == src[:, :1]).all(1).any())      # some balls are padded
    return pos, centers, src


def block_src(pos):
    """the padded balls of the fixed centres around these positions, by the restatement"""
    return restated(CONV_LENS, pos, conv_block_host()[1], CONV_RADIUS, CONV_K, True)[0]


def conv_restated(h, pos, params, w, batch_norm=None):
    """fp64: (out, grads of sum(out * w) w.r.t. h, pos and every (W, b), pre-activation e of the first layer)"""
    centers, src = conv_block_host()[1], block_src(pos)
    M, K = src.shape
    pos = pos.double().clone().requires_grad_(True)
    h = None if h is None else h.double().clone().requires_grad_(True)
    params = [p.double().clone().requires_grad_(True) for p in params]
    s, d = src.flatten(), torch.arange(M).repeat_interleave(K)
    rel = pos[s] - pos[centers][d]
    e = rel if h is None else torch.cat([h[s], rel], 1)
    first = None
    for i in range(0, len(params), 2):
        e = e @ params[i].t() + params[i + 1]
        if first is None:
            first = e.detach()
        if batch_norm is not None:
            gamma, beta, eps = batch_norm
            e = (e - e.mean(0)) / torch.sqrt(e.var(0, unbiased=False) + eps) * gamma.double() + beta.double()
        e = torch.relu(e)
    e3 = e.view(M, K, -1)
    arg = e3.detach().argmax(1, keepdim=True)                                   # the first maximal value (torch.argmax's documented tie rule)
    out = e3.gather(1, arg)[:, 0]
    wrt = ([] if h is None else [h]) + [pos] + params
    grads = torch.autograd.grad((out * w.double()).sum(), wrt, allow_unused=True)
    return out.detach(), [torch.zeros_like(p) if g is None else g for g, p in zip(grads, wrt)], first


def conv_run(in_feats, sizes, h, pos, params, w, device, fused, monkeypatch, batch_norm=None):
    import dgl
    import dgl.geometry
    monkeypatch.setattr(config, "POINTNETCONV_FUSED", fused)
    centers, src = conv_block_host()[1], block_src(pos)
    p = pos.to(device).requires_grad_(True)
    block = dgl.geometry.fixed_radius_block(p, centers.to(device), CONV_RADIUS, CONV_K, list(CONV_LENS))
    assert torch.equal(block._index.csc().indices.cpu().long().view(-1, CONV_K), src)
    conv = dgl.nn.PointNetConv(in_feats, sizes, batch_norm=batch_norm is not None).to(device).train()
    assert dgl.nn.PointNetConv is mg.nn.PointNetConv
    own = [t for layer in conv.layers for t in (layer.weight, layer.bias)]
    with torch.no_grad():
        for t, v in zip(own, params):
            t.copy_(v)
        if batch_norm is not None:
            conv.bns[0].weight.copy_(batch_norm[0])
            conv.bns[0].bias.copy_(batch_norm[1])
    hh = None if h is None else h.to(device).requires_grad_(True)
    out = conv(block, hh)
    grads = torch.autograd.grad(out, ([] if hh is None else [hh]) + [p] + own, w.to(device))
    return out.detach().cpu(), [t.cpu() for t in grads]


def check_conv_exact(device, monkeypatch):
    pos = conv_block_host()[0]
    N, M = pos.shape[0], len(CONV_LENS) * CONV_PER
    for in_feats, sizes in ((0, (8,)), (5, (8,)), (5, (8, 6))):
        gen = torch.Generator().manual_seed(in_feats + len(sizes))
        ri = lambda *shape: torch.randint(-2, 3, shape, generator=gen).float()
        h = ri(N, in_feats) if in_feats else None
        params, fan = [], in_feats + 3
        for size in sizes:
            params += [ri(size, fan), ri(size)]
            fan = size
        w = ri(M, sizes[-1])
        ref_out, ref_grads, _ = conv_restated(h, pos, params, w)
        assert bool((ref_out > 0).any()) and bool((ref_out == 0).any())
        for fused in (True, False):
            out, grads = conv_run(in_feats, sizes, h, pos, params, w, device, fused, monkeypatch)
            what = (in_feats, sizes, fused)
            assert torch.equal(out.double(), ref_out), what
            assert len(grads) == len(ref_grads)
            for got, want in zip(grads, ref_grads):
                assert torch.equal(got.double(), want), what


def test_pointnetconv_integer_data_all_forms_equal(cpu_backend_on, monkeypatch):
    check_conv_exact("cpu", monkeypatch)


@functools.lru_cache(maxsize=None)
def float_conv_case(in_feats):
    """one layer: inputs, the fp64 reference, the bounds, and the conditions under which neither the arg nor the ReLU's side can differ,
    asserted on the reference alone: over a destination's DISTINCT sources the top-two gap of the pre-activation exceeds twice the
    forward bound, and so does the distance of the top from 0"""
    pos, centers, src = conv_block_host()
    N, (M, K), size = pos.shape[0], src.shape, 8
    for seed in range(50):
        gen = torch.Generator().manual_seed(100 * seed + in_feats)
        rn = lambda *shape: torch.randn(shape, generator=gen)
        fpos = pos + 0.25 * rn(N, 3)
        src = block_src(fpos)
        d64 = ((fpos.double()[centers].unsqueeze(1) - fpos.double().unsqueeze(0)) ** 2).sum(-1)
        r2 = radius2_of(CONV_RADIUS)
        if not bool(((d64 - r2).abs() > 5 * 2.0 ** -23 * r2).all()):           # a distance too near the radius: the ball could differ
            continue
        h = rn(N, in_feats) if in_feats else None
        params = [rn(size, in_feats + 3) / (in_feats + 3) ** 0.5, rn(size)]
        w = rn(M, size)
        out, grads, e = conv_restated(h, fpos, params, w)
        s, d = src.flatten(), torch.arange(M).repeat_interleave(K)
        arel = fpos.double().abs()[s] + fpos.double().abs()[centers][d]
        ae = (arel if h is None else torch.cat([h.double().abs()[s], arel], 1)) @ params[0].double().abs().t() + params[1].double().abs()
        fwd_edge = (in_feats + 3 + 3) * 2.0 ** -24 * ae                          # in = in_feats + 3 terms per dot product
        fwd_bound = fwd_edge.view(M, K, size).max(1).values
        ok = True
        for v in range(M):
            uniq = torch.unique(src[v])
            ev = e.view(M, K, size)[v][[src[v].tolist().index(int(u)) for u in uniq]]
            top = ev.topk(min(2, len(uniq)), dim=0).values
            ok = ok and bool((top[0].abs() > 2 * fwd_bound[v]).all()) and (len(uniq) < 2 or bool((top[0] - top[1] > 2 * fwd_bound[v]).all()))
        if not ok:
            continue
        # magnitudes of the gradients: the same expression over absolute values, the arg held fixed
        arg = torch.relu(e).view(M, K, size).argmax(1, keepdim=True)
        ap = fpos.double().abs().requires_grad_(True)
        ah = None if h is None else h.double().abs().requires_grad_(True)
        aw, ab = params[0].double().abs().requires_grad_(True), params[1].double().abs().requires_grad_(True)
        arel = ap[s] + ap[centers][d]
        aee = (arel if ah is None else torch.cat([ah[s], arel], 1)) @ aw.t() + ab
        live = (torch.relu(e).view(M, K, size).gather(1, arg)[:, 0] > 0).double()
        A_sel = aee.view(M, K, size).gather(1, arg)[:, 0] * live
        wrt = ([] if ah is None else [ah]) + [ap, aw, ab]
        A_grads = [torch.zeros_like(t) if g is None else g.detach()
                   for g, t in zip(torch.autograd.grad((A_sel * w.double().abs()).sum(), wrt, allow_unused=True), wrt)]
        out_deg = int(torch.bincount(s, minlength=N).max())
        T = ([] if h is None else [size * (out_deg + 2)]) + [size * (out_deg + K + 2), 2 * M * K, M * K]
        return h, fpos, params, w, out, grads, fwd_bound, A_grads, T, src
    raise AssertionError("no seed with clear margins")


def check_conv_float(device, monkeypatch):
    for in_feats in (0, 5):
        h, pos, params, w, ref_out, ref_grads, fwd_bound, A_grads, T, _ = float_conv_case(in_feats)
        for fused in (True, False):
            out, grads = conv_run(in_feats, (8,), h, pos, params, w, device, fused, monkeypatch)
            what = (in_feats, fused)
            err = (out.double() - ref_out).abs()
            assert bool((err <= fwd_bound).all()), "%s: forward %g of the bound" % (what, float((err / fwd_bound.clamp(min=1e-300)).max()))
            for got, want, A, t in zip(grads, ref_grads, A_grads, T):
                gerr, gbound = (got.double() - want).abs(), (t + 8) * 2.0 ** -23 * A
                assert bool((gerr <= gbound).all()), "%s: gradient %g of the bound" % (what, float((gerr / gbound.clamp(min=1e-300)).max()))


def test_pointnetconv_float_data_within_the_bounds(cpu_backend_on, monkeypatch):
    check_conv_float("cpu", monkeypatch)


def check_conv_batch_norm(device, monkeypatch):
    """batch_norm=True runs the composition whatever the switch says.  The bound is the one tests/test_knn.py derives for EdgeConv's
    batch-norm form: the pre-norm e carries at most de = (in + 3) eps A_e; with E edges the mean adds (E + 8) eps max|e|, so e - mu is off
    by at most 2 D_f, D_f = max_e de + (E + 8) eps max|e|; sigma by a relative 4 D_f / sigma plus (E + 8) eps of summation; the affine
    step and the final rounding 4 eps (|y| + |beta|).  The ReLU is 1-Lipschitz and the max errs by at most the largest bound among a
    row's edges."""
    eps = 2.0 ** -24
    pos, centers, src = conv_block_host()
    (M, K), size = src.shape, 8
    for in_feats in (0, 5):
        case = float_conv_case(in_feats)
        (h, fpos, params, w), src = case[:4], case[-1]
        gen = torch.Generator().manual_seed(3)
        gamma, beta = torch.rand(size, generator=gen) + 0.5, torch.randn(size, generator=gen)
        ref_out, _, e = conv_restated(h, fpos, params, w, batch_norm=(gamma, beta, 1e-5))
        s, d = src.flatten(), torch.arange(M).repeat_interleave(K)
        arel = fpos.double().abs()[s] + fpos.double().abs()[centers][d]
        ae = (arel if h is None else torch.cat([h.double().abs()[s], arel], 1)) @ params[0].double().abs().t() + params[1].double().abs()
        E = e.shape[0]
        Df = ((in_feats + 6) * eps * ae).max(0).values + (E + 8) * eps * e.abs().max(0).values
        sigma = torch.sqrt(e.var(0, unbiased=False) + 1e-5)
        y = (e - e.mean(0)) / sigma * gamma.double() + beta.double()
        yb = gamma.double() / sigma * 2 * Df + (y - beta.double()).abs() * (4 * Df / sigma + (E + 8) * eps) + 4 * eps * (y.abs() + beta.double().abs())
        bound = yb.view(M, K, size).max(1).values
        for fused in (True, False):
            out, _ = conv_run(in_feats, (size,), h, fpos, params, w, device, fused, monkeypatch, batch_norm=(gamma, beta))
            err = (out.double() - ref_out).abs()
            assert bool((err <= bound).all()), "%s: batch-norm forward %g of the bound" % ((in_feats, fused), float((err / bound.clamp(min=1e-300)).max()))


def test_pointnetconv_batch_norm_matches_the_restatement(cpu_backend_on, monkeypatch):
    check_conv_batch_norm("cpu", monkeypatch)


def test_pointnetconv_argument_errors(cpu_backend_on):
    import dgl
    import dgl.geometry
    pos, centers, _ = conv_block_host()
    block = dgl.geometry.fixed_radius_block(pos, centers, CONV_RADIUS, CONV_K, list(CONV_LENS))
    for bad in (lambda: mg.nn.PointNetConv(5, (8,))(block), lambda: mg.nn.PointNetConv(0, (8,))(block, torch.zeros(112, 5)),
                lambda: mg.nn.PointNetConv(0, ()), lambda: mg.nn.PointNetConv(0, (8,), pos_dim=2)(block)):
        with pytest.raises(mg.DGLError):
            bad()
    assert sorted(n for n, _ in mg.nn.PointNetConv(5, (8, 6), batch_norm=True).named_parameters()) == [
        "bns.0.bias", "bns.0.weight", "bns.1.bias", "bns.1.weight", "layers.0.bias", "layers.0.weight", "layers.1.bias", "layers.1.weight"]


@pytest.mark.gpu
def test_pointnetconv_on_the_device_integer_data(monkeypatch):
    check_conv_exact(DEV, monkeypatch)


@pytest.mark.gpu
def test_pointnetconv_on_the_device_float_data(monkeypatch):
    check_conv_float(DEV, monkeypatch)


@pytest.mark.gpu
def test_pointnetconv_on_the_device_batch_norm(monkeypatch):
    check_conv_batch_norm(DEV, monkeypatch)


# ----------------------------------------------------------------------------- the script
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dgl-0.5-benchmark_amd")
TINY = ["--clouds", "4", "--batch", "4", "--points", "64", "--npoints", "16", "8", "--radius", "0.4", "0.8", "--neighbors", "8", "8"]


def test_script_model_trains_one_tiny_epoch_on_the_cpu():
    """pointnet2.py's own parser, model and epoch loop on the OpenMP backend (the script's main() asks for a device)"""
    sys.path.insert(0, PKG)
    import pointnet2 as pn
    from mi355x_graph.datasets import POINT_SHAPES, shapes_like
    args = pn.make_parser().parse_args([])
    assert (args.points, args.batch, args.npoints, args.radius, args.neighbors) == (1024, 32, [512, 128], [0.2, 0.4], [32, 64])
    args = pn.make_parser().parse_args(TINY)
    xyz, label = shapes_like(4, 64, seed=2)
    was = mg.enable_cpu_backend(True)
    try:
        torch.manual_seed(0)
        model = pn.PointNet2(len(POINT_SHAPES), args.npoints, args.radius, args.neighbors)
        assert [tuple(layer.weight.shape) for c in model.convs for layer in c.layers] == [(64, 3), (64, 64), (128, 64), (128, 131), (128, 128), (256, 128)]
        loss = pn.train_epoch(model, torch.device("cpu"), xyz, label, 4, torch.optim.Adam(model.parameters(), lr=1e-3))
        assert math.isfinite(loss)
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    finally:
        mg.enable_cpu_backend(was)


@functools.lru_cache(maxsize=None)
def _script(*args):
    """(losses printed per epoch, whole output) of one run of the script"""
    env = dict(os.environ, PYTHONPATH=PKG)
    cmd = [sys.executable, os.path.join(PKG, "pointnet2.py")] + TINY + ["--dropout", "0", "--no-shuffle"] + list(args)
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
