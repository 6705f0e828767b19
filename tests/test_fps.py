"""Farthest point sampling: csrc/fps.hip (mgx_segment_fps), ops.segment_fps / segment_fps_fused, dgl.geometry.farthest_point_sampler /
FarthestPointSampler.

The reference everywhere is the restatement below, a Python loop over the segments and the samples in fp64 -- never the composed form
and never the kernel:

    mind = +inf;  cur = start (outside the segment: 0);  min(m, len) times: record (cur, mind[cur]), mark cur selected, d64 = ((seg[cur] -
    seg) ** 2).sum(-1), mind = d64 where d64 < mind (NaN: unchanged), cur = first unselected row of greatest mind;  index -1 / dist 0 past len

  exact   integer coordinates in [-3, 3] (ties and duplicates everywhere) and in [-50, 50] with D = 3 (long chains, few ties): every
          distance is an integer below 2^24, exact in fp32 in any order -- torch.equal on the index, bit equality on dist.  A run of m
          samples is a prefix of a run of more, so the restatement is computed once per case and sliced.
  float   normal / row-scaled / a cluster at 1000 + 1e-3 randn.  Trajectories are not compared; greedy validity is checked in fp64 along
          the trajectory the code took: with S_t the rows selected before rank t and m64(j) = min_{i in S_t} d64(i, j), the rows are
          distinct, m64(got[t]) >= (1 - (D + 2) 2^-23) max_{j unselected} m64(j), and dist[t] is within (D + 2) 2^-24 relative of
          m64(got[t]) -- the bound tests/test_knn.py derives: each squared difference carries at most 3 roundings, the sum D - 1 more,
          and two distances are compared.
The kernel's shape follows max_len: 256 threads x 1 point (max_len * (D | 1) <= 4096 floats), 512 x 2 (<= 8192 floats), 512 x 8,
1024 x 8 and 1024 x 16 (<= 38912 floats, 16384 points); every boundary has a length on each side."""
import ctypes
import functools

import pytest
import torch

import mi355x_graph as mg
import mi355x_graph.nn  # noqa: F401
from mi355x_graph import _lib, config, ops
import oracle_backend

DEV = "cuda:0"
INF = float("inf")
NAN = float("nan")


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ----------------------------------------------------------------------------- the restatement (loops over segments and samples, never the code under test)
def restated(lens, x, m, start=None):
    """(index int64 [S, m], dist fp64 [S, m]) by the definition, in fp64"""
    x = x.detach().cpu().double()
    S = len(lens)
    index = torch.full((S, m), -1, dtype=torch.int64)
    dist = torch.zeros((S, m), dtype=torch.float64)
    o = 0
    for s, n in enumerate(lens):
        seg = x[o:o + n]
        mind = torch.full((n,), INF, dtype=torch.float64)
        live = torch.ones(n, dtype=torch.bool)
        cur = 0
        if start is not None and 0 <= int(start[s]) < n:
            cur = int(start[s])
        for t in range(min(m, n)):
            index[s, t], dist[s, t] = o + cur, mind[cur]
            live[cur] = False
            d = ((seg[cur] - seg) ** 2).sum(-1)
            lower = live & (d < mind)
            mind[lower] = d[lower]
            if not bool(live.any()):
                break
            cur = int(torch.argmax(torch.where(live, mind, torch.full_like(mind, -1.0))))   # the first maximal value: the lowest row
        o += n
    assert o == x.shape[0]
    return index, dist


LENS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 0, 1000)      # empty, one point, below / at / above the wave and the 256-thread workgroup, several points per thread
LENS_SMALL = (0, 1, 2, 63, 64, 65, 255, 256)               # max_len 256: the 256 x 1 shape (D <= 15)
LENS_64 = (0, 1, 2, 63, 64, 65, 255, 256, 257, 0, 598)    # D = 64: 598 points is the limit
NPOINTS = (1, 2, 16, 64, 300)
DS = (1, 2, 3, 4, 64)
# one length on each side of every boundary of the dispatch, D = 3 (256 | 257, 1024 | 1025, 4096 | 4097, 8192 | 8193, 12970 | unsupported) and
# D = 64 (63 | 64, 126 | 127, 598 | unsupported)
BOUNDARY_3 = (1024, 1025, 4096, 4097, 8192, 8193, 12970)
BOUNDARY_64 = (63, 64, 126, 127, 598)


def lens_of(D):
    return LENS_64 if D == 64 else LENS


@functools.lru_cache(maxsize=None)
def int_points(lens, D, seed=0, span=3):
    return torch.randint(-span, span + 1, (sum(lens), D), generator=torch.Generator().manual_seed(1000 * D + seed)).float()


@functools.lru_cache(maxsize=None)
def int_case(lens, D, seed=0, span=3, m=300, start=None):
    x = int_points(lens, D, seed, span)
    return x, restated(lens, x, m, start)


@functools.lru_cache(maxsize=None)
def nan_case():
    """one point with a NaN coordinate (in the segment of 65), two in the segment of 257, and the segment of 63 NaN only"""
    x = int_points(LENS, 4, seed=1).clone()
    ends = torch.tensor(LENS).cumsum(0).tolist()
    s65, s63, s257 = LENS.index(65), LENS.index(63), LENS.index(257)
    x[ends[s65] - 30, 2] = NAN
    x[ends[s257] - 7, 0] = NAN
    x[ends[s257] - 200, 3] = NAN
    x[ends[s63] - 63:ends[s63]] = NAN
    return x, restated(LENS, x, 70)


def check_exact(got_index, got_dist, ref, m, what=""):
    ref_index, ref_dist = ref[0][:, :m], ref[1][:, :m]
    assert got_index.dtype == torch.int64 and tuple(got_index.shape) == tuple(ref_index.shape), what
    assert torch.equal(got_index.cpu(), ref_index), what
    if got_dist is not None:
        got = got_dist.cpu()
        assert got.dtype == torch.float32 and not got_dist.requires_grad, what
        assert torch.equal(bits(got), bits(ref_dist.float())), what


def fps(lens, x, m, device, start=None, max_len=None, return_dist=True, seglen_dtype=torch.int64):
    if torch.is_tensor(start):
        start = start.to(device)
    return ops.segment_fps(torch.tensor(lens, dtype=seglen_dtype).to(device), x.to(device), m, start=start, total=int(x.shape[0]),
                           max_len=max_len, return_dist=return_dist)


def launches(monkeypatch):
    rec = []
    monkeypatch.setattr(mg.sparse, "PROFILE", rec)
    return rec


def exact_cases(device, check_fused=None):
    """the cases both forms run: yields nothing, asserts"""
    for D in DS:
        lens = lens_of(D)
        x, ref = int_case(lens, D)
        for m in NPOINTS:
            seglen_dtype = torch.int32 if m % 2 else torch.int64
            if check_fused:
                check_fused(lens, x, m)
            index, dist = fps(lens, x, m, device, seglen_dtype=seglen_dtype)
            check_exact(index, dist, ref, m, (D, m))
            if m == 16:
                only = fps(lens, x, m, device, return_dist=False)
                assert torch.is_tensor(only) and torch.equal(only, index)
    x, ref = int_case(LENS_SMALL, 3)
    check_exact(*fps(LENS_SMALL, x, 64, device), ref, 64, "small")
    x, ref = int_case(LENS, 3, seed=2, span=50)                                # long chains with few ties
    check_exact(*fps(LENS, x, 300, device), ref, 300, "span 50")
    # start: an int, a tensor, out of range (taken as 0)
    S = len(LENS)
    x = int_points(LENS, 3)
    check_exact(*fps(LENS, x, 16, device, start=1), restated(LENS, x, 16, [1] * S), 16, "start 1")
    st = torch.tensor([0, 0, 1, 62, 63, 64, 254, 255, 256, 0, 999])
    check_exact(*fps(LENS, x, 16, device, start=st), restated(LENS, x, 16, st.tolist()), 16, "start tensor")
    bad = torch.tensor([5, 1, 2, -1, 64, 65, 10 ** 12, -2 ** 40, 257, 0, 1000])
    check_exact(*fps(LENS, x, 16, device, start=bad), restated(LENS, x, 16, bad.tolist()), 16, "start out of range")
    assert torch.equal(restated(LENS, x, 16, bad.tolist())[0][3:6, 0], torch.tensor([3, 66, 130]))   # ... is row 0 of the segment
    # NaN rows: selected right after the start, the lowest first; an all-NaN segment is taken in row order
    x, ref = nan_case()
    check_exact(*fps(LENS, x, 70, device), ref, 70, "nan")
    ends = torch.tensor(LENS).cumsum(0).tolist()
    s63, s257 = LENS.index(63), LENS.index(257)
    assert ref[0][s63, :63].tolist() == list(range(ends[s63] - 63, ends[s63]))
    assert ref[0][s257, 1:3].tolist() == [ends[s257] - 200, ends[s257] - 7] and bool((ref[1][s257, :3] == INF).all())
    # a row-strided x
    wide = int_points(LENS, 9)
    block = wide[:, 2:5]
    assert not block.is_contiguous()
    check_exact(*fps(LENS, block.to(device), 64, device), restated(LENS, block, 64), 64, "strided")


def boundary_cases(device, check_fused=None):
    for D, lengths in ((3, BOUNDARY_3), (64, BOUNDARY_64)):
        for n in lengths:
            x, ref = int_case((3, n, 5), D, seed=3, span=3, m=40)
            if check_fused:
                check_fused((3, n, 5), x, 40)
            check_exact(*fps((3, n, 5), x, 40, device), ref, 40, (D, n))


# ----------------------------------------------------------------------------- float cases
FLOAT_LENS = (20, 64, 65, 300, 1000)


@functools.lru_cache(maxsize=None)
def float_points(D, kind, lens=FLOAT_LENS):
    gen = torch.Generator().manual_seed(7 * D + len(kind))
    N = sum(lens)
    x = torch.randn(N, D, generator=gen)
    if kind == "scaled":
        x = x * torch.exp(4 * torch.randn(N, 1, generator=gen))
    elif kind == "cluster":
        x = 1000 + 1e-3 * x
    else:
        assert kind == "normal"
    return x


def check_greedy(got_index, got_dist, lens, x, m, D, what="", local=False):
    """greedy validity in fp64 along the trajectory the code took"""
    index, dist, x64 = got_index.cpu(), got_dist.cpu().double() if got_dist is not None else None, x.detach().cpu().double()
    o, worst = 0, 0.0
    for s, n in enumerate(lens):
        mm = min(m, n)
        got = index[s, :mm] - (0 if local else o)
        assert bool(((got >= 0) & (got < n)).all()), what
        assert len(set(got.tolist())) == mm, "%s: a row twice" % (what,)
        assert bool((index[s, mm:] == -1).all()), what
        seg = x64[o:o + n]
        m64 = torch.full((n,), INF, dtype=torch.float64)
        live = torch.ones(n, dtype=torch.bool)
        for t in range(mm):
            j = int(got[t])
            if t >= 1:
                best = float(m64[live].max())
                assert float(m64[j]) >= (1 - (D + 2) * 2.0 ** -23) * best, "%s: rank %d is not a farthest point" % (what, t)
                worst = max(worst, (best - float(m64[j])) / max(best, 1e-300) / ((D + 2) * 2.0 ** -23))
                if dist is not None:
                    assert abs(float(dist[s, t]) - float(m64[j])) <= (D + 2) * 2.0 ** -24 * float(m64[j]), "%s: dist of rank %d" % (what, t)
            elif dist is not None:
                assert float(dist[s, 0]) == INF, what
            live[j] = False
            m64 = torch.minimum(m64, ((seg[j] - seg) ** 2).sum(-1))
        o += n
    print("fps float %s: worst shortfall / bound %.3f" % (what, worst))


# ----------------------------------------------------------------------------- CPU: the composed form under the checker backend
@pytest.fixture
def cpu_backend_on():
    oracle_backend.install()
    yield
    oracle_backend.uninstall()


def test_restatement_by_hand():
    x = torch.tensor([[0.], [1.], [5.], [5.], [2.], [9.]])
    index, dist = restated([6], x, 8)
    assert index.tolist() == [[0, 5, 2, 4, 1, 3, -1, -1]]                      # the duplicate of row 2 last, at distance 0
    assert dist.tolist() == [[INF, 81., 16., 4., 1., 0., 0., 0.]]


def test_composition_matches_the_restatement_exactly(cpu_backend_on):
    def composed(lens, x, m):
        assert not ops.segment_fps_fused(torch.tensor(lens), x, m)
    exact_cases("cpu", composed)


def test_composition_at_the_kernels_boundaries(cpu_backend_on):
    boundary_cases("cpu")


@pytest.mark.parametrize("kind", ["normal", "scaled", "cluster"])
def test_composition_float_cases(cpu_backend_on, kind):
    for D in (1, 3, 64):
        lens = FLOAT_LENS[:4] if D == 64 else FLOAT_LENS
        x = float_points(D, kind, lens)
        index, dist = fps(lens, x, 48, "cpu")
        check_greedy(index, dist, lens, x, 48, D, "composition %s D=%d" % (kind, D))


def test_no_rows_no_segments_and_argument_errors(cpu_backend_on):
    index, dist = ops.segment_fps(torch.zeros(0, dtype=torch.int64), torch.zeros(0, 3), 4, return_dist=True)
    assert tuple(index.shape) == (0, 4) and tuple(dist.shape) == (0, 4)
    index, dist = ops.segment_fps(torch.tensor([0, 0]), torch.zeros(0, 3), 4, return_dist=True)
    assert torch.equal(index, torch.full((2, 4), -1)) and torch.equal(dist, torch.zeros(2, 4))
    x = int_points((5, 7), 3)
    seglen = torch.tensor([5, 7])
    for bad in (lambda: ops.segment_fps(seglen, x, 0), lambda: ops.segment_fps(seglen, x, True), lambda: ops.segment_fps(seglen, x, 2.0),
                lambda: ops.segment_fps(torch.tensor([5, 6]), x, 2), lambda: ops.segment_fps(seglen, x.double(), 2),
                lambda: ops.segment_fps(seglen, x[:, 0], 2), lambda: ops.segment_fps([5, 7], x, 2),
                lambda: ops.segment_fps(seglen, x, 2, start=1.5), lambda: ops.segment_fps(seglen, x, 2, start=torch.tensor([0])),
                lambda: ops.segment_fps(seglen, x, 2, start=torch.tensor([0, 1], dtype=torch.int32)),
                lambda: ops.segment_fps(seglen, x, 2, max_len=-1), lambda: ops.segment_fps(seglen, x, 2, max_len=7.0)):
        with pytest.raises(mg.DGLError):
            bad()


def test_without_a_cpu_backend_cpu_tensors_fail_loudly(monkeypatch):
    monkeypatch.delitem(mg.sparse._BACKENDS, "cpu", raising=False)
    with pytest.raises(mg.DGLError, match="MI355X"):
        ops.segment_fps(torch.tensor([5, 7]), int_points((5, 7), 3), 2)


def test_abi_argument_checks():
    L = _lib.lib()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("mgx_segment_fps_supported", "mgx_segment_fps"):
        assert hasattr(handle, name) and name in _lib.SIGNATURES
    assert L.mgx_abi_version() == 35
    assert config.FPS_FUSED is True
    for (D, n), want in (((3, 1), 1), ((3, 8192), 1), ((3, 12970), 1), ((3, 12971), 0), ((1, 16384), 1), ((1, 16385), 0), ((2, 12970), 1),
                         ((4, 7782), 1), ((4, 7783), 0), ((64, 598), 1), ((64, 599), 0), ((65, 10), 0), ((0, 10), 0), ((3, -1), 0)):
        assert L.mgx_segment_fps_supported(D, n) == want, (D, n)
    host = (ctypes.c_float * 64)()                                             # never dereferenced: every call below fails a check first
    p = ctypes.c_void_p(ctypes.addressof(host))

    def call(S=2, offsets=p, N=8, D=4, ld=4, x=p, m=2, max_len=8, start=p, index=p, dist=p):
        return L.mgx_segment_fps(S, offsets, N, D, ld, x, m, max_len, start, index, dist, None)

    assert call(m=0) == 1 and b"m must be at least 1" in L.mgx_last_error()
    with pytest.raises(mg.DGLError, match="m must be at least 1"):
        _lib.check(1)
    assert call(m=-3) == 1 and call(S=-1) == 1 and call(N=-1) == 1 and call(D=0) == 1 and call(max_len=-1) == 1
    assert call(ld=3) == 1 and b"row stride" in L.mgx_last_error()
    assert call(D=65, ld=65) == _lib.ERR_UNSUPPORTED and call(D=3, ld=3, max_len=12971) == _lib.ERR_UNSUPPORTED
    assert call(D=64, ld=64, max_len=599) == _lib.ERR_UNSUPPORTED
    assert call(N=2 ** 31) == _lib.ERR_UNSUPPORTED and call(N=2 ** 28, ld=4) == _lib.ERR_UNSUPPORTED   # 2^31 rows; 4 GiB of x
    assert call(S=2 ** 20, m=2 ** 11) == _lib.ERR_UNSUPPORTED                                          # 2^31 outputs
    assert call(offsets=None) == 1 and call(x=None) == 1 and call(index=None) == 1 and b"offsets / x / index is NULL" in L.mgx_last_error()
    assert call(S=0, offsets=None, x=None, index=None, dist=None, start=None) == 0                     # no segments: nothing to do


def check_sampler(device):
    import dgl
    import dgl.geometry
    import dgl.geometry.pytorch
    assert dgl.geometry.pytorch.FarthestPointSampler is dgl.geometry.FarthestPointSampler is mg.nn.FarthestPointSampler
    B, n, D = 3, 24, 3
    x = int_points((B * n,), D, seed=4)
    pos = x.view(B, n, D).to(device)
    got = dgl.geometry.farthest_point_sampler(pos, 7, start_idx=2)
    want = restated([n] * B, x, 7, [2] * B)[0] - torch.arange(B).unsqueeze(1) * n
    assert got.dtype == torch.int64 and tuple(got.shape) == (B, 7) and torch.equal(got.cpu(), want)    # numbers INSIDE each cloud
    for sampler in (lambda: dgl.geometry.farthest_point_sampler(pos, 7), lambda: dgl.geometry.FarthestPointSampler(7)(pos)):
        torch.manual_seed(3)
        rnd = sampler()                                                         # a random start per cloud
        assert tuple(rnd.shape) == (B, 7) and bool(((rnd >= 0) & (rnd < n)).all())
        check_greedy(rnd, None, [n] * B, x, 7, D, "sampler", local=True)
        again = restated([n] * B, x, 7, rnd[:, 0].tolist())[0] - torch.arange(B).unsqueeze(1) * n
        assert torch.equal(rnd.cpu(), again)                                    # integer data: the chain that follows the drawn start
    for bad in (lambda: dgl.geometry.farthest_point_sampler(pos, 25), lambda: dgl.geometry.farthest_point_sampler(pos, 0),
                lambda: dgl.geometry.farthest_point_sampler(pos[0], 3), lambda: dgl.geometry.farthest_point_sampler(pos, 3, start_idx=24),
                lambda: dgl.geometry.farthest_point_sampler(pos.long(), 3)):
        with pytest.raises(mg.DGLError):
            bad()


def test_dgl_geometry_sampler(cpu_backend_on):
    check_sampler("cpu")


# ----------------------------------------------------------------------------- GPU: the kernel against the restatement
def fused_one_launch(monkeypatch):
    def check(lens, x, m):
        assert ops.segment_fps_fused(torch.tensor(lens).to(DEV), x.to(DEV), m, total=int(x.shape[0]))
        rec = launches(monkeypatch)
        index, dist = fps(lens, x, m, DEV)
        assert [r["kernel"] for r in rec] == ["segment_fps"]                    # exactly one launch, nothing else from the library
        again_index, again_dist = fps(lens, x, m, DEV)                         # reruns give identical bits
        assert torch.equal(index, again_index) and torch.equal(bits(dist), bits(again_dist))
    return check


@pytest.mark.gpu
def test_kernel_matches_the_restatement_exactly(monkeypatch):
    exact_cases(DEV, fused_one_launch(monkeypatch))


@pytest.mark.gpu
def test_kernel_at_its_boundaries(monkeypatch):
    boundary_cases(DEV, fused_one_launch(monkeypatch))


@pytest.mark.gpu
def test_kernel_every_shape_on_the_same_segments():
    """max_len is an upper bound: a larger one picks a larger workgroup and more points per thread for the same segments, same result;
    a smaller one (a caller error) samples the first max_len rows of a longer segment and stays in bounds"""
    for D, max_lens in ((3, (1000, 1025, 4097, 8193, 12970)), (4, (1000, 1025, 4097, 7782))):
        x, ref = int_case(LENS, D)
        for max_len in max_lens:
            check_exact(*fps(LENS, x, 64, DEV, max_len=max_len), ref, 64, (D, max_len))
    x = int_points(LENS, 3)
    cut = [min(n, 100) for n in LENS]
    keep = torch.cat([torch.arange(o, o + c) for o, c in zip([0] + torch.tensor(LENS).cumsum(0).tolist()[:-1], cut)])
    index, dist = fps(LENS, x, 64, DEV, max_len=100)
    ref_index, ref_dist = restated(cut, x[keep], 64)
    assert torch.equal(index.cpu(), torch.where(ref_index >= 0, keep[ref_index.clamp(min=0)], ref_index))
    assert torch.equal(bits(dist), bits(ref_dist.float()))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["normal", "scaled", "cluster"])
def test_kernel_float_cases(kind):
    for D in (1, 3, 64):
        lens = FLOAT_LENS[:4] if D == 64 else FLOAT_LENS
        x = float_points(D, kind, lens)
        assert ops.segment_fps_fused(torch.tensor(lens).to(DEV), x.to(DEV), 48)
        index, dist = fps(lens, x, 48, DEV)
        check_greedy(index, dist, lens, x, 48, D, "kernel %s D=%d" % (kind, D))


@pytest.mark.gpu
def test_outside_the_kernels_set_takes_the_composition(monkeypatch):
    rec = launches(monkeypatch)
    lens = (3, 12971, 5)
    x, ref = int_case(lens, 3, seed=3, m=20)
    assert ops.segment_fps_fused(torch.tensor(lens[:1] + (12970,)).to(DEV), x[:12973].to(DEV), 20)
    assert not ops.segment_fps_fused(torch.tensor(lens).to(DEV), x.to(DEV), 20)
    check_exact(*fps(lens, x, 20, DEV), ref, 20, "12971 points")
    lens = (3, 599, 5)
    x, ref = int_case(lens, 64, seed=3, m=20)
    assert not ops.segment_fps_fused(torch.tensor(lens).to(DEV), x.to(DEV), 20)
    check_exact(*fps(lens, x, 20, DEV), ref, 20, "D = 64, 599 points")
    lens = (20, 70, 33)
    x, ref = int_case(lens, 65, m=20)
    assert ops.segment_fps_fused(torch.tensor(lens).to(DEV), x[:, :64].to(DEV), 20)
    assert not ops.segment_fps_fused(torch.tensor(lens).to(DEV), x.to(DEV), 20)
    check_exact(*fps(lens, x, 20, DEV), ref, 20, "D = 65")
    x, ref = int_case(LENS, 3)
    monkeypatch.setattr(config, "FPS_FUSED", False)
    assert not ops.segment_fps_fused(torch.tensor(LENS).to(DEV), x.to(DEV), 16)
    check_exact(*fps(LENS, x, 16, DEV), ref, 16, "switch off")
    assert not any(r["kernel"] == "segment_fps" for r in rec)


@pytest.mark.gpu
def test_captured_in_a_hip_graph():
    """the capture idiom of tests/test_knn.py: warm-up and capture on ONE side stream (a linear stream, no parallel branches), then replay
    with new points in the static input -- with total and max_len from the caller the operator reads nothing back to the host"""
    lens = LENS
    N = sum(lens)
    seglen = torch.tensor(lens).to(DEV)
    static = int_points(lens, 3).to(DEV).clone()
    outs = {}

    def step():
        outs["got"] = ops.segment_fps(seglen, static, 64, total=N, max_len=1000, return_dist=True)

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
    index, dist = outs["got"]
    eager_index, eager_dist = fps(lens, new, 64, DEV)
    assert torch.equal(index, eager_index) and torch.equal(bits(dist), bits(eager_dist))
    check_exact(index, dist, restated(lens, new, 64), 64)


@pytest.mark.gpu
def test_dgl_geometry_sampler_on_the_device(monkeypatch):
    rec = launches(monkeypatch)
    check_sampler(DEV)
    assert rec and all(r["kernel"] == "segment_fps" for r in rec)
