"""Sum of relu(x_u + w_e) messages: csrc/gine.hip (mgx_gine_*), ops.gine_sum, nn.GINEConv, graph_classification.py --fused-message.

The reference everywhere is the fp64 restatement below: a plain loop over the COO edge list on the fp32 inputs, written from

    out[v,:] = sum_{e: u->v} s[e] relu(x[u,:] + w[e,:])
    m[e,:]   = s[e] 1[x[u,:] + w[e,:] > 0] d_out[v,:];   d_w[e,:] = m[e,:];   d_x[u,:] = sum_{e: u->...} m[e,:]

(the fp64 sum of two fp32 numbers has the sign of their fp32 sum, so the restatement and the kernels agree on the mask).

  CPU   the composition behind ops.gine_sum (checker backend and the OpenMP backend), nn.GINEConv, argument errors, the C ABI's
        argument checks and its supported set, the launcher's switch: rtol 1e-5, atol 1e-6
  GPU   the fused kernels: per element |out - ref| <= 1e-4 sum_e |s| relu(.), |d_x - ref| <= 1e-4 sum_e |m|, d_w one product:
        1e-6 |ref| and exactly 0 under the mask; bitwise equality on integer-valued operands; zeros, subnormals, NaN, inf; bitwise
        equal reruns; the switch; peak memory against the operand sizes; the layer, the model and the captured step."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import mi355x_graph as mg
import mi355x_graph.nn  # noqa: F401
from mi355x_graph import _lib, config, ops, schedule, sparse
from conftest import random_graph
import oracle_backend

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dgl-0.5-benchmark_amd")
DEV = "cuda:0"
RTOL = 1e-4


# ----------------------------------------------------------------------------- the restatement (fp64, a loop over edges, never the code under test)
class Restated(object):
    def __init__(self, src, dst, n_src, n_dst, x, w, s=None, dout=None):
        src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
        x, w = (t.detach().cpu().numpy().astype(np.float64) for t in (x, w))
        E, D = w.shape
        s = np.ones(E) if s is None else s.detach().cpu().numpy().astype(np.float64).reshape(E)
        dout = None if dout is None else dout.detach().cpu().numpy().astype(np.float64)
        out, out_abs = np.zeros((n_dst, D)), np.zeros((n_dst, D))
        dx, dx_abs, dw = np.zeros((n_src, D)), np.zeros((n_src, D)), np.zeros((E, D))
        for e in range(E):
            u, v = src[e], dst[e]
            t = x[u] + w[e]
            r = np.where((t > 0) | np.isnan(t), t, 0.0)
            out[v] += s[e] * r
            out_abs[v] += abs(s[e]) * r
            if dout is not None:
                m = np.where(t > 0, s[e] * dout[v], 0.0)
                dw[e] = m
                dx[u] += m
                dx_abs[u] += np.abs(m)
        self.out, self.out_abs, self.dx, self.dx_abs, self.dw = (torch.from_numpy(a) for a in (out, out_abs, dx, dx_abs, dw))


def make_graph(src, dst, n_src, n_dst, device="cpu", idtype=torch.int32):
    s, d = torch.from_numpy(src), torch.from_numpy(dst)
    if n_src == n_dst:
        g = mg.graph((s, d), num_nodes=n_src)
        g = g.int() if idtype == torch.int32 else g.long()
        return g.to(device)
    return mg.create_block((s, d), n_src, n_dst, idtype=idtype, device=device)


def small_graph():
    """bipartite, 37 sources, 29 destinations, 300 edges from an unsorted COO: isolated destinations, duplicates, a self loop"""
    src, dst = random_graph(37, 29, 300, seed=3)
    src[:2], dst[:2] = (4, 9), (4, 9)
    return src, dst, 37, 29


def hubby_graph(n_src, n_dst, nnz, seed, hub_deg=3000):
    """the graph of tests/test_dot_attention.py: random + one hub destination (11) + one hub source (7) + destinations 0..4 without in-edges"""
    src, dst = random_graph(n_src, n_dst, nnz, seed=seed)
    rng = np.random.default_rng(seed)
    keep = dst >= 5
    src, dst = src[keep], dst[keep]
    hs = rng.integers(0, n_src, hub_deg)
    src = np.concatenate([src, hs, np.full(hub_deg, 7)])
    dst = np.concatenate([dst, np.full(hub_deg, 11), rng.integers(5, n_dst, hub_deg)])
    return src.astype(np.int64), dst.astype(np.int64)


def hub_graph():
    src, dst = hubby_graph(200, 200, 40 * 200, seed=17)
    return src, dst, 200, 200


GRAPHS = {"small": small_graph, "hubby": hub_graph}


def operands(n_src, n_dst, E, D, seed, scale=None):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(n_src, D, generator=gen)
    w = torch.randn(E, D, generator=gen)
    up = torch.randn(n_dst, D, generator=gen)
    s = None
    if scale == "positive":
        s = torch.rand(E, generator=gen) + 0.1
    elif scale == "signed":
        s = torch.randn(E, generator=gen)
    return x, w, s, up


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


@pytest.mark.parametrize("name", ["small", "square"])
def test_composition_and_its_gradients_match_the_restatement(cpu_backend_on, name):
    src, dst, n_src, n_dst = small_graph() if name == "small" else random_graph(60, 60, 700, seed=60) + (60, 60)
    assert len(set(zip(src.tolist(), dst.tolist()))) < len(src) and np.bincount(dst, minlength=n_dst).min() == 0
    g = make_graph(src, dst, n_src, n_dst)
    for D, kind in ((1, None), (6, "signed"), (16, "positive")):
        x, w, s, up = operands(n_src, n_dst, len(src), D, seed=D, scale=kind)
        x.requires_grad_(True)
        w.requires_grad_(True)
        assert not ops.gine_sum_fused(g, x, w, s)
        ref = Restated(src, dst, n_src, n_dst, x, w, s, up)
        for sc in (s, None if s is None else s.view(-1, 1)):
            out = ops.gine_sum(g, x, w, sc)
            assert tuple(out.shape) == (n_dst, D)
            assert torch.allclose(out.double(), ref.out, rtol=1e-5, atol=1e-6)
            assert torch.all(out[np.bincount(dst, minlength=n_dst) == 0] == 0)
            gx, gw = torch.autograd.grad((out * up).sum(), (x, w))
            assert torch.allclose(gx.double(), ref.dx, rtol=1e-5, atol=1e-6), (D, kind)
            assert torch.allclose(gw.double(), ref.dw, rtol=1e-5, atol=1e-6), (D, kind)


@pytest.mark.parametrize("block", [False, True])
def test_gine_conv_equals_the_restatement(cpu_backend_on, block):
    n_src, n_dst = (90, 40) if block else (60, 60)
    src, dst = random_graph(n_src, n_dst, 700, seed=5 + n_src)
    g = make_graph(src, dst, n_src, n_dst)
    torch.manual_seed(3)
    D = 8
    feat, efeat = torch.randn(n_src, D), torch.randn(700, D)
    ref = Restated(src, dst, n_src, n_dst, feat, efeat)
    plain = mg.nn.GINEConv()
    assert sorted(plain.state_dict()) == ["eps"] and not list(plain.parameters())
    out = plain(g, feat, efeat)
    assert tuple(out.shape) == (n_dst, D)
    assert torch.allclose(out.double(), feat[:n_dst].double() + ref.out, rtol=1e-5, atol=1e-6)
    lin = nn.Linear(D, 5)
    conv = mg.nn.GINEConv(lin, init_eps=0.25, learn_eps=True)
    assert [n_ for n_, _ in conv.named_parameters()] == ["eps", "apply_func.weight", "apply_func.bias"]
    seen = []                                                                    # what the layer hands to apply_func: rst itself
    hook = lin.register_forward_hook(lambda mod, args, res: seen.append(args[0].detach().clone()))
    out = conv(g, feat, efeat)
    hook.remove()
    assert len(seen) == 1 and tuple(out.shape) == (n_dst, 5)
    assert torch.allclose(seen[0].double(), 1.25 * feat[:n_dst].double() + ref.out, rtol=1e-5, atol=1e-6)
    assert torch.equal(out, lin(seen[0]))                                        # ... and the result is apply_func of it, nothing else
    out.sum().backward()
    d_rst = lin.weight.detach().sum(0).double()                                  # d sum(out) / d rst[v, :]
    want_eps = (feat[:n_dst].double() * d_rst).sum().view(1)
    print("eps.grad %.8f, restated %.8f" % (float(conv.eps.grad), float(want_eps)))
    assert torch.allclose(conv.eps.grad.double(), want_eps, rtol=1e-5, atol=1e-6)
    if block:                                                                    # a pair of inputs
        pair = conv(g, (feat, feat[:n_dst]), efeat)
        assert torch.allclose(pair, out, rtol=1e-5, atol=1e-6)
    import dgl.nn.pytorch as dglnn
    import dgl.ops as dglops
    assert dglnn.GINEConv is mg.nn.GINEConv and dglnn.conv.GINEConv is mg.nn.GINEConv
    assert dglops.gine_sum is ops.gine_sum and dglops.gine_sum_fused is ops.gine_sum_fused


def test_argument_errors_raise_dglerror(cpu_backend_on):
    src, dst = random_graph(20, 20, 100, seed=2)
    g = make_graph(src, dst, 20, 20)
    x, w, s = torch.randn(20, 8), torch.randn(100, 8), torch.rand(100)
    with pytest.raises(mg.DGLError, match=r"\(20, 2, 4\)"):
        ops.gine_sum(g, x.view(20, 2, 4), w)
    with pytest.raises(mg.DGLError, match=r"\(19, 8\)"):
        ops.gine_sum(g, x[:19], w)
    with pytest.raises(mg.DGLError, match=r"\(99, 8\)"):
        ops.gine_sum(g, x, w[:99])
    with pytest.raises(mg.DGLError, match=r"\(100, 4\)"):
        ops.gine_sum(g, x, w[:, :4])
    with pytest.raises(mg.DGLError, match=r"\(100, 2\)"):
        ops.gine_sum(g, x, w, torch.rand(100, 2))
    with pytest.raises(mg.DGLError, match="float32"):
        ops.gine_sum(g, x.double(), w.double())
    with pytest.raises(mg.DGLError, match="float32"):
        ops.gine_sum(g, x, w, s.double())
    with pytest.raises(mg.DGLError, match="no gradient"):
        ops.gine_sum(g, x, w, s.clone().requires_grad_(True))
    with pytest.raises(mg.DGLError):
        ops.gine_sum(g, x, None)
    assert "gine_sum" in ops.__all__ and "gine_sum_fused" in ops.__all__
    assert config.GINE_FUSED is True


def test_abi_argument_checks_and_supported_set():
    L = _lib.lib()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("mgx_gine_supported", "mgx_gine_workspace", "mgx_gine_fwd", "mgx_gine_bwd"):
        assert hasattr(handle, name) and name in _lib.SIGNATURES
    assert L.mgx_abi_version() == 35

    def fwd(c, D, x=None, w=None, s=None, out=None, plan=None, ws=None):
        return L.mgx_gine_fwd(None if c is None else ctypes.byref(c), plan, D, x, w, s, out, ws, None)

    def bwd(c, D, x=None, w=None, s=None, dout=None, dx=None, dw=None, plan=None):
        return L.mgx_gine_bwd(None if c is None else ctypes.byref(c), plan, D, x, w, s, dout, dx, dw, None, None)

    assert fwd(None, 8) == 1 and b"csr is NULL" in L.mgx_last_error()
    assert bwd(None, 8) == 1 and b"csr is NULL" in L.mgx_last_error()
    with pytest.raises(mg.DGLError):
        _lib.check(1)
    host = (ctypes.c_float * 1024)()                                            # never dereferenced: every call below fails a check first
    base = ctypes.addressof(host)
    base += (-base) % 16
    p, odd = ctypes.c_void_p(base), ctypes.c_void_p(base + 4)
    assert fwd(_lib.MgxCsr(4, 4, 8, base, base, None, 16, 0), 8) == 1           # idx_bits 16
    c64 = _lib.MgxCsr(4, 4, 8, base, base, None, 64, 0)
    assert fwd(c64, 8) == _lib.ERR_UNSUPPORTED and bwd(c64, 8) == _lib.ERR_UNSUPPORTED and not L.mgx_gine_supported(ctypes.byref(c64), 8)
    c = _lib.MgxCsr(4, 4, 8, base, base, None, 32, 0)
    for D in (4, 12, 100, 256):
        assert L.mgx_gine_supported(ctypes.byref(c), D), D
    for D in (0, 2, 6, 260):                                                    # the header: wider than 256 is not taken
        assert not L.mgx_gine_supported(ctypes.byref(c), D), D
    for D in (0, 2, 6, -4):                                                     # never a float4 row: an argument error
        assert fwd(c, D, p, p, None, p) == 1 and b"multiple of 4" in L.mgx_last_error(), D
        assert bwd(c, D, p, p, None, p, p, p) == 1, D
    assert fwd(c, 260, p, p, None, p) == _lib.ERR_UNSUPPORTED and bwd(c, 260, p, p, None, p, p, p) == _lib.ERR_UNSUPPORTED
    assert not L.mgx_gine_supported(None, 8)
    empty = _lib.MgxCsr(4, 4, 0, base, None, None, 32, 0)
    assert fwd(empty, 8, p, p, None, p) == _lib.ERR_UNSUPPORTED and not L.mgx_gine_supported(ctypes.byref(empty), 8)
    assert fwd(_lib.MgxCsr(4, 4, 8, None, base, None, 32, 0), 8, p, p, None, p) == 1   # indptr NULL
    assert fwd(c, 8) == 1 and b"NULL pointer" in L.mgx_last_error()
    assert fwd(c, 8, p, p, None, None) == 1 and fwd(c, 8, p, None, None, p) == 1 and fwd(c, 8, None, p, None, p) == 1
    assert fwd(c, 8, odd, p, None, p) == 1 and b"aligned" in L.mgx_last_error()
    assert fwd(c, 8, p, odd, None, p) == 1 and fwd(c, 8, p, p, None, odd) == 1
    assert bwd(c, 8) == 1 and b"NULL pointer" in L.mgx_last_error()
    assert bwd(c, 8, p, p, None, None, p, p) == 1                               # d_out NULL
    assert bwd(c, 8, p, p, None, p, odd, p) == 1 and bwd(c, 8, p, p, None, p, p, odd) == 1 and b"aligned" in L.mgx_last_error()
    # w and d_w are addressed by 32-bit byte offsets: nnz * D * 4 of 4 GiB is outside the supported set, as are x / out / d_out that large
    for rows, cols, nnz in ((4, 4, 2 ** 22), (2 ** 22, 4, 8), (4, 2 ** 22, 8)):
        big = _lib.MgxCsr(rows, cols, nnz, base, base, None, 32, 0)
        assert not L.mgx_gine_supported(ctypes.byref(big), 256) and fwd(big, 256, p, p, None, p) == _lib.ERR_UNSUPPORTED
        assert L.mgx_gine_supported(ctypes.byref(big), 252)
    assert L.mgx_gine_supported(ctypes.byref(_lib.MgxCsr(4, 4, 2 ** 22 - 1, base, base, None, 32, 0)), 256)
    # a malformed plan (plan_check)
    assert L.mgx_gine_workspace(None, 64) == 0
    bad = schedule.MgxSpmmPlan()
    bad.num_items = 4
    assert fwd(c, 8, p, p, None, p, plan=ctypes.byref(bad)) == 1 and b"malformed plan" in L.mgx_last_error()
    assert bwd(c, 8, p, p, None, p, p, p, plan=ctypes.byref(bad)) == 1 and b"malformed plan" in L.mgx_last_error()
    assert fwd(empty, 8, p, p, None, p, plan=ctypes.byref(bad)) == 1 and fwd(c64, 8, p, p, None, p, plan=ctypes.byref(bad)) == 1   # argument errors first
    hubs = schedule.MgxSpmmPlan()
    hubs.num_items, hubs.num_slots = 4, 3
    hubs.item_row = hubs.item_beg = hubs.item_end = hubs.item_node = base
    assert L.mgx_gine_workspace(ctypes.byref(hubs), 64) == 3 * 64 * 4
    assert fwd(c, 8, p, p, None, p, plan=ctypes.byref(hubs)) == 1 and b"hub tables" in L.mgx_last_error()
    hubs.hub_row = hubs.hub_slot_ptr = base
    assert fwd(c, 8, p, p, None, p, plan=ctypes.byref(hubs)) == 1 and b"workspace" in L.mgx_last_error()


def test_launcher_switch_parses_and_is_off_by_default():
    sys.path.insert(0, PKG)
    import graph_classification as gc
    assert gc.make_parser().parse_args([]).fused_message is False
    assert gc.make_parser().parse_args(["--fused-message", "--hipgraph"]).fused_message is True
    plain, fused = gc.GCN(8, 1, 2, 0.0), gc.GCN(8, 1, 2, 0.0, fused=True)
    assert not plain.fused and not plain.layers[0].fused and fused.fused and all(layer.fused for layer in fused.layers)
    assert sorted(plain.state_dict()) == sorted(fused.state_dict())


# ----------------------------------------------------------------------------- GPU
def last_kernel():
    return _lib.lib().mgx_last_spmm_kernel().decode()


@functools.lru_cache(maxsize=None)
def parity_case(name, D, kind):
    src, dst, n_src, n_dst = GRAPHS[name]()
    x, w, s, up = operands(n_src, n_dst, len(src), D, seed=D + len(src), scale=kind)
    return src, dst, n_src, n_dst, x, w, s, up, Restated(src, dst, n_src, n_dst, x, w, s, up)


def check_parity(out, dx, dw, ref, what=""):
    o, gx, gw = (t.detach().cpu().double() for t in (out, dx, dw))
    e_out, e_dx, e_dw = (o - ref.out).abs(), (gx - ref.dx).abs(), (gw - ref.dw).abs()
    print("%s: max err out / sum|s|relu %.3e, d_x / sum|m| %.3e, d_w / |ref| %.3e"
          % (what, float((e_out / (ref.out_abs + 1e-30)).max()), float((e_dx / (ref.dx_abs + 1e-30)).max()),
             float((e_dw / (ref.dw.abs() + 1e-30)).max())))
    assert not (e_out > RTOL * ref.out_abs).any()
    assert not (e_dx > RTOL * ref.dx_abs).any()
    assert not (e_dw > 1e-6 * ref.dw.abs()).any()
    assert torch.all(gw[ref.dw == 0] == 0)


def run_fused(g, x, w, s, up, need_w=True):
    """(out, d_x, d_w) of ops.gine_sum through autograd on the device"""
    xd, wd = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(need_w)
    sd = None if s is None else s.to(DEV)
    out = ops.gine_sum(g, xd, wd, sd)
    grads = torch.autograd.grad((out * up.to(DEV)).sum(), (xd, wd) if need_w else (xd,))
    return out.detach(), grads[0], grads[1] if need_w else None


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [None, "positive", "signed"])
@pytest.mark.parametrize("D", [4, 12, 64, 100, 256])
@pytest.mark.parametrize("name", ["small", "hubby"])
def test_fused_forward_and_gradients_match_the_restatement(name, D, kind):
    src, dst, n_src, n_dst, x, w, s, up, ref = parity_case(name, D, kind)
    g = make_graph(src, dst, n_src, n_dst, DEV)
    csc, csr = g._index.csc(), g._index.csr()
    assert csc.eids is not None and not torch.equal(csc.eids.cpu().long(), torch.arange(len(src)))   # a real permutation
    if name == "hubby":                                                            # chunked rows in both walks
        assert csc.plan().num_slots > 0 and csr.plan().num_slots > 0
    else:
        assert csc.plan() is None and csr.plan() is None                           # plan == NULL: one item per row
    xd, wd, upd = x.to(DEV), w.to(DEV), up.to(DEV)
    sd = None if s is None else s.to(DEV)
    assert ops.gine_sum_fused(g, xd, wd, sd)
    out = ops.gine_sum(g, xd, wd, sd)
    assert last_kernel() == "gine_fwd" and tuple(out.shape) == (n_dst, D)
    # the kernel name is kept per calling thread and autograd's backward runs on another: call the backend from this one
    be = sparse.backend_for(xd)
    dx, dw = be.gine_bwd(csr, xd, wd, sd, upd, True, True)
    assert last_kernel() == "gine_bwd"
    check_parity(out, dx, dw, ref, "%s D=%d scale=%s" % (name, D, kind))
    o2, gx, gw = run_fused(g, x, w, s, up)                                         # the same through autograd
    assert torch.equal(o2, out) and torch.equal(gx, dx) and torch.equal(gw, dw)
    only_x = be.gine_bwd(csr, xd, wd, sd, upd, True, False)                        # d_x and d_w may each be NULL
    only_w = be.gine_bwd(csr, xd, wd, sd, upd, False, True)
    assert only_x[1] is None and only_w[0] is None and torch.equal(only_x[0], dx) and torch.equal(only_w[1], dw)
    if sd is not None:
        assert torch.equal(ops.gine_sum(g, xd, wd, sd.view(-1, 1)), out)


def integer_operands(n_src, n_dst, E, D, seed):
    rng = np.random.default_rng(seed)
    x, w, up = (torch.from_numpy(rng.integers(-8, 9, shape).astype(np.float32)) for shape in ((n_src, D), (E, D), (n_dst, D)))
    s = torch.from_numpy(np.array([0.5, 1.0, 2.0], dtype=np.float32)[rng.integers(0, 3, E)])
    return x, w, s, up


@pytest.mark.gpu
@pytest.mark.parametrize("D", [4, 64])
@pytest.mark.parametrize("name", ["small", "hubby"])
def test_exact_arithmetic_is_bitwise(name, D):
    """integers in [-8, 8] and power-of-two scales: every product and every partial sum is exact in fp32 in any order, so a lost,
    doubled or misrouted edge or edge id changes a value and anything else is bitwise the restatement"""
    src, dst, n_src, n_dst = GRAPHS[name]()
    x, w, s, up = integer_operands(n_src, n_dst, len(src), D, seed=D)
    ref = Restated(src, dst, n_src, n_dst, x, w, s, up)
    assert float(ref.out_abs.max()) < 2 ** 24 and float(ref.dx_abs.max()) < 2 ** 24   # exactly representable sums
    g = make_graph(src, dst, n_src, n_dst, DEV)
    junk = torch.full((len(src), D), 12345.0, device=DEV)                          # a freed block torch.empty may hand back as d_w
    del junk
    out, dx, dw = run_fused(g, x, w, s, up)
    assert torch.equal(out.cpu(), ref.out.float()) and torch.equal(dx.cpu(), ref.dx.float())
    assert torch.equal(dw.cpu(), ref.dw.float())                                   # every row of d_w: written exactly once
    out1, dx1, dw1 = run_fused(g, x, w, None, up)
    ref1 = Restated(src, dst, n_src, n_dst, x, w, None, up)
    assert torch.equal(out1.cpu(), ref1.out.float()) and torch.equal(dx1.cpu(), ref1.dx.float()) and torch.equal(dw1.cpu(), ref1.dw.float())


@pytest.mark.gpu
def test_zero_and_sign_of_the_pre_activation():
    src, dst, n_src, n_dst = small_graph()
    E, D = len(src), 8
    x, w, s, up = operands(n_src, n_dst, E, D, seed=9, scale="signed")
    tiny = float(np.float32(2.0 ** -149))
    up = up.abs() + 0.5
    _, first = np.unique(src, return_index=True)                                   # four edges with different sources (x rows are set
    e_pz, e_nz, e_sub, e_sub2 = (int(e) for e in first[[1, 5, 9, 13]])             # independently), column 3 of each
    assert len({int(src[e]) for e in (e_pz, e_nz, e_sub, e_sub2)}) == 4
    x[src[e_pz], 3], w[e_pz, 3] = 1.5, -1.5                                        # +0
    x[src[e_nz], 3], w[e_nz, 3] = -0.0, -0.0                                       # -0
    x[src[e_sub], 3], w[e_sub, 3] = tiny, 0.0                                      # the smallest subnormal
    big = float(np.float32(2.0 ** -126))
    x[src[e_sub2], 3], w[e_sub2, 3] = big, -(big - tiny)                           # ... as the difference of the smallest normal and the largest subnormal number
    t = x[src] + w
    assert float(t[e_pz, 3]) == 0 and not np.signbit(t[e_pz, 3].numpy()) and float(t[e_nz, 3]) == 0 and np.signbit(t[e_nz, 3].numpy())
    assert float(t[e_sub, 3]) == tiny and float(t[e_sub2, 3]) == tiny and tiny > 0
    g = make_graph(src, dst, n_src, n_dst, DEV)
    ref = Restated(src, dst, n_src, n_dst, x, w, s, up)
    out, dx, dw = run_fused(g, x, w, s, up)
    check_parity(out, dx, dw, ref, "zero and sign")
    for e in (e_pz, e_nz):                                                         # at zero: no contribution, no gradient
        assert float(dw[e, 3]) == 0.0 and float(ref.dw[e, 3]) == 0.0
    for e in (e_sub, e_sub2):                                                      # at the subnormal: the gradient is s * d_out
        assert float(dw[e, 3]) == float(s[e] * up[dst[e], 3]) != 0.0
    # the zero edges alone on a destination of their own: the contribution is exactly 0, d_x too
    s2, d2 = np.array([0, 1, 2, 2]), np.array([0, 0, 1, 1])
    g2 = make_graph(s2, d2, 3, 2, DEV)
    x2 = torch.tensor([[1.5] * 4, [-0.0] * 4, [tiny] * 4])
    w2 = torch.tensor([[-1.5] * 4, [-0.0] * 4, [0.0] * 4, [0.0] * 4])
    sc2 = torch.tensor([-3.0, 2.0, 1.0, -0.5])
    up2 = torch.full((2, 4), 7.0)
    out, dx, dw = run_fused(g2, x2, w2, sc2, up2)
    assert torch.all(out[0] == 0) and torch.all(dx[:2] == 0) and torch.all(dw[:2] == 0)
    assert torch.equal(out[1].cpu(), torch.full((4,), tiny) * 1.0 + torch.full((4,), tiny) * -0.5)
    assert torch.equal(dw[2:].cpu(), torch.tensor([[7.0] * 4, [-3.5] * 4])) and torch.equal(dx[2].cpu(), torch.full((4,), 3.5))


@pytest.mark.gpu
@pytest.mark.parametrize("D", [12, 64])
def test_empty_rows_and_empty_graphs(D):
    src, dst, n_src, n_dst = hub_graph()
    keep = src != 9                                                                # source 9 loses its out-edges
    src, dst = src[keep], dst[keep]
    x, w, s, up = operands(n_src, n_dst, len(src), D, seed=4, scale="signed")
    g = make_graph(src, dst, n_src, n_dst, DEV)
    out, dx, dw = run_fused(g, x, w, s, up)
    no_in, no_out = np.bincount(dst, minlength=n_dst) == 0, np.bincount(src, minlength=n_src) == 0
    assert no_in[:5].all() and no_out[9]
    assert torch.all(out[torch.from_numpy(no_in).to(DEV)] == 0) and torch.all(dx[torch.from_numpy(no_out).to(DEV)] == 0)
    assert float(out.abs().sum()) > 0 and float(dx.abs().sum()) > 0
    # no edge at all: zeros of the right shape, zero gradients, and no kernel of the family
    empty = np.zeros(0, dtype=np.int64)
    for n_s, n_d in ((6, 6), (7, 3)):
        g0 = make_graph(empty, empty, n_s, n_d, DEV)
        x0, w0 = torch.randn(n_s, D, device=DEV, requires_grad=True), torch.zeros(0, D, device=DEV, requires_grad=True)
        ops.gspmm(g, "copy_lhs", "sum", x.to(DEV), None)                           # some other kernel's name
        before = last_kernel()
        assert not before.startswith("gine") and not ops.gine_sum_fused(g0, x0, w0)
        o0 = ops.gine_sum(g0, x0, w0)
        assert last_kernel() == before
        assert tuple(o0.shape) == (n_d, D) and torch.all(o0 == 0)
        gx0, gw0 = torch.autograd.grad(o0.sum(), (x0, w0))
        assert torch.all(gx0 == 0) and tuple(gw0.shape) == (0, D)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["small", "hubby"])
def test_one_nan_reaches_exactly_its_element_and_inf_passes(name):
    src, dst, n_src, n_dst = GRAPHS[name]()
    D = 16
    x, w, s, _ = operands(n_src, n_dst, len(src), D, seed=6, scale="positive")
    g = make_graph(src, dst, n_src, n_dst, DEV)
    xd, sd = x.to(DEV), s.to(DEV)
    clean = ops.gine_sum(g, xd, w.to(DEV), sd)
    assert torch.isfinite(clean).all()
    edges = [0, len(src) - 1] + ([int(np.nonzero(dst == 11)[0][2000])] if name == "hubby" else [])   # ... one deep in the hub row
    for e in edges:
        wn = w.clone()
        wn[e, 5] = float("nan")
        got = ops.gine_sum(g, xd, wn.to(DEV), sd)
        hit = torch.zeros(n_dst, D, dtype=torch.bool)
        hit[dst[e], 5] = True
        assert torch.equal(torch.isnan(got).cpu(), hit)
        assert torch.equal(got[~hit.to(DEV)], clean[~hit.to(DEV)])                 # bitwise
    u = int(src[0])
    xi = x.clone()
    xi[u, 2] = float("inf")
    got = ops.gine_sum(g, xi.to(DEV), w.to(DEV), sd)
    hit = torch.zeros(n_dst, D, dtype=torch.bool)
    hit[torch.from_numpy(np.unique(dst[src == u])), 2] = True
    assert torch.all(got[hit.to(DEV)] == float("inf")) and torch.equal(got[~hit.to(DEV)], clean[~hit.to(DEV)])


@pytest.mark.gpu
@pytest.mark.parametrize("D", [12, 256])
def test_reruns_are_bitwise_equal(D):
    src, dst, n_src, n_dst = hub_graph()
    x, w, s, up = operands(n_src, n_dst, len(src), D, seed=8, scale="signed")
    g = make_graph(src, dst, n_src, n_dst, DEV)
    first = run_fused(g, x, w, s, up)
    torch.empty(1 << 22, device=DEV).fill_(3.0)                                    # other allocations in between
    again = run_fused(make_graph(src, dst, n_src, n_dst, DEV), x, w, s, up)
    for a_, b_ in zip(first, again):
        assert torch.equal(a_, b_)


@pytest.mark.gpu
@pytest.mark.parametrize("name,D,kind", [("small", 12, "signed"), ("hubby", 64, "positive"), ("hubby", 256, None)])
def test_switch_takes_the_composition(monkeypatch, name, D, kind):
    src, dst, n_src, n_dst, x, w, s, up, ref = parity_case(name, D, kind)
    g = make_graph(src, dst, n_src, n_dst, DEV)
    fused = run_fused(g, x, w, s, up)
    monkeypatch.setattr(config, "GINE_FUSED", False)
    xd, wd = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
    sd = None if s is None else s.to(DEV)
    assert not ops.gine_sum_fused(g, xd, wd, sd)
    out = ops.gine_sum(g, xd, wd, sd)
    assert not last_kernel().startswith("gine")
    gx, gw = torch.autograd.grad((out * up.to(DEV)).sum(), (xd, wd))
    check_parity(out, gx, gw, ref, "composition %s D=%d" % (name, D))
    check_parity(*fused, ref, "fused %s D=%d" % (name, D))
    # unsupported shapes take the composition too, with the switch on
    monkeypatch.setattr(config, "GINE_FUSED", True)
    assert ops.gine_sum_fused(g, xd, wd, sd)
    x6, w6, s6, up6 = operands(n_src, n_dst, len(src), 6, seed=1, scale=kind)
    assert not ops.gine_sum_fused(g, x6.to(DEV), w6.to(DEV), None if s6 is None else s6.to(DEV))
    g64 = make_graph(src, dst, n_src, n_dst, DEV, idtype=torch.int64)
    assert not ops.gine_sum_fused(g64, xd, wd, sd)
    # a contiguous view at a storage offset that is no multiple of 16 bytes is not the kernels' either
    flat_x, flat_w = torch.zeros(x.numel() + 1, device=DEV), torch.zeros(w.numel() + 1, device=DEV)
    xo, wo = flat_x[1:].view(x.shape).copy_(x), flat_w[1:].view(w.shape).copy_(w)
    assert xo.is_contiguous() and xo.data_ptr() % 16 == 4
    assert not ops.gine_sum_fused(g, xo, wd, sd) and not ops.gine_sum_fused(g, xd, wo, sd)
    ops.gspmm(g, "copy_lhs", "sum", xd, None)
    off_out = ops.gine_sum(g, xo.requires_grad_(True), wo.requires_grad_(True), sd)
    assert not last_kernel().startswith("gine")
    check_parity(off_out, *torch.autograd.grad((off_out * up.to(DEV)).sum(), (xo, wo)), ref, "offset views")
    if name == "small":
        ref6 = Restated(src, dst, n_src, n_dst, x6, w6, s6, up6)
        check_parity(*run_fused(g, x6, w6, s6, up6), ref6, "D=6")
        check_parity(*run_fused(g64, x, w, s, up), ref, "int64 graph")


@pytest.mark.gpu
def test_no_edge_sized_temporary(monkeypatch):
    """N = 2000, E = 80 000, D = 64: E * D * 4 = 20.5 MB.  Forward + backward above the inputs: out, d_out and d_x are N * D * 4 = 0.5 MB
    each, so the fused call stays below half an [E, D] tensor without d_w and below one and a half with it (d_w itself is one); the
    composition keeps relu's output and holds the gradients of two of its steps at once: three at least."""
    n, E, D = 2000, 80000, 64
    src, dst = random_graph(n, n, E, seed=12)
    g = make_graph(src, dst, n, n, DEV)
    x, w, s, up = (t.to(DEV) for t in operands(n, n, E, D, seed=2, scale="positive"))
    unit = E * D * 4

    def peak(need_w):
        xd, wd = x.clone().requires_grad_(True), w.clone().requires_grad_(need_w)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = ops.gine_sum(g, xd, wd, s)
        grads = torch.autograd.grad((out * up).sum(), (xd, wd) if need_w else (xd,))
        torch.cuda.synchronize()
        top = torch.cuda.max_memory_allocated() - base
        del out, grads
        return top

    peak(True)                                                                     # CSRs, plans and workspaces exist from here on
    assert ops.gine_sum_fused(g, x, w, s)
    without, with_w = peak(False), peak(True)
    monkeypatch.setattr(config, "GINE_FUSED", False)
    peak(True)
    comp = peak(True)
    print("peak above the inputs / (E*D*4): fused %.3f, fused with d_w %.3f, composition %.3f" % (without / unit, with_w / unit, comp / unit))
    assert without < 0.5 * unit
    assert unit <= with_w < 1.5 * unit
    assert comp >= 3 * unit


@pytest.mark.gpu
def test_gine_conv_on_the_device():
    src, dst, n_src, n_dst = hub_graph()
    D = 64
    x, w, _, up = operands(n_src, n_dst, len(src), D, seed=5)
    ref = Restated(src, dst, n_src, n_dst, x, w, None, up)
    g = make_graph(src, dst, n_src, n_dst, DEV)
    conv = mg.nn.GINEConv(init_eps=0.5, learn_eps=True).to(DEV)
    xd, wd = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
    out = conv(g, xd, wd)
    assert last_kernel() == "gine_fwd"
    (out * up.to(DEV)).sum().backward()
    agg = out.detach().cpu().double() - 1.5 * x.double()
    scale = ref.out_abs + 1.5 * x.double().abs()
    assert not ((agg - ref.out).abs() > RTOL * scale).any()
    want_dx = ref.dx + 1.5 * up.double()
    assert not ((xd.grad.cpu().double() - want_dx).abs() > RTOL * (ref.dx_abs + 1.5 * up.double().abs())).any()
    assert not ((wd.grad.cpu().double() - ref.dw).abs() > 1e-6 * ref.dw.abs()).any()
    want_eps, eps_scale = float((x.double() * up.double()).sum()), float((x.double() * up.double()).abs().sum())
    assert abs(float(conv.eps.grad) - want_eps) <= RTOL * eps_scale


def _molhiv_batch(graphs=48, seed=5):
    sys.path.insert(0, PKG)
    import graph_classification as gc
    from mi355x_graph.datasets import molhiv_like
    from dgl.dataloading import GraphDataLoader
    data = molhiv_like(graphs, seed=seed)
    bg, labels = next(iter(GraphDataLoader(data, batch_size=graphs, shuffle=False)))
    return gc, data, bg, labels


def _eager_step(model, bg, labels):
    g = bg.to(DEV).int().formats("coo")
    model.zero_grad(set_to_none=True)
    out = model(g, g.ndata["feat"], g.edata["feat"])
    loss = F.binary_cross_entropy_with_logits(out.float().view(-1), labels.to(DEV).float().view(-1))
    loss.backward()
    return float(loss.detach()), [(n_, p.grad.clone()) for n_, p in model.named_parameters()]


@pytest.mark.gpu
def test_model_step_with_the_fused_message_on_and_off(monkeypatch):
    gc, _, bg, labels = _molhiv_batch()
    calls, real = [], sparse.HipBackend.gine_fwd
    monkeypatch.setattr(sparse.HipBackend, "gine_fwd", lambda self, *a: calls.append(1) or real(self, *a))
    torch.manual_seed(0)
    plain = gc.GCN(64, 1, 3, 0.0).to(DEV)
    fused = gc.GCN(64, 1, 3, 0.0, fused=True).to(DEV)
    fused.load_state_dict(plain.state_dict())
    plain.train()
    fused.train()
    loss_a, grads_a = _eager_step(plain, bg, labels)
    assert not calls
    loss_b, grads_b = _eager_step(fused, bg, labels)
    assert len(calls) == 3                                                         # one fused walk per layer, no silent fall-back
    print("loss: UDF %.8f, fused %.8f" % (loss_a, loss_b))
    assert abs(loss_a - loss_b) <= 1e-5 * abs(loss_a)
    for (na, ga), (nb, gb) in zip(grads_a, grads_b):
        err, top = float((ga - gb).abs().max()), float(ga.abs().max())
        print("%s: max err %.3e of max %.3e" % (na, err, top))
        assert na == nb and err <= 1e-4 * top, (na, err, top)


@pytest.mark.gpu
def test_captured_step_with_the_fused_message(monkeypatch):
    """GraphedBatchTrainer (the one-stream capture recipe): two replayed steps with --fused-message's model, the first one's loss equal to
    the eager fused step's; the fused walks run in the warm-up steps and inside the capture (no fall-back to the composition there)"""
    gc, data, bg, labels = _molhiv_batch(96)
    fwd_calls, bwd_calls, real_fwd, real_bwd = [], [], sparse.HipBackend.gine_fwd, sparse.HipBackend.gine_bwd
    monkeypatch.setattr(sparse.HipBackend, "gine_fwd",
                        lambda self, *a: fwd_calls.append(torch.cuda.is_current_stream_capturing()) or real_fwd(self, *a))
    monkeypatch.setattr(sparse.HipBackend, "gine_bwd", lambda self, *a: bwd_calls.append(1) or real_bwd(self, *a))
    torch.manual_seed(0)
    eager = gc.convert_masked_batchnorm(gc.GCN(64, 1, 3, 0.0, fused=True).to(DEV))
    model = gc.convert_masked_batchnorm(gc.GCN(64, 1, 3, 0.0, fused=True).to(DEV))
    model.load_state_dict(eager.state_dict())
    eager.train()
    model.train()
    want, _ = _eager_step(eager, bg, labels)
    assert fwd_calls == [False] * 3 and len(bwd_calls) == 3                        # three layers
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, capturable=True)
    n_pad, e_pad = gc.GraphedBatchTrainer.static_shape(data, 96)
    tr = gc.GraphedBatchTrainer(model, opt, nn.BCEWithLogitsLoss(), torch.device(DEV), 96, n_pad, e_pad)
    tr.step(bg, labels)
    first = tr.loss_value()
    assert fwd_calls[3:] == [False] * 6 + [True] * 3 and len(bwd_calls) == 12      # two warm-up steps, then the captured one
    tr.step(bg, labels)
    second = tr.loss_value()
    assert len(fwd_calls) == 12 and len(bwd_calls) == 12                           # a replay calls nothing
    print("eager fused %.8f, replay 1 %.8f, replay 2 %.8f" % (want, first, second))
    assert tr.stats["replayed"] == 2 and tr.stats["split"] == 0
    assert np.isfinite(first) and np.isfinite(second)
    assert abs(first - want) <= 1e-5 * abs(want)
