"""Scaled dot-product attention over a graph: csrc/dotattn.hip (mgx_dot_attention_*), ops.dot_attention, nn.DotGatConv, full_graph.DotGAT.

The reference everywhere is the fp64 restatement below, written from the definition over the COO edge list on the fp32 inputs:

    z[e,h] = scale * sum_f q[dst(e),h,f] k[src(e),h,f];  a = exp(z - m[dst]) / s[dst];  out[v,h,:] = sum_{e: u->v} a[e,h] v[u,h,:]
    t = <out, dout>;  dp[e,h] = <v[u,h,:], dout[v,h,:]>;  ds = a (dp - t) scale;  dq[v] = sum ds k[u], dk[u] = sum ds q[v], dv[u] = sum a dout[v]

  CPU   the composition behind ops.dot_attention (checker backend and the OpenMP backend), nn.DotGatConv, argument errors, the C ABI's
        argument checks: rtol 1e-5, atol 1e-6
  GPU   the fused kernels: forward per element |got - ref| <= 1e-4 * sum_e a |v| (the tests/test_gat_fused.py form), gradients
        1e-4 * the reference gradient tensor's max; bitwise equal reruns, aliased and strided operands, exact-arithmetic logits
        over a wide range, uniform attention, one NaN, the fallbacks, the layer and the model with the fused path on and off."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mi355x_graph as mg
import mi355x_graph.nn  # noqa: F401
from mi355x_graph import _lib, config, ops, sparse
from conftest import random_graph
import oracle_backend

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dgl-0.5-benchmark_amd")
DEV = "cuda:0"
RTOL = 1e-4


# ----------------------------------------------------------------------------- the restatement (fp64, COO, never the code under test)
class Restated(object):
    def __init__(self, src, dst, n_src, n_dst, q, k, v, scale, dout=None):
        src, dst = torch.as_tensor(src).long().cpu(), torch.as_tensor(dst).long().cpu()
        q, k, v = (t.detach().cpu().double() for t in (q, k, v))
        H, Fd = q.shape[1], q.shape[2]
        z = (q[dst] * k[src]).sum(-1) * scale                                             # [E, H]
        m = torch.full((n_dst, H), -float("inf"), dtype=torch.float64).index_reduce_(0, dst, z, "amax", include_self=True)
        e = torch.exp(z - m[dst])
        s = torch.zeros((n_dst, H), dtype=torch.float64).index_add_(0, dst, e)
        a = e / s[dst]
        self.z, self.a, self.dst, self.src = z, a, dst, src
        self.out = torch.zeros((n_dst, H, Fd), dtype=torch.float64).index_add_(0, dst, a.unsqueeze(-1) * v[src])
        self.row_scale = torch.zeros((n_dst, H, Fd), dtype=torch.float64).index_add_(0, dst, a.unsqueeze(-1) * v[src].abs())
        if dout is not None:
            dout = dout.detach().cpu().double()
            t = (self.out * dout).sum(-1)
            dp = (v[src] * dout[dst]).sum(-1)
            ds = (a * (dp - t[dst]) * scale).unsqueeze(-1)
            self.dq = torch.zeros((n_dst, H, Fd), dtype=torch.float64).index_add_(0, dst, ds * k[src])
            self.dk = torch.zeros((n_src, H, Fd), dtype=torch.float64).index_add_(0, src, ds * q[dst])
            self.dv = torch.zeros((n_src, H, Fd), dtype=torch.float64).index_add_(0, src, a.unsqueeze(-1) * dout[dst])


def composition(g, q, k, v, scale):
    return ops.gspmm(g, "mul", "sum", v, ops.edge_softmax(g, ops.gsddmm(g, "dot", k, q, "u", "v") * scale))


def make_graph(src, dst, n_src, n_dst, device="cpu", idtype=torch.int32):
    s, d = torch.from_numpy(src), torch.from_numpy(dst)
    if n_src == n_dst:
        g = mg.graph((s, d), num_nodes=n_src)
        g = g.int() if idtype == torch.int32 else g.long()
        return g.to(device)
    return mg.create_block((s, d), n_src, n_dst, idtype=idtype, device=device)


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


@pytest.mark.parametrize("n_src,n_dst", [(60, 60), (90, 40)])
def test_composition_and_its_gradients_match_the_restatement(cpu_backend_on, n_src, n_dst):
    src, dst = random_graph(n_src, n_dst, 700, seed=n_src)                    # isolated destinations, duplicate edges
    assert len(set(zip(src.tolist(), dst.tolist()))) < 700 and np.bincount(dst, minlength=n_dst).min() == 0
    g = make_graph(src, dst, n_src, n_dst)
    gen = torch.Generator().manual_seed(1)
    for H, Fd in ((1, 1), (3, 4), (2, 16)):
        q = torch.randn(n_dst, H, Fd, generator=gen).requires_grad_(True)
        k = torch.randn(n_src, H, Fd, generator=gen).requires_grad_(True)
        v = torch.randn(n_src, H, Fd, generator=gen).requires_grad_(True)
        up = torch.randn(n_dst, H, Fd, generator=gen)
        assert not ops.dot_attention_fused(g, q, k, v)
        for scale in (None, 0.37):
            sc = Fd ** -0.5 if scale is None else scale
            ref = Restated(src, dst, n_src, n_dst, q, k, v, sc, up)
            out = ops.dot_attention(g, q, k, v, scale)
            assert tuple(out.shape) == (n_dst, H, Fd)
            assert torch.allclose(out.double(), ref.out, rtol=1e-5, atol=1e-6)
            assert torch.all(out[np.bincount(dst, minlength=n_dst) == 0] == 0)
            gq, gk, gv = torch.autograd.grad((out * up).sum(), (q, k, v))
            for name, got, want in (("dq", gq, ref.dq), ("dk", gk, ref.dk), ("dv", gv, ref.dv)):
                err = float((got.double() - want).abs().max())
                print("%s H=%d F=%d: max err %.3e, max |reference| %.3e" % (name, H, Fd, err, float(want.abs().max())))
                assert torch.allclose(got.double(), want, rtol=1e-5, atol=1e-6), (name, H, Fd)


@pytest.mark.parametrize("block", [False, True])
def test_dot_gat_conv_equals_the_restatement(cpu_backend_on, block):
    n_src, n_dst = (90, 40) if block else (60, 60)
    src, dst = random_graph(n_src, n_dst, 700, seed=5 + n_src)
    g = make_graph(src, dst, n_src, n_dst)
    torch.manual_seed(3)
    H, Fd = 3, 4
    conv = mg.nn.DotGatConv(6, Fd, H)
    assert sorted(conv.state_dict()) == ["fc.weight"] and tuple(conv.fc.weight.shape) == (H * Fd, 6)
    feat = torch.randn(n_src, 6)
    with pytest.raises(mg.DGLError, match="0-in-degree"):
        conv(g, feat)
    conv.set_allow_zero_in_degree(True)
    h = (feat @ conv.fc.weight.detach().t()).view(n_src, H, Fd)
    ref = Restated(src, dst, n_src, n_dst, h[:n_dst], h, h, Fd ** -0.5)
    out = conv(g, feat)
    assert tuple(out.shape) == (n_dst, H, Fd)
    assert torch.allclose(out.double(), ref.out, rtol=1e-5, atol=1e-6)
    out2, att = conv(g, feat, get_attention=True)
    assert tuple(att.shape) == (700, H, 1)
    assert torch.allclose(out2, out, rtol=1e-5, atol=1e-6)
    assert torch.allclose(att.view(700, H).double(), ref.a, rtol=1e-5, atol=1e-6)   # edge-id order
    sums = torch.zeros(n_dst, H).index_add_(0, torch.from_numpy(dst), att.view(700, H).detach())
    has = torch.from_numpy(np.bincount(dst, minlength=n_dst) > 0)
    assert torch.allclose(sums[has], torch.ones_like(sums[has]), rtol=1e-5, atol=1e-6) and torch.all(sums[~has] == 0)
    if block:                                                                       # a pair of inputs goes through the same fc
        pair = conv(g, (feat, feat[:n_dst]))
        assert torch.allclose(pair, out, rtol=1e-5, atol=1e-6)
    assert mg.nn.DotGatConv(6, Fd, H, allow_zero_in_degree=True)(g, feat).shape == out.shape
    (out * torch.randn(n_dst, H, Fd)).sum().backward()
    assert conv.fc.weight.grad is not None and float(conv.fc.weight.grad.abs().max()) > 0
    import dgl.nn.pytorch as dglnn
    assert dglnn.DotGatConv is mg.nn.DotGatConv and dglnn.conv.DotGatConv is mg.nn.DotGatConv


def test_argument_errors_raise_dglerror(cpu_backend_on):
    src, dst = random_graph(20, 20, 100, seed=2)
    g = make_graph(src, dst, 20, 20)
    q, k, v = torch.randn(20, 2, 4), torch.randn(20, 2, 4), torch.randn(20, 2, 4)
    with pytest.raises(mg.DGLError, match=r"\(20, 8\)"):
        ops.dot_attention(g, q.view(20, 8), k, v)
    with pytest.raises(mg.DGLError, match=r"\(19, 2, 4\)"):
        ops.dot_attention(g, q[:19], k, v)
    with pytest.raises(mg.DGLError, match=r"\(20, 2, 8\)"):
        ops.dot_attention(g, q, k, torch.randn(20, 2, 8))
    with pytest.raises(mg.DGLError, match="float32"):
        ops.dot_attention(g, q.double(), k.double(), v.double())
    with pytest.raises(mg.DGLError):
        ops.dot_attention(g, q, k, None)
    assert "dot_attention" in ops.__all__ and "dot_attention_fused" in ops.__all__
    assert config.DOT_ATTENTION_FUSED is True


def test_abi_argument_checks():
    L = _lib.lib()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("mgx_dot_attention_supported", "mgx_dot_attention_workspace", "mgx_dot_attention_fwd", "mgx_dot_attention_bwd"):
        assert hasattr(handle, name) and name in _lib.SIGNATURES
    assert L.mgx_abi_version() == 35

    def fwd(c, H, Fd, q=None, q_ld=0, k=None, k_ld=0, v=None, v_ld=0, out=None, stat=None):
        return L.mgx_dot_attention_fwd(None if c is None else ctypes.byref(c), None, H, Fd, q, q_ld, k, k_ld, v, v_ld, ctypes.c_float(1.0),
                                       out, stat, None, None)

    assert fwd(None, 8, 16) == 1 and b"csr is NULL" in L.mgx_last_error()
    with pytest.raises(mg.DGLError):
        _lib.check(1)
    host = (ctypes.c_float * 1024)()                                            # never dereferenced: every call below fails a check first
    base = ctypes.addressof(host)
    base += (-base) % 16
    idx = ctypes.c_void_p(base)
    assert fwd(_lib.MgxCsr(4, 4, 8, base, base, None, 16, 0), 8, 16) == 1      # idx_bits 16
    c64 = _lib.MgxCsr(4, 4, 8, base, base, None, 64, 0)
    assert fwd(c64, 8, 16) == _lib.ERR_UNSUPPORTED and not L.mgx_dot_attention_supported(ctypes.byref(c64), 8, 16)
    c = _lib.MgxCsr(4, 4, 8, base, base, None, 32, 0)
    assert fwd(c, 0, 16) == 1 and fwd(c, 8, 0) == 1
    for H, Fd in ((1, 7), (1, 100), (1, 128), (8, 64), (2, 12), (1, 1)):
        assert fwd(c, H, Fd) == _lib.ERR_UNSUPPORTED, (H, Fd)
        assert not L.mgx_dot_attention_supported(ctypes.byref(c), H, Fd)
    for H, Fd in ((1, 4), (8, 16), (4, 64), (3, 16), (64, 4)):
        assert L.mgx_dot_attention_supported(ctypes.byref(c), H, Fd), (H, Fd)
    empty = _lib.MgxCsr(4, 4, 0, base, None, None, 32, 0)
    assert fwd(empty, 8, 16) == _lib.ERR_UNSUPPORTED and not L.mgx_dot_attention_supported(ctypes.byref(empty), 8, 16)
    assert fwd(_lib.MgxCsr(4, 4, 8, None, base, None, 32, 0), 8, 16) == 1      # indptr NULL
    assert fwd(c, 1, 8) == 1 and b"NULL pointer" in L.mgx_last_error()          # operands NULL
    assert fwd(c, 1, 8, idx, 8, idx, 8, idx, 8, idx, None) == 1                 # stat NULL
    assert fwd(c, 1, 8, idx, 6, idx, 8, idx, 8, idx, idx) == 1 and b"row stride" in L.mgx_last_error()   # stride no multiple of 4
    assert fwd(c, 1, 8, idx, 8, idx, 4, idx, 8, idx, idx) == 1                  # stride below H*F
    assert fwd(c, 1, 8, ctypes.c_void_p(base + 4), 8, idx, 8, idx, 8, idx, idx) == 1   # misaligned base
    assert L.mgx_dot_attention_workspace(None, 8, 16) == 0
    # 32-bit byte offsets: a dense [rows, H*F] operand of 4 GiB or more is outside the supported set, on either side of the graph
    for rows, cols in ((4194304, 4), (4, 4194304)):
        big = _lib.MgxCsr(rows, cols, 8, base, base, None, 32, 0)
        assert not L.mgx_dot_attention_supported(ctypes.byref(big), 4, 64) and fwd(big, 4, 64) == _lib.ERR_UNSUPPORTED
        assert L.mgx_dot_attention_supported(ctypes.byref(big), 4, 32) and L.mgx_dot_attention_supported(ctypes.byref(big), 1, 64)
    near = _lib.MgxCsr(4194303, 4194303, 8, base, base, None, 32, 0)
    assert L.mgx_dot_attention_supported(ctypes.byref(near), 4, 64)
    assert not L.mgx_dot_attention_supported(ctypes.byref(_lib.MgxCsr(2 ** 28, 4, 8, base, base, None, 32, 0)), 1, 4)   # stat: 16 bytes per head
    assert fwd(c, 1, 8, idx, 2 ** 28, idx, 8, idx, 8, idx, idx) == _lib.ERR_UNSUPPORTED      # a row stride that takes 4 rows to 4 GiB
    assert fwd(c, 1, 8, idx, 8, idx, 8, idx, 2 ** 28, idx, idx) == _lib.ERR_UNSUPPORTED
    t = _lib.MgxCsr(5, 4, 8, base, base, None, 32, 0)                           # not the transpose of c

    def bwd(csc, csr, H, Fd, p=None, ld=0):
        return L.mgx_dot_attention_bwd(None if csc is None else ctypes.byref(csc), None, None if csr is None else ctypes.byref(csr), None,
                                       H, Fd, p, ld, p, ld, p, ld, ctypes.c_float(1.0), p, p, p, p, p, p, None, None)

    assert bwd(None, c, 1, 8) == 1 and bwd(c, None, 1, 8) == 1
    assert bwd(c, t, 1, 8) == 1 and b"transposes" in L.mgx_last_error()
    assert bwd(c, c, 1, 7) == _lib.ERR_UNSUPPORTED and bwd(c64, c, 1, 8) == _lib.ERR_UNSUPPORTED
    assert bwd(c, c, 1, 8) == 1 and b"NULL pointer" in L.mgx_last_error()
    assert bwd(c, c, 1, 8, idx, 6) == 1


# ----------------------------------------------------------------------------- GPU
def hubby_graph(n_src, n_dst, nnz, seed, hub_deg=3000):
    """random graph + one hub destination (chunked rows) + one hub source + destinations 0..4 without in-edges (tests/test_gat_fused.py)"""
    src, dst = random_graph(n_src, n_dst, nnz, seed=seed)
    rng = np.random.default_rng(seed)
    keep = dst >= 5
    src, dst = src[keep], dst[keep]
    hs = rng.integers(0, n_src, hub_deg)
    src = np.concatenate([src, hs, np.full(hub_deg, 7)])
    dst = np.concatenate([dst, np.full(hub_deg, 11), rng.integers(5, n_dst, hub_deg)])
    return src.astype(np.int64), dst.astype(np.int64)


def operands(n_src, n_dst, H, Fd, seed):
    gen = torch.Generator().manual_seed(seed)
    q = torch.randn(n_dst, H, Fd, generator=gen)
    k = torch.randn(n_src, H, Fd, generator=gen)
    v = torch.randn(n_src, H, Fd, generator=gen)
    up = torch.randn(n_dst, H, Fd, generator=gen)
    return q, k, v, up


def check_forward(got, ref):
    err = (got.detach().cpu().double() - ref.out).abs()
    worst = float((err / (ref.row_scale + 1e-30)).max())
    print("forward: max err / sum_e a|v| = %.3e" % worst)
    assert not (err > RTOL * ref.row_scale + 1e-30).any(), worst


def check_grads(got, ref, names=("dq", "dk", "dv")):
    for name, g_ in zip(names, got):
        want = getattr(ref, name)
        err, top = float((g_.detach().cpu().double() - want).abs().max()), float(want.abs().max())
        print("%s: max err %.3e, max |reference| %.3e" % (name, err, top))
        assert err <= RTOL * top, (name, err, top)


def last_kernel():
    return _lib.lib().mgx_last_spmm_kernel().decode()


SHAPES = [(300, 1, 4), (900, 1, 16), (700, 4, 8), (900, 8, 16), (500, 2, 64), (400, 1, 64), (600, 4, 64)]
IDLE_LANES = [(500, 3, 16), (400, 5, 8), (300, 3, 4)]   # H*F/4 = 12, 10, 3 lanes in a group of 16, 16, 4: the rest of the group idles


@pytest.mark.gpu
@pytest.mark.parametrize("n,H,Fd", SHAPES + IDLE_LANES + [("block", 8, 16)])
def test_fused_forward_matches_the_restatement(n, H, Fd):
    n_src, n_dst = (900, 300) if n == "block" else (n, n)
    src, dst = hubby_graph(n_src, n_dst, 40 * n_src, seed=H * 100 + Fd)
    g = make_graph(src, dst, n_src, n_dst, DEV)
    q, k, v, _ = operands(n_src, n_dst, H, Fd, H + Fd)
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    assert ops.dot_attention_fused(g, qd, kd, vd)
    out = ops.dot_attention(g, qd, kd, vd)
    assert last_kernel() == "dot_attn_fwd"
    assert tuple(out.shape) == (n_dst, H, Fd)
    check_forward(out, Restated(src, dst, n_src, n_dst, q, k, v, Fd ** -0.5))
    assert torch.all(out[:5] == 0)                       # destinations without in-edges aggregate to exactly 0
    assert torch.equal(ops.dot_attention(g, qd, kd, vd), out)
    check_forward(ops.dot_attention(g, qd, kd, vd, 0.7), Restated(src, dst, n_src, n_dst, q, k, v, 0.7))


@pytest.mark.gpu
@pytest.mark.parametrize("n,H,Fd", SHAPES[:5] + IDLE_LANES + [("block", 4, 8)])
def test_fused_gradients_match_the_restatement_and_the_composition(n, H, Fd):
    n_src, n_dst = (900, 300) if n == "block" else (n, n)
    src, dst = hubby_graph(n_src, n_dst, 40 * n_src, seed=H * 7 + Fd)
    g = make_graph(src, dst, n_src, n_dst, DEV)
    q0, k0, v0, up0 = operands(n_src, n_dst, H, Fd, 3 * H + Fd)
    sc = Fd ** -0.5
    ref = Restated(src, dst, n_src, n_dst, q0, k0, v0, sc, up0)
    up = up0.to(DEV)

    def leaves():
        return [t.to(DEV).requires_grad_(True) for t in (q0, k0, v0)]

    ins = leaves()
    out = ops.dot_attention(g, *ins)
    check_forward(out, ref)
    (out * up).sum().backward(retain_graph=True)
    first = [t.grad.clone() for t in ins]
    check_grads(first, ref)
    for t in ins:                                        # a second backward over the same saved tensors: t is rewritten, nothing accumulates
        t.grad = None
    (out * up).sum().backward()
    for a_, b_ in zip(first, ins):
        assert torch.equal(a_, b_.grad)
    again = leaves()                                     # a rerun: bitwise (no atomics anywhere)
    out2 = ops.dot_attention(g, *again)
    (out2 * up).sum().backward()
    assert torch.equal(out2, out)
    for a_, b_ in zip(first, again):
        assert torch.equal(a_, b_.grad)
    comp = leaves()                                      # the composition on the device
    (composition(g, comp[0], comp[1], comp[2], sc) * up).sum().backward()
    for name, a_, b_, want in zip(("dq", "dk", "dv"), first, comp, (ref.dq, ref.dk, ref.dv)):
        err = float((a_ - b_.grad).abs().max())
        assert err <= RTOL * float(want.abs().max()), (name, err)
    # needs_input_grad subsets
    qd, kd, vd = (t.to(DEV) for t in (q0, k0, v0))
    only_q = qd.clone().requires_grad_(True)
    (ops.dot_attention(g, only_q, kd, vd) * up).sum().backward()
    assert torch.equal(only_q.grad, first[0])
    only_v = vd.clone().requires_grad_(True)
    (ops.dot_attention(g, qd, kd, only_v) * up).sum().backward()
    assert torch.equal(only_v.grad, first[2])
    only_k = kd.clone().requires_grad_(True)             # d k without d q: t comes from the small kernel
    (ops.dot_attention(g, qd, only_k, vd) * up).sum().backward()
    check_grads([only_k.grad], ref, names=("dk",))
    none = ops.dot_attention(g, qd, kd, vd)
    assert not none.requires_grad and torch.equal(none, out.detach())
    # the kernel that ran (the name is kept per calling thread, autograd's backward runs on another: call the backend from this one)
    be, gi = sparse.backend_for(up), g._index
    o, st = be.dot_attention_fwd(gi.csc(), qd, kd, vd, sc)
    assert last_kernel() == "dot_attn_fwd" and torch.equal(o, out.detach())
    dq, dk, dv = be.dot_attention_bwd(gi.csc(), gi.csr(), qd, kd, vd, sc, o, up, st, True, False, False)
    assert last_kernel() == "dot_attn_bwd_dst" and dk is None and dv is None and torch.equal(dq, first[0])
    dq, dk, dv = be.dot_attention_bwd(gi.csc(), gi.csr(), qd, kd, vd, sc, o, up, st, True, True, True)
    assert last_kernel() == "dot_attn_bwd_src" and all(torch.equal(a_, b_) for a_, b_ in zip((dq, dk, dv), first))


@pytest.mark.gpu
@pytest.mark.parametrize("H,Fd", [(1, 16), (8, 16), (2, 64)])
def test_aliased_operands(H, Fd):
    n = 600
    src, dst = hubby_graph(n, n, 40 * n, seed=H + Fd)
    g = make_graph(src, dst, n, n, DEV)
    q0, k0, _, up0 = operands(n, n, H, Fd, 11)
    up, sc = up0.to(DEV), Fd ** -0.5
    # k is v
    ref = Restated(src, dst, n, n, q0, k0, k0, sc, up0)
    q, k = q0.to(DEV).requires_grad_(True), k0.to(DEV).requires_grad_(True)
    out = ops.dot_attention(g, q, k, k)
    assert torch.equal(out, ops.dot_attention(g, q.detach(), k.detach(), k.detach().clone()))
    check_forward(out, ref)
    (out * up).sum().backward()
    check_grads([q.grad], ref, names=("dq",))
    want = ref.dk + ref.dv
    err = float((k.grad.cpu().double() - want).abs().max())
    assert err <= RTOL * float(want.abs().max()), err
    # q is k is v
    ref = Restated(src, dst, n, n, k0, k0, k0, sc, up0)
    x = k0.to(DEV).requires_grad_(True)
    out = ops.dot_attention(g, x, x, x)
    xd = x.detach()
    assert torch.equal(out, ops.dot_attention(g, xd.clone(), xd.clone(), xd.clone()))
    check_forward(out, ref)
    (out * up).sum().backward()
    want = ref.dq + ref.dk + ref.dv
    err = float((x.grad.cpu().double() - want).abs().max())
    assert err <= RTOL * float(want.abs().max()), err


@pytest.mark.gpu
@pytest.mark.parametrize("H,Fd", [(1, 4), (8, 16), (4, 64)])
def test_strided_operands_are_column_blocks_of_one_projection(H, Fd):
    n, D = 500, H * Fd
    src, dst = hubby_graph(n, n, 40 * n, seed=2 * H + Fd)
    g = make_graph(src, dst, n, n, DEV)
    torch.manual_seed(H)
    qkv = torch.randn(n, 3 * D, device=DEV).requires_grad_(True)
    up = torch.randn(n, H, Fd, device=DEV)
    q, k, v = (qkv[:, i * D:(i + 1) * D].view(n, H, Fd) for i in range(3))
    assert not q.is_contiguous() and sparse.HipBackend._dot_operand(k)[0] is k and sparse.HipBackend._dot_operand(k)[1] == 3 * D
    out = ops.dot_attention(g, q, k, v)
    (out * up).sum().backward()
    dense = [t.detach().contiguous().requires_grad_(True) for t in (q, k, v)]
    out_d = ops.dot_attention(g, *dense)
    (out_d * up).sum().backward()
    assert torch.equal(out, out_d)
    assert torch.equal(qkv.grad, torch.cat([t.grad.view(n, D) for t in dense], 1))


def _ranged_case(order):
    """q, k integer-valued in [-4, 4], F = 8, scale = 0.25: every logit is an exact multiple of 0.25 in [-32, 32] in any summation
    order.  The edges of every row (the hub row too) are laid out so that the logits ascend (the running maximum grows at every
    step) or descend along the CSR order -- the COO -> CSR conversion is stable."""
    n, H, Fd = 600, 4, 8
    src, dst = hubby_graph(n, n, 40 * n, seed=31)
    rng = np.random.default_rng(9)
    vals = np.array([-4., -3., 3., 4.], dtype=np.float32)
    q = torch.from_numpy(vals[rng.integers(0, 4, (n, H, Fd))])
    k = torch.from_numpy(vals[rng.integers(0, 4, (n, H, Fd))])
    z0 = (q[torch.from_numpy(dst)][:, 0] * k[torch.from_numpy(src)][:, 0]).sum(-1).numpy() * 0.25   # head 0's logit orders the row
    perm = np.lexsort((z0 if order == "ascending" else -z0, dst))
    return n, H, Fd, src[perm], dst[perm], q, k


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_exact_logits_over_a_wide_range(order):
    n, H, Fd, src, dst, q0, k0 = _ranged_case(order)
    gen = torch.Generator().manual_seed(4)
    v0, up0 = torch.randn(n, H, Fd, generator=gen), torch.randn(n, H, Fd, generator=gen)
    ref = Restated(src, dst, n, n, q0, k0, v0, 0.25, up0)
    # from the reference alone: the logits are the exact multiples of 0.25 claimed, ordered as claimed, and span a wide range
    assert torch.equal(ref.z * 4, (ref.z * 4).round()) and float(ref.z.abs().max()) <= 32
    z0 = ref.z[:, 0].numpy()
    same_row = dst[1:] == dst[:-1]
    step = np.diff(z0)[same_row]
    assert np.all(step >= 0) if order == "ascending" else np.all(step <= 0)
    deg = np.bincount(dst, minlength=n)
    hi = torch.full((n, H), -float("inf"), dtype=torch.float64).index_reduce_(0, ref.dst, ref.z, "amax")
    lo = torch.full((n, H), float("inf"), dtype=torch.float64).index_reduce_(0, ref.dst, ref.z, "amin")
    span = (hi - lo)[torch.from_numpy(deg >= 2)]
    wide = float((span >= 16).double().mean())
    print("share of (row, head) pairs with >= 2 edges whose logits span >= 16: %.3f" % wide)
    assert wide >= 0.5 and float((hi - lo)[11].min()) >= 16            # the hub row too
    g = make_graph(src, dst, n, n, DEV)
    csc = g._index.csc()                                               # the order the kernels walk: head 0's logits along every row
    indptr, eids = csc.indptr.cpu().long().numpy(), (None if csc.eids is None else csc.eids.cpu().long().numpy())
    z_csr = z0 if eids is None else z0[eids]
    assert np.array_equal(csc.indices.cpu().long().numpy(), src if eids is None else src[eids])
    inner = np.ones(len(z_csr) - 1, dtype=bool)
    inner[indptr[1:-1][(indptr[1:-1] > 0) & (indptr[1:-1] < len(z_csr))] - 1] = False    # steps that cross a row boundary
    step = np.diff(z_csr)[inner]
    assert np.all(step >= 0) if order == "ascending" else np.all(step <= 0)
    assert (step != 0).sum() > len(step) // 4                         # logits tie (257 values, a 3000-edge hub row), but not mostly
    ins = [t.to(DEV).requires_grad_(True) for t in (q0, k0, v0)]
    assert ops.dot_attention_fused(g, *ins)
    out = ops.dot_attention(g, ins[0], ins[1], ins[2], 0.25)
    check_forward(out, ref)
    (out * up0.to(DEV)).sum().backward()
    check_grads([t.grad for t in ins], ref)


@pytest.mark.gpu
def test_zero_queries_give_the_mean_of_the_neighbours():
    n, H, Fd = 700, 4, 8
    src, dst = hubby_graph(n, n, 40 * n, seed=13)
    g = make_graph(src, dst, n, n, DEV)
    rng = np.random.default_rng(2)
    v0 = torch.from_numpy(rng.integers(-8, 9, (n, H, Fd)).astype(np.float32))
    k0 = torch.randn(n, H, Fd)
    out = ops.dot_attention(g, torch.zeros(n, H, Fd, device=DEV), k0.to(DEV), v0.to(DEV)).cpu().double()
    d = torch.from_numpy(dst)
    tot = torch.zeros(n, H, Fd, dtype=torch.float64).index_add_(0, d, v0.double()[torch.from_numpy(src)])
    mean = tot / torch.from_numpy(np.bincount(dst, minlength=n)).clamp(min=1).double().view(n, 1, 1)
    assert torch.all((out - mean).abs() <= 1e-6 * mean.abs())          # a lost or doubled edge moves an element by >= 1 / degree


@pytest.mark.gpu
def test_one_nan_in_k_reaches_exactly_its_destinations():
    n, H, Fd = 600, 4, 16
    src, dst = hubby_graph(n, n, 40 * n, seed=21)
    g = make_graph(src, dst, n, n, DEV)
    q0, k0, v0, _ = operands(n, n, H, Fd, 6)
    clean = ops.dot_attention(g, q0.to(DEV), k0.to(DEV), v0.to(DEV))
    assert not torch.isnan(clean).any()
    for u0, h0 in ((7, 2), (int(src[0]), 0)):                           # the hub source (its edges reach the hub row too), an ordinary one
        kn = k0.clone()
        kn[u0, h0, 5] = float("nan")
        got = ops.dot_attention(g, q0.to(DEV), kn.to(DEV), v0.to(DEV))
        hit = torch.zeros(n, H, dtype=torch.bool)
        hit[torch.from_numpy(np.unique(dst[src == u0])), h0] = True
        assert u0 != 7 or hit[11, h0]
        hit = hit.to(DEV)
        assert torch.equal(torch.isnan(got), hit.unsqueeze(-1).expand(n, H, Fd))
        assert torch.equal(got[~hit], clean[~hit])                      # bitwise


@pytest.mark.gpu
@pytest.mark.parametrize("H,Fd,idtype", [(1, 7, torch.int32), (1, 100, torch.int32), (8, 16, torch.int64)])
def test_fallbacks_on_the_device(H, Fd, idtype):
    n = 400
    src, dst = hubby_graph(n, n, 40 * n, seed=Fd)
    g = make_graph(src, dst, n, n, DEV, idtype=idtype)
    q0, k0, v0, up0 = operands(n, n, H, Fd, 8)
    ins = [t.to(DEV).requires_grad_(True) for t in (q0, k0, v0)]
    assert not ops.dot_attention_fused(g, *ins)
    ref = Restated(src, dst, n, n, q0, k0, v0, Fd ** -0.5, up0)
    out = ops.dot_attention(g, *ins)
    check_forward(out, ref)
    assert torch.all(out[:5] == 0)
    (out * up0.to(DEV)).sum().backward()
    check_grads([t.grad for t in ins], ref)


def _cora_sized():
    from mi355x_graph.datasets import synthetic_edges
    n = 2708
    src, dst = synthetic_edges(n, 10556, 200, seed=5, symmetric=True)
    g = mg.graph((src, dst), num_nodes=n).add_self_loop().int().formats(["csr", "csc"]).to(DEV)
    gen = torch.Generator().manual_seed(0)
    x = torch.rand(n, 24, generator=gen).to(DEV)
    y = torch.randint(0, 7, (n,), generator=gen).to(DEV)
    idx = torch.nonzero(torch.rand(n, generator=gen) < 0.3).flatten().to(DEV)
    return g, x, y, idx


def _one_step(model, x, y, idx):
    model.zero_grad(set_to_none=True)
    loss = F.cross_entropy(model(x)[idx], y[idx])
    loss.backward()
    return float(loss.detach()), [(n_, p.grad.clone()) for n_, p in model.named_parameters()]


@pytest.mark.gpu
def test_dot_gat_model_with_the_fused_path_on_and_off(monkeypatch):
    sys.path.insert(0, PKG)
    import full_graph
    g, x, y, idx = _cora_sized()
    torch.manual_seed(3)
    model = full_graph.DotGAT(g, 3, 24, 8, 8, [8, 8, 1], feat_drop=0.0).to(DEV)
    model.train()
    assert all(isinstance(layer, mg.nn.DotGatConv) for layer in model.gat_layers)
    with torch.no_grad():
        h = model.gat_layers[0].fc(x).view(-1, 8, 8)
    assert ops.dot_attention_fused(g, h, h, h)
    twin = full_graph.DotGAT(g, 3, 24, 8, 8, [8, 8, 1], feat_drop=0.0).to(DEV)   # for the capture below: its parameters are never
    twin.load_state_dict(model.state_dict())                                     # used on the default stream
    twin.train()
    loss_on, grads_on = _one_step(model, x, y, idx)
    assert last_kernel() == "dot_attn_fwd"                             # the output layer's forward, on this thread
    monkeypatch.setattr(config, "DOT_ATTENTION_FUSED", False)
    assert not ops.dot_attention_fused(g, h, h, h)
    loss_off, grads_off = _one_step(model, x, y, idx)
    monkeypatch.setattr(config, "DOT_ATTENTION_FUSED", True)
    print("loss fused %r, composed %r" % (loss_on, loss_off))
    assert abs(loss_on - loss_off) <= 1e-5 * abs(loss_off)
    for (name, a_), (_, b_) in zip(grads_on, grads_off):
        err, top = float((a_ - b_).abs().max()), float(b_.abs().max())
        print("%s: max err %.3e, max |composed| %.3e" % (name, err, top))
        assert err <= 1e-4 * top, (name, err, top)
    # the same step captured in a HIP graph: the fused path reads nothing back to the host, and the replay equals the model's own
    # eager step bit for bit (same kernels, same order, same data, no atomics).  The captured model is a fresh copy, warmed up and
    # captured on ONE side stream (as utils.GraphedStep does): autograd binds a parameter's gradient accumulator to the stream it
    # first ran on, and the steps above ran on the default stream, which must not be touched during a capture.
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), ops.warming_up_for_capture():
        for _ in range(2):
            twin.zero_grad(set_to_none=True)
            eager_loss = F.cross_entropy(twin(x)[idx], y[idx])
            eager_loss.backward()
        eager_loss = eager_loss.detach().clone()
        eager_grads = [p.grad.clone() for p in twin.parameters()]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    twin.zero_grad(set_to_none=True)
    with torch.cuda.graph(graph, stream=side):
        loss = F.cross_entropy(twin(x)[idx], y[idx])
        loss.backward()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss.detach(), eager_loss)
    for (name, p), e_ in zip(twin.named_parameters(), eager_grads):
        assert torch.equal(p.grad, e_), name
    assert float(eager_loss) == loss_on                                # and the copy computes what the original computed
