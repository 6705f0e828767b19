"""Multi-relation g-SpMM (csrc/spmm_rel.hip), ops.rel_gspmm, nn.RelGraphConv and full_graph.RGCN.

  CPU   the fallback of ops.rel_gspmm and the layer (checker backend) against a per-relation loop through gspmm written from the
        formula  out[v, r, :] = sum | mean_{e: u -> v} w[e, r] x[u, :];  h = sum_r out[:, r, :] W_r + skip(x);  the C ABI's argument checks
  GPU   mgx_spmm_rel / mgx_spmm_rel_grad against R passes of the CPU oracle (u_mul_e): per element |hip - oracle| <= 1e-4 * SUM|terms|
        (BASELINE north_star, as tests/test_spmm_slots.py applies it), plain 1e-4 relative on non-negative operands, bitwise equal reruns,
        the kernel that ran; the module and the model against the loop restatement on the GPU; one full-size (79.1 M edges) pass."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import mi355x_graph as mg
import mi355x_graph.nn  # noqa: F401
from mi355x_graph import _lib, ops, sparse
from conftest import random_graph
import oracle_backend

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dgl-0.5-benchmark_amd")
DEV = "cuda:0"


# ----------------------------------------------------------------------------- the restatement: one gspmm and one matmul per relation
def loop_rel_gspmm(g, x, w, reduce):
    return torch.stack([ops.gspmm(g, "mul", reduce, x, w[:, r:r + 1].contiguous()) for r in range(w.shape[1])], 1)


class LoopRelLayer(torch.nn.Module):
    """h = act(sum_r mean_{e: u -> v}(w[e, r] x_u) W_r + skip(x_v)) with the parameters of nn.RelGraphConv, one pass per relation."""

    def __init__(self, in_feats, out_feats, num_relations, activation=None, dropout=0.):
        super(LoopRelLayer, self).__init__()
        self._rel_fcs = torch.nn.ParameterList([torch.nn.Parameter(torch.empty(in_feats, out_feats)) for _ in range(num_relations)])
        self._skip = torch.nn.Linear(in_feats, out_feats, bias=True)
        self._activation = activation

    def reset_parameters(self):
        pass

    def forward(self, g, x, edge_weights):
        w = edge_weights if torch.is_tensor(edge_weights) else torch.cat(list(edge_weights), 1)
        total = None
        for r in range(w.shape[1]):
            part = torch.matmul(ops.gspmm(g, "mul", "mean", x, w[:, r:r + 1].contiguous()), self._rel_fcs[r])
            total = part if total is None else total + part
        h = total + self._skip(x[:total.shape[0]])
        return self._activation(h) if self._activation else h


def _paired_layers(in_feats, out_feats, R, device, activation=None):
    torch.manual_seed(11)
    new = mg.nn.RelGraphConv(in_feats, out_feats, R, activation=activation).to(device)
    ref = LoopRelLayer(in_feats, out_feats, R, activation=activation).to(device)
    ref.load_state_dict(new.state_dict())          # same names and shapes: the state_dict moves across
    return new, ref


def _compare_layers(new, ref, g, x0, weights_new, weights_ref, loss_tol, grad_tol):
    upstream = torch.randn(g.num_dst_nodes(), new._out_feats, generator=torch.Generator().manual_seed(5)).to(x0.device)
    res = []
    for layer, wts in ((new, weights_new), (ref, weights_ref)):
        x = x0.clone().requires_grad_(True)
        layer.zero_grad()
        loss = (layer(g, x, wts) * upstream).sum() / upstream.numel()
        loss.backward()
        res.append((float(loss.detach()), [("node_feats", x.grad)] + [(n, p.grad) for n, p in layer.named_parameters()]))
    (la, ga), (lb, gb) = res
    print("loss %r vs %r" % (la, lb))
    assert abs(la - lb) <= loss_tol * abs(lb)
    assert [n for n, _ in ga] == [n for n, _ in gb]
    for (name, a), (_, b) in zip(ga, gb):
        err, top = float((a - b).abs().max()), float(b.abs().max())
        print("%s: max err %.3e, max |reference| %.3e" % (name, err, top))
        assert err <= grad_tol * top, (name, err, top)


# ----------------------------------------------------------------------------- CPU: checker backend
@pytest.fixture
def checker():
    oracle_backend.install()
    yield
    oracle_backend.uninstall()


@pytest.mark.parametrize("reduce", ["sum", "mean"])
@pytest.mark.parametrize("n_src,n_dst", [(60, 60), (90, 40)])
def test_rel_gspmm_fallback_equals_the_per_relation_loop(checker, reduce, n_src, n_dst):
    src, dst = random_graph(n_src, n_dst, 700, seed=n_src + len(reduce))     # isolated destinations, duplicate edges
    assert len(set(zip(src.tolist(), dst.tolist()))) < 700 and np.bincount(dst, minlength=n_dst).min() == 0
    if n_src == n_dst:
        g = mg.graph((torch.from_numpy(src), torch.from_numpy(dst)), num_nodes=n_src).int()
    else:
        g = mg.create_block((torch.from_numpy(src), torch.from_numpy(dst)), n_src, n_dst, idtype=torch.int32)
    gen = torch.Generator().manual_seed(1)
    for R, D in ((1, 1), (3, 4), (8, 32)):
        x = torch.randn(n_src, D, generator=gen).requires_grad_(True)
        w = torch.randn(700, R, generator=gen)
        out = ops.rel_gspmm(g, x, w, reduce)
        assert tuple(out.shape) == (n_dst, R, D)
        want = loop_rel_gspmm(g, x, w, reduce)
        assert torch.allclose(out, want, rtol=1e-5, atol=1e-6)
        up = torch.randn(n_dst, R, D, generator=gen)
        gx, = torch.autograd.grad((out * up).sum(), x)
        gx_want, = torch.autograd.grad((want * up).sum(), x)
        assert torch.allclose(gx, gx_want, rtol=1e-5, atol=1e-5)
    with pytest.raises(mg.DGLError):
        ops.rel_gspmm(g, torch.randn(n_src, 4), torch.randn(700, 2), "max")


def test_rel_gspmm_weight_gradient_through_the_fallback(checker):
    src, dst = random_graph(50, 50, 400, seed=3)
    g = mg.graph((torch.from_numpy(src), torch.from_numpy(dst)), num_nodes=50).int()
    gen = torch.Generator().manual_seed(2)
    x, up = torch.randn(50, 4, generator=gen), torch.randn(50, 3, 4, generator=gen)
    w = torch.randn(400, 3, generator=gen).requires_grad_(True)
    gw, = torch.autograd.grad((ops.rel_gspmm(g, x, w, "mean") * up).sum(), w)
    gw_want, = torch.autograd.grad((loop_rel_gspmm(g, x, w, "mean") * up).sum(), w)
    assert torch.allclose(gw, gw_want, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("as_list", [False, True])
def test_rel_graph_conv_equals_the_restatement_on_the_checker(checker, as_list):
    n, E, R = 80, 900, 4
    src, dst = random_graph(n, n, E, seed=7)
    g = mg.graph((torch.from_numpy(src), torch.from_numpy(dst)), num_nodes=n).int()
    new, ref = _paired_layers(6, 5, R, "cpu", activation=torch.relu)
    assert sorted(new.state_dict()) == sorted(["_rel_fcs.%d" % r for r in range(R)] + ["_skip.weight", "_skip.bias"])
    gen = torch.Generator().manual_seed(4)
    w = torch.rand(E, R, generator=gen)
    x0 = torch.randn(n, 6, generator=gen)
    wts = [w[:, r:r + 1] for r in range(R)] if as_list else w
    _compare_layers(new, ref, g, x0, wts, w, 1e-5, 1e-4)
    import dgl.nn.pytorch as dglnn
    assert dglnn.RelGraphConv is mg.nn.RelGraphConv and dglnn.conv.RelGraphConv is mg.nn.RelGraphConv


def test_list_of_views_is_recognised_and_other_lists_are_cached(checker):
    g = mg.graph((torch.tensor([0, 1, 2]), torch.tensor([1, 2, 0])), num_nodes=3).int()
    feat = torch.rand(3, 8)
    m = ops.rel_weight_matrix(g, [feat[:, t:t + 1] for t in range(8)])
    assert m.data_ptr() == feat.data_ptr() and tuple(m.shape) == (3, 8) and torch.equal(m, feat)
    feat.add_(1.0)
    assert m._version == feat._version                                 # a view: the edit is seen through the version counter
    cols = [torch.rand(3, 1) for _ in range(4)]
    a = ops.rel_weight_matrix(g, cols)
    assert ops.rel_weight_matrix(g, cols) is a and torch.equal(a, torch.cat(cols, 1))
    cols[2].mul_(2.0)
    b = ops.rel_weight_matrix(g, cols)
    assert b is not a and torch.equal(b, torch.cat(cols, 1))
    sub = ops.rel_weight_matrix(g, [feat[:, 2:3], feat[:, 3:4]])      # a column range of the matrix is a view too
    assert sub.data_ptr() == feat[:, 2:].data_ptr() and torch.equal(sub, feat[:, 2:4])


# ----------------------------------------------------------------------------- CPU: the C ABI
def test_abi_exports_and_argument_checks():
    L = _lib.lib()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("mgx_spmm_rel", "mgx_spmm_rel_grad"):
        assert hasattr(handle, name) and name in _lib.SIGNATURES
    assert L.mgx_abi_version() == 35
    st = L.mgx_spmm_rel(None, None, 0, 8, 32, None, None, 32, None, None, None, None, None)
    assert st == 1 and b"csr is NULL" in L.mgx_last_error()
    with pytest.raises(mg.DGLError):
        _lib.check(st)
    st = L.mgx_spmm_rel_grad(None, None, 8, 32, None, None, None, None, None, None, None)
    assert st == 1 and b"csr is NULL" in L.mgx_last_error()
    c = _lib.MgxCsr(1, 1, 0, None, None, None, 16, 0)                   # idx_bits 16
    assert L.mgx_spmm_rel(ctypes.byref(c), None, 0, 8, 32, None, None, 32, None, None, None, None, None) == 1
    c = _lib.MgxCsr(1, 1, 0, None, None, None, 32, 0)                   # indptr NULL
    assert L.mgx_spmm_rel(ctypes.byref(c), None, 0, 8, 32, None, None, 32, None, None, None, None, None) == 1
    c = _lib.MgxCsr(0, 0, 0, None, None, None, 32, 0)
    assert L.mgx_spmm_rel(ctypes.byref(c), None, 1, 8, 32, None, None, 32, None, None, None, None, None) == 1   # MAX
    assert L.mgx_spmm_rel(ctypes.byref(c), None, 0, 0, 32, None, None, 32, None, None, None, None, None) == 1   # R = 0
    assert L.mgx_spmm_rel(ctypes.byref(c), None, 0, 8, 32, None, None, 16, None, None, None, None, None) == 1   # stride below D
    for R, D in ((17, 32), (8, 256), (8, 24), (8, 3)):                  # outside the kernels' range: the caller's fallback
        assert L.mgx_spmm_rel(ctypes.byref(c), None, 0, R, D, None, None, D, None, None, None, None, None) == _lib.ERR_UNSUPPORTED
        assert b"mgx_spmm_rel" in L.mgx_last_error()
        assert L.mgx_spmm_rel_grad(ctypes.byref(c), None, R, D, None, None, None, None, None, None, None) == _lib.ERR_UNSUPPORTED
    assert L.mgx_spmm_rel(ctypes.byref(c), None, 0, 8, 32, None, None, 32, None, None, None, None, None) == 0   # no rows: nothing to do
    assert L.mgx_spmm_rel_grad(ctypes.byref(c), None, 8, 32, None, None, None, None, None, None, None) == 0


# ----------------------------------------------------------------------------- GPU: kernels against the oracle
def _hub_graph(n_src, n_dst, seed):
    """Skewed multigraph in a shuffled (not destination-sorted) edge order: one row far beyond the split threshold (256), one just
    above it, empty rows."""
    src, dst = random_graph(n_src, n_dst, 30 * n_dst, seed=seed)
    rng = np.random.default_rng(seed + 1)
    hub = np.concatenate([np.full(1500, 5), np.full(300, n_dst - 3)])
    src = np.concatenate([src, rng.integers(0, n_src, hub.shape[0]), np.full(700, 7)])     # source 7: a split row of the reverse walk
    dst = np.concatenate([dst, hub, rng.integers(0, n_dst, 700)])
    perm = rng.permutation(dst.shape[0])
    src, dst = src[perm], dst[perm]
    assert np.bincount(dst, minlength=n_dst).min() == 0 and bool((np.diff(dst) < 0).any())
    return src, dst


def _device_graph(src, dst, n_src, n_dst, idtype):
    s, d = torch.from_numpy(src), torch.from_numpy(dst)
    if n_src == n_dst:
        g = mg.graph((s, d), num_nodes=n_src)
        g = g.int() if idtype == torch.int32 else g.long()
        return g.to(DEV)
    return mg.create_block((s, d), n_src, n_dst, idtype=idtype, device=DEV)


def _oracle_forward(oracle, csc, X, W, reduce):
    ip, ix, ei = csc
    return np.stack([oracle.spmm(ip, ix, ei, "mul", reduce, X, np.ascontiguousarray(W[:, r:r + 1])) for r in range(W.shape[1])], 1)


def _oracle_reverse(oracle, csr, dZ, W):
    """dX[u] = sum_r sum_{e: u -> v} W[e, r] dZ[v, r, :]; returns the R terms separately."""
    rp, rx, re = csr
    return [oracle.spmm(rp, rx, re, "mul", "sum", np.ascontiguousarray(dZ[:, r, :]), np.ascontiguousarray(W[:, r:r + 1]))
            for r in range(W.shape[1])]


@pytest.mark.gpu
@pytest.mark.parametrize("D", [1, 4, 32, 64, 128])
@pytest.mark.parametrize("R", [1, 3, 8, 16])
def test_rel_kernels_against_the_oracle(oracle, R, D):
    L = _lib.lib()
    worst = {}
    for n_src, n_dst in ((3000, 3000), (4100, 1700)):
        src, dst = _hub_graph(n_src, n_dst, seed=R * 131 + D)
        E = src.shape[0]
        rng = np.random.default_rng(R + 7 * D)
        csc = oracle.coo_to_csr(n_dst, dst, src)
        csr = oracle.coo_to_csr(n_src, src, dst)
        deg = np.maximum(np.diff(csc[0]), 1).astype(np.float32)
        for signed in (True, False):
            X = (rng.standard_normal((n_src, D)) if signed else rng.random((n_src, D))).astype(np.float32)
            W = (rng.standard_normal((E, R)) if signed else rng.random((E, R))).astype(np.float32)
            dZ = (rng.standard_normal((n_dst, R, D)) if signed else rng.random((n_dst, R, D))).astype(np.float32)
            ref = {red: _oracle_forward(oracle, csc, X, W, red) for red in ("sum", "mean")}
            mag = _oracle_forward(oracle, csc, np.abs(X), np.abs(W), "sum")
            for idtype in (torch.int32, torch.int64):
                g = _device_graph(src, dst, n_src, n_dst, idtype)
                assert g._index.csc().indptr.dtype == idtype
                x = torch.from_numpy(X).to(DEV).requires_grad_(True)
                w = torch.from_numpy(W).to(DEV)
                for red in ("sum", "mean"):
                    assert ops.rel_gspmm_fused(g, x, w)
                    out = ops.rel_gspmm(g, x, w, red)
                    assert L.mgx_last_spmm_kernel().decode() == "rel"                       # the new kernel, not the broadcast path
                    plan = g._index.csc().plan()
                    assert plan is not None and plan.num_slots >= 8                          # the hub rows were split
                    got = out.detach().cpu().numpy()
                    scale = mag / deg[:, None, None] if red == "mean" else mag
                    err = np.abs(got - ref[red])
                    worst[("fwd", red)] = max(worst.get(("fwd", red), 0.0), float((err / (scale + 1e-30)).max()))
                    assert bool((err <= 1e-4 * scale + 1e-30).all()), ("fwd", red, idtype, signed)
                    if not signed:                                                         # non-negative pair: plain relative error
                        assert bool((err <= 1e-4 * np.abs(ref[red])).all()), ("fwd rel", red, idtype)
                    assert bool((got[np.diff(csc[0]) == 0] == 0).all())                     # empty rows give 0
                    again = ops.rel_gspmm(g, x, w, red)
                    assert torch.equal(out, again)                                         # bitwise equal reruns
                    # reverse: gradient with respect to x over the out-CSR
                    dz = torch.from_numpy(dZ).to(DEV)
                    gx, = torch.autograd.grad(out, x, dz, retain_graph=True)
                    dZs = dZ / deg[:, None, None] if red == "mean" else dZ
                    terms = _oracle_reverse(oracle, csr, dZs.astype(np.float32), W)
                    want = np.sum(np.stack(terms, 0).astype(np.float64), 0)
                    rmag = np.sum(np.stack(_oracle_reverse(oracle, csr, np.abs(dZs).astype(np.float32), np.abs(W)), 0).astype(np.float64), 0)
                    gerr = np.abs(gx.cpu().numpy() - want)
                    worst[("bwd", red)] = max(worst.get(("bwd", red), 0.0), float((gerr / (rmag + 1e-30)).max()))
                    assert bool((gerr <= 1e-4 * rmag + 1e-30).all()), ("bwd", red, idtype, signed)
                    if not signed:
                        assert bool((gerr <= 1e-4 * np.abs(want)).all()), ("bwd rel", red, idtype)
                    gx2, = torch.autograd.grad(out, x, dz)
                    assert torch.equal(gx, gx2)
    print("R %d D %d worst error / bound terms: %r" % (R, D, worst))


@pytest.mark.gpu
def test_rel_kernel_entry_points_directly(oracle):
    """The C entry points with their optional arguments: no plan (natural rows), src_scale / dst_scale, a row-strided x, and what they
    refuse."""
    L = _lib.lib()
    n_src, n_dst, R, D = 900, 700, 5, 8
    src, dst = random_graph(n_src, n_dst, 9000, seed=21)
    E = src.shape[0]
    rng = np.random.default_rng(3)
    X, W = rng.standard_normal((n_src, D)).astype(np.float32), rng.standard_normal((E, R)).astype(np.float32)
    ss, ds = (rng.random(n_src) + 0.5).astype(np.float32), (rng.random(n_dst) + 0.5).astype(np.float32)
    g = mg.create_block((torch.from_numpy(src), torch.from_numpy(dst)), n_src, n_dst, idtype=torch.int32, device=DEV)
    csc = g._index.csc()
    be = sparse.backend_for(csc.indptr)
    wide = torch.zeros(n_src, 3 * D, device=DEV)
    wide[:, D:2 * D] = torch.from_numpy(X).to(DEV)
    x = wide[:, D:2 * D]
    w_pos = be.gather_rows(torch.from_numpy(W).to(DEV), csc.eids)
    out = torch.full((n_dst, R, D), float("nan"), device=DEV)
    st = L.mgx_spmm_rel(ctypes.byref(csc.c_struct()), None, sparse.REDUCE["mean"], R, D, sparse._ptr(w_pos), sparse._ptr(x), int(x.stride(0)),
                        sparse._ptr(torch.from_numpy(ss).to(DEV)), sparse._ptr(torch.from_numpy(ds).to(DEV)), sparse._ptr(out), None, None)
    torch.cuda.synchronize()
    assert st == 0, L.mgx_last_error()
    ip = oracle.coo_to_csr(n_dst, dst, src)
    Xs = X * ss[:, None]
    ref = _oracle_forward(oracle, ip, Xs, W, "mean") * ds[:, None, None]
    mag = _oracle_forward(oracle, ip, np.abs(Xs), np.abs(W), "mean") * ds[:, None, None]
    assert bool((np.abs(out.cpu().numpy() - ref) <= 1e-4 * mag + 1e-30).all())
    # x at an address that is not 16-byte aligned; a two-part plan
    odd = torch.zeros(n_src * D + 1, device=DEV)[1:].view(n_src, D)
    assert L.mgx_spmm_rel(ctypes.byref(csc.c_struct()), None, 0, R, D, sparse._ptr(w_pos), sparse._ptr(odd), D, None, None, sparse._ptr(out),
                          None, None) == _lib.ERR_UNSUPPORTED
    assert not ops.rel_gspmm_fused(g, odd, torch.from_numpy(W).to(DEV))
    assert not ops.rel_gspmm_fused(g, x, torch.from_numpy(W).to(DEV).requires_grad_(True))
    assert not ops.rel_gspmm_fused(g, torch.zeros(n_src, 24, device=DEV), torch.from_numpy(W).to(DEV))
    fallback = ops.rel_gspmm(g, torch.from_numpy(X).to(DEV)[:, :6].contiguous(), torch.from_numpy(W).to(DEV), "sum")   # D = 6: broadcast path
    assert L.mgx_last_spmm_kernel().decode() not in ("rel", "rel_grad")
    want = _oracle_forward(oracle, ip, np.ascontiguousarray(X[:, :6]), W, "sum")
    assert bool((np.abs(fallback.cpu().numpy() - want) <= 1e-4 * _oracle_forward(oracle, ip, np.abs(X[:, :6]), np.abs(W), "sum") + 1e-30).all())


# ----------------------------------------------------------------------------- GPU: module and model
@pytest.mark.gpu
@pytest.mark.parametrize("as_list", [False, True])
def test_rel_graph_conv_on_the_gpu_against_the_loop(as_list):
    n, R = 6000, 8
    src, dst = _hub_graph(n, n, seed=77)
    g = mg.graph((torch.from_numpy(src), torch.from_numpy(dst)), num_nodes=n).int().formats(["csr", "csc"]).to(DEV)
    E = src.shape[0]
    new, ref = _paired_layers(32, 16, R, DEV, activation=torch.relu)
    gen = torch.Generator().manual_seed(9)
    w = torch.rand(E, R, generator=gen).to(DEV)
    x0 = torch.randn(n, 32, generator=gen).to(DEV)
    wts = [w[:, r:r + 1] for r in range(R)] if as_list else w
    seen = []
    orig = sparse.HipBackend.spmm_rel
    try:
        sparse.HipBackend.spmm_rel = lambda self, *a, **k: (seen.append(1), orig(self, *a, **k))[1]
        _compare_layers(new, ref, g, x0, wts, w, 1e-5, 1e-4)
    finally:
        sparse.HipBackend.spmm_rel = orig
    assert seen == [1]                                                                      # one fused pass, not the fallback
    if as_list:
        assert ops.rel_weight_matrix(g, wts).data_ptr() == w.data_ptr()


@pytest.mark.gpu
def test_cached_permutation_is_not_served_stale():
    n, R, D = 2000, 4, 16
    src, dst = random_graph(n, n, 40000, seed=13)
    g = mg.graph((torch.from_numpy(src), torch.from_numpy(dst)), num_nodes=n).int().to(DEV)
    gen = torch.Generator().manual_seed(1)
    w = torch.rand(40000, R, generator=gen).to(DEV)
    x = torch.randn(n, D, generator=gen).to(DEV).requires_grad_(True)
    cache = ops.rel_weight_cache_for(g)
    first = ops.rel_gspmm(g, x, w, "sum")
    assert cache.holds(g._index, w, "in") and not cache.holds(g._index, w, "out")
    held = cache.get(g._index, w, "in")
    first.sum().backward()
    assert cache.holds(g._index, w, "out") and cache.get(g._index, w, "in") is held           # a hit: the same permuted tensor
    w.mul_(2.0)                                                                              # in place: same address, new version
    assert not cache.holds(g._index, w, "in")
    second = ops.rel_gspmm(g, x, w, "sum")
    assert torch.allclose(second, 2.0 * first, rtol=1e-6, atol=0) and cache.get(g._index, w, "in") is not held
    out = ops.rel_gspmm(g, x, w, "sum")
    w.add_(1.0)                                                                              # between forward and backward: autograd refuses
    with pytest.raises(RuntimeError):
        out.sum().backward()
    other = mg.graph((torch.from_numpy(dst), torch.from_numpy(src)), num_nodes=n).int().to(DEV)
    assert not ops.rel_weight_cache_for(other).holds(other._index, w, "in")                  # caches belong to one graph
    nocache = ops.rel_gspmm(g, x, w, "sum", cache=False)
    assert torch.equal(nocache, ops.rel_gspmm(g, x, w, "sum"))


@pytest.mark.gpu
def test_rgcn_step_decreases_the_loss_on_a_small_proteins_stand_in():
    sys.path.insert(0, PKG)
    import full_graph
    torch.manual_seed(0)
    data, g, node_feats, edge_weights, model, opt = full_graph.build_rgcn(torch.device(DEV), scale=0.01)
    assert len(edge_weights) == 8 and tuple(edge_weights[0].shape) == (g.number_of_edges(), 1)
    model.reset_parameters()
    losses = [full_graph.rgcn_train_step(model, g, node_feats, edge_weights, data.y_true, data.train_idx, opt) for _ in range(5)]
    print("losses", losses)
    assert _lib.lib().mgx_last_spmm_kernel().decode() in ("rel", "rel_grad")
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    # the same model from loop layers, same parameters: same first-step loss
    torch.manual_seed(0)
    loop = full_graph.RGCN(3, 1, 32, data.num_tasks, 8, layer=LoopRelLayer).to(DEV)
    fused = full_graph.RGCN(3, 1, 32, data.num_tasks, 8).to(DEV)
    loop.load_state_dict(fused.state_dict())
    y = data.y_true[data.train_idx].float()
    la = torch.nn.functional.binary_cross_entropy_with_logits(fused(g, node_feats, edge_weights)[data.train_idx], y)
    lb = torch.nn.functional.binary_cross_entropy_with_logits(loop(g, node_feats, edge_weights)[data.train_idx], y)
    assert abs(float(la.detach()) - float(lb.detach())) <= 1e-5 * abs(float(lb.detach()))


# ----------------------------------------------------------------------------- GPU: full size
@pytest.mark.gpu
def test_full_size_proteins_shape_against_the_oracle(oracle):
    """79.1 M edges, R = 8, D = 32: every output row against the oracle's 8 passes (W is 2.53 GB: offsets into it pass 2^31 elements'
    worth of bytes well before the last row)."""
    from mi355x_graph.datasets import SHAPES, synthetic_edges
    spec = SHAPES["proteins"]
    n, R, D = spec["n"], 8, 32
    src, dst = synthetic_edges(n, spec["m"], spec["max_deg"], spec["seed"], DEV, symmetric=True)
    E = int(src.shape[0])
    assert E == 79122504 and E * R * 4 > 2 ** 31
    g = mg.graph((src, dst), num_nodes=n).int().to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(5)
    x = torch.rand(n, D, device=DEV, generator=gen)
    w = torch.rand(E, R, device=DEV, generator=gen)
    out = ops.rel_gspmm(g, x, w, "mean")
    assert _lib.lib().mgx_last_spmm_kernel().decode() == "rel"
    got = out.cpu().numpy()
    csc = g._index.csc()
    ip, ix, ei = csc.indptr.cpu().numpy(), csc.indices.cpu().numpy(), csc.eids.cpu().numpy()
    X, W = x.cpu().numpy(), w.cpu().numpy()
    worst = 0.0
    for r in range(R):
        ref = oracle.spmm(ip, ix, ei, "mul", "mean", X, np.ascontiguousarray(W[:, r:r + 1]))
        err = np.abs(got[:, r, :] - ref)
        worst = max(worst, float((err / (np.abs(ref) + 1e-30)).max()))
        assert bool((err <= 1e-4 * np.abs(ref) + 1e-30).all()), r            # non-negative operands: SUM|terms| = the sum itself
    print("full size: worst relative error %.3e" % worst)
    assert torch.equal(out, ops.rel_gspmm(g, x, w, "mean"))
