"""Graph readout: csrc/segattn.hip (mgx_segment_softmax_*, mgx_segment_attention_*), ops.segment_softmax / segment_attention, readout.py
(sum_nodes ... broadcast_edges), nn.GlobalAttentionPooling / Set2Set / WeightAndSum, graph_classification.py --readout.

The reference everywhere is the fp64 restatement below, written from the definitions with a plain Python loop over the segments, on the fp32
inputs:

    z[i,h] = logits[i,h]  |  scale * sum_f feat[i,h,f] query[g,h,f];   a = exp(z - m[g]) / s[g];   out[g,h,:] = sum_{i in g} a[i,h] feat[i,h,:]
    t = <out, dout>;  dp[i,h] = <feat[i,h,:], dout[g,h,:]>;  dz = a (dp - t);  d logits = dz;  d feat[i] = a dout[g] (+ dz scale query[g]);
    d query[g] = scale sum_i dz feat[i];       softmax: out = exp(x - m) / s per column, d x = out (d out - sum_j out d out)

  CPU   the composition behind the operators (checker backend and the OpenMP backend), the readout functions, the layers, argument errors,
        the C ABI's argument checks: rtol 1e-5, atol 1e-6
  GPU   the fused kernels: forward per element |got - ref| <= 1e-4 * sum_i a |feat|, gradients 1e-4 * the reference gradient tensor's max
        (the bounds of tests/test_dot_attention.py); the softmax per element 1e-4 * the reference value (the same bound with feat = 1, hence
        column sums within 1e-4 of 1); bitwise: reruns, strided operands, exact-arithmetic means, untouched segments next to a NaN."""
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
RTOL = 1e-4
INF = float("inf")


# ----------------------------------------------------------------------------- the restatement (fp64, a loop over segments, never the code under test)
class Restated(object):
    def __init__(self, lens, feat, logits=None, query=None, scale=1.0, dout=None):
        assert (logits is None) != (query is None)
        feat = feat.detach().cpu().double()
        N, H, Fd = feat.shape
        S = len(lens)
        gate = logits is not None
        other = (logits if gate else query).detach().cpu().double()
        dout = None if dout is None else dout.detach().cpu().double()
        self.out = torch.zeros(S, H, Fd, dtype=torch.float64)
        self.row_scale = torch.zeros(S, H, Fd, dtype=torch.float64)
        self.a = torch.zeros(N, H, dtype=torch.float64)
        self.d_feat = torch.zeros(N, H, Fd, dtype=torch.float64)
        self.d_logits = torch.zeros(N, H, dtype=torch.float64)
        self.d_query = torch.zeros(S, H, Fd, dtype=torch.float64)
        o = 0
        for g, n in enumerate(int(v) for v in lens):
            x = feat[o:o + n]
            if n:
                z = other[o:o + n] if gate else scale * (x * other[g]).sum(-1)            # [n, H]
                m = z.max(0).values
                e = torch.exp(z - torch.where(m == -INF, torch.zeros_like(m), m))         # only -inf logits: weights 0
                s = e.sum(0)
                a = e / torch.where(s == 0, torch.ones_like(s), s)
                self.a[o:o + n] = a
                self.out[g] = (a.unsqueeze(-1) * x).sum(0)
                self.row_scale[g] = (a.unsqueeze(-1) * x.abs()).sum(0)
                if dout is not None:
                    t = (self.out[g] * dout[g]).sum(-1)                                   # [H]
                    dp = (x * dout[g]).sum(-1)                                            # [n, H]
                    dz = a * (dp - t)
                    self.d_feat[o:o + n] = a.unsqueeze(-1) * dout[g]
                    if gate:
                        self.d_logits[o:o + n] = dz
                    else:
                        self.d_feat[o:o + n] += dz.unsqueeze(-1) * scale * other[g]
                        self.d_query[g] = scale * (dz.unsqueeze(-1) * x).sum(0)
            o += n
        assert o == N


def restated_softmax(lens, x, dy=None):
    x = x.detach().cpu().double()
    out, dx = torch.zeros_like(x), torch.zeros_like(x)
    o = 0
    for n in (int(v) for v in lens):
        if n:
            z = x[o:o + n]
            e = torch.exp(z - z.max(0).values)
            out[o:o + n] = e / e.sum(0)
            if dy is not None:
                d = dy.detach().cpu().double()[o:o + n]
                dx[o:o + n] = out[o:o + n] * (d - (out[o:o + n] * d).sum(0))
        o += n
    return out, dx


LENS = [0, 1, 2, 3, 15, 16, 17, 63, 64, 65, 0, 257, 1000]      # zeros first and inside; below, at and above one wave step; a long walk
LENS_ZERO_LAST = LENS[1:] + [0]
WIDTHS = [(1, 4), (1, 20), (3, 4), (4, 16), (1, 64), (1, 256)]  # one lane per row; 5 lanes of 8; 3 heads of one lane; 16 .. 1 rows per step


@functools.lru_cache(maxsize=None)
def case(lens_key, H, Fd, mode, seed=0, scale=0.37):
    """Signed normal operands and their restatement, computed once and shared (never modified)."""
    lens = list(lens_key)
    N, S = sum(lens), len(lens)
    gen = torch.Generator().manual_seed(1000 * H + Fd + seed)
    feat = torch.randn(N, H, Fd, generator=gen)
    logits = torch.randn(N, H, generator=gen) * 3 if mode == "gate" else None
    query = torch.randn(S, H, Fd, generator=gen) * (2.0 / Fd ** 0.5) if mode == "query" else None
    up = torch.randn(S, H, Fd, generator=gen)
    ref = Restated(lens, feat, logits, query, scale, up)
    return torch.tensor(lens), feat, logits, query, up, ref


def run(seglen, feat, logits, query, scale, up, device):
    """forward + backward of ops.segment_attention on `device`: (out, {name: gradient})."""
    f = feat.to(device).requires_grad_(True)
    lg = None if logits is None else logits.to(device).requires_grad_(True)
    q = None if query is None else query.to(device).requires_grad_(True)
    out = ops.segment_attention(seglen.to(device), f, logits=lg, query=q, scale=scale, total=int(feat.shape[0]))
    leaves = [("d_feat", f)] + ([("d_logits", lg)] if lg is not None else [("d_query", q)])
    grads = torch.autograd.grad((out * up.to(device)).sum(), [t for _, t in leaves])
    return out.detach(), {name: g_ for (name, _), g_ in zip(leaves, grads)}


def check_forward(got, ref):
    err = (got.detach().cpu().double() - ref.out).abs()
    worst = float((err / (ref.row_scale + 1e-30)).max())
    print("forward: max err / sum_i a|feat| = %.3e" % worst)
    assert not (err > RTOL * ref.row_scale + 1e-30).any(), worst


def check_grads(grads, ref):
    for name, g_ in grads.items():
        want = getattr(ref, name)
        err, top = float((g_.detach().cpu().double() - want).abs().max()), float(want.abs().max())
        print("%s: max err %.3e, max |reference| %.3e" % (name, err, top))
        assert err <= RTOL * top, (name, err, top)


def launches(monkeypatch):
    """the list the backend's timed_call appends one record per C-ABI call to (sparse.PROFILE, bench.py's hook): [{"kernel": name, ...}]"""
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


CPU_LENS = (0, 1, 5, 0, 17, 1, 40)


@pytest.mark.parametrize("mode", ["gate", "query"])
def test_composition_and_its_gradients_match_the_restatement(cpu_backend_on, mode):
    for H, Fd in ((1, 1), (3, 4), (2, 5)):
        seglen, feat, logits, query, up, ref = case(CPU_LENS, H, Fd, mode)
        assert not ops.segment_attention_fused(seglen, feat, logits=logits, query=query)
        out, grads = run(seglen, feat, logits, query, 0.37, up, "cpu")
        assert tuple(out.shape) == (len(CPU_LENS), H, Fd)
        assert torch.allclose(out.double(), ref.out, rtol=1e-5, atol=1e-6)
        assert torch.all(out[torch.tensor(CPU_LENS) == 0] == 0)
        for name, got in grads.items():
            assert torch.allclose(got.double(), getattr(ref, name), rtol=1e-5, atol=1e-6), (name, H, Fd)
    # host lengths need no `total`; a segment of -inf logits only reads out 0 with zero gradients
    seglen, feat, logits, query, up, ref = case(CPU_LENS, 3, 4, "gate")
    assert torch.equal(ops.segment_attention(seglen, feat, logits=logits), run(seglen, feat, logits, None, 1.0, up, "cpu")[0])
    masked = logits.clone()
    masked[6:23] = -INF                                                                    # the segment of 17 rows
    out, grads = run(seglen, feat, masked, None, 1.0, up, "cpu")
    assert torch.all(out[4] == 0) and torch.all(grads["d_feat"][6:23] == 0) and torch.all(grads["d_logits"][6:23] == 0)
    assert torch.allclose(out.double(), Restated(CPU_LENS, feat, masked).out, rtol=1e-5, atol=1e-6)


def test_segment_softmax_matches_the_restatement(cpu_backend_on):
    gen = torch.Generator().manual_seed(5)
    seglen = torch.tensor(CPU_LENS)
    for shape in ((64,), (64, 1), (64, 3), (64, 2, 5)):
        x = (torch.randn(*shape, generator=gen) * 3).requires_grad_(True)
        dy = torch.randn(*shape, generator=gen)
        want, want_dx = restated_softmax(CPU_LENS, x.view(64, -1), dy.view(64, -1))
        out = ops.segment_softmax(seglen, x)
        assert out.shape == x.shape and torch.allclose(out.double().view(64, -1), want, rtol=1e-5, atol=1e-6)
        dx, = torch.autograd.grad((out * dy).sum(), x)
        assert torch.allclose(dx.double().view(64, -1), want_dx, rtol=1e-5, atol=1e-6)
    assert "segment_softmax" in ops.__all__ and "segment_attention" in ops.__all__ and "segment_attention_fused" in ops.__all__


def small_graphs(sizes, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for n in sizes:
        e = int(rng.integers(1, 3 * n + 1))
        out.append(mg.graph((torch.from_numpy(rng.integers(0, n, e)), torch.from_numpy(rng.integers(0, n, e))), num_nodes=n))
    return out


def test_readout_functions_on_a_batch_of_five_graphs(cpu_backend_on):
    import dgl
    graphs = small_graphs([3, 1, 7, 4, 9])
    bg = dgl.batch(graphs)
    nn_, ne_ = [g.number_of_nodes() for g in graphs], [g.number_of_edges() for g in graphs]
    gen = torch.Generator().manual_seed(2)
    h, w = torch.randn(sum(nn_), 6, generator=gen), torch.rand(sum(nn_), 1, generator=gen)
    eh, ew = torch.randn(sum(ne_), 3, generator=gen), torch.rand(sum(ne_), 1, generator=gen)
    bg.ndata["h"], bg.ndata["w"], bg.edata["h"], bg.edata["w"] = h, w, eh, ew
    parts, eparts, wparts, ewparts = h.split(nn_), eh.split(ne_), w.split(nn_), ew.split(ne_)

    def close(got, want):
        return got.shape == want.shape and torch.allclose(got, want, rtol=1e-5, atol=1e-6)

    assert close(dgl.sum_nodes(bg, "h"), torch.stack([p.sum(0) for p in parts]))
    assert close(dgl.sum_nodes(bg, "h", "w"), torch.stack([(p * q).sum(0) for p, q in zip(parts, wparts)]))
    assert close(dgl.mean_nodes(bg, "h"), torch.stack([p.mean(0) for p in parts]))
    assert close(dgl.max_nodes(bg, "h"), torch.stack([p.max(0).values for p in parts]))
    assert close(dgl.readout_nodes(bg, "h", op="mean"), dgl.mean_nodes(bg, "h"))
    assert close(dgl.softmax_nodes(bg, "h"), torch.cat([torch.softmax(p, 0) for p in parts]))
    gf = torch.randn(5, 4, generator=gen)
    assert torch.equal(dgl.broadcast_nodes(bg, gf), torch.cat([gf[i:i + 1].expand(n, 4) for i, n in enumerate(nn_)]))
    assert close(dgl.sum_edges(bg, "h", "w"), torch.stack([(p * q).sum(0) for p, q in zip(eparts, ewparts)]))
    assert close(dgl.mean_edges(bg, "h"), torch.stack([p.mean(0) for p in eparts]))
    assert close(dgl.max_edges(bg, "h"), torch.stack([p.max(0).values for p in eparts]))
    assert close(dgl.softmax_edges(bg, "h"), torch.cat([torch.softmax(p, 0) for p in eparts]))
    assert torch.equal(dgl.broadcast_edges(bg, gf), torch.cat([gf[i:i + 1].expand(n, 4) for i, n in enumerate(ne_)]))
    with pytest.raises(mg.DGLError, match="readout op"):
        dgl.readout_nodes(bg, "h", op="median")
    with pytest.raises(mg.DGLError, match="5 graphs"):
        dgl.broadcast_nodes(bg, gf[:4])
    # an unbatched graph is one segment
    g = graphs[2]
    g.ndata["h"] = parts[2]
    assert close(dgl.sum_nodes(g, "h"), parts[2].sum(0, keepdim=True)) and close(dgl.softmax_nodes(g, "h"), torch.softmax(parts[2], 0))
    assert torch.equal(dgl.broadcast_nodes(g, gf[:1]), gf[:1].expand(7, 4)) and torch.equal(dgl.broadcast_nodes(g, gf[0]), gf[:1].expand(7, 4))
    # gradients flow through broadcast (a segment sum) and softmax
    q = gf.clone().requires_grad_(True)
    dgl.broadcast_nodes(bg, q).sum().backward()
    assert torch.equal(q.grad, torch.tensor(nn_, dtype=torch.float32).view(5, 1).expand(5, 4))
    for name in mg.readout.__all__:
        assert getattr(dgl, name) is getattr(mg.readout, name) is getattr(mg, name)


def lstm_step64(lstm, x, h, c):
    """one time step of an nn.LSTM in fp64 from its parameters (PyTorch's documented formulas; gate order i, f, g, o)"""
    hs, cs = [], []
    for k in range(lstm.num_layers):
        p = {n: getattr(lstm, "%s_l%d" % (n, k)).detach().double() for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")}
        gates = x @ p["weight_ih"].t() + p["bias_ih"] + h[k] @ p["weight_hh"].t() + p["bias_hh"]
        i, f, g_, o = gates.chunk(4, 1)
        ck = torch.sigmoid(f) * c[k] + torch.sigmoid(i) * torch.tanh(g_)
        x = torch.sigmoid(o) * torch.tanh(ck)
        hs.append(x)
        cs.append(ck)
    return x, hs, cs


def test_layers_shapes_state_dicts_and_values(cpu_backend_on):
    import dgl
    import dgl.nn.pytorch as dglnn
    graphs = small_graphs([3, 1, 7, 4, 9], seed=3)
    bg = dgl.batch(graphs)
    lens = [3, 1, 7, 4, 9]
    torch.manual_seed(4)
    feat = torch.randn(24, 6)
    # GlobalAttentionPooling
    pool = dglnn.GlobalAttentionPooling(torch.nn.Linear(6, 1), torch.nn.Linear(6, 8))
    assert sorted(pool.state_dict()) == ["feat_nn.bias", "feat_nn.weight", "gate_nn.bias", "gate_nn.weight"]
    out = pool(bg, feat)
    assert tuple(out.shape) == (5, 8)
    ref = Restated(lens, pool.feat_nn(feat).view(24, 1, 8), logits=pool.gate_nn(feat).view(24, 1))
    assert torch.allclose(out.double(), ref.out.view(5, 8), rtol=1e-5, atol=1e-6)
    out.sum().backward()
    assert pool.gate_nn.weight.grad is not None and float(pool.feat_nn.weight.grad.abs().max()) > 0
    assert tuple(dglnn.GlobalAttentionPooling(torch.nn.Linear(6, 1))(bg, feat).shape) == (5, 6)
    with pytest.raises(mg.DGLError, match="The output of gate_nn should have size 1 at the last axis"):
        dglnn.GlobalAttentionPooling(torch.nn.Linear(6, 2))(bg, feat)
    # Set2Set
    for n_layers in (1, 2):
        s2s = dglnn.Set2Set(6, n_iters=3, n_layers=n_layers)
        keys = ["lstm.%s_l%d" % (n, k) for k in range(n_layers) for n in ("bias_hh", "bias_ih", "weight_hh", "weight_ih")]
        assert sorted(s2s.state_dict()) == sorted(keys)
        assert tuple(s2s.lstm.weight_ih_l0.shape) == (24, 12) and tuple(s2s.lstm.weight_hh_l0.shape) == (24, 6)
        out = s2s(bg, feat)
        assert tuple(out.shape) == (5, 12)
        h = [torch.zeros(5, 6, dtype=torch.float64) for _ in range(n_layers)]
        c = [torch.zeros(5, 6, dtype=torch.float64) for _ in range(n_layers)]
        q_star = torch.zeros(5, 12, dtype=torch.float64)
        for _ in range(3):
            q, h, c = lstm_step64(s2s.lstm, q_star, h, c)
            r = Restated(lens, feat.view(24, 1, 6), query=q.view(5, 1, 6), scale=1.0).out.view(5, 6)
            q_star = torch.cat([q, r], 1)
        assert torch.allclose(out.double(), q_star, rtol=1e-5, atol=1e-6)
        # the written-out step IS nn.LSTM's: one step of the module itself from the zero state
        with torch.no_grad():
            x0 = torch.randn(5, 12)
            y, _ = s2s.lstm(x0.unsqueeze(0))
            mine, _, _ = s2s._lstm_step(x0, [torch.zeros(5, 6)] * n_layers, [torch.zeros(5, 6)] * n_layers)
        assert torch.allclose(y[0], mine, rtol=1e-5, atol=1e-6)
        out.sum().backward()
        assert all(p.grad is not None for p in s2s.parameters())
    # WeightAndSum
    ws = dglnn.WeightAndSum(6)
    assert sorted(ws.state_dict()) == ["atom_weighting.0.bias", "atom_weighting.0.weight"]
    out = ws(bg, feat)
    wgt = torch.sigmoid(feat @ ws.atom_weighting[0].weight.detach().t() + ws.atom_weighting[0].bias.detach())
    assert tuple(out.shape) == (5, 6)
    assert torch.allclose(out, torch.stack([p.sum(0) for p in (feat * wgt).split(lens)]), rtol=1e-5, atol=1e-6)
    assert dglnn.glob.Set2Set is mg.nn.Set2Set and dgl.nn.GlobalAttentionPooling is mg.nn.GlobalAttentionPooling
    assert dglnn.glob.WeightAndSum is mg.nn.WeightAndSum


def test_argument_errors_raise_dglerror(cpu_backend_on):
    seglen, feat, logits, _, _, _ = case(CPU_LENS, 3, 4, "gate")
    query = torch.randn(len(CPU_LENS), 3, 4)
    with pytest.raises(mg.DGLError, match="both"):
        ops.segment_attention(seglen, feat, logits=logits, query=query)
    with pytest.raises(mg.DGLError, match="neither"):
        ops.segment_attention(seglen, feat)
    with pytest.raises(mg.DGLError, match="64 rows|has 63 rows"):
        ops.segment_attention(seglen, feat[:63], logits=logits[:63])
    with pytest.raises(mg.DGLError, match=r"\(63, 3\)"):
        ops.segment_attention(seglen, feat, logits=logits[:63])
    with pytest.raises(mg.DGLError, match=r"\(6, 3, 4\)"):
        ops.segment_attention(seglen, feat, query=query[:6])
    with pytest.raises(mg.DGLError, match="float32"):
        ops.segment_attention(seglen, feat.double(), logits=logits.double())
    with pytest.raises(mg.DGLError, match="float32"):
        ops.segment_attention(seglen, feat, query=query.double())
    with pytest.raises(mg.DGLError, match=r"\(64, 12\)"):
        ops.segment_attention(seglen, feat.view(64, 12), logits=logits)
    with pytest.raises(mg.DGLError, match="float32"):
        ops.segment_softmax(seglen, logits.double())
    with pytest.raises(mg.DGLError, match="63 rows"):
        ops.segment_softmax(seglen, logits[:63])
    assert config.SEGMENT_ATTENTION_FUSED in (True, False)


def test_without_a_cpu_backend_cpu_tensors_fail_loudly(monkeypatch):
    seglen, feat, logits, _, _, _ = case(CPU_LENS, 3, 4, "gate")
    monkeypatch.delitem(mg.sparse._BACKENDS, "cpu", raising=False)
    with pytest.raises(mg.DGLError, match="MI355X"):
        ops.segment_attention(seglen, feat, logits=logits)
    with pytest.raises(mg.DGLError, match="MI355X"):
        ops.segment_softmax(seglen, logits)


def test_abi_argument_checks():
    L = _lib.lib()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("mgx_segment_softmax_fwd", "mgx_segment_softmax_bwd", "mgx_segment_attention_supported", "mgx_segment_attention_fwd",
                 "mgx_segment_attention_bwd"):
        assert hasattr(handle, name) and name in _lib.SIGNATURES
    assert L.mgx_abi_version() == 35
    for (H, Fd), want in (((1, 4), 1), ((1, 20), 1), ((1, 256), 1), ((1, 260), 0), ((3, 4), 1), ((3, 12), 0), ((4, 64), 1), ((8, 64), 0)):
        assert L.mgx_segment_attention_supported(H, Fd, H * Fd) == want, (H, Fd)
    assert not L.mgx_segment_attention_supported(1, 8, 10) and not L.mgx_segment_attention_supported(1, 8, 4)   # stride: no multiple of 4; below H*F
    assert L.mgx_segment_attention_supported(1, 8, 24) and not L.mgx_segment_attention_supported(1, 6, 8)
    host = (ctypes.c_float * 64)()                                             # never dereferenced: every call below fails a check first
    base = ctypes.addressof(host)
    base += (-base) % 16
    p = ctypes.c_void_p(base)

    def fwd(H, Fd, logits=None, query=None, feat=p, ld=None, out=p, stat=p):
        return L.mgx_segment_attention_fwd(2, p, H, Fd, feat, H * Fd if ld is None else ld, logits, query, ctypes.c_float(1.0), out, stat, None)

    assert fwd(1, 8) == 1 and b"neither" in L.mgx_last_error()
    with pytest.raises(mg.DGLError, match="exactly one of logits"):
        _lib.check(1)
    assert fwd(1, 8, p, p) == 1 and b"both" in L.mgx_last_error()
    assert fwd(0, 8, p) == 1 and fwd(1, 0, p) == 1
    assert fwd(1, 260, p) == _lib.ERR_UNSUPPORTED and fwd(3, 12, p) == _lib.ERR_UNSUPPORTED and fwd(1, 8, p, ld=10) == _lib.ERR_UNSUPPORTED
    assert fwd(1, 8, p, feat=None) == 1 and b"feat is NULL" in L.mgx_last_error()
    assert fwd(1, 8, p, feat=ctypes.c_void_p(base + 4)) == 1 and b"aligned" in L.mgx_last_error()
    assert fwd(1, 8, p, out=None) == 1 and fwd(1, 8, query=p, stat=None) == 1
    bwd = L.mgx_segment_attention_bwd
    assert bwd(2, p, 1, 8, p, 8, None, None, ctypes.c_float(1.0), p, p, p, p, None, None, None) == 1
    assert bwd(2, p, 1, 8, p, 8, p, None, ctypes.c_float(1.0), p, p, p, p, None, p, None) == 1 and b"gate mode" in L.mgx_last_error()
    assert bwd(2, p, 1, 8, p, 8, p, None, ctypes.c_float(1.0), None, p, p, p, p, None, None) == 1
    assert L.mgx_segment_softmax_fwd(2, p, 0, p, p, None) == 1 and L.mgx_segment_softmax_fwd(2, None, 4, p, p, None) == 1
    assert L.mgx_segment_softmax_fwd(2, p, 4, None, p, None) == 1 and L.mgx_segment_softmax_bwd(2, p, 4, p, None, p, None) == 1
    assert L.mgx_segment_softmax_fwd(0, None, 4, None, None, None) == 0        # no segments: nothing to do


# ----------------------------------------------------------------------------- GPU: the fused pair against the restatement
@pytest.mark.gpu
@pytest.mark.parametrize("lens", [LENS, LENS_ZERO_LAST], ids=["zero_first_and_inside", "zero_last"])
@pytest.mark.parametrize("H,Fd", WIDTHS)
@pytest.mark.parametrize("mode", ["gate", "query"])
def test_fused_pair_matches_the_restatement(monkeypatch, mode, H, Fd, lens):
    seglen, feat, logits, query, up, ref = case(tuple(lens), H, Fd, mode)
    rec = launches(monkeypatch)
    assert ops.segment_attention_fused(seglen.to(DEV), feat.to(DEV), logits=None if logits is None else logits.to(DEV),
                                       query=None if query is None else query.to(DEV))
    out, grads = run(seglen, feat, logits, query, 0.37, up, DEV)
    assert [r["kernel"] for r in rec] == ["seg_attn_fwd", "seg_attn_bwd"]      # one launch each way, nothing else from the library
    assert tuple(out.shape) == (len(lens), H, Fd)
    check_forward(out, ref)
    empty = (seglen == 0).to(DEV)
    assert torch.all(out[empty] == 0)                                          # empty segments read out exactly 0
    check_grads(grads, ref)
    if mode == "query":
        assert torch.all(grads["d_query"][empty] == 0)
    # the backend called directly: the same bits, the statistics, subsets of the gradients
    be = mg.sparse.backend_for(out)
    offs = torch.cat([torch.zeros(1, dtype=torch.int64), seglen.cumsum(0)]).to(DEV)
    lg, q = (None if t is None else t.to(DEV) for t in (logits, query))
    o, st = be.segment_attention_fwd(offs, feat.to(DEV), lg, q, 0.37)
    assert torch.equal(o, out) and tuple(st.shape) == (len(lens), H, 2)
    assert torch.all(st[empty] == 0)
    g3 = be.segment_attention_bwd(offs, feat.to(DEV), lg, q, 0.37, o, up.to(DEV), st, True, True, True)
    for name, got in zip(("d_feat", "d_logits", "d_query"), g3):
        assert (got is None) == (name not in grads) and (got is None or torch.equal(got, grads[name].view(got.shape)))
    only = be.segment_attention_bwd(offs, feat.to(DEV), lg, q, 0.37, o, up.to(DEV), st, False, True, True)   # needs_input_grad subsets
    assert only[0] is None and all(b_ is None or torch.equal(a_, b_) for a_, b_ in zip(g3[1:], only[1:]))


@pytest.mark.gpu
@pytest.mark.parametrize("H,Fd", [(3, 4), (1, 64)])
def test_gate_logits_spanning_160(H, Fd):
    lens = [7, 300, 2]
    gen = torch.Generator().manual_seed(Fd)
    feat, up = torch.randn(309, H, Fd, generator=gen), torch.randn(3, H, Fd, generator=gen)
    logits = torch.randn(309, H, generator=gen)
    for h in range(H):                                                          # -80 .. 80 across the long segment, in a random order per head
        logits[7:307, h] = torch.linspace(-80, 80, 300)[torch.randperm(300, generator=gen)]
    ref = Restated(lens, feat, logits, dout=up)
    out, grads = run(torch.tensor(lens), feat, logits, None, 1.0, up, DEV)
    check_forward(out, ref)
    check_grads(grads, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["gate", "query"])
@pytest.mark.parametrize("H,Fd,fused", [(1, 20, True), (4, 16, True), (1, 256, True), (1, 260, False), (3, 12, False)])
def test_fused_pair_equals_the_composition(monkeypatch, mode, H, Fd, fused):
    seglen, feat, logits, query, up, ref = case(tuple(LENS), H, Fd, mode, seed=7)
    dev = [None if t is None else t.to(DEV) for t in (seglen, feat, logits, query)]
    monkeypatch.setattr(config, "SEGMENT_ATTENTION_FUSED", True)
    assert ops.segment_attention_fused(dev[0], dev[1], logits=dev[2], query=dev[3]) == fused
    out_on, grads_on = run(seglen, feat, logits, query, 0.37, up, DEV)
    monkeypatch.setattr(config, "SEGMENT_ATTENTION_FUSED", False)
    assert not ops.segment_attention_fused(dev[0], dev[1], logits=dev[2], query=dev[3])
    out_off, grads_off = run(seglen, feat, logits, query, 0.37, up, DEV)
    for out in (out_on, out_off):
        check_forward(out, ref)
        assert torch.all(out[(seglen == 0).to(DEV)] == 0)
    for grads in (grads_on, grads_off):
        check_grads(grads, ref)
    if not fused:                                                               # the same operators either way
        assert torch.equal(out_on, out_off)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["gate", "query"])
@pytest.mark.parametrize("H,Fd", [(1, 4), (1, 20), (4, 16), (1, 256)])
def test_zero_logits_give_the_exact_mean(mode, H, Fd):
    """exp(0) = 1, a sum of at most 256 integers in [-64, 64] is an exact small integer in any order, and dividing by a power of two is
    exact: the output IS the mean, bit for bit -- a lost or doubled row moves it."""
    lens = [1, 2, 4, 8, 64, 256, 4, 1]
    N, S = sum(lens), len(lens)
    rng = np.random.default_rng(Fd)
    feat = torch.from_numpy(rng.integers(-64, 65, (N, H, Fd)).astype(np.float32))
    seglen = torch.tensor(lens)
    kw = {"logits": torch.zeros(N, H, device=DEV)} if mode == "gate" else {"query": torch.zeros(S, H, Fd, device=DEV), "scale": 0.7}
    assert ops.segment_attention_fused(seglen.to(DEV), feat.to(DEV), **kw)
    out = ops.segment_attention(seglen.to(DEV), feat.to(DEV), total=N, **kw).cpu()
    mean = torch.stack([p.double().sum(0) / p.shape[0] for p in feat.split(lens)]).float()
    assert torch.equal(out, mean)


@pytest.mark.gpu
@pytest.mark.parametrize("H,Fd", [(3, 4), (1, 64)])
def test_edge_rules(H, Fd):
    lens = [5, 70, 0, 33, 9]
    seglen, feat, logits, _, up, ref = case(tuple(lens), H, Fd, "gate", seed=3)
    clean, clean_grads = run(seglen, feat, logits, None, 1.0, up, DEV)
    # one -inf logit: the row is ignored -- the result is that of the segment without it (here: of the restatement with weight 0)
    one = logits.clone()
    one[5 + 64, 0] = -INF                                                       # row 64 of the 70-row segment, head 0
    out, grads = run(seglen, feat, one, None, 1.0, up, DEV)
    r1 = Restated(lens, feat, one, dout=up)
    assert float(r1.a[69, 0]) == 0
    check_forward(out, r1)
    check_grads(grads, r1)
    assert torch.all(grads["d_logits"][69, 0] == 0) and torch.all(grads["d_feat"][69, 0] == 0)
    # all -inf: like an empty segment -- 0 in out and in every gradient
    allm = logits.clone()
    allm[75:108] = -INF                                                         # the segment of 33 rows, every head
    out, grads = run(seglen, feat, allm, None, 1.0, up, DEV)
    assert torch.all(out[3] == 0) and torch.all(grads["d_feat"][75:108] == 0) and torch.all(grads["d_logits"][75:108] == 0)
    keep = torch.tensor([0, 1, 2, 4])
    assert torch.equal(out[keep], clean[keep])                                  # bitwise
    # one NaN logit: exactly its own (segment, head)
    nan = logits.clone()
    nan[5 + 17, H - 1] = float("nan")
    out, grads = run(seglen, feat, nan, None, 1.0, up, DEV)
    hit = torch.zeros(5, H, dtype=torch.bool)
    hit[1, H - 1] = True
    hit = hit.to(DEV)
    assert torch.equal(torch.isnan(out), hit.unsqueeze(-1).expand(5, H, Fd))
    assert torch.equal(out[~hit], clean[~hit])                                  # bitwise
    rows = torch.zeros(sum(lens), H, dtype=torch.bool)
    rows[5:75, H - 1] = True
    rows = rows.to(DEV)
    assert torch.equal(torch.isnan(grads["d_logits"]), rows)
    assert torch.equal(grads["d_logits"][~rows], clean_grads["d_logits"][~rows])
    # query mode: a NaN in one query row reaches exactly that (segment, head)
    seglen, feat, _, query, up, _ = case(tuple(lens), H, Fd, "query", seed=3)
    clean, _ = run(seglen, feat, None, query, 0.5, up, DEV)
    qn = query.clone()
    qn[4, 0, 1] = float("nan")
    out, _ = run(seglen, feat, None, qn, 0.5, up, DEV)
    hit = torch.zeros(5, H, dtype=torch.bool)
    hit[4, 0] = True
    hit = hit.to(DEV)
    assert torch.equal(torch.isnan(out), hit.unsqueeze(-1).expand(5, H, Fd)) and torch.equal(out[~hit], clean[~hit])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["gate", "query"])
@pytest.mark.parametrize("H,Fd", [(1, 20), (4, 16), (1, 256)])
def test_reruns_and_strided_features_are_bitwise_equal(mode, H, Fd):
    seglen, feat, logits, query, up, _ = case(tuple(LENS), H, Fd, mode, seed=11)
    first, grads1 = run(seglen, feat, logits, query, 0.37, up, DEV)
    again, grads2 = run(seglen, feat, logits, query, 0.37, up, DEV)
    assert torch.equal(first, again) and all(torch.equal(grads1[k], grads2[k]) for k in grads1)
    N, D = feat.shape[0], H * Fd
    wide = torch.randn(N, D + 8 + D, device=DEV)
    wide[:, D + 8:] = feat.view(N, D).to(DEV)
    wide.requires_grad_(True)
    block = wide[:, D + 8:].view(N, H, Fd)                                      # a column block: feat_ld = 2 D + 8 > H F, 16-byte aligned
    assert not block.is_contiguous() and mg.sparse.HipBackend._seg_operand(block)[1] == 2 * D + 8
    kw = {"logits": logits.to(DEV)} if mode == "gate" else {"query": query.to(DEV)}
    out = ops.segment_attention(seglen.to(DEV), block, scale=0.37, total=N, **kw)
    (out * up.to(DEV)).sum().backward()
    assert torch.equal(out.detach(), first)
    assert torch.equal(wide.grad[:, D + 8:], grads1["d_feat"].view(N, D)) and torch.all(wide.grad[:, :D + 8] == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["gate", "query"])
def test_contiguous_operands_at_an_odd_storage_offset(mode):
    """a contiguous tensor need not start on a 16-byte boundary: a query or features cut out of a flat buffer one float in, an upstream
    gradient that is a slice of a flattened cat -- the backend copies what the kernels would refuse, and the bits are those of aligned operands"""
    H, Fd = 4, 16
    seglen, feat, logits, query, up, _ = case(tuple(LENS), H, Fd, mode, seed=13)
    want, want_grads = run(seglen, feat, logits, query, 0.37, up, DEV)

    def shifted(t):
        flat = torch.zeros(t.numel() + 1, device=DEV)
        flat[1:] = t.reshape(-1).to(DEV)
        v = flat[1:].view(t.shape)
        assert v.is_contiguous() and v.data_ptr() % 16 == 4
        return v

    f = shifted(feat).requires_grad_(True)
    lg = None if logits is None else shifted(logits).requires_grad_(True)
    q = None if query is None else shifted(query).requires_grad_(True)
    assert ops.segment_attention_fused(seglen.to(DEV), f, logits=lg, query=q)
    out = ops.segment_attention(seglen.to(DEV), f, logits=lg, query=q, scale=0.37, total=int(feat.shape[0]))
    assert torch.equal(out.detach(), want)
    both = torch.cat([torch.zeros(1, device=DEV), up.reshape(-1).to(DEV)])       # d(loss)/d(out) arrives as the slice [1:] of this
    (torch.cat([out.new_zeros(1), out.reshape(-1)]) * both).sum().backward()
    got = {"d_feat": f.grad, "d_logits": None if lg is None else lg.grad, "d_query": None if q is None else q.grad}
    for name, g_ in want_grads.items():
        assert torch.equal(got[name], g_), name


@pytest.mark.gpu
@pytest.mark.parametrize("D", [1, 3, 64, 100])
def test_segment_softmax_on_the_device(D):
    for lens in (LENS, LENS_ZERO_LAST):
        N = sum(lens)
        gen = torch.Generator().manual_seed(D)
        x, dy = torch.randn(N, D, generator=gen) * 3, torch.randn(N, D, generator=gen)
        want, want_dx = restated_softmax(lens, x, dy)
        xd = x.to(DEV).requires_grad_(True)
        out = ops.segment_softmax(torch.tensor(lens).to(DEV), xd, total=N)
        err = (out.detach().cpu().double() - want).abs()
        assert not (err > RTOL * want + 1e-30).any(), float((err / want).max())
        sums = torch.stack([p.sum(0) for p in out.detach().cpu().double().split(lens) if p.shape[0]])
        assert float((sums - 1).abs().max()) <= RTOL                            # per-element bound, summed over a column
        dx, = torch.autograd.grad((out * dy.to(DEV)).sum(), xd)
        gerr = float((dx.cpu().double() - want_dx).abs().max())
        assert gerr <= RTOL * float(want_dx.abs().max()), gerr
        out2 = ops.segment_softmax(torch.tensor(lens).to(DEV), x.to(DEV), total=N)
        assert torch.equal(out2, out.detach())
    # the edge rules of the attention kernels, per column
    x = torch.randn(12, 3)
    x[0:4, 1] = -INF
    x[5, 0] = -INF
    x[9, 2] = float("nan")
    out = ops.segment_softmax(torch.tensor([4, 4, 4]).to(DEV), x.to(DEV)).cpu()
    assert torch.all(out[0:4, 1] == 0) and float(out[5, 0]) == 0 and abs(float(out[4:8, 0].sum()) - 1) <= RTOL
    want_nan = torch.zeros(12, 3, dtype=torch.bool)
    want_nan[8:12, 2] = True
    assert torch.equal(torch.isnan(out), want_nan)


def _forty_graphs(width, seed=0):
    import dgl
    from mi355x_graph.datasets import molhiv_like
    data = molhiv_like(40, seed=17)
    bg = dgl.batch([data[i][0] for i in range(40)])
    gen = torch.Generator().manual_seed(seed)
    return bg.to(DEV), torch.randn(bg.number_of_nodes(), width, generator=gen).to(DEV)


def _step(module, bg, feat, up):
    module.zero_grad(set_to_none=True)
    x = feat.clone().requires_grad_(True)
    out = module(bg, x)
    (out * up).sum().backward()
    return out.detach(), [("input", x.grad)] + [(n_, p.grad.clone()) for n_, p in module.named_parameters()]


@pytest.mark.gpu
@pytest.mark.parametrize("layer", ["attention", "set2set"])
def test_layers_with_the_fused_path_on_and_off(monkeypatch, layer):
    bg, feat = _forty_graphs(16)
    torch.manual_seed(1)
    if layer == "attention":
        # a gate without bias: the softmax does not move when every gate of a graph shifts by one constant, so a bias's gradient is
        # exactly 0 and only rounding noise would be left to compare; every tensor here has a gradient the bound can be held against
        module = mg.nn.GlobalAttentionPooling(torch.nn.Linear(16, 1, bias=False), torch.nn.Linear(16, 16)).to(DEV)
        width = 16
    else:
        module = mg.nn.Set2Set(16, n_iters=3, n_layers=1).to(DEV)
        width = 32
    up = torch.randn(40, width, device=DEV)
    monkeypatch.setattr(config, "SEGMENT_ATTENTION_FUSED", True)
    rec = launches(monkeypatch)
    out_on, grads_on = _step(module, bg, feat, up)
    rounds = 1 if layer == "attention" else 3
    assert tuple(out_on.shape) == (40, width)
    assert sorted(r["kernel"] for r in rec) == ["seg_attn_bwd"] * rounds + ["seg_attn_fwd"] * rounds
    monkeypatch.setattr(config, "SEGMENT_ATTENTION_FUSED", False)
    del rec[:]
    out_off, grads_off = _step(module, bg, feat, up)
    assert rec and not any(r["kernel"].startswith("seg_attn") for r in rec)
    err, top = float((out_on - out_off).abs().max()), float(out_off.abs().max())
    print("output: max err %.3e, max |composed| %.3e" % (err, top))
    assert err <= RTOL * top
    for (name, a_), (_, b_) in zip(grads_on, grads_off):
        err, top = float((a_ - b_).abs().max()), float(b_.abs().max())
        print("%s: max err %.3e, max |composed| %.3e" % (name, err, top))
        assert err <= RTOL * top, (name, err, top)


@pytest.mark.gpu
def test_global_attention_pooling_captured_in_a_hip_graph():
    """the capture idiom of tests/test_graphed_batches.py / GraphedBatchTrainer: warm-up and capture on ONE side stream, then replay with
    new feature values in the static input -- the readout reads nothing back to the host"""
    bg, feat = _forty_graphs(16)
    torch.manual_seed(2)
    module = mg.nn.GlobalAttentionPooling(torch.nn.Linear(16, 1, bias=False), torch.nn.Linear(16, 16)).to(DEV)
    up = torch.randn(40, 16, device=DEV)
    static = feat.clone()

    def step():
        module.zero_grad(set_to_none=True)
        out = module(bg, static)
        (out * up).sum().backward()
        return out

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), ops.warming_up_for_capture():
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    module.zero_grad(set_to_none=True)
    with torch.cuda.graph(graph, stream=side):
        out = step()
    new = torch.randn(feat.shape, generator=torch.Generator().manual_seed(9)).to(DEV)
    static.copy_(new)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    got_out, got_grads = out.detach().clone(), [p.grad.clone() for p in module.parameters()]
    twin = mg.nn.GlobalAttentionPooling(torch.nn.Linear(16, 1, bias=False), torch.nn.Linear(16, 16)).to(DEV)   # eager, on the default stream
    twin.load_state_dict(module.state_dict())
    want = twin(bg, new)
    (want * up).sum().backward()
    assert float((got_out - want.detach()).abs().max()) <= RTOL * float(want.detach().abs().max())
    for g_, (name, p) in zip(got_grads, twin.named_parameters()):
        assert float((g_ - p.grad).abs().max()) <= RTOL * float(p.grad.abs().max()), name


@functools.lru_cache(maxsize=None)
def _script(*args):
    """(loss printed for epoch 1, whole output) of one run of the script; a run is shared by the tests that need it"""
    env = dict(os.environ, MGX_DATASET_SCALE="0.01", PYTHONPATH=PKG)
    cmd = [sys.executable, os.path.join(PKG, "graph_classification.py"), "--num_graphs", "320", "--batch_size", "64", "--epochs", "1",
           "--emb_dim", "64", "--num_layers", "2"] + list(args)
    res = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert res.returncode == 0, res.stdout[-3000:]
    m = re.search(r"epoch 1 loss (\S+)", res.stdout)
    assert m, res.stdout[-3000:]
    return m.group(1), res.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("hipgraph", [False, True], ids=["eager", "hipgraph"])
@pytest.mark.parametrize("readout", ["attention", "set2set"])
def test_script_readouts_train_to_a_finite_loss(readout, hipgraph):
    """five batches of 64 molecules (--num_graphs shrinks the molhiv stand-in; MGX_DATASET_SCALE covers the stand-ins that read it)"""
    loss, text = _script("--readout", readout, *(["--hipgraph"] if hipgraph else []))
    assert np.isfinite(float(loss)), text[-2000:]
    if hipgraph:
        replayed = re.search(r"(\d+) steps replayed", text)
        assert replayed and int(replayed.group(1)) >= 5, text[-2000:]


@pytest.mark.gpu
def test_script_mean_readout_trains_to_a_finite_loss():
    loss, text = _script("--readout", "mean")
    assert np.isfinite(float(loss)), text[-2000:]


@pytest.mark.gpu
def test_script_mean_readout_is_the_default_model():
    with_flag, _ = _script("--readout", "mean")                                 # shared with the test above
    without, _ = _script()
    assert with_flag == without and np.isfinite(float(without))
