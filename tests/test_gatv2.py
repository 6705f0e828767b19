"""GATv2 attention over a graph: csrc/gatv2.hip (mgx_gatv2_*), ops.gatv2_attention, nn.GATv2Conv, full_graph.GATv2.

The reference everywhere is the fp64 restatement below, written from the definition over the COO edge list on the fp32 inputs:

    s[e,h,f] = fs[u,h,f] + fd[v,h,f];  z[e,h] = sum_f attn[h,f] lrelu(s);  a = exp(z - m[v]) / S[v];  out[v,h,:] = sum_{e: u->v} a fs[u,h,:]
    t = <out, dout>;  dp[e,h] = <fs[u,h,:], dout[v,h,:]>;  dz = a (dp - t);  g = dz attn lrelu'(s)   (lrelu'(x) = 1 for x > 0, else slope)
    dfd[v] = sum g;  dfs[u] = sum (g + a dout[v]);  dattn[h,f] = sum over all edges of dz lrelu(s)

  CPU   the composition behind ops.gatv2_attention (checker backend and the OpenMP backend) and nn.GATv2Conv: rtol 1e-5, atol 1e-6
  GPU   the fused kernels: forward per element |got - ref| <= 1e-4 * sum_e a |fs|, each gradient 1e-4 * the reference gradient's max"""
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


class Restated(object):
    """fp64, COO, never the code under test"""

    def __init__(self, src, dst, n_src, n_dst, fs, fd, attn, slope, dout=None):
        src, dst = torch.as_tensor(src).long().cpu(), torch.as_tensor(dst).long().cpu()
        fs, fd, attn = (t.detach().cpu().double() for t in (fs, fd, attn))
        H, Fd = fs.shape[1], fs.shape[2]
        attn = attn.reshape(1, H, Fd)
        s = fs[src] + fd[dst]                                                                # [E, H, F]
        lr = torch.where(s > 0, s, s * slope)
        z = (lr * attn).sum(-1)                                                               # [E, H]
        m = torch.full((n_dst, H), -float("inf"), dtype=torch.float64).index_reduce_(0, dst, z, "amax", include_self=True)
        e = torch.exp(z - m[dst])
        a = e / torch.zeros((n_dst, H), dtype=torch.float64).index_add_(0, dst, e)[dst]
        self.s, self.z, self.a = s, z, a
        self.out = torch.zeros((n_dst, H, Fd), dtype=torch.float64).index_add_(0, dst, a.unsqueeze(-1) * fs[src])
        self.row_scale = torch.zeros((n_dst, H, Fd), dtype=torch.float64).index_add_(0, dst, a.unsqueeze(-1) * fs[src].abs())
        if dout is not None:
            dout = dout.detach().cpu().double()
            t = (self.out * dout).sum(-1)
            dz = (a * ((fs[src] * dout[dst]).sum(-1) - t[dst])).unsqueeze(-1)
            g = dz * attn * torch.where(s > 0, 1.0, slope)
            self.dfd = torch.zeros((n_dst, H, Fd), dtype=torch.float64).index_add_(0, dst, g)
            self.dfs = torch.zeros((n_src, H, Fd), dtype=torch.float64).index_add_(0, src, g + a.unsqueeze(-1) * dout[dst])
            self.dattn = (dz * lr).sum(0)


def build(kind, device="cpu", idtype=torch.int32):
    """(graph, src, dst, n_src, n_dst): random graphs with duplicate edges and isolated destinations (`square`, `block`), the degrees
    1, 63, 64, 65 either way (`degrees`: the 64-wide id fetch less one, full, plus one), and a hub destination and a hub source whose
    rows the plan splits (`hub`, as tests/test_dot_attention.py builds it: destinations 0..4 without in-edges)."""
    rng = np.random.default_rng(29)
    if kind in ("square", "block"):
        n_src, n_dst = (300, 300) if kind == "square" else (500, 200)
        src, dst = random_graph(n_src, n_dst, 8 * n_dst, seed=n_src)
    elif kind == "degrees":
        n_src = n_dst = 300
        degs = (1, 63, 64, 65)
        src = np.concatenate([rng.integers(20, 300, d) for d in degs] + [np.full(d, 10 + i) for i, d in enumerate(degs)])
        dst = np.concatenate([np.full(d, i) for i, d in enumerate(degs)] + [rng.integers(20, 300, d) for d in degs])
    else:
        n_src = n_dst = 600
        src, dst = random_graph(n_src, n_dst, 20 * n_src, seed=7)
        src, dst = src[dst >= 5], dst[dst >= 5]
        src = np.concatenate([src, rng.integers(0, n_src, 3000), np.full(3000, 7)])
        dst = np.concatenate([dst, np.full(3000, 11), rng.integers(5, n_dst, 3000)])
    src, dst = src.astype(np.int64), dst.astype(np.int64)
    s, d = torch.from_numpy(src), torch.from_numpy(dst)
    if n_src == n_dst:
        g = mg.graph((s, d), num_nodes=n_src)
        g = (g.int() if idtype == torch.int32 else g.long()).to(device)
    else:
        g = mg.create_block((s, d), n_src, n_dst, idtype=idtype, device=device)
    return g, src, dst, n_src, n_dst


def operands(n_src, n_dst, H, Fd, seed):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(n_src, H, Fd, generator=gen), torch.randn(n_dst, H, Fd, generator=gen), torch.randn(1, H, Fd, generator=gen),
            torch.randn(n_dst, H, Fd, generator=gen))


def check(out, grads, ref, names=("dfs", "dfd", "dattn")):
    err = (out.detach().cpu().double() - ref.out).abs()
    print("forward: max err / sum_e a|fs| = %.3e" % float((err / (ref.row_scale + 1e-30)).max()))
    assert not (err > RTOL * ref.row_scale + 1e-30).any()
    for name, got in zip(names, grads):
        want = getattr(ref, name)
        err, top = float((got.detach().cpu().double().reshape(want.shape) - want).abs().max()), float(want.abs().max())
        print("%s: max err %.3e, max |reference| %.3e" % (name, err, top))
        assert err <= RTOL * top, (name, err, top)


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


@pytest.mark.parametrize("kind", ["square", "block"])
@pytest.mark.parametrize("H,Fd", [(1, 1), (3, 4), (2, 16)])
def test_composition_and_its_gradients_match_the_restatement(cpu_backend_on, kind, H, Fd):
    g, src, dst, n_src, n_dst = build(kind)
    deg = np.bincount(dst, minlength=n_dst)
    assert len(set(zip(src.tolist(), dst.tolist()))) < len(src) and deg.min() == 0      # duplicate edges, isolated destinations
    fs, fd, attn, up = operands(n_src, n_dst, H, Fd, H + Fd)
    # atol 1e-6 is absolute and the composition is fp32: an element of d fd is a sum of ~8 terms that cancel (sum_e dz = 0), its
    # error ~ (rounding steps ~ 8) * 2^-24 * sum |terms|, so the terms must sum to ~ 2 at most; an upstream gradient of N(0, 0.1)
    # puts them there (N(0, 1) leaves sums of ~ 20, i.e. ~ 1e-5 of fp32 rounding)
    up = 0.1 * up
    ins = [t.requires_grad_(True) for t in (fs, fd, attn)]
    assert not ops.gatv2_attention_fused(g, *ins)
    ref = Restated(src, dst, n_src, n_dst, fs, fd, attn, 0.3, up)
    out = ops.gatv2_attention(g, *ins, negative_slope=0.3)
    assert tuple(out.shape) == (n_dst, H, Fd) and torch.all(out[deg == 0] == 0)
    assert torch.allclose(out.double(), ref.out, rtol=1e-5, atol=1e-6)
    for name, got in zip(("dfs", "dfd", "dattn"), torch.autograd.grad((out * up).sum(), ins)):
        assert torch.allclose(got.double().reshape(getattr(ref, name).shape), getattr(ref, name), rtol=1e-5, atol=1e-6), name


@pytest.mark.parametrize("share", [False, True])
@pytest.mark.parametrize("kind", ["square", "block"])
def test_gatv2_conv_equals_the_restatement(cpu_backend_on, kind, share):
    g, src, dst, n_src, n_dst = build(kind)
    torch.manual_seed(3)
    H, Fd, K = 3, 4, 6
    conv = mg.nn.GATv2Conv(K, Fd, H, negative_slope=0.3, residual=True, bias=True, share_weights=share)
    shapes = {k: tuple(v.shape) for k, v in conv.state_dict().items()}
    want = {"fc_src.weight": (H * Fd, K), "fc_src.bias": (H * Fd,), "attn": (1, H, Fd), "res_fc.weight": (H * Fd, K), "res_fc.bias": (H * Fd,)}
    if not share:
        want.update({"fc_dst.weight": (H * Fd, K), "fc_dst.bias": (H * Fd,)})
    assert shapes == want and (conv.fc_dst is conv.fc_src) == share
    assert sorted(mg.nn.GATv2Conv(K, Fd, H, bias=False, share_weights=True).state_dict()) == ["attn", "fc_src.weight"]
    feat = torch.randn(n_src, K)
    with pytest.raises(mg.DGLError, match="0-in-degree"):
        conv(g, feat)
    conv.set_allow_zero_in_degree(True)
    with torch.no_grad():
        for p in conv.parameters():                       # biases start at 0: give them something to do
            p.add_(0.1 * torch.randn_like(p))
        fs = F.linear(feat, conv.fc_src.weight, conv.fc_src.bias).view(n_src, H, Fd)
        fd = F.linear(feat[:n_dst], conv.fc_dst.weight, conv.fc_dst.bias).view(n_dst, H, Fd)
        res = F.linear(feat[:n_dst], conv.res_fc.weight, conv.res_fc.bias).view(n_dst, H, Fd)
    ref = Restated(src, dst, n_src, n_dst, fs, fd, conv.attn, 0.3)
    out = conv(g, feat)
    assert tuple(out.shape) == (n_dst, H, Fd)
    assert torch.allclose(out.double(), ref.out + res.double(), rtol=1e-5, atol=1e-6)
    out2, att = conv(g, feat, get_attention=True)
    assert torch.allclose(out2, out, rtol=1e-5, atol=1e-6)
    assert torch.allclose(att.view(len(src), H).double(), ref.a, rtol=1e-5, atol=1e-6)                 # edge-id order
    if kind == "block":                                                                                 # the (feat_src, feat_dst) form
        assert torch.allclose(conv(g, (feat, feat[:n_dst])), out, rtol=1e-5, atol=1e-6)
    out.sum().backward()
    assert all(p.grad is not None and float(p.grad.abs().max()) > 0 for p in conv.parameters())
    import dgl.nn.pytorch as dglnn
    assert dglnn.GATv2Conv is mg.nn.GATv2Conv and dglnn.conv.GATv2Conv is mg.nn.GATv2Conv and config.GATV2_FUSED is True


# ----------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("H,Fd", [(1, 4), (3, 4), (8, 16), (4, 64)])
@pytest.mark.parametrize("kind", ["square", "block", "degrees", "hub"])
def test_fused_matches_the_restatement(kind, H, Fd):
    g, src, dst, n_src, n_dst = build(kind, DEV)
    fs, fd, attn, up = operands(n_src, n_dst, H, Fd, 3 * H + Fd)
    ref = Restated(src, dst, n_src, n_dst, fs, fd, attn, 0.2, up)
    ins = [t.to(DEV).requires_grad_(True) for t in (fs, fd, attn)]
    assert ops.gatv2_attention_fused(g, *ins)
    out = ops.gatv2_attention(g, *ins)
    assert tuple(out.shape) == (n_dst, H, Fd) and torch.all(out[torch.from_numpy(np.bincount(dst, minlength=n_dst) == 0)] == 0)
    check(out, torch.autograd.grad((out * up.to(DEV)).sum(), ins), ref)
    only_fs = fs.to(DEV).requires_grad_(True)              # d fs alone: t comes from the small pre-pass
    o = ops.gatv2_attention(g, only_fs, ins[1].detach(), ins[2].detach())
    check(o, torch.autograd.grad((o * up.to(DEV)).sum(), [only_fs]), ref, names=("dfs",))


@pytest.mark.gpu
@pytest.mark.parametrize("H,Fd", [(3, 4), (8, 16)])
def test_strided_and_shared_operands(H, Fd):
    g, src, dst, n, _ = build("hub", DEV)
    D = H * Fd
    torch.manual_seed(H)
    both = torch.randn(n, 2 * D, device=DEV).requires_grad_(True)      # fs and fd: the two column blocks of one projection
    attn, up = torch.randn(1, H, Fd, device=DEV), torch.randn(n, H, Fd, device=DEV)
    fs, fd = both[:, :D].view(n, H, Fd), both[:, D:].view(n, H, Fd)
    assert not fs.is_contiguous() and sparse.HipBackend._dot_operand(fd)[0] is fd and sparse.HipBackend._dot_operand(fd)[1] == 2 * D
    out = ops.gatv2_attention(g, fs, fd, attn)
    (out * up).sum().backward()
    dense = [t.detach().contiguous().requires_grad_(True) for t in (fs, fd)]
    out_d = ops.gatv2_attention(g, dense[0], dense[1], attn)
    (out_d * up).sum().backward()
    assert torch.equal(out, out_d) and torch.equal(both.grad, torch.cat([t.grad.view(n, D) for t in dense], 1))
    x = dense[0].detach().clone().requires_grad_(True)                 # fs is fd: share_weights on a square graph
    out_s = ops.gatv2_attention(g, x, x, attn)
    assert torch.equal(out_s, ops.gatv2_attention(g, x.detach().clone(), x.detach().clone(), attn))
    (out_s * up).sum().backward()
    ref = Restated(src, dst, n, n, x, x, attn, 0.2, up)
    check(out_s, [], ref)
    want = ref.dfs + ref.dfd
    err = float((x.grad.cpu().double() - want).abs().max())
    assert err <= RTOL * float(want.abs().max()), err


@pytest.mark.gpu
def test_reruns_are_bitwise_equal_on_the_hub_graph():
    g, src, dst, n, _ = build("hub", DEV)
    fs, fd, attn, up = (t.to(DEV) for t in operands(n, n, 8, 16, 5))
    runs = []
    for _ in range(2):
        ins = [t.clone().requires_grad_(True) for t in (fs, fd, attn)]
        out = ops.gatv2_attention(g, *ins)
        runs.append([out.detach()] + list(torch.autograd.grad((out * up).sum(), ins)))
    assert all(torch.equal(a_, b_) for a_, b_ in zip(*runs))
    # the kernels that ran (the name is kept per calling thread, autograd's backward runs on another: call the backend from this one)
    be, gi, last = sparse.backend_for(up), g._index, lambda: _lib.lib().mgx_last_spmm_kernel().decode()
    assert gi.csc().plan().num_slots > 0 and gi.csr().plan().num_slots > 0                   # rows split both ways
    o, st = be.gatv2_fwd(gi.csc(), fs, fd, attn.view(8, 16), 0.2)
    assert last() == "gatv2_fwd" and torch.equal(o, runs[0][0])
    got = be.gatv2_bwd(gi.csc(), gi.csr(), fs, fd, attn.view(8, 16), 0.2, o, up, st, False, True, True)
    assert last() == "gatv2_bwd_dst" and got[0] is None and torch.equal(got[1], runs[0][2]) and torch.equal(got[2], runs[0][3].view(8, 16))
    got = be.gatv2_bwd(gi.csc(), gi.csr(), fs, fd, attn.view(8, 16), 0.2, o, up, st, True, True, True)
    assert last() == "gatv2_bwd_src" and torch.equal(got[0], runs[0][1])


@pytest.mark.gpu
def test_uniform_attention_gives_the_exact_mean_of_the_neighbours():
    """fs[u,h,:] = (a, a, b, b) and attn[h,:] = 2^-h (1, -1, 1, -1) with slope 0.5: the pair (b, b) always cancels, and so does
    (a, a) + (c, c') wherever both sums are on one side of 0 -- a row's logits are all 2^-h (c - c') (destinations v % 3 == 0:
    c, c' = 64, 66), half that on the slope branch (v % 3 == 1: -64, -66), or 0 where c = c' = -3 meets a = 3 at s == 0 exactly
    and other sources on either side (v % 3 == 2).  Small integers: every sum is exact, so out is the correctly rounded mean."""
    g, src, dst, n, _ = build("degrees", DEV)
    H, Fd = 4, 8
    rng = np.random.default_rng(3)
    fs = torch.from_numpy(rng.integers(-8, 9, (n, H, Fd // 2)).astype(np.float32)).repeat_interleave(2, dim=2)
    fd = torch.from_numpy(rng.integers(-8, 9, (n, H, Fd // 2)).astype(np.float32)).repeat_interleave(2, dim=2)
    kind = torch.arange(n) % 3
    fd[:, :, 0] = torch.tensor([64., -64., -3.])[kind].view(n, 1)
    fd[:, :, 1] = torch.tensor([66., -66., -3.])[kind].view(n, 1)
    attn = (torch.tensor([1., -1.] * (Fd // 2)).view(1, 1, Fd) * 0.5 ** torch.arange(H).view(1, H, 1)).contiguous()
    ref = Restated(src, dst, n, n, fs, fd, attn, 0.5)
    d = torch.from_numpy(dst)
    want_z = (torch.tensor([-2., 1., 0.], dtype=torch.float64)[kind].view(n, 1) * 0.5 ** torch.arange(H).double())[d]
    assert torch.equal(ref.z, want_z)                                   # from the reference alone: the logits are as claimed
    assert bool((ref.s[kind[d] == 1][:, :, :2] < 0).all()) and bool((ref.s[kind[d] == 2] == 0).any())
    deg = torch.from_numpy(np.bincount(dst, minlength=n)).double().view(n, 1, 1)
    mean = (torch.zeros(n, H, Fd, dtype=torch.float64).index_add_(0, d, fs.double()[torch.from_numpy(src)]) / deg.clamp(min=1)).float()
    out = ops.gatv2_attention(g, fs.to(DEV), fd.to(DEV), attn.to(DEV), negative_slope=0.5)
    assert torch.equal(out.cpu(), mean)                                 # a lost or doubled edge moves an element by >= 1 / degree


@pytest.mark.gpu
def test_one_nan_in_fs_reaches_exactly_its_destinations():
    g, src, dst, n, _ = build("hub", DEV)
    H, Fd = 4, 16
    fs, fd, attn, _ = operands(n, n, H, Fd, 6)
    clean = ops.gatv2_attention(g, fs.to(DEV), fd.to(DEV), attn.to(DEV))
    assert not torch.isnan(clean).any()
    for u0, h0 in ((7, 2), (int(src[0]), 0)):                           # the hub source (its edges reach the hub row too), an ordinary one
        bad = fs.clone()
        bad[u0, h0, 5] = float("nan")
        got = ops.gatv2_attention(g, bad.to(DEV), fd.to(DEV), attn.to(DEV))
        hit = torch.zeros(n, H, dtype=torch.bool)
        hit[torch.from_numpy(np.unique(dst[src == u0])), h0] = True
        assert u0 != 7 or hit[11, h0]
        hit = hit.to(DEV)
        assert torch.equal(torch.isnan(got), hit.unsqueeze(-1).expand(n, H, Fd))
        assert torch.equal(got[~hit], clean[~hit])                      # bitwise


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["F=5", "int64", "config"])
def test_fallbacks_on_the_device(case, monkeypatch):
    H, Fd = (2, 5) if case == "F=5" else (8, 16)
    g, src, dst, n, _ = build("hub", DEV, idtype=torch.int64 if case == "int64" else torch.int32)
    if case == "config":
        monkeypatch.setattr(config, "GATV2_FUSED", False)
    fs, fd, attn, up = operands(n, n, H, Fd, 8)
    ins = [t.to(DEV).requires_grad_(True) for t in (fs, fd, attn)]
    assert not ops.gatv2_attention_fused(g, *ins)
    out = ops.gatv2_attention(g, *ins)
    check(out, torch.autograd.grad((out * up.to(DEV)).sum(), ins), Restated(src, dst, n, n, fs, fd, attn, 0.2, up))


@pytest.mark.gpu
def test_gatv2_model_fused_on_and_off_and_under_hip_graph_capture(monkeypatch):
    sys.path.insert(0, PKG)
    import full_graph
    from mi355x_graph.datasets import synthetic_edges
    from mi355x_graph.utils import GraphedStep
    n = 2708                                                            # the cora stand-in
    src, dst = synthetic_edges(n, 10556, 200, seed=5, symmetric=True)
    g = mg.graph((src, dst), num_nodes=n).add_self_loop().int().formats(["csr", "csc"]).to(DEV)
    gen = torch.Generator().manual_seed(0)
    x, y = torch.rand(n, 24, generator=gen).to(DEV), torch.randint(0, 7, (n,), generator=gen).to(DEV)
    idx = torch.nonzero(torch.rand(n, generator=gen) < 0.3).flatten().to(DEV)
    torch.manual_seed(3)
    model = full_graph.GATv2(g, 3, 24, 8, 7, [8, 8, 1], feat_drop=0.0).to(DEV).train()
    assert all(isinstance(layer, mg.nn.GATv2Conv) for layer in model.gat_layers)
    with torch.no_grad():
        h = model.gat_layers[0].fc_src(x).view(-1, 8, 8)
    assert ops.gatv2_attention_fused(g, h, h, model.gat_layers[0].attn)

    def step():
        model.zero_grad(set_to_none=True)
        loss = F.cross_entropy(model(x)[idx], y[idx])
        loss.backward()
        return float(loss.detach()), [p.grad.clone() for p in model.parameters()]

    loss_on, grads_on = step()
    assert _lib.lib().mgx_last_spmm_kernel().decode() == "gatv2_fwd"   # the output layer's forward, on this thread
    monkeypatch.setattr(config, "GATV2_FUSED", False)
    loss_off, grads_off = step()
    monkeypatch.setattr(config, "GATV2_FUSED", True)
    print("loss fused %r, composed %r" % (loss_on, loss_off))
    assert abs(loss_on - loss_off) <= RTOL * abs(loss_off)
    for (name, _), a_, b_ in zip(model.named_parameters(), grads_on, grads_off):
        err, top = float((a_ - b_).abs().max()), float(b_.abs().max())
        print("%s: max err %.3e, max |composed| %.3e" % (name, err, top))
        assert err <= RTOL * top, (name, err, top)
    # the package's capture (full_graph.py --hipgraph) on a copy whose parameters the default stream never touched; a step size of 0
    # leaves them alone, so every replay must give the eager loss of the original: the fused path reads nothing back to the host
    twin = full_graph.GATv2(g, 3, 24, 8, 7, [8, 8, 1], feat_drop=0.0).to(DEV).train()
    twin.load_state_dict(model.state_dict())
    graphed = GraphedStep(lambda: F.cross_entropy(twin(x)[idx], y[idx]), torch.optim.SGD(twin.parameters(), lr=0.0))
    for _ in range(3):
        loss = graphed()
        torch.cuda.synchronize()
        assert float(loss.detach()) == loss_on
