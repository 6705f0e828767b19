"""mgx_spmm_copy_u_strided_init: the accumulating copy_u sum whose initial value comes from a compact [R, D] matrix through a position
map, bit for bit (int32 views: the sign of zero counts) against the sequence it replaces on the same graph and plan --
`zeros.index_copy_(0, rows, d_self)` followed by spmm_copy_u_strided(accumulate=True) -- over a graph that exercises the lane-group
kernel, the wave-per-item kernel and the hub fix-up in one call; what the entry point refuses; and the layer that uses it
(ops.SageMeanCatHeadFn, config.SAGE_HEAD_INIT) against itself with the switch off, a second row list over the same buffer and a
captured step included.  Every map entry is -1 or a valid row of the compact matrix: the kernels do not check them."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dgl-0.5-benchmark_amd")
sys.path.insert(0, PKG)
import mi355x_graph as mg  # noqa: E402
from mi355x_graph import _lib, config, ops, sparse  # noqa: E402
from conftest import random_graph  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N, D = 131072, 64


def _be():
    return sparse.backend_for(torch.zeros(1, device=DEV))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _signed_zeros(t, gen, share=0.1):
    """`share` of the entries become -0.0f, as many +0.0f."""
    r = torch.rand(t.shape, device=t.device, generator=gen)
    t[r < share] = -0.0
    t[r > 1.0 - share] = 0.0
    return t


@pytest.fixture(scope="module")
def world():
    """N = 131 072 destination rows: most with 0 - 8 in-edges (0 included), 3 000 with 17 - 200, 200 with 300 - 3 000 (split at 256
    edges), about 1.2 M edges, sources anywhere.  The two-part plan's threshold of 100 k short items is met."""
    gen = torch.Generator(device=DEV).manual_seed(2024)
    deg = torch.randint(0, 9, (N,), device=DEV, generator=gen)
    special = torch.randperm(N - 1, device=DEV, generator=gen)[:3200]    # (never the last row: it stays a short one)
    mid, hubs = special[:3000], special[3000:]
    deg[mid] = torch.randint(17, 201, (3000,), device=DEV, generator=gen)
    deg[hubs] = torch.randint(300, 3001, (200,), device=DEV, generator=gen)
    deg[N - 1] = 3
    indptr = torch.zeros(N + 1, dtype=torch.int64, device=DEV)
    torch.cumsum(deg, 0, out=indptr[1:])
    nnz = int(indptr[-1])
    indices = torch.randint(0, N, (nnz,), device=DEV, generator=gen)
    empty = torch.nonzero(deg == 0).flatten()
    assert empty.numel() > 1000 and 900_000 < nnz < 1_500_000
    # one row of three edges whose sources will hold nothing but -0.0f
    quiet = int(torch.nonzero(deg == 3).flatten()[7])
    qsrc = torch.tensor([N - 5, N - 6, N - 7], device=DEV)
    lo, hi = int(indptr[quiet]), int(indptr[quiet + 1])
    indices[lo:hi] = qsrc
    csr = sparse.CsrView(N, N, indptr.to(torch.int32), indices.to(torch.int32), None)
    u = _signed_zeros(torch.randn(N, D, device=DEV, generator=gen), gen)
    u[qsrc] = -0.0
    plan, short = csr.spmm_plan_for(D)
    # the call below runs all three: short items on the lane-group kernel, the rest (rows above 16 edges, the 256-edge chunks of the
    # split rows) on the wave-per-item kernel, the split rows' totals in the fix-up
    assert short and plan is not None and plan.rest is not None and csr.tile_plan(D) is None
    assert plan.num_items >= 100_000 and plan.rest.num_items > 3000 and plan.rest.num_hubs == 200 and plan.rest.num_slots >= 400
    perm = torch.randperm(N, device=DEV, generator=gen)
    lists = {
        "empty": torch.zeros(0, dtype=torch.int64, device=DEV),
        "all": torch.arange(N, device=DEV),
        "8 percent": perm[:N * 8 // 100][perm[:N * 8 // 100] != quiet].contiguous(),
        "hub, no in-edges, last": torch.stack([hubs[0], empty[3], torch.tensor(N - 1, device=DEV), hubs[17], empty[0]]),
        "descending": torch.sort(perm[N // 2:N // 2 + 5000][perm[N // 2:N // 2 + 5000] != quiet], descending=True)[0].contiguous(),
    }
    return {"csr": csr, "u": u, "plan": plan, "lists": lists, "quiet": quiet, "gen": gen, "hubs": hubs, "empty": empty}


def _pos(rows, n=N):
    pos = torch.full((n,), -1, dtype=torch.int64, device=DEV)
    pos[rows] = torch.arange(rows.shape[0], dtype=torch.int64, device=DEV)
    return pos


def _today(be, csr, u, rows, d_self, out=None):
    """The sequence the entry point replaces, on the same graph and plan."""
    if out is None:
        out = torch.zeros((csr.num_rows, u.shape[1]), device=DEV)
    else:
        out.zero_()
    out.index_copy_(0, rows, d_self)
    be.spmm_copy_u_strided(csr, "sum", u, out, accumulate=True)
    return out


@pytest.mark.parametrize("name", ["empty", "all", "8 percent", "hub, no in-edges, last", "descending"])
def test_initial_value_from_a_compact_matrix_is_bitwise_the_accumulating_call(world, name):
    be, csr, u, rows = _be(), world["csr"], world["u"], world["lists"][name]
    gen = torch.Generator(device=DEV).manual_seed(len(name))
    d_self = _signed_zeros(torch.randn(rows.shape[0], D, device=DEV, generator=gen), gen)
    if rows.numel():
        d_self[0] = -0.0   # a whole row of -0.0f to start from
    want = _today(be, csr, u, rows, d_self)
    out = torch.full((N, D), float("nan"), device=DEV)   # write-only, every row written: no NaN may survive
    sparse.PROFILE = []
    try:
        got = be.spmm_copy_u_strided_init(csr, "sum", u, d_self, _pos(rows), out)
    finally:
        recs, sparse.PROFILE = sparse.PROFILE, None
    assert got is out
    # which kernels ran, as the library and its host layer record it
    assert _lib.lib().mgx_last_spmm_kernel() == b"rowgroup32"
    assert len(recs) == 1 and "spmm_rowgroup32_kernel" in recs[0]["variant"] and "spmm_rowwave32_kernel" in recs[0]["variant"]
    assert world["plan"].rest.num_hubs > 0
    diff = torch.nonzero((_bits(got) != _bits(want)).any(dim=1)).flatten()
    print("%s: %d rows listed, %d rows differ" % (name, rows.shape[0], diff.numel()))
    assert diff.numel() == 0, diff[:10].tolist()
    assert not bool(torch.isnan(got).any())
    if name != "all":   # the unlisted row whose three sources are all -0.0f: -0 + -0 + -0 added to +0.0f is +0.0f
        assert bool((_bits(got[world["quiet"]]) == 0).all())
        assert bool((_bits(u[csr.indices[csr.indptr[world["quiet"]]:csr.indptr[world["quiet"] + 1]].long()]) == -2 ** 31).all())


def test_row_strides_of_all_three_matrices(world):
    be, csr, u, rows = _be(), world["csr"], world["u"], world["lists"]["8 percent"]
    gen = torch.Generator(device=DEV).manual_seed(99)
    wide_init = _signed_zeros(torch.randn(rows.shape[0], 128, device=DEV, generator=gen), gen)
    d_self = wide_init[:, :D]                                   # row stride 128 floats
    wide_u = torch.full((N, 96), float("nan"), device=DEV)
    wide_u[:, 32:] = u
    wide_out = torch.full((N, 128), float("nan"), device=DEV)
    out = wide_out[:, :D]                                       # the left half of an [N, 128] matrix
    assert d_self.stride(0) == 128 and out.stride(0) == 128
    want = _today(be, csr, u, rows, d_self.contiguous())
    got = be.spmm_copy_u_strided_init(csr, "sum", wide_u[:, 32:], d_self, _pos(rows), out)
    assert got is out and torch.equal(_bits(got), _bits(want))
    assert bool(torch.isnan(wide_out[:, D:]).all())            # nothing written beside it


def test_refusals_leave_the_output_alone(world):
    """mean, a dst_scale, D = 62 and an int64 graph have no such kernel: MGX_ERR_UNSUPPORTED, seen as None, nothing written."""
    be, csr, u, rows = _be(), world["csr"], world["u"], world["lists"]["descending"]
    gen = torch.Generator(device=DEV).manual_seed(5)
    d_self = torch.randn(rows.shape[0], D, device=DEV, generator=gen)
    pos = _pos(rows)
    out = torch.full((N, D), 7.0, device=DEV)
    assert be.spmm_copy_u_strided_init(csr, "mean", u, d_self, pos, out) is None
    assert be.spmm_copy_u_strided_init(csr, "sum", u, d_self, pos, out, dst_scale=torch.ones(N, device=DEV)) is None
    out62 = torch.full((N, 62), 7.0, device=DEV)
    assert be.spmm_copy_u_strided_init(csr, "sum", u[:, :62].contiguous(), d_self[:, :62].contiguous(), pos, out62) is None
    assert be.spmm_copy_u_strided_init(csr.astype(torch.int64), "sum", u, d_self, pos, out) is None
    assert bool((out == 7.0).all()) and bool((out62 == 7.0).all())
    # the entry point itself, not the wrapper
    L = _lib.lib()
    import ctypes
    st = L.mgx_spmm_copy_u_strided_init(ctypes.byref(csr.c_struct()), None, _lib.REDUCE["mean"], u.data_ptr(), D, D, None, d_self.data_ptr(),
                                        rows.shape[0], D, pos.data_ptr(), out.data_ptr(), D, None, 0, None)
    assert st == _lib.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ---- the layer
NL, RL = 65536, 5000   # the layer's gate (ops._ROWS_GEMM_MIN rows)


@pytest.fixture(scope="module")
def layer_world():
    src, dst = random_graph(NL, NL, 10 * NL, seed=31, skew=True)
    g = mg.graph((torch.from_numpy(src), torch.from_numpy(dst)), num_nodes=NL).int().formats(["csr", "csc"]).to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(8)
    perm = torch.randperm(NL, device=DEV, generator=gen)
    w = {"g": g, "h": torch.randn(NL, 64, device=DEV, generator=gen),
         "params": [torch.randn(47, 64, device=DEV, generator=gen) * 0.1, torch.randn(47, 64, device=DEV, generator=gen) * 0.1,
                    torch.randn(47, device=DEV, generator=gen)],
         "rows": [perm[:RL].contiguous(), perm[RL - 100:2 * RL - 100].contiguous()],   # two lists that share 100 rows
         "dyr": torch.randn(RL, 47, device=DEV, generator=gen)}
    return w


def _layer_grads(w, cat, rows, monkeypatch, init):
    monkeypatch.setattr(config, "SAGE_HEAD_INIT", init)
    h = w["h"].clone().requires_grad_(True)
    ws, wn, b = [p.clone().requires_grad_(True) for p in w["params"]]
    y = ops.SageMeanCatHeadFn.apply(w["g"]._index, cat, h, ws, wn, b, rows)
    y.backward(w["dyr"])
    return [h.grad, ws.grad, wn.grad, b.grad]


def test_layer_gives_the_same_four_gradients_with_the_switch_on_and_off(layer_world, monkeypatch):
    w = layer_world
    calls = []
    real = sparse.HipBackend.spmm_copy_u_strided_init

    def spy(self, *a, **k):
        r = real(self, *a, **k)
        calls.append(r is not None)
        return r

    monkeypatch.setattr(sparse.HipBackend, "spmm_copy_u_strided_init", spy)
    cat_on, cat_off = ops.CatBuffer(NL, 64, DEV), ops.CatBuffer(NL, 64, DEV)
    for rows in w["rows"]:   # the second list over the same graph: the matrix kept for d neigh / deg holds the first list's rows
        off = _layer_grads(w, cat_off, rows, monkeypatch, False)
        assert calls == []
        on = _layer_grads(w, cat_on, rows, monkeypatch, True)
        assert calls == [True]
        calls.clear()
        for name, a_, b_ in zip(("d h", "d W_self", "d W_neigh", "d bias"), on, off):
            assert torch.equal(_bits(a_), _bits(b_)), (name, float((a_ - b_).abs().max()))
    # a list written in place between two steps is another list: the matrix kept for d neigh / deg is cleared, not trusted
    rows = w["rows"][0].clone()
    _layer_grads(w, cat_on, rows, monkeypatch, True)
    rows.copy_(w["rows"][1])
    rewritten = _layer_grads(w, cat_on, rows, monkeypatch, True)
    held = w["g"]._index.csr()._head_dn
    assert calls == [True, True] and held is not None and held[1] is rows
    assert all(torch.equal(_bits(a_), _bits(b_)) for a_, b_ in zip(rewritten, off))
    assert not any(t.data_ptr() == held[0].data_ptr() for t in rewritten)   # never handed out
    # an entry point that declines: the layer takes the sequence it had
    monkeypatch.setattr(sparse.HipBackend, "spmm_copy_u_strided_init", lambda self, *a, **k: None)
    declined = _layer_grads(w, cat_on, w["rows"][1], monkeypatch, True)
    assert all(torch.equal(_bits(a_), _bits(b_)) for a_, b_ in zip(declined, off))


def test_layer_in_a_captured_step(layer_world, monkeypatch):
    """The node inside utils.GraphedStep (forward, backward and an optimizer step that moves nothing): the replayed gradients are the
    eager ones with the switch off."""
    from mi355x_graph.utils import GraphedStep
    w = layer_world
    rows = w["rows"][0]
    want = _layer_grads(w, ops.CatBuffer(NL, 64, DEV), rows, monkeypatch, False)
    monkeypatch.setattr(config, "SAGE_HEAD_INIT", True)
    leaves = [torch.nn.Parameter(t.clone()) for t in [w["h"]] + w["params"]]
    cat = ops.CatBuffer(NL, 64, DEV)

    def loss_fn():
        y = ops.SageMeanCatHeadFn.apply(w["g"]._index, cat, leaves[0], leaves[1], leaves[2], leaves[3], rows)
        return (y * w["dyr"]).sum()

    step = GraphedStep(loss_fn, torch.optim.Adam(leaves, lr=0.0, capturable=True), warmup=2)
    for _ in range(2):
        step()
    torch.cuda.synchronize()
    for name, p, b_ in zip(("d h", "d W_self", "d W_neigh", "d bias"), leaves, want):
        assert torch.equal(_bits(p.grad), _bits(b_)), (name, float((p.grad - b_).abs().max()))
