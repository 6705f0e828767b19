"""The last SAGE layer's dense work on the loss rows only: the row-list operands of the two dense kernels (mgx_rows_gemm_rows in
csrc/rowsgemm.hip, mgx_xty_rows / mgx_xty_colsum_rows in csrc/xty.hip) bit for bit against the existing kernels on a gathered copy
and against fp64, mgx_xty_colsum_pos bit for bit against the product with the scattered operand, the wrappers' fallback, and the layer that uses them (ops.SageMeanCatHeadFn, config.SAGE_HEAD_ROWS) against the
layer over all rows followed by the selection.  Every index in every list is valid: the kernels do not check them."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dgl-0.5-benchmark_amd")
sys.path.insert(0, PKG)
import mi355x_graph as mg  # noqa: E402
from mi355x_graph import ops, sparse  # noqa: E402
from conftest import random_graph  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _be():
    return sparse.backend_for(torch.zeros(1, device=DEV))


def _subset(n, r, gen):
    """r distinct rows of range(n) in random order, 0 and n - 1 among them (when r >= 2)."""
    perm = torch.randperm(n - 2, device=DEV, generator=gen)[:max(r - 2, 0)] + 1
    ends = torch.tensor([n - 1, 0][:min(r, 2)], device=DEV, dtype=torch.int64)
    rows = torch.cat([perm, ends])
    return rows[torch.randperm(rows.shape[0], device=DEV, generator=gen)].contiguous()


# ---- 1. rows_gemm_rows, gather
@pytest.mark.parametrize("R", [777, 1, 16])
@pytest.mark.parametrize("M", [47, 64])   # 47: element stores (column guard); 64: float4 stores
def test_rows_gemm_gathers_listed_rows_bitwise(R, M):
    gen = torch.Generator(device=DEV).manual_seed(1000 * R + M)
    be = _be()
    a = torch.randn(5000, 128, device=DEV, generator=gen)
    w = torch.randn(M, 128, device=DEV, generator=gen)
    bias = torch.randn(M, device=DEV, generator=gen)
    rows = _subset(5000, R, gen)
    assert rows.unique().numel() == R and int(rows.max()) < 5000 and int(rows.min()) >= 0
    got = be._rows_gemm_lists(a, w, True, bias, None, 0, 0, rows, None, None)   # the kernel itself: no fallback
    assert got is not None and got.shape == (R, M)
    gathered = a.index_select(0, rows)
    want = be.rows_gemm(gathered, w, b_transposed=True, bias=bias)
    assert torch.equal(got, want)
    assert torch.equal(be.rows_gemm(a, w, b_transposed=True, bias=bias, rows=rows), want)
    ref = gathered.double() @ w.double().t() + bias.double()
    bound = gathered.double().abs() @ w.double().abs().t() + bias.double().abs()
    err = (got.double() - ref).abs()
    assert bool((err <= 1e-5 * bound + 1e-30).all()), float((err / (bound + 1e-30)).max())


# ---- 2. rows_gemm_rows, scatter
@pytest.mark.parametrize("shift", [0, 1])   # 0: contiguous and aligned (the staged span); 1: off by one float (plain dword loads)
def test_rows_gemm_scatters_the_second_half_and_nothing_else(shift):
    gen = torch.Generator(device=DEV).manual_seed(50 + shift)
    be = _be()
    R, K, M = 777, 47, 128
    flat = torch.randn(R * K + 4, device=DEV, generator=gen)
    dyr = flat[shift:shift + R * K].view(R, K)
    assert dyr.data_ptr() % 16 == 4 * shift
    wcat = torch.randn(K, M, device=DEV, generator=gen)
    rs = torch.rand(R, device=DEV, generator=gen) + 0.25
    rows = _subset(5000, R, gen)
    left0, right0 = be.rows_gemm(dyr, wcat, row_scale=rs, scale_from=64, split_col=64)
    c2 = torch.full((5000, 64), 7.0, device=DEV)
    got = be._rows_gemm_lists(dyr, wcat, False, None, rs, 64, 64, None, rows, c2)   # the kernel itself
    assert got is not None and got[1] is c2
    assert torch.equal(got[0], left0)
    assert torch.equal(c2.index_select(0, rows), right0)
    other = torch.ones(5000, dtype=torch.bool, device=DEV)
    other[rows] = False
    assert int(other.sum()) == 5000 - R and bool((c2[other] == 7.0).all())
    c2b = torch.full((5000, 64), 7.0, device=DEV)
    l2, r2 = be.rows_gemm(dyr, wcat, row_scale=rs, scale_from=64, split_col=64, scatter_rows=rows, out2=c2b)
    assert r2 is c2b and torch.equal(l2, left0) and torch.equal(c2b, c2)


# ---- 3. xty_colsum_rows
@pytest.mark.parametrize("R", [5000, 17])   # 5000: 256 waves x 16 rows a trip -- some waves make two trips; 17: most make none
@pytest.mark.parametrize("cols", [(0, 128), (0, 64), (64, 128)])   # the whole [h | neigh] buffer, its left half, its right half
def test_xty_reads_listed_rows_bitwise(R, cols):
    gen = torch.Generator(device=DEV).manual_seed(R + cols[0] + cols[1])
    be = _be()
    buf = torch.randn(20000, 128, device=DEV, generator=gen)
    b = buf[:, cols[0]:cols[1]]                  # the buffer's row stride
    a = torch.randn(R, 47, device=DEV, generator=gen)
    rows = _subset(20000, R, gen)
    got = be._xty_rows(a, b, rows, True)         # the kernel itself
    assert got is not None
    gathered = b.index_select(0, rows)
    want, want_s = be.xty(a, gathered, colsum=True)
    assert torch.equal(got[0], want) and torch.equal(got[1], want_s)
    plain = be._xty_rows(a, b, rows, False)
    assert plain is not None and torch.equal(plain, be.xty(a, gathered))
    pub, pub_s = be.xty(a, b, colsum=True, rows=rows)
    assert torch.equal(pub, want) and torch.equal(pub_s, want_s)
    ref = a.double().t() @ gathered.double()
    scale = float((a.double().abs().t() @ gathered.double().abs()).max())
    assert float((got[0].double() - ref).abs().max()) <= 1e-5 * max(scale, 1e-30)
    assert bool(((got[1].double() - a.double().sum(0)).abs() <= 1e-5 * a.double().abs().sum(0) + 1e-30).all())


# ---- 3b. xty over all rows of b for an a that exists on the listed rows only: the bits of the product with the scattered a
@pytest.mark.parametrize("R", [5600, 17, 1])
@pytest.mark.parametrize("cols", [(0, 128), (64, 128)])
def test_xty_with_a_position_map_is_bitwise_the_product_with_the_scattered_operand(R, cols):
    gen = torch.Generator(device=DEV).manual_seed(7 * R + cols[0])
    be = _be()
    n = 70001                                    # 320 waves x 16 rows a trip: every wave makes 13 or 14 trips, the last tile is ragged
    buf = torch.randn(n, 128, device=DEV, generator=gen)
    b = buf[:, cols[0]:cols[1]]
    a = torch.randn(R, 47, device=DEV, generator=gen)
    rows = _subset(n, R, gen)
    pos = torch.full((n,), -1, dtype=torch.int64, device=DEV)
    pos[rows] = torch.arange(R, device=DEV)
    scattered = torch.zeros(n, 47, device=DEV).index_copy_(0, rows, a)
    want, want_s = be.xty(scattered, b, colsum=True)
    got = be.xty_pos(a, pos, b, colsum=True)     # the kernel itself
    assert got is not None and torch.equal(got[0], want) and torch.equal(got[1], want_s)
    plain = be.xty_pos(a, pos, b)
    assert plain is not None and torch.equal(plain, be.xty(scattered, b))
    ref = scattered.double().t() @ b.double()
    scale = float((scattered.double().abs().t() @ b.double().abs()).max())
    assert float((got[0].double() - ref).abs().max()) <= 1e-5 * max(scale, 1e-30)
    assert bool(((got[1].double() - a.double().sum(0)).abs() <= 1e-5 * a.double().abs().sum(0) + 1e-30).all())
    assert be.xty_pos(a, pos, torch.randn(n, 96, device=DEV, generator=gen)) is None   # no kernel: the caller scatters


# ---- 4. fallback
def test_shapes_without_a_row_list_kernel_take_the_fallback_with_the_same_numbers():
    gen = torch.Generator(device=DEV).manual_seed(4)
    be = _be()
    rows = _subset(5000, 777, gen)
    # K = 96: neither row-list kernel is built
    b96 = torch.randn(5000, 96, device=DEV, generator=gen)
    a = torch.randn(777, 47, device=DEV, generator=gen)
    assert be._xty_rows(a, b96, rows, True) is None
    got, got_s = be.xty(a, b96, colsum=True, rows=rows)
    want, want_s = be.xty(a, b96.index_select(0, rows), colsum=True)
    assert torch.equal(got, want) and torch.equal(got_s, want_s)
    w96 = torch.randn(47, 96, device=DEV, generator=gen)
    bias = torch.randn(47, device=DEV, generator=gen)
    assert be._rows_gemm_lists(b96, w96, True, bias, None, 0, 0, rows, None, None) is None
    got = be.rows_gemm(b96, w96, b_transposed=True, bias=bias, rows=rows)
    want = be.rows_gemm(b96.index_select(0, rows), w96, b_transposed=True, bias=bias)
    assert (got is None and want is None) or torch.equal(got, want)   # (mgx_rows_gemm has no K = 96 kernel either: both None)
    # K = 64: mgx_rows_gemm has the kernel, the row-list entry point does not -- gather (scatter) around the plain call
    a64 = torch.randn(5000, 64, device=DEV, generator=gen)
    w64 = torch.randn(64, 128, device=DEV, generator=gen)
    assert be._rows_gemm_lists(a64, w64, False, None, None, 0, 0, rows, None, None) is None
    got = be.rows_gemm(a64, w64, rows=rows)
    assert got is not None and torch.equal(got, be.rows_gemm(a64.index_select(0, rows), w64))
    d64 = torch.randn(777, 64, device=DEV, generator=gen)
    rs = torch.rand(777, device=DEV, generator=gen) + 0.25
    c2 = torch.full((5000, 64), 7.0, device=DEV)
    assert be._rows_gemm_lists(d64, w64, False, None, rs, 64, 64, None, rows, c2) is None and bool((c2 == 7.0).all())
    left, out2 = be.rows_gemm(d64, w64, row_scale=rs, scale_from=64, split_col=64, scatter_rows=rows, out2=c2)
    left0, right0 = be.rows_gemm(d64, w64, row_scale=rs, scale_from=64, split_col=64)
    assert out2 is c2 and torch.equal(left, left0) and torch.equal(c2.index_select(0, rows), right0)
    other = torch.ones(5000, dtype=torch.bool, device=DEV)
    other[rows] = False
    assert bool((c2[other] == 7.0).all())


# ---- 5 - 7. the model
N = 70000
LONELY = 12345   # a node whose in-edges are removed


@pytest.fixture(scope="module")
def world():
    import full_graph
    src, dst = random_graph(N, N, 14 * N, seed=12, skew=True)
    keep = dst != LONELY
    src, dst = src[keep], dst[keep]
    g = mg.graph((torch.from_numpy(src), torch.from_numpy(dst)), num_nodes=N).int().formats(["csr", "csc"]).to(DEV)
    torch.manual_seed(0)
    x = torch.randn(N, 100, device=DEV)
    y = torch.randint(0, 47, (N,), device=DEV)
    idx = torch.nonzero(torch.rand(N, device=DEV) < 0.08).flatten()   # 8 % of the nodes, from a mask
    assert not bool((dst == LONELY).any()) and bool((src == LONELY).any())
    return {"full_graph": full_graph, "g": g, "x": x, "y": y, "idx": idx, "runs": {}}


def _train(world, monkeypatch, idx, head_rows, sparse_last="0", steps=2):
    """`steps` training steps from the same seeds: [(loss, gradients, node name, aggregation records)]."""
    monkeypatch.setenv("MGX_SAGE_HEAD_ROWS", head_rows)
    monkeypatch.setenv("MGX_SAGE_SPARSE_LAST", sparse_last)
    torch.manual_seed(77)
    ops.ReluDropout._calls = 0
    m = world["full_graph"].GraphSAGE(100, 64, 47, 3, 0.5).to(DEV)
    m.rows_are_distinct = True
    m.train()
    out = []
    for _ in range(steps):
        m.zero_grad()
        sparse.PROFILE = []
        try:
            logp = m(world["g"], world["x"], rows=idx)
            name = type(logp.grad_fn.next_functions[0][0]).__name__
            loss = ops.nll_sum(logp, world["y"][idx]) / max(int(idx.shape[0]), 1)
            loss.backward()
        finally:
            recs, sparse.PROFILE = sparse.PROFILE, None
        out.append((float(loss.detach()), [p.grad.clone() for p in m.parameters()], name, recs))
    return out


def _reference(world, monkeypatch, key, idx):
    """The layer over all rows followed by the selection (MGX_SAGE_HEAD_ROWS=0): computed once per row list, never changed."""
    if key not in world["runs"]:
        world["runs"][key] = _train(world, monkeypatch, idx, "0")
    return world["runs"][key]


def _same_training(run, ref):
    for (l1, g1, _, _), (l2, g2, _, _) in zip(run, ref):
        print("loss %.9g against %.9g" % (l1, l2))
        assert abs(l1 - l2) <= 1e-5 * abs(l2)
        for a_, b_ in zip(g1, g2):
            print("  gradient: max difference %.3g, max %.3g" % (float((a_ - b_).abs().max()), float(b_.abs().max())))
            assert float((a_ - b_).abs().max()) < 2e-4 * float(b_.abs().max()) + 1e-7


def test_head_node_gives_the_gradients_of_the_layer_over_all_rows_bit_for_bit(world):
    """Rounding differences in the last place grow into different training runs under Adam once the gradients are small, so the
    backward of the node forms every sum in the order the layer over all rows followed by the selection forms it."""
    g, idx = world["g"], world["idx"]
    gen = torch.Generator(device=DEV).manual_seed(21)
    h0 = torch.randn(N, 64, device=DEV, generator=gen)
    params = [torch.randn(47, 64, device=DEV, generator=gen) * 0.1, torch.randn(47, 64, device=DEV, generator=gen) * 0.1,
              torch.randn(47, device=DEV, generator=gen)]
    dyr = torch.randn(idx.shape[0], 47, device=DEV, generator=gen)
    legs = []
    for head in (False, True):
        h = h0.clone().requires_grad_(True)
        ws, wn, b = [p.clone().requires_grad_(True) for p in params]
        cat = ops.CatBuffer(N, 64, DEV)
        if head:
            y = ops.SageMeanCatHeadFn.apply(g._index, cat, h, ws, wn, b, idx)
        else:
            y = ops.select_distinct_rows(ops.SageMeanCatFn.apply(g._index, cat, h, ws, wn, b), idx)
        y.backward(dyr)
        legs.append((y.detach(), [h.grad, ws.grad, wn.grad, b.grad]))
    (y0, g0), (y1, g1) = legs
    print("forward bitwise equal to the library GEMM's: %s (max difference %.3g)" % (torch.equal(y0, y1), float((y0 - y1).abs().max())))
    assert float((y0 - y1).abs().max()) <= 1e-5 * float(y0.abs().max())
    for name, a_, b_ in zip(("d h", "d W_self", "d W_neigh", "d bias"), g1, g0):
        assert torch.equal(a_, b_), (name, float((a_ - b_).abs().max()))


def test_model_with_the_head_on_the_loss_rows_trains_the_same(world, monkeypatch):
    ref = _reference(world, monkeypatch, "idx", world["idx"])
    run = _train(world, monkeypatch, world["idx"], "1")
    _same_training(run, ref)
    assert all(name == "SageMeanCatHeadFnBackward" for _, _, name, _ in run)
    assert all("Head" not in name and "SageMeanCatRowsFn" not in name for _, _, name, _ in ref)
    for leg in (run, ref):   # five aggregations over every edge either way
        for _, _, _, recs in leg:
            assert sorted(r["out_len"] for r in recs) == [64, 64, 64, 64, 100]
            assert not any("row-sparse" in str(r.get("variant", "")) for r in recs)
    # the same launches, the accumulate flag included: the last layer's reversed aggregation accumulates into d self in both legs
    # (it starts a row's sum from the value it accumulates into; a plain aggregation + add would give other bits)
    flags = [[sorted((r["out_len"], bool(r.get("accumulate"))) for r in recs) for _, _, _, recs in leg] for leg in (run, ref)]
    assert flags[0] == flags[1] and all((64, True) in f for f in flags[0])
    again = _train(world, monkeypatch, world["idx"], "1")   # no atomics on shared addresses, fixed orders: the same bits
    for (l1, g1, _, _), (l2, g2, _, _) in zip(run, again):
        assert l1 == l2 and all(torch.equal(a_, b_) for a_, b_ in zip(g1, g2))


def test_opt_in_sparse_last_layer_shares_the_row_list_backward(world, monkeypatch):
    ref = _reference(world, monkeypatch, "idx", world["idx"])
    run = _train(world, monkeypatch, world["idx"], "1", sparse_last="1")
    _same_training(run, ref)
    assert all("SageMeanCatRowsFn" in name for _, _, name, _ in run)
    assert all(any(r.get("variant") == "row-sparse" for r in recs) for _, _, _, recs in run)   # its aggregation alone differs
    run0 = _train(world, monkeypatch, world["idx"], "0", sparse_last="1")                      # that switch wins over the other
    assert all("SageMeanCatRowsFn" in name for _, _, name, _ in run0)


@pytest.mark.parametrize("case", ["empty", "all", "ends_and_lonely"])
def test_edges_of_the_row_list_contract(world, monkeypatch, case):
    idx = {"empty": torch.zeros(0, dtype=torch.int64, device=DEV),
           "all": torch.arange(N, device=DEV),
           "ends_and_lonely": torch.tensor([0, LONELY, N - 1], device=DEV)}[case]
    ref = _reference(world, monkeypatch, case, idx)
    run = _train(world, monkeypatch, idx, "1")
    assert all(name == "SageMeanCatHeadFnBackward" for _, _, name, _ in run)
    _same_training(run, ref)
    if case == "empty":
        assert all(l == 0.0 and all(float(g_.abs().max()) == 0.0 for g_ in gs) for l, gs, _, _ in run)


def test_step_with_the_head_on_the_loss_rows_captures_into_a_graph(world, monkeypatch):
    """utils.GraphedStep replays the step; an eager twin that takes the captured forms from the same position of the dropout
    counter gives the same loss."""
    from mi355x_graph.utils import GraphedStep
    monkeypatch.setenv("MGX_SAGE_HEAD_ROWS", "1")
    monkeypatch.setenv("MGX_SAGE_SPARSE_LAST", "0")
    g, x, y, idx = world["g"], world["x"], world["y"], world["idx"]
    torch.manual_seed(5)
    model = world["full_graph"].GraphSAGE(100, 64, 47, 3, 0.5).to(DEV)
    twin = world["full_graph"].GraphSAGE(100, 64, 47, 3, 0.5).to(DEV)
    twin.load_state_dict(model.state_dict())
    names = []

    def loss_of(m):
        logp = m(g, x, rows=idx)
        names.append(type(logp.grad_fn.next_functions[0][0]).__name__)
        return ops.nll_sum(logp, y[idx]) / idx.shape[0]

    for m in (model, twin):
        m.rows_are_distinct = True
        m.train()
    ctr = ops._capture_counter(x.device)
    start = ctr.clone()
    warm = 2
    step = GraphedStep(lambda: loss_of(model), torch.optim.Adam(model.parameters(), lr=0.01, capturable=True), warmup=warm)
    loss_g = float(step().detach())
    assert set(names) == {"SageMeanCatHeadFnBackward"}
    ctr.copy_(start)
    opt = torch.optim.Adam(twin.parameters(), lr=0.01, capturable=True)
    with ops.warming_up_for_capture():
        for _ in range(warm + 1):
            opt.zero_grad(set_to_none=True)
            loss_e = loss_of(twin)
            loss_e.backward()
            opt.step()
    loss_e = float(loss_e.detach())
    print("replayed %.9g, eager %.9g" % (loss_g, loss_e))
    assert abs(loss_g - loss_e) <= 1e-6 * abs(loss_e)
